"""fp64 comparator of the SFRS region head (EmbedRegionNet._compute_region_sim, ibl/models/netvlad.py:123-186),
composed from pieces the oracle already has: oracle.descriptor.netvlad on the four quarter sub-maps and
normalize_vlad; the region sums and the dots are written here.  tests/test_region_golden_cpu.py ties it to vectors
the reference itself produced; the GPU tests use it at sizes that have no fixture.  TEST INFRASTRUCTURE ONLY."""
import torch

from oracle import descriptor as od

# regions in the reference's order: whole image, top / bottom / left / right halves, the four quarters
# (q0 top-left, q1 top-right, q2 bottom-left, q3 bottom-right)
REGIONS = ((0, 1, 2, 3), (0, 1), (2, 3), (0, 2), (1, 3), (0,), (1,), (2,), (3,))


def quarters(feat_nchw: torch.Tensor):
    """[N][C][h][w] -> the four [N][C][h/2][w/2] blocks; an odd map side is rejected (the reference's view raises)."""
    h, w = int(feat_nchw.shape[2]), int(feat_nchw.shape[3])
    if h % 2 or w % 2:
        raise ValueError(f"region head: the conv5 map is {h} x {w}, both sides must be even")
    hh, hw = h // 2, w // 2
    return [feat_nchw[:, :, r * hh:(r + 1) * hh, c * hw:(c + 1) * hw] for r in (0, 1) for c in (0, 1)]


def region_vectors(feat_nchw: torch.Tensor, conv_weight: torch.Tensor, centroids: torch.Tensor,
                   normalize_input: bool = True) -> torch.Tensor:
    """[N][C][h][w] map (any float dtype) -> [N][9][K*C] fp64 unit vectors."""
    f = feat_nchw.double()
    q = [od.netvlad(b.contiguous(), conv_weight.double(), centroids.double(), normalize_input) for b in quarters(f)]
    out = []
    for members in REGIONS:
        raw = q[members[0]]
        for m in members[1:]:
            raw = raw + q[m]
        out.append(od.normalize_vlad(raw))
    return torch.stack(out, dim=1)


def region_scores(vec: torch.Tensor, tuple_size: int) -> torch.Tensor:
    """[T*(1+n)][9][L] tuple-major (anchor first) -> score [T][n][9][9], score[t, j, a, b] = <A[t, a], B[t, j, b]>."""
    v = vec.double().view(tuple_size, -1, vec.shape[1], vec.shape[2])
    return torch.einsum("tal,tjbl->tjab", v[:, 0], v[:, 1:])
