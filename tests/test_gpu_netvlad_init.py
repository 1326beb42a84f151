"""NetVLAD initialisation on the device (csrc/netvlad_init.hip, openibl_amd.cluster, NetVLAD._init_params) against
results the REFERENCE ITSELF produced (tests/golden/netvlad_init.npz: NetVLAD._init_params of ibl/models/netvlad.py
on seeded inputs) and against torch / float64 numpy evaluations of the same steps.

Bounds: sampled descriptors per-row rel-L2 <= 1e-6 (the project's fp32 stage bound); alpha within
1e-4 relative and conv_weight within 1e-4 rel-L2 of the reference's (north_star's bar); centroids bit-equal; gap[]
within 1e-5 absolute of a float64 evaluation (fp32 dot products of unit vectors over C <= 512 sit near 1e-7).
Observed on the MI355X: sampled rows 9e-8 .. 2.3e-7; alpha 0 .. 9.2e-8; conv_weight 0 .. 9.4e-8;
gap[] 1.2e-7 .. 4.0e-7."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import assert_rel_l2, load_golden
from openibl_amd import cluster, models, ops, synth

pytestmark = pytest.mark.gpu

TOL_ROW = 1e-6
TOL_ALPHA = 1e-4
TOL_WEIGHT = 1e-4
TOL_GAP = 1e-5


@pytest.fixture(scope="module")
def golden():
    g = load_golden("netvlad_init")
    return {name: {k: g[f"{name}_{k}"] for k in ("clsts", "traindescs", "alpha", "centroids", "conv_weight")}
            for name in g["cases"].tolist()}


def _gap64(clsts, descs):
    """float64: (clsts_assign, gap[], top-2 cluster indices per descriptor)."""
    c, d = np.asarray(clsts, np.float64), np.asarray(descs, np.float64)
    ca = c / np.linalg.norm(c, axis=1, keepdims=True)
    dots = ca @ d.T                                   # [K][n]
    order = np.argsort(-dots, axis=0, kind="stable")
    top = np.take_along_axis(dots, order[:2], axis=0)
    return ca, top[0] - top[1], order[:2]


# ---- 1. ops.local_descriptors ---------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("shape", [(3, 4, 6, 64), (2, 30, 40, 512)], ids=["3x4x6x64", "2x30x40x512"])
def test_local_descriptors_match_normalize_then_gather(dev, shape, dtype):
    N, h, w, C = shape
    P = h * w
    g = torch.Generator().manual_seed(N * P + C)
    feat = (torch.randn(shape, generator=g) * 3.0).to(dtype)
    feat.view(N, P, C)[1, 7] = 0                      # an all-zero pixel: zeros under the 1e-12 clamp
    want_map = F.normalize(feat.float().view(N, P, C), p=2, dim=2)      # on the upcast map, on the CPU
    rng = np.random.RandomState(5)
    sampled = cluster.sample_positions(N, P, 5, rng)
    sampled[1, 2] = 7
    for name, pos in (("S=5", sampled), ("S=P", cluster.sample_positions(N, P, P, rng))):
        got = ops.local_descriptors(feat.to(dev), pos)
        S = pos.shape[1]
        assert tuple(got.shape) == (N * S, C) and got.dtype == torch.float32 and got.is_cuda
        want = torch.stack([want_map[n, int(p)] for n in range(N) for p in pos[n]])
        got = got.cpu()
        zero = want.norm(dim=1) == 0
        assert int(zero.sum()) >= 1 and bool((got[zero] == 0).all())
        rel = ((got.double() - want.double()).norm(dim=1)[~zero] / want.double().norm(dim=1)[~zero]).max()
        print(f"local_descriptors {tuple(shape)} {dtype} {name}: worst row rel-L2 {float(rel):.3e}")
        assert float(rel) <= TOL_ROW
        # the [N][P][C] form and device-resident positions are the same call
        again = ops.local_descriptors(feat.view(N, P, C).to(dev), torch.from_numpy(pos).to(dev))
        assert torch.equal(again.cpu(), got)


def test_local_descriptors_refuse_positions_outside_the_map(dev, monkeypatch):
    feat = torch.randn((3, 4, 6, 64), device=dev)
    good = ops.local_descriptors(feat, np.zeros((3, 5), np.int64))

    def no_library():
        raise AssertionError("the library was reached: something could have been launched")

    with monkeypatch.context() as m:
        m.setattr(ops._lib, "load", no_library)                 # refused before the C entry is even looked up
        for bad in (24, -1):
            pos = np.zeros((3, 5), np.int64)
            pos[2, 4] = bad
            with pytest.raises(ValueError, match=r"\[0, 24\)"):
                ops.local_descriptors(feat, pos)
            with pytest.raises(ValueError, match=r"\[0, 24\)"):
                ops.local_descriptors(feat, torch.from_numpy(pos).to(dev))
    assert torch.equal(ops.local_descriptors(feat, np.zeros((3, 5), np.int64)), good)
    with pytest.raises(ValueError):
        ops.local_descriptors(feat, np.zeros((2, 5), np.int64))                 # one row per image
    with pytest.raises(ValueError):
        ops.local_descriptors(feat, np.zeros((3, 5), np.float32))


# ---- 2. ops.assign_gap and netvlad_init -----------------------------------------------------------------------
@pytest.mark.parametrize("case", ["k64", "k20", "k2_n1", "k256"])
def test_assign_gap_and_netvlad_init_on_the_reference_cases(dev, golden, case):
    g = golden[case]
    clsts, descs = torch.from_numpy(g["clsts"]).to(dev), torch.from_numpy(g["traindescs"]).to(dev)
    ca, gap, mean_gap = ops.assign_gap(descs, clsts)
    ca64, gap64, _ = _gap64(g["clsts"], g["traindescs"])
    assert tuple(ca.shape) == tuple(clsts.shape) and tuple(gap.shape) == (descs.shape[0],) and isinstance(mean_gap, float)
    assert_rel_l2(f"{case} clsts_assign", ca.cpu(), ca64, 1e-6)
    worst = float(np.abs(gap.cpu().numpy().astype(np.float64) - gap64).max())
    print(f"{case}: gap[] max abs error against float64 {worst:.3e} (mean gap {mean_gap:.6f})")
    assert worst <= TOL_GAP
    assert abs(mean_gap - float(gap.cpu().double().mean())) <= 1e-12
    alpha, centroids, weight = cluster.netvlad_init(g["clsts"], g["traindescs"])
    da = abs(alpha - float(g["alpha"])) / float(g["alpha"])
    print(f"{case}: alpha {alpha:.6f}, reference {float(g['alpha']):.6f}, relative {da:.3e}")
    assert isinstance(alpha, float) and da <= TOL_ALPHA
    assert tuple(weight.shape) == g["conv_weight"].shape and weight.is_cuda
    assert_rel_l2(f"{case} conv_weight", weight.cpu(), g["conv_weight"], TOL_WEIGHT)
    assert np.array_equal(centroids.cpu().numpy(), g["clsts"]) and np.array_equal(g["centroids"], g["clsts"])


@pytest.mark.parametrize("K", [64, 130])
def test_identical_centres_give_a_gap_of_exactly_zero(dev, golden, K):
    """Centres j and dup are the same row (in the same lane pass, and — K = 130 — two passes apart in one lane and in
    different lanes): wherever they are the top pair the gap is 0.0, not a rounding residue."""
    g = golden["k64"]
    rng = np.random.RandomState(K)
    descs = g["traindescs"]
    clsts = np.concatenate([g["clsts"], rng.randn(K - 64, 128).astype(np.float32) * 0.1])
    pairs = ((3, 40),) if K == 64 else ((1, 129), (5, 70))
    for j, dup in pairs:
        clsts[dup] = clsts[j]
    _, gap, _ = ops.assign_gap(torch.from_numpy(descs).to(dev), torch.from_numpy(clsts).to(dev))
    gap = gap.cpu().numpy()
    _, gap64, top = _gap64(clsts, descs)
    dup_top = np.zeros(len(gap), bool)
    for j, dup in pairs:
        dup_top |= np.isin(top[0], (j, dup)) & np.isin(top[1], (j, dup))
    print(f"K = {K}: {int(dup_top.sum())} descriptors have the duplicated centres on top")
    assert dup_top.sum() >= len(pairs)
    assert (gap[dup_top] == 0.0).all()
    assert np.abs(gap - gap64).max() <= TOL_GAP and (gap >= 0).all()


# ---- 3. determinism -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [257, 4099])
def test_assign_gap_is_bit_reproducible(dev, n):
    g = torch.Generator().manual_seed(n)
    descs = F.normalize(torch.randn((n, 512), generator=g), dim=1).to(dev)
    clsts = (torch.randn((64, 512), generator=g) * 0.2).to(dev)
    ca1, gap1, mean1 = ops.assign_gap(descs, clsts)
    ca1, gap1 = ca1.clone(), gap1.clone()
    ops.assign_gap(descs[:33].contiguous(), clsts)               # another launch geometry in between
    ca2, gap2, mean2 = ops.assign_gap(descs, clsts)
    assert mean1 == mean2 and torch.equal(ca1, ca2) and torch.equal(gap1, gap2)
    # a descriptor's gap does not depend on the rows around it (which wave and workgroup it lands in)
    _, gap3, _ = ops.assign_gap(descs[5:].contiguous(), clsts)
    assert torch.equal(gap3, gap1[5:])
    _, gap64, _ = _gap64(clsts.cpu().numpy(), descs.cpu().numpy())
    assert np.abs(gap1.cpu().numpy() - gap64).max() <= TOL_GAP


# ---- 4. NetVLAD._init_params ----------------------------------------------------------------------------------
@pytest.mark.parametrize("where", ["cpu", "device"])
def test_init_params_sets_alpha_centroids_and_weights(dev, golden, where):
    g = golden["k64"]
    torch.manual_seed(0)
    pool = models.create("netvlad", num_clusters=64, dim=128)
    with pytest.raises(ValueError, match="clsts"):
        pool._init_params()
    if where == "device":
        pool = pool.to(dev)
    x = torch.randn((2, 128, 4, 6), generator=torch.Generator().manual_seed(1)).to(dev)
    pool.to(dev)(x)                                              # a forward BEFORE: whatever it cached must not survive
    if where == "cpu":
        pool = pool.cpu()
    pool.clsts, pool.traindescs = g["clsts"], torch.from_numpy(g["traindescs"])     # numpy or tensors
    gen = pool._cache_gen if hasattr(pool, "_cache_gen") else 0
    pool._init_params()
    assert pool.centroids.device.type == ("cpu" if where == "cpu" else "cuda")
    assert isinstance(pool.alpha, float) and abs(pool.alpha - float(g["alpha"])) <= TOL_ALPHA * float(g["alpha"])
    assert_rel_l2("conv.weight", pool.conv.weight.detach().cpu(), g["conv_weight"], TOL_WEIGHT)
    assert np.array_equal(pool.centroids.detach().cpu().numpy(), g["clsts"])
    assert pool._cache_gen > gen
    fresh = models.create("netvlad", num_clusters=64, dim=128)
    fresh.load_state_dict({k: v.detach().cpu().clone() for k, v in pool.state_dict().items()})
    got, want = pool.to(dev)(x), fresh.to(dev)(x)
    assert tuple(got.shape) == (2, 64, 128) and bool(torch.isfinite(got).all())
    assert torch.equal(got, want)


# ---- 5. end to end --------------------------------------------------------------------------------------------
def test_cache_file_to_initialised_model_end_to_end(dev, state_dict, tmp_path):
    base = models.create("vgg16", pretrained=False)
    pool = models.create("netvlad", dim=base.feature_dim)
    model = models.create("embednet", base, pool)
    base.load_state_dict({k[len("base_model."):]: v for k, v in state_dict.items() if k.startswith("base_model.")})
    model = model.to(dev).eval().set_precision("fp32")
    x = synth.images(8, 64, 96, seed=21)                         # 4 x 6 maps: 24 positions
    batches = [x[:3], (x[3:6], None, None, None, None), x[6:]]
    path = str(tmp_path / "vgg16_synthetic_64_desc_cen.hdf5")
    np.random.seed(43)
    cluster.build_init_cache(model, batches, path, num_clusters=64, seed=43, n_descriptors=80, n_per_image=10)
    clsts, descs = cluster.load_init_cache(path)
    assert clsts.shape == (64, 512) and descs.shape == (80, 512) and clsts.dtype == descs.dtype == np.float32
    assert np.abs(np.linalg.norm(descs.astype(np.float64), axis=1) - 1).max() <= 1e-6
    np.random.seed(43)
    pos = cluster.sample_positions(8, 24, 10)
    direct = torch.cat([ops.local_descriptors(base.features_nhwc(x[a:b].to(dev)), pos[a:b])     # the same batches
                        for a, b in ((0, 3), (3, 6), (6, 8))])
    assert np.array_equal(descs, direct.cpu().numpy())
    pool.clsts, pool.traindescs = clsts, descs
    model._init_params()                                          # EmbedNet delegates to base_model and net_vlad
    assert isinstance(pool.alpha, float) and np.isfinite(pool.alpha) and pool.alpha > 0
    assert np.array_equal(pool.centroids.detach().cpu().numpy(), clsts)
    pool_x, vlad = model(x.to(dev))
    assert tuple(vlad.shape) == (8, 64 * 512) and bool(torch.isfinite(vlad).all())
    assert float((vlad.double().norm(dim=1) - 1).abs().max()) <= 1e-5
    region = models.create("embedregionnet", base, pool, tuple_size=1).to(dev)
    region._init_params()
    region.train()
    with pytest.raises(NotImplementedError):
        region(x.to(dev))
