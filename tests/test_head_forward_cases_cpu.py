"""The cases of tests/test_gpu_head_forward_edges.py (and the PCA shapes added to tests/test_gpu_netvlad_pca.py),
checked on the host before any kernel sees them:

1. conditioning — the float32 host restatement of the head (helpers.head_forward_ref.host_fp32) is within 5e-6 of the
   fp64 oracle, per image (NetVLAD) / per (image, region) vector: a kernel that misses its bar on such a case is wrong,
   the case is not.  Measured with these recipes: NetVLAD <= 8.3e-7 per image (bf16-mirrored inputs <= 1.7e-6), region
   <= 2.7e-6 per vector (worst: 3 x (4 x 6), sharpen 4), normalize_input=False <= 4e-7 at max |logit| ~ 790 and ~ 3160;
2. saturation — info["mean_max_a"] >= 0.70 at sharpen 1, >= 0.9999 at sharpen 4; the normalize_input=False cases carry
   logits beyond expf's overflow (88.7): a softmax without its maximum gives inf / inf there;
3. the slab and chunk arithmetic each case is listed for, computed from P and N by the Python restatement of the
   kernels' host arithmetic — which is itself tied to the constants in the kernel sources, and, where a workspace
   query exposes it, to the library.
"""
import re
from pathlib import Path

import pytest
import torch

from helpers import head_forward_ref as hf

CSRC = Path(__file__).resolve().parent.parent / "openibl_amd" / "csrc"
COND = 5e-6


def _src(name):
    return (CSRC / name).read_text()


def _const(text, name):
    m = re.search(r"\b" + name + r"\s*=\s*(\d+)\s*[,;]", text)
    assert m, f"constant {name} not found"
    return int(m.group(1))


# ---- 3a. the restated arithmetic is the kernels' -------------------------------------------------------------------
def test_restated_constants_are_the_sources():
    nv, rg, pca = _src("netvlad.hip"), _src("region.hip"), _src("pca.hip")
    assert _const(nv, "NVF_MIN_N") == hf.NVF_MIN_N
    assert "return (N <= 4 && P >= 256) ? 4 : 1;" in nv
    assert "return N >= 16 ? 160 : N >= 8 ? 96 : N >= 4 ? 64 : 32;" in nv
    assert "(((P + slabs - 1) / slabs + 31) / 32) * 32" in nv
    assert "Cfg::BN == 64 && Cfg::BM == 128" in nv and hf.ASSIGN_BM == 128
    core = _src("vlad_forward_core.h")                                # the slab body both units wrap
    assert '#include "vlad_forward_core.h"' in nv and '#include "vlad_forward_core.h"' in rg
    assert "vlad_fused_slab(PlainSlabs{" in nv and "vlad_fused_slab(QuarterSlabs{" in rg
    assert "p0 += 32" in nv and "p0 += 32" in core and hf.CHUNK == 32
    assert _const(rg, "RG_SLAB_TARGET") == hf.RG_SLAB_TARGET
    for name in ("PS_ROWS", "PS_SPLITS", "PS_MAXN", "PK_WAVES", "PK_SPLITS", "PK_CHUNK", "PK_MAXN", "PRN_PER"):
        assert _const(pca, name) == getattr(hf, name), name
    assert "while (tiles * s < 512 && ksteps % (s * 2) == 0 && ksteps / (s * 2) >= 16) s *= 2;" in pca
    assert "d <= 1024 * PRN_PER" in pca


def test_restated_slab_counts_are_the_librarys():
    """The workspace queries are host arithmetic over the same slab counts (the fused kernel's partials for
    NetVLAD — they outnumber the pixel split's four —, the quarters' partials for the region head)."""
    from openibl_amd import lib
    h = lib.load()

    def up(n):
        return (n + 255) // 256 * 256

    for N, P in [(c.drawn, c.hw[0] * c.hw[1]) for c in hf.NETVLAD_CASES] + [(1, 1200), (32, 1200), (4, 64), (8, 97)]:
        fixed = up(N * P * 4) + up(N * P * 64 * 4) + up(N * 64 * 512 * 4) + up(64 * 512 * 2) + up(N * 64 * 2 * 4)
        slabs = max(hf.nvf_slabs(N, P)[0], hf.nv_pixel_slabs(N, P)[0])
        assert h.oibl_netvlad_workspace_bytes(N, P, 64, 512) == fixed + up(slabs * N * 64 * 512 * 4), (N, P)
    for N, (hh, ww) in [(c.drawn, c.hw) for c in hf.REGION_CASES] + [(1, (30, 40))]:
        nslab = hf.rg_slabs(hh, ww)[1]
        assert h.oibl_region_workspace_bytes(N, hh, ww, 64, 512) == \
            up(N * 4 * nslab * 64 * 512 * 4) + up(N * 9 * 64 * 4), (N, hh, ww)


# ---- 3b. every case has the edge it is listed for ------------------------------------------------------------------
NV_EDGES = {
    # (path, h, w) -> what the arithmetic must say for the largest call
    ("unsplit", 1, 31): dict(P=31, slabs=1, chunks=(1, 31)),
    ("unsplit", 4, 8): dict(P=32, slabs=1, chunks=(1, 32)),
    ("unsplit", 3, 11): dict(P=33, slabs=1, chunks=(2, 1)),
    ("unsplit", 15, 17): dict(P=255, slabs=1, chunks=(8, 31)),
    ("unsplit", 1, 43): dict(P=43, slabs=1, chunks=(2, 11), rows=129),
    ("slabs", 16, 16): dict(P=256, slabs=4, pchunk=64, sizes=[64, 64, 64, 64]),
    ("slabs", 16, 17): dict(P=272, slabs=4, pchunk=96, sizes=[96, 96, 80, 0]),
    ("slabs", 13, 20): dict(P=260, slabs=4, pchunk=96, sizes=[96, 96, 68, 0]),
    ("slabs", 11, 35): dict(P=385, slabs=4, pchunk=128, sizes=[128, 128, 128, 1]),
    ("fused", 3, 53): dict(P=159, sizes=[159]),
    ("fused", 8, 20): dict(P=160, sizes=[160]),
    ("fused", 7, 23): dict(P=161, sizes=[160, 1]),
    ("fused", 3, 107): dict(P=321, sizes=[160, 160, 1]),
    ("fused3", 3, 11): dict(P=33, sizes=[32, 1]),
    ("fused3", 5, 13): dict(P=65, sizes=[64, 1]),
    ("fused3", 1, 97): dict(P=97, sizes=[96, 1]),
}


@pytest.mark.parametrize("case", hf.NETVLAD_CASES, ids=lambda c: f"{c.path}-{c.hw[0]}x{c.hw[1]}")
def test_netvlad_case_arithmetic(case):
    want = NV_EDGES[(case.path, *case.hw)]
    P = case.hw[0] * case.hw[1]
    assert P == want["P"] and case.drawn >= 2 and case.drawn == max(case.calls)
    if case.path in ("unsplit", "slabs"):
        for n in case.calls:                                          # every call takes the named path by default
            assert n < hf.NVF_MIN_N
            slabs, pchunk, sizes = hf.nv_pixel_slabs(n, P)
            assert slabs == want["slabs"]
            if slabs > 1:
                assert pchunk == want["pchunk"] and sizes == want["sizes"] and sum(sizes) == P
            else:
                assert hf.chunks(P) == want["chunks"]
        if "rows" in want:                                            # the assign tile: a second tile of one row
            rows = case.drawn * P
            assert rows == want["rows"] and rows % hf.ASSIGN_BM == 1 and rows // hf.ASSIGN_BM == 1
    elif case.path == "fused":
        for n in case.calls:                                          # one kernel selection, one slab size
            assert n >= hf.NVF_MIN_N and hf.nvf_slab_px(n) == 160
            assert hf.nvf_slabs(n, P)[1] == want["sizes"]
    else:
        px = hf.nvf_slab_px(case.drawn)
        assert px == want["sizes"][0] and case.drawn < hf.NVF_MIN_N
        for n in case.calls:                                          # (the smaller call shares the slab size)
            assert hf.nvf_slab_px(n) == px and hf.nvf_slabs(n, P)[1] == want["sizes"]
    assert set(case.precisions) <= {"fp32", "bf16"}
    if case.path.startswith("fused"):
        assert case.precisions == ("fp32",)                           # bf16 maps never take the fused kernel


def test_the_three_fused_slab_sizes_below_sixteen_images_are_covered():
    assert sorted(hf.nvf_slab_px(c.drawn) for c in hf.NETVLAD_CASES if c.path == "fused3") == [32, 64, 96]


RG_EDGES = {
    (2, 2): dict(pq=1, sizes=[1], hq=1),
    (8, 16): dict(pq=32, sizes=[32], hq=4),
    (6, 22): dict(pq=33, sizes=[33], hq=3),
    (2, 66): dict(pq=33, sizes=[33], hq=1),
    (14, 18): dict(pq=63, sizes=[63], hq=7),
    (16, 16): dict(pq=64, sizes=[64], hq=8),
    (10, 26): dict(pq=65, sizes=[33, 32], hq=5),
    (4, 6): dict(pq=6, sizes=[6], hq=2),
}


@pytest.mark.parametrize("case", hf.REGION_CASES, ids=lambda c: f"{c.drawn}x{c.hw[0]}x{c.hw[1]}")
def test_region_case_arithmetic(case):
    want = RG_EDGES[case.hw]
    pq, nslab, sizes = hf.rg_slabs(*case.hw)
    assert (pq, sizes) == (want["pq"], want["sizes"]) and nslab == len(sizes) and case.hw[0] // 2 == want["hq"]
    assert case.drawn >= 2 and max(sizes) <= hf.RG_SLAB_TARGET


def test_pca_shape_arithmetic():
    """The PCA shapes of tests/test_gpu_netvlad_pca.py reach the kernels and branches they are listed for."""
    # the row-major streaming kernel: kper = D / 8, 512 columns per loop trip
    for (D, d), trips in (((4096, 128), 1), ((8192, 384), 2)):
        assert hf.pca_small_ok(1, D, d) and hf.pca_small_ok(2, D, d) and not hf.pca_small_ok(3, D, d)
        assert D // hf.PS_SPLITS // 512 == trips and d % 128 == 0
    # the tile where the streaming kernel refuses: one split, several
    assert not hf.pca_small_ok(1, 4128, 128) and hf.pca_splits(1, 4128, 128) == (129, 1)
    assert hf.pca_splits(2, 4128, 128) == (129, 1)
    assert not hf.pca_small_ok(1, 2048, 128) and hf.pca_splits(1, 2048, 128) == hf.pca_splits(2, 2048, 128) == (64, 4)
    # bf16 tile
    assert hf.pca_splits(5, 2112, 256, bf16=True) == (33, 1) and hf.pca_splits(5, 4096, 256, bf16=True) == (64, 4)
    # ragged M tiles: one plan for every N compared
    for bf16, plan in ((False, (64, 4)), (True, (32, 2))):
        assert {hf.pca_splits(n, 2048, 256, bf16) for n in (31, 32, 33, 64, 65)} == {plan}
    # packed stream: chunks per K part, the reduction taken
    for (D, d), n_chunks, one_launch, clamped in (((16384, 256), 2, True, True), ((8192, 768), 1, True, True),
                                                  ((8192, 4352), 1, False, False)):
        for n in (3, 32):
            assert hf.pca_stream_ok(n, D, d)
        assert D // hf.PK_SPLITS // hf.PK_CHUNK == n_chunks
        assert (d <= 1024 * hf.PRN_PER) == one_launch
        assert (one_launch and d % 1024 != 0) == clamped
    assert not hf.pca_stream_ok(33, 16384, 256)


# ---- 1 + 2. conditioning and saturation ------------------------------------------------------------------------------
@pytest.mark.parametrize("sharpen", hf.SHARPEN)
@pytest.mark.parametrize("case", hf.NETVLAD_CASES, ids=lambda c: f"{c.path}-{c.drawn}x{c.hw[0]}x{c.hw[1]}")
def test_netvlad_case_is_well_conditioned_and_saturated(case, sharpen):
    x, aw, c, info = hf.netvlad_case(case, sharpen)
    assert tuple(x.shape) == (case.drawn, *case.hw, hf.C) and x.dtype == torch.float32
    assert float(x[0, 0, 0].abs().max()) == 0.0 and float(x[-1, -1, -1].abs().max()) == 0.0
    print(f"{case.path} {case.drawn}x{case.hw} sharpen {sharpen}: mean_max_a {info['mean_max_a']:.6f}")
    assert info["mean_max_a"] >= hf.MIN_MEAN_MAX_A[sharpen]
    for precision in case.precisions:
        r = hf.netvlad_reference(case, sharpen, precision)
        print(f"  {precision}: host fp32 against fp64, worst image: raw {r['host_raw']:.3e} normalised {r['host_nrm']:.3e}")
        assert torch.isfinite(r["raw"]).all() and torch.isfinite(r["nrm"]).all()
        assert r["host_raw"] <= COND and r["host_nrm"] <= COND


@pytest.mark.parametrize("scale", hf.LARGE_LOGIT_SCALES)
def test_large_logit_case_is_well_conditioned_and_overflows_a_naive_softmax(scale):
    x, aw, c, _ = hf.large_logit_case(scale)
    for precision in ("fp32", "bf16"):
        xi, wi = (x, aw) if precision == "fp32" else (hf.bf16_mirror(x), hf.bf16_mirror(aw))
        top = hf.max_abs_logit(xi, wi, False)
        raw, nrm = hf.oracle_netvlad(xi, wi, c, False)
        hr, hn = hf.host_fp32(xi, wi, c, False)
        er, en = hf.worst_row(hr, raw, 2), hf.worst_row(hn, nrm, 2)
        print(f"scale {scale} {precision}: max |logit| {top:.1f}, host fp32 raw {er:.3e} normalised {en:.3e}")
        assert top > hf.EXPF_OVERFLOW
        assert er <= COND and en <= COND


@pytest.mark.parametrize("sharpen", hf.SHARPEN)
@pytest.mark.parametrize("case", hf.REGION_CASES, ids=lambda c: f"{c.drawn}x{c.hw[0]}x{c.hw[1]}")
def test_region_case_is_well_conditioned_and_saturated(case, sharpen):
    x, aw, c, info = hf.region_case(case, sharpen)
    print(f"region {case.drawn}x{case.hw} sharpen {sharpen}: mean_max_a {info['mean_max_a']:.6f}")
    assert info["mean_max_a"] >= hf.MIN_MEAN_MAX_A[sharpen]
    want = hf.oracle_region(x, aw, c, True)
    e = hf.worst_row(hf.host_fp32(x, aw, c, True, region=True), want, case.drawn * 9)
    print(f"  host fp32 against fp64, worst (image, region) vector {e:.3e}")
    assert torch.isfinite(want).all() and e <= COND


def test_region_raw_case_is_well_conditioned():
    x, aw, c, _ = hf.region_raw_case()
    top = hf.max_abs_logit(x, aw, False)
    want = hf.oracle_region(x, aw, c, False)
    e = hf.worst_row(hf.host_fp32(x, aw, c, False, region=True), want, 18)
    print(f"region, normalize_input=False: max |logit| {top:.1f}, host fp32 worst vector {e:.3e}")
    assert top > hf.EXPF_OVERFLOW and e <= COND
