"""The SFRS region head's backward without a GPU: the float64 helper (tests/helpers/region_grad_ref.py) against the
reference's own autograd (tests/golden/region_backward.npz), the three new entries at the C boundary (declared,
exported, bound, documented, validating before any HIP call), the workspace's shape, and the compiler's report of the
new kernels."""
import ctypes
import re
from pathlib import Path

import numpy as np
import pytest

from helpers import region_grad_ref as ref

ROOT = Path(__file__).resolve().parent.parent
HEADER = ROOT / "include" / "openibl_amd.h"
GOLDEN = ROOT / "tests" / "golden" / "region_backward.npz"
ENTRIES = ("oibl_region_backward_workspace_bytes", "oibl_region_vlad_backward", "oibl_region_scores_backward")
CONTRACTIONS = ("rgb_contract_kernel", "rgb_aggregate_kernel", "rgb_dx_kernel")
STREAMING = ("rgb_assign_kernel", "rgb_rowstats_kernel", "rgb_dv_kernel", "rgb_reduce_kernel", "rgb_scores_kernel")
HEAD_CASES = ("trained_3x4x6", "raw_3x4x6", "tuple_1x4x8x8")


def draw_head_case(name, z=None):
    return ref.golden_head_case(name, np.load(GOLDEN) if z is None else z)


@pytest.mark.parametrize("name", HEAD_CASES)
def test_float64_helper_against_the_reference_autograd(name):
    """The reference's fp32 autograd through EmbedRegionNet._compute_region_sim (and, in the tuple case, its
    SFRSTrainer loss) against the float64 formulas: within the reference's own error against its float64 run, plus
    1e-6."""
    z = np.load(GOLDEN)
    (x, w, c, G, Gs, normalize), want = draw_head_case(name, z)
    loss, want = want["loss"], want["exact"]
    N, h, w_, C = x.shape
    ys, hs, dxs = int(z[f"{name}_y_stride"]), int(z[f"{name}_head_stride"]), int(z[f"{name}_dx_stride"])
    ref_err = dict(zip(("dW", "dC", "dX"), z[f"{name}_ref_err"]))
    errs = {"Y": ref.rel_l2(z[f"{name}_Y"], want["Y"][:, :, ::ys]), "score": ref.rel_l2(z[f"{name}_score"], want["score"]),
            "dW": ref.rel_l2(z[f"{name}_dW"], want["dW"].ravel()[::hs]),
            "dC": ref.rel_l2(z[f"{name}_dC"], want["dC"].ravel()[::hs]),
            "dX": ref.rel_l2(z[f"{name}_dX"], want["dX"].reshape(N, h * w_, C)[:, ::dxs])}
    print(name, errs, "stored", ref_err, "loss", float(z[f"{name}_loss"]), loss)
    assert abs(float(z[f"{name}_loss"]) - loss) <= 1e-5 * abs(loss)
    assert errs["Y"] <= 2e-6 and errs["score"] <= 2e-6
    assert max(ref_err.values()) <= 1.25e-5
    for k, v in ref_err.items():
        assert errs[k] <= float(v) + 1e-6, (k, errs[k], v)
    assert GOLDEN.stat().st_size < 1_000_000


def test_scores_backward_helper_and_stored_errors():
    z = np.load(GOLDEN)
    assert [tuple(r[1:]) for r in z["scores_cases"]] == [(1, 1), (1, 3), (2, 2), (1, 10)]
    assert z["scores_ref_err"].max() <= 1.25e-5 and z["scores_ref_err"].min() > 0
    assert z["e2e_ref_err"].shape == (8,) and z["e2e_ref_err"].max() <= 1.25e-5
    # the helper's two einsums against finite differences of the score table
    Y, Gs = ref.draw_vectors(5, 2, 2, L=16)
    d = ref.scores_backward(Y, Gs, 2)
    rs = np.random.RandomState(1)
    E = rs.randn(*Y.shape)
    f = lambda v: float((ref.scores(v, 2) * Gs).sum())
    num = (f(Y.astype(np.float64) + 1e-6 * E) - f(Y.astype(np.float64) - 1e-6 * E)) / 2e-6
    assert abs(num - float((d * E).sum())) <= 1e-7 * max(1.0, abs(num))


def test_header_declares_and_library_exports_the_region_backward_entries():
    from openibl_amd import lib
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    declared = set(re.findall(r"\b(oibl_[a-z0-9_]+)\s*\(", text))
    raw = ctypes.CDLL(str(lib.lib_path()))
    for name in ENTRIES:
        assert name in declared, f"{name} is not declared in the header"
        assert hasattr(raw, name), f"{name} is not exported by the product library"
        assert name in lib.SIGNATURES
        assert name in (ROOT / "INTEGRATION.md").read_text()
    assert lib.load().oibl_abi_version() == 3


def test_region_backward_workspace_is_linear_in_the_batch_and_smaller_without_grad_feat():
    from openibl_amd import lib
    h = lib.load()
    K, C = 64, 512
    full = h.oibl_region_backward_workspace_bytes(12, 30, 40, K, C, 1)
    lean = h.oibl_region_backward_workspace_bytes(12, 30, 40, K, C, 0)
    # a and ds [N][P][64], the four quarters' V and the per-image dW [N][K][C]
    assert full >= 12 * (2 * 1200 * 64 + 5 * K * C) * 4
    assert lean < full and full - lean == 12 * 1200 * 64 * 4
    assert h.oibl_region_backward_workspace_bytes(48, 30, 40, K, C, 1) == 4 * full
    assert h.oibl_region_backward_workspace_bytes(48, 30, 40, K, C, 0) == 4 * lean
    # nothing of the reference's residual[N*4][K][C][P/4] (157 MB per image at 30 x 40)
    assert full < 12 * 2 * 1024 * 1024
    for bad in ((0, 30, 40, K, C), (12, 31, 40, K, C), (12, 30, 39, K, C), (12, 0, 40, K, C), (12, 30, 40, 32, C),
                (12, 30, 40, K, 256), (65536, 30, 40, K, C)):
        assert h.oibl_region_backward_workspace_bytes(*bad, 1) == 0, bad


def test_region_backward_argument_validation_launches_nothing():
    from openibl_amd import lib
    h = lib.load()
    K, C = 64, 512
    F32, BF16 = 1, 0
    buf = ctypes.create_string_buffer(4096 + 256)       # never dereferenced: validation fails first
    ptr = (ctypes.addressof(buf) + 255) // 256 * 256
    big = 1 << 40

    def call(feat=ptr, N=1, hh=4, ww=6, K_=K, C_=C, prec=F32, w=ptr, c=ptr, g=ptr, gw=ptr, gc=ptr, gx=ptr, ws=ptr,
             ws_bytes=big):
        return h.oibl_region_vlad_backward(feat, N, hh, ww, K_, C_, prec, w, c, 1, g, gw, gc, gx, ws, ws_bytes, None)

    for kw in ({"feat": None}, {"w": None}, {"c": None}, {"g": None}, {"ws": None}):
        assert call(**kw) == -1 and b"null" in h.oibl_last_error(), kw
    assert call(gw=None, gc=None, gx=None) == -1 and b"no output" in h.oibl_last_error()
    assert call(hh=5) == -1 and b"5 x 6" in h.oibl_last_error()
    assert call(ww=7) == -1 and b"4 x 7" in h.oibl_last_error()
    assert call(K_=32) == -1 and b"num_clusters" in h.oibl_last_error()
    assert call(C_=256) == -1 and b"num_clusters" in h.oibl_last_error()
    assert call(prec=BF16) == -1 and b"fp32" in h.oibl_last_error()
    assert call(N=0) == -1 and b"N=0" in h.oibl_last_error()
    assert call(N=65536) == -1 and b"65535" in h.oibl_last_error()
    rc = call(ws_bytes=1024)
    assert rc == -2 and b"workspace 1024 <" in h.oibl_last_error()
    lean = h.oibl_region_backward_workspace_bytes(1, 4, 6, K, C, 0)
    assert call(ws_bytes=lean) == -2
    assert call(ws=ptr + 16) == -2 and b"aligned" in h.oibl_last_error()
    with pytest.raises(lib.OpenIBLAmdError):
        lib.check(rc, "region_vlad_backward")

    def scores(v=ptr, T=1, per=2, L=32768, gs=ptr, out=ptr):
        return h.oibl_region_scores_backward(v, T, per, L, gs, out, None)

    for kw in ({"v": None}, {"gs": None}, {"out": None}):
        assert scores(**kw) == -1 and b"null" in h.oibl_last_error(), kw
    assert scores(per=1) == -1 and b"at least one pair" in h.oibl_last_error()
    assert scores(T=0) == -1 and scores(L=6) == -1


def test_region_backward_kernels_do_not_spill_and_fit_the_register_file():
    """hipcc's per-kernel report of the current build: no scratch, and vector + accumulation registers inside the
    256 a wave can address without giving up a second wave per SIMD."""
    from openibl_amd import build
    usage = build.resource_usage()
    seen = set()
    for name, u in usage.items():
        for k in CONTRACTIONS + STREAMING:
            if k in name:
                assert u.get("ScratchSize", 0) == 0, (name, u)
                assert u["VGPRs"] + u.get("AGPRs", 0) <= 256, (name, u)
                seen.add(k)
    assert seen == set(CONTRACTIONS + STREAMING), sorted(set(CONTRACTIONS + STREAMING) - seen)


def test_region_backward_contractions_run_on_the_matrix_cores():
    """da (rgb_contract_kernel), the quarters' V and dW (both instances of rgb_aggregate_kernel) and dxh
    (rgb_dx_kernel) are matrix instructions; the fp64 passes and the scores' backward hold none."""
    from openibl_amd import build
    text = build.kernel_text()
    if not text:
        pytest.skip("llvm-objdump / clang-offload-bundler not found next to hipcc")
    text = {n: t for n, t in text.items() if not n.endswith(".kd")}
    for k, instances, least in (("rgb_contract_kernel", 1, 8), ("rgb_aggregate_kernel", 2, 16), ("rgb_dx_kernel", 1, 4)):
        hits = {n: t for n, t in text.items() if k in n}
        assert len(hits) == instances, sorted(hits)
        for n, t in hits.items():
            print(n, t)
            assert t["mfma"] >= least, (n, t)
    for k in STREAMING:
        hits = {n: t for n, t in text.items() if k in n}
        assert len(hits) == 1, sorted(hits)
        assert all(t["mfma"] == 0 for t in hits.values()), hits


def test_region_backward_has_no_cpu_fallback():
    import torch
    from openibl_amd import lib, ops
    x = torch.zeros(1, 4, 6, 512)
    w, c, g = torch.zeros(64, 512), torch.zeros(64, 512), torch.zeros(1, 9, 64 * 512)
    with pytest.raises(lib.OpenIBLAmdError, match="no CPU fallback"):
        ops.region_vlad_backward(x, w, c, g)
    with pytest.raises(lib.OpenIBLAmdError, match="no CPU fallback"):
        ops.region_vlad_train(x, w, c)
    with pytest.raises(lib.OpenIBLAmdError, match="no CPU fallback"):
        ops.region_scores_backward(torch.zeros(2, 9, 64), torch.zeros(1, 1, 9, 9), 1)
