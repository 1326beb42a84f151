"""The NetVLAD head's backward without a GPU: the float64 helper against the reference's autograd (the goldens), the
two new entries at the C boundary (declared, exported, bound, documented, validating before any HIP call), the
workspace's shape, and the compiler's report of the new kernels."""
import ctypes
import re
from pathlib import Path

import numpy as np
import pytest

from helpers import netvlad_grad_ref as ref

ROOT = Path(__file__).resolve().parent.parent
HEADER = ROOT / "include" / "openibl_amd.h"
GOLDEN = ROOT / "tests" / "golden"
ENTRIES = ("oibl_netvlad_backward_workspace_bytes", "oibl_netvlad_backward")
CONTRACTIONS = ("nvb_contract_kernel", "nvb_aggregate_kernel", "nvb_dx_kernel")
STREAMING = ("nvb_assign_kernel", "nvb_rowstats_kernel", "nvb_dv_kernel", "nvb_reduce_kernel")
CASES = ("netvlad_backward_2x3x5_norm", "netvlad_backward_3x4x6_raw")
TRAINED = "netvlad_backward_trained_2x12x16"
SATURATED = "netvlad_backward_saturated_2x8x8"
TUPLE = "netvlad_backward_tuple_1x4x8x8"
_drawn = {}


def draw_regime_case(name):
    """(inputs, info, float64 gradients) of one of the three trained-regime fixtures, from its seed; once per session."""
    if name not in _drawn:
        z = np.load(GOLDEN / f"{name}.npz")
        N, h, w_, C = map(int, z["shape"])
        if name == TUPLE:
            B, n = map(int, z["tuple"])
            assert B * n == N
            x, w, c, G, info = ref.draw_tuple_inputs(int(z["seed"]), B, n, h, w_, float(z["jitter"]))
        else:
            x, w, c, G, info = ref.draw_trained_inputs(int(z["seed"]), N, h, w_, sharpen=float(z["sharpen"]))
        _drawn[name] = ((x, w, c, G), info, ref.head_and_grads(x, w, c, G, True))
    return _drawn[name]


@pytest.mark.parametrize("name", CASES)
def test_float64_helper_against_the_reference_autograd(name):
    """The reference's fp32 autograd (EmbedNet over a stub base, vlad_x.backward(G)) against the float64 formulas,
    at the generator's bound; the stored error figures are the ones the generator printed."""
    z = np.load(GOLDEN / f"{name}.npz")
    N, h, w_, C = map(int, z["shape"])
    x, w, c, G = ref.draw_inputs(int(z["seed"]), N, h, w_)
    want = ref.head_and_grads(x, w, c, G, bool(z["normalize_input"]))
    stride = int(z["vlad_stride"])
    errs = {"Y": ref.rel_l2(z["vlad_x"], want["Y"][:, ::stride])}
    for k in ("dW", "dC", "dX"):
        assert z[k].shape == want[k].shape
        errs[k] = ref.rel_l2(z[k], want[k])
    print(name, errs, "stored", z["ref_err"].tolist())
    assert max(errs.values()) <= 1e-5, errs
    np.testing.assert_allclose([errs["dW"], errs["dC"], errs["dX"]], z["ref_err"], rtol=1e-6)
    assert (GOLDEN / f"{name}.npz").stat().st_size < 500_000


@pytest.mark.parametrize("name", (TRAINED, SATURATED, TUPLE))
def test_float64_helper_against_the_reference_autograd_in_the_trained_regime(name):
    """As above for the three fixtures of the regime a training run is in.  dX is stored at every dx_stride-th pixel
    of an image: `ref_err` is the generator's figure over the full arrays (dW, dC reproduce it), `ref_err_dx_stored`
    the one over the stored rows.  dW of the saturated case tends to zero with the softmax's saturation; the generator
    does not assert its error, and neither does this test beyond reproducing the stored figure."""
    z = np.load(GOLDEN / f"{name}.npz")
    N, h, w_, C = map(int, z["shape"])
    (x, w, c, G), info, want = draw_regime_case(name)
    assert x.shape == (N, h, w_, C) and bool(z["normalize_input"])
    stride, dxs = int(z["vlad_stride"]), int(z["dx_stride"])
    errs = {"Y": ref.rel_l2(z["vlad_x"], want["Y"][:, ::stride]),
            "dW": ref.rel_l2(z["dW"], want["dW"]), "dC": ref.rel_l2(z["dC"], want["dC"]),
            "dX": ref.rel_l2(z["dX"], want["dX"].reshape(N, h * w_, C)[:, ::dxs])}
    print(name, errs, "stored", z["ref_err"].tolist(), float(z["ref_err_dx_stored"]))
    assert z["dW"].shape == want["dW"].shape and z["dC"].shape == want["dC"].shape
    judged = {k: v for k, v in errs.items() if not (name == SATURATED and k == "dW")}
    assert max(judged.values()) <= 1e-5, errs
    assert float(z["ref_err"][1]) <= 1e-5 and float(z["ref_err"][2]) <= 1e-5
    np.testing.assert_allclose([errs["dW"], errs["dC"]], z["ref_err"][:2], rtol=1e-6)
    np.testing.assert_allclose(errs["dX"], float(z["ref_err_dx_stored"]), rtol=1e-6)
    for k in ("alpha", "mean_max_a", "min_A"):
        np.testing.assert_allclose(info[k], float(z[k]), rtol=1e-9)
    if name == TUPLE:
        np.testing.assert_allclose(info["cancellation"], float(z["cancellation"]), rtol=1e-6)
    assert (GOLDEN / f"{name}.npz").stat().st_size < 500_000


@pytest.mark.parametrize("name", (TRAINED, SATURATED, TUPLE, "random labels"))
def test_trained_recipes_are_deterministic(name):
    """Two draws from the seed are the same bits: the fixtures' inputs, and a draw with random labels."""
    if name == "random labels":
        a, b = ref.draw_trained_inputs(54, 3, 5, 8, 4.0, False), ref.draw_trained_inputs(54, 3, 5, 8, 4.0, False)
    else:
        inputs, info, _ = draw_regime_case(name)
        a = inputs + (info,)
        _drawn.pop(name)
        inputs, info, _ = draw_regime_case(name)
        b = inputs + (info,)
    for s, t in zip(a[:4], b[:4]):
        assert s is not t and s.dtype == np.float32 and s.tobytes() == t.tobytes()
    assert {k: v for k, v in a[4].items() if k != "descs"} == {k: v for k, v in b[4].items() if k != "descs"}


def test_regimes_of_the_cases():
    """What the fixtures are for, on the helper's float64 values: the trained and the tuple case have a peaked but
    unsaturated soft-assignment, the saturated one is saturated, the populated ones leave no cluster empty (with
    a saturated softmax AND near-empty clusters fp32 autograd itself is wrong by half: that regime is no yardstick),
    the tuple's dC contributions cancel at least 10-fold — and draw_inputs under normalize_input is the uniform
    regime: a_pk is 1/64 within some 10 %."""
    for name in (TRAINED, TUPLE):
        info = draw_regime_case(name)[1]
        print(name, {k: v for k, v in info.items() if k != "descs"})
        assert 0.6 <= info["mean_max_a"] <= 0.9
    assert draw_regime_case(SATURATED)[1]["mean_max_a"] >= 0.999
    for name in (TRAINED, SATURATED):
        assert draw_regime_case(name)[1]["min_A"] >= 0.5
    assert draw_regime_case(TUPLE)[1]["cancellation"] >= 10.0
    x, w, c, G = ref.draw_inputs(41, 2, 3, 5)
    a = ref.head_and_grads(x, w, c, G, True)["a"]
    print("draw_inputs, normalised: mean max_k a_pk", a.max(2).mean())
    assert a.max(2).mean() <= 0.05
    # about half of a trained-like map is exact zeros, none of it is negative, and the tuple's G rows cancel
    (x, _, _, _), _, _ = draw_regime_case(TRAINED)
    assert x.min() == 0.0 and 0.4 <= (x == 0).mean() <= 0.6
    G = draw_regime_case(TUPLE)[0][3]
    assert np.abs(G.astype(np.float64).sum(0)).max() <= 1e-6 * np.abs(G).max()


def test_header_declares_and_library_exports_the_backward_entries():
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


def test_backward_workspace_is_linear_in_the_batch_and_smaller_without_grad_feat():
    from openibl_amd import lib
    h = lib.load()
    K, C = 64, 512
    full = h.oibl_netvlad_backward_workspace_bytes(12, 1200, K, C, 1)
    lean = h.oibl_netvlad_backward_workspace_bytes(12, 1200, K, C, 0)
    # a and ds [N][P][64], V and the per-image dW [N][K][C]
    assert full >= 12 * (2 * 1200 * 64 + 2 * K * C) * 4
    assert lean < full and full - lean == 12 * 1200 * 64 * 4
    assert h.oibl_netvlad_backward_workspace_bytes(48, 1200, K, C, 1) == 4 * full
    assert h.oibl_netvlad_backward_workspace_bytes(48, 1200, K, C, 0) == 4 * lean
    # nothing of the reference's residual[N][K][C][P] (157 MB per image at 30 x 40)
    assert full < 12 * 2 * 1024 * 1024
    for bad in ((0, 1200, K, C), (12, 0, K, C), (12, 1200, 32, C), (12, 1200, K, 256)):
        assert h.oibl_netvlad_backward_workspace_bytes(*bad, 1) == 0


def test_backward_argument_validation_launches_nothing():
    from openibl_amd import lib
    h = lib.load()
    K, C = 64, 512
    F32, BF16 = 1, 0
    buf = ctypes.create_string_buffer(4096 + 256)       # never dereferenced: validation fails first
    ptr = (ctypes.addressof(buf) + 255) // 256 * 256
    big = 1 << 40

    def call(feat=ptr, N=1, P=15, K_=K, C_=C, prec=F32, w=ptr, c=ptr, g=ptr, gw=ptr, gc=ptr, gx=ptr, ws=ptr,
             ws_bytes=big):
        return h.oibl_netvlad_backward(feat, N, P, K_, C_, prec, w, c, 1, g, gw, gc, gx, ws, ws_bytes, None)

    for kw in ({"feat": None}, {"w": None}, {"c": None}, {"g": None}, {"ws": None}):
        assert call(**kw) == -1 and b"null" in h.oibl_last_error(), kw
    assert call(gw=None, gc=None, gx=None) == -1 and b"no output" in h.oibl_last_error()
    assert call(K_=32) == -1 and b"num_clusters" in h.oibl_last_error()
    assert call(C_=256) == -1 and b"dim = 512" in h.oibl_last_error()
    assert call(prec=BF16) == -1 and b"fp32" in h.oibl_last_error()
    assert call(N=0) == -1 and b"N=0" in h.oibl_last_error()
    assert call(P=0) == -1 and b"P=0" in h.oibl_last_error()
    assert call(N=65536) == -1 and b"65535" in h.oibl_last_error()      # the image index is a grid dimension
    rc = call(ws_bytes=1024)
    assert rc == -2 and b"workspace 1024 <" in h.oibl_last_error()
    # without grad_feat less is needed: the size that serves that call is short for the full one
    lean = h.oibl_netvlad_backward_workspace_bytes(1, 15, K, C, 0)
    assert call(ws_bytes=lean) == -2
    assert call(ws=ptr + 16) == -2 and b"aligned" in h.oibl_last_error()
    with pytest.raises(lib.OpenIBLAmdError):
        lib.check(rc, "netvlad_backward")


def test_backward_kernels_do_not_spill_and_fit_the_register_file():
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


def test_backward_contractions_run_on_the_matrix_cores():
    """The fp32 contractions are matrix instructions: da (nvb_contract_kernel), V / dW (both instances of
    nvb_aggregate_kernel) and dxh (nvb_dx_kernel); the fp64 assignment (logits on the vector unit: dC needs them
    beyond fp32) and the streaming passes hold none."""
    from openibl_amd import build
    text = build.kernel_text()
    if not text:
        pytest.skip("llvm-objdump / clang-offload-bundler not found next to hipcc")
    text = {n: t for n, t in text.items() if not n.endswith(".kd")}
    for k, instances, least in (("nvb_contract_kernel", 1, 8), ("nvb_aggregate_kernel", 2, 16), ("nvb_dx_kernel", 1, 4)):
        hits = {n: t for n, t in text.items() if k in n}
        assert len(hits) == instances, sorted(hits)
        for n, t in hits.items():
            print(n, t)
            assert t["mfma"] >= least, (n, t)
    for k in STREAMING:
        hits = {n: t for n, t in text.items() if k in n}
        assert len(hits) == 1, sorted(hits)
        assert all(t["mfma"] == 0 for t in hits.values()), hits


def test_netvlad_backward_has_no_cpu_fallback():
    import torch
    from openibl_amd import lib, ops
    x = torch.zeros(1, 3, 5, 512)
    w, c, g = torch.zeros(64, 512), torch.zeros(64, 512), torch.zeros(1, 64 * 512)
    with pytest.raises(lib.OpenIBLAmdError, match="no CPU fallback"):
        ops.netvlad_backward(x, w, c, g)
    with pytest.raises(lib.OpenIBLAmdError, match="no CPU fallback"):
        ops.netvlad_head(x, w, c)
