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
