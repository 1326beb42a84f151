"""The K-general NetVLAD head (num_clusters = 16 .. 128, csrc/netvlad_k.hip) without a GPU: the four entries at the C
boundary validate before any HIP call, their workspaces grow with N, P and K, `ops` routes K = 64 to the tuned
entry points and the other supported K to the new ones, and the golden file's float64 values are what a numpy
restatement of the kernels' scheme — columns padded to a multiple of 32, masked softmax, pixels in chunks of 32 —
gives."""
import ctypes

import numpy as np
import pytest
import torch

from helpers import netvlad_grad_ref as ref
from helpers import netvlad_k_cases as kc

ENTRIES = ("oibl_netvlad_k_workspace_bytes", "oibl_netvlad_forward_k", "oibl_netvlad_k_backward_workspace_bytes",
           "oibl_netvlad_backward_k")


def _aligned(nbytes=4096):
    buf = ctypes.create_string_buffer(nbytes + 256)       # never dereferenced: validation fails first
    return buf, (ctypes.addressof(buf) + 255) // 256 * 256


def test_forward_k_argument_validation_launches_nothing():
    from openibl_amd import lib
    h = lib.load()
    buf, ptr = _aligned()
    big = 1 << 40

    def call(feat=ptr, N=1, P=15, K=32, C=512, w=ptr, c=ptr, raw=ptr, nrm=ptr, ws=ptr, ws_bytes=big):
        return h.oibl_netvlad_forward_k(feat, N, P, K, C, w, c, 1, raw, nrm, ws, ws_bytes, None)

    for kw in ({"feat": None}, {"w": None}, {"c": None}, {"ws": None}):
        assert call(**kw) == -1 and b"null" in h.oibl_last_error(), kw
    assert call(raw=None, nrm=None) == -1 and b"no output" in h.oibl_last_error()
    for K in (24, 144, 0, 8):
        assert call(K=K) == -1
        assert b"num_clusters" in h.oibl_last_error() and str(K).encode() in h.oibl_last_error(), K
    assert call(C=256) == -1 and b"dim" in h.oibl_last_error() and b"256" in h.oibl_last_error()
    assert call(N=0) == -1 and b"N=0" in h.oibl_last_error()
    assert call(P=0) == -1 and b"P=0" in h.oibl_last_error()
    rc = call(ws_bytes=1024)
    assert rc == -2 and b"workspace 1024 <" in h.oibl_last_error()
    assert call(ws=ptr + 16) == -2 and b"aligned" in h.oibl_last_error()
    with pytest.raises(lib.OpenIBLAmdError):
        lib.check(rc, "netvlad_forward_k")


def test_backward_k_argument_validation_launches_nothing():
    from openibl_amd import lib
    h = lib.load()
    buf, ptr = _aligned()
    big = 1 << 40

    def call(feat=ptr, N=1, P=15, K=32, C=512, w=ptr, c=ptr, g=ptr, gw=ptr, gc=ptr, gx=ptr, ws=ptr, ws_bytes=big):
        return h.oibl_netvlad_backward_k(feat, N, P, K, C, w, c, 1, g, gw, gc, gx, ws, ws_bytes, None)

    for kw in ({"feat": None}, {"w": None}, {"c": None}, {"g": None}, {"ws": None}):
        assert call(**kw) == -1 and b"null" in h.oibl_last_error(), kw
    assert call(gw=None, gc=None, gx=None) == -1 and b"no output" in h.oibl_last_error()
    for K in (24, 144):
        assert call(K=K) == -1
        assert b"num_clusters" in h.oibl_last_error() and str(K).encode() in h.oibl_last_error(), K
    assert call(C=256) == -1 and b"dim" in h.oibl_last_error() and b"256" in h.oibl_last_error()
    assert call(N=0) == -1 and call(P=0) == -1
    rc = call(ws_bytes=1024)
    assert rc == -2 and b"workspace 1024 <" in h.oibl_last_error()
    # without grad_feat less is needed: the size that serves that call is short for the full one
    lean = h.oibl_netvlad_k_backward_workspace_bytes(1, 15, 32, 512, 0)
    assert call(ws_bytes=lean) == -2 and call(gx=None, ws_bytes=lean) != -2
    assert call(ws=ptr + 16) == -2 and b"aligned" in h.oibl_last_error()


def test_workspaces_grow_with_n_p_and_k_and_are_zero_for_a_bad_shape():
    from openibl_amd import lib
    h = lib.load()
    queries = (lambda N, P, K: h.oibl_netvlad_k_workspace_bytes(N, P, K, 512),
               lambda N, P, K: h.oibl_netvlad_k_backward_workspace_bytes(N, P, K, 512, 0),
               lambda N, P, K: h.oibl_netvlad_k_backward_workspace_bytes(N, P, K, 512, 1))
    ks = list(range(16, 129, 16))
    for q in queries:
        for K in ks:
            sizes = [q(N, 48, K) for N in (1, 2, 3, 12, 32)]
            assert sizes[0] > 0 and sizes == sorted(sizes) and sizes[0] % 256 == 0, (K, sizes)
            sizes = [q(3, P, K) for P in (1, 15, 31, 32, 33, 48, 1200)]
            assert sizes == sorted(sizes), (K, sizes)
        sizes = [q(3, 48, K) for K in ks]
        assert sizes == sorted(sizes), sizes
        for bad in ((0, 48, 32), (3, 0, 32), (3, 48, 24), (3, 48, 144), (3, 48, 0)):
            assert q(*bad) == 0, bad
    assert h.oibl_netvlad_k_workspace_bytes(3, 48, 32, 256) == 0
    assert h.oibl_netvlad_k_backward_workspace_bytes(3, 48, 32, 256, 1) == 0
    # nothing of the reference's residual[N][K][C][P] (K x 2.4 MB per image at 30 x 40): a and ds [N][P][KP], three
    # [N][K][C] blocks and one in fp64
    full = h.oibl_netvlad_k_backward_workspace_bytes(12, 1200, 128, 512, 1)
    lean = h.oibl_netvlad_k_backward_workspace_bytes(12, 1200, 128, 512, 0)
    assert full - lean == 12 * 1200 * 128 * 4 and full < 12 * 4 * 1024 * 1024


def test_entries_are_declared_bound_and_documented():
    from pathlib import Path
    from openibl_amd import lib
    root = Path(__file__).resolve().parent.parent
    raw = ctypes.CDLL(str(lib.lib_path()))
    for name in ENTRIES:
        assert name in (root / "include" / "openibl_amd.h").read_text()
        assert hasattr(raw, name) and name in lib.SIGNATURES
        assert name in (root / "INTEGRATION.md").read_text()


class _FakeLib:
    """Records the entry points `ops` calls; every call succeeds, every workspace is 256 bytes."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def fn(*args):
            self.calls.append(name)
            return 256 if name.endswith("workspace_bytes") else 0
        return fn


@pytest.fixture
def fake(monkeypatch):
    from openibl_amd import ops
    lib = _FakeLib()
    monkeypatch.setattr(ops._lib, "load", lambda: lib)
    monkeypatch.setattr(ops, "_need_cuda", lambda *t: torch.device("cpu"))
    monkeypatch.setattr(ops, "_stream", lambda dev: 0)
    monkeypatch.setattr(ops, "_WS", {})
    return lib


def _args(K, N=2, P=6):
    return torch.zeros(N, P, 512), torch.zeros(K, 512), torch.zeros(K, 512), torch.zeros(N, K * 512)


def test_ops_route_64_to_the_tuned_entries_and_other_k_to_the_new_ones(fake):
    from openibl_amd import ops
    x, w, c, g = _args(64)
    raw, nrm = ops.netvlad(x, w, c, want_raw=True)
    assert tuple(raw.shape) == (2, 64, 512) and tuple(nrm.shape) == (2, 64 * 512)
    ops.netvlad_backward(x, w, c, g)
    assert fake.calls == ["oibl_netvlad_workspace_bytes", "oibl_netvlad_forward",
                          "oibl_netvlad_backward_workspace_bytes", "oibl_netvlad_backward"]
    for K in (16, 32, 48, 80, 96, 112, 128):
        fake.calls.clear()
        x, w, c, g = _args(K)
        raw, nrm = ops.netvlad(x, w, c, want_raw=True)
        assert tuple(raw.shape) == (2, K, 512) and tuple(nrm.shape) == (2, K * 512)
        gw, gc, gx = ops.netvlad_backward(x, w, c, g, want=("w", "x"))
        assert tuple(gw.shape) == (K, 512) and gc is None and gx.shape == x.shape
        assert fake.calls == ["oibl_netvlad_k_workspace_bytes", "oibl_netvlad_forward_k",
                              "oibl_netvlad_k_backward_workspace_bytes", "oibl_netvlad_backward_k"], (K, fake.calls)
    # the differentiable head: forward and backward through the same routing; a bf16 map is widened first
    fake.calls.clear()
    x, w, c, g = _args(32)
    w.requires_grad_(True)
    y = ops.netvlad_head(x.bfloat16(), w, c)
    y.backward(g)
    assert fake.calls == ["oibl_netvlad_k_workspace_bytes", "oibl_netvlad_forward_k",
                          "oibl_netvlad_k_backward_workspace_bytes", "oibl_netvlad_backward_k"]
    fake.calls.clear()
    ops.netvlad(x.bfloat16(), w.detach(), c)
    assert fake.calls[-1] == "oibl_netvlad_forward_k"


@pytest.mark.parametrize("K", (20, 8, 144, 1))
def test_ops_reject_an_unsupported_k_before_any_library_call(fake, K):
    from openibl_amd import ops
    x, w, c, g = _args(K)
    for call in (lambda: ops.netvlad(x, w, c), lambda: ops.netvlad_backward(x, w, c, g),
                 lambda: ops.netvlad_head(x, w, c)):
        with pytest.raises(ValueError, match=r"16, 32, 48, 64, 80, 96, 112, 128"):
            call()
    assert fake.calls == []


def test_region_model_names_its_limit_for_other_k():
    from ibl import models
    base = models.create("vgg16", pretrained=False)
    region = models.create("embedregionnet", base, models.create("netvlad", num_clusters=32, dim=512), tuple_size=1)
    x = torch.zeros(2, 3, 64, 96)
    for call in (region.region_similarity, region.forward_train):
        with pytest.raises(ValueError, match="num_clusters = 64"):
            call(x)


def _kernel_scheme_forward(x, w, c, normalize):
    """float64 restatement of the forward kernels' scheme for one batch: K padded to KP = a multiple of 32 with zero
    weight rows, max / exp / sum of the softmax over the K live columns only, zeros in the padded columns of a, the
    aggregation over 32-pixel chunks in pixel order, rows K.. never written."""
    N, P, C = x.shape
    K = w.shape[0]
    KP = (K + 31) // 32 * 32
    wp = np.zeros((KP, C))
    wp[:K] = w
    raw = np.zeros((N, K, C))
    for n in range(N):
        acc, A = np.zeros((KP, C)), np.zeros(KP)
        for p0 in range(0, P, 32):
            xc = np.zeros((32, C))
            live = min(32, P - p0)
            xc[:live] = x[n, p0:p0 + live]
            r = np.sqrt((xc * xc).sum(1)) if normalize else np.ones(32)
            inv = 1.0 / np.maximum(r, 1e-12)
            logits = (xc @ wp.T) * inv[:, None]                 # [32][KP], the padded columns are zeros
            mx = logits[:, :K].max(1, keepdims=True)
            e = np.exp(logits[:, :K] - mx)
            a = np.zeros((32, KP))
            a[:, :K] = e / e.sum(1, keepdims=True)
            a[live:] = 0.0                                      # pixels beyond the image are not stored
            acc += a.T @ (xc * inv[:, None])
            A += a.sum(0)
        raw[n] = acc[:K] - A[:K, None] * c
    t = np.maximum(np.sqrt((raw * raw).sum(2, keepdims=True)), 1e-12)
    U = raw / t
    g = np.maximum(np.sqrt((U * U).sum((1, 2), keepdims=True)), 1e-12)
    return raw, (U / g).reshape(N, K * C)


@pytest.mark.parametrize("name", ("k48_3x6x8_norm", "k16_2x3x5_norm", "k32_1x8x8_raw"))
def test_golden_is_the_padded_masked_scheme_in_float64(name):
    """The golden's float64 vlad_raw and vlad_norm (the reference's own module in float64) against the restatement
    above, and its gradients against the float64 formulas of the helper: the file is checked without a GPU."""
    g = kc.load_golden()
    case = kc.BY_NAME[name]
    x, w, c, G, _ = kc.draw_case(case)
    N, K = case["N"], case["K"]
    x64 = x.astype(np.float64).reshape(N, -1, 512)
    raw, nrm = _kernel_scheme_forward(x64, w.astype(np.float64), c.astype(np.float64), case["normalize"])
    errs = {"vlad_raw": kc.stored_error(g, name, "vlad_raw", raw), "vlad_norm": kc.stored_error(g, name, "vlad_norm", nrm)}
    want = ref.head_and_grads(x, w, c, G, case["normalize"])
    for q in ("dW", "dC", "dX"):
        errs[q] = kc.stored_error(g, name, q, want[q])
    print(name, errs, "the reference's fp32 errors", dict(zip(kc.QUANTITIES, g[f"{name}.ref_err"].tolist())))
    assert max(errs.values()) <= 1e-11, errs
    assert int(g[f"{name}.K"]) == K and int(g[f"{name}.seed"]) == case["seed"]
    assert g[f"{name}.vlad_norm"].shape == (-(-N * K * 512 // kc.STRIDE),)


def test_golden_holds_every_case_and_stays_small():
    g = kc.load_golden()
    for case in kc.CASES:
        name = case["name"]
        assert g[f"{name}.ref_err"].shape == (5,) and (g[f"{name}.ref_err"] > 0).all()
        for k in ("seed", "K", "N", "h", "w", "normalize", "jitter", "sharpen"):
            assert g[f"{name}.{k}"] == case[k], (name, k)
    assert float(g["k32_tuple_4x4x4.cancellation"]) >= 10.0          # the images' dC contributions nearly cancel
    assert float(g["k32_saturated_2x8x8.mean_max_a"]) >= 0.999        # near one-hot
    assert kc.GOLDEN.stat().st_size < 500_000


def test_kernels_do_not_spill_and_the_contractions_run_on_the_matrix_cores():
    """hipcc's report of the current build: no nvk_ kernel uses scratch or more than the 256 registers that leave two
    waves per SIMD; logits, da (nvk_assign_kernel, nvk_contract_kernel), V / dW (both nvk_aggregate_kernel) and dxh
    (nvk_dx_kernel) are matrix instructions, the fp64 assignment (four instances, one per number of column tiles) and
    the streaming passes hold none."""
    from openibl_amd import build
    usage = {n: u for n, u in build.resource_usage().items() if "nvk_" in n}
    assert len(usage) == 14, sorted(usage)
    for n, u in usage.items():
        assert u.get("ScratchSize", 0) == 0 and u["VGPRs"] + u.get("AGPRs", 0) <= 256, (n, u)
    text = build.kernel_text()
    if not text:
        pytest.skip("llvm-objdump / clang-offload-bundler not found next to hipcc")
    text = {n: t for n, t in text.items() if "nvk_" in n and not n.endswith(".kd")}
    for k, instances, least in (("nvk_assign_kernel", 1, 4), ("nvk_contract_kernel", 1, 4),
                                ("nvk_aggregate_kernel", 2, 2), ("nvk_dx_kernel", 1, 4)):
        hits = {n: t for n, t in text.items() if k in n}
        assert len(hits) == instances and all(t["mfma"] >= least for t in hits.values()), (k, hits)
    for k, instances in (("nvk_assign64_kernel", 4), ("nvk_rowstats_kernel", 1), ("nvk_apply_kernel", 1),
                         ("nvk_rowstats64_kernel", 1), ("nvk_dv_kernel", 1), ("nvk_reduce_kernel", 1)):
        hits = {n: t for n, t in text.items() if k in n}
        assert len(hits) == instances and all(t["mfma"] == 0 for t in hits.values()), (k, hits)
