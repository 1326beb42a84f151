"""conv5 training without a GPU: the float64 helper (tests/helpers/conv_grad_ref.py) against the reference's own fp32
autograd (tests/golden/conv5_backward.npz), the three new entries at the C boundary (declared, exported, bound,
documented, validating before any HIP call), the workspace's shape, the compiler's report of the new kernels, and the
Python surface's refusals."""
import ctypes
import re
from pathlib import Path

import numpy as np
import pytest
import torch

from helpers import conv_grad_ref as ref

ROOT = Path(__file__).resolve().parent.parent
HEADER = ROOT / "include" / "openibl_amd.h"
GOLDEN = ROOT / "tests" / "golden" / "conv5_backward.npz"
ENTRIES = ("oibl_conv3x3_backward_workspace_bytes", "oibl_conv3x3_backward", "oibl_vgg16_pool4_forward")
KERNELS = ("cb_mask_kernel", "cb_wgrad_kernel", "cb_wreduce_kernel", "cb_bsum_kernel", "cb_breduce_kernel",
           "cb_packT_kernel")
REF_ERR_MAX = 1.25e-5          # the generator's assertion: 8 x stays inside the 1e-4 cap of the device tests' bars
C = 512


def _stored_errors(z, prefix, keys, want):
    """rel-L2 of every stored reference array against the float64 value (weight gradients: the stored rows)."""
    errs = {}
    for k in keys:
        got = z[f"{prefix}_{k}"]
        w = want[k]
        if k in ("dW1", "dW2", "dW3"):
            w = w[:ref.W_ROWS]
        elif k in ("dWv", "dCv"):
            w = w[::int(z["e2e_head_stride"])]
        assert got.shape == w.shape, (k, got.shape, w.shape)
        errs[k] = ref.rel_l2(got, w)
    return errs


@pytest.mark.parametrize("name", ["layer_2x2x3", "layer_3x5x7"])
def test_float64_chain_against_the_reference_autograd(name):
    """The reference's VGG.base[24:] under fp32 autograd against the float64 chain.  What the fixture stores in full
    (dX, db1..3) reproduces the stored `ref_err` figure; the four stored rows of a weight gradient are a sample of the
    tensor the figure was taken over: within twice the figure."""
    z = np.load(GOLDEN)
    N, h, w, _ = map(int, z[f"{name}_shape"])
    x, ws, bs, G = ref.draw_inputs(int(z[f"{name}_seed"]), N, h, w)
    want = ref.chain_grads(x, ws, bs, G)
    stored = dict(zip(ref.GRAD_KEYS, z[f"{name}_ref_err"]))
    errs = _stored_errors(z, name, ref.GRAD_KEYS, want)
    errs["y"] = ref.rel_l2(z[f"{name}_y"], want["y"][..., ::int(z[f"{name}_y_stride"])])
    print(name, errs, "stored", stored)
    assert max(stored.values()) <= REF_ERR_MAX and errs["y"] <= REF_ERR_MAX
    for k in ("dX", "db1", "db2", "db3"):
        np.testing.assert_allclose(errs[k], stored[k], rtol=1e-6)
    for k in ("dW1", "dW2", "dW3"):
        assert errs[k] <= 2 * stored[k], (k, errs[k], stored[k])


def test_float64_embednet_against_the_reference_autograd():
    """The reference's EmbedNet under the triplet loss, fp32, against the float64 evaluation of the whole network."""
    from openibl_amd import synth
    z = np.load(GOLDEN)
    B, n, H, W = map(int, z["e2e_shape"])
    state = {k: v for k, v in synth.embednetpca_state(0).items() if not k.startswith("pca_layer")}
    want = ref.embednet_grads(synth.images(B * n, H, W, seed=int(z["e2e_seed"])), state, B, n)
    stored = dict(zip(ref.E2E_KEYS, z["e2e_ref_err"]))
    errs = _stored_errors(z, "e2e", ref.E2E_KEYS, want)
    print("e2e", errs, "stored", stored, "loss", float(z["e2e_loss"]), want["loss"])
    assert max(stored.values()) <= REF_ERR_MAX
    assert abs(float(z["e2e_loss"]) - want["loss"]) <= 1e-6 * want["loss"] and want["loss"] > 0
    assert ref.rel_l2(z["e2e_vlad"], want["vlad"][:, ::int(z["e2e_vlad_stride"])]) <= 2e-6
    for k in ("db1", "db2", "db3"):
        np.testing.assert_allclose(errs[k], stored[k], rtol=1e-6)
    for k in ("dW1", "dW2", "dW3", "dWv", "dCv"):
        assert errs[k] <= 2 * stored[k], (k, errs[k], stored[k])
    assert GOLDEN.stat().st_size < 1_000_000


def test_layer_helper_is_the_chain_helper_one_layer_at_a_time():
    x, ws, bs, G = ref.draw_inputs(7, 1, 3, 4)
    a1 = ref.conv_forward(x, ws[0], bs[0], True)
    a2 = ref.conv_forward(a1, ws[1], bs[1], True)
    chain = ref.chain_grads(x, ws, bs, G)
    g3 = ref.layer_grads(a2, ws[2], G)
    g2 = ref.layer_grads(a1, ws[1], g3["dX"], out_act=a2)
    g1 = ref.layer_grads(x, ws[0], g2["dX"], out_act=a1)
    for i, g in ((1, g1), (2, g2), (3, g3)):
        assert ref.rel_l2(g["dW"], chain[f"dW{i}"]) < 1e-13 and ref.rel_l2(g["db"], chain[f"db{i}"]) < 1e-13
    assert ref.rel_l2(g1["dX"], chain["dX"]) < 1e-13


def test_header_declares_and_library_exports_the_new_entries():
    from openibl_amd import lib
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    declared = set(re.findall(r"\b(oibl_[a-z0-9_]+)\s*\(", text))
    raw = ctypes.CDLL(str(lib.lib_path()))
    for name in ENTRIES:
        assert name in declared, f"{name} is not declared in the header"
        assert hasattr(raw, name), f"{name} is not exported by the product library"
        assert name in lib.SIGNATURES
        assert name in (ROOT / "INTEGRATION.md").read_text()


def test_workspace_query():
    from openibl_amd import lib
    h = lib.load()
    q = h.oibl_conv3x3_backward_workspace_bytes
    for bad in ((0, 30, 40), (12, 0, 40), (12, 30, 0), (-1, 30, 40)):
        assert q(*bad, C, C, 1) == 0 and q(*bad, C, C, 0) == 0
    assert q(12, 30, 40, 500, C, 1) == 0 and q(12, 30, 40, C, 256, 1) == 0
    lean, full = q(12, 30, 40, C, C, 0), q(12, 30, 40, C, C, 1)
    # with grad_in: the transposed, flipped weight [9][512][512] and a zero bias
    assert lean > 0 and full - lean >= 9 * C * C * 4
    # the masked grad_out [M][512] and at most 7 fp32 partials of the weight gradient
    M = 12 * 30 * 40
    assert lean >= M * C * 4 + 7 * 9 * C * C * 4
    assert lean <= M * C * 4 + 7 * 9 * C * C * 4 + (M // 256 + 1) * C * 8 + 4096
    # the partials do not grow with the batch beyond their cap
    assert q(48, 30, 40, C, C, 0) - lean <= 3 * M * C * 4 + 3 * (M // 256 + 1) * C * 8 + 4096
    # one pixel: one partial
    assert q(1, 1, 1, C, C, 0) < 2 * 9 * C * C * 4


def test_argument_validation_launches_nothing():
    from openibl_amd import lib
    h = lib.load()
    buf = ctypes.create_string_buffer(4096 + 256)       # never dereferenced: validation fails first
    ptr = (ctypes.addressof(buf) + 255) // 256 * 256
    big = 1 << 40

    def call(x=ptr, N=1, H=2, W=3, cin=C, w=ptr, cout=C, act=ptr, g=ptr, gw=ptr, gb=ptr, gx=ptr, ws=ptr, ws_bytes=big):
        return h.oibl_conv3x3_backward(x, N, H, W, cin, w, cout, act, g, gw, gb, gx, ws, ws_bytes, None)

    for kw in ({"x": None}, {"w": None}, {"g": None}, {"ws": None}):
        assert call(**kw) == -1 and b"null" in h.oibl_last_error(), kw
    assert call(gw=None, gb=None, gx=None) == -1 and b"no output" in h.oibl_last_error()
    assert call(cin=500) == -1 and b"512" in h.oibl_last_error()
    assert call(cout=256) == -1 and b"512" in h.oibl_last_error()
    for kw in ({"N": 0}, {"H": 0}, {"W": -1}):
        assert call(**kw) == -1 and b"bad shape" in h.oibl_last_error(), kw
    assert call(N=65536, H=256, W=256) == -1 and b"2^31" in h.oibl_last_error()
    assert call(g=ptr + 4) == -1 and b"aligned" in h.oibl_last_error()
    rc = call(ws_bytes=1024)
    assert rc == -2 and b"workspace 1024 <" in h.oibl_last_error()
    lean = h.oibl_conv3x3_backward_workspace_bytes(1, 2, 3, C, C, 0)
    assert call(ws_bytes=lean) == -2                      # what serves a call without grad_in is short for the full one
    assert call(ws=ptr + 16) == -2 and b"aligned" in h.oibl_last_error()
    with pytest.raises(lib.OpenIBLAmdError):
        lib.check(rc, "conv3x3_backward")
    # the trunk entry validates like the backbone entry it shares its body with
    arr = (ctypes.c_void_p * 13)(*([ptr] * 13))
    assert h.oibl_vgg16_pool4_forward(ptr, 1, 8, 8, arr, arr, 1, ptr, ptr, big, None) == -1
    assert h.oibl_vgg16_pool4_forward(ptr, 1, 32, 48, arr, arr, 1, None, ptr, big, None) == -1
    assert h.oibl_vgg16_pool4_forward(ptr, 1, 32, 48, arr, arr, 1, ptr, ptr, 1024, None) == -2


def test_kernels_do_not_spill_and_keep_two_waves_per_simd():
    from openibl_amd import build
    usage = build.resource_usage()
    seen = set()
    for name, u in usage.items():
        for k in KERNELS:
            if k in name:
                assert u.get("ScratchSize", 0) == 0, (name, u)
                assert u["VGPRs"] + u.get("AGPRs", 0) <= 256, (name, u)
                seen.add(k)
    assert seen == set(KERNELS), sorted(set(KERNELS) - seen)


def test_the_weight_gradient_runs_on_the_matrix_cores():
    """64 fp32 matrix instructions per 32-pixel step (16 pixel pairs x 2 x 2 tiles of 32 x 32 per wave); the streaming
    passes hold none."""
    from openibl_amd import build
    text = build.kernel_text()
    if not text:
        pytest.skip("llvm-objdump / clang-offload-bundler not found next to hipcc")
    text = {n: t for n, t in text.items() if not n.endswith(".kd")}
    for k in KERNELS:
        hits = {n: t for n, t in text.items() if k in n}
        assert len(hits) == 1, (k, sorted(hits))
        for n, t in hits.items():
            print(n, t)
            assert t["mfma"] == (64 if k == "cb_wgrad_kernel" else 0), (n, t)


def test_no_cpu_fallback_and_the_python_refusals():
    from openibl_amd import lib, models, ops
    x, w, g = torch.zeros(1, 2, 3, C), torch.zeros(C, C, 3, 3), torch.zeros(1, 2, 3, C)
    with pytest.raises(lib.OpenIBLAmdError, match="no CPU fallback"):
        ops.conv3x3_backward(x, w, g)
    with pytest.raises(lib.OpenIBLAmdError, match="no CPU fallback"):
        ops.conv3x3_train(x, w, torch.zeros(C), True)
    with pytest.raises(lib.OpenIBLAmdError, match="no CPU fallback"):
        ops.vgg16_pool4(torch.zeros(1, 3, 32, 48), [w] * 13, [torch.zeros(C)] * 13, "fp32")
    model = models.EmbedNet(models.vgg16(pretrained=False), models.NetVLAD())
    for layers in ("conv4", "conv3", "conv2", "full"):
        with pytest.raises(NotImplementedError, match="pool4"):
            model.forward_train(torch.zeros(1, 3, 32, 48), train_layers=layers)
    with pytest.raises(ValueError):
        model.forward_train(torch.zeros(1, 3, 32, 48), train_layers="conv6")
