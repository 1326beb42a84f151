"""The references of tests/test_gpu_stem_u8.py, held to account without a GPU (tests/helpers/stem_u8_ref.py):

1. `fma_normalise` is the fma: u * a_c + b_c in float64 is EXACT on all 768 (channel, byte) pairs (rationals), so
   its one rounding to float32 is fmaf's; it also agrees with the mirror of tests/test_stem_u8_cpu.py.
2. The emulation of the f16mx arithmetic on that input, against the fp64 convolutions, uses a fraction of the bars
   the GPU test applies to the kernel (rel-L2 6e-5; per 32-channel group err <= 3e-4 ref + 1e-6): a bar the
   reference nearly filled would prove nothing about the kernel.  Measured: rel-L2 1.32e-5 .. 1.50e-5 on the random
   cases (1.60e-5 on the flat one), largest group err / ref 4.1e-5.
3. The range-flag case does on the CPU what it is meant to do on the device: conv1_1 inside fp16, conv1_2 beyond.
4. The debug library exports the stand-alone entry, the shipping library does not; the entry refuses what the
   public stem entries refuse, and a misaligned image for the two 4-byte stems."""
from fractions import Fraction

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import rel_l2
from helpers import stem_u8_ref as R


def test_fma_normalise_is_the_exactly_rounded_fma_on_all_768_pairs():
    from test_stem_u8_cpu import fma_mirror
    a, b = R.fma_constants()
    u8 = torch.arange(256, dtype=torch.uint8).view(1, 1, 256, 1).expand(1, 1, 256, 3).contiguous()
    got = R.fma_normalise(u8).numpy()[0, :, 0, :]                       # [3][256]
    for c in range(3):
        fa, fb = Fraction(float(a[c])), Fraction(float(b[c]))
        for u in range(256):
            exact = u * fa + fb
            d = float(u) * float(a[c]) + float(b[c])
            assert Fraction(d) == exact, (c, u)                         # no rounding in float64: one rounding below
            assert got[c, u] == np.float32(d), (c, u)
        assert np.array_equal(got[c], fma_mirror(c)[1]), c
    # and it is not the loader's arithmetic (else the two references of the GPU test were one)
    assert not torch.equal(R.fma_normalise(u8), R.loader_normalise(u8))
    assert (R.fma_normalise(u8) - R.loader_normalise(u8)).abs().max() <= 2.0 ** -16


def test_case_makers():
    u8 = R.images(4, 9, 33, seed=3)
    assert u8.dtype == torch.uint8 and tuple(u8.shape) == (4, 9, 33, 3)
    assert int(u8[0, 0, :-1].max()) == 0 and int(u8[0, 1:-1, 0].max()) == 0        # (the 255 runs own the corners)
    assert int(u8[0, -1].min()) == 255 and int(u8[0, :, -1].min()) == 255
    assert len(torch.unique(u8[1:])) == 256
    f = R.flat(9, 33)
    x = R.fma_normalise(f)
    assert float(x[0].max()) < -100.0 and float(x[1].min()) > 100.0 and float(x[2].abs().max()) <= 0.5
    # the weights are the draws of test_vgg_stem_mx_fused (its generator draws x first)
    w1, b1, w2, b2 = R.weights(9, 33)
    g = torch.Generator().manual_seed(5 * 9 + 33)
    torch.randn((1, 3, 9, 33), generator=g)
    assert torch.equal(w1, torch.randn((64, 3, 3, 3), generator=g) * (2.0 / 27) ** 0.5)


@pytest.mark.parametrize("kind,shape", [("rand", s) for s in R.SHAPES] + [("flat", R.FLAT_SHAPE)],
                         ids=lambda v: v if isinstance(v, str) else "x".join(map(str, v)))
def test_the_emulation_alone_stays_far_inside_the_bars_of_the_gpu_test(kind, shape):
    r = R.reference(kind, shape)
    d = rel_l2(r["emul"], r["host"])
    err, ref = R.group_error(r["emul"], r["host"])
    ratio = float((err / (3e-4 * ref + 1e-6)).max())
    print(f"{kind} {shape}: emulation vs fp64 rel-L2 {d:.2e} (bar 6e-5); worst group err / (3e-4 ref + 1e-6) = "
          f"{ratio:.3f}; largest err / ref {float((err / (ref + 1e-9)).max()):.2e}")
    assert d < 6e-5
    assert (err <= 3e-4 * ref + 1e-6).all()
    # "far inside": the reference's own share of either bar is under a third
    assert d < 2e-5 and ratio < 1.0 / 3.0


def test_range_case_overflows_fp16_in_conv1_2_only():
    u8, w1, b1, w2, b2 = R.range_case()
    x = R.fma_normalise(u8).double()
    h1 = F.relu(F.conv2d(x, w1.double(), b1.double(), padding=1))
    y = R.host_stem(x, w1, b1, w2, b2)
    print(f"range case: conv1_1 max {float(h1.max()):.4g}, pooled conv1_2 max {float(y.max()):.4g} (fp16: 65504)")
    assert float(h1.max()) < 0.1 * 65504.0          # far from the bound: no rounding tips it
    assert float(y.max()) > 1.5 * 65504.0           # far beyond it
    # and the ordinary weights stay far inside on every case (the GPU test asserts a flag of 0 there)
    for kind, shape in [("rand", (4, 9, 33)), ("flat", R.FLAT_SHAPE)]:
        r = R.reference(kind, shape)
        assert float(r["host"].max()) < 0.1 * 65504.0


def test_the_stand_alone_entry_refuses_what_the_public_stem_entries_refuse():
    """Argument validation only: every call below returns OIBL_E_INVALID before any HIP call (the pointers are
    never followed), as tests/test_abi.py tests the public entries."""
    import ctypes as C
    from openibl_amd import lib, ops
    h = lib.debug_hooks()
    try:
        m3, s3 = (C.c_float * 3)(*R.MEAN), (C.c_float * 3)(*R.STD)
        P = 0x10000                       # "device pointers": 16-byte aligned, never dereferenced

        def call(x=P, N=1, H=8, W=32, w1=P, b1=P, w2=P, b2=P, precision=ops.BF16X3, act_scale=1.0, out=P, mean=m3):
            rc = h.oibl_debug_vgg16_stem_u8(x, N, H, W, C.cast(mean, C.c_void_p) if mean is not None else None,
                                            C.cast(s3, C.c_void_p), w1, b1, w2, b2, precision, act_scale, None, out,
                                            None)
            return rc, h.oibl_last_error().decode()
        for kw, word in [(dict(x=None), "null"), (dict(w2=None), "null"), (dict(out=None), "null"),
                         (dict(mean=None), "null"), (dict(N=0), "bad shape"), (dict(H=1), "bad shape"),
                         (dict(W=1), "bad shape"), (dict(W=2, precision=ops.F16MX), "bad shape"),
                         (dict(N=1 << 20, H=1 << 10, W=1 << 10), "exceeds"),
                         (dict(w2=P + 8), "16-byte"), (dict(out=P + 4), "16-byte"),
                         (dict(precision=ops.F32), "bad precision"), (dict(precision=7), "bad precision"),
                         (dict(act_scale=0.125), "act_scale"),
                         # the condition under which vgg_forward_impl takes the 4-byte uint8 stems at all
                         (dict(x=P + 1), "4-byte"), (dict(x=P + 2, precision=ops.F16MX), "4-byte"),
                         (dict(x=P + 3), "4-byte")]:
            rc, msg = call(**kw)
            assert rc == -1 and word in msg, (kw, rc, msg)
    finally:
        lib.use_product_library()


def test_only_the_debug_library_exports_the_stand_alone_entry():
    import subprocess
    from openibl_amd import build, lib
    build.build(verbose=False)        # (nothing to do when the in-tree libraries are current: tests/test_abi.py)

    def exported(path):
        out = subprocess.run(["nm", "-D", "--defined-only", str(path)], check=True, capture_output=True, text=True)
        return {ln.split()[-1] for ln in out.stdout.splitlines() if ln.strip()}
    assert "oibl_debug_vgg16_stem_u8" in exported(lib.debug_lib_path())
    assert "oibl_debug_vgg16_stem_u8" not in exported(lib.lib_path())
    assert "oibl_debug_vgg16_stem_u8" in lib._HOOKS and "oibl_debug_vgg16_stem_u8" not in lib._HOOK_DEFAULTS
