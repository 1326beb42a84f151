"""References and case makers for the three uint8 stems launched by csrc/stem.hip run alone (tests/test_gpu_stem_u8.py, and
tests/test_stem_u8_ref_cpu.py for what can be said without a GPU):

  * `fma_normalise`: the exact input of the bf16x3 / f16mx stems — ToTensor + Normalize as ONE fma per value,
    v = u * a_c + b_c with a_c = 1 / (255 std_c), b_c = -mean_c / std_c built as launch_vgg_stem_x3 builds them;
  * `loader_normalise`: (u / 255 - mean) / std in fp32, the loader's arithmetic and the bf16 stem's table;
  * `images`, `flat`, `weights`, `range_case`: seeded inputs;  `host_stem`, `reference`: the fp64 convolutions and
    the emulation of the f16mx arithmetic (helpers/mx_emul.stem), computed once per case and shared;
  * `run_stem_u8`: the debug library's oibl_debug_vgg16_stem_u8.

Test infrastructure only."""
import ctypes as C
import functools

import numpy as np
import torch
import torch.nn.functional as F

from helpers import mx_emul
from openibl_amd import ops

MEAN, STD = ops.REF_MEAN, ops.REF_STD

# (N, H, W).  A tile is 8 x 32 conv1_2 pixels; the f16mx grid is min(256, tiles), the bf16x3 grid min(128, tiles) x 2.
SHAPES = [(1, 8, 32),      # one full tile
          (4, 2, 3),       # the smallest f16mx input; image bases at 0, 2, 0, 2 mod 4
          (4, 3, 5),       # image bases at 0, 1, 2, 3 mod 4; 3 W mod 4 = 3
          (4, 5, 7),       # image bases at 0, 1, 2, 3 mod 4; 3 W mod 4 = 1
          (3, 7, 10),      # 3 W mod 4 = 2; bases at 0, 2, 0 mod 4
          (4, 9, 33),      # bases at 0, 3, 2, 1 mod 4; partial tiles right and bottom; 16 tiles: per-XCD tile ranges
          (1, 17, 65),     # pooling floors; 9 tiles: plain striding
          (5, 40, 136),    # 125 tiles: not a multiple of 8, below both grids
          (3, 72, 320)]    # 270 tiles: f16mx workgroups run up to two, bf16x3 up to three
FLAT_SHAPE = (3, 9, 33)


def fma_constants(mean=MEAN, std=STD):
    """(a, b) float32 [3], as launch_vgg_stem_x3 makes them: the caller's constants arrive as C floats, the quotients
    are taken in double and rounded to float once."""
    m = np.asarray(mean, dtype=np.float32).astype(np.float64)
    s = np.asarray(std, dtype=np.float32).astype(np.float64)
    return (1.0 / (255.0 * s)).astype(np.float32), (-m / s).astype(np.float32)


def fma_normalise(u8_nhwc, mean=MEAN, std=STD):
    """uint8 [N][H][W][3] -> float32 [N][3][H][W]: fmaf(u, a_c, b_c).  The float64 expression u * a + b is exact for
    the loader's constants (tests/test_stem_u8_ref_cpu.py, with rationals), so its one rounding is the fma's."""
    a, b = fma_constants(mean, std)
    u = torch.as_tensor(u8_nhwc).cpu().numpy().astype(np.float64)
    v = (u * a.astype(np.float64) + b.astype(np.float64)).astype(np.float32)
    return torch.from_numpy(np.ascontiguousarray(v.transpose(0, 3, 1, 2)))


def loader_normalise(u8_nhwc, mean=MEAN, std=STD):
    """uint8 [N][H][W][3] -> float32 [N][3][H][W]: (u / 255 - mean) / std, three rounded fp32 operations."""
    m = torch.tensor(mean, dtype=torch.float32).view(1, 3, 1, 1)
    s = torch.tensor(std, dtype=torch.float32).view(1, 3, 1, 1)
    u = torch.as_tensor(u8_nhwc).cpu().permute(0, 3, 1, 2).float()
    return ((u / 255.0 - m) / s).contiguous()


def images(N, H, W, seed):
    """Random bytes; image 0 carries runs of 0 on its top row and left column and of 255 on its bottom row and right
    column (padding is 0.0, not normalise(0); a neighbour's byte read as a tap is the largest there is)."""
    g = torch.Generator().manual_seed(seed)
    u8 = torch.randint(0, 256, (N, H, W, 3), generator=g, dtype=torch.uint8)
    u8[0, 0, :, :] = 0
    u8[0, :, 0, :] = 0
    u8[0, -1, :, :] = 255
    u8[0, :, -1, :] = 255
    return u8


def flat(H, W, mean=MEAN):
    """Three flat images: all 0 (normalises to about -124 per channel), all 255, all round(255 mean_c) (about 0)."""
    u8 = torch.zeros((3, H, W, 3), dtype=torch.uint8)
    u8[1] = 255
    u8[2] = torch.tensor([int(round(255.0 * m)) for m in mean], dtype=torch.uint8)
    return u8


def _case(N, H, W, cin, cout, seed):
    """The draw of tests/test_gpu_mx.py / tests/test_gpu_x3.py."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn((N, cin, H, W), generator=g)
    w = torch.randn((cout, cin, 3, 3), generator=g) * (2.0 / (9 * cin)) ** 0.5
    b = torch.randn((cout,), generator=g) * 0.1
    return x, w, b


def weights(H, W):
    """(w1, b1, w2, b2) as test_vgg_stem_mx_fused / test_vgg_stem_x3_fused draw them, by the same seeds rule: their
    bars are bars for these weights."""
    _, w1, b1 = _case(1, H, W, 3, 64, seed=5 * H + W)
    _, w2, b2 = _case(1, 4, 4, 64, 64, seed=H + 9 * W)
    return w1, b1, w2, b2


def host_stem(x_nchw, w1, b1, w2, b2, pool=True):
    """conv1_1 + ReLU + conv1_2 + ReLU (+ 2x2 max-pool) in fp64."""
    h1 = F.relu(F.conv2d(x_nchw.double(), w1.double(), b1.double(), padding=1))
    y = F.relu(F.conv2d(h1, w2.double(), b2.double(), padding=1))
    return F.max_pool2d(y, 2, 2) if pool else y


def make_case(kind, shape):
    """(u8, w1, b1, w2, b2) of a named case: kind "rand" = images(), "flat" = flat()."""
    N, H, W = shape
    if kind == "flat":
        assert N == 3
        u8 = flat(H, W)
    else:
        u8 = images(N, H, W, seed=1000 * N + 7 * H + W)
    return (u8,) + weights(H, W)


@functools.lru_cache(maxsize=None)
def reference(kind, shape):
    """dict(u8, w1, b1, w2, b2, x = fma_normalise(u8), host = fp64 stem of x, emul = mx_emul.stem of x), computed
    once per case and shared by the tests: treat it as read-only."""
    u8, w1, b1, w2, b2 = make_case(kind, shape)
    x = fma_normalise(u8)
    return dict(u8=u8, w1=w1, b1=b1, w2=w2, b2=b2, x=x, host=host_stem(x, w1, b1, w2, b2),
                emul=mx_emul.stem(x, w1, b1, w2, b2))


def group_error(got_nchw, want_nchw):
    """Per pixel and 32-channel group: (largest |error|, largest |want|), as test_vgg_stem_mx_fused takes them."""
    N = want_nchw.shape[0]
    err = (got_nchw.double() - want_nchw.double()).abs().reshape(N, 2, 32, -1).amax(2)
    ref = want_nchw.double().abs().reshape(N, 2, 32, -1).amax(2)
    return err, ref


# The range-flag case: the weights of test_range_flag_is_raised_as_by_the_16_wave_kernel (tests/test_gpu_stem_mx12.py:
# w1 = 0.2 randn, w2 = gain randn) for byte-range inputs.  That test feeds x = 1e4 randn with a conv1_2 gain of 0.2; a
# normalised byte has a standard deviation of 255 / sqrt(12) = 73.6, so the same products need 0.2 x 1e4 / 73.6 = 27.
RANGE_SHAPE = (1, 8, 32)
RANGE_W2_GAIN = 27.0


def range_case():
    """(u8, w1, b1, w2, b2) whose conv1_1 stays inside fp16 and whose conv1_2 passes 65504 (checked on the CPU in
    tests/test_stem_u8_ref_cpu.py against the fp64 convolutions)."""
    N, H, W = RANGE_SHAPE
    g = torch.Generator().manual_seed(7)
    u8 = torch.randint(0, 256, (N, H, W, 3), generator=g, dtype=torch.uint8)
    w1 = torch.randn((64, 3, 3, 3), generator=g) * 0.2
    b1 = torch.randn(64, generator=g) * 0.1
    w2 = torch.randn((64, 64, 3, 3), generator=g) * RANGE_W2_GAIN
    b2 = torch.randn(64, generator=g) * 0.1
    return u8, w1, b1, w2, b2


def run_stem_u8(dev, u8, precision, w1, b1, w2, b2, act_scale=1.0, flag=None, mean=MEAN, std=STD):
    """One uint8 stem alone, through oibl_debug_vgg16_stem_u8 of the debug library (the caller restores the product
    library: the suite's autouse fixture does).  u8: uint8 [N][H][W][3], on the host or — a view into a larger buffer,
    to choose its alignment — already on the device, contiguous.  w2 is packed here, in the precision's layout.
    Returns [N][H/2][W/2][64] in the route's container: bf16, or int32 (bf16x3 pairs / f16mx lines)."""
    from openibl_amd import lib
    p = ops.precision_code(precision)
    assert p in (ops.BF16, ops.BF16X3, ops.F16MX), precision
    x = u8 if u8.is_cuda else u8.to(dev)
    assert x.dtype == torch.uint8 and x.dim() == 4 and x.shape[3] == 3 and x.is_contiguous()
    N, H, W, _ = map(int, x.shape)
    w1d, b1d, b2d = w1.to(dev).contiguous(), b1.to(dev).contiguous(), b2.to(dev).contiguous()
    wp2 = ops.pack_conv3x3(w2.to(dev).contiguous(), precision)
    out = torch.empty((N, H // 2, W // 2, 64), dtype=torch.bfloat16 if p == ops.BF16 else torch.int32, device=dev)
    m3 = (C.c_float * 3)(*[float(v) for v in mean])
    s3 = (C.c_float * 3)(*[float(v) for v in std])
    hooks = lib.debug_hooks()
    rc = hooks.oibl_debug_vgg16_stem_u8(x.data_ptr(), N, H, W, C.cast(m3, C.c_void_p), C.cast(s3, C.c_void_p),
                                        w1d.data_ptr(), b1d.data_ptr(), wp2.data_ptr(), b2d.data_ptr(), p,
                                        float(act_scale), None if flag is None else flag.data_ptr(), out.data_ptr(),
                                        torch.cuda.current_stream(dev).cuda_stream)
    lib.check(rc, "debug_vgg16_stem_u8")
    torch.cuda.synchronize(dev)       # (the operands above die with this frame)
    return out
