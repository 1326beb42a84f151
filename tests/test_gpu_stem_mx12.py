"""The 12-wave f16mx stem (csrc/stem_mx12.h: 64 output channels x 64 pixels per consumer wave, weights refilled by
tap group) against the 16-wave kernel it replaces on the float32-input route (vgg_stem_mx_kernel<false> of csrc/stem_mx16.h, selected by
the debug library's oibl_debug_set_stem_mx12(0)): the same seeded inputs through both, the raw int32 lines compared
with torch.equal — every output element accumulates the same products in the same order, so nothing may differ —
and the range flag raised by exactly the same inputs (oibl_debug_set_stem_mx_flag hands the entry point a flag)."""
import pytest
import torch

from openibl_amd import lib, ops

pytestmark = pytest.mark.gpu


def _inputs(dev, shape, seed, x_gain=1.0, w2_gain=0.05):
    g = torch.Generator().manual_seed(seed)
    N, H, W = shape
    x = torch.randn((N, 3, H, W), generator=g) * x_gain
    w1 = torch.randn((64, 3, 3, 3), generator=g) * 0.2
    b1 = torch.randn(64, generator=g) * 0.1
    w2 = torch.randn((64, 64, 3, 3), generator=g) * w2_gain
    b2 = torch.randn(64, generator=g) * 0.1
    return x.to(dev), w1.to(dev), b1.to(dev), ops.pack_conv3x3(w2.to(dev), "f16mx"), b2.to(dev)


def _both(dev, args):
    """(lines, flag) of the 12-wave kernel and of the 16-wave kernel on the same inputs."""
    hooks = lib.debug_hooks()
    out = []
    for mx12 in (1, 0):
        flag = ops.new_range_flag(dev)
        assert hooks.oibl_debug_set_stem_mx12(mx12) == 0
        assert hooks.oibl_debug_set_stem_mx_flag(flag.data_ptr()) == 0
        try:
            lines = ops.vgg16_stem_mx(*args)
            torch.cuda.synchronize(dev)
            # the comparison is only worth what the hook is: the library reports which kernel it launched
            assert hooks.oibl_debug_last_stem_mx_route() == (12 if mx12 else 16)
        finally:
            hooks.oibl_debug_set_stem_mx_flag(None)
            hooks.oibl_debug_set_stem_mx12(1)
        out.append((lines, int(flag.item())))
    return out


# (1, 8, 32): one full tile, first.  (1, 2, 3), (2, 3, 4): less than a tile, odd sizes.  (2, 9, 33), (1, 17, 65):
# partial tiles on the right and bottom edges, pooling floors.  (3, 72, 320): 270 tiles on at most 256 persistent
# workgroups — some run two, so the weight refill wraps from a tile's last stage into the next tile's first.
# (6, 72, 320): 540 tiles, three per workgroup for some.  (6, 77, 320): 600 tiles, three per workgroup for some AND a
# partial bottom tile row (H % 8 = 5: halo rows 6-9, so blocks 7-10 of those tiles lie wholly outside the image) — the
# gathers of such a tile go out behind the weight refill and must not be counted past by the streaming waves' END wait.
@pytest.mark.parametrize("shape", [(1, 8, 32), (1, 2, 3), (2, 3, 4), (2, 9, 33), (1, 17, 65), (3, 72, 320),
                                   (6, 72, 320), (6, 77, 320)])
def test_lines_are_those_of_the_16_wave_kernel(dev, shape):
    (new, nflag), (old, oflag) = _both(dev, _inputs(dev, shape, seed=sum(shape)))
    N, H, W = shape
    assert new.shape == old.shape == (N, H // 2, W // 2, 64) and new.dtype == torch.int32
    assert int(old.ne(0).sum()) > 0 or H // 2 == 0 or W // 2 == 0
    assert torch.equal(new, old)
    assert nflag == oflag == 0


def test_range_flag_is_raised_as_by_the_16_wave_kernel(dev):
    """conv1_1 stays inside fp16 (27 products of ~1e4 x 0.2), conv1_2 does not (576 products of ~1e4 x 0.2): both
    kernels clamp the same elements at the fp16 bound, pack the same lines and raise the flag."""
    args = _inputs(dev, (1, 8, 32), seed=7, x_gain=1e4, w2_gain=0.2)
    (new, nflag), (old, oflag) = _both(dev, args)
    assert oflag == 1 and nflag == 1
    assert torch.equal(new, old)
