"""The output BITS of the seven stem routes, pinned: sha256 of each route's raw output buffer on seeded inputs against
tests/golden/stem_lines.json, which was recorded on the MI355X from the commit in front of the split of csrc/stem.hip
into one header per kernel (helpers/make_stem_lines_golden.py: routes, shapes, inputs; never regenerated from the code
under test).  The stems' source may be rearranged; their lines may not move.

  bf16_f32, bf16_u8   vgg_stem_kernel<U8>       (csrc/stem_bf16.h)
  x3_f32, x3_u8       vgg_stem_x3_kernel<U8>    (csrc/stem_x3.h)
  mx12_f32            stem_mx12_kernel          (csrc/stem_mx12.h)
  mx16_f32, mx_u8     vgg_stem_mx_kernel<U8>    (csrc/stem_mx16.h)

The three f16mx routes also leave the range flag as recorded: 0 on every shape and on the quiet case, 1 where conv1_2
passes the fp16 bound (the magnitudes of tests/test_gpu_stem_mx12.py::test_range_flag_is_raised_as_by_the_16_wave_kernel)."""
import json

import pytest
import torch

from helpers import make_stem_lines_golden as G

pytestmark = pytest.mark.gpu

GOLDEN = json.loads(G.OUT.read_text())


def _id(v):
    return "x".join(map(str, v)) if isinstance(v, tuple) else v


@pytest.mark.parametrize("shape", G.SHAPES, ids=_id)
@pytest.mark.parametrize("route", G.ROUTES)
def test_lines_are_those_recorded(dev, route, shape):
    y, flag = G.run(dev, route, G.inputs(shape))
    N, H, W = shape
    assert tuple(y.shape) == (N, H // 2, W // 2, 64)
    assert int(y.view(torch.int16 if y.dtype == torch.bfloat16 else y.dtype).ne(0).sum()) > 0
    assert G.digest(y) == GOLDEN["lines"][G.key(route, shape)]
    if route in G.MX_ROUTES:
        assert flag == GOLDEN["flags"][G.key(route, shape)] == 0
    else:
        assert flag is None


@pytest.mark.parametrize("case,raised", [("quiet", 0), ("raised", 1)])
@pytest.mark.parametrize("route", G.MX_ROUTES)
def test_range_flag_is_left_as_recorded(dev, route, case, raised):
    """One input that raises the flag and one that does not, through every f16mx route: the flag and the (clamped)
    lines are the recorded ones."""
    y, flag = G.run(dev, route, G.inputs(G.FLAG_SHAPE, **G.FLAG_CASES[case]))
    assert GOLDEN["flags"][f"{route}/{case}"] == raised
    assert flag == raised
    assert G.digest(y) == GOLDEN["lines"][f"{route}/{case}"]
