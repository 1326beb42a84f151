"""Writes tests/golden/stem_lines.json: sha256 digests of the raw output buffers of the seven stem routes, and the
range flag the three f16mx routes leave, on seeded inputs.  The file pins the BITS of the stem kernels across a
rewrite of their source: it is recorded once, on the MI355X, from the commit in front of the rewrite, and never
regenerated from the code it judges (tests/test_gpu_stem_lines.py compares).

    python -m tests.helpers.make_stem_lines_golden [OUTPUT.json]

Routes (csrc/stem.hip, launch_vgg_stem / launch_vgg_stem_x3):
  bf16_f32, bf16_u8      the bf16 stem, float32 NCHW / uint8 NHWC input
  x3_f32, x3_u8          the bf16x3 stem, float32 NCHW / uint8 NHWC input
  mx12_f32               the 12-wave f16mx stem (the float32 route)
  mx16_f32               the 16-wave f16mx stem on float32 input (oibl_debug_set_stem_mx12(0))
  mx_u8                  the 16-wave f16mx stem on uint8 input
Inputs are drawn on the host with numpy.random.default_rng(seed): the float32 image, the uint8 image, w1, b1, w2,
b2; w2 is packed by ops.pack_conv3x3.  The uint8 f16mx route runs at act_scale = 1/8 (vgg_forward_impl's); the
float32 f16mx entry point takes no scale and runs at 1.  uint8 images start on a 4-byte boundary.

Test infrastructure only."""
import functools
import hashlib
import json
import sys
from pathlib import Path

import numpy as np
import torch

TESTS = Path(__file__).resolve().parent.parent
for _p in (TESTS, TESTS.parent):    # run as a script or as a module: `helpers` and `openibl_amd` resolve either way
    if str(_p) not in sys.path:
        sys.path.insert(0, str(_p))

from helpers import stem_u8_ref  # noqa: E402
from openibl_amd import lib, ops  # noqa: E402

OUT = TESTS / "golden" / "stem_lines.json"

ROUTES = ["bf16_f32", "bf16_u8", "x3_f32", "x3_u8", "mx12_f32", "mx16_f32", "mx_u8"]
MX_ROUTES = ["mx12_f32", "mx16_f32", "mx_u8"]
# (N, H, W).  A tile is 8 x 32 conv1_2 pixels.
SHAPES = [(1, 2, 3),       # the smallest f16mx accepts
          (2, 9, 33),      # odd sizes, every tile a border tile, two images
          (1, 26, 98),     # the smallest image with one interior tile (is_interior: H >= 26, W >= 98)
          (3, 40, 160),    # 75 tiles on 75 workgroups: plain striding (the grid is no multiple of 8), one tile each
          (4, 9, 33),      # 16 tiles on 16 workgroups: the per-XCD walk (gridDim.x & 7 == 0)
          (6, 72, 320)]    # 540 tiles on 256 (bf16x3: 128) workgroups: the per-XCD walk with three and more tiles per
                           # workgroup, so the gather runs two tiles ahead of the tile being multiplied
MX_ACT_SCALE = 2.0 ** -3
# The range flag: the magnitudes of tests/test_gpu_stem_mx12.py::test_range_flag_is_raised_as_by_the_16_wave_kernel —
# x = 1e4 randn against a conv1_2 gain of 0.2 (conv1_1 inside fp16, conv1_2 beyond it) — and, for bytes, the gain that
# gives the same products (helpers/stem_u8_ref.RANGE_W2_GAIN = 27 at scale 1, hence 27 / act_scale).
FLAG_SHAPE = (1, 8, 32)
FLAG_CASES = {"quiet": dict(x_gain=1.0, w2_gain=0.05, w2_gain_u8=0.05),
              "raised": dict(x_gain=1e4, w2_gain=0.2, w2_gain_u8=27.0 / MX_ACT_SCALE)}


def key(route, shape):
    return f"{route}/" + "x".join(map(str, shape))


@functools.lru_cache(maxsize=None)
def inputs(shape, x_gain=1.0, w2_gain=0.05, w2_gain_u8=0.05):
    """Host tensors of one case, drawn once and shared by the routes: treat them as read-only."""
    N, H, W = shape
    rng = np.random.default_rng(1000 * N + 7 * H + W)
    f32 = lambda *s: rng.standard_normal(s, dtype=np.float32)
    x = f32(N, 3, H, W) * np.float32(x_gain)
    u8 = rng.integers(0, 256, (N, H, W, 3), dtype=np.uint8)
    w1, b1 = f32(64, 3, 3, 3) * np.float32(0.2), f32(64) * np.float32(0.1)
    w2, b2 = f32(64, 64, 3, 3), f32(64) * np.float32(0.1)
    t = torch.from_numpy
    return dict(x=t(x), u8=t(u8), w1=t(w1), b1=t(b1), w2=t(w2 * np.float32(w2_gain)),
                w2_u8=t(w2 * np.float32(w2_gain_u8)), b2=t(b2))


def run(dev, route, c):
    """(raw output tensor, range flag or None) of one route on the case c = inputs(...)."""
    w1, b1, b2 = c["w1"].to(dev), c["b1"].to(dev), c["b2"].to(dev)
    if route in ("bf16_u8", "x3_u8", "mx_u8"):
        prec = {"bf16_u8": "bf16", "x3_u8": "bf16x3", "mx_u8": "f16mx"}[route]
        u8 = c["u8"].to(dev)
        assert u8.data_ptr() % 4 == 0 and u8.is_contiguous()
        flag = ops.new_range_flag(dev) if route == "mx_u8" else None
        y = stem_u8_ref.run_stem_u8(dev, u8, prec, c["w1"], c["b1"], c["w2_u8"], c["b2"],
                                    act_scale=MX_ACT_SCALE if route == "mx_u8" else 1.0, flag=flag)
        return y, None if flag is None else int(flag.item())
    x = c["x"].to(dev)
    if route == "bf16_f32":
        return ops.vgg16_stem(x, w1, b1, ops.pack_conv3x3(c["w2"].to(dev), "bf16"), b2), None
    if route == "x3_f32":
        return ops.vgg16_stem_x3(x, w1, b1, ops.pack_conv3x3(c["w2"].to(dev), "bf16x3"), b2), None
    waves = {"mx12_f32": 12, "mx16_f32": 16}[route]
    hooks = lib.debug_hooks()
    flag = ops.new_range_flag(dev)
    assert hooks.oibl_debug_set_stem_mx12(1 if waves == 12 else 0) == 0
    assert hooks.oibl_debug_set_stem_mx_flag(flag.data_ptr()) == 0
    try:
        y = ops.vgg16_stem_mx(x, w1, b1, ops.pack_conv3x3(c["w2"].to(dev), "f16mx"), b2)
        torch.cuda.synchronize(dev)
        assert hooks.oibl_debug_last_stem_mx_route() == waves
    finally:
        hooks.oibl_debug_set_stem_mx_flag(None)
        hooks.oibl_debug_set_stem_mx12(1)
    return y, int(flag.item())


def digest(y):
    """sha256 of the output buffer's bytes."""
    raw = y.contiguous().view(torch.int16 if y.dtype == torch.bfloat16 else y.dtype).cpu().numpy()
    return hashlib.sha256(raw.tobytes()).hexdigest()


def main():
    dev = torch.device("cuda", 0)
    lines, flags = {}, {}
    for shape in SHAPES:
        for route in ROUTES:
            y, flag = run(dev, route, inputs(shape))
            N, H, W = shape
            assert tuple(y.shape) == (N, H // 2, W // 2, 64)
            lines[key(route, shape)] = digest(y)
            if flag is not None:
                flags[key(route, shape)] = flag
    for name, gains in FLAG_CASES.items():
        for route in MX_ROUTES:
            y, flag = run(dev, route, inputs(FLAG_SHAPE, **gains))
            lines[f"{route}/{name}"] = digest(y)
            flags[f"{route}/{name}"] = flag
    lib.use_product_library()
    out = Path(sys.argv[1]) if len(sys.argv) > 1 else OUT
    out.write_text(json.dumps({"lines": lines, "flags": flags}, indent=1, sort_keys=True) + "\n")
    print(f"wrote {out} ({out.stat().st_size} bytes)")
    print(json.dumps(flags, sort_keys=True))


if __name__ == "__main__":
    main()
