"""The three uint8 stems launched by csrc/stem.hip run ALONE (oibl_debug_vgg16_stem_u8 of the debug library), not judged twelve
layers later as tests/test_gpu_u8.py and tests/test_gpu_descriptor.py judge them:

  bf16    vgg_stem_kernel<true>     (stem_bf16.h)  3 x 257 table of bf16((u / 255 - mean) / std)
  bf16x3  vgg_stem_x3_kernel<true>  (stem_x3.h)    v = fmaf(u, a_c, b_c), 12-byte dword-aligned gathers, K order (ky, kx, c)
  f16mx   vgg_stem_mx_kernel<true>  (stem_mx16.h)  the same producers (stem_parts.h) in front of the f16mx consumers

against the emulation of their arithmetic and the fp64 convolutions of the exact input (tests/helpers/stem_u8_ref.py;
the references alone are held to the same bars in tests/test_stem_u8_ref_cpu.py), and bit for bit against themselves:
an image's lines depend neither on the image's base alignment, nor on its batch mates, nor on the bytes around the
tensor.  Shapes: helpers/stem_u8_ref.SHAPES (every (base mod 4, 3 W mod 4) combination, partial tiles, both tile
dealing schemes, several tiles per workgroup).

Measured on an MI355X over those nine shapes and the flat case (the figures the bars are to be read against):
  A  f16mx vs the emulation of its arithmetic: rel-L2 3.2e-6 .. 4.4e-6 (flat: 1.1e-6; bar 1e-5), the same at
     act_scale 1 and 2^-3; vs fp64: 1.32e-5 .. 1.51e-5 (flat: 1.60e-5; bar 6e-5) — the emulation's own 1.32e-5 ..
     1.50e-5; largest group err / ref 4.1e-5 (bar 3e-4).
  B  bf16x3 vs fp64: rel-L2 5.1e-6 .. 5.7e-6 (bar 3e-5).  Against the float32-input route, per pixel, max |diff| /
     amax of the pixel's 64 channels, in the order of SHAPES: 1.15e-5, 5.69e-6, 4.81e-6, 1.27e-5, 1.17e-5, 1.45e-5,
     9.36e-6, 1.51e-5, 1.52e-5, flat 4.79e-6 (rel-L2 of the two maps: 1.0e-6 .. 1.6e-6, flat 1.9e-7).
     X3_ROUTE_BAR = 4 x 1.52e-5.  The largest values sit at 2^-16 = 1.526e-5 and do not grow with the shape: they are
     ONE unit of the output element's lo part.  conv1_1's sums differ between the routes in their last fp32 bits; where
     such a sum — or a conv1_2 sum built on it — lies at a rounding boundary of its lo part (bf16(v - hi), 8
     significant bits under hi's 8), lo moves by one unit, 2^-16 of an element whose significand is near 1, and when
     that element is the pixel's largest the figure is 2^-16 of the amax.  The maps as a whole are 1e-6 apart, a
     quarter of either route's distance to fp64."""
import pytest
import torch

from conftest import rel_l2
from helpers import stem_u8_ref as R
from openibl_amd import lib, ops, synth

pytestmark = pytest.mark.gpu

TOL_STEM_EMUL = 1e-5     # tests/test_gpu_mx.py: the float32-input f16mx stem against the same emulation
TOL_MX_HOST = 6e-5       # test_vgg_stem_mx_fused
TOL_X3_HOST = 3e-5       # test_vgg_stem_x3_fused
# bf16x3, uint8 route against the float32-input route on the same values, per output pixel: the two evaluate the same
# sums and differ in conv1_1's accumulation order ((ky, kx, c) against (c, ky, kx)) — order noise of 81 fp32 products
# seen through two 16-bit roundings.  Four times the largest value measured over the shape list (1.52e-5 = one unit
# of an output element's lo part, 2^-16: module docstring); a wrong tap is orders of magnitude larger.
X3_ROUTE_BAR = 4 * 1.52e-5
MX_ACT_SCALE = 2.0 ** -3  # vgg_forward_impl's activation scale (g_mx_act_shift = 3): exact in every format here

PRECISIONS = ["bf16", "bf16x3", "f16mx"]
CASES = [("rand", s) for s in R.SHAPES] + [("flat", R.FLAT_SHAPE)]   # F: the flat batch goes through A and B


def _id(v):
    return v if isinstance(v, str) else "x".join(map(str, v)) if isinstance(v, tuple) else None


def _run(dev, u8, precision, w, flag=None, act_scale=None):
    """One stem on u8 (host tensor, or a contiguous device view) with the weights w = (w1, b1, w2, b2); f16mx at the
    production activation scale unless told otherwise."""
    if act_scale is None:
        act_scale = MX_ACT_SCALE if precision == "f16mx" else 1.0
    return R.run_stem_u8(dev, u8, precision, *w, act_scale=act_scale, flag=flag)


def _nchw(y, precision):
    """The values a stem's output carries: float32 NCHW on the host."""
    if precision == "bf16":
        return y.float().permute(0, 3, 1, 2).contiguous().cpu()
    return ops.nhwc_to_nchw_f32(ops.x3_join(y) if precision == "bf16x3" else ops.mx_join(y, 0)).cpu()


def _weights_of(r):
    return r["w1"], r["b1"], r["w2"], r["b2"]


# ---- A (and F, G): f16mx against its own arithmetic ------------------------------------------------------------
@pytest.mark.parametrize("act_scale", [1.0, MX_ACT_SCALE], ids=["scale1", "scale2^-3"])
@pytest.mark.parametrize("kind,shape", CASES, ids=_id)
def test_f16mx_lines_against_the_emulation_and_fp64(dev, kind, shape, act_scale):
    """The lines of vgg_stem_mx_kernel<true> carry what helpers/mx_emul.stem computes from fma_normalise(u8) —
    the bar of the float32 route against the same emulation — and lie within the bars of test_vgg_stem_mx_fused of the
    fp64 convolutions; they are well-formed lines; the range flag stays 0.  At the production activation scale 2^-3
    (conv1_1's weights and both biases scaled, every line stored scaled) the joined lines times 8 meet the same bars.
    Flat images: padding is 0.0, not normalise(0) = -124 — a padded tap read as a byte fails by far."""
    r = R.reference(kind, shape)
    N, H, W = shape
    flag = ops.new_range_flag(dev)
    y = _run(dev, r["u8"], "f16mx", _weights_of(r), flag=flag, act_scale=act_scale)
    assert tuple(y.shape) == (N, H // 2, W // 2, 64) and y.dtype == torch.int32
    got = _nchw(y, "f16mx").double() / act_scale
    d_emul, d_host = rel_l2(got, r["emul"]), rel_l2(got, r["host"])
    err, ref = R.group_error(got, r["host"])
    print(f"f16mx u8 stem {kind} {shape} act_scale {act_scale:g}: rel-L2 vs emulation {d_emul:.2e} (bar {TOL_STEM_EMUL:g}), "
          f"vs fp64 {d_host:.2e} (bar {TOL_MX_HOST:g}), largest group err / ref {float((err / (ref + 1e-9)).max()):.2e}, "
          f"flag {int(flag.item())}")
    assert torch.isfinite(got).all()
    assert d_emul <= TOL_STEM_EMUL
    assert d_host <= TOL_MX_HOST
    assert (err <= 3e-4 * ref + 1e-6).all(), float((err / (ref + 1e-9)).max())
    # the stored lines against the format: what mx_split makes of their own fp16 parts, |q6(lo)| inside half an
    # fp16 ulp of the group's largest element
    hi = ops.mx_join(y, 1)
    again = ops.mx_split(hi)
    assert torch.equal(ops.mx_join(again, 1), hi)
    assert torch.equal(ops.mx_join(again, 2), ops.mx_join(y, 2))
    gmax = hi.abs().reshape(-1, 32).amax(-1, keepdim=True)
    lo6 = ops.mx_join(y, 3).reshape(-1, 32)
    assert (lo6.abs() <= gmax * 2.0 ** -11 * 1.07 + 1e-30).all()
    assert int(flag.item()) == 0


# ---- B (and F): bf16x3 ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,shape", CASES, ids=_id)
def test_bf16x3_against_fp64_and_the_float32_route(dev, kind, shape):
    """vgg_stem_x3_kernel<true> against the fp64 convolutions of fma_normalise(u8) (the bar of
    test_vgg_stem_x3_fused), and per output pixel against ops.vgg16_stem_x3 on fma_normalise(u8): the same sums in
    another order inside conv1_1.  Measured values: module docstring."""
    r = R.reference(kind, shape)
    N, H, W = shape
    w = _weights_of(r)
    y = _run(dev, r["u8"], "bf16x3", w)
    assert tuple(y.shape) == (N, H // 2, W // 2, 64) and y.dtype == torch.int32
    route = ops.vgg16_stem_x3(r["x"].to(dev), w[0].to(dev), w[1].to(dev), ops.pack_conv3x3(w[2].to(dev), "bf16x3"),
                              w[3].to(dev))
    a, b = ops.x3_join(y).double(), ops.x3_join(route).double()
    per_pixel = float(((a - b).abs().amax(-1) / b.abs().amax(-1).clamp_min(1e-30)).max())
    d_host = rel_l2(_nchw(y, "bf16x3"), r["host"])
    print(f"bf16x3 u8 stem {kind} {shape}: rel-L2 vs fp64 {d_host:.2e} (bar {TOL_X3_HOST:g}); vs the float32 route, "
          f"per pixel max |diff| / amax {per_pixel:.2e} (bar {X3_ROUTE_BAR:g}), rel-L2 {rel_l2(a, b):.2e}")
    assert torch.isfinite(a).all()
    assert d_host <= TOL_X3_HOST
    assert per_pixel <= X3_ROUTE_BAR


# ---- C: bf16 is bit-identical to the float32 route ------------------------------------------------------------------
@pytest.mark.parametrize("kind,shape", CASES, ids=_id)
def test_bf16_is_bit_identical_to_the_normalised_input_at_any_alignment(dev, kind, shape):
    """vgg_stem_kernel<true> looks bf16((u / 255 - mean) / std) up in a table: the claim in front of the kernel is
    "bit-identical to feeding the normalised fp32 tensor".  It reads bytes, and vgg_forward_impl hands it any
    alignment: the same batch as an odd-offset slice of a larger buffer."""
    r = R.reference(kind, shape)
    w = _weights_of(r)
    want = ops.vgg16_stem(R.loader_normalise(r["u8"]).to(dev), w[0].to(dev), w[1].to(dev),
                          ops.pack_conv3x3(w[2].to(dev), "bf16"), w[3].to(dev))
    assert int(want.float().ne(0).sum()) > 0
    assert torch.equal(_run(dev, r["u8"], "bf16", w), want)
    n = r["u8"].numel()
    for off in (1, 2, 3):
        buf = torch.full((n + 8,), 0x5A, dtype=torch.uint8, device=dev)
        view = buf[off:off + n].view(r["u8"].shape)
        view.copy_(r["u8"].to(dev))
        assert view.data_ptr() % 4 == off and view.is_contiguous()
        assert torch.equal(_run(dev, view, "bf16", w), want), off


# ---- D: an image does not depend on where it lies or on who lies beside it ------------------------------------------
D_SHAPES = [(4, 2, 3), (4, 3, 5), (4, 5, 7), (3, 7, 10), (4, 9, 33), (4, 17, 65)]


@pytest.mark.parametrize("neighbours", ["random", "255"])
@pytest.mark.parametrize("shape", D_SHAPES, ids=_id)
@pytest.mark.parametrize("precision", PRECISIONS)
def test_an_image_depends_neither_on_its_base_nor_on_its_batch_mates(dev, precision, shape, neighbours):
    """Image i of a batch (its first byte at i * 3 H W mod 4, its edges against other images' bytes) == the same image
    run alone with N = 1 at an aligned base, bit for bit.  "255": every other image is all 255, so a masked tap at
    an image's edge holds the largest byte there is instead of the zero an out-of-range load returns."""
    N, H, W = shape
    u8 = R.images(N, H, W, seed=31 * H + W)
    w = R.weights(H, W)
    alone = [_run(dev, u8[i:i + 1].contiguous(), precision, w) for i in range(N)]
    assert all(int(a.ne(0).sum()) > 0 for a in alone)
    if neighbours == "random":
        batch = _run(dev, u8, precision, w)
        for i in range(N):
            assert torch.equal(batch[i], alone[i][0]), i
    else:
        for i in range(N):
            mates = torch.full_like(u8, 255)
            mates[i] = u8[i]
            assert torch.equal(_run(dev, mates, precision, w)[i], alone[i][0]), i


# ---- E: bytes behind and in front of the tensor ---------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(1, 3, 5), (3, 5, 7), (1, 9, 33)], ids=_id)
@pytest.mark.parametrize("precision", PRECISIONS)
def test_bytes_around_the_tensor_do_not_matter(dev, precision, shape):
    """Byte counts that are no multiple of 4 (45, 315, 891): the 4-byte stems' descriptor is rounded up to whole
    dwords and their first window starts in front of the tensor.  The batch at a 4-byte aligned offset inside a
    larger buffer, guards of at least 3 (W + 1) + 4 bytes on either side filled with 0x00 and with 0xFF: the same
    bits as on a tensor of its own."""
    N, H, W = shape
    u8 = R.images(N, H, W, seed=17 * H + W)
    w = R.weights(H, W)
    n = u8.numel()
    assert n % 4 != 0
    guard = (3 * (W + 1) + 4 + 3) // 4 * 4
    tight = _run(dev, u8, precision, w)
    assert int(tight.ne(0).sum()) > 0
    for fill in (0x00, 0xFF):
        buf = torch.full((guard + n + guard + 4,), fill, dtype=torch.uint8, device=dev)
        view = buf[guard:guard + n].view(u8.shape)
        view.copy_(u8.to(dev))
        assert view.data_ptr() % 4 == 0
        assert torch.equal(_run(dev, view, precision, w), tight), hex(fill)


# ---- G: the range flag ----------------------------------------------------------------------------------------------
def test_range_flag_is_raised_as_by_the_float32_route(dev):
    """conv1_1 stays inside fp16, conv1_2 passes 65504 (helpers/stem_u8_ref.range_case, checked on the CPU): the uint8
    f16mx stem raises its flag, and so does ops.vgg16_stem_mx on fma_normalise(u8).  Flags only: the two routes' lines
    differ by conv1_1's K order."""
    u8, w1, b1, w2, b2 = R.range_case()
    flag = ops.new_range_flag(dev)
    y = R.run_stem_u8(dev, u8, "f16mx", w1, b1, w2, b2, act_scale=1.0, flag=flag)
    assert torch.isfinite(ops.mx_join(y, 0)).all()
    hooks = lib.debug_hooks()
    flag32 = ops.new_range_flag(dev)
    assert hooks.oibl_debug_set_stem_mx_flag(flag32.data_ptr()) == 0
    try:
        ops.vgg16_stem_mx(R.fma_normalise(u8).to(dev), w1.to(dev), b1.to(dev), ops.pack_conv3x3(w2.to(dev), "f16mx"),
                          b2.to(dev))
        torch.cuda.synchronize(dev)
    finally:
        hooks.oibl_debug_set_stem_mx_flag(None)
    assert int(flag.item()) == 1 and int(flag32.item()) == 1


# ---- H: two runs are bit-identical ----------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", PRECISIONS)
def test_two_runs_are_bit_identical(dev, precision):
    """(3, 72, 320): 270 tiles, several per workgroup in every kernel."""
    r = R.reference("rand", (3, 72, 320))
    x = r["u8"].to(dev)
    first = _run(dev, x, precision, _weights_of(r))
    assert int(first.ne(0).sum()) > 0
    assert torch.equal(_run(dev, x, precision, _weights_of(r)), first)


# ---- I: the misaligned fallback of the public entry -----------------------------------------------------------------
@pytest.mark.parametrize("precision,tol", [("bf16x3", 3e-5), ("f16mx", 6e-5)])
def test_misaligned_uint8_input_takes_the_normalising_pass(dev, state_dict, precision, tol):
    """vgg_forward_impl sends a uint8 image that does not start on a 4-byte boundary through the normalising pass
    (the 4-byte stems fetch aligned dwords): ops.vgg16_conv5 on an odd-offset slice == the aligned copy with the fused
    uint8 stem switched off (both normalise, then run the float32 stem), and within the bars of
    tests/test_gpu_u8.py of the aligned copy on the fused uint8 stem."""
    ws = [state_dict[f"base_model.base.{i}.weight"].to(dev) for i in synth.CONV_IDX]
    bs = [state_dict[f"base_model.base.{i}.bias"].to(dev) for i in synth.CONV_IDX]
    packed = [ws[0]] + [ops.pack_conv3x3(w, precision) for w in ws[1:]]
    u8 = R.images(1, 64, 96, seed=5).to(dev)
    buf = torch.zeros(u8.numel() + 8, dtype=torch.uint8, device=dev)
    odd = buf[1:1 + u8.numel()].view(u8.shape)
    odd.copy_(u8)
    assert u8.data_ptr() % 4 == 0 and odd.data_ptr() % 4 == 1 and odd.is_contiguous()
    fused = ops.vgg16_conv5(u8, packed, bs, precision).clone()
    got = ops.vgg16_conv5(odd, packed, bs, precision).clone()
    hooks = lib.debug_hooks()
    assert hooks.oibl_debug_set_stem_u8(0) == 0
    try:
        passed = ops.vgg16_conv5(u8, packed, bs, precision).clone()
    finally:
        hooks.oibl_debug_set_stem_u8(1)
    d = rel_l2(got.float().cpu(), fused.float().cpu())
    print(f"{precision}: conv5_3 map of a misaligned uint8 image vs the fused uint8 stem: rel-L2 {d:.2e} (bar {tol:g})")
    assert int(got.ne(0).sum()) > 0
    assert torch.equal(got, passed)
    assert 0.0 < d < tol       # (0 would mean the slice took the fused stem after all: its fma is not the pass's arithmetic)
