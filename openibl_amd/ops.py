"""Torch-facing wrappers over the C ABI: tensors in, tensors out, device pointers across.

PyTorch is used only for device memory, streams and dtype bookkeeping; every computation below is
a call into libopenibl_amd.so.  All tensors must live on a CUDA(HIP) device and be contiguous.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional, Sequence, Tuple

import torch

from . import lib as _lib

BF16 = 0
F32 = 1
BF16X3 = 2   # split bf16: (hi, lo) operand pairs, three MFMAs per product, fp32-class results
F16MX = 3    # fp16 main term + MX-fp6 cross terms: 1e-4-class results at half the matrix time of bf16x3
F16R = 4     # matching only (top-k entry points): fp16 filter pass + exact rescoring from the fp32 rows — fp32-exact
             # lists at the cost of a 2-byte operand stream (csrc/match_f16r.h); not a backbone / matrix arithmetic
# element containers: bf16x3 / f16mx activations and packed weights are opaque 4-byte elements (128-byte
# groups of 32 elements, see x3_split / mx_split) carried in int32 tensors of the logical shape
_DTYPES = {BF16: torch.bfloat16, F32: torch.float32, BF16X3: torch.int32, F16MX: torch.int32}
_NAMES = {"bf16": BF16, "bfloat16": BF16, "fp32": F32, "f32": F32, "float32": F32,
          "bf16x3": BF16X3, "x3": BF16X3, "f16mx": F16MX, "mx": F16MX, "f16r": F16R}


def precision_code(p) -> int:
    if isinstance(p, str):
        try:
            return _NAMES[p.lower()]
        except KeyError:
            raise ValueError(f"unknown precision {p!r} (use 'bf16', 'f16mx', 'bf16x3' or 'fp32')")
    if p in (BF16, F32, BF16X3, F16MX, F16R):
        return int(p)
    raise ValueError(f"unknown precision {p!r}")


F16R_MAX_FUSED_K = 496      # the fused f16r path: a member window of 2k + 32 <= 1024 slots (csrc/match.hip, f16r_plan)


def topk_precision(precision, storage_dtype=torch.float32, k: int = 10) -> int:
    """The arithmetic the fused distance + top-k of a model precision runs in: an f16mx model's descriptors are
    matched in f16r — fp16 filter pass + exact rescoring from the stored rows: fp32-exact lists, and faster than
    contracting every pair in f16mx — whatever their storage type (float32, float16, bfloat16: a 16-bit row is
    widened exactly) and for every ranked prefix the reference reads (Recall@1/5/10, and the 120 ranks of spatial
    NMS, ibl/evaluators.py:152-153); everything else as asked."""
    p = precision_code(precision)
    if p == F16MX and storage_dtype in (torch.float32, torch.float16, torch.bfloat16) and k <= F16R_MAX_FUSED_K:
        return F16R
    return p


def head_precision(p) -> int:
    """Precision of the small contractions behind the backbone (NetVLAD assignment, PCA): bf16x3
    runs them in exact fp32 — they are HBM / latency bound there (the PCA streams its weight once
    per batch), so splitting the operands would buy nothing."""
    p = precision_code(p)
    return F32 if p in (BF16X3, F16MX) else p


def elem_dtype(p) -> torch.dtype:
    return _DTYPES[precision_code(p)]


def _need_cuda(*tensors: torch.Tensor) -> torch.device:
    dev = None
    for t in tensors:
        if t is None:
            continue
        if not t.is_cuda:
            raise _lib.OpenIBLAmdError(
                "openibl_amd: tensor is on %s; this path runs only on an AMD GPU through the HIP "
                "extension (there is no CPU fallback)" % t.device)
        if not t.is_contiguous():
            raise ValueError("openibl_amd: tensors must be contiguous")
        if dev is None:
            dev = t.device
        elif t.device != dev:
            raise ValueError("openibl_amd: tensors on different devices")
    return dev


def _stream(dev: torch.device) -> int:
    return torch.cuda.current_stream(dev).cuda_stream


def _ptr(t: Optional[torch.Tensor]):
    return None if t is None else t.data_ptr()


_WS = {}


def workspace(nbytes: int, dev: torch.device, slot: str = "default") -> torch.Tensor:
    """Grow-only per-(device, stream, slot) scratch buffer (torch allocations are 512-B aligned)."""
    key = (dev.index, _stream(dev), slot)
    buf = _WS.get(key)
    if buf is None or buf.numel() < nbytes:
        buf = torch.empty(max(int(nbytes), 256), dtype=torch.uint8, device=dev)
        _WS[key] = buf
    return buf


def release_workspaces() -> None:
    _WS.clear()


def workspaces_snapshot():
    """The scratch buffers currently alive (a captured hipGraph keeps those it recorded referenced:
    the grow-only buffers are replaced, not resized, when a later call needs more)."""
    return list(_WS.values())


# ---------------------------------------------------------------------------------------------
def cast(x: torch.Tensor, precision) -> torch.Tensor:
    """fp32 tensor -> tensor of the precision's element type (bf16 round-to-nearest-even)."""
    p = head_precision(precision)
    dev = _need_cuda(x)
    if x.dtype != torch.float32:
        raise ValueError("cast expects float32 input")
    if p == F32:
        return x
    out = torch.empty(x.shape, dtype=torch.bfloat16, device=dev)
    _lib.check(_lib.load().oibl_cast_f32_to_bf16(_ptr(x), _ptr(out), x.numel(), _stream(dev)),
               "cast_f32_to_bf16")
    return out


def to_f32(x: torch.Tensor) -> torch.Tensor:
    dev = _need_cuda(x)
    if x.dtype == torch.float32:
        return x
    if x.dtype != torch.bfloat16:
        raise ValueError("to_f32 expects bf16 or fp32")
    out = torch.empty(x.shape, dtype=torch.float32, device=dev)
    _lib.check(_lib.load().oibl_cast_bf16_to_f32(_ptr(x), _ptr(out), x.numel(), _stream(dev)),
               "cast_bf16_to_f32")
    return out


def x3_split(x: torch.Tensor) -> torch.Tensor:
    """float32 [..., C] (C % 32 == 0) -> the bf16x3 operand layout (int32 container, same shape):
    per row, C/32 groups of [32 x hi | 32 x lo] with hi = bf16(v), lo = bf16(v - hi)."""
    dev = _need_cuda(x)
    if x.dtype != torch.float32 or x.dim() < 1 or x.shape[-1] % 32 != 0:
        raise ValueError("x3_split expects a float32 tensor whose last dimension is a multiple of 32")
    out = torch.empty(x.shape, dtype=torch.int32, device=dev)
    C_ = int(x.shape[-1])
    _lib.check(_lib.load().oibl_x3_split_rows(_ptr(x), _ptr(out), x.numel() // C_, C_, _stream(dev)),
               "x3_split_rows")
    return out


def new_range_flag(dev: torch.device) -> torch.Tensor:
    """A cleared f16mx range flag (int32 [1] on the device): producers of f16mx lines set it to 1 when they
    meet a value beyond fp16 (|v| > 65504), see include/openibl_amd.h, OIBL_F16MX."""
    return torch.zeros(1, dtype=torch.int32, device=dev)


def mx_split(x: torch.Tensor, range_flag: Optional[torch.Tensor] = None) -> torch.Tensor:
    """float32 [..., C] (C % 32 == 0) -> the f16mx operand layout (int32 container, same shape): per 32
    elements one 128-byte line [32 fp16 | e2m3 images of hi and lo + their scale bytes].  range_flag: optional
    int32 [1] device tensor, set to 1 when a value is beyond fp16."""
    dev = _need_cuda(x, range_flag)
    if x.dtype != torch.float32 or x.shape[-1] % 32 != 0:
        raise ValueError("mx_split expects a float32 tensor whose last dimension is a multiple of 32")
    C_ = int(x.shape[-1])
    out = torch.empty(x.shape, dtype=torch.int32, device=dev)
    _lib.check(_lib.load().oibl_mx_split_rows_flagged(_ptr(x), _ptr(out), x.numel() // C_, C_, _ptr(range_flag),
                                                      _stream(dev)), "mx_split_rows")
    return out


def mx_join(x: torch.Tensor, which: int = 0) -> torch.Tensor:
    """f16mx tensor (int32 container) -> float32: which = 0 hi + q6(lo) (the stored value to ~2^-15 of
    the group's largest element), 1 hi (fp16), 2 q6(hi), 3 q6(lo) — what the kernels multiply."""
    dev = _need_cuda(x)
    if x.dtype != torch.int32 or x.shape[-1] % 32 != 0:
        raise ValueError("mx_join expects an int32 f16mx container whose last dimension is a multiple of 32")
    C_ = int(x.shape[-1])
    out = torch.empty(x.shape, dtype=torch.float32, device=dev)
    _lib.check(_lib.load().oibl_mx_join_rows(_ptr(x), _ptr(out), x.numel() // C_, C_, int(which), _stream(dev)),
               "mx_join_rows")
    return out


def x3_join(x: torch.Tensor) -> torch.Tensor:
    """bf16x3 tensor (int32 container) -> float32 hi + lo (exact)."""
    dev = _need_cuda(x)
    if x.dtype != torch.int32 or x.dim() < 1 or x.shape[-1] % 32 != 0:
        raise ValueError("x3_join expects an int32 bf16x3 container whose last dimension is a multiple of 32")
    out = torch.empty(x.shape, dtype=torch.float32, device=dev)
    C_ = int(x.shape[-1])
    _lib.check(_lib.load().oibl_x3_join_rows(_ptr(x), _ptr(out), x.numel() // C_, C_, _stream(dev)),
               "x3_join_rows")
    return out


def set_regstage(on: bool) -> None:
    """Test hook: run the GEMM main loops register-staged instead of through global_load_lds."""
    _lib.debug_hooks().oibl_debug_set_regstage(1 if on else 0)


def set_conv_tile(mode: int) -> None:
    """Test hook: 0 = auto tile choice, 1 = 128-row tiles, 2 = 256x{128,64}, 3 = 256x256."""
    _lib.debug_hooks().oibl_debug_set_conv_tile(int(mode))


def set_ring_raster(mode: int) -> None:
    """Test hook: tile rasterisation of the ring convolutions (0 = contiguous ids per XCD, 1 = one
    N-tile per XCD, see xcd_tile in csrc/common.h).  Results do not depend on it."""
    _lib.debug_hooks().oibl_debug_set_ring_raster(int(mode))


def set_conv_korder(mode: int) -> None:
    """Test hook: K order of the implicit-GEMM convolutions, 0 = (tap, channel chunk), 1 = (channel
    chunk, tap): 3-8x fewer fetched bytes, slower on all layers but bf16x3 conv2_2; -1 = the per-layer
    default (order 1 for that layer, 0 elsewhere; see csrc/conv.hip)."""
    _lib.debug_hooks().oibl_debug_set_conv_korder(int(mode))


def set_conv_splitk(on: bool) -> None:
    """Test hook: allow / forbid split-K for the backbone layers whose tiling leaves the chip idle
    (small batches: conv4 / conv5 of a single image)."""
    _lib.debug_hooks().oibl_debug_set_conv_splitk(1 if on else 0)


def set_conv_c64(on) -> None:
    """Test hook: resident-weights kernel for Cin = 64 layers (bf16): False/0 = never, True/1 = auto
    (Cout = 64 only; wider layers go to the ring kernel), 2 = every Cin = 64 layer."""
    _lib.debug_hooks().oibl_debug_set_conv_c64(int(on))


def set_conv11_valu(on: bool) -> None:
    """Test hook: run conv1_1 on the vector ALU (exact fp32) also in bf16 mode."""
    _lib.debug_hooks().oibl_debug_set_conv11_valu(1 if on else 0)


# ---- backbone -------------------------------------------------------------------------------
VGG16_CONV_IDX = (0, 2, 5, 7, 10, 12, 14, 17, 19, 21, 24, 26, 28)  # vgg.py:40-42 conv positions
VGG16_CFG = ((3, 64, 1, 0), (64, 64, 1, 1), (64, 128, 1, 0), (128, 128, 1, 1), (128, 256, 1, 0),
             (256, 256, 1, 0), (256, 256, 1, 1), (256, 512, 1, 0), (512, 512, 1, 0),
             (512, 512, 1, 1), (512, 512, 1, 0), (512, 512, 1, 0), (512, 512, 0, 0))


def pack_conv3x3(w: torch.Tensor, precision) -> torch.Tensor:
    """[Cout][Cin][3][3] fp32 -> packed [9][Cout][Cin] in the precision's element type."""
    p = precision_code(precision)
    dev = _need_cuda(w)
    if w.dtype != torch.float32 or w.dim() != 4 or w.shape[2:] != (3, 3):
        raise ValueError("pack_conv3x3 expects a float32 [Cout][Cin][3][3] tensor")
    cout, cin = int(w.shape[0]), int(w.shape[1])
    out = torch.empty((9, cout, cin), dtype=_DTYPES[p], device=dev)
    _lib.check(_lib.load().oibl_pack_conv3x3_weights(_ptr(w), cout, cin, p, _ptr(out),
                                                     _stream(dev)), "pack_conv3x3_weights")
    return out


def conv3x3_nhwc(x: torch.Tensor, packed_w: torch.Tensor, bias: torch.Tensor, relu: bool,
                 pool: bool, precision, range_flag: Optional[torch.Tensor] = None) -> torch.Tensor:
    """x [N][H][W][Cin] T -> [N][Ho][Wo][Cout] T (conv3x3 pad 1 + bias (+ReLU) (+2x2 max-pool)).
    range_flag (f16mx): optional int32 [1] device tensor, set to 1 when an output is beyond fp16."""
    p = precision_code(precision)
    dev = _need_cuda(x, packed_w, bias, range_flag)
    if x.dtype != _DTYPES[p] or packed_w.dtype != _DTYPES[p] or bias.dtype != torch.float32:
        raise ValueError("conv3x3_nhwc: dtype mismatch with precision")
    N, H, W, cin = map(int, x.shape)
    cout = int(packed_w.shape[1])
    if int(packed_w.shape[2]) != cin:
        raise ValueError("conv3x3_nhwc: packed weight Cin mismatch")
    Ho, Wo = (H // 2, W // 2) if pool else (H, W)
    out = torch.empty((N, Ho, Wo, cout), dtype=_DTYPES[p], device=dev)
    lib = _lib.load()
    # scratch for split-K partials: f16mx only here (its small-problem path); the bf16 / bf16x3 / fp32 layers
    # keep running one-pass when called alone — the backbone entry point gives them their scratch — so that
    # the tile-variant tests compare like with like
    ws_bytes = lib.oibl_conv3x3_workspace_bytes(N, H, W, cin, cout, int(pool), p) if p == F16MX else 0
    ws = workspace(ws_bytes, dev, "conv") if ws_bytes else None
    _lib.check(lib.oibl_conv3x3_nhwc_ws(_ptr(x), N, H, W, cin, _ptr(packed_w), _ptr(bias), cout, int(relu),
                                        int(pool), p, _ptr(out), _ptr(ws), ws_bytes, _ptr(range_flag),
                                        _stream(dev)), "conv3x3_nhwc")
    return out


def conv1_1_nchw(x: torch.Tensor, w: torch.Tensor, bias: torch.Tensor, precision) -> torch.Tensor:
    """x [N][3][H][W] fp32 -> [N][H][W][64] T (conv1_1 + bias + ReLU)."""
    p = precision_code(precision)
    dev = _need_cuda(x, w, bias)
    if x.dtype != torch.float32 or w.dtype != torch.float32 or tuple(w.shape) != (64, 3, 3, 3):
        raise ValueError("conv1_1_nchw: expects fp32 x and a [64][3][3][3] fp32 weight")
    N, _, H, W = map(int, x.shape)
    out = torch.empty((N, H, W, 64), dtype=_DTYPES[p], device=dev)
    _lib.check(_lib.load().oibl_conv1_1_nchw(_ptr(x), N, H, W, _ptr(w), _ptr(bias), p, _ptr(out),
                                             _stream(dev)), "conv1_1_nchw")
    return out


def set_stem_fused(on: bool) -> None:
    """Test hook: use / bypass the fused conv1_1+conv1_2+pool stem kernel inside vgg16_conv5 (bf16)."""
    _lib.debug_hooks().oibl_debug_set_stem_fused(1 if on else 0)


def vgg16_stem(x: torch.Tensor, w1: torch.Tensor, b1: torch.Tensor, packed_w2: torch.Tensor,
               b2: torch.Tensor) -> torch.Tensor:
    """Fused bf16 stem: x [N][3][H][W] fp32 -> [N][H//2][W//2][64] bf16 (conv1_1, conv1_2, pool)."""
    dev = _need_cuda(x, w1, b1, packed_w2, b2)
    if x.dtype != torch.float32 or x.dim() != 4 or x.shape[1] != 3:
        raise ValueError("vgg16_stem expects a float32 [N][3][H][W] tensor")
    if tuple(w1.shape) != (64, 3, 3, 3) or tuple(packed_w2.shape) != (9, 64, 64) \
            or packed_w2.dtype != torch.bfloat16:
        raise ValueError("vgg16_stem: conv1_1 must be [64][3][3][3] fp32, conv1_2 packed bf16 [9][64][64]")
    N, _, H, W = map(int, x.shape)
    out = torch.empty((N, H // 2, W // 2, 64), dtype=torch.bfloat16, device=dev)
    _lib.check(_lib.load().oibl_vgg16_stem_bf16(_ptr(x), N, H, W, _ptr(w1), _ptr(b1), _ptr(packed_w2),
                                                _ptr(b2), _ptr(out), _stream(dev)), "vgg16_stem_bf16")
    return out


def vgg16_stem_x3(x: torch.Tensor, w1: torch.Tensor, b1: torch.Tensor, packed_w2: torch.Tensor,
                  b2: torch.Tensor) -> torch.Tensor:
    """Fused bf16x3 stem: x [N][3][H][W] fp32 -> [N][H//2][W//2][64] split elements (int32 container)."""
    dev = _need_cuda(x, w1, b1, packed_w2, b2)
    if x.dtype != torch.float32 or x.dim() != 4 or x.shape[1] != 3:
        raise ValueError("vgg16_stem_x3 expects a float32 [N][3][H][W] tensor")
    if tuple(w1.shape) != (64, 3, 3, 3) or tuple(packed_w2.shape) != (9, 64, 64) \
            or packed_w2.dtype != torch.int32:
        raise ValueError("vgg16_stem_x3: conv1_1 must be [64][3][3][3] fp32, conv1_2 packed bf16x3 [9][64][64]")
    N, _, H, W = map(int, x.shape)
    out = torch.empty((N, H // 2, W // 2, 64), dtype=torch.int32, device=dev)
    _lib.check(_lib.load().oibl_vgg16_stem_x3(_ptr(x), N, H, W, _ptr(w1), _ptr(b1), _ptr(packed_w2),
                                              _ptr(b2), _ptr(out), _stream(dev)), "vgg16_stem_x3")
    return out


def vgg16_stem_mx(x: torch.Tensor, w1: torch.Tensor, b1: torch.Tensor, packed_w2: torch.Tensor,
                  b2: torch.Tensor) -> torch.Tensor:
    """Fused f16mx stem: x [N][3][H][W] fp32 -> [N][H//2][W//2][64] f16mx lines (int32 container);
    packed_w2 = pack_conv3x3(conv1_2, "f16mx")."""
    dev = _need_cuda(x, w1, b1, packed_w2, b2)
    if x.dtype != torch.float32 or x.dim() != 4 or x.shape[1] != 3:
        raise ValueError("vgg16_stem_mx expects a float32 [N][3][H][W] tensor")
    if tuple(w1.shape) != (64, 3, 3, 3) or tuple(packed_w2.shape) != (9, 64, 64) \
            or packed_w2.dtype != torch.int32:
        raise ValueError("vgg16_stem_mx: conv1_1 must be [64][3][3][3] fp32, conv1_2 packed f16mx [9][64][64]")
    N, _, H, W = map(int, x.shape)
    out = torch.empty((N, H // 2, W // 2, 64), dtype=torch.int32, device=dev)
    _lib.check(_lib.load().oibl_vgg16_stem_mx(_ptr(x), N, H, W, _ptr(w1), _ptr(b1), _ptr(packed_w2),
                                              _ptr(b2), _ptr(out), _stream(dev)), "vgg16_stem_mx")
    return out


def vgg16_feature_hw(H: int, W: int) -> Tuple[int, int]:
    for _ in range(4):
        H, W = H // 2, W // 2
    return H, W


# Normalize constants of the reference's loader (ibl/utils/data/__init__.py:40-41): std = 1/255,
# i.e. mean-subtracted 0..255 pixels
REF_MEAN = (0.48501960784313836, 0.4579568627450961, 0.4076039215686255)
REF_STD = (0.00392156862745098, 0.00392156862745098, 0.00392156862745098)


def vgg16_conv5(x: torch.Tensor, weights: Sequence[torch.Tensor], biases: Sequence[torch.Tensor],
                precision, events=None, mean=REF_MEAN, std=REF_STD, return_flag: bool = False,
                out: Optional[torch.Tensor] = None):
    """conv5_3 feature map [N][h][w][512] T (NHWC), h = H//16, w = W//16, of
      x [N][3][H][W] float32, already normalised (what the reference's loader hands over), or
      x [N][H][W][3] uint8, the raw decoded image: ToTensor + Normalize(mean, std) are folded into
        the first kernel (a quarter of the bytes over PCIe; bit-identical results in bf16 / fp32, within
        ~1e-6 / ~1e-5 of the fp32-input result in bf16x3 / f16mx: include/openibl_amd.h).

    weights[0] is the plain conv1_1 tensor, weights[1:] come from pack_conv3x3.
    `events`: optional pair of already-recorded torch.cuda.Event(enable_timing=True); they are
    re-recorded right before / after the matrix-core convolutions (bench.py's roofline).
    return_flag: also return the pass's f16mx range flag — an int32 [1] VIEW of the first word of this
    stream's backbone workspace (None in the other precisions): non-zero once the pass has run = an
    activation was beyond fp16 and `feat` must be recomputed in bf16x3 (models.VGG does).
    out: optional preallocated [N][h][w][512] map (a contiguous slice of a larger batch's map: models.VGG runs an
    f16mx batch beyond the kernels' 32-bit offsets in image groups).  The entry point clears the flag when a pass
    starts; a caller running several groups reads it between them (or accumulates it: models.VGG)."""
    p = precision_code(precision)
    dev = _need_cuda(x, *weights, *biases)
    u8 = x.dtype == torch.uint8
    if u8:
        if x.dim() != 4 or x.shape[3] != 3:
            raise ValueError("vgg16_conv5: uint8 input must be [N][H][W][3]")
        N, H, W, _ = map(int, x.shape)
    else:
        if x.dtype != torch.float32 or x.dim() != 4 or x.shape[1] != 3:
            raise ValueError("vgg16_conv5 expects a float32 [N][3][H][W] or uint8 [N][H][W][3] tensor")
        N, _, H, W = map(int, x.shape)
    if len(weights) != 13 or len(biases) != 13:
        raise ValueError("vgg16_conv5 needs 13 weights and 13 biases")
    x = x.contiguous()
    h, w = vgg16_feature_hw(H, W)
    lib = _lib.load()
    ws_bytes = (lib.oibl_vgg16_u8_workspace_bytes if u8 else lib.oibl_vgg16_workspace_bytes)(N, H, W, p)
    if ws_bytes == 0:
        raise ValueError(f"vgg16_conv5: unsupported input shape {tuple(x.shape)}")
    ws = workspace(ws_bytes, dev, "vgg")
    # bf16x3: the last layer writes a plain fp32 map for the (fp32) head
    if out is not None:
        if tuple(out.shape) != (N, h, w, 512) or out.dtype != _DTYPES[head_precision(p)] or not out.is_contiguous() \
                or out.device != dev:
            raise ValueError("vgg16_conv5: `out` must be a contiguous [N][h][w][512] map of the head's element type")
        feat = out
    else:
        feat = torch.empty((N, h, w, 512), dtype=_DTYPES[head_precision(p)], device=dev)
    wp = (C.c_void_p * 13)(*[t.data_ptr() for t in weights])
    bp = (C.c_void_p * 13)(*[t.data_ptr() for t in biases])
    ev0 = ev1 = None
    if events is not None:
        ev0, ev1 = int(events[0].cuda_event), int(events[1].cuda_event)
    if u8:
        m3 = (C.c_float * 3)(*[float(v) for v in mean])
        s3 = (C.c_float * 3)(*[float(v) for v in std])
        _lib.check(lib.oibl_vgg16_conv5_forward_u8(_ptr(x), N, H, W, m3, s3, wp, bp, p, _ptr(feat),
                                                   _ptr(ws), ws.numel(), _stream(dev), ev0, ev1),
                   "vgg16_conv5_forward_u8")
    else:
        _lib.check(lib.oibl_vgg16_conv5_forward_ev(_ptr(x), N, H, W, wp, bp, p, _ptr(feat), _ptr(ws),
                                                   ws.numel(), _stream(dev), ev0, ev1),
                   "vgg16_conv5_forward")
    if return_flag:
        return feat, (ws[:4].view(torch.int32) if p == F16MX else None)
    return feat


def vgg16_pool4(x: torch.Tensor, weights: Sequence[torch.Tensor], biases: Sequence[torch.Tensor], precision,
                return_flag: bool = False):
    """The frozen trunk of conv5 training (oibl_vgg16_pool4_forward): x [N][3][H][W] float32, normalised ->
    the pooled conv4_3 map [N][H//16][W//16][512], plain fp32 in activation units in every precision; conv1_1 ..
    conv4_3 + pool run exactly as in `vgg16_conv5` (weights / biases as there; entries 0..9 are read).
    return_flag: also the pass's f16mx range flag, as `vgg16_conv5` returns it (None in the other precisions)."""
    p = precision_code(precision)
    dev = _need_cuda(x, *weights[:10], *biases[:10])
    if x.dtype != torch.float32 or x.dim() != 4 or x.shape[1] != 3:
        raise ValueError("vgg16_pool4 expects a float32 [N][3][H][W] tensor")
    if len(weights) < 10 or len(biases) < 10:
        raise ValueError("vgg16_pool4 needs the weights and biases of conv1_1 .. conv4_3")
    N, _, H, W = map(int, x.shape)
    x = x.contiguous()
    h, w = vgg16_feature_hw(H, W)
    lib = _lib.load()
    ws_bytes = lib.oibl_vgg16_workspace_bytes(N, H, W, p)
    if ws_bytes == 0:
        raise ValueError(f"vgg16_pool4: unsupported input shape {tuple(x.shape)}")
    ws = workspace(ws_bytes, dev, "vgg")
    out = torch.empty((N, h, w, 512), dtype=torch.float32, device=dev)
    wp = (C.c_void_p * 13)(*[t.data_ptr() for t in weights[:10]])
    bp = (C.c_void_p * 13)(*[t.data_ptr() for t in biases[:10]])
    _lib.check(lib.oibl_vgg16_pool4_forward(_ptr(x), N, H, W, wp, bp, p, _ptr(out), _ptr(ws), ws.numel(),
                                            _stream(dev)), "vgg16_pool4_forward")
    if return_flag:
        return out, (ws[:4].view(torch.int32) if p == F16MX else None)
    return out


def vgg16_pool4_lines(x: torch.Tensor, weights: Sequence[torch.Tensor], biases: Sequence[torch.Tensor], precision,
                      mean=REF_MEAN, std=REF_STD, return_flag: bool = False, out: Optional[torch.Tensor] = None):
    """The frozen trunk for a cache (oibl_vgg16_pool4_lines_forward[_u8]): x [N][3][H][W] float32 (normalised) or
    [N][H][W][3] uint8 (raw) -> the pooled conv4_3 map [N][H//16][W//16][512] AS IT IS STORED between the layers of
    `vgg16_conv5`, in the precision's element type (bf16; int32 containers of bf16x3 split elements or of f16mx lines,
    the latter with their 2^-3 storage scale; float32) — what `vgg16_conv5_from_pool4` reads.  conv1_1 .. conv4_3 +
    pool run exactly as in `vgg16_conv5` (weights / biases as there; entries 0..9 are read).
    out: optional preallocated map of that shape and type, e.g. a contiguous slice of a cache: written in place.
    return_flag: also the pass's f16mx range flag, as `vgg16_conv5` returns it (None in the other precisions)."""
    p = precision_code(precision)
    if p == F16R:
        raise ValueError("vgg16_pool4_lines: 'f16r' is a matching arithmetic, not a backbone precision")
    dev = _need_cuda(x, *weights[:10], *biases[:10], out)
    u8 = x.dtype == torch.uint8
    if u8:
        if x.dim() != 4 or x.shape[3] != 3:
            raise ValueError("vgg16_pool4_lines: uint8 input must be [N][H][W][3]")
        N, H, W, _ = map(int, x.shape)
    else:
        if x.dtype != torch.float32 or x.dim() != 4 or x.shape[1] != 3:
            raise ValueError("vgg16_pool4_lines expects a float32 [N][3][H][W] or uint8 [N][H][W][3] tensor")
        N, _, H, W = map(int, x.shape)
    if len(weights) < 10 or len(biases) < 10:
        raise ValueError("vgg16_pool4_lines needs the weights and biases of conv1_1 .. conv4_3")
    h, w = vgg16_feature_hw(H, W)
    lib = _lib.load()
    ws_bytes = (lib.oibl_vgg16_u8_workspace_bytes if u8 else lib.oibl_vgg16_workspace_bytes)(N, H, W, p)
    if ws_bytes == 0:
        raise ValueError(f"vgg16_pool4_lines: unsupported input shape {tuple(x.shape)}")
    ws = workspace(ws_bytes, dev, "vgg")
    if out is not None:
        if tuple(out.shape) != (N, h, w, 512) or out.dtype != _DTYPES[p]:
            raise ValueError("vgg16_pool4_lines: `out` must be a contiguous [N][h][w][512] map of the precision's "
                             "element type")
        lines = out
    else:
        lines = torch.empty((N, h, w, 512), dtype=_DTYPES[p], device=dev)
    wp = (C.c_void_p * 13)(*[t.data_ptr() for t in weights[:10]])
    bp = (C.c_void_p * 13)(*[t.data_ptr() for t in biases[:10]])
    if u8:
        m3 = (C.c_float * 3)(*[float(v) for v in mean])
        s3 = (C.c_float * 3)(*[float(v) for v in std])
        _lib.check(lib.oibl_vgg16_pool4_lines_forward_u8(_ptr(x), N, H, W, m3, s3, wp, bp, p, _ptr(lines), _ptr(ws),
                                                         ws.numel(), _stream(dev)), "vgg16_pool4_lines_forward_u8")
    else:
        _lib.check(lib.oibl_vgg16_pool4_lines_forward(_ptr(x), N, H, W, wp, bp, p, _ptr(lines), _ptr(ws),
                                                      ws.numel(), _stream(dev)), "vgg16_pool4_lines_forward")
    if return_flag:
        return lines, (ws[:4].view(torch.int32) if p == F16MX else None)
    return lines


def widen_pool4_lines(lines: torch.Tensor, precision) -> torch.Tensor:
    """Stored pool4 lines (`vgg16_pool4_lines`) -> plain float32 in activation units, what `vgg16_pool4` returns:
    bf16 widened, bf16x3 hi + lo, f16mx hi + q6(lo) with the 2^-3 storage scale undone (exact)."""
    p = precision_code(precision)
    _need_cuda(lines)
    if lines.dtype != _DTYPES.get(p):
        raise ValueError("widen_pool4_lines: the lines are not of the precision's element type")
    if p == F32:
        return lines
    if p == BF16:
        return to_f32(lines)
    if p == BF16X3:
        return x3_join(lines)
    return mx_join(lines).mul_(8.0)


def vgg16_conv5_from_pool4(lines: torch.Tensor, weights: Sequence[torch.Tensor], biases: Sequence[torch.Tensor],
                           precision, return_flag: bool = False, out: Optional[torch.Tensor] = None):
    """conv5_1 .. conv5_3 on stored pool4 lines [N][h][w][512] (`vgg16_pool4_lines`, same precision) -> the conv5_3 map
    [N][h][w][512] in the head's element type, bit-equal to `vgg16_conv5` on the images the lines came from in a batch
    of the same N (oibl_vgg16_conv5_from_pool4: the whole forward's launches for these three layers).  weights /
    biases: the 13 entries of `vgg16_conv5` (entries 10..12 are read) or just those three.  `lines` is only read.
    out: optional preallocated [N][h][w][512] map of the head's element type (a contiguous slice of a larger map).
    return_flag: also the f16mx range flag of these three layers, an int32 [1] view of the first word of this
    stream's backbone workspace (None in the other precisions)."""
    p = precision_code(precision)
    if p == F16R:
        raise ValueError("vgg16_conv5_from_pool4: 'f16r' is a matching arithmetic, not a backbone precision")
    if len(weights) != len(biases) or len(weights) not in (3, 13):
        raise ValueError("vgg16_conv5_from_pool4 needs the 13 weights and biases of the backbone or the 3 of conv5")
    w3, b3 = list(weights[-3:]), list(biases[-3:])
    dev = _need_cuda(lines, *w3, *b3, out)
    if lines.dim() != 4 or int(lines.shape[3]) != 512 or lines.dtype != _DTYPES[p]:
        raise ValueError("vgg16_conv5_from_pool4 expects [N][h][w][512] lines of the precision's element type")
    if any(t.dtype != _DTYPES[p] or tuple(t.shape) != (9, 512, 512) for t in w3):
        raise ValueError("vgg16_conv5_from_pool4: the conv5 weights must be packed [9][512][512] in the same precision")
    N, h, w, _ = map(int, lines.shape)
    lib = _lib.load()
    ws_bytes = lib.oibl_vgg16_conv5_from_pool4_workspace_bytes(N, h, w, p)
    if ws_bytes == 0:
        raise ValueError(f"vgg16_conv5_from_pool4: unsupported shape {tuple(lines.shape)}")
    ws = workspace(ws_bytes, dev, "vgg")
    if out is not None:
        if tuple(out.shape) != (N, h, w, 512) or out.dtype != _DTYPES[head_precision(p)]:
            raise ValueError("vgg16_conv5_from_pool4: `out` must be a contiguous [N][h][w][512] map of the head's "
                             "element type")
        feat = out
    else:
        feat = torch.empty((N, h, w, 512), dtype=_DTYPES[head_precision(p)], device=dev)
    wp = (C.c_void_p * 13)(*([None] * 10 + [t.data_ptr() for t in w3]))
    bp = (C.c_void_p * 13)(*([None] * 10 + [t.data_ptr() for t in b3]))
    _lib.check(lib.oibl_vgg16_conv5_from_pool4(_ptr(lines), N, h, w, wp, bp, p, _ptr(feat), _ptr(ws), ws.numel(),
                                               _stream(dev)), "vgg16_conv5_from_pool4")
    if return_flag:
        return feat, (ws[:4].view(torch.int32) if p == F16MX else None)
    return feat


def global_maxpool_nhwc(feat: torch.Tensor) -> torch.Tensor:
    """[N][h][w][C] T -> [N][C] fp32 (AdaptiveMaxPool2d(1))."""
    dev = _need_cuda(feat)
    p = BF16 if feat.dtype == torch.bfloat16 else F32
    N, C_ = int(feat.shape[0]), int(feat.shape[-1])
    P = feat.numel() // (N * C_)
    out = torch.empty((N, C_), dtype=torch.float32, device=dev)
    _lib.check(_lib.load().oibl_global_maxpool_nhwc(_ptr(feat), N, P, C_, p, _ptr(out),
                                                    _stream(dev)), "global_maxpool_nhwc")
    return out


def nhwc_to_nchw_f32(feat: torch.Tensor) -> torch.Tensor:
    """[N][h][w][C] T -> [N][C][h][w] fp32."""
    dev = _need_cuda(feat)
    p = BF16 if feat.dtype == torch.bfloat16 else F32
    N, h, w, C_ = map(int, feat.shape)
    out = torch.empty((N, C_, h, w), dtype=torch.float32, device=dev)
    _lib.check(_lib.load().oibl_nhwc_to_nchw_f32(_ptr(feat), N, h * w, C_, p, _ptr(out),
                                                 _stream(dev)), "nhwc_to_nchw_f32")
    return out


def nchw_f32_to_nhwc(x: torch.Tensor, precision) -> torch.Tensor:
    """[N][C][h][w] fp32 -> [N][h][w][C] T (bf16x3: fp32, what its head consumes)."""
    p = head_precision(precision)
    dev = _need_cuda(x)
    if x.dtype != torch.float32 or x.dim() != 4:
        raise ValueError("nchw_f32_to_nhwc expects a float32 [N][C][h][w] tensor")
    N, C_, h, w = map(int, x.shape)
    out = torch.empty((N, h, w, C_), dtype=_DTYPES[p], device=dev)
    _lib.check(_lib.load().oibl_nchw_f32_to_nhwc(_ptr(x), N, C_, h * w, p, _ptr(out),
                                                 _stream(dev)), "nchw_f32_to_nhwc")
    return out


# ---- NetVLAD ----------------------------------------------------------------------------------
# argument checks the two heads' wrappers share; `what` is the caller's name, as in _tuple_rows
def _head_weights(what: str, assign_w: torch.Tensor, centroids: torch.Tensor, C_: int, dense_centroids: bool = False):
    """(K, assign_w as a contiguous float32 [K][C] view); the region head also wants its centroids contiguous."""
    K = int(centroids.shape[0])
    aw = assign_w.reshape(K, C_)
    if aw.dtype != torch.float32 or centroids.dtype != torch.float32 or not aw.is_contiguous() \
            or (dense_centroids and not centroids.is_contiguous()):
        raise ValueError(f"{what}: assign_w / centroids must be contiguous float32")
    return K, aw


def _want_letters(what: str, want: Sequence[str]) -> Tuple[str, ...]:
    want = tuple(want)
    if not want or any(t not in ("w", "c", "x") for t in want):
        raise ValueError(f"{what}: want must name some of 'w', 'c', 'x' (got {want!r})")
    return want


def _even_sides(what: str, h: int, w: int) -> None:
    if h % 2 or w % 2 or h == 0 or w == 0:
        raise ValueError(f"{what}: the conv5 map is {h} x {w}, both sides must be even to cut it into quarters")


def _region_tuples(what: str, region_vlad: torch.Tensor, tuple_size: int, tensor_msg: str):
    """Validate region vectors [N][9][L] against tuple_size and return (N, L, T)."""
    if region_vlad.dim() != 3 or int(region_vlad.shape[1]) != 9 or region_vlad.dtype != torch.float32 \
            or not region_vlad.is_contiguous():
        raise ValueError(f"{what}: {tensor_msg}")
    N, _, L = map(int, region_vlad.shape)
    T = int(tuple_size)
    if T <= 0 or N % T:
        raise ValueError(f"{what}: {N} images are not a multiple of tuple_size {T}")
    if N // T < 2:
        raise ValueError(f"{what}: a tuple needs an anchor and at least one pair (got {N // T} image per tuple)")
    return N, L, T


# what the two heads' autograd Functions share (each names its own pair of functions where it calls them)
def _head_forward(ctx, head, feat, assign_w, centroids, normalize_input):
    ctx.save_for_backward(feat, assign_w, centroids)
    ctx.normalize_input = bool(normalize_input)
    return head(feat, assign_w, centroids, normalize_input=ctx.normalize_input)


def _head_backward(ctx, head_backward, grad_out):
    """One call of `head_backward` for exactly the inputs that need a gradient."""
    feat, assign_w, centroids = ctx.saved_tensors
    want = tuple(t for t, n in zip(("x", "w", "c"), ctx.needs_input_grad[:3]) if n)
    if not want:
        return None, None, None, None
    gw, gc, gx = head_backward(feat, assign_w, centroids, grad_out.contiguous(),
                               normalize_input=ctx.normalize_input, want=want)
    if gw is not None:
        gw = gw.reshape(assign_w.shape)
    return gx, gw, gc, None


# The cluster counts the descriptor head runs for: K = 64 on the tuned kernels (oibl_netvlad_forward / _backward), every
# other multiple of 16 up to 128 on the K-general ones (oibl_netvlad_forward_k / _backward_k, csrc/netvlad_k.hip).
NETVLAD_CLUSTERS = tuple(range(16, 129, 16))


def _head_clusters(what: str, K: int) -> bool:
    """True where K takes the K-general entry points, False for the tuned K = 64 ones; another K raises before
    any library call."""
    if K not in NETVLAD_CLUSTERS:
        raise ValueError(f"{what}: num_clusters must be one of {', '.join(map(str, NETVLAD_CLUSTERS))} (got {K})")
    return K != 64


def netvlad(feat: torch.Tensor, assign_w: torch.Tensor, centroids: torch.Tensor,
            normalize_input: bool = True, want_raw: bool = False, want_norm: bool = True):
    """feat [N][h][w][C] (or [N][P][C]) T -> (vlad_raw [N][K][C] | None, vlad_norm [N][K*C] | None).
    K = 64: the tuned kernels, in the map's own element type.  K = 16, 32, 48, 80, 96, 112, 128: the K-general
    fp32 kernels (oibl_netvlad_forward_k); a bf16 map is widened to fp32 first, as `netvlad_head` does."""
    dev = _need_cuda(feat, assign_w, centroids)
    p = BF16 if feat.dtype == torch.bfloat16 else F32
    if feat.dtype not in (torch.bfloat16, torch.float32):
        raise ValueError("netvlad: feature map must be bf16 or fp32")
    N, C_ = int(feat.shape[0]), int(feat.shape[-1])
    P = feat.numel() // (N * C_)
    K, aw = _head_weights("netvlad", assign_w, centroids, C_)
    general = _head_clusters("netvlad", K)
    lib = _lib.load()
    if general:
        if feat.dtype == torch.bfloat16:
            feat = feat.float()
        ws = workspace(lib.oibl_netvlad_k_workspace_bytes(N, P, K, C_), dev, "netvlad_k")
        raw = torch.empty((N, K, C_), dtype=torch.float32, device=dev) if want_raw else None
        nrm = torch.empty((N, K * C_), dtype=torch.float32, device=dev) if want_norm else None
        _lib.check(lib.oibl_netvlad_forward_k(_ptr(feat), N, P, K, C_, _ptr(aw), _ptr(centroids),
                                              int(normalize_input), _ptr(raw), _ptr(nrm), _ptr(ws), ws.numel(),
                                              _stream(dev)), "netvlad_forward_k")
        return raw, nrm
    ws_bytes = lib.oibl_netvlad_workspace_bytes(N, P, K, C_)
    ws = workspace(ws_bytes, dev, "netvlad")
    raw = torch.empty((N, K, C_), dtype=torch.float32, device=dev) if want_raw else None
    nrm = torch.empty((N, K * C_), dtype=torch.float32, device=dev) if want_norm else None
    _lib.check(lib.oibl_netvlad_forward(_ptr(feat), N, P, K, C_, p, _ptr(aw), _ptr(centroids),
                                        int(normalize_input), _ptr(raw), _ptr(nrm), _ptr(ws),
                                        ws.numel(), _stream(dev)), "netvlad_forward")
    return raw, nrm


def netvlad_backward(feat: torch.Tensor, assign_w: torch.Tensor, centroids: torch.Tensor, grad_out: torch.Tensor,
                     normalize_input: bool = True, want: Sequence[str] = ("w", "c", "x")):
    """Gradients of `netvlad(...)`'s vlad_norm (NetVLAD.forward + the two normalisations of EmbedNet.forward,
    ibl/models/netvlad.py:44-61, 78-80; oibl_netvlad_backward).  feat [N][h][w][C] (or [N][P][C]) fp32, grad_out
    [N][K*C] fp32 = dL/d vlad_norm -> (grad_assign_w [K][C] | None, grad_centroids [K][C] | None, grad_feat like
    feat | None) for the letters in `want` ("w", "c", "x").  Stateless: the forward's intermediates are recomputed
    from feat.  Bit-identical from run to run; an output does not depend on which others are asked for.  K = 64 takes
    oibl_netvlad_backward, the other K of NETVLAD_CLUSTERS oibl_netvlad_backward_k."""
    dev = _need_cuda(feat, assign_w, centroids, grad_out)
    want = _want_letters("netvlad_backward", want)
    if feat.dtype != torch.float32 or grad_out.dtype != torch.float32:
        raise ValueError("netvlad_backward: feature map and grad_out must be fp32")
    N, C_ = int(feat.shape[0]), int(feat.shape[-1])
    P = feat.numel() // (N * C_)
    K, aw = _head_weights("netvlad_backward", assign_w, centroids, C_)
    if grad_out.numel() != N * K * C_:
        raise ValueError(f"netvlad_backward: grad_out has {grad_out.numel()} elements, expected {N} x {K * C_}")
    general = _head_clusters("netvlad_backward", K)
    lib = _lib.load()
    gw = torch.empty((K, C_), dtype=torch.float32, device=dev) if "w" in want else None
    gc = torch.empty((K, C_), dtype=torch.float32, device=dev) if "c" in want else None
    gx = torch.empty(feat.shape, dtype=torch.float32, device=dev) if "x" in want else None
    if general:
        ws = workspace(lib.oibl_netvlad_k_backward_workspace_bytes(N, P, K, C_, int("x" in want)), dev,
                       "netvlad_backward_k")
        _lib.check(lib.oibl_netvlad_backward_k(_ptr(feat), N, P, K, C_, _ptr(aw), _ptr(centroids),
                                               int(normalize_input), _ptr(grad_out), _ptr(gw), _ptr(gc), _ptr(gx),
                                               _ptr(ws), ws.numel(), _stream(dev)), "netvlad_backward_k")
        return gw, gc, gx
    ws = workspace(lib.oibl_netvlad_backward_workspace_bytes(N, P, K, C_, int("x" in want)), dev, "netvlad_backward")
    _lib.check(lib.oibl_netvlad_backward(_ptr(feat), N, P, K, C_, F32, _ptr(aw), _ptr(centroids),
                                         int(normalize_input), _ptr(grad_out), _ptr(gw), _ptr(gc), _ptr(gx),
                                         _ptr(ws), ws.numel(), _stream(dev)), "netvlad_backward")
    return gw, gc, gx


class _NetVLADHead(torch.autograd.Function):
    @staticmethod
    def forward(ctx, *args):
        return _head_forward(ctx, netvlad, *args)[1]

    @staticmethod
    def backward(ctx, grad_out):
        return _head_backward(ctx, netvlad_backward, grad_out)


def netvlad_head(feat: torch.Tensor, assign_w: torch.Tensor, centroids: torch.Tensor,
                 normalize_input: bool = True) -> torch.Tensor:
    """The differentiable descriptor head: vlad_norm [N][K*C], bit-equal to `netvlad(..., want_norm=True)`, with a
    graph to whichever of feat, assign_w ([K][C] or conv.weight's [K][C][1][1]) and centroids require a gradient;
    its backward is one call of `netvlad_backward` for exactly those.  A bf16 map is widened to fp32 first (the
    gradient kernels are fp32); its gradient then comes back in bf16 through torch's cast.  K as in `netvlad`: 64 on
    the tuned kernels, the other multiples of 16 up to 128 on the K-general ones, anything else a ValueError."""
    if feat.dtype == torch.bfloat16:
        feat = feat.float()
    _need_cuda(feat, assign_w, centroids)
    return _NetVLADHead.apply(feat, assign_w, centroids, bool(normalize_input))


# ---- conv5 training: gradients of a 3x3 convolution -----------------------------------------------
def conv3x3_backward(x: torch.Tensor, weight: torch.Tensor, grad_out: torch.Tensor,
                     out_act: Optional[torch.Tensor] = None, want: Sequence[str] = ("w", "b", "x")):
    """Gradients of conv3x3(pad 1) (+ ReLU) (oibl_conv3x3_backward; nn.Conv2d + nn.ReLU of ibl/models/vgg.py:41-42
    under autograd).  x [N][H][W][512] fp32 NHWC, the layer's input; weight [512][512][3][3] fp32, the state-dict
    tensor; grad_out [N][H][W][512] fp32 = dL/d output; out_act: None, or the layer's post-ReLU output — grad_out
    then counts as 0 where out_act <= 0 -> (grad_weight like weight | None, grad_bias [512] | None, grad_x like x |
    None) for the letters in `want` ("w", "b", "x").  Exact fp32; bit-identical from run to run; an output does not
    depend on which others are asked for; an image's grad_x rows do not depend on its batch mates."""
    dev = _need_cuda(x, weight, grad_out, out_act)
    want = tuple(want)
    if not want or any(t not in ("w", "b", "x") for t in want):
        raise ValueError(f"conv3x3_backward: want must name some of 'w', 'b', 'x' (got {want!r})")
    if x.dtype != torch.float32 or weight.dtype != torch.float32 or grad_out.dtype != torch.float32 or \
            (out_act is not None and out_act.dtype != torch.float32):
        raise ValueError("conv3x3_backward: every tensor must be fp32")
    if x.dim() != 4 or weight.dim() != 4 or tuple(weight.shape[2:]) != (3, 3) or int(weight.shape[1]) != int(x.shape[3]):
        raise ValueError("conv3x3_backward expects x [N][H][W][Cin] and weight [Cout][Cin][3][3]")
    N, H, W, cin = map(int, x.shape)
    cout = int(weight.shape[0])
    if tuple(grad_out.shape) != (N, H, W, cout) or (out_act is not None and tuple(out_act.shape) != (N, H, W, cout)):
        raise ValueError(f"conv3x3_backward: grad_out / out_act must be [{N}][{H}][{W}][{cout}]")
    lib = _lib.load()
    ws = workspace(lib.oibl_conv3x3_backward_workspace_bytes(N, H, W, cin, cout, int("x" in want)), dev,
                   "conv_backward")
    gw = torch.empty(weight.shape, dtype=torch.float32, device=dev) if "w" in want else None
    gb = torch.empty((cout,), dtype=torch.float32, device=dev) if "b" in want else None
    gx = torch.empty(x.shape, dtype=torch.float32, device=dev) if "x" in want else None
    _lib.check(lib.oibl_conv3x3_backward(_ptr(x), N, H, W, cin, _ptr(weight), cout, _ptr(out_act), _ptr(grad_out),
                                         _ptr(gw), _ptr(gb), _ptr(gx), _ptr(ws), ws.numel(), _stream(dev)),
               "conv3x3_backward")
    return gw, gb, gx


class _Conv3x3Train(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, relu):
        w = weight.detach().float().contiguous()
        y = conv3x3_nhwc(x, pack_conv3x3(w, F32), bias.detach().float().contiguous(), bool(relu), False, F32)
        ctx.relu = bool(relu)
        ctx.save_for_backward(x, w, y if relu else None)   # the post-ReLU output is its own mask
        return y

    @staticmethod
    def backward(ctx, grad_out):
        x, w, y = ctx.saved_tensors
        want = tuple(t for t, n in zip(("x", "w", "b"), ctx.needs_input_grad[:3]) if n)
        if not want:
            return None, None, None, None
        gw, gb, gx = conv3x3_backward(x, w, grad_out.contiguous(), out_act=y, want=want)
        return gx, gw, gb, None


def conv3x3_train(x: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor, relu: bool) -> torch.Tensor:
    """The differentiable conv3x3(pad 1) + bias (+ ReLU) of conv5 training: x [N][H][W][512] fp32 NHWC, weight
    [512][512][3][3] and bias [512] the LIVE parameters -> [N][H][W][512] fp32, bit-equal to `pack_conv3x3` +
    `conv3x3_nhwc` in fp32, with a graph to whichever of x, weight and bias require a gradient; its backward is one
    call of `conv3x3_backward` for exactly those."""
    _need_cuda(x, weight, bias)
    if x.dtype != torch.float32:
        raise ValueError("conv3x3_train: the activation must be fp32")
    return _Conv3x3Train.apply(x, weight, bias, bool(relu))


# ---- SFRS region similarities ---------------------------------------------------------------------
def region_vlad(feat: torch.Tensor, assign_w: torch.Tensor, centroids: torch.Tensor,
                normalize_input: bool = True) -> torch.Tensor:
    """feat [N][h][w][C] fp32 or bf16 (widened to fp32: the region head is fp32), h and w even -> [N][9][K*C] fp32:
    the intra- and L2-normalised NetVLAD of the whole image, its four halves and its four quarters
    (EmbedRegionNet._compute_region_sim, ibl/models/netvlad.py:123-175).  An image's vectors do not depend on the
    batch it is computed in."""
    dev = _need_cuda(feat, assign_w, centroids)
    if feat.dim() != 4 or feat.dtype not in (torch.bfloat16, torch.float32):
        raise ValueError("region_vlad: feature map must be a bf16 or fp32 [N][h][w][C] tensor")
    N, h, w, C_ = map(int, feat.shape)
    _even_sides("region_vlad", h, w)
    feat = feat.float().contiguous()
    K, aw = _head_weights("region_vlad", assign_w, centroids, C_, dense_centroids=True)
    lib = _lib.load()
    ws = workspace(lib.oibl_region_workspace_bytes(N, h, w, K, C_), dev, "region")
    out = torch.empty((N, 9, K * C_), dtype=torch.float32, device=dev)
    _lib.check(lib.oibl_region_vlad_forward(_ptr(feat), N, h, w, K, C_, F32, _ptr(aw), _ptr(centroids),
                                            int(normalize_input), _ptr(out), _ptr(ws), ws.numel(), _stream(dev)),
               "region_vlad_forward")
    return out


def region_scores(region_vlad: torch.Tensor, tuple_size: int) -> torch.Tensor:
    """region_vlad [T*(1+n)][9][L] fp32, tuple-major with the anchor first -> score [T][n][9][9],
    score[t, j, a, b] = <region a of tuple t's anchor, region b of its pair j> (netvlad.py:177-184)."""
    dev = _need_cuda(region_vlad)
    N, L, T = _region_tuples("region_scores", region_vlad, tuple_size, "a contiguous float32 [N][9][L] tensor")
    score = torch.empty((T, N // T - 1, 9, 9), dtype=torch.float32, device=dev)
    _lib.check(_lib.load().oibl_region_scores(_ptr(region_vlad), T, N // T, L, _ptr(score), _stream(dev)),
               "region_scores")
    return score


def region_vlad_backward(feat: torch.Tensor, assign_w: torch.Tensor, centroids: torch.Tensor, grad_out: torch.Tensor,
                         normalize_input: bool = True, want: Sequence[str] = ("w", "c", "x")):
    """Gradients of `region_vlad(...)` (oibl_region_vlad_backward).  feat [N][h][w][C] fp32, h and w even, grad_out
    [N][9][K*C] fp32 = dL/d region_vlad -> (grad_assign_w [K][C] | None, grad_centroids [K][C] | None, grad_feat like
    feat | None) for the letters in `want` ("w", "c", "x").  Stateless: the forward's intermediates are recomputed
    from feat.  Bit-identical from run to run; an output does not depend on which others are asked for."""
    dev = _need_cuda(feat, assign_w, centroids, grad_out)
    want = _want_letters("region_vlad_backward", want)
    if feat.dim() != 4 or feat.dtype != torch.float32 or grad_out.dtype != torch.float32:
        raise ValueError("region_vlad_backward: feature map [N][h][w][C] and grad_out must be fp32")
    if not feat.is_contiguous() or not grad_out.is_contiguous():
        raise ValueError("region_vlad_backward: feature map and grad_out must be contiguous")
    N, h, w, C_ = map(int, feat.shape)
    _even_sides("region_vlad_backward", h, w)
    K, aw = _head_weights("region_vlad_backward", assign_w, centroids, C_, dense_centroids=True)
    if grad_out.numel() != N * 9 * K * C_:
        raise ValueError(f"region_vlad_backward: grad_out has {grad_out.numel()} elements, expected {N} x 9 x {K * C_}")
    lib = _lib.load()
    ws = workspace(lib.oibl_region_backward_workspace_bytes(N, h, w, K, C_, int("x" in want)), dev, "region_backward")
    gw = torch.empty((K, C_), dtype=torch.float32, device=dev) if "w" in want else None
    gc = torch.empty((K, C_), dtype=torch.float32, device=dev) if "c" in want else None
    gx = torch.empty(feat.shape, dtype=torch.float32, device=dev) if "x" in want else None
    _lib.check(lib.oibl_region_vlad_backward(_ptr(feat), N, h, w, K, C_, F32, _ptr(aw), _ptr(centroids),
                                             int(normalize_input), _ptr(grad_out), _ptr(gw), _ptr(gc), _ptr(gx),
                                             _ptr(ws), ws.numel(), _stream(dev)), "region_vlad_backward")
    return gw, gc, gx


def region_scores_backward(region_vlad: torch.Tensor, grad_score: torch.Tensor, tuple_size: int) -> torch.Tensor:
    """Gradient of `region_scores(region_vlad, tuple_size)` (oibl_region_scores_backward): region_vlad
    [T*(1+n)][9][L] fp32 as given to the forward, grad_score [T][n][9][9] fp32 -> dL/d region_vlad, same shape."""
    dev = _need_cuda(region_vlad, grad_score)
    N, L, T = _region_tuples("region_scores_backward", region_vlad, tuple_size,
                             "region_vlad must be a contiguous float32 [N][9][L] tensor")
    if grad_score.dtype != torch.float32 or not grad_score.is_contiguous() \
            or tuple(grad_score.shape) != (T, N // T - 1, 9, 9):
        raise ValueError(f"region_scores_backward: grad_score must be a contiguous float32 [{T}][{N // T - 1}][9][9]")
    out = torch.empty_like(region_vlad)
    _lib.check(_lib.load().oibl_region_scores_backward(_ptr(region_vlad), T, N // T, L, _ptr(grad_score), _ptr(out),
                                                       _stream(dev)), "region_scores_backward")
    return out


class _RegionVLAD(torch.autograd.Function):
    @staticmethod
    def forward(ctx, *args):
        return _head_forward(ctx, region_vlad, *args)

    @staticmethod
    def backward(ctx, grad_out):
        return _head_backward(ctx, region_vlad_backward, grad_out)


class _RegionScores(torch.autograd.Function):
    @staticmethod
    def forward(ctx, vec, tuple_size):
        ctx.save_for_backward(vec)
        ctx.tuple_size = int(tuple_size)
        return region_scores(vec, ctx.tuple_size)

    @staticmethod
    def backward(ctx, grad_score):
        (vec,) = ctx.saved_tensors
        if not ctx.needs_input_grad[0]:
            return None, None
        return region_scores_backward(vec, grad_score.contiguous(), ctx.tuple_size), None


def region_vlad_train(feat: torch.Tensor, assign_w: torch.Tensor, centroids: torch.Tensor,
                      normalize_input: bool = True) -> torch.Tensor:
    """The differentiable region head: [N][9][K*C], bit-equal to `region_vlad`, with a graph to whichever of feat,
    assign_w ([K][C] or conv.weight's [K][C][1][1]) and centroids require a gradient; its backward is one call of
    `region_vlad_backward` for exactly those.  A bf16 map is widened to fp32 first, as `netvlad_head` does."""
    if feat.dtype == torch.bfloat16:
        feat = feat.float()
    _need_cuda(feat, assign_w, centroids)
    if feat.dtype != torch.float32:
        raise ValueError("region_vlad_train: feature map must be bf16 or fp32")
    return _RegionVLAD.apply(feat.contiguous(), assign_w, centroids, bool(normalize_input))


def region_scores_train(vec: torch.Tensor, tuple_size: int) -> torch.Tensor:
    """The differentiable `region_scores`: score [T][n][9][9], bit-equal to it, its backward one call of
    `region_scores_backward`.  Autograd adds this gradient to the one that reaches `vec` from its direct use."""
    _need_cuda(vec)
    return _RegionScores.apply(vec, int(tuple_size))


# ---- training losses ----------------------------------------------------------------------------
LOSS_KINDS = {"triplet": 0, "sare_joint": 1, "sare_ind": 2}
LOSS_SCORES = {"sqdist": 0, "dot": 1}
TUPLE_LOSS_MAX_NEG = 64
SOFT_LABEL_MAX_J = 4096


def _tuple_rows(what: str, anchors: torch.Tensor, positives: torch.Tensor, negatives: torch.Tensor):
    """Validate the three inputs of a tuple loss (strided views welcome: only the last dimension must be contiguous)
    and return (device, B, M, L)."""
    shapes = f"anchors {tuple(anchors.shape)}, positives {tuple(positives.shape)}, negatives {tuple(negatives.shape)}"
    for t in (anchors, positives, negatives):
        if not t.is_cuda:
            raise _lib.OpenIBLAmdError(f"openibl_amd: {what}: tensor is on {t.device}; this path runs only on an AMD "
                                       "GPU through the HIP extension (there is no CPU fallback)")
        if t.device != anchors.device:
            raise ValueError(f"{what}: tensors on different devices")
        if t.dtype != torch.float32:
            raise ValueError(f"{what}: float32 tensors only (got {t.dtype}; {shapes})")
    if anchors.dim() != 2 or positives.shape != anchors.shape or negatives.dim() != 3 \
            or negatives.shape[0] != anchors.shape[0] or negatives.shape[2] != anchors.shape[1]:
        raise ValueError(f"{what}: anchors [B][L], positives [B][L] and negatives [B][M][L] are expected (got {shapes})")
    B, M, L = map(int, negatives.shape)
    if B < 1 or L < 1 or not 1 <= M <= TUPLE_LOSS_MAX_NEG or B > 65535:
        raise ValueError(f"{what}: 1 <= B <= 65535, 1 <= M <= {TUPLE_LOSS_MAX_NEG} and L >= 1 are supported (got {shapes})")
    for name, t in (("anchors", anchors), ("positives", positives), ("negatives", negatives)):
        if (L > 1 and t.stride(-1) != 1) or any(s < 0 for s in t.stride()):
            raise ValueError(f"{what}: the last dimension of {name} must be contiguous (strides {t.stride()}; {shapes})")
    return anchors.device, B, M, L


def _tuple_strides(anchors, positives, negatives):
    return (int(anchors.stride(0)), int(positives.stride(0)), int(negatives.stride(0)), int(negatives.stride(1)))


def tuple_loss_forward(anchors: torch.Tensor, positives: torch.Tensor, negatives: torch.Tensor, kind: str,
                       margin: float = 0.3, temp: float = 0.07, score: str = "sqdist"):
    """oibl_tuple_loss_forward: -> (loss, a 0-dim fp32 tensor; coef [B][1+M] fp64, the table the backward consumes)."""
    if kind not in LOSS_KINDS:
        raise ValueError(f"tuple_loss: unknown loss {kind!r} (one of {sorted(LOSS_KINDS)})")
    if score not in LOSS_SCORES:
        raise ValueError(f"tuple_loss: unknown score {score!r} (one of {sorted(LOSS_SCORES)})")
    dev, B, M, L = _tuple_rows("tuple_loss", anchors, positives, negatives)
    sa, sp, snt, snr = _tuple_strides(anchors, positives, negatives)
    lib = _lib.load()
    ws = workspace(lib.oibl_tuple_loss_workspace_bytes(B, M), dev, "tuple_loss")
    loss = torch.empty((), dtype=torch.float32, device=dev)
    coef = torch.empty((B, 1 + M), dtype=torch.float64, device=dev)
    _lib.check(lib.oibl_tuple_loss_forward(_ptr(anchors), sa, _ptr(positives), sp, _ptr(negatives), snt, snr, B, M, L,
                                           LOSS_KINDS[kind], LOSS_SCORES[score], float(margin), float(temp),
                                           _ptr(loss), _ptr(coef), _ptr(ws), ws.numel(), _stream(dev)),
               "tuple_loss_forward")
    return loss, coef


def tuple_loss_backward(anchors: torch.Tensor, positives: torch.Tensor, negatives: torch.Tensor, coef: torch.Tensor,
                        grad_loss: torch.Tensor, kind: str, score: str = "sqdist", want: Sequence[str] = ("a", "p", "n")):
    """oibl_tuple_loss_backward: one launch -> (grad_anchors [B][L] | None, grad_positives [B][L] | None,
    grad_negatives [B][M][L] | None), compact fp32, for the letters in `want`.  grad_loss is a device fp32 scalar."""
    dev, B, M, L = _tuple_rows("tuple_loss_backward", anchors, positives, negatives)
    want = tuple(want)
    if not want or any(t not in ("a", "p", "n") for t in want):
        raise ValueError(f"tuple_loss_backward: want must name some of 'a', 'p', 'n' (got {want!r})")
    if coef.dtype != torch.float64 or tuple(coef.shape) != (B, 1 + M) or not coef.is_contiguous() or coef.device != dev:
        raise ValueError(f"tuple_loss_backward: the table must be a contiguous float64 [{B}][{1 + M}] "
                         f"(got {coef.dtype} {tuple(coef.shape)})")
    if grad_loss.dtype != torch.float32 or grad_loss.numel() != 1 or grad_loss.device != dev:
        raise ValueError(f"tuple_loss_backward: grad_loss must be one float32 on the device (got {grad_loss.dtype} "
                         f"{tuple(grad_loss.shape)})")
    sa, sp, snt, snr = _tuple_strides(anchors, positives, negatives)
    ga = torch.empty((B, L), dtype=torch.float32, device=dev) if "a" in want else None
    gp = torch.empty((B, L), dtype=torch.float32, device=dev) if "p" in want else None
    gn = torch.empty((B, M, L), dtype=torch.float32, device=dev) if "n" in want else None
    _lib.check(_lib.load().oibl_tuple_loss_backward(_ptr(anchors), sa, _ptr(positives), sp, _ptr(negatives), snt, snr,
                                                    B, M, L, LOSS_KINDS[kind], LOSS_SCORES[score], _ptr(coef),
                                                    _ptr(grad_loss), _ptr(ga), _ptr(gp), _ptr(gn), _stream(dev)),
               "tuple_loss_backward")
    return ga, gp, gn


class _TupleLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, anchors, positives, negatives, kind, margin, temp, score):
        loss, coef = tuple_loss_forward(anchors, positives, negatives, kind, margin=margin, temp=temp, score=score)
        ctx.save_for_backward(anchors, positives, negatives, coef)
        ctx.kind, ctx.score = kind, score
        return loss

    @staticmethod
    def backward(ctx, grad_loss):
        anchors, positives, negatives, coef = ctx.saved_tensors
        want = tuple(t for t, n in zip(("a", "p", "n"), ctx.needs_input_grad[:3]) if n)
        if not want:
            return None, None, None, None, None, None, None
        ga, gp, gn = tuple_loss_backward(anchors, positives, negatives, coef,
                                         grad_loss.to(torch.float32).contiguous(), ctx.kind, ctx.score, want=want)
        return ga, gp, gn, None, None, None, None


def tuple_loss(anchors: torch.Tensor, positives: torch.Tensor, negatives: torch.Tensor, kind: str,
               margin: float = 0.3, temp: float = 0.07, score: str = "sqdist") -> torch.Tensor:
    """The tuple losses of the reference's trainers, fused (oibl_tuple_loss_forward / _backward): anchors [B][L],
    positives [B][L], negatives [B][M][L] fp32, strided views read in place -> the scalar loss, with a graph to
    whichever of the three requires a gradient.
      kind 'triplet'     F.triplet_margin_loss(margin, p=2, reduction='mean') over the B M triples
           'sare_joint'  (-log_softmax([z_pos, z_neg_1 ..], 1)[:, 0]).mean() over B
           'sare_ind'    the same over the B M pairs [z_pos, z_neg_j]
      score 'sqdist'     z = -|a - x|^2 (Trainer._get_loss)      'dot'  z = <a, x> / temp (SFRSTrainer._get_loss)
    Two launches forward, one backward, fp64 inside, bit-identical from run to run."""
    return _TupleLoss.apply(anchors, positives, negatives, kind, float(margin), float(temp), score)


def _soft_rows(what: str, student: torch.Tensor, teacher: Optional[torch.Tensor]):
    shapes = f"student {tuple(student.shape)}" + ("" if teacher is None else f", teacher {tuple(teacher.shape)}")
    dev = _need_cuda(student, teacher)
    if student.dim() != 2 or student.dtype != torch.float32 or (teacher is not None and (
            teacher.shape != student.shape or teacher.dtype != torch.float32)):
        raise ValueError(f"{what}: contiguous float32 [B][J] score tables of one shape are expected (got {shapes})")
    B, J = map(int, student.shape)
    if not 1 <= B <= 65535 or not 1 <= J <= SOFT_LABEL_MAX_J:
        raise ValueError(f"{what}: 1 <= B <= 65535 and 1 <= J <= {SOFT_LABEL_MAX_J} are supported (got {shapes})")
    return dev, B, J


def soft_label_loss_forward(student: torch.Tensor, teacher: torch.Tensor, temp_student: float, temp_teacher: float):
    """oibl_soft_label_loss_forward: -> (loss, 0-dim fp32; coef [B][J] fp64 = dloss / dstudent)."""
    dev, B, J = _soft_rows("soft_label_loss", student, teacher)
    if not (temp_student > 0 and temp_teacher > 0):
        raise ValueError(f"soft_label_loss: temperatures must be positive (got {temp_student}, {temp_teacher})")
    lib = _lib.load()
    ws = workspace(lib.oibl_soft_label_loss_workspace_bytes(B, J), dev, "soft_label_loss")
    loss = torch.empty((), dtype=torch.float32, device=dev)
    coef = torch.empty((B, J), dtype=torch.float64, device=dev)
    _lib.check(lib.oibl_soft_label_loss_forward(_ptr(student), _ptr(teacher), B, J, float(temp_student),
                                                float(temp_teacher), _ptr(loss), _ptr(coef), _ptr(ws), ws.numel(),
                                                _stream(dev)), "soft_label_loss_forward")
    return loss, coef


class _SoftLabelLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, student, teacher, temp_student, temp_teacher):
        loss, coef = soft_label_loss_forward(student, teacher, temp_student, temp_teacher)
        ctx.save_for_backward(coef)
        return loss

    @staticmethod
    def backward(ctx, grad_loss):
        (coef,) = ctx.saved_tensors
        if not ctx.needs_input_grad[0]:
            return None, None, None, None
        B, J = map(int, coef.shape)
        out = torch.empty((B, J), dtype=torch.float32, device=coef.device)
        _lib.check(_lib.load().oibl_soft_label_loss_backward(_ptr(coef), B, J,
                                                             _ptr(grad_loss.to(torch.float32).contiguous()),
                                                             _ptr(out), _stream(coef.device)), "soft_label_loss_backward")
        return out, None, None, None


def soft_label_loss(student: torch.Tensor, teacher: torch.Tensor, temp_student: float, temp_teacher: float) -> torch.Tensor:
    """loss_soft of SFRSTrainer._forward, fused: student, teacher [B][J] fp32 contiguous ->
    (-softmax(teacher / temp_teacher, 1) * log_softmax(student / temp_student, 1)).mean(0).sum().  The teacher is a
    label: it gets no gradient; the student's is (softmax(s / ts) - softmax(t / tt)) / (B ts), one launch."""
    return _SoftLabelLoss.apply(student, teacher.detach(), float(temp_student), float(temp_teacher))


# ---- PCA --------------------------------------------------------------------------------------
class PcaWeight:
    """A PCA weight [d][D] resident on the device, with — fp32 only — the re-packed copy the streaming kernel
    reads (oibl_pca_pack_weight; made on first use by a batch of 3 .. 32 rows, a second d * D * 4 bytes)."""

    def __init__(self, rows: torch.Tensor):
        if rows.dim() != 2 or rows.dtype not in (torch.bfloat16, torch.float32) or not rows.is_contiguous():
            raise ValueError("PcaWeight: a contiguous bf16 or fp32 [d][D] tensor")
        self.rows = rows
        self._packed = None

    def packed(self) -> torch.Tensor:
        if self._packed is None:
            w = self.rows
            if w.dtype != torch.float32:
                raise ValueError("PcaWeight.packed: fp32 weights only")
            dev = _need_cuda(w)
            d, D = map(int, w.shape)
            out = torch.empty_like(w)
            _lib.check(_lib.load().oibl_pca_pack_weight(_ptr(w), D, d, _ptr(out), _stream(dev)), "pca_pack_weight")
            self._packed = out
        return self._packed


PCA_STREAM_MIN_ROWS = 3      # one or two rows: the row-major streaming kernel (pca_small_kernel) is as fast


def pca(v: torch.Tensor, w, b: torch.Tensor, l2norm: bool = True) -> torch.Tensor:
    """normalize(W v + b): v [N][D] fp32, w [d][D] bf16|fp32 (selects the precision) or a PcaWeight, b [d] fp32."""
    holder = w if isinstance(w, PcaWeight) else None
    if holder is not None:
        w = holder.rows
    dev = _need_cuda(v, w, b)
    if w.dtype not in (torch.bfloat16, torch.float32):
        raise ValueError("pca: weight must be bf16 or fp32")
    p = BF16 if w.dtype == torch.bfloat16 else F32
    if v.dtype != torch.float32 or b.dtype != torch.float32:
        raise ValueError("pca: v and b must be float32")
    N, D = map(int, v.shape)
    d = int(w.shape[0])
    if w.numel() != d * D:
        raise ValueError("pca: weight shape mismatch")
    lib = _lib.load()
    ws_bytes = lib.oibl_pca_workspace_bytes(N, D, d, p)
    ws = workspace(ws_bytes, dev, "pca")
    out = torch.empty((N, d), dtype=torch.float32, device=dev)
    if (holder is not None and p == F32 and N >= PCA_STREAM_MIN_ROWS and lib.oibl_pca_packed_supported(N, D, d)):
        _lib.check(lib.oibl_pca_forward_packed(_ptr(v), N, D, _ptr(holder.packed()), _ptr(b), d, int(l2norm),
                                               _ptr(out), _ptr(ws), ws.numel(), _stream(dev)), "pca_forward_packed")
        return out
    _lib.check(lib.oibl_pca_forward(_ptr(v), N, D, _ptr(w), _ptr(b), d, p, int(l2norm), _ptr(out),
                                    _ptr(ws), ws.numel(), _stream(dev)), "pca_forward")
    return out


def l2_normalize(x: torch.Tensor) -> torch.Tensor:
    """Row-wise x / max(||x||, 1e-12) for a float32 [N][D] tensor."""
    dev = _need_cuda(x)
    if x.dtype != torch.float32 or x.dim() != 2:
        raise ValueError("l2_normalize expects a float32 [N][D] tensor")
    out = torch.empty_like(x)
    if x.shape[0] == 0:
        return out
    _lib.check(_lib.load().oibl_l2_normalize_rows(_ptr(x), int(x.shape[0]), int(x.shape[1]),
                                                  _ptr(out), _stream(dev)), "l2_normalize_rows")
    return out


# ---- 16-bit descriptor storage (BASELINE.json configs[4]; no counterpart in the reference) ----------
ST_F32, ST_F16, ST_BF16 = 0, 1, 2
_ST_OF = {torch.float32: ST_F32, torch.float16: ST_F16, torch.bfloat16: ST_BF16}


def storage_code(t: torch.Tensor) -> int:
    try:
        return _ST_OF[t.dtype]
    except KeyError:
        raise ValueError("descriptors must be float32, float16 or bfloat16, not %s" % t.dtype)


def store_descriptors(x: torch.Tensor, dtype: Optional[torch.dtype]) -> torch.Tensor:
    """float32 descriptors -> their storage type (round-to-nearest-even), through the HIP casts."""
    if dtype is None or dtype == torch.float32:
        return x
    dev = _need_cuda(x)
    if x.dtype != torch.float32:
        raise ValueError("store_descriptors expects float32 input")
    if dtype == torch.bfloat16:
        return cast(x, BF16)
    if dtype != torch.float16:
        raise ValueError("descriptor storage must be float32, float16 or bfloat16")
    out = torch.empty(x.shape, dtype=torch.float16, device=dev)
    _lib.check(_lib.load().oibl_cast_f32_to_f16(_ptr(x), _ptr(out), x.numel(), _stream(dev)),
               "cast_f32_to_f16")
    return out


def load_descriptors(x: torch.Tensor) -> torch.Tensor:
    """Stored descriptors widened to float32 (exact)."""
    if x.dtype != torch.float16:
        return to_f32(x)
    dev = _need_cuda(x)
    out = torch.empty(x.shape, dtype=torch.float32, device=dev)
    _lib.check(_lib.load().oibl_cast_f16_to_f32(_ptr(x), _ptr(out), x.numel(), _stream(dev)),
               "cast_f16_to_f32")
    return out


def sum_l2_normalize(xs: torch.Tensor) -> torch.Tensor:
    """float32 [S][N][D] -> [N][D]: rows of xs[0] + xs[1] + ... L2-normalised."""
    dev = _need_cuda(xs)
    if xs.dtype != torch.float32 or xs.dim() != 3:
        raise ValueError("sum_l2_normalize expects a float32 [S][N][D] tensor")
    S, N, D = map(int, xs.shape)
    out = torch.empty((N, D), dtype=torch.float32, device=dev)
    _lib.check(_lib.load().oibl_sum_l2_normalize(_ptr(xs), S, N, D, _ptr(out), _stream(dev)),
               "sum_l2_normalize")
    return out


def resize_bilinear(x: torch.Tensor, size: Tuple[int, int]) -> torch.Tensor:
    """float32 [N][C][H][W] -> [N][C][H2][W2] with the arithmetic of
    F.interpolate(x, size=size, mode="bilinear", align_corners=False)."""
    dev = _need_cuda(x)
    if x.dtype != torch.float32 or x.dim() != 4:
        raise ValueError("resize_bilinear expects a float32 [N][C][H][W] tensor")
    N, Cc, H, W = map(int, x.shape)
    H2, W2 = int(size[0]), int(size[1])
    out = torch.empty((N, Cc, H2, W2), dtype=torch.float32, device=dev)
    _lib.check(_lib.load().oibl_resize_bilinear_nchw(_ptr(x), N, Cc, H, W, _ptr(out), H2, W2,
                                                     _stream(dev)), "resize_bilinear")
    return out


# ---- matching ---------------------------------------------------------------------------------
def _pad_dim(x: torch.Tensor) -> torch.Tensor:
    """Descriptor rows zero-padded to the next multiple of 64 dimensions (the K-tile of the distance
    kernels): zeros change neither norms nor dot products, so e.g. PCA(pca_n_components=16)
    descriptors match like the reference's."""
    d = int(x.shape[1])
    if d % 64 == 0:
        return x
    out = torch.zeros((x.shape[0], d + (-d) % 64), dtype=x.dtype, device=x.device)
    out[:, :d] = x
    return out


def pairwise_sqdist(x: torch.Tensor, y: torch.Tensor, precision=F32,
                    out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """dist[i][j] = |x_i|^2 + |y_j|^2 - 2 x_i.y_j for x [m][d], y [n][d] stored as float32, float16
    or bfloat16 (16-bit rows are widened exactly; see oibl_pairwise_sqdist_st)."""
    p = precision_code(precision)
    if p == F16R:
        raise ValueError("pairwise_sqdist: 'f16r' is a top-k arithmetic (filter + rescoring); a full matrix is "
                         "computed in 'f16mx', 'bf16x3' or 'fp32'")
    dev = _need_cuda(x, y)
    if out is not None and (not out.is_cuda or out.dtype != torch.float32 or out.dim() != 2
                            or out.stride(1) != 1 or out.device != dev):
        raise ValueError("pairwise_sqdist: `out` must be a float32 CUDA matrix with unit column stride")
    if x.dim() != 2 or y.dim() != 2:
        raise ValueError("pairwise_sqdist expects [m][d] and [n][d]")
    xs, ys = storage_code(x), storage_code(y)
    if int(y.shape[1]) != int(x.shape[1]):
        raise ValueError("pairwise_sqdist: dimension mismatch")
    x, y = _pad_dim(x), _pad_dim(y)
    m, d = map(int, x.shape)
    n = int(y.shape[0])
    if out is None:
        out = torch.empty((m, n), dtype=torch.float32, device=dev)
    if m == 0 or n == 0:
        return out
    lib = _lib.load()
    ws_bytes = lib.oibl_pairwise_st_workspace_bytes(m, n, d, p, xs, ys)
    ws = workspace(ws_bytes, dev, "pairwise")
    _lib.check(lib.oibl_pairwise_sqdist_st(_ptr(x), xs, m, _ptr(y), ys, n, d, p, _ptr(out),
                                           int(out.stride(0)), _ptr(ws), ws.numel(), _stream(dev)),
               "pairwise_sqdist")
    return out


def row_topk(vals: torch.Tensor, k: int, index_base: int = 0,
             idx_in: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """k smallest per row, ascending, lowest index first on ties -> (values [m][k], idx [m][k] int32)."""
    dev = _need_cuda(vals, idx_in)
    if vals.dtype != torch.float32 or vals.dim() != 2:
        raise ValueError("row_topk expects a float32 [m][n] tensor")
    if idx_in is not None and (idx_in.dtype != torch.int32 or idx_in.shape != vals.shape):
        raise ValueError("row_topk: idx_in must be int32 with the shape of vals")
    m, n = map(int, vals.shape)
    ov = torch.empty((m, k), dtype=torch.float32, device=dev)
    oi = torch.empty((m, k), dtype=torch.int32, device=dev)
    if m == 0:
        return ov, oi
    _lib.check(_lib.load().oibl_row_topk(_ptr(vals), _ptr(idx_in), m, n, int(vals.stride(0)), k,
                                         int(index_base), _ptr(ov), _ptr(oi), _stream(dev)),
               "row_topk")
    return ov, oi


def row_argsort(vals: torch.Tensor, want_values: bool = False, max_ws_bytes: int = 1 << 31):
    """Stable ascending argsort of every row of a float32 [m][n] device matrix -> int32 [m][n]
    (and the sorted values): torch.argsort(vals, dim=1, stable=True) on the GPU (oibl_row_argsort).
    Rows are sorted in groups so that the ping-pong workspace (16 bytes per element) stays below
    `max_ws_bytes`."""
    if not vals.is_cuda:
        raise _lib.OpenIBLAmdError("openibl_amd: row_argsort runs only on an AMD GPU (there is no CPU fallback)")
    dev = vals.device
    if vals.dtype != torch.float32 or vals.dim() != 2 or (vals.shape[1] > 1 and vals.stride(1) != 1):
        raise ValueError("row_argsort expects a float32 [m][n] tensor with unit column stride")
    m, n = map(int, vals.shape)
    idx = torch.empty((m, n), dtype=torch.int32, device=dev)
    sv = torch.empty((m, n), dtype=torch.float32, device=dev) if want_values else None
    if m == 0 or n == 0:
        return (idx, sv) if want_values else idx
    lib = _lib.load()
    rows = max(1, min(m, int(max_ws_bytes // (16 * n + 1024))))
    ws = workspace(lib.oibl_row_argsort_workspace_bytes(rows, n), dev, "argsort")
    for r0 in range(0, m, rows):
        r = min(rows, m - r0)
        _lib.check(lib.oibl_row_argsort(vals[r0:].data_ptr(), r, n, int(vals.stride(0)),
                                        idx[r0:].data_ptr(), None if sv is None else sv[r0:].data_ptr(),
                                        _ptr(ws), ws.numel(), _stream(dev)), "row_argsort")
    return (idx, sv) if want_values else idx


MINE_MAX_CACHE = 64          # C of oibl_mine_rows
MINE_MAX_POS_POOL = 1024     # pos_pool of oibl_mine_rows
MINE_LDS_EXCL = 4096         # exclusion entries per anchor the kernel searches in LDS (longer: global memory)


def mine_rows(dist: torch.Tensor, pos_off: torch.Tensor, pos_val: torch.Tensor, excl_off: torch.Tensor,
              excl_val: torch.Tensor, cache: Optional[torch.Tensor] = None, pos_pool: int = 1,
              jac: Optional[torch.Tensor] = None, csr_row: Optional[torch.Tensor] = None,
              max_ws_bytes: int = 1 << 31):
    """Hard-negative mining of the A anchor rows dist [A][G] (float32, device): oibl_mine_rows.

    pos_* / excl_* are CSR lists (int32, device; every row ascending, without repeats, inside [0, G)) with one row
    per anchor, or, with csr_row [A] int32, with any number of rows of which csr_row[a] belongs to anchor a.
    cache [A][C] int32 (-1 = none), jac [A][G] float32 are optional.  Returns (cand [A][G], cand_len [A],
    cache_pos [A][C], pos_ranked [A][pos_pool], pos_jac [A][pos_pool] or None), int32 but for pos_jac, on the
    device.  Rows are mined in groups so that the workspace (20 bytes per element) stays below `max_ws_bytes`."""
    if not dist.is_cuda:
        raise _lib.OpenIBLAmdError("openibl_amd: mine_rows runs only on an AMD GPU (there is no CPU fallback)")
    if dist.dtype != torch.float32 or dist.dim() != 2 or (dist.shape[1] > 1 and dist.stride(1) != 1):
        raise ValueError("mine_rows expects a float32 [A][G] tensor with unit column stride")
    dev = _need_cuda(pos_off, pos_val, excl_off, excl_val, cache, csr_row)
    if dev != dist.device:
        raise ValueError("openibl_amd: tensors on different devices")
    A, G = map(int, dist.shape)
    for t in (pos_off, pos_val, excl_off, excl_val, cache, csr_row):
        if t is not None and t.dtype != torch.int32:
            raise ValueError("mine_rows expects int32 lists, cache and csr_row")
    rows = int(pos_off.numel()) - 1
    if pos_off.dim() != 1 or excl_off.dim() != 1 or int(excl_off.numel()) != rows + 1 or rows < 0:
        raise ValueError("mine_rows: pos_off and excl_off must have one entry per CSR row plus one")
    if csr_row is None and rows != A:
        raise ValueError(f"mine_rows: {rows} CSR rows for {A} anchors (pass csr_row to select rows)")
    if csr_row is not None and tuple(csr_row.shape) != (A,):
        raise ValueError("mine_rows: csr_row must have one entry per anchor")
    C = 0 if cache is None else int(cache.shape[1])
    if cache is not None and (cache.dim() != 2 or int(cache.shape[0]) != A):
        raise ValueError("mine_rows: cache must be [A][C]")
    if C > MINE_MAX_CACHE or not 1 <= int(pos_pool) <= MINE_MAX_POS_POOL:
        raise ValueError(f"mine_rows: C <= {MINE_MAX_CACHE} and 1 <= pos_pool <= {MINE_MAX_POS_POOL}")
    if jac is not None and (not jac.is_cuda or jac.device != dev or jac.dtype != torch.float32
                            or tuple(jac.shape) != (A, G) or (G > 1 and jac.stride(1) != 1)):
        raise ValueError("mine_rows: jac must be a float32 [A][G] device tensor with unit column stride")
    pos_pool = int(pos_pool)
    cand = torch.empty((A, G), dtype=torch.int32, device=dev)
    cand_len = torch.empty((A,), dtype=torch.int32, device=dev)
    cache_pos = torch.empty((A, C), dtype=torch.int32, device=dev)
    pos_ranked = torch.empty((A, pos_pool), dtype=torch.int32, device=dev)
    pos_jac = torch.empty((A, pos_pool), dtype=torch.float32, device=dev) if jac is not None else None
    if A == 0 or G == 0:
        return cand, cand_len, cache_pos, pos_ranked, pos_jac
    # the kernel trusts the lists (they live on the device): one check of their frame here, one sync
    ok = torch.ones((), dtype=torch.bool, device=dev)
    for off, val in ((pos_off, pos_val), (excl_off, excl_val)):
        ok = ok & (off[0] >= 0) & (off[-1] <= val.numel()) & (off[1:] >= off[:-1]).all()
        if val.numel():
            ok = ok & (val.min() >= 0) & (val.max() < G)
    if csr_row is not None:
        ok = ok & (csr_row.min() >= 0) & (csr_row.max() < rows)
    if not bool(ok):
        raise ValueError("mine_rows: CSR offsets must ascend inside their value arrays, values lie in [0, G), "
                         "csr_row in [0, rows)")
    if pos_val.numel() == 0 or excl_val.numel() == 0:     # (an empty tensor has no address to pass)
        none = torch.zeros((1,), dtype=torch.int32, device=dev)
        pos_val = pos_val if pos_val.numel() else none
        excl_val = excl_val if excl_val.numel() else none
    lib = _lib.load()
    group = max(1, min(A, int(max_ws_bytes // (20 * G + 2048))))
    ws = workspace(lib.oibl_mine_rows_workspace_bytes(group, G), dev, "mining")
    for r0 in range(0, A, group):
        r = min(group, A - r0)
        # without csr_row the offsets of row r0 onward are the same arrays advanced by r0 entries
        _lib.check(lib.oibl_mine_rows(
            dist[r0:].data_ptr(), r, G, int(dist.stride(0)),
            None if csr_row is None else csr_row[r0:].data_ptr(),
            pos_off.data_ptr() + (4 * r0 if csr_row is None else 0), _ptr(pos_val),
            excl_off.data_ptr() + (4 * r0 if csr_row is None else 0), _ptr(excl_val),
            None if cache is None or C == 0 else cache[r0:].data_ptr(), C,
            None if jac is None else jac[r0:].data_ptr(), 0 if jac is None else int(jac.stride(0)), pos_pool,
            cand[r0:].data_ptr(), G, cand_len[r0:].data_ptr(),
            None if C == 0 else cache_pos[r0:].data_ptr(), pos_ranked[r0:].data_ptr(),
            None if pos_jac is None else pos_jac[r0:].data_ptr(), _ptr(ws), ws.numel(), _stream(dev)), "mine_rows")
    return cand, cand_len, cache_pos, pos_ranked, pos_jac


def first_hit_rank(topk_idx: torch.Tensor, gt_offsets: torch.Tensor, gt_values: torch.Tensor,
                   gallery_pids: Optional[torch.Tensor] = None, nms_window: int = 120) -> torch.Tensor:
    """Per query: rank of the first prediction that is a ground-truth neighbour (-1: none), with
    the reference's spatial NMS when gallery_pids is given.  All tensors int32 on the device."""
    dev = _need_cuda(topk_idx, gt_offsets, gt_values, gallery_pids)
    for t in (topk_idx, gt_offsets, gt_values, gallery_pids):
        if t is not None and t.dtype != torch.int32:
            raise ValueError("first_hit_rank expects int32 tensors")
    m, k = map(int, topk_idx.shape)
    if int(gt_offsets.numel()) != m + 1:
        raise ValueError("first_hit_rank: gt_offsets must have m + 1 entries")
    out = torch.empty((m,), dtype=torch.int32, device=dev)
    if m == 0:
        return out
    _lib.check(_lib.load().oibl_first_hit_rank(_ptr(topk_idx.contiguous()), m, k, _ptr(gt_offsets),
                                               _ptr(gt_values), _ptr(gallery_pids), int(nms_window),
                                               _ptr(out), _stream(dev)), "first_hit_rank")
    return out


def flag_to_host(flag_dev: torch.Tensor, ring: torch.Tensor, index: int) -> None:
    """The int32 device word `flag_dev` -> word `index` of the PINNED host tensor `ring`, by a kernel on the
    current stream (oibl_copy_words: no DMA-engine copy to queue behind a large input transfer).  The host
    reads ring[index] once an event recorded behind this call has fired."""
    dev = _need_cuda(flag_dev)
    if not ring.is_pinned() or ring.dtype != torch.int32 or flag_dev.dtype != torch.int32:
        raise ValueError("flag_to_host: ring must be a pinned int32 host tensor, the flag an int32 device tensor")
    _lib.check(_lib.load().oibl_copy_words(_ptr(flag_dev), ring.data_ptr() + 4 * int(index), 1, _stream(dev)),
               "copy_words")


def event_elapsed_ms(start: "torch.cuda.Event", stop: "torch.cuda.Event") -> float:
    """hipEventElapsedTime on the raw handles — works for events recorded by the event nodes of a
    replayed hipGraph, which torch's own bookkeeping does not see."""
    ms = C.c_float(0.0)
    _lib.check(_lib.load().oibl_event_elapsed_ms(int(start.cuda_event), int(stop.cuda_event),
                                                       C.byref(ms)), "event_elapsed_ms")
    return float(ms.value)


def set_match_ring(mode: int) -> None:
    """Test hook: ring-schedule distance kernel 0 = never, 1 = auto, 2 = whenever legal."""
    _lib.debug_hooks().oibl_debug_set_match_ring(int(mode))


def set_match_splitk(on: bool) -> None:
    """Test hook: allow / forbid the 2-way split-K contraction of the fused path's threshold sample."""
    _lib.debug_hooks().oibl_debug_set_match_splitk(1 if on else 0)


def sqdist_topk(x: torch.Tensor, y: torch.Tensor, k: int, index_base: int = 0, precision=F32,
                exact: bool = False, defer_check: bool = False):
    """k nearest rows of y (squared L2) for every row of x, without materialising the matrix:
    (values [m][k] ascending, indices [m][k] int32 = index_base + row of y).  Equals
    row_topk(pairwise_sqdist(x, y), k).  The fused bf16 path reports candidate-list overflow through
    a device flag; it is read here (one 4-byte copy) and the call repeated on the exact path.
    defer_check=True skips that host synchronisation and returns (values, indices, flag) with the
    int32 device flag: the caller reads it when it synchronises anyway and repeats with exact=True
    if it is set (sharded.sharded_topk ships it with the per-shard lists)."""
    p = precision_code(precision)
    dev = _need_cuda(x, y)
    if x.dim() != 2 or y.dim() != 2:
        raise ValueError("sqdist_topk expects [m][d] and [n][d]")
    if p == F16R:
        if x.shape[0] == 0 or y.shape[0] == 0:
            p = F32                                           # (nothing to prepare: the empty result below)
        else:
            return sqdist_topk_prepared(PreparedRows(x, F16R), PreparedRows(y, F16R), k, index_base=index_base,
                                        exact=exact, defer_check=defer_check)
    xs, ys = storage_code(x), storage_code(y)
    if int(y.shape[1]) != int(x.shape[1]):
        raise ValueError("sqdist_topk: dimension mismatch")
    x, y = _pad_dim(x), _pad_dim(y)
    m, d = map(int, x.shape)
    n = int(y.shape[0])
    ov = torch.full((m, k), float("inf"), dtype=torch.float32, device=dev)
    oi = torch.full((m, k), -1, dtype=torch.int32, device=dev)
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    if m == 0 or n == 0:
        return (ov, oi, flag) if defer_check else (ov, oi)
    lib = _lib.load()
    x, y = x.contiguous(), y.contiguous()
    ws_bytes = lib.oibl_sqdist_topk_st_workspace_bytes(m, n, d, k, p, xs, ys)
    ws = workspace(ws_bytes, dev, "sqdist_topk")

    def run(ex: int) -> None:
        _lib.check(lib.oibl_sqdist_topk_st(_ptr(x), xs, m, _ptr(y), ys, n, d, k, int(index_base), p, ex,
                                           _ptr(ov), _ptr(oi), _ptr(flag), _ptr(ws), ws.numel(),
                                           _stream(dev)), "sqdist_topk")

    if defer_check:
        run(1 if exact else 0)
        return ov, oi, flag
    for ex in ([1] if exact else [0, 1]):
        run(ex)
        if ex == 1 or int(flag.item()) == 0:
            break
    return ov, oi


def cluster_means(x: torch.Tensor, labels: torch.Tensor, centers: torch.Tensor) -> torch.Tensor:
    """Lloyd update step (oibl_cluster_means): centers[c] <- mean of the rows x[i] with labels[i] == c,
    in place (fp64 accumulation in point order, correctly rounded); a centre without points keeps its
    value.  Returns the int32 member counts [num_clusters]."""
    dev = _need_cuda(x, labels, centers)
    if x.dtype != torch.float32 or centers.dtype != torch.float32 or x.dim() != 2 or centers.dim() != 2 \
            or x.shape[1] != centers.shape[1] or not x.is_contiguous() or not centers.is_contiguous():
        raise ValueError("cluster_means expects contiguous float32 x [n][d] and centers [K][d]")
    lab = labels.reshape(-1).to(torch.int32).contiguous()
    if lab.numel() != x.shape[0]:
        raise ValueError("cluster_means: one label per row")
    counts = torch.zeros((centers.shape[0],), dtype=torch.int32, device=dev)
    _lib.check(_lib.load().oibl_cluster_means(_ptr(x), _ptr(lab), int(x.shape[0]), int(x.shape[1]),
                                              int(centers.shape[0]), _ptr(centers), _ptr(counts), _stream(dev)),
               "cluster_means")
    return counts


# ---- NetVLAD initialisation without a checkpoint ----------------------------------------------------
def local_descriptors(feat_nhwc: torch.Tensor, positions) -> torch.Tensor:
    """feat [N][h][w][C] (or [N][P][C]) bf16 / fp32, positions [N][S] integers in [0, P) (numpy or torch, host or
    device) -> [N*S][C] fp32: row n*S + s = F.normalize(feat[n, positions[n, s], :]) (examples/cluster.py:97-104;
    oibl_local_descriptors).  Only the sampled pixels are read.  The range of the positions is checked on the host
    BEFORE anything is launched (ValueError)."""
    dev = _need_cuda(feat_nhwc)
    if feat_nhwc.dim() not in (3, 4) or feat_nhwc.dtype not in (torch.bfloat16, torch.float32):
        raise ValueError("local_descriptors: feature map must be a bf16 or fp32 [N][h][w][C] / [N][P][C] tensor")
    N, C_ = int(feat_nhwc.shape[0]), int(feat_nhwc.shape[-1])
    if N == 0 or C_ == 0 or C_ % 64:
        raise ValueError(f"local_descriptors: {N} images of {C_} channels (C must be a positive multiple of 64)")
    P = feat_nhwc.numel() // (N * C_)
    pos = positions.detach().cpu() if torch.is_tensor(positions) else torch.as_tensor(positions)
    if pos.dim() != 2 or int(pos.shape[0]) != N or int(pos.shape[1]) == 0 or pos.is_floating_point() \
            or pos.dtype == torch.bool:
        raise ValueError(f"local_descriptors: positions must be integers [N = {N}][S >= 1], got {tuple(pos.shape)} "
                         f"{pos.dtype}")
    lo, hi = int(pos.min()), int(pos.max())
    if lo < 0 or hi >= P:
        raise ValueError(f"local_descriptors: positions must lie in [0, {P}) (got {lo} .. {hi})")
    S = int(pos.shape[1])
    pos_dev = pos.to(torch.int32).contiguous().to(dev)
    out = torch.empty((N * S, C_), dtype=torch.float32, device=dev)
    p = BF16 if feat_nhwc.dtype == torch.bfloat16 else F32
    _lib.check(_lib.load().oibl_local_descriptors(_ptr(feat_nhwc), N, P, C_, p, _ptr(pos_dev), S, _ptr(out),
                                                  _stream(dev)), "local_descriptors")
    return out


def assign_gap(descs: torch.Tensor, clsts: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor, float]:
    """descs [n][C], clsts [K][C] fp32 -> (clsts_assign [K][C] = clsts / |clsts|, gap [n] = best minus second best
    of the K products clsts_assign . desc, mean gap as a Python float = gap_sum / n in double): the arithmetic of
    NetVLAD._init_params (ibl/models/netvlad.py:35-40; oibl_assign_gap), without its [K][n] matrix.  Reading the
    mean synchronises with the stream."""
    dev = _need_cuda(descs, clsts)
    if descs.dtype != torch.float32 or clsts.dtype != torch.float32 or descs.dim() != 2 or clsts.dim() != 2 \
            or descs.shape[1] != clsts.shape[1]:
        raise ValueError("assign_gap expects contiguous float32 descs [n][C] and clsts [K][C]")
    n, C_, K = int(descs.shape[0]), int(descs.shape[1]), int(clsts.shape[0])
    if n < 1 or K < 2 or K > 256 or C_ == 0 or C_ % 64:
        raise ValueError(f"assign_gap: n = {n}, K = {K}, C = {C_}: needs n >= 1, 2 <= K <= 256 and C a positive "
                         f"multiple of 64")
    lib = _lib.load()
    ws = workspace(lib.oibl_assign_gap_workspace_bytes(n, K, C_), dev, "assign_gap")
    clsts_assign = torch.empty((K, C_), dtype=torch.float32, device=dev)
    gap = torch.empty((n,), dtype=torch.float32, device=dev)
    gap_sum = torch.empty((1,), dtype=torch.float64, device=dev)
    _lib.check(lib.oibl_assign_gap(_ptr(descs), n, _ptr(clsts), K, C_, _ptr(clsts_assign), _ptr(gap), _ptr(gap_sum),
                                   _ptr(ws), ws.numel(), _stream(dev)), "assign_gap")
    return clsts_assign, gap, float(gap_sum.item()) / n


class PreparedRows:
    """A descriptor matrix ready for matching in one precision: the rows the contraction reads and
    their fp32 squared norms (oibl_match_prepare).  Build it once for a matrix that is matched many
    times — the resident gallery shard — and hand it to sqdist_topk / sharded_topk in place of the
    tensor: the norm / operand pass (8 % of a 8192 x 81920 matching step) leaves the call."""

    def __init__(self, x: torch.Tensor, precision):
        p = precision_code(precision)
        dev = _need_cuda(x)
        if x.dim() != 2:
            raise ValueError("PreparedRows expects [rows][d]")
        x = _pad_dim(x.contiguous())
        st = storage_code(x)
        rows, d = map(int, x.shape)
        self.precision, self.shape, self.device = p, (rows, d), dev
        self.norms = torch.empty((rows,), dtype=torch.float32, device=dev)
        self.operand = x
        self.aux = None
        if p == F16R:
            # four parts: scaled fp16 rows (the filter pass), {2^-e, |x|, |residual|, 0} per row, the fp32 squared
            # norms, and the STORED rows themselves (fp32, fp16 or bf16: read again — widened exactly — by the rescoring)
            self._source = x
            self.operand = torch.empty((rows, d), dtype=torch.float16, device=dev)
            self.aux = torch.empty((rows, 4), dtype=torch.float32, device=dev)
            if rows:
                _lib.check(_lib.load().oibl_match_prepare_f16r_st(_ptr(x), st, rows, d, _ptr(self.norms), _ptr(self.aux),
                                                                  _ptr(self.operand), _stream(dev)), "match_prepare_f16r")
            return
        if rows == 0:
            return
        lib = _lib.load()
        nbytes = lib.oibl_match_operand_bytes(rows, d, p, st)
        buf = torch.empty((nbytes,), dtype=torch.uint8, device=dev) if nbytes else None
        _lib.check(lib.oibl_match_prepare(_ptr(x), st, rows, d, p, _ptr(self.norms), _ptr(buf),
                                          _stream(dev)), "match_prepare")
        self._source = x          # read in place when there is no operand copy
        if buf is not None:
            self.operand = buf

    @property
    def storage(self) -> int:
        """OIBL_ST_* of the rows an f16r rescoring reads (the stored descriptors)."""
        return storage_code(self._source) if self._source is not None else ST_F32

    def operand_rows(self) -> torch.Tensor:
        """The operand as a [rows][bytes per row] uint8 matrix (a view): what travels when prepared
        queries are exchanged between ranks instead of fp32 rows."""
        rows = self.shape[0]
        if self.precision == F16R:
            # one row per query: [d fp16 | 4 fp32 aux | d stored elements] — what a rank that extracted the query ships
            d = self.shape[1]
            es = self._source.element_size()
            return torch.cat([self.operand.view(torch.uint8).reshape(rows, 2 * d),
                              self.aux.view(torch.uint8).reshape(rows, 16),
                              self._source.view(torch.uint8).reshape(rows, es * d)], dim=1)
        per = self.shape[1] * (2 if self.precision == BF16 else 4)
        flat = self.operand.contiguous().view(torch.uint8).reshape(-1)
        return flat[: rows * per].view(rows, per)

    def rows(self, lo: int, hi: int) -> "PreparedRows":
        """Rows [lo, hi) as prepared rows of their own — views of every part, no copies (a query block of
        sharded_topk; ADVICE r05: operand_rows() + from_parts concatenated and re-split the whole f16r set)."""
        n = self.shape[0]
        lo, hi = max(0, min(int(lo), n)), max(0, min(int(hi), n))
        out = type(self).__new__(type(self))
        out.precision, out.device = self.precision, self.device
        out.shape = (hi - lo, self.shape[1])
        out.norms = self.norms[lo:hi]
        out.aux = None if self.aux is None else self.aux[lo:hi]
        out._source = None if self._source is None else self._source[lo:hi]
        if self.precision == F16R or self.operand.dim() == 2:
            out.operand = self.operand[lo:hi]
        else:                                     # a flat byte buffer of whole rows (oibl_match_prepare's operand)
            per = self.shape[1] * (2 if self.precision == BF16 else 4)
            out.operand = self.operand.view(torch.uint8).reshape(-1)[lo * per: hi * per]
        return out

    @classmethod
    def from_parts(cls, operand_rows: torch.Tensor, norms: torch.Tensor, d: int, precision,
                   source_dtype: Optional[torch.dtype] = None) -> "PreparedRows":
        """Re-assemble prepared rows from their exchanged parts (operand_rows() and .norms of one or
        several PreparedRows of the same precision, concatenated along dim 0).  f16r: `source_dtype` = the
        storage type of the rows behind the fp16 image (default float32; a 2-byte tail without it: float16)."""
        self = cls.__new__(cls)
        self.precision = precision_code(precision)
        self.device = operand_rows.device
        self.shape = (int(operand_rows.shape[0]), int(d) + (-int(d)) % 64)
        self.norms = norms.contiguous()
        self._source = None
        self.aux = None
        if self.precision == F16R:
            rows, dd = self.shape
            b = operand_rows
            tail = (int(b.shape[1]) - 2 * dd - 16) // dd
            if source_dtype is None:
                source_dtype = torch.float32 if tail == 4 else torch.float16
            if tail != (4 if source_dtype == torch.float32 else 2):
                raise ValueError("PreparedRows.from_parts: row width does not match the f16r layout of %s rows" % source_dtype)
            self.operand = b[:, : 2 * dd].contiguous().view(torch.float16).reshape(rows, dd)
            self.aux = b[:, 2 * dd: 2 * dd + 16].contiguous().view(torch.float32).reshape(rows, 4)
            self._source = b[:, 2 * dd + 16:].contiguous().view(source_dtype).reshape(rows, dd)
            return self
        self.operand = operand_rows.contiguous()
        return self


def sqdist_topk_prepared(x: "PreparedRows", y: "PreparedRows", k: int, index_base: int = 0,
                         exact: bool = False, defer_check: bool = False):
    """sqdist_topk on prepared operands (same results, bit for bit)."""
    if x.precision != y.precision or x.shape[1] != y.shape[1]:
        raise ValueError("sqdist_topk_prepared: operands prepared for different precisions / dimensions")
    dev, p = x.device, x.precision
    (m, d), n = x.shape, y.shape[0]
    ov = torch.full((m, k), float("inf"), dtype=torch.float32, device=dev)
    oi = torch.full((m, k), -1, dtype=torch.int32, device=dev)
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    if m == 0 or n == 0:
        return (ov, oi, flag) if defer_check else (ov, oi)
    lib = _lib.load()
    if p == F16R:
        xs, ys = x.storage, y.storage
        ws = workspace(lib.oibl_sqdist_topk_f16r_st_workspace_bytes(m, n, d, k, xs, ys), dev, "sqdist_topk")
        xsrc, ysrc = x._source.contiguous(), y._source.contiguous()
        xop, xaux, xnorm = x.operand.contiguous(), x.aux.contiguous(), x.norms.contiguous()

        def run(ex: int) -> None:
            _lib.check(lib.oibl_sqdist_topk_f16r_st(_ptr(xop), _ptr(xaux), _ptr(xnorm), _ptr(xsrc), xs, m,
                                                    _ptr(y.operand), _ptr(y.aux), _ptr(y.norms), _ptr(ysrc), ys, n,
                                                    d, k, int(index_base), ex, _ptr(ov), _ptr(oi), _ptr(flag),
                                                    _ptr(ws), ws.numel(), _stream(dev)), "sqdist_topk_f16r")
    else:
        ws = workspace(lib.oibl_sqdist_topk_prepared_workspace_bytes(m, n, d, k, p), dev, "sqdist_topk")

    def run_generic(ex: int) -> None:
        _lib.check(lib.oibl_sqdist_topk_prepared(_ptr(x.operand), _ptr(x.norms), m, _ptr(y.operand),
                                                 _ptr(y.norms), n, d, k, int(index_base), p, ex, _ptr(ov),
                                                 _ptr(oi), _ptr(flag), _ptr(ws), ws.numel(), _stream(dev)),
                   "sqdist_topk_prepared")

    if p != F16R:
        run = run_generic
    if defer_check:
        run(1 if exact else 0)
        return ov, oi, flag
    for ex in ([1] if exact else [0, 1]):
        run(ex)
        if ex == 1 or int(flag.item()) == 0:
            break
    return ov, oi


# ---- the two stages of the f16r top-k, for gallery-sharded matching (sharded.py) ----------------------------
def f16r_members(k: int) -> int:
    """Member slots per query of an f16r selection (K2)."""
    return int(_lib.load().oibl_f16r_members(int(k)))


def f16r_fused(m: int, n: int, d: int, k: int) -> bool:
    return bool(_lib.load().oibl_f16r_fused(int(m), int(n), int(d), int(k)))


def f16r_filter_select(x: "PreparedRows", y: "PreparedRows", k: int, index_base: int = 0):
    """Stage 1 (sample thresholds, fp16 filter pass, selection): (lval [m][K2] filter distances, lidx [m][K2] int32
    global indices (-1 paddings), ymax [2] = the gallery's largest row norm and fp16 residual norm, flag [1])."""
    if x.precision != F16R or y.precision != F16R:
        raise ValueError("f16r_filter_select expects operands prepared for 'f16r'")
    dev = x.device
    (m, d), n = x.shape, y.shape[0]
    K2 = f16r_members(k)
    lval = torch.empty((m, K2), dtype=torch.float32, device=dev)
    lidx = torch.empty((m, K2), dtype=torch.int32, device=dev)
    ymax = torch.zeros(2, dtype=torch.float32, device=dev)
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    lib = _lib.load()
    ws = workspace(lib.oibl_sqdist_topk_f16r_workspace_bytes(m, n, d, k), dev, "sqdist_topk")
    _lib.check(lib.oibl_f16r_filter_select(_ptr(x.operand), _ptr(x.aux), _ptr(x.norms), m, _ptr(y.operand), _ptr(y.aux),
                                           _ptr(y.norms), n, d, k, int(index_base), _ptr(lval), _ptr(lidx), _ptr(ymax),
                                           _ptr(flag), _ptr(ws), ws.numel(), _stream(dev)), "f16r_filter_select")
    return lval, lidx, ymax, flag


def f16r_keep_members(lval: torch.Tensor, lidx: torch.Tensor, k: int, thr: torch.Tensor, x: "PreparedRows",
                      ymax_all: torch.Tensor) -> None:
    """In place: entries of lidx whose filter distance exceeds thr[row] + 2 eps (eps: x's rows against the maxima
    over all shards, ymax_all [W][2]) become -1."""
    dev = _need_cuda(lval, lidx, thr, ymax_all)
    m = int(lval.shape[0])
    _lib.check(_lib.load().oibl_f16r_keep_members(_ptr(lval), _ptr(lidx), m, int(k), _ptr(thr.contiguous()), _ptr(x.norms),
                                                  _ptr(x.aux), _ptr(ymax_all.contiguous()), int(ymax_all.shape[0]),
                                                  int(x.shape[1]), _stream(dev)), "f16r_keep_members")


def f16r_rescore(x: "PreparedRows", y: "PreparedRows", lidx: torch.Tensor, k: int, index_base: int = 0):
    """Stage 2: exact distances of the listed members, the k smallest (distance, index) per query."""
    dev = x.device
    m, d = x.shape
    ov = torch.full((m, k), float("inf"), dtype=torch.float32, device=dev)
    oi = torch.full((m, k), -1, dtype=torch.int32, device=dev)
    if m == 0 or y.shape[0] == 0:
        return ov, oi
    lidx = lidx.contiguous()
    _lib.check(_lib.load().oibl_f16r_rescore_st(_ptr(x._source.contiguous()), x.storage, _ptr(x.norms.contiguous()), m,
                                                _ptr(y._source), y.storage, _ptr(y.norms), d, int(k),
                                                int(lidx.shape[1]), int(index_base), _ptr(lidx), _ptr(ov), _ptr(oi),
                                                _stream(dev)), "f16r_rescore")
    return ov, oi


def gemm_nt(a: torch.Tensor, b: torch.Tensor, regstage: bool = False) -> torch.Tensor:
    """Diagnostic: C = A . B^T on the MFMA core; A [M][K], B [N][K] both bf16 or both fp32."""
    dev = _need_cuda(a, b)
    if a.dtype != b.dtype or a.dtype not in (torch.bfloat16, torch.float32):
        raise ValueError("gemm_nt: operands must both be bf16 or both fp32")
    p = BF16 if a.dtype == torch.bfloat16 else F32
    M, K = map(int, a.shape)
    N = int(b.shape[0])
    c = torch.empty((M, N), dtype=torch.float32, device=dev)
    _lib.check(_lib.load().oibl_gemm_nt(_ptr(a), M, _ptr(b), N, K, p | (0x100 if regstage else 0),
                                        _ptr(c), N, _stream(dev)), "gemm_nt")
    return c


# ---------------------------------------------------------------------------------------------
# k-reciprocal re-ranking from descriptor rows, one wrapper per stage (csrc/rerank.hip; the
# stages are put together by openibl_amd.rerank.re_ranking_features)
# ---------------------------------------------------------------------------------------------
RERANK_MAX_K1 = 31
RERANK_MAX_K2 = 8


def rerank_half(k1: int) -> int:
    """round(k1 / 2) as the reference rounds it (np.around: halves to even)."""
    return int(round(k1 / 2.0))


def rerank_check_limits(k1: int, k2: int) -> None:
    """ValueError for parameters beyond what the kernels are built for (never a silent truncation)."""
    if int(k1) != k1 or not 1 <= k1 <= RERANK_MAX_K1:
        raise ValueError(f"re-ranking on the device is built for 1 <= k1 <= {RERANK_MAX_K1} (got k1={k1!r})")
    if int(k2) != k2 or not 1 <= k2 <= RERANK_MAX_K2:
        raise ValueError(f"re-ranking on the device is built for 1 <= k2 <= {RERANK_MAX_K2} (got k2={k2!r})")


def rerank_set_stride(k1: int, half: Optional[int] = None) -> int:
    """Slots per item of the set arrays: (k1 + 1)(half + 2), the most members an expanded set can have."""
    rerank_check_limits(k1, 1)
    return (k1 + 1) * ((rerank_half(k1) if half is None else int(half)) + 2)


def _i32(t: torch.Tensor, what: str) -> None:
    if t.dtype != torch.int32:
        raise ValueError(f"{what} must be int32")


def rerank_row_extremes(x: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """x [n][d] float32 -> (norms [n] = |x_i|^2, rowmax [n] = max_r D[r][i]^2) with D the squared-L2 matrix of x
    against itself, contracted in fp32 and never written."""
    dev = _need_cuda(x)
    if x.dtype != torch.float32 or x.dim() != 2:
        raise ValueError("rerank_row_extremes expects a float32 [n][d] tensor")
    n, d = map(int, x.shape)
    norms = torch.empty((n,), dtype=torch.float32, device=dev)
    rowmax = torch.empty((n,), dtype=torch.float32, device=dev)
    if n == 0:
        return norms, rowmax
    lib = _lib.load()
    ws = workspace(lib.oibl_rerank_row_extremes_workspace_bytes(n, d), dev, "rerank")
    _lib.check(lib.oibl_rerank_row_extremes(_ptr(x), n, d, _ptr(norms), _ptr(rowmax), _ptr(ws), ws.numel(),
                                            _stream(dev)), "rerank_row_extremes")
    return norms, rowmax


def rerank_sets(rank: torch.Tensor, k1: int, half: Optional[int] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """rank [n][>= k1 + 1] int32 (nearest first, the item itself included) -> (idx [n][stride] int32: the expanded
    k-reciprocal set of every item, ascending, slots beyond the count undefined; cnt [n] int32)."""
    rerank_check_limits(k1, 1)
    dev = _need_cuda(rank)
    _i32(rank, "rerank_sets: rank")
    half = rerank_half(k1) if half is None else int(half)
    n, ld = map(int, rank.shape)
    stride = rerank_set_stride(k1, half)
    idx = torch.empty((n, stride), dtype=torch.int32, device=dev)
    cnt = torch.zeros((n,), dtype=torch.int32, device=dev)
    if n:
        _lib.check(_lib.load().oibl_rerank_sets(_ptr(rank), ld, n, int(k1), half, _ptr(idx), _ptr(cnt), stride,
                                                _stream(dev)), "rerank_sets")
    return idx, cnt


def rerank_weights(x: torch.Tensor, norms: torch.Tensor, rowmax: torch.Tensor, idx: torch.Tensor,
                   cnt: torch.Tensor) -> torch.Tensor:
    """val [n][stride] float32: exp(-D[i][c]^2 / rowmax[i]) over the members c of item i, normalised to sum 1."""
    dev = _need_cuda(x, norms, rowmax, idx, cnt)
    _i32(idx, "rerank_weights: idx")
    _i32(cnt, "rerank_weights: cnt")
    if x.dtype != torch.float32 or norms.dtype != torch.float32 or rowmax.dtype != torch.float32:
        raise ValueError("rerank_weights expects float32 rows, norms and row maxima")
    n, d = map(int, x.shape)
    val = torch.empty(idx.shape, dtype=torch.float32, device=dev)
    if n:
        _lib.check(_lib.load().oibl_rerank_weights(_ptr(x), _ptr(norms), _ptr(rowmax), n, d, _ptr(idx), _ptr(cnt),
                                                   int(idx.shape[1]), _ptr(val), _stream(dev)), "rerank_weights")
    return val


def rerank_expand(rank: torch.Tensor, k2: int, idx: torch.Tensor, val: torch.Tensor, cnt: torch.Tensor):
    """The k2 query expansion: (idx2, val2, cnt2) with row i the mean of the sparse rows of the k2 nearest items of
    i (rank[i][:k2]), stride k2 * stride."""
    rerank_check_limits(1, k2)
    dev = _need_cuda(rank, idx, val, cnt)
    for t, what in ((rank, "rank"), (idx, "idx"), (cnt, "cnt")):
        _i32(t, "rerank_expand: " + what)
    n, ld = map(int, rank.shape)
    stride = int(idx.shape[1])
    stride2 = int(k2) * stride
    idx2 = torch.empty((n, stride2), dtype=torch.int32, device=dev)
    val2 = torch.empty((n, stride2), dtype=torch.float32, device=dev)
    cnt2 = torch.zeros((n,), dtype=torch.int32, device=dev)
    if n:
        _lib.check(_lib.load().oibl_rerank_expand(_ptr(rank), ld, n, int(k2), _ptr(idx), _ptr(val), _ptr(cnt), stride,
                                                  _ptr(idx2), _ptr(val2), _ptr(cnt2), stride2, _stream(dev)),
                   "rerank_expand")
    return idx2, val2, cnt2


def rerank_invert(idx: torch.Tensor, val: torch.Tensor, cnt: torch.Tensor):
    """The inverted index of the sparse rows: (col_off [n + 1] int32, inv_row [nnz] int32, inv_val [nnz] float32) —
    column c is held by rows inv_row[col_off[c]:col_off[c + 1]], ascending.  Reads the total count back (one
    integer) to size the outputs."""
    dev = _need_cuda(idx, val, cnt)
    _i32(idx, "rerank_invert: idx")
    _i32(cnt, "rerank_invert: cnt")
    n, stride = map(int, idx.shape)
    nnz = int(cnt.sum(dtype=torch.int64).item()) if n else 0
    col_off = torch.zeros((n + 1,), dtype=torch.int32, device=dev)
    inv_row = torch.empty((max(nnz, 1),), dtype=torch.int32, device=dev)
    inv_val = torch.empty((max(nnz, 1),), dtype=torch.float32, device=dev)
    if n:
        lib = _lib.load()
        ws = workspace(lib.oibl_rerank_invert_workspace_bytes(n, nnz), dev, "rerank")
        _lib.check(lib.oibl_rerank_invert(_ptr(idx), _ptr(val), _ptr(cnt), stride, n, nnz, _ptr(col_off),
                                          _ptr(inv_row), _ptr(inv_val), _ptr(ws), ws.numel(), _stream(dev)),
                   "rerank_invert")
    return col_off, inv_row[:nnz], inv_val[:nnz]


def rerank_jaccard(idx: torch.Tensor, val: torch.Tensor, cnt: torch.Tensor, col_off: torch.Tensor,
                   inv_row: torch.Tensor, inv_val: torch.Tensor, rowmax: torch.Tensor, dist: torch.Tensor,
                   lambda_value: float) -> torch.Tensor:
    """dist [Q][G] float32 holds the squared distances of the query rows (items 0..Q-1) to the gallery rows (items
    Q..Q+G-1); it is overwritten with (1 - lambda) * jaccard + lambda * dist^2 / rowmax[i] and returned."""
    dev = _need_cuda(idx, val, cnt, col_off, inv_row, inv_val, rowmax, dist)
    if dist.dtype != torch.float32 or dist.dim() != 2:
        raise ValueError("rerank_jaccard: dist must be a float32 [Q][G] matrix")
    Q, G = map(int, dist.shape)
    if Q + G != int(cnt.shape[0]):
        raise ValueError("rerank_jaccard: dist must be [Q][G] with Q + G = the number of items")
    if Q == 0 or G == 0:
        return dist
    import numpy as _np
    lam = float(_np.float32(lambda_value))
    oml = float(_np.float32(1.0 - lambda_value))
    lib = _lib.load()
    ws = workspace(lib.oibl_rerank_jaccard_workspace_bytes(Q, G), dev, "rerank")
    _lib.check(lib.oibl_rerank_jaccard(_ptr(idx), _ptr(val), _ptr(cnt), int(idx.shape[1]), _ptr(col_off),
                                       _ptr(inv_row), _ptr(inv_val), _ptr(rowmax), Q, G, oml, lam, _ptr(dist),
                                       int(dist.stride(0)), _ptr(ws), ws.numel(), _stream(dev)), "rerank_jaccard")
    return dist


# ---------------------------------------------------------------------------------------------
JITTER_OUT = {"uint8": 0, "float": 1}     # OIBL_JITTER_U8_NHWC, OIBL_JITTER_F32_NCHW
JITTER_RECORD_WORDS = 8                   # a record: four op codes, three fp32 factors (their bits), the hue byte
JITTER_MAX_PIXELS = 1 << 28


def color_jitter(u8: torch.Tensor, params: Optional[torch.Tensor], out: str = "float", mean=REF_MEAN,
                 std=REF_STD) -> torch.Tensor:
    """Training colour jitter of a raw batch on the device (oibl_color_jitter_u8): u8 [N][H][W][3] uint8, `params`
    int32 [N][8] — one record per image: the op codes in application order (0 brightness, 1 contrast, 2 saturation,
    3 hue, -1 skip), the bits of the fp32 brightness / contrast / saturation factors, the hue shift byte
    (openibl_amd.augment.ColorJitter.draw builds them) — or None for no jitter.
    out='uint8': the jittered images [N][H][W][3], PIL's bits; out='float': [N][3][H][W] float32, the loader's
    ToTensor + Normalize of those bytes ((u / 255 - mean) / std): what forward_train takes."""
    if out not in JITTER_OUT:
        raise ValueError(f"color_jitter: out must be 'float' or 'uint8', not {out!r}")
    if u8.dtype != torch.uint8:
        raise ValueError(f"color_jitter expects a uint8 batch, got {u8.dtype}")
    if u8.dim() != 4 or u8.shape[3] != 3 or min(u8.shape) < 1:
        raise ValueError(f"color_jitter expects [N][H][W][3], got {tuple(u8.shape)}")
    N, H, W, _ = u8.shape
    if H * W > JITTER_MAX_PIXELS or N > 65535:
        raise ValueError(f"color_jitter: N <= 65535 and H * W <= 2^28, got {tuple(u8.shape)}")
    if params is not None:
        if params.dtype != torch.int32:
            raise ValueError(f"color_jitter: params must be int32 records, got {params.dtype}")
        if tuple(params.shape) != (N, JITTER_RECORD_WORDS):
            raise ValueError(f"color_jitter: params must be [{N}][{JITTER_RECORD_WORDS}], got {tuple(params.shape)}")
    if not u8.is_contiguous() or (params is not None and not params.is_contiguous()):
        raise ValueError("openibl_amd: tensors must be contiguous")
    dev = _need_cuda(u8, params)
    lib = _lib.load()
    if out == "uint8":
        res = torch.empty((N, H, W, 3), dtype=torch.uint8, device=dev)
    else:
        res = torch.empty((N, 3, H, W), dtype=torch.float32, device=dev)
    ws = None
    if params is not None:
        ws = workspace(lib.oibl_color_jitter_u8_workspace_bytes(N, H, W), dev, slot="color_jitter")
    m3 = (C.c_float * 3)(*[float(v) for v in mean])
    s3 = (C.c_float * 3)(*[float(v) for v in std])
    _lib.check(lib.oibl_color_jitter_u8(_ptr(u8), N, H, W, _ptr(params), JITTER_OUT[out], m3, s3, _ptr(res),
                                        _ptr(ws), 0 if ws is None else ws.numel(), _stream(dev)), "color_jitter_u8")
    return res


# ---------------------------------------------------------------------------------------------
RESIZE_MAX_SCALE = 16         # RS_MAX_SCALE of csrc/resize_tables.h: the largest in / out per axis
RESIZE_MAX_DIM = 32768


def _resize_ksize(in_size: int, out_size: int) -> int:
    """Entries per row of an axis's coefficient table: 2 ceil(max(in / out, 1)) + 1 (PIL's ksize, bilinear)."""
    import math
    return int(math.ceil(max(in_size / out_size, 1.0))) * 2 + 1


def resize_u8_tables(in_size: int, out_size: int, device=None) -> Tuple[torch.Tensor, torch.Tensor]:
    """The tables of one axis of the device resize (oibl_resize_u8_tables), built by the kernel: int32
    bounds [out_size][2] = {first source sample, taps} and int32 coeff [out_size][ksize], the weights times 2^22."""
    in_size, out_size = int(in_size), int(out_size)
    if not (1 <= in_size <= RESIZE_MAX_DIM and 1 <= out_size <= RESIZE_MAX_DIM):
        raise ValueError(f"resize_u8_tables: sizes must be in [1, {RESIZE_MAX_DIM}], got {in_size} -> {out_size}")
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    lib = _lib.load()
    ksize = _resize_ksize(in_size, out_size)
    bounds = torch.empty((out_size, 2), dtype=torch.int32, device=dev)
    coeff = torch.empty((out_size, ksize), dtype=torch.int32, device=dev)
    got = C.c_int(0)
    with torch.cuda.device(dev):
        _lib.check(lib.oibl_resize_u8_tables(in_size, out_size, _ptr(bounds), _ptr(coeff), ksize, C.byref(got),
                                             _stream(dev)), "resize_u8_tables")
    assert got.value == ksize
    return bounds, coeff


def _resize_result(N, H2, W2, out, mean, std, dev):
    """What the two uint8 resizes hand their C calls alike: the result for out = 'uint8' or 'float', mean and std."""
    if out == "uint8":
        res = torch.empty((N, H2, W2, 3), dtype=torch.uint8, device=dev)
    else:
        res = torch.empty((N, 3, H2, W2), dtype=torch.float32, device=dev)
    return res, (C.c_float * 3)(*[float(v) for v in mean]), (C.c_float * 3)(*[float(v) for v in std])


def resize_u8(u8: torch.Tensor, size, out: str = "uint8", mean=REF_MEAN, std=REF_STD) -> torch.Tensor:
    """Bilinear resize of a raw batch on the device (oibl_resize_u8), PIL's bits: u8 [N][H][W][3] uint8,
    size = (height, width) of the result.  It is `Image.resize((width, height), Image.BILINEAR)` of every image —
    what the reference's Resize does on the host — bit for bit.  out='uint8': [N][height][width][3];
    out='float': [N][3][height][width] float32, the loader's ToTensor + Normalize of those bytes
    ((u / 255 - mean) / std).  An axis may shrink by a factor of at most RESIZE_MAX_SCALE (the source rows of a
    tile are kept in LDS); upscaling is not limited."""
    if out not in JITTER_OUT:
        raise ValueError(f"resize_u8: out must be 'float' or 'uint8', not {out!r}")
    if u8.dtype != torch.uint8:
        raise ValueError(f"resize_u8 expects a uint8 batch, got {u8.dtype}")
    if u8.dim() != 4 or u8.shape[3] != 3 or min(u8.shape) < 1:
        raise ValueError(f"resize_u8 expects [N][H][W][3], got {tuple(u8.shape)}")
    if not isinstance(size, (tuple, list)) or len(size) != 2:
        raise ValueError(f"resize_u8: size must be (height, width), got {size!r}")
    H2, W2 = int(size[0]), int(size[1])
    N, H, W, _ = u8.shape
    if H2 < 1 or W2 < 1:
        raise ValueError(f"resize_u8: the target size must be positive, got {H2} x {W2}")
    if max(H, W, H2, W2) > RESIZE_MAX_DIM or N > 65535:
        raise ValueError(f"resize_u8: N <= 65535 and every size <= {RESIZE_MAX_DIM}, got {tuple(u8.shape)} -> "
                         f"{H2} x {W2}")
    if H > RESIZE_MAX_SCALE * H2 or W > RESIZE_MAX_SCALE * W2:
        raise ValueError(f"resize_u8: {H} x {W} -> {H2} x {W2} shrinks an axis by more than the limit of "
                         f"{RESIZE_MAX_SCALE}")
    if not u8.is_contiguous():
        raise ValueError("openibl_amd: tensors must be contiguous")
    dev = _need_cuda(u8)
    lib = _lib.load()
    res, m3, s3 = _resize_result(N, H2, W2, out, mean, std, dev)
    ws = workspace(lib.oibl_resize_u8_workspace_bytes(N, H, W, H2, W2), dev, slot="resize_u8")
    _lib.check(lib.oibl_resize_u8(_ptr(u8), N, H, W, H2, W2, JITTER_OUT[out], m3, s3, _ptr(res), _ptr(ws),
                                  ws.numel(), _stream(dev)), "resize_u8")
    return res


# ---------------------------------------------------------------------------------------------
def _align256(v: int) -> int:
    return (v + 255) // 256 * 256


last_jpeg_route = None     # "serial" or "chunked": the route the last `decode_jpeg` that launched something took
last_jpeg_rounds = None    # chunked: int32 [S] on the device, the settle rounds of every segment (a view of the
                           # workspace, valid until the next call)


def decode_jpeg(batch, check: bool = True, scan: str = "auto", chunk_bytes=None):
    """Decode a `openibl_amd.jpeg.JpegBatch` on the device (oibl_jpeg_decode / oibl_jpeg_decode_chunked):
    [N][H][W][3] uint8, the bytes of `np.asarray(Image.open(f).convert('RGB'))` for every file.  The files the device
    does not decode (progressive, CMYK, not a JPEG, ...) were decoded on the host when the batch was built and are
    copied into their places.
    scan: "serial" gives every segment (a restart interval, or a whole scan) one lane; "chunked" cuts every segment
    into chunks of `chunk_bytes` raw bytes (default: `jpeg.CHUNK_BYTES`, more where the longest segment would have
    more than 1024 chunks) with a lane each — the same bits, for files without restart markers; "auto" takes the
    chunked route when the batch's longest segment has at least `jpeg.CHUNKED_MIN_BYTES` bytes.
    check=True reads the per-image status back (one host sync) and raises ValueError naming the damaged images;
    check=False returns (pixels, status) without a sync: status int32 [N], 0 ok (`jpeg.STATUS_TEXT`), 0 for the
    host-decoded images."""
    from . import jpeg as _jpeg
    if not isinstance(batch, _jpeg.JpegBatch):
        raise ValueError(f"decode_jpeg expects a JpegBatch (openibl_amd.jpeg.collate), got {type(batch).__name__}")
    route, cb = _jpeg_route("decode_jpeg", batch, scan, chunk_bytes)
    dev = _need_cuda(batch.scan, batch.records, batch.segments, batch.host_pixels, batch.dev_index,
                     batch.host_index)
    N, H, W = batch.n, batch.height, batch.width
    nd, nh = int(batch.records.shape[0]), int(batch.host_pixels.shape[0])
    if nd + nh != N or batch.records.shape[1:] != (_jpeg.REC_BYTES,) or batch.host_pixels.shape[1:] != (H, W, 3):
        raise ValueError(f"decode_jpeg: inconsistent batch: {nd} records + {nh} host images for N = {N}")
    status = torch.zeros(N, dtype=torch.int32, device=dev)
    pixels = None
    if nd:
        if not (_jpeg.MIN_WIDTH <= W <= _jpeg.MAX_DIM and 1 <= H <= _jpeg.MAX_DIM and nd <= 65535):
            raise ValueError(f"decode_jpeg: {nd} images of {H} x {W}: at most 65535 of at least "
                             f"{_jpeg.MIN_WIDTH} and at most {_jpeg.MAX_DIM} pixels per side")
        lib = _lib.load()
        S = int(batch.segments.shape[0])
        pixels = torch.empty((nd, H, W, 3), dtype=torch.uint8, device=dev)
        coef_bytes = nd * 3 * _jpeg.plane_blocks(H, W) * 64 * 2     # int16 coef[nd][3][Bh][Bw][64]
        if cb:
            _jpeg_launch(batch, pixels, status, route, coef_bytes,
                         lib.oibl_jpeg_decode_chunked_workspace_bytes(nd, H, W, S, cb), lib.oibl_jpeg_decode_chunked,
                         "jpeg_decode_chunked", (H, W, cb))
        else:
            _jpeg_launch(batch, pixels, status, route, coef_bytes, lib.oibl_jpeg_decode_workspace_bytes(nd, H, W, S),
                         lib.oibl_jpeg_decode, "jpeg_decode", (H, W))
    if nh:
        out = torch.empty((N, H, W, 3), dtype=torch.uint8, device=dev)
        out[batch.host_index] = batch.host_pixels
        if nd:
            out[batch.dev_index] = pixels
        pixels = out
    if not check:
        return pixels, status
    _raise_damaged("decode_jpeg", status)
    return pixels


def _jpeg_route(what, batch, scan, chunk_bytes):
    """(route, chunk_bytes) of a decode call: route "serial" or "chunked" — "auto" looks at the batch's longest
    segment — and the bytes of a lane's chunk, 0 on the serial route."""
    from . import jpeg as _jpeg
    if scan not in _jpeg.SCAN_ROUTES:
        raise ValueError(f"{what}: scan must be one of {_jpeg.SCAN_ROUTES}, not {scan!r}")
    if chunk_bytes is not None and not 4 <= int(chunk_bytes) <= 65536:
        raise ValueError(f"{what}: chunk_bytes {chunk_bytes} must be in [4, 65536]")
    if scan == "auto":
        scan = "chunked" if batch.max_segment_bytes >= _jpeg.CHUNKED_MIN_BYTES else "serial"
    if scan != "chunked":
        return scan, 0
    if chunk_bytes is not None:
        return scan, int(chunk_bytes)
    return scan, min(65536, max(_jpeg.CHUNK_BYTES, -(-batch.max_segment_bytes // _jpeg.MAX_CHUNK_LANES)))


def _jpeg_rounds(ws, coef_bytes, S):
    """The settle rounds of the chunked route, int32 [S], as a view of a decode call's workspace `ws` (uint8).  The
    only place in Python that knows the workspace of csrc/jpeg.hip (jpeg_layout): the coefficients, int32 segment
    status [S], int32 rounds [S], the planes, each region on a multiple of 256 bytes
    (tests/test_jpeg_chunked_cpu.py holds it to the C workspace queries)."""
    at = _align256(coef_bytes) + _align256(4 * S)
    return ws[at:at + 4 * S].view(torch.int32)


def _jpeg_launch(batch, out, status, route, coef_bytes, need, entry, name, geometry):
    """The device's share of a decode call: `entry` (one of the three C decoders; `geometry` is what it takes between
    the image count and the output) writes the pixels to `out` and the statuses to the batch positions `dev_index` of
    `status`; the route and the rounds of the call become `last_jpeg_route` and `last_jpeg_rounds`."""
    global last_jpeg_route, last_jpeg_rounds
    dev = status.device
    nd, S = int(batch.records.shape[0]), int(batch.segments.shape[0])
    st = status if nd == batch.n else torch.empty(nd, dtype=torch.int32, device=dev)
    ws = workspace(need, dev, slot="jpeg_decode")
    _lib.check(entry(_ptr(batch.scan), batch.scan.numel(), _ptr(batch.records), _ptr(batch.segments), S,
                     batch.max_segments, nd, *geometry, _ptr(out), _ptr(st), _ptr(ws), ws.numel(), _stream(dev)), name)
    last_jpeg_rounds = _jpeg_rounds(ws, coef_bytes, S) if route == "chunked" else None
    last_jpeg_route = route
    if st is not status:
        status[batch.dev_index] = st


# ---------------------------------------------------------------------------------------------
def _mixed_sizes(sizes, what: str):
    """sizes (tensor, numpy or a list of (H, W)) -> a contiguous int32 [N][2] numpy array on the host."""
    import numpy as np
    if torch.is_tensor(sizes):
        sizes = sizes.cpu().numpy()
    sizes = np.ascontiguousarray(np.asarray(sizes, dtype=np.int32).reshape(-1, 2))
    if sizes.shape[0] < 1:
        raise ValueError(f"{what}: an empty batch")
    return sizes


def _totals6(totals):
    return (C.c_size_t * 6)(*[int(v) for v in totals])


def _decode_jpeg_mixed_packed(batch, scan, chunk_bytes):
    """The packed pixel buffer (uint8 [batch.totals[2]]) and the statuses (int32 [N]) of a MixedJpegBatch on the
    device: one decoder call for the device-decoded images, one copy per host-decoded image into its slot."""
    from . import jpeg as _jpeg
    if not isinstance(batch, _jpeg.MixedJpegBatch):
        raise ValueError(f"decode_jpeg_mixed expects a MixedJpegBatch (openibl_amd.jpeg.collate_mixed), got "
                         f"{type(batch).__name__}")
    route, cb = _jpeg_route("decode_jpeg_mixed", batch, scan, chunk_bytes)
    dev = _need_cuda(batch.scan, batch.records, batch.segments, batch.host_pixels, batch.dev_index,
                     batch.host_index, batch.geom, batch.dev_geom)
    N = batch.n
    nd, nh = int(batch.records.shape[0]), int(batch.host_index.shape[0])
    if nd + nh != N or batch.records.shape[1:] != (_jpeg.REC_BYTES,) or tuple(batch.sizes.shape) != (N, 2) or \
            tuple(batch.geom.shape) != (N, _jpeg.GEOM_INTS) or tuple(batch.dev_geom.shape) != (nd, _jpeg.GEOM_INTS) or \
            len(batch.host_offsets) != nh + 1 or batch.host_offsets[-1] != batch.host_pixels.numel():
        raise ValueError(f"decode_jpeg_mixed: inconsistent batch: {nd} records + {nh} host images for N = {N}")
    packed = torch.empty(batch.totals[2], dtype=torch.uint8, device=dev)
    status = torch.zeros(N, dtype=torch.int32, device=dev)
    if nd:
        lib = _lib.load()
        S = int(batch.segments.shape[0])
        totals = _totals6(batch.dev_totals)
        need = lib.oibl_jpeg_decode_mixed_workspace_bytes(totals, nd, S)
        if need == 0:
            raise ValueError(f"decode_jpeg_mixed: {nd} images, {S} segments, totals {batch.dev_totals}: outside the "
                             f"decoder's limits (at most 65535 images of at least {_jpeg.MIN_WIDTH} and at most "
                             f"{_jpeg.MAX_DIM} pixels per side)")
        _jpeg_launch(batch, packed, status, route, batch.dev_totals[0], need, lib.oibl_jpeg_decode_mixed,
                     "jpeg_decode_mixed", (_ptr(batch.dev_geom), totals, cb))
    if nh:
        offs = _jpeg.geom_pixel_offsets(batch.geom_host)
        sizes = batch.sizes.tolist()
        for j, i in enumerate(_mixed_host_index(batch)):
            n = 3 * sizes[i][0] * sizes[i][1]
            packed[int(offs[i]):int(offs[i]) + n] = batch.host_pixels[batch.host_offsets[j]:batch.host_offsets[j] + n]
    return packed, status


def _mixed_host_index(batch):
    """The batch positions of the host-decoded images, from `reasons` (host data: no read-back)."""
    return [i for i, r in enumerate(batch.reasons) if r]


def _mixed_views(packed, batch):
    from . import jpeg as _jpeg
    offs = _jpeg.geom_pixel_offsets(batch.geom_host)
    return [packed[int(o):int(o) + 3 * h * w].view(h, w, 3) for o, (h, w) in zip(offs, batch.sizes.tolist())]


def _raise_damaged(what, status):
    from . import jpeg as _jpeg
    bad = status.cpu().numpy()
    if bad.any():
        raise ValueError(f"{what}: damaged JPEG streams: " + ", ".join(
            f"image {i} ({_jpeg.STATUS_TEXT[min(int(s), len(_jpeg.STATUS_TEXT) - 1)]})"
            for i, s in enumerate(bad) if s))


def decode_jpeg_mixed(batch, check: bool = True, scan: str = "auto", chunk_bytes=None):
    """Decode a `openibl_amd.jpeg.MixedJpegBatch` — N files of any stored sizes — on the device
    (oibl_jpeg_decode_mixed): a list of N uint8 views [H_i][W_i][3] into ONE packed buffer, each the bytes of
    `np.asarray(Image.open(f).convert('RGB'))`.  All images' segments decode in one launch; the files the device does
    not decode were decoded on the host when the batch was built and are copied into their slots.  scan, chunk_bytes
    and check as for `decode_jpeg` ("auto" looks at the batch's longest segment); check=False returns
    (views, status): status int32 [N] on the device, 0 ok, 5 for an image whose row of the geometry table is
    inconsistent (`jpeg.STATUS_TEXT`)."""
    packed, status = _decode_jpeg_mixed_packed(batch, scan, chunk_bytes)
    views = _mixed_views(packed, batch)
    if not check:
        return views, status
    _raise_damaged("decode_jpeg_mixed", status)
    return views


def resize_u8_mixed(packed: torch.Tensor, sizes, size, out: str = "uint8", mean=REF_MEAN, std=REF_STD) -> torch.Tensor:
    """Bilinear resize of a PACKED batch of mixed source sizes on the device (oibl_resize_u8_mixed), PIL's bits:
    packed is a 1-D uint8 tensor that holds image i as [H_i][W_i][3] at the offset `jpeg.mixed_layout(sizes)` gives it
    (what `decode_jpeg_mixed` writes), sizes int [N][2] = {H_i, W_i} on the host, size = (height, width) of the
    result.  out='uint8': [N][height][width][3]; out='float': [N][3][height][width] float32, ToTensor + Normalize of
    those bytes.  Every image equals `resize_u8` of that image alone; the per-axis shrink limit RESIZE_MAX_SCALE holds
    per image."""
    from . import jpeg as _jpeg
    if out not in JITTER_OUT:
        raise ValueError(f"resize_u8_mixed: out must be 'float' or 'uint8', not {out!r}")
    if packed.dtype != torch.uint8 or packed.dim() != 1:
        raise ValueError(f"resize_u8_mixed expects a 1-D uint8 packed buffer, got {packed.dtype} {tuple(packed.shape)}")
    if not isinstance(size, (tuple, list)) or len(size) != 2:
        raise ValueError(f"resize_u8_mixed: size must be (height, width), got {size!r}")
    H2, W2 = int(size[0]), int(size[1])
    sizes = _mixed_sizes(sizes, "resize_u8_mixed")
    N = sizes.shape[0]
    if H2 < 1 or W2 < 1:
        raise ValueError(f"resize_u8_mixed: the target size must be positive, got {H2} x {W2}")
    if max(H2, W2) > RESIZE_MAX_DIM or N > 65535:
        raise ValueError(f"resize_u8_mixed: N <= 65535 and every size <= {RESIZE_MAX_DIM}, got {N} images -> "
                         f"{H2} x {W2}")
    geom, totals = _jpeg.mixed_layout(sizes)
    _jpeg.check_shrink(sizes, (H2, W2), "resize_u8_mixed")
    if packed.numel() < totals[2]:
        raise ValueError(f"resize_u8_mixed: the packed buffer has {packed.numel()} bytes, the images need {totals[2]}")
    if not packed.is_contiguous():
        raise ValueError("openibl_amd: tensors must be contiguous")
    dev = _need_cuda(packed)
    return _resize_u8_mixed(packed, torch.from_numpy(geom).to(dev, non_blocking=True), sizes, H2, W2, out, mean, std,
                            dev)


def _resize_u8_mixed(packed, geom_dev, sizes, H2, W2, out, mean, std, dev):
    lib = _lib.load()
    N = sizes.shape[0]
    res, m3, s3 = _resize_result(N, H2, W2, out, mean, std, dev)
    sp = sizes.ctypes.data_as(C.c_void_p)
    ws = workspace(lib.oibl_resize_u8_mixed_workspace_bytes(sp, N, H2, W2), dev, slot="resize_u8")
    _lib.check(lib.oibl_resize_u8_mixed(_ptr(packed), packed.numel(), _ptr(geom_dev), sp, N, H2, W2, JITTER_OUT[out],
                                        m3, s3, _ptr(res), _ptr(ws), ws.numel(), _stream(dev)), "resize_u8_mixed")
    return res


def decode_resize_jpeg(batch, size, out: str = "uint8", check: bool = True, scan: str = "auto", chunk_bytes=None,
                       mean=REF_MEAN, std=REF_STD):
    """From files to the dense batch the model reads, in two device calls: decode a `jpeg.MixedJpegBatch` (any mix of
    stored sizes) into the packed buffer and resize every image to size = (height, width) — [N][height][width][3]
    uint8, or with out='float' [N][3][height][width] float32 normalised.  Every image has the bytes of
    `Image.open(f).convert('RGB').resize((width, height), Image.BILINEAR)`.  A plain `jpeg.JpegBatch` takes the
    uniform calls, `resize_u8(decode_jpeg(batch))`.  check=False returns (batch, status) without a sync."""
    from . import jpeg as _jpeg
    if not isinstance(size, (tuple, list)) or len(size) != 2:
        raise ValueError(f"decode_resize_jpeg: size must be (height, width), got {size!r}")
    if out not in JITTER_OUT:
        raise ValueError(f"decode_resize_jpeg: out must be 'float' or 'uint8', not {out!r}")
    if isinstance(batch, _jpeg.JpegBatch):
        pixels, status = decode_jpeg(batch, check=False, scan=scan, chunk_bytes=chunk_bytes)
        res = resize_u8(pixels, size, out=out, mean=mean, std=std)
    else:
        if not isinstance(batch, _jpeg.MixedJpegBatch):
            raise ValueError(f"decode_resize_jpeg expects a MixedJpegBatch or a JpegBatch (openibl_amd.jpeg."
                             f"collate_mixed / collate), got {type(batch).__name__}")
        H2, W2 = int(size[0]), int(size[1])
        sizes = _mixed_sizes(batch.sizes, "decode_resize_jpeg")
        if H2 > RESIZE_MAX_DIM or W2 > RESIZE_MAX_DIM:
            raise ValueError(f"decode_resize_jpeg: every size <= {RESIZE_MAX_DIM}, got -> {H2} x {W2}")
        _jpeg.check_shrink(sizes, (H2, W2), "decode_resize_jpeg")
        packed, status = _decode_jpeg_mixed_packed(batch, scan, chunk_bytes)
        res = _resize_u8_mixed(packed, batch.geom, sizes, H2, W2, out, mean, std, packed.device)
    if not check:
        return res, status
    _raise_damaged("decode_resize_jpeg", status)
    return res


# ---------------------------------------------------------------------------------------------
def _jitter_params(what, params, N):
    if params is None:
        return
    if not torch.is_tensor(params) or params.dtype != torch.int32:
        raise ValueError(f"{what}: params must be int32 records, got {getattr(params, 'dtype', type(params).__name__)}")
    if tuple(params.shape) != (N, JITTER_RECORD_WORDS):
        raise ValueError(f"{what}: params must be [{N}][{JITTER_RECORD_WORDS}], got {tuple(params.shape)}")
    if not params.is_contiguous():
        raise ValueError("openibl_amd: tensors must be contiguous")


def _jitter_sizes(what, sizes):
    """The limits of oibl_color_jitter_u8_mixed on the host's sizes (the layout's own come from `jpeg.mixed_layout`)."""
    if sizes.shape[0] > 65535:
        raise ValueError(f"{what}: N <= 65535, got {sizes.shape[0]} images")
    for i, (h, w) in enumerate(sizes.tolist()):
        if h >= 1 and w >= 1 and h * w > JITTER_MAX_PIXELS:
            raise ValueError(f"{what}: image {i} is {h} x {w}: more than 2^28 pixels")


def color_jitter_mixed(packed: torch.Tensor, sizes, params: Optional[torch.Tensor], out=None) -> torch.Tensor:
    """Training colour jitter of a PACKED batch of mixed sizes on the device (oibl_color_jitter_u8_mixed), PIL's bits:
    packed is the 1-D uint8 tensor that holds image i as [H_i][W_i][3] at the offset `jpeg.mixed_layout(sizes)` gives
    it (what `decode_jpeg_mixed` writes and `resize_u8_mixed` reads), sizes int [N][2] = {H_i, W_i} on the host,
    `params` int32 [N][8] on the device as for `color_jitter`, or None for no jitter.  out=None allocates a new packed
    buffer, out=packed works in place; the jittered packed buffer is returned.  Every image equals
    `color_jitter(image[None], params[i:i + 1], out='uint8')` of that image alone; the padding between the images is
    never written."""
    from . import jpeg as _jpeg
    what = "color_jitter_mixed"
    if not torch.is_tensor(packed) or packed.dtype != torch.uint8 or packed.dim() != 1:
        raise ValueError(f"{what} expects a 1-D uint8 packed buffer, got "
                         f"{getattr(packed, 'dtype', type(packed).__name__)} {tuple(getattr(packed, 'shape', ()))}")
    sizes = _mixed_sizes(sizes, what)
    N = sizes.shape[0]
    _jitter_sizes(what, sizes)
    geom, totals = _jpeg.mixed_layout(sizes)
    if packed.numel() < totals[2]:
        raise ValueError(f"{what}: the packed buffer has {packed.numel()} bytes, the images need {totals[2]}")
    _jitter_params(what, params, N)
    if out is not None:
        if not torch.is_tensor(out) or out.dtype != torch.uint8 or out.dim() != 1 or out.numel() != packed.numel():
            raise ValueError(f"{what}: out must be a 1-D uint8 buffer of the packed buffer's {packed.numel()} bytes "
                             f"(or the packed buffer itself)")
        if out.device != packed.device:
            raise ValueError(f"{what}: out must be on the packed buffer's device")
    if not packed.is_contiguous() or (out is not None and not out.is_contiguous()):
        raise ValueError("openibl_amd: tensors must be contiguous")
    dev = _need_cuda(packed, params)
    if out is None:
        out = torch.empty_like(packed)
    return _color_jitter_mixed(packed, torch.from_numpy(geom).to(dev, non_blocking=True), sizes, params, out, dev)


def _color_jitter_mixed(packed, geom_dev, sizes, params, out, dev):
    lib = _lib.load()
    N = sizes.shape[0]
    sp = sizes.ctypes.data_as(C.c_void_p)
    ws = None
    if params is not None:
        ws = workspace(lib.oibl_color_jitter_u8_mixed_workspace_bytes(sp, N), dev, slot="color_jitter")
    _lib.check(lib.oibl_color_jitter_u8_mixed(_ptr(packed), packed.numel(), _ptr(geom_dev), sp, N, _ptr(params),
                                              _ptr(out), _ptr(ws), 0 if ws is None else ws.numel(), _stream(dev)),
               "color_jitter_u8_mixed")
    return out


class PackedImages:
    """A MixedJpegBatch decoded on the device: `packed`, the 1-D uint8 buffer that holds image i as [H_i][W_i][3] at
    its offset of `geom` (int32 [N][8] on the device, the batch's geometry table), `sizes` (int32 numpy [N][2] on the
    host) and `status` (int32 [N] on the device, the decoder's per-image status: `jpeg.STATUS_TEXT`).  What
    `color_jitter_mixed` works on in place and `resize_u8_mixed` turns into the dense batch."""

    def __init__(self, packed, sizes, geom, status):
        self.packed, self.sizes, self.geom, self.status = packed, sizes, geom, status

    def __len__(self):
        return int(self.sizes.shape[0])

    @property
    def device(self):
        return self.packed.device


def decode_jpeg_packed(batch, scan: str = "auto", chunk_bytes=None) -> PackedImages:
    """Decode a `jpeg.MixedJpegBatch` on the device into its packed buffer (`PackedImages`), without reading the
    statuses back; the files of the host route are copied into their slots."""
    packed, status = _decode_jpeg_mixed_packed(batch, scan, chunk_bytes)
    return PackedImages(packed, _mixed_sizes(batch.sizes, "decode_jpeg_mixed"), batch.geom, status)


def jitter_packed(images: PackedImages, params: Optional[torch.Tensor]) -> PackedImages:
    """`color_jitter_mixed` in place on a `PackedImages`; params int32 [N][8] on the device, or None."""
    what = "color_jitter_mixed"
    _jitter_sizes(what, images.sizes)
    _jitter_params(what, params, len(images))
    dev = _need_cuda(images.packed, images.geom, params)
    if params is not None:
        _color_jitter_mixed(images.packed, images.geom, images.sizes, params, images.packed, dev)
    return images


def resize_packed(images: PackedImages, size, out: str = "uint8", mean=REF_MEAN, std=REF_STD) -> torch.Tensor:
    """`resize_u8_mixed` of a `PackedImages`: the dense batch [N][height][width][3] uint8 or, out='float',
    [N][3][height][width] float32 normalised."""
    from . import jpeg as _jpeg
    what = "resize_u8_mixed"
    if out not in JITTER_OUT:
        raise ValueError(f"{what}: out must be 'float' or 'uint8', not {out!r}")
    if not isinstance(size, (tuple, list)) or len(size) != 2:
        raise ValueError(f"{what}: size must be (height, width), got {size!r}")
    H2, W2 = int(size[0]), int(size[1])
    if H2 > RESIZE_MAX_DIM or W2 > RESIZE_MAX_DIM:
        raise ValueError(f"{what}: every size <= {RESIZE_MAX_DIM}, got -> {H2} x {W2}")
    _jpeg.check_shrink(images.sizes, (H2, W2), what)
    dev = _need_cuda(images.packed, images.geom)
    return _resize_u8_mixed(images.packed, images.geom, images.sizes, H2, W2, out, mean, std, dev)


def decode_jitter_resize_jpeg(batch, params: Optional[torch.Tensor], size, out: str = "float", check: bool = True,
                              scan: str = "auto", chunk_bytes=None, mean=REF_MEAN, std=REF_STD):
    """From files to the jittered training batch on the device, in the reference's order ColorJitter -> Resize ->
    ToTensor -> Normalize: decode a `jpeg.MixedJpegBatch` (any mix of stored sizes) into the packed buffer, jitter
    every image in place at its stored size (`params` int32 [N][8] on the device as for `color_jitter`, or None) and
    resize it to size = (height, width) — [N][3][height][width] float32 normalised, or with out='uint8'
    [N][height][width][3].  Every image has the bytes of PIL's decode, torchvision's ColorJitter with the record's
    order and factors, and `resize((width, height), Image.BILINEAR)`; the files of the host route (progressive, PNG,
    CMYK, narrower than 8 pixels) are jittered with the rest.  A plain `jpeg.JpegBatch` takes the uniform calls,
    `resize_u8(color_jitter(decode_jpeg(batch), params, out='uint8'), size, out=out)`.  check=False returns
    (batch, status) without a sync."""
    from . import jpeg as _jpeg
    what = "decode_jitter_resize_jpeg"
    if not isinstance(size, (tuple, list)) or len(size) != 2:
        raise ValueError(f"{what}: size must be (height, width), got {size!r}")
    if out not in JITTER_OUT:
        raise ValueError(f"{what}: out must be 'float' or 'uint8', not {out!r}")
    if isinstance(batch, _jpeg.JpegBatch):
        _jitter_params(what, params, batch.n)
        pixels, status = decode_jpeg(batch, check=False, scan=scan, chunk_bytes=chunk_bytes)
        res = resize_u8(color_jitter(pixels, params, out="uint8"), size, out=out, mean=mean, std=std)
    else:
        if not isinstance(batch, _jpeg.MixedJpegBatch):
            raise ValueError(f"{what} expects a MixedJpegBatch or a JpegBatch (openibl_amd.jpeg.collate_tuples / "
                             f"collate_mixed / collate), got {type(batch).__name__}")
        H2, W2 = int(size[0]), int(size[1])
        sizes = _mixed_sizes(batch.sizes, what)
        if H2 > RESIZE_MAX_DIM or W2 > RESIZE_MAX_DIM:
            raise ValueError(f"{what}: every size <= {RESIZE_MAX_DIM}, got -> {H2} x {W2}")
        _jpeg.check_shrink(sizes, (H2, W2), what)
        _jitter_sizes(what, sizes)
        _jitter_params(what, params, batch.n)
        images = jitter_packed(decode_jpeg_packed(batch, scan, chunk_bytes), params)
        res = _resize_u8_mixed(images.packed, images.geom, sizes, H2, W2, out, mean, std, images.device)
        status = images.status
    if not check:
        return res, status
    _raise_damaged(what, status)
    return res
