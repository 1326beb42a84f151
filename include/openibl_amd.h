/*
 * openibl_amd.h — C ABI of the MI355X (gfx950) descriptor + matching hot path.
 *
 * This is the drop-in boundary.  The reference (yxgeee/OpenIBL) has no
 * FFI of its own: its hot path is the Python call surface ibl.models / ibl.pca /
 * ibl.evaluators.  Every entry point below replaces the device work of one reference
 * function (cited per function as path:line under the reference tree) and is what a
 * ctypes binding added to the reference would bind.
 *
 * Conventions
 *   - plain C: pointers and sizes only, no torch / C++ types.
 *   - every pointer argument is a DEVICE pointer valid on the current HIP device unless
 *     the name ends in _host.
 *   - `stream` is a hipStream_t passed as void*; every call is asynchronous and
 *     stream-ordered; re-entrant across streams (no hidden global state besides the
 *     thread-local error string: the shipping library has no mutable statics on any launch path — the
 *     test hooks exist only in libopenibl_amd_dbg.so, built from the same sources with
 *     -DOIBL_DEBUG_HOOKS).
 *   - no hidden allocation: outputs and scratch are caller-provided; scratch size comes
 *     from the matching *_workspace_bytes() query.  Workspace pointers must be 256-byte
 *     aligned.
 *   - return value: 0 = OK, negative = error (OIBL_E_*); message via oibl_last_error().
 *   - `precision` selects the arithmetic of the contraction:
 *       OIBL_BF16 : bf16 operands, fp32 accumulate on v_mfma_f32_32x32x16_bf16
 *       OIBL_F32  : exact fp32 on v_mfma_f32_32x32x2_f32 (parity mode)
 *       OIBL_BF16X3 : "split bf16" — every operand travels as hi = bf16(v), lo = bf16(v - hi) and a
 *                   product is hi.hi + hi.lo + lo.hi on the bf16 matrix cores, fp32 accumulate
 *                   (~2^-17 relative per product: fp32-class descriptors at 3x the bf16 MFMA work
 *                   instead of 16x).  Element = 4 bytes; a row of C elements (C % 32 == 0) is stored
 *                   as C/32 groups of [32 x hi | 32 x lo] (128 bytes), see oibl_x3_split_rows.
 *       OIBL_F16MX : fp16 main term + MX-fp6 cross terms — every operand travels as hi = fp16(v)
 *                   plus block-scaled e2m3 images of hi and of lo = v - hi (one e8m0 scale per 32
 *                   elements); a product is hi.hi on v_mfma_f32_32x32x16_f16 plus
 *                   q6(hi).q6(lo) + q6(lo).q6(hi) on ONE v_mfma_scale_f32_32x32x64_f8f6f4 (the two
 *                   cross terms concatenated along K), fp32 accumulate: ~2^-15 relative per product —
 *                   inside north_star's 1e-4 on the descriptor — at HALF the matrix-pipe time of
 *                   OIBL_BF16X3.  Element = 4 bytes; a row of C elements (C % 32 == 0) is C/32 lines
 *                   of 128 bytes: [32 x fp16 | q6(hi) 16 B | q6(lo) 16 B | q6(hi) 8 B, scale, pad |
 *                   q6(lo) 8 B, scale, pad], see oibl_mx_split_rows.
 *                   RANGE: hi = fp16(v) exists only for |v| <= 65504.  A producer of f16mx lines that meets
 *                   a larger value saturates it (the line is then NOT a 1e-4 image of the value) and raises
 *                   the caller's RANGE FLAG — a uint32 in device memory that the caller zeroes before the
 *                   pass and reads after it: non-zero = the pass must be repeated in OIBL_BF16X3 (same
 *                   tolerance class, no range limit).  oibl_vgg16_conv5_forward* keep the flag in the first
 *                   word of their workspace; oibl_conv3x3_nhwc_flagged / oibl_mx_split_rows_flagged take it
 *                   as an argument; the matching entry points mark an out-of-range descriptor row with a
 *                   +inf norm (all its distances are +inf).  The host mirror (openibl_amd/models.py) reads
 *                   the flag once per batch and re-runs flagged batches in OIBL_BF16X3.
 *     and with it the element type of activation / packed-weight buffers ("T" below:
 *     uint16 bf16 bits, float, or the 4-byte split element).
 */
#ifndef OPENIBL_AMD_H
#define OPENIBL_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define OIBL_OK 0
#define OIBL_E_INVALID (-1)   /* bad argument (shape, alignment, null pointer)      */
#define OIBL_E_WORKSPACE (-2) /* workspace too small                                */
#define OIBL_E_HIP (-3)       /* a HIP runtime call / kernel launch failed           */
#define OIBL_E_UNSUPPORTED (-4)

#define OIBL_BF16 0
#define OIBL_F32 1
#define OIBL_BF16X3 2
#define OIBL_F16MX 3

/* Storage type of a descriptor matrix handed to the *_st matching entry points. */
#define OIBL_ST_F32 0
#define OIBL_ST_F16 1  /* IEEE binary16 */
#define OIBL_ST_BF16 2

#define OIBL_VGG16_NUM_CONV 13

/* ---- library ---------------------------------------------------------------------- */

/* ABI version of this header (bumped on any signature change). */
int oibl_abi_version(void);
/* Last error message of the calling thread (never NULL). */
const char* oibl_last_error(void);
/* Name of the gfx target the kernels were compiled for ("gfx950"). */
const char* oibl_target_arch(void);
/* sizeof(T) for a precision code, 0 if unknown. */
size_t oibl_elem_size(int precision);

/* ---- element conversion helpers --------------------------------------------------- */

/* fp32 -> bf16 (round-to-nearest-even), n elements. */
int oibl_cast_f32_to_bf16(const float* src, uint16_t* dst, size_t n, void* stream);
/* bf16 -> fp32, n elements. */
int oibl_cast_bf16_to_f32(const uint16_t* src, float* dst, size_t n, void* stream);
/* fp32 <-> IEEE binary16 (round-to-nearest-even), n elements: 16-bit descriptor storage
 * (BASELINE.json configs[4], "fp16 descriptors"; no counterpart in the reference). */
int oibl_cast_f32_to_f16(const float* src, uint16_t* dst, size_t n, void* stream);
int oibl_cast_f16_to_f32(const uint16_t* src, float* dst, size_t n, void* stream);

/* fp32 rows [rows][C] <-> OIBL_BF16X3 rows (C/32 groups of [32 hi | 32 lo] per row; C % 32 == 0):
 * the activation / operand layout of the OIBL_BF16X3 kernels.  join returns hi + lo (exact). */
int oibl_x3_split_rows(const float* src, void* dst, size_t rows, int C, void* stream);
int oibl_x3_join_rows(const void* src, float* dst, size_t rows, int C, void* stream);
/* fp32 rows [rows][C] <-> OIBL_F16MX rows (C/32 lines of 128 bytes per row; C % 32 == 0).  join
 * returns what the kernels see of every element: which = 0: hi + q6(lo) (the stored value to ~2^-15
 * of the line's largest element), 1: hi (fp16, exact), 2: q6(hi), 3: q6(lo). */
int oibl_mx_split_rows(const float* src, void* dst, size_t rows, int C, void* stream);
/* The same with a range flag (may be NULL): *range_flag is set to 1 when a group holds a value beyond
 * +-65504 (see OIBL_F16MX above); never cleared by the call. */
int oibl_mx_split_rows_flagged(const float* src, void* dst, size_t rows, int C, uint32_t* range_flag,
                               void* stream);
int oibl_mx_join_rows(const void* src, float* dst, size_t rows, int C, int which, void* stream);

/* ---- bilinear resize --------------------------------------------------------------- *
 * x [N][C][H][W] fp32 -> out [N][C][H2][W2] fp32 with the arithmetic of
 * torch.nn.functional.interpolate(x, size=(H2, W2), mode="bilinear", align_corners=False)
 * (source index (dst + 0.5) * in/out - 0.5 clamped at 0, no antialiasing).  Used by the
 * multi-scale extraction of BASELINE.json configs[4]; the reference itself resizes PIL images in
 * its loader (ibl/utils/data/__init__.py:37-42) and has no multi-scale path. */
int oibl_resize_bilinear_nchw(const float* x, int N, int C, int H, int W, float* out, int H2, int W2,
                              void* stream);

/* ---- VGG16 conv1_1 .. conv5_3 backbone -------------------------------------------- *
 * Replaces VGG.forward's `self.base(x)`  (ibl/models/vgg.py:61-62; layer list built at
 * vgg.py:40-42 = torchvision vgg16.features[:-2]: 13 conv3x3(pad 1)+bias, ReLU after all
 * but the last, 2x2/2 max-pool after conv1_2, conv2_2, conv3_3, conv4_3).                */

/* Re-pack one conv weight from the state-dict layout [Cout][Cin][3][3] fp32 into the
 * kernel layout [tap=ky*3+kx][Cout][Cin_pad] of T (Cin_pad = Cin rounded up to the K-step:
 * 64 elements bf16 / 32 fp32; pad is zero).  packed must hold
 * oibl_conv3x3_packed_bytes(cout, cin, precision) bytes. */
size_t oibl_conv3x3_packed_bytes(int cout, int cin, int precision);
int oibl_pack_conv3x3_weights(const float* w_oihw, int cout, int cin, int precision,
                              void* packed, void* stream);

/* One 3x3 / pad 1 / stride 1 convolution + bias (+ReLU) (+2x2/2 max-pool, floor) on NHWC
 * activations: in [N][H][W][Cin] T -> out [N][Ho][Wo][Cout] T, (Ho,Wo) = (H,W) or
 * (H/2,W/2) when pool != 0.  Cin % 64 == 0 (bf16) / % 32 (fp32); Cout % 64 == 0.
 * (nn.Conv2d + nn.ReLU + nn.MaxPool2d modules of vgg.py:41-42.) */
int oibl_conv3x3_nhwc(const void* in, int N, int H, int W, int cin, const void* packed_w,
                      const float* bias, int cout, int relu, int pool, int precision,
                      void* out, void* stream);
/* The same with a range flag for OIBL_F16MX outputs (may be NULL; ignored by the other precisions):
 * *range_flag is set to 1 when an output of the layer is beyond +-65504 and was saturated (see OIBL_F16MX
 * above); never cleared by the call. */
int oibl_conv3x3_nhwc_flagged(const void* in, int N, int H, int W, int cin, const void* packed_w,
                              const float* bias, int cout, int relu, int pool, int precision,
                              void* out, uint32_t* range_flag, void* stream);
/* The same with scratch: a layer whose tiling would leave most of the chip idle — conv4 / conv5 of a few
 * images — is then contracted split-K (several workgroups per output tile, fp32 partial tiles in `ws`, a
 * fixed-order reduction that also applies bias / ReLU / pool: deterministic, equal to the one-pass result up
 * to fp32 association), in every precision.  oibl_conv3x3_workspace_bytes may return 0; ws == NULL runs the
 * layer in one pass whatever its size.  This is what oibl_vgg16_conv5_forward runs per layer. */
size_t oibl_conv3x3_workspace_bytes(int N, int H, int W, int cin, int cout, int pool, int precision);
int oibl_conv3x3_nhwc_ws(const void* in, int N, int H, int W, int cin, const void* packed_w,
                         const float* bias, int cout, int relu, int pool, int precision, void* out,
                         void* ws, size_t ws_bytes, uint32_t* range_flag, void* stream);

/* First layer: reads the reference's input tensor directly — x [N][3][H][W] fp32 NCHW
 * (already mean/std normalised, ibl/utils/data/__init__.py:40-41) — conv1_1 + bias + ReLU,
 * writes NHWC T [N][H][W][64].  w is the plain state-dict tensor [64][3][3][3] fp32. */
int oibl_conv1_1_nchw(const float* x_nchw, int N, int H, int W, const float* w_oihw,
                      const float* bias, int precision, void* out, void* stream);

/* Global max-pool over positions of an NHWC feature map -> pool_x [N][C] fp32
 * (nn.AdaptiveMaxPool2d(1), vgg.py:43,67-68). */
int oibl_global_maxpool_nhwc(const void* feat, int N, int P, int C, int precision,
                             float* out, void* stream);

/* NHWC T -> NCHW fp32 (the layout VGG.forward returns `x` in, vgg.py:70). */
int oibl_nhwc_to_nchw_f32(const void* feat, int N, int P, int C, int precision, float* out,
                          void* stream);
/* NCHW fp32 -> NHWC T (to feed NetVLAD.forward from a reference-layout tensor). */
int oibl_nchw_f32_to_nhwc(const float* x, int N, int C, int P, int precision, void* out,
                          void* stream);

/* The same backbone fed with the loader's RAW image: x_nhwc [N][H][W][3] uint8 (what
 * PIL / cv2 decode to), ToTensor + Normalize (ibl/utils/data/__init__.py:37-42:
 * (u / 255 - mean) / std, fp32) folded into the first kernel.  mean3_host / std3_host: 3 floats
 * each, HOST pointers.  The host -> device copy shrinks 4x (0.9 MB instead of 3.7 MB per 480x640 image).
 * OIBL_BF16: the fused stem looks the normalised bf16 operand up in a 3 x 257 table built with
 * exactly that arithmetic — bit-identical to oibl_vgg16_conv5_forward on the normalised fp32 tensor.
 * OIBL_BF16X3 / OIBL_F16MX: the fused stems gather the bytes themselves (three 12-byte loads per window)
 * and evaluate Normalize as ONE fma per value, u * 1/(255 std) - mean/std: within 2^-16 of the loader's
 * three rounded operations on values up to 151 (identical bf16 hi parts of conv1_1's operand for all 768
 * (channel, byte) pairs, 42 lo parts one unit apart) — the conv5_3 map is within ~1e-6 (bf16x3) / ~1e-5
 * (f16mx: the size of its own rounding) of the fp32-input result, not bit-identical.  These stems read the image
 * through dword-aligned loads over a descriptor rounded up to whole dwords (a partly covered last dword reads as
 * zero, nothing beyond the rounded size is touched): x_nhwc that is NOT 4-byte aligned takes the normalising
 * pass of OIBL_F32 below instead (same results as the fp32-input route), it is never read misaligned.
 * OIBL_F32 (and shapes the stems do not take): a normalising uint8 -> fp32 NCHW pass into the workspace,
 * then the regular path (bit-identical).  ev_*: optional hipEvent_t recorded around the matrix-core
 * launches (as oibl_vgg16_conv5_forward_ev), may be NULL.      */
size_t oibl_vgg16_u8_workspace_bytes(int N, int H, int W, int precision);
int oibl_vgg16_conv5_forward_u8(const uint8_t* x_nhwc, int N, int H, int W, const float* mean3_host,
                                const float* std3_host, const void* const* packed_w_host,
                                const float* const* bias_host, int precision, void* feat, void* ws,
                                size_t ws_bytes, void* stream, void* ev_igemm_begin,
                                void* ev_igemm_end);

/* Fused VGG stem, bf16: conv1_1 + ReLU + conv1_2 + ReLU + 2x2/2 max-pool in one launch —
 * replaces modules 0-4 of VGG.base (ibl/models/vgg.py:40-42; forward :61-62):
 *   x_nchw [N][3][H][W] fp32 -> out [N][H/2][W/2][64] bf16 (NHWC).
 * w1_oihw / b1: conv1_1 in the state-dict layout (fp32); packed_w2: conv1_2 packed by
 * oibl_pack_conv3x3_weights(..., OIBL_BF16).  Bit-identical to oibl_conv1_1_nchw followed by
 * oibl_conv3x3_nhwc(relu=1, pool=1) in OIBL_BF16; the conv1_1 activations never reach HBM.
 * oibl_vgg16_conv5_forward uses it automatically in OIBL_BF16. */
int oibl_vgg16_stem_bf16(const float* x_nchw, int N, int H, int W, const float* w1_oihw,
                         const float* b1, const void* packed_w2, const float* b2, void* out,
                         void* stream);

/* The same fusion in OIBL_BF16X3: out [N][H/2][W/2][64] as (hi, lo) split elements; packed_w2 from
 * oibl_pack_conv3x3_weights(..., OIBL_BF16X3).  A workgroup serves half of conv1_2's output channels
 * and consumes a tile in two passes over halves of its input channels, so that the split weights
 * (72 KiB) and two 42.5 KiB halo buffers fit LDS.  Bit-identical to oibl_conv1_1_nchw followed by
 * oibl_conv3x3_nhwc(relu=1, pool=1) in OIBL_BF16X3 up to the summation order of conv1_2
 * (channel chunk outer, tap inner); used automatically by oibl_vgg16_conv5_forward. */
int oibl_vgg16_stem_x3(const float* x_nchw, int N, int H, int W, const float* w1_oihw,
                       const float* b1, const void* packed_w2, const float* b2, void* out,
                       void* stream);

/* The same fusion in OIBL_F16MX: out [N][H/2][W/2][64] as f16mx lines; packed_w2 from
 * oibl_pack_conv3x3_weights(..., OIBL_F16MX).  conv1_1 (K = 27) is computed in split bf16, its output is
 * packed into f16mx lines inside LDS, conv1_2 runs in the f16mx arithmetic (2 fp16 + 1 scaled-fp6 MFMA per 32
 * channels) and the pooled map leaves as f16mx lines.  The e2m3 image of a lo part is rounded through fp16
 * here (the other f16mx producers convert it from fp32): its codes can differ by one step from
 * oibl_mx_split_rows of the same values.  H >= 2, W >= 3.  Used automatically by oibl_vgg16_conv5_forward
 * in OIBL_F16MX. */
int oibl_vgg16_stem_mx(const float* x_nchw, int N, int H, int W, const float* w1_oihw,
                       const float* b1, const void* packed_w2, const float* b2, void* out,
                       void* stream);

/* Whole backbone: x [N][3][H][W] fp32 -> feat [N][P][512] T, P = (H/16)*(W/16) (floor at
 * every pool).  packed_w_host / bias_host are HOST arrays of 13 DEVICE pointers: entry 0
 * is the plain [64][3][3][3] fp32 conv1_1 weight, entries 1..12 are packed by
 * oibl_pack_conv3x3_weights; bias entries are [Cout] fp32.
 * OIBL_BF16X3: activations between the layers are (hi, lo) split elements, but `feat` is written as
 * plain fp32 (the head consumes it with OIBL_F32).
 * OIBL_F16MX: every entry packed with OIBL_F16MX (conv1_1 + conv1_2 + pool = oibl_vgg16_stem_mx; the
 * mode has no unfused front and 32-bit-offset kernels only: a batch whose fp32 input or whose largest
 * activation — conv2_2's input, N (H/2) (W/2) 128 x 4 bytes: 95 images of 480x640 — reaches 3.5 GB is
 * refused with OIBL_E_INVALID); `feat` is plain fp32.  The FIRST
 * 32-BIT WORD OF THE WORKSPACE is the pass's range flag: zeroed (stream-ordered) when the call starts,
 * 1 afterwards if any activation between the layers was beyond the format's range — `feat` is then not a 1e-4
 * result and the batch has to be repeated in OIBL_BF16X3 (see OIBL_F16MX at the top).  The whole-backbone
 * entry points store their intermediate activations multiplied by 1/8 (exact: a power of two, undone in the
 * layer that writes `feat`), so that the bound is 8 x 65504 = 5.2e5 in activation units; the stand-alone
 * layer entries (oibl_conv3x3_nhwc*) store what they compute, bound 65504.  The other precisions leave the
 * word untouched.
 * The workspace holds the range flag, the two ping-pong activation buffers and the fp32 partial tiles of
 * the layers that run split-K: a layer whose tiling leaves most of the chip idle (small batches), and in
 * OIBL_F16MX also the tiles of a nearly empty LAST ROUND of a big layer (conv5_x at batch 32: 300 tiles on
 * 256 CUs), are contracted by several workgroups per tile and reduced in a fixed order — deterministic,
 * equal to the one-pass kernels up to fp32 association. */
size_t oibl_vgg16_workspace_bytes(int N, int H, int W, int precision);
int oibl_vgg16_conv5_forward(const float* x_nchw, int N, int H, int W,
                             const void* const* packed_w_host,
                             const float* const* bias_host, int precision, void* feat,
                             void* ws, size_t ws_bytes, void* stream);
/* Same, with two optional hipEvent_t handles (may be NULL) recorded on `stream` right before the
 * first and right after the last implicit-GEMM convolution (conv1_2 .. conv5_3, 12 launches of
 * the dominant kernel): bench.py brackets the kernel it reports a roofline for with these. */
int oibl_vgg16_conv5_forward_ev(const float* x_nchw, int N, int H, int W,
                                const void* const* packed_w_host,
                                const float* const* bias_host, int precision, void* feat,
                                void* ws, size_t ws_bytes, void* stream, void* ev_igemm_begin,
                                void* ev_igemm_end);
/* The frozen trunk of conv5 training: conv1_1 .. conv4_3 + pool exactly as oibl_vgg16_conv5_forward runs them (the
 * same stems, kernels and — OIBL_F16MX — range flag in the workspace's first word), stopped behind the fourth
 * max-pool.  Only entries 0..9 of the two pointer arrays are read.  pool4 [N][H/16][W/16][512] is plain fp32 in
 * activation units in every precision (the stored activation widened: bf16 exactly, bf16x3 hi + lo, f16mx the value
 * conv5_1 would read with the 1/8 storage scale undone).  Workspace from oibl_vgg16_workspace_bytes.             */
int oibl_vgg16_pool4_forward(const float* x_nchw, int N, int H, int W, const void* const* packed_w_host,
                             const float* const* bias_host, int precision, float* pool4,
                             void* ws, size_t ws_bytes, void* stream);
/* The frozen trunk for a cache of stored activations: the same pass, stopped at the same place, but conv4_3 + pool
 * writes the STORED activation — exactly what conv5_1 reads inside oibl_vgg16_conv5_forward — straight into the
 * caller's buffer lines [N][H/16][W/16][512] of the precision's element type (OIBL_BF16: 2-byte bf16; OIBL_BF16X3:
 * split elements; OIBL_F16MX: f16mx lines INCLUDING the 1/8 storage scale; OIBL_F32: plain fp32), and nothing is
 * launched behind it.  `lines` may be a 16-byte-aligned slice of a larger buffer.  Entries 0..9 of the pointer arrays
 * are read; range flag (OIBL_F16MX) in the first word of the workspace; workspace from oibl_vgg16_workspace_bytes,
 * or oibl_vgg16_u8_workspace_bytes for the _u8 variant (x_nhwc, mean3_host, std3_host as in
 * oibl_vgg16_conv5_forward_u8).                                                                                    */
int oibl_vgg16_pool4_lines_forward(const float* x_nchw, int N, int H, int W, const void* const* packed_w_host,
                                   const float* const* bias_host, int precision, void* lines,
                                   void* ws, size_t ws_bytes, void* stream);
int oibl_vgg16_pool4_lines_forward_u8(const uint8_t* x_nhwc, int N, int H, int W, const float* mean3_host,
                                      const float* std3_host, const void* const* packed_w_host,
                                      const float* const* bias_host, int precision, void* lines,
                                      void* ws, size_t ws_bytes, void* stream);
/* conv5_1 .. conv5_3 on such lines [N][h][w][512] (h = H/16, w = W/16 of the images): the three layers are launched
 * exactly as oibl_vgg16_conv5_forward launches them for a batch of the same N, H, W — the same kernels and the same
 * split-K plans, which depend on N, h, w and the precision alone — so `feat` [N][h][w][512] (bf16 in OIBL_BF16,
 * plain fp32 otherwise) is BIT-EQUAL to the whole forward's.  Only entries 10..12 of the two pointer arrays (13
 * entries, as above) are read.  OIBL_F16MX: the first word of the workspace is the range flag, zeroed when the call
 * starts and raised by these three layers; the 1/8 storage scale of the lines is undone in the layer that writes
 * `feat`.  `lines` is only read.  Arguments are validated before any HIP call: OIBL_E_INVALID for null pointers, N,
 * h or w < 1 and an unknown precision, OIBL_E_WORKSPACE for a short workspace.  The query returns 0 for an empty
 * problem or an unknown precision.                                                                                 */
size_t oibl_vgg16_conv5_from_pool4_workspace_bytes(int N, int h, int w, int precision);
int oibl_vgg16_conv5_from_pool4(const void* lines, int N, int h, int w, const void* const* packed_w_host,
                                const float* const* bias_host, int precision, void* feat,
                                void* ws, size_t ws_bytes, void* stream);

/* ---- NetVLAD + intra-norm + L2 ---------------------------------------------------- *
 * Replaces NetVLAD.forward (ibl/models/netvlad.py:44-61) and the normalisation that
 * every Embed* module applies to it (netvlad.py:78-80 / 100-102 / 202-204):
 *   xh = x / max(|x|_2, 1e-12)  per position; a = softmax_k(assign_w . xh);
 *   vlad[k][c] = sum_p a[p][k] * (xh[p][c] - centroids[k][c]).
 * feat [N][P][C] T (NHWC feature map), assign_w [K][C] fp32 (conv.weight[:, :, 0, 0]),
 * centroids [K][C] fp32.  K = 64, C = 512 are what the kernels are built for.
 *   vlad_raw  (optional, may be NULL): [N][K][C] fp32 un-normalised — NetVLAD.forward's
 *             return value.
 *   vlad_norm (optional, may be NULL): [N][K*C] fp32, intra-normalised per cluster then
 *             L2-normalised over K*C, k-major (index k*C + c).
 *   normalize_input: NetVLAD(normalize_input=...) (netvlad.py:46-47).                    */
size_t oibl_netvlad_workspace_bytes(int N, int P, int K, int C);
int oibl_netvlad_forward(const void* feat, int N, int P, int K, int C, int precision,
                         const float* assign_w, const float* centroids, int normalize_input,
                         float* vlad_raw, float* vlad_norm, void* ws, size_t ws_bytes,
                         void* stream);

/* ---- SFRS region similarities (forward only) ---------------------------------------- *
 * Replaces EmbedRegionNet._compute_region_sim (ibl/models/netvlad.py:123-186), which SFRSTrainer._forward
 * calls on the frozen previous-generation model under torch.no_grad() (ibl/trainers.py:243-244).
 * The conv5_3 map of an image is cut into four quarters of h/2 x w/2 pixels (q0 top-left, q1 top-right, q2
 * bottom-left, q3 bottom-right); NetVLAD (as above, same per-pixel normalisation and softmax) is aggregated over
 * each quarter's pixels; 9 regions are sums of quarters, in this order:
 *   [q0+q1+q2+q3, q0+q1, q2+q3, q0+q2, q1+q3, q0, q1, q2, q3]
 * each intra-normalised per cluster, flattened k-major and L2-normalised (eps 1e-12).
 * oibl_region_vlad_forward: feat [N][h][w][C] fp32 (precision must be OIBL_F32; h and w even, K = 64, C = 512)
 *   -> region_vlad [N][9][K*C] fp32.  The map is read once; an image's vectors do not depend on the batch it is
 *   computed in (bit for bit).  Workspace from oibl_region_workspace_bytes (0 for an invalid shape).
 * oibl_region_scores: region_vlad [T*per_tuple][9][L], tuple-major, the first image of each tuple is the anchor,
 *   per_tuple = 1 + n >= 2 -> score [T][n][9][9] fp32,
 *   score[t][j][a][b] = <region_vlad[t*per_tuple][a], region_vlad[t*per_tuple + 1 + j][b]>, summed in a fixed order.
 * Invalid arguments (odd h or w, per_tuple < 2, short workspace) return an error status and launch nothing.   */
size_t oibl_region_workspace_bytes(int N, int h, int w, int K, int C);
int oibl_region_vlad_forward(const void* feat, int N, int h, int w, int K, int C, int precision,
                             const float* assign_w, const float* centroids, int normalize_input,
                             float* region_vlad, void* ws, size_t ws_bytes, void* stream);
int oibl_region_scores(const float* region_vlad, int T, int per_tuple, int L, float* score, void* stream);

/* ---- NetVLAD + intra-norm + L2: gradients ------------------------------------------- *
 * The backward of oibl_netvlad_forward's vlad_norm, i.e. of NetVLAD.forward (ibl/models/netvlad.py:44-61) followed
 * by the two F.normalize calls of EmbedNet.forward (netvlad.py:78-80), as torch autograd differentiates them (a
 * norm clamped at eps = 1e-12 is a constant denominator).  Stateless: nothing is carried over from a forward call,
 * the per-pixel norms, the soft-assignment and the aggregated rows are recomputed from `feat`.
 * feat [N][P][C] fp32 (precision must be OIBL_F32), assign_w / centroids [K][C] fp32, K = 64 and C = 512 only;
 * grad_vlad_norm [N][K*C] fp32, k-major: dL/d vlad_norm.  Outputs, each optional (may be NULL, at least one is
 * needed), OVERWRITTEN, not accumulated into:
 *   grad_assign_w  [K][C]     dL/d conv.weight[:, :, 0, 0], summed over the images in image order
 *   grad_centroids [K][C]     dL/d centroids, summed over the images in image order
 *   grad_feat      [N][P][C]  dL/d feat; with NULL here that stage is not launched.
 * No floating-point atomics: results are bit-identical from run to run, an output does not depend on which other
 * outputs are requested, and the grad_feat rows of an image do not depend on its batch mates.
 * Workspace from oibl_netvlad_backward_workspace_bytes (linear in N, smaller without grad_feat; 0 for an invalid
 * shape), 256-byte aligned; the other pointers 16-byte aligned.  Invalid arguments (a null input, no output, K != 64,
 * C != 512, another precision, N or P < 1, N > 65535: the image index is a grid dimension) return OIBL_E_INVALID, a short or misaligned workspace OIBL_E_WORKSPACE;
 * nothing is launched then.                                                                                        */
size_t oibl_netvlad_backward_workspace_bytes(int N, int P, int K, int C, int want_grad_feat);
int oibl_netvlad_backward(const void* feat, int N, int P, int K, int C, int precision,
                          const float* assign_w, const float* centroids, int normalize_input,
                          const float* grad_vlad_norm, float* grad_assign_w, float* grad_centroids,
                          float* grad_feat, void* ws, size_t ws_bytes, void* stream);

/* ---- NetVLAD + intra-norm + L2 for other cluster counts: forward and gradients ------- *
 * The same two functions as oibl_netvlad_forward (fp32 map) and oibl_netvlad_backward for K = 16, 32, ..., 128
 * clusters (any multiple of 16; K = 64 is accepted too and agrees with the entry points above to rounding, not bit
 * for bit), C = 512, feat [N][P][C] fp32, any N >= 1 and P >= 1 with N ceil(P / 32) < 2^31.  Arguments, outputs and
 * guarantees are those of the two entry points above without `precision`: exact fp32 on v_mfma_f32_32x32x2_f32, the
 * backward stateless with fp64 logits, norms and normalisation gradients, every output optional and OVERWRITTEN, no
 * floating-point atomics, bit-identical from run to run, and an image's vlad rows and grad_feat rows do not depend on
 * its batch mates at ANY N (the pixels are cut into chunks of 32 whatever N is).
 * Workspaces from the two queries (0 for an invalid shape; non-decreasing in N, P and K), 256-byte aligned; the other
 * pointers 16-byte aligned.  Another K or C, a null input, no output, N or P < 1 return OIBL_E_INVALID with a message
 * that names num_clusters / dim and the value, a short or misaligned workspace OIBL_E_WORKSPACE; nothing is launched
 * then.                                                                                                            */
size_t oibl_netvlad_k_workspace_bytes(int N, int P, int K, int C);
int oibl_netvlad_forward_k(const void* feat, int N, int P, int K, int C, const float* assign_w,
                           const float* centroids, int normalize_input, float* vlad_raw, float* vlad_norm,
                           void* ws, size_t ws_bytes, void* stream);
size_t oibl_netvlad_k_backward_workspace_bytes(int N, int P, int K, int C, int want_grad_feat);
int oibl_netvlad_backward_k(const void* feat, int N, int P, int K, int C, const float* assign_w,
                            const float* centroids, int normalize_input, const float* grad_vlad_norm,
                            float* grad_assign_w, float* grad_centroids, float* grad_feat, void* ws,
                            size_t ws_bytes, void* stream);

/* ---- SFRS region head: gradients ---------------------------------------------------- *
 * The backward of oibl_region_vlad_forward and oibl_region_scores, i.e. of EmbedRegionNet._compute_region_sim
 * (ibl/models/netvlad.py:123-186) as torch autograd differentiates it under SFRSTrainer._forward
 * (ibl/trainers.py:235-259).  Stateless like oibl_netvlad_backward: per-pixel norms, soft-assignment and the four
 * quarter aggregates are recomputed from `feat`; the reference's residual[N*4][K][C][P/4] never exists.
 * oibl_region_vlad_backward: feat [N][h][w][C] fp32 (precision must be OIBL_F32; h and w even and >= 2, K = 64,
 *   C = 512, N <= 65535), grad_region_vlad [N][9][K*C] fp32 = dL/d region_vlad, regions in the forward's order.
 *   Outputs, each optional (may be NULL, at least one is needed), OVERWRITTEN, not accumulated into; a stage whose
 *   output is NULL is not launched:
 *     grad_assign_w  [K][C]        summed over the images in image order
 *     grad_centroids [K][C]        summed over the images in image order
 *     grad_feat      [N][h][w][C]  dL/d feat
 *   The heavy contractions are exact fp32 (v_mfma_f32_32x32x2_f32); logits, norms, the normalisations' backward and
 *   the per-image grad_centroids are fp64 (a tuple loss's contributions to grad_centroids cancel over a tuple).
 *   No floating-point atomics: bit-identical from run to run, an output does not depend on which other outputs are
 *   requested, an image's grad_feat rows do not depend on its batch mates.  Measured against float64 (rel-L2, maps
 *   of 2 x 2 to 30 x 40): dW 3.3e-7 .. 1.8e-6, dC 3.6e-8 .. 9.5e-7, dX 2.5e-7 .. 1.2e-6
 *   (tests/test_gpu_region_backward.py).
 *   Workspace from oibl_region_backward_workspace_bytes (linear in N, smaller without grad_feat; 0 for an invalid
 *   shape), 256-byte aligned; the other pointers 16-byte aligned.
 * oibl_region_scores_backward: region_vlad [T*per_tuple][9][L] as given to oibl_region_scores, grad_score
 *   [T][per_tuple-1][9][9] -> grad_region_vlad [T*per_tuple][9][L], OVERWRITTEN:
 *     anchor  dY[t,0][a]   = sum_j sum_b grad_score[t][j][a][b] Y[t,1+j][b]   (pairs in order, fp64 accumulators)
 *     pair j  dY[t,1+j][b] = sum_a grad_score[t][j][a][b] Y[t,0][a]
 *   A pair's rows do not depend on the other pairs.
 * Invalid arguments (a null input, no output, odd h or w, K != 64, C != 512, another precision, per_tuple < 2) return
 * OIBL_E_INVALID, a short or misaligned workspace OIBL_E_WORKSPACE; nothing is launched then.                     */
size_t oibl_region_backward_workspace_bytes(int N, int h, int w, int K, int C, int want_grad_feat);
int oibl_region_vlad_backward(const void* feat, int N, int h, int w, int K, int C, int precision,
                              const float* assign_w, const float* centroids, int normalize_input,
                              const float* grad_region_vlad, float* grad_assign_w, float* grad_centroids,
                              float* grad_feat, void* ws, size_t ws_bytes, void* stream);
int oibl_region_scores_backward(const float* region_vlad, int T, int per_tuple, int L, const float* grad_score,
                                float* grad_region_vlad, void* stream);

/* ---- Tuple losses and the soft-label loss, forward and backward --------------------- *
 * The losses of Trainer._get_loss (ibl/trainers.py:82-162), SFRSTrainer._get_loss / _get_hard_loss (:261-320) and
 * the soft term of SFRSTrainer._forward (:256-257), each fused into at most two launches forward and one backward.
 * A tuple is an anchor, a positive and M negatives, rows of L fp32 with a contiguous last dimension:
 *   anchors [B] rows stride_a apart, positives [B] rows stride_p apart, negatives [B][M] rows at
 *   b * stride_n_tuple + j * stride_n_row — strides in ELEMENTS, >= 0, so strided views (region 0 of a
 *   [B][1+M][9][L] tensor: row stride 9 L) are read in place.  Rows are read with 16-byte loads where the three base
 *   pointers are 16-byte aligned and every stride is a multiple of 4, with 4-byte loads otherwise: same bits.
 *   mode   OIBL_LOSS_TRIPLET     F.triplet_margin_loss(margin, p=2, reduction='mean') over the B M triples, with
 *                                pairwise_distance's eps = 1e-6 added to the difference; `score` and `temp` unused
 *          OIBL_LOSS_SARE_JOINT  mean over B of -log_softmax([z_pos, z_neg_1 .. z_neg_M])[0]
 *          OIBL_LOSS_SARE_IND    mean over B M of -log_softmax([z_pos, z_neg_j])[0]
 *   score  OIBL_SCORE_SQDIST     z = -|a - x|^2 (Trainer; `temp` unused)
 *          OIBL_SCORE_DOT        z = <a, x> / temp (SFRSTrainer), temp > 0
 * oibl_tuple_loss_forward -> loss (one fp32) and coef [B][1+M] fp64: per row of a tuple (positive first) the factor
 *   its gradient is a multiple of, 1 / count included.  Distances and dots, the hinge, the softmax and the table are
 *   fp64; a row is reduced in 8 chunks summed in chunk order.
 * oibl_tuple_loss_backward: the same rows, the table and grad_loss, a DEVICE pointer to the upstream fp32 scalar (no
 *   host synchronisation) -> compact grad_anchors [B][L], grad_positives [B][L], grad_negatives [B][M][L] fp32,
 *   OVERWRITTEN; each may be NULL (at least one is needed) and is then not computed.  A triplet whose hinge is
 *   inactive contributes exactly zero.
 * No atomics: bit-identical from run to run; a tuple's gradients depend on its batch mates through 1 / count only.
 * Limits: 1 <= B <= 65535, 1 <= M <= OIBL_TUPLE_LOSS_MAX_NEG, L >= 1.
 * Soft-label loss: student, teacher [B][J] fp32 contiguous ->
 *   loss = (-softmax(teacher / temp_teacher) * log_softmax(student / temp_student)).mean(0).sum(), one workgroup per
 *   row in fp64, and coef [B][J] fp64 = (softmax(student / temp_student) - softmax(teacher / temp_teacher)) /
 *   (B temp_student); the backward writes grad_student [B][J] = coef x *grad_loss.  1 <= B <= 65535,
 *   1 <= J <= OIBL_SOFT_LABEL_MAX_J, both temperatures > 0.
 * Workspaces from the two queries (0 outside the limits), 256-byte aligned; the tables 8-byte aligned.  Invalid
 * arguments return OIBL_E_INVALID, a short or misaligned workspace OIBL_E_WORKSPACE; nothing is launched then.    */
#define OIBL_LOSS_TRIPLET 0
#define OIBL_LOSS_SARE_JOINT 1
#define OIBL_LOSS_SARE_IND 2
#define OIBL_SCORE_SQDIST 0
#define OIBL_SCORE_DOT 1
#define OIBL_TUPLE_LOSS_MAX_NEG 64
#define OIBL_SOFT_LABEL_MAX_J 4096
size_t oibl_tuple_loss_workspace_bytes(int B, int M);
int oibl_tuple_loss_forward(const float* anchors, long long stride_a, const float* positives, long long stride_p,
                            const float* negatives, long long stride_n_tuple, long long stride_n_row, int B, int M,
                            int L, int mode, int score, double margin, double temp, float* loss, double* coef,
                            void* ws, size_t ws_bytes, void* stream);
int oibl_tuple_loss_backward(const float* anchors, long long stride_a, const float* positives, long long stride_p,
                             const float* negatives, long long stride_n_tuple, long long stride_n_row, int B, int M,
                             int L, int mode, int score, const double* coef, const float* grad_loss,
                             float* grad_anchors, float* grad_positives, float* grad_negatives, void* stream);
size_t oibl_soft_label_loss_workspace_bytes(int B, int J);
int oibl_soft_label_loss_forward(const float* student, const float* teacher, int B, int J, double temp_student,
                                 double temp_teacher, float* loss, double* coef, void* ws, size_t ws_bytes,
                                 void* stream);
int oibl_soft_label_loss_backward(const double* coef, int B, int J, const float* grad_loss, float* grad_student,
                                  void* stream);

/* ---- 3x3 convolution (+ ReLU): gradients -------------------------------------------- *
 * The backward of nn.Conv2d(Cin, Cout, 3, padding=1) followed by nn.ReLU (ibl/models/vgg.py:41-42, 61-62) as torch
 * autograd differentiates them: what trains conv5_1 .. conv5_3, the layers the reference's scripts leave unfrozen
 * (--layers conv5).  Exact fp32 (v_mfma_f32_32x32x2_f32); Cin = Cout = 512 only, every H, W >= 1.
 * in [N][H][W][Cin] fp32 NHWC, the layer's input; w_oihw [Cout][Cin][3][3] fp32, the state-dict tensor;
 * out_act NULL or the layer's post-ReLU output [N][H][W][Cout]: grad_out is taken as 0 where out_act <= 0;
 * grad_out [N][H][W][Cout] fp32: dL/d(output).  With dZ the masked grad_out, the outputs — each optional (may be
 * NULL, at least one is needed), OVERWRITTEN, not accumulated into; a stage whose output is NULL is not launched:
 *   grad_w  [Cout][Cin][3][3]  sum over n, y, x of dZ[n][y][x][co] in[n][y+ky-1][x+kx-1][ci], zeros outside the map
 *   grad_b  [Cout]             sum over n, y, x of dZ[n][y][x][co]
 *   grad_in [N][H][W][Cin]     the transposed convolution of dZ (taps flipped, Cin / Cout swapped)
 * The sums over the pixels run in chains of at most 256 products, the chains' results are added in a fixed order
 * (the last level in fp64, rounded once).  No floating-point atomics: results are bit-identical from run to run, an
 * output does not depend on which other outputs are requested, and the grad_in rows of an image do not depend on
 * its batch mates.
 * Workspace from oibl_conv3x3_backward_workspace_bytes (larger with grad_in; 0 for an invalid shape), 256-byte
 * aligned; the other pointers 16-byte aligned.  Invalid arguments (a null input, no output, other channel counts,
 * N, H or W < 1, N*H*W >= 2^31) return OIBL_E_INVALID, a short or misaligned workspace OIBL_E_WORKSPACE; nothing is
 * launched then.                                                                                                    */
size_t oibl_conv3x3_backward_workspace_bytes(int N, int H, int W, int cin, int cout, int want_grad_in);
int oibl_conv3x3_backward(const float* in, int N, int H, int W, int cin, const float* w_oihw, int cout,
                          const float* out_act, const float* grad_out, float* grad_w, float* grad_b,
                          float* grad_in, void* ws, size_t ws_bytes, void* stream);

/* ---- PCA-whitening projection + L2 ------------------------------------------------ *
 * Replaces EmbedNetPCA.pca_layer + F.normalize (netvlad.py:105-108) and PCA.infer
 * (ibl/pca.py:108-123):  y = normalize(W v + b).
 * v [N][D] fp32; w [d][D] T (row-major, i.e. pca_layer.weight[:, :, 0, 0], cast with
 * oibl_cast_f32_to_bf16 for OIBL_BF16); b [d] fp32; out [N][d] fp32.
 * D % 64 == 0, d % 128 == 0.  l2norm != 0 applies the final F.normalize.               */
size_t oibl_pca_workspace_bytes(int N, int D, int d, int precision);
int oibl_pca_forward(const float* v, int N, int D, const void* w, const float* b, int d,
                     int precision, int l2norm, float* out, void* ws, size_t ws_bytes,
                     void* stream);
/* The same projection in fp32 from a RE-PACKED copy of the weight (round 5): for 1 <= N <= 32 rows the weight
 * stream is the whole cost (537 MB for 32768 -> 4096), and the row-major matrix does not stream as an MFMA
 * operand.  oibl_pca_pack_weight writes w [d][D] fp32 once as 1 KB tiles ([32 output dims][8 k] in operand
 * lane order, the tiles of a 32-dim group consecutive along k; d * D floats, 16-byte aligned);
 * oibl_pca_forward_packed streams it (csrc/pca.hip, pca_stream_kernel).  Same arguments and workspace
 * (oibl_pca_workspace_bytes(N, D, d, OIBL_F32)) as oibl_pca_forward; results differ from it only by the
 * association of the fp32 sums.  oibl_pca_packed_supported: 1 where the packed form serves the shape
 * (N <= 32, d % 256 == 0, D % 8192 == 0), else the caller keeps oibl_pca_forward.                      */
int oibl_pca_pack_weight(const float* w, int D, int d, float* packed, void* stream);
int oibl_pca_packed_supported(int N, int D, int d);
int oibl_pca_forward_packed(const float* v, int N, int D, const float* w_packed, const float* b, int d,
                            int l2norm, float* out, void* ws, size_t ws_bytes, void* stream);

/* Row-wise L2 normalisation x / max(|x|_2, 1e-12)  (F.normalize(dim=-1), e.g. the extra
 * one in extract_cnn_feature, ibl/evaluators.py:29-33).  In place allowed. */
int oibl_l2_normalize_rows(const float* x, int N, int D, float* out, void* stream);
/* out[i] = normalize(xs[0][i] + xs[1][i] + ... + xs[S-1][i]), xs [S][N][D] fp32 (summed in that
 * order): fuses the per-scale descriptors of the multi-scale extraction (BASELINE.json configs[4];
 * no counterpart in the reference) into one unit-norm descriptor. */
int oibl_sum_l2_normalize(const float* xs, int S, int N, int D, float* out, void* stream);

/* ---- query x gallery squared-L2 --------------------------------------------------- *
 * Replaces the arithmetic of pairwise_distance (ibl/evaluators.py:122-129):
 *   dist[i][j] = |x_i|^2 + |y_j|^2 - 2 x_i . y_j      (no clamp, no sqrt)
 * x [m][d] fp32, y [n][d] fp32, dist [m][ldd] fp32 (ldd >= n).  d % 64 == 0.
 * OIBL_BF16 rounds x,y to bf16 for the dot product only (norms stay fp32).              */
size_t oibl_pairwise_workspace_bytes(int m, int n, int d, int precision);
int oibl_pairwise_sqdist(const float* x, int m, const float* y, int n, int d,
                         int precision, float* dist, size_t ldd, void* ws, size_t ws_bytes,
                         void* stream);

/* The same with descriptors stored as fp32, IEEE half or bf16 (OIBL_ST_*): the result is that of
 * oibl_pairwise_sqdist on the stored values widened to fp32 (norms from the widened values; in
 * OIBL_BF16 a bf16-stored operand is read in place, no copy).  x [m][d], y [n][d] of their types. */
size_t oibl_pairwise_st_workspace_bytes(int m, int n, int d, int precision, int x_st, int y_st);
int oibl_pairwise_sqdist_st(const void* x, int x_st, int m, const void* y, int y_st, int n, int d,
                            int precision, float* dist, size_t ldd, void* ws, size_t ws_bytes,
                            void* stream);

/* Fused distance + top-k: the k nearest gallery rows of every query without materialising the
 * [m][n] matrix — what Evaluator.evaluate / evaluate_all need from pairwise_distance + argsort
 * (ibl/evaluators.py:122-129, 143-159) when only ranks are consumed.
 *   out_val [m][k] fp32 ascending, out_idx [m][k] int32 = index_base + gallery row; ties broken
 *   by lowest index; n < k pads with (+inf, -1).  Same arithmetic as oibl_pairwise_sqdist, so the
 *   result equals oibl_row_topk applied to its matrix.
 * OIBL_BF16, large galleries: thresholds from a strided gallery sample, one filtered pass of the
 * distance kernel that appends only candidates, exact selection over the candidates.  A candidate
 * list that outgrows its capacity (possible only for degenerate data, e.g. thousands of duplicate
 * rows) sets *overflow (device int32, may be NULL) to 1 and leaves that call's outputs undefined:
 * repeat the call with exact = 1, which materialises distance tiles inside the workspace (always
 * used for OIBL_F32 and small problems; *overflow stays 0).                                   */
size_t oibl_sqdist_topk_workspace_bytes(int m, int n, int d, int k, int precision);
int oibl_sqdist_topk(const float* x, int m, const float* y, int n, int d, int k, int index_base,
                     int precision, int exact, float* out_val, int32_t* out_idx, int32_t* overflow,
                     void* ws, size_t ws_bytes, void* stream);
/* Storage-typed variant (see oibl_pairwise_sqdist_st). */
size_t oibl_sqdist_topk_st_workspace_bytes(int m, int n, int d, int k, int precision, int x_st,
                                           int y_st);
int oibl_sqdist_topk_st(const void* x, int x_st, int m, const void* y, int y_st, int n, int d, int k,
                        int index_base, int precision, int exact, float* out_val, int32_t* out_idx,
                        int32_t* overflow, void* ws, size_t ws_bytes, void* stream);

/* Prepared operands: a descriptor matrix that is matched many times (the resident gallery shard of
 * a retrieval service, the query set that meets every shard) pays the norm / operand pass once.
 *   oibl_match_operand_bytes : size of the operand buffer for (rows, d, precision, storage); 0 means
 *       the contraction reads the stored rows in place (OIBL_BF16 on bf16 storage, OIBL_F32 on fp32
 *       storage) and `operand` may be NULL.
 *   oibl_match_prepare : norms[rows] = fp32 squared norms of the rows widened to fp32 (the
 *       |x|^2 / |y|^2 terms of ibl/evaluators.py:127-128); operand = what the contraction reads:
 *       bf16 rows (OIBL_BF16), [32 hi | 32 lo] groups (OIBL_BF16X3), fp32 rows (OIBL_F32).
 *   oibl_sqdist_topk_prepared : oibl_sqdist_topk_st behind that pass, bit-identical results; xo / yo
 *       are the prepared operands (or the stored rows where operand_bytes is 0). */
size_t oibl_match_operand_bytes(int rows, int d, int precision, int st);
int oibl_match_prepare(const void* x, int x_st, int rows, int d, int precision, float* norms,
                       void* operand, void* stream);
size_t oibl_sqdist_topk_prepared_workspace_bytes(int m, int n, int d, int k, int precision);
int oibl_sqdist_topk_prepared(const void* xo, const float* xn, int m, const void* yo, const float* yn,
                              int n, int d, int k, int index_base, int precision, int exact,
                              float* out_val, int32_t* out_idx, int32_t* overflow, void* ws,
                              size_t ws_bytes, void* stream);

/* ---- "f16r": fp16 filter pass + exact rescoring ---------------------------------------------- *
 * The k nearest gallery rows per query by fp32 squared-L2 (pairwise_distance + the argsort prefix evaluate_all
 * reads, ibl/evaluators.py:105-130, 142-159) with EXACT lists at the cost of a 2-byte operand stream: every pair
 * is contracted once in fp16 (v_mfma_f32_32x32x16_f16, power-of-two row scales), kept if its distance could
 * belong to a member of the true top-k given a rigorous per-pair error bound (Cauchy-Schwarz on the fp16
 * rounding residuals + the fp32 accumulation slack d 2^-24), and the survivors near the k-th distance (k + a few
 * per query) are recomputed from the resident fp32 rows with fp64 accumulation.  out_val are
 * fl32((|x|^2 + |y|^2) - 2 x.y) with correctly rounded dot products; ties: lowest index first.  The lists do not
 * depend on the fp16 pass (csrc/match_f16r.h has the derivation).
 *   oibl_match_prepare_f16r : x [rows][d] fp32 (d % 64 == 0) -> norms[rows] (the fp32 squared norms of
 *       oibl_match_prepare), rows_f16 [rows][d] (IEEE binary16 of x 2^e, e per row), aux [rows][4] fp32 =
 *       {2^-e, |x| rounded up, |x - rows_f16 2^-e| rounded up, 0}.  The fp32 rows themselves are the fourth
 *       part of a prepared operand: they are read again by the rescoring.
 *   oibl_sqdist_topk_f16r : k <= 1024 (fused path: k <= 496); problems too small for the fused path, exact != 0,
 *       and the repeat after *overflow (device int32, may be NULL: a candidate list outgrew its capacity, or more
 *       than 32 (k <= 16; 2k + 32 otherwise) candidates sat within the bound of the k-th distance — near-duplicate
 *       galleries) take their member set from fp32 distance tiles + oibl_row_topk on the fp32 rows (what OIBL_F32
 *       runs: the oibl_f16r_members(k) nearest) and rescore it like the fused path does.                      */
int oibl_match_prepare_f16r(const float* x, int rows, int d, float* norms, float* aux, void* rows_f16,
                            void* stream);
/* The two stages of oibl_sqdist_topk_f16r on their own — for a caller that puts something between them: gallery-
 * sharded matching exchanges the FILTER lists first, takes the threshold from all shards' lists, and lets every rank
 * rescore only its members of the GLOBAL rescore set (openibl_amd/sharded.py: the rescoring work then divides by the
 * number of ranks instead of being repeated on each).
 *   oibl_f16r_members(k)        member slots per query: K2 = 32 (k <= 16), min(2k + 32, 1024) otherwise
 *   oibl_f16r_fused(m, n, d, k) 1 when the problem takes the fused path (else only oibl_sqdist_topk_f16r serves it)
 *   oibl_f16r_filter_select     stage 1 -> lval / lidx [m][K2]: filter distances and global indices of the candidates
 *       that can belong to the top-k of this gallery (any order; (+inf, -1) paddings); ymax_out (device, 2 floats, may
 *       be NULL): the gallery's largest |y| and largest fp16 residual norm — the pair bound of a query row i towards
 *       ANY row of it is eps_i = A_i ymax[0] + B_i ymax[1] + 1e-6 (|x_i|^2 + ymax[0]^2), A_i = 2 (r_i + g (n_i +
 *       r_i)), B_i = 2 (n_i + r_i)(1 + g), (n_i, r_i) = aux[i][1], aux[i][2], g = d 2^-24.  Workspace as
 *       oibl_sqdist_topk_f16r.
 *   oibl_f16r_rescore           stage 2: exact distances of the members listed in lidx [m][K2] (-1 = none), the k
 *       smallest (distance, index) per query, (+inf, -1) beyond the member count.                              */
int oibl_f16r_members(int k);
int oibl_f16r_fused(int m, int n, int d, int k);
int oibl_f16r_filter_select(const void* xh, const float* xaux, const float* xn, int m, const void* yh,
                            const float* yaux, const float* yn, int n, int d, int k, int index_base, float* lval,
                            int32_t* lidx, float* ymax_out, int32_t* overflow, void* ws, size_t ws_bytes,
                            void* stream);
int oibl_f16r_rescore(const float* xsrc, const float* xn, int m, const float* ysrc, const float* yn, int d, int k,
                      int index_base, const int32_t* lidx, float* out_val, int32_t* out_idx, void* stream);
/* Storage-typed f16r (descriptors stored as fp32, IEEE half or bf16: OIBL_ST_*, as oibl_pairwise_sqdist_st — the lists
 * are those of the stored values widened to fp32) and the whole ranked prefix the reference ever reads: k up to 496
 * on the fused path (spatial NMS looks at max(recall_topk) * 12 = 120 ranks, ibl/evaluators.py:152-153,
 * examples/test.py:130; the k-th filter distance of a list comes from a bisection instead of k register rounds,
 * csrc/match_f16r.h).  An fp16-stored row is its own fp16 image (residual 0): the filter bound of such a gallery is
 * the fp32 accumulation slack alone.  The rescoring reads the STORED rows (8 KB instead of 16 KB per 4096-d member).
 *   oibl_match_prepare_f16r_st        oibl_match_prepare_f16r on stored rows (norms of the widened rows)
 *   oibl_sqdist_topk_f16r_st          xsrc / ysrc = the stored rows; workspace from the _st query.  EVERY path ends in
 *       the same rescoring: the exact path (small problems, exact != 0, the repeat after *overflow) takes the
 *       oibl_f16r_members(k) nearest by fp32 distance tiles and rescores those, so values and tie order do not depend
 *       on the path that produced the member set.
 *   oibl_f16r_rescore_st              stage 2 with an explicit member-slot count (lidx [m][members], <= 1024)      */
int oibl_match_prepare_f16r_st(const void* x, int x_st, int rows, int d, float* norms, float* aux, void* rows_f16,
                               void* stream);
size_t oibl_sqdist_topk_f16r_st_workspace_bytes(int m, int n, int d, int k, int x_st, int y_st);
int oibl_sqdist_topk_f16r_st(const void* xh, const float* xaux, const float* xn, const void* xsrc, int x_st, int m,
                             const void* yh, const float* yaux, const float* yn, const void* ysrc, int y_st, int n,
                             int d, int k, int index_base, int exact, float* out_val, int32_t* out_idx,
                             int32_t* overflow, void* ws, size_t ws_bytes, void* stream);
int oibl_f16r_rescore_st(const void* xsrc, int x_st, const float* xn, int m, const void* ysrc, int y_st,
                         const float* yn, int d, int k, int members, int index_base, const int32_t* lidx,
                         float* out_val, int32_t* out_idx, void* stream);
/* Between the stages, sharded: thr [m] (device) = the k-th smallest filter distance over the lists of ALL shards,
 * ymax_all [shards][2] (device) = every shard's ymax_out; entries of lidx [m][K2] whose lval exceeds thr + 2 eps (eps
 * from the maxima over all shards) are set to -1. */
int oibl_f16r_keep_members(const float* lval, int32_t* lidx, int m, int k, const float* thr, const float* xn,
                           const float* xaux, const float* ymax_all, int shards, int d, void* stream);
size_t oibl_sqdist_topk_f16r_workspace_bytes(int m, int n, int d, int k);
int oibl_sqdist_topk_f16r(const void* xh, const float* xaux, const float* xn, const float* xsrc, int m,
                          const void* yh, const float* yaux, const float* yn, const float* ysrc, int n, int d,
                          int k, int index_base, int exact, float* out_val, int32_t* out_idx, int32_t* overflow,
                          void* ws, size_t ws_bytes, void* stream);

/* ---- top-k ------------------------------------------------------------------------ *
 * Replaces np.argsort(distmat, axis=1) (ibl/evaluators.py:143), of which evaluate_all only
 * consumes the first max(recall_topk) (or 12x that with nms) entries per row.
 * Per row of vals [m][ld] keep the k smallest, ascending, ties broken by lowest index:
 *   out_val [m][k] fp32, out_idx [m][k] int32.
 * idx_in == NULL: element j of a row has index index_base + j (gallery shard offset);
 * idx_in != NULL ([m][ld] int32): element j has index idx_in[row][j] (cross-shard merge).
 * 1 <= k <= 1024; if n < k the tail is filled with (+inf, -1).                          */
int oibl_row_topk(const float* vals, const int32_t* idx_in, int m, int n, size_t ld, int k,
                  int index_base, float* out_val, int32_t* out_idx, void* stream);

/* Full-row ranking: out_idx [m][n] int32 = stable ascending argsort of every row of vals [m][ld]
 * (ties: lowest index first), out_val [m][n] the sorted values (may be NULL).  Replaces
 * torch.argsort(distmat, dim=1) of the hard-negative mining samplers
 * (ibl/utils/data/sampler.py:46-54, 126-135) and serves evaluate_all when more than 1024 ranks per
 * query are needed (np.argsort, ibl/evaluators.py:143).  Per-row radix sort, any n. */
size_t oibl_row_argsort_workspace_bytes(int m, int n);
int oibl_row_argsort(const float* vals, int m, int n, size_t ld, int32_t* out_idx, float* out_val,
                     void* ws, size_t ws_bytes, void* stream);

/* ---- hard-negative mining, per anchor row ---------------------------------------------- *
 * Replaces the per-anchor bookkeeping of the tuple samplers' __iter__ (ibl/utils/data/sampler.py:62-86,
 * 143-190: the membership tests over the whole ranked row) for the A anchors of one mining round.
 *   dist [A][ld] fp32        the anchors' distance rows over G gallery items.  "Rank order" of a row is
 *                            ascending (distance, gallery index): the order of oibl_row_argsort, which ranks
 *                            the rows inside this entry (bit patterns: -0.0 sorts before +0.0).
 *   csr_row [A] int32        the row of the two CSR lists that belongs to anchor a; NULL: row a.
 *   pos_off / pos_val        CSR, int32: the anchor's positives; every row ascending, without repeats, inside
 *   excl_off / excl_val      [0, G) (np.unique of the sampler's pos_list / neg_list entry); the exclusion zone.
 *                            The caller guarantees offsets and rows (they live on the device).
 *   cache [A][C] int32       last round's negatives, -1 = none; C <= 64 (C = 0: cache, cache_pos may be NULL).
 *   jac [A][jac_ld] fp32     the k-reciprocal distances of the same rows, or NULL.
 * Per anchor:
 *   cand [A][cand_ld]        the row in rank order without the excluded entries, -1 behind cand_len[a];
 *                            cand_ld >= G.
 *   cand_len [A]
 *   cache_pos [A][C]         the position in cand of cache[a][c]; -1 for a -1 entry and for an excluded one.
 *   pos_ranked [A][pos_pool] the anchor's positives in rank order, the first pos_pool of them, -1 behind;
 *                            column 0 is the easiest positive.  1 <= pos_pool <= 1024.
 *   pos_jac [A][pos_pool]    jac[a][pos_ranked[a][j]], NaN where pos_ranked is -1; untouched when jac is NULL.
 * One pass over the ranked row per anchor; exclusion lists of up to 4096 entries are searched in LDS, longer
 * ones in global memory.  Integer results and copied floats only, no atomics: identical bits from run to run.
 * The workspace holds the ranking and the sort's buffers: 20 bytes per element of dist; a caller bounds it by
 * mining the rows in groups (every pointer advanced by the rows done; csr_row or the offsets likewise). */
size_t oibl_mine_rows_workspace_bytes(int A, int G);
int oibl_mine_rows(const float* dist, int A, int G, size_t ld, const int32_t* csr_row, const int32_t* pos_off,
                   const int32_t* pos_val, const int32_t* excl_off, const int32_t* excl_val, const int32_t* cache,
                   int C, const float* jac, size_t jac_ld, int pos_pool, int32_t* cand, size_t cand_ld,
                   int32_t* cand_len, int32_t* cache_pos, int32_t* pos_ranked, float* pos_jac, void* ws,
                   size_t ws_bytes, void* stream);

/* ---- training colour jitter on raw uint8 batches ------------------------------------------ *
 * Replaces ColorJitter(0.7, 0.7, 0.7, 0.5) of get_transformer_train (ibl/utils/data/__init__.py:29-35; torchvision
 * delegates to PIL's ImageEnhance.Brightness / Contrast / Color and to a hue shift through PIL's HSV mode) and,
 * for out_kind OIBL_JITTER_F32_NCHW, the ToTensor + Normalize behind it.  The arithmetic is PIL's, rounding by
 * rounding (csrc/augment.hip states it): the uint8 result equals PIL's bit for bit.
 *   x_nhwc [N][H][W][3] uint8   the loader's raw images (any byte alignment; bases that are 4-byte aligned are
 *                               read and written with whole dwords).
 *   records [N] x 32 bytes      one record per image, eight 32-bit words:
 *                                 words 0..3  int32 op codes in application order: 0 brightness, 1 contrast,
 *                                             2 saturation, 3 hue, anything else (-1) skip; every op at most once
 *                                             (a second contrast op in a record is skipped);
 *                                 words 4..6  fp32 factors of brightness, contrast, saturation;
 *                                 word  7     the hue shift added to the H byte, 0..255 (mod 256).  The hue op is
 *                                             the HSV round trip even when the shift is 0 (it is lossy).
 *                               NULL: no jitter — one launch, the plain copy / normalisation.
 *   out_kind OIBL_JITTER_U8_NHWC   out [N][H][W][3] uint8, the jittered images; mean3_host / std3_host unused.
 *            OIBL_JITTER_F32_NCHW  out [N][3][H][W] fp32 = (float(u8) / 255.0f - mean_c) / std_c, both divisions
 *                               IEEE: the bits of the loader's host transform on the jittered bytes.
 * Two launches: per-workgroup integer partial sums of the luma behind the ops ordered before contrast (images
 * without a contrast op return at once), then the pass that finishes the sum, recomputes the prefix and applies
 * everything.  Integer sums, no atomics: identical bits from run to run, and an image's result does not depend on
 * the rest of the batch.  H * W <= 2^28.  Workspace: the partial sums (8 bytes each, at most 1024 per image). */
#define OIBL_JITTER_U8_NHWC 0
#define OIBL_JITTER_F32_NCHW 1
size_t oibl_color_jitter_u8_workspace_bytes(int N, int H, int W);
int oibl_color_jitter_u8(const uint8_t* x_nhwc, int N, int H, int W, const void* records, int out_kind,
                         const float* mean3_host, const float* std3_host, void* out, void* ws, size_t ws_bytes,
                         void* stream);

/* ---- bilinear resize of raw uint8 batches -------------------------------------------------- *
 * Replaces Resize of get_transformer_train / get_transformer_test (ibl/utils/data/__init__.py:
 * img.resize((w, h), Image.BILINEAR) through torchvision and PIL on the host) and, for out_kind
 * OIBL_JITTER_F32_NCHW, the ToTensor + Normalize behind it.  The arithmetic is PIL's 8-bit resampling
 * (csrc/resize_tables.h, csrc/resize.hip state it): per axis a table of windows and 22-bit fixed-point triangle
 * weights computed in IEEE double, then two integer passes, horizontal first, with a uint8 intermediate.  The uint8
 * result equals PIL's bit for bit; a pass whose size does not change is the exact identity.
 *   x_nhwc [N][H][W][3] uint8   the stored images (any byte alignment).
 *   H2, W2                      the target size.  One path only: a workgroup keeps the source rows of its tile of
 *                               16 x 64 output pixels in LDS (at most 64 KiB of it), so H <= 16 H2 and W <= 16 W2
 *                               (a downscale factor of at most 16 per axis; upscaling is not limited); beyond
 *                               that OIBL_E_INVALID with a message that names the limit.  N <= 65535, every size
 *                               <= 32768.
 *   out_kind OIBL_JITTER_U8_NHWC   out [N][H2][W2][3] uint8 (any byte alignment); mean3_host / std3_host unused.
 *            OIBL_JITTER_F32_NCHW  out [N][3][H2][W2] fp32 = (float(u8) / 255.0f - mean_c) / std_c, both divisions
 *                               IEEE: what oibl_color_jitter_u8 without records gives on the resized bytes.
 * Three launches: the two tables are built ON THE DEVICE into the workspace (fp64, one thread per output
 * coordinate), then one fused launch runs both passes.  No host memory, no copy and nothing owned by the library:
 * the call is stream-ordered and can be captured into a graph.  Integer sums, no atomics: identical bits from run
 * to run, and an image's result does not depend on the rest of the batch.
 * Workspace: per axis int32 bounds[out][2] and int32 coeff[out][ksize], each rounded up to 256 bytes (it does not
 * depend on N); oibl_resize_u8_workspace_bytes returns 0 for a shape oibl_resize_u8 rejects.
 *
 * oibl_resize_u8_tables builds the tables of ONE axis, in_size -> out_size samples, into caller memory (device,
 * 4-byte aligned): bounds[out_size][2] = {first source sample, number of taps} and coeff[out_size][ksize], the taps'
 * weights times 2^22, rounded, zero behind the last tap; ksize = 2 ceil(max(in_size / out_size, 1)) + 1 is the row
 * length and is written to *ksize_out_host_or_null on the host before the launch.  ksize_capacity: the row length
 * the caller sized coeff for; a larger ksize is OIBL_E_INVALID and nothing is launched.  No scale limit here. */
size_t oibl_resize_u8_workspace_bytes(int N, int H, int W, int H2, int W2);
int oibl_resize_u8_tables(int in_size, int out_size, int32_t* bounds, int32_t* coeff, int ksize_capacity,
                          int* ksize_out_host_or_null, void* stream);
int oibl_resize_u8(const uint8_t* x_nhwc, int N, int H, int W, int H2, int W2, int out_kind,
                   const float* mean3_host, const float* std3_host, void* out, void* ws, size_t ws_bytes,
                   void* stream);

/* ---- baseline JPEG decoding ------------------------------------------------------------------ *
 * Replaces `Image.open(path).convert('RGB')` of the loader (ibl/utils/data/preprocessor.py) for baseline JPEG files:
 * from the scan's bytes to [N][H][W][3] uint8, the bits of libjpeg-turbo as Pillow uses it (csrc/jpeg.hip and
 * csrc/jpeg_entropy.h state the arithmetic: T.81 F.2.2 entropy decoding, coef * q in int32, the "islow" integer IDCT,
 * "fancy" h2v1 / h2v2 chroma upsampling on the cropped planes, 16-bit fixed-point YCbCr -> RGB).  Equality holds for
 * streams whose dequantised coefficients stay inside int16, as every encoder of 8-bit images keeps them.
 * The markers are parsed on the host (openibl_amd/jpeg.py: `parse`, `collate`); all N images have the size H x W.
 *   scan_bytes [scan_len] uint8   the entropy-coded bytes of all images, back to back, restart markers included
 *                                 (1 <= scan_len < 2^31).
 *   records [N][1408] bytes       per image, 4-byte aligned:
 *       int32 header[16]: 0 components (1 or 3); 1, 2 luma sampling factors h, v — (1,1), (2,1) or (2,2), chroma is
 *                         (1,1); 3..5 quantisation table of each component (0..3); 6..8 its DC table (0, 1);
 *                         9..11 its AC table (0, 1); 12 DRI, the restart interval in MCUs (0: none);
 *                         13 the image's first row of `segments`; 14 how many rows it has;
 *                         15 status slot: a non-zero value found by the parser (4: restart markers missing or out of
 *                         sequence) is what status[n] reports, whatever the device finds.
 *       uint8 qt[4][64]   the 8-bit quantisation tables in natural (row-major) order.
 *       uint8 huff[4][272] DC table 0, DC table 1, AC table 0, AC table 1: counts[16] of the code lengths 1..16, then
 *                         values[256] in code order (unused entries anything).
 *     Every field is forced into its valid range on the device (other values read as the nearest valid one): a
 *     damaged record cannot make a kernel index outside its buffers.
 *   segments [S][2] int32         {begin, end} byte offsets into scan_bytes of every segment — a restart interval, or
 *                                 the whole scan when DRI = 0 — image after image in decoding order; the marker
 *                                 FF D0+(k mod 8) stands at `end` of an image's k-th segment unless it is the last.
 *                                 Offsets beyond scan_len are clamped.  max_segments: the largest header[14].
 *   out_nhwc [N][H][W][3] uint8, status [N] int32 (device): 0 ok, 1 a code no Huffman length matches, 2 a coefficient
 *                                 index above 63, 3 a segment ran out of bytes, 4 a restart marker missing or wrong
 *                                 (or bytes left in front of the marker that ends a segment).  A damaged image yields
 *                                 the pixels of what was decoded; its batch mates are not affected.
 * One memset and three launches, all stream-ordered and capturable: one lane per segment decodes into zeroed int16
 * coefficients, one thread per 8 x 8 block dequantises and transforms, one thread per pixel upsamples and converts.
 * Integer sums only, no atomics: identical bits from run to run, whatever lane served a segment.
 * 1 <= N <= 65535, 1 <= H <= 32768, 8 <= W <= 32768, N <= S <= 2^28; otherwise OIBL_E_INVALID before anything is
 * launched, as for a null pointer; a short or misaligned (256 bytes) workspace is OIBL_E_WORKSPACE / OIBL_E_INVALID.
 * Workspace: int16 coef[N][3][Bh][Bw][64] with Bw = 2 ceil(W / 16), Bh = 2 ceil(H / 16), int32 segment status [S],
 * uint8 planes[N][3][Bh * 8][Bw * 8]; oibl_jpeg_decode_workspace_bytes returns 0 for a shape the call rejects. */
size_t oibl_jpeg_decode_workspace_bytes(int N, int H, int W, int S);
int oibl_jpeg_decode(const uint8_t* scan_bytes, size_t scan_len, const void* records, const int32_t* segments, int S,
                     int max_segments, int N, int H, int W, uint8_t* out_nhwc, int32_t* status, void* ws,
                     size_t ws_bytes, void* stream);

/* The same decoder with many lanes inside one segment, for scans without restart markers, where oibl_jpeg_decode has
 * one lane per image (csrc/jpeg.hip and csrc/jpeg_chunked.h state the method: self-synchronising Huffman
 * decoding).  Arguments, record, segment table, output and status are those of oibl_jpeg_decode, and so are the bits.
 * Every segment is cut into chunks of chunk_bytes raw bytes (4 <= chunk_bytes <= 65536); one workgroup serves a
 * segment with a lane per chunk, at most 1024 — the last lane takes what is left.  The lanes decode their chunks from
 * a guessed state without writing, exchange exit states through LDS until no lane's entry changes (at most as many
 * rounds as lanes, separated by workgroup barriers: no waiting on another workgroup, no spinning, no atomics), take
 * their first block and DC predictors from a prefix over the chunks and decode once more, strictly, into the zeroed
 * coefficients.  The one difference from oibl_jpeg_decode: behind the first damaged block of a damaged segment the
 * coefficients may hold other bounded garbage than there; in front of it, and in the status, there is none.
 * One memset and three launches, stream-ordered and capturable; validation as for oibl_jpeg_decode, before anything
 * is launched.  Workspace: int16 coef[N][3][Bh][Bw][64], int32 segment status [S], int32 settle rounds [S] (for
 * measurements), uint8 planes[N][3][Bh * 8][Bw * 8], each aligned to 256 bytes;
 * oibl_jpeg_decode_chunked_workspace_bytes returns 0 for what the call rejects. */
size_t oibl_jpeg_decode_chunked_workspace_bytes(int N, int H, int W, int S, int chunk_bytes);
int oibl_jpeg_decode_chunked(const uint8_t* scan_bytes, size_t scan_len, const void* records, const int32_t* segments,
                             int S, int max_segments, int N, int H, int W, int chunk_bytes, uint8_t* out_nhwc,
                             int32_t* status, void* ws, size_t ws_bytes, void* stream);

/* ---- JPEG batches of mixed stored sizes -------------------------------------------------------- *
 * The decoder and the resize above for a batch whose images have sizes of their own (a folder that mixes portrait and
 * landscape, or several camera resolutions): all segments of all images decode in ONE entropy launch into a PACKED
 * pixel buffer — image n a contiguous [H_n][W_n][3] uint8 block at its byte offset — and ONE resize launch reads the
 * packed buffer into the dense batch [N][H2][W2][3] the model takes.  The arithmetic, the record, the segment table,
 * the statuses and the bits are those of oibl_jpeg_decode / oibl_jpeg_decode_chunked / oibl_resize_u8 (the same
 * kernel text: csrc/jpeg_stages.h, resize_tile of csrc/resize.hip); an image's result does not depend on its batch
 * mates or its position.  The uniform entry points stay what a batch of one size takes.
 *
 * oibl_jpeg_mixed_layout (host only, nothing is launched or copied): sizes_host [N][2] int32 = {H, W} ->
 *   geom_host [N][8] int32, the per-image geometry table: 0 H; 1 W; 2 the image's base in the int16 coefficients, in
 *             blocks of 64 coefficients; 3 its base in the uint8 sample planes, in units of 64 bytes (the same number:
 *             the images lie back to back in both, each as [3][Bh][Bw] blocks with Bw = 2 ceil(W / 16),
 *             Bh = 2 ceil(H / 16), the uniform decoder's 9 bytes per MCU-padded pixel); 4, 5 its byte offset in the
 *             packed pixels, low 32 bits and high bits (every image starts on a multiple of 64 bytes); 6, 7 zero.
 *   totals_host [6] size_t: 0 coefficient bytes; 1 sample-plane bytes; 2 packed pixel bytes (the end of the last
 *             image); 3 the largest Bw * Bh; 4 the largest H; 5 the largest W.
 *   1 <= N <= 65535, every side in [1, 32768], fewer than 2^31 coefficient blocks and fewer than 2^40 packed pixel
 *   bytes; otherwise OIBL_E_INVALID with a message that names the image.  The caller copies the table to the device
 *   with the batch's other tensors; a caller that decodes only some of the images (the others were decoded on the
 *   host and copied into their slots of the packed buffer) lays those out on their own for entries 2 and 3 and keeps
 *   entries 4 and 5 of the whole batch's layout.
 *
 * oibl_jpeg_decode_mixed: scan_bytes, scan_len, records, segments, S, max_segments, N, status as for oibl_jpeg_decode
 *   (N images with a record each, 8 <= W_n).
 *   geom_dev [N][8] int32 (device, 4-byte aligned), totals_host [6] (host) as above.
 *   chunk_bytes   0: the serial route, a lane per segment; 4..65536: the chunked route, a workgroup per segment.
 *   out_packed    uint8 [totals_host[2]] (device): only the bytes of the N images are written.
 *   status [N]    as for oibl_jpeg_decode, and 5: the image's row of the geometry table is inconsistent — a side
 *                 outside its range or beyond totals_host[4] / [5], or an extent that passes the end of the
 *                 coefficients, the planes or the packed pixels as totals_host gives them.  Such an image is skipped
 *                 by every stage.  Every entry of the table is forced into its range on the device and every extent
 *                 is checked there against the call's totals: no read or write depends on the table being right.
 *   One memset and three launches, stream-ordered and capturable; the grids of the IDCT and colour stages are sized by
 *   totals_host[3..5], and a workgroup outside its image leaves at once.  OIBL_E_INVALID before anything is launched
 *   for a null pointer, N or S outside 1 <= N <= 65535, N <= S <= 2^28, totals that no layout has, chunk_bytes,
 *   scan_len, max_segments or a misaligned pointer; a short workspace is OIBL_E_WORKSPACE.
 *   Workspace: int16 coef [totals_host[0] bytes], int32 segment status [S], int32 settle rounds [S], uint8 planes
 *   [totals_host[1] bytes], each aligned to 256 bytes; oibl_jpeg_decode_mixed_workspace_bytes returns 0 for what the
 *   call rejects.
 *
 * oibl_resize_u8_mixed: packed [packed_bytes] uint8 (device), geom_dev [N][8] (entries 0, 1, 4, 5 are read),
 *   sizes_host [N][2] int32 = {H, W} (host: it sizes the tables, the LDS and checks the limits), H2, W2, out_kind,
 *   mean3_host, std3_host, out as for oibl_resize_u8: out [N][H2][W2][3] uint8 or [N][3][H2][W2] fp32.
 *   Two launches: one builds every image's two tables into the workspace, with rows of the batch's largest ksize per
 *   axis; one runs both passes for every tile of every image, its LDS sized by the batch's largest need.  The limits
 *   are those of oibl_resize_u8 per image (H_n <= 16 H2, W_n <= 16 W2, every size <= 32768, N <= 65535) and
 *   1 <= packed_bytes < 2^40; OIBL_E_INVALID names the image.  On the device H_n, W_n are forced into [1, the largest
 *   of sizes_host] and the extent is checked against packed_bytes; an image whose row fails that check reads nothing
 *   and its output is that of zero bytes.
 *   Workspace: int32 bounds_h [N][W2][2], coeff_h [N][W2][ksh], bounds_v [N][H2][2], coeff_v [N][H2][ksv], each
 *   aligned to 256 bytes; oibl_resize_u8_mixed_workspace_bytes returns 0 for what the call rejects. */
int oibl_jpeg_mixed_layout(const int32_t* sizes_host, int N, int32_t* geom_host, size_t* totals_host);
size_t oibl_jpeg_decode_mixed_workspace_bytes(const size_t* totals_host, int N, int S);
int oibl_jpeg_decode_mixed(const uint8_t* scan_bytes, size_t scan_len, const void* records, const int32_t* segments,
                           int S, int max_segments, int N, const int32_t* geom_dev, const size_t* totals_host,
                           int chunk_bytes, uint8_t* out_packed, int32_t* status, void* ws, size_t ws_bytes,
                           void* stream);
size_t oibl_resize_u8_mixed_workspace_bytes(const int32_t* sizes_host, int N, int H2, int W2);
int oibl_resize_u8_mixed(const uint8_t* packed, size_t packed_bytes, const int32_t* geom_dev,
                         const int32_t* sizes_host, int N, int H2, int W2, int out_kind, const float* mean3_host,
                         const float* std3_host, void* out, void* ws, size_t ws_bytes, void* stream);

/* oibl_color_jitter_u8_mixed: the training colour jitter (oibl_color_jitter_u8) on the packed buffer, between
 * oibl_jpeg_decode_mixed and oibl_resize_u8_mixed — the reference's order ColorJitter -> Resize for files of any mix
 * of stored sizes.
 *   packed [packed_bytes] uint8 (device), geom_dev [N][8] (device, 4-byte aligned; entries 0, 1, 4, 5 are read) as
 *   above; sizes_host [N][2] int32 = {H, W} (host: it sizes the grid and the workspace and checks the limits).
 *   records [N] x 32 bytes as for oibl_color_jitter_u8 (device, 4-byte aligned).  NULL: no jitter — with
 *   out_packed != packed one launch copies the images' bytes, with out_packed == packed nothing is launched.
 *   out_packed uint8 (device) with the layout of packed: only the bytes of the N images are written.
 *   out_packed == packed (in place) is supported; any other overlap is not.
 * The same kernel text as the uniform call, in two launches with the grid (largest part count of the batch, N); a
 * workgroup outside its image leaves at once.  An image's chunk and part count come from its OWN H_n W_n, so its
 * integer partial sums, and its bits, are those of oibl_color_jitter_u8 on that image alone, whatever its batch mates
 * or its position; no atomics, no floating-point reduction.  Every image starts on a multiple of 64 bytes, so it is
 * read and written with whole dwords; the group of four pixels that holds an image's end goes by bytes and touches
 * nothing behind H_n W_n 3 — not the padding, not the next image's slot.
 * On the device every entry of a row is forced into its range, the extent is checked against packed_bytes and the
 * part count against the grid; an image whose row fails is skipped by both launches: it reads and writes nothing.
 * 1 <= N <= 65535, every side in [1, 32768], H_n W_n <= 2^28, 1 <= packed_bytes < 2^40; otherwise OIBL_E_INVALID
 * before anything is launched, with a message that names the image; a short or misaligned (256 bytes) workspace is
 * OIBL_E_WORKSPACE.  Stream-ordered, capturable, nothing owned.
 * Workspace (needed with records only): uint64 partial sums [N][largest part count];
 * oibl_color_jitter_u8_mixed_workspace_bytes returns 0 for what the call rejects. */
size_t oibl_color_jitter_u8_mixed_workspace_bytes(const int32_t* sizes_host, int N);
int oibl_color_jitter_u8_mixed(const uint8_t* packed, size_t packed_bytes, const int32_t* geom_dev,
                               const int32_t* sizes_host, int N, const void* records, uint8_t* out_packed, void* ws,
                               size_t ws_bytes, void* stream);

/* ---- recall counting ---------------------------------------------------------------- *
 * Replaces the per-query Python loop of evaluate_all and spatial_nms
 * (ibl/evaluators.py:132-140, 149-160).  For every query, the rank (0-based, inside the
 * prediction list the reference builds) of the first prediction that is a ground-truth
 * neighbour, -1 if there is none; Recall@N = #(0 <= rank < N) / m for any N.
 *   topk_idx [m][k] int32 ranked gallery positions (-1 = padding), k <= 1024
 *   gt_offsets [m+1], gt_values [gt_offsets[m]] int32: ground truth in CSR form
 *   gallery_pids [n] int32 or NULL.  Non-NULL switches on spatial NMS: only the first
 *   nms_window (= 12 * max(recall_topk) in the reference) predictions count and a prediction
 *   whose pid occurred earlier in the list is dropped.                                        */
int oibl_first_hit_rank(const int32_t* topk_idx, int m, int k, const int32_t* gt_offsets,
                        const int32_t* gt_values, const int32_t* gallery_pids, int nms_window,
                        int32_t* out_rank, void* stream);

/* ---- k-reciprocal re-ranking from descriptor rows -------------------------------------- *
 * Replaces re_ranking (ibl/utils/rerank.py:32-100; Evaluator.evaluate(rerank=True), ibl/evaluators.py:190-200, and
 * the SFRS trainer's update_sampler(rerank=True)) without its dense (Q+G) x (Q+G) arrays.  X = [queries; gallery],
 * n = Q + G rows of d floats; D[i][j] = (|x_i|^2 + |x_j|^2) - 2 x_i.x_j; O[i][j] = D[i][j]^2 / m_i.  One entry per
 * stage, in the order a caller runs them (openibl_amd/rerank.py: re_ranking_features); the neighbour lists `rank`
 * [n][ld] int32 (nearest first, the item itself included, -1 = none) come from oibl_sqdist_topk* of X against X.
 * Limits: k1 <= 31, k2 <= 8, (k1 + 1)(half + 2) <= 576.  No floating-point atomics: results are bit-identical from
 * run to run.
 *   oibl_rerank_row_extremes  x [n][d] fp32 (d % 32 == 0) -> norms [n] = |x_i|^2 and rowmax [n] = m_i =
 *       max(dmax_i^2, dmin_i^2) over row i of D, contracted in fp32 on the matrix cores; D is never written.
 *   oibl_rerank_set_stride    (k1 + 1)(half + 2): the most members a set can have; 0 beyond the limits.
 *   oibl_rerank_sets          half = round(k1 / 2).  idx [n][stride] <- per item the k1-reciprocal set (j among the
 *       k1 + 1 nearest of i with i among the k1 + 1 nearest of j), expanded by the half-reciprocal set of each member
 *       when 3 |sub & base| > 2 |sub| (rerank.py:58-65), sorted ascending without repeats; cnt [n] <- its size.
 *   oibl_rerank_weights       val [n][stride] <- exp(-O[i][idx[i][t]]) / sum over the set (rerank.py:68-69), every
 *       distance recomputed from the two rows with a fp32 dot product.
 *   oibl_rerank_expand        k2 > 1 (rerank.py:71-75): (idx2, val2, cnt2) [n][stride2 >= k2 * stride] <- the mean of
 *       the sparse rows of the k2 nearest items of i, summed in rank order.
 *   oibl_rerank_invert        nnz = sum of cnt (the caller adds it up).  col_off [n + 1], inv_row / inv_val [nnz] <-
 *       per column c the rows i that hold it, ascending, and their values (rerank.py:78-80).
 *   oibl_rerank_jaccard       dist [Q][ldd]: on entry D of the query rows against the GALLERY rows (X[Q..n)), on
 *       return (1 - lambda) (1 - s / (2 - s)) + lambda D^2 / m_i with s[i][j] = sum_c min(V[i][c], V[Q + j][c]),
 *       added in ascending c (rerank.py:82-98); each product, quotient and sum rounded to fp32 on its own, as numpy
 *       does.  one_minus_lambda is passed beside lambda so that both are the caller's fp32 roundings.      */
size_t oibl_rerank_row_extremes_workspace_bytes(int n, int d);
int oibl_rerank_row_extremes(const float* x, int n, int d, float* norms, float* rowmax, void* ws, size_t ws_bytes,
                             void* stream);
int oibl_rerank_set_stride(int k1, int half);
int oibl_rerank_sets(const int32_t* rank, int ld, int n, int k1, int half, int32_t* idx, int32_t* cnt, int stride,
                     void* stream);
int oibl_rerank_weights(const float* x, const float* norms, const float* rowmax, int n, int d, const int32_t* idx,
                        const int32_t* cnt, int stride, float* val, void* stream);
int oibl_rerank_expand(const int32_t* rank, int ld, int n, int k2, const int32_t* idx, const float* val,
                       const int32_t* cnt, int stride, int32_t* idx2, float* val2, int32_t* cnt2, int stride2,
                       void* stream);
size_t oibl_rerank_invert_workspace_bytes(int n, size_t nnz);
int oibl_rerank_invert(const int32_t* idx, const float* val, const int32_t* cnt, int stride, int n, size_t nnz,
                       int32_t* col_off, int32_t* inv_row, float* inv_val, void* ws, size_t ws_bytes, void* stream);
size_t oibl_rerank_jaccard_workspace_bytes(int Q, int G);
int oibl_rerank_jaccard(const int32_t* idx, const float* val, const int32_t* cnt, int stride, const int32_t* col_off,
                        const int32_t* inv_row, const float* inv_val, const float* rowmax, int Q, int G,
                        float one_minus_lambda, float lambda, float* dist, size_t ldd, void* ws, size_t ws_bytes,
                        void* stream);

/* ---- k-means centroid initialisation (f4) -------------------------------------------- *
 * examples/cluster.py:110-115 runs scikit-learn's KMeans(num_clusters, max_iter = 100,
 * random_state = seed) on 50 000 L2-normalised conv5 descriptors.  The assignment step of a Lloyd
 * iteration is oibl_sqdist_topk(k = 1) against the centres; this is the update step:
 *   centers[c] <- mean of the rows x[i] with labels[i] == c   (fp64 accumulation in point order,
 *                 correctly rounded fp32 result), untouched when no row carries the label;
 *   counts[c]  <- number of such rows (the caller relocates empty clusters as scikit-learn does).
 *   x [n][d] fp32, labels [n] int32 in [0, num_clusters), centers [num_clusters][d] fp32.          */
int oibl_cluster_means(const float* x, const int32_t* labels, int n, int d, int num_clusters,
                       float* centers, int32_t* counts, void* stream);

/* ---- NetVLAD initialisation without a checkpoint ------------------------------------- *
 * The device pieces around the k-means above (examples/cluster.py:93-104, ibl/models/netvlad.py:34-42).
 *
 * oibl_local_descriptors: the sampled, channel-normalised local descriptors of a batch of conv5 maps.
 *   feat [N][P][C] (NHWC, P = h * w) in `precision` OIBL_BF16 or OIBL_F32; positions [N][S] int32 in [0, P);
 *   out [N*S][C] fp32: row n * S + s = feat[n][positions[n][s]][:] / max(|.|_2, 1e-12)  (F.normalize, then the
 *   gather).  Only the N * S sampled pixels are read.  C % 64 == 0.  The caller guarantees the range of the
 *   positions (they live on the device: the host mirror checks them before the launch); a position outside
 *   [0, P) is not dereferenced, its row is written as NaN.
 *
 * oibl_assign_gap: descs [n][C] fp32, clsts [K][C] fp32 ->
 *   clsts_assign [K][C] = clsts / |clsts|   (row-wise),
 *   gap [n]             = largest minus second largest of the K products <clsts_assign[k], descs[i]>; the top pair
 *                         is chosen by cluster INDEX: two identical centres on top give exactly 0,
 *   *gap_sum (double)   = sum of gap[] in a fixed order that depends on the indices alone.
 *   alpha of NetVLAD._init_params is -ln(0.01) / (*gap_sum / n).  n >= 1, 2 <= K <= 256, C % 64 == 0.  Exact fp32
 *   FMA, no atomics: bit-identical results from run to run.  No [K][n] matrix is formed; the workspace holds one
 *   transposed copy of clsts_assign.  ws 256-byte aligned, gap_sum 8-byte aligned.                             */
int oibl_local_descriptors(const void* feat, int N, int P, int C, int precision, const int32_t* positions, int S,
                           float* out, void* stream);
size_t oibl_assign_gap_workspace_bytes(int n, int K, int C);
int oibl_assign_gap(const float* descs, int n, const float* clsts, int K, int C, float* clsts_assign, float* gap,
                    double* gap_sum, void* ws, size_t ws_bytes, void* stream);

/* n 32-bit words src -> dst, by a kernel (one workgroup) on `stream`: dst may be pinned (host-coherent)
 * memory mapped into the device — how the f16mx range flag reaches the host behind a replayed graph without a
 * DMA-engine copy that would queue behind the next batch's input transfer. */
int oibl_copy_words(const void* src, void* dst, int n, void* stream);

/* ---- diagnostics ------------------------------------------------------------------ */

/* Elapsed milliseconds between two recorded hipEvent_t (HOST pointer ms_host) — also when the events
 * were recorded by event nodes of a replayed hipGraph, which torch's Event.elapsed_time refuses: how
 * bench.py measures the span of the matrix-core launches inside the replayed forward. */
int oibl_event_elapsed_ms(void* ev_start, void* ev_stop, float* ms_host);

/* Plain C = A . B^T on the shared MFMA GEMM core (used by tests to validate the core and
 * its fragment layout independently of the operators above):
 * A [M][K] T, B [N][K] T, C [M][ldc] fp32; K % (128/sizeof(T)) == 0, N % 64 == 0. */
int oibl_gemm_nt(const void* A, int M, const void* B, int N, int K, int precision, float* C,
                 size_t ldc, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* OPENIBL_AMD_H */
