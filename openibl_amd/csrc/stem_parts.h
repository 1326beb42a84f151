// What the persistent stem kernels share (included by stem.hip inside namespace oibl, behind conv_c64.h and
// StemParams): the tile walk and decode, the bias prologue, conv1_1's weight fragments and its six matrix
// instructions, the producers' gathers (float32 rows, uint8 rows), the f16mx half-line write, the consumers' fragment
// addressing and the f16mx pooled epilogue.  vgg_stem_kernel (stem_bf16.h) uses the decode; vgg_stem_x3_kernel
// (stem_x3.h), vgg_stem_mx_kernel (stem_mx16.h) and stem_mx12_kernel (stem_mx12.h) use the rest.
//
// These kernels sit AT their register limits (128 VGPRs with 16 waves, 168 with 12), and several values exist only to
// steer the allocator: the lane id made inside each role (fresh_lane_id), integer LDS addresses, constants
// materialised behind the stages.  Every function here is inlined and takes such values as ARGUMENTS made at the call
// site; none of them computes a lane id or hoists a constant of its own.
constexpr int ST_HALO_PX = 10 * C64_HW;              // 340
constexpr int ST_HALO_BYTES = ST_HALO_PX * 128;      // 43520
constexpr int ST_BLOCKS = (ST_HALO_PX + 31) / 32;    // 11 blocks of 32 halo pixels
constexpr unsigned ST_OOB = 0xF0000000u;
constexpr int S3_W_BYTES = 2 * 9 * 32 * 128;
constexpr int S3_BIAS_OFF = S3_W_BYTES + 2 * ST_HALO_BYTES;   // conv1_1 bias: 64 floats; f16mx: + conv1_2's 64
constexpr int S3_LDS_BYTES = S3_BIAS_OFF + 256 + 256;    // conv1_1's 64 biases + conv1_2's (bf16x3: unused; f16mx: all 64)

typedef __attribute__((ext_vector_type(2))) float f32x2_t;
typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2_t;
typedef __attribute__((ext_vector_type(2))) short i16x2_t;
// two floats -> one dword of two bf16 (lo in bits 0-15): a single v_cvt_pk_bf16_f32
__device__ static inline uint32_t pack_bf16x2(float lo, float hi) {
  const f32x2_t v = {lo, hi};
  return __builtin_bit_cast(uint32_t, __builtin_convertvector(v, bf16x2_t));
}
// ReLU on two packed bf16: as signed 16-bit integers every negative value (sign bit set, -0
// included) is < 0, so max(x, 0) per half is exactly relu — one v_pk_max_i16 for two values, and
// rounding first / clamping second gives the same bits as clamping first.
__device__ static inline uint32_t relu_bf16x2(uint32_t packed) {
  const i16x2_t z = {0, 0};
  return __builtin_bit_cast(uint32_t, __builtin_elementwise_max(__builtin_bit_cast(i16x2_t, packed), z));
}
// two fp32 values -> the dword of their hi parts and the dword of their lo parts (packed bf16 pairs)
__device__ static inline void x3_split_pair(float v0, float v1, uint32_t& hi, uint32_t& lo) {
  hi = pack_bf16x2(v0, v1);
  lo = pack_bf16x2(v0 - __builtin_bit_cast(float, hi << 16), v1 - __builtin_bit_cast(float, hi & 0xffff0000u));
}

// the lane id, recomputed where it is needed (two VALU instructions, never hoisted): at 128 VGPRs the f16mx stem has
// no register to keep `lane >> 5` alive across its loops — the allocator parked it in scratch and reloaded it once
// per tile in front of a vmcnt(0) (round 6, after the b128 tails took three more registers)
__device__ static inline int fresh_lane_id() {
  int l;
  asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(l));
  return l;
}

// ---- tiles ------------------------------------------------------------------------------------------------------------
// The tiles of a workgroup: tile `first + it * stride`, it < niter.  Workgroups are dealt to the 8 XCDs round-robin
// (id % 8), and every XCD has its own L2: with tile = blockIdx.x + it * gridDim.x (rounds 2-5) the four neighbours
// of a tile — whose 10 x 34-pixel halo windows overlap its own by a third — were gathered through four OTHER L2s
// and the kernel fetched 256 MB for a 118 MB input.  Round 6: XCD x owns the contiguous eighth [x T / 8, (x + 1) T / 8)
// of the tile sequence (whole tile rows of whole images) and deals it to its gridDim.x / 8 workgroups.
struct StemTiles {
  int first, stride, niter;
};
__device__ __forceinline__ StemTiles stem_xcd_tiles(int ntiles) {
  int first = blockIdx.x, stride = gridDim.x, tile_end = ntiles;
  if ((gridDim.x & 7) == 0) {
    const int x = blockIdx.x & 7;
    stride = gridDim.x >> 3;
    first = (int)((long)ntiles * x / 8) + (int)(blockIdx.x >> 3);
    tile_end = (int)((long)ntiles * (x + 1) / 8);
  }
  int niter = 0;
  if (first < tile_end) niter = (tile_end - first + stride - 1) / stride;
  return {first, stride, niter};
}
__device__ __forceinline__ void stem_decode(const StemParams& p, int tile, int& n, int& ty, int& tx) {
  const unsigned r2 = (unsigned)tile / (unsigned)p.tiles_x;
  tx = tile - (int)r2 * p.tiles_x;
  n = (int)(r2 / (unsigned)p.tiles_y);
  ty = (int)r2 - n * p.tiles_y;
}
// a tile is interior when every halo pixel and every tap of every halo pixel lies in the image
__device__ __forceinline__ bool stem_is_interior(const StemParams& p, int ty, int tx) {
  return ty >= 1 && ty * 8 + 10 <= p.H && tx >= 1 && tx * 32 + 34 <= p.W;
}
struct StemTile {
  int n, y0, x0;   // image; image coordinates of the halo's origin (-1 at the image's first tile)
  bool interior;
};
__device__ __forceinline__ StemTile stem_tile(const StemParams& p, int tile) {
  int n, ty, tx;
  stem_decode(p, tile, n, ty, tx);
  return {n, ty * 8 - 1, tx * 32 - 1, stem_is_interior(p, ty, tx)};
}
// halo pixel r = 34 hy + hx of a tile (the 12 surplus lanes of block 10 are clamped to the last pixel: they load valid
// data that is never written)
__device__ __forceinline__ void stem_halo_yx(int r, int& hy, int& hx) {
  const int rc = r < ST_HALO_PX ? r : ST_HALO_PX - 1;
  hy = rc / C64_HW;
  hx = rc - hy * C64_HW;
}
// border tiles only: is halo pixel r inside the image?  (Outside, it is conv1_2's zero padding, not a conv1_1 output.)
__device__ __forceinline__ bool stem_halo_pixel_in_image(const StemParams& p, const StemTile& t, int r) {
  bool pix_ok = true;
  if (!t.interior) {
    int hy, hx;
    stem_halo_yx(r, hy, hx);
    const int y = t.y0 + hy, x = t.x0 + hx;
    pix_ok = y >= 0 && y < p.H && x >= 0 && x < p.W;
  }
  return pix_ok;
}

// ---- prologue ---------------------------------------------------------------------------------------------------------
// conv1_1's bias lives in LDS (the producers have no registers to spare for 2 x 16 values per lane); b2 != nullptr
// (f16mx): conv1_2's 64 behind it.  f16mx: conv1_1's weights and both biases carry the activation scale — every
// activation of the kernel, the halo tile in LDS included, is stored scaled (vgg_forward_impl).
__device__ __forceinline__ void stem_bias_to_lds(char* smem, const float* b1, const float* b2, float scale) {
  float* const dst = reinterpret_cast<float*>(smem + S3_BIAS_OFF);
  if (threadIdx.x < 64) dst[threadIdx.x] = b1[threadIdx.x] * scale;
  if (b2 != nullptr && threadIdx.x >= 64 && threadIdx.x < 128) dst[threadIdx.x] = b2[threadIdx.x - 64] * scale;
  __syncthreads();
}
// 16 floats b[stride * j + 0..3], j = 0..3, as four 16-byte LDS reads
template <typename V>
__device__ __forceinline__ void stem_bias16(const float* b, int stride, V& v) {
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const float4 q = *reinterpret_cast<const float4*>(b + stride * j);
    v[4 * j] = q.x;
    v[4 * j + 1] = q.y;
    v[4 * j + 2] = q.z;
    v[4 * j + 3] = q.w;
  }
}
// the roles' issue priorities (StemParams::prod_prio): raise to 1..3 at the head of a role; back from the 3 of a
// conv1_1 to 0..2 (a role at 3 stays there)
__device__ __forceinline__ void stem_raise_prio(int prio) {
  if (prio == 1) __builtin_amdgcn_s_setprio(1);
  else if (prio == 2) __builtin_amdgcn_s_setprio(2);
  else if (prio == 3) __builtin_amdgcn_s_setprio(3);
}
__device__ __forceinline__ void stem_restore_prio(int prio) {
  if (prio == 0) __builtin_amdgcn_s_setprio(0);
  else if (prio == 1) __builtin_amdgcn_s_setprio(1);
  else if (prio == 2) __builtin_amdgcn_s_setprio(2);
}
// f16mx range guard (common.h): the largest group maximum a lane has packed stays in a register (range_seen); the flag —
// a kernel argument and a global store — is touched once, behind the role's loops, whose lgkmcnt / vmcnt waits are
// counted by hand (a scalar argument load inside them was seen to break the counts)
__device__ __forceinline__ void mx_raise_if_out_of_range(float range_seen, unsigned* range_flag) {
  if (__builtin_amdgcn_ballot_w64(range_seen >= 65504.f) != 0) {
    if (range_seen >= 65504.f) mx_raise_range_flag(range_flag);
  }
}

// ---- conv1_1 ----------------------------------------------------------------------------------------------------------
// conv1_1's weights as the A operand, split: w?[h][s] element e <-> accumulator row l31 of channel half h, K slot
// (s, half, e) of the 32.  Which of the 27 window elements (w1 is [c][ky][kx]) a slot carries follows the gather:
//   K_WINDOW  bf16x3, float32 input: element k = 16 s + 8 half + e, (c, ky, kx) order;
//   K_ROWS    f16mx, float32 input: the window travels as ROWS (mx_gather_rows): slot 8 s + e of a lane half is
//             element kx = idx % 3 of its row idx / 3, the lower half owning rows (c, ky) = 0..4, the upper 5..8;
//   K_BYTES   uint8 input: slot 8 s + e of lane half `half` = window byte idx in (ky, kx, c) order.
// Slots beyond the 27 carry zero weights.  LINE_ROWS (f16mx): row 8 g + 4 hp + r carries channel 16 hp + 4 g + r, so
// that a lane owns 16 CONSECUTIVE elements of the pixel's f16mx line (stem_mx16.h).
enum { K_WINDOW, K_ROWS, K_BYTES };
template <int ORDER, bool LINE_ROWS>
__device__ __forceinline__ void stem_w1_fragments(const float* w1, float scale, int half, int l31,
                                                  bf16x8_t (&wh)[2][2], bf16x8_t (&wlo)[2][2]) {
#pragma unroll
  for (int s = 0; s < 2; ++s)
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      int k = 16 * s + 8 * half + e;
      if (ORDER == K_ROWS) {
        const int idx = 8 * s + e;
        k = idx < (half ? 12 : 15) ? (idx / 3 + (half ? 5 : 0)) * 3 + idx % 3 : 27;
      }
      if (ORDER == K_BYTES) {
        const int idx = 16 * half + 8 * s + e;
        k = idx < 27 ? (idx % 3) * 9 + (idx / 9) * 3 + (idx % 9) / 3 : 27;
      }
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const int ch = LINE_ROWS ? 16 * ((l31 >> 2) & 1) + 4 * (l31 >> 3) + (l31 & 3) : l31;   // channel of row l31
        const float v = k < 27 ? w1[(32 * h + ch) * 27 + k] * scale : 0.f;
        uint16_t hi, lo;
        x3_split(v, hi, lo);
        wh[h][s][e] = (short)hi;
        wlo[h][s][e] = (short)lo;
      }
    }
}
// the gathered window as (hi, lo) B fragments
__device__ __forceinline__ void x3_split_window(const float (&xv)[16], bf16x8_t (&xh)[2], bf16x8_t (&xl)[2]) {
  typedef __attribute__((ext_vector_type(4))) uint32_t u32x4_t;
#pragma unroll
  for (int s = 0; s < 2; ++s) {
    u32x4_t hi4, lo4;
#pragma unroll
    for (int e2 = 0; e2 < 4; ++e2) {
      uint32_t hi, lo;
      x3_split_pair(xv[8 * s + 2 * e2], xv[8 * s + 2 * e2 + 1], hi, lo);
      hi4[e2] = hi;
      lo4[e2] = lo;
    }
    xh[s] = __builtin_bit_cast(bf16x8_t, hi4);
    xl[s] = __builtin_bit_cast(bf16x8_t, lo4);
  }
}
// conv1_1 of one channel half on one block: K = 27 padded to 32, lo.hi + hi.lo + hi.hi per k-step — the order of
// conv1_1_mfma_kernel<X3> — at issue priority 3 (the caller restores its own)
__device__ __forceinline__ f32x16_t conv1_1_sextet(const bf16x8_t (&wh)[2], const bf16x8_t (&wlo)[2], bf16x8_t xh0,
                                                   bf16x8_t xh1, bf16x8_t xl0, bf16x8_t xl1, f32x16_t acc) {
  __builtin_amdgcn_s_setprio(3);
  acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wlo[0], xh0, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wh[0], xl0, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wh[0], xh0, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wlo[1], xh1, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wh[1], xl1, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wh[1], xh1, acc, 0, 0, 0);
  return acc;
}

// ---- float32 input, f16mx: the window as rows ---------------------------------------------------------------------------
// The 3 x 3 x 3 window of halo pixel `row` as nine ROWS (c, ky) of three consecutive pixels x - 1 .. x + 1: five 12-byte
// loads per lane (the lower lane half rows 0-4, the upper half rows 5-8 and row 8 once more under zero weights)
// instead of sixteen 4-byte ones — the sixteen were ~3k cycles of the texture path per tile.  Image edges: a row above /
// below the image is fetched from the out-of-range offset (zeros); at x = 0 the fetch starts at x, at x = W - 1 at
// x - 2 (no byte outside the tensor is ever touched) and mx_edge_fix moves the elements into place.
// g_rel = hy * W + hx of the pixel, hsel = the lane half.  Returns xfix: 1 = the rows were fetched from x (not x - 1),
// 2 = from x - 2, 0 = in place.  Nothing waits here.
__device__ __forceinline__ int mx_gather_rows(const __amdgpu_buffer_rsrc_t rs_x, const StemParams& p, const StemTile& t,
                                              int row, int g_rel, int hsel, float (&xv)[16]) {
  const int plane = p.H * p.W;
  const int origin = ((t.n * 3) * p.H + t.y0) * p.W + t.x0;
  bool in = true, ya = true, yc = true;
  int shift = -1, xfix = 0;
  if (!t.interior) {
    int hy, hx;
    stem_halo_yx(row, hy, hx);
    const int y = t.y0 + hy, x = t.x0 + hx;
    in = y >= 0 && y < p.H && x >= 0 && x < p.W;
    ya = y > 0;
    yc = y + 1 < p.H;
    xfix = !in ? 0 : x == 0 ? 1 : x + 1 >= p.W ? 2 : 0;
    shift = xfix == 1 ? 0 : xfix == 2 ? -2 : -1;
  }
  const int base = origin + g_rel + shift;
#pragma unroll
  for (int i = 0; i < 5; ++i) {
    const int rA = i, rB = i + 5 < 9 ? i + 5 : 8;
    const int oA = (rA / 3) * plane + (rA % 3 - 1) * p.W, oB = (rB / 3) * plane + (rB % 3 - 1) * p.W;
    const int kyA = rA % 3, kyB = rB % 3;
    unsigned off = (unsigned)(base + (hsel ? oB : oA)) * 4u;
    if (!t.interior) {
      const int ky = hsel ? kyB : kyA;
      const bool ok = in && (ky == 0 ? ya : ky == 2 ? yc : true);
      off = ok ? off : ST_OOB;
    }
    // (elements through scalars: __builtin_bit_cast applied to a vector-element lvalue reads element 0)
    const auto d = __builtin_amdgcn_raw_buffer_load_b96(rs_x, (int)off, 0, 0);
    const unsigned d0 = d[0], d1 = d[1], d2 = d[2];
    xv[3 * i] = __builtin_bit_cast(float, d0);
    xv[3 * i + 1] = __builtin_bit_cast(float, d1);
    xv[3 * i + 2] = __builtin_bit_cast(float, d2);
  }
  xv[15] = 0.f;
  return xfix;
}
__device__ __forceinline__ void mx_edge_fix(float (&xv)[16], int xfix) {
  if (__builtin_amdgcn_ballot_w64(xfix != 0) != 0) {   // an image edge inside this block (rare)
    const bool left = xfix == 1, right = xfix == 2;
#pragma unroll
    for (int i = 0; i < 5; ++i) {
      const float a = xv[3 * i], b = xv[3 * i + 1], c = xv[3 * i + 2];
      xv[3 * i] = left ? 0.f : right ? b : a;
      xv[3 * i + 1] = left ? a : right ? c : b;
      xv[3 * i + 2] = left ? b : right ? 0.f : c;
    }
  }
}

// ---- uint8 input (bf16x3 and f16mx alike; only the row order of conv1_1's weights differs) ------------------------------
// The input is the loader's raw uint8 NHWC image (StemParams::x [N][H][W][3]).  The producers gather a pixel's
// 3 x 3 x 3 window as THREE 12-byte loads (one per window row: 9 consecutive bytes = 3 pixels x RGB, fetched from the
// enclosing aligned dwords and shifted into place), the K slots of conv1_1 then follow the bytes — (ky, kx, c) order,
// the lower lane half the first 16 of the 27, the upper half the rest (K_BYTES) — and ToTensor + Normalize become ONE
// fma per value: v = u * a_c + b_c with a_c = 1 / (255 std_c), b_c = -mean_c / std_c (StemParams::mean = a, ::stdv =
// b, rounded from double on the host).  That is NOT the loader's three rounded operations (u / 255 - mean) / std, but
// within 2^-16 of them on values up to 151 — the rounding the loader's own intermediate carries (u / 255 - mean is
// rounded at magnitude <= 1, then scaled by 255); over all 768 (channel, byte) pairs the bf16 hi parts conv1_1
// multiplies are identical and 42 lo parts differ by one unit (tests/test_stem_u8_cpu.py, exhaustive) — far inside the
// arithmetic's own error.  (The exact route, a 3 x 257 table of split values as in the bf16 stem, needs 3 KB of LDS:
// these kernels have 1.6 KB left; three exactly rounded operations per value are ~110 more VALU instructions per tile
// and lane on the role that is already issue-bound.)  Out-of-image taps are zeroed AFTER the normalisation (conv1_1
// pads the normalised tensor), from a 27-bit validity mask per lane, on border tiles only.
struct U8Window {
  unsigned xr[3][3];   // the three window rows as fetched (aligned dwords)
  unsigned xsh;        // the byte shift of row 0
  unsigned xmask;      // border tiles: bit ky * 9 + kx * 3 + c = the tap is inside the image
  bool border;         // the tile in flight is a border tile (wave-uniform)
};
// per-lane Normalize constants in slot order: slot s of this lane half is channel (s + half) % 3
__device__ __forceinline__ void u8_lane_constants(const StemParams& p, int half, float (&ka)[3], float (&kb)[3]) {
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    ka[i] = half ? p.mean[(i + 1) % 3] : p.mean[i];
    kb[i] = half ? p.stdv[(i + 1) % 3] : p.stdv[i];
  }
}
// g_rel = hy * W + hx of halo pixel `row`.  Nothing waits here.
__device__ __forceinline__ void u8_gather_rows(const __amdgpu_buffer_rsrc_t rs_x, const StemParams& p, const StemTile& t,
                                               int row, int g_rel, U8Window& w) {
  // byte offset of the window's first byte: pixel (y - 1, x - 1), channel 0 (negative at the image's
  // first pixels: the unsigned offset is then out of range and the load returns zeros)
  const int b0 = ((t.n * p.H + t.y0) * p.W + t.x0 + g_rel - p.W - 1) * 3;
  w.xsh = (unsigned)b0 & 3u;
  bool in = true, ya = true, yc = true;
  if (!t.interior) {
    int hy, hx;
    stem_halo_yx(row, hy, hx);
    const int y = t.y0 + hy, x = t.x0 + hx;
    in = y >= 0 && y < p.H && x >= 0 && x < p.W;
    ya = y > 0;
    yc = y + 1 < p.H;
    const bool xa = x > 0, xc = x + 1 < p.W;
    const unsigned rows = (ya ? 0x1ffu : 0u) | 0x3fe00u | (yc ? 0x7fc0000u : 0u);
    const unsigned cols = (xa ? 0x0040201u * 7u : 0u) | (0x0040201u * 7u << 3) | (xc ? 0x0040201u * 7u << 6 : 0u);
    w.xmask = in ? rows & cols : 0u;
  }
#pragma unroll
  for (int ky = 0; ky < 3; ++ky) {
    const int offs = (b0 + ky * 3 * p.W) & ~3;
    unsigned off = (unsigned)offs;
    bool early = false;   // the tensor's very first pixel: its row starts 3 bytes before the tensor
    if (!t.interior) {
      const bool ok = in && (ky == 0 ? ya : ky == 2 ? yc : true);
      early = ok && offs < 0;
      off = !ok ? ST_OOB : early ? 0u : off;
    }
    const auto d = __builtin_amdgcn_raw_buffer_load_b96(rs_x, (int)off, 0, 0);
    const unsigned d0 = d[0], d1 = d[1], d2 = d[2];   // (elements through scalars: see mx_gather_rows)
    w.xr[ky][0] = early ? 0u : d0;          // (fetched from 0: one dword late)
    w.xr[ky][1] = early ? d0 : d1;
    w.xr[ky][2] = early ? d1 : d2;
  }
}
// the fetched rows -> the 16 normalised values of this lane half (hsel), taps outside the image zeroed
__device__ __forceinline__ void u8_convert(const StemParams& p, const U8Window& win, const float (&ka)[3],
                                           const float (&kb)[3], int hsel, float (&xv)[16]) {
  // each row's 9 window bytes shifted into place: w[ky][0..1] = bytes 0-7, w[ky][2] byte 0 = byte 8
  const unsigned w3 = (unsigned)(3 * p.W) & 3u;
  unsigned w[3][3];
#pragma unroll
  for (int ky = 0; ky < 3; ++ky) {
    const unsigned sh = (win.xsh + ky * w3) & 3u;
    w[ky][0] = __builtin_amdgcn_alignbyte(win.xr[ky][1], win.xr[ky][0], sh);
    w[ky][1] = __builtin_amdgcn_alignbyte(win.xr[ky][2], win.xr[ky][1], sh);
    w[ky][2] = win.xr[ky][2] >> (8u * sh);
  }
  // the 16 bytes of this lane half: lower = row 0 bytes 0-8, row 1 bytes 0-6; upper = row 1 bytes 7-8,
  // row 2 bytes 0-8, five slots under zero weights (any finite value)
  const unsigned a2 = __builtin_amdgcn_perm(w[1][0], w[0][2], 0x06050400u);
  const unsigned a3 = __builtin_amdgcn_alignbyte(w[1][1], w[1][0], 3u);
  const unsigned t = __builtin_amdgcn_perm(w[1][2], w[1][1], 0x00000403u);
  const unsigned b0 = __builtin_amdgcn_perm(w[2][0], t, 0x05040100u);
  const unsigned b1 = __builtin_amdgcn_alignbyte(w[2][1], w[2][0], 2u);
  const unsigned b2 = __builtin_amdgcn_alignbyte(w[2][2], w[2][1], 2u) & 0x00ffffffu;
  const unsigned dw[4] = {hsel ? b0 : w[0][0], hsel ? b1 : w[0][1], hsel ? b2 : a2, hsel ? 0u : a3};
#pragma unroll
  for (int j = 0; j < 16; ++j) {
    const float u = (float)((dw[j >> 2] >> (8 * (j & 3))) & 0xffu);   // v_cvt_f32_ubyteN
    xv[j] = fmaf(u, ka[j % 3], kb[j % 3]);
  }
  if (win.border) {   // wave-uniform: zero the taps outside the image (conv1_1 pads the NORMALISED tensor)
    const unsigned mk = win.xmask >> (hsel ? 16 : 0);
#pragma unroll
    for (int j = 0; j < 16; ++j) xv[j] = ((mk >> j) & 1u) ? xv[j] : 0.f;
  }
}

// ---- f16mx producers: a pixel's half line ---------------------------------------------------------------------------------
struct MxHalfLine {
  unsigned h16[8], h6[3], l6[3], bh, bl;   // 16 fp16, the e2m3 images of hi and lo (3 dwords each), their scale bytes
};
// conv1_1's 16 channels of this lane -> the packed half line: ReLU, the fp16 bound and conv1_2's zero padding (a halo
// pixel outside the image) in ONE v_med3, then mx_pack_half (one cross-lane maximum)
__device__ __forceinline__ void mx_clamp_pack_half(const f32x16_t& acc, bool pix_ok, MxHalfLine& L, float& range_seen) {
  float c[16];
  const float lim = pix_ok ? 65504.f : 0.f;
#pragma unroll
  for (int j = 0; j < 16; ++j) c[j] = __builtin_amdgcn_fmed3f(acc[j], 0.f, lim);
  mx_pack_half<false>(c, L.h16, L.h6, L.l6, L.bh, L.bl, range_seen);
}
// this lane's 16 consecutive elements of the pixel's line at `row` (slot swizzle sw): fp16 parts = 16-B slots 2 half,
// 2 half + 1; e2m3 images = dwords 3 half .. 3 half + 2 of the 6-dword strings, which the line keeps as
// slot 4 / 5 (hi / lo: dwords 0-3) and slot 6 / 7 (dwords 4, 5, zero, scale byte)
__device__ __forceinline__ void mx_write_half_line(char* row, int sw, int half, const MxHalfLine& L) {
  typedef __attribute__((ext_vector_type(4))) unsigned u4;
  typedef __attribute__((ext_vector_type(3))) unsigned u3;
  *reinterpret_cast<u4*>(row + (((2 * half) ^ sw) << 4)) = (u4){L.h16[0], L.h16[1], L.h16[2], L.h16[3]};
  *reinterpret_cast<u4*>(row + (((2 * half + 1) ^ sw) << 4)) = (u4){L.h16[4], L.h16[5], L.h16[6], L.h16[7]};
  if (half == 0) {
    *reinterpret_cast<u3*>(row + ((4 ^ sw) << 4)) = (u3){L.h6[0], L.h6[1], L.h6[2]};
    *reinterpret_cast<u3*>(row + ((5 ^ sw) << 4)) = (u3){L.l6[0], L.l6[1], L.l6[2]};
  } else {
    *reinterpret_cast<unsigned*>(row + ((4 ^ sw) << 4) + 12) = L.h6[0];
    *reinterpret_cast<unsigned*>(row + ((5 ^ sw) << 4) + 12) = L.l6[0];
    *reinterpret_cast<u4*>(row + ((6 ^ sw) << 4)) = (u4){L.h6[1], L.h6[2], 0u, L.bh};
    *reinterpret_cast<u4*>(row + ((7 ^ sw) << 4)) = (u4){L.l6[1], L.l6[2], 0u, L.bl};
  }
}
// Which halo pixel of its 32-pixel block a producer lane computes is free.  f16mx: lanes 0-7 of a block take its EVEN
// pixels 0, 2, .., 14, lanes 8-15 the odd ones (and so on for pixels 16-31).  A line write is serviced in contiguous
// 8-lane groups over 32 banks, and the slot swizzle ((hx >> 1) & 7) gives two neighbouring pixels the same slot: with
// lane = pixel every 16-byte write of a line was a 2-way conflict (884 extra LDS cycles per tile,
// tools/lds_stem_model.py — with the consumers' tail reads the 2.0e8 SQ_LDS_BANK_CONFLICT cycles per launch of
// profiles/r05_z_pmc.md: 2604 per tile measured, 2612 modelled).
__device__ __forceinline__ int mx_lane_pixel(int l31) { return 2 * (l31 & 7) + ((l31 >> 3) & 1) + 16 * (l31 >> 4); }

// ---- consumers ----------------------------------------------------------------------------------------------------------
// Pixel-fragment addressing of the 4-byte stems' consumers.  Block i's pixel of this lane is (ly, lx) of the 8 x 32
// tile; tap (ky, kx) reads halo pixel (ly + ky, lx + kx): its row is a compile-time distance (ky * 34 + kx) * 128 from
// the lane's own, and its 16-B slot (2 pr + half) ^ swz(hy, hx) differs from the tap-(0,0) slot only
// by   (lx + kx) >> 1 = (lx >> 1) + {0, lx & 1, 1}[kx]   and the constant bits pr << 1, (ky & 1) << 2.
// Block 1's pixel is 16 columns right of block 0's: the same slot ((lx >> 1) & 7 repeats every 16
// columns) 2048 bytes on.  So three per-lane slot offsets (kx = 0, 1, 2), one pixel offset and ONE
// v_xad_u32 per pair of reads replace ~12 VALU instructions per read (hoisted, the 18 x 2 x 2
// addresses would cost ~70 of a kernel's 128 VGPRs): a read's address is (e_kx[kx] ^ const) + pxb + the buffer.
__device__ __forceinline__ void stem_pixel_addressing(int wave, int half, int l31, int (&e_kx)[3], int& pxb) {
  const int ly = 2 * wave + ((l31 >> 1) & 1);
  const int lx = 2 * (l31 >> 2) + (l31 & 1);
  const int fix = half ^ ((ly & 1) << 2);
  e_kx[0] = (fix ^ ((lx >> 1) & 7)) << 4;
  e_kx[2] = (fix ^ (((lx >> 1) + 1) & 7)) << 4;
  e_kx[1] = (lx & 1) ? e_kx[2] : e_kx[0];
  pxb = (ly * C64_HW + lx) * 128;
}
// f16mx: the weight row of this lane; slot 2 kk + half of its line = base ^ (kk << 5) (the slot bits XOR; ONE register
// for the four fragment addresses: the b128 tails cost three registers the 128-VGPR kernel did not have)
__device__ __forceinline__ int mx_weight_row(int half, int l31) { return l31 * 128 + ((half ^ ((l31 >> 1) & 7)) << 4); }
// f16mx: the e2m3 x e2m3 matrix instruction (cbsz = blgp = 2): registers 0-5 of either operand; its scale: byte 0 of
// register 7 = the tail slot's last dword [d4 d5 0 scale].  The operand's tail — e2m3 dwords 4, 5, a zero dword, the
// scale byte: one 16-byte slot of the line — is read as ONE ds_read_b128.  As ds_read_b64 + ds_read_b32 (the form the
// ring kernels keep, whose loop is not bound by LDS cycles) the 32 lanes of a b64 group reach 16 of their 32 bank pairs
// and the 32 scale dwords sit on 8 banks: 12 LDS cycles per tail instead of 4, 1728 extra cycles per tile on the one
// role whose passes ARE the LDS port's time (4 waves x 48 cycles x 18 taps = the 3456 matrix-pipe cycles of a SIMD:
// tools/lds_stem_model.py).
typedef __attribute__((ext_vector_type(4))) unsigned stem_u4;
__device__ __forceinline__ f32x16_t mx_scaled_mfma(stem_u4 wa, stem_u4 wt, stem_u4 ba, stem_u4 bt, f32x16_t acc) {
  typedef __attribute__((ext_vector_type(4))) int i4;
  const i32x8_t a8 = __builtin_shufflevector(__builtin_bit_cast(i4, wa), __builtin_bit_cast(i4, wt), 0, 1, 2, 3, 4, 5, 6, 7);
  const i32x8_t b8 = __builtin_shufflevector(__builtin_bit_cast(i4, ba), __builtin_bit_cast(i4, bt), 0, 1, 2, 3, 4, 5, 6, 7);
  return __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a8, b8, acc, 2, 2, 0, a8[7], 0, b8[7]);
}
// f16mx, one output-channel half cz of a tile: 2x2 max-pool (the window = the lane quad: two DPP steps), bias, ReLU,
// the fp16 bound, pack, store.  a0 / a1 = the accumulators of pixel blocks 0 / 1; lane quad q of block i is pooled
// pixel (wave, 8 i + q) of the tile's 4 x 16.  rs_o = ONE OUTPUT ROW of the map as the buffer: a pixel right of the map,
// a row below it (zero records) and the three non-leader lanes of a quad (offset 2^31) are dropped by the hardware —
// no branch.  bias2 = this lane's 16 scaled conv1_2 biases in LDS; f16max (65504) and zero are the caller's, so that a
// kernel can materialise them where it has the registers.
__device__ __forceinline__ void mx_pooled_epilogue(const f32x16_t& a0, const f32x16_t& a1, const float* bias2, float f16max,
                                                   unsigned zero, const __amdgpu_buffer_rsrc_t rs_o, int tx, int cz,
                                                   int half, int l31, float& range_seen) {
  typedef __attribute__((ext_vector_type(4))) unsigned u4;
  typedef __attribute__((ext_vector_type(2))) unsigned u2;
  float bv[16];
  stem_bias16(bias2, 4, bv);
  // pooling: the window's x pair first (lane ^ 1), then the two blocks merge — even lanes keep block 0,
  // odd lanes block 1 — and the y pair (lane ^ 2) follows on the merged values: ONE line per lane pair
  // (v_max_f32_dpp by hand: through fmaxf + mov_dpp every step is a v_mov_dpp, a v_max and two
  //  canonicalising v_max x, x — 176 instructions instead of 48.  A DPP read needs two wait states behind
  //  the VALU write of its source, which the compiler does not see inside asm: the first round reads
  //  accumulators written long ago, the second carries its own s_nop.)
  float v[16], m0[16], m1[16];
  const bool odd = l31 & 1;
#pragma unroll
  for (int j = 0; j < 16; ++j) {
    asm volatile("v_max_f32_dpp %0, %1, %1 quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf" : "=v"(m0[j]) : "v"(a0[j]));
    asm volatile("v_max_f32_dpp %0, %1, %1 quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf" : "=v"(m1[j]) : "v"(a1[j]));
  }
#pragma unroll
  for (int j = 0; j < 16; ++j) v[j] = odd ? m1[j] : m0[j];
#pragma unroll
  for (int j = 0; j < 16; ++j)   // (s_nop: the select above may be scheduled right in front of its reader)
    asm volatile("s_nop 1\n\tv_max_f32_dpp %0, %1, %1 quad_perm:[2,3,0,1] row_mask:0xf bank_mask:0xf" : "=v"(m0[j]) : "v"(v[j]));
#pragma unroll
  for (int j = 0; j < 16; ++j) v[j] = __builtin_amdgcn_fmed3f(m0[j] + bv[j], 0.f, f16max);   // bias, ReLU, the fp16 bound
  unsigned h16[8], h6[3], l6[3], bh, bl;
  mx_pack_half<false>(v, h16, h6, l6, bh, bl, range_seen);
  // lanes 0, 1 of a quad store: pooled pixel 8 (l31 & 1) + (l31 >> 2) of the tile row
  const unsigned off = (l31 & 2) ? 0x80000000u
                                 : (unsigned)(tx * 16 + 8 * (l31 & 1) + (l31 >> 2)) * 256u + (unsigned)cz * 128u;
  __builtin_amdgcn_raw_buffer_store_b128((u4){h16[0], h16[1], h16[2], h16[3]}, rs_o, (int)(off + 32 * half), 0, 0);
  __builtin_amdgcn_raw_buffer_store_b128((u4){h16[4], h16[5], h16[6], h16[7]}, rs_o, (int)(off + 32 * half + 16), 0, 0);
  // e2m3 strings: this lane's dwords 3 half .. 3 half + 2; dwords 0-3 in slot 4 / 5, dwords 4, 5 in slot 6 / 7
  const unsigned oa = off + (half ? 76u : 64u), ob = off + (half ? 96u : 68u);
  __builtin_amdgcn_raw_buffer_store_b32(h6[0], rs_o, (int)oa, 0, 0);
  __builtin_amdgcn_raw_buffer_store_b64((u2){h6[1], h6[2]}, rs_o, (int)ob, 0, 0);
  __builtin_amdgcn_raw_buffer_store_b32(l6[0], rs_o, (int)(oa + 16), 0, 0);
  __builtin_amdgcn_raw_buffer_store_b64((u2){l6[1], l6[2]}, rs_o, (int)(ob + 16), 0, 0);
  const unsigned ot = half ? off + 104u : 0x80000000u;   // the tails' zero dword + scale byte
  __builtin_amdgcn_raw_buffer_store_b64((u2){zero, bh}, rs_o, (int)ot, 0, 0);
  __builtin_amdgcn_raw_buffer_store_b64((u2){zero, bl}, rs_o, (int)(ot + 16), 0, 0);
}
