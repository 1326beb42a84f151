// The two kernels of csrc/jpeg.hip that follow the entropy stage, declared for csrc/jpeg_chunked.hip, which launches
// them behind an entropy stage of its own.  jpeg.hip defines them and says what they do.
#pragma once

#include "common.h"

namespace oibl {

// grid (ceil(Bw * Bh / 256), 3, N), 256 threads
__global__ __launch_bounds__(256) void jpeg_idct_kernel(const uint8_t* records, const int16_t* coef, int H, int W,
                                                        uint8_t* planes);

// grid (ceil(W / 64), ceil(H / 4), N), (64, 4) threads
__global__ __launch_bounds__(256) void jpeg_colour_kernel(const uint8_t* records, const uint8_t* planes,
                                                          const int32_t* seg_status, int S, int H, int W,
                                                          uint8_t* out, int32_t* status);

}  // namespace oibl
