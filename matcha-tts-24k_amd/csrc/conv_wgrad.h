// The Conv1d(k5, pad 2) weight gradient as its users see it (style_grad.hip, where the kernels live, and dp_grad.hip): the chunk scheme
// of the reduction over the B T rows -- a function of the shape alone, never of the device -- and the launcher.  The scheme is also the
// one the other parameter reductions of dp_grad.hip follow: chunks of conv_wgrad_chunk_rows(M) rows, each chunk a stated order of its
// own, the chunks added in chunk order by a second kernel.
#pragma once
#include "host.h"

#include <algorithm>

namespace mtts {

constexpr int WG_TAPS = 5;
constexpr int WG_CHUNK_UNIT = 256;   // chunk lengths are multiples of this
constexpr int WG_MAX_CHUNKS = 16;

// Rows per chunk of the reduction over M = B T rows: 256 up to 4096 rows, then the multiple of 256 that keeps the chunks at 16 or fewer.
static inline int conv_wgrad_chunk_rows(int64_t M) {
    const int64_t per = (M + (int64_t)WG_CHUNK_UNIT * WG_MAX_CHUNKS - 1) / ((int64_t)WG_CHUNK_UNIT * WG_MAX_CHUNKS);
    return (int)(WG_CHUNK_UNIT * std::max<int64_t>(per, 1));
}
static inline int conv_wgrad_chunks(int64_t M) {
    const int ch = conv_wgrad_chunk_rows(M);
    return (int)((M + ch - 1) / ch);
}
// floats of partial results: [chunks][5][cout][cin] then [chunks][cout]
static inline size_t conv_wgrad_partial_floats(int64_t M, int cin, int cout) {
    return (size_t)conv_wgrad_chunks(M) * ((size_t)WG_TAPS * cout * cin + cout);
}

// The whole weight (and bias) gradient of one Conv1d(k5, pad 2): three launches.  dz [B T][ldz] the gradient at the convolution's output,
// x [B T][ldx] its input rows, lengths int64 [B] or null; dw [cout][cin][5] (torch layout), db [cout] or null; part:
// conv_wgrad_partial_floats floats.
hipError_t launch_conv_wgrad(const float* dz, int ldz, const float* x, int ldx, const int64_t* lengths, int B, int T, int cin, int cout,
                             float* dw, float* db, float* part, hipStream_t s);
static inline double conv_wgrad_flops(int B, int T, int cin, int cout) { return 2.0 * B * T * (double)cin * cout * WG_TAPS; }

}  // namespace mtts
