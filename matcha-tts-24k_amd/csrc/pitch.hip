// Pitch for a ragged batch (gfx950): F0 contours by YIN (de Cheveigne & Kawahara 2002) cut into blocks, and exact order
// statistics of a contour -- include/mtts.h "pitch" is the contract, every order of summation included.  Three launches:
//   1. pitch_block_kernel  (tile of PITCH_TILE blocks, clip): the block sums s_b(tau) = sum_j (x[bH+j] - x[bH+j+tau])^2 for
//                          tau = 1 .. tau_max, each computed ONCE and used by the eight frames that contain block b.  A workgroup
//                          stages its tile's samples in LDS once; a wave owns a block, a lane PITCH_R = 7 consecutive lags, so
//                          x[bH+j] is one broadcast read and the window x[bH+j+tau0 .. +6] slides through registers with one new
//                          read per j: 2 ds_read_b32 per 7 subtract-multiply-adds.  Lane l reads dword 7 l + const: a stride that
//                          is odd, so the 32 lanes of a read group fall on 32 different banks.
//   2. pitch_frame_kernel  (8 frames, clip): a wave owns a frame, a lane 16 consecutive lags: the eight-block sum, the cumulative
//                          mean normalisation (16 sequential adds per lane, a Hillis-Steele scan over the lanes), the walk and the
//                          parabola.
//   3. pitch_stats_kernel  (clip): order statistics of the voiced f0 values by radix select on their bit patterns (positive floats
//                          order like their bits; loudness.hip's loud_r128_kernel has the pattern), four ranks per pass.
// and, for pitch per token (include/mtts.h "prosody"):
//   4. pitch_cand_kernel   (8 frames, clip): in place of 2, after the same block sums: up to 8 record-setting dips of d' per frame
//                          with a probability mass each; pitch_dprime is the d' code the two share.
//   5. pitch_viterbi_kernel (clip): one shortest path through the candidates, one wavefront per clip.
//   6. pitch_fold_kernel   (4 tokens, clip): a contour folded onto token marks, a wave per token.
// No atomics on results (LDS histograms of integers only); a clip's numbers do not depend on its batch or its place in it.
// Lengths are read on the device only; nothing is read outside [0, len_b) of a row.
#include "host.h"
#include "device_utils.h"

#include <algorithm>
#include <cfloat>
#include <climits>

namespace mtts {

using f32x4 = __attribute__((ext_vector_type(4))) float;

constexpr int PITCH_TILE = 8;                  // blocks per workgroup of the block sums (mtts_pitch_tile)
constexpr int PITCH_R = 7;                     // consecutive lags per lane: odd, see above
constexpr int PITCH_MAX_HOP = 512;
constexpr int PITCH_FRAMES_PER_WG = 8;         // 4 waves x 2 frames
constexpr int PITCH_LDS = PITCH_TILE * PITCH_MAX_HOP + MTTS_PITCH_MAX_LAG + 8;     // staged samples + the window's overhang
static_assert(MTTS_PITCH_MAX_LAG == 1024, "a lane of the frame kernel owns 16 lags: 64 x 16");

struct PitchArgs {
    const float* audio = nullptr;      // [B][ld]
    int64_t ld = 0;
    const int64_t* lengths = nullptr;  // [B]
    int B = 0;
    int H = 0, tmin = 0, tmax = 0;     // hop, smallest and largest lag
    int ldt = 0;                       // tmax rounded up to 4: floats per block of S
    int64_t nblk_max = 0;              // blocks per row of S
    float thr = 0.f, fs = 0.f;
    float* f0 = nullptr;               // [B][ld_frames]
    float* aper = nullptr;             // [B][ld_frames]
    int64_t ld_frames = 0;
    int64_t* frames = nullptr;         // [B]
    int64_t* status = nullptr;         // the workspace's header
    float* S = nullptr;                // [B][nblk_max][ldt]: s_b(tau) at tau - 1
    int32_t* flag = nullptr;           // [B][nblk_max]: a non-finite sample among the block's H + tmax
};

struct PitchStatsArgs {
    const float* f0 = nullptr;         // [B][ld_frames]
    int64_t ld_frames = 0;
    const int64_t* frames = nullptr;   // [B]
    int B = 0;
    int64_t tail = 0;
    float* out = nullptr;              // [B][4]: p05, median, p95, tail median
    int64_t* counts = nullptr;         // [B][3]: frames, voiced, voiced in the tail
    int64_t* status = nullptr;
};

__host__ __device__ __forceinline__ int64_t pitch_frames(int64_t L, int H, int tmax) {
    const int64_t need = 8 * (int64_t)H + tmax;
    return L < need ? 0 : (L - need) / H + 1;
}

template <class Refused>
__device__ __forceinline__ void pitch_verdict(int B, const int64_t* values, int64_t* status, int64_t bound, int64_t entry, Refused refused) {
    const int i = first_refused_row(B, refused);
    if (threadIdx.x == 0) {
        status[0] = i < B ? i + 1 : 0;
        status[1] = i < B ? values[i] : 0;
        status[2] = bound;
        status[3] = 0;
        status[4] = entry;
    }
}

// ------------------------------------------------------------------------------------------------ block sums
__global__ __launch_bounds__(256) void pitch_block_kernel(const PitchArgs p) {
    __shared__ float xs[PITCH_LDS];
    const int row = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int H = p.H, tmax = p.tmax;
    const int64_t L = p.lengths[row];
    if (L < 0 || L > p.ld) return;
    const int64_t n = pitch_frames(L, H, tmax);
    const int64_t nblk = n > 0 ? n + 7 : 0;                       // the last frame ends with block n + 6
    const int64_t b0 = (int64_t)blockIdx.x * PITCH_TILE;
    if (b0 >= nblk) return;                                       // (workgroup-uniform)
    const int nb = (int)min((int64_t)PITCH_TILE, nblk - b0);
    // samples [b0 H, b0 H + count) are inside the clip: (b0 + nb) H + tmax <= (n + 7) H + tmax = (n - 1) H + 8 H + tmax <= L
    const int count = nb * H + tmax;
    const float* src = p.audio + (size_t)row * p.ld + b0 * H;
    for (int i = tid; i < count + PITCH_R; i += 256) xs[i] = i < count ? src[i] : 0.f;
    __syncthreads();
    for (int bl = wave; bl < nb; bl += 4) {
        const float* xb = xs + bl * H;
        bool bad = false;
        for (int i = lane; i < H + tmax; i += 64) bad |= !(fabsf(xb[i]) <= FLT_MAX);
        const bool any_bad = __any(bad);
        const size_t at = (size_t)row * p.nblk_max + b0 + bl;
        float* out = p.S + at * p.ldt;
        for (int t0 = 1 + PITCH_R * lane; t0 <= tmax; t0 += 64 * PITCH_R) {
            // lags t0 .. t0 + 6 (those <= tmax are stored); the largest index read is bl H + H - 1 + t0 + 6 < count + PITCH_R
            const float* y = xb + t0;
            float acc[PITCH_R], w[PITCH_R];
#pragma unroll
            for (int k = 0; k < PITCH_R; ++k) acc[k] = 0.f;
#pragma unroll
            for (int k = 0; k < PITCH_R - 1; ++k) w[k] = y[k];
            for (int j = 0; j < H; j += PITCH_R) {
#pragma unroll
                for (int jj = 0; jj < PITCH_R; ++jj) {
                    if (j + jj < H) {                             // (uniform)
                        const float xj = xb[j + jj];
                        w[(jj + PITCH_R - 1) % PITCH_R] = y[j + jj + PITCH_R - 1];      // ring: w[(jj + k) % R] = y[j + jj + k]
#pragma unroll
                        for (int k = 0; k < PITCH_R; ++k) {
                            const float d = xj - w[(jj + k) % PITCH_R];
                            acc[k] = acc[k] + d * d;              // ascending j from 0.0f, no fused multiply-add: the documented order
                        }
                    }
                }
            }
#pragma unroll
            for (int k = 0; k < PITCH_R; ++k)
                if (t0 + k <= tmax) out[t0 + k - 1] = acc[k];
        }
        if (lane == 0) p.flag[at] = any_bad ? 1 : 0;
    }
}

// ------------------------------------------------------------------------------------------------ frames
__device__ __forceinline__ int pitch_min_i(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o));
    return v;
}

// d'(tau) of frame k of a row, shared by the walk (pitch_frame_kernel) and the candidates (pitch_cand_kernel): lane l's 16 lags
// 16 l + 1 .. 16 l + 16 in dq and all of them in dpw (d'(tau) at tau - 1).  Returns whether the frame read a non-finite sample.
__device__ __forceinline__ bool pitch_dprime(const PitchArgs& p, int row, int64_t k, int lane, float (&dq)[16], float* dpw) {
    const int tmax = p.tmax;
    bool bad = false;
    const size_t at = (size_t)row * p.nblk_max + k;
    const float* Sb = p.S + at * p.ldt;
    for (int bb = 0; bb < 8; ++bb) bad |= p.flag[at + bb] != 0;
    // d(tau) = ((((((s_k + s_k+1) + s_k+2) + s_k+3) + s_k+4) + s_k+5) + s_k+6) + s_k+7
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int idx = 16 * lane + 4 * q;
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (idx < tmax) {                                         // (idx + 3 < ldt: ldt is tmax rounded up to 4)
            v = *reinterpret_cast<const f32x4*>(Sb + idx);
            for (int bb = 1; bb < 8; ++bb) {
                const f32x4 u = *reinterpret_cast<const f32x4*>(Sb + (size_t)bb * p.ldt + idx);
                v = v + u;
            }
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) dq[4 * q + e] = idx + e < tmax ? v[e] : 0.f;
    }
    // c(tau): 16 sequential adds inside the lane, an inclusive scan of the lanes' totals, c = (lanes before) + (running sum)
    float run[16];
    float acc = 0.f;
#pragma unroll
    for (int i = 0; i < 16; ++i) { acc = acc + dq[i]; run[i] = acc; }
    float incl = acc;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const float t = __shfl_up(incl, o);
        if (lane >= o) incl = incl + t;
    }
    float before = __shfl_up(incl, 1);
    if (lane == 0) before = 0.f;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const float c = before + run[i];
        const float tau = (float)(16 * lane + i + 1);
        dq[i] = c > 0.f ? (dq[i] * tau) / c : 1.f;
        dpw[16 * lane + i] = dq[i];
    }
    return bad;
}

__global__ __launch_bounds__(256) void pitch_frame_kernel(const PitchArgs p) {
    __shared__ float dps[4][MTTS_PITCH_MAX_LAG + 4];              // d'(tau) at tau - 1, one frame per wave
    const int row = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (blockIdx.x == 0 && row == 0)
        pitch_verdict(p.B, p.lengths, p.status, p.ld, 1, [&](int i) { const int64_t n = p.lengths[i]; return n < 0 || n > p.ld; });
    const int H = p.H, tmin = p.tmin, tmax = p.tmax;
    const int64_t L = p.lengths[row];
    const bool ok = L >= 0 && L <= p.ld;
    const int64_t n = ok ? pitch_frames(L, H, tmax) : 0;
    if (blockIdx.x == 0 && tid == 0) p.frames[row] = ok ? n : -1;
    float* dpw = dps[wave];
    for (int r = 0; r < 2; ++r) {
        const int64_t k = (int64_t)blockIdx.x * PITCH_FRAMES_PER_WG + wave * 2 + r;
        const bool live = k < n;                                  // (wave-uniform; n <= ld_frames, the host checked)
        float dq[16];
        bool bad = false;
        if (live) bad = pitch_dprime(p, row, k, lane, dq, dpw);
        __syncthreads();
        if (live) {
            // the first lag in [tmin, tmax) below the threshold
            int first = INT_MAX;
#pragma unroll
            for (int i = 15; i >= 0; --i) {
                const int tau = 16 * lane + i + 1;
                if (tau >= tmin && tau < tmax && dq[i] < p.thr) first = tau;
            }
            first = pitch_min_i(first);
            int star = INT_MAX;
            if (first != INT_MAX) {
                // ... then right while d'(tau + 1) < d'(tau), below tmax: the first lag at or after it where the descent stops
                const float over = dpw[16 * lane + 16];           // d' of the next lane's first lag (index < 1024 + 4)
#pragma unroll
                for (int i = 15; i >= 0; --i) {
                    const int tau = 16 * lane + i + 1;
                    const float next = i < 15 ? dq[i < 15 ? i + 1 : 15] : over;
                    const bool down = tau + 1 < tmax && next < dq[i];
                    if (tau >= first && tau < tmax && !down) star = tau;
                }
                star = pitch_min_i(star);
            } else {
                // no such lag: the lowest-index minimum over [tmin, tmax)
                float best = INFINITY;
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    const int tau = 16 * lane + i + 1;
                    if (tau >= tmin && tau < tmax && dq[i] < best) { best = dq[i]; star = tau; }
                }
#pragma unroll
                for (int o = 32; o > 0; o >>= 1) {
                    const float ob = __shfl_xor(best, o);
                    const int os = __shfl_xor(star, o);
                    if (ob < best || (ob == best && os < star)) { best = ob; star = os; }
                }
                if (star == INT_MAX) star = tmin;                 // (every d' is NaN or +inf: only with non-finite sums)
            }
            star = min(star, tmax - 1);                           // (already so: the descent ends at tmax - 1 at the latest)
            if (lane == 0) {
                const float b = dpw[star - 1], a = dpw[star - 2], c = dpw[star];
                float delta = 0.f;
                if (star > tmin && star < tmax - 1) {
                    const float den = (a - b) + (c - b);
                    if (den > 0.f) delta = (0.5f * (a - c)) / den;
                }
                const bool voiced = b < p.thr;
                float f0 = voiced ? p.fs / ((float)star + delta) : 0.f;
                float ap = b;
                if (bad) { f0 = 0.f; ap = NAN; }
                p.f0[(size_t)row * p.ld_frames + k] = f0;
                p.aper[(size_t)row * p.ld_frames + k] = ap;
            }
        } else if (k < p.ld_frames && lane == 0) {
            p.f0[(size_t)row * p.ld_frames + k] = 0.f;
            p.aper[(size_t)row * p.ld_frames + k] = 1.f;
        }
        __syncthreads();                                          // the next frame of this wave overwrites dpw
    }
}

hipError_t launch_pitch_track(const PitchArgs& a, hipStream_t s) {
    if (!a.audio || !a.lengths || !a.f0 || !a.aper || !a.frames || !a.status || !a.S || !a.flag) return hipErrorInvalidValue;
    if (a.B <= 0 || a.B > 65535 || a.ld < 4 || (a.ld & 3) || a.H < 8 || a.H > PITCH_MAX_HOP) return hipErrorInvalidValue;
    if (a.tmin < 2 || a.tmin + 2 > a.tmax || a.tmax > MTTS_PITCH_MAX_LAG || a.ldt != ((a.tmax + 3) & ~3)) return hipErrorInvalidValue;
    const int64_t n_max = pitch_frames(a.ld, a.H, a.tmax);
    if (a.ld_frames < 1 || a.ld_frames < n_max || a.nblk_max < n_max + 7) return hipErrorInvalidValue;
    if (n_max > 0) {
        const unsigned tiles = (unsigned)((n_max + 7 + PITCH_TILE - 1) / PITCH_TILE);
        hipLaunchKernelGGL(pitch_block_kernel, dim3(tiles, a.B), dim3(256), 0, s, a);
    }
    const unsigned groups = (unsigned)((a.ld_frames + PITCH_FRAMES_PER_WG - 1) / PITCH_FRAMES_PER_WG);
    hipLaunchKernelGGL(pitch_frame_kernel, dim3(groups, a.B), dim3(256), 0, s, a);
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------ statistics
// Exact order statistics of one row.  Set 0..2: the voiced frames (f0 > 0), ranks (m - 1) / 20, (m - 1) / 2, 19 (m - 1) / 20;
// set 3: the voiced frames with index >= last voiced index - tail, rank (mt - 1) / 2.  Four passes over the bytes of the bit
// pattern, most significant first; thread d owns bin d.
__global__ __launch_bounds__(256) void pitch_stats_kernel(const PitchStatsArgs a) {
    __shared__ unsigned s_hist[4][256], s_wsum[4][4];
    __shared__ unsigned s_pre[4];
    __shared__ long long s_rank[4];
    __shared__ int s_m, s_mt, s_last;                             // (frames < 2^30, the host checked)
    const int row = blockIdx.x, tid = threadIdx.x;
    if (row == 0)
        pitch_verdict(a.B, a.frames, a.status, a.ld_frames, 2, [&](int i) { const int64_t n = a.frames[i]; return n < 0 || n > a.ld_frames; });
    const int64_t n = a.frames[row];
    float* out = a.out + (size_t)row * 4;
    int64_t* cnt = a.counts + (size_t)row * 3;
    if (n < 0 || n > a.ld_frames) {
        if (tid < 4) out[tid] = NAN;
        if (tid < 3) cnt[tid] = tid == 0 ? -1 : 0;
        return;
    }
    const float* f0 = a.f0 + (size_t)row * a.ld_frames;
    if (tid == 0) { s_m = 0; s_mt = 0; s_last = -1; }
    __syncthreads();
    int m = 0;
    int last = -1;
    for (int64_t k = tid; k < n; k += 256)
        if (f0[k] > 0.f) { ++m; last = (int)k; }
    if (m) { atomicAdd(&s_m, m); atomicMax(&s_last, last); }
    __syncthreads();
    const int64_t lo = (int64_t)s_last - a.tail;                         // (s_last = -1 without a voiced frame: nothing is counted)
    int mt = 0;
    for (int64_t k = tid; k < n; k += 256)
        if (f0[k] > 0.f && k >= lo) ++mt;
    if (mt) atomicAdd(&s_mt, mt);
    __syncthreads();
    m = s_m; mt = s_mt;
    if (tid < 4) {
        s_pre[tid] = 0u;
        const long long rank = tid == 0 ? (long long)(m - 1) / 20 : tid == 1 ? (long long)(m - 1) / 2 : tid == 2 ? (long long)(m - 1) * 19 / 20
                                                                                                                 : (long long)(mt - 1) / 2;
        s_rank[tid] = (tid < 3 ? m > 0 : mt >= 3) ? rank : LLONG_MAX;            // LLONG_MAX: no bin holds it, the set is left out
    }
    if (m > 0) {
        for (int pass = 0; pass < 4; ++pass) {
            const int shift = 24 - 8 * pass;
#pragma unroll
            for (int q = 0; q < 4; ++q) s_hist[q][tid] = 0u;
            __syncthreads();
            unsigned pre[4];
            long long rank[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) { pre[q] = s_pre[q]; rank[q] = s_rank[q]; }
            for (int64_t k = tid; k < n; k += 256) {
                const float v = f0[k];
                if (!(v > 0.f)) continue;
                const unsigned u = __float_as_uint(v);
                const unsigned hi = pass == 0 ? 0u : u >> (shift + 8);
                const unsigned d = (u >> shift) & 255u;
#pragma unroll
                for (int q = 0; q < 3; ++q)
                    if (hi == pre[q]) atomicAdd(&s_hist[q][d], 1u);
                if (k >= lo && hi == pre[3]) atomicAdd(&s_hist[3][d], 1u);
            }
            __syncthreads();
            unsigned c[4], incl[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                c[q] = s_hist[q][tid];
                incl[q] = c[q];
                for (int o = 1; o < 64; o <<= 1) {
                    const unsigned up = __shfl_up(incl[q], o, 64);
                    if ((tid & 63) >= o) incl[q] += up;
                }
                if ((tid & 63) == 63) s_wsum[q][tid >> 6] = incl[q];
            }
            __syncthreads();
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                for (int w = 0; w < (tid >> 6); ++w) incl[q] += s_wsum[q][w];
                const long long lo_r = (long long)(incl[q] - c[q]), hi_r = (long long)incl[q];
                if (rank[q] >= lo_r && rank[q] < hi_r) { s_rank[q] = rank[q] - lo_r; s_pre[q] = (pre[q] << 8) | (unsigned)tid; }
            }
            __syncthreads();
        }
    }
    __syncthreads();
    if (tid < 4) out[tid] = (tid < 3 ? m > 0 : mt >= 3) ? __uint_as_float(s_pre[tid]) : NAN;
    if (tid == 0) { cnt[0] = n; cnt[1] = m; cnt[2] = mt; }
}

hipError_t launch_pitch_stats(const PitchStatsArgs& a, hipStream_t s) {
    if (!a.f0 || !a.frames || !a.out || !a.counts || !a.status) return hipErrorInvalidValue;
    if (a.B <= 0 || a.B > 65535 || a.ld_frames < 1 || a.tail < 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(pitch_stats_kernel, dim3(a.B), dim3(256), 0, s, a);
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------ candidates
// The lattice of the path search: every record-setting dip of d' of a frame with its mass under a threshold prior uniform on
// [0, 2 thr].  A wave owns a frame and a lane 16 lags, as in pitch_frame_kernel; a lane finds its dips in registers, the running
// record is an exclusive prefix-minimum over the lanes (a minimum rounds nothing: any scan shape gives the same bits), and the kept
// dips are listed in LDS in ascending lag, where the eight of greatest mass are chosen by counting.
constexpr int PITCH_CAND_LIST = 512;           // a dip needs a higher neighbour on its left: at most one in two lags

struct PitchCandArgs {
    float* period = nullptr;           // [B][ld_frames][8]
    float* mass = nullptr;             // [B][ld_frames][8]
    float* depth = nullptr;            // [B][ld_frames][8]
    int32_t* count = nullptr;          // [B][ld_frames]
    float* unvoiced = nullptr;         // [B][ld_frames]
    float* floor = nullptr;            // [B][ld_frames]
};

__device__ __forceinline__ float pitch_prior_cdf(float v, float thr2) { return fminf(fmaxf(v / thr2, 0.f), 1.f); }

__global__ __launch_bounds__(256) void pitch_cand_kernel(const PitchArgs p, const PitchCandArgs o) {
    __shared__ float dps[4][MTTS_PITCH_MAX_LAG + 4];              // d'(tau) at tau - 1, one frame per wave
    __shared__ float l_mass[4][PITCH_CAND_LIST];
    __shared__ short l_tau[4][PITCH_CAND_LIST];
    __shared__ unsigned char l_sel[4][PITCH_CAND_LIST];
    const int row = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (blockIdx.x == 0 && row == 0)
        pitch_verdict(p.B, p.lengths, p.status, p.ld, 3, [&](int i) { const int64_t n = p.lengths[i]; return n < 0 || n > p.ld; });
    const int H = p.H, tmin = p.tmin, tmax = p.tmax;
    const float thr2 = 2.f * p.thr;
    const int64_t L = p.lengths[row];
    const bool ok = L >= 0 && L <= p.ld;
    const int64_t n = ok ? pitch_frames(L, H, tmax) : 0;
    if (blockIdx.x == 0 && tid == 0) p.frames[row] = ok ? n : -1;
    float* dpw = dps[wave];
    float* lm = l_mass[wave];
    short* lt = l_tau[wave];
    unsigned char* ls = l_sel[wave];
    for (int r = 0; r < 2; ++r) {
        const int64_t k = (int64_t)blockIdx.x * PITCH_FRAMES_PER_WG + wave * 2 + r;
        const bool live = k < n;                                  // (wave-uniform; n <= ld_frames, the host checked)
        const size_t at = (size_t)row * p.ld_frames + k;
        float dq[16];
        bool bad = false;
        if (live) bad = pitch_dprime(p, row, k, lane, dq, dpw);
        __syncthreads();
        int K = 0;                                                // kept dips of the frame
        float unvoiced = 1.f, floor_v = 1.f;
        if (live) {
            // the dips of this lane: tmin < tau < tmax - 1, d'(tau) < d'(tau - 1), d'(tau) <= d'(tau + 1); eligible below 2 thr
            const float under = lane > 0 ? dpw[16 * lane - 1] : INFINITY;          // d' of the previous lane's last lag
            const float over = dpw[16 * lane + 16];                                // d' of the next lane's first lag (index < 1024 + 4)
            unsigned elig = 0u;
            float lane_min = INFINITY;
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const int tau = 16 * lane + i + 1;
                const float prev = i > 0 ? dq[i > 0 ? i - 1 : 0] : under;
                const float next = i < 15 ? dq[i < 15 ? i + 1 : 15] : over;
                if (tau > tmin && tau < tmax - 1 && dq[i] < prev && dq[i] <= next && dq[i] < thr2) {
                    elig |= 1u << i;
                    lane_min = fminf(lane_min, dq[i]);
                }
            }
            float incl = lane_min;
#pragma unroll
            for (int s = 1; s < 64; s <<= 1) {
                const float t = __shfl_up(incl, s);
                if (lane >= s) incl = fminf(incl, t);
            }
            float record = __shfl_up(incl, 1);                    // the lowest eligible depth of the lanes before this one
            if (lane == 0) record = INFINITY;
            const float last = __shfl(incl, 63);                  // the last kept depth of the frame (+inf: none kept)
            // the kept ones: below the record so far.  Mass = F(previous kept depth) - F(depth), F(no previous) = 1.0f
            unsigned kept = 0u;
            float km[16];
            float run = record;
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                km[i] = 0.f;
                if ((elig >> i & 1u) && dq[i] < run) {
                    const float before = run < INFINITY ? pitch_prior_cdf(run, thr2) : 1.f;
                    km[i] = before - pitch_prior_cdf(dq[i], thr2);
                    kept |= 1u << i;
                    run = dq[i];
                }
            }
            const int mine = __popc(kept);
            int pos = mine;                                       // inclusive scan of the counts: where this lane's list starts
#pragma unroll
            for (int s = 1; s < 64; s <<= 1) {
                const int t = __shfl_up(pos, s);
                if (lane >= s) pos += t;
            }
            K = __shfl(pos, 63);
            pos -= mine;
#pragma unroll
            for (int i = 0; i < 16; ++i)
                if (kept >> i & 1u) {                             // (pos < 512: a lane keeps at most 8 of its 16 lags)
                    lm[pos] = km[i];
                    lt[pos] = (short)(16 * lane + i + 1);
                    ++pos;
                }
            unvoiced = last < INFINITY ? pitch_prior_cdf(last, thr2) : 1.f;
            // the floor: the lowest-index minimum of d' over [tmin, tmax), as YIN reports it for an unvoiced frame
            float best = INFINITY;
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const int tau = 16 * lane + i + 1;
                if (tau >= tmin && tau < tmax && dq[i] < best) best = dq[i];
            }
#pragma unroll
            for (int s = 32; s > 0; s >>= 1) {
                const float ob = __shfl_xor(best, s);
                if (ob < best) best = ob;
            }
            floor_v = best < INFINITY ? best : dpw[tmin - 1];    // (every d' is NaN or +inf: only with non-finite sums)
        }
        __syncthreads();
        if (live) {
            // the eight of greatest mass, ties to the lower lag: candidate j is held when fewer than 8 others come before it
            for (int j = lane; j < K; j += 64) {
                const float mj = lm[j];
                int before = 0;
                if (K > MTTS_PITCH_CANDS)
                    for (int i = 0; i < K; ++i) {
                        const float mi = lm[i];
                        before += (mi > mj || (mi == mj && i < j)) ? 1 : 0;
                    }
                ls[j] = before < MTTS_PITCH_CANDS ? 1 : 0;
            }
        }
        __syncthreads();
        if (live) {
            const int held = min(K, MTTS_PITCH_CANDS);
            if (!bad)
                for (int j = lane; j < K; j += 64) {
                    if (!ls[j]) continue;
                    int slot = 0;                                 // ascending lag: the held ones before it
                    if (K > MTTS_PITCH_CANDS) { for (int i = 0; i < j; ++i) slot += ls[i]; } else slot = j;
                    const int tau = lt[j];
                    const float b = dpw[tau - 1], a = dpw[tau - 2], c = dpw[tau];
                    float delta = 0.f;
                    const float den = (a - b) + (c - b);          // (tmin < tau < tmax - 1 holds for every dip)
                    if (den > 0.f) delta = (0.5f * (a - c)) / den;
                    o.period[at * MTTS_PITCH_CANDS + slot] = (float)tau + delta;
                    o.mass[at * MTTS_PITCH_CANDS + slot] = lm[j];
                    o.depth[at * MTTS_PITCH_CANDS + slot] = b;
                }
            const int from = bad ? 0 : held;
            if (lane >= from && lane < MTTS_PITCH_CANDS) {
                o.period[at * MTTS_PITCH_CANDS + lane] = 0.f;
                o.mass[at * MTTS_PITCH_CANDS + lane] = 0.f;
                o.depth[at * MTTS_PITCH_CANDS + lane] = 0.f;
            }
            if (lane == 0) {
                o.count[at] = bad ? -1 : held;
                o.unvoiced[at] = bad ? 1.f : unvoiced;
                o.floor[at] = bad ? NAN : floor_v;
            }
        } else if (k < p.ld_frames) {
            if (lane < MTTS_PITCH_CANDS) {
                o.period[at * MTTS_PITCH_CANDS + lane] = 0.f;
                o.mass[at * MTTS_PITCH_CANDS + lane] = 0.f;
                o.depth[at * MTTS_PITCH_CANDS + lane] = 0.f;
            }
            if (lane == 0) { o.count[at] = 0; o.unvoiced[at] = 1.f; o.floor[at] = 1.f; }
        }
        __syncthreads();                                          // the next frame of this wave overwrites dpw and the lists
    }
}

hipError_t launch_pitch_candidates(const PitchArgs& a, const PitchCandArgs& o, hipStream_t s) {
    if (!a.audio || !a.lengths || !a.frames || !a.status || !a.S || !a.flag) return hipErrorInvalidValue;
    if (!o.period || !o.mass || !o.depth || !o.count || !o.unvoiced || !o.floor) return hipErrorInvalidValue;
    if (a.B <= 0 || a.B > 65535 || a.ld < 4 || (a.ld & 3) || a.H < 8 || a.H > PITCH_MAX_HOP) return hipErrorInvalidValue;
    if (a.tmin < 2 || a.tmin + 2 > a.tmax || a.tmax > MTTS_PITCH_MAX_LAG || a.ldt != ((a.tmax + 3) & ~3)) return hipErrorInvalidValue;
    const int64_t n_max = pitch_frames(a.ld, a.H, a.tmax);
    if (a.ld_frames < 1 || a.ld_frames < n_max || a.nblk_max < n_max + 7) return hipErrorInvalidValue;
    if (n_max > 0) {
        const unsigned tiles = (unsigned)((n_max + 7 + PITCH_TILE - 1) / PITCH_TILE);
        hipLaunchKernelGGL(pitch_block_kernel, dim3(tiles, a.B), dim3(256), 0, s, a);
    }
    const unsigned groups = (unsigned)((a.ld_frames + PITCH_FRAMES_PER_WG - 1) / PITCH_FRAMES_PER_WG);
    hipLaunchKernelGGL(pitch_cand_kernel, dim3(groups, a.B), dim3(256), 0, s, a, o);
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------ shortest path
// One wavefront (one workgroup) per clip; the search is sequential in frames.  A chunk of PITCH_VIT_CHUNK frames is prepared at
// full width -- lane l stages the periods and local costs of frame l with one batch of loads, then lane (r, s) = (lane / 8,
// lane % 8) computes the voiced-to-voiced transition of every frame of the chunk, the one division of the recurrence, from LDS
// into LDS -- and then walked frame by frame with lanes 0 .. 8 as the states: D(r) of the frame before
// is read across lanes (v_readlane), the nine 4-bit back pointers of a frame are one 64-bit word that lane (frame % 64) keeps and
// the chunk stores with an ordinary coalesced vector store.  The way back reads those words a chunk at a time, again across lanes.
constexpr int PITCH_VIT_CHUNK = 64;
constexpr int PITCH_U = MTTS_PITCH_CANDS;      // the index of the unvoiced state

struct PitchPathArgs {
    const float* period = nullptr;     // [B][ld_frames][8]
    const float* mass = nullptr;
    const float* depth = nullptr;
    const int32_t* count = nullptr;    // [B][ld_frames]
    const float* unvoiced = nullptr;
    const float* floor = nullptr;
    int64_t ld_frames = 0;
    const int64_t* frames = nullptr;   // [B]
    int B = 0;
    float fs = 0.f, jump = 0.f, sw = 0.f;
    float* f0 = nullptr;               // [B][ld_frames]
    float* aper = nullptr;
    signed char* state = nullptr;      // [B][ld_frames]
    int64_t* status = nullptr;
    unsigned long long* back = nullptr;    // [B][ld_frames]
};

__device__ __forceinline__ float pitch_lane_f(float v, int l) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), l)); }

__global__ __launch_bounds__(64) void pitch_viterbi_kernel(const PitchPathArgs a) {
    __shared__ float s_trans[PITCH_VIT_CHUNK][64];                // [frame of the chunk][r * 8 + s]
    __shared__ float s_local[PITCH_VIT_CHUNK][8];                 // 1.0f - mass
    __shared__ float s_per[PITCH_VIT_CHUNK + 1][8];               // the periods of the chunk; [0]: the frame before it
    const int row = blockIdx.x, lane = threadIdx.x;
    if (lane < 8) s_per[0][lane] = 0.f;
    if (row == 0)
        pitch_verdict(a.B, a.frames, a.status, a.ld_frames, 4, [&](int i) { const int64_t n = a.frames[i]; return n < 0 || n > a.ld_frames; });
    const int64_t n_in = a.frames[row];
    const int64_t n = n_in < 0 || n_in > a.ld_frames ? 0 : n_in;
    const size_t base = (size_t)row * a.ld_frames;
    for (int64_t k = n + lane; k < a.ld_frames; k += 64) {        // columns at or beyond n, and every column of a refused row
        a.f0[base + k] = 0.f;
        a.aper[base + k] = 1.f;
        a.state[base + k] = -1;
    }
    if (n == 0) return;                                           // (workgroup-uniform)
    const int s = lane & 7, r_of = lane >> 3;
    float D = INFINITY;                                           // lanes 0 .. 8: the cost of state `lane` at the frame before
    for (int64_t k0 = 0; k0 < n; k0 += PITCH_VIT_CHUNK) {
        const int nk = (int)min((int64_t)PITCH_VIT_CHUNK, n - k0);
        // prepare: lane l holds count and unvoiced mass of frame k0 + l; transitions and local costs of the chunk into LDS
        const int cnt_l = lane < nk ? a.count[base + k0 + lane] : 0;
        const float uv_l = lane < nk ? a.unvoiced[base + k0 + lane] : 1.f;
        if (lane < nk) {                                          // lane l stages frame k0 + l: sixteen loads in flight, no loop of waits
            const size_t at = (base + k0 + lane) * MTTS_PITCH_CANDS;
            float pv[MTTS_PITCH_CANDS], mv[MTTS_PITCH_CANDS];
#pragma unroll
            for (int q = 0; q < MTTS_PITCH_CANDS; ++q) { pv[q] = a.period[at + q]; mv[q] = a.mass[at + q]; }
#pragma unroll
            for (int q = 0; q < MTTS_PITCH_CANDS; ++q) { s_per[lane + 1][q] = pv[q]; s_local[lane][q] = 1.0f - mv[q]; }
        }
        __syncthreads();
#pragma unroll 4
        for (int kk = 0; kk < nk; ++kk) {                         // (the transition into frame 0 of the clip is never read)
            const float ps = s_per[kk + 1][s], pr = s_per[kk][r_of];
            s_trans[kk][lane] = a.jump * (fabsf(ps - pr) / fminf(ps, pr));
        }
        __syncthreads();
        if (lane < MTTS_PITCH_CANDS) s_per[0][lane] = s_per[nk][lane];   // the next chunk's "frame before"; staged over after the chunk's last barrier
        unsigned long long word_l = 0ull;
        for (int kk = 0; kk < nk; ++kk) {
            const int cnt_in = __builtin_amdgcn_readlane(cnt_l, kk);
            const float uv = pitch_lane_f(uv_l, kk);
            const bool bad = cnt_in < 0;
            const int cnt = min(max(cnt_in, 0), MTTS_PITCH_CANDS);
            const bool valid = lane < 8 ? lane < cnt : lane == PITCH_U;
            const float local = lane < 8 ? s_local[kk][s] : (bad ? 0.f : 1.0f - uv);
            float best = INFINITY;
            int arg = 0;
            if (k0 + kk > 0) {
#pragma unroll
                for (int r = 0; r < 8; ++r) {                     // from a candidate: a jump, or the switch into U
                    const float dr = pitch_lane_f(D, r);
                    const float t = lane < 8 ? s_trans[kk][r * 8 + s] : a.sw;
                    const float c = dr + t;
                    if (dr < INFINITY && c < best) { best = c; arg = r; }
                }
                const float du = pitch_lane_f(D, PITCH_U);        // from U: the switch, or nothing
                const float cu = du + (lane < 8 ? a.sw : 0.f);
                if (cu < best) { best = cu; arg = PITCH_U; }
            } else {
                best = 0.f;                                       // D_0(s) = local_0(s)
            }
            float Dn = valid ? best + local : INFINITY;
            if (lane > PITCH_U) Dn = INFINITY;
            float m = INFINITY;
            unsigned long long word = 0ull;
#pragma unroll
            for (int q = 0; q <= PITCH_U; ++q) {
                m = fminf(m, pitch_lane_f(Dn, q));
                word |= (unsigned long long)(unsigned)__builtin_amdgcn_readlane(arg, q) << (4 * q);
            }
            D = Dn - m;                                           // one rounding; +inf stays +inf
            if (lane == kk) word_l = word;
        }
        if (lane < nk) a.back[base + k0 + lane] = word_l;
        __syncthreads();                                          // the next chunk overwrites the LDS tables
    }
    // the end state: the lowest-index minimum of the last frame
    int state = 0;
    {
        float m = INFINITY;
#pragma unroll
        for (int q = 0; q <= PITCH_U; ++q) {
            const float d = pitch_lane_f(D, q);
            if (d < m) { m = d; state = q; }
        }
    }
    __threadfence_block();
    __syncthreads();                                              // the back pointers are read by other lanes than wrote them
    for (int64_t k0 = (n - 1) / PITCH_VIT_CHUNK * PITCH_VIT_CHUNK; k0 >= 0; k0 -= PITCH_VIT_CHUNK) {
        const int nk = (int)min((int64_t)PITCH_VIT_CHUNK, n - k0);
        const unsigned long long word_l = lane < nk ? a.back[base + k0 + lane] : 0ull;
        const int lo = (int)(word_l & 0xffffffffull), hi = (int)(word_l >> 32);
        int state_l = 0;
        for (int kk = nk - 1; kk >= 0; --kk) {                    // (uniform: every lane walks, lane kk keeps the state of its frame)
            if (lane == kk) state_l = state;
            const unsigned long long w = (unsigned long long)(unsigned)__builtin_amdgcn_readlane(lo, kk) |
                                         ((unsigned long long)(unsigned)__builtin_amdgcn_readlane(hi, kk) << 32);
            state = (int)(w >> (4 * state) & 15ull);
            state = min(state, PITCH_U);
        }
        if (lane < nk) {
            const size_t at = base + k0 + lane;
            float f0 = 0.f, ap;
            if (state_l < PITCH_U) {
                f0 = a.fs / a.period[at * MTTS_PITCH_CANDS + state_l];
                ap = a.depth[at * MTTS_PITCH_CANDS + state_l];
            } else {
                ap = a.count[at] < 0 ? NAN : a.floor[at];
            }
            a.f0[at] = f0;
            a.aper[at] = ap;
            a.state[at] = (signed char)state_l;
        }
    }
}

hipError_t launch_pitch_viterbi(const PitchPathArgs& a, hipStream_t s) {
    if (!a.period || !a.mass || !a.depth || !a.count || !a.unvoiced || !a.floor || !a.frames) return hipErrorInvalidValue;
    if (!a.f0 || !a.aper || !a.state || !a.status || !a.back) return hipErrorInvalidValue;
    if (a.B <= 0 || a.B > 65535 || a.ld_frames < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(pitch_viterbi_kernel, dim3(a.B), dim3(64), 0, s, a);
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------ fold onto tokens
// A wave per token, four tokens per workgroup, gridded over (tokens / 4, clip).  Every workgroup judges its own row (the marks of
// the row, read once by its 256 threads); workgroup (0, 0) writes the verdict for the batch.
struct PitchFoldArgs {
    const float* f0 = nullptr;         // [B][ld_frames]
    int64_t ld_frames = 0;
    const int64_t* frames = nullptr;   // [B]
    int B = 0, Tx = 0;
    int H = 0;
    int64_t centre = 0;                // W + tmax: twice the offset of a frame's nominal centre
    const int64_t* marks = nullptr;    // [B][Tx][2]
    const int64_t* x_lengths = nullptr;
    const float* audio = nullptr;      // [B][ld] or null
    int64_t ld = 0;
    const int64_t* lengths = nullptr;  // [B] or null
    int32_t* counts = nullptr;         // [B][Tx][2]
    float* hz = nullptr;               // [B][Tx][3]
    double* mean_square = nullptr;     // [B][Tx] or null
    int64_t* status = nullptr;
};

// 0 when row b is accepted, else the reason: 1 frames, 2 x_lengths, 3 length, 4 a mark outside [0, length], 5 start > end,
// 6 marks not ascending.  `t0, step`: the tokens this thread looks at.
__device__ __forceinline__ int pitch_fold_row(const PitchFoldArgs& a, int b, int t0, int step) {
    const int64_t n = a.frames[b], xl = a.x_lengths[b];
    if (n < 0 || n > a.ld_frames) return 1;
    if (xl < 0 || xl > a.Tx) return 2;
    int64_t L = INT64_MAX;
    if (a.lengths) {
        L = a.lengths[b];
        if (L < 0 || (a.audio && L > a.ld)) return 3;
    }
    const int64_t* mk = a.marks + (size_t)b * a.Tx * 2;
    int why = 0;
    for (int64_t i = t0; i < xl; i += step) {
        const int64_t st = mk[2 * i], en = mk[2 * i + 1];
        if (st == -1 && en == -1) continue;                       // no token
        int w = 0;
        if (st < 0 || en < 0 || st > L || en > L) w = 4;
        else if (st > en) w = 5;
        else {
            int64_t j = i - 1;
            while (j >= 0 && mk[2 * j] == -1 && mk[2 * j + 1] == -1) --j;
            if (j >= 0 && st < mk[2 * j + 1]) w = 6;
        }
        if (w && (!why || w < why)) why = w;
    }
    return why;
}

__device__ __forceinline__ int64_t pitch_first_frame(int64_t mark, int64_t centre, int H, int64_t n) {
    // the first k with 2 k H + centre >= 2 mark, inside [0, n]
    const int64_t num = 2 * mark - centre;
    if (num <= 0) return 0;
    return min(n, (num + 2 * (int64_t)H - 1) / (2 * (int64_t)H));
}

__global__ __launch_bounds__(256) void pitch_fold_kernel(const PitchFoldArgs a) {
    const int row = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (blockIdx.x == 0 && row == 0) {
        const int i = first_refused_row(a.B, [&](int b) { return pitch_fold_row(a, b, 0, 1) != 0; });
        if (tid == 0) {
            const int why = i < a.B ? pitch_fold_row(a, i, 0, 1) : 0;
            a.status[0] = i < a.B ? i + 1 : 0;
            a.status[1] = why;
            a.status[2] = 0;
            a.status[3] = 0;
            a.status[4] = 5;
        }
    }
    const bool refused = __syncthreads_or(pitch_fold_row(a, row, tid, 256));
    const int64_t i = (int64_t)blockIdx.x * 4 + wave;
    if (i >= a.Tx) return;                                        // (wave-uniform; no barrier below)
    const size_t at = (size_t)row * a.Tx + i;
    int32_t frames = 0, voiced = 0;
    float med = NAN, first = NAN, last = NAN;
    double ms = 0.0;
    if (refused) {
        frames = -1;
        ms = NAN;
    } else if (i < a.x_lengths[row]) {
        const int64_t st = a.marks[2 * at], en = a.marks[2 * at + 1];
        if (st >= 0) {                                            // (-1, -1): no token
            const int64_t n = a.frames[row];
            const int64_t k_lo = pitch_first_frame(st, a.centre, a.H, n), k_hi = pitch_first_frame(en, a.centre, a.H, n);
            const float* f = a.f0 + (size_t)row * a.ld_frames + k_lo;
            const int F = (int)(k_hi - k_lo);                     // (frames < 2^30, the host checked)
            frames = F;
            int m = 0, lo_i = INT_MAX, hi_i = -1;
            for (int j = lane; j < F; j += 64)
                if (f[j] > 0.f) { ++m; lo_i = min(lo_i, j); hi_i = max(hi_i, j); }
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                m += __shfl_xor(m, o);
                lo_i = min(lo_i, __shfl_xor(lo_i, o));
                hi_i = max(hi_i, __shfl_xor(hi_i, o));
            }
            voiced = m;
            if (m > 0) {
                first = f[lo_i];
                last = f[hi_i];
                // the order statistic v[(m - 1) / 2] by counting: the value with exactly that many before it (ties by index)
                const int want = (m - 1) / 2;
                float found = -1.f;
                for (int j = lane; j < F; j += 64) {
                    const float v = f[j];
                    if (!(v > 0.f)) continue;
                    int before = 0;
                    for (int q = lo_i; q <= hi_i; ++q) {
                        const float u = f[q];
                        before += (u > 0.f && (u < v || (u == v && q < j))) ? 1 : 0;
                    }
                    if (before == want) found = v;
                }
#pragma unroll
                for (int o = 32; o > 0; o >>= 1) found = fmaxf(found, __shfl_xor(found, o));     // exactly one lane found it
                med = found;
            }
            if (a.audio && en > st) {
                // fp64: lane l adds x[st + l + 64 j]^2 for j ascending from 0.0, then v = v + v[lane ^ o] for o = 32 .. 1
                const float* x = a.audio + (size_t)row * a.ld;
                double acc = 0.0;
                bool bad = false;
                for (int64_t q = st + lane; q < en; q += 64) {
                    const float v = x[q];
                    bad |= !(fabsf(v) <= FLT_MAX);
                    acc = acc + (double)v * (double)v;
                }
#pragma unroll
                for (int o = 32; o > 0; o >>= 1) acc = acc + __shfl_xor(acc, o);
                ms = __any(bad) ? (double)NAN : acc / (double)(en - st);
            }
        }
    }
    if (lane == 0) {
        a.counts[2 * at] = frames;
        a.counts[2 * at + 1] = voiced;
        a.hz[3 * at] = med;
        a.hz[3 * at + 1] = first;
        a.hz[3 * at + 2] = last;
        if (a.mean_square) a.mean_square[at] = ms;
    }
}

hipError_t launch_pitch_fold(const PitchFoldArgs& a, hipStream_t s) {
    if (!a.f0 || !a.frames || !a.marks || !a.x_lengths || !a.counts || !a.hz || !a.status) return hipErrorInvalidValue;
    if (a.B <= 0 || a.B > 65535 || a.Tx < 1 || a.ld_frames < 1 || a.H < 8 || a.centre < 1) return hipErrorInvalidValue;
    if ((a.audio != nullptr) != (a.mean_square != nullptr) || (a.audio && (!a.lengths || a.ld < 1))) return hipErrorInvalidValue;
    hipLaunchKernelGGL(pitch_fold_kernel, dim3((unsigned)((a.Tx + 3) / 4), a.B), dim3(256), 0, s, a);
    return hipGetLastError();
}

}  // namespace mtts

using namespace mtts;

// Parameters -> window, smallest and largest lag; false with the error set when the contract refuses them
static bool pitch_plan(const char* who, int sample_rate, int hop, double fmin, double fmax, int* window, int* tmin, int* tmax) {
    const std::string w(who);
    if (sample_rate < 8000 || sample_rate > 48000) { set_error(w + ": sample_rate must lie in [8000, 48000], got " + std::to_string(sample_rate)); return false; }
    if (hop < 8 || hop > PITCH_MAX_HOP) { set_error(w + ": hop must lie in [8, 512] samples, got " + std::to_string(hop)); return false; }
    if (!(fmin > 0.0) || !(fmax > 0.0) || !(fmin <= DBL_MAX) || !(fmax <= DBL_MAX)) { set_error(w + ": fmin and fmax must be positive and finite"); return false; }
    const double hi = std::ceil((double)sample_rate / fmin), lo = std::floor((double)sample_rate / fmax);
    if (lo < 2.0 || lo + 2.0 > hi || hi > (double)MTTS_PITCH_MAX_LAG) {
        set_error(w + ": lags [floor(fs / fmax), ceil(fs / fmin)] = [" + std::to_string((long long)std::min(lo, 1e15)) + ", " +
                  std::to_string((long long)std::min(hi, 1e15)) + "] must satisfy 2 <= min_lag, min_lag + 2 <= max_lag <= " + std::to_string(MTTS_PITCH_MAX_LAG));
        return false;
    }
    *window = 8 * hop;
    *tmin = (int)lo;
    *tmax = (int)hi;
    return true;
}

static void pitch_carve(WS& ws, int B, int64_t ld, int hop, int tmax, PitchArgs* a) {
    const int64_t n_max = pitch_frames(ld, hop, tmax);
    const int64_t nblk = n_max + 7;
    const int ldt = (tmax + 3) & ~3;
    int64_t* status = static_cast<int64_t*>(ws.bytes(256));
    float* S = ws.f((size_t)B * nblk * ldt);
    int32_t* flag = static_cast<int32_t*>(ws.bytes((size_t)B * nblk * sizeof(int32_t)));
    if (a) { a->status = status; a->S = S; a->flag = flag; a->nblk_max = nblk; a->ldt = ldt; }
}

extern "C" {

// ---- pitch (pitch.hip)
int mtts_pitch_tile(void) { return PITCH_TILE; }

int mtts_pitch_plan(int sample_rate, int hop, double fmin, double fmax, int* window, int* min_lag, int* max_lag) {
    int w, lo, hi;
    if (!pitch_plan("mtts_pitch_plan", sample_rate, hop, fmin, fmax, &w, &lo, &hi)) return -1;
    if (window) *window = w;
    if (min_lag) *min_lag = lo;
    if (max_lag) *max_lag = hi;
    return 0;
}

int64_t mtts_pitch_workspace_bytes(int64_t ld, int B, int sample_rate, int hop, double fmin, double fmax) {
    int w, lo, hi;
    if (!pitch_plan("mtts_pitch_workspace_bytes", sample_rate, hop, fmin, fmax, &w, &lo, &hi)) return -1;
    if (ld < 4 || B <= 0) { set_error("mtts_pitch_workspace_bytes: bad shape"); return -1; }
    WS ws(nullptr, 0);
    pitch_carve(ws, B, ld, hop, hi, nullptr);
    return (int64_t)ws.off + 256;
}

int mtts_pitch_track(const float* d_audio, int64_t ld, const int64_t* d_lengths, int B, int sample_rate, int hop, double fmin, double fmax,
                     double threshold, float* d_f0, float* d_aper, int64_t ld_frames, int64_t* d_frames, void* d_ws, int64_t ws_bytes,
                     void* stream) {
    if (!d_audio || !d_lengths || !d_f0 || !d_aper || !d_frames || !d_ws) { set_error("mtts_pitch_track: null argument"); return -1; }
    if (B < 1 || B > 65535) { set_error("mtts_pitch_track: B must lie in [1, 65535]"); return -1; }
    if (ld < 4 || (ld & 3) || (reinterpret_cast<uintptr_t>(d_audio) & 15) || (reinterpret_cast<uintptr_t>(d_ws) & 15)) {
        set_error("mtts_pitch_track: rows must be 16-byte aligned (ld a positive multiple of 4 samples)");
        return -1;
    }
    PitchArgs a;
    int window;
    if (!pitch_plan("mtts_pitch_track", sample_rate, hop, fmin, fmax, &window, &a.tmin, &a.tmax)) return -1;
    if (!(threshold > 0.0) || !(threshold < 1.0)) { set_error("mtts_pitch_track: threshold must lie in (0, 1)"); return -1; }
    const int64_t n_max = pitch_frames(ld, hop, a.tmax);
    if (ld_frames < 1 || ld_frames < n_max) {
        set_error("mtts_pitch_track: ld_frames = " + std::to_string(ld_frames) + " is less than the " + std::to_string(std::max<int64_t>(n_max, 1)) +
                  " frames a row of ld samples can have");
        return -1;
    }
    if (ld_frames > 0x3fffffff) { set_error("mtts_pitch_track: too many frames in a row"); return -1; }
    WS ws(d_ws, (size_t)ws_bytes);
    pitch_carve(ws, B, ld, hop, a.tmax, &a);
    if (ws_bytes < 256 || ws.overflow) { set_error("mtts_pitch_track: workspace too small (mtts_pitch_workspace_bytes)"); return -1; }
    a.audio = d_audio; a.ld = ld; a.lengths = d_lengths; a.B = B; a.H = hop;
    a.thr = (float)threshold; a.fs = (float)sample_rate;
    a.f0 = d_f0; a.aper = d_aper; a.ld_frames = ld_frames; a.frames = d_frames;
    HIP_OK(launch_pitch_track(a, static_cast<hipStream_t>(stream)));
    return 0;
}

int mtts_pitch_stats(const float* d_f0, int64_t ld_frames, const int64_t* d_frames, int B, int64_t tail_frames, float* d_out_hz,
                     int64_t* d_counts, void* d_ws, int64_t ws_bytes, void* stream) {
    if (!d_f0 || !d_frames || !d_out_hz || !d_counts || !d_ws) { set_error("mtts_pitch_stats: null argument"); return -1; }
    if (B < 1 || B > 65535) { set_error("mtts_pitch_stats: B must lie in [1, 65535]"); return -1; }
    if (ld_frames < 1 || ld_frames > 0x3fffffff) { set_error("mtts_pitch_stats: ld_frames must lie in [1, 2^30)"); return -1; }
    if (tail_frames < 0) { set_error("mtts_pitch_stats: tail_frames must not be negative"); return -1; }
    if (reinterpret_cast<uintptr_t>(d_ws) & 15) { set_error("mtts_pitch_stats: misaligned workspace (16 bytes)"); return -1; }
    if (ws_bytes < 256) { set_error("mtts_pitch_stats: workspace too small (256 bytes: the verdict)"); return -1; }
    PitchStatsArgs a;
    a.f0 = d_f0; a.ld_frames = ld_frames; a.frames = d_frames; a.B = B; a.tail = tail_frames; a.out = d_out_hz; a.counts = d_counts;
    a.status = static_cast<int64_t*>(d_ws);
    HIP_OK(launch_pitch_stats(a, static_cast<hipStream_t>(stream)));
    return 0;
}

int mtts_pitch_candidates(const float* d_audio, int64_t ld, const int64_t* d_lengths, int B, int sample_rate, int hop, double fmin, double fmax,
                          double threshold, float* d_period, float* d_mass, float* d_depth, int32_t* d_count, float* d_unvoiced_mass,
                          float* d_floor, int64_t ld_frames, int64_t* d_frames, void* d_ws, int64_t ws_bytes, void* stream) {
    if (!d_audio || !d_lengths || !d_period || !d_mass || !d_depth || !d_count || !d_unvoiced_mass || !d_floor || !d_frames || !d_ws) {
        set_error("mtts_pitch_candidates: null argument");
        return -1;
    }
    if (B < 1 || B > 65535) { set_error("mtts_pitch_candidates: B must lie in [1, 65535]"); return -1; }
    if (ld < 4 || (ld & 3) || (reinterpret_cast<uintptr_t>(d_audio) & 15) || (reinterpret_cast<uintptr_t>(d_ws) & 15)) {
        set_error("mtts_pitch_candidates: rows must be 16-byte aligned (ld a positive multiple of 4 samples)");
        return -1;
    }
    PitchArgs a;
    PitchCandArgs o;
    int window;
    if (!pitch_plan("mtts_pitch_candidates", sample_rate, hop, fmin, fmax, &window, &a.tmin, &a.tmax)) return -1;
    if (!(threshold > 0.0) || !(threshold < 1.0)) { set_error("mtts_pitch_candidates: threshold must lie in (0, 1)"); return -1; }
    const int64_t n_max = pitch_frames(ld, hop, a.tmax);
    if (ld_frames < 1 || ld_frames < n_max) {
        set_error("mtts_pitch_candidates: ld_frames = " + std::to_string(ld_frames) + " is less than the " + std::to_string(std::max<int64_t>(n_max, 1)) +
                  " frames a row of ld samples can have");
        return -1;
    }
    if (ld_frames > 0x3fffffff) { set_error("mtts_pitch_candidates: too many frames in a row"); return -1; }
    WS ws(d_ws, (size_t)ws_bytes);
    pitch_carve(ws, B, ld, hop, a.tmax, &a);
    if (ws_bytes < 256 || ws.overflow) { set_error("mtts_pitch_candidates: workspace too small (mtts_pitch_workspace_bytes)"); return -1; }
    a.audio = d_audio; a.ld = ld; a.lengths = d_lengths; a.B = B; a.H = hop;
    a.thr = (float)threshold; a.fs = (float)sample_rate;
    a.ld_frames = ld_frames; a.frames = d_frames;
    o.period = d_period; o.mass = d_mass; o.depth = d_depth; o.count = d_count; o.unvoiced = d_unvoiced_mass; o.floor = d_floor;
    HIP_OK(launch_pitch_candidates(a, o, static_cast<hipStream_t>(stream)));
    return 0;
}

int64_t mtts_pitch_viterbi_workspace_bytes(int64_t ld_frames, int B) {
    if (ld_frames < 1 || ld_frames > 0x3fffffff || B < 1 || B > 65535) { set_error("mtts_pitch_viterbi_workspace_bytes: bad shape"); return -1; }
    return 256 + (int64_t)B * ld_frames * 8 + 256;
}

int mtts_pitch_viterbi(const float* d_period, const float* d_mass, const float* d_depth, const int32_t* d_count, const float* d_unvoiced_mass,
                       const float* d_floor, int64_t ld_frames, const int64_t* d_frames, int B, int sample_rate, double jump, double switch_cost,
                       float* d_f0, float* d_aper, int8_t* d_state, void* d_ws, int64_t ws_bytes, void* stream) {
    if (!d_period || !d_mass || !d_depth || !d_count || !d_unvoiced_mass || !d_floor || !d_frames || !d_f0 || !d_aper || !d_state || !d_ws) {
        set_error("mtts_pitch_viterbi: null argument");
        return -1;
    }
    if (B < 1 || B > 65535) { set_error("mtts_pitch_viterbi: B must lie in [1, 65535]"); return -1; }
    if (ld_frames < 1 || ld_frames > 0x3fffffff) { set_error("mtts_pitch_viterbi: ld_frames must lie in [1, 2^30)"); return -1; }
    if (sample_rate < 8000 || sample_rate > 48000) { set_error("mtts_pitch_viterbi: sample_rate must lie in [8000, 48000]"); return -1; }
    if (!(jump >= 0.0) || !(jump <= 1e6) || !(switch_cost >= 0.0) || !(switch_cost <= 1e6)) {
        set_error("mtts_pitch_viterbi: jump and switch must lie in [0, 1e6]");
        return -1;
    }
    if (reinterpret_cast<uintptr_t>(d_ws) & 15) { set_error("mtts_pitch_viterbi: misaligned workspace (16 bytes)"); return -1; }
    if (ws_bytes < 256 + (int64_t)B * ld_frames * 8) { set_error("mtts_pitch_viterbi: workspace too small (mtts_pitch_viterbi_workspace_bytes)"); return -1; }
    PitchPathArgs a;
    a.period = d_period; a.mass = d_mass; a.depth = d_depth; a.count = d_count; a.unvoiced = d_unvoiced_mass; a.floor = d_floor;
    a.ld_frames = ld_frames; a.frames = d_frames; a.B = B;
    a.fs = (float)sample_rate; a.jump = (float)jump; a.sw = (float)switch_cost;
    a.f0 = d_f0; a.aper = d_aper; a.state = reinterpret_cast<signed char*>(d_state);
    a.status = static_cast<int64_t*>(d_ws);
    a.back = reinterpret_cast<unsigned long long*>(static_cast<char*>(d_ws) + 256);
    HIP_OK(launch_pitch_viterbi(a, static_cast<hipStream_t>(stream)));
    return 0;
}

int mtts_pitch_fold(const float* d_f0, int64_t ld_frames, const int64_t* d_frames, int B, int hop, int window, int max_lag,
                    const int64_t* d_marks, int Tx, const int64_t* d_x_lengths, const float* d_audio, int64_t ld, const int64_t* d_lengths,
                    int32_t* d_counts, float* d_hz, double* d_mean_square, void* d_ws, int64_t ws_bytes, void* stream) {
    if (!d_f0 || !d_frames || !d_marks || !d_x_lengths || !d_counts || !d_hz || !d_ws) { set_error("mtts_pitch_fold: null argument"); return -1; }
    if (B < 1 || B > 65535) { set_error("mtts_pitch_fold: B must lie in [1, 65535]"); return -1; }
    if (Tx < 1 || Tx > (1 << 20)) { set_error("mtts_pitch_fold: Tx must lie in [1, 2^20]"); return -1; }
    if (ld_frames < 1 || ld_frames > 0x3fffffff) { set_error("mtts_pitch_fold: ld_frames must lie in [1, 2^30)"); return -1; }
    if (hop < 8 || hop > PITCH_MAX_HOP || window != 8 * hop || max_lag < 4 || max_lag > MTTS_PITCH_MAX_LAG) {
        set_error("mtts_pitch_fold: (hop, window, max_lag) must be a plan of mtts_pitch_plan: hop in [8, 512], window = 8 hop, max_lag in [4, 1024]");
        return -1;
    }
    if ((d_audio != nullptr) != (d_mean_square != nullptr)) { set_error("mtts_pitch_fold: d_audio and d_mean_square go together"); return -1; }
    if (d_audio && (!d_lengths || ld < 1)) { set_error("mtts_pitch_fold: audio needs its lengths and ld >= 1"); return -1; }
    if (reinterpret_cast<uintptr_t>(d_ws) & 15) { set_error("mtts_pitch_fold: misaligned workspace (16 bytes)"); return -1; }
    if (ws_bytes < 256) { set_error("mtts_pitch_fold: workspace too small (256 bytes: the verdict)"); return -1; }
    PitchFoldArgs a;
    a.f0 = d_f0; a.ld_frames = ld_frames; a.frames = d_frames; a.B = B; a.Tx = Tx; a.H = hop; a.centre = (int64_t)window + max_lag;
    a.marks = d_marks; a.x_lengths = d_x_lengths; a.audio = d_audio; a.ld = ld; a.lengths = d_lengths;
    a.counts = d_counts; a.hz = d_hz; a.mean_square = d_mean_square; a.status = static_cast<int64_t*>(d_ws);
    HIP_OK(launch_pitch_fold(a, static_cast<hipStream_t>(stream)));
    return 0;
}

// The verdict of the latest mtts_pitch_* call on this workspace.  Waits for the stream.
int mtts_pitch_status(const void* d_ws, void* stream) {
    int64_t st[5];
    if (read_status("mtts_pitch_status", d_ws, stream, st)) return -1;
    if (st[0] == 0) return 0;
    const std::string row = "row " + std::to_string(st[0] - 1);
    if (st[4] == 5) {
        static const char* const why[] = {"", "has a frame count outside [0, ld_frames]", "has an x_length outside [0, Tx]", "has a length outside [0, ld]",
                                          "has a mark outside [0, length]", "has a token with start > end", "has marks that do not ascend"};
        set_error("mtts_pitch_fold: " + row + " " + why[st[1] >= 1 && st[1] <= 6 ? st[1] : 0]);
    } else if (st[4] == 2 || st[4] == 4) {
        set_error(std::string(st[4] == 2 ? "mtts_pitch_stats: " : "mtts_pitch_viterbi: ") + row + " has " + std::to_string(st[1]) +
                  " frames (need 0 <= frames <= ld_frames = " + std::to_string(st[2]) + ")");
    } else {
        set_error(std::string(st[4] == 3 ? "mtts_pitch_candidates: " : "mtts_pitch_track: ") + row + " has length " + std::to_string(st[1]) +
                  " (need 0 <= length <= ld = " + std::to_string(st[2]) + ")");
    }
    return -1;
}

}  // extern "C"
