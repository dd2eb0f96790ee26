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
        if (live) {
            const size_t at = (size_t)row * p.nblk_max + k;
            const float* Sb = p.S + at * p.ldt;
            for (int bb = 0; bb < 8; ++bb) bad |= p.flag[at + bb] != 0;
            // d(tau) = ((((((s_k + s_k+1) + s_k+2) + s_k+3) + s_k+4) + s_k+5) + s_k+6) + s_k+7
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int idx = 16 * lane + 4 * q;
                f32x4 v = {0.f, 0.f, 0.f, 0.f};
                if (idx < tmax) {                                 // (idx + 3 < ldt: ldt is tmax rounded up to 4)
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
        }
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

// The verdict of the latest mtts_pitch_track / mtts_pitch_stats call on this workspace.  Waits for the stream.
int mtts_pitch_status(const void* d_ws, void* stream) {
    int64_t st[5];
    if (read_status("mtts_pitch_status", d_ws, stream, st)) return -1;
    if (st[0] == 0) return 0;
    const std::string row = "row " + std::to_string(st[0] - 1);
    if (st[4] == 2) set_error("mtts_pitch_stats: " + row + " has " + std::to_string(st[1]) + " frames (need 0 <= frames <= ld_frames = " + std::to_string(st[2]) + ")");
    else set_error("mtts_pitch_track: " + row + " has length " + std::to_string(st[1]) + " (need 0 <= length <= ld = " + std::to_string(st[2]) + ")");
    return -1;
}

}  // extern "C"
