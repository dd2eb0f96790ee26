// Integrated loudness of a ragged batch (gfx950): ITU-R BS.1770 K-weighting, 400 ms blocks at 75 % overlap, the absolute and the
// relative gate, then one gain per row towards a target in LUFS -- include/mtts.h "loudness" has the arithmetic, which
// tests/loudness_restated.py restates in NumPy fp64.  Five launches, none of which owns a row:
//   1. loud_chunk_kernel<false> (tile, row): lane l of a workgroup runs the two-biquad cascade (transposed direct form II, fp64) over
//                        chunk l of the tile from ZERO state and stores the four end-state words and the chunk's max |x|
//   2. loud_scan_kernel  (row): s[c + 1] = M s[c] + z[c] along the row, M = A^chunk built on the host in fp64, as a two-level scan
//                        (runs of 32 chunks per lane, P = M^32 across the lanes): the end states become the true entry states, in place
//   3. loud_chunk_kernel<true>: the same walk from the true entry state, summing y * y in sample order -> energy[row][chunk]
//   4. loud_gate_kernel  (row): the row's peak, the 100 ms segments (chunks added in index order), the blocks (4 consecutive
//                        segments), the two gates, L and the gain; workgroup 0 also writes the verdict of the ragged-batch contract
//   5. loud_apply_kernel (tile, row): x = x * g on the rows with g != 1, inside [0, len_b)
// The recurrence is cut in time because a row can be 1.8 M samples with B = 1.  A lane walks its own chunk, so the samples go through
// LDS: the workgroup loads LOUD_SLAB samples of each of its 256 chunks at a time (a wave's load instruction covers two runs of 128
// contiguous bytes), rows padded to LOUD_SLAB + 1 words so that the 32 lanes of a bank group read 32 different banks.  The next
// slab's loads are issued before the current slab is walked.
// State and sums are fp64: an fp32 recurrence is off by 1.4e-5 on a signal of rms 0.09, the fp64 one by 2e-13.
// Every sum has an order that is a function of the row's length alone: not of B, ld, the grid or the row's position.
// mtts_loudness_r128 runs the same passes with two more kernels: loud_true_peak_kernel (tile, row) between 3 and 4, and
// loud_gate_r128_kernel in place of 4, which adds the true peak, the maximum momentary and short-term loudness, the loudness range
// and a true-peak ceiling on the gain.  The true peak is a maximum, which has no order: batch independence follows for free.
#include "host.h"
#include "device_utils.h"

#include <cmath>

namespace mtts {

using f32x4 = __attribute__((ext_vector_type(4))) float;

constexpr int LOUD_THREADS = MTTS_LOUDNESS_CHUNKS;      // chunks per workgroup = lanes
constexpr int LOUD_SLAB = 32;                           // samples of each chunk staged at once
constexpr int LOUD_PITCH = LOUD_SLAB + 1;               // words per staged chunk (bank = (l + t) % 32 for lane l)
constexpr int LOUD_CHUNK_MAX = 256;
constexpr int LOUD_SCAN_RUN = MTTS_LOUDNESS_SCAN_RUN;   // consecutive chunks a lane of the scan owns
constexpr int LOUD_APPLY_TILE = 4096;                   // samples per workgroup of the apply pass
constexpr int TP_TILE = MTTS_TRUE_PEAK_TILE;            // samples per workgroup of the true-peak pass
constexpr int TP_TAPS = MTTS_TRUE_PEAK_TAPS;            // taps per phase of the interpolator: half-width 6 input samples
constexpr int TP_FACTOR_MAX = 8;                        // the largest oversampling factor
static_assert(TP_TILE % 1024 == 0 && TP_TAPS == 12, "the true-peak pass stages whole quads and a halo of 5 + 6 samples");
static_assert(LOUD_THREADS == 256 && (LOUD_THREADS * LOUD_SLAB) % LOUD_THREADS == 0, "the slab loader assumes 256 lanes");

struct LoudArgs {
    float* audio;                // [B][ld]
    const int64_t* lengths;      // [B]
    const float* target;         // [B] or null
    int64_t ld;
    int B, chunk, cps;           // samples per chunk; chunks per 100 ms segment
    int64_t nchunk, nseg;        // row strides of the per-chunk and per-segment arrays
    double k[10];                // shelf b0 b1 b2 a1 a2, high-pass b0 b1 b2 a1 a2
    double M[16];                // A^chunk, row-major
    double P[16];                // A^(chunk * LOUD_SCAN_RUN)
    float ceiling;
    double* state;               // [B][nchunk][4]
    double* energy;              // [B][nchunk]
    float* cpeak;                // [B][nchunk]
    double* seg;                 // [B][nseg]
    double* lufs;                // [B]
    float* gain;                 // [B]
    float* peak;                 // [B]
    int64_t* status;             // header of the workspace
};

// One sample through the cascade: every operation rounded once (no FMA: the build has -ffp-contract=off)
__host__ __device__ __forceinline__ double loud_step(const double* k, double x, double& s1, double& s2, double& t1, double& t2) {
    const double y = k[0] * x + s1;
    s1 = (k[1] * x - k[3] * y) + s2;
    s2 = k[2] * x - k[4] * y;
    const double z = k[5] * y + t1;
    t1 = (k[6] * y - k[8] * z) + t2;
    t2 = k[7] * y - k[9] * z;
    return z;
}

template <bool ENERGY>
__global__ __launch_bounds__(LOUD_THREADS) void loud_chunk_kernel(const LoudArgs a) {
    __shared__ float s_x[LOUD_THREADS * LOUD_PITCH];
    const int tid = threadIdx.x, b = blockIdx.y;
    const int64_t len = a.lengths[b];
    if (len < 0 || len > a.ld) return;                                 // workgroup-uniform: a refused row is not read
    const int C = a.chunk;
    const int64_t j0 = (int64_t)blockIdx.x * LOUD_THREADS * C;
    if (j0 >= len) return;                                             // workgroup-uniform
    const float* row = a.audio + (size_t)b * a.ld;
    const int64_t c = (int64_t)blockIdx.x * LOUD_THREADS + tid;        // this lane's chunk
    const int64_t left = len - c * C;
    const int n = left <= 0 ? 0 : (left < C ? (int)left : C);          // its samples inside the row
    double k[10];
#pragma unroll
    for (int i = 0; i < 10; ++i) k[i] = a.k[i];
    double s1 = 0.0, s2 = 0.0, t1 = 0.0, t2 = 0.0, e = 0.0;
    if (ENERGY && n > 0) {
        const double* st = a.state + ((size_t)b * a.nchunk + c) * 4;
        s1 = st[0]; s2 = st[1]; t1 = st[2]; t2 = st[3];
    }
    float pk = 0.f;
    // element q of a slab: chunk q / SLAB of the tile, sample q % SLAB of the slab; this lane loads q = tid + 256 i
    float r[LOUD_SLAB];
    auto fetch = [&](int t0) {
#pragma unroll
        for (int i = 0; i < LOUD_SLAB; ++i) {
            const int q = tid + LOUD_THREADS * i;
            const int t = t0 + (q & (LOUD_SLAB - 1));
            const int64_t j = j0 + (int64_t)(q / LOUD_SLAB) * C + t;
            r[i] = (t < C && j < len) ? row[j] : 0.f;
        }
    };
    fetch(0);
    for (int t0 = 0; t0 < C; t0 += LOUD_SLAB) {
        __syncthreads();                                               // the previous slab has been walked
#pragma unroll
        for (int i = 0; i < LOUD_SLAB; ++i) {
            const int q = tid + LOUD_THREADS * i;
            s_x[(q / LOUD_SLAB) * LOUD_PITCH + (q & (LOUD_SLAB - 1))] = r[i];
        }
        __syncthreads();
        if (t0 + LOUD_SLAB < C) fetch(t0 + LOUD_SLAB);                 // in flight while this slab is walked
        const int m = n - t0 < LOUD_SLAB ? n - t0 : LOUD_SLAB;
        for (int t = 0; t < m; ++t) {
            const float xf = s_x[tid * LOUD_PITCH + t];
            const double z = loud_step(k, (double)xf, s1, s2, t1, t2);
            if (ENERGY) e = e + z * z;
            else pk = fmaxf(pk, fabsf(xf));
        }
    }
    if (n <= 0) return;
    if (ENERGY) {
        a.energy[(size_t)b * a.nchunk + c] = e;
    } else {
        double* st = a.state + ((size_t)b * a.nchunk + c) * 4;
        st[0] = s1; st[1] = s2; st[2] = t1; st[3] = t2;
        a.cpeak[(size_t)b * a.nchunk + c] = pk;
    }
}

// s' = X s + z, each row of X s as ((X0 s0 + X1 s1) + X2 s2) + X3 s3, then + z
__device__ __forceinline__ void loud_affine(const double* X, double* s, const double* z) {
    double nx[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) nx[i] = (((X[4 * i] * s[0] + X[4 * i + 1] * s[1]) + X[4 * i + 2] * s[2]) + X[4 * i + 3] * s[3]) + z[i];
#pragma unroll
    for (int i = 0; i < 4; ++i) s[i] = nx[i];
}

// One wave per row, LOUD_SCAN_RUN * 64 chunks at a time, in three phases (a plain walk along the row is 7500 dependent steps on the
// long row; this takes 128 steps per 2048 chunks: profiles/r19_loudness.md):
//   A  lane l folds its run of LOUD_SCAN_RUN consecutive chunks from zero state: w = M w + z_c, c ascending (a chunk at or beyond
//      the row's end counts as z = 0)
//   B  every lane walks the 64 runs in order with P = M^LOUD_SCAN_RUN: S_{l+1} = P S_l + w_l (w from LDS, which broadcasts) and
//      keeps S_l, the state its own run is entered with; S_64 is carried into the next 64 runs
//   C  lane l walks its run again from S_l: chunk c is entered with s, then s = M s + z_c; the entry states replace the z_c
__global__ __launch_bounds__(64) void loud_scan_kernel(const LoudArgs a) {
    __shared__ double s_w[64 * 4];
    const int lane = threadIdx.x, b = blockIdx.x;
    const int64_t len = a.lengths[b];
    if (len < 0 || len > a.ld) return;
    const int64_t nc = (len + a.chunk - 1) / a.chunk;
    double* st = a.state + (size_t)b * a.nchunk * 4;
    double M[16], P[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) { M[i] = a.M[i]; P[i] = a.P[i]; }
    double carry[4] = {0.0, 0.0, 0.0, 0.0};
    for (int64_t c0 = 0; c0 < nc; c0 += 64 * LOUD_SCAN_RUN) {
        const int64_t base = c0 + (int64_t)lane * LOUD_SCAN_RUN;
        double w[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll 8
        for (int i = 0; i < LOUD_SCAN_RUN; ++i) {
            const int64_t c = base + i;
            double z[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) z[e] = c < nc ? st[c * 4 + e] : 0.0;
            loud_affine(M, w, z);
        }
        __syncthreads();                                               // the previous round's s_w has been read
#pragma unroll
        for (int e = 0; e < 4; ++e) s_w[lane * 4 + e] = w[e];
        __syncthreads();
        double s[4], mine[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int e = 0; e < 4; ++e) s[e] = carry[e];
        for (int l = 0; l < 64; ++l) {
            if (l == lane) {
#pragma unroll
                for (int e = 0; e < 4; ++e) mine[e] = s[e];
            }
            loud_affine(P, s, &s_w[l * 4]);
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) { carry[e] = s[e]; s[e] = mine[e]; }
#pragma unroll 8
        for (int i = 0; i < LOUD_SCAN_RUN; ++i) {
            const int64_t c = base + i;
            if (c < nc) {
                double z[4];
#pragma unroll
                for (int e = 0; e < 4; ++e) { z[e] = st[c * 4 + e]; st[c * 4 + e] = s[e]; }
                loud_affine(M, s, z);
            }
        }
    }
}

__device__ __forceinline__ double loud_db(double ms) { return -0.691 + 10.0 * log10(ms); }

// (sum, count) over the 256 threads in a fixed shape: v[t] = v[t] + v[t + o], o = 128 .. 1; every thread gets the total
__device__ __forceinline__ void loud_reduce(double* s_v, double* s_n, int tid, double& v, double& n) {
    __syncthreads();
    s_v[tid] = v; s_n[tid] = n;
    __syncthreads();
    for (int o = LOUD_THREADS / 2; o > 0; o >>= 1) {
        if (tid < o) { s_v[tid] = s_v[tid] + s_v[tid + o]; s_n[tid] = s_n[tid] + s_n[tid + o]; }
        __syncthreads();
    }
    v = s_v[0]; n = s_n[0];
}

// What both gate kernels compute of a row in [0, ld]: the sample peak, the 100 ms segments (stored to seg[]) and the integrated
// loudness L.  `l_one`: the loudness of the single block a row under 400 ms is (thread 0 alone has it, as it alone has that row's L).
__device__ __forceinline__ void loud_integrated(const LoudArgs& a, int b, int64_t len, double* s_v, double* s_n, float* s_p, float& pk, double& L,
                                                double& l_one) {
    const int tid = threadIdx.x;
    const int C = a.chunk;
    const int64_t nc = (len + C - 1) / C;
    const int64_t seg_len = (int64_t)a.cps * C;                        // samples of 100 ms
    const int64_t nfull = len / seg_len;                               // whole segments; a partial trailing one is in no block
    const double* en = a.energy + (size_t)b * a.nchunk;
    const float* cp = a.cpeak + (size_t)b * a.nchunk;
    double* seg = a.seg + (size_t)b * a.nseg;
    pk = 0.f;
    for (int64_t c = tid; c < nc; c += LOUD_THREADS) pk = fmaxf(pk, cp[c]);
    s_p[tid] = pk;
    __syncthreads();
    for (int o = LOUD_THREADS / 2; o > 0; o >>= 1) {
        if (tid < o) s_p[tid] = fmaxf(s_p[tid], s_p[tid + o]);
        __syncthreads();
    }
    pk = s_p[0];
    L = -INFINITY;
    l_one = -INFINITY;
    if (nfull >= 4) {
        for (int64_t k = tid; k < nfull; k += LOUD_THREADS) {
            double v = 0.0;
            for (int i = 0; i < a.cps; ++i) v = v + en[k * a.cps + i];
            seg[k] = v;
        }
        __syncthreads();                                               // this workgroup's own stores
        const int64_t nblk = nfull - 3;
        const double inv = 1.0 / (4.0 * (double)seg_len);
        double gate = -INFINITY;
        for (int round = 0; round < 2; ++round) {
            double v = 0.0, n = 0.0;
            for (int64_t j = tid; j < nblk; j += LOUD_THREADS) {
                const double ms = (((seg[j] + seg[j + 1]) + seg[j + 2]) + seg[j + 3]) * inv;
                const double l = loud_db(ms);
                if (l > -70.0 && l > gate) { v = v + ms; n = n + 1.0; }
            }
            loud_reduce(s_v, s_n, tid, v, n);
            L = n > 0.0 ? loud_db(v / n) : -INFINITY;
            gate = L - 10.0;
        }
    } else if (len > 0 && tid == 0) {
        // shorter than one block: one block of the row's own length (a deviation from BS.1770; the absolute gate applies).
        // Thread 0, which alone uses L below, adds the row's few chunks in index order
        double v = 0.0;
        for (int64_t c = 0; c < nc; ++c) v = v + en[c];
        l_one = loud_db(v / (double)len);
        L = l_one > -70.0 ? l_one : -INFINITY;
    }
}

// The gain of a row: towards the target, then the sample-peak ceiling, then (c_tp not NaN) the true-peak ceiling
__device__ __forceinline__ float loud_gain(float tg, double L, int64_t len, float pk, float ceiling, float tp, float c_tp) {
    float g = 1.0f;
    if (len > 0 && tg == tg && L - L == 0.0) {                         // (L - L == 0: L is finite)
        g = (float)pow(10.0, ((double)tg - L) / 20.0);
        if (pk * g > ceiling) {
            g = ceiling / pk;
            for (int i = 0; i < 4 && pk * g > ceiling; ++i) g = __uint_as_float(__float_as_uint(g) - 1u);
        }
        if (c_tp == c_tp && tp * g > c_tp) {
            g = c_tp / tp;
            for (int i = 0; i < 4 && tp * g > c_tp; ++i) g = __uint_as_float(__float_as_uint(g) - 1u);
        }
        if (!(g - g == 0.0f)) g = 1.0f;
    }
    return g;
}

// The verdict of the ragged-batch contract, by workgroup 0 of a gate kernel
__device__ __forceinline__ void loud_verdict(const LoudArgs& a) {
    const int i = first_refused_row(a.B, [&](int r) { const int64_t n = a.lengths[r]; return n < 0 || n > a.ld; });
    if (threadIdx.x == 0) {
        a.status[0] = i < a.B ? i + 1 : 0;
        a.status[1] = i < a.B ? sat32(a.lengths[i]) : 0;
        a.status[2] = a.ld;
    }
}

__global__ __launch_bounds__(LOUD_THREADS) void loud_gate_kernel(const LoudArgs a) {
    __shared__ double s_v[LOUD_THREADS], s_n[LOUD_THREADS];
    __shared__ float s_p[LOUD_THREADS];
    const int tid = threadIdx.x, b = blockIdx.x;
    const int64_t len = a.lengths[b];
    const bool ok = len >= 0 && len <= a.ld;                           // workgroup-uniform
    if (ok) {
        float pk;
        double L, l_one;
        loud_integrated(a, b, len, s_v, s_n, s_p, pk, L, l_one);
        if (tid == 0) {
            a.lufs[b] = L;
            a.gain[b] = loud_gain(a.target ? a.target[b] : NAN, L, len, pk, a.ceiling, 0.f, NAN);
            a.peak[b] = pk;
        }
    } else if (tid == 0) {
        a.lufs[b] = NAN;
        a.gain[b] = 1.0f;
        a.peak[b] = 0.f;
    }
    if (blockIdx.x == 0) loud_verdict(a);
}

// ------------------------------------------------------------------------------------------------ true peak, loudness range
// True peak (include/mtts.h): the row at F times its rate through a 12-tap Hann-windowed sinc per phase, fp32, each product rounded
// and added in ascending tap order.  (tile, row): a workgroup stages TP_TILE samples and a halo of 5 before and 6 behind (8 and 8
// as staged: whole 16-byte quads) in LDS, zeros outside [0, len_b); lane l takes the samples l, l + 256, ... of the tile, so a wave's
// twelve LDS reads per sample are 64 consecutive words each.  One float per workgroup.  A maximum has no order: the row's true peak
// does not depend on B, ld, the grid or the tile.
struct R128Args {
    LoudArgs a;
    float h[(TP_FACTOR_MAX - 1) * TP_TAPS];  // phases 1 .. F - 1
    float c_tp;                  // linear true-peak ceiling, NaN: none
    int64_t ntp;                 // row stride of tpeak
    float* tpeak;                // [B][ntp]
    unsigned long long* st;      // [B][nseg]: the short-term mean squares, then their selection keys
    float* true_peak;            // [B]
    double *lra, *mmax, *smax;   // [B]
};

template <int F>
__global__ __launch_bounds__(256) void loud_true_peak_kernel(const R128Args r) {
    __shared__ __attribute__((aligned(16))) float s_x[TP_TILE + 16];   // s_x[i] = x[j0 - 8 + i]
    __shared__ float s_p[256];
    const int tid = threadIdx.x, b = blockIdx.y;
    const int64_t len = r.a.lengths[b];
    if (len < 0 || len > r.a.ld) return;                               // workgroup-uniform: a refused row is not read
    const int64_t j0 = (int64_t)blockIdx.x * TP_TILE;
    if (j0 >= len) return;                                             // workgroup-uniform
    const float* row = r.a.audio + (size_t)b * r.a.ld;
    for (int q = tid; q < (TP_TILE + 16) / 4; q += 256) {
        const int64_t j = j0 - 8 + 4 * q;
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (j >= 0 && j + 4 <= len) {
            v = *reinterpret_cast<const f32x4*>(row + j);
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (j + e >= 0 && j + e < len) v[e] = row[j + e];
        }
        *reinterpret_cast<f32x4*>(s_x + 4 * q) = v;
    }
    __syncthreads();
    float pk = 0.f;
#pragma unroll 2
    for (int i = 0; i < TP_TILE / 256; ++i) {
        const int t = tid + 256 * i;
        if (j0 + t >= len) break;
        float w[TP_TAPS];
#pragma unroll
        for (int k = 0; k < TP_TAPS; ++k) w[k] = s_x[8 + t - 5 + k];
        pk = fmaxf(pk, fabsf(w[5]));
#pragma unroll
        for (int p = 1; p < F; ++p) {
            float acc = 0.0f;
#pragma unroll
            for (int k = 0; k < TP_TAPS; ++k) acc = acc + r.h[(p - 1) * TP_TAPS + k] * w[k];
            pk = fmaxf(pk, fabsf(acc));
        }
    }
    s_p[tid] = pk;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (tid < o) s_p[tid] = fmaxf(s_p[tid], s_p[tid + o]);
        __syncthreads();
    }
    if (tid == 0) r.tpeak[(size_t)b * r.ntp + blockIdx.x] = s_p[0];
}

// max over the 256 threads (NaN passed over); every thread gets it
__device__ __forceinline__ double loud_reduce_max(double* s_v, int tid, double v) {
    __syncthreads();
    s_v[tid] = v;
    __syncthreads();
    for (int o = LOUD_THREADS / 2; o > 0; o >>= 1) {
        if (tid < o) s_v[tid] = fmax(s_v[tid], s_v[tid + o]);
        __syncthreads();
    }
    return s_v[0];
}

// loud_gate_kernel and, from the same seg[]: the row's true peak (the maximum of its tiles'), the maximum momentary and short-term
// loudness and the loudness range (EBU Tech 3342).  The two order statistics of the range are exact: a radix select on the bit
// patterns of the non-negative doubles, most significant byte first, 8 passes of two 256-bin LDS histograms (one per rank) by this
// row's workgroup.  Counts are integers, so the result is a function of the row's blocks alone.
__global__ __launch_bounds__(LOUD_THREADS) void loud_gate_r128_kernel(const R128Args r) {
    __shared__ double s_v[LOUD_THREADS], s_n[LOUD_THREADS];
    __shared__ float s_p[LOUD_THREADS];
    __shared__ unsigned s_hist[2][256], s_wsum[2][LOUD_THREADS / 64];
    __shared__ unsigned long long s_pre[2];
    __shared__ unsigned long long s_rank[2];
    const LoudArgs& a = r.a;
    const int tid = threadIdx.x, b = blockIdx.x;
    const int64_t len = a.lengths[b];
    const bool ok = len >= 0 && len <= a.ld;                           // workgroup-uniform
    if (ok) {
        float pk;
        double L, l_one;
        loud_integrated(a, b, len, s_v, s_n, s_p, pk, L, l_one);
        // the true peak: one float per tile of the true-peak pass
        const int64_t nt = (len + TP_TILE - 1) / TP_TILE;
        const float* tpk = r.tpeak + (size_t)b * r.ntp;
        float tp = 0.f;
        for (int64_t t = tid; t < nt; t += LOUD_THREADS) tp = fmaxf(tp, tpk[t]);
        __syncthreads();
        s_p[tid] = tp;
        __syncthreads();
        for (int o = LOUD_THREADS / 2; o > 0; o >>= 1) {
            if (tid < o) s_p[tid] = fmaxf(s_p[tid], s_p[tid + o]);
            __syncthreads();
        }
        tp = s_p[0];
        const int64_t seg_len = (int64_t)a.cps * a.chunk;
        const int64_t nfull = len / seg_len;
        const double* seg = a.seg + (size_t)b * a.nseg;
        // maximum momentary loudness: ungated, over the 400 ms blocks (log10 is monotone: the loudest block has the largest ms)
        double mmax = l_one;
        if (nfull >= 4) {
            const double inv = 1.0 / (4.0 * (double)seg_len);
            double mx = 0.0;
            for (int64_t j = tid; j < nfull - 3; j += LOUD_THREADS) mx = fmax(mx, (((seg[j] + seg[j + 1]) + seg[j + 2]) + seg[j + 3]) * inv);
            mmax = loud_db(loud_reduce_max(s_v, tid, mx));
        }
        double smax = -INFINITY, lra = 0.0;
        if (nfull >= 30) {
            unsigned long long* key = r.st + (size_t)b * a.nseg;
            const int64_t n3 = nfull - 29;
            const double den = 30.0 * (double)seg_len;
            double v = 0.0, n = 0.0, mx = 0.0;
            for (int64_t k = tid; k < n3; k += LOUD_THREADS) {
                double S = 0.0;
                for (int i = 0; i < 30; ++i) S = S + seg[k + i];
                const double ms = S / den;
                key[k] = (unsigned long long)__double_as_longlong(ms);
                mx = fmax(mx, ms);
                if (loud_db(ms) > -70.0) { v = v + ms; n = n + 1.0; }
            }
            loud_reduce(s_v, s_n, tid, v, n);
            const double gate = n > 0.0 ? loud_db(v / n) - 20.0 : INFINITY;
            smax = loud_db(loud_reduce_max(s_v, tid, mx));
            // the blocks above both gates keep their bits as keys; the others sort behind every one of them
            v = 0.0; n = 0.0;
            for (int64_t k = tid; k < n3; k += LOUD_THREADS) {
                const double l = loud_db(__longlong_as_double((long long)key[k]));
                if (l > -70.0 && l > gate) n = n + 1.0;
                else key[k] = ~0ull;
            }
            loud_reduce(s_v, s_n, tid, v, n);                          // (also orders the keys ahead of the passes below)
            const int64_t nq = (int64_t)n;
            if (nq > 0) {
                if (tid < 2) {
                    s_pre[tid] = 0ull;
                    s_rank[tid] = (unsigned long long)(((tid == 0 ? 10 : 95) * (nq - 1) + 50) / 100);
                }
                for (int pass = 0; pass < 8; ++pass) {
                    const int shift = 56 - 8 * pass;
                    s_hist[0][tid] = 0u; s_hist[1][tid] = 0u;
                    __syncthreads();
                    const unsigned long long p0 = s_pre[0], p1 = s_pre[1], r0 = s_rank[0], r1 = s_rank[1];
                    for (int64_t k = tid; k < n3; k += LOUD_THREADS) {
                        const unsigned long long u = key[k];
                        const unsigned long long hi = pass == 0 ? 0ull : u >> (shift + 8);
                        const unsigned d = (unsigned)(u >> shift) & 255u;
                        if (hi == p0) atomicAdd(&s_hist[0][d], 1u);
                        if (hi == p1) atomicAdd(&s_hist[1][d], 1u);
                    }
                    __syncthreads();
                    // thread d owns bin d: an inclusive scan of the counts inside each wave, then the totals of the waves before it;
                    // the one bin whose [exclusive, inclusive) holds the rank is the next byte, and the rank inside it is carried on
                    const unsigned c0 = s_hist[0][tid], c1 = s_hist[1][tid];
                    unsigned i0 = c0, i1 = c1;
                    for (int o = 1; o < 64; o <<= 1) {
                        const unsigned u0 = __shfl_up(i0, o, 64), u1 = __shfl_up(i1, o, 64);
                        if ((tid & 63) >= o) { i0 += u0; i1 += u1; }
                    }
                    if ((tid & 63) == 63) { s_wsum[0][tid >> 6] = i0; s_wsum[1][tid >> 6] = i1; }
                    __syncthreads();
                    for (int w = 0; w < (tid >> 6); ++w) { i0 += s_wsum[0][w]; i1 += s_wsum[1][w]; }
                    if (r0 >= i0 - c0 && r0 < i0) { s_rank[0] = r0 - (i0 - c0); s_pre[0] = (p0 << 8) | (unsigned long long)tid; }
                    if (r1 >= i1 - c1 && r1 < i1) { s_rank[1] = r1 - (i1 - c1); s_pre[1] = (p1 << 8) | (unsigned long long)tid; }
                }
                __syncthreads();
                lra = loud_db(__longlong_as_double((long long)s_pre[1])) - loud_db(__longlong_as_double((long long)s_pre[0]));
            }
        }
        if (tid == 0) {
            a.lufs[b] = L;
            a.gain[b] = loud_gain(a.target ? a.target[b] : NAN, L, len, pk, a.ceiling, tp, r.c_tp);
            a.peak[b] = pk;
            r.true_peak[b] = tp;
            r.lra[b] = lra;
            r.mmax[b] = mmax;
            r.smax[b] = smax;
        }
    } else if (tid == 0) {
        a.lufs[b] = NAN;
        a.gain[b] = 1.0f;
        a.peak[b] = 0.f;
        r.true_peak[b] = 0.f;
        r.lra[b] = NAN;
        r.mmax[b] = NAN;
        r.smax[b] = NAN;
    }
    if (blockIdx.x == 0) loud_verdict(a);
}

__global__ __launch_bounds__(256) void loud_apply_kernel(const LoudArgs a) {
    const int b = blockIdx.y, tid = threadIdx.x;
    const float g = a.gain[b];
    if (g == 1.0f) return;                                             // the row keeps its bits
    const int64_t len = a.lengths[b];
    if (len < 0 || len > a.ld) return;
    float* row = a.audio + (size_t)b * a.ld;
    const int64_t j0 = (int64_t)blockIdx.x * LOUD_APPLY_TILE;
#pragma unroll
    for (int q = 0; q < LOUD_APPLY_TILE / 1024; ++q) {
        const int64_t j = j0 + q * 1024 + 4 * tid;
        if (j >= len) continue;
        if (len - j >= 4) {
            f32x4 x = *reinterpret_cast<const f32x4*>(row + j);
#pragma unroll
            for (int e = 0; e < 4; ++e) x[e] = x[e] * g;
            *reinterpret_cast<f32x4*>(row + j) = x;
        } else {
            for (int e = 0; e < (int)(len - j); ++e) row[j + e] = row[j + e] * g;
        }
    }
}

// The chunk: the largest divisor of sample_rate / 100 that is at most LOUD_CHUNK_MAX, so chunk edges fall on 10 ms edges
static int loud_chunk(int sample_rate) {
    const int w = sample_rate / 100;
    for (int c = w < LOUD_CHUNK_MAX ? w : LOUD_CHUNK_MAX; c > 1; --c)
        if (w % c == 0) return c;
    return 1;
}
static bool loud_rate_ok(int sample_rate) { return sample_rate >= 8000 && sample_rate <= 192000 && sample_rate % 100 == 0; }

// K-weighting by the bilinear transform of the analog prototype (include/mtts.h), fp64: shelf b0 b1 b2 a1 a2, high-pass likewise
static void loud_coefficients(int sample_rate, double* k) {
    const double pi = 3.14159265358979323846, fs = (double)sample_rate;
    {
        const double f0 = 1681.974450955533, G = 3.999843853973347, Q = 0.7071752369554196;
        const double K = std::tan(pi * f0 / fs), Vh = std::pow(10.0, G / 20.0), Vb = std::pow(Vh, 0.4996667741545416);
        const double a0 = 1.0 + K / Q + K * K;
        k[0] = (Vh + Vb * K / Q + K * K) / a0;
        k[1] = 2.0 * (K * K - Vh) / a0;
        k[2] = (Vh - Vb * K / Q + K * K) / a0;
        k[3] = 2.0 * (K * K - 1.0) / a0;
        k[4] = (1.0 - K / Q + K * K) / a0;
    }
    {
        const double f0 = 38.13547087602444, Q = 0.5003270373238773;
        const double K = std::tan(pi * f0 / fs), a0 = 1.0 + K / Q + K * K;
        k[5] = 1.0; k[6] = -2.0; k[7] = 1.0;
        k[8] = 2.0 * (K * K - 1.0) / a0;
        k[9] = (1.0 - K / Q + K * K) / a0;
    }
}

struct LoudLayout { size_t status, state, energy, cpeak, seg, total; int64_t nchunk, nseg; int chunk, cps; };
static LoudLayout loud_layout(int64_t ld, int B, int sample_rate) {
    LoudLayout l;
    l.chunk = loud_chunk(sample_rate);
    l.cps = sample_rate / 10 / l.chunk;
    l.nchunk = (ld + l.chunk - 1) / l.chunk;
    l.nseg = ld / ((int64_t)l.cps * l.chunk) + 1;
    WS ws(nullptr, 0);
    ws.bytes(256);                                                         l.status = 0;
    ws.bytes((size_t)B * l.nchunk * 4 * sizeof(double));                   l.state = ws.off - (size_t)B * l.nchunk * 4 * sizeof(double);
    ws.bytes((size_t)B * l.nchunk * sizeof(double));                       l.energy = ws.off - (size_t)B * l.nchunk * sizeof(double);
    ws.bytes((size_t)B * l.nchunk * sizeof(float));                        l.cpeak = ws.off - (size_t)B * l.nchunk * sizeof(float);
    ws.bytes((size_t)B * l.nseg * sizeof(double));                         l.seg = ws.off - (size_t)B * l.nseg * sizeof(double);
    l.total = ws.off + 256;
    return l;
}

static int loud_shape_ok(const char* who, int64_t ld, int64_t B, int sample_rate) {
    if (B < 1 || B > 65535) { set_error(std::string(who) + ": B must lie in [1, 65535]"); return -1; }
    if (ld < 4 || (ld & 3)) { set_error(std::string(who) + ": rows must be 16-byte aligned (ld a positive multiple of 4 samples)"); return -1; }
    if (ld > (int64_t)1 << 30) { set_error(std::string(who) + ": rows longer than 2^30 samples"); return -1; }
    if (!loud_rate_ok(sample_rate)) { set_error(std::string(who) + ": sample_rate must be a multiple of 100 in [8000, 192000]"); return -1; }
    return 0;
}

// What the host can see of a call, shared by the two entries
static int loud_host_checks(const char* who, const float* d_audio, int64_t ld, int64_t B, int sample_rate, float peak_ceiling, const double* d_lufs,
                            const void* d_ws) {
    if (loud_shape_ok(who, ld, B, sample_rate)) return -1;
    if ((reinterpret_cast<uintptr_t>(d_audio) & 15) || (reinterpret_cast<uintptr_t>(d_ws) & 15) || (reinterpret_cast<uintptr_t>(d_lufs) & 7)) {
        set_error(std::string(who) + ": misaligned buffer (d_audio and d_ws 16 bytes, d_lufs 8)");
        return -1;
    }
    if (!(peak_ceiling > 0.f) || !(peak_ceiling - peak_ceiling == 0.f)) { set_error(std::string(who) + ": peak_ceiling must be positive and finite"); return -1; }
    return 0;
}

static void loud_fill(LoudArgs& a, const LoudLayout& l, float* d_audio, int64_t ld, const int64_t* d_lengths, int B, int sample_rate,
                      const float* d_target, float peak_ceiling, double* d_lufs, float* d_gain, float* d_peak, void* d_ws) {
    char* base = static_cast<char*>(d_ws);
    a.audio = d_audio; a.lengths = d_lengths; a.target = d_target; a.ld = ld; a.B = B; a.chunk = l.chunk; a.cps = l.cps;
    a.nchunk = l.nchunk; a.nseg = l.nseg; a.ceiling = peak_ceiling;
    a.status = reinterpret_cast<int64_t*>(base + l.status);
    a.state = reinterpret_cast<double*>(base + l.state);
    a.energy = reinterpret_cast<double*>(base + l.energy);
    a.cpeak = reinterpret_cast<float*>(base + l.cpeak);
    a.seg = reinterpret_cast<double*>(base + l.seg);
    a.lufs = d_lufs; a.gain = d_gain; a.peak = d_peak;
    loud_coefficients(sample_rate, a.k);
    // column j of M = A^chunk: the state after `chunk` samples of silence from the unit state e_j
    for (int j = 0; j < 4; ++j) {
        double s[4] = {0.0, 0.0, 0.0, 0.0};
        s[j] = 1.0;
        for (int t = 0; t < l.chunk; ++t) loud_step(a.k, 0.0, s[0], s[1], s[2], s[3]);
        for (int i = 0; i < 4; ++i) a.M[4 * i + j] = s[i];
        for (int t = l.chunk; t < l.chunk * LOUD_SCAN_RUN; ++t) loud_step(a.k, 0.0, s[0], s[1], s[2], s[3]);
        for (int i = 0; i < 4; ++i) a.P[4 * i + j] = s[i];
    }
}

// The interpolator of the true-peak pass (include/mtts.h): h[p][k] for phase p of F and tap k of 12, fp64 rounded once to fp32; row 0
// is the sample itself (the unit impulse at tap 5).  Returns F.
static int true_peak_filter(int sample_rate, float* h) {
    const double pi = 3.14159265358979323846;
    const int F = sample_rate < 48000 ? 8 : (sample_rate < 96000 ? 4 : 2);
    for (int k = 0; k < TP_TAPS; ++k) h[k] = k == 5 ? 1.0f : 0.0f;
    for (int p = 1; p < F; ++p) {
        double w[TP_TAPS], sum = 0.0;
        for (int k = 0; k < TP_TAPS; ++k) {
            const double d = (double)(k - 5) - (double)p / (double)F;
            w[k] = std::sin(pi * d) / (pi * d) * (0.5 * (1.0 + std::cos(pi * d / 6.0)));
            sum = sum + w[k];
        }
        for (int k = 0; k < TP_TAPS; ++k) h[p * TP_TAPS + k] = (float)(w[k] / sum);
    }
    return F;
}

// The workspace of mtts_loudness_r128: that of mtts_loudness, then one float per tile of the true-peak pass and one word per segment
struct R128Layout { size_t tpeak, st, total; int64_t ntp; };
static R128Layout r128_layout(const LoudLayout& l, int64_t ld, int B) {
    R128Layout x;
    x.ntp = (ld + TP_TILE - 1) / TP_TILE;
    WS ws(nullptr, 0);
    ws.off = l.total;
    ws.bytes((size_t)B * x.ntp * sizeof(float));                           x.tpeak = ws.off - (size_t)B * x.ntp * sizeof(float);
    ws.bytes((size_t)B * l.nseg * sizeof(unsigned long long));             x.st = ws.off - (size_t)B * l.nseg * sizeof(unsigned long long);
    x.total = ws.off + 256;
    return x;
}

}  // namespace mtts

using namespace mtts;

extern "C" {

int mtts_loudness_chunk(int sample_rate) {
    if (!loud_rate_ok(sample_rate)) { set_error("mtts_loudness_chunk: sample_rate must be a multiple of 100 in [8000, 192000]"); return -1; }
    return loud_chunk(sample_rate);
}

int mtts_loudness_tile(void) { return MTTS_LOUDNESS_TILE; }

int mtts_loudness_coefficients(int sample_rate, double* h_out) {
    if (!h_out) { set_error("mtts_loudness_coefficients: null argument"); return -1; }
    if (!loud_rate_ok(sample_rate)) { set_error("mtts_loudness_coefficients: sample_rate must be a multiple of 100 in [8000, 192000]"); return -1; }
    loud_coefficients(sample_rate, h_out);
    return 0;
}

int64_t mtts_loudness_workspace_bytes(int64_t ld, int B, int sample_rate) {
    if (loud_shape_ok("mtts_loudness_workspace_bytes", ld, B, sample_rate)) return -1;
    return (int64_t)loud_layout(ld, B, sample_rate).total;
}

int mtts_loudness(float* d_audio, int64_t ld, const int64_t* d_lengths, int B, int sample_rate, const float* d_target, float peak_ceiling,
                  int apply, double* d_lufs, float* d_gain, float* d_peak, void* d_ws, int64_t ws_bytes, void* stream) {
    if (!d_audio || !d_lengths || !d_lufs || !d_gain || !d_peak || !d_ws) { set_error("mtts_loudness: null argument"); return -1; }
    if (loud_host_checks("mtts_loudness", d_audio, ld, B, sample_rate, peak_ceiling, d_lufs, d_ws)) return -1;
    const LoudLayout l = loud_layout(ld, B, sample_rate);
    if (ws_bytes < (int64_t)l.total) { set_error("mtts_loudness: workspace too small (mtts_loudness_workspace_bytes)"); return -1; }
    LoudArgs a;
    loud_fill(a, l, d_audio, ld, d_lengths, B, sample_rate, d_target, peak_ceiling, d_lufs, d_gain, d_peak, d_ws);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int64_t tiles = (ld + (int64_t)LOUD_THREADS * l.chunk - 1) / ((int64_t)LOUD_THREADS * l.chunk);
    hipLaunchKernelGGL(loud_chunk_kernel<false>, dim3((unsigned)tiles, B), dim3(LOUD_THREADS), 0, s, a);
    hipLaunchKernelGGL(loud_scan_kernel, dim3(B), dim3(64), 0, s, a);
    hipLaunchKernelGGL(loud_chunk_kernel<true>, dim3((unsigned)tiles, B), dim3(LOUD_THREADS), 0, s, a);
    hipLaunchKernelGGL(loud_gate_kernel, dim3(B), dim3(LOUD_THREADS), 0, s, a);
    g_kernel_tag = "loud_gate_kernel";
    if (apply) {
        hipLaunchKernelGGL(loud_apply_kernel, dim3((unsigned)((ld + LOUD_APPLY_TILE - 1) / LOUD_APPLY_TILE), B), dim3(256), 0, s, a);
        g_kernel_tag = "loud_apply_kernel";
    }
    return launched("mtts_loudness");
}

int mtts_true_peak_tile(void) { return MTTS_TRUE_PEAK_TILE; }

int mtts_true_peak_filter(int sample_rate, float* h_out, int* F_out) {
    if (!h_out || !F_out) { set_error("mtts_true_peak_filter: null argument"); return -1; }
    if (!loud_rate_ok(sample_rate)) { set_error("mtts_true_peak_filter: sample_rate must be a multiple of 100 in [8000, 192000]"); return -1; }
    *F_out = true_peak_filter(sample_rate, h_out);
    return 0;
}

int64_t mtts_loudness_r128_workspace_bytes(int64_t ld, int B, int sample_rate) {
    if (loud_shape_ok("mtts_loudness_r128_workspace_bytes", ld, B, sample_rate)) return -1;
    return (int64_t)r128_layout(loud_layout(ld, B, sample_rate), ld, B).total;
}

int mtts_loudness_r128(float* d_audio, int64_t ld, const int64_t* d_lengths, int B, int sample_rate, const float* d_target, float peak_ceiling,
                       float true_peak_ceiling_db, int apply, double* d_lufs, float* d_gain, float* d_peak, float* d_true_peak, double* d_lra,
                       double* d_momentary_max, double* d_short_term_max, void* d_ws, int64_t ws_bytes, void* stream) {
    if (!d_audio || !d_lengths || !d_lufs || !d_gain || !d_peak || !d_true_peak || !d_lra || !d_momentary_max || !d_short_term_max || !d_ws) {
        set_error("mtts_loudness_r128: null argument");
        return -1;
    }
    if (loud_host_checks("mtts_loudness_r128", d_audio, ld, B, sample_rate, peak_ceiling, d_lufs, d_ws)) return -1;
    if ((reinterpret_cast<uintptr_t>(d_lra) & 7) || (reinterpret_cast<uintptr_t>(d_momentary_max) & 7) || (reinterpret_cast<uintptr_t>(d_short_term_max) & 7)) {
        set_error("mtts_loudness_r128: misaligned buffer (d_lra, d_momentary_max and d_short_term_max 8 bytes)");
        return -1;
    }
    if (true_peak_ceiling_db == true_peak_ceiling_db && !(true_peak_ceiling_db <= 0.f && true_peak_ceiling_db - true_peak_ceiling_db == 0.f)) {
        set_error("mtts_loudness_r128: true_peak_ceiling_db must be finite and at most 0 dBTP, or NaN for none");
        return -1;
    }
    const LoudLayout l = loud_layout(ld, B, sample_rate);
    const R128Layout x = r128_layout(l, ld, B);
    if (ws_bytes < (int64_t)x.total) { set_error("mtts_loudness_r128: workspace too small (mtts_loudness_r128_workspace_bytes)"); return -1; }
    R128Args r;
    loud_fill(r.a, l, d_audio, ld, d_lengths, B, sample_rate, d_target, peak_ceiling, d_lufs, d_gain, d_peak, d_ws);
    char* base = static_cast<char*>(d_ws);
    float h[TP_FACTOR_MAX * TP_TAPS];
    const int F = true_peak_filter(sample_rate, h);
    for (int i = 0; i < (TP_FACTOR_MAX - 1) * TP_TAPS; ++i) r.h[i] = i < (F - 1) * TP_TAPS ? h[TP_TAPS + i] : 0.f;
    r.c_tp = true_peak_ceiling_db == true_peak_ceiling_db ? (float)std::pow(10.0, (double)true_peak_ceiling_db / 20.0) : NAN;
    r.ntp = x.ntp;
    r.tpeak = reinterpret_cast<float*>(base + x.tpeak);
    r.st = reinterpret_cast<unsigned long long*>(base + x.st);
    r.true_peak = d_true_peak; r.lra = d_lra; r.mmax = d_momentary_max; r.smax = d_short_term_max;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int64_t tiles = (ld + (int64_t)LOUD_THREADS * l.chunk - 1) / ((int64_t)LOUD_THREADS * l.chunk);
    hipLaunchKernelGGL(loud_chunk_kernel<false>, dim3((unsigned)tiles, B), dim3(LOUD_THREADS), 0, s, r.a);
    hipLaunchKernelGGL(loud_scan_kernel, dim3(B), dim3(64), 0, s, r.a);
    hipLaunchKernelGGL(loud_chunk_kernel<true>, dim3((unsigned)tiles, B), dim3(LOUD_THREADS), 0, s, r.a);
    const dim3 tp_grid((unsigned)x.ntp, B);
    if (F == 8) hipLaunchKernelGGL(loud_true_peak_kernel<8>, tp_grid, dim3(256), 0, s, r);
    else if (F == 4) hipLaunchKernelGGL(loud_true_peak_kernel<4>, tp_grid, dim3(256), 0, s, r);
    else hipLaunchKernelGGL(loud_true_peak_kernel<2>, tp_grid, dim3(256), 0, s, r);
    hipLaunchKernelGGL(loud_gate_r128_kernel, dim3(B), dim3(LOUD_THREADS), 0, s, r);
    g_kernel_tag = "loud_gate_r128_kernel";
    if (apply) {
        hipLaunchKernelGGL(loud_apply_kernel, dim3((unsigned)((ld + LOUD_APPLY_TILE - 1) / LOUD_APPLY_TILE), B), dim3(256), 0, s, r.a);
        g_kernel_tag = "loud_apply_kernel";
    }
    return launched("mtts_loudness_r128");
}

// The verdict of the latest mtts_loudness or mtts_loudness_r128 on this workspace.  Waits for the stream.
int mtts_loudness_status(const void* d_ws, void* stream) {
    int64_t st[3];
    if (read_status("mtts_loudness_status", d_ws, stream, st)) return -1;
    if (st[0] == 0) return 0;
    set_error("mtts_loudness: row " + std::to_string(st[0] - 1) + " (length " + std::to_string(st[1]) + ") is refused: its length is outside [0, ld = " +
              std::to_string(st[2]) + "]");
    return -1;
}

}  // extern "C"
