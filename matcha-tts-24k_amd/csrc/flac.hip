// FLAC out (gfx950): a ragged batch of fp32 rows to one complete mono 16-bit FLAC stream per row (RFC 9639), encoded on the device.
//
// The bytes are include/mtts.h "FLAC out", restated in tests/flac_restated.py: the PCM16 words of mtts_pcm_encode (pcm_quantise.h),
// fixed-size frames, per frame one CONSTANT / FIXED (order 0..4, Rice partitions of 256 residuals) / VERBATIM subframe.  Nothing
// depends on the row index, the grid or the batch.  Three plain launches, no flags between workgroups:
//   1. flac_frame_kernel, grid (frame, row), 256 threads: quantise into LDS, choose the subframe, pack the frame's bits into an LDS
//      bitstream (LDS atomicOr of at most 16 bits at a time: a code touches at most two words), close it with its two CRCs and store
//      it into the frame's fixed-stride staging slot, with its byte count.
//   2. flac_layout_kernel, grid (row): exclusive scan of the row's frame byte counts, their minimum and maximum, the 42 header
//      bytes, d_out_bytes[b].
//   3. flac_compact_kernel, grid (frame, row): the frame's bytes from its slot to their place in the row's stream.  Every output
//      byte is written once, nothing at or beyond d_out_bytes[b].
// A thread owns the samples t, t + 256, ... of its frame, so pass j of a full frame is Rice partition j, one residual per thread.
// Every loop is bounded by the block size, by the frames of a row (ld / block size, which the host checked) or by a constant; a
// unary run is never walked: a code is its offset (from a scan of the code lengths) plus one 16-bit write.
//
// mtts_flac_encode_lpc launches flac_frame_kernel<true> in place of launch 1: the same frame, with LPC subframes among the candidates
// (include/mtts.h "FLAC out", the lpc paragraphs; tests/flac_lpc_restated.py).  Between the order costs and the frame header it
// analyses the frame -- integer window, exact int64 autocorrelation (a thread's strided samples at every lag, one wave_sum tree per
// lag), Levinson-Durbin in fp64 run by every thread alike (no broadcast, no LDS), the candidates' quantised coefficients in
// registers -- and behind the FIXED plan it plans each candidate in the same LDS (u is reused; only the winner's plan is kept, and
// planned again when it was not the last).  Nothing of a candidate reaches the bitstream before its bit count beat FIXED's and
// VERBATIM's.  flac_frame_kernel<false> is what mtts_flac_encode has always launched.
#include "host.h"
#include "pcm_quantise.h"

namespace mtts {

constexpr int FLAC_THREADS = 256;
constexpr int FLAC_WAVES = FLAC_THREADS / 64;
constexpr int FLAC_MAX_PARTS = 16;                 // 4096 / 256
constexpr int FLAC_KS = 15;                        // Rice parameters 0..14 (15 is the escape, never used)
constexpr int FLAC_HEADER = 42;
constexpr int64_t FLAC_MAX_FRAMES = (int64_t)1 << 21;
constexpr int FLAC_LPC_MAX = 12;                   // the largest LPC order written
constexpr int FLAC_LPC_CANDS = 3;                  // orders 4, 8, 12, each capped at max_lpc_order, once each
constexpr int FLAC_LPC_PRECISION = 12;             // bits of a quantised coefficient
constexpr int FLAC_LPC_RANGE = 1 << 20;            // a candidate with a residual at or beyond it is dropped
using u32x4 = __attribute__((ext_vector_type(4))) unsigned int;

struct FlacArgs {
    const float* audio;          // [B][ld]
    const int64_t* lengths;      // [B] samples
    const int32_t* rates;        // [B] Hz
    const int64_t* keys;         // [B] or null
    int64_t ld, nfmax;           // nfmax = ceil(ld / bs): frames a row can have
    int bs, log2bs, slot;        // slot = 2 * bs + 16: bytes of a staging slot, the bound of a frame
    unsigned int seed_lo, seed_hi;
    int dither;
    int lpc;                     // max_lpc_order, 0..12 (read by flac_frame_kernel<true> alone)
    uint8_t* out;                // [B][out_ld]
    int64_t out_ld;
    int64_t* out_bytes;          // [B]
    int32_t* fbytes;             // [B][nfmax] bytes of a frame
    int64_t* foffs;              // [B][nfmax] where a frame begins behind the row's header
    uint8_t* slots;              // [B][nfmax][slot]
};

// frames of row b, or -1 for a row that is refused (the three kernels agree through this one function)
__device__ __forceinline__ int64_t flac_frames(const FlacArgs& a, int b) {
    const int64_t len = a.lengths[b];
    const int rate = a.rates[b];
    if (len < 0 || len > a.ld || rate < 1 || rate > 1048575) return -1;
    const int64_t nf = (len + a.bs - 1) >> a.log2bs;
    return nf > FLAC_MAX_FRAMES ? -1 : nf;
}

template <class T>
__device__ __forceinline__ T wave_sum(T v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
// exclusive scan of v over the workgroup in thread order, and the total; wsum: FLAC_WAVES words of LDS
template <class T>
__device__ __forceinline__ T block_exscan(T v, T* wsum, T& total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    T inc = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const T t = __shfl_up(inc, o);
        if (lane >= o) inc += t;
    }
    __syncthreads();                             // (the previous call's readers are done with wsum)
    if (lane == 63) wsum[wave] = inc;
    __syncthreads();
    T base = 0;
    total = 0;
#pragma unroll
    for (int w = 0; w < FLAC_WAVES; ++w) {
        const T s = wsum[w];
        if (w < wave) base += s;
        total += s;
    }
    return base + inc - v;
}

// nb bits (1..16) of v, MSB first, at bit position pos of the stream: word pos / 32 holds its first bit in bit 31 - pos % 32
__device__ __forceinline__ void put_bits(unsigned int* bits, unsigned int pos, unsigned int v, int nb) {
    const unsigned int wi = pos >> 5;
    const int room = 32 - (int)(pos & 31);
    if (nb <= room) {
        atomicOr(&bits[wi], v << (room - nb));
    } else {
        atomicOr(&bits[wi], v >> (nb - room));
        atomicOr(&bits[wi + 1], v << (32 - (nb - room)));
    }
}
__device__ __forceinline__ unsigned int stream_byte(const unsigned int* bits, int i) { return (bits[i >> 2] >> (24 - 8 * (i & 3))) & 0xFFu; }

__device__ __forceinline__ unsigned int crc8_byte(unsigned int c, unsigned int byte) {
    c ^= byte;
#pragma unroll
    for (int i = 0; i < 8; ++i) c = (c & 0x80u) ? ((c << 1) ^ 0x07u) & 0xFFu : (c << 1) & 0xFFu;
    return c;
}
// CRC-16, polynomial 0x8005, as a polynomial over GF(2): bit i of the register is the coefficient of x^i
constexpr unsigned int crc16_mulx(unsigned int p) { return (p & 0x8000u) ? ((p << 1) ^ 0x8005u) & 0xFFFFu : p << 1; }
__device__ __forceinline__ unsigned int crc16_byte(unsigned int c, unsigned int byte) {
    c ^= byte << 8;
#pragma unroll
    for (int i = 0; i < 8; ++i) c = crc16_mulx(c);
    return c;
}
constexpr unsigned int crc16_mul(unsigned int x, unsigned int y) {          // x * y mod the polynomial
    unsigned int r = 0;
    for (int i = 15; i >= 0; --i) {
        r = crc16_mulx(r);
        if ((y >> i) & 1u) r ^= x;
    }
    return r;
}
// v[l][L] = x^(8 L 2^l) mod the polynomial: what appending 2^l chunks of L bytes multiplies a register by.  L <= 33 covers the
// largest frame (8206 bytes before its CRC-16 over 256 chunks).  Built by the compiler.
constexpr int FLAC_CRC_LEVELS = 8, FLAC_CRC_MAX_L = 33;
struct Crc16Shifts {
    unsigned short v[FLAC_CRC_LEVELS][FLAC_CRC_MAX_L + 1];
    constexpr Crc16Shifts() : v() {
        for (int L = 0; L <= FLAC_CRC_MAX_L; ++L) {
            unsigned int p = 1;
            for (int i = 0; i < 8 * L; ++i) p = crc16_mulx(p);
            for (int l = 0; l < FLAC_CRC_LEVELS; ++l) {
                v[l][L] = (unsigned short)p;
                p = crc16_mul(p, p);
            }
        }
    }
};
constexpr Crc16Shifts CRC16_SHIFTS_HOST{};
static_assert(CRC16_SHIFTS_HOST.v[0][1] == 0x0100 && CRC16_SHIFTS_HOST.v[0][2] == 0x8005 && CRC16_SHIFTS_HOST.v[1][1] == 0x8005 &&
              CRC16_SHIFTS_HOST.v[3][0] == 1, "x^8, x^16 = the polynomial's low bits, x^0");
static_assert((1 << FLAC_CRC_LEVELS) == FLAC_THREADS && FLAC_CRC_MAX_L * FLAC_THREADS >= 2 * 4096 + 14, "one chunk per thread covers a frame");
__constant__ const Crc16Shifts CRC16_SHIFTS{};

// the o-th difference at sample i >= o of the frame's words
__device__ __forceinline__ int fixed_residual(const int* q, int i, int o) {
    const int x0 = q[i];
    if (o == 0) return x0;
    const int x1 = q[i - 1];
    if (o == 1) return x0 - x1;
    const int x2 = q[i - 2];
    if (o == 2) return x0 - 2 * x1 + x2;
    const int x3 = q[i - 3];
    if (o == 3) return x0 - 3 * x1 + 3 * x2 - x3;
    return x0 - 4 * x1 + 6 * x2 - 4 * x3 + q[i - 4];
}

__device__ __forceinline__ int flac_rate_code(int rate) {
    switch (rate) {
        case 88200: return 1;   case 176400: return 2;  case 192000: return 3;  case 8000: return 4;
        case 16000: return 5;   case 22050: return 6;   case 24000: return 7;   case 32000: return 8;
        case 44100: return 9;   case 48000: return 10;  case 96000: return 11;
    }
    if (rate <= 65535) return 13;
    if (rate % 10 == 0 && rate / 10 <= 65535) return 14;
    return 0;
}

// the LPC residual at sample i >= m: 12 taps of 12 bits on 16-bit words keep the sum below 12 * 2^11 * 2^15 < 2^31
__device__ __forceinline__ int lpc_residual(const int* q, int i, const int (&c)[FLAC_LPC_MAX], int m, int shift) {
    int s = 0;
#pragma unroll
    for (int j = 0; j < FLAC_LPC_MAX; ++j)
        if (j < m) s += c[j] * q[i - 1 - j];
    return q[i] - (s >> shift);
}

// The Rice plan of one predictor of order `order` over the frame's n words: the folded residuals into u (0 where a sample has none),
// then sum(u >> k) for the 15 candidates over each run of 256 samples: thread (j, k) = (tid / 16, tid % 16) reads run j from LDS, 16
// bytes at a time, its start rotated by 4 j reads so that the four runs a wave reads lie in different banks.  A run's sum stays below
// 256 * 2^21 = 2^29: 32 bits.  A full frame's partition j is run j; a short frame is one partition of up to 4095 values, the 64-bit
// sum of its runs (up to 2^33).  pk[p], pcost[p]: the k of partition p and its bits, the 4 of k not included; returns the bits of all
// partitions, their 4-bit parameters included.  RANGE: ~0 instead, and nothing planned, when a |residual| reaches FLAC_LPC_RANGE.
template <bool RANGE, class Residual>
__device__ __forceinline__ unsigned long long rice_plan(unsigned int* u, unsigned int (*part)[16], int* pk, unsigned long long* pcost, int n,
                                                        int order, bool full, int passes, Residual residual) {
    const int tid = threadIdx.x;
    int beyond = 0;
    for (int j = 0; j < passes; ++j) {
        const int i = j * FLAC_THREADS + tid;
        unsigned int uu = 0;
        if (i < n && i >= order) {
            const int r = residual(i);
            if (RANGE) beyond |= r >= FLAC_LPC_RANGE || r <= -FLAC_LPC_RANGE;
            uu = r >= 0 ? 2u * (unsigned int)r : 2u * (unsigned int)(-r) - 1u;
        }
        u[i] = uu;
    }
    if (RANGE) {
        if (__syncthreads_or(beyond)) return ~0ull;              // (the same answer in every thread)
    } else {
        __syncthreads();
    }
    {
        const int k = tid & 15, j = tid >> 4;
        if (k < FLAC_KS && j < passes) {
            const u32x4* run = reinterpret_cast<const u32x4*>(u + j * FLAC_THREADS);
            unsigned int s = 0;
            for (int x = 0; x < FLAC_THREADS / 4; ++x) {
                const u32x4 v = run[(x + 4 * j) & (FLAC_THREADS / 4 - 1)];
                s += (v[0] >> k) + (v[1] >> k) + (v[2] >> k) + (v[3] >> k);
            }
            part[j][k] = s;
        }
    }
    __syncthreads();
    const int nparts = full ? passes : 1;
    if (tid < nparts) {                      // k of partition tid: the fewest bits, ties to the smaller k
        const unsigned long long cnt = full ? (unsigned long long)(FLAC_THREADS - (tid == 0 ? order : 0)) : (unsigned long long)(n - order);
        const int j0 = full ? tid : 0, j1 = full ? tid + 1 : passes;
        unsigned long long least = ~0ull;
        int kbest = 0;
        for (int k = 0; k < FLAC_KS; ++k) {
            unsigned long long c = cnt * (k + 1);
            for (int j = j0; j < j1; ++j) c += part[j][k];
            if (c < least) { least = c; kbest = k; }
        }
        pk[tid] = kbest;
        pcost[tid] = least;
    }
    __syncthreads();
    unsigned long long total = 0;
    for (int p = 0; p < nparts; ++p) total += 4ull + pcost[p];
    return total;
}

extern __shared__ __attribute__((aligned(16))) unsigned int flac_lds[];

template <bool LPC>
__global__ __launch_bounds__(FLAC_THREADS) void flac_frame_kernel(const FlacArgs a) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, b = blockIdx.y;
    const int64_t f = blockIdx.x;
    if (f >= flac_frames(a, b)) return;          // no such frame, or a refused row (the layout kernel writes its verdict)
    const int bs = a.bs, passes = bs >> 8;
    const int64_t i0 = f << a.log2bs;
    const int64_t left = a.lengths[b] - i0;
    const int n = left < bs ? (int)left : bs;    // samples of this frame, 1..bs
    const bool full = n == bs;

    int* q = reinterpret_cast<int*>(flac_lds);                   // [bs] the words
    unsigned int* u = flac_lds + bs;                              // [bs] the folded residuals
    unsigned int* bits = flac_lds + 2 * bs;                       // [slot / 4] the frame
    __shared__ unsigned int part[FLAC_MAX_PARTS][16];                             // sum(u >> k) per run of 256 samples and k
    __shared__ unsigned long long red[FLAC_WAVES][6];
    __shared__ unsigned long long pcost[FLAC_MAX_PARTS];
    __shared__ int pk[FLAC_MAX_PARTS];
    __shared__ unsigned int wsum[FLAC_WAVES];
    __shared__ unsigned int crcv[FLAC_THREADS];

    for (int w = tid; w < (a.slot >> 2); w += FLAC_THREADS) bits[w] = 0u;
    const float* row = a.audio + (size_t)b * a.ld + i0;
    const unsigned int hrow = a.dither ? dither_row_hash(a.seed_lo, a.seed_hi, a.keys ? a.keys[b] : 0) : 0u;
    for (int j = 0; j < passes; ++j) {
        const int i = j * FLAC_THREADS + tid;
        if (i < n) {
            float y = row[i] * 32768.f;
            if (a.dither) y = y + dither_tpdf(hrow, (unsigned int)(i0 + i));
            q[i] = quantise16(y);
        }
    }
    __syncthreads();

    // ---- the constant test and the five order costs: sums of |e_o[i]| over i in [4, n).  |e_4| <= 16 * 2^15 and n <= 4096 make a
    // sum reach 2^31: 64-bit accumulators
    unsigned long long cost[5] = {0, 0, 0, 0, 0};
    unsigned long long differ = 0;
    const int q0 = q[0];
    for (int j = 0; j < passes; ++j) {
        const int i = j * FLAC_THREADS + tid;
        if (i < n) {
            differ += q[i] != q0;
            if (i >= 4) {
#pragma unroll
                for (int o = 0; o < 5; ++o) {
                    const int e = fixed_residual(q, i, o);
                    cost[o] += (unsigned long long)(e < 0 ? -e : e);
                }
            }
        }
    }
#pragma unroll
    for (int o = 0; o < 5; ++o) {
        const unsigned long long s = wave_sum(cost[o]);
        if (lane == 0) red[wave][o] = s;
    }
    differ = wave_sum(differ);
    if (lane == 0) red[wave][5] = differ;
    __syncthreads();
    int order = 0;
    unsigned long long best = ~0ull;
#pragma unroll
    for (int o = 0; o < 5; ++o) {
        const unsigned long long s = red[0][o] + red[1][o] + red[2][o] + red[3][o];
        if (s < best) { best = s; order = o; }   // (strict: ties go to the lower order; n <= 4 gives five zeros and order 0)
    }
    const bool constant = red[0][5] + red[1][5] + red[2][5] + red[3][5] == 0;

    // ---- the LPC analysis: per candidate its order (0: none), shift and coefficients, the same in every thread
    int lm[FLAC_LPC_CANDS] = {0, 0, 0}, lshift[FLAC_LPC_CANDS] = {0, 0, 0};
    int lc[FLAC_LPC_CANDS][FLAC_LPC_MAX] = {};
    if constexpr (LPC) {
        __shared__ long long racc[FLAC_WAVES][FLAC_LPC_MAX + 1];
        int cand[FLAC_LPC_CANDS], top = 0;       // the listed orders capped at a.lpc, once each, below n
#pragma unroll
        for (int ci = 0; ci < FLAC_LPC_CANDS; ++ci) {
            const int o = 4 * (ci + 1) < a.lpc ? 4 * (ci + 1) : a.lpc;
            cand[ci] = o > top && o < n ? o : 0;
            top = cand[ci] ? o : top;
        }
        if (!constant && top > 0) {
            // the windowed words into u (free until the first plan): w = 255 - 255 (2 i + 1 - n)^2 / n^2 (integer division) lies in
            // 1..255, and 255 * 4095^2 < 2^32; |q w| < 2^23
            int* x = reinterpret_cast<int*>(u);
            const unsigned int nn = (unsigned int)n * (unsigned int)n;
            for (int j = 0; j < passes; ++j) {
                const int i = j * FLAC_THREADS + tid;
                if (i < n) {
                    const int d = 2 * i + 1 - n;
                    x[i] = q[i] * (255 - (int)(255u * (unsigned int)(d * d) / nn));
                }
            }
            __syncthreads();
            // R[l] = sum_i x[i] x[i + l], exact: a product below 2^46, 4096 of them below 2^58
            long long acc[FLAC_LPC_MAX + 1] = {};
            for (int j = 0; j < passes; ++j) {
                const int i = j * FLAC_THREADS + tid;
                if (i < n) {
                    const long long xi = x[i];
#pragma unroll
                    for (int l = 0; l <= FLAC_LPC_MAX; ++l)
                        if (l <= top && i + l < n) acc[l] += xi * x[i + l];
                }
            }
#pragma unroll
            for (int l = 0; l <= FLAC_LPC_MAX; ++l) {
                if (l <= top) {
                    const long long s = wave_sum(acc[l]);
                    if (lane == 0) racc[wave][l] = s;
                }
            }
            __syncthreads();
            double R[FLAC_LPC_MAX + 1];
#pragma unroll
            for (int l = 0; l <= FLAC_LPC_MAX; ++l) R[l] = l <= top ? (double)(racc[0][l] + racc[1][l] + racc[2][l] + racc[3][l]) : 0.0;
            // Levinson-Durbin, fp64, the one operation order of the contract (no contraction: -ffp-contract=off); al[j - 1] is a_j
            double al[FLAC_LPC_MAX] = {}, err = R[0];
            bool alive = err > 0.0 && err < __builtin_inf();
#pragma unroll
            for (int m = 1; m <= FLAC_LPC_MAX; ++m) {
                if (m <= top && alive) {
                    double s = R[m];
#pragma unroll
                    for (int j = 1; j < m; ++j) s = s - al[j - 1] * R[m - j];
                    const double k = s / err;
                    double an[FLAC_LPC_MAX];
#pragma unroll
                    for (int j = 1; j < m; ++j) an[j - 1] = al[j - 1] - k * al[m - j - 1];
#pragma unroll
                    for (int j = 1; j < m; ++j) al[j - 1] = an[j - 1];
                    al[m - 1] = k;
                    err = err * (1.0 - k * k);
                    alive = err > 0.0 && err < __builtin_inf();
                    if (alive) {
                        // quantise at precision 12: max|a| < 2^e with e from the exponent field, shift = min(15, 11 - e)
                        double cmax = 0.0;
#pragma unroll
                        for (int j = 0; j < m; ++j) cmax = fmax(cmax, fabs(al[j]));
                        const int e = (int)((__double_as_longlong(cmax) >> 52) & 0x7FF) - 1022;
                        const int shift = FLAC_LPC_PRECISION - 1 - e < 15 ? FLAC_LPC_PRECISION - 1 - e : 15;
#pragma unroll
                        for (int ci = 0; ci < FLAC_LPC_CANDS; ++ci) {
                            if (cand[ci] == m && shift >= 0) {
                                lm[ci] = m;
                                lshift[ci] = shift;
#pragma unroll
                                for (int j = 0; j < m; ++j) {
                                    const double v = rint(al[j] * (double)(1 << shift));       // (ties to even)
                                    lc[ci][j] = (int)fmin(fmax(v, -2048.0), 2047.0);
                                }
                            }
                        }
                    }
                }
            }
        }
    }

    // ---- the frame header (thread 0) and its length (every thread)
    const int rate = a.rates[b];
    const int rcode = flac_rate_code(rate);
    const int bcode = full ? 8 + (a.log2bs - 8) : (n <= 256 ? 6 : 7);
    const int nnum = f < 0x80 ? 1 : f < 0x800 ? 2 : f < 0x10000 ? 3 : 4;
    const int hb = 4 + nnum + (bcode == 6 ? 1 : bcode == 7 ? 2 : 0) + (rcode >= 13 ? 2 : 0) + 1;      // header bytes, CRC-8 included
    if (tid == 0) {
        unsigned int crc = 0, at = 0;
        auto emit = [&](unsigned int byte) {
            put_bits(bits, 8 * at, byte, 8);
            crc = crc8_byte(crc, byte);
            ++at;
        };
        emit(0xFFu); emit(0xF8u); emit((unsigned int)(bcode << 4 | rcode)); emit(0x08u);
        const unsigned int v = (unsigned int)f;
        if (nnum == 1) emit(v);
        else if (nnum == 2) { emit(0xC0u | v >> 6); emit(0x80u | (v & 63u)); }
        else if (nnum == 3) { emit(0xE0u | v >> 12); emit(0x80u | ((v >> 6) & 63u)); emit(0x80u | (v & 63u)); }
        else { emit(0xF0u | v >> 18); emit(0x80u | ((v >> 12) & 63u)); emit(0x80u | ((v >> 6) & 63u)); emit(0x80u | (v & 63u)); }
        if (bcode == 6) emit((unsigned int)(n - 1));
        if (bcode == 7) { emit((unsigned int)(n - 1) >> 8); emit((unsigned int)(n - 1) & 0xFFu); }
        if (rcode >= 13) {
            const unsigned int r = rcode == 13 ? (unsigned int)rate : (unsigned int)rate / 10u;
            emit(r >> 8); emit(r & 0xFFu);
        }
        put_bits(bits, 8 * at, crc, 8);
    }
    const unsigned int sb = 8u * hb;             // where the subframe begins
    unsigned int body;                           // bits of the subframe

    if (constant) {
        if (tid == 0) {
            put_bits(bits, sb, 0x00u, 8);
            put_bits(bits, sb + 8, (unsigned int)q0 & 0xFFFFu, 16);
        }
        body = 24;
    } else {
        // ---- FIXED's plan, then each LPC candidate's over the same LDS: the fewest bits win, ties to FIXED, then to the lower order
        const auto fixed = [&](int i) { return fixed_residual(q, i, order); };
        unsigned long long best_bits = 8ull + 16ull * order + 6ull + rice_plan<false>(u, part, pk, pcost, n, order, full, passes, fixed);
        int lpc = 0, shift = 0;                  // the winner: its LPC order (0: FIXED), shift and coefficients
        int cw[FLAC_LPC_MAX] = {};
        if constexpr (LPC) {
            int planned = 0;                     // the order whose plan the LDS holds (0: FIXED's)
#pragma unroll
            for (int ci = 0; ci < FLAC_LPC_CANDS; ++ci) {
                if (lm[ci]) {
                    const int m = lm[ci], sh = lshift[ci];
                    const auto& c = lc[ci];
                    const unsigned long long r = rice_plan<true>(u, part, pk, pcost, n, m, full, passes, [&](int i) { return lpc_residual(q, i, c, m, sh); });
                    const unsigned long long bits_c = 8ull + 16ull * m + 9ull + (unsigned long long)(FLAC_LPC_PRECISION * m) + 6ull + r;
                    planned = m;
                    if (r != ~0ull && bits_c < best_bits) {
                        best_bits = bits_c;
                        lpc = m;
                        shift = sh;
#pragma unroll
                        for (int j = 0; j < FLAC_LPC_MAX; ++j) cw[j] = c[j];
                    }
                }
            }
            if (planned != lpc && best_bits < 8ull + 16ull * n) {                  // the winner's plan again (same values)
                if (lpc) rice_plan<false>(u, part, pk, pcost, n, lpc, full, passes, [&](int i) { return lpc_residual(q, i, cw, lpc, shift); });
                else rice_plan<false>(u, part, pk, pcost, n, order, full, passes, fixed);
            }
        }
        const int worder = lpc ? lpc : order;    // warm-up words
        const unsigned int pre = 8u + 16u * worder + (lpc ? 9u + (unsigned int)(FLAC_LPC_PRECISION * lpc) : 0u);      // bits before the residual

        if (best_bits >= 8ull + 16ull * n) {     // VERBATIM: the bound of a frame, 2 * bs + 16 bytes
            if (tid == 0) put_bits(bits, sb, 0x02u, 8);
            for (int j = 0; j < passes; ++j) {
                const int i = j * FLAC_THREADS + tid;
                if (i < n) put_bits(bits, sb + 8 + 16 * i, (unsigned int)q[i] & 0xFFFFu, 16);
            }
            body = 8 + 16 * n;
        } else {                                 // FIXED or LPC: below 8 + 16 n bits in all, so 32-bit positions hold
            if (tid == 0) {
                put_bits(bits, sb, lpc ? 0x40u | (unsigned int)(lpc - 1) << 1 : 0x10u | (unsigned int)order << 1, 8);
                if (lpc) put_bits(bits, sb + 8 + 16 * lpc, (unsigned int)(FLAC_LPC_PRECISION - 1) << 5 | (unsigned int)shift, 9);
                put_bits(bits, sb + pre, (unsigned int)(full ? a.log2bs - 8 : 0), 6);                 // method 00, partition order
            }
            if (tid < worder) put_bits(bits, sb + 8 + 16 * tid, (unsigned int)q[tid] & 0xFFFFu, 16);
            if constexpr (LPC) {
                if (tid < lpc) {                 // coefficient tid, two's complement
                    int mine = 0;
#pragma unroll
                    for (int j = 0; j < FLAC_LPC_MAX; ++j) mine = tid == j ? cw[j] : mine;
                    put_bits(bits, sb + 8 + 16 * lpc + 9 + FLAC_LPC_PRECISION * tid, (unsigned int)mine & 0xFFFu, FLAC_LPC_PRECISION);
                }
            }
            unsigned int base = sb + pre + 6;
            int k = 0;
            for (int j = 0; j < passes; ++j) {
                if (full || j == 0) {
                    k = pk[full ? j : 0];
                    if (tid == 0) put_bits(bits, base, (unsigned int)k, 4);
                    base += 4;
                }
                const int i = j * FLAC_THREADS + tid;
                const bool coded = i < n && i >= worder;
                const unsigned int uu = coded ? u[i] : 0u;
                unsigned int total;
                const unsigned int at = block_exscan<unsigned int>(coded ? (uu >> k) + 1 + k : 0u, wsum, total);
                // the code: (u >> k) zero bits, which the zeroed stream already holds, then a one and the low k bits of u
                if (coded) put_bits(bits, base + at + (uu >> k), (1u << k) | (uu & ((1u << k) - 1u)), k + 1);
                base += total;
            }
            body = base - sb;
        }
    }
    __syncthreads();                             // every bit of the frame is in LDS

    // ---- CRC-16 over the nbody bytes so far, then the store.  The register is linear in the message and leading zero bytes leave it
    // 0, so the message is cut from its END into 256 chunks of L bytes: thread t takes chunk t (bytes before the frame read as zeros),
    // and a tree joins neighbours: crc(A | B) = crc(A) * x^(8 |B|) + crc(B).
    const int nbody = (int)((sb + body + 7) >> 3);
    const int L = (nbody + FLAC_THREADS - 1) / FLAC_THREADS;
    unsigned int c = 0;
    for (int x = 0, i = nbody - (FLAC_THREADS - tid) * L; x < L; ++x, ++i)
        if (i >= 0) c = crc16_byte(c, stream_byte(bits, i));
    crcv[tid] = c;
    for (int l = 0; l < FLAC_CRC_LEVELS; ++l) {  // level l joins runs of s = 2^l chunks: the left register times x^(8 L s), plus the right
        const int s = 1 << l;
        __syncthreads();
        if ((tid & (2 * s - 1)) == 0) crcv[tid] = crc16_mul(crcv[tid], CRC16_SHIFTS.v[l][L]) ^ crcv[tid + s];
    }
    if (tid == 0) {
        put_bits(bits, 8u * nbody, crcv[0], 16);
        a.fbytes[(size_t)b * a.nfmax + f] = nbody + 2;
    }
    __syncthreads();
    unsigned int* slot = reinterpret_cast<unsigned int*>(a.slots + ((size_t)b * a.nfmax + f) * a.slot);
    for (int w = tid; w < (nbody + 2 + 3) >> 2; w += FLAC_THREADS) slot[w] = __builtin_bswap32(bits[w]);
}

// byte i of the 42 that open a stream: "fLaC", the STREAMINFO block header, STREAMINFO with a zero MD5
__device__ __forceinline__ unsigned int flac_header_byte(int i, int bs, int fmin, int fmax, int rate, int64_t total) {
    if (i < 8) return (0x2200008043614C66ull >> (8 * i)) & 0xFFu;           // 66 4C 61 43 80 00 00 22
    if (i < 12) return (i & 1) ? bs & 0xFF : bs >> 8;
    if (i < 15) return ((unsigned int)fmin >> (8 * (14 - i))) & 0xFFu;
    if (i < 18) return ((unsigned int)fmax >> (8 * (17 - i))) & 0xFFu;
    if (i < 26) {                                                           // rate:20, channels - 1:3, bits - 1:5, samples:36
        const unsigned long long v = (unsigned long long)rate << 44 | 15ull << 36 | (unsigned long long)total;
        return (unsigned int)(v >> (8 * (25 - i))) & 0xFFu;
    }
    return 0u;
}

__global__ __launch_bounds__(FLAC_THREADS) void flac_layout_kernel(const FlacArgs a) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, b = blockIdx.x;
    const int64_t nf = flac_frames(a, b);
    if (nf < 0) {                                // a refused row: no byte written
        if (tid == 0) a.out_bytes[b] = -1;
        return;
    }
    __shared__ long long wsum[FLAC_WAVES];
    __shared__ int wmin[FLAC_WAVES], wmax[FLAC_WAVES];
    const int32_t* fbytes = a.fbytes + (size_t)b * a.nfmax;
    int64_t* foffs = a.foffs + (size_t)b * a.nfmax;
    long long run = 0;
    int fmin = 0x7FFFFFFF, fmax = 0;
    for (int64_t f0 = 0; f0 < nf; f0 += FLAC_THREADS) {           // (nf <= nfmax, which the host derived from ld)
        const int64_t f = f0 + tid;
        const int c = f < nf ? fbytes[f] : 0;
        long long total;
        const long long at = block_exscan<long long>(c, wsum, total);
        if (f < nf) {
            foffs[f] = run + at;
            fmin = c < fmin ? c : fmin;
            fmax = c > fmax ? c : fmax;
        }
        run += total;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const int lo = __shfl_xor(fmin, o), hi = __shfl_xor(fmax, o);
        fmin = lo < fmin ? lo : fmin;
        fmax = hi > fmax ? hi : fmax;
    }
    if (lane == 0) { wmin[wave] = fmin; wmax[wave] = fmax; }
    __syncthreads();
    for (int w = 0; w < FLAC_WAVES; ++w) {
        fmin = wmin[w] < fmin ? wmin[w] : fmin;
        fmax = wmax[w] > fmax ? wmax[w] : fmax;
    }
    if (nf == 0) fmin = 0;
    if (tid < FLAC_HEADER) a.out[(size_t)b * a.out_ld + tid] = (uint8_t)flac_header_byte(tid, a.bs, fmin, fmax, a.rates[b], a.lengths[b]);
    if (tid == 0) a.out_bytes[b] = FLAC_HEADER + run;
}

__global__ __launch_bounds__(FLAC_THREADS) void flac_compact_kernel(const FlacArgs a) {
    const int b = blockIdx.y;
    const int64_t f = blockIdx.x;
    if (f >= flac_frames(a, b)) return;
    const size_t at = (size_t)b * a.nfmax + f;
    const int nbytes = a.fbytes[at];             // <= slot, and the row's total fits out_ld (mtts_flac_row_bytes)
    const uint8_t* src = a.slots + at * a.slot;
    uint8_t* dst = a.out + (size_t)b * a.out_ld + FLAC_HEADER + a.foffs[at];
    for (int i = threadIdx.x; i < nbytes; i += FLAC_THREADS) dst[i] = src[i];
}

}  // namespace mtts

using namespace mtts;

static int flac_log2bs(int block_size) {
    for (int l = 8; l <= 12; ++l)
        if (block_size == 1 << l) return l;
    return -1;
}
static int flac_shape_ok(const char* who, int64_t ld, int block_size) {
    if (flac_log2bs(block_size) < 0) { set_error(std::string(who) + ": block_size is one of 256, 512, 1024, 2048, 4096"); return -1; }
    if (ld < 4 || (ld & 3)) { set_error(std::string(who) + ": rows must be 16-byte aligned (ld a positive multiple of 4 samples)"); return -1; }
    if (ld > (int64_t)1 << 30) { set_error(std::string(who) + ": rows longer than 2^30 samples"); return -1; }
    return 0;
}
// the three sections of the workspace, carved the same way by the size query and by the call
static void flac_carve(WS& ws, FlacArgs& a, int B) {
    const size_t frames = (size_t)B * a.nfmax;
    a.fbytes = static_cast<int32_t*>(ws.bytes(frames * sizeof(int32_t)));
    a.foffs = static_cast<int64_t*>(ws.bytes(frames * sizeof(int64_t)));
    a.slots = static_cast<uint8_t*>(ws.bytes(frames * a.slot));
}
static void flac_shape(FlacArgs& a, int64_t ld, int block_size) {
    a.ld = ld; a.bs = block_size; a.log2bs = flac_log2bs(block_size);
    a.nfmax = (ld + block_size - 1) / block_size;
    a.slot = 2 * block_size + 16;
}
static bool flac_overlap(const void* p, size_t np, const void* q, size_t nq) {
    const uintptr_t a = reinterpret_cast<uintptr_t>(p), b = reinterpret_cast<uintptr_t>(q);
    return a < b + nq && b < a + np;
}

// both entries: max_lpc_order 0 is mtts_flac_encode, launch for launch
static int flac_encode(const std::string& who, const float* d_audio, int64_t ld, const int64_t* d_lengths, const int32_t* d_rates,
                       const int64_t* d_keys, int B, int block_size, int max_lpc_order, int dither, int64_t seed, uint8_t* d_out,
                       int64_t out_ld, int64_t* d_out_bytes, void* d_ws, int64_t ws_bytes, void* stream) {
    if (!d_audio || !d_lengths || !d_rates || !d_out || !d_out_bytes || !d_ws) { set_error(who + ": null argument"); return -1; }
    if (B < 1 || B > 65535) { set_error(who + ": B must lie in [1, 65535]"); return -1; }
    if (flac_shape_ok(who.c_str(), ld, block_size)) return -1;
    FlacArgs a;
    flac_shape(a, ld, block_size);
    if (out_ld < (FLAC_HEADER + a.nfmax * a.slot + 15) / 16 * 16 || (out_ld & 15)) {
        set_error(who + ": out_ld must be a multiple of 16, at least mtts_flac_row_bytes(ld, block_size)");
        return -1;
    }
    WS ws(d_ws, (size_t)(ws_bytes < 0 ? 0 : ws_bytes));
    flac_carve(ws, a, B);
    if (ws.overflow) { set_error(who + ": workspace too small (mtts_flac_workspace_bytes)"); return -1; }
    if ((reinterpret_cast<uintptr_t>(d_audio) & 15) || (reinterpret_cast<uintptr_t>(d_out) & 15) || (reinterpret_cast<uintptr_t>(d_ws) & 15)) {
        set_error(who + ": misaligned buffer (16 bytes)");
        return -1;
    }
    const size_t in_bytes = (size_t)B * ld * sizeof(float), out_bytes = (size_t)B * out_ld;
    if (flac_overlap(d_audio, in_bytes, d_out, out_bytes) || flac_overlap(d_audio, in_bytes, d_ws, ws.off) ||
        flac_overlap(d_out, out_bytes, d_ws, ws.off)) {
        set_error(who + ": d_out, d_ws and d_audio must not overlap");
        return -1;
    }
    a.audio = d_audio; a.lengths = d_lengths; a.rates = d_rates; a.keys = d_keys;
    a.seed_lo = (unsigned int)((uint64_t)seed & 0xFFFFFFFFu);
    a.seed_hi = (unsigned int)((uint64_t)seed >> 32);
    a.dither = dither ? 1 : 0;
    a.lpc = max_lpc_order;
    a.out = d_out; a.out_ld = out_ld; a.out_bytes = d_out_bytes;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const size_t lds = (size_t)2 * a.bs * sizeof(int) + a.slot;
    if (max_lpc_order) hipLaunchKernelGGL(flac_frame_kernel<true>, dim3((unsigned)a.nfmax, B), dim3(FLAC_THREADS), lds, s, a);
    else hipLaunchKernelGGL(flac_frame_kernel<false>, dim3((unsigned)a.nfmax, B), dim3(FLAC_THREADS), lds, s, a);
    RET_IF(launched("flac_frame_kernel"));
    hipLaunchKernelGGL(flac_layout_kernel, dim3(B), dim3(FLAC_THREADS), 0, s, a);
    RET_IF(launched("flac_layout_kernel"));
    hipLaunchKernelGGL(flac_compact_kernel, dim3((unsigned)a.nfmax, B), dim3(FLAC_THREADS), 0, s, a);
    return launched("flac_compact_kernel");
}

extern "C" {

int64_t mtts_flac_row_bytes(int64_t ld, int block_size) {
    if (flac_shape_ok("mtts_flac_row_bytes", ld, block_size)) return -1;
    FlacArgs a;
    flac_shape(a, ld, block_size);
    return (FLAC_HEADER + a.nfmax * a.slot + 15) / 16 * 16;
}

int64_t mtts_flac_workspace_bytes(int B, int64_t ld, int block_size) {
    if (B < 1 || B > 65535) { set_error("mtts_flac_workspace_bytes: B must lie in [1, 65535]"); return -1; }
    if (flac_shape_ok("mtts_flac_workspace_bytes", ld, block_size)) return -1;
    FlacArgs a;
    flac_shape(a, ld, block_size);
    WS ws(nullptr, 0);
    flac_carve(ws, a, B);
    return (int64_t)ws.off;
}

int mtts_flac_encode(const float* d_audio, int64_t ld, const int64_t* d_lengths, const int32_t* d_rates, const int64_t* d_keys, int B,
                     int block_size, int dither, int64_t seed, uint8_t* d_out, int64_t out_ld, int64_t* d_out_bytes, void* d_ws,
                     int64_t ws_bytes, void* stream) {
    return flac_encode("mtts_flac_encode", d_audio, ld, d_lengths, d_rates, d_keys, B, block_size, 0, dither, seed, d_out, out_ld, d_out_bytes,
                       d_ws, ws_bytes, stream);
}

int mtts_flac_encode_lpc(const float* d_audio, int64_t ld, const int64_t* d_lengths, const int32_t* d_rates, const int64_t* d_keys, int B,
                         int block_size, int max_lpc_order, int dither, int64_t seed, uint8_t* d_out, int64_t out_ld, int64_t* d_out_bytes,
                         void* d_ws, int64_t ws_bytes, void* stream) {
    if (max_lpc_order < 0 || max_lpc_order > FLAC_LPC_MAX) { set_error("mtts_flac_encode_lpc: max_lpc_order lies in 0..12"); return -1; }
    return flac_encode("mtts_flac_encode_lpc", d_audio, ld, d_lengths, d_rates, d_keys, B, block_size, max_lpc_order, dither, seed, d_out,
                       out_ld, d_out_bytes, d_ws, ws_bytes, stream);
}

}  // extern "C"
