// Monotonic Alignment Search on the device (gfx950): which fine mel frames belong to which token.
//
// Semantics: the forced alignment of the reference's training forward (matcha/models/matcha_tts.py:184-201): a diagonal-Gaussian
// log-prior of every (token, frame) pair, then the monotone path of largest total log-prior that starts at (0, 0), ends at
// (Tx_b - 1, Tm_b - 1) and gives every token at least one frame (Kim et al. 2020, Glow-TTS, algorithm 1).  The reference takes the
// search from an external package; this file is written from the published recurrence:
//     v[0][0] = lp[0][0];   v[x][y] = lp[x][y] + max(v[x][y-1], v[x-1][y-1])   for max(0, Tx_b-(Tm_b-y)) <= x <= min(y, Tx_b-1)
// with every cell outside that band at -1e9, and the back-pointer rule "walking back from (Tx_b-1, Tm_b-1), at frame y on token x
// step to x-1 iff x > 0 and (x == y or v[x-1][y-1] > v[x][y-1])": ties stay on the same token.  One add and one compare per cell
// in frame order: no summation order to choose, so durations, path and score equal a NumPy fp32 restatement bit for bit
// (tests/mas_restated.py).
//
// Everything is fp32 (the reference computes the log-prior in fp32 on purpose, matcha_tts.py:90-101: reduced precision flips the
// path between near-equal candidates).  Loads are plain HIP loads (no inline asm, no counted waits).
//
// Launches of one mtts_mas call:
//   mas_logprior_kernel<true>   lp[x][y] = -0.5 * sum_f (y[f][y] - mu[f][x])^2, which is -0.5|y|^2 + <mu, y> - 0.5|mu|^2 without the
//                        cancellation of the expanded form: a subtraction and an FMA per term on the vector pipe, fp32 operands and
//                        accumulator, 64 x 64 tile per workgroup, both operands through LDS in chunks of 16 features.  Written
//                        FRAME-major ([B][Tm][64 K], all tokens of one frame contiguous) for the search.  (mas_transpose_kernel
//                        instead when the caller brings a log-prior in the reference's [B, Tx, Tm] layout.)
//   mas_forward_kernel<K>  ONE WAVEFRONT per utterance.  Lane l owns the K = ceil(Tx / 64) consecutive tokens l K .. l K + K - 1 in
//                        registers (K in 1, 2, 4, 8, 16: Tx <= 1024).  Per frame a lane's K cells are independent of one another
//                        and the only cross-lane value is the previous lane's last token: one DPP wave_shr:1.  No LDS, no barrier.
//                        The log-prior rows of the next 64 / K frames are loaded while the current 64 / K are processed (two
//                        register buffers).  The upper band edge (x <= y) is applied to the log-prior (-inf), off the dependent
//                        chain and only while y < 64 K; an out-of-band cell then never wins a comparison, which is all the -1e9 of
//                        the recurrence is for (the lower band edge only spares work: no cell below it can reach an in-band cell).
//                        Decisions are kept as BITS (1 = came from x-1): lane l packs its K bits of 32 / K consecutive frames into
//                        one dword, so a 64-dword row holds 32 / K frames of every token and is stored coalesced.
//   mas_backtrack_kernel<K>  one wavefront per utterance.  Which ROW of decision bits a frame needs is known in advance: rows are
//                        loaded 64 frames ahead, one dword per lane, and the walk's dependent chain per frame is a v_readlane of
//                        the row at lane x / K, a shift and a subtract on the scalar unit.  The first frame of every token goes
//                        to LDS; durations are the differences, written by all lanes.
//   mas_path_kernel      only when the dense 0/1 path [B, Tx, Tm] is asked for (parity with maximum_path, debugging).
// B utterances occupy B CUs at one wave each: the search is latency-bound by its Tm dependent steps and that is accepted
// ("Forced alignment").  No workgroup waits on another and nothing spins.
//
// The lengths live on the device.  A bad utterance (Tx_b < 1, Tx_b > Tx, Tm_b > Tm, Tm_b < Tx_b) is found by the kernels: its
// outputs are zeroed, the others are untouched, and the first such utterance is reported in the workspace header
// (mtts_mas_status).  Lengths are clamped before they index anything.
#include "host.h"
#include "device_utils.h"

#include <string>

namespace mtts {

constexpr int MAS_MAX_TX = 1024;
constexpr int MAS_HEADER_BYTES = 256;      // int32: [0] 1 + first bad utterance or 0, [1] its Tx_b, [2] its Tm_b, [3] Tx, [4] Tm
constexpr int MAS_LP_FC = 16;              // features per LDS chunk of the log-prior kernel

struct MasArgs {
    const float* lpT;            // [B][Tm][ldx] frame-major log-prior
    const int64_t* x_len;        // [B]
    const int64_t* y_len;        // [B]
    int B, Tx, Tm, ldx;
    uint32_t* dec;               // [B][dec_rows][64] decision bits
    int dec_rows;
    int32_t* start;              // [B][Tx + 1] first frame of every token (Tm_b from Tx_b on)
    int32_t* durations;          // [B][Tx]
    float* score;                // [B] or null
    int32_t* status;             // workspace header
};

__device__ __forceinline__ bool mas_bad(int64_t xl, int64_t yl, int Tx, int Tm) { return xl < 1 || xl > Tx || yl > Tm || yl < xl; }

// ---------------------------------------------------------------------------------------------- log-prior
template <bool FRAME_MAJOR>
__global__ __launch_bounds__(256) void mas_logprior_kernel(const float* __restrict__ mu, const float* __restrict__ yv,
                                                           const int64_t* __restrict__ x_len, const int64_t* __restrict__ y_len,
                                                           int F, int Tx, int Tm, float* __restrict__ out, int ldx) {
    __shared__ float ms[MAS_LP_FC][64], ys[MAS_LP_FC][64];
    const int b = blockIdx.z, tid = threadIdx.x;
    const int x0 = blockIdx.y * 64, y0 = blockIdx.x * 64;
    const int txb = (int)min(max(x_len[b], (int64_t)0), (int64_t)Tx), tmb = (int)min(max(y_len[b], (int64_t)0), (int64_t)Tm);
    // the 16 fast threads run along the output's contiguous dimension; a thread's 4 x 4 cells are 16 apart in both
    const int ix = FRAME_MAJOR ? (tid & 15) : (tid >> 4), iy = FRAME_MAJOR ? (tid >> 4) : (tid & 15);
    float acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = 0.f;
    for (int f0 = 0; f0 < F; f0 += MAS_LP_FC) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int e = tid + 256 * i, f = f0 + (e >> 6), c = e & 63;
            ms[e >> 6][c] = (f < F && x0 + c < txb) ? mu[((size_t)b * F + f) * Tx + x0 + c] : 0.f;
            ys[e >> 6][c] = (f < F && y0 + c < tmb) ? yv[((size_t)b * F + f) * Tm + y0 + c] : 0.f;
        }
        __syncthreads();
#pragma unroll
        for (int f = 0; f < MAS_LP_FC; ++f) {
            float a[4], c[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) { a[i] = ms[f][ix + 16 * i]; c[i] = ys[f][iy + 16 * i]; }
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const float d = c[j] - a[i];
                    acc[i][j] = __builtin_fmaf(d, d, acc[i][j]);
                }
        }
        __syncthreads();
    }
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int x = x0 + ix + 16 * i, y = y0 + iy + 16 * j;
            const float val = (x < txb && y < tmb) ? -0.5f * acc[i][j] : 0.f;
            if (FRAME_MAJOR) {
                if (y < Tm && x < ldx) out[((size_t)b * Tm + y) * ldx + x] = val;
            } else {
                if (x < Tx && y < Tm) out[((size_t)b * Tx + x) * Tm + y] = val;
            }
        }
}

// lp [B][Tx][Tm] (the reference's layout) -> frame-major [B][Tm][ldx]; cells beyond an utterance's own lengths are not read
__global__ __launch_bounds__(256) void mas_transpose_kernel(const float* __restrict__ lp, const int64_t* __restrict__ x_len,
                                                            const int64_t* __restrict__ y_len, int Tx, int Tm, int ldx,
                                                            float* __restrict__ lpT) {
    __shared__ float t[32][33];
    const int b = blockIdx.z, x0 = blockIdx.y * 32, y0 = blockIdx.x * 32;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const int txb = (int)min(max(x_len[b], (int64_t)0), (int64_t)Tx), tmb = (int)min(max(y_len[b], (int64_t)0), (int64_t)Tm);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int x = x0 + ty + 8 * i, y = y0 + tx;
        t[ty + 8 * i][tx] = (x < txb && y < tmb) ? lp[((size_t)b * Tx + x) * Tm + y] : 0.f;
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int y = y0 + ty + 8 * i, x = x0 + tx;
        if (y < Tm && x < ldx) lpT[((size_t)b * Tm + y) * ldx + x] = t[tx][ty + 8 * i];
    }
}

// ---------------------------------------------------------------------------------------------- forward pass
template <int K> struct MasVec;
template <> struct MasVec<1> { using T = float; };
template <> struct MasVec<2> { using T = __attribute__((ext_vector_type(2))) float; };
template <> struct MasVec<4> { using T = __attribute__((ext_vector_type(4))) float; };

// K consecutive floats of one lane (16-byte pieces from K = 4 on; rows are 256 K bytes apart and lanes 4 K: aligned)
template <int K>
__device__ __forceinline__ void mas_load_row(const float* __restrict__ p, float (&r)[K]) {
    if constexpr (K <= 4) {
        const typename MasVec<K>::T v = *reinterpret_cast<const typename MasVec<K>::T*>(p);
        if constexpr (K == 1) r[0] = v;
        else
#pragma unroll
            for (int j = 0; j < K; ++j) r[j] = v[j];
    } else {
#pragma unroll
        for (int q = 0; q < K / 4; ++q) {
            const MasVec<4>::T v = reinterpret_cast<const MasVec<4>::T*>(p)[q];
#pragma unroll
            for (int j = 0; j < 4; ++j) r[4 * q + j] = v[j];
        }
    }
}

template <int K>
__device__ __forceinline__ void mas_load_block(const float* __restrict__ lp, int ldx, int y0, int tmb, float (&buf)[64 / K][K]) {
#pragma unroll
    for (int f = 0; f < 64 / K; ++f) {
        if (y0 + f < tmb) mas_load_row<K>(lp + (size_t)(y0 + f) * ldx, buf[f]);        // (wave-uniform: frames past the end are not read)
        else
#pragma unroll
            for (int j = 0; j < K; ++j) buf[f][j] = 0.f;
    }
}

// 64 / K frames of the recurrence on a lane's K tokens; the block's 64 decision bits of the lane go to two dwords of dec
template <int K, bool BAND>
__device__ __forceinline__ void mas_block(float (&v)[K], const float (&buf)[64 / K][K], int y0, int tmb, int x0,
                                          uint32_t* __restrict__ dec) {
    constexpr int FPB = 32 / K;
    const float ninf = -__builtin_inff();
    uint32_t w[2] = {0u, 0u};
#pragma unroll
    for (int f = 0; f < 2 * FPB; ++f) {
        const int y = y0 + f;
        if (y < tmb) {
            // the previous lane's last token; lane 0 has no left neighbour (0 at frame 0 makes v[0][0] = lp[0][0])
            const float edge = y == 0 ? 0.f : ninf;
            const float up = __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(__builtin_bit_cast(int, edge), __builtin_bit_cast(int, v[K - 1]),
                                                                                   0x138 /* wave_shr:1 */, 0xF, 0xF, false));
#pragma unroll
            for (int j = K - 1; j >= 0; --j) {
                const float left = j ? v[j - 1] : up, stay = v[j];
                const bool step = left > stay;                       // ties stay on the same token
                float l = buf[f][j];
                if (BAND) l = (x0 + j <= y) ? l : ninf;
                v[j] = (step ? left : stay) + l;
                w[f / FPB] |= step ? (1u << ((f % FPB) * K + j)) : 0u;
            }
        }
    }
    const int r = y0 / FPB;
    dec[(size_t)r * 64] = w[0];
    dec[(size_t)(r + 1) * 64] = w[1];
}

template <int K>
__global__ __launch_bounds__(64) void mas_forward_kernel(MasArgs a) {
    constexpr int D = 64 / K;                  // frames per block
    const int b = blockIdx.x, lane = threadIdx.x;
    if (b == 0) {                              // the verdict on every utterance's lengths, by one wave
        const int i = first_refused_row(a.B, [&](int r) { return mas_bad(a.x_len[r], a.y_len[r], a.Tx, a.Tm); });
        if (lane == 0) {
            a.status[0] = i < a.B ? i + 1 : 0;
            a.status[1] = i < a.B ? sat32(a.x_len[i]) : 0;
            a.status[2] = i < a.B ? sat32(a.y_len[i]) : 0;
            a.status[3] = a.Tx;
            a.status[4] = a.Tm;
        }
    }
    const int64_t xl = a.x_len[b], yl = a.y_len[b];
    if (mas_bad(xl, yl, a.Tx, a.Tm)) {
        if (lane == 0 && a.score) a.score[b] = 0.f;
        return;
    }
    const int txb = (int)xl, tmb = (int)yl;
    const int x0 = lane * K;
    const float* lp = a.lpT + (size_t)b * a.Tm * a.ldx + x0;
    uint32_t* dec = a.dec + (size_t)b * a.dec_rows * 64 + lane;
    float v[K];
#pragma unroll
    for (int j = 0; j < K; ++j) v[j] = -__builtin_inff();
    float p[D][K], q[D][K];
    mas_load_block<K>(lp, a.ldx, 0, tmb, p);
    for (int y0 = 0; y0 < tmb; y0 += 2 * D) {
        mas_load_block<K>(lp, a.ldx, y0 + D, tmb, q);
        if (y0 < 64 * K) mas_block<K, true>(v, p, y0, tmb, x0, dec);
        else mas_block<K, false>(v, p, y0, tmb, x0, dec);
        if (y0 + D >= tmb) break;
        mas_load_block<K>(lp, a.ldx, y0 + 2 * D, tmb, p);
        if (y0 + D < 64 * K) mas_block<K, true>(v, q, y0 + D, tmb, x0, dec);
        else mas_block<K, false>(v, q, y0 + D, tmb, x0, dec);
    }
    if (a.score) {
        const int xe = txb - 1;
        float s = 0.f;
#pragma unroll
        for (int j = 0; j < K; ++j) s = (xe % K == j) ? v[j] : s;
        if (lane == xe / K) a.score[b] = s;
    }
}

// ---------------------------------------------------------------------------------------------- back-track and durations
template <int K>
__global__ __launch_bounds__(64) void mas_backtrack_kernel(MasArgs a) {
    constexpr int FPB = 32 / K, R = 64 / FPB;        // frames per row of decision words; rows per group of 64 frames
    __shared__ int start[MAS_MAX_TX + 1];
    const int b = blockIdx.x, lane = threadIdx.x;
    const int64_t xl = a.x_len[b], yl = a.y_len[b];
    int32_t* dur = a.durations + (size_t)b * a.Tx;
    int32_t* sg = a.start + (size_t)b * (a.Tx + 1);
    if (mas_bad(xl, yl, a.Tx, a.Tm)) {
        for (int x = lane; x < a.Tx; x += 64) dur[x] = 0;
        for (int x = lane; x <= a.Tx; x += 64) sg[x] = 0;
        return;
    }
    const int txb = (int)xl, tmb = (int)yl;
    for (int x = lane; x <= txb; x += 64) start[x] = x < txb ? 0 : tmb;
    __syncthreads();
    const uint32_t* dec = a.dec + (size_t)b * a.dec_rows * 64 + lane;
    const int rtop = (tmb - 1) / FPB;
    int x = txb - 1;                                  // wave-uniform: the walk runs on the scalar unit
    uint32_t cur[R], nxt[R];
    int g = rtop / R;
#pragma unroll
    for (int i = 0; i < R; ++i) cur[i] = (g * R + i <= rtop) ? dec[(size_t)(g * R + i) * 64] : 0u;
    for (; g >= 0; --g) {
        if (g > 0) {
#pragma unroll
            for (int i = 0; i < R; ++i) nxt[i] = dec[(size_t)((g - 1) * R + i) * 64];
        }
#pragma unroll
        for (int i = R - 1; i >= 0; --i) {
            const int r = g * R + i;
            if (r > rtop) continue;
#pragma unroll 4
            for (int f = FPB - 1; f >= 0; --f) {
                const int y = r * FPB + f;
                if (y >= tmb) continue;
                start[x] = y;                         // frames come in descending order: the last write is the token's first frame
                if (y == 0) continue;
                const uint32_t w = __builtin_amdgcn_readlane(cur[i], (unsigned)x / K);
                const int bit = (w >> (f * K + (unsigned)x % K)) & 1u;
                x = max(x - bit, 0);
            }
        }
#pragma unroll
        for (int i = 0; i < R; ++i) cur[i] = nxt[i];
    }
    __syncthreads();
    for (int t = lane; t <= a.Tx; t += 64) {
        const int s0 = t < txb ? start[t] : tmb;
        if (t < a.Tx) dur[t] = t < txb ? start[t + 1] - s0 : 0;
        sg[t] = s0;
    }
}

// dense 0/1 path [B][Tx][Tm] from the tokens' first frames
__global__ __launch_bounds__(256) void mas_path_kernel(const int32_t* __restrict__ start, int Tx, int Tm, float* __restrict__ path) {
    const int y = blockIdx.x * 256 + threadIdx.x, x = blockIdx.y, b = blockIdx.z;
    if (y >= Tm) return;
    const int32_t* sg = start + (size_t)b * (Tx + 1);
    path[((size_t)b * Tx + x) * Tm + y] = (y >= sg[x] && y < sg[x + 1]) ? 1.f : 0.f;
}

// ---------------------------------------------------------------------------------------------- host side
static int mas_k(int Tx) {
    for (int k = 1; k <= 16; k *= 2)
        if (64 * k >= Tx) return k;
    return 0;
}
struct MasPlan { int K = 0, ldx = 0, dec_rows = 0; size_t lp = 0, dec = 0, start = 0, total = 0; };
static size_t up256(size_t n) { return (n + 255) / 256 * 256; }
static MasPlan mas_plan(int B, int Tx, int Tm) {
    MasPlan p;
    p.K = mas_k(Tx);
    p.ldx = 64 * p.K;
    const int D = 64 / p.K;                                   // frames per forward block, two decision rows each
    p.dec_rows = 2 * ((Tm + D - 1) / D);
    p.lp = MAS_HEADER_BYTES;
    p.dec = p.lp + up256((size_t)B * Tm * p.ldx * sizeof(float));
    p.start = p.dec + up256((size_t)B * p.dec_rows * 64 * sizeof(uint32_t));
    p.total = p.start + up256((size_t)B * (Tx + 1) * sizeof(int32_t));
    return p;
}
static bool mas_shape_ok(const char* who, int B, int Tx, int Tm) {
    if (B < 1 || B > 65535) { set_error(std::string(who) + ": B must be in [1, 65535]"); return false; }
    if (Tx < 1 || Tx > MAS_MAX_TX) { set_error(std::string(who) + ": Tx must be in [1, 1024]"); return false; }
    if (Tm < Tx) { set_error(std::string(who) + ": Tm < Tx (no monotone path gives every token a frame)"); return false; }
    if ((int64_t)B * Tm * 1024 > ((int64_t)1 << 40) || Tm > (1 << 24)) { set_error(std::string(who) + ": batch too large"); return false; }
    return true;
}
template <int K>
static void mas_search(const MasArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(mas_forward_kernel<K>, dim3(a.B), dim3(64), 0, s, a);
    hipLaunchKernelGGL(mas_backtrack_kernel<K>, dim3(a.B), dim3(64), 0, s, a);
}

}  // namespace mtts

using namespace mtts;

extern "C" {

int64_t mtts_mas_workspace_bytes(int B, int Tx, int Tm) {
    if (!mas_shape_ok("mtts_mas_workspace_bytes", B, Tx, Tm)) return -1;
    return (int64_t)mas_plan(B, Tx, Tm).total;
}

int mtts_mas_logprior(const float* d_mu_x, const float* d_y, const int64_t* d_x_lengths, const int64_t* d_y_lengths, int B, int F, int Tx,
                      int Tm, float* d_lp, void* stream) {
    if (!d_mu_x || !d_y || !d_x_lengths || !d_y_lengths || !d_lp) { set_error("mtts_mas_logprior: null argument"); return -1; }
    if (F < 1) { set_error("mtts_mas_logprior: F < 1"); return -1; }
    if (!mas_shape_ok("mtts_mas_logprior", B, Tx, Tm)) return -1;
    hipLaunchKernelGGL(mas_logprior_kernel<false>, dim3((Tm + 63) / 64, (Tx + 63) / 64, B), dim3(256), 0, static_cast<hipStream_t>(stream),
                       d_mu_x, d_y, d_x_lengths, d_y_lengths, F, Tx, Tm, d_lp, 0);
    return launched("mas_logprior_kernel");
}

int mtts_mas(const float* d_lp, const float* d_mu_x, const float* d_y, const int64_t* d_x_lengths, const int64_t* d_y_lengths, int B, int F,
             int Tx, int Tm, int32_t* d_durations, float* d_path, float* d_score, void* d_ws, int64_t ws_bytes, void* stream) {
    if (!d_x_lengths || !d_y_lengths || !d_durations || !d_ws) { set_error("mtts_mas: null argument"); return -1; }
    if (!d_lp && (!d_mu_x || !d_y)) { set_error("mtts_mas: neither a log-prior nor mu_x and y"); return -1; }
    if (!d_lp && F < 1) { set_error("mtts_mas: F < 1"); return -1; }
    if (!mas_shape_ok("mtts_mas", B, Tx, Tm)) return -1;
    const MasPlan p = mas_plan(B, Tx, Tm);
    if (ws_bytes < (int64_t)p.total) { set_error("mtts_mas: workspace too small (mtts_mas_workspace_bytes)"); return -1; }
    if (reinterpret_cast<uintptr_t>(d_ws) & 15) { set_error("mtts_mas: workspace must be 16-byte aligned"); return -1; }
    hipStream_t s = static_cast<hipStream_t>(stream);
    char* ws = static_cast<char*>(d_ws);
    float* lpT = reinterpret_cast<float*>(ws + p.lp);
    if (d_lp) {
        hipLaunchKernelGGL(mas_transpose_kernel, dim3((Tm + 31) / 32, p.ldx / 32, B), dim3(256), 0, s, d_lp, d_x_lengths, d_y_lengths, Tx, Tm,
                           p.ldx, lpT);
        if (launched("mas_transpose_kernel")) return -1;
    } else {
        hipLaunchKernelGGL(mas_logprior_kernel<true>, dim3((Tm + 63) / 64, p.ldx / 64, B), dim3(256), 0, s, d_mu_x, d_y, d_x_lengths,
                           d_y_lengths, F, Tx, Tm, lpT, p.ldx);
        if (launched("mas_logprior_kernel")) return -1;
    }
    MasArgs a;
    a.lpT = lpT; a.x_len = d_x_lengths; a.y_len = d_y_lengths;
    a.B = B; a.Tx = Tx; a.Tm = Tm; a.ldx = p.ldx;
    a.dec = reinterpret_cast<uint32_t*>(ws + p.dec); a.dec_rows = p.dec_rows;
    a.start = reinterpret_cast<int32_t*>(ws + p.start);
    a.durations = d_durations; a.score = d_score; a.status = reinterpret_cast<int32_t*>(ws);
    switch (p.K) {
        case 1: mas_search<1>(a, s); break;
        case 2: mas_search<2>(a, s); break;
        case 4: mas_search<4>(a, s); break;
        case 8: mas_search<8>(a, s); break;
        default: mas_search<16>(a, s); break;
    }
    if (launched("mas_forward_kernel / mas_backtrack_kernel")) return -1;
    if (d_path) {
        hipLaunchKernelGGL(mas_path_kernel, dim3((Tm + 255) / 256, Tx, B), dim3(256), 0, s, a.start, Tx, Tm, d_path);
        if (launched("mas_path_kernel")) return -1;
    }
    return 0;
}

// The lengths check's verdict (the header of the call's workspace).  The one entry of this file that waits for the stream.
int mtts_mas_status(const void* d_ws, void* stream) {
    int st[5];
    if (read_status("mtts_mas_status", d_ws, stream, st)) return -1;
    if (st[0] != 0) {
        set_error("mtts_mas: utterance " + std::to_string(st[0] - 1) + " has x_length = " + std::to_string(st[1]) + ", y_length = " +
                  std::to_string(st[2]) + " (need 1 <= x_length <= Tx = " + std::to_string(st[3]) + " and x_length <= y_length <= Tm = " +
                  std::to_string(st[4]) + ")");
        return -1;
    }
    return 0;
}

}  // extern "C"
