// Speaker-row gradients: d(prior Huber sum) / d e_enc and d(duration Huber sum) / d e_dur per utterance, for fine-tuning a voice from
// recordings (reference matcha/finetune_speaker.py: everything frozen but one row of each speaker table).
//
// What the reference's training forward lets reach the two rows (matcha/models/matcha_tts.py, components/text_encoder.py):
//   * the flow-matching loss does not: mu_y is detached before decoder.compute_loss (matcha_tts.py:154-162) and the estimator has
//     no speaker input -- no decoder backward exists here;
//   * e_dur is seen by the duration predictor alone, whose input is x.detach() (text_encoder.py:404): FiLM, channel LayerNorm, ReLU
//     and the k5 convolutions of layers >= 1, then spk_proj transposed;
//   * e_enc is concatenated behind the prenet (text_encoder.py:400): proj_m, the post-LN encoder layers and a token sum of the
//     speaker channels; no prenet, embedding or weight gradient;
//   * MAS runs under no_grad (matcha_tts.py:187): durations are constants of the step.
//
//   taped forward        the launch sequence of mtts_text_encoder_forward (encoder.hip), same launchers and arguments, with the
//                        intermediates of every layer kept in buffers of their own
//   seed_mu / seed_logw  the two Huber derivatives, token-of-frame rule and verdicts of score.hip
//   seed_match_*         the seeds and sums of the style-training loss (mtts_spk_grad_match): smooth-L1 against the outputs under the
//                        real rows, the same taped forward and the same walks back (SgCall)
//   ln_bwd_kernel        channel LayerNorm backward (+ SiLU' on the way in, FiLM, row mask, ReLU gate on the way out)
//   attn_bwd_q / _kv     RoPE attention backward: dq per query thread, dk / dv per key thread, inverse rotation at the store
//   gate / colsum        SiLU' and ReLU gates, fixed-order sums over an utterance's tokens
//
// Backward arithmetic: the data-gradient GEMMs run on the existing launchers with transposed / tap-reversed panels in NATIVE FP32
// MFMA (GemmArgs::terms 0) whatever the context's forward arithmetic is: gradients are small numbers, and the fp16 two-term split
// loses bits below the fp16 normal range.  The panels live in a buffer of their own (mtts_spk_grad_upload_weights), not in the
// weight image.  The attention backward is plain fp32 FMA, one thread per query (key) row with the other side broadcast from LDS,
// not the matrix pipe: 10 B H Tx^2 D flops per layer (0.15 GFLOP at B = 32, Tx = 128, 6 heads of 48; 10 GFLOP at Tx = 1024).  Measured
// at B = 32 x 128 tokens (profiles/r11_spk_grad.md) it takes 1.23 ms of a 5.4 ms call beside 2.17 ms for all backward GEMMs: latency of
// 192 two-wave workgroups, not arithmetic.  Splitting a row's keys over several threads or a 16x16x4 fp32 MFMA tiling (fits D = 48) is
// the open next step.
//
// Every sum has a FIXED ORDER and there are no floating-point atomics (the rule of score.hip and mas.hip): a thread's serial run in
// key / query / frame / token order, a wave butterfly, four phases combined in order.  Partitions depend on absolute token indices
// only, so an utterance's gradient does not depend on its batch or on the padded shapes.
#include "spk_grad.h"
#include "device_utils.h"

#include <string>

namespace mtts {

// (SG_MAX_TX, SG_SCORE_OFF, SG_MAX_LAYERS, LnBwdArgs, SgBufs and SgCall: spk_grad.h, shared with dp_grad.hip)

__device__ __forceinline__ float sg_wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
__device__ __forceinline__ float sg_sigmoid(float z) { return 1.0f / (1.0f + expf(-z)); }
__device__ __forceinline__ float sg_silu_grad(float z) {
    const float sg = sg_sigmoid(z);
    return sg * (1.0f + z * (1.0f - sg));
}
__device__ __forceinline__ float sg_clamp(float d, float delta) { return fminf(fmaxf(d, -delta), delta); }

// ---------------------------------------------------------------------------------------------- channel LayerNorm backward
// forward (norm_glue.hip layernorm_kernel):  xh = (x - mean) rstd;  a = xh gamma + beta;  [a = silu(a)];  [y = a fg_b + fb_b];  [y *= mask]
__global__ __launch_bounds__(256) void ln_bwd_kernel(const LnBwdArgs p) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (row >= p.M) return;
    const float* xr = p.x + (size_t)row * p.ldx;
    const float* dr = p.dy + (size_t)row * p.lddy;
    float* out = p.dx + (size_t)row * p.lddx;
    float* fp = p.film_prod ? p.film_prod + (size_t)row * p.C : nullptr;
    if (p.mask && p.mask[row] == 0.f) {
        for (int c = lane; c < p.C; c += 64) { out[c] = 0.f; if (fp) fp[c] = 0.f; }
        return;
    }
    float s = 0.f;
    for (int c = lane; c < p.C; c += 64) s += xr[c];
    const float mu = sg_wave_sum(s) / (float)p.C;
    float q = 0.f;
    for (int c = lane; c < p.C; c += 64) { const float d = xr[c] - mu; q += d * d; }
    const float rs = 1.0f / sqrtf(sg_wave_sum(q) / (float)p.C + p.eps);
    const float* film = p.film ? p.film + (size_t)(row / p.T) * 2 * p.C : nullptr;
    // g = d loss / d xh
    auto grad_xh = [&](int c, float xh, bool store) {
        const float ga = p.gamma ? p.gamma[c] : 1.0f;
        float a = xh * ga + (p.beta ? p.beta[c] : 0.f);
        float d = dr[c];
        if (film) {
            const float av = p.act == ACT_SILU ? a * sg_sigmoid(a) : a;
            if (store && fp) fp[c] = d * av;
            d *= film[c];
        }
        if (p.act == ACT_SILU) d *= sg_silu_grad(a);
        return d * ga;
    };
    float s1 = 0.f, s2 = 0.f;
    for (int c = lane; c < p.C; c += 64) {
        const float xh = (xr[c] - mu) * rs;
        const float g = grad_xh(c, xh, true);
        s1 += g;
        s2 += g * xh;
    }
    const float m1 = sg_wave_sum(s1) / (float)p.C, m2 = sg_wave_sum(s2) / (float)p.C;
    for (int c = lane; c < p.C; c += 64) {
        const float xv = xr[c];
        const float xh = (xv - mu) * rs;
        float d = rs * ((grad_xh(c, xh, false) - m1) - xh * m2);
        if (p.gate == ACT_RELU && !(xv > 0.f)) d = 0.f;
        out[c] = d;
    }
}
hipError_t launch_ln_bwd(const LnBwdArgs& a, hipStream_t s) {
    if (!a.x || !a.dy || !a.dx || a.M <= 0 || a.C <= 0 || a.T <= 0 || a.ldx < a.C || a.lddy < a.C || a.lddx < a.C) return hipErrorInvalidValue;
    if (a.film_prod && !a.film) return hipErrorInvalidValue;
    hipLaunchKernelGGL(ln_bwd_kernel, dim3((a.M + 3) / 4), dim3(256), 0, s, a);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------- gates
// mode 0: g *= silu'(ref);  1: g *= (ref > 0) * mask[row], ref fp32 rows;  2: the same with ref a P16 image (32 heads then 32
// residuals per 32-channel group): a ReLU output is positive iff its head is, or the head is zero and the residual positive
__global__ void gate_kernel(float* __restrict__ g, int ldg, int M, int C, int mode, const float* __restrict__ ref, int ldref,
                            const _Float16* __restrict__ ref16, int ld16, const float* __restrict__ mask) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (size_t)M * C) return;
    const int row = (int)(i / C), c = (int)(i % C);
    float* gp = g + (size_t)row * ldg + c;
    if (mode == 0) { *gp = *gp * sg_silu_grad(ref[(size_t)row * ldref + c]); return; }
    bool on;
    if (mode == 1) on = ref[(size_t)row * ldref + c] > 0.f;
    else {
        const _Float16* grp = ref16 + (size_t)row * ld16 + (c >> 5) * 64 + (c & 31);
        const float h = (float)grp[0], r = (float)grp[32];
        on = h > 0.f || (h == 0.f && r > 0.f);
    }
    if (mask && mask[row] == 0.f) on = false;
    if (!on) *gp = 0.f;
}
static hipError_t launch_gate(float* g, int ldg, int M, int C, int mode, const float* ref, int ldref, const _Float16* ref16, int ld16,
                              const float* mask, hipStream_t s) {
    if (!g || M <= 0 || C <= 0 || ldg < C || (mode == 2 ? (!ref16 || ld16 < 2 * C || (C & 31)) : (!ref || ldref < C))) return hipErrorInvalidValue;
    const size_t n = (size_t)M * C;
    hipLaunchKernelGGL(gate_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, g, ldg, M, C, mode, ref, ldref, ref16, ld16, mask);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------- token sums
// dst[b][dcol0 + c] (+)= sum over t < len_b of src[(b T + t) ld + col0 + c], c < C: four phases t = p, p + 4, ... in token order,
// combined as ((p0 + p1) + p2) + p3.  len null: T.  verdict (score.hip, [B][2]) != 0: the utterance's sums are zero.
__global__ __launch_bounds__(256) void colsum_kernel(const float* __restrict__ src, int ld, int col0, int C, int T, const int64_t* __restrict__ len,
                                                     const int32_t* __restrict__ verdict, float* __restrict__ dst, int ldd, int dcol0, int accumulate) {
    __shared__ float part[4][64];
    const int b = blockIdx.y, cl = threadIdx.x & 63, ph = threadIdx.x >> 6;
    const int c = blockIdx.x * 64 + cl;
    int n = T;
    if (len) { const int64_t v = len[b]; n = v < 0 ? 0 : v > T ? T : (int)v; }
    if (verdict && verdict[2 * b] != 0) n = 0;
    float s = 0.f;
    if (c < C)
        for (int t = ph; t < n; t += 4) s += src[((size_t)b * T + t) * ld + col0 + c];
    part[ph][cl] = s;
    __syncthreads();
    if (ph == 0 && c < C) {
        const float v = ((part[0][cl] + part[1][cl]) + part[2][cl]) + part[3][cl];
        float* d = dst + (size_t)b * ldd + dcol0 + c;
        *d = accumulate ? *d + v : v;
    }
}
hipError_t launch_colsum(const float* src, int ld, int col0, int C, int B, int T, const int64_t* len, const int32_t* verdict, float* dst,
                         int ldd, int dcol0, int accumulate, hipStream_t s) {
    if (!src || !dst || B <= 0 || T <= 0 || C <= 0 || ld < col0 + C || ldd < dcol0 + C) return hipErrorInvalidValue;
    hipLaunchKernelGGL(colsum_kernel, dim3((C + 63) / 64, B), dim3(256), 0, s, src, ld, col0, C, T, len, verdict, dst, ldd, dcol0, accumulate);
    return hipGetLastError();
}

__global__ void copy_i32_kernel(const int32_t* __restrict__ src, int32_t* __restrict__ dst, size_t n) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) dst[i] = src[i];
}

// ---------------------------------------------------------------------------------------------- loss seeds
// d prior_sum_b / d mu_x[f, x] = - sum over the frames y of token x of clamp(y_fine[f, y] - mu_x[f, x], +-delta), written as the
// channels-last rows of proj_m's output [B Tx][ldm] (zero-filled beforehand: rows beyond an utterance and the padding columns stay
// zero).  Workgroup (f, b); the frames of a token are [cum[x-1], cum[x]) of the inclusive cumulative durations, which is the
// token-of-frame rule of score_prior_dur_kernel read the other way round; an utterance score.hip refused (verdict) gets no seed.
__global__ __launch_bounds__(256) void seed_mu_kernel(const float* __restrict__ mu_x, const float* __restrict__ y, const int32_t* __restrict__ dur,
                                                      const int64_t* __restrict__ x_len, const int32_t* __restrict__ verdict, int F, int Tx,
                                                      int Tm, float delta, float* __restrict__ g, int ldm) {
    __shared__ int cum[SG_MAX_TX];
    __shared__ int scan[256];
    const int f = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
    if (verdict[2 * b] != 0) return;              // (uniform per workgroup)
    const int txb = (int)x_len[b];                // verdict 0: 1 <= x_len <= Tx, durations in [0, Tm] that sum to y_len <= Tm
    const int32_t* db = dur + (size_t)b * Tx;
    int v[4], run = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int x = 4 * tid + k;
        run += x < txb ? db[x] : 0;
        v[k] = run;
    }
    scan[tid] = run;
    __syncthreads();
    for (int off = 1; off < 256; off <<= 1) {
        const int add = tid >= off ? scan[tid - off] : 0;
        __syncthreads();
        scan[tid] += add;
        __syncthreads();
    }
    const int base = tid ? scan[tid - 1] : 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) cum[4 * tid + k] = base + v[k];
    __syncthreads();
    const float* yr = y + ((size_t)b * F + f) * Tm;
    const float* mr = mu_x + ((size_t)b * F + f) * Tx;
    for (int x = tid; x < txb; x += 256) {
        const int y0 = x ? cum[x - 1] : 0, y1 = min(cum[x], Tm);
        const float m = mr[x];
        float acc = 0.f;
        for (int t = y0; t < y1; ++t) acc += sg_clamp(yr[t] - m, delta);
        g[((size_t)b * Tx + x) * ldm + f] = -acc;
    }
}
// d dur_sum_b / d logw[x] = clamp(logw[x] - log(2 + dur[x]), +-delta) for x < Tx_b of an accepted utterance, else 0, carried through
// the duration predictor's output projection (Conv1d(F, 1, 1) over masked rows, masked): gd[row][c] = seed * w_proj[c].  The
// projection has one output channel, so its transposed "GEMM" is this outer product -- exact, no K = 1 panel.
__global__ void seed_logw_kernel(const float* __restrict__ logw, const int32_t* __restrict__ dur, const int64_t* __restrict__ x_len,
                                 const int32_t* __restrict__ verdict, const float* __restrict__ w_proj, int Tx, int Fd, float delta,
                                 float* __restrict__ gd) {
    const int row = blockIdx.x, b = row / Tx, x = row % Tx;
    float seed = 0.f;
    if (verdict[2 * b] == 0 && x < (int)x_len[b]) seed = sg_clamp(logw[row] - logf(2.0f + (float)dur[row]), delta);
    for (int c = threadIdx.x; c < Fd; c += blockDim.x) gd[(size_t)row * Fd + c] = seed * w_proj[c];
}

// ---------------------------------------------------------------------------------------------- matching-loss seeds (style training)
// The reference's style-encoder loss (style_encoder.py:119-143): smooth-L1 between the frozen text encoder's outputs under predicted
// rows and under the real rows (ref: constants), per term 0.5 d^2 / beta below beta and |d| - 0.5 beta from beta on, whose derivative
// is clamp(d / beta, -1, 1).
__device__ __forceinline__ float sg_smooth_l1(float d, float beta) {
    const float ad = fabsf(d);
    return ad < beta ? 0.5f * d * d / beta : ad - 0.5f * beta;
}
__device__ __forceinline__ float sg_smooth_l1_grad(float d, float beta) { return fminf(fmaxf(d / beta, -1.0f), 1.0f); }

// verdict [B][2] = (1: x_length outside [1, Tx], 0) in score.hip's layout, which the walks read, and the status words
// (1 + first refused utterance or 0, its length, Tx) for mtts_spk_grad_match_status.  One workgroup.
__global__ __launch_bounds__(256) void match_verdict_kernel(const int64_t* __restrict__ x_len, int B, int Tx, int32_t* __restrict__ status,
                                                            int32_t* __restrict__ verdict) {
    for (int b = threadIdx.x; b < B; b += blockDim.x) {
        verdict[2 * b] = (x_len[b] < 1 || x_len[b] > Tx) ? 1 : 0;
        verdict[2 * b + 1] = 0;
    }
    const int i = first_refused_row(B, [&](int r) { return x_len[r] < 1 || x_len[r] > Tx; });
    if (threadIdx.x == 0) {
        status[0] = i < B ? i + 1 : 0;
        status[1] = i < B ? sat32(x_len[i]) : 0;
        status[2] = Tx;
    }
}
// g[(b Tx + x) ldm + f] = clamp((mu_x - mu_ref)[b, f, x] / beta, +-1) for x < len_b (g zero-filled beforehand), and
// part[b][f] = the smooth-L1 sum of feature f over the tokens.  Workgroup (f, b), as seed_mu_kernel; a thread adds its tokens x = tid,
// tid + 256, ... in order, a wave butterfly, the four waves in order.
__global__ __launch_bounds__(256) void seed_match_mu_kernel(const float* __restrict__ mu_x, const float* __restrict__ mu_ref,
                                                            const int64_t* __restrict__ x_len, const int32_t* __restrict__ verdict, int F, int Tx,
                                                            float beta, float* __restrict__ g, int ldm, float* __restrict__ part) {
    __shared__ float wsum[4];
    const int f = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
    if (verdict[2 * b] != 0) {                    // (uniform per workgroup)
        if (tid == 0) part[(size_t)b * F + f] = 0.f;
        return;
    }
    const int txb = (int)x_len[b];                // verdict 0: 1 <= x_len <= Tx
    const float* mr = mu_x + ((size_t)b * F + f) * Tx;
    const float* rr = mu_ref + ((size_t)b * F + f) * Tx;
    float acc = 0.f;
    for (int x = tid; x < txb; x += 256) {
        const float d = mr[x] - rr[x];
        acc += sg_smooth_l1(d, beta);
        g[((size_t)b * Tx + x) * ldm + f] = sg_smooth_l1_grad(d, beta);
    }
    acc = sg_wave_sum(acc);
    if ((tid & 63) == 0) wsum[tid >> 6] = acc;
    __syncthreads();
    if (tid == 0) part[(size_t)b * F + f] = ((wsum[0] + wsum[1]) + wsum[2]) + wsum[3];
}
// as seed_logw_kernel with the matching seed: gd[row][c] = clamp((logw - logw_ref)[row] / beta, +-1) * w_proj[c] for x < len_b, else 0
__global__ void seed_match_logw_kernel(const float* __restrict__ logw, const float* __restrict__ logw_ref, const int64_t* __restrict__ x_len,
                                       const int32_t* __restrict__ verdict, const float* __restrict__ w_proj, int Tx, int Fd, float beta,
                                       float* __restrict__ gd) {
    const int row = blockIdx.x, b = row / Tx, x = row % Tx;
    float seed = 0.f;
    if (verdict[2 * b] == 0 && x < (int)x_len[b]) seed = sg_smooth_l1_grad(logw[row] - logw_ref[row], beta);
    for (int c = threadIdx.x; c < Fd; c += blockDim.x) gd[(size_t)row * Fd + c] = seed * w_proj[c];
}
// One wave per utterance: ac_sum[b] = the features' partial sums (lane f, f + 64, ... in order, then a butterfly); rh_sum[b] = the
// smooth-L1 sum of logw over the tokens (lane x, x + 64, ...).  Zero for a refused utterance.
__global__ __launch_bounds__(64) void match_finish_kernel(const float* __restrict__ part, const float* __restrict__ logw,
                                                          const float* __restrict__ logw_ref, const int64_t* __restrict__ x_len,
                                                          const int32_t* __restrict__ verdict, int F, int Tx, float beta,
                                                          float* __restrict__ ac_sum, float* __restrict__ rh_sum) {
    const int b = blockIdx.x, lane = threadIdx.x;
    const bool ok = verdict[2 * b] == 0;
    const int txb = ok ? (int)x_len[b] : 0;
    float a = 0.f, r = 0.f;
    if (ok)
        for (int f = lane; f < F; f += 64) a += part[(size_t)b * F + f];
    for (int x = lane; x < txb; x += 64) r += sg_smooth_l1(logw[(size_t)b * Tx + x] - logw_ref[(size_t)b * Tx + x], beta);
    a = sg_wave_sum(a);
    r = sg_wave_sum(r);
    if (lane == 0) {
        ac_sum[b] = a;
        rh_sum[b] = r;
    }
}

// ---------------------------------------------------------------------------------------------- RoPE attention backward
// Encoder SDPA (reference text_encoder.py:220-237): boolean query x key mask, rotary on the first D / 2 dims of q and k.  Inputs are
// the saved rows AFTER the rotation (qkv [B T][3 H D]: q | k | v sections, head h at h D), the attention output o and the upstream
// gradient d_o [B T][H D].  With P = softmax(scale q k^T) over the keys j < len_b, Delta_i = <dO_i, O_i>:
//   dS = P o (dO V^T - Delta),  dq = scale dS K,  dk = scale dS^T Q,  dv = P^T dO,
// then the transposed rotation on dq and dk.  Rows at or beyond len_b get zeros and are never read as data.
//   attn_bwd_q_kernel:  thread = query i; pass 1 the running maximum and sum over the keys in key order (kept for the second kernel
//                       in stats [B][H][T][3] = (max, 1 / sum, Delta)), pass 2 dq in key order.  K / V tiles of 32 rows in LDS, read
//                       by all threads at the same address (broadcast).
//   attn_bwd_kv_kernel: thread = key j; dk, dv in query order from Q / dO tiles and the statistics.
// Both recompute p = exp(s - max) / sum with the same expression, so the two kernels see the same probabilities.
constexpr int AB_ROWS = 128, AB_TILE = 32;
struct AttnBwdArgs {
    const float* qkv; const float* o; const float* d_o; const int64_t* len;
    int B, T, H, D;
    float scale;
    const float* cos_t; const float* sin_t;       // [>= T][D / 2]
    float* dqkv; float* stats;
};
template <int D>
__device__ __forceinline__ void unrope_store(const float (&acc)[D], int t, const float* cos_t, const float* sin_t, float* dst) {
    constexpr int R = D / 2, HALF = R / 2;
    float out[D];
#pragma unroll
    for (int k = 0; k < D; ++k) out[k] = acc[k];
#pragma unroll
    for (int k = 0; k < HALF; ++k) {
        const float c0 = cos_t[(size_t)t * R + k], s0 = sin_t[(size_t)t * R + k];
        const float c1 = cos_t[(size_t)t * R + k + HALF], s1 = sin_t[(size_t)t * R + k + HALF];
        // forward: y_k = a c0 - b s0, y_{k+half} = b c1 + a s1
        out[k] = acc[k] * c0 + acc[k + HALF] * s1;
        out[k + HALF] = acc[k + HALF] * c1 - acc[k] * s0;
    }
#pragma unroll
    for (int k = 0; k < D; ++k) dst[k] = out[k];
}
template <int D>
__global__ __launch_bounds__(AB_ROWS) void attn_bwd_q_kernel(const AttnBwdArgs p) {
    __shared__ float Ks[AB_TILE][D];
    __shared__ float Vs[AB_TILE][D];
    const int b = blockIdx.z, h = blockIdx.y, tid = threadIdx.x;
    const int i = blockIdx.x * AB_ROWS + tid;
    const int64_t l64 = p.len[b];
    const int len = l64 < 0 ? 0 : l64 > p.T ? p.T : (int)l64;
    const int ldq = 3 * p.H * D, ldo = p.H * D;
    const bool live = i < len;
    const int nkeys = blockIdx.x * AB_ROWS < len ? len : 0;        // a workgroup whose rows all lie beyond the utterance only writes zeros
    float q[D], go[D], acc[D];
    float delta = 0.f;
    if (live) {
        const float* qr = p.qkv + ((size_t)b * p.T + i) * ldq + h * D;
        const float* gr = p.d_o + ((size_t)b * p.T + i) * ldo + h * D;
        const float* orow = p.o + ((size_t)b * p.T + i) * ldo + h * D;
#pragma unroll
        for (int k = 0; k < D; ++k) { q[k] = qr[k]; go[k] = gr[k]; delta = fmaf(go[k], orow[k], delta); }
    } else {
#pragma unroll
        for (int k = 0; k < D; ++k) { q[k] = 0.f; go[k] = 0.f; }
    }
#pragma unroll
    for (int k = 0; k < D; ++k) acc[k] = 0.f;
    float m = -INFINITY, l = 0.f;
    for (int pass = 0; pass < 2; ++pass) {
        const float inv = pass ? 1.0f / l : 0.f;
        for (int j0 = 0; j0 < nkeys; j0 += AB_TILE) {
            __syncthreads();
            for (int e = tid; e < AB_TILE * D; e += AB_ROWS) {
                const int jj = e / D, k = e % D;
                const int j = j0 + jj;
                const float* base = p.qkv + ((size_t)b * p.T + (j < len ? j : 0)) * ldq + h * D + k;
                Ks[jj][k] = j < len ? base[p.H * D] : 0.f;
                Vs[jj][k] = j < len ? base[2 * p.H * D] : 0.f;
            }
            __syncthreads();
            const int nj = min(AB_TILE, len - j0);
            for (int jj = 0; jj < nj; ++jj) {
                float s = 0.f;
#pragma unroll
                for (int k = 0; k < D; ++k) s = fmaf(q[k], Ks[jj][k], s);
                s *= p.scale;
                if (pass == 0) {
                    const float mn = fmaxf(m, s);
                    l = l * expf(m - mn) + expf(s - mn);
                    m = mn;
                } else {
                    const float pr = expf(s - m) * inv;
                    float dp = 0.f;
#pragma unroll
                    for (int k = 0; k < D; ++k) dp = fmaf(go[k], Vs[jj][k], dp);
                    const float ds = pr * (dp - delta) * p.scale;
#pragma unroll
                    for (int k = 0; k < D; ++k) acc[k] = fmaf(ds, Ks[jj][k], acc[k]);
                }
            }
        }
    }
    if (i < p.T) {
        float* dst = p.dqkv + ((size_t)b * p.T + i) * ldq + h * D;
        if (live) {
            unrope_store<D>(acc, i, p.cos_t, p.sin_t, dst);
            float* st = p.stats + (((size_t)b * p.H + h) * p.T + i) * 3;
            st[0] = m; st[1] = 1.0f / l; st[2] = delta;
        } else {
#pragma unroll
            for (int k = 0; k < D; ++k) dst[k] = 0.f;
        }
    }
}
template <int D>
__global__ __launch_bounds__(AB_ROWS) void attn_bwd_kv_kernel(const AttnBwdArgs p) {
    __shared__ float Qs[AB_TILE][D];
    __shared__ float Gs[AB_TILE][D];
    __shared__ float St[AB_TILE][3];
    const int b = blockIdx.z, h = blockIdx.y, tid = threadIdx.x;
    const int j = blockIdx.x * AB_ROWS + tid;
    const int64_t l64 = p.len[b];
    const int len = l64 < 0 ? 0 : l64 > p.T ? p.T : (int)l64;
    const int ldq = 3 * p.H * D, ldo = p.H * D;
    const bool live = j < len;
    const int nqueries = blockIdx.x * AB_ROWS < len ? len : 0;     // as in attn_bwd_q_kernel
    float kr[D], vr[D], dk[D], dv[D];
    if (live) {
        const float* base = p.qkv + ((size_t)b * p.T + j) * ldq + h * D;
#pragma unroll
        for (int k = 0; k < D; ++k) { kr[k] = base[p.H * D + k]; vr[k] = base[2 * p.H * D + k]; }
    } else {
#pragma unroll
        for (int k = 0; k < D; ++k) { kr[k] = 0.f; vr[k] = 0.f; }
    }
#pragma unroll
    for (int k = 0; k < D; ++k) { dk[k] = 0.f; dv[k] = 0.f; }
    for (int i0 = 0; i0 < nqueries; i0 += AB_TILE) {
        __syncthreads();
        for (int e = tid; e < AB_TILE * D; e += AB_ROWS) {
            const int ii = e / D, k = e % D;
            const int i = i0 + ii;
            const size_t r = (size_t)b * p.T + (i < len ? i : 0);
            Qs[ii][k] = i < len ? p.qkv[r * ldq + h * D + k] : 0.f;
            Gs[ii][k] = i < len ? p.d_o[r * ldo + h * D + k] : 0.f;
        }
        if (tid < AB_TILE * 3) {
            const int ii = tid / 3, w = tid % 3;
            const int i = i0 + ii;
            St[ii][w] = i < len ? p.stats[(((size_t)b * p.H + h) * p.T + i) * 3 + w] : 0.f;
        }
        __syncthreads();
        const int ni = min(AB_TILE, len - i0);
        for (int ii = 0; ii < ni; ++ii) {
            float s = 0.f, dp = 0.f;
#pragma unroll
            for (int k = 0; k < D; ++k) { s = fmaf(Qs[ii][k], kr[k], s); dp = fmaf(Gs[ii][k], vr[k], dp); }
            s *= p.scale;
            const float pr = expf(s - St[ii][0]) * St[ii][1];
            const float ds = pr * (dp - St[ii][2]) * p.scale;
#pragma unroll
            for (int k = 0; k < D; ++k) { dv[k] = fmaf(pr, Gs[ii][k], dv[k]); dk[k] = fmaf(ds, Qs[ii][k], dk[k]); }
        }
    }
    if (j < p.T) {
        float* dst = p.dqkv + ((size_t)b * p.T + j) * ldq + h * D;
        if (live) {
            unrope_store<D>(dk, j, p.cos_t, p.sin_t, dst + p.H * D);
#pragma unroll
            for (int k = 0; k < D; ++k) dst[2 * p.H * D + k] = dv[k];
        } else {
#pragma unroll
            for (int k = 0; k < D; ++k) { dst[p.H * D + k] = 0.f; dst[2 * p.H * D + k] = 0.f; }
        }
    }
}
template <int D>
static void attn_bwd_launch(const AttnBwdArgs& a, hipStream_t s) {
    const dim3 grid((a.T + AB_ROWS - 1) / AB_ROWS, a.H, a.B);
    hipLaunchKernelGGL(attn_bwd_q_kernel<D>, grid, dim3(AB_ROWS), 0, s, a);
    hipLaunchKernelGGL(attn_bwd_kv_kernel<D>, grid, dim3(AB_ROWS), 0, s, a);
}
static bool attn_bwd_head_dim_ok(int D) { return D >= 8 && D <= 64 && D % 8 == 0; }
static hipError_t launch_attn_bwd(const AttnBwdArgs& a, hipStream_t s) {
    if (!a.qkv || !a.o || !a.d_o || !a.len || !a.cos_t || !a.sin_t || !a.dqkv || !a.stats || a.B <= 0 || a.B > 65535 || a.H <= 0 ||
        a.H > 65535 || a.T <= 0 || a.T > SG_MAX_TX || !attn_bwd_head_dim_ok(a.D))
        return hipErrorInvalidValue;
    switch (a.D) {
        case 8: attn_bwd_launch<8>(a, s); break;
        case 16: attn_bwd_launch<16>(a, s); break;
        case 24: attn_bwd_launch<24>(a, s); break;
        case 32: attn_bwd_launch<32>(a, s); break;
        case 40: attn_bwd_launch<40>(a, s); break;
        case 48: attn_bwd_launch<48>(a, s); break;
        case 56: attn_bwd_launch<56>(a, s); break;
        default: attn_bwd_launch<64>(a, s); break;
    }
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------- backward panels (host)
// The transposed weight of a Linear / Conv1d(k, pad k / 2) in torch layout: w [N][C][k] -> wt [C][N][k] with the taps reversed, so
// that the data gradient is the same centred-tap GEMM with in / out channels swapped.  Cp >= C pads the NEW input channels (zeros).
std::vector<float> transposed(const float* w, int N, int C, int k, int Np) {
    Np = Np ? Np : N;
    std::vector<float> t((size_t)C * Np * k, 0.f);
    for (int n = 0; n < N; ++n)
        for (int c = 0; c < C; ++c)
            for (int j = 0; j < k; ++j) t[((size_t)c * Np + n) * k + j] = w[((size_t)n * C + c) * k + (k - 1 - j)];
    return t;
}

int pack_spk_grad(mtts_ctx* c) {
    const mtts_config& g = c->cfg;
    Component& G = c->grad;
    G.image.clear();
    G.gemm_terms = 0;             // native fp32 MFMA for every backward GEMM (file header)
    G.packed = false;
    G.uploaded = false;
    Packer P(&G);
    SpkGradW& W = c->gradw;
    W = SpkGradW();
    const int nch = g.enc_channels, Sd = g.spk_emb_dim, Hd = nch + Sd, Fd = g.dp_filter, Ff = g.enc_filter;
    auto raw = [&](const std::string& key, size_t numel) -> const std::vector<float>* {
        auto it = c->raw.find(key);
        if (it == c->raw.end()) { P.fail("missing tensor " + key); return nullptr; }
        if (it->second.size() != numel) { P.fail("tensor " + key + " has an unexpected size"); return nullptr; }
        return &it->second;
    };
    auto tpanel = [&](const std::string& key, int N, int C, int k, int Np = 0) {
        const auto* w = raw(key, (size_t)N * C * k);
        if (!w) return Panel();
        const std::vector<float> t = transposed(w->data(), N, C, k, Np);
        return P.panel_from(t.data(), nullptr, k == 1 ? 0 : 1, C, Np ? Np : N, k);
    };
    auto S = [](const std::string& a, int i, const std::string& b) { return a + std::to_string(i) + b; };
    W.pm2T = tpanel("encoder.proj_m.2.weight", g.n_feats, nch, 1, round_up(g.n_feats, 4));
    W.pm0T = tpanel("encoder.proj_m.0.weight", nch, Hd, 1);
    for (int l = 0; l < g.enc_layers && P.ok; ++l) {
        const std::string a = S("encoder.encoder.attn_layers.", l, "."), f = S("encoder.encoder.ffn_layers.", l, ".");
        W.oT.push_back(tpanel(a + "conv_o.weight", Hd, Hd, 1));
        const auto* wq = raw(a + "conv_q.weight", (size_t)Hd * Hd);
        const auto* wk = raw(a + "conv_k.weight", (size_t)Hd * Hd);
        const auto* wv = raw(a + "conv_v.weight", (size_t)Hd * Hd);
        if (!wq || !wk || !wv) break;
        std::vector<float> t((size_t)Hd * 3 * Hd);
        const std::vector<float>* parts[3] = {wq, wk, wv};
        for (int part = 0; part < 3; ++part)
            for (int n = 0; n < Hd; ++n)
                for (int cc = 0; cc < Hd; ++cc) t[(size_t)cc * 3 * Hd + part * Hd + n] = (*parts[part])[(size_t)n * Hd + cc];
        W.qkvT.push_back(P.panel_from(t.data(), nullptr, 0, Hd, 3 * Hd, 1));
        W.ffn2T.push_back(tpanel(f + "conv_2.weight", Hd, Ff, g.enc_kernel));
        W.ffn1T.push_back(tpanel(f + "conv_1.weight", Ff, Hd, g.enc_kernel));
    }
    for (int i = 0; i < g.dp_layers && P.ok; ++i)       // (layer 0 reads x.detach(): no data gradient; an empty panel keeps the index)
        W.dp_convT.push_back(i == 0 ? Panel() : tpanel(S("encoder.proj_w.conv_layers.", i, ".weight"), Fd, Fd, g.dp_kernel));
    W.filmT = tpanel("encoder.proj_w.spk_proj.weight", 2 * Fd, Sd, 1);
    if (const auto* w = raw("encoder.proj_w.proj.weight", Fd)) {
        W.dp_proj.off = P.alloc(Fd);
        W.dp_proj.n = Fd;
        std::memcpy(&G.image[W.dp_proj.off], w->data(), Fd * sizeof(float));
    }
    if (!P.ok) { set_error("mtts_spk_grad weights: " + P.why); return -1; }
    G.packed = true;
    return 0;
}

// ---------------------------------------------------------------------------------------------- plan
static void plan_spk_grad(const mtts_ctx* c, int B, int Tx, int Tm, WS& ws, SgBufs& e) {
    const mtts_config& g = c->cfg;
    const size_t M = (size_t)B * Tx;
    const int nch = g.enc_channels, Hd = nch + g.spk_emb_dim, F = g.dp_filter, ldm = round_up(g.n_feats, 4);
    (void)ws.bytes(256);                 // header: the call's range flag (begin_call)
    e.score_bytes = (size_t)mtts_score_workspace_bytes(B, Tx, Tm);
    e.score = ws.bytes(e.score_bytes);   // must land at SG_SCORE_OFF, where mtts_spk_grad_status looks (checked by mtts_spk_grad)
    e.off_score = ws.off - e.score_bytes;
    e.mas_bytes = (size_t)mtts_mas_workspace_bytes(B, Tx, Tm);
    e.mas = ws.bytes(e.mas_bytes);
    e.mu_x = ws.f(M * g.n_feats); e.off_mu_x = ws.off - M * g.n_feats * sizeof(float);
    e.logw = ws.f(M); e.off_logw = ws.off - M * sizeof(float);
    e.xm = ws.f(M); e.off_xm = ws.off - M * sizeof(float);
    e.dur = static_cast<int32_t*>(ws.bytes(M * sizeof(int32_t)));
    e.X0 = ws.f(M * nch); e.P1 = ws.f(M * nch); e.P2 = ws.f(M * nch); e.Y = ws.f(M * nch);
    e.PMpre = ws.f(M * nch); e.PM = ws.f(M * nch); e.MU = ws.f(M * ldm);
    e.FILM = ws.f((size_t)B * 2 * F); e.D1 = ws.f(M * F); e.D2 = ws.f(M * F);
    const int L = std::min(g.enc_layers, SG_MAX_LAYERS), Ld = std::min(g.dp_layers, SG_MAX_LAYERS);      // (more is refused: sg_layers_ok)
    for (int l = 0; l <= L; ++l) e.Hin[l] = ws.f(M * Hd);
    e.off_hout = ws.off - M * Hd * sizeof(float);
    for (int l = 0; l < L; ++l) {
        e.QKV[l] = ws.f(M * 3 * Hd); e.ATT[l] = ws.f(M * Hd); e.S1[l] = ws.f(M * Hd); e.H1[l] = ws.f(M * Hd);
        e.F1[l] = ws.f(M * g.enc_filter); e.S2[l] = ws.f(M * Hd);
    }
    for (int i = 0; i < Ld; ++i) e.DY[i] = ws.f(M * F);
    e.GA = ws.f(M * Hd); e.GB = ws.f(M * Hd); e.GF = ws.f(M * g.enc_filter); e.GQKV = ws.f(M * 3 * Hd); e.GATT = ws.f(M * Hd);
    e.stats = ws.f((size_t)B * g.enc_heads * Tx * 3);
    e.GMU = ws.f(M * ldm); e.GPM = ws.f(M * nch);
    e.GDA = ws.f(M * F); e.GDB = ws.f(M * F); e.FPROD = ws.f(M * F); e.DFILM = ws.f((size_t)B * 2 * F);
}
static bool sg_layers_ok(const char* who, const mtts_ctx* c) {
    if (c->cfg.enc_layers > SG_MAX_LAYERS || c->cfg.dp_layers > SG_MAX_LAYERS) {
        set_error(std::string(who) + ": more than 16 encoder or duration-predictor layers");
        return false;
    }
    return true;
}
static bool sg_shape_ok(const char* who, int B, int Tx, int Tm) {
    if (B < 1 || B > 65535) { set_error(std::string(who) + ": B must be in [1, 65535]"); return false; }
    if (Tx < 1 || Tx > SG_MAX_TX) { set_error(std::string(who) + ": Tx must be in [1, 1024]"); return false; }
    if (Tm < Tx) { set_error(std::string(who) + ": Tm < Tx (no monotone path gives every token a frame)"); return false; }
    if (Tm > (1 << 20)) { set_error(std::string(who) + ": Tm too large"); return false; }
    return true;
}

}  // namespace mtts

using namespace mtts;

extern "C" {

int64_t mtts_spk_grad_weights_bytes(mtts_ctx* c) {
    if (!c) { set_error("mtts_spk_grad_weights_bytes: null context"); return -1; }
    if (!c->grad.packed && pack_spk_grad(c)) return -1;
    return (int64_t)(c->grad.image.size() * sizeof(float));
}

int mtts_spk_grad_upload_weights(mtts_ctx* c, void* d_buf, int64_t bytes) {
    if (!c || !d_buf) { set_error("mtts_spk_grad_upload_weights: null argument"); return -1; }
    if (!c->grad.packed && pack_spk_grad(c)) return -1;
    Component& G = c->grad;
    if ((size_t)bytes < G.image.size() * sizeof(float)) { set_error("mtts_spk_grad_upload_weights: buffer too small (mtts_spk_grad_weights_bytes)"); return -1; }
    HIP_OK(hipMemcpy(d_buf, G.image.data(), G.image.size() * sizeof(float), hipMemcpyHostToDevice));
    G.d_image = static_cast<float*>(d_buf);
    G.uploaded = true;
    return 0;
}

int64_t mtts_spk_grad_workspace_bytes(mtts_ctx* c, int B, int Tx, int Tm) {
    if (!c) { set_error("mtts_spk_grad_workspace_bytes: null context"); return -1; }
    if (!sg_shape_ok("mtts_spk_grad_workspace_bytes", B, Tx, Tm) || !sg_layers_ok("mtts_spk_grad_workspace_bytes", c)) return -1;
    WS ws(nullptr, 0);
    SgBufs e;
    plan_spk_grad(c, B, Tx, Tm, ws, e);
    return (int64_t)ws.off + 256;
}

// Byte offset inside the workspace of what the taped forward of the latest call left: which 0 mu_x [B][F][Tx], 1 logw [B][Tx],
// 2 x_mask [B][Tx] (what mtts_text_encoder_forward returns, bit for bit).
int64_t mtts_spk_grad_tape_offset(mtts_ctx* c, int B, int Tx, int Tm, int which) {
    if (!c) { set_error("mtts_spk_grad_tape_offset: null context"); return -1; }
    if (!sg_shape_ok("mtts_spk_grad_tape_offset", B, Tx, Tm) || !sg_layers_ok("mtts_spk_grad_tape_offset", c)) return -1;
    if (which < 0 || which > 2) { set_error("mtts_spk_grad_tape_offset: which must be 0 (mu_x), 1 (logw) or 2 (x_mask)"); return -1; }
    WS ws(nullptr, 0);
    SgBufs e;
    plan_spk_grad(c, B, Tx, Tm, ws, e);
    return (int64_t)(which == 0 ? e.off_mu_x : which == 1 ? e.off_logw : e.off_xm);
}

// Byte offset inside the workspace of the encoder's output rows of the latest call's taped forward, [B Tx][enc_channels + spk_emb_dim]:
// what proj_m and the duration predictor read (and what mtts_dp_grad's frozen part must reproduce bit for bit).
int64_t mtts_spk_grad_rows_offset(mtts_ctx* c, int B, int Tx, int Tm) {
    if (!c) { set_error("mtts_spk_grad_rows_offset: null context"); return -1; }
    if (!sg_shape_ok("mtts_spk_grad_rows_offset", B, Tx, Tm) || !sg_layers_ok("mtts_spk_grad_rows_offset", c)) return -1;
    WS ws(nullptr, 0);
    SgBufs e;
    plan_spk_grad(c, B, Tx, Tm, ws, e);
    return (int64_t)e.off_hout;
}

}  // extern "C"

// What the entries of this file share -- mtts_spk_grad (the fine-tuning losses) and mtts_spk_grad_match (the style-training losses):
// the taped forward and the two walks back from seeded gradients, with the call's context, buffers and derived sizes.  The entries
// differ in their seeds alone.
namespace mtts {
SgCall::SgCall(mtts_ctx* ctx, const SgBufs& bufs, hipStream_t stream, int B_, int Tx_)
    : c(ctx), e(bufs), s(stream), B(B_), Tx(Tx_), g(ctx->cfg), E(ctx->enc), GW(ctx->gradw), G(&ctx->grad) {
    nch = g.enc_channels; Sd = g.spk_emb_dim; Hd = nch + Sd; F = g.dp_filter; M = B * Tx; nf = g.n_feats;
    dh = Hd / g.enc_heads; d_rope = dh / 2; ldm = round_up(nf, 4); L = g.enc_layers;
    ffn_p16 = c->sw.p16_on && c->gemm_terms == 2 && (g.enc_filter % 32) == 0;
    xm = e.xm;
}
int SgCall::ready(const char* who, const void* d_grad_buf) const {
    if (!c->grad.packed || !c->grad.uploaded || c->grad.d_image != d_grad_buf) {
        set_error(std::string(who) + ": backward panels not uploaded (mtts_spk_grad_upload_weights into d_grad_buf)");
        return -1;
    }
    RET_IF(check_ready(c));
    if ((size_t)Tx * d_rope > (size_t)E.rope_cos.n) { set_error("Phonetic representation too long, exceeds RoPE cache size"); return -1; }
    if (!attn_bwd_head_dim_ok(dh)) { set_error(std::string(who) + ": the encoder's head dim must be a multiple of 8 (<= 64)"); return -1; }
    return 0;
}
int SgCall::tgemm(const Component* comp, const Panel& p, const float* a0, int lda, int c0, int ntaps, const float* res, int ldr,
                  const float* out_mask, float* out, int ldc, int rowsB, int rowsT) const {
    GemmArgs a;
    panel_args(comp, p, a); rows_plain(a, rowsB, rowsT);
    if (ntaps > 1) taps_centered(a, ntaps);
    a.a0 = a0; a.lda0 = lda; a.c0 = c0; a.res = res; a.ldr = ldr; a.out_mask = out_mask; a.out = out; a.ldc = ldc;
    return run_gemm(c, a, s);
}

// ================================================================ taped forward: encoder.hip's launches, buffers per layer
int SgCall::forward_encoder(const int64_t* d_x, const int64_t* d_x_lengths, const float* d_e_enc) const {
    LAUNCH(c, 2, 0, s, launch_seq_mask(d_x_lengths, B, Tx, xm, s));
    LAUNCH(c, 2, 0, s, launch_embedding(d_x, W(c, E.emb.off), M, nch, sqrtf((float)nch), xm, e.X0, nch, s));
    const float* cur = e.X0;
    for (int i = 0; i < g.prenet_layers; ++i) {
        GemmArgs a;
        panel_args(c, E.pre_conv[i], a); rows_plain(a, B, Tx); taps_centered(a, g.prenet_kernel);
        a.a0 = cur; a.lda0 = nch; a.c0 = nch; a.a_mask = xm; a.out = e.Y; a.ldc = nch;
        RET_IF(run_gemm(c, a, s));
        float* dst = (i & 1) ? e.P2 : e.P1;
        LayerNormArgs ln;
        ln.x = e.Y; ln.ldx = nch; ln.y = dst; ln.ldy = nch; ln.M = M; ln.C = nch; ln.T = Tx;
        ln.gamma = W(c, E.pre_g[i].off); ln.beta = W(c, E.pre_b[i].off); ln.act = ACT_SILU;
        LAUNCH(c, 2, 0, s, launch_layernorm(ln, s));
        cur = dst;
    }
    {
        GemmArgs a;
        panel_args(c, E.pre_proj, a); rows_plain(a, B, Tx);
        a.a0 = cur; a.lda0 = nch; a.c0 = nch; a.out_mask = xm; a.res = e.X0; a.ldr = nch; a.out = e.Hin[0]; a.ldc = Hd;
        RET_IF(run_gemm(c, a, s));
    }
    LAUNCH(c, 2, 0, s, launch_bcast_rows(d_e_enc, B, Tx, Sd, xm, e.Hin[0], Hd, nch, s));
    for (int l = 0; l < L; ++l) {
        GemmArgs q;
        panel_args(c, E.qkv[l], q); rows_plain(q, B, Tx);
        q.a0 = e.Hin[l]; q.lda0 = Hd; q.c0 = Hd; q.out = e.QKV[l]; q.ldc = 3 * Hd;
        RET_IF(run_gemm(c, q, s));
        LAUNCH(c, 2, 0, s, launch_rope(e.QKV[l], B, Tx, g.enc_heads, dh, d_rope, W(c, E.rope_cos.off), W(c, E.rope_sin.off), s));
        AttnArgs at;
        at.qkv = e.QKV[l]; at.mask = xm; at.out = e.ATT[l]; at.B = B; at.T = Tx; at.H = g.enc_heads; at.D = dh;
        at.scale = 1.0f / sqrtf((float)dh); at.mask_mode = 1;
        RET_IF(run_attn(c, at, s));
        GemmArgs o;
        panel_args(c, E.o[l], o); rows_plain(o, B, Tx);
        o.a0 = e.ATT[l]; o.lda0 = Hd; o.c0 = Hd; o.res = e.Hin[l]; o.ldr = Hd; o.out = e.S1[l]; o.ldc = Hd;
        RET_IF(run_gemm(c, o, s));
        LayerNormArgs n1;
        n1.x = e.S1[l]; n1.ldx = Hd; n1.y = e.H1[l]; n1.ldy = Hd; n1.M = M; n1.C = Hd; n1.T = Tx;
        n1.gamma = W(c, E.n1_g[l].off); n1.beta = W(c, E.n1_b[l].off); n1.mask = xm;
        LAUNCH(c, 2, 0, s, launch_layernorm(n1, s));
        _Float16* F16 = reinterpret_cast<_Float16*>(e.F1[l]);
        GemmArgs f1;
        panel_args(c, E.ffn1[l], f1); rows_plain(f1, B, Tx); taps_centered(f1, g.enc_kernel);
        f1.a0 = e.H1[l]; f1.lda0 = Hd; f1.c0 = Hd; f1.act = ACT_RELU;
        if (ffn_p16) { f1.out16 = F16; f1.ld16 = 2 * g.enc_filter; f1.out16_mask = xm; }
        else { f1.out = e.F1[l]; f1.ldc = g.enc_filter; }
        RET_IF(run_gemm(c, f1, s));
        GemmArgs f2;
        panel_args(c, E.ffn2[l], f2); rows_plain(f2, B, Tx); taps_centered(f2, g.enc_kernel);
        if (ffn_p16) { f2.a16_0 = F16; f2.lda16_0 = 2 * g.enc_filter; f2.c0 = g.enc_filter; f2.fast16 = false; }
        else { f2.a0 = e.F1[l]; f2.lda0 = g.enc_filter; f2.c0 = g.enc_filter; f2.a_mask = xm; }
        f2.out_mask = xm; f2.res = e.H1[l]; f2.ldr = Hd; f2.out = e.S2[l]; f2.ldc = Hd;
        RET_IF(run_gemm(c, f2, s));
        LayerNormArgs n2 = n1;
        n2.x = e.S2[l]; n2.y = e.Hin[l + 1];
        n2.gamma = W(c, E.n2_g[l].off); n2.beta = W(c, E.n2_b[l].off);
        LAUNCH(c, 2, 0, s, launch_layernorm(n2, s));
    }
    return 0;
}
int SgCall::forward(const int64_t* d_x, const int64_t* d_x_lengths, const float* d_e_enc, const float* d_e_dur) const {
    RET_IF(forward_encoder(d_x, d_x_lengths, d_e_enc));
    const float* Hout = e.Hin[L];
    {
        GemmArgs a;
        panel_args(c, E.pm0, a); rows_plain(a, B, Tx);
        a.a0 = Hout; a.lda0 = Hd; a.c0 = Hd; a.act = ACT_SILU; a.out = e.PM; a.ldc = nch;
        RET_IF(run_gemm(c, a, s));
        GemmArgs pre = a;               // the same product without the activation: proj_m's pre-SiLU rows for the backward
        pre.act = ACT_NONE; pre.out = e.PMpre;
        RET_IF(run_gemm(c, pre, s));
        GemmArgs b;
        panel_args(c, E.pm2, b); rows_plain(b, B, Tx);
        b.a0 = e.PM; b.lda0 = nch; b.c0 = nch; b.out_mask = xm; b.out = e.MU; b.ldc = ldm;
        RET_IF(run_gemm(c, b, s));
        LAUNCH(c, 2, 0, s, launch_cl_to_cf(e.MU, ldm, B, nf, Tx, e.mu_x, Tx, 1.0f, 0.0f, s));
    }
    {
        GemmArgs fm;
        panel_args(c, E.film, fm); rows_plain(fm, B, 1);
        fm.a0 = d_e_dur; fm.lda0 = Sd; fm.c0 = Sd; fm.out = e.FILM; fm.ldc = 2 * F;
        RET_IF(run_gemm(c, fm, s));
        const float* dcur = Hout;
        int dc = Hd;
        for (int i = 0; i < g.dp_layers; ++i) {
            GemmArgs a;
            panel_args(c, E.dp_conv[i], a); rows_plain(a, B, Tx); taps_centered(a, g.dp_kernel);
            a.a0 = dcur; a.lda0 = dc; a.c0 = dc; a.a_mask = xm; a.act = ACT_RELU; a.out = e.DY[i]; a.ldc = F;
            RET_IF(run_gemm(c, a, s));
            float* dst = (i & 1) ? e.D2 : e.D1;
            LayerNormArgs ln;
            ln.x = e.DY[i]; ln.ldx = F; ln.y = dst; ln.ldy = F; ln.M = M; ln.C = F; ln.T = Tx;
            ln.gamma = W(c, E.dp_g[i].off); ln.beta = W(c, E.dp_b[i].off); ln.film = e.FILM;
            LAUNCH(c, 2, 0, s, launch_layernorm(ln, s));
            dcur = dst;
            dc = F;
        }
        GemmArgs p;
        panel_args(c, E.dp_proj, p); rows_plain(p, B, Tx);
        p.a0 = dcur; p.lda0 = dc; p.c0 = dc; p.a_mask = xm; p.out_mask = xm; p.out = e.logw; p.ldc = 1;
        RET_IF(run_gemm(c, p, s));
    }
    return 0;
}

// ================================================================ backward: d sum / d mu_x rows (e.GMU, seeded) -> e_enc
int SgCall::walk_prior(const int64_t* d_x_lengths, const int32_t* verdict, float* d_g_enc) const {
    RET_IF(tgemm(GW.pm2T, e.GMU, ldm, ldm, 1, nullptr, 0, nullptr, e.GPM, nch, B, Tx));
    LAUNCH(c, 2, 0, s, launch_gate(e.GPM, nch, M, nch, 0, e.PMpre, nch, nullptr, 0, nullptr, s));
    RET_IF(tgemm(GW.pm0T, e.GPM, nch, nch, 1, nullptr, 0, nullptr, e.GA, Hd, B, Tx));
    for (int l = L - 1; l >= 0; --l) {
        LnBwdArgs n2;
        n2.x = e.S2[l]; n2.ldx = Hd; n2.dy = e.GA; n2.lddy = Hd; n2.dx = e.GB; n2.lddx = Hd; n2.M = M; n2.C = Hd; n2.T = Tx;
        n2.gamma = W(c, E.n2_g[l].off); n2.beta = W(c, E.n2_b[l].off); n2.mask = xm;
        LAUNCH(c, 2, 0, s, launch_ln_bwd(n2, s));
        RET_IF(tgemm(GW.ffn2T[l], e.GB, Hd, Hd, g.enc_kernel, nullptr, 0, nullptr, e.GF, g.enc_filter, B, Tx));
        LAUNCH(c, 2, 0, s, launch_gate(e.GF, g.enc_filter, M, g.enc_filter, ffn_p16 ? 2 : 1, e.F1[l], g.enc_filter,
                                       reinterpret_cast<const _Float16*>(e.F1[l]), 2 * g.enc_filter, xm, s));
        RET_IF(tgemm(GW.ffn1T[l], e.GF, g.enc_filter, g.enc_filter, g.enc_kernel, e.GB, Hd, nullptr, e.GA, Hd, B, Tx));
        LnBwdArgs n1 = n2;
        n1.x = e.S1[l]; n1.gamma = W(c, E.n1_g[l].off); n1.beta = W(c, E.n1_b[l].off);
        LAUNCH(c, 2, 0, s, launch_ln_bwd(n1, s));
        RET_IF(tgemm(GW.oT[l], e.GB, Hd, Hd, 1, nullptr, 0, nullptr, e.GATT, Hd, B, Tx));
        AttnBwdArgs ab;
        ab.qkv = e.QKV[l]; ab.o = e.ATT[l]; ab.d_o = e.GATT; ab.len = d_x_lengths; ab.B = B; ab.T = Tx; ab.H = g.enc_heads; ab.D = dh;
        ab.scale = 1.0f / sqrtf((float)dh); ab.cos_t = W(c, E.rope_cos.off); ab.sin_t = W(c, E.rope_sin.off);
        ab.dqkv = e.GQKV; ab.stats = e.stats;
        LAUNCHB(c, 1, 10.0 * B * g.enc_heads * double(Tx) * Tx * dh, 0.0, s, launch_attn_bwd(ab, s));
        RET_IF(tgemm(GW.qkvT[l], e.GQKV, 3 * Hd, 3 * Hd, 1, e.GB, Hd, nullptr, e.GA, Hd, B, Tx));
    }
    LAUNCH(c, 2, 0, s, launch_colsum(e.GA, Hd, nch, Sd, B, Tx, d_x_lengths, verdict, d_g_enc, Sd, 0, 0, s));
    return 0;
}

// ================================================================ backward: d sum / d (duration predictor's last rows) (e.GDA, seeded) -> e_dur
int SgCall::walk_dur(const int64_t* d_x_lengths, const int32_t* verdict, float* d_g_dur, const DurTrain* train) const {
    bool first = true;
    const Component* PC = train ? train->comp : G;
    for (int i = g.dp_layers - 1; i >= 0; --i) {
        LAUNCH(c, 2, 0, s, launch_colsum(e.GDA, F, 0, F, B, Tx, d_x_lengths, verdict, e.DFILM, 2 * F, F, first ? 0 : 1, s));
        LnBwdArgs ln;
        ln.x = e.DY[i]; ln.ldx = F; ln.dy = e.GDA; ln.lddy = F; ln.dx = e.GDB; ln.lddx = F; ln.M = M; ln.C = F; ln.T = Tx;
        ln.gamma = train ? train->gamma[i] : W(c, E.dp_g[i].off); ln.beta = train ? train->beta[i] : W(c, E.dp_b[i].off);
        ln.film = e.FILM; ln.film_prod = e.FPROD; ln.gate = ACT_RELU;
        LAUNCH(c, 2, 0, s, launch_ln_bwd(ln, s));
        if (train && train->reduce) RET_IF(train->reduce(train->reduce_ctx, i));
        LAUNCH(c, 2, 0, s, launch_colsum(e.FPROD, F, 0, F, B, Tx, d_x_lengths, verdict, e.DFILM, 2 * F, 0, first ? 0 : 1, s));
        first = false;
        if (i >= 1) RET_IF(tgemm(PC, train ? train->convT[i] : GW.dp_convT[i], e.GDB, F, F, g.dp_kernel, nullptr, 0, xm, e.GDA, F, B, Tx));
    }
    if (d_g_dur) RET_IF(tgemm(PC, train ? train->filmT : GW.filmT, e.DFILM, 2 * F, 2 * F, 1, nullptr, 0, nullptr, d_g_dur, Sd, B, 1));
    return 0;
}
}  // namespace mtts

extern "C" {

int mtts_spk_grad(mtts_ctx* c, const int64_t* d_x, const int64_t* d_x_lengths, const float* d_e_enc, const float* d_e_dur,
                  const float* d_y_fine, const int64_t* d_y_fine_lengths, const int32_t* d_durations_in, float delta_prior,
                  float delta_dur, int B, int Tx, int Tm, float* d_g_enc, float* d_g_dur, float* d_prior_sum, float* d_dur_sum,
                  int32_t* d_durations_out, void* d_grad_buf, void* d_ws, int64_t ws_bytes, void* stream) {
    if (!c || !d_x || !d_x_lengths || !d_e_enc || !d_e_dur || !d_y_fine || !d_y_fine_lengths || !d_g_enc || !d_g_dur || !d_prior_sum ||
        !d_dur_sum || !d_grad_buf || !d_ws) {
        set_error("mtts_spk_grad: null argument");
        return -1;
    }
    if (!sg_shape_ok("mtts_spk_grad", B, Tx, Tm) || !sg_layers_ok("mtts_spk_grad", c)) return -1;
    if (!(delta_prior > 0.f) || !(delta_dur > 0.f)) { set_error("mtts_spk_grad: the Huber thresholds must be positive"); return -1; }
    CTX_GUARD(c);
    WS ws(d_ws, (size_t)ws_bytes);
    SgBufs e;
    plan_spk_grad(c, B, Tx, Tm, ws, e);
    if (ws.overflow || ws_bytes < (int64_t)ws.off) { set_error("mtts_spk_grad: workspace too small (mtts_spk_grad_workspace_bytes)"); return -1; }
    if (reinterpret_cast<uintptr_t>(d_ws) & 15) { set_error("mtts_spk_grad: workspace must be 16-byte aligned"); return -1; }
    if (e.off_score != SG_SCORE_OFF) { set_error("mtts_spk_grad: the score workspace is not where mtts_spk_grad_status reads it"); return -1; }
    hipStream_t s = static_cast<hipStream_t>(stream);
    const SgCall k(c, e, s, B, Tx);
    RET_IF(k.ready("mtts_spk_grad", d_grad_buf));
    RET_IF(begin_call(c, d_ws, s));
    RET_IF(k.forward(d_x, d_x_lengths, d_e_enc, d_e_dur));

    // ================================================================ alignment (constant of the step) and the two sums
    const int32_t* dur = d_durations_in;
    if (!dur) {
        int32_t* dst = d_durations_out ? d_durations_out : e.dur;
        RET_IF(mtts_mas(nullptr, e.mu_x, d_y_fine, d_x_lengths, d_y_fine_lengths, B, k.nf, Tx, Tm, dst, nullptr, nullptr, e.mas,
                        (int64_t)e.mas_bytes, stream));
        dur = dst;
    } else if (d_durations_out && d_durations_out != d_durations_in) {
        hipLaunchKernelGGL(copy_i32_kernel, dim3((k.M + 255) / 256), dim3(256), 0, s, d_durations_in, d_durations_out, (size_t)k.M);
        HIP_OK(hipGetLastError());
    }
    RET_IF(mtts_score_prior_dur(e.mu_x, e.logw, dur, d_y_fine, d_x_lengths, d_y_fine_lengths, B, k.nf, Tx, Tm, delta_prior, delta_dur,
                                d_prior_sum, d_dur_sum, nullptr, nullptr, e.score, (int64_t)e.score_bytes, stream));
    const int32_t* verdict = reinterpret_cast<const int32_t*>(static_cast<char*>(e.score) + SCORE_HEADER_BYTES);

    // ================================================================ the two seeds, each followed by its walk back
    LAUNCH(c, 2, 0, s, launch_fill_cols(e.GMU, k.M, k.ldm, 0, k.ldm, 0.f, s));
    hipLaunchKernelGGL(seed_mu_kernel, dim3(k.nf, B), dim3(256), 0, s, e.mu_x, d_y_fine, dur, d_x_lengths, verdict, k.nf, Tx, Tm, delta_prior,
                       e.GMU, k.ldm);
    HIP_OK(hipGetLastError());
    RET_IF(k.walk_prior(d_x_lengths, verdict, d_g_enc));
    hipLaunchKernelGGL(seed_logw_kernel, dim3(k.M), dim3(64), 0, s, e.logw, dur, d_x_lengths, verdict, k.G->d_image + k.GW.dp_proj.off, Tx, k.F,
                       delta_dur, e.GDA);
    HIP_OK(hipGetLastError());
    RET_IF(k.walk_dur(d_x_lengths, verdict, d_g_dur));
    return 0;
}

// Style-encoder training (reference matcha/models/style_encoder.py:119-143): the frozen text encoder's outputs under PREDICTED rows
// matched against its outputs under the real rows (d_mu_ref, d_logw_ref: constants) with smooth-L1.  The same taped forward and the same
// two walks as mtts_spk_grad; the seeds are clamp((out - ref) / beta, -1, 1) on the tokens x < len_b.
int64_t mtts_spk_grad_match_workspace_bytes(mtts_ctx* c, int B, int Tx) {
    if (!c) { set_error("mtts_spk_grad_match_workspace_bytes: null context"); return -1; }
    if (!sg_shape_ok("mtts_spk_grad_match_workspace_bytes", B, Tx, Tx) || !sg_layers_ok("mtts_spk_grad_match_workspace_bytes", c)) return -1;
    WS ws(nullptr, 0);
    SgBufs e;
    plan_spk_grad(c, B, Tx, Tx, ws, e);
    (void)ws.f((size_t)B * c->cfg.n_feats);
    return (int64_t)ws.off + 256;
}

int mtts_spk_grad_match(mtts_ctx* c, const int64_t* d_x, const int64_t* d_x_lengths, const float* d_e_enc, const float* d_e_dur,
                        const float* d_mu_ref, const float* d_logw_ref, float beta_mu, float beta_logw, int B, int Tx, float* d_g_enc,
                        float* d_g_dur, float* d_ac_sum, float* d_rh_sum, void* d_grad_buf, void* d_ws, int64_t ws_bytes, void* stream) {
    if (!c || !d_x || !d_x_lengths || !d_e_enc || !d_e_dur || !d_mu_ref || !d_logw_ref || !d_g_enc || !d_g_dur || !d_ac_sum || !d_rh_sum ||
        !d_grad_buf || !d_ws) {
        set_error("mtts_spk_grad_match: null argument");
        return -1;
    }
    if (!sg_shape_ok("mtts_spk_grad_match", B, Tx, Tx) || !sg_layers_ok("mtts_spk_grad_match", c)) return -1;
    if (!(beta_mu > 0.f) || !(beta_logw > 0.f)) { set_error("mtts_spk_grad_match: the smooth-L1 betas must be positive"); return -1; }
    CTX_GUARD(c);
    WS ws(d_ws, (size_t)ws_bytes);
    SgBufs e;
    plan_spk_grad(c, B, Tx, Tx, ws, e);
    float* part = ws.f((size_t)B * c->cfg.n_feats);
    if (ws.overflow || ws_bytes < (int64_t)ws.off) { set_error("mtts_spk_grad_match: workspace too small (mtts_spk_grad_match_workspace_bytes)"); return -1; }
    if (reinterpret_cast<uintptr_t>(d_ws) & 15) { set_error("mtts_spk_grad_match: workspace must be 16-byte aligned"); return -1; }
    if (e.off_score != SG_SCORE_OFF) { set_error("mtts_spk_grad_match: the status words are not where mtts_spk_grad_match_status reads them"); return -1; }
    hipStream_t s = static_cast<hipStream_t>(stream);
    const SgCall k(c, e, s, B, Tx);
    RET_IF(k.ready("mtts_spk_grad_match", d_grad_buf));
    RET_IF(begin_call(c, d_ws, s));
    int32_t* status = static_cast<int32_t*>(e.score);
    int32_t* verdict = reinterpret_cast<int32_t*>(static_cast<char*>(e.score) + SCORE_HEADER_BYTES);
    hipLaunchKernelGGL(match_verdict_kernel, dim3(1), dim3(256), 0, s, d_x_lengths, B, Tx, status, verdict);
    HIP_OK(hipGetLastError());
    RET_IF(k.forward(d_x, d_x_lengths, d_e_enc, d_e_dur));
    LAUNCH(c, 2, 0, s, launch_fill_cols(e.GMU, k.M, k.ldm, 0, k.ldm, 0.f, s));
    hipLaunchKernelGGL(seed_match_mu_kernel, dim3(k.nf, B), dim3(256), 0, s, e.mu_x, d_mu_ref, d_x_lengths, verdict, k.nf, Tx, beta_mu, e.GMU,
                       k.ldm, part);
    HIP_OK(hipGetLastError());
    RET_IF(k.walk_prior(d_x_lengths, verdict, d_g_enc));
    hipLaunchKernelGGL(seed_match_logw_kernel, dim3(k.M), dim3(64), 0, s, e.logw, d_logw_ref, d_x_lengths, verdict,
                       k.G->d_image + k.GW.dp_proj.off, Tx, k.F, beta_logw, e.GDA);
    HIP_OK(hipGetLastError());
    RET_IF(k.walk_dur(d_x_lengths, verdict, d_g_dur));
    hipLaunchKernelGGL(match_finish_kernel, dim3(B), dim3(64), 0, s, part, e.logw, d_logw_ref, d_x_lengths, verdict, k.nf, Tx, beta_logw, d_ac_sum,
                       d_rh_sum);
    HIP_OK(hipGetLastError());
    return 0;
}

// The verdict of mtts_spk_grad_match's device-side check of the lengths.  Waits for the stream.
int mtts_spk_grad_match_status(const void* d_ws, void* stream) {
    if (!d_ws) { set_error("mtts_spk_grad_match_status: null workspace"); return -1; }
    int st[4];
    if (read_status("mtts_spk_grad_match_status", static_cast<const char*>(d_ws) + SG_SCORE_OFF, stream, st)) return -1;
    if (st[0] != 0) {
        set_error("mtts_spk_grad_match: utterance " + std::to_string(st[0] - 1) + " has x_length = " + std::to_string(st[1]) +
                  " (need 1 <= x_length <= Tx = " + std::to_string(st[2]) + ")");
        return -1;
    }
    return 0;
}

// The verdict of the call's device-side checks (score.hip's, on this call's lengths and durations).  The one entry of this file that
// waits for the stream.
int mtts_spk_grad_status(const void* d_ws, void* stream) {
    if (!d_ws) { set_error("mtts_spk_grad_status: null workspace"); return -1; }
    if (mtts_score_status(static_cast<const char*>(d_ws) + SG_SCORE_OFF, stream) != 0) {
        std::string m = get_error();
        const std::string from = "mtts_score_prior_dur";
        const size_t at = m.find(from);
        if (at != std::string::npos) m.replace(at, from.size(), "mtts_spk_grad");
        set_error(m);
        return -1;
    }
    return 0;
}

// ---------------------------------------------------------------------------------------------- unit entries (kernel-level parity)
// fp32 rows in and out.  d_dfilm [B][2C] (gamma | beta gradient per utterance over all T rows) needs d_film and d_scratch [B T][C].
int mtts_channel_layernorm_bwd(const float* d_x, const float* d_dy, int B, int T, int C, const float* d_gamma, const float* d_beta, float eps,
                               int act, const float* d_film, const float* d_mask, int gate, float* d_dx, float* d_dfilm, void* d_scratch,
                               void* stream) {
    if (!d_x || !d_dy || !d_dx) { set_error("mtts_channel_layernorm_bwd: null argument"); return -1; }
    if (B <= 0 || T <= 0 || C <= 0) { set_error("mtts_channel_layernorm_bwd: empty batch"); return -1; }
    if (act != ACT_NONE && act != ACT_SILU) { set_error("mtts_channel_layernorm_bwd: act must be 0 (none) or 2 (SiLU)"); return -1; }
    if (gate != ACT_NONE && gate != ACT_RELU) { set_error("mtts_channel_layernorm_bwd: gate must be 0 (none) or 1 (ReLU)"); return -1; }
    if (d_dfilm && (!d_film || !d_scratch)) { set_error("mtts_channel_layernorm_bwd: d_dfilm needs d_film and d_scratch"); return -1; }
    hipStream_t s = static_cast<hipStream_t>(stream);
    LnBwdArgs a;
    a.x = d_x; a.ldx = C; a.dy = d_dy; a.lddy = C; a.dx = d_dx; a.lddx = C; a.M = B * T; a.C = C; a.T = T; a.gamma = d_gamma; a.beta = d_beta;
    a.eps = eps; a.act = act; a.film = d_film; a.film_prod = d_dfilm ? static_cast<float*>(d_scratch) : nullptr; a.mask = d_mask; a.gate = gate;
    HIP_OK(launch_ln_bwd(a, s));
    if (d_dfilm) {
        HIP_OK(launch_colsum(static_cast<const float*>(d_scratch), C, 0, C, B, T, nullptr, nullptr, d_dfilm, 2 * C, 0, 0, s));
        HIP_OK(launch_colsum(d_dy, C, 0, C, B, T, nullptr, nullptr, d_dfilm, 2 * C, C, 0, s));
    }
    return 0;
}

// The seed and sum kernels of mtts_spk_grad_match on given buffers: d_mu / d_mu_ref [B][F][Tx], d_logw / d_logw_ref [B][Tx], d_lengths
// int64 [B], d_w_proj [Fd] -> d_seed_mu [B Tx][F] (zero beyond an utterance), d_seed_logw [B Tx][Fd], d_ac_sum / d_rh_sum [B].
// d_scratch: mtts_match_seeds_scratch_bytes.
int64_t mtts_match_seeds_scratch_bytes(int B, int F) {
    if (B < 1 || F < 1) { set_error("mtts_match_seeds_scratch_bytes: bad shape"); return -1; }
    return (int64_t)(SCORE_HEADER_BYTES + ((size_t)B * 2 * sizeof(int32_t) + 255) / 256 * 256 + (size_t)B * F * sizeof(float));
}
int mtts_match_seeds(const float* d_mu, const float* d_mu_ref, const float* d_logw, const float* d_logw_ref, const int64_t* d_lengths,
                     const float* d_w_proj, int B, int F, int Tx, int Fd, float beta_mu, float beta_logw, float* d_seed_mu, float* d_seed_logw,
                     float* d_ac_sum, float* d_rh_sum, void* d_scratch, void* stream) {
    if (!d_mu || !d_mu_ref || !d_logw || !d_logw_ref || !d_lengths || !d_w_proj || !d_seed_mu || !d_seed_logw || !d_ac_sum || !d_rh_sum || !d_scratch) {
        set_error("mtts_match_seeds: null argument");
        return -1;
    }
    if (B < 1 || B > 65535 || F < 1 || F > 65535 || Fd < 1 || Tx < 1 || Tx > SG_MAX_TX) { set_error("mtts_match_seeds: need B, F, Fd >= 1 and 1 <= Tx <= 1024"); return -1; }
    if (!(beta_mu > 0.f) || !(beta_logw > 0.f)) { set_error("mtts_match_seeds: the smooth-L1 betas must be positive"); return -1; }
    hipStream_t s = static_cast<hipStream_t>(stream);
    char* sc = static_cast<char*>(d_scratch);
    int32_t* status = reinterpret_cast<int32_t*>(sc);
    int32_t* verdict = reinterpret_cast<int32_t*>(sc + SCORE_HEADER_BYTES);
    float* part = reinterpret_cast<float*>(sc + SCORE_HEADER_BYTES + ((size_t)B * 2 * sizeof(int32_t) + 255) / 256 * 256);
    hipLaunchKernelGGL(match_verdict_kernel, dim3(1), dim3(256), 0, s, d_lengths, B, Tx, status, verdict);
    HIP_OK(launch_fill_cols(d_seed_mu, B * Tx, F, 0, F, 0.f, s));
    hipLaunchKernelGGL(seed_match_mu_kernel, dim3(F, B), dim3(256), 0, s, d_mu, d_mu_ref, d_lengths, verdict, F, Tx, beta_mu, d_seed_mu, F, part);
    hipLaunchKernelGGL(seed_match_logw_kernel, dim3(B * Tx), dim3(64), 0, s, d_logw, d_logw_ref, d_lengths, verdict, d_w_proj, Tx, Fd, beta_logw,
                       d_seed_logw);
    hipLaunchKernelGGL(match_finish_kernel, dim3(B), dim3(64), 0, s, part, d_logw, d_logw_ref, d_lengths, verdict, F, Tx, beta_logw, d_ac_sum, d_rh_sum);
    HIP_OK(hipGetLastError());
    return 0;
}

// d_qkv [B T][3 H D] rows AFTER the rotation, d_o / d_do [B T][H D], d_lengths int64 [B], d_cos / d_sin [>= T][D / 2] (rotary on the
// first D / 2 dims); d_dqkv [B T][3 H D] = gradient with respect to q | k | v BEFORE the rotation; d_scratch [B][H][T][3] floats.
int mtts_attention_rope_bwd(const float* d_qkv, const float* d_o, const float* d_do, const int64_t* d_lengths, int B, int T, int H, int D,
                            float scale, const float* d_cos, const float* d_sin, float* d_dqkv, void* d_scratch, void* stream) {
    if (!d_qkv || !d_o || !d_do || !d_lengths || !d_cos || !d_sin || !d_dqkv || !d_scratch) { set_error("mtts_attention_rope_bwd: null argument"); return -1; }
    if (B < 1 || H < 1 || T < 1 || T > SG_MAX_TX) { set_error("mtts_attention_rope_bwd: need B, H >= 1 and 1 <= T <= 1024"); return -1; }
    if (!attn_bwd_head_dim_ok(D)) { set_error("mtts_attention_rope_bwd: D must be a multiple of 8, <= 64"); return -1; }
    AttnBwdArgs a;
    a.qkv = d_qkv; a.o = d_o; a.d_o = d_do; a.len = d_lengths; a.B = B; a.T = T; a.H = H; a.D = D; a.scale = scale; a.cos_t = d_cos; a.sin_t = d_sin;
    a.dqkv = d_dqkv; a.stats = static_cast<float*>(d_scratch);
    HIP_OK(launch_attn_bwd(a, static_cast<hipStream_t>(stream)));
    return 0;
}

// The two seeds of mtts_spk_grad on given buffers, launched as that entry launches them: mtts_score_prior_dur into the scratch for the
// verdicts, the zero fill, seed_mu_kernel, seed_logw_kernel.  d_mu_x [B][F][Tx], d_logw [B][Tx], d_durations int32 [B][Tx], d_y_fine
// [B][F][Tm], d_w_proj [Fd] -> d_seed_mu [B Tx][round_up(F, 4)], d_seed_logw [B Tx][Fd].  The scratch starts with the score workspace
// (mtts_score_status reads the verdict there), then the two sums [B] that the score writes.
static size_t seeds_sums_off(int B, int Tx, int Tm) { return ((size_t)mtts_score_workspace_bytes(B, Tx, Tm) + 255) / 256 * 256; }
int64_t mtts_spk_grad_seeds_scratch_bytes(int B, int Tx, int Tm) {
    if (!sg_shape_ok("mtts_spk_grad_seeds_scratch_bytes", B, Tx, Tm)) return -1;
    return (int64_t)(seeds_sums_off(B, Tx, Tm) + ((size_t)2 * B * sizeof(float) + 255) / 256 * 256);
}
int mtts_spk_grad_seeds(const float* d_mu_x, const float* d_logw, const int32_t* d_durations, const float* d_y_fine, const int64_t* d_x_lengths,
                        const int64_t* d_y_fine_lengths, const float* d_w_proj, int B, int F, int Tx, int Tm, int Fd, float delta_prior,
                        float delta_dur, float* d_seed_mu, float* d_seed_logw, void* d_scratch, int64_t scratch_bytes, void* stream) {
    if (!d_mu_x || !d_logw || !d_durations || !d_y_fine || !d_x_lengths || !d_y_fine_lengths || !d_w_proj || !d_seed_mu || !d_seed_logw ||
        !d_scratch) {
        set_error("mtts_spk_grad_seeds: null argument");
        return -1;
    }
    if (!sg_shape_ok("mtts_spk_grad_seeds", B, Tx, Tm)) return -1;
    if (F < 1 || F > 65535 || Fd < 1) { set_error("mtts_spk_grad_seeds: need 1 <= F <= 65535 and Fd >= 1"); return -1; }
    if (!(delta_prior > 0.f) || !(delta_dur > 0.f)) { set_error("mtts_spk_grad_seeds: the Huber thresholds must be positive"); return -1; }
    if (scratch_bytes < mtts_spk_grad_seeds_scratch_bytes(B, Tx, Tm)) { set_error("mtts_spk_grad_seeds: scratch too small (mtts_spk_grad_seeds_scratch_bytes)"); return -1; }
    if (reinterpret_cast<uintptr_t>(d_scratch) & 15) { set_error("mtts_spk_grad_seeds: scratch must be 16-byte aligned"); return -1; }
    hipStream_t s = static_cast<hipStream_t>(stream);
    char* sc = static_cast<char*>(d_scratch);
    float* sums = reinterpret_cast<float*>(sc + seeds_sums_off(B, Tx, Tm));
    RET_IF(mtts_score_prior_dur(d_mu_x, d_logw, d_durations, d_y_fine, d_x_lengths, d_y_fine_lengths, B, F, Tx, Tm, delta_prior, delta_dur, sums,
                                sums + B, nullptr, nullptr, sc, mtts_score_workspace_bytes(B, Tx, Tm), stream));
    const int32_t* verdict = reinterpret_cast<const int32_t*>(sc + SCORE_HEADER_BYTES);
    const int ldm = round_up(F, 4);
    HIP_OK(launch_fill_cols(d_seed_mu, B * Tx, ldm, 0, ldm, 0.f, s));
    hipLaunchKernelGGL(seed_mu_kernel, dim3(F, B), dim3(256), 0, s, d_mu_x, d_y_fine, d_durations, d_x_lengths, verdict, F, Tx, Tm, delta_prior,
                       d_seed_mu, ldm);
    HIP_OK(hipGetLastError());
    hipLaunchKernelGGL(seed_logw_kernel, dim3(B * Tx), dim3(64), 0, s, d_logw, d_durations, d_x_lengths, verdict, d_w_proj, Tx, Fd, delta_dur,
                       d_seed_logw);
    HIP_OK(hipGetLastError());
    return 0;
}

// gate_kernel on fp32 gradient rows d_g [M][ldg] (in place) against the fp32 reference rows d_ref [M][ldref]: mode 0 SiLU', 1 the ReLU
// gate on the fp32 rows, 2 the ReLU gate on their P16 image, which is built here as the FFN hand-over builds it (residual scale 2^11,
// rows times d_mask) in d_scratch (M * 2 C halves).  d_mask [M] or NULL (modes 1 and 2).
int mtts_grad_gate(float* d_g, int ldg, int M, int C, int mode, const float* d_ref, int ldref, const float* d_mask, void* d_scratch,
                   void* stream) {
    if (!d_g || !d_ref) { set_error("mtts_grad_gate: null argument"); return -1; }
    if (mode < 0 || mode > 2) { set_error("mtts_grad_gate: mode must be 0 (SiLU'), 1 (ReLU on fp32 rows) or 2 (ReLU on the P16 image)"); return -1; }
    if (M < 1 || C < 1 || ldg < C || ldref < C) { set_error("mtts_grad_gate: need M, C >= 1, ldg >= C and ldref >= C"); return -1; }
    hipStream_t s = static_cast<hipStream_t>(stream);
    _Float16* img = nullptr;
    if (mode == 2) {
        if (!d_scratch) { set_error("mtts_grad_gate: mode 2 needs d_scratch (M * 2 C halves)"); return -1; }
        if ((C & 31) || (ldref & 3)) { set_error("mtts_grad_gate: mode 2 needs C a multiple of 32 and ldref a multiple of 4"); return -1; }
        img = static_cast<_Float16*>(d_scratch);
        HIP_OK(launch_to_p16(d_ref, ldref, d_mask, M, C, C, img, 2 * C, F16_RES_SCALE, s));
    }
    HIP_OK(launch_gate(d_g, ldg, M, C, mode, d_ref, ldref, img, 2 * C, d_mask, s));
    return 0;
}

// launch_colsum with every argument: d_dst[b][dcol0 + c] (+)= the sum over t < len_b of d_src[(b T + t) ld + col0 + c], c < C.  d_len
// int64 [B] or NULL (T); d_verdict int32 [B][2] or NULL (non-zero first word: the utterance's sums are zero).
int mtts_token_sums(const float* d_src, int ld, int col0, int C, int B, int T, const int64_t* d_len, const int32_t* d_verdict, float* d_dst,
                    int ldd, int dcol0, int accumulate, void* stream) {
    if (!d_src || !d_dst) { set_error("mtts_token_sums: null argument"); return -1; }
    if (B < 1 || B > 65535 || T < 1 || C < 1) { set_error("mtts_token_sums: need 1 <= B <= 65535 and T, C >= 1"); return -1; }
    if (col0 < 0 || dcol0 < 0 || ld < col0 + C || ldd < dcol0 + C) { set_error("mtts_token_sums: need col0, dcol0 >= 0, ld >= col0 + C and ldd >= dcol0 + C"); return -1; }
    if (accumulate != 0 && accumulate != 1) { set_error("mtts_token_sums: accumulate must be 0 or 1"); return -1; }
    HIP_OK(launch_colsum(d_src, ld, col0, C, B, T, d_len, d_verdict, d_dst, ldd, dcol0, accumulate, static_cast<hipStream_t>(stream)));
    return 0;
}

}  // extern "C"
