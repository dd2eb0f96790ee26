// Parameter gradients of the duration predictor (gfx950): training reference components/text_encoder.py:64-112 (DurationPredictor) on
// the device with everything else frozen.  In the reference logw = proj_w(x.detach(), x_mask, e_dur) (text_encoder.py:404) and the
// duration Huber loss (matcha_tts.py:117,128) is the only loss that reaches encoder.proj_w.*: this IS the reference's gradient for those
// tensors, not an approximation -- except that it is the dropout-free gradient (the reference trains with p_dropout), as mtts_spk_grad's.
//
//   training component    the predictor's forward panels, LayerNorm affines, output projection and the transposed, tap-reversed panels
//                         of the walk back, packed on the host from ONE FLAT fp32 parameter vector (state-dict order) into a buffer of
//                         its own (mtts_dp_train_upload): 2.5 MB at the production size, repacked every step.  Native fp32 MFMA
//                         (gemm_terms 0) for the same reason as pack_spk_grad.  Neither the model's image nor the speaker-row panels
//                         are touched; the model's image is rebuilt once, when training ends.
//   frozen encoder        SgCall::forward_encoder (spk_grad.hip): mask, embedding, prenet, encoder layers from the context's image in the
//                         context's arithmetic -- the rows the predictor reads are mtts_text_encoder_forward's bit for bit
//   predictor forward     the launches of the predictor in encoder.hip from the training component, every layer's rows kept.  Native
//                         fp32: NOT bit-equal to mtts_text_encoder_forward's logw under the default split arithmetic
//   dp_verdict / dp_seed  the ragged-batch verdict (length outside [1, Tx], a negative duration), mtts_spk_grad's seed_logw, the
//                         per-utterance Huber sums
//   SgCall::walk_dur      the walk back (spk_grad.hip) with its panels from the training component; the ping-pong buffers are reused
//                         between layers, so each parameter reduction is launched inside the walk, right after its operands are ready
//   conv weights          launch_conv_wgrad (style_grad.hip): exact fp32 MFMA, chunked
//   ln_film_wgrad_kernel  d gamma[c] = sum_r dy[r,c] gf_b[c] xhat[r,c], d beta[c] = sum_r dy[r,c] gf_b[c]; the row statistics are
//                         recomputed from the taped pre-norm rows
//   rows_wgrad_kernel     d proj.weight[c] = sum_r seed[r] h[r,c], d proj.bias = sum_r seed[r]
//   outer_batch_sum_kernel  d spk_proj.weight = sum_b DFILM_b (x) e_dur_b, d spk_proj.bias = sum_b DFILM_b, batch order
//
// Fixed order (conv_wgrad.h): rows are cut into chunks of conv_wgrad_chunk_rows(M) rows; inside a chunk four phases take the rows
// r0 + p, r0 + p + 4, ... in row order and are combined as ((p0 + p1) + p2) + p3; the chunks are added in chunk order by
// chunk_sum_kernel.  Every product is rounded before it is added (no FMA contraction).  No floating-point atomics: two calls give the
// same bits.
#include "conv_wgrad.h"
#include "device_utils.h"
#include "spk_grad.h"

#include <string>

namespace mtts {

__device__ __forceinline__ float dg_wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
__device__ __forceinline__ int dg_len(const int64_t* __restrict__ lengths, int b, int T) {
    if (!lengths) return T;
    const int64_t n = lengths[b];
    return n < 0 ? 0 : (n > (int64_t)T ? T : (int)n);
}

// ---------------------------------------------------------------------------------------------- LayerNorm + FiLM parameter gradient
// part[chunk][0 .. C) = d gamma, part[chunk][C .. 2C) = d beta of the chunk's rows.  grid (ceil(C / 256), chunks), 256 threads: wave p
// is phase p and takes one row at a time; lane l owns the channels c0 + l + 64 j, j < 4.  A row's mean and rstd are recomputed from the
// pre-norm row x as ln_bwd_kernel computes them (lane-strided sums, a wave butterfly) -- no [M][C] scratch of normalised rows.
// Rows with t >= len_b do not take part (a select, not a product).
__global__ __launch_bounds__(256) void ln_film_wgrad_kernel(const float* __restrict__ x, int ldx, const float* __restrict__ dy, int lddy,
                                                            const float* __restrict__ film, const int64_t* __restrict__ lengths, int B, int T,
                                                            int C, float eps, int chunk, float* __restrict__ part) {
    __shared__ float pg[4][256], pb[4][256];
    const int lane = threadIdx.x & 63, ph = threadIdx.x >> 6;
    const int c0 = blockIdx.x * 256;
    const int M = B * T;
    const int r_begin = blockIdx.y * chunk;
    const int r_end = min(r_begin + chunk, M);
    float ag[4] = {0.f, 0.f, 0.f, 0.f}, ab[4] = {0.f, 0.f, 0.f, 0.f};
    for (int r = r_begin + ph; r < r_end; r += 4) {
        const int b = r / T, t = r - b * T;
        if (t >= dg_len(lengths, b, T)) continue;          // (uniform per wave)
        const float* xr = x + (size_t)r * ldx;
        const float* dr = dy + (size_t)r * lddy;
        const float* gf = film + (size_t)b * 2 * C;
        float s = 0.f;
        for (int c = lane; c < C; c += 64) s += xr[c];
        const float mu = dg_wave_sum(s) / (float)C;
        float q = 0.f;
        for (int c = lane; c < C; c += 64) { const float d = xr[c] - mu; q += d * d; }
        const float rs = 1.0f / sqrtf(dg_wave_sum(q) / (float)C + eps);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int c = c0 + lane + 64 * j;
            if (c < C) {
                const float g = dr[c] * gf[c];
                const float xh = (xr[c] - mu) * rs;
                ag[j] += g * xh;
                ab[j] += g;
            }
        }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) { pg[ph][lane + 64 * j] = ag[j]; pb[ph][lane + 64 * j] = ab[j]; }
    __syncthreads();
    const int cl = threadIdx.x, c = c0 + cl;
    if (c < C) {
        float* dst = part + (size_t)blockIdx.y * 2 * C;
        dst[c] = ((pg[0][cl] + pg[1][cl]) + pg[2][cl]) + pg[3][cl];
        dst[C + c] = ((pb[0][cl] + pb[1][cl]) + pb[2][cl]) + pb[3][cl];
    }
}

// ---------------------------------------------------------------------------------------------- projection (one output channel)
// part[chunk][c] = sum of seed[r] h[r][c] over the chunk's rows with t < len_b, c < C; part[chunk][C] = the sum of seed[r].
// grid (ceil((C + 1) / 64), chunks), 256 threads: phase p = tid >> 6, column = 64 blockIdx.x + (tid & 63).
__global__ __launch_bounds__(256) void rows_wgrad_kernel(const float* __restrict__ seed, const float* __restrict__ h, int ldh,
                                                         const int64_t* __restrict__ lengths, int B, int T, int C, int chunk,
                                                         float* __restrict__ part) {
    __shared__ float pp[4][64];
    const int cl = threadIdx.x & 63, ph = threadIdx.x >> 6;
    const int col = blockIdx.x * 64 + cl;
    const int M = B * T;
    const int r_begin = blockIdx.y * chunk;
    const int r_end = min(r_begin + chunk, M);
    float s = 0.f;
    if (col <= C)
        for (int r = r_begin + ph; r < r_end; r += 4) {
            const int b = r / T, t = r - b * T;
            if (t >= dg_len(lengths, b, T)) continue;
            const float sd = seed[r];
            s += col < C ? sd * h[(size_t)r * ldh + col] : sd;
        }
    pp[ph][cl] = s;
    __syncthreads();
    if (ph == 0 && col <= C) part[(size_t)blockIdx.y * (C + 1) + col] = ((pp[0][cl] + pp[1][cl]) + pp[2][cl]) + pp[3][cl];
}

// dst[e] = part[0][e] + part[1][e] + ... in chunk order, e < n; the first n0 results go to dst0, the others to dst1.
__global__ void chunk_sum_kernel(const float* __restrict__ part, int chunks, int n, int n0, float* __restrict__ dst0, float* __restrict__ dst1) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n) return;
    float s = part[e];
    for (int c = 1; c < chunks; ++c) s += part[(size_t)c * n + e];
    if (e < n0) dst0[e] = s;
    else dst1[e - n0] = s;
}

// ---------------------------------------------------------------------------------------------- FiLM projection
// dw[o][j] = sum_b g[b][o] e[b][j] and db[o] = sum_b g[b][o], both in batch order from zero; one thread per element.
__global__ void outer_batch_sum_kernel(const float* __restrict__ g, const float* __restrict__ e, int B, int O, int J, float* __restrict__ dw,
                                       float* __restrict__ db) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t nw = (size_t)O * J;
    if (i < nw) {
        const int o = (int)(i / J), j = (int)(i % J);
        float s = 0.f;
        for (int b = 0; b < B; ++b) s += g[(size_t)b * O + o] * e[(size_t)b * J + j];
        dw[i] = s;
    } else if (i < nw + O) {
        const int o = (int)(i - nw);
        float s = 0.f;
        for (int b = 0; b < B; ++b) s += g[(size_t)b * O + o];
        db[o] = s;
    }
}

static size_t dp_unit_partial_floats(int64_t M, int C) { return (size_t)conv_wgrad_chunks(M) * (size_t)(2 * C); }   // (>= chunks (C + 1))

// part: dp_unit_partial_floats(B T, C) floats
static hipError_t launch_ln_film_wgrad(const float* x, int ldx, const float* dy, int lddy, const float* film, const int64_t* lengths, int B,
                                       int T, int C, float eps, float* dgamma, float* dbeta, float* part, hipStream_t s) {
    if (!x || !dy || !film || !dgamma || !dbeta || !part || B <= 0 || T <= 0 || C <= 0 || ldx < C || lddy < C || (int64_t)B * T > (int64_t)1 << 30)
        return hipErrorInvalidValue;
    const int64_t M = (int64_t)B * T;
    const int chunk = conv_wgrad_chunk_rows(M), chunks = conv_wgrad_chunks(M);
    hipLaunchKernelGGL(ln_film_wgrad_kernel, dim3((C + 255) / 256, chunks), dim3(256), 0, s, x, ldx, dy, lddy, film, lengths, B, T, C, eps, chunk, part);
    hipLaunchKernelGGL(chunk_sum_kernel, dim3((2 * C + 255) / 256), dim3(256), 0, s, part, chunks, 2 * C, C, dgamma, dbeta);
    return hipGetLastError();
}
static hipError_t launch_rows_wgrad(const float* seed, const float* h, int ldh, const int64_t* lengths, int B, int T, int C, float* dw, float* db,
                                    float* part, hipStream_t s) {
    if (!seed || !h || !dw || !db || !part || B <= 0 || T <= 0 || C <= 0 || ldh < C || (int64_t)B * T > (int64_t)1 << 30) return hipErrorInvalidValue;
    const int64_t M = (int64_t)B * T;
    const int chunk = conv_wgrad_chunk_rows(M), chunks = conv_wgrad_chunks(M);
    hipLaunchKernelGGL(rows_wgrad_kernel, dim3((C + 1 + 63) / 64, chunks), dim3(256), 0, s, seed, h, ldh, lengths, B, T, C, chunk, part);
    hipLaunchKernelGGL(chunk_sum_kernel, dim3((C + 1 + 255) / 256), dim3(256), 0, s, part, chunks, C + 1, C, dw, db);
    return hipGetLastError();
}
static hipError_t launch_outer_batch_sum(const float* g, const float* e, int B, int O, int J, float* dw, float* db, hipStream_t s) {
    if (!g || !e || !dw || !db || B <= 0 || O <= 0 || J <= 0) return hipErrorInvalidValue;
    const size_t n = (size_t)O * J + O;
    hipLaunchKernelGGL(outer_batch_sum_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, g, e, B, O, J, dw, db);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------- verdict, seed, sums
// verdict [B][2] = (1: x_length outside [1, Tx]; 2: a negative duration among the utterance's tokens; second word: the first such token)
// in score.hip's layout, which walk_dur reads, and the status words (1 + first refused utterance or 0, its length, Tx, its verdict,
// the token) for mtts_dp_grad_status.  One workgroup.
__global__ __launch_bounds__(256) void dp_verdict_kernel(const int64_t* __restrict__ x_len, const int32_t* __restrict__ dur, int B, int Tx,
                                                         int32_t* __restrict__ status, int32_t* __restrict__ verdict) {
    for (int b = threadIdx.x; b < B; b += blockDim.x) {
        int v = 0, at = 0;
        const int64_t n = x_len[b];
        if (n < 1 || n > Tx) v = 1;
        else
            for (int x = 0; x < (int)n; ++x)
                if (dur[(size_t)b * Tx + x] < 0) { v = 2; at = x; break; }
        verdict[2 * b] = v;
        verdict[2 * b + 1] = at;
    }
    __syncthreads();
    const int i = first_refused_row(B, [&](int r) { return verdict[2 * r] != 0; });
    if (threadIdx.x == 0) {
        status[0] = i < B ? i + 1 : 0;
        status[1] = i < B ? sat32(x_len[i]) : 0;
        status[2] = Tx;
        status[3] = i < B ? verdict[2 * i] : 0;
        status[4] = i < B ? verdict[2 * i + 1] : 0;
    }
}
// mtts_spk_grad's seed_logw with the seed itself kept: seed[row] = clamp(logw - log(2 + dur), +-delta) for x < len_b of an accepted
// utterance, else 0; gd[row][c] = seed * w_proj[c] (the projection has one output channel: its transpose is this outer product).
__global__ void dp_seed_kernel(const float* __restrict__ logw, const int32_t* __restrict__ dur, const int64_t* __restrict__ x_len,
                               const int32_t* __restrict__ verdict, const float* __restrict__ w_proj, int Tx, int Fd, float delta,
                               float* __restrict__ seed, float* __restrict__ gd) {
    const int row = blockIdx.x, b = row / Tx, x = row % Tx;
    float sd = 0.f;
    if (verdict[2 * b] == 0 && x < (int)x_len[b]) sd = fminf(fmaxf(logw[row] - logf(2.0f + (float)dur[row]), -delta), delta);
    if (threadIdx.x == 0) seed[row] = sd;
    for (int c = threadIdx.x; c < Fd; c += blockDim.x) gd[(size_t)row * Fd + c] = sd * w_proj[c];
}
// dur_sum[b] = the Huber sum of score.hip (torch.nn.functional.huber_loss terms) over the tokens x < len_b: lane l adds x = l, l + 64, ...
// in order, then a wave butterfly.  Zero for a refused utterance.  One wave per utterance.
__global__ __launch_bounds__(64) void dp_sum_kernel(const float* __restrict__ logw, const int32_t* __restrict__ dur, const int64_t* __restrict__ x_len,
                                                    const int32_t* __restrict__ verdict, int Tx, float delta, float* __restrict__ dur_sum) {
    const int b = blockIdx.x, lane = threadIdx.x;
    const int txb = verdict[2 * b] == 0 ? (int)x_len[b] : 0;
    float e = 0.f;
    for (int x = lane; x < txb; x += 64) {
        const float d = logw[(size_t)b * Tx + x] - logf(2.0f + (float)dur[(size_t)b * Tx + x]);
        const float ad = fabsf(d);
        e += ad < delta ? 0.5f * d * d : delta * (ad - 0.5f * delta);
    }
    e = dg_wave_sum(e);
    if (lane == 0) dur_sum[b] = e;
}

static hipError_t launch_dp_verdict(const int64_t* x_len, const int32_t* dur, int B, int Tx, int32_t* status, int32_t* verdict, hipStream_t s) {
    hipLaunchKernelGGL(dp_verdict_kernel, dim3(1), dim3(256), 0, s, x_len, dur, B, Tx, status, verdict);
    return hipGetLastError();
}
static hipError_t launch_dp_seed(const float* logw, const int32_t* dur, const int64_t* x_len, const int32_t* verdict, const float* w_proj, int M,
                                 int Tx, int Fd, float delta, float* seed, float* gd, hipStream_t s) {
    hipLaunchKernelGGL(dp_seed_kernel, dim3(M), dim3(64), 0, s, logw, dur, x_len, verdict, w_proj, Tx, Fd, delta, seed, gd);
    return hipGetLastError();
}
static hipError_t launch_dp_sum(const float* logw, const int32_t* dur, const int64_t* x_len, const int32_t* verdict, int B, int Tx, float delta,
                                float* dur_sum, hipStream_t s) {
    hipLaunchKernelGGL(dp_sum_kernel, dim3(B), dim3(64), 0, s, logw, dur, x_len, verdict, Tx, delta, dur_sum);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------- parameters and the component (host)
struct DpParam { std::string key; size_t off, numel; };
// The flat parameter vector: the keys under encoder.proj_w. in state-dict order
static std::vector<DpParam> dp_params(const mtts_config& g) {
    std::vector<DpParam> p;
    size_t off = 0;
    auto add = [&](const std::string& key, size_t n) { p.push_back({key, off, n}); off += n; };
    const int Sd = g.spk_emb_dim, Hd = g.enc_channels + Sd, F = g.dp_filter;
    add("spk_proj.weight", (size_t)2 * F * Sd);
    add("spk_proj.bias", (size_t)2 * F);
    for (int i = 0; i < g.dp_layers; ++i) {
        const std::string n = std::to_string(i);
        add("conv_layers." + n + ".weight", (size_t)F * (i == 0 ? Hd : F) * g.dp_kernel);
        add("conv_layers." + n + ".bias", F);
        add("norm_layers." + n + ".gamma", F);
        add("norm_layers." + n + ".beta", F);
    }
    add("proj.weight", F);
    add("proj.bias", 1);
    return p;
}
static size_t dp_param_total(const mtts_config& g) {
    const std::vector<DpParam> p = dp_params(g);
    return p.back().off + p.back().numel;
}
// The same offsets as plain numbers, for the launch path (no strings, no host allocation there)
struct DpOffsets {
    size_t film_w = 0, film_b = 0, conv_w[SG_MAX_LAYERS] = {}, conv_b[SG_MAX_LAYERS] = {}, gamma[SG_MAX_LAYERS] = {}, beta[SG_MAX_LAYERS] = {},
           proj_w = 0, proj_b = 0;
};
static DpOffsets dp_offsets(const mtts_config& g) {
    DpOffsets o;
    const size_t Sd = g.spk_emb_dim, Hd = g.enc_channels + Sd, F = g.dp_filter;
    size_t off = 0;
    o.film_w = off; off += 2 * F * Sd;
    o.film_b = off; off += 2 * F;
    for (int i = 0; i < g.dp_layers && i < SG_MAX_LAYERS; ++i) {
        o.conv_w[i] = off; off += F * (i == 0 ? Hd : F) * g.dp_kernel;
        o.conv_b[i] = off; off += F;
        o.gamma[i] = off; off += F;
        o.beta[i] = off; off += F;
    }
    o.proj_w = off; off += F;
    o.proj_b = off;
    return o;
}
static bool dp_arch_ok(const char* who, const mtts_ctx* c) {
    if (c->cfg.dp_kernel != WG_TAPS) { set_error(std::string(who) + ": the weight-gradient kernel is written for dp_kernel == 5"); return false; }
    if (c->cfg.dp_layers < 1 || c->cfg.dp_layers > SG_MAX_LAYERS || c->cfg.enc_layers > SG_MAX_LAYERS) {
        set_error(std::string(who) + ": more than 16 encoder or duration-predictor layers");
        return false;
    }
    return true;
}

// params: dp_param_total floats.  The layout of the image depends on the configuration alone, so every repack lands at the same offsets.
static int pack_dp_train(mtts_ctx* c, const float* params) {
    const mtts_config& g = c->cfg;
    Component& T = c->dptrain;
    T.image.clear();
    T.gemm_terms = 0;             // native fp32 MFMA (file header)
    T.packed = false;
    Packer P(&T);
    DpTrainW& W = c->dptw;
    W = DpTrainW();
    const int Sd = g.spk_emb_dim, Hd = g.enc_channels + Sd, F = g.dp_filter, k = g.dp_kernel;
    const std::vector<DpParam> L = dp_params(g);
    size_t at = 0;
    auto next = [&]() { return params + L[at++].off; };
    auto vec = [&](const float* src, int n) {
        Vec v;
        v.off = P.alloc(n);
        v.n = n;
        std::memcpy(&T.image[v.off], src, n * sizeof(float));
        return v;
    };
    {
        const float* w = next();
        const float* b = next();
        W.film = P.panel_from(w, b, 0, 2 * F, Sd, 1);
        const std::vector<float> t = transposed(w, 2 * F, Sd, 1);
        W.filmT = P.panel_from(t.data(), nullptr, 0, Sd, 2 * F, 1);
    }
    for (int i = 0; i < g.dp_layers; ++i) {
        const int cin = i == 0 ? Hd : F;
        const float* w = next();
        const float* b = next();
        W.conv.push_back(P.panel_from(w, b, 1, F, cin, k));
        if (i == 0) W.convT.push_back(Panel());
        else {
            const std::vector<float> t = transposed(w, F, F, k);
            W.convT.push_back(P.panel_from(t.data(), nullptr, 1, F, F, k));
        }
        W.gamma.push_back(vec(next(), F));
        W.beta.push_back(vec(next(), F));
    }
    {
        const float* w = next();
        const float* b = next();
        W.proj = P.panel_from(w, b, 1, 1, F, 1);
        W.proj_w = vec(w, F);
        W.proj_b = vec(b, 1);
    }
    if (!P.ok) { set_error("mtts_dp_train weights: " + P.why); return -1; }
    T.packed = true;
    return 0;
}
// the flat vector from the tensors registered with mtts_set_tensor
static int dp_params_from_raw(const mtts_ctx* c, std::vector<float>& out) {
    const std::vector<DpParam> L = dp_params(c->cfg);
    out.assign(L.back().off + L.back().numel, 0.f);
    for (const DpParam& p : L) {
        auto it = c->raw.find("encoder.proj_w." + p.key);
        if (it == c->raw.end()) { set_error("mtts_dp_train_upload: missing tensor encoder.proj_w." + p.key); return -1; }
        if (it->second.size() != p.numel) { set_error("mtts_dp_train_upload: tensor encoder.proj_w." + p.key + " has an unexpected size"); return -1; }
        std::memcpy(&out[p.off], it->second.data(), p.numel * sizeof(float));
    }
    return 0;
}
static int dp_pack_any(mtts_ctx* c, const float* h_params) {
    if (h_params) return pack_dp_train(c, h_params);
    std::vector<float> flat;
    RET_IF(dp_params_from_raw(c, flat));
    return pack_dp_train(c, flat.data());
}

// ---------------------------------------------------------------------------------------------- plan
struct DpBufs {
    float *DF[SG_MAX_LAYERS], *seed, *PART;
    int32_t *status, *verdict;
    size_t off_hout = 0, off_logw = 0;
};
static void plan_dp_grad(const mtts_ctx* c, int B, int Tx, WS& ws, SgBufs& e, DpBufs& d) {
    const mtts_config& g = c->cfg;
    const size_t M = (size_t)B * Tx;
    const int nch = g.enc_channels, Hd = nch + g.spk_emb_dim, F = g.dp_filter;
    (void)ws.bytes(256);                 // header: the call's range flag (begin_call)
    d.status = static_cast<int32_t*>(ws.bytes(256));       // at SG_SCORE_OFF, where mtts_dp_grad_status looks
    d.verdict = static_cast<int32_t*>(ws.bytes((size_t)B * 2 * sizeof(int32_t)));
    e.xm = ws.f(M);
    e.X0 = ws.f(M * nch); e.P1 = ws.f(M * nch); e.P2 = ws.f(M * nch); e.Y = ws.f(M * nch);
    const int L = std::min(g.enc_layers, SG_MAX_LAYERS), Ld = std::min(g.dp_layers, SG_MAX_LAYERS);
    for (int l = 0; l <= L; ++l) e.Hin[l] = ws.f(M * Hd);
    d.off_hout = ws.off - M * Hd * sizeof(float);
    for (int l = 0; l < L; ++l) {
        e.QKV[l] = ws.f(M * 3 * Hd); e.ATT[l] = ws.f(M * Hd); e.S1[l] = ws.f(M * Hd); e.H1[l] = ws.f(M * Hd);
        e.F1[l] = ws.f(M * g.enc_filter); e.S2[l] = ws.f(M * Hd);
    }
    e.FILM = ws.f((size_t)B * 2 * F);
    for (int i = 0; i < Ld; ++i) { e.DY[i] = ws.f(M * F); d.DF[i] = ws.f(M * F); }
    e.logw = ws.f(M); d.off_logw = ws.off - M * sizeof(float);
    d.seed = ws.f(M);
    e.GDA = ws.f(M * F); e.GDB = ws.f(M * F); e.FPROD = ws.f(M * F); e.DFILM = ws.f((size_t)B * 2 * F);
    d.PART = ws.f(std::max(conv_wgrad_partial_floats((int64_t)M, std::max(Hd, F), F), dp_unit_partial_floats((int64_t)M, F)));
}
// What walk_dur calls back once per layer (DurTrain::reduce): that layer's LayerNorm + FiLM affines and its convolution's weights
struct DpReduce {
    mtts_ctx* c;
    const SgBufs* e;
    const DpBufs* d;
    const DpOffsets* O;
    float* d_grad;
    const int64_t* d_x_lengths;
    const float* Hout;
    hipStream_t s;
    int B, Tx, F, Hd;
    static int layer(void* self, int i) {
        const DpReduce& r = *static_cast<const DpReduce*>(self);
        LAUNCH(r.c, 2, 0, r.s, launch_ln_film_wgrad(r.e->DY[i], r.F, r.e->GDA, r.F, r.e->FILM, r.d_x_lengths, r.B, r.Tx, r.F, 1e-5f,
                                                    r.d_grad + r.O->gamma[i], r.d_grad + r.O->beta[i], r.d->PART, r.s));
        const float* in = i ? r.d->DF[i - 1] : r.Hout;
        const int cin = i ? r.F : r.Hd;
        LAUNCHB(r.c, 0, conv_wgrad_flops(r.B, r.Tx, cin, r.F), 0.0, r.s,
                launch_conv_wgrad(r.e->GDB, r.F, in, cin, r.d_x_lengths, r.B, r.Tx, cin, r.F, r.d_grad + r.O->conv_w[i], r.d_grad + r.O->conv_b[i],
                                  r.d->PART, r.s));
        return 0;
    }
};
static bool dp_shape_ok(const char* who, int B, int Tx) {
    if (B < 1 || B > 65535) { set_error(std::string(who) + ": B must be in [1, 65535]"); return false; }
    if (Tx < 1 || Tx > SG_MAX_TX) { set_error(std::string(who) + ": Tx must be in [1, 1024]"); return false; }
    return true;
}

}  // namespace mtts

using namespace mtts;

extern "C" {

int64_t mtts_dp_param_count(mtts_ctx* c) {
    if (!c) { set_error("mtts_dp_param_count: null context"); return -1; }
    return (int64_t)dp_param_total(c->cfg);
}
int64_t mtts_dp_param_offset(mtts_ctx* c, const char* key) {
    if (!c || !key) { set_error("mtts_dp_param_offset: null argument"); return -1; }
    for (const DpParam& p : dp_params(c->cfg))
        if (p.key == key) return (int64_t)p.off;
    set_error(std::string("mtts_dp_param_offset: no parameter named ") + key);
    return -1;
}

int64_t mtts_dp_train_weights_bytes(mtts_ctx* c) {
    if (!c) { set_error("mtts_dp_train_weights_bytes: null context"); return -1; }
    if (!dp_arch_ok("mtts_dp_train_weights_bytes", c)) return -1;
    if (!c->dptrain.packed) {            // the size depends on the configuration alone: pack zeros once to learn it
        const std::vector<float> zeros(dp_param_total(c->cfg), 0.f);
        RET_IF(pack_dp_train(c, zeros.data()));
        c->dptrain.uploaded = false;
    }
    return (int64_t)(c->dptrain.image.size() * sizeof(float));
}
// The packed component as it would be uploaded, to the host (what the tests compare): h_out of mtts_dp_train_weights_bytes bytes.
int mtts_dp_train_pack(mtts_ctx* c, const float* h_params, void* h_out, int64_t bytes) {
    if (!c || !h_out) { set_error("mtts_dp_train_pack: null argument"); return -1; }
    if (!dp_arch_ok("mtts_dp_train_pack", c)) return -1;
    CTX_GUARD(c);
    c->dptrain.uploaded = false;
    RET_IF(dp_pack_any(c, h_params));
    if ((size_t)bytes < c->dptrain.image.size() * sizeof(float)) { set_error("mtts_dp_train_pack: buffer too small (mtts_dp_train_weights_bytes)"); return -1; }
    std::memcpy(h_out, c->dptrain.image.data(), c->dptrain.image.size() * sizeof(float));
    return 0;
}
int mtts_dp_train_upload(mtts_ctx* c, const float* h_params, void* d_buf, int64_t bytes) {
    if (!c || !d_buf) { set_error("mtts_dp_train_upload: null argument"); return -1; }
    if (!dp_arch_ok("mtts_dp_train_upload", c)) return -1;
    CTX_GUARD(c);
    Component& T = c->dptrain;
    T.uploaded = false;
    RET_IF(dp_pack_any(c, h_params));
    if ((size_t)bytes < T.image.size() * sizeof(float)) { set_error("mtts_dp_train_upload: buffer too small (mtts_dp_train_weights_bytes)"); return -1; }
    HIP_OK(hipMemcpy(d_buf, T.image.data(), T.image.size() * sizeof(float), hipMemcpyHostToDevice));
    T.d_image = static_cast<float*>(d_buf);
    T.uploaded = true;
    return 0;
}

int64_t mtts_dp_grad_workspace_bytes(mtts_ctx* c, int B, int Tx) {
    if (!c) { set_error("mtts_dp_grad_workspace_bytes: null context"); return -1; }
    if (!dp_shape_ok("mtts_dp_grad_workspace_bytes", B, Tx) || !dp_arch_ok("mtts_dp_grad_workspace_bytes", c)) return -1;
    WS ws(nullptr, 0);
    SgBufs e;
    DpBufs d;
    plan_dp_grad(c, B, Tx, ws, e, d);
    return (int64_t)ws.off + 256;
}
// Byte offset inside the workspace of what the latest call's forward left: which 0 the frozen encoder's output rows [B Tx][Hd] (the rows
// the predictor reads), 1 logw [B][Tx] of the predictor under training.
int64_t mtts_dp_grad_tape_offset(mtts_ctx* c, int B, int Tx, int which) {
    if (!c) { set_error("mtts_dp_grad_tape_offset: null context"); return -1; }
    if (!dp_shape_ok("mtts_dp_grad_tape_offset", B, Tx) || !dp_arch_ok("mtts_dp_grad_tape_offset", c)) return -1;
    if (which < 0 || which > 1) { set_error("mtts_dp_grad_tape_offset: which must be 0 (encoder rows) or 1 (logw)"); return -1; }
    WS ws(nullptr, 0);
    SgBufs e;
    DpBufs d;
    plan_dp_grad(c, B, Tx, ws, e, d);
    return (int64_t)(which == 0 ? d.off_hout : d.off_logw);
}

int mtts_dp_grad(mtts_ctx* c, const int64_t* d_x, const int64_t* d_x_lengths, const float* d_e_enc, const float* d_e_dur,
                 const int32_t* d_durations, float delta_dur, int B, int Tx, void* d_train_buf, float* d_grad, float* d_g_dur,
                 float* d_dur_sum, float* d_logw, void* d_ws, int64_t ws_bytes, void* stream) {
    if (!c || !d_x || !d_x_lengths || !d_e_enc || !d_e_dur || !d_durations || !d_train_buf || !d_grad || !d_dur_sum || !d_ws) {
        set_error("mtts_dp_grad: null argument");
        return -1;
    }
    if (!dp_shape_ok("mtts_dp_grad", B, Tx) || !dp_arch_ok("mtts_dp_grad", c)) return -1;
    if (!(delta_dur > 0.f)) { set_error("mtts_dp_grad: the Huber threshold must be positive"); return -1; }
    CTX_GUARD(c);
    WS ws(d_ws, (size_t)ws_bytes);
    SgBufs e;
    DpBufs d;
    plan_dp_grad(c, B, Tx, ws, e, d);
    if (ws.overflow || ws_bytes < (int64_t)ws.off) { set_error("mtts_dp_grad: workspace too small (mtts_dp_grad_workspace_bytes)"); return -1; }
    if (reinterpret_cast<uintptr_t>(d_ws) & 15) { set_error("mtts_dp_grad: workspace must be 16-byte aligned"); return -1; }
    if (reinterpret_cast<char*>(d.status) - static_cast<char*>(d_ws) != (ptrdiff_t)SG_SCORE_OFF) {
        set_error("mtts_dp_grad: the status words are not where mtts_dp_grad_status reads them");
        return -1;
    }
    const Component* T = &c->dptrain;
    if (!T->packed || !T->uploaded || T->d_image != d_train_buf) {
        set_error("mtts_dp_grad: training component not uploaded (mtts_dp_train_upload into d_train_buf)");
        return -1;
    }
    RET_IF(check_ready(c));
    hipStream_t s = static_cast<hipStream_t>(stream);
    const SgCall k(c, e, s, B, Tx);
    if ((size_t)Tx * k.d_rope > (size_t)k.E.rope_cos.n) { set_error("Phonetic representation too long, exceeds RoPE cache size"); return -1; }
    const mtts_config& g = c->cfg;
    const DpTrainW& TW = c->dptw;
    const int F = k.F, Hd = k.Hd, Sd = k.Sd, Ld = g.dp_layers;
    const DpOffsets O = dp_offsets(g);
    RET_IF(begin_call(c, d_ws, s));
    LAUNCH(c, 2, 0, s, launch_dp_verdict(d_x_lengths, d_durations, B, Tx, d.status, d.verdict, s));

    // ================================================================ frozen encoder, then the predictor from the training component
    RET_IF(k.forward_encoder(d_x, d_x_lengths, d_e_enc));
    const float* Hout = e.Hin[k.L];
    float* logw = d_logw ? d_logw : e.logw;
    {
        GemmArgs fm;
        panel_args(T, TW.film, fm); rows_plain(fm, B, 1);
        fm.a0 = d_e_dur; fm.lda0 = Sd; fm.c0 = Sd; fm.out = e.FILM; fm.ldc = 2 * F;
        RET_IF(run_gemm(c, fm, s));
        const float* dcur = Hout;
        int dc = Hd;
        for (int i = 0; i < Ld; ++i) {
            GemmArgs a;
            panel_args(T, TW.conv[i], a); rows_plain(a, B, Tx); taps_centered(a, g.dp_kernel);
            a.a0 = dcur; a.lda0 = dc; a.c0 = dc; a.a_mask = k.xm; a.act = ACT_RELU; a.out = e.DY[i]; a.ldc = F;
            RET_IF(run_gemm(c, a, s));
            LayerNormArgs ln;
            ln.x = e.DY[i]; ln.ldx = F; ln.y = d.DF[i]; ln.ldy = F; ln.M = k.M; ln.C = F; ln.T = Tx;
            ln.gamma = W(T, TW.gamma[i].off); ln.beta = W(T, TW.beta[i].off); ln.film = e.FILM;
            LAUNCH(c, 2, 0, s, launch_layernorm(ln, s));
            dcur = d.DF[i];
            dc = F;
        }
        GemmArgs p;
        panel_args(T, TW.proj, p); rows_plain(p, B, Tx);
        p.a0 = dcur; p.lda0 = dc; p.c0 = dc; p.a_mask = k.xm; p.out_mask = k.xm; p.out = logw; p.ldc = 1;
        RET_IF(run_gemm(c, p, s));
    }

    // ================================================================ sums, seed, and the walk back with the reductions inside it
    LAUNCH(c, 2, 0, s, launch_dp_sum(logw, d_durations, d_x_lengths, d.verdict, B, Tx, delta_dur, d_dur_sum, s));
    LAUNCH(c, 2, 0, s, launch_dp_seed(logw, d_durations, d_x_lengths, d.verdict, W(T, TW.proj_w.off), k.M, Tx, F, delta_dur, d.seed, e.GDA, s));
    LAUNCH(c, 2, 0, s, launch_rows_wgrad(d.seed, d.DF[Ld - 1], F, d_x_lengths, B, Tx, F, d_grad + O.proj_w, d_grad + O.proj_b, d.PART, s));
    DpReduce red{c, &e, &d, &O, d_grad, d_x_lengths, Hout, s, B, Tx, F, Hd};
    DurTrain tr;
    tr.comp = T;
    tr.convT = TW.convT.data();
    tr.filmT = TW.filmT;
    for (int i = 0; i < Ld; ++i) { tr.gamma[i] = W(T, TW.gamma[i].off); tr.beta[i] = W(T, TW.beta[i].off); }
    tr.reduce = &DpReduce::layer;
    tr.reduce_ctx = &red;
    RET_IF(k.walk_dur(d_x_lengths, d.verdict, d_g_dur, &tr));
    LAUNCH(c, 2, 0, s, launch_outer_batch_sum(e.DFILM, d_e_dur, B, 2 * F, Sd, d_grad + O.film_w, d_grad + O.film_b, s));
    return 0;
}

// The verdict of mtts_dp_grad's device-side check of the lengths and durations.  The one entry here that waits for the stream.
int mtts_dp_grad_status(const void* d_ws, void* stream) {
    if (!d_ws) { set_error("mtts_dp_grad_status: null workspace"); return -1; }
    int st[8];
    if (read_status("mtts_dp_grad_status", static_cast<const char*>(d_ws) + SG_SCORE_OFF, stream, st)) return -1;
    if (st[0] != 0) {
        if (st[3] == 2)
            set_error("mtts_dp_grad: utterance " + std::to_string(st[0] - 1) + " has a negative duration at token " + std::to_string(st[4]));
        else
            set_error("mtts_dp_grad: utterance " + std::to_string(st[0] - 1) + " has x_length = " + std::to_string(st[1]) +
                      " (need 1 <= x_length <= Tx = " + std::to_string(st[2]) + ")");
        return -1;
    }
    return 0;
}

// ---------------------------------------------------------------------------------------------- unit entries (kernel-level parity)
int64_t mtts_dp_unit_workspace_bytes(int B, int T, int C) {
    if (B < 1 || T < 1 || C < 1 || (int64_t)B * T > (int64_t)1 << 30) { set_error("mtts_dp_unit_workspace_bytes: bad shape"); return -1; }
    return (int64_t)(dp_unit_partial_floats((int64_t)B * T, C) * sizeof(float));
}
int mtts_ln_film_wgrad(const float* d_x, const float* d_dy, const float* d_film, const int64_t* d_lengths, int B, int T, int C, float eps,
                       float* d_dgamma, float* d_dbeta, void* d_ws, int64_t ws_bytes, void* stream) {
    if (!d_x || !d_dy || !d_film || !d_dgamma || !d_dbeta || !d_ws) { set_error("mtts_ln_film_wgrad: null argument"); return -1; }
    if (B < 1 || T < 1 || C < 1 || (int64_t)B * T > (int64_t)1 << 30) { set_error("mtts_ln_film_wgrad: bad shape"); return -1; }
    if (ws_bytes < mtts_dp_unit_workspace_bytes(B, T, C)) { set_error("mtts_ln_film_wgrad: workspace too small (mtts_dp_unit_workspace_bytes)"); return -1; }
    HIP_OK(launch_ln_film_wgrad(d_x, C, d_dy, C, d_film, d_lengths, B, T, C, eps, d_dgamma, d_dbeta, static_cast<float*>(d_ws),
                                static_cast<hipStream_t>(stream)));
    return 0;
}
int mtts_rows_wgrad(const float* d_seed, const float* d_h, const int64_t* d_lengths, int B, int T, int C, float* d_dw, float* d_db, void* d_ws,
                    int64_t ws_bytes, void* stream) {
    if (!d_seed || !d_h || !d_dw || !d_db || !d_ws) { set_error("mtts_rows_wgrad: null argument"); return -1; }
    if (B < 1 || T < 1 || C < 1 || (int64_t)B * T > (int64_t)1 << 30) { set_error("mtts_rows_wgrad: bad shape"); return -1; }
    if (ws_bytes < mtts_dp_unit_workspace_bytes(B, T, C)) { set_error("mtts_rows_wgrad: workspace too small (mtts_dp_unit_workspace_bytes)"); return -1; }
    HIP_OK(launch_rows_wgrad(d_seed, d_h, C, d_lengths, B, T, C, d_dw, d_db, static_cast<float*>(d_ws), static_cast<hipStream_t>(stream)));
    return 0;
}
int mtts_outer_batch_sum(const float* d_g, const float* d_e, int B, int O, int J, float* d_dw, float* d_db, void* stream) {
    if (!d_g || !d_e || !d_dw || !d_db) { set_error("mtts_outer_batch_sum: null argument"); return -1; }
    if (B < 1 || O < 1 || J < 1) { set_error("mtts_outer_batch_sum: bad shape"); return -1; }
    HIP_OK(launch_outer_batch_sum(d_g, d_e, B, O, J, d_dw, d_db, static_cast<hipStream_t>(stream)));
    return 0;
}

}  // extern "C"
