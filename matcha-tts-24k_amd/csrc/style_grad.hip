// Parameter gradients of the style encoder (gfx950): the backward of reference matcha/models/style_encoder.py:42-72 for training it on
// the device (reference StyleEncoderLightningModule, style_encoder.py:75-160).  Given upstream g_enc, g_dur [B, E] this file returns the
// gradient of sum_b <g_enc_b, e_enc_b> + <g_dur_b, e_dur_b> with respect to every parameter, in one flat buffer in state-dict order.
//
//   taped forward          the launches of mtts_style_forward (style_encoder.hip) with group == NULL, one activation buffer per layer and
//                          the pooled rows kept
//   style_proj_bwd_kernel  d proj_w = sum_b g (x) pooled, d proj_b = sum_b g (batch order), d pooled = g W (output order)
//   style_pool_bwd_kernel  d H = d pooled / max(len, 1) on the frames that exist, times the last layer's ReLU gate
//   conv_wgrad_f32_kernel  THE weight gradient: dW[co, ci, k] = sum over rows r = (b, t) of dZ[r, co] X[(b, t + k - 2), ci], a reduction
//                          over all B T rows, on __builtin_amdgcn_mfma_f32_32x32x2f32
//   wgrad_bias_kernel      d bias = column sums of dZ, per chunk
//   wgrad_reduce_kernel    the chunks' partial results added in chunk order
//   style_gate_kernel      ReLU gate and prefix mask on a data gradient
// The data gradient of layers >= 1 runs on the GEMM launcher with transposed, tap-reversed panels in NATIVE FP32 MFMA (GemmArgs::terms
// 0), packed on demand into a buffer of their own -- what spk_grad.hip does, for the same reason: gradients are small numbers.
//
// Why 32x32x2 f32 and no transposes: both operands are channels-last rows.  The instruction's A lanes hold A[i = l & 31][k = l >> 5]
// and its B lanes B[k = l >> 5][j = l & 31]; with i = output channel, j = input channel and k = the row being summed, a lane reads
// dZ[row + (l >> 5)][co0 + (l & 31)] and X[row + tap + (l >> 5)][ci0 + (l & 31)]: 32 consecutive floats of one row per half wave, from
// LDS without bank conflicts (ds_read_b32 serves lanes 0-31 and 32-63 in separate cycles), and the five taps read the same staged rows.
// The result of an MFMA is a k-ordered fp32 FMA chain, so a workgroup adds its rows in row order.
//
// Fixed order: the rows are cut into chunks of conv_wgrad_chunk_rows(B, T) rows -- a function of the shape alone, never of the device --
// each chunk's sum is one serial chain, and the chunks are added in chunk order by a second kernel.  No atomics: two calls give the same
// bits on any partition of the device.
#include "conv_wgrad.h"

#include <string>

namespace mtts {

constexpr int WG_SLAB = 32;          // rows staged in LDS per step (16 MFMA k-steps of 2 rows)
constexpr int WG_TILE = 64;          // output channels x input channels per workgroup: 2 x 2 waves of 32 x 32, five taps each
// (WG_TAPS, the chunk constants and conv_wgrad_chunk_rows / _chunks / _partial_floats: conv_wgrad.h, shared with dp_grad.hip)

__device__ __forceinline__ int wg_frames(const int64_t* __restrict__ lengths, int b, int T) {
    if (!lengths) return T;
    const int64_t n = lengths[b];
    return n < 0 ? 0 : (n > (int64_t)T ? T : (int)n);
}

using wg_f32x16 = __attribute__((ext_vector_type(16))) float;

// grid (ceil(cin / 64), ceil(cout / 64), chunks), 256 threads.  Wave w owns output channels co0 + 32 (w >> 1) .. + 31 and input channels
// ci0 + 32 (w & 1) .. + 31.  A row (b, t) takes part when t < len_b; its tap k reads row t + k - 2 of the SAME clip when that lies in
// [0, len_b) -- rows T - 1 of clip b and 0 of clip b + 1 are neighbours in memory and never see each other -- and zero otherwise.  Both
// are selects, not products: what lies beyond a clip's length is never used as data.  Channels beyond cin / cout are staged as zeros and
// not stored.
__global__ __launch_bounds__(256) void conv_wgrad_f32_kernel(const float* __restrict__ dz, int ldz, const float* __restrict__ x, int ldx,
                                                             const int64_t* __restrict__ lengths, int B, int T, int cin, int cout, int chunk,
                                                             float* __restrict__ part) {
    __shared__ float Zs[WG_SLAB][WG_TILE];
    __shared__ float Xs[WG_SLAB + WG_TAPS - 1][WG_TILE];
    __shared__ int trow[WG_SLAB], lrow[WG_SLAB];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31, hi = lane >> 5;
    const int ci0 = blockIdx.x * WG_TILE, co0 = blockIdx.y * WG_TILE;
    const int wco = (wave >> 1) * 32, wci = (wave & 1) * 32;
    const int M = B * T;                          // (<= 2^30: launch_conv_wgrad)
    const int r_begin = blockIdx.z * chunk;
    const int r_end = min(r_begin + chunk, M);
    const bool live = co0 + wco < cout && ci0 + wci < cin;      // (uniform per wave)
    wg_f32x16 acc[WG_TAPS];
#pragma unroll
    for (int k = 0; k < WG_TAPS; ++k)
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[k][i] = 0.f;
    // The next slab travels from global memory to registers while the MFMAs of this one run: 8 floats of dZ and 9 of X per thread
    // (32 x 64 and 36 x 64 elements over 256 threads).
    constexpr int ZN = WG_SLAB * WG_TILE / 256, XN = (WG_SLAB + WG_TAPS - 1) * WG_TILE / 256;
    static_assert(ZN * 256 == WG_SLAB * WG_TILE && XN * 256 == (WG_SLAB + WG_TAPS - 1) * WG_TILE, "slab sizes are multiples of the workgroup");
    float zr[ZN], xr[XN];
    const int c_l = tid & 63, row_l = tid >> 6;   // element e = tid + 256 i sits at row (e >> 6) = row_l + 4 i, column c_l
    const bool z_col = co0 + c_l < cout, x_col = ci0 + c_l < cin;
    auto fetch = [&](int r0) {
#pragma unroll
        for (int i = 0; i < ZN; ++i) {
            const int r = r0 + row_l + 4 * i;
            zr[i] = (z_col && r < r_end) ? dz[(size_t)r * ldz + co0 + c_l] : 0.f;
        }
#pragma unroll
        for (int i = 0; i < XN; ++i) {
            const int r = r0 - WG_TAPS / 2 + row_l + 4 * i;
            xr[i] = (x_col && r >= 0 && r < M) ? x[(size_t)r * ldx + ci0 + c_l] : 0.f;
        }
    };
    fetch(r_begin);
    for (int r0 = r_begin; r0 < r_end; r0 += WG_SLAB) {
        __syncthreads();
#pragma unroll
        for (int i = 0; i < ZN; ++i) Zs[row_l + 4 * i][c_l] = zr[i];
#pragma unroll
        for (int i = 0; i < XN; ++i) Xs[row_l + 4 * i][c_l] = xr[i];
        if (tid < WG_SLAB) {
            const int r = r0 + tid;
            int t = 0, n = 0;
            if (r < r_end) {
                const int b = r / T;
                t = r - b * T;
                n = wg_frames(lengths, b, T);
            }
            trow[tid] = t;
            lrow[tid] = n;
        }
        __syncthreads();
        if (r0 + WG_SLAB < r_end) fetch(r0 + WG_SLAB);
        if (live) {
#pragma unroll 4
            for (int s2 = 0; s2 < WG_SLAB / 2; ++s2) {
                const int row = 2 * s2 + hi;
                const int t = trow[row], n = lrow[row];
                const float a = t < n ? Zs[row][wco + l31] : 0.f;
#pragma unroll
                for (int k = 0; k < WG_TAPS; ++k) {
                    const int tt = t + k - WG_TAPS / 2;
                    const float bv = (tt >= 0 && tt < n) ? Xs[row + k][wci + l31] : 0.f;
                    acc[k] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, bv, acc[k], 0, 0, 0);
                }
            }
        }
    }
    if (!live) return;
    const int ci = ci0 + wci + l31;
    float* dst = part + (size_t)blockIdx.z * WG_TAPS * cout * cin;
#pragma unroll
    for (int k = 0; k < WG_TAPS; ++k)
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int co = co0 + wco + (i & 3) + 8 * (i >> 2) + 4 * hi;
            if (co < cout && ci < cin) dst[((size_t)k * cout + co) * cin + ci] = acc[k][i];
        }
}

// d bias partials: part_b[chunk][co] = sum of dz[r][co] over the chunk's rows with t < len_b, four phases r = p, p + 4, ... in row order
// combined as ((p0 + p1) + p2) + p3.  grid (ceil(cout / 64), chunks), 256 threads.
__global__ __launch_bounds__(256) void wgrad_bias_kernel(const float* __restrict__ dz, int ldz, const int64_t* __restrict__ lengths, int B, int T,
                                                         int cout, int chunk, float* __restrict__ part_b) {
    __shared__ float part[4][64];
    const int cl = threadIdx.x & 63, ph = threadIdx.x >> 6;
    const int co = blockIdx.x * 64 + cl;
    const int M = B * T;
    const int r_begin = blockIdx.y * chunk;
    const int r_end = min(r_begin + chunk, M);
    float s = 0.f;
    if (co < cout && r_begin + ph < r_end) {
        int b = (r_begin + ph) / T, t = (r_begin + ph) - b * T;      // (b, t) of the row, carried along: t += 4 with carry into b
        int n = wg_frames(lengths, b, T);
        for (int r = r_begin + ph; r < r_end; r += 32) {             // eight independent loads in flight, added in row order
            float v[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                v[j] = (r + 4 * j < r_end && t < n) ? dz[(size_t)(r + 4 * j) * ldz + co] : 0.f;
                t += 4;
                while (t >= T) { t -= T; ++b; n = b < B ? wg_frames(lengths, b, T) : 0; }
            }
#pragma unroll
            for (int j = 0; j < 8; ++j) s += v[j];                    // (a row that does not take part adds an exact zero)
        }
    }
    part[ph][cl] = s;
    __syncthreads();
    if (ph == 0 && co < cout) part_b[(size_t)blockIdx.y * cout + co] = ((part[0][cl] + part[1][cl]) + part[2][cl]) + part[3][cl];
}

// dw [cout][cin][5] (torch layout) and db [cout] = the chunks' partials added in chunk order; one thread per element.
__global__ void wgrad_reduce_kernel(const float* __restrict__ part_w, const float* __restrict__ part_b, int chunks, int cin, int cout,
                                    float* __restrict__ dw, float* __restrict__ db) {
    const size_t nw = (size_t)cout * cin * WG_TAPS;
    const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e < nw) {
        const int k = (int)(e % WG_TAPS);
        const size_t cc = e / WG_TAPS;
        const int ci = (int)(cc % cin), co = (int)(cc / cin);
        const float* p = part_w + ((size_t)k * cout + co) * cin + ci;
        float s = p[0];
        for (int c = 1; c < chunks; ++c) s += p[(size_t)c * nw];
        dw[e] = s;
    } else if (db && e < nw + cout) {
        const int co = (int)(e - nw);
        float s = part_b[co];
        for (int c = 1; c < chunks; ++c) s += part_b[(size_t)c * cout + co];
        db[co] = s;
    }
}

// The whole weight (and bias) gradient of one Conv1d(k5, pad 2): three launches.  part: conv_wgrad_partial_floats floats.
hipError_t launch_conv_wgrad(const float* dz, int ldz, const float* x, int ldx, const int64_t* lengths, int B, int T, int cin, int cout,
                             float* dw, float* db, float* part, hipStream_t s) {
    if (!dz || !x || !dw || !part || B <= 0 || T <= 0 || cin <= 0 || cout <= 0 || ldx < cin || ldz < cout ||
        (int64_t)B * T > (int64_t)1 << 30)
        return hipErrorInvalidValue;
    const int64_t M = (int64_t)B * T;
    const int chunk = conv_wgrad_chunk_rows(M), chunks = conv_wgrad_chunks(M);
    const int tci = (cin + WG_TILE - 1) / WG_TILE, tco = (cout + WG_TILE - 1) / WG_TILE;
    if (tco > 65535) return hipErrorInvalidValue;
    float* part_b = part + (size_t)chunks * WG_TAPS * cout * cin;
    hipLaunchKernelGGL(conv_wgrad_f32_kernel, dim3(tci, tco, chunks), dim3(256), 0, s, dz, ldz, x, ldx, lengths, B, T, cin, cout, chunk, part);
    if (db) hipLaunchKernelGGL(wgrad_bias_kernel, dim3((cout + 63) / 64, chunks), dim3(256), 0, s, dz, ldz, lengths, B, T, cout, chunk, part_b);
    const size_t n = (size_t)cout * cin * WG_TAPS + (db ? cout : 0);
    hipLaunchKernelGGL(wgrad_reduce_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, part, part_b, chunks, cin, cout, dw, db);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------- projections and pool, backwards
// g = [g_enc | g_dur] per clip (2E outputs), pw [2E][C] the forward image's projection rows, pooled [B][C].
//   e <  2E C        : d pw[o][c] = sum_b g[b][o] pooled[b][c], batch order, written at the tensor's place in the flat buffer
//   then 2E          : d pb[o]    = sum_b g[b][o]
//   then B C         : d pooled[b][c] = sum_o g[b][o] pw[o][c], output order (enc rows, then dur rows)
__global__ void style_proj_bwd_kernel(const float* __restrict__ g_enc, const float* __restrict__ g_dur, const float* __restrict__ pooled,
                                      const float* __restrict__ pw, int B, int C, int E, float* __restrict__ d_we, float* __restrict__ d_be,
                                      float* __restrict__ d_wd, float* __restrict__ d_bd, float* __restrict__ d_pooled) {
    const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t nw = (size_t)2 * E * C;
    auto g = [&](int b, int o) { return o < E ? g_enc[(size_t)b * E + o] : g_dur[(size_t)b * E + o - E]; };
    if (e < nw) {
        const int o = (int)(e / C), c = (int)(e % C);
        float s = 0.f;
        for (int b = 0; b < B; ++b) s += g(b, o) * pooled[(size_t)b * C + c];
        if (o < E) d_we[(size_t)o * C + c] = s;
        else d_wd[(size_t)(o - E) * C + c] = s;
    } else if (e < nw + 2 * E) {
        const int o = (int)(e - nw);
        float s = 0.f;
        for (int b = 0; b < B; ++b) s += g(b, o);
        if (o < E) d_be[o] = s;
        else d_bd[o - E] = s;
    } else if (e < nw + 2 * E + (size_t)B * C) {
        const size_t i = e - nw - 2 * E;
        const int b = (int)(i / C), c = (int)(i % C);
        float s = 0.f;
        for (int o = 0; o < 2 * E; ++o) s += g(b, o) * pw[(size_t)o * C + c];
        d_pooled[i] = s;
    }
}
// d h[b][t][c] = d pooled[b][c] / max(len_b, 1) where t < len_b and the layer's ReLU output h is positive, else 0
__global__ void style_pool_bwd_kernel(const float* __restrict__ d_pooled, const float* __restrict__ h, const int64_t* __restrict__ lengths, int B,
                                      int T, int C, float* __restrict__ dh) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (size_t)B * T * C) return;
    const int c = (int)(i % C);
    const size_t row = i / C;
    const int b = (int)(row / T), t = (int)(row % T);
    const int n = wg_frames(lengths, b, T);
    const float inv_n = 1.0f / (float)(n > 1 ? n : 1);
    dh[i] = (t < n && h[i] > 0.f) ? d_pooled[(size_t)b * C + c] * inv_n : 0.f;
}
// g[b][t][c] stays where t < len_b and the ReLU output h[b][t][c] is positive, else becomes 0
__global__ void style_gate_kernel(float* __restrict__ g, const float* __restrict__ h, const int64_t* __restrict__ lengths, int B, int T, int C) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (size_t)B * T * C) return;
    const size_t row = i / C;
    const int b = (int)(row / T), t = (int)(row % T);
    if (!(t < wg_frames(lengths, b, T) && h[i] > 0.f)) g[i] = 0.f;
}

static hipError_t launch_style_proj_bwd(const float* g_enc, const float* g_dur, const float* pooled, const float* pw, int B, int C, int E, float* d_we,
                                        float* d_be, float* d_wd, float* d_bd, float* d_pooled, hipStream_t s) {
    const size_t n = (size_t)2 * E * C + 2 * E + (size_t)B * C;
    hipLaunchKernelGGL(style_proj_bwd_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, g_enc, g_dur, pooled, pw, B, C, E, d_we, d_be,
                       d_wd, d_bd, d_pooled);
    return hipGetLastError();
}
static hipError_t launch_style_pool_bwd(const float* d_pooled, const float* h, const int64_t* lengths, int B, int T, int C, float* dh, hipStream_t s) {
    const size_t n = (size_t)B * T * C;
    hipLaunchKernelGGL(style_pool_bwd_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, d_pooled, h, lengths, B, T, C, dh);
    return hipGetLastError();
}
static hipError_t launch_style_gate(float* g, const float* h, const int64_t* lengths, int B, int T, int C, hipStream_t s) {
    const size_t n = (size_t)B * T * C;
    hipLaunchKernelGGL(style_gate_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, g, h, lengths, B, T, C);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------- parameters, panels, plan (host)
struct StyleParam { std::string key; size_t off, numel; };
// The flat parameter buffer in the reference's state-dict order
static std::vector<StyleParam> style_params(const mtts_style* v) {
    std::vector<StyleParam> p;
    size_t off = 0;
    auto add = [&](const std::string& key, size_t n) { p.push_back({key, off, n}); off += n; };
    int cin = v->n_feats;
    for (int i = 0; i < v->layers; ++i) {
        add("convs." + std::to_string(i) + ".weight", (size_t)v->hidden * cin * WG_TAPS);
        add("convs." + std::to_string(i) + ".bias", v->hidden);
        cin = v->hidden;
    }
    for (const char* h : {"proj_enc", "proj_dur"}) {
        add(std::string(h) + ".weight", (size_t)v->emb * v->hidden);
        add(std::string(h) + ".bias", v->emb);
    }
    return p;
}

static int pack_style_grad(mtts_style* v) {
    Component& G = v->grad;
    G.image.clear();
    G.gemm_terms = 0;             // native fp32 MFMA for the backward GEMMs (file header)
    G.packed = false;
    G.uploaded = false;
    Packer P(&G);
    v->gradw = StyleGradW();
    (void)P.alloc(64);            // never empty: a one-layer encoder has no panel, and the buffer is still the proof of an upload
    for (int i = 0; i < v->layers && P.ok; ++i) {
        if (i == 0) { v->gradw.convT.push_back(Panel()); continue; }
        const std::string key = "convs." + std::to_string(i) + ".weight";
        const size_t numel = (size_t)v->hidden * v->hidden * WG_TAPS;
        auto it = v->raw.find(key);
        if (it == v->raw.end()) { P.fail("missing tensor " + key); break; }
        if (it->second.size() != numel) { P.fail("tensor " + key + " has an unexpected size"); break; }
        // w [N][C][k] -> [C][N][k] with the taps reversed: the data gradient is the same centred-tap GEMM with in / out swapped
        const int N = v->hidden, Cc = v->hidden;
        std::vector<float> t(numel);
        for (int n = 0; n < N; ++n)
            for (int c = 0; c < Cc; ++c)
                for (int j = 0; j < WG_TAPS; ++j) t[((size_t)c * N + n) * WG_TAPS + j] = it->second[((size_t)n * Cc + c) * WG_TAPS + (WG_TAPS - 1 - j)];
        v->gradw.convT.push_back(P.panel_from(t.data(), nullptr, 1, Cc, N, WG_TAPS));
    }
    if (!P.ok) { set_error("mtts_style_grad weights: " + P.why); return -1; }
    G.packed = true;
    return 0;
}

struct StyleGradBufs {
    float *X, *MASK, *H[64], *POOLED, *DP, *GA, *GB, *PART;
    size_t off_x = 0, off_mask = 0, off_h[64] = {}, off_pooled = 0;
};
static void style_grad_plan(const mtts_style* v, int B, int T, WS& ws, StyleGradBufs& b) {
    const size_t M = (size_t)B * T;
    const int ldx = round_up(v->n_feats, 4);
    b.X = ws.f(M * ldx); b.off_x = ws.off - M * ldx * sizeof(float);
    b.MASK = ws.f(M); b.off_mask = ws.off - M * sizeof(float);
    for (int l = 0; l < v->layers; ++l) { b.H[l] = ws.f(M * v->hidden); b.off_h[l] = ws.off - M * v->hidden * sizeof(float); }
    b.POOLED = ws.f((size_t)B * v->hidden); b.off_pooled = ws.off - (size_t)B * v->hidden * sizeof(float);
    b.DP = ws.f((size_t)B * v->hidden);
    b.GA = ws.f(M * v->hidden);
    b.GB = ws.f(M * v->hidden);
    b.PART = ws.f(conv_wgrad_partial_floats((int64_t)M, std::max(v->n_feats, v->hidden), v->hidden));
}
static bool style_grad_shape_ok(const char* who, const mtts_style* v, int B, int T) {
    if (!v) { set_error(std::string(who) + ": null context"); return false; }
    if (B < 1 || B > 65535 || T < 1 || (int64_t)B * T > (int64_t)1 << 30) { set_error(std::string(who) + ": bad shape (B in [1, 65535], T >= 1, B * T <= 2^30)"); return false; }
    return true;
}

}  // namespace mtts

using namespace mtts;

extern "C" {

int64_t mtts_style_param_count(mtts_style* v) {
    if (!v) { set_error("mtts_style_param_count: null context"); return -1; }
    const std::vector<StyleParam> p = style_params(v);
    return (int64_t)(p.back().off + p.back().numel);
}
int64_t mtts_style_param_offset(mtts_style* v, const char* key) {
    if (!v || !key) { set_error("mtts_style_param_offset: null argument"); return -1; }
    for (const StyleParam& p : style_params(v))
        if (p.key == key) return (int64_t)p.off;
    set_error(std::string("mtts_style_param_offset: no parameter named ") + key);
    return -1;
}

int64_t mtts_style_grad_weights_bytes(mtts_style* v) {
    if (!v) { set_error("mtts_style_grad_weights_bytes: null context"); return -1; }
    if (!v->grad.packed && pack_style_grad(v)) return -1;
    return (int64_t)(v->grad.image.size() * sizeof(float));
}
int mtts_style_grad_upload_weights(mtts_style* v, void* d_buf, int64_t bytes) {
    if (!v || !d_buf) { set_error("mtts_style_grad_upload_weights: null argument"); return -1; }
    if (!v->grad.packed && pack_style_grad(v)) return -1;
    Component& G = v->grad;
    if ((size_t)bytes < G.image.size() * sizeof(float)) { set_error("mtts_style_grad_upload_weights: buffer too small (mtts_style_grad_weights_bytes)"); return -1; }
    HIP_OK(hipMemcpy(d_buf, G.image.data(), G.image.size() * sizeof(float), hipMemcpyHostToDevice));
    G.d_image = static_cast<float*>(d_buf);
    G.uploaded = true;
    return 0;
}

int64_t mtts_style_grad_workspace_bytes(mtts_style* v, int B, int T) {
    if (!style_grad_shape_ok("mtts_style_grad_workspace_bytes", v, B, T)) return -1;
    WS ws(nullptr, 0);
    StyleGradBufs b;
    style_grad_plan(v, B, T, ws, b);
    return (int64_t)ws.off + 256;
}
// Byte offset inside the workspace of what the taped forward left: which 0 the masked input rows [B T][round_up(n_feats, 4)], 1 ..
// n_layers the ReLU output of layer which - 1 [B T][hidden], n_layers + 1 the pooled rows [B][hidden], n_layers + 2 the prefix mask [B T].
int64_t mtts_style_grad_tape_offset(mtts_style* v, int B, int T, int which) {
    if (!style_grad_shape_ok("mtts_style_grad_tape_offset", v, B, T)) return -1;
    if (which < 0 || which > v->layers + 2) { set_error("mtts_style_grad_tape_offset: which must be in [0, n_layers + 2]"); return -1; }
    WS ws(nullptr, 0);
    StyleGradBufs b;
    style_grad_plan(v, B, T, ws, b);
    if (which == 0) return (int64_t)b.off_x;
    if (which <= v->layers) return (int64_t)b.off_h[which - 1];
    return (int64_t)(which == v->layers + 1 ? b.off_pooled : b.off_mask);
}

// mtts_style_forward with group == NULL, every layer's output kept: the same launchers with the same arguments, so the rows are that
// entry's bit for bit.
int mtts_style_forward_taped(mtts_style* v, const float* d_mel, const int64_t* d_mel_lengths, int B, int T, float* d_e_enc, float* d_e_dur,
                             void* d_ws, int64_t ws_bytes, void* stream) {
    if (!style_grad_shape_ok("mtts_style_forward_taped", v, B, T)) return -1;
    if (!d_mel || !d_mel_lengths || !d_e_enc || !d_e_dur || !d_ws) { set_error("mtts_style_forward_taped: null argument"); return -1; }
    Component* c = v;
    hipStream_t s = static_cast<hipStream_t>(stream);
    WS ws(d_ws, (size_t)ws_bytes);
    StyleGradBufs b;
    style_grad_plan(v, B, T, ws, b);
    if (ws.overflow || ws_bytes < (int64_t)ws.off) { set_error("mtts_style_forward_taped: workspace too small (mtts_style_grad_workspace_bytes)"); return -1; }
    RET_IF(check_ready(c));
    const int ldx = round_up(v->n_feats, 4);
    LAUNCH(c, 2, 0, s, launch_style_prep(d_mel, d_mel_lengths, B, v->n_feats, T, b.X, ldx, b.MASK, s));
    const float* in = b.X;
    int ldin = ldx, cin = v->n_feats;
    for (int i = 0; i < v->layers; ++i) {
        GemmArgs a;
        panel_args(c, v->w.convs[i], a); rows_plain(a, B, T); taps_centered(a, WG_TAPS);
        a.a0 = in; a.lda0 = ldin; a.c0 = cin; a.act = ACT_RELU; a.out_mask = b.MASK; a.out = b.H[i]; a.ldc = v->hidden;
        RET_IF(run_gemm(c, a, s));
        in = b.H[i]; ldin = v->hidden; cin = v->hidden;
    }
    LAUNCH(c, 2, 0, s, launch_style_pool_proj(in, d_mel_lengths, B, T, v->hidden, v->emb, W(c, v->w.proj_w.off), W(c, v->w.proj_b.off),
                                              nullptr, B, d_e_enc, d_e_dur, s, b.POOLED));
    return 0;
}

// Parameter gradients from the tape of the latest mtts_style_forward_taped call in d_ws (same B, T and lengths) and the upstream
// d_g_enc, d_g_dur [B][E]: d_param_grad [mtts_style_param_count] floats, every element written.
int mtts_style_backward(mtts_style* v, const int64_t* d_mel_lengths, int B, int T, const float* d_g_enc, const float* d_g_dur,
                        float* d_param_grad, void* d_grad_buf, void* d_ws, int64_t ws_bytes, void* stream) {
    if (!style_grad_shape_ok("mtts_style_backward", v, B, T)) return -1;
    if (!d_mel_lengths || !d_g_enc || !d_g_dur || !d_param_grad || !d_grad_buf || !d_ws) { set_error("mtts_style_backward: null argument"); return -1; }
    Component* c = v;
    hipStream_t s = static_cast<hipStream_t>(stream);
    WS ws(d_ws, (size_t)ws_bytes);
    StyleGradBufs b;
    style_grad_plan(v, B, T, ws, b);
    if (ws.overflow || ws_bytes < (int64_t)ws.off) { set_error("mtts_style_backward: workspace too small (mtts_style_grad_workspace_bytes)"); return -1; }
    if (!v->grad.packed || !v->grad.uploaded || v->grad.d_image != d_grad_buf) {
        set_error("mtts_style_backward: backward panels not uploaded (mtts_style_grad_upload_weights into d_grad_buf)");
        return -1;
    }
    RET_IF(check_ready(c));
    const std::vector<StyleParam> P = style_params(v);
    const int L = v->layers, Hc = v->hidden, E = v->emb, ldx = round_up(v->n_feats, 4);
    float* pe = d_param_grad + P[2 * L].off;
    LAUNCH(c, 2, 0, s, launch_style_proj_bwd(d_g_enc, d_g_dur, b.POOLED, W(c, v->w.proj_w.off), B, Hc, E, pe, d_param_grad + P[2 * L + 1].off,
                                             d_param_grad + P[2 * L + 2].off, d_param_grad + P[2 * L + 3].off, b.DP, s));
    LAUNCH(c, 2, 0, s, launch_style_pool_bwd(b.DP, b.H[L - 1], d_mel_lengths, B, T, Hc, b.GA, s));
    float* gz = b.GA;             // d loss / d (pre-ReLU output of layer l), gated and masked
    float* gn = b.GB;
    for (int l = L - 1; l >= 0; --l) {
        const float* in = l ? b.H[l - 1] : b.X;
        const int cin = l ? Hc : v->n_feats, ldin = l ? Hc : ldx;
        LAUNCHB(c, 0, conv_wgrad_flops(B, T, cin, Hc), 0.0, s,
                launch_conv_wgrad(gz, Hc, in, ldin, d_mel_lengths, B, T, cin, Hc, d_param_grad + P[2 * l].off, d_param_grad + P[2 * l + 1].off,
                                  b.PART, s));
        if (l == 0) break;
        GemmArgs a;
        panel_args(&v->grad, v->gradw.convT[l], a); rows_plain(a, B, T); taps_centered(a, WG_TAPS);
        a.a0 = gz; a.lda0 = Hc; a.c0 = Hc; a.out = gn; a.ldc = Hc;
        RET_IF(run_gemm(c, a, s));
        LAUNCH(c, 2, 0, s, launch_style_gate(gn, b.H[l - 1], d_mel_lengths, B, T, Hc, s));
        std::swap(gz, gn);
    }
    return 0;
}

// ---------------------------------------------------------------------------------------------- unit entry (kernel-level parity)
int mtts_conv_wgrad_chunk_rows(int B, int T) {
    if (B < 1 || T < 1 || (int64_t)B * T > (int64_t)1 << 30) { set_error("mtts_conv_wgrad_chunk_rows: bad shape"); return -1; }
    return conv_wgrad_chunk_rows((int64_t)B * T);
}
int64_t mtts_conv_wgrad_workspace_bytes(int B, int T, int cin, int cout) {
    if (B < 1 || T < 1 || cin < 1 || cout < 1 || (int64_t)B * T > (int64_t)1 << 30) { set_error("mtts_conv_wgrad_workspace_bytes: bad shape"); return -1; }
    return (int64_t)(conv_wgrad_partial_floats((int64_t)B * T, cin, cout) * sizeof(float));
}
// d_dz [B*T][cout], d_x [B*T][ldx] (ldx >= cin), d_lengths int64 [B] or NULL (every clip has T frames) -> d_dw [cout][cin][5],
// d_db [cout] or NULL.  The partial results are left in d_ws: [chunks][5][cout][cin] then [chunks][cout].
int mtts_conv_wgrad(const float* d_dz, const float* d_x, const int64_t* d_lengths, int B, int T, int cin, int ldx, int cout, float* d_dw,
                    float* d_db, void* d_ws, int64_t ws_bytes, void* stream) {
    if (!d_dz || !d_x || !d_dw || !d_ws) { set_error("mtts_conv_wgrad: null argument"); return -1; }
    if (B < 1 || T < 1 || cin < 1 || cout < 1 || ldx < cin || (int64_t)B * T > (int64_t)1 << 30) { set_error("mtts_conv_wgrad: bad shape"); return -1; }
    if (ws_bytes < mtts_conv_wgrad_workspace_bytes(B, T, cin, cout)) { set_error("mtts_conv_wgrad: workspace too small (mtts_conv_wgrad_workspace_bytes)"); return -1; }
    HIP_OK(launch_conv_wgrad(d_dz, cout, d_x, ldx, d_lengths, B, T, cin, cout, d_dw, d_db, static_cast<float*>(d_ws),
                             static_cast<hipStream_t>(stream)));
    return 0;
}

}  // extern "C"
