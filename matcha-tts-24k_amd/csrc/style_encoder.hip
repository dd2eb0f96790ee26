// Kernels of the style encoder's forward pass that are not GEMMs (gfx950): reference matcha/models/style_encoder.py:36-72
// (StyleEncoder.forward, masked_mean_pool) and the clip average of matcha/add_speaker.py:60-62.  The Conv1d(k5) + ReLU stack
// runs on gemm_f32_kernel (five taps, ReLU and the prefix mask in its epilogue); the launch sequence is behind the kernels
// (mtts_style_forward).
#include "host.h"

namespace mtts {

// Frames of clip b that exist: lengths[b] held inside [0, T], so no index derived from it leaves the buffers.
__device__ __forceinline__ int style_frames(const int64_t* __restrict__ lengths, int b, int T) {
    const int64_t n = lengths[b];
    return n < 0 ? 0 : (n > (int64_t)T ? T : (int)n);
}

// mel [B, C, T] -> rows x [B*T][ld] (channels [C, ld) zero) times the prefix mask (style_encoder.py:69 `x * mel_mask`; frames at
// t >= lengths[b] are written as zero and their source is not read), and the mask itself as floats [B*T] for the convs' epilogues.
__global__ __launch_bounds__(256) void style_prep_kernel(const float* __restrict__ mel, const int64_t* __restrict__ lengths, int C, int T,
                                                         float* __restrict__ x, int ld, float* __restrict__ mask) {
    __shared__ float tl[32][33];
    const int b = blockIdx.z, t0 = blockIdx.x * 32, c0 = blockIdx.y * 32;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const int n = style_frames(lengths, b, T);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int c = c0 + ty + 8 * i, t = t0 + tx;
        tl[ty + 8 * i][tx] = (c < C && t < n) ? mel[((size_t)b * C + c) * T + t] : 0.f;
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int t = t0 + ty + 8 * i, c = c0 + tx;
        if (t < T && c < ld) x[((size_t)b * T + t) * ld + c] = tl[tx][ty + 8 * i];
    }
    if (blockIdx.y == 0 && ty == 0 && t0 + tx < T) mask[(size_t)b * T + t0 + tx] = (t0 + tx < n) ? 1.f : 0.f;
}
hipError_t launch_style_prep(const float* mel, const int64_t* lengths, int B, int C, int T, float* x, int ld, float* mask, hipStream_t s) {
    if (!mel || !lengths || !x || !mask || B <= 0 || B > 65535 || C <= 0 || T <= 0 || ld < C) return hipErrorInvalidValue;
    hipLaunchKernelGGL(style_prep_kernel, dim3((T + 31) / 32, (ld + 31) / 32, B), dim3(256), 0, s, mel, lengths, C, T, x, ld, mask);
    return hipGetLastError();
}

// Masked mean over time, both projections and the clip average, one workgroup per output row.
//   pooled_b[c] = sum_{t < len_b} h[b, t, c] / max(len_b, 1)                  (style_encoder.py:36-39; rows at t >= len_b are not read)
//   row_b       = [proj_enc | proj_dur](pooled_b)                             (style_encoder.py:72)
//   out_g       = mean of row_b over the clips with group[b] == g             (add_speaker.py:60-62);  group == null: out_b = row_b
// 1024 threads = 4 time slices x 256 channels; slice s adds frames s, s + 4, ... in order and the four partial sums are combined
// in a fixed order, the projections' dot products go lane-strided with a butterfly, a group's clips are added in batch order:
// every sum has one order, so two runs and any batch give the same bits for a clip.
__global__ __launch_bounds__(1024) void style_pool_proj_kernel(const float* __restrict__ h, const int64_t* __restrict__ lengths, int B, int T,
                                                               int C, int E, const float* __restrict__ pw, const float* __restrict__ pb,
                                                               const int* __restrict__ group, float* __restrict__ e_enc,
                                                               float* __restrict__ e_dur, float* __restrict__ pooled_out) {
    extern __shared__ float sm[];          // part [4][C] | pooled [C] | acc [2E]
    float* part = sm;
    float* pooled = sm + 4 * C;
    float* acc = pooled + C;
    const int g = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int o = tid; o < 2 * E; o += 1024) acc[o] = 0.f;
    int count = 0;
    for (int b = group ? 0 : g; b < (group ? B : g + 1); ++b) {
        if (group && group[b] != g) continue;       // uniform over the workgroup
        const int n = style_frames(lengths, b, T);
        const float* hb = h + (size_t)b * T * C;
        const int slice = tid >> 8;
        for (int c = tid & 255; c < C; c += 256) {
            float s = 0.f;
            for (int t = slice; t < n; t += 4) s += hb[(size_t)t * C + c];
            part[slice * C + c] = s;
        }
        __syncthreads();
        const float inv_n = 1.0f / (float)(n > 1 ? n : 1);
        for (int c = tid; c < C; c += 1024) pooled[c] = (((part[c] + part[C + c]) + part[2 * C + c]) + part[3 * C + c]) * inv_n;
        __syncthreads();
        if (pooled_out)                             // the taped forward (style_grad.hip) keeps the rows the projections read
            for (int c = tid; c < C; c += 1024) pooled_out[(size_t)b * C + c] = pooled[c];
        for (int o = wave; o < 2 * E; o += 16) {
            float s = 0.f;
            for (int k = lane; k < C; k += 64) s += pooled[k] * pw[(size_t)o * C + k];
#pragma unroll
            for (int d = 32; d > 0; d >>= 1) s += __shfl_xor(s, d);
            if (lane == 0) acc[o] += s + pb[o];
        }
        __syncthreads();
        ++count;
    }
    const float inv = (group && count > 1) ? 1.0f / (float)count : 1.0f;
    for (int o = tid; o < 2 * E; o += 1024) {
        const float v = group ? acc[o] * inv : acc[o];
        if (o < E) e_enc[(size_t)g * E + o] = v;
        else e_dur[(size_t)g * E + o - E] = v;
    }
}
hipError_t launch_style_pool_proj(const float* h, const int64_t* lengths, int B, int T, int C, int E, const float* pw, const float* pb,
                                  const int* group, int n_out, float* e_enc, float* e_dur, hipStream_t s, float* pooled_out) {
    if (!h || !lengths || !pw || !pb || !e_enc || !e_dur || B <= 0 || T <= 0 || C <= 0 || E <= 0 || n_out <= 0) return hipErrorInvalidValue;
    if (!group && n_out != B) return hipErrorInvalidValue;
    const size_t lds = (size_t)(5 * C + 2 * E) * sizeof(float);
    if (lds > 48 * 1024) return hipErrorInvalidValue;
    hipLaunchKernelGGL(style_pool_proj_kernel, dim3(n_out), dim3(1024), lds, s, h, lengths, B, T, C, E, pw, pb, group, e_enc, e_dur, pooled_out);
    return hipGetLastError();
}

}  // namespace mtts

using namespace mtts;

// ================================================================================================ style encoder
// StyleEncoder (reference matcha/models/style_encoder.py:42-72): n_layers x { x * mask -> Conv1d(k5, pad 2) -> ReLU }, masked mean
// over time, Linear(hidden -> spk_emb_dim) twice.  Tensors are registered under the reference's names ("convs.0.weight", ...,
// "proj_enc.weight", "proj_dur.bias").
static int style_pack(mtts_style* v) {
    Component* c = v;
    c->image.clear();
    Packer P(c);
    StyleW& W = v->w;
    W = StyleW();
    int cin = v->n_feats;
    for (int i = 0; i < v->layers; ++i) {
        const std::string p = "convs." + std::to_string(i) + ".";
        W.convs.push_back(P.panel(p + "weight", p + "bias", 1, v->hidden, cin, 5));
        cin = v->hidden;
    }
    const auto* we = P.get("proj_enc.weight", (size_t)v->emb * v->hidden);
    const auto* be = P.get("proj_enc.bias", v->emb);
    const auto* wd = P.get("proj_dur.weight", (size_t)v->emb * v->hidden);
    const auto* bd = P.get("proj_dur.bias", v->emb);
    if (we && be && wd && bd) {
        const size_t n = (size_t)v->emb * v->hidden;
        W.proj_w.off = P.alloc(2 * n); W.proj_w.n = (int)(2 * n);
        W.proj_b.off = P.alloc(2 * v->emb); W.proj_b.n = 2 * v->emb;
        std::memcpy(&c->image[W.proj_w.off], we->data(), n * sizeof(float));
        std::memcpy(&c->image[W.proj_w.off + n], wd->data(), n * sizeof(float));
        std::memcpy(&c->image[W.proj_b.off], be->data(), v->emb * sizeof(float));
        std::memcpy(&c->image[W.proj_b.off + v->emb], bd->data(), v->emb * sizeof(float));
    }
    if (!P.ok) { set_error(P.why); return -1; }
    c->packed = true;
    return 0;
}

struct StyleBufs { float *X, *MASK, *H0, *H1; };
static void style_plan(const mtts_style* v, int B, int T, WS& ws, StyleBufs& b) {
    const size_t M = (size_t)B * T;
    b.X = ws.f(M * round_up(v->n_feats, 4));
    b.MASK = ws.f(M);
    b.H0 = ws.f(M * v->hidden);
    b.H1 = ws.f(M * v->hidden);
}

extern "C" {

mtts_style* mtts_style_create(int n_feats, int hidden, int n_layers, int spk_emb_dim) {
    if (n_feats <= 0 || (n_feats & 3) || hidden <= 0 || (hidden & 3) || n_layers < 1 || n_layers > 64 || spk_emb_dim <= 0 ||
        (size_t)(5 * hidden + 2 * spk_emb_dim) * sizeof(float) > 48 * 1024) {
        set_error("mtts_style_create: unsupported shape (n_feats and hidden multiples of 4, 1..64 layers, 5 * hidden + 2 * spk_emb_dim <= 12288)");
        return nullptr;
    }
    mtts_style* v = new mtts_style();
    v->gemm_terms = read_switches().gemm_terms;
    v->n_feats = n_feats; v->hidden = hidden; v->layers = n_layers; v->emb = spk_emb_dim;
    return v;
}
void mtts_style_destroy(mtts_style* v) { delete v; }
int mtts_style_set_tensor(mtts_style* v, const char* key, const float* h, int64_t numel) {
    if (!v) { set_error("null context"); return -1; }
    v->grad.packed = false;             // the backward panels (style_grad.hip) are copies of these tensors
    v->grad.uploaded = false;
    return set_tensor(v, key, h, numel);
}
int64_t mtts_style_weights_bytes(mtts_style* v) { return weights_bytes(v, style_pack); }
int mtts_style_upload_weights(mtts_style* v, void* d_weights, int64_t bytes) {
    return upload_weights(v, style_pack, "mtts_style_upload_weights", d_weights, bytes);
}
int64_t mtts_style_workspace_bytes(mtts_style* v, int B, int T) {
    if (!v) { set_error("null context"); return -1; }
    if (B <= 0 || T <= 0) { set_error("mtts_style_workspace_bytes: bad shape"); return -1; }
    WS ws(nullptr, 0);
    StyleBufs b;
    style_plan(v, B, T, ws, b);
    return (int64_t)ws.off + 256;
}
// StyleEncoder.forward on a ragged batch + the clip average: n_layers + 2 launches (mask and transpose, the convs, pool and project).
int mtts_style_forward(mtts_style* v, const float* d_mel, const int64_t* d_mel_lengths, int B, int T, const int32_t* d_group, int n_groups,
                       float* d_e_enc, float* d_e_dur, void* d_ws, int64_t ws_bytes, void* stream) {
    if (!v) { set_error("null context"); return -1; }
    Component* c = v;
    RET_IF(check_ready(c));
    if (!d_mel || !d_mel_lengths || !d_e_enc || !d_e_dur || !d_ws || B <= 0 || B > 65535 || T <= 0 || (int64_t)B * T > (int64_t)1 << 30 ||
        (d_group && n_groups <= 0)) {
        set_error("mtts_style_forward: bad argument");
        return -1;
    }
    hipStream_t s = static_cast<hipStream_t>(stream);
    WS ws(d_ws, (size_t)ws_bytes);
    StyleBufs b;
    style_plan(v, B, T, ws, b);
    if (ws.overflow) { set_error("mtts_style_forward: workspace too small"); return -1; }
    const int ldx = round_up(v->n_feats, 4);
    LAUNCH(c, 2, 0, s, launch_style_prep(d_mel, d_mel_lengths, B, v->n_feats, T, b.X, ldx, b.MASK, s));
    const float* in = b.X;
    int ldin = ldx, cin = v->n_feats;
    float* out = b.H0;
    for (int i = 0; i < v->layers; ++i) {       // relu(conv(x * mask)); the mask of the NEXT layer's input is this epilogue's out_mask
        GemmArgs a;
        panel_args(c, v->w.convs[i], a); rows_plain(a, B, T); taps_centered(a, 5);
        a.a0 = in; a.lda0 = ldin; a.c0 = cin; a.act = ACT_RELU; a.out_mask = b.MASK; a.out = out; a.ldc = v->hidden;
        RET_IF(run_gemm(c, a, s));
        in = out; ldin = v->hidden; cin = v->hidden;
        out = (out == b.H0) ? b.H1 : b.H0;
    }
    LAUNCH(c, 2, 0, s, launch_style_pool_proj(in, d_mel_lengths, B, T, v->hidden, v->emb, W(c, v->w.proj_w.off), W(c, v->w.proj_b.off),
                                              d_group, d_group ? n_groups : B, d_e_enc, d_e_dur, s));
    return 0;
}

}  // extern "C"
