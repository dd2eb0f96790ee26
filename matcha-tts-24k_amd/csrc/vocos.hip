// Kernels of the Vocos-24k head that are not GEMMs (gfx950): depthwise k7 conv + LayerNorm, polar spectrum, iSTFT
// overlap-add.  The dense parts (embed conv k7, pwconv1/2, head projection, inverse real DFT as a [n_fft x (n_fft+2)]
// matrix) run on gemm_f32_kernel.  Architecture: reference matcha/vocos24k/config.yaml:10-24 + the vocos package
// (VocosBackbone / ConvNeXtBlock / ISTFTHead); call site reference matcha/vocos24k/vocos_wrapper.py:8-9.
// Behind the kernels: the head's weight packing, workspace plan, launch sequence and C ABI (mtts_vocos_*).
#include "host.h"
#include "device_utils.h"

namespace mtts {

using f32x4 = __attribute__((ext_vector_type(4))) float;
constexpr int DW_MAXV = 8;   // float4 per lane => C <= 2048

__device__ __forceinline__ float wave_sum_v(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// Frames of utterance b that a ragged call treats as present: lengths[b] held inside [0, T], so that no index derived from it
// leaves the buffers whatever the caller passed (vocos_lengths_check_kernel reports the bad value).
__device__ __forceinline__ int frames_of(const int64_t* __restrict__ lengths, int b, int T) {
    const int64_t n = lengths[b];
    return n < 0 ? 0 : (n > (int64_t)T ? T : (int)n);
}

// ConvNeXtBlock front: dwconv(k7, pad 3, groups=C) -> LayerNorm(eps).  One wave per output row; the 7 input rows are
// neighbours' rows too (L1/L2 hits).  HBM-bound: reads and writes the tensor once.
// RAGGED: utterance b ends at lengths[b] frames: a tap at tt >= lengths[b] is the conv's zero padding whatever the buffer holds
// there (after the first block those rows carry residual-stream values, so the decision is the length's, not the data's).
template <bool RAGGED>
__global__ __launch_bounds__(256) void dwconv7_ln_kernel(const float* __restrict__ x, const float* __restrict__ w7,
                                                         const float* __restrict__ bias, const float* __restrict__ gamma,
                                                         const float* __restrict__ beta, float eps, int T, int C, int M,
                                                         const int64_t* __restrict__ lengths, float* __restrict__ y) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (row >= M) return;
    const int t = row % T;
    const int t_end = RAGGED ? frames_of(lengths, row / T, T) : T;
    f32x4 v[DW_MAXV];
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < DW_MAXV; ++i) {
        const int c = (lane + 64 * i) * 4;
        v[i] = (f32x4){0.f, 0.f, 0.f, 0.f};
        if (c < C) {
            f32x4 acc = *reinterpret_cast<const f32x4*>(bias + c);
#pragma unroll
            for (int j = 0; j < 7; ++j) {
                const int tt = t + j - 3;
                if (tt >= 0 && tt < t_end) {
                    const f32x4 xv = *reinterpret_cast<const f32x4*>(x + (size_t)(row + j - 3) * C + c);
                    acc += xv * *reinterpret_cast<const f32x4*>(w7 + (size_t)j * C + c);
                }
            }
            v[i] = acc;
            s += (acc[0] + acc[1]) + (acc[2] + acc[3]);
        }
    }
    const float mu = wave_sum_v(s) / (float)C;
    float q = 0.f;
#pragma unroll
    for (int i = 0; i < DW_MAXV; ++i) {
        const int c = (lane + 64 * i) * 4;
        if (c < C) {
            const f32x4 d = v[i] - mu;
            q += (d[0] * d[0] + d[1] * d[1]) + (d[2] * d[2] + d[3] * d[3]);
        }
    }
    const float rs = 1.0f / sqrtf(wave_sum_v(q) / (float)C + eps);
#pragma unroll
    for (int i = 0; i < DW_MAXV; ++i) {
        const int c = (lane + 64 * i) * 4;
        if (c < C) {
            const f32x4 g = *reinterpret_cast<const f32x4*>(gamma + c);
            const f32x4 b = *reinterpret_cast<const f32x4*>(beta + c);
            *reinterpret_cast<f32x4*>(y + (size_t)row * C + c) = ((v[i] - mu) * rs) * g + b;
        }
    }
}

hipError_t launch_dwconv7_ln(const float* x, const float* w7, const float* bias, const float* gamma, const float* beta, float eps,
                             int B, int T, int C, float* y, hipStream_t s, const int64_t* lengths) {
    if (!x || !w7 || !bias || !gamma || !beta || !y || B <= 0 || T <= 0 || C <= 0 || (C & 3) || C > 64 * 4 * DW_MAXV) return hipErrorInvalidValue;
    const int M = B * T;
    if (lengths)
        hipLaunchKernelGGL(dwconv7_ln_kernel<true>, dim3((M + 3) / 4), dim3(256), 0, s, x, w7, bias, gamma, beta, eps, T, C, M, lengths, y);
    else
        hipLaunchKernelGGL(dwconv7_ln_kernel<false>, dim3((M + 3) / 4), dim3(256), 0, s, x, w7, bias, gamma, beta, eps, T, C, M, lengths, y);
    return hipGetLastError();
}

// ISTFTHead: mag = clip(exp(m), max), S = mag * (cos p + i sin p)
__global__ void spec_polar_kernel(float* __restrict__ x, int M, int ld, int nbins, int off, float clip) {
    const size_t n = (size_t)M * nbins;
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const size_t r = i / nbins, k = i % nbins;
        float* row = x + r * ld;
        const float mag = fminf(expf(row[k]), clip);
        const float p = row[off + k];
        row[k] = mag * cosf(p);
        row[off + k] = mag * sinf(p);
    }
}
hipError_t launch_spec_polar(float* x, int M, int ld, int nbins, int off, float clip, hipStream_t s) {
    if (!x || M <= 0 || nbins <= 0 || off < nbins || off + nbins > ld) return hipErrorInvalidValue;
    const size_t n = (size_t)M * nbins;
    hipLaunchKernelGGL(spec_polar_kernel, dim3((unsigned)min((n + 255) / 256, (size_t)4096)), dim3(256), 0, s, x, M, ld, nbins, off, clip);
    return hipGetLastError();
}

// torch.istft(center=True) tail: y[pos] = sum_f frame_f[pos - f*hop] / sum_f window^2[pos - f*hop], pos = s + n_fft/2,
// output sample s in [0, hop*(T-1)).  (The frames already carry one window factor from the DFT matrix.)
// RAGGED: utterance b has lengths[b] frames of its own: its last frame is lengths[b] - 1 (the envelope is built from its own
// frames only), it has hop * (lengths[b] - 1) samples, and the rest of its row is written as zero.
template <bool RAGGED>
__global__ void istft_ola_kernel(const float* __restrict__ frames, const float* __restrict__ window, int T, int n_fft, int hop,
                                 const int64_t* __restrict__ lengths, float* __restrict__ audio) {
    const int b = blockIdx.y;
    const int L = hop * (T - 1);
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= L) return;
    const int Tb = RAGGED ? frames_of(lengths, b, T) : T;
    if (RAGGED && s >= hop * (Tb - 1)) {
        audio[(size_t)b * L + s] = 0.f;
        return;
    }
    const int pos = s + n_fft / 2;
    int f0 = (pos - n_fft + hop) / hop;     // ceil((pos - n_fft + 1) / hop) for pos - n_fft + 1 > 0
    if (pos - n_fft + 1 <= 0) f0 = 0;
    int f1 = pos / hop;
    if (f1 > Tb - 1) f1 = Tb - 1;
    float acc = 0.f, env = 0.f;
    for (int f = f0; f <= f1; ++f) {
        const int j = pos - f * hop;
        const float w = window[j];
        acc += frames[((size_t)b * T + f) * n_fft + j];
        env += w * w;
    }
    audio[(size_t)b * L + s] = env > 1e-11f ? acc / env : acc;
}
hipError_t launch_istft_ola(const float* frames, const float* window, int B, int T, int n_fft, int hop, float* audio, hipStream_t s,
                            const int64_t* lengths) {
    if (!frames || !window || !audio || B <= 0 || T < 2 || n_fft <= 0 || hop <= 0 || n_fft % hop) return hipErrorInvalidValue;
    const int L = hop * (T - 1);
    if (lengths)
        hipLaunchKernelGGL(istft_ola_kernel<true>, dim3((L + 255) / 256, B), dim3(256), 0, s, frames, window, T, n_fft, hop, lengths, audio);
    else
        hipLaunchKernelGGL(istft_ola_kernel<false>, dim3((L + 255) / 256, B), dim3(256), 0, s, frames, window, T, n_fft, hop, lengths, audio);
    return hipGetLastError();
}

// Validation of a ragged call's lengths where they live: status[0] = 1 + the first row whose length is outside [1, T] (0: all
// good), status[1] = that length (saturated to int32), status[2] = T.  One workgroup, ahead of the decode.
__global__ __launch_bounds__(256) void vocos_lengths_check_kernel(const int64_t* __restrict__ lengths, int B, int T, int* __restrict__ status) {
    const int i = first_refused_row(B, [&](int b) { const int64_t n = lengths[b]; return n < 1 || n > (int64_t)T; });
    if (threadIdx.x == 0) {
        status[0] = i < B ? i + 1 : 0;
        status[1] = i < B ? sat32(lengths[i]) : 0;
        status[2] = T;
    }
}
hipError_t launch_vocos_lengths_check(const int64_t* lengths, int B, int T, int* status, hipStream_t s) {
    if (!lengths || !status || B <= 0 || T <= 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(vocos_lengths_check_kernel, dim3(1), dim3(256), 0, s, lengths, B, T, status);
    return hipGetLastError();
}

}  // namespace mtts

using namespace mtts;

// ================================================================================================ Vocos head
static int vocos_pack(mtts_vocos* v) {
    Component* c = v;
    c->image.clear();
    Packer P(c);
    VocosW& W = v->w;
    W = VocosW();
    const int C = v->dim, nb = v->n_fft / 2 + 1;
    auto S = [](const std::string& a, int i, const std::string& b) { return a + std::to_string(i) + b; };
    W.embed = P.panel("backbone.embed.weight", "backbone.embed.bias", 1, C, v->n_mels, 7);
    W.norm_g = P.vec("backbone.norm.weight", C);
    W.norm_b = P.vec("backbone.norm.bias", C);
    for (int i = 0; i < v->layers; ++i) {
        const std::string p = S("backbone.convnext.", i, ".");
        // depthwise weight [C,1,7] -> [7][C] so that a lane's 4 channels are one float4 per tap
        const auto* dw = P.get(p + "dwconv.weight", (size_t)C * 7);
        if (!dw) break;
        Vec wv;
        wv.off = P.alloc((size_t)7 * C);
        wv.n = 7 * C;
        for (int ch = 0; ch < C; ++ch)
            for (int j = 0; j < 7; ++j) c->image[wv.off + (size_t)j * C + ch] = (*dw)[(size_t)ch * 7 + j];
        W.dw_w.push_back(wv);
        W.dw_b.push_back(P.vec(p + "dwconv.bias", C));
        W.ln_g.push_back(P.vec(p + "norm.weight", C));
        W.ln_b.push_back(P.vec(p + "norm.bias", C));
        W.pw1.push_back(P.panel(p + "pwconv1.weight", p + "pwconv1.bias", 0, v->inter, C, 1));
        // layer scale folded into pwconv2: gamma * (W x + b) = (gamma W) x + gamma b
        const auto* w2 = P.get(p + "pwconv2.weight", (size_t)C * v->inter);
        const auto* b2 = P.get(p + "pwconv2.bias", C);
        const auto* gm = P.get(p + "gamma", C);
        if (!w2 || !b2 || !gm) break;
        std::vector<float> ws(w2->size()), bs(C);
        for (int n = 0; n < C; ++n) {
            for (int k = 0; k < v->inter; ++k) ws[(size_t)n * v->inter + k] = (*gm)[n] * (*w2)[(size_t)n * v->inter + k];
            bs[n] = (*gm)[n] * (*b2)[n];
        }
        W.pw2.push_back(P.panel_from(ws.data(), bs.data(), 0, C, v->inter, 1));
    }
    W.fin_g = P.vec("backbone.final_layer_norm.weight", C);
    W.fin_b = P.vec("backbone.final_layer_norm.bias", C);
    // head: rows [log-magnitude 0..nb) | phase nb..2nb) re-spaced so that both halves start on a multiple of 4 columns
    v->im_off = round_up(nb, 4);
    v->ld_spec = round_up(v->im_off + nb, 4);
    {
        const auto* hw = P.get("head.out.weight", (size_t)2 * nb * C);
        const auto* hb = P.get("head.out.bias", (size_t)2 * nb);
        if (hw && hb) {
            std::vector<float> ws((size_t)v->ld_spec * C, 0.f), bs(v->ld_spec, 0.f);
            for (int r = 0; r < 2 * nb; ++r) {
                const int dst = r < nb ? r : v->im_off + (r - nb);
                std::memcpy(&ws[(size_t)dst * C], &(*hw)[(size_t)r * C], C * sizeof(float));
                bs[dst] = (*hb)[r];
            }
            W.head = P.panel_from(ws.data(), bs.data(), 0, v->ld_spec, C, 1);
        }
    }
    // inverse real DFT (torch.fft.irfft, norm "backward") times the synthesis window, as a [n_fft][ld_spec] matrix:
    // frame[n] = w[n]/N * sum_k c_k (Re_k cos(2 pi k n / N) - Im_k sin(2 pi k n / N)), c_0 = c_{N/2} = 1, else 2
    W.window = P.vec("aux.window", v->n_fft);
    if (P.ok) {
        const int N = v->n_fft;
        std::vector<float> bm((size_t)N * v->ld_spec, 0.f);
        const float* win = &c->image[W.window.off];
        const double two_pi = 6.283185307179586476925286766559;
        for (int n = 0; n < N; ++n)
            for (int k = 0; k < nb; ++k) {
                const double ck = (k == 0 || k == N / 2) ? 1.0 : 2.0;
                const double ang = two_pi * (double)(((long long)k * n) % N) / (double)N;
                bm[(size_t)n * v->ld_spec + k] = (float)((double)win[n] * ck * std::cos(ang) / N);
                bm[(size_t)n * v->ld_spec + v->im_off + k] = (float)(-(double)win[n] * ck * std::sin(ang) / N);
            }
        W.basis = P.panel_from(bm.data(), nullptr, 0, N, v->ld_spec, 1);
    }
    if (!P.ok) { set_error(P.why); return -1; }
    c->packed = true;
    return 0;
}

struct VocosBufs { float *MEL, *X, *Y, *H, *SPEC, *FR; int* STATUS; };
// ragged: the status words of the lengths check FIRST (mtts_vocos_ragged_status reads them at the workspace's base), then the
// buffers of the plain call
static void vocos_plan(const mtts_vocos* v, int B, int T, WS& ws, VocosBufs& b, bool ragged = false) {
    const size_t M = (size_t)B * T;
    b.STATUS = ragged ? static_cast<int*>(ws.bytes(4 * sizeof(int))) : nullptr;
    b.MEL = ws.f(M * round_up(v->n_mels, 4));
    b.X = ws.f(M * v->dim); b.Y = ws.f(M * v->dim); b.H = ws.f(M * v->inter);
    b.SPEC = ws.f(M * v->ld_spec); b.FR = ws.f(M * v->n_fft);
}

extern "C" {

mtts_vocos* mtts_vocos_create(int n_mels, int dim, int inter, int layers, int n_fft, int hop) {
    if (n_mels <= 0 || (n_mels & 3) || dim <= 0 || (dim & 3) || dim > 2048 || inter <= 0 || (inter & 3) || layers < 0 || n_fft <= 0 ||
        (n_fft & 3) || hop <= 0 || n_fft % hop) {
        set_error("mtts_vocos_create: unsupported shape (channels multiples of 4, dim <= 2048, hop divides n_fft)");
        return nullptr;
    }
    mtts_vocos* v = new mtts_vocos();
    v->gemm_terms = read_switches().gemm_terms;
    v->n_mels = n_mels; v->dim = dim; v->inter = inter; v->layers = layers; v->n_fft = n_fft; v->hop = hop;
    return v;
}
void mtts_vocos_destroy(mtts_vocos* v) { delete v; }
int mtts_vocos_set_tensor(mtts_vocos* v, const char* key, const float* h, int64_t numel) {
    if (!v) { set_error("null context"); return -1; }
    return set_tensor(v, key, h, numel);
}
int64_t mtts_vocos_weights_bytes(mtts_vocos* v) { return weights_bytes(v, vocos_pack); }
int mtts_vocos_upload_weights(mtts_vocos* v, void* d_weights, int64_t bytes) {
    return upload_weights(v, vocos_pack, "mtts_vocos_upload_weights", d_weights, bytes);
}
int64_t mtts_vocos_workspace_bytes(mtts_vocos* v, int B, int T) {
    if (!v) { set_error("null context"); return -1; }
    WS ws(nullptr, 0);
    VocosBufs b;
    vocos_plan(v, B, T, ws, b);
    return (int64_t)ws.off + 256;
}

}  // extern "C"

// Vocos.decode (reference matcha/vocos24k/vocos_wrapper.py:8-9): mel [B, n_mels, T] -> audio [B, hop*(T-1)].
// d_lengths (device int64 [B], frames; null = every row has T): row b is decoded as the reference decodes mel[b, :, :len_b] on
// its own -- every k7 conv (embed: zeroed mel rows; eight depthwise: length-aware taps) zero-pads at len_b, the iSTFT ends at
// frame len_b - 1 -- and the row is zero past hop * (len_b - 1).  The per-row kernels (pointwise GEMMs, LayerNorms, head, polar,
// inverse DFT) run on all B * T rows; rows at t >= len_b are computed and never read by a valid row.
static int vocos_decode(mtts_vocos* v, const float* d_mel, const int64_t* d_lengths, int B, int T, float* d_audio, void* d_ws,
                        int64_t ws_bytes, void* stream, const char* who) {
    if (!v) { set_error("null context"); return -1; }
    Component* c = v;
    RET_IF(check_ready(c));
    if (!d_mel || !d_audio || !d_ws || B <= 0) { set_error(std::string(who) + ": bad argument"); return -1; }
    if (T < 2) { set_error(std::string(who) + ": need at least 2 frames"); return -1; }
    hipStream_t s = static_cast<hipStream_t>(stream);
    WS ws(d_ws, (size_t)ws_bytes);
    VocosBufs b;
    vocos_plan(v, B, T, ws, b, d_lengths != nullptr);
    if (ws.overflow) { set_error("vocos workspace too small"); return -1; }
    const VocosW& Wt = v->w;
    const int C = v->dim, M = B * T, ldm = round_up(v->n_mels, 4), nb = v->n_fft / 2 + 1;
    if (d_lengths) LAUNCH(c, 2, 0, s, launch_vocos_lengths_check(d_lengths, B, T, b.STATUS, s));
    // ragged: the transpose writes the rows at t >= len_b as zero, so the embed conv's taps beyond an utterance's end read its
    // zero padding.  (The GEMM's a_mask would multiply instead: one more launch for the mask, and NaN * 0 in a padded mel.)
    LAUNCH(c, 2, 0, s, launch_cf_to_cl(d_mel, nullptr, B, v->n_mels, T, b.MEL, ldm, 0, s, 0, d_lengths));
    {   // embed: Conv1d(n_mels -> dim, k7, pad 3), then LayerNorm(eps 1e-6)
        GemmArgs a;
        panel_args(c, Wt.embed, a); rows_plain(a, B, T); taps_centered(a, 7);
        a.a0 = b.MEL; a.lda0 = ldm; a.c0 = v->n_mels; a.out = b.Y; a.ldc = C;
        RET_IF(run_gemm(c, a, s));
        LayerNormArgs ln;
        ln.x = b.Y; ln.ldx = C; ln.y = b.X; ln.ldy = C; ln.M = M; ln.C = C; ln.T = T; ln.eps = 1e-6f;
        ln.gamma = W(c, Wt.norm_g.off); ln.beta = W(c, Wt.norm_b.off);
        LAUNCH(c, 2, 0, s, launch_layernorm(ln, s));
    }
    for (int i = 0; i < v->layers; ++i) {   // ConvNeXtBlock: x += gamma * pwconv2(GELU(pwconv1(LN(dwconv(x)))))
        LAUNCH(c, 2, 0, s, launch_dwconv7_ln(b.X, W(c, Wt.dw_w[i].off), W(c, Wt.dw_b[i].off), W(c, Wt.ln_g[i].off), W(c, Wt.ln_b[i].off),
                                             1e-6f, B, T, C, b.Y, s, d_lengths));
        GemmArgs p1;
        panel_args(c, Wt.pw1[i], p1); rows_plain(p1, B, T);
        p1.a0 = b.Y; p1.lda0 = C; p1.c0 = C; p1.act = ACT_GELU; p1.out = b.H; p1.ldc = v->inter;
        RET_IF(run_gemm(c, p1, s));
        GemmArgs p2;
        panel_args(c, Wt.pw2[i], p2); rows_plain(p2, B, T);
        p2.a0 = b.H; p2.lda0 = v->inter; p2.c0 = v->inter; p2.res = b.X; p2.ldr = C; p2.out = b.X; p2.ldc = C;
        RET_IF(run_gemm(c, p2, s));
    }
    {
        LayerNormArgs ln;
        ln.x = b.X; ln.ldx = C; ln.y = b.Y; ln.ldy = C; ln.M = M; ln.C = C; ln.T = T; ln.eps = 1e-6f;
        ln.gamma = W(c, Wt.fin_g.off); ln.beta = W(c, Wt.fin_b.off);
        LAUNCH(c, 2, 0, s, launch_layernorm(ln, s));
        GemmArgs h;   // ISTFTHead.out
        panel_args(c, Wt.head, h); rows_plain(h, B, T);
        h.a0 = b.Y; h.lda0 = C; h.c0 = C; h.out = b.SPEC; h.ldc = v->ld_spec;
        RET_IF(run_gemm(c, h, s));
        LAUNCH(c, 2, 0, s, launch_spec_polar(b.SPEC, M, v->ld_spec, nb, v->im_off, 1e2f, s));
        GemmArgs d;   // irfft * window as a GEMM
        panel_args(c, Wt.basis, d); rows_plain(d, B, T);
        d.a0 = b.SPEC; d.lda0 = v->ld_spec; d.c0 = v->ld_spec; d.out = b.FR; d.ldc = v->n_fft;
        RET_IF(run_gemm(c, d, s));
        LAUNCH(c, 2, 0, s, launch_istft_ola(b.FR, W(c, Wt.window.off), B, T, v->n_fft, v->hop, d_audio, s, d_lengths));
    }
    return 0;
}

extern "C" {

int mtts_vocos_decode(mtts_vocos* v, const float* d_mel, int B, int T, float* d_audio, void* d_ws, int64_t ws_bytes, void* stream) {
    return vocos_decode(v, d_mel, nullptr, B, T, d_audio, d_ws, ws_bytes, stream, "mtts_vocos_decode");
}

int64_t mtts_vocos_ragged_workspace_bytes(mtts_vocos* v, int B, int T) {
    if (!v) { set_error("null context"); return -1; }
    if (B <= 0 || T < 2) { set_error("mtts_vocos_ragged_workspace_bytes: bad shape"); return -1; }
    WS ws(nullptr, 0);
    VocosBufs b;
    vocos_plan(v, B, T, ws, b, true);
    return (int64_t)ws.off + 256;
}
int mtts_vocos_decode_ragged(mtts_vocos* v, const float* d_mel, const int64_t* d_lengths, int B, int T, float* d_audio, void* d_ws,
                             int64_t ws_bytes, void* stream) {
    if (!d_lengths) { set_error("mtts_vocos_decode_ragged: null lengths"); return -1; }
    return vocos_decode(v, d_mel, d_lengths, B, T, d_audio, d_ws, ws_bytes, stream, "mtts_vocos_decode_ragged");
}
// The lengths check's verdict (the status words at the base of the ragged call's workspace).  This is the one place that waits
// for the stream: callers that go on to mtts_waveform_finish read its out_lengths instead (-1 marks the same rows).
int mtts_vocos_ragged_status(const void* d_ws, void* stream) {
    int st[3];
    if (read_status("mtts_vocos_ragged_status", d_ws, stream, st)) return -1;
    if (st[0] != 0) {
        set_error("mtts_vocos_decode_ragged: lengths[" + std::to_string(st[0] - 1) + "] = " + std::to_string(st[1]) +
                  " is outside [1, T = " + std::to_string(st[2]) + "]");
        return -1;
    }
    return 0;
}

}  // extern "C"
