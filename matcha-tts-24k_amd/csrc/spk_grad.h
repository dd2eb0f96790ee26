// What spk_grad.hip shares with dp_grad.hip (the duration predictor's parameter gradients): the taped forward of the frozen encoder,
// the walk back through the duration predictor, and the launchers both are made of.  Defined in spk_grad.hip.
#pragma once
#include "host.h"

namespace mtts {

constexpr int SG_MAX_TX = 1024;           // tokens, as mtts_mas / score.hip (cumulative durations in LDS)
constexpr size_t SG_SCORE_OFF = 256;      // the score workspace (status header first) inside this call's workspace: plan_spk_grad
                                          // carves it right behind the 256-byte call header; mtts_spk_grad refuses to run otherwise
constexpr int SG_MAX_LAYERS = 16;         // encoder / duration-predictor layers the per-layer tape has room for

// forward (norm_glue.hip layernorm_kernel):  xh = (x - mean) rstd;  a = xh gamma + beta;  [a = silu(a)];  [y = a fg_b + fb_b];  [y *= mask]
struct LnBwdArgs {
    const float* x = nullptr; int ldx = 0;        // the LayerNorm's input rows
    const float* dy = nullptr; int lddy = 0;      // upstream gradient
    float* dx = nullptr; int lddx = 0;
    int M = 0, C = 0, T = 1;
    const float* gamma = nullptr; const float* beta = nullptr;   // null: 1 / 0
    float eps = 1e-5f;
    int act = ACT_NONE;                           // ACT_SILU: the forward applied SiLU behind the affine
    const float* film = nullptr;                  // [B][2C] gamma | beta of the FiLM
    float* film_prod = nullptr;                   // [M][C]: dy * a, whose token sum is d gamma_b (d beta_b is the token sum of dy)
    const float* mask = nullptr;                  // [M]: rows with 0 get a zero gradient
    int gate = ACT_NONE;                          // ACT_RELU: x is a ReLU output, dx *= (x > 0)
};
hipError_t launch_ln_bwd(const LnBwdArgs& a, hipStream_t s);
hipError_t launch_colsum(const float* src, int ld, int col0, int C, int B, int T, const int64_t* len, const int32_t* verdict, float* dst,
                         int ldd, int dcol0, int accumulate, hipStream_t s);
// The transposed weight of a Linear / Conv1d(k, pad k / 2) in torch layout: w [N][C][k] -> wt [C][N][k] with the taps reversed
std::vector<float> transposed(const float* w, int N, int C, int k, int Np = 0);

struct SgBufs {
    float *X0, *P1, *P2, *Y, *PMpre, *PM, *MU, *FILM, *D1, *D2, *mu_x, *logw, *xm;
    float *Hin[SG_MAX_LAYERS + 1], *QKV[SG_MAX_LAYERS], *ATT[SG_MAX_LAYERS], *S1[SG_MAX_LAYERS], *H1[SG_MAX_LAYERS], *F1[SG_MAX_LAYERS],
        *S2[SG_MAX_LAYERS], *DY[SG_MAX_LAYERS];       // per layer (fixed arrays: no host allocation in the launch path)
    float *GA, *GB, *GF, *GQKV, *GATT, *stats, *GMU, *GPM, *GDA, *GDB, *FPROD, *DFILM;
    int32_t* dur;
    void *score, *mas;
    size_t score_bytes = 0, mas_bytes = 0, off_score = 0, off_mu_x = 0, off_logw = 0, off_xm = 0, off_hout = 0;
};

// The duration predictor under training (dp_grad.hip): walk_dur then takes the transposed panels and the LayerNorm affines from the
// training component instead of the context's backward panels and image, and calls `reduce(i)` once layer i's operands are ready --
// GDA holds the gradient at the layer's output (behind the FiLM), GDB the gradient at its convolution's output (behind the ReLU gate) --
// and before the next GEMM reuses GDA.
struct DurTrain {
    const Component* comp = nullptr;
    const Panel* convT = nullptr;                 // [dp_layers], [0] unused
    Panel filmT;
    const float* gamma[SG_MAX_LAYERS] = {};
    const float* beta[SG_MAX_LAYERS] = {};
    int (*reduce)(void* ctx, int layer) = nullptr;   // (a plain pointer: no host allocation in the launch path)
    void* reduce_ctx = nullptr;
};

// The taped forward and the two walks back from seeded gradients, with the call's context, buffers and derived sizes.
struct SgCall {
    mtts_ctx* c;
    const SgBufs& e;
    hipStream_t s;
    int B, Tx;
    const mtts_config& g;
    const EncW& E;
    const SpkGradW& GW;
    const Component* G;
    int nch, Sd, Hd, F, M, nf, dh, d_rope, ldm, L;
    bool ffn_p16;
    float* xm;
    SgCall(mtts_ctx* ctx, const SgBufs& bufs, hipStream_t stream, int B_, int Tx_);
    // what every entry checks once its workspace is planned (`who` names it in the error texts)
    int ready(const char* who, const void* d_grad_buf) const;
    int tgemm(const Component* comp, const Panel& p, const float* a0, int lda, int c0, int ntaps, const float* res, int ldr,
              const float* out_mask, float* out, int ldc, int rowsB, int rowsT) const;
    int tgemm(const Panel& p, const float* a0, int lda, int c0, int ntaps, const float* res, int ldr, const float* out_mask, float* out,
              int ldc, int rowsB, int rowsT) const {
        return tgemm(G, p, a0, lda, c0, ntaps, res, ldr, out_mask, out, ldc, rowsB, rowsT);
    }
    // the frozen part: mask, embedding, prenet and encoder layers up to the rows proj_m and the duration predictor read (e.Hin[L])
    int forward_encoder(const int64_t* d_x, const int64_t* d_x_lengths, const float* d_e_enc) const;
    int forward(const int64_t* d_x, const int64_t* d_x_lengths, const float* d_e_enc, const float* d_e_dur) const;
    int walk_prior(const int64_t* d_x_lengths, const int32_t* verdict, float* d_g_enc) const;
    // d_g_dur may be null under training (the caller wants the parameter gradients alone)
    int walk_dur(const int64_t* d_x_lengths, const int32_t* verdict, float* d_g_dur, const DurTrain* train = nullptr) const;
};

}  // namespace mtts
