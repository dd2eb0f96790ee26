// TextEncoder.forward on one HIP stream, and the steps between it and the estimator: speaker embeddings, durations, the
// alignment pool.  No torch, no allocation or synchronisation inside the launch functions (graph-capturable).
#include "host.h"

using namespace mtts;

extern "C" {

// ------------------------------------------------------------------------------------------------ text encoder
struct EncBufs {
    float *X0, *P1, *P2, *Y, *H, *H2, *QKV, *ATT, *F1, *PM, *MU, *FILM, *D1, *D2;
};
static void plan_encoder(const mtts_ctx* c, int B, int Tx, WS& ws, EncBufs& e) {
    const mtts_config& g = c->cfg;
    const size_t M = (size_t)B * Tx;
    const int nch = g.enc_channels, Hd = nch + g.spk_emb_dim, F = g.dp_filter;
    (void)ws.bytes(256);                 // header: the call's range flag (begin_call)
    e.X0 = ws.f(M * nch); e.P1 = ws.f(M * nch); e.P2 = ws.f(M * nch); e.Y = ws.f(M * std::max(nch, F));
    e.H = ws.f(M * Hd); e.H2 = ws.f(M * Hd); e.QKV = ws.f(M * 3 * Hd); e.ATT = ws.f(M * Hd);
    e.F1 = ws.f(M * g.enc_filter); e.PM = ws.f(M * nch); e.MU = ws.f(M * round_up(g.n_feats, 4));
    e.FILM = ws.f((size_t)B * 2 * F); e.D1 = ws.f(M * F); e.D2 = ws.f(M * F);
}

int64_t mtts_encoder_workspace_bytes(mtts_ctx* c, int B, int Tx) {
    if (!c || (!c->packed && pack_all(c))) return -1;
    WS ws(nullptr, 0);
    EncBufs e;
    plan_encoder(c, B, Tx, ws, e);
    return (int64_t)ws.off + 256;
}

// TextEncoder.forward (reference text_encoder.py:375-406)
// (spk_grad.hip's taped forward repeats this launch sequence with per-layer buffers and must produce the same bits: a change here is
// mirrored there; tests/test_hip_spk_grad.py compares the two bit for bit)
int mtts_text_encoder_forward(mtts_ctx* c, const int64_t* d_x, const int64_t* d_x_lengths, const float* d_e_enc, const float* d_e_dur,
                              int B, int Tx, float* d_mu_x, float* d_logw, float* d_x_mask, void* d_ws, int64_t ws_bytes, void* stream) {
    CTX_GUARD(c);
    RET_IF(check_ready(c));
    const mtts_config& g = c->cfg;
    const EncW& E = c->enc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int nch = g.enc_channels, Sd = g.spk_emb_dim, Hd = nch + Sd, F = g.dp_filter, M = B * Tx;
    const int dh = Hd / g.enc_heads, d_rope = dh / 2;
    if ((size_t)Tx * d_rope > (size_t)E.rope_cos.n) { set_error("Phonetic representation too long, exceeds RoPE cache size"); return -1; }
    WS ws(d_ws, (size_t)ws_bytes);
    EncBufs e;
    plan_encoder(c, B, Tx, ws, e);
    if (ws.overflow) { set_error("encoder workspace too small"); return -1; }
    RET_IF(begin_call(c, d_ws, s));
    float* xm = d_x_mask;   // [B,1,Tx] == rows [B*Tx]
    LAUNCH(c, 2, 0, s, launch_seq_mask(d_x_lengths, B, Tx, xm, s));
    LAUNCH(c, 2, 0, s, launch_embedding(d_x, W(c, E.emb.off), M, nch, sqrtf((float)nch), xm, e.X0, nch, s));
    // ---- prenet: ConvSiluNorm (reference text_encoder.py:55-62)
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
        GemmArgs a;   // (x_org + proj(x)) * mask, written into the first n_channels columns of the hidden rows
        panel_args(c, E.pre_proj, a); rows_plain(a, B, Tx);
        a.a0 = cur; a.lda0 = nch; a.c0 = nch; a.out_mask = xm; a.res = e.X0; a.ldr = nch; a.out = e.H; a.ldc = Hd;
        RET_IF(run_gemm(c, a, s));
    }
    LAUNCH(c, 2, 0, s, launch_bcast_rows(d_e_enc, B, Tx, Sd, xm, e.H, Hd, nch, s));
    // ---- Encoder: post-LN transformer with RoPE attention and conv FFN (reference text_encoder.py:299-316)
    for (int l = 0; l < g.enc_layers; ++l) {
        GemmArgs q;
        panel_args(c, E.qkv[l], q); rows_plain(q, B, Tx);
        q.a0 = e.H; q.lda0 = Hd; q.c0 = Hd; q.out = e.QKV; q.ldc = 3 * Hd;
        RET_IF(run_gemm(c, q, s));
        LAUNCH(c, 2, 0, s, launch_rope(e.QKV, B, Tx, g.enc_heads, dh, d_rope, W(c, E.rope_cos.off), W(c, E.rope_sin.off), s));
        AttnArgs at;
        at.qkv = e.QKV; at.mask = xm; at.out = e.ATT; at.B = B; at.T = Tx; at.H = g.enc_heads; at.D = dh;
        at.scale = 1.0f / sqrtf((float)dh); at.mask_mode = 1;
        RET_IF(run_attn(c, at, s));
        GemmArgs o;
        panel_args(c, E.o[l], o); rows_plain(o, B, Tx);
        o.a0 = e.ATT; o.lda0 = Hd; o.c0 = Hd; o.res = e.H; o.ldr = Hd; o.out = e.H2; o.ldc = Hd;
        RET_IF(run_gemm(c, o, s));
        LayerNormArgs n1;
        n1.x = e.H2; n1.ldx = Hd; n1.y = e.H; n1.ldy = Hd; n1.M = M; n1.C = Hd; n1.T = Tx;
        n1.gamma = W(c, E.n1_g[l].off); n1.beta = W(c, E.n1_b[l].off); n1.mask = xm;
        LAUNCH(c, 2, 0, s, launch_layernorm(n1, s));
        // FFN: conv k5 -> ReLU -> mask -> conv k5.  The second conv is the encoder's long-K GEMM (K = 5 x filter) on a grid
        // far under one round of workgroups: in the fp16-split mode the hidden layer is handed over as a masked P16 image
        // (written by the first conv's epilogue) so that it runs on gemm_p16.hip's prefetch ring (198 -> ~80 us at B = 32).
        const bool ffn_p16 = c->sw.p16_on && c->gemm_terms == 2 && (g.enc_filter % 32) == 0;
        _Float16* F16 = reinterpret_cast<_Float16*>(e.F1);        // same bytes as the fp32 hidden layer
        GemmArgs f1;
        panel_args(c, E.ffn1[l], f1); rows_plain(f1, B, Tx); taps_centered(f1, g.enc_kernel);
        f1.a0 = e.H; f1.lda0 = Hd; f1.c0 = Hd; f1.act = ACT_RELU;
        if (ffn_p16) { f1.out16 = F16; f1.ld16 = 2 * g.enc_filter; f1.out16_mask = xm; }
        else { f1.out = e.F1; f1.ldc = g.enc_filter; }
        RET_IF(run_gemm(c, f1, s));
        GemmArgs f2;
        panel_args(c, E.ffn2[l], f2); rows_plain(f2, B, Tx); taps_centered(f2, g.enc_kernel);
        if (ffn_p16) { f2.a16_0 = F16; f2.lda16_0 = 2 * g.enc_filter; f2.c0 = g.enc_filter; f2.fast16 = false; }   // durations: full precision
        else { f2.a0 = e.F1; f2.lda0 = g.enc_filter; f2.c0 = g.enc_filter; f2.a_mask = xm; }
        f2.out_mask = xm; f2.res = e.H; f2.ldr = Hd; f2.out = e.H2; f2.ldc = Hd;
        RET_IF(run_gemm(c, f2, s));
        LayerNormArgs n2 = n1;
        n2.gamma = W(c, E.n2_g[l].off); n2.beta = W(c, E.n2_b[l].off);
        LAUNCH(c, 2, 0, s, launch_layernorm(n2, s));
    }
    // ---- proj_m: 1x1 -> SiLU -> 1x1, masked (reference text_encoder.py:359-363,402)
    {
        GemmArgs a;
        panel_args(c, E.pm0, a); rows_plain(a, B, Tx);
        a.a0 = e.H; a.lda0 = Hd; a.c0 = Hd; a.act = ACT_SILU; a.out = e.PM; a.ldc = nch;
        RET_IF(run_gemm(c, a, s));
        GemmArgs b;
        const int ldm = round_up(g.n_feats, 4);
        panel_args(c, E.pm2, b); rows_plain(b, B, Tx);
        b.a0 = e.PM; b.lda0 = nch; b.c0 = nch; b.out_mask = xm; b.out = e.MU; b.ldc = ldm;
        RET_IF(run_gemm(c, b, s));
        LAUNCH(c, 2, 0, s, launch_cl_to_cf(e.MU, ldm, B, g.n_feats, Tx, d_mu_x, Tx, 1.0f, 0.0f, s));
    }
    // ---- DurationPredictor with FiLM (reference text_encoder.py:101-112)
    {
        GemmArgs fm;
        panel_args(c, E.film, fm); rows_plain(fm, B, 1);
        fm.a0 = d_e_dur; fm.lda0 = Sd; fm.c0 = Sd; fm.out = e.FILM; fm.ldc = 2 * F;
        RET_IF(run_gemm(c, fm, s));
        const float* dcur = e.H;
        int dc = Hd;
        for (int i = 0; i < g.dp_layers; ++i) {
            GemmArgs a;
            panel_args(c, E.dp_conv[i], a); rows_plain(a, B, Tx); taps_centered(a, g.dp_kernel);
            a.a0 = dcur; a.lda0 = dc; a.c0 = dc; a.a_mask = xm; a.act = ACT_RELU; a.out = e.Y; a.ldc = F;
            RET_IF(run_gemm(c, a, s));
            float* dst = (i & 1) ? e.D2 : e.D1;
            LayerNormArgs ln;
            ln.x = e.Y; ln.ldx = F; ln.y = dst; ln.ldy = F; ln.M = M; ln.C = F; ln.T = Tx;
            ln.gamma = W(c, E.dp_g[i].off); ln.beta = W(c, E.dp_b[i].off); ln.film = e.FILM;
            LAUNCH(c, 2, 0, s, launch_layernorm(ln, s));
            dcur = dst;
            dc = F;
        }
        GemmArgs p;
        panel_args(c, E.dp_proj, p); rows_plain(p, B, Tx);
        p.a0 = dcur; p.lda0 = dc; p.c0 = dc; p.a_mask = xm; p.out_mask = xm; p.out = d_logw; p.ldc = 1;
        RET_IF(run_gemm(c, p, s));
    }
    return 0;
}

int mtts_speaker_embedding(mtts_ctx* c, int table, const int64_t* d_ids, int B, float* d_out, void* stream) {
    RET_IF(check_ready(c));
    const Vec& v = table == 0 ? c->enc.spk_enc : c->enc.spk_dur;
    HIP_OK(launch_embedding(d_ids, W(c, v.off), B, c->cfg.spk_emb_dim, 1.0f, nullptr, d_out, c->cfg.spk_emb_dim, static_cast<hipStream_t>(stream)));
    return 0;
}

int mtts_durations(const float* d_logw, const float* d_x_mask, float scale_correction, float length_scale, int B, int Tx,
                   float* d_durations, int32_t* d_cum, int64_t* d_y_fine_lengths, void* stream) {
    HIP_OK(launch_durations(d_logw, d_x_mask, scale_correction, length_scale, B, Tx, d_durations, d_cum, d_y_fine_lengths,
                            static_cast<hipStream_t>(stream)));
    return 0;
}

int mtts_durations_per_utterance(const float* d_logw, const float* d_x_mask, const float* d_scale_correction, const float* d_length_scale,
                                 int B, int Tx, float* d_durations, int32_t* d_cum, int64_t* d_y_fine_lengths, void* stream) {
    if (!d_scale_correction || !d_length_scale) { set_error("mtts_durations_per_utterance: null factor array"); return -1; }
    HIP_OK(launch_durations(d_logw, d_x_mask, 1.0f, 1.0f, B, Tx, d_durations, d_cum, d_y_fine_lengths, static_cast<hipStream_t>(stream),
                            d_scale_correction, d_length_scale));
    return 0;
}

int mtts_durations_given(const float* d_dur, const float* d_x_mask, float length_scale, const float* d_length_scale, const int32_t* d_given_rows,
                         int B, int Tx, float* d_durations, int32_t* d_cum, int64_t* d_y_fine_lengths, void* stream) {
    if (!d_dur || !d_x_mask || !d_durations || !d_cum || !d_y_fine_lengths) { set_error("mtts_durations_given: null argument"); return -1; }
    if (B < 1 || Tx < 1) { set_error("mtts_durations_given: bad shape"); return -1; }
    HIP_OK(launch_durations_given(d_dur, d_x_mask, length_scale, d_length_scale, d_given_rows, B, Tx, d_durations, d_cum, d_y_fine_lengths,
                                  static_cast<hipStream_t>(stream)));
    return 0;
}

int mtts_durations_shaped(const float* d_logw, const float* d_x_mask, const float* d_scale_correction, const float* d_length_scale,
                          const float* d_given, const int32_t* d_given_rows, const float* d_token_scale, const float* d_token_extend, int B,
                          int Tx, float* d_durations, int32_t* d_cum, int64_t* d_y_fine_lengths, void* stream) {
    if (!d_x_mask || !d_scale_correction || !d_length_scale || !d_durations || !d_cum || !d_y_fine_lengths) {
        set_error("mtts_durations_shaped: null argument");
        return -1;
    }
    if (!d_logw && !(d_given && !d_given_rows)) { set_error("mtts_durations_shaped: null d_logw (a predicted row reads it)"); return -1; }
    if (d_given_rows && !d_given) { set_error("mtts_durations_shaped: d_given_rows without d_given"); return -1; }
    if (B < 1 || Tx < 1) { set_error("mtts_durations_shaped: bad shape"); return -1; }
    HIP_OK(launch_durations_shaped(d_logw, d_x_mask, d_scale_correction, d_length_scale, d_given, d_given_rows, d_token_scale, d_token_extend,
                                   B, Tx, d_durations, d_cum, d_y_fine_lengths, static_cast<hipStream_t>(stream)));
    return 0;
}

int mtts_align_pool(const float* d_mu_x, const int32_t* d_cum, const int64_t* d_y_fine_lengths, int B, int n_feats, int Tx, int T_pad,
                    float* d_mu_y, float* d_y_mask, int64_t* d_y_lengths, void* stream) {
    HIP_OK(launch_align_pool(d_mu_x, d_cum, d_y_fine_lengths, B, n_feats, Tx, T_pad, d_mu_y, d_y_mask, d_y_lengths,
                             static_cast<hipStream_t>(stream)));
    return 0;
}

}  // extern "C"
