// The estimator and the ODE solver on one HIP stream: workspace planning, the launch sequences of Decoder.forward and
// BASECFM.solve, their C ABI.  No torch, no allocation or synchronisation inside the launch functions (graph-capturable).
#include "host.h"

namespace mtts {

// Prefetch workgroups of a chain launch of qb-row workgroups over M rows (want = Switches::chain_pf): none, or eight, when `want`
// would push a one-round grid into a second round of the chip's CUs.
static int one_round_prefetchers(int M, int qb, int want) {
    const int nwg = (M + qb - 1) / qb;
    if (nwg <= CHIP_CUS && nwg + want > CHIP_CUS) return (want >= 8 && nwg + 8 <= CHIP_CUS) ? 8 : 0;
    return want;
}
// Launch plan of a chain launch over M rows (hidden chunk ch; qb_forced = Switches::chain_qb or 0; want = Switches::chain_pf): rows
// per workgroup and prefetch workgroups.  32-row workgroups while they -- with the prefetchers -- are one round of the chip's CUs (a
// 32-row workgroup lives 99 us, a 48-row one 116 us: both are bound by the 7 MB they stream, profiles/r03_chain_prefetch_stamps.log),
// the largest shape beyond; no prefetchers when they would push a one-round grid into a second round.
void chain_plan(int M, int ch, int qb_forced, int want, int* qb, int* pf) {
    const int qb_big = ch == 256 ? 48 : 64;
    const bool fits32 = (M + 31) / 32 + want <= CHIP_CUS;
    *qb = (qb_forced == 32 || qb_forced == qb_big) ? qb_forced : (fits32 ? 32 : qb_big);
    *pf = one_round_prefetchers(M, *qb, want);
}
constexpr int PAIR_QB = 48;      // rows per tile of the model's pair launches
bool tblock_pair_possible(const Switches& sw, int C, int inner, int n_qkv, int ch) {
    return sw.pair_on && C == 384 && ch == 256 && chain_supported_pair(C, inner, ch, n_qkv) && chain_shape_exists(C, PAIR_QB, ch);
}
// The chain launch when the stream was packed and the batch is large enough that a workgroup per qb rows fills the chip: every
// workgroup streams ALL of the chain's weights (~7 MB at width 384), which only pays when their cost is shared by many rows per CU
// (DESIGN.md section 5).  Below chain_min_rows, from pair_min_rows on: the pair form -- two workgroups of one XCD per 48-row tile,
// each streaming half of the FeedForward and of the q|k|v passes -- while all of them (and the prefetchers) are resident at once.
// Everything else, and any shape the launcher has no kernel for: the tiled launches.
TBlockPlan tblock_plan(const Switches& sw, int C, int inner, int n_qkv, int ch, int M, bool has_chain, bool has_pair) {
    TBlockPlan p;
    if (M <= 0 || !chain_supported(C, inner, n_qkv)) return p;
    if (has_chain && M >= sw.chain_min_rows) {
        int qb = 0, pf = 0;
        chain_plan(M, ch, sw.chain_qb, sw.chain_pf, &qb, &pf);
        if (!chain_shape_exists(C, qb, ch)) return p;
        p.form = 1; p.qb = qb; p.grid = (M + qb - 1) / qb; p.pf = pf;
        return p;
    }
    const int grid = 16 * (((M + PAIR_QB - 1) / PAIR_QB + 7) / 8);
    if (has_pair && tblock_pair_possible(sw, C, inner, n_qkv, ch) && M >= sw.pair_min_rows && grid + 16 <= CHIP_CUS) {
        p.form = 2; p.qb = PAIR_QB; p.grid = grid;
        p.pf = sw.chain_pf ? 16 : 0;      // two per XCD, one per half (pair grids are admitted up to 240 workgroups)
    }
    return p;
}
static int run_chain(mtts_ctx* c, const ChainArgs& a0, hipStream_t s) {
    ChainArgs a = a0;
    a.range_flag = c->cur_flag;
    a.store_wt = c->store_wt & (WT_CHAIN_X | WT_CHAIN_QKV);
    LAUNCHB(c, 0, chain_flops(a), chain_bytes(a), s, launch_tblock_chain(a, s));
    return 0;
}
// Launch plan of the one-plane chain (tblock_chain_h16.hip) over M rows at width C: the smallest workgroup height whose grid -- with
// the prefetchers -- is ONE round of the chip's CUs (a workgroup's lifetime is set by the stream it pulls, not by its rows), the
// tallest one beyond; 96-row workgroups exist at width 384 with hidden chunk 256 only, and chunk 128 there has 64-row ones only.
// qb_forced = Switches::chain16_qb or 0.
static void chain16_plan(int M, int C, int ch, int qb_forced, int want, int* qb, int* pf) {
    const bool tall = C == 384 && ch == 256;
    const int cand[3] = {32, 64, 96};
    const int ncand = tall ? 3 : 2;
    *qb = cand[ncand - 1];
    for (int i = 0; i < ncand; ++i)
        if ((M + cand[i] - 1) / cand[i] + want <= CHIP_CUS) { *qb = cand[i]; break; }
    if (qb_forced == 32 || qb_forced == 64 || (qb_forced == 96 && tall)) *qb = qb_forced;
    if (C == 384 && ch == 128) *qb = 64;
    *pf = one_round_prefetchers(M, *qb, want);
}
static int run_chain_h16(mtts_ctx* c, const ChainH16Args& a0, hipStream_t s) {
    ChainH16Args a = a0;
    a.range_flag = c->cur_flag;
    chain16_plan(a.M, a.C, a.ch, c->sw.chain16_qb, c->sw.chain_pf, &a.qb, &a.pf_wgs);
    LAUNCHB(c, 0, chain_h16_flops(a), chain_h16_bytes(a), s, launch_tblock_chain_h16(a, s));
    return 0;
}
static int run_conv_gn(Component* c, const ConvGnArgs& a0, hipStream_t s) {
    ConvGnArgs a = a0;
    a.range_flag = c->cur_flag;
    a.store_wt = (c->store_wt & WT_CONV_GN) != 0;
    LAUNCHB(c, 0, conv_gn_flops(a), conv_gn_bytes(a), s, launch_conv_gn(a, s));
    return 0;
}

// ================================================================================================ decoder
struct DecBufs {
    int B = 0, T = 0, nl = 0;
    std::vector<int> Tl;                 // frames per level
    std::vector<float*> mask;            // [B*T_l]
    // The flow of the call (p16_decoder): between two launches an activation is either fp32 rows or an image its producer
    // wrote for its consumers -- P16, or H16 in the 16-bit storage mode.  The slots of this group hold whichever the flow uses
    // (an image has at most the bytes of the fp32 rows); everything else is fp32 in both flows.
    bool p16 = false;
    int ew = 2;                          // halves per image element: 2 = P16 (head + residual), 1 = H16 (16-bit storage mode)
    std::vector<float*> bufA, bufB, skip;   // per level: the two slots the blocks alternate between; the down path's output
    float *H = nullptr;                  // Block1D output (conv2 / final projection input), already masked
    float *QKV = nullptr, *ATT = nullptr, *FF = nullptr;
    float *Y = nullptr, *Rr = nullptr;   // conv output the GroupNorm reads; 1x1 residual conv output
    float *mean = nullptr, *rstd = nullptr, *gnp = nullptr, *lnp = nullptr;
    // image flow only
    float* X = nullptr;                  // the residual stream x of the ResNet + transformer blocks in flight (stream())
    float* XM = nullptr;                 // masked x | mu | 0 state
    float* gns = nullptr;                // GroupNorm tile statistics left by the conv GEMMs' epilogues
    // Where a ResNet and its transformer blocks keep their residual stream, unmasked, while their launches update it in place:
    // the image flow in X (the last launch writes the masked copy into the destination slot), fp32 rows in the destination slot
    // itself.
    float* stream(float* dst) const { return p16 ? X : dst; }
    float *xmu = nullptr, *xmu2 = nullptr, *vel[4] = {nullptr, nullptr, nullptr, nullptr};
    float *TS = nullptr, *T1 = nullptr, *T2 = nullptr, *T3 = nullptr, *TB = nullptr;
    int ldx = 0, ldv = 0;
    // frame tables (kernels.h FrameTableArgs), per level: null when every utterance owns all T rows
    int T_true = 0;                      // the reference's padded length; T above is the rows per utterance actually held
    bool folded = false;
    std::vector<int*> nrows, nextra;     // rows in the statistics / attention keys; closed-form bias-row copies
    std::vector<float*> kbias;           // additive attention key bias (= mask when not folded)
    const int* nr(int l) const { return tables ? nrows[l] : nullptr; }
    const int* ne(int l) const { return folded ? nextra[l] : nullptr; }
    const float* kb(int l) const { return folded ? kbias[l] : mask[l]; }
    bool tables = false;
    unsigned int* pair_flag = nullptr;   // pair form of the chain launch: one flag per (row tile, half), zeroed per call
    // One time per utterance (mtts_cfm_step): TB then holds a bias row per (stage, utterance), row stage * B + b, and the ResNets'
    // bias consumers step tb_stride floats per utterance (0: one row per evaluation for the whole batch).
    int tb_stride = 0;
    float *step_tv = nullptr, *step_dt = nullptr;        // [4 * B] stage times, [B] dt
    float *rs_full = nullptr, *rs_half = nullptr;        // [B*T] mask * dt, mask * dt/2: the final projection's row factors
    bool qkv_ready = false;              // the previous block's chain launch already left this block's q|k|v image in QKV
};

// The estimator runs on images (gemm_p16.hip, attention P16 I/O) when the context computes in the fp16-split mode, every level
// has whole 64-channel slices and 64-wide heads, and there is at least one transformer block per ResNet (the ResNet output then
// always feeds a LayerNorm'd projection first); MTTS_P16=0 (read at mtts_create) keeps fp32 rows.  Any other estimator runs
// every block on fp32 rows.
static bool p16_decoder(const mtts_ctx* c) {
    const mtts_config& g = c->cfg;
    if (!c->sw.p16_on || c->gemm_terms != 2 || g.dec_head_dim != 64 || g.dec_n_blocks < 1 || (g.n_feats & 1)) return false;
    for (int l = 0; l < g.dec_levels; ++l)
        if (g.dec_channels[l] % 64) return false;
    return true;
}

// Rows of the time-embedding buffers: the evaluations of a whole solve, or the (stage, utterance) pairs of one rk4 step of B utterances.
static int step_time_rows(int B) { return std::max(MAX_EVALS, 4 * B); }

static int plan_decoder(const mtts_ctx* c, int B, int T, int max_evals, int n_state, int n_vel, WS& ws, DecBufs& d) {
    const mtts_config& g = c->cfg;
    d.B = B; d.T = T; d.nl = g.dec_levels;
    if (T % (1 << (d.nl - 1))) { set_error("T must be a multiple of 2^(levels-1) (reference utils/model.py:15-21)"); return -1; }
    int cmax = 0;
    for (int i = 0; i < d.nl; ++i) cmax = std::max(cmax, g.dec_channels[i]);
    const int inner = g.dec_heads * g.dec_head_dim;
    const size_t M0 = (size_t)B * T;
    d.p16 = p16_decoder(c);
    d.ew = (d.p16 && c->half16) ? 1 : 2;
    d.Tl.resize(d.nl);
    d.mask.resize(d.nl); d.bufA.resize(d.nl); d.bufB.resize(d.nl); d.skip.resize(d.nl);
    (void)ws.bytes(256);                 // header: the call's range flag (begin_call)
    d.pair_flag = static_cast<unsigned int*>(ws.bytes(2048));
    d.nrows.resize(d.nl); d.nextra.resize(d.nl); d.kbias.resize(d.nl);
    for (int l = 0; l < d.nl; ++l) {
        d.Tl[l] = T >> l;
        const size_t Ml = (size_t)B * d.Tl[l];
        d.mask[l] = ws.f(Ml);
        d.kbias[l] = ws.f(Ml);
        d.nrows[l] = reinterpret_cast<int*>(ws.f(B));
        d.nextra[l] = reinterpret_cast<int*>(ws.f(B));
        d.bufA[l] = ws.f(Ml * cmax);
        d.bufB[l] = ws.f(Ml * cmax);
        d.skip[l] = ws.f(Ml * cmax);
    }
    d.Y = ws.f(M0 * cmax); d.H = ws.f(M0 * cmax); d.Rr = ws.f(M0 * cmax);
    d.QKV = ws.f(M0 * 3 * inner); d.ATT = ws.f(M0 * inner); d.FF = ws.f(M0 * 4 * cmax);
    d.mean = ws.f(M0); d.rstd = ws.f(M0);
    d.lnp = ws.f(M0 * (size_t)((cmax + 63) / 64) * 2);
    if (d.p16) {
        d.X = ws.f(M0 * round_up(cmax, 32));
        d.XM = ws.f(M0 * round_up(2 * g.n_feats, 64));
        d.gns = ws.f((M0 / 32 + 2) * 2 * (size_t)((cmax + 63) / 64) * 8);
    }
    d.gnp = ws.f((size_t)B * gn_chunks_max(T) * 8 * 2);
    d.ldx = round_up(2 * g.n_feats, c->half16 ? 64 : GEMM_BK);
    d.ldv = round_up(g.n_feats, 4);
    d.xmu = ws.f(M0 * d.ldx);
    if (n_state > 1) d.xmu2 = ws.f(M0 * d.ldx);
    for (int i = 0; i < n_vel; ++i) d.vel[i] = ws.f(M0 * d.ldv);
    const int temb = g.dec_channels[0] * 4;
    d.TS = ws.f((size_t)max_evals * 2 * g.n_feats);
    d.T1 = ws.f((size_t)max_evals * temb); d.T2 = ws.f((size_t)max_evals * temb); d.T3 = ws.f((size_t)max_evals * temb);
    d.TB = ws.f((size_t)max_evals * c->dec.tb_total);
    d.step_tv = ws.f((size_t)4 * B); d.step_dt = ws.f(B);
    d.rs_full = ws.f(M0); d.rs_half = ws.f(M0);
    return 0;
}

// SinusoidalPosEmb + TimestepEmbedding + every ResNet's Linear(Mish(t)) for all evaluation times at once
// (reference decoder.py:14-29,107-119,51,60): they depend on t only, so the whole ODE grid is done before the loop.
// tv == null: the nt times are d_tv in device memory (one per stage and utterance of a solver step).
static int time_embed(mtts_ctx* c, DecBufs& d, const TimeVals* tv, const float* d_tv, int nt, hipStream_t s) {
    const mtts_config& g = c->cfg;
    const DecW& D = c->dec;
    const int cin0 = 2 * g.n_feats, temb = g.dec_channels[0] * 4;
    if (tv) LAUNCH(c, 2, 0, s, launch_time_sinusoid(W(c, D.freqs.off), *tv, nt, cin0 / 2, 1000.0f, d.TS, s));
    else LAUNCH(c, 2, 0, s, launch_time_sinusoid_dev(W(c, D.freqs.off), d_tv, nt, cin0 / 2, 1000.0f, d.TS, s));
    GemmArgs a;
    panel_args(c, D.t1, a); rows_plain(a, nt, 1);
    a.a0 = d.TS; a.lda0 = cin0; a.c0 = cin0; a.act = ACT_SILU; a.out = d.T1; a.ldc = temb;
    RET_IF(run_gemm(c, a, s));
    GemmArgs b;
    panel_args(c, D.t2, b); rows_plain(b, nt, 1);
    b.a0 = d.T1; b.lda0 = temb; b.c0 = temb; b.out = d.T2; b.ldc = temb;
    RET_IF(run_gemm(c, b, s));
    LAUNCH(c, 2, 0, s, launch_unary(d.T2, d.T3, (int64_t)nt * temb, 1, s));
    GemmArgs m;
    panel_args(c, D.tmlp, m); rows_plain(m, nt, 1);
    m.a0 = d.T3; m.lda0 = temb; m.c0 = temb; m.out = d.TB; m.ldc = D.tb_total;
    RET_IF(run_gemm(c, m, s));
    return 0;
}

// An activation between two launches: c channels per row at p, in the representation of the call's flow (rows of ld floats, or
// an image with rows of ld halves), and the frame mask of its level when the reference multiplies by it before a conv reads the
// activation (null: not masked there, or already masked by its producer's own arithmetic in both flows).
struct Actv {
    const void* p = nullptr;
    int ld = 0, c = 0;
    const float* mask = nullptr;
};
static Actv actv(const DecBufs& d, const float* slot, int c, const float* mask = nullptr) {
    return Actv{slot, d.p16 ? d.ew * c : c, c, mask};
}
static _Float16* image(float* slot) { return reinterpret_cast<_Float16*>(slot); }

// The bind helpers below are the only place that knows the two representations and who multiplies by the frame mask: fp32 rows
// are stored unmasked and the GEMM that reads them multiplies (a_mask); an image goes into the consumer's tiles by LDS-DMA as it
// is, so its producer stores it masked (out16_mask).  Both use the mask of the activation's own level.
static void bind_in(const DecBufs& d, GemmArgs& a, int seg, const Actv& x) {       // x as input segment 0 / 1
    if (d.p16) {
        (seg ? a.a16_1 : a.a16_0) = static_cast<const _Float16*>(x.p);
        (seg ? a.lda16_1 : a.lda16_0) = x.ld;
    } else {
        (seg ? a.a1 : a.a0) = static_cast<const float*>(x.p);
        (seg ? a.lda1 : a.lda0) = x.ld;
        if (x.mask) a.a_mask = x.mask;
    }
    (seg ? a.c1 : a.c0) = x.c;
}
// lscale: residual scale of an image (GemmArgs::out_lscale)
static void bind_out(const DecBufs& d, GemmArgs& a, float* slot, int c, const float* mask = nullptr, float lscale = 2048.0f) {
    if (d.p16) { a.out16 = image(slot); a.ld16 = d.ew * c; a.out16_mask = mask; a.out_lscale = lscale; }
    else { a.out = slot; a.ldc = c; }
}
static void bind_out(const DecBufs& d, GnApplyArgs& g, float* slot, int c) {
    if (d.p16) { g.out16 = image(slot); g.ld16 = d.ew * c; }
    else g.out = slot;
}
static void bind_res(const DecBufs& d, GemmArgs& a, float* slot, int c) {     // residual of the epilogue
    if (d.p16) { a.res16 = image(slot); a.ldr16 = d.ew * c; }
    else { a.res = slot; a.ldr = c; }
}
static void bind_attn(const DecBufs& d, AttnArgs& at, float* qkv, float* out, int inner) {
    if (d.p16) { at.qkv16 = image(qkv); at.ld16 = 3 * d.ew * inner; at.out16 = image(out); at.ldo16 = d.ew * inner; }
    else { at.qkv = qkv; at.out = out; }
}
// The ODE state xin [B*T, ldx] = x | mu as the first ResNet's input: it sees x * mask (reference decoder.py:379).  fp32 rows are
// read in place; the image flow converts them once per evaluation (masked x | mu | zero padding up to the conv's K).
static int bind_state(mtts_ctx* c, DecBufs& d, const float* xin, Actv& x, hipStream_t s) {
    const int nf2 = 2 * c->cfg.n_feats;
    x = Actv{xin, d.ldx, nf2, d.mask[0]};
    if (!d.p16) return 0;
    if (c->dec.res[0].conv1.ktap != d.ldx) { set_error("P16 decoder: unexpected ResNet input width"); return -1; }
    LAUNCH(c, 2, 0, s, launch_to_p16(xin, d.ldx, d.mask[0], d.B * d.T, d.ldx, nf2, image(d.XM), d.ew * d.ldx, 2048.0f, s, c->cur_flag, d.ew == 1, d.ew == 1 && c->bf16));
    x = actv(d, d.XM, d.ldx);
    return 0;
}

// GroupNorm statistics from the conv GEMM's epilogue instead of a gn_partial pass over its output (gemm_epilogue.h): entries per
// wave tile and utterance part, so an utterance must be at least one wave tile long, and groups of >= 32 channels.
// Returns the wave-tile height (the consumers' tile_rows) or 0.
static int gn_fuse_rows(const GemmArgs& a, int C, int G, int T) {
    if (!a.a16_0 || a.fast16 || (C % 64) || (C % G) || (C / G) < 32 || ((C / G) & 7)) return 0;
    const int rows = gemm_p16_wave_rows(a);
    return T >= rows ? rows : 0;
}

// A Block1D's conv (input already bound) into the fp32 rows Y, and the GroupNorm statistics of Y: from the conv's epilogue when
// gn_fuse_rows allows (g.tile_rows != 0 then), else by a pass over Y.  Fills everything of the gn_apply that follows except its
// time bias, residual and output.
static int conv_gn_stats(mtts_ctx* c, DecBufs& d, GemmArgs& a, int lvl, const Vec& gamma, const Vec& beta, const Vec& bias_stats,
                         GnApplyArgs& g, hipStream_t s) {
    const int B = a.B, T = a.T_out, C = a.N;
    a.out = d.Y; a.ldc = C;
    const int fr = gn_fuse_rows(a, C, 8, T);
    if (fr) { a.gn_stats = d.gns; a.gn_groups = 8; a.gn_nrows = d.nr(lvl); g.tile_stats = d.gns; g.tile_rows = fr; }
    RET_IF(run_gemm(c, a, s));
    if (!fr) LAUNCH(c, 2, 0, s, launch_gn_partial(d.Y, B, T, C, 8, d.gnp, s, d.nr(lvl)));
    g.y = d.Y; g.partial = d.gnp; g.gamma = W(c, gamma.off); g.beta = W(c, beta.off); g.mask = d.mask[lvl]; g.nrows = d.nr(lvl);
    if (d.folded) { g.nextra = d.ne(lvl); g.bias_stats = W(c, bias_stats.off); }
    g.B = B; g.T = T; g.C = C;
    return 0;
}

// Where the one-launch Block1D pays (measured): its grid is 8 B workgroups of one per CU, so it needs a batch
// that fills the chip's CUs once -- at B = 64 (two rounds) the tiled launches win by 0.5-1.0 ms per step -- and not much less: the
// short form (<= 192 rows) from half the chip (B = 16: -0.35 ms), the long form only near a full chip (B = 16: +0.35 ms, B = 32:
// -0.5 ms).  Bit 2 of MTTS_RESNET_FUSE lifts the batch gate (tests run small batches).
static bool block1d_fusable(const mtts_ctx* c, const DecBufs& d, int T, int C) {
    if (!d.p16 || c->half_now || c->fast16 || !conv_gn_supported(T, C)) return false;
    if (c->sw.resnet_fuse & 4) return true;
    const int wgs = 8 * d.B;
    return wgs <= CHIP_CUS && wgs >= (T <= CONV_GN_SPLIT_ROWS ? 128 : 192);
}

// A Block1D as one launch (resnet_conv.hip): the conv `a` (input and panel already bound) -> GroupNorm -> Mish -> mask [-> + chbias
// -> mask] into the image slot `dst`.
static int block1d_fused(mtts_ctx* c, DecBufs& d, const GemmArgs& a, int lvl, const Vec& gamma, const Vec& beta, const Vec& bias_stats,
                         const float* chbias, float* dst, hipStream_t s) {
    ConvGnArgs f;
    f.a16_0 = a.a16_0; f.lda16_0 = a.lda16_0; f.c0 = a.c0;
    f.a16_1 = a.a16_1; f.lda16_1 = a.lda16_1; f.c1 = a.c1;
    f.w16 = a.w16; f.bias = a.bias; f.B = a.B; f.T = a.T_out; f.N = a.N;
    f.gamma = W(c, gamma.off); f.beta = W(c, beta.off); f.mask = d.mask[lvl]; f.chbias = chbias; f.chbias_stride = d.tb_stride; f.nrows = d.nr(lvl);
    if (d.folded) { f.nextra = d.ne(lvl); f.bias_stats = W(c, bias_stats.off); }
    f.out16 = image(dst); f.ld16 = d.ew * a.N;
    return run_conv_gn(c, f, s);
}

// ResnetBlock1D.forward (reference decoder.py:58-63) on channels-last rows; input = up to two channel segments (in1.p null: one).
// The output is the residual stream of the transformer blocks that follow, d.stream(dst); emit_stats: with its LayerNorm moments.
static int resnet_block(mtts_ctx* c, DecBufs& d, const ResnetW& r, const Actv& in0, const Actv& in1, int lvl, const float* tbias,
                        float* dst, bool emit_stats, hipStream_t s) {
    const int B = d.B, T = d.Tl[lvl], C = r.cout;
    float* x = d.stream(dst);
    GemmArgs a;
    panel_args(c, r.conv1, a); rows_plain(a, B, T); taps_centered(a, 3);
    bind_in(d, a, 0, in0);
    if (in1.p) bind_in(d, a, 1, in1);
    const bool fusable = block1d_fusable(c, d, T, C);
    if (fusable && (c->sw.resnet_fuse & 1)) {
        // the first Block1D as ONE launch (resnet_conv.hip): a workgroup per (utterance, GroupNorm group) owns its statistics, so
        // neither the conv's fp32 rows nor a gn_apply pass exist.  Width 384 at 65..384 rows per utterance (both levels of the
        // benchmark shape); every other shape keeps the launches below.
        RET_IF(block1d_fused(c, d, a, lvl, r.gn1_g, r.gn1_b, r.gn1_bs, tbias, d.H, s));
    } else {
        GnApplyArgs g1;
        RET_IF(conv_gn_stats(c, d, a, lvl, r.gn1_g, r.gn1_b, r.gn1_bs, g1, s));
        g1.chbias = tbias; g1.chbias_stride = d.tb_stride;
        bind_out(d, g1, d.H, C);
        RET_IF(run_gn_apply(c, g1, s));
    }
    GemmArgs b;
    panel_args(c, r.conv2, b); rows_plain(b, B, T); taps_centered(b, 3);
    bind_in(d, b, 0, actv(d, d.H, C));
    GemmArgs rc;
    panel_args(c, r.res, rc); rows_plain(rc, B, T);
    bind_in(d, rc, 0, in0);
    if (in1.p) bind_in(d, rc, 1, in1);
    if (fusable && (c->sw.resnet_fuse & 2)) {
        // the second Block1D the same way, its masked result as an image in the slot the conv's fp32 rows would take; the 1x1
        // residual conv adds it as its image residual and leaves x with its LayerNorm moments: no fp32 rows, no statistics
        // entries to merge in the residual conv's prologue
        RET_IF(block1d_fused(c, d, b, lvl, r.gn2_g, r.gn2_b, r.gn2_bs, nullptr, d.Y, s));
        bind_res(d, rc, d.Y, C);
        bind_out(d, rc, x, C);
        if (emit_stats && (C % 64) == 0) rc.stats_out = d.lnp;
        RET_IF(run_gemm(c, rc, s));
        return 0;
    }
    GnApplyArgs g2;
    RET_IF(conv_gn_stats(c, d, b, lvl, r.gn2_g, r.gn2_b, r.gn2_bs, g2, s));
    if (g2.tile_rows && T >= 2 * gemm_p16_wave_rows(rc)) {      // a workgroup's rows in at most two utterances
        // The 1x1 residual conv finishes the block: its epilogue adds Mish(GroupNorm(conv2 output)) * mask from the tile
        // statistics conv2 left, and writes x's image + LayerNorm moments -- no gn_apply pass, no residual round trip.
        rc.gnr_y = d.Y; rc.gnr_stats = d.gns; rc.gnr_tile_rows = g2.tile_rows; rc.gnr_groups = 8;
        rc.gnr_gamma = g2.gamma; rc.gnr_beta = g2.beta; rc.gnr_mask = g2.mask;
        rc.gnr_nextra = g2.nextra; rc.gnr_bias_stats = g2.bias_stats;
        bind_out(d, rc, x, C);
        rc.stats_out = d.lnp;
        RET_IF(run_gemm(c, rc, s));
        return 0;
    }
    rc.out = d.Rr; rc.ldc = C;
    RET_IF(run_gemm(c, rc, s));
    g2.res = d.Rr; g2.ldr = C;
    bind_out(d, g2, x, C);
    if (emit_stats && (C % 64) == 0) g2.stats_out = d.lnp;       // for the first transformer block's LayerNorm
    RET_IF(run_gn_apply(c, g2, s));
    return 0;
}

// BasicTransformerBlock.forward (reference transformer.py:230-303, self-attention only), in place on the residual stream
// x = d.stream(dst) [B*T, C].  LayerNorm statistics travel with the data: the launch that writes x (the ResNet block's last one,
// the attention out-projection, the second FF projection) leaves per-row partial moments of its 64-column slices behind
// (stats_out) and the next projection merges them in its prologue.  A width that is not a multiple of 64 has no such slices:
// the row_stats kernel runs in front of each LayerNorm'd projection instead.
// emit_stats: another block of the run follows; the last block's last launch leaves the run's result in dst.
static int transformer_block(mtts_ctx* c, DecBufs& d, const TBlockW& t, int C, int lvl, bool emit_stats, float* dst, hipStream_t s) {
    const mtts_config& g = c->cfg;
    const int B = d.B, T = d.Tl[lvl], M = B * T, inner = g.dec_heads * g.dec_head_dim;
    const bool fuse = (C % 64) == 0;
    float* x = d.stream(dst);
    auto layernorm_in = [&](GemmArgs& p) -> int {       // p reads LayerNorm(x) (the affine is folded into its panel)
        bind_in(d, p, 0, actv(d, x, C));
        if (fuse) { p.a_part = d.lnp; p.a_nparts = C / 64; return 0; }
        LAUNCH(c, 2, 0, s, launch_row_stats(x, M, C, C, 1e-5f, d.mean, d.rstd, s));
        p.a_mean = d.mean; p.a_rstd = d.rstd;
        return 0;
    };
    // the row-local part as one launch (tblock_chain.hip), in its single-workgroup or its pair form, or as the tiled launches below:
    // tblock_plan decides from the row count and the switches; here only what this call can use of the block's packed streams
    const bool p16_streams = t.chain_frags > 0 && !t.chain_h16 && d.p16 && !c->half_now && (emit_stats ? t.chain_nqkv > 0 : true);
    const TBlockPlan plan = tblock_plan(c->sw, C, inner, t.chain_nqkv, t.chain_ch, M, p16_streams,
                                        p16_streams && t.chain_pair_frags > 0 && d.pair_flag != nullptr);
    // 16-bit storage modes: the one-plane chain (tblock_chain_h16.hip) from chain16_min_rows rows on; below, the four tiled launches
    const bool chain16 = t.chain_frags > 0 && t.chain_h16 && d.p16 && c->half_now && d.ew == 1 && M >= c->sw.chain16_min_rows &&
                         (emit_stats ? t.chain_nqkv > 0 : true);
    if (!d.qkv_ready) {
        GemmArgs q;
        panel_args(c, t.qkv, q); rows_plain(q, B, T);
        RET_IF(layernorm_in(q));
        bind_out(d, q, d.QKV, 3 * inner, nullptr, 1.0f);      // (the attention kernel reads unscaled residuals)
        RET_IF(run_gemm(c, q, s));
    }
    d.qkv_ready = false;
    AttnArgs at;
    bind_attn(d, at, d.QKV, d.ATT, inner);
    at.mask = d.kb(lvl); at.B = B; at.T = T; at.H = g.dec_heads; at.D = g.dec_head_dim;
    at.scale = 1.0f / sqrtf((float)g.dec_head_dim); at.mask_mode = 0; at.klen = d.nr(lvl); at.fast16 = c->fast16;
    RET_IF(run_attn(c, at, s));
    // what both chain launches take (kernels.h ChainArgs / ChainH16Args), ew halves per image element
    auto bind_chain = [&](auto& a, int ew) {
        a.M = M; a.C = C; a.inner = inner;
        a.att16 = image(d.ATT); a.ld_att = ew * inner;
        a.x16 = image(x); a.ld_x = ew * C;
        a.wstream = static_cast<decltype(a.wstream)>(static_cast<const void*>(W(c, t.chain))); a.stream_frags = t.chain_frags;
        a.consts = W(c, t.chain_consts);
        a.ld_out = ew * C;
        if (emit_stats) {                 // another block follows: its q|k|v leaves this launch, x stays unmasked
            const TBlockW& nx = c->dec.tb[t.next];
            a.b_qkv = W(c, nx.qkv.b); a.wsum_qkv = W(c, nx.qkv.wsum); a.n_qkv = nx.qkv.N;
            a.qkv16 = image(d.QKV); a.ld_qkv = ew * nx.qkv.N;
            a.x_out = image(x);
            d.qkv_ready = true;
        } else { a.x_out = image(dst); a.x_out_mask = d.mask[lvl]; }
        a.ch = t.chain_ch;
    };
    if (chain16) {                        // (image flow, H16: one 2-byte value per channel)
        ChainH16Args a;
        bind_chain(a, 1);
        a.bf16 = c->bf16;
        return run_chain_h16(c, a, s);
    }
    if (plan.form) {                      // (image flow, P16: rows of 2 halves per channel)
        ChainArgs a;
        bind_chain(a, 2);
        a.qb = plan.qb; a.pf_wgs = plan.pf;
        if (plan.form == 2) {
            a.pair = 1;
            a.wstream = reinterpret_cast<const _Float16*>(W(c, t.chain_pair)); a.stream_frags = t.chain_pair_frags;
            a.pair_part = d.FF;              // (the tiled path's hidden image: unused by a chain launch)
            a.pair_flag = d.pair_flag;
            a.pair_epoch = ++c->pair_epoch;
            if (c->pair_epoch == 0) a.pair_epoch = ++c->pair_epoch;
        }
        return run_chain(c, a, s);
    }
    GemmArgs o;
    panel_args(c, t.out, o); rows_plain(o, B, T);
    bind_in(d, o, 0, actv(d, d.ATT, inner));
    bind_res(d, o, x, C);
    bind_out(d, o, x, C);
    if (fuse) o.stats_out = d.lnp;
    RET_IF(run_gemm(c, o, s));
    GemmArgs f1;
    panel_args(c, t.ff1, f1); rows_plain(f1, B, T);
    RET_IF(layernorm_in(f1));
    f1.act = ACT_SNAKE; f1.p0 = W(c, t.alpha_exp.off); f1.p1 = W(c, t.inv_beta.off);
    bind_out(d, f1, d.FF, 4 * C);
    RET_IF(run_gemm(c, f1, s));
    GemmArgs f2;
    panel_args(c, t.ff2, f2); rows_plain(f2, B, T);
    bind_in(d, f2, 0, actv(d, d.FF, 4 * C));
    bind_res(d, f2, x, C);
    if (emit_stats) {
        bind_out(d, f2, x, C);
        if (fuse) f2.stats_out = d.lnp;
    } else bind_out(d, f2, dst, C, d.mask[lvl]);
    RET_IF(run_gemm(c, f2, s));
    return 0;
}

struct FinalOut {   // where the masked velocity goes: out = v * scale (+ res)
    float* out; int ldc; const float* res; int ldr; float scale;
    const float* row_scale = nullptr;   // [B*T] mask[row] * scale of the row's utterance instead of mask and scale (one dt per utterance)
};

// Decoder.forward (reference decoder.py:359-426) for evaluation `ev` (row of the precomputed time biases; with one time per
// utterance, d.tb_stride != 0, the row of utterance 0).
// xin: channels-last state [B*T, ldx] holding x | mu.
static int unet_eval(mtts_ctx* c, DecBufs& d, const float* xin, int ev, const FinalOut& fo, hipStream_t s) {
    const mtts_config& g = c->cfg;
    const DecW& D = c->dec;
    const int nl = d.nl, nb = g.dec_n_blocks, B = d.B;
    const float* tb = d.TB + (size_t)ev * D.tb_total;
    size_t ri = 0, ti = 0;
    Actv cur;
    RET_IF(bind_state(c, d, xin, cur, s));
    auto other = [&](const Actv& x, int l) { return x.p == d.bufA[l] ? d.bufB[l] : d.bufA[l]; };
    // ---- down path
    for (int l = 0; l < nl; ++l) {
        const ResnetW& r = D.res[ri++];
        RET_IF(resnet_block(c, d, r, cur, Actv(), l, tb + r.tb_off, d.skip[l], nb > 0, s));
        for (int j = 0; j < nb; ++j) RET_IF(transformer_block(c, d, D.tb[ti++], r.cout, l, j + 1 < nb, d.skip[l], s));
        GemmArgs a;
        panel_args(c, D.down[l], a);
        taps_centered(a, 3);
        bind_in(d, a, 0, actv(d, d.skip[l], r.cout, d.mask[l]));
        a.B = B; a.T_in = d.Tl[l];
        const int lo = l < nl - 1 ? l + 1 : l;
        if (l < nl - 1) { a.T_out = d.Tl[lo]; a.in_stride = 2; a.out_T = d.Tl[lo]; }      // Downsample1D: Conv1d(k3, s2, p1) (reference decoder.py:66-72)
        else { a.T_out = d.Tl[l]; a.out_T = d.Tl[l]; }                                    // last level: Conv1d(k3, p1) (reference decoder.py:252-254)
        bind_out(d, a, d.bufA[lo], r.cout, d.mask[lo]);
        RET_IF(run_gemm(c, a, s));
        cur = actv(d, d.bufA[lo], r.cout, d.mask[lo]);
    }
    // ---- mid blocks at the coarsest level
    const int lm = nl - 1;
    for (int i = 0; i < g.dec_mid_blocks; ++i) {
        const ResnetW& r = D.res[ri++];
        float* dst = other(cur, lm);
        RET_IF(resnet_block(c, d, r, cur, Actv(), lm, tb + r.tb_off, dst, nb > 0, s));
        for (int j = 0; j < nb; ++j) RET_IF(transformer_block(c, d, D.tb[ti++], r.cout, lm, j + 1 < nb, dst, s));
        cur = actv(d, dst, r.cout, d.mask[lm]);
    }
    // ---- up path
    for (int i = 0; i < nl; ++i) {
        const int l = nl - 1 - i;
        const ResnetW& r = D.res[ri++];
        float* dst = other(cur, l);
        RET_IF(resnet_block(c, d, r, cur, actv(d, d.skip[l], g.dec_channels[l], d.mask[l]), l, tb + r.tb_off, dst, nb > 0, s));
        for (int j = 0; j < nb; ++j) RET_IF(transformer_block(c, d, D.tb[ti++], r.cout, l, j + 1 < nb, dst, s));
        cur = actv(d, dst, r.cout, d.mask[l]);
        if (i < nl - 1) {   // Upsample1D: ConvTranspose1d(k4, s2, p1) as two phase GEMMs (reference decoder.py:146)
            for (int ph = 0; ph < 2; ++ph) {
                GemmArgs a;
                panel_args(c, ph == 0 ? D.up_even[i] : D.up_odd[i], a);
                bind_in(d, a, 0, cur);
                a.B = B; a.T_in = d.Tl[l]; a.T_out = d.Tl[l]; a.in_stride = 1;
                a.tap_off[0] = ph == 0 ? 0 : 1;
                a.tap_off[1] = ph == 0 ? -1 : 0;
                bind_out(d, a, d.bufA[l - 1], r.cout, d.mask[l - 1]);
                a.out_T = d.Tl[l - 1]; a.out_stride = 2; a.out_off = ph;
                RET_IF(run_gemm(c, a, s));
            }
            cur = actv(d, d.bufA[l - 1], r.cout, d.mask[l - 1]);
        } else {
            GemmArgs a;
            panel_args(c, D.up_last, a); rows_plain(a, B, d.Tl[l]); taps_centered(a, 3);
            bind_in(d, a, 0, cur);
            float* o2 = other(cur, l);
            bind_out(d, a, o2, r.cout, d.mask[l]);
            RET_IF(run_gemm(c, a, s));
            cur = actv(d, o2, r.cout, d.mask[l]);
        }
    }
    // ---- final Block1D + 1x1 projection + mask (reference decoder.py:423-426)
    const int C0 = g.dec_channels[0], T = d.T;
    GemmArgs a;
    panel_args(c, D.final_conv, a); rows_plain(a, B, T); taps_centered(a, 3);
    bind_in(d, a, 0, cur);
    if ((c->sw.resnet_fuse & 1) && block1d_fusable(c, d, T, C0)) {
        RET_IF(block1d_fused(c, d, a, 0, D.fgn_g, D.fgn_b, D.fgn_bs, nullptr, d.H, s));
    } else {
        GnApplyArgs ga;
        RET_IF(conv_gn_stats(c, d, a, 0, D.fgn_g, D.fgn_b, D.fgn_bs, ga, s));
        bind_out(d, ga, d.H, C0);
        RET_IF(run_gn_apply(c, ga, s));
    }
    GemmArgs p;
    panel_args(c, D.final_proj, p); rows_plain(p, B, T);
    bind_in(d, p, 0, actv(d, d.H, C0));
    p.out_mask = fo.row_scale ? fo.row_scale : d.mask[0];
    p.out = fo.out; p.ldc = fo.ldc; p.res = fo.res; p.ldr = fo.ldr; p.out_scale = fo.row_scale ? 1.0f : fo.scale;
    RET_IF(run_gemm(c, p, s));
    return 0;
}
static int decoder_eval(mtts_ctx* c, DecBufs& d, const float* xin, int ev, const FinalOut& fo, hipStream_t s) {
    c->half_now = d.ew == 1;          // 16-bit storage mode: the estimator's images are H16 (kernels.h GemmArgs::half16)
    const int r = unet_eval(c, d, xin, ev, fo, s);
    c->half_now = false;
    return r;
}

// Level masks and frame tables of one call.  y_len == null: any float mask [B, T] (reference decoder.py:390 mask[:, :, ::2]),
// every utterance owns its T rows (or tlen[b] of them: per-request padding).  y_len != null: prefix masks of y_len[b] frames in
// the folded layout -- d.T rows per utterance stand for T_true reference frames (FrameTableArgs).
static int build_frames(mtts_ctx* c, DecBufs& d, const float* mask, const int64_t* y_len, int T_true, hipStream_t s) {
    d.T_true = T_true;
    d.folded = y_len != nullptr;
    d.tables = d.folded || c->d_tlen != nullptr;
    if (!d.folded)
        for (int l = 0; l < d.nl; ++l)
            LAUNCH(c, 2, 0, s, launch_mask_down(mask, d.B, d.T, 1 << l, d.mask[l], d.Tl[l], s));
    if (d.tables) {
        FrameTableArgs f;
        f.y_len = y_len; f.tlen = c->d_tlen; f.B = d.B; f.T_true = T_true; f.nl = d.nl;
        for (int l = 0; l < d.nl; ++l) {
            f.T[l] = d.Tl[l]; f.mask[l] = d.mask[l]; f.kbias[l] = d.kbias[l]; f.nrows[l] = d.nrows[l]; f.nextra[l] = d.nextra[l];
        }
        LAUNCH(c, 2, 0, s, launch_frame_tables(f, s));
    }
    return 0;
}

}  // namespace mtts

using namespace mtts;

extern "C" {

// ------------------------------------------------------------------------------------------------ decoder entry points
int64_t mtts_decoder_workspace_bytes(mtts_ctx* c, int B, int T) {
    if (!c || (!c->packed && pack_all(c))) return -1;
    WS ws(nullptr, 0);
    DecBufs d;
    if (plan_decoder(c, B, T, step_time_rows(B), 2, 4, ws, d)) return -1;
    return (int64_t)ws.off + 256;
}

int mtts_set_frame_limits(mtts_ctx* c, const int32_t* d_t_len) {
    if (!c) { set_error("null context"); return -1; }
    c->d_tlen = d_t_len;
    return 0;
}

// Decoder.forward with one time for the batch (d_t == null: t) or one per utterance (d_t: device fp32 [B]; the time embedding is
// made for B rows and every ResNet block adds its utterance's own bias row, as in mtts_cfm_step).
static int decoder_forward_core(mtts_ctx* c, const float* d_x, const float* d_mask, const float* d_mu, float t, const float* d_t, int B,
                                int T, float* d_out, void* d_ws, int64_t ws_bytes, void* stream) {
    CTX_GUARD(c);
    RET_IF(check_ready(c));
    hipStream_t s = static_cast<hipStream_t>(stream);
    WS ws(d_ws, (size_t)ws_bytes);
    DecBufs d;
    RET_IF(plan_decoder(c, B, T, step_time_rows(B), 2, 4, ws, d));
    if (ws.overflow) { set_error("decoder workspace too small"); return -1; }
    RET_IF(begin_call(c, d_ws, s));
    if (c->sw.pair_on) HIP_OK(launch_fill_cols(reinterpret_cast<float*>(d.pair_flag), 1, 512, 0, 512, 0.f, s));
    const int nf = c->cfg.n_feats;
    RET_IF(build_frames(c, d, d_mask, nullptr, T, s));
    LAUNCH(c, 2, 0, s, launch_fill_cols(d.xmu, B * T, d.ldx, 2 * nf, d.ldx - 2 * nf, 0.f, s));
    LAUNCH(c, 2, 0, s, launch_cf_to_cl(d_x, nullptr, B, nf, T, d.xmu, d.ldx, 0, s));
    LAUNCH(c, 2, 0, s, launch_cf_to_cl(d_mu, nullptr, B, nf, T, d.xmu, d.ldx, nf, s));
    if (d_t) {
        RET_IF(time_embed(c, d, nullptr, d_t, B, s));
        d.tb_stride = (int)c->dec.tb_total;
    } else {
        TimeVals tv;
        tv.t[0] = t;
        RET_IF(time_embed(c, d, &tv, nullptr, 1, s));
    }
    FinalOut fo{d.vel[0], d.ldv, nullptr, 0, 1.0f};
    RET_IF(decoder_eval(c, d, d.xmu, 0, fo, s));
    LAUNCH(c, 2, 0, s, launch_cl_to_cf(d.vel[0], d.ldv, B, nf, T, d_out, T, 1.0f, 0.0f, s));
    return 0;
}

int mtts_decoder_forward(mtts_ctx* c, const float* d_x, const float* d_mask, const float* d_mu, float t, int B, int T,
                         float* d_out, void* d_ws, int64_t ws_bytes, void* stream) {
    return decoder_forward_core(c, d_x, d_mask, d_mu, t, nullptr, B, T, d_out, d_ws, ws_bytes, stream);
}

int mtts_decoder_forward_rows(mtts_ctx* c, const float* d_x, const float* d_mask, const float* d_mu, const float* d_t, int B, int T,
                              float* d_out, void* d_ws, int64_t ws_bytes, void* stream) {
    if (!d_x || !d_mask || !d_mu || !d_t || !d_out || !d_ws) { set_error("mtts_decoder_forward_rows: null argument"); return -1; }
    if (B < 1 || T < 1) { set_error("mtts_decoder_forward_rows: need B >= 1 and T >= 1"); return -1; }
    return decoder_forward_core(c, d_x, d_mask, d_mu, 0.f, d_t, B, T, d_out, d_ws, ws_bytes, stream);
}

// BASECFM.compute_loss (reference flow_matching.py:65-107) without its two random draws: the flow-matching input as state rows
// (cfm_target_kernel), ONE estimator evaluation with utterance b at time d_t[b], and the masked squared error against
// u = x1 - (1 - sigma_min) x0 per utterance (cfm_loss_kernel; its partials borrow the conv scratch, idle once the estimator is done).
int mtts_cfm_loss(mtts_ctx* c, const float* d_x1, const float* d_mu, const float* d_mask, const float* d_noise, const float* d_t,
                  int add_mu, float sigma_min, int B, int T, float* d_sq_sum, float* d_pred, void* d_ws, int64_t ws_bytes, void* stream) {
    if (!d_x1 || !d_mu || !d_mask || !d_noise || !d_t || !d_sq_sum || !d_ws) { set_error("mtts_cfm_loss: null argument"); return -1; }
    if (B < 1 || T < 1) { set_error("mtts_cfm_loss: need B >= 1 and T >= 1"); return -1; }
    if (!(sigma_min >= 0.f) || !(sigma_min < 1.f)) { set_error("mtts_cfm_loss: sigma_min must be in [0, 1)"); return -1; }
    CTX_GUARD(c);
    RET_IF(check_ready(c));
    hipStream_t s = static_cast<hipStream_t>(stream);
    WS ws(d_ws, (size_t)ws_bytes);
    DecBufs d;
    RET_IF(plan_decoder(c, B, T, step_time_rows(B), 2, 4, ws, d));
    if (ws.overflow) { set_error("decoder workspace too small"); return -1; }
    RET_IF(begin_call(c, d_ws, s));
    if (c->sw.pair_on) HIP_OK(launch_fill_cols(reinterpret_cast<float*>(d.pair_flag), 1, 512, 0, 512, 0.f, s));
    const int nf = c->cfg.n_feats;
    const double elems = (double)B * T * nf;
    RET_IF(build_frames(c, d, d_mask, nullptr, T, s));
    LAUNCHB(c, 2, 0, 4.0 * (3.0 * elems + (double)B * T * d.ldx), s,
            launch_cfm_target(d_x1, d_noise, d_mu, d_t, add_mu, sigma_min, B, nf, T, d.xmu, d.ldx, s));
    RET_IF(time_embed(c, d, nullptr, d_t, B, s));
    d.tb_stride = (int)c->dec.tb_total;
    FinalOut fo{d.vel[0], d.ldv, nullptr, 0, 1.0f};
    RET_IF(decoder_eval(c, d, d.xmu, 0, fo, s));
    LAUNCHB(c, 2, 0, 4.0 * ((add_mu ? 3.0 : 2.0) * elems + (double)B * T * d.ldv + (d_pred ? elems : 0.0)), s,
            launch_cfm_loss(d.vel[0], d.ldv, d_x1, d_noise, d_mu, d_mask, add_mu, sigma_min, B, nf, T, d.Y, d_pred, s));
    LAUNCH(c, 2, 0, s, launch_cfm_loss_finish(d.Y, B, nf, T, d_sq_sum, s));
    return 0;
}

// BASECFM.solve (reference flow_matching.py:60-63) + torchdiffeq's fixed-grid loop.  The inputs are [B, n_feats, T_src]; the
// estimator holds T <= T_src rows per utterance (T < T_src: folded padding, y_len gives the prefix masks; else d_mask).
static int solve_core(mtts_ctx* c, const float* d_x0, const float* d_mu, const float* d_mask, const int64_t* d_y_len, int add_mu,
                      const float* h_t_span, int n_steps, int solver, int B, int T_src, int T, float* d_out, int T_out, float out_scale,
                      float out_shift, void* d_ws, int64_t ws_bytes, void* stream) {
    CTX_GUARD(c);
    RET_IF(check_ready(c));
    if (!h_t_span || n_steps < 1) { set_error("mtts_cfm_solve: bad time grid"); return -1; }
    const int stages = solver == MTTS_SOLVER_EULER ? 1 : solver == MTTS_SOLVER_MIDPOINT ? 2 : solver == MTTS_SOLVER_RK4 ? 4 : 0;
    if (!stages) { set_error("unsupported solver"); return -1; }
    if (n_steps * stages > MAX_EVALS) { set_error("too many function evaluations in one solve (max 256)"); return -1; }
    if (T_out > T) { set_error("mtts_cfm_solve: T_out exceeds the rows held per utterance"); return -1; }
    hipStream_t s = static_cast<hipStream_t>(stream);
    WS ws(d_ws, (size_t)ws_bytes);
    DecBufs d;
    RET_IF(plan_decoder(c, B, T, step_time_rows(B), 2, 4, ws, d));
    if (ws.overflow) { set_error("decoder workspace too small"); return -1; }
    RET_IF(begin_call(c, d_ws, s));
    if (c->sw.pair_on) HIP_OK(launch_fill_cols(reinterpret_cast<float*>(d.pair_flag), 1, 512, 0, 512, 0.f, s));
    const int nf = c->cfg.n_feats, M = B * T;
    RET_IF(build_frames(c, d, d_mask, d_y_len, T_src, s));
    // state rows: x | mu | zero pad.  z = mu + noise when use_mu_prior (reference flow_matching.py:52-55)
    float* states[2] = {d.xmu, d.xmu2};
    for (int k = 0; k < (stages > 1 ? 2 : 1); ++k) {
        LAUNCH(c, 2, 0, s, launch_fill_cols(states[k], M, d.ldx, 2 * nf, d.ldx - 2 * nf, 0.f, s));
        LAUNCH(c, 2, 0, s, launch_cf_to_cl(d_mu, nullptr, B, nf, T, states[k], d.ldx, nf, s, T_src));
    }
    LAUNCH(c, 2, 0, s, launch_cf_to_cl(d_x0, add_mu ? d_mu : nullptr, B, nf, T, d.xmu, d.ldx, 0, s, T_src));

    // evaluation times in torchdiffeq's fp32 arithmetic (fixed grid = t_span)
    TimeVals tv;
    int ne = 0;
    for (int i = 0; i < n_steps; ++i) {
        const float t0 = h_t_span[i], t1 = h_t_span[i + 1], dt = t1 - t0;
        if (solver == MTTS_SOLVER_EULER) tv.t[ne++] = t0;
        else if (solver == MTTS_SOLVER_MIDPOINT) { tv.t[ne++] = t0; tv.t[ne++] = t0 + 0.5f * dt; }
        else {
            const float third = 1.0f / 3.0f, two_thirds = 2.0f / 3.0f;
            tv.t[ne++] = t0; tv.t[ne++] = t0 + dt * third; tv.t[ne++] = t0 + dt * two_thirds; tv.t[ne++] = t1;
        }
    }
    RET_IF(time_embed(c, d, &tv, nullptr, ne, s));

    int ev = 0;
    for (int i = 0; i < n_steps; ++i) {
        const float dt = h_t_span[i + 1] - h_t_span[i];
        if (solver == MTTS_SOLVER_EULER) {             // y += dt * f(t0, y), fused into the last GEMM's epilogue
            FinalOut fo{d.xmu, d.ldx, d.xmu, d.ldx, dt};
            RET_IF(decoder_eval(c, d, d.xmu, ev++, fo, s));
        } else if (solver == MTTS_SOLVER_MIDPOINT) {   // y_mid = y + f(t0,y)*dt/2 ; y += dt * f(t0+dt/2, y_mid)
            FinalOut f1{d.xmu2, d.ldx, d.xmu, d.ldx, 0.5f * dt};
            RET_IF(decoder_eval(c, d, d.xmu, ev++, f1, s));
            FinalOut f2{d.xmu, d.ldx, d.xmu, d.ldx, dt};
            RET_IF(decoder_eval(c, d, d.xmu2, ev++, f2, s));
        } else {                                       // rk4, 3/8 rule
            for (int k = 0; k < 4; ++k) {
                FinalOut fk{d.vel[k], d.ldv, nullptr, 0, 1.0f};
                RET_IF(decoder_eval(c, d, k == 0 ? d.xmu : d.xmu2, ev++, fk, s));
                float* dst = k < 3 ? d.xmu2 : d.xmu;
                LAUNCH(c, 2, 0, s, launch_ode_combine(k + 1, dt, d.xmu, d.ldx, d.vel[0], d.vel[1], d.vel[2], d.vel[3], d.ldv, dst, d.ldx, M, nf, s));
            }
        }
    }
    LAUNCH(c, 2, 0, s, launch_cl_to_cf(d.xmu, d.ldx, B, nf, T, d_out, T_out, out_scale, out_shift, s));
    return 0;
}

int mtts_cfm_solve(mtts_ctx* c, const float* d_x0, const float* d_mu, const float* d_mask, int add_mu, const float* h_t_span,
                   int n_steps, int solver, int B, int T, float* d_out, int T_out, float out_scale, float out_shift, void* d_ws,
                   int64_t ws_bytes, void* stream) {
    if (!d_mask) { set_error("mtts_cfm_solve: null mask"); return -1; }
    return solve_core(c, d_x0, d_mu, d_mask, nullptr, add_mu, h_t_span, n_steps, solver, B, T, T, d_out, T_out, out_scale, out_shift,
                      d_ws, ws_bytes, stream);
}

int mtts_fold_rows(mtts_ctx* c, int y_max, int align) {
    if (!c || y_max < 1 || align < 1) { set_error("mtts_fold_rows: bad argument"); return -1; }
    const int f = 1 << (c->cfg.dec_levels - 1);
    return round_up((y_max + f - 1) / f + 1, align) * f;
}

int mtts_cfm_solve_folded(mtts_ctx* c, const float* d_x0, const float* d_mu, const int64_t* d_y_lengths, int y_max, int add_mu,
                          const float* h_t_span, int n_steps, int solver, int B, int T, int T_fold, float* d_out, int T_out,
                          float out_scale, float out_shift, void* d_ws, int64_t ws_bytes, void* stream) {
    if (!c || !d_y_lengths) { set_error("mtts_cfm_solve_folded: bad argument"); return -1; }
    if (T_fold > T || T_fold < mtts_fold_rows(c, y_max, 1)) {
        set_error("mtts_cfm_solve_folded: T_fold must hold ceil(y_max / 2^l) + 1 rows at every level and not exceed T (mtts_fold_rows)");
        return -1;
    }
    if (y_max >= T) { set_error("mtts_cfm_solve_folded: no padded frame to fold (y_max >= T)"); return -1; }
    if (T_fold % (1 << (c->cfg.dec_levels - 1))) {      // (plan_decoder halves the row count per level: a remainder would truncate)
        set_error("mtts_cfm_solve_folded: T_fold must be a multiple of 2^(levels-1) (mtts_fold_rows returns such counts)");
        return -1;
    }
    return solve_core(c, d_x0, d_mu, nullptr, d_y_lengths, add_mu, h_t_span, n_steps, solver, B, T, T_fold, d_out, T_out, out_scale,
                      out_shift, d_ws, ws_bytes, stream);
}

// One solver step of B utterances of a slot pool, each at its own point (t0, t1) of its own grid (include/mtts.h).  The sequence of
// solve_core for ONE grid interval, with what solve_core takes per call taken per utterance: the stage times (launch_step_tables ->
// time_embed on stages * B rows -> a bias row per utterance in every ResNet, DecBufs::tb_stride), dt (the final projection's row
// factors; ode_combine per utterance for rk4), and the state rows, which come from and return to the pool every step.
int mtts_cfm_step(mtts_ctx* c, float* d_z_pool, const float* d_mu_pool, int S, int T_cap, const int32_t* d_slots, const int32_t* h_slots,
                  const float* d_t0, const float* d_t1, const int64_t* d_y_lengths, int y_max, int solver, int B, int T_fold, void* d_ws,
                  int64_t ws_bytes, void* stream) {
    CTX_GUARD(c);
    RET_IF(check_ready(c));
    if (!d_z_pool || !d_mu_pool || !d_slots || !h_slots || !d_t0 || !d_t1 || !d_y_lengths || !d_ws) { set_error("mtts_cfm_step: null argument"); return -1; }
    const int stages = solver == MTTS_SOLVER_EULER ? 1 : solver == MTTS_SOLVER_MIDPOINT ? 2 : solver == MTTS_SOLVER_RK4 ? 4 : 0;
    if (!stages) { set_error("unsupported solver"); return -1; }
    if (S < 1 || T_cap < 1 || B < 1 || B > S) { set_error("mtts_cfm_step: need 1 <= B <= S slots of T_cap >= 1 frames"); return -1; }
    if (y_max < 1 || y_max > T_cap) { set_error("mtts_cfm_step: an utterance of y_max frames does not fit a slot of T_cap frames"); return -1; }
    if (T_fold > T_cap || T_fold < mtts_fold_rows(c, y_max, 1)) {
        set_error("mtts_cfm_step: T_fold must hold ceil(y_max / 2^l) + 1 rows at every level and not exceed T_cap (mtts_fold_rows)");
        return -1;
    }
    if (T_fold % (1 << (c->cfg.dec_levels - 1))) {
        set_error("mtts_cfm_step: T_fold must be a multiple of 2^(levels-1) (mtts_fold_rows returns such counts)");
        return -1;
    }
    {
        std::vector<char> taken((size_t)S, 0);
        for (int b = 0; b < B; ++b) {
            const int32_t sl = h_slots[b];
            if (sl < 0 || sl >= S) { set_error("mtts_cfm_step: slot index out of range"); return -1; }
            if (taken[sl]) { set_error("mtts_cfm_step: a slot appears twice in one step"); return -1; }
            taken[sl] = 1;
        }
    }
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int T = T_fold;
    WS ws(d_ws, (size_t)ws_bytes);
    DecBufs d;
    RET_IF(plan_decoder(c, B, T, step_time_rows(B), 2, 4, ws, d));
    if (ws.overflow) { set_error("decoder workspace too small"); return -1; }
    RET_IF(begin_call(c, d_ws, s));
    if (c->sw.pair_on) HIP_OK(launch_fill_cols(reinterpret_cast<float*>(d.pair_flag), 1, 512, 0, 512, 0.f, s));
    const int nf = c->cfg.n_feats, M = B * T;
    RET_IF(build_frames(c, d, nullptr, d_y_lengths, T_cap, s));
    float* states[2] = {d.xmu, d.xmu2};
    for (int k = 0; k < (stages > 1 ? 2 : 1); ++k) {
        LAUNCH(c, 2, 0, s, launch_fill_cols(states[k], M, d.ldx, 2 * nf, d.ldx - 2 * nf, 0.f, s));
        LAUNCH(c, 2, 0, s, launch_slots_to_cl(d_mu_pool, d_slots, S, T_cap, B, nf, T, states[k], d.ldx, nf, s));
    }
    LAUNCH(c, 2, 0, s, launch_slots_to_cl(d_z_pool, d_slots, S, T_cap, B, nf, T, d.xmu, d.ldx, 0, s));
    LAUNCH(c, 2, 0, s, launch_step_tables(d_t0, d_t1, d.mask[0], B, T, stages, d.step_tv, d.step_dt, d.rs_full, d.rs_half, s));
    RET_IF(time_embed(c, d, nullptr, d.step_tv, stages * B, s));
    d.tb_stride = (int)c->dec.tb_total;
    if (solver == MTTS_SOLVER_EULER) {
        FinalOut fo{d.xmu, d.ldx, d.xmu, d.ldx, 1.0f, d.rs_full};
        RET_IF(decoder_eval(c, d, d.xmu, 0, fo, s));
    } else if (solver == MTTS_SOLVER_MIDPOINT) {
        FinalOut f1{d.xmu2, d.ldx, d.xmu, d.ldx, 1.0f, d.rs_half};
        RET_IF(decoder_eval(c, d, d.xmu, 0, f1, s));
        FinalOut f2{d.xmu, d.ldx, d.xmu, d.ldx, 1.0f, d.rs_full};
        RET_IF(decoder_eval(c, d, d.xmu2, B, f2, s));
    } else {
        for (int k = 0; k < 4; ++k) {
            FinalOut fk{d.vel[k], d.ldv, nullptr, 0, 1.0f};
            RET_IF(decoder_eval(c, d, k == 0 ? d.xmu : d.xmu2, k * B, fk, s));
            float* dst = k < 3 ? d.xmu2 : d.xmu;
            LAUNCH(c, 2, 0, s, launch_ode_combine_rows(k + 1, d.step_dt, T, d.xmu, d.ldx, d.vel[0], d.vel[1], d.vel[2], d.vel[3], d.ldv, dst, d.ldx, M, nf, s));
        }
    }
    LAUNCH(c, 2, 0, s, launch_cl_to_slots(d.xmu, d.ldx, B, nf, T, d_z_pool, d_slots, S, T_cap, s));
    return 0;
}

}  // extern "C"
