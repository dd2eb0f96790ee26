// Host orchestration of the path on one HIP stream: weight packing, workspace planning and the launch sequences.
// No torch, no allocation or synchronisation inside the launch functions (graph-capturable).
#include "model.h"

#include <cmath>
#include <cstdlib>
#include <cstring>
#include <time.h>

namespace mtts {

static thread_local std::string g_err;
void set_error(const std::string& m) { g_err = m; }
const char* get_error() { return g_err.c_str(); }

// The only reader of the environment (model.h Switches).  A value outside a switch's domain leaves its default.
Switches read_switches() {
    Switches w;
    auto num = [](const char* name, int dflt) { const char* e = getenv(name); return e ? atoi(e) : dflt; };
    auto on = [](const char* name) { const char* e = getenv(name); return !(e && e[0] == '0'); };
    const int terms = num("MTTS_GEMM_TERMS", w.gemm_terms);
    if (terms == 0 || terms == 2 || terms == 3 || terms == 6) w.gemm_terms = terms;
    if (terms == 1 || terms == 16 || terms == 17) w.arith16 = terms;
    w.p16_on = on("MTTS_P16");
    w.chain_on = on("MTTS_CHAIN");
    if (num("MTTS_CHAIN_CH", w.chain_ch) == 128) w.chain_ch = 128;
    w.chain_qb = num("MTTS_CHAIN_QB", w.chain_qb);
    w.chain_min_rows = num("MTTS_CHAIN_MIN_ROWS", w.chain_min_rows);
    w.pair_on = on("MTTS_CHAIN_PAIR");
    w.pair_min_rows = num("MTTS_CHAIN_PAIR_MIN_ROWS", w.pair_min_rows);
    w.chain_pf = std::min(std::max(num("MTTS_CHAIN_PF", w.chain_pf), 0), 64);
    w.chain16_on = on("MTTS_CHAIN16");
    w.chain16_min_rows = num("MTTS_CHAIN16_MIN_ROWS", w.chain16_min_rows);
    { const int qb = num("MTTS_CHAIN16_QB", 0); if (qb == 32 || qb == 64 || qb == 96) w.chain16_qb = qb; }
    w.resnet_fuse = num("MTTS_RESNET_FUSE", w.resnet_fuse) & 7;
    return w;
}

#define HIP_OK(expr)                                                                        \
    do {                                                                                    \
        hipError_t _e = (expr);                                                             \
        if (_e != hipSuccess) {                                                             \
            set_error(std::string(#expr) + ": " + hipGetErrorString(_e));                   \
            return -1;                                                                      \
        }                                                                                   \
    } while (0)
#define RET_IF(expr)          \
    do {                      \
        int _r = (expr);      \
        if (_r) return _r;    \
    } while (0)

// ------------------------------------------------------------------------------------------------ profiling wrappers
static int prof_begin(mtts_ctx* c, int klass, double flops, double bytes, hipStream_t s) {
    if (!c || !c->prof_on) return 0;
    while (c->ev_pool.size() < c->ev_used + 2) {
        hipEvent_t e;
        HIP_OK(hipEventCreate(&e));
        c->ev_pool.push_back(e);
    }
    ProfRec r{c->ev_pool[c->ev_used], c->ev_pool[c->ev_used + 1], klass, flops, bytes, std::string()};
    g_kernel_tag = nullptr;
    c->ev_used += 2;
    HIP_OK(hipEventRecord(r.e0, s));
    c->prof.push_back(r);
    return 0;
}
static int prof_end(mtts_ctx* c, hipStream_t s) {
    if (!c || !c->prof_on) return 0;
    HIP_OK(hipEventRecord(c->prof.back().e1, s));
    c->prof.back().tag = g_kernel_tag ? g_kernel_tag : "";        // (set by the launcher that ran in between, or null)
    return 0;
}
#define LAUNCH(ctx, klass, flops, stream, call)  \
    LAUNCHB(ctx, klass, flops, 0.0, stream, call)
#define LAUNCHB(ctx, klass, flops, bytes, stream, call)  \
    do {                                         \
        RET_IF(prof_begin(ctx, klass, flops, bytes, stream)); \
        HIP_OK(call);                            \
        RET_IF(prof_end(ctx, stream));           \
    } while (0)

static int run_gemm(mtts_ctx* c, const GemmArgs& a0, hipStream_t s) {
    GemmArgs a = a0;
    a.range_flag = c->cur_flag;
    a.half16 = c->half_now && a.a16_0 != nullptr;
    a.bf16 = a.half16 && c->bf16;
    LAUNCHB(c, 0, gemm_flops(a), gemm_bytes(a), s, launch_gemm(a, s));
    return 0;
}
static int run_attn(mtts_ctx* c, const AttnArgs& a0, hipStream_t s) {
    AttnArgs a = a0;
    a.range_flag = c->cur_flag;
    a.half16 = c->half_now && a.qkv16 != nullptr;
    a.bf16 = a.half16 && c->bf16;
    LAUNCHB(c, 1, attn_flops(a), attn_bytes(a), s, launch_attention(a, s));
    return 0;
}
// Launch plan of a chain launch over M rows (hidden chunk ch; qb_forced = Switches::chain_qb or 0; want = Switches::chain_pf): rows
// per workgroup and prefetch workgroups.  32-row workgroups while they -- with the prefetchers -- are one round of the chip's CUs (a
// 32-row workgroup lives 99 us, a 48-row one 116 us: both are bound by the 7 MB they stream, profiles/r03_chain_prefetch_stamps.log),
// the largest shape beyond; no prefetchers when they would push a one-round grid into a second round.
static void chain_plan(int M, int ch, int qb_forced, int want, int* qb, int* pf) {
    const int qb_big = ch == 256 ? 48 : 64;
    const bool fits32 = (M + 31) / 32 + want <= CHIP_CUS;
    *qb = (qb_forced == 32 || qb_forced == qb_big) ? qb_forced : (fits32 ? 32 : qb_big);
    const int nwg = (M + *qb - 1) / *qb;
    *pf = want;
    if (nwg <= CHIP_CUS && nwg + *pf > CHIP_CUS) *pf = (want >= 8 && nwg + 8 <= CHIP_CUS) ? 8 : 0;
}
static int run_chain(mtts_ctx* c, const ChainArgs& a0, hipStream_t s) {
    ChainArgs a = a0;
    a.range_flag = c->cur_flag;
    { int qb_unused = 0; chain_plan(a.M, a.ch, a.qb, c->sw.chain_pf, &qb_unused, &a.pf_wgs); }
    if (a.pair) a.pf_wgs = c->sw.chain_pf ? 16 : 0;      // two per XCD, one per half (the model admits pair grids up to 240 workgroups)
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
    const int nwg = (M + *qb - 1) / *qb;
    *pf = want;
    if (nwg <= CHIP_CUS && nwg + *pf > CHIP_CUS) *pf = (want >= 8 && nwg + 8 <= CHIP_CUS) ? 8 : 0;
}
static int run_chain_h16(mtts_ctx* c, const ChainH16Args& a0, hipStream_t s) {
    ChainH16Args a = a0;
    a.range_flag = c->cur_flag;
    chain16_plan(a.M, a.C, a.ch, c->sw.chain16_qb, c->sw.chain_pf, &a.qb, &a.pf_wgs);
    LAUNCHB(c, 0, chain_h16_flops(a), chain_h16_bytes(a), s, launch_tblock_chain_h16(a, s));
    return 0;
}
static int run_gn_apply(mtts_ctx* c, const GnApplyArgs& a0, hipStream_t s) {
    GnApplyArgs a = a0;
    a.range_flag = c->cur_flag;
    a.half16 = c->half_now && a.out16 != nullptr;
    a.bf16 = a.half16 && c->bf16;
    LAUNCH(c, 2, 0, s, launch_gn_apply(a, s));
    return 0;
}
// The sticky range flag of a call = the first word of its workspace, cleared here (include/mtts.h "range guard").
static int run_conv_gn(mtts_ctx* c, const ConvGnArgs& a0, hipStream_t s) {
    ConvGnArgs a = a0;
    a.range_flag = c->cur_flag;
    LAUNCHB(c, 0, conv_gn_flops(a), conv_gn_bytes(a), s, launch_conv_gn(a, s));
    return 0;
}

static int begin_call(mtts_ctx* c, void* d_ws, hipStream_t s) {
    c->cur_flag = static_cast<unsigned int*>(d_ws);
    // a kernel, not hipMemsetAsync: a captured memset node of one HIP graph was seen to write another instantiated graph's
    // bytes (pointer-like words in this header) after a second context captured its own graph (ROCm 7.2); kernel nodes are safe
    HIP_OK(launch_fill_cols(static_cast<float*>(d_ws), 1, 64, 0, 64, 0.f, s));
    return 0;
}

// ------------------------------------------------------------------------------------------------ workspace
struct WS {
    char* base;
    size_t off = 0, cap;
    bool overflow = false;
    WS(void* p, size_t c) : base(static_cast<char*>(p)), cap(c) {}
    void* bytes(size_t n) {
        off = (off + 255) & ~size_t(255);
        void* r = base ? base + off : nullptr;
        off += n;
        if (base && off > cap) overflow = true;
        return r;
    }
    float* f(size_t n) { return static_cast<float*>(bytes(n * sizeof(float))); }
};

// ------------------------------------------------------------------------------------------------ weight packing
struct Packer {
    mtts_ctx* c;
    bool ok = true;
    std::string why;
    int kq = GEMM_BK;          // K padding per tap of the panels being packed: 64 for the estimator in the 16-bit storage mode
    bool h16 = false;          // ... which also get the single fp16 plane (Panel::wh16)
    bool dry = false;          // layout only: offsets and sizes are computed (the registered tensors are still checked for presence and
                               // shape), nothing but zeros is written: mtts_import_weights takes the image itself from a cache
    explicit Packer(mtts_ctx* ctx) : c(ctx) {}
    const std::vector<float>* get(const std::string& key, size_t numel) {
        auto it = c->raw.find(key);
        if (it == c->raw.end()) { fail("missing tensor " + key); return nullptr; }
        if (it->second.size() != numel) {
            fail("tensor " + key + " has " + std::to_string(it->second.size()) + " elements, expected " + std::to_string(numel));
            return nullptr;
        }
        return &it->second;
    }
    void fail(const std::string& m) { if (ok) { ok = false; why = m; } }
    size_t alloc(size_t n) {
        size_t off = (c->image.size() + 63) & ~size_t(63);
        c->image.resize(off + n, 0.f);
        return off;
    }
    Vec vec(const std::string& key, int n) {
        Vec v;
        const auto* t = get(key, n);
        if (!t) return v;
        v.off = alloc(n);
        v.n = n;
        if (!dry) std::memcpy(&c->image[v.off], t->data(), n * sizeof(float));
        return v;
    }
    // Folded padding (kernels.h GnApplyArgs::bias_stats): where every input tap of a conv is a masked (zero) frame its output
    // row is exactly the bias, so any number of such rows enters the following GroupNorm in closed form from, per group,
    // (mean of the bias, sum of squared deviations from that mean), computed here in double.
    Vec bias_group_stats(const Panel& p, int G) {
        Vec v;
        v.off = alloc(2 * G);
        v.n = 2 * G;
        if (dry) return v;
        const int cpg = p.N / G;
        for (int g = 0; g < G; ++g) {
            double m = 0.0, q = 0.0;
            for (int k = 0; k < cpg; ++k) m += p.has_bias ? (double)c->image[p.b + g * cpg + k] : 0.0;
            m /= cpg;
            for (int k = 0; k < cpg; ++k) { const double d = (p.has_bias ? (double)c->image[p.b + g * cpg + k] : 0.0) - m; q += d * d; }
            c->image[v.off + 2 * g] = (float)m;
            c->image[v.off + 2 * g + 1] = (float)q;
        }
        return v;
    }
    // kind 0 Linear [N,C]; 1 Conv1d [N,C,ntaps]; 2 ConvTranspose1d [C,N,kT] with taps tsel
    Panel panel(const std::string& wkey, const std::string& bkey, int kind, int N, int C, int ntaps, int kT = 0,
                const int* tsel = nullptr, const std::vector<float>* col_scale = nullptr,
                const std::vector<float>* col_shift = nullptr) {
        return panel_multi({wkey}, {bkey}, kind, N, C, ntaps, kT, tsel, col_scale, col_shift);
    }
    // bf16 split planes of a finished fp32 panel (split modes only)
    void add_planes(Panel& p) {
        if (c->gemm_terms == 0) return;
        const size_t n = (size_t)round_up(p.N, GEMM_BN) * p.ntaps * p.ktap;
        p.w16 = alloc((3 * n + 1) / 2);
        if (c->gemm_terms == 2) {
            for (size_t i = 0; i < n && !dry; ++i)
                if (std::fabs(c->image[p.w + i]) > 65504.f) { c->weights_saturate = true; break; }
            if (!dry) split_panel_f16_host(&c->image[p.w], n, reinterpret_cast<uint16_t*>(&c->image[p.w16]));
            const int Np = round_up(p.N, GEMM_BN);
            const size_t Kp = (size_t)p.ntaps * p.ktap;
            p.wsum = alloc(Np);
            if (h16) {            // 16-bit storage mode: the fp16 head plane alone + row sums of the ROUNDED weights (LN epilogue)
                p.wh16 = alloc((n + 1) / 2);
                if (!dry && c->bf16) panel_bf16_host(&c->image[p.w], n, reinterpret_cast<uint16_t*>(&c->image[p.wh16]));
                else if (!dry) panel_h16_host(&c->image[p.w], n, reinterpret_cast<uint16_t*>(&c->image[p.wh16]));
            }
            for (int r = 0; r < Np && !dry; ++r) {
                double acc = 0.0;
                for (size_t k = 0; k < Kp; ++k) {
                    const float w = c->image[p.w + (size_t)r * Kp + k];
                    acc += !h16 ? (double)w : c->bf16 ? (double)(float)(__bf16)w : (double)(float)(_Float16)fminf(fmaxf(w, -65504.f), 65504.f);
                }
                c->image[p.wsum + r] = (float)acc;
            }
        } else if (!dry) split_panel_host(&c->image[p.w], n, reinterpret_cast<uint16_t*>(&c->image[p.w16]));
    }
    // a panel from explicit host data (rearranged / synthesised weights)
    Panel panel_from(const float* w, const float* bias, int kind, int N, int C, int ntaps) {
        Panel p;
        p.N = N; p.C = C; p.ntaps = ntaps; p.ktap = round_up(C, kq);
        const int Np = round_up(N, GEMM_BN);
        const size_t Kp = (size_t)ntaps * p.ktap;
        p.w = alloc((size_t)Np * Kp);
        p.b = alloc(Np);
        if (!dry) pack_weight_host(w, kind, N, C, ntaps, 0, nullptr, nullptr, &c->image[p.w], p.ktap);
        if (bias) { p.has_bias = true; if (!dry) std::memcpy(&c->image[p.b], bias, N * sizeof(float)); }
        add_planes(p);
        return p;
    }
    // several [N_i, C(,k)] tensors stacked along N into one panel (q|k|v, concatenated time MLPs)
    Panel panel_multi(const std::vector<std::string>& wkeys, const std::vector<std::string>& bkeys, int kind, int N_each, int C,
                      int ntaps, int kT = 0, const int* tsel = nullptr, const std::vector<float>* col_scale = nullptr,
                      const std::vector<float>* col_shift = nullptr) {
        Panel p;
        const int parts = (int)wkeys.size();
        p.N = N_each * parts;
        p.C = C;
        p.ntaps = ntaps;
        p.ktap = round_up(C, kq);
        const int Np = round_up(p.N, GEMM_BN);
        const size_t Kp = (size_t)ntaps * p.ktap;
        p.w = alloc((size_t)Np * Kp);
        p.b = alloc(Np);
        const size_t per = (kind == 2) ? (size_t)C * N_each * kT : (size_t)N_each * C * ntaps;
        std::vector<float> tmp((size_t)round_up(N_each, GEMM_BN) * Kp);
        for (int part = 0; part < parts; ++part) {
            const auto* w = get(wkeys[part], per);
            if (!w) return p;
            const bool hb = part < (int)bkeys.size() && !bkeys[part].empty();
            const std::vector<float>* b = hb ? get(bkeys[part], N_each) : nullptr;
            if (hb && !b) return p;
            if (hb || col_shift) p.has_bias = true;
            if (dry) continue;
            pack_weight_host(w->data(), kind, N_each, C, ntaps, kT, tsel, col_scale ? col_scale->data() : nullptr, tmp.data(), p.ktap);
            std::memcpy(&c->image[p.w + (size_t)part * N_each * Kp], tmp.data(), (size_t)N_each * Kp * sizeof(float));
            for (int n = 0; n < N_each; ++n) {
                double acc = b ? (double)(*b)[n] : 0.0;
                if (col_shift) {   // LayerNorm beta folded through the projection: b' = b + W . beta
                    for (int cc = 0; cc < C; ++cc) acc += (double)(*w)[(size_t)n * C + cc] * (double)(*col_shift)[cc];
                }
                c->image[p.b + (size_t)part * N_each + n] = (float)acc;
            }
        }
        add_planes(p);
        return p;
    }
};

static int pack_all(mtts_ctx* c, bool dry = false) {
    const mtts_config& g = c->cfg;
    c->image.clear();
    c->weights_saturate = false;
    Packer P(c);
    P.dry = dry;
    auto S = [](const std::string& a, int i, const std::string& b) { return a + std::to_string(i) + b; };

    // ---------------- text encoder (reference text_encoder.py:319-373)
    EncW& E = c->enc;
    E = EncW();
    const int nch = g.enc_channels, Sd = g.spk_emb_dim, Hd = nch + Sd, F = g.dp_filter;
    const int dh = Hd / g.enc_heads, d_rope = dh / 2;
    E.emb = P.vec("encoder.emb.weight", g.n_vocab * nch);
    E.spk_enc = P.vec("speaker_embeddings_enc.weight", g.n_spks * Sd);
    E.spk_dur = P.vec("speaker_embeddings_dur.weight", g.n_spks * Sd);
    {
        auto it = c->raw.find("aux.rope_cos");
        if (it == c->raw.end() || it->second.size() % d_rope) P.fail("aux.rope_cos missing or misshaped");
        else {
            E.rope_cos = P.vec("aux.rope_cos", (int)it->second.size());
            E.rope_sin = P.vec("aux.rope_sin", (int)it->second.size());
        }
    }
    for (int i = 0; i < g.prenet_layers; ++i) {
        E.pre_conv.push_back(P.panel(S("encoder.prenet.conv_layers.", i, ".weight"), S("encoder.prenet.conv_layers.", i, ".bias"), 1, nch, nch, g.prenet_kernel));
        E.pre_g.push_back(P.vec(S("encoder.prenet.norm_layers.", i, ".gamma"), nch));
        E.pre_b.push_back(P.vec(S("encoder.prenet.norm_layers.", i, ".beta"), nch));
    }
    E.pre_proj = P.panel("encoder.prenet.proj.weight", "encoder.prenet.proj.bias", 1, nch, nch, 1);
    for (int i = 0; i < g.enc_layers; ++i) {
        const std::string a = S("encoder.encoder.attn_layers.", i, ".");
        E.qkv.push_back(P.panel_multi({a + "conv_q.weight", a + "conv_k.weight", a + "conv_v.weight"},
                                      {a + "conv_q.bias", a + "conv_k.bias", a + "conv_v.bias"}, 1, Hd, Hd, 1));
        E.o.push_back(P.panel(a + "conv_o.weight", a + "conv_o.bias", 1, Hd, Hd, 1));
        E.n1_g.push_back(P.vec(S("encoder.encoder.norm_layers_1.", i, ".gamma"), Hd));
        E.n1_b.push_back(P.vec(S("encoder.encoder.norm_layers_1.", i, ".beta"), Hd));
        const std::string f = S("encoder.encoder.ffn_layers.", i, ".");
        E.ffn1.push_back(P.panel(f + "conv_1.weight", f + "conv_1.bias", 1, g.enc_filter, Hd, g.enc_kernel));
        E.ffn2.push_back(P.panel(f + "conv_2.weight", f + "conv_2.bias", 1, Hd, g.enc_filter, g.enc_kernel));
        E.n2_g.push_back(P.vec(S("encoder.encoder.norm_layers_2.", i, ".gamma"), Hd));
        E.n2_b.push_back(P.vec(S("encoder.encoder.norm_layers_2.", i, ".beta"), Hd));
    }
    E.pm0 = P.panel("encoder.proj_m.0.weight", "encoder.proj_m.0.bias", 1, nch, Hd, 1);
    E.pm2 = P.panel("encoder.proj_m.2.weight", "encoder.proj_m.2.bias", 1, g.n_feats, nch, 1);
    E.film = P.panel("encoder.proj_w.spk_proj.weight", "encoder.proj_w.spk_proj.bias", 0, 2 * F, Sd, 1);
    for (int i = 0; i < g.dp_layers; ++i) {
        E.dp_conv.push_back(P.panel(S("encoder.proj_w.conv_layers.", i, ".weight"), S("encoder.proj_w.conv_layers.", i, ".bias"), 1, F,
                                    i == 0 ? Hd : F, g.dp_kernel));
        E.dp_g.push_back(P.vec(S("encoder.proj_w.norm_layers.", i, ".gamma"), F));
        E.dp_b.push_back(P.vec(S("encoder.proj_w.norm_layers.", i, ".beta"), F));
    }
    E.dp_proj = P.panel("encoder.proj_w.proj.weight", "encoder.proj_w.proj.bias", 1, 1, F, 1);

    // ---------------- decoder (reference decoder.py:202-310)
    P.kq = c->half16 ? 64 : GEMM_BK;
    P.h16 = c->half16;
    DecW& D = c->dec;
    D = DecW();
    const std::string R = "decoder.estimator.";
    const int cin0 = 2 * g.n_feats, nl = g.dec_levels, temb = g.dec_channels[0] * 4;
    const int inner = g.dec_heads * g.dec_head_dim;
    D.freqs = P.vec("aux.time_freqs", cin0 / 2);
    D.t1 = P.panel(R + "time_mlp.linear_1.weight", R + "time_mlp.linear_1.bias", 0, temb, cin0, 1);
    D.t2 = P.panel(R + "time_mlp.linear_2.weight", R + "time_mlp.linear_2.bias", 0, temb, temb, 1);

    std::vector<std::string> mlp_w, mlp_b;
    std::vector<int> mlp_n;
    auto resnet = [&](const std::string& p, int ci, int co) {
        ResnetW r;
        r.cin = ci;
        r.cout = co;
        r.conv1 = P.panel(p + "block1.block.0.weight", p + "block1.block.0.bias", 1, co, ci, 3);
        r.gn1_g = P.vec(p + "block1.block.1.weight", co);
        r.gn1_b = P.vec(p + "block1.block.1.bias", co);
        r.conv2 = P.panel(p + "block2.block.0.weight", p + "block2.block.0.bias", 1, co, co, 3);
        r.gn2_g = P.vec(p + "block2.block.1.weight", co);
        r.gn2_b = P.vec(p + "block2.block.1.bias", co);
        r.res = P.panel(p + "res_conv.weight", p + "res_conv.bias", 1, co, ci, 1);
        if (P.ok) { r.gn1_bs = P.bias_group_stats(r.conv1, 8); r.gn2_bs = P.bias_group_stats(r.conv2, 8); }
        mlp_w.push_back(p + "mlp.1.weight");
        mlp_b.push_back(p + "mlp.1.bias");
        mlp_n.push_back(co);
        D.res.push_back(r);
    };
    auto tblock = [&](const std::string& p, int ch) {
        TBlockW t;
        const auto* g1 = P.get(p + "norm1.weight", ch);
        const auto* b1 = P.get(p + "norm1.bias", ch);
        const auto* g3 = P.get(p + "norm3.weight", ch);
        const auto* b3 = P.get(p + "norm3.bias", ch);
        if (!g1 || !b1 || !g3 || !b3) return;
        // nn.LayerNorm affine folded into the projection that consumes it: W' = W * gamma (per column), b' = b + W . beta
        t.qkv = P.panel_multi({p + "attn1.to_q.weight", p + "attn1.to_k.weight", p + "attn1.to_v.weight"}, {}, 0, inner, ch, 1, 0,
                              nullptr, g1, b1);
        t.out = P.panel(p + "attn1.to_out.0.weight", p + "attn1.to_out.0.bias", 0, ch, inner, 1);
        t.ff1 = P.panel(p + "ff.net.0.proj.weight", p + "ff.net.0.proj.bias", 0, 4 * ch, ch, 1, 0, nullptr, g3, b3);
        t.alpha_exp = P.vec(p + "ff.net.0.alpha_exp", 4 * ch);
        t.inv_beta = P.vec(p + "ff.net.0.inv_beta", 4 * ch);
        t.ff2 = P.panel(p + "ff.net.2.weight", p + "ff.net.2.bias", 0, ch, 4 * ch, 1);
        D.tb.push_back(t);
    };
    int co = cin0;
    for (int i = 0; i < nl; ++i) {
        const int ci = co;
        co = g.dec_channels[i];
        resnet(R + S("down_blocks.", i, ".0."), ci, co);
        for (int j = 0; j < g.dec_n_blocks; ++j) tblock(R + S("down_blocks.", i, ".1.") + std::to_string(j) + ".", co);
        if (i < nl - 1) D.down.push_back(P.panel(R + S("down_blocks.", i, ".2.conv.weight"), R + S("down_blocks.", i, ".2.conv.bias"), 1, co, co, 3));
        else D.down.push_back(P.panel(R + S("down_blocks.", i, ".2.weight"), R + S("down_blocks.", i, ".2.bias"), 1, co, co, 3));
    }
    const int cmid = g.dec_channels[nl - 1];
    for (int i = 0; i < g.dec_mid_blocks; ++i) {
        resnet(R + S("mid_blocks.", i, ".0."), cmid, cmid);
        for (int j = 0; j < g.dec_n_blocks; ++j) tblock(R + S("mid_blocks.", i, ".1.") + std::to_string(j) + ".", cmid);
    }
    for (int i = 0; i < nl; ++i) {       // up path: channels reversed + channels[0]
        const int ci = g.dec_channels[nl - 1 - i];
        const int cu = (i + 1 < nl) ? g.dec_channels[nl - 2 - i] : g.dec_channels[0];
        resnet(R + S("up_blocks.", i, ".0."), 2 * ci, cu);
        for (int j = 0; j < g.dec_n_blocks; ++j) tblock(R + S("up_blocks.", i, ".1.") + std::to_string(j) + ".", cu);
        if (i < nl - 1) {
            // ConvTranspose1d(k4, s2, p1): out[2j] = W1.x[j] + W3.x[j-1];  out[2j+1] = W0.x[j+1] + W2.x[j]
            const int even[2] = {1, 3}, odd[2] = {0, 2};
            D.up_even.push_back(P.panel(R + S("up_blocks.", i, ".2.conv.weight"), R + S("up_blocks.", i, ".2.conv.bias"), 2, cu, cu, 2, 4, even));
            D.up_odd.push_back(P.panel(R + S("up_blocks.", i, ".2.conv.weight"), R + S("up_blocks.", i, ".2.conv.bias"), 2, cu, cu, 2, 4, odd));
        } else {
            D.up_last = P.panel(R + S("up_blocks.", i, ".2.weight"), R + S("up_blocks.", i, ".2.bias"), 1, cu, cu, 3);
        }
    }
    const int cfin = g.dec_channels[0];
    D.final_conv = P.panel(R + "final_block.block.0.weight", R + "final_block.block.0.bias", 1, cfin, cfin, 3);
    D.fgn_g = P.vec(R + "final_block.block.1.weight", cfin);
    D.fgn_b = P.vec(R + "final_block.block.1.bias", cfin);
    D.final_proj = P.panel(R + "final_proj.weight", R + "final_proj.bias", 1, g.n_feats, cfin, 1);
    if (P.ok) D.fgn_bs = P.bias_group_stats(D.final_conv, 8);
    // per-ResNet Linear(Mish(t)) stacked into one [sum(cout), temb] panel (rows of different blocks may differ in count)
    {
        int total = 0;
        for (size_t i = 0; i < D.res.size(); ++i) { D.res[i].tb_off = total; total += mlp_n[i]; }
        D.tb_total = total;
        Panel p;
        p.N = total; p.C = temb; p.ntaps = 1; p.ktap = round_up(temb, P.kq); p.has_bias = true;
        p.w = P.alloc((size_t)round_up(total, GEMM_BN) * p.ktap);
        p.b = P.alloc(round_up(total, GEMM_BN));
        for (size_t i = 0; i < D.res.size() && P.ok; ++i) {
            const auto* w = P.get(mlp_w[i], (size_t)mlp_n[i] * temb);
            const auto* b = P.get(mlp_b[i], mlp_n[i]);
            if (!w || !b) break;
            for (int n = 0; n < mlp_n[i] && !dry; ++n) {
                std::memcpy(&c->image[p.w + (size_t)(D.res[i].tb_off + n) * p.ktap], &(*w)[(size_t)n * temb], temb * sizeof(float));
                c->image[p.b + D.res[i].tb_off + n] = (*b)[n];
            }
        }
        if (P.ok) P.add_planes(p);
        D.tmlp = p;
    }
    // fragment streams of the transformer blocks' row-local chains (tblock_chain.hip): fp16-split arithmetic, P16 flow only
    if (P.ok && c->sw.chain_on && c->gemm_terms == 2 && !c->half16 && !c->fast16 && c->sw.p16_on && g.dec_head_dim == 64) {
        const int nb = g.dec_n_blocks;
        for (size_t k = 0; k < D.tb.size(); ++k) {
            TBlockW& t = D.tb[k];
            const int C = t.out.N, nq = ((int)(k % nb) + 1 < nb) ? D.tb[k + 1].qkv.N : 0;
            const int ch = (C == 384 && c->sw.chain_ch == 256) ? 256 : 128;
            if (!chain_supported(C, inner, nq) || t.ff1.N != 4 * C || t.ff1.ktap != C || t.ff2.ktap != 4 * C || t.out.ktap != inner) continue;
            if (nq && D.tb[k + 1].qkv.ktap != C) continue;
            t.chain_frags = chain_stream_frags(C, inner, ch, nq);
            t.chain_ch = ch;
            t.chain_nqkv = nq;
            t.next = nq ? (int)k + 1 : -1;
            t.chain = P.alloc((size_t)t.chain_frags * CHAIN_WAVES * 256);
            if (c->sw.pair_on && chain_supported_pair(C, inner, ch, nq)) {
                t.chain_pair_frags = chain_stream_frags_pair(C, inner, ch, nq);
                t.chain_pair = P.alloc((size_t)t.chain_pair_frags * 2 * CHAIN_WAVES * 256);
                if (!dry) chain_stream_pack_pair(C, inner, ch, nq, &c->image[t.out.w], &c->image[t.ff1.w], &c->image[t.ff2.w],
                                                 nq ? &c->image[D.tb[k + 1].qkv.w] : nullptr, reinterpret_cast<uint16_t*>(&c->image[t.chain_pair]),
                                                 &c->weights_saturate);
            }
            t.chain_consts = P.alloc((size_t)18 * C);
            if (!dry) {
                chain_stream_pack(C, inner, ch, nq, &c->image[t.out.w], &c->image[t.ff1.w], &c->image[t.ff2.w],
                                  nq ? &c->image[D.tb[k + 1].qkv.w] : nullptr, reinterpret_cast<uint16_t*>(&c->image[t.chain]),
                                  &c->weights_saturate);
                float* cc = &c->image[t.chain_consts];          // the chain kernel's column constants as one block (kernels.h)
                std::memcpy(cc, &c->image[t.ff1.wsum], (size_t)4 * C * sizeof(float));
                std::memcpy(cc + 4 * C, &c->image[t.ff1.b], (size_t)4 * C * sizeof(float));
                std::memcpy(cc + 8 * C, &c->image[t.alpha_exp.off], (size_t)4 * C * sizeof(float));
                std::memcpy(cc + 12 * C, &c->image[t.inv_beta.off], (size_t)4 * C * sizeof(float));
                std::memcpy(cc + 16 * C, &c->image[t.out.b], (size_t)C * sizeof(float));
                std::memcpy(cc + 17 * C, &c->image[t.ff2.b], (size_t)C * sizeof(float));
            }
        }
    }
    // 16-bit storage modes: the same chains as ONE-plane streams (tblock_chain_h16.hip), fp16 or bfloat16 by c->bf16.  Nothing
    // two-plane is packed in these modes and nothing one-plane in the default one.
    if (P.ok && c->sw.chain_on && c->sw.chain16_on && c->gemm_terms == 2 && c->half16 && c->sw.p16_on && g.dec_head_dim == 64) {
        const int nb = g.dec_n_blocks;
        for (size_t k = 0; k < D.tb.size(); ++k) {
            TBlockW& t = D.tb[k];
            const int C = t.out.N, nq = ((int)(k % nb) + 1 < nb) ? D.tb[k + 1].qkv.N : 0;
            const int ch = (C == 384 && c->sw.chain_ch == 256) ? 256 : 128;
            if (!chain_h16_supported(C, inner, ch, nq) || t.ff1.N != 4 * C || t.ff1.ktap != C || t.ff2.ktap != 4 * C || t.out.ktap != inner) continue;
            if (nq && D.tb[k + 1].qkv.ktap != C) continue;
            t.chain_frags = chain_h16_stream_frags(C, inner, ch, nq);
            t.chain_ch = ch;
            t.chain_nqkv = nq;
            t.chain_h16 = true;
            t.next = nq ? (int)k + 1 : -1;
            t.chain = P.alloc((size_t)t.chain_frags * CHAIN_WAVES * 256);
            t.chain_consts = P.alloc((size_t)18 * C);
            if (!dry) {
                bool sat = false;
                chain_h16_stream_pack(C, inner, ch, nq, &c->image[t.out.w], &c->image[t.ff1.w], &c->image[t.ff2.w],
                                      nq ? &c->image[D.tb[k + 1].qkv.w] : nullptr, c->bf16, reinterpret_cast<uint16_t*>(&c->image[t.chain]), &sat);
                if (sat) c->weights_saturate = true;
                float* cc = &c->image[t.chain_consts];          // (ff1.wsum: row sums of the ROUNDED panel in these modes, add_planes)
                std::memcpy(cc, &c->image[t.ff1.wsum], (size_t)4 * C * sizeof(float));
                std::memcpy(cc + 4 * C, &c->image[t.ff1.b], (size_t)4 * C * sizeof(float));
                std::memcpy(cc + 8 * C, &c->image[t.alpha_exp.off], (size_t)4 * C * sizeof(float));
                std::memcpy(cc + 12 * C, &c->image[t.inv_beta.off], (size_t)4 * C * sizeof(float));
                std::memcpy(cc + 16 * C, &c->image[t.out.b], (size_t)C * sizeof(float));
                std::memcpy(cc + 17 * C, &c->image[t.ff2.b], (size_t)C * sizeof(float));
            }
        }
    }
    if (!P.ok) { set_error(P.why); return -1; }
    c->packed = true;
    return 0;
}

static inline const float* W(const mtts_ctx* c, size_t off) { return c->d_image + off; }

static void panel_args(const mtts_ctx* c, const Panel& p, GemmArgs& a) {
    a.w = W(c, p.w);
    a.terms = c->gemm_terms;
    a.w16 = c->gemm_terms ? static_cast<const void*>(W(c, p.w16)) : nullptr;
    a.bias = p.has_bias ? W(c, p.b) : nullptr;
    a.wsum = c->gemm_terms == 2 ? W(c, p.wsum) : nullptr;
    a.fast16 = c->fast16;
    a.w16h = (c->half16 && p.wh16) ? static_cast<const void*>(W(c, p.wh16)) : nullptr;
    a.N = p.N;
    a.ntaps = p.ntaps;
    a.ktap = p.ktap;
}
static void rows_plain(GemmArgs& a, int B, int T) {
    a.B = B; a.T_in = T; a.T_out = T; a.in_stride = 1;
    a.out_T = T; a.out_stride = 1; a.out_off = 0;
}
static void taps_centered(GemmArgs& a, int k) {
    for (int j = 0; j < k; ++j) a.tap_off[j] = j - k / 2;
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
    return 0;
}

// SinusoidalPosEmb + TimestepEmbedding + every ResNet's Linear(Mish(t)) for all evaluation times at once
// (reference decoder.py:14-29,107-119,51,60): they depend on t only, so the whole ODE grid is done before the loop.
static int time_embed(mtts_ctx* c, DecBufs& d, const TimeVals& tv, int nt, hipStream_t s) {
    const mtts_config& g = c->cfg;
    const DecW& D = c->dec;
    const int cin0 = 2 * g.n_feats, temb = g.dec_channels[0] * 4;
    LAUNCH(c, 2, 0, s, launch_time_sinusoid(W(c, D.freqs.off), tv, nt, cin0 / 2, 1000.0f, d.TS, s));
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
    f.gamma = W(c, gamma.off); f.beta = W(c, beta.off); f.mask = d.mask[lvl]; f.chbias = chbias; f.nrows = d.nr(lvl);
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
        g1.chbias = tbias;
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
    // the row-local part as one launch (tblock_chain.hip) when the stream was packed and the batch is large enough that a
    // workgroup per QB rows fills the chip: every workgroup streams ALL of the chain's weights (~7 MB at width 384), which
    // only pays when their cost is shared by many rows per CU
    const bool chain = t.chain_frags > 0 && !t.chain_h16 && d.p16 && !c->half_now && M >= c->sw.chain_min_rows && (emit_stats ? t.chain_nqkv > 0 : true);
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
    // below that row count: the pair form -- two workgroups of one XCD per 48-row tile, each streaming half of the FeedForward
    // and of the q|k|v passes -- while all of them (and the prefetchers) are resident at once
    const int tiles48 = (M + 47) / 48;
    const bool pair = !chain && !chain16 && c->sw.pair_on && t.chain_pair_frags > 0 && d.p16 && !c->half_now && d.pair_flag && M >= c->sw.pair_min_rows &&
                      16 * ((tiles48 + 7) / 8) + 16 <= CHIP_CUS && (emit_stats ? t.chain_nqkv > 0 : true);
    if (chain16) {                        // (image flow, H16: one 2-byte value per channel)
        ChainH16Args a;
        a.M = M; a.C = C; a.inner = inner; a.bf16 = c->bf16;
        a.att16 = image(d.ATT); a.ld_att = inner;
        a.x16 = image(x); a.ld_x = C;
        a.wstream = W(c, t.chain); a.stream_frags = t.chain_frags;
        a.consts = W(c, t.chain_consts);
        a.ld_out = C;
        if (emit_stats) {                 // another block follows: its q|k|v leaves this launch, x stays unmasked
            const TBlockW& nx = c->dec.tb[t.next];
            a.b_qkv = W(c, nx.qkv.b); a.wsum_qkv = W(c, nx.qkv.wsum); a.n_qkv = nx.qkv.N;
            a.qkv16 = image(d.QKV); a.ld_qkv = nx.qkv.N;
            a.x_out = image(x);
            d.qkv_ready = true;
        } else { a.x_out = image(dst); a.x_out_mask = d.mask[lvl]; }
        a.ch = t.chain_ch;
        return run_chain_h16(c, a, s);
    }
    if (chain || pair) {                  // (image flow, P16: rows of 2 halves per channel)
        ChainArgs a;
        a.M = M; a.C = C; a.inner = inner;
        a.att16 = image(d.ATT); a.ld_att = 2 * inner;
        a.x16 = image(x); a.ld_x = 2 * C;
        a.wstream = reinterpret_cast<const _Float16*>(W(c, t.chain)); a.stream_frags = t.chain_frags;
        a.consts = W(c, t.chain_consts);
        a.ld_out = 2 * C;
        if (emit_stats) {                 // another block follows: its q|k|v leaves this launch, x stays unmasked
            const TBlockW& nx = c->dec.tb[t.next];
            a.b_qkv = W(c, nx.qkv.b); a.wsum_qkv = W(c, nx.qkv.wsum); a.n_qkv = nx.qkv.N;
            a.qkv16 = image(d.QKV); a.ld_qkv = 2 * nx.qkv.N;
            a.x_out = image(x);
            d.qkv_ready = true;
        } else { a.x_out = image(dst); a.x_out_mask = d.mask[lvl]; }
        a.ch = t.chain_ch;
        { int pf_unused = 0; chain_plan(M, a.ch, c->sw.chain_qb, c->sw.chain_pf, &a.qb, &pf_unused); }
        if (pair) {
            a.pair = 1; a.qb = 48;
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
};

// Decoder.forward (reference decoder.py:359-426) for evaluation `ev` (row of the precomputed time biases).
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
    p.out_mask = d.mask[0];
    p.out = fo.out; p.ldc = fo.ldc; p.res = fo.res; p.ldr = fo.ldr; p.out_scale = fo.scale;
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

// Entry-point guard (round-2 verdict item 8 / advisor): a context is single-threaded by design; concurrent use is an error, not a race.
struct CtxGuard {
    mtts_ctx* c;
    bool ok;
    explicit CtxGuard(mtts_ctx* ctx) : c(ctx), ok(false) {
        if (!c) return;
        bool expect = false;
        ok = c->in_use.compare_exchange_strong(expect, true);
        if (!ok) set_error("this mtts_ctx is in use by another thread: a context is single-threaded (one context per worker / stream, include/mtts.h)");
    }
    ~CtxGuard() { if (ok) c->in_use.store(false); }
};
#define CTX_GUARD(ctx)            \
    CtxGuard _guard(ctx);         \
    if ((ctx) && !_guard.ok) return -1

static int check_ready(const mtts_ctx* c) {
    if (!c) { set_error("null context"); return -1; }
    if (!c->uploaded || !c->d_image) { set_error("weights not uploaded (mtts_upload_weights)"); return -1; }
    return 0;
}

}  // namespace mtts

using namespace mtts;

// ================================================================================================ C ABI
extern "C" {

int mtts_abi_version(void) { return MTTS_ABI_VERSION; }
const char* mtts_last_error(void) { return get_error(); }

mtts_ctx* mtts_create(const mtts_config* cfg) {
    if (!cfg) { set_error("null config"); return nullptr; }
    const mtts_config& g = *cfg;
    std::string why;
    if (g.dec_levels < 1 || g.dec_levels > 4) why = "dec_levels must be 1..4";
    else if (g.n_feats <= 0 || (2 * g.n_feats) % 4) why = "n_feats must be even";
    else if ((g.enc_channels + g.spk_emb_dim) % g.enc_heads) why = "encoder hidden size not divisible by heads";
    else if (((g.enc_channels + g.spk_emb_dim) / g.enc_heads) % 4 || (g.enc_channels + g.spk_emb_dim) / g.enc_heads > 64) why = "encoder head dim must be a multiple of 4, <= 64";
    else if (g.dec_head_dim % 4 || g.dec_head_dim > 64) why = "decoder head dim must be a multiple of 4, <= 64";
    else if (g.enc_channels % 4 || g.spk_emb_dim % 4 || g.enc_filter % 4 || g.dp_filter % 4) why = "channel counts must be multiples of 4";
    else if (g.enc_kernel > MAX_TAPS || g.prenet_kernel > MAX_TAPS || g.dp_kernel > MAX_TAPS) why = "kernel sizes above 5 unsupported";
    for (int i = 0; why.empty() && i < g.dec_levels; ++i)
        if (g.dec_channels[i] % 32) why = "decoder channels must be multiples of 32 (8 GroupNorm groups of 4k channels, K segments of 32)";
    if (!why.empty()) { set_error(why); return nullptr; }
    mtts_ctx* c = new mtts_ctx();
    c->cfg = g;
    c->sw = read_switches();
    c->gemm_terms = c->sw.gemm_terms;
    c->fast16 = c->sw.arith16 == 1; c->half16 = c->sw.arith16 >= 16; c->bf16 = c->sw.arith16 == 17;
    if (c->sw.pair_on) {       // the pair form's residency bound assumes the whole chip: a partitioned or smaller device runs without it
        int dev = 0;
        hipDeviceProp_t prop;
        if (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&prop, dev) == hipSuccess && prop.multiProcessorCount < CHIP_CUS) c->sw.pair_on = false;
        (void)hipGetLastError();             // (no device at all -- the CPU-side packing tests -- leaves the setting as it is)
    }
    return c;
}

int mtts_set_arithmetic(mtts_ctx* c, int terms) {
    if (!c) { set_error("null context"); return -1; }
    if (terms != 0 && terms != 1 && terms != 2 && terms != 3 && terms != 6 && terms != 16 && terms != 17) {
        set_error("mtts_set_arithmetic: terms must be 0, 1, 2, 3, 6, 16 or 17");
        return -1;
    }
    c->fast16 = terms == 1;
    c->half16 = terms == 16 || terms == 17;
    c->bf16 = terms == 17;
    c->gemm_terms = (terms == 1 || terms == 16 || terms == 17) ? 2 : terms;
    c->packed = false;
    c->uploaded = false;
    return 0;
}

int mtts_weights_saturate(mtts_ctx* c) {
    if (!c) { set_error("null context"); return -1; }
    if (!c->packed && pack_all(c)) return -1;
    return c->weights_saturate ? 1 : 0;
}

void mtts_destroy(mtts_ctx* c) {
    if (!c) return;
    for (hipEvent_t e : c->ev_pool) (void)hipEventDestroy(e);
    delete c;
}

int mtts_set_tensor(mtts_ctx* c, const char* key, const float* h, int64_t numel) {
    if (!c || !key || !h || numel < 0) { set_error("mtts_set_tensor: bad argument"); return -1; }
    c->raw[key].assign(h, h + numel);
    c->packed = false;
    c->uploaded = false;
    return 0;
}

int64_t mtts_weights_bytes(mtts_ctx* c) {
    if (!c) { set_error("null context"); return -1; }
    if (!c->packed && pack_all(c)) return -1;
    return (int64_t)(c->image.size() * sizeof(float));
}

// The packed image depends on the architecture, the arithmetic and the layout switches -- everything below, as one string: a
// cache file written by mtts_export_weights is valid for a context with the same signature and the same checkpoint tensors.
int mtts_weights_signature(mtts_ctx* c, char* buf, int64_t n) {
    if (!c || !buf || n < 64) { set_error("mtts_weights_signature: bad argument"); return -1; }
    const mtts_config& g = c->cfg;
    const int v[] = {MTTS_ABI_VERSION, MTTS_IMAGE_REVISION, g.n_feats, g.n_spks, g.spk_emb_dim, g.n_vocab, g.enc_channels, g.enc_filter,
                     g.enc_heads, g.enc_layers, g.enc_kernel, g.prenet_layers, g.prenet_kernel, g.dp_filter, g.dp_kernel, g.dp_layers,
                     g.dec_levels, g.dec_channels[0], g.dec_channels[1], g.dec_channels[2], g.dec_channels[3], g.dec_head_dim, g.dec_heads,
                     g.dec_n_blocks, g.dec_mid_blocks, c->gemm_terms, c->half16, c->bf16, c->fast16, c->sw.p16_on, c->sw.chain_on, c->sw.chain_ch, c->sw.pair_on, c->sw.chain16_on};
    std::string sig = "mtts";
    for (int x : v) sig += "-" + std::to_string(x);
    if ((int64_t)sig.size() + 1 > n) { set_error("mtts_weights_signature: buffer too small"); return -1; }
    std::memcpy(buf, sig.c_str(), sig.size() + 1);
    return (int)sig.size();
}
int mtts_export_weights(mtts_ctx* c, void* h_dst, int64_t bytes, int* saturates) {
    if (!c || !h_dst) { set_error("mtts_export_weights: bad argument"); return -1; }
    if (!c->packed && pack_all(c)) return -1;
    if ((size_t)bytes < c->image.size() * sizeof(float)) { set_error("mtts_export_weights: buffer too small"); return -1; }
    std::memcpy(h_dst, c->image.data(), c->image.size() * sizeof(float));
    if (saturates) *saturates = c->weights_saturate ? 1 : 0;
    return 0;
}
// Adopt an image exported earlier by a context of the same signature over the same tensors: the layout pass runs (offsets, sizes,
// presence and shape of every registered tensor), the ~7 s of splitting and fragment packing do not.
int mtts_import_weights(mtts_ctx* c, const void* h_src, int64_t bytes, int saturates) {
    if (!c || !h_src) { set_error("mtts_import_weights: bad argument"); return -1; }
    if (pack_all(c, true)) return -1;
    if ((size_t)bytes != c->image.size() * sizeof(float)) {
        c->packed = false;
        set_error("mtts_import_weights: the image does not have this context's size (other architecture / arithmetic / library?)");
        return -1;
    }
    std::memcpy(c->image.data(), h_src, (size_t)bytes);
    c->weights_saturate = saturates != 0;
    c->uploaded = false;
    return 0;
}

int mtts_upload_weights(mtts_ctx* c, void* d_weights, int64_t bytes) {
    if (!c || !d_weights) { set_error("mtts_upload_weights: bad argument"); return -1; }
    if (!c->packed && pack_all(c)) return -1;
    if ((size_t)bytes < c->image.size() * sizeof(float)) { set_error("weight buffer too small"); return -1; }
    HIP_OK(hipMemcpy(d_weights, c->image.data(), c->image.size() * sizeof(float), hipMemcpyHostToDevice));
    c->d_image = static_cast<float*>(d_weights);
    c->uploaded = true;
    return 0;
}

// ------------------------------------------------------------------------------------------------ decoder entry points
int64_t mtts_decoder_workspace_bytes(mtts_ctx* c, int B, int T) {
    if (!c || (!c->packed && pack_all(c))) return -1;
    WS ws(nullptr, 0);
    DecBufs d;
    if (plan_decoder(c, B, T, MAX_EVALS, 2, 4, ws, d)) return -1;
    return (int64_t)ws.off + 256;
}

// Test hook of the entry-point guard: holds the context as an entry point does, for `ms` milliseconds.
int mtts_debug_hold(mtts_ctx* c, int ms) {
    if (!c) { set_error("null context"); return -1; }
    CTX_GUARD(c);
    struct timespec ts = {ms / 1000, (long)(ms % 1000) * 1000000L};
    nanosleep(&ts, nullptr);
    return 0;
}

int mtts_set_frame_limits(mtts_ctx* c, const int32_t* d_t_len) {
    if (!c) { set_error("null context"); return -1; }
    c->d_tlen = d_t_len;
    return 0;
}

int mtts_decoder_forward(mtts_ctx* c, const float* d_x, const float* d_mask, const float* d_mu, float t, int B, int T,
                         float* d_out, void* d_ws, int64_t ws_bytes, void* stream) {
    CTX_GUARD(c);
    RET_IF(check_ready(c));
    hipStream_t s = static_cast<hipStream_t>(stream);
    WS ws(d_ws, (size_t)ws_bytes);
    DecBufs d;
    RET_IF(plan_decoder(c, B, T, MAX_EVALS, 2, 4, ws, d));
    if (ws.overflow) { set_error("decoder workspace too small"); return -1; }
    RET_IF(begin_call(c, d_ws, s));
    if (c->sw.pair_on) HIP_OK(launch_fill_cols(reinterpret_cast<float*>(d.pair_flag), 1, 512, 0, 512, 0.f, s));
    const int nf = c->cfg.n_feats;
    RET_IF(build_frames(c, d, d_mask, nullptr, T, s));
    LAUNCH(c, 2, 0, s, launch_fill_cols(d.xmu, B * T, d.ldx, 2 * nf, d.ldx - 2 * nf, 0.f, s));
    LAUNCH(c, 2, 0, s, launch_cf_to_cl(d_x, nullptr, B, nf, T, d.xmu, d.ldx, 0, s));
    LAUNCH(c, 2, 0, s, launch_cf_to_cl(d_mu, nullptr, B, nf, T, d.xmu, d.ldx, nf, s));
    TimeVals tv;
    tv.t[0] = t;
    RET_IF(time_embed(c, d, tv, 1, s));
    FinalOut fo{d.vel[0], d.ldv, nullptr, 0, 1.0f};
    RET_IF(decoder_eval(c, d, d.xmu, 0, fo, s));
    LAUNCH(c, 2, 0, s, launch_cl_to_cf(d.vel[0], d.ldv, B, nf, T, d_out, T, 1.0f, 0.0f, s));
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
    RET_IF(plan_decoder(c, B, T, MAX_EVALS, 2, 4, ws, d));
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
    RET_IF(time_embed(c, d, tv, ne, s));

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

int mtts_align_pool(const float* d_mu_x, const int32_t* d_cum, const int64_t* d_y_fine_lengths, int B, int n_feats, int Tx, int T_pad,
                    float* d_mu_y, float* d_y_mask, int64_t* d_y_lengths, void* stream) {
    HIP_OK(launch_align_pool(d_mu_x, d_cum, d_y_fine_lengths, B, n_feats, Tx, T_pad, d_mu_y, d_y_mask, d_y_lengths,
                             static_cast<hipStream_t>(stream)));
    return 0;
}

// ------------------------------------------------------------------------------------------------ single kernels
int64_t mtts_gemm_packed_bytes(int N, int C, int ntaps) {   // fp32 panel + three bf16 planes
    const int64_t n = (int64_t)round_up(N, GEMM_BN) * ntaps * round_up(C, GEMM_BK);
    return n * 4 + ((3 * n + 1) / 2) * 4 + 256;
}

int mtts_gemm_f32(const float* d_a, int lda, int B, int T_in, int C, int ntaps, const int* h_tap_off, int in_stride, int T_out,
                  const float* d_a_mask, const float* d_a_mean, const float* d_a_rstd, const float* d_a_part, int a_nparts,
                  const float* d_w, void* d_wpacked, const float* d_bias, int N, int act, const float* d_p0, const float* d_p1,
                  const float* d_res, int ldr, const float* d_out_mask, float out_scale, float* d_out, int ldc, float* d_stats_out,
                  int terms, void* stream) {
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (ntaps < 1 || ntaps > MAX_TAPS) { set_error("ntaps out of range"); return -1; }
    if (terms < 0) terms = read_switches().gemm_terms;
    if (terms != 0 && terms != 2 && terms != 3 && terms != 6) { set_error("terms must be 0, 2, 3 or 6"); return -1; }
    const size_t npanel = (size_t)round_up(N, GEMM_BN) * ntaps * round_up(C, GEMM_BK);
    float* planes = static_cast<float*>(d_wpacked) + ((npanel + 63) & ~size_t(63));
    if (d_w) {   // NULL: d_wpacked already packed by an earlier call
        HIP_OK(launch_pack_weight(d_w, N, C, ntaps, static_cast<float*>(d_wpacked), s));
        if (terms == 2) HIP_OK(launch_split_panel_f16(static_cast<const float*>(d_wpacked), npanel, planes, s));
        else HIP_OK(launch_split_panel(static_cast<const float*>(d_wpacked), npanel, planes, s));
    }
    GemmArgs a;
    a.a0 = d_a; a.lda0 = lda; a.c0 = C; a.ktap = round_up(C, GEMM_BK); a.ntaps = ntaps;
    for (int j = 0; j < ntaps; ++j) a.tap_off[j] = h_tap_off ? h_tap_off[j] : 0;
    a.in_stride = in_stride; a.B = B; a.T_in = T_in; a.T_out = T_out;
    a.a_mask = d_a_mask; a.a_mean = d_a_mean; a.a_rstd = d_a_rstd; a.a_part = d_a_part; a.a_nparts = a_nparts;
    a.stats_out = d_stats_out;
    a.w = static_cast<const float*>(d_wpacked); a.w16 = planes; a.terms = terms; a.bias = d_bias; a.N = N; a.act = act; a.p0 = d_p0; a.p1 = d_p1;
    a.res = d_res; a.ldr = ldr; a.out_mask = d_out_mask; a.out_scale = out_scale; a.out = d_out; a.ldc = ldc;
    a.out_T = T_out; a.out_stride = 1; a.out_off = 0;
    HIP_OK(launch_gemm(a, s));
    return 0;
}

// Test entry for the P16 GEMM (gemm_p16.hip): the fp32 operand is converted to its P16 image (optionally masked) in
// d_scratch, the panel is packed as for mtts_gemm_f32 (terms = 2) and its row sums are computed for the LayerNorm algebra;
// the optional P16 output is decoded back to fp32 into d_out16_f32.
int64_t mtts_gemm_p16_scratch_bytes(int B, int T_in, int C, int T_out, int N) {
    return (int64_t)B * T_in * C * 4 + (int64_t)B * T_out * round_up(N, 32) * 4 + (int64_t)round_up(N, GEMM_BN) * 4 + 1024;
}
__global__ void panel_rowsum_kernel(const float* __restrict__ panel, int Np, int Kp, float* __restrict__ out) {
    const int n = blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= Np) return;
    double acc = 0.0;
    for (int k = 0; k < Kp; ++k) acc += (double)panel[(size_t)n * Kp + k];
    out[n] = (float)acc;
}
int mtts_gemm_p16(const float* d_a, int lda, int B, int T_in, int C, int ntaps, const int* h_tap_off, int in_stride, int T_out,
                  const float* d_a_mask, const float* d_a_mean, const float* d_a_rstd, const float* d_a_part, int a_nparts,
                  const float* d_w, void* d_wpacked, const float* d_bias, int N, int act, const float* d_p0, const float* d_p1,
                  const float* d_res, int ldr, const float* d_out_mask, float out_scale, float* d_out, int ldc,
                  float* d_out16_f32, float out_lscale, float* d_stats_out, int force_bm, void* d_scratch, void* stream) {
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (ntaps < 1 || ntaps > MAX_TAPS) { set_error("ntaps out of range"); return -1; }
    if (C % GEMM_BK) { set_error("P16 operands need C % 32 == 0"); return -1; }
    if (!d_w || !d_wpacked || !d_scratch) { set_error("null buffer"); return -1; }
    const int Np = round_up(N, GEMM_BN), Kp = ntaps * C;
    const size_t npanel = (size_t)Np * Kp;
    float* planes = static_cast<float*>(d_wpacked) + ((npanel + 63) & ~size_t(63));
    HIP_OK(launch_pack_weight(d_w, N, C, ntaps, static_cast<float*>(d_wpacked), s));
    HIP_OK(launch_split_panel_f16(static_cast<const float*>(d_wpacked), npanel, planes, s));
    char* sc = static_cast<char*>(d_scratch);
    _Float16* a16 = reinterpret_cast<_Float16*>(sc);
    sc += (size_t)B * T_in * C * 4;
    _Float16* o16 = reinterpret_cast<_Float16*>(sc);
    sc += (size_t)B * T_out * round_up(N, 32) * 4;
    float* wsum = reinterpret_cast<float*>(sc);
    HIP_OK(launch_to_p16(d_a, lda, d_a_mask, B * T_in, C, C, a16, 2 * C, 2048.0f, s));
    hipLaunchKernelGGL(panel_rowsum_kernel, dim3((Np + 127) / 128), dim3(128), 0, s, static_cast<const float*>(d_wpacked), Np, Kp, wsum);
    HIP_OK(hipGetLastError());
    GemmArgs a;
    a.a16_0 = a16; a.lda16_0 = 2 * C; a.c0 = C; a.ktap = C; a.ntaps = ntaps;
    for (int j = 0; j < ntaps; ++j) a.tap_off[j] = h_tap_off ? h_tap_off[j] : 0;
    a.in_stride = in_stride; a.B = B; a.T_in = T_in; a.T_out = T_out;
    a.a_mean = d_a_mean; a.a_rstd = d_a_rstd; a.a_part = d_a_part; a.a_nparts = a_nparts; a.wsum = wsum;
    a.stats_out = d_stats_out;
    a.w16 = planes; a.terms = 2; a.bias = d_bias; a.N = N; a.act = act; a.p0 = d_p0; a.p1 = d_p1;
    a.res = d_res; a.ldr = ldr; a.out_mask = d_out_mask; a.out_scale = out_scale; a.out = d_out; a.ldc = ldc;
    if (d_out16_f32) { a.out16 = o16; a.ld16 = 2 * N; a.out_lscale = out_lscale; }
    a.out_T = T_out; a.out_stride = 1; a.out_off = 0; a.force_bm = force_bm;
    HIP_OK(launch_gemm(a, s));
    if (d_out16_f32) HIP_OK(launch_from_p16(o16, 2 * N, B * T_out, N, out_lscale, d_out16_f32, N, s));
    return 0;
}

// Test entry for the one-launch Block1D (resnet_conv.hip): x [B*T, C] fp32 (already masked by the caller where the model would)
// is converted to its P16 image in d_scratch, the Conv1d(k3) weight is packed and split as for mtts_gemm_p16, the P16 output is
// decoded back to fp32 [B*T, N].  c1 > 0: the last c1 channels of x form a second input segment (the up path's skip concat).
int64_t mtts_conv_gn_scratch_bytes(int B, int T, int C, int N) { return (int64_t)B * T * (C + N) * 4 + 1024; }
int mtts_conv_gn(const float* d_x, int B, int T, int C, int c1, const float* d_w, void* d_wpacked, const float* d_bias, int N,
                 const float* d_gamma, const float* d_beta, const float* d_mask, const float* d_chbias, const int* d_nrows,
                 const int* d_nextra, const float* d_bias_stats, float eps, float* d_out, void* d_scratch, void* stream) {
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (!d_x || !d_w || !d_wpacked || !d_scratch || !d_out) { set_error("null buffer"); return -1; }
    if (C <= 0 || (C % 32) || c1 < 0 || (c1 % 32) || c1 >= C) { set_error("mtts_conv_gn: C and c1 must be multiples of 32, c1 < C"); return -1; }
    if (!conv_gn_supported(T, N)) { set_error("mtts_conv_gn: unsupported shape (N = 384, 65 <= T <= 384)"); return -1; }
    const int Np = round_up(N, GEMM_BN), Kp = 3 * C;
    const size_t npanel = (size_t)Np * Kp;
    float* planes = static_cast<float*>(d_wpacked) + ((npanel + 63) & ~size_t(63));
    HIP_OK(launch_pack_weight(d_w, N, C, 3, static_cast<float*>(d_wpacked), s));
    HIP_OK(launch_split_panel_f16(static_cast<const float*>(d_wpacked), npanel, planes, s));
    _Float16* a16 = static_cast<_Float16*>(d_scratch);
    _Float16* o16 = a16 + (size_t)B * T * C * 2;
    HIP_OK(launch_to_p16(d_x, C, nullptr, B * T, C, C, a16, 2 * C, 2048.0f, s));
    ConvGnArgs a;
    a.a16_0 = a16; a.lda16_0 = 2 * C; a.c0 = C - c1;
    if (c1) { a.a16_1 = a16 + 2 * (C - c1); a.lda16_1 = 2 * C; a.c1 = c1; }
    a.w16 = planes; a.bias = d_bias; a.B = B; a.T = T; a.N = N;
    a.gamma = d_gamma; a.beta = d_beta; a.mask = d_mask; a.chbias = d_chbias; a.nrows = d_nrows; a.nextra = d_nextra; a.bias_stats = d_bias_stats;
    a.eps = eps; a.out16 = o16; a.ld16 = 2 * N;
    HIP_OK(launch_conv_gn(a, s));
    HIP_OK(launch_from_p16(o16, 2 * N, B * T, N, 2048.0f, d_out, N, s));
    return 0;
}

int mtts_attention_f32(const float* d_qkv, const float* d_mask, int B, int T, int H, int D, float scale, int mask_mode, float* d_out,
                       void* stream) {
    AttnArgs a;
    a.qkv = d_qkv; a.mask = d_mask; a.out = d_out; a.B = B; a.T = T; a.H = H; a.D = D; a.scale = scale; a.mask_mode = mask_mode;
    HIP_OK(launch_attention(a, static_cast<hipStream_t>(stream)));
    return 0;
}

// Test entry for the attention kernel's P16 I/O: q|k|v converted to a P16 image with unscaled residuals in d_scratch
// (>= 16*B*T*H*64 bytes), the P16 output decoded back to fp32.  D must be 64.
int mtts_attention_p16(const float* d_qkv, const float* d_mask, int B, int T, int H, int D, float scale, int mask_mode, float* d_out,
                       void* d_scratch, void* stream) {
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (D != 64 || !d_scratch) { set_error("P16 attention needs D == 64 and a scratch buffer"); return -1; }
    const int M = B * T, C3 = 3 * H * D;
    _Float16* q16 = static_cast<_Float16*>(d_scratch);
    _Float16* o16 = q16 + (size_t)M * 2 * C3;
    HIP_OK(launch_to_p16(d_qkv, C3, nullptr, M, C3, C3, q16, 2 * C3, 1.0f, s));
    AttnArgs a;
    a.qkv16 = q16; a.ld16 = 2 * C3; a.out16 = o16; a.ldo16 = 2 * H * D; a.mask = d_mask;
    a.B = B; a.T = T; a.H = H; a.D = D; a.scale = scale; a.mask_mode = mask_mode;
    HIP_OK(launch_attention(a, s));
    HIP_OK(launch_from_p16(o16, 2 * H * D, M, H * D, a.out_lscale, d_out, H * D, s));
    return 0;
}

int mtts_row_stats(const float* d_x, int M, int C, int ld, float eps, float* d_mean, float* d_rstd, void* stream) {
    HIP_OK(launch_row_stats(d_x, M, C, ld, eps, d_mean, d_rstd, static_cast<hipStream_t>(stream)));
    return 0;
}

int mtts_channel_layernorm(const float* d_x, int B, int T, int C, const float* d_gamma, const float* d_beta, float eps, int act,
                           const float* d_film, const float* d_mask, float* d_y, void* stream) {
    if (B <= 0 || T <= 0) { set_error("mtts_channel_layernorm: empty batch"); return -1; }
    if (act != ACT_NONE && act != ACT_SILU) { set_error("mtts_channel_layernorm: act must be 0 (none) or 2 (SiLU)"); return -1; }
    LayerNormArgs a;
    a.x = d_x; a.ldx = C; a.y = d_y; a.ldy = C; a.M = B * T; a.C = C; a.T = T; a.gamma = d_gamma; a.beta = d_beta; a.eps = eps;
    a.act = act; a.film = d_film; a.mask = d_mask;
    HIP_OK(launch_layernorm(a, static_cast<hipStream_t>(stream)));
    return 0;
}

int64_t mtts_groupnorm_scratch_bytes(int B, int T, int G) { return (int64_t)B * gn_chunks_max(T) * G * 2 * (int64_t)sizeof(float); }

int mtts_groupnorm_mish(const float* d_y, const float* d_gamma, const float* d_beta, const float* d_mask, int B, int T, int C, int G,
                        float eps, float* d_out, void* d_scratch, void* stream) {
    hipStream_t s = static_cast<hipStream_t>(stream);
    HIP_OK(launch_gn_partial(d_y, B, T, C, G, static_cast<float*>(d_scratch), s));
    GnApplyArgs a;
    a.y = d_y; a.partial = static_cast<const float*>(d_scratch); a.gamma = d_gamma; a.beta = d_beta; a.mask = d_mask;
    a.out = d_out; a.B = B; a.T = T; a.C = C; a.G = G; a.eps = eps;
    HIP_OK(launch_gn_apply(a, s));
    return 0;
}

// Test entry for the transformer-block chain (tblock_chain.hip).  fp32 operands are converted to P16 images in d_scratch, the fp32
// panels (LayerNorm affines already folded: w1 / b1 for the FeedForward, w_qkv / b_qkv for the following block) are packed into a
// fragment stream on the host, and the P16 outputs are decoded back to fp32.  w_qkv == NULL: no q|k|v phase; inner == 0: no
// out-projection (the FeedForward alone on d_x).  h_* pointers are HOST memory, d_* device memory.
// the model's launch plan for M rows (test entry; no GPU): rows per workgroup and prefetch workgroups
int mtts_chain_plan(int M, int ch, int* qb, int* prefetch_wgs) {
    if (M <= 0 || (ch != 128 && ch != 256) || !qb || !prefetch_wgs) { set_error("mtts_chain_plan: bad argument"); return -1; }
    chain_plan(M, ch, 0, read_switches().chain_pf, qb, prefetch_wgs);
    return 0;
}
int64_t mtts_chain_stream_frags(int C, int inner, int ch, int n_qkv) {
    if (!chain_supported(C, inner, n_qkv) || (ch != 128 && ch != 256)) { set_error("mtts_chain_stream_frags: unsupported shape"); return -1; }
    return chain_stream_frags(C, inner, ch, n_qkv);
}
int mtts_chain_stream_pack(int C, int inner, int ch, int n_qkv, const float* h_w_out, const float* h_w1, const float* h_w2,
                           const float* h_w_qkv, uint16_t* h_dst) {
    if (!chain_supported(C, inner, n_qkv) || (ch != 128 && ch != 256) || !h_w1 || !h_w2 || !h_dst || (inner && !h_w_out) || (n_qkv && !h_w_qkv)) {
        set_error("mtts_chain_stream_pack: unsupported shape or null panel");
        return -1;
    }
    chain_stream_pack(C, inner, ch, n_qkv, h_w_out, h_w1, h_w2, h_w_qkv, h_dst, nullptr);
    return 0;
}
// pair form: fragments per (half, wave), and the packing of the 2 x 8 streams (host only)
int64_t mtts_chain_stream_frags_pair(int C, int inner, int ch, int n_qkv) {
    if (!chain_supported_pair(C, inner, ch, n_qkv) || (ch != 128 && ch != 256)) { set_error("mtts_chain_stream_frags_pair: unsupported shape"); return -1; }
    return chain_stream_frags_pair(C, inner, ch, n_qkv);
}
int mtts_chain_stream_pack_pair(int C, int inner, int ch, int n_qkv, const float* h_w_out, const float* h_w1, const float* h_w2,
                                const float* h_w_qkv, uint16_t* h_dst) {
    if (!chain_supported_pair(C, inner, ch, n_qkv) || (ch != 128 && ch != 256) || !h_w_out || !h_w1 || !h_w2 || !h_dst || (n_qkv && !h_w_qkv)) {
        set_error("mtts_chain_stream_pack_pair: unsupported shape or null panel");
        return -1;
    }
    chain_stream_pack_pair(C, inner, ch, n_qkv, h_w_out, h_w1, h_w2, h_w_qkv, h_dst, nullptr);
    return 0;
}
int64_t mtts_tblock_chain_scratch_bytes(int M, int C, int inner, int n_qkv, int ch) {
    if (!chain_supported(C, inner, n_qkv)) return -1;
    int64_t stream = (int64_t)chain_stream_frags(C, inner, ch, n_qkv) * CHAIN_WAVES * 1024;
    if (chain_supported_pair(C, inner, ch, n_qkv)) stream = std::max<int64_t>(stream, (int64_t)chain_stream_frags_pair(C, inner, ch, n_qkv) * 2 * CHAIN_WAVES * 1024);
    const int64_t pair_scratch = 2 * ((int64_t)M + 64) * C * 4 + 2 * ((int64_t)M / 32 + 2) * 4 + 512;       // partial sums + flags of the pair form
    return stream + (int64_t)M * 4 * (inner + 2 * C + n_qkv) + 4 * (int64_t)(2 * n_qkv + 18 * C) + 4096 + pair_scratch;
}
int mtts_tblock_chain(const float* d_att, const float* d_x, int M, int C, int inner, const float* h_w_out, const float* h_b_out,
                      const float* h_w1, const float* h_b1, const float* h_p0, const float* h_p1, const float* h_w2, const float* h_b2,
                      const float* h_w_qkv, const float* h_b_qkv, int n_qkv, const float* d_out_mask, int qb, int ch, float* d_x_out,
                      float* d_qkv_out, void* d_scratch, void* stream) {
    return mtts_tblock_chain_timed(d_att, d_x, M, C, inner, h_w_out, h_b_out, h_w1, h_b1, h_p0, h_p1, h_w2, h_b2, h_w_qkv, h_b_qkv, n_qkv,
                                   d_out_mask, qb, ch, d_x_out, d_qkv_out, d_scratch, stream, 0, nullptr);
}
static int tblock_chain_entry(bool pair, const float* d_att, const float* d_x, int M, int C, int inner, const float* h_w_out, const float* h_b_out,
                              const float* h_w1, const float* h_b1, const float* h_p0, const float* h_p1, const float* h_w2, const float* h_b2,
                              const float* h_w_qkv, const float* h_b_qkv, int n_qkv, const float* d_out_mask, int qb, int ch, float* d_x_out,
                              float* d_qkv_out, void* d_scratch, void* stream, int repeat, float* h_ms) {
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (!h_w_qkv) n_qkv = 0;
    if (!chain_supported(C, inner, n_qkv) || !d_x || !h_w1 || !h_w2 || !d_scratch || !d_x_out) { set_error("mtts_tblock_chain: unsupported shape or null buffer"); return -1; }
    if (pair && !chain_supported_pair(C, inner, ch, n_qkv)) { set_error("mtts_tblock_chain_pair: unsupported shape"); return -1; }
    const long frags = pair ? chain_stream_frags_pair(C, inner, ch, n_qkv) : chain_stream_frags(C, inner, ch, n_qkv);
    std::vector<uint16_t> hs((size_t)frags * (pair ? 2 : 1) * CHAIN_WAVES * 512);
    if (pair) chain_stream_pack_pair(C, inner, ch, n_qkv, h_w_out, h_w1, h_w2, h_w_qkv, hs.data(), nullptr);
    else chain_stream_pack(C, inner, ch, n_qkv, h_w_out, h_w1, h_w2, h_w_qkv, hs.data(), nullptr);
    std::vector<float> hc((size_t)18 * C + 2 * (size_t)n_qkv, 0.f);         // wsum1 | b1 | p0 | p1 | b_out | b2 | wsum_qkv | b_qkv
    for (int n = 0; n < 4 * C; ++n) {
        double a = 0.0;
        for (int k = 0; k < C; ++k) a += (double)h_w1[(size_t)n * C + k];
        hc[n] = (float)a;
        hc[4 * C + n] = h_b1 ? h_b1[n] : 0.f;
        hc[8 * C + n] = h_p0[n];
        hc[12 * C + n] = h_p1[n];
    }
    for (int n = 0; n < C; ++n) { hc[16 * C + n] = (inner && h_b_out) ? h_b_out[n] : 0.f; hc[17 * C + n] = h_b2 ? h_b2[n] : 0.f; }
    for (int n = 0; n < n_qkv; ++n) {
        double a = 0.0;
        for (int k = 0; k < C; ++k) a += (double)h_w_qkv[(size_t)n * C + k];
        hc[18 * C + n] = (float)a;
        hc[18 * C + n_qkv + n] = h_b_qkv ? h_b_qkv[n] : 0.f;
    }
    char* sc = static_cast<char*>(d_scratch);
    _Float16* d_stream = reinterpret_cast<_Float16*>(sc); sc += hs.size() * 2;
    float* d_c = reinterpret_cast<float*>(sc); sc += hc.size() * 4;
    sc = reinterpret_cast<char*>((reinterpret_cast<uintptr_t>(sc) + 255) & ~uintptr_t(255));
    _Float16* att16 = reinterpret_cast<_Float16*>(sc); sc += (size_t)M * inner * 4;
    _Float16* x16 = reinterpret_cast<_Float16*>(sc); sc += (size_t)M * C * 4;
    _Float16* xo16 = reinterpret_cast<_Float16*>(sc); sc += (size_t)M * C * 4;
    _Float16* q16 = reinterpret_cast<_Float16*>(sc); sc += (size_t)M * n_qkv * 4;
    sc = reinterpret_cast<char*>((reinterpret_cast<uintptr_t>(sc) + 255) & ~uintptr_t(255));
    float* d_part = reinterpret_cast<float*>(sc); sc += 2 * ((size_t)M + 64) * C * 4;
    unsigned int* d_flag = reinterpret_cast<unsigned int*>(sc);
    if (pair) HIP_OK(hipMemsetAsync(d_flag, 0, 2 * ((size_t)M / 32 + 2) * 4, s));
    HIP_OK(hipMemcpyAsync(d_stream, hs.data(), hs.size() * 2, hipMemcpyHostToDevice, s));
    HIP_OK(hipMemcpyAsync(d_c, hc.data(), hc.size() * 4, hipMemcpyHostToDevice, s));
    HIP_OK(hipStreamSynchronize(s));                      // (the host vectors go out of scope)
    if (inner) HIP_OK(launch_to_p16(d_att, inner, nullptr, M, inner, inner, att16, 2 * inner, 2048.0f, s));
    HIP_OK(launch_to_p16(d_x, C, nullptr, M, C, C, x16, 2 * C, 2048.0f, s));
    ChainArgs a;
    a.M = M; a.C = C; a.inner = inner; a.att16 = att16; a.ld_att = 2 * inner; a.x16 = x16; a.ld_x = 2 * C;
    a.wstream = d_stream; a.stream_frags = frags;
    a.consts = d_c;
    if (n_qkv) { a.wsum_qkv = d_c + 18 * C; a.b_qkv = d_c + 18 * C + n_qkv; a.n_qkv = n_qkv; a.qkv16 = q16; a.ld_qkv = 2 * n_qkv; }
    a.x_out = xo16; a.ld_out = 2 * C; a.x_out_mask = d_out_mask;
    a.qb = qb; a.ch = ch;
    a.pf_wgs = read_switches().chain_pf;
    if (pair) { a.pair = 1; a.pair_part = d_part; a.pair_flag = d_flag; a.pair_epoch = 1; a.pf_wgs = a.pf_wgs ? 16 : 0; }
#ifdef MTTS_CHAIN_STAMP
    a.kstamp = reinterpret_cast<unsigned long long*>(d_qkv_out);      // (diagnostic build: the stamps land in the q|k|v output buffer)
#endif
    HIP_OK(launch_tblock_chain(a, s));
#ifdef MTTS_CHAIN_STAMP
    HIP_OK(hipStreamSynchronize(s));
    return 0;
#endif
    if (repeat > 0 && h_ms) {                             // measurement: `repeat` further launches between two events
        hipEvent_t e0, e1;
        HIP_OK(hipEventCreate(&e0));
        HIP_OK(hipEventCreate(&e1));
        HIP_OK(hipEventRecord(e0, s));
        for (int i = 0; i < repeat; ++i) { if (pair) a.pair_epoch = 2 + i; HIP_OK(launch_tblock_chain(a, s)); }
        HIP_OK(hipEventRecord(e1, s));
        HIP_OK(hipEventSynchronize(e1));
        HIP_OK(hipEventElapsedTime(h_ms, e0, e1));
        *h_ms /= (float)repeat;
        (void)hipEventDestroy(e0);
        (void)hipEventDestroy(e1);
    }
    HIP_OK(launch_from_p16(xo16, 2 * C, M, C, 2048.0f, d_x_out, C, s));
    if (n_qkv && d_qkv_out) HIP_OK(launch_from_p16(q16, 2 * n_qkv, M, n_qkv, 1.0f, d_qkv_out, n_qkv, s));
    return 0;
}

int mtts_tblock_chain_timed(const float* d_att, const float* d_x, int M, int C, int inner, const float* h_w_out, const float* h_b_out,
                            const float* h_w1, const float* h_b1, const float* h_p0, const float* h_p1, const float* h_w2, const float* h_b2,
                            const float* h_w_qkv, const float* h_b_qkv, int n_qkv, const float* d_out_mask, int qb, int ch, float* d_x_out,
                            float* d_qkv_out, void* d_scratch, void* stream, int repeat, float* h_ms) {
    return tblock_chain_entry(false, d_att, d_x, M, C, inner, h_w_out, h_b_out, h_w1, h_b1, h_p0, h_p1, h_w2, h_b2, h_w_qkv, h_b_qkv, n_qkv,
                              d_out_mask, qb, ch, d_x_out, d_qkv_out, d_scratch, stream, repeat, h_ms);
}
// the pair form of the same launch (two workgroups per row tile; ChainArgs::pair): qb = 48 or 32, at most 120 row tiles
int mtts_tblock_chain_pair_timed(const float* d_att, const float* d_x, int M, int C, int inner, const float* h_w_out, const float* h_b_out,
                                 const float* h_w1, const float* h_b1, const float* h_p0, const float* h_p1, const float* h_w2, const float* h_b2,
                                 const float* h_w_qkv, const float* h_b_qkv, int n_qkv, const float* d_out_mask, int qb, int ch, float* d_x_out,
                                 float* d_qkv_out, void* d_scratch, void* stream, int repeat, float* h_ms) {
    return tblock_chain_entry(true, d_att, d_x, M, C, inner, h_w_out, h_b_out, h_w1, h_b1, h_p0, h_p1, h_w2, h_b2, h_w_qkv, h_b_qkv, n_qkv,
                              d_out_mask, qb, ch, d_x_out, d_qkv_out, d_scratch, stream, repeat, h_ms);
}

// ---- the one-plane chain of the 16-bit storage modes (tblock_chain_h16.hip): host-only stream functions and the unit entry
int64_t mtts_chain_stream_frags_h16(int C, int inner, int ch, int n_qkv) {
    if (!chain_h16_supported(C, inner, ch, n_qkv)) { set_error("mtts_chain_stream_frags_h16: unsupported shape"); return -1; }
    return chain_h16_stream_frags(C, inner, ch, n_qkv);
}
int mtts_chain_stream_pack_h16(int C, int inner, int ch, int n_qkv, const float* h_w_out, const float* h_w1, const float* h_w2,
                               const float* h_w_qkv, int bf16, uint16_t* h_dst, int* saturates) {
    if (!chain_h16_supported(C, inner, ch, n_qkv) || !h_w1 || !h_w2 || !h_dst || (inner && !h_w_out) || (n_qkv && !h_w_qkv)) {
        set_error("mtts_chain_stream_pack_h16: unsupported shape or null panel");
        return -1;
    }
    bool sat = false;
    chain_h16_stream_pack(C, inner, ch, n_qkv, h_w_out, h_w1, h_w2, h_w_qkv, bf16 != 0, h_dst, &sat);
    if (sat && saturates) *saturates = 1;
    return 0;
}
int64_t mtts_tblock_chain_h16_scratch_bytes(int M, int C, int inner, int n_qkv, int ch) {
    if (M <= 0 || !chain_h16_supported(C, inner, ch, n_qkv)) return -1;
    const int64_t stream = (int64_t)chain_h16_stream_frags(C, inner, ch, n_qkv) * CHAIN_WAVES * 1024;
    return stream + (int64_t)M * 2 * (inner + 2 * C + n_qkv) + 4 * (int64_t)(2 * n_qkv + 18 * C) + 4096;
}
// row sums of a panel rounded to the stream's 16-bit type (what the kernel multiplies with)
static double rounded_row_sum(const float* w, int K, bool bf16) {
    double a = 0.0;
    for (int k = 0; k < K; ++k) a += bf16 ? (double)(float)(__bf16)w[k] : (double)(float)(_Float16)fminf(fmaxf(w[k], -65504.f), 65504.f);
    return a;
}
int mtts_tblock_chain_h16_timed(const float* d_att, const float* d_x, int M, int C, int inner, const float* h_w_out, const float* h_b_out,
                                const float* h_w1, const float* h_b1, const float* h_p0, const float* h_p1, const float* h_w2,
                                const float* h_b2, const float* h_w_qkv, const float* h_b_qkv, int n_qkv, const float* d_out_mask,
                                int bf16, int qb, int ch, int pf_wgs, float* d_x_out, float* d_qkv_out, void* d_scratch, void* stream,
                                int repeat, float* h_ms) {
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (!h_w_qkv) n_qkv = 0;
    if (M <= 0 || !chain_h16_supported(C, inner, ch, n_qkv) || !d_x || !h_w1 || !h_w2 || !h_p0 || !h_p1 || !d_scratch || !d_x_out || (inner && (!d_att || !h_w_out)) ||
        (n_qkv && !d_qkv_out)) {
        set_error("mtts_tblock_chain_h16: unsupported shape or null buffer");
        return -1;
    }
    const bool bf = bf16 != 0;
    const long frags = chain_h16_stream_frags(C, inner, ch, n_qkv);
    std::vector<uint16_t> hs((size_t)frags * CHAIN_WAVES * 512);
    chain_h16_stream_pack(C, inner, ch, n_qkv, h_w_out, h_w1, h_w2, h_w_qkv, bf, hs.data(), nullptr);
    std::vector<float> hc((size_t)18 * C + 2 * (size_t)n_qkv, 0.f);         // wsum1 | b1 | p0 | p1 | b_out | b2 | wsum_qkv | b_qkv
    for (int n = 0; n < 4 * C; ++n) {
        hc[n] = (float)rounded_row_sum(h_w1 + (size_t)n * C, C, bf);
        hc[4 * C + n] = h_b1 ? h_b1[n] : 0.f;
        hc[8 * C + n] = h_p0[n];
        hc[12 * C + n] = h_p1[n];
    }
    for (int n = 0; n < C; ++n) { hc[16 * C + n] = (inner && h_b_out) ? h_b_out[n] : 0.f; hc[17 * C + n] = h_b2 ? h_b2[n] : 0.f; }
    for (int n = 0; n < n_qkv; ++n) {
        hc[18 * C + n] = (float)rounded_row_sum(h_w_qkv + (size_t)n * C, C, bf);
        hc[18 * C + n_qkv + n] = h_b_qkv ? h_b_qkv[n] : 0.f;
    }
    char* sc = static_cast<char*>(d_scratch);
    void* d_stream = sc; sc += hs.size() * 2;
    float* d_c = reinterpret_cast<float*>(sc); sc += hc.size() * 4;
    sc = reinterpret_cast<char*>((reinterpret_cast<uintptr_t>(sc) + 255) & ~uintptr_t(255));
    _Float16* att16 = reinterpret_cast<_Float16*>(sc); sc += (size_t)M * inner * 2;
    _Float16* x16 = reinterpret_cast<_Float16*>(sc); sc += (size_t)M * C * 2;
    _Float16* xo16 = reinterpret_cast<_Float16*>(sc); sc += (size_t)M * C * 2;
    _Float16* q16 = reinterpret_cast<_Float16*>(sc); sc += (size_t)M * n_qkv * 2;
    HIP_OK(hipMemcpyAsync(d_stream, hs.data(), hs.size() * 2, hipMemcpyHostToDevice, s));
    HIP_OK(hipMemcpyAsync(d_c, hc.data(), hc.size() * 4, hipMemcpyHostToDevice, s));
    HIP_OK(hipStreamSynchronize(s));                      // (the host vectors go out of scope)
    if (inner) HIP_OK(launch_to_p16(d_att, inner, nullptr, M, inner, inner, att16, inner, 1.0f, s, nullptr, true, bf));
    HIP_OK(launch_to_p16(d_x, C, nullptr, M, C, C, x16, C, 1.0f, s, nullptr, true, bf));
    ChainH16Args a;
    a.M = M; a.C = C; a.inner = inner; a.att16 = att16; a.ld_att = inner; a.x16 = x16; a.ld_x = C; a.bf16 = bf;
    a.wstream = d_stream; a.stream_frags = frags;
    a.consts = d_c;
    if (n_qkv) { a.wsum_qkv = d_c + 18 * C; a.b_qkv = d_c + 18 * C + n_qkv; a.n_qkv = n_qkv; a.qkv16 = q16; a.ld_qkv = n_qkv; }
    a.x_out = xo16; a.ld_out = C; a.x_out_mask = d_out_mask;
    a.qb = qb; a.ch = ch; a.pf_wgs = pf_wgs;
    HIP_OK(launch_tblock_chain_h16(a, s));
    if (repeat > 0 && h_ms) {                             // measurement: `repeat` further launches between two events
        hipEvent_t e0, e1;
        HIP_OK(hipEventCreate(&e0));
        HIP_OK(hipEventCreate(&e1));
        HIP_OK(hipEventRecord(e0, s));
        for (int i = 0; i < repeat; ++i) HIP_OK(launch_tblock_chain_h16(a, s));
        HIP_OK(hipEventRecord(e1, s));
        HIP_OK(hipEventSynchronize(e1));
        HIP_OK(hipEventElapsedTime(h_ms, e0, e1));
        *h_ms /= (float)repeat;
        (void)hipEventDestroy(e0);
        (void)hipEventDestroy(e1);
    }
    HIP_OK(launch_from_h16(xo16, C, M, C, bf, d_x_out, C, s));
    if (n_qkv) HIP_OK(launch_from_h16(q16, n_qkv, M, n_qkv, bf, d_qkv_out, n_qkv, s));
    return 0;
}
int mtts_tblock_chain_h16(const float* d_att, const float* d_x, int M, int C, int inner, const float* h_w_out, const float* h_b_out,
                          const float* h_w1, const float* h_b1, const float* h_p0, const float* h_p1, const float* h_w2,
                          const float* h_b2, const float* h_w_qkv, const float* h_b_qkv, int n_qkv, const float* d_out_mask, int bf16,
                          int qb, int ch, int pf_wgs, float* d_x_out, float* d_qkv_out, void* d_scratch, void* stream) {
    return mtts_tblock_chain_h16_timed(d_att, d_x, M, C, inner, h_w_out, h_b_out, h_w1, h_b1, h_p0, h_p1, h_w2, h_b2, h_w_qkv, h_b_qkv, n_qkv,
                                       d_out_mask, bf16, qb, ch, pf_wgs, d_x_out, d_qkv_out, d_scratch, stream, 0, nullptr);
}

// ------------------------------------------------------------------------------------------------ measurement
int mtts_gemm_terms(mtts_ctx* c) { return c ? (c->bf16 ? 17 : c->half16 ? 16 : c->fast16 ? 1 : c->gemm_terms) : read_switches().gemm_terms; }

int mtts_prof_enable(mtts_ctx* c, int on) {
    if (!c) { set_error("null context"); return -1; }
    c->prof_on = on != 0;
    return 0;
}
int mtts_prof_reset(mtts_ctx* c) {
    if (!c) { set_error("null context"); return -1; }
    c->prof.clear();
    c->ev_used = 0;
    return 0;
}
int mtts_prof_read(mtts_ctx* c, int klass, int64_t* launches, double* ms, double* flops, double* bytes) {
    if (!c) { set_error("null context"); return -1; }
    int64_t n = 0;
    double t = 0, f = 0, by = 0;
    if (!c->prof.empty()) HIP_OK(hipEventSynchronize(c->prof.back().e1));
    for (const ProfRec& r : c->prof) {
        if (r.klass != klass) continue;
        float el = 0.f;
        HIP_OK(hipEventElapsedTime(&el, r.e0, r.e1));
        t += el;
        f += r.flops;
        by += r.bytes;
        ++n;
    }
    if (launches) *launches = n;
    if (ms) *ms = t;
    if (flops) *flops = f;
    if (bytes) *bytes = by;
    return 0;
}

// Per-launch records of the event pass, in launch order: out[i] = (class, ms, flops, bytes); returns the number written.
int64_t mtts_prof_records(mtts_ctx* c, double* out, int64_t max_records) {
    if (!c || !out) { set_error("mtts_prof_records: bad argument"); return -1; }
    if (!c->prof.empty()) HIP_OK(hipEventSynchronize(c->prof.back().e1));
    int64_t n = 0;
    for (const ProfRec& r : c->prof) {
        if (n >= max_records) break;
        float el = 0.f;
        HIP_OK(hipEventElapsedTime(&el, r.e0, r.e1));
        out[4 * n] = r.klass; out[4 * n + 1] = el; out[4 * n + 2] = r.flops; out[4 * n + 3] = r.bytes;
        ++n;
    }
    return n;
}

// the instantiation names of the same records (kernels.h g_kernel_tag), '\n'-separated, "-" for untagged launches
int64_t mtts_prof_tags(mtts_ctx* c, char* out, int64_t max_bytes) {
    if (!c || !out || max_bytes < 2) { set_error("mtts_prof_tags: bad argument"); return -1; }
    std::string all;
    for (const ProfRec& r : c->prof) { all += r.tag.empty() ? "-" : r.tag.c_str(); all += '\n'; }
    if ((int64_t)all.size() + 1 > max_bytes) { set_error("mtts_prof_tags: buffer too small"); return -1; }
    std::memcpy(out, all.c_str(), all.size() + 1);
    return (int64_t)c->prof.size();
}

// ================================================================================================ Vocos head
static int vocos_pack(mtts_vocos* v) {
    mtts_ctx* c = &v->base;
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

mtts_vocos* mtts_vocos_create(int n_mels, int dim, int inter, int layers, int n_fft, int hop) {
    if (n_mels <= 0 || (n_mels & 3) || dim <= 0 || (dim & 3) || dim > 2048 || inter <= 0 || (inter & 3) || layers < 0 || n_fft <= 0 ||
        (n_fft & 3) || hop <= 0 || n_fft % hop) {
        set_error("mtts_vocos_create: unsupported shape (channels multiples of 4, dim <= 2048, hop divides n_fft)");
        return nullptr;
    }
    mtts_vocos* v = new mtts_vocos();
    v->base.gemm_terms = read_switches().gemm_terms;
    v->n_mels = n_mels; v->dim = dim; v->inter = inter; v->layers = layers; v->n_fft = n_fft; v->hop = hop;
    return v;
}
void mtts_vocos_destroy(mtts_vocos* v) {
    if (!v) return;
    for (hipEvent_t e : v->base.ev_pool) (void)hipEventDestroy(e);
    delete v;
}
int mtts_vocos_set_tensor(mtts_vocos* v, const char* key, const float* h, int64_t numel) {
    if (!v) { set_error("null context"); return -1; }
    return mtts_set_tensor(&v->base, key, h, numel);
}
int64_t mtts_vocos_weights_bytes(mtts_vocos* v) {
    if (!v) { set_error("null context"); return -1; }
    if (!v->base.packed && vocos_pack(v)) return -1;
    return (int64_t)(v->base.image.size() * sizeof(float));
}
int mtts_vocos_upload_weights(mtts_vocos* v, void* d_weights, int64_t bytes) {
    if (!v || !d_weights) { set_error("mtts_vocos_upload_weights: bad argument"); return -1; }
    if (!v->base.packed && vocos_pack(v)) return -1;
    mtts_ctx* c = &v->base;
    if ((size_t)bytes < c->image.size() * sizeof(float)) { set_error("weight buffer too small"); return -1; }
    HIP_OK(hipMemcpy(d_weights, c->image.data(), c->image.size() * sizeof(float), hipMemcpyHostToDevice));
    c->d_image = static_cast<float*>(d_weights);
    c->uploaded = true;
    return 0;
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
    mtts_ctx* c = &v->base;
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
    if (!d_ws) { set_error("mtts_vocos_ragged_status: null workspace"); return -1; }
    hipStream_t s = static_cast<hipStream_t>(stream);
    int st[3] = {0, 0, 0};
    HIP_OK(hipMemcpyAsync(st, d_ws, sizeof(st), hipMemcpyDeviceToHost, s));
    HIP_OK(hipStreamSynchronize(s));
    if (st[0] != 0) {
        set_error("mtts_vocos_decode_ragged: lengths[" + std::to_string(st[0] - 1) + "] = " + std::to_string(st[1]) +
                  " is outside [1, T = " + std::to_string(st[2]) + "]");
        return -1;
    }
    return 0;
}

// ---- waveform finish (waveform.hip)
static int wave_window(int sample_rate) { return (int)(0.01 * (double)sample_rate); }       // reference inference.py:270
int64_t mtts_waveform_workspace_bytes(int64_t ld, int B, int sample_rate) {
    const int win = wave_window(sample_rate);
    if (ld < 0 || B <= 0 || win <= 0) { set_error("mtts_waveform_workspace_bytes: bad shape"); return -1; }
    WS ws(nullptr, 0);
    ws.f((size_t)B * ((ld + WAVE_CHUNK - 1) / WAVE_CHUNK + 1));
    ws.f((size_t)B * (ld / win + 1));
    return (int64_t)ws.off + 256;
}
int mtts_waveform_finish(float* d_audio, int64_t ld, const int64_t* d_lengths, int hop, int B, int sample_rate, double threshold_db,
                         float* d_scale, int64_t* d_out_lengths, void* d_ws, int64_t ws_bytes, void* stream) {
    WaveFinishArgs a;
    a.win = wave_window(sample_rate);
    if (!d_audio || !d_lengths || !d_scale || !d_out_lengths || !d_ws || B <= 0 || B > 65535 || ld < 0 || hop < 0 || a.win <= 0) {
        set_error("mtts_waveform_finish: bad argument");
        return -1;
    }
    if ((ld & 3) || (reinterpret_cast<uintptr_t>(d_audio) & 15)) {
        set_error("mtts_waveform_finish: rows must be 16-byte aligned (ld a multiple of 4 samples)");
        return -1;
    }
    WS ws(d_ws, (size_t)ws_bytes);
    a.peaks = ws.f((size_t)B * ((ld + WAVE_CHUNK - 1) / WAVE_CHUNK + 1));
    a.rms = ws.f((size_t)B * (ld / a.win + 1));
    if (ws.overflow) { set_error("mtts_waveform_finish: workspace too small"); return -1; }
    a.audio = d_audio; a.ld = ld; a.lengths = d_lengths; a.hop = hop; a.B = B;
    a.thr = (float)std::pow(10.0, threshold_db / 20.0);         // reference inference.py:271; torch compares the fp32 RMS in fp32
    a.scale = d_scale; a.out_lengths = d_out_lengths;
    HIP_OK(launch_wave_finish(a, static_cast<hipStream_t>(stream)));
    return 0;
}

}  // extern "C"

// ================================================================================================ style encoder
// StyleEncoder (reference matcha/models/style_encoder.py:42-72): n_layers x { x * mask -> Conv1d(k5, pad 2) -> ReLU }, masked mean
// over time, Linear(hidden -> spk_emb_dim) twice.  Tensors are registered under the reference's names ("convs.0.weight", ...,
// "proj_enc.weight", "proj_dur.bias").
static int style_pack(mtts_style* v) {
    mtts_ctx* c = &v->base;
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
    v->base.gemm_terms = read_switches().gemm_terms;
    v->n_feats = n_feats; v->hidden = hidden; v->layers = n_layers; v->emb = spk_emb_dim;
    return v;
}
void mtts_style_destroy(mtts_style* v) {
    if (!v) return;
    for (hipEvent_t e : v->base.ev_pool) (void)hipEventDestroy(e);
    delete v;
}
int mtts_style_set_tensor(mtts_style* v, const char* key, const float* h, int64_t numel) {
    if (!v) { set_error("null context"); return -1; }
    return mtts_set_tensor(&v->base, key, h, numel);
}
int64_t mtts_style_weights_bytes(mtts_style* v) {
    if (!v) { set_error("null context"); return -1; }
    if (!v->base.packed && style_pack(v)) return -1;
    return (int64_t)(v->base.image.size() * sizeof(float));
}
int mtts_style_upload_weights(mtts_style* v, void* d_weights, int64_t bytes) {
    if (!v || !d_weights) { set_error("mtts_style_upload_weights: bad argument"); return -1; }
    if (!v->base.packed && style_pack(v)) return -1;
    mtts_ctx* c = &v->base;
    if ((size_t)bytes < c->image.size() * sizeof(float)) { set_error("weight buffer too small"); return -1; }
    HIP_OK(hipMemcpy(d_weights, c->image.data(), c->image.size() * sizeof(float), hipMemcpyHostToDevice));
    c->d_image = static_cast<float*>(d_weights);
    c->uploaded = true;
    return 0;
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
    mtts_ctx* c = &v->base;
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
