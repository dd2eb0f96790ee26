// Weight packing on the host: the packer every component's image is built with (host.h Packer) and the image of the path's
// context (text encoder, decoder, the transformer blocks' chain streams in their three forms).  The Vocos head and the style encoder
// pack theirs next to their launch sequences (vocos.hip, style_encoder.hip).
#include "host.h"

namespace mtts {

const std::vector<float>* Packer::get(const std::string& key, size_t numel) {
    auto it = c->raw.find(key);
    if (it == c->raw.end()) { fail("missing tensor " + key); return nullptr; }
    if (it->second.size() != numel) {
        fail("tensor " + key + " has " + std::to_string(it->second.size()) + " elements, expected " + std::to_string(numel));
        return nullptr;
    }
    return &it->second;
}
size_t Packer::alloc(size_t n) {
    size_t off = (c->image.size() + 63) & ~size_t(63);
    c->image.resize(off + n, 0.f);
    return off;
}
Vec Packer::vec(const std::string& key, int n) {
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
Vec Packer::bias_group_stats(const Panel& p, int G) {
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
// bf16 split planes of a finished fp32 panel (split modes only)
void Packer::add_planes(Panel& p) {
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
Panel Packer::panel_from(const float* w, const float* bias, int kind, int N, int C, int ntaps) {
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
Panel Packer::panel_multi(const std::vector<std::string>& wkeys, const std::vector<std::string>& bkeys, int kind, int N_each, int C,
                          int ntaps, int kT, const int* tsel, const std::vector<float>* col_scale, const std::vector<float>* col_shift) {
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

int pack_all(mtts_ctx* c, bool dry) {
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
            const int ch = chain_packed_ch(C, c->sw.chain_ch);
            if (!chain_supported(C, inner, nq) || !chain_shape_exists(C, 32, ch) || t.ff1.N != 4 * C || t.ff1.ktap != C || t.ff2.ktap != 4 * C || t.out.ktap != inner) continue;
            if (nq && D.tb[k + 1].qkv.ktap != C) continue;
            t.chain_frags = chain_stream_frags(C, inner, ch, nq);
            t.chain_ch = ch;
            t.chain_nqkv = nq;
            t.next = nq ? (int)k + 1 : -1;
            t.chain = P.alloc((size_t)t.chain_frags * CHAIN_WAVES * 256);
            if (tblock_pair_possible(c->sw, C, inner, nq, ch)) {      // only where the launch decision can take the pair form
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
            const int ch = chain_packed_ch(C, c->sw.chain_ch);
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

}  // namespace mtts
