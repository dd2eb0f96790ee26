// The context behind mtts_ctx: error string, run-time switches, creation, the weight image's life cycle (set / pack / export / import /
// upload) and the profiler read-out.  Packing is in pack.hip, the launch sequences in encoder.hip and decoder.hip; the Vocos head,
// the waveform tail and the style encoder carry their host code and C ABI behind their kernels (vocos.hip, waveform.hip,
// style_encoder.hip), the context-free test entries of the kernels are in unit_entries.hip.
#include "host.h"

#include <cstdlib>
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
    w.store_wt = num("MTTS_STORE_WT", w.store_wt) & WT_ALL;
    return w;
}

}  // namespace mtts

using namespace mtts;

static int pack_ctx(mtts_ctx* c) { return pack_all(c); }

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
    c->store_wt = c->sw.store_wt;
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

void mtts_destroy(mtts_ctx* c) { delete c; }

int mtts_set_tensor(mtts_ctx* c, const char* key, const float* h, int64_t numel) {
    if (c) { c->grad.packed = false; c->grad.uploaded = false; }      // the backward panels (spk_grad.hip) are copies of these tensors
    return set_tensor(c, key, h, numel);
}

int64_t mtts_weights_bytes(mtts_ctx* c) { return weights_bytes(c, pack_ctx); }

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
    return upload_weights(c, pack_ctx, "mtts_upload_weights", d_weights, bytes);
}

// Test hook of the entry-point guard: holds the context as an entry point does, for `ms` milliseconds.
int mtts_debug_hold(mtts_ctx* c, int ms) {
    if (!c) { set_error("null context"); return -1; }
    CTX_GUARD(c);
    struct timespec ts = {ms / 1000, (long)(ms % 1000) * 1000000L};
    nanosleep(&ts, nullptr);
    return 0;
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

}  // extern "C"
