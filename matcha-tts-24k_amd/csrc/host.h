// What the host translation units share (model.hip, pack.hip, decoder.hip, encoder.hip, the host halves of vocos.hip,
// waveform.hip and style_encoder.hip, the ragged-batch entries, unit_entries.hip): error and launch macros, the launch check and
// the status reader of the ragged-batch contract, the profiling wrappers around a launch, the
// workspace carver, the packer's declaration and the weight life cycle of a component.  model.h is the data model, kernels.h the
// kernel interface; nothing here is visible outside csrc/.
#pragma once
#include "model.h"

#include <cmath>
#include <cstring>

namespace mtts {

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

// ------------------------------------------------------------------------------------------------ the ragged-batch contract
// After a launch (or any call that returns a hipError_t): 0, or -1 with the error "<what>: <hip error string>".  (Both helpers
// are static: they add nothing to the symbols the library exports.)
static inline int launched(const char* what, hipError_t e = hipGetLastError()) {
    if (e == hipSuccess) return 0;
    set_error(std::string(what) + ": " + hipGetErrorString(e));
    return -1;
}
// What every *_status entry does before it words its verdict: n header words of the call's workspace to the host.  The one place
// that waits for the stream.  `who` is the entry's name in the error texts.
template <class T>
static int read_status(const char* who, const void* d_ws, void* stream, T* words, size_t n) {
    if (!d_ws) { set_error(std::string(who) + ": null workspace"); return -1; }
    hipStream_t s = static_cast<hipStream_t>(stream);
    hipError_t e = hipMemcpyAsync(words, d_ws, n * sizeof(T), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    return launched(who, e);
}
template <class T, size_t N>
static int read_status(const char* who, const void* d_ws, void* stream, T (&words)[N]) { return read_status(who, d_ws, stream, words, N); }

// ------------------------------------------------------------------------------------------------ profiling wrappers
inline int prof_begin(Component* c, int klass, double flops, double bytes, hipStream_t s) {
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
inline int prof_end(Component* c, hipStream_t s) {
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

inline int run_gemm(Component* c, const GemmArgs& a0, hipStream_t s) {
    GemmArgs a = a0;
    a.range_flag = c->cur_flag;
    a.half16 = c->half_now && a.a16_0 != nullptr;
    a.bf16 = a.half16 && c->bf16;
    a.store_wt = (c->store_wt & WT_GEMM) != 0;
    LAUNCHB(c, 0, gemm_flops(a), gemm_bytes(a), s, launch_gemm(a, s));
    return 0;
}
inline int run_attn(Component* c, const AttnArgs& a0, hipStream_t s) {
    AttnArgs a = a0;
    a.range_flag = c->cur_flag;
    a.half16 = c->half_now && a.qkv16 != nullptr;
    a.bf16 = a.half16 && c->bf16;
    a.store_wt = (c->store_wt & WT_ATTN) != 0;
    LAUNCHB(c, 1, attn_flops(a), attn_bytes(a), s, launch_attention(a, s));
    return 0;
}
inline int run_gn_apply(Component* c, const GnApplyArgs& a0, hipStream_t s) {
    GnApplyArgs a = a0;
    a.range_flag = c->cur_flag;
    a.half16 = c->half_now && a.out16 != nullptr;
    a.bf16 = a.half16 && c->bf16;
    LAUNCH(c, 2, 0, s, launch_gn_apply(a, s));
    return 0;
}

// The sticky range flag of a call = the first word of its workspace, cleared here (include/mtts.h "range guard").
inline int begin_call(Component* c, void* d_ws, hipStream_t s) {
    c->cur_flag = static_cast<unsigned int*>(d_ws);
    // a kernel, not hipMemsetAsync: a captured memset node of one HIP graph was seen to write another instantiated graph's
    // bytes (pointer-like words in this header) after a second context captured its own graph (ROCm 7.2); kernel nodes are safe
    HIP_OK(launch_fill_cols(static_cast<float*>(d_ws), 1, 64, 0, 64, 0.f, s));
    return 0;
}

// Launch plan of a chain launch over M rows (decoder.hip; mtts_chain_plan reports it)
void chain_plan(int M, int ch, int qb_forced, int want, int* qb, int* pf);
// How a transformer block's row-local part runs in the default (P16) arithmetic -- THE launch-form decision (decoder.hip), shared by
// transformer_block, the packer and mtts_tblock_plan.  form 0: the four tiled GEMM launches; 1: the chain launch; 2: its pair form.
// For forms 1 and 2 (C, qb, ch) is a shape of kernels.h chain_shape_exists, grid the row-tile workgroups and pf the prefetch ones.
struct TBlockPlan { int form = 0, qb = 0, grid = 0, pf = 0; };
// n_qkv: width of the following block's q|k|v (0 for the last block of a run); ch: the hidden chunk the block's streams are packed
// for (chain_packed_ch); has_chain / has_pair: that stream is in the weight image and the call can use it.
TBlockPlan tblock_plan(const Switches& sw, int C, int inner, int n_qkv, int ch, int M, bool has_chain, bool has_pair);
// Hidden chunk the chain streams of a width-C block are packed for under MTTS_CHAIN_CH = chain_ch
inline int chain_packed_ch(int C, int chain_ch) { return (C == 384 && chain_ch == 256) ? 256 : 128; }
// Whether tblock_plan can answer "pair" for such a block at some row count and thresholds: what the packer packs a pair stream for.
// The pair form launches 48-row tiles, and it was measured at width 384 with hidden chunk 256 only (profiles/r03_pair_ab.log).
bool tblock_pair_possible(const Switches& sw, int C, int inner, int n_qkv, int ch);

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

// ------------------------------------------------------------------------------------------------ weight packing (pack.hip)
struct Packer {
    Component* c;
    bool ok = true;
    std::string why;
    int kq = GEMM_BK;          // K padding per tap of the panels being packed: 64 for the estimator in the 16-bit storage mode
    bool h16 = false;          // ... which also get the single fp16 plane (Panel::wh16)
    bool dry = false;          // layout only: offsets and sizes are computed (the registered tensors are still checked for presence and
                               // shape), nothing but zeros is written: mtts_import_weights takes the image itself from a cache
    explicit Packer(Component* ctx) : c(ctx) {}
    const std::vector<float>* get(const std::string& key, size_t numel);
    void fail(const std::string& m) { if (ok) { ok = false; why = m; } }
    size_t alloc(size_t n);
    Vec vec(const std::string& key, int n);
    Vec bias_group_stats(const Panel& p, int G);
    // kind 0 Linear [N,C]; 1 Conv1d [N,C,ntaps]; 2 ConvTranspose1d [C,N,kT] with taps tsel
    Panel panel(const std::string& wkey, const std::string& bkey, int kind, int N, int C, int ntaps, int kT = 0,
                const int* tsel = nullptr, const std::vector<float>* col_scale = nullptr,
                const std::vector<float>* col_shift = nullptr) {
        return panel_multi({wkey}, {bkey}, kind, N, C, ntaps, kT, tsel, col_scale, col_shift);
    }
    void add_planes(Panel& p);
    Panel panel_from(const float* w, const float* bias, int kind, int N, int C, int ntaps);
    Panel panel_multi(const std::vector<std::string>& wkeys, const std::vector<std::string>& bkeys, int kind, int N_each, int C,
                      int ntaps, int kT = 0, const int* tsel = nullptr, const std::vector<float>* col_scale = nullptr,
                      const std::vector<float>* col_shift = nullptr);
};
int pack_all(mtts_ctx* c, bool dry = false);
int pack_spk_grad(mtts_ctx* c);      // spk_grad.hip: the backward panels, from the registered tensors

// ------------------------------------------------------------------------------------------------ weight life cycle
// The same for the path's context, the Vocos head and the style encoder; `pack` is the component's packing function and `who` the
// exported function's name (the prefix of its error strings).
inline int set_tensor(Component* c, const char* key, const float* h, int64_t numel) {
    if (!c || !key || !h || numel < 0) { set_error("mtts_set_tensor: bad argument"); return -1; }
    c->raw[key].assign(h, h + numel);
    c->packed = false;
    c->uploaded = false;
    return 0;
}
template <class T>
int64_t weights_bytes(T* c, int (*pack)(T*)) {
    if (!c) { set_error("null context"); return -1; }
    if (!c->packed && pack(c)) return -1;
    return (int64_t)(c->image.size() * sizeof(float));
}
template <class T>
int upload_weights(T* c, int (*pack)(T*), const char* who, void* d_weights, int64_t bytes) {
    if (!c || !d_weights) { set_error(std::string(who) + ": bad argument"); return -1; }
    if (!c->packed && pack(c)) return -1;
    if ((size_t)bytes < c->image.size() * sizeof(float)) { set_error("weight buffer too small"); return -1; }
    HIP_OK(hipMemcpy(d_weights, c->image.data(), c->image.size() * sizeof(float), hipMemcpyHostToDevice));
    c->d_image = static_cast<float*>(d_weights);
    c->uploaded = true;
    return 0;
}

inline const float* W(const Component* c, size_t off) { return c->d_image + off; }

inline void panel_args(const Component* c, const Panel& p, GemmArgs& a) {
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
inline void rows_plain(GemmArgs& a, int B, int T) {
    a.B = B; a.T_in = T; a.T_out = T; a.in_stride = 1;
    a.out_T = T; a.out_stride = 1; a.out_off = 0;
}
inline void taps_centered(GemmArgs& a, int k) {
    for (int j = 0; j < k; ++j) a.tap_off[j] = j - k / 2;
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

inline int check_ready(const Component* c) {
    if (!c) { set_error("null context"); return -1; }
    if (!c->uploaded || !c->d_image) { set_error("weights not uploaded (mtts_upload_weights)"); return -1; }
    return 0;
}

}  // namespace mtts
