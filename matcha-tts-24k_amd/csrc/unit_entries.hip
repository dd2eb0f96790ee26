// Context-free test entries of the kernels (include/mtts.h "single kernels"): each converts fp32 operands to what its kernel
// reads, packs weights as the model does, launches, and converts back.  Nothing in the production path calls into this file.
// One static body per kernel family; the exports below are adapters that keep their own refusals and defaults.
#include "host.h"

using namespace mtts;

#define REFUSE_IF(cond, msg)                 \
    do {                                     \
        if (cond) { set_error(msg); return -1; } \
    } while (0)

// Scratch is carved in 256-byte steps from the 256-aligned start of the caller's buffer.
static size_t up256(size_t n) { return (n + 255) & ~size_t(255); }
struct Scratch {
    uintptr_t p;
    explicit Scratch(void* base) : p(up256(reinterpret_cast<uintptr_t>(base))) {}
    template <class T = char>
    T* carve(size_t bytes) { T* q = reinterpret_cast<T*>(p); p += up256(bytes); return q; }
};
static hipError_t fill16(void* image, unsigned short pattern, size_t halves, hipStream_t s) {
    return hipMemsetD16Async(reinterpret_cast<hipDeviceptr_t>(image), pattern, halves, s);
}
// the tag of the launcher that just ran, into an argument block's tag field
template <size_t N>
static void copy_tag(char (&tag)[N]) {
    if (g_kernel_tag) { std::strncpy(tag, g_kernel_tag, N - 1); tag[N - 1] = 0; }
}
// an image of ew halves per element back to fp32 rows (ew 2: P16 with residual scale lscale, ew 1: H16)
static hipError_t image_to_f32(const _Float16* image, int ld16, int M, int C, int ew, bool bf16, float lscale, float* out, hipStream_t s) {
    return ew == 1 ? launch_from_h16(image, ld16, M, C, bf16, out, C, s) : launch_from_p16(image, ld16, M, C, lscale, out, C, s);
}
static bool bad_pad(int p) { return p < 0 || (p & 7) || p > 4096; }

// row sums of a panel as the kernel multiplies it: exact for the two-plane stream, rounded to the one-plane stream's 16-bit type
static double plain_row_sum(const float* w, int K, bool) {
    double a = 0.0;
    for (int k = 0; k < K; ++k) a += (double)w[k];
    return a;
}
static double rounded_row_sum(const float* w, int K, bool bf16) {
    double a = 0.0;
    for (int k = 0; k < K; ++k) a += bf16 ? (double)(float)(__bf16)w[k] : (double)(float)(_Float16)fminf(fmaxf(w[k], -65504.f), 65504.f);
    return a;
}

// ---- the chain (tblock_chain.hip: P16 images, 2 halves per element, plain or pair; tblock_chain_h16.hip: H16 images, 1 half per
// element, fp16 or bfloat16).  The operands travel in a mtts_chain_args block (the positional entries fill one); ChainMode is what
// the block does not say.
struct ChainMode {
    int ew = 2;                 // halves per image element
    bool bf16 = false;          // (H16)
    int pf_wgs = 0;             // prefetch workgroups
    bool block = false;         // the argument-block entry: sentinel fill, guard rows behind the output images, tag and raw images out
    bool stamp = false;         // the positional P16 entry in a -DMTTS_CHAIN_STAMP build
    int repeat = 0;             // further launches between two events, their mean time to *h_ms
    float* h_ms = nullptr;
};
static mtts_chain_args chain_positional(const float* d_att, const float* d_x, int M, int C, int inner, const float* h_w_out, const float* h_b_out,
                                        const float* h_w1, const float* h_b1, const float* h_p0, const float* h_p1, const float* h_w2,
                                        const float* h_b2, const float* h_w_qkv, const float* h_b_qkv, int n_qkv, const float* d_out_mask, int qb,
                                        int ch, float* d_x_out, float* d_qkv_out) {
    mtts_chain_args g = {};
    g.d_att = d_att; g.d_x = d_x; g.M = M; g.C = C; g.inner = inner; g.h_w_out = h_w_out; g.h_b_out = h_b_out; g.h_w1 = h_w1; g.h_b1 = h_b1;
    g.h_p0 = h_p0; g.h_p1 = h_p1; g.h_w2 = h_w2; g.h_b2 = h_b2; g.h_w_qkv = h_w_qkv; g.h_b_qkv = h_b_qkv; g.n_qkv = h_w_qkv ? n_qkv : 0;
    g.d_out_mask = d_out_mask; g.qb = qb; g.ch = ch; g.d_x_out = d_x_out; g.d_qkv_out = d_qkv_out;
    return g;
}
// the fields ChainArgs and ChainH16Args share
template <class Args>
static void chain_fill(Args& a, const mtts_chain_args& g, int n_qkv, const void* d_stream, long frags, const float* d_c, _Float16* att16, int ld_att,
                       _Float16* x16, int ld_x, _Float16* xo16, int ld_out, _Float16* q16, int ld_qkv, int pf_wgs) {
    a.M = g.M; a.C = g.C; a.inner = g.inner; a.att16 = att16; a.ld_att = ld_att; a.x16 = x16; a.ld_x = ld_x;
    a.wstream = static_cast<decltype(a.wstream)>(d_stream); a.stream_frags = frags; a.consts = d_c;
    if (n_qkv) { a.wsum_qkv = d_c + 18 * g.C; a.b_qkv = d_c + 18 * g.C + n_qkv; a.n_qkv = n_qkv; a.qkv16 = q16; a.ld_qkv = ld_qkv; }
    a.x_out = xo16; a.ld_out = ld_out; a.x_out_mask = g.d_out_mask; a.qb = g.qb; a.ch = g.ch;
    a.range_flag = g.d_range_flag; a.pf_wgs = pf_wgs;
}
// g has passed its entry's checks; n_qkv is 0 without a q|k|v panel.  fp32 operands become images in d_scratch, the fp32 panels
// (LayerNorm affines already folded) a fragment stream packed on the host, the output images come back as fp32.
static int chain_run(mtts_chain_args& g, int n_qkv, const ChainMode& m, void* d_scratch, hipStream_t s) {
    const int M = g.M, C = g.C, inner = g.inner, ch = g.ch, ew = m.ew, Mg = M + (m.block ? MTTS_ENTRY_GUARD_ROWS : 0);
    const bool h16 = ew == 1, bf = h16 && m.bf16, pair = g.pair != 0;
    const float lscale = h16 ? 1.0f : 2048.0f;
    const long frags = h16 ? chain_h16_stream_frags(C, inner, ch, n_qkv) : pair ? chain_stream_frags_pair(C, inner, ch, n_qkv) : chain_stream_frags(C, inner, ch, n_qkv);
    std::vector<uint16_t> hs((size_t)frags * (pair ? 2 : 1) * CHAIN_WAVES * 512);
    if (h16) chain_h16_stream_pack(C, inner, ch, n_qkv, g.h_w_out, g.h_w1, g.h_w2, g.h_w_qkv, bf, hs.data(), nullptr);
    else if (pair) chain_stream_pack_pair(C, inner, ch, n_qkv, g.h_w_out, g.h_w1, g.h_w2, g.h_w_qkv, hs.data(), nullptr);
    else chain_stream_pack(C, inner, ch, n_qkv, g.h_w_out, g.h_w1, g.h_w2, g.h_w_qkv, hs.data(), nullptr);
    // the kernels' column constants: wsum1 | b1 | p0 | p1 | b_out | b2 | wsum_qkv | b_qkv
    double (*row_sum)(const float*, int, bool) = h16 ? rounded_row_sum : plain_row_sum;
    std::vector<float> hc((size_t)18 * C + 2 * (size_t)n_qkv, 0.f);
    for (int n = 0; n < 4 * C; ++n) {
        hc[n] = (float)row_sum(g.h_w1 + (size_t)n * C, C, bf);
        hc[4 * C + n] = g.h_b1 ? g.h_b1[n] : 0.f;
        hc[8 * C + n] = g.h_p0[n];
        hc[12 * C + n] = g.h_p1[n];
    }
    for (int n = 0; n < C; ++n) { hc[16 * C + n] = (inner && g.h_b_out) ? g.h_b_out[n] : 0.f; hc[17 * C + n] = g.h_b2 ? g.h_b2[n] : 0.f; }
    for (int n = 0; n < n_qkv; ++n) {
        hc[18 * C + n] = (float)row_sum(g.h_w_qkv + (size_t)n * C, C, bf);
        hc[18 * C + n_qkv + n] = g.h_b_qkv ? g.h_b_qkv[n] : 0.f;
    }
    const int ld_att = ew * inner + g.pad_att, ld_x = ew * C + g.pad_x, ld_out = ew * C + g.pad_out, ld_qkv = ew * n_qkv + g.pad_qkv;
    Scratch sc(d_scratch);
    void* d_stream = sc.carve(hs.size() * 2);
    float* d_c = sc.carve<float>(hc.size() * 4);
    _Float16* att16 = sc.carve<_Float16>((size_t)M * ld_att * 2);
    _Float16* x16 = sc.carve<_Float16>((size_t)M * ld_x * 2);
    _Float16* xo16 = sc.carve<_Float16>((size_t)Mg * ld_out * 2);
    _Float16* q16 = sc.carve<_Float16>((size_t)Mg * ld_qkv * 2);
    HIP_OK(hipMemcpyAsync(d_stream, hs.data(), hs.size() * 2, hipMemcpyHostToDevice, s));
    HIP_OK(hipMemcpyAsync(d_c, hc.data(), hc.size() * 4, hipMemcpyHostToDevice, s));
    HIP_OK(hipStreamSynchronize(s));                      // (the host vectors go out of scope)
    const unsigned short fill = (unsigned short)g.sentinel;
    if (inner) {
        if (g.pad_att) HIP_OK(fill16(att16, fill, (size_t)M * ld_att, s));
        HIP_OK(launch_to_p16(g.d_att, inner, nullptr, M, inner, inner, att16, ld_att, lscale, s, nullptr, h16, bf));
    }
    if (g.pad_x) HIP_OK(fill16(x16, fill, (size_t)M * ld_x, s));
    HIP_OK(launch_to_p16(g.d_x, C, nullptr, M, C, C, x16, ld_x, lscale, s, nullptr, h16, bf));
    if (m.block) {
        HIP_OK(fill16(xo16, fill, (size_t)Mg * ld_out, s));
        if (n_qkv) HIP_OK(fill16(q16, fill, (size_t)Mg * ld_qkv, s));
    }
    ChainArgs a;
    ChainH16Args ah;
    if (h16) {
        chain_fill(ah, g, n_qkv, d_stream, frags, d_c, att16, ld_att, x16, ld_x, xo16, ld_out, q16, ld_qkv, m.pf_wgs);
        ah.bf16 = bf;
    } else {
        chain_fill(a, g, n_qkv, d_stream, frags, d_c, att16, ld_att, x16, ld_x, xo16, ld_out, q16, ld_qkv, m.pf_wgs);
        a.store_wt = read_switches().store_wt & (WT_CHAIN_X | WT_CHAIN_QKV);
        if (pair) {                                       // partial sums + flags of the pair form
            float* d_part = sc.carve<float>(2 * ((size_t)M + MTTS_ENTRY_GUARD_ROWS) * C * 4);
            unsigned int* d_flag = sc.carve<unsigned int>(2 * ((size_t)M / 32 + 2) * 4);
            HIP_OK(hipMemsetAsync(d_flag, 0, 2 * ((size_t)M / 32 + 2) * 4, s));
            a.pair = 1; a.pair_part = d_part; a.pair_flag = d_flag; a.pair_epoch = 1; a.pf_wgs = a.pf_wgs ? 16 : 0;
        }
#ifdef MTTS_CHAIN_STAMP
        if (m.stamp) a.kstamp = reinterpret_cast<unsigned long long*>(g.d_qkv_out);      // (diagnostic build: the stamps land in the q|k|v output buffer)
#endif
    }
    auto launch = [&](unsigned int epoch) {
        if (h16) return launch_tblock_chain_h16(ah, s);
        if (pair) a.pair_epoch = epoch;
        return launch_tblock_chain(a, s);
    };
    g_kernel_tag = nullptr;
    HIP_OK(launch(1));
    if (m.block) copy_tag(g.tag);
#ifdef MTTS_CHAIN_STAMP
    if (m.stamp) {
        HIP_OK(hipStreamSynchronize(s));
        return 0;
    }
#endif
    if (m.repeat > 0 && m.h_ms) {                         // the measurement: events around re-launches of the kernel only
        hipEvent_t e0, e1;
        HIP_OK(hipEventCreate(&e0));
        HIP_OK(hipEventCreate(&e1));
        HIP_OK(hipEventRecord(e0, s));
        for (int i = 0; i < m.repeat; ++i) HIP_OK(launch(2 + i));
        HIP_OK(hipEventRecord(e1, s));
        HIP_OK(hipEventSynchronize(e1));
        HIP_OK(hipEventElapsedTime(m.h_ms, e0, e1));
        *m.h_ms /= (float)m.repeat;
        (void)hipEventDestroy(e0);
        (void)hipEventDestroy(e1);
    }
    if (g.d_x_out_image) HIP_OK(hipMemcpyAsync(g.d_x_out_image, xo16, (size_t)Mg * ld_out * 2, hipMemcpyDeviceToDevice, s));
    if (n_qkv && g.d_qkv_image) HIP_OK(hipMemcpyAsync(g.d_qkv_image, q16, (size_t)Mg * ld_qkv * 2, hipMemcpyDeviceToDevice, s));
    HIP_OK(image_to_f32(xo16, ld_out, M, C, ew, bf, 2048.0f, g.d_x_out, s));
    if (n_qkv && g.d_qkv_out) HIP_OK(image_to_f32(q16, ld_qkv, M, n_qkv, ew, bf, 1.0f, g.d_qkv_out, s));
    return 0;
}

// ---- the one-launch Block1D (resnet_conv.hip): x [B*T, C] fp32 (already masked by the caller where the model would) becomes its
// P16 image in d_scratch, the Conv1d(k3) weight is packed and split on the device as for mtts_gemm_p16, the P16 output is decoded
// back to fp32 [B*T, N].  c1 > 0: the last c1 channels of x form a second input segment (the up path's skip concat).  `block`:
// the argument-block entry (sentinel fill, guard rows behind the output image, tag and raw image out).
static int conv_gn_run(mtts_conv_gn_args& g, float eps, bool block, void* d_scratch, hipStream_t s) {
    const int B = g.B, T = g.T, C = g.C, c1 = g.c1, N = g.N, rows = B * T, rows_g = rows + (block ? MTTS_ENTRY_GUARD_ROWS : 0);
    const size_t npanel = (size_t)round_up(N, GEMM_BN) * 3 * C;
    float* planes = static_cast<float*>(g.d_wpacked) + ((npanel + 63) & ~size_t(63));
    HIP_OK(launch_pack_weight(g.d_w, N, C, 3, static_cast<float*>(g.d_wpacked), s));
    HIP_OK(launch_split_panel_f16(static_cast<const float*>(g.d_wpacked), npanel, planes, s));
    const int ld_x = 2 * C + g.pad_x, ld_out = 2 * N + g.pad_out;
    Scratch sc(d_scratch);
    _Float16* a16 = sc.carve<_Float16>((size_t)rows * ld_x * 2);
    _Float16* o16 = sc.carve<_Float16>((size_t)rows_g * ld_out * 2);
    const unsigned short fill = (unsigned short)g.sentinel;
    if (g.pad_x) HIP_OK(fill16(a16, fill, (size_t)rows * ld_x, s));
    HIP_OK(launch_to_p16(g.d_x, C, nullptr, rows, C, C, a16, ld_x, 2048.0f, s));
    if (block) HIP_OK(fill16(o16, fill, (size_t)rows_g * ld_out, s));
    ConvGnArgs a;
    a.a16_0 = a16; a.lda16_0 = ld_x; a.c0 = C - c1;
    if (c1) { a.a16_1 = a16 + 2 * (C - c1); a.lda16_1 = ld_x; a.c1 = c1; }
    a.w16 = planes; a.bias = g.d_bias; a.B = B; a.T = T; a.N = N;
    a.gamma = g.d_gamma; a.beta = g.d_beta; a.mask = g.d_mask; a.chbias = g.d_chbias; a.chbias_stride = g.d_chbias ? g.chbias_stride : 0;
    a.nrows = g.d_nrows; a.nextra = g.d_nextra; a.bias_stats = g.d_bias_stats;
    a.eps = eps; a.out16 = o16; a.ld16 = ld_out; a.range_flag = g.d_range_flag;
    a.store_wt = (read_switches().store_wt & WT_CONV_GN) != 0;
    g_kernel_tag = nullptr;
    HIP_OK(launch_conv_gn(a, s));
    if (block) copy_tag(g.tag);
    if (g.d_out_image) HIP_OK(hipMemcpyAsync(g.d_out_image, o16, (size_t)rows_g * ld_out * 2, hipMemcpyDeviceToDevice, s));
    HIP_OK(launch_from_p16(o16, ld_out, rows, N, 2048.0f, g.d_out, N, s));
    return 0;
}
static int conv_gn_positional(const float* d_x, int B, int T, int C, int c1, const float* d_w, void* d_wpacked, const float* d_bias, int N,
                              const float* d_gamma, const float* d_beta, const float* d_mask, const float* d_chbias, int chbias_stride,
                              const int* d_nrows, const int* d_nextra, const float* d_bias_stats, float eps, float* d_out, void* d_scratch,
                              void* stream) {
    REFUSE_IF(!d_x || !d_w || !d_wpacked || !d_scratch || !d_out, "null buffer");
    REFUSE_IF(C <= 0 || (C % 32) || c1 < 0 || (c1 % 32) || c1 >= C, "mtts_conv_gn: C and c1 must be multiples of 32, c1 < C");
    REFUSE_IF(!conv_gn_supported(T, N), "mtts_conv_gn: unsupported shape (N = 384, 65 <= T <= 384)");
    mtts_conv_gn_args g = {};
    g.d_x = d_x; g.B = B; g.T = T; g.C = C; g.c1 = c1; g.d_w = d_w; g.d_wpacked = d_wpacked; g.d_bias = d_bias; g.N = N;
    g.d_gamma = d_gamma; g.d_beta = d_beta; g.d_mask = d_mask; g.d_chbias = d_chbias; g.chbias_stride = chbias_stride;
    g.d_nrows = d_nrows; g.d_nextra = d_nextra; g.d_bias_stats = d_bias_stats; g.d_out = d_out;
    return conv_gn_run(g, eps, false, d_scratch, static_cast<hipStream_t>(stream));
}

// ---- the image GEMMs on the argument block (gemm_p16.hip): mtts_gemm_h16 (ew = 1: H16 images, host 16-bit plane) and
// mtts_gemm_p16_args_run (ew = 2: P16 images, planes split on the device).  mtts_gemm_f32_args_run, whose A stays fp32 rows, shares
// the output-row defaults, the prologue, the epilogue and the tag copy.
struct OutRows { int out_T, out_stride, out_off; };
static int block_out_rows(const mtts_gemm_h16_args* g, const std::string& who, OutRows* r) {
    *r = {g->out_T > 0 ? g->out_T : g->T_out, g->out_T > 0 ? g->out_stride : 1, g->out_T > 0 ? g->out_off : 0};
    REFUSE_IF(r->out_stride < 1 || r->out_off < 0 || (g->T_out - 1) * r->out_stride + r->out_off >= r->out_T, who + "output rows leave [0, out_T)");
    REFUSE_IF(g->ntaps > 1 && !g->h_tap_off, who + "a convolution needs its tap offsets");
    return 0;
}
static bool block_sizes_bad(const mtts_gemm_h16_args* g) {
    return !g || g->B <= 0 || g->T_in <= 0 || g->T_out <= 0 || g->N <= 0 || g->C <= 0 || g->ntaps < 1 || g->ntaps > MAX_TAPS;
}
static void block_prologue(GemmArgs& a, const mtts_gemm_h16_args* g) {
    a.ntaps = g->ntaps;
    for (int j = 0; j < g->ntaps; ++j) a.tap_off[j] = g->h_tap_off ? g->h_tap_off[j] : 0;
    a.in_stride = g->in_stride > 0 ? g->in_stride : 1; a.B = g->B; a.T_in = g->T_in; a.T_out = g->T_out;
    a.a_mean = g->d_a_mean; a.a_rstd = g->d_a_rstd; a.a_part = g->d_a_part; a.a_nparts = g->a_nparts;
}
// o16 / r16 are the output and residual images, ew halves per image element
static void block_epilogue(GemmArgs& a, const mtts_gemm_h16_args* g, _Float16* o16, _Float16* r16, int ew, const OutRows& r) {
    const int N = g->N;
    a.bias = g->d_bias; a.N = N; a.act = g->act; a.p0 = g->d_p0; a.p1 = g->d_p1;
    a.res = g->d_res; a.ldr = g->ldr; a.out_mask = g->d_out_mask; a.out_scale = g->out_scale; a.out = g->d_out; a.ldc = N;
    if (g->d_out16_f32) { a.out16 = o16; a.ld16 = ew * N; a.out16_mask = g->d_out16_mask; }
    if (g->res16_mode == 1) { a.res16 = r16; a.ldr16 = ew * N; }
    if (g->res16_mode == 2) { a.res16 = o16; a.ldr16 = ew * N; }
    a.out_T = r.out_T; a.out_stride = r.out_stride; a.out_off = r.out_off;
    a.stats_out = g->d_stats_out; a.force_bm = g->force_bm; a.range_flag = g->d_range_flag;
    a.gn_stats = g->d_gn_stats; a.gn_groups = g->gn_groups; a.gn_nrows = g->d_gn_nrows;
    a.gnr_y = g->d_gnr_y; a.gnr_stats = g->d_gnr_stats; a.gnr_tile_rows = g->gnr_tile_rows; a.gnr_groups = g->gnr_groups;
    a.gnr_gamma = g->d_gnr_gamma; a.gnr_beta = g->d_gnr_beta; a.gnr_mask = g->d_gnr_mask; a.gnr_eps = g->gnr_eps > 0.f ? g->gnr_eps : 1e-5f;
    a.gnr_nextra = g->d_gnr_nextra; a.gnr_bias_stats = g->d_gnr_bias_stats;
}
// The two weight recipes, from the host panel [Np][Kp]; each uploads, waits (its host vectors go out of scope) and sets the
// weight fields of `a`.  H16: the 16-bit plane and the row sums of the ROUNDED plane (what the model packs, pack.hip add_planes).
static int image_weights_h16(GemmArgs& a, const std::vector<float>& panel, int Np, int Kp, bool bf, Scratch& sc, hipStream_t s) {
    const size_t npanel = panel.size();
    std::vector<uint16_t> plane(npanel);
    if (bf) panel_bf16_host(panel.data(), npanel, plane.data());
    else panel_h16_host(panel.data(), npanel, plane.data());
    std::vector<float> wsum(Np);
    for (int n = 0; n < Np; ++n) wsum[n] = (float)rounded_row_sum(panel.data() + (size_t)n * Kp, Kp, bf);
    void* d_plane = sc.carve(npanel * 2);
    float* d_wsum = sc.carve<float>((size_t)Np * 4);
    HIP_OK(hipMemcpyAsync(d_plane, plane.data(), npanel * 2, hipMemcpyHostToDevice, s));
    HIP_OK(hipMemcpyAsync(d_wsum, wsum.data(), (size_t)Np * 4, hipMemcpyHostToDevice, s));
    HIP_OK(hipStreamSynchronize(s));
    a.half16 = true; a.bf16 = bf; a.w16h = d_plane; a.wsum = d_wsum;
    return 0;
}
// P16: the fp32 panel split on the device, the row sums of the fp32 panel (pack.hip add_planes in this arithmetic)
static int image_weights_p16(GemmArgs& a, const std::vector<float>& panel, int Np, int Kp, Scratch& sc, hipStream_t s) {
    const size_t npanel = panel.size();
    std::vector<float> wsum(Np);
    for (int n = 0; n < Np; ++n) wsum[n] = (float)plain_row_sum(panel.data() + (size_t)n * Kp, Kp, false);
    float* d_panel = sc.carve<float>(npanel * 4);
    void* d_planes = sc.carve(npanel * 4);
    float* d_wsum = sc.carve<float>((size_t)Np * 4);
    HIP_OK(hipMemcpyAsync(d_panel, panel.data(), npanel * 4, hipMemcpyHostToDevice, s));
    HIP_OK(hipMemcpyAsync(d_wsum, wsum.data(), (size_t)Np * 4, hipMemcpyHostToDevice, s));
    HIP_OK(hipStreamSynchronize(s));
    HIP_OK(launch_split_panel_f16(d_panel, npanel, d_planes, s));
    a.w16 = d_planes; a.wsum = d_wsum;
    return 0;
}
static int gemm_image_run(mtts_gemm_h16_args* g, int ew, int fast16, float out_lscale, const char* name, void* d_scratch, void* stream) {
    hipStream_t s = static_cast<hipStream_t>(stream);
    const std::string who = std::string(name) + ": ", kind = ew == 1 ? "H16" : "P16", q = std::to_string(32 * (3 - ew));
    REFUSE_IF(!g, who + "null argument block");
    g->tag[0] = 0; g->wave_rows = 0;
    REFUSE_IF(!g->d_a || !g->h_w || !d_scratch || (!g->d_out && !g->d_out16_f32), who + "null buffer");
    REFUSE_IF(ew == 1 && !g->half16, who + "launches the one-plane instantiations only (half16 must be set)");
    REFUSE_IF(ew == 2 && (g->half16 || g->bf16), who + "launches the two-plane instantiations only (half16 and bf16 must be 0)");
    REFUSE_IF(fast16 != 0 && fast16 != 1, who + "fast16 is 0 or 1");
    REFUSE_IF(out_lscale != 2048.0f && out_lscale != 1.0f, who + "out_lscale is 2048 or 1");
    REFUSE_IF(g->ntaps < 1 || g->ntaps > MAX_TAPS, who + "ntaps out of range");
    REFUSE_IF(g->B <= 0 || g->T_in <= 0 || g->T_out <= 0 || g->N <= 0 || (g->N & 3), who + "bad shape");
    const int quantum = 32 * (3 - ew);
    REFUSE_IF(g->C <= 0 || (g->C % quantum) || g->c1 < 0 || (g->c1 % quantum) || g->c1 >= g->C,
              who + kind + " operands need C % " + q + " == 0 (and c1 % " + q + " == 0, c1 < C)");
    REFUSE_IF(g->lda < g->C || (g->lda & 3), who + "lda");
    const bool want16 = g->d_out16_f32 != nullptr;
    REFUSE_IF((want16 || g->res16_mode) && (g->N % quantum), who + "a" + (ew == 1 ? "n " : " ") + kind + " output or residual image needs N % " + q + " == 0");
    REFUSE_IF(g->res16_mode < 0 || g->res16_mode > 2 || (g->res16_mode == 1 && !g->d_res16_f32) ||
                  (g->res16_mode == 2 && (!want16 || !g->out16_preload || out_lscale != 2048.0f)),
              who + "res16_mode 1 needs d_res16_f32, 2 (in place) needs d_out16_f32 with out16_preload" + (ew == 2 ? " and out_lscale 2048" : ""));
    REFUSE_IF(g->res16_mode && g->d_res, who + "res16 together with res");
    const bool ln = g->d_a_mean || g->d_a_part;
    REFUSE_IF(g->d_gn_stats && fast16, who + "gn_stats with fast16 (that mode keeps the separate statistics pass)");
    REFUSE_IF(g->d_gn_stats && (g->act != ACT_NONE || g->d_res || g->res16_mode || g->d_out_mask || g->out_scale != 1.0f || ln || g->gn_groups <= 0),
              who + "gn_stats with an activation, residual, mask, scale or LayerNorm (bias-only epilogue; gn_groups > 0)");
    OutRows r;
    RET_IF(block_out_rows(g, who, &r));
    const bool h16 = ew == 1, bf = h16 && g->bf16 != 0;
    const int C = g->C, c0 = C - g->c1, N = g->N, Np = round_up(N, GEMM_BN), Kp = g->ntaps * C;
    const size_t out_rows = (size_t)g->B * r.out_T;
    std::vector<float> panel((size_t)Np * Kp);
    pack_weight_host(g->h_w, g->ntaps > 1 ? 1 : 0, N, C, g->ntaps, 0, nullptr, nullptr, panel.data(), C);
    Scratch sc(d_scratch);
    _Float16* a16 = sc.carve<_Float16>((size_t)g->B * g->T_in * C * 2 * ew);
    _Float16* o16 = sc.carve<_Float16>(out_rows * N * 2 * ew);
    _Float16* r16 = sc.carve<_Float16>(out_rows * N * 2 * ew);
    GemmArgs a;
    if (h16) RET_IF(image_weights_h16(a, panel, Np, Kp, bf, sc, s));
    else RET_IF(image_weights_p16(a, panel, Np, Kp, sc, s));
    const float in_lscale = h16 ? 1.0f : 2048.0f;         // (H16: unused)
    HIP_OK(launch_to_p16(g->d_a, g->lda, g->d_a_mask, g->B * g->T_in, C, C, a16, ew * C, in_lscale, s, nullptr, h16, bf));
    if (want16 && g->out16_preload) HIP_OK(launch_to_p16(g->d_out16_f32, N, nullptr, (int)out_rows, N, N, o16, ew * N, h16 ? 1.0f : out_lscale, s, nullptr, h16, bf));
    if (g->res16_mode == 1) HIP_OK(launch_to_p16(g->d_res16_f32, N, nullptr, (int)out_rows, N, N, r16, ew * N, in_lscale, s, nullptr, h16, bf));
    a.a16_0 = a16; a.lda16_0 = ew * C; a.c0 = c0; a.ktap = C;
    if (g->c1) { a.a16_1 = a16 + ew * c0; a.lda16_1 = ew * C; a.c1 = g->c1; }
    block_prologue(a, g);
    a.terms = 2;
    if (!h16) { a.fast16 = fast16 != 0; a.out_lscale = out_lscale; }
    block_epilogue(a, g, o16, r16, ew, r);
    a.store_wt = (read_switches().store_wt & WT_GEMM) != 0;
    g->wave_rows = gemm_p16_wave_rows(a);
    g_kernel_tag = nullptr;
    HIP_OK(launch_gemm(a, s));
    copy_tag(g->tag);
    if (want16) HIP_OK(image_to_f32(o16, ew * N, (int)out_rows, N, ew, bf, out_lscale, g->d_out16_f32, s));
    return 0;
}

// ---- attention (attention_f32.hip): fp32 I/O (ew = 0), or q|k|v converted to an image with unscaled residuals in d_scratch
// (>= 8 ew B T H 64 bytes) and the output image decoded back to fp32 (ew = 2: P16, 1: H16).
struct AttnMode {
    int ew = 0;
    bool bf16 = false, fast16 = false;
    float out_lscale = 2048.0f;
    const int* klen = nullptr;
    unsigned int* range_flag = nullptr;
};
static int attention_run(const float* d_qkv, const float* d_mask, int B, int T, int H, int D, float scale, int mask_mode, float* d_out,
                         const AttnMode& m, void* d_scratch, void* stream) {
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int M = B * T, C3 = 3 * H * D, ew = m.ew;
    const bool h16 = ew == 1;
    AttnArgs a;
    a.mask = d_mask; a.klen = m.klen; a.B = B; a.T = T; a.H = H; a.D = D; a.scale = scale; a.mask_mode = mask_mode;
    a.range_flag = m.range_flag;
    a.store_wt = (read_switches().store_wt & WT_ATTN) != 0;
    _Float16* q16 = static_cast<_Float16*>(d_scratch);
    _Float16* o16 = q16 + (size_t)M * ew * C3;
    if (ew) {
        HIP_OK(launch_to_p16(d_qkv, C3, nullptr, M, C3, C3, q16, ew * C3, 1.0f, s, nullptr, h16, h16 && m.bf16));
        a.qkv16 = q16; a.ld16 = ew * C3; a.out16 = o16; a.ldo16 = ew * H * D;
        a.half16 = h16; a.bf16 = h16 && m.bf16; a.fast16 = m.fast16; a.out_lscale = m.out_lscale;
    } else {
        a.qkv = d_qkv; a.out = d_out;
    }
    g_kernel_tag = nullptr;
    HIP_OK(launch_attention(a, s));
    if (ew) HIP_OK(image_to_f32(o16, ew * H * D, M, H * D, ew, m.bf16, m.out_lscale, d_out, s));
    return 0;
}
// what the two image entries with klen refuse (kind: "H16" / "P16")
static int attention_image_check(const std::string& who, const char* kind, const float* d_qkv, const float* d_mask, int B, int T, int H, int D,
                                 int mask_mode, const float* d_out, const void* d_scratch) {
    REFUSE_IF(!d_qkv || !d_out || !d_scratch, who + "null buffer");
    REFUSE_IF(D != 64 || B <= 0 || T <= 0 || H <= 0, who + kind + " attention needs D == 64 and a non-empty batch");
    REFUSE_IF(mask_mode == 1 && !d_mask, who + "the boolean mask mode needs a mask");
    return 0;
}

// ---- GroupNorm + Mish (norm_glue.hip gn_partial + gn_apply): statistics from gn_partial into d_scratch, or the GEMM's tile_stats;
// the fp32 store, and with ew = 2 / 1 a P16 / H16 image behind the partial sums, decoded into out16_f32.
struct GnEntry {
    const float *y = nullptr, *gamma = nullptr, *beta = nullptr, *mask = nullptr, *chbias = nullptr;
    int chbias_stride = 0;
    const float* res = nullptr;
    int ldr = 0, B = 0, T = 0, C = 0, G = 0;
    float eps = 1e-5f;
    const float* tile_stats = nullptr;
    int tile_rows = 0;
    const int *nrows = nullptr, *nextra = nullptr;
    const float *bias_stats = nullptr, *out16_mask = nullptr;
    float *out = nullptr, *stats_out = nullptr, *out16_f32 = nullptr;
    unsigned int* range_flag = nullptr;
    int ew = 0;
    bool bf16 = false;
};
static int64_t gn_partial_bytes(int B, int T, int G) { return (int64_t)B * gn_chunks_max(T) * G * 2 * (int64_t)sizeof(float); }
static int groupnorm_run(const GnEntry& e, void* d_scratch, void* stream) {
    hipStream_t s = static_cast<hipStream_t>(stream);
    float* partial = static_cast<float*>(d_scratch);
    _Float16* o16 = reinterpret_cast<_Float16*>(static_cast<char*>(d_scratch) + up256((size_t)gn_partial_bytes(e.B, e.T, e.G)));
    GnApplyArgs a;
    a.y = e.y; a.gamma = e.gamma; a.beta = e.beta; a.mask = e.mask; a.chbias = e.chbias; a.chbias_stride = e.chbias_stride;
    a.res = e.res; a.ldr = e.ldr;
    if (e.tile_stats) { a.tile_stats = e.tile_stats; a.tile_rows = e.tile_rows; }
    else { HIP_OK(launch_gn_partial(e.y, e.B, e.T, e.C, e.G, partial, s, e.nrows)); a.partial = partial; a.nrows = e.nrows; }
    a.nextra = e.nextra; a.bias_stats = e.bias_stats; a.stats_out = e.stats_out;
    a.out = e.out; a.range_flag = e.range_flag;
    if (e.ew) { a.out16 = o16; a.ld16 = e.ew * e.C; a.out16_mask = e.out16_mask; a.half16 = e.ew == 1; a.bf16 = e.ew == 1 && e.bf16; }
    a.B = e.B; a.T = e.T; a.C = e.C; a.G = e.G; a.eps = e.eps;
    HIP_OK(launch_gn_apply(a, s));
    if (e.ew) HIP_OK(image_to_f32(o16, e.ew * e.C, e.B * e.T, e.C, e.ew, e.bf16, 2048.0f, e.out16_f32, s));
    return 0;
}
// the two image entries: every argument the decoder passes, and what they refuse (kind "H16" / "P16", C % quantum)
static int groupnorm_image(const char* name, const char* kind, int ew, bool bf16, const float* d_y, const float* d_gamma, const float* d_beta,
                           const float* d_mask, const float* d_chbias, int chbias_stride, int B, int T, int C, int G, float eps,
                           const float* d_tile_stats, int tile_rows, const int* d_nrows, const int* d_nextra, const float* d_bias_stats,
                           const float* d_out16_mask, float* d_out, float* d_out16_f32, unsigned int* d_range_flag, void* d_scratch, void* stream) {
    const std::string who = std::string(name) + ": ", q = std::to_string(32 * (3 - ew));
    REFUSE_IF(!d_y || !d_gamma || !d_beta || !d_mask || !d_out16_f32 || !d_scratch, who + "null buffer");
    REFUSE_IF(B <= 0 || T <= 0 || C <= 0 || (C % (32 * (3 - ew))) || G <= 0 || (C % G), who + kind + " images need C % " + q + " == 0 (and C % G == 0)");
    REFUSE_IF(d_chbias && chbias_stride && chbias_stride < C, who + "a bias row per utterance has at least C values");
    REFUSE_IF((d_nextra != nullptr) != (d_bias_stats != nullptr), who + "nextra and bias_stats come together");
    REFUSE_IF(d_tile_stats && tile_rows <= 0, who + "tile_stats need tile_rows");
    GnEntry e;
    e.y = d_y; e.gamma = d_gamma; e.beta = d_beta; e.mask = d_mask; e.chbias = d_chbias; e.chbias_stride = chbias_stride;
    e.B = B; e.T = T; e.C = C; e.G = G; e.eps = eps; e.tile_stats = d_tile_stats; e.tile_rows = tile_rows;
    e.nrows = d_nrows; e.nextra = d_nextra; e.bias_stats = d_bias_stats; e.out16_mask = d_out16_mask;
    e.out = d_out; e.out16_f32 = d_out16_f32; e.range_flag = d_range_flag; e.ew = ew; e.bf16 = bf16;
    return groupnorm_run(e, d_scratch, stream);
}

// ---- channel LayerNorm (norm_glue.hip)
static int layernorm_run(const float* d_x, int ldx, int B, int T, int C, const float* d_gamma, const float* d_beta, float eps, int act,
                         const float* d_film, const float* d_mask, float* d_y, int ldy, void* stream) {
    LayerNormArgs a;
    a.x = d_x; a.ldx = ldx; a.y = d_y; a.ldy = ldy; a.M = B * T; a.C = C; a.T = T; a.gamma = d_gamma; a.beta = d_beta; a.eps = eps;
    a.act = act; a.film = d_film; a.mask = d_mask;
    HIP_OK(launch_layernorm(a, static_cast<hipStream_t>(stream)));
    return 0;
}

extern "C" {

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
    a.store_wt = (read_switches().store_wt & WT_GEMM) != 0;
    HIP_OK(launch_gemm(a, s));
    if (d_out16_f32) HIP_OK(launch_from_p16(o16, 2 * N, B * T_out, N, out_lscale, d_out16_f32, N, s));
    return 0;
}

int64_t mtts_conv_gn_scratch_bytes(int B, int T, int C, int N) { return (int64_t)B * T * (C + N) * 4 + 1024; }
int mtts_conv_gn(const float* d_x, int B, int T, int C, int c1, const float* d_w, void* d_wpacked, const float* d_bias, int N,
                 const float* d_gamma, const float* d_beta, const float* d_mask, const float* d_chbias, const int* d_nrows,
                 const int* d_nextra, const float* d_bias_stats, float eps, float* d_out, void* d_scratch, void* stream) {
    return conv_gn_positional(d_x, B, T, C, c1, d_w, d_wpacked, d_bias, N, d_gamma, d_beta, d_mask, d_chbias, 0, d_nrows, d_nextra, d_bias_stats,
                              eps, d_out, d_scratch, stream);
}
// ... with one time-embedding bias row per utterance: d_chbias [B][chbias_stride], the first N values of a row are read
int mtts_conv_gn_rows(const float* d_x, int B, int T, int C, int c1, const float* d_w, void* d_wpacked, const float* d_bias, int N,
                      const float* d_gamma, const float* d_beta, const float* d_mask, const float* d_chbias, int chbias_stride,
                      const int* d_nrows, const int* d_nextra, const float* d_bias_stats, float eps, float* d_out, void* d_scratch,
                      void* stream) {
    REFUSE_IF(!d_chbias || chbias_stride < N, "mtts_conv_gn_rows: needs a bias row of at least N values per utterance");
    return conv_gn_positional(d_x, B, T, C, c1, d_w, d_wpacked, d_bias, N, d_gamma, d_beta, d_mask, d_chbias, chbias_stride, d_nrows, d_nextra,
                              d_bias_stats, eps, d_out, d_scratch, stream);
}

int mtts_attention_f32(const float* d_qkv, const float* d_mask, int B, int T, int H, int D, float scale, int mask_mode, float* d_out,
                       void* stream) {
    return attention_run(d_qkv, d_mask, B, T, H, D, scale, mask_mode, d_out, AttnMode(), nullptr, stream);
}

// P16 I/O, d_scratch >= 16*B*T*H*64 bytes.  D must be 64.
int mtts_attention_p16(const float* d_qkv, const float* d_mask, int B, int T, int H, int D, float scale, int mask_mode, float* d_out,
                       void* d_scratch, void* stream) {
    REFUSE_IF(D != 64 || !d_scratch, "P16 attention needs D == 64 and a scratch buffer");
    AttnMode m;
    m.ew = 2;
    return attention_run(d_qkv, d_mask, B, T, H, D, scale, mask_mode, d_out, m, d_scratch, stream);
}

int mtts_row_stats(const float* d_x, int M, int C, int ld, float eps, float* d_mean, float* d_rstd, void* stream) {
    HIP_OK(launch_row_stats(d_x, M, C, ld, eps, d_mean, d_rstd, static_cast<hipStream_t>(stream)));
    return 0;
}

int mtts_channel_layernorm(const float* d_x, int B, int T, int C, const float* d_gamma, const float* d_beta, float eps, int act,
                           const float* d_film, const float* d_mask, float* d_y, void* stream) {
    REFUSE_IF(B <= 0 || T <= 0, "mtts_channel_layernorm: empty batch");
    REFUSE_IF(act != ACT_NONE && act != ACT_SILU, "mtts_channel_layernorm: act must be 0 (none) or 2 (SiLU)");
    return layernorm_run(d_x, C, B, T, C, d_gamma, d_beta, eps, act, d_film, d_mask, d_y, C, stream);
}

int64_t mtts_groupnorm_scratch_bytes(int B, int T, int G) { return gn_partial_bytes(B, T, G); }

// ... with the ResNet block's time-embedding bias, (out + chbias[b]) * mask (reference decoder.py:60), one row per utterance:
// d_chbias [B][chbias_stride] (chbias_stride = 0: one row [C] for the batch); null: none
static int groupnorm_plain(const float* d_y, const float* d_gamma, const float* d_beta, const float* d_mask, const float* d_chbias,
                           int chbias_stride, int B, int T, int C, int G, float eps, float* d_out, void* d_scratch, void* stream) {
    GnEntry e;
    e.y = d_y; e.gamma = d_gamma; e.beta = d_beta; e.mask = d_mask; e.chbias = d_chbias; e.chbias_stride = chbias_stride;
    e.B = B; e.T = T; e.C = C; e.G = G; e.eps = eps; e.out = d_out;
    return groupnorm_run(e, d_scratch, stream);
}
int mtts_groupnorm_mish(const float* d_y, const float* d_gamma, const float* d_beta, const float* d_mask, int B, int T, int C, int G,
                        float eps, float* d_out, void* d_scratch, void* stream) {
    return groupnorm_plain(d_y, d_gamma, d_beta, d_mask, nullptr, 0, B, T, C, G, eps, d_out, d_scratch, stream);
}
int mtts_groupnorm_mish_rows(const float* d_y, const float* d_gamma, const float* d_beta, const float* d_mask, const float* d_chbias,
                             int chbias_stride, int B, int T, int C, int G, float eps, float* d_out, void* d_scratch, void* stream) {
    REFUSE_IF(!d_chbias || (chbias_stride && chbias_stride < C), "mtts_groupnorm_mish_rows: needs a bias row of at least C values per utterance");
    return groupnorm_plain(d_y, d_gamma, d_beta, d_mask, d_chbias, chbias_stride, B, T, C, G, eps, d_out, d_scratch, stream);
}

// ---- the transformer-block chain (tblock_chain.hip).  w_qkv == NULL: no q|k|v phase; inner == 0: no out-projection (the
// FeedForward alone on d_x).  h_* pointers are HOST memory, d_* device memory.
// the model's launch plan for M rows (test entry; no GPU): rows per workgroup and prefetch workgroups
int mtts_chain_plan(int M, int ch, int* qb, int* prefetch_wgs) {
    if (M <= 0 || (ch != 128 && ch != 256) || !qb || !prefetch_wgs) { set_error("mtts_chain_plan: bad argument"); return -1; }
    chain_plan(M, ch, 0, read_switches().chain_pf, qb, prefetch_wgs);
    return 0;
}
int mtts_chain_shape_exists(int C, int qb, int ch) { return chain_shape_exists(C, qb, ch) ? 1 : 0; }
// the model's launch-form decision (decoder.hip tblock_plan) for `count` consecutive row counts, with the switches as arguments
int mtts_tblock_plan(int C, int inner, int n_qkv, int M, int count, int chain_on, int chain_ch, int chain_qb, int chain_pf, int chain_min_rows,
                     int pair_on, int pair_min_rows, int* ch, int* form, int* qb, int* grid_wgs, int* prefetch_wgs) {
    if (M <= 0 || count <= 0 || count > (1 << 24) - M || inner < 0 || n_qkv < 0 || (chain_ch != 128 && chain_ch != 256) || chain_qb < 0 ||
        chain_pf < 0 || chain_pf > 64 || !ch || !form || !qb || !grid_wgs || !prefetch_wgs) {
        set_error("mtts_tblock_plan: bad argument");
        return -1;
    }
    Switches sw;
    sw.chain_on = chain_on != 0; sw.chain_ch = chain_ch; sw.chain_qb = chain_qb; sw.chain_pf = chain_pf; sw.chain_min_rows = chain_min_rows;
    sw.pair_on = pair_on != 0; sw.pair_min_rows = pair_min_rows;
    *ch = chain_packed_ch(C, chain_ch);
    // what pack_all leaves in the image of a default-arithmetic context for such a block
    const bool has_chain = sw.chain_on && chain_supported(C, inner, n_qkv) && chain_shape_exists(C, 32, *ch);
    const bool has_pair = has_chain && tblock_pair_possible(sw, C, inner, n_qkv, *ch);
    for (int i = 0; i < count; ++i) {
        const TBlockPlan p = tblock_plan(sw, C, inner, n_qkv, *ch, M + i, has_chain, has_pair);
        form[i] = p.form; qb[i] = p.qb; grid_wgs[i] = p.grid; prefetch_wgs[i] = p.pf;
    }
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
static int tblock_chain_entry(mtts_chain_args g, void* d_scratch, void* stream, int repeat, float* h_ms) {
    REFUSE_IF(!chain_supported(g.C, g.inner, g.n_qkv) || !g.d_x || !g.h_w1 || !g.h_w2 || !d_scratch || !g.d_x_out, "mtts_tblock_chain: unsupported shape or null buffer");
    REFUSE_IF(g.pair && !chain_supported_pair(g.C, g.inner, g.ch, g.n_qkv), "mtts_tblock_chain_pair: unsupported shape");
    ChainMode m;
    m.pf_wgs = read_switches().chain_pf; m.stamp = true; m.repeat = repeat; m.h_ms = h_ms;
    return chain_run(g, g.n_qkv, m, d_scratch, static_cast<hipStream_t>(stream));
}
int mtts_tblock_chain(const float* d_att, const float* d_x, int M, int C, int inner, const float* h_w_out, const float* h_b_out,
                      const float* h_w1, const float* h_b1, const float* h_p0, const float* h_p1, const float* h_w2, const float* h_b2,
                      const float* h_w_qkv, const float* h_b_qkv, int n_qkv, const float* d_out_mask, int qb, int ch, float* d_x_out,
                      float* d_qkv_out, void* d_scratch, void* stream) {
    return mtts_tblock_chain_timed(d_att, d_x, M, C, inner, h_w_out, h_b_out, h_w1, h_b1, h_p0, h_p1, h_w2, h_b2, h_w_qkv, h_b_qkv, n_qkv, d_out_mask,
                                   qb, ch, d_x_out, d_qkv_out, d_scratch, stream, 0, nullptr);
}
int mtts_tblock_chain_timed(const float* d_att, const float* d_x, int M, int C, int inner, const float* h_w_out, const float* h_b_out,
                            const float* h_w1, const float* h_b1, const float* h_p0, const float* h_p1, const float* h_w2, const float* h_b2,
                            const float* h_w_qkv, const float* h_b_qkv, int n_qkv, const float* d_out_mask, int qb, int ch, float* d_x_out,
                            float* d_qkv_out, void* d_scratch, void* stream, int repeat, float* h_ms) {
    return tblock_chain_entry(chain_positional(d_att, d_x, M, C, inner, h_w_out, h_b_out, h_w1, h_b1, h_p0, h_p1, h_w2, h_b2, h_w_qkv, h_b_qkv, n_qkv, d_out_mask,
                                               qb, ch, d_x_out, d_qkv_out), d_scratch, stream, repeat, h_ms);
}
// the pair form of the same launch (two workgroups per row tile; ChainArgs::pair): qb = 48 or 32, at most 120 row tiles
int mtts_tblock_chain_pair_timed(const float* d_att, const float* d_x, int M, int C, int inner, const float* h_w_out, const float* h_b_out,
                                 const float* h_w1, const float* h_b1, const float* h_p0, const float* h_p1, const float* h_w2, const float* h_b2,
                                 const float* h_w_qkv, const float* h_b_qkv, int n_qkv, const float* d_out_mask, int qb, int ch, float* d_x_out,
                                 float* d_qkv_out, void* d_scratch, void* stream, int repeat, float* h_ms) {
    mtts_chain_args g = chain_positional(d_att, d_x, M, C, inner, h_w_out, h_b_out, h_w1, h_b1, h_p0, h_p1, h_w2, h_b2, h_w_qkv, h_b_qkv, n_qkv, d_out_mask, qb, ch,
                                         d_x_out, d_qkv_out);
    g.pair = 1;
    return tblock_chain_entry(g, d_scratch, stream, repeat, h_ms);
}

// ---- the two fused kernels on argument blocks (include/mtts.h mtts_chain_args, mtts_conv_gn_args): range flag, padded image rows,
// guard rows and the raw output images; every image is filled with the sentinel first.
static int chain_args_check(const mtts_chain_args* g, int* n_qkv) {
    if (!g) { set_error("mtts_tblock_chain_args: null argument block"); return -1; }
    *n_qkv = g->h_w_qkv ? g->n_qkv : 0;
    if (g->M <= 0 || g->M > (1 << 20) || !chain_supported(g->C, g->inner, *n_qkv) || (g->ch != 128 && g->ch != 256)) { set_error("mtts_tblock_chain_args: unsupported shape"); return -1; }
    if (g->pair && !chain_supported_pair(g->C, g->inner, g->ch, *n_qkv)) { set_error("mtts_tblock_chain_args: unsupported shape for the pair form"); return -1; }
    if (bad_pad(g->pad_att) || bad_pad(g->pad_x) || bad_pad(g->pad_out) || bad_pad(g->pad_qkv)) { set_error("mtts_tblock_chain_args: a row pad is a multiple of 8 halves in [0, 4096]"); return -1; }
    if (g->sentinel > 0xffffu) { set_error("mtts_tblock_chain_args: the sentinel is a 16-bit pattern"); return -1; }
    return 0;
}
int64_t mtts_tblock_chain_args_scratch_bytes(const mtts_chain_args* g) {
    int n_qkv = 0;
    RET_IF(chain_args_check(g, &n_qkv));
    const int64_t M = g->M, Mg = M + MTTS_ENTRY_GUARD_ROWS, C = g->C;
    const int64_t frags = g->pair ? 2 * chain_stream_frags_pair(g->C, g->inner, g->ch, n_qkv) : chain_stream_frags(g->C, g->inner, g->ch, n_qkv);
    int64_t n = up256(frags * CHAIN_WAVES * 1024) + up256(4 * (18 * C + 2 * n_qkv));
    n += up256(M * (2 * g->inner + g->pad_att) * 2) + up256(M * (2 * C + g->pad_x) * 2);
    n += up256(Mg * (2 * C + g->pad_out) * 2) + up256(Mg * (2 * n_qkv + g->pad_qkv) * 2);
    n += up256(2 * Mg * C * 4) + up256(2 * (M / 32 + 2) * 4);            // partial sums + flags of the pair form
    return n + 256;
}
int mtts_tblock_chain_args_run(mtts_chain_args* g, void* d_scratch, void* stream) {
    int n_qkv = 0;
    RET_IF(chain_args_check(g, &n_qkv));
    g->tag[0] = 0;
    REFUSE_IF(!g->d_x || !g->h_w1 || !g->h_w2 || !g->h_p0 || !g->h_p1 || !d_scratch || !g->d_x_out || (g->inner && (!g->d_att || !g->h_w_out)) || (n_qkv && !g->d_qkv_out),
              "mtts_tblock_chain_args: null buffer");
    ChainMode m;
    m.pf_wgs = read_switches().chain_pf; m.block = true;
    return chain_run(*g, n_qkv, m, d_scratch, static_cast<hipStream_t>(stream));
}

static int conv_gn_args_check(const mtts_conv_gn_args* g) {
    if (!g) { set_error("mtts_conv_gn_args: null argument block"); return -1; }
    if (g->B <= 0 || g->B > 4096 || g->C <= 0 || (g->C % 32) || g->c1 < 0 || (g->c1 % 32) || g->c1 >= g->C) { set_error("mtts_conv_gn_args: C and c1 must be multiples of 32, c1 < C"); return -1; }
    if (!conv_gn_supported(g->T, g->N)) { set_error("mtts_conv_gn_args: unsupported shape (N = 384, 65 <= T <= 384)"); return -1; }
    if (bad_pad(g->pad_x) || bad_pad(g->pad_out)) { set_error("mtts_conv_gn_args: a row pad is a multiple of 8 halves in [0, 4096]"); return -1; }
    if (g->sentinel > 0xffffu) { set_error("mtts_conv_gn_args: the sentinel is a 16-bit pattern"); return -1; }
    if (g->d_chbias && g->chbias_stride && (g->chbias_stride < g->N || (g->chbias_stride & 3))) { set_error("mtts_conv_gn_args: a bias row per utterance has at least N values (stride % 4 == 0)"); return -1; }
    if ((g->d_nextra != nullptr) != (g->d_bias_stats != nullptr)) { set_error("mtts_conv_gn_args: nextra and bias_stats come together"); return -1; }
    return 0;
}
int64_t mtts_conv_gn_args_scratch_bytes(const mtts_conv_gn_args* g) {
    RET_IF(conv_gn_args_check(g));
    const int64_t rows = (int64_t)g->B * g->T;
    return up256(rows * (2 * g->C + g->pad_x) * 2) + up256((rows + MTTS_ENTRY_GUARD_ROWS) * (2 * g->N + g->pad_out) * 2) + 256;
}
int mtts_conv_gn_args_run(mtts_conv_gn_args* g, void* d_scratch, void* stream) {
    RET_IF(conv_gn_args_check(g));
    g->tag[0] = 0;
    REFUSE_IF(!g->d_x || !g->d_w || !g->d_wpacked || !g->d_bias || !g->d_gamma || !g->d_beta || !g->d_mask || !d_scratch || !g->d_out, "mtts_conv_gn_args: null buffer");
    return conv_gn_run(*g, g->eps > 0.f ? g->eps : 1e-5f, true, d_scratch, static_cast<hipStream_t>(stream));
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
int mtts_tblock_chain_h16_timed(const float* d_att, const float* d_x, int M, int C, int inner, const float* h_w_out, const float* h_b_out,
                                const float* h_w1, const float* h_b1, const float* h_p0, const float* h_p1, const float* h_w2, const float* h_b2,
                                const float* h_w_qkv, const float* h_b_qkv, int n_qkv, const float* d_out_mask, int bf16, int qb, int ch,
                                int pf_wgs, float* d_x_out, float* d_qkv_out, void* d_scratch, void* stream, int repeat, float* h_ms) {
    mtts_chain_args g = chain_positional(d_att, d_x, M, C, inner, h_w_out, h_b_out, h_w1, h_b1, h_p0, h_p1, h_w2, h_b2, h_w_qkv, h_b_qkv, n_qkv, d_out_mask, qb, ch,
                                         d_x_out, d_qkv_out);
    REFUSE_IF(M <= 0 || !chain_h16_supported(C, inner, ch, g.n_qkv) || !d_x || !h_w1 || !h_w2 || !h_p0 || !h_p1 || !d_scratch || !d_x_out || (inner && (!d_att || !h_w_out)) ||
                  (g.n_qkv && !d_qkv_out),
              "mtts_tblock_chain_h16: unsupported shape or null buffer");
    ChainMode m;
    m.ew = 1; m.bf16 = bf16 != 0; m.pf_wgs = pf_wgs; m.repeat = repeat; m.h_ms = h_ms;
    return chain_run(g, g.n_qkv, m, d_scratch, static_cast<hipStream_t>(stream));
}
int mtts_tblock_chain_h16(const float* d_att, const float* d_x, int M, int C, int inner, const float* h_w_out, const float* h_b_out,
                          const float* h_w1, const float* h_b1, const float* h_p0, const float* h_p1, const float* h_w2, const float* h_b2,
                          const float* h_w_qkv, const float* h_b_qkv, int n_qkv, const float* d_out_mask, int bf16, int qb, int ch,
                          int pf_wgs, float* d_x_out, float* d_qkv_out, void* d_scratch, void* stream) {
    return mtts_tblock_chain_h16_timed(d_att, d_x, M, C, inner, h_w_out, h_b_out, h_w1, h_b1, h_p0, h_p1, h_w2, h_b2, h_w_qkv, h_b_qkv, n_qkv,
                                       d_out_mask, bf16, qb, ch, pf_wgs, d_x_out, d_qkv_out, d_scratch, stream, 0, nullptr);
}

// ---- the H16 instantiations of the estimator's kernels (16-bit storage modes: GemmArgs::half16 / bf16), one entry per kernel.
// fp32 rows are rounded to H16 images by launch_to_p16(half16), the kernels' H16 outputs are widened back by launch_from_h16, so
// a test sees exactly the 16-bit values the kernel wrote.  Host code only: every kernel launched here is one the model launches.
const char* mtts_last_kernel_tag(void) { return g_kernel_tag ? g_kernel_tag : ""; }

int mtts_panel_h16_host(const float* h_panel, int64_t n, int bf16, uint16_t* h_plane) {
    if (!h_panel || !h_plane || n <= 0) { set_error("mtts_panel_h16_host: null buffer"); return -1; }
    if (bf16) panel_bf16_host(h_panel, (size_t)n, h_plane);
    else panel_h16_host(h_panel, (size_t)n, h_plane);
    return 0;
}

int mtts_to_h16_roundtrip(const float* d_x, int ld, const float* d_mask, int M, int C, int C_valid, int ld16, int bf16, void* d_image,
                          float* d_out, unsigned int* d_range_flag, void* stream) {
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (!d_x || !d_image || !d_out) { set_error("mtts_to_h16_roundtrip: null buffer"); return -1; }
    if (M <= 0 || C <= 0 || (C % 64)) { set_error("mtts_to_h16_roundtrip: H16 operands need C % 64 == 0"); return -1; }
    if (C_valid < 0 || C_valid > C || (C_valid & 3) || ld < C_valid || (ld & 3) || ld16 < C || (ld16 & 3)) { set_error("mtts_to_h16_roundtrip: bad stride or C_valid"); return -1; }
    HIP_OK(launch_to_p16(d_x, ld, d_mask, M, C, C_valid, static_cast<_Float16*>(d_image), ld16, 1.0f, s, d_range_flag, true, bf16 != 0));
    HIP_OK(launch_from_h16(d_image, ld16, M, C, bf16 != 0, d_out, C, s));
    return 0;
}

int mtts_gemm_h16_wave_rows(int B, int T_out, int N, int force_bm) {
    if (B <= 0 || T_out <= 0 || N <= 0 || (force_bm != 0 && force_bm != 64 && force_bm != 128)) { set_error("mtts_gemm_h16_wave_rows: bad argument"); return -1; }
    GemmArgs a;
    a.B = B; a.T_out = T_out; a.N = N; a.force_bm = force_bm;
    return gemm_p16_wave_rows(a);
}
int64_t mtts_gemm_h16_scratch_bytes(const mtts_gemm_h16_args* g) {
    REFUSE_IF(block_sizes_bad(g), "mtts_gemm_h16_scratch_bytes: bad argument");
    const int64_t out_rows = (int64_t)g->B * (g->out_T > 0 ? g->out_T : g->T_out);
    const int64_t Np = round_up(g->N, GEMM_BN), Kp = (int64_t)g->ntaps * g->C;
    return (int64_t)g->B * g->T_in * g->C * 2 + 2 * out_rows * round_up(g->N, 64) * 2 + Np * Kp * 2 + Np * 4 + 2048;
}
int mtts_gemm_h16(mtts_gemm_h16_args* g, void* d_scratch, void* stream) {
    return gemm_image_run(g, 1, 0, 2048.0f, "mtts_gemm_h16", d_scratch, stream);
}

int mtts_attention_h16(const float* d_qkv, const float* d_mask, const int* d_klen, int B, int T, int H, int D, float scale, int mask_mode,
                       int bf16, float* d_out, unsigned int* d_range_flag, void* d_scratch, void* stream) {
    RET_IF(attention_image_check("mtts_attention_h16: ", "H16", d_qkv, d_mask, B, T, H, D, mask_mode, d_out, d_scratch));
    AttnMode m;
    m.ew = 1; m.bf16 = bf16 != 0; m.klen = d_klen; m.range_flag = d_range_flag;
    return attention_run(d_qkv, d_mask, B, T, H, D, scale, mask_mode, d_out, m, d_scratch, stream);
}

int mtts_groupnorm_mish_h16(const float* d_y, const float* d_gamma, const float* d_beta, const float* d_mask, const float* d_chbias,
                            int chbias_stride, int B, int T, int C, int G, float eps, const float* d_tile_stats, int tile_rows,
                            const int* d_nrows, const int* d_nextra, const float* d_bias_stats, const float* d_out16_mask, int bf16,
                            float* d_out, float* d_out16_f32, unsigned int* d_range_flag, void* d_scratch, void* stream) {
    return groupnorm_image("mtts_groupnorm_mish_h16", "H16", 1, bf16 != 0, d_y, d_gamma, d_beta, d_mask, d_chbias, chbias_stride, B, T, C, G, eps,
                           d_tile_stats, tile_rows, d_nrows, d_nextra, d_bias_stats, d_out16_mask, d_out, d_out16_f32, d_range_flag, d_scratch, stream);
}
int64_t mtts_groupnorm_h16_scratch_bytes(int B, int T, int C, int G) {
    REFUSE_IF(B <= 0 || T <= 0 || C <= 0 || G <= 0, "mtts_groupnorm_h16_scratch_bytes: bad argument");
    return gn_partial_bytes(B, T, G) + 256 + (int64_t)B * T * C * 2;
}

// ---- the two-plane (P16) instantiations of the same kernels: what the default arithmetic runs (gemm_p16_kernel MODE 0, MODE 1 with
// fast16; the <*, true, false, false, false, *> attention kernels; gn_apply_kernel's two-plane store; to_p16 / from_p16), one entry per
// kernel with every argument the decoder passes.  fp32 rows become P16 images by launch_to_p16 (residual scale 2048; 1 for the q|k|v
// image the attention kernel reads), images come back through launch_from_p16 as h + l / lscale.  Host code only.
int mtts_to_p16_roundtrip(const float* d_x, int ld, const float* d_mask, int M, int C, int C_valid, int ld16, float lscale, void* d_image,
                          float* d_out, unsigned int* d_range_flag, void* stream) {
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (!d_x || !d_image || !d_out) { set_error("mtts_to_p16_roundtrip: null buffer"); return -1; }
    if (M <= 0 || C <= 0 || (C % 32)) { set_error("mtts_to_p16_roundtrip: P16 operands need C % 32 == 0"); return -1; }
    if (C_valid < 0 || C_valid > C || (C_valid & 3) || ld < C_valid || (ld & 3) || ld16 < 2 * C || (ld16 & 3)) { set_error("mtts_to_p16_roundtrip: bad stride or C_valid"); return -1; }
    if (lscale != 2048.0f && lscale != 1.0f) { set_error("mtts_to_p16_roundtrip: lscale is 2048 or 1"); return -1; }
    HIP_OK(launch_to_p16(d_x, ld, d_mask, M, C, C_valid, static_cast<_Float16*>(d_image), ld16, lscale, s, d_range_flag));
    HIP_OK(launch_from_p16(static_cast<const _Float16*>(d_image), ld16, M, C, lscale, d_out, C, s));
    return 0;
}

int64_t mtts_gemm_p16_args_scratch_bytes(const mtts_gemm_h16_args* g) {
    REFUSE_IF(block_sizes_bad(g), "mtts_gemm_p16_args_scratch_bytes: bad argument");
    const int64_t out_rows = (int64_t)g->B * (g->out_T > 0 ? g->out_T : g->T_out);
    const int64_t Np = round_up(g->N, GEMM_BN), Kp = (int64_t)g->ntaps * g->C;
    return (int64_t)g->B * g->T_in * g->C * 4 + 2 * out_rows * round_up(g->N, 32) * 4 + 2 * Np * Kp * 4 + Np * 4 + 2048;
}
int mtts_gemm_p16_args_run(mtts_gemm_h16_args* g, int fast16, float out_lscale, void* d_scratch, void* stream) {
    return gemm_image_run(g, 2, fast16, out_lscale, "mtts_gemm_p16_args_run", d_scratch, stream);
}

int mtts_attention_p16_run(const float* d_qkv, const float* d_mask, const int* d_klen, int B, int T, int H, int D, float scale, int mask_mode,
                           int fast16, float out_lscale, float* d_out, unsigned int* d_range_flag, void* d_scratch, void* stream) {
    RET_IF(attention_image_check("mtts_attention_p16_run: ", "P16", d_qkv, d_mask, B, T, H, D, mask_mode, d_out, d_scratch));
    REFUSE_IF(fast16 != 0 && fast16 != 1, "mtts_attention_p16_run: fast16 is 0 or 1");
    REFUSE_IF(out_lscale != 2048.0f && out_lscale != 1.0f, "mtts_attention_p16_run: out_lscale is 2048 or 1");
    AttnMode m;
    m.ew = 2; m.fast16 = fast16 != 0; m.out_lscale = out_lscale; m.klen = d_klen; m.range_flag = d_range_flag;
    return attention_run(d_qkv, d_mask, B, T, H, D, scale, mask_mode, d_out, m, d_scratch, stream);
}

int64_t mtts_groupnorm_p16_scratch_bytes(int B, int T, int C, int G) {
    REFUSE_IF(B <= 0 || T <= 0 || C <= 0 || G <= 0, "mtts_groupnorm_p16_scratch_bytes: bad argument");
    return gn_partial_bytes(B, T, G) + 256 + (int64_t)B * T * C * 4;
}
int mtts_groupnorm_mish_p16(const float* d_y, const float* d_gamma, const float* d_beta, const float* d_mask, const float* d_chbias,
                            int chbias_stride, int B, int T, int C, int G, float eps, const float* d_tile_stats, int tile_rows,
                            const int* d_nrows, const int* d_nextra, const float* d_bias_stats, const float* d_out16_mask, float* d_out,
                            float* d_out16_f32, unsigned int* d_range_flag, void* d_scratch, void* stream) {
    return groupnorm_image("mtts_groupnorm_mish_p16", "P16", 2, false, d_y, d_gamma, d_beta, d_mask, d_chbias, chbias_stride, B, T, C, G, eps,
                           d_tile_stats, tile_rows, d_nrows, d_nextra, d_bias_stats, d_out16_mask, d_out, d_out16_f32, d_range_flag, d_scratch, stream);
}

// ---- the kernels that are not GEMMs: the Vocos tail (vocos.hip) and the solver / layout glue (norm_glue.hip).  Each entry refuses on
// the host what the host can decide, then calls the launcher the model calls, unchanged.
int mtts_dwconv7_ln(const float* d_x, const float* d_w7, const float* d_bias, const float* d_gamma, const float* d_beta, float eps,
                    int B, int T, int C, const int64_t* d_lengths, float* d_y, void* stream) {
    REFUSE_IF(!d_x || !d_w7 || !d_bias || !d_gamma || !d_beta || !d_y, "mtts_dwconv7_ln: null buffer");
    REFUSE_IF(B <= 0 || T <= 0, "mtts_dwconv7_ln: empty batch");
    REFUSE_IF(C <= 0 || (C & 3) || C > 2048, "mtts_dwconv7_ln: C must be a multiple of 4, at most 2048");
    HIP_OK(launch_dwconv7_ln(d_x, d_w7, d_bias, d_gamma, d_beta, eps, B, T, C, d_y, static_cast<hipStream_t>(stream), d_lengths));
    return 0;
}

int mtts_spec_polar(float* d_x, int M, int ld, int nbins, int off, float clip, void* stream) {
    REFUSE_IF(!d_x, "mtts_spec_polar: null buffer");
    REFUSE_IF(M <= 0 || nbins <= 0, "mtts_spec_polar: empty spectrum");
    REFUSE_IF(off < nbins || off + nbins > ld, "mtts_spec_polar: the two halves overlap or leave the row (nbins <= off, off + nbins <= ld)");
    HIP_OK(launch_spec_polar(d_x, M, ld, nbins, off, clip, static_cast<hipStream_t>(stream)));
    return 0;
}

int mtts_istft_ola(const float* d_frames, const float* d_window, int B, int T, int n_fft, int hop, const int64_t* d_lengths,
                   float* d_audio, void* stream) {
    REFUSE_IF(!d_frames || !d_window || !d_audio, "mtts_istft_ola: null buffer");
    REFUSE_IF(B <= 0, "mtts_istft_ola: empty batch");
    REFUSE_IF(T < 2, "mtts_istft_ola: need at least 2 frames");
    REFUSE_IF(n_fft <= 0 || hop <= 0 || n_fft % hop, "mtts_istft_ola: hop must divide n_fft");
    HIP_OK(launch_istft_ola(d_frames, d_window, B, T, n_fft, hop, d_audio, static_cast<hipStream_t>(stream), d_lengths));
    return 0;
}

int mtts_ode_combine(int stage, float dt, const float* d_dt_b, int T, const float* d_y, int ldy, const float* d_k1, const float* d_k2,
                     const float* d_k3, const float* d_k4, int ldk, float* d_out, int ldo, int M, int C, void* stream) {
    hipStream_t s = static_cast<hipStream_t>(stream);
    REFUSE_IF(stage < 0 || stage > 4, "mtts_ode_combine: stage is 0 .. 4");
    REFUSE_IF(!d_y || !d_k1 || !d_out || (stage >= 2 && !d_k2) || (stage >= 3 && !d_k3) || (stage >= 4 && !d_k4),
              "mtts_ode_combine: null buffer (stage k reads k1 .. k_k)");
    REFUSE_IF(M <= 0 || C <= 0, "mtts_ode_combine: empty state");
    REFUSE_IF(ldy < C || ldk < C || ldo < C, "mtts_ode_combine: a leading dimension is smaller than C");
    REFUSE_IF(d_out == d_y && ldo != ldy, "mtts_ode_combine: in place needs ldo == ldy");
    if (!d_dt_b) {
        HIP_OK(launch_ode_combine(stage, dt, d_y, ldy, d_k1, d_k2, d_k3, d_k4, ldk, d_out, ldo, M, C, s));
        return 0;
    }
    REFUSE_IF(T <= 0 || (M % T), "mtts_ode_combine: per-utterance dt needs T > 0 dividing M");
    HIP_OK(launch_ode_combine_rows(stage, d_dt_b, T, d_y, ldy, d_k1, d_k2, d_k3, d_k4, ldk, d_out, ldo, M, C, s));
    return 0;
}

int mtts_step_tables(const float* d_t0, const float* d_t1, const float* d_mask, int B, int T, int stages, float* d_tv, float* d_dt_b,
                     float* d_rs_full, float* d_rs_half, void* stream) {
    REFUSE_IF(!d_t0 || !d_t1 || !d_mask || !d_tv || !d_dt_b || !d_rs_full || !d_rs_half, "mtts_step_tables: null buffer");
    REFUSE_IF(B <= 0 || T <= 0, "mtts_step_tables: empty batch");
    REFUSE_IF(stages != 1 && stages != 2 && stages != 4, "mtts_step_tables: stages is 1 (euler), 2 (midpoint) or 4 (rk4)");
    HIP_OK(launch_step_tables(d_t0, d_t1, d_mask, B, T, stages, d_tv, d_dt_b, d_rs_full, d_rs_half, static_cast<hipStream_t>(stream)));
    return 0;
}

int mtts_time_sinusoid(const float* d_freqs, const float* h_t, const float* d_t, int nt, int half, float scale, float* d_out,
                       void* stream) {
    hipStream_t s = static_cast<hipStream_t>(stream);
    REFUSE_IF(!d_freqs || !d_out, "mtts_time_sinusoid: null buffer");
    REFUSE_IF((h_t != nullptr) == (d_t != nullptr), "mtts_time_sinusoid: the times come from h_t or from d_t, one of the two");
    REFUSE_IF(nt <= 0 || half <= 0, "mtts_time_sinusoid: empty table");
    if (d_t) {
        HIP_OK(launch_time_sinusoid_dev(d_freqs, d_t, nt, half, scale, d_out, s));
        return 0;
    }
    REFUSE_IF(nt > MAX_EVALS, "mtts_time_sinusoid: at most 256 host times (pass more in device memory)");
    TimeVals tv;
    for (int i = 0; i < MAX_EVALS; ++i) tv.t[i] = i < nt ? h_t[i] : 0.f;
    HIP_OK(launch_time_sinusoid(d_freqs, tv, nt, half, scale, d_out, s));
    return 0;
}

int mtts_rope(float* d_qkv, int B, int T, int H, int D, int d_rope, const float* d_cos, const float* d_sin, void* stream) {
    REFUSE_IF(!d_qkv || !d_cos || !d_sin, "mtts_rope: null buffer");
    REFUSE_IF(B <= 0 || T <= 0 || H <= 0 || D <= 0, "mtts_rope: empty batch");
    REFUSE_IF(d_rope <= 0 || (d_rope & 1) || d_rope > D, "mtts_rope: d_rope must be even and within the head (0 < d_rope <= D)");
    HIP_OK(launch_rope(d_qkv, B, T, H, D, d_rope, d_cos, d_sin, static_cast<hipStream_t>(stream)));
    return 0;
}

int mtts_cf_to_cl(const float* d_src, const float* d_add, int B, int C, int T, int T_src, float* d_dst, int ld, int col_off,
                  const int64_t* d_lengths, void* stream) {
    REFUSE_IF(!d_src || !d_dst, "mtts_cf_to_cl: null buffer");
    REFUSE_IF(B <= 0 || C <= 0 || T <= 0, "mtts_cf_to_cl: empty batch");
    REFUSE_IF(T_src != 0 && T_src < T, "mtts_cf_to_cl: T_src is shorter than T");
    REFUSE_IF(col_off < 0 || col_off + C > ld, "mtts_cf_to_cl: ld is smaller than col_off + C");
    HIP_OK(launch_cf_to_cl(d_src, d_add, B, C, T, d_dst, ld, col_off, static_cast<hipStream_t>(stream), T_src, d_lengths));
    return 0;
}

int mtts_cl_to_cf(const float* d_src, int ld, int B, int C, int T, float* d_dst, int T_out, float scale, float shift, void* stream) {
    REFUSE_IF(!d_src || !d_dst, "mtts_cl_to_cf: null buffer");
    REFUSE_IF(B <= 0 || C <= 0 || T <= 0, "mtts_cl_to_cf: empty batch");
    REFUSE_IF(T_out <= 0 || T_out > T, "mtts_cl_to_cf: T_out must be within 1 .. T");
    REFUSE_IF(ld < C, "mtts_cl_to_cf: ld is smaller than C");
    HIP_OK(launch_cl_to_cf(d_src, ld, B, C, T, d_dst, T_out, scale, shift, static_cast<hipStream_t>(stream)));
    return 0;
}

int mtts_slots_to_cl(const float* d_pool, const int32_t* d_slots, int S, int T_pool, int B, int C, int T, float* d_dst, int ld,
                     int col_off, void* stream) {
    REFUSE_IF(!d_pool || !d_slots || !d_dst, "mtts_slots_to_cl: null buffer");
    REFUSE_IF(S <= 0 || B <= 0 || C <= 0 || T <= 0, "mtts_slots_to_cl: empty batch or pool");
    REFUSE_IF(T > T_pool, "mtts_slots_to_cl: T is longer than T_pool");
    REFUSE_IF(col_off < 0 || col_off + C > ld, "mtts_slots_to_cl: ld is smaller than col_off + C");
    HIP_OK(launch_slots_to_cl(d_pool, d_slots, S, T_pool, B, C, T, d_dst, ld, col_off, static_cast<hipStream_t>(stream)));
    return 0;
}

int mtts_cl_to_slots(const float* d_src, int ld, int B, int C, int T, float* d_pool, const int32_t* d_slots, int S, int T_pool,
                     void* stream) {
    REFUSE_IF(!d_src || !d_pool || !d_slots, "mtts_cl_to_slots: null buffer");
    REFUSE_IF(S <= 0 || B <= 0 || C <= 0 || T <= 0, "mtts_cl_to_slots: empty batch or pool");
    REFUSE_IF(T > T_pool, "mtts_cl_to_slots: T is longer than T_pool");
    REFUSE_IF(ld < C, "mtts_cl_to_slots: ld is smaller than C");
    HIP_OK(launch_cl_to_slots(d_src, ld, B, C, T, d_pool, d_slots, S, T_pool, static_cast<hipStream_t>(stream)));
    return 0;
}
// ---- the fp32-row flow (fp32 rows in, fp32 rows out): gemm_f32_kernel at terms 0 / 2 / 6 with every argument the encoder, the
// duration predictor and the full-range estimator pass; attention_f32_kernel<NW, false> with klen; gn_partial + gn_apply with the
// fp32 store.  A stays fp32 rows (no image), the panel and its planes are made on the host as the model's packer makes them.
#define GF "mtts_gemm_f32_args_run: "
static int gemm_f32_args_check(const mtts_gemm_h16_args* g, int terms, const float* d_a1, int lda1, int ldc, float out_lscale, OutRows* r) {
    REFUSE_IF(!g, GF "null argument block");
    REFUSE_IF(!g->d_a || !g->h_w || (!g->d_out && !g->d_out16_f32), GF "null buffer");
    REFUSE_IF(g->half16 || g->bf16, GF "launches the fp32-row instantiations only (half16 and bf16 must be 0)");
    REFUSE_IF(terms != 0 && terms != 2 && terms != 6, GF "terms must be 0, 2 or 6");
    REFUSE_IF(out_lscale != 2048.0f && out_lscale != 1.0f, GF "out_lscale is 2048 or 1");
    REFUSE_IF(g->res16_mode || g->d_res16_f32 || g->out16_preload, GF "res16 and out16_preload belong to the P16 kernel");
    REFUSE_IF(g->d_gn_stats || g->gn_groups || g->d_gn_nrows, GF "gn_stats belongs to the P16 kernel");
    REFUSE_IF(g->d_gnr_y || g->d_gnr_stats || g->d_gnr_gamma || g->d_gnr_beta || g->d_gnr_mask || g->d_gnr_nextra || g->d_gnr_bias_stats,
              GF "gnr (the Block1D tail) belongs to the P16 kernel");
    REFUSE_IF(g->ntaps < 1 || g->ntaps > MAX_TAPS, GF "ntaps out of range");
    REFUSE_IF(g->B <= 0 || g->T_in <= 0 || g->T_out <= 0 || g->N <= 0 || g->in_stride < 0, GF "bad shape");
    const int C = g->C, c1 = g->c1, c0 = C - c1, N = g->N, L = ldc ? ldc : N;
    REFUSE_IF(C <= 0 || c1 < 0 || c1 >= C || (c0 & 3) || (c1 & 3), GF "C and c1 must be multiples of 4, c1 < C");
    REFUSE_IF(c1 && (c0 % GEMM_BK), GF "a second segment needs (C - c1) % 32 == 0");
    REFUSE_IF(d_a1 && !c1, GF "d_a1 without c1");
    REFUSE_IF((g->lda & 3) || g->lda < (d_a1 ? c0 : C), GF "lda");
    REFUSE_IF(d_a1 && ((lda1 & 3) || lda1 < c1), GF "lda1");
    REFUSE_IF(ldc < 0 || (g->d_out && L < N), GF "ldc");
    REFUSE_IF(g->d_res && g->ldr < N, GF "ldr");
    REFUSE_IF(g->d_out16_f32 && ((N % 32) || (g->d_out && (L & 3)) || (g->d_res && (g->ldr & 3))),
              GF "a P16 copy of the result needs N % 32 == 0 and ldc, ldr % 4 == 0");
    REFUSE_IF((g->d_a_mean == nullptr) != (g->d_a_rstd == nullptr), GF "a_mean and a_rstd come together");
    REFUSE_IF(g->d_a_part && (g->d_a_mean || g->a_nparts <= 0), GF "a_part excludes a_mean and needs a_nparts > 0");
    REFUSE_IF((g->d_a_mean || g->d_a_part) && (g->ntaps != 1 || g->in_stride > 1 || (g->h_tap_off && g->h_tap_off[0] != 0)),
              GF "LayerNorm in the prologue needs a plain Linear (one tap, offset 0, stride 1)");
    REFUSE_IF(g->d_stats_out && ((N & 63) || !g->d_out || (L & 3) || (g->d_res && (g->ldr & 3))), GF "stats_out needs N % 64 == 0, fp32 rows and ldc, ldr % 4 == 0");
    REFUSE_IF(g->act < ACT_NONE || g->act > ACT_GELU, GF "act");
    REFUSE_IF(g->act == ACT_SNAKE && (!g->d_p0 || !g->d_p1), GF "SnakeBeta needs p0 and p1");
    REFUSE_IF(g->force_bm != 0 && g->force_bm != 64 && g->force_bm != 128, GF "force_bm is 0, 64 or 128");
    return block_out_rows(g, GF, r);
}
static void gemm_f32_args_sizes(const mtts_gemm_h16_args* g, size_t* image, size_t* npanel) {
    const size_t out_rows = (size_t)g->B * (g->out_T > 0 ? g->out_T : g->T_out);
    *image = g->d_out16_f32 ? (out_rows + MTTS_ENTRY_GUARD_ROWS) * 2 * (size_t)g->N * 2 : 0;
    *npanel = (size_t)round_up(g->N, GEMM_BN) * g->ntaps * round_up(g->C, GEMM_BK);
}
int64_t mtts_gemm_f32_args_scratch_bytes(const mtts_gemm_h16_args* g) {
    REFUSE_IF(block_sizes_bad(g), "mtts_gemm_f32_args_scratch_bytes: bad argument");
    size_t image, npanel;
    gemm_f32_args_sizes(g, &image, &npanel);
    return (int64_t)(up256(image) + up256(npanel * 4) + up256(npanel * 6) + 512);
}
int mtts_gemm_f32_args_run(mtts_gemm_h16_args* g, int terms, const float* d_a1, int lda1, int ldc, float out_lscale, void* d_scratch, void* stream) {
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (g) { g->tag[0] = 0; g->wave_rows = 0; }
    OutRows r;
    RET_IF(gemm_f32_args_check(g, terms, d_a1, lda1, ldc, out_lscale, &r));
    REFUSE_IF(!d_scratch, GF "null buffer");
    const int C = g->C, c1 = g->c1, c0 = C - c1, N = g->N, ktap = round_up(C, GEMM_BK);
    const size_t out_rows = (size_t)g->B * r.out_T;
    size_t image, npanel;
    gemm_f32_args_sizes(g, &image, &npanel);
    // host: the panel, and its planes as the model's packer stores them (pack.hip add_planes)
    std::vector<float> panel(npanel);
    pack_weight_host(g->h_w, g->ntaps > 1 ? 1 : 0, N, C, g->ntaps, 0, nullptr, nullptr, panel.data(), ktap);
    std::vector<uint16_t> planes(terms == 6 ? 3 * npanel : (terms == 2 ? 2 * npanel : 0));
    if (terms == 2) split_panel_f16_host(panel.data(), npanel, planes.data());
    if (terms == 6) split_panel_host(panel.data(), npanel, planes.data());
    Scratch sc(d_scratch);
    _Float16* o16 = sc.carve<_Float16>(image);            // first, so a caller finds the raw image
    float* d_panel = sc.carve<float>(npanel * 4);
    void* d_planes = sc.carve(npanel * 6);
    HIP_OK(hipMemcpyAsync(d_panel, panel.data(), npanel * 4, hipMemcpyHostToDevice, s));
    if (terms) HIP_OK(hipMemcpyAsync(d_planes, planes.data(), planes.size() * 2, hipMemcpyHostToDevice, s));
    HIP_OK(hipStreamSynchronize(s));                      // (the host vectors go out of scope)
    if (image) HIP_OK(fill16(o16, 0x7e00, image / 2, s));
    GemmArgs a;
    a.a0 = g->d_a; a.lda0 = g->lda; a.c0 = c0; a.ktap = ktap;
    if (c1) { a.a1 = d_a1 ? d_a1 : g->d_a + c0; a.lda1 = d_a1 ? lda1 : g->lda; a.c1 = c1; }
    block_prologue(a, g);
    a.a_mask = g->d_a_mask;
    a.w = d_panel; a.w16 = terms ? d_planes : nullptr; a.terms = terms;
    block_epilogue(a, g, o16, nullptr, 2, r);             // (res16, gn_stats and gnr were refused: those fields stay unset)
    a.ldc = ldc ? ldc : N;
    if (g->d_out16_f32) a.out_lscale = out_lscale;
    g_kernel_tag = nullptr;
    HIP_OK(launch_gemm(a, s));
    copy_tag(g->tag);
    if (g->d_out16_f32) HIP_OK(launch_from_p16(o16, 2 * N, (int)out_rows, N, out_lscale, g->d_out16_f32, N, s));
    return 0;
}
#undef GF

int mtts_attention_f32_run(const float* d_qkv, const float* d_mask, const int* d_klen, int B, int T, int H, int D, float scale, int mask_mode,
                           float* d_out, void* stream) {
    REFUSE_IF(!d_qkv || !d_out, "mtts_attention_f32_run: null buffer");
    REFUSE_IF(B <= 0 || T <= 0 || H <= 0, "mtts_attention_f32_run: empty batch");
    REFUSE_IF(D <= 0 || D > 64 || (D & 3), "mtts_attention_f32_run: the head dim is a multiple of 4, at most 64");
    REFUSE_IF(mask_mode != 0 && mask_mode != 1, "mtts_attention_f32_run: mask_mode is 0 or 1");
    REFUSE_IF(mask_mode == 1 && !d_mask, "mtts_attention_f32_run: the boolean mask mode needs a mask");
    AttnMode m;
    m.klen = d_klen;
    return attention_run(d_qkv, d_mask, B, T, H, D, scale, mask_mode, d_out, m, nullptr, stream);
}

int mtts_groupnorm_mish_f32_run(const float* d_y, const float* d_gamma, const float* d_beta, const float* d_mask, const float* d_chbias,
                                int chbias_stride, const float* d_res, int ldr, int B, int T, int C, int G, float eps, const int* d_nrows,
                                const int* d_nextra, const float* d_bias_stats, float* d_out, float* d_stats_out, void* d_scratch,
                                void* stream) {
    REFUSE_IF(!d_y || !d_gamma || !d_beta || !d_mask || !d_out || !d_scratch, "mtts_groupnorm_mish_f32_run: null buffer");
    REFUSE_IF(B <= 0 || T <= 0 || C <= 0 || G <= 0 || G > 64 || (C % G) || ((C / G) & 3) || C > 4096,
              "mtts_groupnorm_mish_f32_run: C % G == 0 with (C / G) % 4 == 0, C <= 4096, G <= 64 and a non-empty batch");
    REFUSE_IF(d_chbias && chbias_stride && (chbias_stride < C || (chbias_stride & 3)),
              "mtts_groupnorm_mish_f32_run: a bias row per utterance has at least C values (stride % 4 == 0)");
    REFUSE_IF((d_nextra != nullptr) != (d_bias_stats != nullptr), "mtts_groupnorm_mish_f32_run: nextra and bias_stats come together");
    REFUSE_IF(d_res && (ldr < C || (ldr & 3)), "mtts_groupnorm_mish_f32_run: ldr is at least C and a multiple of 4");
    REFUSE_IF(d_stats_out && (C & 63), "mtts_groupnorm_mish_f32_run: stats_out needs C % 64 == 0");
    GnEntry e;
    e.y = d_y; e.gamma = d_gamma; e.beta = d_beta; e.mask = d_mask; e.chbias = d_chbias; e.chbias_stride = d_chbias ? chbias_stride : 0;
    e.res = d_res; e.ldr = ldr; e.B = B; e.T = T; e.C = C; e.G = G; e.eps = eps > 0.f ? eps : 1e-5f;
    e.nrows = d_nrows; e.nextra = d_nextra; e.bias_stats = d_bias_stats; e.out = d_out; e.stats_out = d_stats_out;
    return groupnorm_run(e, d_scratch, stream);
}

// mtts_channel_layernorm with the leading dimensions the model passes (rows of a wider buffer in, rows of a wider buffer out)
int mtts_channel_layernorm_ld(const float* d_x, int ldx, int B, int T, int C, const float* d_gamma, const float* d_beta, float eps, int act,
                              const float* d_film, const float* d_mask, float* d_y, int ldy, void* stream) {
    REFUSE_IF(!d_x || !d_gamma || !d_beta || !d_y, "mtts_channel_layernorm_ld: null buffer");
    REFUSE_IF(B <= 0 || T <= 0, "mtts_channel_layernorm_ld: empty batch");
    REFUSE_IF(C <= 0 || (C & 3) || C > 2048, "mtts_channel_layernorm_ld: C must be a multiple of 4, at most 2048");
    REFUSE_IF(ldx < C || (ldx & 3) || ldy < C || (ldy & 3), "mtts_channel_layernorm_ld: a leading dimension is at least C and a multiple of 4");
    REFUSE_IF(act != ACT_NONE && act != ACT_SILU, "mtts_channel_layernorm_ld: act must be 0 (none) or 2 (SiLU)");
    return layernorm_run(d_x, ldx, B, T, C, d_gamma, d_beta, eps, act, d_film, d_mask, d_y, ldy, stream);
}
#undef REFUSE_IF

}  // extern "C"
