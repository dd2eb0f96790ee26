// A Block1D of the decoder's ResNet blocks as ONE launch for gfx950: Conv1d(k3, p1) -> GroupNorm(8) -> Mish -> mask [-> + time
// bias -> mask], P16 image in, P16 image out.
//
// Tiling: one workgroup per (utterance b, GroupNorm group g) -- all T rows of the utterance x the N/8 = 48 channels of the group.
// Such a workgroup owns its GroupNorm statistics completely, so the conv's fp32 rows, the per-tile statistics entries and the
// gn_apply pass of the tiled path (gemm_p16.hip + norm_glue.hip) do not exist here and nothing waits for another workgroup.
// The 8 groups of an utterance run on one XCD (they read the same activation rows through one L2).
//
// Operands as gemm_p16.hip takes them: P16 images (kernels.h) moved global -> LDS by LDS-DMA, the same 128-byte line image with
// the same 16-byte-chunk swizzle, the weight panel as packed for gemm_p16_kernel (a group's 48 channels = 48 panel rows), three
// v_mfma_f32_16x16x32_f16 per 16 x 16 x 32 block in the same order.  What differs is the K loop: because the workgroup owns the
// whole utterance, a ring stage holds the (T + 2)-row SLAB of one 32-channel chunk ONCE and the three taps read it at row offsets
// 0 / 1 / 2 -- a third of the activation traffic of three shifted tiles -- beside the chunk's three 48-row weight lines.
//   stage = [slab: 200 rows x 128 B | weights: 3 taps x 48 rows x 128 B] = 43 KB, 3 stages, two in flight across a raw s_barrier
//   (counted s_waitcnt vmcnt, as gemm_p16_kernel's ring); up to 192 rows per utterance.
// Eight waves = two sets of four; wave w of either set holds rows [48 w, 48 w + 48) x 48 channels (3 x 3 MFMA tiles).  The sets
// split the K axis: k-step u of stage n belongs to set (n + u) & 1.  The sets' partial tiles are added in a fixed order, the
// GroupNorm moments are an exact two-pass reduction in a fixed order: results are run-to-run identical.
// Longer utterances (up to 384 rows, the full-length level): eight waves on eight row blocks, no K split, two stages of a 392-row slab.
// Replaces, on the hot path: Block1D / ResnetBlock1D of the reference decoder (decoder.py:32-63).
#include "kernels.h"
#include "device_utils.h"
#include <string>

namespace mtts {

using f32x4 = __attribute__((ext_vector_type(4))) float;
using f16x8 = __attribute__((ext_vector_type(8))) _Float16;

__device__ __attribute__((aligned(128))) _Float16 g_cg_zero_line[64];      // source of the slab rows outside the utterance

#define MTTS_CG_GLDS16(gp, lp) \
    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(gp), (__attribute__((address_space(3))) void*)(lp), 16, 0, 0)

// Two wave layouts.  KS = 2 (up to 192 rows): two K-splitting sets of four waves, wave w of either set holds rows [48 w, 48 w + 48),
// three ring stages.  KS = 1 (up to 384 rows, the full-length level): eight waves on rows [48 w, 48 w + 48), every wave runs all
// taps, two stages of the longer slab (LDS holds no third).
constexpr int CG_NT = CONV_GN_CPG / 16;            // 16-column tiles per group (48 channels)
constexpr int CG_W_PIECES = CG_NT * 2;             // 8-row DMA pieces of one tap's weight lines
constexpr int CG_PS = CONV_GN_CPG + 4;             // row stride (floats) of the parked tile: the four row blocks of a D fragment on distinct banks
static_assert(CG_NT == 3, "wave tiling below: 3 row tiles x 3 column tiles per wave");
template <int KS>
struct CgShape {
    static constexpr int ROWS = KS == 2 ? CONV_GN_SPLIT_ROWS : CONV_GN_MAX_ROWS;      // row capacity = 48 rows x (4 | 8) waves
    static constexpr int SLAB_PIECES = (ROWS + 2 + 7) / 8;                            // 8-row DMA pieces of the slab (rows -1 .. T)
    static constexpr int PIECES = SLAB_PIECES + 3 * CG_W_PIECES;                      // per stage, dealt round-robin to the 8 waves
    static constexpr int NJ = (PIECES + 7) / 8, NA = (SLAB_PIECES + 7) / 8;           // pieces / slab pieces per wave at most
    static constexpr int STAGE = PIECES * 1024;
    static constexpr int NST = KS == 2 ? 3 : 2;
    static constexpr int RED = NST * STAGE;        // byte offset of the reduction scratch behind the ring
    static constexpr int LDS = RED + 256;
    static constexpr int NPASS = ROWS / 64;        // epilogue passes of 64 rows
    static_assert(ROWS == 48 * 8 / KS, "rows per wave");
    static_assert(LDS <= 160 * 1024, "LDS per workgroup");
    static_assert(ROWS * CG_PS * 4 <= RED, "the parked tile overlays the ring");
};

// wait until at most n of this wave's DMA pieces are outstanding (n = its pieces of the one younger stage), then the barrier:
// the stage about to be computed has landed for everyone and everyone's fragment reads of the stage about to be refilled are done
__device__ __forceinline__ void cg_wait_barrier(int n) {
    switch (n) {
        case 6: asm volatile("s_waitcnt vmcnt(6) lgkmcnt(0)\n\ts_barrier" ::: "memory"); break;
        case 5: asm volatile("s_waitcnt vmcnt(5) lgkmcnt(0)\n\ts_barrier" ::: "memory"); break;
        default: asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)\n\ts_barrier" ::: "memory"); break;
    }
}

// The DMA requests of one wave for one stage: chunk cc of (img0 | img1) into the slab, the three taps' weight lines of 48 rows behind it.
// A plain function of VALUES on purpose: written as a lambda over the kernel's argument struct, the compiler turns the selects
// between operands into loads from a table in scratch memory, and scratch loads would enter the ring's counted waits.
template <int SP, int NJ, int NA>
__device__ __forceinline__ void cg_issue(char* st, int cc, int nc0, const _Float16* img0, const _Float16* img1, int ld0, int ld1,
                                         const _Float16* wgrp, size_t wld, int tapk, int wv, int lane, int ch_a, int ch_w, const int (&ar)[NA]) {
    const bool s1 = cc >= nc0;
    const _Float16* img = (s1 ? img1 : img0) + (s1 ? cc - nc0 : cc) * 64;
    const int ld = s1 ? ld1 : ld0;
    const _Float16* wsrc = wgrp + cc * 64;             // weight line of (row 0 of the group, tap 0, this chunk)
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        const int q = wv + 8 * j;                      // wave-uniform
        if (q >= SP + 3 * CG_W_PIECES) continue;
        const _Float16* src;
        if (j < NA && q < SP) {
            const int a = ar[j < NA ? j : 0];
            src = a >= 0 ? img + (size_t)a * ld + ch_a : g_cg_zero_line + ch_a;
        } else {
            const int pw = q - SP, tap = pw / CG_W_PIECES, row = (pw - tap * CG_W_PIECES) * 8 + (lane >> 3);
            src = wsrc + (size_t)row * wld + tap * tapk + ch_w;
        }
        MTTS_CG_GLDS16(src, st + q * 1024);
    }
}

template <int KS>
__global__ __launch_bounds__(512, 1) void conv_gn_kernel(const ConvGnArgs p) {
    using S = CgShape<KS>;
    extern __shared__ __attribute__((aligned(16))) char lds[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);          // wave of the workgroup: DMA piece owner
    const int ks = KS == 2 ? wv >> 2 : 0, wave = KS == 2 ? wv & 3 : wv;   // K set, row block
    int swz;       // XCD-aware order: the 8 groups of an utterance on one XCD (same remap as gemm_p16_kernel)
    {
        const int nwg = gridDim.x, id = blockIdx.x;
        const int xcd = id & 7, q = nwg >> 3, r = nwg & 7;
        swz = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (id >> 3);
    }
    const int b = swz >> 3, g = swz & 7;
    const int T = p.T;
    const int ktap = p.c0 + p.c1, Kp = 3 * ktap;
    const int nstage = ktap >> 5;              // one stage per 32-channel chunk

    // ---- DMA coordinates.  Piece q of a stage (q < SLAB_PIECES: slab rows 8 q .. 8 q + 7, then the weight pieces) belongs to wave q & 7;
    // lane i fills bytes [16 i, 16 i + 16) of the piece = row i >> 3, slot i & 7, which holds chunk (i & 7) ^ ((row >> 1) & 7).
    const int ch_a = ((lane & 7) ^ (((wv & 1) * 4 + (lane >> 4)) & 7)) * 8;            // slab pieces: piece parity = wv & 1
    const int ch_w = ((lane & 7) ^ ((((wv & 1) ^ (S::SLAB_PIECES & 1)) * 4 + (lane >> 4)) & 7)) * 8;
    int arow[S::NA];                                                   // image row of this lane's slab rows, -1 = outside the utterance
#pragma unroll
    for (int j = 0; j < S::NA; ++j) {
        const int t = (wv + 8 * j) * 8 + (lane >> 3) - 1;
        arow[j] = (unsigned)t < (unsigned)T ? b * T + t : -1;
    }
    const int my_pieces = (S::PIECES - wv + 7) >> 3;                   // this wave's pieces of a stage (KS = 2: 6 for waves 0-2, else 5)
    auto issue = [&](int n, int slot) __attribute__((always_inline)) {
        cg_issue<S::SLAB_PIECES, S::NJ, S::NA>(lds + slot * S::STAGE, n, p.c0 >> 5, p.a16_0, p.a16_1, p.lda16_0, p.lda16_1,
                                               reinterpret_cast<const _Float16*>(p.w16) + (size_t)(g * CONV_GN_CPG) * Kp * 2, (size_t)Kp * 2, ktap * 2,
                                               wv, lane, ch_a, ch_w, arow);
    };

    f32x4 acc[CG_NT][CG_NT], accx[CG_NT][CG_NT];     // [row tile][column tile]
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) { acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f}; accx[i][j] = acc[i][j]; }

    // operand fragment: lane (r = lane & 15, q = lane >> 4) holds k = 8 q .. 8 q + 7 of row r -- head chunk q, residual chunk 4 + q
    const int fr = lane & 15, fq = lane >> 4;
    const int f8w = (fr >> 1) & 7;
    // one k-step = one tap u: slab rows (48 wave + 16 i + r + u) x the tap's weight lines
    auto kstep = [&](const char* st, int u) __attribute__((always_inline)) {
        const int R0 = wave * 48 + fr + u, f8a = (R0 >> 1) & 7;     // (row >> 1) & 7 is the same for the three row tiles
        const char* sa = st + R0 * 128;
        const char* sw = st + S::SLAB_PIECES * 1024 + (u * CONV_GN_CPG + fr) * 128;
        const int ah_o = (fq ^ f8a) * 16, al_o = ((4 + fq) ^ f8a) * 16, bh_o = (fq ^ f8w) * 16, bl_o = ((4 + fq) ^ f8w) * 16;
        f16x8 ah[3], al[3];
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            ah[i] = *reinterpret_cast<const f16x8*>(sa + i * 16 * 128 + ah_o);
            al[i] = *reinterpret_cast<const f16x8*>(sa + i * 16 * 128 + al_o);
        }
        f16x8 bh[3], bl[3];
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            bh[j] = *reinterpret_cast<const f16x8*>(sw + j * 16 * 128 + bh_o);
            bl[j] = *reinterpret_cast<const f16x8*>(sw + j * 16 * 128 + bl_o);
        }
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                accx[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah[i], bl[j], accx[i][j], 0, 0, 0);
                accx[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(al[i], bh[j], accx[i][j], 0, 0, 0);
                acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah[i], bh[j], acc[i][j], 0, 0, 0);
            }
    };

    constexpr int D = S::NST - 1;              // stages in flight: the one about to be computed + D - 1 behind it
    issue(0, 0);
    if (D > 1 && nstage > 1) issue(1, 1);
    int slot = 0;
    for (int n = 0; n < nstage; ++n) {
        cg_wait_barrier(D > 1 && n + 1 < nstage ? my_pieces : 0);
        if (n + D < nstage) issue(n + D, slot == 0 ? S::NST - 1 : slot - 1);       // (the stage computed in the previous iteration)
        const char* st = lds + slot * S::STAGE;
#pragma unroll
        for (int u = 0; u < 3; ++u)
            if (KS == 1 || ((n + u) & 1) == ks) kstep(st, u);
        slot = slot == S::NST - 1 ? 0 : slot + 1;
    }
    __syncthreads();                       // the parked tile overlays the ring: everyone is done reading

    // ---- park the tile; KS = 2: the two sets' partial tiles meet in LDS -- set 1 parks, set 0 adds (set 0 + set 1, fixed) and parks the sum
    float* P = reinterpret_cast<float*>(lds);
    auto park = [&](bool add) __attribute__((always_inline)) {
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int j = 0; j < 3; ++j)
#pragma unroll
                for (int r = 0; r < 4; ++r) {      // D of 16x16x32: lane (col = lane & 15, row block lane >> 4), register r = row 4 (lane >> 4) + r
                    float* q = P + (wave * 48 + i * 16 + 4 * fq + r) * CG_PS + j * 16 + fr;
                    float v = acc[i][j][r] + accx[i][j][r] * (1.0f / F16_RES_SCALE);
                    if (add) v += q[0];
                    q[0] = v;
                }
    };
    if constexpr (KS == 2) {
        if (ks == 1) park(false);
        __syncthreads();
        if (ks == 0) park(true);
    } else park(false);

    // ---- rows: 8 lanes per row (6 of them hold 8 channels each), 64 rows per pass.  Column constants first (their flight
    // overlaps the reductions).
    const int oct = tid & 7, c0g = g * CONV_GN_CPG + (oct < 6 ? oct : 0) * 8;
    const bool live = oct < 6;
    const f32x4 bi0 = *reinterpret_cast<const f32x4*>(p.bias + c0g), bi1 = *reinterpret_cast<const f32x4*>(p.bias + c0g + 4);
    const f32x4 gm0 = *reinterpret_cast<const f32x4*>(p.gamma + c0g), gm1 = *reinterpret_cast<const f32x4*>(p.gamma + c0g + 4);
    const f32x4 bt0 = *reinterpret_cast<const f32x4*>(p.beta + c0g), bt1 = *reinterpret_cast<const f32x4*>(p.beta + c0g + 4);
    f32x4 cb0 = {0.f, 0.f, 0.f, 0.f}, cb1 = cb0;
    if (p.chbias) {        // (chbias_stride != 0: utterance b's own row -- one time per utterance, mtts_cfm_step)
        const float* cbp = p.chbias + (size_t)b * p.chbias_stride + c0g;
        cb0 = *reinterpret_cast<const f32x4*>(cbp); cb1 = *reinterpret_cast<const f32x4*>(cbp + 4);
    }
    const int nr = p.nrows ? max(0, min(T, p.nrows[b])) : T;          // rows that enter the statistics
    float x_ne = 0.f, x_bm = 0.f, x_bq = 0.f;
    if (p.nextra) { x_ne = (float)p.nextra[b]; x_bm = p.bias_stats[2 * g]; x_bq = p.bias_stats[2 * g + 1]; }
    float mk[S::NPASS], m16[S::NPASS];
#pragma unroll
    for (int it = 0; it < S::NPASS; ++it) {
        const int row = it * 64 + (tid >> 3);
        const bool in = row < T;
        mk[it] = in ? p.mask[b * T + row] : 0.f;
        m16[it] = in && p.out16_mask ? p.out16_mask[b * T + row] : 1.0f;
    }
    __syncthreads();                       // the summed tiles are parked

    float v[S::NPASS][8];
    float s = 0.f;
#pragma unroll
    for (int it = 0; it < S::NPASS; ++it) {
        const int row = it * 64 + (tid >> 3);
        const float* q = P + row * CG_PS + (live ? oct : 0) * 8;
        const f32x4 a0 = *reinterpret_cast<const f32x4*>(q) + bi0, a1 = *reinterpret_cast<const f32x4*>(q + 4) + bi1;
#pragma unroll
        for (int e = 0; e < 4; ++e) { v[it][e] = a0[e]; v[it][4 + e] = a1[e]; }
        if (live && row < nr) s += ((a0[0] + a0[1]) + (a0[2] + a0[3])) + ((a1[0] + a1[1]) + (a1[2] + a1[3]));
    }
    float* red = reinterpret_cast<float*>(lds + S::RED);
    auto block_sum = [&](float x, float* slot8) __attribute__((always_inline)) {                      // fixed order: butterfly inside a wave, then the 8 waves in order
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) x += __shfl_xor(x, off);
        if (lane == 0) slot8[wv] = x;
        __syncthreads();
        return ((slot8[0] + slot8[1]) + (slot8[2] + slot8[3])) + ((slot8[4] + slot8[5]) + (slot8[6] + slot8[7]));
    };
    float n = (float)(nr * CONV_GN_CPG);
    const float total = block_sum(s, red);
    float mean = n > 0.f ? total / n : 0.f;
    float qd = 0.f;
#pragma unroll
    for (int it = 0; it < S::NPASS; ++it) {
        const int row = it * 64 + (tid >> 3);
        if (live && row < nr) {
#pragma unroll
            for (int e = 0; e < 8; ++e) { const float d = v[it][e] - mean; qd += d * d; }
        }
    }
    float m2 = block_sum(qd, red + 8);
    if (x_ne > 0.f) {                      // folded padding: nextra copies of the conv's bias row in closed form (as gn_apply_kernel)
        const float nb = x_ne * (float)CONV_GN_CPG, delta = x_bm - mean, nt = n + nb;
        mean += delta * (nb / nt);
        m2 += x_ne * x_bq + delta * delta * (n * nb / nt);
        n = nt;
    }
    const float rs = n > 0.f ? 1.0f / sqrtf(m2 / n + p.eps) : 0.f;

    bool range_bad = false;
#pragma unroll
    for (int it = 0; it < S::NPASS; ++it) {
        const int row = it * 64 + (tid >> 3);
        const bool in = row < T;
        float o[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const float gme = e < 4 ? gm0[e & 3] : gm1[e & 3], bte = e < 4 ? bt0[e & 3] : bt1[e & 3];
            o[e] = mish_f(((v[it][e] - mean) * rs) * gme + bte) * mk[it];
            if (p.chbias) o[e] = (o[e] + (e < 4 ? cb0[e & 3] : cb1[e & 3])) * mk[it];
        }
        if (in && live) {
            using f16x8s = __attribute__((ext_vector_type(8))) _Float16;
            f16x8s hh, ll;
            range_bad |= (out_of_f16_range(o[0], o[1], o[2], o[3]) || out_of_f16_range(o[4], o[5], o[6], o[7])) && m16[it] != 0.f;
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                _Float16 h, l;
                split_f16(o[e] * m16[it], h, l);
                hh[e] = h;
                ll[e] = l;
            }
            _Float16* o16 = p.out16 + (size_t)(b * T + row) * p.ld16 + (c0g >> 5) * 64 + (c0g & 31);
            store16(reinterpret_cast<f16x8s*>(o16), hh, p.store_wt);
            store16(reinterpret_cast<f16x8s*>(o16 + 32), ll, p.store_wt);
        }
    }
    raise_range_flag(p.range_flag, range_bad);
}

bool conv_gn_supported(int T, int N) { return N == 8 * CONV_GN_CPG && T >= CONV_GN_MIN_ROWS && T <= CONV_GN_MAX_ROWS; }

hipError_t launch_conv_gn(const ConvGnArgs& a, hipStream_t s) {
    // shape contract (the kernel indexes without further checks)
    if (a.B <= 0 || a.B > (1 << 20) || !conv_gn_supported(a.T, a.N)) return hipErrorInvalidValue;
    if (!a.a16_0 || !a.w16 || !a.bias || !a.gamma || !a.beta || !a.mask || !a.out16) return hipErrorInvalidValue;
    if (a.c0 <= 0 || (a.c0 & 31) || (a.c1 & 31) || a.c1 < 0 || (a.a16_1 == nullptr) != (a.c1 == 0)) return hipErrorInvalidValue;
    if (a.lda16_0 < 2 * a.c0 || (a.lda16_0 & 7) || (a.a16_1 && (a.lda16_1 < 2 * a.c1 || (a.lda16_1 & 7)))) return hipErrorInvalidValue;
    if (a.ld16 < 2 * a.N || (a.ld16 & 7)) return hipErrorInvalidValue;
    if ((a.nextra != nullptr) != (a.bias_stats != nullptr)) return hipErrorInvalidValue;
    if (a.chbias_stride < 0 || (a.chbias_stride & 3)) return hipErrorInvalidValue;
    const bool split = a.T <= CONV_GN_SPLIT_ROWS;
    static bool configured[2] = {false, false};
    const void* kern = split ? reinterpret_cast<const void*>(conv_gn_kernel<2>) : reinterpret_cast<const void*>(conv_gn_kernel<1>);
    const int lds_bytes = split ? CgShape<2>::LDS : CgShape<1>::LDS;
    if (!configured[split]) {
        hipError_t e = hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, lds_bytes);
        if (e != hipSuccess) return e;
        configured[split] = true;
    }
    g_kernel_tag = split ? "conv_gn_kernel<2>" : "conv_gn_kernel<1>";
    if (split) hipLaunchKernelGGL(conv_gn_kernel<2>, dim3(8 * a.B), dim3(512), lds_bytes, s, a);
    else hipLaunchKernelGGL(conv_gn_kernel<1>, dim3(8 * a.B), dim3(512), lds_bytes, s, a);
    return hipGetLastError();
}

}  // namespace mtts
