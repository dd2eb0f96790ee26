// Transformer-block chain for the 16-bit storage modes (mtts_set_arithmetic 16 / 17): the one-plane sibling of tblock_chain.hip.
// out-projection + residual -> LayerNorm -> FeedForward (Linear, SnakeBeta, Linear) + residual -> LayerNorm -> the NEXT block's
// q|k|v projection as ONE launch over H16 images (kernels.h ChainH16Args; GemmArgs::half16: one plane, rows of C halves, a 128-byte
// line = 64 channels), fp16 or bfloat16 planes.  It replaces the four tiled gemm_p16 launches (out-projection, FF1 + SnakeBeta, FF2,
// q|k|v) a transformer block takes in those modes, with their 2-byte image round trips through HBM.
//
// Same idea and phase structure as tblock_chain.hip (read its header first): a workgroup (8 waves) owns QB rows for the whole chain,
// the residual-stream tile and one hidden chunk live in LDS, the weights stream from L2 into a register ring as 1 KiB lane-major
// fragments in consumption order, products are computed transposed (A = weight fragment, B = activation fragment) so a lane holds 4
// consecutive channels of one row.  What differs:
//   * ONE MFMA per MAC (v_mfma_f32_16x16x32_f16 / _bf16), one accumulator set, fp32 accumulation; LayerNorm moments and SnakeBeta in
//     fp32; every value that crosses a phase is rounded once to the 16-bit type (as the tiled H16 launches round their images).
//   * the stream has one plane: 2 bytes per weight, a k-step of a C-wide product consumes NT = C/128 fragments per wave (FF1: CH/128)
//     instead of twice that.  The ring arithmetic below is derived for that, not copied.
//   * LDS images are H16: per 64-channel group a [QB][128 B] block, 16-byte chunk j of a row = channels 8j..8j+7 of the group, stored
//     at chunk j ^ ((row >> 1) & 7).  k-step s (32 channels) reads group s >> 1, chunks 4 (s & 1) + q.  A 128-byte line of the
//     attention image holds TWO k-steps, so the out-projection advances by "line steps" of two k-steps.
//   * rows per workgroup up to 96 (LDS: x tile QB C 2 + hidden chunk QB CH 2 + 18 C 4 bytes = 109 KB at QB 64, 150 KB at QB 96 for
//     C = 384, CH = 256): staging takes ceil(QB / 64) passes of 64 rows.
//   * no pair form.
// bfloat16 planes: round to nearest even in the producers (v_cvt_pk_bf16_f32), fp32 exponent range, no range guard.  fp16 planes:
// producers clamp to +-65504 and raise the sticky range flag.
#include "kernels.h"
#include "device_utils.h"
#include <cstring>
#include <string>
#include <algorithm>
#include <cmath>

namespace mtts {

using f32x4 = __attribute__((ext_vector_type(4))) float;
using f16x8 = __attribute__((ext_vector_type(8))) _Float16;
using f16x2 = __attribute__((ext_vector_type(2))) _Float16;
using bf16x8 = __attribute__((ext_vector_type(8))) __bf16;
using u32x2 = __attribute__((ext_vector_type(2))) unsigned int;
using u32x4 = __attribute__((ext_vector_type(4))) unsigned int;

constexpr int H16_NW = CHAIN_WAVES;          // waves per workgroup

// Ring depth in fragments.  A line step of the out-projection consumes 2 NT fragments and the attention rows are double-buffered
// in registers over an unrolled ring period, so a period is an EVEN number of line steps: R = 4 NT (two line steps; 12 KiB per wave
// in flight at C = 384, what a ~2k-cycle L2 round trip needs at the CU's ingest rate).
static constexpr int h16_ring(int C) { return 4 * (C / 128); }

template <int C, int QB, int CH>
struct ChainH16Cfg {
    static constexpr int NT = C / (16 * H16_NW);         // 16-channel tiles of the C-wide outputs per wave = fragments per k-step
    static constexpr int NT1 = CH / (16 * H16_NW);       // ... of a hidden chunk per wave = fragments per FF1 k-step
    static constexpr int MT = QB / 16;                   // 16-row tiles
    static constexpr int KG = C / 32, KG2 = CH / 32;     // k-steps over the stream width / over a hidden chunk
    static constexpr int NCH = 4 * C / CH;               // hidden chunks
    static constexpr int SP = (QB + 63) / 64;            // staging passes (8 lanes per 128-byte line, 64 rows per pass)
    static constexpr int R = h16_ring(C);
    static constexpr int XT_BYTES = QB * C * 2, HT_BYTES = QB * CH * 2;
    static constexpr int CT_FLOATS = 18 * C;             // column constants: wsum1 | b1 | p0 | p1/2 (4C each) | b_out | b2 (C each)
    static constexpr int LDS_BYTES = XT_BYTES + HT_BYTES + 2 * QB * 4 + CT_FLOATS * 4;
    static_assert(C % 128 == 0 && CH % 128 == 0 && QB % 16 == 0 && QB <= 128, "shape");
    static_assert(R % NT == 0 && R % NT1 == 0, "a ring period is a whole number of k-steps");
    static_assert((KG * NT1 + KG2 * NT) % R == 0 && (KG * NT) % R == 0, "phases start on ring slot 0");
    static_assert(R % (2 * NT) == 0 && ((R / (2 * NT)) & 1) == 0, "out-projection: even number of line steps per ring period");
    static_assert(HT_BYTES >= 2 * QB * 128, "two attention line stages in the hidden-chunk area");
};

// ------------------------------------------------------------------------------------------------ host: fragment streams
// Per wave: [out-projection: inner/32 k-steps x NT tiles][per hidden chunk: C/32 k-steps x NT1 tiles (FF1), CH/32 k-steps x NT tiles
// (FF2)][q|k|v: passes x C/32 k-steps x NT tiles][R padding fragments]; a tile = ONE fragment [64 lanes][8 values] of 2 bytes.
static int h16_qkv_passes(int C, int n_qkv) {
    const int per_pass = H16_NW * (C / 128);
    return n_qkv > 0 ? ((n_qkv / 16) + per_pass - 1) / per_pass : 0;
}
bool chain_h16_supported(int C, int inner, int ch, int n_qkv) {
    if (C != 128 && C != 256 && C != 384) return false;
    if (ch != 128 && !(ch == 256 && C == 384)) return false;
    if (inner < 0 || (inner % 128) || inner > C) return false;      // whole ring periods of line steps (two 64-channel lines)
    if (n_qkv < 0 || (n_qkv && ((n_qkv % 32) || !inner))) return false;
    return true;
}
long chain_h16_stream_frags(int C, int inner, int ch, int n_qkv) {
    const int NT = C / 128, NT1 = ch / 128;
    long f = (long)(inner / 32) * NT;
    f += (long)(4 * C / ch) * ((C / 32) * NT1 + (ch / 32) * NT);
    f += (long)h16_qkv_passes(C, n_qkv) * (C / 32) * NT;
    return f + h16_ring(C);
}
static uint16_t h16_round(float x, bool bf16, bool* sat) {
    uint16_t u;
    if (bf16) {
        const __bf16 h = (__bf16)x;                       // round to nearest even, like panel_bf16_host
        std::memcpy(&u, &h, 2);
    } else {
        if (std::fabs(x) > 65504.f && sat) *sat = true;
        const _Float16 h = (_Float16)(x < -65504.f ? -65504.f : (x > 65504.f ? 65504.f : x));
        std::memcpy(&u, &h, 2);
    }
    return u;
}
static void put_frag_h16(uint16_t* dst, const float* w, int ldw, int n0, int n_valid, int k0, bool bf16, bool* sat) {
    // dst: [64 lanes][8]; lane (r = lane & 15, q = lane >> 4) holds row n0 + r, k = k0 + 8 q .. + 7
    for (int lane = 0; lane < 64; ++lane)
        for (int j = 0; j < 8; ++j) {
            const int n = n0 + (lane & 15), k = k0 + 8 * (lane >> 4) + j;
            dst[lane * 8 + j] = h16_round(n < n_valid ? w[(size_t)n * ldw + k] : 0.f, bf16, sat);
        }
}
void chain_h16_stream_pack(int C, int inner, int ch, int n_qkv, const float* w_out, const float* w1, const float* w2, const float* w_qkv,
                           bool bf16, uint16_t* dst, bool* saturates) {
    const int NT = C / 128, NT1 = ch / 128, KG = C / 32, KG2 = ch / 32, NCH = 4 * C / ch;
    const long per_wave = chain_h16_stream_frags(C, inner, ch, n_qkv);
    const int passes = h16_qkv_passes(C, n_qkv);
    for (int w = 0; w < H16_NW; ++w) {
        uint16_t* o = dst + (size_t)w * per_wave * 512;
        if (inner && w_out)
            for (int s = 0; s < inner / 32; ++s)
                for (int t = 0; t < NT; ++t, o += 512) put_frag_h16(o, w_out, inner, 16 * (w * NT + t), C, 32 * s, bf16, saturates);
        for (int j = 0; j < NCH; ++j) {
            for (int s = 0; s < KG; ++s)
                for (int t = 0; t < NT1; ++t, o += 512) put_frag_h16(o, w1, C, j * ch + 16 * (w * NT1 + t), 4 * C, 32 * s, bf16, saturates);
            for (int s = 0; s < KG2; ++s)
                for (int t = 0; t < NT; ++t, o += 512) put_frag_h16(o, w2, 4 * C, 16 * (w * NT + t), C, j * ch + 32 * s, bf16, saturates);
        }
        for (int ps = 0; ps < passes; ++ps)
            for (int s = 0; s < KG; ++s)
                for (int t = 0; t < NT; ++t, o += 512)
                    put_frag_h16(o, w_qkv, C, 16 * (ps * H16_NW * NT + w * NT + t), n_qkv, 32 * s, bf16, saturates);
        std::memset(o, 0, (size_t)h16_ring(C) * 512 * sizeof(uint16_t));
    }
}

// ------------------------------------------------------------------------------------------------ device
template <bool BF>
__device__ __forceinline__ f32x4 mfma_h16(u32x4 a, u32x4 b, f32x4 c) {
    if constexpr (BF) return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
    else return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
}
// one packed word of two 16-bit values -> fp32
template <bool BF>
__device__ __forceinline__ void unpack2(unsigned int w, float& a, float& b) {
    if constexpr (BF) unpack_bf16(w, a, b);
    else { const f16x2 h = __builtin_bit_cast(f16x2, w); a = (float)h[0]; b = (float)h[1]; }
}
// 4 consecutive channels -> two packed words.  fp16: clamped to the finite range, |v| tracked for the range flag
template <bool BF>
__device__ __forceinline__ u32x2 pack4(const f32x4 v, float& rmax) {
    u32x2 w;
#pragma unroll
    for (int e = 0; e < 2; ++e) {
        const float x0 = v[2 * e], x1 = v[2 * e + 1];
        if constexpr (BF) w[e] = pack_bf16(x0, x1);
        else {
            asm("v_max3_f32 %0, |%1|, |%2|, %0" : "+v"(rmax) : "v"(x0), "v"(x1));
            const f16x2 hp = {(_Float16)__builtin_amdgcn_fmed3f(x0, -65504.f, 65504.f), (_Float16)__builtin_amdgcn_fmed3f(x1, -65504.f, 65504.f)};
            w[e] = __builtin_bit_cast(unsigned int, hp);
        }
    }
    return w;
}

// The ring's loads are inline asm with hand-written waits (tblock_chain.hip explains why): a load is complete once at most N
// vector-memory operations YOUNGER than it are outstanding, N = the number of younger loads issued by this file's asm.  The registers
// a wait covers pass through an empty asm right behind it (H16_TIE) so their consumers cannot be scheduled above the wait.
#define H16_LOAD(dst, voff, sbase) asm volatile("global_load_dwordx4 %0, %1, %2" : "=&v"(dst) : "v"(voff), "s"(sbase))
#define H16_WAIT(n) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(n))
#define H16_TIE(x) asm volatile("" : "+v"(x))

template <int C, int QB, int CH, bool BF>
__global__ __launch_bounds__(64 * H16_NW, 1) void tblock_h16_kernel(const ChainH16Args p) {
    using K = ChainH16Cfg<C, QB, CH>;
    constexpr int NT = K::NT, NT1 = K::NT1, MT = K::MT, KG = K::KG, KG2 = K::KG2, R = K::R, SP = K::SP;
    extern __shared__ __attribute__((aligned(16))) char lds[];      // x tile | hidden chunk / attention line stages | row statistics | constants
    char* const XT = lds;
    char* const HT = lds + K::XT_BYTES;
    float* const srow = reinterpret_cast<float*>(lds + K::XT_BYTES + K::HT_BYTES);
    float* const CT = srow + 2 * QB;

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int c = lane & 15, q = lane >> 4, swz = (c >> 1) & 7;     // fragment coordinates: row / channel c, k block q
    const int wg = (int)blockIdx.x - p.pf_wgs;                      // the first pf_wgs workgroups only prefetch
    const int M = p.M, m0 = wg * QB;
    const bool has_out = p.inner > 0, has_qkv = p.b_qkv != nullptr;
    const unsigned int lane16 = lane * 16;
    // ---- prefetch workgroups (lowest ids: dispatched first, round-robin over the XCDs): touch the stream just ahead of the computing
    // workgroups so that their loads hit the L2 (tblock_chain.hip).  No output depends on them.
    if (wg < 0) {
        const long bytes = (long)p.stream_frags * 1024;
        unsigned int sink = 0;
        const int pfid = p.pf_wgs + wg;
        const char* base = reinterpret_cast<const char*>(p.wstream) + (size_t)wave * (size_t)p.stream_frags * 1024;
        const int parts = (p.pf_wgs + 7) / 8;
        for (long off = (long)(pfid >> 3) * 8192; off < bytes; off += 8192L * parts) {
            const long o = off + lane * 128;                        // (several prefetch workgroups per XCD interleave their 8 KiB pieces)
            const unsigned int ob = (unsigned int)(o < bytes ? o : bytes - 128);
            asm volatile("global_load_dword %0, %1, %2" : "+v"(sink) : "v"(ob), "s"(base));
            asm volatile("s_waitcnt vmcnt(8)");
        }
        asm volatile("s_waitcnt vmcnt(0)");
        asm volatile("" : "+v"(sink));
        return;
    }

    // ---- the wave's weight stream through a register ring: fragment f of the current position sits in ring[f % R]
    const char* wpos = reinterpret_cast<const char*>(p.wstream) + (size_t)wave * (size_t)p.stream_frags * 1024;
    u32x4 ring[R];
#pragma unroll
    for (int i = 0; i < R; ++i) H16_LOAD(ring[i], lane16, wpos + i * 1024);
    auto refill = [&](int slot, int frag) __attribute__((always_inline)) {
        H16_LOAD(ring[slot % R], lane16, wpos + (frag + R) * 1024);
    };

    // ---- staging coordinates (8 lanes per 128-byte line): thread -> rows (tid >> 3) + 64 pass, 16-byte chunk tid & 7
    const int st_row = tid >> 3, st_chunk = tid & 7;
    const int st_lds = st_row * 128 + ((st_chunk ^ ((st_row >> 1) & 7)) * 16);      // (+ 64 rows: the same swizzle)
    bool st_on[SP];
    size_t st_grow[SP];
    unsigned int att_off[SP];
#pragma unroll
    for (int ps = 0; ps < SP; ++ps) {
        st_on[ps] = st_row + 64 * ps < QB;
        st_grow[ps] = (size_t)min(m0 + st_row + 64 * ps, M - 1);
        att_off[ps] = (unsigned int)((st_grow[ps] * p.ld_att + st_chunk * 8) * 2);
    }
    u32x4 areg[2][SP];
    if (has_out) {
#pragma unroll
        for (int ps = 0; ps < SP; ++ps) H16_LOAD(areg[0][ps], att_off[ps], reinterpret_cast<const char*>(p.att16));
#pragma unroll
        for (int ps = 0; ps < SP; ++ps) H16_LOAD(areg[1][ps], att_off[ps], reinterpret_cast<const char*>(p.att16) + (p.inner > 64 ? 128 : 0));
    }
    // residual stream tile and column constants -> LDS; every load is requested before the first LDS write (one round trip)
    {
        u32x4 xv[SP][C / 64];
#pragma unroll
        for (int ps = 0; ps < SP; ++ps) {
            const unsigned short* src = reinterpret_cast<const unsigned short*>(p.x16) + st_grow[ps] * p.ld_x + st_chunk * 8;
#pragma unroll
            for (int g0 = 0; g0 < C / 64; ++g0) xv[ps][g0] = *reinterpret_cast<const u32x4*>(src + g0 * 64);
        }
        constexpr int NCT = (K::CT_FLOATS / 4 + 64 * H16_NW - 1) / (64 * H16_NW);      // f32x4 per thread
        f32x4 cv[NCT];
#pragma unroll
        for (int n = 0; n < NCT; ++n) {
            const int idx = (tid + n * 64 * H16_NW) * 4;
            cv[n] = *reinterpret_cast<const f32x4*>(p.consts + min(idx, K::CT_FLOATS - 4));
            cv[n] *= (idx >= 12 * C && idx < 16 * C) ? 0.5f : 1.0f;            // SnakeBeta: 1 / (2 (exp(beta) + 1e-9))
        }
#pragma unroll
        for (int ps = 0; ps < SP; ++ps)
            if (st_on[ps]) {
#pragma unroll
                for (int g0 = 0; g0 < C / 64; ++g0) *reinterpret_cast<u32x4*>(XT + g0 * (QB * 128) + 64 * 128 * ps + st_lds) = xv[ps][g0];
            }
#pragma unroll
        for (int n = 0; n < NCT; ++n) {
            const int idx = (tid + n * 64 * H16_NW) * 4;
            if (idx < K::CT_FLOATS) *reinterpret_cast<f32x4*>(CT + idx) = cv[n];
        }
    }
    H16_WAIT(0);
#pragma unroll
    for (int i = 0; i < R; ++i) H16_TIE(ring[i]);
    if (has_out) {
#pragma unroll
        for (int ps = 0; ps < SP; ++ps) { H16_TIE(areg[0][ps]); H16_TIE(areg[1][ps]); }
    }

    // activation fragment (B operand): rows 16 i + c of k-step s of an image at `base`
    auto bfrag = [&](const char* base, int s, int i) -> u32x4 {
        return *reinterpret_cast<const u32x4*>(base + (s >> 1) * (QB * 128) + (16 * i + c) * 128 + ((((s & 1) * 4 + q) ^ swz) * 16));
    };
    // position of this lane's 4 consecutive channels ch..ch+3 of row 16 i + c inside an image (8 bytes)
    auto img_off = [&](int ch, int i) -> int {
        const int off = ch & 63;
        return (ch >> 6) * (QB * 128) + (16 * i + c) * 128 + (((off >> 3) ^ swz) * 16) + (off & 7) * 2;
    };

    f32x4 acc[NT][MT];
    auto zero_acc = [&]() {
#pragma unroll
        for (int t = 0; t < NT; ++t)
#pragma unroll
            for (int i = 0; i < MT; ++i) acc[t][i] = f32x4{0.f, 0.f, 0.f, 0.f};
    };
    // one k-step of a C-wide product: its NT weight fragments (ring slots fb ..) times the activation fragments of k-step s of
    // `base`, then the fragments R further on are requested into the same slots.  The wait, by what else this file has requested
    // since (mode): 0 the R - NT younger fragments of the ring; 1 first k-step of an out-projection line step (see phase 0);
    // 2 none (the second k-step of a line step: its fragments are older than what mode 1 waited for).
    auto step_wide = [&](int fb, const char* base, int s, int frag, int mode) __attribute__((always_inline)) {
        if (mode == 1) H16_WAIT(2 * NT + SP);
        else if (mode == 0) H16_WAIT(R - NT);
#pragma unroll
        for (int f = 0; f < NT; ++f) H16_TIE(ring[(fb + f) % R]);
#pragma unroll
        for (int i = 0; i < MT; ++i) {
            const u32x4 b = bfrag(base, s, i);
#pragma unroll
            for (int t = 0; t < NT; ++t) acc[t][i] = mfma_h16<BF>(ring[(fb + t) % R], b, acc[t][i]);
        }
#pragma unroll
        for (int t = 0; t < NT; ++t) refill(fb + t, frag + t);
    };
    // End of every k-loop: nothing this file requested may be in flight when compiler-scheduled code follows (the compiler treats an
    // asm output as available at once and may copy a ring register before its load has landed: DESIGN.md section 5).
    auto ring_drain = [&]() __attribute__((always_inline)) {
        H16_WAIT(0);
#pragma unroll
        for (int i = 0; i < R; ++i) H16_TIE(ring[i]);
    };
    float rmax = 0.f;
    // acc (+ bias + the residual rows in XT) -> XT, in place: this lane's channels 16 (wave NT + t) + 4 q .. + 3 of rows 16 i + c
    auto rows_to_xt = [&](const float* bias) {
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            const int ch = 16 * (wave * NT + t) + 4 * q;
            const f32x4 b4 = *reinterpret_cast<const f32x4*>(bias + ch);
#pragma unroll
            for (int i = 0; i < MT; ++i) {
                char* px = XT + img_off(ch, i);
                const u32x2 rw = *reinterpret_cast<const u32x2*>(px);
                float r[4];
                f32x4 v;
                unpack2<BF>(rw[0], r[0], r[1]);
                unpack2<BF>(rw[1], r[2], r[3]);
#pragma unroll
                for (int e = 0; e < 4; ++e) v[e] = (acc[t][i][e] + b4[e]) + r[e];
                *reinterpret_cast<u32x2*>(px) = pack4<BF>(v, rmax);
            }
        }
    };
    // LayerNorm moments of the rows in XT -> srow = [mean x QB | rstd x QB].  A wave takes QB/8 rows, 8 lanes per row (each C/64
    // 8-channel chunks of it), 8 rows per round: two passes over values held in registers, reductions over 8 lanes by DPP.
    auto ln_stats = [&]() {
        constexpr int RPW = QB / H16_NW, CPL = C / 64;
#pragma unroll
        for (int r0 = 0; r0 < RPW; r0 += 8) {
            const int rl = r0 + (lane >> 3), part = lane & 7;
            const bool on = rl < RPW;
            const int row = wave * RPW + (on ? rl : 0), rs = (row >> 1) & 7;
            float x[CPL][8];
            float s = 0.f;
#pragma unroll
            for (int k = 0; k < CPL; ++k) {
                const int ck = part * CPL + k;            // 8-channel chunk of the row: group ck >> 3, chunk ck & 7
                const u32x4 w = *reinterpret_cast<const u32x4*>(XT + (ck >> 3) * (QB * 128) + row * 128 + (((ck & 7) ^ rs) * 16));
#pragma unroll
                for (int e = 0; e < 4; ++e) unpack2<BF>(w[e], x[k][2 * e], x[k][2 * e + 1]);
                s += ((x[k][0] + x[k][1]) + (x[k][2] + x[k][3])) + ((x[k][4] + x[k][5]) + (x[k][6] + x[k][7]));
            }
            const float mean = allreduce8(s) * (1.0f / C);
            float m2 = 0.f;
#pragma unroll
            for (int k = 0; k < CPL; ++k)
#pragma unroll
                for (int e = 0; e < 8; ++e) { const float d = x[k][e] - mean; m2 += d * d; }
            m2 = allreduce8(m2);
            if (on && part == 0) {
                srow[row] = mean;
                srow[QB + row] = 1.0f / sqrtf(m2 * (1.0f / C) + p.eps);
            }
        }
    };

    // ================================================================ phase 0: out-projection + residual (reference transformer.py:261)
    if (has_out) {
        constexpr int PER0 = R / (2 * NT);               // line steps per ring period (even)
        constexpr int NS = K::HT_BYTES / (QB * 128);     // attention line stages in HT
        const int nl0 = p.inner >> 6;                    // 128-byte lines of an attention row = line steps (two k-steps each)
#pragma unroll
        for (int ps = 0; ps < SP; ++ps)
            if (st_on[ps]) *reinterpret_cast<u32x4*>(HT + 64 * 128 * ps + st_lds) = areg[0][ps];
        zero_acc();
        __syncthreads();
        for (int s0 = 0; s0 < nl0; s0 += PER0) {
#pragma unroll
            for (int u = 0; u < PER0; ++u) {
                const int s = s0 + u;
                // line s+2 into the registers that held line s (in LDS since the previous step).  Queue, oldest first:
                // ... ATT(s+1) (SP loads) | refills of line step s-1 (2 NT) | ATT(s+2) (SP): this step's 2 NT fragments were refilled
                // two line steps ago, i.e. they are older than ATT(s+1), so one wait for ATT(s+1) -- 2 NT + SP younger loads --
                // covers both k-steps.
#pragma unroll
                for (int ps = 0; ps < SP; ++ps)
                    H16_LOAD(areg[u & 1][ps], att_off[ps], reinterpret_cast<const char*>(p.att16) + min(s + 2, nl0 - 1) * 128);
                const char* stage = HT + (s % NS) * (QB * 128);
                step_wide((u * 2 * NT) % R, stage, 0, u * 2 * NT, 1);
                step_wide((u * 2 * NT + NT) % R, stage, 1, u * 2 * NT + NT, 2);
#pragma unroll
                for (int ps = 0; ps < SP; ++ps) {
                    H16_TIE(areg[(u + 1) & 1][ps]);
                    if (st_on[ps] && s + 1 < nl0) *reinterpret_cast<u32x4*>(HT + ((s + 1) % NS) * (QB * 128) + 64 * 128 * ps + st_lds) = areg[(u + 1) & 1][ps];
                }
                __syncthreads();
            }
            wpos += R * 1024;
        }
        ring_drain();
#pragma unroll
        for (int ps = 0; ps < SP; ++ps) { H16_TIE(areg[0][ps]); H16_TIE(areg[1][ps]); }
        rows_to_xt(CT + 16 * C);
        __syncthreads();
    } else {
        __syncthreads();                                  // the x tile is in LDS
    }
    ln_stats();
    __syncthreads();

    // ================================================================ phase 1: FeedForward (reference transformer.py:278-301,104-120)
    zero_acc();
    {
        constexpr int F1 = KG * NT1;                      // fragments of a chunk's FF1 part
        for (int j = 0; j < K::NCH; ++j) {
            f32x4 a1[NT1][MT];
#pragma unroll
            for (int t = 0; t < NT1; ++t)
#pragma unroll
                for (int i = 0; i < MT; ++i) a1[t][i] = f32x4{0.f, 0.f, 0.f, 0.f};
            // ---- FF1: hidden chunk^T = W1'[chunk] . x^T
#pragma unroll
            for (int s = 0; s < KG; ++s) {
                const int fb = (s * NT1) % R;
                H16_WAIT(R - NT1);
#pragma unroll
                for (int f = 0; f < NT1; ++f) H16_TIE(ring[(fb + f) % R]);
#pragma unroll
                for (int i = 0; i < MT; ++i) {
                    const u32x4 b = bfrag(XT, s, i);
#pragma unroll
                    for (int t = 0; t < NT1; ++t) a1[t][i] = mfma_h16<BF>(ring[(fb + t) % R], b, a1[t][i]);
                }
#pragma unroll
                for (int t = 0; t < NT1; ++t) refill(fb + t, s * NT1 + t);
            }
            ring_drain();
            // ---- LayerNorm after the product, SnakeBeta, one rounding -> hidden chunk image in HT
            float nmr[MT], rstd[MT];                      // this lane's rows: -mean rstd, rstd
#pragma unroll
            for (int i = 0; i < MT; ++i) { rstd[i] = srow[QB + 16 * i + c]; nmr[i] = -(srow[16 * i + c] * rstd[i]); }
#pragma unroll
            for (int t = 0; t < NT1; ++t) {
                const int hl = 16 * (wave * NT1 + t) + 4 * q;          // channel inside the chunk
                const float* cc = CT + j * CH + hl;
                const f32x4 cw = *reinterpret_cast<const f32x4*>(cc), cb = *reinterpret_cast<const f32x4*>(cc + 4 * C),
                            cs0 = *reinterpret_cast<const f32x4*>(cc + 8 * C), cs1h = *reinterpret_cast<const f32x4*>(cc + 12 * C);
#pragma unroll
                for (int i = 0; i < MT; ++i) {
                    f32x4 v;
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const float z = __builtin_fmaf(a1[t][i][e], rstd[i], __builtin_fmaf(nmr[i], cw[e], cb[e]));
                        v[e] = snake_hw(z, cs0[e], cs1h[e]);
                    }
                    *reinterpret_cast<u32x2*>(HT + img_off(hl, i)) = pack4<BF>(v, rmax);
                }
            }
            __syncthreads();
            // ---- FF2: out^T += W2[:, chunk] . hidden chunk^T
#pragma unroll
            for (int s = 0; s < KG2; ++s) step_wide((F1 + s * NT) % R, HT, s, F1 + s * NT, 0);
            ring_drain();
            wpos += (F1 + KG2 * NT) * 1024;
            __syncthreads();                              // the hidden chunk may be overwritten
        }
    }
    rows_to_xt(CT + 17 * C);
    __syncthreads();

    // ---- the block's output rows: LDS image -> global image, whole 16-byte chunks, coalesced
    {
        constexpr int CPR = C / 8;                        // 16-byte chunks per row
        for (int idx = tid; idx < QB * CPR; idx += 64 * H16_NW) {
            const int row = idx / CPR, cc = idx - row * CPR;
            if (m0 + row < M) {
                u32x4 v = *reinterpret_cast<const u32x4*>(XT + (cc >> 3) * (QB * 128) + row * 128 + (((cc & 7) ^ ((row >> 1) & 7)) * 16));
                if (p.x_out_mask && p.x_out_mask[m0 + row] == 0.f) v = u32x4{0u, 0u, 0u, 0u};
                *reinterpret_cast<u32x4*>(reinterpret_cast<unsigned short*>(p.x_out) + (size_t)(m0 + row) * p.ld_out + cc * 8) = v;
            }
        }
    }

    // ================================================================ phase 2: the next block's q|k|v (reference transformer.py:249-258)
    if (has_qkv) {
        ln_stats();
        float* const QC = reinterpret_cast<float*>(HT);   // the hidden-chunk area is free: panel row sums | bias of the q|k|v columns
        for (int idx = tid * 4; idx < 2 * p.n_qkv; idx += 4 * 64 * H16_NW)
            *reinterpret_cast<f32x4*>(QC + idx) = *reinterpret_cast<const f32x4*>(idx < p.n_qkv ? p.wsum_qkv + idx : p.b_qkv + (idx - p.n_qkv));
        __syncthreads();
        const int ntiles = p.n_qkv >> 4;
        const int passes = (ntiles + H16_NW * NT - 1) / (H16_NW * NT);
        const bool all_stores = m0 + QB <= M;             // (uniform) no row of the tile is past the end
        for (int ps = 0; ps < passes; ++ps) {
            zero_acc();
#pragma unroll
            for (int s = 0; s < KG; ++s) step_wide((s * NT) % R, XT, s, s * NT, 0);
            ring_drain();
            wpos += KG * NT * 1024;
            float nmr[MT], rstd[MT];
#pragma unroll
            for (int i = 0; i < MT; ++i) { rstd[i] = srow[QB + 16 * i + c]; nmr[i] = -(srow[16 * i + c] * rstd[i]); }
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                const int tile = ps * H16_NW * NT + wave * NT + t;
                if (tile < ntiles) {
                    const int col = 16 * tile + 4 * q;
                    const f32x4 w4 = *reinterpret_cast<const f32x4*>(QC + col), b4 = *reinterpret_cast<const f32x4*>(QC + p.n_qkv + col);
#pragma unroll
                    for (int i = 0; i < MT; ++i) {
                        const int row = m0 + 16 * i + c;
                        f32x4 v;
#pragma unroll
                        for (int e = 0; e < 4; ++e) v[e] = __builtin_fmaf(acc[t][i][e], rstd[i], __builtin_fmaf(nmr[i], w4[e], b4[e]));
                        const u32x2 w = pack4<BF>(v, rmax);
                        if (all_stores || row < M)
                            *reinterpret_cast<u32x2*>(reinterpret_cast<unsigned short*>(p.qkv16) + (size_t)row * p.ld_qkv + col) = w;
                    }
                }
            }
        }
    }
    if constexpr (!BF) raise_range_flag(p.range_flag, rmax > 65504.f);
}

// H16 image -> fp32 rows (the unit entry's decoder; 8 values per thread)
__global__ void from_h16_kernel(const unsigned int* __restrict__ x, int ld16, int M, int C, bool bf16, float* __restrict__ out, int ld) {
    const long n = (long)M * (C / 2);
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
        const long row = i / (C / 2);
        const int cw = (int)(i - row * (C / 2));
        const unsigned int w = x[row * (ld16 / 2) + cw];
        float a, b;
        if (bf16) unpack2<true>(w, a, b);
        else unpack2<false>(w, a, b);
        out[row * ld + 2 * cw] = a;
        out[row * ld + 2 * cw + 1] = b;
    }
}
hipError_t launch_from_h16(const void* x, int ld16, int M, int C, bool bf16, float* out, int ld, hipStream_t s) {
    if (M <= 0 || (C & 1) || (ld16 & 1)) return hipErrorInvalidValue;
    const long n = (long)M * (C / 2);
    hipLaunchKernelGGL(from_h16_kernel, dim3((unsigned)std::min<long>((n + 255) / 256, 4096)), dim3(256), 0, s, static_cast<const unsigned int*>(x), ld16, M, C, bf16, out, ld);
    return hipGetLastError();
}

template <int C, int QB, int CH, bool BF>
static hipError_t launch_h16_shape(const ChainH16Args& a, hipStream_t s) {
    using K = ChainH16Cfg<C, QB, CH>;
    static_assert(K::LDS_BYTES <= 160 * 1024, "LDS per workgroup");
    auto kern = tblock_h16_kernel<C, QB, CH, BF>;
    // per call: the attribute belongs to the function ON THE CURRENT DEVICE (a process may drive several)
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, K::LDS_BYTES);
    if (e != hipSuccess) return e;
    static const std::string tag = "tblock_h16_kernel<" + std::to_string(C) + ", " + std::to_string(QB) + ", " + std::to_string(CH) + ", " + tf(BF) + ">";
    g_kernel_tag = tag.c_str();
    if (a.n_qkv * 8 > K::HT_BYTES) return hipErrorInvalidValue;      // the q|k|v column constants live in the hidden-chunk area
    const int tiles = (a.M + QB - 1) / QB;
    hipLaunchKernelGGL(kern, dim3(tiles + a.pf_wgs), dim3(64 * H16_NW), K::LDS_BYTES, s, a);
    return hipGetLastError();
}
template <int C, int QB, int CH>
static hipError_t launch_h16_dtype(const ChainH16Args& a, hipStream_t s) {
    return a.bf16 ? launch_h16_shape<C, QB, CH, true>(a, s) : launch_h16_shape<C, QB, CH, false>(a, s);
}

hipError_t launch_tblock_chain_h16(const ChainH16Args& a, hipStream_t s) {
    if (a.pair != 0) return hipErrorInvalidValue;         // no pair form for one-plane operands
    if (a.pf_wgs < 0 || a.pf_wgs > 64) return hipErrorInvalidValue;
    if (a.M <= 0 || !a.x16 || !a.wstream || !a.x_out || !a.consts) return hipErrorInvalidValue;
    if (!chain_h16_supported(a.C, a.inner, a.ch, a.b_qkv ? a.n_qkv : 0)) return hipErrorInvalidValue;
    if (a.inner && (!a.att16 || a.ld_att < a.inner || (a.ld_att & 7))) return hipErrorInvalidValue;
    if (a.b_qkv && (!a.wsum_qkv || !a.qkv16 || a.n_qkv <= 0 || a.ld_qkv < a.n_qkv || (a.ld_qkv & 3))) return hipErrorInvalidValue;
    if (a.ld_x < a.C || (a.ld_x & 7) || a.ld_out < a.C || (a.ld_out & 7)) return hipErrorInvalidValue;
    if (a.stream_frags != chain_h16_stream_frags(a.C, a.inner, a.ch, a.b_qkv ? a.n_qkv : 0)) return hipErrorInvalidValue;
    if (a.C == 384 && a.ch == 256) {
        if (a.qb == 96) return launch_h16_dtype<384, 96, 256>(a, s);
        if (a.qb == 64) return launch_h16_dtype<384, 64, 256>(a, s);
        if (a.qb == 32) return launch_h16_dtype<384, 32, 256>(a, s);
    } else if (a.C == 384 && a.ch == 128) {
        if (a.qb == 64) return launch_h16_dtype<384, 64, 128>(a, s);
    } else if (a.C == 256 && a.ch == 128) {
        if (a.qb == 64) return launch_h16_dtype<256, 64, 128>(a, s);
        if (a.qb == 32) return launch_h16_dtype<256, 32, 128>(a, s);
    } else if (a.C == 128 && a.ch == 128) {
        if (a.qb == 64) return launch_h16_dtype<128, 64, 128>(a, s);
        if (a.qb == 32) return launch_h16_dtype<128, 32, 128>(a, s);
    }
    return hipErrorInvalidValue;
}

}  // namespace mtts
