// Device helpers shared by the GEMM kernels (gemm_f32.hip, gemm_p16.hip), attention and the normalisation kernels.
#pragma once
#include <hip/hip_runtime.h>
#include "kernels.h"

namespace mtts {

constexpr float F16_RES_SCALE = 2048.0f;   // fp16 two-term split: the residual is stored times 2^11

// x ~ h + l / 2^11 with h = fp16(x) (saturating) and l the scaled fp16 residual: 22 significand bits
// (the residual is taken from the CLAMPED value: |xc - h| <= ulp(h)/2, so it needs no clamp of its own; a saturated operand is
// reported through the range flag, device_utils.h out_of_f16_range)
__device__ __forceinline__ void split_f16(float x, _Float16& h, _Float16& l) {
    const float xc = __builtin_amdgcn_fmed3f(x, -65504.f, 65504.f);
    h = (_Float16)xc;
    l = (_Float16)((xc - (float)h) * F16_RES_SCALE);
}
__device__ __forceinline__ void split_f16(float x, float lscale, _Float16& h, _Float16& l) {
    const float xc = __builtin_amdgcn_fmed3f(x, -65504.f, 65504.f);
    h = (_Float16)xc;
    l = (_Float16)((xc - (float)h) * lscale);
}

// bfloat16 planes (GemmArgs::bf16): two values -> one packed word (v_cvt_pk_bf16_f32, round to nearest even), and back
using bf16x2_t = __attribute__((ext_vector_type(2))) __bf16;
__device__ __forceinline__ unsigned int pack_bf16(float a, float b) {
    const bf16x2_t v = {(__bf16)a, (__bf16)b};
    return __builtin_bit_cast(unsigned int, v);
}
__device__ __forceinline__ void unpack_bf16(unsigned int w, float& a, float& b) {
    a = __builtin_bit_cast(float, w << 16);
    b = __builtin_bit_cast(float, w & 0xffff0000u);
}

// n / d by a host-made reciprocal (rcp = floor(2^32 / d) + 1; exact while n * d < 2^32).  rcp == 0 (wave-uniform) means "divide":
// d <= 1, or a launch whose quotients could leave that range (the launcher decides, gemm_p16.hip rcp32)
__device__ __forceinline__ int fdiv(int n, int d, unsigned int rcp) { return rcp ? (int)__umulhi((unsigned int)n, rcp) : (d <= 1 ? n : n / d); }

// Range guard of the fp16 split: an operand beyond +-65504 saturates (h clamps), which the caller must learn about.  Producers
// OR their lanes' findings into a register and raise the sticky flag once per thread (atomics only on the rare bad path).
__device__ __forceinline__ bool out_of_f16_range(float a, float b, float c, float d) {
    return fmaxf(fmaxf(fabsf(a), fabsf(b)), fmaxf(fabsf(c), fabsf(d))) > 65504.f;
}
__device__ __forceinline__ void raise_range_flag(unsigned int* flag, bool bad) {
    if (bad && flag) atomicOr(flag, 1u);
}

// 16-byte global store of an output image, in one of two flavours (wt is wave-uniform: Switches::store_wt decides per kernel family).
// Plain: the line stays dirty in the XCD's L2 and is written back behind the kernel's last workgroup, in front of the dependent
// launch.  Write-through (sc1): the bytes leave for memory while the rest of the epilogue runs and the line is DROPPED from this
// L2, so the kernel's end finds nothing to write back -- and a consumer on the same XCD reads it at the cross-XCD rate.  Only whole
// 16-byte stores go this way (an 8-byte sc1 store costs 2.7x the time per byte) and never `nt`.  The asm store is not counted by
// the compiler: it only makes vmcnt larger than the compiler believes, so every wait it writes is stricter than needed.  `s_nop 1`
// ends the string: the instruction behind it may write the data registers, which a 16-byte store reads over several cycles.
// dst: V* in the generic or the global address space, 16-byte aligned.
template <class V, class PTR>
__device__ __forceinline__ void store16(PTR dst, const V& v, bool wt) {
    static_assert(sizeof(V) == 16, "a 16-byte vector");
    using u32x4_s = __attribute__((ext_vector_type(4))) unsigned int;
    if (wt) asm volatile("global_store_dwordx4 %0, %1, off sc1\n\ts_nop 1" ::"v"(dst), "v"(__builtin_bit_cast(u32x4_s, v)) : "memory");
    else *dst = v;
}

// sin(y)^2 for the SnakeBeta epilogue = (1 - cos(2y)) / 2 with the hardware cosine (v_cos_f32 takes revolutions; v_fract_f32
// reduces the argument first): 4 VALU instructions instead of the ~16 of a Cody-Waite reduction with a minimax sine polynomial.
// The FeedForward's first projection spends half of its workgroup lifetime in this epilogue (profiles/r02_kstamp.log).  Absolute
// error of v_cos_f32 ~1e-6, i.e. ~5e-7 on sin^2 (the polynomial: ~1e-7): the mel error against the goldens is unchanged (5.6e-5 /
// 3.4e-5 / 4.1e-5) and the kernel test against fp64 holds its 1e-5.
__device__ __forceinline__ float sin_sq(float y) {
    const float t = __builtin_amdgcn_fractf(y * 0.31830988618379067154f);     // 2y / (2 pi), reduced to [0, 1)
    return fmaf(-0.5f, __builtin_amdgcn_cosf(t), 0.5f);
}
// x + s1 sin(s0 x)^2 with the identity folded in: (x + s1/2) - (s1/2) cos(2 s0 x) -- an add and an FMA behind the cosine instead of
// FMA, multiply, add (the epilogue of the FeedForward's first projection is vector-issue bound: DESIGN.md section 5)
__device__ __forceinline__ float snake_hw(float x, float s0, float s1_half) {
    const float t = __builtin_amdgcn_fractf((x * s0) * 0.31830988618379067154f);
    return __builtin_fmaf(-s1_half, __builtin_amdgcn_cosf(t), x + s1_half);
}

// Mish(x) = x tanh(softplus(x)) = x w / (w + 2), w = e^x (e^x + 2)   (reference decoder.py:32-45, nn.Mish)
// Hardware exponential and reciprocal (v_exp_f32 on x log2 e, v_rcp_f32: ~1 ulp each, relative error of Mish ~3e-7) instead of
// expf and an IEEE division: ~8 instead of ~30 vector instructions per element.  The fused Block1D tail of the ResNet GEMM
// runs this on 16-32 elements per lane with one wave per SIMD (profiles/r02_kstamp_insitu.log: its first 16-row chunk cost
// 8-10k cycles); mel error against the goldens unchanged.
__device__ __forceinline__ float mish_f(float x) {
    if (x > 20.f) return x;
    const float n = __builtin_amdgcn_exp2f(x * 1.44269504088896340736f);
    const float w = n * (n + 2.f);
    return x * (w * __builtin_amdgcn_rcpf(w + 2.f));
}

__device__ __forceinline__ float act_apply(float c, int act, float p0, float p1) {
    switch (act) {
        case ACT_RELU: return c > 0.f ? c : 0.f;
        case ACT_SILU: return c / (1.0f + expf(-c));
        case ACT_SNAKE: {   // reference transformer.py:75: x + 1/(beta+1e-9) * sin(x*alpha)^2
            return c + p1 * sin_sq(c * p0);
        }
        case ACT_GELU: return 0.5f * c * (1.0f + erff(c * 0.70710678118654752440f));   // exact GELU (vocos ConvNeXtBlock)
        default: return c;
    }
}


// DPP all-reduce sums (every lane gets the total): 16-lane rows via row_mirror, row_half_mirror, quad reverse, quad swap;
// 8-lane groups skip the first step.  One VALU instruction per step instead of a ds_bpermute round trip.
#define MTTS_DPP_ADD(v, ctrl) ((v) + __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, (v)), (ctrl), 0xF, 0xF, true)))
__device__ __forceinline__ float allreduce16(float v) {
    v = MTTS_DPP_ADD(v, 0x140);   // row_mirror
    v = MTTS_DPP_ADD(v, 0x141);   // row_half_mirror
    v = MTTS_DPP_ADD(v, 0x1B);    // quad_perm [3,2,1,0]
    v = MTTS_DPP_ADD(v, 0xB1);    // quad_perm [1,0,3,2]
    return v;
}
__device__ __forceinline__ float allreduce8(float v) {
    v = MTTS_DPP_ADD(v, 0x141);
    v = MTTS_DPP_ADD(v, 0x1B);
    v = MTTS_DPP_ADD(v, 0xB1);
    return v;
}

// ---- the ragged-batch contract: the verdict on every row of a batch, by one workgroup.
// Returns the smallest i in [0, B) with refused(i), or B when there is none, to every thread: each thread scans its stride of
// rows keeping its smallest find, then one LDS atomicMin per thread that found one -- no atomics on memory, and the answer does
// not depend on the order the threads arrive in.  Uses blockDim.x threads and one LDS word.
// PRECONDITION: every thread of the workgroup calls it, under a workgroup-uniform condition (it holds two barriers).
template <class Refused>
__device__ __forceinline__ int first_refused_row(int B, Refused refused) {
    __shared__ int first;
    if (threadIdx.x == 0) first = B;
    __syncthreads();
    int mine = B;
    for (int i = B - 1 - (int)threadIdx.x; i >= 0; i -= (int)blockDim.x)
        if (refused(i)) mine = i;
    if (mine < B) atomicMin(&first, mine);
    __syncthreads();
    return first;
}
// a 64-bit length as a 32-bit report word, saturated symmetrically
__device__ __forceinline__ int sat32(int64_t v) { return (int)max(min(v, (int64_t)0x7fffffff), -(int64_t)0x7fffffff); }

}  // namespace mtts
