// The PCM16 quantiser and its dither (include/mtts.h "encoded audio"): what audio_codec.hip and flac.hip both turn a float sample into
// a 16-bit word with, so that a FLAC stream holds exactly the words mtts_pcm_encode writes.
#pragma once

namespace mtts {

__device__ __forceinline__ unsigned int fmix32(unsigned int h) {
    h ^= h >> 16; h *= 0x85EBCA6Bu; h ^= h >> 13; h *= 0xC2B2AE35u; h ^= h >> 16;
    return h;
}
// the row's part of the hash chain: (seed, key)
__device__ __forceinline__ unsigned int dither_row_hash(unsigned int seed_lo, unsigned int seed_hi, int64_t key) {
    unsigned int h = fmix32(0x9E3779B9u ^ seed_lo);
    h = fmix32(h ^ seed_hi);
    h = fmix32(h ^ (unsigned int)((uint64_t)key & 0xFFFFFFFFu));
    return fmix32(h ^ (unsigned int)((uint64_t)key >> 32));
}
// d = u1 - u2 of sample i: exact in fp32 (both are multiples of 2^-24 below 1)
__device__ __forceinline__ float dither_tpdf(unsigned int hrow, unsigned int i) {
    const float u1 = (float)(fmix32(hrow ^ (2u * i)) >> 8) * 0x1p-24f;
    const float u2 = (float)(fmix32(hrow ^ (2u * i + 1u)) >> 8) * 0x1p-24f;
    return u1 - u2;
}
// q of one sample: y already scaled (and dithered)
__device__ __forceinline__ int quantise16(float y) {
    if (y != y) return 0;
    const float r = fminf(fmaxf(rintf(y), -32768.f), 32767.f);
    return (int)r;
}

}  // namespace mtts
