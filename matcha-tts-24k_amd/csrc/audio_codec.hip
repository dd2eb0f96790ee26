// Encoded audio (gfx950): a ragged batch of fp32 rows to PCM16 / G.711 bytes and back, one launch each, per-row formats.
//
// The arithmetic is include/mtts.h "encoded audio", restated in tests/audio_codec_restated.py: q = clamp(rint(x * 32768 [+ d])),
// G.711 companding of the undithered q in integer operations (no table), TPDF dither from a counter-based hash of (seed, key,
// sample index, stream).  Nothing here depends on the row index, the grid or the batch.
//
// Both kernels: grid (tile, row), 256 threads, CODEC_TILE samples per workgroup; a lane owns the groups of 4 consecutive samples
// l, l + 256, ... of the tile, so a wave's loads (16 bytes per lane) and stores (8 or 4 bytes per lane) are contiguous.  A whole
// group inside [0, len_b) moves as one vector load and one vector store; the last partial group of a row goes sample by sample,
// so that no byte at or beyond the row's byte length is written and nothing outside [0, len_b) is read.  No LDS, no atomics.
#include "host.h"
#include "pcm_quantise.h"

#include <vector>

namespace mtts {

using f32x4 = __attribute__((ext_vector_type(4))) float;
using u32x2 = __attribute__((ext_vector_type(2))) unsigned int;

constexpr int CODEC_TILE = MTTS_CODEC_TILE;
constexpr int CODEC_THREADS = 256;
constexpr int CODEC_GROUPS = CODEC_TILE / (4 * CODEC_THREADS);     // groups of 4 samples per lane
static_assert(CODEC_GROUPS >= 1 && CODEC_GROUPS * 4 * CODEC_THREADS == CODEC_TILE, "a tile is whole groups for every lane");

struct EncodeArgs {
    const float* audio;          // [B][ld]
    const int64_t* lengths;      // [B] samples
    const int32_t* formats;      // [B]
    const int64_t* keys;         // [B] or null
    int64_t ld;
    uint8_t* out;                // [B][2 * ld]
    int64_t* out_bytes;          // [B]
    unsigned int seed_lo, seed_hi;
    int dither;
};
struct DecodeArgs {
    const uint8_t* data;         // [B][ld_bytes]
    const int64_t* lengths;      // [B] samples
    const int32_t* formats;      // [B]
    int64_t ld_bytes, ld;
    float* out;                  // [B][ld]
    int64_t* out_lengths;        // [B]
};

// number of i in [0, 8) with v > (e0 << i) - 1
__device__ __forceinline__ int g711_segment(int v, int e0) {
    int s = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) s += v > (e0 << i) - 1;
    return s;
}
__device__ __forceinline__ unsigned int ulaw_of(int q) {
    int v = q >> 2;
    int mask = 0xFF;
    if (v < 0) { v = -v; mask = 0x7F; }
    v = (v > 8159 ? 8159 : v) + 33;
    const int s = g711_segment(v, 0x40);
    const int c = s == 8 ? 0x7F : ((s << 4) | ((v >> (s + 1)) & 15));
    return (unsigned int)((c ^ mask) & 0xFF);
}
__device__ __forceinline__ unsigned int alaw_of(int q) {
    int v = q >> 3;
    int mask = 0xD5;
    if (v < 0) { v = -v - 1; mask = 0x55; }
    const int s = g711_segment(v, 0x20);
    const int c = s == 8 ? 0x7F : ((s << 4) | ((v >> (s < 2 ? 1 : s)) & 15));
    return (unsigned int)((c ^ mask) & 0xFF);
}
__device__ __forceinline__ int ulaw_linear(unsigned int byte) {
    const int c = (int)(~byte & 0xFFu);
    const int t = (((c & 15) << 3) + 132) << ((c >> 4) & 7);
    return (c & 0x80) ? 132 - t : t - 132;
}
__device__ __forceinline__ int alaw_linear(unsigned int byte) {
    const int c = (int)((byte ^ 0x55u) & 0xFFu);
    const int s = (c >> 4) & 7;
    int t = (c & 15) << 4;
    t = s == 0 ? t + 8 : (t + 0x108) << (s - 1);
    return (c & 0x80) ? t : -t;
}
__device__ __forceinline__ bool codec_format_ok(int fmt) { return fmt == MTTS_PCM16 || fmt == MTTS_ULAW || fmt == MTTS_ALAW; }

__global__ __launch_bounds__(CODEC_THREADS) void pcm_encode_kernel(const EncodeArgs a) {
    const int tid = threadIdx.x;
    const int b = blockIdx.y;
    const int64_t len = a.lengths[b];
    const int fmt = a.formats[b];
    const bool ok = len >= 0 && len <= a.ld && codec_format_ok(fmt);
    const bool wide = fmt == MTTS_PCM16;
    if (blockIdx.x == 0 && tid == 0) a.out_bytes[b] = ok ? len * (wide ? 2 : 1) : -1;
    if (!ok) return;                             // a refused row: no byte written
    const int64_t j0 = (int64_t)blockIdx.x * CODEC_TILE;
    if (j0 >= len) return;
    const float* row = a.audio + (size_t)b * a.ld;
    uint8_t* orow = a.out + (size_t)b * 2 * a.ld;
    const bool dith = a.dither && wide;
    const unsigned int hrow = dith ? dither_row_hash(a.seed_lo, a.seed_hi, a.keys ? a.keys[b] : 0) : 0u;
#pragma unroll
    for (int g = 0; g < CODEC_GROUPS; ++g) {
        const int64_t j = j0 + 4 * (tid + g * CODEC_THREADS);
        if (j >= len) continue;
        const int n = len - j >= 4 ? 4 : (int)(len - j);         // samples of this group inside the row
        f32x4 x = {0.f, 0.f, 0.f, 0.f};
        if (n == 4) {
            x = *reinterpret_cast<const f32x4*>(row + j);
        } else {
#pragma unroll
            for (int e = 0; e < 3; ++e)
                if (e < n) x[e] = row[j + e];
        }
        int q[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            float y = x[e] * 32768.f;
            if (dith) y = y + dither_tpdf(hrow, (unsigned int)(j + e));
            q[e] = quantise16(y);
        }
        if (wide) {
            if (n == 4) {
                u32x2 w;
                w[0] = ((unsigned int)q[0] & 0xFFFFu) | ((unsigned int)q[1] << 16);
                w[1] = ((unsigned int)q[2] & 0xFFFFu) | ((unsigned int)q[3] << 16);
                *reinterpret_cast<u32x2*>(orow + 2 * j) = w;
            } else {
#pragma unroll
                for (int e = 0; e < 3; ++e)
                    if (e < n) *reinterpret_cast<unsigned short*>(orow + 2 * (j + e)) = (unsigned short)((unsigned int)q[e] & 0xFFFFu);
            }
        } else {
            unsigned int c[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) c[e] = fmt == MTTS_ULAW ? ulaw_of(q[e]) : alaw_of(q[e]);
            if (n == 4) {
                *reinterpret_cast<unsigned int*>(orow + j) = c[0] | (c[1] << 8) | (c[2] << 16) | (c[3] << 24);
            } else {
#pragma unroll
                for (int e = 0; e < 3; ++e)
                    if (e < n) orow[j + e] = (uint8_t)c[e];
            }
        }
    }
}

__global__ __launch_bounds__(CODEC_THREADS) void pcm_decode_kernel(const DecodeArgs a) {
    const int tid = threadIdx.x;
    const int b = blockIdx.y;
    const int64_t len = a.lengths[b];
    const int fmt = a.formats[b];
    const bool wide = fmt == MTTS_PCM16;
    const bool ok = codec_format_ok(fmt) && len >= 0 && len <= a.ld && len * (wide ? 2 : 1) <= a.ld_bytes;
    if (blockIdx.x == 0 && tid == 0) a.out_lengths[b] = ok ? len : -1;
    if (!ok) return;                             // a refused row: left unwritten
    const int64_t j0 = (int64_t)blockIdx.x * CODEC_TILE;
    const uint8_t* row = a.data + (size_t)b * a.ld_bytes;
    float* orow = a.out + (size_t)b * a.ld;
#pragma unroll
    for (int g = 0; g < CODEC_GROUPS; ++g) {
        const int64_t j = j0 + 4 * (tid + g * CODEC_THREADS);
        if (j >= a.ld) continue;                 // (ld % 4 == 0: a group is inside the row or outside)
        const int n = j >= len ? 0 : (len - j >= 4 ? 4 : (int)(len - j));
        int v[4] = {0, 0, 0, 0};
        if (wide) {
            if (n == 4) {
                const u32x2 w = *reinterpret_cast<const u32x2*>(row + 2 * j);
                v[0] = (int)(short)(w[0] & 0xFFFFu); v[1] = (int)(short)(w[0] >> 16);
                v[2] = (int)(short)(w[1] & 0xFFFFu); v[3] = (int)(short)(w[1] >> 16);
            } else {
#pragma unroll
                for (int e = 0; e < 3; ++e)
                    if (e < n) v[e] = (int)*reinterpret_cast<const short*>(row + 2 * (j + e));
            }
        } else {
            unsigned int c[4] = {0u, 0u, 0u, 0u};
            if (n == 4) {
                const unsigned int w = *reinterpret_cast<const unsigned int*>(row + j);
                c[0] = w & 0xFFu; c[1] = (w >> 8) & 0xFFu; c[2] = (w >> 16) & 0xFFu; c[3] = w >> 24;
            } else {
#pragma unroll
                for (int e = 0; e < 3; ++e)
                    if (e < n) c[e] = row[j + e];
            }
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = e < n ? (fmt == MTTS_ULAW ? ulaw_linear(c[e]) : alaw_linear(c[e])) : 0;
        }
        f32x4 y;
#pragma unroll
        for (int e = 0; e < 4; ++e) y[e] = (float)v[e] * 0x1p-15f;          // (/ 32768: exact)
        *reinterpret_cast<f32x4*>(orow + j) = y;
    }
}

}  // namespace mtts

using namespace mtts;

// ld, B and the grid's limits, shared by the two entries
static int codec_shape_ok(const char* who, int B, int64_t ld) {
    if (B < 1 || B > 65535) { set_error(std::string(who) + ": B must lie in [1, 65535]"); return -1; }
    if (ld < 4 || (ld & 3)) { set_error(std::string(who) + ": rows must be 16-byte aligned (ld a positive multiple of 4 samples)"); return -1; }
    if (ld > (int64_t)1 << 30) { set_error(std::string(who) + ": rows longer than 2^30 samples"); return -1; }
    return 0;
}
static bool codec_overlap(const void* p, size_t np, const void* q, size_t nq) {
    const uintptr_t a = reinterpret_cast<uintptr_t>(p), b = reinterpret_cast<uintptr_t>(q);
    return a < b + nq && b < a + np;
}

extern "C" {

int mtts_codec_tile(void) { return CODEC_TILE; }

int mtts_pcm_encode(const float* d_audio, int64_t ld, const int64_t* d_lengths, const int32_t* d_formats, const int64_t* d_keys,
                    int B, int dither, int64_t seed, uint8_t* d_out, int64_t* d_out_bytes, void* stream) {
    if (!d_audio || !d_lengths || !d_formats || !d_out || !d_out_bytes) { set_error("mtts_pcm_encode: null argument"); return -1; }
    if (codec_shape_ok("mtts_pcm_encode", B, ld)) return -1;
    if ((reinterpret_cast<uintptr_t>(d_audio) & 15) || (reinterpret_cast<uintptr_t>(d_out) & 15)) {
        set_error("mtts_pcm_encode: misaligned buffer (16 bytes)");
        return -1;
    }
    if (codec_overlap(d_audio, (size_t)B * ld * sizeof(float), d_out, (size_t)B * 2 * ld)) {
        set_error("mtts_pcm_encode: d_out overlaps d_audio");
        return -1;
    }
    EncodeArgs a;
    a.audio = d_audio; a.lengths = d_lengths; a.formats = d_formats; a.keys = d_keys; a.ld = ld; a.out = d_out; a.out_bytes = d_out_bytes;
    a.seed_lo = (unsigned int)((uint64_t)seed & 0xFFFFFFFFu);
    a.seed_hi = (unsigned int)((uint64_t)seed >> 32);
    a.dither = dither ? 1 : 0;
    const unsigned tiles = (unsigned)((ld + CODEC_TILE - 1) / CODEC_TILE);
    hipLaunchKernelGGL(pcm_encode_kernel, dim3(tiles, B), dim3(CODEC_THREADS), 0, static_cast<hipStream_t>(stream), a);
    return launched("pcm_encode_kernel");
}

int mtts_pcm_decode(const uint8_t* d_data, int64_t ld_bytes, const int64_t* d_lengths, const int32_t* d_formats, int B,
                    float* d_out, int64_t ld, int64_t* d_out_lengths, void* stream) {
    if (!d_data || !d_lengths || !d_formats || !d_out || !d_out_lengths) { set_error("mtts_pcm_decode: null argument"); return -1; }
    if (codec_shape_ok("mtts_pcm_decode", B, ld)) return -1;
    if (ld_bytes < 16 || (ld_bytes & 15) || ld_bytes > (int64_t)1 << 31) {
        set_error("mtts_pcm_decode: ld_bytes must be a positive multiple of 16, at most 2^31");
        return -1;
    }
    if ((reinterpret_cast<uintptr_t>(d_data) & 15) || (reinterpret_cast<uintptr_t>(d_out) & 15)) {
        set_error("mtts_pcm_decode: misaligned buffer (16 bytes)");
        return -1;
    }
    if (codec_overlap(d_data, (size_t)B * ld_bytes, d_out, (size_t)B * ld * sizeof(float))) {
        set_error("mtts_pcm_decode: d_out overlaps d_data");
        return -1;
    }
    DecodeArgs a;
    a.data = d_data; a.lengths = d_lengths; a.formats = d_formats; a.ld_bytes = ld_bytes; a.ld = ld; a.out = d_out; a.out_lengths = d_out_lengths;
    const unsigned tiles = (unsigned)((ld + CODEC_TILE - 1) / CODEC_TILE);
    hipLaunchKernelGGL(pcm_decode_kernel, dim3(tiles, B), dim3(CODEC_THREADS), 0, static_cast<hipStream_t>(stream), a);
    return launched("pcm_decode_kernel");
}

// The verdict of a call: its d_out_bytes / d_out_lengths.  The one entry of this file that waits for the stream.
int mtts_pcm_status(const int64_t* d_verdict, int B, void* stream) {
    if (!d_verdict || B < 1 || B > 65535) { set_error("mtts_pcm_status: bad argument"); return -1; }
    std::vector<int64_t> v((size_t)B);
    if (read_status("mtts_pcm_status", d_verdict, stream, v.data(), B)) return -1;
    for (int b = 0; b < B; ++b)
        if (v[b] < 0) {
            set_error("mtts_pcm_encode / mtts_pcm_decode: row " + std::to_string(b) + " was refused (a length outside its row, "
                      "an unknown format, or a row an earlier stage refused)");
            return -1;
        }
    return 0;
}

}  // extern "C"
