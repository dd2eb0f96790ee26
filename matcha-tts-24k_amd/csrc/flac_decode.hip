// FLAC in (gfx950): a ragged batch of whole native FLAC streams (RFC 9639) to fp32 rows, decoded on the device.
//
// The contract is include/mtts.h "FLAC in"; the parser is flac_parse.h, the same functions mtts_flac_parse_host runs on host memory.
// Work is parallel over frames, and a frame's start is known only by finding it.  Six plain launches on a fixed workspace, no flags
// between workgroups, no spinning; every word a kernel reads from the workspace an earlier launch of the same call wrote:
//   0. flac_info_kernel, one thread per row: the metadata chain -> STREAMINFO's words and the first frame's offset, or the row's refusal.
//   1. flac_scan_kernel, grid (tile of 1024 bytes, row), 256 threads: the tile and a halo of 16 bytes staged in LDS by 16-byte loads;
//      every thread tests its byte positions for the candidate rule (header parse + CRC-8); a wave's 64 flags are one ballot word.
//   2. flac_plan_kernel, one workgroup per row: the candidates in position order (popcounts through an ordered block scan, no atomics)
//      with their header facts, and the exclusive scan of their block sizes = their staging offsets.  More than ld / 16 + 64
//      candidates or 2 * ld + max_block staged samples refuse the row.
//   3. flac_frame_kernel, grid (candidate, row), one wavefront: lane 0 runs the serial entropy parse and the prediction restore into
//      LDS (two channels of max_block words: 36 KB at 4608, four waves per CU); then all lanes rebuild channel 0 from the stereo
//      pair, check its range, store it to staging and compute the CRC-16 by chunks joined with x^(8 L 2^l) (the register is linear
//      in the message).  The restore is lane-serial as well: the recurrence x[i] = r[i] + (sum_j c[j] x[i-1-j] >> shift) leaves 32
//      independent MACs per sample, which one lane issues back to back from LDS; spreading them over lanes costs a cross-lane
//      reduction per sample, five DPP steps on the critical path, for at most 32 products.
//   4. flac_walk_kernel, one thread per row: the acceptance chain from the first frame's offset over the candidate list (binary
//      search by position), numbering and total -> d_out_lengths, d_out_rates and each on-walk frame's output offset.
//   5. flac_gather_kernel, grid (candidate + zero tile, row): on-walk frames from staging to d_out as fp32, 16-byte stores where
//      aligned, and the zeros behind the length; nothing for a refused row.
// Every loop is bounded by the block size, 32 coefficients, the row's bytes or the candidate capacity (flac_parse.h).
#include "host.h"
#include "flac_parse.h"

namespace mtts {
namespace fl = mtts_flac;

constexpr int FD_THREADS = 256;
constexpr int FD_WAVES = FD_THREADS / 64;
constexpr int FD_TILE = 1024;                    // bytes of a scan tile: four positions per thread
constexpr int FD_WINDOW = FD_TILE + fl::MAX_HEADER;
constexpr int FD_ZTILE = 4096;                   // samples of a zero tile
using f32x4 = __attribute__((ext_vector_type(4))) float;
using u32x4d = __attribute__((ext_vector_type(4))) unsigned int;

struct FlacDecArgs {
    const uint8_t* data;         // [B][ld_bytes]
    const int64_t* nbytes;       // [B]
    int64_t ld_bytes, ld;
    int B, max_block;
    float* out;                  // [B][ld]
    int64_t* out_lengths;        // [B]
    int32_t* out_rates;          // [B]
    // the workspace
    int64_t nwords, cap, stage_cap;
    fl::Info* info;              // [B]
    int32_t* ncand;              // [B]
    unsigned long long* mask;    // [B][nwords] bit i of word w: byte 64 w + i is a candidate
    int64_t* cpos;               // [B][cap] per candidate: byte position,
    int64_t* cstage;             //   staging offset,
    int64_t* cnum;               //   coded number,
    int64_t* cout;               //   output offset when on the walk, else -1,
    int32_t* cbs;                //   block size,
    int32_t* cvar;               //   blocking strategy bit,
    int32_t* clen;               //   byte length, or -1 when it is no frame
    int32_t* staging;            // [B][stage_cap]
};

__device__ __forceinline__ int64_t fd_row_bytes(const FlacDecArgs& a, int b) {
    const int64_t nb = a.nbytes[b];
    return (nb < 0 || nb > a.ld_bytes) ? -1 : nb;
}

// exclusive scan of v over the workgroup in thread order, and the total; wsum: FD_WAVES words of LDS
__device__ __forceinline__ long long fd_exscan(long long v, long long* wsum, long long& total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    long long inc = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const long long t = __shfl_up(inc, o);
        if (lane >= o) inc += t;
    }
    __syncthreads();
    if (lane == 63) wsum[wave] = inc;
    __syncthreads();
    long long base = 0;
    total = 0;
#pragma unroll
    for (int w = 0; w < FD_WAVES; ++w) {
        const long long s = wsum[w];
        if (w < wave) base += s;
        total += s;
    }
    return base + inc - v;
}

__global__ __launch_bounds__(64) void flac_info_kernel(const FlacDecArgs a) {
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= a.B) return;
    fl::Info info = {};
    const int64_t nb = fd_row_bytes(a, b);
    if (nb < 0 || !fl::parse_info(a.data + (size_t)b * a.ld_bytes, nb, a.max_block, info)) info.ok = 0;
    a.info[b] = info;
}

__global__ __launch_bounds__(FD_THREADS) void flac_scan_kernel(const FlacDecArgs a) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, b = blockIdx.y;
    const fl::Info info = a.info[b];
    if (!info.ok) return;                        // (nothing of a refused row's workspace is read later)
    const int64_t tile0 = (int64_t)blockIdx.x * FD_TILE;
    const int64_t nb = a.nbytes[b];
    __shared__ __attribute__((aligned(16))) uint8_t win[FD_WINDOW];
    const uint8_t* row = a.data + (size_t)b * a.ld_bytes;
    if (tid < FD_WINDOW / 16) {                  // 65 loads of 16 bytes; the stride is a multiple of 16, so a chunk is inside it or outside
        const int64_t at = tile0 + 16 * tid;
        u32x4d v = {0u, 0u, 0u, 0u};
        if (at < a.ld_bytes) v = *reinterpret_cast<const u32x4d*>(row + at);
        *reinterpret_cast<u32x4d*>(win + 16 * tid) = v;
    }
    __syncthreads();
    const int64_t left = nb - tile0;
    const int n_local = left < 0 ? 0 : left < FD_WINDOW ? (int)left : FD_WINDOW;
#pragma unroll
    for (int j = 0; j < FD_TILE / FD_THREADS; ++j) {
        const int local = j * FD_THREADS + tid;
        fl::Header h;
        const bool flag = local < n_local && tile0 + local >= info.first && fl::parse_header(win, n_local, local, info, h);
        const unsigned long long word = __ballot(flag);
        const int64_t widx = (tile0 + j * FD_THREADS + wave * 64) >> 6;
        if (lane == 0 && widx < a.nwords) a.mask[(size_t)b * a.nwords + widx] = word;
    }
}

__global__ __launch_bounds__(FD_THREADS) void flac_plan_kernel(const FlacDecArgs a) {
    const int tid = threadIdx.x, b = blockIdx.x;
    const fl::Info info = a.info[b];
    if (!info.ok) return;
    __shared__ long long wsum[FD_WAVES];
    const int64_t nb = a.nbytes[b];
    const uint8_t* row = a.data + (size_t)b * a.ld_bytes;
    const unsigned long long* mask = a.mask + (size_t)b * a.nwords;
    const size_t c0 = (size_t)b * a.cap;
    long long run_c = 0, run_s = 0;
    for (int64_t w0 = 0; w0 < a.nwords; w0 += FD_THREADS) {  // (nwords = ld_bytes / 64, from the host)
        const int64_t w = w0 + tid;
        const unsigned long long word = w < a.nwords ? mask[w] : 0ull;
        long long mine = 0;
        for (unsigned long long m = word; m; m &= m - 1) {   // (at most 64 passes)
            fl::Header h;
            if (fl::parse_header(row, nb, w * 64 + __builtin_ctzll(m), info, h)) mine += h.bs;
        }
        long long ctotal, stotal;
        const long long cbase = fd_exscan(__popcll(word), wsum, ctotal);
        const long long sbase = fd_exscan(mine, wsum, stotal);
        long long idx = run_c + cbase, at = run_s + sbase;
        for (unsigned long long m = word; m; m &= m - 1, ++idx) {
            fl::Header h;
            const int64_t pos = w * 64 + __builtin_ctzll(m);
            if (!fl::parse_header(row, nb, pos, info, h)) h.bs = 0, h.variable = 0, h.number = -1;   // (the scan's own rule: not reached)
            if (idx < a.cap) {
                a.cpos[c0 + idx] = pos;
                a.cstage[c0 + idx] = at;
                a.cnum[c0 + idx] = h.number;
                a.cout[c0 + idx] = -1;
                a.cbs[c0 + idx] = h.bs;
                a.cvar[c0 + idx] = h.variable;
                a.clen[c0 + idx] = -1;
            }
            at += h.bs;
        }
        run_c += ctotal;
        run_s += stotal;
    }
    if (tid == 0) {
        const bool fits = run_c <= a.cap && run_s <= a.stage_cap;
        a.ncand[b] = fits ? (int32_t)run_c : 0;
        if (!fits) a.info[b].ok = 0;             // (this workgroup is the row's only one; later launches read it)
    }
}

extern __shared__ __attribute__((aligned(16))) int32_t fd_lds[];

__global__ __launch_bounds__(64) void flac_frame_kernel(const FlacDecArgs a) {
    const int lane = threadIdx.x, b = blockIdx.y;
    const int64_t c = blockIdx.x;
    const fl::Info info = a.info[b];
    if (!info.ok || c >= a.ncand[b]) return;
    int32_t* ch0 = fd_lds;                       // [max_block]
    int32_t* ch1 = fd_lds + a.max_block;         // [max_block]
    int32_t* coef = fd_lds + 2 * a.max_block;    // [32]
    __shared__ long long s_len;
    __shared__ int s_assign;
    const int64_t nb = a.nbytes[b];
    const uint8_t* row = a.data + (size_t)b * a.ld_bytes;
    const size_t ci = (size_t)b * a.cap + c;
    const int64_t at = a.cpos[ci];
    const int bs = a.cbs[ci];
    if (lane == 0) {
        fl::Header h = {};
        long long len = -1;
        if (fl::parse_header(row, nb, at, info, h) && h.bs <= a.max_block) len = fl::parse_frame(row, nb, at, h, info.bps, ch0, ch1, coef);
        s_len = len;
        s_assign = h.assign;
    }
    __syncthreads();
    const long long len = s_len;
    if (len < 0) return;                         // (clen stays -1, as the plan kernel wrote it)
    const int assign = s_assign;
    // CRC-16 of the len - 2 bytes ahead of it: lane t takes chunk t of L bytes, cut from the END (bytes ahead of the frame read as zeros
    // and leave a register 0); level l joins runs of 2^l chunks: the left register times x^(8 L 2^l), plus the right
    const long long m = len - 2;
    const long long L = (m + 63) / 64;
    unsigned int crc = 0;
    for (long long x = 0, i = m - (64 - lane) * L; x < L; ++x, ++i)
        if (i >= 0) crc = fl::crc16_byte(crc, row[at + i]);
    unsigned int mult = fl::crc16_xpow(8ull * (unsigned long long)L);
#pragma unroll
    for (int l = 0; l < 6; ++l) {
        const int s = 1 << l;
        const unsigned int right = __shfl_down(crc, s);
        if ((lane & (2 * s - 1)) == 0) crc = fl::crc16_mul(crc, mult) ^ right;
        mult = fl::crc16_mul(mult, mult);
    }
    crc = __shfl(crc, 0);
    bool ok = crc == ((unsigned int)row[at + m] << 8 | row[at + m + 1]);
    // channel 0 from the coded pair, its range, and the store to staging (the plan kernel kept the row's sum inside stage_cap)
    int32_t* stage = a.staging + (size_t)b * a.stage_cap + a.cstage[ci];
    bool bad = false;
    for (int i = lane; i < bs; i += 64) {
        const int32_t v = fl::first_channel(assign, ch0[i], assign >= 9 ? ch1[i] : 0);
        bad |= !fl::in_range(v, info.bps);
        stage[i] = v;
    }
    ok = ok && __ballot(bad) == 0ull;
    if (lane == 0 && ok) a.clen[ci] = (int32_t)len;
}

__global__ __launch_bounds__(64) void flac_walk_kernel(const FlacDecArgs a) {
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= a.B) return;
    const fl::Info info = a.info[b];
    int64_t verdict = -1;
    if (info.ok) {
        const int64_t nb = a.nbytes[b];
        const size_t c0 = (size_t)b * a.cap;
        const int64_t n = a.ncand[b];
        fl::Walk w;
        fl::walk_init(w);
        int64_t at = info.first, from = 0;
        bool good = true;
        while (good && at < nb) {                // (`from` grows with every pass: at most n passes)
            int64_t lo = from, hi = n;           // the candidate at `at`, by position
            while (lo < hi) {
                const int64_t mid = (lo + hi) >> 1;
                if (a.cpos[c0 + mid] < at) lo = mid + 1; else hi = mid;
            }
            good = lo < n && a.cpos[c0 + lo] == at && a.clen[c0 + lo] > 0;
            if (!good) break;
            const int bs = a.cbs[c0 + lo];
            good = fl::walk_step(w, a.cvar[c0 + lo], bs, a.cnum[c0 + lo]) && w.total <= a.ld;
            if (!good) break;
            a.cout[c0 + lo] = w.total - bs;
            at += a.clen[c0 + lo];
            from = lo + 1;
        }
        if (good && at == nb) verdict = fl::walk_verdict(w, info, a.ld);
    }
    a.out_lengths[b] = verdict;
    a.out_rates[b] = verdict >= 0 ? info.rate : 0;
}

__global__ __launch_bounds__(FD_THREADS) void flac_gather_kernel(const FlacDecArgs a) {
    const int tid = threadIdx.x, b = blockIdx.y;
    const int64_t len = a.out_lengths[b];
    if (len < 0) return;                         // a refused row: no word written
    float* orow = a.out + (size_t)b * a.ld;
    const int64_t x = blockIdx.x;
    if (x >= a.cap) {                            // a zero tile: [max(len, tile), min(ld, tile + FD_ZTILE)) in groups of 4 (ld % 4 == 0)
        const int64_t tile0 = (x - a.cap) * FD_ZTILE;
        for (int g = tid; g < FD_ZTILE / 4; g += FD_THREADS) {
            const int64_t i0 = tile0 + 4 * g;
            if (i0 >= a.ld || i0 + 4 <= len) continue;
            if (i0 >= len) {
                *reinterpret_cast<f32x4*>(orow + i0) = f32x4{0.f, 0.f, 0.f, 0.f};
            } else {
                for (int64_t i = len; i < i0 + 4; ++i) orow[i] = 0.f;
            }
        }
        return;
    }
    if (x >= a.ncand[b]) return;
    const size_t ci = (size_t)b * a.cap + x;
    const int64_t o0 = a.cout[ci];
    if (o0 < 0) return;                          // off the walk
    const int n = a.cbs[ci];                     // (o0 + n <= len <= ld: the walk kernel checked)
    const int32_t* src = a.staging + (size_t)b * a.stage_cap + a.cstage[ci];
    float* dst = orow + o0;
    const float scale = 1.f / (float)(1 << (a.info[b].bps - 1));     // a power of two: q * scale is exact for |q| < 2^24
    const int lead = (int)((4 - (o0 & 3)) & 3);
    const int head = lead < n ? lead : n;
    const int body = (n - head) / 4, tail = n - head - 4 * body;
    if (tid < head) dst[tid] = (float)src[tid] * scale;
    for (int g = tid; g < body; g += FD_THREADS) {
        const int i = head + 4 * g;
        *reinterpret_cast<f32x4*>(dst + i) = f32x4{(float)src[i] * scale, (float)src[i + 1] * scale, (float)src[i + 2] * scale, (float)src[i + 3] * scale};
    }
    if (tid < tail) {
        const int i = head + 4 * body + tid;
        dst[i] = (float)src[i] * scale;
    }
}

}  // namespace mtts

using namespace mtts;

static int fd_shape_ok(const char* who, int B, int64_t ld_bytes, int64_t ld, int max_block) {
    if (B < 1 || B > 65535) { set_error(std::string(who) + ": B must lie in [1, 65535]"); return -1; }
    if (ld_bytes < 16 || (ld_bytes & 15) || ld_bytes > (int64_t)1 << 31) {
        set_error(std::string(who) + ": ld_bytes must be a positive multiple of 16, at most 2^31");
        return -1;
    }
    if (ld < 4 || (ld & 3) || ld > (int64_t)1 << 30) {
        set_error(std::string(who) + ": ld must be a positive multiple of 4 samples, at most 2^30");
        return -1;
    }
    if (max_block < fl::MIN_MAX_BLOCK || max_block > fl::MAX_BLOCK) { set_error(std::string(who) + ": max_block must lie in [16, 4608]"); return -1; }
    return 0;
}
// the sections of the workspace, carved the same way by the size query and by the call
static void fd_carve(WS& ws, FlacDecArgs& a) {
    const size_t B = (size_t)a.B, cands = B * (size_t)a.cap;
    a.nwords = (a.ld_bytes + 63) / 64;
    a.info = static_cast<fl::Info*>(ws.bytes(B * sizeof(fl::Info)));
    a.ncand = static_cast<int32_t*>(ws.bytes(B * sizeof(int32_t)));
    a.mask = static_cast<unsigned long long*>(ws.bytes(B * (size_t)a.nwords * 8));
    a.cpos = static_cast<int64_t*>(ws.bytes(cands * 8));
    a.cstage = static_cast<int64_t*>(ws.bytes(cands * 8));
    a.cnum = static_cast<int64_t*>(ws.bytes(cands * 8));
    a.cout = static_cast<int64_t*>(ws.bytes(cands * 8));
    a.cbs = static_cast<int32_t*>(ws.bytes(cands * 4));
    a.cvar = static_cast<int32_t*>(ws.bytes(cands * 4));
    a.clen = static_cast<int32_t*>(ws.bytes(cands * 4));
    a.staging = static_cast<int32_t*>(ws.bytes(B * (size_t)a.stage_cap * 4));
}
static void fd_shape(FlacDecArgs& a, int B, int64_t ld_bytes, int64_t ld, int max_block) {
    a.B = B; a.ld_bytes = ld_bytes; a.ld = ld; a.max_block = max_block;
    a.cap = ld / 16 + 64;
    a.stage_cap = 2 * ld + max_block;
}
static bool fd_overlap(const void* p, size_t np, const void* q, size_t nq) {
    const uintptr_t a = reinterpret_cast<uintptr_t>(p), b = reinterpret_cast<uintptr_t>(q);
    return a < b + nq && b < a + np;
}

extern "C" {

int64_t mtts_flac_decode_workspace_bytes(int B, int64_t ld_bytes, int64_t ld, int max_block) {
    if (fd_shape_ok("mtts_flac_decode_workspace_bytes", B, ld_bytes, ld, max_block)) return -1;
    FlacDecArgs a;
    fd_shape(a, B, ld_bytes, ld, max_block);
    WS ws(nullptr, 0);
    fd_carve(ws, a);
    return (int64_t)ws.off;
}

int mtts_flac_decode(const uint8_t* d_data, int64_t ld_bytes, const int64_t* d_nbytes, int B, int max_block, float* d_out, int64_t ld,
                     int64_t* d_out_lengths, int32_t* d_out_rates, void* d_ws, int64_t ws_bytes, void* stream) {
    if (!d_data || !d_nbytes || !d_out || !d_out_lengths || !d_out_rates || !d_ws) { set_error("mtts_flac_decode: null argument"); return -1; }
    if (fd_shape_ok("mtts_flac_decode", B, ld_bytes, ld, max_block)) return -1;
    FlacDecArgs a;
    fd_shape(a, B, ld_bytes, ld, max_block);
    WS ws(d_ws, (size_t)(ws_bytes < 0 ? 0 : ws_bytes));
    fd_carve(ws, a);
    if (ws.overflow) { set_error("mtts_flac_decode: workspace too small (mtts_flac_decode_workspace_bytes)"); return -1; }
    if ((reinterpret_cast<uintptr_t>(d_data) & 15) || (reinterpret_cast<uintptr_t>(d_out) & 15) || (reinterpret_cast<uintptr_t>(d_ws) & 15)) {
        set_error("mtts_flac_decode: misaligned buffer (16 bytes)");
        return -1;
    }
    const size_t in_bytes = (size_t)B * ld_bytes, out_bytes = (size_t)B * ld * sizeof(float);
    if (fd_overlap(d_data, in_bytes, d_out, out_bytes) || fd_overlap(d_data, in_bytes, d_ws, ws.off) || fd_overlap(d_out, out_bytes, d_ws, ws.off)) {
        set_error("mtts_flac_decode: d_out, d_ws and d_data must not overlap");
        return -1;
    }
    a.data = d_data; a.nbytes = d_nbytes; a.out = d_out; a.out_lengths = d_out_lengths; a.out_rates = d_out_rates;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const unsigned rows64 = (unsigned)((B + 63) / 64);
    hipLaunchKernelGGL(flac_info_kernel, dim3(rows64), dim3(64), 0, s, a);
    RET_IF(launched("flac_info_kernel"));
    hipLaunchKernelGGL(flac_scan_kernel, dim3((unsigned)((ld_bytes + FD_TILE - 1) / FD_TILE), B), dim3(FD_THREADS), 0, s, a);
    RET_IF(launched("flac_scan_kernel"));
    hipLaunchKernelGGL(flac_plan_kernel, dim3(B), dim3(FD_THREADS), 0, s, a);
    RET_IF(launched("flac_plan_kernel"));
    const size_t lds = ((size_t)2 * max_block + fl::MAX_ORDER) * sizeof(int32_t);
    hipLaunchKernelGGL(flac_frame_kernel, dim3((unsigned)a.cap, B), dim3(64), lds, s, a);
    RET_IF(launched("flac_frame_kernel"));
    hipLaunchKernelGGL(flac_walk_kernel, dim3(rows64), dim3(64), 0, s, a);
    RET_IF(launched("flac_walk_kernel"));
    const unsigned ztiles = (unsigned)((ld + FD_ZTILE - 1) / FD_ZTILE);
    hipLaunchKernelGGL(flac_gather_kernel, dim3((unsigned)a.cap + ztiles, B), dim3(FD_THREADS), 0, s, a);
    return launched("flac_gather_kernel");
}

// The host twin: the same parser and the same acceptance walk over host memory.  Never touches the GPU.
int64_t mtts_flac_parse_host(const uint8_t* data, int64_t nbytes, int max_block, int32_t* out, int64_t out_capacity, int* rate, int* channels,
                             int* bps) {
    if (!data || !rate || !channels || !bps || (!out && out_capacity > 0) || nbytes < 0 || out_capacity < 0) {
        set_error("mtts_flac_parse_host: null or negative argument");
        return -1;
    }
    if (max_block < fl::MIN_MAX_BLOCK || max_block > fl::MAX_BLOCK) { set_error("mtts_flac_parse_host: max_block must lie in [16, 4608]"); return -1; }
    std::vector<int32_t> ch1((size_t)max_block);
    fl::Info info;
    const int64_t n = fl::parse_stream(data, nbytes, max_block, out, out_capacity, ch1.data(), info);
    *rate = n >= 0 ? info.rate : 0;
    *channels = n >= 0 ? info.channels : 0;
    *bps = n >= 0 ? info.bps : 0;
    if (n < 0) set_error("mtts_flac_parse_host: the stream is refused (include/mtts.h \"FLAC in\")");
    return n;
}

}  // extern "C"
