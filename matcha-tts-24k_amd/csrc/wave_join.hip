// Document join for a ragged batch (gfx950): the finished rows of mtts_waveform_finish -- one sentence each -- into one waveform per
// document, with silence between the sentences, a short fade at the interior joints and one gain per document, in two launches:
//   1. join_plan_kernel  (one workgroup): the layout check of first_row, then per document (one wave each, 64 rows per step) the
//                        exclusive scan of len_b + gap_b in row order -> starts / out_lengths, the document gain min_b scale[b] and
//                        each row's ratio g_doc / scale[b]; every length, gap and range is checked here, BEFORE the move indexes with
//                        them, and the verdict goes to the workspace header (the ragged-batch contract)
//   2. join_move_kernel  (output tile, document): a gather over the output like sil_norm_kernel (corpus.hip): the source row of an
//                        output sample is the last row of the document whose start is at or before it, found by a search over the
//                        starts staged in LDS, JOIN_STAGE rows at a time; 16-byte stores, 4-byte loads (a start has any alignment)
// A document is spread over the grid, never owned by one workgroup.  Every word of out[g][0 .. out_ld) is written exactly once:
// samples, the zeros of a gap and the zeros behind the document; a refused document is all zeros.  Integer arithmetic is int64 and
// a function of the document alone; samples are moved bit for bit unless a gain or a fade weight applies (include/mtts.h).
#include "host.h"
#include "device_utils.h"

#include <cmath>

namespace mtts {

using f32x4 = __attribute__((ext_vector_type(4))) float;

// Inclusive scan over the 64 lanes of a wave (integers: the order of the additions does not matter)
__device__ __forceinline__ long long join_scan(long long v, int lane) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const long long t = __shfl_up(v, o);
        if (lane >= o) v += t;
    }
    return v;
}
__device__ __forceinline__ float join_min(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fminf(v, __shfl_xor(v, o));
    return v;
}

// What row r of a document [r0, r1) adds to the scan, and why it is refused (0: it is not)
__device__ __forceinline__ int join_row(const WaveJoinArgs& a, int r, int r1, long long& v) {
    const int64_t L = a.lengths[r], gp = r + 1 < r1 ? a.gap[r] : 0;      // the gap after the last row is not read
    v = 0;
    if (L < 0 || L > a.ld) return 1;
    if (gp < 0 || gp > a.gap_max) return 2;
    v = L + gp;
    return 0;
}

__global__ __launch_bounds__(256) void join_plan_kernel(const WaveJoinArgs a) {
    __shared__ int s_firstbad, s_fit_row;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid == 0) { s_firstbad = a.G; s_fit_row = a.B; }
    __syncthreads();
    // the layout: 0 = first_row[0] < first_row[1] < ... < first_row[G] = B.  Documents from the first break on are refused: the
    // ones before it are disjoint ranges inside [0, B)
    int mine = a.G;
    for (int g = a.G - 1 - tid; g >= 0; g -= 256) {
        const int r0 = a.first_row[g], r1 = a.first_row[g + 1];
        if (!(r0 >= 0 && r0 < r1 && r1 <= a.B && (g > 0 || r0 == 0) && (g < a.G - 1 || r1 == a.B))) mine = g;
    }
    if (mine < a.G) atomicMin(&s_firstbad, mine);
    for (int b = tid; b < a.B; b += 256) {
        a.starts[b] = -1;
        a.code[b] = 0;
        a.ratio[b] = 1.0f;
    }
    __syncthreads();
    const int firstbad = s_firstbad;
    for (int g = firstbad + tid; g < a.G; g += 256) a.out_lengths[g] = -1;
    for (int g = wave; g < firstbad; g += 4) {                        // wave-uniform
        const int r0 = a.first_row[g], r1 = a.first_row[g + 1];
        long long carry = 0;
        bool bad = false;
        float gmin = INFINITY;
        for (int c = r0; c < r1; c += 64) {
            const int r = c + lane;
            long long v = 0;
            int code = 0;
            if (r < r1) {
                code = join_row(a, r, r1, v);
                if (code) a.code[r] = code;
                if (a.scale) gmin = fminf(gmin, a.scale[r]);
            }
            bad |= __any(code != 0) != 0;
            carry += __shfl(join_scan(v, lane), 63);
        }
        const float g_doc = a.scale ? join_min(gmin) : 1.0f;
        const bool fits = carry <= a.out_ld;
        if (!bad && !fits && lane == 0) atomicMin(&s_fit_row, r0);
        if (lane == 0) a.out_lengths[g] = bad || !fits ? -1 : carry;
        if (bad || !fits) continue;
        carry = 0;
        for (int c = r0; c < r1; c += 64) {
            const int r = c + lane;
            long long v = 0;
            if (r < r1) join_row(a, r, r1, v);
            const long long incl = join_scan(v, lane);
            if (r < r1) {
                a.starts[r] = carry + incl - v;
                if (a.scale) a.ratio[r] = g_doc / a.scale[r];
            }
            carry += __shfl(incl, 63);
        }
    }
    __syncthreads();
    // the verdict: the first row that is refused for itself (length, gap), that opens a document which does not fit, or at which
    // the layout breaks (the first row no document before the break holds, held to B - 1)
    const int fit_row = s_fit_row;
    int layout_row = a.B;
    if (firstbad < a.G) {
        const int end = firstbad > 0 ? a.first_row[firstbad] : 0;     // (the end of a checked document: inside (0, B])
        layout_row = end < a.B ? end : a.B - 1;
    }
    const int i = first_refused_row(a.B, [&](int r) { return a.code[r] != 0 || r == layout_row || r == fit_row; });
    if (tid == 0) {
        int64_t reason = 0;
        if (i < a.B) reason = a.code[i] == 1 ? 1 : (a.code[i] == 2 || i == layout_row) ? 2 : 3;
        a.status[0] = i < a.B ? i + 1 : 0;
        a.status[1] = i < a.B ? sat32(a.lengths[i]) : 0;
        a.status[2] = a.ld;
        a.status[3] = reason;
        a.status[4] = a.out_ld;
        a.status[5] = a.gap_max;
    }
}

// The first index in [lo, hi) of the ascending `st` whose value is above j (hi when there is none)
template <class P>
__device__ __forceinline__ int join_upper(P st, int lo, int hi, int64_t j) {
    while (lo < hi) {
        const int mid = lo + ((hi - lo) >> 1);
        if (st[mid] <= j) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

__global__ __launch_bounds__(256) void join_move_kernel(const WaveJoinArgs a) {
    __shared__ int64_t s_st[JOIN_STAGE], s_ln[JOIN_STAGE];
    __shared__ float s_rt[JOIN_STAGE];
    const int g = blockIdx.y, tid = threadIdx.x;
    const int64_t total = a.out_lengths[g];                            // -1: refused, the row becomes zeros
    const int64_t j0 = (int64_t)blockIdx.x * JOIN_TILE;
    float* orow = a.out + (size_t)g * a.out_ld;
    f32x4 v[JOIN_TILE / 1024];
#pragma unroll
    for (int q = 0; q < JOIN_TILE / 1024; ++q) v[q] = f32x4{0.f, 0.f, 0.f, 0.f};
    if (j0 < total) {                                                  // workgroup-uniform; first_row[g .. g + 1] passed the plan
        const int r0 = a.first_row[g], r1 = a.first_row[g + 1];
        const int64_t jend = (j0 + JOIN_TILE < total ? j0 + JOIN_TILE : total) - 1;
        // the rows this tile reads: from the row of its first sample to the row of its last one (starts[r0] = 0 <= j0).  Rows of
        // no samples and no gap share a start with their successor and the search passes them by
        const int ra = join_upper(a.starts, r0, r1, j0) - 1, rb = join_upper(a.starts, r0, r1, jend) - 1;
        for (int c = ra; c <= rb; c += JOIN_STAGE) {
            const int n = rb + 1 - c < JOIN_STAGE ? rb + 1 - c : JOIN_STAGE;
            __syncthreads();
            if (tid < n) {
                s_st[tid] = a.starts[c + tid];
                s_ln[tid] = a.lengths[c + tid];
                s_rt[tid] = a.ratio[c + tid];
            }
            __syncthreads();
            // a sample at or after this stage's first start takes its value from this stage; a later stage that starts at or
            // before it overwrites that (only then was this stage's last row not the sample's own, and the value a gap's zero)
#pragma unroll
            for (int q = 0; q < JOIN_TILE / 1024; ++q) {
                const int64_t j = j0 + q * 1024 + 4 * tid;
                if (j >= total || j + 3 < s_st[0]) continue;
                int k = join_upper(s_st, 0, n, j) - 1;
                if (k < 0) k = 0;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int64_t jj = j + e;
                    while (k + 1 < n && s_st[k + 1] <= jj) ++k;
                    if (jj < s_st[k]) continue;
                    const int64_t i = jj - s_st[k], len = s_ln[k];
                    float x = 0.f;
                    if (i < len) {
                        const int row = c + k;
                        x = a.audio[(size_t)row * a.ld + i];
                        const float r = s_rt[k];
                        if (r != 1.0f) x = x * r;
                        const int64_t F = a.fade < len / 2 ? a.fade : len / 2;
                        if (row != r0 && i < F) x = x * ((float)(2 * i + 1) / (float)(2 * F));
                        else if (row != r1 - 1 && len - 1 - i < F) x = x * ((float)(2 * (len - 1 - i) + 1) / (float)(2 * F));
                    }
                    v[q][e] = x;
                }
            }
        }
    }
#pragma unroll
    for (int q = 0; q < JOIN_TILE / 1024; ++q) {
        const int64_t j = j0 + q * 1024 + 4 * tid;                    // out_ld % 4 == 0: a quad is inside the row or outside
        if (j < a.out_ld) *reinterpret_cast<f32x4*>(orow + j) = v[q];
    }
}

hipError_t launch_wave_join(const WaveJoinArgs& a, hipStream_t s) {
    if (!a.audio || !a.lengths || !a.first_row || !a.gap || !a.out || !a.out_lengths || !a.starts || !a.status || !a.ratio || !a.code)
        return hipErrorInvalidValue;
    if (a.B <= 0 || a.B > 65535 || a.G <= 0 || a.G > a.B || a.ld < 4 || a.out_ld < 4 || (a.ld & 3) || (a.out_ld & 3)) return hipErrorInvalidValue;
    if ((reinterpret_cast<uintptr_t>(a.audio) & 15) || (reinterpret_cast<uintptr_t>(a.out) & 15) || a.fade < 0 || a.gap_max < 0) return hipErrorInvalidValue;
    const int64_t tiles = (a.out_ld + JOIN_TILE - 1) / JOIN_TILE;
    if (tiles > 0x7fffffff) return hipErrorInvalidValue;
    hipLaunchKernelGGL(join_plan_kernel, dim3(1), dim3(256), 0, s, a);
    hipLaunchKernelGGL(join_move_kernel, dim3((unsigned)tiles, a.G), dim3(256), 0, s, a);
    return hipGetLastError();
}

}  // namespace mtts

using namespace mtts;

extern "C" {

// ---- document join (wave_join.hip)
int64_t mtts_wave_join_workspace_bytes(int64_t B, int64_t G) {
    if (B < 1 || G < 1 || G > B || B > (int64_t)1 << 56) { set_error("mtts_wave_join_workspace_bytes: need 1 <= G <= B"); return -1; }
    WS ws(nullptr, 0);
    ws.bytes(256);
    ws.f((size_t)B);
    ws.bytes((size_t)B * sizeof(int32_t));
    return (int64_t)ws.off + 256;
}

int mtts_wave_join(const float* d_audio, int64_t ld, const int64_t* d_lengths, const float* d_scale, const int32_t* d_first_row,
                   const int64_t* d_gap, int B, int G, int64_t fade, int64_t gap_max, float* d_out, int64_t out_ld, int64_t* d_out_lengths,
                   int64_t* d_starts, void* d_ws, int64_t ws_bytes, void* stream) {
    if (!d_audio || !d_lengths || !d_first_row || !d_gap || !d_out || !d_out_lengths || !d_starts || !d_ws) {
        set_error("mtts_wave_join: null argument");
        return -1;
    }
    if (B < 1 || B > 65535 || G < 1 || G > B) { set_error("mtts_wave_join: need 1 <= G <= B <= 65535 (no document is empty)"); return -1; }
    if (ld < 4 || out_ld < 4 || (ld & 3) || (out_ld & 3) || (reinterpret_cast<uintptr_t>(d_audio) & 15) || (reinterpret_cast<uintptr_t>(d_out) & 15) ||
        (reinterpret_cast<uintptr_t>(d_ws) & 15)) {
        set_error("mtts_wave_join: rows must be 16-byte aligned (ld and out_ld positive multiples of 4 samples)");
        return -1;
    }
    if (ld > (int64_t)1 << 40 || out_ld > (int64_t)1 << 40 || gap_max > (int64_t)1 << 40) { set_error("mtts_wave_join: a row of more than 2^40 samples"); return -1; }
    if (fade < 0 || gap_max < 0) { set_error("mtts_wave_join: fade and gap_max must not be negative"); return -1; }
    const uintptr_t in0 = reinterpret_cast<uintptr_t>(d_audio), in1 = in0 + (uintptr_t)B * ld * sizeof(float);
    const uintptr_t out0 = reinterpret_cast<uintptr_t>(d_out), out1 = out0 + (uintptr_t)G * out_ld * sizeof(float);
    if (in0 < out1 && out0 < in1) { set_error("mtts_wave_join: the join is not in place (d_out overlaps d_audio)"); return -1; }
    WaveJoinArgs a;
    WS ws(d_ws, (size_t)ws_bytes);
    a.status = static_cast<int64_t*>(ws.bytes(256));
    a.ratio = ws.f((size_t)B);
    a.code = static_cast<int32_t*>(ws.bytes((size_t)B * sizeof(int32_t)));
    if (ws_bytes < 256 || ws.overflow) { set_error("mtts_wave_join: workspace too small (mtts_wave_join_workspace_bytes)"); return -1; }
    a.audio = d_audio; a.ld = ld; a.lengths = d_lengths; a.scale = d_scale; a.first_row = d_first_row; a.gap = d_gap; a.B = B; a.G = G;
    a.fade = fade; a.gap_max = gap_max; a.out = d_out; a.out_ld = out_ld; a.out_lengths = d_out_lengths; a.starts = d_starts;
    HIP_OK(launch_wave_join(a, static_cast<hipStream_t>(stream)));
    return 0;
}

// The verdict of the latest mtts_wave_join on this workspace.  Waits for the stream.
int mtts_wave_join_status(const void* d_ws, void* stream) {
    int64_t st[6];
    if (read_status("mtts_wave_join_status", d_ws, stream, st)) return -1;
    if (st[0] == 0) return 0;
    const std::string row = "mtts_wave_join: row " + std::to_string(st[0] - 1) + " (length " + std::to_string(st[1]) + ") is refused: ";
    if (st[3] == 1) set_error(row + "its length is outside [0, ld = " + std::to_string(st[2]) + "]");
    else if (st[3] == 2)
        set_error(row + "the layout or a gap is wrong (need 0 = first_row[0] < first_row[1] < ... < first_row[G] = B and 0 <= gap <= " +
                  std::to_string(st[5]) + ")");
    else set_error(row + "its document does not fit out_ld = " + std::to_string(st[4]) + " samples");
    return -1;
}

}  // extern "C"
