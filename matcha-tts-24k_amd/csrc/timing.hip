// Token timing for a ragged batch (gfx950): when each token is spoken in the audio mtts_waveform_finish leaves, and pauses cut into
// that audio after chosen tokens, in two launches:
//   1. token_timing_kernel (one workgroup per row, as the duration scan): the row's verdict, then per break the cut c = e_{token+1}
//                          and the pause applied there, the inclusive int64 scan of the applied pauses (serial chunk + block scan)
//                          -> cut / ostart / the new length, and the marks start_i = e_i + P(<i), end_i = e_{i+1} + P(<i); every
//                          length, index and pause is checked here, BEFORE the gather indexes with them (the ragged-batch
//                          contract; the verdict is one record per row, the status entry finds the first)
//   2. wave_breaks_kernel  (output tile, row): a gather over the lengthened row like join_move_kernel (wave_join.hip): the segment
//                          of an output sample is found by a search over ostart; 16-byte stores, 4-byte loads (a cut has any
//                          alignment).  Launched only when a row of the batch has a break.
// Every word of marks[b] and of out[b][0 .. out_ld) is written exactly once; a refused row is all -1 / all zeros.  Integer
// arithmetic is int64 and a function of the row alone; samples are moved bit for bit unless a fade weight applies (include/mtts.h).
#include "host.h"
#include "device_utils.h"

namespace mtts {

using f32x4 = __attribute__((ext_vector_type(4))) float;

constexpr int TIMING_NONE = 0x7fffffff;

// e_k of include/mtts.h: the boundary in front of token k (k in [0, x_len]), held inside [0, keep]
__device__ __forceinline__ int64_t timing_edge(const int32_t* cum, int k, int fine_hop, int64_t keep) {
    if (k == 0) return 0;
    int64_t e = (int64_t)fine_hop * cum[k - 1] - fine_hop / 2;
    e = e < 0 ? 0 : e;
    return e < keep ? e : keep;
}

// The first index in [0, n) of the ascending `v` whose value is at or above x (n when there is none)
template <class T, class U>
__device__ __forceinline__ int timing_lower(const T* v, int n, U x) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = lo + ((hi - lo) >> 1);
        if (v[mid] < x) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

__global__ __launch_bounds__(256) void token_timing_kernel(const TimingArgs a) {
    __shared__ long long part[256];
    __shared__ int s_bad;
    const int b = blockIdx.x, tid = threadIdx.x;
    const int64_t keep = a.keep[b], xl = a.x_len[b];
    const int32_t* cum = a.cum + (size_t)b * a.Tx;
    int64_t* marks = a.marks + (size_t)b * a.Tx * 2;
    if (b == 0 && tid == 0) {
        a.header[0] = a.B; a.header[1] = a.Tx; a.header[2] = a.keep_max; a.header[3] = a.pause_max; a.header[4] = a.out_max; a.header[5] = a.NB;
    }
    // the row itself, then where its breaks lie (workgroup-uniform)
    int reason = 0;
    int64_t detail = keep;
    int k0 = 0, nb = 0;
    if (xl < 1 || xl > a.Tx) { reason = 5; detail = xl; }
    else if (keep < 0 || keep > a.keep_max) reason = 1;
    else if (a.break_first) {
        const int f0 = a.break_first[b], f1 = a.break_first[b + 1];
        if (f0 < 0 || f1 < f0 || f1 > a.NB) { reason = 2; detail = -1; }
        else { k0 = f0; nb = f1 - f0; }
    }
    const int xlen = reason ? 0 : (int)xl;
    const int32_t* tok = a.break_token + k0;
    const int64_t* pause = a.break_pause + k0;
    // the breaks: the first one that is wrong names the reason (the loop runs downwards, so `mine` ends as a thread's smallest)
    if (tid == 0) s_bad = TIMING_NONE;
    __syncthreads();
    int mine = TIMING_NONE;
    for (int i = nb - 1 - tid; i >= 0; i -= 256) {
        const int t = tok[i];
        const int tp = i > 0 ? tok[i - 1] : -1;
        const int64_t p = pause[i];
        int r = 0;
        if (t < 0 || t >= xlen) r = 2;
        else if (i > 0 && tp >= t) r = 3;
        else if (p < 0 || p > a.pause_max) r = 4;
        else if (tp >= 0 && timing_edge(cum, tp + 1, a.fine_hop, keep) > timing_edge(cum, t + 1, a.fine_hop, keep)) r = 6;
        if (r) mine = i * 8 + r;
    }
    if (mine != TIMING_NONE) atomicMin(&s_bad, mine);
    __syncthreads();
    if (!reason && s_bad != TIMING_NONE) { reason = s_bad & 7; detail = s_bad >> 3; }
    // the applied pauses and their inclusive scan
    long long total = 0;
    const int per = (nb + 255) / 256;
    const int i0 = min(nb, tid * per), i1 = min(nb, i0 + per);
    if (!reason && nb > 0) {                                          // workgroup-uniform
        long long s = 0;
        for (int i = i0; i < i1; ++i) {
            const int64_t c = timing_edge(cum, tok[i] + 1, a.fine_hop, keep);
            s += (c == 0 || c >= keep) ? 0 : pause[i];
        }
        part[tid] = s;
        __syncthreads();
        for (int o = 1; o < 256; o <<= 1) {
            const long long v = tid >= o ? part[tid - o] : 0;
            __syncthreads();
            part[tid] += v;
            __syncthreads();
        }
        total = part[255];
        if (keep + total > a.out_max) { reason = 7; detail = keep + total; }
    }
    if (reason) {
        for (int i = tid; i < 2 * a.Tx; i += 256) marks[i] = -1;
        if (tid == 0) {
            a.verdict[2 * b] = reason; a.verdict[2 * b + 1] = detail;
            a.rowinfo[2 * b] = -1; a.rowinfo[2 * b + 1] = -1;
            a.out_lengths[b] = -1;
        }
        return;
    }
    if (nb > 0) {
        long long run = tid ? part[tid - 1] : 0;
        for (int i = i0; i < i1; ++i) {
            const int64_t c = timing_edge(cum, tok[i] + 1, a.fine_hop, keep);
            run += (c == 0 || c >= keep) ? 0 : pause[i];
            a.cut[k0 + i] = c;
            a.ostart[k0 + i] = c + run;
        }
        __syncthreads();                                              // the marks read what other threads wrote
    }
    for (int i = tid; i < a.Tx; i += 256) {
        int64_t st = -1, en = -1;
        if (i < xlen) {
            const int k = timing_lower(tok, nb, i);                   // breaks at tokens < i
            const int64_t P = k > 0 ? a.ostart[k0 + k - 1] - a.cut[k0 + k - 1] : 0;
            st = timing_edge(cum, i, a.fine_hop, keep) + P;
            en = timing_edge(cum, i + 1, a.fine_hop, keep) + P;
        }
        marks[2 * i] = st;
        marks[2 * i + 1] = en;
    }
    if (tid == 0) {
        a.verdict[2 * b] = 0; a.verdict[2 * b + 1] = 0;
        a.rowinfo[2 * b] = keep; a.rowinfo[2 * b + 1] = keep + total;
        a.out_lengths[b] = keep + total;
    }
}

__global__ __launch_bounds__(256) void wave_breaks_kernel(const WaveBreaksArgs a) {
    const int b = blockIdx.y, tid = threadIdx.x;
    const int64_t keep = a.rowinfo[2 * b], total = a.rowinfo[2 * b + 1];   // -1: refused, the row becomes zeros
    const int64_t j0 = (int64_t)blockIdx.x * BREAKS_TILE;
    float* orow = a.out + (size_t)b * a.out_ld;
    f32x4 v[BREAKS_TILE / 1024];
#pragma unroll
    for (int q = 0; q < BREAKS_TILE / 1024; ++q) v[q] = f32x4{0.f, 0.f, 0.f, 0.f};
    // (workgroup-uniform.  The plan in the workspace is that of this batch and break_first[b .. b + 1] passed it; the gather still
    // holds every index it forms inside the workspace and inside [0, keep) of its row, whatever the workspace holds)
    const bool planned = a.header[0] == a.B && a.header[5] == a.NB && keep >= 0 && keep <= a.ld;
    const int k0 = planned && a.break_first ? a.break_first[b] : 0, nb = planned && a.break_first ? a.break_first[b + 1] - k0 : 0;
    if (planned && j0 < total && k0 >= 0 && nb >= 0 && (int64_t)k0 + nb <= a.NB) {
        const float* arow = a.audio + (size_t)b * a.ld;
        const int64_t* cut = a.cut + k0;
        const int64_t* ost = a.ostart + k0;
#pragma unroll
        for (int q = 0; q < BREAKS_TILE / 1024; ++q) {
            const int64_t j = j0 + q * 1024 + 4 * tid;
            if (j >= total) continue;
            int s = timing_lower(ost, nb, j + 1);                     // segment s lies behind break s - 1: the breaks with ostart <= j
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int64_t jj = j + e;
                if (jj >= total) break;
                while (s < nb && ost[s] <= jj) ++s;
                const int64_t p = s ? cut[s - 1] : 0, o = s ? ost[s - 1] : 0, pe = s < nb ? cut[s] : keep;
                const int64_t i = jj - o, n = pe - p;                 // the segment is audio[p .. pe); behind it, its break's pause
                float x = 0.f;
                if (i >= 0 && i < n && p >= 0 && p + i < keep) {
                    x = arow[p + i];
                    const int64_t F = a.fade < n / 2 ? a.fade : n / 2;
                    if (p > 0 && i < F) x = x * ((float)(2 * i + 1) / (float)(2 * F));
                    else if (pe < keep && n - 1 - i < F) x = x * ((float)(2 * (n - 1 - i) + 1) / (float)(2 * F));
                }
                v[q][e] = x;
            }
        }
    }
#pragma unroll
    for (int q = 0; q < BREAKS_TILE / 1024; ++q) {
        const int64_t j = j0 + q * 1024 + 4 * tid;                    // out_ld % 4 == 0: a quad is inside the row or outside
        if (j < a.out_ld) *reinterpret_cast<f32x4*>(orow + j) = v[q];
    }
}

hipError_t launch_token_timing(const TimingArgs& a, hipStream_t s) {
    if (!a.cum || !a.x_len || !a.keep || !a.marks || !a.out_lengths || !a.header || !a.verdict || !a.rowinfo) return hipErrorInvalidValue;
    if (a.B <= 0 || a.B > 65535 || a.Tx <= 0 || a.fine_hop <= 0 || a.NB < 0 || a.NB > (1 << 27)) return hipErrorInvalidValue;
    if (a.break_first && (!a.break_token || !a.break_pause || !a.cut || !a.ostart)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(token_timing_kernel, dim3(a.B), dim3(256), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_wave_breaks(const WaveBreaksArgs& a, hipStream_t s) {
    if (!a.audio || !a.out || !a.header || !a.rowinfo || (a.break_first && (!a.cut || !a.ostart))) return hipErrorInvalidValue;
    if (a.B <= 0 || a.B > 65535 || a.ld < 4 || a.out_ld < 4 || (a.ld & 3) || (a.out_ld & 3) || a.fade < 0) return hipErrorInvalidValue;
    if ((reinterpret_cast<uintptr_t>(a.audio) & 15) || (reinterpret_cast<uintptr_t>(a.out) & 15)) return hipErrorInvalidValue;
    const int64_t tiles = (a.out_ld + BREAKS_TILE - 1) / BREAKS_TILE;
    if (tiles > 0x7fffffff) return hipErrorInvalidValue;
    hipLaunchKernelGGL(wave_breaks_kernel, dim3((unsigned)tiles, a.B), dim3(256), 0, s, a);
    return hipGetLastError();
}

// The workspace both entries carve the same way: header + verdicts (one block, what the status entry copies), the plan of the rows,
// the plan of the breaks
struct TimingWs {
    int64_t *header, *verdict, *rowinfo, *cut, *ostart;
    size_t bytes;
    bool overflow;
};
static TimingWs timing_carve(void* d_ws, size_t cap, int64_t B, int64_t NB) {
    WS ws(d_ws, cap);
    TimingWs t;
    t.header = static_cast<int64_t*>(ws.bytes(256 + (size_t)B * 2 * sizeof(int64_t)));
    t.verdict = t.header ? t.header + 32 : nullptr;
    t.rowinfo = static_cast<int64_t*>(ws.bytes((size_t)B * 2 * sizeof(int64_t)));
    t.cut = static_cast<int64_t*>(ws.bytes((size_t)(NB > 0 ? NB : 1) * sizeof(int64_t)));
    t.ostart = static_cast<int64_t*>(ws.bytes((size_t)(NB > 0 ? NB : 1) * sizeof(int64_t)));
    t.bytes = ws.off + 256;
    t.overflow = ws.overflow || cap < 256;
    return t;
}

}  // namespace mtts

using namespace mtts;

extern "C" {

// ---- token timing (timing.hip)
int64_t mtts_token_timing_workspace_bytes(int64_t B, int64_t NB) {
    if (B < 1 || B > 65535 || NB < 0 || NB > (1 << 27)) { set_error("mtts_token_timing_workspace_bytes: need 1 <= B <= 65535 and 0 <= NB <= 2^27"); return -1; }
    return (int64_t)timing_carve(nullptr, 0, B, NB).bytes;
}

int mtts_token_timing(const int32_t* d_cum, const int64_t* d_x_lengths, const int64_t* d_keep, int B, int Tx, int fine_hop, int64_t keep_max,
                      const int32_t* d_break_first, const int32_t* d_break_token, const int64_t* d_break_pause, int64_t NB, int64_t pause_max,
                      int64_t out_max, int64_t* d_marks, int64_t* d_out_lengths, void* d_ws, int64_t ws_bytes, void* stream) {
    if (!d_cum || !d_x_lengths || !d_keep || !d_marks || !d_out_lengths || !d_ws) { set_error("mtts_token_timing: null argument"); return -1; }
    if (d_break_first && (!d_break_token || !d_break_pause)) { set_error("mtts_token_timing: null argument (breaks without tokens or pauses)"); return -1; }
    if (B < 1 || B > 65535 || Tx < 1) { set_error("mtts_token_timing: need 1 <= B <= 65535 and Tx >= 1"); return -1; }
    if (fine_hop < 2 || (fine_hop & 1) || fine_hop > 65536) { set_error("mtts_token_timing: fine_hop must be even, inside [2, 65536]"); return -1; }
    if (NB < 0 || NB > (1 << 27) || (!d_break_first && NB != 0)) { set_error("mtts_token_timing: need 0 <= NB <= 2^27 (0 without breaks)"); return -1; }
    if (keep_max < 0 || out_max < keep_max || pause_max < 0 || out_max > (int64_t)1 << 40 || pause_max > (int64_t)1 << 40) {
        set_error("mtts_token_timing: need 0 <= keep_max <= out_max <= 2^40 and 0 <= pause_max <= 2^40");
        return -1;
    }
    if (reinterpret_cast<uintptr_t>(d_ws) & 15) { set_error("mtts_token_timing: the workspace must be 16-byte aligned"); return -1; }
    const TimingWs t = timing_carve(d_ws, (size_t)(ws_bytes > 0 ? ws_bytes : 0), B, NB);
    if (t.overflow) { set_error("mtts_token_timing: workspace too small (mtts_token_timing_workspace_bytes)"); return -1; }
    TimingArgs a;
    a.cum = d_cum; a.x_len = d_x_lengths; a.keep = d_keep; a.B = B; a.Tx = Tx; a.fine_hop = fine_hop;
    a.keep_max = keep_max; a.out_max = out_max; a.pause_max = pause_max;
    a.break_first = d_break_first; a.break_token = d_break_token; a.break_pause = d_break_pause; a.NB = (int)NB;
    a.marks = d_marks; a.out_lengths = d_out_lengths;
    a.header = t.header; a.verdict = t.verdict; a.rowinfo = t.rowinfo; a.cut = t.cut; a.ostart = t.ostart;
    HIP_OK(launch_token_timing(a, static_cast<hipStream_t>(stream)));
    return 0;
}

// The verdict of the latest mtts_token_timing on this workspace: the first refused row.  Waits for the stream.
int mtts_token_timing_status(const void* d_ws, int B, void* stream) {
    if (B < 1 || B > 65535) { set_error("mtts_token_timing_status: need 1 <= B <= 65535"); return -1; }
    std::vector<int64_t> w(32 + 2 * (size_t)B);
    if (read_status("mtts_token_timing_status", d_ws, stream, w.data(), w.size())) return -1;
    if (w[0] != B) { set_error("mtts_token_timing_status: the workspace holds the verdict of another batch size"); return -1; }
    for (int b = 0; b < B; ++b) {
        const int64_t reason = w[32 + 2 * b], v = w[33 + 2 * b];
        if (reason == 0) continue;
        const std::string row = "mtts_token_timing: row " + std::to_string(b) + " is refused: ";
        if (reason == 1) set_error(row + "its kept length " + std::to_string(v) + " is outside [0, " + std::to_string(w[2]) + "]");
        else if (reason == 5) set_error(row + "its token count " + std::to_string(v) + " is outside [1, Tx = " + std::to_string(w[1]) + "]");
        else if (reason == 2 && v < 0) set_error(row + "break_first does not ascend inside [0, NB]");
        else if (reason == 2) set_error(row + "break " + std::to_string(v) + " names a token outside [0, x_length)");
        else if (reason == 3) set_error(row + "break " + std::to_string(v) + " does not follow a later token than the break before it");
        else if (reason == 4) set_error(row + "the pause of break " + std::to_string(v) + " is outside [0, " + std::to_string(w[3]) + "]");
        else if (reason == 6) set_error(row + "the cumulative durations decrease at break " + std::to_string(v));
        else set_error(row + "its lengthened row of " + std::to_string(v) + " samples does not fit " + std::to_string(w[4]));
        return -1;
    }
    return 0;
}

int mtts_wave_breaks(const float* d_audio, int64_t ld, const int32_t* d_break_first, int B, int64_t NB, int64_t fade, float* d_out,
                     int64_t out_ld, const void* d_ws, int64_t ws_bytes, void* stream) {
    if (!d_audio || !d_out || !d_ws) { set_error("mtts_wave_breaks: null argument"); return -1; }
    if (B < 1 || B > 65535) { set_error("mtts_wave_breaks: need 1 <= B <= 65535"); return -1; }
    if (NB < 0 || NB > (1 << 27) || (!d_break_first && NB != 0)) { set_error("mtts_wave_breaks: need 0 <= NB <= 2^27 (0 without breaks)"); return -1; }
    if (ld < 4 || out_ld < 4 || (ld & 3) || (out_ld & 3) || (reinterpret_cast<uintptr_t>(d_audio) & 15) || (reinterpret_cast<uintptr_t>(d_out) & 15) ||
        (reinterpret_cast<uintptr_t>(d_ws) & 15)) {
        set_error("mtts_wave_breaks: rows must be 16-byte aligned (ld and out_ld positive multiples of 4 samples)");
        return -1;
    }
    if (ld > (int64_t)1 << 40 || out_ld > (int64_t)1 << 40) { set_error("mtts_wave_breaks: a row of more than 2^40 samples"); return -1; }
    if (fade < 0) { set_error("mtts_wave_breaks: fade must not be negative"); return -1; }
    const uintptr_t in0 = reinterpret_cast<uintptr_t>(d_audio), in1 = in0 + (uintptr_t)B * ld * sizeof(float);
    const uintptr_t out0 = reinterpret_cast<uintptr_t>(d_out), out1 = out0 + (uintptr_t)B * out_ld * sizeof(float);
    if (in0 < out1 && out0 < in1) { set_error("mtts_wave_breaks: the gather is not in place (d_out overlaps d_audio)"); return -1; }
    const TimingWs t = timing_carve(const_cast<void*>(d_ws), (size_t)(ws_bytes > 0 ? ws_bytes : 0), B, NB);
    if (t.overflow) { set_error("mtts_wave_breaks: workspace too small (mtts_token_timing_workspace_bytes)"); return -1; }
    WaveBreaksArgs a;
    a.audio = d_audio; a.ld = ld; a.break_first = d_break_first; a.B = B; a.fade = fade; a.out = d_out; a.out_ld = out_ld;
    a.NB = (int)NB; a.header = t.header; a.rowinfo = t.rowinfo; a.cut = t.cut; a.ostart = t.ostart;
    HIP_OK(launch_wave_breaks(a, static_cast<hipStream_t>(stream)));
    return 0;
}

}  // extern "C"
