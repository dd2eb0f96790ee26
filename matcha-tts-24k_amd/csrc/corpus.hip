// Corpus preparation for a ragged batch (gfx950): what the reference does to one file at a time on the host before training --
//   * silence bounds and run lengths  (reference matcha/utils/measure_silence.py:66-132, normalize_silence.py:86-136),
//   * the rebuild [leading] + content + [trailing]  (reference matcha/utils/normalize_silence.py:157-220),
//   * the per-file mel sums behind mel_mean / mel_std  (reference matcha/utils/generate_data_statistics.py:120-131) --
// as streaming launches over rows of audio [B][ld] (or mel [B][F][T]):
//   1. sil_rms_kernel   (32 windows, row): root mean square of every 10 ms window, the last partial one included (its sum runs
//                       over the samples that exist and is divided by the whole window: the reference pads with zeros)
//   2. sil_scan_kernel  (row): first / last window at or above the effective threshold, leading / trailing runs below each threshold
//   3. sil_norm_kernel  (output tile, row): the rebuilt row; every output sample is in[j + d] with ONE shift d per row, or zero
//   4. mel_part_kernel  (chunk of 256 frames, clip) and mel_total_kernel (clip): sum x, sum x^2 in fp64 and the non-finite flag
// A row is spread over the grid, never owned by one workgroup (a clip can be minutes long and B can be 1, see waveform.hip); 16
// bytes per lane where the window length allows, 4 bytes otherwise.  The window arithmetic is wave_scale_rms_kernel's: exact
// squares summed in fp64 as lane-strided partials and an xor-shuffle tree, so two runs give the same bits and a clip's numbers
// do not depend on its batch.  Lengths are read on the device only; nothing is read outside [0, len_b) of a row.
#include "host.h"
#include "device_utils.h"

#include <cfloat>

namespace mtts {

using f32x4 = __attribute__((ext_vector_type(4))) float;
typedef float f32x4_a4 __attribute__((ext_vector_type(4), aligned(4)));      // a quad at any sample offset of a row

__device__ __forceinline__ double corpus_sum_d(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
__device__ __forceinline__ int corpus_min_i(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o));
    return v;
}
__device__ __forceinline__ int corpus_max_i(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o));
    return v;
}

// The verdict on every row, by one workgroup: status[0] = first refused row + 1, [1] its length, [4] the entry that ran.
template <class Refused>
__device__ __forceinline__ void corpus_verdict(int B, const int64_t* lengths, int64_t* status, int64_t s2, int64_t s3, int64_t entry, Refused refused) {
    const int i = first_refused_row(B, refused);
    if (threadIdx.x == 0) {
        status[0] = i < B ? i + 1 : 0;
        status[1] = i < B ? lengths[i] : 0;
        status[2] = s2;
        status[3] = s3;
        status[4] = entry;
    }
}

// ------------------------------------------------------------------------------------------------ silence: window RMS
constexpr int SIL_WIN_PER_WG = 32;    // 4 waves x 8 windows

// VEC = 4: win % 4 == 0, a lane moves 16 bytes (a window starts on a quad of the row); VEC = 1: any window length
template <int VEC>
__global__ __launch_bounds__(256) void sil_rms_kernel(const SilenceMeasureArgs p) {
    const int b = blockIdx.y, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t L = p.lengths[b];
    if (L <= 0 || L > p.ld) return;
    const int64_t n_win = (L + p.win - 1) / p.win;
    const int64_t w0 = (int64_t)blockIdx.x * SIL_WIN_PER_WG + wave * 8;
    const float* row = p.audio + (size_t)b * p.ld;
    for (int k = 0; k < 8; ++k) {
        const int64_t w = w0 + k;
        if (w >= n_win) break;                                  // wave-uniform
        const int64_t base = w * p.win;
        double q = 0.0;
        for (int e = lane * VEC; e < p.win; e += 64 * VEC) {
            const int64_t i = base + e;
            if (i >= L) break;
            if constexpr (VEC == 4) {
                if (i + 4 <= L) {
                    const f32x4 v = *reinterpret_cast<const f32x4*>(row + i);
#pragma unroll
                    for (int j = 0; j < 4; ++j) q += (double)v[j] * (double)v[j];
                } else {
                    for (int j = 0; j < 4 && i + j < L; ++j) {
                        const float v = row[i + j];
                        q += (double)v * (double)v;
                    }
                }
            } else {
                const float v = row[i];
                q += (double)v * (double)v;
            }
        }
        q = corpus_sum_d(q);
        if (lane == 0) p.rms[(size_t)b * p.nwin_max + w] = (float)sqrt(q / (double)p.win);
    }
}

// `rms >= thr` is content, `rms < thr` is silence; a NaN window is neither: it starts no content and ends a silent run
__global__ __launch_bounds__(256) void sil_scan_kernel(const SilenceMeasureArgs p) {
    __shared__ int part[4][6];
    const int b = blockIdx.x, tid = threadIdx.x;
    if (b == 0)
        corpus_verdict(p.B, p.lengths, p.status, p.ld, 0, 1, [&](int i) { const int64_t n = p.lengths[i]; return n < 0 || n > p.ld; });
    const int64_t L = p.lengths[b];
    int64_t* o = p.out + (size_t)b * 6;
    if (L < 0 || L > p.ld) {
        if (tid < 6) o[tid] = -1;
        return;
    }
    const int n_win = (int)((L + p.win - 1) / p.win);
    int first_act = n_win, first_eff = n_win, first_abs = n_win;       // smallest window: at or above eff; not below eff; not below abs
    int last_act = -1, last_eff = -1, last_abs = -1;                    // largest such window
    const float* rms = p.rms + (size_t)b * p.nwin_max;
    for (int w = tid; w < n_win; w += 256) {
        const float r = rms[w];
        if (r >= p.thr_eff) { first_act = min(first_act, w); last_act = w; }
        if (!(r < p.thr_eff)) { first_eff = min(first_eff, w); last_eff = w; }
        if (!(r < p.thr_abs)) { first_abs = min(first_abs, w); last_abs = w; }
    }
    first_act = corpus_min_i(first_act); first_eff = corpus_min_i(first_eff); first_abs = corpus_min_i(first_abs);
    last_act = corpus_max_i(last_act); last_eff = corpus_max_i(last_eff); last_abs = corpus_max_i(last_abs);
    if ((tid & 63) == 0) {
        int* q = part[tid >> 6];
        q[0] = first_act; q[1] = first_eff; q[2] = first_abs; q[3] = last_act; q[4] = last_eff; q[5] = last_abs;
    }
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < 4; ++w) {
            first_act = min(first_act, part[w][0]); first_eff = min(first_eff, part[w][1]); first_abs = min(first_abs, part[w][2]);
            last_act = max(last_act, part[w][3]); last_eff = max(last_eff, part[w][4]); last_abs = max(last_abs, part[w][5]);
        }
        const int64_t W = p.win;
        const int64_t end = (int64_t)(last_act + 1) * W;
        o[0] = last_act >= 0 ? (int64_t)first_act * W : 0;
        o[1] = last_act >= 0 ? (end < L ? end : L) : 0;
        o[2] = (int64_t)first_eff * W;
        o[3] = (int64_t)first_abs * W;
        o[4] = (int64_t)(n_win - 1 - last_eff) * W;
        o[5] = (int64_t)(n_win - 1 - last_abs) * W;
    }
}

hipError_t launch_silence_measure(const SilenceMeasureArgs& a, hipStream_t s) {
    if (!a.audio || !a.lengths || !a.out || !a.status || !a.rms) return hipErrorInvalidValue;
    if (a.B <= 0 || a.B > 65535 || a.ld < 4 || (a.ld & 3) || (reinterpret_cast<uintptr_t>(a.audio) & 15) || a.win <= 0) return hipErrorInvalidValue;
    if (a.nwin_max < 1 || (int64_t)a.nwin_max * a.win < a.ld) return hipErrorInvalidValue;
    const unsigned nwg = (unsigned)((a.nwin_max + SIL_WIN_PER_WG - 1) / SIL_WIN_PER_WG);
    if (a.win % 4 == 0)
        hipLaunchKernelGGL(sil_rms_kernel<4>, dim3(nwg, a.B), dim3(256), 0, s, a);
    else
        hipLaunchKernelGGL(sil_rms_kernel<1>, dim3(nwg, a.B), dim3(256), 0, s, a);
    hipLaunchKernelGGL(sil_scan_kernel, dim3(a.B), dim3(256), 0, s, a);
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------ silence: the rebuild
// What row b becomes.  Output sample j is in[j + d] for j in [lo, hi) and zero elsewhere; out_len = -1 refuses the row.
struct NormPlan {
    int64_t out_len, d, lo, hi, L;
    int changed;
};
__device__ __forceinline__ NormPlan norm_plan(const SilenceNormArgs& a, int b) {
    NormPlan r{-1, 0, 0, 0, 0, 0};
    const int64_t L = a.lengths[b], cs = a.bounds[(size_t)b * 6], ce = a.bounds[(size_t)b * 6 + 1];
    r.L = L;
    if (L < 0 || L > a.ld_in || cs < 0 || ce < cs || ce > L) return r;
    const int64_t cur_trail = L - ce, body = ce - cs;               // current_leading = cs: the reference's integer comparison
    const bool lead_ok = a.lead < 0 || cs == a.lead, trail_ok = a.trail < 0 || cur_trail == a.trail;
    const bool same = lead_ok && trail_ok;
    const bool lead_src = same || a.lead < 0, trail_src = same || a.trail < 0;
    const int64_t lead_n = lead_src ? cs : a.lead, trail_n = trail_src ? cur_trail : a.trail;
    const int64_t out_len = lead_n + body + trail_n;
    if (out_len > a.ld_out) return r;
    r.out_len = out_len;
    r.changed = same ? 0 : 1;
    r.d = cs - lead_n;
    r.lo = lead_src ? 0 : lead_n;
    r.hi = trail_src ? out_len : lead_n + body;
    return r;
}

__global__ __launch_bounds__(256) void sil_norm_kernel(const SilenceNormArgs a) {
    const int b = blockIdx.y, tid = threadIdx.x;
    if (blockIdx.x == 0 && b == 0)
        corpus_verdict(a.B, a.lengths, a.status, a.ld_in, a.ld_out, 2, [&](int i) { return norm_plan(a, i).out_len < 0; });
    const NormPlan p = norm_plan(a, b);
    if (blockIdx.x == 0 && tid == 0) {
        a.out_lengths[b] = p.out_len;
        a.changed[b] = p.changed;
    }
    const float* src = a.in + (size_t)b * a.ld_in + p.d;            // (dereferenced only at j in [lo, hi): j + d inside [0, L))
    float* orow = a.out + (size_t)b * a.ld_out;
    const bool aligned = (p.d & 3) == 0;
    const int64_t j0 = (int64_t)blockIdx.x * SIL_NORM_TILE;
#pragma unroll
    for (int r = 0; r < SIL_NORM_TILE / 1024; ++r) {
        const int64_t j = j0 + r * 1024 + 4 * tid;                  // ld_out % 4 == 0: a quad is inside the row or outside
        if (j >= a.ld_out) break;
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (j >= p.lo && j + 4 <= p.hi) {                           // (an empty or refused row has hi = 0)
            if (aligned) v = *reinterpret_cast<const f32x4*>(src + j);
            else v = *reinterpret_cast<const f32x4_a4*>(src + j);
        } else if (j < p.hi && j + 4 > p.lo) {
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (j + e >= p.lo && j + e < p.hi) v[e] = src[j + e];
        }
        *reinterpret_cast<f32x4*>(orow + j) = v;
    }
}

hipError_t launch_silence_normalize(const SilenceNormArgs& a, hipStream_t s) {
    if (!a.in || !a.lengths || !a.bounds || !a.out || !a.out_lengths || !a.changed || !a.status) return hipErrorInvalidValue;
    if (a.B <= 0 || a.B > 65535 || a.ld_in < 4 || a.ld_out < 4 || (a.ld_in & 3) || (a.ld_out & 3)) return hipErrorInvalidValue;
    if ((reinterpret_cast<uintptr_t>(a.in) & 15) || (reinterpret_cast<uintptr_t>(a.out) & 15)) return hipErrorInvalidValue;
    const unsigned tiles = (unsigned)((a.ld_out + SIL_NORM_TILE - 1) / SIL_NORM_TILE);
    hipLaunchKernelGGL(sil_norm_kernel, dim3(tiles, a.B), dim3(256), 0, s, a);
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------ mel sums
// Chunk c of clip b: thread i owns frame t = 256 c + i and adds its F values in ascending f (fp64; x and x * x are exact there);
// the 256 threads' sums meet in an xor-shuffle tree per wave and as ((w0 + w1) + w2) + w3 across the waves.
__global__ __launch_bounds__(MEL_STATS_CHUNK) void mel_part_kernel(const MelStatsArgs a) {
    __shared__ double ws[4], wq[4];
    __shared__ int wb[4];
    const int b = blockIdx.y, c = blockIdx.x, tid = threadIdx.x;
    const int64_t len = a.lengths[b];
    if (len < 0 || len > a.T || (int64_t)c * MEL_STATS_CHUNK >= len) return;      // (mel_total_kernel reads the used chunks only)
    const int64_t t = (int64_t)c * MEL_STATS_CHUNK + tid;
    double s = 0.0, q = 0.0;
    bool bad = false;
    if (t < len) {
        const float* x = a.mel + (size_t)b * a.F * a.T + t;
#pragma unroll 4
        for (int f = 0; f < a.F; ++f) {
            const float v = x[(size_t)f * a.T];
            bad |= !(fabsf(v) <= FLT_MAX);
            s += (double)v;
            q += (double)v * (double)v;
        }
    }
    s = corpus_sum_d(s);
    q = corpus_sum_d(q);
    const bool any_bad = __any(bad);
    if ((tid & 63) == 0) { ws[tid >> 6] = s; wq[tid >> 6] = q; wb[tid >> 6] = any_bad ? 1 : 0; }
    __syncthreads();
    if (tid == 0) {
        const size_t at = (size_t)b * a.nchunks + c;
        a.part[2 * at] = ((ws[0] + ws[1]) + ws[2]) + ws[3];
        a.part[2 * at + 1] = ((wq[0] + wq[1]) + wq[2]) + wq[3];
        a.part_flag[at] = wb[0] | wb[1] | wb[2] | wb[3];
    }
}

// The chunks of a clip in ascending order, by one thread
__global__ __launch_bounds__(256) void mel_total_kernel(const MelStatsArgs a) {
    if (blockIdx.x == 0)
        corpus_verdict(a.B, a.lengths, a.status, a.T, 0, 3, [&](int i) { const int64_t n = a.lengths[i]; return n < 0 || n > a.T; });
    const int b = blockIdx.x * 256 + threadIdx.x;
    if (b >= a.B) return;
    const int64_t len = a.lengths[b];
    double s = 0.0, q = 0.0;
    int flag = 0;
    const bool ok = len >= 0 && len <= a.T;
    if (ok) {
        const int used = (int)((len + MEL_STATS_CHUNK - 1) / MEL_STATS_CHUNK);
        for (int c = 0; c < used; ++c) {
            const size_t at = (size_t)b * a.nchunks + c;
            s += a.part[2 * at];
            q += a.part[2 * at + 1];
            flag |= a.part_flag[at];
        }
    }
    a.sums[2 * (size_t)b] = s;
    a.sums[2 * (size_t)b + 1] = q;
    a.frames[b] = ok ? len : -1;
    a.flags[b] = flag;
}

hipError_t launch_mel_stats(const MelStatsArgs& a, hipStream_t s) {
    if (!a.mel || !a.lengths || !a.sums || !a.frames || !a.flags || !a.status || !a.part || !a.part_flag) return hipErrorInvalidValue;
    if (a.B <= 0 || a.B > 65535 || a.F < 1 || a.T < 1 || a.nchunks != (a.T + MEL_STATS_CHUNK - 1) / MEL_STATS_CHUNK) return hipErrorInvalidValue;
    hipLaunchKernelGGL(mel_part_kernel, dim3(a.nchunks, a.B), dim3(MEL_STATS_CHUNK), 0, s, a);
    hipLaunchKernelGGL(mel_total_kernel, dim3((a.B + 255) / 256), dim3(256), 0, s, a);
    return hipGetLastError();
}

}  // namespace mtts

using namespace mtts;

static int corpus_window(int sample_rate) { return (int)(0.01 * (double)sample_rate); }      // reference measure_silence.py:94

// The verdict of a call's lengths check (the header of its workspace); the caller names the entry that ran
static int corpus_status(const char* who, const void* d_ws, void* stream) {
    int64_t st[5];
    if (read_status(who, d_ws, stream, st)) return -1;
    if (st[0] == 0) return 0;
    const std::string row = "row " + std::to_string(st[0] - 1) + " has length " + std::to_string(st[1]);
    if (st[4] == 1) set_error("mtts_silence_measure: " + row + " (need 0 <= length <= ld = " + std::to_string(st[2]) + ")");
    else if (st[4] == 2)
        set_error("mtts_silence_normalize: " + row + " (need 0 <= length <= ld_in = " + std::to_string(st[2]) + ", bounds 0 <= content_start <= "
                  "content_end <= length, and a rebuilt length <= ld_out = " + std::to_string(st[3]) + ")");
    else set_error("mtts_mel_stats: " + row + " (need 0 <= frames <= T = " + std::to_string(st[2]) + ")");
    return -1;
}

extern "C" {

// ---- corpus preparation (corpus.hip)
int mtts_silence_window(int sample_rate) { return corpus_window(sample_rate); }

int64_t mtts_silence_workspace_bytes(int64_t ld, int B, int sample_rate) {
    const int win = corpus_window(sample_rate);
    if (ld < 4 || B <= 0 || win <= 0) { set_error("mtts_silence_workspace_bytes: bad shape"); return -1; }
    WS ws(nullptr, 0);
    ws.bytes(256);
    ws.f((size_t)B * ((ld + win - 1) / win));
    return (int64_t)ws.off + 256;
}

int mtts_silence_measure(const float* d_audio, int64_t ld, const int64_t* d_lengths, int B, int sample_rate, double effective_db,
                         double absolute_db, int64_t* d_out, void* d_ws, int64_t ws_bytes, void* stream) {
    if (!d_audio || !d_lengths || !d_out || !d_ws) { set_error("mtts_silence_measure: null argument"); return -1; }
    if (B < 1 || B > 65535) { set_error("mtts_silence_measure: B must lie in [1, 65535]"); return -1; }
    SilenceMeasureArgs a;
    a.win = corpus_window(sample_rate);
    if (a.win <= 0) { set_error("mtts_silence_measure: sample_rate must be at least 100 Hz (a 10 ms window of one sample)"); return -1; }
    if (ld < 4 || (ld & 3) || (reinterpret_cast<uintptr_t>(d_audio) & 15) || (reinterpret_cast<uintptr_t>(d_ws) & 15)) {
        set_error("mtts_silence_measure: rows must be 16-byte aligned (ld a positive multiple of 4 samples)");
        return -1;
    }
    if ((ld + a.win - 1) / a.win > 0x3fffffff) { set_error("mtts_silence_measure: too many windows in a row"); return -1; }
    a.nwin_max = (int)((ld + a.win - 1) / a.win);
    WS ws(d_ws, (size_t)ws_bytes);
    a.status = static_cast<int64_t*>(ws.bytes(256));
    a.rms = ws.f((size_t)B * a.nwin_max);
    if (ws_bytes < 256 || ws.overflow) { set_error("mtts_silence_measure: workspace too small (mtts_silence_workspace_bytes)"); return -1; }
    a.audio = d_audio; a.ld = ld; a.lengths = d_lengths; a.B = B; a.out = d_out;
    a.thr_eff = (float)std::pow(10.0, effective_db / 20.0);     // reference measure_silence.py:90-91; torch compares the fp32 RMS in fp32
    a.thr_abs = (float)std::pow(10.0, absolute_db / 20.0);
    HIP_OK(launch_silence_measure(a, static_cast<hipStream_t>(stream)));
    return 0;
}

int mtts_silence_normalize(const float* d_in, int64_t ld_in, const int64_t* d_lengths, const int64_t* d_bounds, int B, int sample_rate,
                           int64_t lead_target, int64_t trail_target, float* d_out, int64_t ld_out, int64_t* d_out_lengths,
                           int32_t* d_changed, void* d_ws, int64_t ws_bytes, void* stream) {
    if (!d_in || !d_lengths || !d_bounds || !d_out || !d_out_lengths || !d_changed || !d_ws) { set_error("mtts_silence_normalize: null argument"); return -1; }
    if (B < 1 || B > 65535) { set_error("mtts_silence_normalize: B must lie in [1, 65535]"); return -1; }
    const int win = corpus_window(sample_rate);
    if (win <= 0) { set_error("mtts_silence_normalize: sample_rate must be at least 100 Hz (a 10 ms window of one sample)"); return -1; }
    if (ld_in < 4 || ld_out < 4 || (ld_in & 3) || (ld_out & 3) || (reinterpret_cast<uintptr_t>(d_in) & 15) || (reinterpret_cast<uintptr_t>(d_out) & 15) ||
        (reinterpret_cast<uintptr_t>(d_ws) & 15)) {
        set_error("mtts_silence_normalize: rows must be 16-byte aligned (ld_in and ld_out positive multiples of 4 samples)");
        return -1;
    }
    if (d_out == d_in) { set_error("mtts_silence_normalize: the rebuild is not in place (d_out == d_in)"); return -1; }
    for (const int64_t t : {lead_target, trail_target})            // reference normalize_silence.py:139-154
        if (t < -1 || (t > 0 && t % win != 0)) {
            set_error("mtts_silence_normalize: a target must be -1 (keep that end) or a whole multiple of the 10 ms window (" + std::to_string(win) +
                      " samples), got " + std::to_string(t));
            return -1;
        }
    if (ws_bytes < 256) { set_error("mtts_silence_normalize: workspace too small (mtts_silence_workspace_bytes)"); return -1; }
    SilenceNormArgs a;
    a.in = d_in; a.ld_in = ld_in; a.ld_out = ld_out; a.lengths = d_lengths; a.bounds = d_bounds; a.B = B;
    a.lead = lead_target; a.trail = trail_target; a.out = d_out; a.out_lengths = d_out_lengths; a.changed = d_changed;
    a.status = static_cast<int64_t*>(d_ws);
    HIP_OK(launch_silence_normalize(a, static_cast<hipStream_t>(stream)));
    return 0;
}

// The lengths check's verdict of the latest measure / normalize call on this workspace.  Waits for the stream.
int mtts_silence_status(const void* d_ws, void* stream) { return corpus_status("mtts_silence_status", d_ws, stream); }

int mtts_mel_stats_chunk(void) { return MEL_STATS_CHUNK; }

int64_t mtts_mel_stats_workspace_bytes(int B, int T) {
    if (B <= 0 || T <= 0) { set_error("mtts_mel_stats_workspace_bytes: bad shape"); return -1; }
    const size_t n = (size_t)B * ((T + MEL_STATS_CHUNK - 1) / MEL_STATS_CHUNK);
    WS ws(nullptr, 0);
    ws.bytes(256);
    ws.bytes(n * 2 * sizeof(double));
    ws.bytes(n * sizeof(int32_t));
    return (int64_t)ws.off + 256;
}

int mtts_mel_stats(const float* d_mel, int F, int T, const int64_t* d_lengths, int B, double* d_sums, int64_t* d_frames, int32_t* d_flags,
                   void* d_ws, int64_t ws_bytes, void* stream) {
    if (!d_mel || !d_lengths || !d_sums || !d_frames || !d_flags || !d_ws) { set_error("mtts_mel_stats: null argument"); return -1; }
    if (B < 1 || B > 65535) { set_error("mtts_mel_stats: B must lie in [1, 65535]"); return -1; }
    if (F < 1 || T < 1) { set_error("mtts_mel_stats: F and T must be at least 1"); return -1; }
    if (reinterpret_cast<uintptr_t>(d_ws) & 15) { set_error("mtts_mel_stats: misaligned workspace (16 bytes)"); return -1; }
    MelStatsArgs a;
    a.nchunks = (T + MEL_STATS_CHUNK - 1) / MEL_STATS_CHUNK;
    const size_t n = (size_t)B * a.nchunks;
    WS ws(d_ws, (size_t)ws_bytes);
    a.status = static_cast<int64_t*>(ws.bytes(256));
    a.part = static_cast<double*>(ws.bytes(n * 2 * sizeof(double)));
    a.part_flag = static_cast<int32_t*>(ws.bytes(n * sizeof(int32_t)));
    if (ws_bytes < 256 || ws.overflow) { set_error("mtts_mel_stats: workspace too small (mtts_mel_stats_workspace_bytes)"); return -1; }
    a.mel = d_mel; a.lengths = d_lengths; a.B = B; a.F = F; a.T = T; a.sums = d_sums; a.frames = d_frames; a.flags = d_flags;
    HIP_OK(launch_mel_stats(a, static_cast<hipStream_t>(stream)));
    return 0;
}

int mtts_mel_stats_status(const void* d_ws, void* stream) { return corpus_status("mtts_mel_stats_status", d_ws, stream); }

}  // extern "C"
