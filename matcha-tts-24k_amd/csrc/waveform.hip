// Waveform finish for a ragged batch (gfx950): what the reference does to one utterance on the host after the vocoder --
// peak normalisation (reference matcha/inference.py:260-264, to_waveform) and the trailing-silence trim length
// (reference matcha/inference.py:268-287, trim_trailing_silence) -- for every row of audio [B][ld] in three grid passes:
//   1. wave_peak_kernel      (chunk, row): max |a| of WAVE_CHUNK samples                       -> peaks[row][chunk]
//   2. wave_scale_rms_kernel (32 windows, row): row peak from the chunk peaks; if it is above 1 every valid sample becomes
//                            a / peak * 0.95 in place; root mean square of every full 10 ms window -> rms[row][window]
//   3. wave_trim_kernel      (row): trailing run of windows with rms < threshold              -> out_lengths[row]
// Streaming passes (the audio is read twice and written at most once, 16 bytes per lane where the window length allows); a row
// is spread over the grid, never owned by one workgroup (an utterance can be 1.8 M samples and B can be 1).
// Every reduction has a fixed shape -- lane-strided partials, xor-shuffle tree, maxima that do not depend on order, window sums
// in fp64 over exact squares -- so two runs give the same bits.  The C ABI (mtts_waveform_*) is behind the kernels.
#include "host.h"

namespace mtts {

using f32x4 = __attribute__((ext_vector_type(4))) float;

// torch's max propagates NaN (then `max_abs > 1.0` is false and the row stays as it is): so does this one
__device__ __forceinline__ float nan_max(float m, float v) { return (v > m || v != v) ? v : m; }
__device__ __forceinline__ float wave_nan_max(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = nan_max(v, __shfl_xor(v, o));
    return v;
}
__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// Valid samples of row b, or -1 when its length is outside the row: samples in [0, ld] (hop == 0), frames in [1, ld / hop + 1]
__device__ __forceinline__ int64_t wave_valid(const WaveFinishArgs& p, int b) {
    const int64_t n = p.lengths[b];
    if (p.hop == 0) return (n < 0 || n > p.ld) ? -1 : n;
    if (n < 1 || n - 1 > p.ld / p.hop) return -1;
    return (int64_t)p.hop * (n - 1);
}

__global__ __launch_bounds__(256) void wave_peak_kernel(const WaveFinishArgs p, int nchunks) {
    __shared__ float part[4];
    const int b = blockIdx.y, tid = threadIdx.x;
    const int64_t valid = wave_valid(p, b);
    const int64_t c0 = (int64_t)blockIdx.x * WAVE_CHUNK;
    float m = 0.f;
    if (valid > c0) {
        const float* row = p.audio + (size_t)b * p.ld;
        const int64_t end = valid < c0 + WAVE_CHUNK ? valid : c0 + WAVE_CHUNK;
#pragma unroll 4
        for (int64_t i = c0 + tid * 4; i < end; i += 1024) {      // i + 4 <= ld: i < valid <= ld, both multiples of 4 apart from valid
            const f32x4 v = *reinterpret_cast<const f32x4*>(row + i);
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (i + k < end) m = nan_max(m, fabsf(v[k]));
        }
    }
    m = wave_nan_max(m);
    if ((tid & 63) == 0) part[tid >> 6] = m;
    __syncthreads();
    if (tid == 0) p.peaks[(size_t)b * nchunks + blockIdx.x] = nan_max(nan_max(part[0], part[1]), nan_max(part[2], part[3]));
}

constexpr int WAVE_WIN_PER_WG = 32;   // 4 waves x 8 windows

// VEC = 4: win % 4 == 0, a lane moves 16 bytes; VEC = 1: any window length, 4 bytes per lane (still coalesced)
template <int VEC>
__global__ __launch_bounds__(256) void wave_scale_rms_kernel(const WaveFinishArgs p, int nchunks, int nwin_max) {
    const int b = blockIdx.y, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t valid = wave_valid(p, b);
    if (valid <= 0) {
        if (blockIdx.x == 0 && threadIdx.x == 0) p.scale[b] = 1.0f;
        return;
    }
    const int64_t n_full = valid / p.win;
    const int64_t n_win = (valid + p.win - 1) / p.win;          // the remainder is scaled too, its RMS is never asked for
    const int64_t w0 = (int64_t)blockIdx.x * WAVE_WIN_PER_WG + wave * 8;
    if (w0 >= n_win) return;                                    // (workgroup 0 always has windows: valid > 0)
    // the row's peak: every wave reduces the same chunk peaks (a few hundred floats out of L2), no second launch
    float peak = 0.f;
    const int used = (int)((valid + WAVE_CHUNK - 1) / WAVE_CHUNK);
    for (int c = lane; c < used; c += 64) peak = nan_max(peak, p.peaks[(size_t)b * nchunks + c]);
    peak = wave_nan_max(peak);
    const bool scale = peak > 1.0f;
    if (blockIdx.x == 0 && threadIdx.x == 0) p.scale[b] = scale ? 0.95f / peak : 1.0f;
    float* row = p.audio + (size_t)b * p.ld;
    for (int k = 0; k < 8; ++k) {
        const int64_t w = w0 + k;
        if (w >= n_win) break;                                  // wave-uniform
        const int64_t base = w * p.win;
        double q = 0.0;
        for (int e = lane * VEC; e < p.win; e += 64 * VEC) {
            const int64_t i = base + e;
            if (i >= valid) break;
            if constexpr (VEC == 4) {
                f32x4 v = *reinterpret_cast<const f32x4*>(row + i);          // i + 4 <= ld (ld % 4 == 0)
                const bool whole = i + 4 <= valid;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    if (scale) v[j] = v[j] / peak * 0.95f;
                    if (whole || i + j < valid) q += (double)v[j] * (double)v[j];
                }
                if (scale) {
                    if (whole) *reinterpret_cast<f32x4*>(row + i) = v;
                    else
                        for (int j = 0; j < 4; ++j)
                            if (i + j < valid) row[i + j] = v[j];
                }
            } else {
                float v = row[i];
                if (scale) { v = v / peak * 0.95f; row[i] = v; }
                q += (double)v * (double)v;
            }
        }
        q = wave_sum_d(q);
        if (lane == 0 && w < n_full) p.rms[(size_t)b * nwin_max + w] = (float)sqrt(q / (double)p.win);
    }
}

// out_lengths[b] = valid - (trailing windows with rms < thr) * win; `!(rms < thr)` is loud, so a NaN window ends the run
__global__ __launch_bounds__(256) void wave_trim_kernel(const WaveFinishArgs p, int nwin_max) {
    __shared__ int part[4];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int64_t valid = wave_valid(p, b);
    if (valid < 0) {
        if (tid == 0) { p.out_lengths[b] = -1; p.scale[b] = 1.0f; }
        return;
    }
    const int n_full = (int)(valid / p.win);
    int last = 0;                                               // 1-based index of the last loud window, 0 = none
    for (int w = tid; w < n_full; w += 256)
        if (!(p.rms[(size_t)b * nwin_max + w] < p.thr)) last = w + 1;      // w grows: the thread's latest is its largest
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) last = max(last, __shfl_xor(last, o));
    if ((tid & 63) == 0) part[tid >> 6] = last;
    __syncthreads();
    if (tid == 0) {
        last = max(max(part[0], part[1]), max(part[2], part[3]));
        p.out_lengths[b] = valid - (int64_t)(n_full - last) * p.win;
        if (valid == 0) p.scale[b] = 1.0f;
    }
}

hipError_t launch_wave_finish(const WaveFinishArgs& a, hipStream_t s) {
    if (!a.audio || !a.lengths || !a.scale || !a.out_lengths || !a.peaks || !a.rms) return hipErrorInvalidValue;
    if (a.B <= 0 || a.B > 65535 || a.ld < 0 || (a.ld & 3) || (reinterpret_cast<uintptr_t>(a.audio) & 15) || a.hop < 0 || a.win <= 0)
        return hipErrorInvalidValue;
    if (a.ld / a.win > 0x3fffffff) return hipErrorInvalidValue;
    const int nchunks = (int)((a.ld + WAVE_CHUNK - 1) / WAVE_CHUNK);
    const int nwin_max = (int)(a.ld / a.win);
    if (a.ld > 0) {
        hipLaunchKernelGGL(wave_peak_kernel, dim3(nchunks, a.B), dim3(256), 0, s, a, nchunks);
        const int nwg = (int)((a.ld / a.win + 1 + WAVE_WIN_PER_WG - 1) / WAVE_WIN_PER_WG);
        if (a.win % 4 == 0)
            hipLaunchKernelGGL(wave_scale_rms_kernel<4>, dim3(nwg, a.B), dim3(256), 0, s, a, nchunks, nwin_max);
        else
            hipLaunchKernelGGL(wave_scale_rms_kernel<1>, dim3(nwg, a.B), dim3(256), 0, s, a, nchunks, nwin_max);
    }
    hipLaunchKernelGGL(wave_trim_kernel, dim3(a.B), dim3(256), 0, s, a, nwin_max);
    return hipGetLastError();
}

}  // namespace mtts

using namespace mtts;

extern "C" {

// ---- waveform finish (waveform.hip)
static int wave_window(int sample_rate) { return (int)(0.01 * (double)sample_rate); }       // reference inference.py:270
int64_t mtts_waveform_workspace_bytes(int64_t ld, int B, int sample_rate) {
    const int win = wave_window(sample_rate);
    if (ld < 0 || B <= 0 || win <= 0) { set_error("mtts_waveform_workspace_bytes: bad shape"); return -1; }
    WS ws(nullptr, 0);
    ws.f((size_t)B * ((ld + WAVE_CHUNK - 1) / WAVE_CHUNK + 1));
    ws.f((size_t)B * (ld / win + 1));
    return (int64_t)ws.off + 256;
}
int mtts_waveform_finish(float* d_audio, int64_t ld, const int64_t* d_lengths, int hop, int B, int sample_rate, double threshold_db,
                         float* d_scale, int64_t* d_out_lengths, void* d_ws, int64_t ws_bytes, void* stream) {
    WaveFinishArgs a;
    a.win = wave_window(sample_rate);
    if (!d_audio || !d_lengths || !d_scale || !d_out_lengths || !d_ws || B <= 0 || B > 65535 || ld < 0 || hop < 0 || a.win <= 0) {
        set_error("mtts_waveform_finish: bad argument");
        return -1;
    }
    if ((ld & 3) || (reinterpret_cast<uintptr_t>(d_audio) & 15)) {
        set_error("mtts_waveform_finish: rows must be 16-byte aligned (ld a multiple of 4 samples)");
        return -1;
    }
    WS ws(d_ws, (size_t)ws_bytes);
    a.peaks = ws.f((size_t)B * ((ld + WAVE_CHUNK - 1) / WAVE_CHUNK + 1));
    a.rms = ws.f((size_t)B * (ld / a.win + 1));
    if (ws.overflow) { set_error("mtts_waveform_finish: workspace too small"); return -1; }
    a.audio = d_audio; a.ld = ld; a.lengths = d_lengths; a.hop = hop; a.B = B;
    a.thr = (float)std::pow(10.0, threshold_db / 20.0);         // reference inference.py:271; torch compares the fp32 RMS in fp32
    a.scale = d_scale; a.out_lengths = d_out_lengths;
    HIP_OK(launch_wave_finish(a, static_cast<hipStream_t>(stream)));
    return 0;
}

}  // extern "C"
