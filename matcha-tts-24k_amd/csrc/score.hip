// Scoring a recording against the model: the reductions of the reference's training forward, forward pass only (reference
// matcha/models/matcha_tts.py:64-164, matcha/models/components/flow_matching.py:65-107).
//
//   score_prior_dur_kernel (+ score_finish_kernel)   prior and duration Huber sums per utterance from mu_x, the MAS durations, the
//                                                    fine mel and logw; the [Tx, Tm] path is never materialised
//   cfm_target_kernel                                the flow-matching input y_t as the estimator's channels-last state rows
//   cfm_loss_kernel (+ cfm_loss_finish_kernel)       masked squared error of the estimator's velocity rows against u, per utterance
//
// All three are memory-bound: every input element is read once, everything is fp32.  Every sum has a FIXED ORDER and no
// floating-point atomics: a thread's serial run, an LDS column / wave butterfly, one partial per workgroup, and a last pass of one
// wave per utterance over the partials.  The partition depends on absolute (feature, frame) indices only, so an utterance's sums
// do not depend on the batch it sits in or on the padded shapes.
//
// Serial run lengths (what the fp64 parity test derives its bound from; all terms are non-negative):
//   prior:  r = ceil(F / 16)  terms per thread and frame, then 16 LDS terms per frame, a 64-lane butterfly per workgroup, and
//           ceil(ceil(Tm / 64) / 64) partials per lane + a butterfly in the last pass          (score_prior_serial_run)
//   dur:    r = ceil(Tx / 64) terms per lane + a butterfly
//   cfm:    r = 4 terms per thread, a butterfly, 4 wave sums, then ceil(tiles / 64) partials per lane + a butterfly
#include "host.h"
#include "device_utils.h"

#include <string>

namespace mtts {

constexpr int SCORE_FRAMES = 64;        // fine frames per workgroup of score_prior_dur_kernel
constexpr int SCORE_FLANES = 16;        // feature lanes: thread (fl, yg) owns features fl, fl + 16, ... of frames 4 yg .. 4 yg + 3
constexpr int SCORE_MAX_TX = 1024;      // tokens (the cumulative durations live in LDS), as mtts_mas

__device__ __forceinline__ float score_wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// torch.nn.functional.huber_loss, elementwise
__device__ __forceinline__ float huber(float d, float delta) {
    const float ad = fabsf(d);
    return ad < delta ? 0.5f * d * d : delta * (ad - 0.5f * delta);
}

struct ScoreArgs {
    const float* mu_x;          // [B][F][Tx]
    const float* logw;          // [B][Tx]
    const int32_t* dur;         // [B][Tx]
    const float* y;             // [B][F][Tm]
    const int64_t* x_len;       // [B]
    const int64_t* y_len;       // [B]
    int B, F, Tx, Tm, nchunks, vec4;
    float delta_prior, delta_dur;
    float* prior_sum;           // [B]
    float* dur_sum;             // [B]
    float* prior_frame;         // [B][Tm] or null
    float* dur_err;             // [B][Tx] or null
    int32_t* status;            // workspace header
    int32_t* verdict;           // [B][2]: (0 ok / 1 lengths / 2 durations, duration total)
    float* partial;             // [B][nchunks]
};

// Workgroup (chunk, b): frames [64 chunk, 64 chunk + 64) of utterance b, all features.  Every workgroup of an utterance scans the
// durations itself (<= 1024 integers from L2): no launch in front of this one.
__global__ __launch_bounds__(256) void score_prior_dur_kernel(ScoreArgs a) {
    __shared__ int cum[SCORE_MAX_TX];
    __shared__ int scan[256];
    __shared__ int odd;
    __shared__ float red[SCORE_FLANES][SCORE_FRAMES];
    const int b = blockIdx.y, chunk = blockIdx.x, tid = threadIdx.x;
    const int64_t xl = a.x_len[b], yl = a.y_len[b];
    const bool bad_len = xl < 1 || xl > a.Tx || yl > a.Tm || yl < xl;
    const int txb = bad_len ? 0 : (int)xl, tmb = bad_len ? 0 : (int)yl;
    if (tid == 0) odd = 0;
    __syncthreads();
    // inclusive cumulative durations of the valid tokens
    const int32_t* db = a.dur + (size_t)b * a.Tx;
    int v[4], run = 0;
    bool strange = false;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int x = 4 * tid + k;
        int d = x < txb ? db[x] : 0;
        if (d < 0 || d > a.Tm) { strange = true; d = 0; }
        run += d;
        v[k] = run;
    }
    scan[tid] = run;
    if (strange) odd = 1;
    __syncthreads();
    for (int off = 1; off < 256; off <<= 1) {
        const int add = tid >= off ? scan[tid - off] : 0;
        __syncthreads();
        scan[tid] += add;
        __syncthreads();
    }
    const int base = tid ? scan[tid - 1] : 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) cum[4 * tid + k] = base + v[k];
    __syncthreads();
    const int total = scan[255];
    const int code = bad_len ? 1 : (odd || total != tmb) ? 2 : 0;
    if (chunk == 0 && tid == 0) {
        a.verdict[2 * b] = code;
        a.verdict[2 * b + 1] = total;
    }
    const int yg = tid & 15, fl = tid >> 4;
    const int y0 = chunk * SCORE_FRAMES + 4 * yg;
    float pf[4] = {0.f, 0.f, 0.f, 0.f};
    if (code == 0 && y0 < tmb) {
        int tok[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int y = y0 + k;
            int r = -1;
            if (y < tmb) {                        // first token whose inclusive cumulative duration exceeds y (align_pool_kernel's rule)
                int lo = 0, hi = txb - 1;
                while (lo < hi) {
                    const int mid = (lo + hi) >> 1;
                    if (cum[mid] > y) hi = mid; else lo = mid + 1;
                }
                r = lo;
            }
            tok[k] = r;
        }
        for (int f = fl; f < a.F; f += SCORE_FLANES) {
            const float* yr = a.y + ((size_t)b * a.F + f) * a.Tm + y0;
            const float* mr = a.mu_x + ((size_t)b * a.F + f) * a.Tx;
            float yv[4];
            if (a.vec4) {                         // Tm % 4 == 0 and a 16-byte aligned base: frames y0 .. y0 + 3 are inside the row
                const float4 q = *reinterpret_cast<const float4*>(yr);
                yv[0] = q.x; yv[1] = q.y; yv[2] = q.z; yv[3] = q.w;
            } else {
#pragma unroll
                for (int k = 0; k < 4; ++k) yv[k] = y0 + k < tmb ? yr[k] : 0.f;
            }
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (tok[k] >= 0) pf[k] += huber(yv[k] - mr[tok[k]], a.delta_prior);
        }
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) red[fl][4 * yg + k] = pf[k];
    __syncthreads();
    if (tid < 64) {
        float s = 0.f;
#pragma unroll
        for (int j = 0; j < SCORE_FLANES; ++j) s += red[j][tid];
        const int y = chunk * SCORE_FRAMES + tid;
        if (a.prior_frame && y < a.Tm) a.prior_frame[(size_t)b * a.Tm + y] = s;
        s = score_wave_sum(s);
        if (tid == 0) a.partial[(size_t)b * a.nchunks + chunk] = s;
    }
}

// One wave per utterance: the partials in order, the duration sum, and (utterance 0's wave) the verdict for the status call.
__global__ __launch_bounds__(64) void score_finish_kernel(ScoreArgs a) {
    const int b = blockIdx.x, lane = threadIdx.x;
    if (b == 0) {
        const int i = first_refused_row(a.B, [&](int r) { return a.verdict[2 * r] != 0; });
        if (lane == 0) {
            a.status[0] = i < a.B ? i + 1 : 0;
            a.status[1] = i < a.B ? sat32(a.x_len[i]) : 0;
            a.status[2] = i < a.B ? sat32(a.y_len[i]) : 0;
            a.status[3] = a.Tx;
            a.status[4] = a.Tm;
            a.status[5] = i < a.B ? a.verdict[2 * i] : 0;
            a.status[6] = i < a.B ? a.verdict[2 * i + 1] : 0;
        }
    }
    const bool ok = a.verdict[2 * b] == 0;
    const int txb = ok ? (int)a.x_len[b] : 0;
    float s = 0.f;
    if (ok)
        for (int i = lane; i < a.nchunks; i += 64) s += a.partial[(size_t)b * a.nchunks + i];
    s = score_wave_sum(s);
    float e = 0.f;
    for (int x = lane; x < a.Tx; x += 64) {
        float d = 0.f;
        if (x < txb) {
            d = a.logw[(size_t)b * a.Tx + x] - logf(2.0f + (float)a.dur[(size_t)b * a.Tx + x]);
            e += huber(d, a.delta_dur);
        }
        if (a.dur_err) a.dur_err[(size_t)b * a.Tx + x] = d;
    }
    e = score_wave_sum(e);
    if (lane == 0) {
        a.prior_sum[b] = s;
        a.dur_sum[b] = e;
    }
}

// ---------------------------------------------------------------------------------------------- flow matching
// dst[b*T + t, 0..C) = y_t = (1 - (1 - sigma_min) t_b) x0 + t_b x1 with x0 = noise (+ mu), in the reference's operation order
// (flow_matching.py:84-93; omsm = fp32(1 - sigma_min), as the Python scalar meets the fp32 tensor); dst[.., C..2C) = mu; the
// remaining columns of the row are zero.  [B,C,T] -> rows of [B*T, ld]: what fill_cols + two cf_to_cl launches do for
// mtts_decoder_forward.
__global__ void cfm_target_kernel(const float* __restrict__ x1, const float* __restrict__ noise, const float* __restrict__ mu,
                                  const float* __restrict__ tt, int add_mu, float omsm, int C, int T, float* __restrict__ dst, int ld) {
    __shared__ float tile[32][33];
    __shared__ float tmu[32][33];
    const int b = blockIdx.z, t0 = blockIdx.x * 32, c0 = blockIdx.y * 32;
    const int tx = threadIdx.x, ty = threadIdx.y;
    const float tb = tt[b];
    const float a = 1.0f - omsm * tb;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int c = c0 + ty + 8 * k, t = t0 + tx;
        float v = 0.f, m = 0.f;
        if (c < C && t < T) {
            const size_t i = ((size_t)b * C + c) * T + t;
            m = mu[i];
            float x0 = noise[i];
            if (add_mu) x0 = m + x0;
            v = a * x0 + tb * x1[i];
        }
        tile[ty + 8 * k][tx] = v;
        tmu[ty + 8 * k][tx] = m;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int t = t0 + ty + 8 * k, c = c0 + tx;
        if (t >= T) continue;
        float* row = dst + ((size_t)b * T + t) * ld;
        if (c < C) {
            row[c] = tile[tx][ty + 8 * k];
            row[C + c] = tmu[tx][ty + 8 * k];
        }
        if (blockIdx.y == 0)
            for (int p = 2 * C + tx; p < ld; p += 32) row[p] = 0.f;
    }
}
hipError_t launch_cfm_target(const float* x1, const float* noise, const float* mu, const float* t_b, int add_mu, float sigma_min, int B,
                             int C, int T, float* dst, int ld, hipStream_t s) {
    if (!x1 || !noise || !mu || !t_b || !dst || B <= 0 || C <= 0 || T <= 0 || ld < 2 * C) return hipErrorInvalidValue;
    const float omsm = (float)(1.0 - (double)sigma_min);
    hipLaunchKernelGGL(cfm_target_kernel, dim3((T + 31) / 32, (C + 31) / 32, B), dim3(32, 8), 0, s, x1, noise, mu, t_b, add_mu, omsm, C, T,
                       dst, ld);
    return hipGetLastError();
}

// partial[b][tile] = sum over the tile of (pred * mask - u * mask)^2, u = x1 - (1 - sigma_min) x0 recomputed from its sources
// (flow_matching.py:95,105); pred = velocity rows [B*T, ldv] (channels last), optionally copied out channels first.
__global__ void cfm_loss_kernel(const float* __restrict__ vel, int ldv, const float* __restrict__ x1, const float* __restrict__ noise,
                                const float* __restrict__ mu, const float* __restrict__ mask, int add_mu, float omsm, int C, int T,
                                float* __restrict__ partial, float* __restrict__ pred) {
    __shared__ float tile[32][33];
    __shared__ float wsum[4];
    const int b = blockIdx.z, t0 = blockIdx.x * 32, c0 = blockIdx.y * 32;
    const int tx = threadIdx.x, ty = threadIdx.y;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int t = t0 + ty + 8 * k, c = c0 + tx;
        tile[ty + 8 * k][tx] = (c < C && t < T) ? vel[((size_t)b * T + t) * ldv + c] : 0.f;
    }
    __syncthreads();
    float acc = 0.f;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int c = c0 + ty + 8 * k, t = t0 + tx;
        if (c < C && t < T) {
            const size_t i = ((size_t)b * C + c) * T + t;
            const float p = tile[tx][ty + 8 * k];
            const float m = mask[(size_t)b * T + t];
            float x0 = noise[i];
            if (add_mu) x0 = mu[i] + x0;
            const float u = x1[i] - omsm * x0;
            const float d = p * m - u * m;
            acc += d * d;
            if (pred) pred[i] = p;
        }
    }
    acc = score_wave_sum(acc);
    const int tid = ty * 32 + tx;
    if ((tid & 63) == 0) wsum[tid >> 6] = acc;
    __syncthreads();
    if (tid == 0) partial[((size_t)b * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x] = ((wsum[0] + wsum[1]) + wsum[2]) + wsum[3];
}
__global__ __launch_bounds__(64) void cfm_loss_finish_kernel(const float* __restrict__ partial, int n, float* __restrict__ sq_sum) {
    const int b = blockIdx.x, lane = threadIdx.x;
    float s = 0.f;
    for (int i = lane; i < n; i += 64) s += partial[(size_t)b * n + i];
    s = score_wave_sum(s);
    if (lane == 0) sq_sum[b] = s;
}
int64_t cfm_loss_partials(int B, int C, int T) { return (int64_t)B * ((T + 31) / 32) * ((C + 31) / 32); }
hipError_t launch_cfm_loss(const float* vel, int ldv, const float* x1, const float* noise, const float* mu, const float* mask, int add_mu,
                           float sigma_min, int B, int C, int T, float* partial, float* pred, hipStream_t s) {
    if (!vel || !x1 || !noise || !mu || !mask || !partial || B <= 0 || C <= 0 || T <= 0 || ldv < C) return hipErrorInvalidValue;
    const float omsm = (float)(1.0 - (double)sigma_min);
    hipLaunchKernelGGL(cfm_loss_kernel, dim3((T + 31) / 32, (C + 31) / 32, B), dim3(32, 8), 0, s, vel, ldv, x1, noise, mu, mask, add_mu,
                       omsm, C, T, partial, pred);
    return hipGetLastError();
}
hipError_t launch_cfm_loss_finish(const float* partial, int B, int C, int T, float* sq_sum, hipStream_t s) {
    if (!partial || !sq_sum || B <= 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(cfm_loss_finish_kernel, dim3(B), dim3(64), 0, s, partial, (int)(cfm_loss_partials(B, C, T) / B), sq_sum);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------- host side
struct ScorePlan { int nchunks = 0; size_t verdict = 0, partial = 0, total = 0; };
static ScorePlan score_plan(int B, int Tm) {
    ScorePlan p;
    p.nchunks = (Tm + SCORE_FRAMES - 1) / SCORE_FRAMES;
    p.verdict = SCORE_HEADER_BYTES;
    p.partial = p.verdict + ((size_t)B * 2 * sizeof(int32_t) + 255) / 256 * 256;
    p.total = p.partial + ((size_t)B * p.nchunks * sizeof(float) + 255) / 256 * 256;
    return p;
}
static bool score_shape_ok(const char* who, int B, int F, int Tx, int Tm) {
    if (B < 1 || B > 65535) { set_error(std::string(who) + ": B must be in [1, 65535]"); return false; }
    if (F < 1) { set_error(std::string(who) + ": F < 1"); return false; }
    if (Tx < 1 || Tx > SCORE_MAX_TX) { set_error(std::string(who) + ": Tx must be in [1, 1024]"); return false; }
    if (Tm < Tx) { set_error(std::string(who) + ": Tm < Tx (no monotone path gives every token a frame)"); return false; }
    if (Tm > (1 << 20)) { set_error(std::string(who) + ": Tm too large"); return false; }
    return true;
}

}  // namespace mtts

using namespace mtts;

extern "C" {

int64_t mtts_score_workspace_bytes(int B, int Tx, int Tm) {
    if (!score_shape_ok("mtts_score_workspace_bytes", B, 1, Tx, Tm)) return -1;
    return (int64_t)score_plan(B, Tm).total;
}

int mtts_score_serial_run(int which, int F, int Tx, int Tm) {
    if (which == 0) return (F + SCORE_FLANES - 1) / SCORE_FLANES + SCORE_FLANES + ((Tm + SCORE_FRAMES - 1) / SCORE_FRAMES + 63) / 64;
    if (which == 1) return (Tx + 63) / 64;
    if (which == 2) return 4 + 4 + (int)((cfm_loss_partials(1, F, Tm) + 63) / 64);
    set_error("mtts_score_serial_run: which must be 0 (prior), 1 (duration) or 2 (flow matching)");
    return -1;
}

int mtts_score_prior_dur(const float* d_mu_x, const float* d_logw, const int32_t* d_durations, const float* d_y_fine,
                         const int64_t* d_x_lengths, const int64_t* d_y_fine_lengths, int B, int F, int Tx, int Tm, float delta_prior,
                         float delta_dur, float* d_prior_sum, float* d_dur_sum, float* d_prior_frame, float* d_dur_err, void* d_ws,
                         int64_t ws_bytes, void* stream) {
    if (!d_mu_x || !d_logw || !d_durations || !d_y_fine || !d_x_lengths || !d_y_fine_lengths || !d_prior_sum || !d_dur_sum || !d_ws) {
        set_error("mtts_score_prior_dur: null argument");
        return -1;
    }
    if (!score_shape_ok("mtts_score_prior_dur", B, F, Tx, Tm)) return -1;
    if (!(delta_prior > 0.f) || !(delta_dur > 0.f)) { set_error("mtts_score_prior_dur: the Huber thresholds must be positive"); return -1; }
    const ScorePlan p = score_plan(B, Tm);
    if (ws_bytes < (int64_t)p.total) { set_error("mtts_score_prior_dur: workspace too small (mtts_score_workspace_bytes)"); return -1; }
    if (reinterpret_cast<uintptr_t>(d_ws) & 15) { set_error("mtts_score_prior_dur: workspace must be 16-byte aligned"); return -1; }
    hipStream_t s = static_cast<hipStream_t>(stream);
    char* ws = static_cast<char*>(d_ws);
    ScoreArgs a;
    a.mu_x = d_mu_x; a.logw = d_logw; a.dur = d_durations; a.y = d_y_fine; a.x_len = d_x_lengths; a.y_len = d_y_fine_lengths;
    a.B = B; a.F = F; a.Tx = Tx; a.Tm = Tm; a.nchunks = p.nchunks;
    a.vec4 = (Tm % 4 == 0 && (reinterpret_cast<uintptr_t>(d_y_fine) & 15) == 0) ? 1 : 0;
    a.delta_prior = delta_prior; a.delta_dur = delta_dur;
    a.prior_sum = d_prior_sum; a.dur_sum = d_dur_sum; a.prior_frame = d_prior_frame; a.dur_err = d_dur_err;
    a.status = reinterpret_cast<int32_t*>(ws);
    a.verdict = reinterpret_cast<int32_t*>(ws + p.verdict);
    a.partial = reinterpret_cast<float*>(ws + p.partial);
    hipLaunchKernelGGL(score_prior_dur_kernel, dim3(p.nchunks, B), dim3(256), 0, s, a);
    hipLaunchKernelGGL(score_finish_kernel, dim3(B), dim3(64), 0, s, a);
    return launched("score_prior_dur_kernel / score_finish_kernel");
}

// The verdict of the call's device-side checks (the header of its workspace).  The one entry of this file that waits for the stream.
int mtts_score_status(const void* d_ws, void* stream) {
    int st[7];
    if (read_status("mtts_score_status", d_ws, stream, st)) return -1;
    if (st[0] != 0) {
        const std::string who = "mtts_score_prior_dur: utterance " + std::to_string(st[0] - 1) + " has x_length = " + std::to_string(st[1]) +
                                ", y_length = " + std::to_string(st[2]);
        if (st[5] == 1)
            set_error(who + " (need 1 <= x_length <= Tx = " + std::to_string(st[3]) + " and x_length <= y_length <= Tm = " +
                      std::to_string(st[4]) + ")");
        else
            set_error(who + " and durations that sum to " + std::to_string(st[6]) + " (need non-negative durations that sum to y_length)");
        return -1;
    }
    return 0;
}

}  // extern "C"
