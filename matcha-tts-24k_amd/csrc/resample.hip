// Sample-rate conversion (gfx950): a ragged batch of fp32 clips from orig_freq to new_freq in one launch.
//
// Semantics: the windowed-sinc polyphase interpolation that torchaudio.functional.resample documents as its default
// (resampling_method "sinc_interp_hann", lowpass_filter_width 6, rolloff 0.99), restated from its formulae -- the package is not a
// dependency and no source of it is at hand, see DESIGN.md section 4.  With g = gcd(orig, new), o = orig / g, n = new / g:
//     base = min(o, n) * rolloff,  width = ceil(lpw * o / base),  taps = 2 * width + o
//     t = clamp((-p / n + (k - width) / o) * base, -lpw, lpw)
//     K[p][k] = (t == 0 ? 1 : sin(pi t) / (pi t)) * cos(t pi / lpw / 2)^2 * (base / o)          fp64, rounded once to fp32
//     out[q n + p] = sum_k K[p][k] * x[q o + k - width],  x = 0 outside [0, L),  q n + p < out_len(L) = ceil(n L / o)
// After the rounding the taps at the clamp are exact zeros (their fp64 values are ~1e-49), so each phase keeps a band of `band`
// consecutive taps from first[p] on; only the band is stored and evaluated.  Adding K = 0 terms to a finite sum changes nothing,
// so the band sum in ascending k has the bits of the dense sum in ascending k.
//
// One kernel, grid (output tile, clip), 256 threads, RS_TILE outputs per workgroup:
//   * the banded bank (row stride odd, so that lanes on consecutive phases read different LDS banks) and first[] go to LDS;
//   * the tile's input span goes to LDS by 16-byte loads where a whole quad lies inside [0, len_b), element-wise clipped and
//     zero-filled at the clip's two ends: nothing outside [0, len_b) is ever read;
//   * lane l computes outputs l, l + 256, l + 512, l + 768 of the tile, each as ONE serial chain s = s + K * x over ascending k
//     (multiply and add rounded separately; the build has -ffp-contract=off); the four chains of a lane are independent (ILP);
//   * the results cross LDS once so that every lane stores 16 bytes; a row is written whole, zeros from out_len to ld_out.
// No atomics on memory, no scratch.  A clip's samples do not depend on the batch it is in.
#include "host.h"
#include "device_utils.h"

#include <cmath>
#include <cstring>
#include <numeric>
#include <vector>

namespace mtts {

using f32x4 = __attribute__((ext_vector_type(4))) float;

constexpr int RS_TILE = MTTS_RESAMPLE_TILE;     // outputs per workgroup
constexpr int RS_THREADS = 256;
constexpr int RS_PER_LANE = RS_TILE / RS_THREADS;
static_assert(RS_PER_LANE == 4, "a lane stores one 16-byte quad of the tile");

struct ResampleArgs {
    const float* in;             // [B][ld_in]
    const int64_t* lengths;      // [B]
    int64_t ld_in, ld_out;
    float* out;                  // [B][ld_out]
    int64_t* out_lengths;        // [B]
    int64_t* status;             // workspace header: first refused row + 1 (0: none), its length, ld_in, ld_out
    const float* bank;           // [n][bstride] band of each phase | first[n] as int32
    int B, o, n, width, band, bstride;
    int fmin;                    // smallest first[p]
    int bank_words;              // n * bstride + n rounded up to 4: the LDS image [bank | first]
    int span_words;              // the staged input span, a multiple of 4
};

// out_len of a clip, or -1 for a length the call refuses (outside [0, ld_in], or with more outputs than a row holds)
__device__ __forceinline__ int64_t rs_out_len(int64_t len, const ResampleArgs& a) {
    if (len < 0 || len > a.ld_in) return -1;
    const int64_t m = (len * a.n + a.o - 1) / a.o;
    return m > a.ld_out ? -1 : m;
}

__global__ __launch_bounds__(RS_THREADS) void resample_kernel(const ResampleArgs a) {
    extern __shared__ __attribute__((aligned(16))) float lds[];      // [bank | first] [span] [RS_TILE outputs]
    const int tid = threadIdx.x;
    const int b = blockIdx.y;
    const int64_t j0 = (int64_t)blockIdx.x * RS_TILE;

    if (blockIdx.x == 0 && b == 0) {             // the verdict on every row's length, by one workgroup
        const int i = first_refused_row(a.B, [&](int r) { return rs_out_len(a.lengths[r], a) < 0; });
        if (tid == 0) {
            a.status[0] = i < a.B ? i + 1 : 0;
            a.status[1] = i < a.B ? a.lengths[i] : 0;
            a.status[2] = a.ld_in;
            a.status[3] = a.ld_out;
        }
    }

    const int64_t len = a.lengths[b];
    const int64_t out_len = rs_out_len(len, a);
    if (blockIdx.x == 0 && tid == 0) a.out_lengths[b] = out_len;
    float* orow = a.out + (size_t)b * a.ld_out;
    const int64_t jq = j0 + 4 * tid;             // this lane's quad of the row (ld_out % 4 == 0: a quad is inside the row or outside)
    if (j0 >= out_len) {                         // beyond the clip's outputs, an empty or a refused row: zeros
        if (jq < a.ld_out) *reinterpret_cast<f32x4*>(orow + jq) = f32x4{0.f, 0.f, 0.f, 0.f};
        return;
    }

    float* bank = lds;
    const int* first = reinterpret_cast<const int*>(lds + a.n * a.bstride);
    float* span = lds + a.bank_words;
    float* outs = span + a.span_words;

    for (int i = tid * 4; i < a.bank_words; i += RS_THREADS * 4)
        *reinterpret_cast<f32x4*>(bank + i) = *reinterpret_cast<const f32x4*>(a.bank + i);

    // input sample of span[0]: the first sample any output of the tile can touch, moved down to a 16-byte boundary of the row
    const int q0 = (int)(j0 / a.n);
    const int in0 = (q0 * a.o - a.width + a.fmin) & ~3;
    const float* irow = a.in + (size_t)b * a.ld_in;
    const int L = (int)len;
    for (int i = tid * 4; i < a.span_words; i += RS_THREADS * 4) {
        const int s = in0 + i;
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (s >= 0 && s + 3 < L) {
            v = *reinterpret_cast<const f32x4*>(irow + s);
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (s + e >= 0 && s + e < L) v[e] = irow[s + e];
        }
        *reinterpret_cast<f32x4*>(span + i) = v;
    }
    __syncthreads();

    const float* kp[RS_PER_LANE];
    const float* xp[RS_PER_LANE];
    bool live[RS_PER_LANE];
#pragma unroll
    for (int e = 0; e < RS_PER_LANE; ++e) {
        const int64_t j = j0 + tid + e * RS_THREADS;
        live[e] = j < out_len;
        const int jj = live[e] ? (int)j : (int)j0;          // (a dead slot walks the tile's first output: inside the span)
        const int q = jj / a.n, p = jj - q * a.n;
        kp[e] = bank + p * a.bstride;
        xp[e] = span + (q * a.o - a.width + first[p] - in0);
    }
    float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
    for (int k = 0; k < a.band; ++k) {           // ascending tap index: the documented order
        s0 = s0 + kp[0][k] * xp[0][k];
        s1 = s1 + kp[1][k] * xp[1][k];
        s2 = s2 + kp[2][k] * xp[2][k];
        s3 = s3 + kp[3][k] * xp[3][k];
    }
    outs[tid] = live[0] ? s0 : 0.f;
    outs[tid + RS_THREADS] = live[1] ? s1 : 0.f;
    outs[tid + 2 * RS_THREADS] = live[2] ? s2 : 0.f;
    outs[tid + 3 * RS_THREADS] = live[3] ? s3 : 0.f;
    __syncthreads();
    if (jq < a.ld_out) *reinterpret_cast<f32x4*>(orow + jq) = *reinterpret_cast<const f32x4*>(outs + 4 * tid);
}

}  // namespace mtts

using namespace mtts;

// Host object: the bank in fp64 -> fp32 at create (no device needed), its banded device copy at the first forward.
struct mtts_resampler {
    int orig = 0, dest = 0, lpw = 6;
    double rolloff = 0.99;
    int o = 0, n = 0, width = 0, taps = 0, band = 0, bstride = 0, fmin = 0;
    int bank_words = 0, span_words = 0;
    std::vector<float> K;            // dense [n][taps]
    std::vector<int> first;          // [n] first tap of each phase's band
    void* d_blob = nullptr;
    int device = -1;
};

static void resampler_tables(mtts_resampler* r) {
    const int o = r->o, n = r->n, lpw = r->lpw;
    const double pi = 3.14159265358979323846;
    const double base = (double)std::min(o, n) * r->rolloff;
    r->width = (int)std::ceil((double)lpw * (double)o / base);
    r->taps = 2 * r->width + o;
    const double scale = base / (double)o;
    r->K.assign((size_t)n * r->taps, 0.f);
    for (int p = 0; p < n; ++p)
        for (int k = 0; k < r->taps; ++k) {
            double t = (-(double)p / (double)n + (double)(k - r->width) / (double)o) * base;
            t = t < -(double)lpw ? -(double)lpw : (t > (double)lpw ? (double)lpw : t);
            const double c = std::cos(t * pi / (double)lpw / 2.0);
            const double a = t * pi;
            const double sinc = t == 0.0 ? 1.0 : std::sin(a) / a;
            r->K[(size_t)p * r->taps + k] = (float)(sinc * (c * c) * scale);
        }
    // the band: the widest run from a phase's first to its last non-zero tap; every phase keeps `band` taps from first[p] on
    std::vector<int> lo(n, 0);
    r->band = 1;
    for (int p = 0; p < n; ++p) {
        int a = r->taps, b = -1;
        for (int k = 0; k < r->taps; ++k)
            if (r->K[(size_t)p * r->taps + k] != 0.f) { a = std::min(a, k); b = std::max(b, k); }
        if (b < a) { a = 0; b = 0; }
        lo[p] = a;
        r->band = std::max(r->band, b - a + 1);
    }
    r->first.assign(n, 0);
    int fmin = r->taps, fmax = 0;
    for (int p = 0; p < n; ++p) {
        r->first[p] = std::max(0, std::min(lo[p], r->taps - r->band));
        fmin = std::min(fmin, r->first[p]);
        fmax = std::max(fmax, r->first[p]);
    }
    r->fmin = fmin;
    r->bstride = r->band | 1;
    r->bank_words = round_up(n * r->bstride + n, 4);
    // q of a tile's outputs spans at most ceil((RS_TILE - 1) / n) input periods; + the widest band reach, + 3 for the alignment of
    // span[0] down to a quad, rounded up to whole quads
    const int64_t reach = (int64_t)((RS_TILE - 1 + n - 1) / n) * o + (fmax - fmin) + r->band;
    r->span_words = (int)std::min<int64_t>((reach + 3 + 3) / 4 * 4, 1 << 28);       // (far beyond the LDS budget: create refuses)
}

static int resampler_upload(mtts_resampler* r) {
    int dev = -1;
    (void)hipGetDevice(&dev);
    if (r->d_blob) {
        if (dev != r->device) { set_error("mtts_resample_forward: this resampler's tables live on another device (one object per device)"); return -1; }
        return 0;
    }
    std::vector<float> blob((size_t)r->bank_words, 0.f);
    for (int p = 0; p < r->n; ++p)
        for (int k = 0; k < r->band; ++k) blob[(size_t)p * r->bstride + k] = r->K[(size_t)p * r->taps + r->first[p] + k];
    std::memcpy(blob.data() + (size_t)r->n * r->bstride, r->first.data(), (size_t)r->n * sizeof(int));
    void* d = nullptr;
    hipError_t e = hipMalloc(&d, blob.size() * sizeof(float));
    if (e == hipSuccess) e = hipMemcpy(d, blob.data(), blob.size() * sizeof(float), hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        if (d) (void)hipFree(d);
        set_error(std::string("mtts_resample_forward: table upload: ") + hipGetErrorString(e));
        return -1;
    }
    r->d_blob = d;
    r->device = dev;
    return 0;
}

static size_t resampler_lds_bytes(const mtts_resampler* r) {
    return ((size_t)r->bank_words + (size_t)r->span_words + RS_TILE) * sizeof(float);
}

extern "C" {

int mtts_resample_tile(void) { return RS_TILE; }

mtts_resampler* mtts_resampler_create(int orig_freq, int new_freq, int lowpass_filter_width, double rolloff) {
    if (orig_freq < 4000 || orig_freq > 384000 || new_freq < 4000 || new_freq > 384000) {
        set_error("mtts_resampler_create: rates must lie in [4000, 384000] Hz");
        return nullptr;
    }
    if (orig_freq == new_freq) { set_error("mtts_resampler_create: the two rates are equal (nothing to convert)"); return nullptr; }
    if (lowpass_filter_width < 1 || lowpass_filter_width > 64) { set_error("mtts_resampler_create: lowpass_filter_width must lie in [1, 64]"); return nullptr; }
    if (!(rolloff > 0.0 && rolloff <= 1.0)) { set_error("mtts_resampler_create: rolloff must lie in (0, 1]"); return nullptr; }
    const int g = std::gcd(orig_freq, new_freq);
    const int o = orig_freq / g, n = new_freq / g;
    // sizes before the tables are built: taps = 2 ceil(lpw o / base) + o, band <= taps
    const double base = (double)std::min(o, n) * rolloff;
    const double taps_est = 2.0 * std::ceil((double)lowpass_filter_width * (double)o / base) + (double)o;
    if ((double)n * taps_est > 4.0 * 1024 * 1024) {
        set_error("mtts_resampler_create: the rate pair's polyphase bank is too large (rates with a small common divisor)");
        return nullptr;
    }
    mtts_resampler* r = new mtts_resampler();
    r->orig = orig_freq; r->dest = new_freq; r->lpw = lowpass_filter_width; r->rolloff = rolloff;
    r->o = o; r->n = n;
    resampler_tables(r);
    if ((int64_t)r->n * r->band > MTTS_RESAMPLE_MAX_BANK) {
        set_error("mtts_resampler_create: the banded bank has " + std::to_string((int64_t)r->n * r->band) + " floats, more than "
                  "MTTS_RESAMPLE_MAX_BANK = " + std::to_string(MTTS_RESAMPLE_MAX_BANK) + " (rates with a small common divisor)");
        delete r;
        return nullptr;
    }
    if (resampler_lds_bytes(r) > (size_t)MTTS_RESAMPLE_LDS_BYTES) {
        set_error("mtts_resampler_create: a tile's input span (" + std::to_string(r->span_words) + " samples) does not fit the kernel's LDS "
                  "budget MTTS_RESAMPLE_LDS_BYTES (the decimation ratio is too steep)");
        delete r;
        return nullptr;
    }
    return r;
}
void mtts_resampler_destroy(mtts_resampler* r) {
    if (!r) return;
    if (r->d_blob) (void)hipFree(r->d_blob);
    delete r;
}
int mtts_resample_factors(mtts_resampler* r, int* o, int* n, int* width, int* taps, int* band) {
    if (!r) { set_error("mtts_resample_factors: null resampler"); return -1; }
    if (o) *o = r->o;
    if (n) *n = r->n;
    if (width) *width = r->width;
    if (taps) *taps = r->taps;
    if (band) *band = r->band;
    return 0;
}
int64_t mtts_resample_out_length(mtts_resampler* r, int64_t L) {
    if (!r || L < 0 || L > ((int64_t)1 << 40)) { set_error("mtts_resample_out_length: bad argument"); return -1; }
    return (L * r->n + r->o - 1) / r->o;
}
int mtts_resample_bank(mtts_resampler* r, float* h_K, int64_t numel) {
    if (!r || !h_K || numel != (int64_t)r->K.size()) { set_error("mtts_resample_bank: bad argument (numel = n * taps)"); return -1; }
    std::memcpy(h_K, r->K.data(), r->K.size() * sizeof(float));
    return 0;
}
int64_t mtts_resample_workspace_bytes(mtts_resampler* r, int B, int64_t ld_in) {
    if (!r || B <= 0 || ld_in <= 0) { set_error("mtts_resample_workspace_bytes: bad argument"); return -1; }
    return 256;                                  // the status header
}
int mtts_resample_forward(mtts_resampler* r, const float* d_in, int64_t ld_in, const int64_t* d_lengths, int B, float* d_out, int64_t ld_out,
                          int64_t* d_out_lengths, void* d_ws, int64_t ws_bytes, void* stream) {
    if (!r || !d_in || !d_lengths || !d_out || !d_out_lengths || !d_ws) { set_error("mtts_resample_forward: null argument"); return -1; }
    if (B < 1 || B > 65535) { set_error("mtts_resample_forward: B must lie in [1, 65535]"); return -1; }
    if (ld_in < 4 || ld_out < 4 || (ld_in & 3) || (ld_out & 3)) {
        set_error("mtts_resample_forward: rows must be 16-byte aligned (ld_in and ld_out positive multiples of 4 samples)");
        return -1;
    }
    // samples are indexed in int32 inside the kernel
    if (ld_in > (int64_t)1 << 30 || ld_out > (int64_t)1 << 30) { set_error("mtts_resample_forward: rows longer than 2^30 samples"); return -1; }
    if ((reinterpret_cast<uintptr_t>(d_in) & 15) || (reinterpret_cast<uintptr_t>(d_out) & 15) || (reinterpret_cast<uintptr_t>(d_ws) & 15)) {
        set_error("mtts_resample_forward: misaligned buffer (16 bytes)");
        return -1;
    }
    if (ws_bytes < 256) { set_error("mtts_resample_forward: workspace too small (mtts_resample_workspace_bytes)"); return -1; }
    if (resampler_upload(r)) return -1;
    ResampleArgs a;
    a.in = d_in; a.lengths = d_lengths; a.ld_in = ld_in; a.ld_out = ld_out; a.out = d_out; a.out_lengths = d_out_lengths;
    a.status = static_cast<int64_t*>(d_ws);
    a.bank = static_cast<const float*>(r->d_blob);
    a.B = B; a.o = r->o; a.n = r->n; a.width = r->width; a.band = r->band; a.bstride = r->bstride; a.fmin = r->fmin;
    a.bank_words = r->bank_words; a.span_words = r->span_words;
    const size_t lds = resampler_lds_bytes(r);
    if (lds > 48 * 1024 &&
        launched("resample_kernel", hipFuncSetAttribute(reinterpret_cast<const void*>(resample_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds)))
        return -1;
    const unsigned tiles = (unsigned)((ld_out + RS_TILE - 1) / RS_TILE);
    hipLaunchKernelGGL(resample_kernel, dim3(tiles, B), dim3(RS_THREADS), lds, static_cast<hipStream_t>(stream), a);
    return launched("resample_kernel");
}

// The lengths check's verdict (the header of the call's workspace).  The one entry of this file that waits for the stream.
int mtts_resample_status(const void* d_ws, void* stream) {
    int64_t st[4];
    if (read_status("mtts_resample_status", d_ws, stream, st)) return -1;
    if (st[0] != 0) {
        set_error("mtts_resample_forward: row " + std::to_string(st[0] - 1) + " has length " + std::to_string(st[1]) + " (need 0 <= length <= ld_in = " +
                  std::to_string(st[2]) + " and ceil(n * length / o) <= ld_out = " + std::to_string(st[3]) + ")");
        return -1;
    }
    return 0;
}

}  // extern "C"
