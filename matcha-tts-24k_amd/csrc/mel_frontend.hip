// Log-mel front end (gfx950): waveform -> normalised log-mel, a ragged batch of clips per call.
//
// Semantics: torchaudio MelSpectrogram(sample_rate, n_fft, win_length = n_fft, hop, n_mels, center=True (reflect pad), power=1,
// mel_scale="htk", norm=None) of the clip trimmed to a multiple of hop, log(clamp(., 1e-7)) -- reference
// matcha/vocos24k/mel_extractor.py:6-41 -- then (x - mel_mean) / mel_std -- reference matcha/utils/model.py normalize, as
// matcha/utils/precompute_mels.py:100-113 applies it.
//
// Two launches:
//   mel_dft_kernel      |STFT| as a GEMM on the matrix pipe.  Row (b, t) of the A operand is the frame audio_b[t*hop - n_fft/2 ..
//                       + n_fft): no frame matrix exists, the staging addresses the waveform directly and the reflect padding of
//                       center=True is index arithmetic at the clip's own two ends.  The B operand is the [n_fft x 2 bins] cos | sin
//                       basis with the periodic Hann window folded in, built in fp64 on the host.  Arithmetic, tiling, LDS layout and
//                       MFMA fragments are those of gemm_f32.hip's fp16 two-term split (TERMS = 2: x ~ h + l / 2^11, three
//                       v_mfma_f32_32x32x16_f16 per 16-k block, fp32 accumulate; block tile 64 x 128 x 32, 2 x 2 waves); only the
//                       A staging and the epilogue differ.  Audio lies in [-1, 1] and the basis in [-1, 1], so the split's range
//                       guard (|x| <= 65504) cannot trip and this kernel carries no range flag.
//                       The panel's rows are ordered so that a wave's 64 columns are 32 bins' cos rows then the same bins' sin rows:
//                       re and im of one (frame, bin) are the same register index of the wave's two accumulator tiles, and the
//                       epilogue is sqrt(re^2 + im^2) on the accumulators, stored as magnitude rows [B * T_max][bins padded to 32].
//   mel_filterbank_kernel  the HTK triangular filterbank as a per-filter band sum (each bin feeds at most two filters: the dense
//                       [bins x n_mels] product would be 98 % zeros), log(clamp), the affine normalisation, the transpose to
//                       [B, n_mels, T_max] with zeros beyond a clip's frames, and the frame counts.  A tile of 16 frames' magnitudes
//                       goes through LDS (odd row stride), so both the global reads (along bins) and writes (along time) coalesce.
// Every sum runs in a fixed order over one row's own data: a clip's rows do not depend on its batch (ragged batch == batch of one,
// bit for bit).
#include "host.h"
#include "device_utils.h"

#include <cmath>
#include <cstring>
#include <vector>

namespace mtts {

using f32x16 = __attribute__((ext_vector_type(16))) float;
using f32x4 = __attribute__((ext_vector_type(4))) float;
using f16x8 = __attribute__((ext_vector_type(8))) _Float16;
using f16x4 = __attribute__((ext_vector_type(4))) _Float16;

constexpr int MEL_BM = 64;                 // frames per workgroup
constexpr int MEL_RS = 40;                 // LDS row stride in halves: 32 k + 16 B pad (gemm_f32.hip SPLIT_RS)
constexpr int MEL_FB_ROWS = 16;            // frames per workgroup of the filterbank kernel
constexpr float MEL_LOG_EPS = 1e-7f;       // reference mel_extractor.py: log(clamp(mel, 1e-7))

// Samples of clip b that enter the transform: its length held inside [0, ld] and trimmed to a multiple of hop.  A clip of at most
// n_fft / 2 samples has no reflect padding (torch raises there); it gets no frames and the host entry reports it.
__device__ __forceinline__ int clip_samples(const int64_t* __restrict__ lengths, int b, int64_t ld, int hop) {
    int64_t n = lengths[b];
    n = n < 0 ? 0 : (n > ld ? ld : n);
    return (int)(n / hop) * hop;
}
__device__ __forceinline__ int clip_frames(int L, int hop, int n_fft, int T_max) {
    if (L <= n_fft / 2) return 0;
    const int f = L / hop + 1;
    return f < T_max ? f : T_max;
}

struct MelDftArgs {
    const float* audio;          // [B][ld]
    const int64_t* lengths;      // [B] samples
    int64_t ld;
    int B, T_max, hop, n_fft;
    const _Float16* w16;         // basis panel [Np][n_fft / 32][h 32 | l 32] (kernels.h split_panel_f16_host)
    int Np;                      // panel rows: 2 * nbp rounded up to 128
    float* mag;                  // [B * T_max][nbp]
    int nbp;                     // bins padded to a multiple of 32
};

__global__ __launch_bounds__(256, 2) void mel_dft_kernel(const MelDftArgs p) {
    constexpr int BM = MEL_BM, BN = GEMM_BN, AR = BM / 32;
    constexpr int APLANE = BM * MEL_RS, BPLANE = BN * MEL_RS;
    __shared__ __attribute__((aligned(16))) _Float16 lds[2 * APLANE + 2 * BPLANE];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    const int M = p.B * p.T_max;
    const int n_tiles = p.Np / BN;
    const int m0 = (blockIdx.x / n_tiles) * BM;
    const int n0 = (blockIdx.x % n_tiles) * BN;
    const int Kp = p.n_fft;

    // ---- A staging: a thread owns rows lrow + 32 i and the 4 samples k = lq .. lq + 3 of every 32-wide k-step
    const int lrow = tid >> 3, lq = (tid & 7) * 4;
    const float* arow[AR];
    int aj0[AR], aL[AR];            // sample index of k = 0 (may be negative), trimmed clip length; aL = 0: row without a frame
#pragma unroll
    for (int i = 0; i < AR; ++i) {
        const int m = m0 + lrow + 32 * i;
        arow[i] = p.audio;
        aj0[i] = 0;
        aL[i] = 0;
        if (m < M) {
            const int b = m / p.T_max, t = m - b * p.T_max;
            const int L = clip_samples(p.lengths, b, p.ld, p.hop);
            if (t < clip_frames(L, p.hop, p.n_fft, p.T_max)) {
                arow[i] = p.audio + (size_t)b * p.ld;
                aj0[i] = t * p.hop - p.n_fft / 2;
                aL[i] = L;
            }
        }
    }
    const int wr8 = tid >> 3, wc8 = tid & 7;
    const _Float16* wrow8 = p.w16 + (size_t)(n0 + wr8) * Kp * 2 + wc8 * 8;

    f32x4 ra[AR];
    f16x8 rw[4];
    auto fetch = [&](int kt) {
#pragma unroll
        for (int i = 0; i < AR; ++i) {
            f32x4 v = {0.f, 0.f, 0.f, 0.f};
            const int L = aL[i];
            if (L > 0) {
                const int j = aj0[i] + kt * GEMM_BK + lq;
                if (j >= 0 && j + 3 < L && ((reinterpret_cast<uintptr_t>(arow[i] + j) & 15) == 0)) {
                    v = *reinterpret_cast<const f32x4*>(arow[i] + j);
                } else {
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        int q = j + e;
                        q = q < 0 ? -q : q;                       // reflect at the clip's start ...
                        q = q >= L ? 2 * (L - 1) - q : q;         // ... and at its (trimmed) end: L > n_fft / 2, one fold suffices
                        q = q < 0 ? 0 : (q >= L ? L - 1 : q);     // never leaves the clip whatever the arguments
                        v[e] = arow[i][q];
                    }
                }
            }
            ra[i] = v;
        }
        const _Float16* wp = wrow8 + (size_t)kt * GEMM_BK * 2;
#pragma unroll
        for (int jj = 0; jj < 4; ++jj) rw[jj] = *reinterpret_cast<const f16x8*>(wp + (size_t)(32 * jj) * Kp * 2);
    };
    _Float16* As = lds;
    _Float16* Bs = lds + 2 * APLANE;
    auto stage = [&]() {
#pragma unroll
        for (int i = 0; i < AR; ++i) {
            f16x4 h, l;
#pragma unroll
            for (int e = 0; e < 4; ++e) { _Float16 a, b; split_f16(ra[i][e], a, b); h[e] = a; l[e] = b; }
            _Float16* d = As + (lrow + 32 * i) * MEL_RS + lq;
            *reinterpret_cast<f16x4*>(d) = h;
            *reinterpret_cast<f16x4*>(d + APLANE) = l;
        }
#pragma unroll
        for (int jj = 0; jj < 4; ++jj)
            *reinterpret_cast<f16x8*>(Bs + (wc8 >> 2) * BPLANE + (wr8 + 32 * jj) * MEL_RS + (wc8 & 3) * 8) = rw[jj];
    };

    f32x16 acc[2], accx[2];
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) { acc[j][r] = 0.f; accx[j][r] = 0.f; }

    // Fragment of v_mfma_f32_32x32x16_f16: lane (r = lane & 31, h = lane >> 5) holds k = 8h .. 8h + 7 of a 16-wide k block.
    const int frag = (lane & 31) * MEL_RS + 8 * (lane >> 5);
    const _Float16* Aw = As + (wm * 32) * MEL_RS + frag;
    const _Float16* Bw = Bs + (wn * 64) * MEL_RS + frag;
    const int nk = Kp / GEMM_BK;
    fetch(0);
    for (int kt = 0; kt < nk; ++kt) {
        if (kt) __syncthreads();          // everyone finished reading the previous tile
        stage();
        __syncthreads();
        if (kt + 1 < nk) fetch(kt + 1);
#pragma unroll
        for (int kb = 0; kb < 2; ++kb) {
            const f16x8 ah = *reinterpret_cast<const f16x8*>(Aw + kb * 16);
            const f16x8 al = *reinterpret_cast<const f16x8*>(Aw + APLANE + kb * 16);
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const f16x8 bh = *reinterpret_cast<const f16x8*>(Bw + j * 32 * MEL_RS + kb * 16);
                const f16x8 bl = *reinterpret_cast<const f16x8*>(Bw + BPLANE + j * 32 * MEL_RS + kb * 16);
                accx[j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, bl, accx[j], 0, 0, 0);
                accx[j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(al, bh, accx[j], 0, 0, 0);
                acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, bh, acc[j], 0, 0, 0);
            }
        }
    }

    // ---- epilogue.  Accumulator map (32x32 tile): column = lane & 31, row = (r & 3) + 8 (r >> 2) + 4 (lane >> 5).  Tile 0 of the
    // wave holds Re, tile 1 Im of bin (n0 + wn * 64) / 2 + (lane & 31): the magnitude needs no exchange between lanes.
    const int bin = (n0 >> 1) + wn * 32 + (lane & 31);
    if (bin >= p.nbp) return;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int m = m0 + wm * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
        if (m >= M) continue;
        const float re = acc[0][r] + accx[0][r] * (1.0f / F16_RES_SCALE);
        const float im = acc[1][r] + accx[1][r] * (1.0f / F16_RES_SCALE);
        p.mag[(size_t)m * p.nbp + bin] = sqrtf(re * re + im * im);
    }
}

struct MelFbArgs {
    const float* mag;            // [B * T_max][nbp]
    const int64_t* lengths;
    int64_t ld;
    int B, T_max, hop, n_fft, nbp, n_mels;
    const int* fb_lo;            // [n_mels] first bin of filter m
    const int* fb_off;           // [n_mels + 1] its weights are fb_w[fb_off[m] .. fb_off[m + 1])
    const float* fb_w;
    float mel_mean, mel_std;
    float* mel;                  // [B][n_mels][T_max]
    int64_t* mel_lengths;        // [B]
};

__global__ __launch_bounds__(256) void mel_filterbank_kernel(const MelFbArgs p) {
    extern __shared__ __attribute__((aligned(16))) float tile[];     // [MEL_FB_ROWS][nbp + 1]
    const int b = blockIdx.y;
    const int t0 = blockIdx.x * MEL_FB_ROWS;
    const int L = clip_samples(p.lengths, b, p.ld, p.hop);
    const int frames = clip_frames(L, p.hop, p.n_fft, p.T_max);
    if (blockIdx.x == 0 && threadIdx.x == 0) p.mel_lengths[b] = frames;
    const int ldt = p.nbp + 1;
    const int rows = min(MEL_FB_ROWS, frames - t0);                  // rows of this tile that hold a frame (<= 0: none)
    for (int i = threadIdx.x; i < rows * p.nbp; i += 256) {
        const int r = i / p.nbp, k = i - r * p.nbp;
        tile[r * ldt + k] = p.mag[((size_t)b * p.T_max + t0 + r) * p.nbp + k];
    }
    __syncthreads();
    const int r = threadIdx.x & (MEL_FB_ROWS - 1);
    const int t = t0 + r;
    if (t >= p.T_max) return;
    for (int m = threadIdx.x / MEL_FB_ROWS; m < p.n_mels; m += 256 / MEL_FB_ROWS) {
        float out = 0.f;
        if (r < rows) {
            const int lo = p.fb_lo[m], o0 = p.fb_off[m], n = p.fb_off[m + 1] - o0;
            float s = 0.f;
            for (int k = 0; k < n; ++k) s += tile[r * ldt + lo + k] * p.fb_w[o0 + k];
            out = (logf(fmaxf(s, MEL_LOG_EPS)) - p.mel_mean) / p.mel_std;
        }
        p.mel[((size_t)b * p.n_mels + m) * p.T_max + t] = out;
    }
}

}  // namespace mtts

using namespace mtts;

// Host object: the tables in fp64 -> fp32 at create (no device needed), their device copies at the first forward.
struct mtts_melfe {
    int sample_rate = 24000, n_fft = 1024, n_mels = 100;
    int nb = 0, nbp = 0, Np = 0;
    std::vector<float> basis;        // [n_fft][2 * nb]: columns [0, nb) = w[n] cos(2 pi k n / N), [nb, 2 nb) = -w[n] sin(2 pi k n / N)
    std::vector<float> fb;           // [nb][n_mels] dense HTK filterbank (torchaudio.functional.melscale_fbanks, norm=None)
    std::vector<int> fb_lo, fb_off;
    std::vector<float> fb_w;
    void* d_blob = nullptr;          // device copy: basis image | fb_lo | fb_off | fb_w
    const _Float16* d_w16 = nullptr;
    const int* d_lo = nullptr;
    const int* d_off = nullptr;
    const float* d_w = nullptr;
    int device = -1;
};

static void melfe_tables(mtts_melfe* m) {
    const int N = m->n_fft, nb = m->nb;
    const double two_pi = 6.283185307179586476925286766559;
    m->basis.assign((size_t)N * 2 * nb, 0.f);
    for (int n = 0; n < N; ++n) {
        const double w = 0.5 - 0.5 * std::cos(two_pi * n / N);            // torch.hann_window(N), periodic
        for (int k = 0; k < nb; ++k) {
            const double ang = two_pi * (double)(((long long)k * n) % N) / (double)N;
            m->basis[(size_t)n * 2 * nb + k] = (float)(w * std::cos(ang));
            m->basis[(size_t)n * 2 * nb + nb + k] = (float)(-w * std::sin(ang));
        }
    }
    // HTK mel scale: mel(f) = 2595 log10(1 + f / 700); n_mels + 2 points equally spaced in mel between f_min = 0 and f_max = sr / 2,
    // triangles between neighbouring points, no area normalisation
    const double f_max = m->sample_rate / 2, m_max = 2595.0 * std::log10(1.0 + f_max / 700.0);
    std::vector<double> f_pts(m->n_mels + 2);
    for (int i = 0; i < m->n_mels + 2; ++i) f_pts[i] = 700.0 * (std::pow(10.0, (m_max * i / (m->n_mels + 1)) / 2595.0) - 1.0);
    m->fb.assign((size_t)nb * m->n_mels, 0.f);
    for (int k = 0; k < nb; ++k) {
        const double f = f_max * k / (nb - 1);                             // torch.linspace(0, sr // 2, n_freqs)
        for (int j = 0; j < m->n_mels; ++j) {
            const double down = (f - f_pts[j]) / (f_pts[j + 1] - f_pts[j]);
            const double up = (f_pts[j + 2] - f) / (f_pts[j + 2] - f_pts[j + 1]);
            const double v = std::fmin(down, up);
            m->fb[(size_t)k * m->n_mels + j] = (float)(v > 0.0 ? v : 0.0);
        }
    }
    m->fb_lo.assign(m->n_mels, 0);
    m->fb_off.assign(m->n_mels + 1, 0);
    m->fb_w.clear();
    for (int j = 0; j < m->n_mels; ++j) {
        int lo = nb, hi = -1;
        for (int k = 0; k < nb; ++k)
            if (m->fb[(size_t)k * m->n_mels + j] != 0.f) { lo = std::min(lo, k); hi = std::max(hi, k); }
        if (hi < lo) { lo = 0; hi = -1; }                                  // a filter narrower than one bin: no support
        m->fb_lo[j] = lo;
        m->fb_off[j] = (int)m->fb_w.size();
        for (int k = lo; k <= hi; ++k) m->fb_w.push_back(m->fb[(size_t)k * m->n_mels + j]);
    }
    m->fb_off[m->n_mels] = (int)m->fb_w.size();
}

// device copies of the tables (once per object; the basis goes through the GEMM panel layout and the fp16 two-term split)
static int melfe_upload(mtts_melfe* m) {
    if (m->d_blob) return 0;
    const int N = m->n_fft, nb = m->nb, nbp = m->nbp, Np = m->Np;
    std::vector<float> panel((size_t)Np * N, 0.f);
    for (int row = 0; row < 2 * nbp; ++row) {
        const int g = row / 64, within = row % 64, bin = g * 32 + (within & 31), part = within >> 5;
        if (bin >= nb) continue;
        for (int n = 0; n < N; ++n) panel[(size_t)row * N + n] = m->basis[(size_t)n * 2 * nb + part * nb + bin];
    }
    const size_t img_bytes = (size_t)Np * N * 2 * sizeof(uint16_t);
    auto up256 = [](size_t x) { return (x + 255) & ~size_t(255); };
    const size_t o_lo = up256(img_bytes), o_off = up256(o_lo + m->fb_lo.size() * 4), o_w = up256(o_off + m->fb_off.size() * 4);
    const size_t total = o_w + std::max<size_t>(m->fb_w.size(), 1) * 4;
    std::vector<unsigned char> blob(total, 0);
    split_panel_f16_host(panel.data(), panel.size(), reinterpret_cast<uint16_t*>(blob.data()));
    std::memcpy(blob.data() + o_lo, m->fb_lo.data(), m->fb_lo.size() * 4);
    std::memcpy(blob.data() + o_off, m->fb_off.data(), m->fb_off.size() * 4);
    std::memcpy(blob.data() + o_w, m->fb_w.data(), m->fb_w.size() * 4);
    void* d = nullptr;
    hipError_t e = hipMalloc(&d, total);
    if (e == hipSuccess) e = hipMemcpy(d, blob.data(), total, hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        if (d) (void)hipFree(d);
        set_error(std::string("mtts_melfe_forward: table upload: ") + hipGetErrorString(e));
        return -1;
    }
    (void)hipGetDevice(&m->device);
    m->d_blob = d;
    const char* base = static_cast<const char*>(d);
    m->d_w16 = reinterpret_cast<const _Float16*>(base);
    m->d_lo = reinterpret_cast<const int*>(base + o_lo);
    m->d_off = reinterpret_cast<const int*>(base + o_off);
    m->d_w = reinterpret_cast<const float*>(base + o_w);
    return 0;
}

extern "C" {

mtts_melfe* mtts_melfe_create(int sample_rate, int n_fft, int n_mels) {
    if (sample_rate < 2 || n_fft < 64 || n_fft > 2048 || (n_fft % GEMM_BK) || n_mels < 1 || n_mels > 4096) {
        set_error("mtts_melfe_create: unsupported shape (n_fft a multiple of 32 in [64, 2048], n_mels >= 1)");
        return nullptr;
    }
    mtts_melfe* m = new mtts_melfe();
    m->sample_rate = sample_rate; m->n_fft = n_fft; m->n_mels = n_mels;
    m->nb = n_fft / 2 + 1;
    m->nbp = round_up(m->nb, 32);
    m->Np = round_up(2 * m->nbp, GEMM_BN);
    melfe_tables(m);
    return m;
}
void mtts_melfe_destroy(mtts_melfe* m) {
    if (!m) return;
    if (m->d_blob) (void)hipFree(m->d_blob);
    delete m;
}
int mtts_melfe_n_bins(mtts_melfe* m) { return m ? m->nb : -1; }
int mtts_melfe_basis(mtts_melfe* m, float* h_out, int64_t numel) {
    if (!m || !h_out || numel != (int64_t)m->basis.size()) { set_error("mtts_melfe_basis: bad argument (numel = n_fft * 2 * bins)"); return -1; }
    std::memcpy(h_out, m->basis.data(), m->basis.size() * sizeof(float));
    return 0;
}
int mtts_melfe_filterbank(mtts_melfe* m, float* h_out, int64_t numel) {
    if (!m || !h_out || numel != (int64_t)m->fb.size()) { set_error("mtts_melfe_filterbank: bad argument (numel = bins * n_mels)"); return -1; }
    std::memcpy(h_out, m->fb.data(), m->fb.size() * sizeof(float));
    return 0;
}
int64_t mtts_melfe_workspace_bytes(mtts_melfe* m, int B, int64_t ld, int hop) {
    if (!m || B <= 0 || ld <= 0 || hop <= 0) { set_error("mtts_melfe_workspace_bytes: bad argument"); return -1; }
    const int64_t T = ld / hop + 1;
    return (int64_t)B * T * m->nbp * (int64_t)sizeof(float) + 256;
}
int mtts_melfe_forward(mtts_melfe* m, const float* d_audio, int64_t ld, const int64_t* d_lengths, int B, int hop, float mel_mean,
                       float mel_std, float* d_mel, int T_max, int64_t* d_mel_lengths, void* d_ws, int64_t ws_bytes, void* stream) {
    if (!m || !d_audio || !d_lengths || !d_mel || !d_mel_lengths || !d_ws) { set_error("mtts_melfe_forward: null argument"); return -1; }
    if (B <= 0 || B > 65535 || ld <= 0 || hop <= 0 || T_max <= 0) { set_error("mtts_melfe_forward: bad shape"); return -1; }
    if (ld <= m->n_fft / 2) { set_error("mtts_melfe_forward: clips must be longer than n_fft / 2 samples (reflect padding)"); return -1; }
    if (!(mel_std != 0.f)) { set_error("mtts_melfe_forward: mel_std must not be zero"); return -1; }
    // frames index samples in int32 inside the kernels
    if (ld > (int64_t)1 << 30 || (int64_t)B * T_max > (int64_t)1 << 30) { set_error("mtts_melfe_forward: batch too large"); return -1; }
    const int64_t need = (int64_t)B * T_max * m->nbp * (int64_t)sizeof(float);
    if (ws_bytes < need) { set_error("mtts_melfe_forward: workspace too small"); return -1; }
    if ((reinterpret_cast<uintptr_t>(d_ws) & 15) || (reinterpret_cast<uintptr_t>(d_audio) & 3)) { set_error("mtts_melfe_forward: misaligned buffer"); return -1; }
    if (melfe_upload(m)) return -1;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int M = B * T_max;
    MelDftArgs a;
    a.audio = d_audio; a.lengths = d_lengths; a.ld = ld; a.B = B; a.T_max = T_max; a.hop = hop; a.n_fft = m->n_fft;
    a.w16 = m->d_w16; a.Np = m->Np; a.mag = static_cast<float*>(d_ws); a.nbp = m->nbp;
    const int grid = ((M + MEL_BM - 1) / MEL_BM) * (m->Np / GEMM_BN);
    hipLaunchKernelGGL(mel_dft_kernel, dim3(grid), dim3(256), 0, s, a);
    if (launched("mel_dft_kernel")) return -1;
    MelFbArgs f;
    f.mag = a.mag; f.lengths = d_lengths; f.ld = ld; f.B = B; f.T_max = T_max; f.hop = hop; f.n_fft = m->n_fft; f.nbp = m->nbp;
    f.n_mels = m->n_mels; f.fb_lo = m->d_lo; f.fb_off = m->d_off; f.fb_w = m->d_w; f.mel_mean = mel_mean; f.mel_std = mel_std;
    f.mel = d_mel; f.mel_lengths = d_mel_lengths;
    const size_t lds = (size_t)MEL_FB_ROWS * (m->nbp + 1) * sizeof(float);      // <= 16 * 1057 * 4 = 67,648 B at n_fft 2048
    if (lds > 48 * 1024 &&
        launched("mel_filterbank_kernel", hipFuncSetAttribute(reinterpret_cast<const void*>(mel_filterbank_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds)))
        return -1;
    hipLaunchKernelGGL(mel_filterbank_kernel, dim3((T_max + MEL_FB_ROWS - 1) / MEL_FB_ROWS, B), dim3(256), lds, s, f);
    return launched("mel_filterbank_kernel");
}

}  // extern "C"
