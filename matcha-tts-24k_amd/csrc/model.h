// Host-side data model of the path: packed weights, run-time switches and the contexts behind the opaque handles of
// include/mtts.h.  The launch sequences of TextEncoder.forward, Decoder.forward and BASECFM.solve are in encoder.hip and
// decoder.hip (reference files cited at each function), the packing in pack.hip.
#pragma once
#include <atomic>
#include <map>
#include <string>
#include <vector>

#include "../../include/mtts.h"
#include "kernels.h"

namespace mtts {

void set_error(const std::string& msg);
const char* get_error();

// One GEMM-ready weight panel inside the device image (offsets in floats).
struct Panel {
    size_t w = 0, b = 0;
    size_t w16 = 0;            // bf16 split planes [3][Np][Kp] (offset in floats), present when the context uses a split mode
    bool has_bias = false;
    size_t wsum = 0;           // [Np] row sums of the panel (fp16-split mode): LayerNorm in the P16 GEMM's epilogue
    size_t wh16 = 0;           // 16-bit storage mode: the fp16 head plane alone [Np][Kp] halves (offset in floats)
    int N = 0, C = 0, ntaps = 1, ktap = 0;
};
struct Vec { size_t off = 0; int n = 0; };

struct ResnetW {
    Panel conv1, conv2, res;
    Vec gn1_g, gn1_b, gn2_g, gn2_b;
    Vec gn1_bs, gn2_bs;       // per GroupNorm group (mean, sum of squared deviations) of conv1's / conv2's bias row (folded padding)
    int cin = 0, cout = 0;
    int tb_off = 0;           // column offset of this block's time bias inside the per-evaluation bias row
};
struct TBlockW {
    Panel qkv, out, ff1, ff2;  // LayerNorm affines folded into qkv / ff1
    Vec alpha_exp, inv_beta;
    // fragment stream of the block's row-local chain (kernels.h ChainArgs; tblock_chain.hip): out-projection, FeedForward and --
    // when another block of the same run follows -- that block's q|k|v projection.  0 frags = chain not packed for this block.
    size_t chain = 0;          // offset in the image (floats)
    long chain_frags = 0;
    size_t chain_consts = 0;   // the chain kernel's column constants as one block of 18 C floats (kernels.h ChainArgs::consts)
    int chain_ch = 0;          // hidden chunk the stream was packed for
    int chain_nqkv = 0;        // width of the q|k|v part (0: none)
    int next = -1;             // index of the block whose q|k|v the chain computes
    size_t chain_pair = 0;     // the same chain as TWO half streams per wave (kernels.h ChainArgs::pair), offset in floats
    long chain_pair_frags = 0; // fragments per (half, wave); 0 = not packed
    bool chain_h16 = false;    // 16-bit storage modes: `chain` is a ONE-plane stream (kernels.h ChainH16Args; tblock_chain_h16.hip), fp16 or bfloat16
};
struct DecW {
    Vec freqs;
    Panel t1, t2, tmlp;        // time MLP and the concatenated per-ResNet Linear(Mish(t))
    int tb_total = 0;
    std::vector<ResnetW> res;            // down..., mid..., up... in execution order
    std::vector<TBlockW> tb;             // n_blocks per resnet, execution order
    std::vector<Panel> down;             // per level: stride-2 conv (or k3 conv at the last level)
    std::vector<Panel> up_even, up_odd;  // ConvTranspose phases (levels-1 entries)
    Panel up_last;                       // k3 conv of the last up block
    Panel final_conv, final_proj;
    Vec fgn_g, fgn_b, fgn_bs;
};
struct EncW {
    Vec emb, spk_enc, spk_dur, rope_cos, rope_sin;
    std::vector<Panel> pre_conv;
    std::vector<Vec> pre_g, pre_b;
    Panel pre_proj;
    std::vector<Panel> qkv, o, ffn1, ffn2;
    std::vector<Vec> n1_g, n1_b, n2_g, n2_b;
    Panel pm0, pm2;
    Panel film;
    std::vector<Panel> dp_conv;
    std::vector<Vec> dp_g, dp_b;
    Panel dp_proj;
};

struct VocosW {
    Panel embed, head, basis;
    Vec norm_g, norm_b, fin_g, fin_b, window;
    std::vector<Vec> dw_w, dw_b, ln_g, ln_b;
    std::vector<Panel> pw1, pw2;
};

// Backward panels of the speaker-row gradient (spk_grad.hip): transposed / tap-reversed copies of the text encoder's panels behind the
// speaker rows, packed on demand into a buffer of their own (mtts_ctx::grad), never into the weight image.
struct SpkGradW {
    Panel pm2T, pm0T;
    std::vector<Panel> oT, qkvT, ffn2T, ffn1T;
    std::vector<Panel> dp_convT;   // [0] is empty: the first duration-predictor layer reads x.detach()
    Panel filmT;                   // spk_proj transposed
    Vec dp_proj;                   // the duration predictor's output projection [dp_filter] (one output channel: an outer product)
};

// The duration predictor's training component (dp_grad.hip): its forward panels, LayerNorm affines and output projection, and the
// transposed, tap-reversed panels of its walk back, packed from one flat parameter vector into a buffer of their own (mtts_ctx::dptrain).
struct DpTrainW {
    Panel film, filmT;             // spk_proj and its transpose
    std::vector<Panel> conv, convT;   // convT[0] is empty: the first layer reads x.detach()
    std::vector<Vec> gamma, beta;
    Vec proj_w, proj_b;            // [dp_filter], [1]
    Panel proj;                    // the same projection as a GEMM panel (the forward)
};

struct StyleW {
    std::vector<Panel> convs;      // Conv1d(k5, pad 2) of each layer
    Vec proj_w, proj_b;            // [2 E][hidden] = proj_enc rows then proj_dur rows, [2 E]
};
// Backward panels of the style encoder's data gradient (style_grad.hip): the transposed, tap-reversed convs of layers >= 1, packed on
// demand into a buffer of their own (mtts_style::grad) as SpkGradW's are.
struct StyleGradW {
    std::vector<Panel> convT;      // [0] is empty: the first layer's input is the mel, which gets no gradient
};

// The library's run-time switches with their defaults.  read_switches() (model.hip) is the only reader of the environment:
// mtts_create keeps its result in the context, which never looks at the environment again; the context-free test entries
// (mtts_chain_plan, mtts_tblock_chain*, mtts_gemm_terms(NULL), mtts_gemm_f32 with terms < 0) call it per call.
struct Switches {
    int gemm_terms = 2;         // MTTS_GEMM_TERMS 0 / 2 / 3 / 6: GEMM arithmetic of new contexts (gemm_f32.hip) -- 2 fp16 two-term split with scaled
                                // residual, 6 bf16 three-term split (both fp32-equivalent), 0 native fp32 MFMA, 3 bf16 two-term split (looser, opt-in)
    int arith16 = 0;            // MTTS_GEMM_TERMS 1 / 16 / 17: gemm_terms 2 with that 16-bit mode of the estimator (include/mtts.h mtts_set_arithmetic)
    bool p16_on = true;         // MTTS_P16=0: fp16-split mode without P16 images between the kernels
    bool chain_on = true;       // MTTS_CHAIN=0: a transformer block's row-local part as four GEMM launches instead of the chain launch (tblock_chain.hip)
    int chain_ch = 256;         // MTTS_CHAIN_CH 128 / 256: hidden chunk of the chain's FeedForward at width 384
    int chain_qb = 0;           // MTTS_CHAIN_QB: rows per workgroup of the chain launch (0 = by shape, chain_plan)
    int chain_min_rows = 5761;  // MTTS_CHAIN_MIN_ROWS: estimator rows (B * T of a level) from which the chain replaces the four GEMM launches = where the pair
                                // form's residency bound (120 tiles of 48 rows) ends; at width 384 -- 10304 rows: 138 vs ~160 us per block, 5152 rows:
                                // 100 vs ~92 us (profiles/r03_chain_*)
    bool pair_on = true;        // MTTS_CHAIN_PAIR=0: no pair form of the chain launch below chain_min_rows (mtts_create also clears it on less than the whole chip)
    int pair_min_rows = 3000;   // MTTS_CHAIN_PAIR_MIN_ROWS: rows from which the pair form is taken (3864 rows: -0.3..0.5 ms per step, 2576 rows: +0.3;
                                // profiles/r03_pair_ab.log)
    int chain_pf = 16;          // MTTS_CHAIN_PF 0..64: prefetch workgroups of the chain launch, two per XCD (one alone takes ~93 us for the 7 MB stream and
                                // is the tail of the launches without a q|k|v phase: 16 instead of 8 = -0.15 ms of GEMM time per step); 0: none
    bool chain16_on = true;     // MTTS_CHAIN16=0: the 16-bit storage modes keep the four tiled H16 launches per transformer block (MTTS_CHAIN=0 does the same);
                                // 1: the one-plane chain launch (tblock_chain_h16.hip) at or above chain16_min_rows
    int chain16_min_rows = 5000;// MTTS_CHAIN16_MIN_ROWS: estimator rows (B * T of a level) from which the one-plane chain replaces the four tiled H16 launches:
                                // at width 384 the launch alone takes 47 / 63 / 100 us at 5152 / 10304 / 20608 rows; B = 8 (5152 / 2576 rows) is within the run-to-run
                                // spread either way, B = 16 -0.3..0.5 ms, B = 32 -2.3 ms per step (profiles/r06_chain_h16.md)
    int chain16_qb = 0;         // MTTS_CHAIN16_QB 32 / 64 / 96: rows per workgroup of the one-plane chain (0 = by shape, chain16_plan)
    int resnet_fuse = 3;        // MTTS_RESNET_FUSE: Block1D as one conv + GroupNorm + Mish launch where it applies (resnet_conv.hip) -- bit 0 the first Block1D
                                // of a ResNet block and the decoder's final one, bit 1 the second, bit 2 lifts the batch gate; 0 = the tiled launches
    int store_wt = 31;          // MTTS_STORE_WT, bits of kernels.h StoreWt: the families whose P16 output images leave their epilogues with 16-byte write-through
                                // stores (device_utils.h store16) instead of staying dirty in the L2s until the launch's end -- 1 tiled P16 GEMM, 2 conv_gn, 4 the
                                // chain's x_out, 8 the chain's q|k|v (lanes paired for 16 bytes), 16 attention (lanes paired).  Bench steps, same box, alternated
                                // (profiles/r26_store_wt.md): all bits against 0 -0.49 / -0.62 ms (5 of 5 and 4 of 4 pairs, rocprofv3: 0.4..1.7 us less per launch
                                // of every family); all bits but one against all: +0.24 / +0.15 / +0.16 / +0.29 / +0.18 ms in that order; one bit alone against 0:
                                // -0.12 / 0.00 / +0.21 / +0.05 / -0.05 ms, all inside the spread -- the bits pay together, not one by one.  Never changes a value.
};
Switches read_switches();

struct ProfRec { hipEvent_t e0, e1; int klass; double flops, bytes; std::string tag; };      // tag: a copy (launchers reuse their buffers)

}  // namespace mtts

// What the three weighted objects (mtts_ctx, mtts_vocos, mtts_style) share, and all that the packer (host.h Packer) and the launch
// wrappers (host.h run_gemm, LAUNCH) may depend on: the weight image and its life cycle, the arithmetic the panels are packed for,
// the state of the call being enqueued, the profiler.
namespace mtts {
struct Component {
    std::map<std::string, std::vector<float>> raw;
    std::vector<float> image;     // host staging of the packed device image
    float* d_image = nullptr;     // caller-owned device buffer
    bool packed = false, uploaded = false;
    bool weights_saturate = false;      // fp16-split mode: a weight beyond +-65504 was met while packing
    int gemm_terms = 6;           // 0: fp32 MFMA, 6 / 3: split-bf16 MFMA, 2: split-fp16 (MTTS_GEMM_TERMS; see gemm_f32.hip)
    bool half16 = false;          // 16-bit storage mode (mtts_set_arithmetic(ctx, 16) / MTTS_GEMM_TERMS=16): the estimator's images are
                                  // single fp16 planes, one MFMA per MAC (BASELINE config #3); everything else as for terms 2
    bool bf16 = false;            // ... with bfloat16 planes (mtts_set_arithmetic(ctx, 17) / MTTS_GEMM_TERMS=17; half16 is set as well)
    bool fast16 = false;          // mtts_set_arithmetic(ctx, 1) / MTTS_GEMM_TERMS=1: the estimator's P16 kernels multiply the fp16 heads only
    unsigned int* cur_flag = nullptr;   // range flag of the call being enqueued: first word of its workspace (include/mtts.h)
    bool half_now = false;        // set while the estimator's launches are being enqueued in that mode
    int store_wt = 0;             // Switches::store_wt of the context (0 for the Vocos head and the style encoder: plain stores)
    // profiling
    bool prof_on = false;
    std::vector<ProfRec> prof;
    std::vector<hipEvent_t> ev_pool;
    size_t ev_used = 0;
    Component() = default;
    Component(const Component&) = delete;
    Component& operator=(const Component&) = delete;
    ~Component() { for (hipEvent_t e : ev_pool) (void)hipEventDestroy(e); }
};
}  // namespace mtts

struct mtts_ctx : mtts::Component {
    mtts_config cfg;
    const int* d_tlen = nullptr;  // per-utterance frame limits of the next estimator calls (mtts_set_frame_limits), device [B]
    mtts::Switches sw;            // the run-time switches as mtts_create read them
    unsigned int pair_epoch = 0;  // flag value of the latest pair launch (unique per launch)
    mtts::DecW dec;
    mtts::EncW enc;
    // one thread at a time: the path's entry points hold this while they enqueue (per-call state: cur_flag, half_now,
    // d_tlen, prof); a second thread's call fails instead of interleaving its launches with another call's flag pointer
    std::atomic<bool> in_use{false};
    // speaker-row gradient (spk_grad.hip): the backward panels' own image (native fp32 MFMA: gemm_terms 0) and their offsets
    mtts::Component grad;
    mtts::SpkGradW gradw;
    // duration-predictor training (dp_grad.hip): the predictor's own small component (native fp32 MFMA), repacked from the flat
    // parameter vector every step; touches neither the image above nor `grad`
    mtts::Component dptrain;
    mtts::DpTrainW dptw;
};

// Vocos-24k head: its own weight image and context (the reference loads it as a separate object,
// reference matcha/inference.py:223-231).
struct mtts_vocos : mtts::Component {
    int n_mels = 100, dim = 512, inter = 1536, layers = 8, n_fft = 1024, hop = 256;
    int ld_spec = 0, im_off = 0;     // head output row: [Re/logmag 0..n_fft/2 | pad | Im/phase at im_off.. | pad]
    mtts::VocosW w;
};

// Style encoder (reference matcha/models/style_encoder.py:42-72): its own weight image and context, as the Vocos head.
struct mtts_style : mtts::Component {
    int n_feats = 100, hidden = 256, layers = 4, emb = 96;
    mtts::StyleW w;
    // parameter gradients (style_grad.hip): the backward panels' own image (native fp32 MFMA: gemm_terms 0) and their offsets
    mtts::Component grad;
    mtts::StyleGradW gradw;
};
