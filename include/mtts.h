/*
 * mtts.h -- C ABI of libmtts_hip.so: the MI355X (gfx950) implementation of the mel-synthesis
 * hot path of faltiska/Matcha-TTS-24k.
 *
 * The reference has no native code and no FFI on this path: its boundary is the Python module
 * matcha/inference.py.  This header is what a Python (ctypes) or C++ host
 * binds instead of calling PyTorch ops; each entry point cites the reference function it replaces
 * (paths relative to the reference repository root).
 *
 * Conventions
 *   - every pointer named d_* is a DEVICE pointer (fp32 unless stated); h_* is a HOST pointer
 *   - `stream` is a hipStream_t passed as void* (e.g. torch.cuda.current_stream().cuda_stream)
 *   - functions return 0 on success, <0 on error; mtts_last_error() gives a thread-local message
 *   - launch functions never allocate, never synchronise and never touch the default stream:
 *     scratch memory is a caller-provided workspace sized by the matching *_workspace_bytes()
 *   - tensors use the reference's layouts at the boundary: activations [B, C, T] ("channels first"),
 *     ids/lengths int64
 */
#ifndef MTTS_H
#define MTTS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MTTS_ABI_VERSION 2
/* bumped whenever the packed weight image changes layout (invalidates mtts_export_weights caches) */
#define MTTS_IMAGE_REVISION 7

typedef struct mtts_ctx mtts_ctx;

/* Architecture of the path; mirrors the checkpoint's hyper_parameters
 * (reference matcha/inference.py:45-55, configs/experiment/v20.yaml:17-63). */
typedef struct mtts_config {
    int32_t n_feats;        /* mel bins (100) */
    int32_t n_spks;
    int32_t spk_emb_dim;    /* 96 */
    int32_t n_vocab;        /* 600 */
    /* text encoder, reference text_encoder.py:319-373 */
    int32_t enc_channels;   /* 192; hidden = enc_channels + spk_emb_dim */
    int32_t enc_filter;     /* 1152 */
    int32_t enc_heads;      /* 6 */
    int32_t enc_layers;     /* 4 */
    int32_t enc_kernel;     /* 5 */
    int32_t prenet_layers;  /* 6 */
    int32_t prenet_kernel;  /* 3 */
    int32_t dp_filter;      /* 96 */
    int32_t dp_kernel;      /* 5 */
    int32_t dp_layers;      /* 4 */
    /* decoder, reference decoder.py:202-310 */
    int32_t dec_levels;     /* len(channels) == 2 */
    int32_t dec_channels[4];
    int32_t dec_head_dim;   /* 64 */
    int32_t dec_heads;      /* 6 */
    int32_t dec_n_blocks;   /* 2 */
    int32_t dec_mid_blocks; /* 2 */
} mtts_config;

enum { MTTS_SOLVER_EULER = 0, MTTS_SOLVER_MIDPOINT = 1, MTTS_SOLVER_RK4 = 2 };

/* ---------------------------------------------------------------- library / context */
int mtts_abi_version(void);
const char* mtts_last_error(void);

/* Create a context for one architecture.  Host-side only (no device work). */
mtts_ctx* mtts_create(const mtts_config* cfg);
void mtts_destroy(mtts_ctx* ctx);

/* Register one tensor of the reference state dict by its key, e.g.
 * "decoder.estimator.down_blocks.0.0.block1.block.0.weight".  h_data: host fp32, copied.
 * Replaces nn.Module.load_state_dict (reference inference.py:186-197). */
int mtts_set_tensor(mtts_ctx* ctx, const char* key, const float* h_data, int64_t numel);

/* Threading: a context carries per-call state (the call's range-flag pointer, frame limits, the profiler's records): one thread
 * drives a context at a time -- use one context per serving worker / stream.  The path's entry points (mtts_text_encoder_forward,
 * mtts_decoder_forward, mtts_cfm_solve*) enforce it: a call that finds the context held by another thread returns -1 ("in use
 * by another thread") instead of interleaving.  Only mtts_last_error is thread-local. */

/* (test hook: holds the context as a path entry point does for `ms` milliseconds; a concurrent entry-point call fails) */
int mtts_debug_hold(mtts_ctx* ctx, int ms);

/* Packed-image cache ("pre-packed MFMA weight layouts cached beside the converted checkpoint").
 * mtts_weights_signature: a string naming everything the image layout depends on (ABI and image revision, architecture,
 * arithmetic, layout switches); mtts_export_weights copies the packed image (mtts_weights_bytes) to host memory;
 * mtts_import_weights adopts such an image in a context with the same signature whose tensors have been registered
 * (mtts_set_tensor) -- it runs the layout pass only, not the splitting / fragment packing (~7 s at production size).
 * `saturates`: the range-guard finding of the packing pass (mtts_weights_saturate), stored with the image. */
int mtts_weights_signature(mtts_ctx* ctx, char* buf, int64_t n);
int mtts_export_weights(mtts_ctx* ctx, void* h_dst, int64_t bytes, int* saturates);
int mtts_import_weights(mtts_ctx* ctx, const void* h_src, int64_t bytes, int saturates);

/* After all tensors are registered: size of the packed device image, then pack + upload it
 * (GEMM-ready [N][K] panels, conv taps unrolled along K, LayerNorm affine folded into the
 * following projection, exp() of the SnakeBeta parameters).  Synchronous; load time only. */
int64_t mtts_weights_bytes(mtts_ctx* ctx);
int mtts_upload_weights(mtts_ctx* ctx, void* d_weights, int64_t bytes);

/* ---------------------------------------------------------------- the path */

/* TextEncoder.forward -- reference matcha/models/components/text_encoder.py:375-406.
 * d_x [B,Tx] int64, d_x_lengths [B] int64, d_e_enc/d_e_dur [B,spk_emb_dim].
 * Outputs: d_mu_x [B,n_feats,Tx], d_logw [B,1,Tx], d_x_mask [B,1,Tx] (float 0/1). */
int64_t mtts_encoder_workspace_bytes(mtts_ctx* ctx, int B, int Tx);
int mtts_text_encoder_forward(mtts_ctx* ctx, const int64_t* d_x, const int64_t* d_x_lengths, const float* d_e_enc,
                              const float* d_e_dur, int B, int Tx, float* d_mu_x, float* d_logw, float* d_x_mask,
                              void* d_ws, int64_t ws_bytes, void* stream);

/* Speaker table lookup -- reference inference.py:115-121 (table: 0 = enc, 1 = dur); d_ids [B] int64. */
int mtts_speaker_embedding(mtts_ctx* ctx, int table, const int64_t* d_ids, int B, float* d_out, void* stream);

/* Durations -- reference inference.py:127-146:
 * round((exp(logw)-2)*mask*scale_correction*length_scale).clamp(min=1)*mask, their inclusive cumulative sum and the
 * per-utterance fine length clamp_min(sum,1).
 * d_durations [B,Tx] f32, d_cum [B,Tx] int32, d_y_fine_lengths [B] int64. */
int mtts_durations(const float* d_logw, const float* d_x_mask, float scale_correction, float length_scale, int B, int Tx,
                   float* d_durations, int32_t* d_cum, int64_t* d_y_fine_lengths, void* stream);

/* The same with one (scale_correction, length_scale) pair per utterance, device float [B] each: a serving batch mixes voices
 * (reference inference.py:16-32 VOICES[..]["scale_correction"], server.py:111-115) and client speeds. */
int mtts_durations_per_utterance(const float* d_logw, const float* d_x_mask, const float* d_scale_correction,
                                 const float* d_length_scale, int B, int Tx, float* d_durations, int32_t* d_cum,
                                 int64_t* d_y_fine_lengths, void* stream);

/* Durations the caller brings instead of the predictor's (a measured alignment from mtts_mas, a copied rhythm): the tail of
 * reference inference.py:127-146 with the predictor's term replaced,
 *   d = clamp_min(round(d_dur * length_scale), 0) * mask        (a zero is allowed: mtts_align_pool skips a token without frames)
 * and the same inclusive cumulative sum and fine length clamp_min(sum, 1) as mtts_durations (one scan, shared).  scale_correction
 * has no part in it: it corrects the predictor.  d_dur [B,Tx] f32 (fine frames); d_length_scale: device float [B] or NULL
 * (then length_scale holds for all).  d_given_rows: device int32 [B] or NULL; row b with d_given_rows[b] == 0 keeps what
 * d_durations already holds -- call mtts_durations first, then this, and one batch mixes given and predicted rows without a host
 * read.  Feeding mtts_durations' own d_durations back with length_scale 1 reproduces its d_cum and d_y_fine_lengths exactly. */
int mtts_durations_given(const float* d_dur, const float* d_x_mask, float length_scale, const float* d_length_scale,
                         const int32_t* d_given_rows, int B, int Tx, float* d_durations, int32_t* d_cum,
                         int64_t* d_y_fine_lengths, void* stream);

/* Shaped durations: one launch for a batch that mixes predicted and given rows, with a rate and an extension per token -- what SSML
 * calls <prosody rate> and a lengthened syllable -- ahead of the same scan.  The entries above stay as they are.
 *   d_scale_correction, d_length_scale   device float [B] each
 *   d_given        device float [B,Tx] (fine frames) or NULL;  d_given_rows: device int32 [B] or NULL.  Row b is GIVEN when d_given is
 *                  there and d_given_rows is NULL or d_given_rows[b] != 0; every other row is PREDICTED from d_logw (which may be NULL
 *                  only when every row is given)
 *   d_token_scale  device float [B,Tx] or NULL (s = 1);  d_token_extend: device float [B,Tx], fine frames, or NULL (a = 0)
 * fp32, every operation rounded once, no FMA; m = mask, sc / ls the row's factors:
 *   s = NaN ? 1 : min(max(s, 0), 16);   a = NaN ? 0 : min(max(a, -4096), 4096)      (so no input gives a negative or unbounded length)
 *   predicted:  v = (expf(logw) - 2) * m;  v = v * sc;  v = v * ls;  v = v * s;  v = v + a;  d = fmaxf(rintf(v), s == 0 ? 0 : 1) * m
 *   given:      v = given * ls;                                      v = v * s;  v = v + a;  d = fmaxf(rintf(v), 0) * m
 * A scale of exactly 0 (after the clamp) drops a predicted token, as a given zero does.  With s == 1 and a == 0 the two extra operations
 * are exact and all three outputs equal those of mtts_durations_per_utterance (mtts_durations_given for given rows) bit for bit.
 * Outputs as mtts_durations.  Returns -1 and launches nothing for a null pointer it needs, d_given_rows without d_given, B < 1, Tx < 1. */
int mtts_durations_shaped(const float* d_logw, const float* d_x_mask, const float* d_scale_correction, const float* d_length_scale,
                          const float* d_given, const int32_t* d_given_rows, const float* d_token_scale, const float* d_token_extend,
                          int B, int Tx, float* d_durations, int32_t* d_cum, int64_t* d_y_fine_lengths, void* stream);

/* generate_path + matmul + downsample + sequence_mask -- reference inference.py:146-167,
 * utils/model.py:7-9,24-40,57-68.  T_pad = fix_len_compatibility(max fine length) (host decides it).
 * Outputs: d_mu_y [B,n_feats,T_pad], d_y_mask [B,1,T_pad], d_y_lengths [B] int64. */
int mtts_align_pool(const float* d_mu_x, const int32_t* d_cum, const int64_t* d_y_fine_lengths, int B, int n_feats,
                    int Tx, int T_pad, float* d_mu_y, float* d_y_mask, int64_t* d_y_lengths, void* stream);

/* Per-request padding inside a batch.  The reference computes T_pad, the GroupNorm statistics, the attention key set and
 * the noise shape from the longest utterance of the call (inference.py:147-148, decoder.py:32-45, transformer.py:249-261),
 * so an utterance's mel depends on what it was batched with.  With d_t_len[b] (device int32, even, <= T) set, the next
 * mtts_decoder_forward / mtts_cfm_solve calls treat utterance b as if only frames [0, d_t_len[b]) existed: GroupNorm
 * statistics and attention keys stop there (convolutions already read masked zeros beyond it), so every utterance of a
 * ragged batch gets the values of a batch-of-one call (up to the summation order of differently shaped tiles).  NULL restores whole-batch padding.  The pointer is kept,
 * not copied: it must stay valid until replaced. */
int mtts_set_frame_limits(mtts_ctx* ctx, const int32_t* d_t_len);

/* Decoder.forward -- reference matcha/models/components/decoder.py:359-426 (one evaluation of the velocity field).
 * d_x, d_mu, d_out [B,n_feats,T]; d_mask [B,1,T]; t scalar. */
int64_t mtts_decoder_workspace_bytes(mtts_ctx* ctx, int B, int T);
int mtts_decoder_forward(mtts_ctx* ctx, const float* d_x, const float* d_mask, const float* d_mu, float t, int B, int T,
                         float* d_out, void* d_ws, int64_t ws_bytes, void* stream);
/* The same evaluation with ONE TIME PER UTTERANCE, d_t = device fp32 [B] -- what BASECFM.compute_loss asks of the estimator
 * (reference flow_matching.py:97, t of shape [B]).  It is mtts_decoder_forward with the time embedding made for B rows and every
 * ResNet block adding its utterance's own bias row, as mtts_cfm_step does for stages * B rows.  Same workspace size. */
int mtts_decoder_forward_rows(mtts_ctx* ctx, const float* d_x, const float* d_mask, const float* d_mu, const float* d_t, int B, int T,
                              float* d_out, void* d_ws, int64_t ws_bytes, void* stream);

/* BASECFM.compute_loss -- reference matcha/models/components/flow_matching.py:65-107 -- forward only, with its two random draws
 * given by the caller: d_t device fp32 [B] (the reference draws torch.rand([B])), d_noise [B,n_feats,T] (randn_like(x1)).
 *   x0 = noise (+ mu if add_mu: use_mu_prior);  y_t = (1 - (1 - sigma_min) t_b) * x0 + t_b * x1;  u = x1 - (1 - sigma_min) * x0,
 *   in that operation order, with (1 - sigma_min) rounded to fp32 once as the reference's Python scalar is;
 *   pred = estimator(y_t, mask, mu, t): ONE evaluation, utterance b at time t_b;
 *   d_sq_sum[b] = sum over (f, t) of (pred * mask - u * mask)^2                       (fp32 [B])
 * The reference's loss is sum_b d_sq_sum[b] / (sum(mask) * n_feats); utterance b's own is d_sq_sum[b] / (sum(mask[b]) * n_feats).
 * u is never stored; y_t is written straight into the estimator's state rows.  d_pred [B,n_feats,T] or NULL: the estimator's
 * output (already masked by Decoder.forward), for parity tests.  d_x1, d_mu [B,n_feats,T]; d_mask [B,1,T].
 * Every sum has a fixed order (no floating-point atomics): two calls give the same bits.  mtts_set_frame_limits composes; range
 * guard, pair time-out word and mtts_prof_* as for any estimator call.  Workspace: mtts_decoder_workspace_bytes(ctx, B, T). */
int mtts_cfm_loss(mtts_ctx* ctx, const float* d_x1, const float* d_mu, const float* d_mask, const float* d_noise, const float* d_t,
                  int add_mu, float sigma_min, int B, int T, float* d_sq_sum, float* d_pred, void* d_ws, int64_t ws_bytes, void* stream);

/* BASECFM.solve -- reference matcha/models/components/flow_matching.py:60-63 + torchdiffeq fixed-grid odeint
 * (euler / midpoint / rk4 = 3/8 rule) over the grid h_t_span[0..n_steps].
 * d_x0 [B,n_feats,T] initial state; if add_mu != 0 the state starts at d_x0 + d_mu (use_mu_prior,
 * flow_matching.py:52-55).  d_out [B,n_feats,T_out] receives state[:, :, :T_out]*out_scale + out_shift
 * (the slice and denormalize of reference inference.py:170-172; pass T_out=T, 1, 0 for the raw state). */
int mtts_cfm_solve(mtts_ctx* ctx, const float* d_x0, const float* d_mu, const float* d_mask, int add_mu,
                   const float* h_t_span, int n_steps, int solver, int B, int T, float* d_out, int T_out,
                   float out_scale, float out_shift, void* d_ws, int64_t ws_bytes, void* stream);

/* The same solve on FOLDED padding -- what MatchaTTSInfer.synthesise runs (reference matcha/inference.py:146-170 pads the
 * decoder to T = roundup_even(longest fine length), i.e. twice the valid mel length, and GroupNorm / attention see those
 * frames: decoder.py:32-45, transformer.py:249-261).  With prefix masks (frame t of utterance b valid iff t < d_y_lengths[b])
 * every padded frame of a U-Net level is the same row: convolutions read `x * mask` (decoder.py:43,62), so beyond the first
 * padded frame a conv output is its bias, a ResNet output is the residual conv's bias, and transformer blocks act row-wise with
 * keys that carry no position.  The estimator therefore holds, per utterance and level l, the ceil(y_len / 2^l) valid rows plus
 * ONE row standing for the n_pad padded ones: attention gives that key the bias ln(n_pad) (n_pad reference keys of bias +0),
 * GroupNorm merges the remaining n_pad - 1 bias rows in closed form.  Same results as mtts_cfm_solve on the full [B, n_feats, T]
 * problem up to summation order; T_fold / T of the arithmetic.
 *   d_x0, d_mu [B, n_feats, T] as for mtts_cfm_solve (only frames < T_fold are read; frames of the state at or beyond an
 *   utterance's own length pass through unchanged, as in the reference); d_y_lengths device int64 [B], all <= y_max < T.
 *   T_fold: rows held per utterance, a multiple of 2^(levels-1) with mtts_fold_rows(ctx, y_max, 1) <= T_fold <= T;
 *   mtts_fold_rows(ctx, y_max, align) = roundup(ceil(y_max / 2^(levels-1)) + 1, align) * 2^(levels-1) (align 32 keeps whole
 *   wave tiles per utterance for the fused GroupNorm statistics).  Workspace: mtts_decoder_workspace_bytes(ctx, B, T_fold).
 *   mtts_set_frame_limits composes: utterance b's reference length is then d_t_len[b] instead of T. */
int mtts_fold_rows(mtts_ctx* ctx, int y_max, int align);
int mtts_cfm_solve_folded(mtts_ctx* ctx, const float* d_x0, const float* d_mu, const int64_t* d_y_lengths, int y_max, int add_mu,
                          const float* h_t_span, int n_steps, int solver, int B, int T, int T_fold, float* d_out, int T_out,
                          float out_scale, float out_shift, void* d_ws, int64_t ws_bytes, void* stream);

/* ONE step of that solve for B utterances that sit at DIFFERENT points of their own grids -- the iteration a serving scheduler
 * batches at (batcher.StepBatcher): requests join and leave between two calls.  BASECFM.solve (reference flow_matching.py:60-63)
 * hands the whole grid to torchdiffeq, whose fixed-grid loop is `for t0, t1 in zip(grid[:-1], grid[1:]): dt = t1 - t0;
 * y = y + step(f, t0, dt, t1, y)`; this entry is one pass of that loop body with (t0, t1) per utterance: the time embedding is made
 * for stages * B times, every ResNet block adds its utterance's own bias row, and the update takes its utterance's own dt.
 *   State: pools d_z_pool, d_mu_pool [S, n_feats, T_cap] (fp32, channels first, like mtts_cfm_solve's d_x0 / d_mu; with
 *   use_mu_prior the caller stores z = mu + noise).  Utterance b of the step lives in slot d_slots[b] (device int32 [B], distinct,
 *   in [0, S)); frames [0, T_fold) of its z are replaced by the state after the step, everything else in the pools is left as
 *   it is.  h_slots is the host's copy of the same B indices: it is what this call validates (the device copy is not read back;
 *   kernels skip a slot outside [0, S) should the two disagree).
 *   d_t0, d_t1 (device fp32 [B]): the grid interval of utterance b.  dt = t1 - t0 in fp32, stage times t0 (euler); t0,
 *   t0 + 0.5f * dt (midpoint); t0, t0 + dt * (1/3), t0 + dt * (2/3), t1 (rk4, 3/8 rule) -- torchdiffeq's arithmetic, as
 *   mtts_cfm_solve computes it on the host, so n calls over t_span[i], t_span[i + 1] reproduce the one-call solve.
 *   d_y_lengths (device int64 [B]), y_max, T_fold: folded padding of THIS step's batch as for mtts_cfm_solve_folded, with T_cap in
 *   the place of T: mtts_fold_rows(ctx, y_max, 1) <= T_fold <= T_cap, T_fold a multiple of 2^(levels-1).  mtts_set_frame_limits
 *   composes (d_t_len[b] = the reference's padded length of utterance b, in this step's order); without it that length is T_cap.
 *   Workspace: mtts_decoder_workspace_bytes(ctx, B, T_fold).  Range guard, pair time-out word and mtts_prof_* as for any
 *   estimator call.  Returns -1 (mtts_last_error) without touching the pools for: a slot out of range or named twice, B > S,
 *   y_max > T_cap, a T_fold that breaks the rules above, an unknown solver. */
int mtts_cfm_step(mtts_ctx* ctx, float* d_z_pool, const float* d_mu_pool, int S, int T_cap, const int32_t* d_slots,
                  const int32_t* h_slots, const float* d_t0, const float* d_t1, const int64_t* d_y_lengths, int y_max, int solver,
                  int B, int T_fold, void* d_ws, int64_t ws_bytes, void* stream);

/* ---------------------------------------------------------------- single kernels (parity tests, building blocks) */

/* C[M,N] = epilogue(prologue(A)[M,K] * W[N,K]^T): the fp32-MFMA GEMM every Linear/Conv1d of the path runs on.
 * A is [B*T_in, lda] row major (channels last).  ntaps>1 makes it an implicit 1-D convolution:
 * K = ntaps*C, output row (b,t) reads input rows t*in_stride + tap_off[tap].  W is the *unpacked* torch weight:
 * Linear [N,C] or Conv1d [N,C,ntaps]; it is packed into d_wpacked (mtts_gemm_packed_bytes) on the stream first
 * (d_w = NULL: d_wpacked already holds the packed panel from an earlier call).
 * act: 0 none, 1 relu, 2 silu, 3 SnakeBeta with d_p0 = exp(alpha)[N], d_p1 = 1/(exp(beta)+1e-9)[N]
 * (reference transformer.py:61-77).  Epilogue: c = act(acc + bias); c *= out_mask[row]; c = c*out_scale + res[row][n].
 * terms: arithmetic of the products, all with fp32 accumulation: 0 = v_mfma_f32_32x32x2_f32 (native fp32);
 * 2 = operands split into two fp16 terms with a 2^11-scaled residual (22 significand bits), three f16 MFMA products --
 * measured error equals the fp32 chain's, inputs beyond +-65504 saturate; 6 = three exact bf16 terms, six bf16 MFMA
 * products (full fp32 range); 3 = two bf16 terms (looser, opt-in); -1 = the library default (2, or MTTS_GEMM_TERMS).
 * LayerNorm prologue: either d_a_mean/d_a_rstd [rows], or d_a_part [rows][a_nparts][2] = (mean, M2) of 64-column slices
 * as written by a previous call's d_stats_out [M][N/64][2] (N % 64 == 0).  All optional pointers may be NULL. */
int64_t mtts_gemm_packed_bytes(int N, int C, int ntaps);
int mtts_gemm_f32(const float* d_a, int lda, int B, int T_in, int C, int ntaps, const int* h_tap_off, int in_stride,
                  int T_out, const float* d_a_mask, const float* d_a_mean, const float* d_a_rstd, const float* d_a_part,
                  int a_nparts, const float* d_w,
                  void* d_wpacked, const float* d_bias, int N, int act, const float* d_p0, const float* d_p1,
                  const float* d_res, int ldr, const float* d_out_mask, float out_scale, float* d_out, int ldc,
                  float* d_stats_out, int terms, void* stream);

/* P16 GEMM (csrc/gemm_p16.hip): same contract as mtts_gemm_f32 in its fp16-split mode, but the A operand is first
 * written as a "P16" image (fp16 head + scaled fp16 residual, 128-B lines per 32 channels; here by a conversion pass into
 * d_scratch, in the model by the producing kernel's epilogue) and both tiles reach LDS by LDS-DMA.  C % 32 == 0, N % 4 == 0.
 * LayerNorm statistics (arrays or partial moments) are applied in the epilogue: rstd * (x.W - mean * rowsum(W)).
 * d_out (fp32) and/or d_out16_f32 (the P16 output image decoded back to fp32 [M][N], N % 32 == 0, residual scale
 * out_lscale) receive the result.  Replaces F.linear / F.conv1d like mtts_gemm_f32 (reference decoder.py, transformer.py). */
int64_t mtts_gemm_p16_scratch_bytes(int B, int T_in, int C, int T_out, int N);
int mtts_gemm_p16(const float* d_a, int lda, int B, int T_in, int C, int ntaps, const int* h_tap_off, int in_stride, int T_out,
                  const float* d_a_mask, const float* d_a_mean, const float* d_a_rstd, const float* d_a_part, int a_nparts,
                  const float* d_w, void* d_wpacked, const float* d_bias, int N, int act, const float* d_p0, const float* d_p1,
                  const float* d_res, int ldr, const float* d_out_mask, float out_scale, float* d_out, int ldc,
                  float* d_out16_f32, float out_lscale, float* d_stats_out, int force_bm, void* d_scratch, void* stream);

/* One-launch Block1D (csrc/resnet_conv.hip): Conv1d(C -> N, k3, p1) -> GroupNorm(8) -> Mish -> * mask [-> + chbias -> * mask] on
 * channels-last rows x [B*T, C] (converted to a P16 image in d_scratch), result decoded from its P16 image into d_out [B*T, N].
 * N = 384, 65 <= T <= 384, C % 32 == 0; c1 > 0 reads the last c1 channels as a second input segment.  d_nrows / d_nextra /
 * d_bias_stats as the model's frame tables (null: all T rows, no closed-form rows).  d_w is the torch Conv1d weight [N, C, 3],
 * d_wpacked mtts_gemm_packed_bytes(N, C, 3) bytes.  Replaces Block1D of the reference decoder (decoder.py:32-45). */
int64_t mtts_conv_gn_scratch_bytes(int B, int T, int C, int N);
int mtts_conv_gn(const float* d_x, int B, int T, int C, int c1, const float* d_w, void* d_wpacked, const float* d_bias, int N,
                 const float* d_gamma, const float* d_beta, const float* d_mask, const float* d_chbias, const int* d_nrows,
                 const int* d_nextra, const float* d_bias_stats, float eps, float* d_out, void* d_scratch, void* stream);
/* ... with one time-embedding bias row per utterance (mtts_cfm_step): d_chbias [B][chbias_stride], chbias_stride >= N, % 4 == 0;
 * utterance b adds the first N values of its row.  mtts_conv_gn is this kernel with one row for the batch (stride 0). */
int mtts_conv_gn_rows(const float* d_x, int B, int T, int C, int c1, const float* d_w, void* d_wpacked, const float* d_bias, int N,
                      const float* d_gamma, const float* d_beta, const float* d_mask, const float* d_chbias, int chbias_stride,
                      const int* d_nrows, const int* d_nextra, const float* d_bias_stats, float eps, float* d_out, void* d_scratch,
                      void* stream);

/* Self-attention over packed [B*T, 3*H*D] q|k|v rows -> [B*T, H*D].  mask_mode 0: additive float key bias
 * (diffusers semantics, reference transformer.py:253-258); 1: boolean query*key mask (reference
 * text_encoder.py:228-235,306).  d_mask [B,T] float 0/1. */
int mtts_attention_f32(const float* d_qkv, const float* d_mask, int B, int T, int H, int D, float scale, int mask_mode,
                       float* d_out, void* stream);

/* mtts_attention_f32 with P16 I/O (D == 64): q|k|v read as a P16 image (unscaled residuals), output written as a P16
 * image; here both conversions happen around the kernel, in d_scratch (>= 16*B*T*H*64 bytes). */
int mtts_attention_p16(const float* d_qkv, const float* d_mask, int B, int T, int H, int D, float scale, int mask_mode,
                       float* d_out, void* d_scratch, void* stream);

/* Transformer-block chain (csrc/tblock_chain.hip): the row-local part of a BasicTransformerBlock behind the attention as ONE
 * launch -- x1 = x + att . W_out^T + b_out (reference transformer.py:261); x2 = x1 + W2 . SnakeBeta(W1' . LN(x1) + b1') + b2
 * (transformer.py:278-301, FeedForward :104-120, SnakeBeta :61-77); qkv = W_qkv' . LN(x2) + b_qkv' (the following block's
 * norm1 + to_q/k/v, transformer.py:249-258).  LN = LayerNorm without affine (eps 1e-5): the caller folds gamma / beta into the
 * primed panels, as the model's packer does.  Rows are independent; att [M][inner], x [M][C] fp32 on the device; the panels
 * ([N][K] row major), biases and SnakeBeta constants (p0 = exp(alpha), p1 = 1 / (exp(beta) + 1e-9), [4C]) on the HOST -- this
 * test entry packs the fragment stream itself.  C in {128, 256, 384}, inner % 32 == 0 (0: FeedForward only), h_w_qkv NULL: no
 * q|k|v phase.  d_out_mask [M] (0/1) or NULL multiplies the rows of x_out (the masked image convs read).  qb: rows per
 * workgroup (64 / 48 / 32), ch: hidden chunk (128; 256 with C = 384, qb 48 / 32).  Outputs: x_out [M][C], qkv_out [M][n_qkv]. */
/* Host-only: the fragment stream of a chain (no device needed).  Per wave (8): [out-projection: inner/32 k-steps x C/128 tiles]
 * [per hidden chunk of ch: C/32 k-steps x ch/128 tiles of w1, then ch/32 k-steps x C/128 tiles of w2][q|k|v passes: C/32 k-steps x
 * C/128 tiles] + ring padding; a tile = the fp16 head fragment then the 2^11-scaled residual fragment, a fragment = 64 lanes x 8
 * halves with lane (r = lane & 15, q = lane >> 4) holding panel row n0 + r, columns k0 + 8 q .. + 7 (the A operand of
 * v_mfma_f32_16x16x32_f16).  h_dst: mtts_chain_stream_frags(...) * 8 * 512 halves. */
int64_t mtts_chain_stream_frags(int C, int inner, int ch, int n_qkv);
/* Threading / sharing note for the estimator entry points: between 3000 and 5760 estimator rows the transformer blocks of width 384
 * (hidden chunk 256; mtts_tblock_plan) run the PAIR form of the chain launch (below), in which two workgroups wait for each other inside the kernel.  It assumes the launch has the GPU
 * to itself (one stream per device at a time); a process that shares a device between several contexts sets MTTS_CHAIN_PAIR=0.  A
 * workgroup whose partner does not arrive within ~0.5 s gives up and sets the second word of the workspace header. */
/* The model's launch plan of a chain launch over M rows (hidden chunk ch = 128 / 256): rows per workgroup and the number of
 * prefetch workgroups (MTTS_CHAIN_PF as set at this call, default 16).  Host arithmetic only. */
int mtts_chain_plan(int M, int ch, int* qb, int* prefetch_wgs);
/* 1 when the chain kernel is instantiated for (width C, rows per workgroup qb, hidden chunk ch), else 0: the one table the launcher
 * dispatches through.  Host only. */
int mtts_chain_shape_exists(int C, int qb, int ch);
/* How the estimator runs the row-local part of a transformer block of width C (attention width inner; n_qkv: width of the
 * following block's q|k|v, 0 for the last block of a run) at each of the `count` row counts M, M + 1, ..: the decision
 * mtts_decoder_forward / mtts_cfm_solve take per block and level in the default arithmetic, for a context created under these
 * switch values (MTTS_CHAIN, MTTS_CHAIN_CH, MTTS_CHAIN_QB, MTTS_CHAIN_PF, MTTS_CHAIN_MIN_ROWS, MTTS_CHAIN_PAIR,
 * MTTS_CHAIN_PAIR_MIN_ROWS) on a whole device.  The environment is not read.  *ch: the hidden chunk the block's streams are
 * packed for; arrays of `count`: form[i] 0 = four tiled GEMM launches, 1 = the chain launch, 2 = its pair form; for forms 1 and 2
 * qb[i] rows per workgroup (mtts_chain_shape_exists(C, qb[i], *ch) holds), grid_wgs[i] row-tile workgroups (pair: 16 *
 * ceil(ceil(M / qb) / 8)), prefetch_wgs[i] prefetch workgroups; zeros for form 0.  The pair form is taken at C = 384 with hidden
 * chunk 256 only -- the one shape it was measured at -- and only such blocks carry a pair stream in the weight image.  Host
 * arithmetic only. */
int mtts_tblock_plan(int C, int inner, int n_qkv, int M, int count, int chain_on, int chain_ch, int chain_qb, int chain_pf,
                     int chain_min_rows, int pair_on, int pair_min_rows, int* ch, int* form, int* qb, int* grid_wgs, int* prefetch_wgs);
int mtts_chain_stream_pack(int C, int inner, int ch, int n_qkv, const float* h_w_out, const float* h_w1, const float* h_w2,
                           const float* h_w_qkv, uint16_t* h_dst);
/* pair form (below): fragments per (half, wave) and the packing of the 2 x 8 streams, [half][wave][fragment][64 lanes][8 halves];
 * h_dst: 2 * 8 * mtts_chain_stream_frags_pair(...) * 512 halves.  Host only. */
int64_t mtts_chain_stream_frags_pair(int C, int inner, int ch, int n_qkv);
int mtts_chain_stream_pack_pair(int C, int inner, int ch, int n_qkv, const float* h_w_out, const float* h_w1, const float* h_w2,
                                const float* h_w_qkv, uint16_t* h_dst);
int64_t mtts_tblock_chain_scratch_bytes(int M, int C, int inner, int n_qkv, int ch);
int mtts_tblock_chain(const float* d_att, const float* d_x, int M, int C, int inner, const float* h_w_out, const float* h_b_out,
                      const float* h_w1, const float* h_b1, const float* h_p0, const float* h_p1, const float* h_w2,
                      const float* h_b2, const float* h_w_qkv, const float* h_b_qkv, int n_qkv, const float* d_out_mask, int qb,
                      int ch, float* d_x_out, float* d_qkv_out, void* d_scratch, void* stream);
/* the same, followed by `repeat` further launches of the kernel alone between two events: *h_ms = their mean duration */
int mtts_tblock_chain_timed(const float* d_att, const float* d_x, int M, int C, int inner, const float* h_w_out, const float* h_b_out,
                            const float* h_w1, const float* h_b1, const float* h_p0, const float* h_p1, const float* h_w2,
                            const float* h_b2, const float* h_w_qkv, const float* h_b_qkv, int n_qkv, const float* d_out_mask,
                            int qb, int ch, float* d_x_out, float* d_qkv_out, void* d_scratch, void* stream, int repeat, float* h_ms);
/* the PAIR form of the same launch: two workgroups of one XCD share a row tile, each streams half of the FeedForward's hidden chunks
 * and of the q|k|v passes and they exchange their FF2 partial sums through the L2 (csrc/tblock_chain.hip).  Needs an out-projection
 * (inner > 0), an even number of hidden chunks and a grid that is resident at once: 16 * ceil(ceil(M / qb) / 8) + 16 <= 256. */
int mtts_tblock_chain_pair_timed(const float* d_att, const float* d_x, int M, int C, int inner, const float* h_w_out, const float* h_b_out,
                                 const float* h_w1, const float* h_b1, const float* h_p0, const float* h_p1, const float* h_w2,
                                 const float* h_b2, const float* h_w_qkv, const float* h_b_qkv, int n_qkv, const float* d_out_mask,
                                 int qb, int ch, float* d_x_out, float* d_qkv_out, void* d_scratch, void* stream, int repeat, float* h_ms);

/* The same chain for the 16-bit storage modes (csrc/tblock_chain_h16.hip; mtts_set_arithmetic 16 / 17): H16 images (one plane,
 * rows of C 2-byte values) in and out, ONE v_mfma_f32_16x16x32_f16 / _bf16 per MAC, fp32 accumulation, LayerNorm moments and
 * SnakeBeta in fp32; every value that crosses a phase is rounded once to the 16-bit type.  bf16 != 0: bfloat16 planes (round to
 * nearest even, no range guard); 0: fp16 planes (saturating at +-65504).  Single-workgroup form only.
 * Shapes: C in {128, 256, 384}; inner a multiple of 128, <= C (0: FeedForward only); ch 128, or 256 with C = 384; n_qkv % 32 == 0.
 * Host-only: the one-plane fragment stream, same order and 1 KiB lane-major fragments as mtts_chain_stream_pack with ONE fragment per
 * tile and a ring padding of 4 * C/128 fragments.  h_dst: mtts_chain_stream_frags_h16(...) * 8 * 512 values; *saturates (may be NULL)
 * is set to 1 when an fp16 weight lies beyond +-65504, else left alone. */
int64_t mtts_chain_stream_frags_h16(int C, int inner, int ch, int n_qkv);
int mtts_chain_stream_pack_h16(int C, int inner, int ch, int n_qkv, const float* h_w_out, const float* h_w1, const float* h_w2,
                               const float* h_w_qkv, int bf16, uint16_t* h_dst, int* saturates);
/* Unit entry: fp32 rows in, fp32 rows out (the 16-bit values the kernel wrote, widened); operands as mtts_tblock_chain.  The row sums
 * that LayerNorm needs are taken from the ROUNDED panels.  qb: rows per workgroup (32 / 64; 96 with C = 384, ch = 256);
 * pf_wgs: prefetch workgroups (0..64).  _timed: `repeat` further launches between two events, *h_ms = their mean duration. */
int64_t mtts_tblock_chain_h16_scratch_bytes(int M, int C, int inner, int n_qkv, int ch);
int mtts_tblock_chain_h16(const float* d_att, const float* d_x, int M, int C, int inner, const float* h_w_out, const float* h_b_out,
                          const float* h_w1, const float* h_b1, const float* h_p0, const float* h_p1, const float* h_w2,
                          const float* h_b2, const float* h_w_qkv, const float* h_b_qkv, int n_qkv, const float* d_out_mask, int bf16,
                          int qb, int ch, int pf_wgs, float* d_x_out, float* d_qkv_out, void* d_scratch, void* stream);
int mtts_tblock_chain_h16_timed(const float* d_att, const float* d_x, int M, int C, int inner, const float* h_w_out, const float* h_b_out,
                                const float* h_w1, const float* h_b1, const float* h_p0, const float* h_p1, const float* h_w2,
                                const float* h_b2, const float* h_w_qkv, const float* h_b_qkv, int n_qkv, const float* d_out_mask,
                                int bf16, int qb, int ch, int pf_wgs, float* d_x_out, float* d_qkv_out, void* d_scratch, void* stream,
                                int repeat, float* h_ms);

/* ---- The estimator's other kernels in the 16-bit storage modes (mtts_set_arithmetic 16 / 17), one unit entry per kernel: the
 * one-plane ("H16") instantiations of csrc/gemm_p16.hip (MODE 2 fp16 / 3 bfloat16), csrc/attention_f32.hip (HALF, BF),
 * gn_apply_kernel's H16 store and the fp32 <-> H16 conversions.  An H16 image is ONE plane of 16-bit values, rows of C values
 * (C % 64 == 0: a 128-byte line holds 64 channels).  fp32 rows in are rounded to images by the library's conversion kernel (round
 * to nearest even; fp16 clamps to +-65504 first and raises the range flag, bfloat16 keeps the fp32 range and never raises it);
 * images out come back widened to fp32, i.e. exactly the 16-bit values the kernel stored.  bf16 != 0: bfloat16 planes, else fp16.
 * d_range_flag (may be NULL): one device word, OR-ed with 1 when a value an fp16 producer stores lies beyond +-65504 (the stored
 * value is the clamp); the caller clears it.  Host code only: every kernel launched is an instantiation the model launches. */

/* Name of the kernel instantiation the last launcher call on this thread chose, as rocprofv3 prints it ("" when untagged):
 * "gemm_p16_kernel<BM, LN, stages, MODE, M16, GN, KS>", "attention_f32_kernel<NW, P16, ONE, HALF, BF, KR>".  Host only. */
const char* mtts_last_kernel_tag(void);

/* Host only: an fp32 panel of n values as the 16-bit weight plane of these modes (fp16: clamp to +-65504, then round to nearest
 * even; bfloat16: round to nearest even), same element order.  What the packer stores beside every panel. */
int mtts_panel_h16_host(const float* h_panel, int64_t n, int bf16, uint16_t* h_plane);

/* fp32 rows [M][ld] -> H16 image d_image [M][ld16 values] (times d_mask[row] when given, BEFORE rounding; columns [C_valid, C) are
 * written as zeros) -> fp32 rows d_out [M][C].  d_image is the caller's, so the stored bits can be compared. */
int mtts_to_h16_roundtrip(const float* d_x, int ld, const float* d_mask, int M, int C, int C_valid, int ld16, int bf16, void* d_image,
                          float* d_out, unsigned int* d_range_flag, void* stream);

/* H16 GEMM: the counterpart of mtts_gemm_p16 with every epilogue feature the decoder uses in these modes.  The argument block
 * mirrors the kernel interface (csrc/kernels.h GemmArgs); pointers named d_ are device memory, h_ host memory, all optional ones
 * may be NULL.  Refused before any launch (-1, mtts_last_error): C or c1 not a multiple of 64, bf16 without half16, half16 unset,
 * res16 together with res, gn_stats with anything but a bias-only epilogue, null buffers. */
typedef struct mtts_gemm_h16_args {
    /* A operand: fp32 rows [B*T_in][lda], rounded to an H16 image (times d_a_mask[row] first).  c1 > 0: the last c1 channels form a
     * second channel segment (the up path's skip concat: GemmArgs::a16_1 / c1) */
    const float* d_a; int32_t lda; int32_t C; int32_t c1; const float* d_a_mask;
    int32_t B, T_in, T_out, ntaps; const int32_t* h_tap_off; int32_t in_stride;      /* as mtts_gemm_f32 */
    /* LayerNorm in the epilogue (ntaps == 1): mean / rstd arrays, or partial moments [rows][a_nparts][2] (a d_stats_out) */
    const float* d_a_mean; const float* d_a_rstd; const float* d_a_part; int32_t a_nparts;
    /* B operand: the UNPACKED torch weight on the host, Linear [N][C] or Conv1d [N][C][ntaps]; packed, rounded to the 16-bit plane
     * (mtts_panel_h16_host) and summed per row (LayerNorm algebra, sums of the ROUNDED weights) here */
    const float* h_w; const float* d_bias; int32_t N;
    int32_t act; const float* d_p0; const float* d_p1;                                /* as mtts_gemm_f32 */
    const float* d_res; int32_t ldr;                                                 /* fp32 residual rows */
    /* residual as an H16 image: 1 = a separate image made from d_res16_f32 [out rows][N]; 2 = IN PLACE, the output image itself
     * (GemmArgs::res16 == out16, the residual-stream update; needs out16_preload) */
    int32_t res16_mode; const float* d_res16_f32;
    const float* d_out_mask; float out_scale;
    const float* d_out16_mask;                                                      /* multiplies the H16 copy only */
    float* d_out;                                                                   /* fp32 result [out rows][N] or NULL */
    /* the H16 result widened to fp32 [out rows][N] or NULL.  out16_preload != 0: the image is first filled from this buffer
     * (lossless for values of the 16-bit type), so rows a launch does not write keep their value across calls */
    float* d_out16_f32; int32_t out16_preload;
    /* output row = b * out_T + t * out_stride + out_off (out_T == 0: plain rows); out rows = B * out_T */
    int32_t out_T, out_stride, out_off;
    float* d_stats_out;                                                             /* [out rows][N/64][2] LayerNorm moments */
    /* GroupNorm statistics from the epilogue (GemmArgs::gn_stats): entries of 4 floats per wave tile, part and group slice;
     * 2 * ceil(M / wave_rows + 1) * (N/64) * 2 entries at most.  d_gn_nrows [B] or NULL */
    float* d_gn_stats; int32_t gn_groups; const int32_t* d_gn_nrows;
    /* Block1D tail in the epilogue (GemmArgs::gnr_*): out += Mish(GroupNorm(d_gnr_y)) * d_gnr_mask from a producer's d_gn_stats */
    const float* d_gnr_y; const float* d_gnr_stats; int32_t gnr_tile_rows, gnr_groups;
    const float* d_gnr_gamma; const float* d_gnr_beta; const float* d_gnr_mask; float gnr_eps;
    const int32_t* d_gnr_nextra; const float* d_gnr_bias_stats;
    int32_t force_bm;                                                               /* 0, 64 or 128 */
    int32_t half16, bf16;                                                           /* half16 must be 1 */
    uint32_t* d_range_flag;
    /* written by the call: the instantiation launched and the rows of its wave tile (what a gn_stats consumer is told) */
    int32_t wave_rows; char tag[124];
} mtts_gemm_h16_args;
int64_t mtts_gemm_h16_scratch_bytes(const mtts_gemm_h16_args* g);
int mtts_gemm_h16(mtts_gemm_h16_args* g, void* d_scratch, void* stream);
/* Host only: rows of the wave tile the launcher will choose for these shapes (32 or 64). */
int mtts_gemm_h16_wave_rows(int B, int T_out, int N, int force_bm);

/* H16 attention: as mtts_attention_p16 on H16 images of q|k|v and of the output.  d_klen [B] (may be NULL): keys of utterance b
 * are rows [0, klen[b]); with folded padding d_mask then holds the additive key bias itself (ln(n_pad) on the one row that stands
 * for n_pad padded frames).  d_scratch >= 8 * B*T*H*64 bytes.  The kernel rounds probabilities and the output to 16 bits. */
int mtts_attention_h16(const float* d_qkv, const float* d_mask, const int* d_klen, int B, int T, int H, int D, float scale, int mask_mode,
                       int bf16, float* d_out, unsigned int* d_range_flag, void* d_scratch, void* stream);

/* GroupNorm + Mish + mask [+ chbias, mask] written as an H16 image (d_out16_f32, times d_out16_mask[row]) and optionally as fp32
 * rows (d_out).  Statistics: d_tile_stats / tile_rows (a mtts_gemm_h16 d_gn_stats and its wave_rows), or a statistics pass over
 * d_y (d_nrows [B]: rows that enter it).  d_nextra / d_bias_stats: folded padding, as GnApplyArgs. */
int64_t mtts_groupnorm_h16_scratch_bytes(int B, int T, int C, int G);
int mtts_groupnorm_mish_h16(const float* d_y, const float* d_gamma, const float* d_beta, const float* d_mask, const float* d_chbias,
                            int chbias_stride, int B, int T, int C, int G, float eps, const float* d_tile_stats, int tile_rows,
                            const int* d_nrows, const int* d_nextra, const float* d_bias_stats, const float* d_out16_mask, int bf16,
                            float* d_out, float* d_out16_f32, unsigned int* d_range_flag, void* d_scratch, void* stream);

/* ---- The same kernels in the DEFAULT arithmetic, one unit entry per kernel: the two-plane ("P16") instantiations -- gemm_p16_kernel
 * MODE 0 (fp16 head + scaled fp16 residual, three products per MAC; fast16 != 0: MODE 1, heads only), the <NW, true, false, false,
 * false, KR> attention kernels, gn_apply_kernel's two-plane store and the fp32 <-> P16 conversions -- with every argument the decoder
 * passes.  A P16 image holds, per row and 32-channel group, 32 heads h = fp16(clamp(x, +-65504)) then 32 residuals
 * l = fp16((clamp(x) - h) * lscale): rows of 2 * C halves (C % 32 == 0), value h + l / lscale.  lscale is 2048 everywhere except the
 * q|k|v image the attention kernel reads (1).  Images out come back as fp32 h + l / lscale, i.e. exactly the stored pair.
 * d_range_flag as above.  Host code only: every kernel launched is an instantiation the model launches. */

/* fp32 rows [M][ld] -> P16 image d_image [M][ld16 halves, >= 2 * C] (times d_mask[row] when given, BEFORE the split; columns
 * [C_valid, C) are written as zeros) -> fp32 rows d_out [M][C].  d_image is the caller's, so the stored bits can be compared. */
int mtts_to_p16_roundtrip(const float* d_x, int ld, const float* d_mask, int M, int C, int C_valid, int ld16, float lscale, void* d_image,
                          float* d_out, unsigned int* d_range_flag, void* stream);

/* P16 GEMM on the argument block of mtts_gemm_h16 (half16 and bf16 must be 0; "H16 image" reads "P16 image" throughout, C, c1 and an
 * image's N are multiples of 32).  A, the residual image and a preloaded output image are split with lscale 2048 (the preload with
 * out_lscale); the panel is packed, split on the device as mtts_gemm_p16 does, and summed per row as the model's packer does for this
 * arithmetic (sums of the fp32 panel).  fast16: 1 = MODE 1 (refused with d_gn_stats).  out_lscale: residual scale of the output
 * image, 2048 or 1 (what the attention kernel reads; not with res16_mode 2).  wave_rows and tag are written as by mtts_gemm_h16. */
int64_t mtts_gemm_p16_args_scratch_bytes(const mtts_gemm_h16_args* g);
int mtts_gemm_p16_args_run(mtts_gemm_h16_args* g, int fast16, float out_lscale, void* d_scratch, void* stream);

/* P16 attention with everything the decoder passes: q|k|v image with unscaled residuals, d_klen and the key bias of folded padding
 * as mtts_attention_h16, the output image with residual scale out_lscale (2048 or 1), fast16 (single fp16 product per MAC).
 * d_scratch >= 16 * B*T*H*64 bytes.  The instantiation is read through mtts_last_kernel_tag. */
int mtts_attention_p16_run(const float* d_qkv, const float* d_mask, const int* d_klen, int B, int T, int H, int D, float scale, int mask_mode,
                           int fast16, float out_lscale, float* d_out, unsigned int* d_range_flag, void* d_scratch, void* stream);

/* GroupNorm + Mish + mask [+ chbias, mask] written as a P16 image (d_out16_f32, times d_out16_mask[row]) and optionally as fp32
 * rows (d_out); arguments as mtts_groupnorm_mish_h16 (tile statistics of a mtts_gemm_p16_args_run, or the statistics pass). */
int64_t mtts_groupnorm_p16_scratch_bytes(int B, int T, int C, int G);
int mtts_groupnorm_mish_p16(const float* d_y, const float* d_gamma, const float* d_beta, const float* d_mask, const float* d_chbias,
                            int chbias_stride, int B, int T, int C, int G, float eps, const float* d_tile_stats, int tile_rows,
                            const int* d_nrows, const int* d_nextra, const float* d_bias_stats, const float* d_out16_mask, float* d_out,
                            float* d_out16_f32, unsigned int* d_range_flag, void* d_scratch, void* stream);

/* ---- The fp32-ROW flow (fp32 rows in, fp32 rows out: the text encoder, the duration predictor, the estimator when the range guard
 * reruns on full-range arithmetic, MTTS_P16=0), one unit entry per kernel with every argument the model passes.  Host code only.
 *
 * gemm_f32_kernel<BM, A_MASK, A_NORM, TERMS> on the argument block of mtts_gemm_h16 (half16 = bf16 = 0).  A stays fp32 rows
 * [B*T_in][lda]; the panel is packed on the host with ktap = round_up(C, 32) and its planes are made as the model's packer makes them
 * for `terms`: 0 fp32 panel alone, 2 the interleaved fp16 head / scaled-residual image, 6 three bfloat16 planes.  c1 > 0: a second
 * channel segment of c1 channels, read from d_a1 [B*T_in][lda1] when given, else from the last c1 columns of d_a ((C - c1) % 32 == 0).
 * ldc: row stride of d_out (0 = N); only columns [0, N) of an output row are written.  Honoured from the block: d_a_mask, LayerNorm
 * statistics (arrays or partial moments), act / p0 / p1, d_res + ldr, d_out_mask, out_scale, out_T / out_stride / out_off,
 * d_stats_out, force_bm, d_range_flag (raised by terms 2 when an A element, or by any terms when an image element, lies beyond
 * +-65504), and d_out16_f32 + d_out16_mask: the P16 copy of the result with residual scale out_lscale (2048 or 1), decoded to fp32
 * [out rows][N].  The RAW image, [out rows + MTTS_ENTRY_GUARD_ROWS][2 N] halves (per 32 columns 32 heads then 32 residuals), starts at
 * the first 256-byte boundary of d_scratch and is filled with 0x7e00 before the launch.  `tag` is written, wave_rows is 0.
 * Refused before any launch (-1, mtts_last_error): everything the launcher refuses (null buffers, C or c1 % 4, lda / lda1 / ldc / ldr,
 * one of a_mean / a_rstd, a_part with a_mean, LayerNorm on a convolution, stats_out without N % 64 == 0, an image without N % 32 == 0
 * or with ldc / ldr % 4 != 0, SnakeBeta without constants, terms other than 0 / 2 / 6), res16_mode / out16_preload / gn_stats / gnr
 * (features of the P16 kernel), and output rows leaving [0, out_T). */
int64_t mtts_gemm_f32_args_scratch_bytes(const mtts_gemm_h16_args* g);
int mtts_gemm_f32_args_run(mtts_gemm_h16_args* g, int terms, const float* d_a1, int lda1, int ldc, float out_lscale, void* d_scratch,
                           void* stream);

/* mtts_attention_f32 with d_klen [B] (may be NULL): keys of utterance b are rows [0, klen[b]).  The instantiation is read through
 * mtts_last_kernel_tag: "attention_f32_kernel<2|4, false, false, false, false, 64>". */
int mtts_attention_f32_run(const float* d_qkv, const float* d_mask, const int* d_klen, int B, int T, int H, int D, float scale, int mask_mode,
                           float* d_out, void* stream);

/* gn_partial + gn_apply with the fp32 store and every argument the fp32-row estimator passes: d_chbias [B][chbias_stride] (stride 0:
 * one row [C]), d_res [B*T][ldr] added last, d_nrows [B] (rows that enter the statistics), d_nextra [B] + d_bias_stats [G][2] (folded
 * padding), d_stats_out [B*T][C/64][2] (LayerNorm moments of the output rows).  NULL skips a feature.  d_scratch:
 * mtts_groupnorm_scratch_bytes. */
int mtts_groupnorm_mish_f32_run(const float* d_y, const float* d_gamma, const float* d_beta, const float* d_mask, const float* d_chbias,
                                int chbias_stride, const float* d_res, int ldr, int B, int T, int C, int G, float eps, const int* d_nrows,
                                const int* d_nextra, const float* d_bias_stats, float* d_out, float* d_stats_out, void* d_scratch,
                                void* stream);

/* mtts_channel_layernorm on rows of wider buffers: x [B*T][ldx], y [B*T][ldy]; only columns [0, C) of a row are read and written. */
int mtts_channel_layernorm_ld(const float* d_x, int ldx, int B, int T, int C, const float* d_gamma, const float* d_beta, float eps, int act,
                              const float* d_film, const float* d_mask, float* d_y, int ldy, void* stream);

/* The two fused kernels (tblock_chain_kernel, conv_gn_kernel) on argument blocks, with what the plain entries above cannot pass: the
 * range flag, image rows longer than their payload, and the RAW output images.  Every output image has pad_* extra halves per row
 * (% 8 == 0) and MTTS_ENTRY_GUARD_ROWS rows behind its last row; the entry fills the whole image with `sentinel` (a 16-bit pattern)
 * before the launch, so whatever the kernel did not write still holds it.  Input images with a pad get the sentinel in their pad
 * columns too (0x7e00, an fp16 NaN, poisons any product that reads them).  d_*_image (may be NULL): [rows + guard][2 * width + pad]
 * halves, copied from the entry's scratch after the launch.  `tag` is written by the call (as mtts_last_kernel_tag).
 * Chain: operands as mtts_tblock_chain (h_* on the HOST); pair != 0: the pair form.  conv_gn: operands as mtts_conv_gn_rows
 * (chbias_stride 0: one row for the batch).  Host code only: the kernels launched are the ones the model launches. */
#define MTTS_ENTRY_GUARD_ROWS 64
typedef struct mtts_chain_args {
    const float* d_att; const float* d_x; int32_t M, C, inner;
    const float* h_w_out; const float* h_b_out; const float* h_w1; const float* h_b1; const float* h_p0; const float* h_p1;
    const float* h_w2; const float* h_b2; const float* h_w_qkv; const float* h_b_qkv; int32_t n_qkv;
    const float* d_out_mask; int32_t qb, ch, pair;
    int32_t pad_att, pad_x, pad_out, pad_qkv;                                        /* extra halves per image row */
    uint32_t sentinel;
    uint32_t* d_range_flag;                                                          /* passed to the kernel (may be NULL) */
    float* d_x_out; float* d_qkv_out;                                                /* decoded images [M][C], [M][n_qkv] */
    uint16_t* d_x_out_image; uint16_t* d_qkv_image;                                  /* raw images incl. pad and guard rows, or NULL */
    char tag[124];
} mtts_chain_args;
int64_t mtts_tblock_chain_args_scratch_bytes(const mtts_chain_args* g);
int mtts_tblock_chain_args_run(mtts_chain_args* g, void* d_scratch, void* stream);
typedef struct mtts_conv_gn_args {
    const float* d_x; int32_t B, T, C, c1; const float* d_w; void* d_wpacked; const float* d_bias; int32_t N;
    const float* d_gamma; const float* d_beta; const float* d_mask; const float* d_chbias; int32_t chbias_stride;
    const int32_t* d_nrows; const int32_t* d_nextra; const float* d_bias_stats; float eps;
    int32_t pad_x, pad_out;
    uint32_t sentinel;
    uint32_t* d_range_flag;
    float* d_out;                                                                    /* decoded image [B*T][N] */
    uint16_t* d_out_image;                                                           /* raw image [B*T + guard][2 N + pad_out] or NULL */
    char tag[124];
} mtts_conv_gn_args;
int64_t mtts_conv_gn_args_scratch_bytes(const mtts_conv_gn_args* g);
int mtts_conv_gn_args_run(mtts_conv_gn_args* g, void* d_scratch, void* stream);

/* Row statistics for LayerNorm over C (biased variance, eps inside rsqrt): mean[M], rstd[M]. */
int mtts_row_stats(const float* d_x, int M, int C, int ld, float eps, float* d_mean, float* d_rstd, void* stream);

/* Channel LayerNorm of the text encoder -- reference text_encoder.py:19-27 -- over x [B*T, C] rows, optionally followed by
 * SiLU (act = 2: ConvSiluNorm, text_encoder.py:58-60), the DurationPredictor's speaker FiLM `* gamma_b + beta_b`
 * (d_film [B, 2C] = gamma | beta, text_encoder.py:102-109) and the row mask (d_mask [B*T]).  Null pointers skip a stage. */
int mtts_channel_layernorm(const float* d_x, int B, int T, int C, const float* d_gamma, const float* d_beta, float eps, int act,
                           const float* d_film, const float* d_mask, float* d_y, void* stream);

/* Block1D tail -- reference decoder.py:38-45: Mish(GroupNorm_G(y)) * mask over y [B,T,C] (channels last);
 * statistics over (C/G channels x all T frames).  d_scratch: mtts_groupnorm_scratch_bytes. */
int64_t mtts_groupnorm_scratch_bytes(int B, int T, int G);
int mtts_groupnorm_mish(const float* d_y, const float* d_gamma, const float* d_beta, const float* d_mask, int B, int T,
                        int C, int G, float eps, float* d_out, void* d_scratch, void* stream);
/* ... followed by the ResNet block's time-embedding bias -- reference decoder.py:60: (h + mlp(t)) * mask -- with one bias row per
 * utterance: d_chbias [B][chbias_stride] (chbias_stride >= C, % 4 == 0), or one row [C] for the batch with chbias_stride = 0. */
int mtts_groupnorm_mish_rows(const float* d_y, const float* d_gamma, const float* d_beta, const float* d_mask, const float* d_chbias,
                             int chbias_stride, int B, int T, int C, int G, float eps, float* d_out, void* d_scratch, void* stream);

/* Kernel-level entries of the kernels that are not GEMMs: the Vocos tail (csrc/vocos.hip) and the solver / layout glue
 * (csrc/norm_glue.hip).  No context, fp32 device buffers in the layout the model hands to the kernel, stream-ordered, no
 * allocation.  Each entry decides on the host what the host can decide -- null pointers, the launcher's own shape limits, a leading
 * dimension smaller than col_off + C -- and returns -1 (mtts_last_error) before anything is launched; otherwise it calls the
 * launcher the model calls, unchanged.
 * mtts_dwconv7_ln: ConvNeXtBlock front, y = LayerNorm_C(depthwise_conv_k7(x) + bias) * gamma + beta on rows [B*T, C]; d_w7 is [7][C]
 *   (the packed layout, tap-major); C % 4 == 0, C <= 2048.  d_lengths (int64 [B] or NULL): utterance b ends at clamp(lengths[b], 0, T)
 *   frames, taps beyond it are the conv's zero padding whatever the buffer holds; rows at or beyond it are not defined.
 * mtts_spec_polar: in place on rows [M, ld]: columns (k, off + k), k < nbins, hold (log-magnitude, phase) and become
 *   min(exp(m), clip) * (cos p, sin p); off >= nbins, off + nbins <= ld; no other column is touched.
 * mtts_istft_ola: torch.istft(center=True) tail on windowed frames [B*T, n_fft]: audio [B, hop*(T-1)], sample s = sum of the frames
 *   covering pos = s + n_fft/2 over the sum of window^2 there (kept undivided where that sum is <= 1e-11); T >= 2, hop divides n_fft.
 *   d_lengths (or NULL): row b is the result of its first clamp(lengths[b], 0, T) frames alone, then exact zeros.
 * mtts_ode_combine: the fixed-grid solver's state updates on rows [M, C] with leading dimensions ldy / ldk / ldo >= C: stage 0
 *   y + dt k1; stages 1..4 torchdiffeq's rk4 (3/8 rule) in its operation order (norm_glue.hip).  d_dt_b NULL: one dt; else dt =
 *   d_dt_b[row / T] (M % T == 0).  Stage k reads k1..k_k; d_out may be d_y (with ldo == ldy).
 * mtts_step_tables: per-utterance stage times of one solver step (stages 1, 2 or 4): d_tv [stages*B], d_dt_b [B], row factors
 *   d_rs_full / d_rs_half [B*T] = mask * dt, mask * (0.5 dt).
 * mtts_time_sinusoid: out[i] = sin((scale t_i) f_j) | cos(...), j < half, [nt, 2*half]; the times come from h_t (host, nt <= 256) or
 *   from d_t (device, any nt): exactly one of the two is non-null.
 * mtts_rope: half-rotation RoPE in place on the q and k sections of rows [B*T, 3*H*D], first d_rope (even, <= D) dims of each head,
 *   position = row % T; d_cos / d_sin [>= T, d_rope].
 * mtts_cf_to_cl: dst[b*T + t, col_off + c] = src[b, c, t] (+ add[b, c, t]) for t < T, source rows T_src >= T long (0: T);
 *   d_lengths (or NULL): rows at t >= lengths[b] are written as zero and their source is not read.  col_off + C <= ld.
 * mtts_cl_to_cf: dst[b, c, t] = src[b*T + t, c] * scale + shift for t < T_out <= T; C <= ld.
 * mtts_slots_to_cl / mtts_cl_to_slots: the same two moves between a slot pool [S, C, T_pool] and the rows of utterances living in
 *   slots d_slots[b] (int32 [B]); a slot outside [0, S) is neither read (its rows are written as zero) nor written.  T <= T_pool. */
int mtts_dwconv7_ln(const float* d_x, const float* d_w7, const float* d_bias, const float* d_gamma, const float* d_beta, float eps,
                    int B, int T, int C, const int64_t* d_lengths, float* d_y, void* stream);
int mtts_spec_polar(float* d_x, int M, int ld, int nbins, int off, float clip, void* stream);
int mtts_istft_ola(const float* d_frames, const float* d_window, int B, int T, int n_fft, int hop, const int64_t* d_lengths,
                   float* d_audio, void* stream);
int mtts_ode_combine(int stage, float dt, const float* d_dt_b, int T, const float* d_y, int ldy, const float* d_k1, const float* d_k2,
                     const float* d_k3, const float* d_k4, int ldk, float* d_out, int ldo, int M, int C, void* stream);
int mtts_step_tables(const float* d_t0, const float* d_t1, const float* d_mask, int B, int T, int stages, float* d_tv, float* d_dt_b,
                     float* d_rs_full, float* d_rs_half, void* stream);
int mtts_time_sinusoid(const float* d_freqs, const float* h_t, const float* d_t, int nt, int half, float scale, float* d_out,
                       void* stream);
int mtts_rope(float* d_qkv, int B, int T, int H, int D, int d_rope, const float* d_cos, const float* d_sin, void* stream);
int mtts_cf_to_cl(const float* d_src, const float* d_add, int B, int C, int T, int T_src, float* d_dst, int ld, int col_off,
                  const int64_t* d_lengths, void* stream);
int mtts_cl_to_cf(const float* d_src, int ld, int B, int C, int T, float* d_dst, int T_out, float scale, float shift, void* stream);
int mtts_slots_to_cl(const float* d_pool, const int32_t* d_slots, int S, int T_pool, int B, int C, int T, float* d_dst, int ld,
                     int col_off, void* stream);
int mtts_cl_to_slots(const float* d_src, int ld, int B, int C, int T, float* d_pool, const int32_t* d_slots, int S, int T_pool,
                     void* stream);

/* ---------------------------------------------------------------- Vocos-24k head */

/* Vocos.decode -- reference matcha/vocos24k/vocos_wrapper.py:8-9 (third-party vocos package; architecture sizes from
 * reference matcha/vocos24k/config.yaml:10-24).  mel [B, n_mels, T] -> audio [B, hop*(T-1)] (torch.istft, center=True).
 * Tensors are registered under the vocos state-dict keys ("backbone.embed.weight", "backbone.convnext.0.dwconv.weight",
 * "head.out.weight", ...) plus "aux.window" = the periodic hann window [n_fft]. */
typedef struct mtts_vocos mtts_vocos;
mtts_vocos* mtts_vocos_create(int n_mels, int dim, int intermediate_dim, int num_layers, int n_fft, int hop_length);
void mtts_vocos_destroy(mtts_vocos* v);
int mtts_vocos_set_tensor(mtts_vocos* v, const char* key, const float* h_data, int64_t numel);
int64_t mtts_vocos_weights_bytes(mtts_vocos* v);
int mtts_vocos_upload_weights(mtts_vocos* v, void* d_weights, int64_t bytes);
int64_t mtts_vocos_workspace_bytes(mtts_vocos* v, int B, int T);
int mtts_vocos_decode(mtts_vocos* v, const float* d_mel, int B, int T, float* d_audio, void* d_ws, int64_t ws_bytes,
                      void* stream);

/* Vocos.decode of a RAGGED batch -- what the reference computes when it calls vocos_wrapper.py:8-9 once per utterance on
 * mel[b, :, :len_b] (its server does, reference server.py:116): d_lengths = device int64 [B], frames per utterance, 1 <= len_b <= T.
 * Row b of d_audio [B, hop*(T-1)] holds the hop*(len_b - 1) samples of that utterance (every k7 convolution of the head zero-pads
 * at len_b, the iSTFT and its window envelope end at frame len_b - 1) followed by zeros; len_b == 1 gives no samples.  The padded
 * part of d_mel is never read as data.  A row of T frames equals mtts_vocos_decode's row bit for bit.
 * The lengths are checked on the device, without a host synchronisation in front of the decode: the call enqueues and returns.
 * mtts_vocos_ragged_status(d_ws, stream) waits for the stream and reports the first length outside [1, T] through
 * mtts_last_error (the row and the value); mtts_waveform_finish marks the same rows with out_length -1, so a caller that goes
 * on to it needs no wait of its own.  A row with a bad length is decoded as if the length were clamped into [0, T]: nothing
 * is read or written outside the buffers.  Workspace: mtts_vocos_ragged_workspace_bytes. */
int64_t mtts_vocos_ragged_workspace_bytes(mtts_vocos* v, int B, int T);
int mtts_vocos_decode_ragged(mtts_vocos* v, const float* d_mel, const int64_t* d_lengths, int B, int T, float* d_audio,
                             void* d_ws, int64_t ws_bytes, void* stream);
int mtts_vocos_ragged_status(const void* d_ws, void* stream);

/* ---------------------------------------------------------------- waveform finish (ragged batch) */

/* to_waveform's peak normalisation -- reference matcha/inference.py:260-264 -- and trim_trailing_silence's length --
 * reference matcha/inference.py:268-287 -- for every row of d_audio [B][ld] (fp32, rows 16-byte aligned: ld % 4 == 0) on the
 * device, no host synchronisation.  Row b has `valid` samples: d_lengths[b] when hop == 0, hop * (d_lengths[b] - 1) when
 * hop > 0 (d_lengths = the frame counts given to mtts_vocos_decode_ragged).
 *   peak  = max |a| over the valid samples (NaN propagates, as torch's max).  If peak > 1 every valid sample becomes
 *           a / peak * 0.95 in fp32, in that order, in place, and d_scale[b] = 0.95 / peak; else the row is untouched and
 *           d_scale[b] = 1.
 *   trim  : windows of int(0.01 * sample_rate) samples anchored at sample 0 of the row as normalised (the remainder is never
 *           examined); rms = sqrt(mean(a^2)); the trailing run of windows with rms < 10^(threshold_db / 20) (strict, compared in
 *           fp32; a NaN window ends the run) is dropped: d_out_lengths[b] = valid - run * window.  All full windows may go.
 *           The samples are not moved: the caller keeps the first d_out_lengths[b] of the row.
 * A row whose length is outside its row (samples outside [0, ld], frames outside [1, ld / hop + 1]) is left alone and gets
 * d_out_lengths[b] = -1.  Two calls on the same input give the same bits.  Workspace: mtts_waveform_workspace_bytes. */
int64_t mtts_waveform_workspace_bytes(int64_t ld, int B, int sample_rate);
int mtts_waveform_finish(float* d_audio, int64_t ld, const int64_t* d_lengths, int hop, int B, int sample_rate,
                         double threshold_db, float* d_scale, int64_t* d_out_lengths, void* d_ws, int64_t ws_bytes, void* stream);

/* ---------------------------------------------------------------- voice enrolment: log-mel front end and style encoder */

/* Waveform -> normalised log-mel of a ragged batch of clips -- reference matcha/vocos24k/mel_extractor.py:6-41 (torchaudio
 * MelSpectrogram(sample_rate, n_fft, win_length = n_fft, hop_length = hop, n_mels, center=True with reflect padding, power=1,
 * mel_scale="htk", norm=None, f_min 0, f_max sample_rate / 2) of the clip trimmed to a multiple of hop, then log(clamp(., 1e-7)))
 * followed by (x - mel_mean) / mel_std -- reference matcha/utils/model.py normalize as matcha/utils/precompute_mels.py:100-113
 * applies it (hop 128 there = the style encoder's "fine" mel; mel_mean 0 and mel_std 1 give the extractor's own output).
 * The object owns its tables (Hann-windowed DFT basis, HTK filterbank: built in fp64 at create, no device needed) and their device
 * copy, which the first mtts_melfe_forward makes on the current device (one allocation and a blocking copy: not inside a stream
 * capture).  n_fft: a multiple of 32 in [64, 2048].
 *   d_audio [B][ld] fp32 in [-1, 1], d_lengths [B] int64 samples (held inside [0, ld]) ->
 *   d_mel [B][n_mels][T_max] fp32, zero at frames >= d_mel_lengths[b] = (len_b / hop) + 1 (held to T_max).
 * T_max >= max_b len_b / hop + 1 keeps every frame.  A clip of at most n_fft / 2 samples after trimming has no reflect padding
 * (torch raises there): it gets d_mel_lengths[b] = 0 and a zero row; callers check lengths on the host where they have them.
 * A clip's rows do not depend on the batch it is in (bit for bit).  Nothing is read outside [0, len_b) of a row.
 * mtts_melfe_basis / _filterbank copy the host tables out: [n_fft][2 * bins] (cos columns then -sin columns, bins = n_fft / 2 + 1
 * = mtts_melfe_n_bins) and [bins][n_mels]. */
typedef struct mtts_melfe mtts_melfe;
mtts_melfe* mtts_melfe_create(int sample_rate, int n_fft, int n_mels);
void mtts_melfe_destroy(mtts_melfe* m);
int mtts_melfe_n_bins(mtts_melfe* m);
int mtts_melfe_basis(mtts_melfe* m, float* h_out, int64_t numel);
int mtts_melfe_filterbank(mtts_melfe* m, float* h_out, int64_t numel);
int64_t mtts_melfe_workspace_bytes(mtts_melfe* m, int B, int64_t ld, int hop);
int mtts_melfe_forward(mtts_melfe* m, const float* d_audio, int64_t ld, const int64_t* d_lengths, int B, int hop, float mel_mean,
                       float mel_std, float* d_mel, int T_max, int64_t* d_mel_lengths, void* d_ws, int64_t ws_bytes, void* stream);

/* StyleEncoder.forward -- reference matcha/models/style_encoder.py:42-72 (n_layers x { x * mask -> Conv1d(k5, pad 2) -> ReLU },
 * masked_mean_pool :36-39, proj_enc and proj_dur) -- on a ragged batch of normalised mels, plus the average over the clips of a
 * voice -- reference matcha/add_speaker.py:60-62.  Tensors are registered under the reference's names ("convs.0.weight",
 * "convs.0.bias", ..., "proj_enc.weight", "proj_enc.bias", "proj_dur.weight", "proj_dur.bias"); weights and workspace as for
 * mtts_vocos_*.  n_feats and hidden: multiples of 4.
 *   d_mel [B][n_feats][T] fp32, d_mel_lengths [B] int64 frames (held inside [0, T]; frames beyond are not read) ->
 *   d_group == NULL: d_e_enc / d_e_dur [B][spk_emb_dim], one row per clip;
 *   d_group [B] int32 (clip -> voice; values outside [0, n_groups) are left out): [n_groups][spk_emb_dim], the mean of the rows of
 *   each voice's clips (a voice without clips gets the zero row).
 * Every sum has a fixed order: a clip's row does not depend on the batch it is in, and two calls give the same bits. */
typedef struct mtts_style mtts_style;
mtts_style* mtts_style_create(int n_feats, int hidden, int n_layers, int spk_emb_dim);
void mtts_style_destroy(mtts_style* v);
int mtts_style_set_tensor(mtts_style* v, const char* key, const float* h_data, int64_t numel);
int64_t mtts_style_weights_bytes(mtts_style* v);
int mtts_style_upload_weights(mtts_style* v, void* d_weights, int64_t bytes);
int64_t mtts_style_workspace_bytes(mtts_style* v, int B, int T);
int mtts_style_forward(mtts_style* v, const float* d_mel, const int64_t* d_mel_lengths, int B, int T, const int32_t* d_group,
                       int n_groups, float* d_e_enc, float* d_e_dur, void* d_ws, int64_t ws_bytes, void* stream);

/* Parameter gradients of the style encoder, for training it on the device (reference StyleEncoderLightningModule,
 * matcha/models/style_encoder.py:75-160; the optimiser and the matching loss are the caller's).
 *
 * The parameters as ONE flat fp32 buffer in the reference's state-dict order: convs.i.weight [hidden, cin, 5], convs.i.bias [hidden]
 * for every layer, then proj_enc.weight [E, hidden], proj_enc.bias [E], proj_dur.weight, proj_dur.bias.  mtts_style_param_count is
 * its length in floats, mtts_style_param_offset(v, key) the first float of a tensor (-1: no such key).
 *
 * mtts_style_forward_taped: the launches of mtts_style_forward with d_group == NULL, one activation buffer per layer and the pooled
 *   rows kept in d_ws (mtts_style_grad_workspace_bytes); d_e_enc / d_e_dur [B, E] equal mtts_style_forward's bit for bit.
 *   mtts_style_grad_tape_offset(v, B, T, which): byte offset in d_ws of which = 0 the masked channels-last input rows
 *   [B*T, round_up(n_feats, 4)], 1 .. n_layers the ReLU output of layer which - 1 [B*T, hidden], n_layers + 1 the pooled rows
 *   [B, hidden], n_layers + 2 the prefix mask [B*T].
 * mtts_style_backward: from that tape (same d_ws, B, T, d_mel_lengths) and upstream d_g_enc, d_g_dur [B, E], the gradient of
 *   sum_b <g_enc_b, e_enc_b> + <g_dur_b, e_dur_b> with respect to every parameter -> d_param_grad [mtts_style_param_count], every
 *   float written.  Projections: d W[o,c] = sum_b g[b,o] pooled[b,c] in batch order, d b[o] = sum_b g[b,o], d pooled = g W.  Pool:
 *   d pooled / max(len_b, 1) on the frames t < len_b.  Per layer, last to first: the gate (H_l > 0) times the prefix mask, the bias
 *   and weight gradients (mtts_conv_wgrad below), and for layers >= 1 the data gradient as a GEMM with the transposed, tap-reversed
 *   panel in NATIVE FP32 MFMA (arithmetic 0) whatever the forward arithmetic is.  Those panels are packed on demand from the
 *   registered tensors into a buffer of their own (mtts_style_grad_weights_bytes / mtts_style_grad_upload_weights;
 *   mtts_style_set_tensor invalidates them) and passed as d_grad_buf.  A clip of length 0 contributes exactly zero.  Every sum has a
 *   fixed order and there are no floating-point atomics: two calls give the same bits.  Stream-ordered, no allocation.
 *   Both return -1 (mtts_last_error) for null pointers, B < 1, T < 1, a small workspace, weights (or backward panels) not uploaded.
 *   The clip average (d_group) has no taped form. */
int64_t mtts_style_param_count(mtts_style* v);
int64_t mtts_style_param_offset(mtts_style* v, const char* key);
int64_t mtts_style_grad_weights_bytes(mtts_style* v);
int mtts_style_grad_upload_weights(mtts_style* v, void* d_buf, int64_t bytes);
int64_t mtts_style_grad_workspace_bytes(mtts_style* v, int B, int T);
int64_t mtts_style_grad_tape_offset(mtts_style* v, int B, int T, int which);
int mtts_style_forward_taped(mtts_style* v, const float* d_mel, const int64_t* d_mel_lengths, int B, int T, float* d_e_enc,
                             float* d_e_dur, void* d_ws, int64_t ws_bytes, void* stream);
int mtts_style_backward(mtts_style* v, const int64_t* d_mel_lengths, int B, int T, const float* d_g_enc, const float* d_g_dur,
                        float* d_param_grad, void* d_grad_buf, void* d_ws, int64_t ws_bytes, void* stream);

/* Kernel-level entry of the Conv1d(k5, pad 2) weight gradient (no context):
 *   d_dw[co, ci, k] = sum over rows r = (b, t), t < len_b, of d_dz[r, co] * d_x[(b, t + k - 2), ci]     (taps outside [0, len_b) are zero)
 * d_dz [B*T, cout] and d_x [B*T, ldx] (ldx >= cin) channels-last fp32 rows, d_lengths int64 [B] (held inside [0, T]) or NULL (every
 * clip has T frames) -> d_dw [cout, cin, 5] in torch's layout and d_db [cout] = the column sums of d_dz (NULL: not computed).  What
 * lies at t >= len_b is never used as data, and clips that are neighbours in memory do not see each other.  Exact fp32 FMA chains
 * (v_mfma_f32_32x32x2_f32).  The rows are cut into chunks of mtts_conv_wgrad_chunk_rows(B, T) rows -- 256 up to 4096 rows, beyond
 * that the multiple of 256 that gives at most 16 chunks: a function of the shape alone -- each chunk is one serial sum in row order,
 * the partial results go to d_ws ([chunks, 5, cout, cin] then [chunks, cout]; mtts_conv_wgrad_workspace_bytes) and a second kernel
 * adds them in chunk order.  No atomics: two calls give the same bits. */
int mtts_conv_wgrad_chunk_rows(int B, int T);
int64_t mtts_conv_wgrad_workspace_bytes(int B, int T, int cin, int cout);
int mtts_conv_wgrad(const float* d_dz, const float* d_x, const int64_t* d_lengths, int B, int T, int cin, int ldx, int cout,
                    float* d_dw, float* d_db, void* d_ws, int64_t ws_bytes, void* stream);

/* ---------------------------------------------------------------- sample-rate conversion */

/* A ragged batch of fp32 clips from orig_freq to new_freq: the windowed-sinc polyphase interpolation that
 * torchaudio.functional.resample documents as its default (resampling_method "sinc_interp_hann", lowpass_filter_width 6, rolloff
 * 0.99; the reference converts with it, matcha/utils/utmos_validate.py:78), restated from its formulae -- not pinned to the
 * package.  With g = gcd(orig_freq, new_freq), o = orig_freq / g, n = new_freq / g, lpw = lowpass_filter_width:
 *     base = min(o, n) * rolloff,  width = ceil(lpw * o / base),  taps = 2 * width + o
 *     t = clamp((-p / n + (k - width) / o) * base, -lpw, lpw)                            phase p in [0, n), tap k in [0, taps)
 *     K[p][k] = (t == 0 ? 1 : sin(pi t) / (pi t)) * cos(t pi / lpw / 2)^2 * (base / o)   in fp64, rounded once to fp32
 *     out_len(L) = ceil(n L / o)
 *     out[q n + p] = sum_k K[p][k] * x[q o + k - width]   with x = 0 outside [0, L), for q n + p < out_len(L)
 * The fp32 table is the definition.  After the rounding the taps at the clamp are exact zeros, so each phase has a band of `band`
 * consecutive taps (the widest first-to-last non-zero run of any phase) outside which it is zero; only the band is kept on the
 * device and evaluated.
 *
 * The object owns the host table (built at create, no device needed) and the banded device copy, which the first
 * mtts_resample_forward makes on the current device (one allocation and a blocking copy: not inside a stream capture; one object
 * per device).  mtts_resampler_create returns NULL (mtts_last_error says why) for a rate outside [4000, 384000], equal rates,
 * lowpass_filter_width < 1, rolloff outside (0, 1], a banded bank of more than MTTS_RESAMPLE_MAX_BANK floats (n * band: rate
 * pairs with a small common divisor), or a rate pair whose bank, input span of one tile (about MTTS_RESAMPLE_TILE * o / n samples)
 * and output tile exceed MTTS_RESAMPLE_LDS_BYTES of LDS (decimation by more than about 12).  Every pair of {8000, 11025, 16000,
 * 22050, 24000, 32000, 44100, 48000, 96000} with 24000 is admitted.
 *
 * Host-only queries: mtts_resample_factors (any pointer may be NULL), mtts_resample_out_length = out_len(L), and
 * mtts_resample_bank, which copies the dense fp32 table [n][taps] out.  mtts_resample_tile = MTTS_RESAMPLE_TILE as built.
 *
 * mtts_resample_forward: d_in [B][ld_in], d_out [B][ld_out] fp32 with 16-byte aligned rows (ld % 4 == 0, as
 * mtts_waveform_finish requires), d_lengths device int64 [B].  Row b of d_out receives out_len(len_b) samples followed by zeros
 * up to ld_out, and d_out_lengths[b] that count; len_b == 0 gives 0 samples.  One launch gridded over (output tile, clip).
 *   Every output sample is ONE fp32 sum in a fixed order: s = 0, then s = s + K[p][k] * x[.] for k ascending over the phase's
 *   band, the product and the sum each rounded to fp32 (no FMA), no atomics.  For finite input that has the bits of the dense sum
 *   over k = 0 .. taps - 1 in ascending order.  A clip's samples therefore do not depend on the batch it is in, two calls give the
 *   same bits, and a NumPy fp32 restatement in that order reproduces them bit for bit.
 *   The lengths are checked on the device without a host read: a len_b outside [0, ld_in], or one whose out_len exceeds ld_out,
 *   gives row b zero output and d_out_lengths[b] = -1; the other rows are unaffected.  Nothing is ever read outside [0, len_b) of
 *   a row or written outside the row.  mtts_resample_status(d_ws, stream) -- the one entry here that waits for the stream --
 *   reports the first refused row through mtts_last_error.
 * Stream-ordered, no allocation, no synchronisation (mtts_resample_status excepted).  Workspace: mtts_resample_workspace_bytes,
 * 16-byte aligned.  What the host can see (null pointers, B < 1, an ld that is no multiple of 4, a small workspace) returns -1. */
#define MTTS_RESAMPLE_TILE 1024        /* output samples per workgroup */
#define MTTS_RESAMPLE_MAX_BANK 6144    /* floats of the banded bank (n * band) the kernel keeps in LDS */
#define MTTS_RESAMPLE_LDS_BYTES 65536  /* bank + first-tap table + one tile's input span + the output tile */
typedef struct mtts_resampler mtts_resampler;
mtts_resampler* mtts_resampler_create(int orig_freq, int new_freq, int lowpass_filter_width, double rolloff);
void mtts_resampler_destroy(mtts_resampler* r);
int mtts_resample_tile(void);
int mtts_resample_factors(mtts_resampler* r, int* o, int* n, int* width, int* taps, int* band);
int64_t mtts_resample_out_length(mtts_resampler* r, int64_t L);
int mtts_resample_bank(mtts_resampler* r, float* h_K, int64_t numel);
int64_t mtts_resample_workspace_bytes(mtts_resampler* r, int B, int64_t ld_in);
int mtts_resample_forward(mtts_resampler* r, const float* d_in, int64_t ld_in, const int64_t* d_lengths, int B, float* d_out,
                          int64_t ld_out, int64_t* d_out_lengths, void* d_ws, int64_t ws_bytes, void* stream);
int mtts_resample_status(const void* d_ws, void* stream);

/* ---------------------------------------------------------------- corpus preparation: silence, mel statistics */

/* What the reference does to a corpus before training, one file at a time on the host -- matcha/utils/measure_silence.py:66-132,
 * matcha/utils/normalize_silence.py:86-220 and the per-file sums of matcha/utils/generate_data_statistics.py:120-131 -- for a
 * ragged batch on the device.  Rows as for mtts_resample_forward: fp32 [B][ld] with ld % 4 == 0 and 16-byte aligned, lengths
 * device int64 [B], checked on the device without a host read; stream-ordered, no allocation; nothing is read outside [0, len_b)
 * of a row and nothing is written outside a row; what the host can see (null pointers, B < 1, a bad ld, a small workspace)
 * returns -1; mtts_silence_status / mtts_mel_stats_status(d_ws, stream) -- the only entries here that wait -- report the first
 * refused row of the latest call on that workspace through mtts_last_error.
 *
 * Windows.  W = mtts_silence_window(sample_rate) = (int)(0.01 * sample_rate) samples, anchored at sample 0; a clip of L samples has
 * ceil(L / W) windows.  The last, partial window counts: its sum runs over the samples that exist and is divided by W (the
 * reference pads with zeros).  rms[w] = (float)sqrt(q / W), q the sum of the exact squares in fp64 in a fixed shape: with VEC = 4
 * when W % 4 == 0 and VEC = 1 otherwise, lane l of 64 adds, in ascending order, the squares of the window's samples
 * e = VEC * (l + 64 k) + j (k = 0, 1, ...; j = 0 .. VEC - 1; e < W and inside the clip); then six steps v[l] = v[l] + v[l ^ o],
 * o = 32, 16, 8, 4, 2, 1.  (mtts_waveform_finish's arithmetic.)  Thresholds are (float)pow(10, db / 20), compared in fp32.
 *
 * mtts_silence_measure: d_out int64 [B][6], in samples:
 *   [0] content_start = W * (first window with rms >= thr_effective)
 *   [1] content_end   = min(W * (last such window + 1), L);  both 0 for a clip without such a window
 *   [2] leading_eff, [3] leading_abs, [4] trailing_eff, [5] trailing_abs = W * the length of the leading / trailing run of
 *       windows with rms < thr (effective, absolute).
 * These are the reference's numbers, quirks included: a trailing run counts the zero-padded last window, so trailing_* can exceed
 * the silence that is there by up to W - 1 samples (a silent clip of 3000 samples at 24 kHz reports 3120 in [2..5]); a NaN window
 * is neither "at or above" nor "below": it starts no content and ends a silent run.  L == 0 gives six zeros; a length outside
 * [0, ld] gives six -1, the other rows are unaffected.  Two launches (windows, then one scan per clip); a clip's numbers do not
 * depend on the batch it is in.
 *
 * mtts_silence_normalize: row b of d_out [B][ld_out] becomes
 *     [lead_target zeros, or in[0 : content_start] when lead_target == -1] + in[content_start : content_end]
 *     + [trail_target zeros, or in[content_end : L] when trail_target == -1],      then zeros up to ld_out,
 * with (content_start, content_end) read from d_bounds [B][6] on the device (mtts_silence_measure's d_out), d_out_lengths[b] the
 * new length and d_changed[b] = 0 when every end being normalised already has exactly its target count -- the reference's integer
 * comparison, current_leading = content_start, current_trailing = L - content_end -- in which case the row is a copy of the
 * input, else 1.  Samples are moved, never recomputed.  One launch gridded over (output tile, clip); d_out must not be d_in.
 * A row whose new length exceeds ld_out, whose length is outside [0, ld_in] or whose bounds are not 0 <= start <= end <= L gets
 * d_out_lengths[b] = -1 and zeros.  The host refuses a target that is neither -1 nor a whole multiple of W (reference :139-154).
 *
 * mtts_mel_stats: d_mel [B][F][T] fp32 (any F, any T), d_lengths int64 [B] frames ->
 *   d_sums double [B][2] = (sum x, sum x * x) over f < F, t < len_b;  d_frames int64 [B] = len_b;  d_flags int32 [B] = 1 when one
 *   of those x is NaN or Inf (the reference leaves such a file out, :52-53).  Frames at or beyond len_b are never read.
 *   The order is a function of (f, t) only -- not of T, the batch or the grid: with C = mtts_mel_stats_chunk() = 256, chunk c of a
 *   clip holds frames [C c, C c + C); lane i of the chunk starts from 0.0 and adds x[f][C c + i] (x * x likewise; both exact in
 *   fp64) for f = 0 .. F - 1 in ascending order, a lane at or beyond len_b keeping 0.0; each group of 64 consecutive lanes runs
 *   the steps v[i] = v[i] + v[i ^ o], o = 32 .. 1; the four groups meet as ((g0 + g1) + g2) + g3; the clip's sum starts from 0.0
 *   and adds its ceil(len_b / C) chunks in ascending c.  A NumPy fp64 restatement in that order reproduces the bits.
 *   len_b == 0 gives zeros; a len_b outside [0, T] gives zeros and d_frames[b] = -1.  Two launches. */
int mtts_silence_window(int sample_rate);
int64_t mtts_silence_workspace_bytes(int64_t ld, int B, int sample_rate);
int mtts_silence_measure(const float* d_audio, int64_t ld, const int64_t* d_lengths, int B, int sample_rate, double effective_db,
                         double absolute_db, int64_t* d_out, void* d_ws, int64_t ws_bytes, void* stream);
int mtts_silence_normalize(const float* d_in, int64_t ld_in, const int64_t* d_lengths, const int64_t* d_bounds, int B,
                           int sample_rate, int64_t lead_target, int64_t trail_target, float* d_out, int64_t ld_out,
                           int64_t* d_out_lengths, int32_t* d_changed, void* d_ws, int64_t ws_bytes, void* stream);
int mtts_silence_status(const void* d_ws, void* stream);
int mtts_mel_stats_chunk(void);
int64_t mtts_mel_stats_workspace_bytes(int B, int T);
int mtts_mel_stats(const float* d_mel, int F, int T, const int64_t* d_lengths, int B, double* d_sums, int64_t* d_frames,
                   int32_t* d_flags, void* d_ws, int64_t ws_bytes, void* stream);
int mtts_mel_stats_status(const void* d_ws, void* stream);

/* ---------------------------------------------------------------- pitch: F0 contours and per-clip statistics */

/* How high a voice speaks and whether it rises at the end: the fundamental frequency of every frame of a ragged batch by YIN
 * (de Cheveigne & Kawahara, JASA 111 (4), 2002), stated so that it cuts into blocks, and exact order statistics of a contour.
 * Rows as for mtts_silence_measure: d_audio fp32 [B][ld] with ld % 4 == 0 and 16-byte aligned, d_lengths device int64 [B], judged
 * on the device; a length outside [0, ld] gives d_frames[b] = -1 for that row (its columns hold the fill values) and leaves the
 * other rows alone; stream-ordered, no allocation, one workspace of mtts_pitch_workspace_bytes; what the host can see (null
 * pointers, B < 1, a bad ld, parameters outside the ranges below, a small ld_frames, a small workspace) returns -1;
 * mtts_pitch_status(d_ws, stream) -- the only entry here that waits -- reports the first refused row of the latest call on that
 * workspace through mtts_last_error.  A row's numbers do not depend on its batch or its place in it.
 *
 * Parameters.  sample_rate fs in [8000, 48000]; hop H in [8, 512] samples; fmin, fmax in Hz; threshold thr in (0, 1), compared in
 * fp32 as (float)threshold.  Window W = 8 H; largest lag tmax = ceil(fs / fmin), smallest lag tmin = floor(fs / fmax), both from the
 * double quotient; refused unless 2 <= tmin and tmin + 2 <= tmax <= MTTS_PITCH_MAX_LAG.  mtts_pitch_plan reports (W, tmin, tmax) or
 * refuses the same way.
 *
 * Frames.  A clip of L samples has n = 0 frames when L < W + tmax, else n = (L - W - tmax) / H + 1.  Frame k reads samples
 * [k H, k H + W + tmax) and nothing else: no padding, no read outside [0, L).  Its nominal time is (k H + (W + tmax) / 2) / fs.
 * ld_frames must be at least max(1, frames of a clip of ld samples).
 *
 * Difference function, all in fp32 without fused multiply-adds.  Block b of a clip is samples [b H, b H + H); its sums are
 *     s_b(tau) = sum_{j < H} (x[b H + j] - x[b H + j + tau])^2,   tau = 1 .. tmax:
 *   start from 0.0f and, for j = 0, 1, .. H - 1 in that order, d = x[b H + j] - x[b H + j + tau]; s = s + d * d (three roundings).
 *   A frame's sums are its eight blocks' in ascending order,
 *     d_k(tau) = ((((((s_k + s_k+1) + s_k+2) + s_k+3) + s_k+4) + s_k+5) + s_k+6) + s_k+7.
 *   Each block sum is computed once (mtts_pitch_tile() = 8 blocks per workgroup, which stages its samples once) and used by the
 *   eight frames that hold the block; the order is a function of (b, tau, j) only -- not of the batch, the grid or the tile.
 * Cumulative-mean normalisation.  c(tau) = sum_{u <= tau} d(u) in this shape: lag tau belongs to group g = (tau - 1) / 16, place
 *   i = (tau - 1) % 16 (64 groups; d(u) = 0.0f beyond tmax).  Inside a group r_g(i) = (..((0.0f + d(16 g + 1)) + d(16 g + 2)).. +
 *   d(16 g + i + 1)), and t_g = r_g(15).  The inclusive scan of t over the groups is six steps v[g] = v[g] + v[g - o] for every
 *   g >= o at once, o = 1, 2, 4, 8, 16, 32; P_g = v[g - 1] after them, P_0 = 0.0f.  c(tau) = P_g + r_g(i).
 *   d'(tau) = (d(tau) * (float)tau) / c(tau) when c(tau) > 0, else 1.0f (the division correctly rounded).
 * Walk.  The first tau in [tmin, tmax) with d'(tau) < thr; from there one step to the right while tau + 1 < tmax and
 *   d'(tau + 1) < d'(tau).  Without such a tau: the lowest-index minimum of d' over [tmin, tmax).  tau* is the lag reached.
 * Outputs per frame.  aperiodicity = d'(tau*).  The frame is voiced when d'(tau*) < thr; f0 = (float)fs / ((float)tau* + delta)
 *   when voiced, else 0.  With a = d'(tau* - 1), b = d'(tau*), c = d'(tau* + 1): delta = (0.5f * (a - c)) / ((a - b) + (c - b)),
 *   the offset of the three-point parabola's vertex (0.5 (a - c) / (a - 2 b + c)), taken only when tmin < tau* < tmax - 1 and the
 *   denominator as computed is > 0; otherwise delta = 0.  A frame that reads a NaN or an Inf sample reports f0 = 0 and aperiodicity =
 *   NaN -- exactly the frames k with such a sample in [k H, k H + W + tmax); the other frames are unaffected.  Columns at or beyond n
 *   (up to ld_frames) hold f0 = 0, aperiodicity = 1.  Two launches: block sums gridded over (tile of blocks, clip), then (eight
 *   frames, clip).
 *
 * mtts_pitch_stats: d_f0 [B][ld_frames] and d_frames int64 [B] as mtts_pitch_track wrote them -> exact order statistics of the
 *   voiced values (f0 > 0) of the first d_frames[b] columns, by radix select on their bit patterns.  With the m voiced values sorted
 *   ascending as v[0 .. m): d_out_hz float [B][4] = (v[(m - 1) / 20], v[(m - 1) / 2], v[19 (m - 1) / 20], tail median) -- the 5 %,
 *   50 % and 95 % points, integer division -- where the tail is the voiced frames with index >= (last voiced index) - tail_frames
 *   and its median is t[(mt - 1) / 2] of its mt sorted values; d_counts int64 [B][3] = (frames, m, mt).  m == 0 gives four NaN;
 *   mt < 3 gives a NaN tail median.  A row with d_frames[b] outside [0, ld_frames] (a row mtts_pitch_track refused) gives four NaN
 *   and counts (-1, 0, 0), and is what mtts_pitch_status reports for this call.  One launch, one workgroup per row; the workspace
 *   holds the verdict only (256 bytes). */
#define MTTS_PITCH_MAX_LAG 1024
int mtts_pitch_tile(void);
int mtts_pitch_plan(int sample_rate, int hop, double fmin, double fmax, int* window, int* min_lag, int* max_lag);
int64_t mtts_pitch_workspace_bytes(int64_t ld, int B, int sample_rate, int hop, double fmin, double fmax);
int mtts_pitch_track(const float* d_audio, int64_t ld, const int64_t* d_lengths, int B, int sample_rate, int hop, double fmin,
                     double fmax, double threshold, float* d_f0, float* d_aper, int64_t ld_frames, int64_t* d_frames, void* d_ws,
                     int64_t ws_bytes, void* stream);
int mtts_pitch_stats(const float* d_f0, int64_t ld_frames, const int64_t* d_frames, int B, int64_t tail_frames, float* d_out_hz,
                     int64_t* d_counts, void* d_ws, int64_t ws_bytes, void* stream);
int mtts_pitch_status(const void* d_ws, void* stream);

/* ---------------------------------------------------------------- prosody: a path through pitch candidates, pitch and energy per token */

/* Plain YIN decides every frame alone, and a frame whose odd harmonics dip is reported an octave high.  The three entries below
 * add what a per-token pitch needs: several candidate periods per frame with a probability mass each (the idea of pYIN: Mauch &
 * Dixon, ICASSP 2014, with a threshold prior whose CDF needs no transcendental), one shortest path per clip through them, and the
 * fold of a contour onto token marks.  mtts_pitch_track is untouched.  Rows, refusals, status and workspaces follow the "pitch"
 * section above; mtts_pitch_status words the verdict of these entries too.  fp32, no fused multiply-adds, divisions correctly rounded.
 *
 * mtts_pitch_candidates: the arguments, frame layout, block sums, d'(tau), d_frames and the workspace (mtts_pitch_workspace_bytes)
 *   of mtts_pitch_track.  Per frame, with thr2 = 2.0f * (float)threshold:
 *   Record-setting dips.  Scan tau ascending over tmin < tau < tmax - 1.  tau is a dip when d'(tau) < d'(tau - 1) and
 *     d'(tau) <= d'(tau + 1).  A dip is kept when its depth b = d'(tau) is below every depth kept before it and below thr2.
 *   Mass, under a threshold prior uniform on [0, 2 thr]: F(v) = min(max(v / thr2, 0), 1); mass = F(previous kept depth) - F(b),
 *     where F of "no previous" is exactly 1.0f.  The frame's unvoiced mass is F(last kept depth), or 1.0f with no dip kept.
 *   Period.  p = (float)tau + delta, delta by the parabola rule of mtts_pitch_track: (0.5f * (a - c)) / ((a - b) + (c - b)) when that
 *     denominator as computed is > 0, else 0.
 *   Limit.  At most MTTS_PITCH_CANDS = 8 per frame: with more kept, the 8 of greatest mass, ties to the lower lag.  Ascending lag.
 *   Outputs.  d_period, d_mass, d_depth float [B][ld_frames][8] (unused places 0), d_count int32 [B][ld_frames], d_unvoiced_mass and
 *     d_floor float [B][ld_frames]; floor = the lowest-index minimum of d' over [tmin, tmax), which is what YIN reports for an unvoiced
 *     frame.  A frame that read a NaN or Inf sample: count = -1, no candidates, unvoiced mass 1, floor NaN.  Columns at or beyond the
 *     row's frame count: count = 0, unvoiced mass = 1, floor = 1.  Two launches: block sums, then (eight frames, clip); a wave per
 *     frame and a lane per 16 lags.  A minimum rounds nothing, so the running record is the same bits in any scan shape.
 *
 * mtts_pitch_viterbi: a lattice as mtts_pitch_candidates wrote it (or made by hand: no audio is read) and d_frames [B] -> one path
 *   per clip.  States of a frame: its candidates 0 .. count - 1 (count above 8 is read as 8) and U (unvoiced), index 8, last.
 *   Local cost: 1.0f - mass of a candidate, 1.0f - unvoiced mass of U; a frame with count < 0 has only U, at cost 0.
 *   Transition from state r of frame k - 1 to state s of frame k: voiced to voiced (float)jump * (fabsf(p_s - p_r) / fminf(p_s, p_r))
 *     -- an octave costs jump --, voiced to or from U (float)switch_cost, U to U 0.
 *   Recurrence.  D_0(s) = local_0(s); D_k(s) = (min_r (D_{k-1}(r) + trans(r, s))) + local_k(s), the minimum over r ascending with
 *     strict <, so the lowest index wins a tie; then, at every k including 0, D_k(s) <- D_k(s) - min_s D_k(s) (one rounding), so the
 *     costs stay near 1 however long the clip is.  The end state is the lowest-index minimum of the last frame; the path is walked
 *     back from it.
 *   Outputs in mtts_pitch_track's format, so mtts_pitch_stats takes them unchanged: f0 = (float)fs / p of the chosen candidate or 0
 *     for U; aperiodicity = the chosen candidate's depth, for U the frame's floor, NaN for a frame with count < 0; d_state int8
 *     [B][ld_frames] the chosen state (8 = U).  Columns at or beyond d_frames[b]: f0 = 0, aperiodicity = 1, state = -1.  A row with
 *     d_frames[b] outside [0, ld_frames] is refused through the verdict and holds those fill values in every column.  0 <= jump,
 *     switch_cost <= 1e6.  One launch, one wavefront per clip: sequential in frames.  Workspace: mtts_pitch_viterbi_workspace_bytes
 *     (the verdict and one 64-bit word of nine 4-bit back pointers per frame).
 *
 * mtts_pitch_fold: d_f0 [B][ld_frames] and d_frames [B] as mtts_pitch_track or mtts_pitch_viterbi wrote them with (hop H, window W,
 *   max_lag tmax); d_marks int64 [B][Tx][2] = (start, end) of every token in samples of the clip, as mtts_token_timing writes them
 *   ((-1, -1): no token); d_x_lengths int64 [B]; optionally the audio fp32 [B][ld] with d_lengths [B] (d_lengths alone may be given
 *   too: it bounds the marks).
 *   Membership.  Frame k belongs to token i when 2 start_i <= 2 k H + W + tmax < 2 end_i: the nominal centre, in integers; a token's
 *     frames are [f(start), f(end)) with f(m) = min(n, max(0, ceil((2 m - W - tmax) / (2 H)))).
 *   Per token.  d_counts int32 [B][Tx][2] = (frames, voiced: f0 > 0).  d_hz float [B][Tx][3] = (median, first voiced, last voiced):
 *     the median is the exact order statistic v[(m - 1) / 2] of the token's m voiced values sorted ascending; m == 0 gives three NaN.
 *   With audio: d_mean_square double [B][Tx] = the fp64 sum of x^2 over [start, end) divided by (double)(end - start), in an order
 *     that is a function of (start, end) only: partial sum l = 0 .. 63 starts from 0.0 and adds x[start + l + 64 j]^2 (exact in
 *     fp64) for j = 0, 1, .. while the index is below end; then v[l] = v[l] + v[l ^ o] for every l at once, o = 32, 16, 8, 4, 2, 1;
 *     the sum is v[0].  0 for an empty token; NaN where a sample is not finite.
 *   Refusals, through the verdict, touching no other row: d_frames[b] outside [0, ld_frames]; d_x_lengths[b] outside [0, Tx]; a
 *     length below 0 (or above ld with audio); a mark outside [0, length]; start > end; a start below the end of the token before
 *     it.  Every token of a refused row holds counts (-1, 0), three NaN and a NaN mean square.  Tokens at or beyond d_x_lengths[b],
 *     and tokens with marks (-1, -1), hold the fill values: counts (0, 0), three NaN, mean square 0.  One launch, a wave per token;
 *     the workspace holds the verdict only (256 bytes). */
#define MTTS_PITCH_CANDS 8
int mtts_pitch_candidates(const float* d_audio, int64_t ld, const int64_t* d_lengths, int B, int sample_rate, int hop, double fmin,
                          double fmax, double threshold, float* d_period, float* d_mass, float* d_depth, int32_t* d_count,
                          float* d_unvoiced_mass, float* d_floor, int64_t ld_frames, int64_t* d_frames, void* d_ws, int64_t ws_bytes,
                          void* stream);
int64_t mtts_pitch_viterbi_workspace_bytes(int64_t ld_frames, int B);
int mtts_pitch_viterbi(const float* d_period, const float* d_mass, const float* d_depth, const int32_t* d_count,
                       const float* d_unvoiced_mass, const float* d_floor, int64_t ld_frames, const int64_t* d_frames, int B,
                       int sample_rate, double jump, double switch_cost, float* d_f0, float* d_aper, int8_t* d_state, void* d_ws,
                       int64_t ws_bytes, void* stream);
int mtts_pitch_fold(const float* d_f0, int64_t ld_frames, const int64_t* d_frames, int B, int hop, int window, int max_lag,
                    const int64_t* d_marks, int Tx, const int64_t* d_x_lengths, const float* d_audio, int64_t ld,
                    const int64_t* d_lengths, int32_t* d_counts, float* d_hz, double* d_mean_square, void* d_ws, int64_t ws_bytes,
                    void* stream);

/* ---------------------------------------------------------------- long texts: finished rows joined into documents */

/* The last step of a text longer than one utterance: its sentences are rows of one ragged batch, and the rows mtts_waveform_finish
 * leaves are joined here into one waveform per document, before any rate conversion or encoding.  The reference has no counterpart
 * (its handler refuses a text above 1000 characters, server.py:31,94-96): the arithmetic below is the definition, and a torch fp32
 * restatement in that order reproduces every word (tests/join_restated.py).  Rows as for mtts_resample_forward: fp32 [B][ld] with
 * ld % 4 == 0 and 16-byte aligned; nothing is read on the host on the way in.
 *   d_lengths   device int64 [B]: kept samples of row b (mtts_waveform_finish's d_out_lengths; -1 = refused upstream)
 *   d_scale     device fp32 [B] or NULL: the gain mtts_waveform_finish applied to row b (0.95 / peak, or 1)
 *   d_first_row device int32 [G + 1]: document g is the rows [first_row[g], first_row[g + 1]) in speaking order;
 *               0 = first_row[0] < first_row[1] < ... < first_row[G] = B (no document is empty)
 *   d_gap       device int64 [B]: samples of silence after row b, inside [0, gap_max]; the entry of a document's last row is not read
 *   d_out [G][out_ld] fp32 (out_ld % 4 == 0, 16-byte aligned, not overlapping d_audio), d_out_lengths int64 [G], d_starts int64 [B].
 * Layout (int64, a function of the document alone): starts[b] = the sum of len_r + gap_r over the rows r of b's document before b;
 * out_lengths[g] = starts[last] + len_last.  Row g of d_out holds, for each row b of the document, len_b samples at starts[b], zeros
 * in the gaps and zeros from out_lengths[g] to out_ld: every word is written exactly once, the buffer needs no clearing.
 * Samples (fp32, every operation rounded once, no FMA), x = audio[b][i]:
 *   gain:  g_doc = the minimum of scale over the document's rows (1 when d_scale is NULL), r_b = g_doc / scale[b], one division per
 *          row; x = x * r_b unless r_b == 1.0f, when the sample is moved bit for bit.  A document therefore carries ONE gain, that
 *          of its loudest sentence, instead of one per sentence.
 *   fade:  F' = min(fade, len_b / 2) (integer division).  Sample i < F' of a row that is not the first of its document, and sample
 *          len_b - 1 - i (i < F') of a row that is not the last, become x * w with w = (float)(2 i + 1) / (float)(2 F'); together
 *          y = (x * r_b) * w.  The two ends of a document keep their samples; fade == 0 applies no weight at all.
 * Checks, on the device, before anything is indexed with these values; the verdict is that of the other ragged-batch entries
 * (mtts_wave_join_status(d_ws, stream), the only entry here that waits, words it through mtts_last_error):
 *   reason 1: a len_b outside [0, ld];  reason 2: the layout breaks, or a gap is outside [0, gap_max];  reason 3: the document is
 *   longer than out_ld.  A document with such a row is refused as a whole: out_lengths[g] = -1, its rows' starts = -1, its row of
 *   d_out zeros; the other documents are not touched.  Where the layout breaks at document g, the documents before g stand and
 *   those from g on are refused (their rows' starts are -1); the row reported is the first one no standing document holds (held to
 *   B - 1).  Header words (int64): first refused row + 1 or 0, its length (saturated to 32 bits), ld, the reason, out_ld, gap_max.
 * Two launches: one workgroup plans (a wave per document, 64 rows per step), then a gather gridded over (tile of 2048 output samples,
 * document) with 16-byte stores; a document is spread over the grid.  Stream-ordered, no allocation.  What the host can see returns
 * -1 and launches nothing: null pointers, B < 1, G < 1, G > B, B > 65535, an ld or out_ld that is no positive multiple of 4, a
 * misaligned d_audio / d_out / d_ws, d_out overlapping d_audio, fade < 0, gap_max < 0, a small workspace. */
int64_t mtts_wave_join_workspace_bytes(int64_t B, int64_t G);
int mtts_wave_join(const float* d_audio, int64_t ld, const int64_t* d_lengths, const float* d_scale, const int32_t* d_first_row,
                   const int64_t* d_gap, int B, int G, int64_t fade, int64_t gap_max, float* d_out, int64_t out_ld,
                   int64_t* d_out_lengths, int64_t* d_starts, void* d_ws, int64_t ws_bytes, void* stream);
int mtts_wave_join_status(const void* d_ws, void* stream);

/* ---------------------------------------------------------------- token timing: marks out, breaks in */

/* When each token is spoken in the audio mtts_waveform_finish leaves, and pauses cut into that audio after chosen tokens (what SSML
 * calls <break time>), between the trim and the join.  The reference has no counterpart: the arithmetic below is the definition, and
 * a NumPy restatement in that order reproduces every word (tests/timing_restated.py).  All integers are int64 and a function of the
 * row alone, so a row's marks, length and samples do not depend on what shares its batch.
 *   d_cum        device int32 [B][Tx]: inclusive cumulative durations in fine frames (mtts_durations' d_cum)
 *   d_x_lengths  device int64 [B]: tokens of row b, inside [1, Tx]
 *   d_keep       device int64 [B]: kept samples of row b (mtts_waveform_finish's d_out_lengths, or hop * (frames - 1) untrimmed;
 *                -1 = refused upstream), inside [0, keep_max] (the row stride of the audio)
 *   fine_hop     samples per fine frame: half the vocoder hop, 128 at 24 kHz
 *   breaks, optional (d_break_first NULL, NB 0: none), in CSR form: the breaks of row b are [break_first[b], break_first[b + 1]) of
 *                d_break_token int32 [NB] (the break follows this token; strictly increasing within a row, inside [0, x_len)) and
 *                d_break_pause int64 [NB] (samples, inside [0, pause_max])
 * Boundaries of a row: e_0 = 0 and e_k = min(max(fine_hop * cum[k - 1] - fine_hop / 2, 0), keep) for k = 1 .. x_len.  Why the half
 * frame: the mel front end the model was trained on is center=True, so fine frame f is centred on sample f * fine_hop; mtts_align_pool
 * centres coarse frame t on fine frame 2 t, and the iSTFT centres frame t on sample t * hop = 2 t * fine_hop -- so fine frame f of the
 * alignment is centred on sample f * fine_hop of the output too.  Token k - 1 ends with fine frame cum[k - 1] - 1 and token k begins
 * with fine frame cum[k - 1]; e_k is the midpoint between their centres.  The marks are NOMINAL: the decoder and the vocoder have
 * receptive fields of many frames, which smear what is heard around a boundary.
 * Breaks: a break after token j cuts at c_j = e_{j + 1}.  A break with c_j == 0 or c_j >= keep is DROPPED, its applied pause 0 (the trim
 * has removed what follows it); every other break is applied with its pause, a pause of 0 included (a cut without silence).
 * Marks (d_marks int64 [B][Tx][2]): start_i = e_i + P(<i), end_i = e_{i+1} + P(<i), P(<i) the sum of the applied pauses of the breaks at
 * tokens < i; d_out_lengths[b] = keep + P(all).  Tokens at or beyond x_len, and every token of a refused row, read -1; a refused row's
 * length is -1.
 * Checks, on the device, before anything is indexed with these values (the ragged-batch contract): each refuses ITS ROW ALONE.
 *   reason 5: x_len outside [1, Tx];  1: keep outside [0, keep_max];  2: break_first does not ascend inside [0, NB], or a token index
 *   outside [0, x_len);  3: a token index not above the one before it;  4: a pause outside [0, pause_max];  6: cum decreases between two
 *   breaks;  7: keep + P(all) > out_max.  The workspace holds one verdict record per row; mtts_token_timing_status(d_ws, B, stream), the
 *   only entry here that waits, copies them and words the first through mtts_last_error.
 * One launch, one workgroup of 256 per row (the scan of the applied pauses is the duration scan's: serial chunk + block scan); no
 * allocation.  What the host can see returns -1 and launches nothing: null pointers, breaks without tokens or pauses, B < 1,
 * B > 65535, Tx < 1, a fine_hop that is odd or outside [2, 65536], NB outside [0, 2^27] or non-zero without d_break_first, keep_max < 0,
 * out_max < keep_max, pause_max < 0, a misaligned or small workspace. */
int64_t mtts_token_timing_workspace_bytes(int64_t B, int64_t NB);
int mtts_token_timing(const int32_t* d_cum, const int64_t* d_x_lengths, const int64_t* d_keep, int B, int Tx, int fine_hop,
                      int64_t keep_max, const int32_t* d_break_first, const int32_t* d_break_token, const int64_t* d_break_pause,
                      int64_t NB, int64_t pause_max, int64_t out_max, int64_t* d_marks, int64_t* d_out_lengths, void* d_ws,
                      int64_t ws_bytes, void* stream);
int mtts_token_timing_status(const void* d_ws, int B, void* stream);

/* The breaks in the audio: a gather over the lengthened rows, from the plan the latest mtts_token_timing left in d_ws (same B, NB and
 * d_break_first).  Rows as for mtts_wave_join: fp32 [B][ld] and [B][out_ld], ld and out_ld positive multiples of 4, 16-byte aligned,
 * not overlapping.  Row b of d_out holds the segments of audio[b][0 .. keep) between its applied cuts in order, `pause` zeros after
 * each applied cut, then zeros from its new length to out_ld: every word is written exactly once; a refused row is zeros.
 * Fade, the join's own rule: for a segment of n samples F' = min(fade, n / 2) (integer division); sample i < F' of a segment that lies
 * behind a cut, and sample n - 1 - i (i < F') of a segment that lies ahead of one, become x * w, w = (float)(2 i + 1) / (float)(2 F').
 * The two ends of the row keep their samples; fade == 0 applies no weight; every sample outside a fade is moved bit for bit.  Two
 * breaks that cut at one position (tokens of no duration between them) add their pauses; the empty segment between them has no fade.
 * A row without breaks is copied bit for bit.  Gridded over (tile of 2048 output samples, row), 16-byte stores.  The host passes
 * out_ld = ld + the largest sum of requested pauses of a row, rounded up to 4: no host read is needed.  Returns -1 and launches nothing
 * for: null pointers, B < 1, B > 65535, NB out of range, a misaligned row, an ld or out_ld that is no positive multiple of 4,
 * fade < 0, d_out overlapping d_audio, a small workspace. */
int mtts_wave_breaks(const float* d_audio, int64_t ld, const int32_t* d_break_first, int B, int64_t NB, int64_t fade, float* d_out,
                     int64_t out_ld, const void* d_ws, int64_t ws_bytes, void* stream);

/* ---------------------------------------------------------------- encoded audio: PCM16, G.711 mu-law / A-law */

/* The last stage out and the first stage in: a ragged batch of fp32 rows to the bytes a client is sent (s16le for the OpenAI
 * route's "pcm" and "wav", G.711 for an 8 kHz telephony leg), and a ragged batch of such bytes back to fp32 for the recording
 * entries.  One launch each, gridded over (tile of MTTS_CODEC_TILE samples, row); every row has its own format.  Every byte is
 * defined by the arithmetic below, which a NumPy restatement reproduces bit for bit.
 *
 * Formats: MTTS_PCM16 (s16le, 2 bytes per sample), MTTS_ULAW, MTTS_ALAW (ITU-T G.711, 1 byte per sample).
 *
 * mtts_pcm_encode: d_audio [B][ld] fp32, rows as everywhere else (ld % 4 == 0, 16-byte aligned); d_lengths device int64 [B],
 * samples; d_formats device int32 [B]; d_keys device int64 [B] or NULL (all 0); d_out uint8 [B][2 * ld], one stride for every
 * row (a G.711 row uses the front half), 16-byte aligned; d_out_bytes device int64 [B] = len_b * bytes per sample.
 *   q:      y = x * 32768 in fp32 (exact: a power of two); with dither on a PCM16 row y = y + d, one fp32 add;
 *           q = rint(y), ties to even, clamped to [-32768, 32767]; NaN gives 0.  32768 is the inverse of the / 32768 of
 *           mtts_pcm_decode and of every reader of this project: decode then encode returns each of the 65536 words unchanged.
 *   PCM16:  the two bytes of q, low byte first.
 *   G.711:  companding of the UNDITHERED q (dither touches PCM16 rows only), in integer operations, as CPython's
 *           audioop.lin2ulaw / lin2alaw(.., 2) computes it.  With seg(v, e0) = the number of i in [0, 8) with v > (e0 << i) - 1:
 *           mu-law: v = q >> 2 (arithmetic); mask = 0x7F and v = -v when v < 0, else mask = 0xFF; v = min(v, 8159) + 33;
 *                   s = seg(v, 0x40); byte = (s == 8 ? 0x7F : (s << 4) | ((v >> (s + 1)) & 15)) ^ mask;
 *           A-law:  v = q >> 3; mask = 0x55 and v = -v - 1 when v < 0, else mask = 0xD5; s = seg(v, 0x20);
 *                   byte = (s == 8 ? 0x7F : (s << 4) | ((v >> (s < 2 ? 1 : s)) & 15)) ^ mask.
 *   dither: TPDF of one LSB: d = u1 - u2, u_k = (h_k >> 8) * 2^-24, the difference exact in fp32.  h_k is a 32-bit counter-based
 *           hash of (seed, d_keys[b], the sample's index i within its row, the stream k - 1 in {0, 1}) and of nothing else -- not of
 *           the row index, the grid or the batch -- in uint32 arithmetic, a chain of murmur3 finalisers
 *               fmix(h): h ^= h >> 16; h *= 0x85EBCA6B; h ^= h >> 13; h *= 0xC2B2AE35; h ^= h >> 16
 *               h = fmix(0x9E3779B9 ^ seed_lo); h = fmix(h ^ seed_hi); h = fmix(h ^ key_lo); h = fmix(h ^ key_hi);
 *               h_k = fmix(h ^ (2 * i + (k - 1)))        (lo / hi: the low and high 32 bits of the int64; i < 2^30)
 *           so a row's bytes do not depend on the batch it is in, and two calls give the same bits.
 *   tails:  bytes at or beyond d_out_bytes[b] are never written: whole groups of 4 samples are stored as 8 (PCM16) or 4 (G.711)
 *           bytes, the last partial group of a row sample by sample.  Nothing outside [0, len_b) of a row is read.
 *   refusals: a length outside [0, ld] or a format that is none of the three gives d_out_bytes[b] = -1 and no byte written for
 *           that row; the other rows are unaffected.  A length that already is -1 (a row refused by mtts_waveform_finish or
 *           mtts_resample_forward) therefore stays -1.
 *
 * mtts_pcm_decode: the inverse.  d_data uint8 [B][ld_bytes] (ld_bytes % 16 == 0, 16-byte aligned), d_lengths in samples,
 * d_formats as above -> d_out fp32 [B][ld] (ld % 4 == 0), d_out_lengths int64 [B] = len_b.  PCM16: q / 32768.  G.711: the G.711
 * linear value / 32768, with c = ~byte for mu-law: t = (((c & 15) << 3) + 132) << ((c >> 4) & 7), value = c & 0x80 ? 132 - t :
 * t - 132; with c = byte ^ 0x55 for A-law: s = (c >> 4) & 7, t = (c & 15) << 4, t = s == 0 ? t + 8 : (t + 0x108) << (s - 1),
 * value = c & 0x80 ? t : -t (audioop.ulaw2lin / alaw2lin(.., 2)).  Both quotients are exact.  Samples at or beyond len_b are
 * written as zeros up to ld, as the mel front end expects of a padded row.  A length outside [0, ld], one whose bytes exceed
 * ld_bytes, or an unknown format gives d_out_lengths[b] = -1 and leaves the row unwritten.
 *
 * Both: stream-ordered, no allocation, no synchronisation, no workspace.  What the host can see returns -1 (mtts_last_error):
 * null pointers, B < 1, a bad ld, a misaligned buffer, d_out overlapping the input.  mtts_pcm_status(d_verdict, B, stream) --
 * the one entry here that waits for the stream -- reads d_out_bytes or d_out_lengths of a call and names the first refused row
 * through mtts_last_error.  mtts_codec_tile = MTTS_CODEC_TILE as built. */
#define MTTS_PCM16 0
#define MTTS_ULAW 1
#define MTTS_ALAW 2
#define MTTS_CODEC_TILE 2048           /* samples per workgroup */
int mtts_codec_tile(void);
int mtts_pcm_encode(const float* d_audio, int64_t ld, const int64_t* d_lengths, const int32_t* d_formats, const int64_t* d_keys,
                    int B, int dither, int64_t seed, uint8_t* d_out, int64_t* d_out_bytes, void* stream);
int mtts_pcm_decode(const uint8_t* d_data, int64_t ld_bytes, const int64_t* d_lengths, const int32_t* d_formats, int B,
                    float* d_out, int64_t ld, int64_t* d_out_lengths, void* stream);
int mtts_pcm_status(const int64_t* d_verdict, int B, void* stream);

/* ---------------------------------------------------------------- FLAC out: lossless compressed audio, encoded on the device */

/* A row becomes one complete mono, 16-bit, fixed-blocksize FLAC stream (RFC 9639): the compressed form of the "pcm" bytes above, about
 * 0.7 of their size on speech.  The encoder is deterministic: every byte is a function of the row's samples, its rate, the block size
 * and (seed, key), and of nothing else -- not of the batch, the row index or the grid.  tests/flac_restated.py restates it in NumPy bit
 * for bit, beside an independent decoder.  mtts_flac_encode_lpc also writes LPC subframes (the lpc paragraphs below, restated in
 * tests/flac_lpc_restated.py): about 0.56 of the "pcm" bytes on speech at order 12.  Out of scope: writing stereo, the MD5 signature,
 * seek tables ("FLAC in" below reads them), a search over Rice partition orders, 24-bit output.
 *
 *   samples:  q[i] is exactly the PCM16 word mtts_pcm_encode writes for the row: the same arithmetic, the same dither as a function of
 *             (seed, key, i) when dither is on (the same device functions, csrc/pcm_quantise.h).
 *   header:   42 bytes.  "fLaC"; 80 00 00 22 (last metadata block, STREAMINFO, 34 bytes); then, big-endian and bit-packed: min = max
 *             block size bs (16 bits each); min and max frame size in bytes over the row's frames (24 bits each; 0 for an empty row);
 *             sample rate (20); channels - 1 = 0 (3); bits per sample - 1 = 15 (5); total samples (36); MD5 = 16 zero bytes, which the
 *             format reads as "not computed".  A row of length 0 is these 42 bytes alone.
 *   frames:   bs is one of 256, 512, 1024, 2048, 4096.  Frame f holds the samples [f * bs, min((f + 1) * bs, len)); n is its count.
 *   frame header: FF F8 (sync, fixed block size).  Block-size code (4 bits): 1000..1100 for 256..4096 when n == bs; else 0110 and an 8-bit
 *             n - 1 when n <= 256; else 0111 and a 16-bit n - 1.  Rate code (4 bits), first match: 0001..1011 for 88200, 176400, 192000,
 *             8000, 16000, 22050, 24000, 32000, 44100, 48000, 96000; 1101 and 16-bit Hz when the rate <= 65535; 1110 and 16-bit tens of
 *             Hz when the rate is a multiple of 10 and rate / 10 <= 65535; else 0000 (as STREAMINFO says).  Channel assignment 0000,
 *             sample-size code 100, a reserved 0 bit.  The frame number in the RFC's UTF-8-like coding, 1 to 4 bytes.  The block-size
 *             tail, the rate tail.  CRC-8 of the header so far (polynomial 0x07, initial value 0).
 *   subframe: one.  Its header byte: a 0 bit, a 6-bit type, a wasted-bits flag of 0.
 *             CONSTANT (000000, the value in 16 bits) when all n samples are equal.
 *             Otherwise FIXED of order o (001ooo): o is the order in 0..4 with the smallest sum over i in [4, n) of |e_o[i]|, e_o the
 *             o-th difference of q, ties to the lower order (so o = 0 when n <= 4).  Body: o warm-up samples of 16 bits, then the
 *             residual: method 00 (4-bit parameters); a 4-bit partition order log2(bs / 256) when n == bs, else 0 -- a full frame has
 *             partitions of 256 samples, the first holding 256 - o residuals; a short last frame is one partition.  Per partition a 4-bit
 *             k, then the codes: k in 0..14 minimises cnt * (k + 1) + sum(u >> k), ties to the smaller k (15, the escape, is never used);
 *             u = 2 r for r >= 0, -2 r - 1 otherwise; a code is u >> k zero bits, a one bit, the low k bits of u, MSB first.
 *             VERBATIM (000001, n samples of 16 bits) when the FIXED subframe, its header byte included, has >= 8 + 16 n bits: every
 *             frame is therefore at most 2 * bs + 16 bytes.
 *   close:    zero bits to the byte boundary, then CRC-16 of the whole frame (polynomial 0x8005, initial value 0), big-endian.
 *   ranges:   |e_4| <= 2^19 and u <= 2^20, so a cost over 4095 samples reaches 2^32: the order costs and sum(u >> k) are 64-bit sums
 *             (32 bits inside a partition of 256, where they stay below 2^29).
 *
 * With max_lpc_order = M in 1..12 (mtts_flac_encode_lpc) a frame that is not CONSTANT also tries LPC subframes.  Every step is exact
 * in integers or one fp64 operation order (+ - * / as written, no contraction; the device's fp64 division is correctly rounded):
 *   lpc orders:   the list 4, 8, 12, each capped at M (min(o, M)), once each, ascending, and only orders < n.  M = 1 tries {1}, M = 8
 *             {4, 8}, M = 12 {4, 8, 12}.  No such order (n = 1): the frame is as mtts_flac_encode writes it.
 *   lpc window:   w[i] = 255 - (255 * (2 i + 1 - n)^2) / (n * n), integer division, over the frame's own n: 1..255, and the product
 *             stays below 2^32.  x[i] = q[i] * w[i], |x| < 2^23.
 *   lpc autocorrelation: R[l] = sum over i in [0, n - l) of x[i] * x[i + l] for l = 0..top (the largest order tried), exact in int64 (a
 *             product below 2^46, 4096 of them below 2^58); each R[l] converted to fp64 once.
 *   lpc recursion: Levinson-Durbin in fp64.  err = R[0]; not (0 < err < inf): no order is tried.  For m = 1..top: s = R[m]; for j = 1..
 *             m - 1 in that order s = s - a[j] * R[m - j]; k = s / err; a'[j] = a[j] - k * a[m - j] for j < m, a'[m] = k; err = err *
 *             (1.0 - k * k).  The recursion stops at the first m whose err is not in (0, inf): that order and those above are not tried.
 *   lpc quantisation: precision 12.  e = the biased exponent field of max_j |a[j]|, - 1022 (so max|a| < 2^e; zero and subnormals give a
 *             large shift, an infinity or NaN a negative one); shift = min(15, 11 - e); a negative shift drops the order.  c[j - 1] =
 *             clamp(rint(a[j] * 2^shift), -2048, 2047), ties to even.
 *   lpc residual: r[i] = q[i] - ((sum over j in [0, m) of c[j] * q[i - 1 - j]) >> shift) for i >= m, an arithmetic shift; 12 taps of 12
 *             bits on 16-bit words keep the sum below 12 * 2^11 * 2^15 < 2^31.  An order with any |r[i]| >= 2^20 is dropped, so the
 *             ranges above hold unchanged (u < 2^21).
 *   lpc subframe: type 1ooooo (m - 1); m warm-up words of 16 bits; a 4-bit precision - 1 = 1011; a 5-bit shift; m coefficients of 12 bits,
 *             two's complement; then the residual exactly as FIXED writes it with m in place of o (method 00, the same partition order,
 *             the first partition holding 256 - m residuals, k by the same cost and tie rule).
 *   lpc choice:   exact subframe bits, header and coefficients included: the fewest win, ties go to FIXED, then to the lower order.
 *             VERBATIM when the winner has >= 8 + 16 n bits, as before: a frame is still at most 2 * bs + 16 bytes, never longer than
 *             the frame mtts_flac_encode writes of the same samples, and the two size queries serve both entries.
 *   lpc subset:   orders up to 12, Rice partitions of 256 and blocks up to 4096 keep every subframe inside the limits of the RFC's streamable
 *             subset at every rate (LPC order <= 12 up to 48 kHz, Rice partition order <= 8, blocks <= 4608 up to 48 kHz); a stream
 *             leaves the subset only where it does without LPC, through rate code 0000.
 *   M = 0 is mtts_flac_encode: the same launches, the same bytes.  An M outside 0..12 is a host-visible refusal.  Everything else --
 *   arguments, sizes, refusals, three launches, determinism -- is as for mtts_flac_encode, which keeps its kernels and its bytes.
 *
 * mtts_flac_encode: d_audio [B][ld] fp32 (ld % 4 == 0, 16-byte aligned), d_lengths device int64 [B], d_rates device int32 [B] (Hz),
 * d_keys device int64 [B] or NULL (all 0), dither / seed as mtts_pcm_encode takes them -> d_out uint8 [B][out_ld], row b holding
 * d_out_bytes[b] bytes from its start.  out_ld >= mtts_flac_row_bytes(ld, block_size) = 42 + ceil(ld / bs) * (2 * bs + 16) rounded up to
 * 16, and a multiple of 16.  d_ws: mtts_flac_workspace_bytes(B, ld, block_size) bytes, 16-byte aligned: a fixed-stride staging slot and
 * a byte count per frame; every word read from it was written by the same call.  Three launches (frame encode, row layout, compaction);
 * every output byte is written once and nothing at or beyond d_out_bytes[b] is written.  Stream-ordered, no allocation, no
 * synchronisation.
 *   refusals: a length outside [0, ld] (one that already is -1 included), a rate outside [1, 1048575] or a row of more than 2^21 frames
 *             gives d_out_bytes[b] = -1 and no byte written for that row; the other rows are unaffected.  mtts_pcm_status reads the
 *             verdict as it does for the PCM entries.
 * What the host can see returns -1 (mtts_last_error; the two size queries too): null pointers (d_keys excepted), B < 1, a bad ld, a
 * block_size that is none of the five, a max_lpc_order outside 0..12, a small out_ld or ws_bytes, a misaligned buffer, d_out / d_ws / d_audio overlapping. */
#define MTTS_FLAC 3
int64_t mtts_flac_row_bytes(int64_t ld, int block_size);
int64_t mtts_flac_workspace_bytes(int B, int64_t ld, int block_size);
int mtts_flac_encode(const float* d_audio, int64_t ld, const int64_t* d_lengths, const int32_t* d_rates, const int64_t* d_keys, int B,
                     int block_size, int dither, int64_t seed, uint8_t* d_out, int64_t out_ld, int64_t* d_out_bytes, void* d_ws,
                     int64_t ws_bytes, void* stream);
int mtts_flac_encode_lpc(const float* d_audio, int64_t ld, const int64_t* d_lengths, const int32_t* d_rates, const int64_t* d_keys, int B,
                         int block_size, int max_lpc_order, int dither, int64_t seed, uint8_t* d_out, int64_t out_ld, int64_t* d_out_bytes,
                         void* d_ws, int64_t ws_bytes, void* stream);

/* ---------------------------------------------------------------- FLAC in: recordings decoded on the device */

/* A ragged batch of whole native FLAC streams (RFC 9639) becomes fp32 rows: channel 0 of each stream, integers to the bit.  The frame
 * decoder is general -- LPC, stereo decorrelation, 8 to 24 bits, metadata, any block size up to 4608 -- so files written by other
 * encoders are read, not only the streams of mtts_flac_encode.  A row's samples depend on its bytes alone, not on the batch, the row
 * index or the strides; the verdict is per row and nothing waits for the host.  tests/flac_in_restated.py restates the rules below
 * in Python beside a stream writer; csrc/flac_parse.h is the parser, compiled for the host and for the device.
 *
 *   input:    d_data uint8 [B][ld_bytes] (ld_bytes % 16 == 0, 16-byte aligned); row b is one stream of d_nbytes[b] bytes (device int64).
 *             An nbytes outside [0, ld_bytes] refuses the row.
 *   metadata: "fLaC"; then metadata blocks, each a byte (last flag, 7-bit type) and a 24-bit length.  The first block is STREAMINFO
 *             (type 0, 34 bytes) and no later block is; type 127, a block that runs off the row and a chain without a last block are
 *             refused.  Every other block is skipped by its length, whatever it holds.  STREAMINFO must name: 8..24 bits per sample,
 *             a rate >= 1, 16 <= min block size <= max block size <= max_block (1..8 channels follow from its 3 bits).
 *   candidate: a byte position is a candidate when it holds a frame header: sync FF F8 / FF F9 (the low bit: variable blocking); block-
 *             size code != 0000 (0001: 192; 0010..0101: 576 << (code - 2); 0110 / 0111: an 8- / 16-bit tail + 1; 1000..1111: 1 << code);
 *             rate code != 1111 (0000: STREAMINFO's; 0001..1011 the eleven fixed rates; 1100: 8-bit kHz; 1101: 16-bit Hz; 1110: 16-bit
 *             tens of Hz); channel assignment 0..7 (that many + 1 independent channels), 8 left/side, 9 side/right, 10 mid/side;
 *             sample-size code != 011 (000: STREAMINFO's; 8, 12, -, 16, 20, 24, 32 bits); a reserved 0 bit; the coded number, UTF-8-like,
 *             1 to 7 bytes (up to 36 bits; over-long forms are taken as they are); the block-size tail; the rate tail; the CRC-8
 *             (polynomial 0x07) of the header so far.  And the header agrees with STREAMINFO: the same rate, the same bits per sample,
 *             the same channel count, a block size <= STREAMINFO's maximum.  A header is at most 16 bytes.
 *   subframe: a 0 bit; 6-bit type; wasted-bits flag, and when set a unary count w: wasted = w + 1 < the subframe's bits.  The subframe's
 *             bits are the frame's, + 1 for a side channel, - wasted.  Types: 000000 CONSTANT; 000001 VERBATIM; 001000..001100 FIXED of
 *             order 0..4; 1ooooo LPC of order ooooo + 1 (1..32); every other type is refused, and an order above the block size.
 *             LPC: a 4-bit precision - 1 (1111 is refused), a 5-bit shift (two's complement; negative is refused), the coefficients.
 *             Residual: 2-bit method (00: 4-bit Rice parameters, 01: 5-bit; 1x refused); 4-bit partition order po: 2^po must divide
 *             the block and block >> po must be >= the predictor order (equal: the first partition is empty).  Per partition the
 *             parameter k, or all ones: the escape, a 5-bit width 0..31 and raw two's-complement residuals.  A Rice code is q zero
 *             bits, a one, k bits: u = q << k | low must stay below 2^32 - 1 (a residual is inside (-2^31, 2^31)); r = u >> 1 for even
 *             u, -(u >> 1) - 1 for odd.  Restore: x[i] = r[i] + prediction, the FIXED polynomials or (sum_j c[j] x[i-1-j]) >> shift with
 *             the sum in 64 bits (25-bit samples, 15-bit coefficients and 32 taps need 45) and an arithmetic shift; the sample is the
 *             low 32 bits.  Then x << wasted.
 *   frame:    a candidate is a frame when its subframes (one per channel) parse inside the row, zero to seven padding bits (not looked
 *             at) reach a byte boundary, and the next two bytes are the CRC-16 (polynomial 0x8005) of everything before them.  Channel
 *             0 of its samples: the first channel (independent, left/side); side + right; or (((mid << 1) | (side & 1)) + side) >> 1.
 *             Each must lie in [-2^(bps-1), 2^(bps-1)).  Channels 2..8 are parsed for their length only.
 *   row:      accepted when, starting at the first byte behind the metadata, frames follow one another end to start up to exactly
 *             d_nbytes[b]; all carry the blocking bit of the first; the coded numbers are consecutive from 0 -- frame numbers when the
 *             bit is 0, and when it is 1 sample numbers that each equal the sum of the block sizes before; with bit 0 every frame has
 *             the first frame's block size but the last, which may be shorter; and the sample total equals STREAMINFO's and is <= ld.
 *             Candidates off that walk are ignored (a sync pattern in a PADDING block, a whole valid frame inside a VERBATIM payload).
 *             STREAMINFO's total 0 with no frame is an empty clip of length 0; total 0 with frames (unknown length) is refused.
 *   output:   d_out fp32 [B][ld] (ld % 4 == 0, 16-byte aligned): sample q as q / 2^(bps-1), exact in fp32; zeros from the length up to
 *             ld; d_out_lengths[b] the sample count; d_out_rates[b] STREAMINFO's rate.
 *   refusals: everything else -- a CRC mismatch, a truncated or missing frame, a unary run or raw read that would pass the end of the
 *             row (the reader returns zeros there and the row is refused), a residual outside 32 bits, more than ld / 16 + 64
 *             candidates or 2 * ld + max_block staged samples in a row -- gives d_out_lengths[b] = -1 and d_out_rates[b] = 0; no word
 *             of that row of d_out is written and the other rows are unaffected.  mtts_pcm_status reads the verdict as it does for
 *             the PCM entries.
 * Out of scope: the MD5 signature is not checked (the hash is serial per stream, and the project's own streams carry none), seek
 * tables are not used, and Ogg FLAC, an ID3 prefix, 32-bit samples and blocks above 4608 samples are not read.
 *
 * mtts_flac_decode: six launches (metadata, candidate scan, plan, frame decode, walk, gather) on d_ws of
 * mtts_flac_decode_workspace_bytes(B, ld_bytes, ld, max_block) bytes, 16-byte aligned; every word read from it was written by the same
 * call.  Stream-ordered, no allocation, no synchronisation.  What the host can see returns -1 (mtts_last_error; the size query too):
 * null pointers, B < 1, B > 65535, an ld_bytes that is no positive multiple of 16, an ld that is no positive multiple of 4, a max_block
 * outside [16, 4608], a small workspace, a misaligned buffer, d_data / d_out / d_ws overlapping.
 *
 * mtts_flac_parse_host: the same parser and the same acceptance walk over HOST memory, one stream: channel 0's integers to
 * out[0, out_capacity), the sample count or -1 returned, *rate / *channels / *bps from STREAMINFO (0 when refused).  It never touches
 * the GPU: the parser is proven on the host before a kernel runs it. */
int64_t mtts_flac_decode_workspace_bytes(int B, int64_t ld_bytes, int64_t ld, int max_block);
int mtts_flac_decode(const uint8_t* d_data, int64_t ld_bytes, const int64_t* d_nbytes, int B, int max_block, float* d_out, int64_t ld,
                     int64_t* d_out_lengths, int32_t* d_out_rates, void* d_ws, int64_t ws_bytes, void* stream);
int64_t mtts_flac_parse_host(const uint8_t* data, int64_t nbytes, int max_block, int32_t* out, int64_t out_capacity, int* rate,
                             int* channels, int* bps);

/* ---------------------------------------------------------------- loudness: BS.1770 K-weighted, gated LUFS, one gain per row */

/* How loud a row is, and the gain that brings it to a target: integrated loudness as in ITU-R BS.1770-4 / EBU R 128 for a ragged
 * batch of mono rows, measured and (with `apply`) corrected in place.  The reference has no counterpart (its to_waveform only
 * scales a row whose peak exceeds 1); the arithmetic below is the definition, and tests/loudness_restated.py restates it in NumPy
 * fp64 in plain sample order.  Rows as for the other waveform entries: fp32 [B][ld], ld % 4 == 0, 16-byte aligned; d_lengths device
 * int64 [B], checked on the device without a host read; nothing outside [0, len_b) of a row is read or written.
 *
 * Coefficients (host, fp64, any sample_rate fs with fs % 100 == 0 in [8000, 192000]; mtts_loudness_coefficients returns the ten
 * words b0 b1 b2 a1 a2 of the shelf, then of the high-pass): the bilinear transform of the analog prototype,
 *   shelf:     f0 = 1681.974450955533, G = 3.999843853973347, Q = 0.7071752369554196, K = tan(pi f0 / fs), Vh = 10^(G / 20),
 *              Vb = Vh^0.4996667741545416, a0 = 1 + K / Q + K K;
 *              b = [(Vh + Vb K / Q + K K) / a0, 2 (K K - Vh) / a0, (Vh - Vb K / Q + K K) / a0], a = [1, 2 (K K - 1) / a0, (1 - K / Q + K K) / a0]
 *   high-pass: f0 = 38.13547087602444, Q = 0.5003270373238773, the same K and a0; b = [1, -2, 1], a as above.
 * At 48 kHz these are the table values of BS.1770 to 1e-14.  At other rates the response is that of the bilinear coefficients: a
 * full-scale 997 Hz sine reads -3.0103 LUFS at 48 kHz, -2.984 at 24 kHz and -2.996 at 8 kHz.
 *
 * The cascade, per sample x (fp32, converted exactly), transposed direct form II in fp64, every operation rounded once (no FMA):
 *   y = b0 x + s1;  s1 = (b1 x - a1 y) + s2;  s2 = b2 x - a2 y          (shelf)
 *   z = c0 y + t1;  t1 = (c1 y - d1 z) + t2;  t2 = c2 y - d2 z          (high-pass), all four state words 0 ahead of sample 0.
 * The recurrence is cut in time.  chunk = mtts_loudness_chunk(fs) = the largest divisor of fs / 100 that is at most 256 (240 at 24
 * and 48 kHz, 80 at 8 kHz), so chunk edges fall on 10 ms edges.  Pass 1 runs every chunk from zero state and keeps its end state
 * z_c; pass 2 carries s_{c+1} = M s_c + z_c along the row, M = A^chunk the 4 x 4 transition matrix of `chunk` samples of silence,
 * built on the host in fp64 by running the cascade from the four unit states, each row of M s evaluated as
 * ((M0 s0 + M1 s1) + M2 s2) + M3 s3, then + z; pass 3 reruns every chunk from its true entry state s_c.  Pass 2 is a two-level
 * scan with R = MTTS_LOUDNESS_SCAN_RUN and P = M^R (built the same way over R * chunk samples): run r holds the chunks
 * [R r, R r + R); w_r = the fold w = M w + z_c over the run from w = 0 (a chunk beyond the row's end counts as z = 0);
 * S_0 = 0, S_{r+1} = P S_r + w_r in run order; chunk c of run r is entered with s, which starts at S_r and then becomes M s + z_c.  This equals the plain
 * recurrence up to the rounding of M s (2e-13 absolute on a signal of rms 0.09; an fp32 recurrence is off by 1.4e-5: hence fp64).
 * Sums: e_c = the sum of z z over the chunk's samples inside the row, in sample order from 0.0; a 100 ms segment (fs / 10 samples) is
 * the sum of its chunks in index order from 0.0; block j = ((seg_j + seg_j+1) + seg_j+2) + seg_j+3, taken at every whole segment
 * j <= nfull - 4, nfull = len_b / (fs / 10): 400 ms at 75 % overlap; a partial trailing segment belongs to no block.
 *   ms_j = block_j / (4 fs / 10);  l_j = -0.691 + 10 log10(ms_j)
 *   absolute gate: keep l_j > -70;  relative gate G = -0.691 + 10 log10(mean of the kept ms_j) - 10
 *   L = -0.691 + 10 log10(mean of the ms_j with l_j > -70 and l_j > G);  L = -inf when no block survives.
 *   A mean is (sum, count) over the blocks: thread t of 256 adds its blocks j = t, t + 256, ... in ascending order from 0.0, then
 *   v[t] = v[t] + v[t + o] for o = 128, 64, .. 1.
 *   DEVIATION from BS.1770: a row shorter than one block (nfull < 4; a TTS answer like "Yes." must still be levelled) is a single
 *   block of its own length: ms = (the sum of its chunks' e_c in index order) / len_b, L = l when l > -70, else -inf.
 * Peak: the SAMPLE peak max |x| over [0, len_b) (NaN samples are passed over).  True peak (oversampled) and loudness range:
 * mtts_loudness_r128 below.
 * Gain (d_target fp32 [B] in LUFS; NaN, or a NULL d_target, means measure only):
 *   g = (float)pow(10, ((double)target - L) / 20);  when peak * g > peak_ceiling in fp32, g = peak_ceiling / peak (one fp32 division),
 *   lowered by one unit in the last place while peak * g still exceeds the ceiling, so that no output sample does: the ceiling acts on
 *   the sample peak.  g = 1 exactly when L is not finite, the target is NaN, the row is empty or g is not finite.
 * Apply (apply != 0): x = x * g, one fp32 multiply, on the samples [0, len_b) of the rows with g != 1; rows with g == 1 keep their
 * bits and no sample at or beyond len_b is written.
 * Outputs: d_lufs double [B] = L as measured BEFORE the gain, d_gain fp32 [B], d_peak fp32 [B] (before the gain).
 * Every order above is a function of the row's length and fs alone: a row's L, g and samples are bit-identical whether it runs
 * alone or in a batch, in any ld, and two calls give the same bits.
 * Refusals (the ragged-batch contract): a length outside [0, ld] refuses that row -- d_lufs NaN, d_gain 1, d_peak 0, no sample
 * read or written -- and the other rows are unaffected; d_lengths is not written, so a length that already is -1 (a row refused
 * upstream) stays -1 for the stages behind.  mtts_loudness_status(d_ws, stream) -- the one entry here that waits for the stream --
 * names the first refused row of the latest call on that workspace through mtts_last_error.  Header words (int64): first refused
 * row + 1 or 0, its length (saturated to 32 bits), ld.
 * Launches: (tile, row) zero-state chunks, one wave per row for the scan, (tile, row) energies, one workgroup per row for the
 * gates, (tile, row) apply; a workgroup of the chunk passes holds MTTS_LOUDNESS_CHUNKS chunks, one per lane, its samples staged
 * through LDS in slabs.  mtts_loudness_tile() = MTTS_LOUDNESS_TILE = the samples per such workgroup at 24 and 48 kHz (256 chunks of
 * 240); at another rate it is MTTS_LOUDNESS_CHUNKS * mtts_loudness_chunk(fs).  Stream-ordered, no allocation, no synchronisation;
 * one workspace of mtts_loudness_workspace_bytes(ld, B, sample_rate).  What the host can see returns -1 and launches nothing: null
 * pointers, B outside [1, 65535], an ld that is no positive multiple of 4 or above 2^30, a bad rate, a misaligned d_audio / d_ws /
 * d_lufs, a peak_ceiling that is not positive and finite, a small workspace. */
#define MTTS_LOUDNESS_CHUNKS 256       /* chunks (= lanes) per workgroup of the chunk passes */
#define MTTS_LOUDNESS_TILE 61440       /* samples per workgroup at 24 / 48 kHz */
#define MTTS_LOUDNESS_SCAN_RUN 32      /* consecutive chunks a lane of the scan pass owns */
int mtts_loudness_chunk(int sample_rate);
int mtts_loudness_tile(void);
int mtts_loudness_coefficients(int sample_rate, double* h_out);
int64_t mtts_loudness_workspace_bytes(int64_t ld, int B, int sample_rate);
int mtts_loudness(float* d_audio, int64_t ld, const int64_t* d_lengths, int B, int sample_rate, const float* d_target,
                  float peak_ceiling, int apply, double* d_lufs, float* d_gain, float* d_peak, void* d_ws, int64_t ws_bytes,
                  void* stream);
int mtts_loudness_status(const void* d_ws, void* stream);

/* mtts_loudness_r128: mtts_loudness, and with it the true peak, the loudness range, the maximum momentary and the maximum short-term
 * loudness of every row (EBU R 128 / Tech 3341 / Tech 3342), and a second ceiling on the gain, on the true peak.  d_lufs, d_peak and
 * -- with no true-peak ceiling -- d_gain and the samples are bit for bit those of mtts_loudness on the same rows; tests/r128_restated.py
 * restates what is new.
 *
 * True peak.  The row is read at F times its rate: F = 8 for fs < 48000, 4 for 48000 <= fs < 96000, 2 for fs >= 96000.  The
 * interpolator is a Hann-windowed sinc of half-width 6 input samples, MTTS_TRUE_PEAK_TAPS = 12 taps per phase, the class of filter
 * of BS.1770-4 Annex 2: for phase p in [1, F) and tap k in [0, 12)
 *   d = (k - 5) - p / F;  w[p][k] = sin(pi d) / (pi d) * 0.5 (1 + cos(pi d / 6));  h[p][k] = (float)(w[p][k] / sum_k w[p][k])
 * built on the host in fp64 (the sum in ascending k from 0.0) and rounded once to fp32, so every phase reads DC exactly.  Phase 0 is the
 * sample itself and is not filtered.  mtts_true_peak_filter(fs, h_out, F_out) -- host only, no device needed -- writes F and the F * 12
 * words h[p][k] (row 0: the unit impulse at tap 5).  The value at j + p / F, for every j in [0, len_b), is
 *   v = sum_k h[p][k] x[j - 5 + k]     x = 0 outside [0, len_b); fp32; each product rounded, then added in ascending k from 0.0f
 * and true_peak_b = the maximum over |x[j]| and every |v|, taken with fmaxf: NaN samples and NaN sums are passed over, as for the
 * sample peak.  A maximum has no order, so a row's true peak does not depend on B, ld, the grid or the tile.  Known error of the
 * estimator (profiles/r21_r128.md): on a steady sine anywhere up to 0.45 fs the 12-tap reading lies between 0.15 dB under and 0.07 dB
 * over that of a 129-tap interpolation (the sample peak alone: up to 3.01 dB under); a sine that starts or stops inside the row reads
 * up to 0.1 dB over its amplitude at that edge, where the taps see the step.
 *
 * Maximum momentary loudness: the maximum of l_j over the 400 ms blocks above, ungated; the single block's l for a row under
 * 400 ms (the deviation above); -inf for an empty row.
 * Short-term blocks (3 s): S_k = seg_k + seg_k+1 + ... + seg_k+29 in ascending index from 0.0, at every whole segment k <= nfull - 30
 * (a 100 ms hop); ms_k = S_k / (30 fs / 10).  Maximum short-term loudness: the maximum of -0.691 + 10 log10(ms_k); -inf when nfull < 30.
 * Loudness range (EBU Tech 3342): keep the blocks with l_k > -70; the relative gate is -0.691 + 10 log10(mean of the kept ms_k) - 20,
 * the mean as (sum, count) in the reduction shape of the integrated gate; of the n blocks above both gates in ascending order of ms,
 *   lo = the element at index (10 (n - 1) + 50) / 100,  hi = the element at index (95 (n - 1) + 50) / 100   (integer division)
 *   lra = (-0.691 + 10 log10(hi)) - (-0.691 + 10 log10(lo));  lra = 0 when n == 0 or nfull < 30.
 * The two order statistics are exact (a radix select on the bit patterns of the non-negative doubles, no tolerance) and depend on
 * nothing but the row.
 *
 * Gain: the rule above (target, then the sample-peak ceiling), and then, with c_tp = (float)pow(10, true_peak_ceiling_db / 20): when
 * true_peak * g > c_tp in fp32, g = c_tp / true_peak, lowered by one unit in the last place up to 4 times while the product still
 * exceeds c_tp.  true_peak_ceiling_db is in dBTP, finite and <= 0; NaN means none, and g is then that of mtts_loudness bit for bit.
 * The ceiling acts only on rows that have a target: a row without one, an empty row and a row whose L is not finite keep g == 1
 * and their bits.
 * Outputs beyond those of mtts_loudness: d_true_peak fp32 [B] (linear, before the gain), d_lra, d_momentary_max, d_short_term_max
 * double [B].  A refused row gives NaN for the four loudness figures, 0 for both peaks and gain 1.  The same refusals and the same
 * verdict header, read by mtts_loudness_status.  Launches: the chunk, scan and energy kernels of mtts_loudness, the (tile, row)
 * true-peak pass (MTTS_TRUE_PEAK_TILE samples and a halo of 5 + 6 per workgroup, one float out), one workgroup per row for the gates
 * and the selection, the apply pass.  One workspace of mtts_loudness_r128_workspace_bytes(ld, B, sample_rate). */
#define MTTS_TRUE_PEAK_TILE 4096       /* samples per workgroup of the true-peak pass */
#define MTTS_TRUE_PEAK_TAPS 12         /* taps per phase of the interpolator */
int mtts_true_peak_tile(void);
int mtts_true_peak_filter(int sample_rate, float* h_out, int* F_out);
int64_t mtts_loudness_r128_workspace_bytes(int64_t ld, int B, int sample_rate);
int mtts_loudness_r128(float* d_audio, int64_t ld, const int64_t* d_lengths, int B, int sample_rate, const float* d_target,
                       float peak_ceiling, float true_peak_ceiling_db, int apply, double* d_lufs, float* d_gain, float* d_peak,
                       float* d_true_peak, double* d_lra, double* d_momentary_max, double* d_short_term_max, void* d_ws,
                       int64_t ws_bytes, void* stream);

/* ---------------------------------------------------------------- forced alignment (Monotonic Alignment Search) */

/* Which fine mel frames belong to which token -- the alignment of the reference's training forward, matcha/models/matcha_tts.py:
 * 184-201 (log_prior of the text encoder's mu_x against the ground-truth mel at hop 128, in fp32 on purpose :90-101, then
 * maximum_path; Kim et al. 2020, Glow-TTS, algorithm 1).  Ragged: utterance b has d_x_lengths[b] <= Tx tokens and
 * d_y_lengths[b] <= Tm frames (device int64 [B]); Tx <= 1024, Tm >= Tx.
 *
 * mtts_mas_logprior: d_lp[b][x][y] = -0.5 |y[b,:,y]|^2 + <mu_x[b,:,x], y[b,:,y]> - 0.5 |mu_x[b,:,x]|^2, the diagonal-Gaussian
 *   log-likelihood without its constant (reference matcha_tts.py:184-195), evaluated as -0.5 sum_f (y - mu)^2 in fp32; d_mu_x
 *   [B][F][Tx], d_y [B][F][Tm] (the normalised mel), d_lp [B][Tx][Tm] (the reference's layout), zero beyond an utterance's lengths.
 * mtts_mas: the search.  d_lp [B][Tx][Tm], or NULL to compute it from d_mu_x / d_y (never written to memory in this layout).
 *   v[0][0] = lp[0][0], v[x][y] = lp[x][y] + max(v[x][y-1], v[x-1][y-1]) inside the band max(0, Tx_b - (Tm_b - y)) <= x <=
 *   min(y, Tx_b - 1), -1e9 outside; walking back from (Tx_b - 1, Tm_b - 1), at frame y on token x the path steps to x - 1 iff
 *   x > 0 and (x == y or v[x-1][y-1] > v[x][y-1]): ties stay on the token.  One add and one compare per cell, in frame order:
 *   the outputs equal a NumPy fp32 restatement bit for bit.
 *   d_durations [B][Tx] int32: frames on each token (>= 1 on valid tokens, 0 beyond, summing to Tm_b);
 *   d_path [B][Tx][Tm] fp32 0/1 or NULL (what maximum_path returns); d_score [B] or NULL (v at the end cell).
 *   Cells beyond an utterance's own lengths are never read as data; an utterance's result does not depend on its batch.
 *   The lengths are checked on the device without a host read: an utterance with Tx_b < 1, Tx_b > Tx, Tm_b > Tm or Tm_b < Tx_b
 *   (no monotone path gives every token a frame) gets zero outputs, the others are unaffected, and mtts_mas_status(d_ws, stream)
 *   -- the one entry here that waits for the stream -- reports the first such utterance through mtts_last_error.
 * Stream-ordered, no allocation, safe under HIP graph capture (mtts_mas_status excepted).  Workspace: mtts_mas_workspace_bytes,
 * 16-byte aligned.  What the host can see (null pointers, B < 1, Tx > 1024, Tm < Tx, a small workspace) returns -1. */
int64_t mtts_mas_workspace_bytes(int B, int Tx, int Tm);
int mtts_mas_logprior(const float* d_mu_x, const float* d_y, const int64_t* d_x_lengths, const int64_t* d_y_lengths, int B, int F,
                      int Tx, int Tm, float* d_lp, void* stream);
int mtts_mas(const float* d_lp, const float* d_mu_x, const float* d_y, const int64_t* d_x_lengths, const int64_t* d_y_lengths,
             int B, int F, int Tx, int Tm, int32_t* d_durations, float* d_path, float* d_score, void* d_ws, int64_t ws_bytes,
             void* stream);
int mtts_mas_status(const void* d_ws, void* stream);

/* ---------------------------------------------------------------- scoring a recording (prior and duration losses) */

/* The two alignment-based sums of the reference's training forward, matcha/models/matcha_tts.py:108-145, per utterance and without
 * the [Tx, Tm] path: frame y of utterance b belongs to the first token whose inclusive cumulative duration exceeds y (the rule of
 * mtts_align_pool), so mu_y_fine[:, y] = mu_x[:, tok(y)] is read in place.
 *   d_prior_sum[b] = sum_{f, y < Tm_b} huber(y_fine[b,f,y] - mu_x[b,f,tok(y)], delta_prior)      (matcha_tts.py:124,143-145)
 *   d_dur_sum[b]   = sum_{x < Tx_b}    huber(logw[b,x] - log(2 + durations[b,x]), delta_dur)     (matcha_tts.py:117,128)
 *   huber(d, delta) = 0.5 d^2 for |d| < delta, else delta (|d| - 0.5 delta)                      (torch.nn.functional.huber_loss)
 * The reference multiplies log(2 + durations) by x_mask and sums over all Tx tokens; logw is already masked by the text encoder, so
 * a padded token contributes huber(0 - 0) = 0 there and is simply not visited here.  The reference's batch figures are
 * sum_b d_dur_sum[b] / sum_b Tx_b and sum_b d_prior_sum[b] / sum_b Tm_b (its y_fine_mask has one row, not n_feats).
 * d_mu_x [B,F,Tx]; d_logw [B,1,Tx]; d_durations int32 [B,Tx] (mtts_mas); d_y_fine [B,F,Tm] normalised fine mel; lengths device int64
 * [B].  Optional outputs (NULL to skip): d_prior_frame [B,Tm] = the sum over f per frame, d_dur_err [B,Tx] = the signed difference
 * logw - log(2 + durations); both zero beyond an utterance's lengths.
 * Everything is fp32 and every sum has a fixed order (no floating-point atomics): an utterance's outputs do not depend on the batch
 * or the padded shapes it comes in, and two calls give the same bits.  mtts_score_serial_run(which, F, Tx, Tm): the longest chain
 * of serial additions in the prior (0), duration (1) and flow-matching (2, with F = n_feats, Tm = T) sums, what an error bound
 * against fp64 is derived from.
 * The lengths and durations are checked on the device without a host read: an utterance with Tx_b < 1, Tx_b > Tx, Tm_b > Tm,
 * Tm_b < Tx_b, a negative duration or durations that do not sum to Tm_b gets zero outputs, the others are unaffected, and
 * mtts_score_status(d_ws, stream) -- the one entry here that waits for the stream -- reports the first such utterance through
 * mtts_last_error.  No context needed.  Stream-ordered, no allocation.  Workspace: mtts_score_workspace_bytes, 16-byte aligned.
 * What the host can see (null pointers, B < 1, F < 1, Tx > 1024, Tm < Tx, a threshold <= 0, a small workspace) returns -1. */
int64_t mtts_score_workspace_bytes(int B, int Tx, int Tm);
int mtts_score_serial_run(int which, int F, int Tx, int Tm);
int mtts_score_prior_dur(const float* d_mu_x, const float* d_logw, const int32_t* d_durations, const float* d_y_fine,
                         const int64_t* d_x_lengths, const int64_t* d_y_fine_lengths, int B, int F, int Tx, int Tm, float delta_prior,
                         float delta_dur, float* d_prior_sum, float* d_dur_sum, float* d_prior_frame, float* d_dur_err, void* d_ws,
                         int64_t ws_bytes, void* stream);
int mtts_score_status(const void* d_ws, void* stream);

/* ---------------------------------------------------------------- speaker-row gradients (fine-tuning a voice from recordings) */

/* The gradient of the prior and duration Huber sums of mtts_score_prior_dur with respect to the two speaker rows, per utterance:
 * what the reference's matcha/finetune_speaker.py trains (one row of speaker_embeddings_enc.weight and one of
 * speaker_embeddings_dur.weight, everything else frozen).  What reaches the rows in the reference's training forward:
 *   - not the flow-matching loss: mu_y is detached before decoder.compute_loss (matcha_tts.py:154-162) and the estimator has no
 *     speaker input, so there is no decoder backward;
 *   - e_dur through the duration predictor alone, whose input is x.detach() (text_encoder.py:404): per layer FiLM, the channel
 *     LayerNorm (text_encoder.py:19-27), the ReLU and the k5 convolutions of layers >= 1 (text_encoder.py:101-112), then spk_proj^T;
 *   - e_enc, concatenated behind the prenet (text_encoder.py:400), through proj_m (text_encoder.py:359-363,402), the post-LN encoder
 *     layers (RoPE attention text_encoder.py:220-237, conv FFN :253-258, Encoder.forward :299-316) and a sum over tokens of the
 *     speaker channels; no prenet, embedding or weight gradient;
 *   - MAS runs under no_grad (matcha_tts.py:187): the durations are constants.
 * This is the dropout-free (eval) gradient.
 *
 * Backward panels: the data gradient of a Linear is a GEMM with the transposed panel, that of a Conv1d(k, pad k/2) a GEMM with in /
 * out channels swapped and the taps reversed: proj_m[2]^T, proj_m[0]^T; per encoder layer conv_o^T, conv_q|k|v^T, ffn.conv_2^T,
 * ffn.conv_1^T; dp.conv_layers[1..]^T; spk_proj^T; and dp.proj's weight row (one output channel: its transpose is an outer product
 * inside the seed kernel).  They are packed on demand from the registered tensors into a buffer of their own
 * (mtts_spk_grad_weights_bytes / mtts_spk_grad_upload_weights; mtts_set_tensor invalidates them), not into the weight image, and run
 * on the library's GEMM launchers in NATIVE FP32 MFMA (arithmetic 0) whatever the context's forward arithmetic is: gradients are
 * small numbers and the fp16 two-term split loses bits below the fp16 normal range.
 *
 * mtts_spk_grad: a taped text-encoder forward (the launches of mtts_text_encoder_forward with the same arguments, intermediates kept
 *   per layer: mu_x, logw and x_mask equal that entry's bit for bit and can be read back at mtts_spk_grad_tape_offset), the alignment
 *   (d_durations_in int32 [B,Tx], or NULL: mtts_mas on this forward's mu_x, as the reference does), mtts_score_prior_dur's two sums
 *   (d_prior_sum, d_dur_sum [B]: that entry's bits), the two loss-gradient seeds
 *     d prior_sum_b / d mu_x[f,x] = - sum_{y on token x} huber'(y_fine[f,y] - mu_x[f,x], delta_prior)
 *     d dur_sum_b / d logw[x]     = huber'(logw[x] - log(2 + dur[x]), delta_dur),        huber'(d, delta) = clamp(d, -delta, delta)
 *   and the data-gradient walk back.  d_g_enc, d_g_dur [B, spk_emb_dim]: gradients of the PER-UTTERANCE sums; the reference's batch
 *   loss gradients are sum_b g_dur[b] / sum_b Tx_b and sum_b g_enc[b] / sum_b Tm_b, which the caller forms.  d_durations_out int32
 *   [B,Tx] or NULL.  Arguments d_x .. d_e_dur as for mtts_text_encoder_forward; d_y_fine [B,F,Tm] normalised fine mel.
 *   Every sum has a fixed order, there are no floating-point atomics: an utterance's rows do not depend on its batch or the padded
 *   shapes, and two calls give the same bits.  An utterance mtts_score_prior_dur refuses (lengths, durations) gets zero rows, the
 *   others are unaffected, and mtts_spk_grad_status(d_ws, stream) -- the one entry here that waits for the stream -- names it.
 *   Stream-ordered, no allocation.  Context guard and range-guard word (first word of d_ws) as the neighbouring entries.  Returns -1
 *   (mtts_last_error) for null pointers, B < 1, Tx > 1024, Tm < Tx, a threshold <= 0, a small workspace, backward panels that are
 *   not uploaded in d_grad_buf. */
int64_t mtts_spk_grad_weights_bytes(mtts_ctx* ctx);
int mtts_spk_grad_upload_weights(mtts_ctx* ctx, void* d_buf, int64_t bytes);
int64_t mtts_spk_grad_workspace_bytes(mtts_ctx* ctx, int B, int Tx, int Tm);
int64_t mtts_spk_grad_tape_offset(mtts_ctx* ctx, int B, int Tx, int Tm, int which);      /* byte offset in d_ws of 0 mu_x [B,F,Tx], 1 logw [B,Tx], 2 x_mask [B,Tx] */
int64_t mtts_spk_grad_rows_offset(mtts_ctx* ctx, int B, int Tx, int Tm);                  /* ... of the encoder's output rows [B*Tx, enc_channels + spk_emb_dim] that proj_m and the predictor read */
int mtts_spk_grad(mtts_ctx* ctx, const int64_t* d_x, const int64_t* d_x_lengths, const float* d_e_enc, const float* d_e_dur,
                  const float* d_y_fine, const int64_t* d_y_fine_lengths, const int32_t* d_durations_in, float delta_prior,
                  float delta_dur, int B, int Tx, int Tm, float* d_g_enc, float* d_g_dur, float* d_prior_sum, float* d_dur_sum,
                  int32_t* d_durations_out, void* d_grad_buf, void* d_ws, int64_t ws_bytes, void* stream);
int mtts_spk_grad_status(const void* d_ws, void* stream);

/* Style-encoder training's loss and its gradient with respect to the rows -- reference matcha/models/style_encoder.py:119-143: the
 * frozen text encoder's outputs under PREDICTED rows (d_e_enc, d_e_dur [B, spk_emb_dim]) matched against its outputs under the real
 * rows, d_mu_ref [B, n_feats, Tx] and d_logw_ref [B, Tx] as mtts_text_encoder_forward returned them (constants: the reference
 * computes them under no_grad), with smooth-L1: per term 0.5 d^2 / beta below beta, |d| - 0.5 beta from beta on (the reference's
 * betas: 0.002 for mu, 0.004 for logw).  The reference freezes Matcha in eval() for this training, so this is exactly its gradient.
 *   The taped forward and the two walks back are mtts_spk_grad's (same functions, same panels in d_grad_buf); the seeds are
 *   d ac_sum_b / d mu_x[f, x] = clamp((mu_x - mu_ref) / beta_mu, -1, 1) and the same for logw with beta_logw on x < len_b, zero
 *   elsewhere.  d_g_enc, d_g_dur [B, spk_emb_dim]: gradients of the PER-UTTERANCE sums d_ac_sum, d_rh_sum [B]; the reference's batch
 *   losses and gradients are the batch sums divided by sum_b len_b (for both: tokens, not tokens x channels), which the caller forms.
 *   Every sum has a fixed order, no floating-point atomics: an utterance's rows do not depend on its batch, two calls give the same
 *   bits.  An utterance whose length is outside [1, Tx] gets zero rows and zero sums, the others are unaffected, and
 *   mtts_spk_grad_match_status(d_ws, stream) -- the one entry here that waits for the stream -- names it.  Returns -1
 *   (mtts_last_error) for null pointers, B < 1, Tx > 1024, a beta <= 0, a small workspace (mtts_spk_grad_match_workspace_bytes),
 *   backward panels that are not uploaded in d_grad_buf. */
int64_t mtts_spk_grad_match_workspace_bytes(mtts_ctx* ctx, int B, int Tx);
int mtts_spk_grad_match(mtts_ctx* ctx, const int64_t* d_x, const int64_t* d_x_lengths, const float* d_e_enc, const float* d_e_dur,
                        const float* d_mu_ref, const float* d_logw_ref, float beta_mu, float beta_logw, int B, int Tx, float* d_g_enc,
                        float* d_g_dur, float* d_ac_sum, float* d_rh_sum, void* d_grad_buf, void* d_ws, int64_t ws_bytes, void* stream);
int mtts_spk_grad_match_status(const void* d_ws, void* stream);

/* Kernel-level entry of mtts_spk_grad_match's seed and sum kernels on given buffers (no context): d_mu / d_mu_ref [B, F, Tx],
 * d_logw / d_logw_ref [B, Tx], d_lengths int64 [B], d_w_proj [Fd] (the duration predictor's output projection row) ->
 * d_seed_mu [B*Tx, F] = clamp((mu - mu_ref) / beta_mu, -1, 1) as channels-last rows, d_seed_logw [B*Tx, Fd] = the logw seed times
 * d_w_proj, both zero at x >= len_b; d_ac_sum / d_rh_sum [B] the smooth-L1 sums.  An utterance whose length is outside [1, Tx] gets
 * zeros.  Tx <= 1024; d_scratch: mtts_match_seeds_scratch_bytes(B, F). */
int64_t mtts_match_seeds_scratch_bytes(int B, int F);
int mtts_match_seeds(const float* d_mu, const float* d_mu_ref, const float* d_logw, const float* d_logw_ref, const int64_t* d_lengths,
                     const float* d_w_proj, int B, int F, int Tx, int Fd, float beta_mu, float beta_logw, float* d_seed_mu,
                     float* d_seed_logw, float* d_ac_sum, float* d_rh_sum, void* d_scratch, void* stream);

/* Kernel-level entries of the two backward kernels, fp32 rows in and out (no context).
 * mtts_channel_layernorm_bwd: backward of mtts_channel_layernorm (text_encoder.py:19-27 + SiLU / FiLM / mask as that entry): d_x the
 *   LayerNorm's input rows [B*T, C], d_dy the upstream gradient, d_dx the result; gate 1: d_x is a ReLU output and d_dx is gated by
 *   (x > 0); d_dfilm [B, 2C] or NULL = (d gamma_b | d beta_b) summed over the T rows of each utterance in token order (needs d_film
 *   and d_scratch of B*T*C floats).
 * mtts_attention_rope_bwd: backward of the encoder's SDPA with rotary q / k (text_encoder.py:220-237): d_qkv [B*T, 3*H*D] rows AFTER
 *   the rotation (q | k | v sections), d_o the attention output and d_do its gradient [B*T, H*D], d_lengths int64 [B] (boolean query x
 *   key mask), d_cos / d_sin [>= T, D/2]; d_dqkv = the gradient with respect to q | k | v BEFORE the rotation, zero rows beyond an
 *   utterance's length.  D a multiple of 8, <= 64; T <= 1024; d_scratch B*H*T*3 floats. */
int mtts_channel_layernorm_bwd(const float* d_x, const float* d_dy, int B, int T, int C, const float* d_gamma, const float* d_beta, float eps,
                               int act, const float* d_film, const float* d_mask, int gate, float* d_dx, float* d_dfilm, void* d_scratch,
                               void* stream);
int mtts_attention_rope_bwd(const float* d_qkv, const float* d_o, const float* d_do, const int64_t* d_lengths, int B, int T, int H, int D,
                            float scale, const float* d_cos, const float* d_sin, float* d_dqkv, void* d_scratch, void* stream);

/* Kernel-level entries of mtts_spk_grad's seed, gate and token-sum kernels on given buffers (no context).
 * mtts_spk_grad_seeds: the two Huber seeds, launched as mtts_spk_grad launches them: mtts_score_prior_dur into the scratch for the
 *   verdicts, the zero fill, then the seed kernels.  d_mu_x [B, F, Tx], d_logw [B, Tx], d_durations int32 [B, Tx], d_y_fine
 *   [B, F, Tm], both length vectors int64 [B], d_w_proj [Fd] (the duration predictor's output projection row) ->
 *   d_seed_mu [B*Tx, round_up(F, 4)] = minus the sum over the frames of token x, in frame order, of clamp(y - mu_x, +-delta_prior)
 *   (zeros at x >= len_b and in the padding columns), d_seed_logw [B*Tx, Fd] = clamp(logw - log(2 + dur), +-delta_dur) * d_w_proj
 *   (zeros at x >= len_b).  An utterance that mtts_score_prior_dur refuses gets zeros; mtts_score_status(d_scratch, stream) names
 *   it.  Tx <= 1024, Tm >= Tx, deltas > 0; d_scratch 16-byte aligned, mtts_spk_grad_seeds_scratch_bytes(B, Tx, Tm) bytes.
 * mtts_grad_gate: in place on the gradient rows d_g [M, ldg], columns [0, C), against the forward's rows d_ref [M, ldref]: mode 0
 *   g *= silu'(ref); mode 1 g = 0 where not (ref > 0) or d_mask[row] == 0; mode 2 the same decision on the P16 image of ref (built
 *   in d_scratch, M * 2 C halves, residual scale 2^11, rows times d_mask, as the FFN hand-over writes it): on iff the head is
 *   positive, or the head is zero and the residual positive.  Mode 2 needs C % 32 == 0 and ldref % 4 == 0.  d_mask [M] or NULL.
 * mtts_token_sums: d_dst[b, dcol0 + c] (+)= sum over t < len_b of d_src[(b T + t), col0 + c] for c < C: four phases t = p, p + 4, ...
 *   in token order, combined as ((p0 + p1) + p2) + p3.  d_len int64 [B] or NULL (T; clamped to [0, T]); d_verdict int32 [B, 2] or
 *   NULL (first word non-zero: zero sums); accumulate 0 / 1; ld >= col0 + C, ldd >= dcol0 + C. */
int64_t mtts_spk_grad_seeds_scratch_bytes(int B, int Tx, int Tm);
int mtts_spk_grad_seeds(const float* d_mu_x, const float* d_logw, const int32_t* d_durations, const float* d_y_fine,
                        const int64_t* d_x_lengths, const int64_t* d_y_fine_lengths, const float* d_w_proj, int B, int F, int Tx, int Tm,
                        int Fd, float delta_prior, float delta_dur, float* d_seed_mu, float* d_seed_logw, void* d_scratch,
                        int64_t scratch_bytes, void* stream);
int mtts_grad_gate(float* d_g, int ldg, int M, int C, int mode, const float* d_ref, int ldref, const float* d_mask, void* d_scratch,
                   void* stream);
int mtts_token_sums(const float* d_src, int ld, int col0, int C, int B, int T, const int64_t* d_len, const int32_t* d_verdict,
                    float* d_dst, int ldd, int dcol0, int accumulate, void* stream);

/* ---------------------------------------------------------------- duration-predictor training (parameter gradients) */

/* The gradient of the duration Huber sum with respect to every parameter of the duration predictor (encoder.proj_w.*), everything else
 * frozen.  In the reference logw = proj_w(x.detach(), x_mask, e_dur) (text_encoder.py:404) and the duration loss (matcha_tts.py:117,128)
 * is the only loss that reaches those tensors, so this is the reference's gradient for them -- the dropout-free (eval) one: the
 * reference trains the predictor with p_dropout, the same deviation as mtts_spk_grad's.
 *
 * Parameters: ONE FLAT fp32 vector of mtts_dp_param_count(ctx) floats, the keys below encoder.proj_w. in state-dict order --
 * spk_proj.weight [2F, Sd], spk_proj.bias [2F], then per layer i conv_layers.i.weight [F, Cin, 5], conv_layers.i.bias [F],
 * norm_layers.i.gamma [F], norm_layers.i.beta [F] (Cin = enc_channels + spk_emb_dim for i = 0, else F), then proj.weight [F],
 * proj.bias [1]; mtts_dp_param_offset(ctx, "conv_layers.1.weight") is a tensor's first float.  Neither needs a device.
 *
 * Training component: the predictor's forward panels, LayerNorm affines, output projection and the transposed, tap-reversed panels of
 * the walk back, packed on the host from the flat vector (h_params; NULL: from the tensors registered with mtts_set_tensor) and copied
 * into d_buf (mtts_dp_train_weights_bytes(ctx) bytes, 2.5 MB at the production size; the layout depends on the configuration
 * alone).  The copy is a blocking one on the default stream: a call that still reads d_buf on another stream is NOT waited for --
 * drain that stream first (the Python mirror does).  mtts_dp_train_upload is what a training step calls after every optimiser update: it touches neither the model's weight
 * image nor the backward panels of mtts_spk_grad.  mtts_dp_train_pack writes the same bytes to host memory instead.  Native fp32 MFMA
 * (arithmetic 0) whatever the context's arithmetic is, for mtts_spk_grad's reason.
 *
 * mtts_dp_grad: d_x .. d_e_dur as for mtts_text_encoder_forward; d_durations int32 [B, Tx], required (this entry runs no alignment);
 *   d_train_buf the uploaded component; d_grad [mtts_dp_param_count], every element written; d_g_dur [B, spk_emb_dim] or NULL (the
 *   gradient with respect to the e_dur rows, per utterance, as mtts_spk_grad's); d_dur_sum [B] the per-utterance Huber sums;
 *   d_logw [B, Tx] or NULL.
 *   Forward: the prenet and encoder layers run from the context's image in the context's arithmetic (the taped forward's functions: the
 *   rows the predictor reads equal mtts_text_encoder_forward's bit for bit; proj_m is not run); the predictor runs from d_train_buf in
 *   native fp32 with every layer's rows kept.  Its logw is therefore NOT bit-equal to mtts_text_encoder_forward's under the default
 *   split arithmetic, by design.
 *   Backward: seed[r] = clamp(logw - log(2 + dur), +-delta_dur) on x < len_b (mtts_spk_grad's), the walk back of mtts_spk_grad with the
 *   panels of d_train_buf, and inside it the parameter reductions.  d_grad is the gradient of the SUM over the batch of the
 *   per-utterance sums; the reference's loss gradient is d_grad / sum_b len_b, which the caller forms.
 *   Summation orders.  M = B Tx rows r = b Tx + x are cut into chunks of R = mtts_conv_wgrad_chunk_rows(B, Tx) rows; rows with
 *   x >= len_b take no part (a select).
 *     conv_layers.i.weight / .bias: mtts_conv_wgrad with dz = the gradient at the convolution's output behind the ReLU gate, the input
 *       = the layer's taped input (the encoder's rows for i = 0, the previous FiLM output otherwise), lengths = x_lengths;
 *     norm_layers.i.gamma[c] = sum_r dy[r,c] gf_b[c] xhat[r,c], .beta[c] = sum_r dy[r,c] gf_b[c] (dy the gradient at the FiLM output,
 *       gf_b utterance b's FiLM gamma, xhat the normalised row, its mean and rstd recomputed from the taped pre-norm row by lane-strided
 *       sums and a wave butterfly): per chunk four phases p take the rows r0 + p, r0 + p + 4, ... in row order, each term (dy gf) xhat
 *       rounded product by product before it is added, the phases combined as ((p0 + p1) + p2) + p3, the chunks added in chunk order;
 *     proj.weight[c] = sum_r seed[r] h[r,c], proj.bias = sum_r seed[r] (h the last FiLM output): the same phases and chunks;
 *     spk_proj.weight[o,j] = sum_b DFILM[b,o] e_dur[b,j], spk_proj.bias[o] = sum_b DFILM[b,o], in batch order from zero, DFILM [B, 2F]
 *       the per-utterance (d gamma_b | d beta_b) that the walk accumulates over the layers (last layer first) with mtts_token_sums.
 *   Stream-ordered, no allocation, no floating-point atomics: two calls give the same bits.  An utterance with a length outside
 *   [1, Tx] or a negative duration adds exact zeros to every sum and gets a zero d_dur_sum and d_g_dur row; the others are unaffected,
 *   and mtts_dp_grad_status(d_ws, stream) -- the one entry here that waits for the stream -- names it.  Context guard and range-guard
 *   word (first word of d_ws) as the neighbouring entries.  Returns -1 (mtts_last_error) for null pointers, B < 1, Tx > 1024,
 *   delta_dur <= 0, dp_kernel != 5, a small workspace (mtts_dp_grad_workspace_bytes), a d_train_buf that was not uploaded.
 *   mtts_dp_grad_tape_offset: byte offset in d_ws of which = 0 the frozen encoder's output rows [B*Tx, enc_channels + spk_emb_dim],
 *   1 the logw [B, Tx] of the latest call. */
int64_t mtts_dp_param_count(mtts_ctx* ctx);
int64_t mtts_dp_param_offset(mtts_ctx* ctx, const char* key);
int64_t mtts_dp_train_weights_bytes(mtts_ctx* ctx);
int mtts_dp_train_pack(mtts_ctx* ctx, const float* h_params, void* h_out, int64_t bytes);
int mtts_dp_train_upload(mtts_ctx* ctx, const float* h_params, void* d_buf, int64_t bytes);
int64_t mtts_dp_grad_workspace_bytes(mtts_ctx* ctx, int B, int Tx);
int64_t mtts_dp_grad_tape_offset(mtts_ctx* ctx, int B, int Tx, int which);
int mtts_dp_grad(mtts_ctx* ctx, const int64_t* d_x, const int64_t* d_x_lengths, const float* d_e_enc, const float* d_e_dur,
                 const int32_t* d_durations, float delta_dur, int B, int Tx, void* d_train_buf, float* d_grad, float* d_g_dur,
                 float* d_dur_sum, float* d_logw, void* d_ws, int64_t ws_bytes, void* stream);
int mtts_dp_grad_status(const void* d_ws, void* stream);

/* Kernel-level entries of mtts_dp_grad's three parameter reductions on given buffers (no context), in the orders stated above.
 * mtts_ln_film_wgrad: d_x the pre-norm rows and d_dy the gradient at the FiLM output [B*T, C], d_film [B, 2C] (gamma | beta),
 *   d_lengths int64 [B] or NULL -> d_dgamma, d_dbeta [C].
 * mtts_rows_wgrad: d_seed [B*T], d_h [B*T, C] -> d_dw [C] = sum_r seed[r] h[r, c], d_db [1] = sum_r seed[r].
 * Both leave the chunks' partial results in d_ws (mtts_dp_unit_workspace_bytes(B, T, C) bytes).
 * mtts_outer_batch_sum: d_g [B, O], d_e [B, J] -> d_dw [O, J] = sum_b g[b, o] e[b, j], d_db [O] = sum_b g[b, o], batch order. */
int64_t mtts_dp_unit_workspace_bytes(int B, int T, int C);
int mtts_ln_film_wgrad(const float* d_x, const float* d_dy, const float* d_film, const int64_t* d_lengths, int B, int T, int C, float eps,
                       float* d_dgamma, float* d_dbeta, void* d_ws, int64_t ws_bytes, void* stream);
int mtts_rows_wgrad(const float* d_seed, const float* d_h, const int64_t* d_lengths, int B, int T, int C, float* d_dw, float* d_db,
                    void* d_ws, int64_t ws_bytes, void* stream);
int mtts_outer_batch_sum(const float* d_g, const float* d_e, int B, int O, int J, float* d_dw, float* d_db, void* stream);

/* ---------------------------------------------------------------- arithmetic and its range guard */

/* Range guard of the default arithmetic.  The fp16 two-term split represents an operand x as h + l / 2^11 with h = fp16(x):
 * beyond +-65504 h saturates and the product is wrong.  Every kernel that splits an operand (the P16 image writers: GEMM
 * epilogues, attention, GroupNorm-apply, the state conversion; the fp32-operand GEMM while staging) ORs 1 into the FIRST
 * 32-bit WORD OF THE WORKSPACE of the call it belongs to (mtts_text_encoder_forward / mtts_decoder_forward / mtts_cfm_solve*
 * clear it on entry): read it back after the call; non-zero = rerun on a context whose arithmetic has the fp32 range
 * (mtts_set_arithmetic(ctx, 6): three bf16 terms).  The Python mirror does this in synthesise().
 * mtts_set_arithmetic: products per fp32 multiply-accumulate as for mtts_gemm_f32's `terms` (0, 2, 3, 6; 1 = the opt-in fp16
 * mode on P16 images), overriding MTTS_GEMM_TERMS; call before mtts_weights_bytes / mtts_upload_weights (it invalidates the
 * packed image).  16 = the 16-BIT STORAGE MODE of BASELINE config #3 (the arithmetic torch.autocast gives the reference on its
 * GPU, reference matcha/inference.py:238): every activation image of the estimator and its weight planes are single fp16
 * planes (2 bytes per element, half the operand traffic), one MFMA per multiply-accumulate, fp32 accumulation, fp32
 * GroupNorm / LayerNorm statistics and ODE state; the text encoder and duration predictor keep the fp32-equivalent split
 * (durations must not move).  Not inside the 1e-3 bar: its measured mel error is reported beside its throughput.
 * 17 = the same mode with BFLOAT16 planes (the dtype BASELINE config #3 names): same layout and traffic, bf16 MFMAs, the fp32
 * exponent range (no saturation, the range guard stays silent), 8 significand bits per operand instead of 11 -- the reference's
 * own bf16 autocast deviates ~8x more from its fp32 mel than its fp16 autocast (tests/golden/prod_autocast.npz).
 * mtts_weights_saturate: 1 if a WEIGHT exceeds the fp16 range in the fp16-split mode (decided while packing). */
int mtts_set_arithmetic(mtts_ctx* ctx, int terms);
int mtts_weights_saturate(mtts_ctx* ctx);

/* ---------------------------------------------------------------- measurement */

/* GEMM arithmetic of a context (NULL: the library default): 0 native fp32 MFMA, 2 fp16 two-term split (default),
 * 6 bf16 three-term split, 3 bf16 two-term split -- see mtts_gemm_f32; 1 / 16 / 17 = the 16-bit modes of mtts_set_arithmetic. */
int mtts_gemm_terms(mtts_ctx* ctx);

/* Per-kernel-class timing with HIP events recorded on the launch stream (bench.py's roofline line).
 * Classes: 0 gemm, 1 attention, 2 norm/activation/elementwise. */
int mtts_prof_enable(mtts_ctx* ctx, int on);
int mtts_prof_reset(mtts_ctx* ctx);
/* Synchronises the recorded events; returns launches, summed milliseconds, algorithmic FLOPs and compulsory HBM
 * bytes (every operand and result element once) of a class. */
int mtts_prof_read(mtts_ctx* ctx, int klass, int64_t* launches, double* ms, double* flops, double* bytes);
/* The same records one by one, in launch order: h_out[4 i ..] = (class, ms, flops, bytes); returns the count (<= max_records). */
int64_t mtts_prof_records(mtts_ctx* ctx, double* h_out, int64_t max_records);
/* the kernel instantiation of each of those records, in the same order, '\n'-separated ("-" = untagged): the names rocprofv3
 * prints, e.g. "gemm_p16_kernel<64, false, 3, 0, true, false, 2>"; returns the record count */
int64_t mtts_prof_tags(mtts_ctx* ctx, char* out, int64_t max_bytes);

#ifdef __cplusplus
}
#endif
#endif /* MTTS_H */
