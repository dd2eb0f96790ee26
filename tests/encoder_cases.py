"""The cases the text-encoder tests share (no tests here): three encoders, four batches of token lengths, two pairs of duration factors,
and the fp64 / fp32 oracle answers, computed once per (encoder, batch).  tests/test_encoder_oracle.py checks the references and the
precondition of the duration check on the CPU; tests/test_hip_encoder.py runs mtts_text_encoder_forward against them.

Encoders (weights: synthetic.make_state_dict(hp, seed=7, duration_recipe=False), so the durations vary per token):
  tiny        hparams.tiny(n_spks=2): hidden width 48 = 32 + 16, 2 heads of 24, filter 96, duration filter 32.
  production  hparams.prod_v20(n_spks=3): hidden width 288, 6 heads of 48 (padded to 64 by the attention kernel), d_rope 24, filter 1152.
  odd         tiny with filter_channels=80 and dp_filter_channels=36: multiples of 4 (mtts_create accepts both as they are) that are no
              multiples of 32, so every panel has K padding and the second FFN conv takes the fp32-row branch with a_mask under the
              default arithmetic as well.

Batches (inputs: synthetic.make_inputs(hp, B, Tx, seed=SEED_X, lengths=...), speaker b mod n_spks per row):
  one     [1]                every conv tap but the centre is padding, the key tile holds one key
  edge64  [65, 64, 63, 1]    the 64-key tile edge from both sides and the 64-query block edge
  three   [129, 128, 5]      three key tiles
  five    [257, 200]         five key tiles and the second 256-thread block of seq_mask_kernel; tiny and odd only

Not covered here: the 128-row GEMM tile, which the encoder reaches only above roughly 4700 rows; tests/test_hip_kernels_f32.py forces
it at kernel level.
"""
import dataclasses
import functools

import torch

from conftest import sub

ENCODERS = ("tiny", "production", "odd")
BATCHES = {"one": [1], "edge64": [65, 64, 63, 1], "three": [129, 128, 5], "five": [257, 200]}
BATCHES_OF = {"tiny": ("one", "edge64", "three", "five"), "production": ("one", "edge64", "three"),
              "odd": ("one", "edge64", "three", "five")}
CASES = [(enc, batch) for enc in ENCODERS for batch in BATCHES_OF[enc]]
FACTORS = ((1.0, 1.0), (1.03, 0.9))             # (scale_correction, length_scale)
SEED_W = 7
# (encoder, batch) -> seed of the token ids where it is not 1: with seed 1 one token of each of these two cases sits in the rounding
# band of a factor pair (tiny five at (1.03, 0.9), odd three at (1.0, 1.0); tests/test_encoder_oracle.py)
SEED_X = {("tiny", "five"): 2, ("odd", "three"): 2}
LOGW_BAR = 2e-5                                 # the project's bar on logw and mu_x (test_tiny_encoder_vs_golden)
MU_BAR = 2e-5


@functools.lru_cache(maxsize=None)
def weights(enc):
    """(hp, state dict) of an encoder."""
    hparams, synthetic = sub("hparams"), sub("synthetic")
    if enc == "production":
        hp = hparams.prod_v20(n_spks=3)
    else:
        hp = hparams.tiny(n_spks=2)
        if enc == "odd":
            hp = dataclasses.replace(hp, encoder=dataclasses.replace(hp.encoder, filter_channels=80, dp_filter_channels=36))
    return hp, synthetic.make_state_dict(hp, seed=SEED_W, duration_recipe=False)


@functools.lru_cache(maxsize=None)
def inputs(enc, batch):
    """(x [B, Tx] int64, x_lengths [B], speakers [B], e_enc [B, S], e_dur [B, S]) of a case, on the CPU."""
    hp, sd = weights(enc)
    lengths = BATCHES[batch]
    x, x_len, spk = sub("synthetic").make_inputs(hp, len(lengths), max(lengths), seed=SEED_X.get((enc, batch), 1), lengths=lengths)
    return x, x_len, spk, sd["speaker_embeddings_enc.weight"][spk], sd["speaker_embeddings_dur.weight"][spk]


@functools.lru_cache(maxsize=None)
def reference(enc, batch, dtype=torch.float64):
    """(mu_x, logw, x_mask) of oracle.text_encoder_forward with every floating tensor cast to ``dtype``, plain softmax attention."""
    import matcha_oracle
    hp, sd = weights(enc)
    x, x_len, _, e_enc, e_dur = inputs(enc, batch)
    sd = {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in sd.items()}
    with torch.no_grad():
        return matcha_oracle.text_encoder_forward(sd, hp, x, x_len, e_enc.to(dtype), e_dur.to(dtype), use_torch_sdpa=False)


def rounding_band(logw64, x_mask, sc, ls):
    """The precondition of the integer check on durations: with v = (exp(logw64) - 2) sc ls the fp64 duration before rounding and
    h = sc ls exp(logw64) (2e-5 + 2^-21) what a logw inside the bar (2e-5) and durations_kernel's fp32 work (eight fp32 units for
    expf, the subtraction and the two products) can move it by, a valid token with v > 0.5 - h (below that the clamp to one frame
    decides) must not lie within h of a half-integer.  Returns (tokens in the band, valid tokens, largest frame count)."""
    valid = x_mask.squeeze(1) > 0
    e = torch.exp(logw64.double().squeeze(1))
    v = (e - 2.0) * sc * ls
    h = sc * ls * e * (LOGW_BAR + 2.0 ** -21)
    to_half = ((v - 0.5) - torch.round(v - 0.5)).abs()          # distance to the nearest k + 0.5
    bad = valid & (v > 0.5 - h) & (to_half <= h)
    return int(bad.sum()), int(valid.sum()), int(v[valid].round().clamp(min=1).max())
