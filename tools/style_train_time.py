#!/usr/bin/env python3
"""The measurement behind profiles/r29_style_train.md: ``StyleTrainer.step`` at B = 32 clips of about 600 fine frames with 128-token
texts (prod architecture, random weights) and its parts -- wall clock between device synchronisations, (median, min, max) of 10
after 3 warm-up calls; the weight-gradient entry alone by device events over 20 back-to-back calls.

    python tools/style_train_time.py [OUT.json]"""
import importlib, json, statistics, sys, time
from pathlib import Path
import torch
ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
PKG = "matcha-tts-24k_amd"
hip = importlib.import_module(PKG + "._hip"); style = importlib.import_module(PKG + ".style")
hparams = importlib.import_module(PKG + ".hparams"); synthetic = importlib.import_module(PKG + ".synthetic")
inf = importlib.import_module(PKG + ".inference")
dev = torch.device("cuda")
B, T, Tx, N, WARM = 32, 600, 128, 10, 3

def timed(fn, n=N, warm=WARM):
    for _ in range(warm):
        fn()
    out = []
    for _ in range(n):
        torch.cuda.synchronize(); t = time.perf_counter(); fn(); torch.cuda.synchronize(); out.append((time.perf_counter() - t) * 1e3)
    return statistics.median(out), min(out), max(out)

hp = hparams.prod_v20(n_spks=10)
model = inf.MatchaTTSInfer(**hp.as_reference_kwargs())
model.load_state_dict(synthetic.make_state_dict(hp, seed=7, duration_recipe=False), strict=True)
model = model.to(dev).eval()
torch.manual_seed(0)
enc = style.StyleEncoder(100, 256, 4, 96).to(dev).eval()
g = torch.Generator().manual_seed(1)
lens = torch.randint(520, T + 1, (B,), generator=g); lens[0] = T
xl = torch.randint(100, Tx + 1, (B,), generator=g); xl[0] = Tx
x, _, spk = synthetic.make_inputs(hp, B, Tx, seed=3, lengths=xl.tolist())
mel = torch.randn(B, 100, T, generator=g)
x, xl, spk, mel, lens = x.to(dev), xl.to(dev), spk.to(dev), mel.to(dev), lens.to(dev)
res = {"B": B, "T": T, "Tx": Tx, "fine_frames_mean": float(lens.float().mean()), "tokens": int(xl.sum())}
trainer = style.StyleTrainer(model, enc)
res["step_ms"] = timed(lambda: trainer.step(x, xl, mel, lens, spk))
# the parts, each between synchronisations
h = model.hip
e_enc, e_dur = model._voice_rows(B, dev, spk)
res["style_forward_taped_ms"] = timed(lambda: enc.forward_taped(mel, lens))
res["style_forward_plain_ms"] = timed(lambda: enc(mel, lengths=lens))
res["encoder_forward_ms"] = timed(lambda: h.text_encoder(x, xl, e_enc, e_dur))
p_enc, p_dur = enc.forward_taped(mel, lens)
mu_ref, logw_ref, _ = h.text_encoder(x, xl, e_enc, e_dur)
res["speaker_grad_match_ms"] = timed(lambda: h.speaker_grad_match(x, xl, p_enc, p_dur, mu_ref, logw_ref, check_lengths=False))
res["style_match_grad_ms"] = timed(lambda: model.style_match_grad(x, xl, (p_enc, p_dur), speaker=spk))
out = h.speaker_grad_match(x, xl, p_enc, p_dur, mu_ref, logw_ref)
tok = xl.float().sum()
ge, gd = out["g_enc"] / tok, out["g_dur"] / tok
res["style_backward_ms"] = timed(lambda: enc.backward(ge, gd))
lib = hip.load()
for cin, ldx in ((100, 100), (256, 256)):
    dz = torch.randn(B * T, 256, device=dev); xx = torch.randn(B * T, ldx, device=dev)
    dw = torch.empty(256 * cin * 5, device=dev); db = torch.empty(256, device=dev)
    need = lib.mtts_conv_wgrad_workspace_bytes(B, T, cin, 256)
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    call = lambda: hip.check(lib.mtts_conv_wgrad(hip.ptr(dz), hip.ptr(xx), hip.ptr(lens), B, T, cin, ldx, 256, hip.ptr(dw), hip.ptr(db), ws.data_ptr(), need, hip.stream_ptr()))
    # device time of 20 back-to-back calls between two events
    for _ in range(3):
        call()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(20):
        call()
    b.record(); torch.cuda.synchronize()
    ms = a.elapsed_time(b) / 20
    flops = 2.0 * B * T * cin * 256 * 5
    res[f"conv_wgrad_{cin}x256_ms"] = ms
    res[f"conv_wgrad_{cin}x256_tflops"] = flops / ms / 1e9
    res[f"conv_wgrad_{cin}x256_partials_MiB"] = need / 2 ** 20
grads = enc.backward(ge, gd).clone()
def opt():
    trainer.flat.grad = grads
    trainer.optimizer.step()
res["optimizer_ms"] = timed(opt)
def repack():
    enc.mark_updated()
    enc._ready()
res["repack_forward_image_ms"] = timed(repack)
def repack_panels():
    object.__setattr__(enc, "_grad_weights", None)
    enc.forward_taped(mel, lens); enc.backward(ge, gd)
res["taped_fwd_bwd_with_panel_upload_ms"] = timed(repack_panels)
res["taped_fwd_bwd_ms"] = timed(lambda: (enc.forward_taped(mel, lens), enc.backward(ge, gd)))
if len(sys.argv) > 1:
    Path(sys.argv[1]).write_text(json.dumps(res, indent=1))
print(json.dumps(res, indent=1))
