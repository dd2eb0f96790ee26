"""Voice enrolment end to end on the GPU: clips -> enroll_voice -> synthesise, against the oracle fed with CPU-restated rows;
add_speaker; a batcher batch that mixes a table voice, a voice mix and an enrolled voice."""
import pytest
import torch

from conftest import sub
import enroll_restated as R

pytestmark = pytest.mark.gpu


def maxabs(a, b):
    return (a.detach().cpu().double() - b.detach().cpu().double()).abs().max().item()


@pytest.fixture(scope="module")
def env(hparams, synthetic):
    if not torch.cuda.is_available():
        pytest.fail("a HIP device is required for -m gpu tests (no CPU fallback exists)")
    inf, style = sub("inference"), sub("style")
    dev = torch.device("cuda")
    hp = hparams.tiny(n_spks=3)
    sd = synthetic.make_state_dict(hp, seed=7)
    torch.manual_seed(21)
    enc = style.StyleEncoder(hp.n_feats, 32, 2, hp.spk_emb_dim)
    enc_sd = {k: v.clone() for k, v in enc.state_dict().items()}
    clips = [R.synthetic_clip(n, 30 + i, "voiced") for i, n in enumerate([9000, 6100, 12345])]

    def fresh():
        m = inf.MatchaTTSInfer(**hp.as_reference_kwargs())
        m.load_state_dict(sd, strict=True)
        m = m.to(dev).eval()
        m.decoder.solver = "midpoint"
        return m
    return hp, sd, enc.to(dev).eval(), enc_sd, clips, fresh, dev


def restated_rows(hp, sd, enc_sd, clips):
    rows = [R.style_rows(enc_sd, R.log_mel(c, 128, float(sd["mel_mean"]), float(sd["mel_std"]), n_mels=hp.n_feats),
                         c.numel() // 128 + 1) for c in clips]
    return torch.stack([r[0] for r in rows]).mean(0).float(), torch.stack([r[1] for r in rows]).mean(0).float()


def test_enrolled_voice_matches_oracle(env, synthetic, oracle):
    hp, sd, enc, enc_sd, clips, fresh, dev = env
    model = fresh()
    e_enc, e_dur = model.enroll_voice(clips, enc)
    assert e_enc.shape == e_dur.shape == (1, hp.spk_emb_dim)
    r_enc, r_dur = restated_rows(hp, sd, enc_sd, clips)
    assert maxabs(e_enc[0], r_enc) <= 1e-4 and maxabs(e_dur[0], r_dur) <= 1e-4
    # several voices in one call: voice 0 again, and the single clips as voices of their own
    many = model.enroll_voice([clips, clips[:1], [clips[2].cuda()]], enc)
    assert many[0].shape == (3, hp.spk_emb_dim)
    assert torch.equal(many[0][0], e_enc[0]) and torch.equal(many[1][0], e_dur[0])
    # the oracle reads speaker rows from the state dict: append the restated rows and ask for the new id
    sd2 = dict(sd)
    sd2["speaker_embeddings_enc.weight"] = torch.cat([sd["speaker_embeddings_enc.weight"], r_enc[None]], 0)
    sd2["speaker_embeddings_dur.weight"] = torch.cat([sd["speaker_embeddings_dur.weight"], r_dur[None]], 0)
    x, x_len, _ = synthetic.make_inputs(hp, 2, 12, seed=1234, lengths=[12, 9])
    with torch.inference_mode():
        ref = oracle.synthesise(sd2, hp, x, x_len, 2, speaker=torch.tensor([hp.n_spks, hp.n_spks]), solver="midpoint")
    z = synthetic.cpu_noise((2, hp.n_feats, ref["t_pad"])).to(dev)
    out = model.synthesise(x.to(dev), x_len.to(dev), 2, speaker_embeddings=(e_enc.expand(2, -1).contiguous(), e_dur.expand(2, -1).contiguous()), z=z)
    assert out["mel"].shape == ref["mel"].shape
    assert maxabs(out["mel"], ref["mel"]) <= 1e-3


def test_add_speaker_equals_passing_the_rows_after_a_graph_capture(env, synthetic):
    hp, sd, enc, enc_sd, clips, fresh, dev = env
    model = fresh()
    model.decoder.graph_mode = "1"
    e_enc, e_dur = model.enroll_voice(clips, enc)
    x, x_len, _ = synthetic.make_inputs(hp, 1, 14, seed=99)
    x, x_len = x.to(dev), x_len.to(dev)
    by_rows = model.synthesise(x, x_len, 2, speaker_embeddings=(e_enc, e_dur))["mel"].clone()      # captures a graph on the old table
    replays = model.decoder.graph_replays
    assert replays >= 1
    table0 = model.synthesise(x, x_len, 2, speaker=0)["mel"].clone()
    new_id = model.add_speaker(e_enc, e_dur)
    assert new_id == hp.n_spks == 3 and model.hp.n_spks == 4
    assert model.state_dict()["speaker_embeddings_enc.weight"].shape == (4, hp.spk_emb_dim)
    by_id = model.synthesise(x, x_len, 2, speaker=new_id)["mel"]
    assert model.decoder.graph_replays > replays + 1
    assert maxabs(by_id, by_rows) <= 1e-6
    assert maxabs(model.synthesise(x, x_len, 2, speaker=0)["mel"], table0) <= 1e-6           # the old voices are untouched
    second = model.add_speaker(e_enc * 0.5, e_dur * 0.5)
    assert second == 4 and model.synthesise(x, x_len, 2, speaker=second)["mel"].isfinite().all()


def test_batcher_mixes_table_voice_mix_and_enrolled_voice(env, synthetic):
    hp, sd, enc, enc_sd, clips, fresh, dev = env
    bt = sub("batcher")
    model = fresh()
    pair = tuple(t[0] for t in model.enroll_voice(clips, enc))
    voices = [dict(speaker=2), dict(voice_mix=[(0, 0.7), (1, 0.3)]), dict(speaker_embedding=pair)]
    ids = [synthetic.make_inputs(hp, 1, n, seed=70 + i)[0][0].tolist() for i, n in enumerate([30, 22, 41])]
    with bt.FrameBudgetBatcher(model, max_batch=8, max_tokens=4096, max_wait_ms=50.0) as q:
        futs = [q.submit(tok, solver="midpoint", n_timesteps=2, **v) for tok, v in zip(ids, voices)]
        results = [f.result(timeout=120) for f in futs]
        assert q.batches_run == 1
    for res, tok, v in zip(results, ids, voices):
        x, x_len = torch.tensor([tok], device=dev), torch.tensor([len(tok)], device=dev)
        kw = dict(speaker_embeddings=tuple(t[None] for t in pair)) if "speaker_embedding" in v else v
        solo = model.synthesise(x, x_len, 2, **kw)
        assert res["mel_length"] == int(solo["mel_lengths"][0])
        assert maxabs(res["mel"][None], solo["mel"][:, :, :res["mel_length"]]) < 5e-5
    rows = model.speaker_rows([2, [(0, 0.7), (1, 0.3)], pair])
    assert torch.equal(rows[0][2], pair[0]) and torch.equal(rows[1][2], pair[1])
