"""Voice enrolment without a GPU: the new C entries, the host-built tables of the log-mel front end against fp64 restatements of
their published definitions, the frame-count rule, and the style encoder's state-dict names through the converter."""
import ctypes as C

import numpy as np
import pytest
import torch

from conftest import ROOT, sub
import enroll_restated as R


@pytest.fixture(scope="module")
def lib():
    return sub("_hip").load()


def test_symbols_declared_and_exported(lib):
    header = (ROOT / "include" / "mtts.h").read_text()
    # (declaration, export, arity and types: test_abi.py checks them for every entry of the header)
    # the documented signatures, as the binding declares them
    assert len(lib.mtts_melfe_forward.argtypes) == 14 and lib.mtts_melfe_forward.restype is C.c_int
    assert len(lib.mtts_style_forward.argtypes) == 12 and lib.mtts_style_forward.restype is C.c_int
    assert lib.mtts_melfe_workspace_bytes.restype is C.c_int64 and lib.mtts_style_workspace_bytes.restype is C.c_int64
    assert lib.mtts_abi_version() == 2


def test_workspace_sizes_are_monotone(lib):
    m = lib.mtts_melfe_create(24000, 1024, 100)
    s = lib.mtts_style_create(100, 256, 4, 96)
    try:
        a = [lib.mtts_melfe_workspace_bytes(m, B, 120000, 128) for B in (1, 2, 8, 32)]
        b = [lib.mtts_melfe_workspace_bytes(m, 4, ld, 128) for ld in (1024, 24000, 120000, 480000)]
        c = [lib.mtts_style_workspace_bytes(s, B, 900) for B in (1, 2, 8, 32)]
        d = [lib.mtts_style_workspace_bytes(s, 4, T) for T in (8, 100, 900, 4000)]
        for seq in (a, b, c, d):
            assert all(x > 0 for x in seq) and all(x < y for x, y in zip(seq, seq[1:])), seq
        assert lib.mtts_melfe_workspace_bytes(m, 0, 1000, 128) < 0 and lib.mtts_style_workspace_bytes(s, 1, 0) < 0
    finally:
        lib.mtts_melfe_destroy(m)
        lib.mtts_style_destroy(s)


def test_unsupported_shapes_are_refused(lib):
    assert not lib.mtts_melfe_create(24000, 1000, 100)       # n_fft not a multiple of 32
    assert b"n_fft" in lib.mtts_last_error()
    assert not lib.mtts_style_create(100, 255, 4, 96)        # hidden not a multiple of 4
    assert not lib.mtts_style_create(100, 256, 0, 96)


@pytest.mark.parametrize("sr,n_fft,n_mels", [(24000, 1024, 100), (24000, 1024, 20), (16000, 512, 80)])
def test_host_tables_equal_fp64_restatement(sr, n_fft, n_mels):
    fe = sub("mel").MelFrontEnd(sr, n_fft, n_mels)
    assert fe.n_bins == n_fft // 2 + 1
    assert np.abs(fe.basis().astype(np.float64) - R.dft_basis(n_fft)).max() <= 1e-7
    fb = fe.filterbank().astype(np.float64)
    assert np.abs(fb - R.htk_fbanks(fe.n_bins, sr, n_mels)).max() <= 1e-7
    assert ((fb > 0).sum(axis=1) <= 2).all()                 # each bin feeds at most two filters: the band-sum form is complete


@pytest.mark.parametrize("n_fft,hop,n", [(64, 16, 48), (64, 64, 200), (512, 160, 417), (1024, 256, 768), (1024, 100, 2222), (2048, 300, 5000)])
def test_matrix_form_of_the_stft_equals_torch_stft(n_fft, hop, n):
    """The two-stage restatement the kernel-level tests use (frames times basis, then filterbank and log) is torch.stft's result:
    fp64 against fp64, so the bound is a few fp64 ulps of the frame's largest magnitude."""
    y = R.synthetic_clip(n, n_fft + hop, "noise")
    mag = R.stft_mag(y, hop, n_fft)
    ref = torch.stft(y.double()[: n // hop * hop], n_fft, hop_length=hop, win_length=n_fft, window=torch.hann_window(n_fft, dtype=torch.float64),
                     center=True, pad_mode="reflect", return_complex=True).abs().T
    assert mag.shape == ref.shape == (n // hop + 1, n_fft // 2 + 1)
    assert ((mag - ref).abs().amax(1) / ref.amax(1)).max().item() <= 1e-13
    fb = R.htk_fbanks(n_fft // 2 + 1, 24000, 100)
    assert (R.mel_from_mag(mag, fb, -4.0, 2.0) - R.log_mel(y, hop, -4.0, 2.0, n_fft=n_fft).T).abs().max().item() <= 1e-9
    # the fp32 form (the unit of the device's error) differs from fp64 by fp32 rounding, not by a definition
    c32 = R.stft_mag(y, hop, n_fft, torch.from_numpy(R.dft_basis(n_fft)).float())
    assert c32.dtype == torch.float32 and ((c32.double() - ref).abs().amax(1) / ref.amax(1)).max().item() <= 2e-6


def test_frame_count_rule():
    mel = sub("mel")
    for n, hop in [(641, 128), (1024, 256), (1279, 256), (120000, 128), (120001, 128)]:
        assert mel.n_frames(n, hop) == n // hop + 1
        y = torch.zeros(n)
        ref = torch.stft(y[: n // hop * hop], 1024, hop_length=hop, window=torch.hann_window(1024), center=True, pad_mode="reflect",
                         return_complex=True)
        assert ref.shape[-1] == mel.n_frames(n, hop)


def test_extractor_has_no_cpu_path():
    mel = sub("mel")
    with pytest.raises(RuntimeError, match="HIP device"):
        mel.extract(torch.zeros(1, 4096), [4096], 256)
    with pytest.raises(ValueError, match="log_eps"):
        mel.get_mel_extractor(log_eps=1e-5)


def test_style_state_dict_names_round_trip_through_converter(tmp_path):
    style, ck = sub("style"), sub("checkpoint")
    torch.manual_seed(3)
    src = style.StyleEncoder(20, 32, 3, 16)
    names = [f"convs.{i}.{p}" for i in range(3) for p in ("weight", "bias")] + [f"proj_{h}.{p}" for h in ("enc", "dur") for p in ("weight", "bias")]
    assert sorted(src.state_dict().keys()) == sorted(names)
    # a StyleEncoderLightningModule checkpoint: "style_encoder."-prefixed keys next to the frozen Matcha model's
    lightning_sd = {"style_encoder." + k: v.clone() for k, v in src.state_dict().items()}
    lightning_sd["matcha.encoder.emb.weight"] = torch.zeros(4, 4)
    path = tmp_path / "style.ckpt"
    torch.save({"state_dict": lightning_sd, "hyper_parameters": {}}, str(path))
    out = ck.convert_style_checkpoint(path, tmp_path / "converted")
    assert style.is_converted_style(out)
    from safetensors.torch import load_file
    flat = load_file(str(out / style.STYLE_WEIGHTS))
    assert sorted(flat.keys()) == sorted(names)
    back = style.load_style_encoder(out, device="cpu")
    assert back.cfg == dict(n_feats=20, hidden_channels=32, n_layers=3, spk_emb_dim=16)
    for k, v in src.state_dict().items():
        assert torch.equal(back.state_dict()[k], v), k
    direct = style.StyleEncoder(20, 32, 3, 16)
    direct.load_state_dict(lightning_sd, strict=True)       # the prefixed keys load as they are
    assert torch.equal(direct.proj_dur.weight, src.proj_dur.weight)
    with pytest.raises(RuntimeError, match="HIP device"):
        back(torch.zeros(1, 20, 8))


def test_request_and_speaker_rows_accept_a_pair():
    bt = sub("batcher")
    pair = (torch.zeros(16), torch.ones(16))
    r = bt.Request(ids=[1, 2, 3], speaker_embedding=pair)
    assert r.speaker_embedding is pair and r.group == ("midpoint", 4)
