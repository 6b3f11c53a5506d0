"""awt_audio_encode's conv stem on the live positions only (tuning knob "conv_live") against the stem on every position:
the hidden states -- and the features, where they are returned -- must agree bit for bit, whatever the clip lengths, the batch, the chunking and
the operand precision."""
import numpy as np
import pytest
import torch

from mlx8_ws_audio_transformer_amd import _lib, synth, weights as wts
from oracle import encoder as oracle_enc
from oracle import logmel as oracle_mel
from tests.util import mini_at

pytestmark = pytest.mark.gpu

_ENCODERS = {}


def _enc(S, precision, chunk=0):
    from mlx8_ws_audio_transformer_amd.encoder import NativeWhisperEncoder
    key = (S, precision, chunk)
    if key not in _ENCODERS:       # mini: d = 128, 2 layers, 2 heads, ffn 512, 80 mels
        _ENCODERS[key] = NativeWhisperEncoder(mini_at(S), precision=precision, seed=0, init_profile="test", chunk_clips=chunk).eval()
    return _ENCODERS[key]


def _noise_i16(B, n, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-12000, 12000, (B, n), dtype=torch.int16, generator=g).cuda()


def _both(enc, pcm, n_valid=None, max_valid=None, features=False):
    """(outputs with conv_live = 1, outputs with conv_live = 0); the knob is back at its default afterwards."""
    nv = None if n_valid is None else torch.tensor(n_valid, dtype=torch.int32)
    try:
        _lib.tuning_set("conv_live", 1)
        live = enc.encode_pcm(pcm, n_valid=nv, max_valid=max_valid, return_features=features)
        _lib.tuning_set("conv_live", 0)
        full = enc.encode_pcm(pcm, n_valid=nv, max_valid=max_valid, return_features=features)
    finally:
        _lib.tuning_set("conv_live", 1)
    return live, full


def _assert_same(enc, pcm, n_valid=None, max_valid=None):
    live, full = _both(enc, pcm, n_valid, max_valid)
    assert torch.isfinite(full).all()
    assert torch.equal(live, full)


@pytest.mark.parametrize("precision,n_valid", [(p, n) for p in ("f16f8", "bf16x3") for n in ([64000, 16000, 1], None, [64000, 16000, 0])] + [("fp16x3", [64000, 16000, 1])])
def test_four_second_clips_ragged(precision, n_valid):
    pcm = torch.from_numpy(synth.synth_clips_i16(3, seed=1234, first=20)).cuda()
    assert pcm.shape[1] == 64000 and _lib.conv_stem_positions(1500, 64000) == 204
    _assert_same(_enc(1500, precision), pcm, n_valid, 64000)


@pytest.mark.parametrize("precision", ["f16f8", "bf16x3"])
def test_twenty_short_clips_one_tile_spans_many_clips(precision):
    # Sc = 9: groups of 9 output rows and 18 source rows, a 128-row tile crosses fourteen clips (the GEMM's row maps with short groups)
    assert _lib.conv_stem_positions(1500, 1600) == 9
    _assert_same(_enc(1500, precision), _noise_i16(20, 1600, 1))


@pytest.mark.parametrize("precision", ["f16f8", "bf16x3"])
@pytest.mark.parametrize("max_valid,positions", [(476000, 1492), (478000, 1498), (480000, 1500)])     # 7 broadcast rows, 1 broadcast row, the full path
def test_nearly_full_clips(precision, max_valid, positions):
    assert _lib.conv_stem_positions(1500, max_valid) == positions
    _assert_same(_enc(1500, precision), _noise_i16(2, 480000, 2), None, max_valid)


@pytest.mark.parametrize("precision", ["f16f8", "bf16x3"])
@pytest.mark.parametrize("max_valid,positions", [(62520, 199), (62521, 200), (64000, 200)])     # S = 200: the last length that compacts, the first that does not, live clamped to T
def test_short_encoder_switch_to_the_full_path(precision, max_valid, positions):
    assert _lib.conv_stem_positions(200, max_valid) == positions
    _assert_same(_enc(200, precision), _noise_i16(2, 64000, 3), None, max_valid)


@pytest.mark.parametrize("precision", ["f16f8", "bf16x3"])
def test_chunks_apply_the_bound_each(precision):
    pcm = torch.from_numpy(synth.synth_clips_i16(5, seed=1234, first=40)).cuda()
    n_valid = [64000, 30000, 64000, 5, 48000]
    live, full = _both(_enc(1500, precision, chunk=2), pcm, n_valid, 64000)          # chunks of 2, 2 and 1 clips
    assert torch.equal(live, full)
    assert torch.equal(live, _enc(1500, precision).encode_pcm(pcm, n_valid=torch.tensor(n_valid, dtype=torch.int32), max_valid=64000))


@pytest.mark.parametrize("precision", ["f16f8", "bf16x3"])
def test_returned_features_are_complete(precision):
    pcm = torch.from_numpy(synth.synth_clips_i16(3, seed=1234, first=60)).cuda()
    (h1, f1), (h0, f0) = _both(_enc(1500, precision), pcm, [64000, 16000, 1], 64000, features=True)
    assert torch.equal(h1, h0) and torch.equal(f1, f0)
    assert tuple(f1.shape) == (3, 80, 3000) and torch.isfinite(f1).all()
    assert torch.equal(f1[:, :, 402:], f1[:, :1, 402:403].expand(-1, 80, 2598))     # the padding constant reaches frame T - 1


def test_whisper_tiny_against_the_oracle():
    from mlx8_ws_audio_transformer_amd.encoder import NativeWhisperEncoder
    cfg = wts.config("tiny")
    pcm = synth.synth_clips_i16(2, seed=1234, first=0)
    enc = NativeWhisperEncoder(cfg, precision="f16f8", seed=0, init_profile="test").eval()
    assert _lib.conv_stem_positions(cfg.max_source_positions, 64000) < cfg.max_source_positions
    hidden = enc.encode_pcm(torch.from_numpy(pcm).cuda(), max_valid=64000)
    mel = oracle_mel.whisper_logmel([synth.pcm_i16_to_f32(c) for c in pcm], n_samples=cfg.n_frames * 160)
    ref = oracle_enc.encoder_forward(wts.init_encoder_weights(cfg, 0, "test"), mel, cfg.heads).numpy()
    err = float(np.abs(hidden.cpu().numpy() - ref).max())
    print("tiny f16f8, compact conv stem: hidden max-abs", err)
    assert err <= 1e-3, err
