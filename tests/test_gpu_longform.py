"""GPU: long-form features (`truncation=False, padding="longest"`) against the oracle and HF's mask, and generate with timestamps
(short-form and the long-form seek loop, greedy and beams) against transformers 5.15 on tools/make_golden_timestamps.py's fixture."""
import json
import os
import sys

import numpy as np
import pytest
import torch

from mlx8_ws_audio_transformer_amd import generation as G, weights as wts
from tests.util import golden

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))


def _tool():
    import make_golden_timestamps as T
    return T


@pytest.mark.parametrize("lengths", [(16001, 7 * 16000 + 37, 33 * 16000 + 151), (480000 + 80,), (24000 + 159, 24000 + 1)])
def test_longest_features_match_oracle_and_hf_mask(lengths):
    from mlx8_ws_audio_transformer_amd.feature_extraction import WhisperFeatureExtractor
    from oracle import logmel as omel
    rng = np.random.default_rng(sum(lengths))
    clips = [(0.1 * rng.standard_normal(n)).astype(np.float32) for n in lengths]
    fe = WhisperFeatureExtractor()
    out = fe(clips, sampling_rate=16000, truncation=False, padding="longest", return_attention_mask=True, return_tensors="pt")
    N = max(lengths)
    ref = omel.whisper_logmel(clips, n_samples=N)
    assert out["input_features"].shape == (len(clips), 80, N // 160) == ref.shape
    np.testing.assert_allclose(out["input_features"].numpy(), ref, rtol=0, atol=1e-5)
    mask = out["attention_mask"].numpy()                                  # HF: one column per feature frame (N // 160)
    assert mask.shape == (len(clips), N // 160)
    assert mask.sum(-1).tolist() == [min(-(-n // 160), N // 160) for n in lengths]
    F = golden("generate_timestamps.npz")
    if tuple(F["mask_lengths"]) == lengths:
        np.testing.assert_array_equal(mask, F["mask_ragged"])              # recorded from transformers' extractor
    default = fe(clips, sampling_rate=16000, return_tensors="pt")["input_features"]          # the truncating default is unchanged
    np.testing.assert_allclose(default.numpy(), omel.whisper_logmel([c[:480000] for c in clips], n_samples=480000), rtol=0, atol=1e-5)


def _model(F):
    from mlx8_ws_audio_transformer_amd.finetune import WhisperLoRAModel
    T = _tool()
    cfg = wts.config("mini")
    model = WhisperLoRAModel(cfg, None, decoder_layers=2, vocab=T.VOCAB, max_target_positions=T.DEC["max_pos"])
    model.encoder.load_state_dict({k: torch.from_numpy(v) for k, v in T.encoder_weights(cfg).items()}, strict=False)
    Wd = T.decoder_weights(cfg, int(F["dec_seed"]), float(F["logit_scale"]), float(F["ts_scale"]), float(F["eos_scale"]))
    model.decoder.load_state_dict({k: torch.from_numpy(v) for k, v in Wd.items()}, strict=True)
    model.generation_config = G.GenerationConfig.from_dict(json.loads(str(F["generation_config"])))
    return model.eval()


def _features(seconds, longform=True):
    from mlx8_ws_audio_transformer_amd.feature_extraction import WhisperFeatureExtractor
    T = _tool()
    audio = [T.clip_audio(s, c) for c, s in enumerate(seconds)]
    fe = WhisperFeatureExtractor()
    if longform:
        f = fe(audio, sampling_rate=16000, truncation=False, padding="longest", return_attention_mask=True, return_tensors="pt")
        return f["input_features"].cuda(), f["attention_mask"]
    return fe(audio, sampling_rate=16000, return_tensors="pt")["input_features"].cuda(), None


def _check(out, F, key):
    np.testing.assert_array_equal(out["sequences"].cpu().numpy(), F["seq_" + key], err_msg=key)
    rows = [(c, s) for c, segs in enumerate(out["segments"]) for s in segs]
    assert len(rows) == len(F["seg_" + key]), key
    for (c, s), (c2, a, b, i0, i1), (t0, t1) in zip(rows, F["seg_" + key], F["segtime_" + key]):
        assert c == c2 and s["tokens"].tolist() == F["segtok_" + key][a:b].tolist() and tuple(s["idxs"]) == (i0, i1), key
        assert abs(s["start"] - t0) <= 1e-9 and abs(s["end"] - t1) <= 1e-9, key


@torch.no_grad()
def test_fixture_cases_match_transformers():
    F = golden("generate_timestamps.npz")
    model = _model(F)
    lf, mask = _features(tuple(F["lf_seconds"]))
    sf, _ = _features(tuple(F["sf_seconds"]), longform=False)
    one, _ = _features(tuple(F["lf_seconds"][1:2]))
    np.testing.assert_array_equal(mask.numpy(), F["mask_lf"])
    _check(model.generate(lf, attention_mask=mask, language="en", return_segments=True), F, "lf_greedy")
    _check(model.generate(lf, attention_mask=mask, language="en", num_beams=4, return_segments=True), F, "lf_beam")
    _check(model.generate(lf, attention_mask=mask, return_dict_in_generate=True), F, "lf_detect")
    _check(model.generate(one, language="en", return_segments=True), F, "single")
    _check(model.generate(sf, language="en", return_timestamps=True, return_segments=True), F, "sf_greedy")
    _check(model.generate(sf, language="en", num_beams=3, return_timestamps=True, return_segments=True), F, "sf_beam")
    gc = G.GenerationConfig.from_dict({**model.generation_config.to_dict(), "max_initial_timestamp_index": int(F["mii"])})
    _check(model.generate(lf, attention_mask=mask, language="en", generation_config=gc, return_segments=True), F, "mii")
    plain = model.generate(lf, attention_mask=mask, language="en")
    np.testing.assert_array_equal(plain.cpu().numpy(), F["seq_lf_greedy"])
    with pytest.raises(ValueError, match="attention_mask"):
        model.generate(lf, language="en")
    with pytest.raises(ValueError, match="return_timestamps"):
        model.generate(lf, attention_mask=mask, language="en", return_timestamps=False)
    for kw in (dict(temperature=0.2), dict(condition_on_prev_tokens=True), dict(return_token_timestamps=True), dict(logprob_threshold=-1.0)):
        with pytest.raises(ValueError, match=list(kw)[0]):
            model.generate(lf, attention_mask=mask, language="en", **kw)


@torch.no_grad()
def test_batch_equals_clips_one_at_a_time():
    F = golden("generate_timestamps.npz")
    model = _model(F)
    T = _tool()
    secs = tuple(F["lf_seconds"])
    lf, mask = _features(secs)
    full = model.generate(lf, attention_mask=mask, language="en", return_segments=True)
    for c, s in enumerate(secs):
        from mlx8_ws_audio_transformer_amd.feature_extraction import WhisperFeatureExtractor
        f = WhisperFeatureExtractor()([T.clip_audio(s, c)], sampling_rate=16000, truncation=False, padding="longest", return_tensors="pt")
        one = model.generate(f["input_features"].cuda(), language="en", return_timestamps=True, return_segments=True)
        w = one["sequences"].shape[1]
        assert full["sequences"][c, :w].tolist() == one["sequences"][0].tolist()
        assert [x["tokens"].tolist() for x in full["segments"][c]] == [x["tokens"].tolist() for x in one["segments"][0]]


@torch.no_grad()
def test_transcribe_wav_returns_the_fixture_segments(tmp_path):
    import wave
    from mlx8_ws_audio_transformer_amd.feature_extraction import WhisperProcessor
    from mlx8_ws_audio_transformer_amd.transcribe import NoteTokenizer, transcribe
    F = golden("generate_timestamps.npz")
    model = _model(F)
    T = _tool()
    audio = T.clip_audio(float(F["lf_seconds"][1]), 0)                       # clip 0's audio at the single case's length
    pcm = np.clip(np.round(audio * 32768.0), -32768, 32767).astype(np.int16)
    path = tmp_path / "memo.wav"
    with wave.open(str(path), "wb") as w:
        w.setnchannels(1); w.setsampwidth(2); w.setframerate(16000); w.writeframes(pcm.tobytes())
    proc = WhisperProcessor(tokenizer=NoteTokenizer())
    res = transcribe(model, proc, str(path), language="en")
    ref = model.generate(proc(pcm.astype(np.float32) / 32768.0, sampling_rate=16000, truncation=False, padding="longest",
                              return_tensors="pt")["input_features"].cuda(), language="en", return_segments=True)["segments"][0]
    assert res["language"] == "en" and [s["id"] for s in res["segments"]] == list(range(len(ref)))
    for s, r in zip(res["segments"], ref):
        assert s["tokens"] == [t for t in r["tokens"].tolist() if t < T.TB] and s["start"] == r["start"] and s["end"] == r["end"]
        assert s["seek"] == r["seek"] and s["text"] == proc.decode(s["tokens"])
    assert res["text"] == "".join(s["text"] for s in res["segments"])
    many = transcribe(model, proc, [str(path), audio], language="en", batch_size=2)
    assert len(many) == 2 and [s["tokens"] for s in many[0]["segments"]] == [s["tokens"] for s in res["segments"]]
