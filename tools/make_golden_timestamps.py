"""Writes tests/golden/generate_timestamps.npz: what `WhisperForConditionalGeneration.generate(..., return_timestamps=True)` (transformers
5.15) returns, short-form and long-form (the seek loop over 30 s windows), on the mini encoder with Whisper's real window
(max_source_positions 1500: 3000 frames, 1501 timestamp tokens of 0.02 s) and a 2-layer decoder over a vocabulary laid out like Whisper's:

    text [0, 400) | eos 400 | sot 401 | <|en|> <|fr|> <|de|> 402-404 | translate 405 | transcribe 406 | startoflm 407 | startofprev 408 |
    nospeech 409 | <|notimestamps|> 410 | timestamps 411 .. 1911

    python tools/make_golden_timestamps.py [first_seed last_seed]     (default: seed 0, TS_SCALES="logit:ts:eos,..." = "25:2:1")

Audio is not stored: clip c of a case is `clip_audio(seconds, c)` (synth piano clips, tone + noise, noise).  Features come from
transformers' WhisperFeatureExtractor (`truncation=False, padding="longest", return_attention_mask=True` for long-form).
`mask_lf` / `mask_ragged` are HF's attention masks of the long-form batch and of clips of MASK_LENGTHS samples.
Per case <k>: `seq_<k>` (returned sequences), `init_<k>` (prompt), `seg_<k>` (rows clip, token begin, token end, idx0, idx1 into
`segtok_<k>`), `segtime_<k>` (float64 start, end).  Cases:
  lf_greedy   ragged batch of LF_SECONDS, language "en", greedy          lf_beam    the same, 4 beams
  lf_detect   language None (detection on the first window)             single     one 42 s clip, no attention mask
  sf_greedy   3 short clips, return_timestamps=True                     sf_beam    the same, 3 beams
  mii         lf_greedy with max_initial_timestamp_index = MII
The tool asserts what the cases exercise (see `checks`) and a margin >= GAP at every selection step, both between the k-th and
(k+1)-th candidate and |logsumexp(timestamps) - max(text)| of the timestamp rule.
"""
from __future__ import annotations

import copy
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
GOLD = os.path.join(ROOT, "tests", "golden")

from mlx8_ws_audio_transformer_amd import synth, weights as wts  # noqa: E402

EOS, SOT, NO_TS = 400, 401, 410
TB = NO_TS + 1
VOCAB = TB + 1501
LANG = {"<|en|>": 402, "<|fr|>": 403, "<|de|>": 404}
TASK = {"translate": 405, "transcribe": 406}
DEC = dict(layers=2, max_pos=64)
MAX_LEN = 24
MII = 3
LF_SECONDS = (12.3, 42.05, 78.0137)         # the longest clip is 1 248 219 samples, not a multiple of 160: the features have
                                            # n // 160 frames, HF's mask drops its last column, and the last window ends on that frame
MASK_LENGTHS = (16001, 112037, 528151)      # `mask_ragged`: HF's attention_mask for clips of these sample counts
SF_SECONDS = (4.0, 9.5, 21.0)
CONV_SCALE = 8.0
GAP = 1e-2


def clip_audio(seconds: float, c: int) -> np.ndarray:
    """float32 16 kHz audio: 4 s synth piano clips (seed 1234 + c) with a tone + noise clip and a quiet noise clip mixed in."""
    n = int(round(seconds * 16000))
    parts, i = [], 0
    while sum(len(p) for p in parts) < n:
        k = i % 4
        if k == 1:
            parts.append(synth.tone_noise_clip(c + i)[:64000].astype(np.float32))
        elif k == 3:
            parts.append((0.02 * wts.unit_variates("ts_noise", 32000, c * 100 + i)).astype(np.float32))
        else:
            parts.append(synth.pcm_i16_to_f32(synth.synth_clips_i16(1, seed=1234 + c, first=i)[0]))
        i += 1
    return np.concatenate(parts)[:n].astype(np.float32)


def generation_config_dict():
    return {"decoder_start_token_id": SOT, "eos_token_id": EOS, "pad_token_id": EOS, "bos_token_id": EOS, "max_length": MAX_LEN,
            "lang_to_id": dict(LANG), "task_to_id": dict(TASK), "no_timestamps_token_id": NO_TS, "is_multilingual": True,
            "suppress_tokens": [17, 42, SOT, 405, 406, 407, 408, 409], "begin_suppress_tokens": [220, EOS]}


def encoder_weights(cfg):
    W = wts.init_encoder_weights(cfg, seed=0, profile="test")
    for k in ("conv1.weight", "conv2.weight"):
        W[k] = W[k] * np.float32(CONV_SCALE)
    return W


def decoder_weights(cfg, seed, logit_scale, ts_scale, eos_scale):
    """weights.init_decoder_weights(seed); final LayerNorm x logit_scale; the timestamp embedding rows x ts_scale (the tied output
    projection then sets how strongly timestamps compete with text) and the EOS row x eos_scale."""
    W = wts.init_decoder_weights(cfg.d_model, DEC["layers"], cfg.ffn, VOCAB, DEC["max_pos"], seed=seed)
    for k in ("layer_norm.weight", "layer_norm.bias"):
        W[k] = W[k] * np.float32(logit_scale)
    W["embed_positions.weight"] = W["embed_positions.weight"] * np.float32(0.3)
    E = W["embed_tokens.weight"].copy()
    E[TB:] *= np.float32(ts_scale)
    E[EOS] *= np.float32(eos_scale)
    W["embed_tokens.weight"] = E
    return W


def build_model(cfg, Wd):
    from transformers import WhisperConfig, WhisperForConditionalGeneration
    hc = WhisperConfig(vocab_size=VOCAB, d_model=cfg.d_model, encoder_layers=cfg.layers, encoder_attention_heads=cfg.heads,
                       encoder_ffn_dim=cfg.ffn, num_mel_bins=cfg.n_mels, max_source_positions=cfg.max_source_positions,
                       decoder_layers=DEC["layers"], decoder_attention_heads=cfg.heads, decoder_ffn_dim=cfg.ffn,
                       max_target_positions=DEC["max_pos"], decoder_start_token_id=SOT, pad_token_id=EOS, eos_token_id=EOS, bos_token_id=EOS,
                       suppress_tokens=None, begin_suppress_tokens=None)
    hc._attn_implementation = "eager"
    model = WhisperForConditionalGeneration(hc).eval()
    sd = {"model.encoder." + k: torch.from_numpy(v) for k, v in encoder_weights(cfg).items()}
    sd.update({"model.decoder." + k: torch.from_numpy(v) for k, v in Wd.items()})
    sd["proj_out.weight"] = sd["model.decoder.embed_tokens.weight"]
    missing, unexpected = model.load_state_dict(sd, strict=True)
    assert not missing and not unexpected
    return model


def features(seconds, longform=True):
    from transformers import WhisperFeatureExtractor
    fe = WhisperFeatureExtractor()
    audio = [clip_audio(s, c) for c, s in enumerate(seconds)]
    if longform:
        f = fe(audio, sampling_rate=16000, truncation=False, padding="longest", return_attention_mask=True, return_tensors="pt")
        return f["input_features"], f["attention_mask"]
    f = fe(audio, sampling_rate=16000, return_tensors="pt")
    return f["input_features"], None


class Stats:
    """Margins of every selection step and what the timestamp rule did at non-initial steps."""

    def __init__(self):
        self.gap = float("inf")
        self.ts_margin = float("inf")
        self.fired = self.not_fired = 0
        self.max_len_hit = False

    def note_gap(self, scores, k):
        top = torch.topk(scores.float(), k + 1, dim=-1).values
        fin = torch.isfinite(top[:, k]) & (top[:, k] > -1e8)
        gaps = (top[:, k - 1] - top[:, k])[fin]
        if gaps.numel():
            self.gap = min(self.gap, float(gaps.min()))


def patched_timestamp_processor(stats):
    from transformers.generation.logits_process import WhisperTimeStampLogitsProcessor as P
    orig = P.__call__

    def call(self, input_ids, scores):
        self._detect_timestamp_from_logprob = False
        pre = orig(self, input_ids, scores)
        self._detect_timestamp_from_logprob = True
        if input_ids.shape[1] > self.begin_index:
            lse = torch.logsumexp(pre[:, self.timestamp_begin:].float(), dim=-1)
            mx = pre[:, : self.timestamp_begin].float().max(dim=-1).values
            ok = torch.isfinite(lse) & torch.isfinite(mx)
            if ok.any():
                d = (lse - mx)[ok]
                stats.ts_margin = min(stats.ts_margin, float(d.abs().min()))
                stats.fired += int((d > 0).sum())
                stats.not_fired += int((d <= 0).sum())
        return orig(self, input_ids, scores)
    return P, orig, call


def run(model, feats, mask, gc, stats, **kw):
    from transformers import GenerationConfig, LogitsProcessor, LogitsProcessorList
    g = GenerationConfig(**copy.deepcopy(gc))
    nb = kw.get("num_beams", 1)
    procs = None
    if nb == 1:
        class Rec(LogitsProcessor):
            def __call__(self, input_ids, scores):
                stats.note_gap(scores, 1)
                return scores
        procs = LogitsProcessorList([Rec()])
    orig_topk = model._get_top_k_continuations
    if nb > 1:
        def wrapped(accumulated_log_probs, *a, **k2):
            stats.note_gap(accumulated_log_probs, k2["beams_to_keep"])
            return orig_topk(accumulated_log_probs, *a, **k2)
        model._get_top_k_continuations = wrapped
    P, orig, call = patched_timestamp_processor(stats)
    P.__call__ = call
    orig_post = model._postprocess_outputs

    def post(seek_outputs, decoder_input_ids, return_token_timestamps, generation_config, *a, **k2):
        seqs = seek_outputs if isinstance(seek_outputs, torch.Tensor) else seek_outputs["sequences"]
        if seqs.shape[1] == generation_config.max_length and bool((seqs[:, -1] != EOS).any()):
            stats.max_len_hit = True                    # a row of this window ran to max_length without EOS
        return orig_post(seek_outputs, decoder_input_ids, return_token_timestamps, generation_config, *a, **k2)
    model._postprocess_outputs = post
    try:
        with torch.no_grad():
            extra = {} if mask is None else {"attention_mask": mask}
            out = model.generate(feats, generation_config=g, logits_processor=procs, return_timestamps=True, return_segments=True, **extra, **kw)
    finally:
        P.__call__ = orig
        model._get_top_k_continuations = orig_topk
        model._postprocess_outputs = orig_post
    return out


def pack(out, key, res):
    res["seq_" + key] = out["sequences"].numpy()
    rows, toks, times = [], [], []
    for c, segs in enumerate(out["segments"]):
        for s in segs:
            t = s["tokens"].tolist()
            rows.append([c, len(toks), len(toks) + len(t), int(s["idxs"][0]), int(s["idxs"][1])])
            toks += t
            times.append([float(s["start"]), float(s["end"])])
    res["seg_" + key] = np.array(rows, dtype=np.int64).reshape(-1, 5)
    res["segtok_" + key] = np.array(toks, dtype=np.int64)
    res["segtime_" + key] = np.array(times, dtype=np.float64).reshape(-1, 2)


def init_tokens(model, feats, gc, language):
    from transformers import GenerationConfig
    g = GenerationConfig(**copy.deepcopy(gc))
    g.return_timestamps = True
    model._set_language_and_task(language=language, task=None, is_multilingual=None, generation_config=g)
    return model._retrieve_init_tokens(feats, feats.shape[0], g, model.config, 3000, {}).numpy()


def attempt(cfg, seed, logit_scale, ts_scale, eos_scale):
    model = build_model(cfg, decoder_weights(cfg, seed, logit_scale, ts_scale, eos_scale))
    gc = generation_config_dict()
    st = Stats()
    res = {}
    lf, lf_mask = features(LF_SECONDS)
    sf, _ = features(SF_SECONDS, longform=False)
    one, _ = features(LF_SECONDS[1:2])
    outs = {
        "lf_greedy": run(model, lf, lf_mask, gc, st, language="en"),
        "lf_beam": run(model, lf, lf_mask, gc, st, language="en", num_beams=4),
        "lf_detect": run(model, lf, lf_mask, gc, st),
        "single": run(model, one, None, gc, st, language="en"),
        "sf_greedy": run(model, sf, None, gc, st, language="en"),
        "sf_beam": run(model, sf, None, gc, st, language="en", num_beams=3),
        "mii": run(model, lf, lf_mask, {**gc, "max_initial_timestamp_index": MII}, st, language="en"),
    }
    for k, o in outs.items():
        pack(o, k, res)
    res["init_en"] = init_tokens(model, lf, gc, "en")
    res["mask_lf"] = lf_mask.numpy()
    from transformers import WhisperFeatureExtractor
    res["mask_ragged"] = WhisperFeatureExtractor()([np.zeros(n, dtype=np.float32) for n in MASK_LENGTHS], sampling_rate=16000, truncation=False,
                                                   padding="longest", return_attention_mask=True, return_tensors="np")["attention_mask"]
    res["mask_lengths"] = np.array(MASK_LENGTHS)
    res["init_detect"] = init_tokens(model, lf, gc, None)
    # what the cases exercise
    single_end = double_split_partial = False
    for k, o in outs.items():
        for segs in o["segments"]:
            for s in segs:
                t = s["tokens"]
                if len(t) >= 2 and int(t[-1]) >= TB and int(t[-2]) < TB:
                    single_end = True
        for segs in o["segments"]:
            for a, b in zip(segs, segs[1:]):
                if len(a["tokens"]) >= 2 and int(a["tokens"][-1]) >= TB and int(a["tokens"][-2]) >= TB and b["start"] != a["end"] and \
                        (b["start"] * 100) % 3000 != 0:
                    double_split_partial = True
    n_windows = [len({round(float(s["start"]) // 30) for s in segs}) for segs in outs["lf_greedy"]["segments"]]
    ends = [max(float(s["end"]) for s in segs) if segs else 0.0 for segs in outs["lf_greedy"]["segments"]]
    checks = {
        "single-timestamp ending": single_end,
        "double-timestamp split, then a partial seek": double_split_partial,
        "timestamp rule fires at a non-initial step": st.fired > 0,
        "timestamp rule holds back at a non-initial step": st.not_fired > 0,
        "a clip leaves the batch before the others": ends[0] < ends[-1] and n_windows[-1] > 1,
        "a window stops at max_length": st.max_len_hit,
        "max_initial_timestamp_index changes a choice": not np.array_equal(res["seq_mii"], res["seq_lf_greedy"]),
        f"candidate gaps >= {GAP}": st.gap >= GAP,
        f"timestamp-rule margins >= {GAP}": st.ts_margin >= GAP,
    }
    res.update(dec_seed=np.int64(seed), logit_scale=np.float32(logit_scale), ts_scale=np.float32(ts_scale), eos_scale=np.float32(eos_scale),
               conv_scale=np.float32(CONV_SCALE), max_length=np.int64(MAX_LEN), mii=np.int64(MII), min_gap=np.float64(st.gap),
               min_ts_margin=np.float64(st.ts_margin), lf_seconds=np.array(LF_SECONDS), sf_seconds=np.array(SF_SECONDS),
               generation_config=np.array(json.dumps(gc)))
    return res, checks, st


def main():
    import transformers
    assert transformers.__version__ == "5.15.0", transformers.__version__
    cfg = wts.config("mini")
    first, last = (int(a) for a in (sys.argv[1:3] if len(sys.argv) > 2 else (0, 1)))
    scales = [tuple(float(x) for x in t.split(":")) for t in os.environ.get("TS_SCALES", "25:2:1").split(",")]
    best = None
    for seed in range(first, last):
        for logit_scale, ts_scale, eos_scale in scales:
            res, checks, st = attempt(cfg, seed, logit_scale, ts_scale, eos_scale)
            failed = [k for k, v in checks.items() if not v]
            print(f"seed {seed} logit {logit_scale} ts {ts_scale} eos {eos_scale}: gap {st.gap:.3g} ts margin {st.ts_margin:.3g} "
                  f"fired {st.fired} held {st.not_fired}", failed or "all hold", flush=True)
            if best is None or len(failed) < len(best[1]):
                best = (res, failed)
            if not failed:
                break
        if best and not best[1]:
            break
    res, failed = best
    res["unmet_checks"] = np.array(json.dumps(failed))
    if failed and not os.environ.get("TS_WRITE_ANYWAY"):
        raise SystemExit(f"no setting satisfies every check; best misses {failed} (TS_WRITE_ANYWAY=1 writes it, recording them)")
    np.savez_compressed(os.environ.get("TS_OUT", os.path.join(GOLD, "generate_timestamps.npz")), **res)
    print("timestamp fixture written:", sorted(res), "unmet:", failed)


if __name__ == "__main__":
    main()
