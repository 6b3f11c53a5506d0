"""Writes tests/golden/token_timestamps.npz and tests/golden/token_timestamps_<case>.npz: what transformers 5.15
`WhisperForConditionalGeneration.generate(..., return_timestamps=True, return_token_timestamps=True, return_segments=True)` returns on the
mini model of tools/make_golden_timestamps.py (imported: same encoder with the real 3000-frame window, 2-layer decoder with 2 heads of 64,
Whisper-layout vocabulary, `clip_audio`, SF_SECONDS, LF_SECONDS), with `alignment_heads = [[0, 1], [1, 0], [1, 1]]` and
`median_filter_width = 7`.

    python tools/make_golden_token_timestamps.py [first_seed last_seed]     (default: seed 0, TS_SCALES="logit:ts:eos,..." = "25:2:1")

Cases (language "en"): sf_greedy, sf_beam (3 beams): the 3 short clips, no attention mask (num_frames None: 1500 frames);
lf_greedy, lf_beam (4 beams): the ragged long-form batch with HF's attention mask (per-window num_frames, cropped matrices).

token_timestamps.npz, per case <k>: `seq_<k>`, `tts_<k>` (HF's padded token_timestamps), `seg_<k>` (rows clip, begin, end into
`segtts_<k>`, the segments' token_timestamps concatenated, float64 of HF's values; `segtime_<k>` their start, end), `ncalls_<k>` and per decode call c of the seek loop
`call_<k>_<c>_seq` / `call_<k>_<c>_tts` (what generate returned for the window, prompt included, and what `_extract_token_timestamps`
returned for it) and `call_<k>_<c>_frames` (num_frames of the window's clips, -1 = None), `matrix_sens_<k>`, and `dtw_<k>` (rows: decode
call, clip within the call, token rows, frames, stable).  `weights_pair_w` / `weights_pair_m`: for the narrowest window of lf_greedy
the cropped weights [heads, tokens, frames] that went into the z-score and the matrix HF's DTW got for them (its negative is stored DTW
input).  The DTW calls themselves (wrapping `generation_whisper._dynamic_time_warping`) are in token_timestamps_<k>.npz, per call n:
`m<n>` (the float64 input stored as float32, which it is), `text<n>`, `time<n>` (HF's text_indices / time_indices).  They live in one
file per case because all 24 matrices together (about 3 MB, float32 z-scores do not compress) exceed what one committed file may hold;
no window is left out.

Two robustness fields size the GPU tests' bounds from the reference's own behaviour:
  matrix_sens_<k>  the largest change of any DTW input of the case over SENS_DRAWS seeded draws of Gaussian noise added to HF's encoder
                   output, scaled to max-abs ENC_ERR = 1.1e-4 (this project's measured encoder error, README.md); draws whose tokens
                   differ from the clean run are an error (the margins below forbid it);
  stable           per DTW call: HF's jump frames do not change under STABLE_DRAWS seeded perturbations of the input drawn uniformly from
                   [-eps, +eps], eps = 4 x matrix_sens_<k>.
The tool asserts what the cases exercise (`checks`; a property no searched seed shows is recorded in `unmet_checks`), at least two
stable windows in every case and a third of all, and the candidate-gap / timestamp-rule margins >= GAP of the timestamp tool.
"""
from __future__ import annotations

import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden_timestamps as T  # noqa: E402

ALIGNMENT_HEADS = [[0, 1], [1, 0], [1, 1]]
MEDIAN_WIDTH = 7
ENC_ERR = 1.1e-4
SENS_DRAWS = 8
STABLE_DRAWS = 16
CASES = {"sf_greedy": dict(longform=False), "sf_beam": dict(longform=False, num_beams=3), "lf_greedy": dict(longform=True),
         "lf_beam": dict(longform=True, num_beams=4)}


def jump_frames(text_indices, time_indices):
    jumps = np.pad(np.diff(text_indices), (1, 0), constant_values=1).astype(bool)
    return time_indices[jumps]


class Recorder:
    """Wraps `_dynamic_time_warping` and the model's `_extract_token_timestamps` for one generate call."""

    def __init__(self, model, keep_weights=False):
        self.model, self.keep_weights = model, keep_weights
        self.dtw, self.calls, self.weights = [], [], []

    def __enter__(self):
        from transformers.models.whisper import generation_whisper as GW
        self.GW, self.orig_dtw, self.orig_ext = GW, GW._dynamic_time_warping, self.model._extract_token_timestamps

        def dtw(matrix):
            text, time = self.orig_dtw(matrix)
            self.dtw.append(dict(call=len(self.calls), clip=len([d for d in self.dtw if d["call"] == len(self.calls)]),
                                 m=np.asarray(matrix), text=np.asarray(text), time=np.asarray(time)))
            return text, time

        def extract(generate_outputs, alignment_heads, time_precision=0.02, num_frames=None, num_input_ids=None):
            out = self.orig_ext(generate_outputs, alignment_heads, time_precision=time_precision, num_frames=num_frames, num_input_ids=num_input_ids)
            bi = generate_outputs.get("beam_indices") if hasattr(generate_outputs, "get") else None
            nf = None if num_frames is None else np.asarray(num_frames).astype(np.int64)
            if self.keep_weights and bi is None and nf is not None:
                cross = [torch.cat([x[i] for x in generate_outputs.cross_attentions], dim=2) for i in range(self.model.config.decoder_layers)]
                w = torch.stack([cross[l][:, h] for l, h in alignment_heads]).permute([1, 0, 2, 3])[:, :, num_input_ids:, :]
                for b in range(w.shape[0]):
                    self.weights.append(dict(call=len(self.calls), clip=b, w=w[b, ..., : int(nf[b]) // 2].clone().numpy()))
            self.calls.append(dict(seq=generate_outputs["sequences"].clone().numpy(), tts=out.clone().numpy(), frames=nf,
                                   beam_indices=None if bi is None else bi.clone().numpy(), P=int(num_input_ids)))
            return out

        GW._dynamic_time_warping = dtw
        self.model._extract_token_timestamps = extract
        return self

    def __exit__(self, *exc):
        self.GW._dynamic_time_warping = self.orig_dtw
        del self.model._extract_token_timestamps
        return False


def encoder_noise(model, seed):
    """Forward hook on HF's encoder: adds Gaussian noise of max-abs ENC_ERR to its output, a fresh draw of the seeded stream per call."""
    gen = torch.Generator().manual_seed(seed)

    def hook(module, inputs, output):
        h = output.last_hidden_state
        n = torch.randn(h.shape, generator=gen, dtype=h.dtype)
        h.add_(n * (ENC_ERR / float(n.abs().max())))
        return output
    return model.model.encoder.register_forward_hook(hook)


def generate(model, feats, mask, gc, stats, kw, keep_weights=False):
    with Recorder(model, keep_weights) as rec:
        out = T.run(model, feats, mask, gc, stats, language="en", return_token_timestamps=True, **kw)
    return out, rec


def attempt(cfg, seed, logit_scale, ts_scale, eos_scale):
    model = T.build_model(cfg, T.decoder_weights(cfg, seed, logit_scale, ts_scale, eos_scale))
    model.config.median_filter_width = MEDIAN_WIDTH
    gc = {**T.generation_config_dict(), "alignment_heads": ALIGNMENT_HEADS}
    st = T.Stats()
    lf, lf_mask = T.features(T.LF_SECONDS)
    sf, _ = T.features(T.SF_SECONDS, longform=False)
    res, mats = {}, {}
    seen = dict(early_beam=False, early_greedy=False, ragged=False, equal=False, several_cells=False, shared_frame=False)
    stable_counts = {}
    for key, spec in CASES.items():
        feats, mask = (lf, lf_mask) if spec["longform"] else (sf, None)
        kw = {k: v for k, v in spec.items() if k != "longform"}
        out, rec = generate(model, feats, mask, gc, st, kw, keep_weights=key == "lf_greedy")
        assert out["token_timestamps"].shape == out["sequences"].shape, key
        res["seq_" + key] = out["sequences"].numpy()
        res["tts_" + key] = out["token_timestamps"].numpy()
        rows, vals, times = [], [], []
        for c, segs in enumerate(out["segments"]):
            for s in segs:
                v = s["token_timestamps"].double().tolist()
                assert len(v) == len(s["tokens"]), key
                rows.append([c, len(vals), len(vals) + len(v)])
                vals += v
                times.append([float(s["start"]), float(s["end"])])
        res["seg_" + key] = np.array(rows, dtype=np.int64).reshape(-1, 3)
        res["segtts_" + key] = np.array(vals, dtype=np.float64)
        res["segtime_" + key] = np.array(times, dtype=np.float64).reshape(-1, 2)
        res["ncalls_" + key] = np.int64(len(rec.calls))
        for c, call in enumerate(rec.calls):
            res[f"call_{key}_{c}_seq"] = call["seq"]
            res[f"call_{key}_{c}_tts"] = call["tts"]
            res[f"call_{key}_{c}_frames"] = np.full(call["seq"].shape[0], -1, dtype=np.int64) if call["frames"] is None else call["frames"]
            nf = call["frames"]
            if nf is not None and len(nf) > 1:
                seen["ragged" if len(np.unique(nf)) > 1 else "equal"] = True
            if nf is None:
                seen["equal"] = True
            bi, P = call["beam_indices"], call["P"]
            if bi is not None:
                live = (bi != -1).sum(-1)
                seen["early_beam"] |= bool(len(live) > 1 and live.min() < live.max())
            else:
                gen = call["seq"][:, P:]
                ends = [int(np.argmax(r == T.EOS)) if (r == T.EOS).any() else len(r) for r in gen]
                seen["early_greedy"] |= bool(len(ends) > 1 and min(ends) < max(ends) - 1)
        # sensitivity of HF's own DTW input to encoder noise of this project's size
        sens = 0.0
        for draw in range(SENS_DRAWS):
            h = encoder_noise(model, 1000 * (1 + draw) + len(key))
            try:
                out2, rec2 = generate(model, feats, mask, gc, T.Stats(), kw)
            finally:
                h.remove()
            assert np.array_equal(out2["sequences"].numpy(), res["seq_" + key]) and len(rec2.dtw) == len(rec.dtw), f"{key}: noise draw {draw} changed the tokens"
            for a, b in zip(rec.dtw, rec2.dtw):
                assert a["m"].shape == b["m"].shape, key
                sens = max(sens, float(np.abs(a["m"] - b["m"]).max()))
        res["matrix_sens_" + key] = np.float64(sens)
        eps = 4.0 * sens
        meta, case_mats, stable = [], {}, 0
        for n, d in enumerate(rec.dtw):
            m32 = d["m"].astype(np.float32)
            assert np.array_equal(m32.astype(np.float64), d["m"]), "the DTW input is float32 data"
            base = jump_frames(d["text"], d["time"])
            rng = np.random.default_rng([seed, list(CASES).index(key), n])
            ok = True
            for _ in range(STABLE_DRAWS):
                p = (d["m"] + rng.uniform(-eps, eps, size=d["m"].shape)).astype(np.float32).astype(np.float64)
                ok &= np.array_equal(jump_frames(*rec.orig_dtw(p)), base)
                if not ok:
                    break
            stable += int(ok)
            meta.append([d["call"], d["clip"], m32.shape[0], m32.shape[1], int(ok)])
            case_mats[f"m{n}"], case_mats[f"text{n}"], case_mats[f"time{n}"] = m32, d["text"].astype(np.int32), d["time"].astype(np.int32)
            counts = np.bincount(d["text"])
            seen["several_cells"] |= bool((counts > 1).any())
            seen["shared_frame"] |= bool((np.diff(d["time"]) == 0).any())
        res["dtw_" + key] = np.array(meta, dtype=np.int64).reshape(-1, 5)
        mats[key] = case_mats
        stable_counts[key] = (stable, len(rec.dtw))
        if key == "lf_greedy":
            w = min(rec.weights, key=lambda x: x["w"].shape[-1])
            d = next(d for d in rec.dtw if d["call"] == w["call"] and d["clip"] == w["clip"])
            assert d["m"].shape == w["w"].shape[1:], (d["m"].shape, w["w"].shape)
            res["weights_pair_w"], res["weights_pair_m"] = w["w"].astype(np.float32), (-d["m"]).astype(np.float32)
        print(f"  {key}: {len(rec.calls)} decode calls, {len(rec.dtw)} DTW calls, rows {sorted({m[2] for m in meta})}, frames {sorted({m[3] for m in meta})}, "
              f"matrix_sens {sens:.3g}, stable {stable}", flush=True)
    total = sum(n for _, n in stable_counts.values())
    checks = {
        "a beam hypothesis ends before the longest of its decode call": seen["early_beam"],
        "a greedy row finishes before the others": seen["early_greedy"],
        "a window with ragged num_frames": seen["ragged"],
        "a window with equal num_frames": seen["equal"],
        "a token row with several path cells": seen["several_cells"],
        "a frame shared by two tokens": seen["shared_frame"],
        "two stable windows in every case": all(s >= 2 for s, _ in stable_counts.values()),
        "a third of all windows stable": 3 * sum(s for s, _ in stable_counts.values()) >= total,
        f"candidate gaps >= {T.GAP}": st.gap >= T.GAP,
        f"timestamp-rule margins >= {T.GAP}": st.ts_margin >= T.GAP,
    }
    res.update(dec_seed=np.int64(seed), logit_scale=np.float32(logit_scale), ts_scale=np.float32(ts_scale), eos_scale=np.float32(eos_scale),
               min_gap=np.float64(st.gap), min_ts_margin=np.float64(st.ts_margin), lf_seconds=np.array(T.LF_SECONDS), sf_seconds=np.array(T.SF_SECONDS),
               mask_lf=lf_mask.numpy(), alignment_heads=np.array(ALIGNMENT_HEADS, dtype=np.int64), median_filter_width=np.int64(MEDIAN_WIDTH),
               enc_err=np.float64(ENC_ERR), init_en=T.init_tokens(model, lf, gc, "en"), max_length=np.int64(T.MAX_LEN),
               max_target_positions=np.int64(T.DEC["max_pos"]), generation_config=np.array(json.dumps(gc)), cases=np.array(json.dumps(list(CASES))))
    return res, mats, checks, st


def main():
    import transformers
    assert transformers.__version__ == "5.15.0", transformers.__version__
    cfg = T.wts.config("mini")
    first, last = (int(a) for a in (sys.argv[1:3] if len(sys.argv) > 2 else (0, 1)))
    scales = [tuple(float(x) for x in t.split(":")) for t in os.environ.get("TS_SCALES", "25:2:1").split(",")]
    best = None
    for seed in range(first, last):
        for logit_scale, ts_scale, eos_scale in scales:
            print(f"seed {seed} logit {logit_scale} ts {ts_scale} eos {eos_scale}", flush=True)
            res, mats, checks, st = attempt(cfg, seed, logit_scale, ts_scale, eos_scale)
            failed = [k for k, v in checks.items() if not v]
            print(f"  gap {st.gap:.3g} ts margin {st.ts_margin:.3g}", failed or "all hold", flush=True)
            if best is None or len(failed) < len(best[2]):
                best = (res, mats, failed)
            if not failed:
                break
        if best and not best[2]:
            break
    res, mats, failed = best
    res["unmet_checks"] = np.array(json.dumps(failed))
    if failed and not os.environ.get("TS_WRITE_ANYWAY"):
        raise SystemExit(f"no setting satisfies every check; best misses {failed} (TS_WRITE_ANYWAY=1 writes it, recording them)")
    out = os.environ.get("TS_OUT", os.path.join(T.GOLD, "token_timestamps.npz"))
    np.savez_compressed(out, **res)
    for key, m in mats.items():
        np.savez_compressed(out[: -len(".npz")] + f"_{key}.npz", **m)
    print("token timestamp fixture written:", len(res), "arrays; unmet:", failed)


if __name__ == "__main__":
    main()
