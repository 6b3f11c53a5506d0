"""Long-form transcription timing at the Whisper-small shape with random weights and Whisper's vocabulary layout (eos 50257, sot 50258,
<|en|> 50259, transcribe 50359, <|notimestamps|> 50363, timestamps from 50364): B = 16 clips of 120 s, greedy, the seek loop of
generate(return_timestamps=True).  Prints one JSON line: audio seconds per second, seek passes, and ms per greedy decode step at B = 16
without and with the timestamp rules (generation.greedy on random encoder states, every step runs).

    python tools/longform_bench.py [--clips 16] [--seconds 120] [--steps 64]
Selection share: `rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/longform_bench.py --decode-only` and read
DIR's kernel_stats.csv (select_partial_kernel / select_final_kernel against the whole; 2 x steps greedy steps are traced).
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from mlx8_ws_audio_transformer_amd import generation as G, weights as wts  # noqa: E402
from mlx8_ws_audio_transformer_amd.feature_extraction import WhisperFeatureExtractor  # noqa: E402
from mlx8_ws_audio_transformer_amd.finetune import WhisperLoRAModel  # noqa: E402

EOS, SOT, NO_TS = 50257, 50258, 50363
GC = {"decoder_start_token_id": SOT, "eos_token_id": EOS, "pad_token_id": EOS, "max_length": 448, "no_timestamps_token_id": NO_TS,
      "lang_to_id": {"<|en|>": 50259}, "task_to_id": {"translate": 50358, "transcribe": 50359}, "is_multilingual": True,
      "suppress_tokens": [50358, 50359, 50360, 50361, 50362], "begin_suppress_tokens": [220, EOS]}


def step_ms(model, B, steps, rules):
    hidden = torch.randn((B, 1500, 768), device="cuda")
    cross = model.decoder.cross_kv(hidden, model.precision)
    init = torch.tensor([[SOT, 50259, 50359]] * B, device="cuda")
    times = []
    for _ in range(2):
        steps_obj = model._decode_steps(hidden, cross, B, init.shape[1] + steps)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        G.greedy(steps_obj, init, init.shape[1] + steps, None, EOS, None, None, rules)     # no EOS: every step runs
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3 / steps)
    return min(times)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=16)
    ap.add_argument("--seconds", type=float, default=120.0)
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--decode-only", action="store_true", help="only the greedy steps with the timestamp rules (for a kernel trace)")
    a = ap.parse_args()
    torch.manual_seed(0)
    model = WhisperLoRAModel(wts.config("small"), None).eval()
    model.generation_config = G.GenerationConfig.from_dict(GC)
    if a.decode_only:
        with torch.no_grad():
            ms = step_ms(model, a.clips, a.steps, G.TimestampRules(EOS, NO_TS, 3))
        print(json.dumps({"clips": a.clips, "steps": a.steps, "greedy_step_ms_with_rules": round(ms, 3)}))
        return
    rng = np.random.default_rng(0)
    audio = [(0.1 * rng.standard_normal(int(a.seconds * 16000))).astype(np.float32) for _ in range(a.clips)]
    f = WhisperFeatureExtractor()(audio, sampling_rate=16000, truncation=False, padding="longest", return_attention_mask=True, return_tensors="pt")
    feats = f["input_features"].cuda()
    passes = []
    orig = G.longform_generate

    def counting(*args, **kw):
        decode = args[7]

        def dec(seg, init, max_len):
            passes.append(seg.shape[0])
            return decode(seg, init, max_len)
        return orig(*args[:7], dec, *args[8:], **kw)
    G.longform_generate = counting
    with torch.no_grad():
        model.generate(feats[:2], attention_mask=f["attention_mask"][:2], language="en")           # warm-up
        passes.clear()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = model.generate(feats, attention_mask=f["attention_mask"], language="en", return_segments=True)
        torch.cuda.synchronize()
        wall = time.perf_counter() - t0
        rules = G.TimestampRules(EOS, NO_TS, 3)
        plain, ts = step_ms(model, a.clips, a.steps, None), step_ms(model, a.clips, a.steps, rules)
    G.longform_generate = orig
    print(json.dumps({"clips": a.clips, "seconds_per_clip": a.seconds, "audio_s_per_s": round(a.clips * a.seconds / wall, 1), "wall_s": round(wall, 2),
                      "passes": len(passes), "segments": sum(len(s) for s in out["segments"]), "greedy_step_ms": round(plain, 3),
                      "greedy_step_ms_with_rules": round(ts, 3)}))


if __name__ == "__main__":
    main()
