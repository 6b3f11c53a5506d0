"""Token-level timestamps timing at the Whisper-small shape with random weights (vocabulary layout and clips of tools/longform_bench.py):
B = 16 clips of 120 s, greedy, generate(return_timestamps=True) without and with return_token_timestamps=True, best of two runs each.
Prints one JSON line: audio seconds per second both ways (the run with the feature off is the one to compare with longform_bench's),
the seek passes and the token rows of the largest DTW.

    python tools/token_timestamps_bench.py [--clips 16] [--seconds 120]
Per-launch time of the three kernels: `rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/token_timestamps_bench.py
--kernels-only` (align_weights_kernel, align_matrix_kernel, dtw_kernel in DIR's kernel_stats.csv: 4 launches each at 16 clips x 10 heads
x 444 token rows x 1500 frames).  The host baseline the DTW kernel replaces: `--host-dtw` times HF's `_dynamic_time_warping` (or, where
transformers is not installed, its restatement generation.dtw_reference) once on a 448 x 1500 matrix, on the CPU.
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

EOS, SOT, NO_TS = 50257, 50258, 50363
ALIGNMENT_HEADS = [[5, 3], [5, 9], [8, 0], [8, 4], [8, 7], [8, 8], [9, 0], [9, 7], [9, 9], [10, 5]]      # openai/whisper-small's
GC = {"decoder_start_token_id": SOT, "eos_token_id": EOS, "pad_token_id": EOS, "max_length": 448, "no_timestamps_token_id": NO_TS,
      "lang_to_id": {"<|en|>": 50259}, "task_to_id": {"translate": 50358, "transcribe": 50359}, "is_multilingual": True,
      "suppress_tokens": [50358, 50359, 50360, 50361, 50362], "begin_suppress_tokens": [220, EOS], "alignment_heads": ALIGNMENT_HEADS}


def host_dtw():
    m = np.random.default_rng(0).standard_normal((448, 1500)).astype(np.float32).astype(np.float64)
    try:
        from transformers.models.whisper.generation_whisper import _dynamic_time_warping as fn
        name = "transformers _dynamic_time_warping"
    except ImportError:
        fn, name = G.dtw_reference, "generation.dtw_reference"
    t0 = time.perf_counter()
    fn(m)
    print(json.dumps({"host_dtw": name, "rows": 448, "frames": 1500, "seconds": round(time.perf_counter() - t0, 2)}))


def kernels_only(clips, launches=4):
    torch.manual_seed(0)
    heads, T, S, d, nl = len(ALIGNMENT_HEADS), 444, 1500, 768, 12
    align = G.Alignment(ALIGNMENT_HEADS, 7, nl, d // 64)
    q = torch.randn((len(align.layers), clips, 448, d), device="cuda")
    kv = torch.randn((clips * S, 2 * nl * d), device="cuda")
    for _ in range(launches):
        w = G.alignment_weights(q, kv, nl, S, align.table("cuda"), clips, 1, 3, T, S)
        m = G.alignment_matrix(w, align.width)
        jump = G.dtw(m)[0]
    torch.cuda.synchronize()
    print(json.dumps({"clips": clips, "heads": heads, "token_rows": T, "frames": S, "launches_each": launches, "last_jump": int(jump[0, -1])}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=16)
    ap.add_argument("--seconds", type=float, default=120.0)
    ap.add_argument("--kernels-only", action="store_true", help="only the three alignment launches on random data (for a kernel trace)")
    ap.add_argument("--host-dtw", action="store_true", help="time the host DTW once on a 448 x 1500 matrix (no GPU)")
    a = ap.parse_args()
    if a.host_dtw:
        return host_dtw()
    if a.kernels_only:
        return kernels_only(a.clips)
    from mlx8_ws_audio_transformer_amd.feature_extraction import WhisperFeatureExtractor
    from mlx8_ws_audio_transformer_amd.finetune import WhisperLoRAModel
    torch.manual_seed(0)
    model = WhisperLoRAModel(wts.config("small"), None).eval()
    model.generation_config = G.GenerationConfig.from_dict(GC)
    rng = np.random.default_rng(0)
    audio = [(0.1 * rng.standard_normal(int(a.seconds * 16000))).astype(np.float32) for _ in range(a.clips)]
    f = WhisperFeatureExtractor()(audio, sampling_rate=16000, truncation=False, padding="longest", return_attention_mask=True, return_tensors="pt")
    feats, mask = f["input_features"].cuda(), f["attention_mask"]
    rows = []
    real = G.dtw

    def dtw(matrix, *args, **kw):
        rows.append(tuple(matrix.shape))
        return real(matrix, *args, **kw)
    G.dtw = dtw

    def run(on):
        kw = {"return_token_timestamps": True} if on else {}
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = model.generate(feats, attention_mask=mask, language="en", return_timestamps=True, return_segments=True, **kw)
        torch.cuda.synchronize()
        return time.perf_counter() - t0, out

    with torch.no_grad():
        model.generate(feats[:2], attention_mask=mask[:2], language="en", return_timestamps=True, return_token_timestamps=True)      # warm-up
        rows.clear()
        off = [run(False)[0] for _ in range(2)]
        on = [run(True) for _ in range(2)]
    G.dtw = real
    total = a.clips * a.seconds
    print(json.dumps({"clips": a.clips, "seconds_per_clip": a.seconds, "audio_s_per_s_off": round(total / min(off), 1),
                      "audio_s_per_s_on": round(total / min(t for t, _ in on), 1), "wall_s_off": [round(t, 2) for t in off],
                      "wall_s_on": [round(t, 2) for t, _ in on], "dtw_calls_per_run": len(rows) // 2, "largest_dtw": list(max(rows, key=lambda r: r[1] * r[2])),
                      "token_timestamps_shape": list(on[0][1]["token_timestamps"].shape)}))


if __name__ == "__main__":
    main()
