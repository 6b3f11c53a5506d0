"""Decode-loop timing at the Whisper-small shape without the encoder: B = 16 clips, 12 decoder layers of d 768, vocab 51 865, 1500 encoder
positions, max_length 225 (every step runs: no EOS).  Prints one JSON line:

  greedy_before  finetune.greedy_decode: per-layer caches grown by torch.cat, torch.argmax (the decode loop before generation.py)
  greedy_after   generation.greedy: preallocated cache, awt_op_select_tokens
  beam5          generation.beam_search with 5 beams (awt_op_select_tokens top-10, awt_op_kv_gather reorder)

    python tools/generate_bench.py [--steps N]
Kernel times: run it under `rocprofv3 --kernel-trace --stats -d DIR -- python tools/generate_bench.py --steps 32` and read DIR's
kernel_stats.csv (select_partial_kernel, select_final_kernel, kv_gather_kernel).
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from mlx8_ws_audio_transformer_amd import generation as G  # noqa: E402
from mlx8_ws_audio_transformer_amd.finetune import greedy_decode  # noqa: E402
from mlx8_ws_audio_transformer_amd.native_decoder import NativeWhisperDecoder  # noqa: E402


def decoder(d=768, layers=12, heads=12, ffn=3072, vocab=51865):
    torch.manual_seed(0)
    dec = NativeWhisperDecoder(d, layers, heads, ffn, vocab, 448).cuda()
    with torch.no_grad():
        for name, p in dec.named_parameters():
            if "layer_norm.weight" in name:
                p.copy_(1.0 + 0.1 * torch.randn_like(p))
            elif name.endswith("bias") or "layer_norm" in name:
                p.copy_(0.02 * torch.randn_like(p))
            elif "embed" in name:
                p.copy_((0.5 if "positions" in name else 0.1) * torch.randn_like(p))
            else:
                p.copy_(torch.randn_like(p) * (0.5 / p.shape[1] ** 0.5))
    return dec


def timed(fn, reps):
    fn()                                                                     # warm-up (packing, allocator, code objects)
    torch.cuda.synchronize()
    best = float("inf")
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        best = min(best, time.perf_counter() - t0)
    return best


@torch.no_grad()
def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=225)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--batch", type=int, default=16)
    a = ap.parse_args()
    B, S, start = a.batch, 1500, 50258
    dec = decoder()
    hidden = torch.randn((B, S, dec.d), device="cuda")
    cross = dec.cross_kv(hidden)
    init = torch.full((B, 1), start, dtype=torch.long, device="cuda")
    n = a.steps                                                              # generated tokens per clip (max_length = 1 + n)
    res = {"shape": {"B": B, "layers": dec.n_layers, "d": dec.d, "vocab": dec.vocab, "S": S, "steps": n}}
    runs = {
        "greedy_before": lambda: greedy_decode(dec, hidden, start, 50257, -1, 1 + n, cross=cross),
        "greedy_after": lambda: G.greedy(G._NativeSteps(dec, cross, S, B, 1 + n), init, 1 + n, None, 50257, None, None),
        "beam5": lambda: G.beam_search(G._NativeSteps(dec, cross, S, B, 1 + n), init, 1 + n, None, 50257, None, None, 5, 1.0, False),
    }
    for name, fn in runs.items():
        sec = timed(fn, a.reps)
        res[name] = {"ms_per_step": round(1e3 * sec / n, 4), "tokens_per_s": round(B * n / sec, 1)}
    res["beam5_over_greedy"] = round(res["beam5"]["ms_per_step"] / res["greedy_after"]["ms_per_step"], 3)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
