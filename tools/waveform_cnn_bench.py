#!/usr/bin/env python3
"""Throughput of the raw-waveform CNN classifier (the reference's CNNWaveformClassifier) on the native operators at
batch 16, 4 s clips at 16 kHz: the eval forward, one training step (forward + backward + Adam), and the framed first conv alone with its
achieved output GB/s.  Beside each, the same layer list as plain torch.nn modules in fp32 on the same GPU: that is the comparison.  GPU box only.

    python tools/waveform_cnn_bench.py [--batch 16] [--steps 20] [--out profiles/waveform_cnn_bench.json]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/waveform_cnn_bench.py --conv-only      (kernel times of the two first convs)

The event timings of a single conv include the host's launch path (a wrapper call is a few tens of microseconds, the kernel about ten): the
kernel's own time, and the GB/s DESIGN.md quotes, come from the profiler run.
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.nn as nn
import torch.nn.functional as F

from mlx8_ws_audio_transformer_amd import CNNWaveformClassifier
from mlx8_ws_audio_transformer_amd.autograd_ops import native_cross_entropy
from mlx8_ws_audio_transformer_amd.waveform_classifier import WAVE_KERNEL, WAVE_STRIDE, conv1d_framed, framed_length

N_SAMPLES = 64000


def torch_model():
    """The layer list as plain torch.nn modules (the restatement of tests/test_waveform_classifier_host.py)."""
    def block(cin, cout, **conv):
        return [nn.Conv1d(cin, cout, **conv), nn.BatchNorm1d(cout), nn.ReLU(), nn.MaxPool1d(4)]
    return nn.Sequential(*block(1, 64, kernel_size=80, stride=16), *block(64, 128, kernel_size=3, padding=1),
                         *block(128, 256, kernel_size=3, padding=1), nn.AdaptiveAvgPool1d(1), nn.Flatten(), nn.Linear(256, 128), nn.ReLU(),
                         nn.Dropout(0.3), nn.Linear(128, 10))


def timed(fn, steps, warmup=3):
    """Mean milliseconds per call, by HIP events around `steps` back-to-back calls."""
    for _ in range(warmup):
        fn()
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    start.record()
    for _ in range(steps):
        fn()
    stop.record()
    torch.cuda.synchronize()
    return start.elapsed_time(stop) / steps


def bench_model(model, loss_fn, x, y, steps):
    model.eval()
    with torch.no_grad():
        ev = timed(lambda: model(x), steps)
    model.train()
    opt = torch.optim.Adam(model.parameters(), lr=3e-4, weight_decay=1e-4)

    def step():
        opt.zero_grad()
        loss_fn(model(x), y).backward()
        opt.step()
    return ev, timed(step, steps)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--conv-only", action="store_true", help="only the first conv, native and torch, 200 calls each (for a profiler run)")
    a = ap.parse_args()
    torch.manual_seed(0)
    B = a.batch
    x = 0.5 * torch.randn(B, 1, N_SAMPLES, device="cuda")
    y = torch.randint(0, 10, (B,), device="cuda")
    t1 = framed_length(N_SAMPLES, WAVE_KERNEL, WAVE_STRIDE)
    out_bytes, in_bytes = B * t1 * 64 * 4, B * N_SAMPLES * 4
    res = {"batch": B, "n_samples": N_SAMPLES, "frames": [t1, t1 // 4, t1 // 16, t1 // 64]}

    if a.conv_only:
        nat, ref = CNNWaveformClassifier().cuda(), torch_model().cuda()
        w, b, x2 = nat.conv_layers[0].weight.detach(), nat.conv_layers[0].bias.detach(), x[:, 0].contiguous()
        print("native wrapper call, us:", round(timed(lambda: conv1d_framed(x2, w, b, WAVE_STRIDE), 200, warmup=10) * 1e3, 2))
        with torch.no_grad():
            print("torch first conv call, us:", round(timed(lambda: ref[0](x), 200, warmup=10) * 1e3, 2))
        return

    nat = CNNWaveformClassifier().cuda()
    ev, tr = bench_model(nat, native_cross_entropy, x, y, a.steps)
    w, b, x2 = nat.conv_layers[0].weight.detach(), nat.conv_layers[0].bias.detach(), x[:, 0].contiguous()
    cv = timed(lambda: conv1d_framed(x2, w, b, WAVE_STRIDE), 10 * a.steps, warmup=10)
    res["native"] = {"eval_ms_per_batch": round(ev, 4), "eval_clips_per_s": round(B / ev * 1e3, 1), "train_ms_per_step": round(tr, 4),
                     "train_clips_per_s": round(B / tr * 1e3, 1), "framed_conv_us": round(cv * 1e3, 2),
                     "framed_conv_output_GB_per_s": round(out_bytes / cv / 1e6, 1),
                     "framed_conv_input_plus_output_GB_per_s": round((out_bytes + in_bytes) / cv / 1e6, 1)}
    try:
        ref = torch_model().cuda()
        ev, tr = bench_model(ref, F.cross_entropy, x, y, a.steps)
        conv = ref[0]
        with torch.no_grad():
            cv = timed(lambda: conv(x), 10 * a.steps, warmup=10)
        res["torch_fp32"] = {"eval_ms_per_batch": round(ev, 4), "eval_clips_per_s": round(B / ev * 1e3, 1), "train_ms_per_step": round(tr, 4),
                             "train_clips_per_s": round(B / tr * 1e3, 1), "first_conv_us": round(cv * 1e3, 2),
                             "first_conv_output_GB_per_s": round(out_bytes / cv / 1e6, 1)}
    except Exception as e:       # torch's own conv backend may be unusable on a box without its kernel database: the native figures still stand
        res["torch_fp32"] = {"error": f"{type(e).__name__}: {e}"[:300]}
    line = json.dumps({"metric": "CNNWaveformClassifier, batch of 4 s clips at 16 kHz: native operators beside plain torch.nn in fp32 on the same GPU "
                                 "(ms by HIP events; framed conv output = B x 3996 x 64 fp32)", "results": res})
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
