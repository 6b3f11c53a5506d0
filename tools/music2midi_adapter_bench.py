#!/usr/bin/env python3
"""Time of music2midi.CrossAttentionAdapter (the reference's cross-attention adapter) on the native operators at the reference's
shape -- batch 4, 512 text positions (MAX_SEQUENCE_LENGTH), 1500 encoder positions, audio_dim 512, text_dim 1024, 8 heads of 128 -- forward and
forward + backward, for the whole module and for the attention pair alone (awt_op_cross_attention / _backward).  Beside each, the same module built
from torch.nn in fp32 (attention alone: torch's scaled_dot_product_attention in fp32) on the same GPU: that is the comparison.  GPU box only.

    python tools/music2midi_adapter_bench.py [--steps 10] [--rounds 7] [--precision bf16x3] [--out profiles/music2midi_adapter_bench.json]

Every figure is the median over `rounds` windows of `steps` back-to-back calls each, by HIP events, after a warm-up of every timed shape; native and
torch windows alternate.  The shader clock and package power are read from sysfs while the native forward + backward loops.
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.nn as nn
import torch.nn.functional as F

import bench
from mlx8_ws_audio_transformer_amd import CrossAttentionAdapter, ops

B, L, SA, AUDIO_DIM, TEXT_DIM, HEADS = 4, 512, 1500, 512, 1024, 8


class TorchAdapter(nn.Module):
    """The adapter as stock torch.nn layers (the restatement of tests/music2midi_reference.py, in fp32)."""

    def __init__(self):
        super().__init__()
        self.audio_projection = nn.Linear(AUDIO_DIM, TEXT_DIM)
        self.cross_attention = nn.MultiheadAttention(TEXT_DIM, HEADS, batch_first=True)
        self.layer_norm1, self.layer_norm2 = nn.LayerNorm(TEXT_DIM), nn.LayerNorm(TEXT_DIM)
        self.feedforward = nn.Sequential(nn.Linear(TEXT_DIM, 4 * TEXT_DIM), nn.GELU(), nn.Linear(4 * TEXT_DIM, TEXT_DIM))

    def forward(self, text, audio):
        a = self.audio_projection(audio)
        t1 = self.layer_norm1(text + self.cross_attention(text, a, a, need_weights=False)[0])
        return self.layer_norm2(t1 + self.feedforward(t1))


def window(fn, steps):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    start.record()
    for _ in range(steps):
        fn()
    stop.record()
    torch.cuda.synchronize()
    return start.elapsed_time(stop) / steps


def medians(fns, steps, rounds, warmup=3):
    """{name: median ms per call}: the named callables' windows alternate, round by round."""
    for fn in fns.values():
        for _ in range(warmup):
            fn()
    times = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            times[k].append(window(fn, steps))
    return {k: round(statistics.median(v), 4) for k, v in times.items()}, {k: round(max(v) / min(v), 3) for k, v in times.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--precision", default="bf16x3", choices=["bf16x3", "bf16"])
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    torch.manual_seed(0)
    dev = torch.device("cuda")
    text, audio = torch.randn(B, L, TEXT_DIM, device=dev), torch.randn(B, SA, AUDIO_DIM, device=dev)
    d_out = torch.randn(B, L, TEXT_DIM, device=dev)
    ref = TorchAdapter().to(dev)
    nat = CrossAttentionAdapter(AUDIO_DIM, TEXT_DIM, HEADS, precision=a.precision).to(dev)
    nat.load_state_dict(ref.state_dict())

    def fwd(m):
        with torch.no_grad():
            m(text, audio)

    def fwd_bwd(m):
        for p in m.parameters():
            p.grad = None
        m(text, audio).backward(d_out)

    # the attention pair alone, on operands of the module's layout: q [B L, d], k | v in one [B Sa, 2 d] buffer
    d = TEXT_DIM
    q2, kv2, do2 = 1.7 * torch.randn(B * L, d, device=dev), 1.7 * torch.randn(B * SA, 2 * d, device=dev), torch.randn(B * L, d, device=dev)
    dq2, dkv2 = torch.empty_like(q2), torch.empty_like(kv2)
    ws_f = torch.empty(max(ops.cross_attention_workspace_bytes(B, HEADS, L, SA, False), 256), dtype=torch.uint8, device=dev)
    ws_b = torch.empty(max(ops.cross_attention_workspace_bytes(B, HEADS, L, SA, True), 256), dtype=torch.uint8, device=dev)
    o2, lse2 = torch.empty_like(q2), torch.empty(B, HEADS, L, device=dev)

    def att_fwd():
        ops.cross_attention((q2, 0), d, (kv2, 0), 2 * d, (kv2, d), 2 * d, B, HEADS, L, SA, a.precision, o=(o2, 0), ldo=d, lse=lse2, workspace=ws_f)

    def att_fwd_bwd():
        att_fwd()
        ops.cross_attention_backward((q2, 0), d, (kv2, 0), 2 * d, (kv2, d), 2 * d, (o2, 0), (do2, 0), d, lse2, (dq2, 0), (dkv2, 0), (dkv2, d), B, HEADS, L, SA,
                                     a.precision, workspace=ws_b)

    qh = q2.view(B, L, HEADS, 128).transpose(1, 2).contiguous().requires_grad_(True)
    kh = kv2[:, :d].reshape(B, SA, HEADS, 128).transpose(1, 2).contiguous().requires_grad_(True)
    vh = kv2[:, d:].reshape(B, SA, HEADS, 128).transpose(1, 2).contiguous().requires_grad_(True)
    doh = do2.view(B, L, HEADS, 128).transpose(1, 2).contiguous()

    def sdpa_fwd():
        with torch.no_grad():
            F.scaled_dot_product_attention(qh, kh, vh)

    def sdpa_fwd_bwd():
        qh.grad = kh.grad = vh.grad = None
        F.scaled_dot_product_attention(qh, kh, vh).backward(doh)

    fns = {"native_forward_ms": lambda: fwd(nat), "torch_fp32_forward_ms": lambda: fwd(ref),
           "native_forward_backward_ms": lambda: fwd_bwd(nat), "torch_fp32_forward_backward_ms": lambda: fwd_bwd(ref),
           "native_attention_forward_ms": att_fwd, "torch_fp32_sdpa_forward_ms": sdpa_fwd,
           "native_attention_forward_backward_ms": att_fwd_bwd, "torch_fp32_sdpa_forward_backward_ms": sdpa_fwd_bwd}
    res, spread = medians(fns, a.steps, a.rounds)

    # clock and power while the native training pass loops (sysfs, as bench.py reads them)
    for _ in range(3 * a.steps):
        fwd_bwd(nat)
    state = bench.read_power_sysfs(pci=bench.device_pci_address(torch, torch.cuda.current_device()))
    torch.cuda.synchronize()

    with torch.no_grad():
        parity = float((nat(text, audio) - ref(text, audio)).abs().max())
    flops_att = 4.0 * B * HEADS * L * SA * 128
    res["attention_forward_useful_TFLOP_per_s"] = round(flops_att / res["native_attention_forward_ms"] / 1e9, 1)
    line = json.dumps({"metric": f"CrossAttentionAdapter at B {B}, L {L}, Sa {SA}, audio_dim {AUDIO_DIM}, text_dim {TEXT_DIM}, {HEADS} heads, precision {a.precision}: "
                                 "native operators beside torch.nn in fp32 on the same GPU (median ms per call over alternating windows, HIP events; "
                                 "useful TFLOP/s counts 4 B H L Sa 128 once, not the split products)",
                       "results": res, "max_over_min_of_windows": spread, "steps": a.steps, "rounds": a.rounds,
                       "native_vs_torch_fp32_output_max_abs": parity,
                       "gpu_state_during_native_training_pass": None if state is None else {"package_watts": state[0], "shader_clock_mhz": state[1], "which": state[2]},
                       "device": torch.cuda.get_device_name(0)})
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
