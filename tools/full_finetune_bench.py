"""Full-parameter encoder fine-tuning, timed at the Whisper-small shape in parity mode (S = 1500) with random weights: one optimizer step of
`Seq2SeqTrainer` with `train_encoder=True` against the existing LoRA r = 8 (q_proj, v_proj) step in the same process, at B = 16 (the
reference's batch) and B = 64; the weight-gradient GEMM launches' share of the step and their achieved TFLOP/s (in-library event timing,
class "wgrad"; FLOPs counted as 2 M N K per product, whatever the split-bf16 term count); the per-step re-upload of the updated weights
(`sync_weights` after `optimizer.step()`); and the baseline the weight-gradient kernel replaces, on fc1's shape (M = 24000, N = 3072,
K = 768): two fp32 transposes plus `awt_op_linear`, as autograd_ops.Linear forms dW.  Prints one JSON line.

    python tools/full_finetune_bench.py [--batches 16,64] [--steps 3] [--warmup 2]
Per-kernel table: `rocprofv3 --kernel-trace --stats -- python tools/full_finetune_bench.py --batches 16` (wgrad_kernel / wgrad_reduce_kernel).
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from mlx8_ws_audio_transformer_amd import _lib, ops, weights as wts  # noqa: E402
from mlx8_ws_audio_transformer_amd.finetune import Seq2SeqTrainer, Seq2SeqTrainingArguments, WhisperLoRAModel  # noqa: E402


def timed(fn, warmup, iters):
    for _ in range(warmup):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def step_times(cfg, B, full, warmup, steps):
    model = WhisperLoRAModel(cfg, None if full else wts.LoraSpec(r=8, alpha=16.0), train_encoder=full)
    tr = Seq2SeqTrainer(args=Seq2SeqTrainingArguments(learning_rate=1e-5, warmup_steps=1, max_steps=1000, predict_with_generate=False), model=model)
    g = torch.Generator().manual_seed(0)
    batch = {"input_features": torch.randn((B, cfg.n_mels, cfg.n_frames), generator=g).cuda(), "labels": torch.randint(3, 1000, (B, 12), generator=g).cuda()}
    out = {"step_ms": round(timed(lambda: tr.training_step(batch), warmup, steps), 2), "trainable_params": int(tr.bucket.numel)}
    if full:
        # one more step with the weight-gradient launches event-timed, then the re-upload the next forward would do
        _lib.prof_enable(True, ["wgrad"])
        _lib.prof_collect("wgrad")
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); tr.training_step(batch); b.record()
        torch.cuda.synchronize()
        ms, n, flops = _lib.prof_collect("wgrad")
        _lib.prof_enable(False)
        out.update({"wgrad_ms": round(ms, 2), "wgrad_launch_pairs": int(n), "wgrad_share_of_step": round(ms / a.elapsed_time(b), 3),
                    "wgrad_tflops": round(flops / ms / 1e9, 1)})
        a.record(); pushed = model.encoder.sync_weights(); b.record()
        torch.cuda.synchronize()
        out.update({"reupload_ms": round(a.elapsed_time(b), 2), "reupload_tensors": int(pushed)})
        out["saved_activations_gib_per_clip"] = round(_lib.lib().awt_encoder_train_workspace_bytes(model.encoder._handle, B) / B / 2 ** 30, 3)
    del tr, model
    torch.cuda.empty_cache()
    return out


def wgrad_vs_transposes(M, N, K, warmup, iters):
    g = torch.Generator().manual_seed(1)
    dy, x = torch.randn((M, N), generator=g).cuda(), torch.randn((M, K), generator=g).cuda()
    base = timed(lambda: ops.linear(dy.t().contiguous(), x.t().contiguous(), None, "bf16x3"), warmup, iters)
    new = timed(lambda: ops.weight_grad(dy, x), warmup, iters)
    _lib.prof_enable(True, ["wgrad"])
    _lib.prof_collect("wgrad")
    got = ops.weight_grad(dy, x)
    torch.cuda.synchronize()
    ms, _, flops = _lib.prof_collect("wgrad")
    _lib.prof_enable(False)
    ref = ops.linear(dy.t().contiguous(), x.t().contiguous(), None, "bf16x3")
    return {"shape_MNK": [M, N, K], "transposes_plus_op_linear_ms": round(base, 3), "op_weight_grad_ms": round(new, 3), "kernel_pair_ms": round(ms, 3),
            "kernel_pair_tflops": round(flops / ms / 1e9, 1), "max_abs_diff_of_the_two": float((got - ref).abs().max()),
            "note": "both entries split their fp32 operands into bf16 planes inside the call; kernel_pair = wgrad_kernel + wgrad_reduce_kernel alone"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="16,64")
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    torch.manual_seed(0)
    cfg = wts.config("small")
    res = {"config": "whisper-small, parity (S = 1500), bf16x3", "fc1_weight_gradient": wgrad_vs_transposes(24000, 3072, 768, 2, 5), "steps": {}}
    for B in [int(b) for b in a.batches.split(",") if b]:
        res["steps"][str(B)] = {"full_parameter": step_times(cfg, B, True, a.warmup, a.steps), "lora_r8_qv": step_times(cfg, B, False, a.warmup, a.steps)}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
