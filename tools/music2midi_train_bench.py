#!/usr/bin/env python3
"""Time of one music2midi training step on the native operators: Qwen3-0.6B's shape with seeded weights (28 layers, hidden 1024,
16 / 8 heads of 128, vocab 151936, tied), the reference's rule with the top 4 layers trained, batch 4, 512 text positions, the adapter over 1500 encoder
positions of a stub audio tower -- forward + backward + AdamW step of `MusicTranscriptionModel`, beside a torch fp32 eager restatement of the same step
(same parameters, same trainable set, torch's own scaled_dot_product_attention with the causal mask) on the same GPU.  GPU box only.

    python tools/music2midi_train_bench.py [--steps 3] [--rounds 5] [--precision bf16x3] [--layers 28] [--optimizer torch] [--out profiles/music2midi_train_bench.json]
    python tools/music2midi_train_bench.py --optim-split [--out profiles/music2midi_optim_bench.json]          

--optimizer picks what steps the native model: torch (torch.optim.AdamW, the default and section 4.13's measurement), torch_fused (torch.optim.AdamW(fused=True))
or fused (optim.FusedAdamW).  --optim-split times the native step alone, in three phases between HIP events -- re-pack of the stepped weights (what the next
forward's `_pack()` does), forward + backward, optimizer phase (global-norm clip at 1.0 + AdamW step, the reference loop's two calls) -- once per optimizer kind
on the same model in the same run: the kinds' windows alternate, medians over the rounds, max / min of the windows as the spread.  The fused phase's bytes/s
count 32 B per stepped element (4 read for the norm, 16 read and 12 written by the update) against the 6.29 TB/s a float4 copy reaches on this part.

Step times are medians over `rounds` windows of `steps` steps each, by HIP events, after a warm-up; native and torch windows alternate; max / min of the
windows is the spread.  The shader clock and package power are read from sysfs while the native step loops.  The per-kernel-class shares come from the
library's event timing (awt_prof_collect) over further native steps: events serialise the launches, so they sum kernel time, not the wall time above.

Also timed, alone: awt_op_causal_attention_backward at Lq = T = 512, 16 query heads (8 and 16 KV heads) against the non-causal
awt_op_cross_attention_backward at Lq = Sk = 512, H = 16, with the share of (query tile, key tile) pairs the causal launches visit, computed from the tile
sizes: the dq launch's workgroup of 128 queries streams 64-key tiles to its last query's diagonal (and a wave of 32 queries multiplies only to its own), the
dk / dv launch's 64-key block starts at the first 32-query tile that sees it.
"""
import argparse
import dataclasses
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.nn.functional as F

import bench
from mlx8_ws_audio_transformer_amd import CrossAttentionAdapter, _lib, ops
from mlx8_ws_audio_transformer_amd.music2midi import MusicTranscriptionModel, Qwen3Config, Qwen3Decoder
from mlx8_ws_audio_transformer_amd.optim import FusedAdamW
from music2midi_adapter_bench import TorchAdapter, medians

B, L, SA, AUDIO_DIM, K_TRAINED = 4, 512, 1500, 512, 4


def torch_decoder_loss(p, cfg, x, labels, cos, sin):
    """The decoder and HF's shifted loss in fp32 eager torch over the parameter dict p (HF names)."""
    Bx, Lx, d = x.shape
    Hq, Hkv, eps = cfg.num_attention_heads, cfg.num_key_value_heads, cfg.rms_norm_eps
    norm = lambda t, w: w * t * torch.rsqrt(t.pow(2).mean(-1, keepdim=True) + eps)
    rot = lambda t: torch.cat([t[..., :64] * cos - t[..., 64:] * sin, t[..., 64:] * cos + t[..., :64] * sin], dim=-1)
    for n in range(cfg.num_hidden_layers):
        w = lambda name: p[f"model.layers.{n}.{name}.weight"]
        h = norm(x, w("input_layernorm"))
        q = rot(norm(F.linear(h, w("self_attn.q_proj")).view(Bx, Lx, Hq, 128), w("self_attn.q_norm")).transpose(1, 2))
        k = rot(norm(F.linear(h, w("self_attn.k_proj")).view(Bx, Lx, Hkv, 128), w("self_attn.k_norm")).transpose(1, 2))
        v = F.linear(h, w("self_attn.v_proj")).view(Bx, Lx, Hkv, 128).transpose(1, 2)
        g = Hq // Hkv
        o = F.scaled_dot_product_attention(q, k.repeat_interleave(g, dim=1), v.repeat_interleave(g, dim=1), is_causal=True)
        x = x + F.linear(o.transpose(1, 2).reshape(Bx, Lx, Hq * 128), w("self_attn.o_proj"))
        h = norm(x, w("post_attention_layernorm"))
        x = x + F.linear(F.silu(F.linear(h, w("mlp.gate_proj"))) * F.linear(h, w("mlp.up_proj")), w("mlp.down_proj"))
    logits = F.linear(norm(x, p["model.norm.weight"]), p["model.embed_tokens.weight"])
    return F.cross_entropy(logits[:, :-1].reshape(-1, logits.shape[-1]), labels[:, 1:].reshape(-1), ignore_index=-100)


def visited_share(Lq, T):
    """(staged, multiplied) shares of the (query tile, key tile) pairs of the dq launch and the share of the dk / dv launch, from the tile sizes alone."""
    off = T - Lq
    nqb, nkt = -(-Lq // 128), -(-T // 64)
    staged = sum(-(-(off + min(128 * (qb + 1), Lq)) // 64) for qb in range(nqb)) / (nqb * nkt)
    waves = [min(q0 + 32, Lq) - 1 + off for q0 in range(0, Lq, 32)]
    multiplied = sum(w // 64 + 1 for w in waves) / (len(waves) * nkt)
    nkb, nqt = -(-T // 64), -(-Lq // 32)
    dkv = sum(nqt - max(64 * kb - off, 0) // 32 for kb in range(nkb)) / (nkb * nqt)
    return staged, multiplied, dkv


def make_optimizer(kind, params):
    if kind == "fused":
        return FusedAdamW(params, lr=1e-4, weight_decay=1e-4)
    return torch.optim.AdamW(params, lr=1e-4, weight_decay=1e-4, fused=True if kind == "torch_fused" else None)


COPY_BYTES_PER_S = 6.29e12          # float4 copy on this part
FUSED_BYTES_PER_ELEMENT = 32        # 4 read by the norm pass, 16 read and 12 written by the update


def optimizer_split(model, params, ids, mask, a):
    """The native step in three phases per optimizer kind (the module docstring); prints and writes one JSON line."""
    kinds = ("torch", "torch_fused", "fused")
    opts = {k: make_optimizer(k, params) for k in kinds}
    phases = ("repack_ms", "forward_backward_ms", "optimizer_ms")

    def window(kind, steps):
        opt, marks = opts[kind], []
        for _ in range(steps):
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
            ev[0].record()
            model.text_decoder._pack()
            ev[1].record()
            opt.zero_grad(set_to_none=True)
            model([None] * B, 16000, ids, mask).backward()
            ev[2].record()
            if kind == "fused":
                opt.step(max_norm=1.0)
            else:
                torch.nn.utils.clip_grad_norm_(params, 1.0)
                opt.step()
            ev[3].record()
            marks.append(ev)
        torch.cuda.synchronize()
        return [sum(ev[i].elapsed_time(ev[i + 1]) for ev in marks) / steps for i in range(3)]

    for k in kinds:
        window(k, 2)                                                       # warm-up: state, tables and the first re-pack come into being
    times = {k: [] for k in kinds}
    for _ in range(a.rounds):
        for k in kinds:
            times[k].append(window(k, a.steps))
    res, spread = {}, {}
    for k in kinds:
        cols = list(zip(*times[k]))
        res[k] = {ph: round(statistics.median(c), 4) for ph, c in zip(phases, cols)}
        res[k]["step_ms"] = round(statistics.median(sum(w) for w in times[k]), 4)
        spread[k] = {ph: round(max(c) / min(c), 3) for ph, c in zip(phases, cols)}
    elements = sum(p.numel() for p in params)
    fused_bps = FUSED_BYTES_PER_ELEMENT * elements / (res["fused"]["optimizer_ms"] * 1e-3)
    line = json.dumps({"metric": f"music2midi training step at Qwen3-0.6B's shape ({a.layers} layers, top {min(K_TRAINED, a.layers)} trained, tied head; adapter audio_dim "
                                 f"{AUDIO_DIM} over {SA} positions), B {B}, L {L}, precision {a.precision}, split by HIP events into re-pack of the stepped weights, forward + "
                                 "backward, and optimizer phase (global-norm clip at 1.0 + AdamW step), per optimizer kind on the same model in the same run (median ms over "
                                 "alternating windows)",
                       "results": res, "max_over_min_of_windows": spread, "steps": a.steps, "rounds": a.rounds,
                       "stepped_elements": elements, "stepped_tensors": len(params),
                       "fused_over_torch_optimizer_phase": round(res["fused"]["optimizer_ms"] / res["torch"]["optimizer_ms"], 4),
                       "fused_over_torch_fused_optimizer_phase": round(res["fused"]["optimizer_ms"] / res["torch_fused"]["optimizer_ms"], 4),
                       "fused_bytes_per_s_at_32B_per_element": round(fused_bps, -9), "fraction_of_float4_copy_6p29TBps": round(fused_bps / COPY_BYTES_PER_S, 4),
                       "device": torch.cuda.get_device_name(0)})
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--precision", default="bf16x3", choices=["bf16x3", "bf16"])
    ap.add_argument("--layers", type=int, default=28)
    ap.add_argument("--optimizer", default="torch", choices=["torch", "fused", "torch_fused"])
    ap.add_argument("--optim-split", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    torch.manual_seed(0)
    dev = torch.device("cuda")
    cfg = dataclasses.replace(Qwen3Config.qwen3_0_6b(), num_hidden_layers=a.layers, max_position_embeddings=L)
    dec = Qwen3Decoder(cfg, precision=a.precision, trainable_layers=min(K_TRAINED, a.layers)).to(dev)
    adapter = CrossAttentionAdapter(AUDIO_DIM, cfg.hidden_size, 8, precision=a.precision).to(dev)
    audio = torch.randn(B, SA, AUDIO_DIM, device=dev)
    model = MusicTranscriptionModel(lambda w, sr: audio, adapter, dec)
    ids = torch.randint(0, cfg.vocab_size, (B, L), device=dev)
    mask = torch.ones(B, L, dtype=torch.long, device=dev)
    trainable = [p for p in model.parameters() if p.requires_grad]
    if a.optim_split:
        return optimizer_split(model, trainable, ids, mask, a)
    opt = make_optimizer(a.optimizer, trainable)

    # the torch restatement: its own copies of every parameter, the same trainable set
    t_adapter = TorchAdapter().to(dev)
    t_adapter.load_state_dict(adapter.state_dict())
    t_params = {n: p.detach().clone().requires_grad_(p.requires_grad) for n, p in dec.named_parameters()}
    t_opt = torch.optim.AdamW([p for p in t_params.values() if p.requires_grad] + list(t_adapter.parameters()), lr=1e-4, weight_decay=1e-4)
    cos, sin = (t.to(dev)[:L] for t in dec._rope_tables(dev))

    def native_step():
        opt.zero_grad(set_to_none=True)
        loss = model([None] * B, 16000, ids, mask)
        loss.backward()
        opt.step()
        return loss

    def torch_step():
        t_opt.zero_grad(set_to_none=True)
        text = F.embedding(ids, t_params["model.embed_tokens.weight"])
        loss = torch_decoder_loss(t_params, cfg, t_adapter(text, audio), ids, cos, sin)
        loss.backward()
        t_opt.step()
        return loss

    first = (float(native_step()), float(torch_step()))                    # the two models start from the same parameters
    res, spread = medians({"native_step_ms": native_step, "torch_fp32_step_ms": torch_step}, a.steps, a.rounds, warmup=2)
    last = (float(native_step()), float(torch_step()))

    for _ in range(2 * a.steps):
        native_step()
    state = bench.read_power_sysfs(pci=bench.device_pci_address(torch, torch.cuda.current_device()))
    torch.cuda.synchronize()

    PROF_STEPS = 2
    classes_ = [c for c in _lib.PROF_CLASSES]
    _lib.prof_enable(True, classes_)
    for c in classes_:
        _lib.prof_collect(c)
    for _ in range(PROF_STEPS):
        native_step()
    torch.cuda.synchronize()
    classes = {}
    for c in classes_:
        ms, n, _ = _lib.prof_collect(c)
        if n:
            classes[c] = {"ms_per_step": round(ms / PROF_STEPS, 3), "launches_per_step": round(n / PROF_STEPS, 1)}
    _lib.prof_enable(False)
    total = sum(v["ms_per_step"] for v in classes.values())
    for v in classes.values():
        v["share"] = round(v["ms_per_step"] / total, 3)

    # ---- the causal attention backward beside the non-causal one, Lq = Sk = 512, 16 heads
    H, wq = 16, 16 * 128
    q, do = 1.7 * torch.randn(B * L, wq, device=dev), torch.randn(B * L, wq, device=dev)
    fns = {}
    k16, v16 = 1.7 * torch.randn(B * L, wq, device=dev), torch.randn(B * L, wq, device=dev)
    o, lse = ops.cross_attention((q, 0), wq, (k16, 0), wq, (v16, 0), wq, B, H, L, L, a.precision)
    dq, dk, dv = torch.empty_like(q), torch.empty_like(k16), torch.empty_like(v16)
    ws = _lib.workspace(ops.cross_attention_workspace_bytes(B, H, L, L, True), dev)
    fns["noncausal_backward_ms"] = lambda: ops.cross_attention_backward((q, 0), wq, (k16, 0), wq, (v16, 0), wq, (o, 0), (do, 0), wq, lse, (dq, 0), (dk, 0), (dv, 0),
                                                                        B, H, L, L, a.precision, workspace=ws)
    for Hkv in (16, 8):
        wkv = Hkv * 128
        kc, vc = 1.7 * torch.randn(B, L, wkv, device=dev), torch.randn(B, L, wkv, device=dev)
        oc, lsec = ops.causal_attention_lse((q, 0), wq, (kc, 0), (vc, 0), wkv, L * wkv, B, H, Hkv, L, L, a.precision)
        dkc, dvc = torch.empty_like(kc), torch.empty_like(vc)
        wsc = _lib.workspace(ops.causal_attention_backward_workspace_bytes(B, H, L, L), dev)
        fns[f"causal_backward_hkv{Hkv}_ms"] = (lambda kc=kc, vc=vc, oc=oc, lsec=lsec, dkc=dkc, dvc=dvc, wsc=wsc, wkv=wkv, Hkv=Hkv: ops.causal_attention_backward(
            (q, 0), wq, (kc, 0), (vc, 0), wkv, L * wkv, (oc, 0), (do, 0), wq, lsec, (dq, 0), (dkc, 0), (dvc, 0), wkv, L * wkv, B, H, Hkv, L, L, a.precision, workspace=wsc))
    att, att_spread = medians(fns, 20, a.rounds, warmup=3)
    staged, multiplied, dkv_share = visited_share(L, L)
    att["causal_over_noncausal_hkv16"] = round(att["causal_backward_hkv16_ms"] / att["noncausal_backward_ms"], 3)
    att["causal_over_noncausal_hkv8"] = round(att["causal_backward_hkv8_ms"] / att["noncausal_backward_ms"], 3)
    att["tile_pair_share"] = {"dq_staged": round(staged, 4), "dq_multiplied": round(multiplied, 4), "dkv": round(dkv_share, 4)}

    line = json.dumps({"metric": f"music2midi training step at Qwen3-0.6B's shape ({a.layers} layers, hidden 1024, 16 / 8 heads, vocab 151936, tied; top {min(K_TRAINED, a.layers)} "
                                 f"layers, final norm and head trained; adapter audio_dim {AUDIO_DIM} over {SA} encoder positions), B {B}, L {L}, seeded weights, precision "
                                 f"{a.precision}: forward + backward + AdamW step, native beside a torch fp32 eager restatement on the same GPU (median ms over alternating "
                                 "windows, HIP events)",
                       "results": res, "max_over_min_of_windows": spread, "steps": a.steps, "rounds": a.rounds, "native_optimizer": a.optimizer,
                       "loss_first_step_native_torch": first, "loss_last_step_native_torch": last,
                       "kernel_classes_native_step": classes,
                       "attention_backward_Lq512_T512_B4_H16": att, "attention_backward_max_over_min": att_spread,
                       "gpu_state_during_native_step": None if state is None else {"package_watts": state[0], "shader_clock_mhz": state[1], "which": state[2]},
                       "device": torch.cuda.get_device_name(0)})
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
