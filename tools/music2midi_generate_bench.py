#!/usr/bin/env python3
"""Time of music2midi's inference path at Qwen3-0.6B's shape on one MI355X, seeded weights: `MusicTranscriptionModel.generate`
(adapter on the new token, KV cache, native operators) and `Qwen3Decoder.prefill`, each beside a plain-torch fp32 restatement on the same GPU that does
what the reference does -- per generated token the audio is re-projected, the adapter runs over the whole text and all 28 layers run over the whole
sequence without a cache (.charles/music2midi/model.py:314-341).  GPU box only.

    python tools/music2midi_generate_bench.py [--tokens 256] [--rounds 3] [--precision bf16x3] [--batch 1,8] [--parent-json FILE]
                                              [--out profiles/music2midi_generate_bench.json]
    python tools/music2midi_generate_bench.py --trace-run      # the native generate alone, 64 tokens: the run to put under a kernel tracer

  generate   ms per generated token at batch 1 over `tokens` greedy tokens from one start token (EOS never matches, so every run has the full length)
  batch      `--batch 1,8` (the default): beside batch 1, `generate_batch` of 8 clips (distinct audio, the same start token) as ms per step and clips x tokens / s
  prefill    ms for a 512-token prefill at B = 4: native `prefill` (last position's logits) / the torch decoder's full forward
  parent     `--parent-json FILE`: the output line of the same command on the parent commit, on the same GPU; it is copied into the result, and the batch-1
             figure is judged against it: lower by more than the larger max / min window spread of the two runs, or not
Every figure is the median over `rounds` windows; native and torch windows alternate.  Where the time goes at Lq = 1 comes from the library's own event
timing of its kernel classes (awt_prof_enable) over 16 further steps at the end of a 256-position cache, as ms per token and launches per token.
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.nn.functional as F

import bench
from mlx8_ws_audio_transformer_amd import CrossAttentionAdapter, MusicTranscriptionModel, Qwen3Cache, Qwen3Config, Qwen3Decoder, _lib
from tools.music2midi_adapter_bench import TorchAdapter, AUDIO_DIM, SA

PREFILL_B, PREFILL_L = 4, 512


def rms(x, w, eps):
    return w * (x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + eps))


def rotate(x, cos, sin):
    a, b = x[..., :64], x[..., 64:]
    return torch.cat([a * cos - b * sin, b * cos + a * sin], dim=-1)


def torch_decoder(sd, c, x):
    """Qwen3 over inputs_embeds x [B, L, hidden] in fp32 torch, no cache: logits [B, L, vocab]."""
    B, L, _ = x.shape
    Hq, Hkv, eps = c.num_attention_heads, c.num_key_value_heads, c.rms_norm_eps
    inv_freq = 1.0 / (c.rope_theta ** (torch.arange(0, 128, 2, device=x.device, dtype=torch.float32) / 128))
    ang = torch.arange(L, device=x.device, dtype=torch.float32)[:, None] * inv_freq[None, :]
    cos, sin = ang.cos()[None, None], ang.sin()[None, None]
    for n in range(c.num_hidden_layers):
        p = f"model.layers.{n}."
        h = rms(x, sd[p + "input_layernorm.weight"], eps)
        heads = lambda t, H: t.view(B, L, H, 128).transpose(1, 2)
        q = rotate(rms(heads(F.linear(h, sd[p + "self_attn.q_proj.weight"]), Hq), sd[p + "self_attn.q_norm.weight"], eps), cos, sin)
        k = rotate(rms(heads(F.linear(h, sd[p + "self_attn.k_proj.weight"]), Hkv), sd[p + "self_attn.k_norm.weight"], eps), cos, sin)
        v = heads(F.linear(h, sd[p + "self_attn.v_proj.weight"]), Hkv)
        o = F.scaled_dot_product_attention(q, k.repeat_interleave(Hq // Hkv, dim=1), v.repeat_interleave(Hq // Hkv, dim=1), is_causal=True)
        x = x + F.linear(o.transpose(1, 2).reshape(B, L, Hq * 128), sd[p + "self_attn.o_proj.weight"])
        h = rms(x, sd[p + "post_attention_layernorm.weight"], eps)
        x = x + F.linear(F.silu(F.linear(h, sd[p + "mlp.gate_proj.weight"])) * F.linear(h, sd[p + "mlp.up_proj.weight"]), sd[p + "mlp.down_proj.weight"])
    head = sd["model.embed_tokens.weight"] if c.tie_word_embeddings else sd["lm_head.weight"]
    return F.linear(rms(x, sd["model.norm.weight"], eps), head)


@torch.no_grad()
def torch_generate(sd, c, adapter, audio, start, tokens):
    """The reference's loop (argmax for its multinomial): everything recomputed for every token."""
    ids = torch.tensor([[start]], device=audio.device)
    for _ in range(tokens):
        fused = adapter(sd["model.embed_tokens.weight"][ids], audio)
        nxt = torch_decoder(sd, c, fused)[:, -1].argmax(-1, keepdim=True)
        nxt.item()                                                         # the reference reads every token back for its EOS test
        ids = torch.cat([ids, nxt], dim=1)
    return ids[0, 1:].tolist()


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tokens", type=int, default=256)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--precision", default="bf16x3", choices=["bf16x3", "bf16"])
    ap.add_argument("--trace-run", action="store_true")
    ap.add_argument("--batch", default="1,8", help="batch sizes of the native generate: 1 is always run; each further size B runs generate_batch on B clips")
    ap.add_argument("--parent-json", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    torch.manual_seed(0)
    dev = torch.device("cuda")
    cfg = Qwen3Config.qwen3_0_6b()
    dec = Qwen3Decoder(cfg, precision=a.precision).to(dev).eval()
    ref_adapter = TorchAdapter().to(dev).eval()
    adapter = CrossAttentionAdapter(AUDIO_DIM, cfg.hidden_size, 8, precision=a.precision).to(dev).eval()
    adapter.load_state_dict(ref_adapter.state_dict())
    audio = torch.randn(1, SA, AUDIO_DIM, device=dev)
    batches = sorted({int(b) for b in a.batch.split(",")} - {1})
    more = torch.randn(max(batches + [1]) - 1, SA, AUDIO_DIM, device=dev, generator=torch.Generator(device=dev).manual_seed(1))   # the other clips' audio: its own generator
    clips = torch.cat([audio, more])
    model = MusicTranscriptionModel(lambda w, sr: clips[:len(w)], adapter, dec)
    sd = dict(dec.state_dict())
    start = 1
    native_gen = lambda n=a.tokens: model.generate(None, 16000, max_new_tokens=n, do_sample=False, bos_token_id=start, eos_token_id=-1)
    if a.trace_run:
        native_gen(8)
        print("generated", len(native_gen(64)), "tokens")
        return
    x = torch.randn(PREFILL_B, PREFILL_L, cfg.hidden_size, device=dev)

    def native_prefill():
        with torch.no_grad():
            return dec.prefill(x, Qwen3Cache(cfg, PREFILL_B, PREFILL_L, dev))

    def torch_prefill():
        with torch.no_grad():
            return torch_decoder(sd, cfg, x)[:, -1]

    fns = {"native_generate_ms_per_token": (native_gen, a.tokens), "torch_fp32_full_recompute_generate_ms_per_token": (lambda: torch_generate(sd, cfg, ref_adapter, audio, start, a.tokens), a.tokens),
           "native_prefill_ms": (native_prefill, 1), "torch_fp32_prefill_ms": (torch_prefill, 1)}
    batch_gen = lambda B, n=a.tokens: model.generate_batch([None] * B, 16000, max_new_tokens=n, do_sample=False, bos_token_id=start, eos_token_id=-1)
    for B in batches:
        fns[f"native_generate_batch{B}_ms_per_step"] = (lambda B=B: batch_gen(B), a.tokens)
        batch_gen(B, 8)
    native_gen(8), torch_generate(sd, cfg, ref_adapter, audio, start, 8), native_prefill(), torch_prefill()          # warm-up of every timed shape ...
    outs, times = {}, {k: [] for k in fns}
    for r in range(a.rounds + 1):                                          # ... and one untimed round at full length
        for k, (fn, per) in fns.items():
            ms, outs[k] = timed(fn)
            if r:
                times[k].append(ms / per)
    res = {k: round(statistics.median(v), 4) for k, v in times.items()}
    spread = {k: round(max(v) / min(v), 3) for k, v in times.items()}

    # where a generated token's time goes at Lq = 1: the library's event timing of its kernel classes over PROF_STEPS steps (adapter on one token, decoder
    # step, argmax) at the END of a 256-position cache, i.e. at the longest key length of the run above (events serialise the launches, so the sum is
    # kernel time, not the wall time above)
    from mlx8_ws_audio_transformer_amd.generation import select_tokens
    PROF_STEPS = 16
    with torch.no_grad():
        audio_kv = adapter.encode_audio(audio)
        cache = Qwen3Cache(cfg, 1, 256, dev)
        dec.prefill(torch.randn(1, 256 - PROF_STEPS, cfg.hidden_size, device=dev), cache)
        ids = torch.tensor([[start]], device=dev)
        torch.cuda.synchronize()
        _lib.prof_enable(True)
        for _ in range(PROF_STEPS):
            ids = select_tokens(dec.step(adapter(dec.get_input_embeddings()(ids), audio_kv=audio_kv), cache), cfg.vocab_size)[1][:, :1]
        torch.cuda.synchronize()
    classes = {}
    for klass in ("gemm", "attention", "layernorm", "other"):
        ms, n, _ = _lib.prof_collect(klass)
        classes[klass] = {"ms_per_token": round(ms / PROF_STEPS, 4), "launches_per_token": round(n / PROF_STEPS, 1)}
    _lib.prof_enable(False)
    state = bench.read_power_sysfs(pci=bench.device_pci_address(torch, torch.cuda.current_device()))

    batch = {f"batch{B}": {"ms_per_step": res[f"native_generate_batch{B}_ms_per_step"],
                           "clips_x_tokens_per_s": round(B * 1e3 / res[f"native_generate_batch{B}_ms_per_step"], 1),
                           "clip_0_tokens_equal_batch_1": bool(outs[f"native_generate_batch{B}_ms_per_step"][0] == outs["native_generate_ms_per_token"])}
             for B in batches}
    parent, verdict = None, None
    if a.parent_json:
        parent = json.loads(open(a.parent_json).read())
        key = "native_generate_ms_per_token"
        p_ms, t_ms = parent["results"][key], res[key]
        margin = max(parent["max_over_min_of_windows"][key], spread[key])
        verdict = {"parent_ms_per_token": p_ms, "this_ms_per_token": t_ms, "parent_over_this": round(p_ms / t_ms, 3), "larger_max_over_min_of_the_two_runs": margin,
                   "condition": "this < parent / larger spread", "met": bool(t_ms < p_ms / margin)}
    same = sum(int(p == q) for p, q in zip(outs["native_generate_ms_per_token"], outs["torch_fp32_full_recompute_generate_ms_per_token"]))
    pre_err = float((outs["native_prefill_ms"] - outs["torch_fp32_prefill_ms"]).abs().max())
    line = json.dumps({"metric": f"music2midi inference at Qwen3-0.6B's shape (28 layers, hidden 1024, 16 / 8 heads, vocab 151936; adapter audio_dim {AUDIO_DIM}, {SA} encoder "
                                 f"positions), seeded weights, precision {a.precision}: native generate with KV cache ({a.tokens} greedy tokens, batch 1) and prefill (B {PREFILL_B}, "
                                 f"L {PREFILL_L}) beside a torch fp32 restatement of the reference's full-recompute loop on the same GPU; medians of alternating windows, host clock "
                                 "around a device synchronise",
                       "results": res, "max_over_min_of_windows": spread, "rounds": a.rounds, "tokens": a.tokens,
                       "native_generate_batch": batch, "batch_1_against_the_parent_commit": verdict, "parent_commit": parent,
                       "native_kernel_classes_per_step_at_cache_length_240_to_256": classes,
                       "note_kernel_classes": "gemm = the 4 layer GEMMs x 28 + lm_head + the adapter's linears; attention = awt_op_causal_attention x 28 + the adapter's "
                                              "cross-attention; layernorm = RMSNorm x 57 + the adapter's LayerNorms; other = qk_norm_rope, silu_mul x 28, GELU, argmax",
                       "greedy_tokens_equal_native_vs_torch_fp32": f"{same} of {a.tokens} (seeded N(0, 0.02) weights: near-ties; informational)",
                       "prefill_last_logits_native_vs_torch_fp32_max_abs": pre_err,
                       "gpu_state_after_native_generate": None if state is None else {"package_watts": state[0], "shader_clock_mhz": state[1], "which": state[2]},
                       "device": torch.cuda.get_device_name(0)})
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
