"""music2midi.Qwen3Decoder and MusicTranscriptionModel on the GPU against the float64 restatement (tests/qwen3_reference.py).

Bound, the project's module bound (OUT_TOL of tests/test_gpu_music2midi_adapter.py / test_gpu_classifier.py at bf16x3) scaled to the output's magnitude:
logits max-abs <= 1e-3 * max(1, max |reference logits|); the loss within the same relative figure.  Every figure is printed before it is asserted."""
import functools

import pytest
import torch

from tests import qwen3_reference as qr

pytestmark = pytest.mark.gpu

OUT_TOL = 1e-3


def _decoder(cfg, sd, precision="bf16x3"):
    from mlx8_ws_audio_transformer_amd.music2midi import Qwen3Decoder
    dec = Qwen3Decoder(cfg, precision=precision)
    dec.load_state_dict({k: v.float() for k, v in sd.items()}, strict=True)
    return dec.cuda().eval()


@functools.lru_cache(maxsize=None)
def _case(base, tied, B, L):
    """(cfg, state dict, decoder on the GPU, inputs x float64 [B, L, hidden], labels, reference logits, reference loss); base: "micro" or "wide"."""
    cfg = qr.config(qr.MICRO if base == "micro" else qr.WIDE, tied)
    sd = qr.state_dict(cfg, seed=11)
    x = qr.variates(f"dec.x.{base}", (B, L, cfg.hidden_size), 11)
    labels = (torch.arange(B * L).reshape(B, L) * 37 + 5) % cfg.vocab_size
    ref = qr.forward({k: v.cuda() for k, v in sd.items()}, cfg, x.cuda())
    return cfg, sd, _decoder(cfg, sd), x, labels, ref, qr.causal_lm_loss(ref, labels)


def _bound(ref):
    return OUT_TOL * max(1.0, float(ref.abs().max()))


@pytest.mark.parametrize("base,tied,B,L", [("micro", True, 2, 37), ("micro", False, 2, 37), ("micro", True, 1, 5), ("micro", False, 1, 5), ("wide", True, 1, 130)])
def test_logits_and_loss(base, tied, B, L):
    cfg, sd, dec, x, labels, ref, ref_loss = _case(base, tied, B, L)
    with torch.no_grad():
        logits, loss = dec(x.float().cuda(), labels=labels.cuda())
    assert logits.shape == (B, L, cfg.vocab_size)
    err, tol = float((logits.double() - ref).abs().max()), _bound(ref)
    lerr, ltol = abs(float(loss) - float(ref_loss)), OUT_TOL * max(1.0, abs(float(ref_loss)))
    print(f"{base} tied={tied} B{B} L{L}: logits max-abs {err:.3e} (bound {tol:.3e}, {err / tol:.3f} of it; max |logit| {float(ref.abs().max()):.1f}); "
          f"loss {float(loss):.6f} vs {float(ref_loss):.6f} ({lerr / ltol:.3f} of its bound)")
    assert bool(torch.isfinite(logits).all()) and err <= tol
    assert lerr <= ltol


def test_right_padded_batch():
    """Row 1 of a [2, 37] batch has 29 live positions, labels -100 on its padding: the loss is that of the two unpadded rows computed separately, and the
    live logits equal those of the unpadded runs to the bit (causality: nothing at a live position sees the padding)."""
    cfg, sd, dec, x, labels, _, _ = _case("micro", True, 2, 37)
    xg, n1 = x.float().cuda(), 29
    mask = torch.ones(2, 37, dtype=torch.long)
    mask[1, n1:] = 0
    lab = labels.clone()
    lab[1, n1:] = -100
    with torch.no_grad():
        logits, loss = dec(xg, attention_mask=mask.cuda(), labels=lab.cuda())
        l0, loss0 = dec(xg[:1], labels=lab[:1].cuda())
        l1, loss1 = dec(xg[1:, :n1], labels=lab[1:, :n1].cuda())
    want = (float(loss0) * 36 + float(loss1) * (n1 - 1)) / (36 + n1 - 1)
    print(f"padded-batch loss {float(loss):.6f}, from the unpadded rows {want:.6f}")
    assert abs(float(loss) - want) <= 1e-5 * max(1.0, abs(want))          # the same fp32 row losses, averaged in another order
    assert torch.equal(logits[0], l0[0]) and torch.equal(logits[1, :n1], l1[0])
    with pytest.raises(ValueError, match="right padding"):
        dec(xg, attention_mask=mask.flip(1).cuda())


def test_prefill_then_steps_match_the_full_forward():
    """9 positions prefilled, then 15 single steps: every step's last-position logits against the full forward over the 24 positions (cache rows, positions,
    the causal offset)."""
    from mlx8_ws_audio_transformer_amd.music2midi import Qwen3Cache
    cfg, sd, dec, x, _, ref, _ = _case("micro", False, 2, 37)
    xg, tol = x.float().cuda(), _bound(ref)
    cache = Qwen3Cache(cfg, 2, 24, "cuda")
    for t in cache.k + cache.v:
        t.fill_(float("nan"))                                              # what torch.empty may hold
    with torch.no_grad():
        got = [dec.prefill(xg[:, :9], cache)]
        for t in range(9, 24):
            got.append(dec.step(xg[:, t:t + 1], cache))
    assert cache.length == 24
    errs = [float((g.double() - ref[:, 8 + i]).abs().max()) for i, g in enumerate(got)]
    print(f"prefill 9 + 15 steps: worst last-position logits max-abs {max(errs):.3e} (bound {tol:.3e}, {max(errs) / tol:.3f} of it)")
    assert all(bool(torch.isfinite(g).all()) for g in got) and max(errs) <= tol
    with pytest.raises(ValueError, match="cache holds"):
        dec.step(xg[:, :1], cache)                                         # full


def _model(seed=qr.GREEDY_SEED):
    from mlx8_ws_audio_transformer_amd.music2midi import CrossAttentionAdapter, MusicTranscriptionModel
    cfg, sd, ref_adapter, audio = qr.greedy_fixture(seed)
    adapter = CrossAttentionAdapter(128, cfg.hidden_size, num_heads=2)
    adapter.load_state_dict({k: v.float() for k, v in ref_adapter.state_dict().items()}, strict=True)
    tower = lambda waveforms, sampling_rate: audio.float().cuda().expand(len(waveforms), -1, -1).contiguous()   # a stub audio tower: seeded features [1, 130, 128] per clip
    return MusicTranscriptionModel(tower, adapter.cuda().eval(), _decoder(cfg, sd)), (cfg, sd, ref_adapter, audio)


def test_greedy_generation_reproduces_the_reference_tokens():
    """generate(do_sample=False) -- adapter on the new token only, KV cache -- against the reference's full-recompute loop in float64: the same 24 tokens for
    both prompts, no position excluded (tests/test_qwen3_reference_host.py establishes that the reference's top-2 margins make that fair)."""
    model, (cfg, sd, ref_adapter, audio) = _model()
    sd_g, ref_adapter, audio = {k: v.cuda() for k, v in sd.items()}, ref_adapter.cuda(), audio.cuda()
    for prompt in qr.GREEDY_PROMPTS:
        want, _ = qr.greedy(sd_g, cfg, ref_adapter, audio, prompt, qr.GREEDY_STEPS)
        got = model.generate(None, 16000, max_new_tokens=qr.GREEDY_STEPS, do_sample=False, bos_token_id=prompt if len(prompt) > 1 else prompt[0],
                             eos_token_id=qr.GREEDY_EOS)
        print(f"prompt {prompt}: generated {got}\n{' ' * (len(str(prompt)) + 9)}reference {want}")
        assert got == want
    ref_adapter.cpu()


def test_sampling_is_reproducible_and_stops_at_eos():
    model, _ = _model()
    runs = []
    for _ in range(2):
        gen = torch.Generator(device="cuda").manual_seed(7)
        runs.append(model.generate(None, 16000, max_new_tokens=12, temperature=0.7, do_sample=True, generator=gen, bos_token_id=5, eos_token_id=qr.GREEDY_EOS))
    print("sampled", runs[0])
    assert runs[0] == runs[1] and len(runs[0]) <= 12 and all(0 <= t < 320 for t in runs[0])
    first = model.generate(None, 16000, max_new_tokens=12, do_sample=False, bos_token_id=5, eos_token_id=qr.GREEDY_EOS)
    stopped = model.generate(None, 16000, max_new_tokens=12, do_sample=False, bos_token_id=5, eos_token_id=first[3])
    print("greedy", first, "with eos", first[3], "->", stopped)
    assert stopped == first[:first.index(first[3])]                        # stops at the first EOS, which is not returned


def test_model_forward_returns_the_teacher_forced_loss():
    """MusicTranscriptionModel.forward: embed, adapter over the whole text, decoder loss -- against the float64 pieces."""
    model, (cfg, sd, ref_adapter, audio) = _model()
    ids = ((torch.arange(2 * 9).reshape(2, 9) * 29 + 3) % cfg.vocab_size)
    with torch.no_grad():
        loss = model([None, None], 16000, ids.cuda(), torch.ones(2, 9, dtype=torch.long).cuda())
        text = sd["model.embed_tokens.weight"][ids]
        want = qr.causal_lm_loss(qr.forward(sd, cfg, ref_adapter.cpu()(text, audio.cpu().expand(2, -1, -1))), ids)
    print(f"model loss {float(loss):.6f} vs float64 {float(want):.6f}")
    assert abs(float(loss) - float(want)) <= OUT_TOL * max(1.0, abs(float(want)))
