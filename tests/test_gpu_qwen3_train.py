"""Training through music2midi.Qwen3Decoder(trainable_layers=K) and MusicTranscriptionModel against float64 autograd of tests/qwen3_reference.py's decoder
(`forward` + `causal_lm_loss`) and tests/music2midi_reference.py's adapter.

Bounds, the project's (tests/test_gpu_music2midi_adapter.py): loss within 1e-3 relative; for the gradient of inputs_embeds and of EVERY trainable parameter
err <= 2e-4 * max|grad| + 1e-7; a frozen parameter's grad stays None.  Every figure is printed before it is asserted.  The float64 reference of a case is
computed once (all gradients at once) and shared by the cases that differ only in what they train."""
import functools

import pytest
import torch

from tests import qwen3_reference as qr
from tests import qwen3_train_reference as tr
from tests.music2midi_reference import ReferenceAdapter, nontrivial_

pytestmark = pytest.mark.gpu

LOSS_TOL, GRAD_TOL, GRAD_FLOOR = 1e-3, 2e-4, 1e-7


def _decoder(cfg, sd, K, precision="bf16x3"):
    from mlx8_ws_audio_transformer_amd.music2midi import Qwen3Decoder
    dec = Qwen3Decoder(cfg, precision=precision, trainable_layers=K)
    dec.load_state_dict({k: v.float() for k, v in sd.items()}, strict=True)
    return dec.cuda()


def _labels(cfg, B, L):
    labels = (torch.arange(B * L).reshape(B, L) * 37 + 5) % cfg.vocab_size
    labels[0, 3] = -100
    labels[-1, -4:] = -100                                                 # a padded tail
    return labels


@functools.lru_cache(maxsize=None)
def _reference(base, tied, B, L):
    """(cfg, state dict, x, labels, float64 loss, {name: gradient}) with the gradient of "inputs_embeds" and of every parameter the loss depends on (with
    an untied head the embedding table is not one of them: the decoder is driven by inputs_embeds); never modified."""
    cfg = qr.config(qr.MICRO if base == "micro" else qr.WIDE, tied)
    sd = qr.state_dict(cfg, seed=11)
    x = qr.variates(f"train.x.{base}", (B, L, cfg.hidden_size), 11)
    labels = _labels(cfg, B, L)
    leaves = {k: v.cuda().requires_grad_(True) for k, v in sd.items()}
    xg = x.cuda().requires_grad_(True)
    loss = qr.causal_lm_loss(qr.forward(leaves, cfg, xg), labels)
    names = ["inputs_embeds"] + list(leaves)
    grads = {n: g for n, g in zip(names, torch.autograd.grad(loss, [xg] + list(leaves.values()), allow_unused=True)) if g is not None}
    assert set(names) - set(grads) == (set() if tied else {"model.embed_tokens.weight"})
    return cfg, sd, x, labels, loss.detach(), grads


def _check_grads(label, got, want):
    failed = []
    for name, w in want.items():
        assert got[name] is not None, name
        scale, e = float(w.abs().max()), float((got[name].double() - w).abs().max())
        assert scale > 0 and bool(torch.isfinite(got[name]).all()), name
        print(f"  {label} d {name}: err {e:.3e} = {e / scale:.3e} of max|grad| {scale:.3e} (tol {GRAD_TOL})")
        if not e <= GRAD_TOL * scale + GRAD_FLOOR:
            failed.append((name, e, scale))
    assert not failed, failed


def _check_loss(label, loss, want):
    rel = abs(float(loss) - float(want)) / abs(float(want))
    print(f"{label}: loss {float(loss):.6f} vs float64 {float(want):.6f} ({rel:.3e} relative, tol {LOSS_TOL})")
    assert rel <= LOSS_TOL


CASES = [("micro", tied, K, B, L) for tied in (True, False) for K in (1, 2) for B, L in ((2, 37), (1, 130))] + [("wide", True, 1, 1, 130)]


@pytest.mark.parametrize("base,tied,K,B,L", CASES)
def test_loss_and_every_gradient_match_float64_autograd(base, tied, K, B, L):
    cfg, sd, x, labels, want_loss, want = _reference(base, tied, B, L)
    dec = _decoder(cfg, sd, K)
    xg = x.float().cuda().requires_grad_(True)
    logits, loss = dec(xg, labels=labels.cuda())
    assert logits.shape == (B, L, cfg.vocab_size) and not logits.requires_grad and loss.requires_grad
    loss.backward()
    label = f"{base} tied={tied} K={K} B{B} L{L}"
    trained = tr.trainable_names(cfg, K)
    got = {n: p.grad for n, p in dec.named_parameters()}
    assert {n for n, g in got.items() if g is not None} == trained, "exactly the reference rule's parameters get a gradient; a frozen one keeps grad None"
    got["inputs_embeds"] = xg.grad
    _check_loss(label, loss, want_loss)
    _check_grads(label, got, {n: want[n] for n in ["inputs_embeds"] + sorted(trained)})


def test_logits_are_differentiable_without_labels():
    cfg, sd, x, _, _, _ = _reference("micro", True, 2, 37)
    w = qr.variates("train.dlogits", (2, 37, cfg.vocab_size), 5).cuda()
    leaves = {k: v.cuda().requires_grad_(True) for k, v in sd.items()}
    xr_ = x.cuda().requires_grad_(True)
    names = ["inputs_embeds", "model.norm.weight", "model.embed_tokens.weight", "model.layers.1.self_attn.k_norm.weight"]
    want = dict(zip(names, torch.autograd.grad((qr.forward(leaves, cfg, xr_) * w).sum(), [xr_] + [leaves[n] for n in names[1:]])))
    dec = _decoder(cfg, sd, 1)
    xg = x.float().cuda().requires_grad_(True)
    logits = dec(xg)
    assert logits.shape == (2, 37, cfg.vocab_size) and logits.requires_grad
    (logits * w.float()).sum().backward()
    got = {n: p.grad for n, p in dec.named_parameters()}
    got["inputs_embeds"] = xg.grad
    _check_grads("logits", got, want)


def test_without_an_input_gradient_the_frozen_layers_are_not_walked():
    """inputs_embeds without requires_grad: the trained layer's and the head's gradients are the same bits as with it."""
    cfg, sd, x, labels, _, _ = _reference("micro", False, 2, 37)
    grads = []
    for need_dx in (True, False):
        dec = _decoder(cfg, sd, 1)
        dec(x.float().cuda().requires_grad_(need_dx), labels=labels.cuda())[1].backward()
        grads.append({n: p.grad for n, p in dec.named_parameters() if p.grad is not None})
    assert set(grads[0]) == set(grads[1]) == tr.trainable_names(cfg, 1)
    assert all(torch.equal(grads[0][n], grads[1][n]) for n in grads[0])


# ------------------------------------------------------------------------------------------------ the whole model
def _model(K, tied=True, seed=qr.GREEDY_SEED):
    from mlx8_ws_audio_transformer_amd.music2midi import CrossAttentionAdapter, MusicTranscriptionModel
    cfg = qr.config(qr.MICRO, tied)
    sd = qr.state_dict(cfg, seed)
    ref_adapter = nontrivial_(ReferenceAdapter(128, cfg.hidden_size, num_heads=2), seed)
    audio = qr.variates("qwen3.audio", (1, 130, 128), seed)
    adapter = CrossAttentionAdapter(128, cfg.hidden_size, num_heads=2)
    adapter.load_state_dict({k: v.float() for k, v in ref_adapter.state_dict().items()}, strict=True)
    tower = lambda waveforms, sampling_rate: audio.float().cuda().expand(len(waveforms), -1, -1).contiguous()   # a stub audio tower
    dec = _decoder(cfg, sd, K) if K is not None else _decoder_inference(cfg, sd)
    return MusicTranscriptionModel(tower, adapter.cuda(), dec), (cfg, sd, ref_adapter, audio)


def _decoder_inference(cfg, sd):
    from mlx8_ws_audio_transformer_amd.music2midi import Qwen3Decoder
    dec = Qwen3Decoder(cfg)
    dec.load_state_dict({k: v.float() for k, v in sd.items()}, strict=True)
    return dec.cuda()


def _ids(cfg):
    ids = (torch.arange(2 * 37).reshape(2, 37) * 29 + 3) % cfg.vocab_size
    ids[1, -5:] = -100                                                     # ignored targets; they embed as token 0
    ids[0, 7] = ids[0, 2]                                                  # a repeated token: two rows of the lookup add into one table row
    return ids


def test_model_loss_trains_the_adapter_and_the_tied_embedding():
    model, (cfg, sd, ref_adapter, audio) = _model(1)
    ids = _ids(cfg)
    loss = model([None, None], 16000, ids.cuda(), torch.ones(2, 37, dtype=torch.long).cuda())
    loss.backward()
    leaves = {k: v.cuda().requires_grad_(True) for k, v in sd.items()}
    ref_adapter = ref_adapter.cuda()
    text = leaves["model.embed_tokens.weight"][ids.clamp_min(0).cuda()]
    want_loss = qr.causal_lm_loss(qr.forward(leaves, cfg, ref_adapter(text, audio.cuda().expand(2, -1, -1))), ids)
    params = dict(ref_adapter.named_parameters())
    want = dict(zip(list(params) + ["embed"], torch.autograd.grad(want_loss, list(params.values()) + [leaves["model.embed_tokens.weight"]])))
    ref_adapter.cpu()
    got = {n: p.grad for n, p in model.cross_attention_adapter.named_parameters()}
    assert len(got) == 14 and set(got) == set(params)
    got["embed"] = model.text_decoder.model.embed_tokens.weight.grad        # lookup + head
    _check_loss("model", loss, want_loss.detach())
    _check_grads("model", got, want)


def test_three_adamw_steps_follow_the_float64_model():
    """Three AdamW steps (lr 1e-4, weight_decay 1e-4: the reference's, music2midi/train.py:52-54) of the tied micro decoder with its top layer trained, against the float64 decoder stepped the same way:
    each step's loss within 1e-3 relative.  The packed GEMM operands have to follow the parameters: with stale ones the second and third losses would be
    those of the first step's weights, and the reference's loss moves by far more than the bound between steps (asserted).  A frozen weight's handle is
    neither rebuilt nor re-packed; a trained one is re-packed in place."""
    from mlx8_ws_audio_transformer_amd.native_decoder import PackedLinear
    cfg, sd, x, labels, _, _ = _reference("micro", True, 2, 37)
    dec = _decoder(cfg, sd, 1)
    trained = tr.trainable_names(cfg, 1)
    leaves = {k: v.cuda().requires_grad_(k in trained) for k, v in sd.items()}
    opts = (torch.optim.AdamW([p for p in dec.parameters() if p.requires_grad], lr=1e-4, weight_decay=1e-4),
            torch.optim.AdamW([leaves[n] for n in sorted(trained)], lr=1e-4, weight_decay=1e-4))
    updated, update = [], PackedLinear.update
    PackedLinear.update = lambda self, w, b: (updated.append(id(self)), update(self, w, b))[1]
    try:
        losses, handles = [], None
        for step in range(3):
            loss = dec(x.float().cuda(), labels=labels.cuda())[1]
            want = qr.causal_lm_loss(qr.forward(leaves, cfg, x.cuda()), labels)
            if handles is None:
                pk = dec._pack()
                handles = {(i, k): (id(v), v.handle) for i, lay in enumerate(pk["layers"]) for k, v in lay.items()}
                handles[("head", "lm_head")] = (id(pk["lm_head"]), pk["lm_head"].handle)
            _check_loss(f"step {step}", loss, want.detach())
            losses.append(float(want))
            for opt, l in zip(opts, (loss, want)):
                opt.zero_grad()
                l.backward()
                opt.step()
        pk = dec._pack()                                                   # what the next forward would do: the third step's weights are packed
    finally:
        PackedLinear.update = update
    moved = abs(losses[2] - losses[0]) / losses[0]
    print(f"the float64 loss moved by {moved:.3e} relative over the steps")
    assert moved > 10 * LOSS_TOL
    now = {(i, k): (id(v), v.handle) for i, lay in enumerate(pk["layers"]) for k, v in lay.items()}
    now[("head", "lm_head")] = (id(pk["lm_head"]), pk["lm_head"].handle)
    assert now == handles, "a handle was rebuilt"
    frozen = {handles[(0, k)][0] for k in ("qkv", "o", "gu", "down")}
    live = {handles[(1, k)][0] for k in ("qkv", "o", "gu", "down")} | {handles[("head", "lm_head")][0]}
    assert not frozen & set(updated), "a frozen weight was re-packed"
    assert set(updated) == live and len(updated) == 3 * len(live), "every trained weight is re-packed once per step"


def test_trainable_state_dict_round_trips():
    model, (cfg, _, _, _) = _model(1)
    state = model.trainable_state_dict()
    want = {"text_decoder." + n for n in tr.trainable_names(cfg, 1)} | {"cross_attention_adapter." + n for n, _ in model.cross_attention_adapter.named_parameters()}
    assert set(state) == want and not any(v.requires_grad for v in state.values())
    other, _ = _model(1, seed=qr.GREEDY_SEED + 1)
    ids = _ids(cfg).cuda()
    with torch.no_grad():
        other([None, None], 16000, ids)                                    # packs the decoder's operands from the weights it was built with
    before = {n: p.detach().clone() for n, p in other.named_parameters()}
    res = other.load_state_dict(state, strict=False)
    assert not res.unexpected_keys and set(res.missing_keys).isdisjoint(state)
    for n, p in other.named_parameters():
        if n in state:
            assert torch.equal(p, state[n]) and not torch.equal(p, before[n]), n
        else:
            assert torch.equal(p, before[n]), n
    fresh, _ = _model(1, seed=qr.GREEDY_SEED + 1)                          # the same model, loaded before it ever packed
    fresh.load_state_dict(state, strict=False)
    with torch.no_grad():                                                  # the packed operands followed the loaded parameters
        assert torch.equal(other([None, None], 16000, ids), fresh([None, None], 16000, ids))


def test_inference_only_refusals_still_hold():
    model, (cfg, sd, _, _) = _model(None)
    dec = model.text_decoder
    x = torch.zeros(1, 4, cfg.hidden_size, device="cuda")
    assert not any(p.requires_grad for p in dec.parameters())
    with pytest.raises(NotImplementedError, match="inference only"):
        dec(x.clone().requires_grad_(True))
    with pytest.raises(NotImplementedError, match="inference only"):
        model([None], 16000, torch.zeros(1, 4, dtype=torch.long, device="cuda"))
    with torch.no_grad():
        assert dec(x).shape == (1, 4, cfg.vocab_size)
    trainable = _decoder(cfg, sd, 0)
    from mlx8_ws_audio_transformer_amd.music2midi import Qwen3Cache
    with pytest.raises(NotImplementedError, match="inference only"):      # the cached paths never build a graph
        trainable.prefill(x, Qwen3Cache(cfg, 1, 8, "cuda"))
