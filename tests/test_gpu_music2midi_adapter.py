"""music2midi.CrossAttentionAdapter on the native operators against its float64 torch.nn restatement (tests/music2midi_reference.py).

Bounds, from tests/test_gpu_classifier.py (the deeper classifier at bf16x3): output max-abs error <= 1e-3; for each of the 14 parameter gradients
and both input gradients err <= 2e-4 * max|grad| + 1e-7.  Every figure is printed before it is asserted."""
import functools

import pytest
import torch

from tests.music2midi_reference import ReferenceAdapter, nontrivial_, variates

pytestmark = pytest.mark.gpu

OUT_TOL, GRAD_TOL, GRAD_FLOOR = 1e-3, 2e-4, 1e-7

# (audio_dim, text_dim, heads, B, L, Sa)
SHAPES = [(128, 256, 2, 2, 37, 200), (128, 256, 2, 1, 5, 1500), (512, 1024, 8, 1, 3, 130)]


def _native(ref, audio_dim, text_dim, heads, **kw):
    from mlx8_ws_audio_transformer_amd import CrossAttentionAdapter
    nat = CrossAttentionAdapter(audio_dim, text_dim, heads, **kw)
    state = {k: v.to(nat.audio_projection.weight.dtype) for k, v in ref.state_dict().items()}
    assert not any(nat.load_state_dict(state, strict=True))
    return nat.cuda()


@functools.lru_cache(maxsize=None)
def _reference(audio_dim, text_dim, heads, B, L, Sa):
    """The float64 module, its inputs, output and every gradient under a fixed upstream gradient; computed once per shape, never modified."""
    ref = nontrivial_(ReferenceAdapter(audio_dim, text_dim, heads), seed=audio_dim + L)
    text = variates("m2m.text", (B, L, text_dim), 1).requires_grad_(True)
    audio = variates("m2m.audio", (B, Sa, audio_dim), 2).requires_grad_(True)
    d_out = variates("m2m.dout", (B, L, text_dim), 3)
    out = ref(text, audio)
    out.backward(d_out)
    grads = {name: p.grad.clone() for name, p in ref.named_parameters()}
    grads["text_embeddings"], grads["audio_features"] = text.grad.clone(), audio.grad.clone()
    return ref, text.detach(), audio.detach(), d_out, out.detach(), grads


@pytest.mark.parametrize("audio_dim,text_dim,heads,B,L,Sa", SHAPES)
def test_output_and_every_gradient_match_the_float64_module(audio_dim, text_dim, heads, B, L, Sa):
    ref, text, audio, d_out, want, want_grads = _reference(audio_dim, text_dim, heads, B, L, Sa)
    nat = _native(ref, audio_dim, text_dim, heads)
    t, a = text.float().cuda().requires_grad_(True), audio.float().cuda().requires_grad_(True)
    out = nat(t, a)
    assert out.shape == (B, L, text_dim) and out.dtype == torch.float32
    out.backward(d_out.float().cuda())
    err = float((out.detach().cpu().double() - want).abs().max())
    print(f"output max-abs error {err:.3e} (tol {OUT_TOL})")
    got = {name: p.grad for name, p in nat.named_parameters()}
    got["text_embeddings"], got["audio_features"] = t.grad, a.grad
    assert len(got) == 16 and set(got) == set(want_grads)
    failed = []
    for name, w in want_grads.items():
        assert got[name] is not None, name
        scale, e = float(w.abs().max()), float((got[name].cpu().double() - w).abs().max())
        assert scale > 0, name
        print(f"  d {name}: err {e:.3e} = {e / scale:.3e} of max|grad| {scale:.3e} (tol {GRAD_TOL})")
        if not e <= GRAD_TOL * scale + GRAD_FLOOR:
            failed.append((name, e, scale))
    assert err <= OUT_TOL, err
    assert not failed, failed


def test_audio_kv_reuse_is_bit_identical_and_carries_gradients():
    audio_dim, text_dim, heads, B, L, Sa = SHAPES[0]
    ref, text, audio, d_out, _, _ = _reference(*SHAPES[0])
    nat = _native(ref, audio_dim, text_dim, heads)
    t, a = text.float().cuda(), audio.float().cuda().requires_grad_(True)
    direct = nat(t, a)
    kv = nat.encode_audio(a)
    assert kv.shape == (B, Sa, 2 * text_dim)
    reused = nat(t, audio_kv=kv)
    assert torch.equal(direct, reused)
    assert torch.equal(nat(t[:, :1].contiguous(), audio_kv=kv.detach()), nat(t[:, :1].contiguous(), a).detach())    # one decoding step's query
    direct.backward(d_out.float().cuda())
    g_direct, a.grad = a.grad.clone(), None
    reused.backward(d_out.float().cuda())
    assert torch.equal(g_direct, a.grad)
    with pytest.raises(ValueError, match="exactly one"):
        nat(t, a, audio_kv=kv)


def test_one_adamw_step_moves_every_parameter_like_the_reference():
    """One AdamW step with the reference's own adapter hyper-parameters (music2midi/train.py:52-54: lr 1e-4, weight_decay 1e-4) on both modules, then a
    second forward: every native parameter moved, and the outputs agree to 1e-3.  The learning rate matters to that bound: Adam's first step moves every
    weight by lr * g / (|g| + 1e-8), i.e. by lr * sign(g), so an element whose true gradient lies below the gradient error the suite allows (2e-4 of the
    tensor's largest) may move the other way and end 2 lr from the reference's; the reference's lr is the one a user of this module runs."""
    audio_dim, text_dim, heads, B, L, Sa = SHAPES[0]
    base, text, audio, d_out, _, _ = _reference(*SHAPES[0])
    ref = ReferenceAdapter(audio_dim, text_dim, heads)
    ref.load_state_dict(base.state_dict())
    nat = _native(ref, audio_dim, text_dim, heads)
    before = {k: v.clone() for k, v in nat.state_dict().items()}
    t, a = text.float().cuda(), audio.float().cuda()
    for model, tt, aa, dd in ((ref, text, audio, d_out), (nat, t, a, d_out.float().cuda())):
        opt = torch.optim.AdamW(model.parameters(), lr=1e-4, weight_decay=1e-4)
        (model(tt, aa) * dd).sum().backward()
        opt.step()
    for k, v in nat.state_dict().items():
        assert not torch.equal(v, before[k]), f"{k} did not move"
    moved = float((ref(text, audio).detach() - _reference(*SHAPES[0])[4]).abs().max())
    err = float((nat(t, a).detach().cpu().double() - ref(text, audio).detach()).abs().max())
    print(f"second forward after one AdamW step: max-abs error {err:.3e} (tol 1e-3); the step moved the reference's output by {moved:.3e}")
    assert moved > 1e-3                          # the step is not a no-op at this tolerance
    assert err <= 1e-3


@pytest.mark.parametrize("precision", ["bf16"])
def test_bf16_precision_and_bf16_tensors(precision):
    """precision="bf16" runs (one product per fragment pair: 2^-9 per operand, so only a loose sanity bound); a bf16 module fed bf16 inputs computes in fp32
    and returns bf16, within bf16's own output rounding (2^-8 of |out| <= ~4) of the float64 module on the same bf16-rounded parameters and inputs."""
    audio_dim, text_dim, heads, B, L, Sa = SHAPES[0]
    ref, text, audio, _, want, _ = _reference(*SHAPES[0])
    nat = _native(ref, audio_dim, text_dim, heads, precision=precision)
    out = nat(text.float().cuda(), audio.float().cuda()).detach()
    err = float((out.cpu().double() - want).abs().max())
    print(f"precision bf16: max-abs error {err:.3e}")
    assert out.dtype == torch.float32 and err < 0.25

    ref16 = ReferenceAdapter(audio_dim, text_dim, heads)
    ref16.load_state_dict({k: v.bfloat16().double() for k, v in ref.state_dict().items()})
    nat16 = _native(ref, audio_dim, text_dim, heads, dtype=torch.bfloat16)
    assert nat16.layer_norm1.weight.dtype == torch.bfloat16
    t16, a16 = text.bfloat16().cuda().requires_grad_(True), audio.bfloat16().cuda()
    out16 = nat16(t16, a16)
    assert out16.dtype == torch.bfloat16 and out16.shape == (B, L, text_dim)
    want16 = ref16(t16.detach().cpu().double(), a16.cpu().double()).detach()
    err16 = float((out16.detach().cpu().double() - want16).abs().max())
    print(f"bf16 tensors: max-abs error {err16:.3e} (bf16 output rounding 2^-8 * {float(want16.abs().max()):.2f})")
    assert err16 <= 2.0 ** -8 * float(want16.abs().max()) + 1e-3
    out16.float().sum().backward()
    assert t16.grad is not None and t16.grad.dtype == torch.bfloat16 and nat16.feedforward[0].weight.grad.dtype == torch.bfloat16
