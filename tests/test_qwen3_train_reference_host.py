"""Host checks (no GPU) of tests/qwen3_train_reference.py and of `Qwen3Decoder(..., trainable_layers=K)`'s parameter flags.

Each closed-form backward is held against torch.autograd.grad of tests/qwen3_reference.py's float64 forward to a relative error of 1e-12 (max |difference| over
max |autograd|: both sides are float64 evaluations of the same function, a few hundred terms per sum, so 1e-12 leaves four decimal digits over their
rounding).  The rounded attention backward has to stay near the exact one: its roundings are relative 2^-17 (bf16x3 operands) or 2^-9 (bf16), so per output
the maximum error over the output's maximum is asserted under 2^-12 and 2^-5 -- 32 and 16 roundings' worth, a sanity band that a wrong mask, group or scale
(an O(1) error) cannot meet."""
import pytest
import torch

from mlx8_ws_audio_transformer_amd import music2midi as m2m
from tests import qwen3_reference as qr
from tests import qwen3_train_reference as tr

REL = 1e-12


def _rel(got, want):
    return float((got - want).abs().max() / want.abs().max())


def _grad(out, inputs, dout):
    return torch.autograd.grad(out, inputs, dout)


def _v(name, shape, scale=1.0):
    return qr.variates("train.host." + name, shape, 7, scale)


@pytest.mark.parametrize("with_dres", [False, True])
def test_rmsnorm_backward_is_autograd(with_dres):
    x, dy, gamma = _v("rms.x", (9, 260), 2.0).requires_grad_(True), _v("rms.dy", (9, 260)), (1.0 + 0.3 * _v("rms.g", (260,))).requires_grad_(True)
    dres = _v("rms.dres", (9, 260)) if with_dres else None
    dx, dg = _grad(qr.rmsnorm(x, gamma, 1e-6), (x, gamma), dy)
    assert _rel(tr.rmsnorm_backward(dy, x.detach(), gamma.detach(), 1e-6, dres), dx + (dres if with_dres else 0.0)) <= REL
    assert _rel(tr.rmsnorm_param_grad(dy, x.detach(), 1e-6), dg) <= REL


def test_silu_mul_backward_is_autograd():
    gu = _v("silu.gu", (7, 2 * 96), 4.0)
    gu[0, :6] = torch.tensor([-88.0, 88.0, -20.0, 20.0, 0.0, -1e-3], dtype=torch.float64)
    gu, dy = gu.requires_grad_(True), _v("silu.dy", (7, 96))
    (dgu,) = _grad(qr.silu_mul(gu, 96), (gu,), dy)
    got = tr.silu_mul_backward(gu.detach(), dy, 96)
    assert _rel(got, dgu) <= REL
    assert bool(torch.isfinite(got).all())


@pytest.mark.parametrize("B,Lq,Hq,Hkv", [(2, 5, 4, 1), (1, 3, 4, 2)])
def test_qk_norm_rope_backward_is_autograd(B, Lq, Hq, Hkv):
    rows_, eps = B * Lq, 1e-6
    qkv = _v("rope.qkv", (rows_, (Hq + 2 * Hkv) * 128), 1.5).requires_grad_(True)
    qg, kg = ((1.0 + 0.3 * _v("rope." + n, (128,))).requires_grad_(True) for n in ("qg", "kg"))
    cos, sin = qr.rope_tables(1e6, 900)
    positions = torch.tensor([700, 3, 65, 0, 899, 64, 1, 2, 128, 500][:rows_])
    dq, dk, dv = _v("rope.dq", (rows_, Hq, 128)), _v("rope.dk", (rows_, Hkv, 128)), _v("rope.dv", (rows_, Hkv, 128))
    q, k, v = qr.qk_norm_rope(qkv, qg, kg, cos, sin, positions, Hq, Hkv, eps)
    want = _grad((q * dq).sum() + (k * dk).sum() + (v * dv).sum(), (qkv, qg, kg), torch.ones((), dtype=torch.float64))
    got = tr.qk_norm_rope_backward(qkv.detach(), qg.detach(), kg.detach(), cos, sin, positions, dq, dk, dv, Hq, Hkv, eps)
    for g, w in zip(got, want):
        assert _rel(g, w) <= REL
    assert torch.equal(got[0].view(rows_, -1, 128)[:, Hq + Hkv:], dv)


ATT = [(2, 4, 2, 37, 37), (2, 2, 1, 33, 100), (1, 4, 1, 70, 70), (1, 2, 2, 1, 9)]


@pytest.mark.parametrize("B,Hq,Hkv,Lq,T", ATT)
def test_causal_attention_backward_is_autograd(B, Hq, Hkv, Lq, T):
    q, k = _v("att.q", (B, Hq, Lq, 128), 1.7).requires_grad_(True), _v("att.k", (B, Hkv, T, 128), 1.7).requires_grad_(True)
    v, d_o = _v("att.v", (B, Hkv, T, 128)).requires_grad_(True), _v("att.do", (B, Hq, Lq, 128))
    o = qr.causal_attention(q, k, v)
    want = _grad(o, (q, k, v), d_o)
    got = tr.causal_attention_backward(q.detach(), k.detach(), v.detach(), d_o)
    assert _rel(got.o, o.detach()) <= REL
    for g, w in zip((got.dq, got.dk, got.dv), want):
        assert g.shape == w.shape and _rel(g, w) <= REL


@pytest.mark.parametrize("terms,band", [(3, 2.0 ** -12), (1, 2.0 ** -5)])
@pytest.mark.parametrize("B,Hq,Hkv,Lq,T", ATT[:3])
def test_rounded_causal_attention_backward_stays_near_the_exact_one(B, Hq, Hkv, Lq, T, terms, band):
    q, k = _v("att.q", (B, Hq, Lq, 128), 1.7), _v("att.k", (B, Hkv, T, 128), 1.7)
    v, d_o = _v("att.v", (B, Hkv, T, 128)), _v("att.do", (B, Hq, Lq, 128))
    ex, rnd = tr.causal_attention_backward(q, k, v, d_o), tr.rounded_causal_attention_backward(q, k, v, d_o, terms)
    assert _rel(rnd.o, qr.rounded_causal_attention(q, k, v, terms)) == 0.0           # the forward half is tests/qwen3_reference.py's, to the bit
    for name in ("o", "lse", "dq", "dk", "dv"):
        assert getattr(rnd, name).shape == getattr(ex, name).shape
        assert 0.0 < _rel(getattr(rnd, name), getattr(ex, name)) <= band, name


# ------------------------------------------------------------------------------------------------ the module's flags
def _names_with_grad(dec):
    return {n for n, p in dec.named_parameters() if p.requires_grad}


@pytest.mark.parametrize("tied", [True, False])
def test_trainable_layers_sets_the_reference_rules_flags(tied):
    cfg = qr.config(qr.MICRO, tied)
    for K in (0, 1, cfg.num_hidden_layers):
        dec = m2m.Qwen3Decoder(cfg, trainable_layers=K)
        assert _names_with_grad(dec) == tr.trainable_names(cfg, K), K
        assert set(dict(dec.named_parameters())) == set(qr.parameter_shapes(cfg))
    assert _names_with_grad(m2m.Qwen3Decoder(cfg)) == set()


def test_a_bad_trainable_layers_raises():
    cfg = qr.config(qr.MICRO, True)
    for bad in (-1, cfg.num_hidden_layers + 1, 1.5, "all", True):
        with pytest.raises(ValueError, match="trainable_layers"):
            m2m.Qwen3Decoder(cfg, trainable_layers=bad)


def test_workspace_queries_answer_without_a_gpu():
    from mlx8_ws_audio_transformer_amd import ops
    assert ops.causal_attention_backward_workspace_bytes(2, 4, 37, 37) >= 2 * 4 * 37 * 4          # delta [B, Hq, Lq]
    assert ops.causal_attention_backward_workspace_bytes(2, 0, 37, 37) == 0
    assert ops.qk_norm_rope_backward_workspace_bytes(2, 33, 16, 8) >= (5 + 3) * 128 * 4            # ceil(66 * 16 / 256) + ceil(66 * 8 / 256) slabs of 128 floats
    from mlx8_ws_audio_transformer_amd import _lib
    assert int(_lib.lib().awt_op_rmsnorm_param_grad_workspace_bytes(300, 260)) >= 300 * 4 + 2 * 260 * 4   # r per row and two slabs
