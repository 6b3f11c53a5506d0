"""Float64 closed-form restatements, in plain torch, of the backward operators that train through mlx8_ws_audio_transformer_amd.music2midi.Qwen3Decoder
(include/awt.h: awt_op_rmsnorm_backward, awt_op_rmsnorm_param_grad, awt_op_silu_mul_backward, awt_op_qk_norm_rope_backward,
awt_op_causal_attention_backward), and of the reference's rule for what is trained.  No tests here: tests/test_qwen3_train_reference_host.py holds each
formula against torch.autograd.grad of tests/qwen3_reference.py's forward functions, and the GPU tests hold the kernels against the formulas.

    rmsnorm_backward / rmsnorm_param_grad / silu_mul_backward / qk_norm_rope_backward      the formulas of the header, float64
    causal_attention_backward(q, k, v, d_o)              exact: Outputs(o, lse, dq, dk, dv), grouped KV heads, query i sees key j iff j <= T - Lq + i
    rounded_causal_attention_backward(..., terms)        cross_attention_reference.rounded's roundings with the causal bound and the group sum, nothing else
    trainable_names(cfg, K)                              .charles/music2midi/model.py:242-261: the last K layers, the final norm, the head (the tied tensor)

q, d_o: [B, Hq, Lq, 128]; k, v: [B, Hkv, T, 128]; dk / dv come back per KV head, summed over the head's group of Hq / Hkv query heads."""
import torch

from tests import cross_attention_reference as xr
from tests import qwen3_reference as qr

D = 128


# ------------------------------------------------------------------------------------------------ row operators
def rmsnorm_backward(dy, x, gamma, eps, dres=None):
    """dx = [dres +] r u - x r^3 mean(x u), r = rsqrt(mean(x^2) + eps), u = gamma dy."""
    dy, x = dy.double(), x.double()
    r = torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + eps)
    u = gamma.double() * dy
    dx = r * u - x * r.pow(3) * (x * u).mean(-1, keepdim=True)
    return dx if dres is None else dres.double() + dx


def rmsnorm_param_grad(dy, x, eps):
    """dgamma[j] = sum over every leading index of dy[..., j] x[..., j] r."""
    dy, x = dy.double(), x.double()
    r = torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + eps)
    return (dy * x * r).reshape(-1, x.shape[-1]).sum(0)


def silu_mul_backward(gu, dy, I):
    """dgu [..., 2 I] = (dy up s (1 + g (1 - s)) | dy g s), s = sigmoid(g)."""
    g, u, dy = gu.double()[..., :I], gu.double()[..., I:2 * I], dy.double()
    s = torch.sigmoid(g)
    return torch.cat([dy * u * s * (1.0 + g * (1.0 - s)), dy * g * s], dim=-1)


def rotate_back(y, cos, sin):
    """The transposed rotation of tests/qwen3_reference.rotate: a' = a cos + b sin, b' = b cos - a sin for the pair (i, i + 64)."""
    a, b = y[..., :64], y[..., 64:]
    return torch.cat([a * cos + b * sin, b * cos - a * sin], dim=-1)


def qk_norm_rope_backward(qkv, q_gamma, k_gamma, cos, sin, positions, dq, dk, dv, Hq, Hkv, eps):
    """qkv [rows, (Hq + 2 Hkv) 128]; dq [rows, Hq, 128], dk / dv [rows, Hkv, 128] (the gradients of qr.qk_norm_rope's outputs) ->
    (dqkv [rows, (Hq + 2 Hkv) 128], dq_gamma [128], dk_gamma [128])."""
    rows_ = qkv.shape[0]
    x = qkv.double().view(rows_, Hq + 2 * Hkv, D)
    c, s = cos.double()[positions.long()][:, None, :], sin.double()[positions.long()][:, None, :]
    gq, gk = rotate_back(dq.double(), c, s), rotate_back(dk.double(), c, s)
    xq, xk = x[:, :Hq], x[:, Hq:Hq + Hkv]
    dqkv = torch.cat([rmsnorm_backward(gq, xq, q_gamma, eps), rmsnorm_backward(gk, xk, k_gamma, eps), dv.double()], dim=1)
    return dqkv.reshape(rows_, -1), rmsnorm_param_grad(gq, xq, eps), rmsnorm_param_grad(gk, xk, eps)


# ------------------------------------------------------------------------------------------------ causal attention, grouped KV heads
def _group_sum(x, Hkv):
    """[B, Hq, T, 128] -> [B, Hkv, T, 128]: the sum over each KV head's query heads, in ascending head order."""
    B, Hq, T, _ = x.shape
    return x.view(B, Hkv, Hq // Hkv, T, D).sum(2)


def causal_attention_backward(q, k, v, d_o):
    B, Hq, Lq, _ = q.shape
    Hkv, T = k.shape[1], k.shape[2]
    g = Hq // Hkv
    q, d_o = q.double(), d_o.double()
    kk, vv = k.double().repeat_interleave(g, dim=1), v.double().repeat_interleave(g, dim=1)
    s = (q @ kk.transpose(2, 3) * D ** -0.5).masked_fill(~qr.causal_mask(Lq, T, q.device), float("-inf"))
    lse = torch.logsumexp(s, dim=-1)
    p = torch.exp(s - lse[..., None])
    o = p @ vv
    ds = p * (d_o @ vv.transpose(2, 3) - (d_o * o).sum(-1, keepdim=True))
    dq = ds @ kk * D ** -0.5
    return xr.Outputs(o, lse, dq, _group_sum(ds.transpose(2, 3) @ q * D ** -0.5, Hkv), _group_sum(p.transpose(2, 3) @ d_o, Hkv))


def rounded_causal_attention_backward(q, k, v, d_o, terms=3):
    """cross_attention_reference.rounded (forward and backward roundings, its docstring lists them) with two changes and nothing else: a masked score is -1e30 in
    the forward and a masked probability 0 in the backward, and dk / dv are the fp32 roundings of the GROUP's sum (the kernel keeps its accumulators across the
    group's query heads and rounds to the stored value once)."""
    assert terms in (1, 3)
    B, Hq, Lq, _ = q.shape
    Hkv, T = k.shape[1], k.shape[2]
    g = Hq // Hkv
    mask = qr.causal_mask(Lq, T, q.device)
    kk, vv = k.repeat_interleave(g, dim=1), v.repeat_interleave(g, dim=1)
    qh, ql = xr._split(q, terms)
    kh, kl = xr._split(kk, terms)
    vh, vl = xr._split(vv, terms)
    gh, gl = xr._split(d_o, terms)
    f32c = lambda x: float(torch.tensor(x, dtype=torch.float32))
    sc2 = float(torch.tensor(xr.SCALE, dtype=torch.float32) * torch.tensor(xr.LOG2E, dtype=torch.float32))

    s = torch.zeros((B, Hq, Lq, T), dtype=torch.float64, device=q.device)
    for c in range(0, D, 16):
        a_h, a_l, b_h, b_l = qh[..., c:c + 16], ql[..., c:c + 16], kh[..., c:c + 16].transpose(2, 3), kl[..., c:c + 16].transpose(2, 3)
        if terms == 3:
            s = xr._f32(s + a_h @ b_l)
            s = xr._f32(s + a_l @ b_h)
        s = xr._f32(s + a_h @ b_h)
    s2 = xr._f32(s * sc2).masked_fill(~mask, -1.0e30)

    # ---- forward (tests/qwen3_reference.rounded_causal_attention, keeping m and l for the log-sum-exp)
    m = torch.full((B, Hq, Lq), -1.0e30, dtype=torch.float64, device=q.device)
    l = torch.zeros_like(m)
    acc = torch.zeros((B, Hq, Lq, D), dtype=torch.float64, device=q.device)
    for t0 in range(0, T, xr.KEY_TILE):
        st = s2[..., t0:t0 + xr.KEY_TILE]
        m_new = torch.maximum(m, st.max(-1).values)
        alpha = xr._f32(torch.exp2(m - m_new))
        p = xr._f32(torch.exp2(st - m_new[..., None]))
        l = xr._f32(l * alpha + p.sum(-1))
        ph, pl = xr._split(p, terms)
        acc = xr._f32(acc * alpha[..., None] + xr._prod(ph, pl, vh[..., t0:t0 + xr.KEY_TILE, :], vl[..., t0:t0 + xr.KEY_TILE, :], terms))
        m = m_new
    o = xr._f32(acc * xr._f32(1.0 / l)[..., None])
    lse = xr._f32(xr._f32(m + torch.log2(l)) * f32c(xr.LN2))

    # ---- backward
    delta = xr._f32((xr._f32(d_o) * o).sum(-1))
    lse2 = xr._f32(lse * f32c(xr.LOG2E))
    p = xr._f32(torch.exp2(xr._f32(s * sc2 - lse2[..., None]))).masked_fill(~mask, 0.0)
    dp = xr._prod(gh, gl, vh.transpose(2, 3), vl.transpose(2, 3), terms)
    ds = xr._f32(p * xr._f32(dp - delta[..., None]))
    dsh, dsl = xr._split(ds, terms)
    ph, pl = xr._split(p, terms)
    dq = xr._f32(xr._prod(dsh, dsl, kh, kl, terms) * xr.SCALE)
    dk = xr._f32(_group_sum(xr._prod(dsh.transpose(2, 3), dsl.transpose(2, 3), qh, ql, terms), Hkv) * xr.SCALE)
    dv = xr._f32(_group_sum(xr._prod(ph.transpose(2, 3), pl.transpose(2, 3), gh, gl, terms), Hkv))
    return xr.Outputs(o, lse, dq, dk, dv)


# ------------------------------------------------------------------------------------------------ what the reference trains
def trainable_names(cfg, K):
    """The state-dict names with requires_grad under the reference's rule: every parameter of the last K layers, model.norm.weight and the output head --
    `lm_head.weight`, or with tied embeddings the one tensor HF holds under both names, here `model.embed_tokens.weight`."""
    names = {"model.norm.weight", "model.embed_tokens.weight" if cfg.tie_word_embeddings else "lm_head.weight"}
    first = cfg.num_hidden_layers - K
    for name in qr.parameter_shapes(cfg):
        if name.startswith("model.layers.") and int(name.split(".")[2]) >= first:
            names.add(name)
    return names
