"""Reference of the head_dim-128 cross-attention operator pair (csrc/cross_attention.hip) in float64, plain torch, on whatever device the inputs live on.

    exact(q, k, v, d_o)            float64 autograd of softmax(128^-1/2 q k^T) v
    rounded(q, k, v, d_o, terms)   the same formulas in float64 with the roundings the kernels make, and nothing else
    check(...)                     the bound of the operator tests: the kernel may be FACTOR (4) x as far from `exact` as `rounded` is, per output and per
                                   (batch, head); FACTOR is tests/attention_reference.py's, the suite's allowance for a kernel over a same-precision restatement

q, d_o: [B, H, Lq, 128]; k, v: [B, H, Sk, 128] (head-major; `rows` / `heads` convert to and from the operator's row-major [B * L, H * 128]).  Both return
an `Outputs` of float64 tensors: o [B, H, Lq, 128], lse (natural log) [B, H, Lq], dq like q, dk / dv like k.

The roundings restated by `rounded`, read off the kernels (terms = 3 is split-bf16: every operand a hi + lo pair of bf16 values, hi = rne(x), lo = rne(x - hi),
and a product of two operands is a_lo b_hi + a_hi b_lo + a_hi b_hi -- lo x lo is never formed; terms = 1 keeps hi only):
  * q, k, v and d_o are split from fp32 as they are (the score scale is NOT folded into q);
  * scores: the fp32 accumulator is rounded after each MFMA, i.e. after each 16-wide step of each of the three products (k_lo q_hi, k_hi q_lo, k_hi q_hi), then
    multiplied by fp32(fp32(128^-1/2) log2 e) in fp32;
  * forward: online softmax over tiles of 64 keys with fp32 running max m, sum l and output: p = exp2(s - m) rounded to fp32, l sums the UNSPLIT p, P is split
    per tile and multiplies the split v, the fp32 output accumulator is rescaled and rounded once per tile; o = acc * fp32(1 / l); lse = fp32((m + log2 l) ln 2);
  * backward: delta = fp32(rowsum(d_o * o)) from the fp32 tensors; lse2 = fp32(lse log2 e); P = exp2(fp32(fma(s, scale log2 e, -lse2))) rounded to fp32;
    dP = d_o v^T on split operands; dS = fp32(P fp32(dP - delta)); dS and P are split and multiply the split k, q and d_o;
    dq = fp32(128^-1/2 dS k), dk = fp32(128^-1/2 dS^T q), dv = fp32(P^T d_o).
Not restated: the order of the fp32 sums inside a product (beyond the per-step rounding of the scores; the dk / dv launch forms its scores with the two cross
products in the other order), v_exp_f32 / v_log_f32 / v_rcp_f32, and the tile order of the gradient accumulators.  FACTOR is the allowance for them."""
import collections
import math

import torch

from tests.attention_reference import FACTOR

D = 128
KEY_TILE = 64
LOG2E = 1.4426950408889634
LN2 = 0.6931471805599453
SCALE = float(torch.tensor(0.08838834764831845, dtype=torch.float32))

Outputs = collections.namedtuple("Outputs", "o lse dq dk dv")
NAMES = Outputs._fields


def rows(x):
    """[B, H, L, 128] -> [B * L, H * 128]"""
    B, H, L, _ = x.shape
    return x.permute(0, 2, 1, 3).reshape(B * L, H * D)


def heads(x, B, H):
    """[B * L, H * 128] -> [B, H, L, 128]"""
    return x.reshape(B, -1, H, D).permute(0, 2, 1, 3)


def _f32(x):
    return x.float().double()


def _bf16(x):
    return x.float().bfloat16().double()


def _split(x, terms):
    x = _f32(x)
    hi = _bf16(x)
    return hi, (_bf16(x - hi) if terms == 3 else torch.zeros_like(hi))


def _prod(ah, al, bh, bl, terms):
    return ah @ bh + (ah @ bl + al @ bh if terms == 3 else 0.0)


def exact(q, k, v, d_o):
    q, k, v = (t.detach().double().clone().requires_grad_(True) for t in (q, k, v))
    s = q @ k.transpose(2, 3) * (D ** -0.5)
    o = torch.softmax(s, dim=-1) @ v
    dq, dk, dv = torch.autograd.grad(o, (q, k, v), d_o.detach().double())
    return Outputs(o.detach(), torch.logsumexp(s, dim=-1).detach(), dq, dk, dv)


def rounded(q, k, v, d_o, terms=3):
    assert terms in (1, 3)
    B, H, Lq, _ = q.shape
    Sk = k.shape[2]
    qh, ql = _split(q, terms)
    kh, kl = _split(k, terms)
    vh, vl = _split(v, terms)
    gh, gl = _split(d_o, terms)
    sc2 = float(torch.tensor(SCALE, dtype=torch.float32) * torch.tensor(LOG2E, dtype=torch.float32))

    s = torch.zeros((B, H, Lq, Sk), dtype=torch.float64, device=q.device)
    for c in range(0, D, 16):
        a_h, a_l, b_h, b_l = qh[..., c:c + 16], ql[..., c:c + 16], kh[..., c:c + 16].transpose(2, 3), kl[..., c:c + 16].transpose(2, 3)
        if terms == 3:
            s = _f32(s + a_h @ b_l)          # k_lo q_hi
            s = _f32(s + a_l @ b_h)          # k_hi q_lo
        s = _f32(s + a_h @ b_h)
    s2 = _f32(s * sc2)

    # ---- forward
    m = torch.full((B, H, Lq), -1.0e30, dtype=torch.float64, device=q.device)
    l = torch.zeros_like(m)
    acc = torch.zeros((B, H, Lq, D), dtype=torch.float64, device=q.device)
    for t0 in range(0, Sk, KEY_TILE):
        st = s2[..., t0:t0 + KEY_TILE]
        m_new = torch.maximum(m, st.max(-1).values)
        alpha = _f32(torch.exp2(m - m_new))
        p = _f32(torch.exp2(st - m_new[..., None]))
        l = _f32(l * alpha + p.sum(-1))
        ph, pl = _split(p, terms)
        acc = _f32(acc * alpha[..., None] + _prod(ph, pl, vh[..., t0:t0 + KEY_TILE, :], vl[..., t0:t0 + KEY_TILE, :], terms))
        m = m_new
    o = _f32(acc * _f32(1.0 / l)[..., None])
    lse = _f32(_f32(m + torch.log2(l)) * float(torch.tensor(LN2, dtype=torch.float32)))

    # ---- backward
    delta = _f32((_f32(d_o) * o).sum(-1))
    lse2 = _f32(lse * float(torch.tensor(LOG2E, dtype=torch.float32)))
    p = _f32(torch.exp2(_f32(s * sc2 - lse2[..., None])))
    dp = _prod(gh, gl, vh.transpose(2, 3), vl.transpose(2, 3), terms)
    ds = _f32(p * _f32(dp - delta[..., None]))
    dsh, dsl = _split(ds, terms)
    ph, pl = _split(p, terms)
    dq = _f32(_prod(dsh, dsl, kh, kl, terms) * SCALE)
    dk = _f32(_prod(dsh.transpose(2, 3), dsl.transpose(2, 3), qh, ql, terms) * SCALE)
    dv = _f32(_prod(ph.transpose(2, 3), pl.transpose(2, 3), gh, gl, terms))
    return Outputs(o, lse, dq, dk, dv)


def head_errors(x, ex):
    """(max |x - exact|, max |exact|) per (batch, head), each [B, H]."""
    B, H = ex.shape[:2]
    x, ex = x.double().reshape(B, H, -1), ex.reshape(B, H, -1)
    return (x - ex).abs().amax(-1), ex.abs().amax(-1)


def check(label, got, rnd, ex, names=NAMES, factor=FACTOR):
    """Asserts, per output and per (batch, head): max |got - exact| <= factor x max |rounded - exact|.  Prints each output's worst head (relative to that
    head's max |exact|) beside its bound; returns {name: (rel error, rel tol)} of those heads."""
    report, failed = {}, []
    for name in names:
        e_got, den = head_errors(getattr(got, name), getattr(ex, name))
        e_rnd, _ = head_errors(getattr(rnd, name), getattr(ex, name))
        tol = factor * e_rnd
        unit = torch.where(den > 0, den, torch.ones_like(den))
        ratio = torch.where(e_got > 0, e_got / tol.clamp_min(1e-300), torch.zeros_like(e_got))
        i = int(ratio.argmax())
        rel, rel_tol = float((e_got / unit).flatten()[i]), float((tol / unit).flatten()[i])
        report[name] = (rel, rel_tol)
        finite = bool(torch.isfinite(getattr(got, name)).all())
        print(f"{label} {name}: worst head err {rel:.3e} tol {rel_tol:.3e} ({float(ratio.max()):.2f} of tol)" + ("" if finite else " NOT FINITE"))
        if not finite or not bool((e_got <= tol).all()):
            failed.append(name)
    assert not failed, (label, failed, report)
    return report


def ulp32(x):
    return 2.0 ** (math.floor(math.log2(abs(x))) - 23)
