"""Reference of the encoder's attention training pass (csrc/attention.hip in its training form, csrc/attention_bwd.hip) in float64, plain torch,
on whatever device the inputs live on.

    exact(q, k, v, d_o)                       float64 autograd of softmax(q k^T) v
    rounded(q, k, v, d_o, terms, grad_terms)  the same formulas in float64 with the roundings the kernels make, and nothing else
    rounded(q, k, v, None, terms)             its forward half alone, as awt_op_attention stores it (o in fp32, lse2); also terms 2 and 4
    check(...)                                the bound of the operator tests: the kernel may be 4 x as far from `exact` as `rounded` is

q (pre-scaled by head_dim^-1/2), k, v: [B, H, S, 64]; d_o: [B, S, H * 64].  Both return an `Outputs` of float64 tensors: o [B, S, H * 64], lse2 (the
log-sum-exp of each score row in log2 units) and delta = rowsum(d_o * o) [B, H, S], dq (times qscale), dk, dv [B, H, S, 64].

The roundings restated by `rounded`, read off the two kernels (terms = 3 is split-bf16: every operand a hi + lo pair of bf16 values, hi = rne(x),
lo = rne(x - hi), and a product of two operands is a_hi b_hi + a_hi b_lo + a_lo b_hi -- the lo x lo term is never formed; terms = 1 keeps hi only;
terms = 4 / 2 are the same on fp16 planes, forward only -- common.h split16<true>: hi = fp16(x), lo = fp16(x - hi), no power-of-two scale on lo, so a
lo below 2^-24 is lost and one below 2^-14 keeps fewer than 11 bits):
  * q log2(e) (an fp32 product), k, v and d_o are split;
  * scores: the fp32 accumulator is rounded after each MFMA, i.e. after each 16-wide step of each of the three products (at logits of order 100 one
    fp32 ulp of the exponent is 1e-5 of a probability, the size of the split-bf16 error itself);
  * forward: online softmax over tiles of 64 keys, P = exp2(s - running max) split per tile, o split into the planes the backward reads, lse2 in fp32;
  * backward: delta from the joined planes in fp32; P = exp2(s - lse2); dP = d_o v^T, then dS = P (dP - delta) and P are split and multiply k, q log2(e)
    and d_o; the gradient contractions (dP, dQ, dK, dV) take `grad_terms` products while the scores keep `terms`;
  * dq is scaled by qscale, dk by ln 2 (it was formed against q log2(e)), and all three are stored as hi + lo planes (hi alone with terms = 1).
Not restated: the order of the fp32 sums inside a product and v_exp_f32 / v_log_f32; the factor 4 of `check` is the allowance for them, the one the
suite gives a kernel over a same-precision restatement (LN_DX_TOL of tests/test_gpu_native_decoder.py)."""
import collections
import math

import torch

LOG2E = 1.4426950408889634
LN2 = 0.6931471805599453
KEY_TILE = 64                       # keys per streamed tile of the forward kernel
FACTOR = 4.0

Outputs = collections.namedtuple("Outputs", "o lse2 delta dq dk dv")
NAMES = Outputs._fields


def _f32(x):
    return x.float().double()


def _bf16(x):
    return x.float().bfloat16().double()          # round-to-nearest-even, as v_cvt_pk_bf16_f32


def _fp16(x):
    return x.float().half().double()               # round-to-nearest-even, as v_cvt_f16_f32; subnormals kept


PRODUCTS = {1: 1, 2: 1, 3: 3, 4: 3}                # common.h prec_products: terms 1 / 3 on bf16 planes, 2 / 4 on fp16 planes


def _split(x, terms):
    x = _f32(x)
    rne = _bf16 if terms in (1, 3) else _fp16
    hi = rne(x)
    return hi, (rne(x - hi) if PRODUCTS[terms] == 3 else torch.zeros_like(hi))


def _prod(ah, al, bh, bl, terms):
    """a b for split operands: the hi x lo and lo x hi products join hi x hi only with three terms."""
    return ah @ bh + (ah @ bl + al @ bh if PRODUCTS[terms] == 3 else 0.0)


def _heads(x, H):
    """[B, S, H * 64] -> [B, H, S, 64]"""
    B, S, _ = x.shape
    return x.reshape(B, S, H, 64).permute(0, 2, 1, 3)


def _rows(x):
    """[B, H, S, 64] -> [B, S, H * 64]"""
    B, H, S, _ = x.shape
    return x.permute(0, 2, 1, 3).reshape(B, S, H * 64)


def exact(q, k, v, d_o, qscale=1.0):
    q, k, v = (t.detach().double().clone().requires_grad_(True) for t in (q, k, v))
    d_o = d_o.detach().double()
    s = q @ k.transpose(2, 3)
    o = torch.softmax(s, dim=-1) @ v
    dq, dk, dv = torch.autograd.grad(o, (q, k, v), _heads(d_o, q.shape[1]))
    lse2 = torch.logsumexp(s, dim=-1) * LOG2E
    delta = (_heads(d_o, q.shape[1]) * o).sum(-1)
    return Outputs(_rows(o).detach(), lse2.detach(), delta.detach(), dq * qscale, dk, dv)


def rounded(q, k, v, d_o, terms=3, grad_terms=None, qscale=1.0, drop=()):
    """`drop` names lo planes to lose on purpose, for the test that the bound tells such a loss apart: "ds_lo" (the lo plane of dS in the products
    that form dq and dk), "p_lo" (the lo plane of P in the product that forms dv)."""
    gt = terms if grad_terms is None else grad_terms
    assert terms in PRODUCTS and (gt == terms or (terms == 3 and gt == 1)) and not set(drop) - {"ds_lo", "p_lo"}
    assert d_o is None or terms in (1, 3)                                # the backward kernels have no fp16 form
    B, H, S, _ = q.shape
    qh, ql = _split(q.float() * torch.tensor(LOG2E, dtype=torch.float32), terms)
    kh, kl = _split(k, terms)
    vh, vl = _split(v, terms)

    s = torch.zeros((B, H, S, S), dtype=torch.float64, device=q.device)
    for c in range(0, 64, 16):
        a_h, a_l, b_h, b_l = qh[..., c:c + 16], ql[..., c:c + 16], kh[..., c:c + 16].transpose(2, 3), kl[..., c:c + 16].transpose(2, 3)
        if PRODUCTS[terms] == 3:
            s = _f32(s + a_l @ b_h)
            s = _f32(s + a_h @ b_l)
        s = _f32(s + a_h @ b_h)

    # ---- forward, training form
    m = torch.full((B, H, S), -1.0e30, dtype=torch.float64, device=q.device)
    l = torch.zeros_like(m)
    acc = torch.zeros((B, H, S, 64), dtype=torch.float64, device=q.device)
    for t0 in range(0, S, KEY_TILE):
        st = s[..., t0:t0 + KEY_TILE]
        m_new = torch.maximum(m, st.max(-1).values)
        alpha = torch.exp2(m - m_new)
        p = torch.exp2(st - m_new[..., None])
        l = l * alpha + p.sum(-1)
        ph, pl = _split(p, terms)
        acc = acc * alpha[..., None] + _prod(ph, pl, vh[..., t0:t0 + KEY_TILE, :], vl[..., t0:t0 + KEY_TILE, :], terms)
        m = m_new
    lse2 = _f32(m + torch.log2(l))
    if d_o is None:                                                      # the fp32 store of awt_op_attention: no output planes
        return Outputs(_rows(_f32(acc / l[..., None])), lse2, None, None, None, None)
    oh, ol = _split(acc / l[..., None], terms)
    doh, dol = _split(_heads(d_o, H), terms)

    # ---- backward
    delta = _f32(((doh + dol) * (oh + ol)).sum(-1))
    gl = lambda lo: lo if gt == 3 else torch.zeros_like(lo)             # operand lo planes the gradient contractions read
    p = torch.exp2(s - lse2[..., None])
    dp = _prod(doh, gl(dol), vh.transpose(2, 3), gl(vl).transpose(2, 3), gt)
    dsh, dsl = _split(p * (dp - delta[..., None]), gt)
    ph, pl = _split(p, gt)
    if "ds_lo" in drop:
        dsl = torch.zeros_like(dsl)
    if "p_lo" in drop:
        pl = torch.zeros_like(pl)
    dq = _prod(dsh, dsl, kh, gl(kl), gt) * torch.tensor(qscale, dtype=torch.float32).double()
    dk = _prod(dsh.transpose(2, 3), dsl.transpose(2, 3), qh, gl(ql), gt) * torch.tensor(LN2, dtype=torch.float32).double()
    dv = _prod(ph.transpose(2, 3), pl.transpose(2, 3), doh, gl(dol), gt)
    join = lambda x: sum(_split(x, terms))
    return Outputs(_rows(oh + ol), lse2, delta, join(dq), join(dk), join(dv))


def per_head(name, x):
    """Any output as [B, H, n]: what one (batch, head) pair owns."""
    if name == "o":
        x = _heads(x, x.shape[2] // 64)
    return x.reshape(x.shape[0], x.shape[1], -1)


def head_errors(name, x, ex):
    """(max |x - exact|, max |exact|) per (batch, head), each [B, H]."""
    x, ex = per_head(name, x.double()), per_head(name, ex)
    return (x - ex).abs().amax(-1), ex.abs().amax(-1)


def cancellation_floor(q, k, v, d_o, ex, qscale=1.0):
    """Per-head bound of what fp32 summation alone puts into dq and dk: dS = P (dP - delta) subtracts two 64-term fp32 sums, each off by at most
    64 x 2^-24 times the sum of its terms' magnitudes (first order), so |error(dS)| <= 2^-18 P (|d_o| |v|^T + rowsum |d_o o|), carried through
    dq = dS k and dk = dS^T q.  `check` uses it only where a head's exact gradient is itself below it -- the gradient is cancellation and nothing
    else, and a relative bound has no denominator.  That is the case at S = 1: softmax of one score is 1, dS = dP - delta = 0 identically."""
    H = q.shape[1]
    q, k, v, do = q.double(), k.double(), v.double(), _heads(d_o.double(), H)
    p = torch.softmax(q @ k.transpose(2, 3), dim=-1)
    e = 2.0 ** -18 * p * (do.abs() @ v.abs().transpose(2, 3) + (do * _heads(ex.o, H)).abs().sum(-1, keepdim=True))
    return {"dq": (e @ k.abs()).amax((-1, -2)) * abs(qscale), "dk": (e.transpose(2, 3) @ q.abs()).amax((-1, -2))}


def check(label, got, rnd, ex, floor=None, names=NAMES, factor=FACTOR):
    """Asserts, per output and per (batch, head): max |got - exact| <= factor x max |rounded - exact| -- the relative form of the bound with both
    sides normalised by the same max |exact| of that head.  Prints each output's worst head beside its bound; returns {name: (rel error, rel tol)}
    of those heads.  `floor`: cancellation_floor(...)."""
    report, failed = {}, []
    for name in names:
        e_got, den = head_errors(name, getattr(got, name), getattr(ex, name))
        e_rnd, _ = head_errors(name, getattr(rnd, name), getattr(ex, name))
        tol = factor * e_rnd
        if floor is not None and name in floor:
            tol = torch.where(den <= floor[name], torch.maximum(tol, floor[name]), tol)
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
    """One unit in the last place of the fp32 number of magnitude x."""
    return 2.0 ** (math.floor(math.log2(abs(x))) - 23)
