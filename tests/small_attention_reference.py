"""Reference of the fp32 head_dim-64 attention family (csrc/decoder_ops.hip: small_attn_fwd_kernel, small_attn_dq_kernel, small_attn_dkv_kernel) in
float64, plain torch, on whatever device the inputs live on.

    exact(q, k, v, d_o, causal, causal_off, keep, p)     float64 autograd of softmax(0.125 q k^T + mask) (keep / (1 - p)) v
    rounded(q, k, v, d_o, causal, causal_off, keep, p)   the same formulas in float64 with the fp32 roundings the three kernels make, and nothing else
    check(...)                                           the bound of the operator tests, per output and per (batch, head):
                                                         max |kernel - exact| <= max(FACTOR x max |rounded - exact|, FACTOR x 2^-23 x max |exact|)

q, d_o: [B, H, Lq, 64]; k, v: [B, H, Sk, 64] (head-major; `rows` / `heads` convert to and from the operator's row-major [B * L, H * 64]).  causal: key j is
visible to query i iff j <= i + causal_off.  keep: the 0/1 pattern `attention_keep_mask(...) > 0` [B, H, Lq, Sk] or None; p: the dropout probability as
the Python float the caller passes.  Both return an `Outputs` of float64 tensors: o [B, H, Lq, 64], lse (natural log, of the UNDROPPED softmax) and
delta = rowsum(d_o * o) [B, H, Lq], dq like q, dk / dv like k.  `exact` forms 1 / (1 - p) in float64 from the Python p: the kernel's fp32
inv_keep = 1 / (1 - fp32(p)) is a rounding of the kernel, which `rounded` restates.

FACTOR (4) is tests/attention_reference.py's: the suite's allowance for a kernel over a same-precision restatement.  The second term of the bound is a
floor of one fp32 ulp-spacing of the head's largest value times that factor: with one visible key the softmax is 1 and the restatement's error can be
exactly 0.  The floor exists only where Sk <= 64.  In a larger case the tolerance is the restatement term alone, so the floor cannot hide a failure
there: it could not merely be asserted to be the smaller term, because for lse it is not -- lse is a handful of fp32 operations from its inputs, the
restatement lands within about one ulp-spacing of float64 (0.3 to 1 x 2^-23 max |lse| over the heads of the operator test's cases), and so does a
correct kernel.

The roundings restated by `rounded`, read off the kernels (every operand is fp32; "rounded" = to fp32):
  * scores: q is multiplied by 0.125 (exact), then the 64-term sum q_i . k_j runs in sixteen groups of four exactly as the kernels' score4 spells it,
    s = rounded(s + fma(q3, k3, fma(q2, k2, fma(q0, k0, rounded(q1 k1))))), one rounding per fma.  All three kernels call score4, the dk / dv kernel on
    the unscaled q with 0.125 applied to the finished sum: the same value, so the backward's P is formed from the very score the forward's lse saw;
  * d_o_i . v_j of the backward: sixteen groups of four as the source writes them, dp += ((g0 v0 + g1 v1) + g2 v2) + g3 v3, every product and every add
    rounded;
  * __expf(x) = exp2(rounded(x * fp32(log2 e))) rounded, on the rounded argument x; __logf(x) = rounded(rounded(log2 x) * fp32(ln 2));
  * wave_sum: the butterfly of csrc/common.h over the 64 lanes, x += shfl_xor(x, 32), 16, 8, 4, 2, 1, rounded at each step (a masked or absent lane holds 0);
  * forward: the 64-key chunk c belongs to wave c % 4; each wave keeps fp32 m, l and o[64] per query row and folds its chunks in order:
    m' = max(m, chunk max), alpha = __expf(m - m'), p = __expf(s - m') (0 for a masked key), l = rounded(rounded(l alpha) + wave_sum(p)),
    o = rounded(o alpha), then o gains p keep inv_keep (rounded) times v in sixteen groups of four keys, each group summed like a group of d_o . v.  l sums
    the undropped p.  A wave starts at m = -3.0e38, l = 0, o = 0, which is also what an idle wave hands to the merge;
  * the four-way merge: M = max m_w, f_w = __expf(m_w - M), L = sum_w rounded(l_w f_w) and O = sum_w rounded(o_w f_w) rounded after each term in wave
    order, o = rounded(O / L), lse = rounded(M + __logf(L));
  * backward: delta = wave_sum(rounded(d_o o)) with the restatement's own fp32 o; P = __expf(rounded(s - lse));
    dS = rounded(P rounded(rounded(dP keep inv_keep) - delta)), 0 for a masked key; inv_keep = fp32(1 / (1 - fp32(p)));
  * dq: per wave over its chunks, sixteen groups of four keys summed like a group of d_o . v; then rounded(((w0 + w1) + (w2 + w3)) 0.125) with
    each sum rounded;
  * dk, dv: one accumulator per key, the query rows in order: dk += rounded(rounded(dS 0.125) q_i), dv += rounded(rounded(P keep inv_keep) d_o_i), rounded
    after each row.
Not restated: what the compiler makes of a group of four outside score4 -- it contracts a multiply and an add into one FMA (one rounding fewer) and now and then adds
the four products of a group in another order (packed instructions) -- and the 1-ulp transcendental instructions (v_exp_f32, v_log_f32, the division).
FACTOR is the allowance for these."""
import collections

import numpy as np
import torch

from tests.attention_reference import FACTOR
from tests.cross_attention_reference import head_errors

D = 64
CHUNK = 64                          # keys per chunk
WAVES = 4                           # chunk c belongs to wave c % WAVES
QB = 16                             # query rows per workgroup
NEG = -3.0e38


def _c32(x):
    return float(torch.tensor(x, dtype=torch.float32))


LOG2E_F, LN2_F, NEG_F = _c32(1.4426950408889634), _c32(0.6931471805599453), _c32(NEG)

Outputs = collections.namedtuple("Outputs", "o lse delta dq dk dv")
NAMES = Outputs._fields

# (B, H, Lq, Sk, causal, causal_off) of the operator test: the smallest shapes that reach each branch of a 16-query tile, a 64-key chunk and a four-wave round robin
CASES = [(1, 1, 1, 1, False, 0), (2, 3, 16, 64, False, 0), (2, 2, 17, 65, False, 0), (1, 2, 15, 63, False, 0),      # exact tiles, one past, one short
         (1, 2, 5, 257, False, 0),                    # wave 0's second chunk holds one live key
         (1, 2, 33, 321, False, 0),                   # two waves with two chunks, two idle in the last round
         (2, 2, 7, 1500, False, 0),                   # the Whisper cross length
         (2, 2, 12, 12, True, 0), (1, 2, 80, 80, True, 0),                                                          # tiles whose kmax falls in different chunks
         (1, 2, 130, 130, True, 0),                   # last tile of 2 rows, third chunk
         (2, 2, 1, 9, True, 8),
         (2, 2, 70, 200, True, 130),                  # backward with a positive offset and Lq > 1: chunks 2 and 3 of the dk / dv kernel start at rows 0 and 62
         (1, 1, 20, 300, True, 280)]                  # the offset diagonal crosses key 256
# (B, H, Lq, Sk, causal, causal_off, p)
DROPOUT_CASES = [(2, 3, 70, 70, False, 0, 0.25), (1, 2, 20, 300, False, 0, 0.1), (2, 2, 40, 40, True, 0, 0.5), (1, 2, 17, 90, True, 73, 0.3)]
DROPOUT_SEED = 20240607


def rows(x):
    """[B, H, L, 64] -> [B * L, H * 64]"""
    B, H, L, _ = x.shape
    return x.permute(0, 2, 1, 3).reshape(B * L, H * D)


def heads(x, B, H):
    """[B * L, H * 64] -> [B, H, L, 64]"""
    return x.reshape(B, -1, H, D).permute(0, 2, 1, 3)


def variates(name, shape, scale=1.0, seed=1):
    """Seeded float32 variates of standard deviation `scale` (the package's counter-based generator: the same values on every machine)."""
    from mlx8_ws_audio_transformer_amd import weights as wts
    return (torch.from_numpy(wts.unit_variates(name, int(np.prod(shape)), seed).reshape(shape)) * scale).float()


def inputs(B, H, Lq, Sk, seed=1):
    """q, k (standard deviation 1.7, the suite's choice for attention), v, d_o (1.0): float32, head-major, on the CPU."""
    return (variates("small.q", (B, H, Lq, D), 1.7, seed), variates("small.k", (B, H, Sk, D), 1.7, seed),
            variates("small.v", (B, H, Sk, D), 1.0, seed), variates("small.d_o", (B, H, Lq, D), 1.0, seed))


def visible(Lq, Sk, causal, causal_off, device=None):
    """[Lq, Sk] bool: key j is visible to query i."""
    i, j = torch.arange(Lq, device=device)[:, None], torch.arange(Sk, device=device)[None, :]
    return (j <= i + causal_off) if causal else torch.ones((Lq, Sk), dtype=torch.bool, device=device)


def visible_count(Lq, Sk, causal, causal_off):
    return visible(Lq, Sk, causal, causal_off).sum(-1)


def exact(q, k, v, d_o, causal=False, causal_off=0, keep=None, p=0.0):
    q, k, v = (t.detach().double().clone().requires_grad_(True) for t in (q, k, v))
    d_o = d_o.detach().double()
    s = 0.125 * (q @ k.transpose(2, 3))
    s = s.masked_fill(~visible(q.shape[2], k.shape[2], causal, causal_off, q.device), float("-inf"))
    P = torch.softmax(s, dim=-1)
    if keep is not None:
        P = P * (keep.to(q.device).double() / (1.0 - p))
    o = P @ v
    dq, dk, dv = torch.autograd.grad(o, (q, k, v), d_o)
    o = o.detach()
    return Outputs(o, torch.logsumexp(s, dim=-1).detach(), (d_o * o).sum(-1), dq, dk, dv)


def _f32(x):
    return x.float().double()


def _expf(x):
    return _f32(torch.exp2(_f32(x * LOG2E_F)))


def _logf(x):
    return _f32(_f32(torch.log2(x)) * LN2_F)


def _wave_sum(x):
    """wave_sum of csrc/common.h over the last dimension (at most 64 lanes, absent ones hold 0): x += shfl_xor(x, 32), 16, ... 1, rounded at each step."""
    if x.shape[-1] < 64:
        x = torch.nn.functional.pad(x, (0, 64 - x.shape[-1]))
    lane = torch.arange(64, device=x.device)
    for o in (32, 16, 8, 4, 2, 1):
        x = _f32(x + x[..., lane ^ o])
    return x[..., 0]


def _sum4(terms):
    """((t0 + t1) + t2) + t3 of rounded products, rounded after each add: a group of four as the source writes it."""
    t = None
    for x in terms:
        t = _f32(x) if t is None else _f32(t + _f32(x))
    return t


def _dot64(a, b, fused=False):
    """a [B, H, Lq, 64] . b [B, H, Sk, 64] -> [B, H, Lq, Sk]: sixteen groups of four, s += ((a0 b0 + a1 b1) + a2 b2) + a3 b3 as the source writes d_o . v,
    or (fused) s += fma(a3, b3, fma(a2, b2, fma(a0, b0, a1 b1))), the kernels' score4.  A product of two fp32 numbers is exact in float64."""
    s = torch.zeros(a.shape[:3] + (b.shape[2],), dtype=torch.float64, device=a.device)
    for e in range(0, D, 4):
        pr = [a[:, :, :, None, e + n] * b[:, :, None, :, e + n] for n in range(4)]
        s = _f32(s + (_f32(pr[3] + _f32(pr[2] + _f32(pr[0] + _f32(pr[1])))) if fused else _sum4(pr)))
    return s


def _mac4(acc, x, y):
    """acc [B, H, L, 64] += ((x0 y0 + x1 y1) + x2 y2) + x3 y3 for x [B, H, L, g], y [B, H, g, 64], g <= 4 (an absent key adds a zero)."""
    return _f32(acc + _sum4(x[..., n, None] * y[:, :, None, n, :] for n in range(x.shape[-1])))


def rounded(q, k, v, d_o, causal=False, causal_off=0, keep=None, p=0.0):
    B, H, Lq, _ = q.shape
    Sk, dev = k.shape[2], q.device
    q, k, v, g = (_f32(t.detach()) for t in (q, k, v, d_o))
    ok = visible(Lq, Sk, causal, causal_off, dev)
    if keep is None:
        ks = torch.ones((B, H, Lq, Sk), dtype=torch.float64, device=dev)
    else:
        one = torch.tensor(1.0, dtype=torch.float32)
        ks = keep.to(dev).double() * float(one / (one - torch.tensor(p, dtype=torch.float32)))
    s = _dot64(q * 0.125, k, fused=True)
    sm = torch.where(ok, s, torch.full_like(s, NEG_F))
    chunks = [(c % WAVES, c * CHUNK, min(Sk, (c + 1) * CHUNK)) for c in range((Sk + CHUNK - 1) // CHUNK)]

    # ---- forward
    m = [torch.full((B, H, Lq), NEG_F, dtype=torch.float64, device=dev) for _ in range(WAVES)]
    l = [torch.zeros((B, H, Lq), dtype=torch.float64, device=dev) for _ in range(WAVES)]
    acc = [torch.zeros((B, H, Lq, D), dtype=torch.float64, device=dev) for _ in range(WAVES)]
    for w, j0, j1 in chunks:
        st = sm[..., j0:j1]
        m_new = torch.maximum(m[w], st.amax(-1))
        alpha = _expf(_f32(m[w] - m_new))
        pc = torch.where(ok[:, j0:j1], _expf(_f32(st - m_new[..., None])), torch.zeros_like(st))
        l[w] = _f32(_f32(l[w] * alpha) + _wave_sum(pc))
        acc[w] = _f32(acc[w] * alpha[..., None])
        pd = _f32(pc * ks[..., j0:j1])
        for j in range(j0, j1, 4):
            acc[w] = _mac4(acc[w], pd[..., j - j0:j - j0 + 4], v[..., j:min(j + 4, j1), :])
        m[w] = m_new
    M = torch.stack(m).amax(0)
    L, O = torch.zeros_like(M), torch.zeros_like(acc[0])
    for w in range(WAVES):
        f = _expf(_f32(m[w] - M))
        L = _f32(L + _f32(l[w] * f))
        O = _f32(O + _f32(acc[w] * f[..., None]))
    o = _f32(O / L[..., None])
    lse = _f32(M + _logf(L))

    # ---- backward
    delta = _wave_sum(_f32(g * o))
    dp = _dot64(g, v)
    P = torch.where(ok, _expf(_f32(s - lse[..., None])), torch.zeros_like(s))
    dS = _f32(P * _f32(_f32(dp * ks) - delta[..., None]))
    pq = [torch.zeros((B, H, Lq, D), dtype=torch.float64, device=dev) for _ in range(WAVES)]
    for w, j0, j1 in chunks:
        for j in range(j0, j1, 4):
            pq[w] = _mac4(pq[w], dS[..., j:min(j + 4, j1)], k[..., j:min(j + 4, j1), :])
    dq = _f32(_f32(_f32(pq[0] + pq[1]) + _f32(pq[2] + pq[3])) * 0.125)
    dS8, Pk = _f32(dS * 0.125), _f32(P * ks)
    dk, dv = torch.zeros_like(k), torch.zeros_like(v)
    for i in range(Lq):
        dk = _f32(dk + _f32(dS8[..., i, :, None] * q[..., i, None, :]))
        dv = _f32(dv + _f32(Pk[..., i, :, None] * g[..., i, None, :]))
    return Outputs(o, lse, delta, dq, dk, dv)


def bound(rnd, ex, name, Sk, factor=FACTOR):
    """Per (batch, head): (tolerance, restatement term, floor term, max |exact|) of one output.  The floor term is 0 where Sk > 64."""
    e_rnd, den = head_errors(getattr(rnd, name), getattr(ex, name))
    restated, floor = factor * e_rnd, factor * 2.0 ** -23 * den * (1.0 if Sk <= CHUNK else 0.0)
    return torch.maximum(restated, floor), restated, floor, den


def check(label, got, rnd, ex, Sk, names=NAMES, factor=FACTOR):
    """Asserts the module's bound per output and per (batch, head); the floor can decide a head only where Sk <= 64.  Prints each output's worst head:
    error and tolerance relative to that head's max |exact| (absolute where that is 0), their ratio, and whether the floor set the tolerance.  Returns
    {name: (rel error, rel tolerance, ratio)} of those heads."""
    report, failed = {}, []
    for name in names:
        x = getattr(got, name)
        e_got, _ = head_errors(x, getattr(ex, name))
        tol, restated, floor, den = bound(rnd, ex, name, Sk, factor)
        unit = torch.where(den > 0, den, torch.ones_like(den))
        ratio = torch.where(e_got > 0, e_got / tol.clamp_min(1e-300), torch.zeros_like(e_got))
        i = int(ratio.argmax())
        rel, rel_tol, by_floor = float((e_got / unit).flatten()[i]), float((tol / unit).flatten()[i]), bool((floor > restated).flatten()[i])
        report[name] = (rel, rel_tol, float(ratio.max()))
        finite = bool(torch.isfinite(x).all())
        print(f"{label} {name}: worst head err {rel:.3e} tol {rel_tol:.3e} ({float(ratio.max()):.2f} of tol{', floor' if by_floor else ''})"
              + ("" if finite else " NOT FINITE"))
        if not finite or not bool((e_got <= tol).all()):
            failed.append(name)
    assert not failed, (label, failed, report)
    return report
