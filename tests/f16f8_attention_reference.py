"""Reference of the f16f8 attention forward (csrc/attention_f8.hip, attention_f16f8_pipe_kernel in both of its forms; one launch through
awt_op_attention_ex) in float64, plain torch, on whatever device the inputs live on.

    exact(q, k, v)                               softmax(q k^T) v and the log-sum-exp, no rounding
    rounded(q, k, v, pv8)                        the same formulas with the roundings the kernel makes, and nothing else
    perturbed(q, k, v, pv8, ulps, seed)          `rounded` with every score and every probability multiplied by 1 + u 2^-24, u uniform in +-ulps:
                                                 the yardstick for "the same arithmetic in another order"
    rounded(..., defect=name)                    one wrong formula planted (DEFECTS), for the host test that the bounds tell it from a correct kernel
    bounds(q, k, v, pv8)                         (exact, rounded, yardstick) of one input; check_forward(label, got, *bounds) asserts (a), (b), (c)

q (pre-scaled by head_dim^-1/2), k, v: [B, H, S, 64].  All return attention_reference.Outputs with o [B, S, H * 64] and lse2 [B, H, S] (the log-sum-exp
of each score row in log2 units) as float64 tensors and None for the backward's fields.  pv8 = True: the forms that keep P V's two e4m3 cross terms
("attn_shape" 4 and 5, the training forward); pv8 = False: P V as one fp16 product ("attn_shape" 6, the encoder's inference default).

Roundings restated, read off the kernel and common.h (number formats: tests/gemm_reference.py):
  * each operand is three images (launch_split_planes): x16 = fp16(x), x8 = e4m3(x 2^s) 2^-s, xl8 = e4m3((x - x16) 2^(s + 11)) 2^-(s + 11),
    s = kF8Q = 2 for q, kF8KV = 0 for k and v.  For q, x = q log2(e), and all three are made from the scaled q.  The source names x as an fp32
    product.  In the compiled split kernel (device code is built with floating-point contraction on) that product is fused into what consumes it
    for the first and the last element of each float4 it loads -- x16 is ONE rounding of the exact 48-bit product (v_fma_mixlo_f16) and x - x16 one
    fused multiply-add, rounded to fp32 once (v_fma_mix_f32) -- while the two middle elements (v_pk_mul_f32) and every x8 see the product rounded to
    fp32: FUSED below.  With scale 1 (k, v) the two are the same.  It matters because (fp32(x) - x16) 2^(s + 11) is a multiple of 2^-12 or coarser
    and sits on an e4m3 tie in about 1.4 % of the elements, which the unrounded product breaks the other way half the time: restated with the fp32 product
    throughout, one lo8 byte of q in 290 and one fp16 value in 26000 differ from the kernel's (measured on 131072 elements), a score moves by up to
    7.6e-5 and lse2 by up to 4.9e-5, which is 3 to 6 x bound (b).  From the kernel's own images the scores agree to 1.4e-6 (3 ulp).
    test_gpu_f16f8_attention.test_operand_images pins all nine images byte for byte, so a compiler that fuses differently shows there first;
  * scores (qk_mma, per 32-key sub-tile), in MFMA order:  k8 . ql8  (one 64-deep scaled MFMA into a zero accumulator),  + kl8 . q8  (one more),
    + k16 . q16 in four 16-deep steps; the fp32 accumulator is rounded after each of the six MFMAs;
  * online softmax over tiles of 64 keys: running maximum m, alpha = exp2(m_old - m) and P = exp2(s - m) as fp32 values of an fp32 difference; keys
    >= S of the last tile are masked (P = 0);
  * the normaliser l = l alpha + sum(P) sums the UNROUNDED fp32 P;
  * O = O alpha (fp32), then + fp16(P) . v16 in four 16-key MFMA steps, the accumulator rounded after each; with pv8
    + e4m3((P - fp16(P)) 2^19) . v8  and  + e4m3(P 2^8) . vl8, one 64-key scaled MFMA each, in that order (kF8P = 8);
  * o = O * fp32(1 / l) in fp32; lse2 = m + log2(l) in fp32 (v_log_f32 is a base-2 logarithm).
Not restated: the order of the fp32 sums inside one MFMA and of the row sum, v_exp_f32, v_log_f32 and v_rcp_f32 (each good to about an ulp).  `perturbed`
is the allowance for them: ULPS fp32 ulp on every score and every probability.  ULPS was 16 as first written -- the two places where the kernel forms a
score (prologue and loop), the online rescale, and one v_exp_f32 / v_log_f32 each come to a few ulp; tests/test_gpu_attention_backward.py budgets 8 for
two launches -- and is 32 since the first GPU run, for one term: the sum order inside an MFMA.  Its error is an ulp or two of the PARTIAL sums (|q . k|
over 16 dims is 4 .. 10), whatever the size of the score: from the kernel's own operand images, 2048 single-key scores (S = 1, lse2 is the score)
differ from the restated ones by up to 1.43e-6, which is 24 x 2^-24 |s| at |s| = 1.  A multiplicative 16 under-budgets every score below 1.5, and
(c) was missed once, by 1.23 x, on one of the 256 heads of (B 8, H 32, S 8) -- eight keys, where single roundings of P decide the norm; every other case
of the GPU file was inside all three bounds with 16 (worst (b) 0.50, worst (c) 1.00).  32 covers 1.43e-6 down to |s| = 0.75.

Bounds, all computed from this file alone, per (batch, head):
  (a) max |x - exact| <= 4 x max |rounded - exact| for o and lse2 (attention_reference.check, the suite's factor 4);
  (b) max |lse2 - rounded.lse2| <= max over SEEDS of max |perturbed.lse2 - rounded.lse2|;
  (c) ||o - rounded.o||_2 / ||exact.o||_2 <= the same of `perturbed`, maximum over SEEDS.
Why three: with pv8 = False the single fp16 rounding of P (2^-12 of a head's |o|) dominates (a), which cannot see the logits; lse2 depends on the logits
alone (the normaliser sums the unrounded P), and the L2 norm averages over the fp16 roundings of P that flip under any reordering while the maximum is
one of them.  tests/test_f16f8_attention_reference_host.py measures what each bound tells apart; its docstring has the figures.

DEFECTS (what each leaves untouched is asserted by the host test):
  q_lo             the k8 . ql8 term lost                                              moves o and lse2
  k_lo             the kl8 . q8 term lost                                              moves o and lse2
  q_hi8_unscaled   q8 made from q instead of q log2(e)                                 moves o and lse2
  scale_lo         ql8 read at 2^-(s + 10) instead of 2^-(s + 11): k8 . ql8 doubled    moves o and lse2
  tail_key         the first masked key of a partial last tile not masked; the LDS-DMA clamps its row to the last key, so that key counts twice
                   (S % 64 != 0 only)                                                  moves o and lse2
  stale_v_tile     P V of tile ntiles / 2 taken with the previous tile's V, what a wrong ring slot does (>= 3 tiles only)
                                                                                       moves o; lse2 bit-equal
  p_lo             pv8 only: the pl8 . v8 term lost                                    moves o; lse2 bit-equal"""
import torch

from tests.attention_reference import FACTOR, KEY_TILE, LOG2E, Outputs, _rows, check, head_errors, per_head
from tests.gemm_reference import F8_KV, F8_LO, F8_Q, _e4m3, _f32, _fp16

F8_P = 8                                 # common.h kF8P
ULPS = 32
SEEDS = (0, 1, 2)
DEFECTS = ("q_lo", "k_lo", "q_hi8_unscaled", "scale_lo", "tail_key", "stale_v_tile", "p_lo")
LOGIT_DEFECTS = DEFECTS[:4]


def _out(o, lse2):
    return Outputs(o, lse2, None, None, None, None)


def exact(q, k, v):
    q, k, v = q.double(), k.double(), v.double()
    s = q @ k.transpose(2, 3)
    return _out(_rows(torch.softmax(s, dim=-1) @ v), torch.logsumexp(s, dim=-1) * LOG2E)


def can_act(defect, S, pv8):
    """Whether the defect changes anything at this length and form."""
    ntiles = -(-S // KEY_TILE)
    return {"tail_key": S % KEY_TILE != 0, "stale_v_tile": ntiles >= 3, "p_lo": pv8}.get(defect, True)


def _fp16_once(x):
    """float64 -> binary16 in ONE rounding to nearest even (torch converts a double through float32: two roundings); least exponent -14, 10 mantissa bits."""
    _, e = torch.frexp(x.abs())
    step = torch.exp2((e - 1).clamp_min(-14).double() - 10)
    return torch.round(x / step) * step


FUSED = (True, False, False, True)       # of each float4 of the split kernel: the elements whose product with `scale` is contracted (module docstring)


def _images(x, s, scale=None):
    """The three images launch_split_planes writes of x * scale (x float32 [..., 64], scale a float32 scalar), as the compiled kernel forms them."""
    xd = x.float().double() * (1.0 if scale is None else float(torch.tensor(scale, dtype=torch.float32)))      # 24 x 24 bits: exact in float64
    x32 = _f32(xd)
    fused = torch.tensor(FUSED, device=x.device).repeat(x.shape[-1] // 4)
    x16 = torch.where(fused, _fp16_once(xd), _fp16(x32))
    return x16, _e4m3(x32, s), _e4m3(torch.where(fused, _f32(xd - x16), x32 - x16), s + F8_LO)


def rounded(q, k, v, pv8, defect=None, ulps=0, seed=0):
    assert defect is None or (defect in DEFECTS and can_act(defect, q.shape[2], pv8)), defect
    B, H, S, _ = q.shape
    ntiles = -(-S // KEY_TILE)
    gen = torch.Generator(device=q.device).manual_seed(seed)

    def wobble(x):                        # x (1 + u 2^-24), u uniform in +-ulps
        if not ulps:
            return x
        u = (torch.rand(x.shape, generator=gen, device=x.device, dtype=torch.float64) * 2.0 - 1.0) * ulps
        return x * (1.0 + u * 2.0 ** -24)

    q16, q8, ql8 = _images(q, F8_Q, LOG2E)
    if defect == "q_hi8_unscaled":
        q8 = _e4m3(_f32(q), F8_Q)
    k16, k8, kl8 = _images(k, F8_KV)
    v16, v8, vl8 = _images(v, F8_KV)

    t = lambda a: a.transpose(2, 3)
    s = torch.zeros((B, H, S, S), dtype=torch.float64, device=q.device)
    if defect != "q_lo":
        s = _f32(ql8 @ t(k8)) * (2.0 if defect == "scale_lo" else 1.0)
    if defect != "k_lo":
        s = _f32(s + q8 @ t(kl8))
    for c in range(0, 64, 16):
        s = _f32(s + q16[..., c:c + 16] @ t(k16[..., c:c + 16]))
    s = wobble(s)

    m = torch.full((B, H, S), -1.0e30, dtype=torch.float64, device=q.device)
    l = torch.zeros_like(m)
    acc = torch.zeros((B, H, S, 64), dtype=torch.float64, device=q.device)
    for kt in range(ntiles):
        t0, t1 = kt * KEY_TILE, min(S, (kt + 1) * KEY_TILE)
        st = s[..., t0:t1]
        v0 = t0 - KEY_TILE if (defect == "stale_v_tile" and kt == ntiles // 2) else t0
        tv16, tv8, tvl8 = (a[..., v0:v0 + (t1 - t0), :] for a in (v16, v8, vl8))
        if defect == "tail_key" and kt == ntiles - 1:
            st = torch.cat([st, st[..., -1:]], dim=-1)
            tv16, tv8, tvl8 = (torch.cat([a, a[..., -1:, :]], dim=2) for a in (tv16, tv8, tvl8))
        m_new = torch.maximum(m, st.max(-1).values)
        alpha = _f32(torch.exp2(_f32(m - m_new)))
        p = wobble(_f32(torch.exp2(_f32(st - m_new[..., None]))))
        l = _f32(l * alpha + p.sum(-1))
        p16 = _fp16(p)
        acc = _f32(acc * alpha[..., None])
        for c in range(0, st.shape[-1], 16):
            acc = _f32(acc + p16[..., c:c + 16] @ tv16[..., c:c + 16, :])
        if pv8:
            if defect != "p_lo":
                acc = _f32(acc + _e4m3(p - p16, F8_P + F8_LO) @ tv8)
            acc = _f32(acc + _e4m3(p, F8_P) @ tvl8)
        m = m_new
    o = _f32(acc * _f32(1.0 / l)[..., None])
    return _out(_rows(o), _f32(m + _f32(torch.log2(l))))


def perturbed(q, k, v, pv8, ulps=ULPS, seed=0):
    return rounded(q, k, v, pv8, ulps=ulps, seed=seed)


def lse_distance(x, rnd):
    """(b): max |lse2 - rounded.lse2| per (batch, head), [B, H]"""
    return (x.lse2.double() - rnd.lse2).abs().amax(-1)


def o_distance(x, rnd, ex):
    """(c): ||o - rounded.o||_2 / ||exact.o||_2 per (batch, head), [B, H]"""
    d = per_head("o", x.o.double() - rnd.o)
    return torch.linalg.vector_norm(d, dim=-1) / torch.linalg.vector_norm(per_head("o", ex.o), dim=-1)


def yardstick(q, k, v, pv8, rnd, ex, ulps=ULPS, seeds=SEEDS):
    """(bound of (b), bound of (c)), each [B, H]: the greatest distance of `perturbed` from `rounded` over the seeds."""
    runs = [perturbed(q, k, v, pv8, ulps, seed) for seed in seeds]
    return (torch.stack([lse_distance(r, rnd) for r in runs]).amax(0), torch.stack([o_distance(r, rnd, ex) for r in runs]).amax(0))


def bounds(q, k, v, pv8, ulps=ULPS):
    ex, rnd = exact(q, k, v), rounded(q, k, v, pv8)
    return ex, rnd, yardstick(q, k, v, pv8, rnd, ex, ulps)


def ratios(got, ex, rnd, yard):
    """{bound: distance / bound per (batch, head)} for "a_o", "a_lse2", "b", "c" (lse2 absent from `got`: "a_o" and "c" only); 0 / 0 counts as 0."""
    div = lambda e, tol: torch.where(e > 0, e / tol.clamp_min(1e-300), torch.zeros_like(e))
    res = {}
    for name in ("o", "lse2"):
        if getattr(got, name) is not None:
            res["a_" + name] = div(head_errors(name, getattr(got, name), getattr(ex, name))[0], FACTOR * head_errors(name, getattr(rnd, name), getattr(ex, name))[0])
    if got.lse2 is not None:
        res["b"] = div(lse_distance(got, rnd), yard[0])
    res["c"] = div(o_distance(got, rnd, ex), yard[1])
    return res


def check_forward(label, got, ex, rnd, yard):
    """Asserts (a), (b) and (c) per (batch, head); prints each bound's worst head: distance beside bound.  Returns {bound: worst distance / bound}."""
    names = ("o",) if got.lse2 is None else ("o", "lse2")
    for name in names:
        assert bool(torch.isfinite(getattr(got, name)).all()), (label, name, "not finite")
    worst, failed = {}, []
    try:
        check(label + " (a)", got, rnd, ex, names=names)
    except AssertionError as e:
        failed.append(("a", e.args))
    dist = {"b": (lse_distance(got, rnd), yard[0]) if got.lse2 is not None else None, "c": (o_distance(got, rnd, ex), yard[1])}
    for key, pair in dist.items():
        if pair is None:
            continue
        d, tol = pair
        r = torch.where(d > 0, d / tol.clamp_min(1e-300), torch.zeros_like(d))
        i = int(r.argmax())
        worst[key] = float(r.max())
        what = "max |lse2 - rounded|" if key == "b" else "rel L2 of o - rounded"
        print(f"{label} ({key}) {what}: worst head {float(d.flatten()[i]):.3e} bound {float(tol.flatten()[i]):.3e} ({worst[key]:.2f} of bound)")
        if not bool((d <= tol).all()):
            failed.append((key, float(d.flatten()[i]), float(tol.flatten()[i])))
    assert not failed, (label, failed)
    return worst
