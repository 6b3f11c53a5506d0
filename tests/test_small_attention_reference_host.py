"""CPU: the float64 reference of the fp32 head_dim-64 attention family (tests/small_attention_reference.py) and the host restatement of its dropout
mask, checked against formulations that share nothing with them."""
import math

import pytest
import torch
import torch.nn.functional as F

from tests import small_attention_reference as sr

MASK64 = (1 << 64) - 1


def _randn(shape, seed):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)


def _keep(seed, B, H, Lq, Sk, p):
    from mlx8_ws_audio_transformer_amd.autograd_ops import attention_keep_mask
    return attention_keep_mask(seed, B, H, Lq, Sk, p) > 0


@pytest.mark.parametrize("B,H,Lq,Sk,causal,off,p", [(2, 2, 5, 9, True, 4, 0.0), (1, 2, 7, 70, False, 0, 0.25), (2, 1, 6, 20, True, 14, 0.3)])
def test_exact_agrees_with_scaled_dot_product_attention(B, H, Lq, Sk, causal, off, p):
    """torch's own attention in float64 with a boolean mask.  It has no hook for a given dropout pattern, so the probabilities are taken from it with the
    identity as values and the pattern is multiplied in by hand; lse = s_i0 - ln P_i0 (key 0 is visible to every row)."""
    q, k, v, d_o = _randn((B, H, Lq, 64), 1), _randn((B, H, Sk, 64), 2), _randn((B, H, Sk, 64), 3), _randn((B, H, Lq, 64), 4)
    keep = _keep(11, B, H, Lq, Sk, p) if p > 0 else None
    ex = sr.exact(q, k, v, d_o, causal, off, keep, p)
    q2, k2, v2 = (t.clone().requires_grad_(True) for t in (q, k, v))
    i, j = torch.arange(Lq)[:, None], torch.arange(Sk)[None, :]
    allowed = (j - off <= i) if causal else torch.ones(Lq, Sk, dtype=torch.bool)
    P = F.scaled_dot_product_attention(q2, k2, torch.eye(Sk, dtype=torch.float64).expand(B, H, Sk, Sk), attn_mask=allowed, scale=0.125)
    if keep is not None:
        P = P * keep.double() / (1.0 - p)
    o = P @ v2
    dq, dk, dv = torch.autograd.grad(o, (q2, k2, v2), d_o)
    Pu = F.scaled_dot_product_attention(q, k, torch.eye(Sk, dtype=torch.float64).expand(B, H, Sk, Sk), attn_mask=allowed, scale=0.125)
    lse = (q * k[:, :, :1]).sum(-1) / 8 - torch.log(Pu[..., 0])
    want = sr.Outputs(o.detach(), lse, (d_o * o.detach()).sum(-1), dq, dk, dv)
    for name in sr.NAMES:
        a, b = getattr(ex, name), getattr(want, name)
        rel = float((a - b).abs().max() / b.abs().max())
        print(f"exact vs scaled_dot_product_attention {name}: {rel:.2e}")
        assert rel <= 1e-12, (name, rel)


LARGER = [c + (0.0,) for c in sr.CASES if c[3] > 64] + sr.DROPOUT_CASES


@pytest.mark.parametrize("B,H,Lq,Sk,causal,off,p", LARGER)
def test_rounded_is_an_fp32_distance_from_exact(B, H, Lq, Sk, causal, off, p):
    """What the GPU bound is a multiple of.  A restatement that computes in float64 by accident is at distance 0, one in bf16 at 1e-3.  Every head of a
    case with Sk > 64 must have a restatement term above 0, because there the bound has no floor beside it."""
    q, k, v, d_o = sr.inputs(B, H, Lq, Sk)
    keep = _keep(sr.DROPOUT_SEED, B, H, Lq, Sk, p) if p > 0 else None
    ex, rnd = sr.exact(q, k, v, d_o, causal, off, keep, p), sr.rounded(q, k, v, d_o, causal, off, keep, p)
    for name in sr.NAMES:
        e, r = getattr(ex, name), getattr(rnd, name)
        dist, top = float((r - e).abs().max()), float(e.abs().max())
        tol, restated, floor, den = sr.bound(rnd, ex, name, Sk)
        print(f"rounded vs exact {(B, H, Lq, Sk, causal, off, p)} {name}: {dist:.3e} = {dist / top:.3e} x max |exact|; "
              f"smallest head's restatement term {float((restated / (sr.FACTOR * 2.0 ** -23 * den)).min()):.2f} x 2^-23 max |exact|")
        assert 0.0 < dist <= 1e-5 * top, (name, dist, top)
        assert bool((tol > 0).all()) and (Sk <= sr.CHUNK or (bool((floor == 0).all()) and bool((restated > 0).all()))), name


def _splitmix_keep(seed, flat, p):
    """include/awt.h, awt_op_attention_small_dropout, in Python integers."""
    z = (flat + seed * 0x9E3779B97F4A7C15 + 0x632BE59BD9B4E019) & MASK64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK64
    z ^= z >> 31
    u = (z >> 40) / 16777216.0                      # 24 bits: exact in fp32 and in a Python float
    return u >= float(torch.tensor(p, dtype=torch.float32))


def test_keep_mask_is_splitmix64_of_the_flat_index():
    B, H, Lq, Sk, p, seed = 2, 3, 7, 45, 0.3, 0xDEADBEEFCAFE
    keep = _keep(seed, B, H, Lq, Sk, p)
    from mlx8_ws_audio_transformer_amd.autograd_ops import attention_keep_mask
    values = attention_keep_mask(seed, B, H, Lq, Sk, p)
    assert set(values.unique().tolist()) == {0.0, float(torch.tensor(1.0 / (1.0 - p), dtype=torch.float32))}
    picks = set()
    for bh in range(B * H):
        picks |= {(bh, 0, 0), (bh, Lq - 1, Sk - 1), (bh, 0, Sk - 1), (bh, Lq - 1, 0)}
    g = torch.Generator().manual_seed(3)
    for _ in range(500):
        picks.add((int(torch.randint(B * H, (1,), generator=g)), int(torch.randint(Lq, (1,), generator=g)), int(torch.randint(Sk, (1,), generator=g))))
    for bh, i, j in sorted(picks):
        assert bool(keep[bh // H, bh % H, i, j]) == _splitmix_keep(seed, (bh * Lq + i) * Sk + j, p), (bh, i, j)


@pytest.mark.parametrize("p", [0.1, 0.25, 0.5])
def test_keep_fraction(p):
    """Each element is kept with probability 1 - p (to 2^-24): the fraction of n kept has standard deviation sqrt(p (1 - p) / n)."""
    n = 2 * 3 * 40 * 300
    frac = float(_keep(sr.DROPOUT_SEED, 2, 3, 40, 300, p).double().mean())
    sd = math.sqrt(p * (1.0 - p) / n)
    print(f"keep fraction p {p}: {frac:.5f}, {(frac - (1 - p)) / sd:+.2f} standard deviations from {1 - p}")
    assert abs(frac - (1.0 - p)) <= 4.0 * sd
