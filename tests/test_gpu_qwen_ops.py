"""The four operators of a Qwen3 decoder layer (awt_op_rmsnorm, awt_op_qk_norm_rope, awt_op_silu_mul, awt_op_causal_attention) against float64
(tests/qwen3_reference.py), operator by operator.  Every bound is derived from the arithmetic, not measured; every case prints its figures first.

    rmsnorm         per element |err| <= 2^-20 |exact| + 1e-30: an fp32 sum of <= 4096 squares (serial per lane, then a tree), a 1-ulp rsq and two multiplies come
                    to under 16 units of 2^-24
    qk_norm_rope    per (row, head) max-abs <= 2^-18 x that row's max |exact|: the norm's bound plus one fused multiply-add pair on operands up to the row
                    maximum; a wrong pairing, position, head or order of norm and rotation is an O(1) error
    silu_mul        |err| <= 2^-20 |exact| + 2^-22 |up|: the denominator 1 + exp(-x) carries exp's error where x << 0
    attention       per (batch, head) max-abs <= 4 x the rounded restatement's own distance from float64 (tests/test_gpu_cross_attention.py's yardstick), and
                    the suite's 1e-4 forward cap at bf16x3 for N(0, 1) values; q and k with standard deviation 1.7"""
import functools

import pytest
import torch

from tests import cross_attention_reference as xr
from tests import qwen3_reference as qr

pytestmark = pytest.mark.gpu

NAN_BITS = torch.tensor(float("nan")).view(torch.int32).item()
ATT_TOL_BF16X3 = 1e-4


def _nan(*shape):
    return torch.full(shape, float("nan"), dtype=torch.float32, device="cuda")


def _all_nan_bits(t):
    return bool((t.contiguous().view(torch.int32) == NAN_BITS).all())


# ------------------------------------------------------------------------------------------------ RMSNorm
@pytest.mark.parametrize("M,d", [(1, 128), (5, 1024), (67, 1024), (3, 4096), (67, 260)])
def test_rmsnorm(M, d):
    from mlx8_ws_audio_transformer_amd import ops
    G, ldx, ldy, cx, cy = 2, d + 8, d + 12, 4, 8
    x = qr.variates("ops.rms.x", (M, d), 1, 2.0).cuda()
    gamma = (1.0 + 0.3 * qr.variates("ops.rms.g", (d,), 1)).float().cuda()
    xb, yb = _nan(M + 2 * G, ldx), _nan(M + 2 * G, ldy)
    xb[G:-G, cx:cx + d] = x.float()
    ops.rmsnorm((xb, G * ldx + cx), ldx, gamma, M, d, 1e-6, y=(yb, G * ldy + cy), ldy=ldy)
    got, ex = yb[G:-G, cy:cy + d].double(), qr.rmsnorm(x, gamma, 1e-6)
    ratio = float(((got - ex).abs() / (2.0 ** -20 * ex.abs() + 1e-30)).max())
    print(f"rmsnorm M{M} d{d}: worst |err| / bound = {ratio:.3f}")
    assert bool(torch.isfinite(got).all()) and ratio <= 1.0
    yb[G:-G, cy:cy + d] = float("nan")
    assert _all_nan_bits(yb), "written outside the M x d block"


def test_rmsnorm_refusals():
    from mlx8_ws_audio_transformer_amd import _lib, ops
    x, g = torch.zeros(4, 128, device="cuda"), torch.ones(128, device="cuda")
    with pytest.raises(_lib.AwtError, match="multiple of 4"):
        ops.rmsnorm((x, 0), 128, g, 4, 126, 1e-6)
    with pytest.raises(_lib.AwtError, match="pitches"):
        ops.rmsnorm((x, 0), 64, g, 4, 128, 1e-6)
    with pytest.raises(_lib.AwtError, match="aligned"):
        ops.rmsnorm((x, 1), 128, g, 3, 124, 1e-6)
    with pytest.raises(_lib.AwtError, match="null"):
        _lib.check(_lib.lib().awt_op_rmsnorm(_lib.ctx(x.device), None, 128, g.data_ptr(), x.data_ptr(), 128, 4, 128, 1e-6, _lib.stream_handle()))


# ------------------------------------------------------------------------------------------------ q / k norm + rotary embedding + cache append
@pytest.mark.parametrize("B,Lq,Hq,Hkv,pos0", [(1, 1, 4, 2, 700), (2, 5, 4, 1, 65), (2, 33, 16, 8, 0)])
def test_qk_norm_rope(B, Lq, Hq, Hkv, pos0):
    from mlx8_ws_audio_transformer_amd import ops
    Tmax, rows_, eps = pos0 + Lq + 3, B * Lq, 1e-6
    w, wq, wkv = (Hq + 2 * Hkv) * 128, Hq * 128, Hkv * 128
    ld, ldq, ldkv = w + 8, wq + 4, wkv + 4                                 # pitches wider than the rows
    qkv = qr.variates("ops.rope.qkv", (rows_, w), 2, 1.5).cuda()
    qg = (1.0 + 0.3 * qr.variates("ops.rope.qg", (128,), 2)).float().cuda()
    kg = (1.0 + 0.3 * qr.variates("ops.rope.kg", (128,), 3)).float().cuda()
    cos, sin = (t.cuda() for t in qr.rope_tables(1e6, Tmax))
    positions = (pos0 + torch.arange(Lq, dtype=torch.int32)).repeat(B).cuda()
    qkv_b = _nan(rows_, ld)
    qkv_b[:, :w] = qkv.float()
    q_out, kc, vc = _nan(rows_, ldq), _nan(B, Tmax, ldkv), _nan(B, Tmax, ldkv)
    ops.qk_norm_rope((qkv_b, 0), ld, qg, kg, cos, sin, positions, (q_out, 0), ldq, (kc, 0), (vc, 0), ldkv, Tmax * ldkv, B, Lq, Hq, Hkv, eps)
    q_ex, k_ex, v_ex = qr.qk_norm_rope(qkv, qg, kg, cos, sin, positions, Hq, Hkv, eps)
    live = slice(pos0, pos0 + Lq)
    k_got = kc[:, live, :wkv].reshape(rows_, Hkv, 128)
    for name, got, ex in (("q", q_out[:, :wq].reshape(rows_, Hq, 128), q_ex), ("k", k_got, k_ex)):
        err, mag = (got.double() - ex).abs().amax(-1), ex.abs().amax(-1)
        ratio = float((err / (2.0 ** -18 * mag)).max())
        print(f"qk_norm_rope B{B} Lq{Lq} Hq{Hq} Hkv{Hkv} pos {pos0}: {name} worst (row, head) max-abs / bound = {ratio:.3f}")
        assert bool(torch.isfinite(got).all()) and ratio <= 1.0
    assert torch.equal(vc[:, live, :wkv].reshape(rows_, Hkv, 128), v_ex.float()), "v must arrive bit-identical"
    for buf in (kc, vc):                                                   # every other cache row, and the pitch's guard columns, still hold their NaN
        rest = buf.clone()
        rest[:, live, :wkv] = float("nan")
        assert _all_nan_bits(rest)
    q_rest = q_out.clone()
    q_rest[:, :wq] = float("nan")
    assert _all_nan_bits(q_rest)


def test_qk_norm_rope_refusals():
    from mlx8_ws_audio_transformer_amd import _lib, ops
    z = lambda *s: torch.zeros(*s, device="cuda")
    qkv, g, tab, pos = z(2, 512), torch.ones(128, device="cuda"), z(8, 64), torch.zeros(2, dtype=torch.int32, device="cuda")
    q, kc, vc = z(2, 256), z(1, 8, 128), z(1, 8, 128)
    ops.qk_norm_rope((qkv, 0), 512, g, g, tab, tab, pos, (q, 0), 256, (kc, 0), (vc, 0), 128, 8 * 128, 1, 2, 2, 1, 1e-6)
    with pytest.raises(_lib.AwtError, match="128 columns"):
        ops.qk_norm_rope((qkv, 0), 384, g, g, tab, tab, pos, (q, 0), 256, (kc, 0), (vc, 0), 128, 8 * 128, 1, 2, 2, 1, 1e-6)
    with pytest.raises(_lib.AwtError, match="kv_batch_stride"):
        ops.qk_norm_rope((qkv, 0), 512, g, g, tab, tab, pos, (q, 0), 256, (kc, 0), (vc, 0), 128, 64, 1, 2, 2, 1, 1e-6)
    with pytest.raises(ValueError, match="int32"):
        ops.qk_norm_rope((qkv, 0), 512, g, g, tab, tab, pos.long(), (q, 0), 256, (kc, 0), (vc, 0), 128, 8 * 128, 1, 2, 2, 1, 1e-6)


# ------------------------------------------------------------------------------------------------ SwiGLU
@pytest.mark.parametrize("M,I", [(1, 384), (67, 3072)])
def test_silu_mul(M, I):
    from mlx8_ws_audio_transformer_amd import ops
    G, ld, ldy = 2, 2 * I + 8, I + 4
    gu = qr.variates("ops.silu", (M, 2 * I), 4, 4.0)                      # gate values out to |x| ~ 18
    gu[0, :8] = torch.tensor([-20.0, 20.0, -15.0, 15.0, -1e-3, 0.0, -88.0, 60.0], dtype=torch.float64)
    gub, yb = _nan(M, ld), _nan(M + 2 * G, ldy)
    gub[:, :2 * I] = gu.float().cuda()
    ops.silu_mul((gub, 0), ld, M, I, y=(yb, G * ldy), ldy=ldy)
    got, ex, up = yb[G:-G, :I].double().cpu(), qr.silu_mul(gu, I), gu[:, I:].abs()
    err, bound = (got - ex).abs(), 2.0 ** -20 * ex.abs() + 2.0 ** -22 * up
    ratio = float(torch.where(err > 0, err / bound.clamp_min(1e-300), torch.zeros_like(err)).max())      # an exact result where the bound is 0 (up == 0) is no error
    print(f"silu_mul M{M} I{I}: worst |err| / bound = {ratio:.3f} (largest |gate| {float(gu[:, :I].abs().max()):.1f})")
    assert bool(torch.isfinite(got).all()) and ratio <= 1.0
    yb[G:-G, :I] = float("nan")
    assert _all_nan_bits(yb), "written outside the M x I block"


def test_silu_mul_refusals():
    from mlx8_ws_audio_transformer_amd import _lib, ops
    gu = torch.zeros(2, 256, device="cuda")
    with pytest.raises(_lib.AwtError, match="multiple of 4"):
        ops.silu_mul((gu, 0), 256, 2, 126)
    with pytest.raises(_lib.AwtError, match="2 I columns"):
        ops.silu_mul((gu, 0), 128, 2, 128)
    with pytest.raises(_lib.AwtError, match="aligned"):
        ops.silu_mul((gu, 1), 256, 1, 124)


# ------------------------------------------------------------------------------------------------ causal attention
# (B, Hq, Hkv, Lq, T)
ATT_CASES = [
    (2, 4, 2, 1, 1),          # first decode step
    (2, 4, 2, 1, 77),         # decode, key-tile tail
    (1, 2, 1, 1, 700),        # long cache
    (2, 4, 2, 33, 33),        # prefill, tails on both axes
    (1, 2, 2, 64, 64),        # exact tiles, no grouping
    (2, 4, 1, 5, 70),         # chunked prefill: offset diagonal, group of 4
    (1, 2, 1, 128, 128),      # one workgroup's worth of queries
    (1, 2, 1, 129, 129),      # one query past a workgroup
    (1, 16, 8, 130, 130),     # Qwen3-0.6B head counts, two query workgroups
]
PAD = 37


def _randn(shape, seed, std=1.0):
    return (torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * std).cuda()


@functools.lru_cache(maxsize=None)
def _att_inputs(B, Hq, Hkv, Lq, T):
    q, k, v = _randn((B, Hq, Lq, 128), 1, 1.7), _randn((B, Hkv, T, 128), 2, 1.7), _randn((B, Hkv, T, 128), 3)
    return q, k, v, qr.causal_attention(q, k, v)


def _run_attention(q, k, v, precision):
    """The operator on a cache of Tmax = T + 37 positions whose every position >= T is NaN; o in a NaN-filled buffer with guard rows."""
    from mlx8_ws_audio_transformer_amd import ops
    B, Hq, Lq, _ = q.shape
    Hkv, T = k.shape[1], k.shape[2]
    Tmax, wkv, G = T + PAD, Hkv * 128, 3
    kc, vc = _nan(B, Tmax, wkv), _nan(B, Tmax, wkv)
    kc[:, :T] = k.permute(0, 2, 1, 3).reshape(B, T, wkv)
    vc[:, :T] = v.permute(0, 2, 1, 3).reshape(B, T, wkv)
    ob = _nan(B * Lq + 2 * G, Hq * 128)
    ops.causal_attention((xr.rows(q).contiguous(), 0), Hq * 128, (kc, 0), (vc, 0), wkv, Tmax * wkv, B, Hq, Hkv, Lq, T, precision, o=(ob, G * Hq * 128), ldo=Hq * 128)
    assert _all_nan_bits(ob[:G]) and _all_nan_bits(ob[-G:])
    return xr.heads(ob[G:-G], B, Hq)


@pytest.mark.parametrize("precision", ["bf16x3", "bf16"])
@pytest.mark.parametrize("B,Hq,Hkv,Lq,T", ATT_CASES)
def test_causal_attention_within_the_rounding_model(B, Hq, Hkv, Lq, T, precision):
    q, k, v, ex = _att_inputs(B, Hq, Hkv, Lq, T)
    got = _run_attention(q, k, v, precision)
    assert bool(torch.isfinite(got).all()), "a cache position >= T (NaN) or an unwritten element reached the output"
    rnd = qr.rounded_causal_attention(q, k, v, 3 if precision == "bf16x3" else 1)
    O = xr.Outputs(got, None, None, None, None)
    xr.check(f"B{B} Hq{Hq} Hkv{Hkv} Lq{Lq} T{T} {precision}", O, xr.Outputs(rnd, None, None, None, None), xr.Outputs(ex, None, None, None, None), names=("o",))
    if precision == "bf16x3":
        err = float((got.double() - ex).abs().max())
        print(f"forward max-abs {err:.3e} (tol {ATT_TOL_BF16X3})")
        assert err <= ATT_TOL_BF16X3


@pytest.mark.parametrize("precision", ["bf16x3", "bf16"])
def test_causal_attention_two_runs_are_bit_identical(precision):
    q, k, v, _ = _att_inputs(1, 16, 8, 130, 130)
    assert torch.equal(_run_attention(q, k, v, precision), _run_attention(q, k, v, precision))
    q, k, v, _ = _att_inputs(2, 4, 2, 1, 77)
    assert torch.equal(_run_attention(q, k, v, precision), _run_attention(q, k, v, precision))


def test_causal_attention_refusals():
    from mlx8_ws_audio_transformer_amd import _lib, ops
    q, kc, vc = torch.zeros(4, 256, device="cuda"), torch.zeros(1, 8, 128, device="cuda"), torch.zeros(1, 8, 128, device="cuda")
    ops.causal_attention((q, 0), 256, (kc, 0), (vc, 0), 128, 1024, 1, 2, 1, 4, 8)
    with pytest.raises(_lib.AwtError, match="multiple of Hkv"):
        ops.causal_attention((q, 0), 384, (kc, 0), (vc, 0), 256, 2048, 1, 3, 2, 1, 1)
    with pytest.raises(_lib.AwtError, match="Lq <= T"):
        ops.causal_attention((q, 0), 256, (kc, 0), (vc, 0), 128, 1024, 1, 2, 1, 4, 3)
    with pytest.raises(_lib.AwtError, match="ldkv"):
        ops.causal_attention((q, 0), 256, (kc, 0), (vc, 0), 64, 1024, 1, 2, 1, 4, 8)
    with pytest.raises(_lib.AwtError, match="kv_batch_stride"):
        ops.causal_attention((q, 0), 256, (kc, 0), (vc, 0), 128, 512, 1, 2, 1, 4, 8)
    with pytest.raises(_lib.AwtError, match="terms"):
        ops.causal_attention((q, 0), 256, (kc, 0), (vc, 0), 128, 1024, 1, 2, 1, 4, 8, precision=2)
