"""The backward operators of a Qwen3 decoder layer (awt_op_causal_attention_lse / _backward, awt_op_rmsnorm_backward, awt_op_rmsnorm_param_grad,
awt_op_silu_mul_backward, awt_op_qk_norm_rope_backward) against float64 (tests/qwen3_train_reference.py), operator by operator.  Every output buffer is
NaN-filled with guard rows / columns that must stay NaN, the cache tail is NaN, every case runs twice and must give the same bits, and every case prints
its measured share of the bound before it asserts.

Attention: per output and per (batch, head) -- dk / dv per (batch, KV head) -- the kernel may be 4 x as far from float64 as the rounded restatement is
(tests/cross_attention_reference.check, the project's bound).  Inputs are those of tests/test_gpu_cross_attention.py: q and k with standard deviation 1.7.

Element-wise operators: bounds counted from the formulas, in units of u = 2^-24 (one fp32 rounding), never fitted.  Let n = 4 ceil(d / 256) be a lane's chain of
fused multiply-adds over a row of d, and a wave's butterfly 6 more additions.
  r = rsq(mean(x^2) + eps):  the sum of squares is off by (n + 6) u relative (positive terms), the division and the addition of eps by 2 u more, the square
      root halves that, v_rsq_f32 adds 1 ulp = 2 u:   rho = (n + 8) / 2 + 2.
  rmsnorm_backward, element j of a row, A = max_j |r gamma dy| (the row's largest term), Q = r^2 mean(x u), |Q| <= A:
      r (gamma dy):   rho + 2               (two products)                                  -> (rho + 2) A
      x coef, coef = r^3 mean(x u) = r Q:   three products and a division (4), r^3 (3 rho), the sum x u with its rounded products (n + 7), all relative to
                      mean|x r| |r u| <= A  -> |x_j r| (3 rho + n + 11) A
      the final fused multiply-add rounds once (|dx|), the residual add once more (|dres + dx|).
  rmsnorm_param_grad, column j:  each term dy (x r) carries rho + 2, a slab is a chain of <= 256 fused multiply-adds, the slabs a chain of additions:
      (rho + 2 + min(M, 256) + slabs) sum_m |dy x r|.
  silu_mul_backward:  e = exp(-|g|) = v_exp_f32(-|g| log2 e): the product's rounding moves the exponent by |g| log2 e u, i.e. e by |g| u relative, the instruction
      by 2 u: eps_e = |g| + 2.  inv = 1 / (1 + e): an addition, a division and e's error weighted e / (1 + e) <= 1/2: eps_inv = 2 + eps_e / 2.  sigmoid and
      1 - sigmoid are inv or e inv (one more product): eps_s = eps_e + eps_inv + 1 = 1.5 |g| + 6.
      dup = dy (g s):  eps_s + 2.
      dgate = (dy up) (s F), F = fma(g, 1 - s, 1):  F is off by u |F| + |g (1 - s)| eps_s (F passes through zero near g = -1.28, so its error is absolute),
      three more products:  |dy up s| ((eps_s + 4) |F| + |g (1 - s)| eps_s).
      Where e falls below 2^-126 (|g| > 87.3) it may be flushed to zero, and so may a result: floors of 2^-126 (1 + |dy up| (1 + |g|)) and 2^-126 (1 + |dy g|).
  qk_norm_rope_backward, (row, head): the transposed rotation is a product and a fused multiply-add on values up to Y = max |dy|: off by 4 u Y, and
      |g'| <= sqrt 2 Y; then the norm's backward over d = 128 held two per lane (n = 2) with A <= AY = sqrt 2 r max(gamma) Y:
      ((rho + 6) + |x_j r| (3 rho + n + 15)) AY + |dx|.  Gains: a term g' (x r) carries rho + 2 and 4 u Y |x r| from g'; a wave chains <= 64 terms, four waves
      and the slabs are added in order:  4 sum |x r| Y + (rho + 2 + 64 + 3 + slabs) sum |g' x r|.
  dv must come out bit-identical."""
import functools
import math

import pytest
import torch

from tests import cross_attention_reference as xr
from tests import qwen3_reference as qr
from tests import qwen3_train_reference as tr

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
NAN_BITS = torch.tensor(float("nan")).view(torch.int32).item()


def _nan(*shape):
    return torch.full(shape, float("nan"), dtype=torch.float32, device="cuda")


def _all_nan_bits(t):
    return bool((t.contiguous().view(torch.int32) == NAN_BITS).all())


def _same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _share(label, err, bound):
    """Prints and returns the largest err / bound (an exact result where the bound is zero is no error)."""
    ratio = float(torch.where(err > 0, err / bound.clamp_min(1e-300), torch.zeros_like(err)).max())
    print(f"{label}: worst |err| / bound = {ratio:.3f}")
    return ratio


def _rho(n):
    return (n + 8) / 2 + 2


# ------------------------------------------------------------------------------------------------ causal attention backward
# (B, Hq, Hkv, Lq, T, rows of the cache per batch or None for T + 37, q / dq pitched)
ATT_CASES = [
    (2, 4, 2, 37, 37, None, False),       # tails on both axes
    (1, 2, 2, 64, 64, None, False),       # exact tiles
    (1, 1, 1, 65, 65, None, False),       # one key past the tile
    (1, 2, 1, 129, 129, None, False),     # one query past the first workgroup
    (1, 4, 1, 130, 130, None, False),     # second workgroup, a group of 4
    (2, 2, 1, 33, 100, None, False),      # cache prefix, T > Lq
    (1, 16, 8, 130, 130, None, False),    # the model's head counts
    (1, 2, 1, 40, 70, 96, True),          # cache of 96 rows per batch, pitched q / dq
]
G = 3


def _randn(shape, seed, std=1.0):
    return (torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * std).cuda()


@functools.lru_cache(maxsize=None)
def _att_inputs(B, Hq, Hkv, Lq, T):
    q, k = _randn((B, Hq, Lq, 128), 1, 1.7), _randn((B, Hkv, T, 128), 2, 1.7)
    v, d_o = _randn((B, Hkv, T, 128), 3), _randn((B, Hq, Lq, 128), 4)
    return q, k, v, d_o, tr.causal_attention_backward(q, k, v, d_o)


def _run_attention(q, k, v, d_o, precision, Tmax, pitched):
    """Forward with lse, then the backward, on a cache whose positions >= T are NaN; every output in a NaN-filled buffer with guards.  Returns Outputs and
    the raw output buffers."""
    from mlx8_ws_audio_transformer_amd import ops
    B, Hq, Lq, _ = q.shape
    Hkv, T = k.shape[1], k.shape[2]
    Tmax = T + 37 if Tmax is None else Tmax
    wq, wkv = Hq * 128, Hkv * 128
    ldq, cq = (wq + 64, 32) if pitched else (wq, 0)
    lddkv, Td = wkv + 8, T + 5                                            # dk / dv: their own pitch and batch stride
    kc, vc = _nan(B, Tmax, wkv), _nan(B, Tmax, wkv)
    kc[:, :T] = k.permute(0, 2, 1, 3).reshape(B, T, wkv)
    vc[:, :T] = v.permute(0, 2, 1, 3).reshape(B, T, wkv)
    qb, dqb = _nan(B * Lq + 2 * G, ldq), _nan(B * Lq + 2 * G, ldq)
    qb[G:-G, cq:cq + wq] = xr.rows(q)
    ob, lse = _nan(B * Lq + 2 * G, wq), _nan(B, Hq, Lq)
    dkb, dvb = _nan(B, Td, lddkv), _nan(B, Td, lddkv)
    qa, oa = (qb, G * ldq + cq), (ob, G * wq)
    ops.causal_attention_lse(qa, ldq, (kc, 0), (vc, 0), wkv, Tmax * wkv, B, Hq, Hkv, Lq, T, precision, o=oa, ldo=wq, lse=lse)
    ops.causal_attention_backward(qa, ldq, (kc, 0), (vc, 0), wkv, Tmax * wkv, oa, (xr.rows(d_o).contiguous(), 0), wq, lse, (dqb, G * ldq + cq), (dkb, 0), (dvb, 0),
                                  lddkv, Td * lddkv, B, Hq, Hkv, Lq, T, precision)
    cache = lambda buf: buf[:, :T, :wkv].reshape(B, T, Hkv, 128).permute(0, 2, 1, 3)
    out = xr.Outputs(xr.heads(ob[G:-G], B, Hq), lse, xr.heads(dqb[G:-G, cq:cq + wq], B, Hq), cache(dkb), cache(dvb))
    # guards: the rows around o and dq, dq's pitch columns, the rows >= T and the pitch columns of dk / dv
    assert _all_nan_bits(ob[:G]) and _all_nan_bits(ob[-G:]) and _all_nan_bits(dqb[:G]) and _all_nan_bits(dqb[-G:])
    assert _all_nan_bits(dqb[:, :cq]) and _all_nan_bits(dqb[:, cq + wq:])
    for buf in (dkb, dvb):
        assert _all_nan_bits(buf[:, T:]) and _all_nan_bits(buf[:, :, wkv:])
    return out, (ob, lse, dqb, dkb, dvb)


@pytest.mark.parametrize("precision", ["bf16x3", "bf16"])
@pytest.mark.parametrize("B,Hq,Hkv,Lq,T,Tmax,pitched", ATT_CASES)
def test_causal_attention_backward_within_the_rounding_model(B, Hq, Hkv, Lq, T, Tmax, pitched, precision):
    q, k, v, d_o, ex = _att_inputs(B, Hq, Hkv, Lq, T)
    got, raw = _run_attention(q, k, v, d_o, precision, Tmax, pitched)
    for name in xr.NAMES:
        assert bool(torch.isfinite(getattr(got, name)).all()), f"{name}: a cache position >= T (NaN) or an unwritten element reached the output"
    rnd = tr.rounded_causal_attention_backward(q, k, v, d_o, 3 if precision == "bf16x3" else 1)
    xr.check(f"B{B} Hq{Hq} Hkv{Hkv} Lq{Lq} T{T} {precision}", got, rnd, ex)
    _, again = _run_attention(q, k, v, d_o, precision, Tmax, pitched)
    assert all(_same_bits(a, b) for a, b in zip(raw, again)), "two runs differ"


def test_causal_attention_lse_is_the_forward_with_one_more_output():
    from mlx8_ws_audio_transformer_amd import ops
    q, k, v, _, _ = _att_inputs(2, 2, 1, 33, 100)
    B, Hq, Lq, T, wkv = 2, 2, 33, 100, 128
    kc, vc = (t.permute(0, 2, 1, 3).reshape(B, T, wkv).contiguous() for t in (k, v))
    qa = (xr.rows(q).contiguous(), 0)
    o = ops.causal_attention(qa, Hq * 128, (kc, 0), (vc, 0), wkv, T * wkv, B, Hq, 1, Lq, T)
    o2, _ = ops.causal_attention_lse(qa, Hq * 128, (kc, 0), (vc, 0), wkv, T * wkv, B, Hq, 1, Lq, T)
    assert torch.equal(o, o2)


def test_causal_attention_backward_refusals_and_workspace_query():
    from mlx8_ws_audio_transformer_amd import _lib, ops
    assert ops.causal_attention_backward_workspace_bytes(2, 4, 37, 37) >= 2 * 4 * 37 * 4                      # delta; answers without touching the GPU
    assert ops.causal_attention_backward_workspace_bytes(0, 4, 37, 37) == 0
    z = lambda *s: torch.zeros(*s, device="cuda")
    q, kc, vc, lse = z(4, 256), z(1, 8, 128), z(1, 8, 128), z(1, 2, 4)
    dq, dk, dv = z(4, 256), z(1, 8, 128), z(1, 8, 128)
    run = lambda ldq=256, ldkv=128, kvbs=1024, lddkv=128, dkvbs=1024, Hq=2, Hkv=1, Lq=4, T=8, precision="bf16x3", qoff=0: ops.causal_attention_backward(
        (q, qoff), ldq, (kc, 0), (vc, 0), ldkv, kvbs, (q, 0), (q, 0), 256, lse, (dq, 0), (dk, 0), (dv, 0), lddkv, dkvbs, 1, Hq, Hkv, Lq, T, precision)
    run()
    for kw, match in ((dict(Hq=3, Hkv=2, ldq=384), "multiple of Hkv"), (dict(T=3), "Lq <= T"), (dict(ldkv=64), "ldkv"), (dict(kvbs=512), "kv_batch_stride"),
                      (dict(precision=2), "terms"), (dict(lddkv=64), "lddkv"), (dict(dkvbs=512), "dkv_batch_stride"), (dict(ldq=128), "H \\* 128"),
                      (dict(qoff=1, Lq=3), "aligned")):
        with pytest.raises(_lib.AwtError, match=match):
            run(**kw)
    with pytest.raises(_lib.AwtError, match="null"):                                                         # the lse variant without an lse
        _lib.check(_lib.lib().awt_op_causal_attention_lse(_lib.ctx(q.device), q.data_ptr(), 256, kc.data_ptr(), vc.data_ptr(), 128, 1024, dq.data_ptr(), 256, None,
                                                          1, 2, 1, 4, 8, 3, None, 0, _lib.stream_handle()))


# ------------------------------------------------------------------------------------------------ RMSNorm backward
@pytest.mark.parametrize("M,d,with_dres", [(1, 128, False), (5, 1024, True), (67, 1024, False), (3, 4096, False), (67, 260, True)])
def test_rmsnorm_backward(M, d, with_dres):
    from mlx8_ws_audio_transformer_amd import ops
    Gr, ldx, lddy, lddx, cx, cy, cd, eps = 2, d + 8, d + 4, d + 12, 4, 0, 8, 1e-6
    x, dy = qr.variates("train.rms.x", (M, d), 1, 2.0), qr.variates("train.rms.dy", (M, d), 2)
    gamma = (1.0 + 0.3 * qr.variates("train.rms.g", (d,), 1)).float()
    dres = qr.variates("train.rms.dres", (M, d), 3) if with_dres else None
    xb, yb = _nan(M, ldx), _nan(M, lddy)
    xb[:, cx:cx + d], yb[:, cy:cy + d] = x.float().cuda(), dy.float().cuda()

    def run():
        out = _nan(M + 2 * Gr, lddx)
        res = None
        if with_dres:
            res = (_nan(M + 2 * Gr, lddx), Gr * lddx + cd)
            res[0][Gr:-Gr, cd:cd + d] = dres.float().cuda()
        ops.rmsnorm_backward((yb, cy), lddy, (xb, cx), ldx, gamma.cuda(), M, d, eps, dres=res, dx=(out, Gr * lddx + cd), lddx=lddx)
        return out

    out = run()
    got, ex = out[Gr:-Gr, cd:cd + d].double().cpu(), tr.rmsnorm_backward(dy, x, gamma, eps, dres)
    n = 4 * math.ceil(d / 256)
    rho = _rho(n)
    r = torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + eps)
    A = (r * gamma.double() * dy).abs().amax(-1, keepdim=True)
    plain = tr.rmsnorm_backward(dy, x, gamma, eps)
    bound = U * (A * ((rho + 2) + (x * r).abs() * (3 * rho + n + 11)) + plain.abs() + (ex.abs() if with_dres else 0.0))
    ratio = _share(f"rmsnorm_backward M{M} d{d} dres={with_dres}", (got - ex).abs(), bound)
    assert bool(torch.isfinite(got).all()) and ratio <= 1.0
    assert _same_bits(out, run()), "two runs differ"
    out[Gr:-Gr, cd:cd + d] = float("nan")
    assert _all_nan_bits(out), "written outside the M x d block"


def test_rmsnorm_backward_in_place_on_the_residual_gradient():
    from mlx8_ws_audio_transformer_amd import ops
    M, d, eps = 9, 256, 1e-6
    x, dy, dres = (qr.variates("train.rms.inplace." + n, (M, d), 1).float().cuda() for n in ("x", "dy", "dres"))
    gamma = torch.ones(d, device="cuda")
    want = ops.rmsnorm_backward((dy, 0), d, (x, 0), d, gamma, M, d, eps, dres=(dres, 0), lddx=d, dx=(torch.empty_like(x), 0))
    buf = dres.clone()
    ops.rmsnorm_backward((dy, 0), d, (x, 0), d, gamma, M, d, eps, dres=(buf, 0), dx=(buf, 0), lddx=d)
    assert torch.equal(buf, want)


@pytest.mark.parametrize("M,d", [(1, 128), (67, 1024), (300, 260), (515, 1024)])
def test_rmsnorm_param_grad(M, d):
    """M = 300 and 515 are no multiples of the slab of 256 rows; 515 has three slabs."""
    from mlx8_ws_audio_transformer_amd import ops
    ldx, lddy, eps = d + 8, d + 4, 1e-6
    x, dy = qr.variates("train.rmsg.x", (M, d), 1, 2.0), qr.variates("train.rmsg.dy", (M, d), 2)
    xb, yb = _nan(M, ldx), _nan(M, lddy)
    xb[:, 4:4 + d], yb[:, :d] = x.float().cuda(), dy.float().cuda()
    got = ops.rmsnorm_param_grad((yb, 0), lddy, (xb, 4), ldx, M, d, eps)
    ex = tr.rmsnorm_param_grad(dy, x, eps)
    r = torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + eps)
    slabs = math.ceil(M / 256)
    bound = U * (_rho(4 * math.ceil(d / 256)) + 2 + min(M, 256) + slabs) * (dy * x * r).abs().sum(0)
    ratio = _share(f"rmsnorm_param_grad M{M} d{d}", (got.double().cpu() - ex).abs(), bound)
    assert got.shape == (d,) and bool(torch.isfinite(got).all()) and ratio <= 1.0
    assert torch.equal(got, ops.rmsnorm_param_grad((yb, 0), lddy, (xb, 4), ldx, M, d, eps)), "two runs differ"


def test_rmsnorm_backward_refusals():
    from mlx8_ws_audio_transformer_amd import _lib, ops
    x, g = torch.zeros(4, 128, device="cuda"), torch.ones(128, device="cuda")
    assert int(_lib.lib().awt_op_rmsnorm_param_grad_workspace_bytes(300, 260)) >= 300 * 4 + 2 * 260 * 4
    with pytest.raises(_lib.AwtError, match="multiple of 4"):
        ops.rmsnorm_backward((x, 0), 128, (x, 0), 128, g, 4, 126, 1e-6)
    with pytest.raises(_lib.AwtError, match="pitches"):
        ops.rmsnorm_backward((x, 0), 64, (x, 0), 128, g, 4, 128, 1e-6)
    with pytest.raises(_lib.AwtError, match="aligned"):
        ops.rmsnorm_backward((x, 1), 128, (x, 0), 128, g, 3, 124, 1e-6)
    with pytest.raises(_lib.AwtError, match="multiple of 4"):
        ops.rmsnorm_param_grad((x, 0), 128, (x, 0), 128, 4, 126, 1e-6)
    with pytest.raises(_lib.AwtError, match="pitches"):
        ops.rmsnorm_param_grad((x, 0), 128, (x, 0), 64, 4, 128, 1e-6)


# ------------------------------------------------------------------------------------------------ SwiGLU backward
@pytest.mark.parametrize("M,I", [(1, 384), (67, 3072)])
def test_silu_mul_backward(M, I):
    from mlx8_ws_audio_transformer_amd import ops
    Gr, ld, lddy, lddgu = 2, 2 * I + 8, I + 4, 2 * I + 12
    gu, dy = qr.variates("train.silu.gu", (M, 2 * I), 4, 4.0), qr.variates("train.silu.dy", (M, I), 5)
    gu[0, :10] = torch.tensor([-20.0, 20.0, -15.0, 15.0, -1e-3, 0.0, -88.0, 88.0, 60.0, -1.2785], dtype=torch.float64)
    gub, yb = _nan(M, ld), _nan(M, lddy)
    gub[:, :2 * I], yb[:, :I] = gu.float().cuda(), dy.float().cuda()

    def run():
        out = _nan(M + 2 * Gr, lddgu)
        ops.silu_mul_backward((gub, 0), ld, (yb, 0), lddy, M, I, dgu=(out, Gr * lddgu), lddgu=lddgu)
        return out

    out = run()
    got, ex = out[Gr:-Gr, :2 * I].double().cpu(), tr.silu_mul_backward(gu, dy, I)
    g, up = gu[:, :I], gu[:, I:]
    s = torch.sigmoid(g)
    t1, F, eps_s = 1.0 - s, 1.0 + g * (1.0 - s), 1.5 * g.abs() + 6
    tiny = 2.0 ** -126
    b_gate = U * (dy * up * s).abs() * ((eps_s + 4) * F.abs() + (g * t1).abs() * eps_s) + tiny * (1 + (dy * up).abs() * (1 + g.abs()))
    b_up = U * (eps_s + 2) * (dy * g * s).abs() + tiny * (1 + (dy * g).abs())
    ratio = _share(f"silu_mul_backward M{M} I{I} (largest |gate| {float(g.abs().max()):.1f})", (got - ex).abs(), torch.cat([b_gate, b_up], dim=-1))
    assert bool(torch.isfinite(got).all()) and ratio <= 1.0
    assert _same_bits(out, run()), "two runs differ"
    out[Gr:-Gr, :2 * I] = float("nan")
    assert _all_nan_bits(out), "written outside the M x 2 I block"


def test_silu_mul_backward_refusals():
    from mlx8_ws_audio_transformer_amd import _lib, ops
    gu, dy = torch.zeros(2, 256, device="cuda"), torch.zeros(2, 128, device="cuda")
    with pytest.raises(_lib.AwtError, match="multiple of 4"):
        ops.silu_mul_backward((gu, 0), 256, (dy, 0), 128, 2, 126)
    with pytest.raises(_lib.AwtError, match="2 I columns"):
        ops.silu_mul_backward((gu, 0), 128, (dy, 0), 128, 2, 128)
    with pytest.raises(_lib.AwtError, match="aligned"):
        ops.silu_mul_backward((gu, 1), 256, (dy, 0), 128, 1, 124)


# ------------------------------------------------------------------------------------------------ q / k norm + rotary embedding, backward
@pytest.mark.parametrize("B,Lq,Hq,Hkv,pos0", [(1, 1, 4, 2, 700), (2, 5, 4, 1, 65), (2, 33, 16, 8, 0)])
def test_qk_norm_rope_backward(B, Lq, Hq, Hkv, pos0):
    """The forward test's three shapes; the positions of a batch are scattered (a permutation of pos0 .. pos0 + Lq - 1, another one per batch)."""
    from mlx8_ws_audio_transformer_amd import ops
    Tmax, rows_, eps = pos0 + Lq + 3, B * Lq, 1e-6
    w, wq, wkv = (Hq + 2 * Hkv) * 128, Hq * 128, Hkv * 128
    ld, ldq, ldkv = w + 8, wq + 4, wkv + 4
    qkv = qr.variates("train.rope.qkv", (rows_, w), 2, 1.5)
    qg, kg = (1.0 + 0.3 * qr.variates("train.rope.qg", (128,), 2)).float(), (1.0 + 0.3 * qr.variates("train.rope.kg", (128,), 3)).float()
    cos, sin = qr.rope_tables(1e6, Tmax)
    gen = torch.Generator().manual_seed(11)
    positions = torch.cat([pos0 + torch.randperm(Lq, generator=gen) for _ in range(B)]).to(torch.int32)
    dq, dk, dv = (qr.variates("train.rope." + n, (rows_, h, 128), 6) for n, h in (("dq", Hq), ("dk", Hkv), ("dv", Hkv)))
    qkv_b, dq_b = _nan(rows_, ld), _nan(rows_, ldq)
    qkv_b[:, :w], dq_b[:, :wq] = qkv.float().cuda(), dq.reshape(rows_, wq).float().cuda()
    dkc, dvc = _nan(B, Tmax, ldkv), _nan(B, Tmax, ldkv)                  # the gradients of the cache rows, at the rows' positions; everything else NaN
    bidx, pidx = (torch.arange(rows_) // Lq).cuda(), positions.long().cuda()
    dkc[bidx, pidx, :wkv], dvc[bidx, pidx, :wkv] = dk.reshape(rows_, wkv).float().cuda(), dv.reshape(rows_, wkv).float().cuda()

    def run():
        out = _nan(rows_, ld)
        gains = ops.qk_norm_rope_backward((qkv_b, 0), ld, qg.cuda(), kg.cuda(), cos.cuda(), sin.cuda(), positions.cuda(), (dq_b, 0), ldq, (dkc, 0), (dvc, 0), ldkv,
                                          Tmax * ldkv, (out, 0), B, Lq, Hq, Hkv, eps, want_gains=True)
        return out, gains

    out, (gq, gk) = run()
    ex, ex_gq, ex_gk = tr.qk_norm_rope_backward(qkv, qg, kg, cos, sin, positions, dq, dk, dv, Hq, Hkv, eps)
    got = out[:, :w].double().cpu()
    assert bool(torch.isfinite(got).all())
    assert torch.equal(out[:, wq + wkv:w].cpu(), dv.reshape(rows_, wkv).float()), "dv must arrive bit-identical"
    n, rho = 2, _rho(2)
    label = f"qk_norm_rope_backward B{B} Lq{Lq} Hq{Hq} Hkv{Hkv} pos {pos0}"
    c, s = cos.double()[positions.long()][:, None, :], sin.double()[positions.long()][:, None, :]
    worst = 0.0
    for name, lo, nh, gam, dy, g_got, g_ex in (("q", 0, Hq, qg, dq, gq, ex_gq), ("k", Hq, Hkv, kg, dk, gk, ex_gk)):
        x = qkv.view(rows_, -1, 128)[:, lo:lo + nh]
        r = torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + eps)
        Y = dy.abs().amax(-1, keepdim=True)
        AY = math.sqrt(2.0) * r * float(gam.max()) * Y
        e = ex.view(rows_, -1, 128)[:, lo:lo + nh]
        bound = U * (AY * ((rho + 6) + (x * r).abs() * (3 * rho + n + 15)) + e.abs())
        worst = max(worst, _share(f"{label} d{name}", (got.view(rows_, -1, 128)[:, lo:lo + nh] - e).abs(), bound))
        gp = tr.rotate_back(dy, c, s)
        slabs = math.ceil(rows_ * nh / 256)
        g_bound = U * (4 * ((x * r).abs() * Y).sum((0, 1)) + (rho + 2 + 64 + 3 + slabs) * (gp * x * r).abs().sum((0, 1)))
        worst = max(worst, _share(f"{label} d{name}_gamma", (g_got.double().cpu() - g_ex).abs(), g_bound))
    assert worst <= 1.0
    out2, (gq2, gk2) = run()
    assert _same_bits(out, out2) and torch.equal(gq, gq2) and torch.equal(gk, gk2), "two runs differ"
    rest = out.clone()
    rest[:, :w] = float("nan")
    assert _all_nan_bits(rest), "written outside the rows' (Hq + 2 Hkv) 128 columns"
    # without the gain gradients the row gradient is the same and no workspace is needed
    out3 = _nan(rows_, ld)
    assert ops.qk_norm_rope_backward((qkv_b, 0), ld, qg.cuda(), kg.cuda(), cos.cuda(), sin.cuda(), positions.cuda(), (dq_b, 0), ldq, (dkc, 0), (dvc, 0), ldkv,
                                     Tmax * ldkv, (out3, 0), B, Lq, Hq, Hkv, eps) is None
    assert _same_bits(out, out3)


def test_qk_norm_rope_backward_refusals():
    from mlx8_ws_audio_transformer_amd import _lib, ops
    z = lambda *s: torch.zeros(*s, device="cuda")
    qkv, g, tab, pos = z(2, 512), torch.ones(128, device="cuda"), z(8, 64), torch.zeros(2, dtype=torch.int32, device="cuda")
    dq, dkc, dvc, out = z(2, 256), z(1, 8, 128), z(1, 8, 128), z(2, 512)
    assert ops.qk_norm_rope_backward_workspace_bytes(2, 33, 16, 8) >= (math.ceil(66 * 16 / 256) + math.ceil(66 * 8 / 256)) * 512
    run = lambda ld=512, kvbs=8 * 128, p=pos: ops.qk_norm_rope_backward((qkv, 0), ld, g, g, tab, tab, p, (dq, 0), 256, (dkc, 0), (dvc, 0), 128, kvbs, (out, 0),
                                                                        1, 2, 2, 1, 1e-6)
    run()
    with pytest.raises(_lib.AwtError, match="128 columns"):
        run(ld=384)
    with pytest.raises(_lib.AwtError, match="kv_batch_stride"):
        run(kvbs=64)
    with pytest.raises(ValueError, match="int32"):
        run(p=pos.long())
