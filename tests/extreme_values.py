"""Non-finite and extreme operands for the fp32 row operators: the value classes, the two comparisons, the operand builders and, per operator, the
restatement the GPU results are held against.  (A plain module: the GPU cases are in tests/test_gpu_extreme_values.py, the checks of this plumbing and
of the restatements, on the CPU, in tests/test_extreme_values_host.py.)

A restatement is the operator's own expression written once in torch and evaluated twice: in float64 for values, in float32 for the CLASS (NaN, +inf,
-inf, finite) of the elements whose intermediates overflow in fp32 only -- LayerNorm of a row holding 1e20 has a finite fp64 answer that no fp32
kernel can return.  `expected(case)` splits the elements of every output that are finite in fp64 into
  * value elements: held to fp64 within the bound.  Outside the one row per output that a case names in `class_only`, that is every such element;
  * fp32-held elements (named row only): the fp32 restatement is finite but more than four bounds from fp64 (a LayerNorm row holding 1e20 comes out
    as beta): held to the fp32 restatement within the bound;
  * class-only elements (named row only): the fp32 restatement is not finite (a product with FLT_MAX): the class must match, nothing more;
  * the `ordered` columns of the column sums: the fp32 restatement's bits.
Every element, finite in fp64 or not, must be of the fp32 restatement's class.  tests/test_extreme_values_host.py proves on the CPU that no element
outside a named row is out of fp32's reach, so nothing is excused quietly.  The issue caps the class-only elements at one row per CASE; here it is one
row per OUTPUT, because a parameter gradient (dgamma, one row) misses the overflowing row's term in every column while y and dx miss it in that row.
The bounds are the ones the operators' own test files use, restated next to each restatement with the file they come from.
"""
from __future__ import annotations

import collections
import math

import numpy as np
import torch

from tests.graph_capture import bits

FLT_MAX = 3.4028234663852886e38
U = 2.0 ** -24                                         # unit roundoff of fp32
INF, NAN = float("inf"), float("nan")
SPECIALS = {"+inf": INF, "-inf": -INF, "nan": NAN, "+fltmax": FLT_MAX, "-fltmax": -FLT_MAX, "+1e20": 1e20, "-1e20": -1e20,      # 1e20^2 overflows fp32
            "+1e-30": 1e-30, "-1e-30": -1e-30,                                                                                    # 1e-30^2 underflows
            "subnormal": 1e-40, "-0": -0.0}
NONFINITE = ("+inf", "-inf", "nan")
OVERFLOWING = ("+fltmax", "-fltmax", "+1e20", "-1e20")          # finite, but a square or a product of two leaves fp32

CLASSES = ("nan", "+inf", "-inf", "+0", "-0", "+finite", "-finite")


def classify(t: torch.Tensor) -> torch.Tensor:
    """Per element the index into CLASSES, as int8 on the CPU."""
    t = t.detach().cpu()
    neg = torch.signbit(t)
    c = torch.where(neg, 6, 5)
    c = torch.where(t == 0, torch.where(neg, 4, 3), c)
    c = torch.where(torch.isinf(t), torch.where(neg, 2, 1), c)
    c = torch.where(torch.isnan(t), 0, c)
    return c.to(torch.int8)


def _coarse(c: torch.Tensor) -> torch.Tensor:
    """Zeros and finite values of either sign as one class: a kernel and its reference may round a tiny value to different sides of zero."""
    return torch.where(c >= 3, torch.full_like(c, 5), c)


def _index(shape, flat: int):
    return tuple(int(i) for i in np.unravel_index(flat, tuple(shape))) if len(shape) else ()


def assert_same_class(got: torch.Tensor, want: torch.Tensor, where: str, signs: bool = False) -> None:
    """Every element of `got` is of the class of `want`'s (NaN, +inf, -inf, finite; with `signs` also +0, -0 and the sign of a finite value).  The
    message names the first element that is not, with both values."""
    assert got.shape == want.shape, f"{where}: shape {list(got.shape)} against {list(want.shape)}"
    cg, cw = classify(got), classify(want)
    if not signs:
        cg, cw = _coarse(cg), _coarse(cw)
    bad = (cg != cw).reshape(-1).nonzero()
    if bad.numel():
        i = int(bad[0])
        g, w = got.detach().cpu().reshape(-1)[i].item(), want.detach().cpu().reshape(-1)[i].item()
        name = lambda c: CLASSES[int(c.reshape(-1)[i])] if signs or int(c.reshape(-1)[i]) < 3 else "finite"
        raise AssertionError(f"{where}: {bad.numel()} of {got.numel()} elements of another class, first at {_index(got.shape, i)}: got {g!r} ({name(cg)}), "
                             f"want {w!r} ({name(cw)})")


def assert_contained(got: torch.Tensor, clean: torch.Tensor, touched: torch.Tensor, where: str = "") -> None:
    """Every element outside the boolean mask `touched` (broadcast against the tensors) has the bits it has in the clean run."""
    assert got.shape == clean.shape and got.dtype == clean.dtype, f"{where}: {list(got.shape)} {got.dtype} against {list(clean.shape)} {clean.dtype}"
    free = ~torch.as_tensor(touched, dtype=torch.bool).cpu().broadcast_to(got.shape)
    bad = ((bits(got).cpu().reshape(got.shape) != bits(clean).cpu().reshape(got.shape)) & free).reshape(-1).nonzero()
    if bad.numel():
        i = int(bad[0])
        g, c = got.detach().cpu().reshape(-1)[i].item(), clean.detach().cpu().reshape(-1)[i].item()
        raise AssertionError(f"{where}: {bad.numel()} element(s) outside the touched region differ from the clean run, first at {_index(got.shape, i)}: "
                             f"{g!r} against {c!r}")


# ------------------------------------------------------------------------------------------------------------------- operand builders
def variates(name: str, shape, scale: float = 1.0, seed: int = 1) -> torch.Tensor:
    """Seeded float32 variates of standard deviation `scale` (the package's counter-based generator: the same values on every machine)."""
    from mlx8_ws_audio_transformer_amd import weights as wts
    return (torch.from_numpy(wts.unit_variates("extreme." + name, int(np.prod(shape)), seed).reshape(shape)) * scale).float()


def plant(t: torch.Tensor, value, *index) -> torch.Tensor:
    """A copy of `t` with `value` (a name of SPECIALS or a number) at `index`."""
    out = t.clone()
    out[index] = SPECIALS[value] if isinstance(value, str) else value
    return out


def lane_positions(d: int):
    """Columns of a row of d floats read as float4 by 64 lanes: the first lane's first element, the last element of the row (the float4 that ends where
    the next row begins), and the second element of the last float4."""
    return (0, d - 1, d - 3)


# ------------------------------------------------------------------------------------------------------------------- cases
# op: a key of REF / TOL (and of the runner table of tests/test_gpu_extreme_values.py); operands: CPU float32 (labels, ids: int64) tensors; meta: shapes
# and scalars; class_only: output name -> (row, why) -- the one row of that output in which fp32 cannot return the fp64 value.
Case = collections.namedtuple("Case", "name op operands meta class_only")


def _rows(t: torch.Tensor) -> torch.Tensor:
    return t.reshape(1, -1) if t.dim() < 2 else t.reshape(-1, t.shape[-1])


def _t(operands, dt):
    return {k: (v.to(dt) if v.is_floating_point() else v) for k, v in operands.items()}


# ---- GELU (tests/test_gpu_native_decoder.py: forward within 2.5e-7 max(1, |x|) over the whole domain, backward within 2e-6)
# gelu(+inf) = +inf and its slope there 1; gelu(-inf) is NaN, as in torch (0.5 x (1 + erf) = -inf 0): a pre-activation of -inf is already an overflow and must
# surface, not turn into a clean zero.  The backward follows: NaN at -inf.
def ref_gelu(o, m, dt):
    o = _t(o, dt)
    x, dy = o["x"], o["dy"]
    cdf = 0.5 * (1.0 + torch.erf(x * 0.70710678118654752440))
    y = torch.where(x == INF, x, x * cdf)
    tail = torch.where(x == INF, torch.zeros_like(x), x * 0.39894228040143267794 * torch.exp(-0.5 * x * x))
    return {"y": y, "dx": dy * (cdf + tail)}


def tol_gelu(o, m, want):
    x = o["x"].double()
    return {"y": 2.5e-7 * x.abs().clamp(min=1.0), "dx": torch.full_like(x, 2e-6)}


# ---- LayerNorm, its backward and parameter gradients (tests/test_gpu_ops.py: 5e-6; tests/test_gpu_native_decoder.py: LN_DX_TOL of the largest |dx|, and
# four times LN_PARAM_FP32_ERR of the largest |dgamma| / |dbeta| -- its M = 255 entry, which sums more rows than the M = 5 here).
# The conditioning term below is this module's own, derived here and not taken from an existing test (DESIGN.md section 7 says so too).
# A row whose kappa = max|x| rstd exceeds 64 (mean 1e4, unit spread: 1e4) gets the term its conditioning adds: fp32 rounds the row sum log2(d) + 2 times
# relative to max|x|, so xhat carries an absolute error of ex = (log2 d + 2) u kappa; y that times |gamma|, dx = rstd (g - c1 - xhat c2) eight times
# ex rstd max|g| (xhat's error times c2, c2's error times xhat, rstd's relative error ex), dgamma the row's |dy| ex.  Ordinary rows get no such term.
LN_EPS = 1e-5
LN_DX_TOL = 4 * 1.615e-7
LN_PARAM_TOL = (4 * 3.366e-7, 4 * 4.451e-7)


def ref_layernorm(o, m, dt):
    o = _t(o, dt)
    x, g, b, dy, dres = o["x"], o["g"], o["b"], o["dy"], o["dres"]
    mean = x.mean(-1, keepdim=True)
    xc = x - mean
    rstd = 1.0 / torch.sqrt((xc * xc).mean(-1, keepdim=True) + LN_EPS)
    xhat = xc * rstd
    gg = dy * g
    c1, c2 = gg.mean(-1, keepdim=True), (gg * xhat).mean(-1, keepdim=True)
    dx = rstd * (gg - c1 - xhat * c2)
    return {"y": xhat * g + b, "dx": dx, "dx_dres": dx + dres, "dgamma": (dy * xhat).sum(0), "dbeta": dy.sum(0)}


def tol_layernorm(o, m, want):
    x, g, dy = o["x"].double(), o["g"].double(), o["dy"].double()
    d = x.shape[1]
    rstd = 1.0 / torch.sqrt(x.var(-1, unbiased=False, keepdim=True) + LN_EPS)
    kappa = x.abs().amax(-1, keepdim=True) * rstd
    ex = torch.where(kappa > 64, (math.log2(d) + 2) * U * kappa, torch.zeros_like(kappa))
    gmax = (dy * g).abs().amax(-1, keepdim=True)
    tol = {"y": 5e-6 + ex * g.abs()}
    for k in ("dx", "dx_dres"):
        tol[k] = LN_DX_TOL * want[k].abs().amax(-1, keepdim=True) + 8 * ex * rstd * gmax + torch.zeros_like(x)
    tol["dgamma"] = LN_PARAM_TOL[0] * want["dgamma"].abs().max() + (dy.abs() * ex).sum(0)
    tol["dbeta"] = LN_PARAM_TOL[1] * want["dbeta"].abs().max() + torch.zeros(d, dtype=torch.float64)
    return tol


# ---- RMSNorm, its backward and gain gradient (tests/test_gpu_qwen_ops.py: 2^-20 |y| + 1e-30; tests/test_gpu_qwen_train_ops.py: the two counted bounds)
RMS_EPS = 1e-6


def ref_rmsnorm(o, m, dt):
    o = _t(o, dt)
    x, g, dy, dres = o["x"], o["g"], o["dy"], o["dres"]
    r = torch.rsqrt((x * x).mean(-1, keepdim=True) + RMS_EPS)
    u = g * dy
    coef = r * r * r * (x * u).mean(-1, keepdim=True)
    dx = r * u - x * coef
    return {"y": g * (x * r), "dx": dx, "dx_dres": dx + dres, "dgamma": (dy * (x * r)).sum(0)}


def _rho(n):
    return (n + 8) / 2 + 2


def tol_rmsnorm(o, m, want):
    x, g, dy = o["x"].double(), o["g"].double(), o["dy"].double()
    M, d = x.shape
    n = 4 * math.ceil(d / 256)
    rho = _rho(n)
    r = torch.rsqrt((x * x).mean(-1, keepdim=True) + RMS_EPS)
    A = (r * g * dy).abs().amax(-1, keepdim=True)
    core = A * ((rho + 2) + (x * r).abs() * (3 * rho + n + 11)) + want["dx"].abs()
    return {"y": 2.0 ** -20 * want["y"].abs() + 1e-30, "dx": U * core, "dx_dres": U * (core + want["dx_dres"].abs()),
            "dgamma": U * (rho + 2 + min(M, 256) + math.ceil(M / 256)) * (dy * x * r).abs().sum(0)}


# ---- SwiGLU's element-wise half and its backward (tests/test_gpu_qwen_ops.py and tests/test_gpu_qwen_train_ops.py: the counted bounds, restated)
def ref_silu(o, m, dt):
    o = _t(o, dt)
    I = m["I"]
    g, up, dy = o["gu"][:, :I], o["gu"][:, I:], o["dy"]
    s = torch.sigmoid(g)
    return {"y": g * s * up, "dgu": torch.cat([(dy * up) * (s * (1.0 + g * (1.0 - s))), dy * (g * s)], dim=-1)}      # the kernel's grouping: g s first, so -FLT_MAX 0 = -0


def tol_silu(o, m, want):
    I = m["I"]
    g, up, dy = o["gu"][:, :I].double(), o["gu"][:, I:].double(), o["dy"].double()
    s = torch.sigmoid(g)
    t1, F, eps_s, tiny = 1.0 - s, 1.0 + g * (1.0 - s), 1.5 * g.abs() + 6, 2.0 ** -126
    b_gate = U * (dy * up * s).abs() * ((eps_s + 4) * F.abs() + (g * t1).abs() * eps_s) + tiny * (1 + (dy * up).abs() * (1 + g.abs()))
    b_up = U * (eps_s + 2) * (dy * g * s).abs() + tiny * (1 + (dy * g).abs())
    return {"y": 2.0 ** -20 * want["y"].abs() + 2.0 ** -22 * up.abs(), "dgu": torch.cat([b_gate, b_up], dim=-1)}


# ---- per-head RMSNorm + rotary embedding (tests/test_gpu_qwen_ops.py: 2^-18 of the (row, head)'s largest value; v bit-identical)
def rope_tables(rows: int):
    inv_freq = 1.0 / (1e6 ** (torch.arange(0, 128, 2, dtype=torch.float64) / 128))
    ang = torch.arange(rows, dtype=torch.float64)[:, None] * inv_freq[None, :]
    return ang.cos().float().contiguous(), ang.sin().float().contiguous()


def ref_qk_norm_rope(o, m, dt):
    o = _t(o, dt)
    Hq, Hkv = m["Hq"], m["Hkv"]
    rows = o["qkv"].shape[0]
    heads = o["qkv"].reshape(rows, Hq + 2 * Hkv, 128)
    cs, sn = o["cos"][m["positions"]][:, None, :], o["sin"][m["positions"]][:, None, :]
    out = {}
    for name, h, gain in (("q", heads[:, :Hq], o["qg"]), ("k", heads[:, Hq:Hq + Hkv], o["kg"])):
        r = torch.rsqrt((h * h).mean(-1, keepdim=True) + RMS_EPS)
        n = gain * (h * r)
        n0, n1 = n[..., :64], n[..., 64:]
        out[name] = torch.cat([n0 * cs - n1 * sn, n1 * cs + n0 * sn], dim=-1).reshape(rows, -1)
    out["v"] = heads[:, Hq + Hkv:].reshape(rows, -1)
    return out


def tol_qk_norm_rope(o, m, want):
    tol = {}
    for name in ("q", "k"):
        w = want[name]
        mag = torch.nan_to_num(w, nan=0.0).reshape(w.shape[0], -1, 128).abs().amax(-1, keepdim=True)      # a head of zeros and one NaN: the zeros are exact
        tol[name] = (2.0 ** -18 * mag).expand(-1, -1, 128).reshape(w.shape)
    tol["v"] = torch.zeros_like(want["v"])
    return tol


# ---- row softmax and its backward (tests/test_gpu_native_decoder.py: 1e-6, the backward 1e-6 of max(1, largest |ds|))
def ref_softmax(o, m, dt):
    o = _t(o, dt)
    cols, scale = m["cols"], m["scale"]
    v = o["s"][:, :cols] * scale
    e = torch.exp(v - v.amax(-1, keepdim=True))
    p = e / e.sum(-1, keepdim=True)
    dp = o["dp"][:, :cols]
    return {"p": p, "ds": scale * p * (dp - (p * dp).sum(-1, keepdim=True))}


def tol_softmax(o, m, want):
    ds = want["ds"]
    big = torch.nan_to_num(ds, nan=0.0, posinf=0.0, neginf=0.0).abs().max().clamp(min=1.0)
    return {"p": torch.full_like(want["p"], 1e-6), "ds": torch.full_like(ds, 1e-6) * big}


# ---- cross-entropy (tests/test_gpu_native_decoder.py: the loss within 1e-5, dlogits within 1e-7)
def ref_cross_entropy(o, m, dt):
    o = _t(o, dt)
    vocab, labels = m["vocab"], o["labels"]
    z = o["logits"][:, :vocab]
    counted = labels != -100
    n = int(counted.sum())
    mx = z.amax(-1, keepdim=True)
    e = torch.exp(z - mx)
    lse = mx[:, 0] + torch.log(e.sum(-1))
    lab = labels.clamp(min=0)
    row_loss = torch.where(counted, lse - z.gather(1, lab[:, None])[:, 0], torch.zeros_like(lse))
    onehot = torch.zeros_like(z).scatter_(1, lab[:, None], 1.0)
    dz = torch.where(counted[:, None], (e / e.sum(-1, keepdim=True) - onehot) / n, torch.zeros_like(z))
    return {"loss": (row_loss.sum() / n).reshape(1, 1), "dlogits": dz}


def tol_cross_entropy(o, m, want):
    return {"loss": torch.full((1, 1), 1e-5, dtype=torch.float64), "dlogits": torch.full_like(want["dlogits"], 1e-7)}


# ---- column sums (tests/test_gpu_decoder_param_ops.py: (M - 1) u sum |a|).  Both kernels add in a documented order, restated here, so that the columns
# named in meta["ordered"] -- 1e30, -1e30, 1: a different number in every order, and in fp64 another operation -- are held to the fp32 restatement exactly.
SLAB = 256


def _chain(rows: torch.Tensor) -> torch.Tensor:
    acc = torch.zeros_like(rows[0])
    for r in rows:
        acc = acc + r
    return acc


def ref_column_sums(o, m, dt):
    """awt_op_column_sums: per slab of 256 rows wave w adds rows w, w + 4, ... in order, the four waves as (0 + 1) + (2 + 3), the slabs in order."""
    a = _t(o, dt)["a"]
    total = torch.zeros_like(a[0])
    for r0 in range(0, a.shape[0], SLAB):
        w = [_chain(a[r0:r0 + SLAB][k::4]) if a[r0:r0 + SLAB][k::4].shape[0] else torch.zeros_like(a[0]) for k in range(4)]
        total = total + ((w[0] + w[1]) + (w[2] + w[3]))
    return {"sums": total}


def ref_column_sums_ld(o, m, dt):
    """awt_op_column_sums_ld: a thread walks its columns top to bottom through a slab of 256 rows, the slabs are added in order."""
    a = _t(o, dt)["a"][:, m["col"]:m["col"] + m["width"]]
    total = torch.zeros_like(a[0])
    for r0 in range(0, a.shape[0], SLAB):
        total = total + _chain(a[r0:r0 + SLAB])
    return {"sums": total}


def tol_column_sums(o, m, want):
    a = o["a"].double()[:, m.get("col", 0):m.get("col", 0) + m["width"]]
    return {"sums": (a.shape[0] - 1) * U * a.abs().sum(0)}


# ---- embedding (one fp32 addition per element: correctly rounded, so one rounding of the value)
def ref_embed(o, m, dt):
    o = _t(o, dt)
    ids = o["ids"]
    L = ids.shape[1]
    pos = o["pos"][m["pos0"]:m["pos0"] + L].repeat(ids.shape[0], 1)
    return {"x": o["tok"][ids.reshape(-1)] + pos}


def tol_embed(o, m, want):
    return {"x": U * want["x"].abs()}


# ---- BatchNorm statistics, BatchNorm + ReLU + pooling and its backward (tests/test_gpu_cnn_classifier.py `_bn_bounds`, tests/test_gpu_waveform_classifier.py:
# the same bounds for the two max-4 modes), per channel.  pool: 0 the mean over T, 2 / 4 max over windows of 2 / 4 frames, 5 max-4 then the mean.
BN_EPS = 1e-5


def ref_batchnorm(o, m, dt):
    import torch.nn.functional as F
    o = _t(o, dt)
    B, T, pool = m["B"], m["T"], m["pool"]
    with torch.enable_grad():
        x, g, b = (o[k].detach().clone().requires_grad_(True) for k in ("x", "g", "b"))
        mean = x.mean(0)
        var = ((x - mean) * (x - mean)).mean(0)
        z = (x - mean) * (1.0 / torch.sqrt(var + BN_EPS)) * g + b
        a = torch.relu(z).reshape(B, T, -1).transpose(1, 2)                                       # [B, C, T]
        if pool == 0:
            y = a.mean(-1, keepdim=True)
        else:
            y = F.max_pool1d(a, 2 if pool == 2 else 4)
            y = y.mean(-1, keepdim=True) if pool == 5 else y
        y = y.transpose(1, 2).reshape(-1, x.shape[1])
        dx, dg, db = torch.autograd.grad(y, (x, g, b), o["dy"])
    return {"mean": mean.detach(), "var": var.detach(), "y": y.detach(), "dx": dx, "dgamma": dg, "dbeta": db}


def tol_batchnorm(o, m, want):
    x, g, dy = o["x"].double(), o["g"].double(), o["dy"].double()
    T, pool = m["T"], m["pool"]
    var = want["var"]
    rstd = (var + BN_EPS).rsqrt()
    kappa = x.abs().amax(0) * rstd
    rel = 5e-5 + 8 * U * kappa
    xhat_max = ((x - want["mean"]) * rstd).abs().amax(0)
    gmax = dy.abs().amax(0) / {0: T, 2: 1, 4: 1, 5: T // 4}[pool]
    return {"mean": 1e-5 * want["mean"].abs() + 1e-6,
            "var": (2e-5 + 4 * U * x.abs().amax(0) / var.sqrt().clamp(min=1e-3)) * var + 1e-9,
            "y": 2e-5 + 16 * U * kappa * g.abs() + 2e-5 * want["y"].abs(),
            "dx": rel * torch.maximum(want["dx"].abs().amax(0), g.abs() * rstd * gmax) + 1e-6,
            "dgamma": rel * torch.maximum(want["dgamma"].abs(), gmax * xhat_max.clamp(min=1.0)) + 1e-6,
            "dbeta": rel * torch.maximum(want["dbeta"].abs(), gmax) + 1e-6}


REF = {"batchnorm": ref_batchnorm, "gelu": ref_gelu, "layernorm": ref_layernorm, "rmsnorm": ref_rmsnorm, "silu": ref_silu, "qk_norm_rope": ref_qk_norm_rope, "softmax": ref_softmax,
       "cross_entropy": ref_cross_entropy, "column_sums": ref_column_sums, "column_sums_ld": ref_column_sums_ld, "embed": ref_embed}
TOL = {"batchnorm": tol_batchnorm, "gelu": tol_gelu, "layernorm": tol_layernorm, "rmsnorm": tol_rmsnorm, "silu": tol_silu, "qk_norm_rope": tol_qk_norm_rope, "softmax": tol_softmax,
       "cross_entropy": tol_cross_entropy, "column_sums": tol_column_sums, "column_sums_ld": tol_column_sums, "embed": tol_embed}

Expected = collections.namedtuple("Expected", "want64 want32 bound value fp32_held class_only ordered")


def expected(case: Case) -> dict:
    """Output name -> Expected, every tensor as [rows, columns] on the CPU: the fp64 and fp32 restatements, the bound, and four disjoint element masks
    (module docstring): value, fp32_held, class_only, ordered."""
    w64 = REF[case.op](case.operands, case.meta, torch.float64)
    w32 = REF[case.op](case.operands, case.meta, torch.float32)
    with torch.no_grad():
        tol = TOL[case.op](case.operands, case.meta, w64)
    out = {}
    for k in w64:
        a, b = _rows(w64[k].detach()), _rows(w32[k].detach())
        bound = _rows(tol[k].broadcast_to(w64[k].shape)).double()
        fin = torch.isfinite(a)
        ordered = torch.zeros_like(fin)
        for c in (case.meta.get("ordered", ()) if k == "sums" else ()):          # held to the fp32 restatement bit for bit (ref_column_sums), not to fp64
            ordered[:, c] = True
        reach = torch.isfinite(b) & torch.isfinite(bound)
        near = reach & ((b.double() - a).abs() <= 4 * bound)
        class_only = fin & ~reach & ~ordered
        held = fin & reach & ~near & ~ordered
        value = fin & ~ordered & ~class_only & ~held
        named = torch.zeros_like(fin)
        if k in case.class_only:
            named[case.class_only[k][0]] = True
        value = value | (fin & ~ordered & ~named)            # outside the named row nothing is excused, whatever the restatements say
        out[k] = Expected(a, b, bound, value, held & named, class_only & named, ordered)
    return out


def unexplained(case: Case) -> dict:
    """Output name -> rows holding an element that is finite in fp64, not reached by the fp32 restatement within four bounds, and outside the case's named
    row: empty for every case (tests/test_extreme_values_host.py), or the GPU test would hold a kernel to a value fp32 cannot return."""
    rows = {}
    for k, e in expected(case).items():
        b, bound = e.want32, e.bound
        far = torch.isfinite(e.want64) & ~e.ordered & ~(torch.isfinite(b) & torch.isfinite(bound) & ((b.double() - e.want64).abs() <= 4 * bound))
        if k in case.class_only:
            far[case.class_only[k][0]] = False
        rows[k] = far.any(-1).nonzero().reshape(-1).tolist()
    return rows


def _raise(case, k, g, mask, e, ref, what):
    i = int(mask.reshape(-1).nonzero()[0])
    raise AssertionError(f"{case.name}: {k}: {int(mask.sum())} value(s) outside the bound, first at {_index(g.shape, i)}: got {g.reshape(-1)[i].item()!r}, "
                         f"want {ref.reshape(-1)[i].item()!r} ({what}), bound {e.bound.reshape(-1)[i].item():.3e}")


def check(case: Case, got: dict) -> None:
    """The comparison of the GPU test.  Every element: the class of the fp32 restatement's.  Value elements: within the bound of fp64 (in the named row: of
    fp64 or of the fp32 restatement, which may differ there by up to four bounds).  fp32-held elements: within the bound of the fp32 restatement.
    The columns of meta["ordered"]: the fp32 restatement's bits."""
    exp = expected(case)
    assert set(got) == set(exp), (sorted(got), sorted(exp))
    for k, e in exp.items():
        g = _rows(got[k].detach().cpu())
        assert_same_class(g, e.want32, f"{case.name}: {k}")
        err64, err32 = (g.double() - e.want64).abs(), (g.double() - e.want32.double()).abs()
        named = torch.zeros_like(e.value)
        if k in case.class_only:
            named[case.class_only[k][0]] = True
        bad = e.value & ~((err64 <= e.bound) | (named & (err32 <= e.bound)))
        if bad.any():
            _raise(case, k, g, bad, e, e.want64, "fp64")
        bad = e.fp32_held & ~(err32 <= e.bound)
        if bad.any():
            _raise(case, k, g, bad, e, e.want32, "the fp32 restatement; fp64 is out of fp32's reach here")
        for c in e.ordered[0].nonzero().reshape(-1).tolist():
            assert bits(g[:, c]).equal(bits(e.want32[:, c])), f"{case.name}: {k}: column {c} is {g[0, c].item()!r}, the fp32 sum in the kernel's order is {e.want32[0, c].item()!r}"


# ------------------------------------------------------------------------------------------------------------------- the case list
def _gelu_cases():
    x = variates("gelu.x", (16,), 2.0)
    for i, name in enumerate(SPECIALS):                    # element-wise: every special at once, each in its own element, ordinary values around them
        x = plant(x, name, i)
    return [Case("gelu", "gelu", {"x": x, "dy": variates("gelu.dy", (16,))}, {}, {})]


def _norm_operands(tag, M, d):
    return {"x": variates(tag + ".x", (M, d), 2.0), "g": 1.0 + 0.3 * variates(tag + ".g", (d,)), "dy": variates(tag + ".dy", (M, d)),
            "dres": variates(tag + ".dres", (M, d))}


def _overflow_rows(name, outputs, row, why):
    return {k: (row, why) for k in outputs} if name in OVERFLOWING else {}


def _layernorm_cases():
    """M = 5: one workgroup of four rows plus one.  Row 1 takes the special; row 2 has mean 1e4 and unit spread, row 4 is constant: with a one-pass
    variance (E[x^2] - E[x]^2) row 2 loses every digit, and row 4 comes out as noise instead of beta."""
    cases = []
    for d in (128, 1280):
        base = _norm_operands(f"ln{d}", 5, d)
        base["b"] = variates(f"ln{d}.b", (d,))
        base["x"][2] = 1e4 + variates(f"ln{d}.row2", (d,))
        base["x"][4] = 3.0
        cases.append(Case(f"layernorm-d{d}-clean", "layernorm", base, {}, {}))
        for name in SPECIALS:
            for col in lane_positions(d):
                o = dict(base, x=plant(base["x"], name, 1, col))
                why = "the squared deviation of the row overflows fp32: rstd = 0, the row comes out as beta"
                co = _overflow_rows(name, ("y", "dx", "dx_dres"), 1, why)
                if co:
                    co["dgamma"] = (0, "row 1's xhat is 0 in fp32, so every column misses that row's term")
                cases.append(Case(f"layernorm-d{d}-{name}-col{col}", "layernorm", o, {}, co))
    return cases


def _rmsnorm_cases():
    cases = []
    for d in (128, 260):
        base = _norm_operands(f"rms{d}", 3, d)
        cases.append(Case(f"rmsnorm-d{d}-clean", "rmsnorm", base, {}, {}))
        for name in SPECIALS:
            for col in lane_positions(d):
                o = dict(base, x=plant(base["x"], name, 1, col))
                why = "the sum of squares overflows fp32: r = 0, the row comes out as zeros"
                co = _overflow_rows(name, ("y", "dx", "dx_dres"), 1, why)
                if co:
                    co["dgamma"] = (0, "row 1's x r is 0 in fp32, so every column misses that row's term")
                cases.append(Case(f"rmsnorm-d{d}-{name}-col{col}", "rmsnorm", o, {}, co))
    return cases


def _silu_cases():
    """M = 2, I = 384.  Element-wise: every special at once in row 0 of the gate (first case) or of the up half (second), the first and last lanes
    included; silu(-inf) * up and 0 * inf are among them."""
    M, I = 2, 384
    gu, dy = variates("silu.gu", (M, 2 * I), 4.0), variates("silu.dy", (M, I))
    cols = [0, I - 1, I - 3] + list(range(5, 5 + len(SPECIALS)))
    gate, up = gu.clone(), gu.clone()
    for i, name in enumerate(SPECIALS):
        gate, up = plant(gate, name, 0, cols[i]), plant(up, name, 0, I + cols[i])
    up = plant(plant(up, 0.0, 0, 40), "+inf", 0, I + 40)                                       # 0 * inf
    why = "a product with FLT_MAX or 1e20 leaves fp32"
    return [Case("silu-gate", "silu", {"gu": gate, "dy": dy}, {"I": I}, {"y": (0, why), "dgu": (0, why)}),
            Case("silu-up", "silu", {"gu": up, "dy": dy}, {"I": I}, {"y": (0, why), "dgu": (0, why)})]


def _qk_cases():
    """B = 1, Lq = 2, Hq = 2, Hkv = 1 at positions 1, 2: the special goes into the second q head or the k head of row 0; every other head must come out as
    in the clean case (tests/test_gpu_extreme_values.py compares the bits)."""
    Hq, Hkv, rows, Tmax = 2, 1, 2, 4
    cos, sin = rope_tables(Tmax)
    base = {"qkv": variates("rope.qkv", (rows, (Hq + 2 * Hkv) * 128), 1.5), "qg": 1.0 + 0.3 * variates("rope.qg", (128,)),
            "kg": 1.0 + 0.3 * variates("rope.kg", (128,)), "cos": cos, "sin": sin}
    meta = {"Hq": Hq, "Hkv": Hkv, "B": 1, "Lq": 2, "Tmax": Tmax, "positions": torch.tensor([1, 2])}
    cases = [Case("qk_norm_rope-clean", "qk_norm_rope", base, dict(meta, head=None), {})]
    for name in SPECIALS:
        for head, dim in ((1, 0), (1, 127), (2, 64)):
            o = dict(base, qkv=plant(base["qkv"], name, 0, 128 * head + dim))
            out = "q" if head < Hq else "k"
            co = _overflow_rows(name, (out,), 0, "the head's sum of squares overflows fp32: r = 0")
            cases.append(Case(f"qk_norm_rope-{name}-head{head}-dim{dim}", "qk_norm_rope", o, dict(meta, head=head), co))
    return cases


def _softmax_cases():
    """Padding columns hold NaN.  Rows: +inf in it (all NaN), all -inf (all NaN), some -inf (exact zeros there), ordinary; with scale 1, rows of +-1e38
    (the difference to the maximum does not overflow) and 1e38 next to -inf."""
    rows, cols, ld = 4, 70, 72
    s, dp = variates("softmax.s", (rows, ld), 6.0), variates("softmax.dp", (rows, ld))
    s[:, cols:], dp[:, cols:] = NAN, NAN
    a = s.clone()
    a[0, 69] = INF
    a[1, :cols] = -INF
    a[2, [0, 33, 69]] = -INF
    b = variates("softmax.big", (rows, ld))
    b[:, cols:] = NAN
    b[0, :cols] = torch.where(torch.arange(cols) % 2 == 0, 1e38, -1e38)
    b[1, :cols] = -1e38
    b[2, [3, 68]] = 1e38
    b[3, [0, 69]] = -INF
    one = torch.tensor([[INF], [-INF], [1.0], [1e38]]).repeat(1, 4)
    one[:, 1:] = NAN
    return [Case("softmax-70in72", "softmax", {"s": a, "dp": dp}, {"cols": cols, "scale": 0.125}, {}),
            Case("softmax-70in72-1e38", "softmax", {"s": b, "dp": dp}, {"cols": cols, "scale": 1.0}, {}),
            Case("softmax-1in4", "softmax", {"s": one, "dp": plant(variates("softmax.dp1", (4, 4)), NAN, slice(None), slice(1, None))}, {"cols": 1, "scale": 1.0}, {})]


def _ce_cases():
    """M = 4, vocab = 70 in a pitch of 72 whose padding columns hold NaN throughout (they change nothing)."""
    M, vocab, ld = 4, 70, 72
    z = variates("ce.logits", (M, ld), 3.0)
    z[:, vocab:] = NAN
    labels = torch.tensor([5, 69, -100, 0])
    meta = {"vocab": vocab}
    return [Case("cross_entropy-clean", "cross_entropy", {"logits": z, "labels": labels}, meta, {}),
            Case("cross_entropy-label_logit_-inf", "cross_entropy", {"logits": plant(z, "-inf", 1, 69), "labels": labels}, meta, {}),      # loss +inf
            Case("cross_entropy-other_logit_-inf", "cross_entropy", {"logits": plant(z, "-inf", 1, 3), "labels": labels}, meta, {}),
            Case("cross_entropy-nan_in_ignored_row", "cross_entropy", {"logits": plant(z, "nan", 2, 7), "labels": labels}, meta, {}),      # loss finite
            Case("cross_entropy-nan_in_counted_row", "cross_entropy", {"logits": plant(z, "nan", 3, 69), "labels": labels}, meta, {})]     # loss NaN, row 3 NaN


def _column_sum_cases():
    """M = 300 crosses the slab of 256 rows.  Column 5: one NaN (in the second slab); column 9: +inf and -inf, a slab apart; columns 20 and 21: 1e30, -1e30,
    1 and 1e30, 1, -1e30 in rows 0 .. 2, the `ordered` columns."""
    M, width = 300, 128
    a = variates("colsum.a", (M, width))
    a[270, 5] = NAN
    a[3, 9], a[260, 9] = INF, -INF
    a[0:3, 20] = torch.tensor([1e30, -1e30, 1.0])
    a[0:3, 21] = torch.tensor([1e30, 1.0, -1e30])
    wide = variates("colsum.wide", (M, 2 * width))
    wide[:, width:] = a
    return [Case("column_sums-300x128", "column_sums", {"a": a}, {"width": width, "ordered": (20, 21)}, {}),
            Case("column_sums_ld-300x128in256", "column_sums_ld", {"a": wide}, {"col": width, "width": width, "ordered": (20, 21)}, {})]


def _embed_cases():
    """L = 3, d = 128: ids 2, 0, 2 -- table row 2 holds the special, so positions 0 and 2 carry it and position 1 must not."""
    d, ids = 128, torch.tensor([[2, 0, 2]])
    tok, pos = variates("embed.tok", (4, d)), variates("embed.pos", (5, d))
    cases = []
    for name in SPECIALS:
        for col in lane_positions(d):
            cases.append(Case(f"embed-{name}-col{col}", "embed", {"ids": ids, "tok": plant(tok, name, 2, col), "pos": pos}, {"pos0": 1}, {}))
    return cases


BN = dict(B=2, T=9, C=128, poisoned=7, constant=5, offset=9)


def bn_state(poison=None):
    """B = 2, T = 9, C = 128: channel 5 is constant, channel 9 has mean 1e4 and unit spread; `poison` goes into one element of channel 7."""
    B, T, C = BN["B"], BN["T"], BN["C"]
    x = variates("bn.x", (B * T, C), 1.5)
    x[:, BN["constant"]] = 1.7
    x[:, BN["offset"]] = 1e4 + variates("bn.offset", (B * T,))
    if poison is not None:
        x[5, BN["poisoned"]] = poison
    return x, 1.0 + 0.3 * variates("bn.g", (C,)), variates("bn.b", (C,))


def bn_dy(pool):
    T = BN["T"]
    return variates("bn.dy", (BN["B"] * {0: 1, 2: T // 2, 4: T // 4, 5: 1}[pool], BN["C"]))


def _bn_cases():
    """Every channel of the clean state against fp64 in each pool mode, statistics, forward and backward: the constant and the offset channel pin chan_merge
    and the first-row mean (E[x^2] - E[x]^2 would lose the offset channel's variance, and with it xhat in both directions)."""
    x, g, b = bn_state()
    return [Case(f"batchnorm-pool{pool}", "batchnorm", {"x": x, "g": g, "b": b, "dy": bn_dy(pool)}, {"B": BN["B"], "T": BN["T"], "pool": pool}, {})
            for pool in (0, 2, 4, 5)]


def cases() -> list:
    return (_bn_cases() + _gelu_cases() + _layernorm_cases() + _rmsnorm_cases() + _silu_cases() + _qk_cases() + _softmax_cases() + _ce_cases() + _column_sum_cases()
            + _embed_cases())
