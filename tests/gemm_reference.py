"""Reference of the GEMM's fused epilogues (csrc/gemm.hip, csrc/gemm_pp.h; one launch through awt_op_linear_fused) in float64, plain torch, no GPU needed.

    p = Problem(x, w, bias, segs, M)          the contraction: C[m, n] = sum over K segments of x[row(m), xcol .. + k) . w[n, wcol .. + k)
    exact(p, epi, ...)                        the epilogue's mathematical result
    rounded(p, epi, terms, ...)               the same with the roundings of the kernels' operands and of the stored output, and nothing else
    rounded32(p, epi, terms, ...)             `rounded` with every product accumulated, and the epilogue evaluated, in float32 by torch on the CPU
    bound(p, epi, terms, ...)                 (exact, tol): per output tensor tol = 4 x (max |rounded - exact| + max |rounded32 - rounded|)
    check(label, got, ex, tol)                asserts max |got - exact| <= tol per output tensor, prints both normalised by max |exact|

All three return a dict of float64 tensors: "y" [M, N] (EPI_QKV: "q", "k", "v" [B, H, S, 64], head-major); "pre" [M, N] of EPI_BF16_GELU_SAVE; with
terms = 5 a plane output also has its e4m3 image "<name>_hi8" (the value that image stands for).

Roundings restated by `rounded`, read off the kernels (common.h, gemm.hip):
  * terms 1 / 2: operands bf16 / fp16, one product.  terms 3 / 4: hi = rne(x), lo = rne(x - hi) in bf16 / fp16, products a_hi b_hi + a_hi b_lo + a_lo b_hi
    (fp16-exact weights have b_lo = 0: the exact-weight kernels drop a product that is zero).  terms 5: a16 b16 in fp16, a8 bl8 + al8 b8 in e4m3 with
    x8 = e4m3(x 2^s) 2^-s and xl8 = e4m3((x - fp16(x)) 2^(s + 11)) 2^-(s + 11), s = kF8Act for activations, kF8Wgt for weights (clamped to +-448 first);
  * the stored output: fp32; or a plane pair in the operand format (terms 5: fp16 + lo8 at s + 11, s = kF8Act, kF8Q for q, kF8KV for k and v);
    the saved pre-activation is a bf16 pair (its hi plane alone with one product).
Not restated: the order of the fp32 sums and the polynomial erf / exp of the epilogue (1.6e-7 absolute).  Operand rounding alone is too tight a yardstick
for that: at K = 64 .. 3072 fp32 accumulation differs from `rounded` by 2.4e-7 .. 5.8e-7 in split-fp16, against 1.3e-7 .. 6.2e-7 of operand rounding -- hence
the second term of the bound, also computed from the reference alone.  The factor 4 is tests/attention_reference.py's.

Decoders of the kernels' raw bytes (written from the formats' descriptions in common.h, not with library code): planes16, e4m3, join_f16f8, split_lines.

`defect=` plants one wrong formula in rounded32, for the host test that the bound tells each of them from a correct kernel (DEFECTS)."""
import math

import torch

F8_ACT, F8_WGT, F8_Q, F8_KV, F8_LO = -2, 4, 2, 0, 11           # common.h kF8Act, kF8Wgt, kF8Q, kF8KV, kF8Lo
F16_MAX = 65504.0
FACTOR = 4.0
EPI = {"f32": 0, "f32_resid": 1, "planes": 2, "gelu": 3, "qkv": 4, "gelu_pos": 5, "gelu_save": 6, "dgelu": 7}
F32_EPILOGUES = ("f32", "f32_resid", "gelu_pos")
PRODUCTS = {1: 1, 2: 1, 3: 3, 4: 3, 5: 3}
DEFECTS = ("out_lo", "x_lo", "scale_k", "scale_last_head", "tanh", "pos_row", "resid_row", "pad_row", "pre_hi", "q_hi8_unscaled")


def make_inputs(rows, N, K, seed):
    """The operator tests' inputs: x [rows, K] ~ N(0, 1), w [N, K] ~ N(0, 1 / K), and a bias ~ N(0, 1) that shifts a quarter of the columns by +-4, so
    that both tails of the GELU are hit."""
    g = torch.Generator().manual_seed(seed)
    x, w, bias = torch.randn((rows, K), generator=g), torch.randn((N, K), generator=g) * K ** -0.5, torch.randn((N,), generator=g)
    bias[0::8] += 4.0
    bias[4::8] -= 4.0
    return x, w, bias


def conv_segs(S, Cin):
    """The stride-2 conv stem as three K segments over one activation [B 2 S, Cin] and a weight [N, 3 Cin]: tap t reads row 2 s + t - 1 of the clip."""
    return [(0, t * Cin, Cin, S, 2 * S, 2, t - 1) for t in range(3)]


# ---------------------------------------------------------------- number formats (float64 in, float64 out)
def _f32(x):
    return x.float().double()


def _bf16(x):
    return x.float().bfloat16().double()


def _fp16(x):
    return x.float().half().double()


def _e4m3(x, s):
    """The value the e4m3 image of x 2^s stands for: x clamped to +-448 2^-s, x 2^s rounded to nearest even on the grid of 3 mantissa bits with the
    least exponent -6 (subnormal step 2^-9), times 2^-s."""
    v = x.double().clamp(-448.0 * 2.0 ** -s, 448.0 * 2.0 ** -s) * 2.0 ** s
    _, e = torch.frexp(v.abs())                                 # |v| = m 2^e, m in [0.5, 1)
    step = torch.exp2((e - 1).clamp_min(-6).double() - 3)
    return torch.round(v / step) * step * 2.0 ** -s


def bf16_pair(x):
    """The value of the bf16 hi + lo pair of x: what a saved pre-activation holds."""
    hi = _bf16(x)
    return hi + _bf16(x - hi)


def _split(x, terms):
    hi = _bf16(x) if terms in (1, 3) else _fp16(x)
    if terms in (1, 2):
        return hi, torch.zeros_like(hi)
    return hi, (_bf16(x - hi) if terms == 3 else _fp16(x - hi))


# ---------------------------------------------------------------- the contraction
class Problem:
    """x [x_rows, ldx], w [N, ldw] and bias [N] (or None) as float32 CPU tensors; segs: (xcol, wcol, k, rows_out, rows_in, row_mul, row_add) each,
    None = one plain segment; M output rows.  The accumulators are cached per (kind, terms): every epilogue of a problem shares them."""

    def __init__(self, x, w, bias=None, segs=None, M=None):
        self.x, self.w, self.bias = x.float().cpu(), w.float().cpu(), (None if bias is None else bias.float().cpu())
        self.M = self.x.shape[0] if M is None else M
        self.N = self.w.shape[0]
        self.segs = [(0, 0, self.x.shape[1], self.M, self.M, 1, 0)] if segs is None else list(segs)
        self._acc = {}

    def rows(self, seg, pad_row=False):
        """(source row of each output row, whether it is read) under the row map; pad_row: the defect that reads the row before the group instead of zero."""
        _, _, _, rows_out, rows_in, row_mul, row_add = seg
        m = torch.arange(self.M)
        grp, r = m // rows_out, m % rows_out
        sr = r * row_mul + row_add
        ok = (sr >= 0) & (sr < rows_in)
        src = grp * rows_in + sr
        if pad_row:
            ok = ok | ((src >= 0) & (src < self.x.shape[0]))
        return src.clamp(0, self.x.shape[0] - 1), ok

    def acc(self, kind, terms=0, defect=None):
        """[M, N] float64: kind "exact" (no rounding), "rounded" (operand roundings, float64 sums), "rounded32" (the same, float32 products and sums)."""
        key = (kind, terms if kind != "exact" else 0, defect if defect in ("x_lo", "pad_row") else None)
        if key not in self._acc:
            self._acc[key] = self._contract(*key)
        return self._acc[key]

    def _contract(self, kind, terms, defect):
        f32 = kind == "rounded32"
        mm = (lambda a, b: a.float() @ b.float().t()) if f32 else (lambda a, b: a @ b.t())
        total = torch.zeros((self.M, self.N), dtype=torch.float32 if f32 else torch.float64)
        for seg in self.segs:
            xcol, wcol, k = seg[:3]
            src, ok = self.rows(seg, defect == "pad_row")
            a = self.x[src, xcol:xcol + k].double() * ok[:, None].double()
            b = self.w[:, wcol:wcol + k].double()
            if kind == "exact":
                total = total + a @ b.t()
            elif terms == 5:
                a16, b16 = _fp16(a), _fp16(b)
                total = total + mm(a16, b16) + mm(_e4m3(a, F8_ACT), _e4m3(b - b16, F8_WGT + F8_LO))
                if defect != "x_lo":
                    total = total + mm(_e4m3(a - a16, F8_ACT + F8_LO), _e4m3(b, F8_WGT))
            else:
                (ah, al), (bh, bl) = _split(a, terms), _split(b, terms)
                total = total + mm(ah, bh)
                if PRODUCTS[terms] == 3:
                    total = total + mm(ah, bl)
                    if defect != "x_lo":
                        total = total + mm(al, bh)
        return total.double()


# ---------------------------------------------------------------- the epilogues
def _gelu(v, tanh=False):
    if tanh:
        return 0.5 * v * (1.0 + torch.tanh(math.sqrt(2.0 / math.pi) * (v + 0.044715 * v ** 3)))
    return 0.5 * v * (1.0 + torch.erf(v / math.sqrt(2.0)))


def _dgelu(x):
    return 0.5 * (1.0 + torch.erf(x / math.sqrt(2.0))) + x * torch.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)


def _head_major(v, S, H):
    """[B S, 3 H 64] -> q, k, v [B, H, S, 64] each"""
    B = v.shape[0] // S
    t = v.reshape(B, S, 3, H, 64).permute(2, 0, 3, 1, 4)
    return t[0].contiguous(), t[1].contiguous(), t[2].contiguous()


def _epilogue(p, acc, epi, dt, scale=1.0, S=0, H=0, resid=None, pos=None, rows_pos=0, pre=None, defect=None):
    """The unrounded outputs of one epilogue from the accumulator, evaluated in dtype dt (float64, or float32 for rounded32)."""
    c = lambda t: None if t is None else t.double().cpu().to(dt)
    v = acc.to(dt)
    if p.bias is not None:
        v = v + c(p.bias)
    m = torch.arange(p.M)
    if epi == "f32":
        return {"y": v}
    if epi == "f32_resid":
        return {"y": c(resid)[(m + 1) % p.M if defect == "resid_row" else m] + v}
    if epi == "planes":
        return {"y": v * torch.tensor(scale, dtype=torch.float32).to(dt)}
    if epi == "gelu":
        return {"y": _gelu(v, defect == "tanh")}
    if epi == "gelu_save":
        return {"y": _gelu(v, defect == "tanh"), "pre": v}
    if epi == "gelu_pos":
        return {"y": _gelu(v, defect == "tanh") + c(pos)[((m + 1) if defect == "pos_row" else m) % rows_pos]}
    if epi == "dgelu":
        return {"y": v * _dgelu(_bf16(pre).to(dt) if defect == "pre_hi" else c(pre))}
    assert epi == "qkv" and p.N == 3 * H * 64 and p.M % S == 0
    d, sc = H * 64, torch.tensor(scale, dtype=torch.float32).to(dt)
    v = v.clone()
    lo, hi = (d, 2 * d) if defect == "scale_k" else (0, d - 64 if defect == "scale_last_head" else d)
    v[:, lo:hi] = v[:, lo:hi] * sc
    q, k, vv = _head_major(v, S, H)
    return {"q": q, "k": k, "v": vv}


def _store(outs, epi, terms, skip_v8=False, defect=None, unscaled_q=None):
    """The values the stored bytes stand for: fp32, or the plane pair of the precision (with its e4m3 image under terms 5)."""
    res = {}
    for name, v in outs.items():
        v = _f32(v)
        if epi in F32_EPILOGUES:
            res[name] = v
        elif name == "pre":
            hi = _bf16(v)
            res[name] = hi + (_bf16(v - hi) if PRODUCTS[terms] == 3 and defect != "out_lo" else 0.0)
        elif terms == 5:
            if epi == "dgelu":
                v = v.clamp(-F16_MAX, F16_MAX)
            s = {"q": F8_Q, "k": F8_KV, "v": F8_KV}.get(name, F8_ACT)
            hi = _fp16(v)
            if name == "v" and skip_v8:                        # the single-product P V attention reads v's fp16 plane alone: no e4m3 image is written
                res[name] = hi
                continue
            res[name] = hi + (_e4m3(v - hi, s + F8_LO) if defect != "out_lo" else 0.0)
            res[name + "_hi8"] = _e4m3(_f32(unscaled_q) if name == "q" and defect == "q_hi8_unscaled" else v, s)
        else:
            hi, lo = _split(v, terms)
            res[name] = hi + (lo if defect != "out_lo" else 0.0)
    return res


def exact(p, epi, **side):
    side.pop("skip_v8", None)
    outs = _epilogue(p, p.acc("exact"), epi, torch.float64, **side)
    return outs


def _with_images(ex, like):
    """`exact` under the names of a rounded result: an e4m3 image stands for the same exact value as its plane pair."""
    return {name: ex[name[:-4] if name.endswith("_hi8") else name] for name in like}


def rounded(p, epi, terms, skip_v8=False, **side):
    return _store(_epilogue(p, p.acc("rounded", terms), epi, torch.float64, **side), epi, terms, skip_v8)


def rounded32(p, epi, terms, skip_v8=False, defect=None, **side):
    assert defect is None or defect in DEFECTS
    outs = _epilogue(p, p.acc("rounded32", terms, defect), epi, torch.float32, defect=defect, **side)
    unscaled = None
    if defect == "q_hi8_unscaled":
        unscaled = _epilogue(p, p.acc("rounded32", terms), epi, torch.float32, **dict(side, scale=1.0))["q"]
    return _store(outs, epi, terms, skip_v8, defect, unscaled)


def errors(got, ex):
    """{name: max |got - exact|} over the outputs of `got`"""
    ex = _with_images(ex, got)
    return {name: float((got[name].double().cpu() - ex[name]).abs().max()) for name in got}


def bound(p, epi, terms, skip_v8=False, **side):
    """(exact under the names of the stored outputs, {name: tol}): tol = FACTOR x (max |rounded - exact| + max |rounded32 - rounded|)"""
    rnd, r32 = rounded(p, epi, terms, skip_v8, **side), rounded32(p, epi, terms, skip_v8, **side)
    ex = _with_images(exact(p, epi, **side), rnd)
    e_rnd = errors(rnd, ex)
    tol = {name: FACTOR * (e_rnd[name] + float((r32[name] - rnd[name]).abs().max())) for name in rnd}
    return ex, tol


def check(label, got, ex, tol, quiet=False):
    """Asserts per output tensor max |got - exact| <= tol; prints the error and the bound side by side, both over max |exact|.  Returns {name: error / tol}."""
    assert set(got) == set(tol), (label, sorted(got), sorted(tol))
    err, ratios, failed = errors(got, ex), {}, []
    for name in sorted(got):
        unit = float(ex[name].abs().max()) or 1.0
        finite = bool(torch.isfinite(got[name].double()).all())
        ratios[name] = err[name] / tol[name] if tol[name] > 0 else (0.0 if err[name] == 0 else math.inf)
        if not quiet:
            print(f"{label} {name}: err {err[name] / unit:.3e} bound {tol[name] / unit:.3e} ({ratios[name]:.2f} of bound)" + ("" if finite else " NOT FINITE"))
        if not finite or not err[name] <= tol[name]:
            failed.append(name)
    assert not failed, (label, failed, {n: (err[n], tol[n]) for n in failed})
    return ratios


# ---------------------------------------------------------------- decoders of the kernels' raw bytes (uint8 tensors in, float64 out)
def planes16(raw, fp16):
    """2-byte elements, little endian: IEEE binary16, or bfloat16 = the upper half of a binary32."""
    return raw.contiguous().view(torch.float16 if fp16 else torch.bfloat16).double()


def e4m3(raw, s):
    """One byte per element: sign, 4 exponent bits (bias 7), 3 mantissa bits; exponent 0 is subnormal (m 2^-9); 0x7f / 0xff are NaN.  The image holds x 2^s."""
    b = raw.to(torch.int32)
    sign, e, m = 1.0 - 2.0 * (b >> 7).double(), (b >> 3) & 15, (b & 7).double()
    v = torch.where(e == 0, m * 2.0 ** -9, (1.0 + m / 8.0) * torch.exp2(e.double() - 7.0))
    v = torch.where((b & 0x7F) == 0x7F, torch.full_like(v, math.nan), v)
    return sign * v * 2.0 ** -s


def join_f16f8(raw16, raw_lo8, s):
    """fp16 + lo8 2^-(s + 11)"""
    return planes16(raw16, True) + e4m3(raw_lo8, s + F8_LO)


def e4m3_step(v, s):
    """The spacing of the e4m3 grid of exponent s at value v"""
    _, e = torch.frexp(v.double().abs() * 2.0 ** s)
    return torch.exp2((e - 1).clamp_min(-6).double() - 3) * 2.0 ** -s


def split_lines(raw, M, N):
    """The split-line image of a dense [M, N] activation, N % 64 == 0: [M][N / 64] pairs of 128-byte lines, the 64 elements' fp16, then hi8 x 64 | lo8 x 64.
    Returns the three planes' bytes: fp16 [M, 2 N], hi8 [M, N], lo8 [M, N]."""
    t = raw.reshape(M, N // 64, 256)
    return t[:, :, :128].reshape(M, 2 * N), t[:, :, 128:192].reshape(M, N), t[:, :, 192:].reshape(M, N)
