"""The fp32 head_dim-64 attention family (csrc/decoder_ops.hip: awt_op_attention_small, _backward, the _dropout pair, awt_op_attention_cached) against
float64, output by output: o, lse, delta, dq, dk, dv under the bound of tests/small_attention_reference.py (FACTOR x the distance of a same-precision
restatement from float64, per batch and head; a floor of FACTOR x 2^-23 x max |exact| only where Sk <= 64).  Every case prints its figures first.

The entry points are called through ctypes so that the test owns the layout: every operand and every result is a block inside a NaN-filled buffer whose
pitch is wider than H * 64 (a different padding for q, k, v and o), with two guard rows above and below.  A read outside a block puts a NaN into a
result; a write outside one replaces a NaN bit pattern.  The shapes are the smallest that reach each branch of a 16-query tile, a 64-key chunk and the
round robin of four waves; each case takes milliseconds."""
import functools
import math

import pytest
import torch

from tests import small_attention_reference as sr

pytestmark = pytest.mark.gpu

DEV = "cuda"
G = 2                                                 # guard rows
INVALID = -1
NAN_BITS = torch.tensor(float("nan")).view(torch.int32).item()


def _nan(*shape):
    return torch.full(shape, float("nan"), dtype=torch.float32, device=DEV)


def _all_nan_bits(t):
    return bool((t.contiguous().view(torch.int32) == NAN_BITS).all())


class _Block:
    """A [rows, w] block at (row G, column col) of a NaN-filled [rows + 2 G, ld] buffer (its own, or one shared with other blocks)."""

    def __init__(self, rows, w, ld, col, buf=None, value=None):
        self.rows, self.w, self.ld, self.col = rows, w, ld, col
        self.buf = _nan(rows + 2 * G, ld) if buf is None else buf
        assert self.buf.shape == (rows + 2 * G, ld) and col % 4 == 0 and ld % 4 == 0 and col + w <= ld
        if value is not None:
            self.view().copy_(value)

    def view(self):
        return self.buf[G:G + self.rows, self.col:self.col + self.w]

    def ptr(self):
        return self.buf.data_ptr() + 4 * (G * self.ld + self.col)


class _Vector:
    """[B, H, Lq] fp32 with G guard words on either side."""

    def __init__(self, n):
        self.n, self.buf = n, _nan(n + 2 * G)

    def view(self):
        return self.buf[G:G + self.n]

    def ptr(self):
        return self.buf.data_ptr() + 4 * G


class _Run:
    """One forward + backward of the pair on head-major float32 q, k, v, d_o.  layout: "pitched" (four buffers of their own), "qkv" (q | k | v column
    blocks of one [B L, 3 H 64] matrix, gradients into a matching one), "kv" (k | v as blocks 2 i, 2 i + 1 of a [B Sk, 2 n H 64] matrix, n = 3, i = 1)."""

    def __init__(self, q, k, v, d_o, causal, off, p=0.0, seed=0, layout="pitched", dropout_entry=None):
        self.B, self.H, self.Lq = q.shape[:3]
        self.Sk = k.shape[2]
        self.causal, self.off, self.p, self.seed = int(causal), int(off), float(p), int(seed)
        self.dropout_entry = p > 0 if dropout_entry is None else dropout_entry
        B, H, Lq, Sk, w = self.B, self.H, self.Lq, self.Sk, self.H * 64
        qr, kr, vr, gr = (sr.rows(t).to(DEV) for t in (q, k, v, d_o))
        if layout == "qkv":
            assert Lq == Sk
            src, dst = _nan(B * Lq + 2 * G, 3 * w), _nan(B * Lq + 2 * G, 3 * w)
            self.q, self.k, self.v = (_Block(B * Lq, w, 3 * w, n * w, src, x) for n, x in enumerate((qr, kr, vr)))
            self.dq, self.dk, self.dv = (_Block(B * Lq, w, 3 * w, n * w, dst) for n in range(3))
        else:
            self.q = _Block(B * Lq, w, w + 8, 4, value=qr)
            self.dq = _Block(B * Lq, w, w + 8, 4)
            if layout == "kv":
                ld = 2 * 3 * w
                src, dst = _nan(B * Sk + 2 * G, ld), _nan(B * Sk + 2 * G, ld)
                self.k, self.v = _Block(B * Sk, w, ld, 2 * w, src, kr), _Block(B * Sk, w, ld, 3 * w, src, vr)
                self.dk, self.dv = _Block(B * Sk, w, ld, 2 * w, dst), _Block(B * Sk, w, ld, 3 * w, dst)
            else:
                assert layout == "pitched"
                self.k, self.v = _Block(B * Sk, w, w + 12, 8, value=kr), _Block(B * Sk, w, w + 20, 12, value=vr)
                self.dk, self.dv = _Block(B * Sk, w, w + 12, 8), _Block(B * Sk, w, w + 20, 12)
        self.d_o = _Block(B * Lq, w, w + 16, 4, value=gr)
        self.o = _Block(B * Lq, w, w + 16, 4)
        self.lse, self.delta = _Vector(B * H * Lq), _Vector(B * H * Lq)

    def forward(self):
        from mlx8_ws_audio_transformer_amd import _lib
        L, a = _lib.lib(), self
        head = (_lib.ctx(), a.q.ptr(), a.q.ld, a.k.ptr(), a.k.ld, a.v.ptr(), a.v.ld, a.o.ptr(), a.o.ld, a.lse.ptr(), a.B, a.H, a.Lq, a.Sk, a.causal, a.off)
        if self.dropout_entry:
            rc = L.awt_op_attention_small_dropout(*head, a.p, a.seed, _lib.stream_handle())
        else:
            rc = L.awt_op_attention_small(*head, _lib.stream_handle())
        assert rc == 0, L.awt_last_error()
        torch.cuda.synchronize()
        return self

    def backward(self):
        from mlx8_ws_audio_transformer_amd import _lib
        L, a = _lib.lib(), self
        head = (_lib.ctx(), a.q.ptr(), a.q.ld, a.k.ptr(), a.k.ld, a.v.ptr(), a.v.ld, a.o.ptr(), a.d_o.ptr(), a.o.ld, a.lse.ptr(), a.delta.ptr(),
                a.dq.ptr(), a.dk.ptr(), a.dv.ptr(), a.B, a.H, a.Lq, a.Sk, a.causal, a.off)
        if self.dropout_entry:
            rc = L.awt_op_attention_small_backward_dropout(*head, a.p, a.seed, _lib.stream_handle())
        else:
            rc = L.awt_op_attention_small_backward(*head, _lib.stream_handle())
        assert rc == 0, L.awt_last_error()
        torch.cuda.synchronize()
        return self

    def outputs(self):
        B, H, Lq = self.B, self.H, self.Lq
        hd = lambda blk: sr.heads(blk.view(), B, H).clone()
        return sr.Outputs(hd(self.o), self.lse.view().view(B, H, Lq).clone(), self.delta.view().view(B, H, Lq).clone(), hd(self.dq), hd(self.dk), hd(self.dv))

    def assert_nothing_else_written(self):
        """Every written element is finite; with the written blocks blanked, every word of every result buffer is still the NaN it was filled with."""
        written = (self.o, self.dq, self.dk, self.dv, self.lse, self.delta)
        for x in written:
            assert bool(torch.isfinite(x.view()).all())
        bufs = {}
        for x in written:
            bufs.setdefault(x.buf.data_ptr(), x.buf.clone())
        for x in written:
            c = bufs[x.buf.data_ptr()]
            if isinstance(x, _Vector):
                c[G:G + x.n] = float("nan")
            else:
                c[G:G + x.rows, x.col:x.col + x.w] = float("nan")
        for c in bufs.values():
            assert _all_nan_bits(c), "written outside its block"


def _keep(B, H, Lq, Sk, p, seed=sr.DROPOUT_SEED):
    from mlx8_ws_audio_transformer_amd.autograd_ops import attention_keep_mask
    return attention_keep_mask(seed, B, H, Lq, Sk, p) > 0


@functools.lru_cache(maxsize=None)
def _reference(B, H, Lq, Sk, causal, off, p=0.0):
    """Inputs (CPU) and the two references (on the GPU, float64) of a case: computed once, shared by the tests that use the case, never written to."""
    q, k, v, d_o = sr.inputs(B, H, Lq, Sk)
    keep = _keep(B, H, Lq, Sk, p) if p > 0 else None
    dev = [t.to(DEV) for t in (q, k, v, d_o)]
    return (q, k, v, d_o), sr.exact(*dev, causal, off, keep, p), sr.rounded(*dev, causal, off, keep, p)


def _run_and_check(label, B, H, Lq, Sk, causal, off, p=0.0, layout="pitched"):
    (q, k, v, d_o), ex, rnd = _reference(B, H, Lq, Sk, causal, off, p)
    run = _Run(q, k, v, d_o, causal, off, p, sr.DROPOUT_SEED, layout).forward().backward()
    report = sr.check(label, run.outputs(), rnd, ex, Sk)
    run.assert_nothing_else_written()
    return report


@pytest.mark.parametrize("B,H,Lq,Sk,causal,off", sr.CASES)
def test_pair_against_fp64(B, H, Lq, Sk, causal, off):
    _run_and_check(f"small attention {(B, H, Lq, Sk, causal, off)}", B, H, Lq, Sk, causal, off)


@pytest.mark.parametrize("layout,B,H,Lq,Sk,causal,off", [("qkv", 2, 2, 18, 18, True, 0), ("kv", 2, 2, 5, 70, False, 0)])
def test_fused_layouts_against_fp64(layout, B, H, Lq, Sk, causal, off):
    """The layouts the decoder trains with: the fused projection's [M, 3 d] output read in place with the gradients written into a matching matrix
    (self-attention), and one layer's k | v blocks of the [B Sk, 2 n d] cross-attention projection."""
    _run_and_check(f"small attention {layout} {(B, H, Lq, Sk, causal, off)}", B, H, Lq, Sk, causal, off, layout=layout)


# ------------------------------------------------------------------------------------------------ dropout
@pytest.mark.parametrize("B,H,Lq,Sk,causal,off,p", sr.DROPOUT_CASES)
def test_dropout_pair_against_fp64(B, H, Lq, Sk, causal, off, p):
    _run_and_check(f"small attention dropout {(B, H, Lq, Sk, causal, off, p)}", B, H, Lq, Sk, causal, off, p)


@pytest.mark.parametrize("B,Lq,causal,off,p", [(3, 37, False, 0, 0.25), (2, 20, True, 44, 0.5)])
def test_dropped_probabilities_are_the_masks(B, Lq, causal, off, p):
    """With the identity as values (H = 1, Sk = 64) o is the dropped probability row itself.  A visible probability is exp(s - lse) > 0 (scores of
    standard deviation 3 over 64 keys: never below e^-40), so the kernel's exact zeros among the visible keys are the mask's, one for one."""
    H, Sk = 1, 64
    q, k, _, d_o = sr.inputs(B, H, Lq, Sk)
    v = torch.eye(64).expand(B, H, 64, 64).contiguous()
    P = _Run(q, k, v, d_o, causal, off, p, 77).forward().outputs().o.cpu()
    assert bool(torch.isfinite(P).all())
    vis = sr.visible(Lq, Sk, causal, off).expand(B, H, Lq, Sk)
    keep = _keep(B, H, Lq, Sk, p, seed=77)
    assert torch.equal(P != 0, keep & vis)
    print(f"dropped probabilities {(B, Lq, causal, off, p)}: {int((~keep & vis).sum())} of {int(vis.sum())} visible probabilities dropped")
    assert 0 < int((~keep & vis).sum()) < int(vis.sum())


@pytest.mark.parametrize("B,H,Lq,Sk,causal,off", [(1, 2, 33, 321, False, 0), (2, 2, 12, 12, True, 0)])
def test_drop_p_zero_is_the_plain_pair(B, H, Lq, Sk, causal, off):
    (q, k, v, d_o), _, _ = _reference(B, H, Lq, Sk, causal, off)
    plain = _Run(q, k, v, d_o, causal, off).forward().backward().outputs()
    zero = _Run(q, k, v, d_o, causal, off, 0.0, 12345, dropout_entry=True).forward().backward().outputs()
    for name in sr.NAMES:
        assert torch.equal(getattr(plain, name), getattr(zero, name)), name


# ------------------------------------------------------------------------------------------------ the mask's edge
@pytest.mark.parametrize("mode", ["full", "causal0", "causal_end"])
@pytest.mark.parametrize("Sk", [63, 64, 65, 257])
def test_visible_key_count(Sk, mode):
    """All keys of a (batch, head) equal and all values equal: every visible key has the same score s_i, bit for bit, so every probability of the
    online softmax is exp(0) = 1 and l counts the visible keys.  Then lse_i - s_i = ln(count_i), count_i = i + causal_off + 1 under the mask and Sk
    without, and o_i is the value row.  An off-by-one in the mask or in a tile's last key changes a count, whatever the data: ln(258 / 257) is 3.9e-3,
    the bound below 1e-5.  So that the bound has nothing else to cover, the data sit on grids: q and k are multiples of 1 / 8 below 6 (every product a
    multiple of 1 / 64, every partial sum of 64 of them below 2^12: exact in fp32 in any order, with or without FMA) and the values multiples of 1 / 16
    below 2 (every partial sum of up to 257 equal values exact).  o must equal the value row within FACTOR x 2^-23 of its largest element (it is in
    fact equal), and lse the float64 s_i + ln(count_i) within FACTOR x 2^-23 x max |lse| of the head: the 1-ulp log, its product with ln 2 and the
    final sum."""
    B, H, Lq = 2, 2, 20
    causal, off = {"full": (False, 0), "causal0": (True, 0), "causal_end": (True, Sk - Lq)}[mode]
    grid = lambda x, n, top: torch.round(x.clamp(-top, top) * n) / n
    q, krow = grid(sr.variates("edge.q", (B, H, Lq, 64), 1.7), 8, 5.875), grid(sr.variates("edge.k", (B, H, 1, 64), 1.7), 8, 5.875)
    d_o = sr.variates("edge.d_o", (B, H, Lq, 64))
    vrow = grid(sr.variates("edge.v", (B, H, 1, 64)), 16, 1.9375)
    run = _Run(q, krow.expand(B, H, Sk, 64), vrow.expand(B, H, Sk, 64), d_o, causal, off).forward()
    got = run.outputs()
    assert bool(torch.isfinite(got.o).all()) and bool(torch.isfinite(got.lse).all())
    o_err = (got.o.cpu().double() - vrow.double()).abs().amax((-1, -2))
    o_tol = sr.FACTOR * 2.0 ** -23 * vrow.double().abs().amax((-1, -2))
    count = sr.visible_count(Lq, Sk, causal, off).double()
    want = 0.125 * (q.double() * krow.double()).sum(-1) + torch.log(count)
    lse_err = (got.lse.cpu().double() - want).abs().amax(-1)
    lse_tol = sr.FACTOR * 2.0 ** -23 * want.abs().amax(-1)
    print(f"visible keys Sk {Sk} {mode}: o {float((o_err / o_tol).max()):.2f} of tol, lse {float((lse_err / lse_tol).max()):.2f} of tol "
          f"(counts {int(count.min())}..{int(count.max())})")
    assert bool((o_err <= o_tol).all()) and bool((lse_err <= lse_tol).all())


# ------------------------------------------------------------------------------------------------ rescale and merge
def test_far_apart_maxima_rescale_and_merge():
    """Sk = 600, Lq = 16: rows 0-3 have their score maximum at key 0 (wave 0's first chunk), rows 4-7 at key 100 (wave 1), rows 8-11 at key 300 (wave 0's
    second chunk: its running o and l are rescaled by alpha = e^-60 or so) and rows 12-15 at key 599 (the tail chunk of 24 keys, wave 1's third), each
    about 60 above every other score of the row: the last four dimensions are zero except that a row of group g and that group's key hold 560^1/2 in
    dimension 60 + g, which adds 0.125 x 560 = 70 to that one score (the other 60 dimensions take up to 15 of it back).  In the merge the other three waves' weights exp(m_w - M) are e^-60 or less.  The
    bound is the operator test's.  At scores of 70 one fp32 ulp of a score is 8e-6 of a probability: the backward's P = exp(s - lse) is within the bound
    only if its s is the forward's s to the last bit, which is why all three kernels form it through score4 (before they did, dv was 13 x over)."""
    B, H, Lq, Sk = 1, 2, 16, 600
    q, k, v, d_o = sr.inputs(B, H, Lq, Sk, seed=2)
    q, k = q.clone(), k.clone()
    q[..., 60:], k[..., 60:] = 0.0, 0.0
    for g, key in enumerate((0, 100, 300, 599)):
        q[:, :, 4 * g:4 * g + 4, 60 + g] = math.sqrt(560.0)
        k[:, :, key, 60 + g] = math.sqrt(560.0)
    dev = [t.to(DEV) for t in (q, k, v, d_o)]
    ex, rnd = sr.exact(*dev, False, 0), sr.rounded(*dev, False, 0)
    s = 0.125 * (dev[0].double() @ dev[1].double().transpose(2, 3))
    top2 = s.topk(2, dim=-1)
    gap = top2.values[..., 0] - top2.values[..., 1]
    assert torch.equal(top2.indices[..., 0].cpu(), torch.tensor([0] * 4 + [100] * 4 + [300] * 4 + [599] * 4).expand(B, H, Lq)) and float(gap.min()) > 40
    print(f"far-apart maxima: each row's largest score leads by {float(gap.min()):.1f} to {float(gap.max()):.1f}")
    run = _Run(q, k, v, d_o, False, 0).forward().backward()
    got = run.outputs()
    assert bool(torch.isfinite(got.o).all())
    sr.check("small attention far-apart maxima", got, rnd, ex, Sk)
    run.assert_nothing_else_written()


# ------------------------------------------------------------------------------------------------ invariants
@pytest.mark.parametrize("B,H,Lq,Sk,causal,off", [(1, 2, 33, 321, False, 0), (2, 2, 70, 200, True, 130)])
def test_dv_column_sums_equal_d_o_column_sums(B, H, Lq, Sk, causal, off):
    """sum_j dv[j] = sum_i (sum_j p_ij) d_o[i] = sum_i d_o[i], because every row of P sums to 1.  What separates the two sides in the kernel: p_ij =
    exp(s_ij - lse_i) is formed from the fp32 lse (rounded to 2^-21 absolute for |lse| < 16, which is 2^-21 relative on every p of the row), the rounded
    difference (2^-22 where p matters, |s - lse| < 8), its rounded product with log2 e (2^-21) and a 1-ulp exp2 (2^-23); lse itself carries the same three
    errors of the forward's p and a 1-ulp log: under 2^-19 on a row sum.  Each dv element is then a running fp32 sum over at most 70 rows (70 x 2^-24 <
    2^-17.8 of the terms' magnitudes).  eps = 2^-17 bounds the total per term: each column may differ by eps x sum_i |d_o[i]|.  A row or a key left out
    is an error of order 1."""
    (q, k, v, d_o), _, _ = _reference(B, H, Lq, Sk, causal, off)
    dv = _Run(q, k, v, d_o, causal, off).forward().backward().outputs().dv
    got = dv.double().sum(2).cpu()
    want, mag = d_o.double().sum(2), d_o.double().abs().sum(2)
    worst = float(((got - want).abs() / mag).max())
    print(f"dv column sums {(B, H, Lq, Sk, causal, off)}: worst |difference| / sum |d_o| = {worst:.3e} (eps {2.0 ** -17:.3e})")
    assert worst <= 2.0 ** -17


@pytest.mark.parametrize("B,H,Lq,Sk,causal,off,p", [(1, 2, 33, 321, False, 0, 0.0), (1, 2, 20, 300, False, 0, 0.1)])
def test_two_runs_give_the_same_bits(B, H, Lq, Sk, causal, off, p):
    (q, k, v, d_o), _, _ = _reference(B, H, Lq, Sk, causal, off, p)
    one = _Run(q, k, v, d_o, causal, off, p, sr.DROPOUT_SEED).forward().backward().outputs()
    two = _Run(q, k, v, d_o, causal, off, p, sr.DROPOUT_SEED).forward().backward().outputs()
    for name in sr.NAMES:
        a, b = getattr(one, name), getattr(two, name)
        assert bool(torch.isfinite(a).all()) and torch.equal(a.view(torch.int32), b.view(torch.int32)), name


# ------------------------------------------------------------------------------------------------ the decode cache
@pytest.mark.parametrize("rows,H,Lq,T,Tmax", [(2, 2, 1, 65, 96), (1, 2, 17, 200, 256)])
def test_cached_attention_guards_and_pitches(rows, H, Lq, T, Tmax):
    """awt_op_attention_cached over a [rows, Tmax, 2 H 64 + 8] cache: keys at column 4, values at column H 64 + 4, NaN in the padding and at every
    position >= T; q and o pitched with guard rows.  o is finite, within the operator test's bound of float64, written nowhere else, and has the bits of
    awt_op_attention_small(causal, causal_off = T - Lq) on a packed copy."""
    from mlx8_ws_audio_transformer_amd import _lib
    (q, k, v, d_o), ex, rnd = _reference(rows, H, Lq, T, True, T - Lq)
    w = H * 64
    ldkv = 2 * w + 8
    cache = _nan(rows, Tmax, ldkv)
    cache[:, :T, 4:4 + w] = sr.rows(k).view(rows, T, w).to(DEV)
    cache[:, :T, w + 4:2 * w + 4] = sr.rows(v).view(rows, T, w).to(DEV)
    qb, ob = _Block(rows * Lq, w, w + 8, 4, value=sr.rows(q).to(DEV)), _Block(rows * Lq, w, w + 16, 4)
    L = _lib.lib()
    rc = L.awt_op_attention_cached(_lib.ctx(), qb.ptr(), qb.ld, cache.data_ptr() + 4 * 4, cache.data_ptr() + 4 * (w + 4), ldkv, Tmax * ldkv, ob.ptr(), ob.ld,
                                   rows, H, Lq, T, _lib.stream_handle())
    assert rc == 0, L.awt_last_error()
    torch.cuda.synchronize()
    o = sr.heads(ob.view(), rows, H).clone()
    assert bool(torch.isfinite(o).all())
    sr.check(f"cached attention {(rows, H, Lq, T, Tmax)}", sr.Outputs(o, None, None, None, None, None), rnd, ex, T, names=("o",))
    packed = _Run(q, k, v, d_o, True, T - Lq).forward().outputs().o
    assert torch.equal(o.view(torch.int32), packed.view(torch.int32))
    rest = ob.buf.clone()
    rest[G:G + ob.rows, ob.col:ob.col + ob.w] = float("nan")
    assert _all_nan_bits(rest), "written outside its block"


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals_launch_nothing():
    """Every bad argument is answered with AWT_ERR_INVALID before any launch: the NaN-filled results are untouched.  The calls go through one valid
    argument list with one argument replaced, and the valid list itself is accepted last."""
    from mlx8_ws_audio_transformer_amd import _lib
    B, H, Lq, Sk = 1, 2, 3, 5
    q, k, v, d_o = sr.inputs(B, H, Lq, Sk)
    run = _Run(q, k, v, d_o, True, 2)
    L, w, st = _lib.lib(), H * 64, _lib.stream_handle()
    run.o.view().fill_(0.25)                                  # the backward's inputs: finite, so that the accepted call below is an ordinary one
    run.lse.view().fill_(1.0)
    results = (run.dq, run.dk, run.dv, run.delta)

    def fwd(**kw):
        a = dict(q=run.q.ptr(), ldq=run.q.ld, k=run.k.ptr(), ldk=run.k.ld, v=run.v.ptr(), ldv=run.v.ld, o=run.dq.ptr(), ldo=run.dq.ld, lse=run.delta.ptr(),
                 B=B, H=H, Lq=Lq, Sk=Sk, causal=1, off=2, p=0.0, seed=1)            # writes into dq / delta: the buffers that are still all NaN
        a.update(kw)
        return L.awt_op_attention_small_dropout(_lib.ctx(), a["q"], a["ldq"], a["k"], a["ldk"], a["v"], a["ldv"], a["o"], a["ldo"], a["lse"], a["B"], a["H"],
                                                a["Lq"], a["Sk"], a["causal"], a["off"], a["p"], a["seed"], st)

    def bwd(**kw):
        a = dict(q=run.q.ptr(), ldq=run.q.ld, k=run.k.ptr(), ldk=run.k.ld, v=run.v.ptr(), ldv=run.v.ld, o=run.o.ptr(), dout=run.d_o.ptr(), ldo=run.o.ld,
                 lse=run.lse.ptr(), delta=run.delta.ptr(), dq=run.dq.ptr(), dk=run.dk.ptr(), dv=run.dv.ptr(), B=B, H=H, Lq=Lq, Sk=Sk, causal=1, off=2, p=0.0, seed=1)
        a.update(kw)
        return L.awt_op_attention_small_backward_dropout(_lib.ctx(), a["q"], a["ldq"], a["k"], a["ldk"], a["v"], a["ldv"], a["o"], a["dout"], a["ldo"], a["lse"],
                                                         a["delta"], a["dq"], a["dk"], a["dv"], a["B"], a["H"], a["Lq"], a["Sk"], a["causal"], a["off"], a["p"],
                                                         a["seed"], st)

    def cached(**kw):
        a = dict(q=run.q.ptr(), ldq=run.q.ld, k=run.k.ptr(), v=run.v.ptr(), ldkv=run.k.ld, stride=Sk * run.k.ld, o=run.dq.ptr(), ldo=run.dq.ld, Lq=Lq, T=Sk)
        a.update(kw)
        return L.awt_op_attention_cached(_lib.ctx(), a["q"], a["ldq"], a["k"], a["v"], a["ldkv"], a["stride"], a["o"], a["ldo"], B, H, a["Lq"], a["T"], st)

    def refused(call, needle, **kw):
        assert call(**kw) == INVALID, (call.__name__, kw)
        msg = L.awt_last_error().decode()
        assert needle in msg, (call.__name__, kw, msg)

    for call in (fwd, bwd):
        refused(call, "null", q=None)
        refused(call, "strides", ldq=w - 4)                   # below H * 64
        refused(call, "strides", ldk=run.k.ld + 2)            # not a multiple of 4
        refused(call, "strides", ldv=w - 4)
        refused(call, "strides", ldo=run.o.ld + 1)
        refused(call, "dropout", p=1.0)
        refused(call, "dropout", p=-0.125)
        refused(call, "too many", B=1 << 15, H=1 << 8, Lq=1 << 8, ldq=1 << 14, ldk=1 << 14, ldv=1 << 14, ldo=1 << 14)      # B H Lq = 2^31
        refused(call, "causal_off", off=-1)
        refused(call, "aligned", q=run.q.ptr() + 4)
        refused(call, "aligned", k=run.k.ptr() + 8)
        refused(call, "aligned", v=run.v.ptr() + 4)
    refused(fwd, "null", o=None)
    refused(fwd, "aligned", o=run.dq.ptr() + 4)
    refused(bwd, "null", dq=None)
    refused(bwd, "null", delta=None)
    for name in ("o", "dout", "dq", "dk", "dv"):
        refused(bwd, "aligned", **{name: getattr(run, {"dout": "d_o"}.get(name, name)).ptr() + 4})
    refused(cached, "null", k=None)
    refused(cached, "T >= Lq", Lq=Sk + 1)
    refused(cached, "batch stride", stride=Sk * run.k.ld - 4)
    refused(cached, "aligned", v=run.v.ptr() + 4)
    torch.cuda.synchronize()
    for x in results:
        assert _all_nan_bits(x.buf), "a refused call wrote"
    # the list itself is valid, and a negative offset without the mask is not refused (causal_off is not read then)
    assert bwd() == 0 and bwd(causal=0, off=-1) == 0, L.awt_last_error()
    torch.cuda.synchronize()
    assert all(bool(torch.isfinite(x.view()).all()) for x in results)
