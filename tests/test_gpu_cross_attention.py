"""The head_dim-128 cross-attention operator pair (awt_op_cross_attention / _backward, csrc/cross_attention.hip) against float64, output by output.

The bound is tests/cross_attention_reference.py's: per output (o, lse, dq, dk, dv) and per (batch, head), max |kernel - exact| <= 4 x max |rounded - exact|,
`rounded` being the float64 restatement of the kernels' own roundings.  It is computed from the reference alone; every case prints its figures.

Inputs: q and k with standard deviation 1.7, so the scores 128^-1/2 q.k have a standard deviation near 2.9 and a row's softmax is far from uniform (a
near-uniform softmax hides a wrong key); v and d_o standard normal.

Shapes (the kernels' tiles: 32 lane-resident rows per wave and 128 queries per workgroup in the forward and dq launches, 64 keys per streamed tile; 64 keys
per workgroup and 32 queries per streamed tile in the dk / dv launch): the six the operator was specified with, plus lengths on either side of 128 queries, of 64 keys and of 32 queries."""
import functools

import pytest
import torch

from tests import cross_attention_reference as xr

pytestmark = pytest.mark.gpu

ATT_TOL_BF16X3 = 1e-4      # tests/test_gpu_ops.py ATT_TOL["bf16x3"]: forward max-abs for N(0, 1) values

# (B, H, Lq, Sk, pitched)
CASES = [
    (2, 2, 1, 1500, False),      # generate's first step
    (2, 2, 17, 70, False),       # tails on both axes
    (2, 2, 33, 64, False),       # exact key tile
    (2, 2, 130, 1500, False),    # more than one query tile per workgroup and a second workgroup, at the real key length
    (2, 2, 64, 1, False),        # a single key
    (3, 1, 40, 129, True),       # pitches wider than H * 128: q inside a wider matrix, k and v inside a [B * Sk, 2 * H * 128] buffer
    (1, 2, 128, 65, False),      # exactly one workgroup of queries; one key past the tile and past the dk / dv workgroup
    (1, 2, 129, 63, False),      # one query past it; one key short of the tile
    (1, 1, 31, 128, False),      # one query short of the dk / dv launch's query tile; two full key tiles
]


def _randn(shape, seed, std=1.0):
    return (torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * std).cuda()


@functools.lru_cache(maxsize=None)
def _inputs(B, H, Lq, Sk):
    q, k = _randn((B, H, Lq, 128), 1, 1.7), _randn((B, H, Sk, 128), 2, 1.7)
    v, d_o = _randn((B, H, Sk, 128), 3), _randn((B, H, Lq, 128), 4)
    return q, k, v, d_o, xr.exact(q, k, v, d_o)


class _Layout:
    """The operator's view of head-major tensors.  pitched: q, o, d_o, dq at column 32 of [rows, H * 128 + 64] matrices, k | v and dk | dv in
    [B * Sk, 2 * H * 128] buffers; else dense matrices of their own.  Every output buffer has 3 guard rows above and below and is pre-filled with NaN."""
    GUARD = 3

    def __init__(self, q, k, v, d_o, pitched):
        self.B, self.H, self.Lq = q.shape[:3]
        self.Sk = k.shape[2]
        w = self.H * 128
        self.ldq = w + 64 if pitched else w
        self.qcol = 32 if pitched else 0
        self.ldk = 2 * w if pitched else w
        self.q, self.d_o = self._place(xr.rows(q), self.ldq, self.qcol), self._place(xr.rows(d_o), self.ldq, self.qcol)
        if pitched:
            kv = torch.cat([xr.rows(k), xr.rows(v)], dim=1).contiguous()
            self.k, self.v = (kv, 0), (kv, w)
        else:
            self.k, self.v = (xr.rows(k).contiguous(), 0), (xr.rows(v).contiguous(), 0)
        self.pitched = pitched

    @staticmethod
    def _place(x, ld, col):
        buf = torch.zeros((x.shape[0], ld), dtype=torch.float32, device=x.device)
        buf[:, col:col + x.shape[1]] = x
        return (buf, col)

    def _nan(self, rows_, ld):
        return torch.full((rows_ + 2 * self.GUARD, ld), float("nan"), dtype=torch.float32, device="cuda")

    def forward(self, precision):
        from mlx8_ws_audio_transformer_amd import ops
        G, w = self.GUARD, self.H * 128
        self.o_buf = self._nan(self.B * self.Lq, self.ldq)
        self.lse_buf = torch.full((self.B * self.H * self.Lq + 2 * G,), float("nan"), dtype=torch.float32, device="cuda")
        lse = self.lse_buf[G:-G].view(self.B, self.H, self.Lq)
        ops.cross_attention(self.q, self.ldq, self.k, self.ldk, self.v, self.ldk, self.B, self.H, self.Lq, self.Sk, precision,
                            o=(self.o_buf, G * self.ldq + self.qcol), ldo=self.ldq, lse=lse)
        self.lse = lse
        return self.o_buf[G:-G, self.qcol:self.qcol + w], lse

    def backward(self, precision):
        from mlx8_ws_audio_transformer_amd import ops
        G, w = self.GUARD, self.H * 128
        self.dq_buf = self._nan(self.B * self.Lq, self.ldq)
        self.dkv_buf = self._nan(self.B * self.Sk, self.ldk) if self.pitched else None
        self.dk_buf = self.dkv_buf if self.pitched else self._nan(self.B * self.Sk, w)
        self.dv_buf = self.dkv_buf if self.pitched else self._nan(self.B * self.Sk, w)
        ops.cross_attention_backward(self.q, self.ldq, self.k, self.ldk, self.v, self.ldk, (self.o_buf, G * self.ldq + self.qcol), self.d_o, self.ldq, self.lse,
                                     (self.dq_buf, G * self.ldq + self.qcol), (self.dk_buf, G * self.ldk), (self.dv_buf, G * self.ldk + (w if self.pitched else 0)),
                                     self.B, self.H, self.Lq, self.Sk, precision)
        dq = self.dq_buf[G:-G, self.qcol:self.qcol + w]
        dk = self.dk_buf[G:-G, :w]
        dv = self.dv_buf[G:-G, w:2 * w] if self.pitched else self.dv_buf[G:-G]
        return dq, dk, dv

    def outputs(self, o, lse, dq, dk, dv):
        return xr.Outputs(xr.heads(o, self.B, self.H), lse, xr.heads(dq, self.B, self.H), xr.heads(dk, self.B, self.H), xr.heads(dv, self.B, self.H))

    def guards_intact(self):
        """Everything outside the written blocks still holds the NaN it was filled with, bit for bit."""
        G, w, nan_bits = self.GUARD, self.H * 128, torch.tensor(float("nan")).view(torch.int32).item()

        def outside(buf, c0, c1):
            bits = buf.view(torch.int32).clone()
            bits[G:-G, c0:c1] = nan_bits
            return bool((bits == nan_bits).all())

        ok = outside(self.o_buf, self.qcol, self.qcol + w) and outside(self.dq_buf, self.qcol, self.qcol + w)
        ok = ok and bool((self.lse_buf[:G].view(torch.int32) == nan_bits).all()) and bool((self.lse_buf[-G:].view(torch.int32) == nan_bits).all())
        if self.pitched:
            return ok and outside(self.dkv_buf, 0, 2 * w)
        return ok and outside(self.dk_buf, 0, w) and outside(self.dv_buf, 0, w)


@pytest.mark.parametrize("precision", ["bf16x3", "bf16"])
@pytest.mark.parametrize("B,H,Lq,Sk,pitched", CASES)
def test_forward_and_backward_within_the_rounding_model(B, H, Lq, Sk, pitched, precision):
    """All five outputs inside 4 x the float64 restatement's own distance from exact; nothing unwritten inside the outputs (they start as NaN), nothing
    written beyond them (guard rows and, in the pitched case, guard columns stay bit-intact); the bf16x3 forward inside the suite's 1e-4."""
    q, k, v, d_o, ex = _inputs(B, H, Lq, Sk)
    lay = _Layout(q, k, v, d_o, pitched)
    o, lse = lay.forward(precision)
    dq, dk, dv = lay.backward(precision)
    got = lay.outputs(o, lse, dq, dk, dv)
    for name in xr.NAMES:
        assert not bool(torch.isnan(getattr(got, name)).any()), f"{name}: an element was left unwritten"
    assert lay.guards_intact()
    rnd = xr.rounded(q, k, v, d_o, 3 if precision == "bf16x3" else 1)
    xr.check(f"B{B} H{H} Lq{Lq} Sk{Sk} {precision}", got, rnd, ex)
    if precision == "bf16x3":
        err = float((got.o.double() - ex.o).abs().max())
        print(f"forward max-abs {err:.3e} (tol {ATT_TOL_BF16X3})")
        assert err <= ATT_TOL_BF16X3


@pytest.mark.parametrize("precision", ["bf16x3", "bf16"])
def test_two_runs_are_bit_identical(precision):
    q, k, v, d_o, _ = _inputs(2, 2, 130, 1500)
    runs = []
    for _ in range(2):
        lay = _Layout(q, k, v, d_o, False)
        o, lse = lay.forward(precision)
        runs.append([t.clone() for t in (o, lse, *lay.backward(precision))])
    for a, b in zip(*runs):
        assert torch.equal(a, b)


def test_online_softmax_rescale_branch():
    """One key per late tile dominates one query's row, so the running maximum jumps tile after tile (tests/test_gpu_ops.py
    test_attention_online_softmax_rescale_branch: split precision, bound 3e-4)."""
    from mlx8_ws_audio_transformer_amd import ops
    B, H, Lq, Sk = 1, 1, 40, 448
    q, k, v = _randn((B, H, Lq, 128), 10, 0.2), _randn((B, H, Sk, 128), 11), _randn((B, H, Sk, 128), 12)
    for t, key in enumerate([70, 150, 260, 390]):
        k[0, 0, key] = q[0, 0, 5] * (40.0 + 30 * t)
    o, _ = ops.cross_attention((xr.rows(q).contiguous(), 0), 128, (xr.rows(k).contiguous(), 0), 128, (xr.rows(v).contiguous(), 0), 128, B, H, Lq, Sk, "bf16x3")
    s = q.double() @ k.double().transpose(2, 3) * 128 ** -0.5
    ref = xr.rows(torch.softmax(s, dim=-1) @ v.double())
    err = float((o.double() - ref).abs().max())
    print("rescale branch: max-abs", err, "largest logit", float(s.max()))
    assert float(s.max()) > 30                   # the row's maximum really climbs by tens of units, tile after tile
    assert err < 3e-4, err


@pytest.mark.parametrize("precision", ["bf16x3", "bf16"])
def test_equal_keys_return_the_value_row(precision):
    """All keys of a head equal: every score of a row is the same number, so every probability is exp2(0) = 1 exactly, and with all values of the head
    equal (and bf16-representable, so that the split loses nothing) the output accumulator is Sk v exactly and o = Sk v * fp32(1 / Sk): two fp32 roundings,
    |o - v| <= 2^-22 |v|.  Sk = 150 spans three key tiles with a masked tail."""
    from mlx8_ws_audio_transformer_amd import ops
    B, H, Lq, Sk = 2, 2, 37, 150
    q = _randn((B, H, Lq, 128), 20, 1.7)
    k = _randn((B, H, 1, 128), 21, 1.7).expand(B, H, Sk, 128).contiguous()
    v1 = _randn((B, H, 1, 128), 22).bfloat16().float()
    v = v1.expand(B, H, Sk, 128).contiguous()
    o, _ = ops.cross_attention((xr.rows(q).contiguous(), 0), H * 128, (xr.rows(k).contiguous(), 0), H * 128, (xr.rows(v).contiguous(), 0), H * 128,
                               B, H, Lq, Sk, precision)
    want = v1.expand(B, H, Lq, 128)
    err = (xr.heads(o, B, H).double() - want.double()).abs()
    assert bool((err <= 2.0 ** -22 * want.double().abs()).all()), float(err.max())


@pytest.mark.parametrize("precision,eps", [("bf16x3", 2.0 ** -15), ("bf16", 2.0 ** -7)])
def test_dv_column_sums_equal_d_o_column_sums(precision, eps):
    """sum_j dv[j] = sum_i (sum_j p_ij) d_o[i] = sum_i d_o[i], because every row of P sums to 1.  What separates the two sides in the kernel: P and d_o
    enter the product as split operands (each short by at most 2^-17 relative with three terms -- the residual of the lo plane and the lo x lo product that
    is never formed -- or 2^-9 with one), P = exp2(s - lse2) carries the fp32 rounding of its exponent (logits and lse below 32: 2^-19 absolute, ~1.3e-6
    relative) and the fp32 sums.  eps bounds their total per term: 2^-15 for bf16x3 (2 x 2^-17 + 1.3e-6 + the sums, doubled), 2^-7 for bf16 (2 x 2^-9,
    doubled); each column may differ by eps x sum_i |d_o[i]|."""
    q, k, v, d_o, _ = _inputs(2, 2, 130, 1500)
    lay = _Layout(q, k, v, d_o, False)
    lay.forward(precision)
    _, _, dv = lay.backward(precision)
    got = xr.heads(dv, 2, 2).double().sum(2)
    want, mag = d_o.double().sum(2), d_o.double().abs().sum(2)
    assert bool(((got - want).abs() <= eps * mag).all()), float(((got - want).abs() / mag).max())


def test_offsets_past_2_31_elements():
    """Keys and values in a [B * Sk, 2048] buffer of 2.16e9 elements (8.6 GB; the gradient buffer as much again): the rows of the last batches lie past
    element 2^31, where a 32-bit offset wraps.  One head, one query per batch, so the work stays small; the first batch and the last two are checked in full
    against float64 under the operator tests' bound."""
    from mlx8_ws_audio_transformer_amd import ops
    B, H, Lq, Sk, ld = 704, 1, 1, 1500, 2048
    assert (B - 2) * Sk * ld > 2 ** 31
    gen = torch.Generator("cuda").manual_seed(5)
    kv = torch.randn((B * Sk, ld), device="cuda", generator=gen)
    kv[:, :128] *= 1.7
    q, d_o = 1.7 * torch.randn((B, 128), device="cuda", generator=gen), torch.randn((B, 128), device="cuda", generator=gen)
    o, lse = ops.cross_attention((q, 0), 128, (kv, 0), ld, (kv, 1024), ld, B, H, Lq, Sk, "bf16x3")
    dq, dkv = torch.empty_like(q), torch.empty_like(kv)
    ops.cross_attention_backward((q, 0), 128, (kv, 0), ld, (kv, 1024), ld, (o, 0), (d_o, 0), 128, lse, (dq, 0), (dkv, 0), (dkv, 1024), B, H, Lq, Sk, "bf16x3")
    for b in (0, B - 2, B - 1):
        rows_ = slice(b * Sk, (b + 1) * Sk)
        qb, gb = q[b].view(1, 1, 1, 128), d_o[b].view(1, 1, 1, 128)
        kb, vb = kv[rows_, :128].reshape(1, 1, Sk, 128), kv[rows_, 1024:1152].reshape(1, 1, Sk, 128)
        got = xr.Outputs(o[b].view(1, 1, 1, 128), lse[b].view(1, 1, 1), dq[b].view(1, 1, 1, 128), dkv[rows_, :128].reshape(1, 1, Sk, 128),
                         dkv[rows_, 1024:1152].reshape(1, 1, Sk, 128))
        xr.check(f"batch {b} of {B}", got, xr.rounded(qb, kb, vb, gb, 3), xr.exact(qb, kb, vb, gb))


def test_refusals():
    from mlx8_ws_audio_transformer_amd import _lib, ops
    B, H, Lq, Sk = 1, 2, 8, 16
    q, k, v = _randn((B * Lq, H * 128), 1), _randn((B * Sk, H * 128), 2), _randn((B * Sk, H * 128), 3)
    o, lse = ops.cross_attention((q, 0), 256, (k, 0), 256, (v, 0), 256, B, H, Lq, Sk)
    with pytest.raises(_lib.AwtError, match="H \\* 128"):                      # the pitch holds one head only
        ops.cross_attention((q, 0), 128, (k, 0), 256, (v, 0), 256, B, H, Lq, Sk)
    with pytest.raises(_lib.AwtError, match="multiples of 4"):
        ops.cross_attention((q, 0), 256, (k, 0), 258, (v, 0), 256, B, H, Lq, Sk)
    with pytest.raises(_lib.AwtError, match="terms"):
        ops.cross_attention((q, 0), 256, (k, 0), 256, (v, 0), 256, B, H, Lq, Sk, precision=2)
    d = torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)
    args = ((q, 0), 256, (k, 0), 256, (v, 0), 256, (o, 0), (q, 0), 256, lse, (d[0], 0), (d[1], 0), (d[2], 0), B, H, Lq, Sk)
    with pytest.raises(_lib.AwtError, match="terms"):
        ops.cross_attention_backward(*args, precision=2)
    need = ops.cross_attention_workspace_bytes(B, H, Lq, Sk, backward=True)
    assert need >= B * H * Lq * 4
    short = torch.empty(need + 256, dtype=torch.uint8, device="cuda")[: need - 1]
    with pytest.raises(_lib.AwtError, match="workspace too small"):
        ops.cross_attention_backward(*args, workspace=short)
    with pytest.raises(_lib.AwtError, match="null"):
        L = _lib.lib()
        _lib.check(L.awt_op_cross_attention(_lib.ctx(q.device), None, 256, k.data_ptr(), 256, v.data_ptr(), 256, o.data_ptr(), 256, None, B, H, Lq, Sk, 3,
                                            None, 0, _lib.stream_handle()))
    ops.cross_attention_backward(*args)                                        # and the accepted call still runs
    assert bool(torch.isfinite(d[0]).all())
