"""awt_linear_decode (csrc/gemv.hip, `PackedLinear.forward_decode`): the weight-streaming product of incremental decoding, 1 <= M <= 8 rows, against float64.

Inputs are tests/gemm_reference.py's (`make_inputs`), the tolerance is its `bound(Problem(x, w, bias), epi, terms)` for the epilogues "f32" and "f32_resid" --
the operand roundings of the kernel are the GEMM's, which that file restates -- checked through its `check`: no tolerance of this file's own.  Shapes (N, K):
(200, 64) pads N to 256 and has fewer k-steps than waves; (128, 192) has 6 k-steps, no multiple of the wave count; (128, 3072) is one GEMM column tile of
N and the model's longest K; (1024, 2048) and (384, 1024) are the model's other K; (32900, 192) is past 2048 n-tiles, where a workgroup owns four n-tiles
(the lm_head's form).  Every figure is printed before it is asserted."""
import functools

import pytest
import torch

from tests import gemm_reference as gr

pytestmark = pytest.mark.gpu

SHAPES = [(200, 64), (128, 192), (128, 3072), (1024, 2048), (384, 1024), (32900, 192)]
TERMS = {"bf16": 1, "bf16x3": 3}
TAIL = 8                                                                   # NaN rows below the live ones, in x and in y


@functools.lru_cache(maxsize=None)
def _inputs(N, K):
    """x [8, K], w [N, K], bias [N], resid [8, N] on the CPU (seeded)"""
    x, w, bias = gr.make_inputs(8, N, K, seed=N + K)
    resid = torch.randn((8, N), generator=torch.Generator().manual_seed(N + K + 1))
    return x, w, bias, resid


@functools.lru_cache(maxsize=None)
def _packed(N, K, prec, with_bias):
    from mlx8_ws_audio_transformer_amd.native_decoder import PackedLinear
    _, w, bias, _ = _inputs(N, K)
    return PackedLinear(w.cuda(), bias.cuda() if with_bias else None, prec, backward=False)


def _decode(pl, x, M, resid=None):
    """forward_decode on the top M rows of NaN-tailed buffers; resid (CPU [M, N]) aliases y, its padded columns set to 3.  Returns (y [M, Np], the tail of y)."""
    xbuf = torch.full((M + TAIL, pl.K), float("nan"), device="cuda")
    xbuf[:M] = x[:M].cuda()
    ybuf = torch.full((M + TAIL, pl.Np), float("nan"), device="cuda")
    if resid is not None:
        ybuf[:M] = 3.0
        ybuf[:M, :pl.N] = resid[:M].cuda()
    y = pl.forward_decode(xbuf[:M], resid=None if resid is None else ybuf[:M], out=ybuf[:M])
    assert y.data_ptr() == ybuf.data_ptr()
    return ybuf[:M].clone(), ybuf[M:].clone()


@pytest.mark.parametrize("prec", ["bf16", "bf16x3"])
@pytest.mark.parametrize("M", [1, 3, 8])
@pytest.mark.parametrize("N,K", SHAPES)
def test_against_float64(N, K, M, prec):
    x, w, bias, resid = _inputs(N, K)
    for with_bias in (True, False):
        pl, p = _packed(N, K, prec, with_bias), gr.Problem(x[:M], w, bias if with_bias else None)
        for epi in ("f32", "f32_resid"):
            side = {"resid": resid[:M]} if epi == "f32_resid" else {}
            ex, tol = gr.bound(p, epi, TERMS[prec], **side)
            y, tail = _decode(pl, x, M, resid[:M] if side else None)
            assert bool(torch.isnan(tail).all()), "rows below M of y were written"
            assert bool(torch.isfinite(y).all()), "a NaN row of x was read"
            gr.check(f"decode N{N} K{K} M{M} {prec} bias={with_bias} {epi}", {"y": y[:, :N]}, ex, tol)
            pad = y[:, N:]
            assert bool((pad == (3.0 if side else 0.0)).all()), "columns N .. Np - 1 must come out as 0 + resid"


@pytest.mark.parametrize("prec", ["bf16", "bf16x3"])
@pytest.mark.parametrize("N,K", SHAPES)
def test_rows_do_not_depend_on_the_batch_and_calls_repeat(N, K, prec):
    x, _, _, resid = _inputs(N, K)
    pl = _packed(N, K, prec, True)
    y8, _ = _decode(pl, x, 8, resid)
    again, _ = _decode(pl, x, 8, resid)
    assert torch.equal(y8, again)                                          # bit-reproducible
    for m in range(8):
        y1, _ = _decode(pl, x[m:m + 1], 1, resid[m:m + 1])
        assert torch.equal(y8[m:m + 1], y1), f"row {m} of the M = 8 call differs from the M = 1 call on it"


@pytest.mark.parametrize("prec", ["bf16", "bf16x3"])
@pytest.mark.parametrize("N,K", SHAPES)
def test_agrees_with_the_gemm(N, K, prec):
    """Against `PackedLinear.forward` at the same M: both are within the bound of float64, so they differ by at most the sum of the two (equal) bounds."""
    x, w, bias, _ = _inputs(N, K)
    pl = _packed(N, K, prec, True)
    for M in (1, 3, 8):
        _, tol = gr.bound(gr.Problem(x[:M], w, bias), "f32", TERMS[prec])
        xg = x[:M].cuda()
        diff = float((pl.forward_decode(xg).double() - pl.forward(xg).double()).abs().max())
        print(f"decode vs GEMM N{N} K{K} M{M} {prec}: max-abs {diff:.3e} (sum of the bounds {2 * tol['y']:.3e})")
        assert diff <= 2 * tol["y"]


@pytest.mark.parametrize("prec", ["bf16", "bf16x3"])
def test_after_update_equals_a_fresh_handle(prec):
    from mlx8_ws_audio_transformer_amd.native_decoder import PackedLinear
    x, w0, b0, _ = _inputs(200, 64)
    _, w1, b1 = gr.make_inputs(8, 200, 64, seed=99)
    h, fresh = PackedLinear(w0.cuda(), b0.cuda(), prec), PackedLinear(w1.cuda(), b1.cuda(), prec)
    h.update(w1.cuda(), b1.cuda())
    assert torch.equal(h.forward_decode(x.cuda()), fresh.forward_decode(x.cuda()))
    assert not torch.equal(fresh.forward_decode(x.cuda()), PackedLinear(w0.cuda(), b0.cuda(), prec).forward_decode(x.cuda()))


def test_refusals():
    from mlx8_ws_audio_transformer_amd import _lib
    pl = _packed(200, 64, "bf16x3", True)
    x, y = torch.zeros((9, 64), device="cuda"), torch.zeros((9, pl.Np), device="cuda")
    for M in (0, 9):
        with pytest.raises(_lib.AwtError, match=r"M must be in \[1, 8\]"):
            _lib.check(_lib.lib().awt_linear_decode(_lib.ctx(), pl.handle, _lib.ptr(x), None, _lib.ptr(y), M, _lib.stream_handle()))
    with pytest.raises(_lib.AwtError, match=r"M must be in \[1, 8\]"):
        pl.forward_decode(x)
    assert bool((y == 0).all())
