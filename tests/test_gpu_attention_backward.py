"""GPU: the attention of the encoder's training pass -- the training form of csrc/attention.hip (row-major o planes, saved log-sum-exp) and both
launches of csrc/attention_bwd.hip -- through awt_op_attention_backward, against float64, output by output.

The bound is tests/attention_reference.py's: per output and per (batch, head), max |kernel - exact| <= 4 x max |rounded - exact|, where `rounded` is
the float64 restatement with the kernels' operand roundings; both sides are normalised by that head's max |exact|, and each test prints the two
figures side by side.  It is computed from the reference alone.  tests/test_attention_reference_host.py shows what it tells apart: a lost lo plane
is >= 21 x the bound.  o keeps ATT_TOL of tests/test_gpu_ops.py as well.

Inputs: seeded N(0, 1), q x 0.35 as in test_gpu_ops.test_attention.  H = 3 makes d = 192: head-major, row-major and 3 d strides all differ."""
import functools

import pytest
import torch

from tests import attention_reference as ar
from tests.test_gpu_ops import ATT_TOL, _rand
from tests.util import GUARD, guarded as _guarded, tuning

pytestmark = pytest.mark.gpu

TERMS = {"bf16x3": 3, "bf16": 1}
INVALID, ERR_WORKSPACE = -1, -3


@functools.lru_cache(maxsize=None)
def inputs(B, H, S):
    return _rand((B, H, S, 64), 7, 0.35), _rand((B, H, S, 64), 8), _rand((B, H, S, 64), 9), _rand((B, S, H * 64), 10)


@functools.lru_cache(maxsize=None)
def exact(B, H, S):
    x = inputs(B, H, S)
    ex = ar.exact(*x)
    return ex, ar.cancellation_floor(*x, ex)


@functools.lru_cache(maxsize=None)
def rounded(B, H, S, terms, grad_terms):
    return ar.rounded(*inputs(B, H, S), terms=terms, grad_terms=grad_terms)


def run(x, precision="bf16x3", grad_precision=None, qscale=1.0):
    from mlx8_ws_audio_transformer_amd import ops
    return ar.Outputs(*ops.attention_backward(*x, precision, grad_precision, qscale))


def planes(x, precision="bf16x3", grad_precision=None, qscale=1.0, out=None):
    from mlx8_ws_audio_transformer_amd import ops
    return ops.attention_backward_planes(*x, precision, grad_precision, qscale, out)


def joined(p, B, H, S):
    from mlx8_ws_audio_transformer_amd import ops
    return ar.Outputs(*ops.attention_backward_join(p, B, H, S))


def same_bits(a, b):
    return all((s is None and t is None) or torch.equal(s, t) for s, t in zip(a, b))


def within_bound(label, got, B, H, S, precision, grad_terms=None):
    ex, floor = exact(B, H, S)
    report = ar.check(label, got, rounded(B, H, S, TERMS[precision], grad_terms or TERMS[precision]), ex, floor)
    o_err = (got.o - ex.o).abs().max().item()
    print(f"{label} o: max-abs {o_err:.3e} (ATT_TOL {ATT_TOL[precision]:g})")
    assert o_err < ATT_TOL[precision], o_err
    return report


# S: below one streamed tile with a wave's 32 lanes empty / partly filled / full (1, 8, 31, 33, 63); one tile without and with a tail (64, 65); either side
# of the 128-row lane block (127, 128, 129); a partial second lane block over three tiles (136); three and four tiles (192, 256) and a fifth of one row (257).
# (1, 2, 1500): 24 tiles with a tail.  (3, 5, 257): 45 workgroups, no multiple of the 8 XCDs the workgroup order deals them to.
SHAPES = [(2, 3, S) for S in (1, 8, 31, 33, 63, 64, 65, 127, 128, 129, 136, 192, 256, 257)] + [(1, 2, 1500), (3, 5, 257)]


@pytest.mark.parametrize("precision", ["bf16x3", "bf16"])
@pytest.mark.parametrize("B,H,S", SHAPES)
def test_every_branch_of_both_launches_against_fp64(precision, B, H, S):
    within_bound(f"{precision} {(B, H, S)}", run(inputs(B, H, S), precision), B, H, S, precision)


@pytest.mark.parametrize("precision", ["bf16x3", "bf16"])
@pytest.mark.parametrize("S", [33, 129, 257])
def test_both_query_tilings_of_the_training_forward(precision, S):
    B, H = 2, 3
    got = {}
    for qt in (1, 2):
        with tuning(attn_qt=qt):
            got[qt] = planes(inputs(B, H, S), precision)
        within_bound(f"{precision} S={S} attn_qt={qt}", joined(got[qt], B, H, S), B, H, S, precision)
    assert same_bits(got[1][:3], got[2][:3])          # o_hi, o_lo, lse2: a query's arithmetic does not depend on which tile of its wave holds it
    assert same_bits(got[1], got[2])                  # ... and so neither does anything the backward makes of them


@pytest.mark.parametrize("B,H,S", [(2, 3, 64), (2, 3, 136)])
def test_bf16_gradient_option(B, H, S):
    """terms = 3, grad_terms = 1: the gradient contractions on one bf16 plane.  Within 4 x rounded(3, 1); every gradient of every head outside the
    terms = 3 bound (the mode ran: rounded(3, 1) is >= 48 x that bound on the host); forward outputs the default's, bit for bit."""
    x = inputs(B, H, S)
    default, opt = planes(x, "bf16x3"), planes(x, "bf16x3", "bf16")
    got = joined(opt, B, H, S)
    within_bound(f"bf16x3/bf16 {(B, H, S)}", got, B, H, S, "bf16x3", grad_terms=1)
    assert same_bits(default[:3], opt[:3])
    ex, _ = exact(B, H, S)
    for name in ("dq", "dk", "dv"):
        err, _ = ar.head_errors(name, getattr(got, name), getattr(ex, name))
        tol3, _ = ar.head_errors(name, getattr(rounded(B, H, S, 3, 3), name), getattr(ex, name))
        assert bool((err > ar.FACTOR * tol3).all()), (name, err, tol3)


def test_peaked_rows_recompute_the_forward_probabilities():
    """The input of test_gpu_ops.test_attention_online_softmax_rescale_branch: four keys dominate query 5, one per late tile, logits of 240 log2 units.
    The backward's P = exp2(s - lse2) has to be the forward's: the bound on every output, and with d_o = 1 on row 5 alone dv[key, :] IS that row of P:
    it sums to 1 and P v is o[5]."""
    B, H, S = 1, 1, 448
    q, k, v, d_o = _rand((B, H, S, 64), 10, 0.2), _rand((B, H, S, 64), 11), _rand((B, H, S, 64), 12), _rand((B, S, H * 64), 13)
    for t, key in enumerate([70, 150, 260, 390]):
        k[0, 0, key] = q[0, 0, 5] * (20.0 + 15 * t)
    x = (q, k, v, d_o)
    ex = ar.exact(*x)
    got = run(x)
    ar.check("peaked", got, ar.rounded(*x, terms=3), ex, ar.cancellation_floor(*x, ex))
    assert (got.o - ex.o).abs().max().item() < 3e-4                  # the bound of the forward's own test
    hot = torch.zeros_like(d_o)
    hot[0, 5] = 1.0
    xh = (q, k, v, hot)
    exh = ar.exact(*xh)
    goth = run(xh)
    # (row 5 of P is one key to within 2^-60: its dS, hence all of dq and dk, is cancellation -- nothing to bound there)
    ar.check("peaked, d_o on row 5", goth, ar.rounded(*xh, terms=3), exh, names=("o", "lse2", "delta", "dv"))
    p_row = goth.dv[0, 0, :, 0]
    assert torch.equal(goth.dv[0, 0], p_row[:, None].expand(S, 64).contiguous())        # 1.0 x P: the same value in all 64 columns
    # exponent error of a recomputed P: the two launches sum the score in different orders (a few fp32 ulp each at |s| = 240), lse2 is rounded to fp32
    # and v_log_f32 is good to an ulp: 8 ulp in all, times ln 2; plus 2^-16 for P and dv each stored as hi + lo
    tol = 8 * ar.ulp32(got.lse2.abs().max().item()) * ar.LN2 + 2.0 ** -16
    row_sum, pv = p_row.sum().item(), p_row @ v[0, 0].double()
    print("peaked: |sum P - 1|", abs(row_sum - 1.0), "max |P v - o|", (pv - goth.o[0, 5]).abs().max().item(), "tol", tol, "x max|v|", v.abs().max().item())
    assert abs(row_sum - 1.0) < tol
    assert (pv - goth.o[0, 5]).abs().max().item() < tol * v.abs().max().item()


@pytest.mark.parametrize("precision", ["bf16x3", "bf16"])
@pytest.mark.parametrize("S", [136, 1])
def test_nothing_unwritten_nothing_beyond(precision, S):
    B, H = 2, 3
    lo = precision == "bf16x3"
    specs = [((B * S, H * 64), torch.bfloat16), ((B * S, H * 64), torch.bfloat16), ((B, H, S), torch.float32), ((B, H, S), torch.float32),
             ((B * S, 3 * H * 64), torch.bfloat16), ((B * S, 3 * H * 64), torch.bfloat16)]
    pairs = [_guarded(*spec) for spec in specs]
    out = tuple(None if (i in (1, 5) and not lo) else inner for i, (_, inner) in enumerate(pairs))
    planes(inputs(B, H, S), precision, out=out)
    torch.cuda.synchronize()
    for i, (buf, inner) in enumerate(pairs):
        assert bool((buf[:GUARD] == 0xA5).all()) and bool((buf[-GUARD:] == 0xA5).all()), f"output {i}: a guard byte changed"
        if out[i] is None:
            assert bool(torch.isnan(inner).all()), f"output {i}: a lo plane was written with terms = 1"
        else:
            assert bool(torch.isfinite(inner).all()), f"output {i}: an element was left unwritten"
    assert same_bits(out, planes(inputs(B, H, S), precision))


@pytest.mark.parametrize("precision", ["bf16x3", "bf16"])
def test_exact_identities(precision):
    B, H, S = 3, 2, 136
    q, k, v, d_o = x = inputs(B, H, S)
    base = planes(x, precision)
    assert same_bits(base, planes(x, precision))                                        # no atomics, a fixed workgroup -> rows map
    for b in range(B):                                                                  # a clip's rows do not depend on its neighbours
        alone = planes((q[b:b + 1], k[b:b + 1], v[b:b + 1], d_o[b:b + 1]), precision)
        for t, a in zip(base, alone):
            assert (t is None and a is None) or torch.equal(t.view(B, -1)[b], a.view(-1)), b
    # d_o x 2^7: delta and every gradient plane x 2^7 bit for bit (the encoder's gradient scale, awt_encoder_set_grad_scale_log2, relies on it)
    scaled = planes((q, k, v, d_o * 128.0), precision)
    assert same_bits(scaled[:3], base[:3])
    for i in (3, 4, 5):
        assert (base[i] is None and scaled[i] is None) or torch.equal(scaled[i].float(), base[i].float() * 128.0), i
    # qscale = 2^-3 multiplies dq alone
    d = H * 64
    eighth = planes(x, precision, qscale=0.125)
    assert same_bits(eighth[:4], base[:4])
    for i in (4, 5):
        if base[i] is not None:
            assert torch.equal(eighth[i][:, :d].float(), base[i][:, :d].float() * 0.125) and torch.equal(eighth[i][:, d:], base[i][:, d:]), i


def test_refusals():
    from mlx8_ws_audio_transformer_amd import _lib
    B, H, S = 1, 2, 8
    x = inputs(B, H, S)
    L, s = _lib.lib(), _lib.stream_handle()
    need = int(L.awt_op_attention_backward_workspace_bytes(B, H, S))
    ws = _lib.workspace(need, "cuda")
    out = [torch.full(shape, 7.0, dtype=dt, device="cuda") for shape, dt in
           [((B * S, H * 64), torch.bfloat16)] * 2 + [((B, H, S), torch.float32)] * 2 + [((B * S, 3 * H * 64), torch.bfloat16)] * 2]

    def call(terms=3, grad_terms=3, shape=(B, H, S), ws_bytes=need, null=()):
        ptrs = [None if i in null else _lib.ptr(t) for i, t in enumerate(out)]
        return L.awt_op_attention_backward(_lib.ctx(), *(_lib.ptr(t) for t in x), *ptrs, *shape, 1.0, terms, grad_terms, _lib.ptr(ws), ws_bytes, s)

    cases = [(dict(terms=t, grad_terms=t), INVALID) for t in (2, 4, 5, 0, 6)]
    cases += [(dict(terms=1, grad_terms=3), INVALID), (dict(terms=3, grad_terms=2), INVALID), (dict(terms=5, grad_terms=1), INVALID)]
    cases += [(dict(null=(1,)), INVALID), (dict(null=(5,)), INVALID), (dict(null=(0,)), INVALID), (dict(terms=1, grad_terms=1, null=(4,)), INVALID)]
    cases += [(dict(ws_bytes=need - 1), ERR_WORKSPACE), (dict(shape=(0, H, S)), INVALID), (dict(shape=(B, 0, S)), INVALID), (dict(shape=(B, H, 0)), INVALID)]
    for kwargs, status in cases:
        assert call(**kwargs) == status, kwargs
        assert b"op_attention_backward" in L.awt_last_error(), kwargs
    torch.cuda.synchronize()
    assert all(bool((t == 7).all()) for t in out)
    assert call() == 0 and call(terms=1, grad_terms=1, null=(1, 5)) == 0 and call(grad_terms=1) == 0      # ... and what it accepts
