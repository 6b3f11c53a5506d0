"""CPU-side: the bound of the attention-backward operator tests (tests/attention_reference.py) tells a correct split-bf16 backward from one that lost
a lo plane.  Everything here is the float64 reference against itself; no kernel runs.

Per gradient and per (batch, head), errors are max |x - exact| / max |exact|; tol = 4 x that of rounded(terms = 3).  On the four shapes:
  * rounded(terms = 3) itself stays below 3e-5 (measured here: 0.8e-5 .. 2.2e-5);
  * with the lo plane of dS lost (dq, dk), with the lo plane of P lost (dv), and with grad_terms = 1 (all three) the error exceeds 20 x tol
    (measured: 21 .. 215 x tol), while the outputs such a loss does not touch do not move."""
import pytest
import torch

from tests import attention_reference as ar

SHAPES = [(1, 2, 8), (2, 2, 64), (1, 2, 136), (1, 3, 257)]
GRADS = ("dq", "dk", "dv")


def inputs(B, H, S, seed=7, device="cpu"):
    g = torch.Generator().manual_seed(seed)
    r = lambda *shape: torch.randn(shape, generator=g)
    q, k, v, d_o = r(B, H, S, 64) * 0.35, r(B, H, S, 64), r(B, H, S, 64), r(B, S, H * 64)
    return tuple(t.to(device) for t in (q, k, v, d_o))


def _rel(name, x, ex):
    err, den = ar.head_errors(name, getattr(x, name), getattr(ex, name))
    return err / den


@pytest.fixture(scope="module", params=SHAPES, ids=lambda s: "B%dH%dS%d" % s)
def case(request):
    x = inputs(*request.param)
    return x, ar.exact(*x), ar.rounded(*x, terms=3)


def test_split_bf16_restatement_is_close_to_exact(case):
    _, ex, rnd = case
    for name in GRADS:
        rel = _rel(name, rnd, ex)
        print(name, "rounded(3) per head", rel.flatten().tolist())
        assert float(rel.max()) < 3e-5, (name, rel)
    assert float(_rel("o", rnd, ex).max()) < 3e-5 and float(_rel("lse2", rnd, ex).max()) < 3e-5 and float(_rel("delta", rnd, ex).max()) < 3e-5


@pytest.mark.parametrize("loss,touched", [("ds_lo", ("dq", "dk")), ("p_lo", ("dv",)), ("grad_terms", GRADS)])
def test_a_lost_lo_plane_is_far_outside_the_bound(case, loss, touched):
    x, ex, rnd = case
    bad = ar.rounded(*x, terms=3, grad_terms=1) if loss == "grad_terms" else ar.rounded(*x, terms=3, drop=(loss,))
    for name in ar.NAMES:
        if name in touched:
            tol, rel = ar.FACTOR * _rel(name, rnd, ex), _rel(name, bad, ex)
            print(loss, name, "per head: error / tol", (rel / tol).flatten().tolist())
            assert bool((rel > 20 * tol).all()), (loss, name, rel, tol)
        else:
            assert torch.equal(getattr(bad, name), getattr(rnd, name)), (loss, name)


def test_bf16_restatement_and_the_scales():
    """terms = 1 is single bf16 (2^-9 per operand: percent-level gradients); qscale multiplies dq alone; a head's outputs depend on that head alone."""
    x = inputs(2, 2, 64)
    ex, r1 = ar.exact(*x), ar.rounded(*x, terms=1)
    for name in GRADS:
        assert 1e-4 < float(_rel(name, r1, ex).max()) < 5e-2
    r3, r3s = ar.rounded(*x, terms=3), ar.rounded(*x, terms=3, qscale=0.125)
    assert torch.equal(r3s.dq, r3.dq * 0.125) and torch.equal(r3s.dk, r3.dk) and torch.equal(r3s.dv, r3.dv)
    assert torch.allclose(ar.exact(*x, qscale=0.125).dq, ex.dq * 0.125, rtol=1e-15, atol=0)
    q, k, v, d_o = x
    one = ar.rounded(q[1:, 1:], k[1:, 1:], v[1:, 1:], d_o[1:, :, 64:], terms=3)
    assert torch.equal(one.dq, r3.dq[1:, 1:]) and torch.equal(one.lse2, r3.lse2[1:, 1:]) and torch.equal(one.o, r3.o[1:, :, 64:])


def test_check_rejects_and_accepts():
    x = inputs(1, 2, 136)
    ex, rnd = ar.exact(*x), ar.rounded(*x, terms=3)
    ar.check("same", rnd, rnd, ex, ar.cancellation_floor(*x, ex))
    with pytest.raises(AssertionError):
        ar.check("lost lo", ar.rounded(*x, terms=3, drop=("ds_lo",)), rnd, ex, ar.cancellation_floor(*x, ex))
    wrong = rnd._replace(dk=rnd.dk.clone())
    wrong.dk[0, 1, 130:] *= 1.01                                   # the last rows of the partial lane block, one head, 1 %
    with pytest.raises(AssertionError):
        ar.check("tail rows", wrong, rnd, ex)
    # S = 1: dq and dk vanish identically; fp32 summation noise of the size the floor allows passes, a hundred times as much does not
    x = inputs(2, 3, 1)
    ex, rnd = ar.exact(*x), ar.rounded(*x, terms=1)
    assert float(ex.dq.abs().max()) == 0.0
    floor = ar.cancellation_floor(*x, ex)
    noisy = rnd._replace(dq=rnd.dq + 0.5 * floor["dq"][..., None, None])
    ar.check("S1", noisy, rnd, ex, floor)
    with pytest.raises(AssertionError):
        ar.check("S1", rnd._replace(dq=rnd.dq + 100 * floor["dq"][..., None, None]), rnd, ex, floor)
