"""CPU-side: what the three bounds of the f16f8 attention operator tests (tests/f16f8_attention_reference.py) tell apart.  Everything here is the
float64 reference against itself; no kernel runs.  Each test prints its figures (pytest -s).

Cases: B 2, H 3, S in {8, 257, 700} (one tile with a tail; five tiles with a one-key tail; eleven tiles) on the operator tests' N(0, 1) inputs with
q x 0.35, and the peaked input of the GPU file (B 1, H 2, S = 1000: one key dominates queries 5 and 37 of head 0 in each of tiles 2, 5, 8, 13 and 15,
logits up to 300 log2 units), each with P V as one fp16 product (pv8 = False) and with its two e4m3 cross terms (pv8 = True).

Measured here with ULPS = 32 (distance / bound per (batch, head); a defect has to be >= 4 on every head under at least one bound):
  * `rounded` against exact, max-abs of o: 8.8e-4 .. 9.4e-4 with pv8 = False (cap ATT_TOL 2e-3), 0.7e-4 .. 1.3e-4 with pv8 = True (cap 2e-4); peaked
    6.5e-4 / 4.4e-4 (cap 1.5e-2 of test_attention_online_softmax_rescale_branch: logits of 300 carried to 2^-16);
  * the yardstick, perturbed(32 ulp): lse2 moves by 0.8e-5 .. 4.0e-5 (peaked head: 3.1e-4 = one ulp of lse2 ~ 300 times 10); o by a relative L2 of
    1.3e-6 .. 5.1e-5 with pv8 = False (S = 8: 1e-6 .. 4e-6, few fp16 roundings of P flip among eight keys; S >= 257: 3e-5 .. 5e-5) and 2e-6 .. 8e-6
    with pv8 = True;
  * the logit defects under (b), the lse2 bound: q_lo and scale_lo 28 .. 192, k_lo 42 .. 216, q_hi8_unscaled 13 .. 67; under (c) with pv8 = False
    they are 3.4 .. 15 at S >= 257 and 25 .. 235 at S = 8; under (a) on o with pv8 = False they are 0.2 .. 0.7 (peaked head: 2.5) -- the 4 x bound
    against exact, and a fortiori the flat 2e-3, cannot see them;
  * tail_key: >= 140 under (b); stale_v_tile: >= 7200 under (c) and >= 270 under (a); p_lo: 10.7 .. 29 under (c), 0.25 .. 3.7 under (a);
  * the least ratio of any defect on any head under its best bound: 10.7 (p_lo, S = 700);
  * p_lo and stale_v_tile leave lse2 bit-equal, every other defect moves o and lse2; lse2 does not depend on pv8.
(With ULPS = 16, as first written, every ratio under (b) and (c) was about twice these.)
No defect of the list fails to reach 4 x: none is a printed, unasserted row."""
import functools

import pytest
import torch

from tests import attention_reference as ar
from tests import f16f8_attention_reference as fr

CAPS = {False: 2e-3, True: 2e-4}                   # ATT_TOL["f16f8"], ATT_TOL_F16F8_CROSS of tests/test_gpu_ops.py
PEAKED_CAP = 1.5e-2                                # test_attention_online_softmax_rescale_branch, f16f8
PEAKS = (134, 330, 532, 862, 980)                  # one key in each of tiles 2, 5, 8, 13 and 15 (the partial one) of S = 1000


def inputs(B, H, S, seed=7, device="cpu"):
    g = torch.Generator().manual_seed(seed)
    r = lambda: torch.randn((B, H, S, 64), generator=g)
    q, k, v = r() * 0.35, r(), r()
    return tuple(t.to(device) for t in (q, k, v))


def peaked_inputs(device="cpu"):
    """The input of test_gpu_ops.test_attention_online_softmax_rescale_branch at S = 1000 and H = 2: queries 5 and 37 of head 0 share one direction, and
    one key per tile of PEAKS is that direction times 20, 35, 50, 65, 80."""
    r = lambda seed, scale=1.0: torch.randn((1, 2, 1000, 64), generator=torch.Generator().manual_seed(seed)) * scale
    q, k, v = r(10, 0.2), r(11), r(12)
    q[0, 0, 37] = q[0, 0, 5]
    for t, key in enumerate(PEAKS):
        k[0, 0, key] = q[0, 0, 5] * (20.0 + 15 * t)
    return tuple(t.to(device) for t in (q, k, v))


CASES = ["S8", "S257", "S700", "peaked"]


@functools.lru_cache(maxsize=None)
def case(name, pv8):
    x = peaked_inputs() if name == "peaked" else inputs(2, 3, int(name[1:]))
    return (x,) + fr.bounds(*x, pv8)


@pytest.mark.parametrize("pv8", [False, True])
@pytest.mark.parametrize("name", CASES)
def test_restatement_is_within_the_suite_caps(name, pv8):
    x, ex, rnd, yard = case(name, pv8)
    err = float((rnd.o - ex.o).abs().max())
    cap = PEAKED_CAP if name == "peaked" else CAPS[pv8]
    print(f"{name} pv8={pv8}: rounded max-abs o {err:.3e} (cap {cap:g}); yardstick lse2 {yard[0].flatten().tolist()} o rel L2 {yard[1].flatten().tolist()}")
    assert err < cap
    assert bool((yard[0] > 0).all()) and bool((yard[1] > 0).all())
    fr.check_forward(f"{name} pv8={pv8} rounded against itself", rnd, ex, rnd, yard)
    assert torch.equal(rnd.lse2, case(name, not pv8)[2].lse2)              # the normaliser sums the unrounded P: lse2 does not know the P V form


@pytest.mark.parametrize("defect", fr.DEFECTS)
@pytest.mark.parametrize("pv8", [False, True])
@pytest.mark.parametrize("name", CASES)
def test_every_defect_is_outside_a_bound(name, pv8, defect):
    x, ex, rnd, yard = case(name, pv8)
    if not fr.can_act(defect, x[0].shape[2], pv8):
        with pytest.raises(AssertionError):
            fr.rounded(*x, pv8, defect=defect)
        return
    bad = fr.rounded(*x, pv8, defect=defect)
    r = fr.ratios(bad, ex, rnd, yard)
    best = torch.stack(list(r.values())).amax(0)
    print(f"{name} pv8={pv8} {defect}: distance / bound over heads " + ", ".join(f"({key}) {float(val.min()):.2f} .. {float(val.max()):.2f}" for key, val in r.items()) +
          f"; least best {float(best.min()):.1f}")
    assert bool((best >= 4.0).all()), (name, pv8, defect, {key: val.tolist() for key, val in r.items()})
    with pytest.raises(AssertionError):
        fr.check_forward("planted", bad, ex, rnd, yard)
    assert not torch.equal(bad.o, rnd.o)
    if defect in ("p_lo", "stale_v_tile"):
        assert torch.equal(bad.lse2, rnd.lse2)
    else:
        assert not torch.equal(bad.lse2, rnd.lse2)


def test_the_bound_against_exact_alone_cannot_see_the_logits():
    """Why (b) and (c) exist: with P V as one fp16 product, each logit defect is inside the 4 x bound against exact on o for every head of S >= 257."""
    for name in ("S257", "S700"):
        x, ex, rnd, yard = case(name, False)
        for defect in fr.LOGIT_DEFECTS:
            r = fr.ratios(fr.rounded(*x, False, defect=defect), ex, rnd, yard)
            assert float(r["a_o"].max()) < 1.0 and float(r["b"].min()) > 4.0, (name, defect)


def test_a_head_depends_on_that_head_alone_and_the_seed_matters():
    (q, k, v), ex, rnd, yard = case("S257", False)
    one = fr.rounded(q[1:, 2:], k[1:, 2:], v[1:, 2:], False)
    assert torch.equal(one.o, rnd.o[1:, :, 128:]) and torch.equal(one.lse2, rnd.lse2[1:, 2:])
    a, b = fr.perturbed(q, k, v, False, seed=0), fr.perturbed(q, k, v, False, seed=1)
    assert not torch.equal(a.o, b.o) and torch.equal(a.o, fr.perturbed(q, k, v, False, seed=0).o)
    assert torch.equal(fr.perturbed(q, k, v, False, ulps=0).o, rnd.o)


@pytest.mark.parametrize("terms,cap", [(2, 5e-3), (4, 2e-5)])             # ATT_TOL of tests/test_gpu_ops.py
def test_fp16_forms_of_the_split_restatement(terms, cap):
    """attention_reference.rounded, forward half, on fp16 planes: common.h split16<true> is hi = fp16(x), lo = fp16(x - hi) with no scale on lo."""
    q, k, v = inputs(2, 3, 257)
    ex, rnd = fr.exact(q, k, v), ar.rounded(q, k, v, None, terms=terms)
    err = float((rnd.o - ex.o).abs().max())
    print(f"terms {terms}: rounded max-abs o {err:.3e} (cap {cap:g}), lse2 {float((rnd.lse2 - ex.lse2).abs().max()):.3e}")
    assert err < cap and rnd.delta is None
    hi, lo = ar._split(v, terms)
    assert torch.equal(hi, v.half().double())
    if terms == 4:
        assert torch.equal(lo, (v.double() - hi).float().half().double())
        # lo <= 2^-11 |x| keeps 11 bits while it is a normal fp16 number, and is within half a subnormal step (2^-25) below that
        assert bool(((hi + lo - v.double()).abs() <= torch.maximum(2.0 ** -22 * v.double().abs(), torch.tensor(2.0 ** -25, dtype=torch.float64))).all())
    else:
        assert not bool(lo.any())
    # the forward half of the bf16 forms is the training restatement's: the same lse2, o before its split into planes
    full, fwd = ar.rounded(q, k, v, torch.zeros(2, 257, 192), terms=3), ar.rounded(q, k, v, None, terms=3)
    assert torch.equal(full.lse2, fwd.lse2) and float((full.o - fwd.o).abs().max()) < 2.0 ** -16
