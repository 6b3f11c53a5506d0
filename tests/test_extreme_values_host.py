"""The plumbing of tests/extreme_values.py on the CPU: `classify`, `assert_same_class` and `assert_contained` report each planted mistake, and every
restatement that tests/test_gpu_extreme_values.py holds a kernel against is evaluated here, in fp32 and in fp64, at that test's own operands.  The
elements the GPU test checks for class only -- finite in fp64, out of fp32's reach -- must lie in the one row per output that the case names; anything
else the two restatements disagree on is a mistake in a restatement or a bound, found here and not skipped there.  Needs no GPU."""
import re

import pytest
import torch

from tests import extreme_values as ev
from tests.extreme_values import INF, NAN, SPECIALS, assert_contained, assert_same_class, classify

CASES = ev.cases()


# ------------------------------------------------------------------------------------------------------------------- the helper on planted mistakes
def test_classify_names_every_class():
    t = torch.tensor([NAN, INF, -INF, 0.0, -0.0, 1e-40, -1e-40, ev.FLT_MAX, -ev.FLT_MAX, 2.5])
    assert [ev.CLASSES[int(c)] for c in classify(t)] == ["nan", "+inf", "-inf", "+0", "-0", "+finite", "-finite", "+finite", "-finite", "+finite"]
    assert classify(t.double()).tolist() == classify(t).tolist()
    assert set(classify(torch.tensor(list(SPECIALS.values()), dtype=torch.float32)).tolist()) == {0, 1, 2, 4, 5, 6}        # no special is flushed or mistaken


PLANTS = {                                                  # (got, want) pairs one element apart, and the classes the message must name
    "a NaN hidden as zero": (0.0, NAN, "finite", "nan"),
    "a NaN made up": (NAN, 1.5, "nan", "finite"),
    "+inf turned into NaN": (NAN, INF, "nan", "+inf"),
    "an overflow to +inf": (INF, 2.0 ** 127, "+inf", "finite"),
    "the wrong infinity": (-INF, INF, "-inf", "+inf"),
    "-inf saturated": (-ev.FLT_MAX, -INF, "finite", "-inf"),
}


@pytest.mark.parametrize("plant", list(PLANTS))
def test_assert_same_class_reports_each_planted_mistake(plant):
    g, w, cg, cw = PLANTS[plant]
    want = torch.arange(12, dtype=torch.float32).reshape(3, 4) - 5.0
    got = want.clone()
    assert_same_class(got, want, "same")
    got[2, 1], want[2, 1] = g, w
    with pytest.raises(AssertionError, match=re.escape(f"op: y: 1 of 12 elements of another class, first at (2, 1): got {g!r} ({cg}), want {w!r} ({cw})")):
        assert_same_class(got, want, "op: y")


def test_assert_same_class_signs_and_shapes():
    want = torch.tensor([0.0, -0.0, 1.0, -0.25])
    assert_same_class(torch.tensor([-0.0, 0.0, -2.0, 0.25]), want, "coarse")                      # zeros and signs are one class unless asked for
    with pytest.raises(AssertionError, match=r"first at \(1,\): got 0\.0 \(\+0\), want -0\.0 \(-0\)"):
        assert_same_class(torch.tensor([0.0, 0.0, 1.0, -0.25]), want, "signed", signs=True)
    with pytest.raises(AssertionError, match=r"got 0\.25 \(\+finite\), want -0\.25 \(-finite\)"):
        assert_same_class(torch.tensor([0.0, -0.0, 1.0, 0.25]), want, "signed", signs=True)
    with pytest.raises(AssertionError, match="shape"):
        assert_same_class(torch.zeros(3), want, "shape")


def test_assert_contained_reports_each_planted_leak():
    clean = torch.arange(20, dtype=torch.float32).reshape(4, 5)
    touched = torch.zeros(4, 1, dtype=torch.bool)
    touched[2] = True                                                                                # row 2 may change, nothing else
    got = clean.clone()
    got[2] = NAN
    assert_contained(got, clean, touched, "row 2")
    for where, value in (((0, 4), NAN), ((3, 0), 15.5), ((1, 2), -7.0)):
        leak = got.clone()
        leak[where] = value
        with pytest.raises(AssertionError, match=re.escape(f"first at {where}: {leak[where].item()!r} against {clean[where].item()!r}")):
            assert_contained(leak, clean, touched, "leak")
    zero = torch.zeros(3)
    with pytest.raises(AssertionError, match=r"first at \(1,\): -0\.0 against 0\.0"):               # the bits, not the values: -0 is a change
        assert_contained(torch.tensor([0.0, -0.0, 0.0]), zero, torch.zeros(3, dtype=torch.bool), "sign")
    nan = torch.full((3,), NAN)
    assert_contained(nan.clone(), nan, torch.zeros(3, dtype=torch.bool), "NaN equals itself")


def test_check_reports_a_wrong_value_a_wrong_class_and_a_reordered_sum():
    by_name = {c.name: c for c in CASES}
    case = by_name["gelu"]
    good = {k: v.float() for k, v in ev.REF["gelu"](case.operands, case.meta, torch.float64).items()}
    ev.check(case, good)
    i = list(SPECIALS).index("+inf")
    bad = {k: v.clone() for k, v in good.items()}
    bad["y"][i] = NAN                                                                                # the defect this suite was written for
    with pytest.raises(AssertionError, match=re.escape(f"gelu: y: 1 of 16 elements of another class, first at (0, {i}): got nan (nan), want inf (+inf)")):
        ev.check(case, bad)
    bad = {k: v.clone() for k, v in good.items()}
    bad["y"][15] += 1e-5
    with pytest.raises(AssertionError, match=r"gelu: y: 1 value\(s\) outside the bound, first at \(0, 15\)"):
        ev.check(case, bad)
    case = by_name["column_sums_ld-300x128in256"]
    sums = ev.REF["column_sums_ld"](case.operands, case.meta, torch.float32)["sums"]
    ev.check(case, {"sums": sums})
    dropped = sums.clone()
    dropped[40] -= case.operands["a"][270, 128 + 40]                                                 # a kernel that loses row 270: finite, the right class, the wrong value
    with pytest.raises(AssertionError, match=r"sums: 1 value\(s\) outside the bound, first at \(0, 40\)"):
        ev.check(case, {"sums": dropped})
    other = ev.REF["column_sums"]({"a": case.operands["a"][:, 128:]}, {}, torch.float32)["sums"]     # the other kernel's order: another number in column 21
    assert other[21] != sums[21]
    with pytest.raises(AssertionError, match="column 21"):
        ev.check(case, {"sums": torch.cat([sums[:21], other[21:22], sums[22:]])})


# ------------------------------------------------------------------------------------------------------------------- the restatements
def test_the_case_list_covers_every_operator_and_every_special():
    assert len({c.name for c in CASES}) == len(CASES)
    assert {c.op for c in CASES} == set(ev.REF) == set(ev.TOL)
    for op in ("layernorm", "rmsnorm", "qk_norm_rope", "embed"):                                     # the row-coupled operators: one special at a time
        names = [c.name for c in CASES if c.op == op]
        for s in SPECIALS:
            assert sum(f"-{s}-" in n for n in names) >= 3, (op, s)
    for c in CASES:
        if c.op in ("gelu", "silu"):                                                                 # element-wise: all of them at once
            planted = next(v for k, v in c.operands.items() if k in ("x", "gu"))
            assert set(classify(planted).reshape(-1).tolist()) >= {0, 1, 2, 4, 5, 6}, c.name


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_class_only_elements_lie_in_the_one_named_row(case):
    """Every element that is finite in fp64 is a value element, unless it lies in the row the case names for that output: there it may be held to the fp32
    restatement or to its class."""
    exp = ev.expected(case)
    assert set(case.class_only) <= set(exp), case.class_only
    assert all(rows == [] for rows in ev.unexplained(case).values()), f"fp32 cannot reach fp64 outside the named rows: {ev.unexplained(case)}"
    for k, e in exp.items():
        fin = torch.isfinite(e.want64)
        assert bool(((e.value | e.fp32_held | e.class_only | e.ordered) == fin).all()) and int(e.value.sum() + e.fp32_held.sum() + e.class_only.sum() + e.ordered.sum()) == int(fin.sum())
        assert bool(torch.isfinite(e.bound[e.value]).all()), f"{k}: a value element without a finite bound"
        excused = (e.fp32_held | e.class_only).any(-1).nonzero().reshape(-1).tolist()
        agree = ev._coarse(classify(e.want64)) == ev._coarse(classify(e.want32))
        print(f"{case.name}: {k}: {int(e.value.sum())} value, {int(e.fp32_held.sum())} fp32-held, {int(e.class_only.sum())} class-only in rows {excused}, "
              f"{int(e.ordered.sum())} ordered, {int((~agree).sum())} of another class in fp32 than in fp64")
        if k in case.class_only:
            row, why = case.class_only[k]
            assert why and excused in ([], [row]), f"{k}: the case names row {row}, the elements out of fp32's reach lie in rows {excused}"
        else:
            assert excused == []
        off = (~agree).any(-1).nonzero().reshape(-1).tolist()                                        # a class fp32 and fp64 disagree on: an overflow, in the named row only
        assert off == [] or (k in case.class_only and off == [case.class_only[k][0]]), f"{k}: fp32 and fp64 classes differ in rows {off}"


def test_the_restatements_keep_the_contract_the_issue_states():
    by_name = {c.name: ev.expected(c) for c in CASES if c.op in ("gelu", "cross_entropy", "softmax") or c.name.startswith(("rmsnorm-d128-+inf", "layernorm-d128-nan"))}
    i = {s: n for n, s in enumerate(SPECIALS)}
    y, dx = by_name["gelu"]["y"].want32[0], by_name["gelu"]["dx"].want32[0]
    assert y[i["+inf"]] == INF and torch.isnan(y[i["nan"]]) and torch.isnan(y[i["-inf"]]) and y[i["+fltmax"]] == ev.FLT_MAX
    assert torch.isfinite(dx[i["+inf"]]) and torch.isnan(dx[i["-inf"]]) and torch.isnan(dx[i["nan"]])
    rms = by_name["rmsnorm-d128-+inf-col0"]["y"].want32[1]                                           # zeros plus one NaN, not a row of NaN
    assert torch.isnan(rms[0]) and bool((rms[1:] == 0).all())
    ln = by_name["layernorm-d128-nan-col0"]
    assert bool(torch.isnan(ln["y"].want32[1]).all()) and bool(torch.isnan(ln["dgamma"].want32).all()) and bool(torch.isfinite(ln["y"].want32[[0, 2, 3, 4]]).all())
    assert by_name["cross_entropy-label_logit_-inf"]["loss"].want32.item() == INF
    assert math_isfinite(by_name["cross_entropy-nan_in_ignored_row"]["loss"].want32.item())
    bad = by_name["cross_entropy-nan_in_counted_row"]
    assert torch.isnan(bad["loss"].want32).item() and bool(torch.isnan(bad["dlogits"].want32[3]).all()) and bool(torch.isfinite(bad["dlogits"].want32[:3]).all())
    p = by_name["softmax-70in72"]["p"].want32
    assert bool(torch.isnan(p[:2]).all()) and bool((p[2, [0, 33, 69]] == 0).all()) and abs(float(p[2].sum()) - 1) < 1e-6
    assert bool(torch.isfinite(by_name["softmax-70in72-1e38"]["p"].want32).all())


def math_isfinite(v):
    return v == v and abs(v) != INF
