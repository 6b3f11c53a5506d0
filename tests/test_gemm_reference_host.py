"""CPU-side: the bound of tests/gemm_reference.py separates what it must, at the shapes of tests/test_gpu_gemm_epilogues.py.

A float32 evaluation of the rounded formulas (`rounded32`: what a correct kernel computes, up to the order of its sums) passes the bound for every epilogue
and precision; each planted defect -- one wrong formula in that same evaluation -- exceeds it, by the factor printed.  A defect is planted at the
precisions where the kernels can show it: a lo plane or an x_lo product exists with three products only (terms 3, 4, 5); the tanh form of GELU differs
from the erf form by at most 4.7e-4, which is below what one bf16 or fp16 plane per operand (terms 1, 2) costs; the saved pre-activation has a lo plane,
and the e4m3 images exist, only where noted."""
import math

import pytest
import torch

from tests import gemm_reference as ref

Q_SCALE = 0.125 * 1.4426950408889634
ALL, SPLIT = (1, 2, 3, 4, 5), (3, 4, 5)


def _side(p, epi, seed=7):
    """Side inputs of an epilogue on problem p, seeded: residual, positional table, saved pre-activation."""
    g = torch.Generator().manual_seed(seed)
    if epi == "f32_resid":
        return {"resid": torch.randn((p.M, p.N), generator=g)}
    if epi == "dgelu":
        return {"pre": ref.bf16_pair(torch.randn((p.M, p.N), generator=g) * 1.5)}
    if epi == "planes":
        return {"scale": 0.75}
    if epi == "gelu_pos":
        return {"pos": torch.randn((50, p.N), generator=g), "rows_pos": 50}
    return {}


def _plain(M, N, K, seed=1):
    x, w, b = ref.make_inputs(M, N, K, seed)
    return ref.Problem(x, w, b)


def _qkv(B, S, H, K=128, seed=2):
    x, w, b = ref.make_inputs(B * S, 3 * H * 64, K, seed)
    return ref.Problem(x, w, b), "qkv", {"scale": Q_SCALE, "S": S, "H": H}


def _conv(B, S, Cin, N, seed=3, rows_pos=None):
    x, w, b = ref.make_inputs(B * 2 * S, N, 3 * Cin, seed)
    g = torch.Generator().manual_seed(seed + 100)
    rows_pos = S if rows_pos is None else rows_pos
    pos = torch.randn((rows_pos, N), generator=g) if rows_pos > 1 else torch.zeros((1, N))
    return ref.Problem(x[:, :Cin].contiguous(), w, b, ref.conv_segs(S, Cin), B * S), "gelu_pos", {"pos": pos, "rows_pos": rows_pos}


def _lora(M, N, K, Ku=64, seed=4):
    x, w, b = ref.make_inputs(M, N, K + Ku, seed)
    return ref.Problem(x, w, b, [(0, 0, K, M, M, 1, 0), (K, K, Ku, M, M, 1, 0)])


@pytest.mark.parametrize("terms", ALL)
def test_float32_evaluation_is_inside_the_bound(terms):
    worst = {}
    plain = [_plain(M, N, K) for M in (1, 127, 128, 129, 200, 256, 257, 300) for N, K in ((128, 64), (256, 192), (384, 128), (768, 768))]
    cases = [(p, epi, None) for p in plain for epi in ("f32", "f32_resid", "planes", "gelu", "gelu_pos", "gelu_save", "dgelu")]
    cases += [_qkv(B, S, H) for B, S, H in ((2, 100, 2), (3, 75, 4), (1, 129, 6))]
    cases += [_conv(2, S, 128, N) for S in (100, 129) for N in (128, 384)] + [_conv(2, 100, 128, 128, rows_pos=1)]
    cases += [(_lora(200, 384, 128), "f32_resid", None), (_lora(200, 256, 192), "dgelu", None)]
    for p, epi, side in cases:
        side = _side(p, epi) if side is None else side
        ex, tol = ref.bound(p, epi, terms, **side)
        ratios = ref.check(f"terms {terms} {epi} M={p.M} N={p.N}", ref.rounded32(p, epi, terms, **side), ex, tol, quiet=True)
        for name, r in ratios.items():
            worst[(epi, name)] = max(worst.get((epi, name), 0.0), r)
    print(f"terms {terms}: float32 evaluation, worst error / bound per output:", {f"{e}.{n}": round(r, 3) for (e, n), r in sorted(worst.items())})
    assert worst and max(worst.values()) <= 1.0


# defect -> (problem and side inputs, epilogue, the output it must show in, the precisions it is planted at)
def _defect_case(defect):
    if defect in ("scale_k", "scale_last_head", "q_hi8_unscaled"):
        p, epi, side = _qkv(2, 100, 2)
        return [(p, side, epi, {"scale_k": "k", "scale_last_head": "q", "q_hi8_unscaled": "q_hi8"}[defect], (5,) if defect == "q_hi8_unscaled" else ALL)]
    if defect in ("pos_row", "pad_row"):
        p, epi, side = _conv(2, 100, 128, 128)
        return [(p, side, epi, "y", ALL)]
    p = _plain(200, 256, 192)
    if defect == "tanh":
        # on the fp32 output of the conv stem at every split precision; on a plane output where the plane pair is finer than the defect: the bound is
        # a max norm, and the f16f8 pair (fp16 + 3 mantissa bits of lo8) rounds this test's largest outputs, ~8, by 2.4e-4 -- half of all the tanh form is off by
        pc, epi, side = _conv(2, 100, 128, 128)
        return [(pc, side, epi, "y", SPLIT), (p, {}, "gelu", "y", (3, 4))]
    epi, terms = {"out_lo": ("planes", SPLIT), "x_lo": ("f32", SPLIT), "resid_row": ("f32_resid", ALL), "pre_hi": ("dgelu", SPLIT)}[defect]
    return [(p, _side(p, epi), epi, "y", terms)]


@pytest.mark.parametrize("defect", ref.DEFECTS)
def test_planted_defect_exceeds_the_bound(defect):
    for p, side, epi, name, terms in [(*c[:4], terms) for c in _defect_case(defect) for terms in c[4]]:
        ex, tol = ref.bound(p, epi, terms, **side)
        err = ref.errors(ref.rounded32(p, epi, terms, defect=defect, **side), ex)
        clean = ref.errors(ref.rounded32(p, epi, terms, **side), ex)
        print(f"defect {defect} terms {terms} {epi}.{name}: {err[name] / tol[name]:.1f} x the bound (without the defect {clean[name] / tol[name]:.2f} x)")
        assert err[name] > tol[name] and clean[name] <= tol[name], (defect, terms, err[name], tol[name])
        with pytest.raises(AssertionError):
            ref.check(defect, ref.rounded32(p, epi, terms, defect=defect, **side), ex, tol, quiet=True)


def test_pre_activation_lo_plane_defect_shows_in_the_saved_planes():
    p = _plain(200, 256, 192)
    for terms in SPLIT:
        ex, tol = ref.bound(p, "gelu_save", terms)
        err = ref.errors(ref.rounded32(p, "gelu_save", terms, defect="out_lo"), ex)
        print(f"defect out_lo terms {terms} gelu_save: y {err['y'] / tol['y']:.1f} x, pre {err['pre'] / tol['pre']:.1f} x the bound")
        assert err["y"] > tol["y"] and err["pre"] > tol["pre"]


def test_e4m3_decoder_and_rounding_agree_on_every_byte():
    raw = torch.arange(256, dtype=torch.uint8)
    finite = (raw & 0x7F) != 0x7F
    for s in (ref.F8_ACT, ref.F8_WGT, ref.F8_Q, ref.F8_KV, ref.F8_ACT + ref.F8_LO):
        v = ref.e4m3(raw, s)
        assert bool(torch.isnan(v[~finite]).all()) and bool(torch.isfinite(v[finite]).all())
        assert torch.equal(ref._e4m3(v[finite], s), v[finite])                      # every code point is a fixed point of the rounding
        assert float(v[finite].abs().max()) == 448.0 * 2.0 ** -s and float(v[finite][v[finite] > 0].min()) == 2.0 ** (-9 - s)
    # ties go to the even mantissa, values beyond the range clamp, the subnormal step is 2^-9
    x = torch.tensor([1.0625, 1.1875, 500.0, -1e9, 2.0 ** -10, 3 * 2.0 ** -10, 0.0], dtype=torch.float64)
    assert ref._e4m3(x, 0).tolist() == [1.0, 1.25, 448.0, -448.0, 0.0, 2.0 ** -8, 0.0]
    if hasattr(torch, "float8_e4m3fn"):                                                # torch's own conversion, where this build has it
        y = torch.randn(4096, dtype=torch.float64, generator=torch.Generator().manual_seed(0)) * 8
        assert torch.equal(ref._e4m3(y.float().double(), 0), y.float().to(torch.float8_e4m3fn).double())
        assert torch.equal(ref.e4m3(y.float().to(torch.float8_e4m3fn).view(torch.uint8), 0), y.float().to(torch.float8_e4m3fn).double())


def test_plane_decoders():
    v = torch.randn(3, 128, generator=torch.Generator().manual_seed(1))
    for fp16 in (False, True):
        t = v.half() if fp16 else v.bfloat16()
        assert torch.equal(ref.planes16(t.view(torch.uint8), fp16), t.double())
    # a split-line image built from its description: element (m, n) in pair n / 64 at e = n % 64: fp16 byte 2 e, hi8 byte 128 + e, lo8 byte 192 + e
    M, N = 3, 128
    h16, hi8, lo8 = v.half().view(torch.uint8).reshape(M, 2 * N), torch.arange(M * N).reshape(M, N).to(torch.uint8), (torch.arange(M * N) * 7).reshape(M, N).to(torch.uint8)
    img = torch.zeros(M, N // 64, 256, dtype=torch.uint8)
    for m in range(M):
        for n in range(N):
            pair, e = n // 64, n % 64
            img[m, pair, 2 * e:2 * e + 2] = h16[m, 2 * n:2 * n + 2]
            img[m, pair, 128 + e], img[m, pair, 192 + e] = hi8[m, n], lo8[m, n]
    got = ref.split_lines(img.reshape(-1), M, N)
    assert all(torch.equal(a, b) for a, b in zip(got, (h16, hi8, lo8)))
    x = torch.tensor([0.1, -3.3, 100.7, 1e-3])
    lo = ((x.double() - x.half().double()) * 2.0 ** (ref.F8_ACT + ref.F8_LO)).float().to(torch.float8_e4m3fn).view(torch.uint8) if hasattr(torch, "float8_e4m3fn") else None
    if lo is not None:
        assert float((ref.join_f16f8(x.half().view(torch.uint8), lo, ref.F8_ACT) - x.double()).abs().max() / 100.7) <= 2.0 ** -15


def test_row_map_of_the_conv_stem():
    p, _, _ = _conv(2, 5, 64, 128)
    src, ok = p.rows(p.segs[0])
    assert src.tolist() == [0, 1, 3, 5, 7, 9, 11, 13, 15, 17] and ok.tolist() == [False] + [True] * 4 + [False] + [True] * 4      # tap 0 reads 2 s - 1
    src, ok = p.rows(p.segs[2])
    assert src.tolist() == [1, 3, 5, 7, 9, 11, 13, 15, 17, 19] and bool(ok.all())
    src, ok = p.rows(p.segs[0], pad_row=True)
    assert ok.tolist() == [False] + [True] * 9 and int(src[5]) == 9                                                               # the defect: clip 1 reads clip 0's last row
    assert math.isclose(float(ref._gelu(torch.tensor(1.0, dtype=torch.float64))), 0.8413447460685429, rel_tol=1e-15)
