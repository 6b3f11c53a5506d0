"""GPU: the f16f8 attention forward (csrc/attention_f8.hip) in every loop path and every output form, and the fp16 / fp16x3 modes of csrc/attention.hip --
one launch at a time through awt_op_attention_ex, against float64.

Bounds, per (batch, head), all from tests/f16f8_attention_reference.py (the float64 restatement `rounded` of the kernel's roundings, and `perturbed`, the
same with 32 fp32 ulp on every score and probability), none from the kernel:
  (a) max |x - exact| <= 4 x max |rounded - exact|, for o and lse2;
  (b) max |lse2 - rounded.lse2| <= that of `perturbed`;
  (c) ||o - rounded.o||_2 / ||exact.o||_2 <= that of `perturbed`;
and ATT_TOL / ATT_TOL_F16F8_CROSS of tests/test_gpu_ops.py as a second cap on o.  tests/test_f16f8_attention_reference_host.py shows what they tell
apart: a lost cross term of q k^T, a wrong scale, a q_hi8 without log2 e, an unmasked tail key, a stale V tile, a lost cross term of P V are each >= 10 x
one of them on every head, while (a) alone passes the first four.  Every case prints its worst head beside its bound (pytest -s).

Inputs: seeded N(0, 1), q x 0.35 as in test_gpu_ops.test_attention; H = 2 or 3, so head-major and row-major strides differ.  The references are computed
on the GPU in float64, once per (shape, P V form)."""
import functools

import pytest
import torch

from tests import attention_reference as ar
from tests import f16f8_attention_reference as fr
from tests.gemm_reference import F8_ACT, F8_LO, _e4m3, e4m3, split_lines
from tests.test_f16f8_attention_reference_host import PEAKED_CAP, peaked_inputs
from tests.test_gpu_ops import ATT_TOL, ATT_TOL_F16F8_CROSS, _rand
from tests.util import guarded, guards_intact, tuning

pytestmark = pytest.mark.gpu

INVALID, ERR_WORKSPACE = -1, -3
PV8 = {4: True, 5: True, 6: False}                 # "attn_shape": every cross term on 4 / 8 waves; P V as one fp16 product on 4 waves (the ring form)
CAP = {True: ATT_TOL_F16F8_CROSS, False: ATT_TOL["f16f8"]}


@functools.lru_cache(maxsize=None)
def inputs(B, H, S):
    return _rand((B, H, S, 64), 7, 0.35), _rand((B, H, S, 64), 8), _rand((B, H, S, 64), 9)


@functools.lru_cache(maxsize=None)
def bounds(B, H, S, pv8):
    return fr.bounds(*inputs(B, H, S), pv8)


def forward(x, shape=0, lse=True, precision="f16f8", **knobs):
    """One launch into fresh fp32 buffers: Outputs(o [B, S, H * 64], lse2 [B, H, S] or None) as the kernel wrote them."""
    from mlx8_ws_audio_transformer_amd import ops
    B, H, S, _ = x[0].shape
    out = {"f32": torch.full((B, S, H * 64), float("nan"), device="cuda")}
    if lse:
        out["lse2"] = torch.full((B, H, S), float("nan"), device="cuda")
    with tuning(attn_shape=shape, **knobs):
        ops.attention_ex(*x, precision, out)
    return fr._out(out["f32"], out.get("lse2"))


def within_bounds(label, got, bnd, cap):
    worst = fr.check_forward(label, got, *bnd)
    err = float((got.o.double() - bnd[0].o).abs().max())
    print(f"{label} o: max-abs {err:.3e} (cap {cap:g})")
    assert err < cap, err
    return worst


# ---------------------------------------------------------------------------------------------- the ring form (attn_shape 6), every tile-count path
# The three loops of attention_f16f8_pipe_kernel<4, false> over ntiles = ceil(S / 64) key tiles, kt = 0 at entry:
#   U  while kt + 9 < ntiles: six tiles with compile-time ring slots and lo_full lane offsets;   P  while kt + 3 < ntiles: two tiles;
#   R  the remainder ntiles - kt = 3, 2 or 1 (1 only at ntiles = 1), its last iteration without next scores, the one before with the tail mask.
# A pair / remainder iteration waits vmcnt(K + V loads) while kt + 3 < ntiles, vmcnt(V loads) while kt + 2 < ntiles, else vmcnt(0): the last is every
# remainder's second-to-last iteration, the middle one the first of R3 and the second of the last P trip before R2.
#   n =  1: U0 P0 R1          2: U0 P0 R2          3: U0 P0 R3          4: U0 P1 R2          5: U0 P1 R3
#        8: U0 P3 R2          9: U0 P3 R3         10: U1 P1 R2 (first entry into U: kt + 9 < 10)
#       11: U1 P1 R3         12: U1 P2 R2         13: U1 P2 R3         15: U1 P3 R3 (kt = 6: 15 < 15 fails: a second trip would stage the last tile, K(14))
#       16: U2 P1 R2 (kt = 6: 15 < 16: the second trip stages through K(14) with lo_full; K(15), partial at S = 997, is staged by P with its own offsets)
#       24 (S = 1500): U3 P2 R2 with a tail
# Each n runs as S = 64 n (no tail: the TAIL instantiation still runs, masking nothing) and S = 64 n - 27 (a 37-key last tile whose LDS-DMA rows are
# clamped).  S = 1: one query, one key.
RING_N = (1, 2, 3, 4, 5, 8, 9, 10, 11, 12, 13, 15, 16)
RING_S = sorted({64 * n - d for n in RING_N for d in (0, 27)} | {1, 1500})


@pytest.mark.parametrize("S", RING_S)
def test_every_tile_count_path_of_the_ring_form(S):
    B, H = 2, 3
    x = inputs(B, H, S)
    got = forward(x, shape=6)               # the knob is tested before with_lse: form 6 writes its lse
    within_bounds(f"ring S={S} ({-(-S // 64)} tiles)", got, bounds(B, H, S, False), CAP[False])
    auto = forward(x, shape=0, lse=False)   # the library's own choice without lse2: the same launch
    assert torch.equal(auto.o, got.o)


# ---------------------------------------------------------------------------------------------- every cross term (attn_shape 4 / 5)
# Two loops: pairs while kt + 2 < ntiles, then two tiles or one, the last with or without the tail mask.
#   n = 1: P0 R1     2: P0 R2     3: P1 R1     4: P1 R2     5: P2 R1;   each with S = 64 n and 64 n - 27
@pytest.mark.parametrize("S", sorted({64 * n - d for n in (1, 2, 3, 4, 5) for d in (0, 27)}))
def test_every_tile_count_path_of_the_cross_term_forms(S):
    B, H = 2, 3
    x = inputs(B, H, S)
    bnd = bounds(B, H, S, True)
    got = {shape: forward(x, shape=shape) for shape in (4, 5)}
    for shape in (4, 5):
        within_bounds(f"form {shape} S={S}", got[shape], bnd, CAP[True])
    # a query's arithmetic is the same code on 4 and on 8 waves: the wave count changes who stages which K / V piece and which workgroup holds the query
    assert torch.equal(got[4].o, got[5].o) and torch.equal(got[4].lse2, got[5].lse2)


@pytest.mark.parametrize("B,H,S,waves", [(8, 32, 8, 8), (1, 2, 8, 4)])
def test_the_automatic_form_with_lse(B, H, S, waves):
    """f16f8_form with lse2 requested: 8 waves when ceil(S / 256) B H >= 256, else 4 (restated here), every cross term either way."""
    assert (8 if -(-S // 256) * B * H >= 256 else 4) == waves
    x = inputs(B, H, S)
    auto = forward(x, shape=0)
    within_bounds(f"automatic {(B, H, S)}", auto, bounds(B, H, S, True), CAP[True])
    forced = forward(x, shape={4: 4, 8: 5}[waves])
    assert torch.equal(auto.o, forced.o) and torch.equal(auto.lse2, forced.lse2)
    assert not torch.equal(auto.o, forward(x, shape=6).o)                    # ... and not the single-product form


# ---------------------------------------------------------------------------------------------- query-block edges
# 128 (forms 4, 6) or 256 (form 5) queries per workgroup, 32 per wave: one query; a wave partly filled / just over; a workgroup one short / one over
@pytest.mark.parametrize("shape", [5, 6])
@pytest.mark.parametrize("S", [1, 31, 33, 127, 129, 255, 257])
def test_query_block_edges(shape, S):
    B, H = 2, 3
    x = inputs(B, H, S)
    within_bounds(f"form {shape} S={S}", forward(x, shape=shape), bounds(B, H, S, PV8[shape]), CAP[PV8[shape]])


# ---------------------------------------------------------------------------------------------- peaked rows inside the unrolled loop
@pytest.mark.parametrize("shape", [6, 4])
def test_peaked_rows_in_every_stage_of_the_loop(shape):
    """S = 1000, 16 tiles (U2 P1 R2): one key dominates queries 5 and 37 of head 0 in each of tiles 2, 5 (first unrolled trip), 8 (second), 13 (pair loop)
    and 15 (the partial last tile), each 15 x |q|^2 log2 e ~ 50 log2 units above the one before: the running maximum jumps and O is rescaled to nothing in
    every stage.  (c) uses the restatement's perturbation on this very input."""
    x = peaked_inputs("cuda")
    bnd = fr.bounds(*x, PV8[shape])
    got = forward(x, shape=shape)
    within_bounds(f"peaked form {shape}", got, bnd, PEAKED_CAP)
    key = 980                                                               # rows 5 and 37 are the last dominating key's value row, to fp16
    for row in (5, 37):
        assert float((got.o[0, row, :64].double() - x[2][0, 0, key].double()).abs().max()) < 2.0 ** -10 * float(x[2][0, 0, key].abs().max())


# ---------------------------------------------------------------------------------------------- every output form, exactly
def _stores(x, shape, hi8=True, ilv=False):
    """One launch into guarded buffers: ({name: (buffer, tensor)}, passed names)"""
    B, H, S, _ = x[0].shape
    M, N = B * S, H * 64
    bufs = {"lse2": guarded((B, H, S), torch.float32)}
    if ilv:
        bufs["ilv"] = guarded((M, N * 4), torch.uint8)
    else:
        bufs.update(hi=guarded((M, N), torch.float16), hi8=guarded((M, N), torch.uint8), lo8=guarded((M, N), torch.uint8))
    names = [n for n in bufs if hi8 or n != "hi8"]
    from mlx8_ws_audio_transformer_amd import ops
    with tuning(attn_shape=shape):
        ops.attention_ex(*x, "f16f8", {n: bufs[n][1] for n in names})
    torch.cuda.synchronize()
    return bufs, names


@pytest.mark.parametrize("S", [136, 577])
@pytest.mark.parametrize("shape", [4, 6])
def test_every_output_form_stores_the_same_fp32(shape, S):
    """The fp32 store, the plane store (with and without hi8) and the split-line store are one kernel and one runtime branch on the same fp32 value v:
    fp16 = fp16(v), hi8 = e4m3(v 2^-2), lo8 = e4m3((v - fp16(v)) 2^9) (common.h f16f8x4<kF8Act>), bit for bit."""
    B, H = 2, 3
    M, N = B * S, H * 64
    x = inputs(B, H, S)
    f32 = forward(x, shape=shape)
    v = f32.o.reshape(M, N)
    full, names = _stores(x, shape)
    for name in ("lse2", "hi", "hi8", "lo8"):
        assert guards_intact(full[name][0]), f"{name}: a guard byte changed"
    p16, hi8, lo8, lse2 = (full[n][1] for n in ("hi", "hi8", "lo8", "lse2"))
    assert torch.equal(lse2, f32.lse2)
    assert torch.equal(p16.view(torch.int16), v.half().view(torch.int16))                     # also: nothing unwritten (the fill is NaN)
    assert torch.equal(e4m3(hi8, F8_ACT), _e4m3(v, F8_ACT))                                   # 0xFF, the fill, decodes to NaN and equals nothing
    assert torch.equal(e4m3(lo8, F8_ACT + F8_LO), _e4m3(v.double() - v.half().double(), F8_ACT + F8_LO))
    assert bool((lo8 != 0).any()) and bool((hi8 != 0).any())

    no_hi8, names = _stores(x, shape, hi8=False)
    assert "hi8" not in names and bool((no_hi8["hi8"][1] == 0xFF).all()), "hi8 was written through a null pointer's buffer"
    for name in ("lse2", "hi", "lo8"):
        assert guards_intact(no_hi8[name][0]) and torch.equal(no_hi8[name][1].view(torch.uint8), full[name][1].view(torch.uint8)), name

    lines, _ = _stores(x, shape, ilv=True)
    assert guards_intact(lines["ilv"][0]) and guards_intact(lines["lse2"][0]) and torch.equal(lines["lse2"][1], lse2)
    l16, l_hi8, l_lo8 = split_lines(lines["ilv"][1].reshape(-1), M, N)
    assert torch.equal(l16, p16.view(torch.uint8).reshape(M, 2 * N)) and torch.equal(l_hi8, hi8) and torch.equal(l_lo8, lo8)

    again, _ = _stores(x, shape)                                                              # no atomics, a fixed workgroup -> rows map
    assert all(torch.equal(again[n][1].view(torch.uint8), full[n][1].view(torch.uint8)) for n in again)
    assert torch.equal(forward(x, shape=shape).o, f32.o)


# ---------------------------------------------------------------------------------------------- the operand images the kernel reads
def test_operand_images():
    """awt_op_attention_ex's workspace is six pieces of B H S 64 x 2 bytes, each on a 256-byte boundary: q, k, v as [fp16 plane][hi8 | lo8] (include/awt.h).
    Every byte the launch reads is the restatement's image of that operand -- for q, the images of q log2(e) as the compiled split kernel forms them
    (tests/f16f8_attention_reference.py: fp16 and lo8 see the product before its rounding to fp32).  With lse2 not requested the form reads v's fp16
    plane alone and v's e4m3 images stay unwritten."""
    from mlx8_ws_audio_transformer_amd import ops
    B, H, S = 2, 3, 257
    x = inputs(B, H, S)
    n = B * H * S * 64
    piece = -(-2 * n // 256) * 256
    assert ops.attention_ex_workspace_bytes(B, H, S) == 6 * piece
    for lse in (True, False):
        ws = torch.full((6 * piece,), 0xFF, dtype=torch.uint8, device="cuda")
        out = {"f32": torch.empty((B, S, H * 64), device="cuda")}
        if lse:
            out["lse2"] = torch.empty((B, H, S), device="cuda")
        ops.attention_ex(*x, "f16f8", out, workspace=ws)
        torch.cuda.synchronize()
        for i, (name, s, scale) in enumerate((("q", fr.F8_Q, fr.LOG2E), ("k", fr.F8_KV, None), ("v", fr.F8_KV, None))):
            w16, w8, wl8 = (t.flatten() for t in fr._images(x[i], s, scale))
            p16, b8 = ws[2 * i * piece:2 * i * piece + 2 * n], ws[(2 * i + 1) * piece:(2 * i + 1) * piece + 2 * n]
            assert torch.equal(p16.view(torch.float16).double(), w16), name
            if name == "v" and not lse:
                assert bool((b8 == 0xFF).all())
                continue
            for what, got, want in (("hi8", e4m3(b8[:n], s), w8), ("lo8", e4m3(b8[n:], s + F8_LO), wl8)):
                print(f"{name} {what} lse={lse}: {int((got != want).sum())} of {n} bytes differ from the restated image")
                assert torch.equal(got, want), (name, what)


# ---------------------------------------------------------------------------------------------- fp16 and fp16x3 of attention.hip
@functools.lru_cache(maxsize=None)
def split_bounds(B, H, S, terms):
    x = inputs(B, H, S)
    return fr.exact(*x), ar.rounded(*x, None, terms=terms)


@pytest.mark.parametrize("qt", [1, 2])
@pytest.mark.parametrize("precision,terms", [("fp16", 2), ("fp16x3", 4)])
@pytest.mark.parametrize("S", [33, 129, 257, 700])
def test_fp16_modes_of_the_split_kernel(S, precision, terms, qt):
    """attention_kernel<TERMS, QT, F16 = true> with one and with two query tiles per wave: bound (a) against the restatement on fp16 planes."""
    B, H = 2, 3
    ex, rnd = split_bounds(B, H, S, terms)
    got = forward(inputs(B, H, S), precision=precision, attn_qt=qt)
    ar.check(f"{precision} S={S} attn_qt={qt}", got, rnd, ex, names=("o", "lse2"))
    err = float((got.o.double() - ex.o).abs().max())
    print(f"{precision} S={S} attn_qt={qt} o: max-abs {err:.3e} (ATT_TOL {ATT_TOL[precision]:g})")
    assert err < ATT_TOL[precision]


# ---------------------------------------------------------------------------------------------- refusals
def test_refusals():
    from mlx8_ws_audio_transformer_amd import _lib
    B, H, S = 1, 2, 8
    x = inputs(B, H, S)
    L, s = _lib.lib(), _lib.stream_handle()
    need = int(L.awt_op_attention_ex_workspace_bytes(B, H, S))
    ws = _lib.workspace(need, "cuda")
    M, N = B * S, H * 64
    out = {"f32": torch.full((B, S, N), 7.0, device="cuda"), "hi": torch.full((M, N), 7.0, dtype=torch.float16, device="cuda"),
           "lo": torch.full((M, N), 7.0, dtype=torch.float16, device="cuda"), "hi8": torch.full((M, N), 7, dtype=torch.uint8, device="cuda"),
           "lo8": torch.full((M, N), 7, dtype=torch.uint8, device="cuda"), "ilv": torch.full((M, 4 * N), 7, dtype=torch.uint8, device="cuda"),
           "lse2": torch.full((B, H, S), 7.0, device="cuda")}
    order = ("f32", "hi", "lo", "hi8", "lo8", "ilv", "lse2")

    def call(names, terms=5, shape=(B, H, S), ws_bytes=need):
        ptrs = [_lib.ptr(out[n]) if n in names else None for n in order]
        return L.awt_op_attention_ex(_lib.ctx(), *(_lib.ptr(t) for t in x), *ptrs, *shape, terms, _lib.ptr(ws), ws_bytes, s)

    cases = [(dict(names=()), INVALID), (dict(names=("lse2",)), INVALID)]                                       # no output at all
    cases += [(dict(names=("ilv",), terms=t), INVALID) for t in (1, 2, 3, 4)]                                   # split lines are an f16f8 format
    cases += [(dict(names=("hi", "hi8")), INVALID), (dict(names=("hi8", "lo8")), INVALID), (dict(names=("hi", "lo", "lo8")), INVALID)]      # null lo8 / hi / a 2-byte lo plane with terms 5
    cases += [(dict(names=("hi",), terms=3), INVALID), (dict(names=("hi",), terms=4), INVALID), (dict(names=("hi", "lo", "lo8"), terms=4), INVALID)]
    cases += [(dict(names=("f32", "ilv")), INVALID), (dict(names=("f32", "hi", "lo8")), INVALID), (dict(names=("ilv", "hi", "lo8")), INVALID)]  # more than one form
    cases += [(dict(names=("f32",), terms=t), INVALID) for t in (0, 6)]
    cases += [(dict(names=("f32",), shape=sh), INVALID) for sh in ((0, H, S), (B, 0, S), (B, H, 0))]
    cases += [(dict(names=("f32", "lse2"), ws_bytes=need - 1), ERR_WORKSPACE), (dict(names=("hi", "lo"), terms=3, ws_bytes=need - 1), ERR_WORKSPACE)]
    for kwargs, status in cases:
        assert call(**kwargs) == status, kwargs
        assert b"op_attention_ex" in L.awt_last_error(), kwargs
    torch.cuda.synchronize()
    assert all(bool((t == 7).all()) for t in out.values())
    # ... and what it accepts: every form, hi8 optional, one plane with a single product
    for kwargs in (dict(names=("f32",)), dict(names=("hi", "lo8", "lse2")), dict(names=("hi", "hi8", "lo8")), dict(names=("ilv",)), dict(names=("hi",), terms=2),
                   dict(names=("hi", "lo"), terms=1), dict(names=("hi", "lo", "lse2"), terms=4), dict(names=("f32", "lse2"), terms=3)):
        assert call(**kwargs) == 0, (kwargs, L.awt_last_error())
    torch.cuda.synchronize()
