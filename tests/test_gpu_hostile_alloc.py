"""Every operator wrapper run inside poisoned, canary-fenced buffers (tests/hostile_alloc.py): the call may write nothing outside the tensors it is
given or allocates, may let no byte it did not write (and no byte outside an input) reach a result, and may change no input it does not own.

test_sweep runs every case of tests/test_gpu_graph_capture.py::CASES that way.  test_edges adds, per operator family, shapes that are ragged
against the kernel's vector width or tile -- each taken from a parametrisation of the family's own test file -- so that the canary stands where
a `float4` or a tile can overrun.
"""
import pytest
import torch

from tests.hostile_alloc import IN_PLACE, POISON, run_fenced
from tests.test_gpu_graph_capture import CASES, E, R

pytestmark = pytest.mark.gpu

# Case -> the sentence of include/awt.h (in double quotes) that makes the prior content of a buffer the wrapper allocates an input of the call.
# Such a case runs with the allocator's interiors zeroed instead of poisoned; its guards are checked like everyone's.  At most three entries
# (tests/test_hostile_alloc_host.py).
EXEMPT = {}

EDGES = {}


def edge(name):
    def register(build):
        assert name not in EDGES and name not in CASES
        EDGES[name] = build
        return build
    return register


def _run(name, table):
    fn, make_state = table[name]()[:2]
    with torch.no_grad() if not name.startswith("encoder_train_step") else torch.enable_grad():
        n = run_fenced(fn, make_state, in_place=IN_PLACE.get(name, ()), interior=0x00 if name in EXEMPT else POISON)
    print(f"{name}: {n} allocations intercepted")
    if n == 0:                                                                                 # then every output is a state tensor the call updates
        state = make_state(0)
        outs = fn(state)
        torch.cuda.synchronize()
        ptrs = {t.untyped_storage().data_ptr() for t in state.values()}
        assert all(o.untyped_storage().data_ptr() in ptrs for o in outs), f"{name}: no allocation intercepted, yet an output is no state tensor"
    return n


# =================================================================================================================== the edge cases
# Each shape is one its family's own test file runs (named in the comment); where the list of the hostile-allocator issue names a shape the
# wrapper's own test does not run, the comment says which one stands in.
def I(seed, idx, low, high, *shape, dtype=torch.int64):
    return torch.randint(low, high, shape, generator=torch.Generator().manual_seed(1000 * idx + seed + 1), dtype=dtype).cuda()


# ------------------------------------------------------------------------------------------------------------------- GEMM (test_gpu_ops.py)
def _linear(M, N, K, precision, **knobs):
    from mlx8_ws_audio_transformer_amd import ops
    from tests.util import tuning

    def fn(s):
        with tuning(**knobs):
            return (ops.linear(s["x"], s["w"], s["b"], precision),)
    return fn, lambda seed: {"x": R(seed, 1, M, K), "w": R(seed, 2, N, K, scale=K ** -0.5), "b": R(seed, 3, N)}


for _p in ("bf16x3", "f16f8"):
    edge(f"linear-{_p}-1x128x64")(lambda _p=_p: _linear(1, 128, 64, _p))                       # one row: 127 rows of the tile are padding
    edge(f"linear-{_p}-300x256x192")(lambda _p=_p: _linear(300, 256, 192, _p))                 # test_linear: ragged M against every tile height
for _t in (64, 128, 256):
    edge(f"linear-f16f8-300x256x192-tile{_t}")(lambda _t=_t: _linear(300, 256, 192, "f16f8", gemm_tile=_t))
for _p in ("bf16", "fp16", "fp16x3"):                                                          # test_linear's other operand formats: a kernel each
    edge(f"linear-{_p}-300x256x192")(lambda _p=_p: _linear(300, 256, 192, _p))
for _t in (64, 128, 256):
    edge(f"linear-bf16x3-300x256x192-tile{_t}")(lambda _t=_t: _linear(300, 256, 192, "bf16x3", gemm_tile=_t))
edge("linear-f16f8-300x256x192-ping_pong")(lambda: _linear(300, 256, 192, "f16f8", gemm_pp=2))  # test_linear_ping_pong: the panel past row 300


@edge("packed_linear_forward-12x256x128")
def _():
    """test_packed_linear_forward_and_backward_input's smallest shape, without and with a residual the call does not own."""
    from mlx8_ws_audio_transformer_amd import native_decoder as nd
    M, N, K = 12, 256, 128
    pl = nd.PackedLinear(R(7, 1, N, K, scale=K ** -0.5), R(7, 2, N))
    return lambda s: (pl.forward(s["x"]), pl.forward(s["x"], resid=s["r"])), lambda seed: {"x": R(seed, 3, M, K), "r": R(seed, 4, M, pl.Np)}


@edge("packed_linear_backward_input-12x256x128")
def _():
    from mlx8_ws_audio_transformer_amd import native_decoder as nd
    M, N, K = 12, 256, 128
    pl = nd.PackedLinear(R(7, 1, N, K, scale=K ** -0.5), R(7, 2, N))
    return lambda s: (pl.backward_input(s["dy"]),), lambda seed: {"dy": R(seed, 3, M, pl.Np)}


def _linear_decode(M, precision):
    """test_gpu_linear_decode.SHAPES[0] = (200, 64): N = 200 is padded to Np = 256; plain and with the residual."""
    from mlx8_ws_audio_transformer_amd import native_decoder as nd
    N, K = 200, 64
    pl = nd.PackedLinear(R(7, 1, N, K, scale=0.1), R(7, 2, N), precision, backward=False)
    return lambda s: (pl.forward_decode(s["x"]), pl.forward_decode(s["x"], resid=s["r"])), lambda seed: {"x": R(seed, 3, M, K), "r": R(seed, 4, M, pl.Np)}


for _p in ("bf16", "bf16x3"):
    for _m in (1, 3, 8):
        edge(f"linear_decode-{_p}-M{_m}")(lambda _p=_p, _m=_m: _linear_decode(_m, _p))


def _weight_grad(row_map):
    """The capture case's (600, 128, 80) plus one row, so that M is ragged against the contraction tile as in test_weight_grad_kernel_matches_fp64's
    (2999, 128, 80); the row map is test_weight_grad_kernel_conv2_row_map's (S, 2 S, 2, tap - 1) with one group of S = 601 rows."""
    from mlx8_ws_audio_transformer_amd import ops
    M, N, K = 601, 128, 80
    if row_map:
        return (lambda s: (ops.weight_grad(s["dy"], s["x"], row_map=(M, 2 * M, 2, -1)),),
                lambda seed: {"dy": R(seed, 1, M, N), "x": R(seed, 2, 2 * M, K)})
    return lambda s: (ops.weight_grad(s["dy"], s["x"]),), lambda seed: {"dy": R(seed, 1, M, N), "x": R(seed, 2, M, K)}


edge("weight_grad-601x128x80")(lambda: _weight_grad(False))
edge("weight_grad-601x128x80-row_map")(lambda: _weight_grad(True))


# ------------------------------------------------------------------------------------------------------------------- row operators
def _layernorm(M, d):
    from mlx8_ws_audio_transformer_amd import ops
    return (lambda s: (ops.layernorm(s["x"], s["g"], s["b"]),),
            lambda seed: {"x": R(seed, 1, M, d), "g": 1 + 0.3 * R(seed, 2, d), "b": R(seed, 3, d)})


edge("layernorm-1x1280")(lambda: _layernorm(1, 1280))                                          # test_layernorm_wide_rows
edge("layernorm-3x128")(lambda: _layernorm(3, 128))                                            # test_layernorm's d = 128, test_layernorm_wide_rows' M = 3


def _layernorm_backward(M, d, with_dres):
    """test_layernorm_backward_against_fp64: (d, M, with_dres) in [128 .. 1280] x [1, 50, 777] x [False, True]."""
    from mlx8_ws_audio_transformer_amd import native_decoder as nd
    return (lambda s: (nd.layernorm_backward(s["dy"], s["x"], s["g"], s["dres"] if with_dres else None),),
            lambda seed: {"dy": R(seed, 1, M, d), "x": R(seed, 2, M, d), "g": 1 + 0.3 * R(seed, 3, d), "dres": R(seed, 4, M, d)})


edge("layernorm_backward-1x128")(lambda: _layernorm_backward(1, 128, False))
edge("layernorm_backward-50x1280-dres")(lambda: _layernorm_backward(50, 1280, True))


@edge("layernorm_param_grad-257x1280")
def _():
    """LN_PARAM_FP32_ERR's M = 257: one row in the second 256-row slab, at the widest row."""
    from mlx8_ws_audio_transformer_amd import native_decoder as nd
    M, d = 257, 1280
    return lambda s: tuple(nd.layernorm_param_grad(s["dy"], s["x"])), lambda seed: {"dy": R(seed, 1, M, d), "x": R(seed, 2, M, d)}


@edge("layernorm_param_grad-256x1280")
def _():
    """... and M = 256: the slab exactly full."""
    from mlx8_ws_audio_transformer_amd import native_decoder as nd
    M, d = 256, 1280
    return lambda s: tuple(nd.layernorm_param_grad(s["dy"], s["x"])), lambda seed: {"dy": R(seed, 1, M, d), "x": R(seed, 2, M, d)}


@edge("gelu-4")
def _():
    """Four elements, one float4: the operator takes multiples of 4 (test_cross_entropy_gelu_layernorm_and_embedding_ops)."""
    from mlx8_ws_audio_transformer_amd import native_decoder as nd
    return lambda s: (nd.gelu(s["x"]), nd.gelu_backward(s["x"], s["dy"])), lambda seed: {"x": R(seed, 1, 4, scale=2.0), "dy": R(seed, 2, 4)}


def _embed(backward):
    """test_embed_backward_against_fp64_index_add's (M, L, d, vocab, pos0) = (7, 7, 1280, 509, 5): an odd vocabulary, a position offset."""
    from mlx8_ws_audio_transformer_amd import native_decoder as nd
    M, L, d, vocab, pos0 = 7, 7, 1280, 509, 5

    def make_state(seed):
        ids = I(seed, 1, 0, vocab, M // L, L)
        ids[0, 3], ids[0, 6] = ids[0, 1], vocab - 1
        st = {"ids": ids, "tok": R(seed, 2, vocab, d), "pos": R(seed, 3, pos0 + L + 3, d)}
        if backward:
            st["dx"] = R(seed, 4, M, d)
        return st

    def fn(s):
        if not backward:
            return (nd.embed(s["ids"], s["tok"], s["pos"], pos0),)
        nd.embed_backward(s["ids"], s["dx"], s["tok"], s["pos"], pos0)
        return s["tok"], s["pos"]
    return fn, make_state


edge("embed-7x7x1280x509")(lambda: _embed(False))
edge("embed_backward-7x7x1280x509")(lambda: _embed(True))


@edge("column_sums_ld-37x384x256x128")
def _():
    """test_pitched_column_sums_against_fp64's first case: the last 128 columns of a 384-wide matrix, plain and accumulated."""
    from mlx8_ws_audio_transformer_amd import native_decoder as nd
    M, ld, col, width = 37, 384, 256, 128
    return (lambda s: (nd.column_sums_ld(s["a"], col, width), nd.column_sums_ld(s["a"], col, width, out=s["sums"], accumulate=True)),
            lambda seed: {"a": R(seed, 1, M, ld), "sums": R(seed, 2, width)})


@edge("cross_entropy-51865_in_51968")
def _():
    """Whisper's vocabulary in PackedLinear's pitch, one ignored label (test_gpu_decoder_full_backward.py's logits shape)."""
    from mlx8_ws_audio_transformer_amd import native_decoder as nd
    M, vocab, ld = 3, 51865, 51968

    def make_state(seed):
        labels = I(seed, 1, 0, vocab, M)
        labels[1] = -100
        return {"logits": R(seed, 2, M, ld, scale=3.0), "labels": labels}
    return lambda s: tuple(nd.cross_entropy(s["logits"], s["labels"], vocab)), make_state


def _softmax_rows(rows, cols, ld):
    """test_row_softmax_forward_and_backward: both in place, the padding columns untouched."""
    from mlx8_ws_audio_transformer_amd import native_decoder as nd

    def fn(s):
        nd.softmax_rows(s["s"], cols, 0.125)
        nd.softmax_rows_backward(s["s"], s["dp"], cols, 0.125)
        return s["s"], s["dp"]
    return fn, lambda seed: {"s": R(seed, 1, rows, ld, scale=6.0), "dp": R(seed, 2, rows, ld)}


edge("softmax_rows-3x70x72")(lambda: _softmax_rows(3, 70, 72))
edge("softmax_rows-5x1x4")(lambda: _softmax_rows(5, 1, 4))


# ------------------------------------------------------------------------------------------------------------------- batched products
@edge("bmm-1x257x132x70")
def _():
    """test_batched_products_against_fp64's last case: every extent ragged against the tile, K = 70 padded."""
    from mlx8_ws_audio_transformer_amd import native_decoder as nd
    batch, M, N, K = 1, 257, 132, 70
    pb = nd.PackedBatch(R(7, 1, batch, N, K, scale=K ** -0.5))

    def fn(s):
        out = E(batch, M, N)
        nd.bmm((s["a"], 0, K, M * K), pb, M, (out, 0, N, M * N))
        return (out,)
    return fn, lambda seed: {"a": R(seed, 2, batch, M, K)}


@edge("bmm_kmajor-strided_heads")
def _():
    """test_batched_products_with_k_major_operands' second product: one block per side, strided per-head views of [M, H 64] and [M, H, d]."""
    from mlx8_ws_audio_transformer_amd import native_decoder as nd
    M, H, d = 24, 2, 136

    def fn(s):
        dw = E(H * 64, d)
        nd.bmm(None, nd.PackedBatch(kmajor=((s["c"], 0), None, M, H * d, d, H, d, M)), 64, (dw, 0, d, 64 * d), a_kmajor=((s["da2"], 0), None, M, H * 64, 64))
        return (dw,)
    return fn, lambda seed: {"da2": R(seed, 1, M, H * 64), "c": R(seed, 2, M, H, d)}


@edge("bmm_kmajor-two_blocks_pitched")
def _():
    """... and its first: two blocks per side, the left operand's rows S = 70 in a pitch of 72, the result added to `acc` in place."""
    from mlx8_ws_audio_transformer_amd import native_decoder as nd
    B, Rr, S, Sp, d = 3, 20, 70, 72, 136

    def fn(s):
        rhs = nd.PackedBatch(kmajor=((s["dc"], 0), (s["qt"], 0), Rr, d, Rr * d, B, d, 2 * Rr))
        nd.bmm(None, rhs, S, (s["acc"], 0, d, S * d), resid=(s["acc"], 0, d, S * d), a_kmajor=((s["P"], 0), (s["dS"], 0), Rr, Sp, Rr * Sp))
        return (s["acc"],)
    return fn, lambda seed: {"P": R(seed, 1, B * Rr, Sp), "dS": R(seed, 2, B * Rr, Sp), "dc": R(seed, 3, B * Rr, d), "qt": R(seed, 4, B * Rr, d),
                             "acc": R(seed, 5, B, S, d)}


# ------------------------------------------------------------------------------------------------------------------- attention, head_dim 64
def _attention(precision):
    """test_attention's (B, H, S) = (3, 2, 257): one key past four tiles."""
    from mlx8_ws_audio_transformer_amd import ops
    B, H, S = 3, 2, 257
    return (lambda s: (ops.attention(s["q"], s["k"], s["v"], precision),),
            lambda seed: {"q": R(seed, 1, B, H, S, 64, scale=0.35), "k": R(seed, 2, B, H, S, 64), "v": R(seed, 3, B, H, S, 64)})


edge("attention-bf16x3-3x2x257")(lambda: _attention("bf16x3"))
edge("attention-f16f8-3x2x257")(lambda: _attention("f16f8"))


@edge("attention_small-2x2x1x9-causal_off8")
def _():
    """test_small_attention_forward_and_backward's decode-step shape: one query row over nine keys, forward and backward."""
    from mlx8_ws_audio_transformer_amd import native_decoder as nd
    B, H, Lq, Sk, off = 2, 2, 1, 9, 8
    d = H * 64

    def fn(s):
        q, k, v = (s["q"], 0), (s["k"], 0), (s["v"], 0)
        o, lse = nd.attention_small(q, d, k, d, v, d, B, H, Lq, Sk, True, off)
        dq, dk, dv = E(B * Lq, d), E(B * Sk, d), E(B * Sk, d)
        nd.attention_small_backward(q, d, k, d, v, d, o, s["d_o"], lse, (dq, 0), (dk, 0), (dv, 0), B, H, Lq, Sk, True, off)
        return o, lse, dq, dk, dv
    return fn, lambda seed: {"q": R(seed, 1, B * Lq, d), "k": R(seed, 2, B * Sk, d), "v": R(seed, 3, B * Sk, d), "d_o": R(seed, 4, B * Lq, d)}


def _attention_cached(rows, H, Lq, T, Tmax):
    """test_cached_attention_against_fp64_and_the_packed_kernel: q is the first third of the fused projection's rows; the cache positions >= T are
    NaN, as there."""
    from mlx8_ws_audio_transformer_amd import native_decoder as nd
    d = H * 64

    def make_state(seed):
        cache = R(seed, 2, rows, Tmax, 2 * d)
        cache[:, T:] = float("nan")
        return {"q": R(seed, 1, rows * Lq, 3 * d), "cache": cache}
    return lambda s: (nd.attention_cached((s["q"], 0), 3 * d, s["cache"], T, H, Lq),), make_state


edge("attention_cached-3x2x1x1x8")(lambda: _attention_cached(3, 2, 1, 1, 8))
edge("attention_cached-2x2x3x130x448")(lambda: _attention_cached(2, 2, 3, 130, 448))


# ------------------------------------------------------------------------------------------------------------------- Qwen3 operators
@edge("rmsnorm-67x260-pitched")
def _():
    """test_rmsnorm's (67, 260): 65 float4 per row, x at pitch d + 8 and column 4, y at pitch d + 12 and column 8 between two guard rows."""
    from mlx8_ws_audio_transformer_amd import ops
    M, d = 67, 260
    G, ldx, ldy, cx, cy = 2, d + 8, d + 12, 4, 8

    def fn(s):
        ops.rmsnorm((s["x"], cx), ldx, s["g"], M, d, 1e-6, y=(s["y"], G * ldy + cy), ldy=ldy)
        return (s["y"],)
    return fn, lambda seed: {"x": R(seed, 1, M, ldx), "g": 1 + 0.3 * R(seed, 2, d), "y": R(seed, 3, M + 2 * G, ldy)}


@edge("rmsnorm_backward-67x260-dres")
def _():
    """test_rmsnorm_backward's (67, 260, with_dres)."""
    from mlx8_ws_audio_transformer_amd import ops
    M, d = 67, 260
    return (lambda s: (ops.rmsnorm_backward((s["dy"], 0), d, (s["x"], 0), d, s["g"], M, d, 1e-6, dres=(s["dres"], 0), dx=(E(M, d), 0), lddx=d),),
            lambda seed: {"dy": R(seed, 1, M, d), "x": R(seed, 2, M, d), "g": 1 + 0.3 * R(seed, 3, d), "dres": R(seed, 4, M, d)})


@edge("rmsnorm_param_grad-300x260")
def _():
    from mlx8_ws_audio_transformer_amd import ops
    M, d = 300, 260
    return (lambda s: (ops.rmsnorm_param_grad((s["dy"], 0), d, (s["x"], 0), d, M, d, 1e-6),),
            lambda seed: {"dy": R(seed, 1, M, d), "x": R(seed, 2, M, d)})


@edge("silu_mul-67x3072")
def _():
    """test_silu_mul's (67, 3072), forward and backward."""
    from mlx8_ws_audio_transformer_amd import ops
    M, Iw = 67, 3072
    return (lambda s: (ops.silu_mul((s["gu"], 0), 2 * Iw, M, Iw), ops.silu_mul_backward((s["gu"], 0), 2 * Iw, (s["dy"], 0), Iw, M, Iw)),
            lambda seed: {"gu": R(seed, 1, M, 2 * Iw, scale=4.0), "dy": R(seed, 2, M, Iw)})


def _qk_norm_rope(backward):
    """test_qk_norm_rope's (B, Lq, Hq, Hkv, pos0) = (2, 33, 16, 8, 0): Qwen3-0.6B's head counts, a prefill from position 0."""
    from mlx8_ws_audio_transformer_amd import ops
    from tests.test_gpu_graph_capture import _rope_tables
    B, Lq, Hq, Hkv, pos0 = 2, 33, 16, 8, 0
    Tmax, rows, wq, wkv = pos0 + Lq + 3, B * Lq, Hq * 128, Hkv * 128
    cos, sin = _rope_tables(Tmax)
    positions = (pos0 + torch.arange(Lq, dtype=torch.int32)).repeat(B).cuda()

    def forward(s):
        q = E(rows, wq)
        ops.qk_norm_rope((s["qkv"], 0), wq + 2 * wkv, s["qg"], s["kg"], cos, sin, positions, (q, 0), wq, (s["kc"], 0), (s["vc"], 0), wkv, Tmax * wkv,
                         B, Lq, Hq, Hkv, 1e-6)
        return (q,)

    def backward_(s):
        dqkv = E(rows, wq + 2 * wkv)
        gains = ops.qk_norm_rope_backward((s["qkv"], 0), wq + 2 * wkv, s["qg"], s["kg"], cos, sin, positions, (s["dq"], 0), wq, (s["kc"], 0), (s["vc"], 0), wkv,
                                          Tmax * wkv, (dqkv, 0), B, Lq, Hq, Hkv, 1e-6, want_gains=True)
        return (dqkv, *gains)
    return (backward_ if backward else forward,
            lambda seed: {"qkv": R(seed, 1, rows, wq + 2 * wkv, scale=1.5), "qg": 1 + 0.3 * R(seed, 2, 128), "kg": 1 + 0.3 * R(seed, 3, 128),
                          "dq": R(seed, 4, rows, wq), "kc": R(seed, 5, B, Tmax, wkv), "vc": R(seed, 6, B, Tmax, wkv)})


edge("qk_norm_rope-2x33x16x8")(lambda: _qk_norm_rope(False))
edge("qk_norm_rope_backward-2x33x16x8")(lambda: _qk_norm_rope(True))


def _causal(B, Hq, Hkv, Lq, T, Tmax, pitched, backward):
    """tests/test_gpu_qwen_ops.py and test_gpu_qwen_train_ops.py's `_run_attention`: a cache of Tmax rows per batch whose positions >= T are NaN, q (and
    dq) optionally at pitch Hq 128 + 64 from column 32, dk / dv at their own pitch and batch stride.  The pitched buffers are state: only the
    live block of an output may change, which the bit comparison with the plain run's state shows."""
    from mlx8_ws_audio_transformer_amd import ops
    wq, wkv = Hq * 128, Hkv * 128
    ldq, cq = (wq + 64, 32) if pitched else (wq, 0)
    lddkv, Td = wkv + 8, T + 5

    def make_state(seed):
        kc, vc = R(seed, 2, B, Tmax, wkv, scale=1.7), R(seed, 3, B, Tmax, wkv)
        kc[:, T:], vc[:, T:] = float("nan"), float("nan")
        st = {"q": R(seed, 1, B * Lq, ldq, scale=1.7), "kc": kc, "vc": vc}
        if backward:
            st.update(d_o=R(seed, 4, B * Lq, wq), dq=R(seed, 5, B * Lq, ldq), dk=R(seed, 6, B, Td, lddkv), dv=R(seed, 7, B, Td, lddkv))
        return st

    def fn(s):
        q, kc, vc = (s["q"], cq), (s["kc"], 0), (s["vc"], 0)
        if not backward:
            return (ops.causal_attention(q, ldq, kc, vc, wkv, Tmax * wkv, B, Hq, Hkv, Lq, T),)
        o, lse = ops.causal_attention_lse(q, ldq, kc, vc, wkv, Tmax * wkv, B, Hq, Hkv, Lq, T)
        ops.causal_attention_backward(q, ldq, kc, vc, wkv, Tmax * wkv, (o, 0), (s["d_o"], 0), wq, lse, (s["dq"], cq), (s["dk"], 0), (s["dv"], 0), lddkv, Td * lddkv,
                                      B, Hq, Hkv, Lq, T)
        return o, lse, s["dq"], s["dk"], s["dv"]
    return fn, make_state


edge("causal_attention-2x4x2x33x33")(lambda: _causal(2, 4, 2, 33, 33, 33 + 37, False, False))             # test_gpu_qwen_ops.ATT_CASES: tails on both axes
edge("causal_attention_backward-2x4x2x37x37")(lambda: _causal(2, 4, 2, 37, 37, 37 + 37, False, True))      # test_gpu_qwen_train_ops.ATT_CASES: tails on both axes
edge("causal_attention-1x2x1x40x70-pitched")(lambda: _causal(1, 2, 1, 40, 70, 96, True, False))            # ... and its pitched entry, forward
edge("causal_attention_backward-1x2x1x40x70-pitched")(lambda: _causal(1, 2, 1, 40, 70, 96, True, True))    # ... lse and backward


# ------------------------------------------------------------------------------------------------------------------- generation
def _select_tokens(rows, vocab, ld, beams, k):
    """select_partial_kernel walks a row in float4: vocab = 51865 ends one element into its last float4, and ld = 51868 is the tightest pitch the entry
    point takes (ld % 4 == 0), so the last row's last float4 ends with the tensor.  test_select_tokens_matches_torch runs (5, 51865) and beams = 5 at
    the wider pitch 52096."""
    from mlx8_ws_audio_transformer_amd import generation as G
    bits = G.banned_bits([3, 77, 300, vocab - 1], vocab, "cuda")
    return (lambda s: tuple(G.select_tokens(s["logits"], vocab, beams, bits, s["beam_scores"] if beams > 1 else None, beams > 1, k)),
            lambda seed: {"logits": R(seed, 1, rows, ld, scale=3.0), "beam_scores": R(seed, 2, rows, scale=2.0)})


edge("select_tokens-5x51865_in_51868-beams5")(lambda: _select_tokens(5, 51865, 51868, 5, 10))
edge("select_tokens-1x51865_in_51868-greedy")(lambda: _select_tokens(1, 51865, 51868, 1, 1))          # one row: the wrapper derives ld from the row's length
edge("select_tokens-5x509_in_512")(lambda: _select_tokens(5, 509, 512, 1, 1))


@edge("select_tokens_ts-51866_in_51868")
def _():
    """test_select_tokens_ts_matches_hf_processors' large-v3 layout (vocab 51866, greedy, 3 clips in mixed rule branches) at the tightest pitch."""
    from mlx8_ws_audio_transformer_amd import generation as G
    from tests.test_gpu_timestamps import EOS, LAYOUTS, _history
    vocab, rows, begin = 51866, 3, 4
    cur_len, no_ts, eos = begin + 6, LAYOUTS[vocab], EOS[vocab]
    ld = vocab + (-vocab) % 4
    bits = G.banned_bits([50358, 50359, 50360, 50361, 50362], vocab, "cuda")
    rules = G.TimestampRules(eos, no_ts, begin, None)

    def make_state(seed):
        g = torch.Generator().manual_seed(900 + seed)
        x = torch.randn((rows, ld), generator=g) * 3
        x[:, no_ts + 1:vocab] += torch.linspace(-2.0, 2.5, rows)[:, None]
        return {"logits": x.cuda(), "history": _history(rows, begin, cur_len, no_ts + 1, vocab, "mixed", g).cuda()}
    return lambda s: tuple(G.select_tokens(s["logits"], vocab, 1, bits, None, False, 1, rules=rules, history=s["history"], cur_len=cur_len)), make_state


@edge("kv_gather-2x2to3x1x8x8")
def _():
    """One live position of eight, rows of eight floats (two float4): layers 2, 2 source rows gathered into 3."""
    from mlx8_ws_audio_transformer_amd import native_decoder as nd
    layers, src_rows, dst_rows, T, Tmax, width = 2, 2, 3, 1, 8, 8

    def fn(s):
        nd.kv_gather(s["src"], s["dst"], s["parent"], layers, src_rows, dst_rows, T, Tmax, width)
        return (s["dst"],)
    return fn, lambda seed: {"src": R(seed, 1, layers, src_rows, Tmax, width), "dst": R(seed, 2, layers, dst_rows, Tmax, width),
                             "parent": torch.tensor([1, 0, 1], dtype=torch.int32).cuda()}


def _dtw(T, frames, nf):
    """test_dtw_equals_the_reference_on_random_matrices' T = 1 and T = 65 (one row past the 64-row block), with test_dtw_ragged_batch's ragged
    num_frames; the path arrays are masked in front of path_start as in the capture case."""
    from mlx8_ws_audio_transformer_amd import generation as G
    clips = len(nf)
    nfd = torch.tensor(nf, dtype=torch.int32).cuda()
    col = torch.arange(T + frames, dtype=torch.int32).cuda()

    def fn(s):
        jump, text, time, start = G.dtw(s["m"], nfd, negate=True)
        live = col[None, :] >= start[:, None]
        return jump, torch.where(live, text, -1), torch.where(live, time, -1), start
    return fn, lambda seed: {"m": R(seed, 1, clips, T, frames)}


edge("dtw-T1-ragged")(lambda: _dtw(1, 40, [40, 1, 3]))
edge("dtw-T65-ragged")(lambda: _dtw(65, 90, [90, 64, 65]))
edge("dtw-T448-frames3")(lambda: _dtw(448, 3, [3, 1]))                                         # the longest T the operator holds over the fewest frames


# ------------------------------------------------------------------------------------------------------------------- the CNN classifiers' operators
def _conv1d(B, T, cin, cout):
    """test_gpu_cnn_classifier.CONV_SHAPES."""
    from mlx8_ws_audio_transformer_amd import cnn_classifier as cc
    return (lambda s: (cc.conv1d(s["x"], s["w"], s["b"], B, T), cc.conv1d(s["x"], s["w"], s["b"], B, T, "fp16x3")),
            lambda seed: {"x": R(seed, 1, B * T, cin), "w": R(seed, 2, cout, cin, 3, scale=(3 * cin) ** -0.5), "b": R(seed, 3, cout)})


def _conv1d_grads(B, T, cin, cout):
    from mlx8_ws_audio_transformer_amd import cnn_classifier as cc
    return (lambda s: (cc.conv1d_input_grad(s["dy"], s["w"], B, T), cc.conv1d_weight_grad(s["dy"], s["x"], B, T)),
            lambda seed: {"x": R(seed, 1, B * T, cin), "w": R(seed, 2, cout, cin, 3, scale=(3 * cin) ** -0.5), "dy": R(seed, 4, B * T, cout)})


edge("conv1d_grads-1x1x512x512")(lambda: _conv1d_grads(1, 1, 512, 512))                        # one frame: both neighbours are padding
edge("conv1d-1x1x512x512")(lambda: _conv1d(1, 1, 512, 512))
edge("conv1d-2x13x64x128")(lambda: _conv1d(2, 13, 64, 128))


def _bn(B, T, C, pool):
    """BN_CASES of test_gpu_cnn_classifier.py (pool codes 0 and 2) and BN4_CASES of test_gpu_waveform_classifier.py (4 and 5): statistics, forward and
    backward.  The mean pool (0) runs there with T = 1 and 15 only: T = 15 stands in for 13 and 31."""
    from mlx8_ws_audio_transformer_amd import cnn_classifier as cc
    t_out = {0: 1, 2: T // 2, 4: T // 4, 5: 1}[pool]

    def fn(s):
        mean, var = cc.batchnorm_stats(s["x"])
        y = cc.bn_relu_pool(s["x"], mean, var, s["g"], s["b"], 1e-5, B, T, pool)
        return (mean, var, y, *cc.bn_relu_pool_backward(s["dy"], s["x"], mean, var, s["g"], s["b"], 1e-5, B, T, pool))
    return fn, lambda seed: {"x": R(seed, 1, B * T, C), "g": 1 + 0.3 * R(seed, 2, C), "b": R(seed, 3, C), "dy": R(seed, 4, B * t_out, C)}


for _t in (13, 31):
    for _pool in (2, 4, 5):
        edge(f"bn_relu_pool-3x{_t}x128-pool{_pool}")(lambda _t=_t, _pool=_pool: _bn(3, _t, 128, _pool))
edge("bn_relu_pool-3x15x128-pool0")(lambda: _bn(3, 15, 128, 0))


@edge("conv1d_framed-32x8x32-B3-t17-extra5")
def _():
    """FRAMED_CONFIGS' narrowest output, three clips of 17 frames and 5 samples no frame uses: forward and weight gradient."""
    from mlx8_ws_audio_transformer_amd import waveform_classifier as wc
    kernel, stride, cout, B, t1, extra = 32, 8, 32, 3, 17, 5
    n = kernel + (t1 - 1) * stride + extra
    return (lambda s: (wc.conv1d_framed(s["x"], s["w"], s["b"], stride), wc.conv1d_framed_weight_grad(s["dy"], s["x"], kernel, stride)),
            lambda seed: {"x": R(seed, 1, B, n), "w": R(seed, 2, cout, 1, kernel, scale=kernel ** -0.5), "b": R(seed, 3, cout), "dy": R(seed, 4, B * t1, cout)})


# ------------------------------------------------------------------------------------------------------------------- front ends
@edge("logmel_whisper-short_clip")
def _():
    """test_whisper_logmel_matches_golden_and_oracle's "short" clip as the extractor sends it: 16000 samples, padded by the kernel to 3000 frames."""
    from mlx8_ws_audio_transformer_amd.feature_extraction import logmel_whisper_device
    n = 16000
    nv = torch.tensor([n], dtype=torch.int32).cuda()
    return lambda s: (logmel_whisper_device(s["pcm"], nv, n, 3000),), lambda seed: {"pcm": R(seed, 1, 1, n, scale=0.1)}


@edge("logmel_whisper-ragged_batch_of_3")
def _():
    """test_batch_ragged_lengths_and_per_clip_max's lengths (a full row, 12345 and 7 samples) in the trimmed 400 frames."""
    from mlx8_ws_audio_transformer_amd.feature_extraction import logmel_whisper_device
    n = 16000
    nv = torch.tensor([n, 12345, 7], dtype=torch.int32).cuda()
    return lambda s: (logmel_whisper_device(s["pcm"], nv, n, 400),), lambda seed: {"pcm": R(seed, 1, 3, n, scale=0.1)}


@edge("logmel_whisper-int16-128_mels")
def _():
    """large-v3's 128 mel bins from int16 PCM (tests/test_gpu_encoder.py), one second in the trimmed 400 frames, the second clip shorter."""
    from mlx8_ws_audio_transformer_amd.feature_extraction import logmel_whisper_device
    n = 16000
    nv = torch.tensor([n, 9001], dtype=torch.int32).cuda()
    return (lambda s: (logmel_whisper_device(s["pcm"], nv, n, 400, n_mels=128),),
            lambda seed: {"pcm": I(seed, 1, -20000, 20000, 2, n, dtype=torch.int16)})


@edge("mel_spectrogram_log-400x100x1-201_samples")
def _():
    """GENERIC_LOGMEL_CASES[(400, 100, 1)]: 44.1 kHz, one mel bin, the minimum n_samples = n_fft / 2 + 1 (one reflection covers the whole clip)."""
    from mlx8_ws_audio_transformer_amd import urbansound
    return (lambda s: (urbansound.mel_spectrogram_log(s["w"], sample_rate=44100, n_fft=400, hop_length=100, n_mels=1, f_min=50.0, f_max=16000.0),),
            lambda seed: {"w": R(seed, 1, 1, 201, scale=0.1)})


@edge("prepare_waveform-int16_stereo-22051")
def _():
    """test_truncation_int16_and_interleaved's int16 stereo at 44.1 kHz; 22051 = 50 * 441 + 1 samples: one past a multiple of the 441 : 160 ratio."""
    from mlx8_ws_audio_transformer_amd import urbansound
    return (lambda s: (urbansound.prepare_waveform(s["w"], sample_rate=44100, n_out=8000),),
            lambda seed: {"w": I(seed, 1, -20000, 20000, 2, 22051, dtype=torch.int16)})


@pytest.mark.parametrize("name", list(CASES))
def test_sweep(name):
    """For the encoder_train_step-* cases the backward runs on autograd's device thread, which a thread-local dispatch mode does not reach: the
    allocations of the forward (and of zero_adapter_grads) are hostile, those of the backward are torch's own."""
    _run(name, CASES)


@pytest.mark.parametrize("name", list(EDGES))
def test_edges(name):
    _run(name, EDGES)
