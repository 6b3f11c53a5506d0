"""Every operator wrapper, and three composite passes, captured into a HIP graph on one state and replayed on another (tests/graph_capture.py):
the replay must return the bits of the eager call on the same inputs.  That holds an entry point to what include/awt.h says of it -- all work on
the caller's stream, no synchronisation, no allocation, no host read of device data -- which the default stream cannot show.

One case per wrapper at the smallest shape its own test file uses; two precisions only where they launch different kernels.  A case is a
function returning (fn, make_state) and, for the Qwen3 decode step, how state B reaches the static tensors.  Handles, packed weights, tables and
constant index tensors are built while the case is set up (creation time); everything `fn` does is inside the graph.
"""
import functools

import numpy as np
import pytest
import torch

from tests.graph_capture import COVERED, capture_replay

pytestmark = pytest.mark.gpu

CASES = {}


def case(name):
    def register(build):
        assert name not in CASES
        CASES[name] = build
        return build
    return register


def R(seed, idx, *shape, scale=1.0):
    """Seeded N(0, scale^2) values on the device; (seed, idx) names the tensor, so states A (seed 0) and B (seed 1) differ everywhere."""
    return (torch.randn(shape, generator=torch.Generator().manual_seed(1000 * idx + seed + 1)) * scale).cuda()


def Z(*shape, dtype=torch.float32):
    return torch.zeros(shape, dtype=dtype, device="cuda")


def E(*shape, dtype=torch.float32):
    return torch.empty(shape, dtype=dtype, device="cuda")


# =================================================================================================================== ops.py
def _linear(precision):
    from mlx8_ws_audio_transformer_amd import ops
    M, N, K = 128, 128, 64
    return (lambda s: (ops.linear(s["x"], s["w"], s["b"], precision),),
            lambda seed: {"x": R(seed, 1, M, K), "w": R(seed, 2, N, K), "b": R(seed, 3, N)})


case("linear-bf16x3")(lambda: _linear("bf16x3"))
case("linear-f16f8")(lambda: _linear("f16f8"))


@case("linear_fused-f32_resid")
def _():
    from mlx8_ws_audio_transformer_amd import ops
    M, N, K = 129, 128, 64

    def fn(s):
        ops.linear_fused(s["x"], s["w"], s["b"], "f32_resid", "bf16x3", {"f32": s["y"]}, resid=s["y"])        # in place: y += x w^T + b
        return (s["y"],)
    return fn, lambda seed: {"x": R(seed, 1, M, K), "w": R(seed, 2, N, K), "b": R(seed, 3, N), "y": R(seed, 4, M, N)}


def _linear_fused_qkv(precision):
    """The "qkv" epilogue needs N = 3 H 64 and M % S == 0: M = S = 129 rows, H = 2, so N = 384 is the narrowest it takes."""
    from mlx8_ws_audio_transformer_amd import ops
    M, H, K = 129, 2, 64
    N, f8 = 3 * H * 64, precision == "f16f8"
    keys = ("hi", "hi8", "lo8") if f8 else ("hi", "lo")
    dt = {"hi": torch.float16 if f8 else torch.bfloat16, "lo": torch.bfloat16, "hi8": torch.uint8, "lo8": torch.uint8}

    def fn(s):
        ops.linear_fused(s["x"], s["w"], s["b"], "qkv", precision, {k: s[k] for k in keys}, scale=0.125, S=M, H=H)
        return tuple(s[k] for k in keys)

    def make_state(seed):
        st = {"x": R(seed, 1, M, K), "w": R(seed, 2, N, K), "b": R(seed, 3, N)}
        st.update({k: Z(3, 1, H, M, 64, dtype=dt[k]) for k in keys})
        return st
    return fn, make_state


case("linear_fused-qkv-bf16x3")(lambda: _linear_fused_qkv("bf16x3"))
case("linear_fused-qkv-f16f8")(lambda: _linear_fused_qkv("f16f8"))


@case("layernorm")
def _():
    from mlx8_ws_audio_transformer_amd import ops
    M, d = 5, 384
    return (lambda s: (ops.layernorm(s["x"], s["g"], s["b"]),),
            lambda seed: {"x": R(seed, 1, M, d), "g": 1 + 0.3 * R(seed, 2, d), "b": R(seed, 3, d)})


def _qkv64(seed, B=1, H=2, S=129):
    return {"q": R(seed, 1, B, H, S, 64, scale=0.3), "k": R(seed, 2, B, H, S, 64), "v": R(seed, 3, B, H, S, 64)}


def _attention(precision):
    from mlx8_ws_audio_transformer_amd import ops
    return lambda s: (ops.attention(s["q"], s["k"], s["v"], precision),), _qkv64


case("attention-bf16x3")(lambda: _attention("bf16x3"))
case("attention-f16f8")(lambda: _attention("f16f8"))


@case("attention_ex")
def _():
    from mlx8_ws_audio_transformer_amd import ops
    B, H, S = 1, 2, 129

    def fn(s):
        o, lse2 = E(B, S, H * 64), E(B, H, S)
        ops.attention_ex(s["q"], s["k"], s["v"], "bf16x3", {"f32": o, "lse2": lse2})
        return o, lse2
    return fn, _qkv64


@case("attention_backward")
def _():
    from mlx8_ws_audio_transformer_amd import ops
    B, H, S = 1, 2, 129

    def make_state(seed):
        return dict(_qkv64(seed), d_o=R(seed, 4, B, S, H * 64))
    return lambda s: tuple(ops.attention_backward_planes(s["q"], s["k"], s["v"], s["d_o"], "bf16x3")), make_state


@case("weight_grad-plain")
def _():
    from mlx8_ws_audio_transformer_amd import ops
    M, N, K = 600, 128, 80
    return lambda s: (ops.weight_grad(s["dy"], s["x"]),), lambda seed: {"dy": R(seed, 1, M, N), "x": R(seed, 2, M, K)}


@case("weight_grad-row_map")
def _():
    """conv2's row map: 300 output rows per group read rows 2 m - 1 of the group's 600 (the first one reads as zero)."""
    from mlx8_ws_audio_transformer_amd import ops
    M, N, K = 600, 128, 80
    return (lambda s: (ops.weight_grad(s["dy"], s["x"], row_map=(300, 600, 2, -1)),),
            lambda seed: {"dy": R(seed, 1, M, N), "x": R(seed, 2, 2 * M, K)})


def _cross_attention(B, H, Lq, Sk, backward):
    from mlx8_ws_audio_transformer_amd import ops
    w = H * 128

    def fn(s):
        q, k, v = (s["q"], 0), (s["k"], 0), (s["v"], 0)
        o, lse = ops.cross_attention(q, w, k, w, v, w, B, H, Lq, Sk, "bf16x3")
        if not backward:
            return o, lse
        dq, dk, dv = E(B * Lq, w), E(B * Sk, w), E(B * Sk, w)
        ops.cross_attention_backward(q, w, k, w, v, w, (o, 0), (s["d_o"], 0), w, lse, (dq, 0), (dk, 0), (dv, 0), B, H, Lq, Sk, "bf16x3")
        return dq, dk, dv

    def make_state(seed):
        st = {"q": R(seed, 1, B * Lq, w, scale=1.7), "k": R(seed, 2, B * Sk, w, scale=1.7), "v": R(seed, 3, B * Sk, w)}
        if backward:
            st["d_o"] = R(seed, 4, B * Lq, w)
        return st
    return fn, make_state


# test_gpu_cross_attention.CASES: the one with the fewest scores (a single key) and the smallest with tails on both axes
for _shape in ((2, 2, 64, 1), (2, 2, 17, 70)):
    case("cross_attention-" + "x".join(map(str, _shape)))(functools.partial(_cross_attention, *_shape, False))
    case("cross_attention_backward-" + "x".join(map(str, _shape)))(functools.partial(_cross_attention, *_shape, True))


@case("rmsnorm")
def _():
    from mlx8_ws_audio_transformer_amd import ops
    M, d = 5, 1024
    return (lambda s: (ops.rmsnorm((s["x"], 0), d, s["g"], M, d, 1e-6),),
            lambda seed: {"x": R(seed, 1, M, d), "g": 1 + 0.3 * R(seed, 2, d)})


def _rope_tables(rows):
    inv_freq = 1.0 / (1e6 ** (torch.arange(0, 128, 2, dtype=torch.float32) / 128))
    ang = torch.arange(rows, dtype=torch.float32)[:, None] * inv_freq[None, :]
    return ang.cos().cuda().contiguous(), ang.sin().cuda().contiguous()


@case("qk_norm_rope")
def _():
    from mlx8_ws_audio_transformer_amd import ops
    B, Lq, Hq, Hkv, pos0 = 2, 5, 4, 1, 65
    Tmax, rows, wq, wkv = pos0 + Lq + 3, B * Lq, Hq * 128, Hkv * 128
    cos, sin = _rope_tables(Tmax)
    positions = (pos0 + torch.arange(Lq, dtype=torch.int32)).repeat(B).cuda()

    def fn(s):
        q = E(rows, wq)
        ops.qk_norm_rope((s["qkv"], 0), wq + 2 * wkv, s["qg"], s["kg"], cos, sin, positions, (q, 0), wq, (s["kc"], 0), (s["vc"], 0), wkv, Tmax * wkv,
                         B, Lq, Hq, Hkv, 1e-6)
        return (q,)                                                                            # the KV caches are state: rows pos0 .. pos0 + Lq - 1 are written
    return fn, lambda seed: {"qkv": R(seed, 1, rows, wq + 2 * wkv, scale=1.5), "qg": 1 + 0.3 * R(seed, 2, 128), "kg": 1 + 0.3 * R(seed, 3, 128),
                             "kc": R(seed, 4, B, Tmax, wkv), "vc": R(seed, 5, B, Tmax, wkv)}


@case("qk_norm_rope_backward")
def _():
    from mlx8_ws_audio_transformer_amd import ops
    B, Lq, Hq, Hkv, pos0 = 1, 1, 4, 2, 700
    Tmax, rows, wq, wkv = pos0 + Lq + 3, B * Lq, Hq * 128, Hkv * 128
    cos, sin = _rope_tables(Tmax)
    positions = (pos0 + torch.arange(Lq, dtype=torch.int32)).repeat(B).cuda()

    def fn(s):
        dqkv = E(rows, wq + 2 * wkv)
        gains = ops.qk_norm_rope_backward((s["qkv"], 0), wq + 2 * wkv, s["qg"], s["kg"], cos, sin, positions, (s["dq"], 0), wq, (s["dk"], 0), (s["dv"], 0), wkv,
                                          Tmax * wkv, (dqkv, 0), B, Lq, Hq, Hkv, 1e-6, want_gains=True)
        return (dqkv, *gains)
    return fn, lambda seed: {"qkv": R(seed, 1, rows, wq + 2 * wkv, scale=1.5), "qg": 1 + 0.3 * R(seed, 2, 128), "kg": 1 + 0.3 * R(seed, 3, 128),
                             "dq": R(seed, 4, rows, wq), "dk": R(seed, 5, B, Tmax, wkv), "dv": R(seed, 6, B, Tmax, wkv)}


@case("silu_mul")
def _():
    from mlx8_ws_audio_transformer_amd import ops
    M, I = 1, 384
    return lambda s: (ops.silu_mul((s["gu"], 0), 2 * I, M, I),), lambda seed: {"gu": R(seed, 1, M, 2 * I, scale=4.0)}


@case("silu_mul_backward")
def _():
    from mlx8_ws_audio_transformer_amd import ops
    M, I = 1, 384
    return (lambda s: (ops.silu_mul_backward((s["gu"], 0), 2 * I, (s["dy"], 0), I, M, I),),
            lambda seed: {"gu": R(seed, 1, M, 2 * I, scale=4.0), "dy": R(seed, 2, M, I)})


@case("rmsnorm_backward")
def _():
    from mlx8_ws_audio_transformer_amd import ops
    M, d = 1, 128
    return (lambda s: (ops.rmsnorm_backward((s["dy"], 0), d, (s["x"], 0), d, s["g"], M, d, 1e-6),),
            lambda seed: {"dy": R(seed, 1, M, d), "x": R(seed, 2, M, d), "g": 1 + 0.3 * R(seed, 3, d)})


@case("rmsnorm_backward-dres_in_place")
def _():
    from mlx8_ws_audio_transformer_amd import ops
    M, d = 5, 1024

    def fn(s):
        ops.rmsnorm_backward((s["dy"], 0), d, (s["x"], 0), d, s["g"], M, d, 1e-6, dres=(s["dres"], 0), dx=(s["dres"], 0), lddx=d)
        return (s["dres"],)
    return fn, lambda seed: {"dy": R(seed, 1, M, d), "x": R(seed, 2, M, d), "g": 1 + 0.3 * R(seed, 3, d), "dres": R(seed, 4, M, d)}


@case("rmsnorm_param_grad")
def _():
    from mlx8_ws_audio_transformer_amd import ops
    M, d = 1, 128
    return (lambda s: (ops.rmsnorm_param_grad((s["dy"], 0), d, (s["x"], 0), d, M, d, 1e-6),),
            lambda seed: {"dy": R(seed, 1, M, d), "x": R(seed, 2, M, d)})


def _causal_state(B, Hq, Hkv, Lq, T, backward):
    def make_state(seed):
        st = {"q": R(seed, 1, B * Lq, Hq * 128, scale=1.7), "kc": R(seed, 2, B, T, Hkv * 128, scale=1.7), "vc": R(seed, 3, B, T, Hkv * 128)}
        if backward:
            st["d_o"] = R(seed, 4, B * Lq, Hq * 128)
        return st
    return make_state


def _causal_attention(B, Hq, Hkv, Lq, T):
    from mlx8_ws_audio_transformer_amd import ops
    wq, wkv = Hq * 128, Hkv * 128
    return (lambda s: (ops.causal_attention((s["q"], 0), wq, (s["kc"], 0), (s["vc"], 0), wkv, T * wkv, B, Hq, Hkv, Lq, T),),
            _causal_state(B, Hq, Hkv, Lq, T, False))


case("causal_attention-decode")(lambda: _causal_attention(2, 4, 2, 1, 77))
case("causal_attention-chunked_prefill")(lambda: _causal_attention(2, 4, 1, 5, 70))


def _causal_lse(backward):
    from mlx8_ws_audio_transformer_amd import ops
    B, Hq, Hkv, Lq, T = 2, 4, 1, 5, 70
    wq, wkv = Hq * 128, Hkv * 128

    def fn(s):
        q, kc, vc = (s["q"], 0), (s["kc"], 0), (s["vc"], 0)
        o, lse = ops.causal_attention_lse(q, wq, kc, vc, wkv, T * wkv, B, Hq, Hkv, Lq, T)
        if not backward:
            return o, lse
        dq, dk, dv = E(B * Lq, wq), E(B, T, wkv), E(B, T, wkv)
        ops.causal_attention_backward(q, wq, kc, vc, wkv, T * wkv, (o, 0), (s["d_o"], 0), wq, lse, (dq, 0), (dk, 0), (dv, 0), wkv, T * wkv, B, Hq, Hkv, Lq, T)
        return dq, dk, dv
    return fn, _causal_state(B, Hq, Hkv, Lq, T, backward)


case("causal_attention_lse")(lambda: _causal_lse(False))
case("causal_attention_backward")(lambda: _causal_lse(True))


# =================================================================================================================== native_decoder.py
@case("packed_linear_forward")
def _():
    """In place with `resid`: y = x W^T + b + y."""
    from mlx8_ws_audio_transformer_amd import native_decoder as nd
    M, N, K = 12, 256, 128
    pl = nd.PackedLinear(R(7, 1, N, K), R(7, 2, N))

    def fn(s):
        pl.forward(s["x"], resid=s["y"], out=s["y"])
        return (s["y"],)
    return fn, lambda seed: {"x": R(seed, 3, M, K), "y": R(seed, 4, M, pl.Np)}


def _forward_decode(N, K):
    from mlx8_ws_audio_transformer_amd import native_decoder as nd
    M = 3
    pl = nd.PackedLinear(R(7, 1, N, K, scale=0.1), None, backward=False)
    return lambda s: (pl.forward_decode(s["x"]),), lambda seed: {"x": R(seed, 2, M, K)}


case("packed_linear_forward_decode-200x64")(lambda: _forward_decode(200, 64))
case("packed_linear_forward_decode-32900x192")(lambda: _forward_decode(32900, 192))                     # the four-tile form


@case("packed_linear_backward_input")
def _():
    from mlx8_ws_audio_transformer_amd import native_decoder as nd
    M, N, K = 12, 256, 128
    pl = nd.PackedLinear(R(7, 1, N, K), R(7, 2, N))
    return lambda s: (pl.backward_input(s["dy"]),), lambda seed: {"dy": R(seed, 3, M, pl.Np)}


@case("packed_linear_update_forward")
def _():
    """A stepped weight re-packed into its handle and used, both inside the graph (awt_weight_update allocates nothing)."""
    from mlx8_ws_audio_transformer_amd import native_decoder as nd
    M, N, K = 12, 256, 128
    pl = nd.PackedLinear(Z(N, K), Z(N))

    def fn(s):
        pl.update(s["w"], s["b"])
        return (pl.forward(s["x"]),)
    return fn, lambda seed: {"w": R(seed, 1, N, K), "b": R(seed, 2, N), "x": R(seed, 3, M, K)}


@case("bmm")
def _():
    from mlx8_ws_audio_transformer_amd import native_decoder as nd
    batch, M, N, K = 5, 10, 64, 64
    pb = nd.PackedBatch(R(7, 1, batch, N, K))

    def fn(s):
        out = E(batch, M, N)
        nd.bmm((s["a"], 0, K, M * K), pb, M, (out, 0, N, M * N))
        return (out,)
    return fn, lambda seed: {"a": R(seed, 2, batch, M, K)}


@case("bmm_pack_update")
def _():
    """The B operands change with the state: packed into the existing buffer inside the graph, then multiplied, the result added to `out` in place."""
    from mlx8_ws_audio_transformer_amd import native_decoder as nd
    batch, M, N, K = 5, 10, 64, 64
    pb = nd.PackedBatch(Z(batch, N, K))

    def fn(s):
        pb.update(s["b"])
        nd.bmm((s["a"], 0, K, M * K), pb, M, (s["out"], 0, N, M * N), resid=(s["out"], 0, N, M * N))
        return (s["out"],)
    return fn, lambda seed: {"a": R(seed, 1, batch, M, K), "b": R(seed, 2, batch, N, K), "out": R(seed, 3, batch, M, N)}


@case("bmm_kmajor")
def _():
    """Both operands transposed in memory, each as two blocks stacked along K (the backward's d(enc) product); the pack is part of the graph."""
    from mlx8_ws_audio_transformer_amd import native_decoder as nd
    batch, M, N, K1, K2 = 2, 20, 64, 24, 24
    K = K1 + K2

    def fn(s):
        pb = nd.PackedBatch(kmajor=((s["b1"], 0), (s["b2"], 0), K1, N, K1 * N, batch, N, K))
        out = E(batch, M, N)
        nd.bmm(None, pb, M, (out, 0, N, M * N), a_kmajor=((s["a1"], 0), (s["a2"], 0), K1, M, K1 * M))
        return (out,)
    return fn, lambda seed: {"a1": R(seed, 1, batch, K1, M), "a2": R(seed, 2, batch, K2, M), "b1": R(seed, 3, batch, K1, N), "b2": R(seed, 4, batch, K2, N)}


@case("softmax_rows")
def _():
    from mlx8_ws_audio_transformer_amd import native_decoder as nd
    rows, cols, ld = 3, 70, 72
    return lambda s: (nd.softmax_rows(s["s"], cols, 0.125),), lambda seed: {"s": R(seed, 1, rows, ld, scale=8.0)}


@case("softmax_rows_backward")
def _():
    from mlx8_ws_audio_transformer_amd import native_decoder as nd
    rows, cols, ld = 3, 70, 72
    return (lambda s: (nd.softmax_rows_backward(s["p"], s["dp"], cols, 0.125),),
            lambda seed: {"p": torch.softmax(R(seed, 1, rows, ld), dim=-1), "dp": R(seed, 2, rows, ld)})


def _small_qkv(seed, B=2, H=2, L=12):
    return {"q": R(seed, 1, B * L, H * 64), "k": R(seed, 2, B * L, H * 64), "v": R(seed, 3, B * L, H * 64), "d_o": R(seed, 4, B * L, H * 64)}


def _attention_small(drop_p, backward):
    from mlx8_ws_audio_transformer_amd import native_decoder as nd
    B, H, L = 2, 2, 12
    d = H * 64

    def fn(s):
        q, k, v = (s["q"], 0), (s["k"], 0), (s["v"], 0)
        o, lse = nd.attention_small(q, d, k, d, v, d, B, H, L, L, True, 0, drop_p=drop_p, seed=5)
        if not backward:
            return o, lse
        dq, dk, dv = E(B * L, d), E(B * L, d), E(B * L, d)
        nd.attention_small_backward(q, d, k, d, v, d, o, s["d_o"], lse, (dq, 0), (dk, 0), (dv, 0), B, H, L, L, True, 0, drop_p=drop_p, seed=5)
        return dq, dk, dv
    return fn, _small_qkv


case("attention_small")(lambda: _attention_small(0.0, False))
case("attention_small-dropout")(lambda: _attention_small(0.25, False))
case("attention_small_backward")(lambda: _attention_small(0.0, True))
case("attention_small_backward-dropout")(lambda: _attention_small(0.25, True))


@case("attention_small_abi")
def _():
    """The pair without dropout has entry points of its own that no Python wrapper calls: through ctypes, as tests/test_gpu_small_attention.py does."""
    from mlx8_ws_audio_transformer_amd import _lib
    B, H, L = 2, 2, 12
    d = H * 64

    def fn(s):
        lib, ctx, stream = _lib.lib(), _lib.ctx(), _lib.stream_handle()
        o, lse, delta, dq, dk, dv = E(B * L, d), E(B, H, L), E(B, H, L), E(B * L, d), E(B * L, d), E(B * L, d)
        p = lambda t: t.data_ptr()
        _lib.check(lib.awt_op_attention_small(ctx, p(s["q"]), d, p(s["k"]), d, p(s["v"]), d, p(o), d, p(lse), B, H, L, L, 1, 0, stream))
        _lib.check(lib.awt_op_attention_small_backward(ctx, p(s["q"]), d, p(s["k"]), d, p(s["v"]), d, p(o), p(s["d_o"]), d, p(lse), p(delta), p(dq), p(dk), p(dv),
                                                       B, H, L, L, 1, 0, stream))
        return o, lse, delta, dq, dk, dv
    return fn, _small_qkv


@case("attention_cached")
def _():
    from mlx8_ws_audio_transformer_amd import native_decoder as nd
    rows, H, Lq, T, Tmax = 2, 6, 1, 65, 448
    d = H * 64
    return (lambda s: (nd.attention_cached((s["q"], 0), 3 * d, s["cache"], T, H, Lq),),
            lambda seed: {"q": R(seed, 1, rows * Lq, 3 * d), "cache": R(seed, 2, rows, Tmax, 2 * d)})


def _ids(seed, B, L, vocab):
    return torch.randint(0, vocab, (B, L), generator=torch.Generator().manual_seed(50 + seed)).cuda()


@case("embed")
def _():
    from mlx8_ws_audio_transformer_amd import native_decoder as nd
    B, L, vocab, d = 2, 6, 100, 64
    return (lambda s: (nd.embed(s["ids"], s["tok"], s["pos"], 2),),
            lambda seed: {"ids": _ids(seed, B, L, vocab), "tok": R(seed, 1, vocab, d), "pos": R(seed, 2, 16, d)})


@case("embed_backward")
def _():
    """Added to the two tables' gradients in place; an id is repeated so that a table row sums two terms."""
    from mlx8_ws_audio_transformer_amd import native_decoder as nd
    B, L, vocab, d = 2, 6, 100, 64

    def fn(s):
        nd.embed_backward(s["ids"], s["dx"], s["dtok"], s["dpos"], 2)
        return s["dtok"], s["dpos"]

    def make_state(seed):
        ids = _ids(seed, B, L, vocab)
        ids[1, 3] = ids[0, 1]
        return {"ids": ids, "dx": R(seed, 1, B * L, d), "dtok": R(seed, 2, vocab, d), "dpos": R(seed, 3, 16, d)}
    return fn, make_state


@case("gelu")
def _():
    from mlx8_ws_audio_transformer_amd import native_decoder as nd
    return lambda s: (nd.gelu(s["x"]),), lambda seed: {"x": R(seed, 1, 5, 384, scale=2.0)}


@case("gelu_backward")
def _():
    from mlx8_ws_audio_transformer_amd import native_decoder as nd
    return lambda s: (nd.gelu_backward(s["x"], s["dy"]),), lambda seed: {"x": R(seed, 1, 5, 384, scale=2.0), "dy": R(seed, 2, 5, 384)}


@case("layernorm_backward")
def _():
    from mlx8_ws_audio_transformer_amd import native_decoder as nd
    M, d = 5, 384
    return (lambda s: (nd.layernorm_backward(s["dy"], s["x"], s["g"], s["dres"]),),
            lambda seed: {"dy": R(seed, 1, M, d), "x": R(seed, 2, M, d), "g": 1 + 0.3 * R(seed, 3, d), "dres": R(seed, 4, M, d)})


@case("layernorm_param_grad")
def _():
    from mlx8_ws_audio_transformer_amd import native_decoder as nd
    M, d = 300, 384                                                                            # two slabs of rows
    return lambda s: tuple(nd.layernorm_param_grad(s["dy"], s["x"])), lambda seed: {"dy": R(seed, 1, M, d), "x": R(seed, 2, M, d)}


@case("column_sums")
def _():
    from mlx8_ws_audio_transformer_amd import native_decoder as nd
    return lambda s: (nd.column_sums(s["a"]),), lambda seed: {"a": R(seed, 1, 300, 384)}


@case("column_sums_ld")
def _():
    """A column block of a wider matrix, accumulated into `sums` in place."""
    from mlx8_ws_audio_transformer_amd import native_decoder as nd
    return (lambda s: (nd.column_sums_ld(s["a"], col=8, width=384, out=s["sums"], accumulate=True),),
            lambda seed: {"a": R(seed, 1, 300, 400), "sums": R(seed, 2, 384)})


@case("cross_entropy")
def _():
    """Device labels, one of them -100: the wrapper must not read them on the host."""
    from mlx8_ws_audio_transformer_amd import native_decoder as nd
    M, vocab, ld = 6, 100, 104

    def make_state(seed):
        labels = _ids(seed, 1, M, vocab).reshape(M)
        labels[2 + seed] = -100
        return {"logits": R(seed, 1, M, ld, scale=3.0), "labels": labels}
    return lambda s: tuple(nd.cross_entropy(s["logits"], s["labels"], vocab)), make_state


@case("kv_gather")
def _():
    """The B -> B x beams expansion, 3 rows to 15, with the parents on the device."""
    from mlx8_ws_audio_transformer_amd import native_decoder as nd
    layers, src_rows, dst_rows, Tmax, width, T = 3, 3, 15, 37, 1536, 29

    def fn(s):
        nd.kv_gather(s["src"], s["dst"], s["parent"], layers, src_rows, dst_rows, T, Tmax, width)
        return (s["dst"],)

    def make_state(seed):
        parent = (torch.arange(dst_rows, dtype=torch.int32) // 5 + seed) % src_rows
        return {"src": R(seed, 1, layers, src_rows, Tmax, width), "dst": R(seed, 2, layers, dst_rows, Tmax, width), "parent": parent.cuda()}
    return fn, make_state


# =================================================================================================================== generation.py
@case("select_tokens")
def _():
    from mlx8_ws_audio_transformer_amd import generation as G
    rows, vocab, beams = 5, 512, 5
    bits = G.banned_bits([3, 77, 300, 511], vocab, "cuda")
    return (lambda s: tuple(G.select_tokens(s["logits"], vocab, beams, bits, s["beam_scores"], True, 2 * beams)),
            lambda seed: {"logits": R(seed, 1, rows, vocab, scale=3.0), "beam_scores": R(seed, 2, rows, scale=2.0)})


@case("select_tokens_ts")
def _():
    """tests/test_gpu_timestamps.py's rows in mixed rule branches: 3 clips, greedy, six generated tokens; the token history is on the device."""
    from mlx8_ws_audio_transformer_amd import generation as G
    from tests.test_gpu_timestamps import EOS, LAYOUTS, _history
    vocab, rows, begin = 51865, 3, 4
    cur_len, no_ts, eos = begin + 6, LAYOUTS[51865], EOS[51865]
    ld = vocab + (-vocab) % 128
    bits = G.banned_bits([50358, 50359, 50360, 50361, 50362], vocab, "cuda")
    rules = G.TimestampRules(eos, no_ts, begin, None)

    def make_state(seed):
        g = torch.Generator().manual_seed(900 + seed)
        x = torch.randn((rows, ld), generator=g) * 3
        x[:, no_ts + 1:vocab] += torch.linspace(-2.0, 2.5, rows)[:, None]
        return {"logits": x.cuda(), "history": _history(rows, begin, cur_len, no_ts + 1, vocab, "mixed", g).cuda()}
    return lambda s: tuple(G.select_tokens(s["logits"], vocab, 1, bits, None, False, 1, rules=rules, history=s["history"], cur_len=cur_len)), make_state


@case("alignment_weights")
def _():
    from mlx8_ws_audio_transformer_amd import generation as G
    slots, rows, Tmax, d, nl, S, group, t0, T, frames = 2, 6, 12, 128, 3, 1500, 2, 2, 9, 604
    clips = rows // group
    table = torch.tensor([[0, 0, 1], [1, 2, 0], [1, 2, 1], [0, 0, 0]], dtype=torch.int32).cuda()
    src = torch.randint(0, rows, (clips, T), generator=torch.Generator().manual_seed(3), dtype=torch.int32).cuda()
    return (lambda s: (G.alignment_weights(s["q"], s["kv"], nl, S, table, clips, group, t0, T, frames, src),),
            lambda seed: {"q": R(seed, 1, slots, rows, Tmax, d), "kv": R(seed, 2, clips * S, 2 * nl * d)})


@case("alignment_matrix")
def _():
    """num_frames on the device; clip 0 has no more frames than half the filter width (unfiltered)."""
    from mlx8_ws_audio_transformer_amd import generation as G
    nf = torch.tensor([1, 8], dtype=torch.int32).cuda()
    return (lambda s: (G.alignment_matrix(s["w"], 3, nf),),
            lambda seed: {"w": torch.softmax(2.0 * R(seed, 1, 2, 2, 9, 1500), dim=-1)[..., :8].contiguous()})


@case("dtw")
def _():
    """A ragged batch with num_frames on the device.  The path arrays are written from path_start on only: the elements in front of it are masked (inside
    the graph) before anything is compared."""
    from mlx8_ws_audio_transformer_amd import generation as G
    clips, T, frames = 5, 30, 200
    nf = torch.tensor([200, 1, 77, 130, 2], dtype=torch.int32).cuda()
    col = torch.arange(T + frames, dtype=torch.int32).cuda()

    def fn(s):
        jump, text, time, start = G.dtw(s["m"], nf, negate=True)
        live = col[None, :] >= start[:, None]
        return jump, torch.where(live, text, -1), torch.where(live, time, -1), start
    return fn, lambda seed: {"m": R(seed, 1, clips, T, frames)}


# =================================================================================================================== the CNN classifiers' operators
def _conv_state(seed, B=2, T=13, cin=64, cout=128):
    return {"x": R(seed, 1, B * T, cin), "w": R(seed, 2, cout, cin, 3, scale=0.1), "b": R(seed, 3, cout), "dy": R(seed, 4, B * T, cout)}


@case("conv1d")
def _():
    from mlx8_ws_audio_transformer_amd import cnn_classifier as cc
    return lambda s: (cc.conv1d(s["x"], s["w"], s["b"], 2, 13),), _conv_state


@case("conv1d-fp16x3")
def _():
    from mlx8_ws_audio_transformer_amd import cnn_classifier as cc
    return lambda s: (cc.conv1d(s["x"], s["w"], s["b"], 2, 13, "fp16x3"),), _conv_state


@case("conv1d_input_grad")
def _():
    from mlx8_ws_audio_transformer_amd import cnn_classifier as cc
    return lambda s: (cc.conv1d_input_grad(s["dy"], s["w"], 2, 13),), _conv_state


@case("conv1d_weight_grad")
def _():
    from mlx8_ws_audio_transformer_amd import cnn_classifier as cc
    return lambda s: (cc.conv1d_weight_grad(s["dy"], s["x"], 2, 13),), _conv_state


def _bn_state(seed, B=3, T=13, C=128):
    return {"x": R(seed, 1, B * T, C), "g": 1 + 0.3 * R(seed, 2, C), "b": R(seed, 3, C), "dy": R(seed, 4, B * (T // 2), C)}


@case("batchnorm_stats")
def _():
    from mlx8_ws_audio_transformer_amd import cnn_classifier as cc
    return lambda s: tuple(cc.batchnorm_stats(s["x"])), _bn_state


@case("bn_relu_pool")
def _():
    from mlx8_ws_audio_transformer_amd import cnn_classifier as cc

    def fn(s):
        mean, var = cc.batchnorm_stats(s["x"])
        return (cc.bn_relu_pool(s["x"], mean, var, s["g"], s["b"], 1e-5, 3, 13, cc.POOL_MAX2),)
    return fn, _bn_state


@case("bn_relu_pool_backward")
def _():
    from mlx8_ws_audio_transformer_amd import cnn_classifier as cc

    def fn(s):
        mean, var = cc.batchnorm_stats(s["x"])
        return tuple(cc.bn_relu_pool_backward(s["dy"], s["x"], mean, var, s["g"], s["b"], 1e-5, 3, 13, cc.POOL_MAX2))
    return fn, _bn_state


def _framed(kernel, stride, cout, grad):
    from mlx8_ws_audio_transformer_amd import waveform_classifier as wc
    B, t1 = 1, 17
    n = kernel + (t1 - 1) * stride

    def fn(s):
        if grad:
            return (wc.conv1d_framed_weight_grad(s["dy"], s["x"], kernel, stride),)
        return (wc.conv1d_framed(s["x"], s["w"], s["b"], stride),)
    return fn, lambda seed: {"x": R(seed, 1, B, n), "w": R(seed, 2, cout, 1, kernel), "b": R(seed, 3, cout), "dy": R(seed, 4, B * t1, cout)}


# test_gpu_waveform_classifier.FRAMED_CONFIGS: the shortest kernel and the narrowest output
for _cfg in ((16, 16, 64), (32, 8, 32)):
    case("conv1d_framed" + ("" if _cfg[0] == 16 else "-32x8x32"))(functools.partial(_framed, *_cfg, False))
    case("conv1d_framed_weight_grad" + ("" if _cfg[0] == 16 else "-32x8x32"))(functools.partial(_framed, *_cfg, True))


# =================================================================================================================== front ends
def _pcm_i16(seed, n=64000):
    from mlx8_ws_audio_transformer_amd import synth
    return torch.from_numpy(synth.synth_clips_i16(2, seed=1234 + seed)[:, :n].copy()).cuda()


def _n_valid(seed):
    return torch.tensor([[64000, 40000], [50001, 64000]][seed], dtype=torch.int32).cuda()


@case("logmel_whisper_device")
def _():
    """int16, 2 clips, n_valid on the device, the trimmed 400 frames."""
    from mlx8_ws_audio_transformer_amd.feature_extraction import logmel_whisper_device
    return (lambda s: (logmel_whisper_device(s["pcm"], s["n_valid"], 64000, 400),),
            lambda seed: {"pcm": _pcm_i16(seed), "n_valid": _n_valid(seed)})


@case("logmel_whisper_abi")
def _():
    """awt_logmel_whisper, the 80-bin entry point that the wrappers no longer go through: by ctypes."""
    from mlx8_ws_audio_transformer_amd import _lib

    def fn(s):
        lib = _lib.lib()
        out, ws = E(2, 80, 400), _lib.workspace(lib.awt_logmel_workspace_bytes(2), "cuda")
        _lib.check(lib.awt_logmel_whisper(_lib.ctx(), s["pcm"].data_ptr(), 1, s["pcm"].stride(0), s["n_valid"].data_ptr(), 64000, 2, 400, out.data_ptr(),
                                          ws.data_ptr(), ws.numel(), _lib.stream_handle()))
        return (out,)
    return fn, lambda seed: {"pcm": _pcm_i16(seed), "n_valid": _n_valid(seed)}


@case("logmel_whisper_longest")
def _():
    from mlx8_ws_audio_transformer_amd.feature_extraction import logmel_whisper_longest
    n = 16000
    return (lambda s: (logmel_whisper_longest(s["pcm"], s["n_valid"]),),
            lambda seed: {"pcm": R(seed, 1, 2, n, scale=0.1), "n_valid": torch.tensor([[n, 9000], [12345, n]][seed], dtype=torch.int32).cuda()})


@case("mel_spectrogram_log")
def _():
    from mlx8_ws_audio_transformer_amd import urbansound
    return (lambda s: (urbansound.mel_spectrogram_log(s["w"], n_fft=1024, hop_length=512, n_mels=64),),
            lambda seed: {"w": R(seed, 1, 2, 8000, scale=0.1)})


@case("prepare_waveform")
def _():
    """Two channels at 44.1 kHz mixed down and resampled to 16 kHz; the polyphase taps are built by the first (eager) call."""
    from mlx8_ws_audio_transformer_amd import urbansound
    return (lambda s: (urbansound.prepare_waveform(s["w"], sample_rate=44100, n_out=8000),),
            lambda seed: {"w": R(seed, 1, 2, 22050, scale=0.1)})


# =================================================================================================================== composite passes
def _encoder(name, precision, **kw):
    from mlx8_ws_audio_transformer_amd import weights as wts
    from mlx8_ws_audio_transformer_amd.encoder import NativeWhisperEncoder
    cfg = wts.config(name, True)
    return cfg, NativeWhisperEncoder(cfg, precision=precision, seed=0, init_profile="test", **kw)


def _encode_pcm(precision):
    """`encode_pcm` as tests/test_gpu_encoder.py captures it, with the precision given: the automatic choice reads the device on the host and belongs to
    construction.  The weights are uploaded by the first eager call (awt_encoder_set_weight, which may synchronise)."""
    cfg, enc = _encoder("tiny", precision)
    enc.eval()
    return lambda s: (enc.encode_pcm(s["pcm"]),), lambda seed: {"pcm": _pcm_i16(seed)}


for _p in ("f16f8", "fp16x3", "bf16"):
    case("encode_pcm-" + _p)(functools.partial(_encode_pcm, _p))


@case("encoder_forward_mel")
def _():
    cfg, enc = _encoder("mini", "bf16x3")
    enc.eval()
    return (lambda s: (enc(s["mel"]).last_hidden_state,),
            lambda seed: {"mel": R(seed, 1, 2, cfg.n_mels, cfg.n_frames, scale=0.5)})


def _trainable_encoder(train_base):
    from mlx8_ws_audio_transformer_amd import weights as wts
    if train_base:
        cfg, enc = _encoder("mini", "bf16x3", trainable=True, train_base=True)
    else:
        cfg, enc = _encoder("mini", "bf16x3", trainable=True, lora=wts.LoraSpec(r=8, alpha=16.0, targets=("q_proj", "v_proj")))
        with torch.no_grad():
            for name, p in enc.named_parameters():
                if name.endswith("lora_B"):                                                    # zero at init: the A gradients would all be zero
                    p.copy_(torch.from_numpy(0.05 * wts.unit_variates(name, p.numel(), 2).reshape(p.shape).astype(np.float32)))
    return cfg, enc.train()


def _train_step(train_base):
    """zero_adapter_grads(), the training forward and the backward of (out * dout).sum() in one graph; the gradients land in the bound flat buffer."""
    cfg, enc = _trainable_encoder(train_base)
    flat = enc.bind_grad_buffer()

    def fn(s):
        enc.zero_adapter_grads()
        out = enc(s["mel"]).last_hidden_state
        (out * s["dout"]).sum().backward()
        return out.detach(), flat
    return fn, lambda seed: {"mel": R(seed, 1, 2, cfg.n_mels, cfg.n_frames, scale=0.5), "dout": R(seed, 2, 2, cfg.max_source_positions, cfg.d_model)}


case("encoder_train_step-lora")(lambda: _train_step(False))
case("encoder_train_step-train_base")(lambda: _train_step(True))


@case("encoder_backward_abi")
def _():
    """awt_encoder_backward, the entry point without flags (the module calls awt_encoder_backward_ex): forward_train and backward by ctypes."""
    from mlx8_ws_audio_transformer_amd import _lib
    cfg, enc = _trainable_encoder(False)
    enc.sync_weights()
    lib, B = _lib.lib(), 2
    n = enc.grad_count()

    def fn(s):
        saved = _lib.workspace(lib.awt_encoder_train_workspace_bytes(enc._handle, B), "cuda")
        out, grads = E(B, cfg.max_source_positions, cfg.d_model), E(n)
        _lib.check(lib.awt_encoder_forward_train(enc._handle, s["mel"].data_ptr(), B, cfg.n_frames, out.data_ptr(), saved.data_ptr(), saved.numel(),
                                                 _lib.stream_handle()))
        _lib.check(lib.awt_encoder_backward(enc._handle, s["dout"].data_ptr(), B, saved.data_ptr(), saved.numel(), grads.data_ptr(), n, _lib.stream_handle()))
        return out, grads
    return fn, lambda seed: {"mel": R(seed, 1, 2, cfg.n_mels, cfg.n_frames, scale=0.5), "dout": R(seed, 2, 2, cfg.max_source_positions, cfg.d_model)}


@functools.lru_cache(maxsize=None)
def _qwen3():
    """The smallest configuration of tests/test_gpu_qwen3_decoder.py."""
    from mlx8_ws_audio_transformer_amd.music2midi import Qwen3Decoder
    from tests import qwen3_reference as qr
    cfg = qr.config(qr.MICRO, True)
    dec = Qwen3Decoder(cfg)
    dec.load_state_dict({k: v.float() for k, v in qr.state_dict(cfg, seed=11).items()}, strict=True)
    return cfg, dec.cuda().eval()


def _qwen_cache(cfg, state, batch, tmax, length):
    """A Qwen3Cache over the state's tensors with `length` live positions."""
    from mlx8_ws_audio_transformer_amd.music2midi import Qwen3Cache
    cache = Qwen3Cache.__new__(Qwen3Cache)
    cache.batch, cache.max_length, cache.length = batch, tmax, length
    cache.k = [state[f"k{i}"] for i in range(cfg.num_hidden_layers)]
    cache.v = [state[f"v{i}"] for i in range(cfg.num_hidden_layers)]
    cache.ramp = torch.arange(tmax, dtype=torch.int32, device="cuda")
    return cache


def _qwen_state(cfg, B, tmax, seed, idx):
    st = {"x": R(seed, idx, B, 1, cfg.hidden_size)}
    for i in range(cfg.num_hidden_layers):
        st[f"k{i}"], st[f"v{i}"] = Z(B, tmax, cfg.num_key_value_heads * 128), Z(B, tmax, cfg.num_key_value_heads * 128)
    return st


@case("qwen3_prefill")
def _():
    cfg, dec = _qwen3()
    B, L, tmax = 2, 5, 8

    def fn(s):
        return (dec.prefill(s["x"], _qwen_cache(cfg, s, B, tmax, 0)),)                         # the cache tensors k[i], v[i] are state: rows 0 .. L - 1 are written

    def make_state(seed):
        st = _qwen_state(cfg, B, tmax, seed, 1)
        st["x"] = R(seed, 1, B, L, cfg.hidden_size)
        return st
    return fn, make_state


def _qwen_step(B):
    """One `step` at length t = 5 over a cache prefilled eagerly from the state's own prompt; B <= 8 takes the weight-streaming GEMV, B = 9 the GEMM.

    The host-side `cache.length` advances once, at capture: the graph holds a step at length t, and every replay rewrites position t of every layer's K and V.
    The eager reference for state B is a second cache: B's prompt prefilled, then B's token stepped.  Only the B cache's positions < t and B's token
    embedding are copied into the static tensors (position t is poisoned) before a replay; the logits and position t of every K and V must then equal the
    eager run, and every other position must be as it was."""
    cfg, dec = _qwen3()
    L, tmax = 5, 8

    def make_state(seed):
        st = _qwen_state(cfg, B, tmax, seed, 2)
        with torch.no_grad():
            dec.prefill(R(seed, 3, B, L, cfg.hidden_size), _qwen_cache(cfg, st, B, tmax, 0))
        return st

    def fn(s):
        return (dec.step(s["x"], _qwen_cache(cfg, s, B, tmax, L)),)

    def load(static, src):
        static["x"].copy_(src["x"])
        for k in static:
            if k != "x":
                static[k][:, :L].copy_(src[k][:, :L])
                static[k][:, L].fill_(float("nan"))
    return fn, make_state, load


for _b in (1, 3, 9):
    case(f"qwen3_step-B{_b}")(functools.partial(_qwen_step, _b))


# =================================================================================================================== the test
def test_every_covered_entry_point_names_a_case():
    assert set(COVERED.values()) <= set(CASES), sorted(set(COVERED.values()) - set(CASES))


@pytest.mark.parametrize("fault", ["output_unwritten", "stale_inputs", "ignores_inputs"])
def test_the_harness_refuses_what_it_exists_to_catch(fault):
    """Plain torch on the one stream, no library call: a function whose captured call (the fourth: eager A, eager B, warm-up, capture) does its work
    outside the graph's reach.  output_unwritten: the graph writes a scratch tensor only, the replay leaves the NaN pre-fill.  stale_inputs: the graph computes from a private
    copy of the inputs, so a replay returns state A's result.  ignores_inputs: the outputs never depended on the state."""
    calls, out, snapshot, scratch = [0], E(4, 8), E(4, 8), E(4, 8)

    def fn(s):
        calls[0] += 1
        captured = calls[0] == 4
        if fault == "ignores_inputs":
            return (torch.ones_like(s["x"]),)
        if fault == "stale_inputs":
            if not captured:
                snapshot.copy_(s["x"])
            torch.mul(snapshot, 2.0, out=out)
        else:
            torch.mul(s["x"], 2.0, out=scratch if captured else out)
        return (out,)
    with pytest.raises(AssertionError, match="cannot see a stale replay" if fault == "ignores_inputs" else "first replay: output 0 differs"):
        capture_replay(fn, lambda seed: {"x": R(seed, 1, 4, 8)})


@pytest.mark.parametrize("name", list(CASES))
def test_capture_replay(name):
    with torch.no_grad() if not name.startswith("encoder_train_step") else torch.enable_grad():
        capture_replay(*CASES[name]())
