"""GPU: every entry point whose workspace is cut into several buffers stays inside exactly the bytes its query returns.

Per entry: the workspace is a byte tensor of `need + 4096` bytes filled with 0xA5, `need` from the entry's own query; the entry is called with
ws_bytes = need; the 4096 bytes past `need` must still be 0xA5 (a write past the end lands there and fails the assertion, it does not fault),
and the output must be bit-equal to the same call through the Python wrapper with its own workspace.  With ws_bytes = need - 1 the entry must
return AWT_ERR_WORKSPACE and leave the output alone.  Shapes are the smallest that leave a piece of the layout off a 256-byte multiple."""
import pytest
import torch

from mlx8_ws_audio_transformer_amd import _lib

pytestmark = pytest.mark.gpu

PAD, CANARY, ERR_WORKSPACE = 4096, 0xA5, -3


def _rand(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale).cuda()


def _exact(need, call, outs, want):
    """call(ws, ws_bytes, *outs) -> status.  `outs`: output tensors of the raw call, `want`: the wrapper's results for the same inputs."""
    need = int(need)
    assert need > 0
    ws = torch.full((need + PAD,), CANARY, dtype=torch.uint8, device="cuda")
    assert ws.data_ptr() % 256 == 0
    rc = call(ws, need, *outs)
    assert rc == 0, _lib.lib().awt_last_error()
    torch.cuda.synchronize()
    assert bool((ws[need:] == CANARY).all()), "the entry wrote past the size its query returns"
    for o, w in zip(outs, want):
        assert torch.equal(o, w)
    untouched = [torch.full_like(o, 7) for o in outs]
    assert call(ws, need - 1, *untouched) == ERR_WORKSPACE
    torch.cuda.synchronize()
    assert all(bool((u == 7).all()) for u in untouched)
    return ws


@pytest.mark.parametrize("precision", ["bf16x3", "fp16x3", "f16f8"])
def test_op_linear(precision):
    from mlx8_ws_audio_transformer_amd import ops
    M, N, K = 3, 128, 64                                     # x plane 384 bytes; N % 256 != 0: f16f8 clears its 16-row copies
    x, w, b = _rand((M, K), 1), _rand((N, K), 2, K ** -0.5), _rand((N,), 3)
    L, s = _lib.lib(), _lib.stream_handle()
    call = lambda ws, n, y: L.awt_op_linear(_lib.ctx(), _lib.ptr(x), _lib.ptr(w), _lib.ptr(b), _lib.ptr(y), M, N, K, ops._TERMS[precision], _lib.ptr(ws), n, s)
    _exact(L.awt_op_linear_workspace_bytes(M, N, K), call, [torch.empty(M, N, device="cuda")], [ops.linear(x, w, b, precision)])


@pytest.mark.parametrize("precision,form", [("bf16x3", "conv"), ("fp16x3", "lora"), ("f16f8", "lora"), ("f16f8", "conv")])
def test_op_linear_fused(precision, form):
    """The conv stem's three segments over x [B 2 S, Cin] and w [N, 3 Cin], and the LoRA form [x | u] [W | B]^T: x and w pieces of different sizes."""
    from mlx8_ws_audio_transformer_amd import ops
    if form == "conv":
        S, Cin, N = 3, 64, 128                               # x planes of 6 * 64 * 2 = 768 bytes
        x, w, M = _rand((2 * S, Cin), 1), _rand((N, 3 * Cin), 2, (3 * Cin) ** -0.5), S
        segs, kw = [(0, t * Cin, Cin, S, 2 * S, 2, t - 1) for t in range(3)], dict(pos=_rand((S, N), 4), rows_pos=S)
        epi = "gelu_pos"
    else:
        M, N, K = 3, 128, 64                                 # x planes of 3 * 128 * 2 = 768 bytes
        x, w = _rand((M, K + 64), 1), _rand((N, K + 64), 2, K ** -0.5)
        segs, kw, epi = [(0, 0, K, M, M, 1, 0), (K, K, 64, M, M, 1, 0)], dict(resid=_rand((M, N), 4)), "f32_resid"
    b = _rand((N,), 3)
    want = torch.empty(M, N, device="cuda")
    ops.linear_fused(x, w, b, epi, precision, {"f32": want}, M=M, segs=segs, **kw)

    def call(ws, n, y):
        try:
            ops.linear_fused(x, w, b, epi, precision, {"f32": y}, M=M, segs=segs, workspace=ws, ws_bytes=n, **kw)
        except _lib.AwtError as e:
            return e.code
        return 0
    _exact(ops.linear_fused_workspace_bytes(x.shape[0], x.shape[1], N, w.shape[1]), call, [torch.empty(M, N, device="cuda")], [want])


@pytest.mark.parametrize("precision", ["bf16x3", "f16f8"])
def test_op_attention(precision):
    from mlx8_ws_audio_transformer_amd import ops
    B, H, S = 1, 1, 129                                      # the smallest odd S of test_gpu_ops.test_attention: a plane of 16512 bytes
    q, k, v = _rand((B, H, S, 64), 1, 0.125), _rand((B, H, S, 64), 2), _rand((B, H, S, 64), 3)
    L, s = _lib.lib(), _lib.stream_handle()
    call = lambda ws, n, o: L.awt_op_attention(_lib.ctx(), _lib.ptr(q), _lib.ptr(k), _lib.ptr(v), _lib.ptr(o), B, H, S, ops._TERMS[precision], _lib.ptr(ws), n, s)
    _exact(L.awt_op_attention_workspace_bytes(B, H, S), call, [torch.empty(B, S, H * 64, device="cuda")], [ops.attention(q, k, v, precision)])


@pytest.mark.parametrize("precision,form", [("bf16x3", "planes"), ("fp16x3", "f32"), ("f16f8", "planes"), ("f16f8", "ilv")])
def test_op_attention_ex(precision, form):
    """f16f8 with lse2: the form that reads v's e4m3 images, every byte of the six planes in use; "ilv" without: v's images stay unwritten."""
    from mlx8_ws_audio_transformer_amd import ops
    B, H, S = 1, 1, 129                                      # as test_op_attention
    q, k, v = _rand((B, H, S, 64), 1, 0.125), _rand((B, H, S, 64), 2), _rand((B, H, S, 64), 3)
    if form == "f32":
        names, specs = ["f32", "lse2"], [((B, S, H * 64), torch.float32), ((B, H, S), torch.float32)]
    elif form == "ilv":
        names, specs = ["ilv"], [((B * S, H * 256), torch.uint8)]
    elif precision == "f16f8":
        names, specs = ["hi", "hi8", "lo8", "lse2"], [((B * S, H * 64), torch.float16), ((B * S, H * 64), torch.uint8), ((B * S, H * 64), torch.uint8), ((B, H, S), torch.float32)]
    else:
        names, specs = ["hi", "lo", "lse2"], [((B * S, H * 64), torch.bfloat16)] * 2 + [((B, H, S), torch.float32)]
    new = lambda: [torch.empty(shape, dtype=dt, device="cuda") for shape, dt in specs]
    want = new()
    ops.attention_ex(q, k, v, precision, dict(zip(names, want)))

    def call(ws, n, *outs):
        try:
            ops.attention_ex(q, k, v, precision, dict(zip(names, outs)), workspace=ws, ws_bytes=n)
        except _lib.AwtError as e:
            return e.code
        return 0
    _exact(ops.attention_ex_workspace_bytes(B, H, S), call, new(), want)


def test_op_attention_backward():
    from mlx8_ws_audio_transformer_amd import ops
    B, H, S = 1, 1, 129                                      # as test_op_attention: eight planes of 16512 bytes
    q, k, v, d_o = _rand((B, H, S, 64), 1, 0.125), _rand((B, H, S, 64), 2), _rand((B, H, S, 64), 3), _rand((B, S, H * 64), 4)
    L, s = _lib.lib(), _lib.stream_handle()
    call = lambda ws, n, *out: L.awt_op_attention_backward(_lib.ctx(), _lib.ptr(q), _lib.ptr(k), _lib.ptr(v), _lib.ptr(d_o), *(_lib.ptr(t) for t in out), B, H, S,
                                                           0.125, 3, 3, _lib.ptr(ws), n, s)
    want = ops.attention_backward_planes(q, k, v, d_o, "bf16x3", qscale=0.125)
    _exact(L.awt_op_attention_backward_workspace_bytes(B, H, S), call, [torch.empty_like(t) for t in want], list(want))


def test_linear_forward_and_backward_input():
    from mlx8_ws_audio_transformer_amd.native_decoder import PackedLinear
    L, s, M, N = _lib.lib(), _lib.stream_handle(), 3, 10
    pl = PackedLinear(_rand((N, 64), 1, 0.125), _rand((N,), 2))                       # x planes of 3 * 64 * 2 = 384 bytes
    x, r = _rand((M, 64), 3), _rand((M, pl.Np), 4)
    call = lambda ws, n, y: L.awt_linear_forward(_lib.ctx(), pl.handle, _lib.ptr(x), _lib.ptr(r), _lib.ptr(y), M, _lib.ptr(ws), n, s)
    _exact(L.awt_linear_workspace_bytes(pl.handle, M, 0), call, [torch.empty(M, pl.Np, device="cuda")], [pl.forward(x, resid=r)])
    pb = PackedLinear(_rand((N, 128), 5, 0.09), None)                                 # dy planes of 3 * 128 * 2 = 768 bytes: three whole 256-byte units
    dy = _rand((M, pb.Np), 6)
    call = lambda ws, n, dx: L.awt_linear_backward_input(_lib.ctx(), pb.handle, _lib.ptr(dy), _lib.ptr(dx), M, _lib.ptr(ws), n, s)
    _exact(L.awt_linear_workspace_bytes(pb.handle, M, 1), call, [torch.empty(M, 128, device="cuda")], [pb.backward_input(dy)])


@pytest.mark.parametrize("kmajor", [False, True])
def test_bmm_after_the_matching_pack(kmajor):
    from mlx8_ws_audio_transformer_amd import native_decoder as nd
    L, s, batch, M, N, K = _lib.lib(), _lib.stream_handle(), 1, 3, 4, 8               # A planes of 3 * 64 * 2 = 384 bytes
    a, b = _rand((batch, M, K), 1), _rand((batch, N, K), 2)
    at, bt = a.transpose(1, 2).contiguous(), b.transpose(1, 2).contiguous()           # [K, M], [K, N]: the operands as the k-major entries read them
    want = torch.full((batch, M, N), 7.0, device="cuda")
    if kmajor:
        pb = nd.PackedBatch(kmajor=((bt, 0), None, K, N, K * N, batch, N, K))
        nd.bmm(None, pb, M, (want, 0, N, M * N), a_kmajor=((at, 0), None, K, M, K * M))
        pack = lambda buf, n: L.awt_bmm_pack_kmajor(_lib.ctx(), _lib.ptr(bt), None, K, N, K * N, batch, N, K, _lib.ptr(buf), n, s)
        call = lambda ws, n, o: L.awt_bmm_kmajor(_lib.ctx(), _lib.ptr(at), None, K, M, K * M, _lib.ptr(packed), None, _lib.ptr(o), N, M * N, batch, M, N, K, _lib.ptr(ws), n, s)
    else:
        pb = nd.PackedBatch(b)
        nd.bmm((a, 0, K, M * K), pb, M, (want, 0, N, M * N))
        pack = lambda buf, n: L.awt_bmm_pack(_lib.ctx(), _lib.ptr(b), K, N * K, batch, N, K, _lib.ptr(buf), n, s)
        call = lambda ws, n, o: L.awt_bmm(_lib.ctx(), _lib.ptr(a), K, M * K, _lib.ptr(packed), None, _lib.ptr(o), N, M * N, batch, M, N, K, _lib.ptr(ws), n, s)
    need = int(L.awt_bmm_packed_bytes(batch, N, K))                                   # the packed buffer is a two-plane layout as well
    packed = torch.full((need + PAD,), CANARY, dtype=torch.uint8, device="cuda")
    assert pack(packed, need) == 0 and pack(packed, need - 1) == ERR_WORKSPACE
    assert bool((packed[need:] == CANARY).all()) and torch.equal(packed[:need], pb.buf[:need])
    _exact(L.awt_bmm_workspace_bytes(batch, M, K), call, [torch.empty(batch, M, N, device="cuda")], [want])


@pytest.mark.parametrize("row_map", [None, (2, 2, 1, -1)])
def test_op_weight_grad(row_map):
    from mlx8_ws_audio_transformer_amd import ops
    dy, x = _rand((4, 16), 1), _rand((4, 8), 2)              # dy planes 128 bytes, x planes 64 bytes; widths and pitches multiples of 8
    ro, ri, rm, ra = row_map or (0, 0, 1, 0)
    L, s = _lib.lib(), _lib.stream_handle()
    call = lambda ws, n, o: L.awt_op_weight_grad(_lib.ctx(), _lib.ptr(dy), 16, 0, 16, _lib.ptr(x), 4, 8, 0, 8, 4, ro, ri, rm, ra, 3, 1.0, 0, _lib.ptr(o), 8, 1,
                                                 _lib.ptr(ws), n, s)
    _exact(L.awt_op_weight_grad_workspace_bytes(4, 4, 16, 8, 16, 8), call, [torch.empty(16, 8, device="cuda")], [ops.weight_grad(dy, x, row_map=row_map)])


def test_op_conv1d():
    from mlx8_ws_audio_transformer_amd import cnn_classifier as cc
    B, T, Cin, Cout = 1, 3, 64, 128                          # x planes of 3 * 64 * 2 = 384 bytes
    x, w, b = _rand((B * T, Cin), 1), _rand((Cout, Cin, 3), 2, 0.07), _rand((Cout,), 3)
    L, s = _lib.lib(), _lib.stream_handle()
    call = lambda ws, n, y: L.awt_op_conv1d(_lib.ctx(), _lib.ptr(x), _lib.ptr(w), _lib.ptr(b), _lib.ptr(y), B, T, Cin, Cout, 3, 3, _lib.ptr(ws), n, s)
    _exact(L.awt_op_conv1d_workspace_bytes(B, T, Cin, Cout), call, [torch.empty(B * T, Cout, device="cuda")], [cc.conv1d(x, w, b, B, T)])


def test_audio_encode():
    from mlx8_ws_audio_transformer_amd import synth, weights as wts
    from mlx8_ws_audio_transformer_amd.encoder import NativeWhisperEncoder
    cfg = wts.config("tiny", True)
    enc = NativeWhisperEncoder(cfg, seed=0, init_profile="test").eval()               # default precision (f16f8), default chunk_clips
    pcm = torch.from_numpy(synth.synth_clips_i16(2, seed=1234, first=0)).cuda()
    want, want_feats = enc.encode_pcm(pcm, max_valid=64000, return_features=True)
    L, s, B = _lib.lib(), _lib.stream_handle(), 2
    call = lambda ws, n, feats, hidden: L.awt_audio_encode(enc._handle, _lib.ptr(pcm), 1, pcm.stride(0), None, 64000, B, _lib.ptr(feats), _lib.ptr(hidden),
                                                           _lib.ptr(ws), n, s)
    _exact(L.awt_audio_encode_workspace_bytes(enc._handle, B), call, [torch.empty_like(want_feats), torch.empty_like(want)], [want_feats, want])
    call = lambda ws, n, hidden: L.awt_audio_encode(enc._handle, _lib.ptr(pcm), 1, pcm.stride(0), None, 64000, B, None, _lib.ptr(hidden), _lib.ptr(ws), n, s)
    _exact(L.awt_audio_encode_workspace_bytes(enc._handle, B), call, [torch.empty_like(want)], [want])       # the mel features in the workspace's own buffer


def test_param_grad_reductions():
    """awt_op_layernorm_param_grad and awt_op_column_sums over two slabs (M = 300), d = 68: inside their workspace, the same bits on every call, and
    against torch in fp64 within the tolerances of tests/test_gpu_classifier.py::test_reduction_operators_match_torch."""
    import numpy as np
    M, d = 300, 68
    x, dy = _rand((M, d), 1, 3.0) + 1.0, _rand((M, d), 2)
    L, s = _lib.lib(), _lib.stream_handle()
    need = L.awt_op_param_grad_workspace_bytes(M, d)
    call = lambda ws, n, dg, db: L.awt_op_layernorm_param_grad(_lib.ctx(), _lib.ptr(dy), _lib.ptr(x), _lib.ptr(dg), _lib.ptr(db), M, d, 1e-5, _lib.ptr(ws), n, s)
    dg, db = torch.empty(d, device="cuda"), torch.empty(d, device="cuda")
    assert call(_lib.workspace(need, "cuda"), need, dg, db) == 0
    _exact(need, call, [torch.empty(d, device="cuda"), torch.empty(d, device="cuda")], [dg, db])
    g64, b64 = torch.ones(d, dtype=torch.float64, device="cuda", requires_grad=True), torch.zeros(d, dtype=torch.float64, device="cuda", requires_grad=True)
    torch.nn.functional.layer_norm(x.double(), (d,), g64, b64, 1e-5).backward(dy.double())
    np.testing.assert_allclose(dg.cpu().numpy(), g64.grad.float().cpu().numpy(), rtol=1e-4, atol=2e-4)
    np.testing.assert_allclose(db.cpu().numpy(), b64.grad.float().cpu().numpy(), rtol=1e-4, atol=2e-4)
    call = lambda ws, n, sums: L.awt_op_column_sums(_lib.ctx(), _lib.ptr(dy), _lib.ptr(sums), M, d, _lib.ptr(ws), n, s)
    sums = torch.empty(d, device="cuda")
    assert call(_lib.workspace(need, "cuda"), need, sums) == 0
    _exact(need, call, [torch.empty(d, device="cuda")], [sums])
    np.testing.assert_allclose(sums.cpu().numpy(), dy.double().sum(0).float().cpu().numpy(), rtol=2e-5, atol=2e-5)
