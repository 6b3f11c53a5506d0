"""GPU parity of the full-parameter encoder backward (`train_base=True`: every base weight of the encoder trains, as in the reference's
fineTune.py) against torch autograd on the fp32 oracle, and of its hot path, the MFMA weight-gradient GEMM, against fp64."""
import numpy as np
import pytest
import torch

from mlx8_ws_audio_transformer_amd import weights as wts
from oracle import encoder as oracle_enc
from oracle import logmel as oracle_mel
from tests.util import MINI_LENGTHS, mini_at, piano_clips_f32

pytestmark = pytest.mark.gpu

FROZEN = "embed_positions.weight"


def _oracle_grads(W, mel, cfg, dout):
    Wt = {k: torch.from_numpy(v).clone().requires_grad_(k != FROZEN) for k, v in W.items()}
    out = oracle_enc.encoder_forward(Wt, mel, cfg.heads)
    (out * torch.from_numpy(dout)).sum().backward()
    return out.detach().numpy(), {k: v.grad.numpy() for k, v in Wt.items() if k != FROZEN}


def _klass(name):
    if name.startswith("conv"):
        return name
    leaf = name.split(".", 2)[2] if name.startswith("layers.") else name
    return leaf.replace("self_attn.", "")


def _dout(cfg, B, seed):
    S, d = cfg.max_source_positions, cfg.d_model
    return (wts.unit_variates("dout", B * S * d, seed).reshape(B, S, d) / np.sqrt(S)).astype(np.float32)


def _check_against_oracle(cfg, B, dout_seed, precision="bf16x3", out_atol=1e-3, bound=2e-3):
    from mlx8_ws_audio_transformer_amd.encoder import NativeWhisperEncoder
    W = wts.init_encoder_weights(cfg, 0, "test")
    mel = oracle_mel.whisper_logmel(piano_clips_f32(B), n_samples=cfg.n_frames * 160)
    dout = _dout(cfg, B, dout_seed)
    ref_out, ref_g = _oracle_grads(W, mel, cfg, dout)
    enc = NativeWhisperEncoder(cfg, precision=precision, trainable=True, train_base=True, seed=0, init_profile="test")
    enc.load_state_dict({k: torch.from_numpy(v) for k, v in W.items()})
    out = enc(torch.from_numpy(mel).cuda()).last_hidden_state
    assert out.requires_grad
    print("forward max-abs error", float(np.abs(out.detach().cpu().numpy() - ref_out).max()))
    np.testing.assert_allclose(out.detach().cpu().numpy(), ref_out, rtol=0, atol=out_atol)
    (out * torch.from_numpy(dout).cuda()).sum().backward()
    worst = {}
    for name, p in enc.named_parameters():
        if name == FROZEN:
            assert not p.requires_grad and p.grad is None
            continue
        assert p.requires_grad and p.grad is not None, name
        g_ref = ref_g[name]
        assert tuple(p.grad.shape) == g_ref.shape, name
        err = float(np.abs(p.grad.cpu().numpy() - g_ref).max() / max(np.abs(g_ref).max(), 1e-12))
        worst[_klass(name)] = max(worst.get(_klass(name), 0.0), err)
    assert set(ref_g) == {n for n, _ in enc.named_parameters()} - {FROZEN}
    for k in sorted(worst):
        print(f"worst relative gradient error  {k:32s} {worst[k]:.3e}")
    bad = {k: v for k, v in worst.items() if not v < bound}
    assert not bad, bad
    return worst


@pytest.mark.parametrize("name,trimmed", [("mini", True), ("mini", False), ("tiny", True), ("small", False)])
def test_base_gradients_match_oracle_autograd(name, trimmed):
    _check_against_oracle(wts.config(name, trimmed), 2, 3)


@pytest.mark.parametrize("S,B", MINI_LENGTHS)         # tests/util.py lists the branch each length takes
def test_base_gradients_at_other_sequence_lengths(S, B):
    _check_against_oracle(mini_at(S), B, 3)


def test_base_gradients_at_large_width():
    """d_model 1280 (Whisper large), truncated to two layers."""
    _check_against_oracle(wts.EncoderConfig(1280, 2, 20, 5120, 80, 200, "large-2layer-trimmed"), 1, 5)


def test_one_plane_forward_gives_every_base_gradient():
    """precision="bf16": one bf16 plane per activation (no lo planes anywhere in the pass: bias sums, GELU' planes, the conv stem's strided
    views), one product per fragment pair.  Operands carry 2^-9 instead of 2^-17, so the bounds are those the suite already keeps for the
    single-product modes: the forward inside the bf16 envelope of test_gpu_encoder.py (max-abs 8e-2; rel-L2 1.2e-2), and each parameter class
    within that forward envelope plus the 2e-2 upper edge of the bf16-backward band: 3.2e-2 of the gradient's largest element.  The lower
    edge shows that the single-product mode really ran."""
    worst = _check_against_oracle(wts.config("mini", True), 2, 3, precision="bf16", out_atol=8e-2, bound=3.2e-2)
    assert max(worst.values()) > 1e-5


def test_full_backward_is_reproducible_and_rejects_unsupported_configurations():
    from mlx8_ws_audio_transformer_amd.encoder import NativeWhisperEncoder
    cfg = wts.config("mini", True)
    with pytest.raises(ValueError):
        NativeWhisperEncoder(cfg, train_base=True)                                            # not a training encoder
    with pytest.raises(ValueError):
        NativeWhisperEncoder(cfg, trainable=True, train_base=True, lora=wts.LoraSpec(r=8, alpha=16.0, targets=("q_proj",)))   # adapters and base weights together
    with pytest.raises(ValueError):
        NativeWhisperEncoder(cfg, precision="bf16x3", trainable=True, train_base=True, backward_precision="f16f8")               # backward_terms = 5
    enc = NativeWhisperEncoder(cfg, precision="bf16x3", trainable=True, train_base=True, seed=0, init_profile="test")
    flat = enc.bind_grad_buffer()
    assert flat.numel() == sum(p.numel() for n, p in enc.named_parameters() if n != FROZEN)
    mel = torch.from_numpy(oracle_mel.whisper_logmel(piano_clips_f32(2), n_samples=cfg.n_frames * 160)).cuda()
    runs = []
    for _ in range(2):
        enc.zero_adapter_grads()
        enc(mel).last_hidden_state.square().mean().backward()
        runs.append(flat.clone())
    assert float(runs[0].abs().max()) > 0
    assert torch.equal(runs[0], runs[1])          # slab partials summed in a fixed order, no atomics
    for name, p in enc.named_parameters():        # every .grad is a view of the flat buffer, at the offset the library reports
        assert (p.grad is None) == (name == FROZEN)
    for name, off, shape in enc.base_grad_layout():
        g = enc.get_parameter(name).grad
        assert g.data_ptr() == flat.data_ptr() + 4 * off and tuple(g.shape) == shape, name
    # the library refuses the combinations as well
    from mlx8_ws_audio_transformer_amd import _lib
    import ctypes as C
    for lora_rank, bterms in ((8, 0), (0, 5)):
        c = _lib.EncoderCfg(cfg.d_model, cfg.layers, cfg.heads, cfg.ffn, cfg.n_mels, cfg.max_source_positions, 3, lora_rank, 16.0, 1 if lora_rank else 0, 0, 1, bterms, 1)
        out = C.c_void_p()
        assert _lib.lib().awt_encoder_create(_lib.ctx(torch.device("cuda:0")), C.byref(c), C.byref(out)) == -1
        assert b"train_base" in _lib.lib().awt_last_error()


def test_accumulate_and_gradient_scale_apply_to_base_gradients():
    from mlx8_ws_audio_transformer_amd import _lib
    from mlx8_ws_audio_transformer_amd.encoder import NativeWhisperEncoder
    cfg = wts.config("mini", True)
    enc = NativeWhisperEncoder(cfg, precision="bf16x3", trainable=True, train_base=True, seed=0, init_profile="test")
    flat = enc.bind_grad_buffer()
    mel = torch.from_numpy(oracle_mel.whisper_logmel(piano_clips_f32(2), n_samples=cfg.n_frames * 160)).cuda()
    enc(mel).last_hidden_state.square().mean().backward()
    once = flat.clone()
    enc(mel).last_hidden_state.square().mean().backward()          # second backward on a bound buffer: AWT_BWD_ACCUMULATE
    assert float((flat - 2 * once).abs().max()) <= 1e-6 * float(once.abs().max())
    enc.zero_adapter_grads()
    _lib.check(_lib.lib().awt_encoder_set_grad_scale_log2(enc._handle, 7))   # a power of two carried through the pass and divided out: same gradients
    enc(mel).last_hidden_state.square().mean().backward()
    assert float((flat - once).abs().max()) <= 2e-4 * float(once.abs().max())


def test_bf16_backward_option_of_the_full_backward():
    _check_bf16_backward_band(wts.config("tiny", True))


@pytest.mark.parametrize("S", [64, 128])          # the attention backward's last tile without a tail, on one product per fragment pair
def test_bf16_backward_option_at_other_sequence_lengths(S):
    _check_bf16_backward_band(mini_at(S))


def _check_bf16_backward_band(cfg):
    from mlx8_ws_audio_transformer_amd.encoder import NativeWhisperEncoder
    mel = torch.from_numpy(oracle_mel.whisper_logmel(piano_clips_f32(2), n_samples=cfg.n_frames * 160)).cuda()
    grads, outs = {}, {}
    for bp in (None, "bf16"):
        enc = NativeWhisperEncoder(cfg, precision="bf16x3", trainable=True, train_base=True, seed=0, init_profile="test", backward_precision=bp)
        out = enc(mel).last_hidden_state
        (out * out).sum().backward()
        outs[bp] = out.detach().clone()
        grads[bp] = {n: p.grad.detach().clone() for n, p in enc.named_parameters() if n != FROZEN}
    assert torch.equal(outs[None], outs["bf16"])
    cat = {bp: torch.cat([g.flatten() for g in grads[bp].values()]) for bp in grads}
    rel = float((cat["bf16"] - cat[None]).norm() / cat[None].norm())
    print("bf16 backward vs split-bf16 backward, relative L2:", rel)
    assert 1e-5 < rel < 2e-2, rel
    # the same band per parameter class: a wrong bias or LayerNorm gradient must not hide under the weight matrices
    num, den = {}, {}
    for n, g in grads[None].items():
        k = _klass(n)
        num[k] = num.get(k, 0.0) + float((grads["bf16"][n] - g).double().square().sum())
        den[k] = den.get(k, 0.0) + float(g.double().square().sum())
    for k in sorted(num):
        r = (num[k] / den[k]) ** 0.5
        print(f"bf16 backward band  {k:32s} {r:.3e}")
        if k.startswith("layer_norm."):          # the final LayerNorm's gradients are fp32 row reductions of d(hidden): no product of the backward enters
            assert r == 0.0, (k, r)
        else:
            assert 1e-5 < r < 2e-2, (k, r)


def _wg_case(M, N, K, ldy=None, ldx=None, ycol=0, xcol=0, seed=0, precision="bf16x3"):
    ldy, ldx = ldy or N, ldx or K
    dy = torch.from_numpy(wts.unit_variates("wg_dy", M * ldy, seed).reshape(M, ldy).astype(np.float32)).cuda()
    x = torch.from_numpy(wts.unit_variates("wg_x", M * ldx, seed + 1).reshape(M, ldx).astype(np.float32)).cuda()
    ref = dy[:, ycol: ycol + N].double().t() @ x[:, xcol: xcol + K].double()
    return dy, x, ref


@pytest.mark.parametrize("M,N,K", [(1000, 384, 384), (3001, 768, 768), (777, 1280, 384), (2500, 3072, 768), (1531, 768, 3072), (600, 5120, 1280), (600, 1280, 5120),
                                   (2999, 128, 80)])
def test_weight_grad_kernel_matches_fp64(M, N, K):
    from mlx8_ws_audio_transformer_amd import ops
    dy, x, ref = _wg_case(M, N, K)
    got = ops.weight_grad(dy, x)
    err = float((got.double() - ref).abs().max() / ref.abs().max())
    print(f"weight_grad M={M} N={N} K={K}: max rel err {err:.3e}")
    assert err < 2.0 ** -16, err                # split-bf16: each operand is carried to 2^-17, so a product to 2^-16 (the lo lo term is dropped); fp32 accumulation
    assert torch.equal(got, ops.weight_grad(dy, x))
    one = ops.weight_grad(dy, x, precision="bf16")
    err1 = float((one.double() - ref).abs().max() / ref.abs().max())
    assert 1e-5 < err1 < 2e-2, err1               # one bf16 product: 2^-9 per operand


def test_weight_grad_kernel_column_offsets_strides_scale_and_accumulate():
    from mlx8_ws_audio_transformer_amd import ops
    M, N, K = 1234, 256, 384
    dy, x, ref = _wg_case(M, N, K, ldy=3 * 256, ldx=1024, ycol=512, xcol=128, seed=4)
    got = ops.weight_grad(dy, x, n=N, k=K, ycol=512, xcol=128, scale=0.25)
    assert float((got.double() - 0.25 * ref).abs().max() / ref.abs().max()) < 2.0 ** -16
    base = torch.from_numpy(wts.unit_variates("wg_base", N * K * 3, 9).reshape(N, K, 3).astype(np.float32)).cuda()
    out = base.clone()
    ops.weight_grad(dy, x, n=N, k=K, ycol=512, xcol=128, out=out[:, :, 1], accumulate=True)      # a tap of a Conv1d weight: strides (3 K, 3)
    assert torch.equal(out[:, :, 0], base[:, :, 0]) and torch.equal(out[:, :, 2], base[:, :, 2])
    assert float((out[:, :, 1].double() - (base[:, :, 1].double() + ref)).abs().max() / ref.abs().max()) < 2.0 ** -16


@pytest.mark.parametrize("tap", [0, 1, 2])
def test_weight_grad_kernel_conv2_row_map(tap):
    """conv2's taps: contraction row (b, s) reads x row (b, 2 s + tap - 1), zero outside the clip's [0, T)."""
    from mlx8_ws_audio_transformer_amd import ops
    B, S, N, K = 3, 250, 384, 384
    T = 2 * S
    dy = torch.from_numpy(wts.unit_variates("wg_dy", B * S * N, 11).reshape(B * S, N).astype(np.float32)).cuda()
    x = torch.from_numpy(wts.unit_variates("wg_x", B * T * K, 12).reshape(B * T, K).astype(np.float32)).cuda()
    xp = torch.nn.functional.pad(x.view(B, T, K).double(), (0, 0, 1, 1))                  # rows -1 and T are zero
    xt = xp[:, tap: tap + T: 2, :].reshape(B * S, K)                                      # row 2 s + tap - 1
    ref = dy.double().t() @ xt
    got = ops.weight_grad(dy, x, row_map=(S, T, 2, tap - 1))
    assert float((got.double() - ref).abs().max() / ref.abs().max()) < 2.0 ** -16
