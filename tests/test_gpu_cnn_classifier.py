"""The UrbanSound CNN classifier on the native kernels (cnn_classifier.py, csrc/cnn_ops.hip) against torch on the CPU in fp64:
`F.conv1d`, `nn.BatchNorm1d`, `F.max_pool1d` and the torch.nn restatement of the layer list (tests/test_cnn_classifier_host.py)."""
import copy
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from mlx8_ws_audio_transformer_amd import _lib, weights as wts
from tests.test_cnn_classifier_host import restated_cnn

pytestmark = pytest.mark.gpu


def _uv(name, shape, seed=0):
    """float64 zero-mean unit-variance variates keyed by (name, seed)"""
    return torch.from_numpy(wts.unit_variates(name, int(np.prod(shape)), seed).reshape(shape))


def _rows(x):        # [B, C, T] -> channels-last rows [B T, C] on the device
    return x.transpose(1, 2).reshape(-1, x.shape[1]).float().contiguous().cuda()


def _unrows(y, B):   # [B T, C] -> [B, C, T] fp64 on the host
    return y.reshape(B, -1, y.shape[1]).transpose(1, 2).double().cpu()


def _close(got, want, rel, floor, what):
    """err <= rel * max|want| + floor, the form of the project's gradient bound (test_gpu_classifier.py)"""
    err, scale = float((got.double().cpu() - want).abs().max()), float(want.abs().max())
    assert err <= rel * scale + floor, (what, err, scale)


# ---------------------------------------------------------------------------------------------------------------- 1. conv1d
CONV_SHAPES = [(2, 13, 64, 128), (1, 1, 512, 512), (2, 63, 256, 512), (3, 126, 128, 256)]


@pytest.mark.parametrize("B,T,cin,cout", CONV_SHAPES)
def test_conv1d_matches_f_conv1d_forward_and_gradients(B, T, cin, cout):
    """bf16x3 carries 2^-17 per operand: 2e-4 of the largest output (the project's GEMM bound) covers the K = 3 Cin products."""
    from mlx8_ws_audio_transformer_amd import cnn_classifier as cc
    x, w, b = _uv("cnn.conv.x", (B, cin, T), T).float(), (_uv("cnn.conv.w", (cout, cin, 3), cin) * (3 * cin) ** -0.5).float(), _uv("cnn.conv.b", (cout,)).float()
    dy = _uv("cnn.conv.dy", (B, cout, T), T).float()
    x64, w64, b64 = (t.double().requires_grad_(True) for t in (x, w, b))
    want = F.conv1d(x64, w64, b64, padding=1)
    want.backward(dy.double())
    got = cc.conv1d(_rows(x), w.cuda(), b.cuda(), B, T)
    _close(_unrows(got, B), want.detach(), 2e-4, 1e-7, "y")
    _close(_unrows(cc.conv1d_input_grad(_rows(dy), w.cuda(), B, T), B), x64.grad, 2e-4, 1e-7, "dx (flipped weight)")
    _close(cc.conv1d_weight_grad(_rows(dy), _rows(x), B, T), w64.grad, 2e-4, 1e-7, "dw")
    xg, wg, bg = _rows(x).requires_grad_(True), w.cuda().requires_grad_(True), b.cuda().requires_grad_(True)       # the autograd node: the same three
    cc._Conv1d.apply(xg, wg, bg, B, T, "bf16x3").backward(_rows(dy))
    _close(_unrows(xg.grad, B), x64.grad, 2e-4, 1e-7, "x.grad")
    _close(wg.grad, w64.grad, 2e-4, 1e-7, "w.grad")
    _close(bg.grad, b64.grad, 2e-4, 1e-7, "b.grad")


@pytest.mark.parametrize("B,T,cin,cout", CONV_SHAPES)
def test_conv1d_forward_in_split_fp16(B, T, cin, cout):
    """The forward's operand format, fp16 hi + lo planes: 2^-23 per operand, and the fp32 accumulation of K = 3 Cin <= 1536 products
    (sqrt(K) eps = 2.3e-6 of the largest term): 2e-5 of the largest output, a tenth of the bf16x3 bound."""
    from mlx8_ws_audio_transformer_amd import cnn_classifier as cc
    x, w, b = _uv("cnn.conv.x", (B, cin, T), T).float(), (_uv("cnn.conv.w", (cout, cin, 3), cin) * (3 * cin) ** -0.5).float(), _uv("cnn.conv.b", (cout,)).float()
    want = F.conv1d(x.double(), w.double(), b.double(), padding=1)
    _close(_unrows(cc.conv1d(_rows(x), w.cuda(), b.cuda(), B, T, "fp16x3"), B), want, 2e-5, 1e-7, "y")


@pytest.mark.parametrize("precision", ["bf16", "bf16x3", "fp16x3"])
def test_conv1d_does_not_read_across_clips(precision):
    """Clip 0 large, clip 1 all zeros: clip 1's output is the bias EXACTLY (products with zero are zero in every operand plane)."""
    from mlx8_ws_audio_transformer_amd import cnn_classifier as cc
    B, T, cin, cout = 2, 13, 64, 128
    x = torch.zeros(B, cin, T)
    x[0] = 1e4 * _uv("cnn.iso.x", (cin, T)).float()
    w, b = _uv("cnn.iso.w", (cout, cin, 3)).float(), _uv("cnn.iso.b", (cout,)).float()
    got = cc.conv1d(_rows(x), w.cuda(), b.cuda(), B, T, precision).cpu().reshape(B, T, cout)
    assert torch.equal(got[1], b.expand(T, cout))
    assert float(got[0].abs().max()) > 1e4
    x2 = torch.zeros(3, cin, 5); x2[1] = x[0, :, :5]          # a zero clip on either side
    got = cc.conv1d(_rows(x2), w.cuda(), b.cuda(), 3, 5, precision).cpu().reshape(3, 5, cout)
    assert torch.equal(got[0], b.expand(5, cout)) and torch.equal(got[2], b.expand(5, cout))


# ---------------------------------------------------------------------------------------------------------------- 2. BatchNorm + ReLU + pooling
BN_CASES = [(B, T, C, 2) for T in (2, 13, 31, 63, 126) for C in (128, 512) for B in (1, 3)] + \
           [(B, T, C, 0) for T in (1, 15) for C in (128, 512) for B in (1, 3) if (B, T) != (1, 1)]
KINK = 1e-5      # margin around the kinks of relu / max within which fp32 and fp64 may take different branches


def _bn_inputs(B, T, C):
    x = (_uv("cnn.bn.x", (B, C, T), 7 * T + B) * 3.0 + 1.0).float()
    x[:, 5, :] = 1.7                                       # a constant channel: var = 0, rstd = eps^-1/2
    gamma, beta = (1.0 + 0.3 * _uv("cnn.bn.g", (C,))).float(), (0.3 * _uv("cnn.bn.b", (C,))).float()
    return x, gamma, beta


def _bn_reference(x, gamma, beta, pool, dy, steps=1):
    bn = torch.nn.BatchNorm1d(x.shape[1]).double().train()
    with torch.no_grad():
        bn.weight.copy_(gamma); bn.bias.copy_(beta)
    x64 = x.double().requires_grad_(True)
    for _ in range(steps):
        z = bn(x64)
    y = F.max_pool1d(F.relu(z), 2, 2) if pool == 2 else F.relu(z).mean(-1, keepdim=True)
    y.backward(dy.double())
    return bn, x64, z.detach(), y.detach()


EPS32 = 2.0 ** -24


def _bn_bounds(x, gamma, z, dy, ref_dx, ref_dg, ref_db, pool, T):
    """Per-channel bounds of the fp32 BatchNorm kernels against fp64, from the number format and the reference alone.
    * Sums over M = B T <= 378 rows: M eps = 2.3e-5 bounds a reduction's rounding relative to its largest term -> 5e-5.
    * Conditioning: fp32 rounds x - mean to eps |x|, which rstd magnifies: xhat carries an ABSOLUTE error of about 2 eps kappa with
      kappa = max|x| rstd (2 for an ordinary channel, hundreds when M = 2 and the two values nearly agree), and rstd itself a relative one of
      eps kappa.  Hence rel = 5e-5 + 8 eps kappa.
    * dx = gamma rstd (dz - dbeta / M - xhat dgamma / M) cancels (for M = 2 down to eps / (var + eps) of its terms), so its error is relative
      to the TERMS, gamma rstd max|dz|, where that exceeds the result; likewise dgamma and dbeta relative to max|dz| (max|dz| max|xhat|).
    Returns (keep, tol_y, tol_dx, tol_dg, tol_db): `keep` drops the channels in which the fp64 reference comes within KINK of a kink of
    relu / max (|z| or |z_a - z_b| < 1e-5, exact ties apart), where fp32 may legitimately take the other branch."""
    var = x.double().var((0, 2), unbiased=False)
    rstd = (var + 1e-5).rsqrt()
    kappa = x.double().abs().amax((0, 2)) * rstd
    rel = 5e-5 + 8 * EPS32 * kappa
    xhat_max = ((x.double() - x.double().mean((0, 2), keepdim=True)) * rstd[None, :, None]).abs().amax((0, 2))
    gmax = dy.double().abs().amax((0, 2)) / (1 if pool == 2 else T)
    near = (z.abs() < KINK).any(-1).any(0)
    if pool == 2:
        d = (z[..., 0:2 * (T // 2):2] - z[..., 1:2 * (T // 2):2]).abs()
        near |= ((d < KINK) & (d != 0)).any(-1).any(0)
    g = gamma.double().abs()
    tol_y = 2e-5 + 16 * EPS32 * kappa * g                                  # + rtol 2e-5 of the value
    tol_dx = rel * torch.maximum(ref_dx.abs().amax((0, 2)), g * rstd * gmax) + 1e-6
    tol_dg = rel * torch.maximum(ref_dg.abs(), gmax * xhat_max.clamp(min=1.0)) + 1e-6
    tol_db = rel * torch.maximum(ref_db.abs(), gmax) + 1e-6
    return ~near, tol_y, tol_dx, tol_dg, tol_db


def _bn_compare(bounds, want_y, want_dx, want_dg, want_db, got_y, got_dx, got_dg, got_db, C):
    keep, tol_y, tol_dx, tol_dg, tol_db = bounds
    assert int((~keep).sum()) <= max(1, C // 50), int((~keep).sum())
    ey = ((got_y - want_y).abs() - 2e-5 * want_y.abs()).amax((0, 2))
    assert not (ey > tol_y).any(), ("y", float((ey / tol_y).max()))
    for name, a, w, tol in (("dx", got_dx, want_dx, tol_dx), ("dgamma", got_dg[None, :, None], want_dg[None, :, None], tol_dg),
                            ("dbeta", got_db[None, :, None], want_db[None, :, None], tol_db)):
        err = (a - w).abs().amax((0, 2))
        bad = keep & (err > tol)
        assert not bad.any(), (name, int(bad.sum()), float((err / tol)[bad].max()))


@pytest.mark.parametrize("B,T,C,pool", BN_CASES)
def test_batchnorm_relu_pool_matches_torch_autograd(B, T, C, pool):
    """Statistics, forward and backward of the fp32 kernels against nn.BatchNorm1d + relu + pooling under fp64 autograd; bounds: `_bn_bounds`."""
    from mlx8_ws_audio_transformer_amd import cnn_classifier as cc
    x, gamma, beta = _bn_inputs(B, T, C)
    dy = _uv("cnn.bn.dy", (B, C, T // 2 if pool == 2 else 1), T).float()
    ref, x64, z, want = _bn_reference(x, gamma, beta, pool, dy, steps=1)
    xr = _rows(x)
    mean, var = cc.batchnorm_stats(xr)
    want_mean, want_var = x.double().mean((0, 2)), x.double().var((0, 2), unbiased=False)
    np.testing.assert_allclose(mean.cpu().numpy(), want_mean.numpy(), rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(var.cpu().numpy(), want_var.numpy(), rtol=2e-5 + 4 * EPS32 * float((x.abs().amax((0, 2)) / want_var.sqrt().clamp(min=1e-3)).max()), atol=1e-9)
    assert float(var[5]) == 0.0 and float(mean[5]) == float(torch.tensor(1.7))
    g, b = gamma.cuda(), beta.cuda()
    got = cc.bn_relu_pool(xr, mean, var, g, b, 1e-5, B, T, pool)
    dx, dg, db = cc.bn_relu_pool_backward(_rows(dy), xr, mean, var, g, b, 1e-5, B, T, pool)
    assert torch.isfinite(got).all() and torch.isfinite(dx).all()
    bounds = _bn_bounds(x, gamma, z, dy, x64.grad, ref.weight.grad, ref.bias.grad, pool, T)
    _bn_compare(bounds, want, x64.grad, ref.weight.grad, ref.bias.grad, _unrows(got, B), _unrows(dx, B), dg.double().cpu(), db.double().cpu(), C)


@pytest.mark.parametrize("B,T,C,pool", [(3, 13, 128, 2), (1, 15, 512, 0)])
def test_running_statistics_after_two_steps(B, T, C, pool):
    from mlx8_ws_audio_transformer_amd import cnn_classifier as cc
    x, gamma, beta = _bn_inputs(B, T, C)
    ref, _, _, want = _bn_reference(x, gamma, beta, pool, torch.zeros(B, C, T // 2 if pool == 2 else 1), steps=2)
    bn = torch.nn.BatchNorm1d(C).cuda().train()
    with torch.no_grad():
        bn.weight.copy_(gamma); bn.bias.copy_(beta)
    for _ in range(2):
        got = cc.batchnorm_relu_pool(bn, _rows(x), B, T, pool)
    assert int(bn.num_batches_tracked) == 2 == int(ref.num_batches_tracked)
    np.testing.assert_allclose(bn.running_mean.cpu().numpy(), ref.running_mean.numpy(), rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(bn.running_var.cpu().numpy(), ref.running_var.numpy(), rtol=2e-5, atol=1e-7)      # the UNBIASED batch variance
    np.testing.assert_allclose(_unrows(got.detach(), B).numpy(), want.numpy(), rtol=2e-5, atol=2e-5)
    bn.eval()                                                # eval(): the running statistics through the same kernel, buffers untouched
    got = cc.batchnorm_relu_pool(bn, _rows(x), B, T, pool)
    z = F.relu(ref.eval()(x.double()))
    want = F.max_pool1d(z, 2, 2) if pool == 2 else z.mean(-1, keepdim=True)
    np.testing.assert_allclose(_unrows(got, B).numpy(), want.detach().numpy(), rtol=2e-5, atol=2e-5)
    assert int(bn.num_batches_tracked) == 2


def test_single_value_per_channel_raises_in_train_mode():
    from mlx8_ws_audio_transformer_amd import cnn_classifier as cc
    bn = torch.nn.BatchNorm1d(128).cuda().train()
    with pytest.raises(ValueError, match="more than 1 value per channel"):
        cc.batchnorm_relu_pool(bn, torch.zeros(1, 128).cuda(), 1, 1, 0)
    with pytest.raises(ValueError, match="more than 1 value per channel"):          # torch's own behaviour
        torch.nn.BatchNorm1d(128).train()(torch.zeros(1, 128, 1))
    assert tuple(cc.batchnorm_relu_pool(bn.eval(), torch.zeros(1, 128).cuda(), 1, 1, 0).shape) == (1, 128)


# ---------------------------------------------------------------------------------------------------------------- whole model
def _reference(n_mels, seed, dropout=0.0, n_classes=10):
    """The restatement in fp32 on the CPU with every parameter and buffer non-trivial, perturbed as test_gpu_classifier._pair does."""
    torch.manual_seed(seed)
    ref = restated_cnn(n_classes, n_mels, dropout)
    with torch.no_grad():
        for name, p in ref.named_parameters():
            u = _uv("cnn." + name, p.shape, seed).float()
            is_bn = p.dim() == 1 and name.startswith("conv_layers") and int(name.split(".")[1]) % 5 == 1
            p.copy_(1.0 + 0.1 * u if is_bn and name.endswith("weight") else (p + 0.05 * u if p.dim() > 1 else 0.1 * u))
        for name, buf in ref.named_buffers():
            u = _uv("cnn." + name, buf.shape, seed).float()
            if name.endswith("running_mean"):
                buf.copy_(0.3 * u)
            elif name.endswith("running_var"):
                buf.copy_(1.0 + 0.4 * u.abs())
            else:
                buf.fill_(3)
    return ref


def _pair(n_mels, seed, dropout=0.0, n_classes=10):
    """(fp64 restatement on the CPU, native model on the GPU); both hold the same fp32 values."""
    from mlx8_ws_audio_transformer_amd import CNNUrbanSound8KClassifier
    ref = _reference(n_mels, seed, dropout, n_classes)
    nat = CNNUrbanSound8KClassifier(n_classes=n_classes, n_mels=n_mels, dropout=dropout)
    assert not any(nat.load_state_dict(ref.state_dict(), strict=True))
    return ref.double(), nat.cuda()


def _mel(name, B, n_mels, T, seed=3):
    return (_uv(name, (B, n_mels, T), seed) * 2.0 - 4.0).float()


def _ref_features(ref, x):
    return ref.conv_layers(x).flatten(1)


@pytest.mark.parametrize("n_mels,T,batch", [(64, 126, 3), (80, 126, 2), (128, 501, 2)])
def test_eval_logits_and_embeddings_match_restated_module(n_mels, T, batch):
    ref, nat = _pair(n_mels, seed=n_mels + T)
    ref.eval(); nat.eval()
    x = _mel("cnn.x", batch, n_mels, T)
    with torch.no_grad():
        want_f, want = _ref_features(ref, x.double()), ref.classifier(ref.conv_layers(x.double()))
    got_f, got = nat.get_feature_embeddings(x.cuda()).cpu(), nat(x.cuda()).cpu()
    assert tuple(got.shape) == (batch, 10) and tuple(got_f.shape) == (batch, 512) and not got.requires_grad
    np.testing.assert_allclose(got_f.numpy(), want_f.numpy(), rtol=0, atol=1e-3)
    np.testing.assert_allclose(got.numpy(), want.numpy(), rtol=0, atol=1e-3)
    assert torch.equal(got.argmax(-1), want.argmax(-1))
    assert all(int(b) == 3 for n, b in nat.named_buffers() if n.endswith("num_batches_tracked"))        # eval() leaves the buffers alone


# Largest |fp32 - fp64| of the torch restatement on the CPU for the inputs of the training-step test, per tensor (the loss first), measured with
# tools/cnn_fp32_vs_fp64.py; keyed by (n_mels, T, batch).  BatchNorm's backward subtracts two near-equal sums, so fp32 itself
# is this far from fp64; the bound of a tensor is max(2e-4 max|grad| + 1e-7, 8 x this) -- 8 because bf16x3 products carry about 3 fewer bits
# than fp32.  The table is filled from the reference alone, never from the native output.
FP32_VS_FP64 = {
    (64, 126, 4): {"loss": 5.52e-10, "conv_layers.0.weight": 6.74e-08, "conv_layers.0.bias": 9.16e-09, "conv_layers.1.weight": 1.36e-08,
        "conv_layers.1.bias": 7.02e-09, "conv_layers.5.weight": 2.06e-08, "conv_layers.5.bias": 8.33e-09, "conv_layers.6.weight": 7.45e-09,
        "conv_layers.6.bias": 4.12e-09, "conv_layers.10.weight": 9.02e-09, "conv_layers.10.bias": 4.34e-09, "conv_layers.11.weight": 6.10e-09,
        "conv_layers.11.bias": 2.33e-09, "conv_layers.15.weight": 7.56e-09, "conv_layers.15.bias": 2.12e-09, "conv_layers.16.weight": 5.95e-09,
        "conv_layers.16.bias": 4.38e-09, "classifier.1.weight": 2.32e-08, "classifier.1.bias": 9.46e-09, "classifier.4.weight": 2.75e-08,
        "classifier.4.bias": 5.88e-09, "classifier.7.weight": 8.94e-08, "classifier.7.bias": 1.77e-08},
    (128, 501, 2): {"loss": 4.52e-08, "conv_layers.0.weight": 1.19e-07, "conv_layers.0.bias": 1.28e-08, "conv_layers.1.weight": 8.34e-09,
        "conv_layers.1.bias": 7.91e-09, "conv_layers.5.weight": 3.15e-08, "conv_layers.5.bias": 1.41e-08, "conv_layers.6.weight": 5.23e-09,
        "conv_layers.6.bias": 2.97e-09, "conv_layers.10.weight": 1.08e-08, "conv_layers.10.bias": 5.29e-09, "conv_layers.11.weight": 3.74e-09,
        "conv_layers.11.bias": 1.95e-09, "conv_layers.15.weight": 7.02e-09, "conv_layers.15.bias": 4.50e-09, "conv_layers.16.weight": 9.82e-09,
        "conv_layers.16.bias": 7.45e-09, "classifier.1.weight": 1.92e-08, "classifier.1.bias": 1.32e-08, "classifier.4.weight": 3.13e-08,
        "classifier.4.bias": 1.10e-08, "classifier.7.weight": 1.23e-07, "classifier.7.bias": 1.44e-08},
}


def _step_bounds(key, ref_grads):
    table = FP32_VS_FP64[key]
    return {n: max(2e-4 * float(g.abs().max()) + 1e-7, 8.0 * table[n]) for n, g in ref_grads.items()}


def _labels(batch):
    return torch.tensor([(3 * i + 1) % 10 for i in range(batch)])


def _train_step_reference(ref, x, y):
    ref.train()
    loss = F.cross_entropy(ref.classifier(ref.conv_layers(x.double())), y)
    loss.backward()
    return loss.detach(), {n: p.grad for n, p in ref.named_parameters()}


@pytest.mark.parametrize("n_mels,T,batch", [(64, 126, 4), (128, 501, 2)])
def test_training_step_matches_autograd_of_the_restated_module(n_mels, T, batch):
    """One train() forward + backward with dropout 0: the loss (within 1e-4), the gradient of EVERY parameter (bounds: `_step_bounds`), the
    updated running buffers and counters, against fp64 autograd over the restated module.  Every figure is printed before it is judged.

    relu' and the arg-max of the pooling are discontinuous in the conv outputs, so the comparison also tests the conv FORWARD's operand format:
    with bf16x3 forwards (2^-17 per operand; `forward_precision="bf16x3"`) the (128, 501, 2) case puts one decision of the third block on the
    other side of its kink than fp64 and the gradients up to that block miss their bounds by two orders (conv_layers.5.weight 1.05e-3 against
    2.9e-6, measured on an MI355X and reproduced on the CPU by rounding the conv operands alone).  The model's default, split-fp16 forwards
    (2^-23 per operand, same three products), is what is tested here; the bounds are those of `_step_bounds`, unchanged."""
    from mlx8_ws_audio_transformer_amd.autograd_ops import native_cross_entropy
    ref, nat = _pair(n_mels, seed=7 + T)
    x, y = _mel("cnn.xt", batch, n_mels, T, 5), _labels(batch)
    want_loss, want = _train_step_reference(ref, x, y)
    nat.train()
    got_loss = native_cross_entropy(nat(x.cuda()), y.cuda())
    got_loss.backward()
    bounds = _step_bounds((n_mels, T, batch), want)
    print(f"loss: native {float(got_loss.detach()):.7f} fp64 {float(want_loss):.7f}")
    failures = []
    if abs(float(got_loss.detach()) - float(want_loss)) >= max(1e-4, 8.0 * FP32_VS_FP64[(n_mels, T, batch)]["loss"]):
        failures.append("loss")
    params = dict(nat.named_parameters())
    assert set(params) == set(want)
    for name, w in want.items():
        assert params[name].grad is not None, name
        err = float((params[name].grad.double().cpu() - w).abs().max())
        print(f"{name}: err {err:.3e} bound {bounds[name]:.3e} max|grad| {float(w.abs().max()):.3e}")
        if not err <= bounds[name]:
            failures.append((name, err, bounds[name]))
    want_buf, got_buf = dict(ref.named_buffers()), dict(nat.named_buffers())
    for name, w in want_buf.items():
        if name.endswith("num_batches_tracked"):
            assert int(got_buf[name]) == int(w) == 4, name
        else:
            _close(got_buf[name], w, 2e-4, 1e-7, name)
    assert not failures, failures


# ---------------------------------------------------------------------------------------------------------------- 5. state
def test_eval_after_training_uses_the_updated_parameters_and_deepcopy_works():
    """Two `train_cnn` steps, then eval(): the logits are those of the restatement after the same two Adam steps -- a packed weight or folded
    BatchNorm kept from before the steps would show.  Bound: the eval bound 1e-3 plus what Adam's sign-like first steps (each weight moves by
    about lr whatever the gradient's size) make of gradient differences: elements whose gradient is below the gradient tolerance may move the
    other way, 2 lr each per step; with lr = 1e-3 that is a few 1e-3 on a handful of the 1.5 M weights: 5e-3 in all.  The steps themselves move
    the logits by far more (asserted), so a stale copy cannot pass."""
    from mlx8_ws_audio_transformer_amd import train_cnn
    ref, nat = _pair(64, seed=21)
    x, y = _mel("cnn.xs", 4, 64, 32, 2), _labels(4)
    xe = _mel("cnn.xe", 3, 64, 32, 4)
    before = nat.eval()(xe.cuda()).cpu()
    again = copy.deepcopy(nat)
    assert torch.equal(again(xe.cuda()).cpu(), before) and torch.equal(nat(xe.cuda()).cpu(), before)       # both copies run, bit-identical
    opt = torch.optim.Adam(ref.parameters(), lr=1e-3, weight_decay=1e-4)
    ref.train()
    for _ in range(2):
        opt.zero_grad()
        F.cross_entropy(ref.classifier(ref.conv_layers(x.double())), y).backward()
        opt.step()
    nat, losses = train_cnn([(x, y), (x, y)], model=nat, epochs=1, lr=1e-3, weight_decay=1e-4)
    assert len(losses) == 1 and nat.training
    with torch.no_grad():
        want = ref.eval().classifier(ref.conv_layers(xe.double()))
    got = nat.eval()(xe.cuda()).cpu()
    assert float((want - before.double()).abs().max()) > 5e-2
    np.testing.assert_allclose(got.numpy(), want.numpy(), rtol=0, atol=5e-3)
    assert torch.equal(again(xe.cuda()).cpu(), before)        # the copy made before training kept its own parameters
    assert torch.equal(copy.deepcopy(nat)(xe.cuda()).cpu(), got)


# ---------------------------------------------------------------------------------------------------------------- 6. train_cnn
def _toy(n_mels=64, T=16, per_class=2):
    """Class c = the mel band [6 c, 6 c + 6) carries energy."""
    B = 10 * per_class
    y = torch.arange(B) % 10
    x = -4.0 + 0.2 * _uv("cnn.toy", (B, n_mels, T)).float()
    for i in range(B):
        x[i, 6 * int(y[i]): 6 * int(y[i]) + 6] += 3.0
    return x, y


def test_train_cnn_learns_a_separable_toy_problem():
    from mlx8_ws_audio_transformer_amd import CNNUrbanSound8KClassifier, eval_or_test_cnn, train_cnn
    torch.manual_seed(0)
    x, y = _toy()
    model = CNNUrbanSound8KClassifier(n_mels=64, dropout=0.1).cuda()
    logs = []
    model, losses = train_cnn([(x, y)] * 6, model=model, epochs=4, lr=1e-3, weight_decay=1e-4, log=logs.append)
    assert len(losses) == 4 == len(logs) and losses[-1] < 0.5 * losses[0] and losses[0] < 2.5
    preds = eval_or_test_cnn(model, [(x, y)])
    assert not model.training and preds == y.tolist()
    assert eval_or_test_cnn(model, [x[:7], x[7:]]) == y.tolist()           # batches without labels, any split


def test_one_adam_step_with_weight_decay_matches_the_restated_module():
    """After ONE `train_cnn` batch the weights equal a torch Adam(weight_decay) step on the restatement.  Adam's first step moves a weight
    by lr g / (|g| + 1e-8) with g = grad + wd w: where |g| exceeds twice the training-step test's gradient bound both sides agree on g's
    sign and the moved weights agree to rounding (1e-2 lr); elements below that are noise for Adam and are not compared."""
    from mlx8_ws_audio_transformer_amd import train_cnn
    n_mels, T, batch, lr, wd = 64, 126, 4, 1e-3, 1e-4
    ref, nat = _pair(n_mels, seed=7 + T)
    x, y = _mel("cnn.xt", batch, n_mels, T, 5), _labels(batch)
    before = {n: p.detach().clone() for n, p in ref.named_parameters()}
    opt = torch.optim.Adam(ref.parameters(), lr=lr, weight_decay=wd)
    _, grads = _train_step_reference(ref, x, y)
    opt.step()
    train_cnn([(x, y)], model=nat, epochs=1, lr=lr, weight_decay=wd)
    bounds = _step_bounds((n_mels, T, batch), grads)
    failures = []
    for name, p in nat.named_parameters():
        g = (grads[name] + wd * before[name]).abs()
        live = g > 2.0 * bounds[name]
        assert live.any(), name
        diff = (p.detach().double().cpu() - dict(ref.named_parameters())[name].detach()).abs()[live]
        if float(diff.max()) > 1e-2 * lr:
            failures.append((name, float(diff.max()), int((diff > 1e-2 * lr).sum()), int(live.sum())))
    assert not failures, failures


# ---------------------------------------------------------------------------------------------------------------- 7. determinism, dropout
def test_training_is_bit_reproducible_and_dropout_follows_the_seed():
    from mlx8_ws_audio_transformer_amd.autograd_ops import native_cross_entropy
    _, nat = _pair(64, seed=5)
    x, y = _mel("cnn.xd", 3, 64, 63, 6).cuda(), _labels(3).cuda()
    nat.train()
    runs = []
    for _ in range(2):
        nat.zero_grad()
        native_cross_entropy(nat(x), y).backward()
        runs.append({n: p.grad.clone() for n, p in nat.named_parameters()})
    assert all(torch.equal(runs[0][n], runs[1][n]) for n in runs[0])
    _, drop = _pair(64, seed=5, dropout=0.3)
    drop.train()
    outs = []
    for seed in (1, 1, 2):
        torch.manual_seed(seed)
        outs.append(drop(x).detach().clone())
    assert torch.equal(outs[0], outs[1]) and not torch.equal(outs[0], outs[2])


# ---------------------------------------------------------------------------------------------------------------- 8. errors
def test_bad_arguments_return_a_status_and_launch_nothing():
    """Through ctypes on device buffers, as test_gpu_errors.py: a negative status, awt_last_error set, the output untouched."""
    L, c = _lib.lib(), _lib.ctx()
    t = torch.zeros(1 << 16, device="cuda")
    y = torch.full((1 << 16,), 7.0, device="cuda")
    ws = _lib.workspace(1 << 22, t.device)
    p, s = t.data_ptr(), _lib.stream_handle()
    err = lambda: L.awt_last_error().decode()
    assert L.awt_op_conv1d(c, p, p, p, y.data_ptr(), 2, 13, 64, 128, 5, 3, ws.data_ptr(), ws.numel(), s) == -1 and "taps must be 3" in err()
    assert L.awt_op_conv1d(c, p, p, p, y.data_ptr(), 2, 13, 64, 128, 3, 3, ws.data_ptr(), 4096, s) == -3 and "workspace too small" in err()
    assert L.awt_op_conv1d(c, p, p, p, y.data_ptr(), 2, 13, 62, 128, 3, 3, ws.data_ptr(), ws.numel(), s) == -1 and "multiple of 4" in err()
    assert L.awt_op_batchnorm_stats(c, p, 26, 126, y.data_ptr(), y.data_ptr() + 1024, ws.data_ptr(), ws.numel(), s) == -1 and "multiple of 4" in err()
    assert L.awt_op_batchnorm_stats(c, p, 260, 128, y.data_ptr(), y.data_ptr() + 1024, ws.data_ptr(), 16, s) == -3 and "workspace too small" in err()
    assert L.awt_op_bn_relu_pool(c, p, p, p, p, p, ctypes.c_float(1e-5), y.data_ptr(), 2, 13, 126, 2, s) == -1 and "multiple of 4" in err()
    assert L.awt_op_bn_relu_pool_backward(c, p, p, p, p, p, p, ctypes.c_float(1e-5), y.data_ptr(), y.data_ptr() + 4096, y.data_ptr() + 8192, 2, 13, 126, 2,
                                          ws.data_ptr(), ws.numel(), s) == -1 and "multiple of 4" in err()
    assert L.awt_op_bn_relu_pool_backward(c, p, p, p, p, p, p, ctypes.c_float(1e-5), y.data_ptr(), y.data_ptr() + 4096, y.data_ptr() + 8192, 2, 13, 128, 2,
                                          ws.data_ptr(), 16, s) == -3 and "workspace too small" in err()
    torch.cuda.synchronize()
    assert bool((y == 7.0).all())
