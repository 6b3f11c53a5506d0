"""`CNNUrbanSound8KClassifier` with `train_cnn` / `eval_or_test_cnn` (the reference's UrbanSound8K script, spectrogram.py:442-660: its default
model) on libawt, inference and training.

The layer list, with the reference's `nn.Sequential` indices so that a checkpoint written by its `train_cnn` loads with
`load_state_dict(strict=True)`:

    conv_layers   0 Conv1d(n_mels, 128, 3, padding 1)   1 BatchNorm1d   2 ReLU   3 MaxPool1d(2, 2)   4 Dropout
                  5 Conv1d(128, 256)  6 BN  7 ReLU  8 MaxPool  9 Dropout     10 Conv1d(256, 512)  11 BN  12 ReLU  13 MaxPool  14 Dropout
                  15 Conv1d(512, 512)  16 BN  17 ReLU  18 AdaptiveAvgPool1d(1)
    classifier    0 Flatten   1 Linear(512, 256)  2 ReLU  3 Dropout   4 Linear(256, 128)  5 ReLU  6 Dropout   7 Linear(128, n_classes)

The modules in the two containers hold the parameters and buffers only; `forward` does not call them.  The input [B, n_mels, T] is transposed
once to channels-last rows [B T, C], which every operator below reads and writes:
  * Conv1d: `awt_op_conv1d` -- one MFMA GEMM launch of three row-mapped K segments, one per tap (forward in split fp16, `forward_precision`;
    gradients in `precision`, bf16x3: they need fp32's exponent range); its input gradient is the same call on dy
    with the tap-flipped, channel-transposed weight, its weight gradient `awt_op_weight_grad` once per tap straight into the
    [Cout, Cin, 3] gradient, its bias gradient `awt_op_column_sums`;
  * BatchNorm1d + ReLU + pooling: `awt_op_batchnorm_stats` (train) then `awt_op_bn_relu_pool`, and `awt_op_bn_relu_pool_backward`, which
    recomputes the ReLU mask and the pooling winner from the saved conv output; eval() feeds the running statistics to the same kernel;
  * head: `autograd_ops.Linear` (MFMA GEMM forward and both gradients); loss: `autograd_ops.native_cross_entropy` (inside `train_epoch`).
The running statistics are updated with torch ops on the [C] vectors; ReLU in the head and the five Dropouts are element-wise torch ops under
autograd, as in the Transformer classifier.  There is no torch fallback for conv, BatchNorm or pooling: without libawt the first call raises.
Nothing is cached between calls (the conv weights are packed per call, like `awt_op_linear`'s), so there is no state that a parameter update
or a `copy.deepcopy` could leave stale.  `CNNWaveformClassifier` (spectrogram.py:664-697) is built from the same operators in
waveform_classifier.py.
"""
from __future__ import annotations

from typing import Optional

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _lib, native_decoder as nd, ops
from .autograd_ops import Linear, native_linear, train_epoch
from .urbansound import N_MELS

CNN_DROPOUT, CNN_LR, CNN_WEIGHT_DECAY = 0.3, 3e-4, 1e-4       # spectrogram.py:65-67
CNN_CHANNELS = (128, 256, 512, 512)
HEAD_WIDTHS = (256, 128)
_TERMS = frozenset(("bf16", "bf16x3"))                        # names of ops._TERMS a gradient GEMM takes
_FORWARD_TERMS = _TERMS | {"fp16x3"}                          # ... and a conv forward
POOL_MEAN, POOL_MAX2, POOL_MAX4, POOL_MAX4_MEAN = 0, 2, 4, 5  # include/awt.h AWT_POOL_*
_POOL_WINDOW = {POOL_MEAN: 0, POOL_MAX2: 2, POOL_MAX4: 4, POOL_MAX4_MEAN: 4}


def _terms(precision: str) -> int:
    if precision not in _TERMS:
        raise ValueError("the CNN's GEMMs run in 'bf16' or 'bf16x3' operand planes (gradients need fp32's exponent range)")
    return ops._TERMS[precision]


def _forward_terms(precision: str) -> int:
    if precision not in _FORWARD_TERMS:
        raise ValueError("a conv forward runs in 'bf16', 'bf16x3' or 'fp16x3' operand planes")
    return ops._TERMS[precision]


# ------------------------------------------------------------------------------------------------ operators (no autograd)
def conv1d(x: torch.Tensor, w: torch.Tensor, b: Optional[torch.Tensor], B: int, T: int, precision: str = "bf16x3") -> torch.Tensor:
    """`F.conv1d(padding=1)` on channels-last rows: x [B T, Cin], w [Cout, Cin, 3] -> [B T, Cout] (`awt_op_conv1d`).  Cin is zero-padded
    to a multiple of 64 and Cout to a multiple of 128, the GEMM's K and N multiples.  precision "fp16x3" (fp16 hi + lo planes: 22 bits per
    operand against bf16x3's 16, same three products) is for operands inside fp16's range, i.e. the forward, not gradients."""
    terms = _forward_terms(precision)
    cout, cin, taps = w.shape
    if x.shape != (B * T, cin):
        raise ValueError(f"conv1d: x must be [{B * T}, {cin}], got {tuple(x.shape)}")
    kp, npad = ops.pad_to(cin, 64), ops.pad_to(cout, 128)
    x, w = x.float(), w.float()
    if kp != cin:
        x, w = F.pad(x, (0, kp - cin)), F.pad(w, (0, 0, 0, kp - cin))
    if npad != cout:
        w = F.pad(w, (0, 0, 0, 0, 0, npad - cout))
        b = F.pad(b, (0, npad - cout)) if b is not None else None
    x, w = x.contiguous(), w.contiguous()
    b = b.float().contiguous() if b is not None else None
    L = _lib.lib()
    y = torch.empty((B * T, npad), dtype=torch.float32, device=x.device)
    ws = _lib.workspace(L.awt_op_conv1d_workspace_bytes(B, T, kp, npad), x.device)
    with torch.cuda.device(x.device):
        _lib.check(L.awt_op_conv1d(_lib.ctx(x.device), _lib.ptr(x), _lib.ptr(w), _lib.ptr(b), _lib.ptr(y), B, T, kp, npad, taps, terms,
                                   _lib.ptr(ws), ws.numel(), _lib.stream_handle()))
    return y if npad == cout else y[:, :cout].contiguous()


def conv1d_input_grad(dy: torch.Tensor, w: torch.Tensor, B: int, T: int, precision: str = "bf16x3") -> torch.Tensor:
    """dx of `conv1d`: the same operator on dy [B T, Cout] with w'[ci, co, tap] = w[co, ci, 2 - tap]."""
    return conv1d(dy, w.permute(1, 0, 2).flip(2), None, B, T, precision)


def conv1d_weight_grad(dy: torch.Tensor, x: torch.Tensor, B: int, T: int, precision: str = "bf16x3") -> torch.Tensor:
    """dW [Cout, Cin, 3] of `conv1d`: per tap, dW[:, :, tap] = dy^T x[frame + tap - 1] on the weight-gradient GEMM under the conv's row map,
    written through the gradient's strides (3 Cin, 3) at the tap's offset."""
    cin = x.shape[1]
    kp = ops.pad_to(cin, 8)                 # the weight-gradient GEMM takes widths and pitches in multiples of 8
    if kp != cin:
        x = F.pad(x, (0, kp - cin))
    dw = torch.empty((dy.shape[1], kp, 3), dtype=torch.float32, device=dy.device)
    for tap in range(3):
        ops.weight_grad(dy, x, precision=precision, out=dw[:, :, tap], row_map=(T, T, 1, tap - 1))
    return dw if kp == cin else dw[:, :cin].contiguous()


def _check_rows(x: torch.Tensor, B: int, T: int) -> int:
    C = x.shape[1]
    if x.dim() != 2 or x.shape[0] != B * T or C % 4:
        raise ValueError(f"expected channels-last rows [{B * T}, C] with C a multiple of 4, got {tuple(x.shape)}")
    return C


def batchnorm_stats(x: torch.Tensor):
    """Per-channel mean and biased variance of x [M, C] (`awt_op_batchnorm_stats`)."""
    M, C = x.shape
    mean, var = torch.empty(C, dtype=torch.float32, device=x.device), torch.empty(C, dtype=torch.float32, device=x.device)
    L = _lib.lib()
    ws = _lib.workspace(L.awt_op_batchnorm_stats_workspace_bytes(M, C), x.device)
    with torch.cuda.device(x.device):
        _lib.check(L.awt_op_batchnorm_stats(_lib.ctx(x.device), _lib.ptr(x), M, C, _lib.ptr(mean), _lib.ptr(var), _lib.ptr(ws), ws.numel(),
                                            _lib.stream_handle()))
    return mean, var


def bn_relu_pool(x: torch.Tensor, mean: torch.Tensor, var: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, eps: float, B: int, T: int,
                 pool: int) -> torch.Tensor:
    """pool(relu(batch_norm(x))) of x [B T, C] in one pass (`awt_op_bn_relu_pool`): POOL_MAX2 / POOL_MAX4 -> [B (T // 2), C] / [B (T // 4), C],
    POOL_MEAN (the mean over T) and POOL_MAX4_MEAN (the mean over the T // 4 pooled frames) -> [B, C]."""
    C = _check_rows(x, B, T)
    y = torch.empty((B * (T // pool) if pool in (POOL_MAX2, POOL_MAX4) else B, C), dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        _lib.check(_lib.lib().awt_op_bn_relu_pool(_lib.ctx(x.device), _lib.ptr(x), _lib.ptr(mean), _lib.ptr(var), _lib.ptr(gamma), _lib.ptr(beta),
                                                  float(eps), _lib.ptr(y), B, T, C, pool, _lib.stream_handle()))
    return y


def bn_relu_pool_backward(dy: torch.Tensor, x: torch.Tensor, mean: torch.Tensor, var: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor,
                          eps: float, B: int, T: int, pool: int):
    """(dx, dgamma, dbeta) of `bn_relu_pool` under the batch statistics of x (`awt_op_bn_relu_pool_backward`)."""
    C = _check_rows(x, B, T)
    dx, dg, db = torch.empty_like(x), torch.empty_like(gamma), torch.empty_like(beta)
    L = _lib.lib()
    ws = _lib.workspace(L.awt_op_bn_relu_pool_backward_workspace_bytes(B, T, C), x.device)
    with torch.cuda.device(x.device):
        _lib.check(L.awt_op_bn_relu_pool_backward(_lib.ctx(x.device), _lib.ptr(dy), _lib.ptr(x), _lib.ptr(mean), _lib.ptr(var), _lib.ptr(gamma),
                                                  _lib.ptr(beta), float(eps), _lib.ptr(dx), _lib.ptr(dg), _lib.ptr(db), B, T, C, pool,
                                                  _lib.ptr(ws), ws.numel(), _lib.stream_handle()))
    return dx, dg, db


# ------------------------------------------------------------------------------------------------ trainable operators
class _Conv1d(torch.autograd.Function):
    """y [B T, Cout] = conv1d(x [B T, Cin], w [Cout, Cin, 3]) + b with all three gradients on libawt."""

    @staticmethod
    def forward(ctx, x, w, b, B, T, precision, forward_precision=None):
        ctx.save_for_backward(x, w)
        ctx.shape, ctx.precision = (B, T), precision
        _terms(precision)
        return conv1d(x, w, b, B, T, forward_precision or precision)

    @staticmethod
    def backward(ctx, dy):
        x, w = ctx.saved_tensors
        B, T = ctx.shape
        dy = dy.contiguous()
        dx = conv1d_input_grad(dy, w, B, T, ctx.precision) if ctx.needs_input_grad[0] else None
        return dx, conv1d_weight_grad(dy, x, B, T, ctx.precision), nd.column_sums(dy), None, None, None, None


class _BnReluPool(torch.autograd.Function):
    """Training-mode BatchNorm1d + ReLU + pooling of x [B T, C]; also returns the batch mean and biased variance (not differentiable) for
    the running statistics."""

    @staticmethod
    def forward(ctx, x, gamma, beta, eps, B, T, pool):
        mean, var = batchnorm_stats(x)
        ctx.save_for_backward(x, gamma, beta, mean, var)
        ctx.cfg = (eps, B, T, pool)
        ctx.mark_non_differentiable(mean, var)
        return bn_relu_pool(x, mean, var, gamma, beta, eps, B, T, pool), mean, var

    @staticmethod
    def backward(ctx, dy, _dmean, _dvar):
        x, gamma, beta, mean, var = ctx.saved_tensors
        eps, B, T, pool = ctx.cfg
        dx, dg, db = bn_relu_pool_backward(dy.contiguous(), x, mean, var, gamma, beta, eps, B, T, pool)
        return dx, dg, db, None, None, None, None


def batchnorm_relu_pool(bn: nn.BatchNorm1d, x: torch.Tensor, B: int, T: int, pool: int) -> torch.Tensor:
    """`pool(relu(bn(x)))` for a `nn.BatchNorm1d` holding the parameters and buffers: in train() on the batch statistics (updating
    `running_mean`, `running_var` -- with the unbiased variance -- and `num_batches_tracked` as the module does), in eval() on the running ones."""
    if pool not in _POOL_WINDOW:
        raise ValueError(f"pool must be one of {sorted(_POOL_WINDOW)} (POOL_MEAN, POOL_MAX2, POOL_MAX4, POOL_MAX4_MEAN)")
    if T < _POOL_WINDOW[pool]:
        raise ValueError(f"MaxPool1d({_POOL_WINDOW[pool]}) needs at least {_POOL_WINDOW[pool]} frames")
    x = x.contiguous()
    if not (bn.training or not bn.track_running_stats):
        return bn_relu_pool(x, bn.running_mean, bn.running_var, bn.weight.detach(), bn.bias.detach(), bn.eps, B, T, pool)
    M = B * T
    if M <= 1:
        raise ValueError(f"Expected more than 1 value per channel when training, got input size [{B}, {x.shape[1]}, {T}]")   # as nn.BatchNorm1d
    y, mean, var = _BnReluPool.apply(x, bn.weight, bn.bias, bn.eps, B, T, pool)
    if bn.track_running_stats:
        with torch.no_grad():
            bn.num_batches_tracked += 1
            m = bn.momentum if bn.momentum is not None else 1.0 / float(bn.num_batches_tracked)
            bn.running_mean.mul_(1.0 - m).add_(mean, alpha=m)
            bn.running_var.mul_(1.0 - m).add_(var, alpha=m * M / (M - 1))
    return y


# ------------------------------------------------------------------------------------------------ the model
class CNNUrbanSound8KClassifier(nn.Module):
    def __init__(self, n_classes: int = 10, n_mels: int = N_MELS, dropout: float = CNN_DROPOUT, precision: str = "bf16x3",
                 forward_precision: str = "fp16x3"):
        """precision: operand planes of the gradient GEMMs and of the head.  forward_precision: those of the four conv forwards, train() and
        eval().  BatchNorm + ReLU + max-pool after a conv are discontinuous in its output, so the conv's last bits decide masks and pooling
        winners; log-mel inputs, post-BatchNorm activations and weights lie inside fp16's range, where the fp16 pair carries 22 bits per
        operand against the bf16 pair's 16 at the same three MFMA products.  Pass "bf16x3" for inputs beyond +-65504."""
        super().__init__()
        _terms(precision)
        _forward_terms(forward_precision)
        self.n_mels, self.precision, self.forward_precision = n_mels, precision, forward_precision
        layers, cin = [], n_mels
        for i, cout in enumerate(CNN_CHANNELS):
            last = i == len(CNN_CHANNELS) - 1
            layers += [nn.Conv1d(cin, cout, kernel_size=3, padding=1), nn.BatchNorm1d(cout), nn.ReLU()]
            layers += [nn.AdaptiveAvgPool1d(1)] if last else [nn.MaxPool1d(kernel_size=2, stride=2), nn.Dropout(dropout)]
            cin = cout
        self.conv_layers = nn.Sequential(*layers)
        head = [nn.Flatten()]
        for width in HEAD_WIDTHS:
            head += [nn.Linear(cin, width), nn.ReLU(), nn.Dropout(dropout)]
            cin = width
        self.classifier = nn.Sequential(*head, nn.Linear(cin, n_classes))

    def _blocks(self):
        """(conv, bn, pool, dropout or None) per conv block, read off the container."""
        mods, out, i = list(self.conv_layers), [], 0
        while i < len(mods):
            conv, bn, pool_mod = mods[i], mods[i + 1], mods[i + 3]
            if isinstance(pool_mod, nn.MaxPool1d):
                out.append((conv, bn, 2, mods[i + 4])); i += 5
            else:
                out.append((conv, bn, 0, None)); i += 4
        return out

    def _features(self, x: torch.Tensor) -> torch.Tensor:
        """[B, n_mels, T] -> [B, 512]: the four conv blocks on channels-last rows."""
        if x.dim() != 3 or x.shape[1] != self.n_mels:
            raise ValueError(f"expected [B, {self.n_mels}, n_frames], got {tuple(x.shape)}")
        dev = self.conv_layers[0].weight.device
        _lib.ctx(dev)                                # raises without a GPU: there is no CPU path
        B, _, T = x.shape
        h = x.to(dev, torch.float32).transpose(1, 2).reshape(B * T, self.n_mels)
        train = self.training
        for conv, bn, pool, drop in self._blocks():
            if train:
                h = _Conv1d.apply(h.contiguous(), conv.weight, conv.bias, B, T, self.precision, self.forward_precision)
            else:
                h = conv1d(h, conv.weight, conv.bias, B, T, self.forward_precision)
            h = batchnorm_relu_pool(bn, h, B, T, pool)
            if pool == 2:
                T //= 2
                h = drop(h)
        return h

    def get_feature_embeddings(self, x: torch.Tensor) -> torch.Tensor:
        """[B, n_mels, n_frames] -> pooled features [B, 512] (spectrogram.py:507-515), never differentiable."""
        with torch.no_grad():
            return self._features(x)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        """[B, n_mels, n_frames] -> logits [B, n_classes].  eval(): under no_grad, BatchNorm on the running statistics; train():
        differentiable, every operator's backward in libawt."""
        lin = [m for m in self.classifier if isinstance(m, nn.Linear)]
        drops = [m for m in self.classifier if isinstance(m, nn.Dropout)]
        P = self.precision
        if self.training:
            h = self._features(x)
            for fc, drop in zip(lin[:-1], drops):
                h = drop(F.relu(Linear.apply(h.contiguous(), fc.weight, fc.bias, P)))
            return Linear.apply(h.contiguous(), lin[-1].weight, lin[-1].bias, P)
        with torch.no_grad():
            h = self._features(x)
            for fc in lin[:-1]:
                h = F.relu(native_linear(h, fc.weight, fc.bias, P))
            return native_linear(h, lin[-1].weight, lin[-1].bias, P)


def train_cnn(train_loader, model: Optional[CNNUrbanSound8KClassifier] = None, epochs: int = 1, lr: float = CNN_LR,
              weight_decay: float = CNN_WEIGHT_DECAY, n_classes: int = 10, n_mels: int = N_MELS, device="cuda", log=None):
    """The reference's CNN training loop (spectrogram.py:517-594) over the native operators: Adam with weight decay, `native_cross_entropy`,
    one optimizer step per batch; returns (model, per-epoch mean loss).  Data loading, the per-epoch evaluation metrics, wandb and
    checkpoint naming stay with the caller; `train_loader` yields (xb [B, n_mels, n_frames], yb [B])."""
    if model is None:
        model = CNNUrbanSound8KClassifier(n_classes=n_classes, n_mels=n_mels).to(device)
    optimizer = torch.optim.Adam(model.parameters(), lr=lr, weight_decay=weight_decay)
    losses = []
    for epoch in range(epochs):
        losses.append(train_epoch(model, train_loader, optimizer, device))
        if log is not None:
            log(f"Epoch {epoch + 1}: Train loss={losses[-1]:.4f}")
    return model, losses


def eval_or_test_cnn(model: CNNUrbanSound8KClassifier, loader, device="cuda") -> list:
    """Arg-max class per clip over `loader` (batches xb or (xb, yb)) with the model in eval() (spectrogram.py:642-660); building the
    result DataFrame stays with the caller."""
    model.eval()
    preds = []
    for batch in loader:
        xb = batch[0] if isinstance(batch, (tuple, list)) else batch
        preds.extend(int(p) for p in model(xb.to(device)).argmax(dim=1).cpu())
    return preds
