"""`CNNWaveformClassifier`, `UrbanSoundRawDataset` and `train_waveform_classifier` (the reference's UrbanSound8K script,
spectrogram.py:664-741: its raw-waveform model) on libawt, inference and training.  DESIGN.md section 4.10.

The layer list, with the reference's `nn.Sequential` indices so that a checkpoint written by its `torch.save(model.state_dict())` loads with
`load_state_dict(strict=True)`:

    conv_layers   0 Conv1d(1, 64, 80, stride 16)     1 BatchNorm1d(64)    2 ReLU   3 MaxPool1d(4)
                  4 Conv1d(64, 128, 3, padding 1)    5 BatchNorm1d(128)   6 ReLU   7 MaxPool1d(4)
                  8 Conv1d(128, 256, 3, padding 1)   9 BatchNorm1d(256)  10 ReLU  11 MaxPool1d(4)   12 AdaptiveAvgPool1d(1)
    classifier    0 Flatten   1 Linear(256, 128)   2 ReLU   3 Dropout   4 Linear(128, n_classes)

The modules in the two containers hold the parameters and buffers only; `forward` does not call them.  The waveform [B, N] is the input of
  * the first layer: `awt_op_conv1d_framed`, one launch on the exact-fp32 MFMA that writes channels-last rows [B T1, 64], what every other
    operator reads; its weight gradient is `awt_op_weight_grad` once per block of `stride` taps over the waveform viewed as rows of `stride`
    samples (kernel = 5 stride: a 5-tap convolution without padding over those rows), its bias gradient `awt_op_column_sums`; the waveform is
    data and gets no gradient;
  * blocks 2 and 3: `_Conv1d` / `conv1d` of cnn_classifier.py, which this model is built from (`awt_op_conv1d`: forward in `forward_precision`, gradients in `precision`);
  * BatchNorm1d + ReLU + MaxPool1d(4): `batchnorm_relu_pool` with `POOL_MAX4`; the last block's MaxPool1d(4) + AdaptiveAvgPool1d(1) is one
    launch, `POOL_MAX4_MEAN`, whose pooled tensor is never written;
  * head: `autograd_ops.Linear`; loss: `autograd_ops.native_cross_entropy` (inside `train_epoch`).
There is no torch fallback and nothing is cached between calls.
"""
from __future__ import annotations

import os
from typing import Optional

import torch
import torch.nn as nn
import torch.nn.functional as F
from torch.utils.data import Dataset

from . import _lib, native_decoder as nd, ops
from .autograd_ops import Linear, native_linear, train_epoch
from .cnn_classifier import (CNN_DROPOUT, CNN_LR, CNN_WEIGHT_DECAY, POOL_MAX4, POOL_MAX4_MEAN, _Conv1d, _forward_terms, _terms,
                             batchnorm_relu_pool, conv1d)
from .urbansound import DATA_ROOT, DURATION, METADATA_CSV, SAMPLE_RATE, preprocess_audio_for_cnn, read_wav

WAVE_KERNEL, WAVE_STRIDE = 80, 16                       # spectrogram.py:669
WAVE_CHANNELS = (64, 128, 256)
WAVE_HEAD_WIDTH = 128
FRAMED_ROWS_PER_WORKGROUP = 128                         # output frames one workgroup of awt_op_conv1d_framed owns (csrc/cnn_ops.hip kFramedRows)
MIN_SAMPLES = WAVE_KERNEL + WAVE_STRIDE * 63            # 1088: 64 -> 16 -> 4 -> 1 frames, the shortest clip the layer list accepts


def framed_length(n_samples: int, kernel: int, stride: int) -> int:
    """Frames of an unpadded Conv1d: (n_samples - kernel) // stride + 1."""
    return (n_samples - kernel) // stride + 1


# ------------------------------------------------------------------------------------------------ operators (no autograd)
def conv1d_framed(x: torch.Tensor, w: torch.Tensor, b: torch.Tensor, stride: int) -> torch.Tensor:
    """`F.conv1d(x[:, None], w, b, stride=stride)` in exact fp32 as channels-last rows: x [B, N] device waveform, w [Cout, 1, kernel]
    -> [B T1, Cout] (`awt_op_conv1d_framed`).  stride % 8 == 0, kernel % stride == 0, Cout % 16 == 0, N >= kernel."""
    if x.dim() != 2 or w.dim() != 3 or w.shape[1] != 1:
        raise ValueError(f"conv1d_framed: x must be [B, N] and w [Cout, 1, kernel], got {tuple(x.shape)} and {tuple(w.shape)}")
    B, N = x.shape
    cout, _, kernel = w.shape
    x = x.float()
    if N % 4:                                        # the clip pitch is a multiple of 4 floats (16-byte rows); the padding is never read
        x = F.pad(x, (0, 4 - N % 4))
    x, w, b = x.contiguous(), w.float().contiguous(), b.float().contiguous()
    t1 = max(framed_length(N, kernel, stride), 0) if stride > 0 else 0
    y = torch.empty((B * t1, cout), dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        _lib.check(_lib.lib().awt_op_conv1d_framed(_lib.ctx(x.device), _lib.ptr(x), x.stride(0), _lib.ptr(w), _lib.ptr(b), _lib.ptr(y), B, N,
                                                   kernel, stride, cout, _lib.stream_handle()))
    return y


def conv1d_framed_weight_grad(dy: torch.Tensor, x: torch.Tensor, kernel: int, stride: int, precision: str = "bf16x3") -> torch.Tensor:
    """dW [Cout, 1, kernel] of `conv1d_framed` from dy [B T1, Cout] and the waveform x [B, N].  With m = kernel / stride the layer is an m-tap
    convolution without padding over the waveform as rows [B (T1 + m - 1), stride]: dW[:, 0, j stride : (j + 1) stride] = dy^T rows[frame + j],
    one weight-gradient GEMM per j under the row map (T1, T1 + m - 1, 1, j), written through the gradient's strides (kernel, 1)."""
    B, N = x.shape
    t1, m = framed_length(N, kernel, stride), kernel // stride
    rows = x[:, :stride * (t1 + m - 1)].float().contiguous().view(B * (t1 + m - 1), stride)        # a copy unless N is exactly that length
    dw = torch.empty((dy.shape[1], kernel), dtype=torch.float32, device=dy.device)
    for j in range(m):
        ops.weight_grad(dy, rows, precision=precision, out=dw[:, j * stride:(j + 1) * stride], row_map=(t1, t1 + m - 1, 1, j))
    return dw.unsqueeze(1)


class _Conv1dFramed(torch.autograd.Function):
    """y [B T1, Cout] = conv1d_framed(x [B, N], w [Cout, 1, kernel], b) with dW and db on libawt.  The waveform is data: it gets no gradient."""

    @staticmethod
    def forward(ctx, x, w, b, stride, precision):
        if ctx.needs_input_grad[0]:
            raise ValueError("conv1d_framed: the waveform is data and has no gradient here; pass it without requires_grad")
        _terms(precision)
        ctx.save_for_backward(x)
        ctx.cfg = (int(w.shape[2]), stride, precision)
        return conv1d_framed(x, w, b, stride)

    @staticmethod
    def backward(ctx, dy):
        (x,) = ctx.saved_tensors
        kernel, stride, precision = ctx.cfg
        dy = dy.contiguous()
        return None, conv1d_framed_weight_grad(dy, x, kernel, stride, precision), nd.column_sums(dy), None, None


# ------------------------------------------------------------------------------------------------ the model
class CNNWaveformClassifier(nn.Module):
    def __init__(self, n_classes: int = 10, dropout: float = CNN_DROPOUT, precision: str = "bf16x3", forward_precision: str = "fp16x3"):
        """precision: operand planes of the gradient GEMMs and of the head.  forward_precision: those of the forwards of conv 2 and 3 (see
        `CNNUrbanSound8KClassifier`); conv 1 is always exact fp32."""
        super().__init__()
        _terms(precision)
        _forward_terms(forward_precision)
        if not isinstance(n_classes, int) or n_classes < 1:
            raise ValueError("n_classes must be a positive integer")
        if not 0.0 <= float(dropout) < 1.0:
            raise ValueError("dropout must lie in [0, 1)")
        self.precision, self.forward_precision = precision, forward_precision
        c1, c2, c3 = WAVE_CHANNELS
        self.conv_layers = nn.Sequential(
            nn.Conv1d(1, c1, kernel_size=WAVE_KERNEL, stride=WAVE_STRIDE), nn.BatchNorm1d(c1), nn.ReLU(), nn.MaxPool1d(kernel_size=4),
            nn.Conv1d(c1, c2, kernel_size=3, padding=1), nn.BatchNorm1d(c2), nn.ReLU(), nn.MaxPool1d(kernel_size=4),
            nn.Conv1d(c2, c3, kernel_size=3, padding=1), nn.BatchNorm1d(c3), nn.ReLU(), nn.MaxPool1d(kernel_size=4),
            nn.AdaptiveAvgPool1d(1))
        self.classifier = nn.Sequential(nn.Flatten(), nn.Linear(c3, WAVE_HEAD_WIDTH), nn.ReLU(), nn.Dropout(dropout),
                                        nn.Linear(WAVE_HEAD_WIDTH, n_classes))

    def _features(self, x: torch.Tensor) -> torch.Tensor:
        """[B, 1, N] or [B, N] -> [B, 256]: the three conv blocks on channels-last rows."""
        if x.dim() == 3 and x.shape[1] == 1:
            x = x[:, 0]
        if x.dim() != 2:
            raise ValueError(f"expected a waveform batch [B, 1, n_samples] or [B, n_samples], got {tuple(x.shape)}")
        B, N = x.shape
        if N < MIN_SAMPLES:
            raise ValueError(f"a clip needs at least {MIN_SAMPLES} samples (64 -> 16 -> 4 -> 1 frames), got {N}")
        L = self.conv_layers
        dev = L[0].weight.device
        _lib.ctx(dev)                                # raises without a GPU: there is no CPU path
        x = x.to(dev, torch.float32)
        train = self.training
        T = framed_length(N, WAVE_KERNEL, WAVE_STRIDE)
        if train:
            h = _Conv1dFramed.apply(x, L[0].weight, L[0].bias, WAVE_STRIDE, self.precision)
        else:
            h = conv1d_framed(x, L[0].weight, L[0].bias, WAVE_STRIDE)
        h = batchnorm_relu_pool(L[1], h, B, T, POOL_MAX4)
        T //= 4
        for conv, bn, pool in ((L[4], L[5], POOL_MAX4), (L[8], L[9], POOL_MAX4_MEAN)):
            if train:
                h = _Conv1d.apply(h.contiguous(), conv.weight, conv.bias, B, T, self.precision, self.forward_precision)
            else:
                h = conv1d(h, conv.weight, conv.bias, B, T, self.forward_precision)
            h = batchnorm_relu_pool(bn, h, B, T, pool)
            T //= 4
        return h

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        """[B, 1, n_samples] or [B, n_samples] -> logits [B, n_classes].  eval(): under no_grad, BatchNorm on the running statistics; train():
        differentiable in every parameter, every operator's backward in libawt."""
        fc1, drop, fc2 = self.classifier[1], self.classifier[3], self.classifier[4]
        P = self.precision
        if self.training:
            h = drop(F.relu(Linear.apply(self._features(x).contiguous(), fc1.weight, fc1.bias, P)))
            return Linear.apply(h.contiguous(), fc2.weight, fc2.bias, P)
        with torch.no_grad():
            h = F.relu(native_linear(self._features(x), fc1.weight, fc1.bias, P))
            return native_linear(h, fc2.weight, fc2.bias, P)


# ------------------------------------------------------------------------------------------------ data
class UrbanSoundRawDataset(Dataset):
    """The data set spectrogram.py:702-703 names and never defines: the rows of the UrbanSound8K metadata CSV in `folds`, each item
    `(waveform FloatTensor [1, int(SAMPLE_RATE * DURATION)], class_id)` made by `loader` and `preprocess_audio_for_cnn` (mono mean, resample
    to SAMPLE_RATE, zero-pad or truncate).  `loader(path) -> (samples, rate)` defaults to `read_wav` ([n, C] in file order); a
    torchaudio-style loader returning [C, n] works too (the layout is inferred as in `preprocess_to_parquet`).  A file already at
    SAMPLE_RATE never touches the GPU; one that needs resampling goes through libawt and comes back to the host."""

    def __init__(self, metadata_csv: Optional[str] = None, folds=None, data_root: Optional[str] = None, loader=None):
        import pandas as pd

        self.df = pd.read_csv(metadata_csv or METADATA_CSV)
        if folds is not None:
            self.df = self.df[self.df["fold"].isin(list(folds))].reset_index(drop=True)
        self.data_root = data_root or DATA_ROOT
        self.loader = loader or read_wav

    def __len__(self):
        return len(self.df)

    def __getitem__(self, idx):
        row = self.df.iloc[idx]
        samples, rate = self.loader(os.path.join(self.data_root, "audio", f"fold{row['fold']}", row["slice_file_name"]))
        interleaved = samples.dim() == 2 and samples.shape[1] <= 8 < samples.shape[0]
        w = samples.float() / 32768.0 if samples.dtype == torch.int16 else samples.float()          # 16-bit PCM scaled like torchaudio.load
        if w.dim() == 1:
            w = w.unsqueeze(0)
        elif interleaved:
            w = w.t()
        _, cnn, _ = preprocess_audio_for_cnn(w, rate)
        assert tuple(cnn.shape) == (1, int(SAMPLE_RATE * DURATION))
        return cnn.cpu(), int(row["classID"])


# ------------------------------------------------------------------------------------------------ training
def train_waveform_classifier(train_loader, val_loader=None, model: Optional[CNNWaveformClassifier] = None, epochs: int = 1, lr: float = CNN_LR,
                              weight_decay: float = CNN_WEIGHT_DECAY, device="cuda", log=None, ckpt_path: Optional[str] = None):
    """The reference's loop (spectrogram.py:699-741) over the native operators: Adam with weight decay, `native_cross_entropy`, one optimizer
    step per batch, after each epoch the arg-max accuracy over `val_loader` in eval().  Returns (model, per-epoch mean loss, per-epoch
    validation accuracy); `state_dict()` is saved to `ckpt_path` when one is given.  Building the data sets from METADATA_CSV and the folds
    stays with the caller; the loaders yield (xb [B, 1, n_samples], yb [B])."""
    if model is None:
        model = CNNWaveformClassifier().to(device)
    optimizer = torch.optim.Adam(model.parameters(), lr=lr, weight_decay=weight_decay)
    losses, accuracies = [], []
    for epoch in range(epochs):
        losses.append(train_epoch(model, train_loader, optimizer, device))
        if log is not None:
            log(f"Epoch {epoch + 1}: Train Loss = {losses[-1]:.4f}")
        if val_loader is not None:
            model.eval()
            correct, count = 0, 0
            for xb, yb in val_loader:
                preds = model(xb.to(device)).argmax(dim=1)
                correct += int((preds == yb.to(device)).sum())
                count += yb.size(0)
            accuracies.append(correct / max(count, 1))
            if log is not None:
                log(f"Epoch {epoch + 1}: Val Accuracy = {accuracies[-1]:.4f}")
    if ckpt_path is not None:
        os.makedirs(os.path.dirname(os.path.abspath(ckpt_path)), exist_ok=True)
        torch.save(model.state_dict(), ckpt_path)
    return model, losses, accuracies
