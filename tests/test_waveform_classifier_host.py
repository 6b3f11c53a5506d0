"""Host side of the raw-waveform CNN classifier (waveform_classifier.py, csrc/cnn_ops.hip), no GPU: the module's state_dict against a plain
torch.nn restatement of the layer list, the header's declarations and pool-code names, the argument checks of the C-ABI entries, which return
before they touch a GPU, and `UrbanSoundRawDataset` over WAV files written with the standard library."""
import ctypes
import os
import re
import wave

import numpy as np
import pytest
import torch
import torch.nn as nn

from mlx8_ws_audio_transformer_amd import _lib

NEW_SYMBOLS = {"awt_op_conv1d_framed": 12}
POOL_CODES = {"AWT_POOL_MEAN": 0, "AWT_POOL_MAX2": 2, "AWT_POOL_MAX4": 4, "AWT_POOL_MAX4_MEAN": 5}


def restated_waveform_cnn(n_classes=10, dropout=0.3):
    """The layer list as plain torch.nn modules in two containers named like the model's."""
    def block(cin, cout, **conv):
        return [nn.Conv1d(cin, cout, **conv), nn.BatchNorm1d(cout), nn.ReLU(), nn.MaxPool1d(4)]
    m = nn.Module()
    m.conv_layers = nn.Sequential(*block(1, 64, kernel_size=80, stride=16), *block(64, 128, kernel_size=3, padding=1),
                                  *block(128, 256, kernel_size=3, padding=1), nn.AdaptiveAvgPool1d(1))
    m.classifier = nn.Sequential(nn.Flatten(), nn.Linear(256, 128), nn.ReLU(), nn.Dropout(dropout), nn.Linear(128, n_classes))
    return m


@pytest.mark.parametrize("n_classes", [10, 7])
def test_state_dict_is_that_of_the_layer_list(n_classes):
    from mlx8_ws_audio_transformer_amd import CNNWaveformClassifier
    nat, ref = CNNWaveformClassifier(n_classes=n_classes), restated_waveform_cnn(n_classes)      # the constructor needs no GPU
    a, b = nat.state_dict(), ref.state_dict()
    assert list(a) == list(b)
    idx = sorted({int(k.split(".")[1]) for k in a if k.startswith("conv_layers.")}), sorted({int(k.split(".")[1]) for k in a if k.startswith("classifier.")})
    assert idx == ([0, 1, 4, 5, 8, 9], [1, 4])
    for k in a:
        assert a[k].shape == b[k].shape and a[k].dtype == b[k].dtype, k
    assert tuple(a["conv_layers.0.weight"].shape) == (64, 1, 80) and tuple(a["classifier.4.weight"].shape) == (n_classes, 128)
    with torch.no_grad():
        for i, p in enumerate(ref.parameters()):
            p.fill_(0.25 + i)
        ref.conv_layers[5].running_var.fill_(3.0); ref.conv_layers[9].num_batches_tracked.fill_(5)
    assert not any(nat.load_state_dict(ref.state_dict(), strict=True))
    assert torch.equal(nat.state_dict()["classifier.4.bias"], ref.state_dict()["classifier.4.bias"]) and float(nat.conv_layers[5].running_var[0]) == 3.0
    assert int(nat.conv_layers[9].num_batches_tracked) == 5
    assert not any(restated_waveform_cnn(n_classes).load_state_dict(nat.state_dict(), strict=True))


def test_constructor_arguments_and_exports():
    import mlx8_ws_audio_transformer_amd as pkg
    from mlx8_ws_audio_transformer_amd import cnn_classifier as cc, waveform_classifier as wc
    assert pkg.CNNWaveformClassifier is wc.CNNWaveformClassifier and pkg.UrbanSoundRawDataset is wc.UrbanSoundRawDataset
    assert pkg.train_waveform_classifier is wc.train_waveform_classifier
    assert (cc.POOL_MEAN, cc.POOL_MAX2, cc.POOL_MAX4, cc.POOL_MAX4_MEAN) == (0, 2, 4, 5)
    assert wc.FRAMED_ROWS_PER_WORKGROUP == 128 and wc.MIN_SAMPLES == 1088
    m = wc.CNNWaveformClassifier(dropout=0.5)
    assert m.precision == "bf16x3" and m.forward_precision == "fp16x3"
    assert [d.p for d in m.modules() if isinstance(d, nn.Dropout)] == [0.5]
    assert wc.CNNWaveformClassifier().classifier[3].p == cc.CNN_DROPOUT
    with pytest.raises(ValueError, match="bf16"):
        wc.CNNWaveformClassifier(precision="f16f8")
    with pytest.raises(ValueError, match="conv forward"):
        wc.CNNWaveformClassifier(forward_precision="fp32")
    with pytest.raises(ValueError, match="n_classes"):
        wc.CNNWaveformClassifier(n_classes=0)
    with pytest.raises(ValueError, match="dropout"):
        wc.CNNWaveformClassifier(dropout=1.0)
    with pytest.raises(ValueError, match="at least 1088"):          # checked before any device work
        m(torch.zeros(2, 1, 1087))
    with pytest.raises(ValueError, match=r"\[B, 1, n_samples\]"):
        m(torch.zeros(2, 2, 4160))
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="no CPU fallback"):           # no torch fallback for the conv
            m.eval()(torch.zeros(1, 1, 4160))
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            m.train()(torch.zeros(2, 4160))


def test_the_waveform_gets_no_gradient():
    from mlx8_ws_audio_transformer_amd import waveform_classifier as wc
    w, b = torch.zeros(64, 1, 80, requires_grad=True), torch.zeros(64, requires_grad=True)
    with pytest.raises(ValueError, match="waveform is data"):
        wc._Conv1dFramed.apply(torch.zeros(1, 4160, requires_grad=True), w, b, 16, "bf16x3")


def test_header_declares_the_new_entry_point_and_the_pool_codes():
    text = re.sub(r"/\*.*?\*/", "", open(_lib.HEADER_PATH).read(), flags=re.S)
    for name, nargs in NEW_SYMBOLS.items():
        m = re.search(r"\b%s\s*\(([^;]*)\)\s*;" % name, text)
        assert m, name
        assert len(m.group(1).split(",")) == nargs == len(_lib._SIGNATURES[name][1]), name
    for name, value in POOL_CODES.items():
        assert re.search(r"\b%s\s*=\s*%d\b" % (name, value), text), name
    for name, nargs in (("awt_op_bn_relu_pool", 13), ("awt_op_bn_relu_pool_backward", 18)):       # the signatures did not change
        assert len(re.search(r"\b%s\s*\(([^;]*)\)\s*;" % name, text).group(1).split(",")) == nargs == len(_lib._SIGNATURES[name][1])


@pytest.fixture(scope="module")
def built():
    if not os.path.exists(_lib.LIB_PATH):
        from mlx8_ws_audio_transformer_amd.build import build
        build(verbose=False)
    return _lib.lib()


def test_framed_conv_argument_checks_return_before_any_launch(built):
    L = built
    err = lambda: L.awt_last_error().decode()
    buf = ctypes.create_string_buffer(1 << 12)
    p = (ctypes.addressof(buf) + 255) & ~255      # a non-null aligned host address: every call below is refused before it is used
    INVALID = -1
    call = lambda x=p, pitch=4160, w=p, b=p, y=p, B=2, n=4160, kernel=80, stride=16, cout=64, c=p: \
        L.awt_op_conv1d_framed(c, x, pitch, w, b, y, B, n, kernel, stride, cout, None)
    assert call(kernel=72) == INVALID and "multiple of the stride" in err()
    assert call(kernel=80, stride=20) == INVALID and "multiple of 8" in err()
    assert call(kernel=84, stride=12) == INVALID and "multiple of 8" in err()
    assert call(stride=0) == INVALID and call(kernel=0) == INVALID
    assert call(n=79, pitch=80) == INVALID and "n_samples" in err()
    assert call(cout=40) == INVALID and "Cout" in err()
    assert call(cout=0) == INVALID and "Cout" in err()
    assert call(cout=256) == INVALID and "LDS" in err()                      # 256 x 84 weights do not fit beside the samples
    assert call(c=None) == INVALID and "null" in err()
    for k in ("x", "w", "b", "y"):
        assert call(**{k: None}) == INVALID and "null" in err(), k
        assert call(**{k: p + 4}) == INVALID and "aligned" in err(), k
    assert call(pitch=4158) == INVALID and "pitch" in err()
    assert call(pitch=4000) == INVALID and "pitch" in err()
    assert call(B=0) == INVALID and call(B=65536) == INVALID


def test_pool_code_checks_return_before_any_launch(built):
    L = built
    err = lambda: L.awt_last_error().decode()
    buf = ctypes.create_string_buffer(1 << 12)
    p = (ctypes.addressof(buf) + 255) & ~255
    big, INVALID = 1 << 30, -1
    fwd = lambda T, pool, y=p: L.awt_op_bn_relu_pool(p, p, p, p, p, p, 1e-5, y, 2, T, 128, pool, None)
    bwd = lambda T, pool, ws=p: L.awt_op_bn_relu_pool_backward(p, p, p, p, p, p, p, 1e-5, p, p, p, 2, T, 128, pool, ws, big, None)
    for call in (fwd, bwd):
        for pool in (4, 5):
            assert call(3, pool) == INVALID and "pool" in err(), pool                   # no window of 4 frames
            assert call(4, pool, None) == INVALID and "null" in err(), pool             # the code itself is accepted: refused at the null check
            assert call(13, pool, None) == INVALID and "null" in err(), pool
        for pool in (1, 3, 6, -1):
            assert call(13, pool) == INVALID and "pool" in err(), pool
        assert call(1, 2) == INVALID and "pool" in err()
        assert call(13, 0, None) == INVALID and "null" in err() and call(13, 2, None) == INVALID and "null" in err()


# ---------------------------------------------------------------------------------------------------------------- UrbanSoundRawDataset
def _write_wav(path, samples):
    """int16 [n] or [n, C] -> PCM16 WAV at the front-end's own rate (16 kHz), so that no resampling, hence no GPU, is needed"""
    from mlx8_ws_audio_transformer_amd.urbansound import SAMPLE_RATE
    os.makedirs(os.path.dirname(path), exist_ok=True)
    samples = np.asarray(samples, dtype="<i2")
    with wave.open(path, "wb") as f:
        f.setnchannels(1 if samples.ndim == 1 else samples.shape[1])
        f.setsampwidth(2)
        f.setframerate(SAMPLE_RATE)
        f.writeframes(samples.tobytes())


def test_raw_dataset_items(tmp_path):
    from mlx8_ws_audio_transformer_amd import UrbanSoundRawDataset
    from mlx8_ws_audio_transformer_amd.urbansound import DURATION, SAMPLE_RATE
    n_out = int(SAMPLE_RATE * DURATION)
    rng = np.random.default_rng(0)
    clips = {"short_mono.wav": (1, 3, rng.integers(-30000, 30000, 20001)),
             "long_mono.wav": (2, 7, rng.integers(-30000, 30000, n_out + 6000)),
             "short_stereo.wav": (1, 0, rng.integers(-30000, 30000, (12345, 2))),
             "long_stereo.wav": (3, 9, rng.integers(-30000, 30000, (n_out + 3, 2))),
             "exact_mono.wav": (2, 4, rng.integers(-30000, 30000, n_out))}
    lines = ["slice_file_name,fsID,start,end,salience,fold,classID,class"]
    for name, (fold, cid, s) in clips.items():
        _write_wav(str(tmp_path / "audio" / f"fold{fold}" / name), s)
        lines.append(f"{name},1,0.0,4.0,1,{fold},{cid},c{cid}")
    csv = tmp_path / "meta.csv"
    csv.write_text("\n".join(lines) + "\n")
    ds = UrbanSoundRawDataset(str(csv), data_root=str(tmp_path))
    assert len(ds) == 5 and list(ds.df["slice_file_name"]) == list(clips)
    for i, (name, (fold, cid, s)) in enumerate(clips.items()):
        x, y = ds[i]
        assert y == cid and isinstance(y, int) and tuple(x.shape) == (1, n_out) and x.dtype == torch.float32 and not x.is_cuda, name
        mono = torch.from_numpy(np.asarray(s, dtype=np.float32) / 32768.0)
        mono = mono if mono.dim() == 1 else mono.mean(1)                  # stereo: the channel mean
        n = min(len(mono), n_out)
        assert torch.allclose(x[0, :n], mono[:n], rtol=0, atol=1e-7), name          # a prefix of the file
        assert not x[0, n:].any(), name                                             # zero padding
    sub = UrbanSoundRawDataset(str(csv), folds=[1, 3], data_root=str(tmp_path))
    assert list(sub.df["slice_file_name"]) == ["short_mono.wav", "short_stereo.wav", "long_stereo.wav"] and [sub[i][1] for i in range(3)] == [3, 0, 9]
    assert len(UrbanSoundRawDataset(str(csv), folds=[8], data_root=str(tmp_path))) == 0
    calls = []

    def loader(path):                                      # a torchaudio-style loader: [C, n] float
        calls.append(os.path.basename(path))
        return torch.full((2, 100), 0.25), SAMPLE_RATE
    x, y = UrbanSoundRawDataset(str(csv), folds=[2], data_root=str(tmp_path), loader=loader)[0]
    assert calls == ["long_mono.wav"] and y == 7 and float(x[0, 99]) == 0.25 and float(x[0, 100]) == 0.0
