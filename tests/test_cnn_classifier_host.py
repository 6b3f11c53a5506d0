"""Host side of the CNN classifier (cnn_classifier.py, csrc/cnn_ops.hip), no GPU: the module's state_dict against a plain torch.nn
restatement of the layer list, the header's declarations, and the argument checks of the new C-ABI entries, which return before they touch a GPU."""
import ctypes
import re

import pytest
import torch
import torch.nn as nn

from mlx8_ws_audio_transformer_amd import _lib

NEW_SYMBOLS = {"awt_op_conv1d_workspace_bytes": 4, "awt_op_conv1d": 14, "awt_op_batchnorm_stats_workspace_bytes": 2, "awt_op_batchnorm_stats": 9,
               "awt_op_bn_relu_pool": 13, "awt_op_bn_relu_pool_backward_workspace_bytes": 3, "awt_op_bn_relu_pool_backward": 18}


def restated_cnn(n_classes=10, n_mels=64, dropout=0.3):
    """The layer list as plain torch.nn modules in two containers named like the model's."""
    def block(cin, cout, last=False):
        tail = [nn.AdaptiveAvgPool1d(1)] if last else [nn.MaxPool1d(2, 2), nn.Dropout(dropout)]
        return [nn.Conv1d(cin, cout, 3, padding=1), nn.BatchNorm1d(cout), nn.ReLU()] + tail
    m = nn.Module()
    m.conv_layers = nn.Sequential(*block(n_mels, 128), *block(128, 256), *block(256, 512), *block(512, 512, last=True))
    m.classifier = nn.Sequential(nn.Flatten(), nn.Linear(512, 256), nn.ReLU(), nn.Dropout(dropout), nn.Linear(256, 128), nn.ReLU(), nn.Dropout(dropout),
                                 nn.Linear(128, n_classes))
    return m


@pytest.mark.parametrize("n_mels,n_classes", [(64, 10), (80, 10), (128, 7)])
def test_state_dict_is_that_of_the_layer_list(n_mels, n_classes):
    from mlx8_ws_audio_transformer_amd import CNNUrbanSound8KClassifier
    nat, ref = CNNUrbanSound8KClassifier(n_classes=n_classes, n_mels=n_mels), restated_cnn(n_classes, n_mels)      # the constructor needs no GPU
    a, b = nat.state_dict(), ref.state_dict()
    assert list(a) == list(b)
    idx = sorted({int(k.split(".")[1]) for k in a if k.startswith("conv_layers.")}), sorted({int(k.split(".")[1]) for k in a if k.startswith("classifier.")})
    assert idx == ([0, 1, 5, 6, 10, 11, 15, 16], [1, 4, 7])
    for k in a:
        assert a[k].shape == b[k].shape and a[k].dtype == b[k].dtype, k
    with torch.no_grad():
        for i, p in enumerate(ref.parameters()):
            p.fill_(0.25 + i)
        ref.conv_layers[6].running_var.fill_(3.0); ref.conv_layers[16].num_batches_tracked.fill_(5)
    assert not any(nat.load_state_dict(ref.state_dict(), strict=True))
    assert torch.equal(nat.state_dict()["classifier.7.bias"], ref.state_dict()["classifier.7.bias"]) and float(nat.conv_layers[6].running_var[0]) == 3.0
    assert int(nat.conv_layers[16].num_batches_tracked) == 5
    assert not any(restated_cnn(n_classes, n_mels).load_state_dict(nat.state_dict(), strict=True))


def test_constructor_arguments_and_exports():
    import mlx8_ws_audio_transformer_amd as pkg
    from mlx8_ws_audio_transformer_amd import cnn_classifier as cc
    assert pkg.train_cnn is cc.train_cnn and pkg.eval_or_test_cnn is cc.eval_or_test_cnn
    m = cc.CNNUrbanSound8KClassifier(dropout=0.5)
    assert m.n_mels == cc.N_MELS and m.precision == "bf16x3"
    assert [d.p for d in m.modules() if isinstance(d, nn.Dropout)] == [0.5] * 5
    with pytest.raises(ValueError, match="bf16"):
        cc.CNNUrbanSound8KClassifier(precision="f16f8")
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="no CPU fallback"):           # no torch fallback for the conv
            m.eval()(torch.zeros(1, cc.N_MELS, 16))


def test_header_declares_the_new_entry_points():
    text = re.sub(r"/\*.*?\*/", "", open(_lib.HEADER_PATH).read(), flags=re.S)
    for name, nargs in NEW_SYMBOLS.items():
        m = re.search(r"\b%s\s*\(([^;]*)\)\s*;" % name, text)
        assert m, name
        assert len(m.group(1).split(",")) == nargs == len(_lib._SIGNATURES[name][1]), name


@pytest.fixture(scope="module")
def built():
    import os
    if not os.path.exists(_lib.LIB_PATH):
        from mlx8_ws_audio_transformer_amd.build import build
        build(verbose=False)
    return _lib.lib()


def test_workspace_sizes(built):
    L = built
    assert L.awt_op_conv1d_workspace_bytes(0, 4, 64, 128) == 0 and L.awt_op_batchnorm_stats_workspace_bytes(5, 0) == 0
    assert L.awt_op_bn_relu_pool_backward_workspace_bytes(1, 0, 4) == 0
    assert L.awt_op_conv1d_workspace_bytes(3, 126, 128, 256) >= 2 * 378 * 128 * 2 + 2 * 256 * 384 * 2       # hi + lo planes of x and of the packed weight
    assert L.awt_op_batchnorm_stats_workspace_bytes(64, 128) == 2 * 128 * 4 and L.awt_op_batchnorm_stats_workspace_bytes(65, 128) == 2 * 2 * 128 * 4
    assert L.awt_op_bn_relu_pool_backward_workspace_bytes(2, 33, 512) == 2 * 2 * 512 * 4


def test_argument_checks_return_before_any_launch(built):
    L = built
    err = lambda: L.awt_last_error().decode()
    buf = ctypes.create_string_buffer(1 << 12)
    p = (ctypes.addressof(buf) + 255) & ~255      # a non-null aligned host address: every call below is refused before it is used
    big, INVALID, WORKSPACE = 1 << 30, -1, -3
    assert L.awt_op_conv1d(p, p, p, p, p, 2, 13, 64, 128, 5, 3, p, big, None) == INVALID and "taps must be 3" in err()
    assert L.awt_op_conv1d(p, p, p, p, p, 2, 13, 64, 128, 3, 5, p, big, None) == INVALID and "terms" in err()
    assert L.awt_op_conv1d(p, p, p, p, p, 2, 13, 62, 128, 3, 3, p, big, None) == INVALID and "Cin % 64" in err()
    assert L.awt_op_conv1d(p, p, p, p, p, 2, 13, 64, 130, 3, 3, p, big, None) == INVALID
    assert L.awt_op_conv1d(None, p, p, p, p, 2, 13, 64, 128, 3, 3, p, big, None) == INVALID and "null" in err()
    assert L.awt_op_conv1d(p, p + 4, p, p, p, 2, 13, 64, 128, 3, 3, p, big, None) == INVALID and "aligned" in err()
    assert L.awt_op_conv1d(p, p, p, p, p, 2, 13, 64, 128, 3, 3, p, 1024, None) == WORKSPACE and "op_conv1d: workspace too small" in err()
    assert L.awt_op_batchnorm_stats(p, p, 100, 126, p, p, p, big, None) == INVALID and "multiple of 4" in err()
    assert L.awt_op_batchnorm_stats(p, p, 0, 128, p, p, p, big, None) == INVALID
    assert L.awt_op_batchnorm_stats(p, None, 100, 128, p, p, p, big, None) == INVALID
    assert L.awt_op_batchnorm_stats(p, p, 100, 128, p, p, p, 2 * 2 * 128 * 4 - 1, None) == WORKSPACE and "op_batchnorm_stats" in err()
    assert L.awt_op_bn_relu_pool(p, p, p, p, p, p, 1e-5, p, 2, 13, 130, 2, None) == INVALID and "multiple of 4" in err()
    assert L.awt_op_bn_relu_pool(p, p, p, p, p, p, 1e-5, p, 2, 13, 128, 3, None) == INVALID and "pool" in err()
    assert L.awt_op_bn_relu_pool(p, p, p, p, p, p, 1e-5, p, 2, 1, 128, 2, None) == INVALID            # no frame pair to pool
    assert L.awt_op_bn_relu_pool(p, p, p, p, p, p, 1e-5, None, 2, 13, 128, 2, None) == INVALID
    assert L.awt_op_bn_relu_pool_backward(p, p, p, p, p, p, p, 1e-5, p, p, p, 2, 13, 6, 2, p, big, None) == INVALID and "multiple of 4" in err()
    assert L.awt_op_bn_relu_pool_backward(p, p, p, p, p, p, p, 1e-5, p, p, p, 2, 13, 128, 1, p, big, None) == INVALID
    assert L.awt_op_bn_relu_pool_backward(p, p, p, p, p, p, p, 1e-5, p, p, p, 2, 13, 128, 2, None, big, None) == INVALID
    assert L.awt_op_bn_relu_pool_backward(p, p, p, p, p, p, p, 1e-5, p, p, p, 2, 13, 128, 2, p, 16, None) == WORKSPACE and "op_bn_relu_pool_backward" in err()
