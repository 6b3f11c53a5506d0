"""CPU-side checks of the full-parameter fine-tuning surface: the new C-ABI symbols are exported and bound, the constructors validate their
arguments before anything touches the GPU, and the trainable-parameter count of Whisper-small's encoder is the reference's."""
import ctypes
import os

import pytest

from mlx8_ws_audio_transformer_amd import _lib, weights as wts

NEW_SYMBOLS = {"awt_encoder_base_grad_count": 1, "awt_encoder_base_grad_params": 1, "awt_encoder_base_grad_param": 6,
               "awt_op_weight_grad_workspace_bytes": 6, "awt_op_weight_grad": 24}


@pytest.fixture(scope="module")
def built():
    if not os.path.exists(_lib.LIB_PATH):
        from mlx8_ws_audio_transformer_amd.build import build
        build(verbose=False)
    return _lib.lib()


def test_new_symbols_are_declared_exported_and_bound(built):
    declared = set(_lib.declared_symbols())
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name, nargs in NEW_SYMBOLS.items():
        assert name in declared, f"{name} is not declared in include/awt.h"
        assert hasattr(raw, name), f"{name} is not exported by libawt.so"
        res, args = _lib._SIGNATURES[name]
        assert len(args) == nargs and getattr(built, name).argtypes == args, name
    assert [f for f, _ in _lib.EncoderCfg._fields_][-1] == "train_base"      # the trailing field: callers that leave it zero get the adapter-only library
    assert ctypes.sizeof(_lib.EncoderCfg) == 14 * 4


def test_queries_answer_without_a_handle(built):
    assert built.awt_encoder_base_grad_count(None) == 0
    assert built.awt_encoder_base_grad_params(None) == 0
    assert built.awt_op_weight_grad_workspace_bytes(24000, 24000, 3072, 768, 3072, 768) >= 2 * 24000 * (3072 + 768) * 2 + 3072 * 768 * 4
    assert built.awt_op_weight_grad_workspace_bytes(0, 0, 8, 8, 8, 8) == 0


def test_constructors_validate_the_full_parameter_mode():
    from mlx8_ws_audio_transformer_amd.encoder import NativeWhisperEncoder
    cfg = wts.config("mini", True)
    with pytest.raises(ValueError, match="trainable"):
        NativeWhisperEncoder(cfg, train_base=True, device="cpu")
    with pytest.raises(ValueError, match="LoRA"):
        NativeWhisperEncoder(cfg, trainable=True, train_base=True, lora=wts.LoraSpec(r=8, alpha=16.0, targets=("q_proj",)), device="cpu")
    with pytest.raises(ValueError, match="f16f8"):
        NativeWhisperEncoder(cfg, precision="bf16x3", trainable=True, train_base=True, backward_precision="f16f8", device="cpu")
    with pytest.raises(ValueError, match="needs LoRA"):
        NativeWhisperEncoder(cfg, trainable=True, device="cpu")                  # unchanged: nothing to train


def test_trainable_parameter_count_of_whisper_small():
    from mlx8_ws_audio_transformer_amd.encoder import NativeWhisperEncoder
    enc = NativeWhisperEncoder(wts.config("small"), trainable=True, train_base=True, device="cpu", seed=None)
    trainable = {n: p for n, p in enc.named_parameters() if p.requires_grad}
    assert "embed_positions.weight" not in trainable
    assert sum(p.numel() for p in trainable.values()) == 87_002_112
    assert len(trainable) == len(list(enc.parameters())) - 1
