"""CPU: what the decoder's full-parameter fine-tuning checks before any device work -- the constructor errors, and the argument errors of the
new C-ABI entries (include/awt.h: awt_op_embed_backward, awt_op_column_sums_ld, awt_weight_update), which return before they touch a GPU."""
import ctypes as C

import pytest

from mlx8_ws_audio_transformer_amd import _lib, weights as wts

INVALID = -1          # AWT_ERR_INVALID


def test_train_decoder_rejects_decoder_adapters_before_building_anything():
    from mlx8_ws_audio_transformer_amd.finetune import WhisperLoRAModel
    cfg = wts.config("mini", True)
    with pytest.raises(ValueError, match="train_decoder=True trains the decoder's base weights"):
        WhisperLoRAModel(cfg, None, train_decoder=True, decoder_lora=wts.LoraSpec(r=8, alpha=16.0))
    with pytest.raises(ValueError, match="train_decoder=True trains the decoder's base weights"):
        WhisperLoRAModel(cfg, wts.LoraSpec(r=8, alpha=16.0), train_decoder=True, decoder_lora=wts.LoraSpec(r=8, alpha=16.0))


def test_train_base_rejects_adapters_and_marks_every_parameter_trainable():
    from mlx8_ws_audio_transformer_amd.native_decoder import NativeWhisperDecoder
    with pytest.raises(ValueError, match="train_base=True trains the decoder's base weights"):
        NativeWhisperDecoder(128, 1, 2, 512, 512, 64, lora=wts.LoraSpec(r=8, alpha=16.0), train_base=True)
    dec = NativeWhisperDecoder(128, 1, 2, 512, 512, 64, train_base=True)
    names = [n for n, _ in dec.named_parameters()]
    assert all(p.requires_grad for p in dec.parameters()) and "embed_positions.weight" in names and "embed_tokens.weight" in names
    assert [id(p) for p in dec.base_parameters()] == [id(p) for p in dec.parameters()]
    assert not any(p.requires_grad for p in NativeWhisperDecoder(128, 1, 2, 512, 512, 64).parameters())


def _err():
    return _lib.lib().awt_last_error().decode()


def test_embed_backward_argument_errors():
    L = _lib.lib()
    p = C.c_void_p(4096)          # never dereferenced: the checks come first
    assert L.awt_op_embed_backward(None, p, p, p, p, 24, 12, 128, 0, 512, None) == INVALID and "op_embed_backward" in _err()
    assert L.awt_op_embed_backward(p, None, p, p, p, 24, 12, 128, 0, 512, None) == INVALID
    assert L.awt_op_embed_backward(p, p, None, p, p, 24, 12, 128, 0, 512, None) == INVALID
    assert L.awt_op_embed_backward(p, p, p, None, p, 24, 12, 128, 0, 512, None) == INVALID
    assert L.awt_op_embed_backward(p, p, p, p, None, 24, 12, 128, 0, 512, None) == INVALID
    for M, Lq, d, pos0, vocab in [(0, 12, 128, 0, 512), (24, 0, 128, 0, 512), (24, 12, 0, 0, 512), (24, 12, 128, 0, 0), (24, 12, 130, 0, 512),
                                  (25, 12, 128, 0, 512), (24, 12, 128, -1, 512), (24, 12, 4096, 0, 512)]:
        assert L.awt_op_embed_backward(p, p, p, p, p, M, Lq, d, pos0, vocab, None) == INVALID, (M, Lq, d, pos0, vocab)


def test_pitched_column_sums_argument_errors():
    L = _lib.lib()
    p = C.c_void_p(4096)
    big = 1 << 30
    assert L.awt_op_column_sums_ld(None, p, 384, 0, 128, p, 37, 0, p, big, None) == INVALID and "op_column_sums_ld" in _err()
    assert L.awt_op_column_sums_ld(p, None, 384, 0, 128, p, 37, 0, p, big, None) == INVALID
    assert L.awt_op_column_sums_ld(p, p, 384, 0, 128, None, 37, 0, p, big, None) == INVALID
    assert L.awt_op_column_sums_ld(p, p, 384, 0, 128, p, 37, 0, None, big, None) == INVALID
    assert L.awt_op_column_sums_ld(p, p, 384, 0, 128, p, 0, 0, p, big, None) == INVALID          # no rows
    assert L.awt_op_column_sums_ld(p, p, 384, 0, 0, p, 37, 0, p, big, None) == INVALID           # no columns
    assert L.awt_op_column_sums_ld(p, p, 384, 0, 126, p, 37, 0, p, big, None) == INVALID and "multiples of 4" in _err()
    assert L.awt_op_column_sums_ld(p, p, 384, 2, 128, p, 37, 0, p, big, None) == INVALID
    assert L.awt_op_column_sums_ld(p, p, 384, 320, 128, p, 37, 0, p, big, None) == INVALID       # the window leaves the row
    assert L.awt_op_column_sums_ld(p, p, 384, 0, 128, p, 300, 0, p, 16, None) == -3              # AWT_ERR_WORKSPACE
    assert L.awt_op_column_sums_ld_workspace_bytes(0, 128) == 0 and L.awt_op_column_sums_ld_workspace_bytes(300, 128) == 2 * 128 * 4


def test_weight_update_argument_errors():
    L = _lib.lib()
    p = C.c_void_p(4096)
    assert L.awt_weight_update(p, None, p, None, None) == INVALID and "weight_update" in _err()      # a null handle
    assert L.awt_weight_update(None, None, p, None, None) == INVALID
