"""GPU: `copy.deepcopy` of a model that has cached library handles (native_decoder.PackedSet, autograd_ops.PackedCache, the encoder's handle).  The copy
computes the same bits on handles of its own, and dropping it leaves the original's handles alive and in place: the original computes the same bits
again, through the same objects.  (tests/test_packed_set_host.py pins the copy rule itself, without a GPU.)"""
import copy
import gc

import numpy as np
import pytest
import torch

from mlx8_ws_audio_transformer_amd import weights as wts
from tests import qwen3_reference as qr

pytestmark = pytest.mark.gpu


def _variates(name, *shape):
    return torch.from_numpy(wts.unit_variates("packed_copy." + name, int(np.prod(shape)), 5).reshape(shape).astype(np.float32))


def _check(model, run, objects):
    """run(model) -> output tensor; objects(model) -> the handle owners the model caches, in a fixed order (non-empty after a run)."""
    def addresses(objs):
        return {o.handle if hasattr(o, "handle") else o.buf.data_ptr() for o in objs}

    with torch.no_grad():
        want = run(model).detach().clone()
        mine = objects(model)
        assert mine and None not in addresses(mine) and 0 not in addresses(mine)
        twin = copy.deepcopy(model)
        assert torch.equal(run(twin).detach(), want)
        theirs = objects(twin)
        assert len(theirs) == len(mine) and not addresses(theirs) & addresses(mine)
        del twin, theirs
        gc.collect()
        torch.cuda.synchronize()
        assert torch.equal(run(model).detach(), want)
        again = objects(model)
        assert len(again) == len(mine) and all(a is b for a, b in zip(again, mine))


def _packed_objects(pk):
    out = [v for v in pk.values() if not isinstance(v, list)]
    for group in (v for v in pk.values() if isinstance(v, list)):
        for slot in group:
            out += list(slot.values())
    return out


def test_whisper_decoder_copy_packs_its_own_weights():
    from mlx8_ws_audio_transformer_amd.native_decoder import NativeWhisperDecoder
    cfg = wts.config("mini", True)
    dec = NativeWhisperDecoder(cfg.d_model, 2, cfg.heads, cfg.ffn, 512, 64)
    dec.load_state_dict({k: torch.from_numpy(v) for k, v in wts.init_decoder_weights(cfg.d_model, 2, cfg.ffn, 512, 64, seed=0).items()}, strict=True)
    dec = dec.cuda()
    ids = ((torch.arange(8).reshape(2, 4) * 61 + 7) % 512).cuda()
    enc = _variates("enc", 2, 8, cfg.d_model).cuda()
    _check(dec, lambda m: m(ids, enc), lambda m: _packed_objects(m.packed()))
    assert len(_packed_objects(dec.packed())) == 22


def test_qwen3_decoder_copy_packs_its_own_weights():
    from mlx8_ws_audio_transformer_amd.music2midi import Qwen3Decoder
    cfg = qr.config(qr.MICRO, True)
    dec = Qwen3Decoder(cfg)
    dec.load_state_dict({k: v.float() for k, v in qr.state_dict(cfg, seed=11).items()}, strict=True)
    dec = dec.cuda()
    x = _variates("x", 2, 5, cfg.hidden_size).cuda()
    _check(dec, lambda m: m(x), lambda m: _packed_objects(m._pack()))
    assert len(_packed_objects(dec._pack())) == 9


def test_classifier_copy_in_eval_packs_its_own_weights():
    from mlx8_ws_audio_transformer_amd.urbansound_classifier import TransformerUrbanSound8KClassifier
    torch.manual_seed(3)
    nat = TransformerUrbanSound8KClassifier(n_mels=64).cuda().eval()
    x = _variates("mel", 2, 64, 126).cuda() * 2.0 - 4.0
    _check(nat, lambda m: m(x), lambda m: [hit[1] for hit in m._packed.items.values()])
    assert len(nat._packed.items) >= 8


def test_encoder_copy_builds_its_own_handle():
    from mlx8_ws_audio_transformer_amd.encoder import NativeWhisperEncoder
    enc = NativeWhisperEncoder(wts.config("mini", True), precision="bf16x3")        # explicit precision: no load-time probe
    mel = _variates("mel", 2, 80, 400).cuda()
    with torch.no_grad():
        want = enc(mel).last_hidden_state.clone()
        mine = enc._handle
        assert mine and len(enc._synced) == len(list(enc.parameters()))
        twin = copy.deepcopy(enc)
        assert twin._handle is None and twin._synced == {} and twin._ws is None and twin.precision == "bf16x3"
        assert torch.equal(twin(mel).last_hidden_state, want)
        assert twin._handle not in (None, mine) and enc._handle == mine
        del twin
        gc.collect()
        torch.cuda.synchronize()
        assert torch.equal(enc(mel).last_hidden_state, want) and enc._handle == mine
