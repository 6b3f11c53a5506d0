"""CPU: Whisper's generation config -- generation_config.json through checkpoint.py, and the prompt generate forces (HF 5.15
`_retrieve_init_tokens`) against the prompts tools/make_golden_generate.py recorded from transformers (tests/golden/generate.npz)."""
import json

import numpy as np
import pytest

from mlx8_ws_audio_transformer_amd import generation as G
from tests.util import golden


def _gc(key="generation_config"):
    return G.GenerationConfig.from_dict(json.loads(str(golden("generate.npz")[key])))


def test_generation_config_json_round_trips_through_checkpoint(tmp_path):
    from mlx8_ws_audio_transformer_amd import checkpoint as ck
    assert ck.load_generation_config(str(tmp_path)) is None                 # a directory without one loads as before
    gc = _gc()
    gc.language, gc.task = "en", "transcribe"                               # what AB/fineTune.py:132-134 sets before training
    gc.extra["return_timestamps"] = False
    gc.save(str(tmp_path))
    back = ck.load_generation_config(str(tmp_path))
    assert back.to_dict() == gc.to_dict()
    assert back.language == "en" and back.lang_to_id == gc.lang_to_id and back.suppress_tokens == gc.suppress_tokens
    assert back.extra == {"return_timestamps": False} and back.whisper_prompt


def test_constructed_config_has_no_whisper_prompt():
    gc = G.GenerationConfig(decoder_start_token_id=50258, pad_token_id=50257, eos_token_id=50257, max_length=225)
    assert not gc.whisper_prompt and gc.num_beams == 1 and gc.lang_to_id is None


@pytest.mark.parametrize("case,language,task", [("a", "en", "transcribe"), ("b", "en", None), ("e", ["en", "fr", "de", "en"], None)])
def test_prompt_matches_transformers(case, language, task):
    F = golden("generate.npz")
    gc = _gc()
    G.set_language_and_task(gc, language, task, None)
    init = G.retrieve_init_tokens(gc, F["init_" + case].shape[0])
    np.testing.assert_array_equal(np.array(init), F["init_" + case])


def test_prompt_with_language_detection_matches_transformers():
    F = golden("generate.npz")
    gc = _gc()
    calls = []

    def detect():
        calls.append(1)
        return F["detected_c"].tolist()

    init = G.retrieve_init_tokens(gc, F["init_c"].shape[0], detect=detect)
    assert calls == [1]
    np.testing.assert_array_equal(np.array(init), F["init_c"])


def test_prompt_from_forced_decoder_ids_matches_transformers():
    F = golden("generate.npz")
    gc = _gc("generation_config_d")
    assert gc.lang_to_id is None and gc.forced_decoder_ids is not None and gc.whisper_prompt
    init = G.retrieve_init_tokens(gc, F["init_d"].shape[0], detect=lambda: pytest.fail("no detection with a forced language"))
    np.testing.assert_array_equal(np.array(init), F["init_d"])


def test_prompt_errors_are_transformers_errors():
    gc = _gc()
    with pytest.raises(ValueError, match="Unsupported language: xx"):
        G.set_language_and_task(gc, "xx", None, None)
        G.retrieve_init_tokens(gc, 1)
    gc = _gc()
    with pytest.raises(ValueError, match="is not supported by this specific model"):
        G.set_language_and_task(gc, "hindi", None, None)                    # a known language missing from this config's lang_to_id
        G.retrieve_init_tokens(gc, 1)
    gc = _gc()
    gc.is_multilingual = False
    with pytest.raises(ValueError, match="English-only"):
        G.set_language_and_task(gc, "en", None, None)
    with pytest.raises(ValueError, match="lang_to_id"):
        G.set_language_and_task(_gc("generation_config_d"), "en", None, None)
    gc = _gc()
    G.set_language_and_task(gc, ["en", "fr"], None, None)
    with pytest.raises(ValueError, match="length of the list must match the batch size"):
        G.retrieve_init_tokens(gc, 3)
    gc = _gc()
    G.set_language_and_task(gc, None, "dictate", None)
    with pytest.raises(ValueError, match="task is not supported"):
        G.retrieve_init_tokens(gc, 1, detect=lambda: [500])


def test_banned_bits_layout():
    import torch
    bits = G.banned_bits([0, 31, 32, 511, 600], 512, "cpu")
    words = bits.to(torch.int64) & 0xFFFFFFFF
    assert words.shape == (16,) and int(words[0]) == (1 | (1 << 31)) and int(words[1]) == 1 and int(words[15]) == 1 << 31
    inv = G.banned_bits([3], 35, "cpu", invert=True).to(torch.int64) & 0xFFFFFFFF
    assert int(inv[0]) == 0xFFFFFFFF & ~(1 << 3) and int(inv[1]) == 0b111                # columns >= vocab stay clear


def test_strip_prompt_follows_whisper_short_form_return():
    import torch
    seqs = torch.tensor([[1, 500, 7, 8, 2, 2, 2], [1, 500, 7, 9, 10, 11, 12], [1, 500, 2, 2, 2, 2, 2]])
    out = G.strip_prompt(seqs, 2, pad_id=2, eos_id=2)
    assert out.tolist() == [[7, 8, 2, 2, 2], [7, 9, 10, 11, 12], [2, 2, 2, 2, 2]]
