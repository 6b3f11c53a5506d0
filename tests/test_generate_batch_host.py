"""CPU checks of the batch fixture of tests/test_gpu_generate_batch.py (tests/qwen3_batch_reference.py), from the float64 restatement alone, and of the
refusals of `MusicTranscriptionModel.generate_batch` that need no GPU."""
import pytest
import torch

from mlx8_ws_audio_transformer_amd import music2midi as m2m
from tests import qwen3_batch_reference as br
from tests import qwen3_reference as qr


def test_batch_fixture_conditions():
    """What makes the exact-token comparison of the GPU test fair, per clip, as tests/test_qwen3_reference_host.py::test_greedy_fixture_conditions has it:
    every step's top-2 margin is at least 10 x the GPU logit bound and the EOS id is never the argmax.  And what makes the batch test tell rows apart:
    the three token lists differ pairwise, and there is a token that clip 0 emits at a step j >= 2 before the other two clips do."""
    ref = br.reference()
    tokens = [t for t, _ in ref]
    for i, (toks, logits) in enumerate(ref):
        margin, bound = br.margins(logits)
        print(f"clip {i}: {len(set(toks))} distinct tokens, smallest top-2 margin {margin:.4f}, GPU logit bound {bound:.5f} "
              f"(max |logit| {float(logits.abs().max()):.2f}), tokens {toks}")
        assert len(toks) == qr.GREEDY_STEPS and qr.GREEDY_EOS not in toks
        assert margin >= 10 * bound
    assert all(tokens[i] != tokens[j] for i in range(br.CLIPS) for j in range(i))
    case = br.eos_case(tokens)
    print("EOS case (token, step of clip 0):", case)
    assert case is not None
    t, j = case
    assert j >= 2 and tokens[0].index(t) == j and all(t not in other[:j + 1] for other in tokens[1:])


def test_batch_seed_is_the_first_that_qualifies():
    """The recorded seed satisfies `conditions`, and the seed before it does not (the whole search is `python -m tests.qwen3_batch_reference`)."""
    assert br.conditions(br.BATCH_SEED)
    assert br.BATCH_SEED == 0 or not br.conditions(br.BATCH_SEED - 1)


def _tiny_model(tokenizer=None):
    cfg = m2m.Qwen3Config(vocab_size=64, hidden_size=128, intermediate_size=64, num_hidden_layers=1, num_attention_heads=2, num_key_value_heads=1,
                          rms_norm_eps=1e-6, rope_theta=1e6, tie_word_embeddings=True, max_position_embeddings=32)
    tower = lambda waveforms, sampling_rate: torch.zeros(len(waveforms), 4, 128)
    return m2m.MusicTranscriptionModel(tower, m2m.CrossAttentionAdapter(128, 128, num_heads=1), m2m.Qwen3Decoder(cfg), tokenizer)


def test_generate_batch_refusals_need_no_gpu():
    model = _tiny_model()
    with pytest.raises(ValueError, match="at least one clip"):
        model.generate_batch([], 16000, bos_token_id=1, eos_token_id=2)
    with pytest.raises(ValueError, match="bos_token_id and eos_token_id"):
        model.generate_batch([None], 16000)
    with pytest.raises(ValueError, match="bos_token_id and eos_token_id"):
        model.generate_batch([None], 16000, bos_token_id=1)
    with pytest.raises(ValueError, match="temperature"):
        model.generate_batch([None], 16000, temperature=0.0, bos_token_id=1, eos_token_id=2)
    with pytest.raises(ValueError, match="prompt token"):
        model.generate_batch([None], 16000, bos_token_id=[], eos_token_id=2)
    with pytest.raises(ValueError, match="bos_token_id and eos_token_id"):
        model.generate(None, 16000)                                        # the one-clip form refuses the same way


def test_linear_decode_refuses_bad_arguments_before_touching_a_gpu():
    from mlx8_ws_audio_transformer_amd import _lib
    L, p = _lib.lib(), 256                                                 # any non-null value: every refusal below comes before a dereference
    err = lambda: L.awt_last_error().decode()
    assert L.awt_linear_decode(None, None, None, None, None, 1, None) == -1 and "linear_decode" in err()      # AWT_ERR_INVALID: null arguments
    assert L.awt_linear_decode(p, None, p, None, p, 1, None) == -1 and "null argument" in err()                # a null handle
