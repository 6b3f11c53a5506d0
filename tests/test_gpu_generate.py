"""GPU: Whisper generate -- the token-selection and cache-gather kernels against torch, and the decode loop against
WhisperForConditionalGeneration.generate (transformers 5.15) on the fixture of tools/make_golden_generate.py."""
import json

import numpy as np
import pytest
import torch

from mlx8_ws_audio_transformer_amd import _lib, generation as G, weights as wts
from tests.util import golden

pytestmark = pytest.mark.gpu

WHISPER_SUPPRESS = [1, 2, 7, 8, 9, 10, 14, 25, 26, 27, 28, 29, 31, 58, 59, 60, 61, 62, 63, 90, 91, 92, 93, 359, 503, 522, 542, 873, 893, 902,
                    918, 922, 931, 1350, 1853, 1982, 2460, 2627, 3246, 3253, 3268, 3536, 3846, 3961, 4183, 4667, 6585, 6647, 7273, 9061, 9383,
                    10428, 10929, 11938, 12033, 12331, 12562, 13793, 14157, 14635, 15265, 15618, 16553, 16604, 18362, 18956, 20075, 21675,
                    22520, 26130, 26161, 26435, 28279, 29464, 31650, 32302, 32470, 36865, 42863, 47425, 49870, 50254, 50258, 50358, 50359,
                    50360, 50361, 50362]


def _reference(x, vocab, beams, banned, bs, log_softmax, k):
    """torch: log-softmax over the vocabulary, banned -> -inf, + beam score, stable descending sort over the clip's beams x vocab."""
    x = x[:, :vocab].double().float()
    s = torch.log_softmax(x, dim=-1) if log_softmax else x.clone()
    if banned:
        s[:, list(banned)] = float("-inf")
    if bs is not None:
        s = s + bs[:, None]
    flat = s.reshape(-1, beams * vocab)
    vals, idx = torch.sort(flat, dim=1, descending=True, stable=True)
    return vals[:, :k], idx[:, :k] % vocab, (idx[:, :k] // vocab).to(torch.int32)


CASES = [(1, 512, 1), (5, 512, 5), (64, 512, 8), (80, 512, 4), (1, 51865, 1), (5, 51865, 1), (64, 51865, 2), (80, 51865, 5),
         (80, 51866, 8), (64, 51866, 4), (5, 51866, 5), (16, 51865, 1)]


@pytest.mark.parametrize("rows,vocab,beams", CASES)
@pytest.mark.parametrize("ban", ["none", "whisper", "languages"])
def test_select_tokens_matches_torch(rows, vocab, beams, ban):
    g = torch.Generator(device="cuda").manual_seed(rows * 7 + vocab + beams)
    ld = vocab + (-vocab) % 128 + 128                                          # padded pitch, like PackedLinear's Np
    x = torch.randn((rows, ld), generator=g, device="cuda") * 3
    x[:, vocab:] = 1e4                                                         # padding columns must never be chosen
    banned = {"none": [], "whisper": [t % vocab for t in WHISPER_SUPPRESS],
              "languages": sorted(set(range(vocab)) - set(range(min(50259, vocab - 100), min(50358, vocab))))}[ban]
    bits = G.banned_bits(banned, vocab, "cuda")
    bs = torch.randn(rows, generator=g, device="cuda") * 2 if beams > 1 else None
    for log_softmax, k in ((True, 2 * beams), (False, 1), (True, min(16, beams * vocab))):
        got = G.select_tokens(x, vocab, beams, bits, bs, log_softmax, k)
        ref = _reference(x, vocab, beams, set(banned), bs, log_softmax, k)
        fin = torch.isfinite(ref[0])
        np.testing.assert_array_equal(got[1].cpu().numpy(), ref[1].cpu().numpy())
        np.testing.assert_array_equal(got[2].cpu().numpy(), ref[2].cpu().numpy())
        assert torch.equal(torch.isfinite(got[0]), fin)
        torch.testing.assert_close(got[0][fin], ref[0][fin], rtol=1e-5, atol=1e-5)


def test_select_greedy_ties_inf_and_nan_follow_argmax():
    vocab, ld = 51865, 51968
    x = torch.randn((6, ld), device="cuda")
    x[0, 100] = x[0, 40000] = 50.0                                            # a tie: the lower index wins
    x[1, :vocab] = float("-inf")                                               # an all -inf row: index 0
    x[2, 777] = float("nan"); x[2, 33] = float("nan")                          # NaN wins, the first one
    x[3, 5] = float("inf")
    x[4, 3000:] = 7.0; x[4, :3000] = -1.0                                      # a long run of equal values
    x[5, 10] = 99.0                                                            # banned: not chosen
    bits = G.banned_bits([10], vocab, "cuda")
    got = G.select_tokens(x, vocab, 1, bits, None, False, 1)[1][:, 0]
    ref = x[:, :vocab].clone()
    ref[:, 10] = float("-inf")
    np.testing.assert_array_equal(got.cpu().numpy(), ref.argmax(dim=-1).cpu().numpy())
    assert got.tolist()[:5] == [100, 0, 33, 5, 3000]


@pytest.mark.parametrize("src_rows,dst_rows", [(4, 4), (3, 15), (16, 80)])
def test_kv_gather_equals_index_select(src_rows, dst_rows):
    from mlx8_ws_audio_transformer_amd.native_decoder import kv_gather
    layers, Tmax, width, T = 3, 37, 1536, 29
    src = torch.randn((layers, src_rows, Tmax, width), device="cuda")
    dst = torch.full((layers, dst_rows, Tmax, width), -7.0, device="cuda")
    if src_rows == dst_rows:
        parent = torch.randperm(src_rows, device="cuda")
    else:
        parent = torch.arange(dst_rows, device="cuda") // (dst_rows // src_rows)   # the B -> B x beams expansion
    kv_gather(src, dst, parent, layers, src_rows, dst_rows, T, Tmax, width)
    ref = src.index_select(1, parent)
    assert torch.equal(dst[:, :, :T], ref[:, :, :T])
    assert bool((dst[:, :, T:] == -7.0).all())                                # positions >= T untouched


def test_bad_arguments_fail_through_ctypes():
    L = _lib.lib()
    ctx = _lib.ctx()
    x = torch.zeros((8, 512), device="cuda")
    out_s = torch.empty(64, device="cuda"); out_t = torch.empty(64, dtype=torch.int64, device="cuda"); out_p = torch.empty(64, dtype=torch.int32, device="cuda")
    ws = torch.empty(1 << 20, dtype=torch.uint8, device="cuda")
    s = _lib.stream_handle()

    def sel(rows=8, vocab=512, ld=512, beams=1, k=1, wsb=ws.numel(), logits=x.data_ptr()):
        return L.awt_op_select_tokens(ctx, logits, ld, rows, vocab, beams, None, None, 1, k, out_s.data_ptr(), out_t.data_ptr(), out_p.data_ptr(),
                                      ws.data_ptr(), wsb, s)

    assert sel() == 0
    for bad in (dict(beams=9, rows=9), dict(k=17), dict(rows=6, beams=4), dict(ld=510, vocab=500), dict(vocab=600), dict(wsb=16),
                dict(logits=x.data_ptr() + 4), dict(k=3, vocab=1, beams=2, rows=8)):
        assert sel(**bad) != 0, bad
        assert L.awt_last_error().decode()
    src = torch.zeros((1, 2, 4, 8), device="cuda"); dst = torch.zeros_like(src); parent = torch.zeros(2, dtype=torch.int32, device="cuda")
    assert L.awt_op_kv_gather(ctx, src.data_ptr(), dst.data_ptr(), parent.data_ptr(), 1, 2, 2, 4, 4, 8, s) == 0
    assert L.awt_op_kv_gather(ctx, src.data_ptr(), src.data_ptr(), parent.data_ptr(), 1, 2, 2, 4, 4, 8, s) != 0         # in place
    assert L.awt_op_kv_gather(ctx, src.data_ptr(), dst.data_ptr(), parent.data_ptr(), 1, 2, 2, 5, 4, 8, s) != 0         # T > Tmax
    assert L.awt_op_kv_gather(ctx, src.data_ptr(), dst.data_ptr(), parent.data_ptr(), 1, 2, 2, 4, 4, 6, s) != 0         # width % 4
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ against transformers
def _fixture_model(F, gc_key="generation_config"):
    """WhisperLoRAModel (inference) with the fixture's weights (tools/make_golden_generate.py: encoder_weights / decoder_weights)."""
    from mlx8_ws_audio_transformer_amd.finetune import WhisperLoRAModel
    cfg = wts.config("mini", True)
    We, Wd = _fixture_weights(F, cfg)
    model = WhisperLoRAModel(cfg, None, decoder_layers=2, vocab=512, max_target_positions=64)
    model.encoder.load_state_dict({k: torch.from_numpy(v) for k, v in We.items()}, strict=False)
    model.decoder.load_state_dict({k: torch.from_numpy(v) for k, v in Wd.items()}, strict=True)
    model.generation_config = G.GenerationConfig.from_dict(json.loads(str(F[gc_key])))
    return model.eval(), _fixture_mel(cfg)


def _fixture_weights(F, cfg):
    We = wts.init_encoder_weights(cfg, seed=0, profile="test")
    for k in ("conv1.weight", "conv2.weight"):
        We[k] = We[k] * np.float32(F["conv_scale"])
    Wd = wts.init_decoder_weights(cfg.d_model, 2, cfg.ffn, 512, 64, seed=int(F["dec_seed"]))
    Wd["embed_positions.weight"] = Wd["embed_positions.weight"] * np.float32(F["pos_scale"])
    for k in [k for k in Wd if "encoder_attn.v_proj" in k]:
        Wd[k] = Wd[k] * np.float32(F["cross_scale"])
    for k in ("layer_norm.weight", "layer_norm.bias"):
        Wd[k] = Wd[k] * np.float32(F["logit_scale"])
    Wd["embed_tokens.weight"] = Wd["embed_tokens.weight"].copy()
    Wd["embed_tokens.weight"][2] *= np.float32(F["eos_scale"])
    return We, Wd


def _fixture_mel(cfg):
    from mlx8_ws_audio_transformer_amd import synth
    from oracle import logmel as oracle_mel
    piano = [synth.pcm_i16_to_f32(c) for c in synth.synth_clips_i16(3, seed=1234, first=0)]
    clips = [piano[0], synth.tone_noise_clip(0)[:64000], (0.1 * wts.unit_variates("f2_noise", 64000, 0)).astype(np.float32), piano[2]]
    return torch.from_numpy(oracle_mel.whisper_logmel(clips, n_samples=2 * cfg.max_source_positions * 160)).cuda()


def test_fixture_cases_match_transformers():
    F = golden("generate.npz")
    model, mel = _fixture_model(F)
    n = int(F["max_length"])
    out = model.generate(mel, max_length=n, language="en", task="transcribe").cpu().numpy()
    np.testing.assert_array_equal(out, F["seq_a"])
    gc = model.generation_config
    model.generation_config = G.GenerationConfig.from_dict({**gc.to_dict(), "suppress_tokens": None, "begin_suppress_tokens": None})
    np.testing.assert_array_equal(model.generate(mel, max_length=n, language="en", task="transcribe").cpu().numpy(), F["seq_a_unsuppressed"])
    model.generation_config = gc
    for key in [k[len("seq_"):] for k in F.files if k.startswith("seq_b_")]:
        _, nb, lp, es = key.split("_")
        res = model.generate(mel, max_length=n, language="en", num_beams=int(nb), length_penalty=float(lp.replace("p", ".")), early_stopping=bool(int(es)),
                             return_dict_in_generate=True)
        np.testing.assert_array_equal(res.sequences.cpu().numpy(), F["seq_" + key], err_msg=key)
        np.testing.assert_allclose(res.sequences_scores.cpu().numpy(), F["score_" + key], rtol=0, atol=1e-3, err_msg=key)
    np.testing.assert_array_equal(model.detect_language(mel).cpu().numpy(), F["detected_c"])
    np.testing.assert_array_equal(model.generate(mel, max_length=n).cpu().numpy(), F["seq_c"])
    np.testing.assert_array_equal(model.generate(mel, max_length=n, language=["en", "fr", "de", "en"]).cpu().numpy(), F["seq_e"])
    model_d, _ = _fixture_model(F, "generation_config_d")
    np.testing.assert_array_equal(model_d.generate(mel, max_length=n).cpu().numpy(), F["seq_d"])


def test_unsupported_generate_arguments_raise():
    F = golden("generate.npz")
    model, mel = _fixture_model(F)
    for kw, msg in ((dict(return_timestamps=True), "return_timestamps"), (dict(do_sample=True), "do_sample"),
                    (dict(num_return_sequences=2), "num_return_sequences"), (dict(num_beams=9), "num_beams")):
        with pytest.raises(ValueError, match=msg):
            model.generate(mel, **kw)
    with pytest.raises(ValueError, match="window"):
        model.generate(torch.cat([mel, mel], dim=-1))
    with pytest.raises(TypeError, match="prompt_ids"):
        model.generate(mel, prompt_ids=torch.tensor([1]))
    plain, _ = _fixture_model(F)
    plain.generation_config = G.GenerationConfig(decoder_start_token_id=1, pad_token_id=2, eos_token_id=2, max_length=10)
    with pytest.raises(ValueError, match="lang_to_id"):
        plain.generate(mel, language="en")


def test_checkpoint_directory_with_generation_config_reproduces_case_a(tmp_path):
    from mlx8_ws_audio_transformer_amd import checkpoint as ck
    from mlx8_ws_audio_transformer_amd.finetune import WhisperLoRAModel
    F = golden("generate.npz")
    cfg = wts.config("mini", True)
    We, Wd = _fixture_weights(F, cfg)
    hf = {"architectures": ["WhisperForConditionalGeneration"], "model_type": "whisper", "d_model": cfg.d_model, "encoder_layers": cfg.layers,
          "encoder_attention_heads": cfg.heads, "encoder_ffn_dim": cfg.ffn, "decoder_layers": 2, "decoder_attention_heads": cfg.heads, "decoder_ffn_dim": cfg.ffn,
          "num_mel_bins": 80, "max_source_positions": cfg.max_source_positions, "max_target_positions": 64, "vocab_size": 512,
          "decoder_start_token_id": 1, "pad_token_id": 2, "eos_token_id": 2}
    path = ck.save_pretrained_dir(str(tmp_path / "whisper-small-hi"), hf, {k: torch.from_numpy(v) for k, v in We.items()},
                                  {k: torch.from_numpy(v) for k, v in Wd.items()})
    gc = G.GenerationConfig.from_dict(json.loads(str(F["generation_config"])))
    gc.language, gc.task = "en", "transcribe"                                  # AB/fineTune.py:132-134, saved by trainer.save_model()
    gc.save(path)
    model = WhisperLoRAModel.from_pretrained(path).eval()
    assert model.generation_config.language == "en"
    mel = _fixture_mel(cfg)
    np.testing.assert_array_equal(model.generate(mel, max_length=int(F["max_length"])).cpu().numpy(), F["seq_a"])
    out = tmp_path / "again"
    model.save_pretrained(str(out))
    assert ck.load_generation_config(str(out)).to_dict() == gc.to_dict()


def _beam_inputs(model, mel, language="en"):
    gc = model.generation_config
    hidden = model.encoder(mel).last_hidden_state
    cross = model.decoder.cross_kv(hidden, model.precision)
    g2 = G.GenerationConfig.from_dict(gc.to_dict())
    G.set_language_and_task(g2, language, None, None)
    init = torch.tensor(G.retrieve_init_tokens(g2, mel.shape[0]), device=mel.device)
    return hidden, cross, init, g2


@torch.no_grad()
def test_beam_path_with_one_beam_equals_greedy_and_batch_equals_single_clips():
    F = golden("generate.npz")
    model, mel = _fixture_model(F)
    hidden, cross, init, gc = _beam_inputs(model, mel)
    max_len = init.shape[1] + int(F["max_length"])
    g = G.greedy(model._decode_steps(hidden, cross, mel.shape[0], max_len), init, max_len, 2, 2, gc.suppress_tokens, gc.begin_suppress_tokens)
    b, _, lens = G.beam_search(model._decode_steps(hidden, cross, mel.shape[0], max_len), init, max_len, 2, 2, gc.suppress_tokens,
                               gc.begin_suppress_tokens, 1, 1.0, False)
    for r in range(mel.shape[0]):
        n = init.shape[1] + int(lens[r])
        assert g[r, :n].tolist() == b[r, :n].tolist()
    full = model.generate(mel, max_length=int(F["max_length"]), language="en", num_beams=4, return_dict_in_generate=True)
    for r in range(mel.shape[0]):
        one = model.generate(mel[r:r + 1], max_length=int(F["max_length"]), language="en", num_beams=4, return_dict_in_generate=True)
        w = one.sequences.shape[1]
        assert full.sequences[r, :w].tolist() == one.sequences[0].tolist() and bool((full.sequences[r, w:] == 2).all())
        assert abs(float(full.sequences_scores[r]) - float(one.sequences_scores[0])) < 1e-4


@torch.no_grad()
def test_whisper_small_shaped_beam_search_scores_match_teacher_forced_rescoring():
    """B = 16, 5 beams, vocab 51 865, 12 layers of d 768, max_length 225 on random encoder states: each returned hypothesis' score equals
    the length-penalised sum of its tokens' log-probabilities under a full (uncached) decoder forward."""
    from mlx8_ws_audio_transformer_amd.native_decoder import NativeWhisperDecoder
    torch.manual_seed(0)
    d, nl, ffn, vocab, S, B, nb = 768, 12, 3072, 51865, 1500, 16, 5
    dec = NativeWhisperDecoder(d, nl, 12, ffn, vocab, 448).cuda()
    with torch.no_grad():
        for name, p in dec.named_parameters():
            if "layer_norm.weight" in name:
                p.copy_(1.0 + 0.1 * torch.randn_like(p))
            elif name.endswith("bias") or "layer_norm" in name:
                p.copy_(0.02 * torch.randn_like(p))
            elif "embed" in name:
                p.copy_((0.5 if "positions" in name else 0.1) * torch.randn_like(p))
            else:
                p.copy_(torch.randn_like(p) * (0.5 / p.shape[1] ** 0.5))
    hidden = torch.randn((B, S, d), device="cuda")
    cross = dec.cross_kv(hidden)
    init = torch.tensor([[50258, 50259, 50359, 50363]] * B, device="cuda")
    P, max_len, lp = init.shape[1], init.shape[1] + 225, 1.0
    steps = G._NativeSteps(dec, cross, S, B, max_len)
    seqs, scores, lens = G.beam_search(steps, init, max_len, 50257, 50257, None, None, nb, lp, False)
    assert seqs.shape[0] == B and bool(torch.isfinite(scores).all())
    logits = dec(seqs[:, :-1], hidden, cross=cross).float()
    logp = torch.log_softmax(logits, dim=-1)
    tok = torch.gather(logp[:, P - 1:], 2, seqs[:, P:, None])[:, :, 0]
    for r in range(B):
        n = int(lens[r])
        ref = float(tok[r, :n].double().sum()) / (n ** lp)
        assert abs(ref - float(scores[r])) < 1e-3, (r, n, ref, float(scores[r]))
