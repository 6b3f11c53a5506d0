"""CPU checks around music2midi.Qwen3Decoder: the float64 restatement the GPU tests measure against (tests/qwen3_reference.py) agrees with Hugging Face's
`Qwen3ForCausalLM` where `transformers` is installed; the fixture conditions the GPU tests rely on hold, from the restatement alone; and the module's
refusals, its state-dict names and the workspace query work without a GPU."""
import pytest
import torch

from mlx8_ws_audio_transformer_amd import music2midi as m2m
from tests import qwen3_reference as qr

GPU_LOGIT_TOL = 1e-3                  # tests/test_gpu_qwen3_decoder.py: logits max-abs <= 1e-3 * max(1, max |reference logits|)


@pytest.mark.parametrize("tied", [True, False])
def test_restatement_agrees_with_hf_qwen3(tied):
    """Micro config in float64.  HF computes its RMSNorm and its rotary table in fp32 even in a float64 model, so the two agree at fp32 level: bound
    2e-6 * max |logits|.  The masked run (right padding) equals the unmasked one on the live rows."""
    transformers = pytest.importorskip("transformers")
    cfg = qr.config(qr.MICRO, tied)
    hf_cfg = transformers.Qwen3Config(vocab_size=cfg.vocab_size, hidden_size=cfg.hidden_size, intermediate_size=cfg.intermediate_size,
                                      num_hidden_layers=cfg.num_hidden_layers, num_attention_heads=cfg.num_attention_heads,
                                      num_key_value_heads=cfg.num_key_value_heads, head_dim=128, rms_norm_eps=cfg.rms_norm_eps, rope_theta=cfg.rope_theta,
                                      tie_word_embeddings=tied, max_position_embeddings=cfg.max_position_embeddings, attention_bias=False,
                                      use_sliding_window=False, attn_implementation="eager")
    hf = transformers.Qwen3ForCausalLM(hf_cfg).double().eval()
    sd = qr.state_dict(cfg, seed=3)
    hf_sd = dict(sd)
    if tied:
        hf_sd["lm_head.weight"] = sd["model.embed_tokens.weight"]
    hf.load_state_dict(hf_sd, strict=True)
    x = qr.variates("host.x", (2, 37, cfg.hidden_size), 3)
    labels = torch.from_numpy(__import__("numpy").arange(2 * 37).reshape(2, 37) * 7 % cfg.vocab_size)
    with torch.no_grad():
        out = hf(inputs_embeds=x, labels=labels)
        mask = torch.ones(2, 37, dtype=torch.long)
        mask[1, 29:] = 0
        masked = hf(inputs_embeds=x, attention_mask=mask).logits
    ref = qr.forward(sd, cfg, x)
    err, mag = float((ref - out.logits).abs().max()), float(ref.abs().max())
    print(f"tied={tied}: restatement vs HF max-abs {err:.3e} at max |logits| {mag:.1f} ({err / mag:.2e} relative; bound 2e-6)")
    assert err <= 2e-6 * mag
    loss = qr.causal_lm_loss(ref, labels)
    print(f"loss {float(loss):.6f} vs HF {float(out.loss):.6f}")
    assert abs(float(loss) - float(out.loss)) <= 2e-6 * max(1.0, abs(float(loss)))
    assert torch.equal(masked[0], out.logits[0]) and torch.equal(masked[1, :29], out.logits[1, :29])


def test_right_padding_needs_no_key_mask():
    """Causality alone: the logits at a row's live positions do not depend on what follows them, so a right-padded batch needs no key mask."""
    cfg = qr.config(qr.MICRO, True)
    sd = qr.state_dict(cfg, seed=4)
    x = qr.variates("host.pad", (1, 37, cfg.hidden_size), 4)
    full, short = qr.forward(sd, cfg, x), qr.forward(sd, cfg, x[:, :29])
    err = float((full[:, :29] - short).abs().max())
    print("live rows, padded vs unpadded: max-abs", err)
    assert err <= 1e-12 * float(full.abs().max())


def test_greedy_fixture_conditions():
    """What makes the exact-token comparison of the GPU greedy test fair: over the 24 greedy steps of each prompt the reference emits at least 8 distinct
    tokens, never the EOS id, and every step's top-2 logit margin is at least 10 x the GPU logit bound."""
    cfg, sd, adapter, audio = qr.greedy_fixture()
    for prompt in qr.GREEDY_PROMPTS:
        tokens, logits = qr.greedy(sd, cfg, adapter, audio, prompt, qr.GREEDY_STEPS)
        top = logits.topk(2, dim=-1).values
        margin, bound = float((top[:, 0] - top[:, 1]).min()), GPU_LOGIT_TOL * max(1.0, float(logits.abs().max()))
        print(f"prompt {prompt}: {len(set(tokens))} distinct tokens, smallest top-2 margin {margin:.4f}, GPU logit bound {bound:.5f} "
              f"(max |logit| {float(logits.abs().max()):.2f}), tokens {tokens}")
        assert len(tokens) == qr.GREEDY_STEPS and qr.GREEDY_EOS not in tokens
        assert len(set(tokens)) >= 8
        assert margin >= 10 * bound


def test_rounded_attention_model_is_causal_and_grouped():
    """The rounded restatement stays within bf16x3's reach of the exact one and follows the head grouping (a wrong KV head is an O(1) error)."""
    q, k, v = qr.variates("host.q", (1, 4, 5, 128), 1, 1.7), qr.variates("host.k", (1, 2, 70, 128), 1, 1.7), qr.variates("host.v", (1, 2, 70, 128), 1)
    ex = qr.causal_attention(q, k, v)
    for terms, tol in ((3, 1e-4), (1, 5e-2)):
        assert float((qr.rounded_causal_attention(q, k, v, terms) - ex).abs().max()) < tol


def _tiny(tied=True):
    return m2m.Qwen3Config(vocab_size=64, hidden_size=128, intermediate_size=64, num_hidden_layers=1, num_attention_heads=2, num_key_value_heads=1,
                           rms_norm_eps=1e-6, rope_theta=1e6, tie_word_embeddings=tied, max_position_embeddings=32)


def test_config_has_no_silent_defaults():
    with pytest.raises(TypeError):
        m2m.Qwen3Config()                                                  # nothing but head_dim is assumed
    c = m2m.Qwen3Config.qwen3_0_6b()
    assert (c.vocab_size, c.hidden_size, c.intermediate_size, c.num_hidden_layers, c.num_attention_heads, c.num_key_value_heads, c.head_dim) == \
        (151936, 1024, 3072, 28, 16, 8, 128)
    assert c.tie_word_embeddings and c.rms_norm_eps == 1e-6 and c.rope_theta == 1e6


def test_refusals_need_no_gpu():
    import dataclasses
    with pytest.raises(ValueError, match="head_dim"):
        m2m.Qwen3Decoder(dataclasses.replace(_tiny(), head_dim=64))
    with pytest.raises(ValueError, match="multiple of num_key_value_heads"):
        m2m.Qwen3Decoder(dataclasses.replace(_tiny(), num_attention_heads=3, num_key_value_heads=2))
    with pytest.raises(ValueError, match="precision"):
        m2m.Qwen3Decoder(_tiny(), precision="f16f8")
    dec = m2m.Qwen3Decoder(_tiny())
    x = torch.zeros(1, 4, 128)
    with pytest.raises(ValueError, match="inputs_embeds"):
        dec(torch.zeros(1, 4, 64))
    with pytest.raises(NotImplementedError, match="inference only"):
        dec(x.clone().requires_grad_(True))
    dec.model.norm.weight.requires_grad_(True)
    with pytest.raises(NotImplementedError, match="inference only"):
        dec(x)
    dec.model.norm.weight.requires_grad_(False)
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="no CPU fallback"):         # a missing GPU is an error, not an eager-torch run
            dec(x)
    with pytest.raises(ValueError, match="max_length"):
        m2m.Qwen3Cache(_tiny(), 1, 33, "cpu")


def test_attention_mask_must_be_right_padding():
    dec = m2m.Qwen3Decoder(_tiny())
    x = torch.zeros(2, 4, 128)
    for bad in ([[1, 1, 1, 1], [0, 1, 1, 1]], [[1, 0, 1, 1], [1, 1, 1, 1]], [[1, 1, 2, 1], [1, 1, 1, 1]]):
        with pytest.raises(ValueError, match="right padding"):
            dec._check_mask(torch.tensor(bad), 2, 4)
    with pytest.raises(ValueError, match="right padding"):
        dec._check_mask(torch.ones(2, 5, dtype=torch.long), 2, 4)
    dec._check_mask(torch.tensor([[1, 1, 1, 1], [1, 1, 0, 0]]), 2, 4)
    dec._check_mask(None, 2, 4)
    del x


@pytest.mark.parametrize("tied", [True, False])
def test_hf_named_state_dict_loads_strictly(tied):
    cfg = _tiny(tied)
    dec = m2m.Qwen3Decoder(cfg)
    sd = qr.state_dict(cfg, seed=1)
    assert set(dec.state_dict().keys()) == set(qr.parameter_shapes(cfg).keys())
    assert ("lm_head.weight" in sd) == (not tied)
    dec.load_state_dict({k: v.bfloat16() for k, v in sd.items()}, strict=True)          # a bf16 checkpoint is upcast on load
    for name, p in dec.state_dict().items():
        assert p.dtype == torch.float32 and torch.equal(p, sd[name].bfloat16().float()), name
    if tied:                                                              # HF's own state_dict() names the tied head as well: accepted, not a new tensor
        dec.load_state_dict({**sd, "lm_head.weight": sd["model.embed_tokens.weight"]}, strict=True)
    with pytest.raises(RuntimeError):
        dec.load_state_dict({k: v for k, v in sd.items() if k != "model.norm.weight"}, strict=True)
    assert dec.get_input_embeddings() is dec.model.embed_tokens
    emb = dec.resize_token_embeddings(80)
    assert emb.weight.shape == (80, 128) and dec.config.vocab_size == 80
    assert torch.equal(emb.weight[:64], sd["model.embed_tokens.weight"].float())
    if not tied:
        assert dec.lm_head.weight.shape == (80, 128) and torch.equal(dec.lm_head.weight[:64], sd["lm_head.weight"].float())


def test_model_refuses_a_graph_and_a_missing_tokenizer():
    dec = m2m.Qwen3Decoder(_tiny())
    adapter = m2m.CrossAttentionAdapter(64, 128, num_heads=1)
    model = m2m.MusicTranscriptionModel(lambda w, sr: torch.zeros(1, 3, 64), adapter, dec)
    with pytest.raises(NotImplementedError, match="inference only"):
        model(None, 16000, torch.zeros(1, 4, dtype=torch.long))
    with pytest.raises(ValueError, match="tokenizer"):
        model.generate(None, 16000)
    with pytest.raises(ValueError, match="text_dim"):
        m2m.MusicTranscriptionModel(None, m2m.CrossAttentionAdapter(64, 256, num_heads=2), dec)


def test_causal_attention_workspace_query_needs_no_gpu():
    from mlx8_ws_audio_transformer_amd import ops
    assert ops.causal_attention_workspace_bytes(2, 16, 130, 130) == 0      # the forward keeps nothing outside registers and LDS
    assert ops.causal_attention_workspace_bytes(0, 16, 1, 1) == 0
