"""GPU: the decoder's parameter gradients (`NativeWhisperDecoder(train_base=True)`, `WhisperLoRAModel(train_decoder=True)`)
against torch autograd on the stock-PyTorch decoder (`native_decoder=False, native_cross_kv=False`, itself pinned to
`WhisperForConditionalGeneration` by tests/golden/decoder.npz).  Tolerances are the project's (test_gpu_native_decoder.py):
every gradient within 2e-3 of its largest element, loss within 2e-4 relative, logits within 2e-3."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from mlx8_ws_audio_transformer_amd import weights as wts
from oracle import logmel as oracle_mel
from tests.util import golden, piano_clips_f32

pytestmark = pytest.mark.gpu

ENC_FROZEN = "embed_positions.weight"


def _klass(name):
    return name.split(".", 2)[2] if name.startswith("layers.") else name


def _labels(variant):
    lab = torch.from_numpy(golden("decoder.npz")["labels"]).clone()
    if variant == "padded":          # -100 in both rows (the ignore path) and a token repeated within a row (the duplicate-id path of the embedding backward)
        lab[0, 5:] = -100
        lab[1, 3] = lab[1, 2]
        lab[0, 2] = lab[0, 1]
    return lab.cuda()


@functools.lru_cache(maxsize=None)
def _mel():
    cfg = wts.config("mini", True)
    return torch.from_numpy(oracle_mel.whisper_logmel(piano_clips_f32(2), n_samples=2 * cfg.max_source_positions * 160))


def _model(native, enc_mode, **kw):
    """`_pair` of test_gpu_native_decoder.py (mini encoder, 2 decoder layers, vocab 512, 64 positions, the weights of decoder.npz) with a trained decoder."""
    from mlx8_ws_audio_transformer_amd.finetune import WhisperLoRAModel
    cfg = wts.config("mini", True)
    lora = wts.LoraSpec(r=8, alpha=16.0) if enc_mode == "lora" else None
    m = WhisperLoRAModel(cfg, lora, train_encoder=enc_mode == "full", train_decoder=True, decoder_layers=2, vocab=512, max_target_positions=64,
                         native_decoder=native, native_cross_kv=native, **kw)
    m.config.decoder_start_token_id, m.config.pad_token_id, m.config.eos_token_id = 1, 0, 2
    We = wts.init_encoder_weights(cfg, seed=0, profile="test")
    Wd = wts.init_decoder_weights(cfg.d_model, 2, cfg.ffn, 512, 64, seed=0)
    m.encoder.load_state_dict({k: torch.from_numpy(v) for k, v in We.items()}, strict=False)
    m.decoder.load_state_dict({k: torch.from_numpy(v) for k, v in Wd.items()}, strict=True)
    with torch.no_grad():
        for n, p in m.encoder.named_parameters():
            if "lora_B" in n:            # non-zero B so that every adapter matrix gets a gradient
                p.copy_(torch.from_numpy(0.05 * wts.unit_variates("ndec", p.numel(), 1).reshape(p.shape).astype(np.float32)))
    return m


def _step(m, labels):
    m.zero_grad(set_to_none=True)
    out = m(input_features=_mel().cuda(), labels=labels)
    out.loss.backward()
    enc = {n: p.grad.detach().clone() for n, p in m.encoder.named_parameters() if p.requires_grad}
    dec = {n: p.grad.detach().clone() for n, p in m.decoder.named_parameters()}
    return float(out.loss.detach()), out.logits.detach().float().clone(), enc, dec


@functools.lru_cache(maxsize=None)
def _reference(enc_mode, variant):
    """torch autograd over the stock decoder, once per (encoder mode, labels) and shared by the cross modes."""
    return _step(_model(False, enc_mode), _labels(variant))


def _compare(got, ref, bound, what):
    worst = {}
    for n, g_ref in ref.items():
        g = got[n]
        assert g is not None and g.shape == g_ref.shape and bool(torch.isfinite(g).all()), n
        assert float(g.abs().max()) > 0 and float(g_ref.abs().max()) > 0, n
        worst[_klass(n)] = max(worst.get(_klass(n), 0.0), float((g - g_ref).abs().max() / g_ref.abs().max()))
    assert set(got) == set(ref)
    for k in sorted(worst):
        print(f"worst relative gradient error  {what:8s} {k:36s} {worst[k]:.3e}")
    bad = {k: v for k, v in worst.items() if not v < bound}
    assert not bad, bad


@pytest.mark.parametrize("enc_mode", ["lora", "full"])
@pytest.mark.parametrize("cross_mode", ["kv", "absorbed"])
def test_every_decoder_gradient_matches_torch_autograd(cross_mode, enc_mode):
    m = _model(True, enc_mode)
    m.decoder.cross_mode = cross_mode
    assert all(p.requires_grad for p in m.decoder.parameters()) and m.decoder.train_base
    assert [n for n, p in m.encoder.named_parameters() if p.requires_grad and n == ENC_FROZEN] == []
    for variant in ("golden", "padded"):
        labels = _labels(variant)
        assert m.decoder.absorbed_cross(labels.shape[1], m.encoder.cfg.max_source_positions) == (cross_mode == "absorbed")
        loss, logits, enc, dec = _step(m, labels)
        r_loss, r_logits, r_enc, r_dec = _reference(enc_mode, variant)
        print(variant, "loss", loss, "reference", r_loss, "logits max-abs", float((logits - r_logits).abs().max()))
        assert abs(loss - r_loss) < 2e-4 * abs(r_loss)
        assert float((logits - r_logits).abs().max()) < 2e-3
        _compare(dec, r_dec, 2e-3, "decoder")
        _compare(enc, r_enc, 2e-3, "encoder")


# ---------------------------------------------------------------------------------------------------- the decoder alone
def _decoders(d, layers, heads, ffn, vocab, maxpos, precision="bf16x3", train_base=True):
    from mlx8_ws_audio_transformer_amd.finetune import WhisperDecoder
    from mlx8_ws_audio_transformer_amd.native_decoder import NativeWhisperDecoder
    torch.manual_seed(0)
    ref = WhisperDecoder(d, layers, heads, ffn, vocab, maxpos)
    with torch.no_grad():                                   # embeddings of Whisper's scale: logits of order one
        ref.embed_tokens.weight.mul_(0.05)
        ref.embed_positions.weight.mul_(0.05)
    nat = NativeWhisperDecoder(d, layers, heads, ffn, vocab, maxpos, precision=precision, train_base=train_base)
    nat.load_state_dict(ref.state_dict())
    return nat.cuda(), ref.cuda()


def _alone_inputs(B, S, d, L, vocab, seed=0):
    from mlx8_ws_audio_transformer_amd.finetune import shift_tokens_right
    g = torch.Generator().manual_seed(seed)
    enc = torch.randn((B, S, d), generator=g).cuda()
    labels = torch.randint(0, vocab, (B, L), generator=g)
    labels[0, 0], labels[1, 0], labels[0, 1] = vocab - 1, 0, vocab - 1          # both ends of the table; the last row of a ragged vocabulary
    labels[1, 2] = labels[1, 1]                                                 # a token repeated within a row
    labels[1, L - 3:] = -100                                                    # padding: ignored rows, and the pad id repeated in the decoder input
    ids = shift_tokens_right(labels, vocab - 2, vocab - 3)
    return enc, ids.cuda(), labels.cuda()


def _native_alone(nat, enc, ids, labels):
    nat.zero_grad(set_to_none=True)
    e = enc.clone().requires_grad_(True)
    loss, logits = nat.loss(ids, labels, e)
    loss.backward()
    grads = {n: (None if p.grad is None else p.grad.detach().clone()) for n, p in nat.named_parameters()}
    return float(loss.detach()), logits.detach().clone(), e.grad.detach().clone(), grads


def _torch_alone(ref, enc, ids, labels):
    ref.zero_grad(set_to_none=True)
    e = enc.clone().requires_grad_(True)
    logits = ref(ids, e)
    loss = F.cross_entropy(logits.view(-1, logits.shape[-1]), labels.reshape(-1), ignore_index=-100)
    loss.backward()
    return float(loss.detach()), logits.detach(), e.grad.detach(), {n: p.grad.detach() for n, p in ref.named_parameters()}


@pytest.mark.parametrize("cross_mode", ["kv", "absorbed"])
def test_decoder_alone_at_whisper_small_width(cross_mode):
    """d = 768, 12 heads, ffn 3072, the ragged vocabulary 51865 (-> 51968 padded columns), 448 positions: one layer, L = 12, S = 200."""
    nat, ref = _decoders(768, 1, 12, 3072, 51865, 448)
    nat.cross_mode = cross_mode
    enc, ids, labels = _alone_inputs(2, 200, 768, 12, 51865)
    loss, logits, d_enc, grads = _native_alone(nat, enc, ids, labels)
    r_loss, r_logits, r_enc, r_grads = _torch_alone(ref, enc, ids, labels)
    print("loss", loss, "reference", r_loss, "logits max-abs", float((logits - r_logits).abs().max()))
    assert abs(loss - r_loss) < 2e-4 * abs(r_loss)
    assert float((logits - r_logits).abs().max()) < 2e-3
    _compare(dict(grads, encoder_states=d_enc), dict(r_grads, encoder_states=r_enc), 2e-3, "alone")
    assert float(grads["embed_positions.weight"][12:].abs().max()) == 0.0            # position rows beyond L get no gradient


MINI = (128, 2, 2, 512, 512, 64)


@pytest.mark.parametrize("cross_mode", ["kv", "absorbed"])
def test_two_backward_passes_give_identical_gradients(cross_mode):
    nat, _ = _decoders(*MINI)
    nat.cross_mode = cross_mode
    enc, ids, labels = _alone_inputs(2, 100, 128, 7, 512)
    a, b = _native_alone(nat, enc, ids, labels), _native_alone(nat, enc, ids, labels)
    assert a[0] == b[0] and torch.equal(a[2], b[2])
    for n in a[3]:
        assert torch.equal(a[3][n], b[3][n]), n


@pytest.mark.parametrize("cross_mode", ["kv", "absorbed"])
def test_one_product_precision_stays_in_its_band(cross_mode):
    """precision="bf16" (one bf16 product per fragment pair, forward and weight gradients): the band DESIGN §4.5b records for the encoder's
    one-product mode, 2e-2 of each gradient's largest element -- a sanity bound, not tuned to this code."""
    nat, ref = _decoders(*MINI, precision="bf16")
    nat.cross_mode = cross_mode
    enc, ids, labels = _alone_inputs(2, 100, 128, 7, 512)
    _, _, d_enc, grads = _native_alone(nat, enc, ids, labels)
    _, _, r_enc, r_grads = _torch_alone(ref, enc, ids, labels)
    _compare(dict(grads, encoder_states=d_enc), dict(r_grads, encoder_states=r_enc), 2e-2, "bf16")


@pytest.mark.parametrize("cross_mode", ["kv", "absorbed"])
def test_frozen_decoder_is_unchanged_by_the_new_mode(cross_mode):
    """train_base=False: no base gradient, and d(encoder states) / loss / logits are bit for bit those of the path that also forms the
    parameter gradients (the parameter gradients are side products: they do not enter the chain to the encoder).  This shows that the two
    modes of this code agree, not that the frozen mode equals the code before the mode existed: that is what the unchanged
    tests/test_gpu_native_decoder.py and tests/test_gpu_full_finetune.py check."""
    frozen, _ = _decoders(*MINI, train_base=False)
    trained, _ = _decoders(*MINI, train_base=True)
    frozen.cross_mode = trained.cross_mode = cross_mode
    assert not any(p.requires_grad for p in frozen.parameters())
    enc, ids, labels = _alone_inputs(2, 100, 128, 7, 512)
    f, t = _native_alone(frozen, enc, ids, labels), _native_alone(trained, enc, ids, labels)
    assert all(g is None for g in f[3].values()) and all(g is not None for g in t[3].values())
    assert f[0] == t[0] and torch.equal(f[1], t[1]) and torch.equal(f[2], t[2])
    # a frozen encoder under the trained decoder: the gradient to the encoder states is skipped, the parameter gradients are the same bits
    trained.zero_grad(set_to_none=True)
    loss, _ = trained.loss(ids, labels, enc)
    loss.backward()
    for n, p in trained.named_parameters():
        assert torch.equal(p.grad, t[3][n]), n


def test_train_base_rejects_adapters():
    from mlx8_ws_audio_transformer_amd.native_decoder import NativeWhisperDecoder
    with pytest.raises(ValueError, match="train_base=True"):
        NativeWhisperDecoder(128, 1, 2, 512, 512, 64, lora=wts.LoraSpec(r=8, alpha=16.0), train_base=True)
