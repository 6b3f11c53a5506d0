"""Host side of music2midi.CrossAttentionAdapter and of the cross-attention operator's C ABI, no GPU: the module's state_dict against the torch.nn
restatement (tests/music2midi_reference.py), the constructor's refusals, the workspace queries, and the refusal to compute without a GPU."""
import pytest
import torch

from mlx8_ws_audio_transformer_amd import _lib
from tests.music2midi_reference import ReferenceAdapter, nontrivial_

NAMES = ["audio_projection.weight", "audio_projection.bias", "cross_attention.in_proj_weight", "cross_attention.in_proj_bias",
         "cross_attention.out_proj.weight", "cross_attention.out_proj.bias", "layer_norm1.weight", "layer_norm1.bias", "layer_norm2.weight",
         "layer_norm2.bias", "feedforward.0.weight", "feedforward.0.bias", "feedforward.2.weight", "feedforward.2.bias"]


@pytest.mark.parametrize("audio_dim,text_dim,heads", [(512, 1024, 8), (128, 256, 2), (64, 1280, 10)])
def test_state_dict_is_that_of_the_torch_nn_restatement(audio_dim, text_dim, heads):
    import mlx8_ws_audio_transformer_amd as pkg
    from mlx8_ws_audio_transformer_amd import music2midi
    assert pkg.CrossAttentionAdapter is music2midi.CrossAttentionAdapter
    nat = music2midi.CrossAttentionAdapter(audio_dim, text_dim, heads)                      # the constructor needs no GPU
    ref = nontrivial_(ReferenceAdapter(audio_dim, text_dim, heads, dtype=torch.float32), seed=1)
    a, b = nat.state_dict(), ref.state_dict()
    assert sorted(a) == sorted(NAMES) and sorted(b) == sorted(NAMES)
    for k in NAMES:
        assert a[k].shape == b[k].shape and a[k].dtype == b[k].dtype, k
    assert tuple(a["cross_attention.in_proj_weight"].shape) == (3 * text_dim, text_dim) and tuple(a["feedforward.0.weight"].shape) == (4 * text_dim, text_dim)
    # a reference checkpoint's entries load once the prefix is stripped
    ckpt = {"cross_attention_adapter." + k: v for k, v in b.items()}
    stripped = {k[len("cross_attention_adapter."):]: v for k, v in ckpt.items()}
    assert not any(nat.load_state_dict(stripped, strict=True))
    assert all(torch.equal(nat.state_dict()[k], b[k]) for k in NAMES)
    assert nat.precision == "bf16x3" and all(p.requires_grad for p in nat.parameters()) and len(list(nat.parameters())) == 14
    assert music2midi.CrossAttentionAdapter(audio_dim, text_dim, heads, dtype=torch.bfloat16).feedforward[2].bias.dtype == torch.bfloat16


def test_constructor_refusals():
    from mlx8_ws_audio_transformer_amd import CrossAttentionAdapter
    with pytest.raises(ValueError, match="128"):
        CrossAttentionAdapter(512, 1024, 16)               # head_dim 64
    with pytest.raises(ValueError, match="128"):
        CrossAttentionAdapter(512, 768, 8)                 # head_dim 96
    with pytest.raises(ValueError, match="1280"):
        CrossAttentionAdapter(512, 1536, 12)               # head_dim 128, beyond the LayerNorm kernels
    with pytest.raises(ValueError, match="multiple of 64"):
        CrossAttentionAdapter(80, 1024, 8)
    with pytest.raises(ValueError, match="precision"):
        CrossAttentionAdapter(512, 1024, 8, precision="f16f8")


def test_workspace_queries_answer_without_a_gpu_and_are_monotone():
    from mlx8_ws_audio_transformer_amd import ops
    q = ops.cross_attention_workspace_bytes
    assert q(4, 8, 512, 1500, backward=True) >= 4 * 8 * 512 * 4          # delta [B, H, Lq]
    assert q(4, 8, 512, 1500, backward=True) % 256 == 0
    assert q(0, 8, 512, 1500, backward=True) == 0
    for backward in (False, True):
        sizes = [q(2, 8, Lq, 1500, backward) for Lq in (1, 2, 63, 64, 65, 512, 513, 4096)]
        assert sizes == sorted(sizes)
        sizes = [q(2, 8, 512, Sk, backward) for Sk in (1, 63, 64, 65, 1500, 3000)]
        assert sizes == sorted(sizes)
        assert q(2, 8, 512, 1500, True) >= q(2, 8, 512, 1500, backward)


def test_argument_checks_return_before_touching_a_gpu():
    """The entry points validate before they launch: with a dummy context pointer and dummy tensor addresses every refusal below is AWT_ERR_INVALID."""
    L = _lib.lib()
    ctx, p = 0x1000, 0x10000                                               # never dereferenced: each call fails its checks first
    fwd = lambda **kw: L.awt_op_cross_attention(kw.get("ctx", ctx), kw.get("q", p), kw.get("ldq", 256), p, kw.get("ldk", 256), p, 256, p, 256, None, 1, 2, 8, 16,
                                                kw.get("terms", 3), None, 0, None)
    for kw, text in ((dict(ldq=128), "H * 128"), (dict(ldk=258), "multiples of 4"), (dict(terms=2), "terms"), (dict(q=None), "null"), (dict(ctx=None), "null")):
        assert fwd(**kw) == -1, kw
        assert text in L.awt_last_error().decode(), (kw, L.awt_last_error())
    bwd = lambda terms, ws, n: L.awt_op_cross_attention_backward(ctx, p, 256, p, 256, p, 256, p, p, 256, p, p, p, p, 1, 2, 8, 16, terms, ws, n, None)
    need = L.awt_op_cross_attention_workspace_bytes(1, 2, 8, 16, 1)
    assert bwd(3, 0x20000, need - 1) == -1 and "workspace too small" in L.awt_last_error().decode()
    assert bwd(3, None, need) == -1 and "null" in L.awt_last_error().decode()
    assert bwd(0, 0x20000, need) == -1 and "terms" in L.awt_last_error().decode()


def test_forward_raises_without_a_gpu():
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from mlx8_ws_audio_transformer_amd import CrossAttentionAdapter
    m = CrossAttentionAdapter(128, 256, 2)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m(torch.zeros(1, 3, 256), torch.zeros(1, 5, 128))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.encode_audio(torch.zeros(1, 5, 128))
