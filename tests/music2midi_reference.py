"""The cross-attention adapter of the music-transcription model as a float64 module of stock torch.nn layers: what
mlx8_ws_audio_transformer_amd.music2midi.CrossAttentionAdapter must compute, and the names its state_dict must carry.

    a   = audio_projection(audio)                         Linear(audio_dim -> text_dim)
    t1  = layer_norm1(text + MHA(query = text, key = a, value = a))     nn.MultiheadAttention(batch_first=True), no mask, weights discarded
    out = layer_norm2(t1 + feedforward(t1))               Linear(text_dim -> 4 text_dim), exact erf GELU, Linear(4 text_dim -> text_dim)

`nontrivial_(module, seed)` overwrites every parameter with values from `weights.unit_variates` (as tests/test_gpu_classifier.py `_pair` does): LayerNorm
gains around 1, biases and LayerNorm shifts of magnitude 0.1, matrices at K^-1/2 times 1.5, so the attention logits spread over a few units."""
import numpy as np
import torch
import torch.nn as nn

from mlx8_ws_audio_transformer_amd import weights as wts


class ReferenceAdapter(nn.Module):
    def __init__(self, audio_dim, text_dim, num_heads=8, dtype=torch.float64):
        super().__init__()
        self.audio_projection = nn.Linear(audio_dim, text_dim, dtype=dtype)
        self.cross_attention = nn.MultiheadAttention(text_dim, num_heads, batch_first=True, dtype=dtype)
        self.layer_norm1 = nn.LayerNorm(text_dim, dtype=dtype)
        self.layer_norm2 = nn.LayerNorm(text_dim, dtype=dtype)
        self.feedforward = nn.Sequential(nn.Linear(text_dim, 4 * text_dim, dtype=dtype), nn.GELU(), nn.Linear(4 * text_dim, text_dim, dtype=dtype))

    def forward(self, text, audio):
        a = self.audio_projection(audio)
        t1 = self.layer_norm1(text + self.cross_attention(text, a, a, need_weights=False)[0])
        return self.layer_norm2(t1 + self.feedforward(t1))


def nontrivial_(module, seed):
    with torch.no_grad():
        for name, p in module.named_parameters():
            u = torch.from_numpy(wts.unit_variates("m2m." + name, p.numel(), seed).reshape(p.shape)).to(p.dtype)
            if "layer_norm" in name:
                p.copy_(1.0 + 0.1 * u if name.endswith("weight") else 0.1 * u)
            elif p.dim() > 1:
                p.copy_(1.5 * p.shape[1] ** -0.5 * u)
            else:
                p.copy_(0.1 * u)
    return module


def variates(name, shape, seed, scale=1.0):
    return torch.from_numpy(wts.unit_variates(name, int(np.prod(shape)), seed).reshape(shape)) * scale
