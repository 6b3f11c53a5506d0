"""`CrossAttentionAdapter` (the reference's .charles/music2midi/model.py:125-188), the consumer of `WhisperAudioEncoder`, on libawt.

The reference's music-transcription model is three pieces: the Whisper audio tower (`audio_encoder.WhisperAudioEncoder` here), a stock Qwen
decoder, and between them this adapter -- the one fully trainable module the reference defines itself.  Text embeddings attend to the projected
encoder states:

    a    = audio_projection(audio_features)                                            [B, Sa, text_dim]
    attn = MultiheadAttention(query = text, key = value = a)   (nn.MultiheadAttention(batch_first=True): packed in-projection, q scaled by
                                                                head_dim^-1/2, no mask, no dropout; the attention weights are not returned)
    x    = layer_norm1(text + attn)
    out  = layer_norm2(x + W2 gelu(W1 x))                       (exact erf GELU)

Same constructor and parameter names as the reference (`audio_projection`, `cross_attention.in_proj_weight / in_proj_bias / out_proj`,
`layer_norm1`, `layer_norm2`, `feedforward.0`, `feedforward.2`: 14 tensors), so the `cross_attention_adapter.*` entries of a reference
`trainable_state_dict` load with `load_state_dict(strict=True)` once the prefix is stripped.

Every operator is a `torch.autograd.Function` whose forward AND backward are libawt calls (`AlignedLinear`, `LayerNorm` and `Gelu` of
autograd_ops.py, shared with the classifiers; `_CrossAttention` here):
  * linears: y = x W^T + b and dx = dy W on the MFMA GEMM (`awt_op_linear`), dW = dy^T x on the weight-gradient GEMM (`awt_op_weight_grad`),
    db by pitched column sums (`awt_op_column_sums_ld`; fc1 has 4 text_dim columns);
  * keys and values are ONE GEMM of N = 2 text_dim against rows text_dim .. 3 text_dim of `in_proj_weight`; the attention reads that
    [B Sa, 2 text_dim] buffer in place (ldk = ldv = 2 text_dim) and writes its gradient into a buffer of the same layout;
  * attention: `awt_op_cross_attention` / `_backward` (csrc/cross_attention.hip: head_dim 128, flash-style on the bf16 MFMAs, P recomputed from
    the saved log-sum-exp in the backward);
  * LayerNorm: `awt_op_layernorm`, `awt_op_layernorm_backward` (dx), `awt_op_layernorm_param_grad`; GELU: `awt_op_gelu` / `awt_op_gelu_backward`.
The two residual adds, the dtype casts and the row slices of `in_proj_weight` are element-wise / view ops of torch under autograd.  There is no
torch fallback for any operator above: without libawt or without a GPU the first call raises.

`encode_audio(audio_features)` returns the projected key / value buffer `audio_kv` [B, Sa, 2 text_dim]; `forward(text, audio_kv=audio_kv)` reuses it.
The reference's `generate` recomputes the projection for every new token (model.py:314-341); a caller of this module computes it once per clip.
"""
from __future__ import annotations

from typing import Optional

import torch
import torch.nn as nn

from . import _lib, ops
from .autograd_ops import AlignedLinear, Gelu, LayerNorm

HEAD_DIM = 128            # csrc/cross_attention.hip
MAX_TEXT_DIM = 1280       # the LayerNorm kernels' row limit


class _CrossAttention(torch.autograd.Function):
    """q [B * L, H * 128], kv [B * Sa, 2 * H * 128] (keys | values per row) -> o [B * L, H * 128]; the score scale 128^-1/2 is applied in the kernel."""

    @staticmethod
    def forward(ctx, q, kv, B, H, L, Sa, precision):
        d = H * HEAD_DIM
        o, lse = ops.cross_attention((q, 0), d, (kv, 0), 2 * d, (kv, d), 2 * d, B, H, L, Sa, precision, want_lse=True)
        ctx.save_for_backward(q, kv, o, lse)
        ctx.shape, ctx.precision = (B, H, L, Sa), precision
        return o

    @staticmethod
    def backward(ctx, do):
        q, kv, o, lse = ctx.saved_tensors
        B, H, L, Sa = ctx.shape
        d = H * HEAD_DIM
        dq, dkv = torch.empty_like(q), torch.empty_like(kv)            # every element of both is written
        ops.cross_attention_backward((q, 0), d, (kv, 0), 2 * d, (kv, d), 2 * d, (o, 0), (do.contiguous(), 0), d, lse, (dq, 0), (dkv, 0), (dkv, d),
                                     B, H, L, Sa, ctx.precision)
        return dq, dkv, None, None, None, None, None


class CrossAttentionAdapter(nn.Module):
    def __init__(self, audio_dim: int, text_dim: int, num_heads: int = 8, dtype=None, precision: str = "bf16x3"):
        super().__init__()
        if num_heads <= 0 or text_dim % num_heads or text_dim // num_heads != HEAD_DIM:
            raise ValueError(f"text_dim // num_heads must be {HEAD_DIM}, the native cross-attention kernel's head_dim (got {text_dim} / {num_heads})")
        if text_dim > MAX_TEXT_DIM:
            raise ValueError(f"text_dim must be <= {MAX_TEXT_DIM} (the native LayerNorm kernels' row limit), got {text_dim}")
        if audio_dim <= 0 or audio_dim % 64:
            raise ValueError(f"audio_dim must be a multiple of 64 (the MFMA GEMM's K step), got {audio_dim}")
        if precision not in ("bf16", "bf16x3"):
            raise ValueError("precision must be 'bf16x3' or 'bf16' (training needs fp32's exponent range in the operand planes)")
        self.audio_dim, self.text_dim, self.num_heads, self.precision = audio_dim, text_dim, num_heads, precision
        self.dtype = dtype or torch.float32
        self.audio_projection = nn.Linear(audio_dim, text_dim, dtype=self.dtype)
        # holds the parameters under the reference's names (in_proj_weight, in_proj_bias, out_proj.*); its own forward is never called
        self.cross_attention = nn.MultiheadAttention(embed_dim=text_dim, num_heads=num_heads, batch_first=True, dtype=self.dtype)
        self.layer_norm1 = nn.LayerNorm(text_dim, dtype=self.dtype)
        self.layer_norm2 = nn.LayerNorm(text_dim, dtype=self.dtype)
        self.feedforward = nn.Sequential(nn.Linear(text_dim, text_dim * 4, dtype=self.dtype), nn.GELU(), nn.Linear(text_dim * 4, text_dim, dtype=self.dtype))

    def _linear(self, x: torch.Tensor, w: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
        return AlignedLinear.apply(x, w.float(), b.float(), self.precision)

    def _layer_norm(self, ln: nn.LayerNorm, x: torch.Tensor) -> torch.Tensor:
        return LayerNorm.apply(x.contiguous(), ln.weight.float(), ln.bias.float(), ln.eps)

    def encode_audio(self, audio_features: torch.Tensor) -> torch.Tensor:
        """audio_features [B, Sa, audio_dim] -> audio_kv [B, Sa, 2 text_dim] fp32: the keys (first text_dim columns) and values of every head, what
        `forward` attends to.  Compute it once per clip and pass it as `forward(text, audio_kv=...)` for every decoding step."""
        if audio_features.dim() != 3 or audio_features.shape[-1] != self.audio_dim:
            raise ValueError(f"audio_features must be [B, Sa, {self.audio_dim}], got {tuple(audio_features.shape)}")
        _lib.ctx(audio_features.device)                                    # raises without a GPU: no CPU fallback
        B, Sa, _ = audio_features.shape
        d, att = self.text_dim, self.cross_attention
        a = self._linear(audio_features.float().reshape(B * Sa, -1).contiguous(), self.audio_projection.weight, self.audio_projection.bias)
        kv = self._linear(a, att.in_proj_weight[d:], att.in_proj_bias[d:])   # K and V as one GEMM of N = 2 text_dim
        return kv.reshape(B, Sa, 2 * d)

    def forward(self, text_embeddings: torch.Tensor, audio_features: Optional[torch.Tensor] = None, audio_kv: Optional[torch.Tensor] = None) -> torch.Tensor:
        """text_embeddings [B, L, text_dim], audio_features [B, Sa, audio_dim] (or audio_kv from `encode_audio`) -> [B, L, text_dim] in
        text_embeddings' dtype (model.py:157-188).  The arithmetic runs in fp32 whatever the dtype of the inputs and the parameters."""
        if (audio_features is None) == (audio_kv is None):
            raise ValueError("pass exactly one of audio_features and audio_kv")
        if text_embeddings.dim() != 3 or text_embeddings.shape[-1] != self.text_dim:
            raise ValueError(f"text_embeddings must be [B, L, {self.text_dim}], got {tuple(text_embeddings.shape)}")
        _lib.ctx(text_embeddings.device)                                   # raises without a GPU: no CPU fallback
        if audio_kv is None:
            audio_kv = self.encode_audio(audio_features)
        B, L, d = text_embeddings.shape
        if audio_kv.dim() != 3 or audio_kv.shape[0] != B or audio_kv.shape[-1] != 2 * d:
            raise ValueError(f"audio_kv must be [{B}, Sa, {2 * d}], got {tuple(audio_kv.shape)}")
        Sa, att, ff = audio_kv.shape[1], self.cross_attention, self.feedforward
        text = text_embeddings.float().reshape(B * L, d).contiguous()
        q = self._linear(text, att.in_proj_weight[:d], att.in_proj_bias[:d])
        o = _CrossAttention.apply(q, audio_kv.float().reshape(B * Sa, 2 * d).contiguous(), B, self.num_heads, L, Sa, self.precision)
        x = self._layer_norm(self.layer_norm1, text + self._linear(o, att.out_proj.weight, att.out_proj.bias))
        h = Gelu.apply(self._linear(x, ff[0].weight, ff[0].bias))
        out = self._layer_norm(self.layer_norm2, x + self._linear(h, ff[2].weight, ff[2].bias))
        return out.reshape(B, L, d).to(text_embeddings.dtype)
