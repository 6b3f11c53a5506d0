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

`Qwen3Decoder` and `MusicTranscriptionModel` (further down; DESIGN.md sections 4.12 and 4.13) are the stock Qwen decoder and the model around all three pieces:
teacher-forced loss and logits, and `generate` with a KV cache, on awt_op_rmsnorm / awt_op_qk_norm_rope / awt_op_causal_attention / awt_op_silu_mul and the packed-weight
GEMMs (operands kept by native_decoder.PackedSet; a copy of the decoder packs its own).  Built with `trainable_layers=K` the decoder also trains, under the reference's rule
(the top K layers, the final norm, the output head), and passes the gradient of `inputs_embeds` down through every layer to the adapter: `_Qwen3Graph` is one autograd node
whose backward is libawt calls (awt_op_causal_attention_backward, awt_op_qk_norm_rope_backward, awt_op_rmsnorm_backward / _param_grad, awt_op_silu_mul_backward,
awt_linear_backward_input, awt_op_weight_grad, awt_op_embed_backward).

`encode_audio(audio_features)` returns the projected key / value buffer `audio_kv` [B, Sa, 2 text_dim]; `forward(text, audio_kv=audio_kv)` reuses it.
The reference's `generate` recomputes the projection for every new token (model.py:314-341); a caller of this module computes it once per clip.
"""
from __future__ import annotations

import dataclasses
from typing import Optional

import torch
import torch.nn as nn

from . import _lib, ops
from .autograd_ops import AlignedLinear, Gelu, LayerNorm
from .native_decoder import PackedLinear, PackedSet, cross_entropy, embed_backward

HEAD_DIM = 128            # csrc/cross_attention.hip
MAX_TEXT_DIM = 1280       # the LayerNorm kernels' row limit
DECODE_ROWS = 8           # awt_linear_decode's row limit (csrc/gemv.hip): `step` up to this batch, and the group size of `generate_batch`


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


# ====================================================================================================================== Qwen3 text decoder (inference)
@dataclasses.dataclass
class Qwen3Config:
    """The fields of a Qwen3 `config.json` that the decoder reads.  Only head_dim has a default: a checkpoint's other values come from its config, which
    this package cannot fetch, so they are never assumed -- `Qwen3Config.qwen3_0_6b()` names the published values of Qwen/Qwen3-0.6B-Base."""
    vocab_size: int
    hidden_size: int
    intermediate_size: int
    num_hidden_layers: int
    num_attention_heads: int
    num_key_value_heads: int
    rms_norm_eps: float
    rope_theta: float
    tie_word_embeddings: bool
    max_position_embeddings: int
    head_dim: int = HEAD_DIM

    @classmethod
    def qwen3_0_6b(cls) -> "Qwen3Config":
        return cls(vocab_size=151936, hidden_size=1024, intermediate_size=3072, num_hidden_layers=28, num_attention_heads=16, num_key_value_heads=8,
                   rms_norm_eps=1e-6, rope_theta=1e6, tie_word_embeddings=True, max_position_embeddings=40960)


class _Weight(nn.Module):
    """A parameter named `weight`: the RMSNorm gains and the bias-free projections under HF's state-dict names."""

    def __init__(self, *shape, ones: bool = False):
        super().__init__()
        self.weight = nn.Parameter(torch.ones(shape) if ones else torch.empty(shape), requires_grad=False)
        if not ones:
            nn.init.normal_(self.weight, std=0.02)                         # HF's initializer_range


class Qwen3Cache:
    """Keys and values of incremental decoding: per layer k and v [B, Tmax, Hkv * 128] (uninitialised: the kernels never read past `length`), the
    number of live positions, and the int32 position ramp the rotary kernel indexes."""

    def __init__(self, config: Qwen3Config, batch: int, max_length: int, device):
        if max_length < 1 or max_length > config.max_position_embeddings:
            raise ValueError(f"max_length must be in [1, {config.max_position_embeddings}] (max_position_embeddings), got {max_length}")
        w = config.num_key_value_heads * HEAD_DIM
        self.batch, self.max_length, self.length = batch, max_length, 0
        self.k = [torch.empty((batch, max_length, w), dtype=torch.float32, device=device) for _ in range(config.num_hidden_layers)]
        self.v = [torch.empty((batch, max_length, w), dtype=torch.float32, device=device) for _ in range(config.num_hidden_layers)]
        self.ramp = torch.arange(max_length, dtype=torch.int32, device=device)


class Qwen3Decoder(nn.Module):
    """`Qwen3ForCausalLM` driven by `inputs_embeds` (the reference's text decoder, .charles/music2midi/model.py:209-213), inference only, on libawt:

        per layer   h = RMSNorm(x); q | k | v = h Wqkv^T (ONE GEMM); per-head RMSNorm of q and k, rotary embedding, k and v into the cache (awt_op_qk_norm_rope);
                    causal attention over the cache with grouped KV heads (awt_op_causal_attention); x += o Wo^T (residual in the GEMM's epilogue);
                    h = RMSNorm(x); gate | up = h Wgu^T (ONE GEMM); x += (silu(gate) * up) Wdown^T (awt_op_silu_mul, residual in the epilogue)
        then        logits = RMSNorm(x) Wlm^T

    Parameters carry HF's names (`model.embed_tokens.weight`, `model.layers.N.self_attn.q_proj.weight`, ..., `model.norm.weight`, `lm_head.weight` when
    untied), fp32; a bf16 checkpoint is upcast by `load_state_dict`.  The packed GEMM operands are built on first use and again after `load_state_dict`,
    `resize_token_embeddings` or a move to another device.  There is no torch fallback: without libawt or a GPU it raises.

    trainable_layers=None (the default) is the inference-only decoder: every parameter frozen, everything under `torch.no_grad()`, and asked for an autograd
    graph it raises NotImplementedError.  trainable_layers=K, an int in [0, num_hidden_layers], is the reference's fine-tuning rule (.charles/music2midi/
    model.py:242-261): requires_grad on every parameter of the last K layers, on `model.norm.weight` and on the output head -- `lm_head.weight`, or with tied
    embeddings `model.embed_tokens.weight`, the one tensor HF holds under both names -- and nothing else.  `forward` then builds a graph when grad is enabled
    (`_Qwen3Graph`): gradients reach `inputs_embeds` through all layers and every trainable parameter; the packed operands carry their transpose planes and
    follow the parameters after an optimizer step (only what changed is packed again, `PackedLinear.update`).  `prefill` / `step` stay inference only."""

    def __init__(self, config: Qwen3Config, precision: str = "bf16x3", trainable_layers: Optional[int] = None):
        super().__init__()
        c = config
        if trainable_layers is not None and (isinstance(trainable_layers, bool) or not isinstance(trainable_layers, int)
                                             or not 0 <= trainable_layers <= c.num_hidden_layers):
            raise ValueError(f"trainable_layers must be None or an int in [0, {c.num_hidden_layers}] (num_hidden_layers), got {trainable_layers!r}")
        if c.head_dim != HEAD_DIM:
            raise ValueError(f"head_dim must be {HEAD_DIM}, the native kernels' head_dim (got {c.head_dim})")
        if precision not in ("bf16", "bf16x3"):
            raise ValueError("precision must be 'bf16x3' or 'bf16'")
        if c.num_attention_heads <= 0 or c.num_key_value_heads <= 0 or c.num_attention_heads % c.num_key_value_heads:
            raise ValueError("num_attention_heads must be a positive multiple of num_key_value_heads")
        if c.hidden_size <= 0 or c.hidden_size % 128 or c.intermediate_size <= 0 or c.intermediate_size % 64:
            raise ValueError("hidden_size must be a multiple of 128 and intermediate_size of 64 (the MFMA GEMM's N tile and K step)")
        self.config, self.precision, self.trainable_layers = c, precision, trainable_layers
        d, I, Hq, Hkv = c.hidden_size, c.intermediate_size, c.num_attention_heads, c.num_key_value_heads
        self.model = nn.Module()
        self.model.embed_tokens = nn.Embedding(c.vocab_size, d)
        nn.init.normal_(self.model.embed_tokens.weight, std=0.02)
        self.model.embed_tokens.weight.requires_grad_(False)
        layers = []
        for _ in range(c.num_hidden_layers):
            layer, att, mlp = nn.Module(), nn.Module(), nn.Module()
            att.q_proj, att.k_proj, att.v_proj, att.o_proj = _Weight(Hq * HEAD_DIM, d), _Weight(Hkv * HEAD_DIM, d), _Weight(Hkv * HEAD_DIM, d), _Weight(d, Hq * HEAD_DIM)
            att.q_norm, att.k_norm = _Weight(HEAD_DIM, ones=True), _Weight(HEAD_DIM, ones=True)
            mlp.gate_proj, mlp.up_proj, mlp.down_proj = _Weight(I, d), _Weight(I, d), _Weight(d, I)
            layer.self_attn, layer.mlp = att, mlp
            layer.input_layernorm, layer.post_attention_layernorm = _Weight(d, ones=True), _Weight(d, ones=True)
            layers.append(layer)
        self.model.layers = nn.ModuleList(layers)
        self.model.norm = _Weight(d, ones=True)
        if not c.tie_word_embeddings:
            self.lm_head = _Weight(c.vocab_size, d)
        self._packed = PackedSet()
        self._rope = None
        if trainable_layers is not None:
            for p in self._reference_trainable():
                p.requires_grad_(True)

    # ---- parameters
    def _head_weight(self) -> nn.Parameter:
        return self.model.embed_tokens.weight if self.config.tie_word_embeddings else self.lm_head.weight

    def _reference_trainable(self) -> list:
        """The parameters the reference trains: the last `trainable_layers` layers, the final norm, the output head."""
        first = self.config.num_hidden_layers - self.trainable_layers
        return [p for layer in self.model.layers[first:] for p in layer.parameters()] + [self.model.norm.weight, self._head_weight()]

    def get_input_embeddings(self) -> nn.Embedding:
        return self.model.embed_tokens

    def resize_token_embeddings(self, n: int) -> nn.Embedding:
        """Grows or shrinks the vocabulary to n rows (model.py:221): the rows both sizes share are kept, new rows are drawn as the old ones were initialised;
        the output head follows (the same tensor when tied)."""
        old = self.model.embed_tokens.weight

        def resized(w):
            out = torch.empty((n, w.shape[1]), dtype=w.dtype, device=w.device)
            nn.init.normal_(out, std=0.02)
            out[: min(n, w.shape[0])] = w[: min(n, w.shape[0])]
            return nn.Parameter(out, requires_grad=w.requires_grad)

        emb = nn.Embedding(n, old.shape[1], device=old.device, dtype=old.dtype)
        emb.weight = resized(old)
        self.model.embed_tokens = emb
        if not self.config.tie_word_embeddings:
            self.lm_head.weight = resized(self.lm_head.weight)
        self.config = dataclasses.replace(self.config, vocab_size=n)
        self._packed.invalidate()
        return emb

    def load_state_dict(self, state_dict, strict: bool = True, **kw):
        sd = {k: (v.float() if torch.is_tensor(v) and v.is_floating_point() else v) for k, v in state_dict.items()}
        if self.config.tie_word_embeddings:
            sd.pop("lm_head.weight", None)                                 # HF lists the tied head as a second name of the embedding
        out = super().load_state_dict(sd, strict=strict, **kw)
        self._packed.invalidate()
        return out

    def _apply(self, fn, *a, **kw):
        self._packed.invalidate()
        self._rope = None
        return super()._apply(fn, *a, **kw)

    def _pack(self) -> dict:
        """The fused q | k | v, o, gate | up and down projections of every layer and the output head as `awt_weight` handles (native_decoder.PackedSet).
        Inference only: packed once.  Trainable: with the transpose planes of `backward_input`, and following every parameter."""
        train = self.trainable_layers is not None

        def plan():
            plan = []
            for i, layer in enumerate(self.model.layers):
                att, mlp, where = layer.self_attn, layer.mlp, ("layers", i)
                plan += [(where, "qkv", (att.q_proj.weight, att.k_proj.weight, att.v_proj.weight), lambda att=att: (torch.cat([att.q_proj.weight, att.k_proj.weight, att.v_proj.weight]), None)),
                         (where, "o", (att.o_proj.weight,), lambda att=att: (att.o_proj.weight, None)),
                         (where, "gu", (mlp.gate_proj.weight, mlp.up_proj.weight), lambda mlp=mlp: (torch.cat([mlp.gate_proj.weight, mlp.up_proj.weight]), None)),
                         (where, "down", (mlp.down_proj.weight,), lambda mlp=mlp: (mlp.down_proj.weight, None))]
            return {"layers": [{} for _ in self.model.layers]}, plan + [((), "lm_head", (self._head_weight(),), lambda: (self._head_weight(), None))]

        return self._packed.refresh(list(self.parameters()) if train else None, plan, lambda w, b: PackedLinear(w, b, self.precision, backward=train))

    def _rope_tables(self, device):
        """cos / sin [max_position_embeddings, 64] fp32 as HF's Qwen3RotaryEmbedding forms them: fp32 inv_freq, fp32 outer product, then cos / sin."""
        if self._rope is None or self._rope[0].device != device:
            c = self.config
            inv_freq = 1.0 / (c.rope_theta ** (torch.arange(0, HEAD_DIM, 2, dtype=torch.int64).to(dtype=torch.float32) / HEAD_DIM))   # on the host, as HF does
            ang = torch.arange(c.max_position_embeddings, dtype=torch.float32)[:, None] * inv_freq[None, :]
            self._rope = (ang.cos().to(device).contiguous(), ang.sin().to(device).contiguous())
        return self._rope

    # ---- the layers
    def _check_input(self, x: torch.Tensor, graph_ok: bool = False) -> bool:
        """Validates inputs_embeds; True when the call has to build an autograd graph (a trainable decoder's `forward` with grad enabled)."""
        if x.dim() != 3 or x.shape[-1] != self.config.hidden_size:
            raise ValueError(f"inputs_embeds must be [B, L, {self.config.hidden_size}], got {tuple(x.shape)}")
        graph = torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in self.parameters()))
        if graph and self.trainable_layers is None:
            raise NotImplementedError("Qwen3Decoder is inference only: there is no backward through the decoder (call it under torch.no_grad(), with its "
                                      "parameters frozen), or build it with trainable_layers=K to train it")
        if graph and not graph_ok:
            raise NotImplementedError("Qwen3Decoder.prefill / step are inference only (call them under torch.no_grad()); `forward` is what builds a graph")
        _lib.ctx(x.device)                                                 # raises without a GPU: no CPU fallback
        return graph

    @staticmethod
    def _check_mask(m: Optional[torch.Tensor], B: int, L: int) -> None:
        if m is not None and (tuple(m.shape) != (B, L) or bool(((m != 0) & (m != 1)).any()) or bool((m[:, 1:] > m[:, :-1]).any())):
            raise ValueError("attention_mask must be [B, L] rows of ones followed by zeros (right padding); other masks are not supported")

    @torch.no_grad()
    def _run(self, inputs_embeds: torch.Tensor, cache: Qwen3Cache, last_only: bool, decode: bool = False) -> torch.Tensor:
        """Appends the L positions of inputs_embeds [B, L, hidden] to the cache; the lm_head GEMM's output [B * L, Np] (Np = vocab padded to the GEMM's N
        tile), or [B, Np] for the last position of each row with last_only.  decode (`step` at B <= DECODE_ROWS): the five linears run on the
        weight-streaming `awt_linear_decode` (`PackedLinear.forward_decode`) instead of the GEMM -- the same products, summed over K in another order."""
        c, dev = self.config, inputs_embeds.device
        B, L, d = inputs_embeds.shape
        if B != cache.batch or cache.length + L > cache.max_length:
            raise ValueError(f"the cache holds {cache.batch} rows of {cache.max_length} positions ({cache.length} live); cannot append [{B}, {L}]")
        Hq, Hkv, I, eps = c.num_attention_heads, c.num_key_value_heads, c.intermediate_size, c.rms_norm_eps
        M, T, wkv = B * L, cache.length + L, Hkv * HEAD_DIM
        packed, (cos, sin) = self._pack(), self._rope_tables(dev)
        positions = cache.ramp[cache.length:T]
        positions = positions if B == 1 else positions.repeat(B)
        linear = (lambda pl: pl.forward_decode) if decode else (lambda pl: pl.forward)
        x = inputs_embeds.float().reshape(M, d).contiguous()
        if x.data_ptr() == inputs_embeds.data_ptr():
            x = x.clone()                                                  # the residual GEMMs write x in place
        q = torch.empty((M, Hq * HEAD_DIM), dtype=torch.float32, device=dev)
        o = torch.empty_like(q)
        h = torch.empty_like(x)
        act = torch.empty((M, I), dtype=torch.float32, device=dev)
        ws = _lib.workspace(ops.causal_attention_workspace_bytes(B, Hq, L, T), dev)
        for i, (layer, pk) in enumerate(zip(self.model.layers, packed["layers"])):
            ops.rmsnorm((x, 0), d, layer.input_layernorm.weight, M, d, eps, y=(h, 0), ldy=d)
            qkv = linear(pk["qkv"])(h)
            ops.qk_norm_rope((qkv, 0), pk["qkv"].Np, layer.self_attn.q_norm.weight, layer.self_attn.k_norm.weight, cos, sin, positions, (q, 0), Hq * HEAD_DIM,
                             (cache.k[i], 0), (cache.v[i], 0), wkv, cache.max_length * wkv, B, L, Hq, Hkv, eps)
            ops.causal_attention((q, 0), Hq * HEAD_DIM, (cache.k[i], 0), (cache.v[i], 0), wkv, cache.max_length * wkv, B, Hq, Hkv, L, T, self.precision,
                                 o=(o, 0), ldo=Hq * HEAD_DIM, workspace=ws)
            linear(pk["o"])(o, resid=x, out=x)
            ops.rmsnorm((x, 0), d, layer.post_attention_layernorm.weight, M, d, eps, y=(h, 0), ldy=d)
            gu = linear(pk["gu"])(h)
            ops.silu_mul((gu, 0), pk["gu"].Np, M, I, y=(act, 0), ldy=I)
            linear(pk["down"])(act, resid=x, out=x)
        cache.length = T
        if last_only:
            x = x.view(B, L, d)[:, -1].contiguous()
        hn = ops.rmsnorm((x, 0), d, self.model.norm.weight, x.shape[0], d, eps)
        return linear(packed["lm_head"])(hn)

    def prefill(self, inputs_embeds: torch.Tensor, cache: Qwen3Cache) -> torch.Tensor:
        """Appends L positions to the cache (from position cache.length on); returns the last position's logits [B, vocab] (a view of the padded GEMM output)."""
        self._check_input(inputs_embeds)
        return self._run(inputs_embeds, cache, True)[:, : self.config.vocab_size]

    def step(self, inputs_embeds: torch.Tensor, cache: Qwen3Cache) -> torch.Tensor:
        """One new position per row: inputs_embeds [B, 1, hidden] -> logits [B, vocab].  Up to DECODE_ROWS rows the linears of the step, the lm_head among
        them, are weight-streaming launches (`awt_linear_decode`); beyond, the GEMM with B rows."""
        self._check_input(inputs_embeds)
        if inputs_embeds.shape[1] != 1:
            raise ValueError(f"step takes one position per row, got {inputs_embeds.shape[1]} (use prefill)")
        return self._run(inputs_embeds, cache, True, decode=inputs_embeds.shape[0] <= DECODE_ROWS)[:, : self.config.vocab_size]

    def forward(self, inputs_embeds: torch.Tensor, attention_mask: Optional[torch.Tensor] = None, labels: Optional[torch.Tensor] = None):
        """logits [B, L, vocab], and with labels (logits, loss): HF's causal-LM loss -- the logits at t against the label at t + 1, ignore_index -100, mean over
        the counted positions (awt_op_cross_entropy).  attention_mask: rows of ones followed by zeros (right padding) or None.  Under causality a live position
        never sees a padded one, so the mask changes nothing at live positions and is only validated; the outputs at padded positions are unspecified.
        A decoder built with `trainable_layers`, called with grad enabled, returns them with a graph (`_Qwen3Graph`): the loss is differentiable when labels
        are given (the logits beside it are then detached), else the logits are."""
        graph = self._check_input(inputs_embeds, graph_ok=True)
        B, L, _ = inputs_embeds.shape
        self._check_mask(attention_mask, B, L)
        if labels is not None and tuple(labels.shape) != (B, L):
            raise ValueError(f"labels must be [{B}, {L}], got {tuple(labels.shape)}")
        if graph:
            return self._forward_graph(inputs_embeds, labels)
        padded = self._run(inputs_embeds, Qwen3Cache(self.config, B, L, inputs_embeds.device), False)
        logits = padded.view(B, L, -1)[:, :, : self.config.vocab_size]
        if labels is None:
            return logits
        return logits, cross_entropy(padded, self._shifted(labels, padded.device).reshape(-1), self.config.vocab_size)[0]

    @staticmethod
    def _shifted(labels: torch.Tensor, device) -> torch.Tensor:
        """HF's causal-LM targets: position t is scored against the label at t + 1, the last position against nothing."""
        B, L = labels.shape
        shifted = torch.full((B, L), -100, dtype=torch.int64, device=device)
        shifted[:, :-1] = labels[:, 1:].to(device)
        return shifted

    def _forward_graph(self, inputs_embeds: torch.Tensor, labels: Optional[torch.Tensor]):
        B, L, _ = inputs_embeds.shape
        if L > self.config.max_position_embeddings:                        # the rotary tables' rows (the inference path checks it in Qwen3Cache)
            raise ValueError(f"inputs_embeds holds {L} positions, more than max_position_embeddings ({self.config.max_position_embeddings})")
        trained = [p for p in self.parameters() if p.requires_grad]
        holder: list = []
        shifted = None if labels is None else self._shifted(labels, inputs_embeds.device)
        out = _Qwen3Graph.apply(inputs_embeds, self, shifted, holder, *trained)
        if labels is None:
            return out.view(B, L, -1)[:, :, : self.config.vocab_size]
        return holder[0].view(B, L, -1)[:, :, : self.config.vocab_size], out


class _Qwen3Graph(torch.autograd.Function):
    """The decoder, its head and (with labels) HF's shifted cross-entropy as ONE autograd node with a hand-written native backward (the `_DecoderLoss`
    pattern of native_decoder.py): d / d(inputs_embeds) through every layer, and the gradient of every trainable parameter, each formed where its dY is live.

    Saved per layer (fp32, M = B L rows): the layer's input x0 and the stream after the attention half x1 [M, d] each, the pre-norm qkv [M, (Hq + 2 Hkv) 128],
    the rotated q and the attention output o [M, Hq 128] each, the layer's k / v cache [B, L, Hkv 128] each, lse [B, Hq, L], and gate | up [M, 2 I].  The two
    RMSNorm outputs h and the SwiGLU output act are NOT saved: the backward recomputes them (one row pass each), and only in trained layers, whose weight
    gradients are their only readers.  Without a gradient for inputs_embeds the layers below the first trained one save nothing and are not walked back.

    Returns the loss (labels given; the padded logits go to `holder`) or the padded logits [M, Np]."""

    @staticmethod
    def forward(ctx, inputs_embeds, dec: "Qwen3Decoder", shifted, holder, *trained):
        c, dev = dec.config, inputs_embeds.device
        B, L, d = inputs_embeds.shape
        Hq, Hkv, I, eps = c.num_attention_heads, c.num_key_value_heads, c.intermediate_size, c.rms_norm_eps
        M, wq, wkv = B * L, Hq * HEAD_DIM, Hkv * HEAD_DIM
        packed, (cos, sin) = dec._pack(), dec._rope_tables(dev)
        positions = torch.arange(L, dtype=torch.int32, device=dev).repeat(B)
        first_saved = 0 if inputs_embeds.requires_grad else c.num_hidden_layers - dec.trainable_layers
        x = inputs_embeds.detach().float().reshape(M, d).contiguous()
        if x.data_ptr() == inputs_embeds.data_ptr() and first_saved > 0:
            x = x.clone()                                                  # the unsaved layers' residual GEMMs write x in place
        h = torch.empty_like(x)
        act = torch.empty((M, I), dtype=torch.float32, device=dev)
        ws = _lib.workspace(ops.causal_attention_workspace_bytes(B, Hq, L, L), dev)
        saved = []
        for i, (layer, pk) in enumerate(zip(dec.model.layers, packed["layers"])):
            keep = i >= first_saved
            ops.rmsnorm((x, 0), d, layer.input_layernorm.weight, M, d, eps, y=(h, 0), ldy=d)
            qkv = pk["qkv"].forward(h)
            q, o = torch.empty((M, wq), dtype=torch.float32, device=dev), torch.empty((M, wq), dtype=torch.float32, device=dev)
            kc, vc = torch.empty((B, L, wkv), dtype=torch.float32, device=dev), torch.empty((B, L, wkv), dtype=torch.float32, device=dev)
            ops.qk_norm_rope((qkv, 0), pk["qkv"].Np, layer.self_attn.q_norm.weight, layer.self_attn.k_norm.weight, cos, sin, positions, (q, 0), wq,
                             (kc, 0), (vc, 0), wkv, L * wkv, B, L, Hq, Hkv, eps)
            _, lse = ops.causal_attention_lse((q, 0), wq, (kc, 0), (vc, 0), wkv, L * wkv, B, Hq, Hkv, L, L, dec.precision, o=(o, 0), ldo=wq, workspace=ws)
            x1 = pk["o"].forward(o, resid=x, out=torch.empty_like(x) if keep else x)
            ops.rmsnorm((x1, 0), d, layer.post_attention_layernorm.weight, M, d, eps, y=(h, 0), ldy=d)
            gu = pk["gu"].forward(h)
            ops.silu_mul((gu, 0), pk["gu"].Np, M, I, y=(act, 0), ldy=I)
            x2 = pk["down"].forward(act, resid=x1, out=torch.empty_like(x) if keep else x1)
            if keep:
                saved.append((x, qkv, q, kc, vc, o, lse, x1, gu))
            x = x2
        xf = ops.rmsnorm((x, 0), d, dec.model.norm.weight, M, d, eps)
        logits = packed["lm_head"].forward(xf)                             # [M, Np]
        ctx.dec, ctx.saved, ctx.first_saved, ctx.x_last, ctx.xf, ctx.shape, ctx.positions = dec, saved, first_saved, x, xf, (B, L), positions
        ctx.trained_ids = [id(p) for p in trained]
        if shifted is None:
            ctx.dlogits = None
            return logits
        loss, ctx.dlogits = cross_entropy(logits, shifted.reshape(-1), c.vocab_size)
        holder.append(logits)
        return loss

    @staticmethod
    def backward(ctx, g):
        dec, (B, L) = ctx.dec, ctx.shape
        c, prec = dec.config, dec.precision
        d, Hq, Hkv, I, eps = c.hidden_size, c.num_attention_heads, c.num_key_value_heads, c.intermediate_size, c.rms_norm_eps
        M, wq, wkv = B * L, Hq * HEAD_DIM, Hkv * HEAD_DIM
        pk, (cos, sin) = dec._pack(), dec._rope_tables(g.device)
        grads = {}                                                         # id(parameter) -> gradient

        # head: logits = RMSNorm(x) W^T.  The padding columns of dlogits are zero, so dW runs on the vocabulary rounded up to the weight-gradient GEMM's 8.
        dlogits = (g.contiguous() if ctx.dlogits is None else ctx.dlogits * g).float()
        dxf = pk["lm_head"].backward_input(dlogits)
        norm = dec.model.norm.weight
        grads[id(dec._head_weight())] = ops.weight_grad(dlogits, ctx.xf, n=ops.pad_to(c.vocab_size, 8), precision=prec)[: c.vocab_size]
        grads[id(norm)] = ops.rmsnorm_param_grad((dxf, 0), d, (ctx.x_last, 0), d, M, d, eps)
        dx = ops.rmsnorm_backward((dxf, 0), d, (ctx.x_last, 0), d, norm, M, d, eps)
        del dxf, dlogits

        first_trained = c.num_hidden_layers - dec.trainable_layers
        ws = _lib.workspace(ops.causal_attention_backward_workspace_bytes(B, Hq, L, L), dx.device)
        for i in range(c.num_hidden_layers - 1, ctx.first_saved - 1, -1):
            layer, p, trained = dec.model.layers[i], pk["layers"][i], i >= first_trained
            att, mlp = layer.self_attn, layer.mlp
            x0, qkv, q, kc, vc, o, lse, x1, gu = ctx.saved[i - ctx.first_saved]
            # MLP half: x2 = x1 + down(silu(gate) * up), gate | up = gu(RMSNorm(x1))
            dact = p["down"].backward_input(dx)
            dgu = ops.silu_mul_backward((gu, 0), p["gu"].Np, (dact, 0), I, M, I)
            dh = p["gu"].backward_input(dgu)
            if trained:
                grads[id(mlp.down_proj.weight)] = ops.weight_grad(dx, ops.silu_mul((gu, 0), p["gu"].Np, M, I), precision=prec)
                hn = ops.rmsnorm((x1, 0), d, layer.post_attention_layernorm.weight, M, d, eps)
                grads[id(mlp.gate_proj.weight)] = ops.weight_grad(dgu, hn, n=I, ycol=0, precision=prec)
                grads[id(mlp.up_proj.weight)] = ops.weight_grad(dgu, hn, n=I, ycol=I, precision=prec)
                grads[id(layer.post_attention_layernorm.weight)] = ops.rmsnorm_param_grad((dh, 0), d, (x1, 0), d, M, d, eps)
            ops.rmsnorm_backward((dh, 0), d, (x1, 0), d, layer.post_attention_layernorm.weight, M, d, eps, dres=(dx, 0), dx=(dx, 0), lddx=d)
            del dact, dgu, dh
            # attention half: x1 = x0 + o_proj(attention(qk_norm_rope(qkv(RMSNorm(x0)))))
            do = p["o"].backward_input(dx)
            dq = torch.empty_like(q)
            dkc, dvc = torch.empty_like(kc), torch.empty_like(vc)       # every element of all three is written
            ops.causal_attention_backward((q, 0), wq, (kc, 0), (vc, 0), wkv, L * wkv, (o, 0), (do, 0), wq, lse, (dq, 0), (dkc, 0), (dvc, 0), wkv, L * wkv,
                                          B, Hq, Hkv, L, L, prec, workspace=ws)
            dqkv = torch.empty_like(qkv)
            gains = ops.qk_norm_rope_backward((qkv, 0), p["qkv"].Np, att.q_norm.weight, att.k_norm.weight, cos, sin, ctx.positions, (dq, 0), wq, (dkc, 0), (dvc, 0),
                                              wkv, L * wkv, (dqkv, 0), B, L, Hq, Hkv, eps, want_gains=trained)
            dh = p["qkv"].backward_input(dqkv)
            if trained:
                grads[id(att.o_proj.weight)] = ops.weight_grad(dx, o, precision=prec)
                hn = ops.rmsnorm((x0, 0), d, layer.input_layernorm.weight, M, d, eps)
                for proj, n, col in ((att.q_proj, wq, 0), (att.k_proj, wkv, wq), (att.v_proj, wkv, wq + wkv)):      # the fused gradient, split by column
                    grads[id(proj.weight)] = ops.weight_grad(dqkv, hn, n=n, ycol=col, precision=prec)
                grads[id(att.q_norm.weight)], grads[id(att.k_norm.weight)] = gains
                grads[id(layer.input_layernorm.weight)] = ops.rmsnorm_param_grad((dh, 0), d, (x0, 0), d, M, d, eps)
            ops.rmsnorm_backward((dh, 0), d, (x0, 0), d, layer.input_layernorm.weight, M, d, eps, dres=(dx, 0), dx=(dx, 0), lddx=d)
            del do, dq, dkc, dvc, dqkv, dh
            ctx.saved[i - ctx.first_saved] = None
        ctx.saved = ctx.dlogits = ctx.xf = ctx.x_last = None
        dx_in = dx.view(B, L, d) if ctx.needs_input_grad[0] else None
        return (dx_in, None, None, None, *(grads[i] for i in ctx.trained_ids))


class _EmbedLookup(torch.autograd.Function):
    """weight[ids] whose backward ADDS the rows' gradients into a zeroed table with awt_op_embed_backward (one workgroup per table row, ascending order, no
    atomics) instead of torch's atomic scatter: the lookup side of the tied embedding's gradient.  autograd adds it to the head's side."""

    @staticmethod
    def forward(ctx, weight, ids):
        ctx.ids, ctx.rows = ids, weight.shape[0]
        return weight.detach()[ids]

    @staticmethod
    def backward(ctx, g):
        B, L = ctx.ids.shape
        d = g.shape[-1]
        dtok = torch.zeros((ctx.rows, d), dtype=torch.float32, device=g.device)
        dpos = torch.zeros((L, d), dtype=torch.float32, device=g.device)          # the operator's position table: not wanted here, thrown away
        embed_backward(ctx.ids, g.float().reshape(B * L, d).contiguous(), dtok, dpos)
        return dtok, None


class MusicTranscriptionModel(nn.Module):
    """The reference's MusicTranscriptionModel (model.py:190-344) from its three pieces: an audio tower (`WhisperAudioEncoder`, or any callable
    (waveforms, sampling_rate) -> [B, Sa, audio_dim]), the `CrossAttentionAdapter` and a `Qwen3Decoder`.  `forward` returns the teacher-forced loss,
    `generate` decodes with a KV cache.  With an inference-only decoder `forward` runs under `torch.no_grad()` only; with a decoder built with
    `trainable_layers` and grad enabled the loss is differentiable: the adapter, the decoder's trainable parameters and (tied) the embedding train, the
    audio tower runs under `no_grad` as in the reference (model.py:242-261)."""

    def __init__(self, audio_encoder, adapter: CrossAttentionAdapter, decoder: Qwen3Decoder, tokenizer=None):
        super().__init__()
        if adapter.text_dim != decoder.config.hidden_size:
            raise ValueError(f"the adapter's text_dim ({adapter.text_dim}) must be the decoder's hidden_size ({decoder.config.hidden_size})")
        self.audio_encoder, self.cross_attention_adapter, self.text_decoder, self.tokenizer = audio_encoder, adapter, decoder, tokenizer

    def _embed(self, ids: torch.Tensor) -> torch.Tensor:
        emb = self.text_decoder.get_input_embeddings()
        ids = ids.to(emb.weight.device)
        if torch.is_grad_enabled() and emb.weight.requires_grad:           # the tied embedding trains: its lookup's backward is awt_op_embed_backward
            return _EmbedLookup.apply(emb.weight, ids)
        return emb(ids)

    def forward(self, waveforms, sampling_rate: int, target_token_ids: torch.Tensor, attention_mask: Optional[torch.Tensor] = None) -> torch.Tensor:
        """The teacher-forced loss of model.py:263-288 (labels = target_token_ids, shifted inside).  The reference leaves the labels at padded positions as
        they are; so does this: pass -100 there through `target_token_ids`' own padding convention if they are to be ignored.  With grad enabled and a
        decoder built with `trainable_layers` the loss carries a graph; the audio tower runs under `no_grad` either way."""
        if torch.is_grad_enabled() and self.text_decoder.trainable_layers is None:
            raise NotImplementedError("MusicTranscriptionModel.forward is inference only with an inference-only decoder: the adapter's gradient needs a "
                                      "backward through the decoder (call it under torch.no_grad(), or build the decoder with trainable_layers=K)")
        with torch.no_grad():
            audio = self.audio_encoder(waveforms, sampling_rate)
        fused = self.cross_attention_adapter(self._embed(target_token_ids.clamp_min(0)), audio.float())
        return self.text_decoder(fused, attention_mask=attention_mask, labels=target_token_ids)[1]

    def trainable_state_dict(self) -> dict:
        """The requires_grad entries under the reference's names, `cross_attention_adapter.*` and `text_decoder.*` (train.py:285-288), detached;
        `load_state_dict(..., strict=False)` takes it back."""
        return {n: p.detach() for n, p in self.named_parameters() if p.requires_grad and n.startswith(("cross_attention_adapter.", "text_decoder."))}

    @torch.no_grad()
    def generate_batch(self, waveforms, sampling_rate: int, max_new_tokens: int = 256, temperature: float = 0.7, do_sample: bool = True,
                       generator: Optional[torch.Generator] = None, bos_token_id=None, eos_token_id: Optional[int] = None) -> list:
        """model.py:293-344 with a KV cache, for a non-empty list of clips; one entry per clip: the decoded string with a tokenizer, else the generated ids
        (EOS excluded, as the reference does).  The clips are decoded in groups of at most DECODE_ROWS: per group the audio tower runs once on the group's
        list, the audio is projected once (`encode_audio`), and each step runs the adapter on the NEW tokens' embeddings [B, 1] only -- the adapter is
        position-wise in the text and causal decoding over a cache equals full recomputation, so this is the reference's computation, not an approximation
        of it -- then `prefill` (the prompt) or `step`, the token choice on [B, vocab], and ONE host read of the B ids.  Every row starts from the same
        prompt.  A row that has produced EOS is finished: it is fed the EOS id from then on and what it produces is dropped; the loop ends when every row
        is finished or at max_new_tokens.  bos_token_id: the start token, or a sequence of prompt ids; with a tokenizer both ids default to its bos (else
        eos) / eos ids, without one they are required.  do_sample: torch.multinomial(softmax(logits / temperature)) with `generator`, the reference's
        expression; else argmax (awt_op_select_tokens)."""
        from .generation import select_tokens
        tok, dec = self.tokenizer, self.text_decoder
        waveforms = list(waveforms)
        if not waveforms:
            raise ValueError("generate_batch needs at least one clip")
        if bos_token_id is None and tok is not None:
            bos_token_id = tok.bos_token_id if tok.bos_token_id is not None else tok.eos_token_id
        if eos_token_id is None and tok is not None:
            eos_token_id = tok.eos_token_id
        if bos_token_id is None or eos_token_id is None:
            raise ValueError("generate needs bos_token_id and eos_token_id when the model has no tokenizer")
        if do_sample and not temperature > 0:
            raise ValueError("temperature must be positive when sampling")
        prompt = [int(bos_token_id)] if isinstance(bos_token_id, int) else [int(t) for t in bos_token_id]
        if not prompt or max_new_tokens < 1:
            raise ValueError("generate needs at least one prompt token and max_new_tokens >= 1")
        dev, vocab = dec.get_input_embeddings().weight.device, dec.config.vocab_size
        results = []
        for g0 in range(0, len(waveforms), DECODE_ROWS):
            group = waveforms[g0:g0 + DECODE_ROWS]
            B = len(group)
            audio = self.audio_encoder(group, sampling_rate)
            audio_kv = self.cross_attention_adapter.encode_audio(audio.float().to(dev))
            cache = Qwen3Cache(dec.config, B, len(prompt) + max_new_tokens - 1, dev)
            ids = torch.tensor([prompt] * B, dtype=torch.long, device=dev)
            out, done = [[] for _ in range(B)], [False] * B
            for n in range(max_new_tokens):
                fused = self.cross_attention_adapter(self._embed(ids), audio_kv=audio_kv)
                logits = dec.prefill(fused, cache) if n == 0 else dec.step(fused, cache)
                if do_sample:
                    ids = torch.multinomial(torch.softmax(logits / temperature, dim=-1), 1, generator=generator)
                else:
                    ids = select_tokens(logits, vocab)[1][:, :1]
                for b, nxt in enumerate(ids[:, 0].tolist()):               # the step's one host read
                    if not done[b]:
                        done[b] = nxt == eos_token_id
                        if not done[b]:
                            out[b].append(nxt)
                if all(done):
                    break
                if any(done):
                    ids = torch.where(torch.tensor(done, device=dev)[:, None], torch.full_like(ids, eos_token_id), ids)
            results += out
        return [tok.decode(o, skip_special_tokens=True) for o in results] if tok is not None else results

    def generate(self, waveform, sampling_rate: int, max_new_tokens: int = 256, temperature: float = 0.7, do_sample: bool = True,
                 generator: Optional[torch.Generator] = None, bos_token_id=None, eos_token_id: Optional[int] = None):
        """`generate_batch` for one clip: the decoded string with a tokenizer, else the generated ids (EOS excluded)."""
        return self.generate_batch([waveform], sampling_rate, max_new_tokens=max_new_tokens, temperature=temperature, do_sample=do_sample, generator=generator,
                                   bos_token_id=bos_token_id, eos_token_id=eos_token_id)[0]
