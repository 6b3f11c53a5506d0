"""`NativeWhisperDecoder`: the decoder half of `WhisperForConditionalGeneration.forward` on libawt (scope row f1).

Reference: /root/reference/AB/fineTune.py:131 loads `WhisperForConditionalGeneration`, `trainer.train()` (:186-199) calls its
forward with `input_features` and `labels`: shift labels right, encoder, decoder (pre-LN layers of causal self-attention,
cross-attention over the 1500 encoder positions, GELU MLP), tied vocabulary projection, cross-entropy with ignore_index -100
(HF:modeling_whisper.py:416-507, 649-797, 994-1100).

Everything after the encoder runs in libawt here (include/awt.h "Decoder-side operators"): the linears on the MFMA GEMM against
weights packed once (`awt_weight`), attention in the fp32 row kernels, embedding / LayerNorm / GELU / cross-entropy as row
kernels.  The decoder weights are frozen (only the encoder's adapters train), so the backward pass carries ONE gradient, d(loss) /
d(encoder hidden states), and the whole decoder + loss is a single autograd node (`_DecoderLoss`): no autograd graph, no per-layer
tensors beyond the activations the native backward needs, and the twelve layers' cross-attention key / value gradients are written
side by side into one buffer that a single GEMM turns into d(encoder hidden states).

Cross-attention in the training step runs in its ABSORBED form (`_AbsorbedCross`, csrc/bmm.hip): with L ~ 12 label rows per clip the key /
value projections of the B x 1500 encoder rows (2 x 768 x 768 MACs per row and decoder layer, forward and backward, plus a 7 GB key / value
tensor and its gradient at B = 64) are re-associated onto the query side -- scores = (q_h W_k,h) enc^T, context = (P_h enc) W_v,h^T + b_v --
so that each layer costs two [H L, d] x [d, S] products per clip against the encoder states themselves (packed once per step as the GEMM's B
operand and shared by all layers, forward and backward).  Exact re-association: results differ from the key / value form by rounding only.
`generate` / `forward` (many decoding steps against the same clip) keep the projected keys / values (`cross_kv`).

Parameter names are HF's (`WhisperDecoder.state_dict()` loads unchanged); `forward` has `finetune.WhisperDecoder`'s signature, so
`greedy_decode` / `generate` run on it as well (incremental decoding with a self-attention cache).

LoRA on the decoder (scope row f1, second half; build-defined like the encoder's adapters: y = x W^T + b + (alpha / r) (x A^T) B^T): with
`lora=LoraSpec(targets=("q_proj", "v_proj"))` the self-attention and the cross-attention query / value projections of every layer get
trainable `lora_A` [r, d] / `lora_B` [d, r] (B = 0 at init).  The base stays frozen and packed; the adapter terms and their gradients are
small GEMMs on the same MFMA kernel (`awt_op_linear`): du = dy B, dA = (alpha / r) du^T x, dB = (alpha / r) dy^T u, dx += (alpha / r) du A.
The cross-attention VALUE adapters act on the encoder states (B x 1500 rows): all layers' u = enc A^T come from one GEMM, and their share
of d(loss) / d(encoder states) from one more.

Full-parameter fine-tuning (`train_base=True`): every base parameter requires grad, the backward also forms their gradients
(weight-gradient GEMM, pitched column sums, LayerNorm parameter gradients, `awt_op_embed_backward` for the tied table and the positions), and
`packed()` re-packs the stepped weights into the handles it already has (`awt_weight_update`): its plan runs on `PackedSet`, the one tracker of
parameter versions (music2midi's decoder uses it too).  A `PackedLinear` owns its handle and refuses copy / pickle; a copied `PackedSet` is empty.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Dict, List, Optional, Tuple

import torch
import torch.nn as nn

from . import _lib, ops

_PREC = {name: ops._TERMS[name] for name in ("bf16", "bf16x3")}          # the operand planes `awt_weight` packs, out of ops' PREC_* table


class PackedLinear:
    """A frozen nn.Linear packed once into libawt's fragment-major operand planes (`awt_weight`)."""

    def __init__(self, weight: torch.Tensor, bias: Optional[torch.Tensor], precision: str = "bf16x3", backward: bool = True):
        w = weight.detach().float().contiguous()
        b = None if bias is None else bias.detach().float().contiguous()
        self.N, self.K = w.shape
        self.device = w.device
        out = C.c_void_p()
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib().awt_weight_create(_lib.ctx(self.device), _lib.ptr(w), _lib.ptr(b), self.N, self.K, _PREC[precision], int(backward),
                                                    _lib.stream_handle(), C.byref(out)))
        self.handle = out.value
        self.Np = int(_lib.lib().awt_weight_padded_rows(self.handle))

    def forward(self, x: torch.Tensor, resid: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """y [M, Np] = x [M, K] W^T + b (+ resid)."""
        L = _lib.lib()
        M = x.shape[0]
        y = torch.empty((M, self.Np), dtype=torch.float32, device=x.device) if out is None else out
        ws = _lib.workspace(L.awt_linear_workspace_bytes(self.handle, M, 0), x.device)
        with torch.cuda.device(x.device):
            _lib.check(L.awt_linear_forward(_lib.ctx(x.device), self.handle, _lib.ptr(x), _lib.ptr(resid), _lib.ptr(y), M, _lib.ptr(ws), ws.numel(),
                                            _lib.stream_handle()))
        return y

    def forward_decode(self, x: torch.Tensor, resid: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """`forward` for the 1 <= M <= 8 rows of incremental decoding (`awt_linear_decode`): one weight-streaming launch, no workspace, no plane split;
        any other M raises.  Row m of the result does not depend on M."""
        M = x.shape[0]
        y = torch.empty((M, self.Np), dtype=torch.float32, device=x.device) if out is None else out
        with torch.cuda.device(x.device):
            _lib.check(_lib.lib().awt_linear_decode(_lib.ctx(x.device), self.handle, _lib.ptr(x), _lib.ptr(resid), _lib.ptr(y), M, _lib.stream_handle()))
        return y

    def backward_input(self, dy: torch.Tensor) -> torch.Tensor:
        """dx [M, K] = dy [M, Np] W."""
        L = _lib.lib()
        M = dy.shape[0]
        dx = torch.empty((M, self.K), dtype=torch.float32, device=dy.device)
        ws = _lib.workspace(L.awt_linear_workspace_bytes(self.handle, M, 1), dy.device)
        with torch.cuda.device(dy.device):
            _lib.check(L.awt_linear_backward_input(_lib.ctx(dy.device), self.handle, _lib.ptr(dy), _lib.ptr(dx), M, _lib.ptr(ws), ws.numel(),
                                                   _lib.stream_handle()))
        return dx

    def update(self, weight: torch.Tensor, bias: Optional[torch.Tensor]) -> None:
        """Re-packs a changed weight (and bias) into this handle's planes, in place (`awt_weight_update`): what a trained decoder does after
        an optimizer step instead of building a new handle."""
        w = weight.detach().float().contiguous()
        b = None if bias is None else bias.detach().float().contiguous()
        if tuple(w.shape) != (self.N, self.K) or (b is not None and tuple(b.shape) != (self.N,)):
            raise ValueError(f"PackedLinear.update: the handle holds a [{self.N}, {self.K}] weight, got {tuple(w.shape)}"
                             + ("" if b is None else f" with bias {tuple(b.shape)}"))
        if w.device != self.device:
            raise ValueError(f"PackedLinear.update: the handle lives on {self.device}, the weight on {w.device}")
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib().awt_weight_update(_lib.ctx(self.device), self.handle, _lib.ptr(w), _lib.ptr(b), _lib.stream_handle()))

    def __reduce_ex__(self, protocol):
        raise TypeError("PackedLinear owns a library handle (awt_weight) that its __del__ frees: it cannot be copied or pickled; pack the weight again")

    def __del__(self):
        try:
            if self.handle:
                _lib.lib().awt_weight_destroy(self.handle)
        except Exception:
            pass


# ------------------------------------------------------------------------------------------------ thin op wrappers
VALIDATE_LABELS = os.environ.get("AWT_VALIDATE_LABELS", "0") == "1"   # cross_entropy: range-check device labels on the host (a stream synchronisation per call)

def _ctx(t):
    return _lib.ctx(t.device)


def layernorm(x, g, b, eps=1e-5):
    y = torch.empty_like(x)
    with torch.cuda.device(x.device):
        _lib.check(_lib.lib().awt_op_layernorm(_ctx(x), _lib.ptr(x), _lib.ptr(g), _lib.ptr(b), _lib.ptr(y), x.shape[0], x.shape[1], eps, _lib.stream_handle()))
    return y


def layernorm_backward(dy, x, g, dres=None, eps=1e-5):
    dx = torch.empty_like(x)
    with torch.cuda.device(x.device):
        _lib.check(_lib.lib().awt_op_layernorm_backward(_ctx(x), _lib.ptr(dy), _lib.ptr(x), _lib.ptr(g), _lib.ptr(dres), _lib.ptr(dx), x.shape[0], x.shape[1],
                                                        eps, _lib.stream_handle()))
    return dx


def gelu(x):
    y = torch.empty_like(x)
    with torch.cuda.device(x.device):
        _lib.check(_lib.lib().awt_op_gelu(_ctx(x), _lib.ptr(x), _lib.ptr(y), x.numel(), _lib.stream_handle()))
    return y


def gelu_backward(x, dy):
    dx = torch.empty_like(x)
    with torch.cuda.device(x.device):
        _lib.check(_lib.lib().awt_op_gelu_backward(_ctx(x), _lib.ptr(x), _lib.ptr(dy), _lib.ptr(dx), x.numel(), _lib.stream_handle()))
    return dx


def attention_small(q, ldq, k, ldk, v, ldv, B, H, Lq, Sk, causal, causal_off, want_lse=True, drop_p=0.0, seed=0):
    """q / k / v: (tensor, column offset in elements) pairs over row-major fp32 matrices; returns o [B * Lq, H * 64] and lse [B, H, Lq].
    drop_p > 0: attention-probability dropout with the seeded in-kernel mask (include/awt.h awt_op_attention_small_dropout)."""
    (qt, qo), (kt, ko), (vt, vo) = q, k, v
    o = torch.empty((B * Lq, H * 64), dtype=torch.float32, device=qt.device)
    lse = torch.empty((B, H, Lq), dtype=torch.float32, device=qt.device) if want_lse else None
    with torch.cuda.device(qt.device):
        _lib.check(_lib.lib().awt_op_attention_small_dropout(_ctx(qt), qt.data_ptr() + 4 * qo, ldq, kt.data_ptr() + 4 * ko, ldk, vt.data_ptr() + 4 * vo, ldv,
                                                             _lib.ptr(o), H * 64, _lib.ptr(lse), B, H, Lq, Sk, int(causal), int(causal_off), float(drop_p), int(seed),
                                                             _lib.stream_handle()))
    return o, lse


def attention_small_backward(q, ldq, k, ldk, v, ldv, o, dout, lse, dq, dk, dv, B, H, Lq, Sk, causal, causal_off, drop_p=0.0, seed=0):
    """Writes dq / dk / dv at (tensor, column offset) destinations laid out like q / k / v."""
    (qt, qo), (kt, ko), (vt, vo) = q, k, v
    (dqt, dqo), (dkt, dko), (dvt, dvo) = dq, dk, dv
    delta = torch.empty((B, H, Lq), dtype=torch.float32, device=qt.device)
    with torch.cuda.device(qt.device):
        _lib.check(_lib.lib().awt_op_attention_small_backward_dropout(
            _ctx(qt), qt.data_ptr() + 4 * qo, ldq, kt.data_ptr() + 4 * ko, ldk, vt.data_ptr() + 4 * vo, ldv, _lib.ptr(o), _lib.ptr(dout), H * 64, _lib.ptr(lse),
            _lib.ptr(delta), dqt.data_ptr() + 4 * dqo, dkt.data_ptr() + 4 * dko, dvt.data_ptr() + 4 * dvo, B, H, Lq, Sk, int(causal), int(causal_off),
            float(drop_p), int(seed), _lib.stream_handle()))


def attention_cached(q, ldq, cache, T, H, Lq):
    """Causal attention of Lq new query rows per cache row over the first T positions of a decode cache [rows, Tmax, 2 H 64] (keys in the first
    H * 64 columns, values in the rest; positions >= T are not read).  q: (tensor, column offset) as in attention_small; returns o [rows * Lq, H * 64]."""
    qt, qo = q
    rows, Tmax, width = cache.shape
    d = H * 64
    o = torch.empty((rows * Lq, d), dtype=torch.float32, device=qt.device)
    with torch.cuda.device(qt.device):
        _lib.check(_lib.lib().awt_op_attention_cached(_ctx(qt), qt.data_ptr() + 4 * qo, ldq, cache.data_ptr(), cache.data_ptr() + 4 * d, width, Tmax * width,
                                                      _lib.ptr(o), d, rows, H, Lq, T, _lib.stream_handle()))
    return o


def embed(ids: torch.Tensor, tok: torch.Tensor, pos: torch.Tensor, position_offset: int = 0) -> torch.Tensor:
    """ids [B, L] -> x [B * L, d] = tok[ids] + pos[position_offset + column] (awt_op_embed; an id outside [0, vocab) reads the nearest valid row)."""
    B, L = ids.shape
    vocab, d = tok.shape
    ids = ids.to(device=tok.device, dtype=torch.int64).contiguous()
    x = torch.empty((B * L, d), dtype=torch.float32, device=tok.device)
    with torch.cuda.device(tok.device):
        _lib.check(_lib.lib().awt_op_embed(_ctx(tok), _lib.ptr(ids), _lib.ptr(tok), _lib.ptr(pos), _lib.ptr(x), B * L, L, d, int(position_offset), vocab,
                                           _lib.stream_handle()))
    return x


def embed_backward(ids: torch.Tensor, dx: torch.Tensor, dtok: torch.Tensor, dpos: torch.Tensor, position_offset: int = 0) -> None:
    """Adds the backward of `embed` to the two tables' gradients: dtok[clamp(ids[m])] += dx[m], dpos[position_offset + column] += dx[m]
    (awt_op_embed_backward: no atomics, every table row's terms added in ascending m)."""
    B, L = ids.shape
    vocab, d = dtok.shape
    ids = ids.to(device=dx.device, dtype=torch.int64).contiguous()
    if dx.shape != (B * L, d) or dpos.shape[1] != d or dpos.shape[0] < position_offset + L:
        raise ValueError("embed_backward: dx must be [B * L, d] and dpos must hold position_offset + L rows of d")
    with torch.cuda.device(dx.device):
        _lib.check(_lib.lib().awt_op_embed_backward(_ctx(dx), _lib.ptr(ids), _lib.ptr(dx), _lib.ptr(dtok), _lib.ptr(dpos), B * L, L, d, int(position_offset),
                                                    vocab, _lib.stream_handle()))


def column_sums_ld(a: torch.Tensor, col: int = 0, width: Optional[int] = None, out: Optional[torch.Tensor] = None, accumulate: bool = False) -> torch.Tensor:
    """sums[c] (+)= sum_m a[m, col + c] for c < width over a row-major [M, ld] matrix (awt_op_column_sums_ld; bias gradients)."""
    M, ld = a.shape
    width = ld - col if width is None else width
    if out is None:
        if accumulate:
            raise ValueError("column_sums_ld: accumulate needs out")
        out = torch.empty(width, dtype=torch.float32, device=a.device)
    if out.shape != (width,):
        raise ValueError(f"column_sums_ld: out must hold {width} elements")
    L = _lib.lib()
    ws = _lib.workspace(L.awt_op_column_sums_ld_workspace_bytes(M, width), a.device)
    with torch.cuda.device(a.device):
        _lib.check(L.awt_op_column_sums_ld(_ctx(a), _lib.ptr(a), ld, int(col), int(width), _lib.ptr(out), M, int(accumulate), _lib.ptr(ws), ws.numel(),
                                           _lib.stream_handle()))
    return out


def layernorm_param_grad(dy: torch.Tensor, x: torch.Tensor, eps: float = 1e-5) -> Tuple[torch.Tensor, torch.Tensor]:
    """(dgamma, dbeta) of y = LayerNorm(x) gamma + beta for the gradient dy (awt_op_layernorm_param_grad)."""
    M, d = x.shape
    dg = torch.empty(d, dtype=torch.float32, device=x.device)
    db = torch.empty_like(dg)
    L = _lib.lib()
    ws = _lib.workspace(L.awt_op_param_grad_workspace_bytes(M, d), x.device)
    with torch.cuda.device(x.device):
        _lib.check(L.awt_op_layernorm_param_grad(_ctx(x), _lib.ptr(dy), _lib.ptr(x), _lib.ptr(dg), _lib.ptr(db), M, d, eps, _lib.ptr(ws), ws.numel(),
                                                 _lib.stream_handle()))
    return dg, db


def column_sums(a: torch.Tensor) -> torch.Tensor:
    """sums[c] = sum_m a[m, c] over a contiguous [M, d] matrix, d <= 1280 (awt_op_column_sums; bias gradients of the classifiers)."""
    M, d = a.shape
    out = torch.empty(d, dtype=torch.float32, device=a.device)
    L = _lib.lib()
    ws = _lib.workspace(L.awt_op_param_grad_workspace_bytes(M, d), a.device)
    with torch.cuda.device(a.device):
        _lib.check(L.awt_op_column_sums(_ctx(a), _lib.ptr(a), _lib.ptr(out), M, d, _lib.ptr(ws), ws.numel(), _lib.stream_handle()))
    return out


def gemm(x: torch.Tensor, w: torch.Tensor, precision: str = "bf16x3", bias: Optional[torch.Tensor] = None) -> torch.Tensor:
    """x [M, K] @ w [N, K]^T (+ bias [N]) on libawt's MFMA GEMM (`awt_op_linear`): K zero-padded to a multiple of 64, N to a multiple of 128."""
    pad = torch.nn.functional.pad
    M, K = x.shape
    N = w.shape[0]
    kp, np_ = ops.pad_to(K, 64), ops.pad_to(N, 128)
    if kp != K:
        x, w = pad(x, (0, kp - K)), pad(w, (0, kp - K))
    if np_ != N:
        w = pad(w, (0, 0, 0, np_ - N))
        bias = pad(bias, (0, np_ - N)) if bias is not None else None
    return ops.linear(x, w, bias, precision)[:, :N]                  # ops.linear makes its operands fp32 and contiguous


class PackedBatch:
    """B operands of `bmm`, packed once into the GEMM's fragment-major weight planes: fp32 [batch, N, K] (contiguous; `awt_bmm_pack`), or with
    `kmajor=((t1, off1), (t2, off2) | None, K1, ld, stride, batch, N, K)` the operand given transposed in memory, B_z[n, k] =
    (k < K1 ? t1 : t2)[off + z stride + (k | k - K1) ld + n] (`awt_bmm_pack_kmajor`)."""

    def __init__(self, b: Optional[torch.Tensor] = None, kmajor=None):
        L = _lib.lib()
        if kmajor is None:
            b = b.detach().float().contiguous()
            self.batch, self.N, self.K = b.shape
            dev = b.device
        else:
            (t1, o1), second, K1, ld, stride, self.batch, self.N, self.K = kmajor
            dev = t1.device
        nbytes = int(L.awt_bmm_packed_bytes(self.batch, self.N, self.K))
        self.buf = _lib.workspace(nbytes, dev)
        with torch.cuda.device(dev):
            if kmajor is None:
                _lib.check(L.awt_bmm_pack(_lib.ctx(dev), _lib.ptr(b), self.K, self.N * self.K, self.batch, self.N, self.K, _lib.ptr(self.buf), self.buf.numel(),
                                          _lib.stream_handle()))
            else:
                p2 = None if second is None else second[0].data_ptr() + 4 * second[1]
                _lib.check(L.awt_bmm_pack_kmajor(_lib.ctx(dev), t1.data_ptr() + 4 * o1, p2, K1, ld, stride, self.batch, self.N, self.K, _lib.ptr(self.buf),
                                                 self.buf.numel(), _lib.stream_handle()))

    def update(self, b: torch.Tensor) -> None:
        """Packs changed operands of the same [batch, N, K] shape into the existing buffer (`awt_bmm_pack` again; no allocation)."""
        b = b.detach().float().contiguous()
        if tuple(b.shape) != (self.batch, self.N, self.K) or b.device != self.buf.device:
            raise ValueError(f"PackedBatch.update: the buffer holds [{self.batch}, {self.N}, {self.K}] operands on {self.buf.device}, got {tuple(b.shape)} on {b.device}")
        with torch.cuda.device(b.device):
            _lib.check(_lib.lib().awt_bmm_pack(_lib.ctx(b.device), _lib.ptr(b), self.K, self.N * self.K, self.batch, self.N, self.K, _lib.ptr(self.buf),
                                               self.buf.numel(), _lib.stream_handle()))


class PackedSet:
    """The packed objects of one module (`objects`: a dict of PackedLinear / PackedBatch, or None) and the parameter versions they were packed from.
    A copy or a pickle of it is EMPTY: the copy of a model packs its own weights at first use and never shares or frees the original's handles."""
    objects = _versions = None

    def __reduce_ex__(self, protocol):
        return PackedSet, ()

    def invalidate(self) -> None:
        self.objects = None               # the next `refresh` builds every object: after load_state_dict, _apply (.to(), .float()), a resized table

    def refresh(self, params, plan, new) -> dict:
        """`objects`, brought up to date with `params`: the parameters to watch (walked once per call), or None to pack once and follow nothing.
        plan() -> (the empty result, [(where, key, sources, make)]): result[key], or result[name][i][key] with where = (name, i), is made of the
        parameters `sources` out of the operand tuple make() returns.  The same Parameter objects at new versions (an optimizer step) pack only the
        entries with a changed source again, in place (`update(*operands)`); anything else builds every object (`new(*operands)`)."""
        vers = None if params is None else [(id(p), p._version) for p in params]           # identity too: a replaced Parameter starts at version 0 again
        if self.objects is not None and self._versions == vers:
            return self.objects
        fresh = self.objects is None or None in (vers, self._versions) or [i for i, _ in self._versions] != [i for i, _ in vers]
        changed = set() if fresh else {i for (i, v), (_, v0) in zip(vers, self._versions) if v != v0}
        pk, entries = plan()
        pk = pk if fresh else self.objects
        with torch.no_grad():
            for where, key, sources, make in entries:
                slot = pk[where[0]][where[1]] if where else pk
                if fresh:
                    slot[key] = new(*make())
                elif any(id(p) in changed for p in sources):
                    slot[key].update(*make())
        self.objects, self._versions = pk, vers
        return pk


def bmm(a, pb: PackedBatch, M: int, out, resid=None, a_kmajor=None) -> None:
    """out_z [M, N] = a_z [M, K] B_z^T (+ resid_z) for z < pb.batch.  `a`, `out`, `resid`: (tensor, element offset, row pitch, matrix stride) views
    of row-major fp32 storage (`resid` shares the output's pitch / stride and may be the output itself).  `a_kmajor=((t1, off1), (t2, off2) | None,
    K1, ld, stride)` instead of `a`: the left operand given transposed in memory, optionally as two matrices stacked along K (as PackedBatch)."""
    ot, oo, ldo, so = out
    dev = ot.device
    L = _lib.lib()
    ws = _lib.workspace(L.awt_bmm_workspace_bytes(pb.batch, M, pb.K), dev)
    rp = None
    if resid is not None:
        rt, ro, ldr, sr = resid
        if (ldr, sr) != (ldo, so):
            raise ValueError("bmm: the residual must have the output's pitch and stride")
        rp = rt.data_ptr() + 4 * ro
    with torch.cuda.device(dev):
        if a_kmajor is None:
            at, ao, lda, sa = a
            _lib.check(L.awt_bmm(_lib.ctx(dev), at.data_ptr() + 4 * ao, lda, sa, _lib.ptr(pb.buf), rp, ot.data_ptr() + 4 * oo, ldo, so, pb.batch, M, pb.N, pb.K,
                                 _lib.ptr(ws), ws.numel(), _lib.stream_handle()))
        else:
            (t1, o1), second, K1, lda, sa = a_kmajor
            p2 = None if second is None else second[0].data_ptr() + 4 * second[1]
            _lib.check(L.awt_bmm_kmajor(_lib.ctx(dev), t1.data_ptr() + 4 * o1, p2, K1, lda, sa, _lib.ptr(pb.buf), rp, ot.data_ptr() + 4 * oo, ldo, so, pb.batch,
                                        M, pb.N, pb.K, _lib.ptr(ws), ws.numel(), _lib.stream_handle()))


def softmax_rows(s: torch.Tensor, cols: int, scale: float) -> torch.Tensor:
    """In place: rows of the 2-D view [rows, ld] -> softmax(scale * row[:cols])."""
    rows, ld = s.shape
    with torch.cuda.device(s.device):
        _lib.check(_lib.lib().awt_op_softmax_rows(_ctx(s), _lib.ptr(s), _lib.ptr(s), rows, cols, ld, scale, _lib.stream_handle()))
    return s


def softmax_rows_backward(p: torch.Tensor, dp: torch.Tensor, cols: int, scale: float) -> torch.Tensor:
    """In place on dp: scale * p * (dp - rowsum(p dp))."""
    rows, ld = p.shape
    with torch.cuda.device(p.device):
        _lib.check(_lib.lib().awt_op_softmax_rows_backward(_ctx(p), _lib.ptr(p), _lib.ptr(dp), _lib.ptr(dp), rows, cols, ld, scale, _lib.stream_handle()))
    return dp


class _AbsorbedCross:
    """One step's cross-attention over the encoder states `enc` [B, S, d] with the key / value projections moved to the query side (module
    docstring).  Rows of the per-clip matrices are ordered r = l * H + h, so that [B L, H, d] storage is at once `H` strided per-head matrices
    (pitch H d, stride d) and `B` per-clip matrices [L H, d].  HF:modeling_whisper.py:284-356."""

    ROW_LIMIT = 512          # H L above which the projected keys / values (cross_kv) are the cheaper form: 6 H L > 4 d

    def __init__(self, dec: "NativeWhisperDecoder", enc: torch.Tensor):
        self.dec = dec
        self.B, self.S, self.d = enc.shape
        self.Sp = (self.S + 3) // 4 * 4
        self.enc_p = PackedBatch(enc)                                           # B operand [S, d] of scores and dP
        self.encT_p = PackedBatch(enc.transpose(1, 2))                          # B operand [d, S] of the context and d(q~)
        self.eff: Dict[int, dict] = {}

    def _heads(self, i: int) -> dict:
        """Per-head blocks of layer i's key / value projections as batched B operands; with a value adapter the merged weight
        W_v + (alpha / r) B A of this step (the adapter's gradient comes back through d(merged weight), `backward`)."""
        dec, H, d = self.dec, self.dec.heads, self.d
        pk = dec.packed()["cross_heads"][i]
        ab = dec._adapter(i, "encoder_attn", "v_proj")
        if ab is None:
            return pk
        if i not in self.eff:
            A, Bm = ab
            wv = dec.layers[i].encoder_attn.v_proj.weight.detach() + gemm(Bm.detach(), A.detach().t().contiguous(), dec.precision) * dec.lora.scale
            self.eff[i] = dict(pk, v=PackedBatch(wv.view(H, 64, d)), vT=PackedBatch(wv.view(H, 64, d).transpose(1, 2)))
        return self.eff[i]

    def attend(self, i: int, q: torch.Tensor, L: int):
        """q [B L, d] (bias and adapter applied, unscaled) -> (attention output [B L, d] before out_proj, what `backward` needs)."""
        B, S, Sp, d, H = self.B, self.S, self.Sp, self.d, self.dec.heads
        R, M = L * H, B * L
        hw = self._heads(i)
        dev = q.device
        qt = torch.empty((M, H, d), dtype=torch.float32, device=dev)
        bmm((q, 0, d, 64), hw["kT"], M, (qt, 0, H * d, d))                                      # q~_h = q_h W_k,h
        P = torch.empty((B * R, Sp), dtype=torch.float32, device=dev)
        bmm((qt, 0, d, R * d), self.enc_p, R, (P, 0, Sp, R * Sp))                                # scores = q~ enc^T
        softmax_rows(P, S, 0.125)
        c = torch.empty((M, H, d), dtype=torch.float32, device=dev)
        bmm((P, 0, Sp, R * Sp), self.encT_p, R, (c, 0, d, R * d))                                # context = P enc
        a2 = torch.empty((M, d), dtype=torch.float32, device=dev)
        bmm((c, 0, H * d, d), hw["v"], M, (a2, 0, d, 64))                                        # (P enc) W_v,h^T
        a2 += self.dec.layers[i].encoder_attn.v_proj.bias                                       # rows of P sum to one
        return a2, (qt, P, c)

    def backward(self, i: int, saved, da2: torch.Tensor, d_enc: Optional[torch.Tensor], L: int, grads: dict, q: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Adds this layer's share of d(loss) / d(encoder states) to `d_enc` [B, S, d] (None: nobody needs it); returns dq [B L, d].
        `q` (the saved query rows, bias applied, unscaled; decoder in train_base mode): also records d(loss) / d(k_proj.weight, v_proj.weight,
        v_proj.bias) of this layer in `grads`: dW_k,h = q_h^T d(q~)_h, dW_v,h = da2_h^T context_h, db_v = column sums of da2."""
        B, S, Sp, d, H = self.B, self.S, self.Sp, self.d, self.dec.heads
        R, M = L * H, B * L
        qt, P, c = saved
        hw = self._heads(i)
        dev = da2.device
        da2 = da2.contiguous()
        dc = torch.empty((M, H, d), dtype=torch.float32, device=dev)
        bmm((da2, 0, d, 64), hw["vT"], M, (dc, 0, H * d, d))                                     # d(context)_h = da2_h W_v,h
        dS = torch.empty((B * R, Sp), dtype=torch.float32, device=dev)
        bmm((dc, 0, d, R * d), self.enc_p, R, (dS, 0, Sp, R * Sp))                               # dP = d(context) enc^T
        softmax_rows_backward(P, dS, S, 0.125)
        dqt = torch.empty((M, H, d), dtype=torch.float32, device=dev)
        bmm((dS, 0, Sp, R * Sp), self.encT_p, R, (dqt, 0, d, R * d))                             # d(q~) = dS enc
        # d(enc)_b += P_b^T d(context)_b + dS_b^T q~_b : one [S, 2 R] x [2 R, d] product per clip
        # (all four matrices are read where they lie: both operands are K-major, two blocks stacked along K)
        if d_enc is not None:
            rhs = PackedBatch(kmajor=((dc, 0), (qt, 0), R, d, R * d, B, d, 2 * R))               # B operand [d, 2 R] = [d(context)_b ; q~_b]^T
            bmm(None, rhs, S, (d_enc, 0, d, S * d), resid=(d_enc, 0, d, S * d), a_kmajor=((P, 0), (dS, 0), R, Sp, R * Sp))
        dq = torch.empty((M, d), dtype=torch.float32, device=dev)
        bmm((dqt, 0, H * d, d), hw["k"], M, (dq, 0, d, 64))                                      # dq_h = d(q~)_h W_k,h^T
        ab = self.dec._adapter(i, "encoder_attn", "v_proj")
        if ab is not None or q is not None:                                                      # d(W_v)_h = da2_h^T context_h (W_v: the merged weight under an adapter)
            dw = torch.empty((d, d), dtype=torch.float32, device=dev)
            bmm(None, PackedBatch(kmajor=((c, 0), None, M, H * d, d, H, d, M)), 64, (dw, 0, d, 64 * d), a_kmajor=((da2, 0), None, M, d, 64))
        if q is not None:
            ca = self.dec.layers[i].encoder_attn
            dwk = torch.empty((d, d), dtype=torch.float32, device=dev)                           # d(W_k)_h = q_h^T d(q~)_h (d(q~) carries the 0.125)
            bmm(None, PackedBatch(kmajor=((dqt, 0), None, M, H * d, d, H, d, M)), 64, (dwk, 0, d, 64 * d), a_kmajor=((q, 0), None, M, d, 64))
            grads[id(ca.k_proj.weight)], grads[id(ca.v_proj.weight)] = dwk, dw
            grads[id(ca.v_proj.bias)] = column_sums_ld(da2)                                      # rows of P sum to one
        if ab is not None:                                                                       # through W_v + s B A
            A, Bm = ab
            scale, prec = self.dec.lora.scale, self.dec.precision
            grads[id(Bm)] = gemm(dw, A.detach(), prec) * scale                                   # dB [d, r] = s dW A^T
            grads[id(A)] = gemm(Bm.detach().t().contiguous(), dw.t().contiguous(), prec) * scale  # dA [r, d] = s B^T dW
        return dq


def cross_entropy(logits, labels, vocab):
    """(loss scalar tensor, dlogits [M, ld]) of CrossEntropyLoss(ignore_index=-100) over the first `vocab` columns."""
    M, ld = logits.shape
    flat = labels.reshape(-1)
    if VALIDATE_LABELS or not flat.is_cuda:
        # torch.nn.CrossEntropyLoss raises for targets outside [0, vocab) other than -100; so do we -- but on device labels that check is a host
        # synchronisation in front of every loss launch, so it runs only for host labels (free) or when AWT_VALIDATE_LABELS=1 asks for it:
        # the kernel itself poisons the loss with NaN for an out-of-range device target (tests/test_gpu_native_decoder.py), which a training loop sees at once
        bad = (flat != -100) & ((flat < 0) | (flat >= vocab))
        if bool(bad.any()):
            raise IndexError(f"Target {int(flat[bad][0])} is out of bounds.")
    loss = torch.empty((), dtype=torch.float32, device=logits.device)
    dlogits = torch.empty_like(logits)
    scratch = torch.empty(M + 1, dtype=torch.float32, device=logits.device)
    lab = labels.reshape(-1).to(device=logits.device, dtype=torch.int64).contiguous()
    with torch.cuda.device(logits.device):
        _lib.check(_lib.lib().awt_op_cross_entropy(_ctx(logits), _lib.ptr(logits), _lib.ptr(lab), M, vocab, ld, _lib.ptr(loss), _lib.ptr(dlogits),
                                                   _lib.ptr(scratch), _lib.stream_handle()))
    return loss, dlogits


class DecodeCache:
    """Self-attention keys / values of incremental decoding, preallocated once per generate call: [layers, rows, Tmax, 2 d] (keys in the first
    d columns).  A step appends its L new positions in place at T; beam search reorders rows into a second buffer of the same shape with
    awt_op_kv_gather (`gather`) and swaps the two.

    `keep_queries(layers)` (token timestamps, generation.extract_token_timestamps): from then on every step also stores the cross-attention
    query rows of those decoder layers at their positions in `align_q` [len(layers), rows, Tmax, d].  That buffer is never reordered: a
    row of it is the batch row that ran the step, and beam search's `beam_indices` say which row that was for each returned token."""

    def __init__(self, layers: int, rows: int, Tmax: int, d: int, device, double: bool = False):
        self.layers, self.rows, self.Tmax, self.d, self.T = layers, rows, Tmax, d, 0
        self.buf = torch.empty((layers, rows, Tmax, 2 * d), dtype=torch.float32, device=device)
        self.spare = torch.empty_like(self.buf) if double else None
        self.align_q: Optional[torch.Tensor] = None
        self.align_slots: Dict[int, int] = {}

    def keep_queries(self, layers) -> None:
        self.align_slots = {int(l): s for s, l in enumerate(layers)}
        self.align_q = torch.zeros((len(self.align_slots), self.rows, self.Tmax, self.d), dtype=torch.float32, device=self.buf.device)

    def attend(self, i: int, qkv: torch.Tensor, L: int) -> torch.Tensor:
        d, T = self.d, self.T + L
        if T > self.Tmax:
            raise ValueError(f"decode cache holds {self.Tmax} positions, step needs {T}")
        self.buf[i, :, self.T:T].copy_(qkv.view(self.rows, L, 3 * d)[:, :, d:])
        return attention_cached((qkv, 0), 3 * d, self.buf[i], T, d // 64, L)

    def gather(self, parent: torch.Tensor, src: Optional["DecodeCache"] = None) -> None:
        """Row r of this cache <- row parent[r] (int32, on the device) of `src` (default: this cache itself, through the spare buffer)."""
        src_buf, src_rows = (self.buf, self.rows) if src is None else (src.buf, src.rows)
        dst = self.spare if src is None else self.buf
        T = self.T if src is None else src.T
        kv_gather(src_buf, dst, parent, self.layers, src_rows, self.rows, T, self.Tmax, 2 * self.d)
        if src is None:
            self.buf, self.spare = self.spare, self.buf
        else:
            self.T = src.T


def kv_gather(src: torch.Tensor, dst: torch.Tensor, parent: torch.Tensor, layers: int, src_rows: int, dst_rows: int, T: int, Tmax: int, width: int) -> None:
    """dst[l, r, :T] = src[l, parent[r], :T] over [layers, rows, Tmax, width] buffers (include/awt.h awt_op_kv_gather)."""
    parent = parent.to(torch.int32).contiguous()
    with torch.cuda.device(src.device):
        _lib.check(_lib.lib().awt_op_kv_gather(_ctx(src), _lib.ptr(src), _lib.ptr(dst), _lib.ptr(parent), layers, src_rows, dst_rows, T, Tmax, width,
                                               _lib.stream_handle()))


class _Leaf(nn.Module):
    pass


class NativeWhisperDecoder(nn.Module):
    """Pre-LN Whisper decoder with tied output projection on libawt.  HF parameter names.  The base parameters are frozen unless
    `train_base=True` (full-parameter fine-tuning): then every one of them requires grad -- the token table and the LEARNED
    position table included, as in HF -- and `loss` returns their gradients; no adapters in that mode."""

    LORA_TARGETS = ("q_proj", "v_proj")

    def __init__(self, d: int, layers: int, heads: int, ffn: int, vocab: int = 51865, max_target_positions: int = 448, precision: str = "bf16x3",
                 lora=None, lora_seed: int = 0, train_base: bool = False):
        super().__init__()
        if train_base and lora is not None:
            raise ValueError("train_base=True trains the decoder's base weights: pass lora=None")
        self.train_base = bool(train_base)
        if d != heads * 64:
            raise ValueError("the native attention kernels are specialised for head_dim 64 (every Whisper size)")
        self.d, self.n_layers, self.heads, self.ffn, self.vocab, self.precision = d, layers, heads, ffn, vocab, precision
        if lora is not None and not set(lora.targets) <= set(self.LORA_TARGETS):
            raise ValueError(f"decoder adapters are built for {self.LORA_TARGETS} of self_attn and encoder_attn, got {lora.targets}")
        self.lora = lora

        def P(*shape):
            return nn.Parameter(torch.zeros(*shape), requires_grad=self.train_base)

        self.embed_tokens = _Leaf(); self.embed_tokens.weight = P(vocab, d)
        self.embed_positions = _Leaf(); self.embed_positions.weight = P(max_target_positions, d)
        self.layers = nn.ModuleList()
        for _ in range(layers):
            lay = _Leaf()
            for att in ("self_attn", "encoder_attn"):
                a = _Leaf()
                for proj, has_bias in (("q_proj", True), ("k_proj", False), ("v_proj", True), ("out_proj", True)):
                    p = _Leaf(); p.weight = P(d, d)
                    if has_bias:
                        p.bias = P(d)
                    setattr(a, proj, p)
                setattr(lay, att, a)
                ln = _Leaf(); ln.weight = P(d); ln.bias = P(d)
                setattr(lay, att + "_layer_norm", ln)
            lay.fc1 = _Leaf(); lay.fc1.weight = P(ffn, d); lay.fc1.bias = P(ffn)
            lay.fc2 = _Leaf(); lay.fc2.weight = P(d, ffn); lay.fc2.bias = P(d)
            lay.final_layer_norm = _Leaf(); lay.final_layer_norm.weight = P(d); lay.final_layer_norm.bias = P(d)
            self.layers.append(lay)
        self.layer_norm = _Leaf(); self.layer_norm.weight = P(d); self.layer_norm.bias = P(d)
        if lora is not None:
            import math
            from .weights import unit_variates
            for i, lay in enumerate(self.layers):
                for att in ("self_attn", "encoder_attn"):
                    for proj in lora.targets:
                        leaf = getattr(getattr(lay, att), proj)
                        a = unit_variates(f"decoder.layers.{i}.{att}.{proj}.lora_A", lora.r * d, lora_seed) / math.sqrt(d)
                        leaf.lora_A = nn.Parameter(torch.from_numpy(a.astype("float32").reshape(lora.r, d)), requires_grad=True)
                        leaf.lora_B = nn.Parameter(torch.zeros(d, lora.r), requires_grad=True)          # B = 0: the adapter starts inert
        self._packed = PackedSet()
        self.cross_mode = os.environ.get("AWT_DECODER_CROSS", "auto")          # "auto" | "kv" | "absorbed" (A/B runs: tools, bench)
        if self.cross_mode not in ("auto", "kv", "absorbed"):
            raise ValueError("AWT_DECODER_CROSS must be auto, kv or absorbed")

    def absorbed_cross(self, L: int, S: int) -> bool:
        """Whether the training step's cross-attention takes the absorbed form (`cross_mode`: "auto" = by the row count H L, "kv", "absorbed")."""
        if self.cross_mode == "auto":
            return self.heads * L <= _AbsorbedCross.ROW_LIMIT and S % 4 == 0 and S <= 4096
        if self.cross_mode == "absorbed" and (S % 4 != 0 or S > 4096):
            raise ValueError("absorbed cross-attention needs a multiple of 4 and at most 4096 encoder positions")
        return self.cross_mode == "absorbed"

    # ------------------------------------------------------------------------------------------------ adapters
    def lora_parameters(self) -> List[nn.Parameter]:
        """Adapter parameters in a fixed order: per layer, self_attn then encoder_attn, per target: lora_A then lora_B."""
        out: List[nn.Parameter] = []
        if self.lora is not None:
            for lay in self.layers:
                for att in ("self_attn", "encoder_attn"):
                    for proj in self.lora.targets:
                        leaf = getattr(getattr(lay, att), proj)
                        out += [leaf.lora_A, leaf.lora_B]
        return out

    def base_parameters(self) -> List[nn.Parameter]:
        """Every base parameter, in `named_parameters()` order (what `train_base` trains)."""
        return [p for n, p in self.named_parameters() if "lora_" not in n]

    def _adapter(self, i: int, att: str, proj: str):
        if self.lora is None or proj not in self.lora.targets:
            return None
        leaf = getattr(getattr(self.layers[i], att), proj)
        return leaf.lora_A, leaf.lora_B

    def _lora_term(self, x: torch.Tensor, ab) -> Tuple[torch.Tensor, torch.Tensor]:
        """(u = x A^T [M, r], (alpha / r) u B^T [M, d]) on the native GEMM."""
        A, Bm = ab
        u = gemm(x, A.detach(), self.precision)
        return u, gemm(u, Bm.detach(), self.precision) * self.lora.scale

    def _cross_v_adapters(self, enc2d: torch.Tensor, kv: torch.Tensor):
        """Adds (alpha / r) (enc A_i^T) B_i^T to layer i's VALUE block of the fused cross-attention projection; returns u of all layers
        [B * S, layers * r] (one GEMM over the encoder states), or None without value adapters."""
        if self.lora is None or "v_proj" not in self.lora.targets:
            return None
        r, d, nl = self.lora.r, self.d, self.n_layers
        a_all = torch.cat([self.layers[i].encoder_attn.v_proj.lora_A.detach() for i in range(nl)], dim=0)        # [layers * r, d]
        u_all = gemm(enc2d, a_all, self.precision)
        blocks = kv.view(kv.shape[0], 2 * nl, d)
        for i in range(nl):
            blocks[:, 2 * i + 1] += gemm(u_all[:, i * r:(i + 1) * r], self.layers[i].encoder_attn.v_proj.lora_B.detach(), self.precision) * self.lora.scale
        return u_all

    # ------------------------------------------------------------------------------------------------ packing
    def load_state_dict(self, state_dict, strict: bool = True, **kw):
        res = super().load_state_dict(state_dict, strict=strict, **kw)
        self._packed.invalidate()
        return res

    def _apply(self, fn, *a, **kw):
        self._packed.invalidate()
        return super()._apply(fn, *a, **kw)

    def packed(self) -> Dict[str, object]:
        """The weights as `awt_weight` handles, brought up to date when a parameter changed (`PackedSet`; what an optimizer step of the train_base
        mode needs): per layer the fused self-attention q|k|v projection, the two output projections, the cross-attention query projection, fc1,
        fc2; the fused cross-attention k|v projection of ALL layers (one GEMM over the encoder output) and the tied vocabulary projection."""
        def plan():
            # the operands: a (weight, bias) pair becomes a PackedLinear, one [H, N, K] tensor the per-head B operands of _AbsorbedCross (a PackedBatch)
            H, d = self.heads, self.d
            zeros = torch.zeros(d, device=self.embed_tokens.weight.device)
            plan = []
            for i, lay in enumerate(self.layers):
                sa, ca = lay.self_attn, lay.encoder_attn
                where = ("layers", i)
                plan += [(where, "qkv", (sa.q_proj.weight, sa.k_proj.weight, sa.v_proj.weight, sa.q_proj.bias, sa.v_proj.bias),
                          lambda sa=sa: (torch.cat([sa.q_proj.weight, sa.k_proj.weight, sa.v_proj.weight]), torch.cat([sa.q_proj.bias, zeros, sa.v_proj.bias]))),
                         (where, "so", (sa.out_proj.weight, sa.out_proj.bias), lambda sa=sa: (sa.out_proj.weight, sa.out_proj.bias)),
                         (where, "cq", (ca.q_proj.weight, ca.q_proj.bias), lambda ca=ca: (ca.q_proj.weight, ca.q_proj.bias)),
                         (where, "co", (ca.out_proj.weight, ca.out_proj.bias), lambda ca=ca: (ca.out_proj.weight, ca.out_proj.bias)),
                         (where, "fc1", (lay.fc1.weight, lay.fc1.bias), lambda lay=lay: (lay.fc1.weight, lay.fc1.bias)),
                         (where, "fc2", (lay.fc2.weight, lay.fc2.bias), lambda lay=lay: (lay.fc2.weight, lay.fc2.bias))]
                where = ("cross_heads", i)                                             # per-head blocks of W_k / W_v as batched B operands
                plan += [(where, "k", (ca.k_proj.weight,), lambda ca=ca: (ca.k_proj.weight.detach().view(H, 64, d),)),
                         (where, "kT", (ca.k_proj.weight,), lambda ca=ca: (ca.k_proj.weight.detach().view(H, 64, d).transpose(1, 2),)),
                         (where, "v", (ca.v_proj.weight,), lambda ca=ca: (ca.v_proj.weight.detach().view(H, 64, d),)),
                         (where, "vT", (ca.v_proj.weight,), lambda ca=ca: (ca.v_proj.weight.detach().view(H, 64, d).transpose(1, 2),))]
            att = [l.encoder_attn for l in self.layers]
            plan += [((), "ckv", tuple(t for a in att for t in (a.k_proj.weight, a.v_proj.weight, a.v_proj.bias)),
                      lambda: (torch.cat([w for a in att for w in (a.k_proj.weight, a.v_proj.weight)]), torch.cat([b for a in att for b in (zeros, a.v_proj.bias)]))),
                     ((), "vocab", (self.embed_tokens.weight,), lambda: (self.embed_tokens.weight, None))]
            return {"layers": [{} for _ in self.layers], "cross_heads": [{} for _ in self.layers]}, plan

        return self._packed.refresh([p for n, p in self.named_parameters() if "lora_" not in n], plan, lambda w, *b: PackedLinear(w, *b, self.precision) if b else PackedBatch(w))

    # ------------------------------------------------------------------------------------------------ forward pieces
    def cross_kv(self, enc: torch.Tensor, precision: Optional[str] = None) -> torch.Tensor:
        """[B * S, 2 * layers * d]: cross-attention keys (even d-wide blocks) and values (odd blocks) of every layer."""
        B, S, d = enc.shape
        enc2d = enc.reshape(B * S, d).float().contiguous()
        kv = self.packed()["ckv"].forward(enc2d)
        self._cross_v_adapters(enc2d, kv)
        return kv

    def _embed(self, ids: torch.Tensor, position_offset: int) -> torch.Tensor:
        return embed(ids, self.embed_tokens.weight, self.embed_positions.weight, position_offset)

    def _run(self, ids: torch.Tensor, kv: torch.Tensor, S: int, save: Optional[list], caches=None, position_offset: int = 0,
             cross_group: int = 1) -> torch.Tensor:
        """Token ids [B, L] + cross keys / values (the `cross_kv` tensor, or an `_AbsorbedCross` over the encoder states) -> final-LayerNorm
        input x [B * L, d] (saving what the backward needs in `save`).  `caches`: a `DecodeCache` (generate) or per-layer dicts.
        cross_group: rows of ids per clip of `kv` (beam search: the beams of a clip attend to that clip's keys / values as its query rows)."""
        pk = self.packed()
        B, L = ids.shape
        d, H, nl = self.d, self.heads, self.n_layers
        if isinstance(caches, DecodeCache):
            position_offset = caches.T
        x = self._embed(ids, position_offset)
        for i, (lay, p) in enumerate(zip(self.layers, pk["layers"])):
            h = layernorm(x, lay.self_attn_layer_norm.weight, lay.self_attn_layer_norm.bias)
            qkv = p["qkv"].forward(h)                                                   # [B L, 3 d]
            us = {}
            for proj, col in (("q_proj", 0), ("v_proj", 2 * d)):                         # adapters on the self-attention query / value projections
                ab = self._adapter(i, "self_attn", proj)
                if ab is not None:
                    us[proj], delta = self._lora_term(h, ab)
                    qkv[:, col: col + d] += delta
            if caches is None:
                a, lse = attention_small((qkv, 0), 3 * d, (qkv, d), 3 * d, (qkv, 2 * d), 3 * d, B, H, L, L, True, 0, save is not None)
            elif isinstance(caches, DecodeCache):                                       # preallocated cache: append in place, attend over T positions
                a, lse = caches.attend(i, qkv, L), None
            else:                                                                       # incremental decoding: keys / values of all positions so far
                c = caches[i]
                kvn = qkv.view(B, L, 3 * d)[:, :, d:]
                c["kv"] = kvn.contiguous() if "kv" not in c else torch.cat([c["kv"], kvn], dim=1)
                T = c["kv"].shape[1]
                a, lse = attention_small((qkv, 0), 3 * d, (c["kv"], 0), 2 * d, (c["kv"], d), 2 * d, B, H, L, T, True, T - L, False)
            x1 = p["so"].forward(a, resid=x)
            h2 = layernorm(x1, lay.encoder_attn_layer_norm.weight, lay.encoder_attn_layer_norm.bias)
            q = p["cq"].forward(h2)
            ab = self._adapter(i, "encoder_attn", "q_proj")
            if ab is not None:
                us["cq"], delta = self._lora_term(h2, ab)
                q += delta
            if isinstance(caches, DecodeCache) and caches.align_q is not None and i in caches.align_slots:
                caches.align_q[caches.align_slots[i], :, caches.T: caches.T + L].copy_(q.view(B, L, d))
            if isinstance(kv, _AbsorbedCross):
                a2, lse2 = kv.attend(i, q, L)                                            # lse2: (q~, P, context) for the backward
            else:
                a2, lse2 = attention_small((q, 0), d, (kv, 2 * i * d), 2 * nl * d, (kv, (2 * i + 1) * d), 2 * nl * d, B // cross_group, H, L * cross_group, S,
                                           False, 0, save is not None)
            x2 = p["co"].forward(a2, resid=x1)
            h3 = layernorm(x2, lay.final_layer_norm.weight, lay.final_layer_norm.bias)
            f = p["fc1"].forward(h3)
            x3 = p["fc2"].forward(gelu(f), resid=x2)
            if save is not None:
                save.append((x, qkv, a, lse, x1, q, a2, lse2, x2, f, us))
            x = x3
        if isinstance(caches, DecodeCache):
            caches.T += L
        return x

    def forward(self, input_ids: torch.Tensor, encoder_hidden_states: torch.Tensor, native_precision: Optional[str] = None, cross=None, caches=None,
                position_offset: int = 0) -> torch.Tensor:
        """Logits [B, L, vocab] (no autograd graph: training goes through `loss`).  `cross`: the tensor `cross_kv` returned."""
        with torch.no_grad():
            B, L = input_ids.shape
            kv = cross if cross is not None else self.cross_kv(encoder_hidden_states)
            x = self._run(input_ids, kv, encoder_hidden_states.shape[1], None, caches, position_offset)
            xf = layernorm(x, self.layer_norm.weight, self.layer_norm.bias)
            logits = self.packed()["vocab"].forward(xf)
            return logits.view(B, L, -1)[:, :, : self.vocab]

    def decode_logits(self, ids: torch.Tensor, cross: torch.Tensor, S: int, cache: "DecodeCache", cross_group: int = 1) -> torch.Tensor:
        """One incremental decoding step for generate: ids [rows, L] at positions cache.T.. -> padded logits of the LAST position, a [rows, Np]
        view of the vocabulary projection's output (row pitch L * Np; columns >= vocab are padding)."""
        with torch.no_grad():
            rows, L = ids.shape
            x = self._run(ids, cross, S, None, cache, cross_group=cross_group)
            xf = layernorm(x, self.layer_norm.weight, self.layer_norm.bias)
            logits = self.packed()["vocab"].forward(xf)
            return logits.view(rows, L, -1)[:, L - 1]

    def loss(self, decoder_input_ids: torch.Tensor, labels: torch.Tensor, encoder_hidden_states: torch.Tensor):
        """(loss, logits [B, L, vocab]): differentiable w.r.t. `encoder_hidden_states` and the decoder's trainable parameters (its adapters, or
        with `train_base` every base parameter; none for the frozen decoder)."""
        holder: List[torch.Tensor] = []
        trained = self.base_parameters() if self.train_base else self.lora_parameters()
        loss = _DecoderLoss.apply(encoder_hidden_states, self, decoder_input_ids, labels, holder, *trained)
        return loss, holder[0]


class _DecoderLoss(torch.autograd.Function):
    """decoder + tied projection + cross-entropy as ONE autograd node with a hand-written native backward: d(loss) / d(encoder states) and,
    with decoder adapters, d(loss) / d(lora_A, lora_B) in `NativeWhisperDecoder.lora_parameters()` order, or in the `train_base` mode the
    gradient of every base parameter in `base_parameters()` order.  Each parameter gradient is formed where its dY is live in the backward
    (DESIGN §4.6b): weights on the weight-gradient GEMM (`ops.weight_grad`, fused operands read in place by column offset), biases as pitched
    column sums, LayerNorm affines by `awt_op_layernorm_param_grad`, the tied embedding as the projection's product plus `awt_op_embed_backward`."""

    @staticmethod
    def forward(ctx, enc, dec: NativeWhisperDecoder, ids, labels, holder, *adapters):
        B, S, d = enc.shape
        L = ids.shape[1]
        enc2d = enc.reshape(B * S, d).float().contiguous()
        if dec.absorbed_cross(L, S):
            kv, u_cv = _AbsorbedCross(dec, enc2d.view(B, S, d)), None
        else:
            kv = dec.packed()["ckv"].forward(enc2d)
            u_cv = dec._cross_v_adapters(enc2d, kv)
        save: list = []
        x = dec._run(ids, kv, S, save)
        xf = layernorm(x, dec.layer_norm.weight, dec.layer_norm.bias)
        logits = dec.packed()["vocab"].forward(xf)                                          # [B L, Np]
        loss, dlogits = cross_entropy(logits, labels, dec.vocab)
        holder.append(logits.view(B, L, -1)[:, :, : dec.vocab])
        ctx.dec, ctx.saved, ctx.kv, ctx.x_last, ctx.dlogits, ctx.shape = dec, save, kv, x, dlogits, (B, S, L)
        keep_enc = u_cv is not None or (dec.train_base and not isinstance(kv, _AbsorbedCross))     # the X of the value adapters' / the cross k | v weights' gradients
        ctx.enc2d, ctx.u_cv, ctx.n_adapters = (enc2d if keep_enc else None), u_cv, len(adapters)
        if dec.train_base:
            ctx.ids, ctx.xf = ids, xf                                                       # the embedding's backward and the tied projection's X
        return loss

    @staticmethod
    def backward(ctx, g):
        dec, save, kv, (B, S, L) = ctx.dec, ctx.saved, ctx.kv, ctx.shape
        pk = dec.packed()
        d, H, nl = dec.d, dec.heads, dec.n_layers
        prec = dec.precision
        scale = dec.lora.scale if dec.lora is not None else 0.0
        grads: Dict[int, torch.Tensor] = {}                                                 # id(parameter) -> gradient

        def adapter_backward(ab, x_in, u, dy):
            """Adapter (A, B) on input x_in with u = x_in A^T: records dA, dB and returns the adapter's share of d(x_in)."""
            A, Bm = ab
            du = gemm(dy, Bm.detach().t().contiguous(), prec)                               # [M, r] = dy B
            grads[id(A)] = gemm(du.t().contiguous(), x_in.t().contiguous(), prec) * scale   # dA [r, d] = (alpha / r) du^T x
            grads[id(Bm)] = gemm(dy.t().contiguous(), u.t().contiguous(), prec) * scale     # dB [d, r] = (alpha / r) dy^T u
            return gemm(du, A.detach().t().contiguous(), prec) * scale                      # [M, d] = (alpha / r) du A

        base = dec.train_base
        need_enc = ctx.needs_input_grad[0] or not base                                      # a frozen encoder under train_base: no d(encoder states)

        def wgrad(dy, x, **kw):                                                             # dW [n, k] = dy[:, ycol: ycol + n]^T x[:, xcol: xcol + k]
            return ops.weight_grad(dy, x, precision=prec, **kw)

        def linear_grads(leaf, dy, x):
            """Records d(weight) = dy^T x and d(bias) = column sums of dy of one nn.Linear."""
            n = leaf.weight.shape[0]
            grads[id(leaf.weight)] = wgrad(dy, x, n=n)
            grads[id(leaf.bias)] = column_sums_ld(dy, 0, n)

        def norm_grads(leaf, dy, x):
            grads[id(leaf.weight)], grads[id(leaf.bias)] = layernorm_param_grad(dy, x)

        dlogits = ctx.dlogits * g                                                           # upstream scalar (1 / micro-batches, ...)
        dxf = pk["vocab"].backward_input(dlogits)
        if base:
            norm_grads(dec.layer_norm, dxf, ctx.x_last)
            # the tied table, projection side: dlogits^T LN(x_last) over the padded vocabulary [Np, d] (the padding columns of dlogits are zero);
            # the parameter's gradient is its first `vocab` rows, and the lookup side is added to them after the last layer
            d_tok = wgrad(dlogits, ctx.xf)
        dx = layernorm_backward(dxf, ctx.x_last, dec.layer_norm.weight)
        del dxf
        absorbed = isinstance(kv, _AbsorbedCross)
        if absorbed:
            d_enc = torch.zeros((B, S, d), dtype=torch.float32, device=dx.device) if need_enc else None     # every layer adds its share (one batched GEMM each)
        else:
            dkv = torch.empty_like(kv)                                                      # every layer writes its own two d-wide blocks
        for i in range(nl - 1, -1, -1):
            lay, p = dec.layers[i], pk["layers"][i]
            x0, qkv, a, lse, x1, q, a2, lse2, x2, f, us = save[i]
            # MLP: x3 = x2 + fc2(gelu(fc1(LN3(x2))))
            df = gelu_backward(f, p["fc2"].backward_input(dx))
            dh3 = p["fc1"].backward_input(df)
            if base:                                                                        # LayerNorm outputs and gelu(f) are recomputed: B x L rows
                linear_grads(lay.fc2, dx, gelu(f))
                linear_grads(lay.fc1, df, layernorm(x2, lay.final_layer_norm.weight, lay.final_layer_norm.bias))
                norm_grads(lay.final_layer_norm, dh3, x2)
            dx = layernorm_backward(dh3, x2, lay.final_layer_norm.weight, dres=dx)
            del dh3
            # cross-attention: x2 = x1 + out(attn(q(LN2(x1)), K_i, V_i))
            if base:
                linear_grads(lay.encoder_attn.out_proj, dx, a2)
            da2 = p["co"].backward_input(dx)
            if absorbed:
                dq = kv.backward(i, lse2, da2, d_enc, L, grads, q if base else None)
            else:
                dq = torch.empty_like(q)
                attention_small_backward((q, 0), d, (kv, 2 * i * d), 2 * nl * d, (kv, (2 * i + 1) * d), 2 * nl * d, a2, da2, lse2,
                                         (dq, 0), (dkv, 2 * i * d), (dkv, (2 * i + 1) * d), B, H, L, S, False, 0)
            dh2 = p["cq"].backward_input(dq)
            if base:
                linear_grads(lay.encoder_attn.q_proj, dq, layernorm(x1, lay.encoder_attn_layer_norm.weight, lay.encoder_attn_layer_norm.bias))
                norm_grads(lay.encoder_attn_layer_norm, dh2, x1)
            ab = dec._adapter(i, "encoder_attn", "q_proj")
            if ab is not None:
                h2 = layernorm(x1, lay.encoder_attn_layer_norm.weight, lay.encoder_attn_layer_norm.bias)      # recomputed: B x L rows
                dh2 = dh2 + adapter_backward(ab, h2, us["cq"], dq)
            dx = layernorm_backward(dh2, x1, lay.encoder_attn_layer_norm.weight, dres=dx)
            # self-attention: x1 = x0 + out(attn(qkv(LN1(x0))))
            if base:
                linear_grads(lay.self_attn.out_proj, dx, a)
            da = p["so"].backward_input(dx)
            dqkv = torch.empty_like(qkv)
            attention_small_backward((qkv, 0), 3 * d, (qkv, d), 3 * d, (qkv, 2 * d), 3 * d, a, da, lse,
                                     (dqkv, 0), (dqkv, d), (dqkv, 2 * d), B, H, L, L, True, 0)
            dh = p["qkv"].backward_input(dqkv)
            if base:                                                                        # q | k | v: ONE [3 d, d] product, its row blocks are the three gradients
                sa = lay.self_attn
                dw = wgrad(dqkv, layernorm(x0, lay.self_attn_layer_norm.weight, lay.self_attn_layer_norm.bias))
                grads[id(sa.q_proj.weight)], grads[id(sa.k_proj.weight)], grads[id(sa.v_proj.weight)] = dw[:d], dw[d: 2 * d], dw[2 * d:]
                grads[id(sa.q_proj.bias)], grads[id(sa.v_proj.bias)] = column_sums_ld(dqkv, 0, d), column_sums_ld(dqkv, 2 * d, d)
                norm_grads(lay.self_attn_layer_norm, dh, x0)
            if us:
                h = None
                for proj, col in (("q_proj", 0), ("v_proj", 2 * d)):
                    ab = dec._adapter(i, "self_attn", proj)
                    if ab is not None:
                        if h is None:
                            h = layernorm(x0, lay.self_attn_layer_norm.weight, lay.self_attn_layer_norm.bias)
                        dh = dh + adapter_backward(ab, h, us[proj], dqkv[:, col: col + d].contiguous())
            dx = layernorm_backward(dh, x0, lay.self_attn_layer_norm.weight, dres=dx)
        ctx.saved = ctx.kv = ctx.dlogits = None
        if base:                                                                            # the lookup side of the tied table, and the position rows
            d_pos = torch.zeros_like(dec.embed_positions.weight)
            embed_backward(ctx.ids, dx, d_tok[: dec.vocab], d_pos)
            grads[id(dec.embed_tokens.weight)], grads[id(dec.embed_positions.weight)] = d_tok[: dec.vocab], d_pos
            if not absorbed:                                                                # all layers' cross k / v weights: ONE product dkv^T enc
                dw = wgrad(dkv, ctx.enc2d)
                for i, lay in enumerate(dec.layers):
                    ca = lay.encoder_attn
                    grads[id(ca.k_proj.weight)], grads[id(ca.v_proj.weight)] = dw[2 * i * d: (2 * i + 1) * d], dw[(2 * i + 1) * d: (2 * i + 2) * d]
                    grads[id(ca.v_proj.bias)] = column_sums_ld(dkv, (2 * i + 1) * d, d)
                ctx.enc2d = None
            ctx.ids = ctx.xf = None
        if not absorbed:
            d_enc = pk["ckv"].backward_input(dkv) if need_enc else None                     # [B S, d]
        if ctx.u_cv is not None:
            # cross-attention value adapters: dV_i = dkv block 2 i + 1 (B x S rows); their share of d(encoder states) is ONE GEMM over all layers
            r = dec.lora.r
            dv = dkv.view(dkv.shape[0], 2 * nl, d)
            du_all = torch.empty_like(ctx.u_cv)
            enc_t = ctx.enc2d.t().contiguous()
            for i in range(nl):
                A, Bm = dec._adapter(i, "encoder_attn", "v_proj")
                dvi = dv[:, 2 * i + 1].contiguous()
                du = gemm(dvi, Bm.detach().t().contiguous(), prec)
                du_all[:, i * r:(i + 1) * r] = du
                grads[id(Bm)] = gemm(dvi.t().contiguous(), ctx.u_cv[:, i * r:(i + 1) * r].t().contiguous(), prec) * scale
                grads[id(A)] = gemm(du.t().contiguous(), enc_t, prec) * scale
            a_all_t = torch.cat([dec._adapter(i, "encoder_attn", "v_proj")[0].detach() for i in range(nl)], dim=0).t().contiguous()   # [d, layers * r]
            d_enc = d_enc + gemm(du_all, a_all_t, prec) * scale
            ctx.enc2d = ctx.u_cv = None
        params = (dec.base_parameters() if base else dec.lora_parameters()) if ctx.n_adapters else []
        return (d_enc.view(B, S, d) if d_enc is not None else None, None, None, None, None, *[grads.get(id(p)) for p in params])
