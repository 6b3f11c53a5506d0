"""Single-operator entry points of libawt (what the encoder is built from), as torch functions on device tensors.
Used by the per-kernel parity tests; each raises if the library or the GPU is missing."""
from __future__ import annotations

import ctypes
from typing import Optional

import torch

from . import _lib

_TERMS = {"bf16": 1, "fp16": 2, "bf16x3": 3, "fp16x3": 4, "f16f8": 5}   # common.h PREC_*


def _terms(precision: str) -> int:
    if precision not in _TERMS:
        raise ValueError(f"unknown precision {precision!r}: one of {', '.join(_TERMS)}")
    return _TERMS[precision]


def pad_to(n: int, multiple: int) -> int:
    """n rounded up to a multiple (the GEMM's K step of 64 and N tile of 128, the weight-gradient GEMM's widths of 8)."""
    return (n + multiple - 1) // multiple * multiple


def linear(x: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor] = None, precision: str = "bf16x3") -> torch.Tensor:
    """y = x w^T + bias on the MFMA GEMM kernel; x [M, K], w [N, K] fp32 device tensors, N % 128 == 0, K % 64 == 0."""
    terms = _terms(precision)
    x, w = x.float().contiguous(), w.float().contiguous()
    M, K = x.shape
    N = w.shape[0]
    L = _lib.lib()
    y = torch.empty((M, N), dtype=torch.float32, device=x.device)
    ws = _lib.workspace(L.awt_op_linear_workspace_bytes(M, N, K), x.device)
    b = bias.float().contiguous() if bias is not None else None
    with torch.cuda.device(x.device):
        _lib.check(L.awt_op_linear(_lib.ctx(x.device), _lib.ptr(x), _lib.ptr(w), _lib.ptr(b), _lib.ptr(y), M, N, K,
                                   terms, _lib.ptr(ws), ws.numel(), _lib.stream_handle()))
    return y


# GemmEpilogue of csrc/common.h
EPILOGUES = {"f32": 0, "f32_resid": 1, "planes": 2, "gelu": 3, "qkv": 4, "gelu_pos": 5, "gelu_save": 6, "dgelu": 7}


def linear_fused_workspace_bytes(x_rows: int, ldx: int, N: int, ldw: int) -> int:
    """Workspace of `linear_fused`; answers without a GPU."""
    return int(_lib.lib().awt_op_linear_fused_workspace_bytes(int(x_rows), int(ldx), int(N), int(ldw)))


def linear_fused(x: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor], epi, precision, out: dict, M: Optional[int] = None, segs=None, *,
                 resid: Optional[torch.Tensor] = None, pos: Optional[torch.Tensor] = None, rows_pos: int = 0, pre: tuple = (None, None), scale: float = 1.0,
                 S: int = 0, H: int = 0, skip_v8: bool = False, n_valid: int = 0, m_pick: int = 0, split_lines: bool = False, ldo: int = 0,
                 workspace: Optional[torch.Tensor] = None, ws_bytes: Optional[int] = None) -> None:
    """One GEMM launch with a fused epilogue (include/awt.h: awt_op_linear_fused); the kernel's raw bytes land in the caller's tensors `out`, a dict over
    "f32", "hi", "lo", "hi8", "lo8", "ilv", "hi2", "lo2" (any dtype; nothing is converted).  x [x_rows, ldx], w [N, ldw] fp32; segs: up to three
    (xcol, wcol, k, rows_out, rows_in, row_mul, row_add), default one plain segment over all of x; epi: a name of EPILOGUES or its number; precision: a name
    or the operator's `terms`; pre: the (hi, lo) bf16 planes "dgelu" reads.  Raises _lib.AwtError where the library refuses the call."""
    terms = precision if isinstance(precision, int) else _terms(precision)
    x_rows, ldx = x.shape
    N, ldw = w.shape
    M = x_rows if M is None else M
    segs = [(0, 0, ldx, M, M, 1, 0)] if segs is None else list(segs)
    a = _lib.LinearFusedArgs()
    a.M, a.N, a.terms, a.epi, a.nseg = M, N, terms, EPILOGUES.get(epi, epi), len(segs)
    a.x_rows, a.ldx, a.ldw = x_rows, ldx, ldw
    for i, sg in enumerate(segs[:3]):
        for name, value in zip(("seg_xcol", "seg_wcol", "seg_k", "seg_rows_out", "seg_rows_in", "seg_row_mul", "seg_row_add"), sg):
            getattr(a, name)[i] = int(value)
    a.rows_pos, a.S, a.H, a.skip_v8, a.n_valid, a.m_pick, a.split_lines, a.ldo = rows_pos, S, H, int(skip_v8), n_valid, m_pick, int(split_lines), ldo
    a.scale = float(scale)
    a.x, a.w, a.bias, a.resid, a.pos, a.pre_hi, a.pre_lo = (_lib.ptr(t) for t in (x, w, bias, resid, pos, pre[0], pre[1]))
    for key in ("f32", "hi", "lo", "hi8", "lo8", "ilv", "hi2", "lo2"):
        setattr(a, "out_" + key, _lib.ptr(out.get(key)))
    L = _lib.lib()
    ws = _lib.workspace(L.awt_op_linear_fused_workspace_bytes(x_rows, ldx, N, ldw), x.device) if workspace is None else workspace
    with torch.cuda.device(x.device):
        _lib.check(L.awt_op_linear_fused(_lib.ctx(x.device), ctypes.byref(a), _lib.ptr(ws), ws.numel() if ws_bytes is None else int(ws_bytes), _lib.stream_handle()))


def layernorm(x: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, eps: float = 1e-5) -> torch.Tensor:
    x = x.float().contiguous()
    M, d = x.shape
    y = torch.empty_like(x)
    with torch.cuda.device(x.device):
        _lib.check(_lib.lib().awt_op_layernorm(_lib.ctx(x.device), _lib.ptr(x), _lib.ptr(gamma.float().contiguous()),
                                               _lib.ptr(beta.float().contiguous()), _lib.ptr(y), M, d, eps, _lib.stream_handle()))
    return y


def attention(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, precision: str = "bf16x3") -> torch.Tensor:
    """softmax(q k^T) v for q (pre-scaled), k, v: [B, H, S, 64] fp32 -> [B, S, H * 64] fp32."""
    terms = _terms(precision)
    q, k, v = (t.float().contiguous() for t in (q, k, v))
    B, H, S, hd = q.shape
    if hd != 64:
        raise ValueError("head_dim must be 64")
    L = _lib.lib()
    o = torch.empty((B, S, H * 64), dtype=torch.float32, device=q.device)
    ws = _lib.workspace(L.awt_op_attention_workspace_bytes(B, H, S), q.device)
    with torch.cuda.device(q.device):
        _lib.check(L.awt_op_attention(_lib.ctx(q.device), _lib.ptr(q), _lib.ptr(k), _lib.ptr(v), _lib.ptr(o), B, H, S,
                                      terms, _lib.ptr(ws), ws.numel(), _lib.stream_handle()))
    return o


def attention_ex_workspace_bytes(B: int, H: int, S: int) -> int:
    """Workspace of `attention_ex`; answers without a GPU."""
    return int(_lib.lib().awt_op_attention_ex_workspace_bytes(int(B), int(H), int(S)))


def attention_ex(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, precision, out: dict, workspace: Optional[torch.Tensor] = None,
                 ws_bytes: Optional[int] = None) -> None:
    """One attention forward launch with any of its output forms (include/awt.h: awt_op_attention_ex); the kernel's raw bytes land in the caller's tensors
    `out`, a dict over "f32", "hi", "lo", "hi8", "lo8", "ilv", "lse2" (any dtype; nothing is converted).  q (pre-scaled), k, v: [B, H, S, 64] fp32;
    precision: a name or the operator's `terms`.  Raises _lib.AwtError where the library refuses the call."""
    terms = precision if isinstance(precision, int) else _terms(precision)
    q, k, v = (t.float().contiguous() for t in (q, k, v))
    B, H, S, hd = q.shape
    if hd != 64 or k.shape != q.shape or v.shape != q.shape:
        raise ValueError("attention_ex: q, k, v must share the shape [B, H, S, 64]")
    unknown = set(out) - {"f32", "hi", "lo", "hi8", "lo8", "ilv", "lse2"}
    if unknown:
        raise KeyError(f"attention_ex: no output named {sorted(unknown)}")
    L = _lib.lib()
    ws = _lib.workspace(L.awt_op_attention_ex_workspace_bytes(B, H, S), q.device) if workspace is None else workspace
    with torch.cuda.device(q.device):
        _lib.check(L.awt_op_attention_ex(_lib.ctx(q.device), _lib.ptr(q), _lib.ptr(k), _lib.ptr(v), *(_lib.ptr(out.get(key)) for key in ("f32", "hi", "lo", "hi8", "lo8", "ilv", "lse2")),
                                         B, H, S, terms, _lib.ptr(ws), ws.numel() if ws_bytes is None else int(ws_bytes), _lib.stream_handle()))


def attention_backward_planes(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, d_o: torch.Tensor, precision: str = "bf16x3",
                              grad_precision: Optional[str] = None, qscale: float = 1.0, out: Optional[tuple] = None) -> tuple:
    """The attention of an encoder layer's training pass (include/awt.h: awt_op_attention_backward) with its outputs as the library writes them:
    (o_hi, o_lo, lse2, delta, g_hi, g_lo) -- o planes bf16 [B * S, H * 64], lse2 / delta fp32 [B, H, S], gradient planes bf16 [B * S, 3 * H * 64]
    (dq | dk | dv per row).  precision "bf16": the lo planes are None.  `out`: the same six tensors allocated by the caller (written in place)."""
    terms = _terms(precision)
    grad_terms = terms if grad_precision is None else _terms(grad_precision)
    q, k, v, d_o = (t.float().contiguous() for t in (q, k, v, d_o))
    B, H, S, hd = q.shape
    if hd != 64:
        raise ValueError("head_dim must be 64")
    if k.shape != q.shape or v.shape != q.shape or d_o.shape != (B, S, H * 64):
        raise ValueError("attention_backward: k, v must have q's shape [B, H, S, 64] and d_o must be [B, S, H * 64]")
    L = _lib.lib()
    if out is None:
        plane = lambda w: torch.empty((B * S, w), dtype=torch.bfloat16, device=q.device)
        stat = lambda: torch.empty((B, H, S), dtype=torch.float32, device=q.device)
        lo = terms != 1
        out = (plane(H * 64), plane(H * 64) if lo else None, stat(), stat(), plane(3 * H * 64), plane(3 * H * 64) if lo else None)
    o_hi, o_lo, lse2, delta, g_hi, g_lo = out
    ws = _lib.workspace(L.awt_op_attention_backward_workspace_bytes(B, H, S), q.device)
    with torch.cuda.device(q.device):
        _lib.check(L.awt_op_attention_backward(_lib.ctx(q.device), _lib.ptr(q), _lib.ptr(k), _lib.ptr(v), _lib.ptr(d_o), _lib.ptr(o_hi), _lib.ptr(o_lo),
                                               _lib.ptr(lse2), _lib.ptr(delta), _lib.ptr(g_hi), _lib.ptr(g_lo), B, H, S, float(qscale), terms, grad_terms,
                                               _lib.ptr(ws), ws.numel(), _lib.stream_handle()))
    return out


def attention_backward_join(planes: tuple, B: int, H: int, S: int) -> tuple:
    """(o [B, S, H * 64], lse2, delta [B, H, S], dq, dk, dv [B, H, S, 64]) in float64 from the six tensors of attention_backward_planes: a value is hi + lo."""
    o_hi, o_lo, lse2, delta, g_hi, g_lo = planes
    join = lambda hi, lo: hi.double() if lo is None else hi.double() + lo.double()
    g = join(g_hi, g_lo).view(B, S, 3, H, 64).permute(2, 0, 3, 1, 4)
    return join(o_hi, o_lo).view(B, S, H * 64), lse2.double(), delta.double(), g[0].contiguous(), g[1].contiguous(), g[2].contiguous()


def attention_backward(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, d_o: torch.Tensor, precision: str = "bf16x3",
                       grad_precision: Optional[str] = None, qscale: float = 1.0) -> tuple:
    """(o, lse2, delta, dq, dk, dv) of softmax(q k^T) v under the upstream gradient d_o, as the encoder's training pass computes them: q (pre-scaled),
    k, v [B, H, S, 64], d_o [B, S, H * 64].  o is [B, S, H * 64], lse2 (log2 units) and delta = rowsum(d_o * o) are [B, H, S], dq (times qscale), dk, dv are
    [B, H, S, 64]; all float64, the plane pairs joined.  precision "bf16" or "bf16x3"; grad_precision "bf16" with "bf16x3" is the bf16-gradient option."""
    B, H, S, _ = q.shape
    return attention_backward_join(attention_backward_planes(q, k, v, d_o, precision, grad_precision, qscale), B, H, S)


def weight_grad(dy: torch.Tensor, x: torch.Tensor, n: Optional[int] = None, k: Optional[int] = None, ycol: int = 0, xcol: int = 0,
                precision: str = "bf16x3", scale: float = 1.0, out: Optional[torch.Tensor] = None, accumulate: bool = False,
                row_map: Optional[tuple] = None) -> torch.Tensor:
    """dW[n, k] = scale * sum_m dy[m, ycol + n] x[row(m), xcol + k] on the MFMA weight-gradient GEMM (include/awt.h: awt_op_weight_grad).
    dy [M, ldy], x [rows, ldx] fp32 device tensors; n / k default to the full widths.  row_map = (rows_out, rows_in, row_mul, row_add): the
    conv-stem row map (rows outside [0, rows_in) of their group read as zero).  `out` [n, k] (any strides) is written, or added to with `accumulate`."""
    if precision not in ("bf16", "bf16x3"):
        raise ValueError("weight_grad: precision must be 'bf16' or 'bf16x3'")
    dy, x = dy.float().contiguous(), x.float().contiguous()
    M, ldy = dy.shape
    rows_x, ldx = x.shape
    n = ldy - ycol if n is None else n
    k = ldx - xcol if k is None else k
    if out is None:
        if accumulate:
            raise ValueError("weight_grad: accumulate needs out")
        out = torch.empty((n, k), dtype=torch.float32, device=dy.device)
    if out.shape != (n, k) or out.dtype != torch.float32 or out.device != dy.device:
        raise ValueError(f"weight_grad: out must be a float32 [{n}, {k}] tensor on {dy.device}")
    ro, ri, rm, ra = row_map if row_map is not None else (0, 0, 1, 0)
    L = _lib.lib()
    ws = _lib.workspace(L.awt_op_weight_grad_workspace_bytes(M, rows_x, ldy, ldx, n, k), dy.device)
    with torch.cuda.device(dy.device):
        _lib.check(L.awt_op_weight_grad(_lib.ctx(dy.device), _lib.ptr(dy), ldy, ycol, n, _lib.ptr(x), rows_x, ldx, xcol, k, M, ro, ri, rm, ra,
                                        1 if precision == "bf16" else 3, float(scale), int(accumulate), out.data_ptr(), out.stride(0), out.stride(1),
                                        _lib.ptr(ws), ws.numel(), _lib.stream_handle()))
    return out


def _at(pair) -> int:
    """Device address of element `col` of a (tensor, column offset) pair over a row-major fp32 matrix."""
    t, col = pair
    if t.dtype != torch.float32:
        raise ValueError("libawt's pitched operators take float32 tensors")
    return _lib.ptr(t) + 4 * int(col)


def cross_attention_workspace_bytes(B: int, H: int, Lq: int, Sk: int, backward: bool = False) -> int:
    """Workspace of `cross_attention` / `cross_attention_backward`; answers without a GPU."""
    return int(_lib.lib().awt_op_cross_attention_workspace_bytes(int(B), int(H), int(Lq), int(Sk), int(backward)))


def cross_attention(q, ldq: int, k, ldk: int, v, ldv: int, B: int, H: int, Lq: int, Sk: int, precision="bf16x3", want_lse: bool = True,
                    o=None, ldo: Optional[int] = None, lse: Optional[torch.Tensor] = None, workspace: Optional[torch.Tensor] = None):
    """softmax(128^-1/2 q k^T) v for head_dim 128, no mask (include/awt.h: awt_op_cross_attention).  q / k / v (and o, when given with its pitch ldo): (tensor,
    column offset) pairs over row-major fp32 matrices, row (b, i) of q at pitch ldq, row (b, j) of k / v at ldk / ldv, head h in columns 128 h ...  Returns
    (o [B * Lq, H * 128] unless given, lse [B, H, Lq] or None).  precision: "bf16x3", "bf16", or the operator's `terms` as an int."""
    terms = precision if isinstance(precision, int) else _terms(precision)
    dev = q[0].device
    if o is None:
        o, ldo = (torch.empty((B * Lq, H * 128), dtype=torch.float32, device=dev), 0), H * 128
    if lse is None and want_lse:
        lse = torch.empty((B, H, Lq), dtype=torch.float32, device=dev)
    L = _lib.lib()
    ws = _lib.workspace(L.awt_op_cross_attention_workspace_bytes(B, H, Lq, Sk, 0), dev) if workspace is None else workspace
    with torch.cuda.device(dev):
        _lib.check(L.awt_op_cross_attention(_lib.ctx(dev), _at(q), int(ldq), _at(k), int(ldk), _at(v), int(ldv), _at(o), int(ldo), _lib.ptr(lse), B, H, Lq, Sk,
                                            int(terms), _lib.ptr(ws), ws.numel(), _lib.stream_handle()))
    return o[0], lse


def cross_attention_backward(q, ldq: int, k, ldk: int, v, ldv: int, o, dout, ldo: int, lse: torch.Tensor, dq, dk, dv, B: int, H: int, Lq: int, Sk: int,
                             precision="bf16x3", workspace: Optional[torch.Tensor] = None) -> None:
    """Writes dq / dk / dv at (tensor, column offset) destinations laid out like q / k / v (include/awt.h: awt_op_cross_attention_backward); o and dout are
    (tensor, column offset) pairs at pitch ldo, lse the forward's [B, H, Lq]."""
    terms = precision if isinstance(precision, int) else _terms(precision)
    dev = q[0].device
    L = _lib.lib()
    ws = _lib.workspace(L.awt_op_cross_attention_workspace_bytes(B, H, Lq, Sk, 1), dev) if workspace is None else workspace
    with torch.cuda.device(dev):
        _lib.check(L.awt_op_cross_attention_backward(_lib.ctx(dev), _at(q), int(ldq), _at(k), int(ldk), _at(v), int(ldv), _at(o), _at(dout), int(ldo),
                                                     _lib.ptr(lse), _at(dq), _at(dk), _at(dv), B, H, Lq, Sk, int(terms), _lib.ptr(ws), ws.numel(),
                                                     _lib.stream_handle()))


# ---- the operators of a Qwen3 decoder layer (include/awt.h; csrc/qwen_ops.hip and the causal variant of csrc/cross_attention.hip)
def rmsnorm(x, ldx: int, gamma: torch.Tensor, M: int, d: int, eps: float, y=None, ldy: Optional[int] = None):
    """y[m, :] = gamma * x[m, :] * rsqrt(mean(x[m, :]^2) + eps) (awt_op_rmsnorm).  x (and y, when given with its pitch ldy): (tensor, element offset) pairs over
    row-major fp32 matrices of pitch ldx / ldy.  Returns y's tensor ([M, d] unless given)."""
    dev = x[0].device
    if y is None:
        y, ldy = (torch.empty((M, d), dtype=torch.float32, device=dev), 0), d
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().awt_op_rmsnorm(_lib.ctx(dev), _at(x), int(ldx), _at((gamma, 0)), _at(y), int(ldy), int(M), int(d), float(eps), _lib.stream_handle()))
    return y[0]


def qk_norm_rope(qkv, ld: int, q_gamma: torch.Tensor, k_gamma: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor, positions: torch.Tensor, q_out, ldq: int,
                 k_cache, v_cache, ldkv: int, kv_batch_stride: int, B: int, Lq: int, Hq: int, Hkv: int, eps: float) -> None:
    """Per-head RMSNorm of q and k, rotary embedding, q to q_out, k and v into the decode cache at positions[r] (awt_op_qk_norm_rope).  qkv, q_out, k_cache,
    v_cache: (tensor, element offset) pairs; cos / sin fp32 [rows, 64]; positions int32 [B * Lq] on the device."""
    dev = qkv[0].device
    if positions.dtype != torch.int32 or positions.numel() != B * Lq or not positions.is_contiguous():
        raise ValueError("qk_norm_rope: positions must be a contiguous int32 tensor of B * Lq elements")
    if cos.dtype != torch.float32 or sin.dtype != torch.float32 or cos.shape != sin.shape or cos.dim() != 2 or cos.shape[1] != 64:
        raise ValueError("qk_norm_rope: cos and sin must be float32 [rows, 64]")
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().awt_op_qk_norm_rope(_lib.ctx(dev), _at(qkv), int(ld), _at((q_gamma, 0)), _at((k_gamma, 0)), _at((cos, 0)), _at((sin, 0)),
                                                  _lib.ptr(positions), _at(q_out), int(ldq), _at(k_cache), _at(v_cache), int(ldkv), int(kv_batch_stride),
                                                  int(B), int(Lq), int(Hq), int(Hkv), float(eps), _lib.stream_handle()))


def causal_attention_workspace_bytes(B: int, Hq: int, Lq: int, T: int) -> int:
    """Workspace of `causal_attention`; answers without a GPU."""
    return int(_lib.lib().awt_op_causal_attention_workspace_bytes(int(B), int(Hq), int(Lq), int(T)))


def causal_attention(q, ldq: int, k, v, ldkv: int, kv_batch_stride: int, B: int, Hq: int, Hkv: int, Lq: int, T: int, precision="bf16x3", o=None,
                     ldo: Optional[int] = None, workspace: Optional[torch.Tensor] = None):
    """Causal attention of Lq new query rows per batch over T live positions of a decode cache, head_dim 128, grouped KV heads (awt_op_causal_attention).
    q / k / v (and o, when given with its pitch ldo): (tensor, element offset) pairs.  Returns o's tensor ([B * Lq, Hq * 128] unless given)."""
    terms = precision if isinstance(precision, int) else _terms(precision)
    dev = q[0].device
    if o is None:
        o, ldo = (torch.empty((B * Lq, Hq * 128), dtype=torch.float32, device=dev), 0), Hq * 128
    L = _lib.lib()
    ws = _lib.workspace(L.awt_op_causal_attention_workspace_bytes(B, Hq, Lq, T), dev) if workspace is None else workspace
    with torch.cuda.device(dev):
        _lib.check(L.awt_op_causal_attention(_lib.ctx(dev), _at(q), int(ldq), _at(k), _at(v), int(ldkv), int(kv_batch_stride), _at(o), int(ldo), int(B), int(Hq),
                                             int(Hkv), int(Lq), int(T), int(terms), _lib.ptr(ws), ws.numel(), _lib.stream_handle()))
    return o[0]


def silu_mul(gu, ld: int, M: int, I: int, y=None, ldy: Optional[int] = None):
    """y[m, i] = silu(gu[m, i]) * gu[m, I + i] (awt_op_silu_mul).  gu (and y, when given with its pitch ldy): (tensor, element offset) pairs.  Returns y's
    tensor ([M, I] unless given)."""
    dev = gu[0].device
    if y is None:
        y, ldy = (torch.empty((M, I), dtype=torch.float32, device=dev), 0), I
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().awt_op_silu_mul(_lib.ctx(dev), _at(gu), int(ld), _at(y), int(ldy), int(M), int(I), _lib.stream_handle()))
    return y[0]


# ---- their backward (include/awt.h): what music2midi.Qwen3Decoder's training pass is chained from
def causal_attention_lse(q, ldq: int, k, v, ldkv: int, kv_batch_stride: int, B: int, Hq: int, Hkv: int, Lq: int, T: int, precision="bf16x3", o=None,
                         ldo: Optional[int] = None, lse: Optional[torch.Tensor] = None, workspace: Optional[torch.Tensor] = None):
    """`causal_attention` that also writes the log-sum-exp (awt_op_causal_attention_lse).  Returns (o's tensor, lse [B, Hq, Lq])."""
    terms = precision if isinstance(precision, int) else _terms(precision)
    dev = q[0].device
    if o is None:
        o, ldo = (torch.empty((B * Lq, Hq * 128), dtype=torch.float32, device=dev), 0), Hq * 128
    if lse is None:
        lse = torch.empty((B, Hq, Lq), dtype=torch.float32, device=dev)
    L = _lib.lib()
    ws = _lib.workspace(L.awt_op_causal_attention_workspace_bytes(B, Hq, Lq, T), dev) if workspace is None else workspace
    with torch.cuda.device(dev):
        _lib.check(L.awt_op_causal_attention_lse(_lib.ctx(dev), _at(q), int(ldq), _at(k), _at(v), int(ldkv), int(kv_batch_stride), _at(o), int(ldo), _lib.ptr(lse),
                                                 int(B), int(Hq), int(Hkv), int(Lq), int(T), int(terms), _lib.ptr(ws), ws.numel(), _lib.stream_handle()))
    return o[0], lse


def causal_attention_backward_workspace_bytes(B: int, Hq: int, Lq: int, T: int) -> int:
    """Workspace of `causal_attention_backward`; answers without a GPU."""
    return int(_lib.lib().awt_op_causal_attention_backward_workspace_bytes(int(B), int(Hq), int(Lq), int(T)))


def causal_attention_backward(q, ldq: int, k, v, ldkv: int, kv_batch_stride: int, o, dout, ldo: int, lse: torch.Tensor, dq, dk, dv, lddkv: int,
                              dkv_batch_stride: int, B: int, Hq: int, Hkv: int, Lq: int, T: int, precision="bf16x3",
                              workspace: Optional[torch.Tensor] = None) -> None:
    """Writes dq (laid out like q) and dk / dv (the cache's layout at pitch lddkv and batch stride dkv_batch_stride) of `causal_attention_lse`
    (awt_op_causal_attention_backward).  Every tensor argument but lse is a (tensor, element offset) pair."""
    terms = precision if isinstance(precision, int) else _terms(precision)
    dev = q[0].device
    L = _lib.lib()
    ws = _lib.workspace(L.awt_op_causal_attention_backward_workspace_bytes(B, Hq, Lq, T), dev) if workspace is None else workspace
    with torch.cuda.device(dev):
        _lib.check(L.awt_op_causal_attention_backward(_lib.ctx(dev), _at(q), int(ldq), _at(k), _at(v), int(ldkv), int(kv_batch_stride), _at(o), _at(dout), int(ldo),
                                                      _lib.ptr(lse), _at(dq), _at(dk), _at(dv), int(lddkv), int(dkv_batch_stride), int(B), int(Hq), int(Hkv),
                                                      int(Lq), int(T), int(terms), _lib.ptr(ws), ws.numel(), _lib.stream_handle()))


def rmsnorm_backward(dy, lddy: int, x, ldx: int, gamma: torch.Tensor, M: int, d: int, eps: float, dres=None, dx=None, lddx: Optional[int] = None):
    """dx = [dres +] d(RMSNorm(x) gamma)/dx . dy (awt_op_rmsnorm_backward).  dy, x (and dres / dx, both at pitch lddx): (tensor, element offset) pairs.
    Returns dx's tensor ([M, d] unless given; dx may be dres)."""
    dev = x[0].device
    if dx is None:
        dx, lddx = (torch.empty((M, d), dtype=torch.float32, device=dev), 0), d
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().awt_op_rmsnorm_backward(_lib.ctx(dev), _at(dy), int(lddy), _at(x), int(ldx), _at((gamma, 0)), None if dres is None else _at(dres),
                                                      _at(dx), int(lddx), int(M), int(d), float(eps), _lib.stream_handle()))
    return dx[0]


def rmsnorm_param_grad(dy, lddy: int, x, ldx: int, M: int, d: int, eps: float) -> torch.Tensor:
    """dgamma [d] = sum_m dy[m] * x[m] * rsqrt(mean(x[m]^2) + eps) (awt_op_rmsnorm_param_grad)."""
    dev = x[0].device
    L = _lib.lib()
    dg = torch.empty(d, dtype=torch.float32, device=dev)
    ws = _lib.workspace(L.awt_op_rmsnorm_param_grad_workspace_bytes(M, d), dev)
    with torch.cuda.device(dev):
        _lib.check(L.awt_op_rmsnorm_param_grad(_lib.ctx(dev), _at(dy), int(lddy), _at(x), int(ldx), _lib.ptr(dg), int(M), int(d), float(eps), _lib.ptr(ws),
                                               ws.numel(), _lib.stream_handle()))
    return dg


def silu_mul_backward(gu, ld: int, dy, lddy: int, M: int, I: int, dgu=None, lddgu: Optional[int] = None):
    """dgu [M, 2 I] (gate | up) of `silu_mul` under dy [M, I] (awt_op_silu_mul_backward).  Returns dgu's tensor ([M, 2 I] unless given)."""
    dev = gu[0].device
    if dgu is None:
        dgu, lddgu = (torch.empty((M, 2 * I), dtype=torch.float32, device=dev), 0), 2 * I
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().awt_op_silu_mul_backward(_lib.ctx(dev), _at(gu), int(ld), _at(dy), int(lddy), _at(dgu), int(lddgu), int(M), int(I), _lib.stream_handle()))
    return dgu[0]


def qk_norm_rope_backward_workspace_bytes(B: int, Lq: int, Hq: int, Hkv: int) -> int:
    """Workspace of `qk_norm_rope_backward`'s gain gradients; answers without a GPU."""
    return int(_lib.lib().awt_op_qk_norm_rope_backward_workspace_bytes(int(B), int(Lq), int(Hq), int(Hkv)))


def qk_norm_rope_backward(qkv, ld: int, q_gamma: torch.Tensor, k_gamma: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor, positions: torch.Tensor, dq, ldq: int,
                          dk, dv, ldkv: int, kv_batch_stride: int, dqkv, B: int, Lq: int, Hq: int, Hkv: int, eps: float, want_gains: bool = False):
    """Backward of `qk_norm_rope` into dqkv (laid out like qkv) from dq and the cache-layout dk / dv (awt_op_qk_norm_rope_backward).  With want_gains returns
    (dq_gamma, dk_gamma) [128] each, else None."""
    dev = qkv[0].device
    if positions.dtype != torch.int32 or positions.numel() != B * Lq or not positions.is_contiguous():
        raise ValueError("qk_norm_rope_backward: positions must be a contiguous int32 tensor of B * Lq elements")
    L = _lib.lib()
    gains = (torch.empty(128, dtype=torch.float32, device=dev), torch.empty(128, dtype=torch.float32, device=dev)) if want_gains else (None, None)
    ws = _lib.workspace(L.awt_op_qk_norm_rope_backward_workspace_bytes(B, Lq, Hq, Hkv), dev) if want_gains else None
    with torch.cuda.device(dev):
        _lib.check(L.awt_op_qk_norm_rope_backward(_lib.ctx(dev), _at(qkv), int(ld), _at((q_gamma, 0)), _at((k_gamma, 0)), _at((cos, 0)), _at((sin, 0)),
                                                  _lib.ptr(positions), _at(dq), int(ldq), _at(dk), _at(dv), int(ldkv), int(kv_batch_stride), _at(dqkv),
                                                  _lib.ptr(gains[0]), _lib.ptr(gains[1]), int(B), int(Lq), int(Hq), int(Hkv), float(eps), _lib.ptr(ws),
                                                  0 if ws is None else ws.numel(), _lib.stream_handle()))
    return gains if want_gains else None
