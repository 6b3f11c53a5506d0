"""A hostile allocator under the shipping wrappers: every tensor an operator call allocates or is handed lies between two canaries, is exactly
as long as was asked for and holds NaN until the operator writes it.  (A plain module: the cases are in tests/test_gpu_hostile_alloc.py, the
checks of this plumbing, on the CPU, in tests/test_hostile_alloc_host.py.)

torch's caching allocator hides three kinds of bug:
  * a write outside a tensor lands in a neighbouring cached block: no fault, and no assertion looks at that block;
  * a read of bytes nobody wrote (an uncleared workspace slab, the element past an input's end) returns small finite leftovers;
  * a write to an input the operator does not own goes unseen, because nothing compares an input with itself.

`run_fenced(fn, make_state, in_place)` runs `fn` once the plain way and once with every state tensor re-homed between 0xFF guards (`fence`)
and every factory call of the wrappers served by `HostileAlloc`; then the guards must be whole, outputs and state must have the plain run's
bits, and every state tensor the call is not documented to update must have the bits it had before.  There is no tolerance anywhere.
"""
from __future__ import annotations

import torch
from torch.utils._python_dispatch import TorchDispatchMode

from tests.graph_capture import bits, same_bits

GUARD_BYTES = 65536
ALIGN = 256
CANARY = 0xA5                  # guards of a buffer the operator's wrapper allocated: a write there is the finding
POISON = 0xFF                  # NaN in fp32, fp16, bf16 and e4m3, -1 in the integer types: interiors before the call, and the guards of inputs

_aten = torch.ops.aten
_EMPTY = {_aten.empty.memory_format, _aten.empty_strided.default, _aten.empty_like.default, _aten.new_empty.default}
_ZEROS = {_aten.zeros.default, _aten.zeros_like.default, _aten.new_zeros.default}
_FULL = {_aten.full.default, _aten.full_like.default, _aten.new_full.default}
_LIKE = {_aten.empty_like.default, _aten.zeros_like.default, _aten.full_like.default}
_NEW = {_aten.new_empty.default, _aten.new_zeros.default, _aten.new_full.default}
FACTORIES = _EMPTY | _ZEROS | _FULL


class Buffer:
    """One allocation: `raw` is the uint8 tensor guard + n + guard long, `tensor` its interior in the requested dtype and shape."""

    def __init__(self, raw, tensor, guard, fill, name):
        self.raw, self.tensor, self.guard, self.fill, self.name = raw, tensor, guard, fill, name

    def broken_guards(self):
        """Human-readable places of the guard bytes that no longer hold their fill (empty: both guards are whole)."""
        g, found = self.guard, []
        for side, part, base in (("in front of", self.raw[:g], -g), ("behind", self.raw[self.raw.numel() - g:], 0)):
            bad = (part != self.fill).nonzero()
            if bad.numel():
                first, last = int(bad[0]) + base, int(bad[-1]) + base
                found.append(f"{bad.numel()} byte(s) {side} it, offsets {first} .. {last} from that end")
        return found


def _matches(got: torch.device, want: torch.device) -> bool:
    return got.type == want.type and (got.index is None or want.index is None or got.index == want.index)


def guarded_buffer(shape, dtype, device, guard=GUARD_BYTES, guard_fill=CANARY, name="") -> Buffer:
    """A tensor of POISON bytes, exactly numel * itemsize long and 256-byte aligned, between two guards of `guard_fill` bytes."""
    shape = tuple(int(d) for d in shape)
    numel = 1
    for d in shape:
        numel *= d
    n = numel * torch.empty((), dtype=dtype).element_size()
    assert guard % ALIGN == 0
    slab = torch.empty(guard + n + guard + ALIGN, dtype=torch.uint8, device=device)
    shift = (-slab.data_ptr()) % ALIGN                     # 0 wherever the allocator already aligns to 256 bytes (the device's does)
    raw = slab[shift:shift + guard + n + guard]
    raw.fill_(guard_fill)
    raw[guard:guard + n] = POISON
    tensor = raw[guard:guard + n].view(dtype).view(shape)
    assert tensor.data_ptr() % ALIGN == 0 and tensor.is_contiguous() and tensor.numel() * tensor.element_size() == n
    return Buffer(raw, tensor, guard, guard_fill, name)


def _contiguous_strides(size):
    strides, acc = [], 1
    for d in reversed(tuple(size)):
        strides.append(acc)
        acc *= max(int(d), 1)
    return tuple(reversed(strides))


class HostileAlloc(TorchDispatchMode):
    """Serves the factory ops that target `device` from guarded, poisoned, exactly-sized buffers; everything else passes through untouched."""

    def __init__(self, device, guard_bytes=GUARD_BYTES, interior=POISON):
        super().__init__()
        self.device, self.guard, self.interior = torch.device(device), int(guard_bytes), interior
        self.buffers: list[Buffer] = []
        self.passed_through = 0

    def _request(self, func, args, kwargs):
        """(shape, dtype, fill) of a contiguous request on our device, or None to pass the call through."""
        if kwargs.get("layout") not in (None, torch.strided) or kwargs.get("pin_memory"):
            return None
        like = func in _LIKE or func in _NEW
        src = args[0] if like else None
        device = kwargs.get("device")
        device = torch.device(device) if device is not None else (src.device if like else torch.device("cpu"))
        if not _matches(device, self.device):
            return None
        dtype = kwargs.get("dtype") or (src.dtype if like else torch.get_default_dtype())
        if func in _LIKE:
            fmt = kwargs.get("memory_format") or torch.preserve_format
            if fmt not in (torch.preserve_format, torch.contiguous_format) or (fmt == torch.preserve_format and not src.is_contiguous()):
                return None
            shape = tuple(src.shape)
        else:
            shape = tuple(args[1] if func in _NEW else args[0])
            if func is _aten.empty.memory_format and kwargs.get("memory_format") not in (None, torch.contiguous_format):
                return None
            if func is _aten.empty_strided.default:
                stride = tuple(args[1])
                if any(d > 1 and s != c for d, s, c in zip(shape, stride, _contiguous_strides(shape))):
                    return None
        if any(not isinstance(d, int) for d in shape):
            return None
        fill = None
        if func in _ZEROS:
            fill = 0
        elif func in _FULL:
            fill = args[2] if func in _NEW else args[1]
            if "dtype" not in kwargs and not like:                     # torch.full infers the dtype from the fill value
                dtype = torch.bool if isinstance(fill, bool) else torch.int64 if isinstance(fill, int) else dtype
        if dtype.is_complex or (dtype == torch.bool and fill is None):
            return None                                                # no NaN / -1 reading of 0xFF bytes: left to torch
        return shape, dtype, fill

    def __torch_dispatch__(self, func, types, args=(), kwargs=None):
        kwargs = kwargs or {}
        req = self._request(func, args, kwargs) if func in FACTORIES else None
        if req is None:
            self.passed_through += func in FACTORIES
            return func(*args, **kwargs)
        shape, dtype, fill = req
        buf = guarded_buffer(shape, dtype, self.device, self.guard, CANARY, name=f"allocation {len(self.buffers)} ({func.name()} {list(shape)} {dtype})")
        if self.interior != POISON:
            buf.raw[self.guard:buf.raw.numel() - self.guard] = self.interior
        if fill is not None:
            buf.tensor.fill_(fill)
        self.buffers.append(buf)
        return buf.tensor


def fence(state: dict, device, guard_bytes=GUARD_BYTES):
    """Every tensor of `state` copied into a buffer of the same construction whose guards are POISON: what is read from just outside an input is
    a NaN.  Returns (the new dict, the buffers)."""
    out, bufs = {}, []
    for k, t in state.items():
        assert t.is_contiguous(), f"state tensor {k!r} is not contiguous: build the view inside fn"
        b = guarded_buffer(t.shape, t.dtype, device, guard_bytes, POISON, name=f"state tensor {k!r}")
        b.tensor.copy_(t)
        out[k] = b.tensor
        bufs.append(b)
    return out, bufs


def _sync(device):
    if torch.device(device).type == "cuda":
        torch.cuda.synchronize()


def _clone(state):
    return {k: v.detach().clone() for k, v in state.items()}


def _outputs(fn, state):
    outs = fn(state)
    assert isinstance(outs, tuple) and outs and all(isinstance(o, torch.Tensor) for o in outs), "fn must return a tuple of tensors"
    return outs


def run_fenced(fn, make_state, in_place=(), device="cuda", guard_bytes=GUARD_BYTES, interior=POISON):
    """fn(state) -> tuple of tensors and make_state(seed) -> dict of tensors as in tests/graph_capture.py; `in_place` names the state keys the call is
    documented to update.  Returns the number of allocations the hostile run intercepted."""
    unknown = set(in_place) - set(make_state(0))
    assert not unknown, f"in_place names no state tensor: {sorted(unknown)}"

    plain = make_state(0)
    before = _clone(plain)
    plain_outs = _outputs(fn, plain)
    _sync(device)
    plain_outs, plain_after = tuple(o.detach().clone() for o in plain_outs), _clone(plain)

    state, bufs = fence(make_state(0), device, guard_bytes)
    for k in state:
        assert same_bits(state[k], before[k]), f"make_state(0) is not reproducible: state tensor {k!r}"
    with HostileAlloc(device, guard_bytes, interior) as mode:
        outs = _outputs(fn, state)
        _sync(device)

    for b in bufs + mode.buffers:
        broken = b.broken_guards()
        assert not broken, f"guard bytes overwritten around {b.name}: " + "; ".join(broken)
    assert len(outs) == len(plain_outs)
    for i, (got, want) in enumerate(zip(outs, plain_outs)):
        assert same_bits(got, want), f"output {i} of the hostile run is not bit-equal to the plain run{_where(got, want)}"
    for k in state:
        assert same_bits(state[k], plain_after[k]), f"state tensor {k!r} after the hostile run is not bit-equal to the plain run{_where(state[k], plain_after[k])}"
    for k in state:
        if k not in in_place:
            assert same_bits(plain_after[k], before[k]), f"input {k!r} is not declared in_place but changed in the plain run{_where(plain_after[k], before[k])}"
            assert same_bits(state[k], before[k]), f"input {k!r} is not declared in_place but changed in the hostile run{_where(state[k], before[k])}"
    for k in in_place:
        assert not same_bits(plain_after[k], before[k]), f"stale IN_PLACE table: {k!r} is declared in_place but the plain run left it unchanged"
    return len(mode.buffers)


def _where(got, want) -> str:
    """Where two tensors of one shape first differ, for the message."""
    if got.shape != want.shape or got.dtype != want.dtype:
        return f" ({list(got.shape)} {got.dtype} against {list(want.shape)} {want.dtype})"
    diff = (bits(got) != bits(want)).reshape(-1).nonzero()
    if not diff.numel():
        return ""
    i = int(diff[0])
    return f" ({diff.numel()} of {got.numel()} elements, first at flat index {i}: {got.reshape(-1)[i].item()!r} against {want.reshape(-1)[i].item()!r})"


# ---------------------------------------------------------------------------------------------------------------------------------------
# Case of tests/test_gpu_graph_capture.py::CASES (and of EDGES in tests/test_gpu_hostile_alloc.py) -> the state keys the call is documented to
# update (include/awt.h, and the case's own comments).  A case that is not here updates nothing: every state tensor must keep its bits.
IN_PLACE = {
    "linear_fused-f32_resid": ("y",),                                  # y += x w^T + b: `resid` and the output are the same buffer
    "linear_fused-qkv-bf16x3": ("hi", "lo"),                           # the head-major planes are the caller's
    "linear_fused-qkv-f16f8": ("hi", "hi8", "lo8"),
    "qk_norm_rope": ("kc", "vc"),                                      # rows pos0 .. pos0 + Lq - 1 of both caches
    "rmsnorm_backward-dres_in_place": ("dres",),                       # dx and dres are the same buffer
    "packed_linear_forward": ("y",),                                   # y = x W^T + b + y
    "bmm_pack_update": ("out",),                                       # out += a b^T
    "embed_backward": ("dtok", "dpos"),                                # added to the two tables' gradients
    "column_sums_ld": ("sums",),                                       # accumulate = True
    "kv_gather": ("dst",),
    "softmax_rows": ("s",),                                            # in place: rows -> softmax(scale * row[:cols])
    "softmax_rows_backward": ("dp",),                                  # in place on dp
    "qwen3_prefill": ("k0", "v0", "k1", "v1"),                         # rows 0 .. L - 1 of every layer's cache
    "qwen3_step-B1": ("k0", "v0", "k1", "v1"),                         # row t of every layer's cache
    "qwen3_step-B3": ("k0", "v0", "k1", "v1"),
    "qwen3_step-B9": ("k0", "v0", "k1", "v1"),
    # the edge cases of tests/test_gpu_hostile_alloc.py
    "embed_backward-7x7x1280x509": ("tok", "pos"),
    "column_sums_ld-37x384x256x128": ("sums",),
    "softmax_rows-3x70x72": ("s", "dp"),
    "softmax_rows-5x1x4": ("s", "dp"),
    "bmm_kmajor-two_blocks_pitched": ("acc",),
    "rmsnorm-67x260-pitched": ("y",),
    "qk_norm_rope-2x33x16x8": ("kc", "vc"),
    "causal_attention_backward-2x4x2x37x37": ("dq", "dk", "dv"),
    "causal_attention_backward-1x2x1x40x70-pitched": ("dq", "dk", "dv"),
    "kv_gather-2x2to3x1x8x8": ("dst",),
}
