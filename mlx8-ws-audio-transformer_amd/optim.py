"""The optimizer phase of a training step on libawt: `FusedAdamW`, global-norm clipping and AdamW over every parameter in three kernel launches
(include/awt_optim.h, csrc/optim.hip).

    opt = FusedAdamW([{"params": adapter, "lr": 1e-4}, {"params": qwen, "lr": 2e-5}], weight_decay=1e-4)
    loss.backward()
    norm = opt.step(max_norm=1.0)          # = clip_grad_norm_(params, 1.0); opt.step() -- except that the .grad tensors keep their values

The step counters, the hyper-parameters and the tensor table live on the device: `step()` reads nothing back, so it runs under
`torch.cuda.set_sync_debug_mode("error")`, and a learning-rate scheduler reaches the kernel through `param_groups` as it does with torch's optimizers.
There is no fallback: without libawt or a GPU `step()` raises.
"""
from __future__ import annotations

import math
from typing import List, Optional, Sequence, Tuple

import torch

from . import _lib

TENSOR_WORDS = 6            # awt_optim_tensor as int64 words: p, g, m, v, n, group | index << 32
GROUP_FLOATS = 8            # awt_optim_group: lr, weight_decay, beta1, beta2, eps, pad[3]


def chunk_elems() -> int:
    """Elements one workgroup handles (`awt_optim_chunk_elems`); answers without a GPU."""
    return int(_lib.lib().awt_optim_chunk_elems())


def workspace_bytes(chunks: int) -> int:
    """Workspace of a step over `chunks` chunks (`awt_op_adamw_workspace_bytes`); answers without a GPU."""
    return int(_lib.lib().awt_op_adamw_workspace_bytes(int(chunks)))


def chunk_table(sizes: Sequence[int], chunk: Optional[int] = None) -> List[int]:
    """first_chunk of include/awt_optim.h for tensors of the given element counts: [0, c_0, c_0 + c_1, ...] with c_t = ceil(n_t / chunk); the last entry
    is the launch's workgroup count."""
    chunk = chunk or chunk_elems()
    first = [0]
    for n in sizes:
        if n < 1:
            raise ValueError("a tensor of the optimizer's table needs at least one element")
        first.append(first[-1] + (int(n) + chunk - 1) // chunk)
    return first


def tensor_table(entries: Sequence[Tuple[int, int, int, int, int, int, int]]) -> torch.Tensor:
    """Host int64 [T, 6] image of awt_optim_tensor[T] from (p, g, m, v pointers, n, group, index) rows."""
    rows = [[p, g, m, v, n, (group & 0xFFFFFFFF) | (index << 32)] for p, g, m, v, n, group, index in entries]
    return torch.tensor(rows, dtype=torch.int64).reshape(len(rows), TENSOR_WORDS)


def group_table(groups: Sequence[Tuple[float, float, float, float, float]]) -> torch.Tensor:
    """Host float32 [G, 8] image of awt_optim_group[G] from (lr, weight_decay, beta1, beta2, eps) rows."""
    return torch.tensor([list(g) + [0.0] * (GROUP_FLOATS - 5) for g in groups], dtype=torch.float32).reshape(len(groups), GROUP_FLOATS)


def adamw_step(tensors: torch.Tensor, first_chunk: torch.Tensor, chunks: int, groups: torch.Tensor, steps: torch.Tensor, max_norm: float = 0.0,
               norm_out: Optional[torch.Tensor] = None, workspace: Optional[torch.Tensor] = None) -> torch.Tensor:
    """`awt_op_adamw_step` on device tables: tensors int64 [T, 6] (`tensor_table`), first_chunk int32 [T + 1] and chunks, its last entry (`chunk_table`),
    groups float32 [G, 8] (`group_table`), steps float32 [P].  Updates the p, m, v the table points at and `steps` in place; returns norm_out float32 [2]
    = (total norm, clip coefficient).  max_norm <= 0 or infinite: no clipping.  The caller keeps the tensors the table points at alive and apart."""
    L = _lib.lib()
    T, G = tensors.shape[0], groups.shape[0]
    if tensors.dtype != torch.int64 or tensors.shape != (T, TENSOR_WORDS) or first_chunk.dtype != torch.int32 or first_chunk.shape != (T + 1,):
        raise ValueError("adamw_step: tensors must be int64 [T, 6] and first_chunk int32 [T + 1]")
    if groups.dtype != torch.float32 or groups.shape != (G, GROUP_FLOATS) or steps.dtype != torch.float32:
        raise ValueError("adamw_step: groups must be float32 [G, 8] and steps float32")
    dev = tensors.device
    norm_out = torch.empty(2, dtype=torch.float32, device=dev) if norm_out is None else norm_out
    need = workspace_bytes(chunks)
    ws = _lib.workspace(need, dev) if workspace is None else workspace
    with torch.cuda.device(dev):
        _lib.check(L.awt_op_adamw_step(_lib.ctx(dev), _lib.ptr(tensors), _lib.ptr(first_chunk), T, int(chunks), _lib.ptr(groups), G, _lib.ptr(steps),
                                       float(max_norm), _lib.ptr(norm_out), _lib.ptr(ws), ws.numel() * ws.element_size(), _lib.stream_handle()))
    return norm_out


class FusedAdamW(torch.optim.Optimizer):
    """torch.optim.AdamW's constructor, parameter groups and state (`step`, `exp_avg`, `exp_avg_sq` per parameter, so `state_dict()` /
    `load_state_dict()` exchange with torch.optim.AdamW in both directions) on one fused operator, with the global-norm clip in the same pass:
    `step(max_norm)` returns the total gradient norm as a device tensor, whether or not it clipped.

    Only what the kernel computes is accepted: fp32 contiguous parameters on one GPU; `amsgrad` and `maximize` raise ValueError.  Unlike
    `clip_grad_norm_`, the `.grad` tensors are left as they are (the coefficient is applied on the fly).  The `step` entries of the state are views of
    one device vector.  A parameter without a gradient is left out of the step and its counter does not advance; a parameter object listed twice is
    stepped once.  After the launch the autograd version of every stepped parameter is bumped, so whatever tracks `(id, _version)` -- the decoders'
    packed operands -- sees exactly the changed ones."""

    def __init__(self, params, lr: float = 1e-3, betas: Tuple[float, float] = (0.9, 0.999), eps: float = 1e-8, weight_decay: float = 1e-2,
                 amsgrad: bool = False, *, maximize: bool = False):
        if amsgrad or maximize:
            raise ValueError("FusedAdamW computes torch.optim.AdamW with amsgrad=False and maximize=False only")
        if isinstance(lr, torch.Tensor):
            raise ValueError("FusedAdamW takes lr as a Python number (it is sent to the device when it changes)")
        if not 0.0 <= lr or not 0.0 <= eps or not 0.0 <= weight_decay or not 0.0 <= betas[0] < 1.0 or not 0.0 <= betas[1] < 1.0:
            raise ValueError(f"invalid hyper-parameter: lr {lr}, betas {betas}, eps {eps}, weight_decay {weight_decay}")
        # every key the installed torch.optim.AdamW keeps in a group, at torch's own defaults (foreach, capturable, ...): a state dict of this class loads into
        # torch's and steps there
        defaults = dict(torch.optim.AdamW([torch.nn.Parameter(torch.zeros(1))]).defaults)
        defaults.update(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=False, maximize=False)
        self._index, self._device, self._steps = {}, None, None
        super().__init__(params, defaults)
        self._tensors = self._first = self._groups = self._workspace = self._chunks = None
        self._tensor_key = self._group_key = None
        self.last_norm = None              # float32 [2] of the last step: total norm, clip coefficient

    # ---- state
    def add_param_group(self, param_group) -> None:
        super().add_param_group(param_group)
        group = self.param_groups[-1]
        if group.get("amsgrad") or group.get("maximize"):
            raise ValueError("FusedAdamW computes torch.optim.AdamW with amsgrad=False and maximize=False only")
        for p in group["params"]:
            if p.dtype != torch.float32 or not p.is_contiguous() or p.is_sparse:
                raise ValueError(f"FusedAdamW needs fp32 contiguous parameters, got {p.dtype} with strides {tuple(p.stride())}")
            self._index.setdefault(id(p), len(self._index))                # one counter per parameter object: a parameter listed twice has one
        if self._steps is not None and self._steps.numel() < len(self._index):          # a group added after the first step: the vector grows
            self._steps = torch.cat([self._steps, self._steps.new_zeros(len(self._index) - self._steps.numel())])
            for q, st in self.state.items():
                if "step" in st:
                    st["step"] = self._steps[self._index[id(q)]]

    def _ensure_steps(self, device) -> torch.Tensor:
        if self._steps is None:
            if device.type != "cuda":
                raise RuntimeError("FusedAdamW steps parameters on an MI355X (gfx950) GPU: there is no CPU fallback")
            self._steps, self._device = torch.zeros(len(self._index), dtype=torch.float32, device=device), device
        elif device != self._device:
            raise ValueError(f"FusedAdamW: every parameter must live on {self._device}, got {device}")
        return self._steps

    def _state_of(self, p) -> dict:
        st = self.state[p]
        if not st:
            st["step"] = self._ensure_steps(p.device)[self._index[id(p)]]
            st["exp_avg"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
            st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
        return st

    def load_state_dict(self, state_dict) -> None:
        """torch's loading (a state dict of torch.optim.AdamW or of this class), then the counters are gathered into the device vector again."""
        super().load_state_dict(state_dict)
        host, seen = [0.0] * len(self._index), []
        for p, st in self.state.items():
            if "step" in st:
                host[self._index[id(p)]] = float(st["step"])
                seen.append(p)
        if not seen:
            return
        self._steps = None
        steps = self._ensure_steps(seen[0].device)
        steps.copy_(torch.tensor(host, dtype=torch.float32))
        for p in seen:
            st = self.state[p]
            st["step"] = steps[self._index[id(p)]]
            for k in ("exp_avg", "exp_avg_sq"):
                st[k] = st[k].to(device=p.device, dtype=torch.float32).contiguous()
        self._tensor_key = None

    # ---- the step
    def _upload(self, host: torch.Tensor, dst: Optional[torch.Tensor]) -> torch.Tensor:
        """host -> device through a pinned staging tensor of its own: torch's host allocator hands a pinned block out again only after the copies
        that read it have completed on their streams, so the next upload never overwrites bytes an earlier copy has still to read."""
        stage = torch.empty(host.shape, dtype=host.dtype, pin_memory=True)
        stage.copy_(host)
        if dst is None or dst.shape != host.shape:
            dst = torch.empty(host.shape, dtype=host.dtype, device=self._device)
        dst.copy_(stage, non_blocking=True)
        return dst

    @torch.no_grad()
    def step(self, max_norm: Optional[float] = None) -> Optional[torch.Tensor]:
        """One AdamW step of every parameter that has a gradient, after scaling the gradients (on the fly) to a total norm of at most `max_norm`
        (None, <= 0 or inf: no clipping).  Returns the total norm before clipping, a 0-dim device tensor; None when no parameter has a gradient.
        A closure is refused: `step` returns the norm, not a closure's loss."""
        if callable(max_norm):                                             # torch's convention step(closure)
            raise ValueError("FusedAdamW.step takes no closure (it returns the gradient norm): evaluate the loss and call backward() before step()")
        entries, params, seen = [], [], set()
        for gi, group in enumerate(self.param_groups):
            for p in group["params"]:
                g = p.grad
                if g is None or id(p) in seen or p.numel() == 0:
                    continue
                seen.add(id(p))
                if g.is_sparse or g.dtype != torch.float32 or not g.is_contiguous() or g.device != p.device or not p.is_contiguous():
                    raise ValueError("FusedAdamW needs dense fp32 contiguous gradients on the parameter's device")
                st = self._state_of(p)
                entries.append((p.data_ptr(), g.data_ptr(), st["exp_avg"].data_ptr(), st["exp_avg_sq"].data_ptr(), p.numel(), gi, self._index[id(p)]))
                params.append(p)
        if not entries:
            return None
        key = tuple(entries)
        if key != self._tensor_key:
            first = chunk_table([e[4] for e in entries])
            self._tensors = self._upload(tensor_table(entries), self._tensors)
            self._first = self._upload(torch.tensor(first, dtype=torch.int32), self._first)
            if first[-1] != self._chunks:
                self._chunks, self._workspace = first[-1], _lib.workspace(workspace_bytes(first[-1]), self._device)
            self._tensor_key = key
        gkey = tuple((float(g["lr"]), float(g["weight_decay"]), float(g["betas"][0]), float(g["betas"][1]), float(g["eps"])) for g in self.param_groups)
        if gkey != self._group_key:
            self._groups = self._upload(group_table(gkey), self._groups)
            self._group_key = gkey
        clip = 0.0 if max_norm is None or math.isinf(float(max_norm)) else float(max_norm)
        self.last_norm = adamw_step(self._tensors, self._first, self._chunks, self._groups, self._steps, clip, workspace=self._workspace)
        torch.autograd.graph.increment_version(params)
        return self.last_norm[0]
