"""Global-norm clipping + AdamW restated on plain tensors, with a step counter per parameter (a plain module: tests/test_optim_host.py holds it to
`clip_grad_norm_` + `torch.optim.AdamW` in float64, tests/test_gpu_optim.py compares csrc/optim.hip with it).

It computes in the dtype of the tensors it is given: float64 tensors make it the reference, float32 tensors the "fp32 torch restatement" whose own
distance from float64 scales the GPU test's bound.  Hyper-parameters are Python floats, as torch's optimizers hold them."""
import math

import torch

CLIP_EPS = 1e-6          # clip_grad_norm_: max_norm / (total_norm + 1e-6)


def total_norm(grads):
    """The 2-norm of all gradients together, formed as clip_grad_norm_ forms it: the norm of the per-tensor norms."""
    return torch.linalg.vector_norm(torch.stack([torch.linalg.vector_norm(g) for g in grads]))


def clip_coefficient(norm, max_norm):
    """min(1, max_norm / (norm + 1e-6)); 1 when max_norm is None, <= 0 or infinite.  A NaN norm gives a NaN coefficient (torch.clamp keeps it)."""
    if max_norm is None or max_norm <= 0 or math.isinf(max_norm):
        return torch.ones_like(norm)
    return torch.clamp(max_norm / (norm + CLIP_EPS), max=1.0)


class ReferenceAdamW:
    """params: tensors, updated in place; group_of[i]: the group of params[i]; groups: dicts with lr, weight_decay, betas, eps (lr may be changed
    between steps, as a scheduler does).  State per parameter: steps[i] (int), m[i], v[i]."""

    def __init__(self, params, group_of, groups):
        self.params, self.group_of, self.groups = list(params), list(group_of), [dict(g) for g in groups]
        self.steps = [0] * len(self.params)
        self.m = [torch.zeros_like(p) for p in self.params]
        self.v = [torch.zeros_like(p) for p in self.params]

    def step(self, grads, max_norm=None):
        """grads[i]: the gradient of params[i], or None: that parameter is left out (its counter does not advance, the norm does not see it).
        The gradients are not modified.  Returns (total norm, clip coefficient)."""
        live = [i for i, g in enumerate(grads) if g is not None]
        norm = total_norm([grads[i] for i in live])
        coef = clip_coefficient(norm, max_norm)
        for i in live:
            h = self.groups[self.group_of[i]]
            lr, wd, (b1, b2), eps = h["lr"], h["weight_decay"], h["betas"], h["eps"]
            p, m, v = self.params[i], self.m[i], self.v[i]
            g = grads[i] * coef
            self.steps[i] += 1
            t = self.steps[i]
            bc1, bc2 = 1.0 - b1 ** t, 1.0 - b2 ** t
            p.mul_(1.0 - lr * wd)
            m.add_((g - m) * (1.0 - b1))
            v.mul_(b2).add_((1.0 - b2) * (g * g))
            denom = v.sqrt() / math.sqrt(bc2) + eps
            p.sub_((lr / bc1) * (m / denom))
        return norm, coef


# ---- the schedule tests/test_optim_host.py (against torch in float64) and tests/test_gpu_optim.py (FusedAdamW beside torch on the GPU) share
SHAPES = [(7,), (3, 5), (1,), (4, 4)]
GROUP_OF = [0, 0, 1, 1]
# learning rates well below |p| / 2 of the one-element parameter: there one u of difference in the clip coefficient moves the update by less than the u |p| an
# fp32 result is allowed to be off by (tests/test_gpu_optim.py compares fp32 optimizers on this schedule)
GROUPS = [dict(lr=1e-3, weight_decay=1e-2, betas=(0.9, 0.999), eps=1e-8), dict(lr=3e-4, weight_decay=0.0, betas=(0.8, 0.99), eps=1e-6)]
MAX_NORM = 1.0


def schedule_grads(step, shapes=SHAPES, dtype=torch.float64):
    """The gradients of step 0 .. 4 of the shared schedule: seeded, large enough that max_norm = 1 clips in some steps and not in others; parameter 1 has
    no gradient in step 3 (index 2)."""
    gen = torch.Generator().manual_seed(100 + step)
    scale = (2.0, 0.05, 1.0, 0.02, 0.7)[step]
    grads = [(scale * torch.randn(s, generator=gen, dtype=torch.float64)).to(dtype) for s in shapes]
    if step == 2:
        grads[1] = None
    return grads


def schedule_params(shapes=SHAPES, dtype=torch.float64):
    gen = torch.Generator().manual_seed(7)
    return [torch.randn(s, generator=gen, dtype=torch.float64).to(dtype) for s in shapes]
