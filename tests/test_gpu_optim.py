"""The optimizer phase on the GPU: awt_op_adamw_step (csrc/optim.hip) against the float64 restatement of tests/adamw_reference.py, `FusedAdamW` beside
`clip_grad_norm_` + `torch.optim.AdamW`, and `train_music2midi` on the micro tied model of tests/test_gpu_qwen3_train.py.

Bounds.  Per tensor and per step, max|native - f64| <= 4 x max|fp32 restatement - f64| + 2^-24 max|p|: the restatement is the same class on float32
tensors, so the bound moves with what fp32 arithmetic itself loses on the case's values.  The operator runs four consecutive steps on its own state; each
step's float64 and fp32 restatements start from the state the operator started that step from (two fp32 trajectories that once round an element to
different neighbours drift apart by whole ulps, which says nothing about either).  That bound is asked of p.  m and v, which no later quantity hides,
are held too, to a bound of this file's own: the same form with the floor (k NORM_REL + 4 u) scale, k = 1 and scale = max(|m|, |g coef|) for m, k = 2 and scale = max(|v|, (g coef)^2) for v: the kernel's element
arithmetic rounds where the restatement rounds, but its clip coefficient comes from another summation order.

The norm.  A thread adds the rounded squares of C / 256 elements one after the other: a relative error of at most (C / 256) u on a sum of non-negative
terms (u = 2^-24; the first addition is exact).  The butterfly over the wave adds 6 roundings, the four waves' partials 3 more.  The partials are then
added in float64 (below 2^-40 here).  The square root halves the relative error, the conversion to fp32 adds one u:
    NORM_REL = ((C / 256 + 9) / 2 + 1) u, times 1.01 for the second-order terms            (21.5 u = 1.3e-6 at C = 8192).
Every figure is printed before it is asserted."""
import copy
import functools
import math

import pytest
import torch

from tests.adamw_reference import GROUP_OF, GROUPS, MAX_NORM, ReferenceAdamW, clip_coefficient, schedule_grads, schedule_params
from tests.graph_capture import capture_replay, same_bits
from tests.hostile_alloc import run_fenced

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
ROLES = ("p", "g", "m", "v")


def f32(x):
    return float(torch.tensor(x, dtype=torch.float32))


# The operator's hyper-parameters are floats: the reference gets the values the table holds.  The learning rates are the training loop's (1e-4 and 2e-5):
# one u of the clip coefficient moves an element's update by about 2 u lr, and the bound's floor for a one-element tensor is u |p|, so the bound can only be
# asked of an fp32 implementation with a summation order of its own where lr is well below |p| / 2.  weight_decay 0.1 makes the decay factor 1 - 1e-5
# something fp32 can hold (the loop's 1 - 1e-8 rounds to 1).
OP_GROUPS = [dict(lr=f32(1e-4), weight_decay=f32(0.1), betas=(f32(0.9), f32(0.999)), eps=f32(1e-8)),
             dict(lr=f32(2e-5), weight_decay=0.0, betas=(f32(0.8), f32(0.99)), eps=f32(1e-6))]


@functools.lru_cache(maxsize=None)
def chunk():
    from mlx8_ws_audio_transformer_amd import optim
    return optim.chunk_elems()


def norm_rel():
    return ((chunk() / 256 + 9) / 2 + 1) * U * 1.01


def edge_sizes():
    C = chunk()
    return [1, 3, 4, 5, 255, 256, 257, C - 1, C, C + 1, 2 * C + 7]


class Table:
    """Tensors cut from four flat buffers (one per role): tensor t of role r starts shifts[r][t] floats (0 .. 3) behind a 16-byte boundary."""

    def __init__(self, sizes, shifts, group_of, groups=OP_GROUPS):
        self.sizes, self.group_of, self.groups = list(sizes), list(group_of), groups
        self.offs, total = {r: [] for r in ROLES}, 0
        for t, n in enumerate(self.sizes):
            for r in ROLES:
                self.offs[r].append(total + shifts[r][t])
            total += (n + 3) // 4 * 4 + 4
        self.total, self._tables = total, {}

    def view(self, buf, role, t):
        return buf[self.offs[role][t]:self.offs[role][t] + self.sizes[t]]

    def make_state(self, seed, g_scale=1.0):
        gen = torch.Generator().manual_seed(50 + seed)
        r = lambda: torch.randn(self.total, generator=gen)
        return {"p": r().cuda(), "g": (g_scale * r()).cuda(), "m": (0.1 * r()).cuda(), "v": (0.01 * r() ** 2).cuda(),
                "steps": torch.arange(len(self.sizes), dtype=torch.float32).remainder(3).cuda()}

    def device_tables(self, s):
        """The operator's tables for the buffers of state s, built from their pointers; kept per pointer set (a graph capture replays the call on the
        same buffers, and uploads nothing)."""
        from mlx8_ws_audio_transformer_amd import optim
        key = tuple(s[r].data_ptr() for r in ROLES)
        if key not in self._tables:
            assert all(s[r].data_ptr() % 16 == 0 for r in ROLES)
            entries = [tuple(s[r].data_ptr() + 4 * self.offs[r][t] for r in ROLES) + (n, self.group_of[t], t) for t, n in enumerate(self.sizes)]
            first = optim.chunk_table(self.sizes)
            groups = [(g["lr"], g["weight_decay"], g["betas"][0], g["betas"][1], g["eps"]) for g in self.groups]
            self._tables[key] = (optim.tensor_table(entries).cuda(), torch.tensor(first, dtype=torch.int32).cuda(), first[-1], optim.group_table(groups).cuda())
        return self._tables[key]

    def fn(self, max_norm):
        from mlx8_ws_audio_transformer_amd import optim

        def run(s):
            tensors, first, chunks, groups = self.device_tables(s)
            return (optim.adamw_step(tensors, first, chunks, groups, s["steps"], max_norm),)
        return run

    def reference(self, s, dtype):
        ref = ReferenceAdamW([self.view(s["p"], "p", t).to(dtype).clone() for t in range(len(self.sizes))], self.group_of, self.groups)
        ref.m = [self.view(s["m"], "m", t).to(dtype).clone() for t in range(len(self.sizes))]
        ref.v = [self.view(s["v"], "v", t).to(dtype).clone() for t in range(len(self.sizes))]
        ref.steps = [int(x) for x in s["steps"].tolist()]
        return ref


def shifts_aligned(T):
    return {r: [0] * T for r in ROLES}


def shifts_mixed(T):
    """Each role's offset chosen on its own: over t every combination class occurs (all equal, all different, one role off), and t % 7 == 0 is all-aligned."""
    mult = {"p": 1, "g": 3, "m": 2, "v": 5}
    return {r: [0 if t % 7 == 0 else (mult[r] * t + (t // 4) * (i + 1)) % 4 for t in range(T)] for i, r in enumerate(ROLES)}


def _mixed_70():
    C = chunk()
    sizes = [(1, 2, 7, 64, 100, 1000, 4097, C // 2 + 3, C, C + 5)[t % 10] + t for t in range(70)]
    return Table(sizes, shifts_mixed(70), [t % 2 for t in range(70)])


TABLES = {
    "edges-aligned-clipping": lambda: (Table(edge_sizes(), shifts_aligned(11), [t % 2 for t in range(11)]), 1.0),
    "edges-offsets-clip_inactive": lambda: (Table(edge_sizes(), shifts_mixed(11), [t % 2 for t in range(11)]), 1e6),
    "mixed70-offsets-clip_off": lambda: (_mixed_70(), 0.0),
    "ones300-offsets-clipping": lambda: (Table([1] * 300, shifts_mixed(300), [(t // 3) % 2 for t in range(300)]), 1.0),
}


@pytest.mark.parametrize("name", list(TABLES))
def test_four_steps_against_float64(name):
    table, max_norm = TABLES[name]()
    T = len(table.sizes)
    s = table.make_state(0)
    g0 = s["g"].clone()
    run = table.fn(max_norm)
    worst, clipped = {"p": 0.0, "m": 0.0, "v": 0.0, "norm": 0.0}, []
    assert len({tuple(table.offs[r][t] % 4 for r in ROLES) for t in range(T)}) > (1 if "offsets" in name else 0)
    want_steps = [int(x) for x in s["steps"].tolist()]
    for step in range(4):
        s["g"].copy_(torch.roll(g0, 17 * step) * (1.0, 0.3, 2.0, 0.01)[step])
        grads = [table.view(s["g"], "g", t) for t in range(T)]
        g_before = s["g"].clone()
        r64, r32 = table.reference(s, torch.float64), table.reference(s, torch.float32)      # this step, from the state the operator starts it from
        assert r64.steps == want_steps, "the counters carry over from the operator's previous step"
        norm_out = run(s)[0]
        n64, c64 = r64.step([g.double() for g in grads], max_norm or None)
        r32.step([g.clone() for g in grads], max_norm or None)
        want_steps = r64.steps
        assert same_bits(s["g"], g_before), "the gradients are read only"
        got_norm, got_coef = (float(x) for x in norm_out.tolist())
        rel = abs(got_norm - float(n64)) / float(n64)
        worst["norm"] = max(worst["norm"], rel)
        want_coef = float(clip_coefficient(torch.tensor(got_norm, dtype=torch.float32), max_norm or None))
        print(f"{name} step {step}: norm {got_norm:.6f} vs f64 {float(n64):.6f} ({rel / U:.2f} u, bound {norm_rel() / U:.1f} u), coef {got_coef:.6f}")
        assert rel <= norm_rel()
        assert abs(got_coef - want_coef) <= 2 * U * want_coef and (got_coef < 1.0) == (float(c64) < 1.0)
        clipped.append(got_coef < 1.0)
        failed = []
        for t in range(T):
            gc = grads[t].double() * c64
            floors = {"p": U * float(r64.params[t].abs().max()),
                      "m": (norm_rel() + 4 * U) * max(float(r64.m[t].abs().max()), float(gc.abs().max())),
                      "v": (2 * norm_rel() + 4 * U) * max(float(r64.v[t].abs().max()), float((gc * gc).max()))}
            for role, want, want32 in (("p", r64.params[t], r32.params[t]), ("m", r64.m[t], r32.m[t]), ("v", r64.v[t], r32.v[t])):
                err = float((table.view(s[role], role, t).double() - want).abs().max())
                err32 = float((want32.double() - want).abs().max())
                bound = 4 * err32 + floors[role]
                worst[role] = max(worst[role], err / bound)
                if not err <= bound:
                    failed.append((step, t, role, err, err32, bound))
        assert not failed, failed[:5]
        assert torch.equal(s["steps"].cpu(), torch.tensor(want_steps, dtype=torch.float32))
    assert any(clipped) == name.endswith("-clipping"), clipped                 # active in one case, inactive (a large max_norm) and off in the others
    print(f"{name}: worst share of the bound p {worst['p']:.3f} m {worst['m']:.3f} v {worst['v']:.3f}; norm {worst['norm'] / U:.2f} u of {norm_rel() / U:.1f} u")


def test_the_update_itself_where_eps_decides_it():
    """The bound on p above is blind to the last formula while lr is far below |p|.  Here it is not: lr 1e-2 and 3e-3 on |p| ~ 1e-3, gradients of
    1e-7 and then 1e-8 so that sqrt(v) stands beside eps (1e-8 in one group, 1e-6 in the other), clipping off (the coefficient is exactly 1), two steps
    from zero moments.  Compared is the update alone, p_after - p_before (1 - lr wd), with float64 from the same state.  On the way to it the kernel
    rounds at most 5 times for m (its one sum of mixed signs has a condition below 1.3), 6.5 for sqrt(v) / sqrt(bc2) + eps, once to divide, twice for
    lr / bc1 and the product: below 16 u of the update; forming p rounds the decay factor, the decayed p and the result: 3 u max|p|."""
    groups = [dict(lr=f32(1e-2), weight_decay=f32(0.1), betas=(f32(0.9), f32(0.999)), eps=f32(1e-8)),
              dict(lr=f32(3e-3), weight_decay=0.0, betas=(f32(0.8), f32(0.99)), eps=f32(1e-6))]
    table = Table(edge_sizes(), shifts_mixed(11), [t % 2 for t in range(11)], groups)
    T = len(table.sizes)
    s = table.make_state(0)
    g0 = s["g"].clone()
    s["p"].mul_(1e-3)
    for k in ("m", "v", "steps"):
        s[k].zero_()
    run, worst, largest = table.fn(0.0), 0.0, 0.0
    for step in range(2):
        s["g"].copy_(g0 * (1e-7, 1e-8)[step])
        before = s["p"].clone()
        r64 = table.reference(s, torch.float64)
        run(s)
        r64.step([table.view(s["g"], "g", t).double() for t in range(T)], None)
        for t in range(T):
            h = groups[table.group_of[t]]
            decayed = table.view(before, "p", t).double() * (1.0 - h["lr"] * h["weight_decay"])
            got, want = table.view(s["p"], "p", t).double() - decayed, r64.params[t] - decayed
            scale = max(float(table.view(before, "p", t).abs().max()), float(table.view(s["p"], "p", t).abs().max()))
            err, tol = float((got - want).abs().max()), 16 * U * float(want.abs().max()) + 3 * U * scale
            worst = max(worst, err / tol)
            largest = max(largest, float(want.abs().max()) / h["lr"])
            assert err <= tol, (step, t, err, tol, err / h["lr"])
    print(f"update against float64: worst share of 16 u |update| + 3 u |p|: {worst:.3f}; largest update {largest:.3f} lr")
    assert largest > 0.5, "the updates are of the learning rate's size, far above u |p|"


def test_two_runs_are_bit_identical():
    table, max_norm = TABLES["edges-offsets-clip_inactive"]()
    outs = []
    for _ in range(2):
        s = table.make_state(3, g_scale=5.0)
        norm = table.fn(1.0)(s)[0]
        torch.cuda.synchronize()
        outs.append(dict(s, norm=norm))
    assert float(outs[0]["norm"][1]) < 1.0
    for k in outs[0]:
        assert same_bits(outs[0][k], outs[1][k]), k


@pytest.mark.parametrize("bad", [float("inf"), float("nan")])
def test_a_non_finite_gradient_does_what_it_does_in_torch(bad):
    """clip_grad_norm_(error_if_nonfinite=False) + AdamW: an inf gives coefficient 0, its own element NaN and every other element a finite step; a NaN
    gives a NaN coefficient and every element of every tensor NaN.  The same elements of p, m and v end up non-finite."""
    C = chunk()
    table = Table([5, 257, C + 1], shifts_aligned(3), [0, 1, 0])
    s = table.make_state(0)
    s["steps"].zero_()
    table.view(s["g"], "g", 1)[100] = bad
    params = [torch.nn.Parameter(table.view(s["p"], "p", t).clone()) for t in range(3)]
    opt = torch.optim.AdamW([dict(params=[params[0], params[2]], **OP_GROUPS[0]), dict(params=[params[1]], **OP_GROUPS[1])])
    for t, p in enumerate(params):
        p.grad = table.view(s["g"], "g", t).clone()
        opt.state[p].update(step=torch.tensor(0.0), exp_avg=table.view(s["m"], "m", t).clone(), exp_avg_sq=table.view(s["v"], "v", t).clone())
    torch.nn.utils.clip_grad_norm_(params, 1.0, error_if_nonfinite=False)
    opt.step()
    norm_out = table.fn(1.0)(s)[0]
    print(f"gradient element {bad}: norm, coefficient {norm_out.tolist()}")
    total = 0
    for t, p in enumerate(params):
        for role, want in (("p", p.detach()), ("m", opt.state[p]["exp_avg"]), ("v", opt.state[p]["exp_avg_sq"])):
            got = table.view(s[role], role, t)
            assert torch.equal(torch.isfinite(got), torch.isfinite(want)), (t, role)
            total += int((~torch.isfinite(got)).sum())
    assert total == (3 if math.isinf(bad) else 3 * sum(table.sizes))


def test_capture_and_replay():
    """Captured on one state and replayed on another: p, m, v and the counters of the replay are the eager call's bits; every replay is one more step."""
    table, _ = TABLES["edges-offsets-clip_inactive"]()
    outs = capture_replay(table.fn(1.0), lambda seed: table.make_state(seed, g_scale=1.0 + seed))
    assert outs[0].shape == (2,)


def test_between_canaries():
    """The size list inside guard bytes, the table built from the fenced pointers inside fn; workspace and norm come from the hostile allocator."""
    for shifts in (shifts_aligned, shifts_mixed):
        table = Table(edge_sizes(), shifts(11), [t % 2 for t in range(11)])
        n = run_fenced(table.fn(1.0), lambda seed: table.make_state(seed, g_scale=3.0), in_place=("p", "m", "v", "steps"))
        assert n >= 2                                                       # norm_out and the workspace


# ------------------------------------------------------------------------------------------------ FusedAdamW
def _optimizers(params64):
    from mlx8_ws_audio_transformer_amd import FusedAdamW
    make = lambda: [torch.nn.Parameter(p.float().cuda()) for p in params64]
    groups = lambda ps: [dict(params=[ps[i] for i in range(len(ps)) if GROUP_OF[i] == g], **GROUPS[g]) for g in range(2)]
    pf, pt = make(), make()
    return (pf, FusedAdamW(groups(pf))), (pt, torch.optim.AdamW(groups(pt)))


def _set_grads(params, grads):
    for p, g in zip(params, grads):
        p.grad = None if g is None else g.float().cuda()


def _check_params(label, got, want64, torch32):
    failed = []
    for i, (g, w, t) in enumerate(zip(got, want64, torch32)):
        err, err32 = float((g.detach().double().cpu() - w).abs().max()), float((t.detach().double().cpu() - w).abs().max())
        bound = 4 * err32 + U * float(w.abs().max())
        print(f"  {label} parameter {i}: err {err:.3e}, torch fp32 {err32:.3e}, bound {bound:.3e}")
        if not err <= bound:
            failed.append((i, err, err32, bound))
    assert not failed, failed


def test_fused_adamw_beside_torch_adamw_and_state_dicts_both_ways():
    """The host test's schedule: 5 steps, two groups, lr halved after step 2, parameter 1 without a gradient in step 3.  At that step a torch optimizer
    takes over FusedAdamW's state dict and a FusedAdamW takes over torch's; both next steps agree with float64 as the uninterrupted ones do."""
    from mlx8_ws_audio_transformer_amd import FusedAdamW
    ref = ReferenceAdamW(schedule_params(), GROUP_OF, GROUPS)
    (pf, fused), (pt, torch_opt) = _optimizers(schedule_params())
    for step in range(5):
        if step == 2:
            for opt in (fused, torch_opt):
                for g in opt.param_groups:
                    g["lr"] *= 0.5
            for g in ref.groups:
                g["lr"] *= 0.5
            px = [torch.nn.Parameter(p.detach().clone()) for p in pf]      # torch takes over from fused ...
            x = torch.optim.AdamW([dict(params=[px[i] for i in range(4) if GROUP_OF[i] == g]) for g in range(2)])
            x.load_state_dict(copy.deepcopy(fused.state_dict()))             # state_dict() hands out references, as torch's does: a copy, as a saved file is
            py = [torch.nn.Parameter(p.detach().clone()) for p in pt]      # ... and fused from torch
            y = FusedAdamW([dict(params=[py[i] for i in range(4) if GROUP_OF[i] == g]) for g in range(2)])
            y.load_state_dict(copy.deepcopy(torch_opt.state_dict()))
            assert [g["lr"] for g in x.param_groups] == [g["lr"] for g in y.param_groups] == [5e-4, 1.5e-4]
        grads = schedule_grads(step)
        _set_grads(pf, grads)
        _set_grads(pt, grads)
        versions = [p._version for p in pf]
        norm = fused.step(max_norm=MAX_NORM)
        want_norm = torch.nn.utils.clip_grad_norm_(pt, MAX_NORM)
        torch_opt.step()
        n64, _ = ref.step(grads, MAX_NORM)
        rel = abs(float(norm) - float(want_norm)) / float(want_norm)
        print(f"step {step}: norm {float(norm):.7f}, torch {float(want_norm):.7f} ({rel / U:.2f} u), f64 {float(n64):.7f}")
        assert norm.is_cuda and norm.dim() == 0 and rel <= norm_rel() + 12 * U      # torch's own fp32 norm of <= 16-element tensors and of 4 norms: <= 12 u
        assert abs(float(norm) - float(n64)) <= norm_rel() * float(n64)
        _check_params(f"step {step}", pf, ref.params, pt)
        assert [p._version - v for p, v in zip(pf, versions)] == [0 if g is None else 1 for g in grads], "exactly the stepped parameters' versions move"
        assert all(same_bits(p.grad, g.float().cuda()) for p, g in zip(pf, grads) if g is not None), "the gradients keep their values"
        if step == 2:
            _set_grads(px, grads)
            _set_grads(py, grads)
            torch.nn.utils.clip_grad_norm_(px, MAX_NORM)
            x.step()
            y.step(max_norm=MAX_NORM)
            _check_params("torch on fused's state", px, ref.params, pt)
            _check_params("fused on torch's state", py, ref.params, pt)
            assert [float(y.state[p]["step"]) for p in py] == [3.0, 2.0, 3.0, 3.0] == [float(x.state[p]["step"]) for p in px]
    steps = [fused.state[p]["step"] for p in pf]
    assert [float(s) for s in steps] == [5.0, 4.0, 5.0, 5.0]
    assert all(s.is_cuda and s.untyped_storage().data_ptr() == steps[0].untyped_storage().data_ptr() for s in steps), "views of one device vector"
    assert set(fused.state[pf[0]]) == {"step", "exp_avg", "exp_avg_sq"}


def test_step_runs_under_sync_debug_error():
    """The first step (tables and state come into being), a step after a learning-rate change (the group table is sent again) and a step after a
    gradient moved (the tensor table is sent again): none synchronises."""
    (pf, fused), _ = _optimizers(schedule_params())
    _set_grads(pf, schedule_grads(0))
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        fused.step(max_norm=1.0)
        fused.param_groups[0]["lr"] *= 0.5
        fused.step(max_norm=1.0)
        before = fused._tensors.clone()
        pf[0].grad = pf[0].grad.clone()
        norm = fused.step()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert not torch.equal(before, fused._tensors) and float(fused.last_norm[1]) == 1.0 and float(norm) > 0
    assert float(fused._groups[0, 0]) == f32(5e-4)


def test_amsgrad_raises():
    from mlx8_ws_audio_transformer_amd import FusedAdamW
    with pytest.raises(ValueError, match="amsgrad"):
        FusedAdamW([torch.nn.Parameter(torch.zeros(4, device="cuda"))], amsgrad=True)


# ------------------------------------------------------------------------------------------------ the loop on the micro tied model (2 layers, K = 1)
def _micro():
    from tests.test_gpu_qwen3_train import _model
    model, (cfg, _, _, _) = _model(1)
    return model, cfg


def _dataset(cfg, n=6, L=37):
    items = []
    for i in range(n):
        ids = (torch.arange(L) * 29 + 3 + 7 * i) % cfg.vocab_size
        ids[5] = ids[1]                                                    # a repeated token
        items.append({"waveform": torch.zeros(8).numpy(), "sampling_rate": 16000, "input_ids": ids, "attention_mask": torch.ones(L, dtype=torch.long),
                      "filename": f"clip{i}"})
    return items


def test_the_loop_with_the_fused_optimizer_follows_the_loop_with_torchs():
    from mlx8_ws_audio_transformer_amd import FusedAdamW, train_music2midi
    out = {}
    for which in ("fused", "torch"):
        model, cfg = _micro()
        out[which] = train_music2midi(model, _dataset(cfg), _dataset(cfg, 2), epochs=2, batch_size=2, optimizer=which, log=lambda *_: None)
    assert isinstance(out["fused"]["optimizer"], FusedAdamW) and isinstance(out["torch"]["optimizer"], torch.optim.AdamW)
    for key in ("train_losses", "val_losses"):
        for a, b in zip(out["fused"][key], out["torch"][key]):
            print(f"{key}: fused {a:.6f} torch {b:.6f} ({abs(a - b) / abs(b):.3e} relative, tol 1e-3)")
            assert abs(a - b) <= 1e-3 * abs(b)
        assert len(out["fused"][key]) == len(out["torch"][key]) == 2
    assert out["fused"]["train_losses"][1] < out["fused"]["train_losses"][0]
    assert [float(out["fused"]["optimizer"].state[p]["step"]) for g in out["fused"]["optimizer"].param_groups for p in g["params"]] \
        == [6.0] * sum(len(g["params"]) for g in out["fused"]["optimizer"].param_groups)


def test_a_step_repacks_exactly_the_handles_of_stepped_parameters():
    from mlx8_ws_audio_transformer_amd import collate_fn, setup_optimizers
    from mlx8_ws_audio_transformer_amd.music2midi_train import train_step
    from mlx8_ws_audio_transformer_amd.native_decoder import PackedLinear
    model, cfg = _micro()
    opt = setup_optimizers(model, log=lambda *_: None)
    batch = collate_fn(_dataset(cfg, 2))
    updated, update = [], PackedLinear.update
    PackedLinear.update = lambda self, w, b: (updated.append(id(self)), update(self, w, b))[1]
    try:
        for step in range(2):
            train_step(model, opt, batch)
            del updated[:]
            pk = model.text_decoder._pack()                                # what the next forward does
            live = {id(pk["layers"][1][k]) for k in ("qkv", "o", "gu", "down")} | {id(pk["lm_head"])}
            frozen = {id(pk["layers"][0][k]) for k in ("qkv", "o", "gu", "down")}
            assert sorted(updated) == sorted(live) and not frozen & set(updated), "one re-pack per handle made of a stepped parameter, none else"
    finally:
        PackedLinear.update = update


def test_resuming_from_a_checkpoint_continues_bit_for_bit(tmp_path):
    from mlx8_ws_audio_transformer_amd import collate_fn, load_checkpoint, save_checkpoint, setup_optimizers
    from mlx8_ws_audio_transformer_amd.music2midi_train import train_step
    model, cfg = _micro()
    opt = setup_optimizers(model, log=lambda *_: None)
    batches = [collate_fn(_dataset(cfg)[i:i + 2]) for i in (0, 2, 4, 0)]
    for b in batches[:2]:
        train_step(model, opt, b)
    path = save_checkpoint(model, opt, 1, 0.0, str(tmp_path))
    want = [float(train_step(model, opt, b)) for b in batches[2:]]

    fresh, _ = _micro()
    with torch.no_grad():
        for p in fresh.parameters():
            if p.requires_grad:
                p.mul_(1.5)                                                # what the checkpoint has to put right
    fresh_opt = setup_optimizers(fresh, log=lambda *_: None)
    assert load_checkpoint(fresh, fresh_opt, path) == (1, 0.0)
    got = [float(train_step(fresh, fresh_opt, b)) for b in batches[2:]]
    print(f"uninterrupted {want}, resumed {got}")
    assert got == want, "the step after the resume (parameters) and the one after it (optimizer state) are the uninterrupted run's bits"
