"""GPU: what every fp32 row operator returns when an operand is NaN, infinite, huge, tiny or -0 (tests/extreme_values.py: the cases, the restatements
and the comparison; tests/test_extreme_values_host.py checks those on the CPU), and that the operators whose rows or clips are independent keep a NaN
where it belongs: every output that does not depend on the poisoned row or clip has the clean run's bits.

Propagation: the class (NaN, +inf, -inf, finite) of every output element against the fp32 restatement, the value of every element fp32 can reach against
fp64 within the operator's own bound.  Containment: bit-identity outside the dependent region, and NaN inside it (a NaN must not be hidden either).
Every operand is a valid fp32 tensor of a valid shape: non-finite values are data here, not addresses."""
import pytest
import torch

from tests import extreme_values as ev
from tests.extreme_values import INF, NAN, assert_contained, assert_same_class, variates

pytestmark = pytest.mark.gpu

CASES = ev.cases()


def _cuda(operands):
    return {k: v.cuda() for k, v in operands.items()}


# ------------------------------------------------------------------------------------------------------------------- propagation: one runner per operator
def run_gelu(o, m):
    from mlx8_ws_audio_transformer_amd import native_decoder as nd
    return {"y": nd.gelu(o["x"]), "dx": nd.gelu_backward(o["x"], o["dy"])}


def run_layernorm(o, m):
    from mlx8_ws_audio_transformer_amd import native_decoder as nd, ops
    dg, db = nd.layernorm_param_grad(o["dy"], o["x"])
    return {"y": ops.layernorm(o["x"], o["g"], o["b"]), "dx": nd.layernorm_backward(o["dy"], o["x"], o["g"]),
            "dx_dres": nd.layernorm_backward(o["dy"], o["x"], o["g"], dres=o["dres"]), "dgamma": dg, "dbeta": db}


def run_rmsnorm(o, m):
    from mlx8_ws_audio_transformer_amd import ops
    M, d = o["x"].shape
    x, dy = (o["x"], 0), (o["dy"], 0)
    return {"y": ops.rmsnorm(x, d, o["g"], M, d, ev.RMS_EPS),
            "dx": ops.rmsnorm_backward(dy, d, x, d, o["g"], M, d, ev.RMS_EPS, dx=(torch.empty_like(o["x"]), 0), lddx=d),
            "dx_dres": ops.rmsnorm_backward(dy, d, x, d, o["g"], M, d, ev.RMS_EPS, dres=(o["dres"], 0), dx=(torch.empty_like(o["x"]), 0), lddx=d),
            "dgamma": ops.rmsnorm_param_grad(dy, d, x, d, M, d, ev.RMS_EPS)}


def run_silu(o, m):
    from mlx8_ws_audio_transformer_amd import ops
    M, I = o["dy"].shape
    return {"y": ops.silu_mul((o["gu"], 0), 2 * I, M, I), "dgu": ops.silu_mul_backward((o["gu"], 0), 2 * I, (o["dy"], 0), I, M, I)}


def run_qk_norm_rope(o, m):
    from mlx8_ws_audio_transformer_amd import ops
    B, Lq, Hq, Hkv, Tmax = m["B"], m["Lq"], m["Hq"], m["Hkv"], m["Tmax"]
    rows, wq, wkv = B * Lq, Hq * 128, Hkv * 128
    q = torch.full((rows, wq), NAN, device="cuda")
    kc, vc = torch.full((B, Tmax, wkv), NAN, device="cuda"), torch.full((B, Tmax, wkv), NAN, device="cuda")
    pos = m["positions"].to(torch.int32).cuda()
    ops.qk_norm_rope((o["qkv"], 0), wq + 2 * wkv, o["qg"], o["kg"], o["cos"], o["sin"], pos, (q, 0), wq, (kc, 0), (vc, 0), wkv, Tmax * wkv, B, Lq, Hq, Hkv, ev.RMS_EPS)
    live = m["positions"].tolist()                         # B = 1: row i of the call lands at cache position positions[i]
    return {"q": q, "k": kc[0, live], "v": vc[0, live]}


def run_softmax(o, m):
    from mlx8_ws_audio_transformer_amd import native_decoder as nd
    cols = m["cols"]
    p = nd.softmax_rows(o["s"].clone(), cols, m["scale"])
    ds = nd.softmax_rows_backward(p.clone(), o["dp"].clone(), cols, m["scale"])
    for name, t, src in (("p", p, o["s"]), ("ds", ds, o["dp"])):                                   # both in place: the padding columns keep their (NaN) bits
        assert_contained(t, src, torch.arange(t.shape[1]) < cols, f"softmax {name}: padding columns")
    return {"p": p[:, :cols], "ds": ds[:, :cols]}


def run_cross_entropy(o, m):
    from mlx8_ws_audio_transformer_amd import native_decoder as nd
    vocab = m["vocab"]
    loss, dlogits = nd.cross_entropy(o["logits"], o["labels"], vocab)
    assert bool((dlogits[:, vocab:] == 0).all()), "cross_entropy: the padding columns of dlogits are zero whatever the logits' padding holds"
    return {"loss": loss.reshape(1, 1), "dlogits": dlogits[:, :vocab]}


def run_column_sums(o, m):
    from mlx8_ws_audio_transformer_amd import native_decoder as nd
    return {"sums": nd.column_sums(o["a"])}


def run_column_sums_ld(o, m):
    from mlx8_ws_audio_transformer_amd import native_decoder as nd
    return {"sums": nd.column_sums_ld(o["a"], m["col"], m["width"])}


def run_embed(o, m):
    from mlx8_ws_audio_transformer_amd import native_decoder as nd
    return {"x": nd.embed(o["ids"], o["tok"], o["pos"], m["pos0"])}


RUN = {"gelu": run_gelu, "layernorm": run_layernorm, "rmsnorm": run_rmsnorm, "silu": run_silu, "qk_norm_rope": run_qk_norm_rope, "softmax": run_softmax,
       "cross_entropy": run_cross_entropy, "column_sums": run_column_sums, "column_sums_ld": run_column_sums_ld, "embed": run_embed}


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_propagation(case):
    got = RUN[case.op](_cuda(case.operands), case.meta)
    ev.check(case, got)


def test_gelu_pins_the_infinite_ends():
    """gelu(+inf) = +inf with slope 1; gelu(-inf) and its slope are NaN as in torch (a -inf pre-activation is an overflow that must surface); NaN stays NaN;
    a large negative finite x gives zero."""
    case = next(c for c in CASES if c.op == "gelu")
    got = {k: v.cpu() for k, v in run_gelu(_cuda(case.operands), case.meta).items()}
    i = {s: n for n, s in enumerate(ev.SPECIALS)}
    y, dx, dy = got["y"], got["dx"], case.operands["dy"]
    assert y[i["+inf"]].item() == INF, f"gelu(+inf) = {y[i['+inf']].item()!r} at element {i['+inf']}"
    assert dx[i["+inf"]].item() == dy[i["+inf"]].item(), "gelu_backward(+inf, dy) = dy"
    assert torch.isnan(y[i["-inf"]]) and torch.isnan(dx[i["-inf"]]) and torch.isnan(y[i["nan"]]) and torch.isnan(dx[i["nan"]])
    x = case.operands["x"]
    for s in ("+fltmax", "+1e20"):                                                                  # the identity far out, slope exactly 1
        assert y[i[s]].item() == x[i[s]].item() and dx[i[s]].item() == dy[i[s]].item(), s
    for s in ("-fltmax", "-1e20"):                                                                  # zero far out on the other side, slope 0
        assert y[i[s]].item() == 0.0 and dx[i[s]].item() == 0.0, s


def test_softmax_zeros_are_exact():
    from mlx8_ws_audio_transformer_amd import native_decoder as nd
    case = next(c for c in CASES if c.name == "softmax-70in72")
    p = nd.softmax_rows(case.operands["s"].cuda(), 70, 0.125).cpu()
    assert_same_class(p[2, [0, 33, 69]], torch.zeros(3), "softmax: the -inf columns of row 2", signs=True)


def test_qk_norm_rope_special_stays_in_its_head():
    clean = next(c for c in CASES if c.name == "qk_norm_rope-clean")
    base = {k: v.cpu() for k, v in run_qk_norm_rope(_cuda(clean.operands), clean.meta).items()}
    for case in (c for c in CASES if c.op == "qk_norm_rope" and c.meta["head"] is not None):
        got = run_qk_norm_rope(_cuda(case.operands), case.meta)
        head = case.meta["head"]
        for name, first in (("q", 0), ("k", clean.meta["Hq"]), ("v", clean.meta["Hq"] + clean.meta["Hkv"])):
            touched = torch.zeros(base[name].shape, dtype=torch.bool)
            if first <= head < first + base[name].shape[1] // 128:
                touched[0, 128 * (head - first):128 * (head - first + 1)] = True                     # row 0, the planted head
            assert_contained(got[name].cpu(), base[name], touched, f"{case.name}: {name}")


def test_embed_special_reaches_only_the_positions_that_name_its_row():
    clean = {"ids": torch.tensor([[2, 0, 2]]), "tok": variates("embed.tok", (4, 128)), "pos": variates("embed.pos", (5, 128))}
    base = run_embed(_cuda(clean), {"pos0": 1})["x"].cpu()
    for case in (c for c in CASES if c.op == "embed"):
        touched = torch.tensor([True, False, True])[:, None]
        assert_contained(run_embed(_cuda(case.operands), case.meta)["x"].cpu(), base, touched, case.name)


# ------------------------------------------------------------------------------------------------------------------- BatchNorm + ReLU + pooling
BN = ev.BN


def _bn_run(x, g, b, pool, dy=None):
    from mlx8_ws_audio_transformer_amd import cnn_classifier as cc
    B, T = BN["B"], BN["T"]
    x, g, b, dy = x.cuda(), g.cuda(), b.cuda(), (ev.bn_dy(pool) if dy is None else dy).cuda()
    mean, var = cc.batchnorm_stats(x)
    y = cc.bn_relu_pool(x, mean, var, g, b, ev.BN_EPS, B, T, pool)
    dx, dg, db = cc.bn_relu_pool_backward(dy, x, mean, var, g, b, ev.BN_EPS, B, T, pool)
    return {"mean": mean, "var": var, "y": y, "dx": dx, "dgamma": dg, "dbeta": db}


def run_batchnorm(o, m):
    return _bn_run(o["x"], o["g"], o["b"], m["pool"], o["dy"])


RUN["batchnorm"] = run_batchnorm


@pytest.mark.parametrize("pool", [0, 2, 4, 5])
@pytest.mark.parametrize("poison", ["nan", "+inf", "-inf"])
def test_batchnorm_poisoned_channel_stays_alone(pool, poison):
    """One non-finite value in channel 7: the other 127 channels of the statistics, the forward and the backward have the clean run's bits; channel 7's
    statistics, output and input gradient are NaN (torch's batch_norm + relu + pooling gives the same: relu(NaN) = NaN)."""
    clean = _bn_run(*ev.bn_state(), pool)
    got = _bn_run(*ev.bn_state(ev.SPECIALS[poison]), pool)
    touched = torch.arange(BN["C"]) == BN["poisoned"]
    for k in clean:
        assert_contained(got[k], clean[k], touched, f"pool {pool}, {poison} in channel {BN['poisoned']}: {k}")
    for k in ("mean", "var", "y", "dx", "dgamma"):
        col = got[k].cpu().reshape(-1, BN["C"])[:, BN["poisoned"]]
        assert_same_class(col, torch.full_like(col, NAN), f"pool {pool}, {poison}: channel {BN['poisoned']} of {k}")


def test_batchnorm_constant_channel_is_exact():
    """The values of every channel in every pool mode are test_propagation[batchnorm-pool*]; beyond its bound, a constant channel has variance exactly 0 and
    its own value as the mean (the first-row mean and chan_merge are exact for equal values)."""
    got = _bn_run(*ev.bn_state(), 2)
    c = BN["constant"]
    assert got["var"][c].item() == 0.0 and got["mean"][c].item() == torch.tensor(1.7).item()


# ------------------------------------------------------------------------------------------------------------------- containment
def _nan_rows(t, rows):
    assert bool(torch.isnan(t.cpu().reshape(t.shape[0], -1)[rows]).all()), "the poisoned rows' outputs must be NaN: a NaN operand may not be hidden"


@pytest.mark.parametrize("precision", ["bf16x3", "bf16", "fp16x3", "f16f8"])
def test_linear_contains_a_nan_row(precision):
    """M = 130 against the 64-row tile: the NaN row on both sides of the first tile edge, first and in the ragged tail."""
    from mlx8_ws_audio_transformer_amd import ops
    M, N, K = 130, 128, 64
    x, w, b = variates("lin.x", (M, K)), variates("lin.w", (N, K), K ** -0.5).cuda(), variates("lin.b", (N,)).cuda()
    clean = ops.linear(x.cuda(), w, b, precision)
    for row in (0, 63, 64, 129):
        got = ops.linear(ev.plant(x, NAN, row).cuda(), w, b, precision)
        assert_contained(got, clean, (torch.arange(M) == row)[:, None], f"linear {precision}, NaN row {row}")
        _nan_rows(got, [row])


@pytest.mark.parametrize("decode", [False, True])
def test_packed_linear_contains_a_nan_row(decode):
    from mlx8_ws_audio_transformer_amd import native_decoder as nd
    M, N, K = 3, 200, 64
    pl = nd.PackedLinear(variates("pl.w", (N, K), 0.1).cuda(), variates("pl.b", (N,)).cuda(), "bf16x3", backward=False)
    x = variates("pl.x", (M, K))
    fwd = pl.forward_decode if decode else pl.forward
    clean, got = fwd(x.cuda()), fwd(ev.plant(x, NAN, 1).cuda())
    assert_contained(got, clean, torch.tensor([False, True, False])[:, None], f"PackedLinear decode={decode}")
    _nan_rows(got[:, :N], [1])


def test_bmm_contains_a_nan_batch_member():
    from mlx8_ws_audio_transformer_amd import native_decoder as nd
    batch, M, N, K = 3, 10, 64, 64
    a, pb = variates("bmm.a", (batch, M, K)), nd.PackedBatch(variates("bmm.b", (batch, N, K), K ** -0.5).cuda())

    def run(a):
        out = torch.full((batch, M, N), 7.0, device="cuda")
        nd.bmm((a.cuda(), 0, K, M * K), pb, M, (out, 0, N, M * N))
        return out
    clean, got = run(a), run(ev.plant(a, NAN, 1))
    assert_contained(got, clean, torch.tensor([False, True, False])[:, None, None], "bmm, NaN batch member 1")
    _nan_rows(got, [1])


def _poison_clip(t, clip):
    return ev.plant(t, NAN, clip)


def test_attention_contains_a_nan_clip():
    from mlx8_ws_audio_transformer_amd import ops
    B, H, S = 2, 2, 70
    q, k, v = variates("att.q", (B, H, S, 64), 0.35), variates("att.k", (B, H, S, 64)), variates("att.v", (B, H, S, 64))
    clean = ops.attention(q.cuda(), k.cuda(), v.cuda())
    for name, args in (("q", (_poison_clip(q, 1), k, v)), ("k", (q, _poison_clip(k, 1), v))):
        got = ops.attention(*(t.cuda() for t in args))
        assert_contained(got, clean, torch.tensor([False, True])[:, None, None], f"attention, NaN {name} of clip 1")
        _nan_rows(got, [1])


def test_attention_small_contains_a_nan_clip():
    from mlx8_ws_audio_transformer_amd import native_decoder as nd
    B, H, Lq, Sk = 2, 2, 17, 70
    d = H * 64
    q, k, v = variates("small.q", (B, Lq, d), 1.7), variates("small.k", (B, Sk, d), 1.7), variates("small.v", (B, Sk, d))

    def run(q, k):
        o, lse = nd.attention_small((q.reshape(-1, d).cuda(), 0), d, (k.reshape(-1, d).cuda(), 0), d, (v.reshape(-1, d).cuda(), 0), d, B, H, Lq, Sk, False, 0)
        return o.reshape(B, Lq, d), lse
    clean = run(q, k)
    for name, args in (("q", (_poison_clip(q, 1), k)), ("k", (q, _poison_clip(k, 1)))):
        got = run(*args)
        for what, g, c in zip(("o", "lse"), got, clean):
            assert_contained(g, c, torch.tensor([False, True]).reshape(2, 1, 1), f"attention_small, NaN {name} of clip 1: {what}")
            _nan_rows(g, [1])


def test_cross_attention_contains_a_nan_clip():
    from mlx8_ws_audio_transformer_amd import ops
    B, H, Lq, Sk = 2, 1, 5, 70
    d = H * 128
    q, k, v = variates("cross.q", (B, Lq, d), 1.7), variates("cross.k", (B, Sk, d), 1.7), variates("cross.v", (B, Sk, d))

    def run(q, k):
        o, lse = ops.cross_attention((q.reshape(-1, d).cuda(), 0), d, (k.reshape(-1, d).cuda(), 0), d, (v.reshape(-1, d).cuda(), 0), d, B, H, Lq, Sk)
        return o.reshape(B, Lq, d), lse
    clean = run(q, k)
    for name, args in (("q", (_poison_clip(q, 1), k)), ("k", (q, _poison_clip(k, 1)))):
        got = run(*args)
        for what, g, c in zip(("o", "lse"), got, clean):
            assert_contained(g, c, torch.tensor([False, True]).reshape(2, 1, 1), f"cross_attention, NaN {name} of clip 1: {what}")
            _nan_rows(g, [1])


def test_causal_attention_contains_a_nan_clip_and_a_nan_key_position():
    """Also the causal mask: a NaN key at position j is masked for the query rows < j, which keep the clean run's bits; the rows >= j are NaN."""
    from mlx8_ws_audio_transformer_amd import ops
    B, Hq, Hkv, L = 2, 2, 1, 20
    wq, wkv = Hq * 128, Hkv * 128
    q, k, v = variates("causal.q", (B, L, wq), 1.7), variates("causal.k", (B, L, wkv), 1.7), variates("causal.v", (B, L, wkv))

    def run(q, k):
        return ops.causal_attention((q.reshape(-1, wq).cuda(), 0), wq, (k.cuda(), 0), (v.cuda(), 0), wkv, L * wkv, B, Hq, Hkv, L, L).reshape(B, L, wq)
    clean = run(q, k)
    for name, args in (("q", (_poison_clip(q, 1), k)), ("k", (q, _poison_clip(k, 1)))):
        got = run(*args)
        assert_contained(got, clean, torch.tensor([False, True]).reshape(2, 1, 1), f"causal_attention, NaN {name} of clip 1")
        _nan_rows(got, [1])
    j = 12
    got = run(q, ev.plant(k, NAN, 0, j))
    touched = torch.zeros(B, L, 1, dtype=torch.bool)
    touched[0, j:] = True
    assert_contained(got, clean, touched, f"causal_attention, NaN key at position {j} of clip 0")
    assert bool(torch.isnan(got[0, j:]).all()), "the query rows that see the NaN key must be NaN"


def test_weight_grad_contains_a_nan_column():
    """A NaN in column n of dy makes row n of dW NaN and no other row."""
    from mlx8_ws_audio_transformer_amd import ops
    M, N, K, n = 40, 128, 128, 5
    dy, x = variates("wgrad.dy", (M, N)), variates("wgrad.x", (M, K)).cuda()
    clean, got = ops.weight_grad(dy.cuda(), x), ops.weight_grad(ev.plant(dy, NAN, 17, n).cuda(), x)
    assert_contained(got, clean, (torch.arange(N) == n)[:, None], f"weight_grad, NaN in column {n} of dy")
    _nan_rows(got, [n])


# ------------------------------------------------------------------------------------------------------------------- the GELU epilogue of the GEMM
@pytest.mark.parametrize("terms", [1, 3])
def test_fused_gelu_epilogue_of_an_overflowing_pre_activation(terms):
    """Row 3 of x and row 5 of w hold 1e20 over K = 64: the pre-activation (3, 5) overflows fp32 to +inf, and gelu(+inf) = +inf in the fp32 output form
    (EPI_F32_GELU_POS, a zero positional table) and in the bf16 plane form (EPI_BF16_GELU), where +inf is the plane's saturated value.  Its neighbours in
    row 3 and column 5 are +-1e20-sized pre-activations: finite, and gelu of them x or -0.
    bf16 operand planes only: 1e20 is outside fp16, whose operand split already turns it into inf - inf (see below)."""
    from mlx8_ws_audio_transformer_amd import ops
    M, N, K = 64, 128, 64
    x, w = variates("epi.x", (M, K), 0.5), variates("epi.w", (N, K), K ** -0.5)
    x[3], w[5] = 1e20, 1e20
    pre = x.double() @ w.double().t()
    want_class = torch.nn.functional.gelu(pre).float()                                             # finite everywhere but at (3, 5)
    want_class[3, 5] = INF
    out = {"f32": torch.full((M, N), NAN, device="cuda")}
    ops.linear_fused(x.cuda(), w.cuda(), None, "gelu_pos", terms, out, pos=torch.zeros((M, N), device="cuda"), rows_pos=M)
    y = out["f32"].cpu()
    assert y[3, 5].item() == INF, f"terms {terms}: EPI_F32_GELU_POS at (3, 5), pre-activation +inf: {y[3, 5].item()!r}"
    assert_same_class(y, want_class, f"terms {terms}: EPI_F32_GELU_POS")
    planes = {"hi": torch.zeros((M, N), dtype=torch.bfloat16, device="cuda")}
    if terms == 3:
        planes["lo"] = torch.zeros((M, N), dtype=torch.bfloat16, device="cuda")
    ops.linear_fused(x.cuda(), w.cuda(), None, "gelu", terms, planes)
    hi = planes["hi"].float().cpu()
    assert hi[3, 5].item() == INF, f"terms {terms}: EPI_BF16_GELU hi plane at (3, 5), pre-activation +inf: {hi[3, 5].item()!r}"
    assert_same_class(hi, want_class, f"terms {terms}: EPI_BF16_GELU hi plane")
    if terms == 3:
        # Known defect (the non-finite contract): split_bf16 forms lo = x - hi, which is inf - inf = NaN for an infinite x, so the pair's sum is
        # NaN although its hi plane is right.  Pinned as it is; every finite element's lo is finite.
        lo = planes["lo"].float().cpu()
        assert torch.isnan(lo[3, 5]), "the lo plane of an infinite value (lo = x - hi): NaN today"
        lo[3, 5] = 0.0
        assert bool(torch.isfinite(lo).all())


def test_fused_gelu_epilogue_fp16_plane_of_an_infinite_pre_activation():
    """The single-plane fp16 form (terms 2): 1e20 is +inf in the fp16 operand planes, so the pre-activation (3, 5) is a sum of inf * inf = +inf, and the output
    plane holds +inf there -- activations are not clamped to 65504 (only the gradient planes saturate), an overflow stays visible.  The rest of row 3 and
    column 5 mixes +inf and -inf terms and is not asserted; the split formats (terms 4, 5) meet the lo = x - hi defect at the operand split already."""
    from mlx8_ws_audio_transformer_amd import ops
    M, N, K = 64, 128, 64
    x, w = variates("epi.x", (M, K), 0.5), variates("epi.w", (N, K), K ** -0.5)
    x[3], w[5] = 1e20, 1e20
    planes = {"hi": torch.zeros((M, N), dtype=torch.float16, device="cuda")}
    ops.linear_fused(x.cuda(), w.cuda(), None, "gelu", 2, planes)
    hi = planes["hi"].float().cpu()
    assert hi[3, 5].item() == INF, f"terms 2: EPI_BF16_GELU fp16 plane at (3, 5), pre-activation +inf: {hi[3, 5].item()!r}"
    rest = hi.clone()
    rest[3], rest[:, 5] = 0.0, 0.0
    assert bool(torch.isfinite(rest).all()), "terms 2: an element outside row 3 and column 5 is not finite"
