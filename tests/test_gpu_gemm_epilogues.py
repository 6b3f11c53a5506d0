"""GPU: every fused epilogue of the GEMM on every kernel that has it -- gemm_kernel on its three tiles, gemm_f8_kernel on its two, gemm_f8s_kernel,
gemm_pp_kernel (csrc/gemm.hip, csrc/gemm_pp.h) -- one launch at a time through awt_op_linear_fused, against float64 (tests/gemm_reference.py).

Per launch: every output buffer is pre-filled with a sentinel byte and carries a guard band (256 rows after a row-major output, one whole plane stride after
the q | k | v planes); rows >= M, columns >= n_valid and the band must come back unchanged, so a failed store mask is a failed assertion, not an access
outside the allocation.  The raw bytes are decoded in Python (gemm_reference's decoders) and each output tensor must satisfy
    max |kernel - exact| <= 4 x (max |rounded - exact| + max |rounded32 - rounded|)
with the right side computed from the reference alone; error and bound are printed side by side, and each test ends with a RATIO line per epilogue and
kernel (worst error / bound), the source of DESIGN.md's table.  The library does not report the kernel a launch took, so `route` restates the launcher's
rule (launch_epi / pick_tile of gemm.hip, the ping-pong rule of awt_op_linear_fused) and every test asserts the kernel it means to run."""
import collections

import pytest
import torch

from tests import gemm_reference as ref
from tests.test_gpu_ops import TOL
from tests.util import tuning

pytestmark = pytest.mark.gpu

SENT, GUARD_ROWS, ERR_INVALID, ERR_WORKSPACE = 0x5A, 256, -1, -3
Q_SCALE = 0.125 * 1.4426950408889634
PRECISION = {1: "bf16", 2: "fp16", 3: "bf16x3", 4: "fp16x3", 5: "f16f8"}
MS = (1, 127, 128, 129, 200, 256, 257, 300)
NKS = ((128, 64), (256, 192), (384, 128), (768, 768))
ROW_EPILOGUES = ("f32", "f32_resid", "planes", "gelu", "gelu_pos", "gelu_save", "dgelu")
PP_EPILOGUES = ("f32", "f32_resid", "planes", "gelu")                                   # and "qkv": test_qkv
F8_EXP = {"q": ref.F8_Q, "k": ref.F8_KV, "v": ref.F8_KV}


# ---------------------------------------------------------------- the launcher's rule, restated
def route(terms, M, N, K, nseg=1, exact=False, tile=0, mfma16=1, pp=1, plain=True):
    """The kernel a launch of M rows (or of m_pick rows) takes."""
    ceil = lambda a, b: (a + b - 1) // b
    if terms == 5:
        if pp == 2 and plain and nseg == 1 and N % 256 == 0 and K >= 128:
            return "pp"
        n256 = ceil(N, 256) * 256
        f8s_ok = bool(mfma16) and nseg == 1 and not exact and (N % 256 == 0 or n256 * 3 <= N * 4)
        t = tile or (256 if (N % 256 == 0 or f8s_ok) and ceil(M, 128) * ((n256 if f8s_ok else N) // 256) >= 512 else 128)
        if t == 256 and f8s_ok:
            return "f8s"
        form = "_multi" if nseg > 1 else ("_wx" if exact else "")
        return ("f8_128x256" if t == 256 and N % 256 == 0 else "f8_128x128") + form
    t = tile or (256 if N % 256 == 0 and ceil(M, 128) * (N // 256) >= 512 else (128 if ceil(M, 128) * (N // 128) >= 512 else 64))
    t = 128 if t == 256 and N % 256 else t
    return f"gemm{t}" + ("_wx" if terms == 4 and nseg == 1 and exact else "")


# ---------------------------------------------------------------- one launch
def _sent(nbytes):
    return torch.full((int(nbytes),), SENT, dtype=torch.uint8, device="cuda")


def _dev(p):
    if not hasattr(p, "dev"):
        p.dev = (p.x.cuda(), p.w.cuda(), None if p.bias is None else p.bias.cuda())
    return p.dev


Launch = collections.namedtuple("Launch", "out epi terms M N nv S H skip_v8 split_lines ld")


def launch(p, epi, terms, knobs=None, side=None, n_valid=0, m_pick=0, split_lines=False, skip_v8=False, inplace=False, hi8=True, pre=(None, None), M=None, ldo=0):
    """One awt_op_linear_fused call on problem p into sentinel-filled, guard-banded buffers; `side` as the reference takes it (pre: the raw planes instead)."""
    from mlx8_ws_audio_transformer_amd import ops
    side = dict(side or {})
    x, w, bias = _dev(p)
    M, N, f8, three = (p.M if M is None else M), p.N, terms == 5, ref.PRODUCTS[terms] == 3
    S, H, ld = side.get("S", 0), side.get("H", 0), ldo or N                   # ld: the pitch of row-major outputs and side inputs
    rows, out = M + GUARD_ROWS, {}
    if epi in ref.F32_EPILOGUES:
        out["f32"] = _sent(rows * ld * 4)
    elif split_lines:
        out["ilv"] = _sent(rows * ld * 4)
    else:
        elems = 4 * M * H * 64 if epi == "qkv" else rows * ld
        out["hi"] = _sent(elems * 2)
        if f8:
            out["lo8"] = _sent(elems)
            if hi8:
                out["hi8"] = _sent(elems)
        elif three:
            out["lo"] = _sent(elems * 2)
    if epi == "gelu_save":
        out["hi2"] = _sent(rows * ld * 2)
        if three:
            out["lo2"] = _sent(rows * ld * 2)
    resid = side.get("resid")
    if resid is not None:
        resid = resid.float().cuda()
        if inplace:
            out["f32"].view(torch.float32)[:M * ld] = resid.flatten()
            resid = out["f32"].view(torch.float32)
    pos = side.get("pos")
    with tuning(**(knobs or {})):
        ops.linear_fused(x, w, bias, epi, terms, out, M=M, segs=p.segs, resid=resid, pos=None if pos is None else pos.float().cuda(),
                         rows_pos=side.get("rows_pos", 0), pre=pre, scale=side.get("scale", 1.0), S=S, H=H, skip_v8=skip_v8, n_valid=n_valid, m_pick=m_pick,
                         split_lines=split_lines, ldo=ldo)
    torch.cuda.synchronize()
    return Launch(out, epi, terms, M, N, n_valid or N, S, H, skip_v8, split_lines, ld)


def untouched(r):
    """Rows >= M, columns >= n_valid and the guard band still hold the sentinel."""
    for key, buf in r.out.items():
        el = {"f32": 4, "ilv": 4, "hi8": 1, "lo8": 1}.get(key, 2)
        if r.epi == "qkv" and key in ("hi", "lo", "hi8", "lo8"):
            plane = r.M * r.H * 64 * el
            assert bool((buf[3 * plane:] == SENT).all()), f"{key}: a store beyond the three planes"
            if r.skip_v8 and key in ("hi8", "lo8"):
                assert bool((buf[2 * plane:3 * plane] == SENT).all()), f"{key}: skip_v8 must leave v's e4m3 images alone"
            continue
        t = buf.view(r.M + GUARD_ROWS, r.ld * el)
        assert bool((t[r.M:] == SENT).all()), f"{key}: a store to a row >= M"
        assert bool((t[:r.M, r.nv * el:] == SENT).all()), f"{key}: a store to a column >= n_valid"


def raw_planes(r):
    """The bytes the launch wrote, per plane and restricted to [0, M) x [0, n_valid), on the CPU; split lines are de-interleaved into their three planes."""
    if r.split_lines:
        b16, b8, bl8 = ref.split_lines(r.out["ilv"][:r.M * r.N * 4].cpu(), r.M, r.N)
        return {"hi": b16, "hi8": b8, "lo8": bl8}
    res = {}
    for key, buf in r.out.items():
        el = {"f32": 4, "hi8": 1, "lo8": 1}.get(key, 2)
        if r.epi == "qkv" and key in ("hi", "lo", "hi8", "lo8"):
            res[key] = buf[:3 * r.M * r.H * 64 * el].cpu().view(3, -1)
        else:
            res[key] = buf[:r.M * r.ld * el].cpu().view(r.M, r.ld * el)[:, :r.nv * el].contiguous()
    return res


def decode(r):
    """The launch's outputs as float64 tensors under the reference's names."""
    raw, fp16, f8 = raw_planes(r), r.terms in (2, 4, 5), r.terms == 5
    res = {}
    if "f32" in raw:
        return {"y": raw["f32"].view(torch.float32).double()}
    names = ("q", "k", "v") if r.epi == "qkv" else ("y",)
    for i, name in enumerate(names):
        pick = (lambda key: raw[key][i]) if r.epi == "qkv" else (lambda key: raw[key])
        shape = (r.M // r.S, r.H, r.S, 64) if r.epi == "qkv" else (r.M, r.nv)
        s = F8_EXP.get(name, ref.F8_ACT)
        v = ref.planes16(pick("hi"), fp16)
        if f8:
            if not (name == "v" and r.skip_v8):
                v = v + ref.e4m3(pick("lo8"), s + ref.F8_LO).reshape(v.shape)
                if "hi8" in raw:
                    res[name + "_hi8"] = ref.e4m3(pick("hi8"), s).reshape(shape)
        elif "lo" in raw:
            v = v + ref.planes16(pick("lo"), fp16)
        res[name] = v.reshape(shape)
    if "hi2" in raw:
        res["pre"] = ref.planes16(raw["hi2"], False) + (ref.planes16(raw["lo2"], False) if "lo2" in raw else 0.0)
    return res


def same_bytes(a, b, rows=None):
    """Two launches wrote the same bytes (the first `rows` rows of row-major outputs)."""
    ra, rb = raw_planes(a), raw_planes(b)
    assert set(ra) == set(rb)
    return all(torch.equal(ra[k][:rows], rb[k][:rows]) for k in ra)


class Worst:
    """Worst error / bound per (epilogue, kernel, output); printed as the RATIO lines."""
    def __init__(self):
        self.r = {}

    def add(self, epi, kernel, ratios):
        for name, v in ratios.items():
            self.r[(epi, kernel, name)] = max(self.r.get((epi, kernel, name), 0.0), v)

    def report(self, label):
        for (epi, kernel, name), v in sorted(self.r.items()):
            print(f"RATIO {label} {epi} {kernel} {name} {v:.3f}")


def side_inputs(p, epi, seed=7):
    """Seeded side inputs of a row-major epilogue on problem p, as the reference takes them (dgelu's `pre` as the value of a bf16 pair)."""
    g = torch.Generator().manual_seed(seed)
    if epi == "f32_resid":
        return {"resid": torch.randn((p.M, p.N), generator=g)}
    if epi == "gelu_pos":
        return {"pos": torch.randn((50, p.N), generator=g), "rows_pos": 50}
    if epi == "dgelu":
        return {"pre": torch.randn((p.M, p.N), generator=g) * 1.5}
    if epi == "planes":
        return {"scale": 0.75}
    return {}


def pre_planes(pre, three):
    """(reference value, raw (hi, lo) device planes) of a saved pre-activation."""
    hi = pre.float().bfloat16()
    lo = (pre.float() - hi.float()).bfloat16()
    value = hi.double() + (lo.double() if three else 0.0)
    return value, (hi.cuda(), lo.cuda() if three else None)


class Identities:
    """Bit identities between launches, collected so that one test run reports all of them."""
    def __init__(self):
        self.broken = []

    def same(self, a, b, what, rows=None):
        if not same_bytes(a, b, rows):
            self.broken.append(what)

    def done(self):
        assert not self.broken, self.broken


def run_checked(label, p, epi, terms, kernel, worst, knobs=None, side=None, ex_tol=None, **kw):
    """launch + untouched + bound (+ TOL of test_gpu_ops for EPI_F32, + each hi8 byte within one e4m3 step of the decoded value); returns the Launch.
    `side` as the reference takes it; the raw planes of a saved pre-activation go in `pre`."""
    side = dict(side or {})
    r = launch(p, epi, terms, knobs, side, **kw)
    untouched(r)
    ex, tol = ex_tol if ex_tol is not None else ref.bound(p, epi, terms, skip_v8=kw.get("skip_v8", False), **side)
    got = decode(r)
    if not kw.get("hi8", True):
        ex, tol = {k: v for k, v in ex.items() if not k.endswith("_hi8")}, {k: v for k, v in tol.items() if not k.endswith("_hi8")}
    worst.add(epi, kernel, ref.check(f"{label} {epi} {kernel} M={r.M} N={r.N}", got, ex, tol))
    if epi == "f32":
        err, top = float((got["y"] - ex["y"]).abs().max()), float(ex["y"].abs().max())
        assert err < TOL[PRECISION[terms]] * max(1.0, top), (label, err)
    for name in [n for n in got if n.endswith("_hi8")]:
        assert bool(((got[name] - got[name[:-4]]).abs() <= ref.e4m3_step(got[name[:-4]], F8_EXP.get(name[:-4], ref.F8_ACT))).all()), (label, epi, kernel, name)
    return r


def problems(N, K, seed, exact=False):
    """One x [300, K], w, bias; the problem of M rows is its first M rows, so that launches of different M can be compared row by row."""
    x, w, b = ref.make_inputs(max(MS), N, K, seed)
    if exact:
        w = w.half().float()
    return {M: ref.Problem(x[:M].contiguous(), w, b) for M in MS}


# ---------------------------------------------------------------- gemm_kernel: terms 1 - 4, every tile, every row-major epilogue
@pytest.mark.parametrize("N,K", NKS)
@pytest.mark.parametrize("terms,exact", [(1, False), (2, False), (3, False), (4, False), (4, True)])
def test_row_epilogues_on_every_tile(terms, exact, N, K):
    ps, worst, ident = problems(N, K, 11, exact), Worst(), Identities()
    for epi in ROW_EPILOGUES:
        prev = {}
        for M in MS:
            p = ps[M]
            side = side_inputs(ps[max(MS)], epi)                          # one side input for all M: its first M rows
            side = {k: (v[:M] if k in ("resid", "pre") else v) for k, v in side.items()}
            ex_tol, runs = None, {}
            for tile in (64, 128, 256):
                kernel = route(terms, M, N, K, exact=exact, tile=tile)
                assert kernel == f"gemm{128 if tile == 256 and N % 256 else tile}" + ("_wx" if exact else "")
                if epi == "dgelu":
                    value, planes = pre_planes(side["pre"], ref.PRODUCTS[terms] == 3)
                    ex_tol = ex_tol or ref.bound(p, epi, terms, pre=value)
                    r = run_checked(f"terms {terms}", p, epi, terms, kernel, worst, {"gemm_tile": tile}, {"pre": value}, ex_tol, pre=planes)
                else:
                    ex_tol = ex_tol or ref.bound(p, epi, terms, **side)
                    r = run_checked(f"terms {terms}", p, epi, terms, kernel, worst, {"gemm_tile": tile}, side, ex_tol)
                runs[tile] = r
                if M == 200:
                    ident.same(r, launch(p, epi, terms, {"gemm_tile": tile}, side, pre=planes if epi == "dgelu" else (None, None)), f"{epi} tile {tile}: two runs")
                # a forced tile: the first M' rows of this launch are the launch of M' rows (ragged tiles against the predicate-free path)
                if tile in prev:
                    ident.same(r, prev[tile], f"{epi} tile {tile}: the first {prev[tile].M} rows of M = {M}", rows=prev[tile].M)
            prev = runs
            if terms in (1, 3):                                                # the tiles share one summation order
                ident.same(runs[64], runs[128], f"{epi} M = {M}: tiles 64 / 128")
                ident.same(runs[128], runs[256], f"{epi} M = {M}: tiles 128 / 256")
        if N >= 256:                                                           # the store mask: the last 128 columns are not written
            M, nv = 200, N - 128
            pn = ref.Problem(ps[M].x, ps[M].w[:nv], ps[M].bias[:nv])
            side = side_inputs(pn, epi)
            wide = {k: (torch.cat([v, v[:, :128]], 1) if torch.is_tensor(v) and v.dim() == 2 else v) for k, v in side.items()}    # the launch's pitch is N
            for tile in (64, 128, 256):
                if epi == "dgelu":
                    value, planes = pre_planes(wide["pre"], ref.PRODUCTS[terms] == 3)
                    ex_tol = ref.bound(pn, epi, terms, pre=value[:, :nv])
                    r = launch(ps[M], epi, terms, {"gemm_tile": tile}, n_valid=nv, pre=planes)
                else:
                    ex_tol = ref.bound(pn, epi, terms, **side)
                    r = launch(ps[M], epi, terms, {"gemm_tile": tile}, wide, n_valid=nv)
                untouched(r)
                ref.check(f"terms {terms} {epi} tile {tile} n_valid {nv}", decode(r), *ex_tol)
    worst.report(f"terms{terms}{'x' if exact else ''} N={N} K={K}")
    ident.done()


# ---------------------------------------------------------------- f16f8: gemm_f8_kernel on both tiles, gemm_f8s_kernel, gemm_pp_kernel
def f8_routes(N, K, exact):
    """(kernel, knobs, split_lines) of every f16f8 kernel this shape can reach."""
    routes = [("f8_128x128" + ("_wx" if exact else ""), {"gemm_tile": 128}, False)]
    if N % 256 == 0:
        routes.append(("f8_128x256" + ("_wx" if exact else ""), {"gemm_tile": 256, "gemm_mfma16": 0}, False))
    if not exact and (N % 256 == 0 or N == 384):
        routes.append(("f8s", {"gemm_tile": 256}, False))
    if N % 256 == 0 and K >= 128:
        routes += [("pp", {"gemm_pp": 2}, False), ("pp", {"gemm_pp": 2}, True)]
    return routes


@pytest.mark.parametrize("N,K", NKS)
@pytest.mark.parametrize("exact", [False, True])
def test_row_epilogues_f16f8(exact, N, K):
    ps, worst, ident = problems(N, K, 12, exact), Worst(), Identities()
    for epi in ROW_EPILOGUES:
        prev = {}
        for M in MS:
            p = ps[M]
            side = side_inputs(ps[max(MS)], epi)
            side = {k: (v[:M] if k in ("resid", "pre") else v) for k, v in side.items()}
            planes = (None, None)
            if epi == "dgelu":
                side["pre"], planes = pre_planes(side["pre"], True)
            ex_tol, runs = ref.bound(p, epi, 5, **side), {}
            for kernel, knobs, ilv in f8_routes(N, K, exact):
                if kernel == "pp" and (epi not in PP_EPILOGUES or (ilv and epi not in ("planes", "gelu"))):
                    continue
                assert route(5, M, N, K, exact=exact, tile=knobs.get("gemm_tile", 0), mfma16=knobs.get("gemm_mfma16", 1), pp=knobs.get("gemm_pp", 1)) == kernel
                r = run_checked("f16f8", p, epi, 5, kernel + ("_lines" if ilv else ""), worst, knobs, side, ex_tol, split_lines=ilv, pre=planes)
                runs[(kernel, ilv)] = r
                if (kernel, ilv) in prev:
                    ident.same(r, prev[(kernel, ilv)], f"{epi} {kernel}: the first {prev[(kernel, ilv)].M} rows of M = {M}", rows=prev[(kernel, ilv)].M)
                if M == 200 and not ilv:
                    ident.same(r, launch(p, epi, 5, knobs, side, pre=planes), f"{epi} {kernel}: two runs")
                if M == 200 and exact and kernel != "pp" and epi in ("planes", "gelu"):     # no hi8 image for a consumer on fp16-exact weights: the other planes as before
                    bare = run_checked("f16f8 no hi8", p, epi, 5, kernel, worst, knobs, side, ex_tol, hi8=False)
                    full = raw_planes(r)
                    assert all(torch.equal(v, full[k]) for k, v in raw_planes(bare).items()), (epi, kernel)
            prev = runs
            if ("pp", False) in runs:
                if ("f8s", False) in runs:                                     # the ping-pong kernel is the 16 x 16 form's arithmetic in another schedule
                    ident.same(runs[("pp", False)], runs[("f8s", False)], f"{epi} M = {M}: ping-pong / 16 x 16 form")
                if ("pp", True) in runs:                                       # split lines are the planes' bytes, interleaved
                    ident.same(runs[("pp", True)], runs[("pp", False)], f"{epi} M = {M}: split lines / planes")
            if ("f8s", False) in runs and ("f8_128x256", False) in runs:        # gemm_mfma16 1 vs 0: the same products in another summation order
                a, b = decode(runs[("f8s", False)]), decode(runs[("f8_128x256", False)])
                top = max(1.0, float(ex_tol[0]["y"].abs().max()))
                if epi in ref.F32_EPILOGUES:
                    assert float((a["y"] - b["y"]).abs().max()) < 2e-5 * top, (epi, M)
        if N >= 256:
            M, nv = 200, N - 128
            pn = ref.Problem(ps[M].x, ps[M].w[:nv], ps[M].bias[:nv])
            side = side_inputs(pn, epi)
            wide = {k: (torch.cat([v, v[:, :128]], 1) if torch.is_tensor(v) and v.dim() == 2 else v) for k, v in side.items()}
            planes = (None, None)
            if epi == "dgelu":
                value, planes = pre_planes(wide["pre"], True)
                side["pre"] = value[:, :nv]
            ex_tol = ref.bound(pn, epi, 5, **side)
            for kernel, knobs, ilv in f8_routes(N, K, exact):
                if ilv or (kernel == "pp" and epi not in PP_EPILOGUES):
                    continue
                r = launch(ps[M], epi, 5, knobs, wide, n_valid=nv, pre=planes)
                untouched(r)
                ref.check(f"f16f8 {epi} {kernel} n_valid {nv}", decode(r), *ex_tol)
    worst.report(f"f16f8{'x' if exact else ''} N={N} K={K}")
    ident.done()


# ---------------------------------------------------------------- EPI_QKV
def qkv_problem(B, S, H, K=128, lora=False, seed=21):
    x, w, b = ref.make_inputs(B * S, 3 * H * 64, K + (64 if lora else 0), seed)
    M = B * S
    return ref.Problem(x, w, b, [(0, 0, K, M, M, 1, 0), (K, K, 64, M, M, 1, 0)] if lora else None), {"scale": Q_SCALE, "S": S, "H": H}


@pytest.mark.parametrize("B,S,H", [(2, 100, 2), (3, 75, 4), (1, 129, 6)])
@pytest.mark.parametrize("terms", [1, 2, 3, 4, 5])
def test_qkv(terms, B, S, H):
    p, side = qkv_problem(B, S, H)
    M, N, K, worst = p.M, p.N, 128, Worst()
    if terms < 5:
        ex_tol, runs = ref.bound(p, "qkv", terms, **side), []
        for tile in (64, 128, 256):
            kernel = route(terms, M, N, K, tile=tile)
            assert kernel == f"gemm{128 if tile == 256 and N % 256 else tile}"
            runs.append(run_checked(f"terms {terms}", p, "qkv", terms, kernel, worst, {"gemm_tile": tile}, side, ex_tol))
        if terms in (1, 3):
            assert same_bytes(runs[0], runs[1]) and same_bytes(runs[1], runs[2]), "tiles 64 / 128 / 256"
    else:
        # H = 2 (N = 384) and H = 6 (N = 1152): the 16 x 16 kernel's last 256-column tile is half / three-quarters full; H = 4 (N = 768): every f16f8 kernel
        routes = [("f8_128x128", {"gemm_tile": 128}), ("f8s", {"gemm_tile": 256})]
        if N % 256 == 0:
            routes += [("f8_128x256", {"gemm_tile": 256, "gemm_mfma16": 0}), ("pp", {"gemm_pp": 2})]
        for skip_v8 in (False, True):
            ex_tol, runs = ref.bound(p, "qkv", 5, skip_v8=skip_v8, **side), {}
            for kernel, knobs in routes:
                assert route(5, M, N, K, tile=knobs.get("gemm_tile", 0), mfma16=knobs.get("gemm_mfma16", 1), pp=knobs.get("gemm_pp", 1)) == kernel
                runs[kernel] = run_checked(f"f16f8 skip_v8={int(skip_v8)}", p, "qkv", 5, kernel, worst, knobs, side, ex_tol, skip_v8=skip_v8)
                again = launch(p, "qkv", 5, knobs, side, skip_v8=skip_v8)
                assert same_bytes(runs[kernel], again)
            if "pp" in runs:
                assert same_bytes(runs["pp"], runs["f8s"])
    worst.report(f"terms{terms} B={B} S={S} H={H}")


def test_qkv_at_whisper_tinys_width_on_the_automatic_route():
    """N = 1152 (H = 6) with K = 384: from nine clips of 1500 positions on, the automatic rule gives EPI_QKV to the 16 x 16 kernel with a last column tile
    that is three-quarters full.  A column >= n_valid would land in a fourth plane, so only the store mask keeps that launch inside its planes: the guard
    band is that fourth plane.  Values are compared on the first and the last clip (the bound's reference over 13 500 rows would take the test's time)."""
    B, S, H, K = 9, 1500, 6, 384
    assert route(5, B * S, 3 * H * 64, K) == "f8s" and route(5, (B - 1) * S, 3 * H * 64, K) == "f8_128x128"
    p, side = qkv_problem(B, S, H, K, seed=23)
    r = launch(p, "qkv", 5, None, side)
    untouched(r)
    got = decode(r)
    ends = ref.Problem(torch.cat([p.x[:S], p.x[-S:]]), p.w, p.bias)
    ex, tol = ref.bound(ends, "qkv", 5, **side)
    ref.check("f16f8 qkv f8s automatic, clips 0 and 8", {k: v[[0, B - 1]] for k, v in got.items()}, ex, tol)
    assert all(bool(torch.isfinite(v).all()) for v in got.values())
    assert same_bytes(r, launch(p, "qkv", 5, {"gemm_tile": 256}, side))


@pytest.mark.parametrize("terms", [1, 2, 3, 4, 5])
def test_lora_projection_writes_a_narrow_matrix(terms):
    """u = (alpha / r) x A^T as linear_with_lora launches it: N = 128 columns computed, n_valid = ldo = 64 stored, densely -- a store past the mask would
    land in the next row's first columns."""
    worst, scale = Worst(), 16.0 / 8.0
    for M, K in ((200, 128), (257, 768)):
        x, w, _ = ref.make_inputs(M, 128, K, 81)
        wide, narrow = ref.Problem(x, w, None), ref.Problem(x, w[:64], None)
        ex_tol = ref.bound(narrow, "planes", terms, scale=scale)
        for tile in (64, 128, 256):
            kernel = route(terms, M, 128, K, tile=tile)
            assert kernel == ("f8_128x128" if terms == 5 else f"gemm{min(tile, 128)}")
            r = launch(wide, "planes", terms, {"gemm_tile": tile}, {"scale": scale}, n_valid=64, ldo=64)
            untouched(r)
            worst.add("planes", kernel + "_narrow", ref.check(f"terms {terms} lora projection {kernel} M={M}", decode(r), *ex_tol))
    worst.report(f"terms{terms} lora-projection")


@pytest.mark.parametrize("terms", [1, 3, 5])
def test_qkv_and_residual_with_a_lora_segment(terms):
    """[x | u] [W | B]^T with Ku = 64: the two-segment launches of linear_with_lora."""
    worst = Worst()
    p, side = qkv_problem(2, 100, 2, lora=True)
    kernel = route(terms, p.M, p.N, 128, nseg=2, tile=128)
    assert kernel == ("f8_128x128_multi" if terms == 5 else "gemm128")
    run_checked(f"terms {terms} lora", p, "qkv", terms, kernel, worst, {"gemm_tile": 128}, side)
    p4, side4 = qkv_problem(3, 75, 4, lora=True)
    for tile in (128, 256):
        kernel = route(terms, p4.M, p4.N, 128, nseg=2, tile=tile)
        assert kernel == (f"f8_128x{tile}_multi" if terms == 5 else f"gemm{tile}")
        run_checked(f"terms {terms} lora", p4, "qkv", terms, kernel, worst, {"gemm_tile": tile}, side4)
    for M, N, K in ((200, 384, 128), (257, 256, 192)):
        x, w, b = ref.make_inputs(M, N, K + 64, 31)
        pr = ref.Problem(x, w, b, [(0, 0, K, M, M, 1, 0), (K, K, 64, M, M, 1, 0)])
        sr = side_inputs(pr, "f32_resid")
        ex_tol = ref.bound(pr, "f32_resid", terms, **sr)
        for tile in (64, 128, 256):
            kernel = route(terms, M, N, K, nseg=2, tile=tile)
            out_of_place = run_checked(f"terms {terms} lora", pr, "f32_resid", terms, kernel, worst, {"gemm_tile": tile}, sr, ex_tol)
            in_place = launch(pr, "f32_resid", terms, {"gemm_tile": tile}, sr, inplace=True)
            untouched(in_place)
            assert same_bytes(in_place, out_of_place), (M, N, tile)
    worst.report(f"terms{terms} lora")


# ---------------------------------------------------------------- EPI_F32_GELU_POS behind the conv stem's row map
def conv_problem(B, S, Cin, N, rows_pos=None, seed=41):
    x, (_, w, b) = ref.make_inputs(B * 2 * S, 1, Cin, seed)[0], ref.make_inputs(1, N, 3 * Cin, seed + 2)
    rows_pos = S if rows_pos is None else rows_pos
    pos = torch.randn((rows_pos, N), generator=torch.Generator().manual_seed(seed + 1)) if rows_pos > 1 else torch.zeros((1, N))
    return ref.Problem(x, w, b, ref.conv_segs(S, Cin), B * S), {"pos": pos, "rows_pos": rows_pos}


@pytest.mark.parametrize("S,N", [(100, 128), (100, 384), (129, 128), (129, 384)])
@pytest.mark.parametrize("terms", [1, 2, 3, 4, 5])
def test_conv_stem_gelu_pos(terms, S, N):
    worst = Worst()
    for rows_pos in (None, 1):                                                 # the positional table; then one zero row, as the compact stem's conv2 runs
        p, side = conv_problem(2, S, 128, N, rows_pos)
        ex_tol, runs = ref.bound(p, "gelu_pos", terms, **side), []
        for tile in (64, 128, 256):
            kernel = route(terms, p.M, N, 128, nseg=3, tile=tile)
            assert kernel == ("f8_128x128_multi" if terms == 5 else f"gemm{128 if tile == 256 else tile}")
            runs.append(run_checked(f"terms {terms} rows_pos={side['rows_pos']}", p, "gelu_pos", terms, kernel, worst, {"gemm_tile": tile}, side, ex_tol))
        if terms in (1, 3):
            assert same_bytes(runs[0], runs[1]) and same_bytes(runs[1], runs[2])
    worst.report(f"terms{terms} conv S={S} N={N}")


@pytest.mark.parametrize("terms,N,clips", [(3, 384, 220), (5, 256, 656)])
def test_conv_stem_m_pick(terms, N, clips):
    """A launch of M rows whose kernel is chosen as for m_pick rows equals the first M rows of a launch of m_pick rows, bit for bit: how the compact conv
    stem keeps the full stem's summation order.  The two row counts take different kernels on their own."""
    S, Cin = 100, 128
    big, side = conv_problem(clips, S, Cin, N, seed=43)
    M, m_pick = 2 * S, big.M
    small = ref.Problem(big.x[:2 * M].contiguous(), big.w, big.bias, ref.conv_segs(S, Cin), M)
    assert route(terms, M, N, Cin, nseg=3) != route(terms, m_pick, N, Cin, nseg=3)
    full = launch(big, "gelu_pos", terms, None, side)
    picked = launch(small, "gelu_pos", terms, None, side, m_pick=m_pick)
    untouched(full), untouched(picked)
    assert same_bytes(picked, full, rows=M)
    ref.check(f"terms {terms} m_pick", decode(picked), *ref.bound(small, "gelu_pos", terms, **side))


# ---------------------------------------------------------------- EPI_BF16_GELU_SAVE -> EPI_BF16_DGELU
@pytest.mark.parametrize("terms", [1, 3, 5])
def test_gelu_save_then_dgelu_round_trip(terms):
    """fc1's training forward saves its pre-activation; fc2's backward reads it back: the planes the first launch wrote are the side input of the second,
    and each launch is compared with its own float64 result (the second one's from the value its planes hold)."""
    worst, three = Worst(), ref.PRODUCTS[terms] == 3
    for M, d, f in ((200, 128, 256), (257, 192, 384)):
        x, w1, b1 = ref.make_inputs(M, f, d, 51)
        fwd = ref.Problem(x, w1, b1)
        for tile in ((128, 256) if terms == 5 else (64, 128, 256)):
            knobs = {"gemm_tile": tile, "gemm_mfma16": 0} if terms == 5 else {"gemm_tile": tile}
            k1 = route(terms, M, f, d, tile=tile, mfma16=0)
            r1 = run_checked(f"terms {terms} save", fwd, "gelu_save", terms, k1, worst, knobs)
            hi2 = r1.out["hi2"].view(torch.bfloat16)[:M * f].view(M, f).contiguous()
            lo2 = r1.out["lo2"].view(torch.bfloat16)[:M * f].view(M, f).contiguous() if three else None
            pre = hi2.double().cpu() + (lo2.double().cpu() if three else 0.0)
            # backward: one segment dy W2^T-transposed ([M, d] . [f, d]^T), then the two-segment form with an adapter term of 64 columns
            for lora in (False, True):
                dy, w2, _ = ref.make_inputs(M, f, d + (64 if lora else 0), 52)
                bwd = ref.Problem(dy, w2, None, [(0, 0, d, M, M, 1, 0), (d, d, 64, M, M, 1, 0)] if lora else None)
                k2 = route(terms, M, f, d, nseg=2 if lora else 1, tile=tile, mfma16=0)
                run_checked(f"terms {terms} dgelu", bwd, "dgelu", terms, k2 + ("_2seg" if lora and "multi" not in k2 else ""), worst, knobs, {"pre": pre},
                            ref.bound(bwd, "dgelu", terms, pre=pre), pre=(hi2, lo2))
        if terms == 5:                                                         # and on the 16 x 16 form, which the training MLP takes at full size
            r = run_checked("terms 5 save", fwd, "gelu_save", 5, "f8s", worst, {"gemm_tile": 256})
            assert route(5, M, f, d, tile=256) == "f8s" and same_bytes(r, launch(fwd, "gelu_save", 5, {"gemm_tile": 256}))
    worst.report(f"terms{terms} save-dgelu")


# ---------------------------------------------------------------- the output planes' contract
@pytest.mark.parametrize("terms", [1, 2, 3, 4, 5])
def test_output_planes_keep_their_contract(terms):
    """EPI_BF16 with scale 1 rounds the very fp32 value EPI_F32 stores (same kernel, same products, no side input): the decoded planes are within the
    format's stated error of it -- |x - hi - lo| <= 2^-17 |x| for a bf16 pair, 2^-16 |x| for fp16 + lo8 (plus half the e4m3 subnormal step, 2^-19, below
    |x| = 2^-3: common.h), half an ulp for a single plane (2^-8 |x| bf16, 2^-11 |x| fp16), and an fp16 pair to 2^-23 |x| down to half fp16's subnormal
    step, 2^-25 -- and each hi8 byte is within one e4m3 step of the decoded value at its exponent (run_checked asserts that for every f16f8 launch)."""
    rel, floor = {1: 2.0 ** -8, 2: 2.0 ** -11, 3: 2.0 ** -17, 4: 2.0 ** -23, 5: 2.0 ** -16}[terms], {1: 0.0, 2: 2.0 ** -25, 3: 0.0, 4: 2.0 ** -25, 5: 2.0 ** -19}[terms]
    for M, N, K in ((129, 128, 64), (300, 256, 192), (200, 768, 768)):
        x, w, b = ref.make_inputs(M, N, K, 61)
        p = ref.Problem(x, w, b)
        routes = [{"gemm_tile": t} for t in (64, 128, 256)] if terms < 5 else [k for _, k, ilv in f8_routes(N, K, False)]
        for i, knobs in enumerate(routes):
            ilv = terms == 5 and i == len(routes) - 1 and knobs.get("gemm_pp") == 2
            y = decode(launch(p, "f32", terms, knobs))["y"]
            r = launch(p, "planes", terms, knobs, {"scale": 1.0}, split_lines=ilv)
            untouched(r)
            got = decode(r)
            excess = ((got["y"] - y).abs() - rel * y.abs() - floor).max()
            print(f"terms {terms} {(M, N, K)} {knobs}: worst |decoded - fp32| / |fp32| = {float(((got['y'] - y).abs() / y.abs().clamp_min(2.0 ** -3)).max()):.3e} (contract {rel:.3e})")
            assert float(excess) <= 0.0, (knobs, float(excess))
            if terms == 5:
                assert bool(((got["y_hi8"] - got["y"]).abs() <= ref.e4m3_step(got["y"], ref.F8_ACT)).all()), knobs


# ---------------------------------------------------------------- refusals
def test_refusals_leave_the_outputs_alone():
    from mlx8_ws_audio_transformer_amd import _lib, ops
    M, N, K = 200, 256, 192
    x, w, b = ref.make_inputs(M, N, K, 71)
    p = ref.Problem(x, w, b)
    xd, wd, bd = _dev(p)

    def refused(code, epi, terms, knobs=None, **kw):
        out = {"f32": _sent(M * N * 4), "hi": _sent(M * N * 2), "lo": _sent(M * N * 2), "hi8": _sent(M * N), "lo8": _sent(M * N), "ilv": _sent(M * N * 4),
               "hi2": _sent(M * N * 2), "lo2": _sent(M * N * 2)}
        for key in kw.pop("without", ()):
            del out[key]
        with tuning(**(knobs or {})), pytest.raises(_lib.AwtError) as e:
            ops.linear_fused(xd, wd, bd, epi, terms, out, **kw)
        torch.cuda.synchronize()
        assert e.value.code == code and "op_linear_fused" in e.value.msg, (epi, terms, kw, e.value)
        assert all(bool((t == SENT).all()) for t in out.values()), (epi, terms, kw)

    refused(ERR_INVALID, 8, 3)                                                  # unknown epilogue
    refused(ERR_INVALID, -1, 3)
    for epi in ("gelu_pos", "gelu_save", "dgelu"):                              # epilogues the ping-pong kernel lacks, under gemm_pp = 2
        refused(ERR_INVALID, epi, 5, {"gemm_pp": 2}, pos=bd.repeat(2, 1), rows_pos=2, pre=(_sent(M * N * 2), None))
    for nv in (N + 4, 6, 130, -4):                                              # n_valid above N, not a multiple of 4
        refused(ERR_INVALID, "f32", 3, n_valid=nv)
    refused(ERR_INVALID, "f32", 5, n_valid=132)                                 # f16f8 stores eight columns at a time
    refused(ERR_INVALID, "planes", 3, without=("hi",))                          # null planes
    refused(ERR_INVALID, "planes", 3, without=("lo",))
    refused(ERR_INVALID, "planes", 5, without=("lo8",))
    refused(ERR_INVALID, "gelu_save", 3, without=("hi2",))
    refused(ERR_INVALID, "gelu_save", 3, without=("lo2",))
    refused(ERR_INVALID, "f32", 3, without=("f32",))
    refused(ERR_INVALID, "f32_resid", 3)                                        # no residual
    refused(ERR_INVALID, "gelu_pos", 3)                                         # no positional table
    refused(ERR_INVALID, "dgelu", 3)                                            # no saved pre-activation
    refused(ERR_INVALID, "planes", 5, split_lines=True)                         # split lines without the ping-pong kernel
    refused(ERR_INVALID, "f32", 5, {"gemm_pp": 2}, split_lines=True)            # ... or with an fp32 epilogue
    refused(ERR_INVALID, "qkv", 3, S=100, H=2)                                  # N != 3 H 64
    refused(ERR_INVALID, "f32", 3, segs=[(0, 0, K, M, 2 * M, 1, 0)])            # rows_in != row_mul * rows_out
    refused(ERR_INVALID, "f32", 3, segs=[(0, 0, K, 100, 200, 2, 0)])            # the row map reads beyond x
    refused(ERR_INVALID, "f32", 3, segs=[(0, 64, K, M, M, 1, 0)])               # the segment leaves w
    refused(ERR_INVALID, "f32", 6)                                              # unknown precision
    need = ops.linear_fused_workspace_bytes(M, K, N, K)
    refused(ERR_WORKSPACE, "f32", 3, workspace=_lib.workspace(need, "cuda"), ws_bytes=need - 1)
