"""GPU: token-level timestamps (generate(return_token_timestamps=True)): the three kernels of csrc/alignment.hip against their host
restatements, and the four cases of tools/make_golden_token_timestamps.py's fixture (transformers 5.15) end to end on the mini model."""
import json
import os
import sys

import numpy as np
import pytest
import torch

from mlx8_ws_audio_transformer_amd import generation as G, weights as wts
from tests.util import golden

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))

CASES = ("sf_greedy", "sf_beam", "lf_greedy", "lf_beam")


def _tool():
    import make_golden_timestamps as T
    return T


# ------------------------------------------------------------------------------------------------ awt_op_dtw
def _device_paths(m, nf=None, negate=False):
    """One launch over the batch m [clips, T, frames]: per clip (jump frames, text_idx, time_idx)."""
    dm = torch.from_numpy(np.ascontiguousarray(m, dtype=np.float32)).cuda()
    dn = None if nf is None else torch.tensor(nf, dtype=torch.int32).cuda()
    jump, text, time, start = (t.cpu().numpy() for t in G.dtw(dm, dn, negate=negate))
    return [(jump[c], text[c, start[c]:], time[c, start[c]:]) for c in range(m.shape[0])], (jump, text, time, start)


def _check_dtw(m, nf=None, negate=False, what=""):
    got, raw = _device_paths(m, nf, negate)
    again, raw2 = _device_paths(m, nf, negate)
    for c, (jump, text, time) in enumerate(got):
        f = m.shape[2] if nf is None else nf[c]
        ref_text, ref_time = G.dtw_reference((-m[c, :, :f] if negate else m[c, :, :f]).astype(np.float32))
        np.testing.assert_array_equal(text, ref_text, err_msg=f"{what} clip {c} text")
        np.testing.assert_array_equal(time, ref_time, err_msg=f"{what} clip {c} time")
        first = ref_time[np.pad(np.diff(ref_text), (1, 0), constant_values=1).astype(bool)]
        np.testing.assert_array_equal(jump, first, err_msg=f"{what} clip {c} jump frames")
        for a, b in zip(got[c], again[c]):                                   # run twice: bit-identical
            np.testing.assert_array_equal(a, b)
    np.testing.assert_array_equal(raw[0], raw2[0])
    np.testing.assert_array_equal(raw[3], raw2[3])


def test_dtw_equals_the_reference_on_every_fixture_matrix():
    F = golden("token_timestamps.npz")
    for key in CASES:
        D = golden(f"token_timestamps_{key}.npz")
        for i in range(len(F["dtw_" + key])):
            m = D[f"m{i}"]
            got, _ = _device_paths(m[None])
            np.testing.assert_array_equal(got[0][1], D[f"text{i}"], err_msg=f"{key} {i}")      # HF's recorded path itself
            np.testing.assert_array_equal(got[0][2], D[f"time{i}"], err_msg=f"{key} {i}")
            again, _ = _device_paths(m[None])
            for a, b in zip(got[0], again[0]):
                np.testing.assert_array_equal(a, b)


@pytest.mark.parametrize("T", [1, 2, 63, 64, 65, 448])
def test_dtw_equals_the_reference_on_random_matrices(T):
    rng = np.random.default_rng(100 + T)
    for frames in (1, 3, 4, 750, 1500):
        _check_dtw(rng.standard_normal((1, T, frames)).astype(np.float32), what=f"T {T} frames {frames}")
    _check_dtw(rng.standard_normal((1, T, 40)).astype(np.float32), negate=True, what=f"T {T} negated")


def test_dtw_ragged_batch_ties_and_extreme_magnitudes():
    rng = np.random.default_rng(7)
    _check_dtw(rng.standard_normal((5, 30, 200)).astype(np.float32), nf=[200, 1, 77, 130, 2], what="ragged")
    _check_dtw(rng.standard_normal((3, 70, 90)).astype(np.float32), nf=[90, 64, 65], negate=True, what="ragged negated")
    _check_dtw(np.full((2, 66, 130), 0.25, dtype=np.float32), what="constant")                      # every comparison ties
    _check_dtw(np.zeros((1, 5, 9), dtype=np.float32), what="zeros")
    _check_dtw(rng.integers(-2, 3, size=(3, 65, 300)).astype(np.float32), what="small integers")   # exact sums, many ties
    _check_dtw((rng.standard_normal((2, 20, 60)) * 1e30).astype(np.float32), what="1e30")          # sums stay finite: 80 cells x 5e30
    _check_dtw((rng.standard_normal((2, 20, 60)) * 1e-30).astype(np.float32), what="1e-30")
    big = rng.standard_normal((1, 12, 40)).astype(np.float32)
    big[0, ::3] *= 1e20
    _check_dtw(big, what="mixed magnitudes")                                                       # small terms vanish in the float32 rounding, as in HF


def test_dtw_refuses_what_it_cannot_hold():
    m = torch.zeros((1, 449, 4), device="cuda")
    with pytest.raises(Exception, match="448"):
        G.dtw(m)


# ------------------------------------------------------------------------------------------------ awt_op_alignment_matrix
# max |device - alignment_matrix_reference| measured on the fixture's shapes (3 heads, 23-29 token rows, 604-1500 frames, width 7) on an
# MI355X: 1.5 x 2^-23, i.e. 3/8 ulp of the largest z-scores there.  The tests assert 4x that (margin for other shapes' summation order);
# both numbers are in DESIGN.md 4.8.  The differences are rounding of the z-scores, so they scale with |z|, and a z-score over T rows is at
# most sqrt(T - 1) (5.3 for the fixture's T <= 29): a shape with more token rows gets the bound times sqrt((T - 1) / 28).
MATRIX_DIFF_MEASURED = 1.79e-7


def _matrix_bound(T):
    return 4 * MATRIX_DIFF_MEASURED * max(1.0, ((T - 1) / 28.0) ** 0.5)


def _weights(shape, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return torch.softmax(2.0 * torch.randn(shape[:-1] + (1500,), generator=g, device="cuda"), dim=-1)[..., : shape[-1]].contiguous()


def _matrix_diff(w, width, nf=None):
    dn = None if nf is None else torch.tensor(nf, dtype=torch.int32).cuda()
    out = G.alignment_matrix(w, width, dn)
    worst = 0.0
    for c in range(w.shape[0]):
        f = w.shape[-1] if nf is None else nf[c]
        ref = G.alignment_matrix_reference(w[c, ..., :f], width)
        assert bool(torch.isfinite(out[c, :, :f]).all())
        worst = max(worst, float((out[c, :, :f] - ref).abs().max()))
        assert bool((out[c, :, f:] == 0).all())
    return worst


def test_alignment_matrix_against_the_torch_restatement():
    F = golden("token_timestamps.npz")
    shapes = sorted({(int(r), int(f)) for key in CASES for _, _, r, f, _ in F["dtw_" + key]})
    fixture = max(_matrix_diff(_weights((2, 3, r, f), 11 * r + f), 7) for r, f in shapes)
    print(f"alignment_matrix: max-abs difference on the fixture shapes {fixture:.3e} (recorded {MATRIX_DIFF_MEASURED:.3e})")
    bound = _matrix_bound(26)
    assert fixture <= bound == 4 * MATRIX_DIFF_MEASURED
    for width in (1, 3, 7, 15):
        d = _matrix_diff(_weights((3, 3, 26, 700), width), width, nf=[700, 604, 65])
        few = _matrix_diff(_weights((2, 2, 9, 8), 50 + width), width, nf=[max(width // 2, 1), 8])       # a clip with frames <= width // 2: unfiltered
        one = _matrix_diff(_weights((1, 6, 448, 130), 70 + width), width)
        print(f"alignment_matrix: width {width}: ragged {d:.3e}, few frames {few:.3e}, 448 rows x 6 heads {one:.3e}")
        assert max(d, few) <= bound and one <= _matrix_bound(448)
    w = _weights((2, 3, 26, 700), 5)
    a, b = G.alignment_matrix(w, 7), G.alignment_matrix(w, 7)
    assert torch.equal(a, b)
    for width in (0, 4, 17):
        with pytest.raises(ValueError, match="median_filter_width"):
            G.alignment_matrix(w, width)


# ------------------------------------------------------------------------------------------------ awt_op_alignment_weights
def test_alignment_weights_against_fp64_softmax():
    """Bound from the operand format.  Queries and keys are fp32 and the products are fp32 FMAs (the decoder's own cross-attention form,
    DESIGN.md section 3: no reduced-precision operand), u = 2^-24.  A score s = sum_e (0.125 q_e) k_e of 64 terms carries at most
    |ds| <= 65 u sum_e |0.125 q_e k_e| =: delta (64 sequential additions plus the product rounding; scaling by 0.125 is exact).  A
    probability p = exp(s - m) / sum_j exp(s_j - m) then has a relative error of at most 2 delta (numerator and every term of the
    denominator move by delta) + 2 |s - m| u (rounding of the difference and the argument scaling inside the hardware exponential)
    + 4 u (exponential and division) + S u (the fp32 sum of S terms): bound = p (2 delta + (2 max|s - m| + 4 + S) u) + 1e-30."""
    torch.manual_seed(3)
    slots, rows, Tmax, d, nl, S, group = 2, 6, 12, 128, 3, 1500, 2
    clips = rows // group
    q = torch.randn((slots, rows, Tmax, d), device="cuda")
    kv = torch.randn((clips * S, 2 * nl * d), device="cuda")
    table = torch.tensor([[0, 0, 1], [1, 2, 0], [1, 2, 1], [0, 0, 0]], dtype=torch.int32).cuda()
    t0, T = 2, 9
    src = torch.randint(0, rows, (clips, T), dtype=torch.int32).cuda()
    src[1, 5:] = 0                                                           # beam search's substitution: row 0 (clip 0) inside clip 1's tile
    u = 2.0 ** -24
    for src_row, grp, n_clips in ((src, group, clips), (None, 1, rows)):
        kv_use = kv if src_row is not None else torch.randn((rows * S, 2 * nl * d), device="cuda")
        for frames in (S, 604):
            out = G.alignment_weights(q, kv_use, nl, S, table, n_clips, grp, t0, T, frames, src_row)
            assert out.shape == (n_clips, 4, T, frames)
            worst = 0.0
            for c in range(n_clips):
                for hs, (slot, layer, head) in enumerate(table.tolist()):
                    for t in range(T):
                        r = int(src_row[c, t]) if src_row is not None else c * grp
                        qq = q[slot, r, t0 + t, 64 * head: 64 * head + 64].double() * 0.125
                        kk = kv_use[(r // grp) * S: (r // grp + 1) * S, 2 * layer * d + 64 * head: 2 * layer * d + 64 * head + 64].double()
                        s = kk @ qq
                        p = torch.softmax(s, dim=0)
                        delta = 65 * u * float((kk.abs() @ qq.abs()).max())
                        bound = p * (2 * delta + (2 * float((s.max() - s).max()) + 4 + S) * u) + 1e-30
                        err = (out[c, hs, t].double() - p[:frames]).abs()
                        assert bool((err <= bound[:frames]).all()), (c, hs, t, float((err / bound[:frames]).max()))
                        worst = max(worst, float((err / bound[:frames]).max()))
            print(f"alignment_weights: frames {frames}, gather {src_row is not None}: worst error / bound {worst:.3f}")
    full = G.alignment_weights(q, kv, nl, S, table, clips, group, t0, T, S, src)
    crop = G.alignment_weights(q, kv, nl, S, table, clips, group, t0, T, 604, src)
    assert torch.equal(full[..., :604], crop)                                # the crop applies to the stores, never to the sum
    assert float((full.sum(-1) - 1).abs().max()) < 1e-4


# ------------------------------------------------------------------------------------------------ end to end
def _model(F):
    from mlx8_ws_audio_transformer_amd.finetune import WhisperLoRAModel
    T = _tool()
    cfg = wts.config("mini")
    model = WhisperLoRAModel(cfg, None, decoder_layers=2, vocab=T.VOCAB, max_target_positions=T.DEC["max_pos"])
    model.encoder.load_state_dict({k: torch.from_numpy(v) for k, v in T.encoder_weights(cfg).items()}, strict=False)
    Wd = T.decoder_weights(cfg, int(F["dec_seed"]), float(F["logit_scale"]), float(F["ts_scale"]), float(F["eos_scale"]))
    model.decoder.load_state_dict({k: torch.from_numpy(v) for k, v in Wd.items()}, strict=True)
    model.generation_config = G.GenerationConfig.from_dict(json.loads(str(F["generation_config"])))
    model.config.median_filter_width = int(F["median_filter_width"])
    return model.eval()


def _features(seconds, longform=True):
    from mlx8_ws_audio_transformer_amd.feature_extraction import WhisperFeatureExtractor
    T = _tool()
    audio = [T.clip_audio(s, c) for c, s in enumerate(seconds)]
    fe = WhisperFeatureExtractor()
    if longform:
        f = fe(audio, sampling_rate=16000, truncation=False, padding="longest", return_attention_mask=True, return_tensors="pt")
        return f["input_features"].cuda(), f["attention_mask"]
    return fe(audio, sampling_rate=16000, return_tensors="pt")["input_features"].cuda(), None


@pytest.fixture(scope="module")
def loaded():
    F = golden("token_timestamps.npz")
    model = _model(F)
    lf, mask = _features(tuple(F["lf_seconds"]))
    sf, _ = _features(tuple(F["sf_seconds"]), longform=False)
    np.testing.assert_array_equal(mask.numpy(), F["mask_lf"])
    return F, model, {"lf": (lf, mask), "sf": (sf, None)}


@torch.no_grad()
@pytest.mark.parametrize("key", CASES)
def test_fixture_cases_against_transformers(loaded, key, monkeypatch):
    """Sequences and segment boundaries equal transformers'.  The alignment: (1) the device's DTW input is within 4 x matrix_sens of HF's
    recorded one on every window, (2) the device's path is as cheap under HF's matrix as HF's own, up to what (1) and the float32 cost
    array allow, on every window, (3) on the windows the fixture marks stable the token timestamps equal HF's exactly."""
    F, model, feats = loaded
    D = golden(f"token_timestamps_{key}.npz")
    x, mask = feats[key[:2]]
    windows, calls = [], []
    real_dtw, real_extract = G.dtw, G.extract_token_timestamps

    def dtw(matrix, num_frames=None, negate=True):
        out = real_dtw(matrix, num_frames, negate)
        jump, text, time, start = (t.cpu().numpy() for t in out)
        for c in range(matrix.shape[0]):
            f = matrix.shape[2] if num_frames is None else int(num_frames[c])
            windows.append(dict(m=-matrix[c, :, :f].cpu().numpy().astype(np.float64), jump=jump[c], text=text[c, start[c]:], time=time[c, start[c]:]))
        return out

    def extract(*a, **kw):
        out = real_extract(*a, **kw)
        calls.append(out.numpy().copy())
        return out

    monkeypatch.setattr(G, "dtw", dtw)
    monkeypatch.setattr(G, "extract_token_timestamps", extract)
    kw = {} if mask is None else {"attention_mask": mask}
    nb = {"sf_beam": 3, "lf_beam": 4}.get(key)
    out = model.generate(x, language="en", return_timestamps=True, return_token_timestamps=True, return_segments=True,
                         **({} if nb is None else {"num_beams": nb}), **kw)
    assert sorted(out) == ["segments", "sequences", "token_timestamps"]
    np.testing.assert_array_equal(out["sequences"].cpu().numpy(), F["seq_" + key])
    tts = out["token_timestamps"]
    assert tts.dtype == torch.float32 and tts.shape == out["sequences"].shape
    rows = [(c, s) for c, segs in enumerate(out["segments"]) for s in segs]
    assert len(rows) == len(F["seg_" + key])
    for (c, s), (c2, a, b), (t0, t1) in zip(rows, F["seg_" + key], F["segtime_" + key]):
        assert c == c2 and len(s["tokens"]) == b - a == len(s["token_timestamps"])
        assert abs(s["start"] - t0) <= 1e-9 and abs(s["end"] - t1) <= 1e-9
    meta = F["dtw_" + key]
    assert len(calls) == int(F["ncalls_" + key]) and len(windows) == len(meta)
    sens = float(F["matrix_sens_" + key])
    n_stable = 0
    for i, (w, (call, clip, n_rows, frames, stable)) in enumerate(zip(windows, meta)):
        mh = D[f"m{i}"].astype(np.float64)
        assert w["m"].shape == mh.shape == (n_rows, frames)
        tau = float(np.abs(w["m"] - mh).max())
        th, fh = D[f"text{i}"], D[f"time{i}"]
        cost = G.dtw_reference(mh, return_cost=True)[2]
        cmax = float(np.abs(cost[np.isfinite(cost)]).max())
        ld, lh = len(w["text"]), len(th)
        cd, ch = float(mh[w["text"], w["time"]].sum()), float(mh[th, fh].sum())
        slack = tau * (ld + lh) + (ld + lh) * 2.0 ** -23 * cmax
        same = np.array_equal(w["text"], th) and np.array_equal(w["time"], fh)
        print(f"{key} window {i} (call {call} clip {clip}, {n_rows} x {frames}, stable {stable}): tau {tau:.3e} (bound {4 * sens:.3e}), "
              f"cost_h(device path) - cost_h(HF path) {cd - ch:.3e} (slack {slack:.3e}), path equal {same}")
        assert tau <= 4 * sens, (key, i)
        assert cd <= ch + slack, (key, i)
        if stable:
            n_stable += 1
            np.testing.assert_array_equal(calls[call][clip], F[f"call_{key}_{call}_tts"][clip], err_msg=f"{key} window {i}")
    assert n_stable >= 2
    again = model.generate(x, language="en", return_timestamps=True, return_token_timestamps=True, **({} if nb is None else {"num_beams": nb}), **kw)
    assert torch.equal(again["token_timestamps"], tts)                       # bit-reproducible


@torch.no_grad()
def test_transcribe_token_timestamps(loaded):
    from mlx8_ws_audio_transformer_amd.feature_extraction import WhisperProcessor
    from mlx8_ws_audio_transformer_amd.transcribe import NoteTokenizer, transcribe
    F, model, _ = loaded
    T = _tool()
    audio = T.clip_audio(float(F["lf_seconds"][1]), 0)
    proc = WhisperProcessor(tokenizer=NoteTokenizer())
    plain = transcribe(model, proc, audio, language="en")
    res = transcribe(model, proc, audio, language="en", token_timestamps=True)
    assert [s["tokens"] for s in res["segments"]] == [s["tokens"] for s in plain["segments"]] and "token_timestamps" not in plain["segments"][0]
    for s in res["segments"]:
        ts = s["token_timestamps"]
        assert len(ts) == len(s["tokens"]) and all(b >= a for a, b in zip(ts, ts[1:]))
        assert all(s["seek"] * 0.01 - 1e-6 <= t <= s["seek"] * 0.01 + 30.0 for t in ts)
