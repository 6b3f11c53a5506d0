"""`MusicTranscriptionModel.generate_batch` and `Qwen3Decoder.step` on the weight-streaming linears (awt_linear_decode), on the GPU: the micro model of
tests/qwen3_reference.py's greedy fixture with a stub audio tower that returns the batch fixture's features per clip (tests/qwen3_batch_reference.py;
tests/test_generate_batch_host.py establishes on the CPU that the reference's top-2 margins make the exact-token comparison fair).  A "waveform" here is
the clip's index.  The logits bound is tests/test_gpu_qwen3_decoder.py's: max-abs <= 1e-3 max(1, max |reference logits|)."""
import functools

import pytest
import torch

from tests import qwen3_batch_reference as br
from tests import qwen3_reference as qr

pytestmark = pytest.mark.gpu

OUT_TOL = 1e-3                                                             # tests/test_gpu_qwen3_decoder.py


@functools.lru_cache(maxsize=None)
def _model():
    """(model, calls): calls lists the clip indices of every audio-tower call."""
    from mlx8_ws_audio_transformer_amd.music2midi import CrossAttentionAdapter, MusicTranscriptionModel, Qwen3Decoder
    cfg, sd, ref_adapter, audio = br.fixture()
    dec = Qwen3Decoder(cfg)
    dec.load_state_dict({k: v.float() for k, v in sd.items()}, strict=True)
    adapter = CrossAttentionAdapter(128, cfg.hidden_size, num_heads=2)
    adapter.load_state_dict({k: v.float() for k, v in ref_adapter.state_dict().items()}, strict=True)
    feats, calls = torch.cat(audio).float().cuda(), []

    def tower(waveforms, sampling_rate):
        calls.append(list(waveforms))
        return feats[torch.tensor(list(waveforms))].contiguous()

    return MusicTranscriptionModel(tower, adapter.cuda().eval(), dec.cuda().eval()), calls


def _greedy(model, clips, **kw):
    kw.setdefault("max_new_tokens", qr.GREEDY_STEPS)
    kw.setdefault("eos_token_id", qr.GREEDY_EOS)
    return model.generate_batch(clips, 16000, do_sample=False, bos_token_id=br.PROMPT[0], **kw)


def test_greedy_batch_reproduces_the_reference_and_the_single_clip_tokens():
    model, calls = _model()
    want = [t for t, _ in br.reference()]
    del calls[:]
    got = _greedy(model, [0, 1, 2])
    for i in range(br.CLIPS):
        print(f"clip {i}: generated {got[i]}\n        reference {want[i]}")
    assert calls == [[0, 1, 2]]                                            # the tower ran once, on the group's list
    assert got == want
    for i in range(br.CLIPS):
        alone = model.generate(i, 16000, max_new_tokens=qr.GREEDY_STEPS, do_sample=False, bos_token_id=br.PROMPT[0], eos_token_id=qr.GREEDY_EOS)
        assert alone == got[i]


def test_rows_stop_at_their_own_eos():
    model, _ = _model()
    want = [t for t, _ in br.reference()]
    eos, j = br.eos_case(want)
    got = _greedy(model, [0, 1, 2], eos_token_id=eos)
    cut = [w[:w.index(eos)] if eos in w else w for w in want]
    print(f"eos {eos}: lengths {[len(g) for g in got]} (clip 0 stops at step {j})")
    assert len(cut[0]) == j and len(cut[1]) > j and len(cut[2]) > j
    assert got == cut


def test_nine_clips_run_as_groups_of_eight_and_one():
    model, calls = _model()
    single = [_greedy(model, [i], max_new_tokens=4)[0] for i in range(br.CLIPS)]
    clips = [i % br.CLIPS for i in range(9)]
    del calls[:]
    got = _greedy(model, clips, max_new_tokens=4)
    assert calls == [clips[:8], clips[8:]]
    assert got == [single[c] for c in clips] and all(len(g) == 4 for g in got)


def test_sampling_is_reproducible():
    model, _ = _model()
    runs = []
    for _ in range(2):
        gen = torch.Generator(device="cuda").manual_seed(7)
        runs.append(model.generate_batch([0, 1, 2], 16000, max_new_tokens=12, temperature=0.7, do_sample=True, generator=gen, bos_token_id=br.PROMPT[0],
                                         eos_token_id=qr.GREEDY_EOS))
    print("sampled", runs[0])
    assert runs[0] == runs[1] and len(runs[0]) == 3
    assert all(len(r) <= 12 and all(0 <= t < 320 for t in r) for r in runs[0])


@pytest.mark.parametrize("B", [9, 8])
def test_step_logits_at_the_gemm_fallback_and_on_the_decode_path(B):
    """5 positions prefilled, then 3 single steps at B = 9 (the GEMM) and B = 8 (awt_linear_decode): every step's logits against the float64 full forward,
    over a cache pre-filled with NaN."""
    from mlx8_ws_audio_transformer_amd.music2midi import Qwen3Cache
    model, _ = _model()
    dec = model.text_decoder
    cfg, sd = br.fixture()[:2]
    x = qr.variates(f"batch.step.x.{B}", (B, 8, cfg.hidden_size), 3)
    ref = qr.forward({k: v.cuda() for k, v in sd.items()}, cfg, x.cuda())
    tol, xg = OUT_TOL * max(1.0, float(ref.abs().max())), x.float().cuda()
    cache = Qwen3Cache(cfg, B, 8, "cuda")
    for t in cache.k + cache.v:
        t.fill_(float("nan"))
    from mlx8_ws_audio_transformer_amd.native_decoder import PackedLinear
    decode, calls = PackedLinear.forward_decode, []
    PackedLinear.forward_decode = lambda self, *a, **kw: (calls.append(self.N), decode(self, *a, **kw))[1]
    try:
        with torch.no_grad():
            got = [dec.prefill(xg[:, :5], cache)] + [dec.step(xg[:, t:t + 1], cache) for t in range(5, 8)]
    finally:
        PackedLinear.forward_decode = decode
    assert len(calls) == (0 if B > 8 else 3 * (4 * cfg.num_hidden_layers + 1))   # the four projections of every layer and the lm_head, per step; never the prefill
    errs = [float((g.double() - ref[:, 4 + i]).abs().max()) for i, g in enumerate(got)]
    print(f"B {B}: prefill 5 + 3 steps, worst last-position logits max-abs {max(errs):.3e} (bound {tol:.3e}, {max(errs) / tol:.3f} of it)")
    assert all(bool(torch.isfinite(g).all()) for g in got) and max(errs) <= tol
