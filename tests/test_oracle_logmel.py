"""Pins oracle/logmel.py to the reference's arithmetic (transformers' Whisper feature extractor) through the
committed golden vectors, and checks the front-end's edge cases.  CPU only."""
import numpy as np
import pytest

from oracle import logmel
from tests.util import GENERIC_LOGMEL_CASES, generic_logmel_clip, golden, logmel_inputs

G = golden("logmel_whisper.npz")


def test_mel_filters_match_reference():
    fb = logmel.whisper_mel_filters()
    assert fb.shape == (201, 80)
    np.testing.assert_allclose(fb, G["mel_filters_201x80"], rtol=0, atol=1e-15)
    nnz = (fb > 0).sum(axis=0)
    assert nnz.min() >= 1 and nnz.max() <= 14 and int((fb > 0).sum()) == 391


@pytest.mark.parametrize("name", ["noise", "tone", "zeros", "short", "piano"])
def test_whisper_logmel_matches_reference_numpy_path(name):
    out = logmel.whisper_logmel([logmel_inputs()[name]])[0]
    assert out.shape == (80, 3000) and out.dtype == np.float32
    np.testing.assert_allclose(out[:, :404], G[f"{name}_np_live"], rtol=0, atol=2e-6)
    np.testing.assert_allclose(out[:, -4:], G[f"{name}_np_tail"], rtol=0, atol=2e-6)
    assert abs(float(out[0, 1500]) - float(G[f"{name}_np_padconst"])) <= 2e-6


@pytest.mark.parametrize("name,atol", [("noise", 1e-5), ("tone", 1e-5), ("short", 1e-5), ("piano", 1e-4)])
def test_whisper_logmel_vs_reference_torch_path(name, atol):
    # The path transformers 5.x takes when torch is importable (fp32 torch.stft); north-star mel tolerance 1e-5.
    # On clips with digital silence between pure tones ("piano") the reference's OWN two paths disagree by
    # 3.9e-5 in 0.2 % of the bins (fp32 FFT noise in bins ~8 decades below the clip maximum), so that input is
    # pinned to the float64 NumPy path at 2e-6 above and only bounded at 1e-4 here.
    out = logmel.whisper_logmel([logmel_inputs()[name]])[0]
    np.testing.assert_allclose(out[:, :404], G[f"{name}_torch_live"], rtol=0, atol=atol)


def test_zero_clip_is_the_degenerate_constant():
    out = logmel.whisper_logmel([np.zeros(64000, np.float32)])[0]
    assert np.all(out == np.float32(-1.5))  # (log10(1e-10) + 4) / 4


def test_padding_frames_are_one_constant_per_clip():
    out = logmel.whisper_logmel([logmel_inputs()["tone"]])[0]
    assert np.all(out[:, 402:] == out[0, 402])
    assert out[0, 402] == np.float32((out.max() * 4 - 4 - 8 + 4) / 4) or abs(out[0, 402] - (out.max() - 2.0)) < 1e-6


def test_per_clip_max_does_not_leak_across_the_batch():
    ins = logmel_inputs()
    out = logmel.whisper_logmel([ins["tone"], ins["short"] * 0.01])
    np.testing.assert_allclose(out[:, :, :404], G["batch2_torch_live"], rtol=0, atol=1e-5)


def test_trimmed_mode_matches_reference_extractor_padded_to_4s():
    out = logmel.whisper_logmel([logmel_inputs()["tone"]], n_samples=64000)[0]
    assert out.shape == (80, 400)
    np.testing.assert_allclose(out, G["tone_torch_trimmed"], rtol=0, atol=1e-5)


def test_long_clip_is_truncated_to_30s():
    x = np.concatenate([logmel_inputs()["tone"]] * 8)[:500000]
    a = logmel.whisper_logmel([x])[0]
    b = logmel.whisper_logmel([x[:480000]])[0]
    assert a.shape == (80, 3000) and np.array_equal(a, b)


@pytest.mark.parametrize("n_mels,hop", [(80, 512), (128, 512), (128, 128), (64, 512)])
def test_urbansound_logmel(n_mels, hop):
    G3 = golden("logmel_urbansound.npz")
    out = logmel.urbansound_logmel(logmel_inputs()["tone"], n_fft=1024, hop=hop, n_mels=n_mels)
    ref = G3[f"mels{n_mels}_hop{hop}"]
    assert out.shape == ref.shape == (n_mels, 1 + 64000 // hop)
    np.testing.assert_allclose(out, ref, rtol=0, atol=2e-4)  # ln() of small powers: fp32 stft vs fp64 oracle


def test_urbansound_logmel_other_configurations_against_torch_stft():
    """The configurations tests/test_gpu_logmel.py runs the HIP kernel at (n_fft 400 / 512, hop = n_fft and n_fft / 4, other sample rates, f_min > 0,
    f_max < sr / 2, clip lengths that are not a multiple of hop, the minimum length): the oracle against torch.stft in float64 (centre, reflect,
    periodic Hann) and torchaudio's published HTK filter-bank formula, restated here."""
    import torch
    for (n_fft, hop, n_mels), (sr, f_min, f_max, n, _) in sorted(GENERIC_LOGMEL_CASES.items()):
        clip = generic_logmel_clip(n)
        out = logmel.urbansound_logmel(clip, sample_rate=sr, n_fft=n_fft, hop=hop, n_mels=n_mels, f_min=f_min, f_max=f_max)
        spec = torch.stft(torch.from_numpy(clip).double(), n_fft, hop_length=hop, window=torch.hann_window(n_fft, periodic=True, dtype=torch.float64),
                          center=True, pad_mode="reflect", return_complex=True)
        power = (spec.real ** 2 + spec.imag ** 2).numpy()
        freqs = np.linspace(0, sr // 2, n_fft // 2 + 1)
        m = np.linspace(2595.0 * np.log10(1.0 + f_min / 700.0), 2595.0 * np.log10(1.0 + f_max / 700.0), n_mels + 2)
        f = 700.0 * (10.0 ** (m / 2595.0) - 1.0)
        slopes = f[None, :] - freqs[:, None]
        fb = np.maximum(0.0, np.minimum(-slopes[:, :-2] / np.diff(f)[:-1], slopes[:, 2:] / np.diff(f)[1:]))
        ref = np.log(fb.T @ power + 1e-6)
        assert out.shape == ref.shape == (n_mels, 1 + n // hop), (n_fft, hop, n_mels)
        np.testing.assert_allclose(out, ref, rtol=0, atol=1e-5, err_msg=str((n_fft, hop, n_mels)))


def test_urbansound_prepare_mono_pad_trim():
    st = np.stack([np.ones(1000, np.float32), 3 * np.ones(1000, np.float32)])
    w = logmel.urbansound_prepare(st)
    assert w.shape == (64000,) and np.all(w[:1000] == 2.0) and np.all(w[1000:] == 0)
    assert logmel.urbansound_prepare(np.ones(70000, np.float32)).shape == (64000,)


def test_real_recording_matches_reference_numpy_path():
    """First 4 s of the reference's own sample recording (.charles/samples/..._00_08s.wav, stereo PCM16 -> channel mean): on real spectra the
    reference's fp32 torch.stft path and its float64 NumPy path differ by 1.7e-5 (stored in the fixture); the oracle follows the float64 path."""
    from tests.util import real_audio
    pcm, mono, R = real_audio()
    assert pcm.shape == (64000, 2) and pcm.dtype == np.int16 and float(R["np_vs_torch_max_abs"]) > 1e-5
    out = logmel.whisper_logmel([mono])[0]
    np.testing.assert_allclose(out[:, :404], R["np_live"], rtol=0, atol=2e-6)
    assert np.all(out[:, 404:] == out[0, 1500]) and abs(float(out[0, 1500]) - float(R["np_padconst"])) <= 2e-6
    np.testing.assert_allclose(out[:, :404], R["torch_live"], rtol=0, atol=5e-5)
