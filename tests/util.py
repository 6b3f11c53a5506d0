"""Shared seeded inputs for the parity tests (regenerates exactly what tools/make_golden.py fed the reference), and the tuning-knob context."""
import contextlib
import os

import numpy as np

from mlx8_ws_audio_transformer_amd import synth, weights as wts

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


# the library's defaults of the tuning knobs the tests change (include/awt.h, awt_tuning_set)
TUNING_DEFAULTS = {"gemm_tile": 0, "gemm_pp": 1, "gemm_pp_mask": 12, "gemm_mfma16": 1, "attn_shape": 0, "attn_qt": 0}


@contextlib.contextmanager
def tuning(**knobs):
    """Sets the given tuning knobs for the block; on exit every knob of TUNING_DEFAULTS is back at its library default."""
    from mlx8_ws_audio_transformer_amd import _lib

    unknown = set(knobs) - set(TUNING_DEFAULTS)
    if unknown:
        raise KeyError(f"tuning: no default recorded for {sorted(unknown)}")
    try:
        for key, value in knobs.items():
            _lib.tuning_set(key, value)
        yield
    finally:
        for key, value in TUNING_DEFAULTS.items():
            _lib.tuning_set(key, value)


GUARD = 4096


def guarded(shape, dtype, device="cuda"):
    """(buffer, tensor): a tensor of 0xFF bytes (NaN in every floating-point format) between two 4 KiB guards of 0xA5 bytes.
    For a whole operator call -- inputs, outputs and the workspaces its wrapper allocates -- see tests/hostile_alloc.py (`run_fenced`)."""
    import torch

    n = torch.empty(shape, dtype=dtype).numel() * torch.empty((), dtype=dtype).element_size()
    buf = torch.full((GUARD + n + GUARD,), 0xA5, dtype=torch.uint8, device=device)
    buf[GUARD:GUARD + n] = 0xFF
    inner = buf[GUARD:GUARD + n].view(dtype).view(shape)
    assert inner.data_ptr() % 256 == 0 and (not inner.is_floating_point() or bool(torch.isnan(inner).all()))
    return buf, inner


def guards_intact(buf):
    return bool((buf[:GUARD] == 0xA5).all()) and bool((buf[-GUARD:] == 0xA5).all())


def golden(name):
    return np.load(os.path.join(GOLD, name))


def logmel_inputs():
    noise = (0.1 * wts.unit_variates("f2_noise", 64000, 0)).astype(np.float32)
    tone = synth.tone_noise_clip(0)
    zeros = np.zeros(64000, dtype=np.float32)
    short = tone[:16000].copy()
    piano = synth.pcm_i16_to_f32(synth.synth_clips_i16(1, seed=1234, first=3)[0])
    return {"noise": noise, "tone": tone, "zeros": zeros, "short": short, "piano": piano}


def piano_clips_f32(batch, first=0):
    return [synth.pcm_i16_to_f32(c) for c in synth.synth_clips_i16(batch, seed=1234, first=first)]


def real_audio():
    """(int16 stereo excerpt [64000, 2] of the reference's sample recording, its channel mean as float32, the fixture): tests/golden/real_audio.npz
    (tools/make_golden.py gen_real_audio)."""
    G = golden("real_audio.npz")
    pcm = G["pcm_i16_stereo"]
    return pcm, (pcm.astype(np.float32) / 32768.0).mean(axis=1), G


def mini_at(S):
    """The mini shape at another sequence length: S picks the last-tile, lane-block and tile-count branches of the attention kernels."""
    return wts.EncoderConfig(128, 2, 2, 512, 80, S, f"mini-S{S}")


# (S, batch) of the tests that run the encoder and both backward passes away from S = 200 and 1500 (neither is a multiple of 64), on mini_at(S):
#   S = 8    one key tile with a tail; three of a workgroup's four waves without a query; 16 GEMM rows
#   S = 64   one tile, no tail (the attention backward's no-tail last tile)
#   S = 128  two tiles, no tail, one full 128-row lane block
#   S = 136  three tiles with a tail, a second, partial lane block (batch 3)
#   S = 192  three tiles, no tail
#   S = 256  four tiles, two full lane blocks; the f16f8 attention crosses its (S + 255) / 256 boundary
MINI_LENGTHS = [(8, 2), (64, 2), (128, 2), (136, 3), (192, 2), (256, 2)]


# (n_fft, hop, n_mels) -> (sample_rate, f_min, f_max, n_samples, batch): every n_fft the header promises besides 1024, hop == n_fft and n_fft / 4, one / some / the
# most mel bins, with the other arguments off their defaults in turn: sample rates 22050 and 44100, f_min = 50, f_max below sr / 2, n_samples that are not a
# multiple of hop, the minimum n_samples = n_fft / 2 + 1 (one reflection covers the whole clip), batches of 3.  128 bins over 201 FFT bins (n_fft = 400,
# 16 kHz) include filters that hold no FFT bin: their value is ln(log_eps) in the oracle and in the kernel.
GENERIC_LOGMEL_CASES = {
    (400, 400, 1): (16000, 0.0, 8000.0, 64000, 1),
    (400, 400, 40): (22050, 50.0, 11025.0, 30011, 1),
    (400, 400, 128): (16000, 0.0, 8000.0, 64000, 3),
    (400, 100, 1): (44100, 50.0, 16000.0, 201, 1),
    (400, 100, 40): (16000, 50.0, 7600.0, 12345, 3),
    (400, 100, 128): (44100, 0.0, 22050.0, 30011, 1),
    (512, 512, 1): (22050, 0.0, 8000.0, 257, 1),
    (512, 512, 40): (44100, 50.0, 16000.0, 64000, 3),
    (512, 512, 128): (16000, 50.0, 8000.0, 40001, 1),
    (512, 128, 1): (16000, 0.0, 8000.0, 64000, 1),
    (512, 128, 40): (22050, 50.0, 8000.0, 257, 3),
    (512, 128, 128): (22050, 0.0, 11025.0, 64000, 1),
}


def generic_logmel_clip(n, i=0):
    """Clip i of a GENERIC_LOGMEL_CASES batch: piano notes over a tone and a noise floor -- tonal and broadband content in every frame, the first
    n_fft / 2 + 1 samples included."""
    return (0.5 * piano_clips_f32(1, 7 + i)[0] + 0.5 * synth.tone_noise_clip(i, tone_hz=440.0 * (i + 1)))[:n].astype(np.float32)
