"""The conv stem on the live positions only (awt_audio_encode): the host bound `awt_conv_stem_positions` and the
three-rule reconstruction, checked without a GPU against the oracle's conv stem in float64.

Log-mel pads a clip with one constant from frame `live` on.  With P0 = (live + 3) // 2, Sc = P0 + 2 and Tc = 2 Sc, the stem of the first Tc
frames, g[0 .. Sc), gives every position of the full stem: g[p] for p < Sc - 1, g[Sc - 2] for Sc - 1 <= p <= S - 2, g[Sc - 1] for p = S - 1."""
import numpy as np
import pytest
import torch

from mlx8_ws_audio_transformer_amd import _lib, weights as wts
from oracle import encoder as oracle_enc

N_FFT, HOP = 400, 160


def _live(n_valid, T):
    n = min(n_valid, T * HOP)
    return 0 if n <= 0 else min(T, (n + N_FFT // 2 + HOP - 1) // HOP)


def _expected_positions(S, n_valid):
    sc = (_live(n_valid, 2 * S) + 3) // 2 + 2
    return sc if sc < S else S


def _stem(W, mel, S):
    """The oracle's conv stem (conv1 / GELU / stride-2 conv2 / GELU) of mel [1, n_mels, 2 S] in float64, before the positional add: [S, d]."""
    Wz = dict(W)
    Wz["embed_positions.weight"] = np.zeros((S, W["conv1.weight"].shape[0]), dtype=np.float32)
    _, bounds = oracle_enc.encoder_forward(Wz, mel, heads=2, dtype=torch.float64, return_boundaries=True)
    return bounds[0][0]


@pytest.fixture(scope="module")
def stem_weights():
    """Equality is required, but the oracle's float64 stem is not the same arithmetic at every position: its convolution is a library GEMM whose summation
    order depends on where a position falls in the blocking (the same position of a 1508-frame and a 3000-frame input came out 8.9e-16 apart), and its
    elementwise GELU takes a vector or a scalar path by the element's place in memory (one ulp apart).  So the operands make every step exact: integer mel
    frames, integer conv weights that are multiples of 16 in conv1, biases that are multiples of 16 -- every sum is then an integer far below 2^53, exact in
    any order, and every pre-activation is 0 or at least 16 in magnitude, where float64 GELU returns exactly x or 0 on either path."""
    cfg = wts.EncoderConfig(16, 1, 2, 16, 8, 1500, "stem-only")
    W = wts.init_encoder_weights(cfg, 0, "test")
    rng = np.random.default_rng(7)
    W["conv1.weight"] = (16 * rng.integers(-2, 3, W["conv1.weight"].shape)).astype(np.float32)
    W["conv1.bias"] = (16 * rng.integers(-4, 5, W["conv1.bias"].shape)).astype(np.float32)
    W["conv2.weight"] = rng.integers(-2, 3, W["conv2.weight"].shape).astype(np.float32)
    W["conv2.bias"] = (16 * rng.integers(-64, 65, W["conv2.bias"].shape)).astype(np.float32)
    return W


# S = 1500: the issue's lengths; S = 200: the two values either side of the switch to the full path (live = 392 | 393), and a clip whose `live` clamps to T
CASES = [(1500, n) for n in (0, 1, 160, 16000, 63999, 64000, 64001, 240000, 476000, 478000, 478520, 478521, 480000)] + [(200, 62520), (200, 62521), (200, 64000)]


@pytest.mark.parametrize("S,n_valid", CASES)
def test_bound_and_reconstruction_match_the_full_stem(stem_weights, S, n_valid):
    T = 2 * S
    Sc = _lib.conv_stem_positions(S, n_valid)
    assert Sc == _expected_positions(S, n_valid)
    live = _live(n_valid, T)
    assert (Sc == S) == ((live + 3) // 2 + 2 >= S)          # the full path exactly when Sc >= S: no earlier threshold
    rng = np.random.default_rng(S + n_valid)
    mel = rng.integers(-8, 9, (1, 8, T)).astype(np.float64)
    mel[:, :, live:] = -5.0                                   # the padding: one constant, every bin and frame
    full = _stem(stem_weights, mel, S)
    if Sc == S:
        return
    assert full.unique(dim=0).shape[0] > min(S, live // 2)    # the live positions differ from each other: a wrong index cannot hide
    g = _stem(stem_weights, np.ascontiguousarray(mel[:, :, :2 * Sc]), Sc)
    src = torch.arange(S).clamp(max=Sc - 2)
    src[S - 1] = Sc - 1
    assert torch.equal(g[src], full)


def test_known_values():
    assert _lib.conv_stem_positions(1500, 64000) == 204      # 402 live frames
    assert _lib.conv_stem_positions(1500, 1600) == 9
    assert _lib.conv_stem_positions(1500, 476000) == 1492 and _lib.conv_stem_positions(1500, 478000) == 1498
    assert _lib.conv_stem_positions(1500, 480000) == 1500 and _lib.conv_stem_positions(1500, 10 ** 9) == 1500
    assert _lib.conv_stem_positions(1500, 0) == 3 and _lib.conv_stem_positions(1500, -5) == 3
    assert _lib.conv_stem_positions(2, 0) == 2                # an encoder shorter than the smallest compact stem
