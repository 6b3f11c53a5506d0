"""The f16f8 attention forward keeps its arithmetic when its instruction schedule changes: every output below has the bits the kernel
produced when tests/golden/attention_f16f8_sha256.json was recorded (tools/make_golden_attention.py), and stays within the fp64 bound of
tests/test_gpu_ops.py.  A hash that differs means the order of some floating-point operation moved (the row sum's chain, the
l_run * alpha + psum contraction, an accumulator's MFMA order, the running maximum): find which one, do not re-record the file.

Sequence lengths (64-key tiles; B = 1, H = 2): one tile with a partly filled wave (33) and full (64); two, three, ... nine tiles with and
without a tail tile -- every remainder of the tile loop's unroll by two and by six, both forms of the last iteration, and a prologue that
stages one, two and three or more tiles; then 10, 11 and 17 tiles (640, 641, 1025): one and two trips of the loop unrolled by six, which needs
ten tiles to start, followed by zero and one trip of the loop by two and by a remainder of two and of three tiles; and the workload's own 24
tiles (1500) once.  `rescale448` is the input of test_attention_online_softmax_rescale_branch: the running maximum carried from one
iteration to the next changes in every tile.
`pv8_*` pin the two instantiations that keep P V's e4m3 cross terms (attn_shape 4 / 5: four and eight waves), which share the kernel's
source with the inference form.  (The library launches those forms by itself only for a call with lse, and no encoder configuration
reaches that call: training refuses the f16f8 operand format.  The knob runs the same instantiations; their bound is the tighter one
test_attention_f16f8_workgroup_shapes holds them to.)
"""
import hashlib
import json
import os

import pytest
import torch

from tests.test_gpu_ops import ATT_TOL, ATT_TOL_F16F8_CROSS, _rand
from tests.util import GOLD, tuning

pytestmark = pytest.mark.gpu

GOLDEN_FILE = os.path.join(GOLD, "attention_f16f8_sha256.json")

# name -> (B, H, S, attn_shape knob, max-abs bound vs fp64)
CASES = {f"S{S}": (1, 2, S, 0, ATT_TOL["f16f8"]) for S in (33, 64, 65, 128, 191, 192, 256, 320, 321, 384, 385, 448, 512, 513, 640, 641, 1025)}
CASES["S1500"] = (1, 1, 1500, 0, ATT_TOL["f16f8"])
CASES["rescale448"] = (1, 1, 448, 0, ATT_TOL["f16f8"])
for _shape, _S in ((4, 128), (4, 321), (5, 128), (5, 321)):
    CASES[f"pv8_shape{_shape}_S{_S}"] = (1, 2, _S, _shape, ATT_TOL_F16F8_CROSS)


def inputs(name):
    B, H, S, _, _ = CASES[name]
    if name == "rescale448":
        q, k, v = _rand((B, H, S, 64), 10, 0.2), _rand((B, H, S, 64), 11), _rand((B, H, S, 64), 12)
        for t, key in enumerate([70, 150, 260, 390]):
            k[0, 0, key] = q[0, 0, 5] * (20.0 + 15 * t)
        return q, k, v
    return _rand((B, H, S, 64), 7, 0.35), _rand((B, H, S, 64), 8), _rand((B, H, S, 64), 9)


def run(name, q, k, v):
    from mlx8_ws_audio_transformer_amd import ops
    with tuning(attn_shape=CASES[name][3]):
        return ops.attention(q, k, v, "f16f8")


def sha256(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


@pytest.fixture(scope="module")
def recorded():
    with open(GOLDEN_FILE) as f:
        return json.load(f)


def test_every_case_is_recorded(recorded):
    assert set(recorded["sha256"]) == set(CASES)


@pytest.mark.parametrize("name", list(CASES))
def test_attention_f16f8_bits_and_bound(name, recorded):
    B, H, S, _, bound = CASES[name]
    q, k, v = inputs(name)
    o = run(name, q, k, v)
    p = torch.softmax(q.double() @ k.double().transpose(2, 3), dim=-1)
    ref = (p @ v.double()).transpose(1, 2).reshape(B, S, H * 64)
    err = (o.double() - ref).abs().max().item()
    got = sha256(o)
    print(name, (B, H, S), "max-abs", err, "sha256", got)
    assert torch.isfinite(o).all() and err < bound, err
    assert got == recorded["sha256"][name]
