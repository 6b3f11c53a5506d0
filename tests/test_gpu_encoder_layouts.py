"""GPU: the encoder's own layouts, pinned number for number -- its three workspace sizes, its gradient counts and the gradient table's offsets.

No kernel is launched: a handle is created (which needs a device) and integer queries are made of it.  The expected values were recorded by running
the same queries (`measure` below) on the library built from the commit BEFORE the encoder's host code moved onto one plane-pair type, one gradient
layout and one carve of the conv-phase planes, and pasting the results in: they are the sizes and offsets callers have always been given.

Every configuration is `weights.config("mini", trimmed=True)` (d 128, 2 layers, S 200: the smallest shape the library accepts).  There the `lse` and
`delta` pieces are 2 * 200 * 4 = 1600 bytes per clip, not a multiple of 256, so a layout that drops a piece's padding changes a number here."""
import ctypes as C

import pytest

from mlx8_ws_audio_transformer_amd import _lib, weights as wts
from mlx8_ws_audio_transformer_amd.encoder import PRECISIONS

pytestmark = pytest.mark.gpu

ALL_TARGETS = ("q_proj", "k_proj", "v_proj", "out_proj", "fc1", "fc2")
# name -> (precision, adapter targets, rank, training, backward precision, train_base)
CONFIGS = {
    "infer_bf16": ("bf16", (), 0, False, None, False),
    "infer_fp16": ("fp16", (), 0, False, None, False),
    "infer_bf16x3": ("bf16x3", (), 0, False, None, False),
    "infer_fp16x3": ("fp16x3", (), 0, False, None, False),
    "infer_f16f8": ("f16f8", (), 0, False, None, False),
    "train_lora_qv_r8": ("bf16x3", ("q_proj", "v_proj"), 8, True, None, False),
    "train_lora_all_r16": ("bf16x3", ALL_TARGETS, 16, True, None, False),
    "train_base": ("bf16x3", (), 0, True, None, True),
    "train_backward_f16f8": ("bf16x3", ("q_proj", "v_proj"), 8, True, "f16f8", False),
}
BATCHES = (1, 3)

# per configuration: awt_encoder_workspace_bytes, awt_audio_encode_workspace_bytes and awt_encoder_train_workspace_bytes at B = 1 and B = 3 (a training
# query of an inference handle returns 0), awt_encoder_lora_grad_count, awt_encoder_base_grad_count
EXPECTED = {
    'infer_bf16': {'encoder_ws': [614400, 1843200], 'audio_ws': [742656, 2227456], 'train_ws': [0, 0], 'lora_grads': 0, 'base_grads': 0},
    'infer_bf16x3': {'encoder_ws': [1126400, 3379200], 'audio_ws': [1254656, 3763456], 'train_ws': [0, 0], 'lora_grads': 0, 'base_grads': 0},
    'infer_f16f8': {'encoder_ws': [1650688, 3903488], 'audio_ws': [1778944, 4287744], 'train_ws': [0, 0], 'lora_grads': 0, 'base_grads': 0},
    'infer_fp16': {'encoder_ws': [614400, 1843200], 'audio_ws': [742656, 2227456], 'train_ws': [0, 0], 'lora_grads': 0, 'base_grads': 0},
    'infer_fp16x3': {'encoder_ws': [1126400, 3379200], 'audio_ws': [1254656, 3763456], 'train_ws': [0, 0], 'lora_grads': 0, 'base_grads': 0},
    'train_backward_f16f8': {'encoder_ws': [1126400, 3379200], 'audio_ws': [1254656, 3763456], 'train_ws': [4543744, 13629696], 'lora_grads': 8192, 'base_grads': 0},
    'train_base': {'encoder_ws': [1126400, 3379200], 'audio_ws': [1254656, 3763456], 'train_ws': [6001920, 18004224], 'lora_grads': 0, 'base_grads': 476672},
    'train_lora_all_r16': {'encoder_ws': [1126400, 3379200], 'audio_ws': [1254656, 3763456], 'train_ws': [6010112, 18028800], 'lora_grads': 73728, 'base_grads': 0},
    'train_lora_qv_r8': {'encoder_ws': [1126400, 3379200], 'audio_ws': [1254656, 3763456], 'train_ws': [4543744, 13629696], 'lora_grads': 8192, 'base_grads': 0},
}
# every row of awt_encoder_base_grad_param for "train_base": (state-dict key, element offset, shape); the other configurations have no rows
EXPECTED_LAYOUT = [
    ('conv1.weight', 0, (128, 80, 3)),
    ('conv1.bias', 30720, (128,)),
    ('conv2.weight', 30848, (128, 128, 3)),
    ('conv2.bias', 80000, (128,)),
    ('layer_norm.weight', 80128, (128,)),
    ('layer_norm.bias', 80256, (128,)),
    ('layers.0.self_attn.q_proj.weight', 80384, (128, 128)),
    ('layers.0.self_attn.k_proj.weight', 96768, (128, 128)),
    ('layers.0.self_attn.v_proj.weight', 113152, (128, 128)),
    ('layers.0.self_attn.q_proj.bias', 129536, (128,)),
    ('layers.0.self_attn.v_proj.bias', 129664, (128,)),
    ('layers.0.self_attn.out_proj.weight', 129792, (128, 128)),
    ('layers.0.self_attn.out_proj.bias', 146176, (128,)),
    ('layers.0.self_attn_layer_norm.weight', 146304, (128,)),
    ('layers.0.self_attn_layer_norm.bias', 146432, (128,)),
    ('layers.0.fc1.weight', 146560, (512, 128)),
    ('layers.0.fc1.bias', 212096, (512,)),
    ('layers.0.fc2.weight', 212608, (128, 512)),
    ('layers.0.fc2.bias', 278144, (128,)),
    ('layers.0.final_layer_norm.weight', 278272, (128,)),
    ('layers.0.final_layer_norm.bias', 278400, (128,)),
    ('layers.1.self_attn.q_proj.weight', 278528, (128, 128)),
    ('layers.1.self_attn.k_proj.weight', 294912, (128, 128)),
    ('layers.1.self_attn.v_proj.weight', 311296, (128, 128)),
    ('layers.1.self_attn.q_proj.bias', 327680, (128,)),
    ('layers.1.self_attn.v_proj.bias', 327808, (128,)),
    ('layers.1.self_attn.out_proj.weight', 327936, (128, 128)),
    ('layers.1.self_attn.out_proj.bias', 344320, (128,)),
    ('layers.1.self_attn_layer_norm.weight', 344448, (128,)),
    ('layers.1.self_attn_layer_norm.bias', 344576, (128,)),
    ('layers.1.fc1.weight', 344704, (512, 128)),
    ('layers.1.fc1.bias', 410240, (512,)),
    ('layers.1.fc2.weight', 410752, (128, 512)),
    ('layers.1.fc2.bias', 476288, (128,)),
    ('layers.1.final_layer_norm.weight', 476416, (128,)),
    ('layers.1.final_layer_norm.bias', 476544, (128,)),
]


def measure(name):
    """The queries of one configuration on the loaded library: {query: value}."""
    precision, targets, rank, training, backward, train_base = CONFIGS[name]
    c, L = wts.config("mini", trimmed=True), _lib.lib()
    bits = 0
    for t in targets:
        bits |= _lib.LORA_BITS[t]
    cfg = _lib.EncoderCfg(c.d_model, c.layers, c.heads, c.ffn, c.n_mels, c.max_source_positions, PRECISIONS[precision], rank, 2.0 * rank, bits, 0,
                          1 if training else 0, PRECISIONS[backward] if backward else 0, 1 if train_base else 0)
    h = C.c_void_p()
    _lib.check(L.awt_encoder_create(_lib.ctx(), C.byref(cfg), C.byref(h)))
    try:
        got = {"encoder_ws": [int(L.awt_encoder_workspace_bytes(h, B)) for B in BATCHES],
               "audio_ws": [int(L.awt_audio_encode_workspace_bytes(h, B)) for B in BATCHES],
               "train_ws": [int(L.awt_encoder_train_workspace_bytes(h, B)) for B in BATCHES],
               "lora_grads": int(L.awt_encoder_lora_grad_count(h)), "base_grads": int(L.awt_encoder_base_grad_count(h)), "layout": []}
        for i in range(L.awt_encoder_base_grad_params(h)):
            nm, off, shape, rk = C.c_char_p(), C.c_size_t(), (C.c_int64 * 3)(), C.c_int()
            _lib.check(L.awt_encoder_base_grad_param(h, i, C.byref(nm), C.byref(off), shape, C.byref(rk)))
            got["layout"].append((nm.value.decode(), int(off.value), tuple(int(shape[j]) for j in range(rk.value))))
    finally:
        L.awt_encoder_destroy(h)
    return got


@pytest.mark.parametrize("name", sorted(CONFIGS))
def test_encoder_queries_return_the_recorded_values(name):
    got = measure(name)
    layout = got.pop("layout")
    print(name, got)
    assert got == EXPECTED[name]
    assert layout == (EXPECTED_LAYOUT if CONFIGS[name][5] else [])
