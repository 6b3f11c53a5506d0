"""Capture-and-replay harness for the promise that include/awt.h makes of every operator: its work goes to the caller's stream, without a
synchronisation, an allocation or a host read of device data.  (A plain module: the cases are in tests/test_gpu_graph_capture.py, the
completeness check of the two tables below in tests/test_graph_capture_coverage_host.py.)

On torch's default stream none of those bugs shows: the legacy null stream orders itself against everything.  Under a HIP-graph capture
all of them do, deterministically:
  * work sent to the null stream during a capture, or a host read of device data, is a capture error;
  * work sent to any other stream is missing from the graph, so a replay on NEW inputs returns the OLD bits (or the NaN pre-fill).

`capture_replay(fn, make_state)` therefore runs `fn` eagerly on two different states A and B, captures it once on A, replays it on B and
asks for the eager B bits, twice.  Every comparison is `torch.equal` on the raw bits; there is no tolerance anywhere.
"""
from __future__ import annotations

import torch

_INT_VIEW = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}
INT_SENTINEL = -77


def bits(t: torch.Tensor) -> torch.Tensor:
    """The tensor's elements as integers of the same width (floating point: so that NaN compares equal to itself and -0 differs from 0)."""
    t = t.detach().contiguous()
    return t.view(_INT_VIEW[t.element_size()]) if t.is_floating_point() else t


def same_bits(a: torch.Tensor, b: torch.Tensor) -> bool:
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(bits(a), bits(b))


def _clone_state(state: dict) -> dict:
    return {k: v.clone() for k, v in state.items()}


def _aliases(t: torch.Tensor, state: dict) -> bool:
    p = t.untyped_storage().data_ptr()
    return any(p == s.untyped_storage().data_ptr() for s in state.values())


def _poison(outs, state: dict) -> None:
    """NaN (integers: a sentinel) into every output that is not a view of a state tensor: what a replay leaves unwritten cannot pass."""
    for o in outs:
        if not _aliases(o, state):
            o.fill_(float("nan") if o.is_floating_point() else INT_SENTINEL)


def _eager(fn, state: dict):
    """fn on a clone of `state`, default stream: (clones of the outputs, clones of every state tensor after the run)."""
    s = _clone_state(state)
    outs = fn(s)
    assert isinstance(outs, tuple) and outs and all(isinstance(o, torch.Tensor) for o in outs), "fn must return a tuple of tensors"
    torch.cuda.synchronize()
    return tuple(o.clone() for o in outs), _clone_state(s)


def _check(what: str, outs, static: dict, want_outs, want_state) -> None:
    assert len(outs) == len(want_outs)
    for i, (got, want) in enumerate(zip(outs, want_outs)):
        assert same_bits(got, want), f"{what}: output {i} differs from the eager run on the same inputs"
    for k in static:
        assert same_bits(static[k], want_state[k]), f"{what}: state tensor {k!r} differs from the eager run on the same inputs"


def capture_replay(fn, make_state, load=None):
    """fn(state) -> tuple of output tensors; make_state(seed) -> dict of device tensors holding every input and every buffer the call
    updates in place.  `load(static, B)` replaces the plain copy of B into the static tensors where a case has to say how B arrives (the
    Qwen3 decode step: only the cache positions in front of the new one).  Returns the graph's outputs after the second replay."""
    A, B = make_state(0), make_state(1)
    assert A.keys() == B.keys() and all(A[k].shape == B[k].shape and A[k].dtype == B[k].dtype and A[k].is_cuda for k in A)
    load = load or (lambda static, src: [static[k].copy_(src[k]) for k in static])
    eager_a, _ = _eager(fn, A)
    eager_b, state_b = _eager(fn, B)
    assert any(not same_bits(a, b) for a, b in zip(eager_a, eager_b)), "the two input states give the same outputs: the case cannot see a stale replay"

    static = _clone_state(A)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fn(static)                                          # warm-up: tables, packed weights and rope tables come into being here
    torch.cuda.current_stream().wait_stream(side)
    for k in static:
        static[k].copy_(A[k])
    torch.cuda.synchronize()

    g = torch.cuda.CUDAGraph()
    try:
        with torch.cuda.graph(g, stream=side):
            outs = fn(static)
    except BaseException:
        torch.cuda.synchronize()                            # the context has ended the capture; nothing is retried
        raise
    assert isinstance(outs, tuple) and len(outs) == len(eager_b)

    for what in ("first replay", "second replay"):
        load(static, B)
        _poison(outs, static)
        g.replay()
        torch.cuda.synchronize()
        _check(what, outs, static, eager_b, state_b)
    return outs


# ---------------------------------------------------------------------------------------------------------------------------------------
# Every awt_* function of include/awt.h with a `void* stream` parameter is in exactly one of these two tables
# (tests/test_graph_capture_coverage_host.py).  COVERED: entry point -> the case of tests/test_gpu_graph_capture.py that captures and
# replays it.
COVERED = {
    "awt_logmel_whisper": "logmel_whisper_abi",
    "awt_logmel_whisper_mels": "logmel_whisper_device",
    "awt_logmel_whisper_signal": "logmel_whisper_longest",
    "awt_logmel_generic": "mel_spectrogram_log",
    "awt_prepare_waveform": "prepare_waveform",
    "awt_encoder_forward": "encoder_forward_mel",
    "awt_encoder_forward_train": "encoder_train_step-lora",
    "awt_encoder_backward": "encoder_backward_abi",
    "awt_encoder_backward_ex": "encoder_train_step-lora",
    "awt_audio_encode": "encode_pcm-f16f8",
    "awt_op_linear": "linear-bf16x3",
    "awt_op_layernorm": "layernorm",
    "awt_op_attention": "attention-bf16x3",
    "awt_op_attention_ex": "attention_ex",
    "awt_op_attention_backward": "attention_backward",
    "awt_op_linear_fused": "linear_fused-f32_resid",
    "awt_weight_update": "packed_linear_update_forward",
    "awt_linear_forward": "packed_linear_forward",
    "awt_linear_decode": "packed_linear_forward_decode-200x64",
    "awt_linear_backward_input": "packed_linear_backward_input",
    "awt_bmm_pack": "bmm_pack_update",
    "awt_bmm": "bmm",
    "awt_bmm_pack_kmajor": "bmm_kmajor",
    "awt_bmm_kmajor": "bmm_kmajor",
    "awt_op_softmax_rows": "softmax_rows",
    "awt_op_softmax_rows_backward": "softmax_rows_backward",
    "awt_op_embed": "embed",
    "awt_op_gelu": "gelu",
    "awt_op_gelu_backward": "gelu_backward",
    "awt_op_layernorm_backward": "layernorm_backward",
    "awt_op_layernorm_param_grad": "layernorm_param_grad",
    "awt_op_column_sums": "column_sums",
    "awt_op_column_sums_ld": "column_sums_ld",
    "awt_op_embed_backward": "embed_backward",
    "awt_op_weight_grad": "weight_grad-plain",
    "awt_op_cross_entropy": "cross_entropy",
    "awt_op_attention_small": "attention_small_abi",
    "awt_op_attention_small_backward": "attention_small_abi",
    "awt_op_attention_small_dropout": "attention_small-dropout",
    "awt_op_attention_small_backward_dropout": "attention_small_backward-dropout",
    "awt_op_cross_attention": "cross_attention-2x2x17x70",
    "awt_op_cross_attention_backward": "cross_attention_backward-2x2x17x70",
    "awt_op_rmsnorm": "rmsnorm",
    "awt_op_qk_norm_rope": "qk_norm_rope",
    "awt_op_causal_attention": "causal_attention-decode",
    "awt_op_silu_mul": "silu_mul",
    "awt_op_causal_attention_lse": "causal_attention_lse",
    "awt_op_causal_attention_backward": "causal_attention_backward",
    "awt_op_rmsnorm_backward": "rmsnorm_backward",
    "awt_op_rmsnorm_param_grad": "rmsnorm_param_grad",
    "awt_op_silu_mul_backward": "silu_mul_backward",
    "awt_op_qk_norm_rope_backward": "qk_norm_rope_backward",
    "awt_op_attention_cached": "attention_cached",
    "awt_op_select_tokens": "select_tokens",
    "awt_op_select_tokens_ts": "select_tokens_ts",
    "awt_op_kv_gather": "kv_gather",
    "awt_op_alignment_weights": "alignment_weights",
    "awt_op_alignment_matrix": "alignment_matrix",
    "awt_op_dtw": "dtw",
    "awt_op_conv1d": "conv1d",
    "awt_op_batchnorm_stats": "batchnorm_stats",
    "awt_op_bn_relu_pool": "bn_relu_pool",
    "awt_op_bn_relu_pool_backward": "bn_relu_pool_backward",
    "awt_op_conv1d_framed": "conv1d_framed",
}

# Creation, upload and weight-set calls, which allocate or synchronise by design, and the communicator's calls, which run on its own
# second stream: entry point -> why it is not part of a captured step.
NOT_ON_THE_HOT_PATH = {
    "awt_encoder_set_weight": "upload: converts into library-owned planes; the f16f8 format reads the fp16-exact flag back and synchronises the stream",
    "awt_weight_create": "creation: hipMalloc and a blocking hipMemset of the planes the handle owns",
    "awt_allreduce_sum_f32": "communicator: RCCL collective between processes, multi-rank only",
    "awt_allreduce_mean_f32": "communicator: RCCL collective between processes, multi-rank only",
}
