"""The batch fixture of `MusicTranscriptionModel.generate_batch`: three clips over the decoder and adapter of tests/qwen3_reference.py's greedy fixture, and
their float64 greedy tokens from the reference's full-recompute loop (`qr.greedy`).  No tests here (tests/test_generate_batch_host.py checks the conditions
below on the CPU, tests/test_gpu_generate_batch.py decodes the clips on the GPU).

    fixture()            (cfg, state dict, float64 reference adapter, [audio features [1, 130, 128] per clip])
    reference()          per clip (tokens, per-step last-position logits), float64, computed once per process
    eos_case(tokens)     (token, j): a token clip 0 emits first at step j >= 2 and no other clip has emitted by then -- with it as EOS clip 0 stops at step j
                         while the others are still running; None when there is none
    conditions(seed)     whether a seed qualifies: what BATCH_SEED was found with

BATCH_SEED is the first seed, counting from 0, at which `conditions` holds: every step's top-2 logit margin of every clip is at least 10 x the GPU logit
bound (1e-3 max(1, max |logits|), tests/test_gpu_qwen3_decoder.py), `qr.GREEDY_EOS` is never the argmax, the three token lists differ pairwise, and an
EOS case exists.  Found on the CPU by `python -m tests.qwen3_batch_reference`."""
import functools

from tests import qwen3_reference as qr

BATCH_SEED = 296                      # the first seed at which `conditions` holds (tests/test_generate_batch_host.py checks it and the seed before)
CLIPS = 3
PROMPT = [5]
GPU_LOGIT_TOL = 1e-3                  # tests/test_gpu_qwen3_decoder.py OUT_TOL
MARGIN_FACTOR = 10.0                  # tests/test_qwen3_reference_host.py test_greedy_fixture_conditions


def audio(seed=None):
    seed = BATCH_SEED if seed is None else seed
    return [qr.variates(f"batch.audio.{i}", (1, 130, 128), seed) for i in range(CLIPS)]


def fixture(seed=None):
    cfg, sd, adapter, _ = qr.greedy_fixture(qr.GREEDY_SEED)
    return cfg, sd, adapter, audio(seed)


@functools.lru_cache(maxsize=None)
def _model():
    return qr.greedy_fixture(qr.GREEDY_SEED)[:3]


@functools.lru_cache(maxsize=4)
def reference(seed=None):
    """[(tokens, logits [steps, vocab])] per clip, float64 on the CPU."""
    cfg, sd, adapter = _model()
    return [qr.greedy(sd, cfg, adapter, a, PROMPT, qr.GREEDY_STEPS) for a in audio(seed)]


def margins(logits):
    """(smallest top-2 margin over the steps, the GPU logit bound) of one clip's per-step logits."""
    top = logits.topk(2, dim=-1).values
    return float((top[:, 0] - top[:, 1]).min()), GPU_LOGIT_TOL * max(1.0, float(logits.abs().max()))


def eos_case(tokens):
    first = lambda toks, t: toks.index(t) if t in toks else len(toks)
    for j in range(2, len(tokens[0])):
        t = tokens[0][j]
        if first(tokens[0], t) == j and all(first(other, t) > j for other in tokens[1:]):
            return t, j
    return None


def conditions(seed):
    ref = reference(seed)
    tokens = [t for t, _ in ref]
    for toks, logits in ref:
        margin, bound = margins(logits)
        if len(toks) != qr.GREEDY_STEPS or qr.GREEDY_EOS in toks or margin < MARGIN_FACTOR * bound:
            return False
    if any(tokens[i] == tokens[j] for i in range(CLIPS) for j in range(i)):
        return False
    return eos_case(tokens) is not None


if __name__ == "__main__":
    seed = 0
    while not conditions(seed):
        seed += 1
    print("first qualifying seed:", seed, "eos case (token, step):", eos_case([t for t, _ in reference(seed)]))
