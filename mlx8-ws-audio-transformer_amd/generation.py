"""Whisper's `generate` for short-form input: prompt, token suppression, greedy and beam search (HF 5.15
`WhisperForConditionalGeneration.generate`, transformers/models/whisper/generation_whisper.py, and `GenerationMixin._sample` /
`_beam_search`, transformers/generation/utils.py).

The reference decodes with `model.generate(input_features)` (AB/wavToWhisper.py:58-59, AB/fineTuneMidiTester.py:34) and
`predict_with_generate` (AB/fineTune.py:172-174), after setting `generation_config.language` / `task` (AB/fineTune.py:132-134).
Per step the next tokens come from one libawt op (include/awt.h awt_op_select_tokens: log-softmax, suppression, running beam scores
and the top 2 x num_beams of a clip's beams in two launches); the native decoder keeps its self-attention keys / values in one
preallocated cache that beam search reorders with awt_op_kv_gather.  The remaining beam bookkeeping is HF's vectorised algorithm as
device tensor ops; a step synchronises with the host once (the stop test).

With `return_timestamps=True`, and for inputs longer than one window, `longform_generate` restates HF's seek loop
(`WhisperGenerationMixin.generate` with timestamps): the selection op then also applies `WhisperTimeStampLogitsProcessor`
(awt_op_select_tokens_ts), each row's rule state derived on the device from the token history the loop already holds.

With `return_token_timestamps=True` every token also gets a time (HF `_extract_token_timestamps`): the decoding steps keep the
cross-attention query rows of the alignment layers, and after each decode call three libawt ops (csrc/alignment.hip) turn them into the
alignment heads' probabilities (awt_op_alignment_weights), the z-scored, median-filtered head mean (awt_op_alignment_matrix) and the DTW
path's first frame per token (awt_op_dtw); `extract_token_timestamps` is the host glue, one synchronisation per decode call.
`dtw_reference` / `alignment_matrix_reference` restate HF's host code for the tests.

What this module does not build raises: sampling and temperature fallback, num_return_sequences > 1, num_beams > 8, beam search on the
torch decoder, prompt_ids, condition_on_prev_tokens, token timestamps without timestamp tokens, grouping tokens into words.
"""
from __future__ import annotations

import copy
import json
import os
from typing import Callable, List, Optional, Sequence

import torch

from . import _lib

MAX_BEAMS = 8
TASK_IDS = ["translate", "transcribe"]
# HF's TO_LANGUAGE_CODE (transformers/models/whisper/tokenization_whisper.py): language names -> codes, for `language="english"` etc.
TO_LANGUAGE_CODE = {
    "english": "en", "chinese": "zh", "german": "de", "spanish": "es", "russian": "ru", "korean": "ko", "french": "fr", "japanese": "ja",
    "portuguese": "pt", "turkish": "tr", "polish": "pl", "catalan": "ca", "dutch": "nl", "arabic": "ar", "swedish": "sv", "italian": "it",
    "indonesian": "id", "hindi": "hi", "finnish": "fi", "vietnamese": "vi", "hebrew": "he", "ukrainian": "uk", "greek": "el", "malay": "ms",
    "czech": "cs", "romanian": "ro", "danish": "da", "hungarian": "hu", "tamil": "ta", "norwegian": "no", "thai": "th", "urdu": "ur",
    "croatian": "hr", "bulgarian": "bg", "lithuanian": "lt", "latin": "la", "maori": "mi", "malayalam": "ml", "welsh": "cy", "slovak": "sk",
    "telugu": "te", "persian": "fa", "latvian": "lv", "bengali": "bn", "serbian": "sr", "azerbaijani": "az", "slovenian": "sl",
    "kannada": "kn", "estonian": "et", "macedonian": "mk", "breton": "br", "basque": "eu", "icelandic": "is", "armenian": "hy",
    "nepali": "ne", "mongolian": "mn", "bosnian": "bs", "kazakh": "kk", "albanian": "sq", "swahili": "sw", "galician": "gl",
    "marathi": "mr", "punjabi": "pa", "sinhala": "si", "khmer": "km", "shona": "sn", "yoruba": "yo", "somali": "so", "afrikaans": "af",
    "occitan": "oc", "georgian": "ka", "belarusian": "be", "tajik": "tg", "sindhi": "sd", "gujarati": "gu", "amharic": "am",
    "yiddish": "yi", "lao": "lo", "uzbek": "uz", "faroese": "fo", "haitian creole": "ht", "pashto": "ps", "turkmen": "tk", "nynorsk": "nn",
    "maltese": "mt", "sanskrit": "sa", "luxembourgish": "lb", "myanmar": "my", "tibetan": "bo", "tagalog": "tl", "malagasy": "mg",
    "assamese": "as", "tatar": "tt", "hawaiian": "haw", "lingala": "ln", "hausa": "ha", "bashkir": "ba", "javanese": "jw",
    "sundanese": "su", "cantonese": "yue", "burmese": "my", "valencian": "ca", "flemish": "nl", "haitian": "ht", "letzeburgesch": "lb",
    "pushto": "ps", "panjabi": "pa", "moldavian": "ro", "moldovan": "ro", "sinhalese": "si", "castilian": "es", "mandarin": "zh",
}

FIELDS = ("decoder_start_token_id", "pad_token_id", "eos_token_id", "max_length", "num_beams", "length_penalty", "early_stopping",
          "suppress_tokens", "begin_suppress_tokens", "forced_decoder_ids", "language", "task", "lang_to_id", "task_to_id",
          "no_timestamps_token_id", "is_multilingual")
PROMPT_FIELDS = ("lang_to_id", "task_to_id", "no_timestamps_token_id", "forced_decoder_ids")


class GenerationConfig:
    """The fields of `generation_config.json` that Whisper's generate reads; settable attributes, None = absent.  Other keys of a loaded
    file are kept in `extra` and written back unchanged."""

    def __init__(self, **kw):
        for f in FIELDS:
            setattr(self, f, None)
        self.num_beams, self.length_penalty, self.early_stopping = 1, 1.0, False
        self.extra = {}
        for k, v in kw.items():
            if k in FIELDS:
                setattr(self, k, v)
            else:
                self.extra[k] = v

    @property
    def whisper_prompt(self) -> bool:
        """Whether generate builds Whisper's prompt and returns only the generated tokens (any prompt field set)."""
        return any(getattr(self, f) is not None for f in PROMPT_FIELDS)

    def to_dict(self) -> dict:
        out = dict(self.extra)
        out.update({f: getattr(self, f) for f in FIELDS if getattr(self, f) is not None})
        return out

    @classmethod
    def from_dict(cls, d: dict) -> "GenerationConfig":
        return cls(**copy.deepcopy(d))

    @classmethod
    def from_json_file(cls, path: str) -> "GenerationConfig":
        with open(path) as f:
            return cls.from_dict(json.load(f))

    def save(self, directory: str) -> str:
        path = os.path.join(directory, "generation_config.json")
        with open(path, "w") as f:
            json.dump(self.to_dict(), f, indent=2, sort_keys=True)
        return path

    def __repr__(self):
        return f"GenerationConfig({self.to_dict()})"


def set_language_and_task(gc: GenerationConfig, language, task, is_multilingual) -> None:
    """`WhisperGenerationMixin._set_language_and_task` (None fields count as absent)."""
    if is_multilingual is not None:
        gc.is_multilingual = is_multilingual
    if gc.is_multilingual is not None and not gc.is_multilingual and (task is not None or language is not None):
        raise ValueError("Cannot specify `task` or `language` for an English-only model. If the model is intended to be multilingual, pass "
                         "`is_multilingual=True` to generate, or update the generation config.")
    if language is not None:
        if gc.lang_to_id is None:
            raise ValueError("The generation config has no `lang_to_id`, so the `language` argument is not supported: add Whisper's "
                             "`lang_to_id` / `task_to_id` / `no_timestamps_token_id` to generation_config.json.")
        gc.language = language
    if task is not None:
        if gc.task_to_id is None:
            raise ValueError("The generation config has no `task_to_id`, so the `task` argument is not supported.")
        gc.task = task


def _language_to_id(gc: GenerationConfig, language: str) -> int:
    language = language.lower()
    if language in gc.lang_to_id:
        token = language
    elif language in TO_LANGUAGE_CODE:
        token = f"<|{TO_LANGUAGE_CODE[language]}|>"
    elif language in TO_LANGUAGE_CODE.values():
        token = f"<|{language}|>"
    else:
        is_code = len(language) == 2
        raise ValueError(f"Unsupported language: {language}. Language should be one of:"
                         f" {list(TO_LANGUAGE_CODE.values()) if is_code else list(TO_LANGUAGE_CODE.keys())}.")
    if token not in gc.lang_to_id:
        raise ValueError(f"{token} is not supported by this specific model as it is not in the `generation_config.lang_to_id`. "
                         "(You should just add it to the generation config)")
    return int(gc.lang_to_id[token])


def retrieve_init_tokens(gc: GenerationConfig, batch_size: int, detect: Optional[Callable[[], Sequence[int]]] = None,
                         return_timestamps: bool = False) -> List[List[int]]:
    """`WhisperGenerationMixin._retrieve_init_tokens`: the per-clip prompt.  `detect()` returns the detected language ids of the clips
    (called only when the language is unset on a config with `lang_to_id`).  With timestamps, <|notimestamps|> is left out."""
    task, language = gc.task, gc.language
    init = [gc.decoder_start_token_id]
    if task is None and language is None and gc.forced_decoder_ids is not None:
        forced = [list(f) for f in gc.forced_decoder_ids]
        if forced and forced[0][0] == 1:
            i = 1
            while forced and forced[0][0] == i:
                init.append(forced[0][1])
                forced = forced[1:]
                i += 1
            if forced:
                raise ValueError(f"You are using token ids in `forced_decoder_ids` that do not seem to correctly follow the prompt pattern of "
                                 f"Whisper. Make sure that {forced} has an entry for all indices >= 1 and < {forced[0][0]}.")
    lang_undefined = len(init) <= 1 or init[1] is None
    if isinstance(language, (list, tuple)):
        if any(l is None for l in language):
            raise TypeError("Expected `language` to be `None`, a single string (e.g. `'en'`), or a list of strings with length equal to the "
                            "batch size (e.g. `('en', 'fr')` for a batch size of 2). Got a list containing `None`.")
        if len(language) != batch_size:
            raise ValueError("When passing a list of languages, the length of the list must match the batch size. "
                             f"Expected length of {batch_size}, but got {len(language)} languages.")
        languages = list(language)
    elif language is None:
        languages = [None] * batch_size
    else:
        languages = [language]
    inits = [list(init) for _ in languages]
    lang_ids = None
    if language is not None:
        lang_ids = [_language_to_id(gc, l) for l in languages]
    elif gc.lang_to_id is not None and lang_undefined:
        if detect is None:
            raise ValueError("language detection needs the input features")
        lang_ids = [int(t) for t in detect()]
    if lang_ids is not None:
        for i in range(len(inits)):
            if len(inits[i]) > 1:
                inits[i][1] = lang_ids[i]
            else:
                inits[i].append(lang_ids[i])
    for i in range(len(inits)):
        if task is not None:
            if task not in TASK_IDS:
                raise ValueError(f"The `{task}` task is not supported. The task should be one of `{TASK_IDS}`")
            task_id = int(gc.task_to_id[task])
            inits[i].append(task_id)                   # (HF's replace_or_add after this append finds the id and changes nothing)
        elif language is not None and gc.task_to_id is not None:
            if not any(int(t) in inits[i] for t in gc.task_to_id.values()):
                inits[i].append(int(gc.task_to_id["transcribe"]))
        if not return_timestamps and gc.no_timestamps_token_id is not None and inits[i][-1] != gc.no_timestamps_token_id:
            inits[i].append(int(gc.no_timestamps_token_id))
        elif return_timestamps and inits[i][-1] == gc.no_timestamps_token_id:
            inits[i] = inits[i][:-1]
        inits[i] = [int(t) for t in inits[i] if t is not None]
    if len(inits) == 1 and batch_size > 1:
        inits = inits * batch_size
    return inits


# ------------------------------------------------------------------------------------------------ device ops
def banned_bits(tokens, vocab: int, device, invert: bool = False) -> Optional[torch.Tensor]:
    """Bit set over the vocabulary ((vocab + 31) / 32 int32 words) with the given tokens set (invert: every other token); None when empty."""
    toks = sorted({int(t) for t in (tokens or []) if 0 <= int(t) < vocab})
    if not toks and not invert:
        return None
    mask = torch.zeros(((vocab + 31) // 32) * 32, dtype=torch.bool)
    mask[toks] = True
    if invert:
        mask[:vocab] = ~mask[:vocab]
    words = (mask.view(-1, 32).to(torch.int64) << torch.arange(32, dtype=torch.int64)).sum(dim=1)
    words = torch.where(words >= 2 ** 31, words - 2 ** 32, words).to(torch.int32)
    return words.to(device)


class TimestampRules:
    """HF `WhisperTimeStampLogitsProcessor`'s settings: eos (`eos_token_id or bos_token_id`), <|notimestamps|> (timestamps follow it),
    `max_initial_timestamp_index` (None: no clamp) and `begin`, the index of the first generated token in each row's history."""

    def __init__(self, eos_token_id: int, no_timestamps_token_id: int, begin: int, max_initial_timestamp_index: Optional[int] = None):
        self.eos, self.no_ts, self.begin = int(eos_token_id), int(no_timestamps_token_id), int(begin)
        self.mii = -1 if max_initial_timestamp_index is None else int(max_initial_timestamp_index)

    @property
    def timestamp_begin(self) -> int:
        return self.no_ts + 1

    def struct(self, history: torch.Tensor, cur_len: int):
        """The awt_ts_rules of one step: history is a device int64 [rows, >= cur_len] view with unit column stride."""
        import ctypes as C

        class _Rules(C.Structure):
            _fields_ = [("history", C.c_void_p), ("hist_ld", C.c_int64), ("begin", C.c_int), ("cur_len", C.c_int), ("eos_token_id", C.c_int),
                        ("no_timestamps_token_id", C.c_int), ("max_initial_timestamp_index", C.c_int)]
        if history.dtype != torch.int64 or history.stride(-1) != 1:
            raise ValueError("the token history must be int64 with unit column stride")
        ld = history.stride(0) if history.shape[0] > 1 else history.shape[-1]
        return _Rules(history.data_ptr(), int(ld), self.begin, int(cur_len), self.eos, self.no_ts, self.mii)


def select_tokens(logits: torch.Tensor, vocab: int, beams: int = 1, banned: Optional[torch.Tensor] = None, beam_scores: Optional[torch.Tensor] = None,
                  log_softmax: bool = False, k: int = 1, rules: Optional[TimestampRules] = None, history: Optional[torch.Tensor] = None,
                  cur_len: int = 0):
    """awt_op_select_tokens on rows of padded logits (a [rows, >= vocab] fp32 view with unit column stride): (scores [clips, k],
    tokens int64 [clips, k], parents int32 [clips, k]).  With `rules`: awt_op_select_tokens_ts on the rows' token history
    ([rows, >= cur_len] int64, the first cur_len tokens live)."""
    if rules is not None:
        import ctypes as C
        rows = logits.shape[0]
        ld = logits.stride(0) if rows > 1 else max(logits.shape[1], vocab + (-vocab) % 4)
        if logits.dtype != torch.float32 or logits.stride(1) != 1 or not logits.is_cuda:
            raise ValueError("select_tokens needs fp32 device logits with unit column stride")
        dev = logits.device
        clips = rows // beams if beams > 0 else 0
        scores = torch.empty((max(clips, 1), k), dtype=torch.float32, device=dev)
        tokens = torch.empty((max(clips, 1), k), dtype=torch.int64, device=dev)
        parents = torch.empty((max(clips, 1), k), dtype=torch.int32, device=dev)
        L = _lib.lib()
        ws = _lib.workspace(L.awt_select_tokens_ts_workspace_bytes(rows, vocab, k), dev)
        st = rules.struct(history, cur_len)
        with torch.cuda.device(dev):
            _lib.check(L.awt_op_select_tokens_ts(_lib.ctx(dev), logits.data_ptr(), int(ld), rows, int(vocab), int(beams), _lib.ptr(banned),
                                                 _lib.ptr(beam_scores), int(bool(log_softmax)), int(k), C.addressof(st), _lib.ptr(scores),
                                                 _lib.ptr(tokens), _lib.ptr(parents), _lib.ptr(ws), ws.numel(), _lib.stream_handle()))
        return scores, tokens, parents
    rows = logits.shape[0]
    ld = logits.stride(0) if rows > 1 else max(logits.shape[1], vocab + (-vocab) % 4)
    if logits.dtype != torch.float32 or logits.stride(1) != 1 or not logits.is_cuda:
        raise ValueError("select_tokens needs fp32 device logits with unit column stride")
    dev = logits.device
    clips = rows // beams if beams > 0 else 0
    scores = torch.empty((max(clips, 1), k), dtype=torch.float32, device=dev)
    tokens = torch.empty((max(clips, 1), k), dtype=torch.int64, device=dev)
    parents = torch.empty((max(clips, 1), k), dtype=torch.int32, device=dev)
    L = _lib.lib()
    ws = _lib.workspace(L.awt_select_tokens_workspace_bytes(rows, vocab, k), dev)
    with torch.cuda.device(dev):
        _lib.check(L.awt_op_select_tokens(_lib.ctx(dev), logits.data_ptr(), int(ld), rows, int(vocab), int(beams), _lib.ptr(banned), _lib.ptr(beam_scores),
                                          int(bool(log_softmax)), int(k), _lib.ptr(scores), _lib.ptr(tokens), _lib.ptr(parents), _lib.ptr(ws), ws.numel(),
                                          _lib.stream_handle()))
    return scores, tokens, parents


# ------------------------------------------------------------------------------------------------ decoders behind one step interface
class _NativeSteps:
    """The native decoder: preallocated self-attention cache, cross-attention keys / values of the B clips shared by their beams."""

    def __init__(self, dec, cross: torch.Tensor, S: int, B: int, Tmax: int):
        self.dec, self.cross, self.S, self.B, self.Tmax = dec, cross, S, B, Tmax
        self.vocab = dec.vocab
        self.cache = None
        self.group = 1
        self.align: Optional["Alignment"] = None        # set: the steps after the prompt keep the alignment layers' cross-attention queries

    def prefill(self, ids: torch.Tensor) -> torch.Tensor:
        from .native_decoder import DecodeCache
        self.cache = DecodeCache(self.dec.n_layers, ids.shape[0], self.Tmax, self.dec.d, ids.device)
        return self.dec.decode_logits(ids, self.cross, self.S, self.cache)

    def expand(self, beams: int) -> None:
        """B-row prompt cache -> B x beams rows (parent r / beams), double-buffered for the per-step reorder."""
        from .native_decoder import DecodeCache
        big = DecodeCache(self.dec.n_layers, self.B * beams, self.Tmax, self.dec.d, self.cache.buf.device, double=True)
        parent = torch.arange(self.B * beams, device=big.buf.device, dtype=torch.int32) // beams
        big.gather(parent, src=self.cache)
        self.cache, self.group = big, beams

    def reorder(self, parent: torch.Tensor) -> None:
        self.cache.gather(parent)

    def step(self, tokens: torch.Tensor) -> torch.Tensor:
        if self.align is not None and self.cache.align_q is None:
            self.cache.keep_queries(self.align.layers)
        return self.dec.decode_logits(tokens[:, None], self.cross, self.S, self.cache, cross_group=self.group)


class _TorchSteps:
    """The stock-PyTorch decoder (native_decoder=False): its own per-layer caches; logits copied into a 4-aligned pitch for the kernel."""

    def __init__(self, dec, hidden: torch.Tensor, cross, autocast):
        self.dec, self.hidden, self.cross, self.autocast = dec, hidden, cross, autocast
        self.vocab = dec.embed_tokens.weight.shape[0]
        self.caches = [dict() for _ in dec.layers]
        self.pos = 0
        if self.cross is None:
            self.cross = [(l.encoder_attn.k_proj(hidden), l.encoder_attn.v_proj(hidden)) for l in dec.layers]

    def _logits(self, ids):
        with torch.autocast("cuda", dtype=self.autocast or torch.bfloat16, enabled=self.autocast is not None):
            lg = self.dec(ids, self.hidden, cross=self.cross, caches=self.caches, position_offset=self.pos)
        self.pos += ids.shape[1]
        last = lg[:, -1].float()
        out = torch.empty((last.shape[0], self.vocab + (-self.vocab) % 4), dtype=torch.float32, device=last.device)
        out[:, : self.vocab].copy_(last)
        return out

    def prefill(self, ids):
        return self._logits(ids)

    def step(self, tokens):
        return self._logits(tokens[:, None])


# ------------------------------------------------------------------------------------------------ decoding loops
def greedy(steps, init: torch.Tensor, max_len: int, eos_id: Optional[int], pad_id: int, suppress, begin_suppress,
           rules: Optional[TimestampRules] = None) -> torch.Tensor:
    """`GenerationMixin._sample` without sampling: [B, <= max_len] ids starting with the prompt; finished rows continue with pad.
    `rules`: Whisper's timestamp rules, applied from the history in `ids`."""
    B, P = init.shape
    dev = init.device
    vocab = steps.vocab
    ban = banned_bits(suppress, vocab, dev)
    ban0 = banned_bits(list(suppress or []) + list(begin_suppress or []), vocab, dev)
    ids = init
    done = torch.zeros(B, dtype=torch.bool, device=dev)
    if ids.shape[1] >= max_len:
        return ids
    logits = steps.prefill(init)
    first = True
    while True:
        _, nxt, _ = select_tokens(logits, vocab, banned=ban0 if first else ban, rules=rules, history=ids, cur_len=ids.shape[1])
        nxt = nxt[:, 0]
        first = False
        nxt = torch.where(done, torch.full_like(nxt, pad_id), nxt)
        ids = torch.cat([ids, nxt[:, None]], dim=1)
        if eos_id is not None:
            done = done | (nxt == eos_id)
        if ids.shape[1] >= max_len or bool(done.all()):
            return ids
        logits = steps.step(nxt)


def beam_search(steps, init: torch.Tensor, max_len: int, eos_id: Optional[int], pad_id: Optional[int], suppress, begin_suppress, num_beams: int,
                length_penalty: float, early_stopping, rules: Optional[TimestampRules] = None, return_beam_indices: bool = False):
    """`GenerationMixin._beam_search` (HF 5.15, vectorised) on device tensors: (sequences [B, P + generated], sequences_scores [B], generated
    length of each returned hypothesis [B], EOS included).  return_beam_indices: a fourth element, HF's `beam_indices` [B, generated]
    (int64): the row of the B x num_beams batch whose logits produced each token of the returned hypothesis, -1 after its end."""
    B, P = init.shape
    dev = init.device
    nb, vocab = num_beams, steps.vocab
    n_eos = 0 if eos_id is None else 1
    k = max(2, 1 + n_eos) * nb
    top_mask = torch.cat([torch.ones(nb, dtype=torch.bool), torch.zeros(k - nb, dtype=torch.bool)]).to(dev)
    fill = pad_id if pad_id else (eos_id if eos_id is not None else -1)      # HF: `pad_token_id or eos_token_id[0]`
    ban = banned_bits(suppress, vocab, dev)
    ban0 = banned_bits(list(suppress or []) + list(begin_suppress or []), vocab, dev)
    running_sequences = torch.full((B, nb, max_len), fill, dtype=torch.int64, device=dev)
    running_sequences[:, :, :P] = init[:, None, :]
    sequences = running_sequences.clone()
    running_scores = torch.zeros((B, nb), dtype=torch.float32, device=dev)
    running_scores[:, 1:] = -1e9
    beam_scores = torch.full((B, nb), -1e9, dtype=torch.float32, device=dev)
    finished = torch.zeros((B, nb), dtype=torch.bool, device=dev)
    finished_len = torch.zeros((B, nb), dtype=torch.int64, device=dev)          # generated tokens of each kept hypothesis (HF: beam_indices >= 0)
    heur_unsat = torch.ones((B, 1), dtype=torch.bool, device=dev)
    batch_offset = torch.arange(B, device=dev)[:, None] * nb
    running_beam_indices = beam_indices = None
    if return_beam_indices:
        running_beam_indices = torch.full((B, nb, max_len - P), -1, dtype=torch.int64, device=dev)
        beam_indices = running_beam_indices.clone()
    cur_len = P
    logits = steps.prefill(init)                                                # [B, Np]: every beam of a clip sees the same prompt
    logits = logits.repeat_interleave(nb, dim=0) if nb > 1 else logits.contiguous()
    first = True
    while True:
        topk_log_probs, topk_ids, topk_parent = select_tokens(logits, vocab, nb, ban0 if first else ban, running_scores.reshape(-1), True, k,
                                                              rules=rules, history=running_sequences.view(B * nb, max_len), cur_len=cur_len)
        topk_parent = topk_parent.to(torch.int64)
        topk_sequences = torch.take_along_dim(running_sequences, topk_parent[:, :, None], dim=1)
        topk_sequences[:, :, cur_len] = topk_ids
        hits = torch.full_like(topk_ids, cur_len + 1 >= max_len, dtype=torch.bool)
        if eos_id is not None:
            hits = hits | (topk_ids == eos_id)
        # running beams of the next step
        topk_running = topk_log_probs + hits.to(torch.float32) * -1.0e9
        nxt = torch.topk(topk_running, k=nb)[1]
        running_sequences = torch.take_along_dim(topk_sequences, nxt[:, :, None], dim=1)
        running_scores = torch.take_along_dim(topk_running, nxt, dim=1)
        if return_beam_indices:
            topk_beam_indices = torch.take_along_dim(running_beam_indices, topk_parent[:, :, None], dim=1)
            topk_beam_indices[:, :, cur_len - P] = topk_parent + batch_offset
            running_beam_indices = torch.take_along_dim(topk_beam_indices, nxt[:, :, None], dim=1)
        parent = (torch.take_along_dim(topk_parent, nxt, dim=1) + batch_offset).reshape(-1)
        # finished hypotheses
        did = hits & top_mask[None, :]
        lp = topk_log_probs / ((cur_len + 1 - P) ** length_penalty)
        full = torch.all(finished, dim=-1, keepdim=True) & (early_stopping is True)
        lp = lp + full.to(torch.float32) * -1.0e9
        lp = lp + (~heur_unsat).to(torch.float32) * -1.0e9
        lp = lp + (~did) * -1.0e9
        merged_idx = torch.topk(torch.cat([beam_scores, lp], dim=1), k=nb)[1]
        sequences = torch.take_along_dim(torch.cat([sequences, topk_sequences], dim=1), merged_idx[:, :, None], dim=1)
        beam_scores = torch.take_along_dim(torch.cat([beam_scores, lp], dim=1), merged_idx, dim=1)
        finished_len = torch.take_along_dim(torch.cat([finished_len, torch.full_like(topk_ids, cur_len + 1 - P)], dim=1), merged_idx, dim=1)
        finished = torch.take_along_dim(torch.cat([finished, did], dim=1), merged_idx, dim=1)
        if return_beam_indices:
            beam_indices = torch.take_along_dim(torch.cat([beam_indices, topk_beam_indices], dim=1), merged_idx[:, :, None], dim=1)
        cur_len += 1
        # early-stop heuristic (HF _check_early_stop_heuristic)
        best_len = (max_len - P) if (early_stopping == "never" and length_penalty > 0.0) else (cur_len - P)
        best_running = running_scores[:, :1] / (best_len ** length_penalty)
        worst_finished = torch.where(finished, torch.min(beam_scores, dim=1, keepdim=True)[0], -1.0e9)
        heur_unsat = heur_unsat & torch.any(best_running > worst_finished, dim=-1, keepdim=True)
        go = torch.any(heur_unsat) & ~(torch.all(finished) & (early_stopping is True)) & ~torch.all(hits)
        if not bool(go):
            break
        if first:
            steps.expand(nb)            # every beam of a clip holds the same prompt, so the first reorder is the expansion (parent r / nb)
        else:
            steps.reorder(parent)
        first = False
        logits = steps.step(running_sequences[:, :, cur_len - 1].reshape(-1))
    gen = int(finished_len[:, 0].max())                                        # HF: generated length of the longest returned hypothesis
    if return_beam_indices:
        return sequences[:, 0, : P + gen], beam_scores[:, 0], finished_len[:, 0], beam_indices[:, 0, :gen]
    return sequences[:, 0, : P + gen], beam_scores[:, 0], finished_len[:, 0]


def strip_prompt(seqs: torch.Tensor, P: int, pad_id: Optional[int], eos_id: Optional[int]) -> torch.Tensor:
    """WhisperGenerationMixin's short-form return: prompt removed; per clip trailing padding (HF counts every pad of the row, one less when
    pad == eos) and a final EOS dropped; right-padded with pad_token_id to the longest clip."""
    rows = []
    for r in seqs[:, P:].cpu():
        if r.numel() and pad_id is not None and int(r[-1]) == pad_id:
            n = int((r == pad_id).sum())
            if pad_id == eos_id:
                n -= 1
            if n:
                r = r[:-n]
        if r.numel() and eos_id is not None and int(r[-1]) == eos_id:
            r = r[:-1]
        rows.append(r)
    width = max((len(r) for r in rows), default=0)
    out = torch.full((len(rows), width), pad_id if pad_id is not None else 0, dtype=torch.int64)
    for i, r in enumerate(rows):
        out[i, : len(r)] = r
    return out.to(seqs.device)


# ------------------------------------------------------------------------------------------------ timestamps and long-form (seek loop)
TIME_PRECISION = 0.02               # seconds per timestamp token
TIME_PRECISION_FEATURES = 0.01      # seconds per log-mel frame
INPUT_STRIDE = 2                    # log-mel frames per encoder position (conv1 stride x conv2 stride)


def strip_generated(row: torch.Tensor, pad_id: Optional[int], eos_id: Optional[int]) -> torch.Tensor:
    """`generate_with_fallback`'s clean-up of one generated row: trailing padding removed (HF counts every pad of the row, one less when
    pad == eos), then a final EOS."""
    if row.numel() and pad_id is not None and int(row[-1]) == pad_id:
        n = int((row == pad_id).sum())
        if pad_id == eos_id:
            n -= 1
        if n:
            row = row[:-n]
    if row.numel() and eos_id is not None and int(row[-1]) == eos_id:
        row = row[:-1]
    return row


def retrieve_segment(seq: torch.Tensor, time_offset: float, timestamp_begin: int, seek_num_frames: int, idx_offset: int,
                     token_timestamps: Optional[torch.Tensor] = None):
    """`WhisperGenerationMixin._retrieve_segment` for one clip's generated tokens (CPU int64): ([{start, end, tokens, idxs}], seek advance
    in frames).  Two consecutive timestamps end a segment; a single final timestamp means no speech after it (seek the whole window);
    otherwise the unfinished tail is dropped and the seek goes to the last timestamp.  token_timestamps: the window's float32 row (prompt
    included); every segment then carries "token_timestamps", its slice plus the window's time offset."""
    if token_timestamps is not None:
        segments, offset = retrieve_segment(seq, time_offset, timestamp_begin, seek_num_frames, idx_offset)
        for d in segments:
            d["token_timestamps"] = token_timestamps[d["idxs"][0]: d["idxs"][1]] + torch.tensor(time_offset, dtype=torch.float64)
        return segments, offset
    ts = seq.ge(timestamp_begin)
    single_ending = ts[-2:].tolist() == [False, True]
    cuts = (torch.where(ts[:-1] & ts[1:])[0] + 1).tolist()
    if cuts:
        segments = []
        if single_ending:
            cuts.append(len(seq))
        else:
            cuts[-1] += 1
        last = 0
        for i, cur in enumerate(cuts):
            is_last = i == len(cuts) - 1
            toks = seq[last:cur]
            start_pos = int(toks[0]) - timestamp_begin
            end_pos = int(toks[-1 if not is_last or single_ending else -2]) - timestamp_begin
            segments.append({"start": time_offset + float(start_pos) * TIME_PRECISION, "end": time_offset + float(end_pos) * TIME_PRECISION,
                             "tokens": toks, "idxs": (idx_offset + last, idx_offset + cur)})
            last = cur
        if single_ending:
            offset = seek_num_frames
        else:
            offset = (int(seq[last - 2]) - timestamp_begin) * INPUT_STRIDE
        return segments, offset
    stamps = seq[ts]
    # HF: a long tensor times python floats is float32 arithmetic, then int()
    last_pos = int(torch.tensor(seek_num_frames, dtype=torch.long) * TIME_PRECISION_FEATURES / TIME_PRECISION)
    if stamps.numel() > 0 and int(stamps[-1]) != timestamp_begin:
        last_pos = float(int(stamps[-1]) - timestamp_begin)
    return [{"start": time_offset, "end": time_offset + last_pos * TIME_PRECISION, "tokens": seq,
             "idxs": (idx_offset, idx_offset + len(seq))}], seek_num_frames


def pad_segments(segments: List[list], pad_id: int, device=None) -> torch.Tensor:
    """The final `_pad_to_max_length`: each clip's segment tokens concatenated, right-padded with pad_token_id to the longest clip."""
    rows = [torch.cat([d["tokens"] for d in segs]) if segs else torch.zeros(0, dtype=torch.int64) for segs in segments]
    width = max((len(r) for r in rows), default=0)
    out = torch.full((len(rows), width), pad_id, dtype=torch.int64)
    for i, r in enumerate(rows):
        out[i, : len(r)] = r
    return out if device is None else out.to(device)


def pad_token_timestamps(rows: List[list], width: int) -> torch.Tensor:
    """`_pad_to_max_length(return_token_timestamps=True)`: each clip's slices concatenated, right-padded to `width` with the row's last
    value (0.0 for a clip without segments)."""
    out = torch.zeros((len(rows), width), dtype=torch.float32)
    for i, parts in enumerate(rows):
        r = torch.cat(parts) if parts else torch.zeros(0, dtype=torch.float32)
        out[i, : len(r)] = r
        if len(r):
            out[i, len(r):] = r[-1]
    return out


def max_frames_and_seek(batch_size: int, attention_mask: Optional[torch.Tensor], total_frames: int, is_shortform: bool):
    """`_retrieve_max_frames_and_seek`."""
    if batch_size > 1 and not is_shortform and attention_mask is None:
        raise ValueError("When doing batched long-form audio transcription, make sure to pass an `attention_mask`. You can retrieve the "
                         "`attention_mask` by doing `processor(audio, ..., return_attention_mask=True)`")
    if batch_size > 1 and not is_shortform:
        max_frames = torch.as_tensor(attention_mask).sum(-1).cpu().to(torch.long)
    else:
        max_frames = torch.ones((batch_size,), dtype=torch.long) * total_frames
    return max_frames, torch.zeros((batch_size,), dtype=torch.long)


def longform_generate(input_features: torch.Tensor, attention_mask, init_tokens: torch.Tensor, gc: GenerationConfig, max_length: int,
                      max_target_positions: int, num_segment_frames: int, decode: Callable, rules: TimestampRules,
                      return_token_timestamps: bool = False, num_frames: Optional[torch.Tensor] = None):
    """HF 5.15 `WhisperGenerationMixin.generate` with `return_timestamps=True` (short-form and long-form): the seek loop over 30 s windows.
    `decode(segment_input [b, mels, window], init [b, P], max_len)` returns the generated rows [b, >= P] (prompt included).  Returns
    (sequences [B, T] on the input's device, segments: per clip a list of {start, end, tokens, idxs, seek}).

    return_token_timestamps: `decode(segment_input, init, max_len, window_frames)` returns (rows, float32 token timestamps of the same
    shape, seconds from the window's start), window_frames the live clips' `num_frames - seek` (None without `num_frames`, HF
    `_set_num_frames` / `_postprocess_outputs`); the segments gain "token_timestamps" and a third result is HF's padded
    `token_timestamps` [B, T] (float32: each clip's segment slices, right-padded with the row's last value, 0.0 for an empty row)."""
    B, total = input_features.shape[0], input_features.shape[-1]
    is_shortform = total <= num_segment_frames
    max_frames, seek = max_frames_and_seek(B, attention_mask, total, is_shortform)
    P = init_tokens.shape[1]
    idx_map = list(range(B))
    feats = input_features
    segments: List[list] = [[] for _ in range(B)]
    tb = rules.timestamp_begin
    raw: List[list] = [[] for _ in range(B)]            # per clip the segments' slices of the windows' token timestamps, without the offset
    while bool((seek < max_frames).any()):
        # _maybe_reduce_batch
        keep = [i for i, prev in enumerate(idx_map) if seek[prev] < max_frames[prev]]
        if len(keep) != len(idx_map):
            feats = feats[keep]
            idx_map = [idx_map[i] for i in keep]
        time_offset = seek.to(torch.float64) * TIME_PRECISION / INPUT_STRIDE
        seek_num_frames = (max_frames - seek).clamp(max=num_segment_frames)
        # _get_input_segment: the window from seek, zero-padded in log-mel space
        seg = torch.zeros((len(idx_map), feats.shape[1], num_segment_frames), dtype=feats.dtype, device=feats.device)
        for i, prev in enumerate(idx_map):
            sl = feats[i, :, int(seek[prev]): int(seek[prev]) + int(seek_num_frames[prev])]    # slice, then zero-pad (HF slices past the end too)
            seg[i, :, : sl.shape[-1]] = sl
        # _set_max_new_tokens_and_length: HF writes the grown max_length back into the generation config every pass
        max_length = min(max_length + min(max_target_positions // 2 - 1, P), max_target_positions)
        ts = None
        if return_token_timestamps:
            window_frames = None if num_frames is None else [int(num_frames[prev]) - int(seek[prev]) for prev in idx_map]
            out, ts = decode(seg, init_tokens[idx_map], max_length, window_frames)
            out, ts = out.cpu(), ts.cpu()
        else:
            out = decode(seg, init_tokens[idx_map], max_length).cpu()
        for i, prev in enumerate(idx_map):
            seq = strip_generated(out[i, P:], gc.pad_token_id, gc.eos_token_id)
            segs, offset = retrieve_segment(seq, float(time_offset[prev]), tb, int(seek_num_frames[prev]), P, None if ts is None else ts[i])
            for d in segs:
                d["seek"] = int(seek[prev])             # the window's first frame (openai-whisper's segment "seek")
                if ts is not None:
                    raw[prev].append(ts[i, d["idxs"][0]: d["idxs"][1]])
            seek[prev] += offset
            segments[prev] += segs
    seqs = pad_segments(segments, gc.pad_token_id, input_features.device)
    if return_token_timestamps:
        return seqs, segments, pad_token_timestamps(raw, seqs.shape[1]).to(input_features.device)
    return seqs, segments


# ------------------------------------------------------------------------------------------------ token-level timestamps (cross-attention DTW)
MAX_MEDIAN_WIDTH = 15
MAX_ALIGNMENT_HEADS = 32


class Alignment:
    """`generation_config.alignment_heads` ([layer, head] pairs, in HF's order) and the model config's `median_filter_width`, checked
    against the decoder's shape.  `layers`: the distinct decoder layers, in the order of the kept-query buffer's slots."""

    def __init__(self, alignment_heads, median_filter_width: int, n_layers: int, n_heads: int):
        try:
            heads = [(int(l), int(h)) for l, h in alignment_heads]
        except (TypeError, ValueError):
            raise ValueError(f"generation_config.alignment_heads must be a list of [layer, head] pairs, got {alignment_heads!r}")
        if not heads or len(heads) > MAX_ALIGNMENT_HEADS:
            raise ValueError(f"generation_config.alignment_heads must hold between 1 and {MAX_ALIGNMENT_HEADS} [layer, head] pairs, got {len(heads)}")
        for l, h in heads:
            if not (0 <= l < n_layers and 0 <= h < n_heads):
                raise ValueError(f"generation_config.alignment_heads: [{l}, {h}] is out of range for a decoder of {n_layers} layers with {n_heads} heads")
        w = median_filter_width
        if not isinstance(w, int) or isinstance(w, bool) or w <= 0 or w % 2 != 1 or w > MAX_MEDIAN_WIDTH:
            raise ValueError(f"median_filter_width must be an odd number between 1 and {MAX_MEDIAN_WIDTH}, got {w!r}")
        self.heads, self.width, self.n_layers = heads, w, n_layers
        self.layers = sorted({l for l, _ in heads})
        self._table = None

    def table(self, device) -> torch.Tensor:
        """Device int32 [n_sel, 3]: (slot in the kept-query buffer, decoder layer, head)."""
        if self._table is None or self._table.device != torch.device(device):
            slot = {l: s for s, l in enumerate(self.layers)}
            self._table = torch.tensor([[slot[l], l, h] for l, h in self.heads], dtype=torch.int32).to(device)
        return self._table


def dtw_reference(matrix, return_cost: bool = False):
    """HF `_dynamic_time_warping` (generation_whisper.py:64-115) on the host: (text_indices, time_indices) of the cheapest monotone path
    through `matrix` [tokens, frames].  The cost array is float32; a cell is float32(float64(matrix) + float64(c)), c the smallest of
    diagonal / up / left: strictly smaller than both others wins, diagonal tested first, then up, otherwise left.  return_cost: the
    float32 cost array [tokens + 1, frames + 1] as a third result."""
    import numpy as np
    matrix = np.asarray(matrix, dtype=np.float64)
    n, m = matrix.shape
    cost = np.full((n + 1, m + 1), np.inf, dtype=np.float32)
    trace = np.full((n + 1, m + 1), -1, dtype=np.int8)
    cost[0, 0] = 0
    with np.errstate(invalid="ignore", over="ignore"):
        for i in range(1, n + 1):                       # row by row instead of HF's column by column: every cell sees the same three neighbours
            up = cost[i - 1]
            row = cost[i]
            mrow = matrix[i - 1]
            trow = trace[i]
            left = row[0]
            for j in range(1, m + 1):
                c0, c1 = up[j - 1], up[j]
                if c0 < c1 and c0 < left:
                    c, t = c0, 0
                elif c1 < c0 and c1 < left:
                    c, t = c1, 1
                else:
                    c, t = left, 2
                left = np.float32(mrow[j - 1] + np.float64(c))
                row[j] = left
                trow[j] = t
    trace[0, :] = 2
    trace[:, 0] = 1
    i, j = n, m
    text, time = [], []
    while i > 0 or j > 0:
        text.append(i - 1)
        time.append(j - 1)
        t = trace[i, j]
        if t == 0:
            i, j = i - 1, j - 1
        elif t == 1:
            i -= 1
        else:
            j -= 1
    path = np.array(text, dtype=np.int64)[::-1], np.array(time, dtype=np.int64)[::-1]
    return path + (cost,) if return_cost else path


def alignment_matrix_reference(weights: torch.Tensor, width: int) -> torch.Tensor:
    """Steps 4-5 of `_extract_token_timestamps` in HF's torch ops and order: weights [..., heads, tokens, frames] -> [..., tokens, frames]:
    z-score over tokens (population std), median of `width` along frames with reflect padding (unfiltered when frames <= width // 2),
    mean over heads."""
    if width <= 0 or width % 2 != 1:
        raise ValueError("`filter_width` should be an odd number")
    std = torch.std(weights, dim=-2, keepdim=True, unbiased=False)
    mean = torch.mean(weights, dim=-2, keepdim=True)
    w = (weights - mean) / std
    pad = width // 2
    if w.shape[-1] > pad:
        lead = w.shape[:-2]
        w = torch.nn.functional.pad(w.reshape((-1,) + w.shape[-2:])[None], (pad, pad, 0, 0), mode="reflect")[0].reshape(lead + (w.shape[-2], -1))
        w = w.unfold(-1, width, 1).sort()[0][..., pad]
    return w.mean(dim=-3)


def alignment_weights(q: torch.Tensor, cross_kv: torch.Tensor, n_layers: int, S: int, table: torch.Tensor, clips: int, group: int, t0: int,
                      T: int, frames: int, src_row: Optional[torch.Tensor] = None) -> torch.Tensor:
    """awt_op_alignment_weights: q [slots, rows, Tmax, d] kept queries, cross_kv the `cross_kv` tensor -> fp32 [clips, n_sel, T, frames]."""
    slots, rows, Tmax, d = q.shape
    out = torch.empty((clips, table.shape[0], T, frames), dtype=torch.float32, device=q.device)
    with torch.cuda.device(q.device):
        _lib.check(_lib.lib().awt_op_alignment_weights(_lib.ctx(q.device), _lib.ptr(q), slots, rows, Tmax, d, int(group), _lib.ptr(cross_kv), int(n_layers),
                                                       int(S), _lib.ptr(table), table.shape[0], _lib.ptr(src_row), int(clips), int(t0), int(T), _lib.ptr(out),
                                                       int(frames), _lib.stream_handle()))
    return out


def alignment_matrix(weights: torch.Tensor, width: int, num_frames: Optional[torch.Tensor] = None) -> torch.Tensor:
    """awt_op_alignment_matrix: weights fp32 [clips, heads, T, frames] (+ device int32 frames per clip) -> fp32 [clips, T, frames]."""
    clips, n_sel, T, frames = weights.shape
    out = torch.empty((clips, T, frames), dtype=torch.float32, device=weights.device)
    with torch.cuda.device(weights.device):
        _lib.check(_lib.lib().awt_op_alignment_matrix(_lib.ctx(weights.device), _lib.ptr(weights), clips, n_sel, T, frames, _lib.ptr(num_frames), int(width),
                                                      _lib.ptr(out), _lib.stream_handle()))
    return out


def dtw(matrix: torch.Tensor, num_frames: Optional[torch.Tensor] = None, negate: bool = True):
    """awt_op_dtw on fp32 [clips, T, frames] (negate: of -matrix, as HF calls it): (jump_frame int32 [clips, T], text_idx, time_idx int32
    [clips, T + frames], path_start int32 [clips]); clip c's path is text_idx[c, path_start[c]:] / time_idx[c, path_start[c]:]."""
    clips, T, frames = matrix.shape
    dev = matrix.device
    jump = torch.empty((clips, T), dtype=torch.int32, device=dev)
    text = torch.empty((clips, T + frames), dtype=torch.int32, device=dev)
    time = torch.empty((clips, T + frames), dtype=torch.int32, device=dev)
    start = torch.empty((clips,), dtype=torch.int32, device=dev)
    L = _lib.lib()
    ws = _lib.workspace(L.awt_dtw_workspace_bytes(clips, T, frames), dev)
    with torch.cuda.device(dev):
        _lib.check(L.awt_op_dtw(_lib.ctx(dev), _lib.ptr(matrix), clips, T, frames, _lib.ptr(num_frames), int(bool(negate)), _lib.ptr(jump), _lib.ptr(text),
                                _lib.ptr(time), _lib.ptr(start), _lib.ptr(ws), ws.numel(), _lib.stream_handle()))
    return jump, text, time, start


def alignment_matrix_of(steps, align: Alignment, rows: int, L: int, P: int, window_frames=None, beam_indices: Optional[torch.Tensor] = None):
    """Steps 1-5 of `_extract_token_timestamps` for one decode call on the native decoder: (matrix fp32 [rows, L - 1 - P, frames], device
    int32 frames per clip or None).  `steps`: the `_NativeSteps` that decoded, its cache holding the kept queries."""
    T = L - 1 - P
    S = steps.S
    dev = steps.cross.device
    nf = None
    frames = S
    if window_frames is not None:
        # HF crops to num_frames // 2 (a slice: never more than S).  A window of a single frame would leave nothing to align; keep one frame.
        counts = [min(max(int(n) // 2, 1), S) for n in window_frames]
        frames = max(counts)
        nf = torch.tensor(counts, dtype=torch.int32).to(dev)
    src = None
    if beam_indices is not None:
        # input position P + t was decoded by the row that produced token P + t + 1; after a hypothesis' end (-1) HF gathers row 0 of the batch
        src = beam_indices[:, 1: 1 + T].clamp(min=0).to(torch.int32).contiguous()
    w = alignment_weights(steps.cache.align_q, steps.cross, align.n_layers, S, align.table(dev), rows, steps.group, P, T, frames, src)
    return alignment_matrix(w, align.width, nf), nf


def extract_token_timestamps(steps, align: Alignment, rows: int, L: int, P: int, window_frames=None,
                             beam_indices: Optional[torch.Tensor] = None) -> torch.Tensor:
    """`_extract_token_timestamps` for one decode call: float32 CPU [rows, L], seconds from the window's start: zeros for the P prompt
    tokens, 0.02 x the first frame of each token's stretch of the DTW path, the last value repeated for the final token (whose
    cross-attention no step computed).  Fewer than two generated tokens: all zeros."""
    import numpy as np
    out = torch.zeros((rows, L), dtype=torch.float32)
    T = L - 1 - P
    if T <= 0:
        return out
    matrix, nf = alignment_matrix_of(steps, align, rows, L, P, window_frames, beam_indices)
    jump = dtw(matrix, nf, negate=True)[0].cpu().numpy()                     # the decode call's one host synchronisation for this feature
    times = torch.from_numpy((jump.astype(np.float64) * TIME_PRECISION).astype(np.float32))
    out[:, P: P + T] = times
    out[:, P + T] = times[:, -1]
    return out
