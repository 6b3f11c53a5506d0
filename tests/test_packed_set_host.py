"""CPU: when `NativeWhisperDecoder.packed()` and `Qwen3Decoder._pack()` build, update or keep their packed operands (native_decoder.PackedSet), and what a
copy of an object that owns a library handle is.  `PackedLinear` and `PackedBatch` are replaced by fakes that record every construction and every update,
so nothing here touches libawt: a mistake in this logic does not crash on the GPU, it trains on stale planes."""
import copy
import pickle

import pytest
import torch
import torch.nn as nn

from mlx8_ws_audio_transformer_amd import music2midi as m2m
from mlx8_ws_audio_transformer_amd import native_decoder as nd


@pytest.fixture
def log(monkeypatch):
    """[("new" | "update", fake)] in call order; the fakes take exactly the arguments the real classes take."""
    events = []

    class FakeLinear:
        def __init__(self, weight, bias, precision="bf16x3", backward=True):
            self.backward = backward
            events.append(("new", self))

        def update(self, weight, bias):
            events.append(("update", self))

    class FakeBatch:
        def __init__(self, b):
            events.append(("new", self))

        def update(self, b):
            events.append(("update", self))

    monkeypatch.setattr(nd, "PackedLinear", FakeLinear)
    monkeypatch.setattr(nd, "PackedBatch", FakeBatch)
    monkeypatch.setattr(m2m, "PackedLinear", FakeLinear, raising=False)
    return events


def _whisper():
    return nd.NativeWhisperDecoder(128, 2, 2, 256, vocab=64, max_target_positions=16, train_base=True)


def _qwen(trainable_layers=1, tied=True):
    cfg = m2m.Qwen3Config(vocab_size=64, hidden_size=128, intermediate_size=128, num_hidden_layers=2, num_attention_heads=2, num_key_value_heads=1,
                          rms_norm_eps=1e-6, rope_theta=1e6, tie_word_embeddings=tied, max_position_embeddings=32)
    return m2m.Qwen3Decoder(cfg, trainable_layers=trainable_layers)


def _objects(pk):
    out = [v for k, v in pk.items() if not isinstance(v, list)]
    for group in (v for v in pk.values() if isinstance(v, list)):
        for slot in group:
            out += list(slot.values())
    return out


def _bump(p):
    with torch.no_grad():
        p.add_(1.0)


def _updated(log, pk):
    """The updates recorded in `log` as paths into pk, in call order; fails if anything was built."""
    assert all(kind == "update" for kind, _ in log), "an object was rebuilt"
    where = {id(v): (name,) for name, v in pk.items() if not isinstance(v, list)}
    for name, group in pk.items():
        if isinstance(group, list):
            for i, slot in enumerate(group):
                where.update({id(v): (name, i, k) for k, v in slot.items()})
    return [where[id(obj)] for _, obj in log]


# ------------------------------------------------------------------------------------------------ the tracker's contract, on the Whisper decoder
def test_whisper_builds_once_and_keeps_the_dict(log):
    dec = _whisper()
    pk = dec.packed()
    assert set(pk) == {"layers", "cross_heads", "ckv", "vocab"}
    assert [set(s) for s in pk["layers"]] == [{"qkv", "so", "cq", "co", "fc1", "fc2"}] * 2 and [set(s) for s in pk["cross_heads"]] == [{"k", "kT", "v", "vT"}] * 2
    assert len(log) == 22 and all(kind == "new" for kind, _ in log) and {id(o) for _, o in log} == {id(o) for o in _objects(pk)}
    del log[:]
    assert dec.packed() is pk and dec.packed() is pk and log == []


def test_whisper_in_place_change_updates_the_owners_in_plan_order(log):
    dec = _whisper()
    pk = dec.packed()
    objects = _objects(pk)
    for param, want in ((dec.layers[1].fc1.bias, [("layers", 1, "fc1")]),
                        (dec.layers[0].encoder_attn.v_proj.weight, [("cross_heads", 0, "v"), ("cross_heads", 0, "vT"), ("ckv",)]),
                        (dec.layers[0].self_attn.k_proj.weight, [("layers", 0, "qkv")]),
                        (dec.embed_tokens.weight, [("vocab",)]),
                        (dec.layers[0].final_layer_norm.weight, []),
                        (dec.embed_positions.weight, [])):
        del log[:]
        _bump(param)
        assert dec.packed() is pk and _updated(log, pk) == want
        assert all(a is b for a, b in zip(_objects(pk), objects))
        del log[:]
        assert dec.packed() is pk and log == []


def test_whisper_two_changes_update_each_owner_once(log):
    dec = _whisper()
    pk = dec.packed()
    del log[:]
    for p in (dec.layers[0].encoder_attn.v_proj.bias, dec.layers[1].encoder_attn.k_proj.weight, dec.layers[1].fc2.weight):
        _bump(p)
    assert dec.packed() is pk
    assert _updated(log, pk) == [("layers", 1, "fc2"), ("cross_heads", 1, "k"), ("cross_heads", 1, "kT"), ("ckv",)]


@pytest.mark.parametrize("how", ["replace", "load_state_dict", "apply"])
def test_whisper_new_parameter_objects_rebuild_everything(log, how):
    dec = _whisper()
    pk = dec.packed()
    old = _objects(pk)
    del log[:]
    if how == "replace":
        dec.layers[0].fc1.weight = nn.Parameter(dec.layers[0].fc1.weight.detach().clone())
    elif how == "load_state_dict":
        dec.load_state_dict(dec.state_dict())
    else:
        dec.float()
    pk2 = dec.packed()
    assert pk2 is not pk and len(log) == 22 and all(kind == "new" for kind, _ in log)
    assert not {id(o) for o in _objects(pk2)} & {id(o) for o in old}
    del log[:]
    assert dec.packed() is pk2 and log == []


def test_whisper_watches_the_base_parameters_only_in_one_walk(log):
    from mlx8_ws_audio_transformer_amd.weights import LoraSpec
    dec = nd.NativeWhisperDecoder(128, 2, 2, 256, vocab=64, max_target_positions=16, lora=LoraSpec(r=4, alpha=8.0, targets=("q_proj", "v_proj")))
    pk = dec.packed()
    del log[:]
    _bump(dec.layers[0].self_attn.q_proj.lora_A)
    _bump(dec.layers[1].encoder_attn.v_proj.lora_B)
    assert dec.packed() is pk and log == []
    walks, walk = [], dec.named_parameters
    dec.named_parameters = lambda *a, **kw: (walks.append(1), walk(*a, **kw))[1]
    assert dec.packed() is pk and len(walks) == 1


# ------------------------------------------------------------------------------------------------ the same contract, on the Qwen3 decoder
def test_qwen_trainable_follows_in_place_changes(log):
    dec = _qwen(trainable_layers=1)
    pk = dec._pack()
    assert set(pk) == {"layers", "lm_head"} and [set(s) for s in pk["layers"]] == [{"qkv", "o", "gu", "down"}] * 2
    assert len(log) == 9 and all(kind == "new" and obj.backward is True for kind, obj in log)
    del log[:]
    assert dec._pack() is pk and log == []
    for param, want in ((dec.model.layers[1].mlp.up_proj.weight, [("layers", 1, "gu")]),
                        (dec.model.embed_tokens.weight, [("lm_head",)]),
                        (dec.model.layers[0].self_attn.v_proj.weight, [("layers", 0, "qkv")]),
                        (dec.model.layers[1].self_attn.q_norm.weight, []),
                        (dec.model.norm.weight, [])):
        del log[:]
        _bump(param)
        assert dec._pack() is pk and _updated(log, pk) == want
    walks, walk = [], dec.parameters
    dec.parameters = lambda *a, **kw: (walks.append(1), walk(*a, **kw))[1]
    assert dec._pack() is pk and len(walks) == 1


def test_qwen_untied_head_is_its_own_parameter(log):
    dec = _qwen(trainable_layers=0, tied=False)
    pk = dec._pack()
    del log[:]
    _bump(dec.model.embed_tokens.weight)
    assert dec._pack() is pk and log == []
    _bump(dec.lm_head.weight)
    assert dec._pack() is pk and _updated(log, pk) == [("lm_head",)]


@pytest.mark.parametrize("trainable_layers", [None, 1])
@pytest.mark.parametrize("how", ["replace", "load_state_dict", "apply", "resize"])
def test_qwen_rebuilds_after_the_invalidating_calls(log, trainable_layers, how):
    dec = _qwen(trainable_layers)
    pk = dec._pack()
    old = _objects(pk)
    del log[:]
    if how == "replace":
        w = dec.model.layers[0].mlp.down_proj
        w.weight = nn.Parameter(w.weight.detach().clone(), requires_grad=False)
    elif how == "load_state_dict":
        dec.load_state_dict(dec.state_dict())
    elif how == "apply":
        dec.float()
    else:
        dec.resize_token_embeddings(72)
    pk2 = dec._pack()
    if how == "replace" and trainable_layers is None:                      # the inference-only decoder watches nothing (its docstring): packed once
        assert pk2 is pk and log == []
        return
    assert pk2 is not pk and len(log) == 9 and all(kind == "new" and obj.backward is (trainable_layers is not None) for kind, obj in log)
    assert not {id(o) for o in _objects(pk2)} & {id(o) for o in old}
    del log[:]
    assert dec._pack() is pk2 and log == []


def test_qwen_inference_only_packs_once_without_a_walk(log):
    dec = _qwen(trainable_layers=None)
    pk = dec._pack()
    assert len(log) == 9 and all(kind == "new" and obj.backward is False for kind, obj in log)
    del log[:]
    _bump(dec.model.layers[1].mlp.up_proj.weight)
    walks, walk = [], dec.parameters
    dec.parameters = lambda *a, **kw: (walks.append(1), walk(*a, **kw))[1]
    assert dec._pack() is pk and log == [] and walks == []


# ------------------------------------------------------------------------------------------------ copies of handle owners
def _copies(obj):
    return (lambda: copy.copy(obj)), (lambda: copy.deepcopy(obj)), (lambda: pickle.dumps(obj))


def test_packed_linear_cannot_be_copied_or_pickled():
    pl = object.__new__(nd.PackedLinear)
    pl.handle = 0                                                          # falsy: __del__ hands nothing to the library
    for attempt in _copies(pl):
        with pytest.raises(TypeError, match="library handle"):
            attempt()
    with pytest.raises(TypeError, match="library handle"):
        copy.deepcopy({"layers": [{"fc1": pl}]})


def test_awt_comm_cannot_be_copied_or_pickled():
    from mlx8_ws_audio_transformer_amd.dist import AwtComm
    comm = object.__new__(AwtComm)
    comm.handle = 0
    try:
        for attempt in _copies(comm):
            with pytest.raises(TypeError, match="library handle"):
                attempt()
    finally:
        comm.handle = None                                                 # close() frees whatever is not None


@pytest.mark.parametrize("make,pack", [(_whisper, "packed"), (_qwen, "_pack")])
def test_a_decoder_copy_starts_with_an_empty_set(log, make, pack):
    dec = make()
    pk = getattr(dec, pack)()
    built = len(log)
    for clone in (copy.deepcopy(dec), pickle.loads(pickle.dumps(dec)), copy.copy(dec._packed), copy.deepcopy(dec._packed)):
        tracker = clone._packed if isinstance(clone, nn.Module) else clone
        assert isinstance(tracker, nd.PackedSet) and tracker is not dec._packed and tracker.objects is None
    assert len(log) == built and getattr(dec, pack)() is pk and len(log) == built          # the original is untouched
    twin = copy.deepcopy(dec)
    pk2 = getattr(twin, pack)()
    assert pk2 is not pk and len(log) == 2 * built and not {id(o) for o in _objects(pk2)} & {id(o) for o in _objects(pk)}
    assert getattr(dec, pack)() is pk and len(log) == 2 * built


def test_packed_cache_copies_as_empty(log):
    from mlx8_ws_audio_transformer_amd.autograd_ops import PackedCache
    cache, w = PackedCache(), torch.zeros(128, 64)
    fake = cache.get(w, None, "bf16x3")
    assert cache.get(w, None, "bf16x3") is fake and len(cache.items) == 1 and len(log) == 1
    for clone in (copy.copy(cache), copy.deepcopy(cache), pickle.loads(pickle.dumps(cache)), copy.deepcopy({"c": cache})["c"]):
        assert isinstance(clone, PackedCache) and clone.items == {} and clone.items is not cache.items
    assert cache.get(w, None, "bf16x3") is fake and len(log) == 1


def test_an_encoder_copy_starts_without_library_state():
    from mlx8_ws_audio_transformer_amd import weights as wts
    from mlx8_ws_audio_transformer_amd.encoder import NativeWhisperEncoder
    enc = NativeWhisperEncoder(wts.config("mini", True), precision="bf16x3", device="cpu")
    sentinel = object()                                                    # not an integer: nothing could hand it to the library
    enc._handle, enc._comm, enc._ws, enc._grad_flat = sentinel, sentinel, torch.zeros(4), torch.zeros(4)
    enc._synced.update({n: p._version for n, p in enc.named_parameters()})
    enc._param_cache, enc._param_ids, enc._base_layout = list(enc.named_parameters()), enc._epoch[0], [("x", 0, (1,))]
    enc._grad_params, enc._grad_views, enc._grad_fresh = [enc.conv1.weight], [torch.zeros(1)], False
    try:
        fresh = NativeWhisperEncoder(wts.config("mini", True), precision="bf16x3", device="cpu")
        state = ("_handle", "_synced", "_ws", "_param_cache", "_param_ids", "_base_layout", "_grad_flat", "_grad_params", "_grad_views", "_grad_fresh", "_comm")
        for clone in (copy.deepcopy(enc), pickle.loads(pickle.dumps(enc))):
            assert clone._handle is None and clone._synced == {} and clone._synced is not enc._synced
            for name in state:
                assert getattr(clone, name) == getattr(fresh, name), name
            assert clone.precision == "bf16x3" and clone.cfg == enc.cfg and clone._auto_precision is False
            mine, theirs = dict(enc.named_parameters()), dict(clone.named_parameters())
            assert list(mine) == list(theirs)
            assert all(torch.equal(mine[n], theirs[n]) and mine[n] is not theirs[n] for n in mine)
            before, original = clone._epoch[0], enc._epoch[0]
            clone.conv1.weight = nn.Parameter(clone.conv1.weight.detach().clone())     # the copy's leaves bump the copy's epoch, not the original's
            assert clone._epoch[0] > before and enc._epoch[0] == original
        assert enc._handle is sentinel and len(enc._synced) == len(list(enc.parameters())) and enc._comm is sentinel
    finally:
        enc._handle = None
