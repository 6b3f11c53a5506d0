"""The plumbing of tests/hostile_alloc.py on the CPU, with plain torch functions: the allocator intercepts what it says it does, and `run_fenced`
refuses each kind of function it exists to catch, with the message of that kind.  Every planted function stays inside the buffers the harness
itself allocated (the 64 KiB guards are part of them), so nothing faults.  Needs no GPU."""
import os
import re

import pytest
import torch

from tests import hostile_alloc as ha
from tests.hostile_alloc import CANARY, GUARD_BYTES, IN_PLACE, POISON, HostileAlloc, fence, run_fenced

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "awt.h")
CPU = torch.device("cpu")


def _state(seed):
    g = torch.Generator().manual_seed(seed + 1)
    return {"x": torch.randn(5, 7, generator=g), "w": torch.randn(7, generator=g)}


def _beyond(t, offset):
    """One element `offset` elements from the start of contiguous `t`, inside or outside it, as a view over its storage."""
    return torch.as_strided(t, (1,), (1,), t.storage_offset() + offset)


# ------------------------------------------------------------------------------------------------------------------- the allocator
FACTORY_CALLS = {
    "empty.memory_format": lambda src: torch.empty(3, 5, dtype=torch.float16),
    "empty_strided": lambda src: torch.empty_strided((3, 5), (5, 1), dtype=torch.bfloat16),
    "empty_like": lambda src: torch.empty_like(src),
    "new_empty": lambda src: src.new_empty((3, 5), dtype=torch.int32),
    "zeros": lambda src: torch.zeros(3, 5),
    "zeros_like": lambda src: torch.zeros_like(src, dtype=torch.int64),
    "new_zeros": lambda src: src.new_zeros((3, 5)),
    "full": lambda src: torch.full((3, 5), 2.5),
    "full_like": lambda src: torch.full_like(src, -3.0),
    "new_full": lambda src: src.new_full((3, 5), 7, dtype=torch.uint8),
}
EXPECT = {"empty.memory_format": torch.float16, "empty_strided": torch.bfloat16, "empty_like": torch.float32, "new_empty": torch.int32,
          "zeros": torch.float32, "zeros_like": torch.int64, "new_zeros": torch.float32, "full": torch.float32, "full_like": torch.float32,
          "new_full": torch.uint8}
VALUE = {"zeros": 0, "zeros_like": 0, "new_zeros": 0, "full": 2.5, "full_like": -3.0, "new_full": 7}


def test_the_factory_list_is_the_one_the_allocator_intercepts():
    assert {f.name().removeprefix("aten::").removesuffix(".default") for f in ha.FACTORIES} == set(FACTORY_CALLS)


@pytest.mark.parametrize("op", list(FACTORY_CALLS))
def test_every_factory_op_is_intercepted(op):
    src = torch.ones(3, 5)
    with HostileAlloc("cpu") as mode:
        t = FACTORY_CALLS[op](src)
    assert len(mode.buffers) == 1 and mode.passed_through == 0, op
    buf = mode.buffers[0]
    assert t.data_ptr() == buf.tensor.data_ptr() and t.shape == (3, 5) and t.dtype == EXPECT[op] and t.device == CPU and t.is_contiguous()
    n = 15 * t.element_size()
    assert t.data_ptr() % 256 == 0 and buf.raw.numel() == 2 * GUARD_BYTES + n                  # exactly n bytes between the guards
    assert t.data_ptr() == buf.raw.data_ptr() + GUARD_BYTES
    assert bool((buf.raw[:GUARD_BYTES] == CANARY).all()) and bool((buf.raw[GUARD_BYTES + n:] == CANARY).all()) and not buf.broken_guards()
    if op in VALUE:
        assert bool((t == VALUE[op]).all())
    else:
        assert bool((buf.raw[GUARD_BYTES:GUARD_BYTES + n] == POISON).all())
        assert bool(torch.isnan(t).all()) if t.is_floating_point() else bool((t == -1).all())


def test_an_odd_byte_count_is_not_rounded_up():
    with HostileAlloc("cpu") as mode:
        t = torch.empty(257, dtype=torch.uint8)
        u = torch.empty(0)
    assert mode.buffers[0].raw.numel() == 2 * GUARD_BYTES + 257 and int(mode.buffers[0].raw[GUARD_BYTES + 257]) == CANARY
    assert t.numel() == 257 and u.numel() == 0 and mode.buffers[1].raw.numel() == 2 * GUARD_BYTES


def test_other_devices_other_layouts_and_other_ops_pass_through():
    src = torch.ones(3, 5)
    with HostileAlloc("meta") as mode:                                                         # every CPU request is one for another device
        for make in FACTORY_CALLS.values():
            t = make(src)
            assert t.device == CPU and t.shape == (3, 5)
        assert bool((torch.zeros(3) == 0).all()) and bool((torch.full((3,), 2.5) == 2.5).all())
    assert not mode.buffers and mode.passed_through == len(FACTORY_CALLS) + 2
    with HostileAlloc("cpu") as mode:
        a = torch.empty(2, 3, 4, 5, memory_format=torch.channels_last)
        b = torch.empty_strided((3, 5), (1, 3))
        c = torch.empty_like(src.t())                                                          # preserve_format of a transposed tensor: not contiguous
        d = src + 1                                                                            # no factory op: its result is torch's own
        e = torch.empty_like(src.t(), memory_format=torch.contiguous_format)
    assert not a.is_contiguous() and b.stride() == (1, 3) and c.stride() == (1, 5)
    assert len(mode.buffers) == 1 and mode.buffers[0].tensor.data_ptr() == e.data_ptr() and e.is_contiguous()
    assert mode.passed_through == 3 and bool((d == 2).all())


def test_fence_copies_the_contents_between_nan_guards():
    plain = _state(0)
    state, bufs = fence(plain, "cpu")
    assert state.keys() == plain.keys() and len(bufs) == 2
    for (k, t), b in zip(state.items(), bufs):
        assert torch.equal(t, plain[k]) and t.data_ptr() % 256 == 0 and t.data_ptr() != plain[k].data_ptr() and k in b.name
        assert bool((b.raw[:GUARD_BYTES] == POISON).all()) and bool((b.raw[GUARD_BYTES + t.numel() * 4:] == POISON).all())
        assert bool(torch.isnan(_beyond(t, t.numel())).all()) and bool(torch.isnan(_beyond(t, -1)).all())


# ------------------------------------------------------------------------------------------------------------------- run_fenced
def _correct(s):
    y = torch.empty(5, dtype=torch.float32)
    torch.mv(s["x"], s["w"], out=y)
    return (y,)


def _room(t):
    """(elements of t's storage in front of t, elements behind it): a plant writes outside its output only where the storage holds that element, which
    is the harness's guard in the hostile run and nothing at all in the plain run (torch.empty's storage ends with the tensor)."""
    return t.storage_offset(), t.untyped_storage().nbytes() // t.element_size() - t.storage_offset() - t.numel()


def _writes_past_the_end(s):
    (y,) = _correct(s)
    if _room(y)[1]:
        _beyond(y, y.numel()).fill_(1.0)
    return (y,)


def _writes_in_front(s):
    (y,) = _correct(s)
    if _room(y)[0]:
        _beyond(y, -1).fill_(1.0)
    return (y,)


def _leaves_an_element_unwritten(s):
    y = torch.empty(5, dtype=torch.float32)
    torch.mv(s["x"][:4], s["w"], out=y[:4])
    return (y,)


def _reads_past_an_input(s):
    (y,) = _correct(s)
    y[4] += _beyond(s["w"], s["w"].numel())[0]                       # the plain run reads whatever follows w in its own storage: guard against that below
    return (y,)


def _scales_an_input(s):
    s["w"].mul_(2.0)
    return _correct(s)


PLANTS = {
    "writes_past_the_end": (_writes_past_the_end, (), "guard bytes overwritten around allocation 0 .*4 byte.s. behind it"),
    "writes_in_front": (_writes_in_front, (), "guard bytes overwritten around allocation 0 .*4 byte.s. in front of it"),
    "leaves_an_element_unwritten": (_leaves_an_element_unwritten, (), "output 0 of the hostile run is not bit-equal to the plain run .*flat index 4: nan"),
    "reads_past_an_input": (_reads_past_an_input, (), "output 0 of the hostile run is not bit-equal to the plain run .*flat index 4: nan"),
    "scales_an_undeclared_input": (_scales_an_input, (), "input 'w' is not declared in_place but changed in the plain run"),
    "declared_in_place_changes_nothing": (_correct, ("w",), "stale IN_PLACE table: 'w' is declared in_place"),
}


def _padded_state(seed):
    """_state with `w` as the front of a longer storage, so that the plain run of reads_past_an_input reads a finite element it owns."""
    st = _state(seed)
    st["w"] = torch.cat([st["w"], torch.ones(1)])[:7]
    return st


@pytest.mark.parametrize("plant", list(PLANTS))
def test_run_fenced_refuses_what_it_exists_to_catch(plant):
    fn, in_place, message = PLANTS[plant]
    with pytest.raises(AssertionError, match=message):
        run_fenced(fn, _padded_state, in_place=in_place, device="cpu")


def test_run_fenced_passes_a_correct_function():
    assert run_fenced(_correct, _state, device="cpu") == 1
    assert run_fenced(_scales_an_input, _state, in_place=("w",), device="cpu") == 1


def test_a_write_outside_a_state_tensor_is_a_guard_failure_too():
    def fn(s):
        if _room(s["x"])[1]:
            _beyond(s["x"], s["x"].numel()).fill_(0.0)
        return _correct(s)
    with pytest.raises(AssertionError, match="guard bytes overwritten around state tensor 'x'"):
        run_fenced(fn, _state, device="cpu")


def test_in_place_must_name_state_tensors():
    with pytest.raises(AssertionError, match="in_place names no state tensor"):
        run_fenced(_correct, _state, in_place=("y",), device="cpu")


# ------------------------------------------------------------------------------------------------------------------- the two tables
def test_the_tables_name_cases_and_exemptions_quote_the_header():
    """IN_PLACE and EXEMPT name cases that exist.  EXEMPT holds at most three entries, and each reason quotes, between double quotes, a sentence of
    include/awt.h: the header itself has to say that the prior content of the buffer is an input."""
    from tests import test_gpu_hostile_alloc as gpu
    names = set(gpu.CASES) | set(gpu.EDGES)
    assert set(IN_PLACE) <= names, sorted(set(IN_PLACE) - names)
    assert all(isinstance(v, tuple) and v and all(isinstance(k, str) for k in v) for v in IN_PLACE.values())
    assert set(gpu.EXEMPT) <= names and len(gpu.EXEMPT) <= 3
    header = " ".join(re.sub(r"^\s*(/\*+|\*+/?|//+)", " ", line) for line in open(HEADER).read().splitlines())
    header = " ".join(header.split())
    for name, reason in gpu.EXEMPT.items():
        assert isinstance(reason, str) and "\n" not in reason, name
        quoted = re.findall(r'"([^"]{20,})"', reason)
        assert quoted and all(" ".join(q.split()) in header for q in quoted), f"{name}: the reason quotes no sentence of include/awt.h"
