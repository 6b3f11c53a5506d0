"""Completeness of the capture-and-replay suite (tests/graph_capture.py, tests/test_gpu_graph_capture.py); needs no GPU.

include/awt.h is read as text: every awt_* function whose prototype takes a `void* stream` is in exactly one of the two tables of
tests/graph_capture.py -- COVERED (the case that captures and replays it) or NOT_ON_THE_HOT_PATH (creation, upload and communicator calls, with
the reason) -- so that a new operator cannot arrive unclassified.  An entry point whose own header comment promises "no synchronisation" cannot be
in the second table, and every case a COVERED entry names exists in the GPU file."""
import os
import re

from tests.graph_capture import COVERED, NOT_ON_THE_HOT_PATH

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "awt.h")
GPU_FILE = os.path.join(ROOT, "tests", "test_gpu_graph_capture.py")

_TOKEN = re.compile(r"/\*.*?\*/|\b(awt_[a-z0-9_]+)\s*\(([^;{()]*)\)\s*;", re.S)


def stream_entry_points(text):
    """{function: the comment block in front of its prototype} for the prototypes with a `void* stream` parameter.  Prototypes that follow one
    another without a comment between them share the comment in front of the first."""
    out, comment = {}, ""
    for m in _TOKEN.finditer(text):
        if m.group(1) is None:
            comment = m.group(0)
        elif re.search(r"\bvoid\s*\*\s*stream\b", re.sub(r"/\*.*?\*/", "", m.group(2), flags=re.S)):
            out[m.group(1)] = comment
    return out


def test_the_parser_sees_the_header():
    eps = stream_entry_points(open(HEADER).read())
    assert len(eps) >= 60
    for name in ("awt_audio_encode", "awt_op_linear_fused", "awt_linear_decode", "awt_op_dtw", "awt_op_conv1d_framed", "awt_encoder_set_weight",
                 "awt_allreduce_mean_f32"):
        assert name in eps, name
    for name in ("awt_ctx_create", "awt_op_linear_workspace_bytes", "awt_tuning_set", "awt_comm_create", "awt_encoder_set_comm"):
        assert name not in eps, name                                      # no stream parameter
    # a prototype inside a comment is no prototype, and one spread over several lines with a comment inside its parameters is one
    sample = "/* int awt_ghost(void* stream); */\nint awt_real(int a /* [3] */,\n   void* stream);\nint awt_plain(int a);"
    assert set(stream_entry_points(sample)) == {"awt_real"}


def test_every_stream_entry_point_is_in_exactly_one_table():
    eps = set(stream_entry_points(open(HEADER).read()))
    both = set(COVERED) & set(NOT_ON_THE_HOT_PATH)
    neither = eps - set(COVERED) - set(NOT_ON_THE_HOT_PATH)
    unknown = (set(COVERED) | set(NOT_ON_THE_HOT_PATH)) - eps
    assert not both, f"in both tables: {sorted(both)}"
    assert not neither, f"entry points with a stream parameter that no table names: {sorted(neither)}"
    assert not unknown, f"table entries that include/awt.h does not declare with a stream parameter: {sorted(unknown)}"
    assert all(isinstance(r, str) and r.strip() and "\n" not in r for r in NOT_ON_THE_HOT_PATH.values()), "every exemption carries a one-line reason"


def test_no_exempt_entry_point_promises_no_synchronisation():
    eps = stream_entry_points(open(HEADER).read())
    for name in NOT_ON_THE_HOT_PATH:
        assert not re.search(r"no\s+synchroni[sz]ation", eps[name]), f"{name}: its header comment says 'no synchronisation'; it has to be captured, not exempted"


def test_every_covered_entry_point_names_a_case_of_the_gpu_file():
    """The GPU file is read as text (its cases are registered under literal names, or names built from a literal prefix)."""
    src = open(GPU_FILE).read()
    literal = set(re.findall(r'case\(f?"([^"{]+)"', src))
    prefixes = set(re.findall(r'case\(f?"([^"{]*)"\s*\+|case\(f"([^"{]*)\{', src))
    prefixes = {p for pair in prefixes for p in pair if p}
    for name, where in COVERED.items():
        assert where in literal or any(where.startswith(p) for p in prefixes), f"{name}: no case named {where!r} in tests/test_gpu_graph_capture.py"
