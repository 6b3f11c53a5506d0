#!/usr/bin/env python3
"""Records the bits of the f16f8 attention forward on the seeded inputs of tests/test_gpu_attention_schedule.py (GPU box only).

    python tools/make_golden_attention.py [--lib path/to/libawt.so] [--out tests/golden/attention_f16f8_sha256.json]

Writes the SHA-256 of each output's bytes.  Run it with the library of the commit whose arithmetic is to be kept (AWT_LIB or --lib names
a library built elsewhere, e.g. from a worktree of the parent commit); a later build that schedules the same arithmetic differently has
to reproduce every hash, so the file is recorded once and not from the build under test.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default=None, help="libawt.so to record (default: the tree's own build)")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "attention_f16f8_sha256.json"))
    a = ap.parse_args()
    if a.lib:
        os.environ["AWT_LIB"] = os.path.abspath(a.lib)
    import torch

    from mlx8_ws_audio_transformer_amd import _lib
    from tests import test_gpu_attention_schedule as t

    torch.cuda.set_device(0)
    hashes = {}
    for name in t.CASES:
        q, k, v = t.inputs(name)
        o = t.run(name, q, k, v)
        torch.cuda.synchronize()
        p = torch.softmax(q.double() @ k.double().transpose(2, 3), dim=-1)
        err = (o.double() - (p @ v.double()).transpose(1, 2).reshape(o.shape)).abs().max().item()
        hashes[name] = t.sha256(o)
        print("%-20s B, H, S = %s max-abs vs fp64 %.3e  %s" % (name, t.CASES[name][:3], err, hashes[name]), flush=True)
    with open(a.out, "w") as f:
        json.dump({"library": os.path.basename(_lib.LIB_PATH), "inputs": "tests/test_gpu_attention_schedule.py: inputs(name)", "sha256": hashes}, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
