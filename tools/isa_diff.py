"""Per-kernel comparison of two device assembly files (`hipcc --save-temps`: <unit>-hip-amdgcn-amd-amdhsa-gfx950.s).

    python tools/isa_diff.py before.s after.s [--rename 'REGEX=REPLACEMENT' ...]

Kernels are matched by demangled name with `(anonymous namespace)::` left out; the demangler is llvm-cxxfilt or c++filt from PATH, else
/opt/rocm/llvm/bin/llvm-cxxfilt (ROCm's default place), and without one the mangled names are used, with a warning.
(--rename rewrites the names of the FIRST file, e.g. after a template parameter was dropped:
--rename 'gemm_f8s_kernel<(\\d+), false>=gemm_f8s_kernel<\\1>').  Compared per kernel, as text:
  * the instruction stream between the kernel's label and its end, `;` comments stripped, local labels renumbered in order of first
    appearance and the kernel's own symbol replaced by a placeholder;
  * the metadata rows vgpr_count, agpr_count, sgpr_count, vgpr_spill_count, sgpr_spill_count, private_segment_fixed_size, group_segment_fixed_size.
One line per kernel: `identical`, or `DIFFERS` with both metadata rows and both instruction counts; `WORSE` where the second file has more spilled
registers, scratch bytes, LDS or VGPRs + AGPRs.  Exit status 1 if the kernel sets differ or any kernel is WORSE.

    python tools/isa_diff.py before.s after.s --table 'gemm_pp_kernel|gemm_f8s_kernel'

prints, for every kernel whose demangled name matches the regex, one row per file: VGPRs, AGPRs, scratch bytes, occupancy (the `; Occupancy:` comment
behind the kernel), instruction count, and where its `s_waitcnt vmcnt(0)` and scratch (spill) instructions sit relative to the matrix work:
  k-loop     between the kernel's first and last MFMA
  ahead      between the last MFMA and the full-tile epilogue
  full-tile  inside the full-tile epilogue: the branch-free stretch behind the last MFMA that holds the most global stores (the ragged path predicates
             every row group, so its stores are separated by branches)
  rest       everything behind it (the ragged path, the kernel's end)
Same exit status as the comparison: 1 if a matched kernel of the second file has more scratch, lower occupancy or more k-loop instructions.
"""
from __future__ import annotations

import argparse
import re
import shutil
import subprocess
import sys

META = ["vgpr_count", "agpr_count", "sgpr_count", "vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size", "group_segment_fixed_size"]
LOCAL = re.compile(r"\.L[A-Za-z_$.]*[0-9][A-Za-z0-9_$.]*")


def demangle(names: list[str]) -> list[str]:
    tool = shutil.which("llvm-cxxfilt") or shutil.which("c++filt") or shutil.which("llvm-cxxfilt", path="/opt/rocm/llvm/bin")
    if not names:
        return []
    out = subprocess.run([tool], input="\n".join(names) + "\n", capture_output=True, text=True, check=True).stdout.splitlines() if tool else []
    if len(out) != len(names):
        print("isa_diff: " + ("the demangler's output does not line up with its input" if tool else "no llvm-cxxfilt or c++filt found") +
              ": kernels keep their mangled names, which a --rename pattern written for demangled names will not match", file=sys.stderr)
        return list(names)
    return [n.replace("(anonymous namespace)::", "") for n in out]


def parse(path: str) -> dict[str, dict]:
    """mangled kernel name -> {"meta": {row: int}, "code": [normalised instruction lines]}"""
    lines = open(path).read().splitlines()
    # ---- metadata: the entries of amdhsa.kernels
    meta: dict[str, dict] = {}
    try:
        i = lines.index("amdhsa.kernels:") + 1
    except ValueError:
        i = len(lines)
    cur: dict = {}
    while i < len(lines) and (lines[i].startswith("  ") or not lines[i].strip()):
        ln = lines[i]
        if ln.startswith("  - "):
            cur = {}
            ln = "    " + ln[4:]
        m = re.match(r"^    \.(\w+):\s+(\S+)\s*$", ln)
        if m:
            if m.group(1) == "name":
                meta[m.group(2)] = cur
            elif m.group(1) in META:
                cur[m.group(1)] = int(m.group(2))
        i += 1
    # ---- instruction streams
    kernels: dict[str, dict] = {}
    i = 0
    while i < len(lines):
        m = re.match(r"^([A-Za-z_][\w$.]*):", lines[i])
        if not m or m.group(1) not in meta:
            i += 1
            continue
        name = m.group(1)
        labels: dict[str, str] = {}
        code = []
        i += 1
        while i < len(lines) and not re.match(r"^\.Lfunc_end\d+:|^\t\.section\b", lines[i]):
            ln = lines[i].split(";", 1)[0].rstrip()
            i += 1
            if not ln.strip():
                continue
            ln = ln.replace(name, "<kernel>")
            ln = LOCAL.sub(lambda t: labels.setdefault(t.group(0), f".L{len(labels)}"), ln)
            code.append(re.sub(r"\s+", " ", ln.strip()))
        occ = -1
        for j in range(i, min(i + 400, len(lines))):                            # the resource comments behind the kernel
            mo = re.match(r"^; Occupancy: (\d+)", lines[j])
            if mo:
                occ = int(mo.group(1))
                break
        kernels[name] = {"meta": meta[name], "code": code, "occupancy": occ}
    return kernels


def table_row(k: dict) -> dict:
    """Resource and wait columns of one kernel for --table (see the module docstring)."""
    code = [ln for ln in k["code"] if not ln.startswith(".") or ln.endswith(":")]
    is_inst = lambda ln: not ln.endswith(":")
    mf = [i for i, ln in enumerate(code) if ln.startswith("v_mfma") or ln.startswith("v_smfma")]
    first, last = (mf[0], mf[-1]) if mf else (0, 0)
    # branch-free stretches behind the last MFMA
    blocks, start = [], last + 1
    for i in range(last + 1, len(code) + 1):
        if i == len(code) or code[i].endswith(":") or code[i].startswith(("s_cbranch", "s_branch", "s_endpgm")):
            blocks.append((start, i))
            start = i + 1
    stores = lambda b: sum(1 for ln in code[b[0]:b[1]] if ln.startswith(("global_store", "buffer_store", "flat_store")))
    full = max(blocks, key=stores) if blocks else (len(code), len(code))
    spans = {"k-loop": (first, last), "ahead": (last + 1, full[0]), "full-tile": full, "rest": (full[1], len(code))}
    drain = lambda ln: ln.startswith("s_waitcnt") and "vmcnt(0)" in ln
    spill = lambda ln: ln.startswith("scratch_")
    out = {"vgpr": k["meta"].get("vgpr_count", -1), "agpr": k["meta"].get("agpr_count", -1), "scratch": k["meta"].get("private_segment_fixed_size", -1),
           "occupancy": k.get("occupancy", -1), "instructions": sum(1 for ln in code if is_inst(ln)), "k-loop instructions": sum(1 for ln in code[first:last + 1] if is_inst(ln)),
           "full-tile stores": stores(full)}
    for name, (a, b) in spans.items():
        out[f"vmcnt(0) {name}"] = sum(1 for ln in code[a:b] if drain(ln))
        out[f"spill ops {name}"] = sum(1 for ln in code[a:b] if spill(ln))
    return out


def table(paths: list[str], sides: list[dict], pattern: str) -> int:
    rx, bad = re.compile(pattern), 0
    cols = ["vgpr", "agpr", "scratch", "occupancy", "instructions", "k-loop instructions", "full-tile stores"] + [f"{w} {s}" for s in ("k-loop", "ahead", "full-tile", "rest") for w in ("vmcnt(0)", "spill ops")]
    print("# columns: " + " | ".join(cols))
    for name in sorted(n for n in set(sides[0]) | set(sides[1]) if rx.search(n)):
        rows = [table_row(sd[name]) if name in sd else None for sd in sides]
        print(name)
        for path, r in zip(paths, rows):
            print(f"  {path}: " + ("(absent)" if r is None else " | ".join(str(r[c]) for c in cols)))
        if rows[0] and rows[1] and (rows[1]["scratch"] > rows[0]["scratch"] or rows[1]["occupancy"] < rows[0]["occupancy"] or rows[1]["k-loop instructions"] > rows[0]["k-loop instructions"]):
            print("  WORSE")
            bad += 1
    return 1 if bad else 0


def row(k: dict) -> str:
    n = sum(1 for ln in k["code"] if not ln.endswith(":") and not ln.startswith("."))     # labels and directives are compared, not counted
    return " ".join(f"{m}={k['meta'].get(m, '?')}" for m in META) + f" instructions={n}"


def worse(a: dict, b: dict) -> bool:
    g = lambda m, k: m.get(k, 0)
    return (g(b, "vgpr_spill_count") > g(a, "vgpr_spill_count") or g(b, "sgpr_spill_count") > g(a, "sgpr_spill_count") or
            g(b, "private_segment_fixed_size") > g(a, "private_segment_fixed_size") or g(b, "group_segment_fixed_size") > g(a, "group_segment_fixed_size") or
            g(b, "vgpr_count") + g(b, "agpr_count") > g(a, "vgpr_count") + g(a, "agpr_count"))


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("before")
    ap.add_argument("after")
    ap.add_argument("--rename", action="append", default=[], metavar="REGEX=REPLACEMENT", help="rewrite demangled kernel names of the first file")
    ap.add_argument("--table", metavar="REGEX", default=None, help="resource / wait table of the kernels whose demangled name matches, instead of the comparison")
    args = ap.parse_args()
    sides = []
    for path, renames in ((args.before, args.rename), (args.after, [])):
        k = parse(path)
        names = demangle(list(k))
        for r in renames:
            pat, _, repl = r.partition("=")
            names = [re.sub(pat, repl, n) for n in names]
        sides.append(dict(zip(names, k.values())))
    if args.table:
        return table([args.before, args.after], sides, args.table)
    a, b = sides
    n_same = n_diff = n_worse = 0
    for name in sorted(set(a) & set(b)):
        ka, kb = a[name], b[name]
        if ka["code"] == kb["code"] and ka["meta"] == kb["meta"]:
            n_same += 1
            print(f"identical  {name}")
            continue
        w = worse(ka["meta"], kb["meta"])
        n_diff += 1
        n_worse += w
        print(f"{'WORSE' if w else 'DIFFERS'}  {name}  | before: {row(ka)} | after: {row(kb)}")
    only_a, only_b = sorted(set(a) - set(b)), sorted(set(b) - set(a))
    for name in only_a:
        print(f"ONLY IN FIRST  {name}")
    for name in only_b:
        print(f"ONLY IN SECOND  {name}")
    print(f"# {args.before} -> {args.after}: {len(a)} / {len(b)} kernels, {n_same} identical, {n_diff} differ ({n_worse} worse), {len(only_a)} only in the first, {len(only_b)} only in the second")
    return 1 if (only_a or only_b or n_worse) else 0


if __name__ == "__main__":
    sys.exit(main())
