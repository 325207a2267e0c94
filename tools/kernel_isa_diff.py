#!/usr/bin/env python3
"""Compare two device-assembly files of one translation unit kernel by kernel:
    python tools/kernel_isa_diff.py parent/ey_generic.dev.s eeyore_amd/lib/obj/ey_generic.dev.s
Per kernel family: how many instantiations have the same instruction stream, and for each one that differs its name with
instruction count, VGPRs, SGPRs and scratch bytes, before -> after.  Comments, labels and directives are ignored."""
import collections
import re
import subprocess
import sys

KEYS = {".amdhsa_next_free_vgpr": "vgpr", ".amdhsa_next_free_sgpr": "sgpr", ".amdhsa_private_segment_fixed_size": "scratch"}


def parse(path):
    """{kernel (or device function) name without its parameter list: (instruction lines, {vgpr, sgpr, scratch}, symbol)}"""
    bodies, meta, sym, cur = {}, {}, None, None
    for line in open(path):
        m = re.match(r"(\w+):", line)
        s = line.strip()
        if m:
            sym = m.group(1)
            bodies[sym] = []
        elif s.startswith(".amdhsa_kernel "):
            cur, sym = s.split()[1], None
            meta[cur] = {}
        elif s.startswith(".end_amdhsa_kernel"):
            cur = None
        elif cur is not None:
            p = s.split()
            if p and p[0] in KEYS:
                meta[cur][KEYS[p[0]]] = int(p[1])
        elif sym is not None and s and s[0] not in ";." and not s.endswith(":"):
            # (a local label carries its function's number in the unit: .LBB<function>_<block>)
            bodies[sym].append(re.sub(r"\.L(\w+?)\d+_(\d+)", r".L\1_\2", re.sub(r"\s*;.*$", "", s)))
    meta.update({k: {} for k in bodies if k not in meta and bodies[k] and k.startswith("_Z")})  # device functions the kernels call out of line
    syms = sorted(meta)
    out = subprocess.run(["c++filt"], input="\n".join(syms), capture_output=True, text=True).stdout.split("\n")
    return {re.sub(r"^\w+ (?=\w+<)", "", d).split("(")[0]: (bodies[k], meta[k], k) for k, d in zip(syms, out)}


def main(before, after):
    a, b = parse(before), parse(after)
    family = lambda k: re.match(r"\w+", k).group(0)
    print(f"{len(a)} kernels and device functions before, {len(b)} after")
    for k in sorted(set(a) ^ set(b)):
        print(f"  only {'before' if k in a else 'after'}: {k}")
    moved = collections.Counter(family(k) for k in set(a) & set(b) if a[k][2] != b[k][2])
    for f in sorted(moved):
        print(f"  {f}: the signature (mangled name) of {moved[f]} instantiations changed")
    same, rows = collections.Counter(), collections.defaultdict(list)
    for k in sorted(set(a) & set(b)):
        if a[k][0] == b[k][0]:
            same[family(k)] += 1
        else:
            rows[family(k)].append(k)
    for f in sorted(set(same) | set(rows)):
        print(f"{f}: {same[f]} of {same[f] + len(rows[f])} instantiations identical")
        for k in rows[f]:
            cols = [f"instructions {len(a[k][0])} -> {len(b[k][0])}"]
            cols += [f"{key} {a[k][1].get(key)} -> {b[k][1].get(key)}" for key in ("vgpr", "sgpr", "scratch")]
            print(f"  {k}\n    " + ", ".join(cols))


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2])
