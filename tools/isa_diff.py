#!/usr/bin/env python3
"""Compares two tools/isa_dump.sh output directories kernel by kernel: for every kernel of every .s
file the resources of its metadata (LDS, scratch, SGPRs, VGPRs, spills), the instruction count, the
opcode histogram difference and the index of the first differing opcode.  Exits 1 when a resource
field differs anywhere (register renumbering and a few moved scalar instructions do not).
usage: tools/isa_diff.py DIR_A DIR_B"""
import collections
import os
import re
import sys

FIELDS = ["group_segment_fixed_size", "private_segment_fixed_size", "sgpr_count", "sgpr_spill_count", "vgpr_count",
          "vgpr_spill_count"]


def kernels(path):
    """{kernel name: (resources, opcodes)} of one .s file"""
    lines = open(path).read().split("\n")
    res, cur = {}, None
    for ln in lines:  # the amdhsa.kernels metadata: one record per kernel, fields in alphabetical order
        m = re.match(r"    \.(\w+):\s+(\S+)", ln)  # a kernel's own fields (its arguments' sit deeper)
        if m and m.group(1) == FIELDS[0]:
            cur = {}
        if m and cur is not None and m.group(1) in FIELDS + ["name"]:
            cur[m.group(1)] = m.group(2)
            if m.group(1) == "name":
                res[m.group(2)] = cur
    out = {}
    for name, r in res.items():
        ops, i = [], next(j for j, ln in enumerate(lines) if ln.startswith(name + ":")) + 1
        while not lines[i].startswith(".Lfunc_end"):
            tok = lines[i].split(";")[0].split()
            if tok and lines[i][0] in " \t" and not tok[0].startswith(".") and not tok[0].endswith(":"):
                ops.append(tok[0])
            i += 1
        out[name] = ([r.get(f, "?") for f in FIELDS], ops)
    return out


a_dir, b_dir = sys.argv[1:3]
bad = 0
for f in sorted(os.listdir(a_dir)):
    if not f.endswith(".s"):
        continue
    A, B = kernels(os.path.join(a_dir, f)), kernels(os.path.join(b_dir, f))
    same_file = open(os.path.join(a_dir, f)).read() == open(os.path.join(b_dir, f)).read()
    print(f"== {f}: {len(A)} kernels, {'byte-identical' if same_file else 'differs'}")
    for name in sorted(set(A) | set(B)):
        if name not in A or name not in B:
            print(f"  {name[:100]}: only in {'A' if name in A else 'B'}")
            bad += 1
            continue
        (ra, oa), (rb, ob) = A[name], B[name]
        if ra != rb:
            bad += 1
        if same_file or (ra == rb and oa == ob):
            continue
        hist = collections.Counter(ob)
        hist.subtract(oa)
        first = next((i for i, (x, y) in enumerate(zip(oa, ob)) if x != y), min(len(oa), len(ob)))
        print(f"  {name[:100]}\n    lds/scratch/sgpr/sgpr-spill/vgpr/vgpr-spill A {' '.join(ra)} | B {' '.join(rb)}"
              f"{'' if ra == rb else '  <-- RESOURCES DIFFER'}\n    instructions A {len(oa)} B {len(ob)}, first differing opcode at"
              f" {first}, histogram B-A: {' '.join(f'{k}{v:+d}' for k, v in sorted(hist.items()) if v) or 'none'}")
print("resources differ" if bad else "resources equal")
sys.exit(1 if bad else 0)
