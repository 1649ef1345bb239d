#!/usr/bin/env python3
"""Compare two directories of `make asm` listings kernel by kernel ("Which edits leave the machine code alone").

usage: isa_same.py PARENT_DIR THIS_DIR
Per kernel of every *.s file: the instruction count on each side, whether the instruction streams are identical (comments,
directives and labels dropped), whether the opcode sequences are, and the resource figures of scripts/resources.sh (registers,
spills, scratch, LDS, occupancy) where they differ.  Class A: same stream.  B: same opcodes, same resources.  C: anything else.
Exits 1 if a listing or a kernel exists on one side only."""
import os, re, sys

RES = ("vgpr_count", "agpr_count", "sgpr_count", "sgpr_spill_count", "vgpr_spill_count",
       "private_segment_fixed_size", "group_segment_fixed_size")

def kernels(path):
    """{kernel: (instructions, resources)} of one listing"""
    code, res, cur, last, meta = {}, {}, None, None, {}
    for raw in open(path):
        line = raw.split(";")[0].strip()
        m = re.match(r"; Occupancy: (\d+)", raw)
        if m and last is not None: res.setdefault(last, {})["occupancy"] = m.group(1)
        m = re.match(r"\s+(?:- )?\.(\w+):\s+(\S+)$", raw)              # the metadata note: one block per kernel, keys sorted
        if m:
            if m.group(1) == "agpr_count": meta = {}
            meta[m.group(1)] = m.group(2)
            if m.group(1) == "vgpr_spill_count" and meta.get("name") in res:
                res[meta["name"]].update({k: meta.get(k) for k in RES})
            continue
        m = re.match(r"\.type\s+(\w+),@function", line)
        if m: cur = last = m.group(1); code[cur] = []; continue
        if line.startswith(".Lfunc_end"): cur = None
        if cur is None or not line or line.startswith(".") or line.endswith(":"): continue
        code[cur].append(" ".join(line.split()))
    bare = [k for k in code if len(res.get(k, {})) <= 1]                # no figures: the metadata note is not laid out as expected
    if bare: sys.exit("%s: no resource figures for %s" % (path, ", ".join(bare)))
    return {k: (code[k], res[k]) for k in code}

def main(a_dir, b_dir):
    files = lambda d: {f for f in os.listdir(d) if f.endswith(".s")}
    missing = sorted(files(a_dir) ^ files(b_dir))
    print("%-44s %7s %7s %6s %7s  %s" % ("kernel", "parent", "this", "stream", "opcodes", "class  occ vgpr agpr sgpr sgprSpill vgprSpill scratch lds"))
    for f in sorted(files(a_dir) & files(b_dir)):
        a, b = kernels(os.path.join(a_dir, f)), kernels(os.path.join(b_dir, f))
        missing += sorted("%s:%s" % (f, k) for k in set(a) ^ set(b))
        for k in a:
            if k not in b: continue
            (ca, ra), (cb, rb) = a[k], b[k]
            same, ops = ca == cb, [i.split()[0] for i in ca] == [i.split()[0] for i in cb]
            cls = "A" if same else "B" if ops and ra == rb else "C"
            show = " ".join(ra[r] if ra[r] == rb.get(r) else "%s->%s" % (ra[r], rb.get(r)) for r in ("occupancy",) + RES)
            print("%-44s %7d %7d %6s %7s  %s  %s" % (k, len(ca), len(cb), "same" if same else "DIFF", "same" if ops else "DIFF", cls, show))
    for m in missing: print("only on one side:", m)
    return 1 if missing else 0

if __name__ == "__main__":
    if len(sys.argv) != 3: sys.exit(__doc__)
    sys.exit(main(sys.argv[1], sys.argv[2]))
