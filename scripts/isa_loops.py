#!/usr/bin/env python3
"""Scratch accesses inside the loops of the two traced kernels (the companion of scripts/isa_census.py: "no scratch access inside a traversal loop").

  python scripts/isa_loops.py [stages.hip] [extra hipcc flags: stages.hip -DRT_SKY=1 is the build sky, ...]

Compiles the unit as isa_census.py does and lists, for k_direct_stage and k_indirect_stage, every loop (a backward branch to a .LBB label) of more than 100
instructions: its length, its 16-byte loads (a traversal loop fetches nodes and triangle records: 5 or more), its DPP moves (the eight-lanes-per-ray tail) and the
scratch loads / stores between its header and its back edge.  The traversal loops must show 0; the bounce loop of the indirect stage, which contains the ray pools
AND the shading of a path vertex, is the one long loop (> 10 000 instructions) that may not.  Re-run after a compiler update: it is also how to see whether
tracePool still needs splitLdsPointer (traverse.h) — take the call out and look for scratch_load in the loops with 26 and 18 16-byte loads.  Runs without a GPU."""
import os, re, sys, tempfile
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import isa_census


def loops(path):
    lines = open(path).read().split("\n")
    heads = [(i, m.group(1)) for i, l in enumerate(lines) for m in [re.match(r"^(_Z\w+):", l)] if m and "k_" in m.group(1)]
    heads.append((len(lines), None))
    for (a, k), (b, _) in zip(heads, heads[1:]):
        if "k_direct_stage" not in k and "k_indirect_stage" not in k:
            continue
        labels = {m.group(1): i for i in range(a, b) for m in [re.match(r"^(\.LBB\d+_\d+):", lines[i])] if m}
        found = []
        for i in range(a, b):
            m = re.match(r"\s+s_c?branch\w*\s+(\.LBB\d+_\d+)", lines[i])
            if m and labels.get(m.group(1), i) < i:
                found.append((labels[m.group(1)], i))
        print(k)
        for s, e in sorted(found):
            body = lines[s:e]
            n = sum(1 for l in body if re.match(r"\s+[vs]_", l))
            if n <= 100:
                continue
            scr = [l.split(";")[0].strip() for l in body if re.match(r"\s+scratch_(load|store)", l)]
            print("  loop at +%-6d %5d instructions  %2d 16-byte loads  %2d dpp  scratch accesses %d %s" % (
                s - a, n, sum(1 for l in body if "global_load_dwordx4" in l), sum(1 for l in body if "dpp" in l), len(scr), scr[:3] if scr else ""))


if __name__ == "__main__":
    src = sys.argv[1] if len(sys.argv) > 1 else "stages.hip"
    out = os.path.join(tempfile.mkdtemp(prefix="isa_"), "unit.s")
    isa_census.census(src, sys.argv[2:], keep=out)
    loops(out)
