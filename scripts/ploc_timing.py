"""What the PLOC builder of the device rebuild costs and buys (rt_set_rebuild_options) on bench.py's headline workload (config 4, 1080p).

Every instance but the largest meshes is displaced by a growing offset (scripts/refit_timing.py's degrade sequence, as scripts/accel_build_timing.py uses it).  One
context follows the scene through rt_update_instances and rebuilds the SAME moved scene with each builder in turn — LBVH, PLOC at radius 8 / 16, LBVH, PLOC at radius
32 / 64, LBVH: the three LBVH measurements of a displacement give the run's own spread —, one uploads and host-builds it.  Per displacement and builder:
  (a) the rebuild (HIP events, host wall time including the drain, PLOC's merge iterations) against rt_upload_scene + rt_build_accel (host wall time);
  (b) ms per frame with frames in flight on that tree, and on the host-built tree;
  (c) node / triangle steps of one frame (rt_set_counting).

  python scripts/ploc_timing.py [--footprint real|lite] [--steps 24] [--warmup 8] [--sigmas 0.1,1.0,4.0] [--out profiles/ploc_timing.txt] [--bench-ab FILE]
One JSON line per measurement on stdout; the tables made of them are written to --out.  --bench-ab FILE: lines "parent {bench.py's JSON line}" / "this {...}" of
bench.py --gpus 1 run on the parent commit's library and on this one, alternated in the same visit (RESTIR_HIP_LIB selects the library)."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import restir_amd  # noqa: E402,F401
from restir_amd import abi, host  # noqa: E402
from restir_amd.renderer import Renderer  # noqa: E402
from refit_timing import W, H, instances, moved, frame_ms  # noqa: E402
from accel_build_timing import steps_per_frame  # noqa: E402

ORDER = (("lbvh", 0), ("ploc", 8), ("ploc", 16), ("lbvh", 0), ("ploc", 32), ("ploc", 64), ("lbvh", 0))


def write_profile(path, a, rows, bench):
    out = ["The PLOC builder of rt_rebuild_accel on bench.py's headline workload (config 4, %s footprint, %dx%d), one run of scripts/ploc_timing.py --steps %d --warmup %d." % (
               a.footprint, W, H, a.steps, a.warmup),
           "One context rebuilds the same moved scene (scripts/refit_timing.py's degrade sequence) with each builder in turn, one uploads and host-builds it.", "",
           "scene (host build): " + json.dumps(rows[0]), "first builds:       " + json.dumps(rows[1]), "",
           "(a) rebuild, (b) ms per frame (frames in flight, host-timed), (c) node / triangle steps of one frame; `host` = rt_upload_scene + rt_build_accel",
           "  sigma   builder   event ms   wall ms   iterations   nodes/levels   ms/frame   / host    node steps   tri steps"]
    for r in rows:
        if r["what"] == "tree":
            out.append("  %-5s   %-7s  %8.3f  %8.1f   %6d      %8d / %2d   %7.3f   %6.3f x  %10d  %10d" % (
                r["sigma"], r["builder"], r["event_ms"], r["wall_ms"], r["iterations"], r["nodes"], r["levels"], r["ms_per_frame"], r["over_host"], r["node_steps"], r["tri_steps"]))
    out.append("")
    trees = [r for r in rows if r["what"] == "tree"]
    for s in sorted({r["sigma"] for r in trees}):
        lb = [r["ms_per_frame"] for r in trees if r["sigma"] == s and r["builder"] == "lbvh"]
        mean = sum(lb) / len(lb)
        line = "  sigma %-4s  LBVH ms/frame %s: mean %.3f, spread %.3f (%.2f %%);" % (s, " ".join("%.3f" % v for v in lb), mean, max(lb) - min(lb), (max(lb) - min(lb)) / mean * 100)
        for r in trees:
            if r["sigma"] == s and r["builder"].startswith("ploc"):
                line += "  %s %+.2f %%" % (r["builder"], (r["ms_per_frame"] / mean - 1) * 100)
        out.append(line)
    ploc_wall = [r["wall_ms"] for r in trees if r["builder"].startswith("ploc")]
    host_wall = [r["wall_ms"] for r in trees if r["builder"] == "host"]
    if ploc_wall and host_wall:
        out += ["", "The one condition on time, PLOC rebuild faster than upload + host build measured in the same run: slowest PLOC rebuild %.1f ms wall, fastest host rebuild %.1f ms (%s)." % (
            max(ploc_wall), min(host_wall), "met" if max(ploc_wall) < min(host_wall) else "NOT met")]
    if bench:
        out += ["", "Default path: bench.py --gpus 1, the parent commit's library and this one alternated in one visit (the default builder never calls the new code)."]
        ms = {"parent": [], "this": []}
        for line in bench:
            who, js = line.split(None, 1)
            d = json.loads(js)
            ms[who].append(d["ms_per_step"])
            out.append("  %-6s  ms_per_step %.4f   %.2f %s" % (who, d["ms_per_step"], d["value"], d["unit"]))
        if ms["parent"] and ms["this"]:
            mp, mt = sum(ms["parent"]) / len(ms["parent"]), sum(ms["this"]) / len(ms["this"])
            out.append("  mean parent %.4f ms (spread %.4f), this %.4f ms (spread %.4f): %+.2f %%" % (
                mp, max(ms["parent"]) - min(ms["parent"]), mt, max(ms["this"]) - min(ms["this"]), (mt / mp - 1) * 100))
    with open(path, "w") as f:
        f.write("\n".join(out) + "\n")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--footprint", default="real", choices=["real", "lite"])
    ap.add_argument("--steps", type=int, default=24)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--sigmas", default="0.1,1.0,4.0")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ploc_timing.txt"))
    ap.add_argument("--bench-ab", default=None)
    a = ap.parse_args()
    rows = []

    def emit(row):
        rows.append(row)
        print(json.dumps(row), flush=True)
    kind = abi.PROC_BISTRO_EXT_REAL if a.footprint == "real" else abi.PROC_BISTRO_EXT
    sc = host.Scene().makeProcedural(kind, 1.0, 1)
    env = host.HdrSampling()
    env.makeSyntheticSky(2048, 1024, 5e4, 7)
    st = host.default_state(W, H, sc, env)
    desc = sc.desc(env)
    home = instances(desc)["objectToWorld"]
    rng = np.random.default_rng(5)
    dev, hst = Renderer().setup(0), Renderer().setup(0)
    for r in (dev, hst):
        r.load_scene(desc)
        r.update(W, H)
    emit({"what": "scene", "footprint": a.footprint, "instances": len(home), **hst.accel_stats()})
    first = {}
    for builder in (abi.REBUILD_LBVH, abi.REBUILD_PLOC):      # the first build of each kind allocates: kept out of the timings below
        dev.set_rebuild_options(builder)
        t0 = time.perf_counter()
        dev.rebuild_accel()
        first["ploc" if builder else "lbvh"] = round((time.perf_counter() - t0) * 1e3, 3)
    emit({"what": "first builds (allocate: the working buffers and two trees, then PLOC's cluster buffers)", "wall_ms": first, "default_radius": dev.rebuild_options().radius})
    pm = np.frombuffer((C.c_char * (desc.numPrimMeshes * 20)).from_address(desc.primMeshes), dtype=np.uint32).reshape(-1, 5)
    tris = pm[instances(desc)["primMesh"], 3] // 3
    movable = np.nonzero(tris < np.percentile(tris, 90))[0].astype(np.uint32)
    direction = rng.normal(0, 1, (len(movable), 3)).astype(np.float32)
    direction[:, 1] *= 0.2
    fd = fh = 0
    for disp in [float(s) for s in a.sigmas.split(",")]:
        xf = moved(home[movable], direction * np.float32(disp))
        dev.update_instances(movable, xf)
        sc.updateInstances(movable, xf)
        d2 = sc.desc(env)
        dev.update_lights(d2)
        t0 = time.perf_counter()
        hst.load_scene(d2)
        host_wall = (time.perf_counter() - t0) * 1e3
        host_ms, fh = frame_ms(hst, sc, st, a, fh)
        hn, ht = steps_per_frame(hst, sc, st, fh)
        fh += 1
        hs = hst.accel_stats()
        emit({"what": "tree", "sigma": disp, "builder": "host", "event_ms": 0.0, "wall_ms": round(host_wall, 1), "iterations": 0, "nodes": hs["nodes"], "levels": hs["max_depth"],
              "ms_per_frame": round(host_ms, 4), "over_host": 1.0, "node_steps": hn, "tri_steps": ht})
        for builder, radius in ORDER:
            dev.set_rebuild_options(abi.REBUILD_PLOC if builder == "ploc" else abi.REBUILD_LBVH, radius)
            dev.sync()
            t0 = time.perf_counter()
            dev.rebuild_accel()
            wall = (time.perf_counter() - t0) * 1e3
            s = dev.rebuild_stats()
            ms, fd = frame_ms(dev, sc, st, a, fd)
            n, t = steps_per_frame(dev, sc, st, fd)
            fd += 1
            emit({"what": "tree", "sigma": disp, "builder": builder + (str(radius) if radius else ""), "event_ms": round(s.ms, 4), "wall_ms": round(wall, 3), "iterations": s.iterations,
                  "nodes": s.nodes, "levels": s.levels, "ms_per_frame": round(ms, 4), "over_host": round(ms / host_ms, 4), "node_steps": n, "tri_steps": t})
    dev.destroy(); hst.destroy()
    bench = [l.strip() for l in open(a.bench_ab)] if a.bench_ab else []
    write_profile(a.out, a, rows, [l for l in bench if l])


if __name__ == "__main__":
    main()
