"""What adding and removing instances on the device costs (rt_set_instances) on bench.py's headline workload (config 4, 1080p).

One context follows a table that grows and shrinks through rt_set_instances; a second context takes the only route there was before the call for the same new scene,
rt_upload_scene + rt_build_accel.  The added instances are copies of non-emissive instances of the smaller meshes, displaced, appended behind the scene's own
(the emitter rule); removing them truncates the table again.
  (c) the first call (allocations, the templates of every alpha-tested mesh), wall time, reported on its own;
  (a) steady state, adding 1 / 15 / 150 instances and removing as many, five calls each: HIP-event ms of the call and of its expansion kernels, host wall time,
      bytes moved host -> device — against the host wall time of rt_upload_scene + rt_build_accel of the same new scene;
  (b) ms per frame with frames in flight on the resulting device-built tree against the host-built tree of the same scene.

  python scripts/instances_timing.py [--footprint real|lite] [--steps 24] [--warmup 8] [--out profiles/instances_timing.txt] [--bench-ab FILE]
One JSON line per measurement on stdout; the tables made of them are written to --out.  --bench-ab FILE: lines "parent {bench.py's JSON line}" / "this {...}" of
bench.py --gpus 1 --steps 100 --warmup 20 run on the parent commit's library and on this one, alternated in the same visit (RESTIR_HIP_LIB selects the library)."""
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

COUNTS = (1, 15, 150)
CALLS = 5


def emissive_instances(desc, inst):
    """the scene's light rule (host/scene.cpp createTrigLightBuffer) per instance"""
    pm = np.frombuffer((C.c_char * (desc.numPrimMeshes * 20)).from_address(desc.primMeshes), dtype=np.int32).reshape(-1, 5)
    mats = np.frombuffer((C.c_char * (desc.numMaterials * 80)).from_address(desc.materials), dtype=np.float32).reshape(-1, 20)
    lum = 0.2126 * mats[:, 9] + 0.7152 * mats[:, 10] + 0.0722 * mats[:, 11]
    return lum[np.maximum(pm[inst["primMesh"], 4], 0)] > 1e-2


def write_profile(path, a, rows, bench):
    first = [r for r in rows if r["what"] == "first call"][0]
    out = ["rt_set_instances on bench.py's headline workload (config 4, %s footprint, %dx%d), one run of scripts/instances_timing.py --steps %d --warmup %d." % (a.footprint, W, H, a.steps, a.warmup),
           "scene: " + json.dumps([r for r in rows if r["what"] == "scene"][0]), "",
           "(c) the first call (allocates the working buffers, two trees, two tables; makes and uploads the templates of every alpha-tested mesh in the table):",
           "  " + json.dumps(first), "",
           "(a) steady state, %d calls each (mean; min .. max of the wall time): rt_set_instances against rt_upload_scene + rt_build_accel of the same new scene" % CALLS,
           "  change        instances   triangles   event ms   expand ms   wall ms (min .. max)        bytes up    upload + host build wall ms   host / device wall"]
    for r in [r for r in rows if r["what"] == "steady"]:
        out.append("  %-12s  %7d   %9d   %8.3f   %8.4f   %8.3f (%7.3f .. %7.3f)   %9d   %12.1f                  %7.1f x" % (
            r["change"], r["instances"], r["triangles"], r["event_ms"], r["expand_ms"], r["wall_ms"], r["wall_ms_min"], r["wall_ms_max"], r["bytes_uploaded"],
            r["host_route_wall_ms"], r["host_over_device_wall"]))
    out += ["", "(b) ms per frame (frames in flight, host-timed) on the tree rt_set_instances left against the host-built tree of the same scene:"]
    out += ["  " + json.dumps(r) for r in rows if r["what"] == "frame"]
    if bench:
        out += ["", "Default path: bench.py --gpus 1 --steps 100 --warmup 20, the parent commit's library and this one alternated in one visit."]
        ms = {"parent": [], "this": []}
        for line in bench:
            who, js = line.split(None, 1)
            d = json.loads(js)
            ms[who].append(d["ms_per_step"])
            out.append("  %-6s  ms_per_step %.4f   %.2f %s" % (who, d["ms_per_step"], d["value"], d["unit"]))
        if len(ms["parent"]) > 1 and ms["this"]:
            mp, mt = sum(ms["parent"]) / len(ms["parent"]), sum(ms["this"]) / len(ms["this"])
            out.append("  mean parent %.4f ms, this %.4f ms: %+.2f %%; the parent's own runs differ by %.2f %% in this visit.  The default path never calls the new code." % (
                mp, mt, (mt / mp - 1) * 100, (max(ms["parent"]) / min(ms["parent"]) - 1) * 100))
    with open(path, "w") as f:
        f.write("\n".join(out) + "\n")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--footprint", default="real", choices=["real", "lite"])
    ap.add_argument("--steps", type=int, default=24)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "instances_timing.txt"))
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
    base = instances(desc)
    pm = np.frombuffer((C.c_char * (desc.numPrimMeshes * 20)).from_address(desc.primMeshes), dtype=np.uint32).reshape(-1, 5)
    tris = pm[base["primMesh"], 3] // 3
    pool = np.nonzero((tris < np.percentile(tris, 90)) & ~emissive_instances(desc, base))[0]
    rng = np.random.default_rng(5)

    def table(k):
        pick = pool[rng.permutation(len(pool))[:k]]
        extra = base[pick].copy()
        offs = rng.normal(0, 1, (k, 3)).astype(np.float32) * np.float32([2.0, 0.2, 2.0])
        extra["objectToWorld"] = moved(extra["objectToWorld"], offs)
        return np.concatenate([base, extra])
    dev, hst = Renderer().setup(0), Renderer().setup(0)
    for r in (dev, hst):
        r.load_scene(desc)
        r.update(W, H)
    emit({"what": "scene", "footprint": a.footprint, "instances": len(base), "alpha_tested_instances": int(((base["flags"] & 1) == 0).sum()), **hst.accel_stats()})

    def timed_set(t):
        dev.sync()
        t0 = time.perf_counter()
        dev.set_instances(t)
        wall = (time.perf_counter() - t0) * 1e3
        s = dev.instances_stats()
        return wall, s

    def host_route(t):
        sc.setInstances(t)
        d2 = sc.desc(env)
        hst.sync()
        t0 = time.perf_counter()
        hst.load_scene(d2)
        return (time.perf_counter() - t0) * 1e3, d2
    wall, s = timed_set(table(1))
    emit({"what": "first call", "wall_ms": round(wall, 3), "event_ms": round(s.ms, 4), "expand_ms": round(s.expandMs, 4), "bytes_uploaded": s.bytesUploaded,
          "reallocated": s.reallocated, "instances": s.instances, "triangles": s.triangles})
    timed_set(base)
    frames = {"dev": 0, "hst": 0}
    for k in COUNTS:
        add, rem = [], []
        for _ in range(CALLS):
            t = table(k)
            add.append(timed_set(t))
            rem.append(timed_set(base))
        for change, runs, tab in (("add %d" % k, add, t), ("remove %d" % k, rem, base)):
            hw, d2 = host_route(tab)
            w = [x[0] for x in runs]
            s = runs[-1][1]
            emit({"what": "steady", "change": change, "instances": s.instances, "triangles": s.triangles, "event_ms": round(float(np.mean([x[1].ms for x in runs])), 4),
                  "expand_ms": round(float(np.mean([x[1].expandMs for x in runs])), 4), "wall_ms": round(float(np.mean(w)), 4), "wall_ms_min": round(min(w), 4),
                  "wall_ms_max": round(max(w), 4), "bytes_uploaded": s.bytesUploaded, "reallocated_any": int(any(x[1].reallocated for x in runs)),
                  "host_route_wall_ms": round(hw, 1), "host_over_device_wall": round(hw / float(np.mean(w)), 2)})
        if k == COUNTS[-1]:     # (b): both contexts on the scene with the last 150 added
            timed_set(t)
            hw, d2 = host_route(t)
            dev.update_lights(d2)
            ms_dev, frames["dev"] = frame_ms(dev, sc, st, a, frames["dev"])
            ms_hst, frames["hst"] = frame_ms(hst, sc, st, a, frames["hst"])
            emit({"what": "frame", "instances": len(t), "ms_per_frame_after_set_instances": round(ms_dev, 4), "ms_per_frame_host_built": round(ms_hst, 4),
                  "device_over_host": round(ms_dev / ms_hst, 4)})
    dev.destroy(); hst.destroy()
    bench = [l.strip() for l in open(a.bench_ab)] if a.bench_ab else []
    write_profile(a.out, a, rows, [l for l in bench if l])


if __name__ == "__main__":
    main()
