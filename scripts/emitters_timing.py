"""What adding and removing emitters on the device costs (rt_set_emitter_meshes + rt_set_instances) on bench.py's headline workload (config 4, 1080p).

One context has the emitter mode on and follows a table to which copies of the scene's emissive instances are appended, displaced, and from which they are removed
again; a second context takes the only route there was before the mode for the same new scene, rt_upload_scene + rt_build_accel.
  (a) steady state, adding 1 / 15 emissive instances and removing as many, five calls each: host wall time, HIP-event ms of the call, of k_light_expand alone, bytes
      moved host -> device (the call's own and the lights') — against the host wall time of rt_upload_scene + rt_build_accel of the same new scene;
  (b) --plain LABEL: one JSON line with the wall and event time of rt_set_instances on a NON-emissive change (15 instances added, removed), mode on when LABEL ends in
      "on", for the library RESTIR_HIP_LIB selects: run once per library / mode, alternated, and handed to the main run as --plain-ab FILE.

  python scripts/emitters_timing.py [--footprint real|lite] [--out profiles/emitters_timing.txt] [--plain-ab FILE] [--bench-ab FILE]
  python scripts/emitters_timing.py --plain parent|off|on [--footprint real|lite]
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
from refit_timing import W, H, instances, moved  # noqa: E402
from instances_timing import emissive_instances  # noqa: E402

COUNTS = (1, 15)
CALLS = 5


def write_profile(path, a, rows, plain, bench):
    out = ["The emitter mode on bench.py's headline workload (config 4, %s footprint, %dx%d), one run of scripts/emitters_timing.py." % (a.footprint, W, H),
           "scene: " + json.dumps([r for r in rows if r["what"] == "scene"][0]),
           "switch-on: " + json.dumps([r for r in rows if r["what"] == "switch on"][0]), "",
           "(a) steady state, %d calls each (mean; min .. max of the wall time), emissive instances appended / removed with the mode on, against rt_upload_scene +" % CALLS,
           "    rt_build_accel of the same new scene on a second context",
           "  change      instances   records   event ms   k_light_expand ms   wall ms (min .. max)        bytes up (call + lights)   upload + host build wall ms   host / device wall"]
    for r in [r for r in rows if r["what"] == "steady"]:
        out.append("  %-10s  %7d   %7d   %8.3f   %14.4f      %8.3f (%7.3f .. %7.3f)   %9d + %-9d      %12.1f                  %7.1f x" % (
            r["change"], r["instances"], r["records"], r["event_ms"], r["expand_ms"], r["wall_ms"], r["wall_ms_min"], r["wall_ms_max"], r["bytes_call"], r["bytes_lights"],
            r["host_route_wall_ms"], r["host_over_device_wall"]))
    if plain:
        out += ["", "(b) rt_set_instances on a non-emissive change (15 instances appended, removed; %d calls each, mean wall / event ms), one process per line, alternated:" % CALLS]
        out += ["  " + l for l in plain]
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "emitters_timing.txt"))
    ap.add_argument("--plain", default=None)
    ap.add_argument("--plain-ab", default=None)
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
    desc = sc.desc(env)
    base = instances(desc)
    emissive = emissive_instances(desc, base)
    rng = np.random.default_rng(5)

    def table(k, pool):
        pick = pool[rng.integers(0, len(pool), k)]
        extra = base[pick].copy()
        offs = rng.normal(0, 1, (k, 3)).astype(np.float32) * np.float32([2.0, 0.2, 2.0])
        extra["objectToWorld"] = moved(extra["objectToWorld"], offs)
        return np.concatenate([base, extra])
    dev = Renderer().setup(0)
    dev.load_scene(desc)
    dev.update(W, H)

    def timed_set(t):
        dev.sync()
        t0 = time.perf_counter()
        dev.set_instances(t)
        return (time.perf_counter() - t0) * 1e3, dev.instances_stats(), (dev.emitter_stats() if hasattr(dev, "emitter_stats") and a.plain != "parent" else None)
    meshes, erows = sc.emitterMeshes()
    if a.plain:      # (b): a change that touches no light, on the library of this process
        if a.plain.endswith("on"):
            dev.set_emitter_meshes(meshes, erows, sc.lightWeights[0])
        pm = np.frombuffer((C.c_char * (desc.numPrimMeshes * 20)).from_address(desc.primMeshes), dtype=np.uint32).reshape(-1, 5)
        tris = pm[base["primMesh"], 3] // 3
        pool = np.nonzero((tris < np.percentile(tris, 90)) & ~emissive)[0]
        timed_set(table(15, pool)); timed_set(base)      # the first calls allocate
        add, rem = [], []
        for _ in range(CALLS):
            add.append(timed_set(table(15, pool)))
            rem.append(timed_set(base))
        print("plain " + json.dumps({"library": a.plain, "add15_wall_ms": round(float(np.mean([x[0] for x in add])), 3), "add15_event_ms": round(float(np.mean([x[1].ms for x in add])), 3),
                                     "remove15_wall_ms": round(float(np.mean([x[0] for x in rem])), 3), "remove15_event_ms": round(float(np.mean([x[1].ms for x in rem])), 3),
                                     "add15_wall_ms_min_max": [round(min(x[0] for x in add), 3), round(max(x[0] for x in add), 3)]}), flush=True)
        dev.destroy()
        return
    hst = Renderer().setup(0)
    hst.load_scene(desc)
    hst.update(W, H)
    pool = np.nonzero(emissive)[0]
    emit({"what": "scene", "footprint": a.footprint, "instances": len(base), "emissive_instances": int(emissive.sum()), "trig_lights": desc.lightInfo.trigLightSize,
          "emissive_prim_meshes": len(meshes), "template_rows": len(erows), **hst.accel_stats()})
    dev.sync()
    t0 = time.perf_counter()
    dev.set_emitter_meshes(meshes, erows, sc.lightWeights[0])
    s = dev.emitter_stats()
    emit({"what": "switch on", "wall_ms": round((time.perf_counter() - t0) * 1e3, 3), "records": s.records, "emitting_instances": s.emittingInstances, "bytes_uploaded": s.bytesUploaded,
          "k_light_expand_ms": round(s.expandMs, 4)})

    def host_route(t):
        sc.setInstances(t)
        d2 = sc.desc(env)
        hst.sync()
        t0 = time.perf_counter()
        hst.load_scene(d2)
        return (time.perf_counter() - t0) * 1e3
    timed_set(table(1, pool)); timed_set(base); timed_set(base)      # the first calls allocate the call's buffers and both sets of light buffers
    for k in COUNTS:
        add, rem = [], []
        for _ in range(CALLS):
            t = table(k, pool)
            add.append(timed_set(t))
            rem.append(timed_set(base))
        for change, runs, tab in (("add %d" % k, add, t), ("remove %d" % k, rem, base)):
            hw = host_route(tab)
            w = [x[0] for x in runs]
            s, e = runs[-1][1], runs[-1][2]
            emit({"what": "steady", "change": change, "instances": s.instances, "records": e.records, "event_ms": round(float(np.mean([x[1].ms for x in runs])), 4),
                  "expand_ms": round(float(np.mean([x[2].expandMs for x in runs])), 4), "wall_ms": round(float(np.mean(w)), 4), "wall_ms_min": round(min(w), 4),
                  "wall_ms_max": round(max(w), 4), "bytes_call": s.bytesUploaded, "bytes_lights": e.bytesUploaded, "reallocated_any": int(any(x[2].reallocated for x in runs)),
                  "host_route_wall_ms": round(hw, 1), "host_over_device_wall": round(hw / float(np.mean(w)), 2)})
    dev.destroy(); hst.destroy()
    read = lambda p: [l.strip() for l in open(p) if l.strip()] if p else []      # noqa: E731
    write_profile(a.out, a, rows, [l for l in read(a.plain_ab) if l.startswith("plain ")], [l for l in read(a.bench_ab) if l.split()[0] in ("parent", "this")])


if __name__ == "__main__":
    main()
