"""What rebuilding on the device costs and buys (rt_rebuild_accel) on bench.py's headline workload (config 4, 1080p).

Every instance but the largest meshes is displaced by a growing offset (scripts/refit_timing.py's degrade sequence).  Three contexts follow the scene: one refits
cumulatively (rt_update_instances), one refits and then rebuilds on the device (rt_rebuild_accel), one uploads and host-builds the moved scene (rt_upload_scene +
rt_build_accel: what a host needs without the call).  Per displacement:
  (a) the device rebuild (HIP events, and host wall time including the drain) against the host rebuild (host wall time) of the same moved scene, and their ratio;
  (b) ms per frame on the device-built tree against the host-built tree;
  (c) ... and against the cumulatively refitted tree;
  (d) node / triangle steps per frame of the device-built and the host-built tree (rt_set_counting), at the first and the last displacement.

  python scripts/accel_build_timing.py [--footprint real|lite] [--steps 24] [--warmup 8] [--out profiles/accel_build_timing.txt] [--bench-ab FILE]
One JSON line per measurement on stdout; the tables made of them are written to --out.  --bench-ab FILE: lines "parent {bench.py's JSON line}" / "this {...}" of
bench.py --gpus 1 --steps 100 --warmup 20 run on the parent commit's library and on this one, alternated in the same visit (RESTIR_HIP_LIB selects the library);
they go into the default-path section of the file."""
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


def steps_per_frame(r, sc, st, f):
    """node / triangle steps of one frame with the counting build of the traced kernels"""
    r.sync()
    r.set_counting(True)
    before = r.counters()
    st.time = 1000 + f; sc.updateCamera(W, H); r.set_camera(sc.getCamera()); r.run(st, f)
    r.sync()
    after = r.counters()
    r.set_counting(False)
    return int(after.nodesVisited - before.nodesVisited), int(after.trisTested - before.trisTested)


def write_profile(path, a, rows, bench):
    """the tables of profiles/accel_build_timing.txt from the run's JSON rows"""
    out = ["rt_rebuild_accel on bench.py's headline workload (config 4, %s footprint, %dx%d), one run of scripts/accel_build_timing.py --steps %d --warmup %d." % (a.footprint, W, H, a.steps, a.warmup),
           "Three contexts follow scripts/refit_timing.py's degrade sequence (every instance but the largest meshes displaced by sigma): one refits cumulatively, one refits",
           "and rebuilds on the device, one uploads and host-builds the moved scene.", "",
           "scene (host build):   " + json.dumps(rows[0]), "first device rebuild: " + json.dumps(rows[1]), "",
           "(a) rebuild of the same moved scene: device (HIP events / host wall incl. the drain) against rt_upload_scene + rt_build_accel (host wall)",
           "  sigma   device event ms   of which sort   device wall ms   host wall ms   host / device   device nodes/levels   host nodes/depth"]
    reb = [r for r in rows if r["what"] == "rebuild"]
    frm = [r for r in rows if r["what"] == "frame"]
    for r in reb:
        out.append("  %-5s   %9.3f         %7.3f         %8.3f         %8.1f       %7.1f x       %7d / %2d          %7d / %2d" % (
            r["displacement_sigma_m"], r["device_event_ms"], r["device_sort_ms"], r["device_wall_ms"], r["host_upload_plus_build_wall_ms"], r["host_over_device_wall"],
            r["device_nodes"], r["device_levels"], r["host_nodes"], r["host_depth"]))
    out += ["", "(b), (c) ms per frame (frames in flight, host-timed): device-built tree against the host-built tree and against the cumulatively refitted tree",
            "  sigma   device-built   host-built   refitted   device / host   refitted / device"]
    for r in frm:
        out.append("  %-5s   %8.3f      %8.3f    %8.3f     %6.3f x        %6.2f x" % (r["displacement_sigma_m"], r["ms_per_frame_device_built"], r["ms_per_frame_host_built"],
                                                                                 r["ms_per_frame_refitted"], r["device_over_host"], r["refitted_over_device"]))
    out += ["", "(d) node / triangle steps of one frame (rt_set_counting)"]
    out += ["  " + json.dumps(r) for r in rows if r["what"] == "steps per frame"]
    ratio = [r["host_over_device_wall"] for r in reb]
    out += ["", "The one condition on time, device rebuild faster than the host rebuild measured in the same run: host / device = %.1f .. %.1f x (%s)." % (
        min(ratio), max(ratio), "met" if min(ratio) > 1.0 else "NOT met"),
        "Frames on the device-built tree (an LBVH: no SAH, no spatial splits) take %.2f .. %.2f x the host-built tree's time; the refitted tree takes %.1f .. %.1f x the" % (
        min(r["device_over_host"] for r in frm), max(r["device_over_host"] for r in frm), min(r["refitted_over_device"] for r in frm), max(r["refitted_over_device"] for r in frm)),
        "device-built tree's."]
    if bench:
        out += ["", "Default path: bench.py --gpus 1 --steps 100 --warmup 20, the parent commit's library and this one alternated in one visit."]
        ms = {"parent": [], "this": []}
        for line in bench:
            who, js = line.split(None, 1)
            d = json.loads(js)
            ms[who].append(d["ms_per_step"])
            out.append("  %-6s  ms_per_step %.4f   %.2f %s" % (who, d["ms_per_step"], d["value"], d["unit"]))
        if ms["parent"] and ms["this"]:
            mp, mt = sum(ms["parent"]) / len(ms["parent"]), sum(ms["this"]) / len(ms["this"])
            out.append("  mean parent %.4f ms, this %.4f ms: %+.2f %% (run-to-run spread 0.3-0.4 %%, DESIGN.md section 18); the default path never calls the new code." % (mp, mt, (mt / mp - 1) * 100))
    with open(path, "w") as f:
        f.write("\n".join(out) + "\n")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--footprint", default="real", choices=["real", "lite"])
    ap.add_argument("--steps", type=int, default=24)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "accel_build_timing.txt"))
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
    ctx = {}
    for name in ("refit", "device", "host"):
        ctx[name] = Renderer().setup(0)
        ctx[name].load_scene(desc)
        ctx[name].update(W, H)
    emit({"what": "scene", "footprint": a.footprint, "instances": len(home), **ctx["host"].accel_stats()})
    t0 = time.perf_counter()
    ctx["device"].rebuild_accel()
    s = ctx["device"].rebuild_stats()
    emit({"what": "first rebuild (allocates the working buffers and two trees, derives the per-triangle table and the update's maps)",
                      "wall_ms": round((time.perf_counter() - t0) * 1e3, 3), "event_ms": round(s.ms, 4), **ctx["device"].accel_stats()})
    pm = np.frombuffer((C.c_char * (desc.numPrimMeshes * 20)).from_address(desc.primMeshes), dtype=np.uint32).reshape(-1, 5)
    tris = pm[instances(desc)["primMesh"], 3] // 3
    movable = np.nonzero(tris < np.percentile(tris, 90))[0].astype(np.uint32)
    direction = rng.normal(0, 1, (len(movable), 3)).astype(np.float32)
    direction[:, 1] *= 0.2
    frames = {k: 0 for k in ctx}
    disps = (0.05, 0.1, 0.25, 0.5, 1.0, 2.0, 4.0)
    for disp in disps:
        xf = moved(home[movable], direction * np.float32(disp))
        ctx["refit"].update_instances(movable, xf)
        ctx["device"].update_instances(movable, xf)
        sc.updateInstances(movable, xf)
        d2 = sc.desc(env)
        ctx["device"].sync()
        t0 = time.perf_counter()
        ctx["device"].rebuild_accel()
        dev_wall = (time.perf_counter() - t0) * 1e3
        s = ctx["device"].rebuild_stats()
        t0 = time.perf_counter()
        ctx["host"].load_scene(d2)
        host_wall = (time.perf_counter() - t0) * 1e3
        emit({"what": "rebuild", "displacement_sigma_m": disp, "device_event_ms": round(s.ms, 4), "device_sort_ms": round(s.sortMs, 4), "device_wall_ms": round(dev_wall, 4),
                          "host_upload_plus_build_wall_ms": round(host_wall, 1), "host_over_device_wall": round(host_wall / dev_wall, 2), "device_nodes": s.nodes,
                          "device_levels": s.levels, "host_nodes": ctx["host"].accel_stats()["nodes"], "host_depth": ctx["host"].accel_stats()["max_depth"]})
        ms = {}
        for name in ("device", "host", "refit"):
            ctx[name].update_lights(d2)
            ms[name], frames[name] = frame_ms(ctx[name], sc, st, a, frames[name])
        emit({"what": "frame", "displacement_sigma_m": disp, "ms_per_frame_device_built": round(ms["device"], 4), "ms_per_frame_host_built": round(ms["host"], 4),
                          "ms_per_frame_refitted": round(ms["refit"], 4), "device_over_host": round(ms["device"] / ms["host"], 4),
                          "refitted_over_device": round(ms["refit"] / ms["device"], 4)})
        if disp in (disps[0], disps[-1]):
            out = {"what": "steps per frame", "displacement_sigma_m": disp}
            for name in ("device", "host"):
                nodes, tri = steps_per_frame(ctx[name], sc, st, frames[name])
                frames[name] += 1
                out[name + "_node_steps"], out[name + "_tri_steps"] = nodes, tri
            out["node_steps_device_over_host"] = round(out["device_node_steps"] / max(1, out["host_node_steps"]), 4)
            out["tri_steps_device_over_host"] = round(out["device_tri_steps"] / max(1, out["host_tri_steps"]), 4)
            emit(out)
    for r in ctx.values():
        r.destroy()
    bench = [l.strip() for l in open(a.bench_ab)] if a.bench_ab else []
    write_profile(a.out, a, rows, [l for l in bench if l])


if __name__ == "__main__":
    main()
