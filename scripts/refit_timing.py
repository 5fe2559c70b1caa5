"""What moving instances costs (rt_update_instances) on bench.py's headline workload (config 4, 1080p).

  update    one instance, about 1 %, 10 % and all instances translated: HIP-event time of the call's kernels (rt_get_refit_stats) and host wall time of the call
            including the drain, against what the same change costs without the call: rt_upload_scene + rt_build_accel of the moved scene (host wall time).
  degrade   every instance but the largest meshes (ground, facades) displaced by a growing random offset, cumulatively refitted: ms per frame (frames in flight,
            host-timed) on the refitted tree against a fresh build of the same moved scene.

  python scripts/refit_timing.py [--footprint real|lite] [--steps 24] [--warmup 8] [--skip-degrade] [--skip-update] [--degrade-directions random|inward]
One JSON line per measurement."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import restir_amd  # noqa: E402,F401
from restir_amd import abi, host  # noqa: E402
from restir_amd.renderer import Renderer  # noqa: E402

W, H = 1920, 1080
INSTANCE_DT = np.dtype([("objectToWorld", "<f4", 12), ("primMesh", "<u4"), ("flags", "<u4")])


def instances(desc):
    return np.frombuffer((C.c_char * (desc.numInstances * 56)).from_address(desc.instances), dtype=INSTANCE_DT).copy()


def moved(xf, offsets):
    out = xf.copy()
    out[:, 3] += offsets[:, 0]; out[:, 7] += offsets[:, 1]; out[:, 11] += offsets[:, 2]
    return out


def frame_ms(r, sc, st, a, f0):
    f = f0
    for _ in range(a.warmup):
        st.time = 1000 + f; sc.updateCamera(W, H); r.set_camera(sc.getCamera()); r.run(st, f); f += 1
    r.sync()
    t0 = time.perf_counter()
    for _ in range(a.steps):
        st.time = 1000 + f; sc.updateCamera(W, H); r.set_camera(sc.getCamera()); r.run(st, f); f += 1
    r.sync()
    return (time.perf_counter() - t0) * 1e3 / a.steps, f


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--footprint", default="real", choices=["real", "lite"])
    ap.add_argument("--steps", type=int, default=24)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--skip-degrade", action="store_true")
    ap.add_argument("--skip-update", action="store_true")
    ap.add_argument("--degrade-directions", default="random", choices=["random", "inward"],
                    help="random: any direction (instances at the rim move outward, the pad grows and every step is a full refit); inward: towards the scene's centre in x / z (the pad never grows)")
    a = ap.parse_args()
    kind = abi.PROC_BISTRO_EXT_REAL if a.footprint == "real" else abi.PROC_BISTRO_EXT
    sc = host.Scene().makeProcedural(kind, 1.0, 1)
    env = host.HdrSampling()
    env.makeSyntheticSky(2048, 1024, 5e4, 7)
    st = host.default_state(W, H, sc, env)
    desc = sc.desc(env)
    home = instances(desc)["objectToWorld"]
    n = len(home)
    rng = np.random.default_rng(5)
    r = Renderer().setup(0)
    t0 = time.perf_counter()
    r.load_scene(desc)
    load_s = time.perf_counter() - t0
    r.update(W, H)
    print(json.dumps({"what": "scene", "footprint": a.footprint, "instances": n, **r.accel_stats(), "first_load_s": round(load_s, 3)}), flush=True)
    base_ms, f = frame_ms(r, sc, st, a, 0)
    print(json.dumps({"what": "frame", "tree": "fresh build, nothing moved", "ms_per_frame": round(base_ms, 4)}), flush=True)

    # ---- update time by the number of moved instances (the first call also derives the update's maps from the device tree: reported on its own)
    t0 = time.perf_counter()
    r.update_instances([], np.zeros((0, 12), np.float32))
    print(json.dumps({"what": "first update (derives the record -> node map, level ranges, per-instance maxima)", "wall_ms": round((time.perf_counter() - t0) * 1e3, 3)}), flush=True)
    order = rng.permutation(n)
    for label, k in (() if a.skip_update else (("1 instance", 1), ("1 %", max(1, n // 100)), ("10 %", max(1, n // 10)), ("all", n))):
        ids = np.sort(order[:k]).astype(np.uint32)
        for rep in range(3):
            xf = moved(home[ids], rng.normal(0, 0.05, (k, 3)).astype(np.float32))
            r.sync()
            t0 = time.perf_counter()
            r.update_instances(ids, xf)
            wall = (time.perf_counter() - t0) * 1e3
            s = r.refit_stats()
            print(json.dumps({"what": "update", "moved": label, "instances": int(k), "rep": rep, "event_ms": round(s.ms, 4), "wall_ms": round(wall, 4), "leaf_records": s.leafRecords,
                              "nodes_refitted": s.nodes, "levels": s.levels, "full_refit": s.fullRefit}), flush=True)
        sc.updateInstances(ids, xf)
        d2 = sc.desc(env)
        t0 = time.perf_counter()
        r.load_scene(d2)
        print(json.dumps({"what": "rebuild", "moved": label, "upload_scene_plus_build_accel_wall_ms": round((time.perf_counter() - t0) * 1e3, 1)}), flush=True)
        sc.updateInstances(ids, home[ids])
        r.load_scene(sc.desc(env))

    if a.skip_degrade:
        r.destroy()
        return
    # ---- tree degradation: cumulative refits of a growing displacement against a fresh build of the same scene
    pm = np.frombuffer((C.c_char * (desc.numPrimMeshes * 20)).from_address(desc.primMeshes), dtype=np.uint32).reshape(-1, 5)
    tris = pm[instances(desc)["primMesh"], 3] // 3
    movable = np.nonzero(tris < np.percentile(tris, 90))[0].astype(np.uint32)    # the props, trees, lamps and furniture; the ground and the facades stay
    direction = rng.normal(0, 1, (len(movable), 3)).astype(np.float32)
    direction[:, 1] *= 0.2
    if a.degrade_directions == "inward":
        pos = home[movable][:, [3, 7, 11]]
        direction[:, 0] = -np.sign(pos[:, 0]) * np.abs(direction[:, 0]); direction[:, 2] = -np.sign(pos[:, 2]) * np.abs(direction[:, 2]); direction[:, 1] = -np.abs(direction[:, 1]) * 0.0
    fresh = Renderer().setup(0)
    f = 0
    for disp in (0.05, 0.1, 0.25, 0.5, 1.0, 2.0, 4.0):
        xf = moved(home[movable], direction * np.float32(disp))
        r.update_instances(movable, xf)
        s = r.refit_stats()
        sc.updateInstances(movable, xf)
        d2 = sc.desc(env)
        r.update_lights(d2)
        ms_refit, f = frame_ms(r, sc, st, a, f)
        fresh.load_scene(d2)
        fresh.update(W, H)
        ms_fresh, _ = frame_ms(fresh, sc, st, a, 0)
        print(json.dumps({"what": "degrade", "displacement_sigma_m": disp, "moved_instances": int(len(movable)), "ms_per_frame_refitted": round(ms_refit, 4),
                          "ms_per_frame_fresh_build": round(ms_fresh, 4), "ratio": round(ms_refit / ms_fresh, 4), "update_event_ms": round(s.ms, 4), "full_refit": s.fullRefit}), flush=True)
    r.destroy(); fresh.destroy()


if __name__ == "__main__":
    main()
