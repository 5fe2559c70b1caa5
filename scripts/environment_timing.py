"""What swapping the environment costs (rt_set_environment) on bench.py's headline scene.

  (a) the device build at 2048 x 1024 and 4096 x 2048 (a random sky with a sun): HIP-event ms from rt_get_environment_stats (copies and kernels) and host wall time
      of the whole call, CALLS calls per size; the first call of a size allocates and is listed apart;
  (b) the same tables on this machine's CPU: HdrSampling::createEnvironmentAccel (host.HdrSampling.setEnvironment, which also copies the texels) and rt_env_accel
      (the device's rule on the host), wall time;
  (c) the copy path (rt_set_environment with a table) at the same sizes;
  (d) the only route there was before the call: rt_upload_scene + rt_build_accel of the scene with the new map, host wall time; the first load builds the tree, the
      later ones find the host build in the cache (the geometry has not changed), so they are the upload alone.

  python scripts/environment_timing.py [--footprint real|lite] [--out profiles/environment_timing.txt]
One JSON line per measurement on stdout; the tables made of them are written to --out."""
import argparse
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
CALLS, REPEATS = 5, 3
SIZES = ((2048, 1024), (4096, 2048))


def sky(w, h, seed):
    rng = np.random.default_rng(seed)
    a = np.ones((h, w, 4), np.float32)
    a[..., :3] = rng.uniform(0.05, 1.0, (h, w, 3)).astype(np.float32)
    a[h // 3, w // 4, :3] = np.float32(5e4)
    return a


def wall(fn):
    t0 = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t0) * 1e3, out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--footprint", default="real", choices=["real", "lite"])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "environment_timing.txt"))
    a = ap.parse_args()
    rows = []

    def emit(row):
        rows.append(row)
        print(json.dumps(row), flush=True)
    sc = host.Scene().makeProcedural(abi.PROC_BISTRO_EXT_REAL if a.footprint == "real" else abi.PROC_BISTRO_EXT, 1.0, 1)
    env0 = host.HdrSampling()
    env0.makeSyntheticSky(2048, 1024, 5e4, 7)
    r = Renderer().setup(0)
    loads = []
    for k in range(REPEATS):      # (d)
        d = sc.desc(env0)
        r.sync()
        loads.append(wall(lambda: r.load_scene(d))[0])
    r.update(W, H)
    emit({"what": "host route", "upload_and_build_wall_ms": [round(x, 1) for x in loads], "note": "first: upload + host build; later: upload + cached build", **r.accel_stats()})
    for w, h in SIZES:
        texels = sky(w, h, w)
        for k in range(CALLS):      # (a)
            r.sync()
            ms, _ = wall(lambda: r.set_environment(texels))
            s = r.environment_stats()
            emit({"what": "device build", "size": [w, h], "call": k, "event_ms": round(s.ms, 4), "wall_ms": round(ms, 3), "smalls": s.numSmall, "larges": s.numLarge,
                  "integral": s.integral, "device_bytes": s.deviceBytes})
        table = r.environment_readback(abi.ENV_ACCEL).copy()
        for k in range(CALLS):      # (c)
            r.sync()
            ms, _ = wall(lambda: r.set_environment(texels, table))
            emit({"what": "copy path", "size": [w, h], "call": k, "event_ms": round(r.environment_stats().ms, 4), "wall_ms": round(ms, 3)})
        e = host.HdrSampling()
        for k in range(REPEATS):      # (b)
            ms_h, _ = wall(lambda: e.setEnvironment(texels))
            ms_r, out = wall(lambda: Renderer.env_accel(texels))
            emit({"what": "cpu", "size": [w, h], "run": k, "HdrSampling_wall_ms": round(ms_h, 1), "rt_env_accel_wall_ms": round(ms_r, 1),
                  "same_table_as_device": bool(np.array_equal(out[0].view(np.uint32), table.view(np.uint32))), "HdrSampling_integral": e.getIntegral(), "rule_integral": out[1]})
    r.destroy()
    get = lambda what: [x for x in rows if x["what"] == what]      # noqa: E731
    out = ["rt_set_environment on bench.py's headline scene (%s footprint), one run of scripts/environment_timing.py." % a.footprint, "",
           "(a) the device build (accel == NULL); event_ms = copies + kernels, wall_ms = the whole call; call 0 of a size allocates"]
    out += ["  " + json.dumps(x) for x in get("device build")]
    out += ["", "(b) the same map on this machine's CPU: HdrSampling::createEnvironmentAccel, and rt_env_accel (the device's rule, sequential)"]
    out += ["  " + json.dumps(x) for x in get("cpu")]
    out += ["", "(c) the copy path (a table handed over)"]
    out += ["  " + json.dumps(x) for x in get("copy path")]
    out += ["", "(d) the route without the call: rt_upload_scene + rt_build_accel with the new map"]
    out += ["  " + json.dumps(x) for x in get("host route")]
    for w, h in SIZES:
        dev = [x for x in get("device build") if x["size"] == [w, h]][1:]
        cpu = [x for x in get("cpu") if x["size"] == [w, h]]
        route = get("host route")[0]["upload_and_build_wall_ms"]
        out += ["", "summary %d x %d: " % (w, h) + json.dumps({
            "device_event_ms": round(float(np.mean([x["event_ms"] for x in dev])), 3), "device_wall_ms": round(float(np.mean([x["wall_ms"] for x in dev])), 3),
            "HdrSampling_wall_ms": round(float(np.mean([x["HdrSampling_wall_ms"] for x in cpu])), 1), "rt_env_accel_wall_ms": round(float(np.mean([x["rt_env_accel_wall_ms"] for x in cpu])), 1),
            "upload_and_build_first_ms": route[0], "upload_and_cached_build_ms": round(float(np.mean(route[1:])), 1)})]
    with open(a.out, "w") as f:
        f.write("\n".join(out) + "\n")


if __name__ == "__main__":
    main()
