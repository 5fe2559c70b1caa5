"""What object motion vectors cost and buy (rt_set_object_motion).

  cost      bench.py's headline workload (config 4, 1080p): ms per frame (frames in flight, host-timed) on one sequence in which 1 %, 10 % and all instances
            translate a little every frame (rt_update_instances before each frame: its drain is part of both sides), with the mode off and on; and the same
            without any motion (mode on: the object-motion builds without a table).
  quality   Cornell, 256 x 192, temporal reuse, a static camera, the two boxes translating: for every moved pose the converged image of rt_reference_*, and the
            mean relative error of the composed frame (direct + indirect result) over the pixels of the moving boxes, with the mode off and on.

  python scripts/object_motion.py [--footprint real|lite] [--steps 24] [--warmup 8] [--skip-cost] [--skip-quality] [--spp 2048]
One JSON line per measurement.  (The default path's A/B against the parent's library is bench.py's own, run with RESTIR_HIP_LIB; see profiles/object_motion.txt.)"""
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

INSTANCE_DT = np.dtype([("objectToWorld", "<f4", 12), ("primMesh", "<u4"), ("flags", "<u4")])
LUM = np.array([0.2126, 0.7152, 0.0722])


def instances(desc):
    return np.frombuffer((C.c_char * (desc.numInstances * 56)).from_address(desc.instances), dtype=INSTANCE_DT).copy()


def moved(xf, offsets):
    out = xf.copy()
    out[:, 3] += offsets[:, 0]; out[:, 7] += offsets[:, 1]; out[:, 11] += offsets[:, 2]
    return out


def cost(a):
    W, H = 1920, 1080
    kind = abi.PROC_BISTRO_EXT_REAL if a.footprint == "real" else abi.PROC_BISTRO_EXT
    sc = host.Scene().makeProcedural(kind, 1.0, 1)
    env = host.HdrSampling()
    env.makeSyntheticSky(2048, 1024, 5e4, 7)
    st = host.default_state(W, H, sc, env)
    desc = sc.desc(env)
    home = instances(desc)["objectToWorld"]
    n = len(home)
    order = np.random.default_rng(5).permutation(n)
    r = Renderer().setup(0)
    r.load_scene(desc)
    r.update(W, H)
    r.update_instances([], np.zeros((0, 12), np.float32))    # the update's maps, derived once
    f = 0
    for label, k in (("none", 0), ("1 %", max(1, n // 100)), ("10 %", max(1, n // 10)), ("all", n)):
        ids = np.sort(order[:k]).astype(np.uint32)
        step = np.tile(np.array([[0.004, 0.0, 0.002]], np.float32), (k, 1))
        res = {}
        for mode in (abi.OBJECT_MOTION_OFF, abi.OBJECT_MOTION_ON, abi.OBJECT_MOTION_OFF, abi.OBJECT_MOTION_ON):
            r.set_object_motion(mode)
            t0 = None
            for i in range(a.warmup + a.steps):
                if i == a.warmup:
                    r.sync(); t0 = time.perf_counter()
                if k:
                    r.update_instances(ids, moved(home[ids], step * np.float32(1 + i % 8)))
                st.time = 1000 + f; sc.updateCamera(W, H); r.set_camera(sc.getCamera()); r.run(st, f); f += 1
            r.sync()
            res.setdefault(mode, []).append(round((time.perf_counter() - t0) * 1e3 / a.steps, 4))
            if k:
                r.update_instances(ids, home[ids])
        print(json.dumps({"what": "cost", "in_motion": label, "instances": int(k), "of": n, "ms_per_frame_off": res[0], "ms_per_frame_on": res[1],
                          "on_over_off": round(float(np.mean(res[1]) / np.mean(res[0])), 4)}), flush=True)
    r.destroy()


def quality(a):
    W, H = 256, 192
    sc = host.Scene().makeProcedural(abi.PROC_CORNELL)
    st = host.default_state(W, H, sc, None)
    st.environmentProb = 0.0
    st.ReSTIRState = abi.RESTIR_TEMPORAL
    st.modulate = 1          # the composed images carry the albedo, like the reference's (scripts/reference_bias.py)
    desc = sc.desc(None)
    home = instances(desc)["objectToWorld"]
    ids = np.array([3, 4], np.uint32)
    sc.updateCamera(W, H); sc.updateCamera(W, H)
    cam = sc.getCamera()
    frames = 8
    out = {}
    for mode in (abi.OBJECT_MOTION_OFF, abi.OBJECT_MOTION_ON):
        r = Renderer().setup(0)
        r.load_scene(desc)
        r.update(W, H)
        r.set_object_motion(abi.OBJECT_MOTION_ON)    # (on for the warm-up frame, so that both runs have the instance image of the props)
        errs = []
        for f in range(frames):
            if f == 1:
                r.set_object_motion(mode)
            xf = moved(home[ids], np.tile(np.array([[0.012 * f, 0.0, 0.004 * f]], np.float32), (2, 1)))
            r.update_instances(ids, xf)
            st.time = 1000 + f
            r.set_camera(cam)
            r.run(st, f)
            img = (r.readback(abi.BUF_DIRECT_RESULT0 + (f & 1)).view(np.float32).reshape(H, W, 4)[..., :3].astype(np.float64)
                   + r.readback(abi.BUF_INDIRECT_RESULT0 + (f & 1)).view(np.float32).reshape(H, W, 4)[..., :3])
            if f < 2:
                continue
            pick = np.full((H, W), -1)
            for y in range(H):
                for x in range(W):
                    pick[y, x] = r.pick(cam.viewInverse, cam.projInverse, (x + 0.5) / W, (y + 0.5) / H).instanceID
            mask = np.isin(pick, ids)
            r.reference_reset()
            r.reference_render(st, a.spp)
            ref = r.reference_readback(abi.REF_SUM)[..., :3].astype(np.float64)
            lf, lg = img[mask] @ LUM, ref[mask] @ LUM
            errs.append(float(np.abs(lf - lg).mean() / lg.mean()))
        out[mode] = errs
        r.destroy()
    print(json.dumps({"what": "quality", "scene": "cornell 256x192, boxes 3 and 4 translating, static camera, temporal reuse", "reference_spp": a.spp,
                      "mean_relative_error_off_by_frame": [round(e, 4) for e in out[0]], "mean_relative_error_on_by_frame": [round(e, 4) for e in out[1]],
                      "mean_off": round(float(np.mean(out[0])), 4), "mean_on": round(float(np.mean(out[1])), 4)}), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--footprint", default="real", choices=["real", "lite"])
    ap.add_argument("--steps", type=int, default=24)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--spp", type=int, default=2048)
    ap.add_argument("--skip-cost", action="store_true")
    ap.add_argument("--skip-quality", action="store_true")
    a = ap.parse_args()
    if not a.skip_quality:
        quality(a)
    if not a.skip_cost:
        cost(a)


if __name__ == "__main__":
    main()
