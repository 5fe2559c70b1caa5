"""Cost of the temporal anti-aliasing resolve (rt_set_taa) on bench.py's 1080p workloads: per configuration, TAA off and on, the
RT_STAGE_COMPOSE entry of rt_get_counters per frame with every stage serial on one stream (overlap 0; HIP events; the pass is timed under that entry, so the
pass alone is the difference to mode off, whose compose does the same work), and the frame period with frames in flight (overlap 2, host-timed over the steps,
synchronised at both ends).  Fixed camera, time = 1000 + f, default settings.

  python scripts/taa_timing.py [--configs 4 3] [--steps 32] [--warmup 8] [--footprint real|lite]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import restir_amd  # noqa: E402,F401
from restir_amd import abi, host  # noqa: E402
from restir_amd.renderer import Renderer  # noqa: E402

# (lite kind, real kind, size, env, state overrides): bench.py's CONFIGS 3 and 4
CONFIGS = {3: ("PROC_SPONZA", "PROC_SPONZA_1K", (1920, 1080), (2048, 1024), {"maxDepth": 2}),
           4: ("PROC_BISTRO_EXT", "PROC_BISTRO_EXT_REAL", (1920, 1080), (2048, 1024), {})}
MODES = {"off": abi.TAA_OFF, "on": abi.TAA_ON}


def run(config, mode, overlap, a):
    lite, real, (W, H), env_size, over = CONFIGS[config]
    sc = host.Scene().makeProcedural(getattr(abi, real if a.footprint == "real" else lite), 1.0, 1)
    env = host.HdrSampling()
    env.makeSyntheticSky(env_size[0], env_size[1], 5e4, 7)
    st = host.default_state(W, H, sc, env)
    for k, v in over.items():
        setattr(st, k, v)
    r = Renderer().setup(0)
    r.set_overlap(overlap)
    r.load_scene(sc.desc(env))
    r.update(W, H)
    r.set_taa(abi.Taa(mode=MODES[mode]))
    sc.updateCamera(W, H)
    f = 0
    for _ in range(a.warmup):
        st.time = 1000 + f; sc.updateCamera(W, H); r.set_camera(sc.getCamera()); r.run(st, f); f += 1
    r.sync()
    r.set_counting(0)   # resets the accumulated timings
    t0 = time.perf_counter()
    for _ in range(a.steps):
        st.time = 1000 + f; sc.updateCamera(W, H); r.set_camera(sc.getCamera()); r.run(st, f); f += 1
    r.sync()
    period = (time.perf_counter() - t0) * 1e3 / a.steps
    c = r.counters()
    out = {"config": config, "footprint": a.footprint, "taa": mode, "overlap": overlap, "frames": a.steps, "ms_per_frame_host": round(period, 4)}
    if overlap == 0:
        n = max(1, c.framesTimed)
        out["compose_stage_ms"] = round(list(c.stageMs)[abi.STAGE_COMPOSE] / n, 4)
    r.destroy()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--configs", type=int, nargs="+", default=[4, 3])
    ap.add_argument("--steps", type=int, default=32)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--footprint", default="real", choices=["real", "lite"])
    a = ap.parse_args()
    for config in a.configs:
        base = None
        for overlap in (0, 2):
            for mode in MODES:
                out = run(config, mode, overlap, a)
                if overlap == 0:
                    base = out["compose_stage_ms"] if mode == "off" else base
                    if mode != "off":
                        out["pass_ms"] = round(out["compose_stage_ms"] - base, 4)
                        out["pass_GBps_at_130B_per_px"] = round(1920 * 1080 * 130 / (out["pass_ms"] * 1e-3) / 1e9, 1) if out["pass_ms"] > 0 else None
                print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
