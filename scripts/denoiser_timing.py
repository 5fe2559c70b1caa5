"""Timing A/B of the two denoisers (rt_set_denoiser: A-Trous vs SVGF) on bench.py's 1080p workloads: per configuration and mode, the filter
chains' stageMs per frame (rt_get_counters: RT_STAGE_DENOISE_DIRECT / _INDIRECT, HIP events) with every stage serial on one stream (overlap 0),
and the frame period with frames in flight (overlap 2, host-timed over the steps, synchronised at both ends).  Fixed camera, time = 1000 + f.

  python scripts/denoiser_timing.py [--configs 4 3] [--steps 32] [--warmup 8] [--footprint real|lite]
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


def run(config, mode, overlap, steps, warmup, footprint):
    lite, real, (W, H), env_size, over = CONFIGS[config]
    sc = host.Scene().makeProcedural(getattr(abi, real if footprint == "real" else lite), 1.0, 1)
    env = host.HdrSampling()
    env.makeSyntheticSky(env_size[0], env_size[1], 5e4, 7)
    st = host.default_state(W, H, sc, env)
    for k, v in over.items():
        setattr(st, k, v)
    r = Renderer().setup(0)
    r.set_overlap(overlap)
    r.load_scene(sc.desc(env))
    r.update(W, H)
    r.set_denoiser(abi.Denoiser(mode=mode))
    sc.updateCamera(W, H)
    f = 0
    for _ in range(warmup):
        st.time = 1000 + f; sc.updateCamera(W, H); r.set_camera(sc.getCamera()); r.run(st, f); f += 1
    r.sync()
    r.set_counting(0)   # resets the accumulated timings
    t0 = time.perf_counter()
    for _ in range(steps):
        st.time = 1000 + f; sc.updateCamera(W, H); r.set_camera(sc.getCamera()); r.run(st, f); f += 1
    r.sync()
    period = (time.perf_counter() - t0) * 1e3 / steps
    c = r.counters()
    out = {"config": config, "footprint": footprint, "denoiser": "svgf" if mode == abi.DENOISER_SVGF else "atrous", "overlap": overlap,
           "frames": steps, "ms_per_frame_host": round(period, 4)}
    if overlap == 0:
        n = max(1, c.framesTimed)
        sm = list(c.stageMs)
        out.update(filter_direct_ms=round(sm[abi.STAGE_DENOISE_DIRECT] / n, 4), filter_indirect_ms=round(sm[abi.STAGE_DENOISE_INDIRECT] / n, 4),
                   compose_ms=round(sm[abi.STAGE_COMPOSE] / n, 4))
    r.destroy()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", type=int, nargs="+", default=[4, 3])
    ap.add_argument("--steps", type=int, default=32)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--footprint", default="real", choices=["real", "lite"])
    a = ap.parse_args()
    for config in a.configs:
        for overlap in (0, 2):
            for mode in (abi.DENOISER_ATROUS, abi.DENOISER_SVGF):
                print(json.dumps(run(config, mode, overlap, a.steps, a.warmup, a.footprint)), flush=True)


if __name__ == "__main__":
    main()
