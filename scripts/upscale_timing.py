"""Cost and pay-off of temporal upsampling (rt_set_upscale) on bench.py's flagship scene: per pair render size -> output size

  pass      the RT_STAGE_COMPOSE entry of rt_get_counters per frame with every stage serial on one stream (overlap 0; HIP events; the pass is timed under that
            entry), mode off and on at the render size: the pass alone is the difference.  pass_GBps counts the bytes the pass has to move once:
            72 B per output pixel (the history read and written: two RGBA32F images and n) + 64 B per render pixel (G(f), G(f-1), the two composed images).
  frame     the frame period with frames in flight (overlap 2, host-timed over the steps, synchronised at both ends): the render-size frame plus the pass
            (`upscaled`) and the output-size frame rendered natively (`native`).  --native-only prints the native rows alone and never touches the new entry
            points: run it with RESTIR_HIP_LIB pointing at another build of the library (the parent commit's) for the reference row.
Fixed camera, time = 1000 + f, default settings.

  python scripts/upscale_timing.py [--pairs 1280x720:1920x1080 1920x1080:3840x2160] [--config 4] [--steps 32] [--warmup 8] [--footprint real|lite] [--native-only]
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

# (lite kind, real kind, env, state overrides): bench.py's CONFIGS 3 and 4
CONFIGS = {3: ("PROC_SPONZA", "PROC_SPONZA_1K", (2048, 1024), {"maxDepth": 2}),
           4: ("PROC_BISTRO_EXT", "PROC_BISTRO_EXT_REAL", (2048, 1024), {})}


def run(a, size, out_size, overlap):
    """frames at `size`; out_size: None = mode off (the entry points are not called), else resolved to it"""
    lite, real, env_size, over = CONFIGS[a.config]
    W, H = size
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
    if out_size is not None:
        r.set_upscale(abi.Upscale(mode=abi.UPSCALE_TEMPORAL, outWidth=out_size[0], outHeight=out_size[1]))
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
    out = {"config": a.config, "footprint": a.footprint, "render": list(size), "output": list(out_size) if out_size else None, "overlap": overlap,
           "frames": a.steps, "ms_per_frame_host": round(period, 4)}
    if overlap == 0:
        out["compose_stage_ms"] = round(list(c.stageMs)[abi.STAGE_COMPOSE] / max(1, c.framesTimed), 4)
    r.destroy()
    return out


def size_of(s):
    w, h = s.split("x")
    return int(w), int(h)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--pairs", nargs="+", default=["1280x720:1920x1080", "1920x1080:3840x2160"])
    ap.add_argument("--config", type=int, default=4, choices=sorted(CONFIGS))
    ap.add_argument("--steps", type=int, default=32)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--footprint", default="real", choices=["real", "lite"])
    ap.add_argument("--native-only", action="store_true")
    a = ap.parse_args()
    lib = os.environ.get("RESTIR_HIP_LIB", "")
    for pair in a.pairs:
        lo, hi = map(size_of, pair.split(":"))
        if not a.native_only:
            off = run(a, lo, None, 0)
            on = run(a, lo, hi, 0)
            on["pass_ms"] = round(on["compose_stage_ms"] - off["compose_stage_ms"], 4)
            nbytes = hi[0] * hi[1] * 72 + lo[0] * lo[1] * 64
            on["pass_bytes"] = nbytes
            on["pass_GBps"] = round(nbytes / (on["pass_ms"] * 1e-3) / 1e9, 1) if on["pass_ms"] > 0 else None
            for row, what in ((off, "render size, mode off, serial"), (on, "upscaled, serial")):
                print(json.dumps(dict(row, what=what)), flush=True)
            print(json.dumps(dict(run(a, lo, hi, 2), what="upscaled, frames in flight")), flush=True)
        print(json.dumps(dict(run(a, hi, None, 2), what="native output size, frames in flight", **({"library": lib} if lib else {}))), flush=True)


if __name__ == "__main__":
    main()
