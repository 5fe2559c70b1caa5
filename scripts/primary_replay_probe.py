#!/usr/bin/env python3
"""Settled primary visibility on a bench.py workload with the camera at rest: what the recording found, and what the frames cost.

  python scripts/primary_replay_probe.py [--config N] [--pose N] [--scene-footprint lite|real] [--frames 14] [--overlap 0]

Builds the workload as bench.py does, renders `--frames` frames at rest, synchronising after each (so a frame's time is its own: normal, normal, record, replay, ...),
and prints one JSON line: per-frame ms, rt_get_primary_replay_stats, and the histogram of listed candidates per pixel.  Run it with RESTIR_VIS_K=64 for the
histogram that chooses RT_VIS_K_DEFAULT (the smallest of 8 / 16 / 32 / 64 that leaves under 2 % of the headline view's pixels in overflow), with
RESTIR_PRIMARY_REPLAY=0 for the same frames without the feature."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    import bench
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", type=int, default=4, choices=[2, 3, 4, 5])
    ap.add_argument("--pose", type=int, default=0, choices=[0, 1, 2])
    ap.add_argument("--scene-footprint", choices=["lite", "real"], default=bench.DEFAULT_FOOTPRINT)
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--frames", type=int, default=14)
    ap.add_argument("--overlap", type=int, default=0, help="rt_set_overlap mode (0: every stage in order on one stream, so that a frame's time is the sum of its stages)")
    args = ap.parse_args()
    import restir_amd  # noqa: F401
    from restir_amd import abi, host
    from restir_amd.renderer import Renderer
    cfg = bench.CONFIGS[args.config]
    W, H = cfg["size"]
    scene = host.Scene().makeProcedural(bench.scene_kind(abi, args.config, bench.footprint_of(args)), args.scale, 1)
    bench.apply_pose(args, scene)
    env = None
    if cfg["env"]:
        env = host.HdrSampling()
        env.makeSyntheticSky(cfg["env"][0], cfg["env"][1], 5e4, 7)
    st = host.default_state(W, H, scene, env)
    for k, v in cfg.get("state", {}).items():
        setattr(st, k, v)
    di_only = cfg.get("di_only", False)
    r = Renderer().setup(0)
    r.set_overlap(args.overlap)
    r.load_scene(scene.desc(env))
    r.update(W, H)
    scene.updateCamera(W, H)
    ms, launches = [], []
    for f in range(args.frames):
        st.time = 1000 + f
        scene.updateCamera(W, H)
        r.set_camera(scene.getCamera())
        r.sync()
        t0 = time.perf_counter()
        if di_only:
            r.run_stage(st, f, abi.STAGE_DIRECT, 0)
        else:
            r.run(st, f)
        r.sync()
        ms.append(round((time.perf_counter() - t0) * 1e3, 3))
        s = r.primary_replay_stats()
        launches.append((s.launchesRecorded, s.launchesReplayed))
    s = r.primary_replay_stats()
    out = {"config": args.config, "pose": args.pose, "footprint": bench.footprint_of(args), "size": [W, H], "overlap": args.overlap, "frame_ms": ms, "launches": launches,
           "stats": {k: getattr(s, k) for k in ("state", "K", "pixelsSettled", "pixelsListed", "pixelsOverflow", "launchesRecorded", "launchesReplayed")}}
    if s.state == 1:
        cnt = r.primary_replay_readback(W, H).reshape(-1)
        listed = cnt[cnt != 0xffffffff]
        edges = [0, 1, 2, 3, 5, 9, 17, 33, 65]
        out["histogram"] = {("%d" % a if b == a + 1 else "%d-%d" % (a, b - 1)): int(((listed >= a) & (listed < b)).sum()) for a, b in zip(edges, edges[1:])}
        out["histogram"]["overflow"] = int((cnt == 0xffffffff).sum())
        n = float(cnt.size)
        out["over_k_percent"] = {str(k): round(100.0 * (int((listed > k).sum()) + int((cnt == 0xffffffff).sum())) / n, 3) for k in (8, 16, 32, 64) if k <= s.K}
        out["mean_listed"] = round(float(listed.mean()), 3) if listed.size else 0.0
        out["plane_bytes"] = int(cnt.size) * 4 * (2 + s.K)
    r.destroy()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
