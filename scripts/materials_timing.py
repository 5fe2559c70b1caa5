"""What editing materials and texels on the device costs (rt_update_materials / rt_update_texture) on bench.py's headline workload (config 4, 1080p).

  (a) rt_update_materials changing alphaCutoff of every RT_ALPHA_MASK material (the foliage and cut-out materials), CALLS calls that alternate between two
      cutoffs: HIP-event ms from rt_get_material_stats, host wall time, the alpha records rebuilt, the leaf records rewritten and the texels scanned;
  (b) rt_update_texture of one full cut-out texture (every alpha byte changes and changes back), CALLS calls;
  (c) ms per frame (frames in flight, host-timed) before the edits and after them, REPEATS runs each: the spread among the runs is stated beside the means;
  (d) the only route there was before the calls: rt_upload_scene + rt_build_accel of the edited scene, host wall time.  With --parent-lib FILE it runs in a child
      process on that library (the parent commit's build of csrc/librestir_hip.so), else on this one: the two calls are the same code in both.

  python scripts/materials_timing.py [--footprint real|lite] [--steps 24] [--warmup 8] [--parent-lib FILE] [--out profiles/materials_timing.txt]
One JSON line per measurement on stdout; the tables made of them are written to --out."""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import restir_amd  # noqa: E402,F401
from restir_amd import abi, host  # noqa: E402
from restir_amd.renderer import Renderer  # noqa: E402
from refit_timing import W, H, frame_ms  # noqa: E402

CALLS, REPEATS = 6, 3
CUTOFFS = (0.35, 0.5)
ALPHA_MASK = 1
W_BASE_TEXTURE, W_ALPHA_MODE, W_ALPHA_CUTOFF = 4, 17, 18


def materials_of(desc):
    return np.frombuffer((C.c_char * (desc.numMaterials * 80)).from_address(desc.materials), dtype=np.uint32).reshape(-1, 20).copy()


def texture_of(desc, t):
    row = np.frombuffer((C.c_char * 32).from_address(desc.textures + 32 * t), dtype=np.uint8)
    ptr, (w, h) = int(row[:8].view(np.uint64)[0]), [int(x) for x in row[8:16].view(np.int32)]
    return np.frombuffer((C.c_char * (w * h * 4)).from_address(ptr), dtype=np.uint8).reshape(h, w, 4).copy()


def scene(footprint):
    kind = abi.PROC_BISTRO_EXT_REAL if footprint == "real" else abi.PROC_BISTRO_EXT
    sc = host.Scene().makeProcedural(kind, 1.0, 1)
    env = host.HdrSampling()
    env.makeSyntheticSky(2048, 1024, 5e4, 7)
    return sc, env


def with_cutoff(mats, ids, cutoff):
    rows = mats[ids].copy()
    rows[:, W_ALPHA_CUTOFF] = np.array([cutoff], np.float32).view(np.uint32)[0]
    return rows


def host_route(a):
    """(d): in this process, on whatever library RESTIR_HIP_LIB names"""
    sc, env = scene(a.footprint)
    mats = materials_of(sc.desc(env))
    ids = np.nonzero(mats[:, W_ALPHA_MODE] == ALPHA_MASK)[0].astype(np.uint32)
    r = Renderer().setup(0)
    r.load_scene(sc.desc(env))
    r.update(W, H)
    walls = []
    for k in range(REPEATS):
        sc.setMaterials(ids, with_cutoff(mats, ids, CUTOFFS[k % 2]))
        d = sc.desc(env)
        r.sync()
        t0 = time.perf_counter()
        r.load_scene(d)
        walls.append((time.perf_counter() - t0) * 1e3)
    print(json.dumps({"what": "host route", "library": "the parent commit's build" if a.parent else "this", "wall_ms": [round(x, 1) for x in walls]}), flush=True)
    r.destroy()


def write_profile(path, a, rows):
    get = lambda what: [r for r in rows if r["what"] == what]      # noqa: E731
    out = ["rt_update_materials / rt_update_texture on bench.py's headline workload (config 4, %s footprint, %dx%d), one run of scripts/materials_timing.py --steps %d --warmup %d."
           % (a.footprint, W, H, a.steps, a.warmup), "scene: " + json.dumps(get("scene")[0]), "",
           "(a) rt_update_materials: alphaCutoff of the %d RT_ALPHA_MASK materials, %d calls alternating %s" % (get("scene")[0]["mask_materials"], CALLS, list(CUTOFFS))]
    out += ["  " + json.dumps(r) for r in get("materials")]
    out += ["", "(b) rt_update_texture: one full cut-out texture, every alpha byte changed, %d calls" % CALLS]
    out += ["  " + json.dumps(r) for r in get("texture")]
    out += ["", "(c) ms per frame (frames in flight, host-timed), %d runs before the edits and %d after:" % (REPEATS, REPEATS)]
    out += ["  " + json.dumps(r) for r in get("frame")]
    out += ["", "(d) the route without the calls, rt_upload_scene + rt_build_accel of the edited scene (host wall time; every run builds: the cache key changes"
            " with the cutoff):"]
    out += ["  " + json.dumps(r) for r in get("host route")]
    s = get("summary")
    if s:
        out += ["", "summary: " + json.dumps(s[0])]
    with open(path, "w") as f:
        f.write("\n".join(out) + "\n")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--footprint", default="real", choices=["real", "lite"])
    ap.add_argument("--steps", type=int, default=24)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--host-route-only", action="store_true", help="(internal) run (d) and exit")
    ap.add_argument("--parent", action="store_true", help="(internal) the library in use is --parent-lib's")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "materials_timing.txt"))
    a = ap.parse_args()
    if a.host_route_only:
        return host_route(a)
    rows = []

    def emit(row):
        rows.append(row)
        print(json.dumps(row), flush=True)
    sc, env = scene(a.footprint)
    st = host.default_state(W, H, sc, env)
    desc = sc.desc(env)
    mats = materials_of(desc)
    ids = np.nonzero(mats[:, W_ALPHA_MODE] == ALPHA_MASK)[0].astype(np.uint32)
    r = Renderer().setup(0)
    r.load_scene(desc)
    r.update(W, H)
    emit({"what": "scene", "footprint": a.footprint, "materials": len(mats), "mask_materials": len(ids), "textures": desc.numTextures, **r.accel_stats()})
    f = 0
    before = []
    for _ in range(REPEATS):
        ms, f = frame_ms(r, sc, st, a, f)
        before.append(ms)
    # (a)
    for k in range(CALLS):
        rows_k = with_cutoff(mats, ids, CUTOFFS[k % 2])
        r.sync()
        t0 = time.perf_counter()
        r.update_materials(ids, rows_k)
        wall = (time.perf_counter() - t0) * 1e3
        s = r.material_stats()
        emit({"what": "materials", "call": k, "cutoff": CUTOFFS[k % 2], "event_ms": round(s.ms, 4), "wall_ms": round(wall, 4), "dirty_materials": s.dirtyMaterials,
              "alpha_records": s.alphaRecords, "leaf_records": s.leafRecords, "texels_scanned": s.texelsScanned, "bytes_uploaded": s.bytesUploaded})
    # (b): the base colour texture of the first MASK material that has one
    tex = next(int(t) for t in mats[ids, W_BASE_TEXTURE].view(np.int32) if t >= 0)
    texels = texture_of(desc, tex)
    users = int((mats[:, W_BASE_TEXTURE].view(np.int32) == tex).sum())
    for k in range(CALLS):
        edited = texels.copy()
        if k % 2 == 0:
            edited[..., 3] = 255 - edited[..., 3]
        r.sync()
        t0 = time.perf_counter()
        r.update_texture(tex, 0, 0, edited)
        wall = (time.perf_counter() - t0) * 1e3
        s = r.material_stats()
        emit({"what": "texture", "call": k, "texture": tex, "size": [texels.shape[1], texels.shape[0]], "materials_using_it": users, "event_ms": round(s.ms, 4),
              "wall_ms": round(wall, 4), "alpha_records": s.alphaRecords, "leaf_records": s.leafRecords, "texels_scanned": s.texelsScanned, "bytes_uploaded": s.bytesUploaded})
    after = []
    for _ in range(REPEATS):
        ms, f = frame_ms(r, sc, st, a, f)
        after.append(ms)
    spread = lambda x: round((max(x) / min(x) - 1) * 100, 2)      # noqa: E731
    emit({"what": "frame", "ms_per_frame_before": [round(x, 4) for x in before], "ms_per_frame_after": [round(x, 4) for x in after],
          "mean_before": round(float(np.mean(before)), 4), "mean_after": round(float(np.mean(after)), 4), "after_over_before": round(float(np.mean(after) / np.mean(before)), 4),
          "spread_before_percent": spread(before), "spread_after_percent": spread(after)})
    r.destroy()
    # (d)
    cmd = [sys.executable, os.path.abspath(__file__), "--host-route-only", "--footprint", a.footprint]
    envp = dict(os.environ)
    if a.parent_lib:
        envp["RESTIR_HIP_LIB"] = os.path.abspath(a.parent_lib)
        cmd.append("--parent")
    out = subprocess.run(cmd, env=envp, capture_output=True, text=True, timeout=900)
    for line in out.stdout.splitlines():
        if line.startswith("{"):
            emit(json.loads(line))
    route = [x for x in rows if x["what"] == "host route"]
    if route:
        d = float(np.mean(route[0]["wall_ms"]))
        am = [x for x in rows if x["what"] == "materials"][1:]      # (the first call allocates the device words)
        bt = [x for x in rows if x["what"] == "texture"]
        emit({"what": "summary", "host_route_wall_ms": round(d, 1), "update_materials_wall_ms": round(float(np.mean([x["wall_ms"] for x in am])), 3),
              "update_texture_wall_ms": round(float(np.mean([x["wall_ms"] for x in bt])), 3),
              "host_over_update_materials": round(d / float(np.mean([x["wall_ms"] for x in am])), 1),
              "host_over_update_texture": round(d / float(np.mean([x["wall_ms"] for x in bt])), 1)})
    else:
        print(out.stdout[-2000:], out.stderr[-2000:], file=sys.stderr)
    write_profile(a.out, a, rows)


if __name__ == "__main__":
    main()
