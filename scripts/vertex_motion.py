"""What per-vertex motion vectors cost and buy (rt_set_object_motion mode OBJECT_MOTION_VERTEX).

  cost      bench.py's headline workload (config 4, 1080p): ms per frame (frames in flight, host-timed) with the mode off / on / vertex, every row measured
            off, on, vertex, off, on, vertex in one context: nothing moving; one skinned mesh re-posed before every frame (§21's meshes: (a) the most-instanced prim mesh, (b) the
            single-instance prim mesh nearest 1e5 triangles); 1 % of the instances moved before every frame; every instance moved ("everything flagged").  The
            update's drain and refit are part of all three sides.
  quality   the street scene (lite footprint) at 256 x 192, temporal reuse, static camera: the TEXTURED, non-emissive prim mesh with the most pixels under the
            camera is skinned (four joints by height) and oscillates over 8 frames.  For every pose the converged image of rt_reference_* (rendered once per
            pose); per mode and per `time` seed the mean relative error of the composed frame's luminance over the mesh's pixels, frames 2..8, and the share of
            those pixels whose direct reservoir carries history (num > RISSampleNum).  Mean and range over the seeds.

  python scripts/vertex_motion.py [--footprint real|lite] [--steps 24] [--warmup 8] [--spp 2048] [--seeds 4] [--skip-cost] [--skip-quality] [--out profiles/vertex_motion.txt]
One JSON line per measurement on stdout; --out receives them with the tables made of them.  (The default path's A/B against the parent's library is bench.py's own,
run with RESTIR_HIP_LIB.)"""
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
from skin_timing import Skin, PRIM_DT, JOINTS  # noqa: E402
from object_motion import instances, moved, LUM  # noqa: E402

MODES = (abi.OBJECT_MOTION_OFF, abi.OBJECT_MOTION_ON, abi.OBJECT_MOTION_VERTEX)


def scene_arrays(desc):
    pm = np.frombuffer((C.c_char * (desc.numPrimMeshes * 20)).from_address(desc.primMeshes), dtype=PRIM_DT).copy()
    verts = np.frombuffer((C.c_char * (desc.numVertices * 32)).from_address(desc.vertices), dtype=abi.VERTEX_DT).copy()
    mats = np.frombuffer((C.c_char * (desc.numMaterials * 80)).from_address(desc.materials), dtype=np.float32).reshape(-1, 20).copy()
    return pm, verts, mats


def non_emissive(pm, mats):
    lum = 0.2126 * mats[:, 9] + 0.7152 * mats[:, 10] + 0.0722 * mats[:, 11]
    return (lum[np.maximum(pm["materialIndex"], 0)] <= 1e-2) & (pm["vertexCount"] > 0)


def set_one_skin(r, s):
    tab = np.zeros(1, abi.SKIN_DT)
    tab[0] = (s.mesh, 0, JOINTS, 0)
    r.set_skins(tab, s.inf)


def cost(a, emit):
    W, H = 1920, 1080
    kind = abi.PROC_BISTRO_EXT_REAL if a.footprint == "real" else abi.PROC_BISTRO_EXT
    sc = host.Scene().makeProcedural(kind, 1.0, 1)
    env = host.HdrSampling()
    env.makeSyntheticSky(2048, 1024, 5e4, 7)
    st = host.default_state(W, H, sc, env)
    desc = sc.desc(env)
    inst = instances(desc)
    home = inst["objectToWorld"]
    n = len(home)
    pm, verts, mats = scene_arrays(desc)
    usable = non_emissive(pm, mats)
    uses = np.bincount(inst["primMesh"], minlength=len(pm))
    tris = pm["indexCount"] // 3
    mesh_a = int(np.argmax(np.where(usable, uses, -1)))
    mesh_b = int(np.argmin(np.where(usable & (uses == 1), np.abs(tris.astype(np.int64) - 100000), 1 << 60)))
    order = np.random.default_rng(5).permutation(n)
    rows = (("nothing moving", None, 0), ("skinned mesh (a), %d instances" % uses[mesh_a], mesh_a, 0), ("skinned mesh (b), %d triangles" % tris[mesh_b], mesh_b, 0),
            ("1 % of the instances moved", None, max(1, n // 100)), ("every instance moved", None, n))
    f = 0
    for label, mesh, k in rows:
        r = Renderer().setup(0)      # (a context per row: rt_set_skins stays for the life of a scene)
        r.load_scene(desc)
        r.update(W, H)
        r.set_object_motion(abi.OBJECT_MOTION_VERTEX)      # the plane and the images exist for every side
        r.update_instances([], np.zeros((0, 12), np.float32))
        skin = None
        if mesh is not None:
            skin = Skin(verts, pm, mesh)
            set_one_skin(r, skin)
        ids = np.sort(order[:k]).astype(np.uint32)
        step = np.tile(np.array([[0.004, 0.0, 0.002]], np.float32), (k, 1))
        res = {}
        for mode in MODES + MODES:
            r.set_object_motion(mode)
            t0 = None
            for i in range(a.warmup + a.steps):
                if i == a.warmup:
                    r.sync(); t0 = time.perf_counter()
                if k:
                    r.update_instances(ids, moved(home[ids], step * np.float32(1 + i % 8)))
                if skin is not None:
                    r.update_skins([0], skin.matrices(0.5 + 0.5 * np.sin(2 * np.pi * (i % 8) / 8)))
                st.time = 1000 + f; sc.updateCamera(W, H); r.set_camera(sc.getCamera()); r.run(st, f); f += 1
            r.sync()
            res.setdefault(mode, []).append(round((time.perf_counter() - t0) * 1e3 / a.steps, 4))
            if k:
                r.update_instances(ids, home[ids])
        off, on, vtx = (res[m] for m in MODES)
        m0 = float(np.mean(off))
        emit({"what": "cost", "row": label, "ms_per_frame_off": off, "ms_per_frame_on": on, "ms_per_frame_vertex": vtx,
              "on_over_off": round(float(np.mean(on)) / m0, 4), "vertex_over_off": round(float(np.mean(vtx)) / m0, 4),
              "two_runs_differ_pct": [round(100 * abs(x[0] - x[1]) / min(x), 2) for x in (off, on, vtx)]})
        r.destroy()


def quality(a, emit):
    W, H = 256, 192
    frames = 9      # frame 0 at rest, 1..8 one period of the oscillation
    sc = host.Scene().makeProcedural(abi.PROC_BISTRO_EXT, 1.0, 1)
    env = host.HdrSampling()
    env.makeSyntheticSky(2048, 1024, 5e4, 7)
    st = host.default_state(W, H, sc, env)
    st.ReSTIRState = abi.RESTIR_TEMPORAL
    st.modulate = 1
    desc = sc.desc(env)
    inst = instances(desc)
    pm, verts, mats = scene_arrays(desc)
    textured = mats.view(np.int32)[:, 4][np.maximum(pm["materialIndex"], 0)] > -1
    ok = non_emissive(pm, mats) & textured
    sc.updateCamera(W, H); sc.updateCamera(W, H)
    cam = sc.getCamera()
    amount = lambda f: 2.0 * np.sin(2 * np.pi * f / 8)      # noqa: E731  (Skin.matrices: 0.15 rad and 1 % of the mesh's size per unit at the top joint)

    def context():
        r = Renderer().setup(0)
        r.load_scene(desc)
        r.update(W, H)
        r.set_object_motion(abi.OBJECT_MOTION_VERTEX)
        return r

    # the subject: the textured mesh with the most pixels; per pose its mask (the instance image) and the converged image
    r = context()
    st.time = 1; r.set_camera(cam); r.run(st, 0)
    seen = inst["primMesh"][np.minimum(r.object_motion_readback(), len(inst) - 1)]
    seen = seen[r.object_motion_readback() != 0xFFFFFFFF]
    px = np.bincount(seen, minlength=len(pm)) * ok
    mesh = int(np.argmax(px))
    skin = Skin(verts, pm, mesh)
    set_one_skin(r, skin)
    masks, refs = [], []
    for f in range(frames):
        r.update_skins([0], skin.matrices(amount(f)))
        st.time = 10 + f; r.set_camera(cam); r.run(st, f)
        ii = r.object_motion_readback()
        masks.append((inst["primMesh"][np.minimum(ii, len(inst) - 1)] == mesh) & (ii != 0xFFFFFFFF))
        r.reference_reset()
        r.reference_render(st, a.spp)
        refs.append(r.reference_readback(abi.REF_SUM)[..., :3].astype(np.float64).reshape(-1, 3) @ LUM)
    r.destroy()
    emit({"what": "subject", "mesh": mesh, "vertices": skin.count, "instances": int((inst["primMesh"] == mesh).sum()), "pixels_per_frame": [int(m.sum()) for m in masks],
          "material_texture": int(mats.view(np.int32)[max(int(pm["materialIndex"][mesh]), 0), 4]), "reference_spp": a.spp})
    out = {}
    for mode in MODES:
        r = context()
        set_one_skin(r, skin)
        for seed in range(a.seeds):
            r.update(W, H)                       # a fresh history
            r.set_object_motion(mode)
            errs, hist = [], []
            for f in range(frames):
                r.update_skins([0], skin.matrices(amount(f)))
                st.time = 1000 * (seed + 1) + f
                r.set_camera(cam)
                r.run(st, f)
                if f < 2:
                    continue
                m = masks[f]
                img = (r.readback(abi.BUF_DIRECT_RESULT0 + (f & 1)).view(np.float32).reshape(-1, 4)[:, :3].astype(np.float64)
                       + r.readback(abi.BUF_INDIRECT_RESULT0 + (f & 1)).view(np.float32).reshape(-1, 4)[:, :3]) @ LUM
                errs.append(float(np.abs(img[m] - refs[f][m]).mean() / refs[f][m].mean()))
                num = r.readback(abi.BUF_DIRECT_RESV0 + (f & 1)).view(np.uint32).reshape(-1, 9)[:, 7]
                hist.append(float((num[m] > st.RISSampleNum).mean()))
            out.setdefault(mode, []).append((float(np.mean(errs)), float(np.mean(hist))))
        r.destroy()
    for mode in MODES:
        e, h = np.array(out[mode]).T
        emit({"what": "quality", "mode": int(mode), "seeds": a.seeds, "mean_relative_error_by_seed": [round(x, 4) for x in e], "mean": round(float(e.mean()), 4),
              "range": [round(float(e.min()), 4), round(float(e.max()), 4)], "share_with_history_by_seed": [round(x, 4) for x in h],
              "share_with_history_mean": round(float(h.mean()), 4)})


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--footprint", default="real", choices=["real", "lite"])
    ap.add_argument("--steps", type=int, default=24)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--spp", type=int, default=2048)
    ap.add_argument("--seeds", type=int, default=4)
    ap.add_argument("--skip-cost", action="store_true")
    ap.add_argument("--skip-quality", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = []

    def emit(row):
        lines.append(json.dumps(row))
        print(lines[-1], flush=True)
        if a.out:
            with open(a.out, "w") as fh:
                fh.write("\n".join(lines) + "\n")
    if not a.skip_quality:
        quality(a, emit)
    if not a.skip_cost:
        cost(a, emit)


if __name__ == "__main__":
    main()
