"""What deforming a mesh on the device costs and buys (rt_set_skins / rt_update_skins) on bench.py's headline workload (config 4, 1080p).

Three configurations, each skinned with four joints by height and bent: (a) the most-instanced prim mesh, (b) the single-instance prim mesh closest to 1e5
triangles, (c) 1 % of the prim meshes.  Emissive meshes are left out (rt_set_skins refuses them).  Per configuration, in one run:
  - rt_update_skins: HIP-event time and host wall time of the steady-state call (the second and later calls; the first one also derives the update's maps),
    rt_deform_stats::skinMs, the leaf records and nodes refitted;
  - the route without the call, measured in the same run: linear-blend skinning of the positions on the host (numpy, fp32; normals and tangents left out, so this
    side is a lower bound) + rt_upload_scene + rt_build_accel on a second context (host wall);
  - ms per frame on the refitted tree after the bend, against rt_rebuild_accel and against a fresh rt_build_accel of the same deformed scene.

  python scripts/skin_timing.py [--footprint real|lite] [--steps 24] [--warmup 8] [--out profiles/skin_timing.txt] [--bench-ab FILE]
One JSON line per measurement on stdout; the tables made of them are written to --out.  --bench-ab FILE: lines "parent {bench.py's JSON line}" / "this {...}" of
bench.py --gpus 1 --steps 100 --warmup 20 run on the parent commit's library and on this one, alternated in the same visit (RESTIR_HIP_LIB selects the library)."""
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
from restir_amd.renderer import Renderer, hip_lib  # noqa: E402
from refit_timing import W, H, instances, frame_ms  # noqa: E402

JOINTS = 4
PRIM_DT = np.dtype([("vertexOffset", "<u4"), ("vertexCount", "<u4"), ("firstIndex", "<u4"), ("indexCount", "<u4"), ("materialIndex", "<i4")])


def rot_z(a):
    c, s = np.cos(a), np.sin(a)
    return np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]])


def affine(R, t, about):
    M = np.zeros((3, 4))
    M[:, :3] = R
    M[:, 3] = about + t - R @ about
    return M.reshape(12).astype(np.float32)


class Skin:
    """one skinned prim mesh: influences by height (each vertex blends the two joints around it), and a bend of amount s"""

    def __init__(self, verts, pm, mesh):
        self.mesh, self.first, self.count = mesh, int(pm["vertexOffset"][mesh]), int(pm["vertexCount"][mesh])
        p = verts["position"][self.first:self.first + self.count].astype(np.float64)
        lo, hi = p.min(axis=0), p.max(axis=0)
        self.centre, self.size = 0.5 * (lo + hi), float(np.linalg.norm(hi - lo))
        u = (p[:, 1] - lo[1]) / max(hi[1] - lo[1], 1e-9) * (JOINTS - 1)
        j0 = np.minimum(np.floor(u).astype(np.int64), JOINTS - 1)
        self.inf = np.zeros(self.count, abi.SKIN_INFLUENCE_DT)
        self.inf["joint"][:, 0], self.inf["joint"][:, 1] = j0, np.minimum(j0 + 1, JOINTS - 1)
        f = (u - j0).astype(np.float32)
        self.inf["weight"][:, 0], self.inf["weight"][:, 1] = np.float32(1) - f, f

    def matrices(self, s):
        return np.stack([affine(rot_z(0.15 * s * k / (JOINTS - 1)), np.array([0.01 * s * self.size * k / (JOINTS - 1), 0, 0]), self.centre) for k in range(JOINTS)])

    def host_pose(self, verts, mats):
        """the positions on the host, fp32, the blend order of the header"""
        M = mats.reshape(JOINTS, 12)
        w, j = self.inf["weight"], self.inf["joint"]
        B = w[:, 0:1] * M[j[:, 0]]
        B = B + w[:, 1:2] * M[j[:, 1]]
        p = verts["position"][self.first:self.first + self.count]
        out = np.empty_like(p)
        for r in range(3):
            out[:, r] = ((B[:, 4 * r] * p[:, 0] + B[:, 4 * r + 1] * p[:, 1]) + B[:, 4 * r + 2] * p[:, 2]) + B[:, 4 * r + 3]
        return out


def write_profile(path, a, rows, bench):
    out = ["rt_update_skins on bench.py's headline workload (config 4, %s footprint, %dx%d), one run of scripts/skin_timing.py --steps %d --warmup %d." % (a.footprint, W, H, a.steps, a.warmup),
           "Skins of %d joints by height, bent.  `host route` = numpy skinning of the positions + rt_upload_scene + rt_build_accel on a second context: what a host" % JOINTS,
           "needs without the call.", "", "scene: " + json.dumps(rows[0]), ""]
    for r in rows[1:]:
        if r["what"] == "config":
            out += ["%s: %d prim mesh(es), %d vertices, %d triangles in %d instance(s)" % (r["name"], r["meshes"], r["vertices"], r["instanced_triangles"], r["instances"])]
        elif r["what"] == "update":
            out += ["  rt_update_skins, steady state (%d calls): event ms %s; host wall ms %s; skinMs %s" % (len(r["event_ms"]), r["event_ms"], r["wall_ms"], r["skin_ms"]),
                    "    first call (derives the update's maps): wall %.3f ms.  leaf records refitted %d, nodes %d of %d, full refit %d, vertexBytesCopied %d" % (
                        r["first_wall_ms"], r["leaf_records"], r["nodes"], r["tree_nodes"], r["full_refit"], r["vertex_bytes_copied"])]
        elif r["what"] == "host route":
            out += ["  host route: skinning %.3f ms + rt_upload_scene + rt_build_accel %.1f ms = %.1f ms wall; / rt_update_skins wall = %.0f x" % (
                r["host_skin_ms"], r["upload_build_ms"], r["host_skin_ms"] + r["upload_build_ms"], r["over_update_wall"])]
        elif r["what"] == "frame":
            out += ["  ms per frame (frames in flight, host-timed): before %.3f; refitted after the bend %.3f; rt_rebuild_accel %.3f; fresh rt_build_accel %.3f;  refitted / fresh = %.3f x" % (
                r["before"], r["refitted"], r["device_rebuilt"], r["host_built"], r["refitted"] / r["host_built"]), ""]
    if bench:
        out += ["Default path: bench.py --gpus 1 --steps 100 --warmup 20, the parent commit's library and this one alternated in one visit."]
        ms = {"parent": [], "this": []}
        for line in bench:
            who, js = line.split(None, 1)
            d = json.loads(js)
            ms[who].append(d["ms_per_step"])
            out.append("  %-6s  ms_per_step %.4f   %.2f %s" % (who, d["ms_per_step"], d["value"], d["unit"]))
        if len(ms["parent"]) > 1 and ms["this"]:
            mp, mt = sum(ms["parent"]) / len(ms["parent"]), sum(ms["this"]) / len(ms["this"])
            out.append("  mean parent %.4f ms, this %.4f ms: %+.2f %%; the parent's own runs differ by %.2f %%.  The default path never calls the new code." % (
                mp, mt, (mt / mp - 1) * 100, (max(ms["parent"]) / min(ms["parent"]) - 1) * 100))
    with open(path, "w") as f:
        f.write("\n".join(out) + "\n")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--footprint", default="real", choices=["real", "lite"])
    ap.add_argument("--steps", type=int, default=24)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "skin_timing.txt"))
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
    inst = instances(desc)
    pm = np.frombuffer((C.c_char * (desc.numPrimMeshes * 20)).from_address(desc.primMeshes), dtype=PRIM_DT).copy()
    verts = np.frombuffer((C.c_char * (desc.numVertices * 32)).from_address(desc.vertices), dtype=abi.VERTEX_DT).copy()
    mats = np.frombuffer((C.c_char * (desc.numMaterials * 80)).from_address(desc.materials), dtype=np.float32).reshape(-1, 20)
    lum = 0.2126 * mats[:, 9] + 0.7152 * mats[:, 10] + 0.0722 * mats[:, 11]
    usable = (lum[np.maximum(pm["materialIndex"], 0)] <= 1e-2) & (pm["vertexCount"] > 0)
    uses = np.bincount(inst["primMesh"], minlength=len(pm))
    tris = pm["indexCount"] // 3
    rng = np.random.default_rng(5)
    configs = {
        "(a) the most-instanced prim mesh": [int(np.argmax(np.where(usable, uses, -1)))],
        "(b) one single-instance prim mesh of about 1e5 triangles": [int(np.argmin(np.where(usable & (uses == 1), np.abs(tris.astype(np.int64) - 100000), 1 << 60)))],
        "(c) 1 % of the prim meshes": sorted(int(m) for m in rng.choice(np.nonzero(usable & (uses > 0))[0], max(1, len(pm) // 100), replace=False)),
    }
    r = Renderer().setup(0)
    r.load_scene(desc)
    r.update(W, H)
    base = Renderer().setup(0)      # the host route's context
    emit({"what": "scene", "footprint": a.footprint, "instances": len(inst), "prim_meshes": len(pm), "vertices": int(desc.numVertices), **r.accel_stats()})
    f = 0
    for name, meshes in configs.items():
        r.load_scene(desc)          # every configuration starts from the host-built tree of the rest pose
        skins = [Skin(verts, pm, m) for m in meshes]
        emit({"what": "config", "name": name, "meshes": len(meshes), "vertices": sum(s.count for s in skins), "instances": int(uses[meshes].sum()),
              "instanced_triangles": int((tris[meshes] * uses[meshes]).sum())})
        before, f = frame_ms(r, sc, st, a, f)
        tab = np.zeros(len(skins), abi.SKIN_DT)
        first = 0
        for k, s in enumerate(skins):
            tab[k] = (s.mesh, 0, JOINTS, first)
            first += s.count
        r.set_skins(tab, np.concatenate([s.inf for s in skins]))
        ids = np.arange(len(skins), dtype=np.uint32)
        t0 = time.perf_counter()
        r.update_skins(ids, np.concatenate([s.matrices(0.2) for s in skins]))
        first_wall = (time.perf_counter() - t0) * 1e3
        ev, wall, skin_ms = [], [], []
        for k in range(a.calls):
            m = np.concatenate([s.matrices(0.4 + 0.6 * (k + 1) / a.calls) for s in skins])
            r.sync()
            t0 = time.perf_counter()
            r.update_skins(ids, m)
            wall.append(round((time.perf_counter() - t0) * 1e3, 4))
            ev.append(round(r.deform_stats().ms, 4)); skin_ms.append(round(r.deform_stats().skinMs, 4))
        rs, ds = r.refit_stats(), r.deform_stats()
        emit({"what": "update", "event_ms": ev, "wall_ms": wall, "skin_ms": skin_ms, "first_wall_ms": round(first_wall, 3), "leaf_records": rs.leafRecords, "nodes": rs.nodes,
              "tree_nodes": r.accel_stats()["nodes"], "full_refit": rs.fullRefit, "vertex_bytes_copied": ds.vertexBytesCopied})
        # the host route for the same pose
        t0 = time.perf_counter()
        v2 = verts.copy()
        for s in skins:
            v2["position"][s.first:s.first + s.count] = s.host_pose(verts, s.matrices(1.0))      # (the last pose of the loop above)
        host_skin = (time.perf_counter() - t0) * 1e3
        d2 = abi.SceneDesc.from_buffer_copy(desc)
        d2.vertices = v2.ctypes.data
        t0 = time.perf_counter()
        base.load_scene(d2)
        up = (time.perf_counter() - t0) * 1e3
        emit({"what": "host route", "host_skin_ms": round(host_skin, 3), "upload_build_ms": round(up, 1), "over_update_wall": round((host_skin + up) / float(np.median(wall)), 1)})
        refitted, f = frame_ms(r, sc, st, a, f)
        r.rebuild_accel()
        rebuilt, f = frame_ms(r, sc, st, a, f)
        assert hip_lib().rt_build_accel(r._h) == 0
        built, f = frame_ms(r, sc, st, a, f)
        emit({"what": "frame", "before": round(before, 4), "refitted": round(refitted, 4), "device_rebuilt": round(rebuilt, 4), "host_built": round(built, 4)})
    r.destroy(); base.destroy()
    bench = [l.strip() for l in open(a.bench_ab)] if a.bench_ab else []
    write_profile(a.out, a, rows, [l for l in bench if l])


if __name__ == "__main__":
    main()
