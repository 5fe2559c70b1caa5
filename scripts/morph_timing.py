"""What morphing a mesh on the device costs and buys (rt_set_morph_targets / rt_update_morphs) on bench.py's headline workload (config 4, 1080p).

Two meshes: (a) the single-instance prim mesh closest to 1e5 triangles, (b) the most-instanced prim mesh.  Emissive meshes are left out.  Per mesh, sets of 8 and
of 64 targets (position planes; one extra row with the normal and tangent planes as well), each with all targets active and with 4 active.  Per case, in one run:
  - rt_update_morphs: HIP-event time and host wall time of the steady-state call (the second and later calls), rt_morph_stats::morphMs, the bytes over the bus
    (rt_deform_stats::vertexBytesCopied) and the delta bytes the kernel streams (planes x 16 B x active targets x vertices);
  - the route it replaces, measured in the same run on a second context: a numpy fp32 blend of the positions of the active targets on the host (normals and
    tangents left out, so this side is a lower bound) + rt_update_vertices of the mesh (host wall; 32 B per vertex over the bus).

  python scripts/morph_timing.py [--footprint real|lite] [--calls 5] [--out profiles/morph_timing.txt] [--bench-ab FILE]
One JSON line per measurement on stdout; the table made of them is written to --out.  --bench-ab FILE: lines "parent {bench.py's JSON line}" / "this {...}" of
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
from restir_amd.renderer import Renderer  # noqa: E402
from refit_timing import W, H, instances  # noqa: E402
from skin_timing import PRIM_DT  # noqa: E402


def write_profile(path, a, rows, bench):
    out = ["rt_update_morphs on bench.py's headline workload (config 4, %s footprint, %dx%d), one run of scripts/morph_timing.py --calls %d." % (a.footprint, W, H, a.calls),
           "`host route` = numpy fp32 blend of the active targets' positions + rt_update_vertices on a second context: what a host does without the call.",
           "Times are medians over the steady-state calls, ms.", "", "scene: " + json.dumps(rows[0]), ""]
    for r in rows[1:]:
        if r["what"] == "mesh":
            out += ["%s: prim mesh %d, %d vertices, %d triangles, %d instance(s)" % (r["name"], r["mesh"], r["vertices"], r["triangles"], r["instances"]),
                    "  targets active planes | rt_update_morphs: event   wall  morphMs  bus bytes  delta MB streamed  GB/s of morphMs | host route: blend  update_vertices   wall  bus bytes | host / device wall"]
        elif r["what"] == "case":
            out += ["  %7d %6d %6d | %24.4f %6.4f %8.4f %10d %18.2f %16.1f | %17.4f %16.4f %6.4f %10d | %8.1f x" % (
                r["targets"], r["active"], r["planes"], r["event_ms"], r["wall_ms"], r["morph_ms"], r["bus_bytes"], r["delta_mb"], r["gbps"],
                r["host_blend_ms"], r["host_update_ms"], r["host_wall_ms"], r["host_bus_bytes"], r["ratio"])]
    out.append("")
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
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "morph_timing.txt"))
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
    desc = sc.desc(env)
    inst = instances(desc)
    pm = np.frombuffer((C.c_char * (desc.numPrimMeshes * 20)).from_address(desc.primMeshes), dtype=PRIM_DT).copy()
    verts = np.frombuffer((C.c_char * (desc.numVertices * 32)).from_address(desc.vertices), dtype=abi.VERTEX_DT).copy()
    mats = np.frombuffer((C.c_char * (desc.numMaterials * 80)).from_address(desc.materials), dtype=np.float32).reshape(-1, 20)
    lum = 0.2126 * mats[:, 9] + 0.7152 * mats[:, 10] + 0.0722 * mats[:, 11]
    usable = (lum[np.maximum(pm["materialIndex"], 0)] <= 1e-2) & (pm["vertexCount"] > 0)
    uses = np.bincount(inst["primMesh"], minlength=len(pm))
    tris = pm["indexCount"] // 3
    meshes = {
        "(a) the single-instance prim mesh closest to 1e5 triangles": int(np.argmin(np.where(usable & (uses == 1), np.abs(tris.astype(np.int64) - 100000), 1 << 60))),
        "(b) the most-instanced prim mesh": int(np.argmax(np.where(usable, uses, -1))),
    }
    r = Renderer().setup(0)
    r.load_scene(desc)
    r.update(W, H)
    base = Renderer().setup(0)      # the host route's context
    base.load_scene(desc)
    emit({"what": "scene", "footprint": a.footprint, "instances": len(inst), "prim_meshes": len(pm), "vertices": int(desc.numVertices), **r.accel_stats()})
    rng = np.random.default_rng(3)
    for name, m in meshes.items():
        first, V = int(pm["vertexOffset"][m]), int(pm["vertexCount"][m])
        rest = verts[first:first + V]
        size = float(np.linalg.norm(rest["position"].max(axis=0) - rest["position"].min(axis=0)))
        emit({"what": "mesh", "name": name, "mesh": m, "vertices": V, "triangles": int(tris[m]), "instances": int(uses[m])})
        for targets, planes in ((8, 0), (64, 0), (8, 3)):
            P = 1 + (planes & 1) + (planes >> 1)
            d = np.zeros(targets * P * V, abi.MORPH_DELTA_DT)
            d["d"] = rng.uniform(-0.01 * size, 0.01 * size, (d.size, 3)).astype(np.float32)
            dpos = d["d"].reshape(targets, P, V, 3)[:, 0]
            r.set_morph_targets(np.array([(m, targets, 0, planes)], abi.MORPH_SET_DT), d)
            for active in (targets, 4):
                def weights(k):
                    w = np.zeros(targets, np.float32)
                    w[np.linspace(0, targets - 1, active).astype(np.int64)] = 0.1 + 0.05 * k
                    return w
                r.update_morphs([0], weights(0))      # the first call also derives the update's maps
                ev, wall, mms = [], [], []
                for k in range(a.calls):
                    w = weights(k + 1)
                    r.sync()
                    t0 = time.perf_counter()
                    r.update_morphs([0], w)
                    wall.append((time.perf_counter() - t0) * 1e3)
                    ms = r.morph_stats()
                    ev.append(ms.ms); mms.append(ms.morphMs)
                assert r.morph_stats().targetsApplied == active
                bus = r.deform_stats().vertexBytesCopied
                # the route it replaces: blend on the host, push the rows
                hb, hu, hw = [], [], []
                base.update_vertices(m, 0, rest)
                for k in range(a.calls):
                    w = weights(k + 1)
                    base.sync()
                    t0 = time.perf_counter()
                    posed = rest.copy()
                    p = posed["position"]
                    for t in np.nonzero(w)[0]:
                        p += w[t] * dpos[t]
                    t1 = time.perf_counter()
                    base.update_vertices(m, 0, posed)
                    t2 = time.perf_counter()
                    hb.append((t1 - t0) * 1e3); hu.append((t2 - t1) * 1e3); hw.append((t2 - t0) * 1e3)
                hbus = base.deform_stats().vertexBytesCopied
                med = lambda x: float(np.median(x))      # noqa: E731
                delta_bytes = P * 16 * active * V
                emit({"what": "case", "targets": targets, "active": active, "planes": planes, "event_ms": round(med(ev), 4), "wall_ms": round(med(wall), 4),
                      "morph_ms": round(med(mms), 4), "bus_bytes": int(bus), "delta_mb": round(delta_bytes / 1e6, 2),
                      "gbps": round((delta_bytes + 64 * V) / 1e9 / max(med(mms) * 1e-3, 1e-9), 1),
                      "host_blend_ms": round(med(hb), 4), "host_update_ms": round(med(hu), 4), "host_wall_ms": round(med(hw), 4), "host_bus_bytes": int(hbus),
                      "ratio": round(med(hw) / med(wall), 1)})
                base.update_vertices(m, 0, rest)
            r.update_morphs([0], np.zeros(targets, np.float32))      # back to the rest pose before the sets are replaced
    r.destroy(); base.destroy()
    bench = [l.strip() for l in open(a.bench_ab)] if a.bench_ab else []
    write_profile(a.out, a, rows, [l for l in bench if l])


if __name__ == "__main__":
    main()
