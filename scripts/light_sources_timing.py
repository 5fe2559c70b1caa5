"""What keeping the triangle-light records on the device costs and saves (rt_set_light_sources) on config 5 (the interior scene, about 2 k emissive
triangles) and on bench.py's headline workload (config 4).

Per scene, in one run:
  - rt_update_instances on the emissive instance with the most light records, without a binding (the light records stay behind) and with one: HIP-event time of
    the call, rt_light_stats::ms of the light kernel, host wall time;
  - the route without the binding, measured in the same run: Scene::updateInstances (every record and the alias table recomputed on the host) +
    rt_update_instances + rt_update_lights (host wall);
  - rt_update_skins on the emissive prim mesh with the most vertices with the binding on, against host skinning of the positions (numpy, fp32) +
    Scene::updateVertices + rt_update_vertices + rt_update_lights;
  - after every bound call the device records are compared with the records the Scene recomputed (the line says `records_equal_scene`).
--mode default-update: rt_update_instances of one emissive instance with NO binding, event and wall ms per call, for the library RESTIR_HIP_LIB selects: run on
the parent commit's library and on this one, alternated, the lines collected with a "parent " / "this " prefix in the file --ab names.

  python scripts/light_sources_timing.py [--footprint real|lite] [--calls 5] [--out profiles/light_sources_timing.txt] [--ab FILE] [--mode all|default-update]
One JSON line per measurement on stdout; the tables made of them are written to --out.  --ab FILE also takes bench.py's JSON lines with the same prefixes
(bench.py --gpus 1 --steps 100 --warmup 20 on both libraries, alternated in the same visit)."""
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
from refit_timing import instances, moved  # noqa: E402
from skin_timing import Skin, PRIM_DT  # noqa: E402


def records(desc):
    n = desc.lightInfo.trigLightSize if desc.trigLights else 0
    return np.frombuffer((C.c_char * (n * 96)).from_address(desc.trigLights), dtype=abi.TRIG_LIGHT_DT).copy()


def load(name, footprint):
    kind = {"config 5": abi.PROC_BISTRO_INT, "headline": abi.PROC_BISTRO_EXT_REAL if footprint == "real" else abi.PROC_BISTRO_EXT}[name]
    sc = host.Scene().makeProcedural(kind, 1.0, 1)
    return sc, sc.desc()


def nudge(home_row, k):
    return moved(home_row[None, :], np.array([[0.01 * (k + 1), 0.0, 0.005 * (k + 1)]], np.float32))


def timed(fn):
    t0 = time.perf_counter()
    fn()
    return round((time.perf_counter() - t0) * 1e3, 4)


def default_update(a, emit):
    """rt_update_instances with no binding: what the default path costs on the library in use"""
    sc, desc = load("headline", a.footprint)
    src = sc.lightSources()
    inst = int(np.bincount(src["instance"]).argmax())
    home = instances(desc)["objectToWorld"]
    r = Renderer().setup(0)
    r.load_scene(desc)
    r.update_instances([], np.zeros((0, 12), np.float32))      # derives the update's maps
    ev, wall = [], []
    for k in range(a.calls + 1):
        xf = nudge(home[inst], k)
        r.sync()
        w = timed(lambda: r.update_instances([inst], xf))
        if k:      # (the first call warms the path)
            ev.append(round(r.refit_stats().ms, 4)); wall.append(w)
    emit({"what": "default update", "event_ms": ev, "wall_ms": wall})
    r.destroy()


def scene_rows(name, a, emit):
    sc, desc = load(name, a.footprint)
    src = sc.lightSources()
    n = src.size
    inst_tab = instances(desc)
    home = inst_tab["objectToWorld"]
    per_inst = np.bincount(src["instance"], minlength=len(home))
    inst = int(per_inst.argmax())
    pm = np.frombuffer((C.c_char * (desc.numPrimMeshes * 20)).from_address(desc.primMeshes), dtype=PRIM_DT).copy()
    r = Renderer().setup(0)
    r.load_scene(desc)
    emit({"what": "scene", "name": name, "instances": len(home), "prim_meshes": len(pm), "light_records": int(n), "emissive_instances": int((per_inst > 0).sum()),
          "moved_instance_records": int(per_inst[inst]), **r.accel_stats()})
    r.update_instances([], np.zeros((0, 12), np.float32))      # derives the update's maps
    # ---- the moved emitter without a binding, then the host route, then with the binding
    ev, wall = [], []
    for k in range(a.calls):
        xf = nudge(home[inst], k)
        r.sync()
        wall.append(timed(lambda: r.update_instances([inst], xf)))
        ev.append(round(r.refit_stats().ms, 4))
    emit({"what": "update_instances, no binding (the lights stay behind)", "event_ms": ev, "wall_ms": wall})
    host_ms, wall = [], []
    for k in range(a.calls):
        xf = nudge(home[inst], a.calls + k)
        r.sync()
        t0 = time.perf_counter()
        sc.updateInstances([inst], xf)
        d = sc.desc()
        t1 = time.perf_counter()
        r.update_instances([inst], xf)
        r.update_lights(d)
        t2 = time.perf_counter()
        host_ms.append(round((t1 - t0) * 1e3, 4)); wall.append(round((t2 - t0) * 1e3, 4))
    emit({"what": "host route: Scene::updateInstances + rt_update_instances + rt_update_lights", "scene_ms": host_ms, "wall_ms": wall, "light_bytes_copied": r.light_stats().lightBytesCopied})
    bind_ms = timed(lambda: r.set_light_sources(src))
    ev, wall, lms, same = [], [], [], True
    for k in range(a.calls):
        xf = nudge(home[inst], 2 * a.calls + k)
        r.sync()
        wall.append(timed(lambda: r.update_instances([inst], xf)))
        ev.append(round(r.refit_stats().ms, 4)); lms.append(round(r.light_stats().ms, 4))
        sc.updateInstances([inst], xf)
        same = same and np.array_equal(r.lights_readback(abi.LIGHTS_TRIG, n).view(np.uint8), records(sc.desc()).view(np.uint8))
    s = r.light_stats()
    emit({"what": "update_instances, binding on", "bind_wall_ms": bind_ms, "event_ms": ev, "light_kernel_ms": lms, "wall_ms": wall, "rewritten": s.rewritten,
          "light_bytes_copied": s.lightBytesCopied, "records_equal_scene": bool(same)})
    # ---- the skinned emitter: the emissive prim mesh with the most vertices
    meshes = np.unique(inst_tab["primMesh"][per_inst > 0])
    mesh = int(meshes[np.argmax(pm["vertexCount"][meshes])])
    verts = np.frombuffer((C.c_char * (desc.numVertices * 32)).from_address(desc.vertices), dtype=abi.VERTEX_DT).copy()
    sk = Skin(verts, pm, mesh)
    on_mesh = int(per_inst[inst_tab["primMesh"] == mesh].sum())
    host_ms, wall = [], []
    for k in range(a.calls):
        mats = sk.matrices(0.2 + 0.1 * k)
        r.sync()
        t0 = time.perf_counter()
        rows = verts[sk.first:sk.first + sk.count].copy()
        rows["position"] = sk.host_pose(verts, mats)
        sc.updateVertices(mesh, 0, rows)
        d = sc.desc()
        t1 = time.perf_counter()
        r.update_vertices(mesh, 0, rows)
        r.update_lights(d)
        t2 = time.perf_counter()
        host_ms.append(round((t1 - t0) * 1e3, 4)); wall.append(round((t2 - t0) * 1e3, 4))
    emit({"what": "host route: host skinning + Scene::updateVertices + rt_update_vertices + rt_update_lights", "mesh_vertices": sk.count, "records_on_mesh": on_mesh,
          "host_ms": host_ms, "wall_ms": wall})
    rest = verts[sk.first:sk.first + sk.count]
    sc.updateVertices(mesh, 0, rest)
    r.update_vertices(mesh, 0, rest)      # back to the rest pose: the skin captures it (the bound records follow on the device)
    tab = np.zeros(1, abi.SKIN_DT)
    tab[0] = (mesh, 0, 4, 0)
    r.set_skins(tab, sk.inf)
    ev, wall, lms, skin_ms = [], [], [], []
    for k in range(a.calls + 1):
        mats = sk.matrices(0.2 + 0.1 * k)
        r.sync()
        w = timed(lambda: r.update_skins([0], mats))
        if k:
            wall.append(w); ev.append(round(r.deform_stats().ms, 4)); skin_ms.append(round(r.deform_stats().skinMs, 4)); lms.append(round(r.light_stats().ms, 4))
    s = r.light_stats()
    emit({"what": "update_skins on the emissive mesh, binding on", "event_ms": ev, "skin_ms": skin_ms, "light_kernel_ms": lms, "wall_ms": wall, "rewritten": s.rewritten,
          "light_bytes_copied": s.lightBytesCopied, "vertex_bytes_copied": r.deform_stats().vertexBytesCopied})
    r.destroy()


def write_profile(path, a, rows, ab):
    out = ["rt_set_light_sources: one run of scripts/light_sources_timing.py --calls %d (headline scene: %s footprint).  Times in ms; event = HIP events on the main" % (a.calls, a.footprint),
           "stream, wall = host wall time of the call(s) including the drain.", ""]
    for r in rows:
        if r["what"] == "scene":
            out += ["", "%s: %s" % (r["name"], json.dumps({k: v for k, v in r.items() if k not in ("what", "name")}))]
        else:
            out += ["  %s" % r["what"]] + ["    %s: %s" % (k, v) for k, v in r.items() if k != "what"]
    if ab:
        out += ["", "Unchanged default: the parent commit's library and this one, alternated in one visit."]
        upd = {"parent": [], "this": []}
        ms = {"parent": [], "this": []}
        for line in ab:
            who, js = line.split(None, 1)
            d = json.loads(js)
            if d.get("what") == "default update":
                upd[who].append(float(np.median(d["event_ms"])))
                out.append("  %-6s  rt_update_instances, no binding: event ms %s; wall ms %s" % (who, d["event_ms"], d["wall_ms"]))
            elif "ms_per_step" in d:
                ms[who].append(d["ms_per_step"])
                out.append("  %-6s  bench.py --gpus 1 --steps 100 --warmup 20: ms_per_step %.4f   %.2f %s" % (who, d["ms_per_step"], d["value"], d["unit"]))
        for label, t in (("rt_update_instances event ms (median per run)", upd), ("bench.py ms_per_step", ms)):
            if len(t["parent"]) > 1 and t["this"]:
                mp, mt = sum(t["parent"]) / len(t["parent"]), sum(t["this"]) / len(t["this"])
                out.append("  %s: mean parent %.4f, this %.4f: %+.2f %%; the parent's own runs differ by %.2f %%." % (
                    label, mp, mt, (mt / mp - 1) * 100, (max(t["parent"]) / min(t["parent"]) - 1) * 100))
    with open(path, "w") as f:
        f.write("\n".join(out) + "\n")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--footprint", default="real", choices=["real", "lite"])
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--mode", default="all", choices=["all", "default-update"])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "light_sources_timing.txt"))
    ap.add_argument("--ab", default=None)
    a = ap.parse_args()
    rows = []

    def emit(row):
        rows.append(row)
        print(json.dumps(row), flush=True)
    if a.mode == "default-update":
        default_update(a, emit)
        return
    for name in ("config 5", "headline"):
        scene_rows(name, a, emit)
    ab = [l.strip() for l in open(a.ab)] if a.ab else []
    write_profile(a.out, a, rows, [l for l in ab if l.startswith(("parent ", "this "))])


if __name__ == "__main__":
    main()
