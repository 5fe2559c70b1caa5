"""ctypes driver of tests/instances_checker.cpp (the CPU restatement of rt_set_instances: the verdict on a table, the expansion into the device builder's input)
and the instance tables the CPU and the GPU tests share.  The checker is compiled once per process together with csrc/bvh8_builder.cpp (g++, no GPU)."""
import ctypes as C
import os
import subprocess
import numpy as np

from helpers import ROOT, abi
import accel_build
import refit

SRC = os.path.join(ROOT, "tests", "instances_checker.cpp")
_lib = None
DT = refit.INSTANCE_DT
FORCE_OPAQUE, CULL_DISABLE = 1, 2
TRI_OPAQUE, TRI_NOCULL, TRI_FLIP = 1, 2, 4
FLIP_BIT = 0x80000000
# isc_verdict's codes, and the words rt_last_error uses for the same refusal
(OK, NULL, NO_INSTANCES, PRIM_MESH, NON_FINITE, SINGULAR, NO_INVERSE, TOO_MANY, NO_TRIANGLES, EMITTER_CHANGED, EMITTER_ADDED) = range(11)
MESSAGE = {NULL: "NULL instance table", NO_INSTANCES: "at least one instance", PRIM_MESH: "prim mesh out of range", NON_FINITE: "non-finite matrix entry",
           SINGULAR: "singular matrix", NO_INVERSE: "no finite inverse", TOO_MANY: "more than 2^31 - 1 triangles", NO_TRIANGLES: "no triangles",
           EMITTER_CHANGED: "must stay in place", EMITTER_ADDED: "new instance of an emissive prim mesh"}
PER_INSTANCE = (PRIM_MESH, NON_FINITE, SINGULAR, NO_INVERSE, TOO_MANY, EMITTER_CHANGED, EMITTER_ADDED)     # rt_last_error names the instance


def build(out_dir):
    global _lib
    if _lib is not None:
        return _lib
    so = os.path.join(str(out_dir), "libinstanceschk.so")
    subprocess.check_call([os.environ.get("CXX", "g++")] + refit.FLAGS + [SRC, refit.BUILDER, "-o", so])
    L = C.CDLL(so)
    L.isc_verdict.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]
    L.isc_mesh_alpha_base.argtypes = [C.c_void_p, C.c_void_p]
    L.isc_expand.restype = C.c_uint32
    L.isc_expand.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.isc_flatten.restype = C.c_int64
    L.isc_flatten.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    _lib = L
    return L


def rows(table):
    return np.ascontiguousarray(table, dtype=DT).reshape(-1)


def desc_with(desc, table):
    """a copy of a scene description with another instance table (everything else, the light records included, as it was: valid under the emitter rule)"""
    t = rows(table)
    d = abi.SceneDesc.from_buffer_copy(desc)
    d.numInstances, d.instances = len(t), t.ctypes.data
    d._keep = (t, desc)
    return d


def verdict(L, desc, table, count=None, bound=()):
    """(code, offender) of isc_verdict for `table` as the new table of `desc`; table None: the NULL pointer; bound: the instances a light-source binding names"""
    off = C.c_uint32(0)
    mask = np.zeros(max(desc.numInstances, 1), np.uint8)
    mask[list(bound)] = 1
    bp = mask.ctypes.data if len(bound) else None
    if table is None:
        return L.isc_verdict(C.addressof(desc), bp, 1 if count is None else count, None, C.byref(off)), off.value
    t = rows(table)
    keep = t if len(t) else np.zeros(1, DT)      # (an empty table still has an address)
    return L.isc_verdict(C.addressof(desc), bp, len(t) if count is None else count, keep.ctypes.data, C.byref(off)), off.value


def mesh_alpha_base(L, desc):
    out = np.zeros(desc.numPrimMeshes, np.uint32)
    L.isc_mesh_alpha_base(C.addressof(desc), out.ctypes.data)
    return out


def expand(L, desc, table):
    """(prefix words, triRef (n, 2), records (n, 3): globalId / flags / alphaIdx) of isc_expand"""
    t = rows(table)
    prefix = np.zeros(len(t) + 1, np.uint32)
    n = L.isc_expand(C.addressof(desc), len(t), t.ctypes.data, prefix.ctypes.data, None, None)
    ref, rec = np.zeros((n, 2), np.uint32), np.zeros((n, 3), np.uint32)
    assert L.isc_expand(C.addressof(desc), len(t), t.ctypes.data, prefix.ctypes.data, ref.ctypes.data, rec.ctypes.data) == n
    return prefix, ref, rec


def flatten(L, desc, threads=4):
    """(triRef (n, 2), flags (n,)) of buildBvh8's flatten step for a description"""
    n = L.isc_flatten(C.addressof(desc), threads, None, None)
    assert n >= 0
    ref, flags = np.zeros((n, 2), np.uint32), np.zeros(n, np.uint32)
    assert L.isc_flatten(C.addressof(desc), threads, ref.ctypes.data, flags.ctypes.data) == n
    return ref, flags


# ---- building tables ---------------------------------------------------------------------------------------------------------------------------------------
def placed(desc, i, kind, extent=1.0, shift=(0.0, 0.0, 0.0)):
    """a copy of instance i's row with its matrix moved by one of refit.move_matrix's classes, then shifted"""
    r = refit.instances_of(desc)[i:i + 1].copy()
    r["objectToWorld"][0] = refit.compose(refit.translation(shift), refit.move_matrix(kind, desc, i, extent))
    return r


def emitters_first(sc):
    """the scene with its emissive instances moved to the front of the table (Scene.setInstances): what a host does that wants to add and remove the others"""
    desc = sc.desc()
    inst = refit.instances_of(desc)
    em = [int(i) for i in refit.describe(desc)["emissive"]]
    order = em + [i for i in range(len(inst)) if i not in em]
    sc.setInstances(inst[order])
    return sc


class OneAndEmpty(accel_build.TinyScene):
    """tiny `one` with a second prim mesh that has no triangles"""

    def __init__(self):
        super().__init__(accel_build.tiny("one").vertices[:, :3].reshape(-1, 3, 3))
        self.prim = np.array([[0, 3, 0, 3, 0], [0, 3, 0, 0, 0]], np.uint32)
        self._desc.numPrimMeshes, self._desc.primMeshes = 2, self.prim.ctypes.data


TABLES = ("one", "same30", "cornell", "street", "street_lazy", "empty_mesh")


def tables(name):
    """(scene object with .desc(), [(label, new table)]): the successive tables of one case; the first is applied to the scene as built"""
    if name == "one":           # growth past one leaf slot and past one node; shrink; re-allocation
        sc = accel_build.tiny("one")
        r = refit.instances_of(sc.desc())

        def at(k):
            q = r.copy()
            q["objectToWorld"][0][3] = np.float32(0.4 * k)
            return q
        return sc, [("two", np.concatenate([at(0), at(1)])), ("row25", np.concatenate([at(k) for k in range(25)])), ("back to one", at(0)),
                    ("twenty, inside the capacity", np.concatenate([at(k) for k in range(20)]))]
    if name == "same30":        # equal Morton keys across instances: the order is the new globalIds'
        sc = accel_build.tiny("same30")
        r = refit.instances_of(sc.desc())
        return sc, [("three times the same", np.concatenate([r, r, r]))]
    if name == "empty_mesh":    # instances without triangles between the others: the search in the prefix words steps over them
        sc = OneAndEmpty()
        r = refit.instances_of(sc.desc())
        e = r.copy()
        e["primMesh"] = 1
        far = r.copy()
        far["objectToWorld"][0][3] = np.float32(0.7)
        return sc, [("empty first, between and last", np.concatenate([e, r, e, e, far, e]))]
    if name == "cornell":       # TRI_FLIP of new instances; index shift of the instances after a removal
        sc = emitters_first(refit.cornell())
        desc = sc.desc()
        base = refit.instances_of(desc)
        box = 4                 # the short box (instance 3 of the scene as generated)
        t1 = np.concatenate([base, placed(desc, box, "rotate", shift=(0.15, 0.0, -0.3)), placed(desc, box, "mirror", shift=(-0.7, 0.62, 0.1)),
                             placed(desc, box, "scale", shift=(-0.2, 1.0, -0.4))])
        return sc, [("three more boxes", t1), ("the original box removed", np.delete(t1, box))]
    if name in ("street", "street_lazy"):
        sc = emitters_first(refit.street())
        desc = sc.desc()
        base = refit.instances_of(desc)
        pm = base["primMesh"]
        leafs = [int(i) for i in np.nonzero((base["flags"] & FORCE_OPAQUE) == 0)[0]]       # the alpha-tested leaf cards: one instance per mesh
        trunk = int(np.nonzero(pm == pm[leafs[0] - 1])[0][0])                                 # the instanced tree mesh stands in front of its leaves
        assert len(leafs) == 2 and np.count_nonzero(pm == pm[trunk]) == 2
        if name == "street":    # templates of a mesh; opaque and non-opaque instances of one mesh side by side
            t1 = np.concatenate([base, placed(desc, trunk, "translate", 60.0, (3.0, 0.0, 2.0)), placed(desc, leafs[0], "translate", 60.0, (3.0, 0.0, 2.0))])
            t2 = np.delete(t1, 20)
            opaque = placed(desc, leafs[0], "translate", 60.0, (-2.0, 0.5, 4.0))
            opaque["flags"] |= FORCE_OPAQUE
            return sc, [("a tree and its leaves", t1), ("a prop removed", t2), ("opaque leaves beside them", np.concatenate([t2, opaque]))]
        prop = placed(desc, 25, "rotate", 60.0, (1.0, 0.0, 1.0))
        l0 = np.concatenate([base, prop])
        l1 = np.delete(l0, leafs[1])
        l2 = np.concatenate([l1, placed(desc, 30, "scale", 60.0, (0.0, 0.0, 2.0))])
        return sc, [("a prop", l0), ("the second leaf mesh's only instance removed", l1), ("another prop", l2), ("the leaves again", np.concatenate([l2, base[leafs[1]:leafs[1] + 1]]))]
    raise ValueError(name)


def added_ids(old, new):
    """indices of `new` whose row is not at the same index in `old`"""
    old, new = rows(old), rows(new)
    return [i for i in range(len(new)) if i >= len(old) or old[i].tobytes() != new[i].tobytes()]


# ---- refusals ----------------------------------------------------------------------------------------------------------------------------------------------
def refusals(name):
    """(scene, [(label, table or None, expected verdict, expected offender)]) — every refusal of rt_set_instances on a scene that can show it"""
    if name == "cornell":
        sc = refit.cornell()
        desc = sc.desc()
        base = refit.instances_of(desc)
        em = int(refit.describe(desc)["emissive"][0])      # 5: the last instance

        def edit(i, fn):
            t = base.copy()
            fn(t[i:i + 1])
            return t

        def setm(k, v):
            def f(r):
                r["objectToWorld"][0][k] = v
            return f

        def scale(f):
            def g(r):
                r["objectToWorld"][0][[0, 5, 10]] = np.float32(f)
            return g

        def mesh(m):
            def f(r):
                r["primMesh"] = m
            return f

        def flag(r):
            r["flags"] ^= CULL_DISABLE
        return sc, [("NULL table", None, NULL, 0), ("no instances", base[:0], NO_INSTANCES, 0), ("prim mesh out of range", edit(2, mesh(desc.numPrimMeshes)), PRIM_MESH, 2),
                    ("NaN", edit(3, setm(7, np.nan)), NON_FINITE, 3), ("infinity", edit(1, setm(0, np.inf)), NON_FINITE, 1),
                    ("two equal rows", edit(4, lambda r: r["objectToWorld"][0].__setitem__(slice(4, 7), r["objectToWorld"][0][0:3])), SINGULAR, 4),
                    ("determinant underflows to zero", edit(0, scale(1e-30)), SINGULAR, 0), ("inverse overflows", edit(0, scale(1e-13)), NO_INVERSE, 0),
                    ("emitter moved", edit(em, setm(3, 0.25)), EMITTER_CHANGED, em), ("emitter's flags changed", edit(em, flag), EMITTER_CHANGED, em),
                    ("emitter removed", base[:em], EMITTER_CHANGED, em), ("emitter shifted by a removal", np.delete(base, 3), EMITTER_CHANGED, em),
                    ("a second emitter", np.concatenate([base, base[em:em + 1]]), EMITTER_ADDED, len(base)),
                    ("an emitter in a box's place", edit(3, mesh(base["primMesh"][em])), EMITTER_ADDED, 3),
                    ("first offender of two", np.concatenate([edit(2, setm(1, np.nan))[:3], edit(4, mesh(99))[3:]]), NON_FINITE, 2)]
    if name == "street":        # 784 401 instances of the 2738-triangle ground: past 2^31 - 1 records
        sc = refit.street()
        base = refit.instances_of(sc.desc())
        tris = int(refit.prim_meshes_of(sc.desc())["indexCount"][base["primMesh"][0]]) // 3
        n = (2 ** 31 - 1) // tris + 1
        return sc, [("too many triangles", np.repeat(base[0:1], n), TOO_MANY, n - 1)]
    if name == "empty_mesh":
        sc = OneAndEmpty()
        e = refit.instances_of(sc.desc()).copy()
        e["primMesh"] = 1
        return sc, [("no triangles", np.concatenate([e, e]), NO_TRIANGLES, 0)]
    raise ValueError(name)


REFUSALS = ("cornell", "street", "empty_mesh")


# ---- rays ----------------------------------------------------------------------------------------------------------------------------------------------------
# (street: 12 of the seeds 1..29 gives the most hits on the added leaf cards, 38; tests/test_instances_cpu.py checks every count on the oracle's ray code)
RAYS, RAY_SEED = 4096, {"one": 11, "same30": 11, "cornell": 11, "street": 12, "street_lazy": 11, "empty_mesh": 11}


def new_rows(old, new):
    """indices of `new` whose row occurs nowhere in `old`: the instances a step adds, as opposed to those it shifts"""
    have = {r.tobytes() for r in rows(old)}
    return [i for i, r in enumerate(rows(new)) if r.tobytes() not in have]


def aim_ids(old, new):
    """(the instances the rays of a step are aimed at: of the added ones the new before the shifted, at most 8, and two that stayed; all added ones)"""
    fresh = new_rows(old, new)
    added = fresh + [i for i in added_ids(old, new) if i not in fresh]
    kept = [i for i in range(len(rows(new))) if i not in added]
    return added[:8] + kept[:1] + kept[-1:], added


def alpha_added(old, new):
    """the new instances of a step that are alpha-tested (without RT_INST_FORCE_OPAQUE)"""
    return [i for i in new_rows(old, new) if not rows(new)["flags"][i] & FORCE_OPAQUE]


def informative(desc, closest, ids, alpha_ids):
    """(rays that hit, of them on the aimed-at instances, of them on the instances `alpha_ids`) of a trace_closest result"""
    tri = closest.view(np.uint32)[:, 1]
    hit = tri != 0xffffffff
    inst_of = refit.tri_ref(desc)[tri[hit], 0]
    return int(hit.sum()), int(np.isin(inst_of, ids).sum()), int(np.isin(inst_of, alpha_ids).sum())


def bound_box_scene(light_lib):
    """(scene, description, sources, bound instances, a table that moves the box): Cornell whose second light record is taken from triangle 0 of the short box, a
    non-emissive instance — a light-source binding over these records names the box, and rt_set_instances then holds the box in place like the emitter"""
    import lights
    sc = refit.cornell()
    desc = sc.desc()
    inst, pm = refit.instances_of(desc), refit.prim_meshes_of(desc)
    box = 3
    src, rec = sc.lightSources().copy(), lights.records_of(desc)
    src[1] = (box, 0)
    rec["matIndex"][1] = pm["materialIndex"][inst["primMesh"][box]]
    rec, n = lights.rewrite(light_lib, desc, src, rec)
    assert n == len(src) == 2
    moved = inst.copy()
    moved["objectToWorld"][box][3] += np.float32(0.125)
    return sc, lights.with_lights(desc, rec), src, sorted(set(int(i) for i in src["instance"])), box, moved
