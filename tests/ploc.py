"""ctypes driver of tests/ploc_checker.cpp (the CPU restatement of the device build with a builder selector: the LBVH of rt_rebuild_accel or PLOC) and
the tiny scenes the PLOC tests add to those of tests/accel_build.py.  The checker is compiled once per process as a library of its own, together with
tests/refit_checker.cpp and csrc/bvh8_builder.cpp; it includes tests/accel_build_checker.cpp as source, so abc_build and abc_check_structure are in the same library."""
import ctypes as C
import os
import subprocess
import numpy as np

from helpers import ROOT
import accel_build
import refit

SRC = os.path.join(ROOT, "tests", "ploc_checker.cpp")
LBVH, PLOC = 0, 1                 # rt_rebuild_options.builder
DEFAULT_RADIUS = 16               # csrc/accel_build.h ACCEL_PLOC_RADIUS_DEFAULT
DEFAULT_MAX_ITERATIONS = 512
RADII = (1, 2, DEFAULT_RADIUS, 64)
_lib = None


def build(out_dir):
    global _lib
    if _lib is not None:
        return _lib
    ref = refit.build(out_dir)
    so = os.path.join(str(out_dir), "libplocchk.so")
    subprocess.check_call([os.environ.get("CXX", "g++")] + refit.FLAGS + [SRC, refit.SRC, refit.BUILDER, "-o", so])
    L = C.CDLL(so)
    for name in ("rfc_build", "rfc_free", "rfc_counts", "rfc_pad", "rfc_copy", "rfc_refit", "rfc_check_tree"):
        getattr(L, name).argtypes = getattr(ref, name).argtypes
        getattr(L, name).restype = getattr(ref, name).restype
    L.abc_build.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    L.abc_check_structure.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_uint32, C.c_int, C.c_int, C.c_char_p, C.c_int]
    L.plc_build.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32, C.c_int, C.c_int, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p,
                            C.c_void_p, C.c_void_p]
    L.plc_inspect.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    _lib = L
    return L


REFUSED_DEPTH, REFUSED_ITERATIONS = 1, 3      # plc_build's return codes that are properties of the scene


def rebuilt(L, desc, host_tree, builder=PLOC, radius=DEFAULT_RADIUS, max_iterations=DEFAULT_MAX_ITERATIONS, max_levels=accel_build.STACK_MAX):
    """accel_build.rebuilt with a builder selector: the restated device build as a refit.Tree with .depth, .iterations, .sah_node, .sah_tri; the refusal code
    (REFUSED_*) when the builder refuses"""
    n = host_tree.ref.shape[0]
    table = accel_build.table_of(host_tree)
    nodes, recs = np.zeros(max(n, 1) * refit.NODE, np.uint8), np.zeros(n * refit.REC, np.uint8)
    counts, sah = np.zeros(4, np.uint32), np.zeros(2, np.float64)
    ref = np.ascontiguousarray(host_tree.ref)
    rc = L.plc_build(C.addressof(desc), host_tree.inst.ctypes.data, host_tree.inst.size // refit.INST, ref.ctypes.data, table.ctypes.data, n, max_levels,
                     builder, radius, max_iterations, nodes.ctypes.data, recs.ctypes.data, counts.ctypes.data, sah.ctypes.data)
    if rc in (REFUSED_DEPTH, REFUSED_ITERATIONS):
        return rc
    assert rc == 0, rc
    t = refit.Tree(L, desc, nodes[:int(counts[0]) * refit.NODE], recs, host_tree.inst, 0.0)
    assert t.refit([], np.zeros((0, 12), np.float32)) == 0      # the boxes: the restated refit in its full mode
    assert t.stats[3] == 1 and int(t.stats[1]) == int(counts[0])
    t.depth = t.levels_built = int(counts[1])
    t.iterations = int(counts[2])
    t.sah_node, t.sah_tri = float(sah[0]), float(sah[1])
    return t


def inspect(L, desc, host_tree, radius=DEFAULT_RADIUS):
    """what plc_build does not report (plc_inspect): (globalId by Morton position, the position every cluster chose in PLOC's first iteration, globalId by final leaf
    position, leaves of the root's left child — the first that many of the final order)"""
    n = host_tree.ref.shape[0]
    table = accel_build.table_of(host_tree)
    ref = np.ascontiguousarray(host_tree.ref)
    order, nn, final, left = np.zeros(n, np.uint32), np.zeros(n, np.uint32), np.zeros(n, np.uint32), C.c_uint32(0)
    rc = L.plc_inspect(C.addressof(desc), host_tree.inst.ctypes.data, host_tree.inst.size // refit.INST, ref.ctypes.data, table.ctypes.data, n, radius, max(n, 1),
                       order.ctypes.data, nn.ctypes.data, final.ctypes.data, C.addressof(left))
    assert rc == 0, rc
    return order, nn, final, int(left.value)


# ---- tiny scenes ------------------------------------------------------------------------------------------------------------------------------------------
def tiny(name):
    if name == "row600":        # 600 triangles on a line with irregular gaps: three 256-thread blocks, the window clipped at both ends.  One y and one z for all, so
        # the centres have no extent on those axes, the key depends on x only and the Morton order is the order of k; the closest pairs of their neighbourhoods are
        # k = 255 / 256 and 511 / 512 (gap 0.02, every other gap >= 0.05), each followed by a wide gap: mutual nearest neighbours across the block boundaries
        rng = np.random.default_rng(17)
        x = np.cumsum(0.05 + 0.6 * rng.random(600) ** 3)
        x[256] = x[255] + 0.02
        x[257:] += x[256] - x[257] + 0.9
        x[512] = x[511] + 0.02
        x[513:] += x[512] - x[513] + 0.9
        return accel_build.TinyScene([accel_build._tri([xk, 0.0, 0.0], 0.04) for xk in x])
    if name == "nested40":      # 40 concentric triangles, each box inside the next: every cluster prefers the smallest, one merge per iteration
        out = []
        for k in range(40):
            h = np.float32((k + 1) / 1024.0) * np.float32([1, 1, 1])     # c - h and c + h are exact, so every box centre is exactly c: all keys equal, the order is by size
            c = np.float32([1, 2, 3])
            out.append([c - h, c + h * np.float32([1, -1, 1]), c + h])
        return accel_build.TinyScene(out)
    if name == "two_far":       # two clumps of 20, far apart in space and in Morton order: a window of 1 or 2 positions sees the other clump only from the clump's edge
        rng = np.random.default_rng(23)
        out = [accel_build._tri(0.5 * rng.random(3), 0.05) for _ in range(20)]
        out += [accel_build._tri(np.float32([40, 30, 20]) + 0.5 * rng.random(3), 0.05) for _ in range(20)]
        return accel_build.TinyScene(out)
    raise ValueError(name)


TINY = ("row600", "nested40", "two_far")
SCENES = accel_build.SCENES + TINY


def make(name):
    """accel_build.make over SCENES"""
    if name in TINY:
        return tiny(name), [], np.zeros((0, 12), np.float32)
    return accel_build.make(name)


def host_tree(L, name):
    """accel_build.host_tree over SCENES: (scene, desc of the moved scene, the host-built refit.Tree carried through the moves, ids, transforms)"""
    sc, ids, xf = make(name)
    t = refit.Tree.built(L, sc.desc())
    if len(ids):
        assert t.refit(ids, xf) == 0
        sc.updateInstances(ids, xf)
    return sc, sc.desc(), t, ids, xf
