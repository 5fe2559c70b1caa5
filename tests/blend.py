"""Blended variants of scene descriptions: what the alpha-blend tests share (tests/test_blend_cpu.py, tests/test_gpu_blend.py, the veiled fuzz sweep).

Every non-opaque material of the procedural scenes is RT_ALPHA_MASK: its opacity is 0 or 1, so the alpha draw keyed on (ray seed, triangle id) — DESIGN.md §6
deviation 1 — never decides anything and a frame at rest repeats its G-buffer texel for texel.  `veil` turns materials into RT_ALPHA_BLEND at a base alpha
strictly between 0 and 1: then which surface a ray stops at depends on the frame's seed.  The procedural scenes themselves stay as they are; the edit happens
on a copy of the description."""
import ctypes as C
import os
import numpy as np

from helpers import abi, host
import refit

GLTF = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "blend_panes.gltf")
ALPHA_OPAQUE, ALPHA_MASK, ALPHA_BLEND = 0, 1, 2
INST_FORCE_OPAQUE = 1
# rt_material as 20 words
W_BASE_ALPHA, W_BASE_TEXTURE, W_EMISSIVE, W_ALPHA_MODE, W_ALPHA_CUTOFF = 3, 4, slice(9, 12), 17, 18


def materials_of(desc):
    """a copy of the material table as rows of 20 words (uint32; view as float32 for the factors)"""
    return np.frombuffer((C.c_char * (desc.numMaterials * 80)).from_address(desc.materials), dtype=np.uint32).reshape(-1, 20).copy()


def with_parts(desc, materials=None, instances=None):
    """a copy of the description that reads the edited material rows / instance rows (kept alive by the copy, like the description it was copied from)"""
    d = abi.SceneDesc.from_buffer_copy(desc)
    keep = [desc]
    if materials is not None:
        m = np.ascontiguousarray(materials).view(np.uint32).reshape(-1, 20)
        assert m.shape[0] == desc.numMaterials
        d.materials = m.ctypes.data
        keep.append(m)
    if instances is not None:
        i = np.ascontiguousarray(instances, dtype=refit.INSTANCE_DT)
        assert i.size == desc.numInstances
        d.instances = i.ctypes.data
        keep.append(i)
    d._keep = keep
    return d


def blended_materials(desc, every, alpha):
    """(edited material rows, indices of the materials that became RT_ALPHA_BLEND): every `every`-th material that does not emit, and every MASK material"""
    mats = materials_of(desc)
    emits = (mats[:, W_EMISSIVE].view(np.float32) != 0).any(axis=1)
    pick = ((np.arange(len(mats)) % every == 0) | (mats[:, W_ALPHA_MODE] == ALPHA_MASK)) & ~emits
    mats[pick, W_ALPHA_MODE] = ALPHA_BLEND
    mats[pick, W_BASE_ALPHA] = np.array([alpha], np.float32).view(np.uint32)[0]
    return mats, np.nonzero(pick)[0]


def veil_desc(desc, every=2, alpha=0.5):
    mats, picked = blended_materials(desc, every, alpha)
    inst, pm = refit.instances_of(desc), refit.prim_meshes_of(desc)
    blended = np.isin(np.maximum(pm["materialIndex"][inst["primMesh"]], 0), picked)
    inst["flags"][blended] &= ~np.uint32(INST_FORCE_OPAQUE)
    return with_parts(desc, mats, inst)


def veil(sc, every=2, alpha=0.5, env=None):
    """the scene's description with every `every`-th non-emissive material and every MASK material blended at base alpha `alpha`, and RT_INST_FORCE_OPAQUE
    cleared on the instances that use one.  Emitters stay opaque: the light records are those of the scene"""
    return veil_desc(sc.desc(env), every, alpha)


def blended_instances(desc):
    """instances that go through the alpha test and whose material is RT_ALPHA_BLEND"""
    inst, pm, mats = refit.instances_of(desc), refit.prim_meshes_of(desc), materials_of(desc)
    mode = mats[np.maximum(pm["materialIndex"][inst["primMesh"]], 0), W_ALPHA_MODE]
    return np.nonzero(((inst["flags"] & INST_FORCE_OPAQUE) == 0) & (mode == ALPHA_BLEND))[0]


SCENES = ("cornell", "street")


def scene(name):
    """(host scene, its plain description, the veiled one) — `gltf` is the fixture, blended as loaded"""
    if name == "gltf":
        sc = host.Scene()
        assert sc.load(GLTF), GLTF
        return sc, None, sc.desc()
    sc = refit.cornell() if name == "cornell" else refit.street()
    return sc, sc.desc(), veil(sc)


def state(sc, w, h):
    st = host.default_state(w, h, sc, None)
    st.environmentProb = 0.0
    if not np.isfinite(st.fireflyClampThreshold) or st.fireflyClampThreshold <= 0:
        st.fireflyClampThreshold = 100.0
    return st


def rest_camera(sc, w, h):
    """the scene's own pose, history matrices advanced as between two frames at rest; a copy"""
    sc.updateCamera(w, h)
    cam = sc.getCamera()
    return type(cam).from_buffer_copy(cam)


def changing_texels(oracle, sc, w, h, frames=8):
    """[texels of G-buffer that differ between frame f - 1 and f] for f = 1 .. frames - 1, at rest, st.time = 1000 + f"""
    st = state(sc, w, h)
    oracle.resize(w, h)
    sc.updateCamera(w, h)
    out, last = [], None
    for f in range(frames):
        st.time = 1000 + f
        oracle.set_camera(rest_camera(sc, w, h))
        oracle.render_frame(st, f)
        g = oracle.readback(abi.BUF_GBUFFER0 + (f & 1)).view(np.uint32).reshape(h * w, -1).copy()
        if last is not None:
            out.append(int((g != last).any(axis=1).sum()))
        last = g
    return out


# ---- the draw's distribution: one ray through two blended surfaces, many seeds
def all_blended(sc, alpha):
    """every material blended at `alpha` (emitters too: the rays below ask about geometry, not light), every instance through the alpha test"""
    desc = sc.desc()
    mats = materials_of(desc)
    mats[:, W_ALPHA_MODE] = ALPHA_BLEND
    mats[:, W_BASE_ALPHA] = np.array([alpha], np.float32).view(np.uint32)[0]
    inst = refit.instances_of(desc)
    inst["flags"] &= ~np.uint32(INST_FORCE_OPAQUE)
    return with_parts(desc, mats, inst)


def seeded_ray(origin, direction, n):
    """the same ray n times with n distinct seeds in word 7"""
    rays = np.zeros((n, 8), np.float32)
    rays[:, :3], rays[:, 3:6], rays[:, 6] = origin, np.asarray(direction, np.float64) / np.linalg.norm(direction), 1e28
    rays[:, 7] = (np.arange(n, dtype=np.uint64) * 30011 + 977).astype(np.uint32).view(np.float32)      # distinct, below 2^31
    return rays


def binomial_bound(p, n):
    """five standard deviations of a share of n independent draws of probability p"""
    return 5.0 * np.sqrt(p * (1.0 - p) / n)


def shares(hits):
    """(share of rays at the nearest surface seen, share of misses, number of distinct finite distances) of closest-hit results of one ray under many seeds"""
    t = hits[:, 0]
    hit = t < 1e27
    first = t[hit].min()
    return float((t == first).mean()), float((~hit).mean()), len(np.unique(t[hit]))


N_SEEDS = 65536
CENTRE_RAY = ((0.02, 1.0, 0.3), (0.0, 0.0, -1.0))     # Cornell: from near the middle of the box at the tall block's front face, the back wall behind it: two surfaces


def check_distribution(trace, alpha):
    """one ray, N_SEEDS seeds, through two surfaces of opacity alpha (all_blended Cornell): it stops at the first with probability alpha and passes both with
    probability (1 - alpha)^2; trace: rays -> closest-hit results"""
    first, miss, distances = shares(trace(seeded_ray(*CENTRE_RAY, N_SEEDS)))
    print("alpha", alpha, "first", first, "miss", miss)
    assert distances == 2
    assert abs(first - alpha) <= binomial_bound(alpha, N_SEEDS), (alpha, first)
    p = (1.0 - alpha) ** 2
    assert abs(miss - p) <= binomial_bound(p, N_SEEDS), (alpha, miss, p)


def random_rays(desc, n, seed):
    """n rays from inside the scene's box, a random seed each"""
    rng = np.random.default_rng(seed)
    lo = np.min([refit.world_bounds(desc, i)[0] for i in range(desc.numInstances)], axis=0)
    hi = np.max([refit.world_bounds(desc, i)[1] for i in range(desc.numInstances)], axis=0)
    rays = np.zeros((n, 8), np.float32)
    rays[:, :3] = rng.uniform(lo, hi, (n, 3))
    d = rng.normal(size=(n, 3))
    # every other ray is aimed into the box of a blended instance (the street is open to the sky: most random directions leave it)
    ids = blended_instances(desc)
    if len(ids):
        box = np.array([refit.world_bounds(desc, int(i)) for i in ids])[rng.integers(0, len(ids), n // 2)]
        d[::2][:n // 2] = rng.uniform(box[:, 0], box[:, 1]) - rays[::2, :3][:n // 2]
    rays[:, 3:6] = d / np.linalg.norm(d, axis=1, keepdims=True)
    rays[:, 6] = 1e28
    rays[:, 7] = rng.integers(0, 2 ** 31, n).astype(np.uint32).view(np.float32)
    return rays


# ---- the opacity micro-map against float64
def cell_points(rng):
    """16 barycentric (u, v) inside each of the 36 cells of the 8 x 8 micro-map that meet the triangle: cell (i, j) is u in [i/8, (i+1)/8), v in [j/8, (j+1)/8),
    and on the diagonal cells (i + j == 7) only the half with u + v < 1.  Returns (cells, 16, 2) and the cell numbers j * 8 + i"""
    cells = [(i, j) for j in range(8) for i in range(8 - j)]
    p = rng.uniform(0.02, 0.98, (len(cells), 16, 2))
    out = np.zeros_like(p)
    for c, (i, j) in enumerate(cells):
        q = p[c].copy()
        if i + j == 7:
            over = q.sum(axis=1) >= 1.0
            q[over] = 1.0 - q[over]
        out[c] = (q + [i, j]) / 8.0
    assert (out.sum(axis=2) < 1.0).all()
    return out, np.array([j * 8 + i for i, j in cells])


def micro_map_violations(desc, recs, seed=41):
    """recs: leaf records (refit.REC_DT fields globalId, omm) of non-opaque triangles of `desc`.  For every cell, the opacity at 16 points inside it in float64
    (base alpha x the alpha channel through test_trace_pin.sample_f64): state 1 requires opacity >= 1 at every point (blend) or > cutoff (mask), state 2 opacity
    == 0 at every point (blend) or < cutoff (mask).  Returns ([(globalId, cell, state, lowest, highest opacity)], {(alpha mode, state): cells})"""
    from test_trace_pin import sample_f64, _textures
    ref = refit.tri_ref(desc)
    inst, pm, mats = refit.instances_of(desc), refit.prim_meshes_of(desc), materials_of(desc)
    texcoord = np.frombuffer((C.c_char * (desc.numVertices * 32)).from_address(desc.vertices), dtype=abi.VERTEX_DT)["texcoord"]
    idx = np.frombuffer((C.c_char * (desc.numIndices * 4)).from_address(desc.indices), dtype=np.uint32)
    textures = _textures(desc)
    pts, cells = cell_points(np.random.default_rng(seed))
    u, v = pts[..., 0], pts[..., 1]
    seen = {(mode, s): 0 for mode in (ALPHA_MASK, ALPHA_BLEND) for s in (0, 1, 2)}
    bad = []
    for rec in recs:
        i, prim = ref[rec["globalId"]]
        mesh = pm[inst["primMesh"][i]]
        mat = mats[max(0, int(mesh["materialIndex"]))]
        mode, tex = int(mat[W_ALPHA_MODE]), int(mat[W_BASE_TEXTURE].view(np.int32))
        base, cutoff = float(mat[W_BASE_ALPHA].view(np.float32)), float(mat[W_ALPHA_CUTOFF].view(np.float32))
        assert mode in (ALPHA_MASK, ALPHA_BLEND), int(rec["globalId"])
        opacity = np.full(u.shape, base)
        if tex >= 0 and textures[tex][0] is not None:
            tri = idx[int(mesh["firstIndex"]) + 3 * int(prim):][:3].astype(np.int64) + int(mesh["vertexOffset"])
            t = texcoord[tri].astype(np.float64)
            uv = t[0] * (1.0 - u - v)[..., None] + t[1] * u[..., None] + t[2] * v[..., None]
            opacity = base * sample_f64(textures[tex], uv, 3)
        states = (rec["omm"][cells >> 4] >> ((cells & 15) * 2).astype(np.uint32)) & 3
        lo, hi = opacity.min(axis=1), opacity.max(axis=1)
        for s in (0, 1, 2):
            seen[(mode, s)] += int((states == s).sum())
        if mode == ALPHA_BLEND:
            wrong = (states == 3) | ((states == 1) & ~(lo >= 1.0)) | ((states == 2) & ~(hi == 0.0))
        else:
            wrong = (states == 3) | ((states == 1) & ~(lo > cutoff)) | ((states == 2) & ~(hi < cutoff))
        bad += [(int(rec["globalId"]), int(cells[c]), int(states[c]), float(lo[c]), float(hi[c])) for c in np.nonzero(wrong)[0]]
    return bad, seen
