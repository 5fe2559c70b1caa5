"""What the material / texture edit tests share (tests/test_materials_cpu.py, tests/test_gpu_materials.py).

Tables   a scene description whose material rows, texels and instance rows live in numpy arrays of this object: an edit changes the arrays, `desc()` is the
         edited description a fresh context uploads.
edge()   the edge scene: 30 alpha-tested triangles in seven prim meshes (one per material) over an opaque floor, textures of 1x1, 37x19 and 64x64 texels with
         alpha ramps (bands of columns: exact 0, 90, mixed, 160, 255), and uvs that take every path of the micro-map rule (csrc/opacity_map.h).
ops()    a seeded generator of edit sequences, interleaved with rt_set_instances / rt_update_instances / rt_rebuild_accel steps and with refused calls.
No tolerance anywhere: every comparison is word for word."""
import ctypes as C
import numpy as np

from helpers import abi
import blend
import refit

WRAP_REPEAT, WRAP_CLAMP, WRAP_MIRROR = 10497, 33071, 33648
FILTER_NEAREST, FILTER_LINEAR = 9728, 9729
FORCE_OPAQUE, CULL_DISABLE = 1, 2
TEXTURE_DT = np.dtype([("bgra8", "<u8"), ("width", "<i4"), ("height", "<i4"), ("wrapS", "<i4"), ("wrapT", "<i4"), ("magFilter", "<i4"), ("pad", "<i4")])   # rt_texture, 32 B
W_ROUGHNESS, W_EMISSIVE_TEXTURE, W_COLOUR = 6, 8, slice(0, 3)
ALPHA_WORDS = (blend.W_BASE_ALPHA, blend.W_BASE_TEXTURE, blend.W_ALPHA_MODE, blend.W_ALPHA_CUTOFF)      # the alpha-relevant fields of a material row
f2u = lambda x: np.array([x], np.float32).view(np.uint32)[0]      # noqa: E731


def _raw(ptr, nbytes):
    return np.frombuffer((C.c_char * nbytes).from_address(ptr), dtype=np.uint8)


class Tables:
    """the editable parts of a description (material rows as 20 words, texels per texture, instance rows) next to the description they were copied from"""

    def __init__(self, desc, keep=()):
        self.base, self.keep = desc, list(keep)
        self.mats = blend.materials_of(desc)
        self.inst = refit.instances_of(desc)
        self.tex_rows = _raw(desc.textures, desc.numTextures * 32).view(TEXTURE_DT).copy() if desc.textures else np.zeros(0, TEXTURE_DT)
        self.texels = []
        for t in self.tex_rows:
            ok = t["bgra8"] and t["width"] > 0 and t["height"] > 0
            self.texels.append(_raw(int(t["bgra8"]), int(t["width"]) * int(t["height"]) * 4).reshape(int(t["height"]), int(t["width"]), 4).copy() if ok else None)

    def desc(self, instances=None):
        """the description as edited so far (a new object each time; the arrays it points into are copies, kept alive by it)"""
        d = abi.SceneDesc.from_buffer_copy(self.base)
        mats, inst = self.mats.copy(), (self.inst if instances is None else np.ascontiguousarray(instances, dtype=refit.INSTANCE_DT)).copy()
        rows, texels = self.tex_rows.copy(), [None if t is None else t.copy() for t in self.texels]
        for k, t in enumerate(texels):
            if t is not None:
                rows["bgra8"][k] = t.ctypes.data
        d.materials, d.instances, d.numInstances = mats.ctypes.data, inst.ctypes.data, len(inst)
        if len(rows):
            d.textures = rows.ctypes.data
        d._keep = [self.base, self.keep, mats, inst, rows, texels]
        return d

    def material_of_mesh(self, mesh):
        return max(0, int(refit.prim_meshes_of(self.base)["materialIndex"][mesh]))

    def texture_size(self, t):
        return int(self.tex_rows["width"][t]), int(self.tex_rows["height"][t])

    def alpha_instances(self, materials):
        """instances of the current table that take the alpha test and use one of `materials`"""
        pm = refit.prim_meshes_of(self.base)
        m = np.maximum(pm["materialIndex"][self.inst["primMesh"]], 0)
        return np.nonzero(np.isin(m, list(materials)) & ((self.inst["flags"] & FORCE_OPAQUE) == 0))[0]


def of_scene(sc, desc=None):
    """Tables over a host scene's description (or over an edited copy of it, such as blend.veil's); the scene stays alive with them"""
    return Tables(sc.desc() if desc is None else desc, keep=[sc])


# ---- the edge scene --------------------------------------------------------------------------------------------------------------------------------------------
def ramp(w, h, seed):
    """BGRA8 texels whose alpha runs in five bands of columns: exact 0, 90, mixed values (per texel), 160, 255"""
    rng = np.random.default_rng(seed)
    t = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
    edges = [round(w * k / 5) for k in range(6)]
    for band, value in ((0, 0), (1, 90), (3, 160), (4, 255)):
        t[:, edges[band]:edges[band + 1], 3] = value
    return t


def _material(base_alpha=1.0, texture=-1, mode=blend.ALPHA_MASK, cutoff=0.5, emissive_texture=-1):
    m = np.zeros(20, np.float32)
    m[0:3], m[3] = 0.8, base_alpha
    m.view(np.int32)[[4, 7, 8, 12, 15]] = -1
    m.view(np.int32)[4], m.view(np.int32)[8] = texture, emissive_texture
    m[5], m[6], m[13], m[16] = 0.0, 0.7, 1.0, 1.5
    m.view(np.int32)[17], m[18] = mode, cutoff
    return m.view(np.uint32)


# texture ids of the edge scene; materials 1..7 are the alpha-tested ones, 0 is the floor
T_ONE, T_ODD, T_SQUARE, T_SQUARE_CLAMPED, T_EMISSIVE = range(5)
NAN, INF = float("nan"), float("inf")
# per alpha-tested material: the uv triples of its triangles (uv0 uv1 uv2).  What each is there for stands beside it.
EDGE_UVS = {
    1: [(0.05, 0.1, 0.30, 0.1, 0.05, 0.35), (0.70, 0.2, 0.95, 0.2, 0.70, 0.45), (0.36, 0.6, 0.60, 0.6, 0.36, 0.85),          # 64x64 REPEAT LINEAR, MASK: the bands of 0, of 255 and the mixed one
        (-1.95, -0.9, -1.70, -0.9, -1.95, -0.65), (-0.30, -2.2, -0.05, -2.2, -0.30, -1.95),                                      # negative texcoords under REPEAT
        (0.0, 0.0, 600.0, 0.0, 0.0, 1.0),                                                                                         # a span of 4096 texels or more
        (0.22, 0.1, 0.38, 0.1, 0.22, 0.3), (0.63, 0.5, 0.78, 0.5, 0.63, 0.7)],                                                   # the bands of 90 and of 160: a cutoff edit opens and closes their cells
    2: [(0.05, 0.1, 0.30, 0.1, 0.05, 0.5), (0.72, 0.3, 0.97, 0.3, 0.72, 0.8), (-0.95, -0.4, -0.72, -0.4, -0.95, -0.1),          # 37x19 MIRROR / CLAMP NEAREST; negative texcoords
        (0.0, 0.0, 64.0, 0.0, 0.0, 96.0),                                                                                         # more than 65536 texels per cell (8 x 12 wraps)
        (NAN, 0.1, 0.3, 0.1, 0.05, 0.5), (0.05, 0.1, INF, 0.1, 0.05, 0.5)],                                                       # non-finite texcoords
    3: [(0.05, 0.1, 0.30, 0.1, 0.05, 0.35), (0.70, 0.2, 0.95, 0.2, 0.70, 0.45), (-0.9, -1.4, -0.6, -1.4, -0.9, -1.1),            # 64x64 CLAMP / MIRROR LINEAR, BLEND; negative texcoords
        (1.2, 0.3, 1.6, 0.3, 1.2, 0.7), (0.36, 0.6, 0.60, 0.6, 0.36, 0.85)],
    4: [(0.0, 0.0, 1.0, 0.0, 0.0, 1.0), (0.3, 0.3, 0.5, 0.3, 0.3, 0.5)],                                                        # no texture
    5: [(0.0, 0.0, 1.0, 0.0, 0.0, 1.0), (0.3, 0.3, 0.5, 0.3, 0.3, 0.5)],                                                        # negative base alpha, 1x1 texture
    6: [(0.05, 0.1, 0.30, 0.1, 0.05, 0.35), (0.70, 0.2, 0.95, 0.2, 0.70, 0.45), (0.36, 0.6, 0.60, 0.6, 0.36, 0.85),              # BLEND at base alpha 1.5 on the texture material 1 uses
        (-0.28, 0.2, -0.05, 0.2, -0.28, 0.45), (0.1, 0.1, 0.9, 0.1, 0.1, 0.9)],
    7: [(0.0, 0.0, 1.0, 0.0, 0.0, 1.0), (-5.0, 3.0, 9.0, 3.0, -5.0, 40.0)],                                                      # 1x1 texture, huge uvs
}


class _EdgeArrays:
    pass


def edge():
    """the edge scene as Tables"""
    k = _EdgeArrays()
    k.texels = [np.array([[[10, 20, 30, 200]]], np.uint8), ramp(37, 19, 1), ramp(64, 64, 2), ramp(64, 64, 2), ramp(8, 8, 3)]
    samplers = [(WRAP_REPEAT, WRAP_REPEAT, FILTER_NEAREST), (WRAP_MIRROR, WRAP_CLAMP, FILTER_NEAREST), (WRAP_REPEAT, WRAP_REPEAT, FILTER_LINEAR),
                (WRAP_CLAMP, WRAP_MIRROR, FILTER_LINEAR), (WRAP_REPEAT, WRAP_REPEAT, FILTER_LINEAR)]
    k.tex = np.zeros(len(k.texels), TEXTURE_DT)
    for i, (t, s) in enumerate(zip(k.texels, samplers)):
        k.tex[i] = (t.ctypes.data, t.shape[1], t.shape[0], s[0], s[1], s[2], 0)
    k.mats = np.stack([_material(mode=blend.ALPHA_OPAQUE),
                       _material(1.0, T_SQUARE, blend.ALPHA_MASK, 0.5, emissive_texture=T_EMISSIVE), _material(1.0, T_ODD, blend.ALPHA_MASK, 0.5),
                       _material(1.0, T_SQUARE_CLAMPED, blend.ALPHA_BLEND), _material(0.8, -1, blend.ALPHA_MASK, 0.5), _material(-0.5, T_ONE, blend.ALPHA_MASK, 0.5),
                       _material(1.5, T_SQUARE, blend.ALPHA_BLEND), _material(1.0, T_ONE, blend.ALPHA_MASK, 0.5)])
    verts, prims = [], []
    slot = 0
    for m in sorted(EDGE_UVS):
        first = len(verts)
        for uv in EDGE_UVS[m]:
            x, y = 1.25 * (slot % 6), 1.25 * (slot // 6)
            slot += 1
            for (px, py), (u, v) in zip(((x, y), (x + 1.0, y), (x, y + 1.0)), (uv[0:2], uv[2:4], uv[4:6])):
                verts.append([px, py, 0.0, 0.0, u, v, 0.0, 0.0])
        prims.append([first, len(verts) - first, first, len(verts) - first, m])
    first = len(verts)      # the floor: two opaque triangles under everything
    for p in ((-1, -1), (9, -1), (9, 9), (-1, -1), (9, 9), (-1, 9)):
        verts.append([p[0], p[1], -1.0, 0.0, 0.0, 0.0, 0.0, 0.0])
    prims.append([first, 6, first, 6, 0])
    k.verts = np.array(verts, np.float32)
    k.indices = np.concatenate([np.arange(p[1], dtype=np.uint32) for p in prims])
    k.prims = np.array(prims, np.int32)
    k.inst = np.zeros(len(prims), refit.INSTANCE_DT)
    k.inst["objectToWorld"][:] = np.eye(4, dtype=np.float32)[:3].reshape(12)
    k.inst["primMesh"] = np.arange(len(prims))
    k.inst["flags"] = CULL_DISABLE
    k.inst["flags"][-1] |= FORCE_OPAQUE
    d = abi.SceneDesc()
    d.numPrimMeshes, d.primMeshes = len(prims), k.prims.ctypes.data
    d.numVertices, d.vertices = len(k.verts), k.verts.ctypes.data
    d.numIndices, d.indices = len(k.indices), k.indices.ctypes.data
    d.numInstances, d.instances = len(k.inst), k.inst.ctypes.data
    d.numMaterials, d.materials = len(k.mats), k.mats.ctypes.data
    d.numTextures, d.textures = len(k.tex), k.tex.ctypes.data
    return Tables(d, keep=[k])


def triangle_inputs(t):
    """[(material, uv(6), texture or -1)] of every triangle of an alpha-tested instance of Tables `t`, in (instance, triangle) order"""
    d = t.desc()
    pm = refit.prim_meshes_of(d)
    uv = _raw(d.vertices, d.numVertices * 32).view(np.float32).reshape(-1, 8)[:, 4:6]
    idx = _raw(d.indices, d.numIndices * 4).view(np.uint32)
    out = []
    for i in t.inst:
        if i["flags"] & FORCE_OPAQUE:
            continue
        mesh = pm[i["primMesh"]]
        m = max(0, int(mesh["materialIndex"]))
        for p in range(int(mesh["indexCount"]) // 3):
            tri = idx[int(mesh["firstIndex"]) + 3 * p:][:3].astype(np.int64) + int(mesh["vertexOffset"])
            out.append((m, uv[tri].reshape(6).copy(), int(t.mats[m, blend.W_BASE_TEXTURE].view(np.int32))))
    return out


def opacity_map(t, material, uv):
    """rt_opacity_map of one triangle under material row `material` of Tables `t`"""
    from restir_amd.renderer import Renderer
    row = t.mats[material]
    tex = int(row[blend.W_BASE_TEXTURE].view(np.int32))
    s = t.tex_rows[tex] if tex >= 0 else None
    return Renderer.opacity_map(uv, row[blend.W_BASE_ALPHA].view(np.float32), row[blend.W_ALPHA_CUTOFF].view(np.float32), int(row[blend.W_ALPHA_MODE]),
                                t.texels[tex] if tex >= 0 else None, *((int(s["wrapS"]), int(s["wrapT"]), int(s["magFilter"])) if tex >= 0 else ()))


CELLS = np.array([j * 8 + i for j in range(8) for i in range(8 - j)])


def states(omm):
    """the 36 cell states of four micro-map words (or of rows of them)"""
    omm = np.asarray(omm, np.uint32)
    return (omm[..., CELLS >> 4] >> ((CELLS & 15) * 2).astype(np.uint32)) & 3


def expected_alpha_record(t, material, uv):
    """the alpha record (abi.ALPHA_REC_DT) a build derives for a triangle with these texcoords under material row `material`"""
    row = t.mats[material]
    a = np.zeros((), abi.ALPHA_REC_DT)
    a["uv"], a["baseAlpha"], a["cutoff"] = uv, row[blend.W_BASE_ALPHA].view(np.float32), row[blend.W_ALPHA_CUTOFF].view(np.float32)
    a["alphaMode"], a["texture"] = int(row[blend.W_ALPHA_MODE]), 0xffffffffffffffff
    tex = int(row[blend.W_BASE_TEXTURE].view(np.int32))
    if tex >= 0:
        s = t.tex_rows[tex]
        a["texture"], a["w"], a["h"], a["wrapS"], a["wrapT"], a["filter"] = tex, s["width"], s["height"], s["wrapS"], s["wrapT"], s["magFilter"]
    return a


# ---- edit sequences ------------------------------------------------------------------------------------------------------------------------------------------
MATERIAL_KINDS = ("cutoff", "base_alpha", "mode", "base_texture", "roughness", "colour")
RECT_KINDS = ("one", "full_width", "last_row", "last_column", "padded", "same_alpha")
OTHER_KINDS = ("set_instances", "update_instances", "rebuild_accel")
REFUSALS = ("null", "id_range", "duplicate", "bad_texture", "light_rule_on", "light_rule_off", "texture_range", "empty_rect", "rect_outside", "pitch", "null_texels")
KINDS = MATERIAL_KINDS + RECT_KINDS + OTHER_KINDS + ("refused",)
SEEDS, OPS = (1, 2, 3, 4, 5, 6), 12
MESSAGE = {"null": "NULL ids / rows", "id_range": "id out of range", "duplicate": "listed twice", "bad_texture": "material references a missing texture",
           "light_rule_on": "light rule", "light_rule_off": "light rule", "texture_range": "out of range", "empty_rect": "empty rectangle",
           "rect_outside": "leaves the texture", "pitch": "rowPitchBytes", "null_texels": "NULL texels"}


def _emissive(t):
    e = t.mats[:, blend.W_EMISSIVE].view(np.float32)
    return 0.2126 * e[:, 0] + 0.7152 * e[:, 1] + 0.0722 * e[:, 2] > 1e-2


def alpha_materials(t):
    """materials that an alpha-tested instance of the table uses and that do not emit"""
    pm = refit.prim_meshes_of(t.base)
    used = np.unique(np.maximum(pm["materialIndex"][t.inst["primMesh"][(t.inst["flags"] & FORCE_OPAQUE) == 0]], 0))
    return [int(m) for m in used if not _emissive(t)[m]]


def draw(t, rng, kind):
    """one op of `kind` over Tables `t` as a dict; applying it is `apply` (the tables) and `issue` (a context)"""
    mats = alpha_materials(t) or [0]
    m = int(rng.choice(mats))
    row = t.mats[m].copy()
    if kind in MATERIAL_KINDS:
        if kind == "cutoff":
            row[blend.W_ALPHA_CUTOFF] = f2u(rng.choice([0.0, 0.1, 0.5, 0.9, 1.0, 2.0]))
        elif kind == "base_alpha":
            row[blend.W_BASE_ALPHA] = f2u(rng.choice([0.0, 0.25, 0.6, 1.0, 1.5, -0.5]))
        elif kind == "mode":
            row[blend.W_ALPHA_MODE] = blend.ALPHA_BLEND if row[blend.W_ALPHA_MODE] == blend.ALPHA_MASK else blend.ALPHA_MASK
        elif kind == "base_texture":
            row[blend.W_BASE_TEXTURE] = np.array([rng.integers(-1, len(t.tex_rows))], np.int32).view(np.uint32)[0]
        elif kind == "roughness":
            row[W_ROUGHNESS] = f2u(rng.uniform(0.05, 1.0))
        else:
            row[W_COLOUR] = rng.uniform(0.1, 1.0, 3).astype(np.float32).view(np.uint32)
        return {"kind": kind, "ids": [m], "rows": row.reshape(1, 20)}
    if kind in RECT_KINDS:
        used = [int(x) for x in t.mats[mats, blend.W_BASE_TEXTURE].view(np.int32) if x >= 0]
        tex = int(rng.choice(used)) if used and rng.random() < 0.8 else int(rng.integers(0, len(t.tex_rows)))
        w, h = t.texture_size(tex)
        if kind == "one":
            x, y, rw, rh = int(rng.integers(0, w)), int(rng.integers(0, h)), 1, 1
        elif kind == "full_width":
            y = int(rng.integers(0, h)); x, rw, rh = 0, w, int(rng.integers(1, h - y + 1))
        elif kind == "last_row":
            x = int(rng.integers(0, w)); y, rw, rh = h - 1, int(rng.integers(1, w - x + 1)), 1
        elif kind == "last_column":
            y = int(rng.integers(0, h)); x, rw, rh = w - 1, 1, int(rng.integers(1, h - y + 1))
        else:
            x, y = int(rng.integers(0, w)), int(rng.integers(0, h)); rw, rh = int(rng.integers(1, w - x + 1)), int(rng.integers(1, h - y + 1))
        texels = rng.integers(0, 256, (rh, rw, 4), dtype=np.uint8)
        texels[..., 3] = rng.choice([0, 255, 90, 160], (rh, rw))
        if kind == "same_alpha":      # colour changes, every alpha byte stays
            texels[..., 3] = t.texels[tex][y:y + rh, x:x + rw, 3]
        return {"kind": kind, "texture": tex, "x": x, "y": y, "texels": texels, "pitch": 4 * rw + 12 if kind == "padded" else None}
    if kind == "rebuild_accel":
        return {"kind": kind, "builder": int(rng.integers(0, 2))}
    if kind == "update_instances":
        ids = sorted(int(i) for i in rng.choice(len(t.inst), min(2, len(t.inst)), replace=False) if not _emissive(t)[t.material_of_mesh(t.inst["primMesh"][i])])
        xf = np.stack([refit.compose(refit.translation(rng.uniform(-0.2, 0.2, 3)), t.inst["objectToWorld"][i]) for i in ids]) if ids else np.zeros((0, 12), np.float32)
        return {"kind": kind, "ids": ids, "xf": xf.astype(np.float32)}
    if kind == "set_instances":      # one more instance of a non-emissive mesh at the end, or the last added one goes again: emissive instances stay in place
        table = t.inst.copy()
        if len(table) > t.base.numInstances and rng.random() < 0.4:
            return {"kind": kind, "table": table[:-1]}
        pm = refit.prim_meshes_of(t.base)
        free = [k for k in range(len(pm)) if not _emissive(t)[t.material_of_mesh(k)] and pm["indexCount"][k] > 0]
        src = int(rng.choice([i for i in range(len(table)) if table["primMesh"][i] in free]))
        new = table[src:src + 1].copy()
        new["objectToWorld"][0] = refit.compose(refit.translation(rng.uniform(-0.5, 0.5, 3)), new["objectToWorld"][0])
        new["flags"][0] &= ~np.uint32(FORCE_OPAQUE)
        return {"kind": kind, "table": np.concatenate([table, new])}
    raise ValueError(kind)


def draw_refusal(t, rng, why):
    m = (alpha_materials(t) or [0])[0]
    row = t.mats[m].copy().reshape(1, 20)
    if why == "null":
        return {"kind": "refused", "why": why, "call": "materials", "ids": None, "rows": None, "count": 1}
    if why == "id_range":
        return {"kind": "refused", "why": why, "call": "materials", "ids": [len(t.mats)], "rows": row}
    if why == "duplicate":
        return {"kind": "refused", "why": why, "call": "materials", "ids": [m, m], "rows": np.concatenate([row, row])}
    if why == "bad_texture":
        row[0, blend.W_BASE_TEXTURE] = len(t.tex_rows)
        return {"kind": "refused", "why": why, "call": "materials", "ids": [m], "rows": row}
    if why in ("light_rule_on", "light_rule_off"):
        lit = np.nonzero(_emissive(t))[0]
        if why == "light_rule_off" and not len(lit):
            why = "light_rule_on"
        m = m if why == "light_rule_on" else int(lit[0])
        row = t.mats[m].copy().reshape(1, 20)
        row[0, blend.W_EMISSIVE] = np.float32([5, 5, 5] if why == "light_rule_on" else [0, 0, 0]).view(np.uint32)
        return {"kind": "refused", "why": why, "call": "materials", "ids": [m], "rows": row}
    tex = 0
    w, h = t.texture_size(tex) if len(t.tex_rows) else (1, 1)
    one = np.zeros((1, 1, 4), np.uint8)
    rect = {"texture_range": (len(t.tex_rows), 0, 0, one, None), "empty_rect": (tex, 0, 0, np.zeros((0, 1, 4), np.uint8), None), "rect_outside": (tex, w, 0, one, None),
            "pitch": (tex, 0, 0, one, 3), "null_texels": (tex, 0, 0, None, None)}[why]
    return {"kind": "refused", "why": why, "call": "texture", "texture": rect[0], "x": rect[1], "y": rect[2], "texels": rect[3], "pitch": rect[4]}


def ops(t, seed, n=OPS):
    """n ops over a copy of Tables `t` (the generator follows its own edits): every kind of KINDS appears within SEEDS at OPS ops each, refusals included"""
    t = clone(t)
    rng = np.random.default_rng(1000 + seed)
    out = []
    plain = KINDS[:-1]
    for k in range(n):      # every third op is a refused call; the kinds rotate so that SEEDS x OPS reach all of them, the parameters are the seed's
        if k % 3 == 2:
            op = draw_refusal(t, rng, REFUSALS[(seed * 4 + k // 3) % len(REFUSALS)])
        else:
            op = draw(t, rng, plain[(seed * 8 + k - k // 3) % len(plain)])
        apply(t, op)
        out.append(op)
    return out


def clone(t):
    c = Tables.__new__(Tables)
    c.base, c.keep = t.base, t.keep
    c.mats, c.inst, c.tex_rows = t.mats.copy(), t.inst.copy(), t.tex_rows.copy()
    c.texels = [None if x is None else x.copy() for x in t.texels]
    return c


def clone_shallow(t):
    """Tables that share every array with `t`: for readers (draw, draw_refusal) that need another instance table over the same rows and texels"""
    c = Tables.__new__(Tables)
    c.base, c.keep, c.mats, c.inst, c.tex_rows, c.texels = t.base, t.keep, t.mats, t.inst, t.tex_rows, t.texels
    return c


def apply(t, op):
    """the op on the tables (what a fresh context of t.desc() then uploads); a refused op changes nothing"""
    kind = op["kind"]
    if kind in MATERIAL_KINDS:
        t.mats[op["ids"]] = op["rows"]
    elif kind in RECT_KINDS:
        h, w = op["texels"].shape[:2]
        t.texels[op["texture"]][op["y"]:op["y"] + h, op["x"]:op["x"] + w] = op["texels"]
    elif kind == "update_instances":
        for i, m in zip(op["ids"], op["xf"]):
            t.inst["objectToWorld"][i] = m
    elif kind == "set_instances":
        t.inst = op["table"].copy()


def issue(r, op):
    """the op on a Renderer's context.  Returns the library's message for a refused op (the call must fail), else None"""
    from restir_amd.renderer import RtError, hip_lib
    kind = op["kind"]
    if kind in MATERIAL_KINDS:
        r.update_materials(op["ids"], op["rows"])
    elif kind in RECT_KINDS:
        r.update_texture(op["texture"], op["x"], op["y"], op["texels"], op["pitch"])
    elif kind == "update_instances":
        r.update_instances(op["ids"], op["xf"])
    elif kind == "set_instances":
        r.set_instances(op["table"])
    elif kind == "rebuild_accel":
        r.set_rebuild_options(op["builder"])
        r.rebuild_accel()
    else:
        L = hip_lib()
        if op["call"] == "materials":
            ids = None if op["ids"] is None else np.asarray(op["ids"], np.uint32)
            rows = None if op["rows"] is None else np.ascontiguousarray(op["rows"])
            rc = L.rt_update_materials(r._h, op.get("count", 0 if ids is None else len(ids)), None if ids is None else ids.ctypes.data, None if rows is None else rows.ctypes.data)
        else:
            tx = op["texels"]
            h, w = (1, 1) if tx is None else tx.shape[:2]
            buf = None if tx is None else np.ascontiguousarray(tx if tx.size else np.zeros((1, 1, 4), np.uint8))
            rc = L.rt_update_texture(r._h, op["texture"], op["x"], op["y"], w, h, None if buf is None else buf.ctypes.data, 4 * w if op["pitch"] is None else op["pitch"])
        assert rc == -1, (op["why"], rc)      # RT_ERR_INVALID_ARG
        return L.rt_last_error(r._h).decode()
    return None


def describe(op):
    """one line per op, enough to replay it by hand"""
    keep = {k: (v.tolist() if isinstance(v, np.ndarray) and v.size <= 24 else (v.shape if isinstance(v, np.ndarray) else v)) for k, v in op.items()}
    return repr(keep)
