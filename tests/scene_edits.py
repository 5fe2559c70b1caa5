"""The model and the generator of the scene-edit sweep (tests/test_gpu_scene_edits.py, tests/test_scene_edits_cpu.py): not a test, no GPU.

Twin: a host.Scene plus the per-mesh skin and morph state.  It mirrors every scene-edit call of include/rt_abi.h with the host-side calls that already exist
(Scene.updateInstances / setInstances / updateVertices; the posed rows from tests/skin_checker.cpp and tests/morph_checker.cpp, morph first, then skin), so
Twin.desc() is at any point the description a host would upload from scratch.  It never reads anything back from a renderer.

ops(scene, seed, n): a list of plain records (kind, args) over the alphabet KINDS + REFUSED (KINDS_V2 + REFUSED for a seed outside SEEDS, see "Two families").  The arguments are symbolic (instance ids and the name of a move,
not matrices): Twin.calls() turns a record into the concrete calls against the twin's state at that point, so a sequence is reproducible from (scene, seed, n)
alone and prints as a few lines of JSON.  Every call carries the CPU verdict of the ABI's refusal rules on it (instances.verdict for tables, the restated rules
of the other calls below); the generator emits only records whose calls pass, except the one REFUSED record per sequence, whose call must fail.

The order of the kinds: the sweep has to contain every ordered pair of kinds in a handful of short sequences, which independent random walks do not give
(six walks of 24 cover about 70 of the 100 pairs).  So the walks of the default sequences (SCENES x SEEDS) are drawn together: each step prefers a pair no
earlier step of any default sequence has used, ties broken by the seeded generator.  Any other seed walks on its own with the same preference.  All arguments
are seeded random draws.

What the alphabet leaves out on purpose: a re-bind may pass through the empty table (set_skins / set_morph_targets with no entries) but ends with one skin table
and one morph table in place, and a morph set goes to a skinned mesh only once that skin has been posed — so that update_skins and update_morphs stay legal at
every step and the order of the kinds can be planned without looking at the state.

Two families.  Seeds in SEEDS walk KINDS, and their records are what they were before the alphabet was widened (tests/test_scene_edits_cpu.py holds their digest).
Every other seed walks KINDS_V2 = KINDS + materials, texture, rebuild_options (rt_update_materials, rt_update_texture, rt_set_rebuild_options).
The default sequences of the wider family (SCENES x SEEDS_V2, one seed per light mode) are drawn together over the 69 ordered pairs that have a new kind on a side:
each walk takes its share and goes on with the pairs it has not held itself, so every sequence alternates old and new kinds.  Their records stay symbolic:
  materials        a kind of materials.MATERIAL_KINDS, material ids and a seed; the rows are materials.draw over materials.of_scene(twin.sc), the twin follows with
                   Scene.setMaterials.  model: rt_material_stats' dirtyMaterials (an alpha field changed bitwise) and alphaRecords (Twin.alpha_records).
  texture          a kind of materials.RECT_KINDS, a texture, the material that steered the draw and a seed; the twin follows with Scene.setTexture.
  rebuild_options  a builder and a radius of ploc.RADII; the twin remembers the options in force (they survive build_accel), what the last device build ran with,
                   and whether PLOC's buffers exist: the first PLOC build on the working buffers makes rt_set_instances report a reallocation.
The refusals of the three calls are restated from include/rt_abi.h in _update_materials, _update_texture and _set_rebuild_options (NULL arrays cannot be passed
through the Renderer's methods and are left to tests/test_gpu_materials.py).  The generator steers three arguments and never the order of the kinds: where no instance takes
the alpha test (Cornell as loaded) the next table change clears RT_INST_FORCE_OPAQUE of a non-emitter, and the next edit gives that instance's material a MASK
mode; an edit of an alpha field names a material of an alpha-tested instance where there is one; the street sequences' refused record is one of each new call, the emitter-mode one's
the luminance change that only that mode refuses.
Emission: materials.MATERIAL_KINDS never touches emissiveFactor, so every fourth materials record is of the extra kind "emission": it scales the emissiveFactor of
an emissive material inside the light rule (a row across the rule is a refusal).  In mode "update" the checkpoint's rt_update_lights carries the twin's records;
in mode "binding" the row is followed by rt_update_lights, which include/rt_abi.h prescribes for a host that changed an emission and which leaves the binding in
place (the light-source section defines that combination, so such rows are drawn in that mode too); in mode "emitter" the row is accepted only while the luminance
keeps its bits, so the scale is 1 and the roughness alone changes — the row that changes the luminance is one of that mode's refusals.  The twin re-derives
lightLuminIntegInv of its state after every accepted row, as a host does."""
import tempfile
from collections import namedtuple
import numpy as np

from helpers import abi, host
import blend
import emitters
import instances
import materials
import morph
import ploc
import refit
import skin

KINDS = ("update_instances", "rebuild_accel", "build_accel", "set_instances", "set_emitters", "update_skins", "update_morphs", "update_vertices", "rebind", "lights")
KINDS_V2 = KINDS + ("materials", "texture", "rebuild_options")      # the wider alphabet: DESIGN.md §31 and §32
NEW_KINDS = KINDS_V2[len(KINDS):]
REFUSED = "refused"
UPDATES = ("update_instances", "update_skins", "update_morphs", "update_vertices")      # the kinds that refit the tree in place
SCENES = ("cornell", "street")
SEEDS = (1, 2, 3)                       # these seeds walk KINDS; every other seed walks KINDS_V2
SEEDS_V2 = (4, 5, 6)                    # the default sequences of the wider alphabet, one per light mode
OPS, EVERY = 24, 4                      # ops per sequence; a checkpoint after every fourth op and after the last
DEVICE_BUILDS = ("rebuild_accel", "set_instances", "set_emitters")      # the kinds that build a tree with the builder of rt_set_rebuild_options
ALPHA_KINDS = ("cutoff", "base_alpha", "mode", "base_texture")          # the materials.MATERIAL_KINDS that change an alpha-relevant field
TEXTURE_WORDS = (4, 7, 8, 12, 15)       # rt_material: base colour, metallic-roughness, emissive, normal, transmission texture
MODES = ("binding", "update", "emitter")   # how a sequence keeps its light records current: rt_set_light_sources, rt_update_lights, rt_set_emitter_meshes
SIZE = (67, 45)                         # test_gpu_refit.SIZES[1]: ragged tiles
Libs = namedtuple("Libs", "inst skin morph")
_libs = None


def build(out_dir=None):
    """the CPU checkers the twin needs, compiled once per process"""
    global _libs
    if _libs is None:
        d = out_dir if out_dir is not None else tempfile.mkdtemp(prefix="scene_edits")
        _libs = Libs(instances.build(d), skin.build(d), morph.build(d))
    return _libs


def mode_of(seed):
    return MODES[seed % 3]


def kinds_of_seed(seed):
    """the alphabet a seed walks"""
    return KINDS if seed in SEEDS else KINDS_V2


def checkpoints(n):
    """the op indices after which a sequence of n ops is checked"""
    return [i for i in range(n) if (i + 1) % EVERY == 0 or i == n - 1]


Call = namedtuple("Call", "name args verdict model")      # name: the Renderer method; verdict: None (accepted) or the reason the ABI refuses the call


def finite(a):
    return bool(np.isfinite(np.asarray(a, np.float32)).all())


class Twin:
    def __init__(self, scene, mode, libs=None, wide=False):
        self.libs = libs or build()
        self.scene, self.mode, self.wide = scene, mode, wide      # wide: the sequence walks KINDS_V2 (the generator steers a few arguments, see _draw)
        self.options = (ploc.LBVH, ploc.DEFAULT_RADIUS)      # rt_set_rebuild_options in force (builder, radius); they survive build_accel
        self.ploc_buffers = False               # PLOC's buffers exist in the pool of the rebuild's working buffers
        self.tree = "host"                      # "host": host tree and host alpha records; "rebuilt": a device tree over the host's alpha records (the builder's
        #                                         table exists); "templates": rt_set_instances has put the per-mesh templates in force
        self.built_with = None                  # the options the last device build ran with; None after a host build
        self.pristine = True                    # nothing has changed the tree since the last host build: a fresh context numbers its alpha records alike
        self.drawn = {"materials": 0, "texture": 0, "rebuild_options": 0}      # how many records of a kind the generator has drawn (their arguments take turns)
        self.refuse = None                      # (call, reason or None) the generator's REFUSED record is held to (None: any)
        self._tables = None                     # materials.Tables over the scene as it is now (_tables_of); dropped by every edit of rows, texels or the table
        self.sc = refit.cornell() if scene == "cornell" else refit.street()
        d = self.sc.desc()
        self.base = refit.instances_of(d)
        self.home = self.base["objectToWorld"].copy()
        self.extent = float(max(np.abs(np.concatenate(refit.world_bounds(d, i))).max() for i in range(d.numInstances)))
        about = refit.describe(d)
        self.emissive_meshes = sorted(set(int(m) for m in self.base["primMesh"][about["emissive"]]))
        self.alpha_meshes = sorted(set(int(m) for m in self.base["primMesh"][about["alpha"]]))
        self.tris_of = refit.prim_meshes_of(d)["indexCount"] // 3
        self.vertex_count = refit.prim_meshes_of(d)["vertexCount"]
        self.skins, self.sets = [], []          # [{"sk": SkinnedMesh, "joints": matrices or None}], [{"mm": MorphedMesh, "weights": float32 array}]
        self.cap = None                         # (triangle, instance) capacity of rt_set_instances' buffers; None: the next call allocates
        self.far = set()                        # instances a "far" move has taken out of the scene
        self.emitter_moved = False
        self.tables_set = 0
        self.pose = self.sc.cameraPose()
        self.st = host.default_state(SIZE[0], SIZE[1], self.sc, None)
        self.st.environmentProb = 0.0

    # ---- what a host would upload now
    def desc(self):
        return self.sc.desc()

    def table(self):
        return refit.instances_of(self.sc.desc())

    def vertices(self):
        return skin.vertices_of(self.sc.desc())

    def emitting(self):
        return [int(i) for i in refit.describe(self.sc.desc())["emissive"]]

    def bound(self):
        """the instances a light-source binding names"""
        return sorted(set(int(i) for i in self.sc.lightSources()["instance"])) if self.mode == "binding" else []

    def skin_of(self, mesh):
        return next((s for s in self.skins if s["sk"].mesh == mesh), None)

    def set_of(self, mesh):
        return next((s for s in self.sets if s["mm"].mesh == mesh), None)

    def free_meshes(self):
        """prim meshes rt_update_vertices accepts: no skin, no morph set, at least one vertex"""
        return [m for m in range(len(self.tris_of)) if self.vertex_count[m] and not self.skin_of(m) and not self.set_of(m)]

    # ---- materials, textures and what an edit re-derives (include/rt_abi.h "Editing materials and textures")
    def material_of_mesh(self):
        """the material row of every prim mesh (an index below 0 reads row 0)"""
        return np.maximum(refit.prim_meshes_of(self.sc.desc())["materialIndex"], 0)

    def tested(self):
        """instances of the current table that take the alpha test (no RT_INST_FORCE_OPAQUE)"""
        return np.nonzero((self.table()["flags"] & instances.FORCE_OPAQUE) == 0)[0]

    def hot_materials(self):
        """materials of the alpha-tested instances: an edit of their alpha fields re-derives records"""
        m = self.material_of_mesh()
        return sorted(set(int(m[self.table()["primMesh"][i]]) for i in self.tested()))

    def lit_materials(self):
        """materials the scene's light rule calls emissive: luminance of emissiveFactor > 1e-2"""
        return [k for k, row in enumerate(blend.materials_of(self.sc.desc())) if _luminance(row) > np.float32(1e-2)]

    def deformed_materials(self):
        """materials of the prim meshes that have a skin or a morph set now"""
        m = self.material_of_mesh()
        return sorted(set(int(m[s["sk"].mesh]) for s in self.skins) | set(int(m[s["mm"].mesh]) for s in self.sets))

    def alpha_records(self, dirty):
        """rt_material_stats.alphaRecords of an edit that makes the materials `dirty` dirty: on the host's alpha records one per (instance, triangle) pair of
        their alpha-tested instances; once the templates are in force one per triangle of their prim meshes that have such an instance"""
        table, m = self.table(), self.material_of_mesh()
        mesh = [int(table["primMesh"][i]) for i in self.tested() if int(m[table["primMesh"][i]]) in dirty]
        return int(sum(int(self.tris_of[k]) for k in (sorted(set(mesh)) if self.tree == "templates" else mesh)))

    def deformable(self):
        """prim meshes the sequences bind skins and morph sets to: the meshes the deform tests use, an emissive one where the light records can follow"""
        d = self.sc.desc()
        if self.scene == "cornell":
            out = [3, 4, 0]
        else:
            out = [skin.deformed_mesh("street", instances.desc_with(d, self.base)), skin.alpha_mesh(instances.desc_with(d, self.base)), 1, 7]
        return out + (self.emissive_meshes[:1] if self.mode != "update" else [])

    def camera(self, f, W, H):
        """the orbit of test_gpu_refit.Sequence.step"""
        eye, center, up, fov = self.pose
        a = 0.06 * f
        d = np.asarray(eye, np.float64) - center
        e = center + np.array([np.cos(a) * d[0] + np.sin(a) * d[2], d[1], -np.sin(a) * d[0] + np.cos(a) * d[2]])
        self.sc.setCamera(e.astype(np.float32), center, up, fov)
        self.sc.updateCamera(W, H)
        self.st.time = 1000 + f
        return self.sc.getCamera()

    # ---- the rows of a deformed mesh: morph, then skin
    def posed_rows(self, mesh, weights=None, joints=None):
        """(rows, non-finite positions) of a mesh from its set's weights (or `weights`) and its skin's matrices (or `joints`)"""
        st, sk = self.set_of(mesh), self.skin_of(mesh)
        bad = 0
        if st is not None:
            mm = st["mm"]
            rows, bad, _ = morph.morph(self.libs.morph, mm.rest, mm.deltas, mm.target_count, mm.planes, st["weights"] if weights is None else weights)
        else:
            rows = sk["sk"].rest
        j = joints if joints is not None else (sk["joints"] if sk is not None else None)
        if sk is not None and j is not None and bad == 0:
            rows, bad = skin.pose(self.libs.skin, rows, sk["sk"].influences, j)
        return rows, bad

    # ---- set-up: what a sequence binds before its first op
    def setup(self):
        yield from self._lights_on()
        m = self.deformable()
        yield from self.calls(("rebind", {"skins": [m[0]], "morphs": [m[1]], "via_empty": False, "seed": 0}))

    def _lights_on(self):
        if self.mode == "binding":
            yield Call("set_light_sources", (self.sc.lightSources(),), None, None)
        elif self.mode == "emitter":
            meshes, rows = self.sc.emitterMeshes()
            yield Call("set_emitter_meshes", (meshes, rows, self.sc.lightWeights[0]), None, None)

    # ---- a record -> concrete calls.  A generator: the caller commits a call (Twin.commit) before it asks for the next, which reads the state that call left
    def calls(self, op):
        kind, a = op
        d = self.sc.desc()
        if kind == "update_instances":
            xf = [refit.move_matrix(k, d, i, self.extent, self.home) for i, k in zip(a["ids"], a["moves"])]
            yield self._update_instances(a["ids"], np.stack(xf) if xf else np.zeros((0, 12), np.float32), a["moves"])
        elif kind in ("rebuild_accel", "build_accel"):
            yield Call(kind, (), None, None)
        elif kind in ("set_instances", "set_emitters"):
            yield self._set_instances(self._table_for(kind, a))
        elif kind == "update_skins":
            sk = self.skins[a["skin"]]["sk"]
            yield self._update_skins([a["skin"]], sk.matrices(a["pose"], self.extent))
        elif kind == "update_morphs":
            yield self._update_morphs([a["set"]], np.asarray(a["weights"], np.float32))
        elif kind == "update_vertices":
            first, _ = skin.mesh_range(d, a["mesh"])
            rows = skin.vertices_of(d)[first + a["first"]:first + a["first"] + a["count"]].copy()
            k = np.arange(a["count"], dtype=np.float32)[:, None]
            rows["position"] += (np.asarray(a["delta"], np.float32) * (np.float32(1) + np.float32(0.01) * k)).astype(np.float32)   # as lights.positions_moved
            yield self._update_vertices(a["mesh"], a["first"], rows)
        elif kind == "rebind":
            yield from self._rebind(a)
        elif kind == "lights":
            if self.mode == "binding":
                yield Call("set_light_sources", (self.sc.lightSources(),), None, None)
            else:
                yield Call("update_lights", (), None, None)      # (the description is the twin's at the time of the call)
        elif kind == "materials":
            yield self._update_materials(a["ids"], self._rows_for(a))
            if a["kind"] == "emission" and a["scale"] != 1.0 and self.mode == "binding":      # a host that changed an emission follows with rt_update_lights, which
                yield Call("update_lights", (), None, None)                                   # leaves the binding in place (in mode "update" the checkpoint's call does)
        elif kind == "texture":
            op = self._rect_for(a)
            yield self._update_texture(op["texture"], op["x"], op["y"], op["texels"], op["pitch"])
        elif kind == "rebuild_options":
            yield self._set_rebuild_options(a["builder"], a["radius"])
        elif kind == REFUSED:
            yield self._refused(a)
        else:
            raise ValueError(kind)

    def _tables_of(self, material=None):
        """materials.Tables over the twin's scene; with `material`, over a one-row table that makes it the only material materials.draw can pick"""
        if self._tables is None:      # (a copy of every texel: made once per edit, not once per question)
            self._tables = materials.of_scene(self.sc)
        t = materials.clone_shallow(self._tables)      # the rows and texels are shared and only read; the instance rows are the twin's current ones
        t.inst = self.table()
        if material is not None:
            row = t.inst[:1].copy()
            row["primMesh"], row["flags"] = int(np.nonzero(self.material_of_mesh() == material)[0][0]), 0
            t.inst = row
        return t

    def _rows_for(self, a):
        """the rows of a `materials` record: materials.draw of the record's kind, once per id, from the record's seed"""
        rows = []
        if a["kind"] == "emission":      # not one of materials.MATERIAL_KINDS: emissiveFactor times the record's scale (inside the light rule) and a drawn roughness
            for k, m in enumerate(a["ids"]):
                row = blend.materials_of(self.sc.desc())[m].copy()
                row[blend.W_EMISSIVE] = (row[blend.W_EMISSIVE].view(np.float32) * np.float32(a["scale"])).view(np.uint32)
                row[materials.W_ROUGHNESS] = materials.f2u(np.random.default_rng([a["seed"], k]).uniform(0.05, 1.0))
                rows.append(row)
            return np.stack(rows)
        for k, m in enumerate(a["ids"]):
            op = materials.draw(self._tables_of(m), np.random.default_rng([a["seed"], k]), a["kind"])
            assert op["ids"] == [m], (op["ids"], m)
            rows.append(op["rows"][0])
        return np.stack(rows)

    def _rect_for(self, a, tables=None):
        """the rectangle of a `texture` record: materials.draw of the record's kind from the record's seed, over the tables the record's material selects"""
        op = materials.draw(tables if tables is not None else self._tables_of(a["material"]), np.random.default_rng([a["seed"], 0]), a["kind"])
        assert op["texture"] == a["texture"], (op["texture"], a)
        return op

    def _table_for(self, kind, a):
        d, cur = self.sc.desc(), self.table()
        if kind == "set_emitters":
            if self.emitting() and len(cur) - len(self.emitting()) >= 2:
                steps = emitters.sequence(d)
                return steps[a["step"] % len(steps)][1]
            return self.base.copy()      # no emitter left: the scene's own table again
        how = a["how"]
        if how == "append":
            return np.concatenate([cur, instances.placed(d, a["src"], a["move"], self.extent, np.asarray(a["shift"]) * self.extent)])
        if how == "grow":
            return np.concatenate([cur] + [instances.placed(d, a["src"], "translate", self.extent, np.array([0.02 * (k + 1), 0.01 * k, -0.015 * (k + 1)]) * self.extent)
                                           for k in range(a["count"])])
        if how == "delete":
            return np.delete(cur, a["inst"])
        if how == "shrink":
            return cur[:a["count"]].copy()
        if how == "opaque":
            t = cur.copy()
            t["flags"][a["inst"]] ^= instances.FORCE_OPAQUE
            return t
        raise ValueError(how)

    # ---- the ABI's refusal rules, restated (include/rt_abi.h); instances.verdict for tables
    def _update_instances(self, ids, xf, moves=()):
        ids = [int(i) for i in ids]
        xf = np.ascontiguousarray(xf, np.float32).reshape(-1, 12)
        why = None
        if any(i >= len(self.table()) for i in ids):
            why = "id out of range"
        elif len(set(ids)) != len(ids):
            why = "duplicate id"
        elif not finite(xf):
            why = "non-finite matrix entry"
        else:
            for m in xf:
                det = np.linalg.det(m.reshape(3, 4)[:, :3].astype(np.float64))
                if not np.isfinite(np.float32(det)) or np.float32(det) == 0:
                    why = "singular matrix"
        return Call("update_instances", (ids, xf), why, list(moves))

    def _set_instances(self, table):
        d = self.sc.desc()
        if self.mode == "emitter":      # the emitter rule gives way to the template rule, and every emissive prim mesh of these scenes has a template
            d = abi.SceneDesc.from_buffer_copy(d)
            d.trigLights = None
            d._keep = self.sc
        code, off = instances.verdict(self.libs.inst, d, table, bound=self.bound())
        t = None if table is None else instances.rows(table)
        n, tris = (0, 0) if t is None else (len(t), int(self.tris_of[t["primMesh"][t["primMesh"] < len(self.tris_of)]].sum()))
        fits = self.cap is not None and tris <= self.cap[0] and n <= self.cap[1]
        first_ploc = self.options[0] == ploc.PLOC and not self.ploc_buffers      # the first PLOC build on the working buffers allocates PLOC's own
        return Call("set_instances", (t,), None if code == instances.OK else "%s (instance %d)" % (instances.MESSAGE[code], off),
                    {"reallocates": not fits or first_ploc, "fits": fits})

    def _update_skins(self, ids, joints):
        joints = np.ascontiguousarray(joints, np.float32).reshape(-1, 12)
        why = None
        if not self.skins:
            why = "no skins"
        elif any(i >= len(self.skins) for i in ids):
            why = "skin out of range"
        elif len(set(ids)) != len(ids):
            why = "skin listed twice"
        elif not finite(joints):
            why = "non-finite matrix entry"
        rows = []
        if why is None:
            at = 0
            for i in ids:
                sk = self.skins[i]["sk"]
                j = joints[at:at + sk.joint_count]
                at += sk.joint_count
                r, bad = self.posed_rows(sk.mesh, joints=j)
                if bad:
                    why = "non-finite position"
                rows.append((i, j, r))
        return Call("update_skins", (ids, joints), why, rows)

    def _update_morphs(self, ids, weights):
        weights = np.ascontiguousarray(weights, np.float32).reshape(-1)
        why = None
        if not self.sets:
            why = "no sets"
        elif any(i >= len(self.sets) for i in ids):
            why = "set out of range"
        elif len(set(ids)) != len(ids):
            why = "set listed twice"
        elif not finite(weights):
            why = "non-finite weight"
        rows = []
        if why is None:
            at = 0
            for i in ids:
                mm = self.sets[i]["mm"]
                w = weights[at:at + mm.target_count]
                at += mm.target_count
                sk = self.skin_of(mm.mesh)
                if sk is not None and sk["joints"] is None:
                    why = "pose the skin first"
                    break
                r, bad = self.posed_rows(mm.mesh, weights=w)
                if bad:
                    why = "non-finite position"
                rows.append((i, w, r))
        return Call("update_morphs", (ids, weights), why, rows)

    def _update_vertices(self, mesh, first, rows):
        why = None
        if mesh >= len(self.tris_of):
            why = "prim mesh out of range"
        elif first + len(rows) > int(self.vertex_count[mesh]):
            why = "range outside the mesh"
        elif not finite(rows["position"]):
            why = "non-finite position"
        elif self.skin_of(mesh) or self.set_of(mesh):
            why = "the mesh has a skin or a morph set"
        else:
            at = skin.mesh_range(self.sc.desc(), mesh)[0] + first
            if self.vertices()["texcoord"][at:at + len(rows)].tobytes() != rows["texcoord"].tobytes():
                why = "texcoord bits differ"
        return Call("update_vertices", (mesh, first, rows), why, None)

    def _update_materials(self, ids, rows):
        """rt_update_materials: refused for an id out of range, an id listed twice, a texture id outside the scene's textures, a row that crosses the light rule in
        either direction, and — emitter mode on — a row that changes the luminance of an emissive material.  model: what rt_material_stats reports"""
        ids = [int(i) for i in ids]
        rows = np.ascontiguousarray(rows, np.uint32).reshape(-1, 20)
        d = self.sc.desc()
        cur = blend.materials_of(d)
        why = None
        if any(i >= len(cur) for i in ids):
            why = "id out of range"
        elif len(set(ids)) != len(ids):
            why = "id listed twice"
        else:
            for i, row in zip(ids, rows):
                tex = row[list(TEXTURE_WORDS)].view(np.int32)
                was, now = _luminance(cur[i]), _luminance(row)
                if ((tex < -1) | (tex >= int(d.numTextures))).any():
                    why = "a missing texture"
                elif (was > np.float32(1e-2)) != (now > np.float32(1e-2)):
                    why = "the row crosses the light rule"
                elif self.mode == "emitter" and was > np.float32(1e-2) and not was == now:
                    why = "emitter mode: the luminance of an emissive material changes"
                if why:
                    break
        model = None
        if why is None:      # a field changed bitwise counts
            words = list(materials.ALPHA_WORDS)
            dirty = [i for i, row in zip(ids, rows) if not np.array_equal(row[words], cur[i][words])]
            model = self._edit_model(dirty)
        return Call("update_materials", (ids, rows), why, model)

    def _update_texture(self, texture, x, y, texels, pitch=None):
        """rt_update_texture: refused for a texture outside the scene's textures, an empty rectangle, one that leaves the texture, and a pitch below 4 w"""
        t = self._tables_of()
        h, w = texels.shape[:2]
        why, model = None, None
        if texture >= len(t.tex_rows):
            why = "texture out of range"
        elif w == 0 or h == 0:
            why = "empty rectangle"
        elif x + w > t.texture_size(texture)[0] or y + h > t.texture_size(texture)[1]:
            why = "the rectangle leaves the texture"
        elif pitch is not None and pitch < 4 * w:
            why = "rowPitchBytes below 4 w"
        else:      # an alpha byte changed counts: every material whose base colour texture this is
            changed = not np.array_equal(t.texels[texture][y:y + h, x:x + w, 3], texels[..., 3])
            dirty = [int(m) for m in np.nonzero(t.mats[:, blend.W_BASE_TEXTURE].view(np.int32) == texture)[0]] if changed else []
            model = self._edit_model(dirty)
        return Call("update_texture", (texture, x, y, texels, pitch), why, model)

    def _edit_model(self, dirty):
        """what rt_material_stats reports of an accepted edit, and where the edit falls: the state of the tree, the materials of the deformed meshes, whether
        the tree is still the last host build's (the check after the edit then compares every word with a fresh context's, alphaIdx included)"""
        return {"dirty": len(dirty), "records": self.alpha_records(dirty), "materials": dirty, "state": self.tree, "deformed": self.deformed_materials(),
                "pristine": self.pristine}

    def _set_rebuild_options(self, builder, radius=0, max_iterations=0):
        """rt_set_rebuild_options: builder LBVH or PLOC, radius 0..64 (0: the default), maxIterations >= 0 (0: the default); anything else is refused"""
        why = None
        if builder not in (ploc.LBVH, ploc.PLOC):
            why = "unknown builder"
        elif not 0 <= radius <= 64:
            why = "radius outside 0..64"
        elif max_iterations < 0:
            why = "negative maxIterations"
        return Call("set_rebuild_options", (builder, radius, max_iterations), why, None)

    def options_readback(self):
        """rt_get_rebuild_options as the twin expects it: [builder, radius, maxIterations, reserved] (the sequences leave the iteration cap at its default)"""
        return [self.options[0], self.options[1], ploc.DEFAULT_MAX_ITERATIONS, 0]

    def _emissive_refused(self, meshes):
        return self.mode == "update" and any(m in self.emissive_meshes for m in meshes)      # no binding: the host could no longer supply the light records

    def _set_skins(self, meshes, joint_count, seed):
        d = self.sc.desc()
        models = [skin.SkinnedMesh(self.libs.skin, d, m, joint_count, seed + k) for k, m in enumerate(meshes)]      # the rest pose: the rows as they are now
        why = None
        if self.sets:
            why = "morph sets exist: skins first"
        elif len(set(meshes)) != len(meshes):
            why = "prim mesh listed twice"
        elif self._emissive_refused(meshes):
            why = "emissive mesh without a light-source binding"
        return Call("set_skins", skin.skins_table(models), why, models)

    def _set_morph_targets(self, meshes, targets, planes, seed):
        d = self.sc.desc()
        models = []
        for k, m in enumerate(meshes):
            mm = morph.MorphedMesh(self.libs.morph, d, m, targets, planes, seed + k, scale=0.02 * self.extent)
            sk = self.skin_of(m)
            if sk is not None:      # a mesh that has a skin uses the skin's rest pose
                mm.rest = sk["sk"].rest.copy()
            models.append(mm)
        why = None
        if len(set(meshes)) != len(meshes):
            why = "prim mesh listed twice"
        elif self._emissive_refused(meshes):
            why = "emissive mesh without a light-source binding"
        return Call("set_morph_targets", morph.sets_table(models), why, models)

    def _rebind(self, a):
        seed = int(a["seed"])
        if a["skins"] is not None:
            if self.sets:
                yield self._set_morph_targets([], 1, 0, seed)      # remove the sets, set the skins, set the sets again
            if a["via_empty"]:
                yield self._set_skins([], 1, seed)
            yield self._set_skins(a["skins"], 1 + seed % 3, seed)
        elif a["via_empty"]:
            yield self._set_morph_targets([], 1, 0, seed)
        yield self._set_morph_targets(a["morphs"], 1 + seed % 4, seed % 4, seed)

    def _refused(self, a):
        d, cur = self.sc.desc(), self.table()
        call, why = a["call"], a["why"]
        ok = cur["objectToWorld"][0:1].copy()
        bad = _spoil(ok[0], why)[None] if why in ("nan", "singular") else ok
        if call == "update_instances":
            if why == "range":
                return self._update_instances([len(cur)], ok)
            if why == "twice":
                return self._update_instances([1, 1], np.concatenate([cur["objectToWorld"][1:2]] * 2))
            return self._update_instances([0], bad)
        if call == "set_instances":
            t = cur.copy()
            if why in ("nan", "singular"):
                t["objectToWorld"][a["inst"]] = _spoil(t["objectToWorld"][a["inst"]], why)
            elif why == "prim_mesh":
                t["primMesh"][a["inst"]] = len(self.tris_of)
            elif why == "empty":
                t = t[:0]
            elif why == "emitter_moved":
                t["objectToWorld"][self.emitting()[0]][3] += np.float32(0.25)
            return self._set_instances(t)
        if call == "update_skins":
            sk = self.skins[0]["sk"]
            j = sk.matrices("bend", self.extent)
            if why == "range":
                return self._update_skins([len(self.skins)], j)
            j[0, 5] = np.inf
            return self._update_skins([0], j)
        if call == "update_morphs":
            mm = self.sets[0]["mm"]
            w = np.zeros(mm.target_count, np.float32)
            if why == "range":
                return self._update_morphs([len(self.sets)], w)
            if why == "twice":
                return self._update_morphs([0, 0], np.concatenate([w, w]))
            w[-1] = np.nan
            return self._update_morphs([0], w)
        if call == "update_vertices":
            mesh = self.skins[0]["sk"].mesh if why == "skinned" else self.free_meshes()[0]
            first, count = skin.mesh_range(d, mesh)
            rows = skin.vertices_of(d)[first:first + count].copy()
            if why == "outside":
                return self._update_vertices(mesh, 1, rows)
            if why == "nan":
                rows["position"][count // 2, 1] = np.nan
            return self._update_vertices(mesh, 0, rows)
        if call == "set_skins":
            return self._set_skins([self.free_meshes()[0]], 2, 0)      # refused while a morph set exists
        if call == "materials":
            t = self._tables_of()
            if why == "emitter_luminance":      # twice as bright: inside the light rule, refused only while the emitter mode is on
                m = self.lit_materials()[0]
                row = t.mats[m].copy()
                row[blend.W_EMISSIVE] = (row[blend.W_EMISSIVE].view(np.float32) * np.float32(2)).view(np.uint32)
                return self._update_materials([m], row.reshape(1, 20))
            op = materials.draw_refusal(t, np.random.default_rng(a["inst"]), why)
            return self._update_materials(op["ids"], op["rows"])
        if call == "texture":
            op = materials.draw_refusal(self._tables_of(), np.random.default_rng(a["inst"]), why)
            return self._update_texture(op["texture"], op["x"], op["y"], op["texels"], op["pitch"])
        if call == "rebuild_options":
            return self._set_rebuild_options(*{"builder": (2, 0, 0), "radius": (ploc.PLOC, 65, 0), "negative_radius": (ploc.PLOC, -1, 0), "iterations": (ploc.PLOC, 16, -1)}[why])
        raise ValueError(call)

    # ---- committing a call: the twin follows; returns the instances the call touched
    def commit(self, call):
        assert call.verdict is None, call.verdict
        name, d = call.name, self.sc.desc()
        if name in ("update_instances", "update_skins", "update_morphs", "update_vertices", "rebuild_accel", "set_instances"):
            self.pristine = False
        if name in ("update_materials", "update_texture", "set_instances"):
            self._tables = None
        if name in ("update_materials", "update_texture"):      # touched: the alpha-tested instances of the dirty materials, so that the next rays are aimed at them
            if name == "update_materials":
                self.sc.setMaterials(call.args[0], call.args[1])
                p, t = self.sc.lightWeights      # a changed emission changes the weight of the lights: the state a host derives from it (host.default_state)
                self.st.lightLuminIntegInv = 1.0 / (p + t) if (p + t) > 0 else float("inf")
            else:
                texture, x, y, texels, _ = call.args
                self.sc.setTexture(texture, x, y, texels)
            m, table = self.material_of_mesh(), self.table()      # (... and at the first and the last instance: the edit may have made the others invisible)
            return [int(i) for i in self.tested() if int(m[table["primMesh"][i]]) in call.model["materials"]] + [0, len(table) - 1]
        if name == "set_rebuild_options":
            self.options = (call.args[0], call.args[1] or ploc.DEFAULT_RADIUS)
            return []
        if name == "rebuild_accel":
            self.tree = "rebuilt" if self.tree == "host" else self.tree
            self.built_with = self.options
            self.ploc_buffers |= self.options[0] == ploc.PLOC
            return []
        if name == "update_instances":
            ids, xf = call.args
            self.emitter_moved |= bool(set(ids) & set(self.emitting()))
            self.sc.updateInstances(ids, xf)
            for i, k in zip(ids, call.model):
                if k == "far":
                    self.far.add(i)
                elif k == "back":
                    self.far.discard(i)
            return list(ids)
        if name == "build_accel":      # a host build drops the rebuild's working buffers (PLOC's with them) and the templates' numbering; the options stay
            self.cap = None
            self.tree, self.built_with, self.ploc_buffers, self.pristine = "host", None, False, True
            return []
        if name == "set_instances":
            old, new = self.table(), call.args[0]
            if not call.model["fits"]:
                tris = int(self.tris_of[new["primMesh"]].sum())
                self.cap = (tris + tris // 8, len(new) + len(new) // 8)
                self.ploc_buffers = False      # new working buffers
            self.ploc_buffers |= self.options[0] == ploc.PLOC
            self.tree, self.built_with = "templates", self.options
            self.sc.setInstances(new)
            self.home = new["objectToWorld"].copy()
            self.far = set()
            return instances.aim_ids(old, new)[0]
        if name == "update_skins":
            touched = []
            for i, j, rows in call.model:
                self.skins[i]["joints"] = j.copy()
                self.sc.updateVertices(self.skins[i]["sk"].mesh, 0, rows)
                touched += [int(x) for x in skin.instances_of_mesh(d, self.skins[i]["sk"].mesh)]
            return touched
        if name == "update_morphs":
            touched = []
            for i, w, rows in call.model:
                self.sets[i]["weights"] = w.copy()
                self.sc.updateVertices(self.sets[i]["mm"].mesh, 0, rows)
                touched += [int(x) for x in skin.instances_of_mesh(d, self.sets[i]["mm"].mesh)]
            return touched
        if name == "update_vertices":
            mesh, first, rows = call.args
            self.sc.updateVertices(mesh, first, rows)
            return [int(x) for x in skin.instances_of_mesh(d, mesh)]
        if name == "set_skins":
            self.skins = [{"sk": m, "joints": None} for m in call.model]
        elif name == "set_morph_targets":
            self.sets = [{"mm": m, "weights": np.zeros(m.target_count, np.float32)} for m in call.model]
        return []      # rebuild_accel, the light calls and the bindings change nothing a host would upload

    def apply(self, op):
        """commit every call of a record that the ABI accepts; returns (calls, touched instances)"""
        out, touched = [], []
        for call in self.calls(op):
            out.append(call)
            if call.verdict is None:
                touched += self.commit(call)
        return out, touched


def _luminance(row):
    """luminance of emissiveFactor of a material row (20 words) in fp32, term by term: what the scene's light rule compares with 1e-2"""
    e = np.asarray(row, np.uint32)[blend.W_EMISSIVE].view(np.float32)
    return np.float32(np.float32(e[0] * np.float32(0.2126) + e[1] * np.float32(0.7152)) + e[2] * np.float32(0.0722))


def _spoil(m, why):
    m = m.copy()
    if why == "nan":
        m[7] = np.nan
    else:
        m[0:3] = 0      # a zero row: the determinant is exactly zero in any arithmetic
    return m


# ---- the order of the kinds -----------------------------------------------------------------------------------------------------------------------------------
def _walk(rng, n, emitter, todo, kinds=KINDS, quota=None):
    """n kinds with one REFUSED among them; every step prefers a pair (previous kind, kind) that is still in `todo`, and takes it out.  quota: after that many
    pairs (or once `todo` is empty) the walk leaves the rest of `todo` to the walks drawn after it and goes on over the pairs of pairs_v2() it has not held itself"""
    allowed = [k for k in kinds if emitter or k != "set_emitters"]
    refused_at = int(rng.integers(2, max(3, n - 2)))
    shared, taken = todo, 0

    def open_from(a):
        return sum((a, b) in todo for b in allowed)

    out, prev = [], None
    for i in range(n):
        if i == refused_at:
            out.append(REFUSED)
            prev = None
            continue
        new = {b: prev is not None and (prev, b) in todo for b in allowed}
        # an open pair first; among those the ones only this sequence can hold, then a kind followed by itself (it opens nothing, so it would always lose the tie)
        score = {b: open_from(b) + (100 if new[b] else 0) + (40 if new[b] and emitter and "set_emitters" in (prev, b) else 0) + (20 if new[b] and b == prev else 0) for b in allowed}
        best = max(score.values())
        pick = [b for b in allowed if score[b] == best]
        b = pick[int(rng.integers(len(pick)))]
        if prev is not None:
            taken += (prev, b) in todo
            shared.discard((prev, b))
            todo.discard((prev, b))
            if quota is not None and (taken >= quota or not shared) and todo is shared:      # from here on the pairs of its own that this walk has not held yet
                todo = {p for p in pairs_v2() if all(k in allowed for k in p)} - set(zip(out, out[1:] + [b]))
        out.append(b)
        prev = b
    return out


_plans = {}


def _default_plans(n, salt):
    """the default sequences drawn together, the emitter-mode ones first: only they can hold the pairs with set_emitters, half of them each"""
    todo = {(a, b) for a in KINDS for b in KINDS}
    slots = sorted(((sc, sd) for sc in SCENES for sd in SEEDS), key=lambda s: (mode_of(s[1]) != "emitter", SCENES.index(s[0]), s[1]))
    later = {p for p in todo if "set_emitters" in p and (KINDS.index(p[0]) > 4 or KINDS.index(p[1]) > 4)}
    plans = {}
    for k, s in enumerate(slots):
        if k == 0:
            todo -= later
        plans[s] = _walk(np.random.default_rng([n, SCENES.index(s[0]), s[1], salt]), n, mode_of(s[1]) == "emitter", todo)
        if k == 0:
            todo |= later
    return plans, todo


SALT_V2 = 0      # where the wider family's search for a tie-break salt starts: the first start whose sequences meet every coverage condition of
#                  tests/test_scene_edits_cpu.py (edits in each state of the tree, on a deformed mesh, under each builder ...), which looking at pairs alone does not give


def pairs_v2():
    """what the wider family has to cover: the 69 ordered pairs of KINDS_V2 with a new kind on at least one side"""
    return {(a, b) for a in KINDS_V2 for b in KINDS_V2 if a in NEW_KINDS or b in NEW_KINDS}


def _default_plans_v2(n, salt):
    """the default sequences of the wider alphabet (SCENES x SEEDS_V2) drawn together, the emitter-mode ones first, over pairs_v2()"""
    todo = pairs_v2()
    slots = sorted(((sc, sd) for sc in SCENES for sd in SEEDS_V2), key=lambda s: (mode_of(s[1]) != "emitter", SCENES.index(s[0]), s[1]))
    share = -(-len(todo) // len(slots))      # each walk but the last takes its share of the pairs and then goes on with pairs of its own: every sequence is dense in new kinds
    plans = {s: _walk(np.random.default_rng([n, SCENES.index(s[0]), s[1], salt]), n, mode_of(s[1]) == "emitter", todo, KINDS_V2, share if k + 1 < len(slots) else n)
             for k, s in enumerate(slots)}
    return plans, todo


def kinds_of(scene, seed, n):
    """the order of the kinds of one sequence"""
    if seed in SEEDS_V2:
        if ("v2", n) not in _plans:      # as below, over the wider family
            best = None
            for salt in range(SALT_V2, SALT_V2 + 64):
                plans, left = _default_plans_v2(n, salt)
                if best is None or len(left) < len(best[1]):
                    best = (plans, left)
                if not left:
                    break
            _plans[("v2", n)] = best[0]
        return list(_plans[("v2", n)][(scene, seed)])
    if seed not in SEEDS:
        return _walk(np.random.default_rng([n, SCENES.index(scene), seed]), n, mode_of(seed) == "emitter", {(a, b) for a in KINDS_V2 for b in KINDS_V2}, KINDS_V2)
    if n not in _plans:      # the first tie-break salt that leaves no pair open (or, for a short n, the one that leaves the fewest)
        best = None
        for salt in range(64):
            plans, left = _default_plans(n, salt)
            if best is None or len(left) < len(best[1]):
                best = (plans, left)
            if not left:
                break
        _plans[n] = best[0]
    return list(_plans[n][(scene, seed)])


# ---- the arguments --------------------------------------------------------------------------------------------------------------------------------------------
def _draw(kind, t, rng):
    """symbolic arguments of one record against the twin's state; a REFUSED record's call fails its verdict, every other record's calls pass"""
    cur = t.table()
    n = len(cur)
    pick = lambda seq: seq[int(rng.integers(len(seq)))]      # noqa: E731
    if kind == "update_instances":
        size = int(pick([0, 1, 1, 2, 2, 3]))
        ids = sorted(int(i) for i in rng.choice(n, min(size, n), replace=False))
        em = t.emitting()
        if em and size and (not t.emitter_moved or rng.random() < 0.3) and em[0] not in ids:      # an emitter moves, once per sequence at least: its light records follow
            ids = sorted(ids[:-1] + [em[0]])
        moves = []
        for i in ids:
            k = "back" if i in t.far and rng.random() < 0.7 else pick(refit.MOVES)
            if k == "far" and (i in t.far or len(t.far) >= 1):
                k = "rotate"
            moves.append(k)
        return {"ids": ids, "moves": moves}
    if kind in ("rebuild_accel", "build_accel", "lights"):
        return {}
    if kind == "set_instances":
        plain = [i for i in range(n) if int(cur["primMesh"][i]) not in t.emissive_meshes and t.tris_of[cur["primMesh"][i]] <= 64]
        alpha = [i for i in range(n) if int(cur["primMesh"][i]) in t.alpha_meshes]
        steer = t.wide and not len(t.tested())      # no instance takes the alpha test (Cornell as loaded): a flip clears RT_INST_FORCE_OPAQUE of a non-emitter first
        if steer:
            alpha = [i for i in range(n) if int(cur["primMesh"][i]) not in t.emissive_meshes]
        room = (t.cap[1] - n + 1) if t.cap is not None else 2
        variants = [{"how": "append", "src": pick(plain), "move": pick(("mirror", "scale", "rotate")), "shift": [round(float(x), 3) for x in rng.uniform(-0.15, 0.15, 3)]},
                    {"how": "delete", "inst": max(i for i in range(n) if int(cur["primMesh"][i]) not in t.emissive_meshes)},      # the last non-emitter
                    {"how": "grow", "src": pick(plain), "count": int(max(2, room))},
                    {"how": "shrink", "count": len(t.base) if n > len(t.base) else n - 1}]
        if alpha:
            variants.append({"how": "opaque", "inst": pick(alpha)})
        turn = SCENES.index(t.scene) + 2 * MODES.index(t.mode) + 3 * t.tables_set      # the ways take turns, so that a few sequences use all of them
        t.tables_set += 1
        order = [(turn + k) % len(variants) for k in range(len(variants))]
        if n > len(t.base) + 10:      # large enough: shrink first
            order = [3] + [k for k in order if k not in (0, 2, 3)] + [0]
        if steer:
            order = [4] + [k for k in order if k != 4]
        for k in order:
            a = variants[k]
            if (a["how"] == "shrink" and a["count"] < 1) or (a["how"] == "grow" and n + a["count"] > len(t.base) + 16):
                continue
            if t._set_instances(t._table_for(kind, a)).verdict is None:
                return a
        return variants[0]
    if kind == "set_emitters":
        return {"step": int(rng.integers(0, 9))}
    if kind == "update_skins":
        k = int(rng.integers(len(t.skins)))
        return {"skin": k, "pose": pick([p for p in skin.POSES if p != "far" or not t.far])}
    if kind == "update_morphs":
        ready = [k for k, s in enumerate(t.sets) if t.skin_of(s["mm"].mesh) is None or t.skin_of(s["mm"].mesh)["joints"] is not None]
        k = pick(ready)
        tc = t.sets[k]["mm"].target_count
        how = int(rng.integers(4))
        if how == 0:
            w = [0.0] * tc                                    # no active target: the rest pose
        elif how == 1:
            w = [0.0] * tc                                    # a single active target
            w[int(rng.integers(tc))] = round(float(rng.uniform(-1.2, 1.5)), 3)
        else:
            w = [round(float(x), 3) for x in rng.uniform(-1.0, 1.5, tc)]
            if tc > 1 and how == 3:
                w[0] = -0.0
        return {"set": k, "weights": w}
    if kind == "update_vertices":
        used = sorted(set(int(m) for m in cur["primMesh"]))
        free = [m for m in t.free_meshes() if m in used]
        small = [m for m in free if t.vertex_count[m] <= 100] or free
        m = pick(small)
        vc = int(t.vertex_count[m])
        first = int(rng.integers(0, max(1, vc // 2)))
        count = int(rng.integers(1, vc - first + 1))
        return {"mesh": m, "first": first, "count": count, "delta": [round(float(x) * t.extent, 4) for x in rng.uniform(-0.03, 0.03, 3)]}
    if kind == "rebind":
        cand = t.deformable()
        seed = int(rng.integers(1, 1000))
        via_empty = bool(rng.integers(2))
        if rng.random() < 0.5:      # the skins move to other meshes (one or two); the sets go to meshes without an unposed skin
            skins = [int(m) for m in rng.choice(cand, int(rng.integers(1, 3)), replace=False)]
            morphs = [pick([m for m in cand if m not in skins])]
            return {"skins": skins, "morphs": morphs, "via_empty": via_empty, "seed": seed}
        ok = [m for m in cand if t.skin_of(m) is None or t.skin_of(m)["joints"] is not None]
        posed = [m for m in ok if t.skin_of(m) is not None]
        morphs = [pick(posed)] if posed and rng.random() < 0.6 else [pick(ok)]      # on a posed skin: morph, then skin
        if len(ok) > 1 and rng.random() < 0.4:
            morphs.append(pick([m for m in ok if m not in morphs]))
        return {"skins": None, "morphs": morphs, "via_empty": via_empty, "seed": seed}
    if kind in NEW_KINDS:      # their arguments take turns, from a start that differs per sequence, so that a few sequences reach every variant
        turn = 3 * SCENES.index(t.scene) + MODES.index(t.mode) + t.drawn[kind]
        t.drawn[kind] += 1
        lit = t.lit_materials()
        hot = [m for m in t.hot_materials() if m not in lit]
    if kind == "materials" and lit and t.drawn[kind] % 4 == 2:      # every fourth record, from the second on, changes an emission without crossing the light rule: the
        # emitter mode accepts the row only while the luminance keeps its bits (scale 1: the roughness alone changes)
        a = {"kind": "emission", "ids": [lit[0]], "seed": int(rng.integers(1, 1 << 20)), "scale": 1.0 if t.mode == "emitter" else float(pick([0.5, 1.5, 2.0]))}
        if t._update_materials(a["ids"], t._rows_for(a)).verdict is not None:      # (dimmed down to the light rule: brighter instead)
            a["scale"] = 2.0
        return a
    if kind == "materials":
        mk = materials.MATERIAL_KINDS[turn % len(materials.MATERIAL_KINDS)]
        mats = blend.materials_of(t.sc.desc())
        plain = [m for m in hot if mats[m, blend.W_ALPHA_MODE] == blend.ALPHA_OPAQUE]
        if hot and len(plain) == len(hot):      # every alpha-tested instance still has an OPAQUE material (Cornell after its flip): the first edit gives one a MASK
            mk, hot = "mode", plain
        cold = [m for m in sorted(set(int(m) for m in t.material_of_mesh())) if m not in lit and m not in hot]
        ids = [pick(hot)] if hot and (mk in ALPHA_KINDS or not cold or rng.random() < 0.5) else [pick(cold)]
        rest = [m for m in hot + cold if m not in ids]
        if rest and rng.random() < 0.35:
            ids.append(pick(rest))
        return {"kind": mk, "ids": ids, "seed": int(rng.integers(1, 1 << 20))}
    if kind == "texture":
        rk = materials.RECT_KINDS[turn % len(materials.RECT_KINDS)]
        mats = blend.materials_of(t.sc.desc())
        textured = [m for m in hot if mats[m, blend.W_BASE_TEXTURE].view(np.int32) >= 0]
        material = pick(textured) if textured and rng.random() < 0.8 else None      # mostly a texture whose alpha an alpha-tested instance reads
        seed = int(rng.integers(1, 1 << 20))
        op = materials.draw(t._tables_of(material), np.random.default_rng([seed, 0]), rk)
        return {"kind": rk, "texture": int(op["texture"]), "material": material, "seed": seed}
    if kind == "rebuild_options":      # always the other builder, so every record switches
        return {"builder": ploc.LBVH if t.options[0] == ploc.PLOC else ploc.PLOC, "radius": int(ploc.RADII[turn % len(ploc.RADII)])}
    if kind == REFUSED:
        cases = [("update_instances", w) for w in ("range", "twice", "nan", "singular")] + [("set_instances", w) for w in ("nan", "singular", "prim_mesh", "empty")] + \
                [("update_skins", w) for w in ("range", "nan")] + [("update_morphs", w) for w in ("range", "twice", "nan")] + \
                [("update_vertices", w) for w in ("outside", "nan", "skinned")] + [("set_skins", "morphs_exist")]
        if t.wide:
            cases += [("materials", w) for w in ("id_range", "duplicate", "bad_texture", "light_rule_on", "light_rule_off", "emitter_luminance")] + \
                     [("texture", w) for w in ("texture_range", "empty_rect", "rect_outside", "pitch")] + \
                     [("rebuild_options", w) for w in ("builder", "radius", "negative_radius", "iterations")]
        if t.mode != "emitter" and t.emitting():
            cases.append(("set_instances", "emitter_moved"))
        if t.refuse:      # (the default street sequences of the wider family: one per new call, so that the six hold a refusal of each)
            cases = [c for c in cases if c[0] == t.refuse[0] and t.refuse[1] in (None, c[1])]
        for k in rng.permutation(len(cases)):
            a = {"call": cases[int(k)][0], "why": cases[int(k)][1], "inst": int(rng.integers(n))}
            if t._refused(a).verdict is not None:
                return a
    raise ValueError(kind)


_ops = {}


def twin_of(scene, seed):
    """the twin a sequence starts from, before its set-up"""
    t = Twin(scene, mode_of(seed), wide=seed not in SEEDS)
    if seed in SEEDS_V2 and scene == "street":      # one refusal of each new call; the emitter-mode sequence holds the refusal only that mode has
        t.refuse = {"update": ("texture", None), "emitter": ("materials", "emitter_luminance"), "binding": ("rebuild_options", None)}[t.mode]
    return t


def ops(scene, seed, n=OPS):
    """the records of one sequence: [(kind, args)]"""
    key = (scene, seed, n)
    if key not in _ops:
        rng = np.random.default_rng([SCENES.index(scene), seed, n, 8])
        t = twin_of(scene, seed)
        for call in t.setup():
            t.commit(call)
        out = []
        for kind in kinds_of(scene, seed, n):
            op = (kind, _draw(kind, t, rng))
            t.apply(op)
            out.append(op)
        _ops[key] = out
    return [(k, dict(a)) for k, a in _ops[key]]


def replay(scene, seed, n=OPS, records=None):
    """(twin before its set-up, the records): what a runner starts from.  `records`: these instead of the generated ones (a hand-written sequence)"""
    return twin_of(scene, seed), ops(scene, seed, n) if records is None else [(k, dict(a)) for k, a in records]


def touched_or_ends(touched, count):
    """the instances the rays of a checkpoint are aimed at: the ones touched since the last checkpoint (at most 8), else the first and the last"""
    ids = [i for i in dict.fromkeys(touched) if i < count][:8]
    return ids or [0, count - 1]


def aimed_rays(desc, touched, seed, f):
    """(the instances aimed at, instances.RAYS rays) of checkpoint f of a sequence"""
    ids = touched_or_ends(touched, desc.numInstances)
    return ids, refit.make_rays(desc, ids, instances.RAYS, 100 * seed + f)


# ---- the oracle's frames of a sequence --------------------------------------------------------------------------------------------------------------------
_frames = {}


def oracle_frames(scene, seed, n=OPS, records=None, forget=()):
    """[{buffer: bytes}] per checkpoint: the oracle is given twin.desc() before each frame, as test_gpu_refit.Sequence.oracle_frames does.  `records` / `forget`: a
    hand-written sequence, and the indices of its records that the twin does not follow (tests/test_gpu_scene_edits.py, the forgetful drivers); not kept"""
    from helpers import frame_buffers
    from oracle.binding import Oracle
    key = (scene, seed, n)
    if key not in _frames or records is not None:
        W, H = SIZE
        t, records_ = replay(scene, seed, n, records)
        for call in t.setup():
            t.commit(call)
        o = Oracle(0)
        o.upload_scene(t.desc())
        o.resize(W, H)
        out, marks = [], checkpoints(len(records_))
        for i, op in enumerate(records_):
            if i not in forget:
                t.apply(op)
            if i in marks:
                f = len(out)
                cam = t.camera(f, W, H)
                o.upload_scene(t.desc())
                o.set_camera(cam)
                o.render_frame(t.st, f)
                out.append({b: o.readback(b).copy() for b in frame_buffers(f)})
        if records is not None:
            return out
        _frames[key] = out
    return _frames[key]
