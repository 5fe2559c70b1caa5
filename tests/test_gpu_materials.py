"""rt_update_materials / rt_update_texture on the GPU: after every edit the leaf records, the alpha records, the micro-maps, rays and frames equal
those of a fresh context that uploaded and built the edited description (or of the oracle rendering it from the carried-over history), word for word; every
micro-map the kernels wrote equals rt_opacity_map of its alpha record; the edits commute with rt_rebuild_accel, rt_update_instances and rt_set_instances; refused
calls change nothing.  No tolerance anywhere: results are a function of the scene, never of the tree or of which reference owned a record.
tests/test_materials_cpu.py proves the reference function and the edge scene's inputs without a GPU."""
import ctypes as C
import numpy as np
import pytest

from helpers import abi, frame_buffers
from oracle.binding import Oracle
import blend
import instances
import materials
import optin
import refit
import test_gpu_refit

pytestmark = pytest.mark.gpu

SIZES = test_gpu_refit.SIZES
renderer = test_gpu_refit.renderer
BOTH = (abi.TRAVERSAL_THROUGHPUT, abi.TRAVERSAL_LATENCY)


# ---- what a context derived, by triangle ------------------------------------------------------------------------------------------------------------------------
def derived(r):
    """(globalId, flags, omm, alpha record) of every triangle of a context, by globalId: the references of one triangle agree among themselves, and alphaIdx is
    followed into the alpha records, so two contexts that number their records differently compare equal"""
    recs = r.accel_readback(abi.ACCEL_TRIS).view(refit.REC_DT)
    alpha = r.accel_readback(abi.ACCEL_ALPHA).view(abi.ALPHA_REC_DT)
    order = np.argsort(recs["globalId"], kind="stable")
    recs = recs[order]
    same = recs["globalId"][1:] == recs["globalId"][:-1]
    assert (recs["omm"][1:][same] == recs["omm"][:-1][same]).all() and (recs["alphaIdx"][1:][same] == recs["alphaIdx"][:-1][same]).all()
    recs = recs[np.concatenate([[True], ~same])]
    assert ((recs["alphaIdx"] != 0) == ((recs["flags"] & 1) == 0)).all()
    return recs["globalId"], recs["flags"] & ~np.uint32(refit.TRI_FLIP), recs["omm"], alpha[recs["alphaIdx"]]


def diff_derived(a, b):
    return {"ids": int((a[0] != b[0]).sum()), "flags": int((a[1] != b[1]).sum()), "omm": int((a[2] != b[2]).any(axis=1).sum()),
            "alpha": optin.words(a[3].view(np.uint8), b[3].view(np.uint8))}


SAME = {"ids": 0, "flags": 0, "omm": 0, "alpha": 0}


def diff_words(r, fresh):
    """the leaf records and the alpha records of two contexts with the same tree, word for word, alphaIdx included"""
    return {"records": optin.words(r.accel_readback(abi.ACCEL_TRIS), fresh.accel_readback(abi.ACCEL_TRIS)),
            "alpha": optin.words(r.accel_readback(abi.ACCEL_ALPHA), fresh.accel_readback(abi.ACCEL_ALPHA))}


def maps_equal_the_host_function(r, t):
    """every alpha-tested triangle's omm equals rt_opacity_map of its own alpha record; returns how many were checked"""
    from restir_amd.renderer import Renderer
    _, flags, omm, alpha = derived(r)
    n = 0
    for fl, o, a in zip(flags, omm, alpha):
        if fl & 1:      # an opaque triangle: record 0
            continue
        tex = None if a["texture"] == 0xffffffffffffffff else int(a["texture"])
        want = Renderer.opacity_map(a["uv"], a["baseAlpha"], a["cutoff"], int(a["alphaMode"]), None if tex is None else t.texels[tex], int(a["wrapS"]), int(a["wrapT"]),
                                    int(a["filter"]))
        assert np.array_equal(o, want), (n, a, o, want)
        n += 1
    return n


def same_rays(r, fresh, rays):
    for mode in BOTH:
        r.set_traversal(mode); fresh.set_traversal(mode)
        a, b = r.trace_closest(rays), fresh.trace_closest(rays)
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), mode      # (distance, globalId, u, v: nothing of the tree)
        assert np.array_equal(r.trace_any(rays), fresh.trace_any(rays)), mode
    return a


def edit(r, t, kind_or_op, **kw):
    """one material edit on the context and on the tables"""
    op = kind_or_op if isinstance(kind_or_op, dict) else {"kind": kind_or_op, **kw}
    assert materials.issue(r, op) is None
    materials.apply(t, op)
    return r.material_stats()


def row(t, m, **words):
    out = t.mats[m].copy()
    for k, v in words.items():
        w = {"cutoff": blend.W_ALPHA_CUTOFF, "base": blend.W_BASE_ALPHA, "mode": blend.W_ALPHA_MODE, "texture": blend.W_BASE_TEXTURE, "rough": materials.W_ROUGHNESS}[k]
        out[w] = materials.f2u(v) if k in ("cutoff", "base", "rough") else np.array([v], np.int32).view(np.uint32)[0]
    return out


def tris_of_materials(t, mats):
    return sum(1 for m, _, _ in materials.triangle_inputs(t) if m in mats)


# ---- 1. the edge scene on a host-built tree ---------------------------------------------------------------------------------------------------------------------
EDGE_EDITS = [([1], dict(cutoff=0.9)), ([1], dict(cutoff=0.1)), ([6], dict(base=0.6)), ([3], dict(mode=blend.ALPHA_MASK)), ([4], dict(texture=materials.T_ODD)),
              ([2], dict(texture=-1)), ([5], dict(base=1.0)), ([1, 7], dict(cutoff=0.5, base=0.3))]


def test_edge_scene_edits_equal_a_fresh_context_word_for_word():
    t = materials.edge()
    r = renderer(t.desc())
    checked = 0
    for ids, words in EDGE_EDITS:
        st = edit(r, t, "cutoff", ids=ids, rows=np.stack([row(t, m, **words) for m in ids]))
        fresh = renderer(t.desc())
        diff = diff_words(r, fresh)
        fresh.destroy()
        print(ids, words, diff, "records", st.alphaRecords, "leaves", st.leafRecords, "texels", st.texelsScanned, "ms", round(st.ms, 3))
        assert diff == {"records": 0, "alpha": 0}, (ids, words)
        n = tris_of_materials(t, ids)
        assert (st.materialsWritten, st.dirtyMaterials, st.alphaRecords) == (len(ids), len(ids), n) and st.leafRecords >= n
        checked += maps_equal_the_host_function(r, t)
    assert checked == 30 * len(EDGE_EDITS)
    r.destroy()


# ---- 2. templates in force ----------------------------------------------------------------------------------------------------------------------------------------
def test_templates_follow_an_edit_and_later_tables_are_made_from_the_edited_rows():
    sc = refit.street()
    t = materials.of_scene(sc)
    desc = t.desc()
    about, pm = refit.describe(desc), refit.prim_meshes_of(desc)
    leaf_inst = int(about["alpha"][0])
    leaf_mesh = int(t.inst["primMesh"][leaf_inst])
    leaf = t.material_of_mesh(leaf_mesh)
    r = renderer(desc)
    r.set_instances(t.inst)                                        # the templates are in force
    st = edit(r, t, "cutoff", ids=[leaf], rows=row(t, leaf, cutoff=0.85, base=0.9).reshape(1, 20))
    live = set(int(m) for m in t.inst["primMesh"][(t.inst["flags"] & materials.FORCE_OPAQUE) == 0] if t.material_of_mesh(m) == leaf)
    assert st.dirtyMaterials == 1 and st.alphaRecords == sum(int(pm["indexCount"][m]) // 3 for m in live)      # one template per triangle of a mesh, however many instances
    # one more instance of the edited mesh, and one of a mesh whose templates were never made (so far it has force-opaque instances only)
    made = set(int(m) for m in t.inst["primMesh"][(t.inst["flags"] & materials.FORCE_OPAQUE) == 0])
    emissive = set(int(m) for m in t.inst["primMesh"][about["emissive"]])
    other = next(i for i in range(len(t.inst)) if int(t.inst["primMesh"][i]) not in made | emissive and pm["indexCount"][t.inst["primMesh"][i]] > 0)
    new = t.inst[[leaf_inst, other]].copy()
    new["objectToWorld"][:, 3] += np.float32(0.4)
    new["flags"] &= ~np.uint32(materials.FORCE_OPAQUE)
    table = np.concatenate([t.inst, new])
    edit(r, t, "set_instances", table=table)
    fresh = renderer(t.desc())
    a, b = derived(r), derived(fresh)
    assert diff_derived(a, b) == SAME
    # the alphaIdx formula: the prim mesh's first template + the triangle + 1
    recs = r.accel_readback(abi.ACCEL_TRIS).view(refit.REC_DT)
    ref = refit.tri_ref(t.desc())[recs["globalId"]]
    base = np.concatenate([[0], np.cumsum(pm["indexCount"] // 3)])[:-1]
    want = np.where(recs["flags"] & 1, 0, base[t.inst["primMesh"][ref[:, 0]]] + ref[:, 1] + 1)
    assert np.array_equal(recs["alphaIdx"], want.astype(np.uint32))
    ids = [leaf_inst, len(table) - 2, len(table) - 1]
    hit = instances.informative(t.desc(), same_rays(r, fresh, refit.make_rays(t.desc(), ids, 4096, 12)), ids, ids)
    print("rays", hit)
    assert hit[2] >= 20
    r.destroy(); fresh.destroy()


# ---- 3. rays --------------------------------------------------------------------------------------------------------------------------------------------------------
def test_rays_after_a_cutoff_that_closes_cells_and_one_that_opens_them():
    t = materials.edge()
    r = renderer(t.desc())
    closed = None
    for cutoff in (0.9, 0.1):      # 0.9 closes the bands of 160 and 90 (opacity below the cutoff), 0.1 opens them
        edit(r, t, "cutoff", ids=[1, 2], rows=np.stack([row(t, 1, cutoff=cutoff), row(t, 2, cutoff=cutoff)]))
        fresh = renderer(t.desc())
        ids = [int(i) for i in t.alpha_instances([1, 2])]
        rays = refit.make_rays(t.desc(), ids, 4096, 11)
        hits, aimed, on_edited = instances.informative(t.desc(), same_rays(r, fresh, rays), ids, ids)
        print("cutoff", cutoff, "rays that hit", hits, "on edited materials", on_edited)
        assert on_edited >= 20
        closed = on_edited if closed is None else closed
        fresh.destroy()
    assert on_edited > closed      # more of the edited triangles stop rays once their cells are open
    r.destroy()


def look_at_leaves(sc, desc, W, H):
    """(the last alpha-tested tree instance, its material): the scene's camera goes a little more than one tree size away from its crown, looking at it (from
    the scene's own pose the trees are a few pixels)"""
    i = int(refit.describe(desc)["alpha"][-1])
    lo, hi = refit.world_bounds(desc, i)
    c, size = 0.5 * (lo + hi), float((hi - lo).max())
    _, _, up, fov = sc.cameraPose()
    sc.setCamera((c + size * np.array([-1.2, 0.1, 0.2])).astype(np.float32), c.astype(np.float32), up, fov)
    sc.updateCamera(W, H)
    pm, inst = refit.prim_meshes_of(desc), refit.instances_of(desc)
    return i, max(0, int(pm["materialIndex"][inst["primMesh"][i]]))


# ---- 4. frames ------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", SIZES, ids=["%dx%d" % s for s in SIZES])
def test_frames_with_an_edit_before_each_of_the_last_three_equal_the_oracle(size):
    """two frames as uploaded, then one edit before each further frame: roughness only (2), texels whose alpha bytes stay (3), the alpha parameters (4).  Every
    frame equals the oracle rendering the edited description from the carried-over history, and each edit by itself changes its frame: per edit one more oracle
    stays a step behind, with the same history and every earlier edit but not this one"""
    W, H = size
    sc = refit.street()
    t = materials.of_scene(sc)
    desc = t.desc()
    _, leaf = look_at_leaves(sc, desc, W, H)
    tex = int(t.mats[leaf, blend.W_BASE_TEXTURE].view(np.int32))
    assert tex >= 0
    st = blend.state(sc, W, H)
    r = renderer(desc, W, H, overlap=0)
    o, behind = Oracle(0), {2: Oracle(0), 3: Oracle(0), 4: Oracle(0)}
    for x in [o] + list(behind.values()):
        x.upload_scene(desc); x.resize(W, H)
    differs = {}
    for f in range(5):
        if f == 2:      # nothing is re-derived, the frame changes
            ms = edit(r, t, "roughness", ids=[leaf], rows=row(t, leaf, rough=0.05).reshape(1, 20))
            assert (ms.materialsWritten, ms.dirtyMaterials, ms.alphaRecords, ms.leafRecords, ms.texelsScanned) == (1, 0, 0, 0, 0)
        if f == 3:      # the colours of the whole leaf texture change, every alpha byte stays: nothing is launched, the frame changes
            texels = t.texels[tex].copy()
            texels[..., :3] = 255 - texels[..., :3]
            ms = edit(r, t, "same_alpha", texture=tex, x=0, y=0, texels=texels, pitch=None)
            assert (ms.dirtyMaterials, ms.alphaRecords, ms.leafRecords, ms.texelsScanned) == (0, 0, 0, 0) and ms.bytesUploaded == texels.size
        if f == 4:      # base alpha x texel falls below the cutoff everywhere, the micro-maps say so, the leaves are gone
            ms = edit(r, t, "cutoff", ids=[leaf], rows=row(t, leaf, cutoff=0.5, base=0.4).reshape(1, 20))
            assert ms.alphaRecords > 0 and ms.leafRecords >= ms.alphaRecords
        if f >= 2:
            for x in [o] + [behind[k] for k in behind if k > f]:
                x.upload_scene(t.desc())      # (an oracle keeps its history across an upload)
        st.time = 1000 + f
        cam = blend.rest_camera(sc, W, H)
        r.set_camera(cam); r.run(st, f)
        for x in [o] + [behind[k] for k in behind if k >= f]:
            x.set_camera(cam); x.render_frame(st, f)
        got = {b: r.readback(b) for b in frame_buffers(f)}
        bad = {abi.BUFFER_NAMES[b]: optin.words(got[b], o.readback(b)) for b in got}
        assert not any(bad.values()), (f, bad)
        if f >= 2:
            differs[f] = sum(optin.words(got[b], behind[f].readback(b)) for b in got)
    print(size, "words that differ from the frame without the edit: roughness, texel colours, alpha:", differs)
    assert all(differs[f] > 0 for f in (2, 3, 4)), differs
    r.destroy()


def test_a_frame_after_each_rectangle_kind_equals_the_oracle():
    """the texels of the leaf texture, colours and alpha, through every rectangle kind — one texel, full width, the last row, the last column, a padded pitch — one
    frame after each against the oracle that uploaded the edited texture; the larger rectangles are in view and change the frame"""
    W, H = SIZES[1]
    sc = refit.street()
    t = materials.of_scene(sc)
    desc = t.desc()
    _, leaf = look_at_leaves(sc, desc, W, H)
    tex = int(t.mats[leaf, blend.W_BASE_TEXTURE].view(np.int32))
    w, h = t.texture_size(tex)
    assert tex >= 0 and w >= 8 and h >= 8
    st = blend.state(sc, W, H)
    r = renderer(desc, W, H, overlap=0)
    o, behind = Oracle(0), Oracle(0)
    for x in (o, behind):
        x.upload_scene(desc); x.resize(W, H)
    rng = np.random.default_rng(9)
    rects = {"one": (w // 2, h // 2, 1, 1), "full_width": (0, h // 4, w, h // 2), "last_row": (w // 5, h - 1, w // 2, 1), "last_column": (w - 1, h // 5, 1, h // 2),
             "padded": (w // 3, h // 3, w // 3 + 1, h // 3 + 1)}
    differs = {}
    for f, kind in enumerate(materials.RECT_KINDS[:5]):
        x0, y0, rw, rh = rects[kind]
        texels = rng.integers(0, 256, (rh, rw, 4), dtype=np.uint8)
        texels[..., 3] = rng.choice([0, 255], (rh, rw))
        ms = edit(r, t, kind, texture=tex, x=x0, y=y0, texels=texels, pitch=4 * rw + 12 if kind == "padded" else None)
        assert ms.bytesUploaded >= texels.size
        o.upload_scene(t.desc())
        st.time = 1000 + f
        cam = blend.rest_camera(sc, W, H)
        r.set_camera(cam); r.run(st, f)
        for x in (o, behind):
            x.set_camera(cam); x.render_frame(st, f)
        got = {b: r.readback(b) for b in frame_buffers(f)}
        bad = {abi.BUFFER_NAMES[b]: optin.words(got[b], o.readback(b)) for b in got}
        assert not any(bad.values()), (kind, bad)
        differs[kind] = sum(optin.words(got[b], behind.readback(b)) for b in got)      # (behind: the scene as uploaded, its own history)
    print("words that differ from the unedited scene's frames:", differs)
    assert differs["full_width"] > 0 and differs["padded"] > 0
    r.destroy()


# ---- 5. the edits commute with the other edits ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("builder", [abi.REBUILD_LBVH, abi.REBUILD_PLOC], ids=["lbvh", "ploc"])
def test_an_edit_and_a_device_rebuild_commute(builder):
    t = materials.edge()
    rows = np.stack([row(t, 1, cutoff=0.9), row(t, 6, base=0.7, mode=blend.ALPHA_MASK)])
    trees = []
    for order in ("edit first", "rebuild first", "rebuild, edit, rebuild"):
        k = materials.clone(t)
        r = renderer(k.desc())
        r.set_rebuild_options(builder)
        if order != "edit first":
            r.rebuild_accel()
        edit(r, k, "cutoff", ids=[1, 6], rows=rows)
        if order != "rebuild first":
            r.rebuild_accel()
        trees.append((order, r, k))
    fresh = renderer(trees[0][2].desc())
    fresh.set_rebuild_options(builder)
    fresh.rebuild_accel()
    for order, r, k in trees:
        diff = dict(diff_words(r, fresh), nodes=optin.words(r.accel_readback(abi.ACCEL_NODES), fresh.accel_readback(abi.ACCEL_NODES)))
        assert diff == {"records": 0, "alpha": 0, "nodes": 0}, order
        assert maps_equal_the_host_function(r, k) == 30
        r.destroy()
    fresh.destroy()


def test_an_edit_and_an_instance_move_commute():
    t = materials.edge()
    rows = np.stack([row(t, 2, cutoff=0.1), row(t, 3, base=1.5)])
    ids = [0, 2]
    xf = np.stack([refit.compose(refit.translation([0.3, -0.2, 0.1]), t.inst["objectToWorld"][i]) for i in ids]).astype(np.float32)
    done = []
    for order in ("edit first", "move first"):
        k = materials.clone(t)
        r = renderer(k.desc())
        for step in (("edit", "move") if order == "edit first" else ("move", "edit")):
            if step == "edit":
                edit(r, k, "cutoff", ids=[2, 3], rows=rows)
            else:
                r.update_instances(ids, xf)      # (the tables keep the home matrices: the fresh context below moves too)
        done.append((order, r, k))
    fresh = renderer(done[0][2].desc())
    fresh.update_instances(ids, xf)
    for order, r, k in done:
        diff = dict(diff_words(r, fresh), nodes=optin.words(r.accel_readback(abi.ACCEL_NODES), fresh.accel_readback(abi.ACCEL_NODES)))
        assert diff == {"records": 0, "alpha": 0, "nodes": 0}, order
        r.destroy()
    fresh.destroy()


@pytest.mark.parametrize("seed", materials.SEEDS)
def test_generated_sequences_equal_the_twin(seed):
    t = materials.edge()
    r = renderer(t.desc())
    ops = materials.ops(t, seed)
    print("replay: materials.ops(materials.edge(), %d)" % seed)
    for k, op in enumerate(ops):
        print(k, materials.describe(op))
        before = r.material_stats()
        msg = materials.issue(r, op)
        if op["kind"] == "refused":
            assert materials.MESSAGE[op["why"]] in msg, (op["why"], msg)
            after = r.material_stats()
            assert bytes(before) == bytes(after)
        materials.apply(t, op)
        if k % 4 == 3 or k == len(ops) - 1:
            fresh = renderer(t.desc())
            assert diff_derived(derived(r), derived(fresh)) == SAME, (seed, k)
            ids = [int(i) for i in t.alpha_instances(range(1, 8))][:8]
            same_rays(r, fresh, refit.make_rays(t.desc(), ids, 1024, 100 * seed + k))
            fresh.destroy()
    maps_equal_the_host_function(r, t)
    r.destroy()


# ---- 6. textures ------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", [k for k in materials.RECT_KINDS if k != "same_alpha"])
def test_texel_rectangles_equal_a_fresh_context_that_uploaded_the_edited_texture(kind):
    t = materials.edge()
    r = renderer(t.desc())
    rng = np.random.default_rng(7)
    for tex, shared in ((materials.T_SQUARE, [1, 6]), (materials.T_ODD, [2])):
        op = None
        while op is None or op["texture"] != tex or (op["texels"][..., 3] == t.texels[tex][op["y"]:op["y"] + op["texels"].shape[0], op["x"]:op["x"] + op["texels"].shape[1], 3]).all():
            op = materials.draw(t, rng, kind)
        st = edit(r, t, op)
        fresh = renderer(t.desc())
        assert diff_words(r, fresh) == {"records": 0, "alpha": 0}, (kind, tex)
        # every material whose base colour texture this is was rebuilt, and no other
        n = tris_of_materials(t, shared)
        assert (st.materialsWritten, st.dirtyMaterials, st.alphaRecords) == (0, len(shared), n), (kind, tex)
        assert st.bytesUploaded >= op["texels"].size
        ids = [int(i) for i in t.alpha_instances(shared)]
        same_rays(r, fresh, refit.make_rays(t.desc(), ids, 1024, 5))
        fresh.destroy()
    assert maps_equal_the_host_function(r, t) == 30
    r.destroy()


def test_a_texture_no_base_colour_uses_launches_nothing():
    t = materials.edge()
    r = renderer(t.desc())
    before = r.accel_readback(abi.ACCEL_TRIS).copy()
    st = edit(r, t, "padded", texture=materials.T_EMISSIVE, x=1, y=2, texels=np.full((3, 4, 4), 77, np.uint8), pitch=4 * 4 + 12)
    assert (st.dirtyMaterials, st.alphaRecords, st.leafRecords, st.texelsScanned) == (0, 0, 0, 0) and st.bytesUploaded == 3 * 4 * 4
    assert np.array_equal(before, r.accel_readback(abi.ACCEL_TRIS))
    r.destroy()


# ---- 7. rt_build_accel after edits, next to a context that has cached the unedited scene ------------------------------------------------------------------------------
def test_a_host_build_after_edits_does_not_reuse_the_cached_build_of_the_old_scene():
    t = materials.edge()
    other = renderer(t.desc())      # its host build of the unedited scene is the process's cached one
    r = renderer(t.desc())
    edit(r, t, "cutoff", ids=[1], rows=row(t, 1, cutoff=0.9).reshape(1, 20))
    texels = t.texels[materials.T_ODD].copy()
    texels[..., 3] = 255 - texels[..., 3]
    edit(r, t, "full_width", texture=materials.T_ODD, x=0, y=0, texels=texels, pitch=None)
    assert refit.hip_build_accel(r) == 0
    assert maps_equal_the_host_function(r, t) == 30
    fresh = renderer(t.desc())
    assert diff_words(r, fresh) == {"records": 0, "alpha": 0}
    assert optin.words(other.accel_readback(abi.ACCEL_TRIS), fresh.accel_readback(abi.ACCEL_TRIS)) > 0      # the old scene's maps are other ones
    for x in (other, r, fresh):
        x.destroy()


# ---- 8. refusals, and what a successful edit resets ----------------------------------------------------------------------------------------------------------------------
def digest(r):
    return [r.accel_readback(w).tobytes() for w in (abi.ACCEL_NODES, abi.ACCEL_TRIS, abi.ACCEL_ALPHA)] + [bytes(r.material_stats())]


def test_every_refusal_changes_nothing():
    W, H = SIZES[1]
    sc = refit.street()
    t = materials.of_scene(sc)
    desc = t.desc()
    st = blend.state(sc, W, H)
    r = renderer(desc, W, H, overlap=0)
    o = Oracle(0); o.upload_scene(desc); o.resize(W, H)
    sc.updateCamera(W, H)

    def frame(f):
        st.time = 1000 + f
        cam = blend.rest_camera(sc, W, H)
        r.set_camera(cam); o.set_camera(cam)
        r.run(st, f); o.render_frame(st, f)
        bad = {abi.BUFFER_NAMES[b]: optin.words(r.readback(b), o.readback(b)) for b in frame_buffers(f)}
        assert not any(bad.values()), (f, bad)

    frame(0)
    leaf = t.material_of_mesh(int(t.inst["primMesh"][int(refit.describe(desc)["alpha"][0])]))
    edit(r, t, "roughness", ids=[leaf], rows=t.mats[leaf].reshape(1, 20))      # (an edit that changes no bit: the stats are those of a call)
    was = digest(r)
    rng = np.random.default_rng(3)
    for why in materials.REFUSALS:
        op = materials.draw_refusal(t, rng, why)
        msg = materials.issue(r, op)
        print(why, "->", msg)
        assert materials.MESSAGE[op["why"]] in msg and digest(r) == was, why
        if op["call"] == "materials" and op["ids"] is not None:
            assert ("material %d" % op["ids"][-1 if why == "duplicate" else 0]) in msg, (why, msg)      # the first offender by name
    # the emitter mode: the luminance of an emissive material is fixed (the derived alias table would go stale); its other fields are not
    lit = int(np.nonzero(materials._emissive(t))[0][0])
    r.set_emitter_meshes(*sc.emitterMeshes(), sc.lightWeights[0])
    was = digest(r)
    brighter = t.mats[lit].copy()
    brighter[blend.W_EMISSIVE] = (brighter[blend.W_EMISSIVE].view(np.float32) * np.float32(2)).view(np.uint32)
    from restir_amd.renderer import RtError
    with pytest.raises(RtError, match="emitter mode"):
        r.update_materials([lit], brighter.reshape(1, 20))
    assert digest(r) == was
    r.set_emitter_meshes()
    # The material rows have no readback to digest.  The device rows: the next frame is the unedited scene's.  The context's copy: a host build from it gives the
    # leaf records and alpha records of a fresh context of the unedited description (its cache key reads every byte of the rows).
    frame(1)
    assert refit.hip_build_accel(r) == 0
    fresh = renderer(desc)
    assert diff_words(r, fresh) == {"records": 0, "alpha": 0}
    r.destroy(); fresh.destroy()


def test_a_successful_edit_resets_the_reference_sums_and_drops_settled_visibility():
    W, H = SIZES[0]
    sc = refit.street()
    t = materials.of_scene(sc)
    desc = t.desc()
    st = blend.state(sc, W, H)
    r = renderer(desc, W, H, overlap=0, traversal=abi.TRAVERSAL_THROUGHPUT)
    sc.updateCamera(W, H)
    def rest(frames):
        for f in frames:
            st.time = 1000 + f
            r.set_camera(blend.rest_camera(sc, W, H))
            r.run(st, f)

    rest(range(4))      # the third launch at a camera records, the fourth replays
    before = r.primary_replay_stats()
    r.reference_render(st, 2)
    assert before.state == 1 and r.reference_samples() == 2
    leaf = t.material_of_mesh(int(t.inst["primMesh"][int(refit.describe(desc)["alpha"][0])]))
    for kind, words in (("alpha", dict(cutoff=0.7)), ("plain", dict(rough=0.2))):
        if kind == "plain":      # settle again
            rest(range(4, 8))
            r.reference_render(st, 2)
            assert r.primary_replay_stats().state == 1 and r.reference_samples() == 2
        edit(r, t, "cutoff", ids=[leaf], rows=row(t, leaf, **words).reshape(1, 20))
        assert r.primary_replay_stats().state == 0 and r.reference_samples() == 0, kind
    # before a build the call is a row copy; before a scene it is refused
    from restir_amd.renderer import Renderer, hip_lib
    bare = Renderer().setup(0)
    m = np.ascontiguousarray(t.mats[:1])
    ids = np.zeros(1, np.uint32)
    assert hip_lib().rt_update_materials(bare._h, 1, ids.ctypes.data, m.ctypes.data) == -4      # RT_ERR_NO_SCENE
    assert hip_lib().rt_upload_scene(bare._h, C.byref(t.desc())) == 0
    bare.update_materials([leaf], row(t, leaf, cutoff=0.3).reshape(1, 20))
    s = bare.material_stats()
    assert (s.materialsWritten, s.dirtyMaterials, s.alphaRecords) == (1, 1, 0)
    assert hip_lib().rt_build_accel(bare._h) == 0      # the build reads the edited row
    materials.apply(t, {"kind": "cutoff", "ids": [leaf], "rows": row(t, leaf, cutoff=0.3).reshape(1, 20)})
    fresh = renderer(t.desc())
    assert diff_words(bare, fresh) == {"records": 0, "alpha": 0}
    for x in (r, bare, fresh):
        x.destroy()
