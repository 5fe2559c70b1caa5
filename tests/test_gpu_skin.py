"""Deforming meshes on the GPU: rt_update_skins' vertices equal the CPU restatement (tests/skin_checker.cpp) word for word; the refitted tree equals the refit
checker on the deformed description word for word; rays and frames equal those of a fresh build / of the oracle rendering the deformed scene bit for bit;
rt_update_vertices gives the same frames from host-posed rows; refused calls change nothing; a steady-state rt_update_skins moves no vertex across the bus.
No tolerance anywhere: results are a function of the triangle set, never of the tree."""
import ctypes as C
import numpy as np
import pytest

from helpers import abi, host, frame_buffers
from oracle.binding import Oracle
import optin
import refit
import skin

pytestmark = pytest.mark.gpu

FRAMES = 8
SIZES = ((64, 48), (67, 45))
TALL, SHORT = 4, 3      # Cornell's boxes (instances)


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    return refit.build(tmp_path_factory.mktemp("refit"))


@pytest.fixture(scope="module")
def chk(tmp_path_factory):
    return skin.build(tmp_path_factory.mktemp("skin"))


def renderer(desc, W=None, H=None, overlap=None, traversal=None):
    from restir_amd.renderer import Renderer
    r = Renderer().setup(0)
    if overlap is not None:
        r.set_overlap(overlap)
    r.load_scene(desc)
    if W:
        r.update(W, H)
    if traversal is not None:
        r.set_traversal(traversal)
    return r


def device_tree(lib, r, desc):
    st = r.refit_stats()
    return refit.Tree(lib, desc, r.accel_readback(abi.ACCEL_NODES), r.accel_readback(abi.ACCEL_TRIS), r.accel_readback(abi.ACCEL_INSTANCES, desc.numInstances), st.treePad)


def same_tree(r, t, desc):
    return {"nodes": optin.words(r.accel_readback(abi.ACCEL_NODES), t.nodes), "records": optin.words(r.accel_readback(abi.ACCEL_TRIS), t.recs),
            "instances": optin.words(r.accel_readback(abi.ACCEL_INSTANCES, desc.numInstances), t.inst)}


def all_state(r, desc):
    """everything a refused call must leave alone"""
    return [r.vertices_readback(0, desc.numVertices).tobytes()] + [r.accel_readback(w, desc.numInstances).tobytes() for w in range(3)] + \
           [bytes(r.refit_stats()), bytes(r.deform_stats())]


def by_global_id(rec):
    out = {}
    for k in np.argsort(rec["globalId"], kind="stable"):
        out.setdefault(int(rec["globalId"][k]), rec[k])
    return out


# ---- 1. vertices word for word ---------------------------------------------------------------------------------------------------------------------------
def test_skinned_vertices_equal_the_checker_word_for_word(chk):
    counts, joints = (1, 63, 64, 65, 257), (1, 5, 1, 5, 5)      # triangles per mesh: below a wave of vertices ... above a 256-thread block
    sc = skin.Patches(chk, counts)
    desc = sc.desc()
    r = renderer(desc)
    meshes = [skin.SkinnedMesh(chk, desc, m, j, seed=m) for m, j in enumerate(joints)]
    assert any((m.influences["weight"][:, 3] == 1).any() for m in meshes)          # a vertex whose whole weight sits in slot 3
    r.set_skins(*skin.skins_table(meshes))
    want = skin.vertices_of(desc)
    assert np.array_equal(r.vertices_readback(0, desc.numVertices).view(np.uint32), want.view(np.uint32))
    for kind, ids in (("bend", [1, 4]), ("mirror", [0, 2, 3]), ("twist", [4, 3, 2, 1, 0]), ("mirror", [3]), ("back", [])):
        mats = [meshes[k].matrices(kind, 2.0) for k in ids]
        for k, m in zip(ids, mats):
            want[meshes[k].first:meshes[k].first + meshes[k].count] = meshes[k].posed(m)
        r.update_skins(ids, np.concatenate(mats) if mats else np.zeros((0, 12), np.float32))
        got = r.vertices_readback(0, desc.numVertices)
        assert optin.words(got, want) == 0, (kind, ids)
        st = r.deform_stats()
        assert (st.meshes, st.vertices, st.instances, st.vertexBytesCopied) == (len(ids), sum(meshes[k].count for k in ids), len(ids), 0)
    assert want["normal"][0] == 0xffffffff and (want["normal"][1:] != skin.vertices_of(desc)["normal"][1:]).any()
    r.destroy()


def test_skinned_street_meshes_equal_the_checker(chk):
    """the street scene has no single mesh that is shared, alpha-tested and thousands of vertices large: the instanced (shared, one instance mirrored) tree mesh and
    the alpha-tested leaf mesh, which has thousands of vertices at this scale, are skinned together"""
    sc = refit.street(0.2)
    desc = sc.desc()
    a, b = skin.deformed_mesh("street", desc), skin.alpha_mesh(desc)
    assert len(skin.instances_of_mesh(desc, a)) > 2 and skin.mesh_range(desc, b)[1] > 2000
    r = renderer(desc)
    meshes = [skin.SkinnedMesh(chk, desc, a, 5), skin.SkinnedMesh(chk, desc, b, 5)]
    r.set_skins(*skin.skins_table(meshes))
    want = skin.vertices_of(desc)
    for kind in ("bend", "mirror"):
        mats = [m.matrices(kind, 10.0) for m in meshes]
        for m, j in zip(meshes, mats):
            want[m.first:m.first + m.count] = m.posed(j)
        r.update_skins([0, 1], np.concatenate(mats))
        assert optin.words(r.vertices_readback(0, desc.numVertices), want) == 0, kind
    assert r.deform_stats().instances == len(skin.instances_of_mesh(desc, a)) + len(skin.instances_of_mesh(desc, b))
    r.destroy()


# ---- 2. the tree word for word ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["cornell", "street"])
def test_device_tree_equals_the_refit_checker_word_for_word(lib, chk, name):
    sc = refit.cornell() if name == "cornell" else refit.street()
    desc = sc.desc()
    r = renderer(desc)
    m = skin.deformed_mesh(name, desc)
    ids = skin.instances_of_mesh(desc, m)
    inst = refit.instances_of(desc)
    xf = inst["objectToWorld"][ids]
    mirrored = [int(i) for i in ids if i in refit.describe(desc)["mirrored"]]
    if name == "street":
        assert len(ids) > 1 and mirrored
    r.update_instances([], np.zeros((0, 12), np.float32))      # tells the build's pad; changes no word
    t = device_tree(lib, r, desc)
    assert t.check() == (0, "")
    ext = refit.scene_extent(t)
    sk = skin.SkinnedMesh(chk, desc, m, 3)
    r.set_skins(*skin.skins_table([sk]))
    verts = skin.vertices_of(desc)
    fulls = 0
    for kind in skin.POSES:
        mats = sk.matrices(kind, ext)
        verts[sk.first:sk.first + sk.count] = sk.posed(mats)
        t.desc = skin.with_vertices(desc, verts.copy())
        assert t.refit(ids, xf) == 0
        r.update_skins([0], mats)
        st = r.refit_stats()
        diff = same_tree(r, t, desc)
        print(name, kind, diff, "records", st.leafRecords, "nodes", st.nodes, "full", st.fullRefit, "ms", round(st.ms, 3), "skin ms", round(r.deform_stats().skinMs, 3))
        assert diff == {"nodes": 0, "records": 0, "instances": 0}, kind
        assert t.check() == (0, ""), kind
        assert [st.instances, st.leafRecords, st.nodes, st.levels, st.fullRefit] == [len(ids)] + [int(x) for x in t.stats], kind
        assert np.float32(st.triPad) == np.float32(t.tri_pad) and np.float32(st.treePad) == np.float32(t.tree_pad)
        fulls += st.fullRefit
        if kind == "far":
            assert st.fullRefit == 1
        rec = r.accel_readback(abi.ACCEL_TRIS).view(refit.REC_DT)
        for i in mirrored:      # k_refit_tris rewrites TRI_FLIP from the flip bits: a mirrored instance of the deformed mesh keeps it
            mine = t.ref[rec["globalId"], 0] == i
            assert mine.any() and (rec["flags"][mine] & refit.TRI_FLIP).all(), (kind, i)
        for i in ids:
            if i not in mirrored:
                assert not (rec["flags"][t.ref[rec["globalId"], 0] == i] & refit.TRI_FLIP).any()
    assert fulls >= 1
    r.destroy()


def test_an_unreferenced_vertex_does_not_move_the_pad(lib, chk):
    sc = skin.Patches(chk, (65, 20), extra=(900.0, 0.5, -700.0), mirror_instance_of=0)
    desc = sc.desc()
    r = renderer(desc)
    sk = skin.SkinnedMesh(chk, desc, 0, 2)
    sk.centre = np.array([0.2, 1.4, 0.0])      # of the triangles (the stray vertex would put the poses' pivot far outside them)
    r.set_skins(*skin.skins_table([sk]))
    mats = sk.matrices("bend", 2.0)
    verts = skin.vertices_of(desc)
    verts[sk.first:sk.first + sk.count] = sk.posed(mats)
    assert np.abs(verts["position"][sk.first + sk.count - 1]).max() > 500      # the stray vertex is posed like the others, and stays far away
    r.update_skins([0], mats)
    fresh = refit.Tree.built(lib, skin.with_vertices(desc, verts))
    st = r.refit_stats()
    assert np.float32(st.triPad).tobytes() == np.float32(fresh.tri_pad).tobytes() and st.triPad < 2e-5 * 100 and st.instances == 2
    # ... and the same through rt_update_vertices on the other mesh
    first, count = skin.mesh_range(desc, 1)
    rows = verts[first:first + count].copy()
    rows["position"][:-1] += np.float32(0.25)
    rows["position"][-1] *= np.float32(2)
    r.update_vertices(1, 0, rows)
    verts[first:first + count] = rows
    fresh = refit.Tree.built(lib, skin.with_vertices(desc, verts))
    assert np.float32(r.refit_stats().triPad).tobytes() == np.float32(fresh.tri_pad).tobytes()
    r.destroy()


# ---- 3. rays: the updated context against a fresh context that uploaded and built the deformed scene ---------------------------------------------------------
def make_rays(desc, ids, n, seed):
    """tests/test_gpu_refit.py's construction: half of the rays through the boxes of `ids`"""
    rng = np.random.default_rng(seed)
    inst = refit.instances_of(desc)
    lo = np.min([refit.world_bounds(desc, i)[0] for i in range(len(inst))], axis=0)
    hi = np.max([refit.world_bounds(desc, i)[1] for i in range(len(inst))], axis=0)
    c, rad = 0.5 * (lo + hi), 0.5 * np.linalg.norm(hi - lo)
    target = lo + rng.random((n, 3)) * (hi - lo)
    for k in range(n // 2):
        a, b = refit.world_bounds(desc, ids[k % len(ids)])
        target[k] = a + rng.random(3) * (b - a)
    d = rng.normal(size=(n, 3))
    origin = c + 1.5 * rad * d / np.linalg.norm(d, axis=1, keepdims=True)
    inside = rng.random(n) < 0.25
    origin[inside] = lo + rng.random((int(inside.sum()), 3)) * (hi - lo)
    dirs = target - origin
    dist = np.linalg.norm(dirs, axis=1, keepdims=True)
    rays = np.zeros((n, 8), np.float32)
    rays[:, 0:3], rays[:, 3:6] = origin, dirs / dist
    rays[:, 6] = (dist[:, 0] * rng.uniform(0.3, 2.0, n)).astype(np.float32)
    rays[:, 7] = rng.integers(0, 2 ** 32, n, dtype=np.uint32).view(np.float32)
    return rays


@pytest.mark.parametrize("name", ["cornell", "street"])
def test_rays_equal_a_fresh_build_also_after_both_rebuilds(chk, name):
    sc = refit.cornell() if name == "cornell" else refit.street()
    desc = sc.desc()
    r = renderer(desc)
    m = skin.deformed_mesh(name, desc)
    ids = [int(i) for i in skin.instances_of_mesh(desc, m)]
    ext = max(np.abs(refit.world_bounds(desc, i)).max() for i in range(desc.numInstances))
    sk = skin.SkinnedMesh(chk, desc, m, 3)
    r.set_skins(*skin.skins_table([sk]))
    verts = skin.vertices_of(desc)
    for kind in ("twist", "far", "back", "mirror", "bend"):
        mats = sk.matrices(kind, ext)
        r.update_skins([0], mats)
    verts[sk.first:sk.first + sk.count] = sk.posed(mats)
    d2 = skin.with_vertices(desc, verts)
    fresh = renderer(d2)
    rays = make_rays(d2, ids, 4096, 11)

    def same_hits():
        for mode in (abi.TRAVERSAL_THROUGHPUT, abi.TRAVERSAL_LATENCY):
            r.set_traversal(mode); fresh.set_traversal(mode)
            a, b = r.trace_closest(rays), fresh.trace_closest(rays)
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), mode
            assert np.array_equal(r.trace_any(rays), fresh.trace_any(rays)), mode
        return a.view(np.uint32)[:, 1]

    gid = same_hits()
    hit = gid[gid != 0xffffffff]
    on_deformed = int(np.isin(refit.tri_ref(d2)[hit, 0], ids).sum())
    print(name, "rays that hit:", hit.size, "of them on deformed instances:", on_deformed)
    assert on_deformed > 20
    want = by_global_id(fresh.accel_readback(abi.ACCEL_TRIS).view(refit.REC_DT))

    def same_records():
        rec = r.accel_readback(abi.ACCEL_TRIS).view(refit.REC_DT)
        w = np.array([want[int(g)] for g in rec["globalId"]], dtype=refit.REC_DT)
        for field in ("v0", "e1", "e2", "flags", "omm"):
            assert np.array_equal(rec[field].view(np.uint32), w[field].view(np.uint32)), field

    same_records()
    r.rebuild_accel()                       # the device builder reads the device vertices
    same_hits(); same_records()
    assert refit.hip_build_accel(r) == 0    # the host builder reads the context's copy, which rt_update_skins left stale: it is refreshed first
    same_hits(); same_records()
    assert optin.words(r.vertices_readback(0, desc.numVertices), verts) == 0
    r.update_skins([0], sk.matrices("twist", ext))      # the skins survive both rebuilds
    verts[sk.first:sk.first + sk.count] = sk.posed(sk.matrices("twist", ext))
    assert optin.words(r.vertices_readback(0, desc.numVertices), verts) == 0
    r.destroy(); fresh.destroy()


# ---- 4. frames: an 8-frame Cornell sequence, orbiting camera; the tall box is skinned with two joints, the short box moves -------------------------------------
def box_move(f, home):
    return refit.compose(refit.translation([0.03 * f, 0.0, -0.02 * f]), refit.compose(refit.rotation_y(0.1 * f, (0.33, 0.3, 0.35)), home[SHORT]))


class Sequence:
    """the scene, the skinned mesh, the per-frame poses and cameras; the oracle's frames are rendered once per variant and shared by the cases.
    which: "tall" = the tall box deforms (rows from the checker), "light" = the emissive quad deforms (Scene.updateVertices recomputes the light records)"""
    cache = {}

    def __init__(self, chk, W, H, move_box=True, which="tall"):
        self.W, self.H, self.move_box, self.which = W, H, move_box, which
        self.sc = refit.cornell()
        desc = self.sc.desc()
        self.home = refit.instances_of(desc)["objectToWorld"]
        self.mesh = int(refit.instances_of(desc)["primMesh"][TALL if which == "tall" else 5])
        self.sk = skin.SkinnedMesh(chk, desc, self.mesh, 2)
        if which == "light":      # flat in y: its +x half follows joint 1
            self.sk.influences["joint"][:, 0] = self.sk.rest["position"][:, 0] > 0
            self.sk.influences["weight"][:] = [1, 0, 0, 0]
        self.verts = skin.vertices_of(desc)
        self.st = host.default_state(W, H, self.sc, None)
        self.st.environmentProb = 0.0
        self.pose = self.sc.cameraPose()

    def matrices(self, f):
        """joint 0 stays; joint 1 (the top ring) twists and leans a little more every frame"""
        c = self.sk.centre
        if self.which == "light":
            return np.stack([skin.affine(), skin.affine(skin.rot("z", -0.05 * (f + 1)), (0.01 * f, 0, 0), c)])
        return np.stack([skin.affine(), skin.affine(skin.rot("z", 0.03 * (f + 1)) @ skin.rot("y", 0.08 * (f + 1)), (0.01 * f, 0, 0), c)])

    def step(self, f):
        """deform (and move) the scene for frame f: (joint matrices, posed rows, description, camera)"""
        mats = self.matrices(f)
        rows = self.sk.posed(mats)
        self.verts[self.sk.first:self.sk.first + self.sk.count] = rows
        if self.move_box:
            self.sc.updateInstances([SHORT], [box_move(f, self.home)])
        if self.which == "light":
            self.sc.updateVertices(self.mesh, 0, rows)
            desc = self.sc.desc()
        else:
            desc = skin.with_vertices(self.sc.desc(), self.verts.copy())
        eye, center, up, fov = self.pose
        a = 0.06 * f
        d = np.asarray(eye, np.float64) - center
        e = center + np.array([np.cos(a) * d[0] + np.sin(a) * d[2], d[1], -np.sin(a) * d[0] + np.cos(a) * d[2]])
        self.sc.setCamera(e.astype(np.float32), center, up, fov)
        self.sc.updateCamera(self.W, self.H)
        self.st.time = 1000 + f
        return mats, rows, desc, self.sc.getCamera()

    @classmethod
    def oracle_frames(cls, chk, W, H, move_box=True, which="tall", frames=FRAMES):
        key = (W, H, move_box, which, frames)
        if key not in cls.cache:
            s = cls(chk, W, H, move_box, which)
            o = Oracle(0)
            o.upload_scene(s.sc.desc())
            o.resize(W, H)
            out = []
            for f in range(frames):
                _, _, desc, cam = s.step(f)
                o.upload_scene(desc)          # (the oracle keeps its frame buffers across a scene upload: the history carries over)
                o.set_camera(cam)
                o.render_frame(s.st, f)
                out.append({b: o.readback(b).copy() for b in frame_buffers(f)})
            cls.cache[key] = out
        return cls.cache[key]


def frame_diff(r, want, f):
    return {abi.BUFFER_NAMES[b]: optin.words(r.readback(b), want[f][b]) for b in frame_buffers(f) if optin.words(r.readback(b), want[f][b])}


def run_case(chk, W, H, overlap, traversal, path="skins", move_box=True, which="tall", frames=FRAMES, setup=None):
    want = Sequence.oracle_frames(chk, W, H, move_box, which, frames)
    s = Sequence(chk, W, H, move_box, which)
    r = renderer(s.sc.desc(), W, H, overlap, traversal)
    if setup:
        setup(r)
    if path == "skins":
        r.set_skins(*skin.skins_table([s.sk]))
    bad = {}
    for f in range(frames):
        mats, rows, desc, cam = s.step(f)
        if path == "skins":
            r.update_skins([0], mats)
        else:
            r.update_vertices(s.mesh, 0, rows)
        if which == "light":
            r.update_lights(desc)
        if move_box:
            r.update_instances([SHORT], [box_move(f, s.home)])
        r.set_camera(cam)
        r.run(s.st, f)
        d = frame_diff(r, want, f)
        if d:
            bad[f] = d
    return r, s, bad


@pytest.mark.parametrize("W,H", SIZES)
@pytest.mark.parametrize("traversal", [abi.TRAVERSAL_THROUGHPUT, abi.TRAVERSAL_LATENCY])
@pytest.mark.parametrize("overlap", [0, 1, 2, 3])
def test_frames_equal_the_oracle_rendering_the_deformed_scene(chk, W, H, overlap, traversal):
    r, s, bad = run_case(chk, W, H, overlap, traversal)
    r.destroy()
    assert bad == {}
    want = Sequence.oracle_frames(chk, W, H)      # the sequence is not a still
    assert optin.words(want[2][abi.BUF_GBUFFER0], want[4][abi.BUF_GBUFFER0]) > 0
    # ... and the deformation alone changes what is seen: the same frames without the moving box
    still = Sequence.oracle_frames(chk, W, H, move_box=False)
    assert optin.words(still[2][abi.BUF_GBUFFER0], still[4][abi.BUF_GBUFFER0]) > 0


@pytest.mark.parametrize("which", ["svgf", "gi_spatial", "taa"])
def test_deformation_with_an_opt_in_pass(tmp_path, chk, which):
    import gi_spatial
    W, H = SIZES[1]
    kw = {"svgf": dict(den=abi.Denoiser(mode=abi.DENOISER_SVGF)), "gi_spatial": dict(gis=abi.GiSpatial(mode=abi.GI_SPATIAL_VISIBILITY)), "taa": dict(t=abi.Taa(mode=abi.TAA_ON))}[which]
    rig = optin.Rig(tmp_path, abi.PROC_CORNELL, 1.0, None, W, H, overlap=2, **kw)
    desc = rig.sc.desc()
    home = refit.instances_of(desc)["objectToWorld"]
    sk = skin.SkinnedMesh(chk, desc, int(refit.instances_of(desc)["primMesh"][TALL]), 2)
    rig.r.set_skins(*skin.skins_table([sk]))
    verts = skin.vertices_of(desc)
    for f in range(5):
        mats = np.stack([skin.affine(), skin.affine(skin.rot("z", 0.03 * (f + 1)) @ skin.rot("y", 0.08 * (f + 1)), (0.01 * f, 0, 0), sk.centre)])
        verts[sk.first:sk.first + sk.count] = sk.posed(mats)
        rig.sc.updateInstances([SHORT], [box_move(f, home)])
        d2 = skin.with_vertices(rig.sc.desc(), verts.copy())
        rig.r.update_skins([0], mats)
        rig.r.update_instances([SHORT], [box_move(f, home)])
        rig.o.upload_scene(d2)
        rig.kg = gi_spatial.GiSpatialChecker(gi_spatial.build(tmp_path), d2)
        rig.desc = d2
        rig.frame(f)
        assert rig.diff(f) == {}, f
    n = rig.history_lengths()
    if which != "gi_spatial":      # the histories on the undeformed surfaces were carried across the updates, not dropped
        assert all(v.max() >= 3 for v in n.values()), {k: v.max() for k, v in n.items()}
    rig.destroy()


def test_a_deformation_alone_puts_no_instance_in_motion(chk):
    W, H = SIZES[0]
    r, s, bad = run_case(chk, W, H, 2, None, move_box=False, setup=lambda r: r.set_object_motion(abi.OBJECT_MOTION_ON))
    r.destroy()
    assert bad == {}      # the oracle's plain frames: no instance's matrix changed, so no pixel takes a per-instance camera


# ---- 5. the host path ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("overlap", [0, 2])
def test_update_vertices_with_the_checkers_rows_gives_the_same_frames(chk, overlap):
    W, H = SIZES[1]
    r, s, bad = run_case(chk, W, H, overlap, None, path="vertices")
    assert bad == {}
    assert r.deform_stats().vertexBytesCopied == s.sk.count * 32
    r.destroy()


def test_a_deformed_emitter_through_scene_update_vertices_and_update_lights(chk):
    W, H = SIZES[0]
    r, s, bad = run_case(chk, W, H, 2, None, path="vertices", move_box=False, which="light", frames=4)
    r.destroy()
    assert bad == {}
    want = Sequence.oracle_frames(chk, W, H, False, "light", 4)
    assert optin.words(want[1][abi.BUF_DIRECT_RESULT0 + 1], want[3][abi.BUF_DIRECT_RESULT0 + 1]) > 0


def test_a_partial_range_updates_only_that_range(chk):
    sc = refit.cornell()
    desc = sc.desc()
    r = renderer(desc)
    m = int(refit.instances_of(desc)["primMesh"][TALL])
    first, count = skin.mesh_range(desc, m)
    want = skin.vertices_of(desc)
    rows = want[first + 5:first + 9].copy()
    rows["position"] += np.float32(0.01)
    rows["normal"] = chk.skc_encode(0.0, 0.0, 1.0)
    rows["color"] = 0x11223344
    r.update_vertices(m, 5, rows)
    want[first + 5:first + 9] = rows
    assert optin.words(r.vertices_readback(0, desc.numVertices), want) == 0
    assert optin.words(r.vertices_readback(first + 5, 4), rows) == 0
    st = r.deform_stats()
    assert (st.meshes, st.vertices, st.instances, st.vertexBytesCopied) == (1, 4, 1, 4 * 32)
    r.update_vertices(m, count, np.zeros(0, skin.VERTEX_DT))      # an empty range at the end of the mesh is valid and changes nothing
    assert optin.words(r.vertices_readback(0, desc.numVertices), want) == 0 and r.deform_stats().vertices == 0
    r.destroy()


# ---- 6. refusals change nothing ---------------------------------------------------------------------------------------------------------------------------
def test_refused_calls_change_nothing_and_the_next_frame_matches(chk):
    from restir_amd.renderer import Renderer, RtError, hip_lib
    W, H = SIZES[0]
    want = Sequence.oracle_frames(chk, W, H)
    s = Sequence(chk, W, H)
    desc0 = s.sc.desc()
    L = hip_lib()
    sk_tab, inf_tab = skin.skins_table([s.sk])
    one = np.zeros(1, np.uint32)
    ident = np.stack([skin.affine(), skin.affine()])
    # before rt_upload_scene / rt_build_accel
    r0 = Renderer().setup(0)
    rows0 = s.sk.rest.copy()
    assert L.rt_update_vertices(r0._h, s.mesh, 0, 1, rows0.ctypes.data) == abi.ERR_NO_SCENE
    assert L.rt_set_skins(r0._h, 1, sk_tab.ctypes.data, inf_tab.size, inf_tab.ctypes.data) == abi.ERR_NO_SCENE
    assert L.rt_upload_scene(r0._h, C.byref(desc0)) == 0
    assert L.rt_update_vertices(r0._h, s.mesh, 0, 1, rows0.ctypes.data) == abi.ERR_NO_ACCEL
    assert L.rt_set_skins(r0._h, 1, sk_tab.ctypes.data, inf_tab.size, inf_tab.ctypes.data) == 0      # valid after rt_upload_scene
    assert L.rt_update_skins(r0._h, 1, one.ctypes.data, ident.ctypes.data) == abi.ERR_NO_ACCEL
    r0.destroy()
    r = renderer(desc0, W, H, 2)
    with pytest.raises(RtError):      # before rt_set_skins
        r.update_skins([0], ident)
    r.set_skins(sk_tab, inf_tab)
    for f in range(2):
        mats, rows, desc, cam = s.step(f)
        r.update_skins([0], mats)
        r.update_instances([SHORT], [box_move(f, s.home)])
        r.set_camera(cam)
        r.run(s.st, f)
    r.sync()
    state = all_state(r, desc0)
    other = int(refit.instances_of(desc0)["primMesh"][SHORT])
    light = int(refit.instances_of(desc0)["primMesh"][5])
    ofirst, ocount = skin.mesh_range(desc0, other)
    ok_rows = skin.vertices_of(desc0)[ofirst:ofirst + ocount]
    nan_rows = ok_rows.copy(); nan_rows["position"][2, 1] = np.nan
    inf_rows = ok_rows.copy(); inf_rows["position"][0, 0] = np.inf
    tc = ok_rows["texcoord"].copy()
    tc.view(np.uint32)[1, 1] ^= 1                                                 # the handedness bit
    uv_rows = ok_rows.copy(); uv_rows["texcoord"] = tc
    refused = [
        lambda: r.update_vertices(desc0.numPrimMeshes, 0, ok_rows[:1]),          # a mesh that does not exist
        lambda: r.update_vertices(other, ocount - 1, ok_rows[:2]),                # a range outside the mesh
        lambda: r.update_vertices(other, 0, nan_rows), lambda: r.update_vertices(other, 0, inf_rows),
        lambda: r.update_vertices(other, 0, uv_rows),
        lambda: r.update_vertices(s.mesh, 0, s.sk.rest),                          # a mesh that has a skin
        lambda: r.update_skins([1], ident), lambda: r.update_skins([0, 0], np.concatenate([ident, ident])),
        lambda: r.update_skins([0], np.stack([skin.affine(), skin.affine(t=(np.nan, 0, 0))])),
        # finite entries of 3e38 scale: the weights of a row sum to 1, so the blend stays finite and y' = (3e38 y) + 3e38 overflows for the box's upper vertices
        lambda: r.update_skins([0], np.stack([skin.affine(np.eye(3) * 3e38, (0, 3e38, 0))] * 2)),
    ]
    for k, call in enumerate(refused):
        with pytest.raises(RtError):
            call()
        assert all_state(r, desc0) == state, k
    # rt_set_skins' refusals leave the skins in place (the next frame below re-poses skin 0)
    def skins(**kw):
        t = sk_tab.copy()
        for key, v in kw.items():
            t[key] = v
        return t
    bad_joint = inf_tab.copy(); bad_joint["joint"][3, 2] = 2
    bad_weight = inf_tab.copy(); bad_weight["weight"][1, 0] = np.inf
    for k, (tab, inf) in enumerate([(skins(primMesh=desc0.numPrimMeshes), inf_tab), (np.concatenate([sk_tab, sk_tab]), inf_tab), (skins(jointCount=0), inf_tab),
                                    (skins(firstInfluence=1), inf_tab), (sk_tab, inf_tab[:-1]), (sk_tab, bad_joint), (sk_tab, bad_weight),
                                    (skins(primMesh=light), np.zeros(64, skin.INFLUENCE_DT))]):
        with pytest.raises(RtError):
            r.set_skins(tab, inf)
        assert all_state(r, desc0) == state, ("set_skins", k)
    with pytest.raises(RtError):
        r.vertices_readback(desc0.numVertices, 1)
    # the next frame of the sequence still matches the oracle
    mats, rows, desc, cam = s.step(2)
    r.update_skins([0], mats)
    r.update_instances([SHORT], [box_move(2, s.home)])
    r.set_camera(cam)
    r.run(s.st, 2)
    assert frame_diff(r, want, 2) == {}
    # rt_upload_scene drops the skins
    r.load_scene(desc0)
    with pytest.raises(RtError):
        r.update_skins([0], ident)
    r.destroy()


# ---- 7. steady state -------------------------------------------------------------------------------------------------------------------------------------
def test_steady_state_copies_no_vertices_and_resets_what_it_must(chk):
    W, H = SIZES[0]
    s = Sequence(chk, W, H)
    r = renderer(s.sc.desc(), W, H, 2)
    for f in range(4):      # past the probe frames: the context has decided its stream priorities
        _, _, _, cam = s.step(f)
        r.set_camera(cam)
        r.run(s.st, f)
    r.sync()
    before = r.stream_priorities()
    assert before["decided"]
    r.reference_render(s.st, 2)
    assert r.reference_samples() == 2
    r.set_skins(*skin.skins_table([s.sk]))
    assert r.reference_samples() == 0
    r.reference_render(s.st, 1)
    r.update_skins([0], s.matrices(4))
    assert r.reference_samples() == 0 and r.deform_stats().vertexBytesCopied == 0
    r.update_skins([0], s.matrices(5))
    st = r.deform_stats()
    assert (st.meshes, st.vertices, st.instances, st.vertexBytesCopied) == (1, s.sk.count, 1, 0) and st.skinMs > 0 and st.ms >= st.skinMs
    r.reference_render(s.st, 1)
    other = int(refit.instances_of(s.sc.desc())["primMesh"][SHORT])
    first, count = skin.mesh_range(s.sc.desc(), other)
    r.update_vertices(other, 0, skin.vertices_of(s.sc.desc())[first:first + count])
    assert r.reference_samples() == 0 and r.deform_stats().vertexBytesCopied == count * 32
    assert r.stream_priorities() == before
    r.destroy()
