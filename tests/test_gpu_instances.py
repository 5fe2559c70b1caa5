"""rt_set_instances on the GPU: after every table of tests/instances.py the device tree equals the CPU restatement of a device build over a fresh context's
host-built records (tests/accel_build_checker.cpp) word for word — leaf records with the alphaIdx word masked, whose numbering is per prim mesh by design —, rays
equal a fresh context's bit for bit, an update on top works, frames equal the oracle's, refused calls change nothing.  No tolerance anywhere: results are a
function of the triangle set, never of the tree.  The scenes, the ray generator and the Cornell sequence are those of tests/test_gpu_refit.py."""
import ctypes as C
import numpy as np
import pytest

from helpers import abi, frame_buffers
import accel_build
import instances
import optin
import refit
import test_gpu_accel_build as tab
import test_gpu_refit as seq

pytestmark = pytest.mark.gpu

SIZES = seq.SIZES
ALPHA_IDX_WORD = 11      # of the 16 words of a leaf record (csrc/bvh8.h Tri48)


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    d = tmp_path_factory.mktemp("instances_gpu")
    return accel_build.build(d), instances.build(d)


def expected_tree(L, desc, fresh):
    """the restated device build of `desc` over the records a fresh context host-built for it"""
    return accel_build.rebuilt(L, desc, tab.host_tree_of(L, fresh, desc, refit.Tree.built(L, desc)))


def tree_of(r, n_inst):
    return [r.accel_readback(w, n_inst).copy() for w in (abi.ACCEL_NODES, abi.ACCEL_TRIS, abi.ACCEL_INSTANCES)]


def diff_tree(r, t, n_inst):
    nodes, recs, inst = tree_of(r, n_inst)
    a, b = recs.view(np.uint32).reshape(-1, 16).copy(), t.recs.view(np.uint32).reshape(-1, 16).copy()
    if a.shape != b.shape:
        return {"records": (a.shape, b.shape)}
    a[:, ALPHA_IDX_WORD] = b[:, ALPHA_IDX_WORD] = 0
    return {"nodes": optin.words(nodes, t.nodes), "records": int((a != b).sum()), "instances": optin.words(inst, t.inst)}


SAME = {"nodes": 0, "records": 0, "instances": 0}


def steady_bytes(n_inst):
    return n_inst * 112 + (n_inst + 1) * 4 + 24      # rows, prefix words, the seed of the build's centre bounds (include/rt_abi.h)


def same_rays(r, fresh, rays):
    for mode in (abi.TRAVERSAL_THROUGHPUT, abi.TRAVERSAL_LATENCY):
        r.set_traversal(mode); fresh.set_traversal(mode)
        a, b = r.trace_closest(rays), fresh.trace_closest(rays)
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), mode
        assert np.array_equal(r.trace_any(rays), fresh.trace_any(rays)), mode
    return a


# ---- every table: tree, stats, rays, then an update on top -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", instances.TABLES)
def test_tree_rays_and_an_update_on_top(lib, name):
    L, IL = lib
    sc, steps = instances.tables(name)
    desc0 = sc.desc()
    r = seq.renderer(desc0)
    cur = refit.instances_of(desc0)
    tris_of = refit.prim_meshes_of(desc0)["indexCount"] // 3
    base = instances.mesh_alpha_base(IL, desc0)
    realloc, uploaded = [], []
    for label, table in steps:
        desc = instances.desc_with(desc0, table)
        n_inst, n = len(table), int(tris_of[table["primMesh"]].sum())
        assert instances.verdict(IL, instances.desc_with(desc0, cur), table)[0] == instances.OK
        r.set_instances(table)
        st = r.instances_stats()
        first = tree_of(r, n_inst)
        realloc.append(st.reallocated); uploaded.append(st.bytesUploaded)
        same = 0
        while same < min(len(cur), n_inst) and cur[same].tobytes() == table[same].tobytes():
            same += 1
        assert [st.instances, st.triangles, st.added, st.removed] == [n_inst, n, n_inst - same, len(cur) - same], label
        assert st.bytesUploaded >= steady_bytes(n_inst), label
        # the same table again: the same words, alphaIdx included, nothing allocated, the steady-state traffic
        r.set_instances(table)
        st = r.instances_stats()
        assert all(np.array_equal(a, b) for a, b in zip(first, tree_of(r, n_inst))), label
        assert [st.instances, st.triangles, st.added, st.removed, st.reallocated, st.bytesUploaded] == [n_inst, n, 0, 0, 0, steady_bytes(n_inst)], label
        # 1. the tree against a fresh context's
        fresh = seq.renderer(desc)
        t = expected_tree(L, desc, fresh)
        d = diff_tree(r, t, n_inst)
        print(name, label, d, "instances", n_inst, "triangles", n, "ms", round(st.ms, 3), "expand", round(st.expandMs, 3), "bytes", uploaded[-1], st.bytesUploaded)
        assert d == SAME, label
        dev = refit.Tree(L, desc, first[0], first[1], first[2], 0.0)
        dev.depth = r.rebuild_stats().levels
        assert accel_build.structure(L, dev) == (0, ""), label
        recs = first[1].view(refit.REC_DT)
        opaque = (recs["flags"] & instances.TRI_OPAQUE) != 0
        ref = refit.tri_ref(desc)[recs["globalId"]]
        assert np.array_equal(recs["alphaIdx"], np.where(opaque, 0, base[table["primMesh"][ref[:, 0]]] + ref[:, 1] + 1).astype(np.uint32)), label
        acc, rs = r.accel_stats(), r.rebuild_stats()
        assert [acc["nodes"], acc["triangles"], acc["references"], acc["max_depth"], acc["spatial_splits"]] == [t.num_nodes, t.num_recs, t.num_recs, t.depth, 0], label
        assert [rs.triangles, rs.nodes, rs.levels] == [t.num_recs, t.num_nodes, t.depth] and np.float32(rs.triPad) == np.float32(t.tri_pad), label
        # 2. rays
        ids, added = instances.aim_ids(cur, table)
        rays = seq.make_rays(desc, ids, instances.RAYS, instances.RAY_SEED[name])
        leaves = instances.alpha_added(cur, table)
        hits, aimed, alpha = instances.informative(desc, same_rays(r, fresh, rays), ids, leaves)
        print(name, label, "rays that hit:", hits, "on the aimed-at instances:", aimed, "on non-opaque triangles of an added instance:", alpha)
        assert hits > 400 and aimed > 20, label
        if name == "street" and leaves:
            assert alpha >= 20, label
        # 3. an update on top: the refit state re-derived by the call is the new tree's
        mover = next((i for i in added if tris_of[table["primMesh"][i]]), n_inst - 1)
        xf = np.stack([refit.move_matrix("rotate", desc, mover, refit.scene_extent(t))])
        assert t.refit([mover], xf) == 0
        r.update_instances([mover], xf)
        fresh.update_instances([mover], xf)
        d = diff_tree(r, t, n_inst)
        rst = r.refit_stats()
        assert d == SAME and t.check() == (0, ""), label
        assert [rst.instances, rst.leafRecords, rst.nodes, rst.levels, rst.fullRefit] == [1] + [int(x) for x in t.stats], label
        moved = table.copy()
        moved["objectToWorld"][mover] = xf[0]
        same_rays(r, fresh, seq.make_rays(instances.desc_with(desc0, moved), ids, instances.RAYS, instances.RAY_SEED[name] + 1))
        fresh.destroy()
        r.set_instances(table)      # the instance back where the table has it: the next step starts from the table
        cur = table
    if name == "one":               # the first call after a host build and the first growth that does not fit allocate; the shrink and a growth inside the capacity do not
        assert realloc == [1, 1, 0, 0]
    if name == "street_lazy":       # templates are made once per prim mesh: by the first table with a non-opaque instance of it, never again
        leaf_tris = int(sum(tris_of[m] for m in set(steps[0][1]["primMesh"][(steps[0][1]["flags"] & instances.FORCE_OPAQUE) == 0].tolist())))
        assert uploaded[0] == steady_bytes(len(steps[0][1])) + 4 * desc0.numPrimMeshes + 80 * leaf_tris
        assert uploaded[1:] == [steady_bytes(len(t)) for _, t in steps[1:]]
    r.destroy()


def test_skins_follow_on_the_new_tree(lib, tmp_path):
    """street: rt_update_skins of the tree mesh after a call that added an instance of it — every instance of the mesh, the new one included, is refitted, and the
    rays equal those of a fresh context that was given the same table and the same pose"""
    import skin
    L, IL = lib
    chk = skin.build(tmp_path)
    sc, steps = instances.tables("street")
    desc0 = sc.desc()
    label, table = steps[0]
    desc = instances.desc_with(desc0, table)
    ids, added = instances.aim_ids(refit.instances_of(desc0), table)
    mesh = int(table["primMesh"][added[0]])
    out = []
    for which in range(2):
        r = seq.renderer(desc0 if which == 0 else desc)
        if which == 0:
            r.set_instances(table)
        sk = skin.SkinnedMesh(chk, desc, mesh, 3)
        r.set_skins(*skin.skins_table([sk]))
        r.update_skins([0], sk.matrices("bend", 60.0))
        assert r.deform_stats().instances == int((table["primMesh"] == mesh).sum()) == 3
        out.append((r, r.vertices_readback(0, desc.numVertices)))
    (r, va), (fresh, vb) = out
    assert np.array_equal(va, vb)
    same_rays(r, fresh, seq.make_rays(desc, ids, instances.RAYS, 5))
    r.destroy(); fresh.destroy()


# ---- frames: the Cornell sequence of tests/test_gpu_refit.py with the table changing on frames 2, 4, 5 and 7 ---------------------------------------------------
def table_plan(f, desc):
    """the extra instances (behind the scene's six, so the emitter stays at its index) from frame f on: add, remove, add with a mirrored matrix, remove"""
    extra = {2: [("rotate", (0.15, 0.0, -0.3))], 4: [], 5: [("mirror", (-0.7, 0.62, 0.1))], 7: []}
    if f not in extra:
        return None
    return [instances.placed(desc, 3, kind, shift=shift) for kind, shift in extra[f]]


class Frames(seq.Sequence):
    """test_gpu_refit.Sequence with a changing table: the scene object follows through Scene.setInstances, the moves of plan() go on on top"""
    cache = {}

    def step(self, f):
        """(the new table when frame f changes it — with the matrices of frame f - 1, which the moves of frame f then follow —, else None; ids, xf, desc, camera)"""
        new = table_plan(f, self.sc.desc())
        table = None
        if new is not None:
            table = np.concatenate([refit.instances_of(self.sc.desc())[:6]] + new)
            self.sc.setInstances(table)
        return (table,) + super().step(f)

    @classmethod
    def oracle_frames(cls, W, H, frames=seq.FRAMES):
        """the oracle is given each frame's description, as test_gpu_refit.Sequence.oracle_frames does: its history carry takes a changed instance count"""
        from oracle.binding import Oracle
        if (W, H) not in cls.cache:
            s = cls(W, H)
            o = Oracle(0)
            o.upload_scene(s.sc.desc())
            o.resize(W, H)
            out = []
            for f in range(frames):
                desc, cam = s.step(f)[-2:]
                o.upload_scene(desc)
                o.set_camera(cam)
                o.render_frame(s.st, f)
                out.append({b: o.readback(b).copy() for b in frame_buffers(f)})
            cls.cache[(W, H)] = out
        return cls.cache[(W, H)]


def run_frames(W, H, overlap, traversal, frames=seq.FRAMES, after=None):
    want = Frames.oracle_frames(W, H)
    s = Frames(W, H)
    r = seq.renderer(s.sc.desc(), W, H, overlap, traversal)
    bad = {}
    for f in range(frames):
        table, ids, xf, desc, cam = s.step(f)
        if table is not None:
            r.set_instances(table)
        r.update_instances(ids, xf)
        r.update_lights(desc)
        r.set_camera(cam)
        r.run(s.st, f)
        if after:
            after(r, s, f)
        for b in frame_buffers(f):
            d = optin.words(r.readback(b), want[f][b])
            if d:
                bad[(f, abi.BUFFER_NAMES[b])] = d
    return r, s, bad


@pytest.mark.parametrize("W,H", SIZES)
@pytest.mark.parametrize("traversal", [abi.TRAVERSAL_THROUGHPUT, abi.TRAVERSAL_LATENCY])
@pytest.mark.parametrize("overlap", [0, 2])
def test_frames_equal_the_oracle(W, H, overlap, traversal):
    r, s, bad = run_frames(W, H, overlap, traversal)
    r.destroy()
    assert bad == {}
    want = Frames.oracle_frames(W, H)       # the added boxes are in view: the frames differ from the sequence without them
    plain = seq.Sequence.oracle_frames(W, H)
    assert all(optin.words(want[f][abi.BUF_GBUFFER0 + (f & 1)], plain[f][abi.BUF_GBUFFER0 + (f & 1)]) > 0 for f in (2, 3, 5, 6))
    assert all(optin.words(want[f][abi.BUF_GBUFFER0 + (f & 1)], plain[f][abi.BUF_GBUFFER0 + (f & 1)]) == 0 for f in (0, 1))


@pytest.mark.parametrize("which", ["svgf", "gi_spatial", "taa", "vertex_motion"])
def test_a_changing_table_with_an_opt_in_pass(tmp_path, which):
    """the histories survive the call: every frame, the ones after a call included, equals the oracle's / the pass's checker"""
    import gi_spatial
    W, H = SIZES[1]
    kw = {"svgf": dict(den=abi.Denoiser(mode=abi.DENOISER_SVGF)), "gi_spatial": dict(gis=abi.GiSpatial(mode=abi.GI_SPATIAL_VISIBILITY)), "taa": dict(t=abi.Taa(mode=abi.TAA_ON)),
          "vertex_motion": {}}[which]
    rig = optin.Rig(tmp_path, abi.PROC_CORNELL, 1.0, None, W, H, overlap=2, **kw)
    if which == "vertex_motion":
        rig.r.set_object_motion(abi.OBJECT_MOTION_VERTEX)
    home = refit.instances_of(rig.sc.desc())
    for f in range(6):
        new = table_plan(f, instances.desc_with(rig.sc.desc(), home))
        if new is not None:
            table = np.concatenate([home] + new)
            if which == "vertex_motion":    # a move the call makes the motion state forget: the previous matrices become the current ones
                rig.r.update_instances([3], refit.move_matrix("translate", rig.sc.desc(), 3, 1.0)[None])
            rig.sc.setInstances(table)
            rig.r.set_instances(table)
            desc = rig.sc.desc()
            rig.o.upload_scene(desc)
            rig.kg = gi_spatial.GiSpatialChecker(gi_spatial.build(tmp_path), desc)
            rig.desc = desc
        rig.frame(f)
        assert rig.diff(f) == {}, f
    n = rig.history_lengths()
    if which in ("svgf", "taa"):
        assert set(n) == ({"svgf_direct", "svgf_indirect"} if which == "svgf" else {"taa"}), sorted(n)
        assert all(v.max() >= 3 for v in n.values()), {k: v.max() for k, v in n.items()}     # carried across the calls, not dropped
    rig.destroy()


# ---- contract ------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", instances.REFUSALS)
def test_refused_tables_change_nothing(lib, name):
    from restir_amd.renderer import hip_lib
    L, IL = lib
    sc, cases = instances.refusals(name)
    desc = sc.desc()
    n_inst = desc.numInstances
    r = seq.renderer(desc)
    if name == "cornell":       # on a device-built tree with the call's own buffers in place
        r.set_instances(refit.instances_of(desc))
    state, stats = tree_of(r, n_inst), bytes(r.instances_stats())
    rays = seq.make_rays(desc, [0], 512, 3)
    hits = r.trace_closest(rays).copy()
    for label, table, code, offender in cases:
        assert instances.verdict(IL, desc, table)[0] == code, label
        t = None if table is None else instances.rows(table)
        keep = np.zeros(1, instances.DT) if t is not None and len(t) == 0 else t
        rc = hip_lib().rt_set_instances(r._h, 1 if t is None else len(t), None if t is None else keep.ctypes.data)
        msg = hip_lib().rt_last_error(r._h).decode()
        assert rc == abi.ERR_INVALID_ARG and instances.MESSAGE[code] in msg, (label, rc, msg)
        if code in instances.PER_INSTANCE:
            assert ("instance %d:" % offender) in msg, (label, msg)
        assert all(np.array_equal(a, b) for a, b in zip(state, tree_of(r, n_inst))), label
        assert bytes(r.instances_stats()) == stats, label
    assert np.array_equal(r.trace_closest(rays).view(np.uint32), hits.view(np.uint32))
    # ... and the table is the old one: its last instance exists and can be moved (to where it is: the rows and every hit stay; a host-built tree's boxes may be
    # requantised by the refit, so the nodes are not compared)
    r.update_instances([n_inst - 1], refit.instances_of(desc)["objectToWorld"][n_inst - 1:])
    assert np.array_equal(state[2], tree_of(r, n_inst)[2])
    assert np.array_equal(r.trace_closest(rays).view(np.uint32), hits.view(np.uint32))
    r.destroy()


def test_an_instance_a_binding_names_is_held_in_place(lib, tmp_path):
    """the emitter rule covers what a light-source binding names, emissive or not: the checker's verdict and the library's agree, and without the binding the table passes"""
    import lights
    from restir_amd.renderer import Renderer, hip_lib
    L, IL = lib
    sc, desc, src, bound, box, moved = instances.bound_box_scene(lights.build(tmp_path))
    r = Renderer().setup(0)
    r.load_scene(desc)
    r.set_light_sources(src)
    r.set_instances(refit.instances_of(desc))       # the table as it is: accepted with the binding in place
    state = tree_of(r, len(moved))
    for table in (moved, np.delete(moved, box)):
        assert instances.verdict(IL, desc, table, bound=bound) == (instances.EMITTER_CHANGED, box)
        t = instances.rows(table)
        rc = hip_lib().rt_set_instances(r._h, len(t), t.ctypes.data)
        msg = hip_lib().rt_last_error(r._h).decode()
        assert rc == abi.ERR_INVALID_ARG and instances.MESSAGE[instances.EMITTER_CHANGED] in msg and ("instance %d:" % box) in msg, (rc, msg)
        assert all(np.array_equal(a, b) for a, b in zip(state, tree_of(r, len(moved))))
    r.set_light_sources(np.zeros(0, abi.LIGHT_SOURCE_DT))       # the binding removed: the box may move, as the checker says
    assert instances.verdict(IL, desc, moved) == (instances.OK, 0)
    r.set_instances(moved)
    assert np.array_equal(r.accel_readback(abi.ACCEL_INSTANCES, len(moved)).view(np.float32).reshape(-1, 28)[box, :12], moved["objectToWorld"][box])
    r.destroy()


def test_before_a_scene_and_before_a_build():
    from restir_amd.renderer import Renderer, hip_lib
    sc = refit.cornell()
    desc = sc.desc()
    table = refit.instances_of(desc)
    r0 = Renderer().setup(0)
    assert hip_lib().rt_set_instances(r0._h, len(table), table.ctypes.data) == abi.ERR_NO_SCENE
    assert hip_lib().rt_upload_scene(r0._h, C.byref(desc)) == 0
    assert hip_lib().rt_set_instances(r0._h, len(table), table.ctypes.data) == abi.ERR_NO_ACCEL
    r0.destroy()


def test_reference_sums_restart_priorities_stay_and_a_later_host_build_matches():
    W, H = SIZES[0]
    want = Frames.oracle_frames(W, H)
    s = Frames(W, H)
    r = seq.renderer(s.sc.desc(), W, H, 2)
    for f in range(4):      # past the probe frames: the context has decided; frame 2 changes the table
        table, ids, xf, desc, cam = s.step(f)
        if f == 2:
            r.sync()
            before = r.stream_priorities()
            r.reference_render(s.st, 2)
            assert r.reference_samples() == 2
            r.set_instances(table)
            assert r.reference_samples() == 0
            assert r.stream_priorities() == before
        r.update_instances(ids, xf)
        r.update_lights(desc)
        r.set_camera(cam)
        r.run(s.st, f)
    for f in (4, 5):        # frame 4 removes the box again; frame 5 adds the mirrored one and is rendered after a host build of the new scene
        table, ids, xf, desc, cam = s.step(f)
        r.sync()
        before = r.stream_priorities()
        assert before["decided"]
        r.set_instances(table)
        assert r.stream_priorities() == before
        r.update_instances(ids, xf)
        if f == 5:
            assert refit.hip_build_accel(r) == 0
            assert r.accel_stats()["triangles"] == len(refit.tri_ref(desc))
        r.update_lights(desc)
        r.set_camera(cam)
        r.run(s.st, f)
        assert {abi.BUFFER_NAMES[b]: optin.words(r.readback(b), want[f][b]) for b in frame_buffers(f) if optin.words(r.readback(b), want[f][b])} == {}, f
    r.destroy()


def test_a_kept_emitter_still_moves_its_light_records(tmp_path):
    """with a light-source binding set, rt_update_instances of the emitter after the call rewrites its records: rt_lights_readback against tests/light_checker.cpp"""
    import lights
    W, H = SIZES[0]
    sc = refit.cornell()
    desc = sc.desc()
    r = seq.renderer(desc, W, H)
    src = sc.lightSources()
    r.set_light_sources(src)
    table = np.concatenate([refit.instances_of(desc), instances.placed(desc, 3, "rotate", shift=(0.15, 0.0, -0.3))])
    r.set_instances(table)
    em = int(refit.describe(desc)["emissive"][0])
    xf = refit.compose(refit.translation([0.2, -0.1, 0.1]), table["objectToWorld"][em])[None]
    r.update_instances([em], xf)
    moved = table.copy()
    moved["objectToWorld"][em] = xf[0]
    want, cnt = lights.rewrite(lights.build(tmp_path), instances.desc_with(desc, moved), src, lights.records_of(desc), dirty=[em])
    assert cnt == len(src) == r.light_stats().rewritten == 2
    got = r.lights_readback(abi.LIGHTS_TRIG, len(src))
    assert np.array_equal(lights.raw(got), lights.raw(want))
    assert not np.array_equal(lights.raw(got), lights.raw(lights.records_of(desc)))
    r.destroy()
