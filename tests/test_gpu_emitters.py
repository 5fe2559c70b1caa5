"""The emitter mode on the GPU (rt_set_emitter_meshes): with the mode on, rt_set_instances adds, removes and re-indexes emissive instances, and the
device light array equals the CPU restatement (tests/light_derive_checker.cpp) and the records host.Scene.setInstances computes, word for word, all 96 bytes; the
update calls move a spawned emitter's records; frames of a lamp that appears, moves and disappears equal the oracle's bit for bit without any rt_update_lights;
with the mode off the emitter rule holds as before; refused calls change nothing; the mode's life cycle and the growth of its buffers.  No tolerance anywhere."""
import numpy as np
import pytest

from helpers import abi, frame_buffers
from oracle.binding import Oracle
import emitters
import instances
import lights
import optin
import refit
import skin
import test_gpu_refit as seq

pytestmark = pytest.mark.gpu

SIZES = seq.SIZES
LAMP = 5      # Cornell's ceiling light (instance and prim mesh)


@pytest.fixture(scope="module")
def chk(tmp_path_factory):
    return emitters.build(tmp_path_factory.mktemp("emitters"))


@pytest.fixture(scope="module")
def skc(tmp_path_factory):
    return skin.build(tmp_path_factory.mktemp("skin"))


def switch_on(r, sc):
    meshes, rows = sc.emitterMeshes()
    r.set_emitter_meshes(meshes, rows, sc.lightWeights[0])
    return meshes, rows


def trig(r):
    return r.lights_readback(abi.LIGHTS_TRIG, r.emitter_stats().records)


def light_state(r, n):
    """everything of the lights a refused call must leave alone (n: the device's triangle-light records)"""
    return lights.raw(r.lights_readback(abi.LIGHTS_TRIG, n)).copy(), bytes(r.light_stats()), bytes(r.emitter_stats()), bytes(r.instances_stats())


def same_state(a, b):
    return np.array_equal(a[0], b[0]) and a[1:] == b[1:]


def call_refused(fn, *fragments):
    from restir_amd.renderer import RtError
    with pytest.raises(RtError) as e:
        fn()
    msg = str(e.value)
    assert "(%d)" % abi.ERR_INVALID_ARG in msg and all(f in msg for f in fragments), msg
    return msg


# ---- 1. records word for word ---------------------------------------------------------------------------------------------------------------------------------
def test_records_equal_the_checker_and_the_scene_word_for_word(tmp_path, chk, skc):
    counts = (1, 63, 64, 65, 257)      # triangles per emissive mesh: below a wave ... above one 256-thread block
    em = lights.Emitters(tmp_path, counts, plain=29, mirror_of=3)
    sc = em.sc
    desc0 = sc.desc()
    assert 34 in refit.describe(desc0)["mirrored"] and sorted(int(i) for i in refit.describe(desc0)["emissive"]) == [29, 30, 31, 32, 33, 34]
    from restir_amd.renderer import Renderer
    r = Renderer().setup(0)
    r.load_scene(desc0)
    before = lights.raw(r.lights_readback(abi.LIGHTS_TRIG, desc0.lightInfo.trigLightSize)).copy()
    meshes, rows = switch_on(r, sc)
    punc = sc.lightWeights[0]
    st = r.emitter_stats()
    assert [st.enabled, st.records, st.emittingInstances] == [1, sum(counts) + 65, 6] and r.light_stats().bound == st.records
    assert st.bytesUploaded == rows.size * 32 + desc0.numPrimMeshes * 4 + emitters.bus_bytes(st.records, 6)
    assert np.array_equal(lights.raw(trig(r)), before)      # switching the mode on changes no bit
    vertices = r.vertices_readback(0, desc0.numVertices).copy()
    info = emitters.info_of(desc0)
    base = refit.instances_of(desc0)      # (taken now: Scene.setInstances replaces the array desc0 points at)
    spawn = instances.placed(desc0, em.emitter[3], "scale", shift=(0.3, 0.2, -0.4))
    sizes = []
    for label, table in emitters.sequence(desc0):
        sc.setInstances(table)
        desc = sc.desc()
        rec, src, info, emitting = emitters.derive(chk, desc, table, meshes, rows, punc, info)
        r.set_instances(table)
        got, st, ls = trig(r), r.emitter_stats(), r.light_stats()
        scn = lights.records_of(desc)
        print(label, "records", st.records, "emitting", st.emittingInstances, "bytes", st.bytesUploaded, "reallocated", st.reallocated, "k_light_expand ms", round(st.expandMs, 4),
              "differs from checker / scene in", optin.words(got, rec), optin.words(got, scn), "words")
        assert [st.enabled, st.records, st.emittingInstances] == [1, rec.size, emitting] and rec.size == scn.size == desc.lightInfo.trigLightSize, label
        assert np.array_equal(lights.raw(got), lights.raw(rec)), label
        assert np.array_equal(lights.raw(got), lights.raw(scn)), label
        assert [ls.bound, ls.rewritten, ls.lightBytesCopied] == [rec.size, 0, 0], label
        assert st.bytesUploaded == emitters.bus_bytes(rec.size, emitting), label
        assert r.deform_stats().vertexBytesCopied == 0 and np.array_equal(r.vertices_readback(0, desc0.numVertices), vertices), label      # no vertex byte moved
        r.set_instances(table)      # the same table again: the same words, from the other set of buffers
        assert np.array_equal(lights.raw(trig(r)), lights.raw(got)) and r.emitter_stats().bytesUploaded == st.bytesUploaded, label
        assert r.instances_stats().bytesUploaded == len(table) * 112 + (len(table) + 1) * 4 + 24, label      # the call's own steady-state traffic, as with the mode off
        sizes.append(rec.size)
    assert 0 in sizes and sizes[-1] == desc0.lightInfo.trigLightSize and len(set(sizes)) > 3
    # a spawned emitter follows the update calls through the binding: exactly its records are rewritten
    spawned = len(base)
    table = np.concatenate([base, spawn])
    sc.setInstances(table)
    r.set_instances(table)
    n = sc.desc().lightInfo.trigLightSize
    assert n == desc0.lightInfo.trigLightSize + 65 and r.light_stats().bound == n
    cur = trig(r)
    assert np.array_equal(lights.raw(cur), lights.raw(lights.records_of(sc.desc())))
    src = sc.lightSources()
    xf = refit.compose(refit.scaling((-1.2, 0.7, 1.1), (0.5, 0.0, 0.5)), table["objectToWorld"][spawned])[None]      # mirrored and non-uniformly scaled
    sc.updateInstances([spawned], xf)
    r.update_instances([spawned], xf)
    got = trig(r)
    mine = src["instance"] == spawned
    assert mine.sum() == 65 and r.light_stats().rewritten == 65 and r.light_stats().lightBytesCopied == 0
    assert np.array_equal(lights.raw(got), lights.raw(lights.records_of(sc.desc())))
    assert np.array_equal(lights.raw(got)[~mine], lights.raw(cur)[~mine]) and not np.array_equal(lights.raw(got)[mine], lights.raw(cur)[mine])
    sk = skin.SkinnedMesh(skc, sc.desc(), em.prim_mesh(3), 3)      # the 65-triangle mesh: its plain, its mirrored and its spawned instance follow
    r.set_skins(*skin.skins_table([sk]))
    mats = sk.matrices("bend", 2.0)
    sc.updateVertices(sk.mesh, 0, sk.posed(mats))
    r.update_skins([0], mats)
    assert r.light_stats().rewritten == 3 * 65 and r.deform_stats().vertexBytesCopied == 0
    assert np.array_equal(lights.raw(trig(r)), lights.raw(lights.records_of(sc.desc())))
    r.destroy()


# ---- 2. frames: the Cornell sequence of tests/test_gpu_refit.py with a second ceiling lamp that appears, moves and disappears ----------------------------------
class Frames(seq.Sequence):
    """a second ceiling lamp appears on frame 2, moves on frame 4 and disappears on frame 5; on frame 7 all lamps are gone.  The box and the first lamp go on
    moving as in the sequence (while they exist); the scene object follows through Scene.setInstances / updateInstances"""
    cache = {}

    def step(self, f):
        """(the new table when frame f changes it, else None; ids, xf of the frame's moves; desc; camera)"""
        cur = refit.instances_of(self.sc.desc())
        table = None
        if f == 2:
            table = np.concatenate([cur[:6], instances.placed(self.sc.desc(), LAMP, "rotate", shift=(-0.55, 0.0, 0.45))])
        elif f == 5:
            table = cur[:6]
        elif f == 7:
            table = cur[:5]
        if table is not None:
            self.sc.setInstances(table)
        ids, xf = seq.plan(f, self.home)
        if f == 4:      # the spawned lamp moves: through the binding on the device
            ids, xf = ids + [6], np.concatenate([xf, refit.compose(refit.translation((0.12, 0.0, -0.2)), cur[6]["objectToWorld"])[None]])
        if f >= 7:
            ids, xf = ids[:1], xf[:1]
        self.sc.updateInstances(ids, xf)
        eye, center, up, fov = self.pose
        a = 0.06 * f
        d = np.asarray(eye, np.float64) - center
        e = center + np.array([np.cos(a) * d[0] + np.sin(a) * d[2], d[1], -np.sin(a) * d[0] + np.cos(a) * d[2]])
        self.sc.setCamera(e.astype(np.float32), center, up, fov)
        self.sc.updateCamera(self.W, self.H)
        self.st.time = 1000 + f
        return table, ids, xf, self.sc.desc(), self.sc.getCamera()

    @classmethod
    def oracle_frames(cls, W, H, frames=seq.FRAMES):
        """the oracle is given each frame's Scene description (its history carries over a scene upload, a changed light count included)"""
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


@pytest.mark.parametrize("W,H", SIZES)
@pytest.mark.parametrize("traversal", [abi.TRAVERSAL_THROUGHPUT, abi.TRAVERSAL_LATENCY])
@pytest.mark.parametrize("overlap", [0, 2])
def test_frames_equal_the_oracle_without_update_lights(W, H, overlap, traversal):
    want = Frames.oracle_frames(W, H)
    s = Frames(W, H)
    r = seq.renderer(s.sc.desc(), W, H, overlap, traversal)
    switch_on(r, s.sc)
    bad, counts = {}, []
    for f in range(seq.FRAMES):
        table, ids, xf, desc, cam = s.step(f)
        if table is not None:
            r.set_instances(table)
        r.update_instances(ids, xf)
        r.set_camera(cam)
        r.run(s.st, f)
        for b in frame_buffers(f):
            d = optin.words(r.readback(b), want[f][b])
            if d:
                bad[(f, abi.BUFFER_NAMES[b])] = d
        counts.append(r.light_stats().bound)
        assert np.array_equal(lights.raw(trig(r)), lights.raw(lights.records_of(desc))), f
    r.destroy()
    print("records per frame", counts, "differing words", bad)
    assert counts == [2, 2, 4, 4, 4, 2, 2, 0]
    assert bad == {}
    # control: the sequence without the second lamp gives another direct image while the lamp exists, and the same one before
    plain = seq.Sequence.oracle_frames(W, H)
    direct = lambda f: abi.BUF_DIRECT_RESULT0 + (f & 1)      # noqa: E731
    assert all(optin.words(want[f][direct(f)], plain[f][direct(f)]) > 0 for f in (2, 3, 4, 7))
    assert all(optin.words(want[f][direct(f)], plain[f][direct(f)]) == 0 for f in (0, 1))


# ---- 3. mode off: the emitter rule, as before -------------------------------------------------------------------------------------------------------------------
def test_with_the_mode_off_the_emitter_rule_holds():
    sc = refit.cornell()
    desc = sc.desc()
    base = refit.instances_of(desc)
    added = np.concatenate([base, instances.placed(desc, LAMP, "rotate", shift=(-0.55, 0.0, 0.45))])
    r = seq.renderer(desc)
    r.set_instances(base)
    assert r.emitter_stats().enabled == 0
    for round_ in range(2):
        state = light_state(r, 2)
        call_refused(lambda: r.set_instances(added), "instance 6:", instances.MESSAGE[instances.EMITTER_ADDED])
        call_refused(lambda: r.set_instances(base[:5]), "instance 5:", instances.MESSAGE[instances.EMITTER_CHANGED])
        assert same_state(state, light_state(r, 2))
        if round_ == 0:      # on: accepted; off again: the rule applies to the table as it is now
            switch_on(r, sc)
            r.set_instances(added)
            assert r.light_stats().bound == 4
            r.set_instances(base)
            r.set_emitter_meshes()
            assert r.emitter_stats().enabled == 0 and r.light_stats().bound == 2
    r.destroy()


# ---- 4. refusals and life cycle -----------------------------------------------------------------------------------------------------------------------------
def test_refused_calls_change_nothing():
    W, H = SIZES[0]
    sc = refit.street()
    desc = sc.desc()
    base = refit.instances_of(desc)
    st = seq.host.default_state(W, H, sc, None)
    st.environmentProb = 0.0
    sc.updateCamera(W, H)
    cam = sc.getCamera()
    meshes, rows = sc.emitterMeshes()
    assert len(meshes) == 2
    a, b = (int(m) for m in meshes["primMesh"])
    plain_mesh = int(base["primMesh"][0])
    assert plain_mesh not in (a, b)

    def edit(arr, i, field, value):
        out = arr.copy()
        out[field][i] = value
        return out

    def uv(i, value):
        out = rows.copy()
        out["uv"][i][3] = value
        return out

    frames = {}
    for which in ("control", "refusals"):
        r = seq.renderer(desc, W, H, 0, abi.TRAVERSAL_THROUGHPUT)
        r.set_camera(cam)
        st.time = 1000
        r.run(st, 0)
        if which == "refusals":
            for round_ in range(2):      # with the mode off, then with it on: a refused switch leaves it as it was
                state = light_state(r, 96)
                on = lambda m, w, p=0.0: (lambda: r.set_emitter_meshes(m, w, p))      # noqa: E731
                call_refused(on(edit(meshes, 1, "primMesh", desc.numPrimMeshes), rows), "template 1", "prim mesh out of range")
                call_refused(on(edit(meshes, 1, "primMesh", a), rows), "template 1", "listed twice")
                call_refused(on(edit(meshes, 0, "primMesh", plain_mesh), rows), "template 0", "not emissive")
                call_refused(on(meshes[:1], rows), "emissive prim mesh %d has no emitter template" % b, "instance %d:" % int(np.nonzero(base["primMesh"] == b)[0][0]))
                call_refused(on(edit(meshes, 1, "rowCount", meshes["rowCount"][1] + 1), rows), "template 1", "row range outside rows")
                call_refused(on(meshes, edit(rows, 50, "triangle", 48)), "template 1", "row 50", "triangle beyond")
                call_refused(on(meshes, uv(3, np.nan)), "template 0", "row 3", "non-finite uv")
                call_refused(on(meshes, rows, np.inf), "puncLightWeight")
                call_refused(on(meshes, rows, 1.0), "trigSampProb")                                              # inconsistent: another punctual weight
                call_refused(on(meshes, uv(70, 0.123)), "record 70 ", "row 22 of instance %d" % int(np.nonzero(base["primMesh"] == b)[0][0]))      # ... another texcoord
                call_refused(on(meshes, np.concatenate([rows[:48], rows[49:96], rows[48:49]])), "record 48 ")   # ... another order of triangles
                call_refused(on(edit(meshes, 1, "rowCount", 47), rows), "derive 95 records, the device holds 96")
                assert r.emitter_stats().enabled == round_ and same_state(state, light_state(r, 96))
                if round_ == 0:
                    switch_on(r, sc)
            call_refused(lambda: r.set_light_sources(sc.lightSources()), "emitter mode is on")
            # a table that uses an emissive prim mesh without a template
            gone = base[base["primMesh"] != b]
            r.set_instances(gone)
            r.set_emitter_meshes(meshes[:1], rows, 0.0)      # accepted: mesh b has no instance now
            state = light_state(r, 48)
            call_refused(lambda: r.set_instances(base), "instance %d:" % int(np.nonzero(base["primMesh"] == b)[0][0]), "has no emitter template")
            assert same_state(state, light_state(r, 48))
            switch_on(r, sc)
            r.set_instances(base)
            assert np.array_equal(lights.raw(trig(r)), lights.raw(lights.records_of(desc)))
        st.time = 1001
        r.run(st, 1)
        frames[which] = {b_: r.readback(b_).copy() for b_ in frame_buffers(1)}
        r.destroy()
    assert all(optin.words(frames["control"][b_], frames["refusals"][b_]) == 0 for b_ in frames["control"])


def test_stale_records_refuse_the_switch():
    sc = refit.cornell()
    desc = sc.desc()
    r = seq.renderer(desc)
    xf = refit.compose(refit.translation((0.1, 0.0, 0.0)), refit.instances_of(desc)["objectToWorld"][LAMP])[None]
    r.update_instances([LAMP], xf)      # no binding: the light records stay where they were uploaded
    state = light_state(r, 2)
    meshes, rows = sc.emitterMeshes()
    call_refused(lambda: r.set_emitter_meshes(meshes, rows, 0.0), "record 0 ", "row 0 of instance 5", "rt_update_lights first")
    assert same_state(state, light_state(r, 2)) and r.emitter_stats().enabled == 0
    sc.updateInstances([LAMP], xf)
    r.update_lights(sc.desc())
    switch_on(r, sc)
    assert r.emitter_stats().enabled == 1
    r.destroy()


def test_life_cycle_and_capacity(chk):
    W, H = SIZES[0]
    sc = refit.cornell()
    desc = sc.desc()
    base = refit.instances_of(desc)
    lamps = [instances.placed(desc, LAMP, "rotate", shift=(-0.6 + 0.3 * k, 0.0, 0.5)) for k in range(5)]
    lamp = lambda k: lamps[k]      # noqa: E731
    r = seq.renderer(desc, W, H)
    meshes, rows = switch_on(r, sc)

    def set_and_check(table, label):
        sc.setInstances(table)
        r.set_instances(table)
        rec = emitters.derive(chk, sc.desc(), table, meshes, rows, 0.0, emitters.info_of(desc))[0]
        got = trig(r)
        assert np.array_equal(lights.raw(got), lights.raw(rec)) and np.array_equal(lights.raw(got), lights.raw(lights.records_of(sc.desc()))), label
        return r.emitter_stats().reallocated

    one = np.concatenate([base, lamp(0)])
    # each of the two sets of light buffers is allocated by the first call that writes it; then nothing is
    assert [set_and_check(one, "first"), set_and_check(one, "second"), set_and_check(base, "third"), set_and_check(one, "fourth")] == [1, 1, 0, 0]
    for what, fn in (("rt_build_accel", lambda: refit.hip_build_accel(r)), ("rt_rebuild_accel", r.rebuild_accel), ("rt_resize", lambda: r.update(SIZES[1][0], SIZES[1][1]))):
        fn()
        assert r.emitter_stats().enabled == 1, what
        assert set_and_check(base if what == "rt_rebuild_accel" else one, what) == 0, what      # an emitter added or removed: the mode is still on
    # a table that outgrows the slack: 4 records of capacity (4 + 4 / 8), 12 wanted
    many = np.concatenate([base] + [lamp(k) for k in range(5)])
    assert set_and_check(many, "grown") == 1 and r.light_stats().bound == 12
    assert set_and_check(many, "grown, the other set") == 1
    assert [set_and_check(many, "fits"), set_and_check(one, "shrunk"), set_and_check(many, "fits again")] == [0, 0, 0]
    assert set_and_check(base[:5], "no lamp") == 0 and r.light_stats().bound == 0
    assert set_and_check(many, "from none to many") == 0
    # rt_upload_scene drops the mode: the emitter rule is back
    sc.setInstances(base)
    r.load_scene(sc.desc())
    assert r.emitter_stats().enabled == 0
    call_refused(lambda: r.set_instances(one), instances.MESSAGE[instances.EMITTER_ADDED])
    r.destroy()
