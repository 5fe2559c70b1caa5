"""Light sources on the GPU (rt_set_light_sources): after rt_update_instances, rt_update_vertices and rt_update_skins the device light array equals the
CPU restatement (tests/light_checker.cpp) and the records host.Scene recomputes, word for word; frames of a deformed or moved emitter equal the oracle rendering
the Scene-updated description bit for bit without any rt_update_lights; refused bindings change nothing; the binding's life cycle.  No tolerance anywhere."""
import ctypes as C
import numpy as np
import pytest

from helpers import abi, frame_buffers
from oracle.binding import Oracle
import lights
import objmotion
import optin
import refit
import skin
import test_gpu_skin as deform      # the Cornell "light" sequence: the ceiling light's +x half turns a little more every frame

pytestmark = pytest.mark.gpu

SIZES = ((64, 48), (67, 45))
LIGHT, SHORT = 5, 3      # Cornell's ceiling light and short box (instances)
FRAMES = 4
KEEP = np.ones(96, bool)
KEEP[lights.POS] = False      # the bytes of a record no update may touch


@pytest.fixture(scope="module")
def chk(tmp_path_factory):
    return lights.build(tmp_path_factory.mktemp("lights"))


@pytest.fixture(scope="module")
def skc(tmp_path_factory):
    return skin.build(tmp_path_factory.mktemp("skin"))


def trig(r, n):
    return r.lights_readback(abi.LIGHTS_TRIG, n)


def stats(r):
    s = r.light_stats()
    return (s.bound, s.rewritten, s.lightBytesCopied)


# ---- 1. records word for word -----------------------------------------------------------------------------------------------------------------------------
def test_records_equal_the_checker_and_the_scene_word_for_word(tmp_path, chk, skc):
    counts = (1, 63, 64, 65, 257)      # triangles per emissive mesh: below a wave ... above one 256-thread block
    em = lights.Emitters(tmp_path, counts, plain=29, mirror_of=3)
    sc = em.sc
    desc = sc.desc()
    inst = refit.instances_of(desc)
    e1, e63, e64, e65, e257 = (em.emitter[m] for m in range(5))
    assert (e64, e65, e257) == (31, 32, 33) and em.mirrored == 34      # emitters on both sides of the boundary of a dirty-bit word
    assert sorted(int(i) for i in refit.describe(desc)["emissive"]) == [29, 30, 31, 32, 33, 34] and 34 in refit.describe(desc)["mirrored"]
    n = desc.lightInfo.trigLightSize
    assert n == sum(counts) + 65 and n > 2 * 256
    perm = lights.interleave(n)      # the binding lists the records interleaved, not grouped by instance
    rec0, src = lights.permuted(lights.records_of(desc), sc.lightSources(), perm)
    assert (np.diff(src["instance"].astype(np.int64)) != 0).mean() > 0.5
    scene_records = lambda: lights.records_of(sc.desc())[perm]      # noqa: E731  (only v0 v1 v2 of the scene's records ever change)

    from restir_amd.renderer import Renderer
    r = Renderer().setup(0)
    r.load_scene(lights.with_lights(desc, rec0))
    r.set_light_sources(src)
    assert stats(r) == (n, 0, 0)
    assert np.array_equal(lights.raw(trig(r, n)), lights.raw(rec0))      # switching the binding on changes no bit
    cur = rec0

    def check(what, dirty, expect):
        nonlocal cur
        got = trig(r, n)
        want, cnt = lights.rewrite(chk, sc.desc(), src, cur, dirty=dirty)
        scn = scene_records()
        print(what, "rewritten", r.light_stats().rewritten, "ms", round(r.light_stats().ms, 4), "differs from checker / scene in",
              optin.words(got, want), optin.words(lights.raw(got)[:, lights.POS], lights.raw(scn)[:, lights.POS]), "words")
        assert cnt == expect
        assert np.array_equal(lights.raw(got), lights.raw(want)), what
        assert np.array_equal(lights.raw(got)[:, lights.POS], lights.raw(scn)[:, lights.POS]), what
        assert np.array_equal(lights.raw(got)[:, KEEP], lights.raw(rec0)[:, KEEP]), what      # bytes outside 8..43: the uploaded ones
        other = ~np.isin(src["instance"], dirty)
        assert other.any() and np.array_equal(lights.raw(got)[other], lights.raw(cur)[other]), what      # untouched instances keep all 96 bytes
        assert not np.array_equal(lights.raw(got)[~other], lights.raw(cur)[~other]), what
        assert stats(r) == (n, expect, 0), what
        cur = got

    # instances: the mirrored instance of the 65-triangle mesh but not the plain one of the same mesh; a plain instance rides along
    ids = [em.mirrored, e64, e1, 5]
    home = inst["objectToWorld"]
    xf = np.stack([refit.compose(refit.scaling((-1.3, 0.6, 0.9), (1, 0.5, 0)), home[em.mirrored]),      # mirrored twice over and non-uniformly scaled
                   refit.compose(refit.rotation_y(0.7, (2, 0, -1)), home[e64]),
                   refit.compose(refit.scaling((-1.0, 1.0, 1.0)), home[e1]),                              # mirrored
                   refit.compose(refit.translation((0.1, 0.2, 0.3)), home[5])])
    sc.updateInstances(ids, xf)
    r.update_instances(ids, xf)
    check("update_instances", ids, 65 + 64 + 1)
    # vertices: the largest mesh
    m257 = em.prim_mesh(4)
    rows = lights.positions_moved(sc.desc(), m257, (0.03, -0.02, 0.01))
    sc.updateVertices(m257, 0, rows)
    r.update_vertices(m257, 0, rows)
    check("update_vertices", [e257], 257)
    assert r.deform_stats().vertexBytesCopied == rows.size * 32
    # skins on emissive meshes: the shared 65-triangle mesh (both instances follow, one of them mirrored) and the 63-triangle one
    meshes = [skin.SkinnedMesh(skc, sc.desc(), em.prim_mesh(3), 3), skin.SkinnedMesh(skc, sc.desc(), em.prim_mesh(1), 2, seed=1)]
    r.set_skins(*skin.skins_table(meshes))
    for kind, which in (("bend", [0, 1]), ("mirror", [1]), ("back", [0]), ("back", [])):
        mats = [meshes[k].matrices(kind, 2.0) for k in which]
        dirty = []
        for k, mm in zip(which, mats):
            sc.updateVertices(meshes[k].mesh, 0, meshes[k].posed(mm))      # (rt_update_skins' rows equal the skin checker's: tests/test_gpu_skin.py)
            dirty += [e65, em.mirrored] if k == 0 else [e63]
        r.update_skins(which, np.concatenate(mats) if mats else np.zeros((0, 12), np.float32))
        if which:
            check("update_skins " + kind, dirty, sum(2 * 65 if k == 0 else 63 for k in which))
        else:      # an update that refits nothing rewrites nothing
            assert stats(r) == (n, 0, 0) and np.array_equal(lights.raw(trig(r, n)), lights.raw(cur))
    assert r.deform_stats().vertexBytesCopied == 0
    # the device vertices are what the scene holds: the records above were computed from the same rows
    assert optin.words(r.vertices_readback(0, desc.numVertices), skin.vertices_of(sc.desc())) == 0
    # rt_update_lights still works and leaves the binding in place
    r.update_lights(lights.with_lights(sc.desc(), cur))
    assert stats(r) == (n, 0, n * 96)
    xf2 = refit.compose(refit.translation((0.0, 0.4, 0.0)), refit.instances_of(sc.desc())["objectToWorld"][e257])
    sc.updateInstances([e257], [xf2])
    r.update_instances([e257], [xf2])
    check("update_instances after update_lights", [e257], 257)
    r.destroy()


# ---- 2. frames --------------------------------------------------------------------------------------------------------------------------------------------
def light_move(f, home):
    return refit.compose(refit.translation([0.02 * (f + 1), -0.015 * (f + 1), 0.01 * f]), refit.compose(refit.rotation_y(0.12 * (f + 1), (0.0, 1.0, 0.0)), home[LIGHT]))


class MovedLight(deform.Sequence):
    """the sequence's scene and cameras with the ceiling light moved as an instance instead of deformed"""

    def __init__(self, chk, W, H):
        super().__init__(chk, W, H, move_box=False, which="light")

    def step(self, f):
        self.sc.updateInstances([LIGHT], [light_move(f, self.home)])
        eye, center, up, fov = self.pose
        a = 0.06 * f
        d = np.asarray(eye, np.float64) - center
        e = center + np.array([np.cos(a) * d[0] + np.sin(a) * d[2], d[1], -np.sin(a) * d[0] + np.cos(a) * d[2]])
        self.sc.setCamera(e.astype(np.float32), center, up, fov)
        self.sc.updateCamera(self.W, self.H)
        self.st.time = 1000 + f
        return None, None, self.sc.desc(), self.sc.getCamera()


_oracle = {}


def sequence(skc, W, H, way):
    return MovedLight(skc, W, H) if way == "instances" else deform.Sequence(skc, W, H, False, "light")


def oracle_frames(skc, W, H, way, stale_lights=False):
    """the oracle rendering the Scene-updated description of every frame; stale_lights: the same geometry with the light records left where they were uploaded"""
    if way != "instances" and not stale_lights:
        return deform.Sequence.oracle_frames(skc, W, H, False, "light", FRAMES)
    key = (W, H, way, stale_lights)
    if key not in _oracle:
        s = sequence(skc, W, H, way)
        rec0 = lights.records_of(s.sc.desc())
        o = Oracle(0)
        o.upload_scene(s.sc.desc())
        o.resize(W, H)
        out = []
        for f in range(FRAMES):
            _, _, desc, cam = s.step(f)
            o.upload_scene(lights.with_lights(desc, rec0) if stale_lights else desc)
            o.set_camera(cam)
            o.render_frame(s.st, f)
            out.append({b: o.readback(b).copy() for b in frame_buffers(f)})
        _oracle[key] = out
    return _oracle[key]


@pytest.mark.parametrize("W,H", SIZES)
@pytest.mark.parametrize("traversal", [abi.TRAVERSAL_THROUGHPUT, abi.TRAVERSAL_LATENCY])
@pytest.mark.parametrize("overlap", [0, 2])
@pytest.mark.parametrize("way", ["skins", "vertices", "instances"])
def test_frames_equal_the_oracle_without_update_lights(skc, way, overlap, traversal, W, H):
    want = oracle_frames(skc, W, H, way)
    s = sequence(skc, W, H, way)
    r = deform.renderer(s.sc.desc(), W, H, overlap, traversal)
    r.set_light_sources(s.sc.lightSources())
    if way == "skins":
        r.set_skins(*skin.skins_table([s.sk]))      # the emissive mesh: refused without the binding
    bad = {}
    n = s.sc.desc().lightInfo.trigLightSize
    for f in range(FRAMES):
        mats, rows, desc, cam = s.step(f)
        if way == "skins":
            r.update_skins([0], mats)
        elif way == "vertices":
            r.update_vertices(s.mesh, 0, rows)
        else:
            r.update_instances([LIGHT], [light_move(f, s.home)])
        assert np.array_equal(lights.raw(trig(r, n)), lights.raw(lights.records_of(desc))), f
        r.set_camera(cam)
        r.run(s.st, f)
        d = deform.frame_diff(r, want, f)
        if d:
            bad[f] = d
    assert stats(r) == (n, n, 0)
    r.destroy()
    assert bad == {}


@pytest.mark.parametrize("way", ["skins", "instances"])
def test_the_sequence_sees_where_the_lights_are(skc, way):
    """control: the oracle's direct result with the moved lights differs from the one with the light records left in place"""
    W, H = SIZES[0]
    want, stale = oracle_frames(skc, W, H, way), oracle_frames(skc, W, H, way, stale_lights=True)
    f = FRAMES - 1
    b = abi.BUF_DIRECT_RESULT0 + (f & 1)
    assert optin.words(want[f][abi.BUF_GBUFFER0 + (f & 1)], stale[f][abi.BUF_GBUFFER0 + (f & 1)]) == 0      # the same geometry
    assert optin.words(want[f][b], stale[f][b]) > 0


class BoundCase(objmotion.Case):
    """objmotion.Case whose updates leave the light records to the binding: no rt_update_lights"""

    def update(self, ids, xf):
        cur = refit.instances_of(self.desc)["objectToWorld"]
        for i in ids:
            self.pending.setdefault(int(i), cur[int(i)].copy())
        self.sc.updateInstances(np.asarray(ids, np.uint32), np.asarray(xf, np.float32))
        self.desc = self.sc.desc()
        self.r.update_instances(ids, xf)
        self.o.upload_scene(self.desc)


def test_a_moving_emitter_with_object_motion_vectors():
    W, H = SIZES[0]
    case = BoundCase("cornell", W, H, overlap=2, movers=[LIGHT, SHORT])
    case.r.set_light_sources(case.sc.lightSources())
    n = case.desc.lightInfo.trigLightSize
    for f, k in enumerate((None,) + objmotion.SEQUENCE[:3]):
        case.frame(f, k)
        assert case.diff(f) == {}, (f, k)
        assert np.array_equal(lights.raw(trig(case.r, n)), lights.raw(lights.records_of(case.desc))), f
        if k is not None:
            assert [g[0] for g in case.groups] == [SHORT, LIGHT] and stats(case.r) == (n, n, 0)
    case.destroy()


# ---- 3. refusals change nothing ---------------------------------------------------------------------------------------------------------------------------
def test_refused_bindings_change_nothing_and_the_next_frame_matches(skc):
    from restir_amd.renderer import Renderer, RtError, hip_lib
    W, H = SIZES[0]
    want = oracle_frames(skc, W, H, "instances")
    s = sequence(skc, W, H, "instances")
    desc0 = s.sc.desc()
    home_records = lights.records_of(desc0)      # (a copy: a description reads the scene's own arrays, which the updates below rewrite)
    src = s.sc.lightSources()
    n = src.size
    assert n >= 2
    L = hip_lib()
    r0 = Renderer().setup(0)
    assert L.rt_set_light_sources(r0._h, n, src.ctypes.data) == abi.ERR_NO_SCENE
    assert L.rt_lights_readback(r0._h, abi.LIGHTS_TRIG, None, 0) == abi.ERR_NO_SCENE
    assert L.rt_upload_scene(r0._h, C.byref(desc0)) == 0
    assert L.rt_set_light_sources(r0._h, n, src.ctypes.data) == 0      # valid after rt_upload_scene, before rt_build_accel
    st = abi.LightStats()
    assert L.rt_get_light_stats(r0._h, C.byref(st)) == 0 and st.bound == n
    r0.destroy()

    r = deform.renderer(desc0, W, H, 2)
    r.set_light_sources(src)
    for f in range(2):
        _, _, desc, cam = s.step(f)
        r.update_instances([LIGHT], [light_move(f, s.home)])
        r.set_camera(cam)
        r.run(s.st, f)
    r.sync()
    state = lambda: [trig(r, n).tobytes(), r.lights_readback(abi.LIGHTS_PUNC, desc0.lightInfo.puncLightSize).tobytes(), bytes(r.light_stats())]      # noqa: E731
    before = state()

    def variant(k, field, v):
        t = src.copy()
        t[field][k] = v
        return t
    other_material = next(i for i in range(desc0.numInstances) if refit.prim_meshes_of(desc0)["materialIndex"][refit.instances_of(desc0)["primMesh"][i]]
                          != refit.prim_meshes_of(desc0)["materialIndex"][refit.instances_of(desc0)["primMesh"][LIGHT]])
    swapped = src.copy()
    swapped[[0, 1]] = swapped[[1, 0]]      # two records of different triangles of one instance: every index check passes, the positions do not
    assert swapped[0]["instance"] == swapped[1]["instance"] and swapped[0]["triangle"] != swapped[1]["triangle"]
    refused = [src[:-1], np.concatenate([src, src[:1]]),                                   # a wrong count
               variant(0, "instance", desc0.numInstances), variant(1, "triangle", 1 << 20),
               variant(n - 1, "triangle", int(refit.prim_meshes_of(desc0)["indexCount"][refit.instances_of(desc0)["primMesh"][LIGHT]]) // 3),
               variant(0, "instance", other_material),                               # a matIndex mismatch
               swapped]
    for k, t in enumerate(refused):
        with pytest.raises(RtError) as e:
            r.set_light_sources(t)
        assert "(-1)" in str(e.value), k
        assert state() == before, k
    with pytest.raises(RtError, match="record 0 "):      # the message names the first record that differs
        r.set_light_sources(swapped)
    assert L.rt_set_light_sources(r._h, n, None) == abi.ERR_INVALID_ARG
    for which, size in ((abi.LIGHTS_TRIG, n * 96 - 1), (2, 0)):
        assert L.rt_lights_readback(r._h, which, np.zeros(n * 96, np.uint8).ctypes.data, size) == abi.ERR_INVALID_ARG
    assert state() == before
    # stale records are refused too: a host that let them go stale calls rt_update_lights first
    r2 = deform.renderer(lights.with_lights(desc, home_records), W, H, 2)      # moved geometry, the lights left in place
    with pytest.raises(RtError):
        r2.set_light_sources(src)
    r2.update_lights(desc)
    r2.set_light_sources(src)
    r2.destroy()
    # the next frame of the sequence still matches the oracle
    _, _, desc, cam = s.step(2)
    r.update_instances([LIGHT], [light_move(2, s.home)])
    r.set_camera(cam)
    r.run(s.st, 2)
    assert deform.frame_diff(r, want, 2) == {}
    r.destroy()


# ---- 4. life cycle ----------------------------------------------------------------------------------------------------------------------------------------
def test_the_binding_survives_both_builds_and_upload_scene_drops_it(skc):
    from restir_amd.renderer import RtError
    W, H = SIZES[0]
    s = sequence(skc, W, H, "skins")
    desc0 = s.sc.desc()
    home_records = lights.records_of(desc0)      # (a copy: a description reads the scene's own arrays, which the updates below rewrite)
    src = s.sc.lightSources()
    n = src.size
    r = deform.renderer(desc0, W, H, 2)
    sk_tab, inf_tab = skin.skins_table([s.sk])
    with pytest.raises(RtError, match="the prim mesh is emissive"):      # without a binding: today's refusal, today's message
        r.set_skins(sk_tab, inf_tab)
    r.set_light_sources(src)
    r.update(W + 2, H)      # rt_resize does not touch the binding
    for k, build in enumerate((lambda: refit.hip_build_accel(r), lambda: r.rebuild_accel())):
        assert build() in (0, None)
        xf = light_move(k, s.home)
        s.sc.updateInstances([LIGHT], [xf])
        r.update_instances([LIGHT], [xf])
        assert stats(r) == (n, n, 0)
        assert np.array_equal(lights.raw(trig(r, n)), lights.raw(lights.records_of(s.sc.desc()))), k
    # an update whose pad grows takes the full-refit path and still rewrites the lights (only those of the moved instance)
    far = refit.compose(refit.translation((300.0, 50.0, -200.0)), s.home[SHORT])
    s.sc.updateInstances([SHORT, LIGHT], [far, s.home[LIGHT]])
    r.update_instances([SHORT, LIGHT], [far, s.home[LIGHT]])
    assert r.refit_stats().fullRefit == 1 and stats(r) == (n, n, 0)
    assert np.array_equal(lights.raw(trig(r, n)), lights.raw(lights.records_of(s.sc.desc())))
    assert np.array_equal(lights.raw(trig(r, n)), lights.raw(home_records))      # ... back home
    s.sc.updateInstances([SHORT], [far])
    r.update_instances([SHORT], [far])      # an update that moves no emitter rewrites no light
    assert stats(r) == (n, 0, 0)
    # removing the binding under an emissive skin is refused; without the skin it goes
    r.set_skins(sk_tab, inf_tab)
    with pytest.raises(RtError, match="skin on an emissive"):
        r.set_light_sources(np.zeros(0, abi.LIGHT_SOURCE_DT))
    assert r.light_stats().bound == n
    mats, rows, _, _ = s.step(0)
    r.update_skins([0], mats)
    assert stats(r) == (n, n, 0) and np.array_equal(lights.raw(trig(r, n)), lights.raw(lights.records_of(s.sc.desc())))
    # a pose with a non-finite position is refused before the commit: no light record is written
    held = trig(r, n).tobytes()
    with pytest.raises(RtError):
        r.update_skins([0], np.stack([skin.affine(np.eye(3) * 3e38, (3e38, 3e38, 3e38))] * 2))
    assert trig(r, n).tobytes() == held and stats(r) == (n, n, 0)
    r.set_skins(np.zeros(0, abi.SKIN_DT), np.zeros(0, abi.SKIN_INFLUENCE_DT))
    r.set_light_sources(np.zeros(0, abi.LIGHT_SOURCE_DT))
    assert stats(r) == (0, 0, 0)
    r.update_instances([LIGHT], [light_move(3, s.home)])      # unbound: the emitter's records stay where they are
    assert trig(r, n).tobytes() == held and stats(r) == (0, 0, 0)
    # rt_upload_scene drops the binding
    r.set_light_sources(np.zeros(0, abi.LIGHT_SOURCE_DT))
    r.load_scene(desc0)
    r.set_light_sources(src)
    r.load_scene(desc0)
    assert r.light_stats().bound == 0
    with pytest.raises(RtError, match="the prim mesh is emissive"):
        r.set_skins(sk_tab, inf_tab)
    r.destroy()
