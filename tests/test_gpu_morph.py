"""Morph targets on the GPU (rt_set_morph_targets / rt_update_morphs): the device vertex array equals the CPU restatement (tests/morph_checker.cpp)
word for word, alone and composed with skins (skin.pose of the morphed rows); the refitted tree equals the refit checker; frames equal the oracle rendering the
checker's rows bit for bit; a morphed emitter's light records follow; refused calls change nothing; the sets' life cycle.  No tolerance anywhere."""
import ctypes as C
import numpy as np
import pytest

from helpers import abi, frame_buffers
from oracle.binding import Oracle
import lights
import morph
import optin
import refit
import skin
import test_gpu_skin as deform      # renderer(), device_tree(), the Cornell sequence

pytestmark = pytest.mark.gpu

SIZES = ((64, 48), (67, 45))
FRAMES = 4
TALL, SHORT, LIGHT = 4, 3, 5      # Cornell's boxes and ceiling light (instances)
TRIANGLES = (1, 21, 21, 22, 85, 86)      # vertices: 3, 63, 64 (with the unreferenced extra vertex), 66, 255, 258
TARGETS = (1, 2, 9, 9, 2, 1)
PLANES = (0, 1, 2, 3, 3, 1)
W9 = [0.0, 1.5, -0.0, -0.7, 0.0, 0.25, 2.0, 0.0, -1.2]      # zeros, a -0, negatives, values > 1
WEIGHTS = {1: [0.8], 2: [-0.5, 1.25], 9: W9}


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    return refit.build(tmp_path_factory.mktemp("refit"))


@pytest.fixture(scope="module")
def skc(tmp_path_factory):
    return skin.build(tmp_path_factory.mktemp("skin"))


@pytest.fixture(scope="module")
def mpc(tmp_path_factory):
    return morph.build(tmp_path_factory.mktemp("morph"))


def patches(skc):
    """six meshes side by side, mesh 2 with one vertex no index references, and a mirrored second instance of mesh 1"""
    sc = skin.Patches(skc, TRIANGLES, mirror_instance_of=1)
    end = int(sc.prim[2, 0] + sc.prim[2, 1])
    row = sc.vertices[end - 1:end].copy()
    row["position"] = (0.4, 0.5, -0.3)
    sc.vertices = np.concatenate([sc.vertices[:end], row, sc.vertices[end:]])
    sc.prim[2, 1] += 1
    sc.prim[3:, 0] += 1
    d = sc.desc()
    d.numVertices, d.vertices = sc.vertices.size, sc.vertices.ctypes.data
    assert [int(n) for n in sc.prim[:, 1]] == [3, 63, 64, 66, 255, 258]
    return sc


def morphed_meshes(mpc, desc):
    return [morph.MorphedMesh(mpc, desc, m, TARGETS[m], PLANES[m], seed=m) for m in range(len(TRIANGLES))]


def concat(ws):
    return np.concatenate([np.asarray(w, np.float32) for w in ws]) if ws else np.zeros(0, np.float32)


def instances_of(desc, meshes):
    return np.sort(np.concatenate([skin.instances_of_mesh(desc, m) for m in meshes])).astype(np.uint32)


# ---- 1. device rows against the checker ---------------------------------------------------------------------------------------------------------------------
def test_morphed_vertices_equal_the_checker_word_for_word(skc, mpc):
    sc = patches(skc)
    desc = sc.desc()
    r = deform.renderer(desc)
    mm = morphed_meshes(mpc, desc)
    assert sorted(set(PLANES)) == [0, 1, 2, 3] and sorted(set(TARGETS)) == [1, 2, 9]
    r.set_morph_targets(*morph.sets_table(mm))
    want = skin.vertices_of(desc)
    assert optin.words(r.vertices_readback(0, desc.numVertices), want) == 0
    rounds = [([5, 2, 0], None), ([4, 3, 1], None), ([3], [[0.0] * 9]), ([2, 5], [[-0.0] * 9, [-2.5]]), ([], None)]
    for ids, ws in rounds:
        ws = [WEIGHTS[mm[k].target_count] for k in ids] if ws is None else ws
        before = r.vertices_readback(0, desc.numVertices)
        for k, w in zip(ids, ws):
            want[mm[k].first:mm[k].first + mm[k].count] = mm[k].morphed(w)
        r.update_morphs(ids, concat(ws))
        got = r.vertices_readback(0, desc.numVertices)
        assert optin.words(got, want) == 0, ids
        for k in set(range(len(mm))) - set(ids):      # the rows of unlisted meshes keep all 32 bytes
            assert got[mm[k].first:mm[k].first + mm[k].count].tobytes() == before[mm[k].first:mm[k].first + mm[k].count].tobytes(), (ids, k)
        st, ds = r.morph_stats(), r.deform_stats()
        n_inst = len(instances_of(desc, ids)) if ids else 0
        assert (st.sets, st.vertices, st.targetsApplied, st.instances) == (len(ids), sum(mm[k].count for k in ids), sum(mm[k].active(w) for k, w in zip(ids, ws)), n_inst), ids
        assert (ds.meshes, ds.vertices, ds.instances, ds.vertexBytesCopied) == (len(ids), st.vertices, n_inst, 0)
    first, count = mm[3].first, mm[3].count      # all weights zero: the rest rows, the packed directions included
    assert want[first:first + count].tobytes() == skin.vertices_of(desc)[first:first + count].tobytes()
    assert (want["normal"][mm[4].first + 1:mm[4].first + mm[4].count] != mm[4].rest["normal"][1:]).any() and want["normal"][mm[4].first] == 0xffffffff
    r.destroy()


# ---- 2. morph and skin together -----------------------------------------------------------------------------------------------------------------------------
def test_morph_then_skin_equals_the_two_checkers_and_the_tree_the_refit_checker(lib, skc, mpc):
    sc = patches(skc)
    desc = sc.desc()
    r, plain = deform.renderer(desc), deform.renderer(desc)
    mm = morphed_meshes(mpc, desc)
    skinned = (1, 3, 5)      # half of the morphed meshes; skin k poses mesh skinned[k]
    sk = [skin.SkinnedMesh(skc, desc, m, j, seed=m) for m, j in zip(skinned, (5, 1, 5))]
    skin_of = {m: k for k, m in enumerate(skinned)}
    for x in (r, plain):
        x.set_skins(*skin.skins_table(sk))
    r.set_morph_targets(*morph.sets_table(mm))
    r.update_instances([], np.zeros((0, 12), np.float32))      # tells the build's pad; changes no word
    t = deform.device_tree(lib, r, desc)
    inst = refit.instances_of(desc)
    want = skin.vertices_of(desc)
    weights = {m: [0.0] * TARGETS[m] for m in range(len(mm))}
    mats = {}

    def expect(meshes):
        for m in meshes:
            rows = mm[m].morphed(weights[m])
            if m in skin_of:
                rows, bad = skin.pose(skc, rows, sk[skin_of[m]].influences, mats[m])
                assert bad == 0
            want[mm[m].first:mm[m].first + mm[m].count] = rows
        ids = instances_of(desc, meshes)
        t.desc = skin.with_vertices(desc, want.copy())
        assert t.refit(ids, inst["objectToWorld"][ids]) == 0
        assert optin.words(r.vertices_readback(0, desc.numVertices), want) == 0, meshes
        assert deform.same_tree(r, t, desc) == {"nodes": 0, "records": 0, "instances": 0}, meshes
        assert t.check() == (0, "")
        st = r.refit_stats()
        assert [st.instances, st.leafRecords, st.nodes, st.levels, st.fullRefit] == [len(ids)] + [int(x) for x in t.stats], meshes

    def update_skins(meshes, kind):
        for m in meshes:
            mats[m] = sk[skin_of[m]].matrices(kind, 2.0)
        r.update_skins([skin_of[m] for m in meshes], np.concatenate([mats[m] for m in meshes]))
        expect(meshes)

    def update_morphs(meshes, ws=None):
        for m in meshes:
            weights[m] = WEIGHTS[TARGETS[m]] if ws is None else ws[m]
        r.update_morphs(meshes, concat([weights[m] for m in meshes]))
        expect(meshes)

    from restir_amd.renderer import RtError
    with pytest.raises(RtError, match="pose the skin first"):
        r.update_morphs([1], WEIGHTS[TARGETS[1]])
    # all stored weights zero: rt_update_skins gives the words it gives with no morph sets at all
    update_skins([5, 1, 3], "bend")
    plain.update_skins([2, 0, 1], np.concatenate([mats[5], mats[1], mats[3]]))
    assert optin.words(r.vertices_readback(0, desc.numVertices), plain.vertices_readback(0, desc.numVertices)) == 0
    assert bytes(r.deform_stats())[:16] == bytes(plain.deform_stats())[:16]
    update_morphs([5, 4, 1, 0])            # skinned and morph-only sets in one call, with the stored matrices
    update_skins([3, 1], "twist")          # mesh 1: the stored weights first, then the new matrices; mesh 3: weights still zero
    update_morphs([3, 2])                  # the reverse order on mesh 3
    update_skins([5], "mirror")
    update_morphs([1, 5], {1: [0.0, -0.0], 5: [0.3]})      # a morphed skin with no active target poses from the rest pose
    assert r.morph_stats().targetsApplied == 1 and r.deform_stats().vertexBytesCopied == 0
    assert want["normal"][mm[1].first] == 0xffffffff
    r.destroy(); plain.destroy()


# ---- 3. frames against the oracle ----------------------------------------------------------------------------------------------------------------------------
class MorphSequence(deform.Sequence):
    """the Cornell sequence of tests/test_gpu_skin.py with the tall box morphed instead: two targets, a bulge (with normal deltas) and a shear, weights animated over
    the frames; skinned: the morphed rows are posed by the sequence's two-joint skin as well; still: the rest pose (the control)"""

    def __init__(self, skc, mpc, W, H, skinned=False, still=False, which="tall"):
        super().__init__(skc, W, H, move_box=which == "tall", which=which)
        self.skc, self.skinned, self.still = skc, skinned, still
        p = self.sk.rest["position"].astype(np.float64)
        lo, hi = p.min(axis=0), p.max(axis=0)
        h = (p[:, 1] - lo[1]) / max(hi[1] - lo[1], 1e-9)
        radial = (p - self.sk.centre) * [1, 0, 1]
        if which == "tall":
            bulge, shear = 0.6 * radial * h[:, None], np.stack([0.25 * h * (hi[1] - lo[1]), 0 * h, -0.1 * h * (hi[1] - lo[1])], axis=1)
        else:      # the ceiling light is flat in y: it sags and slides
            bulge = np.stack([0 * h, -0.3 * np.abs(radial).sum(axis=1), 0 * h], axis=1)
            shear = np.stack([0.1 + 0 * h, 0 * h, 0.3 * radial[:, 0]], axis=1)
        d = np.zeros((2, 2, self.sk.count, 3), np.float32)      # target, plane (position, normal), vertex
        d[0, 0], d[1, 0] = bulge, shear
        d[0, 1] = 0.5 * radial / np.maximum(np.linalg.norm(radial, axis=1, keepdims=True), 1e-9)
        deltas = np.zeros(d.size // 3, morph.DELTA_DT)
        deltas["d"] = d.reshape(-1, 3)
        self.mm = morph.MorphedMesh(mpc, self.sc.desc(), self.mesh, 2, abi.MORPH_NORMALS, deltas=deltas)

    def weights(self, f):
        return np.array([0.15 * f, 0.5 * np.sin(0.9 * (f + 1))], np.float32)      # frame 0: the bulge is inactive

    def step(self, f):
        mats = self.matrices(f)
        rows = self.mm.rest.copy() if self.still else self.mm.morphed(self.weights(f))
        if self.skinned and not self.still:
            rows, bad = skin.pose(self.skc, rows, self.sk.influences, mats)
            assert bad == 0
        self.verts[self.sk.first:self.sk.first + self.sk.count] = rows
        if self.move_box:
            self.sc.updateInstances([SHORT], [deform.box_move(f, self.home)])
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


_oracle = {}


def oracle_frames(skc, mpc, W, H, skinned=False, still=False, which="tall"):
    """the oracle rendering the description whose vertices are the checkers' rows, once per variant"""
    key = (W, H, skinned, still, which)
    if key not in _oracle:
        s = MorphSequence(skc, mpc, W, H, skinned, still, which)
        o = Oracle(0)
        o.upload_scene(s.sc.desc())
        o.resize(W, H)
        out = []
        for f in range(FRAMES):
            _, _, desc, cam = s.step(f)
            o.upload_scene(desc)
            o.set_camera(cam)
            o.render_frame(s.st, f)
            out.append({b: o.readback(b).copy() for b in frame_buffers(f)})
        _oracle[key] = out
    return _oracle[key]


def run_frames(skc, mpc, W, H, overlap, traversal, skinned=False, which="tall"):
    want = oracle_frames(skc, mpc, W, H, skinned, False, which)
    s = MorphSequence(skc, mpc, W, H, skinned, False, which)
    r = deform.renderer(s.sc.desc(), W, H, overlap, traversal)
    if which == "light":
        r.set_light_sources(s.sc.lightSources())
    if skinned:
        r.set_skins(*skin.skins_table([s.sk]))
    r.set_morph_targets(*morph.sets_table([s.mm]))
    bad = {}
    n = s.sc.desc().lightInfo.trigLightSize
    for f in range(FRAMES):
        mats, rows, desc, cam = s.step(f)
        if skinned and f % 2 == 0:      # both orders over the sequence: the skin first on even frames, the morph first on odd ones
            r.update_skins([0], mats)
            r.update_morphs([0], s.weights(f))
        else:
            r.update_morphs([0], s.weights(f))
            if skinned:
                r.update_skins([0], mats)
        if which == "light":
            assert np.array_equal(lights.raw(r.lights_readback(abi.LIGHTS_TRIG, n)), lights.raw(lights.records_of(desc))), f
        if s.move_box:
            r.update_instances([SHORT], [deform.box_move(f, s.home)])
        r.set_camera(cam)
        r.run(s.st, f)
        d = deform.frame_diff(r, want, f)
        if d:
            bad[f] = d
    return r, s, bad


@pytest.mark.parametrize("W,H", SIZES)
@pytest.mark.parametrize("traversal", [abi.TRAVERSAL_THROUGHPUT, abi.TRAVERSAL_LATENCY])
@pytest.mark.parametrize("overlap", [0, 2])
def test_frames_equal_the_oracle_rendering_the_morphed_scene(skc, mpc, W, H, overlap, traversal):
    r, s, bad = run_frames(skc, mpc, W, H, overlap, traversal)
    r.destroy()
    assert bad == {}
    want, rest = oracle_frames(skc, mpc, W, H), oracle_frames(skc, mpc, W, H, still=True)      # control: the rest pose gives a different direct image
    assert optin.words(want[3][abi.BUF_DIRECT_RESULT0 + 1], rest[3][abi.BUF_DIRECT_RESULT0 + 1]) > 0


def test_frames_of_a_morphed_and_skinned_box_equal_the_oracle(skc, mpc):
    W, H = SIZES[1]
    r, s, bad = run_frames(skc, mpc, W, H, 2, None, skinned=True)
    r.destroy()
    assert bad == {}
    assert optin.words(oracle_frames(skc, mpc, W, H, skinned=True)[3][abi.BUF_GBUFFER0 + 1], oracle_frames(skc, mpc, W, H)[3][abi.BUF_GBUFFER0 + 1]) > 0


# ---- 4. a morphed emitter -------------------------------------------------------------------------------------------------------------------------------------
def test_a_morphed_emitter_rewrites_its_light_records(tmp_path, skc, mpc):
    from restir_amd.renderer import RtError
    W, H = SIZES[0]
    lc = lights.build(tmp_path)
    r, s, bad = run_frames(skc, mpc, W, H, 2, None, which="light")      # (asserts records == the Scene's after every update)
    assert bad == {}
    n = s.sc.desc().lightInfo.trigLightSize
    got = r.lights_readback(abi.LIGHTS_TRIG, n)
    home = MorphSequence(skc, mpc, W, H, which="light")
    want, cnt = lights.rewrite(lc, skin.with_vertices(s.sc.desc(), s.verts), s.sc.lightSources(), lights.records_of(home.sc.desc()))
    assert cnt == n and np.array_equal(lights.raw(got), lights.raw(want))
    assert not np.array_equal(lights.raw(got), lights.raw(lights.records_of(home.sc.desc())))
    ls = r.light_stats()
    assert (ls.bound, ls.lightBytesCopied) == (n, 0) and ls.rewritten > 0
    with pytest.raises(RtError):      # removing the binding under a morphed emitter
        r.set_light_sources(np.zeros(0, abi.LIGHT_SOURCE_DT))
    r.destroy()
    # without the binding the set is refused
    r = deform.renderer(home.sc.desc(), W, H, 2)
    with pytest.raises(RtError, match="emissive"):
        r.set_morph_targets(*morph.sets_table([home.mm]))
    assert r.morph_stats().sets == 0
    r.destroy()


# ---- 5. refusals change nothing ---------------------------------------------------------------------------------------------------------------------------
def all_state(r, desc, n_lights):
    return deform.all_state(r, desc) + [bytes(r.morph_stats()), r.lights_readback(abi.LIGHTS_TRIG, n_lights).tobytes(), bytes(r.light_stats())]


def test_refused_calls_change_nothing_and_the_next_frame_matches(skc, mpc):
    from restir_amd.renderer import Renderer, RtError, hip_lib
    W, H = SIZES[0]
    want = oracle_frames(skc, mpc, W, H)
    s = MorphSequence(skc, mpc, W, H)
    desc0 = s.sc.desc()
    n_lights = desc0.lightInfo.trigLightSize
    L = hip_lib()
    sets, deltas = morph.sets_table([s.mm])
    one, w2 = np.zeros(1, np.uint32), np.zeros(2, np.float32)
    r0 = Renderer().setup(0)
    assert L.rt_set_morph_targets(r0._h, 1, sets.ctypes.data, deltas.size, deltas.ctypes.data) == abi.ERR_NO_SCENE
    assert L.rt_upload_scene(r0._h, C.byref(desc0)) == 0
    assert L.rt_set_morph_targets(r0._h, 1, sets.ctypes.data, deltas.size, deltas.ctypes.data) == 0      # valid after rt_upload_scene
    assert L.rt_update_morphs(r0._h, 1, one.ctypes.data, w2.ctypes.data) == abi.ERR_NO_ACCEL
    r0.destroy()
    r = deform.renderer(desc0, W, H, 2)
    with pytest.raises(RtError):      # before rt_set_morph_targets
        r.update_morphs([0], w2)
    r.set_morph_targets(sets, deltas)
    for f in range(2):
        _, _, desc, cam = s.step(f)
        r.update_morphs([0], s.weights(f))
        r.update_instances([SHORT], [deform.box_move(f, s.home)])
        r.set_camera(cam)
        r.run(s.st, f)
    r.sync()
    state = all_state(r, desc0, n_lights)
    far = s.mm.deltas.copy()
    far["d"][0] = [10, 0, 0]
    refused = [
        lambda: r.update_morphs([1], w2), lambda: r.update_morphs([0, 0], np.zeros(4, np.float32)),
        lambda: r.update_morphs([0], [np.nan, 0]), lambda: r.update_morphs([0], [0, np.inf]),
        lambda: r.update_vertices(s.mesh, 0, s.mm.rest),                              # a mesh that has a morph set
        lambda: r.set_skins(*skin.skins_table([s.sk])), lambda: r.set_skins(np.zeros(0, abi.SKIN_DT), np.zeros(0, abi.SKIN_INFLUENCE_DT)),      # skins first
    ]
    for k, call in enumerate(refused):
        with pytest.raises(RtError):
            call()
        assert all_state(r, desc0, n_lights) == state, k

    def table(**kw):
        t = sets.copy()
        for key, v in kw.items():
            t[key] = v
        return t
    nan_d = deltas.copy(); nan_d["d"][5, 1] = np.nan
    light = int(refit.instances_of(desc0)["primMesh"][LIGHT])
    for k, (tab, dl) in enumerate([(table(primMesh=desc0.numPrimMeshes), deltas), (np.concatenate([sets, sets]), deltas), (table(targetCount=0), deltas),
                                   (table(targetCount=4097), deltas), (table(planes=4), deltas), (table(planes=3), deltas), (table(firstDelta=1), deltas),
                                   (sets, deltas[:-1]), (sets, nan_d), (table(primMesh=light, planes=0), np.zeros(64, morph.DELTA_DT))]):
        with pytest.raises(RtError):
            r.set_morph_targets(tab, dl)
        assert all_state(r, desc0, n_lights) == state, ("set_morph_targets", k)
    # a pose with a non-finite position: one weight of 3e38 on a delta of 10 (the sets are replaced: stored weights start at zero, no vertex changes)
    r.set_morph_targets(sets, far)
    assert all_state(r, desc0, n_lights) == state
    with pytest.raises(RtError, match="non-finite position"):
        r.update_morphs([0], [3e38, 0])
    assert all_state(r, desc0, n_lights) == state
    r.set_morph_targets(np.zeros(0, morph.SET_DT), np.zeros(0, morph.DELTA_DT))
    # the sets were removed while the mesh was morphed: a new set's rest pose would be the morphed rows, so the scene starts again for the next frame
    r.destroy()
    s = MorphSequence(skc, mpc, W, H)
    r = deform.renderer(s.sc.desc(), W, H, 2)
    r.set_morph_targets(sets, deltas)
    for f in range(3):
        _, _, desc, cam = s.step(f)
        r.update_morphs([0], s.weights(f))
        if f == 1:      # refusals between the frames of a sequence
            with pytest.raises(RtError):
                r.update_morphs([0], [np.nan, 0])
            with pytest.raises(RtError):
                r.update_morphs([0, 0], np.zeros(4, np.float32))
        r.update_instances([SHORT], [deform.box_move(f, s.home)])
        r.set_camera(cam)
        r.run(s.st, f)
        assert deform.frame_diff(r, want, f) == {}, f
    r.destroy()


# ---- 6. life cycle -----------------------------------------------------------------------------------------------------------------------------------------
def test_the_sets_survive_both_builds_and_upload_scene_drops_them(skc, mpc):
    from restir_amd.renderer import RtError
    sc = patches(skc)
    desc = sc.desc()
    r = deform.renderer(desc)
    mm = morphed_meshes(mpc, desc)
    r.set_morph_targets(*morph.sets_table(mm))
    want = skin.vertices_of(desc)
    r.update_morphs([4], WEIGHTS[2])
    want[mm[4].first:mm[4].first + mm[4].count] = mm[4].morphed(WEIGHTS[2])
    r.rebuild_accel()
    assert refit.hip_build_accel(r) == 0      # the host builder reads the context's copy, refreshed from the device first
    assert optin.words(r.vertices_readback(0, desc.numVertices), want) == 0
    r.update_morphs([2], W9)                  # the sets, their rest poses and the deltas survived both builds
    want[mm[2].first:mm[2].first + mm[2].count] = mm[2].morphed(W9)
    assert optin.words(r.vertices_readback(0, desc.numVertices), want) == 0
    r.update(32, 24)                          # rt_resize keeps them
    r.update_morphs([4], [0.0, 0.0])
    want[mm[4].first:mm[4].first + mm[4].count] = mm[4].rest
    assert optin.words(r.vertices_readback(0, desc.numVertices), want) == 0
    sk = skin.SkinnedMesh(skc, desc, 0, 2)
    with pytest.raises(RtError):              # skins first
        r.set_skins(*skin.skins_table([sk]))
    rows = mm[0].rest.copy()
    rows["position"] += np.float32(0.01)
    with pytest.raises(RtError):
        r.update_vertices(0, 0, rows)
    r.set_morph_targets(np.zeros(0, morph.SET_DT), np.zeros(0, morph.DELTA_DT))      # removal allows rt_update_vertices again
    r.update_vertices(0, 0, rows)
    want[mm[0].first:mm[0].first + mm[0].count] = rows
    assert optin.words(r.vertices_readback(0, desc.numVertices), want) == 0
    with pytest.raises(RtError):
        r.update_morphs([0], [0.5])
    r.set_morph_targets(*morph.sets_table(mm[1:2]))
    r.load_scene(desc)                        # rt_upload_scene drops the sets
    with pytest.raises(RtError):
        r.update_morphs([0], [0.5, 0.5])
    r.destroy()
