"""Seeded primary rays (DESIGN.md §3 "Seeded primary rays"): k_direct_stage tests the leaf record its pixel hit last frame before the traversal loop, from a
context-owned plane of record indices.  The plane may only change how many steps a ray takes, never a bit of any buffer: every test compares words with the oracle
(or with a fresh context), with warm, stale, emptied and foreign planes, and the counters show that the seed is used and only removes work.

Shapes: 70 x 50 — neither a multiple of the 8 x 8 tile, 9 x 7 tiles = more than one workgroup, an odd 35 x 25 half resolution — of the exterior street scene at a
few thousand triangles (tests/refit.py street(): instanced trees with alpha-tested leaf cards, mirrored props, long thin triangles that the builder splits into
duplicate references).  Images this small would take the latency build under RT_TRAVERSAL_AUTO, so the tests name the build they are about."""
import numpy as np
import pytest

from helpers import abi, host, frame_buffers
from oracle.binding import Oracle
import optin
import refit

pytestmark = pytest.mark.gpu

W, H = 70, 50
STEP = np.array([0.05, 0.012, -0.04], dtype=np.float32)
# test 1: six frames at rest, three in motion (the plane then holds the previous view's records), two at rest again
OFFSETS = [0] * 6 + [1, 2, 3] + [3, 3]
COUNTER_FIELDS = ("closestHitRays", "anyHitRays", "nodesVisited", "trisTested", "hitsShaded", "risCandidates", "laneRounds", "laneLiveRounds")


def renderer(desc, w=W, h=H, overlap=None, traversal=abi.TRAVERSAL_THROUGHPUT):
    from restir_amd.renderer import Renderer
    r = Renderer().setup(0)
    if overlap is not None:
        r.set_overlap(overlap)
    r.load_scene(desc)
    r.update(w, h)
    if traversal is not None:
        r.set_traversal(traversal)
    return r


def state(sc, w=W, h=H):
    st = host.default_state(w, h, sc, None)
    st.environmentProb = 0.0
    return st


def camera(sc, pose, k, w=W, h=H):
    """the scene's camera moved k steps off its pose, history matrices advanced as SampleExample::updateFrame does; returns a copy"""
    eye, center, up, fov = pose
    sc.setCamera(eye + np.float32(k) * STEP, center, up, fov)
    sc.updateCamera(w, h)
    cam = sc.getCamera()
    return type(cam).from_buffer_copy(cam)


def bad_buffers(r, want):
    bad = {abi.BUFFER_NAMES[b]: optin.words(r.readback(b), w) for b, w in want.items()}
    return {k: v for k, v in bad.items() if v}


# ---- 1. bit-exact with a warm plane, a stale one and a warm one again ---------------------------------------------------------------------------------------------
_refs = {}


def reference(sky):
    """the oracle's eleven frames (camera, {buffer: bytes}), rendered once per environment for the builds that share them"""
    if sky not in _refs:
        sc = refit.street()
        desc = sc.desc()
        st = state(sc)
        o = Oracle(0); o.upload_scene(desc); o.resize(W, H)
        if sky:
            o.set_sun_and_sky(abi.SunAndSky(in_use=1))
        pose = sc.cameraPose()
        sc.updateCamera(W, H)
        frames = []
        for f, k in enumerate(OFFSETS):
            st.time = 1000 + f
            cam = camera(sc, pose, k)
            o.set_camera(cam); o.render_frame(st, f)
            frames.append((cam, {b: o.readback(b).copy() for b in frame_buffers(f)}))
        _refs[sky] = (sc, desc, frames)
    return _refs[sky]


# base and sky builds; the object-motion build (mode on, nothing in motion: the frames are the oracle's); serial launches; and a context whose frames alternate
# between the latency build, which writes the plane without reading it, and the throughput build, which then reads what the latency build wrote
@pytest.mark.parametrize("build", ["base", "sky", "object-motion", "base-serial", "latency-throughput-alternating"])
def test_frames_equal_the_oracle_with_a_warm_a_stale_and_a_warm_plane(build):
    sky = build == "sky"
    sc, desc, frames = reference(sky)
    st = state(sc)
    r = renderer(desc, overlap=0 if build == "base-serial" else None)
    if sky:
        r.set_sun_and_sky(abi.SunAndSky(in_use=1))
    if build == "object-motion":
        r.set_object_motion(abi.OBJECT_MOTION_ON)
    if build == "base":
        st_acc = r.accel_stats()
        print("street:", st_acc)
        assert st_acc["references"] > st_acc["triangles"]      # the scene has duplicate references: a seed may name either copy of a triangle
    for f, (cam, want) in enumerate(frames):
        st.time = 1000 + f
        if build == "latency-throughput-alternating":
            r.set_traversal(abi.TRAVERSAL_LATENCY if f % 2 == 0 else abi.TRAVERSAL_THROUGHPUT)
        r.set_camera(cam)
        r.run(st, f)
        assert bad_buffers(r, want) == {}, (build, f)
    img = r.readback(abi.BUF_DIRECT_RESULT0 + ((len(frames) - 1) & 1)).view(np.float32)
    assert np.isfinite(img).all() and img.max() > 0.01       # not comparing two empty frames
    r.destroy()


# ---- 2. the seed is used, and only removes work ----------------------------------------------------------------------------------------------------------------------
def _direct_once(r, st, counting=True):
    """one direct stage; returns its own counters (the context's are cumulative)"""
    r.set_counting(counting)
    before = r.counters()
    r.run_stage(st, 0, abi.STAGE_DIRECT)
    r.sync()
    after = r.counters()
    return {k: getattr(after, k) - getattr(before, k) for k in COUNTER_FIELDS}


@pytest.mark.parametrize("first", ["throughput", "latency"])
def test_a_warm_plane_removes_node_steps_and_changes_no_ray_and_no_word(first):
    """ReSTIRState none: the direct stage reads no history, so the same (time, frame) twice is the same frame twice.  Context A's second run, seeded by its first,
    against fresh context B's only run.  `first` = latency: A's first run is the latency build (counting off, which is what lets the context select it) — the plane
    it wrote must seed the counted throughput run just as well."""
    sc = refit.street()
    desc = sc.desc()
    st = state(sc)
    st.ReSTIRState = abi.RESTIR_NONE
    st.time = 1234
    sc.updateCamera(W, H); sc.updateCamera(W, H)
    cam = sc.getCamera()
    a, b = renderer(desc), renderer(desc)
    a.set_camera(cam); b.set_camera(cam)
    if first == "latency":
        a.set_traversal(abi.TRAVERSAL_LATENCY)
        _direct_once(a, st, counting=False)
        a.set_traversal(abi.TRAVERSAL_THROUGHPUT)
        cold = None
    else:
        cold = _direct_once(a, st)
    warm = _direct_once(a, st)
    fresh = _direct_once(b, st)
    print(first, "cold", cold, "warm", warm, "fresh", fresh)
    for buf in frame_buffers(0, indirect=False):
        assert optin.words(a.readback(buf), b.readback(buf)) == 0, abi.BUFFER_NAMES[buf]
    if cold is not None:
        assert cold == fresh                                   # an empty plane: the unseeded trace, step for step
    assert fresh["closestHitRays"] == W * H
    assert warm["closestHitRays"] == fresh["closestHitRays"] and warm["anyHitRays"] == fresh["anyHitRays"]
    assert warm["hitsShaded"] == fresh["hitsShaded"] and warm["risCandidates"] == fresh["risCandidates"]
    assert warm["nodesVisited"] < fresh["nodesVisited"]
    a.destroy(); b.destroy()


# ---- 3. seeds that point nowhere: another scene, another order of the records, moved triangles ------------------------------------------------------------------------
def test_a_smaller_scene_a_rebuild_and_moved_instances_in_one_context():
    """One context and one oracle through the same calls, no rt_resize in between: two frames of the street; upload + build of the Cornell box (far fewer records than
    the street's seeds name); rt_rebuild_accel (same records, new order); rt_update_instances (same indices, moved triangles).  Two frames after each equal the oracle."""
    big, small = refit.street(), refit.cornell()
    r = renderer(big.desc(), overlap=0)
    o = Oracle(0); o.upload_scene(big.desc()); o.resize(W, H)
    refs_big = r.accel_stats()["references"]
    f = 0

    def two_frames(sc, st, pose, what):
        nonlocal f
        for _ in range(2):
            st.time = 1000 + f
            cam = camera(sc, pose, 0)
            r.set_camera(cam); o.set_camera(cam)
            r.run(st, f); o.render_frame(st, f)
            bad = bad_buffers(r, {b: o.readback(b) for b in frame_buffers(f)})
            assert bad == {}, (what, f, bad)
            f += 1

    big.updateCamera(W, H)
    two_frames(big, state(big), big.cameraPose(), "street")
    desc = small.desc()
    r.load_scene(desc); o.upload_scene(desc)
    assert r.accel_stats()["references"] * 8 < refs_big           # what the plane held lies beyond the new record array
    st, pose = state(small), small.cameraPose()
    st.fireflyClampThreshold = 100.0
    small.updateCamera(W, H)
    two_frames(small, st, pose, "cornell after the street")
    r.rebuild_accel()
    two_frames(small, st, pose, "after rt_rebuild_accel")
    ids = [3, 5]
    ext = float(max(np.abs(np.concatenate(refit.world_bounds(desc, i))).max() for i in range(desc.numInstances)))
    xf = np.stack([refit.move_matrix("rotate", desc, i, ext) for i in ids])
    r.update_instances(ids, xf)
    small.updateInstances(np.asarray(ids, np.uint32), np.asarray(xf, np.float32))
    desc = small.desc()
    r.update_lights(desc); o.upload_scene(desc)
    two_frames(small, st, pose, "after rt_update_instances")
    r.destroy()


# ---- 4. row bands ----------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("traversal", [abi.TRAVERSAL_THROUGHPUT, abi.TRAVERSAL_AUTO], ids=["throughput", "auto"])
def test_the_direct_stage_in_three_ragged_bands_after_a_full_frame(traversal):
    """a full frame warms the plane; the next frame's direct stage runs as the bands [0, 16), [16, 24), [24, 50) — each reads and writes its own rows of the plane
    (auto: bands this small take the latency build) —, and one more full direct stage follows on the plane the bands left"""
    sc = refit.street()
    desc = sc.desc()
    st = state(sc)
    pose = sc.cameraPose()
    r = renderer(desc, overlap=0, traversal=traversal)
    o = Oracle(0); o.upload_scene(desc); o.resize(W, H)
    sc.updateCamera(W, H)
    for f in range(3):
        st.time = 1000 + f
        cam = camera(sc, pose, 0)
        r.set_camera(cam); o.set_camera(cam)
        if f == 0:
            r.run(st, f); o.render_frame(st, f)
            bufs = frame_buffers(f)
        else:
            for y0, y1 in (((0, 16), (16, 24), (24, H)) if f == 1 else ((0, 0),)):
                r.run_stage(st, f, abi.STAGE_DIRECT, 0, y0, y1)
            o.run_stage(st, f, abi.STAGE_DIRECT)
            bufs = frame_buffers(f, indirect=False)
        assert bad_buffers(r, {b: o.readback(b) for b in bufs}) == {}, f
    r.destroy()


# ---- 5. equal calls, equal counters ----------------------------------------------------------------------------------------------------------------------------------
def test_two_contexts_with_the_same_calls_report_the_same_counters():
    """frames, a resize, frames, a rebuild, frames, a host build, frames — on two contexts: every counter and every buffer agree (the plane is emptied where the record
    order or the image changes, on the context's stream, so neither context starts a frame warmer than the other)"""
    sc = refit.street()
    desc = sc.desc()
    pose = sc.cameraPose()
    rs = [renderer(desc), renderer(desc)]
    for r in rs:
        r.set_counting(True)
    f = 0
    size = (W, H)

    def frames(n):
        nonlocal f
        st = state(sc, *size)
        for _ in range(n):
            st.time = 1000 + f
            cam = camera(sc, pose, 0, *size)
            for r in rs:
                r.set_camera(cam); r.run(st, f)
            f += 1

    sc.updateCamera(*size)
    frames(3)
    size = (45, 67)
    for r in rs:
        r.update(*size)
    sc.updateCamera(*size)
    frames(2)
    for r in rs:
        r.rebuild_accel()
    frames(2)
    for r in rs:
        assert refit.hip_build_accel(r) == 0
    frames(2)
    ca, cb = rs[0].counters(), rs[1].counters()
    for field in COUNTER_FIELDS:
        assert getattr(ca, field) == getattr(cb, field), field
    assert ca.closestHitRays > 0 and ca.nodesVisited > 0
    for b in frame_buffers(f - 1):
        assert optin.words(rs[0].readback(b), rs[1].readback(b)) == 0, abi.BUFFER_NAMES[b]
    for r in rs:
        r.destroy()
