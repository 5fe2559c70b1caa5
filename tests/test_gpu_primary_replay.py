"""Settled primary visibility: while camera and scene are at rest the direct stage stops tracing its primary ray — the third launch at a camera
records, per pixel, the closest deterministic accept and the stochastic candidates in front of it, later launches re-test those records with the frame's seed.
Not a bit of any buffer may change: every comparison is word for word against the oracle (or a second context) over all frame buffers, and
rt_get_primary_replay_stats shows that the record and replay launches happened where the test expects them — and nowhere else.

Shapes: 70 x 50 — ragged against the 8 x 8 tile, 9 x 7 tiles, a pixel count that is no multiple of 64 — of the exterior street scene at a few thousand triangles
(tests/refit.py street(): instanced trees with alpha-tested leaf cards, mirrored props, long thin triangles that the builder splits into duplicate references), so
that pixels have stochastic candidates in front of their deterministic hit; one 8 x 8 and one 9 x 1 image.  Images this small would take the latency build under
RT_TRAVERSAL_AUTO, so the tests name the throughput build.  RESTIR_VIS_K and RESTIR_PRIMARY_REPLAY are read once per process: those cases run this file as a
program in a fresh child process."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from helpers import ROOT, abi, host, frame_buffers
from oracle.binding import Oracle
import optin
import refit
import skin

pytestmark = pytest.mark.gpu

W, H = 70, 50
STEP = np.array([0.05, 0.012, -0.04], dtype=np.float32)
# at rest for 7 frames (normal, normal, record, replay x 4), moved for 2, at rest for 3 (normal, normal, record)
OFFSETS = [0] * 7 + [1, 2] + [3] * 3
LAUNCHES = [(0, 0), (0, 0), (1, 0), (1, 1), (1, 2), (1, 3), (1, 4), (1, 4), (1, 4), (1, 4), (1, 4), (2, 4)]   # (recorded, replayed) after each frame
REST5 = [(0, 0), (0, 0), (1, 0), (1, 1), (1, 2)]
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
    """the scene's camera moved k steps off its pose, history matrices advanced as SampleExample::updateFrame does (so two frames at rest differ in their history
    matrices and in nothing a primary ray reads); returns a copy"""
    eye, center, up, fov = pose
    sc.setCamera(eye + np.float32(k) * STEP, center, up, fov)
    sc.updateCamera(w, h)
    cam = sc.getCamera()
    return type(cam).from_buffer_copy(cam)


def foliage_pose(sc, desc):
    """a pose a little more than one tree size away from the crown of the last alpha-tested tree instance, looking at it: from the scene's own pose the trees are a
    few pixels, and the test is about the primary rays that cross leaf cards — through their cut-out cells in most pixels, so that stochastic candidates lie in
    front of the deterministic hit behind the tree"""
    i = int(refit.describe(desc)["alpha"][-1])
    lo, hi = refit.world_bounds(desc, i)
    c, size = 0.5 * (lo + hi), float((hi - lo).max())
    _, _, up, fov = sc.cameraPose()
    return (c + size * np.array([-1.2, 0.1, 0.2])).astype(np.float32), c.astype(np.float32), up, fov


def bad_buffers(r, want):
    bad = {abi.BUFFER_NAMES[b]: optin.words(r.readback(b), w) for b, w in want.items()}
    return {k: v for k, v in bad.items() if v}


def launches(r):
    s = r.primary_replay_stats()
    return (s.launchesRecorded, s.launchesReplayed)


_refs = {}


def street_at_the_foliage():
    sc = refit.street()
    desc = sc.desc()
    return sc, desc, foliage_pose(sc, desc)


def reference(sky=False, w=W, h=H, offsets=OFFSETS, scene=street_at_the_foliage):
    """the oracle's frames (camera, {buffer: bytes}) of one sequence, rendered once and shared by the tests that need them; scene: a function that returns
    (host scene, description, camera pose)"""
    key = (sky, w, h, tuple(offsets), scene.__name__)
    if key not in _refs:
        sc, desc, pose = scene()
        st = state(sc, w, h)
        o = Oracle(0); o.upload_scene(desc); o.resize(w, h)
        if sky:
            o.set_sun_and_sky(abi.SunAndSky(in_use=1))
        sc.updateCamera(w, h)
        frames = []
        for f, k in enumerate(offsets):
            st.time = 1000 + f
            cam = camera(sc, pose, k, w, h)
            o.set_camera(cam); o.render_frame(st, f)
            frames.append((cam, {b: o.readback(b).copy() for b in frame_buffers(f)}))
        _refs[key] = (sc, desc, frames)
    return _refs[key]


def run_sequence(build, w=W, h=H, offsets=OFFSETS, expect=LAUNCHES, setup=None, scene=street_at_the_foliage):
    """the sequence on a fresh context; returns (problems, stats after the last frame).  expect: (recorded, replayed) after each frame"""
    sky = build == "sky"
    sc, desc, frames = reference(sky, w, h, offsets, scene)
    st = state(sc, w, h)
    r = renderer(desc, w, h, overlap=0 if build == "serial" else None)
    if sky:
        r.set_sun_and_sky(abi.SunAndSky(in_use=1))
    if setup is not None:
        setup(r)
    problems = []
    for f, (cam, want) in enumerate(frames):
        st.time = 1000 + f
        r.set_camera(cam)
        r.run(st, f)
        bad = bad_buffers(r, want)
        if bad:
            problems.append(("buffers", f, bad))
        if launches(r) != tuple(expect[f]):
            problems.append(("launches", f, launches(r), tuple(expect[f])))
    s = r.primary_replay_stats()
    stats = {k: getattr(s, k) for k in ("state", "K", "pixelsSettled", "pixelsListed", "pixelsOverflow", "launchesRecorded", "launchesReplayed")}
    img = r.readback(abi.BUF_DIRECT_RESULT0 + ((len(frames) - 1) & 1)).view(np.float32)
    if not (np.isfinite(img).all() and img.max() > 0.01):
        problems.append(("empty frame",))
    r.destroy()
    return problems, stats


# ---- 1. twelve frames: rest, move, rest ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("build", ["base", "sky", "serial"])
def test_twelve_frames_equal_the_oracle_and_record_and_replay_where_expected(build):
    problems, stats = run_sequence(build)
    print(build, stats)
    assert problems == []
    assert stats["state"] == 1 and stats["pixelsSettled"] + stats["pixelsListed"] + stats["pixelsOverflow"] == W * H
    assert stats["pixelsListed"] + stats["pixelsOverflow"] > 0     # the street has alpha-tested cards in front of opaque surfaces: R is more than {d*} somewhere


# (the third case is the one that reaches the build sky_rp_cnt: sun & sky and counting on, recorded and replayed)
@pytest.mark.parametrize("size,build,counting", [((8, 8), "base", False), ((9, 1), "base", False), ((8, 8), "sky", True)], ids=["8x8", "9x1", "8x8-sky-counting"])
def test_one_tile_and_one_row(size, build, counting):
    problems, stats = run_sequence(build, *size, offsets=[0] * 5, expect=REST5, setup=(lambda r: r.set_counting(True)) if counting else None)
    print(size, stats)
    assert problems == [] and stats["state"] == 1
    assert stats["pixelsSettled"] + stats["pixelsListed"] + stats["pixelsOverflow"] == size[0] * size[1]


# ---- 2. the list length, and the switch: fresh processes ---------------------------------------------------------------------------------------------------------
def child(build, **env):
    e = dict(os.environ)
    for k in ("RESTIR_VIS_K", "RESTIR_PRIMARY_REPLAY", "RESTIR_VIS_REST_FRAMES"):
        e.pop(k, None)
    e.update(env)
    p = subprocess.run([sys.executable, os.path.abspath(__file__), build], capture_output=True, text=True, timeout=600, env=e, cwd=ROOT)
    assert p.returncode == 0, (p.returncode, p.stdout[-2000:], p.stderr[-2000:])
    return json.loads(p.stdout.strip().splitlines()[-1])


def test_list_length_one_mixes_settled_listed_and_overflow_pixels():
    out = child("base", RESTIR_VIS_K="1")
    print(out)
    assert out["problems"] == [] and out["stats"]["K"] == 1
    s = out["stats"]
    assert s["pixelsSettled"] > 0 and s["pixelsListed"] > 0 and s["pixelsOverflow"] > 0     # foliage pixels overflow, their neighbours do not
    assert s["pixelsSettled"] + s["pixelsListed"] + s["pixelsOverflow"] == W * H


def test_default_list_length_in_a_fresh_process():
    out = child("base")
    print(out)
    assert out["problems"] == [] and out["stats"]["K"] in (8, 16, 32, 64) and out["stats"]["state"] == 1


def test_switched_off_by_the_environment():
    out = child("off", RESTIR_PRIMARY_REPLAY="0")
    print(out)
    assert out["problems"] == [] and out["stats"]["state"] == 0 and out["stats"]["launchesRecorded"] == 0 and out["stats"]["launchesReplayed"] == 0


# ---- 3. calls that change what a primary ray hits, with the camera at rest ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("call", ["update_instances", "update_vertices", "rebuild_accel", "resize", "upload_scene"])
def test_a_scene_or_target_change_at_rest_drops_the_state(call):
    """four frames at rest (the state is VALID and a replay has run), the call, two more frames at the same camera: the state is NONE right after the call, neither
    of the two frames replays, and both equal the oracle that was given the same change"""
    sc = refit.street()
    desc = sc.desc()
    size = (W, H)
    r = renderer(desc, overlap=0)
    o = Oracle(0); o.upload_scene(desc); o.resize(W, H)
    st, pose = state(sc), foliage_pose(sc, desc)
    sc.updateCamera(W, H)
    f = 0

    def frames(n, what):
        nonlocal f
        for _ in range(n):
            st.time = 1000 + f
            cam = camera(sc, pose, 0, *size)
            r.set_camera(cam); o.set_camera(cam)
            r.run(st, f); o.render_frame(st, f)
            bad = bad_buffers(r, {b: o.readback(b) for b in frame_buffers(f)})
            assert bad == {}, (what, f, bad)
            f += 1

    frames(4, "at rest")
    assert launches(r) == (1, 1) and r.primary_replay_stats().state == 1
    if call == "update_instances":
        ids = [int(refit.describe(desc)["alpha"][-1]), int(refit.describe(desc)["mirrored"][0])]      # the tree in view and a mirrored prop
        ext = float(max(np.abs(np.concatenate(refit.world_bounds(desc, i))).max() for i in range(desc.numInstances)))
        xf = np.stack([refit.move_matrix("rotate", desc, i, ext) for i in ids])
        r.update_instances(ids, xf)
        sc.updateInstances(np.asarray(ids, np.uint32), np.asarray(xf, np.float32))
        desc = sc.desc()
        r.update_lights(desc); o.upload_scene(desc)
    elif call == "update_vertices":
        m = int(refit.instances_of(desc)["primMesh"][int(refit.describe(desc)["alpha"][-1])])          # the mesh of the tree in view
        first, count = skin.mesh_range(desc, m)
        verts = skin.vertices_of(desc)
        rows = verts[first:first + count].copy()
        rows["position"] += np.float32(0.25)
        r.update_vertices(m, 0, rows)
        verts[first:first + count] = rows
        o.upload_scene(skin.with_vertices(desc, verts))
    elif call == "rebuild_accel":
        r.rebuild_accel()          # same triangles, the leaf records in a new order: what the planes hold names other triangles now
    elif call == "resize":
        size = (50, 70)            # as many pixels as before: a plane of the old size would be read without leaving it
        r.update(*size); o.resize(*size)
        st = state(sc, *size)
        sc.updateCamera(*size)
    else:
        sc = refit.cornell()       # far fewer records than the planes' entries name
        desc = sc.desc()
        r.load_scene(desc); o.upload_scene(desc)
        st, pose = state(sc), sc.cameraPose()
        st.fireflyClampThreshold = 100.0
        sc.updateCamera(W, H)
    s = r.primary_replay_stats()
    assert s.state == 0 and (s.launchesRecorded, s.launchesReplayed) == (1, 1)
    frames(2, "after " + call)
    assert launches(r) == (1, 1) and r.primary_replay_stats().state == 0
    frames(2, "at rest after " + call)     # ... and the third launch at the camera records again, the fourth replays
    assert launches(r) == (2, 2)
    r.destroy()


# ---- 4. launches that never replay ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["taa", "object-motion", "vertex-motion", "latency"])
def test_never_entered_with_taa_motion_vectors_or_the_latency_build(mode):
    sc, desc, frames = reference(False, W, H, [0] * 5)
    st = state(sc)
    r = renderer(desc, traversal=abi.TRAVERSAL_LATENCY if mode == "latency" else abi.TRAVERSAL_THROUGHPUT)
    o = None
    if mode == "taa":
        r.set_taa(mode=abi.TAA_ON)
        o = Oracle(0); o.upload_scene(desc); o.resize(W, H)
    elif mode == "object-motion":
        r.set_object_motion(abi.OBJECT_MOTION_ON)
    elif mode == "vertex-motion":
        r.set_object_motion(abi.OBJECT_MOTION_VERTEX)
    for f, (cam, want) in enumerate(frames):
        st.time = 1000 + f
        r.set_camera(cam)
        r.run(st, f)
        if o is not None:      # the oracle's frame with the jittered camera of this frame
            o.set_camera(r.taa_jitter_camera(cam, f, abi.Taa().jitterPhases, W, H)); o.render_frame(st, f)
            want = {b: o.readback(b) for b in frame_buffers(f)}
        assert bad_buffers(r, want) == {}, (mode, f)
        s = r.primary_replay_stats()
        assert (s.state, s.launchesRecorded, s.launchesReplayed) == (0, 0, 0), (mode, f)
    r.destroy()


def test_a_band_launch_drops_the_state():
    """four direct stages at rest (valid, one replay), then the next frame's direct stage in three ragged bands, then full direct stages again"""
    sc = refit.street()
    desc = sc.desc()
    st, pose = state(sc), foliage_pose(sc, desc)
    r = renderer(desc, overlap=0)
    o = Oracle(0); o.upload_scene(desc); o.resize(W, H)
    sc.updateCamera(W, H)
    want_launches = [(0, 0), (0, 0), (1, 0), (1, 1), (1, 1), (1, 1), (1, 1), (2, 1), (2, 2)]
    for f in range(9):
        st.time = 1000 + f
        cam = camera(sc, pose, 0)
        r.set_camera(cam); o.set_camera(cam)
        for y0, y1 in (((0, 16), (16, 24), (24, H)) if f == 4 else ((0, 0),)):
            r.run_stage(st, f, abi.STAGE_DIRECT, 0, y0, y1)
        o.run_stage(st, f, abi.STAGE_DIRECT)
        assert bad_buffers(r, {b: o.readback(b) for b in frame_buffers(f, indirect=False)}) == {}, f
        assert launches(r) == want_launches[f], f
        if f == 4:
            assert r.primary_replay_stats().state == 0
    r.destroy()


# ---- 5. counters -----------------------------------------------------------------------------------------------------------------------------------------------------
def _direct_once(r, st):
    """one direct stage with counting on; returns its own counters (the context's are cumulative)"""
    r.set_counting(True)
    before = r.counters()
    r.run_stage(st, 0, abi.STAGE_DIRECT)
    r.sync()
    after = r.counters()
    return {k: getattr(after, k) - getattr(before, k) for k in COUNTER_FIELDS}


def test_a_replay_counts_the_same_rays_and_fewer_node_steps():
    """ReSTIRState none: the direct stage reads no history, so the same (time, frame) again is the same frame again.  Contexts A and A2 issue the same five launches
    (normal, normal, record, replay, replay), fresh context B one: A's replay reports B's rays, shaded hits and RIS candidates and strictly fewer node steps, its
    buffers are B's, and A and A2 agree in every counter of every launch."""
    sc = refit.street()
    desc = sc.desc()
    st = state(sc)
    st.ReSTIRState = abi.RESTIR_NONE
    st.time = 1234
    sc.updateCamera(W, H)
    cam = camera(sc, foliage_pose(sc, desc), 0)
    a, a2, b = renderer(desc), renderer(desc), renderer(desc)
    for r in (a, a2, b):
        r.set_camera(cam)
    runs = [[_direct_once(r, st) for _ in range(5)] for r in (a, a2)]
    fresh = _direct_once(b, st)
    print("fresh", fresh)
    for k, c in enumerate(runs[0]):
        print(k, c)
    assert launches(a) == (1, 2) and launches(a2) == (1, 2) and launches(b) == (0, 0)
    assert runs[0] == runs[1]
    for buf in frame_buffers(0, indirect=False):
        assert optin.words(a.readback(buf), b.readback(buf)) == 0, abi.BUFFER_NAMES[buf]
    assert fresh["closestHitRays"] == W * H
    for c in runs[0]:                  # a recorded and a replayed query count as one query each
        for k in ("closestHitRays", "anyHitRays", "hitsShaded", "risCandidates"):
            assert c[k] == fresh[k], k
    seeded, recorded, replayed = runs[0][1], runs[0][2], runs[0][3]
    assert replayed["nodesVisited"] < seeded["nodesVisited"] < fresh["nodesVisited"]
    assert recorded["nodesVisited"] > seeded["nodesVisited"]      # the recording traces twice
    assert runs[0][4] == replayed
    for r in (a, a2, b):
        r.destroy()


# ---- 6. frames in flight -----------------------------------------------------------------------------------------------------------------------------------------------
def test_forty_frames_at_rest_in_flight_equal_forty_serial_frames():
    sc = refit.street()
    desc = sc.desc()
    st, pose = state(sc), foliage_pose(sc, desc)
    rs = [renderer(desc, overlap=2), renderer(desc, overlap=0)]
    sc.updateCamera(W, H)
    for f in range(40):
        st.time = 1000 + f
        cam = camera(sc, pose, 0)
        for r in rs:
            r.set_camera(cam); r.run(st, f)
        if f in (3, 20, 39):      # (a readback drains the frames in flight: only here)
            for b in frame_buffers(f):
                assert optin.words(rs[0].readback(b), rs[1].readback(b)) == 0, (f, abi.BUFFER_NAMES[b])
    for r in rs:
        assert launches(r) == (1, 37)
        r.destroy()


if __name__ == "__main__":
    # a fresh process for the cases whose environment variable is read once: the twelve frames of test 1 on one build ("off": with the launches of a context
    # that never records); one JSON line
    which = sys.argv[1]
    from restir_amd import build as _build
    _build.build_host(); _build.build_hip()
    from oracle import binding as _binding
    _binding.build()
    problems, stats = run_sequence("base" if which == "off" else which, expect=[(0, 0)] * len(OFFSETS) if which == "off" else LAUNCHES)
    print(json.dumps({"problems": problems, "stats": stats}))
