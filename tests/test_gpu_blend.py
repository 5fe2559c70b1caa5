"""Alpha-blended surfaces on the GPU.  Every non-opaque material of the procedural scenes is RT_ALPHA_MASK, whose opacity is 0 or 1: the alpha
draw keyed on (ray seed, triangle id) then decides nothing, and no frame of the rest of the suite has a pixel whose primary hit depends on the frame's seed.  The
veiled scenes of tests/blend.py and the glTF fixture tests/golden/blend_panes.gltf do (tests/test_blend_cpu.py holds that premise on the oracle: at least 10 % of
the G-buffer texels change from one frame at rest to the next).  Here the paths that rest on "a verdict depends on (ray, triangle) alone" run on them: whole
frames on both traversal builds, rt_trace_rays with per-ray seeds, settled primary visibility (§25), the wide tail, a two-entry LDS stack, refits and rebuilds,
the opacity micro-map against float64, reference mode.

Every comparison is word for word (optin.words over helpers.frame_buffers against the oracle); the only other numbers are the binomial bound of the draw's
distribution (blend.binomial_bound) and the 10 % of W x H that a replay case must report as listed or overflow pixels.  Images this small would take the latency
build under RT_TRAVERSAL_AUTO, so the cases name their build.  RESTIR_VIS_K and RESTIR_STACK_LDS are read once per process: those cases run this file as a
program in a fresh child process."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from helpers import ROOT, abi, frame_buffers
from oracle.binding import Oracle
import blend
import optin
import refit
import skin
from test_gpu_primary_replay import run_sequence, OFFSETS, LAUNCHES, launches, bad_buffers
from test_gpu_wide_tail import renderer as tail_renderer

pytestmark = pytest.mark.gpu

SIZES = [(8, 8), (13, 11), (70, 50)]
W, H = 70, 50
BUILDS = {"throughput": abi.TRAVERSAL_THROUGHPUT, "latency": abi.TRAVERSAL_LATENCY}
STEP = np.array([0.05, 0.012, -0.04], dtype=np.float32)

_scenes = {}


def scene(name):
    """(host scene, veiled description) of blend.scene, made once"""
    if name not in _scenes:
        sc, _, veiled = blend.scene(name)
        _scenes[name] = (sc, veiled, sc.cameraPose())
    return _scenes[name][:2]


def home(name):
    """the scene's own camera pose (the tests move the shared scene's camera)"""
    scene(name)
    return _scenes[name][2]


def renderer(desc, w, h, traversal=abi.TRAVERSAL_THROUGHPUT, overlap=0):
    from restir_amd.renderer import Renderer
    r = Renderer().setup(0)
    r.set_overlap(overlap)
    r.load_scene(desc)
    r.update(w, h)
    r.set_traversal(traversal)
    return r


def oracle(desc, w, h):
    o = Oracle(0)
    o.upload_scene(desc)
    o.resize(w, h)
    return o


def camera(sc, pose, k, w, h):
    eye, center, up, fov = pose
    sc.setCamera(eye + np.float32(k) * STEP, center, up, fov)
    sc.updateCamera(w, h)
    cam = sc.getCamera()
    return type(cam).from_buffer_copy(cam)


def frames_equal(r, o, sc, st, pose, w, h, first, count, what, move=0, indirect=True):
    """`count` frames from frame index `first` on both sides, the camera `move` steps further each frame; every buffer word for word after each"""
    for f in range(first, first + count):
        st.time = 1000 + f
        cam = camera(sc, pose, move * f, w, h)
        r.set_camera(cam); o.set_camera(cam)
        r.run(st, f); o.render_frame(st, f)
        bad = bad_buffers(r, {b: o.readback(b) for b in frame_buffers(f, indirect)})
        assert bad == {}, (what, "frame", f, bad)


# ---- a. frames ----------------------------------------------------------------------------------------------------------------------------------------------------
_frame_refs = {}


def frame_reference(name, w, h, sky):
    """the oracle's three frames with a moving camera, rendered once per (scene, size) and shared by the builds and schedules"""
    key = (name, w, h, sky)
    if key not in _frame_refs:
        sc, desc = scene(name)
        st, pose = blend.state(sc, w, h), home(name)
        o = oracle(desc, w, h)
        if sky:
            o.set_sun_and_sky(abi.SunAndSky(in_use=1))
        sc.updateCamera(w, h)
        frames = []
        for f in range(3):
            st.time = 1000 + f
            cam = camera(sc, pose, f, w, h)
            o.set_camera(cam); o.render_frame(st, f)
            frames.append((cam, {b: o.readback(b).copy() for b in frame_buffers(f)}))
        _frame_refs[key] = frames
    return _frame_refs[key]


def run_frames(name, w, h, build, overlap, sky=False):
    sc, desc = scene(name)
    frames = frame_reference(name, w, h, sky)
    st = blend.state(sc, w, h)
    r = renderer(desc, w, h, BUILDS[build], overlap)
    if sky:
        r.set_sun_and_sky(abi.SunAndSky(in_use=1))
    for f, (cam, want) in enumerate(frames):
        st.time = 1000 + f
        r.set_camera(cam)
        r.run(st, f)
        assert bad_buffers(r, want) == {}, (name, w, h, build, overlap, "frame", f)
    r.destroy()


@pytest.mark.parametrize("overlap", [0, 2], ids=["serial", "frames-in-flight"])
@pytest.mark.parametrize("build", list(BUILDS))
@pytest.mark.parametrize("size", SIZES, ids=["%dx%d" % s for s in SIZES])
@pytest.mark.parametrize("name", ["cornell", "street", "gltf"])
def test_three_frames_with_a_moving_camera_equal_the_oracle(name, size, build, overlap):
    run_frames(name, *size, build, overlap)


def test_three_frames_on_the_sky_build_equal_the_oracle():
    run_frames("street", 13, 11, "throughput", 0, sky=True)


# ---- b. rays ------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["cornell", "street", "gltf"])
def test_trace_rays_with_random_seeds_equals_the_oracles_brute_force(name):
    sc, desc = scene(name)
    rays = blend.random_rays(desc, 20000, 31)
    o = Oracle(0); o.upload_scene(desc)
    from restir_amd.renderer import Renderer
    r = Renderer().setup(0); r.load_scene(desc)
    want = o.trace_closest(rays, brute=True)
    got = r.trace_closest(rays)
    assert optin.words(got, want) == 0
    hit = want[:, 0] < 1e27
    assert hit.mean() > 0.1                      # (not vacuous; half of the rays are aimed at blended instances)
    # any-hit with the range just behind and just in front of the closest accept of the same seed: the draw is the same draw, so the verdicts are fixed
    for factor, verdict in ((1.001, 1), (0.999, 0)):
        q = rays.copy()
        q[:, 6] = np.where(hit, want[:, 0].astype(np.float64) * factor, 1.0).astype(np.float32)
        a = r.trace_any(q)
        assert np.array_equal(a, o.trace_any(q)), (factor, int((a != o.trace_any(q)).sum()))
        assert (a[hit] == verdict).all(), (factor, int((a[hit] != verdict).sum()))
    r.destroy()


@pytest.mark.parametrize("alpha", [0.25, 0.5, 0.7])
def test_the_alpha_draw_accepts_with_probability_alpha_on_the_gpu(alpha):
    from restir_amd.renderer import Renderer
    sc = refit.cornell()
    r = Renderer().setup(0); r.load_scene(blend.all_blended(sc, alpha))
    blend.check_distribution(r.trace_closest, alpha)
    r.destroy()


# ---- c. settled primary visibility ---------------------------------------------------------------------------------------------------------------------------------
def veiled_street_at_the_scene_pose():
    sc, desc = scene("street")
    return sc, desc, home("street")


def check_replay_stats(stats, w=W, h=H):
    assert stats["state"] == 1 and stats["pixelsSettled"] + stats["pixelsListed"] + stats["pixelsOverflow"] == w * h
    assert stats["pixelsListed"] + stats["pixelsOverflow"] >= 0.10 * w * h, stats


def test_twelve_frames_of_rest_move_rest_on_the_veiled_street():
    problems, stats = run_sequence("base", offsets=OFFSETS, expect=LAUNCHES, scene=veiled_street_at_the_scene_pose)
    print(stats)
    assert problems == []
    check_replay_stats(stats)


def child(what, **env):
    e = dict(os.environ)
    for k in ("RESTIR_VIS_K", "RESTIR_PRIMARY_REPLAY", "RESTIR_VIS_REST_FRAMES", "RESTIR_STACK_LDS", "RESTIR_WIDE_TAIL"):
        e.pop(k, None)
    e.update(env)
    p = subprocess.run([sys.executable, os.path.abspath(__file__), what], capture_output=True, text=True, timeout=600, env=e, cwd=ROOT)
    assert p.returncode == 0, (p.returncode, p.stdout[-2000:], p.stderr[-2000:])
    return json.loads(p.stdout.strip().splitlines()[-1])


def test_list_length_one_on_the_veiled_street():
    out = child("replay", RESTIR_VIS_K="1")
    print(out)
    s = out["stats"]
    assert out["problems"] == [] and s["K"] == 1
    assert s["pixelsSettled"] > 0 and s["pixelsListed"] > 0 and s["pixelsOverflow"] > 0
    check_replay_stats(s)


def test_list_length_sixty_four_on_the_veiled_street():
    out = child("replay", RESTIR_VIS_K="64")
    print(out)
    assert out["problems"] == [] and out["stats"]["K"] == 64
    check_replay_stats(out["stats"])


def test_thirty_two_replays_with_thirty_two_seeds():
    """ReSTIRState none: the direct stage reads no history, so each launch is its (time, camera) alone.  Three launches bring the context to VALID; the next 32, each
    with another st.time, replay the one recording and must each equal the oracle's direct stage at that time"""
    sc, desc, pose = veiled_street_at_the_scene_pose()
    st = blend.state(sc, W, H)
    st.ReSTIRState = abi.RESTIR_NONE
    r, o = renderer(desc, W, H), oracle(desc, W, H)
    sc.updateCamera(W, H)
    cam = camera(sc, pose, 0, W, H)
    r.set_camera(cam); o.set_camera(cam)
    gbuffers = set()
    for k in range(35):
        st.time = 1000 + k if k < 3 else 5000 + 7919 * k
        r.run_stage(st, 0, abi.STAGE_DIRECT); o.run_stage(st, 0, abi.STAGE_DIRECT)
        want = {b: o.readback(b) for b in frame_buffers(0, indirect=False)}
        assert bad_buffers(r, want) == {}, k
        gbuffers.add(want[abi.BUF_GBUFFER0].tobytes())
        assert launches(r) == (min(k // 2, 1) if k < 3 else 1, max(0, k - 2)), k
    assert launches(r) == (1, 32) and len(gbuffers) == 35      # ... and no two of the frames stopped at the same surfaces
    s = r.primary_replay_stats()
    assert s.pixelsListed + s.pixelsOverflow >= 0.10 * W * H
    r.destroy()


def test_the_halves_of_the_spatial_modes_record_and_replay():
    """RT_RESTIR_SPATIOTEMPORAL: six frames at rest through rt_render_frame, then six whose direct stage is issued as its two halves (level 1 spawns the primary
    rays and passes through the rule of primary_replay.h, level 2 is no launch for it) — the camera moves once among them, so that a recording happens in a half too"""
    sc, desc, pose = veiled_street_at_the_scene_pose()
    st = blend.state(sc, W, H)
    st.ReSTIRState = abi.RESTIR_SPATIOTEMPORAL
    r, o = renderer(desc, W, H), oracle(desc, W, H)
    sc.updateCamera(W, H)
    offsets = [0] * 6 + [0, 0, 1, 1, 1, 1]
    expect = [(0, 0), (0, 0), (1, 0), (1, 1), (1, 2), (1, 3), (1, 4), (1, 5), (1, 5), (1, 5), (2, 5), (2, 6)]
    for f, k in enumerate(offsets):
        st.time = 1000 + f
        cam = camera(sc, pose, k, W, H)
        r.set_camera(cam); o.set_camera(cam)
        if f < 6:
            r.run(st, f); o.render_frame(st, f)
            bufs = frame_buffers(f)
        else:
            for level in (1, 2):
                r.run_stage(st, f, abi.STAGE_DIRECT, level); o.run_stage(st, f, abi.STAGE_DIRECT, level)
                if level == 1:
                    assert launches(r) == expect[f], (f, "after level 1")
            bufs = frame_buffers(f, indirect=False) + [abi.BUF_DIRECT_RESV_TEMP]
        assert bad_buffers(r, {b: o.readback(b) for b in bufs}) == {}, f
        assert launches(r) == expect[f], f
    s = r.primary_replay_stats()
    assert s.state == 1 and s.pixelsListed + s.pixelsOverflow >= 0.10 * W * H
    r.destroy()


def test_switches_in_the_middle_of_a_stay():
    """at rest throughout.  Counting on and off and sun & sky on and off choose another kernel for the same recording: the state stays and the launches go on
    replaying.  One launch of the latency build drops it: the stay starts over"""
    sc, desc, pose = veiled_street_at_the_scene_pose()
    st = blend.state(sc, W, H)
    r, o = renderer(desc, W, H), oracle(desc, W, H)
    sc.updateCamera(W, H)
    f = 0

    def frames(n, what, expect):
        nonlocal f
        frames_equal(r, o, sc, st, pose, W, H, f, n, what)
        f += n
        assert launches(r) == expect, (what, launches(r))

    def sky(on):
        ss = abi.SunAndSky(in_use=1 if on else 0)
        r.set_sun_and_sky(ss); o.set_sun_and_sky(ss)

    frames(4, "at rest", (1, 1))
    r.set_counting(True); frames(1, "counting on", (1, 2))
    r.set_counting(False); frames(1, "counting off", (1, 3))
    sky(True); frames(1, "sun and sky", (1, 4))
    sky(False); frames(1, "no sun and sky", (1, 5))
    assert r.primary_replay_stats().state == 1
    r.set_traversal(abi.TRAVERSAL_LATENCY); frames(1, "latency build", (1, 5))
    assert r.primary_replay_stats().state == 0
    r.set_traversal(abi.TRAVERSAL_THROUGHPUT); frames(2, "throughput build again", (1, 5))
    frames(2, "the stay starts over", (2, 6))
    r.destroy()


# ---- d. launch shapes -----------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", [(24, 16), (13, 11)], ids=["24x16", "13x11"])
def test_the_wide_tail_on_and_off(size):
    sc, desc = scene("street")
    w, h = size
    o = oracle(desc, w, h)
    rs = [tail_renderer(desc, w, h, tail) for tail in (None, 0)]
    st, pose = blend.state(sc, w, h), home("street")
    sc.updateCamera(w, h)
    for f in range(3):
        st.time = 1000 + f
        cam = camera(sc, pose, 0, w, h)
        o.set_camera(cam); o.render_frame(st, f)
        want = {b: o.readback(b) for b in frame_buffers(f)}
        for tail, r in zip(("on", "off"), rs):
            r.set_camera(cam); r.run(st, f)
            assert bad_buffers(r, want) == {}, (size, "tail", tail, "frame", f)
    for r in rs:
        r.destroy()


def test_two_lds_stack_entries_in_a_fresh_process():
    out = child("frames", RESTIR_STACK_LDS="2")
    print(out)
    assert out["problems"] == [] and out["frames"] == 6


# ---- e. dynamic geometry --------------------------------------------------------------------------------------------------------------------------------------------
def records_by_id(r):
    """{globalId: (flags, alphaIdx != 0, omm)} of a context's leaf records; the references of one triangle (spatial splits) must agree among themselves"""
    recs = r.accel_readback(abi.ACCEL_TRIS).view(refit.REC_DT)
    order = np.argsort(recs["globalId"], kind="stable")
    recs = recs[order]
    same = recs["globalId"][1:] == recs["globalId"][:-1]
    for k in ("flags", "alphaIdx"):
        assert (recs[k][1:][same] == recs[k][:-1][same]).all(), k
    assert (recs["omm"][1:][same] == recs["omm"][:-1][same]).all()
    first = np.concatenate([[True], ~same])
    return recs[first]


def assert_records_equal_a_fresh_build(r, desc, what, before):
    """flags and micro-maps by globalId equal those of a fresh context built from `desc`.  alphaIdx names a row of the context's alpha records, which a build
    numbers in the order of its own leaves: against the fresh context it is held up to that numbering (0, "no alpha test", is 0; distinct rows stay distinct),
    and exactly against what this context's records held before the call (`before`)"""
    from restir_amd.renderer import Renderer
    fresh = Renderer().setup(0)
    fresh.load_scene(desc)
    a, b = records_by_id(r), records_by_id(fresh)
    fresh.destroy()
    assert np.array_equal(a["globalId"], b["globalId"]) and np.array_equal(a["globalId"], before["globalId"]), what
    assert np.array_equal(a["flags"], b["flags"]), (what, int((a["flags"] != b["flags"]).sum()))
    assert np.array_equal(a["omm"], b["omm"]), (what, int((a["omm"] != b["omm"]).any(axis=1).sum()))
    assert np.array_equal(a["alphaIdx"], before["alphaIdx"]), (what, int((a["alphaIdx"] != before["alphaIdx"]).sum()))
    blended = (a["flags"] & 1) == 0
    assert blended.any() and np.array_equal(a["alphaIdx"] != 0, blended) and np.array_equal(b["alphaIdx"] != 0, blended), what
    pairs = np.unique(np.stack([a["alphaIdx"], b["alphaIdx"]], axis=1), axis=0)
    assert len(pairs) == len(np.unique(a["alphaIdx"])) == len(np.unique(b["alphaIdx"])), what
    return a


def test_refit_vertex_update_and_rebuild_keep_the_blended_records():
    sc = refit.street()
    desc = blend.veil(sc)
    pose = sc.cameraPose()
    st = blend.state(sc, W, H)
    r, o = renderer(desc, W, H), oracle(desc, W, H)
    sc.updateCamera(W, H)
    f = 0

    def two_frames(what):
        nonlocal f
        frames_equal(r, o, sc, st, pose, W, H, f, 2, what)
        f += 2

    two_frames("as built")
    recs = records_by_id(r)
    # a blended tree instance (shared mesh) and a mirrored blended prop turn about their own centres
    d = refit.describe(desc)
    blended = set(int(i) for i in blend.blended_instances(desc))
    tree = [int(i) for i in d["shared"] if int(i) in blended][-1]
    prop = [int(i) for i in d["mirrored"] if int(i) in blended][0]
    ids = [tree, prop]
    ext = float(max(np.abs(np.concatenate(refit.world_bounds(desc, i))).max() for i in range(desc.numInstances)))
    xf = np.stack([refit.move_matrix("rotate", desc, i, ext) for i in ids])
    r.update_instances(ids, xf)
    sc.updateInstances(np.asarray(ids, np.uint32), np.asarray(xf, np.float32))
    desc = blend.veil(sc)
    r.update_lights(desc); o.upload_scene(desc)
    two_frames("after rt_update_instances")
    recs = assert_records_equal_a_fresh_build(r, desc, "after rt_update_instances", recs)
    # the tree's mesh moves
    m = int(refit.instances_of(desc)["primMesh"][tree])
    first, count = skin.mesh_range(desc, m)
    rows = skin.vertices_of(desc)[first:first + count].copy()
    rows["position"] += np.float32(0.25)
    r.update_vertices(m, 0, rows)
    sc.updateVertices(m, 0, rows)
    desc = blend.veil(sc)
    o.upload_scene(desc)
    two_frames("after rt_update_vertices")
    recs = assert_records_equal_a_fresh_build(r, desc, "after rt_update_vertices", recs)
    r.rebuild_accel()
    two_frames("after rt_rebuild_accel")
    recs = assert_records_equal_a_fresh_build(r, desc, "after rt_rebuild_accel", recs)
    r.destroy()


# ---- f. the opacity micro-map against float64 -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["gltf", "street"])
def test_micro_map_states_are_sound_against_float64(name):
    """every cell of every non-opaque triangle's map, as the device holds it, against blend.micro_map_violations (tests/test_blend_cpu.py shows that the check
    rejects a wrong map)"""
    from restir_amd.renderer import Renderer
    sc, desc = scene(name)
    r = Renderer().setup(0); r.load_scene(desc)
    recs = records_by_id(r)
    r.destroy()
    bad, seen = blend.micro_map_violations(desc, recs[(recs["flags"] & 1) == 0])
    print(name, seen)
    assert bad == []
    assert seen[(blend.ALPHA_BLEND, 0)] > 0 and seen[(blend.ALPHA_BLEND, 2)] > 0


# ---- g. reference mode ------------------------------------------------------------------------------------------------------------------------------------------------
def test_reference_mode_on_veiled_cornell_equals_its_cpu_checker(tmp_path_factory):
    import refpt
    lib = refpt.build(tmp_path_factory.mktemp("refpt"))
    sc, desc = scene("cornell")
    w = h = 48
    st = blend.state(sc, w, h)
    from restir_amd.renderer import Renderer
    r = Renderer().setup(0); r.load_scene(desc); r.update(w, h)
    k = refpt.RefChecker(lib, desc); k.resize(w, h)
    cam = camera(sc, home("cornell"), 0, w, h)
    r.set_camera(cam); k.set_camera(cam)
    for max_depth, mis in ((1, 0), (4, 1)):
        s = abi.RtxState.from_buffer_copy(st)
        s.maxDepth, s.MIS = max_depth, mis
        for n in (1, 3, 4):
            r.reference_render(s, n)
        k.reset(); k.render(s, 8)
        assert r.reference_samples() == 8 and k.samples() == 8
        for c in range(3):
            g = r.reference_readback(c)
            assert optin.words(g, k.readback(c)) == 0, (max_depth, mis, c)
        assert np.isfinite(g).all() and g[..., :3].max() > 0
    r.destroy()


if __name__ == "__main__":
    # a fresh process for the cases whose environment variable is read once; one JSON line
    which = sys.argv[1]
    from restir_amd import build as _build
    _build.build_host(); _build.build_hip()
    from oracle import binding as _binding
    _binding.build()
    if which == "replay":      # the twelve frames of rest, move, rest
        problems, stats = run_sequence("base", offsets=OFFSETS, expect=LAUNCHES, scene=veiled_street_at_the_scene_pose)
        print(json.dumps({"problems": problems, "stats": stats}))
    else:                      # three frames of the veiled street with a moving camera on the throughput build, at two sizes
        sc, desc = scene("street")
        problems, done = [], 0
        for w, h in ((13, 11), (70, 50)):
            r, o = renderer(desc, w, h), oracle(desc, w, h)
            st, pose = blend.state(sc, w, h), home("street")
            sc.updateCamera(w, h)
            try:
                frames_equal(r, o, sc, st, pose, w, h, 0, 3, "moving", move=1)
                done += 3
            except AssertionError as e:
                problems.append(str(e))
            r.destroy()
        print(json.dumps({"problems": problems, "frames": done}))
