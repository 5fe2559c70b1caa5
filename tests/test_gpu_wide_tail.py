"""The wide tail of the throughput traversal (csrc/traverse.h wideTail): when a ray pool of the indirect stage is dry and at most DevScene::wideTail
rays of the wave are live, they move to eight lanes per ray and finish there.  That may change how many steps are counted, never a word of any buffer: every case
compares every buffer of helpers.frame_buffers with the oracle, with the tail on (the default) and off (RESTIR_WIDE_TAIL=0, read at every acceleration-structure
build), over three frames from a cold history (the seed plane of the primary rays, which has no readback, goes cold -> warm beside it).

Sizes: 8 x 8 is one tile (its 4 x 4 half resolution leaves 48 lanes of the indirect stage's wave without a pixel: they serve the pool and the tail); 24 x 16 six
tiles; 13 x 11 and 8 x 5 have ragged tiles at their right / bottom edges at both resolutions: lanes without a pixel, in a wave that is still whole.  (The
indirect stage's pools always run with all 64 lanes of their block, so the partial-wave guard of the tail is never false here: no case covers its other branch.)
Images this small would take the latency build under RT_TRAVERSAL_AUTO, so the tests name the throughput build."""
import os
import subprocess
import sys

import numpy as np
import pytest

from helpers import abi, host, make_scene, frame_buffers
from oracle.binding import Oracle
import optin

pytestmark = pytest.mark.gpu

SCENES = {
    "cornell": (abi.PROC_CORNELL, 1.0, None),
    "bistro-ext-real": (abi.PROC_BISTRO_EXT_REAL, 0.02, (64, 32)),   # alpha cards (the texture path of travTriW), mirrored instances
    "sponza": (abi.PROC_SPONZA, 0.03, None),
}
SIZES = [(8, 8), (24, 16), (13, 11), (8, 5)]
FRAMES = 3
EQUAL_COUNTERS = ("closestHitRays", "anyHitRays", "hitsShaded", "risCandidates")

_scenes, _refs = {}, {}


def scene(name):
    if name not in _scenes:
        kind, scale, env_size = SCENES[name]
        sc, env = make_scene(kind, scale, 1, env_size)
        _scenes[name] = (sc, env, sc.desc(env))
    return _scenes[name]


def state(sc, env, W, H):
    st = host.default_state(W, H, sc, env)
    if env is None:
        st.environmentProb = 0.0; st.fireflyClampThreshold = 100.0
    return st


def reference(name, W, H):
    """the oracle's three frames of one (scene, size): [(camera, {buffer: words})], rendered once and shared"""
    if (name, W, H) not in _refs:
        sc, env, desc = scene(name)
        st = state(sc, env, W, H)
        o = Oracle(0); o.upload_scene(desc); o.resize(W, H)
        sc.updateCamera(W, H)
        frames = []
        for f in range(FRAMES):
            st.time = 1000 + f
            sc.updateCamera(W, H)
            cam = sc.getCamera()
            cam = type(cam).from_buffer_copy(cam)
            o.set_camera(cam); o.render_frame(st, f)
            frames.append((cam, {b: o.readback(b).copy() for b in frame_buffers(f)}))
        _refs[(name, W, H)] = frames
    return _refs[(name, W, H)]


def renderer(desc, W, H, tail, overlap=0):
    """a throughput-build context whose acceleration structure was built with the tail on (None: the library's default) or off"""
    from restir_amd.renderer import Renderer
    old = os.environ.pop("RESTIR_WIDE_TAIL", None)
    if tail is not None:
        os.environ["RESTIR_WIDE_TAIL"] = str(tail)
    try:
        r = Renderer().setup(0)
        r.set_overlap(overlap)
        r.load_scene(desc)
    finally:
        os.environ.pop("RESTIR_WIDE_TAIL", None)
        if old is not None:
            os.environ["RESTIR_WIDE_TAIL"] = old
    r.update(W, H)
    r.set_traversal(abi.TRAVERSAL_THROUGHPUT)
    return r


def bad_buffers(r, want):
    bad = {abi.BUFFER_NAMES[b]: optin.words(r.readback(b), w) for b, w in want.items()}
    return {k: v for k, v in bad.items() if v}


def frames_equal_the_oracle(name, W, H, overlap):
    sc, env, desc = scene(name)
    frames = reference(name, W, H)
    st = state(sc, env, W, H)
    for tail in (None, 0):
        r = renderer(desc, W, H, tail, overlap)
        for f, (cam, want) in enumerate(frames):
            st.time = 1000 + f
            r.set_camera(cam)
            r.run(st, f)
            assert bad_buffers(r, want) == {}, (name, W, H, overlap, "tail", tail, "frame", f)
        r.destroy()
    return frames


@pytest.mark.parametrize("overlap", [0, 2], ids=["serial", "frames-in-flight"])
@pytest.mark.parametrize("W,H", SIZES, ids=["%dx%d" % s for s in SIZES])
@pytest.mark.parametrize("name", list(SCENES))
def test_three_frames_equal_the_oracle_with_the_tail_on_and_off(name, W, H, overlap):
    frames = frames_equal_the_oracle(name, W, H, overlap)
    img = frames[-1][1][abi.BUF_DIRECT_RESULT0 + ((FRAMES - 1) & 1)].view(np.float32)
    assert np.isfinite(img).all() and img.max() > 0.01       # not comparing empty frames


@pytest.mark.parametrize("name", list(SCENES))
def test_the_tail_runs_and_changes_no_ray(name):
    """counting build, 24 x 16, three frames with the tail on and off: the same rays, shaded hits and RIS candidates; fewer lane-rounds with the tail (a lane-round is
    one lane sitting through one scheduling round of its wave, and the tail's triangle rounds serve up to eight pending triangles of a ray) — which proves the path
    runs.  Node and triangle steps are NOT compared: an any-hit ray tests up to eight triangles in the step that finds its hit."""
    W, H = 24, 16
    sc, env, desc = scene(name)
    frames = reference(name, W, H)
    st = state(sc, env, W, H)
    got = {}
    for tail in (None, 0):
        r = renderer(desc, W, H, tail)
        r.set_counting(True)
        for f, (cam, want) in enumerate(frames):
            st.time = 1000 + f
            r.set_camera(cam)
            r.run(st, f)
            assert bad_buffers(r, want) == {}, (name, "counting", "tail", tail, "frame", f)
        c = r.counters()
        got[tail] = {k: getattr(c, k) for k in EQUAL_COUNTERS + ("nodesVisited", "trisTested", "laneRounds", "laneLiveRounds")}
        r.destroy()
    print(name, "tail on", got[None], "off", got[0])
    for k in EQUAL_COUNTERS:
        assert got[None][k] == got[0][k], k
    assert got[None]["closestHitRays"] >= FRAMES * W * H
    assert got[None]["laneRounds"] < got[0]["laneRounds"]


def test_stage_bands_whose_rows_are_no_multiple_of_eight():
    """24 x 21: a full frame, then the next frame's direct stage as the row bands [0, 8) and [8, 21) — 13 rows (a band starts on the tile grid), the last tile row
    with 5 of its 8 pixel rows — and the whole indirect stage, whose pools end in the tail, on the G-buffer the bands left"""
    name, W, H = "bistro-ext-real", 24, 21
    sc, env, desc = scene(name)
    st = state(sc, env, W, H)
    r = renderer(desc, W, H, None)
    o = Oracle(0); o.upload_scene(desc); o.resize(W, H)
    sc.updateCamera(W, H)
    for f in range(2):
        st.time = 1000 + f
        sc.updateCamera(W, H)
        cam = sc.getCamera()
        r.set_camera(cam); o.set_camera(cam)
        if f == 0:
            r.run(st, f); o.render_frame(st, f)
            bufs = frame_buffers(f)
        else:
            for y0, y1 in ((0, 8), (8, H)):
                r.run_stage(st, f, abi.STAGE_DIRECT, 0, y0, y1)
            r.run_stage(st, f, abi.STAGE_INDIRECT)
            o.run_stage(st, f, abi.STAGE_DIRECT); o.run_stage(st, f, abi.STAGE_INDIRECT)
            bufs = frame_buffers(f, indirect=False) + [abi.BUF_INDIRECT_RESV0 + (f & 1), abi.BUF_DENOISE_IND_A]
        assert bad_buffers(r, {b: o.readback(b) for b in bufs}) == {}, f
    r.destroy()


def test_two_lds_stack_entries_so_that_the_tail_reaches_the_overflow_slots():
    """RESTIR_STACK_LDS=2, the smallest the library accepts: all but two entries of a ray's stack are in the owner thread's overflow slots in HBM, which the eight lanes
    of a group read and lane 0 writes.  The library reads that switch once per process, hence a child process (this file as a script)."""
    env = dict(os.environ)
    env["RESTIR_STACK_LDS"] = "2"
    env.pop("RESTIR_WIDE_TAIL", None)
    out = subprocess.run([sys.executable, os.path.abspath(__file__)], env=env, cwd=os.path.dirname(os.path.abspath(__file__)), capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "stack-lds cases equal" in out.stdout, out.stdout[-2000:] + out.stderr[-2000:]


if __name__ == "__main__":
    for scene_name in ("bistro-ext-real", "sponza"):
        frames_equal_the_oracle(scene_name, 24, 16, 0)
    print("stack-lds cases equal")
