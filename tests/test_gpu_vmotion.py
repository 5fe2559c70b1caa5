"""Per-vertex motion vectors on the GPU (rt_set_object_motion mode OBJECT_MOTION_VERTEX).  Every frame of a sequence in which a mesh bends, stops,
bends while its instance moves, is posed twice before a frame and is rewritten from host rows: the delta image, the instance image and RT_BUF_MOTION equal
tests/vmotion_checker.cpp word for word, and every buffer of helpers.frame_buffers(f) equals the frame the UNMODIFIED oracle renders from the warped history
(tests/vmotion.py expected_frame) word for word.  No tolerance anywhere.  tests/test_vmotion_cpu.py proves the harness against the oracle's own frames."""
import ctypes as C
import numpy as np
import pytest

from helpers import abi, frame_buffers
import optin
import refit
import vmotion

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def tmp(tmp_path_factory):
    return tmp_path_factory.mktemp("vmotion_gpu")


def run(tmp, kind, W, H, frames=7, move=0.0, **kw):
    """the sequence of tests/vmotion.run_sequence; {frame: differing words per buffer}, and what the frames exercised"""
    k = vmotion.Case(tmp, kind, W, H, **kw)
    bad, flagged, moved_px, inexpressible = {}, [], 0, 0
    for f, _ in vmotion.run_sequence(k, frames, move):
        d = k.diff(f)
        if d:
            bad[f] = d
        flagged.append(bool(k.flagged[0].any() or k.flagged[1].any()))
        moved_px += int(np.abs(k.info["vm"]["d"]).max(axis=1).astype(bool).sum())
        inexpressible += k.info["inexpressible"]
    k.destroy()
    return bad, flagged, moved_px, inexpressible


FLAGGED = [False, True, True, False, True, True, True]      # frames 0 and 3 have nothing in motion or deformed


@pytest.mark.parametrize("W,H", [(16, 8), (33, 17)])
@pytest.mark.parametrize("traversal", [abi.TRAVERSAL_THROUGHPUT, abi.TRAVERSAL_LATENCY])
@pytest.mark.parametrize("overlap", [0, 1, 2, 3])
def test_cornell_sequence_equals_the_checker_and_the_warped_oracle(tmp, W, H, overlap, traversal):
    bad, flagged, moved_px, inexpressible = run(tmp, "cornell", W, H, overlap=overlap, traversal=traversal)
    assert flagged == FLAGGED and moved_px > 0 and inexpressible == 0      # (the poses keep the deforming mesh clear of columns 0-1)
    assert not bad, bad


@pytest.mark.parametrize("restir", [abi.RESTIR_TEMPORAL, abi.RESTIR_SPATIOTEMPORAL])
def test_street_sequence_skinned_instances_and_morphed_leaves(tmp, restir):
    bad, flagged, moved_px, inexpressible = run(tmp, "street", 64, 48, restir=restir)
    assert flagged == FLAGGED and moved_px > 10 and inexpressible == 0
    assert not bad, bad


def test_cornell_spatiotemporal(tmp):
    bad, flagged, moved_px, inexpressible = run(tmp, "cornell", 33, 17, restir=abi.RESTIR_SPATIOTEMPORAL)
    assert flagged == FLAGGED and moved_px > 0 and inexpressible == 0
    assert not bad, bad


def test_with_the_camera_step(tmp):
    bad, flagged, moved_px, inexpressible = run(tmp, "cornell", 33, 17, move=0.01)
    assert flagged == FLAGGED and moved_px > 0 and inexpressible <= 2 * 17
    assert not bad, bad


@pytest.mark.parametrize("which", ["svgf", "gi_spatial", "sky", "sky-throughput"])
def test_with_an_opt_in_pass_or_the_sky_build(tmp, which):
    kw = {}
    W, H, frames = 33, 17, 5
    if which == "svgf":
        den = abi.Denoiser()
        den.mode = abi.DENOISER_SVGF
        kw["den"] = den
    elif which == "gi_spatial":
        gis = abi.GiSpatial()
        gis.mode = abi.GI_SPATIAL_VISIBILITY
        kw["gis"] = gis
    else:
        kw["sky"] = abi.SunAndSky(in_use=1)
        if which == "sky-throughput":     # an image this small takes the build sky_lat_vm unless told otherwise: this case is the one that reaches sky_vm
            kw["traversal"] = abi.TRAVERSAL_THROUGHPUT
            W, H, frames = 16, 8, 2
    bad, flagged, moved_px, _ = run(tmp, "cornell", W, H, frames=frames, **kw)      # (with SVGF on, diff() compares the histories)
    assert flagged == FLAGGED[:frames] and moved_px > 0
    assert not bad, bad


def test_static_case_vertex_mode_with_nothing_moving_equals_mode_off(tmp):
    """no instance in motion, no mesh deformed: no table exists, every pixel takes the camera's values and the frame equals the mode-off frame word for word"""
    a = vmotion.Case(tmp, "cornell", 33, 17, mode=abi.OBJECT_MOTION_VERTEX)
    b = vmotion.Case(tmp, "cornell", 33, 17, mode=abi.OBJECT_MOTION_OFF)
    for f in range(4):
        for k in (a, b):
            k.st.time = 1000 + f
            k.r.set_camera(k.camera(f, 0.01))
            k.r.run(k.st, f)
        bad = {abi.BUFFER_NAMES[x]: optin.words(a.r.readback(x), b.r.readback(x)) for x in frame_buffers(f) if optin.words(a.r.readback(x), b.r.readback(x))}
        assert not bad, (f, bad)
        assert not a.r.vertex_motion_readback().any()
    a.destroy(); b.destroy()


def test_a_rigid_only_move_through_the_same_harness(tmp):
    k = vmotion.Case(tmp, "cornell", 33, 17)
    for f, kind in enumerate((None, "translate", "rotate", None, "scale")):
        if kind:
            k.move(kind)
        k.frame(f)
        assert k.flagged[1].any() == (kind is not None) and not k.flagged[0].any()
        assert k.diff(f) == {}, (f, k.diff(f))
        assert k.info["vm"]["d"].any() == (kind is not None)
    k.destroy()


def test_refusals_and_the_readback_rule(tmp):
    from restir_amd.renderer import hip_lib
    k = vmotion.Case(tmp, "cornell", 32, 24)
    r, L = k.r, hip_lib()
    buf = np.zeros((32 * 24, 4), np.float32)
    # before any frame with the mode on: RT_ERR_NO_TARGET; a wrong size: RT_ERR_INVALID_ARG; a mode beyond the enum: RT_ERR_INVALID_ARG
    assert L.rt_vertex_motion_readback(r._h, buf.ctypes.data, buf.nbytes) == abi.ERR_NO_TARGET
    assert all(L.rt_set_object_motion(r._h, m) == abi.ERR_INVALID_ARG for m in (2, 4, -1))      # (2 lies between the modes and is none)
    k.frame(0)
    assert L.rt_vertex_motion_readback(r._h, buf.ctypes.data, buf.nbytes - 16) == abi.ERR_INVALID_ARG
    assert L.rt_vertex_motion_readback(r._h, buf.ctypes.data, buf.nbytes) == 0
    # the counting build has no motion-vector form: refused while a mesh is deformed, and the message names the combination
    r.set_counting(True)
    k.bend(1.0)
    k.st.time = 1001
    r.set_camera(k.camera(1))
    assert L.rt_render_frame(r._h, C.byref(k.st), 1) == abi.ERR_INVALID_ARG
    msg = L.rt_last_error(r._h).decode()
    assert "rt_set_counting" in msg and "rt_set_object_motion" in msg and "deformed" in msg, msg
    # the refused frame rendered nothing: the mesh is still deformed for the frame that follows without counting
    r.set_counting(False)
    k.frame(1)
    assert k.flagged[0].any() and k.diff(1) == {}
    # a counting frame with nothing in motion runs the counting kernels
    r.set_counting(True)
    k.st.time = 1002
    r.set_camera(k.camera(2))
    assert L.rt_render_frame(r._h, C.byref(k.st), 2) == 0
    r.set_counting(False)
    k.destroy()


def test_state_survives_both_builds_and_is_cleared_by_resize_and_upload(tmp):
    from restir_amd.renderer import hip_lib
    L = hip_lib()
    # a bend, then rt_build_accel and rt_rebuild_accel, then the frame: the mesh is still deformed since the last rendered frame, with that frame's positions
    k = vmotion.Case(tmp, "cornell", 33, 17)
    k.frame(0)
    k.bend(1.0)
    assert refit.hip_build_accel(k.r) == 0
    k.r.rebuild_accel()
    k.move("translate")
    k.r.rebuild_accel()
    k.frame(1)
    assert k.flagged[0].any() and k.flagged[1].any() and k.info["vm"]["d"].any()
    assert k.diff(1) == {}, k.diff(1)
    # rt_resize clears the marks and the delta image: the bend before it is not "since the last frame" for the frame after it
    k.bend(1.5)
    k.r.update(33, 17)
    buf = np.zeros((33 * 17, 4), np.float32)
    assert L.rt_vertex_motion_readback(k.r._h, buf.ctypes.data, buf.nbytes) == abi.ERR_NO_TARGET
    k.st.time = 1002
    k.r.set_camera(k.camera(2))
    k.r.run(k.st, 2)
    assert not k.r.vertex_motion_readback().any()
    # rt_upload_scene clears them too (and the skins: the rows come from rt_update_vertices here)
    k.rows(1.0)
    k.r.load_scene(k.desc())
    k.st.time = 1003
    k.r.set_camera(k.camera(3))
    k.r.run(k.st, 3)
    assert not k.r.vertex_motion_readback().any()
    # ... and the plane of the new scene works: rows after the upload are seen by the next frame
    first, count = vmotion.skin.mesh_range(k.sc.desc(), k.rows_mesh)
    rows = k.verts[first:first + count].copy()
    rows["position"][:, 0] += np.float32(0.02)
    k.r.update_vertices(k.rows_mesh, 0, rows)
    k.st.time = 1004
    k.r.set_camera(k.camera(4))
    k.r.run(k.st, 4)
    d = k.r.vertex_motion_readback()
    inst = k.r.object_motion_readback()
    on_box = inst == 3
    assert on_box.any() and d[on_box][:, :3].any(axis=1).all() and not d[~on_box].any()
    assert np.abs(d[on_box][:, 0] + 0.02).max() < 1e-4      # x_prev - x of a mesh shifted by +0.02 along x
    k.destroy()
