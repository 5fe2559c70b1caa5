"""Object motion vectors without a GPU: the three entry points exist, rt_object_motion_camera (a pure host function) does what include/rt_abi.h
states — bit identity for an unmoved instance, the projection and the depth of the per-instance camera against float64, the camera's own values for a singular
matrix —, and the composite driver of tests/objmotion.py is neutral when nothing is in motion."""
import ctypes as C
import os
import re
import numpy as np

from helpers import ROOT, abi, frame_buffers
from oracle.binding import Oracle
import objmotion
import optin
import refit

NAMES = ("rt_set_object_motion", "rt_object_motion_camera", "rt_object_motion_readback")
W, H = 64, 48


def lib():
    from restir_amd import renderer
    return renderer.hip_lib()


def scene_camera(frames=2):
    """a Cornell camera with a history: lastProjView / lastPosition are those of the previous pose"""
    sc = refit.cornell()
    eye, center, up, fov = sc.cameraPose()
    for f in range(frames):
        sc.setCamera((np.array(eye, np.float64) + 0.05 * f * np.array([1.0, 0.25, -0.75])).astype(np.float32), center, up, fov)
        sc.updateCamera(W, H)
    return sc, sc.getCamera()


def moves(sc):
    """(name, P, C) for the four transform classes on the taller Cornell box; the rotation is 0.2 rad about y"""
    desc = sc.desc()
    i = 3
    P = refit.instances_of(desc)["objectToWorld"][i].copy()
    lo, hi = refit.world_bounds(desc, i)
    out = [(k, P, refit.move_matrix(k, desc, i, 1.0)) for k in ("translate", "scale", "mirror")]
    out.insert(1, ("rotate", P, refit.compose(refit.rotation_y(0.2, 0.5 * (lo + hi)), P)))
    return out


def affine64(m):
    A = np.eye(4)
    A[:3] = np.asarray(m, np.float64).reshape(3, 4)
    return A


def mat64(m):
    return np.array(list(m.m), np.float64).reshape(4, 4).T   # column-major m[c * 4 + r]


def test_header_and_library_have_the_entry_points():
    src = open(os.path.join(ROOT, "include", "rt_abi.h")).read()
    assert re.search(r"\bint rt_object_motion_camera\(const rt_scene_camera\* cam, const float prevObjectToWorld\[12\], const float curObjectToWorld\[12\], rt_scene_camera\* out\);", src)
    assert re.search(r"\bint rt_set_object_motion\(rt_ctx\* ctx, int mode\);", src) and re.search(r"\bint rt_object_motion_readback\(rt_ctx\* ctx, void\* dst, size_t bytes\);", src)
    assert "RT_OBJECT_MOTION_OFF = 0" in src and "RT_OBJECT_MOTION_ON = 1" in src
    from restir_amd import renderer
    L = lib()
    for n in NAMES:
        assert hasattr(L, n) and n in renderer.ABI_SYMBOLS, n
    assert L.rt_abi_version() == (2 << 16) | 4
    cam = abi.SceneCamera()
    m = np.zeros(12, np.float32)
    assert L.rt_object_motion_camera(None, m.ctypes.data, m.ctypes.data, C.byref(cam)) == abi.ERR_INVALID_ARG
    assert L.rt_set_object_motion(None, 1) == abi.ERR_INVALID_ARG


def test_unmoved_instance_returns_the_camera_byte_for_byte():
    sc, cam = scene_camera()
    for _, P, Cm in moves(sc):
        for m in (P, Cm):
            assert bytes(objmotion.motion_camera(cam, m, m.copy())) == bytes(cam)


def test_only_the_two_history_fields_change():
    sc, cam = scene_camera()
    for name, P, Cm in moves(sc):
        out = objmotion.motion_camera(cam, P, Cm)
        raw, got = bytearray(bytes(cam)), bytearray(bytes(out))
        a, b = abi.SceneCamera.lastProjView.offset, abi.SceneCamera.lastPosition.offset
        assert raw[:a] == got[:a] and raw[b + 12:] == got[b + 12:], name
        assert raw[a:b + 12] != got[a:b + 12], name


def test_projection_against_float64():
    """project M x with lastProjView in float64 and x with lastProjView_i in float32 (the kernel's expression): the pixel indices may differ only where the
    float64 sub-pixel position lies within 1e-3 of a pixel edge"""
    sc, cam = scene_camera()
    rng = np.random.default_rng(5)
    L64 = mat64(cam.lastProjView)
    inv_view = mat64(cam.viewInverse)
    for name, P, Cm in moves(sc):
        out = objmotion.motion_camera(cam, P, Cm)
        Li = np.array(list(out.lastProjView.m), np.float32).reshape(4, 4).T
        M = affine64(P) @ np.linalg.inv(affine64(Cm))
        n = 0
        # 64 points in front of the camera: view-space points 1.5 .. 4 units down -z inside the frustum's middle
        for _ in range(64):
            v = np.array([rng.uniform(-0.4, 0.4), rng.uniform(-0.4, 0.4), -rng.uniform(1.5, 4.0), 1.0])
            x = (inv_view @ v).astype(np.float32)
            x[3] = 1.0
            p64 = L64 @ (M @ x.astype(np.float64))
            s64 = (p64[:2] / p64[3] * 0.5 + 0.5) * np.array([W, H], np.float64)
            # the kernel: ((m0 x + m4 y) + m8 z) + m12 w per row, /w, * 0.5 + 0.5, * size, truncation — all in float32
            p = ((Li[:, 0] * x[0] + Li[:, 1] * x[1]) + Li[:, 2] * x[2]) + Li[:, 3] * x[3]
            s = ((p[:2] / p[3]) * np.float32(0.5) + np.float32(0.5)) * np.array([W, H], np.float32)
            assert s.dtype == np.float32
            near_edge = np.abs(s64 - np.round(s64)) < 1e-3
            same = np.trunc(s).astype(np.int64) == np.trunc(s64).astype(np.int64)
            assert (same | near_edge).all(), (name, s, s64)
            n += int(same.all())
        assert n >= 60, (name, n)


def test_rigid_motion_keeps_the_depth():
    """|lastPosition_i - x| == |lastPosition - M x| for rigid motion, to a relative 1e-5: three float32 matrix products (inverse(P), · lastPosition, C ·) of a
    few terms each, every term rounded to 2^-24 relative to coordinates no larger than ~10 x the distance: 3 x 4 x 6e-8 x 10 = 7e-6 < 1e-5"""
    sc, cam = scene_camera()
    rng = np.random.default_rng(6)
    lp = np.array([cam.lastPosition.x, cam.lastPosition.y, cam.lastPosition.z], np.float64)
    for name, P, Cm in moves(sc)[:2]:   # the translation and the rotation
        out = objmotion.motion_camera(cam, P, Cm)
        lpi = np.array([out.lastPosition.x, out.lastPosition.y, out.lastPosition.z], np.float64)
        M = affine64(P) @ np.linalg.inv(affine64(Cm))
        for _ in range(64):
            x = np.append(rng.uniform(-1.0, 1.0, 3), 1.0)
            a, b = np.linalg.norm(lpi - x[:3]), np.linalg.norm(lp - (M @ x)[:3])
            assert abs(a - b) <= 1e-5 * b, (name, a, b)


def test_singular_matrix_returns_the_cameras_values():
    sc, cam = scene_camera()
    _, P, Cm = moves(sc)[0]
    flat = P.copy()
    flat[[0, 4, 8]] = 0.0    # a zero column: determinant 0
    nan = P.copy()
    nan[3] = np.nan
    for a, b in ((flat, Cm), (P, flat), (nan, Cm), (P, nan)):
        assert bytes(objmotion.motion_camera(cam, a, b)) == bytes(cam)


def test_composite_of_one_group_is_the_oracles_frame():
    """nothing in motion: the driver's save / restore / stage chain equals Oracle.render_frame word for word, and a scene re-upload in between changes nothing"""
    case = objmotion.Case("cornell", 32, 24, gpu=False, movers=[3])
    ref = Oracle(0)
    ref.upload_scene(case.desc)
    ref.resize(32, 24)
    for f in range(3):
        cam = case.frame(f)
        assert case.groups == []
        ref.set_camera(cam)
        ref.render_frame(case.st, f)
        assert {abi.BUFFER_NAMES[b]: optin.words(case.o.readback(b), ref.readback(b)) for b in frame_buffers(f) if optin.words(case.o.readback(b), ref.readback(b))} == {}, f


def test_composite_in_motion_differs_from_the_camera_only_frame_only_on_the_mover():
    """the composite with a translating box: every pixel outside the box (full resolution, by the pick image) equals the plain oracle frame of the moved scene"""
    Wc, Hc = 32, 24
    case = objmotion.Case("cornell", Wc, Hc, gpu=False, movers=[3])
    ref = Oracle(0)
    ref.upload_scene(case.desc)
    ref.resize(Wc, Hc)
    changed = 0
    for f, kind in enumerate((None, "translate", "translate")):
        cam = case.frame(f, kind)
        ref.upload_scene(case.desc)
        ref.set_camera(cam)
        ref.render_frame(case.st, f)
        assert len(case.groups) == (0 if kind is None else 1)
        off = case.inst != 3
        for b in (abi.BUF_MOTION, abi.BUF_GBUFFER0 + (f & 1), abi.BUF_DIRECT_RESV0 + (f & 1)):
            a, e = case.o.readback(b).reshape(Wc * Hc, -1), ref.readback(b).reshape(Wc * Hc, -1)
            assert (a[off] == e[off]).all(), (f, abi.BUFFER_NAMES[b])
            changed += int((a[~off] != e[~off]).sum())
    assert changed > 0    # ... and on the box the per-instance camera changed the motion vectors


def test_footprint_mask_of_the_spatial_modes():
    """one_group_footprint: a pixel counts when its clipped (2 r + 1)^2 neighbourhood lies in one group"""
    g = np.zeros((6, 7), np.int32)
    g[2:5, 3:6] = 1
    ok = objmotion.one_group_footprint(g, 1)
    want = np.ones((6, 7), bool)
    want[1:6, 2:7] = False      # the block and its one-pixel rim ...
    want[3, 4] = True           # ... but the block's centre sees the block alone
    assert (ok == want).all()
    far = objmotion.one_group_footprint(g, 2)
    assert far[:, 0].all() and far.sum() == 6    # at radius 2 only column 0 does not reach the block


def test_poses_of_the_spatial_mode_test_exclude_at_most_a_quarter_of_the_image():
    """the sequence of the GPU test of the spatial ReSTIRState modes on the oracle's own pick image: the pixels whose 3 x 3 footprint crosses a group boundary are at
    most 25 % of the image, and pixels of the mover remain to be compared"""
    Wc, Hc = 64, 48
    case = objmotion.Case("cornell", Wc, Hc, gpu=False, movers=[3], restir=abi.RESTIR_SPATIAL)
    case.st.denoise = 0
    for f, kind in enumerate((None, "translate", "rotate", None, "scale")):
        case.frame(f, kind)
        g = case.group_image()
        ok = objmotion.one_group_footprint(g, 1)
        assert 1.0 - ok.mean() <= 0.25, (f, 1.0 - ok.mean())
        assert kind is None or (ok & (g == 1)).sum() > 20, (f, kind)
