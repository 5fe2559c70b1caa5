"""Object motion vectors on the GPU (rt_set_object_motion): with the mode on, every frame buffer equals the oracle's composite of one run per
per-instance camera (tests/objmotion.py) word for word — static scenes, instances in motion under translate / rotate / scale / a frame without an update /
mirror, in the overlap modes and both traversal builds, with SVGF and with GI spatial reuse on; in the spatial ReSTIRState modes every pixel whose reuse footprint
lies in one group —, the instance image equals the oracle's pick image off the silhouettes, the motion state follows the
rules of include/rt_abi.h, and a translating box keeps its direct history, which it loses with the mode off; its stored motion vectors are the float64 projection of the previous world position."""
import ctypes as C
import numpy as np
import pytest

from helpers import abi
import objmotion
import refit

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def tmp(tmp_path_factory):
    return tmp_path_factory.mktemp("objmotion")


def sky():
    return abi.SunAndSky(in_use=1)


def test_static_scene_equals_the_oracle_and_the_instance_image_the_pick_image():
    case = objmotion.Case("cornell", 48, 40, overlap=2, movers=[])
    for f in range(4):
        cam = case.frame(f)
        assert case.groups == []
        assert case.diff(f) == {}, f
        share = objmotion.check_instance_image(case.inst, objmotion.pick_image(case.o, cam, 48, 40))
        print("frame %d: instance image off the pick image at %.2f %% of the pixels (silhouettes)" % (f, 100 * share))
    case.destroy()


# (scene, W, H, overlap, traversal, ReSTIRState, sky, opt-in pass): 64 x 48 of both scenes, the ragged 37 x 29 (odd width and height, a partial tile in both axes, the half-resolution
# grid drops a column and a row), 16 x 8 (a single tile row, which the latency build handles); ReSTIRState none and temporal; overlap 0, 2 and 3; both traversal builds;
# SVGF on (its checker receives the composite motion buffer) and GI spatial reuse on (its checker the composite G-buffer, reservoirs and IND_A)
CASES = [("cornell", 64, 48, 0, abi.TRAVERSAL_THROUGHPUT, abi.RESTIR_TEMPORAL, False, None),
         ("street", 64, 48, 2, None, abi.RESTIR_TEMPORAL, False, None),
         ("cornell", 37, 29, 3, abi.TRAVERSAL_LATENCY, abi.RESTIR_TEMPORAL, False, None),
         ("cornell", 16, 8, 0, None, abi.RESTIR_NONE, False, None),
         ("cornell", 64, 48, 2, abi.TRAVERSAL_THROUGHPUT, abi.RESTIR_TEMPORAL, True, None),
         ("street", 37, 29, 0, abi.TRAVERSAL_LATENCY, abi.RESTIR_NONE, True, None),
         ("cornell", 64, 48, 2, None, abi.RESTIR_TEMPORAL, False, "svgf"),
         ("cornell", 37, 29, 0, None, abi.RESTIR_TEMPORAL, False, "gi_spatial")]


@pytest.mark.parametrize("kind,W,H,overlap,traversal,restir,with_sky,opt", CASES)
def test_frames_in_motion_equal_the_composite(tmp, kind, W, H, overlap, traversal, restir, with_sky, opt):
    den = abi.Denoiser(mode=abi.DENOISER_SVGF) if opt == "svgf" else None
    gis = abi.GiSpatial(mode=abi.GI_SPATIAL_VISIBILITY, samples=6, radius=6) if opt == "gi_spatial" else None
    case = objmotion.Case(kind, W, H, overlap=overlap, traversal=traversal, restir=restir, sky=sky() if with_sky else None, den=den, gis=gis, tmp=tmp)
    assert 1 <= len(case.movers) <= 3
    moved_pixels = taps = 0
    for f, k in enumerate((None,) + objmotion.SEQUENCE):
        cam = case.frame(f, k)
        # an update puts the movers in motion for exactly one frame: the frame without an update runs with no group
        assert len(case.groups) == (len(case.movers) if k is not None else 0), (f, k)
        assert case.diff(f) == {}, (f, k)
        objmotion.check_instance_image(case.inst, objmotion.pick_image(case.o, cam, W, H))
        moved_pixels += int(np.isin(case.inst, case.movers).sum()) if k is not None else 0
        if gis is not None:
            taps += int(case.gis_taps.sum())
    case.destroy()
    assert moved_pixels > 0    # the movers were in view: the composite was not group 0 alone
    assert gis is None or taps > 0


# k_direct_spatial (csrc/stages.hip): a pixel merges the cached reservoirs of two rounds of five neighbours q = round(p + d), d in the unit disk, so |q - p| <= 1
# in both axes: its footprint is its 3 x 3 neighbourhood (the kernel stages exactly the 10 x 10 block around its 8 x 8 tile).  The oracle runs both phases of the
# direct stage in one call, so the composite's direct result is the frame's only where that whole neighbourhood lies in one group; everything the first phase
# writes (G-buffer, motion, both reservoirs, the cached reservoir, the light id) and the indirect reservoir are per-pixel and compared everywhere.  denoise = 0
# keeps the filters from spreading the excluded pixels.
@pytest.mark.parametrize("restir,traversal,overlap", [(abi.RESTIR_SPATIAL, abi.TRAVERSAL_THROUGHPUT, 0), (abi.RESTIR_SPATIOTEMPORAL, abi.TRAVERSAL_LATENCY, 2)])
def test_spatial_modes_equal_the_composite_where_the_footprint_lies_in_one_group(restir, traversal, overlap):
    W, H = 64, 48
    case = objmotion.Case("cornell", W, H, overlap=overlap, traversal=traversal, restir=restir, movers=[3])
    case.st.denoise = 0
    compared = 0
    for f, k in enumerate((None, "translate", "rotate", None, "scale")):
        cam = case.frame(f, k)
        cur = f & 1
        objmotion.check_instance_image(case.inst, objmotion.pick_image(case.o, cam, W, H))
        for b in (abi.BUF_GBUFFER0 + cur, abi.BUF_MOTION, abi.BUF_DIRECT_RESV0 + cur, abi.BUF_LIGHT_ID0 + cur, abi.BUF_DIRECT_RESV_TEMP, abi.BUF_INDIRECT_RESV0 + cur):
            assert objmotion.optin.words(case.r.readback(b), case.o.readback(b)) == 0, (f, k, abi.BUFFER_NAMES[b])
        g = case.group_image()
        ok = objmotion.one_group_footprint(g, 1)
        assert 1.0 - ok.mean() <= 0.25, (f, 1.0 - ok.mean())
        # every pixel of group 0 with no pixel of the mover within two pixels is among the compared ones
        far = objmotion.one_group_footprint(g, 2) & (g == 0)
        assert not (far & ~ok).any() and far.sum() > W * H // 2
        a = case.r.readback(abi.BUF_DIRECT_RESULT0 + cur).view(np.uint32).reshape(H, W, -1)
        e = case.o.readback(abi.BUF_DIRECT_RESULT0 + cur).view(np.uint32).reshape(H, W, -1)
        bad = (a != e).any(axis=2)
        assert not (bad & ok).any(), (f, k, np.argwhere(bad & ok)[:4].tolist())
        if k is not None:
            assert (g == 1).any()
            compared += int((ok & (g == 1)).sum())
    case.destroy()
    assert compared > 0    # pixels of the mover in motion were compared, not group 0 alone


def test_two_updates_between_two_frames_keep_the_rendered_frames_matrix():
    case = objmotion.Case("cornell", 64, 48, overlap=2, movers=[3])
    case.frame(0)
    desc0 = case.desc
    P = refit.instances_of(desc0)["objectToWorld"][3].copy()
    case.update([3], np.stack([refit.move_matrix("translate", case.desc, 3, case.extent)]))
    case.update([3], np.stack([refit.move_matrix("rotate", case.desc, 3, case.extent)]))
    case.frame(1)
    assert len(case.groups) == 1 and case.groups[0][1].tobytes() == P.tobytes()
    assert case.diff(1) == {}
    # there and back again before the next frame: not in motion
    here = refit.instances_of(case.desc)["objectToWorld"][3].copy()
    case.update([3], np.stack([refit.move_matrix("scale", case.desc, 3, case.extent)]))
    case.update([3], np.stack([here]))
    case.frame(2)
    assert case.groups == [] and case.diff(2) == {}
    case.destroy()


def test_rebuild_accel_between_two_frames_with_motion():
    case = objmotion.Case("cornell", 64, 48, overlap=2, movers=[3, 4])
    case.frame(0)
    case.frame(1, "translate")
    assert case.diff(1) == {}
    case.update(case.movers, np.stack([refit.move_matrix("rotate", case.desc, i, case.extent) for i in case.movers]))
    case.r.rebuild_accel()      # after the update, before the frame: the motion state survives
    case.frame(2)
    assert len(case.groups) == 2 and case.diff(2) == {}
    case.r.rebuild_accel()
    case.frame(3, "scale")
    assert len(case.groups) == 2 and case.diff(3) == {}
    case.destroy()


def _box_sequence(mode, frames=5, W=64, H=48):
    """Cornell, static camera, temporal reuse, box 3 translating parallel to the image plane by about two pixels per frame.  Returns per frame the direct
    reservoirs' `num`, the motion buffer, (mode on) the instance image and the box's objectToWorld; and the camera and the last frame's primary hits (rt_pick)"""
    from restir_amd.renderer import Renderer
    sc = refit.cornell()
    st = objmotion.host.default_state(W, H, sc, None)
    st.environmentProb = 0.0
    st.ReSTIRState = abi.RESTIR_TEMPORAL
    desc = sc.desc()
    r = Renderer().setup(0)
    r.set_overlap(0)
    r.load_scene(desc)
    r.update(W, H)
    r.set_object_motion(mode)
    sc.updateCamera(W, H)
    sc.updateCamera(W, H)
    cam = sc.getCamera()    # a camera at rest: lastProjView == projView
    # the camera's right vector, and the world length of two pixels at the box's depth (float64; aiming only)
    VI = np.array(list(cam.viewInverse.m), np.float64).reshape(4, 4).T
    PV = np.array(list(cam.projView.m), np.float64).reshape(4, 4).T
    lo, hi = refit.world_bounds(desc, 3)
    c = np.append(0.5 * (lo + hi), 1.0)
    right = VI[:3, 0]
    ndc = lambda p: (PV @ p)[0] / (PV @ p)[3]   # noqa: E731
    step = right * (2.0 * (2.0 / W) / (ndc(c + np.append(right, 0.0)) - ndc(c)))
    out = []
    home = refit.instances_of(desc)["objectToWorld"][3].copy()
    for f in range(frames):
        if f:
            xf = refit.compose(refit.translation(step * f), home)
            sc.updateInstances(np.array([3], np.uint32), xf.reshape(1, 12))
            r.update_instances([3], xf.reshape(1, 12))
        st.time = 1000 + f
        r.set_camera(cam)
        r.run(st, f)
        resv = r.readback(abi.BUF_DIRECT_RESV0 + (f & 1)).view(np.uint32).reshape(H, W, 9)
        mv = r.readback(abi.BUF_MOTION).view(np.int16).reshape(H, W, 2)
        out.append((resv[..., 7].copy(), mv.copy(), r.object_motion_readback().reshape(H, W) if mode else None, refit.instances_of(sc.desc())["objectToWorld"][3].copy()))
    hits = None
    if mode:   # the last frame's primary hits in world space: origin + hitT * direction of the ray through the pixel centre
        hits = np.full((H, W, 3), np.nan)
        for y in range(H):
            for x in range(W):
                p = r.pick(cam.viewInverse, cam.projInverse, (x + 0.5) / W, (y + 0.5) / H)
                if p.instanceID == 3:
                    hits[y, x] = np.array(p.worldRayOrigin[:3], np.float64) + np.float64(p.hitT) * np.array(p.worldRayDirection[:3], np.float64)
    r.destroy()
    return out, st.RISSampleNum, cam, hits


@pytest.fixture(scope="module")
def box():
    """the sequence with the mode on and off, and its interior pixels at frame 4: the instance image holds the box in this frame and at the reprojected position
    in the previous frame"""
    on, M, cam, hits = _box_sequence(abi.OBJECT_MOTION_ON)
    off = _box_sequence(abi.OBJECT_MOTION_OFF)[0]
    mv, inst, prev = on[4][1], on[4][2], on[3][2]
    H, W = inst.shape
    ys, xs = np.nonzero(inst == 3)
    qx, qy = mv[ys, xs, 0].astype(int), mv[ys, xs, 1].astype(int)
    ok = (qx >= 0) & (qx < W) & (qy >= 0) & (qy < H)
    ok[ok] &= prev[qy[ok], qx[ok]] == 3
    return dict(on=on, off=off, M=M, cam=cam, hits=hits, ys=ys[ok], xs=xs[ok])


def test_a_translating_box_keeps_its_direct_history_only_with_the_mode_on(box):
    ys, xs, M = box["ys"], box["xs"], box["M"]
    assert ys.size > 50, ys.size
    share_on = float((box["on"][4][0][ys, xs] > M).mean())
    share_off = float((box["off"][4][0][ys, xs] > M).mean())
    print("interior pixels %d: direct reservoirs with history (num > RISSampleNum = %d): mode on %.3f, mode off %.3f" % (ys.size, M, share_on, share_off))
    assert share_on > 0.5 and share_on > share_off


def test_the_stored_motion_vector_is_the_float64_projection_of_the_previous_world_position(box):
    """on the interior pixels: the hit point x (rt_pick's ray through the pixel centre), where that material point was one frame earlier, P · inverse(C) · x in
    float64, projected with the camera's lastProjView in float64; the stored index (a truncation, so its centre is compared) lies within one pixel of it"""
    ys, xs, cam, hits = box["ys"], box["xs"], box["cam"], box["hits"]
    mv = box["on"][4][1]
    H, W = mv.shape[:2]
    P, Cm = (np.vstack([box["on"][f][3].astype(np.float64).reshape(3, 4), [0, 0, 0, 1]]) for f in (3, 4))
    L = np.array(list(cam.lastProjView.m), np.float64).reshape(4, 4).T   # column-major m[c * 4 + r]
    x = hits[ys, xs]
    keep = np.isfinite(x).all(axis=1)    # (rt_pick's ray and raySpawn's may differ in the last bit on a silhouette)
    assert keep.sum() > 50 and keep.mean() > 0.9, (keep.sum(), keep.mean())
    x, ys, xs = np.concatenate([x[keep], np.ones((int(keep.sum()), 1))], axis=1), ys[keep], xs[keep]
    prev = (P @ np.linalg.inv(Cm) @ x.T).T
    p = (L @ prev.T).T
    s = (p[:, :2] / p[:, 3:4] * 0.5 + 0.5) * np.array([W, H], np.float64)
    err = np.abs(mv[ys, xs].astype(np.float64) + 0.5 - s)
    # the box moves: the previous position is about two pixels from the pixel itself, so the camera-only vector would miss this bound
    away = np.abs(s - np.stack([xs, ys], axis=1) - 0.5).max(axis=1)
    print("interior pixels %d: stored motion vector off the float64 projection by at most %.3f px; the projection is %.2f .. %.2f px from the pixel" %
          (ys.size, err.max(), away.min(), away.max()))
    assert away.min() > 1.0
    assert err.max() <= 1.0, err.max()


def test_refusals_and_the_readback_rule():
    from restir_amd.renderer import Renderer, RtError, hip_lib
    case = objmotion.Case("cornell", 32, 24, overlap=0, movers=[3])
    r, L = case.r, hip_lib()
    buf = np.zeros(32 * 24, np.uint32)
    # before any frame with the mode on: RT_ERR_NO_TARGET; a wrong size: RT_ERR_INVALID_ARG
    assert L.rt_object_motion_readback(r._h, buf.ctypes.data, buf.nbytes) == abi.ERR_NO_TARGET
    assert L.rt_set_object_motion(r._h, 2) == abi.ERR_INVALID_ARG
    case.frame(0)
    assert L.rt_object_motion_readback(r._h, buf.ctypes.data, buf.nbytes - 4) == abi.ERR_INVALID_ARG
    assert L.rt_object_motion_readback(r._h, buf.ctypes.data, buf.nbytes) == 0
    # the counting build has no object-motion form: refused while an instance is in motion, and the message names the combination
    r.set_counting(True)
    case.update([3], np.stack([refit.move_matrix("translate", case.desc, 3, case.extent)]))
    r.set_camera(case.camera(1))
    assert L.rt_render_frame(r._h, C.byref(case.st), 1) == abi.ERR_INVALID_ARG
    msg = L.rt_last_error(r._h).decode()
    assert "rt_set_counting" in msg and "rt_set_object_motion" in msg and "motion" in msg, msg
    # the refused frame rendered nothing: the instance is still in motion for the frame that follows without counting
    r.set_counting(False)
    case.frame(1)
    assert len(case.groups) == 1 and case.diff(1) == {}
    # rt_resize clears the motion state and the image
    case.update([3], np.stack([refit.move_matrix("rotate", case.desc, 3, case.extent)]))
    r.update(32, 24)
    assert L.rt_object_motion_readback(r._h, buf.ctypes.data, buf.nbytes) == abi.ERR_NO_TARGET
    case.destroy()
