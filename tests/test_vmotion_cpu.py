"""Per-vertex motion vectors without a GPU: the harness of tests/vmotion.py against the unmodified oracle's own frames, the CPU restatement of the
new arithmetic (tests/vmotion_checker.cpp) against float64 numpy, its static properties, and the checker under the sanitizers in a program of its own.
tests/test_gpu_vmotion.py holds the HIP kernels to the checker and to the warped-history frames word for word."""
import ctypes as C
import os
import subprocess
import numpy as np
import pytest

from helpers import ROOT, abi, frame_buffers
from oracle.binding import Oracle
import optin
import refit
import vmotion


@pytest.fixture(scope="module")
def tmp(tmp_path_factory):
    return tmp_path_factory.mktemp("vmotion")


def test_the_abi_names_the_mode_and_the_readback():
    from restir_amd import renderer
    assert abi.OBJECT_MOTION_VERTEX == 3 and "rt_vertex_motion_readback" in renderer.ABI_SYMBOLS
    text = open(os.path.join(ROOT, "include", "rt_abi.h")).read()
    assert "RT_OBJECT_MOTION_VERTEX = 3" in text and "int rt_vertex_motion_readback(rt_ctx* ctx, void* dst, size_t bytes);" in text


# ---- 1. the harness: with nothing deformed the warped history reproduces the oracle's own frames --------------------------------------------------------------
@pytest.mark.parametrize("restir", [abi.RESTIR_TEMPORAL, abi.RESTIR_SPATIOTEMPORAL])
@pytest.mark.parametrize("kind,W,H", [("cornell", 16, 8), ("cornell", 33, 17), ("street", 64, 48)])
def test_expected_frame_reproduces_the_oracle_with_nothing_deformed(tmp, kind, W, H, restir):
    """m_v = m_o (the checker's motion index of an unmoved point IS the oracle's), depths recomputed by the checker, camera step 0.01: every buffer of frames 0-4 equals
    o.render_frame word for word — which proves the gather and the numpy accept decision"""
    k = vmotion.Case(tmp, kind, W, H, gpu=False, restir=restir)
    ref = Oracle(0)
    ref.upload_scene(k.desc())
    ref.resize(W, H)
    for f in range(5):
        cam = k.frame(f, k.camera(f, 0.01))
        ref.set_camera(cam)
        ref.render_frame(k.st, f)
        info = k.info
        assert np.array_equal(info["vm"]["m16"][info["hit"]].astype(np.int32), info["m_o"][info["hit"]]) and not info["vm"]["d"].any()
        assert info["inexpressible"] == 0
        bad = {abi.BUFFER_NAMES[b]: optin.words(k.o.readback(b), ref.readback(b)) for b in frame_buffers(f) if optin.words(k.o.readback(b), ref.readback(b))}
        assert not bad, (f, bad)


@pytest.mark.parametrize("kind,W,H", [("cornell", 64, 48), ("cornell", 33, 17), ("cornell", 16, 8), ("street", 64, 48), ("street", 33, 17), ("street", 16, 8)])
def test_static_camera_motion_index_is_the_pixel_and_a_small_step_stays_injective(tmp, kind, W, H):
    k = vmotion.Case(tmp, kind, W, H, gpu=False)
    n = W * H
    own = np.stack([np.arange(n) % W, np.arange(n) // W], axis=1)
    for f in range(4):
        k.frame(f, k.camera(f, 0.0))
        if f >= 1:
            assert np.array_equal(k.info["m_o"][k.info["hit"]], own[k.info["hit"]]), f
    k2 = vmotion.Case(tmp, kind, W, H, gpu=False)
    for f in range(4):
        k2.frame(f, k2.camera(f, 0.01))      # (expected_frame asserts the injectivity)


# ---- 2. the checker against float64 ---------------------------------------------------------------------------------------------------------------------------------
def float64_xprev(desc, verts, prev, hits):
    """P * interp(q) in float64 and the bound's sum of |P| |q| per component, for the hit pixels"""
    pos, md, o2w, im = prev
    pm, inst, idx = refit.prim_meshes_of(desc), refit.instances_of(desc), np.frombuffer((C.c_uint32 * desc.numIndices).from_address(desc.indices), np.uint32)
    out, mag, flagged = [], [], []
    for h in hits:
        i, mesh = int(h["inst"]), int(inst["primMesh"][int(h["inst"])])
        tri = idx[int(pm["firstIndex"][mesh]) + 3 * int(h["prim"]):][:3].astype(np.int64) + int(pm["vertexOffset"][mesh])
        q = (pos if md[mesh] else verts["position"])[tri].astype(np.float64)
        u, v = np.float64(h["u"]), np.float64(h["v"])
        b = np.array([1.0 - u - v, u, v])
        P = (o2w[i] if im[i] else inst["objectToWorld"][i].reshape(12)).astype(np.float64).reshape(3, 4)
        out.append(P[:, :3] @ (b @ q) + P[:, 3])
        mag.append(np.abs(P[:, :3]) @ (np.abs(b) @ np.abs(q)) + np.abs(P[:, 3]))
        flagged.append(bool(md[mesh] or im[i]))
    return np.array(out), np.array(mag), np.array(flagged)


CASES = {"skinned bend": lambda k: k.bend(1.0), "morph": lambda k: k.bend(0.7), "rows": lambda k: k.rows(1.0), "rigid move": lambda k: k.move("rotate"),
         "both": lambda k: (k.bend(1.3), k.move("translate"))}


@pytest.mark.parametrize("case", list(CASES))
def test_xprev_against_float64(tmp, case):
    kind = "street" if case == "morph" else "cornell"
    k = vmotion.Case(tmp, kind, 64, 48, gpu=False)
    k.frame(0)
    CASES[case](k)
    desc = k.desc()
    prev = k.previous(desc)
    k.frame(1)
    vm = k.info["vm"]
    hit = vm["hits"]["inst"] != vmotion.MISS
    want, mag, flagged = float64_xprev(desc, k.verts, prev, vm["hits"][hit])
    assert flagged.sum() > 20, flagged.sum()                    # pixels that see a moved or deformed surface
    err = np.abs(vm["xprev"][hit].astype(np.float64) - want)
    assert (err[flagged] <= 16 * 2.0 ** -24 * mag[flagged]).all(), float((err[flagged] / mag[flagged]).max() * 2 ** 24)
    moved = np.abs(vm["d"][hit][flagged][:, :3]).max(axis=1) > 0
    assert moved.mean() > 0.5                                   # the pose moves the surface under most of its pixels
    assert not vm["d"][hit][~flagged].any() and not vm["d"][~hit].any() and not vm["d"][:, 3].any()    # copied elsewhere; zero at a miss; w = 0


# ---- 3. static properties --------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["cornell", "street"])
def test_nothing_moved_means_zero_delta_and_a_stopped_mesh_is_undeformed(tmp, kind):
    k = vmotion.Case(tmp, kind, 33, 17, gpu=False)
    for f, _ in vmotion.run_sequence(k, frames=5):
        vm, hit = k.info["vm"], k.info["hit"]
        flagged = k.flagged[0].any() or k.flagged[1].any()
        assert flagged == (f in (1, 2, 4)), f
        if f in (0, 3):         # frame 3: the mesh stopped for a frame
            assert not vm["d"].any() and np.array_equal(vm["m16"][hit].astype(np.int32), k.info["m_o"][hit]), f
        else:
            assert vm["d"].any(), f
        assert k.info["inexpressible"] == 0


# ---- 4. the checker under AddressSanitizer + UndefinedBehaviorSanitizer, in a program of its own --------------------------------------------------------------
def test_checker_under_the_sanitizers(tmp_path):
    host = os.path.join(ROOT, "cis-565-final-vr-raytracer_amd", "host")
    exe = str(tmp_path / "vmotion_san")
    srcs = [os.path.join(ROOT, "tests", "vmotion_san_main.cpp"), os.path.join(ROOT, "tests", "vmotion_checker.cpp"), os.path.join(ROOT, "oracle", "orc_scene.cpp")] + \
           [os.path.join(host, s) for s in ("scene.cpp", "scene_gen.cpp", "gltf_loader.cpp", "jpeg_decoder.cpp")]
    flags = ["-O1", "-g", "-std=c++17", "-pthread", "-mfma", "-ffp-contract=off", "-fno-fast-math", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
             "-fno-omit-frame-pointer", "-w"]
    cxx = os.environ.get("CXX", "g++")
    objs = [str(tmp_path / (os.path.basename(src) + ".o")) for src in srcs]
    jobs = [subprocess.Popen([cxx] + flags + ["-c", src, "-o", obj]) for src, obj in zip(srcs, objs)]      # one compiler per file, side by side
    assert all(j.wait() == 0 for j in jobs)
    subprocess.check_call([cxx] + flags + objs + ["-o", exe, "-lz"])
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "ok" in p.stdout
