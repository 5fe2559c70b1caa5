"""Light sources without a GPU: the CPU restatement of the light-record rewrite (tests/light_checker.cpp) against the records host.Scene recomputes after
updateInstances and updateVertices, Scene.lightSources against the uploaded records, the declared symbols, and the checker + Scene::lightSources under the
sanitizers in a program of their own.  tests/test_gpu_light_sources.py holds the HIP kernel to the checker word for word."""
import ctypes as C
import os
import re
import subprocess
import numpy as np
import pytest

from helpers import ROOT, abi
import lights
import refit
import skin

NAMES = ("rt_set_light_sources", "rt_lights_readback", "rt_get_light_stats")


@pytest.fixture(scope="module")
def chk(tmp_path_factory):
    return lights.build(tmp_path_factory.mktemp("lights"))


def scene_of(name):
    return refit.cornell() if name == "cornell" else refit.street()


def test_symbols_are_declared_and_listed():
    src = open(os.path.join(ROOT, "include", "rt_abi.h")).read()
    for n in NAMES:
        assert re.search(r"\bint " + n + r"\(rt_ctx\* ctx", src), n
    assert 'static_assert(sizeof(rt_light_stats) == 32, "rt_light_stats");' in src and 'static_assert(sizeof(rt_light_source) == 8, "rt_light_source");' in src
    assert re.search(r"#define RT_ABI_VERSION_MINOR (\d+)u", src).group(1) == "4"
    assert C.sizeof(abi.LightStats) == 32 and abi.LIGHT_SOURCE_DT.itemsize == 8 and abi.TRIG_LIGHT_DT.itemsize == 96 and abi.PUNC_LIGHT_DT.itemsize == 80
    from restir_amd import renderer, host
    assert set(NAMES) <= set(renderer.ABI_SYMBOLS)
    for m in ("set_light_sources", "lights_readback", "light_stats"):
        assert hasattr(renderer.Renderer, m)
    assert hasattr(host.Scene, "lightSources")
    L = C.CDLL(renderer.HIP_LIB_PATH)
    for n in NAMES:
        assert hasattr(L, n), n
    assert L.rt_set_light_sources(None, 0, None) == abi.ERR_INVALID_ARG and L.rt_get_light_stats(None, None) == abi.ERR_INVALID_ARG
    assert L.rt_lights_readback(None, 0, None, 0) == abi.ERR_INVALID_ARG


@pytest.mark.parametrize("name", ["cornell", "street"])
def test_light_sources_reproduce_the_uploaded_positions(chk, name):
    sc = scene_of(name)
    desc = sc.desc()
    src, rec = sc.lightSources(), lights.records_of(desc)
    inst, pm = refit.instances_of(desc), refit.prim_meshes_of(desc)
    assert src.size == rec.size == desc.lightInfo.trigLightSize > 0
    # the order createTrigLightBuffer emits: every emissive instance in order, its triangles in order
    want = [(int(i), k) for i in refit.describe(desc)["emissive"] for k in range(int(pm["indexCount"][inst["primMesh"][i]]) // 3)]
    assert [(int(s["instance"]), int(s["triangle"])) for s in src] == want
    blank = rec.copy()
    for f in ("v0", "v1", "v2"):
        blank[f] = np.nan
    got, n = lights.rewrite(chk, desc, src, blank)
    assert n == rec.size and np.array_equal(lights.raw(got), lights.raw(rec))


@pytest.mark.parametrize("name", ["cornell", "street"])
def test_checker_equals_the_scene_after_moves_and_deformations(chk, name):
    sc = scene_of(name)
    desc = sc.desc()
    src = sc.lightSources()
    home = refit.instances_of(desc)["objectToWorld"].copy()
    emissive = [int(i) for i in refit.describe(desc)["emissive"]]
    plain = next(i for i in range(desc.numInstances) if i not in emissive)
    extent = float(max(np.abs(np.concatenate(refit.world_bounds(desc, i))).max() for i in range(desc.numInstances)))
    rec = lights.records_of(desc)
    first = rec.copy()
    moved_any = False
    for step, kind in enumerate(("mirror", "scale", "rotate", "translate", "back")):
        ids = emissive[step % len(emissive)::2][:3] + [plain]      # a subset of the emitters and an instance that carries no light
        xf = np.stack([refit.move_matrix(kind, desc, i, extent, home) for i in ids])
        if kind in ("mirror", "scale"):
            dets = [np.linalg.det(m.reshape(3, 4)[:, :3].astype(np.float64)) for m in xf]
            assert (kind == "mirror" and min(dets) < 0) or (kind == "scale" and len(set(np.round(np.linalg.svd(xf[0].reshape(3, 4)[:, :3])[1], 3))) == 3)
        sc.updateInstances(ids, xf)
        desc = sc.desc()
        want = lights.records_of(desc)
        got, n = lights.rewrite(chk, desc, src, rec, dirty=ids)
        assert n == int(np.isin(src["instance"], ids).sum()) > 0
        assert np.array_equal(lights.raw(got), lights.raw(want)), kind
        moved_any |= not np.array_equal(lights.raw(want), lights.raw(rec))
        rec = want
    assert moved_any
    # deformation: every instance of the deformed mesh follows, the others keep their bytes
    m = int(refit.instances_of(desc)["primMesh"][emissive[0]])
    rows = lights.positions_moved(desc, m, (0.02, -0.01, 0.03))
    sc.updateVertices(m, 0, rows)
    desc = sc.desc()
    want = lights.records_of(desc)
    ids = skin.instances_of_mesh(desc, m)
    got, n = lights.rewrite(chk, desc, src, rec, dirty=ids)
    assert n == int(np.isin(src["instance"], ids).sum()) and np.array_equal(lights.raw(got), lights.raw(want))
    assert not np.array_equal(lights.raw(want)[:, lights.POS], lights.raw(rec)[:, lights.POS])
    # only bytes 8..43 ever moved
    keep = np.ones(96, bool)
    keep[lights.POS] = False
    assert np.array_equal(lights.raw(want)[:, keep], lights.raw(first)[:, keep])
    # the binding in another order: records and sources permuted together describe the same lights
    perm = np.arange(src.size)[::-1].copy()
    prec, psrc = lights.permuted(want, src, perm)
    got, _ = lights.rewrite(chk, desc, psrc, prec)
    assert np.array_equal(lights.raw(got), lights.raw(prec))
    assert np.array_equal(prec["impSamp"]["alias"][np.argsort(perm)], np.argsort(perm)[want["impSamp"]["alias"]])


def test_checker_and_light_sources_under_the_sanitizers(tmp_path):
    host = os.path.join(ROOT, "cis-565-final-vr-raytracer_amd", "host")
    exe = str(tmp_path / "lights_san")
    srcs = [os.path.join(ROOT, "tests", "lights_san_main.cpp"), os.path.join(ROOT, "tests", "light_checker.cpp")] + \
           [os.path.join(host, s) for s in ("scene.cpp", "scene_gen.cpp", "gltf_loader.cpp", "jpeg_decoder.cpp")]
    flags = ["-O1", "-g", "-std=c++17", "-pthread", "-ffp-contract=off", "-fno-fast-math", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
             "-fno-omit-frame-pointer", "-w"]
    cxx = os.environ.get("CXX", "g++")
    objs = [str(tmp_path / (os.path.basename(src) + ".o")) for src in srcs]
    jobs = [subprocess.Popen([cxx] + flags + ["-c", src, "-o", obj]) for src, obj in zip(srcs, objs)]      # one compiler per file, side by side
    assert all(j.wait() == 0 for j in jobs)
    subprocess.check_call([cxx] + flags + objs + ["-o", exe, "-lz"])
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "ok" in p.stdout
