"""The emitter mode without a GPU (include/rt_abi.h "Emitters"): the sequential restatement of the derived light records (tests/light_derive_checker.cpp) with the
templates of Scene.emitterMeshes gives, for tables that add, remove, swap and interleave emitters, the records, the count and trigSampProb host.Scene.setInstances
computes, all 96 bytes of every record; the declared symbols; the checker + Scene::emitterMeshes under the sanitizers in a program of their own.
tests/test_gpu_emitters.py holds the HIP kernel and the context to the checker word for word.  Exact comparisons only."""
import ctypes as C
import os
import re
import subprocess
import numpy as np
import pytest

from helpers import ROOT, abi
import emitters
import lights
import refit

NAMES = ("rt_set_emitter_meshes", "rt_get_emitter_stats")


@pytest.fixture(scope="module")
def chk(tmp_path_factory):
    return emitters.build(tmp_path_factory.mktemp("emitters"))


def scene_of(name):
    return refit.cornell() if name == "cornell" else refit.street()


def test_symbols_are_declared_and_listed():
    src = open(os.path.join(ROOT, "include", "rt_abi.h")).read()
    for n in NAMES:
        assert re.search(r"\bint " + n + r"\(rt_ctx\* ctx", src), n
    assert "sizeof(rt_emitter_mesh) == 16 && sizeof(rt_emitter_row) == 32 && sizeof(rt_emitter_stats) == 32" in src
    assert re.search(r"#define RT_ABI_VERSION_MINOR (\d+)u", src).group(1) == "4"
    assert C.sizeof(abi.EmitterStats) == 32 and abi.EMITTER_MESH_DT.itemsize == 16 and abi.EMITTER_ROW_DT.itemsize == 32
    from restir_amd import renderer, host
    assert set(NAMES) <= set(renderer.ABI_SYMBOLS)
    for m in ("set_emitter_meshes", "emitter_stats"):
        assert hasattr(renderer.Renderer, m)
    assert hasattr(host.Scene, "emitterMeshes")
    L = C.CDLL(renderer.HIP_LIB_PATH)
    for n in NAMES:
        assert hasattr(L, n), n
    L.rt_set_emitter_meshes.argtypes = abi.SET_EMITTER_MESHES_ARGTYPES
    assert L.rt_set_emitter_meshes(None, 0, None, 0, None, 0.0) == abi.ERR_INVALID_ARG and L.rt_get_emitter_stats(None, None) == abi.ERR_INVALID_ARG


@pytest.mark.parametrize("name", ["cornell", "street"])
def test_templates_reproduce_the_uploaded_records(chk, name):
    sc = scene_of(name)
    desc = sc.desc()
    meshes, rows = sc.emitterMeshes()
    pm, inst = refit.prim_meshes_of(desc), refit.instances_of(desc)
    em = refit.describe(desc)["emissive"]
    assert sorted(int(m) for m in meshes["primMesh"]) == sorted(set(int(inst["primMesh"][i]) for i in em))      # (every emissive mesh of these scenes has an instance)
    for m in meshes:      # ascending triangles, all of them, the rows of a mesh contiguous
        assert np.array_equal(rows["triangle"][m["firstRow"]:m["firstRow"] + m["rowCount"]], np.arange(int(pm["indexCount"][m["primMesh"]]) // 3))
    rec, src, info, emitting = emitters.derive(chk, desc, inst, meshes, rows, sc.lightWeights[0], emitters.info_of(desc))
    want = lights.records_of(desc)
    assert rec.size == want.size == desc.lightInfo.trigLightSize > 0 and emitting == len(em)
    assert np.array_equal(lights.raw(rec), lights.raw(want))
    assert np.array_equal(src, sc.lightSources())
    assert info.trigLightSize == desc.lightInfo.trigLightSize and emitters.prob_bits(info) == emitters.prob_bits(desc.lightInfo)
    # an emissive mesh without a template: the first instance that uses it is named
    first = int(meshes["primMesh"][0])
    assert emitters.derive(chk, desc, inst, meshes[1:], rows, 0.0, emitters.info_of(desc)) == int(np.nonzero(inst["primMesh"] == first)[0][0])


@pytest.mark.parametrize("name", ["cornell", "street"])
def test_checker_equals_the_scene_over_the_table_sequence(chk, name):
    sc = scene_of(name)
    desc0 = sc.desc()
    meshes, rows = sc.emitterMeshes()
    punc = sc.lightWeights[0]
    steps = emitters.sequence(desc0)
    dets = [np.linalg.det(m.reshape(3, 4)[:, :3].astype(np.float64)) for _, t in steps for m in t["objectToWorld"]]
    assert min(dets) < 0      # mirrored copies are among the tables
    assert any(len(set(np.round(np.linalg.svd(m.reshape(3, 4)[:, :3].astype(np.float64))[1], 3))) == 3 for _, t in steps for m in t["objectToWorld"])      # and non-uniformly scaled ones
    info = emitters.info_of(desc0)
    counts = []
    for label, table in steps:
        before = emitters.LightInfo.from_buffer_copy(info)
        sc.setInstances(table)
        desc = sc.desc()
        want = lights.records_of(desc)
        rec, src, info, emitting = emitters.derive(chk, desc, table, meshes, rows, punc, before)
        print(name, label, "records", rec.size, "emitting", emitting, "trigSampProb", info.trigSampProb)
        assert rec.size == want.size == desc.lightInfo.trigLightSize == info.trigLightSize, label
        assert np.array_equal(lights.raw(rec), lights.raw(want)), label      # all 96 bytes
        assert np.array_equal(src, sc.lightSources()), label
        assert emitters.prob_bits(info) == emitters.prob_bits(desc.lightInfo), label
        if rec.size == 0 and info.puncLightSize == 0:      # no light of either kind: the value stays
            assert emitters.prob_bits(info) == emitters.prob_bits(before) and before.trigSampProb > 0, label
        counts.append(rec.size)
    assert 0 in counts and counts[-1] == desc0.lightInfo.trigLightSize and len(set(counts)) > 2
    if name == "cornell":
        assert desc0.lightInfo.puncLightSize == 0      # the both-counts-zero case above is taken


def test_checker_and_emitter_meshes_under_the_sanitizers(tmp_path):
    host = os.path.join(ROOT, "cis-565-final-vr-raytracer_amd", "host")
    exe = str(tmp_path / "emitters_san")
    srcs = [os.path.join(ROOT, "tests", "emitters_san_main.cpp"), emitters.SRC] + [os.path.join(host, s) for s in ("scene.cpp", "scene_gen.cpp", "gltf_loader.cpp", "jpeg_decoder.cpp")]
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
