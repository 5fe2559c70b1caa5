"""Deforming meshes without a GPU: the CPU restatement of the skinning arithmetic (tests/skin_checker.cpp) against float64 numpy, the refit checker on a deformed
scene against a fresh build of it, Scene.updateVertices' light records against numpy, and the checker + Scene::updateVertices under the sanitizers in a program of
their own.  tests/test_gpu_skin.py holds the HIP kernels to the checker word for word."""
import ctypes as C
import os
import re
import subprocess
import numpy as np
import pytest

from helpers import ROOT, abi
import refit
import skin

NAMES = ("rt_update_vertices", "rt_set_skins", "rt_update_skins", "rt_vertices_readback", "rt_get_deform_stats")
TRIG_DT = np.dtype([("matIndex", "<u4"), ("transformIndex", "<u4"), ("v", "<f4", (3, 3)), ("uv", "<f4", (3, 2)), ("impSamp", "<u4", 4), ("pad", "<f4", 3)])


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    return refit.build(tmp_path_factory.mktemp("refit"))


@pytest.fixture(scope="module")
def chk(tmp_path_factory):
    return skin.build(tmp_path_factory.mktemp("skin"))


def test_header_and_python_mirror():
    src = open(os.path.join(ROOT, "include", "rt_abi.h")).read()
    for n in NAMES:
        assert re.search(r"\bint " + n + r"\(rt_ctx\* ctx", src), n
    assert 'static_assert(sizeof(rt_deform_stats) == 32, "rt_deform_stats");' in src and 'static_assert(sizeof(rt_skin_influence) == 24, "rt_skin_influence");' in src
    assert re.search(r"#define RT_ABI_VERSION_MINOR (\d+)u", src).group(1) == "4"
    assert C.sizeof(abi.DeformStats) == 32 and abi.SKIN_DT.itemsize == 16 and abi.SKIN_INFLUENCE_DT.itemsize == 24 and abi.VERTEX_DT.itemsize == 32
    from restir_amd import renderer, host
    assert set(NAMES) <= set(renderer.ABI_SYMBOLS)
    for m in ("update_vertices", "set_skins", "update_skins", "vertices_readback", "deform_stats"):
        assert hasattr(renderer.Renderer, m)
    assert hasattr(host.Scene, "updateVertices")
    L = C.CDLL(renderer.HIP_LIB_PATH)
    for n in NAMES:
        assert hasattr(L, n), n
    assert L.rt_update_skins(None, 0, None, None) == abi.ERR_INVALID_ARG and L.rt_get_deform_stats(None, None) == abi.ERR_INVALID_ARG


# ---- 1. the checker against float64 numpy ----------------------------------------------------------------------------------------------------------------
def random_case(chk, rng, n, joints, mirrored):
    rest = np.zeros(n, skin.VERTEX_DT)
    rest["position"] = rng.uniform(-2, 2, (n, 3)).astype(np.float32)
    rest["normal"] = [chk.skc_encode(*x) for x in rng.normal(size=(n, 3)).astype(np.float32)]
    rest["tangent"] = [chk.skc_encode(*x) for x in rng.normal(size=(n, 3)).astype(np.float32)]
    rest["texcoord"] = rng.random((n, 2)).astype(np.float32)
    rest["color"] = rng.integers(0, 2 ** 32, n, dtype=np.uint32)
    inf = np.zeros(n, skin.INFLUENCE_DT)
    inf["joint"] = rng.integers(0, joints, (n, 4))
    w = rng.random((n, 4))
    w[rng.random((n, 4)) < 0.3] = 0.0
    w[0] = 0.0                                    # a zero-weight row: B = 0, the position collapses to 0 and the directions keep the rest values
    w[1:] /= np.maximum(w[1:].sum(axis=1, keepdims=True), 1e-3)
    inf["weight"] = w.astype(np.float32)
    M = []
    for k in range(joints):
        A = skin.rot("xyz"[k % 3], rng.uniform(-2, 2)) @ skin.rot("y", rng.uniform(-1, 1)) @ np.diag(rng.uniform(0.6, 1.5, 3))
        if k == mirrored:
            A = A @ np.diag([1.0, -1.0, 1.0])
        M.append(skin.affine(A, rng.uniform(-1, 1, 3)))
    return rest, inf, np.stack(M)


@pytest.mark.parametrize("seed,joints", [(1, 1), (2, 5), (3, 9)])
def test_checker_against_float64_linear_blend(chk, seed, joints):
    rng = np.random.default_rng(seed)
    n = 400
    rest, inf, M = random_case(chk, rng, n, joints, mirrored=joints - 1 if joints > 1 else None)
    out, bad = skin.pose(chk, rest, inf, M)
    assert bad == 0
    assert np.array_equal(out["texcoord"].view(np.uint32), rest["texcoord"].view(np.uint32)) and np.array_equal(out["color"], rest["color"])
    Mj = M.astype(np.float64).reshape(-1, 3, 4)[inf["joint"]]            # n x 4 x 3 x 4
    w = inf["weight"].astype(np.float64)
    p1 = np.concatenate([rest["position"].astype(np.float64), np.ones((n, 1))], axis=1)
    want = np.einsum("nk,nkrc,nc->nr", w, Mj, p1)
    bound = 16 * 2.0 ** -24 * np.einsum("nk,nkrc,nc->nr", np.abs(w), np.abs(Mj), np.abs(p1))
    err = np.abs(out["position"].astype(np.float64) - want)
    print("largest position error / bound:", float((err / np.maximum(bound, 1e-300)).max()))
    assert (err <= bound).all()
    assert np.array_equal(out["position"][0], np.zeros(3, np.float32)) and out["normal"][0] == rest["normal"][0] and out["tangent"][0] == rest["tangent"][0]
    # directions: within the oct grid's step of the float64 vector.  The codec rounds x and y of the L1-normalised vector to multiples of 1 / 32767 (an error of at
    # most half a unit each) and takes z from them (at most one unit): the L1 point is off by at most sqrt(1.5) / 32767, and normalising stretches by at most sqrt(3)
    # (an L1-unit vector is at least 1 / sqrt(3) long).  The step allows the full neighbour distance sqrt(2) sqrt(3) / 32767 = 7.5e-5, which leaves 1e-5 over the
    # codec's 6.5e-5 for the fp32 transform: 2^-23 relative per cofactor, times the condition number, below 1.2e-5 for the blends kept here (condition below 10).
    # Both sides start from the same decoded fp32 input.
    step = np.sqrt(2.0) * np.sqrt(3.0) / 32767.0
    B = np.einsum("nk,nkrc->nrc", w, Mj)[:, :, :3]
    live = np.array([np.linalg.cond(b) < 10 if np.abs(b).max() > 0 else False for b in B])
    assert live.sum() > n // 4
    nrm, tng = skin.decode(chk, rest["normal"]).astype(np.float64), skin.decode(chk, rest["tangent"]).astype(np.float64)
    wn = np.einsum("nrc,nc->nr", np.linalg.inv(B[live]).transpose(0, 2, 1), nrm[live])
    wn /= np.linalg.norm(wn, axis=1, keepdims=True)
    wt = np.einsum("nrc,nc->nr", B[live], tng[live])
    wt /= np.linalg.norm(wt, axis=1, keepdims=True)
    gn, gt = skin.decode(chk, out["normal"][live]).astype(np.float64), skin.decode(chk, out["tangent"][live]).astype(np.float64)
    en, et = np.linalg.norm(gn - wn, axis=1), np.linalg.norm(gt - wt, axis=1)
    print("largest normal / tangent error in grid steps:", float(en.max() / step), float(et.max() / step))
    assert (en <= step).all() and (et <= step).all()
    # a mirrored blend keeps the normal on the outside: inverse transpose times the sign of the determinant is what the cofactors give
    flipped = np.linalg.det(B[live]) < 0
    assert flipped.any() == (joints > 1) and (~flipped).any()


def test_sentinel_and_degenerate_directions_keep_the_rest_values(chk):
    rest = np.zeros(3, skin.VERTEX_DT)
    rest["position"] = [[1, 2, 3]] * 3
    rest["normal"] = [0xffffffff, chk.skc_encode(0, 1, 0), chk.skc_encode(0, 1, 0)]
    rest["tangent"] = [chk.skc_encode(1, 0, 0), 0xffffffff, chk.skc_encode(1, 0, 0)]
    inf = np.zeros(3, skin.INFLUENCE_DT)
    inf["weight"][:, 0] = 1
    flat = skin.affine(np.diag([1.0, 0.0, 0.0]))          # rank 1: every cofactor is 0; the tangent along x survives
    out, bad = skin.pose(chk, rest, inf, [flat])
    assert bad == 0 and list(out["normal"]) == list(rest["normal"]) and out["tangent"][1] == 0xffffffff and out["tangent"][2] == rest["tangent"][2]
    huge = skin.affine(np.eye(3) * 3e38)
    inf["weight"][:, 1] = 1                                 # 3e38 + 3e38 overflows in the blend
    out, bad = skin.pose(chk, rest, inf, [huge])
    assert bad == 3


# ---- 2. the refit checker on a deformed scene ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["cornell", "street"])
def test_refit_of_a_deformed_scene_equals_a_fresh_build(lib, chk, name):
    sc = refit.cornell() if name == "cornell" else refit.street()
    desc = sc.desc()
    t = refit.Tree.built(lib, desc)
    ext = refit.scene_extent(t)
    m = skin.deformed_mesh(name, desc)
    ids = skin.instances_of_mesh(desc, m)
    xf = refit.instances_of(desc)["objectToWorld"][ids]
    sk = skin.SkinnedMesh(chk, desc, m, 3)
    verts = skin.vertices_of(desc)
    fulls = 0
    for kind in skin.POSES:
        verts[sk.first:sk.first + sk.count] = sk.posed(sk.matrices(kind, ext))
        d2 = skin.with_vertices(desc, verts.copy())
        t.desc = d2
        assert t.refit(ids, xf) == 0, kind
        assert t.check() == (0, ""), kind
        fulls += int(t.stats[3])
        f = refit.Tree.built(lib, d2)
        assert np.float32(f.tri_pad).tobytes() == np.float32(t.tri_pad).tobytes(), kind
        assert f.inst.tobytes() == t.inst.tobytes()
        by_id = {}
        fr = f.records()
        for k in np.argsort(fr["globalId"], kind="stable"):
            by_id.setdefault(int(fr["globalId"][k]), fr[k])
        r = t.records()
        want = np.array([by_id[int(g)] for g in r["globalId"]], dtype=refit.REC_DT)
        for field in ("v0", "e1", "e2", "flags"):
            assert np.array_equal(r[field].view(np.uint32), want[field].view(np.uint32)), (kind, field)
    assert fulls >= 1


# ---- 3. Scene.updateVertices -----------------------------------------------------------------------------------------------------------------------------
def test_scene_update_vertices_recomputes_the_light_records(chk):
    sc = refit.cornell()
    desc = sc.desc()
    inst, pm = refit.instances_of(desc), refit.prim_meshes_of(desc)
    light = int(refit.describe(desc)["emissive"][0])
    m = int(inst["primMesh"][light])
    nt = desc.lightInfo.trigLightSize
    before = np.frombuffer((C.c_char * (nt * 96)).from_address(desc.trigLights), dtype=TRIG_DT).copy()
    sk = skin.SkinnedMesh(chk, desc, m, 2)
    sk.influences["joint"][:, 0] = sk.rest["position"][:, 0] > 0      # (the light is flat in y: its +x half follows joint 1)
    sk.influences["weight"][:] = [1, 0, 0, 0]
    rows = sk.posed(sk.matrices("bend", 1.0))
    assert not np.array_equal(rows["position"], sk.rest["position"])
    # a partial range first, then the whole mesh
    sc.updateVertices(m, 1, rows[1:3])
    assert np.array_equal(skin.vertices_of(sc.desc())[sk.first + 1:sk.first + 3].view(np.uint32), rows[1:3].view(np.uint32))
    assert np.array_equal(skin.vertices_of(sc.desc())[sk.first:sk.first + 1].view(np.uint32), sk.rest[:1].view(np.uint32))
    sc.updateVertices(m, 0, rows)
    desc = sc.desc()
    verts = skin.vertices_of(desc)
    assert np.array_equal(verts[sk.first:sk.first + sk.count].view(np.uint32), rows.view(np.uint32))
    assert desc.lightInfo.trigLightSize == nt
    after = np.frombuffer((C.c_char * (nt * 96)).from_address(desc.trigLights), dtype=TRIG_DT).copy()
    # numpy: every emissive instance in order, every triangle: ((m0 x + m1 y) + m2 z) + m3 per row, fp32
    idx = np.frombuffer((C.c_char * (desc.numIndices * 4)).from_address(desc.indices), dtype=np.uint32)
    mats = np.frombuffer((C.c_char * (desc.numMaterials * 80)).from_address(desc.materials), dtype=np.float32).reshape(-1, 20)
    want_v, power = [], []
    for i in refit.describe(desc)["emissive"]:
        p = pm[inst["primMesh"][i]]
        M = inst["objectToWorld"][i].reshape(3, 4)
        e = mats[max(int(p["materialIndex"]), 0), 9:12]
        for k in range(int(p["indexCount"]) // 3):
            tri = verts["position"][int(p["vertexOffset"]) + idx[int(p["firstIndex"]) + 3 * k:int(p["firstIndex"]) + 3 * k + 3]]
            want_v.append(((M[:, 0] * tri[:, 0:1] + M[:, 1] * tri[:, 1:2]) + M[:, 2] * tri[:, 2:3]) + M[:, 3])
            power.append((e[0] * np.float32(0.2126) + e[1] * np.float32(0.7152)) + e[2] * np.float32(0.0722))
    want_v = np.array(want_v, np.float32)
    assert want_v.shape == after["v"].shape
    assert np.array_equal(after["v"].view(np.uint32), want_v.view(np.uint32))
    assert not np.array_equal(after["v"], before["v"])
    for field in ("matIndex", "uv", "impSamp"):
        assert np.array_equal(after[field], before[field]), field      # the alias table depends on the materials only
    total = np.float32(0)
    for x in power:
        total = np.float32(total + x)
    punc = np.float32(sc.lightWeights[0])
    assert np.float32(desc.lightInfo.trigSampProb).tobytes() == np.float32(total / np.float32(total + punc)).tobytes()
    # refusals change nothing
    with pytest.raises(ValueError):
        sc.updateVertices(m, sk.count - 1, rows[:2])
    with pytest.raises(ValueError):
        sc.updateVertices(desc.numPrimMeshes, 0, rows[:1])
    assert np.array_equal(skin.vertices_of(sc.desc()).view(np.uint32), verts.view(np.uint32))


# ---- 4. the checker and Scene::updateVertices under AddressSanitizer + UndefinedBehaviorSanitizer, in a program of their own -------------------------------
def test_checker_and_update_vertices_under_the_sanitizers(tmp_path):
    host = os.path.join(ROOT, "cis-565-final-vr-raytracer_amd", "host")
    exe = str(tmp_path / "skin_san")
    srcs = [os.path.join(ROOT, "tests", "skin_san_main.cpp"), os.path.join(ROOT, "tests", "skin_checker.cpp")] + \
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
