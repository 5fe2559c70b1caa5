"""Morph targets without a GPU: the CPU restatement of the arithmetic (tests/morph_checker.cpp) against a numpy float32 evaluation in the stated order, bit for
bit (numpy does not contract); the rules around zero weights, the sentinel, absent planes and overflow; the symbols and struct sizes; and the checker under the
sanitizers in a program of its own.  tests/test_gpu_morph.py holds the HIP kernel to the checker word for word."""
import ctypes as C
import os
import re
import subprocess
import numpy as np
import pytest

from helpers import ROOT, abi
import morph
import skin

NAMES = ("rt_set_morph_targets", "rt_update_morphs", "rt_get_morph_stats")


@pytest.fixture(scope="module")
def chk(tmp_path_factory):
    return morph.build(tmp_path_factory.mktemp("morph"))


@pytest.fixture(scope="module")
def sk(tmp_path_factory):
    return skin.build(tmp_path_factory.mktemp("skin"))


def rest_rows(chk, rng, n):
    rest = np.zeros(n, morph.VERTEX_DT)
    rest["position"] = rng.uniform(-2, 2, (n, 3)).astype(np.float32)
    rest["normal"] = [chk.mpc_encode(*x) for x in rng.normal(size=(n, 3)).astype(np.float32)]
    rest["tangent"] = [chk.mpc_encode(*x) for x in rng.normal(size=(n, 3)).astype(np.float32)]
    rest["texcoord"] = rng.random((n, 2)).astype(np.float32)
    rest["color"] = rng.integers(0, 2 ** 32, n, dtype=np.uint32)
    rest["normal"][0] = 0xffffffff
    rest["tangent"][1] = 0xffffffff
    return rest


def test_header_and_python_mirror():
    src = open(os.path.join(ROOT, "include", "rt_abi.h")).read()
    for n in NAMES:
        assert re.search(r"\bint " + n + r"\(rt_ctx\* ctx", src), n
    for t in ("rt_morph_set) == 16", "rt_morph_delta) == 16", "rt_morph_stats) == 32"):
        assert "static_assert(sizeof(" + t in src
    assert re.search(r"#define RT_ABI_VERSION_MINOR (\d+)u", src).group(1) == "4"
    assert "enum { RT_MORPH_NORMALS = 1, RT_MORPH_TANGENTS = 2 };" in src
    assert C.sizeof(abi.MorphStats) == 32 and abi.MORPH_SET_DT.itemsize == 16 and abi.MORPH_DELTA_DT.itemsize == 16
    assert (abi.MORPH_NORMALS, abi.MORPH_TANGENTS) == (1, 2)
    from restir_amd import renderer
    assert set(NAMES) <= set(renderer.ABI_SYMBOLS)
    for m in ("set_morph_targets", "update_morphs", "morph_stats"):
        assert hasattr(renderer.Renderer, m)
    hpp = open(os.path.join(ROOT, "cis-565-final-vr-raytracer_amd", "host", "renderer.hpp")).read()
    assert "bool setMorphTargets(" in hpp and "bool updateMorphs(" in hpp
    L = C.CDLL(renderer.HIP_LIB_PATH)
    for n in NAMES:
        assert hasattr(L, n), n
    L.rt_set_morph_targets.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint64, C.c_void_p]
    assert L.rt_set_morph_targets(None, 0, None, 0, None) == abi.ERR_INVALID_ARG
    assert L.rt_update_morphs(None, 0, None, None) != 0 and L.rt_get_morph_stats(None, None) == abi.ERR_INVALID_ARG


# ---- 1. the checker's positions against numpy float32 in the stated order, bit for bit ---------------------------------------------------------------------
@pytest.mark.parametrize("seed,targets,planes", [(1, 1, 0), (2, 2, 3), (3, 9, 1), (4, 9, 2)])
def test_positions_equal_numpy_float32_in_the_stated_order(chk, sk, seed, targets, planes):
    rng = np.random.default_rng(seed)
    n = 301
    rest = rest_rows(chk, rng, n)
    deltas = morph.random_deltas(n, targets, planes, seed)
    w = rng.uniform(-1.5, 2.5, targets).astype(np.float32)
    if targets > 2:
        w[[1, 4]] = 0.0
        w[6] = -0.0
    out, bad, active = morph.morph(chk, rest, deltas, targets, planes, w)
    assert bad == 0 and active == int((w != 0).sum())
    P = morph.planes_per_target(planes)
    dP = deltas["d"].reshape(targets, P, n, 3)[:, 0]
    p = rest["position"].copy()
    for t in range(targets):
        if w[t] != 0:
            prod = (w[t] * dP[t]).astype(np.float32)      # rounded before the add
            p = (p + prod).astype(np.float32)
    assert p.dtype == np.float32 and np.array_equal(out["position"].view(np.uint32), p.view(np.uint32))
    assert not np.array_equal(out["position"], rest["position"])
    assert np.array_equal(out["texcoord"].view(np.uint32), rest["texcoord"].view(np.uint32)) and np.array_equal(out["color"], rest["color"])
    # directions: a plane that is present turns the packed value (except the sentinel); a plane that is absent keeps it
    assert out["normal"][0] == 0xffffffff and out["tangent"][1] == 0xffffffff
    assert ((out["normal"][1:] != rest["normal"][1:]).mean() > 0.9) == bool(planes & 1)
    assert ((out["tangent"][2:] != rest["tangent"][2:]).mean() > 0.9) == bool(planes & 2)
    if not planes & 1:
        assert np.array_equal(out["normal"], rest["normal"])
    if not planes & 2:
        assert np.array_equal(out["tangent"], rest["tangent"])
    # the packed normal is the numpy float32 sum in the stated order, normalised in float32 and encoded (decoder: tests/skin_checker.cpp's; encoder: host/pack.h)
    if planes & 1:
        dN = deltas["d"].reshape(targets, P, n, 3)[:, 1]
        m = skin.decode(sk, rest["normal"])
        for t in range(targets):
            if w[t] != 0:
                m = (m + (w[t] * dN[t]).astype(np.float32)).astype(np.float32)
        d = ((m[:, 0] * m[:, 0] + m[:, 1] * m[:, 1]).astype(np.float32) + m[:, 2] * m[:, 2]).astype(np.float32)
        assert (d > 0).all()
        q = (np.float32(1) / np.sqrt(d)).astype(np.float32)
        want = [chk.mpc_encode(*(m[k] * q[k])) for k in range(n)]
        assert list(out["normal"][1:]) == want[1:]


# ---- 2. the rules ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("planes", [0, 1, 2, 3])
def test_zero_and_negative_zero_weights_give_the_rest_rows_bit_for_bit(chk, planes):
    rng = np.random.default_rng(7)
    n = 70
    rest = rest_rows(chk, rng, n)
    rest["position"][3] = [-0.0, 0.0, -0.0]            # -0 + 0 d would give +0: an inactive target is skipped, not multiplied
    deltas = morph.random_deltas(n, 3, planes, 7)
    for w in ([0, 0, 0], [-0.0, 0, -0.0]):
        out, bad, active = morph.morph(chk, rest, deltas, 3, planes, np.array(w, np.float32))
        assert (bad, active) == (0, 0)
        assert np.array_equal(out.view(np.uint32), rest.view(np.uint32))      # the packed normals and tangents included: no decode / encode round trip
    # one active target among inactive ones equals that target alone
    a, _, na = morph.morph(chk, rest, deltas, 3, planes, np.array([0, 0.75, -0.0], np.float32))
    P = morph.planes_per_target(planes)
    b, _, nb = morph.morph(chk, rest, deltas[P * n:2 * P * n], 1, planes, np.array([0.75], np.float32))
    assert (na, nb) == (1, 1) and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def test_the_sentinel_stays_and_a_vanishing_direction_keeps_the_rest_value(chk, sk):
    rest = np.zeros(3, morph.VERTEX_DT)
    rest["normal"] = [0xffffffff, chk.mpc_encode(0, 1, 0), chk.mpc_encode(0, 1, 0)]
    rest["tangent"] = [chk.mpc_encode(1, 0, 0), 0xffffffff, chk.mpc_encode(1, 0, 0)]
    n1 = skin.decode(sk, rest["normal"][1:2])[0]
    deltas = np.zeros(9, morph.DELTA_DT)                  # one target, three planes, three vertices
    deltas["d"][3:6] = -n1                               # normal plane: cancels the decoded normal exactly (weight 1): d = 0, the rest value stays
    deltas["d"][6:9] = [0, 2, 0]                         # tangent plane
    out, bad, _ = morph.morph(chk, rest, deltas, 1, 3, [1.0])
    assert bad == 0
    assert out["normal"][0] == 0xffffffff and out["normal"][1] == rest["normal"][1] and out["normal"][2] == rest["normal"][2]
    assert out["tangent"][1] == 0xffffffff and out["tangent"][0] != rest["tangent"][0] and out["tangent"][0] == out["tangent"][2]


def test_an_overflowing_weight_delta_pair_is_counted(chk):
    rng = np.random.default_rng(9)
    rest = rest_rows(chk, rng, 5)
    deltas = np.zeros(5, morph.DELTA_DT)
    deltas["d"][2] = [10, 0, 0]
    deltas["d"][4] = [0, 0, -10]
    out, bad, active = morph.morph(chk, rest, deltas, 1, 0, [3e38])
    assert (bad, active) == (2, 1) and np.isinf(out["position"][2, 0]) and np.isinf(out["position"][4, 2])


def test_morph_then_skin_feeds_the_skin_checker(chk, sk):
    rng = np.random.default_rng(11)
    rest = rest_rows(chk, rng, 40)
    deltas = morph.random_deltas(40, 2, 3, 11)
    inf = skin.influences_by_height(rest, 3)
    mats = skin.pose_matrices("bend", 3, np.zeros(3), 1.0)
    same, _, _ = morph.morph(chk, rest, deltas, 2, 3, [0, 0])
    a, bad = skin.pose(sk, same, inf, mats)
    b, _ = skin.pose(sk, rest, inf, mats)
    assert bad == 0 and np.array_equal(a.view(np.uint32), b.view(np.uint32))      # zero weights: the skin alone
    moved, _, _ = morph.morph(chk, rest, deltas, 2, 3, [0.5, -0.25])
    c, bad = skin.pose(sk, moved, inf, mats)
    assert bad == 0 and not np.array_equal(c["position"], b["position"])


# ---- 3. the checker under AddressSanitizer + UndefinedBehaviorSanitizer, in a program of its own ------------------------------------------------------------
def test_checker_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / "morph_san")
    srcs = [os.path.join(ROOT, "tests", "morph_san_main.cpp"), os.path.join(ROOT, "tests", "morph_checker.cpp")]
    flags = ["-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
             "-fno-omit-frame-pointer", "-w"]
    subprocess.check_call([os.environ.get("CXX", "g++")] + flags + srcs + ["-o", exe])
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "ok" in p.stdout
