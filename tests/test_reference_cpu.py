"""Reference mode (rt_reference_*, ABI 2.4) without a GPU: the CPU restatement tests/refpt_checker.cpp builds over the oracle's shading library,
keeps its determinism contract (split invariance, fp64 sums, float(sum / n)) and is exact where the estimator has no randomness (emitter and miss
pixels, against the oracle's own direct stage); include/rt_abi.h declares the entry points the product library exports."""
import ctypes as C
import os
import re
import numpy as np
import pytest
from helpers import ROOT, abi, host, make_scene
import refpt
from refpt import deterministic_pixels

# (name, kind, scale, env, W, H)
SCENES = [("cornell", abi.PROC_CORNELL, 1.0, None, 48, 48), ("sponza-env", abi.PROC_SPONZA, 0.01, (64, 32), 48, 32)]


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    return refpt.build(tmp_path_factory.mktemp("refpt"))


def _setup(lib, kind, scale, env_size, W, H):
    sc, env = make_scene(kind, scale, 1, env_size)
    st = host.default_state(W, H, sc, env)
    if env is None:
        st.environmentProb = 0.0
    desc = sc.desc(env)
    k = refpt.RefChecker(lib, desc)
    k.resize(W, H)
    sc.updateCamera(W, H)
    cam = sc.getCamera()
    k.set_camera(cam)
    return sc, env, desc, st, cam, k


def test_checker_builds(lib):
    for n in ("refpt_create", "refpt_render", "refpt_readback", "refpt_reset", "refpt_samples"):
        assert hasattr(lib, n)


@pytest.mark.parametrize("name,kind,scale,env_size,W,H", SCENES, ids=[s[0] for s in SCENES])
def test_checker_split_invariant(lib, name, kind, scale, env_size, W, H):
    """8 samples as 1 x 8, 8 x 1 and 3 + 5 (and over 1 or 8 threads): identical bytes, n = 8"""
    sc, env, desc, st, cam, k = _setup(lib, kind, scale, env_size, W, H)
    outs = []
    for split, threads in (([8], 8), ([1] * 8, 8), ([3, 5], 1)):
        k.reset()
        for s in split:
            k.render(st, s, threads)
        assert k.samples() == 8
        outs.append([k.readback(c) for c in range(3)])
    for o in outs[1:]:
        for c in range(3):
            assert np.array_equal(o[c].view(np.uint32), outs[0][c].view(np.uint32)), c
    d, i, s = outs[0]
    assert np.isfinite(s).all() and s[..., :3].max() > 0 and (s[..., 3] == 1).all()
    # component 2 is float((sumD + sumI) / n): within one rounding of the two float means' sum
    assert np.allclose(s[..., :3], d[..., :3] + i[..., :3], rtol=1e-6, atol=0)


@pytest.mark.parametrize("name,kind,scale,env_size,W,H", SCENES, ids=[s[0] for s in SCENES])
def test_checker_emitter_and_miss_pixels_exact(lib, name, kind, scale, env_size, W, H):
    sc, env, desc, st, cam, k = _setup(lib, kind, scale, env_size, W, H)
    k.render(st, 3)
    d, i = k.readback(abi.REF_DIRECT), k.readback(abi.REF_INDIRECT)
    miss, emit, want = deterministic_pixels(desc, st, cam, W, H)
    assert emit.sum() > 0, "no emitter in view"
    if env_size is not None:
        assert miss.sum() > 0, "no sky in view"
    m = miss | emit
    assert np.array_equal(d[m][:, :3].view(np.uint32), want[m][:, :3].view(np.uint32))
    assert (i[m][:, :3] == 0).all()
    assert (d[~m][:, :3] != want[~m][:, :3]).any()   # the other pixels are estimated, not copied


def test_header_declares_the_reference_entry_points():
    src = open(os.path.join(ROOT, "include", "rt_abi.h")).read()
    for n in ("rt_reference_render", "rt_reference_reset", "rt_reference_samples", "rt_reference_readback", "rt_reference_tonemap"):
        assert re.search(r"\bint " + n + r"\(rt_ctx\* ctx", src), n
    assert re.search(r"#define RT_ABI_VERSION_MINOR (\d+)u", src).group(1) == "4"
    assert "tea(W * y + x, tea(s, 0x52454631))" in src


def test_library_exports_the_reference_entry_points():
    from restir_amd import renderer
    lib = C.CDLL(renderer.HIP_LIB_PATH)
    for n in ("rt_reference_render", "rt_reference_reset", "rt_reference_samples", "rt_reference_readback", "rt_reference_tonemap"):
        assert hasattr(lib, n) and n in renderer.ABI_SYMBOLS
    lib.rt_abi_version.restype = C.c_uint32
    assert lib.rt_abi_version() == (2 << 16) | 4
    # the error convention without a context
    assert lib.rt_reference_reset(None) == -1 and lib.rt_reference_samples(None, None) == -1
