"""The environment's importance table without a GPU (include/rt_abi.h "The environment"): rt_env_accel — the host statement of the rule of
csrc/env_accel.h — against the sequential restatement tests/env_accel_checker.cpp word for word on every map of tests/env.py; the table's own properties (range,
implied probabilities, integral); its inputs against HdrSampling's; the refusals; the host class that adopts a context's table; the struct sizes; and the rule
with the checker under AddressSanitizer + UndefinedBehaviorSanitizer in a program of its own.  tests/test_gpu_environment.py holds the HIP kernels to the same
words."""
import ctypes as C
import os
import subprocess
import numpy as np
import pytest

from helpers import abi, host, ROOT
import env


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    return env.build(tmp_path_factory.mktemp("env"))


def host_rule(name):
    from restir_amd.renderer import Renderer
    return Renderer.env_accel(env.make(name))


@pytest.mark.parametrize("name", list(env.MAPS))
def test_rt_env_accel_equals_the_checker_word_for_word(lib, name):
    table, integral, average = host_rule(name)
    want, wi, wa, small = env.check(lib, name)
    assert np.array_equal(env.words(table), env.words(want))
    assert env.f32_words(integral) == env.f32_words(wi) and env.f32_words(average) == env.f32_words(wa)
    print(name, "smalls", small, "larges", len(want) - small, "integral", integral, "average", average)


def test_the_maps_are_what_they_are_for(lib):
    small = {name: env.check(lib, name)[3] for name in env.MAPS}
    n = {name: env.make(name).shape[0] * env.make(name).shape[1] for name in env.MAPS}
    assert small["64x1_equal"] == 0 and small["8x4_black"] == 0 and small["1x1"] == 0 and small["2x1"] == 1
    assert 0.15 <= 1 - small["16x8_random"] / n["16x8_random"] <= 0.35      # about a quarter large
    assert n["37x19_sun"] - small["37x19_sun"] == 2                        # two larges, a long run of smalls each
    t = env.check(lib, "37x19_sun")[0]
    assert min(np.bincount(t["alias"], minlength=len(t))[[19 // 2 * 37 + 37 // 2, 19 // 2 * 37 + 37 // 2 + 1]]) > 100
    t = env.check(lib, "64x32_lower_black")[0]
    assert (t["q"][32 * 16 * 2:] == 0).all() and (t["pdf"][32 * 16 * 2:] == 0).all()      # W = 0: q = 0
    t = env.check(lib, "64x32_ramp")[0]
    cascade = (t["q"] < 1) & (t["alias"] != np.arange(len(t))) & (np.bincount(t["alias"], minlength=len(t)) > 0)
    assert cascade.sum() > 100                                             # exhausted larges that hand on to the next large
    assert n["257x129_sun"] == 33153 and n["257x129_sun"] > 32 * 1024 and 257 % 1024 != 0      # several scan tiles of 1024, a boundary inside a row
    t = env.check(lib, "8x4_black")
    assert np.array_equal(t[0]["alias"], np.arange(32)) and (t[0]["q"] == 1).all() and not t[0]["pdf"].any() and not t[0]["aliasPdf"].any() and t[1] == 0 and t[2] == 0
    a = env.make("16x8_nan_negative")
    imp = env.importance(lib, a)
    assert imp[2, 3] == 0 and imp[5, 9] == 0 and imp[6, 1] > 0 and np.isfinite(imp).all()
    assert env.check(lib, env.REFUSED) is None


@pytest.mark.parametrize("name", list(env.MAPS))
def test_every_alias_is_in_range_and_every_q_in_the_unit_interval(name):
    table, _, _ = host_rule(name)
    assert ((table["alias"] >= 0) & (table["alias"] < len(table))).all()
    assert ((table["q"] >= 0) & (table["q"] <= 1)).all()
    assert np.array_equal(table["aliasPdf"].view(np.uint32), table["pdf"][table["alias"]].view(np.uint32))


@pytest.mark.parametrize("name", [m for m in env.MAPS if m != "8x4_black"])
def test_the_implied_probabilities_are_the_quantised_weights(lib, name):
    """p_i = (q_i + sum over k with alias_k = i of (1 - q_k)) / n against W_i / T, within 1e-6 / n.

    q is a multiple of 2^-24 and what a texel gives away is the difference of two rounded marks of a cumulative sum, so the shares one large collects telescope:
    the error is at most one grid step (6e-8 / n) however many smalls alias to it — the sun of 257x129_sun is the alias of 19 486.  Measured (max
    |p_i - W_i / T| x n): between 2.5e-8 and 5.9e-8 on every map, 0 on the one-texel and the all-equal map.  (With q rounded per texel, as
    float(double(n W) / double(T)), that map measured 2.5e-6: the roundings of the sun's smalls added up like a random walk.)"""
    table, _, _ = host_rule(name)
    W, T = env.weights(lib, env.make(name))
    n = len(table)
    err = np.abs(env.implied_probabilities(table) - W.astype(np.float64) / T).max()
    print(name, "max |p - W/T| x n = %.3g" % (err * n))
    assert err <= 1e-6 / n


@pytest.mark.parametrize("name", list(env.MAPS))
def test_the_integral_is_the_float64_sum_of_the_importances(lib, name):
    _, integral, _ = host_rule(name)
    ref = env.importance(lib, env.make(name)).astype(np.float64).sum()
    print(name, integral, ref)
    assert abs(integral - ref) <= 2.0 ** -16 * ref


@pytest.mark.parametrize("name", list(env.MAPS))
def test_importances_equal_hdr_samplings_bit_for_bit(name):
    """step 1 against HdrSampling::createEnvironmentAccel's own expressions; where HdrSampling's importance is negative or NaN the rule counts 0"""
    from restir_amd.renderer import Renderer
    a = env.make(name)
    h = host.HdrSampling()
    h.setEnvironment(a)
    theirs = h.importance()
    want = np.where(theirs > 0, theirs, np.float32(0))
    assert np.array_equal(Renderer.env_importance(a).view(np.uint32), want.view(np.uint32))
    if "nan" not in name:
        assert np.array_equal(theirs.view(np.uint32), want.view(np.uint32))      # nothing was clamped on the ordinary maps


@pytest.mark.parametrize("name", [m for m in env.MAPS if "nan" not in m and "black" not in m.split("_")[-1]])
def test_pdf_is_hdr_samplings_with_the_same_integral(name):
    """HdrSampling: pdf = max(r, g, b) * (1.0f / integral) in fp32"""
    table, integral, _ = host_rule(name)
    mx = env.make(name)[..., :3].max(axis=2).reshape(-1)
    want = mx * (np.float32(1) / np.float32(integral))
    assert want.dtype == np.float32 and np.array_equal(table["pdf"].view(np.uint32), want.view(np.uint32))


def test_the_average_is_the_mean_luminance(lib):
    for name in env.MAPS:
        a = env.make(name).astype(np.float64)
        lum = a[..., 0] * np.float64(np.float32(0.2126)) + a[..., 1] * np.float64(np.float32(0.7152)) + a[..., 2] * np.float64(np.float32(0.0722))
        ref = np.where(lum > 0, lum, 0).mean()
        _, _, average = host_rule(name)
        assert abs(average - ref) <= 2.0 ** -16 * ref + 1e-12, name      # fp32 luminance per texel, the quantisation, one fp32 rounding


def test_rt_env_accel_refuses_bad_arguments_and_the_inf_map():
    from restir_amd.renderer import hip_lib
    L = hip_lib()
    a = np.array(env.make("5x3"))
    out = np.full(15, 7, abi.IMPT_SAMP_DT)
    before = out.copy()
    assert L.rt_env_accel(5, 3, None, out.ctypes.data, None, None) == -1 and L.rt_env_accel(5, 3, a.ctypes.data, None, None, None) == -1
    assert L.rt_env_accel(0, 3, a.ctypes.data, out.ctypes.data, None, None) == -1 and L.rt_env_accel(5, -3, a.ctypes.data, out.ctypes.data, None, None) == -1
    assert L.rt_env_accel(4096, 2049, a.ctypes.data, out.ctypes.data, None, None) == -1      # more than 2^23 texels: refused before anything is read
    bad = env.make(env.REFUSED)
    big = np.full(bad.shape[0] * bad.shape[1], 7, abi.IMPT_SAMP_DT)
    assert L.rt_env_accel(bad.shape[1], bad.shape[0], bad.ctypes.data, big.ctypes.data, None, None) == -1 and (big == big[0]).all()
    assert np.array_equal(out, before)
    overflow = np.array(env.make("1x1"))      # finite texels whose importance overflows: the area of a 1 x 1 map is 4 pi
    overflow[0, 0, :3] = np.float32(3e38)
    assert L.rt_env_accel(1, 1, overflow.ctypes.data, out.ctypes.data, None, None) == -1
    assert L.rt_env_accel(5, 3, a.ctypes.data, out.ctypes.data, None, None) == 0 and not np.array_equal(out, before)


class TableOnly:
    """stands in for a renderer.Renderer: what HdrSampling.setEnvironment(rgba, renderer) asks of one, answered by rt_env_accel"""
    def set_environment(self, rgba):
        from restir_amd.renderer import Renderer
        self.table, integral, average = Renderer.env_accel(rgba)
        self.stats = abi.EnvironmentStats(width=rgba.shape[1], height=rgba.shape[0], integral=integral, average=average)
    def environment_stats(self): return self.stats
    def environment_readback(self, which): return self.table


def test_the_host_class_adopts_the_contexts_table():
    a = env.make("16x8_random")
    h = host.HdrSampling()
    h.setEnvironment(env.make("5x3"))
    own = h.getIntegral()
    r = TableOnly()
    h.setEnvironment(a, r)
    assert h.size == (16, 8) and np.array_equal(env.words(h.accel()), env.words(r.table))
    assert h.getIntegral() == r.stats.integral != own and h.getAverage() == r.stats.average
    d = host.Scene().makeProcedural(abi.PROC_CORNELL).desc(h)      # the description carries the adopted table
    got = np.frombuffer((C.c_char * (128 * 16)).from_address(d.envAccel), dtype=abi.IMPT_SAMP_DT)
    assert (d.envWidth, d.envHeight) == (16, 8) and np.array_equal(env.words(got), env.words(r.table))


def test_struct_sizes_and_the_header():
    assert C.sizeof(abi.EnvironmentStats) == 40 and abi.IMPT_SAMP_DT.itemsize == 16 and (abi.ENV_TEXELS, abi.ENV_ACCEL) == (0, 1)
    header = open(os.path.join(ROOT, "include", "rt_abi.h")).read()
    assert "RT_ENV_TEXELS = 0, RT_ENV_ACCEL = 1" in header and "sizeof(rt_environment_stats) == 40" in header
    for name in ("rt_set_environment", "rt_environment_readback", "rt_get_environment_stats", "rt_env_accel", "rt_env_importance"):
        assert ("int %s(" % name) in header
    import re
    assert re.search(r"#define RT_ABI_VERSION_MINOR (\d+)u", header).group(1) == "4"      # an addition that changes no existing call
    from restir_amd.renderer import hip_lib, ABI_SYMBOLS
    assert all(hasattr(hip_lib(), s) for s in ABI_SYMBOLS)


def test_the_rule_and_the_checker_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / "env_san")
    flags = ["-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-fsanitize=address,undefined", "-fsanitize=float-cast-overflow",
             "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-Wall"]
    subprocess.check_call([os.environ.get("CXX", "g++")] + flags + [os.path.join(ROOT, "tests", "env_san_main.cpp"), env.SRC, "-o", exe])
    files = []
    for name in env.ALL:
        a = env.make(name)
        files.append(str(tmp_path / (name + ".bin")))
        with open(files[-1], "wb") as f:
            f.write(np.int32([a.shape[1], a.shape[0]]).tobytes() + a.tobytes())
    p = subprocess.run([exe] + files, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "ok maps %d refused 1" % len(env.ALL) in p.stdout
