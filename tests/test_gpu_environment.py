"""rt_set_environment on the GPU (include/rt_abi.h "The environment"): the table the device builds equals tests/env_accel_checker.cpp and rt_env_accel
word for word on every map of tests/env.py; a context that swapped its map renders, and traces, what a fresh context of the new map renders, and what the oracle
renders from the same table; the call commutes with rt_update_instances and rt_rebuild_accel; refused calls change nothing; sun & sky still wins.  No tolerance
anywhere.  The scene is the suite's smallest environment-lit one (the Cornell box under a 16 x 8 map) at 64 x 48.  tests/test_environment_cpu.py proves the rule
and the checker without a GPU."""
import numpy as np
import pytest

from helpers import abi, host, frame_buffers
from oracle.binding import Oracle
import env
import optin
import refit
import test_gpu_refit

pytestmark = pytest.mark.gpu

W, H = test_gpu_refit.SIZES[0]
renderer = test_gpu_refit.renderer
MAP0, MAP1 = "16x8_random", "37x19_sun"


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    return env.build(tmp_path_factory.mktemp("env"))


def hdr(name):
    """an HdrSampling of a named map with its own (host) table"""
    h = host.HdrSampling()
    h.setEnvironment(env.make(name))
    return h


def scene():
    return host.Scene().makeProcedural(abi.PROC_CORNELL, 1.0, 1)


def state(sc, e):
    sc.updateCamera(W, H)
    return host.default_state(W, H, sc, e)


def render(r, sc, st, frames, first=0):
    """frames [first, first + frames) on a renderer or an oracle: [{buffer: bytes}]"""
    out = []
    for f in range(first, first + frames):
        st.time = 1000 + f
        r.set_camera(sc.getCamera())
        (r.run if hasattr(r, "run") else r.render_frame)(st, f)
        out.append({b: r.readback(b).copy() for b in frame_buffers(f)})
    return out


def diff(a, b):
    return {(f, abi.BUFFER_NAMES[k]): optin.words(x[k], y[k]) for f, (x, y) in enumerate(zip(a, b)) for k in x if optin.words(x[k], y[k])}


def in_use(r):
    return r.environment_readback(abi.ENV_TEXELS).copy(), r.environment_readback(abi.ENV_ACCEL).copy()


@pytest.fixture(scope="module")
def ctx():
    """one context of the scene under MAP0 for the table tests"""
    sc, e0 = scene(), hdr(MAP0)      # (a description points into its scene and its HdrSampling: both live until the upload is done)
    r = renderer(sc.desc(e0), W, H)
    yield r
    r.destroy()


class Fresh:
    """what a context that never saw another map gives for (MAP1, the device's table of MAP1), by scene variant: frames 0..2 and a batch of rays, rendered once"""
    cache = {}

    @classmethod
    def get(cls, moved):
        if moved not in cls.cache:
            sc = scene()
            if moved:
                sc.updateInstances(*move())
            e0, e1 = hdr(MAP0), host.HdrSampling()
            donor = renderer(sc.desc(e0))
            e1.setEnvironment(env.make(MAP1), donor)      # the host class forwards to the device and adopts its table
            donor.destroy()
            st = state(sc, e1)
            r = renderer(sc.desc(e1), W, H)
            rays = refit.make_rays(sc.desc(), [3], 256, 5)
            cls.cache[moved] = dict(frames=render(r, sc, st, 3), closest=r.trace_closest(rays), any=r.trace_any(rays), rays=rays, env=e1, table=e1.accel().copy())
            r.destroy()
        return cls.cache[moved]


def move():
    """the short box slides: (ids, 3 x 4 matrices) for rt_update_instances and Scene.updateInstances"""
    sc = scene()
    return [3], refit.compose(refit.translation([0.05, 0.0, -0.04]), refit.instances_of(sc.desc())["objectToWorld"][3]).reshape(1, 12)


# ---- 1. the device build -------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(env.MAPS))
def test_the_device_table_equals_the_checker_and_rt_env_accel_word_for_word(lib, ctx, name):
    from restir_amd.renderer import Renderer
    a = env.make(name)
    ctx.set_environment(a)
    texels, table = in_use(ctx)
    st = ctx.environment_stats()
    want, wi, wa, small = env.check(lib, name)
    mine, hi, ha = Renderer.env_accel(a)
    print(name, "ms", round(st.ms, 3), "smalls", st.numSmall, "larges", st.numLarge, "integral", st.integral)
    assert np.array_equal(texels.view(np.uint32), a.view(np.uint32))
    assert np.array_equal(env.words(table), env.words(want)) and np.array_equal(env.words(table), env.words(mine))
    assert env.f32_words(st.integral) == env.f32_words(wi) == env.f32_words(hi) and env.f32_words(st.average) == env.f32_words(wa) == env.f32_words(ha)
    assert (st.width, st.height, st.numSmall, st.numLarge, st.builtOnDevice) == (a.shape[1], a.shape[0], small, len(want) - small, 1)


def test_a_repeated_call_gives_identical_bytes_and_allocates_nothing(ctx):
    a = env.make("257x129_sun")
    ctx.set_environment(a)
    ctx.set_environment(a)                      # both pairs have held the map
    first, held = in_use(ctx), ctx.environment_stats().deviceBytes
    for _ in range(3):
        ctx.set_environment(a)
        again = in_use(ctx)
        assert np.array_equal(first[0].view(np.uint32), again[0].view(np.uint32)) and np.array_equal(env.words(first[1]), env.words(again[1]))
        assert ctx.environment_stats().deviceBytes == held
    n = a.shape[0] * a.shape[1]
    assert held >= (2 * 32 + 28) * n      # two pairs of 16 + 16 B per texel, 8 + 16 + 4 B of work arrays


def test_the_size_may_change_and_change_back(lib, ctx):
    for name in ("16x8_random", "64x32_ramp", "16x8_random", "64x32_lower_black", "1x1", "16x8_random"):
        ctx.set_environment(env.make(name))
        texels, table = in_use(ctx)
        assert texels.shape == env.make(name).shape and np.array_equal(env.words(table), env.words(env.check(lib, name)[0])), name
    held = ctx.environment_stats().deviceBytes
    ctx.set_environment(env.make("64x32_ramp"))
    ctx.set_environment(env.make("16x8_random"))
    assert ctx.environment_stats().deviceBytes == held      # every pair has held the largest map: nothing grows


def test_an_empty_map_is_the_black_texel(ctx):
    from restir_amd.renderer import hip_lib
    some = env.make("5x3")
    for w, h, texels in ((0, 5, some), (5, 0, some), (5, 3, None)):
        assert hip_lib().rt_set_environment(ctx._h, w, h, texels.ctypes.data if texels is not None else None, None) == 0
        texels, table = in_use(ctx)
        assert texels.shape == (1, 1, 4) and not texels.any()
        assert (int(table["alias"][0]), float(table["q"][0]), float(table["pdf"][0]), float(table["aliasPdf"][0])) == (0, 1.0, 0.0, 0.0)
        ctx.set_environment(some)


# ---- 2. against a fresh context and the oracle ---------------------------------------------------------------------------------------------------------------------
def test_a_swap_before_rendering_equals_a_fresh_context_and_the_oracle():
    want = Fresh.get(False)
    sc = scene()
    e0 = hdr(MAP0)
    a = renderer(sc.desc(e0), W, H)
    e1 = host.HdrSampling()
    e1.setEnvironment(env.make(MAP1), a)
    assert np.array_equal(env.words(e1.accel()), env.words(want["table"])) and e1.getIntegral() == want["env"].getIntegral() != e0.getIntegral()
    st = state(sc, e1)
    frames = render(a, sc, st, 3)
    assert diff(frames, want["frames"]) == {}
    assert np.array_equal(a.trace_closest(want["rays"]).view(np.uint32), want["closest"].view(np.uint32)) and np.array_equal(a.trace_any(want["rays"]), want["any"])
    a.destroy()
    o = Oracle(0)
    o.upload_scene(sc.desc(e1))
    o.resize(W, H)
    assert diff(frames, render(o, sc, st, 3)) == {}
    # the frames depend on the map: the same context under MAP0 renders something else
    b = renderer(sc.desc(e0), W, H)
    other = render(b, sc, state(sc, e0), 1)
    b.destroy()
    assert optin.words(other[0][abi.BUF_DIRECT_RESULT0], frames[0][abi.BUF_DIRECT_RESULT0]) > 0


def test_a_swap_mid_stream_equals_the_copy_path_twin():
    sc = scene()
    e0 = hdr(MAP0)
    st0 = state(sc, e0)
    a, b = renderer(sc.desc(e0), W, H), renderer(sc.desc(e0), W, H)
    assert diff(render(a, sc, st0, 2), render(b, sc, st0, 2)) == {}
    e1 = host.HdrSampling()
    e1.setEnvironment(env.make(MAP1), a)                       # A builds on the device
    b.set_environment(env.make(MAP1), e1.accel())              # B copies A's table
    assert b.environment_stats().builtOnDevice == 0 and a.environment_stats().builtOnDevice == 1
    assert all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(in_use(a), in_use(b)))
    st1 = state(sc, e1)
    fa, fb = render(a, sc, st1, 3, first=2), render(b, sc, st1, 3, first=2)
    a.destroy(); b.destroy()
    assert diff(fa, fb) == {}
    # ... and the swap shows: the oracle that keeps MAP0 renders other frames from the same history
    o = Oracle(0)
    o.upload_scene(sc.desc(e0))
    o.resize(W, H)
    keep = render(o, sc, st0, 5)
    assert optin.words(keep[2][abi.BUF_DIRECT_RESULT0], fa[0][abi.BUF_DIRECT_RESULT0]) > 0


# ---- 3. pairs with the other edits -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", ["env,move", "move,env", "env,rebuild", "rebuild,env", "move,rebuild,env", "env,move,rebuild"])
def test_the_call_commutes_with_instance_moves_and_rebuilds(order):
    ops = order.split(",")
    want = Fresh.get("move" in ops)
    sc, e0 = scene(), hdr(MAP0)
    r = renderer(sc.desc(e0), W, H)
    for op in ops:
        if op == "env":
            r.set_environment(env.make(MAP1))
        elif op == "move":
            r.update_instances(*move())
            sc.updateInstances(*move())
        else:
            r.rebuild_accel()
    assert np.array_equal(env.words(r.environment_readback(abi.ENV_ACCEL)), env.words(want["table"]))
    st = state(sc, want["env"])
    frames = render(r, sc, st, 2)
    closest, any_hit = r.trace_closest(want["rays"]), r.trace_any(want["rays"])
    r.destroy()
    assert diff(frames, want["frames"][:2]) == {}
    assert np.array_equal(closest.view(np.uint32), want["closest"].view(np.uint32)) and np.array_equal(any_hit, want["any"])


# ---- 4. rejected and neutral calls -----------------------------------------------------------------------------------------------------------------------------------
def test_every_refusal_leaves_the_environment_as_it_was():
    from restir_amd.renderer import Renderer, hip_lib
    L = hip_lib()
    empty = Renderer().setup(0)
    assert L.rt_set_environment(empty._h, 5, 3, env.make("5x3").ctypes.data, None) == -4      # RT_ERR_NO_SCENE
    empty.destroy()
    sc = scene()
    e0 = hdr(MAP0)
    r = renderer(sc.desc(e0), W, H)
    good = env.make("16x8_random")
    for a in (good, good, env.make("5x3")):      # both pairs and the work arrays have held 16 x 8: a refused build allocates nothing either
        r.set_environment(a)
    before, stats = in_use(r), bytes(r.environment_stats())
    table = Renderer.env_accel(good)[0].copy()
    bad_alias = table.copy(); bad_alias["alias"][77] = 128
    neg_alias = table.copy(); neg_alias["alias"][0] = -1
    inf = env.make(env.REFUSED)
    overflow = np.array(env.make("1x1")); overflow[0, 0, :3] = np.float32(3e38)
    refusals = {
        "negative width": lambda: L.rt_set_environment(r._h, -1, 8, good.ctypes.data, None),
        "negative height": lambda: L.rt_set_environment(r._h, 16, -8, good.ctypes.data, table.ctypes.data),
        "more than 2^23 texels for the device": lambda: L.rt_set_environment(r._h, 4096, 2049, good.ctypes.data, None),      # (refused before a texel is read)
        "alias past the table": lambda: L.rt_set_environment(r._h, 16, 8, good.ctypes.data, bad_alias.ctypes.data),
        "negative alias": lambda: L.rt_set_environment(r._h, 16, 8, good.ctypes.data, neg_alias.ctypes.data),
        "+inf on the copy path": lambda: L.rt_set_environment(r._h, 16, 8, inf.ctypes.data, table.ctypes.data),
        "+inf on the device path": lambda: L.rt_set_environment(r._h, 16, 8, inf.ctypes.data, None),
        "importance overflow on the device path": lambda: L.rt_set_environment(r._h, 1, 1, overflow.ctypes.data, None),
    }
    for why, call in refusals.items():
        assert call() == -1, why
        assert L.rt_last_error(r._h).decode().startswith("rt_set_environment"), why
        now = in_use(r)
        assert all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(before, now)) and bytes(r.environment_stats()) == stats, why
    assert L.rt_environment_readback(r._h, 2, before[0].ctypes.data, before[0].nbytes) == -1 and L.rt_environment_readback(r._h, 0, before[0].ctypes.data, 16) == -1
    # ... and the context still works: the refused +inf build ran in the staging pair only
    r.set_environment(env.make(MAP1))
    e1 = Fresh.get(False)["env"]
    frames = render(r, sc, state(sc, e1), 1)
    r.destroy()
    assert diff(frames, Fresh.get(False)["frames"][:1]) == {}


def test_sun_and_sky_in_use_hides_the_new_map_until_it_is_switched_off():
    sc = scene()
    e0 = hdr(MAP0)
    sky = abi.SunAndSky(in_use=1)
    a, b = renderer(sc.desc(e0), W, H), renderer(sc.desc(e0), W, H)
    a.set_sun_and_sky(sky); b.set_sun_and_sky(sky)
    a.set_environment(env.make(MAP1))                          # stored, not seen
    e1 = Fresh.get(False)["env"]
    st = state(sc, e1)
    assert diff(render(a, sc, st, 1), render(b, sc, st, 1)) == {}
    b.destroy()
    off = abi.SunAndSky(in_use=0)
    a.set_sun_and_sky(off)
    c = renderer(sc.desc(e1), W, H)
    c.set_sun_and_sky(sky)
    render(c, sc, st, 1)                                       # the same history: one frame under the sky
    c.set_sun_and_sky(off)
    fa, fc = render(a, sc, st, 2, first=1), render(c, sc, st, 2, first=1)
    a.destroy(); c.destroy()
    assert diff(fa, fc) == {}
