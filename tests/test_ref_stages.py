"""Stage-level pin of the oracle to the REFERENCE'S OWN shader source.

oracle/kat/build_ref_stages.sh compiles shaders/direct_stage.comp, direct_gen.comp, direct_reuse.comp, indirect_stage.comp,
denoise_direct.comp, denoise_indirect.comp, compose.comp — with everything they #include: pathtrace.glsl, env_sampling.glsl,
shade_state.glsl, gltf_material.glsl, pbr_metallicworkflow.glsl, reservoir.glsl, traceray_rq.glsl (ClosestHit / AnyHit / HitTest
as written, over a ray-query stand-in), sun_and_sky.glsl, compress.glsl, random.glsl, common.glsl, denoise_common.glsl — from where
they lie under /root/reference into oracle/_ref/libref_stages.so (authoring container only).  Two kinds of tests:

  * live: the oracle and the compiled reference render the same seeded frames; EVERY screen-space buffer must agree bit for bit —
    G-buffer words, motion vectors, direct and indirect reservoirs, both result images and the four filter temporaries — over
    scenes, RtxState variants, camera motion, HDR / sun & sky / no environment, the 2-pass direct_gen + direct_reuse split and
    the glTF file scene.  Where the library is absent (away from the authoring container) the oracle's buffers are held to the
    SHA-256 of the reference's, stored in tests/golden/ref_live_digests.json (minted by tests/golden/make_ref_live_digests.py);
    where it is present, the stored digests are checked against it too.
  * travelling: tests/golden/ref_stage_vectors.npz holds the per-pixel output of the compiled reference for small seeded frames
    (minted by tests/golden/make_ref_stage_vectors.py); the oracle must reproduce them bit for bit on any machine, and
    tests/test_gpu_ref_vectors.py holds the HIP path to the same file.

Bit-exactness is possible because the GLSL run-time (oracle/kat/glsl_cpu.h) binds what GLSL leaves implementation-defined
(transcendentals, float->int conversion, vector operation order) to this repository's numerics contract; tolerance 0.
Not covered (and listed as unpinned in oracle/README.md): what the reference delegates to the Vulkan driver / nvpro_core —
ray/triangle arithmetic and hit order, instance inverse transforms, texture filtering — which both sides take from orc::Scene;
HitTest's per-candidate seed follows deviation 1 on both sides; ReSTIRState spatial / spatiotemporal (the reference's
in-dispatch neighbour exchange races by construction, deviation 4).
"""
import hashlib
import json
import os
import numpy as np
import pytest
from helpers import abi, host, make_scene, compare_buffers
from oracle import ref_binding
from oracle.binding import Oracle

HERE = os.path.dirname(os.path.abspath(__file__))
VECTORS = os.path.join(HERE, "golden", "ref_stage_vectors.npz")
LIVE_DIGESTS = os.path.join(HERE, "golden", "ref_live_digests.json")


def all_buffers(f):
    cur = f & 1
    return [abi.BUF_GBUFFER0 + cur, abi.BUF_MOTION, abi.BUF_DIRECT_RESV0 + cur, abi.BUF_DIRECT_RESULT0 + cur, abi.BUF_INDIRECT_RESV0 + cur,
            abi.BUF_INDIRECT_RESULT0 + cur, abi.BUF_DENOISE_DIR_A, abi.BUF_DENOISE_DIR_B, abi.BUF_DENOISE_IND_A, abi.BUF_DENOISE_IND_B]


FULL = [(abi.STAGE_DIRECT, 0), (abi.STAGE_INDIRECT, 0)] + [(abi.STAGE_DENOISE_DIRECT, l) for l in range(4)] + \
       [(abi.STAGE_DENOISE_INDIRECT, l) for l in range(5)] + [(abi.STAGE_COMPOSE, 0)]
SPLIT = [(abi.STAGE_DIRECT_GEN, 0), (abi.STAGE_DIRECT_REUSE, 0)] + FULL[1:]


def drive(backends, sc, st, W, H, nframes, moving=False, stages=None, each_frame=None):
    """same camera path / seeds for every backend; each_frame(f) is called after frame f was rendered by all of them"""
    eye, center, up, fov = sc.cameraPose()
    sc.updateCamera(W, H)
    for f in range(nframes):
        st.time = 1000 + f
        if moving:
            sc.setCamera(eye + np.array([0.04 * f, 0.01 * f, -0.03 * f], dtype=np.float32), center, up, fov)
        sc.updateCamera(W, H)
        cam = sc.getCamera()
        for b in backends:
            b.set_camera(cam)
            if stages is None:
                b.render_frame(st, f)
            else:
                for stage, level in stages:
                    b.run_stage(st, f, stage, level)
        if each_frame:
            each_frame(f)


def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).view(np.uint8).tobytes()).hexdigest()


def frame_digests(backend, f):
    """{buffer name: SHA-256 of its bytes} of every screen-space buffer of frame f"""
    return {abi.BUFFER_NAMES[buf]: _sha(backend.readback(buf)) for buf in all_buffers(f)}


needs_ref = pytest.mark.skipif(not ref_binding.available(), reason="oracle/_ref/libref_stages.so is built only where /root/reference exists")

LIVE_CASES = [
    # name, kind, scale, W, H, frames, env, moving
    ("cornell", abi.PROC_CORNELL, 1.0, 64, 64, 4, None, False),
    ("cornell-odd-size", abi.PROC_CORNELL, 1.0, 45, 27, 3, None, True),       # ragged workgroups, odd half resolution
    ("helmet-env", abi.PROC_HELMET, 0.03, 64, 48, 3, (128, 64), True),        # base colour / metal-rough / normal textures, HDR env sampling
    ("sponza-moving", abi.PROC_SPONZA, 0.01, 80, 48, 4, (128, 64), True),     # instancing, emissive mesh, reprojection
    ("bistro-ext", abi.PROC_BISTRO_EXT, 0.002, 80, 48, 3, (128, 64), True),   # alpha-masked foliage through the reference's HitTest
    ("bistro-int", abi.PROC_BISTRO_INT, 0.003, 64, 40, 3, None, True),        # many emissive triangles, punctual lights, no env
]

VARIANTS = ["restir_none", "ris_only", "no_denoise", "no_modulate", "no_mis_depth2", "depth6", "m16_clamp4", "gen_reuse_split", "env_only", "no_env",
            "firefly_tight"] + [f"debug_{m}" for m in range(1, 10)]

# every live case by key: `live/<name>` (LIVE_CASES), `variant/<name>` (VARIANTS), `sun_and_sky`, `gltf_file`
LIVE_KEYS = [f"live/{c[0]}" for c in LIVE_CASES] + [f"variant/{v}" for v in VARIANTS] + ["sun_and_sky", "gltf_file"]


def live_case(key):
    """(scene, env, state, W, H, frames, moving camera, stages or None, sun & sky or None) of a live case"""
    stages, sky = None, None
    if key.startswith("live/"):
        name, kind, scale, W, H, frames, env_size, moving = next(c for c in LIVE_CASES if c[0] == key[5:])
        sc, env = make_scene(kind, scale, 1, env_size)
        st = host.default_state(W, H, sc, env)
        if env is None:
            st.environmentProb = 0.0; st.fireflyClampThreshold = 100.0
        return sc, env, st, W, H, frames, moving, stages, sky
    W, H, frames, moving = 64, 40, 3, True
    if key.startswith("variant/"):
        variant = key[8:]
        sc, env = make_scene(abi.PROC_SPONZA, 0.01, 1, (128, 64))
        st = host.default_state(W, H, sc, env)
        if variant == "restir_none": st.ReSTIRState = abi.RESTIR_NONE
        if variant == "ris_only": st.ReSTIRState = abi.RESTIR_RIS
        if variant == "no_denoise": st.denoise = 0
        if variant == "no_modulate": st.modulate = 0
        if variant == "no_mis_depth2": st.MIS = 0; st.maxDepth = 2
        if variant == "depth6": st.maxDepth = 6
        if variant == "m16_clamp4": st.RISSampleNum = 16; st.reservoirClamp = 4
        if variant == "gen_reuse_split": stages = SPLIT
        if variant == "env_only": st.environmentProb = 1.0
        if variant == "no_env": st.environmentProb = 0.0
        if variant == "firefly_tight": st.fireflyClampThreshold = 0.5
        if variant.startswith("debug_"): st.debugging_mode = int(variant.split("_")[1])
    elif key == "sun_and_sky":
        sc, env = make_scene(abi.PROC_SPONZA, 0.01, 1, None)
        st = host.default_state(W, H, sc, None)
        st.environmentProb = 0.5
        sky = abi.SunAndSky(in_use=1, haze=0.5, sun_disk_scale=3.0, physically_scaled_sun=0, multiplier=0.02)
    elif key == "gltf_file":
        W, H = 80, 48
        sc = host.Scene()
        assert sc.load(os.path.join(HERE, "golden", "mini_scene.gltf"))
        env = host.HdrSampling(); env.makeSyntheticSky(64, 32, 5e3, 7)
        st = host.default_state(W, H, sc, env)
    else:
        raise KeyError(key)
    return sc, env, st, W, H, frames, moving, stages, sky


def make_backend(cls, sc, env, W, H, sky):
    b = cls(); b.upload_scene(sc.desc(env)); b.resize(W, H)
    if sky is not None:
        b.set_sun_and_sky(sky)
    return b


def check_live_case(key):
    """The oracle against the compiled reference when it is built here (every buffer of every frame, word for word, and the stored digests against
    the reference); elsewhere against the reference's stored digests (tests/golden/ref_live_digests.json): bit for bit either way."""
    sc, env, st, W, H, frames, moving, stages, sky = live_case(key)
    with open(LIVE_DIGESTS) as fh:
        want = json.load(fh)[key]
    assert set(want) == {f"f{f}" for f in range(frames)}, f"{key}: tests/golden/ref_live_digests.json does not cover the case's frames"
    o = make_backend(Oracle, sc, env, W, H, sky)
    r = make_backend(ref_binding.Reference, sc, env, W, H, sky) if ref_binding.available() else None
    seen = {"lit": False}
    def check(f):
        if r is not None:
            bad = {k: v for k, v in compare_buffers(o, r, all_buffers(f)).items() if v[0]}
            assert not bad, f"frame {f}: oracle differs from the compiled reference in {bad}"
            stale = [k for k, d in frame_digests(r, f).items() if d != want[f"f{f}"][k]]
            assert not stale, f"{key} frame {f}: tests/golden/ref_live_digests.json is stale in {stale} (tests/golden/make_ref_live_digests.py)"
        else:
            bad = [k for k, d in frame_digests(o, f).items() if d != want[f"f{f}"][k]]
            assert not bad, f"{key} frame {f}: oracle differs from the compiled reference's stored output in {bad}"
        img = o.readback(abi.BUF_DIRECT_RESULT0 + (f & 1)).view(np.float32)
        seen["lit"] |= bool(np.isfinite(img).all() and img.max() > 0.01)
    drive([o] + ([r] if r is not None else []), sc, st, W, H, frames, moving, stages, check)
    assert seen["lit"], "two empty frames compare equal trivially"


@pytest.mark.parametrize("name,kind,scale,W,H,frames,env_size,moving", LIVE_CASES, ids=[c[0] for c in LIVE_CASES])
def test_oracle_equals_compiled_reference(name, kind, scale, W, H, frames, env_size, moving):
    check_live_case(f"live/{name}")


@pytest.mark.parametrize("variant", VARIANTS)
def test_state_variants_equal_compiled_reference(variant):
    check_live_case(f"variant/{variant}")


def test_sun_and_sky_equals_compiled_reference():
    """`_sunAndSky.in_use = 1`: EnvRadiance / EnvSample / EnvEval through the reference's sun_and_sky.glsl as compiled"""
    check_live_case("sun_and_sky")


def test_gltf_file_scene_equals_compiled_reference():
    """Scene::load path: TRS hierarchy, nearest / clamp / mirror samplers, MASK material, transmission + ior, spot light"""
    check_live_case("gltf_file")


# ---- travelling vectors ------------------------------------------------------------------------------------------------------
GOLDEN_CASES = {
    # name: (kind, scale, W, H, frames, env, moving)
    "cornell32": (abi.PROC_CORNELL, 1.0, 32, 32, 3, None, False),
    "textured48x32": (abi.PROC_HELMET, 0.03, 48, 32, 3, (64, 32), True),
    "foliage48x32": (abi.PROC_BISTRO_EXT, 0.002, 48, 32, 3, (64, 32), True),
}


def golden_setup(name):
    kind, scale, W, H, frames, env_size, moving = GOLDEN_CASES[name]
    sc, env = make_scene(kind, scale, 1, env_size)
    st = host.default_state(W, H, sc, env)
    if env is None:
        st.environmentProb = 0.0; st.fireflyClampThreshold = 100.0
    return sc, env, st, W, H, frames, moving


def check_against_vectors(backend_factory, name):
    """render the golden case on `backend` and compare every buffer of every frame with the reference's stored output"""
    assert os.path.exists(VECTORS), "tests/golden/ref_stage_vectors.npz is part of the repository"
    vec = np.load(VECTORS)
    sc, env, st, W, H, frames, moving = golden_setup(name)
    b = backend_factory(sc.desc(env), W, H)
    def check(f):
        for buf in all_buffers(f):
            want = vec[f"{name}/f{f}/{abi.BUFFER_NAMES[buf]}"]
            got = b.readback(buf).view(np.uint32)
            assert got.shape == want.shape, (name, f, abi.BUFFER_NAMES[buf])
            nbad = int((got != want).sum())
            assert nbad == 0, f"{name} frame {f} {abi.BUFFER_NAMES[buf]}: {nbad} of {want.size} words differ from the reference's own output"
    drive([b], sc, st, W, H, frames, moving, None, check)


@pytest.mark.parametrize("name", sorted(GOLDEN_CASES))
def test_oracle_reproduces_reference_vectors(name):
    def mk(desc, W, H):
        o = Oracle(0); o.upload_scene(desc); o.resize(W, H); return o
    check_against_vectors(mk, name)


@needs_ref
@pytest.mark.parametrize("name", sorted(GOLDEN_CASES))
def test_vectors_are_what_the_reference_build_produces(name):
    """the committed file is not stale: the compiled reference still produces it"""
    def mk(desc, W, H):
        r = ref_binding.Reference(); r.upload_scene(desc); r.resize(W, H); return r
    check_against_vectors(mk, name)
