"""The opt-in passes on the MI355X at the image sizes where tile kernels go wrong: the reference path tracer (csrc/reference.hip), SVGF (csrc/svgf.hip), GI spatial
reuse (csrc/gi_spatial.hip) and the TAA resolve (csrc/taa.hip), each alone and SVGF + GI spatial + TAA together, against the oracle chained with their CPU
checkers (tests/optin.py), every buffer word for word.  tests/test_optin_shapes_cpu.py holds the checkers to their float64 models at odd sizes.

What each group reaches that the per-pass modules (multiples of 8 / 16, fewer than 24 tile rows, one reference band) do not:
  ragged      the ragged-tile guards (`p.x >= A.W || p.y >= A.H`, svgfPixel's `r.valid`, `px.x >= indSize.x`, `px.x >= st.size.x || px.y >= rowEnd`) and odd W / H
              under a half-resolution grid (stride W / 2 against stride W, G-buffer at 2p, motion(2p) >> 1)
  stripes     the second regime of the XCD-striped tile order (tileChunk: whole tile rows per XCD from 24 tile rows on) and its `tile.valid == false` tail
  bands       rt_reference_render's row-band loop: r0 > 0, a last band that is no multiple of 8 rows, refN + s across two calls
  tiny        sizes below one tile (half-resolution grid 0 x 0 ... 4 x 4), the base frame included; one child process per size
  sweep       a seeded random sweep over scene, size, environment, ReSTIRState, depth, denoise, debug view, traversal build, schedule, subset of passes, their
              parameters over the whole accepted range, and the events with reset rules (RESTIR_OPTIN_CASES configurations, default 48, seed RESTIR_OPTIN_SEED, default 1;
              `python tests/test_gpu_optin_shapes.py CASES SEED [FIRST]` runs a long sweep by hand)

Wall time on one MI355X host, same visit: `pytest -m gpu` without this module 235 s, this module 45 s (19 %; the budget was a third).  Chosen from that: 48 sweep
cases (14 s; 0.3 s per case), the reference band case at the full 4096 x 267 (under 2 s, the wide Cornell view is mostly sky).  DESIGN.md §17 has the summary."""
import json
import os
import subprocess
import sys
import numpy as np
import pytest
from helpers import abi
import optin
import refpt
import svgf
import gi_spatial
import taa

pytestmark = pytest.mark.gpu

SPONZA = (abi.PROC_SPONZA, 0.01, (64, 32))
CORNELL = (abi.PROC_CORNELL, 1.0, None)
# W, H: what the size hits
RAGGED = [
    (101, 51),   # ragged in both directions at full resolution (13 x 7 tiles, 5 / 3 live columns / rows in the last) and at half resolution (50 x 25); odd W and H
    (67, 45),    # odd W and H, half resolution 33 x 22: one live column in the last half-res tile column
    (33, 17),    # half resolution 16 x 8 is whole tiles, full resolution is ragged: one ragged grid only
]
STRIPES = [
    (123, 187),  # 24 full-resolution tile rows (187 = 23 * 8 + 3), exactly the first size of the regime (`tilesY < 24` fails): SVGF direct, TAA and the stages
                 # deal whole tile rows per XCD; half resolution (61 x 93, 12 tile rows) stays in chunks of 8.  24 rows are 3 per XCD: no workgroup without a tile.
    (83, 391),   # half resolution 41 x 195: 25 half-res tile rows (195 = 24 * 8 + 3), so the indirect SVGF chain and k_gi_spatial cross over too, and both grids
                 # (full resolution: 49 tile rows) have a `tile.valid == false` tail, which the regime has whenever tilesY is no multiple of 8.  (83 x 379, half
                 # resolution 24 tile rows, has none.)
]
TINY = [(1, 1), (2, 3), (7, 5), (9, 9), (16, 1), (1, 16)]   # half resolution 0x0, 1x1, 3x2, 4x4, 8x0, 0x8
SUBSETS = ["svgf", "gi_spatial", "taa", "all"]
N = 5
CUT = 3    # the camera turns round before this frame: most of every history is rejected


@pytest.fixture(scope="module")
def tmp(tmp_path_factory):
    return tmp_path_factory.mktemp("optin")


def settings(which):
    """(denoiser, GI spatial, TAA) of a named subset; None = the pass stays off"""
    on = {"svgf", "gi_spatial", "taa"} if which == "all" else {which}
    return (abi.Denoiser(mode=abi.DENOISER_SVGF) if "svgf" in on else None,
            abi.GiSpatial(mode=abi.GI_SPATIAL_VISIBILITY, samples=6, radius=6) if "gi_spatial" in on else None,
            abi.Taa(mode=abi.TAA_ON) if "taa" in on else None)


def run_case(tmp, scene, W, H, which, overlap=0, frames=N, cut=CUT, live=True):
    """`frames` frames of a moving camera with one cut, compared after every frame; returns {pass: (pixels that accepted history, pixels that rejected it)}"""
    den, gis, t = settings(which) if which else (None, None, None)
    rig = optin.Rig(tmp, *scene, W, H, den=den, gis=gis, t=t, overlap=overlap)
    seen = {}
    taps = 0
    try:
        for f in range(frames):
            rig.frame(f, rig.camera(f, cut=cut))
            bad = rig.diff(f)
            print(json.dumps(dict(W=W, H=H, passes=which, overlap=overlap, frame=f, differing=bad)), flush=True)
            assert not bad, f"{W}x{H} {which} overlap {overlap} frame {f}: {bad}"
            if f > 0:
                for name, n in rig.history_lengths().items():
                    a, r = seen.get(name, (0, 0))
                    seen[name] = (a + int((n > 1).sum()), r + int((n == 1).sum()))
            if gis is not None:
                taps += int(rig.gis_taps.sum())
    finally:
        rig.destroy()
    if live:   # a comparison of two empty histories proves nothing
        for name, (a, r) in seen.items():
            assert a > 0 and r > 0, (name, a, r)
        assert gis is None or taps > 0
    return seen


@pytest.mark.parametrize("which", SUBSETS)
@pytest.mark.parametrize("W,H", RAGGED, ids=lambda v: str(v))
def test_ragged_tiles_and_odd_half_resolution(tmp, W, H, which):
    """the ragged-tile guards and odd W or H with a half-resolution grid: every pass alone, and all three together"""
    assert W % 8 and H % 8 and W % 2 and H % 2                      # masked lanes at full resolution; 2 * (W / 2) != W
    assert (W // 2) % 8 or (H // 2) % 8 or (W, H) == (33, 17)       # ... and at half resolution, except in the case that is there for one ragged grid only
    run_case(tmp, SPONZA, W, H, which)


@pytest.mark.parametrize("overlap", [1, 2, 3])
def test_every_schedule_at_a_ragged_size(tmp, overlap):
    """rt_set_overlap 1, 2, 3 (0 is the case above) with all three passes at 101 x 51"""
    run_case(tmp, SPONZA, 101, 51, "all", overlap=overlap)


@pytest.mark.parametrize("which", SUBSETS)
@pytest.mark.parametrize("W,H", STRIPES, ids=lambda v: str(v))
def test_stripe_regime_of_the_tile_order(tmp, W, H, which):
    """the XCD-striped tile order from 24 tile rows on (tileChunk deals whole tile rows), with ragged edges and a `tile.valid == false` tail"""
    full, half = (optin.tiles(W), optin.tiles(H)), (optin.tiles(W // 2), optin.tiles(H // 2))
    for tx, ty in (full, half) if (W, H) != STRIPES[0] else (full,):
        assert ty >= optin.TILE_SMALL_ROWS and optin.tile_chunk(tx, ty) == tx != optin.TILE_SMALL_CHUNK     # really the stripe regime ...
        assert (optin.tile_grid(tx, ty) > tx * ty) == ((W, H) != STRIPES[0])                                 # ... with workgroups that own no tile
    assert W % 8 and H % 8 and (W // 2) % 8 and (H // 2) % 8
    run_case(tmp, SPONZA, W, H, which, frames=4, cut=2)


# ---- reference mode
def _reference(tmp, scene, W, H, splits, max_depth):
    from restir_amd.renderer import Renderer
    from helpers import host, make_scene
    sc, env = make_scene(scene[0], scene[1], 1, scene[2])
    st = host.default_state(W, H, sc, env)
    if env is None:
        st.environmentProb = 0.0
    st.maxDepth = max_depth
    desc = sc.desc(env)
    r = Renderer().setup(0)
    r.load_scene(desc)
    r.update(W, H)
    k = refpt.RefChecker(refpt.build(tmp), desc)
    k.resize(W, H)
    sc.updateCamera(W, H)
    cam = sc.getCamera()
    r.set_camera(cam)
    k.set_camera(cam)
    total = 0
    for n in splits:
        r.reference_render(st, n)
        k.render(st, n, threads=16)
        total += n
        assert r.reference_samples() == total == k.samples()
        got, want = [r.reference_readback(c) for c in range(3)], [k.readback(c) for c in range(3)]
        bad = [optin.words(a, b) for a, b in zip(got, want)]
        print(json.dumps(dict(W=W, H=H, samples=total, differing=bad)), flush=True)
        assert bad == [0, 0, 0], f"{W}x{H} after {total} samples: differing words (direct, indirect, sum) {bad}"
    assert np.isfinite(got[2]).all() and got[0][..., :3].max() > 0 and got[1][..., :3].max() > 0
    r.destroy()


@pytest.mark.parametrize("W,H", RAGGED, ids=lambda v: str(v))
def test_reference_at_ragged_sizes(tmp, W, H):
    """k_reference's guard `px.x >= st.size.x || px.y >= rowEnd` with masked lanes in both directions; 2 + 1 samples"""
    assert W % 8 and H % 8 and optin.ref_band_rows(W) >= H           # one band: the ragged last tile row is the band's
    _reference(tmp, SPONZA, W, H, (2, 1), 3)


def test_reference_row_bands(tmp):
    """rt_reference_render cuts the image into bands of max(8, (2^20 / W) & ~7) rows: 4096 x 267 is rows 0..255 and 256..266 (r0 > 0, a last band of 11 rows),
    one sample, then one more in a second call (refN + s), compared with the band-less CPU statement after each call"""
    W, H = 4096, 267
    band = optin.ref_band_rows(W)
    assert band == 256 and -(-H // band) == 2 and (H - band) % 8 != 0
    _reference(tmp, CORNELL, W, H, (1, 1), 2)


# ---- below one tile: one child process per size
def tiny_child(W, H):
    """the base frame, every pass alone and all three together at W x H; exit status 0 when every word matches"""
    svgf.load(os.environ["RESTIR_OPTIN_SVGF"]); gi_spatial.load(os.environ["RESTIR_OPTIN_GIS"]); taa.load(os.environ["RESTIR_OPTIN_TAA"])
    for which in [None] + SUBSETS:
        for overlap in (0, 2):
            run_case(None, CORNELL, W, H, which, overlap=overlap, frames=4, cut=None, live=False)
    print("tiny ok", W, H, flush=True)
    return 0


@pytest.mark.parametrize("W,H", TINY, ids=lambda v: str(v))
def test_below_one_tile(tmp, W, H):
    """rt_resize accepts 1..32767: sizes below one 8 x 8 tile (W / 2 == 0 at 1 x 1, 1 x 16; H / 2 == 0 at 16 x 1) render and match — the base frame, every pass
    alone, all three together, serial and with frames in flight.  A child process of its own per size, with its own time limit."""
    assert optin.tiles(W // 2) * optin.tiles(H // 2) <= 1 and (W // 2 == 0 or H // 2 == 0 or min(W, H) < 8 or (W, H) == (9, 9))
    env = dict(os.environ, RESTIR_OPTIN_SVGF=svgf.build(tmp) and svgf.lib_path, RESTIR_OPTIN_GIS=gi_spatial.build(tmp) and gi_spatial.lib_path,
               RESTIR_OPTIN_TAA=taa.build(tmp) and taa.lib_path)
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--tiny", str(W), str(H)], env=env, cwd=os.path.dirname(os.path.abspath(__file__)),
                         capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and f"tiny ok {W} {H}" in out.stdout, out.stdout[-3000:] + out.stderr[-3000:]


# ---- the sweep
KINDS = [(abi.PROC_CORNELL, 1.0), (abi.PROC_HELMET, 0.04), (abi.PROC_SPONZA, 0.02), (abi.PROC_BISTRO_EXT, 0.008), (abi.PROC_BISTRO_INT, 0.01)]
EVENTS = ["none", "taa_reset", "denoiser_reset", "denoiser_switch", "resize", "skip_parity"]


def _unit(rng):
    """(0, 1]"""
    return float(np.float32(1.0) - np.float32(rng.uniform(0.0, 1.0))) or 1.0


def _odd_size(rng):
    W, H = int(rng.integers(33, 260)), int(rng.integers(17, 150))
    force = int(rng.integers(0, 4))     # 0 / 1: as drawn (three in four of those have an odd side); 2: odd W; 3: odd H
    return (W | 1 if force == 2 else W), (H | 1 if force == 3 else H)


def draw_case(rng):
    """every random number of one case, in one place: _skip_case consumes the same"""
    c = {}
    c["kind"] = int(rng.integers(len(KINDS)))
    c["W"], c["H"] = _odd_size(rng)
    c["env"] = int(rng.integers(3))                      # 0 none, 1 HDR, 2 sun & sky
    c["seed"] = int(rng.integers(1, 1000))
    c["restir"] = int(rng.integers(0, 5)); c["depth"] = int(rng.integers(1, 5)); c["M"] = int(rng.integers(1, 9)); c["mis"] = int(rng.integers(0, 2))
    c["denoise"] = int(rng.choice([1, 1, 1, 0])); c["dbg"] = int(rng.choice([0, 0, 0, 0, 0, 0, 1, 4, 7, 9]))
    c["sky"] = dict(haze=float(rng.uniform(0, 5)), sun_direction=[float(v) for v in rng.normal(size=3)], horizon_height=float(rng.uniform(-0.5, 0.5)))
    c["latency"] = bool(rng.integers(0, 2)); c["overlap"] = int(rng.integers(0, 4))
    c["passes"] = int(rng.integers(1, 8))                # bit 0 SVGF, 1 GI spatial, 2 TAA
    c["svgf"] = dict(alphaColor=_unit(rng), alphaMoments=_unit(rng), historyCap=int(rng.choice([1, 2, 4, 32, 100000])),
                     phiLumDirect=float(10 ** rng.uniform(-2, 2)), phiLumIndirect=float(10 ** rng.uniform(-2, 2)))
    c["gis"] = dict(mode=int(rng.integers(1, 3)), samples=int(rng.integers(0, 17)), radius=int(rng.integers(1, 65)),
                    normalThreshold=float(rng.choice([-1.0, 0.0, 0.9, 1.0, rng.uniform(-1, 1)])), depthThreshold=float(10 ** rng.uniform(-2, 1)),
                    jacobianMax=float(rng.choice([1.0, 2.0, 10.0, 1e6, 1.0 + 10 ** rng.uniform(-2, 2)])))
    c["taa"] = dict(jitterPhases=int(rng.integers(0, 17)), alpha=_unit(rng), clipGamma=float(10 ** rng.uniform(-3, 1.5)))
    c["frames"] = int(rng.integers(3, 6))
    c["event"] = EVENTS[int(rng.integers(len(EVENTS)))]; c["event_at"] = int(rng.integers(1, 3))
    c["W2"], c["H2"] = _odd_size(rng)
    c["vel"] = [float(v) for v in rng.normal(scale=0.03, size=3)]
    c["dbg_at"] = int(rng.integers(0, 5))                # the debug view (if any) is on in this frame only: the frames around it have the reset rule to follow
    return c


def _skip_case(rng):
    """Consumes exactly the random numbers one case of run_sweep draws (to reproduce case N of a seed without rendering 0..N-1)."""
    draw_case(rng)


def run_one(c, tmp=None):
    """one drawn case: 3-5 frames, every frame compared; returns the {name: words} of the first mismatching frame, or {}"""
    from helpers import host, make_scene   # noqa: F401
    kind, scale = KINDS[c["kind"]]
    den = abi.Denoiser(mode=abi.DENOISER_SVGF, **c["svgf"]) if c["passes"] & 1 else abi.Denoiser()
    gis = abi.GiSpatial(**c["gis"]) if c["passes"] & 2 else None
    t = abi.Taa(mode=abi.TAA_ON, **c["taa"]) if c["passes"] & 4 else None
    sky = abi.SunAndSky(in_use=1, **c["sky"]) if c["env"] == 2 else None
    rig = optin.Rig(tmp, kind, scale, (64, 32) if c["env"] == 1 else None, c["W"], c["H"], seed=c["seed"], den=den, gis=gis, t=t, overlap=c["overlap"], sky=sky,
                    traversal=abi.TRAVERSAL_LATENCY if c["latency"] else abi.TRAVERSAL_THROUGHPUT)
    st = rig.st
    st.maxDepth, st.RISSampleNum, st.ReSTIRState, st.MIS, st.denoise = c["depth"], c["M"], c["restir"], c["mis"], c["denoise"]
    if c["env"] == 2:
        st.environmentProb = 0.5; st.envMapLuminIntegInv = 0.0
    eye, center, up, fov = rig.pose
    vel = np.array(c["vel"], dtype=np.float32)
    f = 0
    try:
        for i in range(c["frames"]):
            if i == c["event_at"]:
                ev = c["event"]
                if ev == "taa_reset":
                    rig.taa_reset()
                elif ev == "denoiser_reset":
                    rig.denoiser_reset()
                elif ev == "denoiser_switch":    # to the other filter, and back one frame later
                    rig.set_denoiser(abi.Denoiser(mode=abi.DENOISER_ATROUS if rig.den.mode == abi.DENOISER_SVGF else abi.DENOISER_SVGF, **c["svgf"]))
                elif ev == "resize":
                    rig.resize(c["W2"], c["H2"])
                elif ev == "skip_parity":
                    f += 1
            elif i == c["event_at"] + 1 and c["event"] == "denoiser_switch":
                rig.set_denoiser(den)
            st.debugging_mode = c["dbg"] if i == c["dbg_at"] else 0
            rig.sc.setCamera(eye + vel * i, center, up, fov)
            rig.sc.updateCamera(rig.W, rig.H)
            rig.frame(f, rig.sc.getCamera(), time0=77)
            bad = rig.diff(f)
            if bad:
                return dict(frame=f, differing=bad)
            f += 1
    finally:
        rig.destroy()
    return {}


def run_sweep(cases, seed, first=0, tmp=None):
    rng = np.random.default_rng(seed)
    bad = odd = 0
    for ci in range(cases):
        if ci < first:
            _skip_case(rng)
            continue
        c = draw_case(rng)
        odd += (c["W"] | c["H"]) & 1
        miss = run_one(c, tmp)
        if miss:
            bad += 1
        print("MISMATCH" if miss else "ok", json.dumps(dict(case=ci, sweep_seed=seed, **c)), json.dumps(miss) if miss else "", flush=True)
    print("cases", cases, "mismatching", bad, "odd-sized", odd)
    return bad


def test_random_configurations_of_the_opt_in_passes(tmp):
    assert run_sweep(int(os.environ.get("RESTIR_OPTIN_CASES", "48")), int(os.environ.get("RESTIR_OPTIN_SEED", "1")), tmp=tmp) == 0


def test_sweep_draws_mostly_odd_sizes_and_every_event():
    """the generator's promises, without rendering: at least half the cases have an odd W or H; every subset, event, ReSTIRState and build is drawn"""
    rng = np.random.default_rng(1)
    cs = [draw_case(rng) for _ in range(400)]
    assert sum((c["W"] | c["H"]) & 1 for c in cs) >= 200
    assert {c["passes"] for c in cs} == set(range(1, 8)) and {c["event"] for c in cs} == set(EVENTS) and {c["restir"] for c in cs} == set(range(5))
    assert {c["latency"] for c in cs} == {False, True} and {c["overlap"] for c in cs} == {0, 1, 2, 3} and {c["gis"]["mode"] for c in cs} == {1, 2}
    assert min(c["taa"]["jitterPhases"] for c in cs) == 0 and max(c["taa"]["jitterPhases"] for c in cs) == 16
    assert all(0 < c["taa"]["alpha"] <= 1 and 0 < c["svgf"]["alphaColor"] <= 1 and c["gis"]["jacobianMax"] >= 1 and c["taa"]["clipGamma"] >= 1e-3 for c in cs)
    a, b = np.random.default_rng(5), np.random.default_rng(5)
    draw_case(a); _skip_case(b)
    assert draw_case(a) == draw_case(b)


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--tiny":
        sys.exit(tiny_child(int(sys.argv[2]), int(sys.argv[3])))
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        sys.exit(1 if run_sweep(int(sys.argv[1]) if len(sys.argv) > 1 else 30, int(sys.argv[2]) if len(sys.argv) > 2 else 1, int(sys.argv[3]) if len(sys.argv) > 3 else 0,
                                tmp=d) else 0)
