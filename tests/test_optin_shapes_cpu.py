"""The CPU half of the opt-in passes' shape coverage (tests/test_gpu_optin_shapes.py is the GPU half); nothing here needs a GPU.

* The three checkers (tests/svgf_checker.cpp, gi_spatial_checker.cpp, taa_checker.cpp), which the GPU tests hold the kernels to word for word, against their
  independent float64 models at image sizes that are odd in W only, odd in both directions, and smaller than one 8 x 8 tile.  At even sizes 2 * (W / 2) == W,
  so a slip between W / 2, (W + 1) / 2 and W shared by a kernel and its checker would pass every GPU comparison; here it meets a model that has its own indexing.
  The models are the ones of test_svgf_cpu.py / test_gi_spatial_cpu.py / test_taa_cpu.py (imported, with their tolerances).
* The XCD-striped tile order (tileChunk / tileOfBlock / tileGrid of csrc/stage_common.h) as a bijection, in both regimes and across the crossover at 24 tile
  rows.  stage_common.h cannot be included by a host compiler (it pulls in the traversal code: wave intrinsics, blockIdx), and the library exports no entry for
  it, so the Python restatement (tests/optin.py, written from the header's comment) is tested as the specification, its constants are read back from the
  header, and the GPU cases at 123 x 187 and 83 x 391 hold the kernels' own copy to it through the images.
* The oracle and every checker at sizes below one tile (half-resolution grid 0 x 0, 1 x 1, 3 x 2): no crash, finite images, the readback shapes.
* RefChecker's split invariance at a ragged size: the CPU statement has no row bands, which is why it is the reference for rt_reference_render's band loop.

Wall time of `pytest tests -m "not gpu"` on an 8-core machine: about 700 s before this module; this module adds 27 s."""
import os
import re
import numpy as np
import pytest
from helpers import ROOT, abi, host, make_scene
import optin
import refpt
import svgf
import gi_spatial
import taa
import test_svgf_cpu
import test_gi_spatial_cpu
import test_taa_cpu

# W x H: why
ODD_SIZES = [
    (45, 32),   # odd in W only: half-res 22 x 16, 2 * (W / 2) = 44 != W, so the half-res stride differs from W / 2 rounded up
    (37, 27),   # odd in both: half-res 18 x 13; the last full-res row and column have no half-res pixel
]
TINY = (7, 5)   # below one tile: half-res 3 x 2; the 7 x 7 moment window, the step-16 taps and the 4 x 4 Catmull-Rom footprint are larger than the image
BELOW_ONE_TILE = [(1, 1), (2, 3), (7, 5), (9, 9), (16, 1), (1, 16)]   # half-res 0x0, 1x1, 3x2, 4x4, 8x0, 0x8


@pytest.fixture(scope="module")
def tmp(tmp_path_factory):
    return tmp_path_factory.mktemp("optin")


# ---- checkers against their float64 models
@pytest.mark.parametrize("W,H", ODD_SIZES + [TINY], ids=lambda v: str(v))
def test_svgf_checker_matches_its_model_at_odd_sizes(tmp, W, H):
    """odd W or H with a half-resolution grid (geometry and history stride W / 2, images stride W, G-buffer at 2p, motion(2p) >> 1), and below one tile"""
    assert W % 2 == 1
    got = test_svgf_cpu.check_model(svgf.build(tmp), W, H)
    assert got["accepted"] > 0 and got["peak_direct"] > 0 and got["peak_indirect"] > 0, got
    if (W, H) != TINY:
        assert got["rejected"] > 0 and got["long_history"] > W * H // 4 and got["long_history_indirect"] > 0, got


@pytest.mark.parametrize("W,H", ODD_SIZES + [TINY], ids=lambda v: str(v))
def test_gi_spatial_checker_matches_its_model_at_odd_sizes(tmp, W, H):
    """odd W or H: the seed, the reservoir stride and raySpawn use W / 2, the G-buffer W"""
    assert W % 2 == 1
    # (in a 3 x 2 grid the default radius sends nearly every tap outside: radius 1, more taps)
    s = abi.GiSpatial(mode=abi.GI_SPATIAL_ON, samples=16, radius=1, normalThreshold=0.5, depthThreshold=0.5) if (W, H) == TINY else None
    got = test_gi_spatial_cpu.check_model(gi_spatial.build(tmp), W, H, s)
    assert got["surface"] > 0 and got["merged"] > 0, got
    if (W, H) != TINY:
        assert got["merged"] > got["surface"] // 4 and got["moved"] > 20, got


@pytest.mark.parametrize("W,H", ODD_SIZES + [TINY], ids=lambda v: str(v))
def test_taa_checker_matches_its_model_at_odd_sizes(tmp, W, H):
    """sizes that are no multiple of the tile, and a 7 x 5 image where every Catmull-Rom tap row and column is clamped.
    The cap on pixels left out as borderline stays 5 % of the image.  7 x 5 has 35 pixels, 5 % of which is 1.75: one borderline pixel is within the cap and two
    are not, although two of 35 say nothing different about the checker than 76 of 1536 (48 x 32) do.  Borderline pixels are those whose reprojected position
    lies within 1e-3 px of a pixel edge (or whose normal / depth test is within 1e-4 of its threshold); under the camera move of the model test the probability
    per pixel is about 4e-3 per axis, so among 35 pixels two in one frame is already a < 4 % event.  The allowance for this size is therefore stated as an
    absolute count: at most 2 pixels per frame."""
    got = test_taa_cpu.check_model(taa.build(tmp), W, H, border_pixels=2 if (W, H) == TINY else None)
    assert got["accepted"] > 0 and got["peak"] > 0, got
    if (W, H) != TINY:
        assert got["accepted"] > W * H and got["rejected"] > 0 and got["clipped"] > 0, got


# ---- the tile order
def test_tile_order_constants_are_the_headers():
    src = open(os.path.join(ROOT, "cis-565-final-vr-raytracer_amd", "csrc", "stage_common.h")).read()
    val = lambda name: int(re.search(r"#define " + name + r" (\d+)", src).group(1))   # noqa: E731
    assert val("RT_TILE_SMALL_ROWS") == optin.TILE_SMALL_ROWS and val("RT_TILE_SMALL_CHUNK") == optin.TILE_SMALL_CHUNK
    assert val("RT_TILE_STRIPE") == 1 and val("RT_TILE_CHUNK") == 0      # whole tile rows, one per stripe: tile_chunk's second regime
    assert "tilesY < RT_TILE_SMALL_ROWS ? RT_TILE_SMALL_CHUNK : TILE_STRIPE * tilesX" in src
    # the row bands of rt_reference_render
    ref = open(os.path.join(ROOT, "cis-565-final-vr-raytracer_amd", "csrc", "reference.h")).read()
    m = re.search(r"REF_BAND_PIXELS = (\d+) << (\d+);", ref)
    assert int(m.group(1)) << int(m.group(2)) == optin.REF_BAND_PIXELS
    assert "std::max(8, (REF_BAND_PIXELS / c->W) & ~7)" in open(os.path.join(ROOT, "cis-565-final-vr-raytracer_amd", "csrc", "rt_api.cpp")).read()
    assert optin.ref_band_rows(4096) == 256 and optin.ref_band_rows(64) == 16384


def test_tile_order_is_a_bijection_in_both_regimes():
    """every (tilesX, tilesY) in 1..40 x 1..40 — chunks of 8 tiles below 24 tile rows, whole tile rows from 24 on: the valid workgroups hit every tile exactly
    once, the invalid ones (the grid is rounded up to 8 x perXcd x G) none, and tile (x, y) of XCD L % 8 is where the header's comment puts it"""
    regimes = set()
    for ty in range(1, 41):
        for tx in range(1, 41):
            G = optin.tile_chunk(tx, ty)
            regimes.add(G == tx and ty >= optin.TILE_SMALL_ROWS)
            grid = optin.tile_grid(tx, ty)
            assert grid % (8 * G) == 0 and grid >= tx * ty and grid - tx * ty < 8 * G + 8 * G, (tx, ty, grid)
            seen = np.zeros((ty, tx), dtype=np.int32)
            invalid = 0
            for L in range(grid):
                x, y, valid = optin.tile_of_block(L, tx, ty)
                if valid:
                    assert 0 <= x < tx and 0 <= y < ty
                    seen[y, x] += 1
                    chunk = (y * tx + x) // G
                    assert chunk % 8 == L % 8, (tx, ty, L)          # chunk c belongs to XCD c % 8
                    if ty >= optin.TILE_SMALL_ROWS:
                        assert y % 8 == L % 8                         # stripe regime: tile row y belongs to XCD y % 8
                else:
                    invalid += 1
            assert (seen == 1).all(), (tx, ty)
            assert invalid == grid - tx * ty
    assert regimes == {False, True}
    # the crossover itself: 23 tile rows are dealt in chunks of 8, 24 in whole rows
    assert optin.tile_chunk(11, 23) == 8 and optin.tile_chunk(11, 24) == 11
    # the sizes the GPU stripe cases use are in the second regime, full resolution and half resolution
    assert optin.tiles(187) == 24 and optin.tiles(391 // 2) == 25 and optin.tiles(391) == 49 and optin.tiles(184) == 23


# ---- below one tile: the oracle and every checker, before a GPU sees these sizes
@pytest.mark.parametrize("W,H", BELOW_ONE_TILE, ids=lambda v: str(v))
def test_oracle_and_checkers_below_one_tile(tmp, W, H):
    """rt_resize accepts 1..32767: at 1x1, 2x3, 7x5, 9x9, 16x1, 1x16 the half-resolution grid is 0x0, 1x1, 3x2, 4x4, 8x0, 0x8"""
    assert optin.tiles(W) * optin.tiles(H) <= 4 and (min(W, H) < 8 or (W, H) == (9, 9))
    rig = optin.Rig(tmp, abi.PROC_CORNELL, 1.0, None, W, H, den=abi.Denoiser(mode=abi.DENOISER_SVGF),
                    gis=abi.GiSpatial(mode=abi.GI_SPATIAL_VISIBILITY, samples=6, radius=3), t=abi.Taa(mode=abi.TAA_ON), gpu=False)
    n_taa = n_svgf = 0
    for f in range(6):
        rig.frame(f)
        cur = f & 1
        for b in (abi.BUF_DIRECT_RESULT0 + cur, abi.BUF_INDIRECT_RESULT0 + cur, abi.BUF_DENOISE_IND_B):
            img = rig.o.readback(b).view(np.float32)
            assert img.size == W * H * 4 and np.isfinite(img).all(), abi.BUFFER_NAMES[b]
        assert rig.o.readback(abi.BUF_INDIRECT_RESV0 + cur).size == (W // 2) * (H // 2) * gi_spatial.RESV_BYTES
        assert rig.gis_out.size == (W // 2) * (H // 2) * gi_spatial.RESV_BYTES and rig.gis_taps.shape == (H // 2, W // 2)
        for w in optin.HISTORY:
            h = rig.ks.history(w)
            assert h.shape == ((H // 2, W // 2) if w & 1 else (H, W)) + ((4,) if w < 2 else (2,)) and np.isfinite(h).all()
        D, I, N = rig.kt.D[cur], rig.kt.I[cur], rig.kt.N[cur]
        assert D.shape == I.shape == (H, W, 4) and N.shape == (H, W) and np.isfinite(D).all() and np.isfinite(I).all() and (N >= 1).all()
        n_taa, n_svgf = max(n_taa, int(N.max())), max(n_svgf, int(rig.ks.history(abi.SVGF_DIRECT_COLOR)[..., 3].max()))
    assert rig.o.readback(abi.BUF_DIRECT_RESULT0 + 1).view(np.float32).max() > 0      # the Cornell box fills even one pixel
    # history was accepted in some frame (the sub-pixel jitter of a one-pixel image is half its field of view: not in every frame)
    # (16 x 1: the vertical jitter moves the single row between ceiling, back wall and floor, and no frame of the six accepts any)
    assert (n_taa > 1 and n_svgf > 1) or (W, H) == (16, 1), (n_taa, n_svgf)


# ---- the reference checker has no bands
def test_ref_checker_split_invariance_at_a_ragged_size(tmp):
    """2 + 1 samples == 3 samples at 67 x 45 (neither a multiple of 8), word for word"""
    W, H = 67, 45
    sc, env = make_scene(abi.PROC_SPONZA, 0.01, 1, (64, 32))
    st = host.default_state(W, H, sc, env)
    st.maxDepth = 3
    desc = sc.desc(env)
    sc.updateCamera(W, H)
    out = []
    for split in ((2, 1), (3,)):
        k = refpt.RefChecker(refpt.build(tmp), desc)
        k.resize(W, H)
        k.set_camera(sc.getCamera())
        for n in split:
            k.render(st, n)
        assert k.samples() == 3
        out.append([k.readback(c) for c in range(3)])
    for a, b in zip(*out):
        assert a.shape == (H, W, 4) and optin.words(a, b) == 0
    assert out[0][2][..., :3].max() > 0 and out[0][1][..., :3].max() > 0
