"""One driver for "frame f with any subset of the opt-in passes": SVGF (rt_set_denoiser), GI spatial reuse (rt_set_gi_spatial) and TAA (rt_set_taa).

`Rig` holds the HIP renderer (optional: the CPU tests run without one) next to the oracle and the three checkers, applies every setting and every event with a
reset rule to both sides, and renders a frame on each.  The CPU side chains the oracle's stages and the checkers in the order rt_render_frame runs them:
jittered camera (TAA on, debugging_mode == 0), DIRECT, INDIRECT, the GI-spatial checker (rewrites IND_A), the SVGF checker or the A-Trous levels, COMPOSE, the
TAA checker.  `Rig.diff(f)` returns {name: differing 32-bit words} over everything either side exposes after frame f; the comparison is exact.
`tile_of_block` / `tile_grid` restate the XCD-striped tile order of csrc/stage_common.h; `ref_band_rows` the row-band rule of rt_reference_render."""
import numpy as np

from helpers import abi, host, make_scene, frame_buffers
from oracle.binding import Oracle
import gi_spatial
import svgf
import taa

HISTORY = (abi.SVGF_DIRECT_COLOR, abi.SVGF_INDIRECT_COLOR, abi.SVGF_DIRECT_MOMENTS, abi.SVGF_INDIRECT_MOMENTS)
TAA_IMAGES = (abi.TAA_DIRECT, abi.TAA_INDIRECT, abi.TAA_HISTORY_LENGTH)
# what a frame filtered by SVGF leaves in these is the chains' scratch (svgfArgs in csrc/rt_api.cpp: bufA / bufB), which the checker does not restate
SVGF_SCRATCH = (abi.BUF_DENOISE_DIR_A, abi.BUF_DENOISE_DIR_B, abi.BUF_DENOISE_IND_A)

TILE_SMALL_ROWS = 24      # RT_TILE_SMALL_ROWS: from this many tile rows on a launch deals whole tile rows per XCD
TILE_SMALL_CHUNK = 8      # RT_TILE_SMALL_CHUNK: below, chunks of this many tiles
REF_BAND_PIXELS = 1 << 20


# ---- the tile order of csrc/stage_common.h, restated from its comment: workgroup L runs on XCD L % 8; chunk c (row-major tile order, G tiles) belongs to XCD c % 8
def tile_chunk(tiles_x, tiles_y):
    return TILE_SMALL_CHUNK if tiles_y < TILE_SMALL_ROWS else tiles_x


def tile_of_block(L, tiles_x, tiles_y):
    """(x, y, valid) of workgroup L"""
    G = tile_chunk(tiles_x, tiles_y)
    xcd, k = L % 8, L // 8            # the k-th workgroup of its XCD
    j, off = divmod(k, G)             # its j-th chunk, tile `off` of it
    t = (j * 8 + xcd) * G + off       # chunk j * 8 + xcd is that XCD's j-th
    return t % tiles_x, t // tiles_x, t < tiles_x * tiles_y


def tile_grid(tiles_x, tiles_y):
    G = tile_chunk(tiles_x, tiles_y)
    chunks = -(-tiles_x * tiles_y // G)
    return 8 * -(-chunks // 8) * G


def tiles(n):
    return (n + 7) // 8


def ref_band_rows(W):
    """rows per launch of rt_reference_render"""
    return max(8, (REF_BAND_PIXELS // W) & ~7)


def words(a, b):
    """differing 32-bit words of two arrays of equal byte size"""
    a, b = np.ascontiguousarray(a).reshape(-1).view(np.uint8), np.ascontiguousarray(b).reshape(-1).view(np.uint8)
    assert a.size == b.size, (a.size, b.size)
    return int((a.view(np.uint32) != b.view(np.uint32)).sum()) if a.size % 4 == 0 else int((a != b).sum())


class Rig:
    def __init__(self, tmp, kind, scale, env_size, W, H, seed=1, den=None, gis=None, t=None, overlap=0, sky=None, traversal=None, gpu=True):
        self.tmp = tmp
        self.sc, self.env = make_scene(kind, scale, seed, env_size)
        self.W, self.H = W, H
        self.st = host.default_state(W, H, self.sc, self.env)
        if self.env is None:
            self.st.environmentProb = 0.0
        self.desc = self.sc.desc(self.env)
        self.den, self.gis, self.taa = den or abi.Denoiser(), gis or abi.GiSpatial(), t or abi.Taa()
        self.r = None
        if gpu:
            from restir_amd.renderer import Renderer
            self.r = Renderer().setup(0)
            self.r.set_overlap(overlap)
            self.r.load_scene(self.desc)
            self.r.update(W, H)
            if traversal is not None:
                self.r.set_traversal(traversal)
            self.r.set_denoiser(self.den)
            self.r.set_gi_spatial(self.gis)
            self.r.set_taa(self.taa)
        self.o = Oracle(0)
        self.o.upload_scene(self.desc)
        self.o.resize(W, H)
        if sky is not None:
            self.o.set_sun_and_sky(sky)
            if self.r:
                self.r.set_sun_and_sky(sky)
        self.kg = gi_spatial.GiSpatialChecker(gi_spatial.build(tmp), self.desc)
        self._sized_checkers()
        self.pose = self.sc.cameraPose()
        self.gis_out = None          # the GI checker's reservoirs of the last frame it ran in
        self.svgf_ran = self.taa_ran = False

    def _sized_checkers(self):
        self.ks = svgf.SvgfChecker(svgf.build(self.tmp), self.W, self.H, self.den)
        self.kt = taa.TaaChecker(taa.build(self.tmp), self.W, self.H, self.taa)

    def destroy(self):
        if self.r:
            self.r.destroy()
            self.r = None

    # ---- settings and events, on both sides (each follows the rule of include/rt_abi.h: a setter that changes nothing invalidates nothing)
    def set_denoiser(self, den):
        if self.r:
            self.r.set_denoiser(den)
        if bytes(den) != bytes(self.den):
            self.ks.set(den)
        self.den = den

    def set_gi_spatial(self, gis):
        if self.r:
            self.r.set_gi_spatial(gis)
        self.gis = gis

    def set_taa(self, t):
        if self.r:
            self.r.set_taa(t)
        self.kt.set(t)
        self.taa = t

    def taa_reset(self):
        if self.r:
            self.r.taa_reset()
        self.kt.reset()

    def denoiser_reset(self):
        if self.r:
            self.r.denoiser_reset()
        self.ks.reset()

    def resize(self, W, H):
        """rt_resize: every history is gone"""
        self.W, self.H = W, H
        self.st.size.x, self.st.size.y = W, H
        if self.r:
            self.r.update(W, H)
        self.o.resize(W, H)
        self._sized_checkers()
        self.gis_out = None

    # ---- frames
    def camera(self, f, move=0.01, cut=None):
        """the scene's pose moved along a fixed direction; from frame `cut` on seen from the opposite side (most of every history is rejected)"""
        eye, center, up, fov = self.pose
        eye = np.array(eye, dtype=np.float64)
        if cut is not None and f >= cut:
            eye = np.array(center, dtype=np.float64) * 2 - eye
        eye = eye + move * f * np.array([1.0, 0.25, -0.75])
        self.sc.setCamera(eye.astype(np.float32), center, up, fov)
        self.sc.updateCamera(self.W, self.H)
        return self.sc.getCamera()

    def gpu_frame(self, f, cam):
        self.r.set_camera(cam)
        self.r.run(self.st, f)

    def cpu_frame(self, f, cam):
        o, st = self.o, self.st
        cur = f & 1
        self.taa_ran = self.taa.mode == abi.TAA_ON and st.debugging_mode == 0
        jc = taa.jitter_camera(cam, f, self.taa.jitterPhases, self.W, self.H) if self.taa_ran else cam
        o.set_camera(jc)
        o.run_stage(st, f, abi.STAGE_DIRECT)
        o.run_stage(st, f, abi.STAGE_INDIRECT)
        if self.gis.mode != abi.GI_SPATIAL_OFF:
            self.gis_out, img, self.gis_taps = self.kg.run(st, jc, self.gis, o.readback(abi.BUF_GBUFFER0 + cur), o.readback(abi.BUF_INDIRECT_RESV0 + cur),
                                                           o.readback(abi.BUF_DENOISE_IND_A))
            o.upload_history(abi.BUF_DENOISE_IND_A, img)
        self.svgf_ran = self.den.mode == abi.DENOISER_SVGF and st.denoise > 0
        if self.den.mode == abi.DENOISER_SVGF:   # (a denoise == 0 frame invalidates the history: svgf_frame's rule)
            out_d, out_i = self.ks.frame(st, jc, f, this_g=o.readback(abi.BUF_GBUFFER0 + cur), last_g=o.readback(abi.BUF_GBUFFER0 + 1 - cur),
                                         motion=o.readback(abi.BUF_MOTION), noisy_dir=o.readback(abi.BUF_DIRECT_RESULT0 + cur),
                                         noisy_ind=o.readback(abi.BUF_DENOISE_IND_A))
            if self.svgf_ran:
                o.upload_history(abi.BUF_DIRECT_RESULT0 + cur, out_d)
                o.upload_history(abi.BUF_DENOISE_IND_B, out_i)
        elif st.denoise > 0:
            for i in range(4):
                o.run_stage(st, f, abi.STAGE_DENOISE_DIRECT, i)
            for i in range(5):
                o.run_stage(st, f, abi.STAGE_DENOISE_INDIRECT, i)
        o.run_stage(st, f, abi.STAGE_COMPOSE)
        if self.taa_ran:
            self.kt.frame(jc, f, o.readback(abi.BUF_GBUFFER0 + cur), o.readback(abi.BUF_GBUFFER0 + 1 - cur), o.readback(abi.BUF_DIRECT_RESULT0 + cur),
                          o.readback(abi.BUF_INDIRECT_RESULT0 + cur))
        else:
            self.kt.skip()
        return jc

    def frame(self, f, cam=None, time0=1000):
        self.st.time = time0 + f
        cam = cam if cam is not None else self.camera(f)
        if self.r:
            self.gpu_frame(f, cam)
        return self.cpu_frame(f, cam)

    def diff(self, f):
        """{name: differing words} after frame f on both sides; empty when everything matches"""
        bad = {}
        cur = f & 1
        bufs = frame_buffers(f) + ([abi.BUF_DIRECT_RESV_TEMP] if self.st.ReSTIRState in (2, 4) else [])
        for b in bufs:
            if self.svgf_ran and b in SVGF_SCRATCH:
                continue
            d = words(self.r.readback(b), self.o.readback(b))
            if d:
                bad[abi.BUFFER_NAMES[b]] = d
        if self.svgf_ran:
            for w in HISTORY:
                d = words(self.r.denoiser_readback(w), self.ks.history(w))
                if d:
                    bad["svgf_history%d" % w] = d
        if self.gis.mode != abi.GI_SPATIAL_OFF:
            d = words(self.r.gi_spatial_readback(), self.gis_out)
            if d:
                bad["gi_spatial_resv"] = d
        if self.taa_ran:
            for which, want in zip(TAA_IMAGES, (self.kt.D[cur], self.kt.I[cur], self.kt.N[cur])):
                d = words(self.r.taa_readback(which), want)
                if d:
                    bad["taa%d" % which] = d
        return bad

    # ---- what the checkers saw: the sanity assertions of the tests ("a comparison of two empty histories proves nothing")
    def history_lengths(self):
        """{pass: array of n over the pixels with a surface} of the last frame"""
        out = {}
        if self.svgf_ran:
            for name, w in (("svgf_direct", abi.SVGF_DIRECT_COLOR), ("svgf_indirect", abi.SVGF_INDIRECT_COLOR)):
                n = self.ks.history(w)[..., 3]
                out[name] = n[n > 0]
        if self.taa_ran:
            g = self.o.readback(abi.BUF_GBUFFER0 + (self.kt.last & 1)).view(np.uint32).reshape(self.H, self.W, 4)
            out["taa"] = self.kt.N[self.kt.last][(g[..., 3] & np.uint32(0xFF000000)) != 0xFF000000]
        return out
