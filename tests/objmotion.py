"""Shared driver of the object-motion tests (rt_set_object_motion): not a test.

The feature is defined so that the unmodified oracle can produce the expected frame: for a pixel that sees instance i the frame behaves as if the previous camera
had been rt_object_motion_camera(cam, P_i, C_i).  `composite_frame` therefore runs the oracle's DIRECT and INDIRECT stages once per distinct camera from the same
saved buffers — one group per instance in motion, group 0 (everything else) with the real camera —, keeps every per-pixel output, composites them per pixel by
the instance image (half-resolution outputs by the instance at 2p), uploads the composite and runs the A-Trous levels and compose as optin.Rig.cpu_frame does.
Every pixel's random stream is a function of (pixel, time) alone, so the groups draw the same numbers.
`Case` holds a scene, the HIP renderer (optional) and the oracle, moves instances with the transform classes of refit.move_matrix and re-uploads the moved scene
to the oracle between frames, as the refit tests do.  With SVGF (`den`) or GI spatial reuse (`gis`) on, the checkers of tests/svgf.py and tests/gi_spatial.py run on
the composite in the order optin.Rig.cpu_frame runs them; the SVGF checker receives the composite motion buffer."""
import numpy as np

from helpers import abi, host, frame_buffers
from oracle.binding import Oracle
import optin
import refit

MISS = 0xFFFFFFFF
FULL = lambda cur: (abi.BUF_GBUFFER0 + cur, abi.BUF_MOTION, abi.BUF_DIRECT_RESV0 + cur, abi.BUF_LIGHT_ID0 + cur, abi.BUF_DIRECT_RESULT0 + cur)   # noqa: E731
HALF = lambda cur: (abi.BUF_INDIRECT_RESV0 + cur,)   # noqa: E731  (+ DENOISE_IND_A, an image at half resolution in a full-resolution allocation: see _composite)
SAVED = [b for b in range(abi.BUF_COUNT) if b != abi.BUF_LDR]


def motion_camera(cam, prev, cur):
    from restir_amd.renderer import Renderer
    return Renderer.object_motion_camera(cam, prev, cur)


def pick_image(o, cam, W, H):
    """the oracle's instance under every pixel centre (MISS where the ray leaves the scene)"""
    out = np.empty((H, W), np.uint32)
    for y in range(H):
        for x in range(W):
            p = o.pick(cam.viewInverse, cam.projInverse, (x + 0.5) / W, (y + 0.5) / H)
            out[y, x] = MISS if p.instanceID < 0 else p.instanceID
    return out


def silhouette(pick):
    """pixels whose 4-neighbourhood in the pick image holds more than one instance"""
    s = np.zeros(pick.shape, bool)
    s[1:, :] |= pick[1:, :] != pick[:-1, :]
    s[:-1, :] |= pick[:-1, :] != pick[1:, :]
    s[:, 1:] |= pick[:, 1:] != pick[:, :-1]
    s[:, :-1] |= pick[:, :-1] != pick[:, 1:]
    return s


def check_instance_image(inst, pick):
    """the rule of the issue: a disagreement only at a silhouette pixel of the pick image, and at most 2 % of the image.  Returns the tolerated share.
    The issue also asks for poses whose pick image has under 2 % silhouette pixels; these scenes have none (every wall is an instance, so 7 % of the pixels at
    street 64 x 48 up to 68 % at Cornell 16 x 8 are silhouette pixels).  The first clause alone would therefore tolerate a wrong instance id on that many
    pixels: what bounds a wrong id there is the 2 % cap (2 pixels at 16 x 8, 61 at 64 x 48), not the silhouette clause."""
    inst, pick = inst.reshape(pick.shape), pick
    bad = inst != pick
    assert not (bad & ~silhouette(pick)).any(), "the instance image differs from the pick image off a silhouette at %s" % (np.argwhere(bad & ~silhouette(pick))[:4].tolist(),)
    assert bad.mean() <= 0.02, bad.mean()
    return float(bad.mean())


def spatial_mode(st):
    return st.ReSTIRState in (abi.RESTIR_SPATIAL, abi.RESTIR_SPATIOTEMPORAL)


def _composite(o, outs, ids, inst, W, H, cur, full):
    """per pixel: group k's output where the instance image holds ids[k], the last entry of `outs` (group 0) elsewhere; uploads the result"""
    inst = inst.reshape(H, W)
    half = inst[0:2 * (H // 2):2, 0:2 * (W // 2):2]
    want = {}
    for b in full + HALF(cur) + (abi.BUF_DENOISE_IND_A,):
        sel, n = (inst, W * H) if b in full else (half, (W // 2) * (H // 2))
        if b == abi.BUF_DENOISE_IND_A:   # rows of W texels; the half-resolution image occupies [0, H/2) x [0, W/2)
            a = outs[-1][b].copy().reshape(H, W, -1)
            for k, i in enumerate(ids):
                m = half == i
                a[:H // 2, :W // 2][m] = outs[k][b].reshape(H, W, -1)[:H // 2, :W // 2][m]
        else:
            a = outs[-1][b].copy().reshape(n, -1)
            for k, i in enumerate(ids):
                m = (sel == i).reshape(-1)
                a[m] = outs[k][b].reshape(n, -1)[m]
        want[b] = a.reshape(-1)
        o.upload_history(b, want[b])
    return want


def composite_frame(o, st, f, cam, groups, inst, W, H, checkers=None):
    """frame f on oracle `o`: `groups` = [(instance, P, C)] for the instances in motion, `inst` the instance image that steers the composite.
    `checkers`: None, or the `Case` whose GI-spatial / SVGF checkers run on the composite (the order of optin.Rig.cpu_frame)"""
    cur = f & 1
    # the spatial modes cache every pixel's reservoir before the spatial phase: a per-pixel output like the others
    full = FULL(cur) + ((abi.BUF_DIRECT_RESV_TEMP,) if spatial_mode(st) else ())
    snap = {b: o.readback(b).copy() for b in SAVED}
    outs = []
    cams = [motion_camera(cam, P, Cm) for _, P, Cm in groups] + [cam]
    for gc in cams:
        for b, d in snap.items():
            o.upload_history(b, d)
        o.set_camera(gc)
        o.run_stage(st, f, abi.STAGE_DIRECT)
        o.run_stage(st, f, abi.STAGE_INDIRECT)
        outs.append({b: o.readback(b).copy() for b in full + HALF(cur) + (abi.BUF_DENOISE_IND_A,)})
    if groups:
        _composite(o, outs, [g[0] for g in groups], inst, W, H, cur, full)
    o.set_camera(cam)
    k = checkers
    if k is not None and k.gis.mode != abi.GI_SPATIAL_OFF:
        k.gis_out, img, k.gis_taps = k.kg.run(st, cam, k.gis, o.readback(abi.BUF_GBUFFER0 + cur), o.readback(abi.BUF_INDIRECT_RESV0 + cur), o.readback(abi.BUF_DENOISE_IND_A))
        o.upload_history(abi.BUF_DENOISE_IND_A, img)
    if k is not None and k.den.mode == abi.DENOISER_SVGF:
        out_d, out_i = k.ks.frame(st, cam, f, this_g=o.readback(abi.BUF_GBUFFER0 + cur), last_g=o.readback(abi.BUF_GBUFFER0 + 1 - cur),
                                  motion=o.readback(abi.BUF_MOTION), noisy_dir=o.readback(abi.BUF_DIRECT_RESULT0 + cur), noisy_ind=o.readback(abi.BUF_DENOISE_IND_A))
        if st.denoise > 0:
            o.upload_history(abi.BUF_DIRECT_RESULT0 + cur, out_d)
            o.upload_history(abi.BUF_DENOISE_IND_B, out_i)
    elif st.denoise > 0:
        for i in range(4):
            o.run_stage(st, f, abi.STAGE_DENOISE_DIRECT, i)
        for i in range(5):
            o.run_stage(st, f, abi.STAGE_DENOISE_INDIRECT, i)
    o.run_stage(st, f, abi.STAGE_COMPOSE)


SEQUENCE = ("translate", "rotate", "scale", None, "mirror")   # frames 1..5; frame 0 and the `None` frame have no update


class Case:
    def __init__(self, kind, W, H, gpu=True, overlap=0, traversal=None, restir=abi.RESTIR_TEMPORAL, sky=None, movers=None, den=None, gis=None, tmp=None):
        self.sc = refit.cornell() if kind == "cornell" else refit.street()
        self.W, self.H = W, H
        self.st = host.default_state(W, H, self.sc, None)
        self.st.environmentProb = 0.0
        self.st.ReSTIRState = restir
        self.desc = self.sc.desc()
        self.home = refit.instances_of(self.desc)["objectToWorld"].copy()
        self.extent = float(max(np.abs(np.concatenate(refit.world_bounds(self.desc, i))).max() for i in range(self.desc.numInstances)))
        self.pose = self.sc.cameraPose()
        self.o = Oracle(0)
        self.o.upload_scene(self.desc)
        self.o.resize(W, H)
        self.r = None
        if gpu:
            from restir_amd.renderer import Renderer
            self.r = Renderer().setup(0)
            self.r.set_overlap(overlap)
            self.r.load_scene(self.desc)
            self.r.update(W, H)
            if traversal is not None:
                self.r.set_traversal(traversal)
            self.r.set_object_motion(abi.OBJECT_MOTION_ON)
        self.den, self.gis = den or abi.Denoiser(), gis or abi.GiSpatial()
        self.checked = den is not None or gis is not None    # (the checkers are built into `tmp`)
        if self.checked:
            import gi_spatial
            import svgf
            self.gi_lib = gi_spatial.build(tmp)
            self.kg = gi_spatial.GiSpatialChecker(self.gi_lib, self.desc)
            self.ks = svgf.SvgfChecker(svgf.build(tmp), W, H, self.den)
            self.gis_out = None
            if self.r:
                self.r.set_denoiser(self.den)
                self.r.set_gi_spatial(self.gis)
        if sky is not None:
            self.o.set_sun_and_sky(sky)
            if self.r:
                self.r.set_sun_and_sky(sky)
        self.movers = list(movers) if movers is not None else self.default_movers()
        self.inst = None
        self.groups = []
        self.pending = {}    # instance -> its objectToWorld at the last rendered frame, for the instances updated since

    def destroy(self):
        if self.r:
            self.r.destroy()
            self.r = None

    def default_movers(self, count=2):
        """the non-emissive instances with the most pixels under the first camera that cover less than a sixth of the image (props, not walls)"""
        pick = pick_image(self.o, self.camera(0), self.W, self.H)
        emissive = set(refit.describe(self.desc)["emissive"].tolist())
        ids, n = np.unique(pick[pick != MISS], return_counts=True)
        cand = [(int(c), int(i)) for i, c in zip(ids, n) if int(i) not in emissive and c < pick.size / 6]
        return [i for _, i in sorted(cand, reverse=True)[:count]]

    def camera(self, f, move=0.01):
        eye, center, up, fov = self.pose
        e = np.array(eye, np.float64) + move * f * np.array([1.0, 0.25, -0.75])
        self.sc.setCamera(e.astype(np.float32), center, up, fov)
        self.sc.updateCamera(self.W, self.H)
        return self.sc.getCamera()

    def update(self, ids, xf):
        """rt_update_instances on both sides; remembers, per moved instance, the matrix of the last rendered frame (once)"""
        cur = refit.instances_of(self.desc)["objectToWorld"]
        for i in ids:
            self.pending.setdefault(int(i), cur[int(i)].copy())
        self.sc.updateInstances(np.asarray(ids, np.uint32), np.asarray(xf, np.float32))
        self.desc = self.sc.desc()
        if self.r:
            self.r.update_instances(ids, xf)
            self.r.update_lights(self.desc)
        self.o.upload_scene(self.desc)
        if self.checked:   # the GI checker traces its visibility rays in the scene it was created with: the moved scene, like the oracle
            import gi_spatial
            self.kg = gi_spatial.GiSpatialChecker(self.gi_lib, self.desc)

    def frame(self, f, kind=None, cam=None, time0=1000):
        """move `movers` by `kind` (None: no update), render frame f on both sides; the oracle's buffers hold the composite expectation afterwards"""
        if kind is not None:
            ids = self.movers
            self.update(ids, np.stack([refit.move_matrix(kind, self.desc, i, self.extent, self.home) for i in ids]))
        self.st.time = time0 + f
        cam = cam if cam is not None else self.camera(f)
        now = refit.instances_of(self.desc)["objectToWorld"]
        self.groups = [(i, P, now[i].copy()) for i, P in sorted(self.pending.items()) if P.tobytes() != now[i].tobytes()]
        self.pending = {}
        if self.r:
            self.r.set_camera(cam)
            self.r.run(self.st, f)
            self.inst = self.r.object_motion_readback()
        else:
            self.inst = pick_image(self.o, cam, self.W, self.H).reshape(-1)
        composite_frame(self.o, self.st, f, cam, self.groups, self.inst, self.W, self.H, self if self.checked else None)
        return cam

    def diff(self, f):
        """{name: differing words} after frame f; with a checker on, what optin.Rig.diff compares for that pass"""
        bad = {}
        svgf_ran = self.den.mode == abi.DENOISER_SVGF and self.st.denoise > 0
        for b in frame_buffers(f):
            if svgf_ran and b in optin.SVGF_SCRATCH:
                continue
            d = optin.words(self.r.readback(b), self.o.readback(b))
            if d:
                bad[abi.BUFFER_NAMES[b]] = d
        if svgf_ran:
            for w in optin.HISTORY:
                d = optin.words(self.r.denoiser_readback(w), self.ks.history(w))
                if d:
                    bad["svgf_history%d" % w] = d
        if self.gis.mode != abi.GI_SPATIAL_OFF:
            d = optin.words(self.r.gi_spatial_readback(), self.gis_out)
            if d:
                bad["gi_spatial_resv"] = d
        return bad

    def group_image(self):
        """per pixel the index of its group in the last frame: k + 1 where the instance image holds the k-th instance in motion, 0 elsewhere"""
        g = np.zeros((self.H, self.W), np.int32)
        for k, (i, _, _) in enumerate(self.groups):
            g[self.inst.reshape(self.H, self.W) == i] = k + 1
        return g


def one_group_footprint(g, radius=1):
    """pixels whose (2 radius + 1)^2 neighbourhood, clipped to the image, lies in one group of the group image `g`"""
    H, W = g.shape
    ok = np.ones((H, W), bool)
    for dy in range(-radius, radius + 1):
        for dx in range(-radius, radius + 1):
            ys, xs = slice(max(0, -dy), H - max(0, dy)), slice(max(0, -dx), W - max(0, dx))
            yn, xn = slice(max(0, dy), H - max(0, -dy)), slice(max(0, dx), W - max(0, -dx))
            ok[ys, xs] &= g[ys, xs] == g[yn, xn]
    return ok
