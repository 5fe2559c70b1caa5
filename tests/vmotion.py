"""Shared driver of the per-vertex motion-vector tests (rt_set_object_motion mode OBJECT_MOTION_VERTEX): not a test.

`VmChecker` drives tests/vmotion_checker.cpp (the CPU restatement of the new arithmetic: delta, motion index, both reprojDepth).  The oracle has no hook for the two
changed expressions, but its last-frame buffers are uploadable and every pixel looks up one known location in them: `expected_frame` therefore WARPS THE HISTORY.
For a hit pixel p the unmodified oracle looks at t = m_o(p) (its own motion index); the feature looks at s = m_v(p) and decides the depth test with its own
reprojDepth.  So L'[t] = L[s] with the depth word replaced by 1e30 (the oracle's depth test then passes) when the feature's depth test accepts, and by 0.0 (it
then fails) when it does not; the oracle's own hash and normal tests run on the gathered words.  The direct and the indirect stage get a warped history each,
the true one is restored before the filters, and the expected motion buffer replaces the oracle's.
`Case` holds a scene whose meshes deform (skins, a morph set, host rows) and whose instances move, the HIP renderer (optional) and the oracle, and keeps, like the
context, the positions / matrices of the last rendered frame for what changed since."""
import ctypes as C
import os
import subprocess
import numpy as np

from helpers import ROOT, abi, host, frame_buffers
from oracle.binding import Oracle
import optin
import refit
import skin
import morph
from objmotion import SAVED, FULL, MISS, spatial_mode

SRC = os.path.join(ROOT, "tests", "vmotion_checker.cpp")
FLAGS = ["-O2", "-std=c++17", "-fPIC", "-mfma", "-ffp-contract=off", "-fno-fast-math", "-pthread", "-shared"]   # the oracle's (oracle/Makefile), as tests/gi_spatial.py
HIT_DT = np.dtype([("inst", "<u4"), ("prim", "<u4"), ("u", "<f4"), ("v", "<f4")])
_lib = None


def build(out_dir):
    """compile the checker + oracle/orc_scene.cpp into out_dir/libvmchk.so (once per process) and load it"""
    global _lib
    if _lib is None:
        so = os.path.join(str(out_dir), "libvmchk.so")
        subprocess.check_call([os.environ.get("CXX", "g++")] + FLAGS + [SRC, os.path.join(ROOT, "oracle", "orc_scene.cpp"), "-o", so])
        L = C.CDLL(so)
        L.vmc_create.restype = C.c_void_p
        L.vmc_create.argtypes = [C.c_void_p]
        L.vmc_destroy.argtypes = [C.c_void_p]
        L.vmc_run.argtypes = [C.c_void_p] * 15
        _lib = L
    return _lib


class VmChecker:
    """the checker on one (current) scene description"""

    def __init__(self, lib, desc):
        self.L, self._desc = lib, desc
        self.h = lib.vmc_create(C.byref(desc))

    def __del__(self):
        if getattr(self, "h", None):
            self.L.vmc_destroy(self.h)
            self.h = None

    def run(self, st, cam, prev_pos=None, mesh_deformed=None, prev_o2w=None, inst_moved=None, this_g=None):
        """prev_pos (numVertices x 3) / mesh_deformed (per prim mesh) and prev_o2w (numInstances x 12) / inst_moved (per instance) describe the last rendered frame;
        this_g: the frame's G-buffer (for the half-resolution depths).  Returns a dict of arrays: d (n, 4) f32, xprev (n, 3) f32, m32 (n, 2) i32, m16 (n, 2) i16,
        depthD (n) f32, hits (n) HIT_DT, depthI (nh) f32 or None"""
        W, H = st.size.x, st.size.y
        n, nh = W * H, (W // 2) * (H // 2)
        keep = [None if a is None else np.ascontiguousarray(a, dtype=t) for a, t in ((prev_pos, np.float32), (mesh_deformed, np.uint8), (prev_o2w, np.float32), (inst_moved, np.uint8))]
        g = None if this_g is None else np.ascontiguousarray(this_g).view(np.uint8).reshape(-1)[:n * 16].copy()
        out = {"d": np.zeros((n, 4), np.float32), "xprev": np.zeros((n, 3), np.float32), "m32": np.zeros((n, 2), np.int32), "m16": np.zeros((n, 2), np.int16),
               "depthD": np.zeros(n, np.float32), "hits": np.zeros(n, HIT_DT), "depthI": None if g is None else np.zeros(nh, np.float32)}
        p = lambda a: None if a is None else a.ctypes.data   # noqa: E731
        rc = self.L.vmc_run(self.h, C.byref(st), C.byref(cam), p(keep[0]), p(keep[1]), p(keep[2]), p(keep[3]), p(g), p(out["d"]), p(out["xprev"]), p(out["m32"]),
                            p(out["m16"]), p(out["depthD"]), p(out["hits"]), p(out["depthI"]))
        assert rc == 0, rc
        return out


# ---- the expected frame from the unmodified oracle ---------------------------------------------------------------------------------------------------------------
F32 = np.float32
PASS_BITS = np.array([1e30], F32).view(np.uint32)[0]


def _rows(a, n):
    return np.ascontiguousarray(a).reshape(-1).view(np.uint8).reshape(n, -1)


def _in_image(m, W, H):
    return (m[:, 0] >= 0) & (m[:, 0] < W) & (m[:, 1] >= 0) & (m[:, 1] < H)


def _depth_of(G, idx):
    return G[idx].copy().view(F32)[:, 0]


def expected_frame(o, st, f, cam, vm, checkers=None, gpu=None):
    """frame f on oracle `o` (scene already uploaded).  vm: the checker's output, or a callable(this_g) that returns it (the half-resolution depths need the frame's
    G-buffer, which the probe below delivers).  checkers: None or the `Case` whose GI-spatial / SVGF checkers run (the order of optin.Rig.cpu_frame).  gpu: the
    renderer whose values the inexpressible pixels take.  Returns {"vm", "m_o", "hit", "inexpressible"}; the oracle's buffers hold the expectation afterwards."""
    W, H = st.size.x, st.size.y
    n, Wh, Hh = W * H, W // 2, H // 2
    cur, last = f & 1, (f + 1) & 1
    temporal = st.ReSTIRState in (abi.RESTIR_TEMPORAL, abi.RESTIR_SPATIOTEMPORAL)
    snap = {b: o.readback(b).copy() for b in SAVED}
    o.set_camera(cam)
    # 1. probe: the oracle's own motion index and the hit mask
    o.run_stage(st, f, abi.STAGE_DIRECT)
    m_o = o.readback(abi.BUF_MOTION).view(np.int16).reshape(-1)[:2 * n].reshape(n, 2).astype(np.int32)
    this_g = o.readback(abi.BUF_GBUFFER0 + cur).copy()
    hit = _rows(this_g, n).view(F32)[:, 0] < F32(0.8e28)
    for b, d in snap.items():
        o.upload_history(b, d)
    if callable(vm):
        vm = vm(this_g)
    assert np.array_equal(hit, vm["hits"]["inst"] != MISS)
    pix = np.nonzero(hit)[0]
    t, s = m_o[pix], vm["m32"][pix]
    t_in, s_in = _in_image(t, W, H), _in_image(s, W, H)
    ti, si = t[:, 1] * W + t[:, 0], s[:, 1] * W + s[:, 0]
    G, R, Lid = (_rows(snap[b + last], n) for b in (abi.BUF_GBUFFER0, abi.BUF_DIRECT_RESV0, abi.BUF_LIGHT_ID0))
    # 2. no two hit pixels look at the same place.  (The first frame of a context has no previous camera and an all-zero history: its motion index may collide, and
    # every lookup rejects on the zero depth word whatever it gathers; the read-back checks below hold it to that.)
    empty = not G.any()
    assert empty or np.unique(ti[t_in]).size == int(t_in.sum()), "the oracle's motion index is not injective over the hit pixels"
    IR = _rows(snap[abi.BUF_INDIRECT_RESV0 + last], Wh * Hh)
    # 3. direct stage
    inexpressible = 0
    if temporal:
        accept = s_in & (s[:, 0] >= 2)
        accept[accept] &= vm["depthD"][pix][accept].astype(F32) < (_depth_of(G, si[accept]) * F32(1.05)).astype(F32)
        lost = accept & t_in & (t[:, 0] < 2)      # the oracle cannot be made to accept in columns 0-1
        inexpressible = int(lost.sum())
        assert inexpressible <= 2 * H, inexpressible
        G1, R1, L1 = G.copy(), R.copy(), Lid.copy()
        w = t_in & accept
        G1[ti[w]] = G[si[w]]; R1[ti[w]] = R[si[w]]; L1[ti[w]] = Lid[si[w]]
        G1w = G1.view(np.uint32)
        G1w[ti[w], 0] = PASS_BITS
        G1w[ti[t_in & ~accept], 0] = 0
        assert np.array_equal(G1[ti[w], 4:], G[si[w], 4:]) and (G1w[ti[w], 0] == PASS_BITS).all() and not G1w[ti[t_in & ~accept], 0].any()   # every pixel finds what it wants
        o.upload_history(abi.BUF_GBUFFER0 + last, G1.reshape(-1)); o.upload_history(abi.BUF_DIRECT_RESV0 + last, R1.reshape(-1)); o.upload_history(abi.BUF_LIGHT_ID0 + last, L1.reshape(-1))
    o.run_stage(st, f, abi.STAGE_DIRECT)
    if inexpressible:
        assert gpu is not None and not spatial_mode(st), "inexpressible pixels need the renderer's values (and would spread through spatial reuse)"
        for b in FULL(cur):
            if b == abi.BUF_MOTION:
                continue
            a, g = _rows(o.readback(b).copy(), n), _rows(gpu.readback(b), n)
            a[pix[lost]] = g[pix[lost]]
            o.upload_history(b, a.reshape(-1))
    # 4. indirect stage: the oracle's motion buffer still holds m_o
    if temporal:
        qy, qx = np.meshgrid(np.arange(Hh), np.arange(Wh), indexing="ij")
        full = (2 * qy * W + 2 * qx).reshape(-1)
        q = np.nonzero(hit[full])[0]
        t, s = m_o[full[q]], vm["m16"][full[q]].astype(np.int32)
        t_in, s_in = _in_image(t, W, H), _in_image(s, W, H)
        ti, si = t[:, 1] * W + t[:, 0], s[:, 1] * W + s[:, 0]
        th_in = t_in & (t[:, 0] // 2 < Wh) & (t[:, 1] // 2 < Hh)
        thi, shi = (t[:, 1] // 2) * Wh + t[:, 0] // 2, (s[:, 1] // 2) * Wh + s[:, 0] // 2
        accept = s_in & (s[:, 0] // 2 < Wh) & (s[:, 1] // 2 < Hh)
        accept[accept] &= vm["depthI"][q][accept] < _depth_of(G, si[accept]) * F32(1.1)
        assert empty or np.unique(thi[th_in]).size == int(th_in.sum()), "t / 2 is not injective over the half-resolution pixels"
        assert not (accept & ~th_in).any(), "a half-resolution pixel accepts where the oracle's lookup leaves the half-resolution grid"
        G2, I2 = G.copy(), IR.copy()
        w = th_in & accept
        G2[ti[w]] = G[si[w]]; I2[thi[w]] = IR[shi[w]]
        G2w = G2.view(np.uint32)
        G2w[ti[w], 0] = PASS_BITS
        G2w[ti[t_in & ~accept], 0] = 0
        assert np.array_equal(G2[ti[w], 4:], G[si[w], 4:]) and (G2w[ti[w], 0] == PASS_BITS).all() and not G2w[ti[t_in & ~accept], 0].any()
        o.upload_history(abi.BUF_GBUFFER0 + last, G2.reshape(-1)); o.upload_history(abi.BUF_INDIRECT_RESV0 + last, I2.reshape(-1))
    o.run_stage(st, f, abi.STAGE_INDIRECT)
    # 5. the expected motion buffer and the true history
    mv = vm["m16"].copy()
    mv[~hit] = 0
    mb = np.ascontiguousarray(o.readback(abi.BUF_MOTION)).reshape(-1).view(np.uint8).copy()
    mb[:4 * n] = mv.reshape(-1).view(np.uint8)
    o.upload_history(abi.BUF_MOTION, mb)
    for b in (abi.BUF_GBUFFER0, abi.BUF_DIRECT_RESV0, abi.BUF_LIGHT_ID0, abi.BUF_INDIRECT_RESV0):
        o.upload_history(b + last, snap[b + last])
    # 6. the passes after the indirect stage, as objmotion.composite_frame runs them
    k = checkers
    if k is not None and k.gis.mode != abi.GI_SPATIAL_OFF:
        k.gis_out, img, k.gis_taps = k.kg.run(st, cam, k.gis, o.readback(abi.BUF_GBUFFER0 + cur), o.readback(abi.BUF_INDIRECT_RESV0 + cur), o.readback(abi.BUF_DENOISE_IND_A))
        o.upload_history(abi.BUF_DENOISE_IND_A, img)
    if k is not None and k.den.mode == abi.DENOISER_SVGF:
        out_d, out_i = k.ks.frame(st, cam, f, this_g=o.readback(abi.BUF_GBUFFER0 + cur), last_g=o.readback(abi.BUF_GBUFFER0 + last),
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
    return {"vm": vm, "m_o": m_o, "hit": hit, "inexpressible": inexpressible}


# ---- a deforming, moving scene on both sides -------------------------------------------------------------------------------------------------------------------------
class Case:
    """kind "cornell": the tall box skinned with two joints; "street": the instanced tree mesh (one instance mirrored) skinned and the alpha-tested leaf mesh morphed.
    Actions before a frame: bend(amount) (skin + morph), rows(amount) (rt_update_vertices on a mesh without skin: Cornell's short box / none on the street), move(kind)."""

    def __init__(self, tmp, kind, W, H, gpu=True, overlap=0, traversal=None, restir=abi.RESTIR_TEMPORAL, sky=None, den=None, gis=None, mode=None, scale=None):
        self.kind, self.W, self.H = kind, W, H
        self.sc = refit.cornell() if kind == "cornell" else (refit.street() if scale is None else refit.street(scale))
        self.st = host.default_state(W, H, self.sc, None)
        self.st.environmentProb = 0.0
        self.st.ReSTIRState = restir
        desc = self.sc.desc()
        self.home = refit.instances_of(desc)["objectToWorld"].copy()
        self.extent = float(max(np.abs(np.concatenate(refit.world_bounds(desc, i))).max() for i in range(desc.numInstances)))
        self.pose = self.sc.cameraPose()
        if kind == "street":      # the scene's own camera sees neither subject: this one sees the mirrored instance of the tree mesh and the leaves, and keeps them
            # clear of columns 0-1 through the whole sequence of run_sequence (the instance moves in frame 4)
            self.pose = (np.array([-48.0, 4.0, -1.0], np.float32), np.array([-56.5, 2.0, -2.0], np.float32)) + tuple(self.pose[2:])
        self.verts = skin.vertices_of(desc)
        self.lib = build(tmp)
        chk, mchk = skin.build(tmp), morph.build(tmp)
        self.skinned = skin.SkinnedMesh(chk, desc, skin.deformed_mesh(kind, desc), 2)
        self.morphed = morph.MorphedMesh(mchk, desc, skin.alpha_mesh(desc), 2, 0, seed=5, scale=0.02 * self.extent) if kind == "street" else None
        inst = refit.instances_of(desc)
        self.rows_mesh = int(inst["primMesh"][3]) if kind == "cornell" else None      # Cornell's short box: host rows
        self.movers = [int(skin.instances_of_mesh(desc, self.skinned.mesh)[0])]         # rt_update_instances on an instance of the skinned mesh
        self.o = Oracle(0)
        self.o.upload_scene(desc)
        self.o.resize(W, H)
        self.r = None
        if gpu:
            from restir_amd.renderer import Renderer
            self.r = Renderer().setup(0)
            self.r.set_overlap(overlap)
            self.r.load_scene(desc)
            self.r.update(W, H)
            if traversal is not None:
                self.r.set_traversal(traversal)
            self.r.set_object_motion(abi.OBJECT_MOTION_VERTEX if mode is None else mode)
            self.r.set_skins(*skin.skins_table([self.skinned]))
            if self.morphed is not None:
                self.r.set_morph_targets(*morph.sets_table([self.morphed]))
        self.den, self.gis = den or abi.Denoiser(), gis or abi.GiSpatial()
        self.checked = den is not None or gis is not None
        if self.checked:
            import gi_spatial
            import svgf
            self.gi_lib = gi_spatial.build(tmp)
            self.kg = gi_spatial.GiSpatialChecker(self.gi_lib, desc)
            self.ks = svgf.SvgfChecker(svgf.build(tmp), W, H, self.den)
            self.gis_out = None
            if self.r:
                self.r.set_denoiser(self.den)
                self.r.set_gi_spatial(self.gis)
        if sky is not None:
            self.o.set_sun_and_sky(sky)
            if self.r:
                self.r.set_sun_and_sky(sky)
        self.prev_pos = {}     # prim mesh -> its positions at the last rendered frame, for the meshes deformed since (recorded once)
        self.prev_o2w = {}     # instance -> its objectToWorld at the last rendered frame, for the instances updated since (recorded once)
        self.info = None

    def destroy(self):
        if self.r:
            self.r.destroy()
            self.r = None

    def desc(self):
        return skin.with_vertices(self.sc.desc(), self.verts.copy())

    def camera(self, f, move=0.0):
        eye, center, up, fov = self.pose
        e = np.array(eye, np.float64) + move * f * np.array([1.0, 0.25, -0.75])
        self.sc.setCamera(e.astype(np.float32), center, up, fov)
        self.sc.updateCamera(self.W, self.H)
        return self.sc.getCamera()

    # ---- actions
    def _deformed(self, mesh, first, count, rows):
        self.prev_pos.setdefault(mesh, self.verts["position"][first:first + count].copy())
        self.verts[first:first + count] = rows

    def bend(self, amount):
        """pose the skinned mesh (joint 0 stays, joint 1 leans and twists by `amount`) and, on the street, morph the leaves"""
        sk = self.skinned
        mats = np.stack([skin.affine(), skin.affine(skin.rot("z", 0.15 * amount) @ skin.rot("y", 0.2 * amount), (0.01 * amount * self.extent, 0, 0), sk.centre)])
        self._deformed(sk.mesh, sk.first, sk.count, sk.posed(mats))
        if self.r:
            self.r.update_skins([0], mats)
        if self.morphed is not None:
            mo = self.morphed
            w = np.array([0.5 * amount, -0.25 * amount], np.float32)
            self._deformed(mo.mesh, mo.first, mo.count, mo.morphed(w))
            if self.r:
                self.r.update_morphs([0], w)

    def rows(self, amount):
        """rt_update_vertices: shear the top of Cornell's short box (a mesh without a skin); on the street the skinned mesh's pose comes from bend() instead"""
        if self.rows_mesh is None:
            return self.bend(amount)
        first, count = skin.mesh_range(self.sc.desc(), self.rows_mesh)
        rows = self.verts[first:first + count].copy()
        y = rows["position"][:, 1]
        rows["position"][:, 0] += (np.float32(0.05 * amount) * (y - y.min())).astype(np.float32)
        self._deformed(self.rows_mesh, first, count, rows)
        if self.r:
            self.r.update_vertices(self.rows_mesh, 0, rows)

    def move(self, kind="translate", ids=None):
        ids = self.movers if ids is None else ids
        cur = refit.instances_of(self.sc.desc())["objectToWorld"]
        for i in ids:
            self.prev_o2w.setdefault(int(i), cur[int(i)].copy())
        d = self.desc()
        xf = np.stack([refit.move_matrix(kind, d, i, self.extent, self.home) for i in ids])
        self.sc.updateInstances(np.asarray(ids, np.uint32), np.asarray(xf, np.float32))
        if self.r:
            self.r.update_instances(ids, xf)
            self.r.update_lights(self.sc.desc())

    # ---- a frame
    def previous(self, desc):
        """(prev_pos, mesh_deformed, prev_o2w, inst_moved) of the frame about to be rendered"""
        pm, inst = refit.prim_meshes_of(desc), refit.instances_of(desc)
        pos = self.verts["position"].copy()
        md = np.zeros(desc.numPrimMeshes, np.uint8)
        for m, p in self.prev_pos.items():
            first = int(pm["vertexOffset"][m])
            pos[first:first + len(p)] = p
            md[m] = 1
        o2w = inst["objectToWorld"].copy().reshape(-1, 12)
        im = np.zeros(desc.numInstances, np.uint8)
        for i, P in self.prev_o2w.items():
            if P.tobytes() != inst["objectToWorld"][i].tobytes():
                o2w[i] = P.reshape(12)
                im[i] = 1
        return pos, md, o2w, im

    def frame(self, f, cam=None, time0=1000, render=True):
        """render frame f on both sides; the oracle's buffers hold the expectation afterwards; self.info = expected_frame's result"""
        self.st.time = time0 + f
        cam = cam if cam is not None else self.camera(f)
        desc = self.desc()
        self.o.upload_scene(desc)      # (the oracle keeps its frame buffers across a scene upload: the history carries over)
        if self.checked:
            import gi_spatial
            self.kg = gi_spatial.GiSpatialChecker(self.gi_lib, desc)
        k = VmChecker(self.lib, desc)
        prev = self.previous(desc)
        self.flagged = (prev[1], prev[3])
        self.prev_pos, self.prev_o2w = {}, {}
        if self.r and render:
            self.r.set_camera(cam)
            self.r.run(self.st, f)
        self.info = expected_frame(self.o, self.st, f, cam, lambda g: k.run(self.st, cam, *prev, this_g=g), self if self.checked else None, self.r)
        return cam

    def diff(self, f):
        """{name: differing words} after frame f: the delta image, the instance image and every buffer of helpers.frame_buffers(f); with a checker on, what
        optin.Rig.diff compares for that pass"""
        bad = {}
        vm = self.info["vm"]
        for name, got, want in (("delta", self.r.vertex_motion_readback(), vm["d"]), ("instance_image", self.r.object_motion_readback(), vm["hits"]["inst"])):
            d = optin.words(got, want)
            if d:
                bad[name] = d
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


def run_sequence(case, frames=7, move=0.0):
    """the sequence of the issue — 0: no update, 1: bend, 2: bend further, 3: no update (the mesh stops), 4: bend AND rt_update_instances on the same instance,
    5: two deforming calls before the frame, 6: rt_update_vertices rows (street: another pose).  Yields (f, camera) after each frame."""
    for f in range(frames):
        if f == 1:
            case.bend(1.0)
        elif f == 2:
            case.bend(1.6)
        elif f == 4:
            case.bend(0.8)
            case.move("translate")
        elif f == 5:
            case.bend(0.2)
            case.bend(1.2)
        elif f == 6:
            case.rows(1.0)
        yield f, case.frame(f, case.camera(f, move))
