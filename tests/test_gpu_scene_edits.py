"""Random interleavings of the scene-edit calls against a fresh build (the sweep of tests/scene_edits.py on the GPU).  The calls that change a loaded scene —
rt_update_instances, rt_rebuild_accel, rt_build_accel, rt_set_instances (with and without the emitter mode), rt_update_skins, rt_update_morphs,
rt_update_vertices, rt_set_skins / rt_set_morph_targets, rt_set_light_sources / rt_update_lights, and (seeds 4-6, below) rt_update_materials, rt_update_texture
and rt_set_rebuild_options — share state inside the library (the lazily refreshed host
vertices, the refit state that two calls re-derive and swap, capacities with slack, bindings that name instances by index, one refit tail); each has its own
test file with a hand-written plan.  Here seeded sequences of them run on ONE long-lived context next to a twin that mirrors every edit on the host, and after
every fourth record the context must be what include/rt_abi.h promises: bit for bit a context that uploaded and built the twin's description.  No tolerance
anywhere: results are a function of the triangle set, never of the tree.

At a checkpoint: (1) the device vertices equal the twin's words; (2) rays aimed at the instances touched since the last checkpoint give the same closest hits
and the same any-hits as a fresh context, on both traversal builds, and enough of them hit (a sequence that moved everything out of sight fails); (3) the
instance rows equal the twin's table, a device-built tree passes the structural check, every triangle lies in the boxes above it with the fresh context's
pad, the pad the library reports is that pad, TRI_FLIP of every leaf record is the handedness of its instance (this one after every record), and directly after rt_rebuild_accel / rt_set_instances the tree equals the restated device build word for word;
(4) the light records equal the twin's word for word, whichever way the sequence keeps them current; (5) a frame at 67 x 45 with an orbiting camera equals
the oracle's, which was given the twin's description before that frame.  After the refused record: RT_ERR_INVALID_ARG, and tree, instance rows, vertices,
light records, alpha records and rebuild options read back as before.  Every sequence runs with overlap 0 (all checks) and again with two frames in flight
(vertices, lights, frames).

Seeds 4, 5, 6 (one per light mode) walk the wider alphabet of scene_edits.KINDS_V2: rt_update_materials, rt_update_texture and rt_set_rebuild_options (LBVH / PLOC)
between the other calls — on meshes that have a skin or a morph set, next to rt_update_vertices, the emitter mode's tables, re-binds and light calls, on the host's
alpha records, on a device tree over them and with the templates of rt_set_instances in force.  Their checkpoints add: (6) by globalId the flags and micro-map words
of the leaf records and the alpha record behind every alphaIdx equal a fresh context's (every word, alphaIdx included, while nothing has changed the tree since the
last host build), and every micro-map equals rt_opacity_map of its own alpha record — this one also directly after every materials / texture record, before a
later build can repair a stale word; rt_material_stats after each accepted edit equals the twin's dirtyMaterials and alphaRecords; the tree of (3) is the restated
build of the builder and radius in force (accel_build.rebuilt or ploc.rebuilt), rebuild_stats().iterations > 0 exactly under PLOC, rt_get_rebuild_options reads
back what the twin holds, and rt_instances_stats.reallocated also follows the first PLOC build on the working buffers.  The last three tests run the same machinery
with a driver that forgets to tell the twin of one call (a cutoff edit, a builder switch, a change of PLOC's radius — the last reaches the word-for-word
comparison of the tree) and must end in Case.fail: the sweep sees such a fault.

On a mismatch the case is printed as one line of JSON (scene, seed, ops, the index of the record, the check, the records so far), and
`python tests/test_gpu_scene_edits.py <scene> <seed> [n]` replays that sequence alone.  RESTIR_EDIT_SEEDS (comma separated) and RESTIR_EDIT_OPS widen the
sweep by hand; the defaults are the sequences whose coverage tests/test_scene_edits_cpu.py asserts.

Out of scope: the object and vertex motion modes and the opt-in passes (SVGF, GI spatial, TAA, upscaling) — their reference is a composite or a per-pass
checker, not the plain oracle, and each has a changing-scene case in its own file; rt_resize and rt_upload_scene mid-sequence (they drop the state the sweep
is about); rt_mgpu_* contexts, where rt_set_instances is documented as not done."""
import json
import os
import sys
import tempfile
import time
import numpy as np
import pytest

from helpers import abi, frame_buffers
import accel_build
import blend
import instances
import lights
import materials
import optin
import ploc
import refit
import scene_edits as se
import test_gpu_instances as tgi      # same_rays, expected_tree, diff_tree, tree_of
import test_gpu_materials as tgm      # derived, diff_derived, diff_words, maps_equal_the_host_function
import test_gpu_refit as seq          # renderer

pytestmark = pytest.mark.gpu

SEEDS = [int(x) for x in os.environ.get("RESTIR_EDIT_SEEDS", "").split(",") if x.strip()] or list(se.SEEDS + se.SEEDS_V2)      # (a seed outside se.SEEDS walks KINDS_V2)
OPS = int(os.environ.get("RESTIR_EDIT_OPS", str(se.OPS)))
W, H = se.SIZE
_lib = _ploc = None


def checker(out_dir=None):
    """the CPU restatements of the refit and of the device build (compiled once per process; a replay by hand compiles into a temporary directory)"""
    global _lib, _ploc
    if _lib is None:
        d = out_dir if out_dir is not None else tempfile.mkdtemp(prefix="scene_edits_gpu")
        se.build(d)
        _lib, _ploc = accel_build.build(d), ploc.build(d)
    return _lib


def expected_tree(desc, fresh, options):
    """the restated device build of `desc` with the builder and the radius of `options`, over the records a fresh context host-built for it"""
    if options[0] == ploc.LBVH:
        return tgi.expected_tree(checker(), desc, fresh)
    checker()
    t = ploc.rebuilt(_ploc, desc, tgi.tab.host_tree_of(_ploc, fresh, desc, refit.Tree.built(_ploc, desc)), radius=options[1])
    assert not isinstance(t, int), "the restated PLOC build refuses (%d): tests/test_scene_edits_cpu.py keeps such builds out of the sequences" % t
    return t


@pytest.fixture(scope="module", autouse=True)
def libs(tmp_path_factory):
    return checker(tmp_path_factory.mktemp("scene_edits_gpu"))


class Case:
    """what a failure prints: enough to replay the sequence"""

    def __init__(self, scene, seed, n, overlap, records):
        self.scene, self.seed, self.n, self.overlap, self.records, self.at = scene, seed, n, overlap, records, -1

    def fail(self, check, detail=""):
        line = dict(scene=self.scene, seed=self.seed, ops=self.n, overlap=self.overlap, op=self.at, check=check, records=self.records[:self.at + 1])
        print("MISMATCH", json.dumps(line), detail, flush=True)
        raise AssertionError("%s %d, record %d: %s %s" % (self.scene, self.seed, self.at, check, detail))


def issue(r, call, twin):
    if call.name == "build_accel":
        rc = refit.hip_build_accel(r)
        if rc:
            from restir_amd.renderer import RtError
            raise RtError("rt_build_accel failed (%d)" % rc)
    elif call.name == "update_lights":
        r.update_lights(twin.desc())
    else:
        getattr(r, call.name)(*call.args)


def light_count(desc):
    return int(desc.lightInfo.trigLightSize) if desc.trigLights else 0


def options(r):
    o = r.rebuild_options()
    return [o.builder, o.radius, o.maxIterations, o.reserved]


def state_of(r, twin):
    """everything a refused call must leave alone"""
    d = twin.desc()
    out = [a.tobytes() for a in tgi.tree_of(r, d.numInstances)] + [r.vertices_readback(0, d.numVertices).tobytes()]
    out += [r.accel_readback(abi.ACCEL_ALPHA).tobytes(), repr(options(r)).encode()]
    if light_count(d):
        out.append(r.lights_readback(abi.LIGHTS_TRIG, light_count(d)).tobytes())
    return out


def check_handedness(case, r, twin):
    """TRI_FLIP of every leaf record is the handedness of its instance's matrix in the twin's table.  Cheap, so it runs after every record that changes the tree: a
    record rewritten with the wrong bit is put right by the next build, which may come before the next checkpoint"""
    desc = twin.desc()
    recs = r.accel_readback(abi.ACCEL_TRIS).view(refit.REC_DT)
    if (recs["globalId"] >= len(refit.tri_ref(desc))).any():
        case.fail("handedness", "a globalId beyond the twin's triangle count")
    det = np.array([np.linalg.det(m.reshape(3, 4)[:, :3].astype(np.float64)) for m in twin.table()["objectToWorld"]])
    want = det[refit.tri_ref(desc)[recs["globalId"], 0]] < 0
    got = (recs["flags"] & refit.TRI_FLIP) != 0
    if not np.array_equal(got, want):
        case.fail("handedness", "TRI_FLIP is wrong in %d of %d leaf records" % (int((got != want).sum()), len(recs)))


def check_alpha(case, r, twin, fresh=None):
    """What the material and texel edits re-derive, against a fresh context of the twin's description: by globalId the flags (but TRI_FLIP, which has a check of
    its own) and the micro-map words of the leaf records, and the alpha record each alphaIdx leads to; alphaIdx itself and every other word while both contexts
    number their alpha records alike (nothing has changed the tree since the last host build); every micro-map equals rt_opacity_map of its own alpha record.
    Runs directly after every materials / texture record, as check_handedness does after a tree change: the next build would put a stale word right"""
    own = fresh is None
    if own:
        fresh = seq.renderer(twin.desc())
    try:
        try:
            mine, theirs = tgm.derived(r), tgm.derived(fresh)
        except AssertionError:
            case.fail("alpha records", "the references of one triangle disagree, or alphaIdx != 0 is not TRI_OPAQUE clear")
        if len(mine[0]) != len(theirs[0]):
            case.fail("alpha records", "%d triangles, a fresh context has %d" % (len(mine[0]), len(theirs[0])))
        diff = tgm.diff_derived(mine, theirs)
        if diff != tgm.SAME:
            case.fail("alpha records", "by globalId, against a fresh context: %s" % diff)
        if twin.pristine:
            diff = tgm.diff_words(r, fresh)
            if diff != {"records": 0, "alpha": 0}:
                case.fail("alpha records", "word for word (same tree, same numbering), against a fresh context: %s" % diff)
        try:
            tgm.maps_equal_the_host_function(r, twin._tables_of())
        except AssertionError as e:
            case.fail("micro-maps", "a map is not rt_opacity_map of its alpha record: %s" % str(e)[:300])
    finally:
        if own:
            fresh.destroy()


def check_edit_stats(case, r, call):
    st = r.material_stats()
    if (st.dirtyMaterials, st.alphaRecords) != (call.model["dirty"], call.model["records"]):
        case.fail("material stats", "%s: dirtyMaterials %d, alphaRecords %d; the twin has %d and %d (%s)" % (call.name, st.dirtyMaterials, st.alphaRecords, call.model["dirty"],
                                                                                                         call.model["records"], call.model["state"]))


def checkpoint(case, r, twin, f, since, last, device_built, traversal, want, full):
    """last: the last call that changed the tree (word-for-word equality with the restated device build holds while that is a device build)"""
    desc = twin.desc()
    n_inst = desc.numInstances
    if twin.mode == "update":      # this sequence's way of keeping the light records current
        r.update_lights(desc)
    # 1. vertices
    d = optin.words(r.vertices_readback(0, desc.numVertices), twin.vertices())
    if d:
        case.fail("vertices", "%d words differ" % d)
    # 4. light records
    n = light_count(desc)
    bound = r.light_stats().bound
    if twin.mode != "update" and bound != n:
        case.fail("light records", "bound %d, the twin has %d" % (bound, n))
    if n:
        try:
            got = r.lights_readback(abi.LIGHTS_TRIG, n)
        except Exception as e:      # (the size must be the device's count)
            case.fail("light records", str(e))
        if not np.array_equal(lights.raw(got), lights.raw(lights.records_of(desc))):
            case.fail("light records", "%d words differ" % optin.words(got, lights.records_of(desc)))
    if full:
        L = checker()
        fresh = seq.renderer(desc)
        # 2. rays
        ids, rays = se.aimed_rays(desc, since, case.seed, f)
        try:
            closest = tgi.same_rays(r, fresh, rays)
        except AssertionError as e:
            case.fail("rays", "aimed at the instances %s: closest hits or any-hits differ from a fresh context's (traversal build %s)" % (ids, str(e).splitlines()[0] if str(e) else "?"))
        r.set_traversal(traversal)
        hits, aimed, _ = instances.informative(desc, closest, ids, [])
        if not (hits > 400 and aimed > 20):
            case.fail("rays", "uninformative: %d hit, %d on the instances %s" % (hits, aimed, ids))
        # 3. tree
        nodes, recs, inst = tgi.tree_of(r, n_inst)
        rows = inst.view(np.uint32).reshape(-1, 28)
        table = twin.table()
        if not (np.array_equal(rows[:, :12], table["objectToWorld"].view(np.uint32)) and np.array_equal(rows[:, 24], table["primMesh"]) and np.array_equal(rows[:, 25], table["flags"])):
            case.fail("tree", "the instance rows are not the twin's table")
        dev = refit.Tree(L, desc, nodes, recs, inst, 0.0)
        if device_built:
            dev.depth = r.accel_stats()["max_depth"]
            bad = accel_build.structure(L, dev)
            if bad != (0, ""):
                case.fail("tree", "structure: %s" % (bad,))
        if last in se.DEVICE_BUILDS:
            want_tree = expected_tree(desc, fresh, twin.built_with)
            have = r.accel_stats()["nodes"]
            diff = tgi.diff_tree(r, want_tree, n_inst) if have == want_tree.num_nodes else {"nodes": "%d, the restated build has %d" % (have, want_tree.num_nodes)}
            if diff != tgi.SAME:
                case.fail("tree", "differs from the restated device build (builder %d, radius %d): %s" % (twin.built_with + (diff,)))
        fresh.update_instances([], np.zeros((0, 12), np.float32))      # tells the fresh build's pad; changes no word
        pad = np.float32(fresh.refit_stats().triPad)
        dev.tri_pad = float(pad)
        bad = dev.check()
        if bad != (0, ""):
            case.fail("tree", "containment with the fresh build's pad %g: %s" % (pad, bad))
        mine = r.refit_stats().triPad if last in se.UPDATES else r.rebuild_stats().triPad if last in se.DEVICE_BUILDS else None
        if mine is not None and np.float32(mine) != pad:
            case.fail("tree", "pad %g after %s, a fresh build has %g" % (mine, last, pad))
        if options(r) != twin.options_readback():
            case.fail("options", "rt_get_rebuild_options gives %s, the twin has %s" % (options(r), twin.options_readback()))
        # 6. what the material and texel edits re-derive
        check_alpha(case, r, twin, fresh)
        fresh.destroy()
    # 5. a frame
    cam = twin.camera(f, W, H)
    r.set_camera(cam)
    r.run(twin.st, f)
    bad = {abi.BUFFER_NAMES[b]: optin.words(r.readback(b), want[f][b]) for b in frame_buffers(f)}
    bad = {k: v for k, v in bad.items() if v}
    if bad:
        case.fail("frame %d" % f, str(bad))


def run_sequence(scene, seed, n=OPS, overlap=0, full=True, records=None, forget=()):
    """one sequence on one context; raises AssertionError at the first mismatch (nothing further is started on the GPU).  `records`: a hand-written sequence
    instead of the generated one; `forget`: the indices of its records whose calls reach the context but not the twin — a driver that forgets something, which the
    checks must notice (the two tests at the end of this file)"""
    from restir_amd.renderer import RtError
    if records is not None:
        n = len(records)
    want = se.oracle_frames(scene, seed, n, records, forget)
    twin, records = se.replay(scene, seed, n, records)
    case = Case(scene, seed, n, overlap, records)
    traversal = abi.TRAVERSAL_LATENCY if seed & 1 else abi.TRAVERSAL_THROUGHPUT
    r = seq.renderer(twin.desc(), W, H, overlap, traversal)
    try:
        for call in twin.setup():
            issue(r, call, twin)
            twin.commit(call)
        marks, since, f, device_built, last_tree = se.checkpoints(n), [], 0, False, None
        for i, op in enumerate(records):
            case.at = i
            kind = op[0]
            before = state_of(r, twin) if kind == se.REFUSED else None
            for call in twin.calls(op):
                try:
                    issue(r, call, twin)
                    if call.verdict is not None:
                        case.fail("refused", "%s was accepted; the ABI refuses it: %s" % (call.name, call.verdict))
                except RtError as e:
                    if call.verdict is None:
                        case.fail("accepted", "%s failed: %s" % (call.name, e))
                    if "(%d)" % abi.ERR_INVALID_ARG not in str(e):
                        case.fail("refused", "%s: not RT_ERR_INVALID_ARG: %s" % (call.name, e))
                    continue
                if call.name == "set_instances":
                    if bool(r.instances_stats().reallocated) != call.model["reallocates"]:
                        case.fail("capacity", "reallocated %d, the slack rule and the builder's buffers say %s" % (r.instances_stats().reallocated, call.model["reallocates"]))
                    device_built = True
                elif call.name == "rebuild_accel":
                    device_built = True
                elif call.name == "build_accel":
                    device_built = False
                elif call.name in ("update_materials", "update_texture") and full:
                    check_edit_stats(case, r, call)
                if i not in forget:
                    since += twin.commit(call)
            if kind == se.REFUSED:
                if state_of(r, twin) != before:
                    case.fail("refused", "the refused %s changed the tree, the instance rows, the vertices, the light records, the alpha records or the rebuild options" % op[1]["call"])
            elif kind in se.UPDATES + se.DEVICE_BUILDS + ("build_accel",):
                last_tree = kind
                if full:
                    check_handedness(case, r, twin)
                if kind in se.DEVICE_BUILDS and (r.rebuild_stats().iterations > 0) != (twin.built_with[0] == ploc.PLOC):
                    case.fail("tree", "%d merge iterations; the builder in force is %s" % (r.rebuild_stats().iterations, "PLOC" if twin.built_with[0] == ploc.PLOC else "the LBVH"))
            elif kind in ("materials", "texture") and full and i not in marks:      # (at a mark the checkpoint below does the same, directly after the record too)
                check_alpha(case, r, twin)
            if i in marks:
                checkpoint(case, r, twin, f, since, last_tree, device_built, traversal, want, full)
                since, f = [], f + 1
    finally:
        r.destroy()


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("scene", se.SCENES)
def test_random_scene_edits_equal_a_fresh_build(scene, seed):
    t0 = time.time()
    run_sequence(scene, seed, OPS, 0, True)
    t1 = time.time()
    run_sequence(scene, seed, OPS, 2, False)      # frames in flight
    print("scene edits", scene, seed, "ops", OPS, "overlap 0: %.2f s, overlap 2: %.2f s" % (t1 - t0, time.time() - t1))


# ---- the sweep sees a fault: a driver that forgets one thing ends in Case.fail (these compare words; nothing is provoked on the device) ---------------------------
def test_a_cutoff_edit_the_twin_never_heard_of_is_noticed(capsys):
    twin = se.twin_of("street", 4)
    leaf = twin.hot_materials()[0]
    assert leaf == 40
    was = materials.of_scene(twin.sc).mats[leaf, blend.W_ALPHA_CUTOFF]
    seed = next(s for s in range(64) if twin._rows_for({"kind": "cutoff", "ids": [leaf], "seed": s})[0, blend.W_ALPHA_CUTOFF] != was)      # a cutoff that differs
    records = [("materials", {"kind": "cutoff", "ids": [leaf], "seed": seed}), ("lights", {})]
    with pytest.raises(AssertionError, match="street 4, record [01]: (alpha records|micro-maps|rays)"):
        run_sequence("street", 4, records=records, forget=(0,))
    assert "MISMATCH" in capsys.readouterr().out
    run_sequence("street", 4, records=records)      # (the same records with a driver that forgets nothing pass)


def test_a_builder_switch_the_twin_never_heard_of_is_noticed(capsys):
    records = [("rebuild_options", {"builder": ploc.PLOC, "radius": ploc.DEFAULT_RADIUS}), ("rebuild_accel", {})]
    with pytest.raises(AssertionError, match="street 4, record 1: tree"):
        run_sequence("street", 4, records=records, forget=(0,))
    assert "MISMATCH" in capsys.readouterr().out
    run_sequence("street", 4, records=records)


def test_a_radius_change_the_twin_never_heard_of_is_noticed_by_the_word_for_word_comparison(capsys):
    """PLOC on both sides, so the iteration count says nothing: the comparison with the restated build at the twin's radius is what fails"""
    records = [("rebuild_options", {"builder": ploc.PLOC, "radius": 64}), ("rebuild_options", {"builder": ploc.PLOC, "radius": 1}), ("rebuild_accel", {})]
    with pytest.raises(AssertionError, match="street 4, record 2: tree differs from the restated device build"):
        run_sequence("street", 4, records=records, forget=(1,))
    assert "MISMATCH" in capsys.readouterr().out
    run_sequence("street", 4, records=records)


if __name__ == "__main__":
    scene, seed = sys.argv[1], int(sys.argv[2])
    n = int(sys.argv[3]) if len(sys.argv) > 3 else OPS
    for k, rec in enumerate(se.ops(scene, seed, n)):
        print(k, json.dumps(rec))
    checker()
    run_sequence(scene, seed, n, 0, True)
    run_sequence(scene, seed, n, 2, False)
    print("ok", scene, seed, n)
