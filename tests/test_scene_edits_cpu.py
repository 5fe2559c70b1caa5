"""The scene-edit sweep without a GPU (tests/scene_edits.py): the generator is deterministic, emits only calls the ABI accepts plus the one refused call per
sequence, and the default sequences of tests/test_gpu_scene_edits.py contain every kind, every ordered pair of the ten non-refused kinds, a table change that
reallocates and one that fits, an emitter that moves; the rays of every checkpoint are informative and the frames of a Cornell sequence change from checkpoint
to checkpoint (the oracle's ray and frame code on the CPU).

The wider family (seeds 4-6, scene_edits.KINDS_V2): the old family's records still have the digest they had before the alphabet was widened; the six wider
sequences contain all 69 ordered pairs with a material edit, a texel edit or a builder switch on a side, every material kind, rectangles that change alpha and one
that does not, edits that re-derive records in every state of the tree (host records, a device tree over them, templates in force), on a deformed mesh and in
Cornell after a flip, both builders at a rebuild and at a table change, a refit of a PLOC tree, an emission row in every light mode, a refusal of each new call;
no PLOC build of theirs is one the builder refuses; the twin's reallocation model restates the builder-switching rule; the oracle sees an edited row and an
edited texel of a street sequence."""
import numpy as np
import pytest

from helpers import abi
import blend
import instances
import materials
import optin
import ploc
import scene_edits as se

@pytest.fixture(scope="module", autouse=True)
def libs(tmp_path_factory):
    return se.build(tmp_path_factory.mktemp("scene_edits"))


DEFAULT = [(scene, seed) for scene in se.SCENES for seed in se.SEEDS]      # exactly the cases tests/test_gpu_scene_edits.py runs by default
DEFAULT_V2 = [(scene, seed) for scene in se.SCENES for seed in se.SEEDS_V2]      # ... and the wider family's
# sha256 of json.dumps([[scene, seed, se.ops(scene, seed)] for DEFAULT], sort_keys=True), recorded on the commit before the alphabet was widened
OLD_RECORDS = "cb0bf619457837ff1e026bbc65a6612287033fc62ec44682a8ce5de531a24310"


def walk(scene, seed, n=se.OPS):
    """(index, kind, args, calls, touched instances, the twin after the record) over a replay of a sequence"""
    t, records = se.replay(scene, seed, n)
    for call in t.setup():
        assert call.verdict is None, call
        t.commit(call)
    for i, (kind, args) in enumerate(records):
        calls, touched = t.apply((kind, args))
        yield i, kind, args, calls, touched, t


@pytest.mark.parametrize("scene,seed", DEFAULT + DEFAULT_V2 + [("cornell", 11), ("street", 12), ("street", 13)])
def test_the_same_seed_gives_the_same_records(scene, seed):
    a, b = se.ops(scene, seed), se.ops(scene, seed)
    assert a == b and len(a) == se.OPS
    se._ops.clear(); se._plans.clear()      # ... also when they are drawn again from nothing
    assert se.ops(scene, seed) == a
    assert se.ops(scene, seed, 9) == se.ops(scene, seed, 9) and len(se.ops(scene, seed, 9)) == 9


@pytest.mark.parametrize("scene,seed", DEFAULT + DEFAULT_V2 + [("cornell", 11), ("street", 12), ("street", 13)])
def test_every_record_passes_its_verdict_and_the_refused_one_fails_it(scene, seed):
    refused = 0
    for i, kind, args, calls, touched, t in walk(scene, seed):
        assert calls, (i, kind)
        if kind == se.REFUSED:
            refused += 1
            assert len(calls) == 1 and calls[0].verdict is not None, (i, args)
        else:
            assert all(c.verdict is None for c in calls), (i, kind, args, [c.verdict for c in calls])
        assert np.isfinite(t.vertices()["position"]).all() and t.desc().numInstances >= 1
    assert refused == 1


def test_the_default_sequences_cover_the_alphabet():
    """a condition, not a measurement: a change of the generator that thins the sweep fails here"""
    kinds, pairs, reallocs, moved_emitter, poses, weights, hows, refusals, empty_updates = set(), set(), set(), set(), set(), set(), set(), set(), 0
    for scene, seed in DEFAULT:
        prev = None
        for i, kind, args, calls, touched, t in walk(scene, seed):
            kinds.add(kind)
            if prev is not None and se.REFUSED not in (prev, kind):
                pairs.add((prev, kind))
            prev = kind
            for c in calls:
                if c.name == "set_instances" and c.verdict is None:
                    reallocs.add(bool(c.model["reallocates"]))
            if kind == "update_instances":
                empty_updates += not args["ids"]
                if set(args["ids"]) & set(t.emitting()):
                    moved_emitter.add(scene)
            if kind == "update_skins":
                poses.add(args["pose"])
            if kind == "update_morphs":
                weights.add(sum(w != 0 for w in args["weights"]) if len(args["weights"]) > 1 else -sum(w != 0 for w in args["weights"]))
            if kind == "set_instances":
                hows.add(args["how"])
            if kind == se.REFUSED:
                refusals.add(args["call"])
    assert kinds == set(se.KINDS) | {se.REFUSED}
    assert pairs == {(a, b) for a in se.KINDS for b in se.KINDS}, sorted({(a, b) for a in se.KINDS for b in se.KINDS} - pairs)
    assert reallocs == {True, False}
    assert moved_emitter == set(se.SCENES)
    assert empty_updates >= 1 and len(poses) >= 3 and hows >= {"append", "delete", "shrink", "grow"} and len(refusals) >= 3
    assert 0 in {abs(w) for w in weights} and 1 in weights      # no active target; a single active target of several
    assert sorted(se.mode_of(seed) for seed in se.SEEDS) == sorted(se.MODES)


@pytest.mark.parametrize("scene,seed", DEFAULT + DEFAULT_V2)
def test_the_rays_of_every_checkpoint_are_informative(scene, seed):
    """the counts tests/test_gpu_scene_edits.py asserts on the GPU's hits: the oracle's ray code traces the same rays on the CPU"""
    from oracle.binding import Oracle
    marks, since, f = se.checkpoints(se.OPS), [], 0
    for i, kind, args, calls, touched, t in walk(scene, seed):
        since += touched
        if i in marks:
            desc = t.desc()
            ids, rays = se.aimed_rays(desc, since, seed, f)
            o = Oracle(0)
            o.upload_scene(desc)
            hits, aimed, _ = instances.informative(desc, o.trace_closest(rays), ids, [])
            assert hits > 400 and aimed > 20, (i, ids, hits, aimed)
            since, f = [], f + 1


def test_the_oracle_sees_the_edits_of_a_cornell_sequence():
    frames = se.oracle_frames("cornell", 1)
    assert len(frames) == len(se.checkpoints(se.OPS)) == 6
    for f, bufs in enumerate(frames):
        img = bufs[abi.BUF_DIRECT_RESULT0 + (f & 1)].view(np.float32)
        assert np.isfinite(img).all() and img.max() > 0, f
    g = [frames[f][abi.BUF_GBUFFER0 + (f & 1)] for f in range(len(frames))]
    assert all(optin.words(g[f], g[f + 1]) > 0 for f in range(len(g) - 1))


# ---- the wider family (KINDS_V2: rt_update_materials, rt_update_texture, rt_set_rebuild_options) -----------------------------------------------------------
def test_the_old_family_draws_the_records_it_drew_before_the_alphabet_was_widened():
    import hashlib
    import json
    records = [[scene, seed, se.ops(scene, seed)] for scene, seed in DEFAULT]
    assert hashlib.sha256(json.dumps(records, sort_keys=True).encode()).hexdigest() == OLD_RECORDS
    assert all(kind in se.KINDS + (se.REFUSED,) for _, _, ops in records for kind, _ in ops)
    assert se.KINDS_V2 == se.KINDS + ("materials", "texture", "rebuild_options") and se.SEEDS_V2 == (4, 5, 6)
    assert sorted(se.mode_of(seed) for seed in se.SEEDS_V2) == sorted(se.MODES)
    assert len(se.pairs_v2()) == 69
    for seed in (0, 7, 11):      # every seed outside SEEDS walks the wider alphabet
        assert se.kinds_of_seed(seed) == se.KINDS_V2 and set(k for k, _ in se.ops("cornell", seed)) & set(se.NEW_KINDS)


def alpha_tested(row):
    """a material row that is more than a plain opaque one: MASK or BLEND, or a base alpha below 1"""
    return int(row[blend.W_ALPHA_MODE]) != blend.ALPHA_OPAQUE or row[blend.W_BASE_ALPHA].view(np.float32) < 1


def test_the_wider_sequences_meet_their_coverage_conditions():
    """conditions, not measurements (the states are those of scene_edits.Twin.tree)"""
    pairs, mat_kinds, rect_kinds, refusals, builds = set(), set(), set(), set(), set()
    edits = {scene: [] for scene in se.SCENES}      # the state of the tree at every edit that predicts alphaRecords > 0
    texel_dirty = texel_clean = deformed = refits_on_ploc = cornell_tested = 0
    word_for_word = {scene: 0 for scene in se.SCENES}      # edits after which the context's tree is still the last host build's: every word is compared
    refused_why = set()
    emission = {mode: [] for mode in se.MODES}      # per light mode: (scale, the calls) of the rows that change an emission inside the light rule
    for scene, seed in DEFAULT_V2:
        prev = None
        for i, kind, args, calls, touched, t in walk(scene, seed):
            if prev is not None and se.REFUSED not in (prev, kind):
                pairs.add((prev, kind))
            prev = kind
            model = calls[0].model
            if kind == "materials":
                mat_kinds.add(args["kind"])
                if args["kind"] == "emission":
                    emission[t.mode].append((args["scale"], [c.name for c in calls]))
            if kind == "texture":
                rect_kinds.add(args["kind"])
                texel_dirty += model["dirty"] > 0 and model["records"] > 0
                texel_clean += args["kind"] == "same_alpha" and (model["dirty"], model["records"]) == (0, 0)
            if kind in ("materials", "texture"):
                word_for_word[scene] += model["pristine"] and (scene == "cornell" or model["records"] > 0)
            if kind in ("materials", "texture") and model["records"] > 0:
                edits[scene].append(model["state"])
                deformed += scene == "street" and bool(set(model["materials"]) & set(model["deformed"]))
                rows = blend.materials_of(t.desc())
                cornell_tested += scene == "cornell" and any(alpha_tested(rows[m]) for m in model["materials"] if m in t.hot_materials())
            if kind in se.DEVICE_BUILDS:
                builds.add((t.built_with[0], "rebuild" if kind == "rebuild_accel" else "table"))
            if kind in se.UPDATES and t.built_with is not None:
                refits_on_ploc += t.built_with[0] == ploc.PLOC
            if kind == se.REFUSED:
                refusals.add(args["call"])
                refused_why.add((t.mode, args["call"], args["why"]))
    assert pairs >= se.pairs_v2(), sorted(se.pairs_v2() - pairs)
    assert mat_kinds == set(materials.MATERIAL_KINDS) | {"emission"}
    # an emission changes: the checkpoint's rt_update_lights carries it ("update"), rt_update_lights follows the row ("binding"); the emitter mode takes the row of
    # an emissive material only while the luminance keeps its bits
    assert any(scale != 1 and names == ["update_materials"] for scale, names in emission["update"]), emission
    assert emission["binding"] and all(scale != 1 and names == ["update_materials", "update_lights"] for scale, names in emission["binding"]), emission
    assert emission["emitter"] and all(scale == 1 and names == ["update_materials"] for scale, names in emission["emitter"]), emission
    assert len(rect_kinds) >= 4 and texel_dirty >= 1 and texel_clean >= 1, (rect_kinds, texel_dirty, texel_clean)
    assert len(edits["street"]) >= 3 and set(edits["street"]) == {"host", "rebuilt", "templates"}, edits
    assert len(edits["cornell"]) >= 1 and cornell_tested >= 1, (edits, cornell_tested)
    assert deformed >= 1
    assert builds == {(b, what) for b in (ploc.LBVH, ploc.PLOC) for what in ("rebuild", "table")}, builds
    assert refits_on_ploc >= 1
    assert refusals >= {"materials", "texture", "rebuild_options"}, refusals
    assert ("emitter", "materials", "emitter_luminance") in refused_why, refused_why      # the refusal only the emitter mode has
    assert all(n >= 1 for n in word_for_word.values()), word_for_word      # (on the street: of an edit that re-derives records)


def test_a_first_ploc_build_on_the_working_buffers_reallocates():
    """the rule tests/test_gpu_ploc.py::test_switching_builders_on_one_context shows on the GPU, in the twin's model: the same table five times"""
    t = se.Twin("street", "update", wide=True)
    seen = []
    for builder in (ploc.LBVH, ploc.PLOC, ploc.LBVH, ploc.PLOC, ploc.PLOC):
        t.commit(t._set_rebuild_options(builder))
        call = t._set_instances(t.table())
        seen.append(call.model["reallocates"])
        t.commit(call)
    assert seen == [True, True, False, False, False]
    t.commit(se.Call("build_accel", (), None, None))      # a host build drops the buffers; the options stay
    assert t.options[0] == ploc.PLOC and t._set_instances(t.table()).model == {"reallocates": True, "fits": False} and not t.ploc_buffers


def test_no_ploc_build_of_the_wider_sequences_is_one_the_builder_refuses(tmp_path):
    """a sequence must not run into the depth or the iteration limit: the restated PLOC build of every device build under PLOC succeeds"""
    import refit
    L = ploc.build(tmp_path)
    built = 0
    for scene, seed in DEFAULT_V2:
        for i, kind, args, calls, touched, t in walk(scene, seed):
            if kind in se.DEVICE_BUILDS and t.built_with[0] == ploc.PLOC:
                desc = t.desc()
                tree = ploc.rebuilt(L, desc, refit.Tree.built(L, desc), radius=t.built_with[1])
                assert not isinstance(tree, int) and tree.iterations > 0, (scene, seed, i, tree)
                built += 1
    assert built >= 2


def street_edit_records(t):
    """eight hand-written records over the street twin `t`: four material rows, then four texel rectangles, all on materials in view"""
    big = int(t.material_of_mesh()[0])      # the material of the largest prim mesh
    tex = int(blend.materials_of(t.desc())[big, blend.W_BASE_TEXTURE].view(np.int32))
    assert tex >= 0
    rows = [("materials", {"kind": k, "ids": [big], "seed": 5 + n}) for n, k in enumerate(("colour", "roughness", "colour", "base_alpha"))]
    rects, seed = [], 0
    for k in ("full_width", "padded", "full_width", "full_width"):
        while int(materials.draw(t._tables_of(big), np.random.default_rng([seed, 0]), k)["texture"]) != tex:
            seed += 1
        rects.append(("texture", {"kind": k, "texture": tex, "material": big, "seed": seed}))
        seed += 1
    return rows + rects


def test_the_oracle_sees_an_edited_row_and_an_edited_texel_of_a_street_sequence():
    """a street sequence of the wider family whose two checkpoints follow four material rows and four texel rectangles and nothing else: each frame differs from
    the frame of the twin that did not follow those four records (same camera, same earlier history)"""
    records = street_edit_records(se.twin_of("street", 5))
    frames = se.oracle_frames("street", 5, records=records)
    no_rows = se.oracle_frames("street", 5, records=records, forget=(0, 1, 2, 3))
    no_texels = se.oracle_frames("street", 5, records=records, forget=(4, 5, 6, 7))
    assert len(frames) == 2

    def differ(a, b, f):
        return sum(optin.words(a[f][x + (f & 1)], b[f][x + (f & 1)]) for x in (abi.BUF_GBUFFER0, abi.BUF_DIRECT_RESULT0))

    assert differ(frames, no_rows, 0) > 0 and differ(frames, no_texels, 0) == 0 and differ(frames, no_texels, 1) > 0
    # ... and a generated sequence of the family renders: the frames are finite and lit
    for f, bufs in enumerate(se.oracle_frames("street", 5)):
        img = bufs[abi.BUF_DIRECT_RESULT0 + (f & 1)].view(np.float32)
        assert np.isfinite(img).all() and img.max() > 0, f
