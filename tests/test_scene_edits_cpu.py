"""The scene-edit sweep without a GPU (tests/scene_edits.py): the generator is deterministic, emits only calls the ABI accepts plus the one refused call per
sequence, and the default sequences of tests/test_gpu_scene_edits.py contain every kind, every ordered pair of the ten non-refused kinds, a table change that
reallocates and one that fits, an emitter that moves; the rays of every checkpoint are informative and the frames of a Cornell sequence change from checkpoint
to checkpoint (the oracle's ray and frame code on the CPU)."""
import numpy as np
import pytest

from helpers import abi
import instances
import optin
import scene_edits as se

@pytest.fixture(scope="module", autouse=True)
def libs(tmp_path_factory):
    return se.build(tmp_path_factory.mktemp("scene_edits"))


DEFAULT = [(scene, seed) for scene in se.SCENES for seed in se.SEEDS]      # exactly the cases tests/test_gpu_scene_edits.py runs by default


def walk(scene, seed, n=se.OPS):
    """(index, kind, args, calls, touched instances, the twin after the record) over a replay of a sequence"""
    t, records = se.replay(scene, seed, n)
    for call in t.setup():
        assert call.verdict is None, call
        t.commit(call)
    for i, (kind, args) in enumerate(records):
        calls, touched = t.apply((kind, args))
        yield i, kind, args, calls, touched, t


@pytest.mark.parametrize("scene,seed", DEFAULT + [("cornell", 11), ("street", 12), ("street", 13)])
def test_the_same_seed_gives_the_same_records(scene, seed):
    a, b = se.ops(scene, seed), se.ops(scene, seed)
    assert a == b and len(a) == se.OPS
    se._ops.clear(); se._plans.clear()      # ... also when they are drawn again from nothing
    assert se.ops(scene, seed) == a
    assert se.ops(scene, seed, 9) == se.ops(scene, seed, 9) and len(se.ops(scene, seed, 9)) == 9


@pytest.mark.parametrize("scene,seed", DEFAULT + [("cornell", 11), ("street", 12), ("street", 13)])
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


@pytest.mark.parametrize("scene,seed", DEFAULT)
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
