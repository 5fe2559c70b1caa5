"""The CPU restatement of the device build with a builder selector (tests/ploc_checker.cpp).  With the LBVH selector it equals tests/accel_build_checker.cpp word for
word, which pins its restated collapse to the one the device is already held to; with PLOC it builds sound, well-formed, reproducible trees at every
radius on every scene of the rebuild tests and three of its own, the iteration cap refuses exactly where it should, and on `street` the tree's SAH sums are strictly
below the LBVH tree's.  No GPU: this pins the algorithm the device's PLOC builder is held to word for word (tests/test_gpu_ploc.py)."""
import numpy as np
import pytest

import accel_build
import ploc
import refit


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    return ploc.build(tmp_path_factory.mktemp("ploc"))


@pytest.fixture(scope="module")
def hosts(lib):
    """name -> (scene, desc, host tree), built once and left unchanged"""
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = ploc.host_tree(lib, name)[:3]
        return cache[name]
    return get


@pytest.mark.parametrize("name", accel_build.SCENES)
def test_lbvh_selector_equals_the_old_checker_word_for_word(lib, hosts, name):
    _, desc, host = hosts(name)
    a = accel_build.rebuilt(lib, desc, host)
    b = ploc.rebuilt(lib, desc, host, builder=ploc.LBVH)
    assert np.array_equal(a.nodes, b.nodes) and np.array_equal(a.recs, b.recs) and a.depth == b.depth and b.iterations == 0


@pytest.mark.parametrize("radius", ploc.RADII)
@pytest.mark.parametrize("name", ploc.SCENES)
def test_ploc_tree_is_sound_well_formed_and_reproducible(lib, hosts, name, radius):
    _, desc, host = hosts(name)
    n = host.ref.shape[0]
    t = ploc.rebuilt(lib, desc, host, radius=radius, max_iterations=max(n, 1))
    assert not isinstance(t, int), t
    assert accel_build.structure(lib, t) == (0, "")
    assert sorted(t.records()["globalId"].tolist()) == list(range(n))
    assert t.depth <= accel_build.STACK_MAX
    assert t.moved.all() and t.check() == (0, "")          # rfc_check_tree: every record inside its leaf slot's box, every box inside its parent's
    assert t.iterations <= max(n - 1, 0) and (t.iterations > 0) == (n > 1)
    u = ploc.rebuilt(lib, desc, host, radius=radius, max_iterations=max(n, 1))
    assert np.array_equal(t.nodes, u.nodes) and np.array_equal(t.recs, u.recs) and (t.depth, t.iterations) == (u.depth, u.iterations)
    # the iteration cap: one short is refused, exactly enough is not
    if t.iterations > 0:
        assert ploc.rebuilt(lib, desc, host, radius=radius, max_iterations=t.iterations - 1) == ploc.REFUSED_ITERATIONS
        v = ploc.rebuilt(lib, desc, host, radius=radius, max_iterations=t.iterations)
        assert np.array_equal(t.nodes, v.nodes) and np.array_equal(t.recs, v.recs)


def test_shapes_of_the_tiny_scenes(lib, hosts):
    """the scenes do what they were made for"""
    it = {(name, r): ploc.rebuilt(lib, hosts(name)[1], hosts(name)[2], radius=r, max_iterations=600).iterations for name in ploc.TINY for r in (1, 2, 64)}
    print(it)
    assert all(it[("nested40", r)] == 39 for r in (1, 2, 64))      # one merge per iteration: everyone prefers the smallest
    for r in ploc.RADII:
        # row600: the Morton order is the order the triangles were laid out in, and the pairs at the block boundaries choose each other in the first iteration;
        # the window is clipped at both ends (the first and the last position have one side only)
        order, nn, _, _ = ploc.inspect(lib, hosts("row600")[1], hosts("row600")[2], r)
        assert np.array_equal(order, np.arange(600)), r
        assert [int(nn[k]) for k in (255, 256, 511, 512)] == [256, 255, 512, 511], r
        assert nn[0] >= 1 and nn[599] <= 598 and np.all(np.abs(nn.astype(np.int64) - np.arange(600)) <= r) and np.all(nn != np.arange(600)), r
        # nested40: the order is by size; the union with any smaller box is the cluster's own box, so every distance below it ties and the tie-break picks the
        # lowest position of the window — only positions 0 and 1 choose each other
        order, nn, _, _ = ploc.inspect(lib, hosts("nested40")[1], hosts("nested40")[2], r)
        assert np.array_equal(order, np.arange(40)) and nn[0] == 1 and np.array_equal(nn[1:], np.maximum(np.arange(1, 40) - r, 0)), r
        # two_far: the clumps are apart in the Morton order, and the root's children are exactly the two clumps — so every merge but the last stayed inside a
        # clump: each clump was one cluster before any merge across them (a merge across them earlier would leave a child of the root holding both)
        order, _, final, left = ploc.inspect(lib, hosts("two_far")[1], hosts("two_far")[2], r)
        assert sorted(order[:20].tolist()) == list(range(20)) and sorted(order[20:].tolist()) == list(range(20, 40)), r
        assert left == 20 and sorted(final[:20].tolist()) == list(range(20)) and sorted(final[20:].tolist()) == list(range(20, 40)), r


def test_ploc_lowers_the_sah_sums_on_street(lib, hosts):
    rows = {}
    for name in ("cornell", "street", "row600"):
        _, desc, host = hosts(name)
        a = ploc.rebuilt(lib, desc, host, builder=ploc.LBVH)
        row = {"lbvh": (a.sah_node, a.sah_tri, a.num_nodes, a.depth, 0)}
        for r in (8, 16, 32, 64):
            b = ploc.rebuilt(lib, desc, host, radius=r, max_iterations=host.ref.shape[0])
            row[r] = (b.sah_node, b.sah_tri, b.num_nodes, b.depth, b.iterations)
        rows[name] = row
        for k, v in row.items():
            print("%-8s %-5s sahNode %9.3f sahTri %9.3f sum %9.3f nodes %5d depth %2d iterations %3d" % (name, k, v[0], v[1], v[0] + v[1], v[2], v[3], v[4]))
    lb, pl = rows["street"]["lbvh"], rows["street"][ploc.DEFAULT_RADIUS]
    assert pl[0] + pl[1] < lb[0] + lb[1]
