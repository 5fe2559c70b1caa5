"""Alpha-blended surfaces on the CPU side: the loader's BLEND mapping, the premise of tests/test_gpu_blend.py — on the veiled scenes of
tests/blend.py the G-buffer of a frame at rest depends on the frame's seed, on the scenes as generated it does not —, the oracle's tree against its brute force
with per-ray seeds, and the distribution of the alpha draw of DESIGN.md §6 deviation 1 held to a binomial bound.

Numbers: 10 % of the texels is the condition that keeps a later edit from making the GPU tests vacuous again (measured: 34 % on veiled Cornell and 22 % on the
veiled street at 70 x 50, 37-48 % / 20-29 % at 13 x 11, 44-52 % / 20-30 % at 8 x 8), not a tolerance; 5 sqrt(p (1 - p) / N) is five standard deviations of a
share of N independent draws.  Everything else is an exact comparison."""
import ctypes as C
import json
import numpy as np
import pytest

from helpers import host
from oracle.binding import Oracle
import blend
import refit

SIZES = [(70, 50), (13, 11), (8, 8)]


# ---- the loader ---------------------------------------------------------------------------------------------------------------------------------------------------
def _modes(sc):
    d = sc.desc()
    g = json.load(open(blend.GLTF))
    mats, inst, pm = blend.materials_of(d), refit.instances_of(d), refit.prim_meshes_of(d)
    assert len(mats) == len(g["materials"]) and len(inst) == len(g["meshes"])
    for k, m in enumerate(g["materials"]):
        want = {"OPAQUE": blend.ALPHA_OPAQUE, "MASK": blend.ALPHA_MASK, "BLEND": blend.ALPHA_BLEND}[m.get("alphaMode", "OPAQUE")]
        assert mats[k, blend.W_ALPHA_MODE] == want, (k, m["name"])
        assert mats[k, blend.W_BASE_ALPHA].view(np.float32) == np.float32(m["pbrMetallicRoughness"]["baseColorFactor"][3]), m["name"]
        assert mats[k, blend.W_BASE_TEXTURE].view(np.int32) == m["pbrMetallicRoughness"].get("baseColorTexture", {"index": -1})["index"], m["name"]
    # every pane goes through the alpha test (the untextured ones too: their factor is not 1); wall and lamp do not
    for i, row in enumerate(inst):
        m = g["materials"][int(pm["materialIndex"][row["primMesh"]])]
        assert bool(row["flags"] & blend.INST_FORCE_OPAQUE) == (m.get("alphaMode", "OPAQUE") == "OPAQUE"), (i, m["name"])
    return mats


def test_loader_maps_blend_and_leaves_the_panes_non_opaque():
    sc, _, d = blend.scene("gltf")
    mats = _modes(sc)
    assert (mats[:, blend.W_ALPHA_MODE] == blend.ALPHA_BLEND).sum() == 6
    assert len(blend.blended_instances(d)) == 6
    tex = np.frombuffer((C.c_char * (d.numTextures * 32)).from_address(d.textures), dtype=np.int32).reshape(-1, 8)
    assert tex[:, 2:7].tolist() == [[16, 8, 10497, 10497, 9729], [4, 4, 33071, 33648, 9728]]      # width, height, wrapS, wrapT, filter


def test_writer_and_loader_keep_the_mode(tmp_path):
    sc, _, d = blend.scene("gltf")
    out = str(tmp_path / "again.gltf")
    assert sc.saveGltf(out)
    assert [m.get("alphaMode") for m in json.load(open(out))["materials"]] == ["OPAQUE"] + ["BLEND"] * 6 + ["OPAQUE"]
    sc2 = host.Scene()
    assert sc2.load(out)
    _modes(sc2)
    d2 = sc2.desc()
    assert np.array_equal(blend.materials_of(d)[:, :19], blend.materials_of(d2)[:, :19])
    assert np.array_equal(refit.instances_of(d)["flags"], refit.instances_of(d2)["flags"])


def test_veil_blends_what_it_says_and_nothing_else():
    for name in blend.SCENES:
        sc, plain, veiled = blend.scene(name)
        a, b = blend.materials_of(plain), blend.materials_of(veiled)
        changed = np.nonzero((a != b).any(axis=1))[0]
        emits = (a[:, blend.W_EMISSIVE].view(np.float32) != 0).any(axis=1)
        assert not emits[changed].any() and len(changed) >= len(a[~emits]) // 2
        assert (b[changed, blend.W_ALPHA_MODE] == blend.ALPHA_BLEND).all() and (b[:, blend.W_ALPHA_MODE] != blend.ALPHA_MASK)[~emits].all()
        assert (b[changed, blend.W_BASE_ALPHA].view(np.float32) == 0.5).all()
        cols = np.ones(20, bool)
        cols[[blend.W_BASE_ALPHA, blend.W_ALPHA_MODE]] = False
        assert np.array_equal(a[:, cols], b[:, cols])
        ia, ib = refit.instances_of(plain), refit.instances_of(veiled)
        assert np.array_equal(ia["objectToWorld"], ib["objectToWorld"]) and np.array_equal(ia["primMesh"], ib["primMesh"])
        assert np.array_equal(ia["flags"] & ~np.uint32(1), ib["flags"] & ~np.uint32(1))
        assert len(blend.blended_instances(veiled)) > 0 and len(blend.blended_instances(plain)) == 0
        # the light records are the scene's
        assert veiled.trigLights == plain.trigLights and bytes(veiled.lightInfo) == bytes(plain.lightInfo)
    # the street keeps its bilinear alpha textures under blended materials
    sc, plain, veiled = blend.scene("street")
    b = blend.materials_of(veiled)
    assert ((b[:, blend.W_ALPHA_MODE] == blend.ALPHA_BLEND) & (b[:, blend.W_BASE_TEXTURE].view(np.int32) >= 0)).any()


# ---- the premise ------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", blend.SCENES)
def test_a_veiled_frame_at_rest_depends_on_its_seed_and_a_plain_one_does_not(name):
    sc, plain, veiled = blend.scene(name)
    o = Oracle(0)
    for w, h in SIZES:
        o.upload_scene(plain)
        same = blend.changing_texels(o, sc, w, h)
        o.upload_scene(veiled)
        moving = blend.changing_texels(o, sc, w, h)
        print(name, (w, h), "plain", same, "veiled", moving, "of", w * h)
        assert same == [0] * 7, (name, w, h)
        assert len(moving) == 7 and min(moving) >= 0.10 * w * h, (name, w, h, moving)


def test_the_fixture_at_rest_depends_on_its_seed():
    sc, _, d = blend.scene("gltf")
    o = Oracle(0)
    o.upload_scene(d)
    for w, h in SIZES:
        moving = blend.changing_texels(o, sc, w, h)
        print("gltf", (w, h), moving, "of", w * h)
        assert min(moving) >= 0.10 * w * h, (w, h, moving)


# ---- tree against brute force --------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", blend.SCENES + ("gltf",))
def test_oracle_tree_equals_oracle_brute_force_with_random_seeds(name):
    sc, _, veiled = blend.scene(name)
    o = Oracle(0)
    o.upload_scene(veiled)
    rays = blend.random_rays(veiled, 1 << 16, 23)
    tree, brute = o.trace_closest(rays), o.trace_closest(rays, brute=True)
    hit = brute[:, 0] < 1e27
    print(name, "hit share", hit.mean())
    assert hit.mean() > 0.1            # (not vacuous; half of the rays are aimed at blended instances)
    assert np.array_equal(tree.view(np.uint32), brute.view(np.uint32)), int((tree.view(np.uint32) != brute.view(np.uint32)).any(axis=1).sum())
    if name != "gltf":
        # the seeds matter: the same rays with other seeds stop elsewhere
        other = rays.copy()
        other[:, 7] = (rays[:, 7].view(np.uint32) ^ np.uint32(0x2545f491)).view(np.float32)
        assert (o.trace_closest(other).view(np.uint32) != tree.view(np.uint32)).any(axis=1).mean() > 0.01


# ---- the draw's distribution ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("alpha", [0.25, 0.5, 0.7])
def test_the_alpha_draw_accepts_with_probability_alpha(alpha):
    sc = refit.cornell()
    o = Oracle(0)
    o.upload_scene(blend.all_blended(sc, alpha))
    blend.check_distribution(o.trace_closest, alpha)
    blend.check_distribution(lambda rays: o.trace_closest(rays, brute=True), alpha)


# ---- the micro-map check of tests/test_gpu_blend.py rejects a wrong map ---------------------------------------------------------------------------------------------------
def test_the_micro_map_check_rejects_wrong_maps():
    """records made here, not by the library: an all-unknown map passes on every triangle; "accepts everywhere" fails on every blended triangle whose opacity
    is below 1 somewhere, "opacity 0 everywhere" on every one whose opacity is above 0 somewhere — and passes on the pane whose alpha factor is exactly 0"""
    sc, _, d = blend.scene("gltf")
    ids = np.nonzero(np.isin(refit.tri_ref(d)[:, 0], blend.blended_instances(d)))[0]
    recs = np.zeros(len(ids), refit.REC_DT)
    recs["globalId"] = ids
    assert len(ids) == 12
    bad, seen = blend.micro_map_violations(d, recs)
    assert bad == [] and seen[(blend.ALPHA_BLEND, 0)] == 12 * 36
    recs["omm"] = 0x55555555          # state 1 in every cell
    bad, _ = blend.micro_map_violations(d, recs)
    assert {b[0] for b in bad} == set(int(i) for i in ids)
    recs["omm"] = 0xaaaaaaaa          # state 2 in every cell
    bad, _ = blend.micro_map_violations(d, recs)
    inst, pm = refit.instances_of(d), refit.prim_meshes_of(d)
    zero = {int(g) for g in ids if blend.materials_of(d)[pm["materialIndex"][inst["primMesh"][refit.tri_ref(d)[g, 0]]], blend.W_BASE_ALPHA].view(np.float32) == 0}
    assert len(zero) == 2 and {b[0] for b in bad} == set(int(i) for i in ids) - zero
    # the alpha ramp's pane: the cells over its columns of exact 0 may be called empty, no other cell of it
    ramp = [b for b in bad if b[0] == int(ids[0])]
    assert 0 < len(ramp) < 36
