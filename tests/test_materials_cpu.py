"""Material and texture edits without a GPU: rt_opacity_map, the host statement of the micro-map rule of csrc/opacity_map.h, on the edge scene of
tests/materials.py against blend.py's float64 check; the conditions the edge scene's inputs must meet; the edit generator's coverage; the new struct sizes; and the
rule's header under AddressSanitizer + UndefinedBehaviorSanitizer in a program of its own (tests/materials_san_main.cpp).  tests/test_gpu_materials.py holds the
HIP kernels to the same function word for word."""
import ctypes as C
import os
import subprocess
import numpy as np

from helpers import abi, ROOT
import blend
import materials
import refit


def edge_maps(t):
    """[(material, uv, omm)] of every alpha-tested triangle of the edge scene, by rt_opacity_map"""
    return [(m, uv, materials.opacity_map(t, m, uv)) for m, uv, _ in materials.triangle_inputs(t)]


def test_opacity_map_on_the_edge_scene_is_sound_against_float64():
    t = materials.edge()
    desc = t.desc()
    maps = edge_maps(t)
    assert len(maps) == 30
    recs = np.zeros(len(maps), refit.REC_DT)
    recs["globalId"] = np.arange(len(maps))          # the alpha-tested instances come first in the table, in (instance, triangle) order
    recs["omm"] = np.stack([o for _, _, o in maps])
    ref = refit.tri_ref(desc)
    pm = refit.prim_meshes_of(desc)
    assert [max(0, int(pm["materialIndex"][refit.instances_of(desc)["primMesh"][ref[g, 0]]])) for g in range(len(maps))] == [m for m, _, _ in maps]
    finite = np.array([np.isfinite(uv).all() for _, uv, _ in maps])      # (the float64 sampler has no answer for a non-finite texcoord; those maps are all-unknown, below)
    bad, seen = blend.micro_map_violations(desc, recs[finite])
    print(seen)
    assert bad == []
    # the conditions on the inputs: each state in at least 20 cells under MASK, states 1 and 2 under BLEND
    assert all(seen[(blend.ALPHA_MASK, s)] >= 20 for s in (0, 1, 2)), seen
    assert seen[(blend.ALPHA_BLEND, 1)] >= 1 and seen[(blend.ALPHA_BLEND, 2)] >= 1, seen
    assert not (recs["omm"][~finite] != 0).any() and (~finite).sum() == 2


def test_the_edge_scene_takes_every_path_of_the_rule():
    t = materials.edge()
    ins = materials.triangle_inputs(t)
    maps = {k: materials.states(materials.opacity_map(t, m, uv)) for k, (m, uv, _) in enumerate(ins)}

    def cell_spans(k):
        m, uv, tex = ins[k]
        w, h = t.texture_size(tex)
        p = uv.reshape(3, 2).astype(np.float64) * [w, h]
        return (p.max(axis=0) - p.min(axis=0)) / 8.0

    by_material = {m: [k for k, x in enumerate(ins) if x[0] == m] for m in range(1, 8)}
    wide = [k for k in by_material[1] if cell_spans(k).max() >= 4096]
    assert wide and all((maps[k] == 0).all() for k in wide)                                           # span >= 4096
    big = [k for k in by_material[2] if np.isfinite(ins[k][1]).all() and cell_spans(k).max() < 4096 and np.prod(cell_spans(k) + 4) > 65536]
    assert big and all((maps[k] == 0).all() for k in big)                                             # footprint > 65536 texels
    assert sum(not np.isfinite(x[1]).all() for x in ins) == 2                                          # non-finite texcoords
    assert all(x[2] == -1 for x in ins if x[0] == 4) and all((maps[k] == 1).all() for k in by_material[4])      # no texture
    assert t.mats[5, blend.W_BASE_ALPHA].view(np.float32) < 0 and all((maps[k] == 0).all() for k in by_material[5])      # negative base alpha
    wraps = {(int(t.tex_rows["wrapS"][x[2]]), int(t.tex_rows["wrapT"][x[2]])) for x in ins if x[2] >= 0 and (x[1] < 0).any()}
    assert {w for pair in wraps for w in pair} == {materials.WRAP_REPEAT, materials.WRAP_CLAMP, materials.WRAP_MIRROR}      # negative texcoords under all three
    assert {int(t.tex_rows["magFilter"][x[2]]) for x in ins if x[2] >= 0} == {materials.FILTER_NEAREST, materials.FILTER_LINEAR}
    assert {t.texture_size(x[2]) for x in ins if x[2] >= 0} == {(1, 1), (37, 19), (64, 64)}
    # two materials share a base colour texture; one texture is used only as an emissive texture
    assert t.mats[1, blend.W_BASE_TEXTURE] == t.mats[6, blend.W_BASE_TEXTURE] == materials.T_SQUARE
    assert materials.T_EMISSIVE not in t.mats[:, blend.W_BASE_TEXTURE].view(np.int32) and materials.T_EMISSIVE in t.mats[:, materials.W_EMISSIVE_TEXTURE].view(np.int32)


def test_a_cutoff_edit_opens_and_closes_cells():
    """the same triangles under cutoffs 0.1 / 0.5 / 0.9: cells decided at one cutoff are unknown or decided the other way at another"""
    t = materials.edge()
    k = [x for x in materials.triangle_inputs(t) if x[0] == 1]
    counts = {}
    for cutoff in (0.1, 0.5, 0.9):
        t.mats[1, blend.W_ALPHA_CUTOFF] = materials.f2u(cutoff)
        s = np.stack([materials.states(materials.opacity_map(t, m, uv)) for m, uv, _ in k])
        counts[cutoff] = [int((s == v).sum()) for v in (0, 1, 2)]
    print(counts)
    assert counts[0.1][1] > counts[0.5][1] > counts[0.9][1] and counts[0.1][2] <= counts[0.5][2] < counts[0.9][2]


def test_rt_opacity_map_refuses_bad_arguments():
    from restir_amd.renderer import hip_lib
    L = hip_lib()
    d, out, tex = abi.OpacityMapDesc(), (C.c_uint32 * 4)(), np.zeros((1, 1, 4), np.uint8)
    assert L.rt_opacity_map(None, None, out) == -1 and L.rt_opacity_map(C.byref(d), None, None) == -1
    assert L.rt_opacity_map(C.byref(d), tex.ctypes.data, out) == -1      # a texture of 0 x 0 texels
    d.w = d.h = 1
    assert L.rt_opacity_map(C.byref(d), tex.ctypes.data, out) == 0


def test_the_generator_reaches_every_op_kind_and_every_refusal():
    for make in (materials.edge, lambda: materials.of_scene(refit.street())):
        kinds, whys = set(), set()
        for seed in materials.SEEDS:
            t = make()
            for op in materials.ops(t, seed):
                kinds.add(op["kind"])
                if op["kind"] == "refused":
                    whys.add(op["why"])
                materials.describe(op)
        assert kinds == set(materials.KINDS), set(materials.KINDS) - kinds
    assert whys == set(materials.REFUSALS), set(materials.REFUSALS) - whys      # (the street has emissive materials: both directions of the light rule)


def test_generated_ops_keep_the_tables_a_valid_description():
    t = materials.edge()
    for op in materials.ops(t, 2):
        materials.apply(t, op)
    d = t.desc()
    assert d.numInstances == len(t.inst) and d.numMaterials == len(t.mats) == 8
    tex = t.mats[:, blend.W_BASE_TEXTURE].view(np.int32)
    assert ((tex >= -1) & (tex < len(t.tex_rows))).all()


def test_the_host_scene_edits_its_own_tables():
    """Scene.setMaterials / Scene.setTexture: desc() afterwards describes the edited scene; a changed emission recomputes the light records' alias entries; a
    row that moves a material across the light rule, an id or a rectangle out of range are refused and change nothing"""
    import lights
    import pytest
    sc = refit.street()
    t = materials.of_scene(sc)
    lit = int(np.nonzero(materials._emissive(t))[0][0])
    plain = materials.alpha_materials(t)[0]
    before = lights.records_of(sc.desc()).copy()
    row = t.mats[plain].copy()
    row[materials.W_ROUGHNESS] = materials.f2u(0.125)
    sc.setMaterials([plain], row.reshape(1, 20))
    assert np.array_equal(blend.materials_of(sc.desc())[plain], row) and np.array_equal(lights.records_of(sc.desc()), before)
    lit_rows = np.nonzero(materials._emissive(t))[0]
    if len(lit_rows) > 1:      # one of several emitters twice as bright: the alias entries of the records change, their count does not
        row = t.mats[lit].copy()
        row[blend.W_EMISSIVE] = (row[blend.W_EMISSIVE].view(np.float32) * np.float32(2)).view(np.uint32)
        sc.setMaterials([lit], row.reshape(1, 20))
        after = lights.records_of(sc.desc())
        assert len(after) == len(before) and not np.array_equal(after["impSamp"], before["impSamp"])
    for ids, rows in (([len(t.mats)], t.mats[:1]), ([plain], None), ([lit], None)):
        if rows is None:      # across the light rule, either way
            rows = t.mats[ids[0]].copy().reshape(1, 20)
            rows[0, blend.W_EMISSIVE] = np.float32([0, 0, 0] if ids[0] == lit else [5, 5, 5]).view(np.uint32)
        was = blend.materials_of(sc.desc())
        with pytest.raises(ValueError):
            sc.setMaterials(ids, rows)
        assert np.array_equal(blend.materials_of(sc.desc()), was)
    tex = int(t.mats[plain, blend.W_BASE_TEXTURE].view(np.int32))
    w, h = t.texture_size(tex)
    texels = np.full((2, 3, 4), 9, np.uint8)
    sc.setTexture(tex, w - 3, h - 2, texels)
    now = materials.of_scene(sc).texels[tex]
    want = t.texels[tex].copy()
    want[h - 2:, w - 3:] = 9
    assert np.array_equal(now, want)
    with pytest.raises(ValueError):
        sc.setTexture(tex, w - 2, h - 2, texels)
    with pytest.raises(ValueError):
        sc.setTexture(len(t.tex_rows), 0, 0, texels)
    assert np.array_equal(materials.of_scene(sc).texels[tex], want)


def test_struct_sizes_and_the_enum_value():
    assert C.sizeof(abi.OpacityMapDesc) == 64 and C.sizeof(abi.MaterialStats) == 32 and abi.ALPHA_REC_DT.itemsize == 64 and abi.MATERIAL_DT.itemsize == 80
    assert abi.ACCEL_ALPHA == 3 and abi.ACCEL_RECORD_BYTES[abi.ACCEL_ALPHA] == 64
    header = open(os.path.join(ROOT, "include", "rt_abi.h")).read()
    assert "RT_ACCEL_ALPHA = 3" in header
    for name in ("rt_update_materials", "rt_update_texture", "rt_get_material_stats", "rt_opacity_map"):
        assert ("int %s(" % name) in header
    assert "sizeof(rt_opacity_map_desc) == 64 && sizeof(rt_material_stats) == 32" in header


def test_the_rule_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / "materials_san")
    flags = ["-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-fsanitize=address,undefined", "-fsanitize=float-cast-overflow",
             "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-Wall"]
    subprocess.check_call([os.environ.get("CXX", "g++")] + flags + [os.path.join(ROOT, "tests", "materials_san_main.cpp"), "-o", exe])
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "ok" in p.stdout
