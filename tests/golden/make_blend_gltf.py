#!/usr/bin/env python3
"""Generates tests/golden/blend_panes.gltf: a hand-written glTF 2.0 scene whose panes say "alphaMode": "BLEND" (tests/blend.py reads it through Scene.load), written
with nothing but json / struct / zlib like make_mini_gltf.py.  Seen from the camera at z = 7, front to back:

  * `veil`     one large untextured pane, baseColorFactor[3] = 0.25, in front of everything: every primary ray has a stochastic candidate
  * `coplanarA`, `coplanarB`  two overlapping panes in the same plane (equal t: the lower globalId wins), alpha 0.5 and 0.6
  * `zero`     alpha factor exactly 0 (the micro-map's state 2 in every cell: never accepted, and not force-opaque)
  * `nearest`  a 4 x 4 alpha checker through a nearest sampler, wrapS clamp / wrapT mirror, texcoords from -0.75 to 2.25
  * `gradient` a 16 x 8 alpha ramp (eight columns of exact 0, then up to exact 255) through a linear sampler, repeat
  * an opaque wall behind them, and an opaque emissive panel above the camera's side of the veil (so that shadow rays cross the panes as well)

Usage: python tests/golden/make_blend_gltf.py   (rewrites the file next to it)"""
import json, os, sys
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_mini_gltf import png, uri  # noqa: E402


def quad_xy(x0, x1, y0, y1):
    """in the plane z = 0, normal +z"""
    return np.array([[x0, y0, 0], [x1, y0, 0], [x1, y1, 0], [x0, y1, 0]], np.float32)


def main():
    blob, views, accessors = bytearray(), [], []

    def add(b):
        while len(blob) % 4:
            blob.append(0)
        views.append({"buffer": 0, "byteOffset": len(blob), "byteLength": len(b)})
        blob.extend(b)
        return len(views) - 1

    def accessor(a, kind):
        a = np.ascontiguousarray(a)
        acc = {"bufferView": add(a.tobytes()), "componentType": 5126 if a.dtype == np.float32 else 5123, "count": len(a), "type": kind}
        if kind == "VEC3":
            acc["min"], acc["max"] = [float(v) for v in a.min(0)], [float(v) for v in a.max(0)]
        accessors.append(acc)
        return len(accessors) - 1

    idx = accessor(np.array([0, 1, 2, 0, 2, 3], np.uint16), "SCALAR")
    meshes, nodes = [], []

    def pane(name, pos, material, at, uv=None):
        attrs = {"POSITION": accessor(pos, "VEC3")}
        if uv is not None:
            attrs["TEXCOORD_0"] = accessor(np.array(uv, np.float32), "VEC2")
        meshes.append({"name": name, "primitives": [{"attributes": attrs, "indices": idx, "material": material}]})
        nodes.append({"name": name, "mesh": len(meshes) - 1, "translation": [float(v) for v in at]})

    unit = [[0, 0], [1, 0], [1, 1], [0, 1]]
    wide = [[-0.75, -0.75], [2.25, -0.75], [2.25, 2.25], [-0.75, 2.25]]
    # instance order = globalId order: the wall first, coplanarA before coplanarB
    pane("wall", quad_xy(-5, 5, -3.5, 3.5), 0, (0, 0, -1))
    pane("gradient", quad_xy(-0.8, 0.8, -0.6, 0.6), 1, (-1.8, 0.7, 0.0), unit)
    pane("nearest", quad_xy(-0.8, 0.8, -0.6, 0.6), 2, (0.0, 0.7, 0.3), wide)
    pane("zero", quad_xy(-0.8, 0.8, -0.6, 0.6), 4, (1.8, 0.7, 0.6))
    pane("coplanarA", quad_xy(-0.8, 0.8, -0.6, 0.6), 5, (-0.4, -0.7, 1.2))
    pane("coplanarB", quad_xy(-0.8, 0.8, -0.6, 0.6), 6, (0.5, -0.6, 1.2))
    pane("veil", quad_xy(-3, 3, -2, 2), 3, (0, 0, 2))
    pane("lamp", np.array([[-1, 0, 0], [1, 0, 0], [1, 0, 2], [-1, 0, 2]], np.float32), 7, (0, 2.6, 2.5))     # normal -y
    nodes.append({"name": "camNode", "translation": [0.0, 0.0, 7.0], "camera": 0})

    # ---- images: RGBA8, white with the alpha under test
    ramp = np.array([0] * 8 + [30, 70, 110, 150, 190, 230, 255, 255], np.uint8)     # eight columns of exact 0: whole micro-map cells of state 2 beside mixed ones
    grad = np.full((8, 16, 4), 255, np.uint8)
    grad[..., 3] = ramp[None, :]
    grad[5:, 8:, 3] = ramp[:7:-1][None, :] // 2        # the lower rows of the right half: another ramp, so that the bilinear weights matter in y as well
    chk = np.full((4, 4, 4), 255, np.uint8)
    chk[..., 3] = np.array([[0, 255, 64, 192], [255, 0, 192, 64], [128, 32, 0, 255], [16, 240, 255, 0]], np.uint8)
    images = [png(16, 8, 6, grad.reshape(8, 64), [0, 1, 2]), png(4, 4, 6, chk.reshape(4, 16), [4, 3])]

    def blend(name, rgba, texture=None):
        pbr = {"baseColorFactor": rgba, "metallicFactor": 0.0, "roughnessFactor": 0.8}
        if texture is not None:
            pbr["baseColorTexture"] = {"index": texture}
        return {"name": name, "pbrMetallicRoughness": pbr, "alphaMode": "BLEND", "doubleSided": True}

    gltf = {
        "asset": {"version": "2.0", "generator": "tests/golden/make_blend_gltf.py"},
        "scene": 0,
        "scenes": [{"nodes": list(range(len(nodes)))}],
        "nodes": nodes,
        "cameras": [{"type": "perspective", "perspective": {"yfov": 0.7, "znear": 0.1}}],
        "meshes": meshes,
        "materials": [
            {"name": "wall", "pbrMetallicRoughness": {"baseColorFactor": [0.7, 0.7, 0.65, 1.0], "metallicFactor": 0.0, "roughnessFactor": 0.9}},
            blend("gradient", [0.9, 0.3, 0.2, 1.0], 0),
            blend("nearest", [0.2, 0.8, 0.3, 0.75], 1),
            blend("veil", [0.3, 0.4, 0.9, 0.25]),
            blend("zero", [1.0, 1.0, 0.0, 0.0]),
            blend("coplanarA", [0.9, 0.1, 0.8, 0.5]),
            blend("coplanarB", [0.1, 0.9, 0.8, 0.6]),
            {"name": "lamp", "pbrMetallicRoughness": {"baseColorFactor": [1.0, 1.0, 1.0, 1.0]}, "emissiveFactor": [1.0, 0.95, 0.9],
             "extensions": {"KHR_materials_emissive_strength": {"emissiveStrength": 12.0}}},
        ],
        "samplers": [{"magFilter": 9729, "minFilter": 9729, "wrapS": 10497, "wrapT": 10497}, {"magFilter": 9728, "minFilter": 9728, "wrapS": 33071, "wrapT": 33648}],
        "textures": [{"source": 0, "sampler": 0}, {"source": 1, "sampler": 1}],
        "images": [{"uri": uri(im, "image/png")} for im in images],
        "extensionsUsed": ["KHR_materials_emissive_strength"],
        "bufferViews": views,
        "accessors": accessors,
    }
    gltf["buffers"] = [{"byteLength": len(blob), "uri": uri(bytes(blob))}]
    with open(os.path.join(HERE, "blend_panes.gltf"), "w") as f:
        json.dump(gltf, f, indent=1)


if __name__ == "__main__":
    main()
