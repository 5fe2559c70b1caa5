"""How far the shipped real-time frame is from the image it estimates: K real-time frames at a fixed camera (modulate = 1) averaged, against the
reference mode (rt_reference_render) at S samples per pixel, per component (direct, indirect, sum).

Per configuration (bench.py's CONFIGS: 2 Cornell 512^2, 3 Sponza-class 1080p maxDepth 2, 4 bistro-exterior-class 1080p, lite footprint) and per variant
of the real-time state (default; denoise off; temporal reuse off = ReSTIRState RIS) it prints one JSON line with, per component and over all pixels and over
the pixels whose primary ray hits a surface (G-buffer depth < infinity):
  lum_ratio    mean luminance of the frame average / mean luminance of the reference
  median_px_ratio  median over pixels of (frame luminance / reference luminance) — not dominated by the few brightest pixels
  rel_rmse     RMS of (frame average - reference) over pixels and channels / mean of the reference over pixels and channels
  out_3sigma   share of pixels whose luminance difference exceeds 3 sigma of the reference's own mean (sigma from B batch means of the reference)
  flicker      frame-to-frame noise: the mean over pixels of the per-pixel standard deviation of the luminance over the K frames (fixed camera) / the mean
               luminance of the reference
--denoiser selects the filter of the real-time frames (rt_set_denoiser), one JSON line per entry: `atrous` (the default), `svgf` (library defaults) or
`svgf:key=value:...` with rt_denoiser fields (alphaColor, alphaMoments, historyCap, phiLumDirect, phiLumIndirect) — the reference is taken once per configuration.
--taa selects temporal anti-aliasing (rt_set_taa), one JSON line per entry: `off` (the default), `on` (library defaults) or `on:key=value:...` with rt_taa fields
(jitterPhases, alpha, clipGamma); with TAA on the frame average is taken over the resolved images (rt_taa_readback).  --ref-supersample S renders the reference
at S·W × S·H in a context of its own and averages S×S blocks: the box-filtered pixel a jittered TAA frame estimates (the plain reference is point-sampled at
pixel centres).  Every line also reports the metrics over the edge pixels: pixels whose 3×3 G-buffer neighbourhood (an unjittered frame) holds another
material hash or a relative depth step above 10 %.
--upscale selects temporal upsampling (rt_set_upscale), one JSON line per entry: `off` (the default: native rendering at the configuration's size), `R` or
`R:key=value:...` (render at round(W / R) x round(H / R), resolve to W x H; rt_upscale fields jitterPhases, alpha, clipGamma) or `bilinear:R` (the same
low-resolution frames without jitter, each upsampled bilinearly to W x H: what a host without the pass would show).  The reference, the surface and the edge
pixels are taken at the OUTPUT size W x H (use --ref-supersample: a resolved pixel estimates the box-filtered one).
The reference ignores the real-time state (its sums are taken once per configuration); every frame of the average uses the same camera (its history matrices
advanced per frame, as SampleExample::updateFrame does), time = 1000 + f.
Config 2 runs the whole frame here (bench.py times the direct stage alone for it).

  python scripts/reference_bias.py [--configs 2 3 4] [--frames 64] [--warmup 8] [--spp 256] [--batches 8] [--out profiles/reference_bias.jsonl]
  python scripts/reference_bias.py --denoiser atrous svgf --variants default [--out profiles/denoiser_svgf.jsonl]      # the denoiser A/B
  python scripts/reference_bias.py --gi-spatial off on vis --denoiser atrous svgf --variants default [--out profiles/gi_spatial.jsonl]
  python scripts/reference_bias.py --taa off on on:jitterPhases=0 --denoiser atrous svgf --variants default --ref-supersample 4 [--out profiles/taa.jsonl]   # §16
  python scripts/reference_bias.py --upscale off 1.5 bilinear:1.5 --variants default --ref-supersample 2 [--out profiles/upscale.jsonl]   # §29
  python scripts/reference_bias.py --timing [--configs 4 2] [--spp 16]      # reference time per sample at the configuration's size (host-timed, synchronised)
  python scripts/reference_bias.py --rays-per-path [--configs 4 2]         # CPU only: ray queries per path of the CPU restatement (tests/refpt_checker.cpp)
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import restir_amd  # noqa: E402,F401
from restir_amd import abi, host  # noqa: E402

# (kind, size, env, state overrides) of bench.py's CONFIGS, lite footprint
CONFIGS = {
    2: ("PROC_CORNELL", (512, 512), None, {"environmentProb": 0.0, "fireflyClampThreshold": 100.0}),
    3: ("PROC_SPONZA", (1920, 1080), (2048, 1024), {"maxDepth": 2}),
    4: ("PROC_BISTRO_EXT", (1920, 1080), (2048, 1024), {}),
}
VARIANTS = {"default": {}, "denoise_off": {"denoise": 0}, "temporal_off": {"ReSTIRState": abi.RESTIR_RIS}}
LUM = np.array([0.2126, 0.7152, 0.0722])


def setup(config, width=0, height=0):
    kind, size, env_size, over = CONFIGS[config]
    W, H = width or size[0], height or size[1]
    sc = host.Scene().makeProcedural(getattr(abi, kind), 1.0, 1)
    env = None
    if env_size:
        env = host.HdrSampling()
        env.makeSyntheticSky(env_size[0], env_size[1], 5e4, 7)
    st = host.default_state(W, H, sc, env)
    for k, v in over.items():
        setattr(st, k, v)
    st.modulate = 1
    sc.updateCamera(W, H)
    return sc, env, st, W, H


def reference(r, st, spp, batches):
    """mean of each component after spp samples, and the standard error of the luminance of the sum's mean (from `batches` batch means)"""
    r.reference_reset()
    per = spp // batches
    prev = np.zeros((st.size.y, st.size.x, 3))
    bmeans = []
    t0 = time.time()
    for b in range(batches):
        r.reference_render(st, per)
        cur = r.reference_readback(abi.REF_SUM)[..., :3].astype(np.float64)
        n = r.reference_samples()
        bmeans.append((cur * n - prev * (n - per)) / per)     # the batch's own mean
        prev = cur
    secs = time.time() - t0
    lum_b = np.stack([m @ LUM for m in bmeans])
    sigma = lum_b.std(axis=0, ddof=1) / np.sqrt(batches)
    return [r.reference_readback(c)[..., :3].astype(np.float64) for c in range(3)], sigma, secs


def denoiser_settings(spec):
    """`atrous` | `svgf` | `svgf:key=value:...` -> (label, abi.Denoiser)"""
    parts = spec.split(":")
    if parts[0] not in ("atrous", "svgf"):
        raise SystemExit(f"--denoiser {spec}: atrous or svgf[:key=value...]")
    kw = {}
    for p in parts[1:]:
        k, v = p.split("=")
        kw[k] = int(v) if k == "historyCap" else float(v)
    return spec, abi.Denoiser(mode=abi.DENOISER_SVGF if parts[0] == "svgf" else abi.DENOISER_ATROUS, **kw)


def gi_spatial_settings(spec):
    """`off` | `on` | `vis` | `on:key=value:...` with rt_gi_spatial fields (samples, radius, normalThreshold, depthThreshold, jacobianMax) -> (label, abi.GiSpatial)"""
    parts = spec.split(":")
    modes = {"off": abi.GI_SPATIAL_OFF, "on": abi.GI_SPATIAL_ON, "vis": abi.GI_SPATIAL_VISIBILITY}
    if parts[0] not in modes:
        raise SystemExit(f"--gi-spatial {spec}: off, on or vis[:key=value...]")
    kw = {}
    for p in parts[1:]:
        k, v = p.split("=")
        kw[k] = int(v) if k in ("samples", "radius") else float(v)
    return spec, abi.GiSpatial(mode=modes[parts[0]], **kw)


def taa_settings(spec):
    """`off` | `on` | `on:key=value:...` with rt_taa fields (jitterPhases, alpha, clipGamma) -> (label, abi.Taa)"""
    parts = spec.split(":")
    if parts[0] not in ("off", "on"):
        raise SystemExit(f"--taa {spec}: off or on[:key=value...]")
    kw = {}
    for p in parts[1:]:
        k, v = p.split("=")
        kw[k] = int(v) if k == "jitterPhases" else float(v)
    return spec, abi.Taa(mode=abi.TAA_ON if parts[0] == "on" else abi.TAA_OFF, **kw)


def upscale_settings(spec, W, H):
    """`off` | `R[:key=value...]` | `bilinear:R` -> (label, kind, (w, h) render size, abi.Upscale) for the output size W x H"""
    parts = spec.split(":")
    if parts[0] == "off":
        return spec, "off", (W, H), abi.Upscale()
    try:
        if parts[0] == "bilinear":
            R, kind, rest = float(parts[1]), "bilinear", []
        else:
            R, kind, rest = float(parts[0]), "temporal", parts[1:]
    except (ValueError, IndexError):
        raise SystemExit(f"--upscale {spec}: off, R[:key=value...] or bilinear:R with 1 <= R <= 4")
    kw = {}
    for p in rest:
        k, v = p.split("=")
        kw[k] = int(v) if k == "jitterPhases" else float(v)
    w, h = max(1, int(round(W / R))), max(1, int(round(H / R)))
    if not (w <= W <= 4 * w and h <= H <= 4 * h):
        raise SystemExit(f"--upscale {spec}: the ratio must lie in 1..4")
    return spec, kind, (w, h), (abi.Upscale(mode=abi.UPSCALE_TEMPORAL, outWidth=W, outHeight=H, **kw) if kind == "temporal" else abi.Upscale())


def bilinear_upsample(img, W, H):
    """(h, w, C) -> (H, W, C), pixel centres aligned, edge texels repeated"""
    h, w = img.shape[:2]
    x = np.clip((np.arange(W) + 0.5) * w / W - 0.5, 0, w - 1); y = np.clip((np.arange(H) + 0.5) * h / H - 0.5, 0, h - 1)
    x0, y0 = np.floor(x).astype(int), np.floor(y).astype(int)
    x1, y1 = np.minimum(x0 + 1, w - 1), np.minimum(y0 + 1, h - 1)
    fx, fy = (x - x0)[None, :, None], (y - y0)[:, None, None]
    top = img[y0][:, x0] * (1 - fx) + img[y0][:, x1] * fx
    bot = img[y1][:, x0] * (1 - fx) + img[y1][:, x1] * fx
    return top * (1 - fy) + bot * fy


def edge_pixels(g):
    """pixels whose 3x3 neighbourhood in the G-buffer g (H, W, 4 u32) has another material hash or a relative depth step above 10 %"""
    H, W = g.shape[:2]
    mat = g[..., 3] & np.uint32(0xFF000000)
    depth = g[..., 0].view(np.float32).astype(np.float64)
    edge = np.zeros((H, W), bool)
    for j in (-1, 0, 1):
        for i in (-1, 0, 1):
            yy, xx = np.clip(np.arange(H) + j, 0, H - 1), np.clip(np.arange(W) + i, 0, W - 1)
            mq, dq = mat[yy][:, xx], depth[yy][:, xx]
            with np.errstate(invalid="ignore", over="ignore"):
                step = np.abs(dq - depth) > 0.1 * np.minimum(dq, depth)
            edge |= (mq != mat) | step
    return edge


def supersampled_reference(desc, config, W, H, S, spp, batches):
    """the reference at S*W x S*H in a context of its own, averaged over S x S blocks (the box-filtered pixel); sigma of the sum's luminance likewise"""
    from restir_amd.renderer import Renderer
    sc, env, st, _, _ = setup(config, W * S, H * S)
    r = Renderer().setup(0)
    r.load_scene(desc)
    r.update(W * S, H * S)
    r.set_camera(sc.getCamera())
    ref, sigma, secs = reference(r, st, spp, batches)
    r.destroy()
    box = lambda a: a.reshape(H, S, W, S, *a.shape[2:]).mean(axis=(1, 3))  # noqa: E731
    return [box(c) for c in ref], np.sqrt(box(sigma ** 2) / (S * S)), secs


def realtime_average(r, sc, st, frames, warmup, taa_on=False, upscale=None):
    """the mean of each component over the frames after warm-up, the per-pixel standard deviation of each component's luminance over those frames,
    and the pixels that hit a surface.  upscale = (kind, W, H): the frames are rendered at st.size and the images taken at W x H, from the resolved frame
    (`temporal`, rt_upscale_readback) or bilinearly upsampled (`bilinear`)"""
    acc = [None, None, None]
    lsum = [0.0, 0.0, 0.0]
    lsq = [0.0, 0.0, 0.0]
    for f in range(warmup + frames):
        st.time = 1000 + f
        st.frame = f
        sc.updateCamera(st.size.x, st.size.y)                   # static camera; advances the history matrices like SampleExample does (temporal reuse needs them)
        r.set_camera(sc.getCamera())
        r.run(st, f)
        if f >= warmup:
            cur = f & 1
            if upscale is not None and upscale[0] == "temporal":
                imgs = [r.upscale_readback(w)[..., :3].astype(np.float64) for w in (abi.UPSCALE_DIRECT, abi.UPSCALE_INDIRECT)]
            elif taa_on:
                imgs = [r.taa_readback(w)[..., :3].astype(np.float64) for w in (abi.TAA_DIRECT, abi.TAA_INDIRECT)]
            else:
                imgs = [r.readback(buf).view(np.float32).reshape(st.size.y, st.size.x, 4)[..., :3].astype(np.float64)
                        for buf in (abi.BUF_DIRECT_RESULT0 + cur, abi.BUF_INDIRECT_RESULT0 + cur)]
            if upscale is not None and upscale[0] == "bilinear":
                imgs = [bilinear_upsample(img, upscale[1], upscale[2]) for img in imgs]
            imgs.append(imgs[0] + imgs[1])
            for k, img in enumerate(imgs):
                acc[k] = img if acc[k] is None else acc[k] + img
                lum = img @ LUM
                lsum[k] = lsum[k] + lum
                lsq[k] = lsq[k] + lum * lum
    last = (warmup + frames - 1) & 1
    g = r.readback(abi.BUF_GBUFFER0 + last).view(np.uint32).reshape(st.size.y, st.size.x, 4)
    surface = g[..., 0].view(np.float32) < 1e28 * 0.8
    d, i = acc[0] / frames, acc[1] / frames
    std = [np.sqrt(np.maximum(lsq[k] / frames - (lsum[k] / frames) ** 2, 0.0)) for k in range(3)]
    return [d, i, d + i], std, surface


def metrics(frame, ref, sigma, mask, std=None):
    f, g = frame[mask], ref[mask]
    lf, lg = f @ LUM, g @ LUM
    pos = lg > 0
    extra = {} if std is None else {"flicker": round(float(std[mask].mean() / lg.mean()), 4) if lg.mean() > 0 else None}
    return {**extra, "lum_ratio": round(float(lf.mean() / lg.mean()), 4) if lg.mean() > 0 else None,
            "median_px_ratio": round(float(np.median(lf[pos] / lg[pos])), 4) if pos.any() else None,
            "rel_rmse": round(float(np.sqrt(((f - g) ** 2).mean()) / g.mean()), 4) if g.mean() > 0 else None,
            "out_3sigma": round(float((np.abs(lf - lg) > 3 * sigma[mask]).mean()), 4) if sigma is not None else None}


def bias(args):
    from restir_amd.renderer import Renderer
    for config in args.configs:
        sc, env, st0, W, H = setup(config, args.width, args.height)
        desc = sc.desc(env)
        r = Renderer().setup(0)
        r.load_scene(desc)
        r.update(W, H)
        r.set_camera(sc.getCamera())
        if args.ref_supersample > 1:
            ref, sigma, secs = supersampled_reference(desc, config, W, H, args.ref_supersample, args.spp, args.batches)
            sc.updateCamera(W, H)
        else:
            ref, sigma, secs = reference(r, st0, args.spp, args.batches)
        # the edge pixels, from one unjittered frame
        r.set_camera(sc.getCamera())
        r.run(st0, 0)
        g_native = r.readback(abi.BUF_GBUFFER0).view(np.uint32).reshape(H, W, 4)
        edge = edge_pixels(g_native)
        surface_native = g_native[..., 0].view(np.float32) < 1e28 * 0.8
        runs = [(v, d, g, t, u) for v in VARIANTS.items() if v[0] in args.variants for d in map(denoiser_settings, args.denoiser)
                for g in map(gi_spatial_settings, args.gi_spatial) for t in map(taa_settings, args.taa) for u in (upscale_settings(x, W, H) for x in args.upscale)]
        edges = args.taa != ["off"] or args.upscale != ["off"]
        for (vname, over), (dname, den), (gname, gis), (tname, taa), (uname, ukind, (w, h), ups) in runs:
            st = abi.RtxState.from_buffer_copy(st0)
            for k, v in over.items():
                setattr(st, k, v)
            st.size.x, st.size.y = w, h
            if args.upscale != ["off"]:
                r.set_upscale(abi.Upscale())                    # (the ratio limits are checked against the size in force)
            r.update(w, h)                                      # fresh history for every variant
            r.set_denoiser(den)
            r.set_gi_spatial(gis)
            r.set_taa(taa)
            if ukind == "temporal":
                r.set_upscale(ups)
            sc.updateCamera(w, h)
            r.set_camera(sc.getCamera())
            frame, std, surface = realtime_average(r, sc, st, args.frames, args.warmup, taa.mode == abi.TAA_ON, None if ukind == "off" else (ukind, W, H))
            if ukind != "off":
                surface = surface_native
            out = {"config": config, "variant": vname, "denoiser": dname, **({"gi_spatial": gname} if args.gi_spatial != ["off"] else {}),
                   **({"taa": tname} if args.taa != ["off"] else {}), **({"upscale": uname, "render_size": [w, h]} if args.upscale != ["off"] else {}),
                   **({"ref_supersample": args.ref_supersample, "edge_share": round(float(edge.mean()), 4)} if edges else {}),
                   "size": [W, H], "frames": args.frames, "warmup": args.warmup, "ref_spp": args.spp,
                   "ref_batches": args.batches, "ref_seconds": round(secs, 2), "surface_share": round(float(surface.mean()), 4)}
            everything = np.ones_like(surface)
            for name, c in (("direct", 0), ("indirect", 1), ("sum", 2)):
                out[name] = {"all": metrics(frame[c], ref[c], sigma if c == 2 else None, everything, std[c]),
                             "surface": metrics(frame[c], ref[c], sigma if c == 2 else None, surface, std[c])}
                if edges:
                    out[name]["edge"] = metrics(frame[c], ref[c], sigma if c == 2 else None, edge, std[c])
            line = json.dumps(out)
            print(line, flush=True)
            if args.out:
                with open(args.out, "a") as fh:
                    fh.write(line + "\n")
        r.destroy()


def timing(args):
    from restir_amd.renderer import Renderer
    for config in args.configs:
        sc, env, st, W, H = setup(config, args.width, args.height)
        r = Renderer().setup(0)
        r.load_scene(sc.desc(env))
        r.update(W, H)
        r.set_camera(sc.getCamera())
        r.reference_render(st, 1)
        r.reference_readback(abi.REF_SUM)                        # warm: first launch, allocation
        r.reference_reset()
        t0 = time.time()
        r.reference_render(st, args.spp)
        r.reference_readback(abi.REF_SUM)
        dt = (time.time() - t0) / args.spp
        print(json.dumps({"config": config, "size": [W, H], "maxDepth": st.maxDepth, "spp": args.spp, "ms_per_sample": round(dt * 1e3, 3),
                          "paths_per_s": round(W * H / dt / 1e6, 2), "unit": "Mpaths/s (host-timed, includes one readback)"}), flush=True)
        r.destroy()


def rays_per_path(args):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import tempfile
    import refpt
    lib = refpt.build(tempfile.mkdtemp(prefix="refpt"))
    for config in args.configs:
        sc, env, st, W, H = setup(config, args.width, args.height)
        w, h = max(8, W // 8), max(8, H // 8)
        s = abi.RtxState.from_buffer_copy(st); s.size.x, s.size.y = w, h
        sc.updateCamera(w, h)
        desc = sc.desc(env)
        k = refpt.RefChecker(lib, desc)
        k.resize(w, h)
        k.set_camera(sc.getCamera())
        k.render(s, args.spp, threads=os.cpu_count() and min(16, os.cpu_count()))
        print(json.dumps({"config": config, "size": [w, h], "spp": args.spp, "maxDepth": s.maxDepth,
                          "rays_per_path": round(k.rays() / (w * h * args.spp), 3), "source": "CPU restatement (tests/refpt_checker.cpp), same camera at 1/8 size"}), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--configs", type=int, nargs="+", default=[2, 3, 4], choices=sorted(CONFIGS))
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--spp", type=int, default=256)
    ap.add_argument("--batches", type=int, default=8)
    ap.add_argument("--width", type=int, default=0)
    ap.add_argument("--height", type=int, default=0)
    ap.add_argument("--out", default="")
    ap.add_argument("--denoiser", nargs="+", default=["atrous"], help="atrous | svgf | svgf:key=value:... (one run of the real-time frames per entry)")
    ap.add_argument("--gi-spatial", nargs="+", default=["off"], help="off | on | vis | on:key=value:... (ReSTIR GI spatial reuse; one run per entry)")
    ap.add_argument("--taa", nargs="+", default=["off"], help="off | on | on:key=value:... (temporal anti-aliasing; one run per entry)")
    ap.add_argument("--upscale", nargs="+", default=["off"], help="off | R[:key=value:...] | bilinear:R (temporal upsampling from 1/R of the size; one run per entry)")
    ap.add_argument("--ref-supersample", type=int, default=1, help="S: the reference at S*W x S*H, averaged over S x S blocks")
    ap.add_argument("--variants", nargs="+", default=list(VARIANTS), choices=list(VARIANTS))
    ap.add_argument("--timing", action="store_true")
    ap.add_argument("--rays-per-path", action="store_true")
    args = ap.parse_args()
    if args.rays_per_path:
        rays_per_path(args)
    elif args.timing:
        timing(args)
    else:
        assert args.spp % args.batches == 0 and args.batches >= 2
        bias(args)


if __name__ == "__main__":
    main()
