"""One side of a same-box A/B of the filter stages (A-Trous chains, compose): the benchmark frame with frames in flight and serial, and the three stages as row
bands through rt_run_stage.  The library under test is the tree's or the one RESTIR_HIP_LIB names; the caller alternates processes of the two.

    [RESTIR_HIP_LIB=.../csrc/_ab/lib_old.so] python scripts/filters_ab.py LABEL [WINDOWS]

Prints one JSON line per (configuration, window): wall ms per frame (host clock around FRAMES frames that end in rt_sync), the per-stage event times of
rt_get_counters, and for the band case the host-clock time of each stage's whole chain over all bands; and a digest of the last frame's images."""
import hashlib, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
from helpers import abi, host, make_scene
from restir_amd.renderer import Renderer, HIP_LIB_PATH

LABEL = sys.argv[1] if len(sys.argv) > 1 else "tree"
WINDOWS = int(sys.argv[2]) if len(sys.argv) > 2 else 3
W, H, WARM, FRAMES = 1920, 1080, 16, 200
STAGES = ["direct", "indirect", "denoise_direct", "denoise_indirect", "compose"]
BANDS = [(0, 256), (256, 368), (368, 496), (496, 528), (528, 576), (576, 656), (656, 800), (800, 1080)]   # the cost-weighted bands of an 8-GPU frame (scripts/band_ab.py)
FILTERS = [("denoise_direct", abi.STAGE_DENOISE_DIRECT, 4, 1), ("denoise_indirect", abi.STAGE_DENOISE_INDIRECT, 5, 2), ("compose", abi.STAGE_COMPOSE, 1, 1)]

lib_hash = hashlib.sha256(open(HIP_LIB_PATH, "rb").read()).hexdigest()[:16]
sc, env = make_scene(abi.PROC_BISTRO_EXT, 1.0, 1, (2048, 1024))
desc = sc.desc(env)


def out(**kw):
    print(json.dumps(dict(label=LABEL, lib=lib_hash, **kw)), flush=True)


for overlap in (2, 0):
    st = host.default_state(W, H, sc, env); st.maxDepth = 4
    r = Renderer().setup(0); r.set_overlap(overlap); r.load_scene(desc); r.update(W, H)
    sc.updateCamera(W, H)
    f = 0

    def frame():
        global f
        st.time = 1000 + f; sc.updateCamera(W, H); r.set_camera(sc.getCamera()); r.run(st, f); f += 1

    for _ in range(WARM): frame()
    for w in range(WINDOWS):
        r.set_counting(False)    # (synchronises and zeroes the stage timers)
        t0 = time.perf_counter()
        for _ in range(FRAMES): frame()
        r.sync(); wall = (time.perf_counter() - t0) / FRAMES * 1e3
        c = r.counters()
        out(case="overlap%d" % overlap, window=w, wall_ms=round(wall, 4), stage_ms={STAGES[i]: round(c.stageMs[i] / max(1, c.framesTimed), 4) for i in range(5)})
    if overlap == 0:
        cur = (f - 1) & 1
        out(case="digest", images=hashlib.sha256(r.readback(abi.BUF_DIRECT_RESULT0 + cur).tobytes() + r.readback(abi.BUF_INDIRECT_RESULT0 + cur).tobytes()).hexdigest()[:16])
        # the row-band case: every level of a chain band after band, as the hosts of a row-tiled frame launch them (rows of the stage's own grid)
        for w in range(WINDOWS):
            ms = {}
            for name, stage, levels, div in FILTERS:
                def chain():
                    for level in range(levels):
                        for y0, y1 in BANDS: r.run_stage(st, f - 1, stage, level, y0 // div, y1 // div)
                chain(); r.sync(); t0 = time.perf_counter()
                for _ in range(100): chain()
                r.sync(); ms[name] = round((time.perf_counter() - t0) / 100 * 1e3, 4)
            out(case="bands", window=w, stage_ms=ms)
    r.destroy()
