"""Which build of the traced stages runs a launch, without a GPU: the builds compute the same bits, so a wrong choice costs only time and no image
test sees it.  The rule (csrc/stage_select.h, pure functions) is driven through tests/stage_select_driver.cpp, a stand-alone program built with AddressSanitizer and
UndefinedBehaviorSanitizer; the list of builds it names is held against the table that compiles them (STAGE_BUILDS in build.py) and the lists made from it."""
import itertools
import os
import re
import subprocess

import pytest

from helpers import ROOT, abi
from restir_amd import build

SRC = os.path.join(ROOT, "tests", "stage_select_driver.cpp")
INC = os.path.join(ROOT, "cis-565-final-vr-raytracer_amd", "csrc")
TRACED = (abi.STAGE_DIRECT, abi.STAGE_INDIRECT, abi.STAGE_DIRECT_GEN, abi.STAGE_DIRECT_REUSE)
FILTERS = (abi.STAGE_DENOISE_DIRECT, abi.STAGE_DENOISE_INDIRECT, abi.STAGE_COMPOSE)
NONE, OBJECT, VERTEX = 0, 1, 2        # StageMotion
NORMAL, RECORD, REPLAY = 0, 1, 2      # PrimaryReplayAction
ALONE, SHARED = (2000, 2000), (512, 640)   # rt_api.cpp's thresholds (direct, indirect at half resolution): a launch alone on the device / with frames in flight


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    d = tmp_path_factory.mktemp("stage_select")
    exe = str(d / "stage_select_driver")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-I", INC, SRC, "-o", exe])

    def run(script):
        """the driver's answers to the script's calls, one per call"""
        path = d / "script.txt"
        path.write_text("\n".join(script) + "\n")
        p = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=60)
        assert p.returncode == 0 and p.stderr == "", (p.returncode, p.stderr)
        out = p.stdout.split("\n")[:-1]
        assert len(out) == len(script)
        return out

    return run


def lat(stage, W, H, tiles=ALONE, counting=0, traversal=abi.TRAVERSAL_AUTO, rows=(0, 0)):
    return "lat %d %d %d %d %d %d %d %d %d" % (counting, traversal, stage, W, H, rows[0], rows[1], tiles[0], tiles[1])


def test_auto_mode_boundaries(driver):
    D, I = abi.STAGE_DIRECT, abi.STAGE_INDIRECT
    rows = [(D, ALONE, 400, 320, "latency"), (D, ALONE, 408, 320, "throughput"),        # 2000 / 2040 tiles
            (D, SHARED, 256, 128, "latency"), (D, SHARED, 264, 128, "throughput"),      # 512 / 528
            (I, ALONE, 800, 640, "latency"), (I, ALONE, 816, 640, "throughput"),        # half resolution: 2000 / 2040
            (I, SHARED, 512, 320, "latency"), (I, SHARED, 528, 320, "throughput")]      # 640 / 660
    assert driver([lat(s, W, H, t) for s, t, W, H, _ in rows]) == [r[4] for r in rows]


def test_odd_sizes_and_row_bands(driver):
    D, I = abi.STAGE_DIRECT, abi.STAGE_INDIRECT
    # 101x51: 13 x 7 = 91 tiles; its half resolution is 50x25: 7 x 4 = 28 tiles
    script = [lat(D, 101, 51, (91, 0)), lat(D, 101, 51, (90, 10**6)), lat(I, 101, 51, (0, 28)), lat(I, 101, 51, (10**6, 27))]
    want = ["latency", "throughput", "latency", "throughput"]
    # 1x1: one tile; the indirect stage's half resolution is empty, 0 tiles
    script += [lat(D, 1, 1, (1, 0)), lat(D, 1, 1, (0, 0)), lat(I, 1, 1, (0, 0))]
    want += ["latency", "throughput", "latency"]
    # row bands of a 408x320 image (51 tiles a row): rowEnd <= 0 and rowEnd > H mean the last row, rowBegin < 0 the first
    for rows, tiles in (((0, 0), 2040), ((0, -5), 2040), ((0, 321), 2040), ((-8, 320), 2040), ((-8, 400), 2040), ((8, 0), 1989), ((0, 312), 1989), ((8, 16), 51),
                        ((8, 17), 102), ((16, 8), 0), ((320, 0), 0)):
        script += [lat(D, 408, 320, (tiles, 0), rows=rows), lat(D, 408, 320, (max(tiles - 1, 0), 0), rows=rows)]
        want += ["latency", "latency" if tiles == 0 else "throughput"]     # (an empty band: 0 tiles, within every threshold; launchStage then launches nothing)
    # ... of the indirect stage, in half-resolution rows: 408x320 -> 204x160, 26 tiles a row
    for rows, tiles in (((0, 0), 520), ((0, 161), 520), ((-1, 160), 520), ((0, 152), 494), ((8, 16), 26)):
        script += [lat(I, 408, 320, (0, tiles), rows=rows), lat(I, 408, 320, (10**6, tiles - 1), rows=rows)]
        want += ["latency", "throughput"]
    assert driver(script) == want


def test_counting_traversal_mode_and_the_stages_without_a_latency_build(driver):
    D, I = abi.STAGE_DIRECT, abi.STAGE_INDIRECT
    script, want = [], []
    for stage in (D, I):
        for W, H in ((8, 8), (1920, 1080)):
            # counting forces throughput, whatever the mode; rt_set_traversal forces either build otherwise
            script += [lat(stage, W, H, counting=1, traversal=t) for t in (abi.TRAVERSAL_AUTO, abi.TRAVERSAL_THROUGHPUT, abi.TRAVERSAL_LATENCY)]
            want += ["throughput"] * 3
            script += [lat(stage, W, H, traversal=abi.TRAVERSAL_LATENCY), lat(stage, W, H, traversal=abi.TRAVERSAL_THROUGHPUT)]
            want += ["latency", "throughput"]
    for stage in FILTERS + (abi.STAGE_DIRECT_GEN, abi.STAGE_DIRECT_REUSE):
        script += [lat(stage, 8, 8, traversal=t) for t in (abi.TRAVERSAL_AUTO, abi.TRAVERSAL_LATENCY)]
        want += ["throughput"] * 2
    assert driver(script) == want


def forbidden(switches):
    """the #error guards of csrc/stages.hip"""
    s = set(switches)
    return ("RT_REPLAY" in s and s & {"RT_OM", "RT_VM", "RT_LAT"}) or (s & {"RT_OM", "RT_VM"} and "RT_COUNT" in s) or {"RT_OM", "RT_VM"} <= s or {"RT_LAT", "RT_COUNT"} <= s


def test_the_full_cross_of_the_traced_stages(driver):
    cross = list(itertools.product((0, 1), (0, 1), (0, 1), TRACED, (NONE, OBJECT, VERTEX), (NORMAL, RECORD, REPLAY)))
    out = driver(["build %d %d %d %d %d %d" % c for c in cross])
    assert set(out) == set(build.STAGE_BUILDS)   # every one of the eighteen is reached, and nothing else
    for (sky, counting, latency, stage, motion, action), name in zip(cross, out):
        sw = set(build.STAGE_BUILDS[name])
        why = (sky, counting, latency, stage, motion, action, name)
        assert not forbidden(sw), why
        assert ("RT_SKY" in sw) == bool(sky), why
        assert ("RT_COUNT" in sw) == bool(counting), why            # the counting builds are throughput builds: counting wins over latency
        two = stage in (abi.STAGE_DIRECT, abi.STAGE_INDIRECT)
        assert ("RT_LAT" in sw) == bool(latency and two and not counting), why
        replay = action != NORMAL and stage == abi.STAGE_DIRECT and "RT_LAT" not in sw
        assert ("RT_REPLAY" in sw) == replay, why                   # replay beats motion
        assert ("RT_OM" in sw) == (motion == OBJECT and two and not counting and not replay), why
        assert ("RT_VM" in sw) == (motion == VERTEX and two and not counting and not replay), why


def test_named_choices(driver):
    D, I, G = abi.STAGE_DIRECT, abi.STAGE_INDIRECT, abi.STAGE_DIRECT_GEN
    rows = [((0, 0, 0, D, NONE, NORMAL), "base"), ((1, 0, 0, I, NONE, NORMAL), "sky"), ((0, 1, 0, D, NONE, NORMAL), "base_cnt"), ((1, 1, 0, G, NONE, NORMAL), "sky_cnt"),
            ((0, 0, 1, D, NONE, NORMAL), "base_lat"), ((1, 0, 1, I, NONE, NORMAL), "sky_lat"), ((1, 0, 1, G, NONE, NORMAL), "sky"),
            ((0, 0, 0, D, OBJECT, NORMAL), "base_om"), ((1, 0, 1, I, OBJECT, NORMAL), "sky_lat_om"), ((0, 0, 1, D, VERTEX, NORMAL), "base_lat_vm"),
            ((1, 0, 0, I, VERTEX, NORMAL), "sky_vm"), ((0, 0, 0, G, OBJECT, NORMAL), "base"), ((0, 1, 0, D, OBJECT, NORMAL), "base_cnt"),
            ((0, 0, 0, D, NONE, RECORD), "base_rp"), ((1, 0, 0, D, NONE, REPLAY), "sky_rp"), ((0, 1, 0, D, NONE, REPLAY), "base_rp_cnt"), ((1, 1, 0, D, NONE, RECORD), "sky_rp_cnt"),
            ((0, 0, 0, D, OBJECT, REPLAY), "base_rp"), ((1, 0, 0, D, VERTEX, RECORD), "sky_rp"), ((0, 0, 0, I, NONE, REPLAY), "base")]
    assert driver(["build %d %d %d %d %d %d" % r[0] for r in rows]) == [r[1] for r in rows]
    # the filter chains and compose exist once, whatever else is asked
    cross = list(itertools.product((0, 1), (0, 1), (0, 1), FILTERS, (NONE, OBJECT, VERTEX), (NORMAL, RECORD, REPLAY)))
    assert set(driver(["build %d %d %d %d %d %d" % c for c in cross])) == {"filters"}


def test_the_lists_of_builds_agree(driver):
    sel = open(os.path.join(INC, "stage_select.h")).read()
    m = re.search(r"#define RT_STAGE_BUILDS\(X\)((?:.*\\\n)*.*)\n", sel)
    names = re.findall(r"X\((\w+)\)", m.group(1))
    assert len(names) == 18 and len(set(names)) == 18
    assert driver(["names"]) == [" ".join(names + ["filters"])]
    # the table that compiles them: the same set, and each name is what csrc/stages.hip pastes from the entry's switches
    assert set(build.STAGE_BUILDS) == set(names)
    for name, sw in build.STAGE_BUILDS.items():
        assert set(sw) <= {"RT_SKY", "RT_COUNT", "RT_LAT", "RT_OM", "RT_VM", "RT_REPLAY"} and not forbidden(sw), name
        form = [f for s, f in (("RT_OM", "_om"), ("RT_VM", "_vm"), ("RT_REPLAY", "_rp")) if s in sw]
        assert name == ("sky" if "RT_SKY" in sw else "base") + ("_lat" if "RT_LAT" in sw else "") + "".join(form) + ("_cnt" if "RT_COUNT" in sw else ""), name
    objs = [stem for src, stem, _ in build.hip_units() if src == "stages.hip"]
    assert len(set(objs)) == 18 and "stages" in objs and "stages_lat" in objs and "stages_sky_rp_cnt" in objs and not any("base" in o for o in objs)
    # the declarations and the table of launchers are made from the list, and nothing declares a launcher beside it
    hdr = open(os.path.join(INC, "stages.h")).read()
    assert re.findall(r"^RT_DECL_LAUNCH\w*\(\w+\)|^RT_STAGE_BUILDS\(\w+\)", hdr, re.M) == ["RT_STAGE_BUILDS(RT_DECL_LAUNCH)"]
    assert len(re.findall(r"\blaunchStage\(", hdr)) == 1
    api = open(os.path.join(INC, "rt_api.cpp")).read()
    assert re.search(r"g_stageLaunchers\[rt::STAGE_BUILD_COUNT\] = \{[^;]*RT_STAGE_BUILDS\(RT_STAGE_LAUNCHER\)[^;]*filterLauncher\};", api)
    assert not re.search(r"rt::(base|sky)\w*::launchStage", api)
    assert not [f for f in os.listdir(INC) if re.fullmatch(r"stages_\w+\.hip|reference_sky\.hip", f)]   # no stub files: the table is the one statement
