"""Settled primary visibility without a GPU: the rule that says when a direct launch may record or replay (csrc/primary_replay.h, a pure function of
host state) over scripted call sequences.  The rule is driven through tests/primary_replay_driver.cpp, a stand-alone program built with AddressSanitizer and
UndefinedBehaviorSanitizer; the entry point and its Python mirror are checked against the header."""
import ctypes as C
import os
import re
import subprocess

import pytest

from helpers import ROOT, abi

SRC = os.path.join(ROOT, "tests", "primary_replay_driver.cpp")
INC = os.path.join(ROOT, "cis-565-final-vr-raytracer_amd", "csrc")


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    d = tmp_path_factory.mktemp("primary_replay")
    exe = str(d / "primary_replay_driver")
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


def launches(driver, script):
    """only the answers of the `launch` calls"""
    return [o for s, o in zip(script, driver(script)) if s.startswith("launch")]


def test_rest_move_rest(driver):
    # seven launches at rest, two at two new cameras, three at rest: the third launch at a camera records, later ones replay, a move starts over
    script = ["cam a"] + ["launch"] * 7 + ["cam b", "launch", "cam c", "launch", "cam d"] + ["launch"] * 3 + ["state"]
    out = driver(script)
    assert [o for s, o in zip(script, out) if s == "launch"] == ["normal", "normal", "record"] + ["replay"] * 4 + ["normal", "normal"] + ["normal", "normal", "record"]
    assert out[-1] == "state 1 atRest 2"
    # going back to a camera that was recorded earlier is a new camera: the planes hold the last recording only
    assert launches(driver, ["cam a"] + ["launch"] * 4 + ["cam b", "launch", "cam a"] + ["launch"] * 4) == \
        ["normal", "normal", "record", "replay", "normal", "normal", "normal", "record", "replay"]


def test_a_one_frame_pause_pays_for_no_recording(driver):
    script = []
    for k in range(6):   # a new camera every frame, except that cameras 2 and 4 are held for one more frame
        script += ["cam c%d" % k, "launch"] + (["launch"] if k in (2, 4) else [])
    assert launches(driver, script) == ["normal"] * 8


def test_every_invalidating_call_at_rest_starts_over(driver):
    # in state NONE (after one and after two launches) and in state VALID (after the recording, after a replay)
    for before in range(1, 6):
        script = ["cam a"] + ["launch"] * before + ["invalidate", "state"] + ["launch"] * 4
        out = driver(script)
        assert out[1 + before] == "dropped" and out[2 + before] == "state 0 atRest 0"
        assert out[3 + before:] == ["normal", "normal", "record", "replay"], before


def test_a_band_launch_and_an_ineligible_launch_never_replay_and_drop_the_state(driver):
    for flag in ("band", "ineligible", "band ineligible"):
        script = ["cam a"] + ["launch"] * 4 + ["launch " + flag, "state"] + ["launch"] * 4 + ["launch " + flag] * 4 + ["launch"]
        out = launches(driver, script)
        assert out == ["normal", "normal", "record", "replay", "normal"] + ["normal", "normal", "record", "replay"] + ["normal"] * 4 + ["normal"], flag
        assert driver(script)[6] == "state 0 atRest 0"
    # the first launches at a camera are bands: the count starts at the first full frame
    assert launches(driver, ["cam a", "launch band", "launch band", "launch", "launch", "launch", "launch"]) == ["normal"] * 4 + ["record", "replay"]


def test_the_rest_frame_count(driver):
    for rest, want in ((2, 2), (3, 3), (5, 5), (1, 2), (0, 2), (-4, 2)):   # below 2 the rule keeps 2: the second launch at a camera never records
        out = launches(driver, ["rest %d" % rest, "cam a"] + ["launch"] * (want + 3))
        assert out == ["normal"] * want + ["record", "replay", "replay"], rest


def test_cameras_that_differ_only_in_history_are_equal_and_one_bit_of_projinverse_is_not(driver):
    # lastProjView, lastPosition & co. change every frame of a camera at rest (they describe the PREVIOUS frame): not part of a view
    script = ["cam a", "launch", "history a", "launch", "history a", "launch", "history a", "launch"]
    assert launches(driver, script) == ["normal", "normal", "record", "replay"]
    for bit in (0, 1, 22, 23, 31, 32, 255, 256, 480, 511):   # mantissa, exponent and sign bits of several elements
        script = ["cam a"] + ["launch"] * 4 + ["flip a %d" % bit] + ["launch"] * 4 + ["flip a %d" % bit] + ["launch"] * 2
        assert launches(driver, script) == ["normal", "normal", "record", "replay"] * 2 + ["normal", "normal"], bit


def test_the_image_size_is_part_of_a_view(driver):
    script = ["cam a", "size 70 50"] + ["launch"] * 4 + ["size 50 70", "launch", "launch", "size 70 50", "launch"]
    assert launches(driver, script) == ["normal", "normal", "record", "replay", "normal", "normal", "normal"]


def test_header_library_and_python_mirror_have_the_entry_point():
    src = open(os.path.join(ROOT, "include", "rt_abi.h")).read()
    assert re.search(r"\bint rt_get_primary_replay_stats\(rt_ctx\* ctx, rt_primary_replay_stats\* out\);", src)
    m = re.search(r"#define RT_VIS_K_DEFAULT (\d+)", src)
    assert m and int(m.group(1)) in (8, 16, 32, 64)
    from restir_amd import renderer
    L = renderer.hip_lib()
    assert hasattr(L, "rt_get_primary_replay_stats") and "rt_get_primary_replay_stats" in renderer.ABI_SYMBOLS
    assert C.sizeof(abi.PrimaryReplayStats) == 32
    s = abi.PrimaryReplayStats()
    assert L.rt_get_primary_replay_stats(None, C.byref(s)) == abi.ERR_INVALID_ARG
