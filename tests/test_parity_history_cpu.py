"""The histories of the temporal passes without a GPU: the rule that says when a frame of SVGF, TAA or temporal upsampling may read the
history of the other parity, and which frame a parity's planes hold (csrc/parity_history.h, plain host state), over scripted call sequences.  The rule is driven
through tests/parity_history_driver.cpp, a stand-alone program built with AddressSanitizer and UndefinedBehaviorSanitizer, and held against an independent model
of it below: every script of up to five steps, and a named case for each rule the GPU tests assert (test_invalidation_rules, test_reset_rules)."""
import itertools
import os
import subprocess

import pytest

from helpers import ROOT

SRC = os.path.join(ROOT, "tests", "parity_history_driver.cpp")
INC = os.path.join(ROOT, "cis-565-final-vr-raytracer_amd", "csrc")
INT_MIN, INT_MAX = -2 ** 31, 2 ** 31 - 1


class Model:
    """The rule, kept another way than the header keeps it: the frame whose pass was enqueued last, for as long as the next frame may read what it wrote, and
    per parity the frame whose images the planes hold."""

    def __init__(self):
        self.reset()

    def reset(self):
        self.chain, self.latest, self.planes = None, -1, {}

    def invalidate(self):
        self.chain = None

    def begin(self, f):
        readable = self.chain is not None and (f - self.chain) % 2 == 1
        self.chain = None
        self.planes.pop(f % 2, None)
        return readable

    def commit(self, f):
        self.chain, self.latest = f, f % 2
        self.planes[f % 2] = f

    def holds(self, f):
        return self.planes.get(f % 2) == f


def model(script):
    """the model's answers to the script's calls, in the driver's words"""
    m, out = Model(), []
    for line in script:
        op, _, arg = line.partition(" ")
        f = int(arg) if arg else None
        if op == "begin":
            out.append("read" if m.begin(f) else "fresh")
        elif op == "holds":
            out.append("yes" if m.holds(f) else "no")
        elif op == "latest":
            out.append(str(m.latest))
        elif op == "parity":
            out.append("%d %d" % (f % 2, 1 - f % 2))
        else:
            if op == "new":
                m = Model()
            elif op == "commit":
                m.commit(f)
            else:
                {"reset": m.reset, "invalidate": m.invalidate}[op]()
            out.append("ok")
    return out


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    d = tmp_path_factory.mktemp("parity_history")
    exe = str(d / "parity_history_driver")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-I", INC, SRC, "-o", exe])

    def run(script):
        """the driver's answers to the script's calls, one per call"""
        path = d / "script.txt"
        path.write_text("\n".join(script) + "\n")
        p = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=120)
        assert p.returncode == 0 and p.stderr == "", (p.returncode, p.stderr)
        out = p.stdout.split("\n")[:-1]
        assert len(out) == len(script)
        return out

    return run


def both(driver, script):
    """the answers to the script, on which driver and model agree"""
    got, want = driver(script), model(script)
    bad = [i for i in range(len(script)) if got[i] != want[i]]
    assert not bad, (bad[0], script[max(0, bad[0] - 12):bad[0] + 1], got[bad[0]], want[bad[0]])
    return got


def frame(f):
    """frame f runs its pass: begin and commit"""
    return ["begin %d" % f, "commit %d" % f]


# one step of a script: (the frame number moves on by 0, 1 or 2; the frame's pass is enqueued or not), or a call between frames
STEPS = [(d, commit) for commit in (True, False) for d in (0, 1, 2)] + ["invalidate", "reset"]


def scripts(base, length):
    """every script of `length` steps from frame number `base`, each from a new history; after every step: latest, and holds for the last three frame numbers"""
    out = []
    for steps in itertools.product(STEPS, repeat=length):
        out.append("new")
        f = base
        for s in steps:
            if isinstance(s, str):
                out.append(s)
            else:
                f += s[0]
                out += frame(f) if s[1] else ["begin %d" % f]
            out.append("latest")
            out += ["holds %d" % g for g in (f, f - 1, f - 2) if g >= INT_MIN]
    return out


def test_every_script_of_up_to_five_steps(driver):
    # (a script of fewer steps is the beginning of one of five, and every step is followed by the questions)
    script = scripts(0, 5)
    assert script.count("new") == 8 ** 5
    both(driver, script)


def test_frame_numbers_at_the_ends_of_int(driver):
    # three steps move on by up to 6: from -3 over -1 and 0, from INT_MIN, and up to INT_MAX - 1 and INT_MAX; (frames + 1) & 1 would overflow there
    for base in (-3, INT_MIN, INT_MAX - 6):
        both(driver, scripts(base, 3))
    ends = (-1, INT_MIN, INT_MAX - 1, INT_MAX)
    assert both(driver, ["parity %d" % f for f in ends]) == ["1 0", "0 1", "0 1", "1 0"]
    out = both(driver, frame(INT_MAX - 1) + frame(INT_MAX) + ["holds %d" % INT_MAX, "holds %d" % (INT_MAX - 1), "latest"] +   # consecutive: reads
               frame(INT_MIN) + ["holds %d" % INT_MIN, "holds %d" % INT_MAX] + frame(-1) + frame(0) + ["holds -1", "holds 0"])  # a counter that wraps: parities alternate
    assert out == ["fresh", "ok", "read", "ok", "yes", "yes", "1", "read", "ok", "yes", "yes", "read", "ok", "read", "ok", "yes", "yes"]


def test_a_skipped_frame_does_not_read(driver):
    # frames 4, 5, then 7: the history frame 7 would read is frame 5's, of its own parity (test_invalidation_rules: "a skipped frame")
    assert both(driver, frame(4) + frame(5) + frame(7) + frame(8)) == ["fresh", "ok", "read", "ok", "fresh", "ok", "read", "ok"]
    # ... and a frame number rendered twice does not read itself
    assert both(driver, frame(4) + frame(4))[2] == "fresh"


def test_a_frame_after_invalidate_does_not_read(driver):
    # (the setters, the *_reset calls, rt_upload_scene, rt_build_accel); the frame after it reads again, and what the planes hold is untouched
    out = both(driver, frame(4) + frame(5) + ["invalidate", "holds 5", "latest"] + frame(6) + frame(7))
    assert out == ["fresh", "ok", "read", "ok", "ok", "yes", "1", "fresh", "ok", "read", "ok"]


def test_a_frame_after_an_uncommitted_frame_does_not_read(driver):
    # frame 6 began and its pass did not run (mode off, a debug view, an error return): frame 7 starts without history
    out = both(driver, frame(4) + frame(5) + ["begin 6", "latest"] + frame(7) + frame(8))
    assert out == ["fresh", "ok", "read", "ok", "read", "1", "fresh", "ok", "read", "ok"]


def test_holds_is_false_after_a_later_frame_of_the_same_parity_began(driver):
    # rt_tonemap / rt_upscale_tonemap of frame 4 after frame 6 began: the planes are being overwritten, whether or not frame 6 commits
    out = both(driver, frame(4) + frame(5) + ["holds 4", "holds 5", "begin 6", "holds 4", "holds 5", "holds 6", "commit 6", "holds 4", "holds 6"])
    assert out[4:] == ["yes", "yes", "read", "no", "yes", "no", "ok", "no", "yes"]


def test_reset_forgets_the_planes_and_a_new_history_is_a_reset_one(driver):
    out = both(driver, ["latest", "holds 0"] + frame(4) + frame(5) + ["reset", "latest", "holds 4", "holds 5"] + frame(6))
    assert out == ["-1", "no", "fresh", "ok", "read", "ok", "ok", "-1", "no", "no", "fresh", "ok"]
