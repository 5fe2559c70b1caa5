#!/usr/bin/env python3
"""Is the device code of every build of the traced stages and of the reference tracer what another tree's is?  No GPU needed.

  python scripts/stage_builds_ab.py <path of the other checkout> [jobs]

For each entry of STAGE_BUILDS and REFERENCE_BUILDS (restir_amd/build.py) the unit is compiled device-only, unbundled and with a fixed unit id, with the product
flags, from the other tree and from this one, and the two gfx950 code objects are compared byte for byte.  (The object files of these units cannot be compared
with cmp: they carry the unit id, which is a hash of the source path and the command line.)  A tree from before the table, which has a stub file per build
(csrc/stages_sky_lat.hip, ...), is compiled through its stubs.  One line per build, then the verdict; the exit status is the number of builds that differ."""
import importlib.util
import os
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = "cis-565-final-vr-raytracer_amd"


def load_build(root):
    spec = importlib.util.spec_from_file_location("build_of_" + str(abs(hash(root))), os.path.join(root, PKG, "build.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def device_object(root, flags, src, stem, switches, out):
    """the gfx950 code object of one unit of the tree at `root`: through its stub file where the tree has one, else the source with the entry's switches"""
    csrc = os.path.join(root, PKG, "csrc")
    stub = os.path.join(csrc, stem + ".hip")
    unit = [stub] if os.path.exists(stub) else ["-D%s=1" % s for s in switches] + [os.path.join(csrc, src)]
    cmd = [os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")] + flags + ["--cuda-device-only", "--no-gpu-bundle-output", "-cuid=fixed", "-c"] + unit + ["-o", out]
    subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    return open(out, "rb").read()


def main():
    if len(sys.argv) < 2:
        sys.exit(__doc__)
    other = os.path.abspath(sys.argv[1])
    jobs = int(sys.argv[2]) if len(sys.argv) > 2 else 8
    build = load_build(ROOT)
    units = [u for u in build.hip_units() if u[0] in ("stages.hip", "reference.hip")]
    flags = [("-Os" if f == "-O3" else f) for f in build.HIP_FLAGS if f != "-shared"]   # as build_hip compiles a kernel unit
    tmp = tempfile.mkdtemp(prefix="stage_builds_ab_")

    def one(u):
        src, stem, switches = u
        a = device_object(other, flags, src, stem, switches, os.path.join(tmp, stem + ".other.co"))
        b = device_object(ROOT, flags, src, stem, switches, os.path.join(tmp, stem + ".this.co"))
        return stem, switches, len(a), len(b), a == b

    with ThreadPoolExecutor(jobs) as pool:
        rows = list(pool.map(one, units))
    print("# device code of %s, other tree = its stub file or the same switches, this tree = the source + switches; %s" % (PKG + "/csrc", " ".join(flags)))
    for stem, switches, na, nb, same in rows:
        print("%-20s %-34s %9d B %9d B  %s" % (stem, " ".join("-D%s=1" % s for s in switches) or "-", na, nb, "identical" if same else "DIFFERENT"))
    bad = [r[0] for r in rows if not r[4]]
    print("verdict: %d of %d code objects identical%s" % (len(rows) - len(bad), len(rows), "" if not bad else "; different: " + " ".join(bad)))
    return len(bad)


if __name__ == "__main__":
    sys.exit(main())
