"""Mints tests/golden/ref_live_digests.json from the REFERENCE's own shaders compiled for the CPU (oracle/_ref/libref_stages.so,
built from /root/reference by oracle/kat/build_ref_stages.sh) — run in the authoring container:

    python tests/golden/make_ref_live_digests.py

Per live case of tests/test_ref_stages.py (LIVE_KEYS) and frame, the SHA-256 of every screen-space buffer the compiled reference
produces.  Where the library cannot be built, the live tests hold the oracle to these digests instead of to the library.  The file
holds digests only; no reference source is stored.
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import test_ref_stages as T  # noqa: E402
from oracle import ref_binding  # noqa: E402


def main():
    assert ref_binding.build(), "needs /root/reference (authoring container)"
    out = {}
    for key in T.LIVE_KEYS:
        sc, env, st, W, H, frames, moving, stages, sky = T.live_case(key)
        r = T.make_backend(ref_binding.Reference, sc, env, W, H, sky)
        out[key] = {}
        def grab(f):
            out[key][f"f{f}"] = T.frame_digests(r, f)
        T.drive([r], sc, st, W, H, frames, moving, stages, grab)
    with open(T.LIVE_DIGESTS, "w") as fh:
        json.dump(out, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print("wrote", T.LIVE_DIGESTS, os.path.getsize(T.LIVE_DIGESTS), "bytes,", len(out), "cases")


if __name__ == "__main__":
    main()
