#!/usr/bin/env python3
"""Regenerate tests/golden/*.f32 (packed fp32 framebuffers, [x][z][3]).

The images are produced by the CPU oracle (oracle/rt_oracle.c) and are kept
only if their SHA-256 equals the digest SURVEY.md Appendix D recorded for the
same scene/size/depth from the survey's build of the reference.  This script
does not run the reference; make_ref_pins.py does, through oracle/_ref/ref_harness,
and writes the same three files byte for byte.
Also writes extra.json: digests of larger oracle renders used by GPU tests; each
of them is also in ref/digests.json, where the reference's binary wrote it.
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import oracle_lib  # noqa: E402

for key in ("b64d4", "g32_64d4", "g16_64d8"):
    name, W, H, depth, digest = oracle_lib.SURVEY_PINS[key]
    img = oracle_lib.OracleScene.named(name).render(W, H, depth)
    assert oracle_lib.sha256(img) == digest, key
    img.tofile(os.path.join(HERE, key + ".f32"))
    print("wrote", key, digest)

extra = {"_about": "SHA-256 of oracle renders (oracle/rt_oracle.c) that the GPU tests meet.  Every value here is also the digest of "
                   "the reference's own frame: tests/golden/ref/digests.json, written by a build of the reference's sources "
                   "(golden/make_ref_pins.py), holds the same cases, and test_reference_pins_cpu.py asserts the two files equal."}
for name, W, H, depth in (("grid32", 64, 64, 4), ("grid16", 64, 64, 8), ("twomirrors", 48, 48, 6),
                          ("builtin", 500, 504, 50), ("grid32", 256, 256, 4), ("grid16", 256, 256, 8)):
    img = oracle_lib.OracleScene.named(name).render(W, H, depth)
    extra[f"{name}_{W}x{H}_d{depth}"] = oracle_lib.sha256(img)
json.dump(extra, open(os.path.join(HERE, "extra.json"), "w"), indent=1, sort_keys=True)
print(extra)
