#!/usr/bin/env python3
"""Input fixtures: the reference's own test inputs, the data its tests/input_files/ holds -- OpenSCENARIO scenarios and the
catalogs they name, road-network JSON files -- for the tests that read them (tests/test_host_api.py, tests/test_ingest_json.py):

  inputs_xosc.npz     Scenarios/*.xosc + Catalogs/**/*.xosc
  inputs_roads_1.npz  Road_Networks/*.json, the two largest networks
  inputs_roads_2.npz  Road_Networks/*.json, the other four (two files: each stays under 1 MiB)

    SG_REFERENCE=<checkout of the reference> python tests/golden/make_golden_inputs.py

Every file is one uint8 array under its path relative to tests/input_files/, xz-compressed (lzma preset 9 | extreme); the
`reference_inputs` fixture of tests/conftest.py unpacks them into a directory of the same layout (the scenarios name their
catalogs and road networks by relative paths).  Only DATA is written: the files' bytes, unchanged."""
import lzma
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.environ.get("SG_GOLDEN_OUT", HERE)
REF = os.environ.get("SG_REFERENCE")
if not REF:
    raise SystemExit("make_golden_inputs: set SG_REFERENCE to a checkout of the reference")
SRC = os.path.join(REF, "tests", "input_files")
ROADS_1 = ["Greenwich_Road_Network_002.json", "Rural_Road_Network.json"]


def files(sub, ext):
    top = os.path.join(SRC, sub)
    return sorted(os.path.relpath(os.path.join(d, f), SRC) for d, _, fs in os.walk(top) for f in fs if f.endswith(ext))


def write(stem, rels):
    arrays = {}
    for rel in rels:
        with open(os.path.join(SRC, rel), "rb") as f:
            arrays[rel] = np.frombuffer(lzma.compress(f.read(), preset=9 | lzma.PRESET_EXTREME), np.uint8)
    np.savez(os.path.join(OUT, stem + ".npz"), **arrays)


roads = files("Road_Networks", ".json")
assert all(os.path.join("Road_Networks", n) in roads for n in ROADS_1)
write("inputs_xosc", files("Scenarios", ".xosc") + files("Catalogs", ".xosc"))
write("inputs_roads_1", [os.path.join("Road_Networks", n) for n in ROADS_1])
write("inputs_roads_2", [r for r in roads if os.path.basename(r) not in ROADS_1])
