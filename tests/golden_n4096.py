"""Loader for the N = 4096 golden fixtures (tests/golden/N4096/, made by `tools/gen_golden.js --n4096`).

They have a manifest of their own (tests/golden/N4096/manifest.json, the layout of tests/golden/manifest.json
with the one size), so golden_io's loader reads them once it is handed that manifest."""
import json
import os

import golden_io

N = 4096


def manifest():
    with open(os.path.join(golden_io.GOLDEN, "N4096", "manifest.json")) as f:
        return json.load(f)


def load():
    """golden_io.load(4096), from the size's own manifest."""
    m = manifest()
    old = golden_io.manifest
    golden_io.manifest = lambda: m
    try:
        return golden_io.load(N)
    finally:
        golden_io.manifest = old
