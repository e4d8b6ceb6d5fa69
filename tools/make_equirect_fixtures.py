#!/usr/bin/env python3
"""Dev-time: store the reference's two equirectangular test images (test/data/equirectangular_image_00{1,2}.jpg) at their native
1920 x 960 as gray PNGs under tests/golden/ (equirect{1,2}_1920x960.png), for the equirectangular camera tests of the post-extract step.
Gray = PIL 'L' conversion, as tools/make_fixtures.py.  The reference tree is not needed to run the tests: the PNGs are committed.

usage: make_equirect_fixtures.py <reference source root>
"""
import pathlib
import sys

from PIL import Image

out = pathlib.Path(__file__).resolve().parents[1] / "tests" / "golden"
out.mkdir(parents=True, exist_ok=True)
ref = pathlib.Path(sys.argv[1])
for idx in (1, 2):
    im = Image.open(ref / "test" / "data" / f"equirectangular_image_00{idx}.jpg").convert("L")
    assert im.size == (1920, 960), im.size
    im.save(out / f"equirect{idx}_1920x960.png", optimize=True)
print(sorted(p.name for p in out.glob("equirect*_1920x960.png")))
