"""Copies the 19 stock OpenCV Haar XMLs the reference ships into tests/golden/xml/ as haarcascade_<name>.xml.xz (verbatim
text, xz-compressed), so that the loader tests read the XML itself on any machine, without the reference checkout.

    python tools/make_xml_golden.py <directory of the reference's haarcascade_*.xml files>
"""
import glob
import lzma
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "xml")

src = sys.argv[1]
paths = sorted(glob.glob(os.path.join(src, "haarcascade_*.xml")))
assert len(paths) == 19, f"expected the 19 stock XMLs in {src}, found {len(paths)}"
os.makedirs(OUT, exist_ok=True)
for p in paths:
    data = open(p, "rb").read()
    with open(os.path.join(OUT, os.path.basename(p) + ".xz"), "wb") as f:
        f.write(lzma.compress(data, preset=9 | lzma.PRESET_EXTREME))
    print(os.path.basename(p), len(data))
