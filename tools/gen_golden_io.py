#!/usr/bin/env python3
"""Golden cases for faster_rcnn/utils_io.get_image: the reference's own get_image (utils.py:111-132), imported from where it
lies as tools/gen_golden.py does, with cv2.imdecode stubbed and np.fromfile recording the path it is given.  Each case holds the
inputs (path, types, random_type, seed of NumPy's global stream), the path the reference opened and the position of the stream
after the call (its next uniform draw).  Data only.

    python tools/gen_golden_io.py         # rewrites tests/golden/get_image.json
"""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gen_golden as G  # noqa: E402

TYPES = {2: ["blended_grey", "depth"], 3: ["blended_grey", "depth", "normal"], 5: ["blended_grey", "depth", "normal", "ao", "pro"]}
PATHS = ["data/panel_01.png", "data/site/wall/panel_02.png", "/srv/maps/panel_03.png", "panel_04.png"]


def main():
    _, _, rutils, _ = G._import_reference()
    import cv2
    cv2.IMREAD_COLOR = 1
    cv2.imdecode = lambda buf, flag: buf
    seen = []
    real = np.fromfile

    def fromfile(path, dtype=None, *a, **kw):
        seen.append(path)
        return np.zeros(1, np.uint8)

    cases = []
    np.fromfile = fromfile
    try:
        for i, (path, n, random_type) in enumerate([(p, n, r) for r in (False, True) for p, n in zip(PATHS + PATHS[:2], (2, 3, 5, 3, 5, 2))]):
            seed = 100 + i
            np.random.seed(seed)
            del seen[:]
            rutils.get_image(path, list(TYPES[n]), random_type=random_type)
            cases.append(dict(img_path=path, types=TYPES[n], random_type=random_type, seed=seed, opened=seen[0], next_uniform=float(np.random.random())))
    finally:
        np.fromfile = real
    with open(os.path.join(G.OUT, "get_image.json"), "w") as f:
        json.dump(dict(numpy=np.__version__, cases=cases), f, indent=1)
        f.write("\n")
    print("wrote %d cases" % len(cases))


if __name__ == "__main__":
    main()
