"""Writes tests/golden/face_crops_pil.npz: six small uint8 sources and the bytes Pillow's
Image.fromarray(a).resize((128, 128), Image.BILINEAR) returns for each, with the Pillow version that made them.  The fixture is
what tests/test_face_crops_host.py and tests/test_gpu_face_crops.py compare with on machines without Pillow."""
import os

import numpy as np
import PIL
from PIL import Image

SHAPES = [(1, 1), (2, 3), (75, 75), (129, 127), (37, 300), (300, 2)]          # (height, width); the last is a tall strip (h > 100 w)


def main():
    rng = np.random.default_rng(20240611)
    out = {"pillow_version": np.array(PIL.__version__), "shapes": np.array(SHAPES, dtype=np.int32)}
    for i, (h, w) in enumerate(SHAPES):
        a = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        out[f"src{i}"] = a
        out[f"out{i}"] = np.asarray(Image.fromarray(a).resize((128, 128), Image.BILINEAR))
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "face_crops_pil.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
