#!/usr/bin/env python3
"""PNG files for the PNG reader test on real camera content (tests/test_frontend_and_eval.py), written from the committed
kinect50mm_excerpt.npz (pixel data of the reference's data/KINECT_50MM, see make_real_fixtures.py):

  kinect50mm_rgb8.png     the colour excerpt without its alpha channel: 8-bit RGB, 212 x 256 (the form of the webcam frames)
  kinect50mm_depth16.png  the depth excerpt: 16-bit gray, 212 x 256, sensor holes included

Encoded by PIL with its defaults (adaptive per-row filters, zlib): real image content makes the encoder pick every filter type.
    python tests/golden/make_png_fixtures.py
"""
import os

import numpy as np
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))


def main():
    fx = np.load(os.path.join(HERE, "kinect50mm_excerpt.npz"))
    rgb = np.ascontiguousarray(fx["rgba"][..., :3])
    d16 = np.ascontiguousarray(fx["depth16"])
    Image.fromarray(rgb).save(os.path.join(HERE, "kinect50mm_rgb8.png"))
    Image.fromarray(d16).save(os.path.join(HERE, "kinect50mm_depth16.png"))


if __name__ == "__main__":
    main()
