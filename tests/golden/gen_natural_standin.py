#!/usr/bin/env python3
"""Generates tests/golden/standin/{in,tar}{0,1,2,3,4}.png: committed stand-ins for the reference's ten demo photographs (demo/example/in/*.png, third-party images
that are never committed), with what the natural-image tests exist to exercise and cosines + noise lack:
  - large groups of ONE colour: a flat rectangle over a quarter of the image and a disc (kNN hubs with in-degrees in the thousands, many-source vote targets,
    stiff WLS systems), and a posterised band along the bottom (a few colours repeated over thousands of pixels);
  - isolated colours: a few single pixels of a saturated colour far from everything else in the image;
  - sharp one-pixel edges: a block of alternating light / dark columns (text-like structure).
Sizes are the demo's divided by 3, colour types the demo's (RGBA where the demo file is RGBA: the alpha channel must be dropped), so the CPU oracle runs a pair in
seconds. Deterministic: a second run writes the same pixels. The pair_<case>.npz fixtures next to them come from gen_natural.py."""
import os
import sys
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(HERE)), "scripts"))
import numpy as np
from PIL import Image
import natural_inputs
import synth
from demo_validate import DEMO_GEOMETRY


def standin(seed, H, W):
    img = synth.image_flat(seed, H, W)
    rng = np.random.default_rng(seed + 91)
    yy, xx = np.mgrid[0:H, 0:W]
    cy, cx, r = H * 3 // 4 - H // 8, W * 3 // 4, min(H, W) // 6
    img[(yy - cy) ** 2 + (xx - cx) ** 2 <= r * r] = rng.integers(30, 220, 3)
    y0, x0 = H // 16, W - W // 5
    img[y0:y0 + H // 6, x0:x0 + W // 8] = 235
    img[y0:y0 + H // 6, x0:x0 + W // 8:2] = 15
    for _ in range(6):
        img[int(rng.integers(0, H)), int(rng.integers(0, W))] = (255, 0, 255)
    return img


def main():
    os.makedirs(natural_inputs.STANDIN_DIR, exist_ok=True)
    for i, name in enumerate(natural_inputs.NAMES):
        w, h, mode = DEMO_GEOMETRY[name]
        bgr = standin(3000 + i, h // 3, w // 3)
        rgb = np.ascontiguousarray(bgr[..., ::-1])
        if mode == "RGBA":
            alpha = np.broadcast_to(np.linspace(255, 96, w // 3).astype(np.uint8)[None, :, None], (h // 3, w // 3, 1))       # dropped on read
            im = Image.fromarray(np.concatenate([rgb, alpha], -1), "RGBA")
        else:
            im = Image.fromarray(rgb, "RGB")
        im.save(os.path.join(natural_inputs.STANDIN_DIR, name + ".png"), optimize=True)
        print(name, im.size, im.mode)


if __name__ == "__main__":
    main()
