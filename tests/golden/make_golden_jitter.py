"""Writes tests/golden/g13_jitter.npz: Pillow's own colour jitter on two small images, made with Pillow alone.

    python tests/golden/make_golden_jitter.py

What Pillow computes is taken from its public interface only: ImageEnhance.Brightness / Contrast / Color (what torchvision's
adjust_brightness / adjust_contrast / adjust_saturation call) and the HSV round trip of adjust_hue -- convert("HSV"), a uint8 add
on the H plane that wraps, convert("RGB").  Two random uint8 images that also hold gray, black, white and primary pixels, one of
37x53 and one of 70x131.  For each:
  * all 24 orders of the four operations at FACTORS and SHIFT, each operation on the uint8 result of the one before;
  * every single operation at the factors SINGLE_FACTORS, and the hue round trip at SINGLE_SHIFTS.
A result is 6 to 28 KB of noise that does not compress, and there are 90 of them, so the file holds the SHA-256 of every result's
bytes ([H,W,3] uint8, C order) and, in full, the results of the four orders FULL_ORDERS on the small image: a test that misses a
digest computes the numpy restatement to name the first differing pixel.  Also the SHA-256 of the hue round trip over the
4096x4096 image of all 2^24 colours (colour c at pixel c: R = c >> 16, G = (c >> 8) & 255, B = c & 255) at shifts 0 and 77, and
the Pillow version."""
import hashlib
import itertools
import os

import numpy as np
import PIL
from PIL import Image, ImageEnhance

FACTORS = (0.83, 1.17, 1.4)                   # brightness, contrast, saturation
SHIFT = 77
SINGLE_FACTORS = (0.0, 0.6, 0.83, 1.0, 1.17, 1.4)
SINGLE_SHIFTS = (0, 77, 231)
ORDERS = list(itertools.permutations(range(4)))
FULL_ORDERS = ((0, 1, 2, 3), (1, 3, 0, 2), (2, 0, 3, 1), (3, 2, 1, 0))
SIZES = {"small": (37, 53), "large": (70, 131)}
ENHANCERS = (ImageEnhance.Brightness, ImageEnhance.Contrast, ImageEnhance.Color)


def make_image(h, w, seed):
    rng = np.random.default_rng(seed)
    img = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    img[0, :16] = np.repeat(rng.integers(0, 256, (16, 1), dtype=np.uint8), 3, 1)       # grays: max == min
    img[1, :8] = [(0, 0, 0), (255, 255, 255), (255, 0, 0), (0, 255, 0), (0, 0, 255), (255, 255, 0), (0, 255, 255), (255, 0, 255)]
    img[2, :w // 2, 1] = img[2, :w // 2, 0]                                             # ties between two channels
    return img


def pil_hue(im, shift):
    h, s, v = im.convert("HSV").split()
    np_h = np.array(h, dtype=np.uint8)
    with np.errstate(over="ignore"):
        np_h += np.uint8(shift)
    return Image.merge("HSV", (Image.fromarray(np_h, "L"), s, v)).convert("RGB")


def pil_op(im, code, factors, shift):
    return pil_hue(im, shift) if code == 3 else ENHANCERS[code](im).enhance(factors[code])


def pil_jitter(img, factors, order, shift):
    im = Image.fromarray(img, "RGB")
    for code in order:
        im = pil_op(im, code, factors, shift)
    return np.array(im)


def all_colours():
    c = np.arange(1 << 24, dtype=np.uint32)
    return np.stack([c >> 16, (c >> 8) & 255, c & 255], -1).astype(np.uint8).reshape(4096, 4096, 3)


def digest(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def main():
    out = {"pillow_version": np.array(PIL.__version__), "factors": np.array(FACTORS), "shift": np.array(SHIFT),
           "single_factors": np.array(SINGLE_FACTORS), "single_shifts": np.array(SINGLE_SHIFTS), "orders": np.array(ORDERS, np.int32),
           "full_orders": np.array(FULL_ORDERS, np.int32)}
    for seed, (name, (h, w)) in enumerate(SIZES.items()):
        img = make_image(h, w, 20130 + seed)
        out[f"{name}_image"] = img
        out[f"{name}_order_sha"] = np.array([digest(pil_jitter(img, FACTORS, o, SHIFT)) for o in ORDERS])
        out[f"{name}_single_sha"] = np.array([[digest(pil_jitter(img, (f, f, f), (code,), 0)) for f in SINGLE_FACTORS] for code in range(3)])
        out[f"{name}_hue_sha"] = np.array([digest(pil_jitter(img, FACTORS, (3,), s)) for s in SINGLE_SHIFTS])
    out["small_full"] = np.stack([pil_jitter(out["small_image"], FACTORS, o, SHIFT) for o in FULL_ORDERS])
    colours = all_colours()
    out["all_colours_hue_sha"] = np.array([digest(pil_jitter(colours, FACTORS, (3,), s)) for s in (0, 77)])
    out["all_colours_shifts"] = np.array([0, 77])
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "g13_jitter.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes, Pillow", PIL.__version__)


if __name__ == "__main__":
    main()
