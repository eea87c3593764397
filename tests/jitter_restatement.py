"""The colour jitter of include/ecm_augment.h restated in numpy, operation for operation: what
tests/test_color_jitter_cpu.py holds to Pillow and tests/test_hip_color_jitter.py holds the kernels to.  Not a test module.

Every fp32 operation below is one numpy float32 operation (numpy rounds each one separately: there is no fused multiply-add), and
the fp64 ones are float64 operations on widened values."""
import numpy as np

BRIGHTNESS, CONTRAST, SATURATION, HUE = 0, 1, 2, 3
F32, F64 = np.float32, np.float64


def gray(img):
    """L of an [..., 3] uint8 image, uint8."""
    a = img.astype(np.int64)
    return ((19595 * a[..., 0] + 38470 * a[..., 1] + 7471 * a[..., 2] + 0x8000) >> 16).astype(np.uint8)


def blend(deg, img, f):
    """deg + f * (img - deg) in fp32, 0 where <= 0, 255 where >= 255, truncated between (for 0 <= f <= 1 that IS the truncation)."""
    f = F32(f)
    d, a = np.asarray(deg).astype(F32), img.astype(F32)
    t = d + f * (a - d)
    out = np.where(t <= 0, 0, np.where(t >= 255, 255, t)).astype(F32)
    return np.broadcast_to(out.astype(np.int32).astype(np.uint8), img.shape).copy()


def contrast_mean(img):
    """floor((2 S + n) / (2 n)) over the gray image: PIL's int(mean + 0.5)."""
    L = gray(img)
    S, n = int(L.astype(np.int64).sum()), L.size
    return (2 * S + n) // (2 * n)


def rgb_to_hsv(img):
    a = img.astype(np.int32)
    r, g, b = a[..., 0], a[..., 1], a[..., 2]
    mx, mn = np.maximum(np.maximum(r, g), b), np.minimum(np.minimum(r, g), b)
    flat = mx == mn
    cr = np.where(flat, 1, mx - mn).astype(F32)
    mxf = np.where(flat, 1, mx).astype(F32)
    s = cr / mxf
    rc, gc, bc = (mx - r).astype(F32) / cr, (mx - g).astype(F32) / cr, (mx - b).astype(F32) / cr
    h = np.where(r == mx, (bc - gc).astype(F64),
                 np.where(g == mx, F64(2.0) + rc.astype(F64) - bc.astype(F64), F64(4.0) + gc.astype(F64) - rc.astype(F64)))
    h = h.astype(F32).astype(F64)
    h = np.fmod(h / F64(6.0) + F64(1.0), F64(1.0)).astype(F32)
    uh = np.clip((h.astype(F64) * F64(255.0)).astype(np.int32), 0, 255)
    us = np.clip((s.astype(F64) * F64(255.0)).astype(np.int32), 0, 255)
    uh, us = np.where(flat, 0, uh), np.where(flat, 0, us)
    return np.stack([uh, us, mx], -1).astype(np.uint8)


def hsv_to_rgb(hsv):
    h, s, v = hsv[..., 0].astype(F32), hsv[..., 1].astype(F32), hsv[..., 2].astype(F32)
    one, half = F32(1), F32(0.5)
    fs = s / F32(255)
    f = h * F32(6) / F32(255)
    i = np.floor(f)
    f = f - i
    p = np.clip(np.floor(v * (one - fs) + half), 0, 255)
    q = np.clip(np.floor(v * (one - fs * f) + half), 0, 255)
    t = np.clip(np.floor(v * (one - fs * (one - f)) + half), 0, 255)
    i = i.astype(np.int32) % 6
    r = np.choose(i, [v, q, p, p, t, v])
    g = np.choose(i, [t, v, v, q, p, p])
    b = np.choose(i, [p, p, t, v, v, q])
    flat = hsv[..., 1] == 0
    out = np.stack([np.where(flat, v, r), np.where(flat, v, g), np.where(flat, v, b)], -1)
    return out.astype(np.uint8)


def hue(img, shift):
    hsv = rgb_to_hsv(img)
    hsv[..., 0] = (hsv[..., 0].astype(np.int32) + int(shift)) % 256
    return hsv_to_rgb(hsv)


def hue_shift_of(hue_factor):
    """adjust_hue's np.uint8(hue_factor * 255) wrap: trunc(hue_factor * 255) mod 256, in double."""
    return int(float(hue_factor) * 255) % 256


def apply_op(img, code, factors, shift):
    if code == BRIGHTNESS:
        return blend(0, img, factors[BRIGHTNESS])
    if code == CONTRAST:
        return blend(contrast_mean(img), img, factors[CONTRAST])
    if code == SATURATION:
        return blend(gray(img)[..., None], img, factors[SATURATION])
    if code == HUE:
        return hue(img, shift)
    raise ValueError(code)


def jitter(img, factors, order, shift):
    """One [H,W,3] uint8 view through the operations of `order` (codes, -1 = none), each on the uint8 result of the one before."""
    out = np.ascontiguousarray(img)
    for code in order:
        if code >= 0:
            out = apply_op(out, int(code), factors, shift)
    return out


def finish(u8, pca, mean, std):
    """KITTI.py:171-191 behind the jitter, in fp32: (image [3,H,W] clamped to 0..1, the normalised view [3,H,W]).  The tests' reference is
    frame_fixtures.loader_statements; tests/test_color_jitter_cpu.py holds the two to each other."""
    x = u8.astype(F32).transpose(2, 0, 1) / F32(255)
    x = x + np.asarray(pca, F32).reshape(3, 1, 1)
    x = np.minimum(np.maximum(x, F32(0)), F32(1))
    return x, (x - np.asarray(mean, F32).reshape(3, 1, 1)) / np.asarray(std, F32).reshape(3, 1, 1)
