"""include/rt_capi_image.h's definition in numpy float32, for the tests: the two built-in tables by their float64 formulas, and the
encode itself -- one fp32 multiply, a count of thresholds reached, the transpose, the flip, the alpha.  Nothing here evaluates a
transfer curve on a pixel: like the definition, a code is comparisons against T."""
import os

import numpy as np

F = np.float32
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "image")
SRGB, LINEAR, CUSTOM = 0, 1, 2


def srgb_decode(u):
    """E(u), float64: the linear value of the sRGB-encoded u"""
    u = np.asarray(u, dtype=np.float64)
    return np.where(u <= 0.04045, u / 12.92, ((u + 0.055) / 1.055) ** 2.4)


def srgb_formula():
    """T[k] = (float)E((k - 0.5) / 255), k = 1..255, by this machine's pow (the fixture, not this, is the definition)"""
    return srgb_decode((np.arange(1, 256, dtype=np.float64) - 0.5) / 255.0).astype(F)


def linear_formula():
    """T[k] = (float)((2k - 1) / 510.0), k = 1..255"""
    return ((2.0 * np.arange(1, 256, dtype=np.float64) - 1.0) / 510.0).astype(F)


def srgb_fixture():
    """the committed table: 255 little-endian floats"""
    t = np.fromfile(os.path.join(GOLDEN, "srgb_thresholds.f32"), dtype="<f4")
    assert t.shape == (255,)
    return t.astype(F)


def table(transfer):
    return {"srgb": srgb_fixture, SRGB: srgb_fixture, "linear": linear_formula, LINEAR: linear_formula}[transfer]()


def codes(rgb, T, exposure=1.0):
    """float32 array of any shape -> uint8 codes of the same shape"""
    T = np.asarray(T, dtype=F)
    assert T.shape == (255,) and not np.isnan(T).any() and (T[1:] >= T[:-1]).all()
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        v = np.asarray(rgb, dtype=F) * F(exposure)            # one fp32 multiply (numpy keeps denormals)
    assert v.dtype == F
    n = np.searchsorted(T, v, side="right")                   # the number of T[k] <= v ... but numpy sorts NaN last: 255
    return np.where(np.isnan(v), 0, n).astype(np.uint8)


def encode(rgb, T, channels=3, exposure=1.0, bottom_up=False):
    """rgb float32 (Wn, H, 3) -> uint8 (H, Wn, channels)"""
    rgb = np.asarray(rgb, dtype=F)
    assert rgb.ndim == 3 and rgb.shape[2] == 3 and channels in (3, 4)
    c = codes(rgb, T, exposure).transpose(1, 0, 2)           # [z][x][c]
    if not bottom_up:
        c = c[::-1]                                          # row 0 is z = H - 1
    if channels == 4:
        c = np.concatenate([c, np.full(c.shape[:2] + (1,), 255, dtype=np.uint8)], axis=2)
    return np.ascontiguousarray(c)


def encode_into(out, pitch, x0, rgb, T, channels=3, exposure=1.0, bottom_up=False):
    """the bytes the definition names, written into the flat uint8 array `out` holding rows of `pitch` bytes, for a strip whose
    first column is x0 of the image: every other byte of out keeps its value"""
    img = encode(rgb, T, channels, exposure, bottom_up)
    H, Wn = img.shape[:2]
    for r in range(H):
        a = r * pitch + x0 * channels
        out[a:a + Wn * channels] = img[r].reshape(-1)
    return out
