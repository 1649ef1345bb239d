"""The reference of include/rt_capi_adaptive.h, for the tests: FLAGS restated in numpy float32 over whole rectangles, and the
frame as a selection between two frames.  Every comparison is the header's -- ~(t >= cos), ~(|d| <= thr) -- so that a NaN flags
the pixel; never a `<` or a maximum."""
import numpy as np

F = np.float32


def _differ(rgb_p, hit_p, rgb_q, hit_q, thr, cos):
    """differ(p, q) of the header, elementwise over two equally shaped windows of a rectangle"""
    with np.errstate(all="ignore"):
        n_p, n_q = hit_p["normal"].astype(F), hit_q["normal"].astype(F)
        t = (n_p[..., 0] * n_q[..., 0] + n_p[..., 1] * n_q[..., 1]).astype(F) + (n_p[..., 2] * n_q[..., 2]).astype(F)
        d = hit_p["object"] != hit_q["object"]
        d = d | ((hit_p["object"] >= 0) & ~(t.astype(F) >= F(cos)))
        diff = np.abs((rgb_p.astype(F) - rgb_q.astype(F)).astype(F))
        d = d | (~(diff <= F(thr))).any(axis=-1)
    return d


def flags(rgb, hits, color_threshold=1 / 32, normal_cos=0.9, flag_all=False):
    """FLAGS of a rectangle: rgb float32 (Wn, H, 3), hits HIT_DTYPE (Wn, H) -> bool (Wn, H).  Only neighbours inside the rectangle
    exist."""
    rgb = np.asarray(rgb, dtype=F)
    Wn, H = rgb.shape[:2]
    assert hits.shape == (Wn, H), (hits.shape, rgb.shape)
    out = np.full((Wn, H), bool(flag_all))
    if Wn > 1:                                                         # (x+1, z)
        out[:-1, :] |= _differ(rgb[:-1], hits[:-1], rgb[1:], hits[1:], color_threshold, normal_cos)
    if H > 1:                                                          # (x, z+1)
        out[:, :-1] |= _differ(rgb[:, :-1], hits[:, :-1], rgb[:, 1:], hits[:, 1:], color_threshold, normal_cos)
    if Wn > 1 and H > 1:                                               # (x+1, z+1)
        out[:-1, :-1] |= _differ(rgb[:-1, :-1], hits[:-1, :-1], rgb[1:, 1:], hits[1:, 1:], color_threshold, normal_cos)
    return out


def frame_flags(rgb, hits, x0, x1, **kw):
    """the flags of columns [x0, x1) of a whole frame's colours and records: FLAGS of columns [x0, min(x1 + 1, W)), cropped"""
    W = rgb.shape[0]
    x1h = min(x1 + 1, W)
    return flags(rgb[x0:x1h], hits[x0:x1h], **kw)[:x1 - x0]


def expected_frame(flags_, ssaa, plain):
    """where(flags, ssaa, plain) per pixel, bits kept"""
    assert ssaa.shape == plain.shape == flags_.shape + (3,), (flags_.shape, ssaa.shape, plain.shape)
    return np.where(flags_[..., None], ssaa.view(np.uint32), plain.view(np.uint32)).view(F)


def share(flags_):
    return float(flags_.mean())


def assert_share(flags_, what, lo=0.05, hi=0.75):
    """the share condition: a frame compared bit for bit holds flagged and unflagged pixels, the flagged between 5 % and 75 %"""
    s = share(flags_)
    assert lo <= s <= hi, f"{what}: flagged share {s:.3f} outside [{lo}, {hi}]: where(flags, ...) would test one branch only"
    return s
