"""The reference of include/rt_clamp.h, for the tests: the header's definition restated in numpy float32, vectorised per tap -- for
each offset (a, b) of the window, in the header's order, every pixel's tap at once, one rounding per operation (numpy's float32
ufuncs do not contract, and divide and take square roots correctly rounded).  Comparisons are written as the header writes them,
so that a NaN gives "skip" or "leave": where(t > 0, t, 0), never maximum; where(c < mn, c, mn), never minimum."""
import numpy as np

from denoise_ref import _window
from svgf_ref import dead_records, lum

F = np.float32
NAMES = ("value", "moments", "length", "variance", "flags")


def clamp(cur, hits, value, moments, length, box=0, radius=1, match_color=True, min_taps=3, clip_history=4, normal_cos=0.9,
          gamma=1.0, details=False):
    """rt_history_clamp: cur and value float32 (Wn, H[, 3]), hits HIT_DTYPE (Wn, H), moments (Wn, H, 2), length (Wn, H) ->
    (value, moments, length, variance, flags uint8); with details also a dict: "walked", bool (Wn, H), the live pixels with a
    history longer than one, and "taps", float32 (Wn, H), the taps the window counted"""
    cur, value = np.ascontiguousarray(cur, dtype=F), np.ascontiguousarray(value, dtype=F)
    moments, length = np.ascontiguousarray(moments, dtype=F), np.ascontiguousarray(length, dtype=F)
    Wn, H = hits.shape
    c, v = cur.reshape(Wn, H, -1), value.reshape(Wn, H, -1)
    assert c.shape[2] in (1, 3) and v.shape == c.shape and moments.shape == (Wn, H, 2) and length.shape == (Wn, H)
    assert box in (0, 1) and 1 <= radius <= 3 and 1 <= min_taps <= 49 and 1 <= clip_history <= 65535
    dead = dead_records(hits)
    obj, side, nrm = hits["object"], hits["flags"] & 3, hits["normal"]
    col = np.ascontiguousarray(hits["color"]).view(np.uint32)
    walked = ~dead & (length > F(1.0))
    cnt = np.zeros((Wn, H), dtype=F)
    s1, s2 = np.zeros(c.shape, dtype=F), np.zeros(c.shape, dtype=F)
    mn, mx = c.copy(), c.copy()
    r = int(radius)
    with np.errstate(all="ignore"):
        for a in range(-r, r + 1):
            wx = _window(Wn, a)
            if wx is None:
                continue
            for b in range(-r, r + 1):
                wz = _window(H, b)
                if wz is None:
                    continue
                P, Q = (wx[0], wz[0]), (wx[1], wz[1])
                if a == 0 and b == 0:
                    counts = np.ones(cnt[P].shape, dtype=bool)
                else:
                    same = (obj[Q] == obj[P]) & (side[Q] == side[P])
                    if match_color:
                        same &= (col[Q] == col[P]).all(axis=-1)
                    n_p, n_q = nrm[P], nrm[Q]
                    t = (n_p[..., 0] * n_q[..., 0] + n_p[..., 1] * n_q[..., 1]) + n_p[..., 2] * n_q[..., 2]
                    counts = ~dead[Q] & same & (t >= F(normal_cos))
                cq, k = c[Q], counts[..., None]
                cnt[P] = np.where(counts, cnt[P] + F(1.0), cnt[P])
                s1[P] = np.where(k, s1[P] + cq, s1[P])
                s2[P] = np.where(k, s2[P] + cq * cq, s2[P])
                mn[P] = np.where(k & (cq < mn[P]), cq, mn[P])
                mx[P] = np.where(k & (cq > mx[P]), cq, mx[P])
        few = walked & (cnt < F(min_taps))
        if box == 0:
            lo, hi = mn, mx
        else:
            mean, e2 = s1 / cnt[..., None], s2 / cnt[..., None]
            var = e2 - mean * mean
            var = np.where(var > 0, var, F(0))
            w = F(gamma) * np.sqrt(var)
            lo, hi = mean - w, mean + w
        below = v < lo
        t = np.where(below, lo, v)
        above = t > hi
        t = np.where(above, hi, t)
        clipped = walked & ~few & (below | above).any(axis=-1)
        m1, m2 = moments[..., 0], moments[..., 1]
        m1c = m1 + (lum(t) - lum(v))
        m2c = m2 + (m1c * m1c - m1 * m1)
        out_value = np.where(clipped[..., None], t, v).astype(F)
        out_len = np.where(clipped & ~(length <= F(clip_history)), F(clip_history), length).astype(F)
        m1o, m2o = np.where(clipped, m1c, m1), np.where(clipped, m2c, m2)
        tt = m2o - m1o * m1o
        variance = np.where(tt > 0, tt, F(0)).astype(F)
    flags = np.where(clipped, 1, np.where(few, 2, 0)).astype(np.uint8)
    out = (np.ascontiguousarray(out_value.reshape(cur.shape)), np.ascontiguousarray(np.stack([m1o, m2o], axis=-1), dtype=F),
           np.ascontiguousarray(out_len), np.ascontiguousarray(variance), flags)
    return out + (dict(walked=walked, taps=cnt),) if details else out
