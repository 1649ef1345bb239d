"""The reference of include/rt_gradient.h, for the tests: the header's definition restated in numpy float32, vectorised per cell
offset -- for each offset (a, b) of the window, in the header's order, every pixel's cell at once, one rounding per operation
(numpy's float32 ufuncs do not contract, and divide correctly rounded).  Comparisons are written as the header writes them, so
that a NaN gives "skip" or "leave": where(t > 0, t, 0), never maximum."""
import numpy as np

from svgf_ref import dead_records, lum

F = np.float32
NAMES = ("value", "moments", "length", "variance", "lambda", "flags")
DEFAULTS = dict(scale=2, radius=1, match_color=True, normal_cos=0.9, gain=2.0, lambda_min=0.0, den_floor=1e-6)


def cell_shape(Wn, H, scale):
    return -(-Wn // scale), -(-H // scale)


def cells(now_lo, then_lo, lo_hits, then_hits=None):
    """the header's per-cell lines -> (d, m) float32 (Wl, Hl)"""
    Wl, Hl = lo_hits.shape
    with np.errstate(all="ignore"):
        ln = lum(np.ascontiguousarray(now_lo, dtype=F).reshape(Wl, Hl, -1))
        lt = lum(np.ascontiguousarray(then_lo, dtype=F).reshape(Wl, Hl, -1))
        d = ln - lt
        d = np.where(d < 0, -d, d)
        m = np.where(lt > ln, lt, ln)
        if then_hits is not None:
            changed = (then_hits["object"] != lo_hits["object"]) | ((then_hits["flags"] & 3) != (lo_hits["flags"] & 3))
            d = np.where(changed, m, d)
    return d.astype(F), m.astype(F)


def reweight(cur, hits, value, moments, length, now_lo, then_lo, lo_hits, then_hits=None, scale=2, radius=1, match_color=True,
             normal_cos=0.9, gain=2.0, lambda_min=0.0, den_floor=1e-6, details=False):
    """rt_gradient_reweight: cur and value float32 (Wn, H[, 3]), hits HIT_DTYPE (Wn, H), moments (Wn, H, 2), length (Wn, H),
    now_lo and then_lo (Wl, Hl[, 3]), lo_hits and then_hits (or None) HIT_DTYPE (Wl, Hl) -> (value, moments, length, variance,
    lambda, flags uint8); with details also a dict: "walked", bool (Wn, H), the live pixels with a history longer than one, and
    "cells", int (Wn, H), the cells the window counted"""
    cur, value = np.ascontiguousarray(cur, dtype=F), np.ascontiguousarray(value, dtype=F)
    moments, length = np.ascontiguousarray(moments, dtype=F), np.ascontiguousarray(length, dtype=F)
    Wn, H = hits.shape
    s, r = int(scale), int(radius)
    c, v = cur.reshape(Wn, H, -1), value.reshape(Wn, H, -1)
    assert c.shape[2] in (1, 3) and v.shape == c.shape and moments.shape == (Wn, H, 2) and length.shape == (Wn, H)
    assert 2 <= s <= 8 and 0 <= r <= 2
    Wl, Hl = cell_shape(Wn, H, s)
    assert lo_hits.shape == (Wl, Hl) and (then_hits is None or then_hits.shape == (Wl, Hl))
    d, m = cells(now_lo, then_lo, lo_hits, then_hits)
    dead_q = dead_records(lo_hits)
    col_p = np.ascontiguousarray(hits["color"]).view(np.uint32)
    col_q = np.ascontiguousarray(lo_hits["color"]).view(np.uint32)
    walked = ~dead_records(hits) & (length > F(1.0))
    i0, j0 = np.arange(Wn) // s, np.arange(H) // s
    cnt = np.zeros((Wn, H), dtype=np.int64)
    num, den = np.zeros((Wn, H), dtype=F), np.zeros((Wn, H), dtype=F)
    one, zero = F(1.0), F(0.0)
    with np.errstate(all="ignore"):
        for a in range(-r, r + 2):
            for b in range(-r, r + 2):
                i, j = i0 + a, j0 + b
                exists = ((i >= 0) & (i < Wl))[:, None] & ((j >= 0) & (j < Hl))[None, :]
                Q = (np.clip(i, 0, Wl - 1)[:, None], np.clip(j, 0, Hl - 1)[None, :])
                g = lo_hits[Q]
                same = (g["object"] == hits["object"]) & ((g["flags"] & 3) == (hits["flags"] & 3))
                if match_color:
                    same &= (col_q[Q] == col_p).all(axis=-1)
                n_p, n_q = hits["normal"], g["normal"]
                t = (n_p[..., 0] * n_q[..., 0] + n_p[..., 1] * n_q[..., 1]) + n_p[..., 2] * n_q[..., 2]
                counts = exists & ~dead_q[Q] & same & (t >= F(normal_cos))
                cnt = np.where(counts, cnt + 1, cnt)
                num = np.where(counts, num + d[Q], num)
                den = np.where(counts, den + m[Q], den)
        none = walked & (cnt == 0)
        t = np.where(den > F(den_floor), num / den, zero).astype(F)
        lam = F(gain) * t
        lam = np.where(lam > one, one, lam).astype(F)
        weighed = walked & ~none
        lam_out = np.where(weighed & (lam > 0), lam, zero).astype(F)
        touched = weighed & (lam > F(lambda_min))
        restart = touched & (lam == one)
        reblend = touched & ~restart
        l = lum(c)
        ll = l * l
        m1, m2 = moments[..., 0], moments[..., 1]
        vb = v + lam[..., None] * (c - v)
        m1b = m1 + lam * (l - m1)
        m2b = m2 + lam * (ll - m2)
        al = one / length
        a2 = al + lam * (one - al)
        Lb = one / a2
        Lb = np.where(Lb >= one, Lb, one)
        Lb = np.where(Lb <= length, Lb, length)
        out_value = np.where(restart[..., None], c, np.where(reblend[..., None], vb, v)).astype(F)
        m1o = np.where(restart, l, np.where(reblend, m1b, m1)).astype(F)
        m2o = np.where(restart, ll, np.where(reblend, m2b, m2)).astype(F)
        out_len = np.where(restart, one, np.where(reblend, Lb, length)).astype(F)
        tt = m2o - m1o * m1o
        variance = np.where(tt > 0, tt, zero).astype(F)
    flags = np.where(restart, 3, np.where(reblend, 1, np.where(none, 2, 0))).astype(np.uint8)
    out = (np.ascontiguousarray(out_value.reshape(cur.shape)), np.ascontiguousarray(np.stack([m1o, m2o], axis=-1), dtype=F),
           np.ascontiguousarray(out_len), np.ascontiguousarray(variance), np.ascontiguousarray(lam_out), flags)
    return out + (dict(walked=walked, cells=cnt),) if details else out
