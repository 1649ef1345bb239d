"""The reference of include/rt_temporal.h, for the tests: the header's definition restated in numpy float32, vectorised per
tap -- for each of the four cells (a, b), in the header's order, every pixel's tap at once, one rounding per operation (numpy's
float32 ufuncs do not contract and divide correctly rounded).  Comparisons are written as the header writes them, so that a NaN
gives "no history" or "skip": where(t > 0, t, 0), never maximum."""
import ctypes as C

import numpy as np

F = np.float32
RT_HIT_LIGHT = 2


def dead_records(hits):
    return (hits["object"] < 0) | ((hits["flags"] & RT_HIT_LIGHT) != 0)


def camera_words(cam):
    """the 16 floats of an RtCameraDesc, in its order"""
    return np.frombuffer(bytes(C.string_at(C.addressof(cam), 64)), dtype=F).copy()


def dot(a, b):
    t = a[..., 0] * b[..., 0]
    u = a[..., 1] * b[..., 1]
    t = t + u
    u = a[..., 2] * b[..., 2]
    return t + u


def cross(a, b):
    out = np.empty(np.broadcast(a, b).shape, dtype=F)
    t = a[..., 1] * b[..., 2]
    u = a[..., 2] * b[..., 1]
    out[..., 0] = t - u
    t = a[..., 2] * b[..., 0]
    u = a[..., 0] * b[..., 2]
    out[..., 1] = t - u
    t = a[..., 0] * b[..., 1]
    u = a[..., 1] * b[..., 0]
    out[..., 2] = t - u
    return out


def lum(c):
    if c.ndim == 2:
        return c
    t = F(0.25) * c[..., 0]
    u = F(0.5) * c[..., 1]
    t = t + u
    u = F(0.25) * c[..., 2]
    return t + u


def project(cam_prev, point, W, H):
    """header step 3 -> (seen bool, px, pz float32) of every point"""
    w = camera_words(cam_prev)
    sw, sh, shw, shh = w[0], w[1], w[2], w[3]
    so, hv, vv, eye = w[4:7], w[7:10], w[10:13], w[13:16]
    O = so - eye
    nh = cross(hv, vv)
    na = cross(vv, O)
    nb = cross(O, hv)
    q = dot(O, nh)
    D = point - eye
    s = dot(D, nh)
    a = dot(D, na) / s
    b = dot(D, nb) / s
    px = a + shw
    px = px / sw
    px = px * F(W)
    pz = b + shh
    pz = pz / sh
    pz = pz * F(H)
    sq = s * q
    seen = (sq > 0) & (px > -1) & (px < F(W)) & (pz > -1) & (pz < F(H))
    return seen, px, pz


def tap_columns(cam_prev, hits, W, H, points=None):
    """the columns [lo, hi) of the previous W x H frame that hold every cell a reprojected tap of the live records `hits` can
    fall on (what accumulate's prev_x0 window must hold); points: where the records' points were (motion_ref.moved), if not their
    own.  None if no record is seen."""
    with np.errstate(all="ignore"):
        seen, px, _ = project(cam_prev, hits["point"] if points is None else points, W, H)
        seen = seen & ~dead_records(hits)
        if not seen.any():
            return None
        i0 = np.floor(px[seen]).astype(np.int64)
    return max(int(i0.min()), 0), min(int(i0.max()) + 2, W)


def accumulate(cur, hits, cam, prev=None, x0=0, W=None, match_color=False, max_history=32, normal_cos=0.9, plane_eps=0.05,
               alpha=0.0, alpha_moments=0.0, details=False, prev_x0=0):
    """rt_temporal_accumulate: cur float32 (Wn, H[, 3]), hits HIT_DTYPE (Wn, H), prev None or (camera, hits, value, moments,
    length) of the whole W x H previous frame -> (value, moments (Wn, H, 2), length, variance, flags bool); with details also a
    dict: "outside" bool (Wn, H), live pixels that project outside the previous frame (or behind its eye), and "passing" int
    (Wn, H), for the other live pixels how many of their cells inside the frame passed the tap tests (before the bw > 0 test).
    With prev_x0 (and W) the previous frame's four arrays hold only its columns [prev_x0, prev_x0 + n): a frame too large to have on
    the host.  A tap on a cell of the frame outside those columns raises IndexError; it never counts as a rejected tap."""
    cur = np.asarray(cur, dtype=F)
    Wn, H = hits.shape
    one = cur.ndim == 2
    c = cur.reshape(Wn, H, -1)
    Cn = c.shape[2]
    assert Cn in (1, 3) and c.shape[:2] == (Wn, H)
    with np.errstate(all="ignore"):
        l = lum(cur)
        ll = l * l
        acc = np.zeros((Wn, H, Cn + 3), dtype=F)
        wsum = np.zeros((Wn, H), dtype=F)
        info = dict(outside=np.zeros((Wn, H), dtype=bool), passing=np.zeros((Wn, H), dtype=np.int64))
        if prev is not None:
            cam_prev, g_all, p_value, p_moments, p_len = prev
            W = g_all.shape[0] if W is None else W
            n_prev = g_all.shape[0]                              # the previous frame's columns [prev_x0, prev_x0 + n_prev) are here
            assert g_all.shape == (n_prev, H) and 0 <= prev_x0 and prev_x0 + n_prev <= W
            words = np.concatenate([np.asarray(p_value, dtype=F).reshape(n_prev, H, Cn),
                                    np.asarray(p_moments, dtype=F).reshape(n_prev, H, 2),
                                    np.asarray(p_len, dtype=F).reshape(n_prev, H, 1)], axis=-1)
            live = ~dead_records(hits)
            nrm, pnt = hits["normal"], hits["point"]
            col = np.ascontiguousarray(hits["color"]).view(np.uint32)
            g_col = np.ascontiguousarray(g_all["color"]).view(np.uint32)
            identity = camera_words(cam_prev).tobytes() == camera_words(cam).tobytes()
            if identity:
                x, z = np.meshgrid(np.arange(x0, x0 + Wn), np.arange(H), indexing="ij")
                seen, i0, j0 = live, x, z
                fx = fz = np.zeros((Wn, H), dtype=F)
            else:
                seen, px, pz = project(cam_prev, pnt, W, H)
                info["outside"] = live & ~seen
                seen = seen & live
                flx, flz = np.floor(px), np.floor(pz)
                i0 = np.where(seen, flx, 0).astype(np.int64)
                j0 = np.where(seen, flz, 0).astype(np.int64)
                fx = px - flx
                fz = pz - flz
            eps2 = F(plane_eps) * F(plane_eps)
            for a in (0, 1):
                for b in (0, 1):
                    if identity and (a or b):
                        continue
                    i, j = i0 + a, j0 + b
                    wx = fx if a else F(1.0) - fx
                    wz = fz if b else F(1.0) - fz
                    bw = np.ones((Wn, H), dtype=F) if identity else wx * wz
                    inside = seen & (i >= 0) & (i < W) & (j >= 0) & (j < H)
                    held = (i >= prev_x0) & (i < prev_x0 + n_prev)
                    if (inside & ~held).any():
                        raise IndexError(f"{int((inside & ~held).sum())} taps fall on columns {int(i[inside & ~held].min())}.."
                                         f"{int(i[inside & ~held].max())} of the previous frame, of which only "
                                         f"{prev_x0}:{prev_x0 + n_prev} are given")
                    cell = (np.clip(i - prev_x0, 0, n_prev - 1), np.clip(j, 0, H - 1))   # (a cell that does not exist is never taken)
                    g = g_all[cell]
                    take = (g["object"] == hits["object"]) & ((g["flags"] & 3) == (hits["flags"] & 3))
                    if match_color:
                        take &= (g_col[cell] == col).all(axis=-1)
                    t = dot(nrm, g["normal"])
                    take &= t >= F(normal_cos)
                    if F(plane_eps) > 0:
                        e = g["point"] - pnt
                        d = dot(e, nrm)
                        dd = d * d
                        take &= dd <= eps2
                    take &= inside
                    info["passing"] += take
                    take &= bw > 0
                    term = bw[..., None] * words[cell]
                    acc = np.where(take[..., None], acc + term, acc)
                    wsum = np.where(take, wsum + bw, wsum)
        history = wsum > 0
        hk = acc / wsum[..., None]
        N = hk[..., Cn + 2] + F(1.0)
        N = np.where(N <= F(max_history), N, F(max_history))
        ac = F(1.0) / N
        am = ac
        ac = np.where(ac >= F(alpha), ac, F(alpha))
        am = np.where(am >= F(alpha_moments), am, F(alpha_moments))
        hc = hk[..., :Cn]
        t = c - hc
        t = ac[..., None] * t
        value = hc + t
        hm1, hm2 = hk[..., Cn], hk[..., Cn + 1]
        t = l - hm1
        t = am * t
        m1 = hm1 + t
        t = ll - hm2
        t = am * t
        m2 = hm2 + t
        t = m1 * m1
        v = m2 - t
        variance = np.where(v > 0, v, F(0))
        value = np.where(history[..., None], value, c)
        moments = np.stack([np.where(history, m1, l), np.where(history, m2, ll)], axis=-1)
        length = np.where(history, N, F(1.0))
        variance = np.where(history, variance, F(0))
    out = (np.ascontiguousarray(value.reshape(Wn, H) if one else value, dtype=F), np.ascontiguousarray(moments, dtype=F),
           np.ascontiguousarray(length, dtype=F), np.ascontiguousarray(variance, dtype=F), ~history)
    return out + (info,) if details else out
