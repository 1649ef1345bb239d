"""The reference of include/rt_motion.h, for the tests: the header's definition restated in numpy float32 in the manner of
temporal_ref.py, whose helpers it uses -- for each of the four cells (a, b), in the header's order, every pixel's tap at once,
one rounding per operation.  Where rt_motion.h changes rt_temporal.h's definition -- static or moving, where the point and the
normal were, who takes the identity tap -- this file says so; everything else is temporal_ref.accumulate's, line for line."""
import numpy as np

import temporal_ref
from temporal_ref import F, camera_words, dead_records, dot, lum, project

IDENTITY = np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0], dtype=F)


def table_of(motions):
    """None or (n, 12) -> float32 (n, 12)"""
    return np.zeros((0, 12), dtype=F) if motions is None else np.ascontiguousarray(motions, dtype=F).reshape(-1, 12)


def moving_records(hits, motions):
    """STATIC OR MOVING -> bool, hits' shape: the live records whose object has an entry that differs, as bits, from IDENTITY"""
    table = table_of(motions)
    obj = hits["object"]
    has = ~dead_records(hits) & (obj < table.shape[0])
    differs = (table.view(np.uint32) != IDENTITY.view(np.uint32)).any(axis=1)
    return has & np.concatenate([differs, [False]])[np.where(has, obj, table.shape[0])]


def moved(hits, motions, moving):
    """WHERE THE POINT AND NORMAL WERE -> (Pp, Np) float32 hits.shape + (3,): the record's words for a static record"""
    table = table_of(motions)
    P, N = hits["point"], hits["normal"]
    if not moving.any():
        return P, N
    m = np.concatenate([table, IDENTITY[None]])[np.where(moving, hits["object"], table.shape[0])]      # hits.shape + (12,)
    Pp, Np = np.empty(P.shape, dtype=F), np.empty(N.shape, dtype=F)
    for k in range(3):
        t = m[..., 4 * k] * P[..., 0]
        u = m[..., 4 * k + 1] * P[..., 1]
        t = t + u
        u = m[..., 4 * k + 2] * P[..., 2]
        t = t + u
        Pp[..., k] = t + m[..., 4 * k + 3]
        t = m[..., 4 * k] * N[..., 0]
        u = m[..., 4 * k + 1] * N[..., 1]
        t = t + u
        u = m[..., 4 * k + 2] * N[..., 2]
        Np[..., k] = t + u
    return np.where(moving[..., None], Pp, P), np.where(moving[..., None], Np, N)


def accumulate(cur, hits, cam, prev=None, motions=None, x0=0, W=None, match_color=False, max_history=32, normal_cos=0.9,
               plane_eps=0.05, alpha=0.0, alpha_moments=0.0, details=False, prev_x0=0):
    """rt_motion_accumulate: temporal_ref.accumulate's arguments and result, with motions None or float32 (n, 12); with details
    also a dict: "moving" bool (Wn, H), "outside" bool (Wn, H), live pixels that are reprojected and land outside the previous
    frame (or behind its eye), "identity" bool (Wn, H), the live pixels that take the identity tap, and "passing" int (Wn, H), for
    the other live pixels how many of their cells inside the frame passed the tap tests (before the bw > 0 test).  prev_x0:
    temporal_ref.accumulate's -- the previous frame's arrays hold its columns [prev_x0, prev_x0 + n) only, and a tap outside them
    raises IndexError."""
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
        none = np.zeros((Wn, H), dtype=bool)
        info = dict(moving=none, outside=none, identity=none, passing=np.zeros((Wn, H), dtype=np.int64))
        if prev is not None:
            cam_prev, g_all, p_value, p_moments, p_len = prev
            W = g_all.shape[0] if W is None else W
            n_prev = g_all.shape[0]                              # the previous frame's columns [prev_x0, prev_x0 + n_prev) are here
            assert g_all.shape == (n_prev, H) and 0 <= prev_x0 and prev_x0 + n_prev <= W
            words = np.concatenate([np.asarray(p_value, dtype=F).reshape(n_prev, H, Cn),
                                    np.asarray(p_moments, dtype=F).reshape(n_prev, H, 2),
                                    np.asarray(p_len, dtype=F).reshape(n_prev, H, 1)], axis=-1)
            live = ~dead_records(hits)
            moving = moving_records(hits, motions)
            pnt, nrm = moved(hits, motions, moving)              # Pp and Np: the tap tests and the reprojection read these
            col = np.ascontiguousarray(hits["color"]).view(np.uint32)
            g_col = np.ascontiguousarray(g_all["color"]).view(np.uint32)
            equal = camera_words(cam_prev).tobytes() == camera_words(cam).tobytes()
            identity = ~moving if equal else none                # step 2: equal cameras AND a static record
            x, z = np.meshgrid(np.arange(x0, x0 + Wn), np.arange(H), indexing="ij")
            seen, px, pz = project(cam_prev, pnt, W, H)          # step 3, D = Pp - eye
            seen = np.where(identity, True, seen)
            info.update(moving=moving, outside=live & ~seen, identity=live & identity)
            seen = seen & live
            flx, flz = np.floor(px), np.floor(pz)
            i0 = np.where(identity, x, np.where(seen, flx, 0).astype(np.int64))
            j0 = np.where(identity, z, np.where(seen, flz, 0).astype(np.int64))
            fx = px - flx
            fz = pz - flz
            eps2 = F(plane_eps) * F(plane_eps)
            for a in (0, 1):
                for b in (0, 1):
                    i, j = i0 + a, j0 + b
                    wx = fx if a else F(1.0) - fx
                    wz = fz if b else F(1.0) - fz
                    bw = np.where(identity, F(1.0), wx * wz).astype(F)
                    inside = seen & (i >= 0) & (i < W) & (j >= 0) & (j < H)
                    if a or b:
                        inside = inside & ~identity              # the identity's only tap is its own cell
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
                    info["passing"] += take & ~identity
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


assert temporal_ref.RT_HIT_LIGHT == 2
