"""The reference of include/rt_svgf.h, for the tests: the header's definition restated in numpy float32, vectorised per tap -- for
each offset (a, b) of a window, in the header's order, every pixel's tap at once, one rounding per operation (numpy's float32
ufuncs do not contract and divide correctly rounded).  Comparisons are written as the header writes them, so that a NaN gives
"skip": where(t > 0, t, 0), never maximum."""
import numpy as np

from denoise_ref import B3, _window, same_bits  # noqa: F401

F = np.float32
RT_HIT_LIGHT = 2
G3 = [F(0.25), F(0.5), F(0.25)]


def dead_records(hits):
    return (hits["object"] < 0) | ((hits["flags"] & RT_HIT_LIGHT) != 0)


def lum(c):
    """c: (..., channels)"""
    if c.shape[-1] == 1:
        return c[..., 0]
    return (F(0.25) * c[..., 0] + F(0.5) * c[..., 1]) + F(0.25) * c[..., 2]


class _Guide:
    """the records' fields the definition reads, and key(p, q) and geo(p, q) over windows P, Q"""

    def __init__(self, hits, normal_squarings, match_color, sigma_plane):
        self.obj, self.side = hits["object"], hits["flags"] & 3
        self.col = np.ascontiguousarray(hits["color"]).view(np.uint32)
        self.nrm, self.pnt = hits["normal"], hits["point"]
        self.squarings, self.match_color = int(normal_squarings), bool(match_color)
        self.plane = F(sigma_plane) > F(0)
        if self.plane:
            self.invp = F(1.0) / (F(sigma_plane) * F(sigma_plane))

    def key(self, P, Q):
        same = (self.obj[Q] == self.obj[P]) & (self.side[Q] == self.side[P])
        if self.match_color:
            same &= (self.col[Q] == self.col[P]).all(axis=-1)
        return same

    def geo(self, P, Q):
        n_p, n_q = self.nrm[P], self.nrm[Q]
        t = (n_p[..., 0] * n_q[..., 0] + n_p[..., 1] * n_q[..., 1]) + n_p[..., 2] * n_q[..., 2]
        wn = np.where(t > 0, t, F(0))
        for _ in range(self.squarings):
            wn = wn * wn
        if self.plane:
            e = self.pnt[Q] - self.pnt[P]
            d = (e[..., 0] * n_p[..., 0] + e[..., 1] * n_p[..., 1]) + e[..., 2] * n_p[..., 2]
            u = F(1.0) - (d * d) * self.invp
            wn = wn * np.where(u > 0, u, F(0))
        return wn


def _windows(Wn, H, offsets_x, offsets_z):
    """(a, b, P, Q) of every offset pair, in the header's order, where a tap exists"""
    for a, ox in offsets_x:
        wx = _window(Wn, ox)
        if wx is None:
            continue
        for b, oz in offsets_z:
            wz = _window(H, oz)
            if wz is None:
                continue
            yield a, b, (wx[0], wz[0]), (wx[1], wz[1])


def estimate(guide, hits, moments, length, min_history, spatial_radius, info=None):
    """header step A -> var0 float32 (Wn, H)"""
    Wn, H = hits.shape
    dead = dead_records(hits)
    m1, m2 = np.ascontiguousarray(moments[..., 0]), np.ascontiguousarray(moments[..., 1])
    vt = m2 - m1 * m1
    vt = np.where(vt > 0, vt, F(0))
    short = ~dead & ~(length >= F(min_history))
    a1, a2, ws = (np.zeros((Wn, H), dtype=F) for _ in range(3))
    r = int(spatial_radius)
    offs = [(k, k) for k in range(-r, r + 1)]
    for a, b, P, Q in _windows(Wn, H, offs, offs):
        w = guide.geo(P, Q)
        take = guide.key(P, Q) & (w > 0)
        a1[P] = np.where(take, a1[P] + w * m1[Q], a1[P])
        a2[P] = np.where(take, a2[P] + w * m2[Q], a2[P])
        ws[P] = np.where(take, ws[P] + w, ws[P])
    some = ws > 0
    s1, s2 = a1 / ws, a2 / ws
    vs = s2 - s1 * s1
    vs = np.where(vs > 0, vs, F(0))
    k = F(min_history) / length
    k = np.where(k >= F(1.0), k, F(1.0))
    spatial = np.where(some, vs * k, vt)
    if info is not None:
        info["spatial"] = short
        info["spatial_taps"] = short & some
    return np.where(dead, F(0), np.where(short, spatial, vt)).astype(F)


def iterate(guide, hits, inp, vin, i, sigma_l, epsilon, info=None):
    """iteration i (step 1 << i) of header step B over float32 (Wn, H, channels) values and (Wn, H) variances -> (out, vout)"""
    Wn, H, Cn = inp.shape
    s = 1 << i
    dead = dead_records(hits)
    use_lum = F(sigma_l) > F(0)
    if use_lum:
        gv, gs = np.zeros((Wn, H), dtype=F), np.zeros((Wn, H), dtype=F)
        unit = [(k, k) for k in (-1, 0, 1)]
        for a, b, P, Q in _windows(Wn, H, unit, unit):
            gg = G3[a + 1] * G3[b + 1]
            gv[P] = gv[P] + gg * vin[Q]
            gs[P] = gs[P] + gg
        vf = gv / gs
        invl = F(1.0) / ((F(sigma_l) * F(sigma_l)) * vf + F(epsilon))
        L = lum(inp)
    acc = np.zeros((Wn, H, Cn), dtype=F)
    vacc, wsum = np.zeros((Wn, H), dtype=F), np.zeros((Wn, H), dtype=F)
    offs = [(k, k * s) for k in range(-2, 3)]
    for a, b, P, Q in _windows(Wn, H, offs, offs):
        same = guide.key(P, Q)
        w = (B3[a + 2] * B3[b + 2]) * guide.geo(P, Q)
        if use_lum:
            before = w
            d = L[Q] - L[P]
            u = F(1.0) - (d * d) * invl[P]
            w = w * np.where(u > 0, u, F(0))
        take = same & (w > 0)                                 # (NaN > 0 is False)
        if info is not None:
            live = ~dead[P]
            info["key_rejected"][P] |= live & ~same
            if use_lum:
                info["lum_dropped"][P] |= live & same & (before > 0) & ~(w > 0)
        acc[P] = np.where(take[..., None], acc[P] + w[..., None] * inp[Q], acc[P])
        vacc[P] = np.where(take, vacc[P] + (w * w) * vin[Q], vacc[P])
        wsum[P] = np.where(take, wsum[P] + w, wsum[P])
    some = (wsum > 0) & ~dead
    out = np.where(some[..., None], acc / wsum[..., None], inp)
    vout = np.where(some, vacc / (wsum * wsum), vin)
    return out.astype(F, copy=False), vout.astype(F, copy=False)


def svgf(value, hits, moments, length, iterations=4, sigma_l=2.0, min_history=4, spatial_radius=3, normal_squarings=3,
         match_color=True, sigma_plane=0.0, epsilon=1e-8, details=False):
    """rt_svgf_filter: value float32 (Wn, H[, 3]), hits HIT_DTYPE (Wn, H), moments (Wn, H, 2), length (Wn, H) -> (out_value,
    out_variance, out_estimate); with details also a dict of bool (Wn, H) planes: "spatial", the live pixels whose history is
    shorter than min_history ("spatial_taps": those of them whose window held a tap), "key_rejected", the live pixels one of
    whose taps inside the rectangle, in any iteration, a key rejected, and "lum_dropped", the live pixels for which the luminance
    term dropped a tap that the key admitted and whose geometric weight was positive"""
    value = np.ascontiguousarray(value, dtype=F)
    Wn, H = hits.shape
    one = value.ndim == 2
    cur = value.reshape(Wn, H, -1)
    assert cur.shape[2] in (1, 3) and moments.shape == (Wn, H, 2) and length.shape == (Wn, H)
    assert 1 <= iterations <= 5 and 0 <= normal_squarings <= 6 and 1 <= spatial_radius <= 3 and 1 <= min_history <= 65535
    moments, length = np.asarray(moments, dtype=F), np.asarray(length, dtype=F)
    info = dict(key_rejected=np.zeros((Wn, H), dtype=bool), lum_dropped=np.zeros((Wn, H), dtype=bool)) if details else None
    guide = _Guide(hits, normal_squarings, match_color, sigma_plane)
    with np.errstate(all="ignore"):
        var0 = estimate(guide, hits, moments, length, min_history, spatial_radius, info)
        var = var0
        for i in range(iterations):
            cur, var = iterate(guide, hits, cur, var, i, sigma_l, epsilon, info)
    out = (np.ascontiguousarray(cur.reshape(Wn, H) if one else cur, dtype=F), np.ascontiguousarray(var, dtype=F),
           np.ascontiguousarray(var0, dtype=F))
    return out + (info,) if details else out
