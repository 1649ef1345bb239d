"""The reference of include/rt_capi_denoise.h, for the tests: the header's definition restated in numpy float32, vectorised per
tap -- for each of the 25 offsets (a, b), in the header's order, every pixel's tap at once, one rounding per operation (numpy's
float32 ufuncs do not contract and divide correctly rounded).  Comparisons are written as the header writes them, so that a NaN
gives "skip": where(t > 0, t, 0), never maximum."""
import numpy as np

F = np.float32
RT_HIT_LIGHT = 2
B3 = [F(1.0 / 16.0), F(0.25), F(0.375), F(0.25), F(1.0 / 16.0)]


def lum(c):
    return (F(0.25) * c[..., 0] + F(0.5) * c[..., 1]) + F(0.25) * c[..., 2]


def _window(n, off):
    """the slices of p and of q = p + off along an axis of n pixels, where both exist (None: nowhere)"""
    lo, hi = max(0, -off), n - max(0, off)
    if lo >= hi:
        return None
    return slice(lo, hi), slice(lo + off, hi + off)


def iterate(inp, hits, i, sigma_color, normal_squarings):
    """iteration i (step 1 << i) of the definition over float32 (Wn, H, 3) colours `inp`"""
    Wn, H = inp.shape[:2]
    s = 1 << i
    obj = hits["object"]
    col = np.ascontiguousarray(hits["color"]).view(np.uint32)
    nrm = hits["normal"]
    passthrough = (obj < 0) | ((hits["flags"] & RT_HIT_LIGHT) != 0)
    use_colour = F(sigma_color) > F(0)
    acc = np.zeros((Wn, H, 3), dtype=F)
    wsum = np.zeros((Wn, H), dtype=F)
    with np.errstate(all="ignore"):
        if use_colour:
            sc = F(sigma_color) * F(2.0 ** -i)
            inv = F(1.0) / (sc * sc)
            L = lum(inp)
        for a in range(-2, 3):
            wx = _window(Wn, a * s)
            if wx is None:
                continue
            for b in range(-2, 3):
                wz = _window(H, b * s)
                if wz is None:
                    continue
                P, Q = (wx[0], wz[0]), (wx[1], wz[1])
                same = (obj[Q] == obj[P]) & (col[Q] == col[P]).all(axis=-1)
                n_p, n_q = nrm[P], nrm[Q]
                t = (n_p[..., 0] * n_q[..., 0] + n_p[..., 1] * n_q[..., 1]) + n_p[..., 2] * n_q[..., 2]
                wn = np.where(t > 0, t, F(0))
                for _ in range(normal_squarings):
                    wn = wn * wn
                w = (B3[a + 2] * B3[b + 2]) * wn
                if use_colour:
                    d = L[Q] - L[P]
                    u = F(1.0) - (d * d) * inv
                    w = w * np.where(u > 0, u, F(0))
                take = same & (w > 0)                     # (NaN > 0 is False)
                acc[P] = np.where(take[..., None], acc[P] + w[..., None] * inp[Q], acc[P])
                wsum[P] = np.where(take, wsum[P] + w, wsum[P])
        some = (wsum > 0) & ~passthrough
        out = np.where(some[..., None], acc / wsum[..., None], inp)
    return out.astype(F, copy=False)


def denoise(rgb, hits, iterations=2, sigma_color=1.0, normal_squarings=3):
    """rt_denoise of float32 (Wn, H, 3) colours and HIT_DTYPE (Wn, H) records -> float32 (Wn, H, 3)"""
    cur = np.ascontiguousarray(rgb, dtype=F)
    assert cur.ndim == 3 and cur.shape[2] == 3 and hits.shape == cur.shape[:2]
    assert 1 <= iterations <= 5 and 0 <= normal_squarings <= 6
    for i in range(iterations):
        cur = iterate(cur, hits, i, sigma_color, normal_squarings)
    return cur


def same_bits(got, want):
    """bit-equal, except that a NaN of the reference is matched by any NaN"""
    got, want = np.asarray(got, dtype=F), np.asarray(want, dtype=F)
    return got.shape == want.shape and bool(((got.view(np.uint32) == want.view(np.uint32)) | (np.isnan(got) & np.isnan(want))).all())


def psnr(a, b, peak=1.0):
    """10 log10(peak^2 / mean squared error) over all pixels and channels, in float64"""
    d = a.astype(np.float64) - b.astype(np.float64)
    return 10.0 * np.log10(peak * peak / np.mean(d * d))
