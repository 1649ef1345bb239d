"""The reference of include/rt_capi_upsample.h, for the tests: the header's definition restated in numpy float32, vectorised per
tap -- for each of the four cells (a, b), in the header's order, every pixel's tap at once, one rounding per operation (numpy's
float32 ufuncs do not contract and divide correctly rounded).  Comparisons are written as the header writes them, so that a NaN
gives "skip": where(t > 0, t, 0), never maximum."""
import numpy as np

F = np.float32
RT_HIT_LIGHT = 2


def cells_of(n, s):
    return -(-n // s)


def dead_records(hits):
    return (hits["object"] < 0) | ((hits["flags"] & RT_HIT_LIGHT) != 0)


def subsample(hits, s, white=False):
    """rt_subsample_hits: HIT_DTYPE (Wn, H) -> (Wl, Hl)"""
    out = np.array(hits[::s, ::s], order="C")
    if white:
        out["color"][~dead_records(out)] = F(1.0)
    return out


def upsample(hits, lo, s, normal_squarings=3, match_color=False, modulate=False, sigma_plane=0.0, dead_value=0.0, base=None,
             details=False):
    """rt_upsample_guided of HIT_DTYPE (Wn, H) records and float32 (Wl, Hl[, 3]) values -> (out float32 (Wn, H[, 3]), flags bool
    (Wn, H)); with details also a dict of bool (Wn, H) masks: for each clause, the pixels one of whose existing taps of nonzero
    tent it rejected (a tap is counted for the first clause that rejects it, in the header's order)"""
    Wn, H = hits.shape
    Wl, Hl = cells_of(Wn, s), cells_of(H, s)
    lo = np.asarray(lo, dtype=F)
    one = lo.ndim == 2
    lo3 = lo.reshape(Wl, Hl, -1)
    C = lo3.shape[2]
    assert lo3.shape[:2] == (Wl, Hl) and C in (1, 3) and 2 <= s <= 8 and not (modulate and C != 3)
    x, z = np.meshgrid(np.arange(Wn), np.arange(H), indexing="ij")
    i0, j0 = x // s, z // s
    fx, fz = x - i0 * s, z - j0 * s
    obj, flg, nrm, pnt = hits["object"], hits["flags"], hits["normal"], hits["point"]
    col = np.ascontiguousarray(hits["color"]).view(np.uint32)
    dead = dead_records(hits)
    own = (fx == 0) & (fz == 0)
    acc, allc = np.zeros((Wn, H, C), dtype=F), np.zeros((Wn, H, C), dtype=F)
    wsum, tsum = np.zeros((Wn, H), dtype=F), np.zeros((Wn, H), dtype=F)
    rejected = {k: np.zeros((Wn, H), dtype=bool) for k in ("object", "side", "color", "normal", "plane")}
    plane = F(sigma_plane) > F(0)
    with np.errstate(all="ignore"):
        if plane:
            inv = F(1.0) / (F(sigma_plane) * F(sigma_plane))
        for a in (0, 1):
            for b in (0, 1):
                i, j = i0 + a, j0 + b
                ti = (fx if a else s - fx) * (fz if b else s - fz)
                exists = (i < Wl) & (j < Hl) & (ti != 0)
                ic, jc = np.minimum(i, Wl - 1), np.minimum(j, Hl - 1)       # (a cell that does not exist is never taken)
                tent = ti.astype(F)
                g = (ic * s, jc * s)
                lv = lo3[ic, jc]
                allc = np.where(exists[..., None], allc + tent[..., None] * lv, allc)
                tsum = np.where(exists, tsum + tent, tsum)
                same_obj = obj[g] == obj
                same_side = (flg[g] & 3) == (flg & 3)
                same_col = (col[g] == col).all(axis=-1) if match_color else np.ones((Wn, H), dtype=bool)
                n_q = nrm[g]
                t = (nrm[..., 0] * n_q[..., 0] + nrm[..., 1] * n_q[..., 1]) + nrm[..., 2] * n_q[..., 2]
                wn = np.where(t > 0, t, F(0))
                for _ in range(normal_squarings):
                    wn = wn * wn
                w = tent * wn
                after_normal = w > 0
                if plane:
                    e = pnt[g] - pnt
                    d = (e[..., 0] * nrm[..., 0] + e[..., 1] * nrm[..., 1]) + e[..., 2] * nrm[..., 2]
                    u = F(1.0) - (d * d) * inv
                    w = w * np.where(u > 0, u, F(0))
                take = exists & same_obj & same_side & same_col & (w > 0)          # (NaN > 0 is False)
                acc = np.where(take[..., None], acc + w[..., None] * lv, acc)
                wsum = np.where(take, wsum + w, wsum)
                live_tap = exists & ~dead & ~own
                rejected["object"] |= live_tap & ~same_obj
                rejected["side"] |= live_tap & same_obj & ~same_side
                rejected["color"] |= live_tap & same_obj & same_side & ~same_col
                rejected["normal"] |= live_tap & same_obj & same_side & same_col & ~after_normal
                rejected["plane"] |= live_tap & same_obj & same_side & same_col & after_normal & ~(w > 0)
        some = wsum > 0
        v = np.where(some[..., None], acc / wsum[..., None], allc / tsum[..., None])
        v = np.where(own[..., None], lo3[i0, j0], v)
        if modulate:
            v = v * hits["color"]
        v = np.where(dead[..., None], F(dead_value), v).astype(F)
        flags = ~some & ~own & ~dead
        out = v if base is None else np.asarray(base, dtype=F).reshape(Wn, H, C) + v
    out = np.ascontiguousarray(out.reshape(Wn, H) if one else out, dtype=F)
    return (out, flags, rejected) if details else (out, flags)


def same_bits(got, want):
    """bit-equal, except that a NaN of the reference is matched by any NaN"""
    got, want = np.asarray(got, dtype=F), np.asarray(want, dtype=F)
    return got.shape == want.shape and bool(((got.view(np.uint32) == want.view(np.uint32)) | (np.isnan(got) & np.isnan(want))).all())


def distinct_colours(frame):
    a = np.ascontiguousarray(frame, dtype=F)
    return len(np.unique(a.view(np.uint32).reshape(-1, a.shape[-1] if a.ndim == 3 else 1), axis=0))
