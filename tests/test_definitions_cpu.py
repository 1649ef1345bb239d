"""The headers' definitions against their own geometry, in float64.  refract_ref and soft_ref restate the kernels' fp32 arithmetic
and the kernels match them bit for bit, so an error in a definition itself would be shared by both; these tests check the two
premises the definitions rest on:
  * the glass sphere's transmitted child (include/rt_capi_refract.h) is Snell's refraction in and out of a sphere -- it exists
    exactly when float64 finds neither total internal reflection nor an empty chord, sin t1 = ior sin t2 at the entry, the exit
    point lies on the sphere 1e-3 out along the normal, and the ray leaves at the angle it came in;
  * every area-light sample Q (include/rt_capi_soft.h) lies within r' = soft_reach() of the light's centre on every axis --
    the reach by which every soft-shadow cull and the SHADOW VOXELS grow the light."""
import numpy as np
import pytest

import oracle_lib as oracle
import query_ref
import refract_ref
import soft_ref

F = np.float32
EPS = float(np.finfo(np.float32).eps)


# ---- Snell's geometry of the glass sphere -----------------------------------------------------------------------------------

def outside_hits(rng, c, r, n):
    """n rays from outside towards a sphere (centre c, radius r), a third of them within 1e-3 r of its rim -> (sphere, E, d, t,
    P, N) of the rays that hit it from outside, query_ref's records"""
    o = oracle.OracleScene()
    o.add_sphere(tuple(float(v) for v in c), float(r))
    sphere = o.get_object(0)
    w = rng.normal(size=(n, 3))
    w /= np.linalg.norm(w, axis=1, keepdims=True)
    E = c + w * (r * rng.uniform(1.5, 20.0, (n, 1)))
    u = np.cross(w, rng.normal(size=(n, 3)))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    b = np.where(rng.rand(n) < 1 / 3, 1.0 - rng.uniform(0, 1e-3, n), np.sqrt(rng.uniform(0, 1, n)))
    T = c + u * (r * b)[:, None]
    rays = np.concatenate([E, T], axis=1).astype(F)
    E, d = rays[:, :3], query_ref.directions(rays)
    hit, t, P, N, _, inside = query_ref._collision(sphere, E, d, True)
    keep = hit & ~inside
    return sphere, E[keep], d[keep], t[keep], P[keep], N[keep]


def snell64(c, d, P, ior):
    """float64 from the fp32 hit: (cos t1, sin t1, the refracted sin t2, the chord's length, total internal reflection)"""
    d, P = d.astype(np.float64), P.astype(np.float64)
    n = P - c
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    cos1 = -np.einsum("ij,ij->i", n, d)
    sin1 = np.sqrt(np.maximum(0.0, 1.0 - cos1 * cos1))
    sin2 = sin1 / ior
    tir = sin2 > 1.0
    cos2 = np.sqrt(np.maximum(0.0, 1.0 - sin2 * sin2))
    T1 = d / ior + n[:, :] * (cos1 / ior - cos2)[:, None]
    chord = -2.0 * np.einsum("ij,ij->i", T1, P - c)
    return cos1, sin1, sin2, chord, tir, n


@pytest.mark.parametrize("ior", [0.6, 1.0, 1.33, 1.5, 2.4])
def test_glass_sphere_is_snell_in_float64(ior):
    rng = np.random.RandomState(int(ior * 100))
    worst = {"entry": 0.0, "exit_point": 0.0, "exit_angle": 0.0}
    for trial in range(4):
        c = rng.uniform(-10, 10, 3).astype(F).astype(np.float64)
        r = float(F(rng.uniform(0.3, 3.0)))
        sphere, E, d, t, P, N = outside_hits(rng, c, r, 5000)
        assert len(P) > 3000
        ok, origin, direction = refract_ref.transmitted(sphere, E, d, t, P, N, F(ior))
        cos1, sin1, sin2, chord, tir, n = snell64(c, d, P, ior)
        # conditioning: a position is good to a few ulps of the scene's magnitude, an angle to that over the sphere's size
        pos = EPS * (np.abs(c).max() + r)
        # the child exists exactly when float64 finds neither total internal reflection nor an empty chord -- but within a few
        # ulps of the critical angle or of a tangent
        exists = ~tir & (chord > 0)
        critical = np.abs(sin2 - 1.0) < 64 * EPS
        tangent = (cos1 < 1e-3) & (chord < 64 * pos)
        disagree = ok != exists
        assert not (disagree & ~critical & ~tangent).any(), (ior, np.nonzero(disagree & ~critical & ~tangent)[0][:5])
        assert disagree.sum() <= 8, (ior, int(disagree.sum()))
        if ior >= 1:
            assert ok.mean() > 0.95
        else:
            assert 0.2 < ok.mean() < 0.95                        # rays beyond the critical angle are reflected whole
        s = ok & exists
        # the exit point: on the sphere, 1e-3 out along the normal there.  "The sphere" is the one the entry point lies on: the
        # float sphere test puts a hit up to ~1e-4 r off the radius near grazing, and the chord keeps it
        o64, dir64 = origin[s].astype(np.float64), direction[s].astype(np.float64)
        rho = np.linalg.norm(o64 - c, axis=1)
        err = np.abs(rho - (np.linalg.norm(P[s].astype(np.float64) - c, axis=1) + 1e-3))
        tol = 16 * pos + 2 * EPS * 1e-3
        assert (err <= tol).all(), (ior, err.max(), tol)
        worst["exit_point"] = max(worst["exit_point"], float(err.max() / tol))
        # entry: sin t1 = ior sin t2, t2 the angle between the chord and the inward normal
        N2 = (o64 - c) / rho[:, None]
        P2 = o64 - N2 * float(F(1e-3))
        chord_dir = P2 - P[s].astype(np.float64)
        L = np.linalg.norm(chord_dir, axis=1)
        sin_t2 = np.linalg.norm(np.cross(n[s], chord_dir / L[:, None]), axis=1)
        err = np.abs(sin1[s] - ior * sin_t2)
        tol = 96 * ior * pos / L + 16 * EPS
        assert (err <= tol).all(), (ior, float((err / tol).max()))
        worst["entry"] = max(worst["entry"], float((err / tol).max()))
        # exit: the ray leaves at the angle it came in (its cosine to the outward normal is cos t1); the error grows as
        # ior^2 / cos t1 near grazing, where the exit's sqrt(1 - ior^2 sin^2) is ill-conditioned
        cos_exit = np.einsum("ij,ij->i", dir64, N2)
        err = np.abs(cos_exit - cos1[s])
        tol = 2 * (pos / r + EPS) * (1 + ior * ior / np.maximum(cos1[s], 1e-7))
        assert (err <= tol).all(), (ior, float((err / tol).max()), float(err.max()))
        worst["exit_angle"] = max(worst["exit_angle"], float((err / tol).max()))
    assert all(v > 0 for v in worst.values()), worst


# ---- r', the reach of an area light's samples ------------------------------------------------------------------------------

def soft_reach(r, C):
    """rt_capi.hip, soft_reach(): r (1 + 2^-10) + 2^-22 max |C_k|, rounded up to a float"""
    if not r > 0:
        return 0.0
    want = float(r) * (1.0 + 2.0 ** -10) + 2.0 ** -22 * float(np.abs(np.asarray(C, dtype=np.float64)).max())
    f = F(want)
    if float(f) < want:
        f = np.nextafter(f, F(np.inf))
    return float(f)


def test_every_area_light_sample_lies_within_the_reach():
    """Thousands of (P, C, r, n, seed): |C| from 1e-3 to 3e4, r from 1e-6 to 1e3, shading points from 1e-2 to 1e4 radii away;
    every sample's distance from the centre on every axis, in float64, is at most r'.  The samples reach the rim: the largest
    of them come within a percent of r'."""
    rng = np.random.RandomState(2024)
    worst = 0.0
    for _ in range(3000):
        C = (rng.normal(size=3) * 10.0 ** rng.uniform(-3, np.log10(3e4))).astype(F)
        r = F(10.0 ** rng.uniform(-6, 3))
        n = int(rng.randint(1, 5))
        seed = int(rng.randint(0, 2 ** 32, dtype=np.uint64))
        w = rng.normal(size=(8, 3))
        w /= np.linalg.norm(w, axis=1, keepdims=True)
        P = (C + w * (float(r) * 10.0 ** rng.uniform(-2, 4, (8, 1)))).astype(F)
        P = P[np.any(P != C, axis=1)]
        key = rng.randint(0, 2 ** 32, len(P), dtype=np.uint64).astype(np.uint32)
        reach = soft_reach(r, C)
        for Q in soft_ref.disc_samples(seed, P, key, int(rng.randint(0, 9)), int(rng.randint(0, 2)), C, n, r):
            ok = np.isfinite(Q).all(axis=1)
            dev = np.abs(Q[ok].astype(np.float64) - C.astype(np.float64)).max(axis=1) if ok.any() else np.zeros(1)
            assert (dev <= reach).all(), (C, r, n, seed, float(dev.max()), reach)
            worst = max(worst, float(dev.max() / reach))
    assert 0.99 < worst <= 1.0, worst
