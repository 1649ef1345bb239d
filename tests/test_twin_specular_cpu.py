"""The exactness argument of the SPECULAR GATE (csrc/rt_kernel.hip, RT_LIGHT_TERMS), in float32 on the CPU.

The reference's statement (src/RayTracer.cpp:561-588), operation by operation as the kernels compute it:
    R = L - N * (2 * (L . N));  dot = d . R;  if (dot > 0) C += light_colour * (dot^20 * specular_factor)
with dot^20 as nineteen multiplies.  The gate skips it where the specular factor is +-0 and the light's colour is finite.  The
test asserts that under exactly that condition no bit of C changes -- for C = +0, a small and a large value, every sign and
size of colour, vectors at the bound of the argument -- and that just outside it (the smallest factor that is not zero, an
infinite colour, a C of -0 that shading never has) bits do change."""
import numpy as np

F = np.float32
N_SAMPLES = 4096


def dot3(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def specular_term(C, N, d, L, factor, colour):
    """C after the statement; float32 arrays (n, 3), factor (n,), colour (n, 3)"""
    assert all(v.dtype == F for v in (C, N, d, L, factor, colour))
    R = L - N * (F(2.0) * dot3(L, N))[..., None]
    dot = dot3(d, R)
    pw = dot.copy()
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        for _ in range(19):
            pw = pw * dot
        spec = pw * factor
        added = C + colour * spec[..., None]
    return np.where((dot > 0)[..., None], added, C), dot, pw


def unit_vectors(rng, n):
    v = rng.standard_normal((n, 3)).astype(F)
    length = np.sqrt(dot3(v, v))
    return (v / length[..., None]).astype(F)


def vectors(rng):
    """random unit vectors, then the corners of the argument's bound: every component of magnitude 1"""
    N, d, L = (unit_vectors(rng, N_SAMPLES) for _ in range(3))
    signs = np.array([[sx, sy, sz] for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)], dtype=F)
    cn, cd, cl = (signs[i] for i in np.indices((8, 8, 8)).reshape(3, -1))
    return np.concatenate([N, cn]), np.concatenate([d, cd]), np.concatenate([L, cl])


def bits(a):
    return np.ascontiguousarray(a, dtype=F).view(np.uint32)


ZERO_FACTORS = [F(0.0), F(-0.0)]
FINITE_COLOURS = [(0.0, -1.0, 1e30), (-0.0, 1.0, -1e30), (3.0e38, -3.0e38, 1e-45), (0.5, 0.25, 1.0)]
STARTS = [F(0.0), F(1e-30), F(1.0)]                 # C: +0 at the top of shading, then sums clamped to at most 1


def test_bound_of_the_power():
    """|d . R| < 2^6.4 wherever every component is at most 1 in magnitude, so the twentieth power is finite"""
    N, d, L = vectors(np.random.default_rng(1))
    C = np.zeros_like(N)
    _, dot, pw = specular_term(C, N, d, L, np.zeros(len(N), dtype=F), np.zeros_like(N))
    assert np.abs(dot).max() < 2.0 ** 6.4 and np.abs(dot).max() >= 15.0          # (the corners reach 15)
    assert np.isfinite(pw).all() and (pw > 0).sum() > 1000


def test_no_bit_changes_under_the_gate():
    N, d, L = vectors(np.random.default_rng(2))
    n = len(N)
    live = 0
    for factor in ZERO_FACTORS:
        for colour in FINITE_COLOURS:
            for start in STARTS:
                C = np.full((n, 3), start, dtype=F)
                after, dot, _ = specular_term(C, N, d, L, np.full(n, factor, dtype=F), np.tile(np.array(colour, dtype=F), (n, 1)))
                assert (bits(after) == bits(C)).all(), (factor, colour, start)
                live += int((dot > 0).sum())
    assert live > 10000                                  # the statement ran: the rows with dot > 0 added their +-0


def test_a_nan_dot_adds_nothing():
    """a NaN normal: the dot product is NaN and fails dot > 0, with or without the gate"""
    N, d, L = vectors(np.random.default_rng(3))
    N = N.copy()
    N[::2, 1] = np.nan
    C = np.full_like(N, 0.25)
    after, dot, _ = specular_term(C, N, d, L, np.full(len(N), 0.5, dtype=F), np.ones_like(N))
    assert np.isnan(dot[::2]).all() and (bits(after[::2]) == bits(C[::2])).all()
    assert (bits(after[1::2]) != bits(C[1::2])).any()


def test_bits_change_just_outside_the_gate():
    N, d, L = vectors(np.random.default_rng(4))
    n = len(N)
    zero, ones = np.zeros((n, 3), dtype=F), np.ones((n, 3), dtype=F)

    def changed(C, factor, colour):
        after, dot, pw = specular_term(C, N, d, L, np.full(n, factor, dtype=F), colour)
        return (bits(after) != bits(C)).any(axis=-1), dot, pw

    # the smallest factor that is not zero, under a large finite colour
    diff, dot, pw = changed(zero, F(1e-45), np.full((n, 3), 1e30, dtype=F))
    assert F(1e-45) != 0 and diff[(dot > 0) & (pw >= 1.0)].all() and diff.sum() > 8
    # an infinite colour component under factor 0: 0 x inf
    colour = ones.copy()
    colour[:, 1] = np.inf
    diff, dot, _ = changed(zero, F(0.0), colour)
    assert (diff == (dot > 0)).all() and diff.sum() > 1000
    # C = -0, which shading never holds (it starts at +0, and a sum is -0 only if both addends are): -0 + +0 = +0
    diff, dot, _ = changed(np.full((n, 3), -0.0, dtype=F), F(0.0), ones)
    assert (diff == (dot > 0)).all() and diff.sum() > 1000
    # ... and sums from +0 never are -0, whatever the sign of the addend
    for addend in (F(-0.0), F(0.0), F(-1e-45), F(1e-45)):
        assert bits(F(0.0) + addend) != bits(F(-0.0))
