"""DEAD REFLECTIONS (csrc/rt_kernel.hip, RT_TWIN_DEAD_REFLECTIONS): the argument, in float32.

The unwind folds a reflection as final = local + (f * C_next) * oc, component by component.  Where oc is +-0, f * C_next is
finite and local is not -0, the sum has the bits of local: the reflected ray need not be traced.  Each condition has the
counter-example that makes it necessary, and the bound that makes f * C_next finite in a tame scene is evaluated."""
import numpy as np

F = np.float32
BITS = lambda a: np.asarray(a, dtype=F).view(np.uint32)


def fold(local, C_next, f, oc):
    """fold_child(): every operation rounded to float32, in the reference's order"""
    with np.errstate(all="ignore"):
        return np.asarray(local, F) + (np.asarray(f, F) * np.asarray(C_next, F)) * np.asarray(oc, F)


def test_zero_colour_leaves_local():
    rng = np.random.default_rng(20260)
    n = 200_000
    local = rng.integers(0, 2**32, n, dtype=np.uint64).astype(np.uint32).view(F)      # every bit pattern ...
    C_next = rng.integers(0, 2**32, n, dtype=np.uint64).astype(np.uint32).view(F)
    f = rng.uniform(-1.0, 1.0, n).astype(F)
    keep = np.isfinite(local) & np.isfinite(C_next) & (BITS(local) != 0x80000000)     # ... that is finite and not -0
    local, C_next, f = local[keep], C_next[keep], f[keep]
    # and the edges by hand: +0, the denormals, the largest floats, factors of +-1 and +-0
    tiny, huge = F(1e-45), np.finfo(F).max
    edge = np.array([0.0, tiny, -tiny, huge, -huge, 1.0, -1.0], dtype=F)
    el, ec, ef = np.meshgrid(edge, np.append(edge, F(-0.0)), np.array([1.0, -1.0, 0.0, -0.0, 0.5], dtype=F), indexing="ij")
    local, C_next, f = np.append(local, el.ravel()), np.append(C_next, ec.ravel()), np.append(f, ef.ravel())
    assert len(local) > 150_000
    for z in (F(0.0), F(-0.0)):
        got = fold(local, C_next, f, np.full_like(local, z))
        assert (BITS(got) == BITS(local)).all(), z


def test_each_condition_is_needed():
    zero = F(0.0)
    # (a) an infinite or NaN C_next: the product with +-0 is a NaN, and so is the pixel
    assert np.isnan(fold(F(0.25), F(np.inf), F(0.5), zero))
    assert np.isnan(fold(F(0.25), F(np.nan), F(0.5), zero))
    # ... which a finite C_next above FLT_MAX / |f| would also produce if |f| could exceed 1: f * C_next overflows
    assert np.isnan(fold(F(0.25), np.finfo(F).max, F(2.0), zero))
    # (c) local = -0 with a +0 addend: the reference returns +0, skipping would return -0
    assert BITS(fold(F(-0.0), F(1.0), F(0.5), zero)) == 0 and BITS(F(-0.0)) == 0x80000000
    # ... and -0 + -0 stays -0, which is why "never -0" is about local and not about the addend
    assert BITS(fold(F(-0.0), F(1.0), F(0.5), F(-0.0))) == 0x80000000
    # (b) a colour with one component 1e-45 is not zero: that component of the fold changes
    oc = np.array([0.0, 0.0, 1e-45], dtype=F)
    local = np.array([0.0, 0.0, 0.0], dtype=F)
    got = fold(local, np.full(3, 3.0, dtype=F), np.full(3, 1.0, dtype=F), oc)
    assert (BITS(got)[:2] == 0).all() and got[2] != 0.0
    # the kernel's test on the bits: ((x | y | z) << 1) == 0 -- -0 is zero, 1e-45 and a NaN are not
    def dead(c):
        b = BITS(np.array(c, dtype=F)).astype(np.uint64)
        return ((int(b[0] | b[1] | b[2]) << 1) & 0xFFFFFFFF) == 0
    assert dead((0.0, 0.0, 0.0)) and dead((-0.0, 0.0, -0.0))
    assert not dead((0.0, 0.0, 1e-45)) and not dead((0.0, np.nan, 0.0)) and not dead((0.0, 0.0, 0.5)) and not dead((-1e-45, 0.0, 0.0))


def test_bound_is_finite():
    """(a): |cos| <= 3 and |V.R| <= 21 for unit-length-within-rounding vectors; a light's addends are at most 3 (the diffuse sum
    is clamped to 1 where the diffuse factor is positive, unclamped terms have |cos * df * I * oc * lc| <= 3) plus 21^20 < 2^88;
    4 000 lights a level, and a fold with |f|, |oc| <= 1 adds at most the child: |C| <= (depth + 1) * n_lights * (3 + 2^88)."""
    assert 21.0 ** 20 < 2.0 ** 88
    level = 4000 * (3 + 2 ** 88)                      # exact, in Python integers
    assert level < 2 ** 101
    bound = (2 ** 20 + 1) * 2 ** 101
    assert bound < int(np.finfo(F).max)
    assert float(bound) < float(np.finfo(F).max) / 64
    # and in float32 arithmetic itself, the sum of a level's addends does not overflow
    assert np.isfinite(F(4000) * (F(3) + F(2.0 ** 88)) * F(2 ** 20 + 1))
