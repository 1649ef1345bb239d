"""Pin the oracle: its output must reproduce the SHA-256 digests and spot
pixel values recorded in SURVEY.md Appendix D from the survey's scratch build
of the reference, and the committed golden fixtures must be those same images.

The reference ships no tests and no fixtures of its own.  These recorded
digests were the first external pin; test_reference_pins_cpu.py holds the
oracle to a repeatable build of the reference itself (DESIGN.md "Oracle").
"""
import hashlib
import os

import numpy as np
import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.mark.parametrize("key", ["b64d4", "g32_64d4", "g16_64d8", "b256d4", "g32d4", "g16d8", "b512d3"])
def test_oracle_reproduces_survey_digest(oracle, key):
    name, W, H, depth, digest = oracle.SURVEY_PINS[key]
    img = oracle.OracleScene.named(name).render(W, H, depth)
    assert oracle.sha256(img) == digest


def test_spot_values_b64d4(oracle):
    img = oracle.OracleScene.builtin().render(64, 64, 4)
    np.testing.assert_array_equal(img[0, 0], np.float32([0.62334645, 0.54042655, 0.54042655]))
    np.testing.assert_array_equal(img[32, 32], np.float32([0.5022828, 0, 0]))
    np.testing.assert_array_equal(img[63, 63], np.float32([0.15409102, 0.15409102, 0.15409102]))


@pytest.mark.parametrize("key", ["b64d4", "g32_64d4", "g16_64d8"])
def test_golden_fixture_is_the_pinned_image(oracle, key):
    name, W, H, depth, digest = oracle.SURVEY_PINS[key]
    raw = open(os.path.join(GOLDEN, key + ".f32"), "rb").read()
    assert len(raw) == W * H * 3 * 4
    assert hashlib.sha256(raw).hexdigest() == digest


def test_strip_equals_full_render(oracle):
    s = oracle.OracleScene.builtin()
    full = s.render(96, 40, 3)
    np.testing.assert_array_equal(s.render(96, 40, 3, 17, 61).view(np.uint32), full[17:61].view(np.uint32))
    assert s.render(96, 40, 3, 5, 5).shape == (0, 40, 3)


def test_stride_subsample_property(oracle):
    # (float)(8k)/512 == (float)k/64: a stride-8 subsample of the 512^2 render is the 64^2 render
    s = oracle.OracleScene.builtin()
    big = s.render(512, 512, 2)
    small = s.render(64, 64, 2)
    np.testing.assert_array_equal(big[::8, ::8].view(np.uint32), small.view(np.uint32))


def test_depth_zero_and_background(oracle):
    s = oracle.OracleScene.grid(4, shadows=True)
    img = s.render(32, 32, 0)
    assert np.isfinite(img).all()
    # horizon row: rays parallel to floor and ceiling miss everything -> NULL_COLOR
    np.testing.assert_array_equal(img[16, 16], np.float32([0.75, 0.75, 0.75]))


def test_no_final_clamp(oracle):
    img = oracle.OracleScene.builtin().render(128, 128, 4)
    assert img.max() > 1.0     # the reference's final clamp is commented out (src/RayTracer.cpp:619-631)


def test_work_counters(oracle):
    s = oracle.OracleScene.builtin()
    s.render(64, 64, 3)
    c = oracle.OracleScene.counters()
    assert c.nearest_rays >= 64 * 64 and c.shadow_rays > 0 and c.collision_tests > c.nearest_rays
