"""poisoned.py's checking half, on numpy arrays: what the helper is for must be refused, and a clean output must pass.  No
device, no torch."""
import subprocess
import sys
import os

import numpy as np
import pytest

import poisoned
from large_extents import SENTINEL, SENTINEL_BYTE

W, H = 37, 29                             # 10 x 2 tiles of 4 x 16, the last of either side ragged
TX, TZ = 4, 16
GUARD = 256


def buffers(words_per_cell=3, dtype=np.int32, fill=SENTINEL):
    """a written W x H output between two guards, with slack -> (head, body, tail, needed, layout)"""
    needed = W * H * words_per_cell
    rng = np.random.RandomState(3)
    body = np.full(needed + poisoned.SLACK_CELLS * words_per_cell, fill, dtype=dtype)
    body[:needed] = rng.randint(0, 2, needed) if dtype == np.uint8 else rng.rand(needed).astype(np.float32).view(np.int32)
    head, tail = np.full(GUARD, fill, dtype=dtype), np.full(GUARD, fill, dtype=dtype)
    return head, body, tail, needed, poisoned.layout(words_per_cell, H, 0, TX, TZ, 1, poisoned.RGB[:words_per_cell])


def test_a_written_output_passes_and_comes_back():
    head, body, tail, needed, lay = buffers()
    out = poisoned.check_output(head, body, tail, needed, lay, "clean")
    assert out.shape == (needed,) and np.array_equal(out.view(np.int32), body[:needed])
    head, body, tail, needed, lay = buffers(1, np.uint8, SENTINEL_BYTE)
    assert poisoned.check_output(head, body, tail, needed, lay, "clean bytes", SENTINEL_BYTE).shape == (needed,)


def test_one_tile_left_at_the_sentinel_is_named_as_that_tile():
    """tile column 5, tile row 1 (a ragged one: rows 16..28) of 4 x 16 tiles: every word of its pixels unwritten"""
    head, body, tail, needed, lay = buffers()
    frame = body[:needed].reshape(W, H, 3)
    frame[5 * TX:6 * TX, 1 * TZ:2 * TZ] = SENTINEL
    with pytest.raises(AssertionError) as e:
        poisoned.check_output(head, body, tail, needed, lay, "one tile")
    text = str(e.value)
    assert f"{4 * 13 * 3} of {needed} output words were never written" in text
    assert "first at pixel (x=20, z=16) channel r" in text
    assert "tile column 5, tile row 1" in text and "1 tile:" in text and "tile (5, 1) was dropped whole (52 cells)" in text
    # a full 64-word tile of a one-word output (the AO plane), and one cell of it alone
    head, body, tail, needed, lay = buffers(1)
    plane = body[:needed].reshape(W, H)
    plane[2 * TX:3 * TX, 0:TZ] = SENTINEL
    with pytest.raises(AssertionError) as e:
        poisoned.check_output(head, body, tail, needed, lay, "one tile of 64 words")
    assert "64 of" in str(e.value) and "tile (2, 0) was dropped whole (64 cells)" in str(e.value)
    plane[2 * TX:3 * TX, 0:TZ] = 7
    plane[9, 3] = SENTINEL
    with pytest.raises(AssertionError) as e:
        poisoned.check_output(head, body, tail, needed, lay, "one cell")
    assert "pixel (x=9, z=3)" in str(e.value) and "1 of the 64 cells of tile (2, 0)" in str(e.value)


def test_tiles_of_a_strip_and_of_a_supersampled_frame():
    """a strip's tiles count from its x0; a k x k frame's tiles are the virtual image's, k times the output's pixels"""
    lay = poisoned.layout(3, H, x0=100, tile_x=TX, tile_z=TZ)
    assert poisoned.locate((9 * H + 17) * 3 + 2, lay) == (109, 17, "2", (2, 1))
    lay = poisoned.layout(3, H, 0, 4, 16, scale=2)
    assert poisoned.locate((9 * H + 17) * 3, lay)[3] == (4, 2)
    assert poisoned.locate(5, poisoned.layout(12, 7, channels=poisoned.HIT_FIELDS))[:3] == (0, 0, "normal.x")


def test_one_slack_word_overwritten():
    head, body, tail, needed, lay = buffers()
    body[needed + 5] = 0
    with pytest.raises(AssertionError) as e:
        poisoned.check_output(head, body, tail, needed, lay, "slack")
    assert "slack" in str(e.value) and "the first 5 words past it" in str(e.value)
    head, body, tail, needed, lay = buffers(1, np.uint8, SENTINEL_BYTE)
    body[-1] = 1
    with pytest.raises(AssertionError):
        poisoned.check_output(head, body, tail, needed, lay, "slack byte", SENTINEL_BYTE)


@pytest.mark.parametrize("which, at", [("head", GUARD - 1), ("head", 0), ("tail", 0), ("tail", GUARD - 1)])
def test_one_guard_word_overwritten(which, at):
    head, body, tail, needed, lay = buffers()
    (head if which == "head" else tail)[at] = 0x3F800000
    with pytest.raises(AssertionError) as e:
        poisoned.check_output(head, body, tail, needed, lay, "guard")
    assert "guard" in str(e.value) and ("before" if which == "head" else "after") in str(e.value)


def test_a_reference_that_contains_the_sentinel():
    want = np.random.RandomState(1).rand(W, H, 3).astype(np.float32)
    poisoned.assert_reference_has_no_sentinel(want, "fine")
    want.view(np.uint32)[3, 4, 1] = SENTINEL
    with pytest.raises(AssertionError) as e:
        poisoned.assert_reference_has_no_sentinel(want, "frame")
    assert "sentinel" in str(e.value)
    from tilecoderaytracer_amd.renderer import HIT_DTYPE
    records = np.zeros((5, 3), dtype=HIT_DTYPE)
    poisoned.assert_reference_has_no_sentinel((np.ones((5, 3, 3), np.float32), records), "fine")
    records["normal"][2, 1, 2] = np.array([SENTINEL], dtype=np.uint32).view(np.float32)[0]
    with pytest.raises(AssertionError):
        poisoned.assert_reference_has_no_sentinel((np.ones((5, 3, 3), np.float32), records), "records")
    # an arithmetic NaN is not the sentinel
    poisoned.assert_reference_has_no_sentinel(np.full(4, np.nan, dtype=np.float32), "NaN")
    verdicts = np.zeros(9, dtype=np.bool_)
    poisoned.assert_reference_has_no_sentinel(verdicts.view(np.uint8), "verdicts")
    with pytest.raises(AssertionError):
        poisoned.assert_reference_has_no_sentinel(np.full(3, SENTINEL_BYTE, dtype=np.uint8), "bytes")


def test_importing_the_helper_needs_neither_torch_nor_a_device():
    code = ("import sys; sys.modules['torch'] = None; import poisoned; "
            "assert 'tilecoderaytracer_amd.capi' not in sys.modules; print('ok')")
    p = subprocess.run([sys.executable, "-c", code], cwd=os.path.dirname(os.path.abspath(__file__)), capture_output=True,
                       text=True, timeout=120)
    assert p.returncode == 0 and p.stdout.strip() == "ok", (p.stdout, p.stderr[-500:])
