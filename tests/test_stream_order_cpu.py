"""What tests/test_stream_order_gpu.py relies on, from the references alone (tests/stream_order_refs.py): the two calls of a pair
have references that differ in more than half of their pixels or records -- outputs that mixed the two calls, or a test that
confused them, could then not pass -- and no reference holds the sentinel the outputs are filled with before the calls."""
import numpy as np
import pytest

import poisoned
import stream_order_refs as refs


@pytest.mark.parametrize("case", refs.DIFFERING)
def test_the_two_references_of_a_pair_differ_in_more_than_half_of_their_cells(case):
    one, two = refs.reference(case, 0), refs.reference(case, 1)
    assert len(one) == len(two) and all(a.shape == b.shape and a.dtype == b.dtype for a, b in zip(one, two)), case
    share = refs.differing_share(one, two)
    print(f"{case}: the references differ in {share:.3f} of {refs.W * refs.H} cells")
    assert share > 0.5, (case, share)


def test_the_pairs_left_out_cannot_be_confused_or_are_one_frame_on_purpose():
    assert set(refs.PAIRS) - set(refs.DIFFERING) == {"rays-queries", "repack"}
    colours, = refs.reference("rays-queries", 0)
    hits, = refs.reference("rays-queries", 1)
    assert colours.dtype == np.float32 and colours.shape == (refs.W, refs.H, 3) and hits.dtype.itemsize == 48
    assert refs.differing_share(refs.reference("repack", 0), refs.reference("repack", 1)) == 0.0


def test_the_frames_of_the_two_handles_differ_pairwise():
    frames = [refs.two_handles_reference(i) for i in range(len(refs.TWO_HANDLES))]
    for i in range(len(frames)):
        for j in range(i + 1, len(frames)):
            share = refs.differing_share((frames[i],), (frames[j],))
            print(f"two handles, frames {i} and {j}: differ in {share:.3f}")
            assert share > 0.5, (refs.TWO_HANDLES[i], refs.TWO_HANDLES[j], share)


@pytest.mark.parametrize("case", list(refs.PAIRS))
def test_no_reference_holds_the_sentinel(case):
    for k in (0, 1):
        for a in refs.reference(case, k):
            poisoned.assert_reference_has_no_sentinel(a, f"{case}, call {k + 1}")        # (bytes: the byte sentinel)
    if case == "repack":
        for i in range(len(refs.TWO_HANDLES)):
            poisoned.assert_reference_has_no_sentinel(refs.two_handles_reference(i), f"two handles, frame {i}")
