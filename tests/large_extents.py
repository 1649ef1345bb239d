"""Shared by test_large_extents_gpu.py and test_limits_cpu.py: where the byte boundaries 2^31, 2^32, ... fall in a buffer of
columns, the camera's rays of single columns of a frame too large to build whole, and device buffers between guards.

The conventions the large tests hold the kernels to ("Index widths"): a pixel, ray or record NUMBER fits 32 bits
(the API's int arguments), a number of pixels in a launch and every BYTE or WORD offset derived from one is 64-bit before it is
multiplied.  Every reference here is independent of that arithmetic: the oracle and the numpy restatements compute one column
at a time, and the kernels' own strips of at most 1024 columns start at offset 0 of a small buffer, the regime the rest of the
suite pins."""
import numpy as np

F = np.float32
# A quiet NaN with a payload: no kernel produces it (the scenes here make no NaN at all, and an arithmetic NaN is 0x7FC00000 or
# 0xFFC00000), so a word that still holds it was not written, and a guard word that no longer holds it was.
SENTINEL = 0x7FC5A5A5
SENTINEL_BYTE = 0xA5                      # the verdicts are 0 or 1
GUARD_BYTES = 1 << 20
STRIP_COLUMNS = 1024
CHUNK_WORDS = 1 << 28                     # the device reductions below go a GiB at a time: no temporary of the buffer's size


def boundary_columns(boundaries, stride_bytes, n_cols):
    """The columns to check against the oracle-side reference in a buffer of n_cols columns of stride_bytes each: column 0, the
    last one, and for every byte boundary B the column that straddles it with its two neighbours.  B must fall INSIDE a column
    (B % stride != 0) and inside the buffer."""
    cols = {0, n_cols - 1}
    for B in boundaries:
        assert B % stride_bytes != 0, f"boundary {B} falls between two columns of {stride_bytes} bytes: choose another H"
        c = B // stride_bytes
        assert 1 <= c <= n_cols - 2, f"boundary {B} is not inside a buffer of {n_cols} columns of {stride_bytes} bytes"
        cols |= {c - 1, c, c + 1}
    return sorted(cols)


def runs(cols):
    """sorted column numbers -> [(x0, x1)) runs of consecutive ones"""
    out = []
    for c in cols:
        if out and out[-1][1] == c:
            out[-1][1] = c + 1
        else:
            out.append([c, c + 1])
    return [tuple(r) for r in out]


def column_rays(cam, W, H, x0, x1):
    """rays_ref.camera_rays(cam, W, H)[x0:x1] without building the frame's: the (x1 - x0, H, 6) rays rt_render traces for columns
    [x0, x1) of a W x H frame, {eye, pixel}, the pixel as create_eye_ray computes it in fp32, one rounding per operation"""
    if hasattr(cam, "contents"):
        cam = cam.contents
    xyz = lambda v: np.array([v.x, v.y, v.z] if hasattr(v, "x") else [v[0], v[1], v[2]], dtype=F)
    dx = np.arange(x0, x1).astype(F) / F(W)                       # (float)x / W
    dz = np.arange(H).astype(F) / F(H)
    scalar_x = dx * F(cam.screen_width) - F(cam.screen_halfwidth)
    scalar_y = dz * F(cam.screen_height) - F(cam.screen_halfheight)
    so, ch, cv = xyz(cam.screen_origin), xyz(cam.vector_horizontal), xyz(cam.vector_vertical)
    pixel = so[None, None, :] + ch[None, None, :] * scalar_x[:, None, None]
    pixel = pixel + cv[None, None, :] * scalar_y[None, :, None]
    rays = np.empty((x1 - x0, H, 6), dtype=F)
    rays[..., :3] = xyz(cam.eye_origin)
    rays[..., 3:] = pixel
    return rays


def column_keys(H, x0, x1):
    """the sampling keys of columns [x0, x1) of a frame H high: x * H + z, modulo 2^32 (soft_ref.render's)"""
    keys = np.arange(x0, x1, dtype=np.uint64)[:, None] * np.uint64(H) + np.arange(H, dtype=np.uint64)[None, :]
    return (keys & np.uint64(0xFFFFFFFF)).astype(np.uint32)


def first_difference(got, want):
    """int32 numpy views of equal shape -> None, or (flat word index of the first difference, got word, want word, how many
    words differ)"""
    g, w = np.ascontiguousarray(got).reshape(-1), np.ascontiguousarray(want).reshape(-1)
    bad = np.flatnonzero(g != w)
    return None if len(bad) == 0 else (int(bad[0]), int(g[bad[0]]), int(w[bad[0]]), len(bad))


# ---- on the device (torch is imported by the caller's process: conftest.py) ---------------------------------------------------

class Guarded:
    """n int32 words (or, as_bytes=True, n bytes) of device memory inside one larger tensor: GUARD_BYTES before and after, every
    word of all three filled with the sentinel.  body is the view a launch writes; its address is 16-byte aligned."""

    def __init__(self, n, as_bytes=False):
        import torch
        self.torch = torch
        self.n = int(n)
        self.guard = GUARD_BYTES if as_bytes else GUARD_BYTES // 4
        self.fill = SENTINEL_BYTE if as_bytes else SENTINEL
        self.all = torch.full((self.guard + self.n + self.guard,), self.fill, dtype=torch.uint8 if as_bytes else torch.int32,
                              device="cuda")
        self.body = self.all[self.guard:self.guard + self.n]
        assert self.body.data_ptr() % 16 == 0

    @staticmethod
    def need(n, as_bytes=False):
        return int(n) * (1 if as_bytes else 4) + 2 * GUARD_BYTES

    @property
    def ptr(self):
        return self.body.data_ptr()

    def refill(self):
        self.all.fill_(self.fill)

    def guards_untouched(self):
        head, tail = self.all[:self.guard], self.all[self.guard + self.n:]
        return bool((head == self.fill).all()) and bool((tail == self.fill).all())

    def sentinels_left(self, upto=None):
        """how many words of body[:upto] still hold the sentinel"""
        body = self.body if upto is None else self.body[:upto]
        return count_equal(body, self.fill)

    def assert_written(self, what, upto=None):
        assert self.guards_untouched(), f"{what}: a guard word before or after the output was overwritten"
        left = self.sentinels_left(upto)
        assert left == 0, f"{what}: {left} output words were never written"

    def free(self):
        self.all = self.body = None


def hashed(n, salt, scale=1.0, offset=0.0):
    """n floats in [offset, offset + scale) on the device, a hash of their index, made a chunk at a time (never the sentinel: it is
    no finite number)"""
    import torch
    out = torch.empty((n,), dtype=torch.float32, device="cuda")
    step = 1 << 26
    for c0 in range(0, n, step):
        k = torch.arange(c0, min(c0 + step, n), dtype=torch.int64, device="cuda")
        out[c0:c0 + step] = ((((k + salt) * 2654435761) >> 7) & 0xFFFF).to(torch.float32) * (scale / 65536.0) + offset
        del k
    return out


def count_equal(t, value):
    total = 0
    flat = t.reshape(-1)
    for c0 in range(0, flat.numel(), CHUNK_WORDS):
        total += int((flat[c0:c0 + CHUNK_WORDS] == value).sum())
    return total


def checksum(t):
    """a 64-bit sum and a 64-bit position-weighted sum of an int32 tensor's words, a GiB at a time (wrapping: any changed word
    changes the first unless another changes by the opposite amount, and then the second)"""
    import torch
    flat = t.reshape(-1)
    a = b = 0
    step = CHUNK_WORDS >> 2                # (three int64 temporaries of this many words)
    for k, c0 in enumerate(range(0, flat.numel(), step)):
        part = flat[c0:c0 + step].to(torch.int64)
        a = (a + int(part.sum())) & 0xFFFFFFFFFFFFFFFF
        weights = torch.arange(1, part.numel() + 1, dtype=torch.int64, device=part.device)
        b = (b + (k + 1) * int((part * weights).sum())) & 0xFFFFFFFFFFFFFFFF
        del part, weights
    return a, b


def device_difference(got, want, words_per_column, what, first_column=0):
    """two int32 device tensors of equal length -> None, or the text of the first differing word: its number, its column
    (counted from first_column) and word within the column, its byte offset in the output, both values, and how many differ"""
    import torch
    assert got.numel() == want.numel(), (what, got.numel(), want.numel())
    if torch.equal(got, want):
        return None
    n_bad, first = 0, None
    for c0 in range(0, got.numel(), CHUNK_WORDS):
        ne = got[c0:c0 + CHUNK_WORDS] != want[c0:c0 + CHUNK_WORDS]
        k = int(ne.sum())
        if k and first is None:
            first = c0 + int(ne.nonzero()[0])
        n_bad += k
        del ne
    g, w = int(got[first]) & 0xFFFFFFFF, int(want[first]) & 0xFFFFFFFF
    at = first_column * words_per_column + first
    return (f"{what}: {n_bad} of {got.numel()} words differ, first at word {at} of the output (column {at // words_per_column}, "
            f"word {at % words_per_column} of it, byte offset {at * 4}): got 0x{g:08x}, want 0x{w:08x}"
            + (" (the sentinel: never written)" if g == SENTINEL else ""))


def assert_columns_equal_strips(render_strip, outputs, n_cols, what, strip_columns=STRIP_COLUMNS):
    """Ground rule (b): every word of a launch's large outputs equals the same kernel's strips of at most strip_columns columns,
    each rendered at offset 0 of small guarded buffers -- the regime the rest of the suite pins.  outputs: [(int32 device view of
    n_cols columns, words per column)], one per output of the call; render_strip(x0, x1, *addresses) enqueues columns [x0, x1)."""
    import torch
    small = [Guarded(strip_columns * wpc) for _, wpc in outputs]
    try:
        for x0 in range(0, n_cols, strip_columns):
            x1 = min(x0 + strip_columns, n_cols)
            for s in small:
                s.refill()
            render_strip(x0, x1, *[s.ptr for s in small])
            torch.cuda.synchronize()
            for k, ((big, wpc), s) in enumerate(zip(outputs, small)):
                words = (x1 - x0) * wpc
                s.assert_written(f"{what}: output {k} of strip {x0}:{x1}", words)
                assert s.sentinels_left() == s.n - words, f"{what}: output {k} of strip {x0}:{x1} was written past its end"
                text = device_difference(big[x0 * wpc:x1 * wpc], s.body[:words], wpc,
                                         f"{what}: output {k}, columns {x0}:{x1} against their own strip", x0)
                assert text is None, text
    finally:
        for s in small:
            s.free()


def require_device_memory(need_bytes):
    """skip only if the device's free memory is below 1.1 x the test's need (both numbers in the message) -> free bytes"""
    import pytest
    import torch
    torch.cuda.empty_cache()
    free, _ = torch.cuda.mem_get_info()
    assert need_bytes <= 48e9, f"a single test may need at most 48 GB, not {need_bytes}"
    if free < 1.1 * need_bytes:
        pytest.skip(f"needs {need_bytes} bytes of device memory (x 1.1), {free} are free")
    return free
