"""A stream that is held busy for a measured time, so that a test can issue a call on it, then -- with nothing synchronised -- a
call on another stream, and know that the first call had not started when the second was issued (tests/test_stream_order_gpu.py).

hold(stream, ms) enqueues a timed busy kernel on `stream` between two events: torch.cuda._sleep, its cycles calibrated once per
process by two events; without _sleep, a chain of plain device fills calibrated the same way.  Nothing in it waits for the host:
the hold ends by itself whatever becomes of the test.  Held.query() is True once the hold has ended; Held.lasted_ms(), after the
streams are synchronised, is how long it did last.

How long to hold is measured as well (idle_times(), planned_ms()): at least WALL_FACTOR times the wall-clock time of the second
call on an idle handle, so that the host-side part of that call cannot outlast the hold, never less than the first call's own
kernels take on an idle stream, and never less than FLOOR_MS (a ray query returns in 0.03 ms).  The kernel is asked for MARGIN
times the plan, and the tests assert the plan."""
import time

WALL_FACTOR = 20.0
MARGIN = 1.5
FLOOR_MS = 2.0
FILL_WORDS = 1 << 24                      # the fallback's fills: 64 MiB each
_rate = None                              # ("sleep", cycles per ms) or ("fill", fills per ms, the buffer)


def _calibrate():
    global _rate
    if _rate is not None:
        return _rate
    import torch
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    if hasattr(torch.cuda, "_sleep"):
        def timed(cycles):
            t0.record()
            torch.cuda._sleep(cycles)
            t1.record()
            t1.synchronize()
            return t0.elapsed_time(t1)

        timed(1000)                                               # the kernel's load is no part of any measurement
        cycles = 1_000_000
        for _ in range(8):
            if timed(cycles) >= 5.0:
                break
            cycles *= 4
        # the shortest of three: whatever else a measurement holds makes the rate too low and the holds too short
        ms = min(timed(cycles) for _ in range(3))
        assert ms >= 1.0, f"torch.cuda._sleep({cycles}) took {ms} ms: cannot be calibrated"
        _rate = ("sleep", cycles / ms, None)
    else:
        buf = torch.empty(FILL_WORDS, dtype=torch.int32, device="cuda")
        buf.fill_(0)
        fills = 64

        def timed():
            t0.record()
            for k in range(fills):
                buf.fill_(k)
            t1.record()
            t1.synchronize()
            return t0.elapsed_time(t1)

        _rate = ("fill", fills / min(timed() for _ in range(3)), buf)
    return _rate


class Held:
    def __init__(self, start, end, planned_ms):
        self.start, self.end, self.planned_ms = start, end, planned_ms

    def query(self):
        """True once the hold has ended"""
        return self.end.query()

    def lasted_ms(self):
        self.end.synchronize()
        return self.start.elapsed_time(self.end)


def hold(stream, ms):
    """keep `stream` (a torch stream) busy for at least `ms` from when it gets there -> Held"""
    import torch
    kind, per_ms, buf = _calibrate()
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with torch.cuda.stream(stream):
        start.record(stream)
        if kind == "sleep":
            torch.cuda._sleep(int(ms * MARGIN * per_ms) + 1)
        else:
            for k in range(int(ms * MARGIN * per_ms) + 1):
                buf.fill_(k)
        end.record(stream)
    return Held(start, end, float(ms))


def idle_times(call1, call2, a, b):
    """both calls once with the device idle, call1(stream a) then call2(stream b) -> (the ms call 1's kernels take on the idle
    stream, by two events; the wall-clock ms of call 2, from before it is issued until its stream has drained)"""
    import torch
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record(a)
    call1(a.cuda_stream)
    t1.record(a)
    t1.synchronize()
    kernels_ms = t0.elapsed_time(t1)
    torch.cuda.synchronize()
    w0 = time.perf_counter()
    call2(b.cuda_stream)
    b.synchronize()
    wall_ms = (time.perf_counter() - w0) * 1.0e3
    torch.cuda.synchronize()
    return kernels_ms, wall_ms


def planned_ms(kernels_ms, wall_ms):
    return max(WALL_FACTOR * wall_ms, kernels_ms, FLOOR_MS)


def independent(a, b, ms=5.0):
    """work on stream b finishes while stream a is held: the two do not share a hardware queue"""
    import torch
    torch.cuda.synchronize()
    word = torch.zeros(16, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    held = hold(a, ms)
    with torch.cuda.stream(b):
        word.fill_(1)
    b.synchronize()
    free = not held.query()
    torch.cuda.synchronize()
    return free


def streams(candidates=8):
    """-> {"null": the null stream, "side", "other": two side streams}, each pair of which runs independently (independent()):
    the runtime spreads its streams over a few hardware queues, and two streams that share one would queue behind each other
    whatever the library does"""
    import torch
    null = torch.cuda.default_stream()
    assert null.cuda_stream == 0
    _calibrate()
    made = [torch.cuda.Stream() for _ in range(candidates)]
    good = [s for s in made if s.cuda_stream != 0 and independent(s, null) and independent(null, s)]
    for i, s in enumerate(good):
        for t in good[i + 1:]:
            if independent(s, t) and independent(t, s):
                return {"null": null, "side": s, "other": t}
    raise AssertionError(f"of {candidates} side streams no two run independently of each other and of the null stream")
