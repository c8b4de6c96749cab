"""A stalled device for the stream-ordering tests (tests/test_gpu_stream_order.py).  On an idle device a missing wait between two
streams nearly always passes: the producer has finished before the consumer is even queued.  `stall` puts a bounded device-side
delay on the producer's stream, so that everything queued behind it is late by construction, and a consumer on another stream that
lacks its wait runs at once and reads what was there before -- the poison the tests put there.

The delay is torch.cuda._sleep, which spins for a number of ticks of a device clock whose rate is not known beforehand: it is
measured once per process (`ticks_per_ms`), one sleep between two events on a warm device, and every stall is scaled from that
figure.  Nothing here loops until a delay "is long enough", and no call queues more than MAX_STALL_MS.

A stall that has drained by the time the call under test returns proves nothing, so every test of an asynchronous call asserts
`assert_still_stalled` right behind the call, and every test of a call that blocks by contract asserts `assert_host_was_held`.
profiles/NOTES.md ("stream ordering under a stalled device") has the measured tick rate and why STALL_MS is what it is."""
import time

import torch

STALL_MS = 50.0             # the stall of every test unless it says otherwise
MAX_STALL_MS = 250.0        # no single call queues more
PROBE_TICKS = 1_000_000     # the calibrating sleep: 10 ms at the 100 MHz of a constant-rate counter, 0.4 ms at a 2.4 GHz shader clock
WARM_TICKS = 5 * PROBE_TICKS    # spun right before it: the counter follows the shader clock, and an idle device has let that drop

_TICKS_PER_MS = {}


def ticks_per_ms(device):
    """How many ticks torch.cuda._sleep spins per millisecond on `device`: one probe sleep timed with events on the device's
    default stream, behind a spin of WARM_TICKS that loads the kernel and brings the clock up.  Measured once per process and device."""
    device = torch.device(device)
    key = device.index if device.index is not None else torch.cuda.current_device()
    if key not in _TICKS_PER_MS:
        with torch.cuda.device(key):
            torch.cuda._sleep(WARM_TICKS)               # warm: the spin kernel is loaded, the queue exists, the clock has come up
            torch.cuda.synchronize()
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            torch.cuda._sleep(PROBE_TICKS)
            t1.record()
            t1.synchronize()
            ms = t0.elapsed_time(t1)
        assert 0.05 < ms < MAX_STALL_MS, f"a sleep of {PROBE_TICKS} ticks took {ms} ms: the tick rate cannot be told from that"
        _TICKS_PER_MS[key] = PROBE_TICKS / ms
    return _TICKS_PER_MS[key]


class StallEvent(torch.cuda.Event):
    """The event `stall` returns, recorded right behind the delay; `begin` was recorded right in front of it."""

    def stalled_ms(self):
        """How long the delay really held the stream, measured by the device (synchronises on this event)."""
        self.synchronize()
        return self.begin.elapsed_time(self)


def stall(stream, ms=STALL_MS):
    """Queues a device-side delay of about `ms` milliseconds on `stream`; whatever is queued on it afterwards runs behind the
    delay.  Returns the event recorded right behind the delay: not complete while the stream is still held."""
    assert 0 < ms <= MAX_STALL_MS, f"a stall of {ms} ms: at most {MAX_STALL_MS} ms are queued in one call"
    ticks = int(ms * ticks_per_ms(stream.device))
    begin, end = torch.cuda.Event(enable_timing=True), StallEvent(enable_timing=True)
    with torch.cuda.stream(stream):
        begin.record(stream)
        torch.cuda._sleep(ticks)
        end.record(stream)
    end.begin = begin
    return end


def assert_still_stalled(event, what=""):
    """Right behind an asynchronous call: the stream it was queued on is still held, so nothing of the call has run where it was
    told to run.  If this fails the test has shown nothing -- the stall is too short for what the host does in between."""
    assert not event.query(), f"{what + ': ' if what else ''}the stall had drained when the call returned, so the call was never held to its ordering"


def assert_host_was_held(event, seconds, what=""):
    """Behind a call that blocks by contract and took `seconds` of host time: at least half of the device-measured stall passed
    inside the call (the other half covers what the host did between queueing the stall and entering the call)."""
    ms = event.stalled_ms()
    assert seconds * 1e3 >= 0.5 * ms, f"{what + ': ' if what else ''}the call returned after {seconds * 1e3:.2f} ms on a stream stalled for {ms:.2f} ms"


def timed(fn, *args, **kwargs):
    """(fn's result, the host seconds it took)."""
    t0 = time.perf_counter()
    out = fn(*args, **kwargs)
    return out, time.perf_counter() - t0


def caller_streams(device, n=4):
    """n non-default streams created back to back.  The hardware queues are handed to streams in turn, so one of any four
    consecutive streams may share a queue with the library's side stream or a worker's -- which orders the two by accident and
    hides a missing wait.  Every contract is therefore run once per stream of this list, and holds only if it holds on all."""
    return [torch.cuda.Stream(device=device) for _ in range(n)]
