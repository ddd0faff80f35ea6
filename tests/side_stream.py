"""A lagging side stream for the tests: while `lagging(lib, delay)` is open

  * the current stream is a fresh torch.cuda.Stream() (PyTorch creates these non-blocking: nothing orders it with the null
    stream),
  * every entry of the loaded library object -- every key of every *_SYMBOLS ledger of abnet3_amd/_lib.py -- is wrapped so
    that `delay()` runs on the current stream immediately before the call (and the call is recorded, as
    dirty_memory.recorded records SYMBOLS),
  * `delay()` also runs in front of torch.empty, torch.empty_like, torch.zeros, torch.zeros_like, torch.full and torch.ones,
  * a dirty_memory.dirty(0xFF) window is open inside, so the poison fill of an output is enqueued BEHIND a delay on the side
    stream.

So the side stream always lags the host.  Whatever an entry or its wrapper sends elsewhere -- to the null stream, to a stream
taken earlier, to a stream of its own that does not wait for the caller's -- runs ahead of its producers and ahead of the
poison fill: its output is overwritten with NaN / -1 afterwards, or it is computed from stale intermediates.  Code that keeps
everything on the caller's stream gives exactly the null-stream result.

THE PROPERTY THAT MATTERS: timing can only HIDE a mistake here, it can never fail correct code.  A delay that turns out too
short, a machine that is slow to launch, a stream that drains early: each of them only lets a misplaced operation land in
order by luck.  Nothing correct code does depends on how long a delay lasts.

`delay` is injectable (the host tests pass a counter).  On the GPU it is `gpu_delay()`: torch.cuda._sleep(cycles), with
cycles calibrated once per process by two events around a long _sleep (the way PyTorch's own tests derive cycles per
millisecond).  The delay's length is a condition, not a measurement of the code under test: at least MIN_LATENCIES times the
launch-to-start latency of an empty launch on an idle stream (measured here, at first use, as the host time of launch +
synchronize, an upper bound), and never below MIN_DELAY_MS.

The side stream is picked: the runtime spreads its streams over a few hardware queues, and a stream that shares the null
stream's queue runs in submission order with it, which would hide exactly the mistakes this window is for.  So `lagging`
takes the first fresh stream on which `runs_ahead` sees a null-stream launch finish while the stream is stalled, and says in
`Lag.independent` whether it found one.  Like every matter of timing here, a stream that is not independent can hide a
mistake and fails nothing by itself.

Everything patched comes back on exit, also after an exception and when nested (dirty's guarantee).  The window must never be
open during a hipGraph capture.  A plain helper module: no fixture, not a conftest."""
import contextlib
import time

import torch

from dirty_memory import dirty

LEDGERS = ('SYMBOLS',) + tuple('NEXT%s_SYMBOLS' % n for n in ('', 2, 3, 4, 5, 6, 7)) + ('EVAL_SYMBOLS', 'CAE_SYMBOLS', 'SDTW_SYMBOLS')
ALLOCATORS = ('empty', 'empty_like', 'zeros', 'zeros_like', 'full', 'ones')
MIN_DELAY_MS = 0.5
MIN_LATENCIES = 20


def all_symbols():
    """Every entry name of every ledger of abnet3_amd/_lib.py, in ledger order."""
    from abnet3_amd import _lib
    names = []
    for ledger in LEDGERS:
        names += list(getattr(_lib, ledger))
    assert len(set(names)) == len(names)
    return names


class Lag(object):
    """What `lagging` yields: the side stream (None without a device), the entries called in call order, the delays put in
    front of entries and in front of allocations, dirty's count of poisoned allocations, and whether the null stream was
    seen to run ahead of the stalled side stream (runs_ahead)."""

    def __init__(self):
        self.side, self.calls, self.entry_delays, self.alloc_delays, self.poisoned, self.independent = None, [], 0, 0, None, None

    def __repr__(self):
        return 'Lag(calls=%d, entry_delays=%d, alloc_delays=%d, poisoned=%r)' % (len(self.calls), self.entry_delays, self.alloc_delays,
                                                                                 self.poisoned)


@contextlib.contextmanager
def lagging(lib, delay):
    lag = Lag()
    names = all_symbols()
    saved_entries = {name: getattr(lib, name) for name in names}
    saved_torch = {name: getattr(torch, name) for name in ALLOCATORS}

    def wrap_entry(name, fn):
        def call(*args):
            delay()
            lag.entry_delays += 1
            lag.calls.append(name)
            return fn(*args)
        return call

    def wrap_allocator(fn):
        def call(*args, **kwargs):
            delay()
            lag.alloc_delays += 1
            return fn(*args, **kwargs)
        return call

    with contextlib.ExitStack() as stack:
        if torch.cuda.is_available():
            assert not torch.cuda.is_current_stream_capturing(), 'never open during a graph capture'
            null = torch.cuda.default_stream()
            lag.side, lag.independent = pick_stream(lambda s: runs_ahead(null, s, delay))
            stack.enter_context(torch.cuda.stream(lag.side))
        try:
            for name, fn in saved_entries.items():
                setattr(lib, name, wrap_entry(name, fn))
            for name, fn in saved_torch.items():
                setattr(torch, name, wrap_allocator(fn))
            with dirty(0xFF) as lag.poisoned:            # (it wraps the delayed torch.empty: delay, allocation, poison fill)
                yield lag
        finally:
            for name, fn in saved_torch.items():
                setattr(torch, name, fn)
            for name, fn in saved_entries.items():
                setattr(lib, name, fn)


def runs_ahead(free, stalled, delay):
    """True when a tiny launch on the stream `free` completes while the stream `stalled` is still held by one delay().  The
    runtime spreads its streams over a few hardware queues (GPU_MAX_HW_QUEUES), and two streams that share one run in the
    order of their submissions: between such a pair a misplaced operation lands in order by luck.  Costs one delay."""
    stalled.synchronize()
    free.synchronize()
    behind, ahead = torch.cuda.Event(), torch.cuda.Event()
    with torch.cuda.stream(stalled):
        delay()
        behind.record()
    with torch.cuda.stream(free):
        torch.cuda._sleep(1)
        ahead.record()
    ahead.synchronize()
    ahead_first = not behind.query()
    stalled.synchronize()
    return ahead_first


def pick_stream(ok, tries=8):
    """(a fresh torch.cuda.Stream() that passes ok(stream), True): the first of at most `tries` streams of torch's pool (which
    hands them out in turn: no stream is created beyond those the pool holds anyway); only the picked one is used.  (the
    last one tried, False) when none passes: correct code must not fail over that, a detector may."""
    for _ in range(tries):
        s = torch.cuda.Stream()
        if ok(s):
            return s, True
    print('side_stream: none of %d fresh streams ran independently of its counterpart (one hardware queue?): ordering mistakes '
          'between the two can hide' % tries)
    return s, False


_CALIBRATION = {}


def calibration():
    """{'cycles_per_ms', 'launch_latency_ms', 'delay_ms', 'delay_cycles'}, measured once per process on the current device and
    printed once.  Both measurements are medians; the latency is the host time from launching an empty _sleep on an idle
    stream to the end of its synchronize, which bounds the launch-to-start latency from above."""
    if _CALIBRATION:
        return _CALIBRATION
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        torch.cuda._sleep(1000)
        s.synchronize()
        rates = []
        for _ in range(3):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            torch.cuda._sleep(2000000)
            b.record()
            b.synchronize()
            rates.append(2000000 / a.elapsed_time(b))
        lat = []
        for _ in range(21):
            s.synchronize()
            t0 = time.perf_counter()
            torch.cuda._sleep(1)
            s.synchronize()
            lat.append((time.perf_counter() - t0) * 1e3)
    rate, latency = sorted(rates)[1], sorted(lat)[10]
    delay_ms = max(MIN_DELAY_MS, MIN_LATENCIES * latency)
    _CALIBRATION.update(cycles_per_ms=rate, launch_latency_ms=latency, delay_ms=delay_ms, delay_cycles=int(delay_ms * rate) + 1)
    print('side_stream: %.0f cycles per ms, empty launch %.4f ms, delay %.3f ms = %d cycles' % (
        rate, latency, delay_ms, _CALIBRATION['delay_cycles']))
    return _CALIBRATION


def gpu_delay():
    """delay() for the GPU: one calibrated torch.cuda._sleep on the current stream."""
    cycles = calibration()['delay_cycles']
    return lambda: torch.cuda._sleep(cycles)
