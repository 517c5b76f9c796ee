"""A gate for stream-ordering tests (tests/test_gpu_stream_order.py): it makes work that the library queues on the WRONG stream fail
deterministically, so that no test depends on a race being lost by luck.

``include/nutls.h`` promises that the device entries are asynchronous on the stream they are given and that calls on one handle take
effect in the order they are made.  A launch, copy or zeroing that goes to another stream (NULL, the handle's private stream, a chunk
stream without its event) is invisible as long as every call is followed by a synchronisation on the legacy default stream.  Here a
sequence of calls runs on a fresh non-blocking side stream behind a GATE:

  1. ``torch.cuda._sleep(cycles)`` is queued on the side stream (a bounded spin: nothing can hang);
  2. a marker event is recorded behind it;
  3. the copies that put the REAL inputs, masks and counts into the buffers the calls were given are queued behind the marker -- until
     they run the buffers hold POISON (NaN; 0x7fff / 0x8000 int16; 0xff bytes in masks and counts), the outputs a sentinel;
  4. the library calls of the sequence are made with no host synchronisation between them;
  5. the host synchronises only at the end.

Whatever the library queued elsewhere runs during the sleep, on poison or on stale state; NaN in the model state never heals until
``nutls_reset`` (tests/test_gpu_poison.py holds that it does then, and that it never reaches another row), so the
comparison with the synchronous run of the same sequence (``Seq(gated=False)``: default stream, a synchronisation after every call)
sees it.  A gated run counts only if the marker is still incomplete when the last non-blocking call of the sequence has returned
(``Seq.check_held``, called by ``Seq.close`` or by the test just before the first host-blocking call): otherwise the run fails with
"gate opened early, inconclusive" -- it is never skipped or repeated.

The sleep is calibrated once per process against the GPU's event clock (``calibrate``), never against the code under test.

The side streams come from ``side_streams``: the runtime serves all HIP streams of a process from a few hardware queues (four by
default), and two streams that share one run in order whatever their flags say.  A side stream that shares its queue with the NULL
stream would make every synchronous NULL-stream operation of the library (the zeroing of a lazily allocated buffer, a table upload) wait
for the gate -- the gate "opens early" although nothing is wrong.  So the gated streams are chosen once per process among fresh torch
streams by the premise itself: while the candidate sleeps, a tiny copy on the NULL stream (and on the streams chosen before it) must
complete.  The same sharing can hide a fault -- a launch on a wrong stream that happens to share the gated stream's queue waits for the
gate like a correct one; the library's own streams cannot be seen from here, so each path is exercised by several cases.
Nothing here touches the GPU at import."""
import numpy as np

TARGET_MS = 250.0            # length of a gate
CAL_CYCLES = 2_000_000       # the first calibration sleep
MAX_GATE_MS = 2000.0         # a calibration that gives a longer gate than this is refused
SENTINEL = {"float32": -7777.0, "int16": 0x1234, "uint8": 0x5a, "int32": 0x5a5a5a5a}

_cycles = None


def _timed_sleep(torch, cycles):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    torch.cuda._sleep(int(cycles))
    b.record()
    b.synchronize()
    return float(a.elapsed_time(b))


def calibrate():
    """Cycles of ``torch.cuda._sleep`` that last TARGET_MS on this GPU: a CAL_CYCLES sleep is timed between two events on the idle default
    stream and scaled; where that sleep was too short for its launch not to matter (< 5 ms) a second one, scaled to 25 ms, is timed and
    scaled instead.  The resulting gate is then timed once itself and must lie in [TARGET_MS / 2, MAX_GATE_MS]."""
    global _cycles
    if _cycles is not None:
        return _cycles
    import torch
    torch.cuda.synchronize()
    _timed_sleep(torch, CAL_CYCLES)                  # (first launch of the sleep kernel: not timed)
    ms = _timed_sleep(torch, CAL_CYCLES)
    cycles, used = CAL_CYCLES, ms
    if ms < 5.0:
        cycles = int(CAL_CYCLES * 25.0 / max(ms, 1e-3))
        assert cycles < (1 << 40), "stream gate: a %d-cycle sleep took %.4f ms: the sleep does not scale" % (CAL_CYCLES, ms)
        used = _timed_sleep(torch, cycles)
    gate = int(cycles * TARGET_MS / max(used, 1e-3))
    assert gate < (1 << 44), "stream gate: calibration gives %d cycles" % gate
    got = _timed_sleep(torch, gate)
    print("stream gate calibration: %d cycles took %.3f ms, %d cycles took %.3f ms -> %d cycles for %.0f ms, measured %.1f ms"
          % (CAL_CYCLES, ms, cycles, used, gate, TARGET_MS, got))
    assert TARGET_MS / 2 <= got <= MAX_GATE_MS, "stream gate: the calibrated gate lasts %.1f ms, wanted about %.0f" % (got, TARGET_MS)
    _cycles = gate
    return gate


_streams = None


def _independent(torch, busy, probes, cycles):
    """While ``busy`` sleeps, a tiny copy on every stream of ``probes`` completes: none of them waits for it."""
    src, dst = torch.ones(16, device="cuda"), torch.zeros(16, device="cuda")
    torch.cuda.synchronize()
    with torch.cuda.stream(busy):
        torch.cuda._sleep(cycles)
        marker = torch.cuda.Event()
        marker.record()
    ok = True
    for p in probes:
        with torch.cuda.stream(p):
            dst.copy_(src)
            done = torch.cuda.Event()
            done.record()
        done.synchronize()
        ok = ok and not marker.query()
    torch.cuda.synchronize()
    return ok


def side_streams():
    """Two torch side streams that wait neither for the NULL stream's work nor for each other's (see the module's docstring), chosen once
    per process among at most 16 fresh ones with a sleep of a tenth of a gate each."""
    global _streams
    if _streams is not None:
        return _streams
    import torch
    cycles = max(1, calibrate() // 10)
    found, tried = [], 0
    while len(found) < 2 and tried < 16:
        cand = torch.cuda.Stream()
        tried += 1
        if _independent(torch, cand, [torch.cuda.default_stream()] + found, cycles):
            found.append(cand)
    print("stream gate: %d of %d fresh side streams run beside the NULL stream and each other" % (len(found), tried))
    assert len(found) == 2, "stream gate: no two side streams that run beside the NULL stream among %d fresh ones" % tried
    _streams = found
    return found


def poison_(t):
    """Fill a device tensor with poison in place: NaN (float), alternating 0x7fff / 0x8000 (int16), 0xff bytes (uint8 masks, int32 counts)."""
    import torch
    if t.dtype == torch.float32:
        t.fill_(float("nan"))
    elif t.dtype == torch.int16:
        flat = t.view(-1)
        flat[0::2] = 0x7fff
        flat[1::2] = -0x8000
    elif t.dtype == torch.uint8:
        t.fill_(0xff)
    elif t.dtype == torch.int32:
        t.fill_(-1)
    else:
        raise TypeError("no poison for %s" % t.dtype)
    return t


class Seq:
    """One run of a call sequence.  ``gated=False`` (S): the legacy default stream, a device synchronisation after every call.
    ``gated=True`` (G): a side stream (``side_streams``) behind a gate, no synchronisation before ``close``.

        q = Seq(gated)
        x = q.input(array)            # device tensor: the real values (S) / poison until the gate opens (G)
        o = q.output(shape, dtype)    # device tensor full of a sentinel
        q.open()
        with q:                       # the run's stream is torch's current stream
            q.call(eng.step, x, out=o)
        q.close()                     # G: asserts that the gate held, then synchronises
    """

    def __init__(self, gated, name="", slot=0):
        """``slot``: which of the two ``side_streams`` a gated run takes (two gated runs side by side: 0 and 1)."""
        import torch
        self.torch, self.gated, self.name = torch, bool(gated), name
        self.stream = side_streams()[slot] if gated else torch.cuda.default_stream()
        self.marker, self.held, self._staged, self._ctx = None, None, [], None

    def input(self, array):
        torch = self.torch
        src = torch.from_numpy(np.ascontiguousarray(array)).cuda()
        if not self.gated:
            return src
        dst = poison_(torch.empty_like(src))
        self._staged.append((dst, src))
        return dst

    def output(self, shape, dtype="float32"):
        torch = self.torch
        return torch.full(tuple(shape), SENTINEL[dtype], dtype=getattr(torch, dtype), device="cuda")

    def open(self, sync=True):
        """Queue the gate: sleep, marker, then the copies of the real inputs.  ``sync=False``: a second gate beside one that is already
        queued (two gated streams): the device is not synchronised first."""
        torch = self.torch
        if sync:
            torch.cuda.synchronize()
        if not self.gated:
            return
        cycles = calibrate()
        with torch.cuda.stream(self.stream):
            torch.cuda._sleep(cycles)
            self.marker = torch.cuda.Event()
            self.marker.record()
            for dst, src in self._staged:
                dst.copy_(src, non_blocking=True)

    def __enter__(self):
        self._ctx = self.torch.cuda.stream(self.stream)
        self._ctx.__enter__()
        return self

    def __exit__(self, *exc):
        ctx, self._ctx = self._ctx, None
        return ctx.__exit__(*exc)

    def call(self, fn, *args, **kwargs):
        res = fn(*args, **kwargs)
        if not self.gated:
            self.torch.cuda.synchronize()
        return res

    def check_held(self):
        """The condition of a gated run: the marker has not completed yet.  Checked once -- when the last non-blocking call has returned,
        or just before the first host-blocking call of the sequence."""
        if not self.gated or self.held is not None:
            return
        self.held = not self.marker.query()
        assert self.held, "gate opened early, inconclusive (%s): the marker had completed before the calls of the sequence were made" % self.name
        print("gate held (%s)" % self.name)

    def close(self):
        self.check_held()
        self.torch.cuda.synchronize()


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def assert_same(sync, gated, what):
    """Every result of the gated run equals the synchronous run's bit for bit; the message names the first that does not, and whether
    it is non-finite, still the sentinel, or different."""
    assert sorted(sync) == sorted(gated), (what, sorted(sync), sorted(gated))
    for key in sorted(sync):
        s, g = np.asarray(sync[key]), np.asarray(gated[key])
        if same_bits(s, g):
            continue
        kind = "differs"
        if g.dtype.kind == "f" and not np.isfinite(g).all():
            kind = "is not finite (%d of %d values)" % (int((~np.isfinite(g)).sum()), g.size)
        elif g.dtype.name in SENTINEL and (g == np.asarray(SENTINEL[g.dtype.name], g.dtype)).any():
            kind = "still holds the sentinel in %d of %d values" % (int((g == np.asarray(SENTINEL[g.dtype.name], g.dtype)).sum()), g.size)
        else:
            kind = "differs in %d of %d values" % (int((s.reshape(-1).view(np.uint8) != g.reshape(-1).view(np.uint8)).sum()), s.nbytes)
        raise AssertionError("%s: '%s' of the gated run %s" % (what, key, kind))
