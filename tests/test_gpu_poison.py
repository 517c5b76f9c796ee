"""Non-finite input on a LIVE row stays contained and heals (include/nutls.h, "Non-finite input"), for every kernel family.

One handle serves many callers: a workgroup steps two or four streams side by side, a per-layer tile of 128 positions spans several
streams, in block mode a tile spans frames and utterances, a stereo frame row carries two talkers, the corpus scheduler reuses a slot.  The
rest of the suite shows bit for bit that partners and slots do not matter for FINITE data, and that a held row may hold NaN.  A leak that
is multiplied by zero -- a halo row, a zero-padded weight column, a masked reduction across lanes, a K split summed over waves -- is
0 * x = 0 there and invisible; with NaN or Inf it is NaN.  And a reset that "zeroes" by scaling, or misses a carried sum, a ring slot, a
resampler tail or a follow energy, passes every reset test that starts from finite state and keeps a stream dead for ever after one bad hop.

Every test makes two runs of one configuration -- poisoned, and the clean twin that feeds the bad row zeros (tests/poison_reference.py) --
plus a fresh handle for the healing part, and every comparison is ``np.array_equal`` / ``torch.equal`` or a finiteness check:
  1. containment across rows: every other row of the poisoned run equals the clean twin's, outputs at every frame and all states;
  2. containment in time (block entries): the poisoned utterance's outputs before the poison equal the clean run's;
  3. the stateless halves change only inside the windows of tests/poison_reference.py (shown right against float64 by
     tests/test_poison_reference.py) and are finite again behind them;
  4. healing: after ``reset(b)`` row b equals the same row of a fresh handle fed the same continuation.
The clean twin's neighbours are non-zero, and once per plan within ``WF.OUT_BOUND`` of the float64 oracle: what is compared is the real
function.  What the poisoned row itself returns is not specified (point 5) and not asserted, except that the poison did arrive.

The frame script: 3 clean frames, poison at frames 3 and 4 (the edge poison through its other position), a clean frame, ``reset(b)``
before frame 6, 6 more frames -- in the causal 32-frame mode every sum reads all 31 ring slots, so one slot that kept its NaN shows."""
import ctypes
import functools

import numpy as np
import pytest
import torch      # (before the first handle: torch must bring up the HIP runtime it ships with itself)

import poison_reference as P
import weight_families as WF
from nunet_amd import NutlsEngine, NutlsOffline, runner
from nunet_amd.runner import plan_ragged_blocks
from nunet_amd.weights import parse_blob
from oracle.nutls_ref import NutlsRef

pytestmark = pytest.mark.gpu

FRAMES = 12
BAD = (3, 4)               # the poisoned frames
RESET = 6                  # reset(row) in front of this frame
SNAPS = (5, FRAMES - 1)    # all states are read after these frames
ORACLE_FRAMES = 3          # the clean frames in front of the poison, the same in every run: these are held against float64
TILE_MIN = "NUTLS_CONV_TILE_MIN"
FP32 = "NUTLS_OFFLINE_FP32"


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.cpu().numpy().copy()


@functools.lru_cache(maxsize=None)
def mags():
    """[FRAMES, 8, 256] float32, read-only: eight noise rows, each of its own draw and level."""
    level = np.float32([0.25, 0.1, 0.5, 0.05, 0.3, 0.15, 0.4, 0.2])
    x = np.stack([level[b] * np.abs(np.random.default_rng([41, b]).standard_normal((FRAMES, 256))) for b in range(8)], axis=1).astype(np.float32)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def waves():
    """[FRAMES, 8, 256] float32, read-only: eight rows of noise at speech level, hop by hop."""
    level = np.float32([0.05, 0.02, 0.1, 0.01, 0.06, 0.03, 0.08, 0.04])
    x = np.stack([level[b] * np.random.default_rng([43, b]).standard_normal((FRAMES, 256)) for b in range(8)], axis=1).astype(np.float32)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def oracle_out(variant, ctfa_mode):
    """Rows 0 .. 3 of ``mags()``, frames 0 .. ORACLE_FRAMES - 1, through the float64 oracle on the container the handles run (computed once)."""
    blob = None if variant == "lstm" else parse_blob(WF.container("plain", variant="baseline"))
    ref = NutlsRef(blob, batch=4, ctfa_mode=ctfa_mode, variant=variant, dtype=torch.float64)
    out = np.stack([ref.step(mags()[f, :4]).numpy().astype(np.float64) for f in range(ORACLE_FRAMES)])
    out.setflags(write=False)
    return out


def check_oracle(out, rows, variant="lstm", ctfa_mode="frame"):
    """``out [frames, B, 256]`` of a clean twin: the rows ``rows`` (< 4) within WF.OUT_BOUND of float64 on the frames in front of the poison."""
    want = oracle_out(variant, ctfa_mode)
    rows = [b for b in rows if b < 4]
    assert rows
    for f in range(ORACLE_FRAMES):
        for b in rows:
            r = WF.scaled_rms(out[f, b], want[f, b]) / WF.OUT_BOUND
            assert r < 1.0, "clean twin, frame %d row %d: %.3g x OUT_BOUND from the float64 oracle" % (f, b, r)


class Run:
    def __init__(self, out, snaps, extra=None):
        self.out, self.snaps, self.extra = out, snaps, extra or {}


def states_of(h, variant="lstm"):
    return {n: h.state_get(n) for n in WF.state_names(variant)}


def script(make, x, row, step, variant="lstm", extra=None):
    """The frame script on a new handle: ``x [FRAMES, B, n]`` frame by frame through ``step(handle, frame) -> [B, n]`` numpy, ``reset(row)``
    in front of frame RESET, all states after the frames of SNAPS (``extra(handle)``: more per-row library state, read with them)."""
    h = make()
    outs, snaps, ex = [], {}, {}
    for f in range(x.shape[0]):
        if f == RESET:
            h.reset(row)
        outs.append(step(h, x[f]))
        if f in SNAPS:
            snaps[f] = states_of(h, variant)
            if extra is not None:
                ex[f] = extra(h)
    h.close()
    return Run(np.stack(outs), snaps, ex)


def fresh_run(make, x, step, variant="lstm", extra=None):
    """A fresh handle of the same configuration fed the continuation, frames RESET .. of ``x``."""
    h = make()
    outs = [step(h, x[f]) for f in range(RESET, x.shape[0])]
    snap = states_of(h, variant)
    ex = extra(h) if extra is not None else None
    h.close()
    return Run(np.stack(outs), {FRAMES - 1: snap}, {FRAMES - 1: ex})


def same(a, b):
    return np.array_equal(a, b, equal_nan=False) and a.dtype == b.dtype


def check_script(what, bad, clean, fresh, row, B, live_from=0):
    """Points 1 and 4 on one poisoned run against its clean twin and the fresh handle.  ``live_from``: the first frame whose output carries
    signal (the gateway's first packets are its priming silence and its lag)."""
    others = [b for b in range(B) if b != row]
    for b in others:
        assert clean.out[live_from:, b].any(axis=-1).all(), "%s: the clean twin's row %d has an all-zero output frame" % (what, b)
        for f in range(bad.out.shape[0]):
            assert same(bad.out[f, b], clean.out[f, b]), "%s: output of row %d differs from the clean twin's at frame %d (row %d poisoned at %s)" % (
                what, b, f, row, BAD)
    assert not np.isfinite(bad.out[BAD[0]:RESET, row]).all(), "%s: the poison did not arrive in row %d" % (what, row)
    for f in SNAPS:
        for n, v in bad.snaps[f].items():
            assert same(v[others], clean.snaps[f][n][others]), "%s: state %s of another row differs from the clean twin's after frame %d" % (what, n, f)
        for k in bad.extra.get(f) or {}:
            assert same(np.asarray(bad.extra[f][k])[others], np.asarray(clean.extra[f][k])[others]), "%s: %s of another row differs after frame %d" % (what, k, f)
    # healing: the reset row against the same row of the fresh handle
    assert np.isfinite(bad.out[RESET:, row]).all(), "%s: row %d is not finite after its reset" % (what, row)
    for f in range(RESET, bad.out.shape[0]):
        assert same(bad.out[f, row], fresh.out[f - RESET, row]), "%s: row %d, %d frames after its reset, differs from a fresh handle's" % (what, row, f - RESET)
    last = FRAMES - 1
    for n, v in bad.snaps[last].items():
        assert same(v[row], fresh.snaps[last][n][row]), "%s: state %s of the reset row differs from a fresh handle's" % (what, n)
    for k in (bad.extra.get(last) or {}):
        assert same(np.asarray(bad.extra[last][k])[row], np.asarray(fresh.extra[last][k])[row]), "%s: %s of the reset row differs from a fresh handle's" % (what, k)


def poison_rounds(make, x, rows, step, B, what, variant="lstm", extra=None, oracle=None, kinds=P.KINDS):
    """For every row of ``rows`` in turn: the clean twin, then the three poisons; one fresh handle for all (its rows do not depend on each
    other, or the comparison fails).  ``oracle``: (variant, ctfa_mode) -- the first clean twin is held against float64."""
    fresh = fresh_run(make, x, step, variant, extra)
    for i, row in enumerate(rows):
        clean = script(make, P.clean_twin(x, row, BAD), row, step, variant, extra)
        if oracle is not None and i == 0:
            check_oracle(clean.out, [b for b in range(B) if b != row], *oracle)
        for kind in kinds:
            bad = script(make, P.poisoned(x, row, BAD, kind), row, step, variant, extra)
            check_script("%s, row %d, %s" % (what, row, kind), bad, clean, fresh, row, B)


def step_device(h, frame):
    return host(h.step(dev(frame)))


def step_host(h, frame):
    return h.step(np.ascontiguousarray(frame)).copy()


def hop_device(h, frame):
    return host(h.enhance_hop(dev(frame)))


def hop_host(h, frame):
    return h.enhance_hop(np.ascontiguousarray(frame)).copy()


# ---- a. the fused step, LSTM variant, shipped container ------------------------------------------------------------------------------------
FUSED = [(spw, B, "frame", False, slot) for spw, B in ((1, 3), (2, 4), (4, 8)) for slot in range(spw)]
FUSED += [(spw, B, "causal32", False, slot) for spw, B in ((1, 3), (2, 4)) for slot in range(spw)]
FUSED += [(1, 3, "frame", True, 0)]


@pytest.mark.parametrize("spw,B,ctfa,trace,slot", FUSED, ids=["plan%d-B%d-%s%s-slot%d" % (s, b, c, "-trace" if t else "", k) for s, b, c, t, k in FUSED])
def test_fused_step_contains_and_heals(spw, B, ctfa, trace, slot):
    """One-, two- and four-stream plans (B = 3; 4: two workgroups; 8), each slot of workgroup 0 poisoned in turn: the workgroup's other slots
    and the other workgroup are bit-clean, the reset row is bit-fresh.  causal32: the 32-frame ring hands no NaN slot to the sums after
    the reset.  ``debug_trace``: the profiling build."""
    def make():
        e = NutlsEngine(batch=B, streams_per_workgroup=spw)
        assert e.mode == "fused" and e.streams_per_workgroup == spw
        if ctfa != "frame":
            e.set_ctfa_mode(ctfa)
        if trace:
            e.debug_trace(True)
        return e

    x = np.ascontiguousarray(mags()[:, :B])
    poison_rounds(make, x, [slot], step_device, B, "fused step, %d-stream plan, %s%s" % (spw, ctfa, ", profiling build" if trace else ""),
                  oracle=("lstm", ctfa) if slot == 0 else None)


# ---- b. the baseline variant -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["fused", "launches", "graph"])
def test_baseline_contains_and_heals(mode):
    """The dilated-dense baseline on its plain synthetic container, B = 3, fused plan and per-layer modes 0 and 1: its history rings sit at
    a slot derived from the handle's frame counter, the reset row's are zeros at every slot."""
    B, blob = 3, WF.container("plain", variant="baseline")
    make = lambda: NutlsEngine(blob, batch=B, variant="baseline", mode=mode)
    poison_rounds(make, np.ascontiguousarray(mags()[:, :B]), [1], step_device, B, "baseline, mode %s" % mode, variant="baseline",
                  oracle=("baseline", "frame"))


# ---- c. the per-layer kernels, LSTM variant --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode,forced", [("launches", False), ("graph", False), ("graph", True)])
def test_per_layer_kernels_contain_and_heal(mode, forced, monkeypatch):
    """Modes 0 and 1 (graph replay) at B = 3, the middle stream poisoned; once on the forced 128-position tiles (the knob of
    tests/test_gpu_conv_variants.py), where a tile really spans all three streams."""
    B = 3

    def make():
        if forced:
            monkeypatch.setenv(TILE_MIN, "0")
        try:
            e = NutlsEngine(batch=B, mode=mode)
        finally:
            monkeypatch.delenv(TILE_MIN, raising=False)
        if forced:
            assert all(p["family"].endswith("/w4") for p in e.launch_plan() if p["family"].startswith("conv_"))
        return e

    poison_rounds(make, np.ascontiguousarray(mags()[:, :B]), [1], step_device, B, "per-layer kernels, mode %s%s" % (mode, ", forced tiles" if forced else ""),
                  oracle=("lstm", "frame"))


# ---- d. the hop entries ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fusion", [False, True])
@pytest.mark.parametrize("spw,B", [(1, 3), (2, 4)])
def test_hop_entries_contain_and_heal(spw, B, fusion):
    """``enhance_hop`` as three launches and as one (``hop_fusion``), one- and two-stream plans, waveform samples of one row poisoned: the
    previous hop, the overlap tail and the phasors of the other rows never see them, and the reset row's are zeros again."""
    make = lambda: NutlsEngine(batch=B, streams_per_workgroup=spw, hop_fusion=fusion)
    x = np.ascontiguousarray(waves()[:, :B])
    h = make()
    assert h.launches_per_hop == (1 if fusion else 3)
    h.close()
    poison_rounds(make, x, [1], hop_device, B, "enhance_hop, %d-stream plan, %s" % (spw, "one launch" if fusion else "three launches"))


def test_host_entries_contain_and_heal():
    """One hop poisoned through the ``_host`` entry (pageable arrays), and a frame through ``nutls_step_host``."""
    B = 3
    make = lambda: NutlsEngine(batch=B)
    poison_rounds(make, np.ascontiguousarray(waves()[:, :B]), [0], hop_host, B, "enhance_hop_host", kinds=("nan", "inf"))
    poison_rounds(make, np.ascontiguousarray(mags()[:, :B]), [2], step_host, B, "step_host", kinds=("nan",))


# ---- e. block mode -----------------------------------------------------------------------------------------------------------------------------
U, MAXF, CALLS, BAD_UTT, BAD_FRAME = 3, 24, (24, 7, 24), 1, 13
RAGGED = (24, 24, 9)


@functools.lru_cache(maxsize=None)
def block_mags():
    """[U, 55, 256] float32: the three calls' frames of three utterances."""
    n = sum(CALLS)
    level = np.float32([0.25, 0.1, 0.4])
    x = np.stack([level[u] * np.abs(np.random.default_rng([47, u]).standard_normal((n, 256))) for u in range(U)]).astype(np.float32)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def block_waves():
    n = sum(CALLS) * 256
    level = np.float32([0.05, 0.02, 0.08])
    x = np.stack([level[u] * np.random.default_rng([49, u]).standard_normal(n) for u in range(U)]).astype(np.float32)
    x.setflags(write=False)
    return x


def block_poisoned(x, kind, unit):
    """Utterance BAD_UTT, frame (hop) BAD_FRAME of the first call, ``unit`` values per frame."""
    out = np.array(x)
    a = BAD_FRAME * unit
    out[BAD_UTT, a:a + unit] = P.poison(out[BAD_UTT, a:a + unit].reshape(-1), kind, "last").reshape(out[BAD_UTT, a:a + unit].shape)
    return out


def block_twin(x, unit):
    out = np.array(x)
    out[BAD_UTT, BAD_FRAME * unit:(BAD_FRAME + 1) * unit] = 0.0
    return out


def offline_states(off):
    return {n: off.state_get(n) for n in WF.state_names()}


def block_script(make, x, unit, call, counts=None, fresh=False):
    """The three calls on a new handle (``fresh``: the third alone); ``reset_utterance(BAD_UTT)`` in front of the third.  ``call(off, block,
    counts) -> [U, n * unit...]`` numpy; ``counts``: ragged counts of the FIRST call.  -> ([outputs per call], [states after calls 2 and 3])."""
    off = make()
    outs, snaps, a = [], [], 0
    for k, n in enumerate(CALLS):
        blk = np.ascontiguousarray(x[:, a * unit:(a + n) * unit])
        a += n
        if k < 2 and fresh:
            continue
        if k == 2 and not fresh:
            off.reset_utterance(BAD_UTT)
        outs.append(call(off, blk, counts if k == 0 else None))
        if k >= 1:
            snaps.append(offline_states(off))
    off.close()
    return outs, snaps


def check_block(what, bad, clean, fresh, unit, counts=None):
    (bo, bs), (co, cs), (fo, fs) = bad, clean, fresh
    others = [u for u in range(U) if u != BAD_UTT]
    for k in range(3):
        for u in others:
            n = CALLS[k] if counts is None or k else counts[u]
            assert co[k][u][:n * unit].any(), "%s: the clean twin's utterance %d is all zero in call %d" % (what, u, k)
            assert same(bo[k][u], co[k][u]), "%s: utterance %d differs from the clean twin's in call %d" % (what, u, k)
    # containment in time: the poisoned utterance before the poison
    assert same(bo[0][BAD_UTT][:BAD_FRAME * unit], co[0][BAD_UTT][:BAD_FRAME * unit]), "%s: utterance %d differs BEFORE its poisoned frame %d" % (
        what, BAD_UTT, BAD_FRAME)
    assert not np.isfinite(bo[0][BAD_UTT][BAD_FRAME * unit:]).all() and not np.isfinite(bo[1][BAD_UTT]).all(), "%s: the poison did not arrive" % what
    for i in range(2):
        for n in bs[i]:
            assert same(bs[i][n][others], cs[i][n][others]), "%s: state %s of another utterance differs after call %d" % (what, n, i + 1)
    # healing
    assert np.isfinite(bo[2][BAD_UTT]).all() and same(bo[2][BAD_UTT], fo[0][BAD_UTT]), "%s: utterance %d after reset_utterance differs from a fresh handle's" % (what, BAD_UTT)
    for n in bs[1]:
        assert same(bs[1][n][BAD_UTT], fs[0][n][BAD_UTT]), "%s: state %s of the reset utterance differs from a fresh handle's" % (what, n)


def call_process(off, blk, counts):
    return host(off.process_block_device(dev(blk.reshape(U, -1, 256)), frames=None if counts is None else np.asarray(counts, np.int32))).reshape(U, -1)


def call_process_ragged_host(off, blk, counts):
    """``process_ragged`` (the _host entry): lists of [n_u, 256]; the rows behind a count come back as zeros here, as the device entry writes them."""
    blk = blk.reshape(U, -1, 256)
    cnt = [blk.shape[1]] * U if counts is None else counts
    got = off.process_ragged([blk[u, :cnt[u]] for u in range(U)])
    out = np.zeros_like(blk)
    for u in range(U):
        out[u, :cnt[u]] = got[u]
    return out.reshape(U, -1)


def call_enhance(off, blk, counts):
    return host(off.enhance_block_device(dev(blk), hops=None if counts is None else np.asarray(counts, np.int32)))


OFFLINE = [(c, p, n) for c in ("frame", "causal32") for p in ("bf16", "fp32") for n in (1, 2)]


def make_offline(ctfa, pipe, chunks, monkeypatch):
    def make():
        if pipe == "fp32":
            monkeypatch.setenv(FP32, "1")
        else:
            monkeypatch.delenv(FP32, raising=False)
        try:
            return NutlsOffline(max_frames=MAXF, utterances=U, ctfa_mode=ctfa, pipeline=chunks)
        finally:
            monkeypatch.delenv(FP32, raising=False)
    return make


@pytest.mark.parametrize("ctfa,pipe,chunks", OFFLINE, ids=["%s-%s-pipeline%d" % c for c in OFFLINE])
def test_block_mode_contains_in_rows_and_in_time_and_heals(ctfa, pipe, chunks, monkeypatch):
    """Three utterances x 24 frames: a tile of the block's launches spans frames and utterances.  Calls of 24, 7 and 24 frames, utterance 1
    poisoned at frame 13 of the first: utterances 0 and 2 bit-clean in all three calls, utterance 1 bit-clean in frames 0 .. 12,
    ``reset_utterance(1)`` before the third call gives a fresh handle's bits."""
    make = make_offline(ctfa, pipe, chunks, monkeypatch)
    x = block_mags().reshape(U, -1)
    clean = block_script(make, block_twin(x, 256), 256, call_process)
    fresh = block_script(make, x, 256, call_process, fresh=True)
    if (ctfa, chunks) == ("frame", 1):          # the real function: utterance 0's first frames against the float64 oracle of the streaming model
        want = oracle_block()
        for f in range(ORACLE_FRAMES):
            r = WF.scaled_rms(clean[0][0][0].reshape(-1, 256)[f], want[f]) / WF.OUT_BOUND
            assert r < 1.0, "block mode (%s), frame %d: %.3g x OUT_BOUND from the float64 oracle" % (pipe, f, r)
    for kind in P.KINDS:
        bad = block_script(make, block_poisoned(x, kind, 256), 256, call_process)
        check_block("process_block, %s, %s, pipeline %d, %s" % (ctfa, pipe, chunks, kind), bad, clean, fresh, 256)


@functools.lru_cache(maxsize=None)
def oracle_block():
    ref = NutlsRef(batch=1, dtype=torch.float64)
    return np.stack([ref.step(block_mags()[0:1, f]).numpy().astype(np.float64)[0] for f in range(ORACLE_FRAMES)])


@pytest.mark.parametrize("ctfa", ["frame", "causal32"])
def test_ragged_blocks_contain_and_heal(ctfa, monkeypatch):
    """``process_ragged`` with counts (24, 24, 9): the poisoned frame lies inside its count, the gather of the carried state takes
    utterance 2 from frame 9 of a block whose tile holds utterance 1's frame 13."""
    make = make_offline(ctfa, "bf16", 1, monkeypatch)
    x = block_mags().reshape(U, -1)
    clean = block_script(make, block_twin(x, 256), 256, call_process_ragged_host, counts=RAGGED)
    # the fresh handle's third call does not depend on the first call's counts
    fresh = block_script(make, x, 256, call_process_ragged_host, fresh=True)
    for kind in P.KINDS:
        bad = block_script(make, block_poisoned(x, kind, 256), 256, call_process_ragged_host, counts=RAGGED)
        check_block("process_ragged %s, %s, %s" % (RAGGED, ctfa, kind), bad, clean, fresh, 256, counts=RAGGED)


@pytest.mark.parametrize("ctfa", ["frame", "causal32"])
def test_waveform_blocks_contain_in_rows_and_in_time_and_heal(ctfa, monkeypatch):
    """``enhance_block`` with waveform poison in hop 13 of utterance 1: output hops 0 .. 12 of that utterance -- samples 0 .. 13 * 256 - 1 --
    are bit-clean (include/nutls.h, "Non-finite input", 2: output hop t is the first that may differ)."""
    make = make_offline(ctfa, "bf16", 1, monkeypatch)
    x = block_waves()
    clean = block_script(make, block_twin(x, 256), 256, call_enhance)
    fresh = block_script(make, x, 256, call_enhance, fresh=True)
    for kind in P.KINDS:
        bad = block_script(make, block_poisoned(x, kind, 256), 256, call_enhance)
        check_block("enhance_block, %s, %s" % (ctfa, kind), bad, clean, fresh, 256)


# ---- f. the stateless halves -------------------------------------------------------------------------------------------------------------------
HB, HOPS, HROW, HHOP = 3, 8, 1, 2          # rows, hops, the poisoned row and hop of the halves' tests
UPPER_HOPS = 10          # with follow a sample at the end of hop 2 reaches the output hops 2 .. 8 (W + 1 = 5 hops behind decoded hop 3): one clean hop behind
SAMPLES = (("first", np.nan), ("last", np.nan), ("first", np.inf), ("last", np.inf))


def _hip():
    for name in ("libamdhip64.so", "/opt/rocm/lib/libamdhip64.so"):
        try:
            return ctypes.CDLL(name)
        except OSError:
            continue
    raise RuntimeError("libamdhip64.so not loadable through ctypes")


def one_sample(x, unit, edge, value):
    """``x [rows, hops * unit]`` with ONE sample of row HROW poisoned: the first or the last of hop HHOP -> (the copy, the sample's index)."""
    n = HHOP * unit + (0 if edge == "first" else unit - 1)
    out = np.array(x)
    out[HROW, n] = value
    return out, n


def check_window(what, bad, clean, window, after=True):
    """``bad``, ``clean`` [rows, n]: the other rows equal, row HROW equal outside ``window`` and finite behind it."""
    others = [b for b in range(bad.shape[0]) if b != HROW]
    assert clean[others].any(axis=-1).all() and np.isfinite(clean).all(), "%s: the clean run is zero or not finite" % what
    assert same(bad[others], clean[others]), "%s: another row differs from the clean run" % what
    window = P.clip(window, bad.shape[1])
    got = P.changed(bad[HROW], clean[HROW])
    assert len(got), "%s: the poison did not arrive" % what
    assert np.isin(got, window).all(), "%s: row %d differs at %s, outside the documented window %d .. %d" % (
        what, HROW, got[~np.isin(got, window)][:8], window[0], window[-1])
    if after:
        assert window[-1] + 1 < bad.shape[1], "%s: the run ends inside the window" % what
        assert np.isfinite(bad[HROW, window[-1] + 1:]).all(), "%s: row %d is not finite behind the window" % (what, HROW)


def halves_wave(hops=HOPS):
    return np.ascontiguousarray(waves()[:hops, :HB].transpose(1, 0, 2).reshape(HB, hops * 256))


def stft_istft_hops(x):
    """``stft_hop``, the library's mag_in copied to mag_out (the model the identity), ``istft_hop``, hop by hop on a new handle ->
    (mag [B, hops, 256], pcm [B, hops * 256])."""
    eng, hip = NutlsEngine(batch=HB), _hip()
    y = torch.empty(HB, 256, device="cuda")
    mags_, outs = [], []
    for i in range(HOPS):
        eng.stft_hop(dev(x[:, i * 256:(i + 1) * 256]))
        mags_.append(eng.debug_get("mag_in", (256,)))
        torch.cuda.synchronize()
        # hipMemcpyDeviceToDevice = 3
        assert hip.hipMemcpy(ctypes.c_void_p(eng.io_out_ptr), ctypes.c_void_p(eng.io_in_ptr), ctypes.c_size_t(HB * 256 * 4), 3) == 0
        eng.istft_hop(y)
        outs.append(host(y))
    eng.close()
    return np.stack(mags_, axis=1), np.concatenate(outs, axis=1)


def stft_istft_block(x):
    off = NutlsOffline(max_frames=HOPS, utterances=HB)
    mag = off.stft_block_device(dev(x))
    out = host(off.istft_block_device(mag))
    mag = host(mag)
    off.close()
    return mag, out


@pytest.mark.parametrize("form", ["hop", "block"])
def test_transform_halves_forget_a_sample(form):
    """``stft`` / ``istft`` alone: one poisoned sample reaches two magnitude frames and three output hops, nothing else."""
    run = stft_istft_hops if form == "hop" else stft_istft_block
    x = halves_wave()
    mag0, out0 = run(x)
    for edge, value in SAMPLES:
        xb, n = one_sample(x, 256, edge, value)
        mag, out = run(xb)
        what = "%s transforms, sample %d = %r" % (form, n, value)
        frames = np.repeat(P.stft_support(n) * 256, 256) + np.tile(np.arange(256), 2)
        check_window(what + " (analysis)", mag.reshape(HB, -1), mag0.reshape(HB, -1), frames)
        check_window(what + " (analysis, synthesis)", out, out0, P.stft_istft_support(n))


def pcm_halves(rate, x16, xr, block, upper=0.0, follow=False, chain=False):
    """The decode half on ``xr [rows, hops * S]`` and the encode half on ``x16 [rows, hops * 256]`` (``chain``: on what the decode half
    returned), hop entries of a streaming handle or block entries of an offline one -> (decoded [rows, hops * 256], encoded [rows, hops * S])."""
    S = P.hop_samples(rate)
    hops = xr.shape[1] // S
    h = NutlsOffline(max_frames=hops, utterances=HB) if block else NutlsEngine(batch=HB)
    h.set_pcm_format(rate, "float32")
    if upper:
        h.set_pcm_upper_band(upper)
        h.set_pcm_upper_follow(follow)
    if block:
        d = h.pcm_decode_block_device(dev(xr))
        e = host(h.pcm_encode_block_device(d if chain else dev(x16)))
        d = host(d)
    else:
        ds, es = [], []
        for i in range(hops):
            di = h.pcm_decode_hop(dev(xr[:, i * S:(i + 1) * S]))
            es.append(host(h.pcm_encode_hop(di if chain else dev(x16[:, i * 256:(i + 1) * 256]))))
            ds.append(host(di))
        d, e = np.concatenate(ds, axis=1), np.concatenate(es, axis=1)
    h.close()
    return d, e


def rate_wave(rate, hops=HOPS):
    S = P.hop_samples(rate)
    return np.stack([0.1 * (b + 1) * np.random.default_rng([53, rate, b]).standard_normal(hops * S) for b in range(HB)]).astype(np.float32)


@pytest.mark.parametrize("block", [False, True], ids=["hop", "block"])
@pytest.mark.parametrize("rate", [8000, 32000, 48000])
def test_resampler_halves_forget_a_sample(rate, block):
    """``pcm_decode`` / ``pcm_encode`` alone at 8, 32 and 48 kHz float32: the windows follow from ``nutls_pcm_filter_taps``."""
    taps, S = len(runner.pcm_filter(rate)), P.hop_samples(rate)
    xr, x16 = rate_wave(rate), halves_wave()
    d0, e0 = pcm_halves(rate, x16, xr, block)
    for edge, value in SAMPLES:
        xb, n = one_sample(xr, S, edge, value)
        yb, m = one_sample(x16, 256, edge, value)
        d, e = pcm_halves(rate, yb, xb, block)
        check_window("decode %d Hz, sample %d = %r" % (rate, n, value), d, d0, P.decode_support(n, rate, taps))
        check_window("encode %d Hz, sample %d = %r" % (rate, m, value), e, e0, P.encode_support(m, rate, taps))


@pytest.mark.parametrize("block", [False, True], ids=["hop", "block"])
@pytest.mark.parametrize("follow", [False, True], ids=["fixed", "follow"])
def test_upper_band_halves_forget_a_sample(follow, block):
    """48 kHz, gain 1, ``encode(decode(x))``: the round trip, the upper band one hop later and -- with follow -- the whole hops that the
    energies of the touched hops reach (NUTLS_PCM_FOLLOW_HOPS); behind that the row is finite and bit-clean again."""
    rate = 48000
    taps, S = len(runner.pcm_filter(rate)), P.hop_samples(rate)
    xr = rate_wave(rate, UPPER_HOPS)
    d0, e0 = pcm_halves(rate, None, xr, block, upper=1.0, follow=follow, chain=True)
    for edge, value in SAMPLES:
        xb, n = one_sample(xr, S, edge, value)
        d, e = pcm_halves(rate, None, xb, block, upper=1.0, follow=follow, chain=True)
        what = "upper band%s, sample %d = %r" % (" with follow" if follow else "", n, value)
        check_window(what + " (decode)", d, d0, P.decode_support(n, rate, taps))
        check_window(what + " (encode)", e, e0, P.upper_chain_support(n, rate, taps, follow))


@pytest.mark.parametrize("switch", ["format", "gain", "follow"])
def test_gateway_switches_restart_poisoned_histories(switch):
    """Point 4 for the switches that restart a history: after a NaN hop through both halves (48 kHz, upper band with follow) a format
    switch, a gain change or a follow toggle -- each back to the same configuration -- leaves every row bit-identical to a fresh handle's."""
    rate = 48000
    S, hops = P.hop_samples(rate), 6
    xr = rate_wave(rate, hops)

    def prepare(h):
        h.set_pcm_format(rate, "float32")
        h.set_pcm_upper_band(1.0)
        h.set_pcm_upper_follow(True)

    def hop(h, x):
        d = h.pcm_decode_hop(dev(x))
        return host(d), host(h.pcm_encode_hop(d))

    a, b = NutlsEngine(batch=HB), NutlsEngine(batch=HB)
    prepare(a)
    prepare(b)
    bad = xr[:, :S].copy()
    bad[HROW] = np.nan
    d, e = hop(a, bad)
    assert np.isnan(d[HROW]).all() and np.isnan(e[HROW]).any() and np.isfinite(d[[0, 2]]).all()
    if switch == "format":
        prepare(a)
    elif switch == "gain":
        a.set_pcm_upper_band(0.5)
        a.set_pcm_upper_band(1.0)
    else:
        a.set_pcm_upper_follow(False)
        a.set_pcm_upper_follow(True)
    assert a.pcm_upper_band == 1.0 and a.pcm_upper_follow and not a.pcm_follow_gain().any()
    for i in range(1, hops):
        got, want = hop(a, xr[:, i * S:(i + 1) * S]), hop(b, xr[:, i * S:(i + 1) * S])
        assert np.isfinite(got[0]).all() and np.isfinite(got[1]).all() and want[1].any(axis=-1).all(), (switch, i)
        assert same(got[0], want[0]) and same(got[1], want[1]), "after the %s switch hop %d differs from a fresh handle's" % (switch, i)
    assert same(a.pcm_follow_gain(), b.pcm_follow_gain())
    a.close()
    b.close()


# ---- g. the gateway end to end -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("entry", ["packet", "hop"])
def test_gateway_contains_and_heals(entry):
    """48 kHz float32, two channels per frame row, B = 4, 20 ms packets (or hops), upper band with follow: channel 0 of frame row 0 --
    stream 0 -- is poisoned for two packets, then ``reset(0)``.  Its partner in the 16-byte words of the frame row, and row 1, are bit-clean
    throughout, with their follow gains and FIFO counters; after the reset channel 0 is bit-fresh."""
    B, C, rate = 4, 2, 48000
    n = 960 if entry == "packet" else P.hop_samples(rate)

    def make():
        e = NutlsEngine(batch=B)
        e.set_pcm_format(rate, "float32")
        e.set_pcm_upper_band(1.0)
        e.set_pcm_upper_follow(True)
        e.set_pcm_channels(C)
        if entry == "packet":
            e.set_pcm_packet(ms=20)
            assert e.pcm_packet_samples == n
        return e

    def step(h, frame):          # frame [B, n], one row per stream -> the callers' frame rows [B / C, n * C] and back
        inter = np.ascontiguousarray(frame.reshape(B // C, C, n).transpose(0, 2, 1).reshape(B // C, n * C))
        out = host(h.enhance_packet_pcm(dev(inter)) if entry == "packet" else h.enhance_hop_pcm(dev(inter)))
        return np.ascontiguousarray(out.reshape(B // C, n, C).transpose(0, 2, 1).reshape(B, n))

    def extra(h):
        res = {"pcm_follow_gain": h.pcm_follow_gain()}
        if entry == "packet":
            res["pcm_packet_fill"] = h.pcm_packet_fill()
        return res

    x = np.stack([0.05 * (b + 1) * np.random.default_rng([59, b]).standard_normal((FRAMES, n)) for b in range(B)], axis=1).astype(np.float32)
    # (the first packets return the priming silence and the lag -- D + S + nutls_pcm_delay_samples = 1 488 samples: non-zero from the third on)
    fresh = fresh_run(make, x, step, extra=extra)
    clean = script(make, P.clean_twin(x, 0, BAD), 0, step, extra=extra)
    for kind in P.KINDS:
        bad = script(make, P.poisoned(x, 0, BAD, kind), 0, step, extra=extra)
        check_script("gateway, %s entry, %s" % (entry, kind), bad, clean, fresh, 0, B, live_from=2)


# ---- h. the corpus scheduler -------------------------------------------------------------------------------------------------------------------
def test_corpus_scheduler_hands_on_a_clean_slot():
    """``enhance_many`` on five recordings of 5 to 20 hops through two slots of 8 frames; the second-longest is NaN from its third hop on.
    The four others are bit-identical to the run that zeroes the bad part (the same schedule) -- the recording that inherits the poisoned
    slot included: the production form of healing."""
    hops = (12, 20, 5, 17, 8)
    bad_item = 3
    recs = [(0.05 * np.random.default_rng([61, i]).standard_normal((h + 1) * 256 + 100)).astype(np.float32) for i, h in enumerate(hops)]
    assert sorted(hops)[-2] == hops[bad_item]
    plan = plan_ragged_blocks(hops, 2, 8)
    slot = {s for blk in plan for s, item, _, _, _ in blk if item == bad_item}
    assert len(slot) == 1
    heirs = [item for blk in plan for s, item, first, _, _ in blk if s in slot and item != bad_item and first == 0]
    later = [i for i, blk in enumerate(plan) for s, item, _, _, _ in blk if item in heirs]
    last_bad = max(i for i, blk in enumerate(plan) for s, item, _, _, _ in blk if item == bad_item)
    assert heirs and min(later) > last_bad, "no recording inherits the poisoned slot"
    poisoned, zeroed = [r.copy() for r in recs], [r.copy() for r in recs]
    poisoned[bad_item][2 * 256:] = np.nan
    zeroed[bad_item][2 * 256:] = 0.0
    off = NutlsOffline(max_frames=8, utterances=2)
    got = off.enhance_many(poisoned)
    off.close()
    off = NutlsOffline(max_frames=8, utterances=2)
    want = off.enhance_many(zeroed)
    off.close()
    assert not np.isfinite(got[bad_item]).all(), "the poison did not arrive"
    for i in range(len(recs)):
        if i != bad_item:
            assert want[i].any() and np.isfinite(got[i]).all(), i
            assert same(got[i], want[i]), "recording %d differs from the clean run%s" % (i, " (it inherits the poisoned slot)" if i in heirs else "")
