"""GPU checks of the per-stream active mask (include/nutls.h nutls_step_active; csrc/fused_step.hip hold_stream): a handle's streams run
on their own clocks -- a stream held at a tick keeps its whole state, and what it computes depends on the frames it took, not on the
ticks it took them at.  The reference steps ONE stream per call (dnn_model/interpreter_proposed.py:215-350), so each of its streams
trivially has its own clock; the reference here is therefore a second handle of this library stepped unmasked, in which stream b
receives its k-th frame at step k.

Comparisons are bitwise (np.array_equal): the hold path is a copy, and the project already asserts bit-identity of a stream across
slots, partners and handles (test_gpu_packed.py::test_packed_vs_oracle_and_slot_independence).  The one tolerance, for a stream whose
state was restored through nutls_state_set, is the one test_gpu_parity.py::test_fused_carried_sums_follow_mode_switches_and_state_edits
uses for such a stream (rms < 1e-6: the carried sums are rebuilt by another kernel, in another summation order)."""
import ctypes
import os

import numpy as np
import pytest

import nunet_amd
from conftest import GOLDEN
from nunet_amd import NutlsEngine, NutlsOffline
from nunet_amd import runner

pytestmark = pytest.mark.gpu
RESTORED_RMS = 1e-6      # test_gpu_parity.py::test_fused_carried_sums_follow_mode_switches_and_state_edits


def rms(a, b):
    return float(np.sqrt(np.mean((np.asarray(a, np.float64) - np.asarray(b, np.float64)) ** 2)))


@pytest.fixture(scope="module")
def clip():
    return np.load(os.path.join(GOLDEN, "clip_4s.npz"))


def frame_of(clip, b, k):
    """k-th frame of stream b: the golden clip's magnitudes at a per-stream offset."""
    n = clip["mags_in"].shape[0]
    return clip["mags_in"][(31 * b + k) % n]


def schedule(B, ticks, G, seed):
    """Seeded random masks [ticks, B] with the cases the feature must survive forced in."""
    rng = np.random.default_rng(seed)
    m = (rng.random((ticks, B)) < 0.6).astype(np.uint8)
    m[:5, 2] = 0                 # a stream held from the very first tick
    m[3, :] = 0                  # everybody held
    m[5, :] = 1                  # everybody active (stream 2's first frame)
    m[7, :] = 1; m[7, 1] = 0     # exactly one slot of a packed group held (group 0 of the 2- and of the 4-stream plan)
    m[8, :] = 1; m[8, B - 2] = 0  # ... and of the last group, the other slot parity
    m[9, :] = 0; m[9, 0] = 1     # exactly one slot of one group ACTIVE, every other group entirely held
    return m


def lockstep_reference(clip, B, G, steps, snapshots=True):
    """The reference handle: same B and plan, unmasked, stream b gets its k-th frame at step k.  -> outputs [steps][B,256], states [steps][B][...]"""
    ref = NutlsEngine(batch=B, streams_per_workgroup=G)
    outs, snaps = [], []
    for k in range(steps):
        outs.append(ref.step(np.stack([frame_of(clip, b, k) for b in range(B)])).copy())
        if snapshots:
            snaps.append([ref.state_get_all(b) for b in range(B)])
    ref.close()
    return outs, snaps


@pytest.mark.parametrize("G", [1, 2, 4])
def test_schedule_equivalence(clip, G):
    """Every stream consumes its own frame sequence on its own random clock: each active output row, and each stream's states at the end,
    equal the lockstep reference's for that stream's frame count -- bit for bit, on all three plans."""
    B, ticks = 8, 20
    masks = schedule(B, ticks, G, seed=100 + G)
    counts = masks.sum(axis=0)
    assert counts.min() >= 1 and counts.max() < ticks and len(set(counts.tolist())) > 2      # (the clocks really differ)
    want_out, want_state = lockstep_reference(clip, B, G, int(counts.max()))
    eng = NutlsEngine(batch=B, streams_per_workgroup=G)
    assert eng.streams_per_workgroup == G and eng.mode == "fused"
    cnt = [0] * B
    for t in range(ticks):
        x = np.full((B, 256), np.nan, np.float32)          # a held stream's row is not used: it holds NaN
        for b in range(B):
            if masks[t, b]:
                x[b] = frame_of(clip, b, cnt[b])
        out = eng.step(x, active=masks[t])
        for b in range(B):
            if masks[t, b]:
                assert np.array_equal(out[b], want_out[cnt[b]][b]), (t, b, cnt[b])
                cnt[b] += 1
            else:
                assert not out[b].any(), (t, b)
        if t in (3, 9):      # (somebody looks at the states in the middle: the lazily written ones are rebuilt under held streams too)
            for b in (0, 2, 5):
                if cnt[b]:
                    assert np.array_equal(eng.state_get_all(b), want_state[cnt[b] - 1][b]), (t, b)
    for b in range(B):
        assert np.array_equal(eng.state_get_all(b), want_state[cnt[b] - 1][b]), b
    eng.close()


@pytest.mark.parametrize("G", [1, 2])
def test_held_rows(clip, G):
    """Held rows of the output are zero, a held stream's states are identical before and after the call, and a NaN-filled held input row
    leaves the other streams' outputs unaffected and finite."""
    B = 4
    for held in ([1], [0, 1], [0, 3], [0, 1, 2, 3]):
        eng, twin = NutlsEngine(batch=B, streams_per_workgroup=G), NutlsEngine(batch=B, streams_per_workgroup=G)
        for k in range(3):
            x = np.stack([frame_of(clip, b, k) for b in range(B)])
            assert np.array_equal(eng.step(x), twin.step(x))
        mask = np.ones(B, bool)
        mask[held] = False
        live = [b for b in range(B) if mask[b]]
        before = {b: eng.state_get_all(b) for b in held}
        x = np.stack([frame_of(clip, b, 3) for b in range(B)])
        xm = x.copy()
        xm[held] = np.nan
        for rep in range(2):      # (twice: both state parities have been the held side)
            out = eng.step(xm, active=mask)
            assert not out[held].any()
            for b in held:
                assert np.array_equal(eng.state_get_all(b), before[b]), (held, b, rep)
            tout = twin.step(x)       # the twin steps everybody
            assert np.isfinite(out[live]).all()
            assert np.array_equal(out[live], tout[live]), (held, rep)
        for b in live:
            assert np.array_equal(eng.state_get_all(b), twin.state_get_all(b)), (held, b)
        eng.close(); twin.close()


@pytest.mark.parametrize("G", [1, 2])
def test_full_mask_and_no_mask(clip, G):
    """active=None and an all-ones mask both equal step() on a twin handle (outputs and states)."""
    B = 4
    plain, none, ones = (NutlsEngine(batch=B, streams_per_workgroup=G) for _ in range(3))
    for k in range(5):
        x = np.stack([frame_of(clip, b, k) for b in range(B)])
        want = plain.step(x)
        assert np.array_equal(none.step(x, active=None), want)
        assert np.array_equal(ones.step(x, active=np.ones(B, np.uint8)), want)
    for b in range(B):
        s = plain.state_get_all(b)
        assert np.array_equal(none.state_get_all(b), s) and np.array_equal(ones.state_get_all(b), s)
    for e in (plain, none, ones):
        e.close()


def test_host_entries(clip):
    """Pageable buffers and host_alloc buffers (the zero-copy path) with a mask give the device-buffer result."""
    import torch
    B = 6
    dev, page, pin = (NutlsEngine(batch=B, streams_per_workgroup=2) for _ in range(3))
    pin_in, pin_out = nunet_amd.host_alloc((B, 256)), nunet_amd.host_alloc((B, 256))
    rng = np.random.default_rng(5)
    for k in range(8):
        mask = (rng.random(B) < 0.5).astype(np.uint8) if k else np.ones(B, np.uint8)
        x = np.stack([frame_of(clip, b, k) for b in range(B)])
        xt, mt = torch.from_numpy(x).cuda(), torch.from_numpy(mask).cuda()
        want = dev.step(xt, active=mt)
        torch.cuda.synchronize()
        want = want.cpu().numpy()
        assert not want[mask == 0].any()
        assert np.array_equal(page.step(x, active=mask.astype(bool)), want), k
        pin_in[...] = x
        got = pin.step(pin_in, out=pin_out, active=mask)
        assert got is pin_out and np.array_equal(got, want), k
    for b in range(B):
        s = dev.state_get_all(b)
        assert np.array_equal(page.state_get_all(b), s) and np.array_equal(pin.state_get_all(b), s)
    for e in (dev, page, pin):
        e.close()


def test_waveform_path(clip):
    """enhance_hop(..., active=...) with streams fed hops at different ticks: per stream the PCM of a reference handle fed hop by hop in
    lockstep; held ticks return zero hops (and the previous hop / overlap tail of a held stream stay: its next hop continues seamlessly)."""
    import torch
    B, ticks = 4, 14
    pcm = clip["noisy_i16"].astype(np.float32) / 32768.0

    def hop_of(b, k):
        o = 4000 * b + 256 * k
        return pcm[o:o + 256]

    masks = schedule(8, ticks, 2, seed=9)[:, :B].copy()
    masks[5, :] = 1
    counts = masks.sum(axis=0)
    ref = NutlsEngine(batch=B)
    want = [ref.enhance_hop(np.stack([hop_of(b, k) for b in range(B)])).copy() for k in range(int(counts.max()))]
    ref.close()
    for device in (False, True):
        eng = NutlsEngine(batch=B)
        cnt = [0] * B
        for t in range(ticks):
            x = np.full((B, 256), np.nan, np.float32)
            for b in range(B):
                if masks[t, b]:
                    x[b] = hop_of(b, cnt[b])
            if device:
                out = eng.enhance_hop(torch.from_numpy(x).cuda(), active=torch.from_numpy(masks[t]).cuda())
                torch.cuda.synchronize()
                out = out.cpu().numpy()
            else:
                out = eng.enhance_hop(x, active=masks[t])
            for b in range(B):
                if masks[t, b]:
                    assert np.array_equal(out[b], want[cnt[b]][b]), (device, t, b)
                    cnt[b] += 1
                else:
                    assert not out[b].any(), (device, t, b)
        eng.close()


def test_state_edits_under_holds(clip):
    """nutls_state_set on one stream between masked steps: the restored stream continues like the stream it was copied from (within the
    restored-stream tolerance of test_gpu_parity.py), is held right after the edit without losing it, and the other streams stay bit-exact."""
    B = 4
    eng, ref, donor = NutlsEngine(batch=B), NutlsEngine(batch=B), NutlsEngine(batch=B)
    names = [n for n, _ in eng.state_specs()]
    # the donor: stream 0 of an uninterrupted handle, 6 frames of ITS sequence (stream index 9 of the frame table)
    for k in range(6):
        donor.step(np.stack([frame_of(clip, 9 + b, k) for b in range(B)]))
    # phase 1: streams 1..3 take 5 frames, stream 0 only 3 of the 5 ticks; the reference in lockstep
    for t in range(5):
        mask = np.ones(B, np.uint8)
        mask[0] = t not in (1, 3)
        x = np.stack([frame_of(clip, b, t) for b in range(B)])      # (stream 0's history does not matter: it is about to be replaced)
        out = eng.step(x, active=mask)
        want = ref.step(np.stack([frame_of(clip, b, t) for b in range(B)]))
        assert np.array_equal(out[1:], want[1:]), t
    # the edit: stream 0 of both handles becomes the donor's stream 0 (get, change one row, set)
    for e in (eng, ref):
        for n in names:
            v = e.state_get(n)
            v[0] = donor.state_get(n)[0]
            e.state_set(n, v)
    edited = eng.state_get_all(0)
    assert np.array_equal(edited, donor.state_get_all(0))
    # phase 2: stream 0 is held on the first ticks after the edit, the others run on their own clocks
    masks = np.array([[0, 1, 1, 0], [0, 0, 1, 1], [1, 1, 1, 1], [1, 1, 0, 1], [0, 1, 1, 1], [1, 0, 1, 1], [1, 1, 1, 0]], np.uint8)
    counts = masks.sum(axis=0)
    want_out, want0 = [], []
    for k in range(int(counts.max())):
        want_out.append(ref.step(np.stack([frame_of(clip, 9, 6 + k)] + [frame_of(clip, b, 5 + k) for b in range(1, B)])).copy())
        want0.append(donor.step(np.stack([frame_of(clip, 9 + b, 6 + k) for b in range(B)]))[0].copy())
    cnt = [0] * B
    for t in range(len(masks)):
        x = np.full((B, 256), np.nan, np.float32)
        if masks[t, 0]:
            x[0] = frame_of(clip, 9, 6 + cnt[0])
        for b in range(1, B):
            if masks[t, b]:
                x[b] = frame_of(clip, b, 5 + cnt[b])
        out = eng.step(x, active=masks[t])
        if t == 1:
            assert np.array_equal(eng.state_get_all(0), edited)      # two holds after the edit: still exactly what was set
        for b in range(B):
            if not masks[t, b]:
                assert not out[b].any()
                continue
            if b == 0:
                print("restored stream, frame %d: rms vs the uninterrupted donor %.3e" % (cnt[0], rms(out[0], want0[cnt[0]])))
                assert rms(out[0], want0[cnt[0]]) < RESTORED_RMS, (t, cnt[0])
                assert np.array_equal(out[0], want_out[cnt[0]][0]), (t, cnt[0])      # (and bit for bit like the unmasked handle with the same edit)
            else:
                assert np.array_equal(out[b], want_out[cnt[b]][b]), (t, b)
            cnt[b] += 1
    for e in (eng, ref, donor):
        e.close()


def test_refusals(clip):
    """A mask where it is not supported is a ValueError with the reason, never a silent full step; the handle's state is unchanged."""
    from nunet_amd.weights import synthetic_weights, write_blob
    x = np.stack([frame_of(clip, b, 0) for b in range(2)])
    mask = np.array([1, 0], np.uint8)

    def refused(eng, match, call=None):
        before = [eng.state_get_all(b) for b in range(2)]
        with pytest.raises(ValueError, match=match):
            (call or (lambda: eng.step(x, active=mask)))()
        for b in range(2):
            assert np.array_equal(eng.state_get_all(b), before[b])

    eng = NutlsEngine(batch=2)
    eng.step(x)
    refused(eng, "length 2", lambda: eng.step(x, active=np.ones(3, np.uint8)))          # wrong length
    refused(eng, "bool / uint8", lambda: eng.step(x, active=np.ones(2, np.int32)))       # wrong dtype
    refused(eng, "length 2", lambda: eng.enhance_hop(x, active=np.ones(1, bool)))
    for mode in ("launches", "graph"):                                                   # modes 0 / 1
        eng.set_mode(mode)
        refused(eng, "mode 3")
        refused(eng, "mode 3", lambda: eng.enhance_hop(x, active=mask))
    eng.set_mode("fused")
    eng.set_ctfa_mode("causal32")                                                        # the time-attention ring
    refused(eng, "CAUSAL32")
    eng.set_ctfa_mode("frame")
    want = NutlsEngine(batch=2)
    want.step(x)
    out = eng.step(x, active=mask)                                                       # ... and back in the supported configuration it runs
    assert np.array_equal(out[0], want.step(x)[0]) and not out[1].any()
    eng.close(); want.close()
    base = NutlsEngine(write_blob(synthetic_weights("baseline", seed=4321, bias_std=0.1, affine_jitter=0.1), int8_convs=True),
                       batch=2, variant="baseline")                                      # baseline variant: history rings
    assert base.mode == "fused"
    base.step(x)
    refused(base, "baseline")
    base.close()
    off = NutlsOffline(max_frames=8)                                                     # an offline handle
    lib, buf, m = off._lib, np.zeros((8, 256), np.float32), np.ones(8, np.uint8)
    fp = buf.ctypes.data_as(ctypes.POINTER(ctypes.c_float))
    with pytest.raises(ValueError, match="streaming handle"):
        runner._check(lib, lib.nutls_step_host_active(off._h, fp, fp, m.ctypes.data))
    with pytest.raises(ValueError, match="streaming handle"):
        runner._check(lib, lib.nutls_enhance_hop_host_active(off._h, fp, fp, m.ctypes.data, 0))
    with pytest.raises(ValueError, match="streaming handle"):
        runner._check(lib, lib.nutls_step_active(off._h, buf.ctypes.data, buf.ctypes.data, m.ctypes.data, None))
    off.close()
