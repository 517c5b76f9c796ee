"""``-m gpu``: ragged blocks of the offline batch handles (``nutls_process_block_ragged``, include/nutls.h "Ragged blocks"): per-utterance
frame counts around the unchanged block.  Three utterances (different offsets into the golden clip, as tests/test_gpu_offline.py's batch
test) in one ``NutlsOffline(max_frames=24, utterances=3)``.  What is compared bit for bit is the ragged call against the uniform call of
the same width on the same handle shape (same launches, same sizes); against one-utterance handles the bounds are the project's own for
"batched equals one-utterance handles" (tests/test_gpu_offline.py: RMS < 1e-6 on outputs; states and goldens < 2e-5)."""
import ctypes
import os

import numpy as np
import pytest
import torch      # (before the first handle: torch must bring up the HIP runtime it ships with itself)

from nunet_amd import NutlsOffline
from nunet_amd.runner import NUTLS_ERR_ARG, _fptr

from conftest import GOLDEN

pytestmark = pytest.mark.gpu

U, W = 3, 24
STARTS = [0, 60, 131]
C1, C2 = [24, 7, 0], [5, 24, 13]


def rms(a, b):
    return float(np.sqrt(np.mean((np.asarray(a, np.float64) - np.asarray(b, np.float64)) ** 2)))


@pytest.fixture(scope="module")
def clip():
    return np.load(os.path.join(GOLDEN, "clip_4s.npz"))


@pytest.fixture(scope="module")
def x(clip):
    """[U, 48, 256]: utterance u = the clip from frame STARTS[u]."""
    return np.stack([clip["mags_in"][s:s + 2 * W] for s in STARTS])


@pytest.fixture(scope="module")
def off():
    h = NutlsOffline(max_frames=W, utterances=U)
    yield h
    h.close()


def _names(h):
    out, nm, d0, d1 = [], ctypes.c_char_p(), ctypes.c_int(), ctypes.c_int()
    for i in range(h._lib.nutls_state_count(h._h)):
        assert h._lib.nutls_state_info(h._h, i, ctypes.byref(nm), ctypes.byref(d0), ctypes.byref(d1)) == 0
        out.append(nm.value.decode())
    return out


def states(h):
    """All 130 carried state tensors, name -> [utterances, ...]."""
    names = _names(h)
    assert len(names) == 130
    return {n: h.state_get(n) for n in names}


def block(x, first, counts, fill=0.0):
    """[U, W, 256]: utterance u's frames first[u] .. first[u] + counts[u] - 1 in its leading rows, `fill` behind."""
    b = np.full((U, W, 256), fill, np.float32)
    for u in range(U):
        b[u, :counts[u]] = x[u, first[u]:first[u] + counts[u]]
    return b


def run(h, blk, frames=None):
    got = h.process_block_device(torch.from_numpy(blk).cuda(), frames=frames)
    return got.cpu().numpy()


@pytest.fixture(scope="module")
def uniform(off, x):
    """The uniform call of width 24 on the freshly reset handle: outputs and states."""
    off.reset()
    out = run(off, np.ascontiguousarray(x[:, :W]))
    return out, states(off)


@pytest.fixture(scope="module")
def ragged1(off, x, uniform):
    """The ragged call [24, 7, 0] on the freshly reset handle (rows behind the counts: zeros in the input): outputs and states."""
    off.reset()
    out = run(off, block(x, [0, 0, 0], C1), C1)
    return out, states(off)


def test_valid_rows_are_the_uniform_calls_bits_and_the_rest_is_zero(off, x, uniform, ragged1):
    want, _ = uniform
    got, st = ragged1
    for u, k in enumerate(C1):
        np.testing.assert_array_equal(got[u, :k], want[u, :k])
        np.testing.assert_array_equal(got[u, k:], 0.0)
    assert np.abs(got[0]).max() > 0
    # whatever the caller's rows behind the counts hold -- NaN here -- has no effect: same bits, and nothing of it in any state
    off.reset()
    blk = block(x, [0, 0, 0], C1, fill=np.nan)
    again = run(off, blk, C1)
    np.testing.assert_array_equal(again, got)
    assert np.isfinite(again).all()
    for name, a in states(off).items():
        assert np.isfinite(a).all(), name
        np.testing.assert_array_equal(a, st[name], err_msg=name)
    assert np.isnan(blk[2]).all()          # (the caller's buffer is not written)


def test_full_counts_are_the_uniform_call(off, x, uniform):
    want, want_st = uniform
    off.reset()
    got = run(off, np.ascontiguousarray(x[:, :W]), [W] * U)
    np.testing.assert_array_equal(got, want)
    for name, a in states(off).items():
        np.testing.assert_array_equal(a, want_st[name], err_msg=name)
    # frames=None is the entry without counts
    off.reset()
    np.testing.assert_array_equal(run(off, np.ascontiguousarray(x[:, :W]), None), want)


def two_ragged_calls(h, x, c1, c2):
    """Counts c1 then c2 -> each utterance's concatenated valid rows (garbage, not zeros, behind the counts on the way in)."""
    a = run(h, block(x, [0] * U, c1, fill=1e3), c1)
    b = run(h, block(x, c1, c2, fill=-7.0), c2)
    for u in range(U):
        assert not a[u, c1[u]:].any() and not b[u, c2[u]:].any()
    return [np.concatenate([a[u, :c1[u]], b[u, :c2[u]]]) for u in range(U)]


def check_against_one_utterance_handles(got, x, ctfa_mode, h):
    for u in range(U):
        n = len(got[u])
        one = NutlsOffline(max_frames=W, ctfa_mode=ctfa_mode)
        want = one.process(x[u, :n])          # one call of 24 or fewer frames, or two
        e_out = rms(got[u], want)
        e_h = rms(h.state_get("msfe4_en_h")[u], one.state_get("msfe4_en_h")[0])
        e_p = rms(h.state_get("msfe6_ee_prev1")[u], one.state_get("msfe6_ee_prev1")[0])
        one.close()
        print("%s utterance %d (%d frames): output rms %.3e (bound 1e-6), msfe4_en_h %.3e, msfe6_ee_prev1 %.3e (bound 2e-5)" % (ctfa_mode, u, n, e_out, e_h, e_p))
        assert e_out < 1e-6, u
        assert e_h < 2e-5 and e_p < 2e-5, u


def test_state_is_carried_from_each_utterances_own_last_frame(off, x, clip):
    off.reset()
    got = two_ragged_calls(off, x, C1, C2)
    assert [len(g) for g in got] == [29, 31, 13]
    check_against_one_utterance_handles(got, x, "frame", off)
    # the goldens are the clip from its first frame: every slot fed from frame 0, same counts
    off.reset()
    x0 = np.stack([clip["mags_in"][:2 * W]] * U)
    for u, g in enumerate(two_ragged_calls(off, x0, C1, C2)):
        e = rms(g, clip["mags_out"][:len(g)])
        print("utterance %d from frame 0: rms vs goldens %.3e (bound 2e-5)" % (u, e))
        assert e < 2e-5, u


def test_a_held_utterance_keeps_every_state_and_disturbs_nobody(off, x):
    results = []
    for other in (x[2, W:2 * W], np.full((W, 256), np.nan, np.float32)):
        off.reset()
        run(off, np.ascontiguousarray(x[:, :8]))          # everybody has a history
        before = states(off)
        blk = block(x, [8, 8, 8], C1)
        blk[2] = other                                    # the held utterance's rows
        out = run(off, blk, C1)
        after = states(off)
        for name in before:
            np.testing.assert_array_equal(after[name][2], before[name][2], err_msg=name)
        assert any(np.abs(before[n][2]).max() > 0 for n in before)
        assert not np.array_equal(after["msfe4_en_h"][0], before["msfe4_en_h"][0])
        results.append((out, after))
    (out_a, st_a), (out_b, st_b) = results
    np.testing.assert_array_equal(out_a, out_b)
    for name in st_a:
        np.testing.assert_array_equal(st_a[name], st_b[name], err_msg=name)


def test_causal32_history_is_rolled_from_each_utterances_own_last_frame(x):
    """Counts below 31 throughout: source and destination rows of the history roll overlap."""
    c1, c2 = [3, 24, 0], [24, 1, 9]
    h = NutlsOffline(max_frames=W, utterances=U, ctfa_mode="causal32")
    got = two_ragged_calls(h, x, c1, c2)
    assert [len(g) for g in got] == [27, 25, 9]
    check_against_one_utterance_handles(got, x, "causal32", h)
    h.close()


@pytest.mark.parametrize("ctfa_mode", ["frame", "causal32"])
def test_chunk_pipeline_with_counts(x, ctfa_mode):
    """The existing chunk-independence bound (tests/test_gpu_offline.py: RMS < 1e-6, max abs < 5e-5), outputs and all states; a second block
    so that what the commit carried (state, history) is used too."""
    res = []
    for chunks in (1, 2):
        h = NutlsOffline(max_frames=W, utterances=U, ctfa_mode=ctfa_mode, pipeline=chunks)
        a = run(h, block(x, [0] * U, C1), C1)
        b = run(h, block(x, C1, C2), C2)
        res.append((np.concatenate([a, b], axis=1), states(h)))
        h.close()
    (one, st1), (two, st2) = res
    worst = (rms(two, one), float(np.abs(two - one).max()))
    for name in st1:
        worst = (max(worst[0], rms(st2[name], st1[name])), max(worst[1], float(np.abs(st2[name] - st1[name]).max())))
    print("%s, 2 chunks vs 1: worst rms %.3e (bound 1e-6), worst max abs %.3e (bound 5e-5) over outputs and 130 states" % ((ctfa_mode,) + worst))
    assert rms(two, one) < 1e-6 and float(np.abs(two - one).max()) < 5e-5
    for name in st1:
        assert rms(st2[name], st1[name]) < 1e-6 and float(np.abs(st2[name] - st1[name]).max()) < 5e-5, name


def test_device_counts_are_clamped_and_host_counts_are_checked(off, x, ragged1):
    wild = [99, -3, 7]
    off.reset()
    blk = block(x, [0] * U, [W, 0, 7])
    want = run(off, blk, [W, 0, 7])
    want_st = states(off)
    off.reset()
    got = run(off, blk, torch.tensor(wild, dtype=torch.int32, device="cuda"))
    np.testing.assert_array_equal(got, want)
    for name, a in states(off).items():
        np.testing.assert_array_equal(a, want_st[name], err_msg=name)
    # the same values in host memory are refused, and nothing is touched
    off.reset()
    cnt = np.array(wild, np.int32)
    out = np.empty_like(blk)
    rc = off._lib.nutls_process_block_ragged_host(off._h, _fptr(blk), _fptr(out), W, cnt.ctypes.data_as(ctypes.POINTER(ctypes.c_int)))
    assert rc == NUTLS_ERR_ARG and b"outside" in off._lib.nutls_last_error()
    with pytest.raises(ValueError):
        off.process_block_device(torch.from_numpy(blk).cuda(), frames=wild)
    ref_out, ref_st = ragged1
    np.testing.assert_array_equal(run(off, block(x, [0] * U, C1), C1), ref_out)
    for name, a in states(off).items():
        np.testing.assert_array_equal(a, ref_st[name], err_msg=name)


def test_process_ragged_takes_any_lengths(off, x):
    lens = [31, 0, 13]
    off.reset()
    got = off.process_ragged([x[u, :n] for u, n in enumerate(lens)])
    assert [g.shape for g in got] == [(n, 256) for n in lens]
    for u, n in enumerate(lens):
        if n:
            one = NutlsOffline(max_frames=W)
            assert rms(got[u], one.process(x[u, :n])) < 1e-6, u
            one.close()
    with pytest.raises(ValueError):
        off.process_ragged([x[0], x[1]])
