"""CPU-side checks of the ragged block calls (include/nutls.h, "Ragged blocks"): the six entries are declared with the documented
signatures, exported and bound, they refuse a null handle before touching a device, the new kernels are a source of the library, and
the schedule of ``NutlsOffline.enhance_many`` (``plan_ragged_blocks``, a pure function) keeps its invariants on seeded length sets.
No reference counterpart: the reference enhances one recording at a time (dnn_model/interpreter_proposed.py:203-370)."""
import ctypes
import os
import re

import numpy as np
import pytest

from nunet_amd import plan_ragged_blocks, runner
from nunet_amd.build import SOURCES, build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIGNATURES = {
    "nutls_process_block_ragged": "nutls_handle* h, const float* mag_in, float* mag_out, int n_frames, const int* frames, void* stream",
    "nutls_process_block_ragged_host": "nutls_handle* h, const float* mag_in, float* mag_out, int n_frames, const int* frames",
    "nutls_enhance_block_ragged": "nutls_handle* h, const float* pcm_in, float* pcm_out, int n_hops, const int* hops, int dc_mode, void* stream",
    "nutls_enhance_block_ragged_host": "nutls_handle* h, const float* pcm_in, float* pcm_out, int n_hops, const int* hops, int dc_mode",
    "nutls_stft_block_ragged": "nutls_handle* h, const float* pcm_in, float* mag, int n_hops, const int* hops, void* stream",
    "nutls_istft_block_ragged": "nutls_handle* h, const float* mag, float* pcm_out, int n_hops, const int* hops, int dc_mode, void* stream",
}


@pytest.fixture(scope="module")
def lib():
    build()
    return runner.load_library()


def test_the_six_symbols_are_declared_exported_and_bound(lib):
    hdr = open(os.path.join(ROOT, "include", "nutls.h")).read()
    declared = dict(re.findall(r"^int (nutls_[a-z_]+)\(([^)]*)\);", hdr, re.M))
    for name, params in SIGNATURES.items():
        assert " ".join(declared.get(name, "").split()) == params, name
        assert name in runner.ABI_SYMBOLS, name
        fn = getattr(lib, name)
        assert fn.argtypes is not None and len(fn.argtypes) == params.count(",") + 1 and fn.restype is ctypes.c_int, name
    for method in ("process_ragged", "enhance_ragged", "enhance_many"):
        assert callable(getattr(runner.NutlsOffline, method)), method
    assert "ragged.hip" in SOURCES


def test_a_null_handle_is_an_argument_error_with_a_message(lib):
    x = np.zeros(256, np.float32)
    cnt = np.zeros(1, np.int32)
    fp, ip = runner._fptr, cnt.ctypes.data_as(ctypes.POINTER(ctypes.c_int))
    addr, caddr = x.ctypes.data, cnt.ctypes.data
    calls = (
        lambda: lib.nutls_process_block_ragged(None, addr, addr, 1, caddr, None),
        lambda: lib.nutls_process_block_ragged_host(None, fp(x), fp(x), 1, ip),
        lambda: lib.nutls_enhance_block_ragged(None, addr, addr, 1, caddr, 0, None),
        lambda: lib.nutls_enhance_block_ragged_host(None, fp(x), fp(x), 1, ip, 0),
        lambda: lib.nutls_stft_block_ragged(None, addr, addr, 1, caddr, None),
        lambda: lib.nutls_istft_block_ragged(None, addr, addr, 1, caddr, 0, None),
    )
    for call in calls:
        assert call() == runner.NUTLS_ERR_ARG
        assert b"null" in lib.nutls_last_error()


def length_sets():
    """A dozen seeded sets: (lengths, utterances, max_frames) -- zero-length items, items of several blocks, fewer items than slots."""
    rng = np.random.default_rng(20240)
    sets = [
        ([0, 0, 0], 2, 8),                       # nothing to do
        ([5], 4, 8),                             # fewer items than slots
        ([100, 3], 3, 8),                        # one long item next to a short one, a slot never used
        ([8, 8, 8, 8], 2, 8),                    # exact multiples of the block
        ([0, 17, 0, 1, 64, 9, 0], 3, 16),
    ]
    for _ in range(7):
        n_items = int(rng.integers(1, 24))
        max_frames = int(rng.choice([1, 7, 8, 24, 256]))
        lengths = rng.integers(0, 5 * max_frames + 2, size=n_items)
        lengths[rng.random(n_items) < 0.2] = 0
        sets.append(([int(n) for n in lengths], int(rng.integers(1, 9)), max_frames))
    assert len(sets) == 12
    return sets


@pytest.mark.parametrize("lengths,utterances,max_frames", length_sets())
def test_plan_ragged_blocks_invariants(lengths, utterances, max_frames):
    blocks = plan_ragged_blocks(lengths, utterances, max_frames)
    next_hop = [0] * len(lengths)
    slot_of_item = {}
    holder = [None] * utterances          # item the slot held in the previous block, if it goes on
    for block in blocks:
        assert block, "no empty blocks"
        slots = [e[0] for e in block]
        assert len(set(slots)) == len(slots), "a slot holds one item per block"
        assert len({e[1] for e in block}) == len(block), "an item is in one slot"
        for slot, item, first, count, reset_before in block:
            assert 0 <= slot < utterances and 0 <= item < len(lengths)
            assert 1 <= count <= max_frames
            assert first == next_hop[item], "hops in order, none twice, none skipped"
            next_hop[item] = first + count
            assert slot_of_item.setdefault(item, slot) == slot, "an item never changes slot"
            assert reset_before == (first == 0), "reset exactly in front of an item's first block"
            if first > 0:
                assert holder[slot] == item, "an item continues in consecutive blocks, and nobody took its slot in between"
            else:
                assert holder[slot] is None, "a slot is free before it takes a new item"
        for slot in range(utterances):
            entry = [e for e in block if e[0] == slot]
            holder[slot] = entry[0][1] if entry and next_hop[entry[0][1]] < lengths[entry[0][1]] else None
    assert next_hop == list(lengths), "every hop of every item exactly once"
    # longest first: the items' first blocks come in order of decreasing length
    started = [item for block in blocks for _, item, first, _, _ in block if first == 0]
    assert [lengths[i] for i in started] == sorted((n for n in lengths if n > 0), reverse=True)


def test_plan_ragged_blocks_rejects_nonsense():
    for args in (([1], 0, 8), ([1], 2, 0), ([-1], 2, 8)):
        with pytest.raises(ValueError):
            plan_ragged_blocks(*args)
