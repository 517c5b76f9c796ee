"""CPU-side checks of the per-stream active mask's entry points (include/nutls.h, nutls_step_active): the four symbols are declared,
exported and bound, and they validate before touching a device.  No reference counterpart: the reference steps one stream per call
(dnn_model/interpreter_proposed.py:215), the batch dimension -- and with it a stream's own clock -- is this project's addition."""
import ctypes
import os
import re

import numpy as np
import pytest

from nunet_amd import runner
from nunet_amd.build import build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("nutls_step_active", "nutls_step_host_active", "nutls_enhance_hop_active", "nutls_enhance_hop_host_active")


@pytest.fixture(scope="module")
def lib():
    build()
    return runner.load_library()


def test_the_four_symbols_are_declared_exported_and_bound(lib):
    hdr = open(os.path.join(ROOT, "include", "nutls.h")).read()
    declared = set(re.findall(r"^int (nutls_[a-z_]+)\(", hdr, re.M))
    for name in ENTRIES:
        assert name in declared, name
        assert name in runner.ABI_SYMBOLS, name
        fn = getattr(lib, name)
        assert fn.argtypes is not None and fn.restype is ctypes.c_int, name


def test_a_null_handle_is_an_argument_error_with_a_message(lib):
    mask = np.ones(4, np.uint8)
    for m in (None, mask.ctypes.data):          # (without a mask the call IS the unmasked entry: it answers for it)
        assert lib.nutls_step_active(None, None, None, m, None) == -1
        assert b"null" in lib.nutls_last_error()
        assert lib.nutls_step_host_active(None, None, None, m) == -1
        assert b"null" in lib.nutls_last_error()
        assert lib.nutls_enhance_hop_active(None, None, None, m, 0, None) == -1
        assert b"null" in lib.nutls_last_error()
        assert lib.nutls_enhance_hop_host_active(None, None, None, m, 0) == -1
        assert b"null" in lib.nutls_last_error()
    assert b"nutls_enhance_hop_host_active" in lib.nutls_last_error()


def test_python_checks_the_mask_before_the_library_is_called():
    """A wrong length or dtype raises ValueError in the wrapper: exercised on an engine object that has no handle at all."""
    eng = runner.NutlsEngine.__new__(runner.NutlsEngine)
    eng.batch = 4
    assert eng._host_mask(np.array([1, 0, 1, 1], np.uint8)).tolist() == [1, 0, 1, 1]
    assert eng._host_mask(np.array([True, False, True, True])).tolist() == [1, 0, 1, 1]
    with pytest.raises(ValueError, match="length 4"):
        eng._host_mask(np.ones(5, np.uint8))
    with pytest.raises(ValueError, match="length 4"):
        eng._host_mask(np.ones((4, 1), np.uint8))
    with pytest.raises(ValueError, match="bool / uint8"):
        eng._host_mask(np.ones(4, np.float32))
    with pytest.raises(ValueError, match="bool / uint8"):
        eng._host_mask([1, 0, 1, 1])
    eng._h = None      # (nothing for __del__ to release)
