"""CPU-side checks of the waveform block mode (PCM in, PCM out for offline handles): the four C entries exist, are
declared to the ctypes wrapper and validate their arguments before touching a device; the Python surface is there."""
import ctypes

import pytest

import nunet_amd
from nunet_amd import runner
from nunet_amd.build import build

NAMES = ("nutls_enhance_block", "nutls_enhance_block_host", "nutls_stft_block", "nutls_istft_block")


@pytest.fixture(scope="module")
def lib():
    build()
    return runner.load_library()


def test_the_four_entries_are_exported_and_listed(lib):
    for name in NAMES:
        assert name in runner.ABI_SYMBOLS, name
        assert getattr(lib, name) is not None
        assert getattr(lib, name).argtypes is not None, name


def test_null_arguments_are_reported_before_any_device_work(lib):
    assert lib.nutls_enhance_block_host(None, None, None, 1, 0) == -1
    assert lib.nutls_last_error()
    assert b"nutls_enhance_block_host" in lib.nutls_last_error()
    assert lib.nutls_stft_block(None, None, None, 1, None) == -1
    assert lib.nutls_last_error()
    assert b"nutls_stft_block" in lib.nutls_last_error()
    assert lib.nutls_istft_block(None, None, None, 1, 0, None) == -1
    assert lib.nutls_last_error()
    assert b"nutls_istft_block" in lib.nutls_last_error()
    assert lib.nutls_enhance_block(None, None, None, 1, 0, None) == -1
    assert b"nutls_enhance_block" in lib.nutls_last_error()


def test_offline_class_has_the_waveform_methods():
    for name in ("enhance", "enhance_block_device", "stft_block_device", "istft_block_device", "enhance_block_host", "debug_get"):
        assert callable(getattr(nunet_amd.NutlsOffline, name, None)), name
    from nunet_amd import stream_enhance as SE
    assert callable(SE.enhance_utterances_offline)


def test_quality_harness_rejects_an_unknown_engine(tmp_path):
    from nunet_amd.evaluate import evaluate_directory
    with pytest.raises(ValueError, match="engine"):
        evaluate_directory(str(tmp_path), engine="nonsense")
