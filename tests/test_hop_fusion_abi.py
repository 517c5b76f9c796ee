"""CPU-side checks of hop fusion's entry points (include/nutls.h, nutls_set_hop_fusion): the two symbols are declared, exported and
bound, they validate before touching a device, and the wave-level transform the hop builds share with the waveform block mode
(csrc/stft_wave.hpp) still is the one tools/check_stft_block_lds.py models.  No reference counterpart: the reference's loop runs its
STFT in numpy on the host (dnn_model/interpreter_proposed.py:203-213, 352-365); how many launches a hop takes is this project's concern."""
import ctypes
import os
import re

import pytest

from nunet_amd import runner
from nunet_amd.build import SOURCES, build
from tools import check_stft_block_lds as model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "nested-u-net-based-real-time-speech-enhancement-mobile-app_amd", "csrc")
ENTRIES = ("nutls_set_hop_fusion", "nutls_launches_per_hop")


@pytest.fixture(scope="module")
def lib():
    build()
    return runner.load_library()


def test_the_two_symbols_are_declared_exported_and_bound(lib):
    hdr = open(os.path.join(ROOT, "include", "nutls.h")).read()
    declared = set(re.findall(r"^int (nutls_[a-z_]+)\(", hdr, re.M))
    for name in ENTRIES:
        assert name in declared, name
        assert name in runner.ABI_SYMBOLS, name
        fn = getattr(lib, name)
        assert fn.argtypes is not None and fn.restype is ctypes.c_int, name
    assert callable(runner.NutlsEngine.set_hop_fusion) and isinstance(runner.NutlsEngine.launches_per_hop, property)


def test_a_null_handle_is_an_argument_error_with_a_message(lib):
    for enable in (0, 1):
        assert lib.nutls_set_hop_fusion(None, enable) == -1
        assert b"null" in lib.nutls_last_error()
    assert lib.nutls_launches_per_hop(None) == -1
    assert b"null" in lib.nutls_last_error()


def test_the_hop_builds_are_sources_of_the_library_and_nothing_else_defines_fz_hop():
    assert "fused_step_hop.hip" in SOURCES and "fused_step_g2_hop.hip" in SOURCES
    for f in sorted(os.listdir(CSRC)):
        if f.endswith(".hip") and f != "fused_step.hip":
            defines = re.search(r"^#define FZ_HOP 1$", open(os.path.join(CSRC, f)).read(), re.M) is not None
            assert defines == (f in ("fused_step_hop.hip", "fused_step_g2_hop.hip")), f


def test_shared_wave_transform_is_the_one_the_lds_model_describes():
    """stft_block.hip's wave-level code moved to stft_wave.hpp: the constants and index expressions the numpy model restates are there."""
    src = open(os.path.join(CSRC, "stft_wave.hpp")).read()
    assert int(re.search(r"constexpr int kWaveImage = (\d+);", src).group(1)) == model.IMAGE
    assert "return k ^ (((k >> 4) & 1) << 1) ^ ((k >> 5) & 1);" in src          # nat()
    assert "return k ^ ((k >> 4) & 1);" in src                                    # spec()
    for expr in ("80 * k0 + l0 + 16 * a", "80 * k0 + 20 * k1 + l00 + 4 * a", "80 * k0 + 20 * k1 + 4 * l00 + (q ^ l00)",
                 "80 * k0 + 20 * k1 + 4 * a + (l00 ^ a)"):
        assert expr in src, expr
    for user in ("stft_block.hip", "fused_step.hip"):
        assert '#include "stft_wave.hpp"' in open(os.path.join(CSRC, user)).read(), user
