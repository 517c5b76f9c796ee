"""CPU-side checks of packet mode in the PCM gateway (include/nutls.h, "Packet mode"): the eight entries are declared, exported, bound and
listed; ``nutls_pcm_packet_plan`` equals the brute-force simulation of the FIFO arithmetic (tests/packet_reference.py) for EVERY accepted
packet length at all four rates in all formats; every refusal of the length rule names the entry and writes nothing; the entries that take
a handle refuse a null one; the kernels' source is part of the build.  No reference counterpart: the reference takes float samples at 16 kHz
in hops only (dnn_model/interpreter_proposed.py:384-385)."""
import ctypes
import os
import re

import pytest

import packet_reference as PK
from nunet_amd import runner
from nunet_amd.build import SOURCES, build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NUTLS_ERR_ARG = runner.NUTLS_ERR_ARG
FMT = {"float32": 0, "int16": 1, "ulaw": 2, "alaw": 3}
BYTES = {"float32": 4, "int16": 2, "ulaw": 1, "alaw": 1}
RATES = (8000, 16000, 32000, 48000)
SIGNATURES = {
    "nutls_pcm_packet_plan": "int rate_hz, int sample_format, int samples, int* delay, int* rounds, int* fifo",
    "nutls_set_pcm_packet": "nutls_handle* h, int samples",
    "nutls_pcm_packet_samples": "nutls_handle* h",
    "nutls_pcm_packet_delay_samples": "nutls_handle* h",
    "nutls_pcm_packet_fill": "nutls_handle* h, int* fill, int n",
    "nutls_pcm_packet_last_rounds": "nutls_handle* h",
    "nutls_enhance_packet_pcm": "nutls_handle* h, const void* pcm_in, void* pcm_out, const unsigned char* active, int dc_mode, void* stream",
    "nutls_enhance_packet_pcm_host": "nutls_handle* h, const void* pcm_in, void* pcm_out, const unsigned char* active, int dc_mode",
}


@pytest.fixture(scope="module")
def lib():
    build()
    return runner.load_library()


def formats(rate):
    return ("float32", "int16", "ulaw", "alaw") if rate == 8000 else ("float32", "int16")


def plan_of(lib, rate, fmt, P):
    d, r, f = ctypes.c_int(-7), ctypes.c_int(-7), ctypes.c_int(-7)
    rc = lib.nutls_pcm_packet_plan(rate, FMT[fmt], P, ctypes.byref(d), ctypes.byref(r), ctypes.byref(f))
    return rc, {"delay": d.value, "rounds": r.value, "fifo": f.value}


def test_the_eight_entries_are_declared_exported_bound_and_listed(lib):
    hdr = open(os.path.join(ROOT, "include", "nutls.h")).read()
    declared = dict(re.findall(r"^int (nutls_[a-z_0-9]+)\(([^)]*)\);", hdr, re.M))
    for name, params in SIGNATURES.items():
        assert " ".join(declared.get(name, "").split()) == params, name
        assert name in runner.ABI_SYMBOLS, name
        fn = getattr(lib, name)      # AttributeError: not exported
        assert fn.argtypes is not None and len(fn.argtypes) == params.count(",") + 1 and fn.restype is ctypes.c_int, name
    # the new text stands at the end of the "PCM gateway" section, behind the ragged entries and in front of the next section
    at = [hdr.index("int %s(" % n) for n in SIGNATURES]
    assert hdr.index("int nutls_pcm_encode_block_ragged(") < min(at) and max(at) < hdr.index("/* ---- Attenuation limit")
    flat = " ".join(hdr.replace("\n * ", " ").split())
    for text in ("D = S - g samples of silence", "fill_in + fill_out = D", "R = floor((S - g + P) / S)", "1 <= P <= 4 S", "is a multiple of 16",
                 "until nutls_reset(h, -1) or nutls_set_pcm_packet"):
        assert text in flat, text


def test_the_kernels_are_part_of_the_build():
    assert "packet.hip" in SOURCES
    for name in ("packet.hip", "packet.hpp"):
        assert os.path.exists(os.path.join(os.path.dirname(os.path.abspath(runner.__file__)), "csrc", name)), name


@pytest.mark.parametrize("rate", RATES)
def test_plan_equals_the_brute_force_simulation_for_every_accepted_length(lib, rate):
    S = 256 * rate // 16000
    checked = 0
    for fmt in formats(rate):
        for P in range(1, 4 * S + 1):
            if not PK.accepted(P, S, BYTES[fmt]):
                continue
            rc, got = plan_of(lib, rate, fmt, P)
            assert rc == 0, (rate, fmt, P, lib.nutls_last_error())
            assert got == PK.plan(P, S) == PK.brute_force(P, S), (rate, fmt, P)
            assert 1 <= got["rounds"] <= 4 and got["fifo"] == got["delay"] + P
            checked += 1
    assert checked == sum(4 * S * BYTES[f] // 16 for f in formats(rate))
    assert runner.pcm_packet_plan(rate, "int16", S, lib) == {"delay": 0, "rounds": 1, "fifo": S}


def test_the_pairs_of_the_contract_over_5000_ticks():
    """The facts the header states, by brute force over 5 000 ticks -- pairs the length rule refuses included: the arithmetic is general."""
    for P, S in ((160, 128), (80, 128), (240, 128), (480, 768), (960, 768), (320, 256), (160, 256), (128, 128), (256, 128), (441, 768), (1, 128),
                 (2048, 128), (100, 128)):
        assert PK.brute_force(P, S, 5000) == PK.plan(P, S), (P, S)
    assert PK.plan(160, 128) == {"delay": 96, "rounds": 2, "fifo": 256}
    assert PK.plan(80, 128) == {"delay": 112, "rounds": 1, "fifo": 192}
    assert PK.plan(480, 768) == {"delay": 672, "rounds": 1, "fifo": 1152}
    assert PK.plan(1024, 256) == {"delay": 0, "rounds": 4, "fifo": 1024}


def test_every_refusal_of_the_length_rule(lib):
    cases = [(8000, "ulaw", 0), (8000, "ulaw", -16), (8000, "ulaw", 4 * 128 + 16), (8000, "ulaw", 8), (8000, "ulaw", 100), (8000, "ulaw", 161),
             (8000, "int16", 4), (8000, "int16", 100), (8000, "int16", 4 * 128 + 8), (8000, "float32", 2), (8000, "float32", 4 * 128 + 4),
             (16000, "float32", 441), (16000, "int16", 1), (16000, "float32", 4 * 256 + 4), (48000, "int16", 441), (48000, "float32", 4 * 768 + 4),
             (32000, "int16", 0), (16000, "ulaw", 160), (48000, "alaw", 480), (44100, "int16", 440), (0, "float32", 160)]
    for rate, fmt, P in cases:
        rc, got = plan_of(lib, rate, fmt, P)
        assert rc == NUTLS_ERR_ARG and got == {"delay": -7, "rounds": -7, "fifo": -7}, (rate, fmt, P)
        assert lib.nutls_last_error().decode().startswith("nutls_pcm_packet_plan: "), (rate, fmt, P)
    assert lib.nutls_pcm_packet_plan(8000, 7, 160, None, None, None) == NUTLS_ERR_ARG      # an unknown format
    assert lib.nutls_pcm_packet_plan(8000, FMT["ulaw"], 160, None, None, None) == 0          # (every pointer may be NULL)
    with pytest.raises(ValueError):
        runner.pcm_packet_plan(8000, "ulaw", 100, lib)
    with pytest.raises(ValueError):
        runner.pcm_packet_plan(8000, "float64", 160, lib)
    # the lengths next to the ends of the rule are accepted
    for rate, fmt, P in ((8000, "ulaw", 16), (8000, "ulaw", 512), (8000, "int16", 8), (16000, "float32", 4), (48000, "float32", 3072)):
        assert plan_of(lib, rate, fmt, P)[0] == 0, (rate, fmt, P)


def test_null_handle_returns(lib):
    fill = (ctypes.c_int * 4)(5, 5, 5, 5)
    buf = ctypes.create_string_buffer(64)
    for rc in (lib.nutls_set_pcm_packet(None, 160), lib.nutls_pcm_packet_samples(None), lib.nutls_pcm_packet_delay_samples(None),
               lib.nutls_pcm_packet_last_rounds(None), lib.nutls_pcm_packet_fill(None, fill, 4),
               lib.nutls_enhance_packet_pcm(None, ctypes.addressof(buf), ctypes.addressof(buf), None, 0, None),
               lib.nutls_enhance_packet_pcm_host(None, ctypes.addressof(buf), ctypes.addressof(buf), None, 0)):
        assert rc == NUTLS_ERR_ARG
        assert b"null" in lib.nutls_last_error()
    assert list(fill) == [5, 5, 5, 5]
