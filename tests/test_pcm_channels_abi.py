"""CPU-side checks of the channels of the PCM gateway (include/nutls.h, "Channels"): the four entries are declared with their signatures,
exported, bound, listed and stand where the header's sections say; the kernels' source is part of the build; ``nutls_pcm_deinterleave`` and
``nutls_pcm_interleave`` equal the numpy transpose (tests/channels_reference.py) on the raw bytes in all four formats, for 2 and 4 channels
and lengths around a quad, and each is the other's inverse; every refusal returns NUTLS_ERR_ARG, names its entry and writes nothing; the two
entries that take a handle refuse a null one.  No reference counterpart: the reference takes one float row per call
(dnn_model/interpreter_proposed.py:384-385)."""
import ctypes
import os
import re

import numpy as np
import pytest

import channels_reference as CH
from nunet_amd import runner
from nunet_amd.build import SOURCES, build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NUTLS_ERR_ARG = runner.NUTLS_ERR_ARG
FMT = {"float32": 0, "int16": 1, "ulaw": 2, "alaw": 3}
DTYPE = {"float32": np.float32, "int16": np.int16, "ulaw": np.uint8, "alaw": np.uint8}
LENGTHS = (0, 1, 15, 16, 17, 1000)
SIGNATURES = {
    "nutls_set_pcm_channels": "nutls_handle* h, int channels",
    "nutls_pcm_channels": "nutls_handle* h",
    "nutls_pcm_deinterleave": "int sample_format, int channels, const void* frames, void* rows, size_t n",
    "nutls_pcm_interleave": "int sample_format, int channels, const void* rows, void* frames, size_t n",
}


@pytest.fixture(scope="module")
def lib():
    build()
    return runner.load_library()


def samples(fmt, shape, seed):
    """Every byte pattern counts: floats include NaNs with payloads, infinities and -0.0."""
    rng = np.random.default_rng(seed)
    raw = rng.integers(0, 256, size=int(np.prod(shape)) * np.dtype(DTYPE[fmt]).itemsize, dtype=np.uint8)
    x = raw.view(DTYPE[fmt]).reshape(shape).copy()
    if fmt == "float32" and x.size >= 4:
        flat = x.reshape(-1).view(np.uint32)
        flat[0], flat[1], flat[2], flat[-1] = 0x7FC12345, 0xFFA00001, 0x80000000, 0x7F800000      # quiet and signalling NaN payloads, -0.0, inf
    return x


def call(lib, name, fmt, channels, src, dst, n):
    return getattr(lib, name)(fmt, channels, None if src is None else src.ctypes.data, None if dst is None else dst.ctypes.data, n)


def test_the_four_entries_are_declared_exported_bound_and_listed(lib):
    hdr = open(os.path.join(ROOT, "include", "nutls.h")).read()
    declared = dict(re.findall(r"^int (nutls_[a-z_0-9]+)\(([^)]*)\);", hdr, re.M))
    for name, params in SIGNATURES.items():
        assert " ".join(declared.get(name, "").split()) == params, name
        assert name in runner.ABI_SYMBOLS, name
        fn = getattr(lib, name)      # AttributeError: not exported
        assert fn.argtypes is not None and len(fn.argtypes) == params.count(",") + 1 and fn.restype is ctypes.c_int, name
    # the section stands behind the packet entries and in front of the attenuation limit
    at = [hdr.index("int %s(" % n) for n in SIGNATURES]
    assert hdr.index("int nutls_enhance_packet_pcm_host(") < hdr.index("/* ---- Channels") < min(at)
    assert max(at) < hdr.index("/* ---- Attenuation limit")
    flat = " ".join(hdr.replace("\n * ", " ").split())
    for text in ("sample i of stream r * C + c is at column i * C + c of row r", "E_C(x) == interleave(E_1(deinterleave(x))) in every bit",
                 "HAVE NO EFFECT", "survives nutls_reset and nutls_set_pcm_format", "Setting the value in force is a no-op",
                 "pcm_in == pcm_out (the same base pointer) stays allowed"):
        assert text in flat, text


def test_the_kernels_are_part_of_the_build():
    assert "channels.hip" in SOURCES
    for name in ("channels.hip", "channels.hpp"):
        assert os.path.exists(os.path.join(os.path.dirname(os.path.abspath(runner.__file__)), "csrc", name)), name


@pytest.mark.parametrize("fmt", sorted(FMT))
@pytest.mark.parametrize("channels", (2, 4))
def test_the_host_functions_are_the_transpose_and_each_others_inverse(lib, fmt, channels):
    for n in LENGTHS:
        frames = samples(fmt, (n, channels), 1000 * channels + n)
        want = CH.deinterleave(frames)
        rows = np.full((channels, n), 0x5A, np.uint8).repeat(frames.itemsize, axis=1).view(frames.dtype)
        assert call(lib, "nutls_pcm_deinterleave", FMT[fmt], channels, frames, rows, n) == 0, lib.nutls_last_error()
        assert rows.tobytes() == want.tobytes(), (fmt, channels, n)
        back = np.empty_like(frames)
        assert call(lib, "nutls_pcm_interleave", FMT[fmt], channels, rows, back, n) == 0, lib.nutls_last_error()
        assert back.tobytes() == frames.tobytes() == CH.interleave(want).tobytes(), (fmt, channels, n)
        if n and fmt != "alaw":      # the Python wrappers: a dtype names the sample size (a byte is a byte in either law)
            assert runner.pcm_deinterleave(frames, lib).tobytes() == want.tobytes()
            assert runner.pcm_interleave(want, lib).tobytes() == frames.tobytes()


def test_the_reference_helpers_are_the_rule_of_the_header():
    """Sample i of stream r * C + c is at column i * C + c of row r."""
    for channels in (2, 4):
        rows, n = 2 * channels, 5
        x = np.arange(rows * n, dtype=np.int16).reshape(rows // channels, n * channels)
        split = CH.split_rows(x, channels)
        for r in range(rows // channels):
            for c in range(channels):
                for i in range(n):
                    assert split[r * channels + c, i] == x[r, i * channels + c]
        assert (CH.join_rows(split, channels) == x).all()
        assert (CH.split_rows(x.reshape(rows // channels, n, channels), channels) == split).all()


def test_every_refusal_names_its_entry_and_writes_nothing(lib):
    n = 16
    for name in ("nutls_pcm_deinterleave", "nutls_pcm_interleave"):
        src = samples("int16", (n, 8), 7)
        for fmt, channels, has_src, has_dst in [(1, 0, True, True), (1, 1, True, True), (1, 3, True, True), (1, 8, True, True), (1, -2, True, True),
                                                (4, 2, True, True), (-1, 2, True, True), (7, 4, True, True),
                                                (1, 2, False, True), (1, 2, True, False), (0, 4, False, False)]:
            dst = np.full(n * 8, 0x5A5A, np.uint16)
            rc = call(lib, name, fmt, channels, src if has_src else None, dst if has_dst else None, n)
            assert rc == NUTLS_ERR_ARG, (name, fmt, channels, has_src, has_dst)
            assert lib.nutls_last_error().decode().startswith(name + ": "), (name, lib.nutls_last_error())
            assert (dst == 0x5A5A).all(), (name, fmt, channels)
    with pytest.raises(ValueError):
        runner.pcm_deinterleave(np.zeros((16, 3), np.int16), lib)
    with pytest.raises(ValueError):
        runner.pcm_interleave(np.zeros((1, 16), np.float32), lib)
    with pytest.raises(ValueError):
        runner.pcm_deinterleave(np.zeros((16, 2), np.float64), lib)


def test_null_handle_returns(lib):
    for name, refused in (("nutls_set_pcm_channels", lambda: lib.nutls_set_pcm_channels(None, 2)), ("nutls_pcm_channels", lambda: lib.nutls_pcm_channels(None))):
        assert refused() == NUTLS_ERR_ARG, name
        err = lib.nutls_last_error()
        assert err.decode().startswith(name + ": ") and b"null" in err, err
