"""CPU test (no GPU): the rule by which the library picks an instantiation of the two per-layer conv kernels (``conv_choose`` in
csrc/kernels.hip, reached through ``nutls_conv_dispatch``) is pinned to the rule the launch code held before one function owned it.

``_rule`` below restates that launch code (``launch_conv_t`` as of the commit before ``conv_choose`` existed) line by line, with the kinds'
compile-time shapes as literals; every sweep is compared against it, and the edges the rule turns on are also written out as numbers."""
import ctypes

import pytest

from nunet_amd.build import build
from nunet_amd import runner
from nunet_amd.runner import CONV_KINDS, conv_dispatch

#            kind        cin  nt stride tt kf   (conv_shape / the template arguments of launch_conv)
SHAPES = {"el_c32": (32, 1, 2, 2, 3), "el_c64": (64, 1, 2, 2, 3), "el_c128": (128, 1, 2, 2, 3), "dl_n64": (64, 2, 1, 2, 3),
          "dl_n128": (64, 4, 1, 2, 3), "in_c64": (64, 2, 1, 1, 1), "in_c128": (128, 2, 1, 1, 1), "down": (64, 2, 2, 1, 3),
          "up_even": (128, 4, 1, 1, 2), "up_odd": (128, 4, 1, 1, 1)}
F_OUTS = (1, 2, 4, 8, 16, 32, 64, 128, 256)


@pytest.fixture(scope="module", autouse=True)
def lib():
    build()
    return runner.load_library()


def _lds(kind, f_out, nw, bf16):
    cin, nt, stride, tt, kf = SHAPES[kind]
    cc = min(cin, 64)
    tp = 32 * nw
    seg = min(f_out, tp)
    nseg = tp // seg
    rs = seg + kf - 1 if stride == 1 else seg + (kf - 1) // 2
    if bf16:
        return nseg * rs * (3 * (cc if stride == 1 else 2 * cc) * 2 + 16)
    return nseg * rs * ((cc + 4) if stride == 1 else (2 * cc + 4)) * 4


def _rule(kind, B, f_out, bf16, ksplit=True):
    """(NW, ALL, tile, grid, LDS bytes) as the former launch code chose them; thresholds 64 * 512 (bf16) and 128 * 512 (fp32)"""
    total = B * f_out
    if not bf16:
        nw = 4 if total >= 128 * 512 else 1
        return nw, 0, 32 * nw, (total + 32 * nw - 1) // (32 * nw), _lds(kind, f_out, nw, False)
    if total >= 64 * 512:
        return 4, 0, 128, (total + 127) // 128, _lds(kind, f_out, 4, True)
    cin, nt, stride, tt, kf = SHAPES[kind]
    cc = min(cin, 64)
    nph, wph = tt * (cin // cc), kf * (cc // 16) * nt
    ldsb = _lds(kind, f_out, 1, True)
    phase_b = (ldsb + 255) & ~255
    grid = (total + 31) // 32
    if (nph * kf * (cc // 16)) % 4 == 0 and nph * wph <= 192:
        need = max(nph * phase_b, 3 * nt * 4096)
        if ksplit and need <= 128 * 1024:
            return 4, 1, 32, grid, need
    if nph > 1 and nph * wph <= 48 and nph * phase_b <= 64 * 1024:
        return 1, 1, 32, grid, nph * phase_b
    return 1, 0, 32, grid, ldsb


# The one place where the rule departs from the former launch code: the 128-position image of these (kind, F_out) on the bf16 pipe is
# 128 segments x 2 row pairs x 784 B = 200 704 B, more than the 160 KiB of LDS a workgroup can have -- the former code chose a launch that
# could not start (32 768 or more dense streams: no test and no benchmark ever got there).  They stay on the 32-position tiles.
TOO_LARGE_FOR_128 = {("el_c64", 1): (4, 1, 32), ("el_c128", 1): (1, 0, 32), ("down", 1): (4, 1, 32)}          # -> (NW, ALL, tile) they run instead
LDS_MAX = 160 * 1024


def _got(kind, B, f_out, bf16, **kw):
    d = conv_dispatch(kind, B, f_out, bf16=bf16, **kw)
    return d["nw"], d["all"], d["tile"], d["grid"], d["lds"]


def test_kinds_are_the_librarys():
    assert CONV_KINDS == tuple(SHAPES) and len(CONV_KINDS) == 10


def test_both_thresholds_at_their_exact_edges():
    """bf16: 128-position tiles iff B * F_out >= 32 768; fp32: iff >= 65 536 -- for every kind, at every F_out, one position below / at the edge
    (B = edge / F_out - 1 and B = edge / F_out)."""
    for kind in CONV_KINDS:
        for f_out in F_OUTS:
            for bf16, edge in ((True, 32768), (False, 65536)):
                below, at = _got(kind, edge // f_out - 1, f_out, bf16), _got(kind, edge // f_out, f_out, bf16)
                assert below[2] == 32 and (below[0], below[1]) != (4, 0), (kind, f_out, bf16, below)
                assert below == _rule(kind, edge // f_out - 1, f_out, bf16)
                want = _rule(kind, edge // f_out, f_out, bf16)
                assert (want[0], want[1], want[2]) == (4, 0, 128)
                if bf16 and (kind, f_out) in TOO_LARGE_FOR_128:
                    assert want[4] == 200704 and at[:3] == TOO_LARGE_FOR_128[kind, f_out] and at[3] == 1024 and at[4] == below[4], (kind, f_out, at)
                else:
                    assert at == want and at[4] <= LDS_MAX, (kind, f_out, bf16, at)
    assert {(k, f) for k in CONV_KINDS for f in F_OUTS for bf16 in (True, False) if _lds(k, f, 4, bf16) > LDS_MAX} == set(TOO_LARGE_FOR_128)
    assert all(_lds(k, f, 4, False) <= LDS_MAX for k in CONV_KINDS for f in F_OUTS)
    # the literal edges at F_out = 1
    assert _got("dl_n64", 32767, 1, True)[:3] == (4, 1, 32) and _got("dl_n64", 32768, 1, True)[:3] == (4, 0, 128)
    assert _got("dl_n64", 65535, 1, False)[:3] == (1, 0, 32) and _got("dl_n64", 65536, 1, False)[:3] == (4, 0, 128)
    assert _got("dl_n64", 65535, 1, True)[:3] == (4, 0, 128) and _got("dl_n64", 32768, 1, False)[:3] == (1, 0, 32)


def test_grid_sizes_for_a_non_multiple_of_the_tile():
    # 5 utterances x 205 frames: 1025 streams
    assert _got("in_c64", 1025, 32, True)[2:4] == (128, 257)           # 32 800 positions = 256 tiles + 32 positions
    assert _got("in_c64", 1025, 64, True)[2:4] == (128, 513)           # 65 600 = 512 tiles + 64
    assert _got("in_c64", 1025, 16, True)[2:4] == (32, 513)            # 16 400 = 512 tiles of 32 + 16
    assert _got("in_c64", 1025, 64, False)[2:4] == (128, 513)
    assert _got("in_c64", 1025, 32, False)[2:4] == (32, 1025)
    assert _got("el_c32", 27, 1, True)[2:4] == (32, 1) and _got("el_c32", 33, 1, True)[2:4] == (32, 2)
    assert _got("up_odd", 3, 128, False)[2:4] == (32, 12) and _got("up_odd", 3, 128, False, tile_min=0)[2:4] == (128, 3)
    assert _got("el_c32", 27, 8, True, tile_min=0)[2:4] == (128, 2)    # 216 positions: one full tile, one of 88


def test_default_rule_all_kinds_all_sizes():
    """The K split is chosen for all ten kinds wherever its image fits 128 KiB -- everywhere but `el_c128` at F_out <= 2 --, F_out = 1 .. 256,
    at one stream, an odd few and just below the tile threshold; LDS bytes and grids as the former launch code computed them."""
    for kind in CONV_KINDS:
        for f_out in F_OUTS:
            for B in (1, 3, 27, 32767 // f_out):
                got = _got(kind, B, f_out, True)
                assert got == _rule(kind, B, f_out, True), (kind, B, f_out)
                if kind == "el_c128" and f_out <= 2:
                    assert got[:3] == (1, 0, 32), (kind, f_out, got)
                else:
                    assert got[:3] == (4, 1, 32) and got[4] <= 128 * 1024, (kind, f_out, got)
                assert _got(kind, B, f_out, False) == _rule(kind, B, f_out, False), (kind, B, f_out)
    # the tightest K-split image of the network, and the two sizes behind it (which no layer of the network has)
    assert _got("el_c128", 8, 4, True) == (4, 1, 32, 1, 125952)
    assert _got("el_c128", 8, 2, True) == (1, 0, 32, 1, 37632)          # 4 x 37 632 = 150 528 > 131 072, and > 65 536 for <1, true>
    assert _got("el_c128", 8, 1, True) == (1, 0, 32, 1, 50176)
    # the exchange buffer sets the size where the image is smaller: 3 waves x NT x 4 KiB
    assert _got("up_odd", 1, 1, True) == (4, 1, 32, 1, 49152)


def test_one_wave_choices_without_the_k_split():
    """NUTLS_OFFLINE_KSPLIT=0: <1, true> (all phases resident) for the kinds with more than one phase and at most 48 weight fragments --
    el_c32, el_c64, el_c128, dl_n64, in_c128, up_odd -- while the phases fit 64 KiB, <1, false> otherwise."""
    has_all1 = {"el_c32", "el_c64", "el_c128", "dl_n64", "in_c128", "up_odd"}
    seen = set()
    for kind in CONV_KINDS:
        for f_out in F_OUTS:
            for B in (1, 27, 32767 // f_out):
                got = _got(kind, B, f_out, True, ksplit=False)
                assert got == _rule(kind, B, f_out, True, ksplit=False), (kind, B, f_out)
                assert got[0] == 1 and got[2] == 32
                assert got[1] == 0 or (kind in has_all1 and got[4] <= 64 * 1024), (kind, f_out, got)
                seen.add((kind, got[1]))
    # el_c128 qualifies by its weights but its four phases never fit; el_c32, in_c128 and up_odd fit at every size
    assert seen == {("el_c32", 1), ("el_c64", 0), ("el_c64", 1), ("el_c128", 0), ("dl_n64", 0), ("dl_n64", 1), ("dl_n128", 0), ("in_c64", 0),
                    ("in_c128", 1), ("down", 0), ("up_even", 0), ("up_odd", 1)}
    # where <1, true> gives way to <1, false>: el_c64 keeps two phases of 31 488 B at F_out = 4 and would need two of 37 632 B at F_out = 2
    assert _got("el_c64", 27, 4, True, ksplit=False) == (1, 1, 32, 4, 62976)
    assert _got("el_c64", 27, 2, True, ksplit=False) == (1, 0, 32, 2, 37632)
    # el_c128 has four phases: 4 x 26 112 B at F_out >= 32 is past 64 KiB at every size
    assert all(_got("el_c128", 3, f, True, ksplit=False)[:2] == (1, 0) for f in F_OUTS)
    # the fp32 kernel does not know the knob
    assert _got("el_c64", 27, 4, False, ksplit=False) == _got("el_c64", 27, 4, False)


def test_tile_knob_forces_the_tiles_everywhere_or_nowhere():
    for kind in CONV_KINDS:
        for f_out in F_OUTS:
            for bf16 in (True, False):
                forced = _got(kind, 1, f_out, bf16, tile_min=0)
                assert forced[:3] == (TOO_LARGE_FOR_128[kind, f_out] if bf16 and (kind, f_out) in TOO_LARGE_FOR_128 else (4, 0, 128)), (kind, f_out, bf16, forced)
                big = _got(kind, 1 << 20, f_out, bf16, tile_min=1 << 40)
                assert big[2] == 32 and big == _got(kind, 1 << 20, f_out, bf16, tile_min=1 << 40, ksplit=True)
                assert _got(kind, 1 << 20, f_out, bf16)[:3] == (TOO_LARGE_FOR_128[kind, f_out] if bf16 and (kind, f_out) in TOO_LARGE_FOR_128 else (4, 0, 128))
    assert _got("in_c64", 2, 64, True, tile_min=128)[:3] == (4, 0, 128) and _got("in_c64", 1, 64, True, tile_min=128)[:3] == (4, 1, 32)


def test_bad_arguments(lib):
    i = ctypes.c_int()
    assert lib.nutls_conv_dispatch(10, 1, 1, 1, 1, -1, ctypes.byref(i), None, None, None, None) == runner.NUTLS_ERR_ARG
    assert lib.nutls_conv_dispatch(-1, 1, 1, 1, 1, -1, None, None, None, None, None) == runner.NUTLS_ERR_ARG
    assert lib.nutls_conv_dispatch(0, 0, 1, 1, 1, -1, None, None, None, None, None) == runner.NUTLS_ERR_ARG
    assert lib.nutls_conv_dispatch(0, 1, 3, 1, 1, -1, None, None, None, None, None) == runner.NUTLS_ERR_ARG
    assert b"nutls_conv_dispatch" in lib.nutls_last_error()
    assert lib.nutls_conv_dispatch(0, 1, 4, 1, 1, -1, None, None, None, None, None) == 0
    assert lib.nutls_launch_conv_shape(None, 0, None, None) == runner.NUTLS_ERR_ARG
