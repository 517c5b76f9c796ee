"""``-m gpu``: every instantiation of the two per-layer conv kernels (csrc/kernels.hip: ``conv_bf16x3_kernel``, block mode on int8
containers; ``conv_mfma_kernel``, the streaming modes 0 / 1 and ``NUTLS_OFFLINE_FP32``) that this network can reach, each against oracle B
in float64 on synthetic weight families (tests/weight_families.py) -- every output frame of every utterance, all 130 carried states after
every block, and all 130 states in the MIDDLE of a block, read through ragged counts.

Which instantiation a launch runs is the library's own answer (``nunet_amd.runner.conv_dispatch`` = ``nutls_conv_dispatch``, the function
``launch_conv`` dispatches on; its default rule is pinned by tests/test_conv_dispatch.py), so coverage is asserted, not assumed.  Handles
read the developer knobs (``NUTLS_OFFLINE_FP32``, ``NUTLS_OFFLINE_KSPLIT``, ``NUTLS_CONV_TILE_MIN``) when they are created: one process
holds handles of every configuration.

Bounds: the project's own (tests/test_gpu_synthetic_weights.py) -- outputs RMS < 2e-5 x max(1, max|want|) per frame and utterance, each
state of each utterance RMS < 1e-4 x max(1, max|want|), device path against device path 1e-6 RMS.  tests/test_weight_families.py shows that
the float32 oracle uses at most 1/20 of the first two on every reference used here.  A failure names the first offending tensor in the
order of the per-layer plan: the layer whose kernel to read."""
import ctypes

import numpy as np
import pytest

import weight_families as WF
from test_gpu_synthetic_weights import DEVICE_RMS, LAST_OP, Ledger
from nunet_amd import NutlsEngine, NutlsOffline
from nunet_amd.runner import CONV_KINDS, conv_dispatch

pytestmark = pytest.mark.gpu

FP32, KSPLIT, TILE_MIN = "NUTLS_OFFLINE_FP32", "NUTLS_OFFLINE_KSPLIT", "NUTLS_CONV_TILE_MIN"
NOWHERE = 1 << 40          # a tile threshold no launch reaches
# the five handle configurations of the block mode: what conv_dispatch is asked, and the environment the handle is created under
CONFIGS = {
    "bf16, K split (default)": {"bf16": True, "ksplit": True, "tile_min": None},
    "bf16, 128-position tiles forced": {"bf16": True, "ksplit": True, "tile_min": 0},
    "bf16, KSPLIT=0": {"bf16": True, "ksplit": False, "tile_min": None},
    "fp32, 1-wave tiles": {"bf16": False, "ksplit": True, "tile_min": None},
    "fp32, 128-position tiles forced": {"bf16": False, "ksplit": True, "tile_min": 0},
}
F_OUTS = [1, 2, 4, 8, 16, 32, 64, 128, 256]
# compiled (the `if constexpr` conditions of launch_conv_t hold for the kind) but out of this network's reach: el_c32, in_c128 and up_odd keep
# all phases resident at every size, so their <1, false> never runs; el_c128's four phases never fit 64 KiB, so its <1, true> never runs
UNREACHABLE = {("bf16", "el_c32", 1, 0), ("bf16", "in_c128", 1, 0), ("bf16", "up_odd", 1, 0), ("bf16", "el_c128", 1, 1)}
HAS_ALL1 = ("el_c32", "el_c64", "el_c128", "dl_n64", "in_c128", "up_odd")


def _create(monkeypatch, cfg, make):
    """``make()`` under the environment of ``cfg``; the environment is cleared again (the handle has read it)"""
    for var, val in ((FP32, None if cfg["bf16"] else "1"), (KSPLIT, None if cfg["ksplit"] else "0"),
                     (TILE_MIN, None if cfg["tile_min"] is None else str(cfg["tile_min"]))):
        if val is None:
            monkeypatch.delenv(var, raising=False)
        else:
            monkeypatch.setenv(var, val)
    try:
        return make()
    finally:
        for var in (FP32, KSPLIT, TILE_MIN):
            monkeypatch.delenv(var, raising=False)


def _plan(h):
    """the per-layer plan as ``first_in_plan_order`` wants it: every launch's layer name, in issue order"""
    res, layer = [], ctypes.c_char_p()
    for i in range(h._lib.nutls_launches_per_step(h._h)):
        assert h._lib.nutls_launch_info(h._h, i, ctypes.byref(layer), None, None, None) == 0
        res.append({"layer": layer.value.decode()})
    return res


def _variant(cfg, kind, batch, f_out):
    d = conv_dispatch(kind, batch, f_out, bf16=cfg["bf16"], ksplit=cfg["ksplit"], tile_min=cfg["tile_min"])
    return ("bf16" if cfg["bf16"] else "fp32", kind, d["nw"], d["all"])


def _all_states(h):
    return {n: h.state_get(n) for n in WF.state_names()}


# ---- the sampled mid-block frames see full and partly filled 128-position tiles -------------------------------------------------------------
def _check_samples(launches):
    """Three-utterance set, 128-position tiles forced: for every F_out of the network the (utterance, frame) pairs whose states the ragged
    counts read include a position in the partly filled last tile of its launch wherever a launch has one (F_out <= 64: U n is odd) and a
    position in a full tile wherever a launch has one (F_out >= 8: at F_out <= 4 the 27 F_out positions of the largest block are one
    partly filled tile).  Tiles and grids are the library's (``conv_dispatch``)."""
    U, cfg = 3, WF.BLOCK_SETS[3]
    assert sorted({f for _, _, f in launches}) == F_OUTS
    for f_out in F_OUTS:
        kinds = sorted({k for _, k, f in launches if f == f_out})
        has = {"partial": False, "full": False}
        hit = {"partial": False, "full": False}
        for i, counts in cfg["ragged"].items():
            n = cfg["blocks"][i]
            assert max(counts) == n and all((U * m) % 2 == 1 for m in cfg["blocks"])
            total = U * n * f_out
            for k in kinds:
                d = conv_dispatch(k, U * n, f_out, bf16=True, tile_min=0)
                if (k, f_out) == ("el_c64", 1):          # its 128-position image would be 200 704 B of LDS: the K split at every size
                    assert (d["nw"], d["all"], d["tile"]) == (4, 1, 32), d
                    continue
                assert (d["nw"], d["all"], d["tile"], d["grid"]) == (4, 0, 128, -(-total // 128)), (k, f_out, d)
            n_full, partial = total // 128, total % 128 != 0
            has["partial"] |= partial
            has["full"] |= n_full > 0
            for u, c in enumerate(counts):
                first = (u * n + c - 1) * f_out
                tiles = range(first // 128, (first + f_out - 1) // 128 + 1)
                hit["partial"] |= partial and n_full in tiles
                hit["full"] |= any(t < n_full for t in tiles)
        assert has == {"partial": f_out <= 64, "full": f_out >= 8}, (f_out, has)
        assert hit == has, (f_out, hit, has)


# ---- a. block mode, five configurations -----------------------------------------------------------------------------------------------------
def _run_blocks(off, U):
    """The set's blocks, uniform; then, for every block that is also run ragged, the blocks in front of it again and that block with its
    counts.  -> outputs [U, frames, 256], all 130 states after every block, all 130 states after the ragged blocks, and per ragged block
    and utterance whether the rows it keeps are the uniform block's bits (the ragged block is the uniform block's launches)."""
    cfg, x, starts = WF.BLOCK_SETS[U], WF.block_set_inputs(U), WF.block_starts(U)
    outs, ends, mids, same = [], [], {}, {}
    for a, n in zip(starts, cfg["blocks"]):
        outs.append(off.process(x[:, a:a + n]))
        ends.append(_all_states(off))
    out = np.concatenate(outs, axis=1)
    for i, counts in cfg["ragged"].items():
        off.reset()
        for a, n in zip(starts[:i], cfg["blocks"][:i]):
            off.process(x[:, a:a + n])
        a = starts[i]
        got = off.process_ragged([x[u, a:a + c] for u, c in enumerate(counts)])
        for u, c in enumerate(counts):
            same[i, u] = np.array_equal(got[u], out[u, a:a + c])
        mids[i] = _all_states(off)
    return out, ends, mids, same


@pytest.mark.parametrize("U,family", [(U, f) for U in (2, 3) for f in WF.block_set_families(U)])
def test_block_mode_five_configurations(U, family, monkeypatch):
    """Each configuration on the two-utterance blocks (17, 1, 9) or the three-utterance blocks (9, 1, 7): against the float64 oracle every
    output frame of every utterance, all 130 states of every utterance after every block, and all 130 states at the mid-block frames the
    ragged counts select; the five configurations pairwise within 1e-6 RMS on every utterance's outputs."""
    blob, ref = WF.container(family), WF.block_reference(family, utterances=U)
    cfg, starts = WF.BLOCK_SETS[U], WF.block_starts(U)
    frames = sum(cfg["blocks"])
    led, outs, plan, launches = None, {}, None, None
    for name, c in CONFIGS.items():
        off = _create(monkeypatch, c, lambda: NutlsOffline(blob, max_frames=max(cfg["blocks"]), utterances=U))
        if led is None:
            plan, launches = _plan(off), off.conv_launches()
            led = Ledger("%s, block mode, %d utterances" % (family, U), plan)
            if U == 3:
                _check_samples(launches)
        assert off.conv_launches() == launches
        out, ends, mids, same = _run_blocks(off, U)
        off.close()
        assert out.shape == (U, frames, 256) and np.isfinite(out).all(), name
        outs[name] = out
        worst = {"outputs": 0.0, "states after a block": 0.0, "states inside a block": 0.0}

        def add(kind, label, op, ratio):
            led.add("%s: %s" % (name, label), op, ratio)
            worst[kind] = max(worst[kind], ratio if np.isfinite(ratio) else float("inf"))

        for f in range(frames):
            for u in range(U):
                add("outputs", "output, frame %d, utterance %d" % (f, u), LAST_OP, WF.scaled_rms(out[u, f], ref.out[f, u]) / WF.OUT_BOUND)
        for i, (a, n) in enumerate(zip(starts, cfg["blocks"])):
            want = ref.states_at[a + n - 1]
            for sn in WF.state_names():
                for u in range(U):
                    add("states after a block", "state %s after block %d, utterance %d" % (sn, i, u), WF.state_consumer(sn),
                        WF.scaled_rms(ends[i][sn][u].reshape(-1), want[sn][u].reshape(-1)) / WF.STATE_BOUND)
        for i, counts in cfg["ragged"].items():
            for u, cnt in enumerate(counts):
                want = ref.states_at[starts[i] + cnt - 1]
                for sn in WF.state_names():
                    add("states inside a block", "state %s after frame %d of block %d, utterance %d" % (sn, cnt, i, u), WF.state_consumer(sn),
                        WF.scaled_rms(mids[i][sn][u].reshape(-1), want[sn][u].reshape(-1)) / WF.STATE_BOUND)
        for (i, u), ok in same.items():
            led.add("%s: ragged block %d against the uniform block, kept output rows of utterance %d (bit for bit)" % (name, i, u), LAST_OP,
                    0.0 if ok else float("inf"), device=True)
        print("conv variants | %d utterances | %s | %s | worst ratio to the bound: outputs %.3f, states after a block %.3f, states inside a block %.3f"
              % (U, family, name, worst["outputs"], worst["states after a block"], worst["states inside a block"]))
    names = list(CONFIGS)
    for i, a in enumerate(names):
        for b in names[i + 1:]:
            for u in range(U):
                led.add("%s against %s, outputs of utterance %d" % (a, b, u), LAST_OP, WF.rms(outs[a][u], outs[b][u]) / DEVICE_RMS, device=True)
    assert len(led.ratio) == 5 * (U * frames + 130 * U * (3 + 2) + 2 * U) + 10 * U
    led.close()


# ---- b. coverage, asserted ----------------------------------------------------------------------------------------------------------------------
def test_every_reachable_instantiation_is_run():
    """The instantiations the block-mode test above runs (per configuration: the library's choice for every conv launch of the block plan at
    the dense stream count U n of every block of both sets) are, together, EVERY instantiation ``launch_conv`` can reach for this network's
    (kind, F_out) pairs at any stream count and knob setting; what is compiled beyond that is `UNREACHABLE`."""
    off = NutlsOffline(WF.container("plain"), max_frames=2, utterances=1)
    launches = off.conv_launches()
    off.close()
    pairs = sorted({(k, f) for _, k, f in launches})
    assert {k for k, _ in pairs} == set(CONV_KINDS) and len(launches) >= 116
    reachable = set()
    for k, f in pairs:
        for bf16 in (True, False):
            for ksplit in (True, False):
                for B in (1, 3, 27, 1025, max(1, 32767 // f), 32768 // f + 1, max(1, 65535 // f), 65536 // f + 1, 1 << 20):
                    reachable.add(_variant({"bf16": bf16, "ksplit": ksplit, "tile_min": None}, k, B, f))
    ran = {}
    for name, c in CONFIGS.items():
        ran[name] = {_variant(c, k, U * n, f) for _, k, f in launches for U in (2, 3) for n in WF.BLOCK_SETS[U]["blocks"]}
    union = set().union(*ran.values())
    compiled = {("bf16", k, nw, al) for k in CONV_KINDS for nw, al in ((4, 0), (4, 1), (1, 0))} | {("bf16", k, 1, 1) for k in HAS_ALL1} \
        | {("fp32", k, nw, 0) for k in CONV_KINDS for nw in (1, 4)}
    print("instantiation (pipe, kind, NW, ALL)           reachable  run by")
    for v in sorted(compiled):
        print("  %-5s %-8s <%d, %-5s>                    %-9s  %s" % (v[0], v[1], v[2], "true" if v[3] else "false", "yes" if v in reachable else "no",
                                                                   "; ".join(n for n in CONFIGS if v in ran[n]) or "-"))
    assert len(compiled) == 56 and reachable <= compiled
    assert compiled - reachable == UNREACHABLE
    assert union == reachable, (sorted(reachable - union), sorted(union - reachable))


# ---- c. streaming per-layer modes on the 128-position fp32 kernel ---------------------------------------------------------------------------
@pytest.mark.parametrize("form", [None, "float"])
def test_streaming_modes_on_forced_tiles(form, monkeypatch):
    """Three streams, plain launches and hipGraph replay with the tile knob at 0: every conv launch runs ``conv_mfma_kernel<..., 4>`` at 3 to
    768 positions (one partly filled tile at F_out <= 32, 1.5 tiles at 64).  Outputs and all 130 states of every stream against the float64
    oracle; graph replay equals plain launches bit for bit."""
    B = 3
    blob, ref, x = WF.container("plain", form), WF.reference("plain", form=form), WF.inputs(B)
    cfg = {"bf16": False, "ksplit": True, "tile_min": 0}
    a = _create(monkeypatch, cfg, lambda: NutlsEngine(blob, batch=B, mode="graph"))
    b = _create(monkeypatch, cfg, lambda: NutlsEngine(blob, batch=B, mode="launches"))
    for eng in (a, b):
        assert all(_variant(cfg, k, B, f) == ("fp32", k, 4, 0) for _, k, f in eng.conv_launches())
        assert all(p["family"].endswith("/w4") for p in eng.launch_plan() if p["family"].startswith("conv_"))
    assert sorted({f for _, _, f in a.conv_launches()}) == F_OUTS
    led = Ledger("plain (%s container), per-layer kernels on 128-position tiles" % (form or "shipped-form"), _plan(a))
    for f in range(WF.FRAMES):
        oa, ob = a.step(x[f]), b.step(x[f])
        assert np.array_equal(oa, ob), f
        for s in range(B):
            led.add("output, frame %d, stream %d" % (f, s), LAST_OP, WF.scaled_rms(oa[s], ref.out[f, s]) / WF.OUT_BOUND)
    led.states(a, ref.state, range(B))
    for name in WF.state_names():
        assert np.array_equal(a.state_get(name), b.state_get(name)), name
    a.close()
    b.close()
    assert len(led.ratio) == WF.FRAMES * B + 130 * B
    led.close()


# ---- d. the natural thresholds at real size, no knob -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("pipe", ["bf16", "fp32"])
def test_natural_thresholds_at_real_size(pipe, monkeypatch):
    """Five utterances x 205 frames in one block (1025 dense streams), default knobs: the bf16 launches with F_out >= 32 -- all ten kinds have
    one -- run 128-position tiles, partly filled at the end for F_out = 32 and 64 (fp32: F_out >= 64, partly filled at 64).  Outputs and all
    130 states of every utterance within 1e-6 RMS of a handle whose tile threshold no launch reaches (the K split / the 1-wave fp32 kernel
    everywhere, which the block-mode test holds against the oracle)."""
    U, n = 5, 205
    bf16 = pipe == "bf16"
    x = (0.25 * np.abs(np.random.default_rng(WF.SEED + 7).standard_normal((U, n, 256)))).astype(np.float32)
    blob = WF.container("plain")
    res = {}
    for which, tile_min in (("natural", None), ("small tiles", NOWHERE)):
        cfg = {"bf16": bf16, "ksplit": True, "tile_min": tile_min}
        off = _create(monkeypatch, cfg, lambda: NutlsOffline(blob, max_frames=n, utterances=U))
        launches = off.conv_launches()
        big = {}
        for _, k, f in launches:
            d = conv_dispatch(k, U * n, f, bf16=bf16, ksplit=True, tile_min=tile_min)
            if which == "natural":
                edge = 32 if bf16 else 64
                assert (d["nw"], d["all"], d["tile"]) == ((4, 0, 128) if f >= edge else (4, 1, 32) if bf16 else (1, 0, 32)), (k, f, d)
                if f >= edge:
                    big.setdefault(k, set()).add(f)
                    assert (d["grid"] * 128 > U * n * f) == (f <= 64), (k, f, d)          # 32 800 and 65 600 positions: a partly filled last tile
            else:
                assert d["tile"] == 32 and (d["nw"], d["all"]) == ((4, 1) if bf16 else (1, 0)), (k, f, d)
        if which == "natural":
            assert set(big) == set(CONV_KINDS), sorted(big)
            assert all(64 in fs for fs in big.values()) and (not bf16 or all(32 in fs for fs in big.values())), big
        plan = _plan(off)
        res[which] = (off.process(x), _all_states(off))
        off.close()
    (oa, sa), (ob, sb) = res["natural"], res["small tiles"]
    assert np.isfinite(oa).all() and float(np.abs(ob).max()) > 1e-3
    led = Ledger("plain, %d x %d frames, %s pipe, natural tile threshold against small tiles" % (U, n, pipe), plan)
    for u in range(U):
        led.add("outputs, utterance %d" % u, LAST_OP, WF.rms(oa[u], ob[u]) / DEVICE_RMS, device=True)
        for sn in WF.state_names():
            led.add("state %s, utterance %d" % (sn, u), WF.state_consumer(sn), WF.rms(sa[sn][u], sb[sn][u]) / DEVICE_RMS, device=True)
    assert len(led.ratio) == U * 131
    led.close()
