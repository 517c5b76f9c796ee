"""Synthetic weight families, inputs and float64 reference values for the LSTM-variant kernels (a plain helper module: the CPU tests
of tests/test_weight_families.py and tests/test_ctfa_families.py and the GPU tests of tests/test_gpu_synthetic_weights.py,
tests/test_gpu_conv_variants.py and tests/test_gpu_ctfa_families.py share it, and its caches) and, in its second
half (``variant="baseline"``), for the dilated-dense baseline's (tests/test_baseline_families.py, tests/test_gpu_baseline_families.py).

Every family starts from ``synthetic_weights("lstm", SEED, bias_std=0.1, affine_jitter=0.1)`` and is stored as the export stores the
trained network (``weights.quantize_like_export``); the oracle is fed ``parse_blob`` of the very container the engine is given, so
quantisation is not part of any difference measured here.  The reference is oracle B in double (``NutlsRef(dtype=torch.float64)``);
the float32 oracle's distance from it is what decides whether a family is fit to test with (the conditioning cap).

The baseline half: every family starts from ``synthetic_weights("baseline", SEED, bias_std=0.1, affine_jitter=0.1)``, is stored with
``write_blob(..., int8_convs=True)`` (the form the fused kernel takes) and runs BASE_FRAMES = 37 frames: block 6 of every dilated-dense
block taps the frame 32 steps back, so its history is live for the last 5 frames only, and at 37 every history ring of depth >= 2 sits at
a non-zero phase (37 & (d - 1) = 1, 1, 5, 5, 5 for d = 2, 4, 8, 16, 32).

The section "large offsets" near the end: the index maps, the eight-utterance call sequence and the references of the handles whose arena
offsets pass 2^31 and 2^32 (tests/test_large_offsets.py, tests/test_gpu_large_offsets.py)."""
import functools

import numpy as np
import torch

from nunet_amd import topology as T
from nunet_amd.weights import EXPORT_FORMS, parse_blob, quantize_like_export, synthetic_weights, write_blob
from oracle.nutls_ref import NutlsRef

SEED = 11
FRAMES = 6

# The project's bounds (tests/test_gpu_packed.py TIGHT_RMS, tests/test_gpu_trace.py, the state bound of
# test_packed_vs_oracle_and_slot_independence), applied against the float64 oracle.
OUT_BOUND = 2e-5          # RMS < OUT_BOUND x max(1, max|want|)
TRACE_BOUND = 2e-5        # relative RMS
STATE_BOUND = 1e-4        # RMS < STATE_BOUND x max(1, max|want|), per tensor
CAP = 1.0 / 20.0          # the float32 oracle may use at most this share of a bound

SAT_PATTERN = np.float32([-100.0, -30.0, -8.0, 0.0, 8.0, 30.0, 100.0])
CONST_LAYERS = ("msfe6_en_conv3", "msfe4_de_spconv1", "msfe5_en_in")
# a strided conv, two sub-pixel convs (the second the 128-channel last one of its stage), a down- and an up-sampling conv
DEAD_LAYERS = ("msfe6_en_conv2", "msfe5_de_spconv2", "msfe6_de_spconv6", "msfe4_down_sampling", "msfe4_upsampling2")
ALPHAS = np.float32([-0.5, 0.0, 1.0, 1.7])
# Seed of the `scales` exponents.  Nine octaves of channel scales in front of a LayerNorm leave few channels that carry weight, and the
# float32 oracle's own distance from the float64 one on the small decoder stages' traced tensors then lies between 0.6e-6 and 2.8e-6
# relative RMS, depending on the draw (seeds 20..43 scanned, oracle against oracle, no kernel involved); the cap allows 1e-6.  This
# draw gives 6.1e-7 on the traced tensors and 6.1e-7 x scale on the states.
SCALES_SEED = 41

# LayerNorm variance about equal to its epsilon (1e-8): the kernel times 3e-4, the bias zero so that nothing cancels.  With a variance of
# exactly 0 (`const`) the output is beta whatever a non-zero eps is, and on plain weights eps is 1e-8 next to a variance of order 1; here
# the output depends on eps to first order, at every site that sets it in its own place in the code.
TINYVAR_CONVS = ("input_layer", "msfe5_en_conv2", "msfe4_de_spconv1", "msfe6_de_in", "msfe6_de_spconv6")
TINYVAR_FACTOR = np.float32(3e-4)

# The CTFA gate perceptrons (`*_ta` / `*_fa` .w1 .b1 .w2 .b2, 24 of them): `gatesat` puts SAT_PATTERN on every b2 (gates of exactly 0 and
# 1), `gatedead` kills hidden layers, hidden units or output rows, `gatehist` makes the frequency branch answer strongly to its input, which
# in the causal 32-frame mode is the mean of the last 32 time-attention vectors.
# `gatehist` scales w1 of BOTH gates of every stage.  With the frequency gates alone the history hardly matters: every gate sits behind a
# LayerNorm, so on plain weights the time attention of stream 1 of `causal_streams` moves by 0.003 between silence and a tone of 50, and the
# frequency attention, 16 times as sensitive, by 0.043 between frame 32 and frame 64 (float64 oracle).  With the time gates scaled as well
# it moves by 0.23 (tests/test_ctfa_families.py asserts more than 0.1); fa.w1 x 64 alone gives 0.12, fa.w1 x 16 with ta.w1 x 4 gives 0.12.
GATEHIST_FACTOR = np.float32(16.0)
GATE_FAMILIES = ("gatesat", "gatedead", "gatehist")
BASE_FAMILIES = ("plain", "satbias", "const", "dead", "scales", "alpha", "tinyvar") + GATE_FAMILIES
FORM_FAMILIES = tuple("forms_" + f for f in EXPORT_FORMS if f != "shipped")
FAMILIES = BASE_FAMILIES + FORM_FAMILIES


# ---- the baseline half's constants -----------------------------------------------------------------------------------------------------
BASE_FRAMES = 37
BASELINE_FAMILIES = ("plain", "const", "tinyvar", "alpha", "dead", "scales")
# one block each of an F = 4, an F = 2 and an F = 1 stage (G = 16) and of the central block (F = 4, G = 32)
CONST_BLOCKS = ("msfe6_en_ddb_3", "msfe4_de2_ddb_2", "msfe4_en3_ddb_1", "ddb_6")
TINYVAR_BLOCKS = ("msfe6_en_ddb_2", "ddb_4", "msfe4_en3_ddb_6", "msfe4_de2_ddb_1", "msfe6_de_ddb_5")
DEAD_BLOCKS = ("ddb_3", "msfe4_en2_ddb_5", "msfe3_de_ddb_2")          # (F, G) = (4, 32), (2, 16), (1, 16)


def state_names(variant="lstm"):
    """The 130 (LSTM variant) or 208 (baseline) state tensors under the names ``state_get`` and ``NutlsRef.state`` use."""
    return [base if len(shp) == 1 else base.format("prev") for base, shp in T.state_specs(variant)]


def traced_names():
    """The 18 tensors the profiling build copies out and the oracle traces: 12 CTFA outputs, 6 up-sampling outputs."""
    return ["%s.y" % st.prefix for st in T.STAGES] + ["%s.up" % st.prefix for st in T.DECODER]


def traced_shape(name):
    prefix, kind = name.split(".")
    return (T.STAGE_BY_PREFIX[prefix].f0, 64 if kind == "y" else 128)


def _scale_rows(a, rng):
    """2^k, k in [-6, 2], per output channel (axis 0): exact, nine octaves of per-channel scales"""
    e = rng.integers(-6, 3, size=a.shape[0])
    return (a * np.exp2(e).reshape((-1,) + (1,) * (a.ndim - 1))).astype(np.float32)


def _baseline_tensors(family):
    w = synthetic_weights("baseline", SEED, bias_std=0.1, affine_jitter=0.1)
    if family == "plain":
        return w
    if family == "const":
        # z = b1 = 0.5 in every channel: the block's LayerNorm sees a variance of exactly 0 and the block's output is PReLU(beta)
        for blk in CONST_BLOCKS:
            w[blk + ".w1"] = np.zeros_like(w[blk + ".w1"])
            w[blk + ".b1"] = np.full_like(w[blk + ".b1"], 0.5)
        for layer in CONST_LAYERS:
            w[layer + ".w"] = np.zeros_like(w[layer + ".w"])
            w[layer + ".b"] = np.full_like(w[layer + ".b"], 0.5)
    elif family == "tinyvar":
        for blk in TINYVAR_BLOCKS:
            w[blk + ".w1"] = (w[blk + ".w1"] * TINYVAR_FACTOR).astype(np.float32)
            w[blk + ".b1"] = np.zeros_like(w[blk + ".b1"])
        for layer in TINYVAR_CONVS:
            w[layer + ".w"] = (w[layer + ".w"] * TINYVAR_FACTOR).astype(np.float32)
            w[layer + ".b"] = np.zeros_like(w[layer + ".b"])
    elif family == "alpha":
        # sorted order puts the eight slopes of one block (_1 .. _6, _in, _out) next to each other: they differ inside every block
        for n, k in enumerate(sorted(k for k in w if k.endswith(".alpha"))):
            w[k] = np.full_like(w[k], ALPHAS[n % 4])
    elif family == "dead":
        for blk in DEAD_BLOCKS:
            w[blk + ".w1"][::3] = 0.0          # the 1x1 conv's output channel is its bias alone
            w[blk + ".wg"][1::3] = 0.0         # the grouped conv's output channel is its bias alone
        for layer in DEAD_LAYERS:
            w[layer + ".w"][::3] = 0.0          # all-zero output channels: quantiser scale 1.0
    elif family == "scales":
        rng = np.random.default_rng(SCALES_SEED)
        for k in w:
            if k.endswith(".w") and w[k].ndim == 4 and w[k].size >= 1024:
                w[k] = _scale_rows(w[k], rng)
            elif k.endswith(".w1") and w[k].ndim == 2:          # the rows of every block's 1x1 kernel
                w[k] = _scale_rows(w[k], rng)
    else:
        raise ValueError("unknown baseline family %s" % family)
    return w


def family_tensors(family, variant="lstm"):
    """Float32 tensors of a family, before quantisation."""
    if variant == "baseline":
        return _baseline_tensors(family)
    w = synthetic_weights("lstm", SEED, bias_std=0.1, affine_jitter=0.1)
    if family == "plain" or family.startswith("forms_"):
        return w
    if family == "satbias":
        # every gate type (i, f, g, o: 21 consecutive entries each) gets every value three times; +-100 overflows __expf
        for n, k in enumerate(sorted(k for k in w if k.endswith("lstm.b"))):
            w[k] = (w[k] + SAT_PATTERN[(np.arange(84) * 5 + n) % 7]).astype(np.float32)
    elif family == "const":
        # every channel exactly 0.5 (sums of 0.5 are exact in fp32): variance exactly 0, LayerNorm's output is beta, eps alone keeps it finite
        for layer in CONST_LAYERS:
            w[layer + ".w"] = np.zeros_like(w[layer + ".w"])
            w[layer + ".b"] = np.full_like(w[layer + ".b"], 0.5)
    elif family == "dead":
        for layer in DEAD_LAYERS:
            w[layer + ".w"][::3] = 0.0          # all-zero output channels: quantiser scale 1.0
    elif family == "scales":
        rng = np.random.default_rng(SCALES_SEED)
        for k in w:
            if k.endswith(".w") and w[k].ndim == 4 and w[k].size >= 1024:
                e = rng.integers(-6, 3, size=w[k].shape[0])          # 2^k, k in [-6, 2]: exact, nine octaves of per-channel scales
                w[k] = (w[k] * np.exp2(e).reshape(-1, 1, 1, 1)).astype(np.float32)
    elif family == "alpha":
        for n, k in enumerate(sorted(k for k in w if k.endswith(".alpha"))):
            w[k] = np.full_like(w[k], ALPHAS[n % 4])
    elif family == "tinyvar":
        for layer in TINYVAR_CONVS:
            w[layer + ".w"] = (w[layer + ".w"] * TINYVAR_FACTOR).astype(np.float32)
            w[layer + ".b"] = np.zeros_like(w[layer + ".b"])
    elif family == "gatesat":
        # every gate of every stage has channels at +-100, +-30, +-8 and 0: __expf overflows to inf and the reciprocal gives exactly 0
        for n, g in enumerate(gate_prefixes()):
            w[g + ".b2"] = (w[g + ".b2"] + SAT_PATTERN[(np.arange(64) * 5 + n) % 7]).astype(np.float32)
    elif family == "gatedead":
        for n, g in enumerate(gate_prefixes()):
            if n % 3 == 0:
                w[g + ".b1"] = np.full_like(w[g + ".b1"], -10.0)          # hidden layer all zero after ReLU: the gate is sigmoid(b2)
            elif n % 3 == 1:
                w[g + ".w1"][::2] = 0.0          # every second hidden unit is relu(b1) whatever comes in
            else:
                w[g + ".w2"][::3] = 0.0          # every third gate channel is sigmoid(b2) whatever comes in
    elif family == "gatehist":
        for g in gate_prefixes():          # (both gates: see GATEHIST_FACTOR)
            w[g + ".w1"] = (w[g + ".w1"] * GATEHIST_FACTOR).astype(np.float32)
    else:
        raise ValueError("unknown family %s" % family)
    return w


def gate_prefixes():
    """The 24 gate perceptrons, sorted: ``<stage>_fa`` and ``<stage>_ta`` of the 12 stages."""
    return sorted("%s_%s" % (st.prefix, kind) for st in T.STAGES for kind in ("ta", "fa"))


def gate_traced_names():
    """The oracle's trace keys of the gates: ``<stage>.ta`` / ``.fa`` [B, 64] and their hidden layers ``.ta_hid`` / ``.fa_hid`` [B, 16]."""
    return ["%s.%s%s" % (st.prefix, kind, hid) for st in T.STAGES for kind in ("ta", "fa") for hid in ("", "_hid")]


@functools.lru_cache(maxsize=None)
def container(family, form=None, variant="lstm"):
    """The family's container.  ``form``: an export form of ``quantize_like_export`` ("shipped" unless the family is one of the
    ``forms_*``), or "float" (no quantisation at all: per-layer kernels only).  Baseline: ``write_blob(..., int8_convs=True)`` (form
    None) or "float"."""
    if variant == "baseline":
        if form not in (None, "float"):
            raise ValueError("the baseline containers are the int8-conv one (form None) and \"float\"")
        return write_blob(family_tensors(family, variant), int8_convs=form is None)
    if form is None:
        form = family[len("forms_"):] if family.startswith("forms_") else "shipped"
    w = family_tensors(family)
    return write_blob(w) if form == "float" else write_blob(quantize_like_export(w, form))


@functools.lru_cache(maxsize=None)
def base_streams():
    """[FRAMES, 4, 256] float32: noise, silence then a single bin at 50 from frame 2 on, other noise, 1e-20 everywhere."""
    rng = np.random.default_rng(SEED + 2)
    x = np.zeros((FRAMES, 4, 256), np.float32)
    x[:, 0] = 0.25 * np.abs(rng.standard_normal((FRAMES, 256)))
    x[2:, 1, 40] = 50.0
    x[:, 2] = 0.25 * np.abs(rng.standard_normal((FRAMES, 256)))
    x[:, 3] = 1e-20
    x.setflags(write=False)
    return x


BASE_TAIL = 8          # frames past BASE_FRAMES that the baseline streams' generators go on for (the state-transplant test)


@functools.lru_cache(maxsize=None)
def baseline_streams():
    """[BASE_FRAMES + BASE_TAIL, 4, 256] float32: the recipe of `base_streams` for the baseline half, with seeds of its own (one
    generator per noise stream, so that the first BASE_FRAMES frames do not depend on how far the generators are run)."""
    n = BASE_FRAMES + BASE_TAIL
    x = np.zeros((n, 4, 256), np.float32)
    x[:, 0] = 0.25 * np.abs(np.random.default_rng([SEED + 5, 0]).standard_normal((n, 256)))
    x[2:, 1, 40] = 50.0
    x[:, 2] = 0.25 * np.abs(np.random.default_rng([SEED + 5, 2]).standard_normal((n, 256)))
    x[:, 3] = 1e-20
    x.setflags(write=False)
    return x


def inputs(batch, variant="lstm", tail=False):
    """[FRAMES, batch, 256]: the base streams, repeated (stream b is base stream b % 4).  Baseline: [BASE_FRAMES, batch, 256], or with
    ``tail`` the BASE_TAIL frames that follow."""
    if variant == "baseline":
        x = baseline_streams()[BASE_FRAMES:] if tail else baseline_streams()[:BASE_FRAMES]
        return np.ascontiguousarray(x[:, np.arange(batch) % 4])
    return np.ascontiguousarray(base_streams()[:, np.arange(batch) % 4])


# ---- the causal 32-frame CTFA (tests/test_ctfa_families.py, tests/test_gpu_ctfa_families.py) ------------------------------------------------
# 70 frames: the streaming handle's history ring wraps at 32 and at 64 and the run ends at slot 6.  The onsets at 33 and 40 enter the
# 32-frame window just after a wrap and fill it before the end.
CAUSAL_FRAMES = 70
CAUSAL_FAMILIES = ("plain", "gatesat", "gatedead", "gatehist")
# the frames whose 18 traced tensors the causal references keep: the start, around the first frame with a full window (31), both wraps, the end
CAUSAL_TRACE_FRAMES = (0, 1, 30, 31, 32, 33, 63, 64, 65, 69)
# The offline block sets: (utterances = base streams, blocks, ragged calls [(block length, counts)]).  (17, 1, 31, 2, 19): the history is
# rolled from a partly filled one, by one frame, by exactly 31; (33, 32, 5): blocks longer than the history; the ragged calls hold
# utterance 1 (count 0) and then advance both by different counts.
CAUSAL_BLOCKS = {2: ((0, 1), (17, 1, 31, 2, 19)), 1: ((3,), (33, 32, 5))}
CAUSAL_RAGGED = ((17, (17, 0)), (20, (9, 20)))
CAUSAL_RESTART = 40          # test c: `reset(1)` after this many frames
CAUSAL_SWITCH = (10, 45)     # test c: frames in frame mode, then frames in causal32


def causal_keep_frames():
    """The frames after which the causal references keep all states: the end of every block of CAUSAL_BLOCKS, each utterance's own last
    frame after each ragged call, and the last frame."""
    keep = {CAUSAL_FRAMES - 1}
    for _, blocks in CAUSAL_BLOCKS.values():
        keep |= {sum(blocks[:i + 1]) - 1 for i in range(len(blocks))}
    done = [0, 0]
    for _, counts in CAUSAL_RAGGED:
        done = [d + c for d, c in zip(done, counts)]
        keep |= {d - 1 for d in done if d}
    return frozenset(keep)


@functools.lru_cache(maxsize=None)
def causal_streams():
    """[CAUSAL_FRAMES, 4, 256] float32: noise under a gain that swings between 0.02 and 1 from frame to frame; silence, then bin 40 at 50
    from frame 33 on; steady noise; noise for 40 frames, then 1e-20 everywhere.  One generator per noise stream."""
    n = CAUSAL_FRAMES
    x = np.zeros((n, 4, 256), np.float32)
    gain = np.float32(0.51 + 0.49 * np.cos(1.3 * np.arange(n)))
    x[:, 0] = 0.25 * np.abs(np.random.default_rng([SEED + 7, 0]).standard_normal((n, 256))) * gain[:, None]
    x[33:, 1, 40] = 50.0
    x[:, 2] = 0.25 * np.abs(np.random.default_rng([SEED + 7, 2]).standard_normal((n, 256)))
    x[:40, 3] = 0.25 * np.abs(np.random.default_rng([SEED + 7, 3]).standard_normal((40, 256)))
    x[40:, 3] = 1e-20
    x.setflags(write=False)
    return x


BLOCK_FRAMES = 27
BLOCK_FAMILIES = ("plain", "satbias", "const", "dead", "tinyvar")          # the families the block mode runs (2 utterances, BLOCK_FRAMES frames)


@functools.lru_cache(maxsize=None)
def block_inputs():
    """[2, BLOCK_FRAMES, 256] for the block mode: utterance 0 noise; utterance 1 silence, a single bin at 50 from frame 2 on, and
    1e-20 everywhere from frame 20 on."""
    rng = np.random.default_rng(SEED + 3)
    x = np.zeros((2, BLOCK_FRAMES, 256), np.float32)
    x[0] = 0.25 * np.abs(rng.standard_normal((BLOCK_FRAMES, 256)))
    x[1, 2:20, 40] = 50.0
    x[1, 20:] = 1e-20
    x.setflags(write=False)
    return x


# ---- the block sets of tests/test_gpu_conv_variants.py -------------------------------------------------------------------------------------
# Per number of utterances U: the blocks the frames are cut into, and which of them are also run RAGGED (block index -> one count per
# utterance, the longest equal to the block's length so that the launches are the uniform block's): the carried state of utterance u is then
# taken from frame counts[u] of the block, which is how a test reads states in the middle of a block.
# U = 3: every dense position count U * n is odd (27, 3, 21), so at F_out = 64 the last 128-position tile of every launch is half filled.  Of
# block 0 (27 dense streams) the counts (4, 6, 9) sample dense streams 3, 14 and 26: at every F_out <= 64 stream 26 lies in the partly filled
# last tile of a 128-position launch, and at every F_out >= 8 stream 3 lies in a full one (F_out <= 4: 27 F_out < 128, the launch is one
# partly filled tile; F_out >= 128: every tile is full).
BLOCK3_FRAMES = 17
BLOCK3_FAMILIES = ("plain", "tinyvar", "dead")
BLOCK_SETS = {2: {"blocks": (17, 1, 9), "ragged": {0: (6, 17), 2: (9, 4)}},
              3: {"blocks": (9, 1, 7), "ragged": {0: (4, 6, 9), 2: (3, 5, 7)}}}


def block_set_inputs(utterances):
    return block_inputs() if utterances == 2 else block3_inputs() if utterances == 3 else block8_inputs()


def block_set_families(utterances):
    return BLOCK_FAMILIES if utterances == 2 else BLOCK3_FAMILIES


def block_starts(utterances):
    blocks = BLOCK_SETS[utterances]["blocks"]
    return [sum(blocks[:i]) for i in range(len(blocks))]


def block_keep_frames(utterances):
    """The frames after which the block references keep all states: the last frame of every block and the ragged sample frames."""
    cfg, starts = BLOCK_SETS[utterances], block_starts(utterances)
    keep = {a + n - 1 for a, n in zip(starts, cfg["blocks"])}
    for i, counts in cfg["ragged"].items():
        keep |= {starts[i] + c - 1 for c in counts}
    return frozenset(keep)


@functools.lru_cache(maxsize=None)
def block3_inputs():
    """[3, BLOCK3_FRAMES, 256]: utterances 0 and 1 are the first 17 frames of `block_inputs`; utterance 2 is noise of its own draw under a
    gain that swings between 0.02 and 1 from frame to frame."""
    x = np.zeros((3, BLOCK3_FRAMES, 256), np.float32)
    x[:2] = block_inputs()[:, :BLOCK3_FRAMES]
    rng = np.random.default_rng(SEED + 6)
    gain = np.float32(0.51 + 0.49 * np.cos(1.3 * np.arange(BLOCK3_FRAMES)))
    x[2] = 0.25 * np.abs(rng.standard_normal((BLOCK3_FRAMES, 256))) * gain[:, None]
    x.setflags(write=False)
    return x


class Run:
    """What an oracle run leaves: ``out [frames, B, 256]``, ``trace[name] [frames, B, F, C]``, ``state[name] [B, ...]`` after the last
    frame, ``states_at[f][name] [B, ...]`` after frame f (0-based) for the frames that were asked for -- all float64 numpy, read-only."""

    def __init__(self, out, trace, state, states_at=None):
        self.out, self.trace, self.state, self.states_at = out, trace, state, states_at or {}
        traced = [a for v in trace.values() for a in (v.values() if isinstance(v, dict) else [v])]
        for a in [out] + traced + list(state.values()) + [a for d in self.states_at.values() for a in d.values()]:
            a.setflags(write=False)


def _oracle(blob, x, dtype, trace, variant="lstm", state=None, keep=(), ctfa_mode="frame", switch=None, trace_frames=None, gates=False,
            oracle=NutlsRef):
    """x [frames, B, 256] through oracle B in ``dtype``; ``state``: the state tensors to start from (zeros otherwise); ``keep``: frame
    indices after which all states are kept (``Run.states_at``).  ``ctfa_mode``: the oracle's; ``switch = (frame, mode)``: the mode is
    changed in front of that frame, as ``nutls_set_ctfa_mode`` does it (the states carry over, the attention history starts empty).
    ``trace_frames``: the frames whose 18 traced tensors are kept (``Run.trace[name]`` is then a dict frame -> tensor; None: every frame,
    stacked); ``gates``: the gates and their hidden layers (`gate_traced_names`) of every frame too.  ``oracle``: the class (a mutant's)."""
    ref = oracle(parse_blob(blob), batch=x.shape[1], dtype=dtype, variant=variant, ctfa_mode=ctfa_mode)
    if state is not None:
        for n in state_names(variant):
            assert ref.state[n].shape == state[n].shape, n
            ref.state[n] = torch.from_numpy(np.array(state[n])).to(dtype)
    outs, tr = [], {n: {} for n in traced_names()} if trace else {}
    gt = {n: [] for n in gate_traced_names()} if gates else {}
    states_at = {}
    for f in range(x.shape[0]):
        if switch is not None and f == switch[0]:
            ref.ctfa_mode, ref.ta_hist = switch[1], {}
        ref.trace = {} if trace or gates else None
        outs.append(ref.step(x[f]).numpy().astype(np.float64))
        if trace_frames is None or f in trace_frames:
            for n in tr:
                tr[n][f] = ref.trace[n].numpy().astype(np.float64)
        for n in gt:
            gt[n].append(ref.trace[n].numpy().astype(np.float64))
        if f in keep:
            states_at[f] = {n: ref.state[n].numpy().astype(np.float64) for n in state_names(variant)}
    state = {n: ref.state[n].numpy().astype(np.float64) for n in state_names(variant)}
    if trace_frames is None:
        tr = {n: np.stack([v[f] for f in range(x.shape[0])]) for n, v in tr.items()}
    tr.update({n: np.stack(v) for n, v in gt.items()})
    return Run(np.stack(outs), tr, state, states_at)


@functools.lru_cache(maxsize=None)
def reference(family, dtype=torch.float64, form=None, variant="lstm", ctfa_mode="frame", frames="base"):
    """The four base streams through the oracle on the family's container (computed once per process, never modified).
    ``ctfa_mode="causal32"`` or ``frames="causal"``: the CAUSAL_FRAMES frames of `causal_streams` instead, the 18 traced tensors of
    CAUSAL_TRACE_FRAMES, the gates of every frame, and all states after the frames of `causal_keep_frames`."""
    if ctfa_mode == "causal32" or frames == "causal":
        if variant != "lstm":
            raise ValueError("the causal inputs are the LSTM variant's")
        return _oracle(container(family, form), causal_streams(), dtype, trace=True, keep=causal_keep_frames(), ctfa_mode=ctfa_mode,
                       trace_frames=frozenset(CAUSAL_TRACE_FRAMES), gates=True)
    return _oracle(container(family, form, variant), inputs(4, variant), dtype, trace=True, variant=variant)


@functools.lru_cache(maxsize=None)
def causal_restart_reference(family):
    """Base stream 1 of `causal_streams` from frame CAUSAL_RESTART on through a float64 oracle that starts from nothing, causal32."""
    return _oracle(container(family), np.ascontiguousarray(causal_streams()[CAUSAL_RESTART:, 1:2]), torch.float64, trace=False, ctfa_mode="causal32")


@functools.lru_cache(maxsize=None)
def causal_switch_reference(family):
    """Base streams 0 and 1: CAUSAL_SWITCH[0] frames in frame mode, then CAUSAL_SWITCH[1] frames in causal32 (float64)."""
    n0, n1 = CAUSAL_SWITCH
    return _oracle(container(family), np.ascontiguousarray(causal_streams()[:n0 + n1, :2]), torch.float64, trace=False, ctfa_mode="frame",
                   switch=(n0, "causal32"))


@functools.lru_cache(maxsize=None)
def baseline_continuation(family):
    """The float64 baseline reference carried on from its states after frame BASE_FRAMES through the BASE_TAIL frames that follow
    (the state tensors are all of the oracle's state, so this is the run of BASE_FRAMES + BASE_TAIL frames)."""
    start = reference(family, variant="baseline")
    return _oracle(container(family, variant="baseline"), inputs(4, "baseline", tail=True), torch.float64, trace=False, variant="baseline",
                   state=start.state)


@functools.lru_cache(maxsize=None)
def block_reference(family, dtype=torch.float64, utterances=2, ctfa_mode="frame"):
    """The block-mode inputs (two utterances, or the three of `block3_inputs`), frame by frame through the oracle (utterances as the
    batch); all states are kept after the frames of `block_keep_frames`.  ``utterances=8``: the call sequence of the large-offset set
    (`Block8Reference`; ``ctfa_mode`` is for that set alone)."""
    if utterances == 8:
        return Block8Reference(family, dtype, ctfa_mode)
    if ctfa_mode != "frame":
        raise ValueError("the two- and three-utterance sets run the frame-wise CTFA")
    x = block_set_inputs(utterances)
    return _oracle(container(family), np.ascontiguousarray(x.transpose(1, 0, 2)), dtype, trace=False, keep=block_keep_frames(utterances))


# ---- large offsets (tests/test_large_offsets.py, tests/test_gpu_large_offsets.py) -----------------------------------------------------------
# Every kernel addresses a stream's (a frame's) slice as arena + row * sstride.  NUTLS_STRIDE_ALIGN (floats; read by `arena_commit` when a
# handle is created) rounds the slice stride up to a multiple of its value: with 2^24 floats every slice is 2^26 bytes, whatever the layout
# (the largest slice, an offline row, is about 2.6 MB), and row r starts r x 2^26 bytes into the arena.
STRIDE_ALIGN = 1 << 24          # floats
ROW_BYTES = 4 * STRIDE_ALIGN
# what an offset can outgrow -> the first row that starts at or beyond it
THRESHOLD_ROWS = {"2^31 bytes": (1 << 31) // ROW_BYTES, "2^32 bytes": (1 << 32) // ROW_BYTES,
                  "2^31 floats": (4 << 31) // ROW_BYTES, "2^32 floats": (4 << 32) // ROW_BYTES}
# the streaming handles: (variant, streams per workgroup as requested from `NutlsEngine` (None: the library's choice), B, the plan that runs)
LARGE_HANDLES = (("lstm", 1, 264, 1), ("lstm", 2, 300, 2), ("lstm", 4, 264, 4), ("baseline", None, 264, 1))
LARGE_FOURTH = (5, 70, 200)          # rows that carry base stream 3, beside row B - 1
# the tensors whose row B - 1 is edited through `state_set`, and read whole ([B, ...]) through `state_get`: a conv-input state and a small one
LARGE_EDITED = {"lstm": ("msfe6_ee_prev1", "state_h"), "baseline": ("msfe6_ee_prev1", "ddb_prev3")}


def large_index_map(B):
    """idx[r]: the base stream that row r of a B-row handle carries.  (r // 32) % 3: the rows 32, 64, 128 and 256 below r (1, 2, 4, 8 groups of
    32: 1, 2, 1, 2 modulo 3) carry another stream, so a row whose offset lost its bits above 2^31 or 2^32, of bytes or of floats, lands on
    different data -- never on a replica that hides the mistake.  Base stream 3 rides on the rows of LARGE_FOURTH and on row B - 1."""
    idx = (np.arange(B) // 32) % 3
    idx[list(LARGE_FOURTH) + [B - 1]] = 3
    return idx


def large_map_ok(idx):
    """The condition on an index map: idx[r] != idx[r - T] for every threshold distance T and every r >= T."""
    return all(not np.any(idx[T:] == idx[:-T]) for T in THRESHOLD_ROWS.values() if T < len(idx))


def large_sample_rows(B):
    """The rows whose whole state is read: both sides of every threshold, the first and the last."""
    return sorted({0, B - 1} | {T - 1 for T in THRESHOLD_ROWS.values()} | set(THRESHOLD_ROWS.values()))


def large_held_rows(B):
    """The rows the masked step holds."""
    return (255, 256, B - 1)


class LargeContinuation:
    """What follows the base run on a large streaming handle, through the float64 oracle on five rows: base streams 0 .. 3 as they go on,
    and row 4 = the handle's row B - 1 (base stream 3).
      step 1: row 4 starts from the states of stream 3 with the tensors of LARGE_EDITED replaced by ``edits`` (float32 values; the handle is
              given the same through `state_set`); every row takes frame ``extra[0]`` of its stream.
      step 2: row 4 starts from nothing (`reset(B - 1)`) and takes frame 0 of stream 3; the others take ``extra[1]``.
      step 3: the others take ``extra[2]`` (the handle holds three rows here, row B - 1 among them).
    ``steps[i]``: a `Run` of one frame, ``out [1, 5, 256]`` and ``state``."""

    def __init__(self, variant):
        start = reference("plain", variant=variant)
        names = state_names(variant)
        x = baseline_streams() if variant == "baseline" else base_streams()
        self.extra = (BASE_FRAMES, BASE_FRAMES + 1, BASE_FRAMES + 2) if variant == "baseline" else (1, 2, 3)
        a, b = LARGE_EDITED[variant]
        self.edits = {a: np.float32(start.state[a][0]), b: np.float32(0.5 * start.state[b][3] + 0.25)}
        state = {n: np.concatenate([start.state[n], start.state[n][3:4]]) for n in names}
        for n, v in self.edits.items():
            state[n][4] = v
        blob, self.steps = container("plain", variant=variant), []
        for i, f in enumerate(self.extra):
            frame = np.concatenate([x[f], x[0 if i == 1 else f][3:4]])[None]
            if i == 1:
                for n in names:
                    state[n][4] = 0.0
            run = _oracle(blob, frame, torch.float64, trace=False, variant=variant, state=state)
            self.steps.append(run)
            state = {n: np.array(run.state[n]) for n in names}


@functools.lru_cache(maxsize=None)
def large_continuation(variant="lstm"):
    return LargeContinuation(variant)


# The offline set: eight utterances in a handle of max_frames = 32 (8 x 33 = 264 arena rows; utterance u's carried slot is row 33 u, its
# frame t row 33 u + 1 + t: utterance 7's frames 25 .. 32 start beyond 2^32 floats).  Per call one count per utterance: a uniform block of
# 32, a ragged block of width 32 (an utterance held, one frame, a full row next to short ones), a uniform block of 7; then utterance
# BLOCK8_RESET starts anew and a uniform block of BLOCK8_TAIL follows.  Every utterance takes its own stream's frames in order.
BLOCK8_MAX = 32
BLOCK8_CALLS = ((32,) * 8, (32, 0, 1, 17, 32, 5, 31, 32), (7,) * 8)
BLOCK8_RESET = 7
BLOCK8_TAIL = 5
BLOCK8_FRAMES = 32 + 32 + 7 + BLOCK8_TAIL
BLOCK8_MODES = ("frame", "causal32")


def block8_calls():
    """All four calls: the three of BLOCK8_CALLS and the block behind the reset."""
    return BLOCK8_CALLS + ((BLOCK8_TAIL,) * 8,)


def block8_starts():
    """starts[k][u]: the frames of its stream that utterance u has taken before call k (k = 0 .. 4; 4: at the end)."""
    starts = [[0] * 8]
    for counts in block8_calls():
        starts.append([a + c for a, c in zip(starts[-1], counts)])
    return starts


@functools.lru_cache(maxsize=None)
def block8_inputs():
    """[8, BLOCK8_FRAMES, 256]: the recipes of `block_inputs` and `block3_inputs` (noise; silence, a single bin at 50, then 1e-20; noise under
    a swinging gain) and five more streams of noise, each of its own draw and level, one of them falling to 1e-20 after 20 frames."""
    n = BLOCK8_FRAMES
    noise = lambda u: np.abs(np.random.default_rng([SEED + 9, u]).standard_normal((n, 256)))
    x = np.zeros((8, n, 256), np.float32)
    x[0] = 0.25 * noise(0)
    x[1, 2:40, 40] = 50.0
    x[1, 40:] = 1e-20
    x[2] = 0.25 * noise(2) * np.float32(0.51 + 0.49 * np.cos(1.3 * np.arange(n)))[:, None]
    x[3] = 0.05 * noise(3)
    x[4] = 1.0 * noise(4)
    x[5] = 0.25 * noise(5)
    x[5, 20:] = 1e-20
    x[6] = 0.5 * noise(6)
    x[7] = 0.25 * noise(7)
    x.setflags(write=False)
    return x


class Block8Reference:
    """The call sequence of the offline set through the oracle, utterances as the batch, frame by frame: ``out(k, u) [count, 256]``, the
    output rows of utterance u in call k, and ``state(k, u)[name]``, its states after that call (after its last frame so far: a held
    utterance keeps what it had).  Utterance BLOCK8_RESET's last call comes from a second oracle that starts from nothing."""

    def __init__(self, family, dtype, ctfa_mode):
        x, blob = block8_inputs(), container(family)
        self.starts, self.calls = block8_starts(), block8_calls()
        names = state_names()
        ends = {}          # frame -> [(call, utterance)]: whose state to keep behind that frame
        for k, counts in enumerate(self.calls):
            for u in range(8):
                if not (k == 3 and u == BLOCK8_RESET):
                    ends.setdefault(self.starts[k + 1][u] - 1, []).append((k, u))
        self._out, self._state = {}, {}

        def run(frames, rows, ends):
            ref = NutlsRef(parse_blob(blob), batch=len(rows), dtype=dtype, variant="lstm", ctfa_mode=ctfa_mode)
            outs = []
            for f in range(frames.shape[0]):
                outs.append(ref.step(frames[f]).numpy().astype(np.float64))
                for k, u in ends.get(f, ()):
                    self._state[k, u] = {n: ref.state[n][rows.index(u)].numpy().astype(np.float64) for n in names}
            return np.stack(outs)

        main = run(np.ascontiguousarray(x.transpose(1, 0, 2)), list(range(8)), ends)
        a = self.starts[3][BLOCK8_RESET]
        fresh = run(np.ascontiguousarray(x[BLOCK8_RESET:BLOCK8_RESET + 1, a:a + BLOCK8_TAIL].transpose(1, 0, 2)), [BLOCK8_RESET],
                    {BLOCK8_TAIL - 1: [(3, BLOCK8_RESET)]})
        for k, counts in enumerate(self.calls):
            for u, c in enumerate(counts):
                a = self.starts[k][u]
                self._out[k, u] = fresh[:, 0] if (k == 3 and u == BLOCK8_RESET) else main[a:a + c, u]
        for a in list(self._out.values()) + [v for d in self._state.values() for v in d.values()]:
            a.setflags(write=False)

    def out(self, call, utterance):
        return self._out[call, utterance]

    def state(self, call, utterance):
        return self._state[call, utterance]


# ---- measures ----------------------------------------------------------------------------------------------------------------------
def rms(a, b):
    return float(np.sqrt(np.mean((np.asarray(a, np.float64) - np.asarray(b, np.float64)) ** 2)))


def scaled_rms(got, want):
    """RMS of the difference over max(1, max|want|): what OUT_BOUND and STATE_BOUND bound."""
    return rms(got, want) / max(1.0, float(np.abs(want).max()))


def rel_rms(got, want):
    """RMS of the difference over the RMS of ``want``: what TRACE_BOUND bounds."""
    want = np.asarray(want, np.float64)
    return rms(got, want) / max(1e-12, float(np.sqrt(np.mean(want ** 2))))


def ddb_state(name):
    """``X_ddb_prev_in`` / ``X_ddb_prevK`` / ``X_ddb_prev_out`` (central: ``ddb_...``) -> (the plan's op name ``X_ddb`` / ``ddb``, "in" /
    K / "out"); None for any other state."""
    for prefix, _, _ in T.bottlenecks():
        tag = (prefix + "_ddb") if prefix else "ddb"
        if name.startswith(tag + "_prev"):
            part = name[len(tag) + 5:]
            if part in ("_in", "_out"):
                return tag, part[1:]
            if part.isdigit() and 1 <= int(part) <= T.DDB_BLOCKS:
                return tag, int(part)
    return None


def state_label(name, stream):
    """What a ledger calls a state tensor of a stream; a block's history ring says which block's output its newest frame starts with."""
    d = ddb_state(name)
    if d is not None and isinstance(d[1], int):
        return "state %s (block %d output, newest frame), stream %d" % (name, d[1] - 1, stream)
    return "state %s, stream %d" % (name, stream)


def state_consumer(name):
    """The layer of the fused plan that a state tensor belongs to: the conv whose previous-frame input it is, the stage's LSTM, or
    (baseline) the dilated-dense block op."""
    if name in ("state_h", "state_c"):
        return "lstm"
    if ddb_state(name) is not None:
        return ddb_state(name)[0]
    for st in T.STAGES:
        if name in (st.prefix + "_h", st.prefix + "_c"):
            return st.prefix + "_lstm"
        for tag, kind in ((st.conv_tag, "conv"), (st.spconv_tag, "spconv")):
            if name.startswith(tag + "_prev") and name[len(tag) + 5:].isdigit():
                return "%s_%s%s" % (st.prefix, kind, name[len(tag) + 5:])
    raise ValueError(name)


def traced_op(name):
    """The op of the fused plan that writes a traced tensor."""
    prefix, kind = name.split(".")
    return prefix + "_ctfa" if kind == "y" else T.STAGE_BY_PREFIX[prefix].resample


def first_in_plan_order(plan, offenders):
    """``plan``: ``eng.fused_plan()``; ``offenders``: {tensor label: op name}.  The label whose op comes first in the plan (an op the
    plan does not name sorts last), so that a failure points at the earliest op that went wrong."""
    pos = {}
    for i, op in enumerate(plan):
        pos.setdefault(op["layer"].split("#")[0], i)
    return min(offenders, key=lambda k: (pos.get(offenders[k], len(plan)), k))
