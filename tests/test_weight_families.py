"""CPU tests behind tests/test_gpu_synthetic_weights.py and tests/test_gpu_conv_variants.py (no GPU): the export-form quantiser is pinned to the shipped container as data,
the float64 oracle is the same function as the float32 one, and every synthetic weight family is well conditioned in the reference
itself -- the float32 oracle stays within 1/20 of every bound the GPU tests apply against the float64 oracle."""
import os

import numpy as np
import pytest
import torch

import weight_families as WF
from conftest import GOLDEN
from nunet_amd import topology as T
from nunet_amd.weights import DEFAULT_WEIGHTS, EXPORT_FORMS, parse_blob, quantize_like_export, read_blob, write_blob
from oracle.nutls_ref import NutlsRef


def _rows(q, scales):
    """int8 payload as [scales, elements per scale]"""
    return q.reshape(scales.size, -1)


def test_quantiser_reproduces_the_shipped_container():
    """`quantize_like_export` of the de-quantised shipped tensors gives the shipped container back: dtype code, scale count and scales of
    every tensor; the int8 payload exactly wherever the shipped channel (or tensor) attains |q| = 127 -- there `max|w| / 127` is the
    shipped scale -- and within one step elsewhere.  The shipped file has 9635 quantised channels / single-scale tensors
    (128 conv kernels, 48 gate matrices, 26 LSTM kernels, 9 Dense kernels) and EVERY one of them attains 127: 0 fall under "elsewhere"."""
    blob = read_blob(DEFAULT_WEIGHTS)
    shipped = parse_blob(blob, dequantize=False)
    got = quantize_like_export(parse_blob(blob), "shipped")
    assert list(got) == list(shipped)
    forms = {}
    groups = attained = 0
    for name, want in shipped.items():
        g = got[name]
        assert isinstance(g, tuple) == isinstance(want, tuple), name
        if not isinstance(want, tuple):
            assert np.asarray(g).dtype == np.float32 and np.array_equal(g, want), name
            continue
        (q, sc), (gq, gsc) = want, g
        assert gq.dtype == np.int8 and gq.shape == q.shape and gsc.dtype == np.float32 and gsc.shape == sc.shape, name
        suffix = name.rsplit(".", 1)[1]
        forms[(suffix, q.ndim, "per channel" if sc.size > 1 else "one scale")] = forms.get((suffix, q.ndim, "per channel" if sc.size > 1 else "one scale"), 0) + 1
        if sc.size > 1:
            assert sc.size == q.shape[0], name
        hit = np.abs(_rows(q, sc)).max(axis=1) == 127
        groups += hit.size
        attained += int(hit.sum())
        assert np.array_equal(gsc[hit], sc[hit]), name
        assert np.array_equal(_rows(gq, sc)[hit], _rows(q, sc)[hit]), name
        if not hit.all():
            assert np.abs(_rows(gq, sc)[~hit].astype(np.int32) - _rows(q, sc)[~hit]).max() <= 1, name
    assert forms == {("w", 4, "per channel"): 128, ("w1", 4, "per channel"): 24, ("w2", 4, "per channel"): 24,
                     ("wx", 2, "one scale"): 13, ("wh", 2, "one scale"): 13, ("w", 2, "one scale"): 9}
    floats = [n for n, v in shipped.items() if not isinstance(v, tuple) and n.endswith(".w")]
    assert sorted(np.asarray(shipped[n]).shape for n in floats) == sorted([(32, 21)] * 4 + [(64, 1, 1, 1), (1, 1, 1, 64)])
    print("quantised channels / single-scale tensors: %d, attaining |q| = 127: %d, within one step only: %d" % (groups, attained, groups - attained))
    assert (groups, attained) == (9635, 9635)
    # the container written from it is the shipped one, byte for byte, and parses back to the same values
    again = write_blob(got)
    assert again == blob
    back = parse_blob(again)
    for name, v in parse_blob(blob).items():
        assert np.array_equal(back[name], v), name


def test_quantiser_forms_on_synthetic_weights():
    """The rule itself (scale = max|w| / 127, 1.0 for an all-zero channel; q = clip(rint(w / scale), -127, 127)) and the three alternative
    forms, on the `dead` family's tensors; `write_blob` passes the tuples through."""
    w = WF.family_tensors("dead")
    for form in EXPORT_FORMS:
        q = quantize_like_export(w, form)
        back = parse_blob(write_blob(q))
        raw = parse_blob(write_blob(q), dequantize=False)
        for name, a in w.items():
            v = raw[name]
            small_dense = name.endswith(".w") and a.ndim == 2 and a.shape[0] < 64
            gate = name.endswith((".w1", ".w2"))
            conv = name.endswith(".w") and a.ndim == 4 and a.size >= 1024
            quantised = conv or name.endswith((".wx", ".wh")) or (gate and form != "float_gates") or \
                (name.endswith(".w") and a.ndim == 2 and (not small_dense or form == "int8_small_dense"))
            assert isinstance(v, tuple) == quantised, (form, name)
            if not quantised:
                assert np.array_equal(v, a), (form, name)
                continue
            qq, sc = v
            per_channel = (conv and form != "single_scale_convs") or gate
            assert sc.size == (a.shape[0] if per_channel else 1), (form, name)
            amax = np.abs(a).reshape(sc.size, -1).max(axis=1)
            assert np.array_equal(sc, np.where(amax > 0, amax / 127.0, 1.0).astype(np.float32)), (form, name)
            assert np.array_equal(qq.reshape(sc.size, -1), np.clip(np.rint(a.reshape(sc.size, -1) / sc[:, None]), -127, 127)), (form, name)
            assert np.abs(back[name] - a).reshape(sc.size, -1).max(axis=1).max() <= 0.5 * sc.max() * (1 + 1e-6), (form, name)
    dead = quantize_like_export(w, "shipped")["msfe6_de_spconv6.w"]
    assert (dead[1][::3] == 1.0).all() and not dead[0][::3].any() and (dead[1][1::3] != 1.0).all()
    with pytest.raises(ValueError):
        quantize_like_export(w, "per_row_gates")


def test_float64_oracle_is_the_same_function():
    """Shipped weights, first frames of the golden clip: the float64 run agrees with the float32 run, the golden outputs and the golden
    states within the bounds tests/test_oracle.py uses for the float32 oracle (1e-6 RMS on outputs, rtol = atol = 2e-5 on states), and
    it really is double throughout."""
    clip = np.load(os.path.join(GOLDEN, "clip_4s.npz"))
    r32, r64 = NutlsRef(batch=1), NutlsRef(batch=1, dtype=torch.float64)
    assert all(v.dtype == torch.float64 for v in r64.w.values()) and all(v.dtype == torch.float64 for v in r64.state.values())
    assert all(v.dtype == torch.float32 for v in r32.w.values())
    o32, o64 = [], []
    for i in range(3):
        r64.trace = {}
        o32.append(r32.step(clip["mags_in"][i:i + 1]).numpy().reshape(-1))
        out = r64.step(clip["mags_in"][i:i + 1])
        assert out.dtype == torch.float64 and all(v.dtype == torch.float64 for v in r64.trace.values())
        o64.append(out.numpy().reshape(-1))
    assert all(v.dtype == torch.float64 for v in r64.state.values())
    assert WF.rms(np.stack(o64), np.stack(o32)) < 1e-6
    assert WF.rms(np.stack(o64), clip["mags_out"][:3]) < 1e-6
    st = np.load(os.path.join(GOLDEN, "state_f3.npz"))
    for base, shp in T.state_specs():
        k_ref = base if len(shp) == 1 else base.format("prev")
        k_gold = base if len(shp) == 1 else base.format("cur")
        np.testing.assert_allclose(r64.state[k_ref].numpy().reshape(-1), st[k_gold].reshape(-1), rtol=2e-5, atol=2e-5, err_msg=k_gold)
        np.testing.assert_allclose(r64.state[k_ref].numpy().reshape(-1), r32.state[k_ref].numpy().reshape(-1), rtol=2e-5, atol=2e-5, err_msg=k_ref)


# Tensors left out of the GPU comparison because the REFERENCE is ill conditioned on them: family -> names (at most 2 states each).
EXCLUDED = {}


@pytest.mark.parametrize("family", WF.FAMILIES)
def test_conditioning_cap(family):
    """A condition on the families, not a measurement of any kernel: on every family, for the output of every frame, each of the 18
    traced tensors of every frame and each of the 130 final states of every stream, the float32 oracle lies within 1/20 of the bound
    the GPU tests apply to that quantity against the float64 oracle; the same for both block-mode input sets of the families that run
    there: every output frame of every utterance and all 130 states of every utterance at every frame the block references keep them for.
    A family that fails here is changed or dropped -- no bound is widened."""
    assert not EXCLUDED.get(family), "nothing is excluded today"
    r64, r32 = WF.reference(family), WF.reference(family, torch.float32)
    assert np.isfinite(r64.out).all() and np.isfinite(r32.out).all()
    out = max(WF.scaled_rms(r32.out[f], r64.out[f]) for f in range(WF.FRAMES))
    tr = max((WF.rel_rms(r32.trace[n][f], r64.trace[n][f]), n, f) for n in WF.traced_names() for f in range(WF.FRAMES))
    st = max((WF.scaled_rms(r32.state[n][b], r64.state[n][b]), n, b) for n in WF.state_names() for b in range(4))
    print("%s: float32 oracle vs float64 oracle: outputs %.2e x scale (cap %.1e), traced %.2e rel (%s, frame %d; cap %.1e), "
          "states %.2e x scale (%s, stream %d; cap %.1e), exclusions: none"
          % (family, out, WF.CAP * WF.OUT_BOUND, tr[0], tr[1], tr[2], WF.CAP * WF.TRACE_BOUND, st[0], st[1], st[2], WF.CAP * WF.STATE_BOUND))
    assert len(WF.traced_names()) == 18 and len(WF.state_names()) == 130
    assert out <= WF.CAP * WF.OUT_BOUND
    assert tr[0] <= WF.CAP * WF.TRACE_BOUND, tr
    assert st[0] <= WF.CAP * WF.STATE_BOUND, st
    if family == "plain":          # its float container too (the per-layer kernels run it; no traced tensors there)
        f64, f32 = WF.reference(family, form="float"), WF.reference(family, torch.float32, form="float")
        out = max(WF.scaled_rms(f32.out[f], f64.out[f]) for f in range(WF.FRAMES))
        st = max((WF.scaled_rms(f32.state[n][b], f64.state[n][b]), n, b) for n in WF.state_names() for b in range(4))
        print("%s, float container: outputs %.2e x scale, states %.2e x scale (%s)" % (family, out, st[0], st[1]))
        assert out <= WF.CAP * WF.OUT_BOUND
        assert st[0] <= WF.CAP * WF.STATE_BOUND, st
    for U in (2, 3):
        # both block sets: every output frame of every utterance, and all 130 states of every utterance after every frame the references
        # keep them for (the end of every block and the mid-block frames tests/test_gpu_conv_variants.py reads through ragged counts)
        if family not in WF.block_set_families(U):
            continue
        b64, b32 = WF.block_reference(family, utterances=U), WF.block_reference(family, torch.float32, utterances=U)
        frames = b64.out.shape[0]
        assert frames == (WF.BLOCK_FRAMES if U == 2 else WF.BLOCK3_FRAMES) and b64.out.shape[1] == U
        assert set(b64.states_at) == set(b32.states_at) == set(WF.block_keep_frames(U)) and frames - 1 in b64.states_at
        out = max((WF.scaled_rms(b32.out[f, u], b64.out[f, u]), f, u) for f in range(frames) for u in range(U))
        st = max((WF.scaled_rms(b32.states_at[f][n][u], b64.states_at[f][n][u]), n, f, u)
                 for f in b64.states_at for n in WF.state_names() for u in range(U))
        print("%s, block-mode inputs, %d utterances: outputs %.2e x scale (share of the bound %.4f; frame %d, utterance %d), all 130 states after %d "
              "frames %.2e x scale (share %.4f; %s, frame %d, utterance %d)"
              % (family, U, out[0], out[0] / WF.OUT_BOUND, out[1], out[2], len(b64.states_at), st[0], st[0] / WF.STATE_BOUND, st[1], st[2], st[3]))
        assert out[0] <= WF.CAP * WF.OUT_BOUND, out
        assert st[0] <= WF.CAP * WF.STATE_BOUND, st
        for n in WF.state_names():
            assert np.array_equal(b64.states_at[frames - 1][n], b64.state[n]), n


def test_families_are_what_they_say():
    """The properties the GPU tests rely on, checked on the float64 oracle's own tensors: saturated gates in `satbias`, exactly constant
    LayerNorm rows in `const`, all-zero channels with scale 1.0 in `dead`, nine octaves of scales in `scales`, the four slopes in `alpha`,
    the three alternative container forms."""
    b = WF.family_tensors("satbias")["msfe4_en_lstm.b"].reshape(4, 21)
    for gate in range(4):
        assert sorted(set(np.rint(b[gate] / 2) * 2)) == [-100, -30, -8, 0, 8, 30, 100]
    ref = NutlsRef(parse_blob(WF.container("const")), batch=4, dtype=torch.float64)
    ref.trace = {}
    ref.step(WF.inputs(4)[0])
    beta, alpha = ref.w["msfe5_en_in.beta"], ref.w["msfe5_en_in.alpha"].reshape(())
    want = torch.clamp(beta, min=0) + alpha * torch.clamp(beta, max=0)
    assert torch.equal(ref.trace["msfe5_en.e0"], want.expand(4, 128, 64))          # variance exactly 0: the row is beta through PReLU
    raw = parse_blob(WF.container("dead"), dequantize=False)
    for layer in WF.DEAD_LAYERS:
        q, sc = raw[layer + ".w"]
        assert (sc[::3] == 1.0).all() and not q[::3].any(), layer
    raw = parse_blob(WF.container("scales"), dequantize=False)
    sc = raw["msfe6_en_conv2.w"][1]
    assert sc.max() / sc.min() > 64.0
    al = sorted({float(v.reshape(-1)[0]) for k, v in WF.family_tensors("alpha").items() if k.endswith(".alpha")})
    assert al == sorted(float(a) for a in WF.ALPHAS)
    raw = parse_blob(WF.container("forms_single_scale_convs"), dequantize=False)
    assert raw["msfe6_en_conv2.w"][1].size == 1 and raw["msfe6_en_ta.w1"][1].size == 16
    raw = parse_blob(WF.container("forms_int8_small_dense"), dequantize=False)
    assert sum(1 for k, v in raw.items() if isinstance(v, tuple) and v[0].shape == (32, 21)) == 4
    raw = parse_blob(WF.container("forms_float_gates"), dequantize=False)
    assert not isinstance(raw["msfe6_en_ta.w1"], tuple) and isinstance(raw["msfe6_en_lstm.wx"], tuple)


def test_the_bounds_see_one_wrong_entry_of_a_channel_permutation():
    """What the `scales` family is for.  A kernel that applied two neighbouring output channels' scales the wrong way round in ONE conv
    (one wrong entry pair of the packed channel permutation) is simulated on the float32 oracle: on `scales`, whose neighbours differ by
    octaves, the traced tensor behind that conv misses the GPU tests' bound many times over, and the first offender in plan order is that
    stage's CTFA output."""
    layer, (c0, c1) = "msfe4_de2_spconv3.w", (5, 6)
    raw = parse_blob(WF.container("scales"), dequantize=False)
    q, sc = raw[layer]
    assert sc[c0] != sc[c1]
    sc = sc.copy()
    sc[[c0, c1]] = sc[[c1, c0]]
    raw[layer] = (q, sc)
    x = WF.inputs(4)[:2]
    got, want = WF._oracle(write_blob(raw), x, torch.float32, trace=True), WF.reference("scales")
    bad = {n: WF.traced_op(n) for n in WF.traced_names() if not WF.rel_rms(got.trace[n][1], want.trace[n][1]) < WF.TRACE_BOUND}
    plan = [{"layer": "%s_ctfa" % st.prefix} for st in T.STAGES]
    assert bad and WF.first_in_plan_order(plan, bad) == "msfe4_de2.y", bad
    assert WF.rel_rms(got.trace["msfe4_de2.y"][1], want.trace["msfe4_de2.y"][1]) > 10 * WF.TRACE_BOUND
    assert not WF.scaled_rms(got.out[1], want.out[1]) < WF.OUT_BOUND
