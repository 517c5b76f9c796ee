"""CPU tests behind tests/test_gpu_ctfa_families.py (no GPU): the three gate families of tests/weight_families.py are what they say, the
float32 oracle stays within 1/20 of every bound on the 70 causal frames in both CTFA modes, and the bounds the GPU tests apply see an
attention window that is one frame short, one frame long, or not there at all -- oracle against oracle, no kernel involved."""
import numpy as np
import pytest
import torch

import weight_families as WF
from nunet_amd import topology as T
from oracle.nutls_ref import NutlsRef


def test_gate_families_are_what_they_say():
    """On the float64 causal32 reference's own gates.  `gatesat`: every stage has a time-attention channel under 1e-40 and one within
    1e-7 of 1.0, and so has its frequency attention, and a channel with such a ta hands the residual through unchanged, bit for bit.
    (Under 1e-40, not equal to 0.0: exp(100) does not overflow in double, sigmoid(-100) is 3.7e-44 there.  That is below float32's
    smallest normal number, 1.2e-38: in float32 with `__expf` and a reciprocal it is exactly 0, in double it is as good as 0.)  `gatedead`: the
    hidden layers of the gates n % 3 == 0 are identically zero on every frame, every second hidden unit of the gates n % 3 == 1 and every
    third channel of the gates n % 3 == 2 do not move.  `gatehist`: the frequency attention of stream 1 (silence, then a tone from frame 33
    on) moves by more than 0.1 in some channel between frame 32 and frame 64 -- the history matters."""
    gates = WF.gate_prefixes()
    assert len(gates) == 24 and gates[0].endswith("_fa") and gates[1].endswith("_ta")
    sat = WF.reference("gatesat", ctfa_mode="causal32")
    for st in T.STAGES:
        for kind in ("ta", "fa"):
            g = sat.trace["%s.%s" % (st.prefix, kind)]          # [frames, 4, 64]
            assert g.shape == (WF.CAUSAL_FRAMES, 4, 64)
            assert (g.min(axis=2) < 1e-40).all() and (g.max(axis=2) > 1.0 - 1e-7).all(), (st.prefix, kind)
    w = WF.family_tensors("gatesat")
    for n, g in enumerate(gates):
        assert sorted(set(np.rint(w[g + ".b2"] / 2) * 2)) == [-100, -30, -8, 0, 8, 30, 100], g
    # ta = 0 in a channel: the CTFA output of that channel is the residual e0, bit for bit
    ref = NutlsRef(WF.parse_blob(WF.container("gatesat")), batch=4, dtype=torch.float64, ctfa_mode="causal32")
    ref.trace = {}
    ref.step(WF.causal_streams()[0])
    for st in T.STAGES:
        zero = ref.trace[st.prefix + ".ta"] < 1e-40         # [4, 64]
        assert zero.any(dim=1).all()
        y, e0 = ref.trace[st.prefix + ".y"], ref.trace[st.prefix + ".e0"]
        sel = zero.unsqueeze(1).expand_as(y)
        assert torch.equal(y[sel], e0[sel]), st.prefix

    dead = WF.reference("gatedead", ctfa_mode="causal32")
    plain = WF.reference("plain", ctfa_mode="causal32")
    for n, g in enumerate(gates):
        prefix, kind = g.rsplit("_", 1)
        hid, gate = dead.trace["%s.%s_hid" % (prefix, kind)], dead.trace["%s.%s" % (prefix, kind)]
        assert hid.shape == (WF.CAUSAL_FRAMES, 4, 16)
        if n % 3 == 0:
            assert not hid.any(), g
            assert (gate == gate[0, 0]).all(), g          # sigmoid(b2) whatever comes in
            assert plain.trace["%s.%s_hid" % (prefix, kind)].any(), g
        elif n % 3 == 1:
            assert (hid[:, :, ::2] == hid[0, 0, ::2]).all() and not (hid[:, :, 1::2] == hid[0, 0, 1::2]).all(), g
        else:
            assert (gate[:, :, ::3] == gate[0, 0, ::3]).all() and not (gate[:, :, 1::3] == gate[0, 0, 1::3]).all(), g

    hist = WF.reference("gatehist", ctfa_mode="causal32")
    moved = max(float(np.abs(hist.trace[st.prefix + ".fa"][64, 1] - hist.trace[st.prefix + ".fa"][32, 1]).max()) for st in T.STAGES)
    plain_moved = max(float(np.abs(plain.trace[st.prefix + ".fa"][64, 1] - plain.trace[st.prefix + ".fa"][32, 1]).max()) for st in T.STAGES)
    print("fa of stream 1, frame 32 -> 64, largest move of a channel: gatehist %.3f, plain %.3f" % (moved, plain_moved))
    assert moved > 0.1


def test_causal_inputs_and_kept_frames():
    x = WF.causal_streams()
    assert x.shape == (WF.CAUSAL_FRAMES, 4, 256) and x.dtype == np.float32 and not x.flags.writeable
    assert not x[:33, 1].any() and (x[33:, 1, 40] == 50.0).all() and np.count_nonzero(x[33:, 1]) == WF.CAUSAL_FRAMES - 33
    assert (x[40:, 3] == np.float32(1e-20)).all() and x[:40, 3].max() > 0.1
    assert x[:, 0].max() > 0.5 and x[2, 0].max() < 0.2 * x[0, 0].max()          # the gain swings
    assert WF.causal_keep_frames() == frozenset({16, 17, 48, 50, 69, 32, 64, 25, 19})
    assert set(WF.CAUSAL_FAMILIES) <= set(WF.BASE_FAMILIES) and set(WF.GATE_FAMILIES) <= set(WF.CAUSAL_FAMILIES)
    assert not set(WF.GATE_FAMILIES) & (set(WF.BLOCK_FAMILIES) | set(WF.BLOCK3_FAMILIES))


@pytest.mark.parametrize("ctfa_mode", ["frame", "causal32"])
@pytest.mark.parametrize("family", WF.CAUSAL_FAMILIES)
def test_causal_conditioning_cap(family, ctfa_mode):
    """The condition of tests/test_weight_families.py::test_conditioning_cap on the 70 causal frames, in both CTFA modes: the float32
    oracle lies within 1/20 of the bound on the output of every frame, on each of the 18 traced tensors of every frame of
    CAUSAL_TRACE_FRAMES and on each of the 130 states of every stream after every frame the references keep them for."""
    r64, r32 = WF.reference(family, ctfa_mode=ctfa_mode, frames="causal"), WF.reference(family, torch.float32, ctfa_mode=ctfa_mode, frames="causal")
    assert np.isfinite(r64.out).all() and np.isfinite(r32.out).all() and r64.out.shape == (WF.CAUSAL_FRAMES, 4, 256)
    assert set(r64.states_at) == set(WF.causal_keep_frames())
    out = max((WF.scaled_rms(r32.out[f], r64.out[f]), f) for f in range(WF.CAUSAL_FRAMES))
    tr = max((WF.rel_rms(r32.trace[n][f], r64.trace[n][f]), n, f) for n in WF.traced_names() for f in WF.CAUSAL_TRACE_FRAMES)
    st = max((WF.scaled_rms(r32.states_at[f][n][b], r64.states_at[f][n][b]), n, f, b)
             for f in r64.states_at for n in WF.state_names() for b in range(4))
    print("%s, %s, 70 causal frames: float32 oracle vs float64 oracle: outputs %.4f of the bound (frame %d), traced %.4f of the bound (%s, "
          "frame %d), states %.4f of the bound (%s after frame %d, stream %d); cap %.4f"
          % (family, ctfa_mode, out[0] / WF.OUT_BOUND, out[1], tr[0] / WF.TRACE_BOUND, tr[1], tr[2], st[0] / WF.STATE_BOUND, st[1], st[2], st[3], WF.CAP))
    assert out[0] <= WF.CAP * WF.OUT_BOUND, out
    assert tr[0] <= WF.CAP * WF.TRACE_BOUND, tr
    assert st[0] <= WF.CAP * WF.STATE_BOUND, st
    for n in WF.state_names():
        assert np.array_equal(r64.states_at[WF.CAUSAL_FRAMES - 1][n], r64.state[n]), n


ROUNDING = 1e-12          # float64 runs of the same function whose sums are formed in another order


class _Window(NutlsRef):
    """The causal32 oracle with ``rows`` frames of history next to the current one instead of 31; still divided by 32."""
    rows = 31

    def _ctfa(self, x, e0, prefix):
        ta = self._mlp_gate(x.mean(dim=1), prefix + "_ta")
        hist = self.ta_hist.setdefault(prefix, torch.zeros(self.batch, self.rows, 64, dtype=self.dtype))
        fa = self._mlp_gate((hist.sum(dim=1) + ta) / 32.0, prefix + "_fa")
        self.ta_hist[prefix] = torch.cat([hist[:, 1:], ta.unsqueeze(1)], dim=1)
        return x * (ta * fa).unsqueeze(1) + e0


class _Window31(_Window):
    rows = 30


class _Window33(_Window):
    """what a ring of 32 rows gives when the row about to be overwritten (the frame 32 back) is summed too"""
    rows = 32


def test_window_mutant_is_the_oracle_at_31_rows():
    x = WF.causal_streams()[:34, :1]
    a = WF._oracle(WF.container("plain"), x, torch.float64, trace=False, ctfa_mode="causal32", oracle=_Window)
    assert WF.scaled_rms(a.out, WF.reference("plain", ctfa_mode="causal32").out[:34, :1]) < ROUNDING          # (another batch size: not bit for bit)


@pytest.mark.parametrize("family", WF.CAUSAL_FAMILIES)
def test_the_bounds_see_a_wrong_attention_window(family):
    """float64 against float64 on the 70 causal frames, frames >= 32: an attention window of 31 frames, one of 33 frames, and the
    frame-mode formula each miss OUT_BOUND on at least one frame by at least 10x.  The factors are printed."""
    want = WF.reference(family, ctfa_mode="causal32")
    blob, x = WF.container(family), WF.causal_streams()
    mutants = {"31-frame window": WF._oracle(blob, x, torch.float64, trace=False, ctfa_mode="causal32", oracle=_Window31),
               "33-frame window": WF._oracle(blob, x, torch.float64, trace=False, ctfa_mode="causal32", oracle=_Window33),
               "frame-mode formula": WF.reference(family, ctfa_mode="frame", frames="causal")}
    factors = {}
    for name, got in mutants.items():
        first = 31 if name == "31-frame window" else 32 if name == "33-frame window" else 1
        # the mutant is the oracle until the frame at which its window first differs (sums of other lengths round differently: not bit for bit)
        assert WF.scaled_rms(got.out[:first], want.out[:first]) < ROUNDING < 1e-9 < WF.scaled_rms(got.out[first], want.out[first]), name
        factors[name] = max((WF.scaled_rms(got.out[f], want.out[f]) / WF.OUT_BOUND, f) for f in range(32, WF.CAUSAL_FRAMES))
    print("%s: worst frame >= 32 over OUT_BOUND: %s" % (family, ", ".join("%s %.0fx (frame %d)" % (k, v[0], v[1]) for k, v in factors.items())))
    for name, (factor, _) in factors.items():
        assert factor >= 10.0, (name, factor)
