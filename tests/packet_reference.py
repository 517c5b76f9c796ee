"""Packet mode of the PCM gateway (include/nutls.h, "Packet mode"): the arithmetic in plain numpy -- a per-stream FIFO model, no library.

S = samples of a hop, P = samples of a packet, g = gcd(P, S).  Every stream has an input FIFO that starts empty and an output FIFO that
starts with D = S - g samples of silence.  A tick, for every active stream: push P samples; while at least S are waiting take the oldest S
as one hop and append the hop's result to the output FIFO; pop P samples.  A held stream keeps everything and returns silence.

``plan`` is the closed form, ``brute_force`` the simulation it is held against (tests/test_pcm_packet_abi.py).  ``FifoModel`` follows a run
tick by tick: from the mask schedule and the packets fed it says which hops each stream takes (``items``: what a reference handle is fed
through the hop entry, in lockstep: ``lockstep``), the fill of every input FIFO after every tick and the rounds of every tick; from the hop
outputs of that reference run it returns the expected packets (``expected``)."""
from math import gcd

import numpy as np


def plan(P, S):
    """{"delay": D, "rounds": R, "fifo": S - g + P}"""
    g = gcd(P, S)
    return {"delay": S - g, "rounds": (S - g + P) // S, "fifo": S - g + P}


def accepted(P, S, sample_bytes):
    """The length rule: the packet's bytes are a multiple of 16 and 1 <= P <= 4 S"""
    return 1 <= P <= 4 * S and (P * sample_bytes) % 16 == 0


def brute_force(P, S, ticks=None):
    """Simulate one always-active stream WITHOUT priming for ``ticks`` ticks (default: two periods of S / g) and read the plan off it:
    delay = the smallest priming with which the pop never underruns, rounds = the most hops a tick took, fifo = the most samples either FIFO
    held at any moment once primed with that delay."""
    ticks = ticks or 2 * S // gcd(P, S)
    fill_in = out = 0
    low = rounds = most_in = 0
    outs = []
    for _ in range(ticks):
        fill_in += P
        most_in = max(most_in, fill_in)
        r = 0
        while fill_in >= S:
            fill_in -= S
            out += S
            r += 1
        outs.append(out)          # the output FIFO at its fullest in this tick, less the priming
        out -= P
        low = min(low, out)
        rounds = max(rounds, r)
    delay = -low
    most_out = max(o + delay for o in outs)
    return {"delay": delay, "rounds": rounds, "fifo": max(most_in, most_out)}


class FifoModel:
    """B streams, packets of P samples, hops of S samples, ``silence`` the sample value of silence in ``dtype``."""

    def __init__(self, B, P, S, silence, dtype):
        self.B, self.S, self.silence, self.dtype = B, S, silence, np.dtype(dtype)
        self.items = [[] for _ in range(B)]          # per stream: [reset_before, hop input [S]] in the order the stream takes them
        self.fresh = [True] * B                      # the stream's next hop is the first since its reset
        self.log = []                                # ("tick", active [B], took [B], P) | ("prime", b, D)
        self.fills, self.rounds = [], []             # per tick: fill of every input FIFO after it [B], hop rounds
        self.fifo = [np.empty(0, self.dtype) for _ in range(B)]
        self.set_packet(P)

    def set_packet(self, P):
        """nutls_set_pcm_packet: every stream's FIFOs start anew; model state and resampler histories stay (no reset mark)"""
        self.P, self.D = P, plan(P, self.S)["delay"]
        for b in range(self.B):
            self.fifo[b] = np.empty(0, self.dtype)
            self.log.append(("prime", b, self.D))

    def reset(self, b=-1):
        """nutls_reset(h, b): the stream starts anew, FIFOs included"""
        for s in (range(self.B) if b < 0 else [b]):
            self.fifo[s] = np.empty(0, self.dtype)
            self.fresh[s] = True
            self.log.append(("prime", s, self.D))

    def tick(self, active, packets):
        """``active`` [B] or None, ``packets`` [B, P] (held rows are not looked at).  Returns (rounds, fills)."""
        act = np.ones(self.B, bool) if active is None else np.asarray(active).astype(bool)
        took = np.zeros(self.B, int)
        for b in range(self.B):
            if not act[b]:
                continue
            self.fifo[b] = np.concatenate([self.fifo[b], np.asarray(packets[b], self.dtype)])
            while len(self.fifo[b]) >= self.S:
                self.items[b].append([self.fresh[b], self.fifo[b][:self.S].copy()])
                self.fresh[b] = False
                self.fifo[b] = self.fifo[b][self.S:]
                took[b] += 1
        self.log.append(("tick", act, took, self.P))
        self.fills.append(np.array([len(f) for f in self.fifo], np.int32))
        self.rounds.append(int(took.max()))
        return self.rounds[-1], self.fills[-1]

    def expected(self, hop_outs):
        """``hop_outs[b]``: the results [S] of the stream's hops, one per item -> the expected packets of every tick, [ticks][B, P(tick)]"""
        out = [np.empty(0, self.dtype) for _ in range(self.B)]
        used = [0] * self.B
        res = []
        for ev in self.log:
            if ev[0] == "prime":
                out[ev[1]] = np.full(ev[2], self.silence, self.dtype)
                continue
            _, act, took, P = ev
            pk = np.full((self.B, P), self.silence, self.dtype)
            for b in range(self.B):
                if not act[b]:
                    continue
                for _ in range(took[b]):
                    out[b] = np.concatenate([out[b], np.asarray(hop_outs[b][used[b]], self.dtype)])
                    used[b] += 1
                assert len(out[b]) >= P, "the model underran: stream %d holds %d of %d samples" % (b, len(out[b]), P)
                pk[b], out[b] = out[b][:P], out[b][P:]
            res.append(pk)
        return res


def lockstep(items, hop, reset, B, S, dtype, poison):
    """Feed a reference handle every stream's hops through the hop entry, in lockstep BY HOP INDEX (not by the packet run's ticks: the masks
    differ from the packet handle's, and the header promises that this changes no bit): step i takes item i of every stream that has one.
    ``hop(x [B, S], active [B] bool or None) -> [B, S]``; ``reset(b)``; held rows are fed ``poison``.  Returns hop_outs[b] = [result [S], ...]."""
    outs = [[] for _ in range(B)]
    for i in range(max(len(it) for it in items)):
        have = np.array([len(it) > i for it in items])
        x = np.full((B, S), poison, dtype)
        for b in range(B):
            if have[b]:
                if items[b][i][0]:
                    reset(b)
                x[b] = items[b][i][1]
        y = hop(x, None if have.all() else have)
        for b in range(B):
            if have[b]:
                outs[b].append(np.array(y[b]))
    return outs
