"""Model of one wavefront of csrc/stft_block.hip in numpy: the index arithmetic of the four radix-4 stages, of the
exchanges through the wave's LDS image and of the real-transform split / merge passes, lane by lane.

    python tools/check_stft_block_lds.py

* checks the transform against ``np.fft`` (forward: rfft of a real frame; inverse: irfft of a Hermitian spectrum);
* enumerates, for every LDS instruction of every exchange, the float2 slots of each lane group and counts the bank
  conflicts by the gfx950 rules for 8-byte accesses: ``ds_write_b64`` is served in four groups of 16 consecutive
  lanes with bank = dword address mod 32 (float2 slot mod 16), ``ds_read_b64`` in two groups of 32 lanes with
  bank = dword address mod 64 (float2 slot mod 32).  Expected: 0 extra cycles everywhere.

The formulas here restate the kernel's; when one changes, change both (tests/test_stft_block_model.py runs this).
"""
from __future__ import annotations

import numpy as np

LANES = np.arange(64)
IMAGE = 320


def nat(k):
    return k ^ (((k >> 4) & 1) << 1) ^ ((k >> 5) & 1)


def spec(k):
    return k ^ ((k >> 4) & 1)


class Image:
    """The wave's LDS image; records the extra cycles of every access."""

    def __init__(self):
        self.buf = np.zeros(IMAGE, np.complex128)
        self.conflicts = []

    @staticmethod
    def _extra(slots, group, modulus):
        extra = 0
        for g in range(0, 64, group):
            s = np.unique(slots[g:g + group])          # identical addresses broadcast
            banks = s % modulus
            extra += int(np.max(np.bincount(banks, minlength=modulus))) - 1
        return extra

    def write(self, name, slots, values, mask=None):
        slots = np.asarray(slots)
        if mask is None:
            self.conflicts.append((name + " (write)", self._extra(slots, 16, 16)))
            assert len(np.unique(slots)) == 64, name
            self.buf[slots] = values
        else:
            self.buf[slots[mask]] = np.asarray(values)[mask]

    def read(self, name, slots):
        slots = np.asarray(slots)
        self.conflicts.append((name + " (read)", self._extra(slots, 32, 32)))
        return self.buf[slots].copy()


def bfly4(x):
    """x [64, 4] -> y[:, q] = sum_a x[:, a] (-i)^(a q)"""
    q = np.arange(4)
    return x @ ((-1j) ** np.outer(q, q))


def fft256(x, img):
    """x [64, 4]: lane l holds z[l + 64 a].  Leaves Z[k] at image slot nat(k)."""
    l = LANES
    k0, l0, k1, l00 = l >> 4, l & 15, (l >> 2) & 3, l & 3
    q = np.arange(4)
    x = bfly4(x) * np.exp(-2j * np.pi * np.outer(l, q) / 256)
    for j in range(4):
        img.write("exchange 1", 80 * j + l, x[:, j])
    x = np.stack([img.read("exchange 1", 80 * k0 + l0 + 16 * a) for a in range(4)], axis=1)
    x = bfly4(x) * np.exp(-2j * np.pi * np.outer(l0, q) / 64)
    for j in range(4):
        img.write("exchange 2", 80 * k0 + 20 * j + l0, x[:, j])
    x = np.stack([img.read("exchange 2", 80 * k0 + 20 * k1 + l00 + 4 * a) for a in range(4)], axis=1)
    x = bfly4(x) * np.exp(-2j * np.pi * np.outer(l00, q) / 16)
    for j in range(4):
        img.write("exchange 3", 80 * k0 + 20 * k1 + 4 * l00 + (j ^ l00), x[:, j])
    x = np.stack([img.read("exchange 3", 80 * k0 + 20 * k1 + 4 * a + (l00 ^ a)) for a in range(4)], axis=1)
    x = bfly4(x)
    kb = k0 + 4 * k1 + 16 * l00
    for j in range(4):
        img.write("exchange 4", nat(kb + 64 * j), x[:, j])


def analysis(frame):
    """512 real samples -> X[0..256] as the kernel computes it."""
    img = Image()
    l = LANES
    z = frame[0::2] + 1j * frame[1::2]
    fft256(np.stack([z[l + 64 * a] for a in range(4)], axis=1), img)
    out = np.zeros(257, np.complex128)
    for i in range(4):
        k = 2 * l + 1 + (i & 1) + 128 * (i >> 1)
        zk, zm = img.read("split", nat(k & 255)), img.read("split mirror", nat(256 - k))
        e, o = 0.5 * (zk + np.conj(zm)), -0.5j * (zk - np.conj(zm))
        out[k] = e + np.exp(-2j * np.pi * k / 512) * o
    z0 = img.buf[0]
    out[0] = z0.real + z0.imag
    return out, img.conflicts


def synthesis(spectrum):
    """Y[0..256] -> the 512 real samples of the unscaled inverse transform, as the kernel computes them."""
    img = Image()
    l = LANES
    for i in range(4):
        k = 2 * l + 1 + (i & 1) + 128 * (i >> 1)
        y = np.where(k == 256, spectrum[k].real, spectrum[k])
        img.write("spectrum", np.where(k == 256, 256, spec(k)), y)
    img.write("spectrum bin 0", np.zeros(64, int), np.full(64, spectrum[0].real), mask=l == 0)
    x = []
    for a in range(4):
        k = l + 64 * a
        yk, ym = img.read("merge", spec(k)), img.read("merge mirror", np.where(k == 0, 256, spec((256 - k) & 255)))
        e, o = yk + np.conj(ym), (yk - np.conj(ym)) * np.exp(2j * np.pi * k / 512)
        zz = e + 1j * o
        x.append(zz.imag + 1j * zz.real)                       # re / im swapped: the forward FFT then computes the inverse
    fft256(np.stack(x, axis=1), img)
    out = np.zeros(512)
    for a in range(4):
        z = img.read("result", nat(l + 64 * a))
        out[2 * (l + 64 * a)] = z.imag
        out[2 * (l + 64 * a) + 1] = z.real
    return out, img.conflicts


def main():
    rng = np.random.default_rng(0)
    frame = rng.standard_normal(512)
    got, c1 = analysis(frame)
    err_f = np.abs(got - np.fft.rfft(frame)).max()
    spectrum = np.fft.rfft(rng.standard_normal(512))
    back, c2 = synthesis(spectrum)
    err_i = np.abs(back / 512 - np.fft.irfft(spectrum)).max()
    worst = {}
    for name, extra in c1 + c2:
        worst[name] = max(worst.get(name, 0), extra)
    for name, extra in worst.items():
        print("%-28s extra LDS cycles per instruction: %d" % (name, extra))
    print("forward max error %.2e, inverse max error %.2e" % (err_f, err_i))
    return err_f, err_i, worst


if __name__ == "__main__":
    main()
