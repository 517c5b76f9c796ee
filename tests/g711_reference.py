"""G.711 mu-law and A-law in numpy, written from the text of include/nutls.h ("PCM gateway", G.711) alone: it does not call the library.
``expand(codec)``: the int16 value of each of the 256 codes; ``compress(codec, s)``: the codes of an int16 array.  ``>>`` on numpy's
signed integers is the arithmetic shift the header asks for."""
import numpy as np

CODECS = ("ulaw", "alaw")
SILENCE = {"ulaw": 0xFF, "alaw": 0xD5}
# the segment ends of the two compressions, and the int16 range of the two expansions
ENDS = {"ulaw": (0x3F, 0x7F, 0xFF, 0x1FF, 0x3FF, 0x7FF, 0xFFF, 0x1FFF), "alaw": (0x1F, 0x3F, 0x7F, 0xFF, 0x1FF, 0x3FF, 0x7FF, 0xFFF)}
PEAK = {"ulaw": 32124, "alaw": 32256}


def expand(codec):
    """[256] int16: table[c] = the value of code c."""
    c = np.arange(256, dtype=np.int64)
    if codec == "ulaw":
        u = ~c & 0xFF
        t = (((u & 15) << 3) + 0x84) << ((u & 0x70) >> 4)
        s = np.where(u & 0x80, 0x84 - t, t - 0x84)
    elif codec == "alaw":
        a = c ^ 0x55
        t = (a & 15) << 4
        g = (a & 0x70) >> 4
        t = np.where(g == 0, t + 8, (t + 0x108) << np.maximum(g - 1, 0))
        s = np.where(a & 0x80, t, -t)
    else:
        raise ValueError(codec)
    assert np.abs(s).max() == PEAK[codec]
    return s.astype(np.int16)


def compress(codec, s):
    """uint8 array of s's shape: the code of every int16 value."""
    s = np.asarray(s)
    assert s.dtype == np.int16
    s = s.astype(np.int64)
    if codec == "ulaw":
        v = s >> 2
        mask = np.where(v < 0, 0x7F, 0xFF)
        v = np.where(v < 0, -v, v)
        v = np.minimum(v, 8159) + 33
        seg = sum((v > end).astype(np.int64) for end in ENDS[codec])
        code = np.where(seg >= 8, 0x7F, (np.minimum(seg, 7) << 4) | ((v >> (seg + 1)) & 15))
    elif codec == "alaw":
        v = s >> 3
        mask = np.where(v < 0, 0x55, 0xD5)
        v = np.where(v < 0, -v - 1, v)
        seg = sum((v > end).astype(np.int64) for end in ENDS[codec])
        code = np.where(seg >= 8, 0x7F, (np.minimum(seg, 7) << 4) | (np.where(seg < 2, v >> 1, v >> seg) & 15))
    else:
        raise ValueError(codec)
    return (code ^ mask).astype(np.uint8)


def segment_edges(codec):
    """The int16 values on both sides of every segment end of ``codec``'s compression, for both signs: the smallest |s| whose magnitude v
    exceeds the end, and the one below it."""
    out = []
    for end in ENDS[codec]:
        if codec == "ulaw":          # v = (|s| >> 2) + 33 for s >= 0; for s < 0, v = -(s >> 2) + 33
            first = (end + 1 - 33) << 2              # the smallest s >= 0 with v = end + 1
            out += [first - 1, first]
            out += [-(first - 4), -(first - 4) - 1]   # s < 0: -(s >> 2) = ceil(-s / 4); v = end + 1 from -s = first - 3 on
        else:                        # v = s >> 3 for s >= 0; for s < 0, v = -(s >> 3) - 1 = (-s - 1) >> 3
            first = (end + 1) << 3
            out += [first - 1, first, -first, -first - 1]
    return [int(x) for x in out if -32768 <= x <= 32767]
