"""The layout rule of ``nutls_set_pcm_channels`` (include/nutls.h, "Channels") in numpy: a reshape and a transpose, nothing else.  The
library's host functions, its kernels and every ``_pcm`` entry with C channels are compared with these, bit for bit
(tests/test_pcm_channels_abi.py, tests/test_gpu_pcm_channels.py).  No reference counterpart: the reference takes one float row per call
(dnn_model/interpreter_proposed.py:384-385)."""
import numpy as np


def deinterleave(frames):
    """``[n, C]`` -> ``[C, n]``: one row per channel."""
    frames = np.asarray(frames)
    assert frames.ndim == 2
    return np.ascontiguousarray(frames.T)


def interleave(rows):
    """``[C, n]`` -> ``[n, C]``: the inverse."""
    rows = np.asarray(rows)
    assert rows.ndim == 2
    return np.ascontiguousarray(rows.T)


def split_rows(x, channels):
    """A callers' buffer ``[B / C, n * C]`` (or ``[B / C, n, C]``) -> ``[B, n]``: row ``r * C + c`` is channel c of frame row r."""
    x = np.asarray(x)
    r = x.shape[0]
    n = x.shape[1] // channels if x.ndim == 2 else x.shape[1]
    return np.ascontiguousarray(x.reshape(r, n, channels).transpose(0, 2, 1).reshape(r * channels, n))


def join_rows(rows, channels):
    """``[B, n]`` -> the callers' buffer ``[B / C, n * C]``: the inverse of :func:`split_rows`."""
    rows = np.asarray(rows)
    b, n = rows.shape
    return np.ascontiguousarray(rows.reshape(b // channels, channels, n).transpose(0, 2, 1).reshape(b // channels, n * channels))
