"""The attenuation limit (include/nutls.h, "Attenuation limit") in double, and the limits the tests put on the eight designed signals of
tests/transform_signals.py -- a plain helper module shared by tests/test_atten_limit_abi.py and tests/test_gpu_atten_limit.py."""
import numpy as np

L = np.float32([0.0, 1.0, 0.5, 0.1, 2.0 ** -10, 1.0 - 2.0 ** -24, 0.999, 1e-3])
"""One limit per row of ``transform_signals.signals()``: both exact ends, a half, a typical 20 dB cap, a small power of two, the float32 below
1 (whose companion weight is 2^-24), a value whose companion weight is inexact, and a small inexact value."""


def companion(limit):
    """``c = (float)(1.0 - (double)l)`` as the library forms it, float32"""
    return (1.0 - np.asarray(limit, np.float32).astype(np.float64)).astype(np.float32)


def mix64(noisy, est, limit):
    """``l x + c e`` in double, not rounded: ``noisy``, ``est`` ``[S, n, 256]``, ``limit [S]`` (the float32 values the getter returns)."""
    l32 = np.asarray(limit, np.float32)
    l, c = l32.astype(np.float64), companion(l32).astype(np.float64)
    shape = (-1,) + (1,) * (np.ndim(noisy) - 1)
    return l.reshape(shape) * np.asarray(noisy, np.float64) + c.reshape(shape) * np.asarray(est, np.float64)
