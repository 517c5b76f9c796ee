"""Host-side mirror of the reference's model call surface, bound to the HIP library through
the C ABI of ``include/nutls.h`` with ``ctypes``.

* :class:`NutlsRunner` -- drop-in for the TF-Lite signature runner the reference obtains with
  ``interpreter.get_signature_runner('nutls_lstm_sm')`` and calls once per frame with 131 named
  tensors (``/root/reference/dnn_model/interpreter_proposed.py:380, 215-350``): same names,
  shapes, dtypes, same ``ValueError`` on unknown / missing names or wrong shapes; batch 1.
* :class:`NutlsEngine` -- the batched form of the same step: ``B`` independent streams, all 130
  recurrent-state tensors resident in HBM, ``step(mag[B,256]) -> out[B,256]``.

There is no CPU fallback: constructing either class without the built ``libnutls_hip.so`` or
without a gfx950 GPU raises ``RuntimeError``.
"""
from __future__ import annotations

import ctypes
import os
from typing import Dict, List, Optional, Tuple

import numpy as np

from . import topology as T
from .weights import DEFAULT_WEIGHTS, parse_blob, read_blob

_HERE_LIB = os.path.join(os.path.dirname(os.path.abspath(__file__)), "libnutls_hip.so")
# NUTLS_LIB: developer knob -- another build of the SAME library (tools/exp: timing experiments on the step kernel).  Honoured only
# together with NUTLS_DEV=1, and the library must report the version string this wrapper was written against (load_library).
_LIB_PATH = (os.environ.get("NUTLS_LIB") if os.environ.get("NUTLS_DEV") == "1" else None) or _HERE_LIB
ABI_VERSION_PREFIX = b"nutls-hip 0.4"
_lib = None

NUTLS_ERR_ARG = -1

# every symbol include/nutls.h declares (tests check the library exports all of them)
ABI_SYMBOLS = (
    "nutls_create", "nutls_destroy", "nutls_step", "nutls_step_host", "nutls_io_buffers",
    "nutls_use_graph", "nutls_set_mode", "nutls_state_get", "nutls_state_set", "nutls_state_count",
    "nutls_state_info", "nutls_reset", "nutls_debug_get", "nutls_debug_trace", "nutls_debug_knob", "nutls_batch",
    "nutls_launches_per_step", "nutls_launch_info", "nutls_profile_step",
    "nutls_last_error",
    "nutls_version", "nutls_host_alloc", "nutls_host_free",
    "nutls_enhance_hop", "nutls_enhance_hop_host", "nutls_stft_hop", "nutls_istft_hop",
    "nutls_create_offline", "nutls_create_offline_batch", "nutls_process_block", "nutls_process_block_host",
    "nutls_fused_num_ops", "nutls_fused_op_info", "nutls_profile_fused", "nutls_profile_production",
    "nutls_fused_blob_floats", "nutls_fused_pack_blob", "nutls_state_get_all", "nutls_offline_set_ctfa_mode",
    "nutls_offline_set_pipeline", "nutls_streams_per_workgroup", "nutls_fused_plan_blob_floats", "nutls_fused_pack_blob_plan",
    "nutls_set_ctfa_mode", "nutls_fused_plan_num_ops", "nutls_fused_plan_op_info", "nutls_create_plan",
    "nutls_enhance_block", "nutls_enhance_block_host", "nutls_stft_block", "nutls_istft_block",
    "nutls_step_active", "nutls_step_host_active", "nutls_enhance_hop_active", "nutls_enhance_hop_host_active",
    "nutls_set_hop_fusion", "nutls_launches_per_hop",
    "nutls_process_block_ragged", "nutls_process_block_ragged_host", "nutls_enhance_block_ragged", "nutls_enhance_block_ragged_host",
    "nutls_stft_block_ragged", "nutls_istft_block_ragged",
    "nutls_launch_conv_shape", "nutls_conv_dispatch",
    "nutls_set_pcm_format", "nutls_pcm_hop_samples", "nutls_pcm_delay_samples", "nutls_pcm_filter_taps", "nutls_pcm_filter",
    "nutls_enhance_hop_pcm", "nutls_enhance_hop_pcm_active", "nutls_enhance_hop_pcm_host", "nutls_enhance_hop_pcm_host_active",
    "nutls_pcm_decode_hop", "nutls_pcm_encode_hop",
    "nutls_enhance_block_pcm", "nutls_enhance_block_pcm_host", "nutls_pcm_decode_block", "nutls_pcm_encode_block",
    "nutls_enhance_block_pcm_ragged", "nutls_enhance_block_pcm_ragged_host", "nutls_pcm_decode_block_ragged", "nutls_pcm_encode_block_ragged",
    "nutls_set_pcm_upper_band", "nutls_pcm_upper_band",
    "nutls_set_pcm_upper_follow", "nutls_pcm_upper_follow", "nutls_pcm_follow_gain",
    "nutls_set_atten_limit", "nutls_atten_limit", "nutls_istft_block_mix",
    "nutls_pcm_packet_plan", "nutls_set_pcm_packet", "nutls_pcm_packet_samples", "nutls_pcm_packet_delay_samples", "nutls_pcm_packet_fill",
    "nutls_pcm_packet_last_rounds", "nutls_enhance_packet_pcm", "nutls_enhance_packet_pcm_host",
    "nutls_set_pcm_channels", "nutls_pcm_channels", "nutls_pcm_deinterleave", "nutls_pcm_interleave",
)
# ... and the declared symbols whose names carry a digit, listed apart: tests/test_abi.py compares ABI_SYMBOLS with the names it finds in
# the header by a pattern of lower-case letters and underscores, which cannot see these
ABI_SYMBOLS_G711 = ("nutls_pcm_g711_expand", "nutls_pcm_g711_compress")


def load_library(path: Optional[str] = None) -> ctypes.CDLL:
    """dlopen the HIP library and declare the C ABI.  Fails loudly when it is missing."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    p = path or _LIB_PATH
    if not os.path.exists(p):
        raise RuntimeError(
            "HIP library %s not found -- build it with `python -m nunet_amd.build` "
            "(there is no CPU fallback for the model step)" % p)
    lib = ctypes.CDLL(p)
    c = ctypes
    lib.nutls_version.restype = c.c_char_p
    ver = lib.nutls_version()
    if not ver.startswith(ABI_VERSION_PREFIX):
        raise RuntimeError("%s reports %r, this wrapper binds %r: rebuild the library (python -m nunet_amd.build)"
                           % (p, ver, ABI_VERSION_PREFIX))
    fp = c.POINTER(c.c_float)
    dev_lib = p != _HERE_LIB      # (NUTLS_DEV=1 NUTLS_LIB=...: an experimental or OLDER build for an A/B run may lack the newest entry points)
    lib.nutls_create.argtypes = [c.c_void_p, c.c_size_t, c.c_int, c.c_int, c.c_int, c.POINTER(c.c_void_p)]
    lib.nutls_create_plan.argtypes = [c.c_void_p, c.c_size_t, c.c_int, c.c_int, c.c_int, c.c_int, c.POINTER(c.c_void_p)]
    lib.nutls_destroy.argtypes = [c.c_void_p]
    lib.nutls_step.argtypes = [c.c_void_p, c.c_void_p, c.c_void_p, c.c_void_p]
    lib.nutls_step_host.argtypes = [c.c_void_p, fp, fp]
    if not dev_lib or hasattr(lib, "nutls_host_alloc"):
        lib.nutls_host_alloc.argtypes = [c.c_size_t]
        lib.nutls_host_alloc.restype = c.c_void_p
        lib.nutls_host_free.argtypes = [c.c_void_p]
        lib.nutls_host_free.restype = None
    lib.nutls_io_buffers.argtypes = [c.c_void_p, c.POINTER(c.c_void_p), c.POINTER(c.c_void_p)]
    lib.nutls_use_graph.argtypes = [c.c_void_p, c.c_int]
    lib.nutls_set_mode.argtypes = [c.c_void_p, c.c_int]
    lib.nutls_state_get.argtypes = [c.c_void_p, c.c_char_p, fp, c.c_size_t]
    lib.nutls_state_set.argtypes = [c.c_void_p, c.c_char_p, fp, c.c_size_t]
    lib.nutls_state_get_all.argtypes = [c.c_void_p, c.c_int, fp, c.c_size_t]
    lib.nutls_state_count.argtypes = [c.c_void_p]
    lib.nutls_state_info.argtypes = [c.c_void_p, c.c_int, c.POINTER(c.c_char_p), c.POINTER(c.c_int), c.POINTER(c.c_int)]
    lib.nutls_reset.argtypes = [c.c_void_p, c.c_int]
    lib.nutls_debug_get.argtypes = [c.c_void_p, c.c_char_p, fp, c.c_size_t]
    if not dev_lib or hasattr(lib, "nutls_debug_trace"):
        lib.nutls_debug_trace.argtypes = [c.c_void_p, c.c_int]
    if not dev_lib or hasattr(lib, "nutls_debug_knob"):
        lib.nutls_debug_knob.argtypes = [c.c_void_p, c.c_char_p, c.c_int]
    lib.nutls_batch.argtypes = [c.c_void_p]
    lib.nutls_streams_per_workgroup.argtypes = [c.c_void_p]
    lib.nutls_launches_per_step.argtypes = [c.c_void_p]
    lib.nutls_launch_info.argtypes = [c.c_void_p, c.c_int, c.POINTER(c.c_char_p), c.POINTER(c.c_char_p),
                                      c.POINTER(c.c_double), c.POINTER(c.c_double)]
    lib.nutls_profile_step.argtypes = [c.c_void_p, fp, c.c_int]
    lib.nutls_enhance_hop.argtypes = [c.c_void_p, c.c_void_p, c.c_void_p, c.c_int, c.c_void_p]
    lib.nutls_enhance_hop_host.argtypes = [c.c_void_p, fp, fp, c.c_int]
    lib.nutls_stft_hop.argtypes = [c.c_void_p, c.c_void_p, c.c_void_p]
    lib.nutls_istft_hop.argtypes = [c.c_void_p, c.c_void_p, c.c_int, c.c_void_p]
    if not dev_lib or hasattr(lib, "nutls_enhance_block"):
        lib.nutls_enhance_block.argtypes = [c.c_void_p, c.c_void_p, c.c_void_p, c.c_int, c.c_int, c.c_void_p]
        lib.nutls_enhance_block_host.argtypes = [c.c_void_p, fp, fp, c.c_int, c.c_int]
        lib.nutls_stft_block.argtypes = [c.c_void_p, c.c_void_p, c.c_void_p, c.c_int, c.c_void_p]
        lib.nutls_istft_block.argtypes = [c.c_void_p, c.c_void_p, c.c_void_p, c.c_int, c.c_int, c.c_void_p]
    if not dev_lib or hasattr(lib, "nutls_step_active"):
        lib.nutls_step_active.argtypes = [c.c_void_p, c.c_void_p, c.c_void_p, c.c_void_p, c.c_void_p]
        lib.nutls_step_host_active.argtypes = [c.c_void_p, fp, fp, c.c_void_p]
        lib.nutls_enhance_hop_active.argtypes = [c.c_void_p, c.c_void_p, c.c_void_p, c.c_void_p, c.c_int, c.c_void_p]
        lib.nutls_enhance_hop_host_active.argtypes = [c.c_void_p, fp, fp, c.c_void_p, c.c_int]
    if not dev_lib or hasattr(lib, "nutls_set_hop_fusion"):
        lib.nutls_set_hop_fusion.argtypes = [c.c_void_p, c.c_int]
        lib.nutls_launches_per_hop.argtypes = [c.c_void_p]
    if not dev_lib or hasattr(lib, "nutls_process_block_ragged"):
        ip = c.POINTER(c.c_int)
        lib.nutls_process_block_ragged.argtypes = [c.c_void_p, c.c_void_p, c.c_void_p, c.c_int, c.c_void_p, c.c_void_p]
        lib.nutls_process_block_ragged_host.argtypes = [c.c_void_p, fp, fp, c.c_int, ip]
        lib.nutls_enhance_block_ragged.argtypes = [c.c_void_p, c.c_void_p, c.c_void_p, c.c_int, c.c_void_p, c.c_int, c.c_void_p]
        lib.nutls_enhance_block_ragged_host.argtypes = [c.c_void_p, fp, fp, c.c_int, ip, c.c_int]
        lib.nutls_stft_block_ragged.argtypes = [c.c_void_p, c.c_void_p, c.c_void_p, c.c_int, c.c_void_p, c.c_void_p]
        lib.nutls_istft_block_ragged.argtypes = [c.c_void_p, c.c_void_p, c.c_void_p, c.c_int, c.c_void_p, c.c_int, c.c_void_p]
    if not dev_lib or hasattr(lib, "nutls_conv_dispatch"):
        ip, lp = c.POINTER(c.c_int), c.POINTER(c.c_longlong)
        lib.nutls_launch_conv_shape.argtypes = [c.c_void_p, c.c_int, ip, ip]
        lib.nutls_conv_dispatch.argtypes = [c.c_int, c.c_int, c.c_int, c.c_int, c.c_int, c.c_longlong, ip, ip, ip, lp, lp]
    if not dev_lib or hasattr(lib, "nutls_set_pcm_format"):
        vp = c.c_void_p
        lib.nutls_set_pcm_format.argtypes = [vp, c.c_int, c.c_int]
        lib.nutls_pcm_hop_samples.argtypes = [vp]
        lib.nutls_pcm_delay_samples.argtypes = [vp]
        lib.nutls_pcm_filter_taps.argtypes = [c.c_int]
        lib.nutls_pcm_filter.argtypes = [c.c_int, fp, c.c_int]
        lib.nutls_enhance_hop_pcm.argtypes = [vp, vp, vp, c.c_int, vp]
        lib.nutls_enhance_hop_pcm_active.argtypes = [vp, vp, vp, vp, c.c_int, vp]
        lib.nutls_enhance_hop_pcm_host.argtypes = [vp, vp, vp, c.c_int]
        lib.nutls_enhance_hop_pcm_host_active.argtypes = [vp, vp, vp, vp, c.c_int]
        lib.nutls_pcm_decode_hop.argtypes = [vp, vp, vp, vp, vp]
        lib.nutls_pcm_encode_hop.argtypes = [vp, vp, vp, vp, vp]
        lib.nutls_enhance_block_pcm.argtypes = [vp, vp, vp, c.c_int, c.c_int, vp]
        lib.nutls_enhance_block_pcm_host.argtypes = [vp, vp, vp, c.c_int, c.c_int]
        lib.nutls_pcm_decode_block.argtypes = [vp, vp, vp, c.c_int, vp]
        lib.nutls_pcm_encode_block.argtypes = [vp, vp, vp, c.c_int, vp]
    if not dev_lib or hasattr(lib, "nutls_enhance_block_pcm_ragged"):
        vp = c.c_void_p
        lib.nutls_enhance_block_pcm_ragged.argtypes = [vp, vp, vp, c.c_int, vp, c.c_int, vp]
        lib.nutls_enhance_block_pcm_ragged_host.argtypes = [vp, vp, vp, c.c_int, c.POINTER(c.c_int), c.c_int]
        lib.nutls_pcm_decode_block_ragged.argtypes = [vp, vp, vp, c.c_int, vp, vp]
        lib.nutls_pcm_encode_block_ragged.argtypes = [vp, vp, vp, c.c_int, vp, vp]
    if not dev_lib or hasattr(lib, "nutls_set_pcm_upper_band"):
        lib.nutls_set_pcm_upper_band.argtypes = [c.c_void_p, c.c_float]
        lib.nutls_pcm_upper_band.argtypes = [c.c_void_p, fp]
    if not dev_lib or hasattr(lib, "nutls_set_pcm_upper_follow"):
        lib.nutls_set_pcm_upper_follow.argtypes = [c.c_void_p, c.c_int]
        lib.nutls_pcm_upper_follow.argtypes = [c.c_void_p, c.POINTER(c.c_int)]
        lib.nutls_pcm_follow_gain.argtypes = [c.c_void_p, fp, c.c_int]
    if not dev_lib or hasattr(lib, "nutls_set_atten_limit"):
        lib.nutls_set_atten_limit.argtypes = [c.c_void_p, fp, c.c_int]
        lib.nutls_atten_limit.argtypes = [c.c_void_p, fp, c.c_int]
        lib.nutls_istft_block_mix.argtypes = [c.c_void_p, c.c_void_p, c.c_void_p, c.c_void_p, c.c_int, c.c_void_p, c.c_int, c.c_void_p]
    if not dev_lib or hasattr(lib, "nutls_set_pcm_packet"):
        vp, ip = c.c_void_p, c.POINTER(c.c_int)
        lib.nutls_pcm_packet_plan.argtypes = [c.c_int, c.c_int, c.c_int, ip, ip, ip]
        lib.nutls_set_pcm_packet.argtypes = [vp, c.c_int]
        lib.nutls_pcm_packet_samples.argtypes = [vp]
        lib.nutls_pcm_packet_delay_samples.argtypes = [vp]
        lib.nutls_pcm_packet_fill.argtypes = [vp, ip, c.c_int]
        lib.nutls_pcm_packet_last_rounds.argtypes = [vp]
        lib.nutls_enhance_packet_pcm.argtypes = [vp, vp, vp, vp, c.c_int, vp]
        lib.nutls_enhance_packet_pcm_host.argtypes = [vp, vp, vp, vp, c.c_int]
    if not dev_lib or hasattr(lib, "nutls_set_pcm_channels"):
        lib.nutls_set_pcm_channels.argtypes = [c.c_void_p, c.c_int]
        lib.nutls_pcm_channels.argtypes = [c.c_void_p]
        lib.nutls_pcm_deinterleave.argtypes = [c.c_int, c.c_int, c.c_void_p, c.c_void_p, c.c_size_t]
        lib.nutls_pcm_interleave.argtypes = [c.c_int, c.c_int, c.c_void_p, c.c_void_p, c.c_size_t]
    if not dev_lib or hasattr(lib, "nutls_pcm_g711_expand"):
        lib.nutls_pcm_g711_expand.argtypes = [c.c_int, c.POINTER(c.c_short), c.c_int]
        lib.nutls_pcm_g711_compress.argtypes = [c.c_int, c.POINTER(c.c_short), c.POINTER(c.c_ubyte), c.c_size_t]
    lib.nutls_create_offline.argtypes = [c.c_void_p, c.c_size_t, c.c_int, c.c_int, c.POINTER(c.c_void_p)]
    if not dev_lib or hasattr(lib, "nutls_create_offline_batch"):
        lib.nutls_create_offline_batch.argtypes = [c.c_void_p, c.c_size_t, c.c_int, c.c_int, c.c_int, c.POINTER(c.c_void_p)]
    lib.nutls_process_block.argtypes = [c.c_void_p, c.c_void_p, c.c_void_p, c.c_int, c.c_void_p]
    lib.nutls_process_block_host.argtypes = [c.c_void_p, fp, fp, c.c_int]
    lib.nutls_offline_set_ctfa_mode.argtypes = [c.c_void_p, c.c_int]
    lib.nutls_set_ctfa_mode.argtypes = [c.c_void_p, c.c_int]
    lib.nutls_offline_set_pipeline.argtypes = [c.c_void_p, c.c_int]
    lib.nutls_fused_num_ops.argtypes = [c.c_int]
    lib.nutls_fused_op_info.argtypes = [c.c_int, c.c_int, c.POINTER(c.c_char_p), c.POINTER(c.c_double)]
    lib.nutls_profile_fused.argtypes = [c.c_void_p, c.POINTER(c.c_double), c.c_int]
    if not dev_lib or hasattr(lib, "nutls_profile_production"):
        lib.nutls_profile_production.argtypes = [c.c_void_p, c.POINTER(c.c_double), c.c_int, c.c_int, c.c_int]
    lib.nutls_fused_blob_floats.argtypes = [c.c_int]
    lib.nutls_fused_pack_blob.argtypes = [c.c_void_p, c.c_size_t, c.c_int, fp, c.c_size_t]
    lib.nutls_fused_plan_blob_floats.argtypes = [c.c_int, c.c_int]
    lib.nutls_fused_plan_num_ops.argtypes = [c.c_int, c.c_int]
    lib.nutls_fused_plan_op_info.argtypes = [c.c_int, c.c_int, c.c_int, c.POINTER(c.c_char_p), c.POINTER(c.c_double)]
    lib.nutls_fused_pack_blob_plan.argtypes = [c.c_void_p, c.c_size_t, c.c_int, c.c_int, fp, c.c_size_t]
    lib.nutls_last_error.restype = c.c_char_p
    lib.nutls_version.restype = c.c_char_p
    for name in ABI_SYMBOLS + ABI_SYMBOLS_G711:
        if dev_lib and not hasattr(lib, name):
            continue
        fn = getattr(lib, name)
        if fn.restype is None or fn.restype is c.c_int:
            fn.restype = c.c_int
    if path is None:
        _lib = lib
    return lib


def _check(lib, rc: int):
    if rc == 0:
        return
    msg = lib.nutls_last_error().decode("utf-8", "replace")
    if rc == NUTLS_ERR_ARG:
        raise ValueError(msg)      # what TF-Lite raises for bad names / shapes
    raise RuntimeError("nutls error %d: %s" % (rc, msg))


def _fptr(a: np.ndarray):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_float))


def host_alloc(shape, lib: Optional[ctypes.CDLL] = None) -> np.ndarray:
    """A float32 numpy array in page-locked, device-visible host memory (``nutls_host_alloc``): frames handed to ``NutlsEngine.step``
    / results received in its ``out=`` from such arrays cross the link without the runtime's staging copies, and the fused kernel
    reads / writes them directly.  The memory is released when the array (and every view of it) is gone."""
    import weakref
    lib = lib or load_library()
    n = int(np.prod(shape))
    p = lib.nutls_host_alloc(n * 4)
    if not p:
        raise RuntimeError(lib.nutls_last_error().decode())
    buf = (ctypes.c_float * n).from_address(p)
    arr = np.frombuffer(buf, dtype=np.float32).reshape(shape)
    weakref.finalize(buf, lib.nutls_host_free, p)      # (the array keeps `buf` alive through its base chain)
    arr[...] = 0.0
    return arr


def pcm_filter(rate: int, lib: Optional[ctypes.CDLL] = None) -> np.ndarray:
    """The fp32 prototype filter the PCM gateway's kernels use for ``rate`` (8000, 32000, 48000: ``2 * 24 * q + 1`` taps; 16000: the single
    tap 1.0) -- ``nutls_pcm_filter``.  Host only: needs no GPU."""
    lib = lib or load_library()
    n = lib.nutls_pcm_filter_taps(int(rate))
    if n < 0:
        raise ValueError("rate must be 8000, 16000, 32000 or 48000, got %r" % (rate,))
    taps = np.empty(n, np.float32)
    _check(lib, lib.nutls_pcm_filter(int(rate), _fptr(taps), n))
    return taps


def pcm_packet_plan(rate: int, dtype, samples: int, lib: Optional[ctypes.CDLL] = None) -> dict:
    """What packet mode makes of packets of ``samples`` samples at ``rate`` in ``dtype`` ("float32", "int16", "ulaw", "alaw"):
    ``{"delay": D, "rounds": R, "fifo": S - g + P}`` -- the silence in front of every stream, the hop rounds a tick can take and the samples
    each FIFO can hold (``nutls_pcm_packet_plan``).  Host only: needs no GPU.  ``ValueError``: a rate, format or length that is not accepted
    (the packet's bytes a multiple of 16, 1 .. 4 hops)."""
    name = dtype if isinstance(dtype, str) and dtype in G711_CODECS else np.dtype(dtype).name
    if name not in _PcmFormat._PCM_FORMATS:
        raise ValueError("dtype must be float32, int16, 'ulaw' or 'alaw', got %s" % name)
    lib = lib or load_library()
    d, r, f = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int(0)
    _check(lib, lib.nutls_pcm_packet_plan(int(rate), _PcmFormat._PCM_FORMATS[name], int(samples), ctypes.byref(d), ctypes.byref(r), ctypes.byref(f)))
    return {"delay": d.value, "rounds": r.value, "fifo": f.value}


# G.711 (NUTLS_PCM_ULAW / NUTLS_PCM_ALAW; 8000 Hz only): the codec names, their format codes and the silence code of each -- what a zero
# hop compresses to, and what pads a recording and stands where the other formats have zeros
G711_CODECS = {"ulaw": 2, "alaw": 3}
G711_SILENCE = {"ulaw": 0xFF, "alaw": 0xD5}


def _g711_format(codec) -> int:
    if not isinstance(codec, str) or codec not in G711_CODECS:
        raise ValueError("codec must be 'ulaw' or 'alaw', got %r" % (codec,))
    return G711_CODECS[codec]


def g711_expand(codec: str, lib: Optional[ctypes.CDLL] = None) -> np.ndarray:
    """The int16 value of each of the 256 codes of ``codec`` ("ulaw" or "alaw"), ``[256]`` int16: ``table[c]`` is what the PCM gateway's
    decode makes of byte ``c`` before it scales by 1 / 32768 (``nutls_pcm_g711_expand``).  Host only: needs no GPU."""
    fmt = _g711_format(codec)
    lib = lib or load_library()
    table = np.empty(256, np.int16)
    _check(lib, lib.nutls_pcm_g711_expand(fmt, table.ctypes.data_as(ctypes.POINTER(ctypes.c_short)), 256))
    return table


def g711_compress(codec: str, samples, lib: Optional[ctypes.CDLL] = None) -> np.ndarray:
    """The codes of ``codec`` ("ulaw" or "alaw") for an int16 array of any shape -> uint8 array of that shape: what the PCM gateway's encode
    makes of the int16 value it has quantised a sample to (``nutls_pcm_g711_compress``).  Host only: needs no GPU."""
    fmt = _g711_format(codec)
    x = np.asarray(samples)
    if x.dtype != np.int16:
        raise ValueError("samples must be int16, got %s" % x.dtype.name)
    x = np.ascontiguousarray(x)
    lib = lib or load_library()
    out = np.empty(x.shape, np.uint8)
    _check(lib, lib.nutls_pcm_g711_compress(fmt, x.ctypes.data_as(ctypes.POINTER(ctypes.c_short)), out.ctypes.data_as(ctypes.POINTER(ctypes.c_ubyte)), x.size))
    return out


# Channels (nutls_set_pcm_channels): the sample types of the two host functions and their format codes (one byte is one byte: either law)
_CHANNEL_FORMATS = {"float32": 0, "int16": 1, "uint8": 2}


def _channel_layout(fn_name: str, x, frames_in: bool, lib) -> np.ndarray:
    x = np.asarray(x)
    if x.dtype.name not in _CHANNEL_FORMATS or x.ndim != 2:
        raise ValueError("%s takes a 2-D float32, int16 or uint8 array, got %s %s" % (fn_name, x.dtype.name, x.shape))
    x = np.ascontiguousarray(x)
    n, ch = x.shape if frames_in else x.shape[::-1]
    lib = lib or load_library()
    out = np.empty((ch, n) if frames_in else (n, ch), x.dtype)
    _check(lib, getattr(lib, fn_name)(_CHANNEL_FORMATS[x.dtype.name], int(ch), x.ctypes.data, out.ctypes.data, int(n)))
    return out


def pcm_deinterleave(frames, lib: Optional[ctypes.CDLL] = None) -> np.ndarray:
    """Frames ``[n, C]`` (the layout of ``scipy.io.wavfile`` / ``soundfile``; float32, int16 or uint8, C 2 or 4) -> one row per channel,
    ``[C, n]``: the rule of ``set_pcm_channels``, stated by the library (``nutls_pcm_deinterleave``).  Host only: needs no GPU."""
    return _channel_layout("nutls_pcm_deinterleave", frames, True, lib)


def pcm_interleave(rows, lib: Optional[ctypes.CDLL] = None) -> np.ndarray:
    """One row per channel ``[C, n]`` -> frames ``[n, C]``: the inverse of :func:`pcm_deinterleave` (``nutls_pcm_interleave``)."""
    return _channel_layout("nutls_pcm_interleave", rows, False, lib)


def atten_limit_from_db(db) -> np.float32:
    """The attenuation limit ``l`` of a cap of ``db`` decibels on the noise removed: ``float32(10 ** (-db / 20))``; 0 dB -> 1 (nothing is
    removed), ``None`` -> 0 (no cap: the model's full suppression).  ``ValueError``: a negative or NaN value."""
    if db is None:
        return np.float32(0.0)
    d = float(db)
    if not d >= 0.0:
        raise ValueError("atten_lim_db must be >= 0 dB or None, got %r" % (db,))
    return np.float32(10.0 ** (-d / 20.0))


class _PcmFormat:
    """The callers' sample format of a handle (``nutls_set_pcm_format``) and its attenuation limit (``nutls_set_atten_limit``): shared by
    :class:`NutlsEngine` and :class:`NutlsOffline`."""

    def _rows(self) -> int:
        return getattr(self, "utterances", None) or self.batch

    def set_atten_limit(self, limit=None, db=None) -> None:
        """A cap on how much noise the waveform methods remove, per row (stream of a streaming handle, utterance of an offline one):
        ``limit`` in [0, 1], a scalar for every row or one value per row -- every frame is synthesised from
        ``limit * noisy + (1 - limit) * enhanced`` magnitudes on the frame's phase, so no bin is attenuated below ``limit`` times its input
        (``nutls_set_atten_limit``).  ``db`` instead of ``limit``: the cap in decibels, scalar or per row, entries ``None`` for no cap
        (:func:`atten_limit_from_db`).  Neither: every row back to 0, the model's full suppression, bit for bit as without this call.
        A setting, not stream state: ``reset`` and ``set_pcm_format`` keep it; a change holds from the next call.  Synchronises the device.
        ``ValueError``: a value outside [0, 1] or NaN, a wrong count, a negative ``db``, a value other than 0 while hop fusion is on --
        nothing changes."""
        if limit is not None and db is not None:
            raise ValueError("give limit or db, not both")
        rows = self._rows()
        if db is not None:
            seq = list(db) if isinstance(db, (list, tuple, np.ndarray)) else [db] * rows
            vals = [atten_limit_from_db(d) for d in seq]
        elif limit is not None:
            vals = list(np.asarray(limit, dtype=np.float32).reshape(-1)) if np.ndim(limit) else [np.float32(limit)] * rows
        else:
            _check(self._lib, self._lib.nutls_set_atten_limit(self._h, None, rows))
            return
        a = np.ascontiguousarray(vals, dtype=np.float32)
        _check(self._lib, self._lib.nutls_set_atten_limit(self._h, _fptr(a), len(a)))

    @property
    def atten_limit(self) -> np.ndarray:
        """``[rows]`` float32: the attenuation limit in force for every stream / utterance (``nutls_atten_limit``); all 0 by default."""
        a = np.zeros(self._rows(), np.float32)
        _check(self._lib, self._lib.nutls_atten_limit(self._h, _fptr(a), len(a)))
        return a

    _PCM_FORMATS = {"float32": 0, "int16": 1, "ulaw": 2, "alaw": 3}
    pcm_rate, pcm_dtype, pcm_codec = 16000, "float32", None

    def set_pcm_format(self, rate: int = 16000, dtype="float32") -> None:
        """What the ``_pcm`` methods take and return from now on: ``rate`` 8000, 16000, 32000 or 48000, ``dtype`` "float32" or "int16"
        (32768 = 1.0) -- or, at 8000 only, "ulaw" or "alaw": G.711, one byte per sample, which the ``_pcm`` methods take and return as
        ``uint8`` arrays / ``torch.uint8`` tensors (``pcm_dtype`` is then "uint8" and ``pcm_codec`` the law; held rows and hops behind a
        count come back as the law's silence code, 0xFF / 0xD5, not as zero bytes).  May be called between any two hops; every stream's
        resampler history restarts from zeros and the upper band (``set_pcm_upper_band``) is off again.  The other methods keep taking
        float32 at 16 kHz.  ``ValueError``: another rate or dtype, a G.711 law at a rate other than 8000 -- nothing changes."""
        name = dtype if isinstance(dtype, str) and dtype in G711_CODECS else np.dtype(dtype).name
        if name not in self._PCM_FORMATS:
            raise ValueError("dtype must be float32, int16, 'ulaw' or 'alaw', got %s" % name)
        _check(self._lib, self._lib.nutls_set_pcm_format(self._h, int(rate), self._PCM_FORMATS[name]))
        self.pcm_codec = name if name in G711_CODECS else None
        self.pcm_rate, self.pcm_dtype = int(rate), "uint8" if self.pcm_codec else name

    @property
    def pcm_silence(self) -> int:
        """The sample value of silence in the handle's format: 0, or the silence code of its G.711 law (0xFF / 0xD5)."""
        return G711_SILENCE[self.pcm_codec] if self.pcm_codec else 0

    def set_pcm_upper_band(self, gain: float) -> None:
        """The band above 8 kHz of a 32 or 48 kHz caller, passed around the model and added back at ``gain`` in [0, 1], aligned with the
        enhanced low band (``nutls_set_pcm_upper_band``); 0.0, the default, is off: the ``_pcm`` methods then return audio band-limited to
        8 kHz, bit for bit as without this call.  May be called between any two hops: every stream's resampler history and upper-band state
        restart from zeros (nothing happens when ``gain`` is the value in force).  ``set_pcm_format`` turns it off, so call this after it.
        ``ValueError``: NaN, a gain outside [0, 1], or a gain other than 0 at 8000 / 16000 Hz."""
        _check(self._lib, self._lib.nutls_set_pcm_upper_band(self._h, float(gain)))

    @property
    def pcm_upper_band(self) -> float:
        """The upper band's gain in force (``nutls_pcm_upper_band``); 0.0: off."""
        g = ctypes.c_float(0.0)
        _check(self._lib, self._lib.nutls_pcm_upper_band(self._h, ctypes.byref(g)))
        return float(g.value)

    def set_pcm_upper_follow(self, enable: bool) -> None:
        """The upper band's gain FOLLOWS the model (``nutls_set_pcm_upper_follow``): per hop it is the gain of ``set_pcm_upper_band`` -- now
        the ceiling -- times ``min(1, sqrt(energy of the model's output / energy of its input))`` over the last 4 hops, ramped linearly
        across the hop, so a pause loses its hiss above 8 kHz as it loses its noise below.  May be called between any two hops: a change
        restarts every stream's resampler history, upper-band and follow state from zeros (nothing happens when ``enable`` is the value
        in force).  ``set_pcm_format`` and ``set_pcm_upper_band(0)`` turn it off.  ``ValueError``: enabling while the gain is 0, which
        includes every 8000 / 16000 Hz handle."""
        _check(self._lib, self._lib.nutls_set_pcm_upper_follow(self._h, 1 if enable else 0))

    @property
    def pcm_upper_follow(self) -> bool:
        """Whether the upper band's gain follows the model (``nutls_pcm_upper_follow``)."""
        on = ctypes.c_int(0)
        _check(self._lib, self._lib.nutls_pcm_upper_follow(self._h, ctypes.byref(on)))
        return bool(on.value)

    def pcm_follow_gain(self) -> np.ndarray:
        """``[rows]`` float32 (streams of a streaming handle, utterances of an offline one): the followed gain of each row's last real
        encoded hop, 0.0 after a reset (``nutls_pcm_follow_gain``; synchronises).  ``ValueError`` while follow is off."""
        g = np.zeros(getattr(self, "utterances", None) or self.batch, np.float32)
        _check(self._lib, self._lib.nutls_pcm_follow_gain(self._h, _fptr(g), len(g)))
        return g

    @property
    def pcm_hop_samples(self) -> int:
        """Samples of one 16 ms hop at the callers' rate: 128, 256, 512 or 768."""
        return int(self._lib.nutls_pcm_hop_samples(self._h))

    @property
    def pcm_delay_samples(self) -> int:
        """Delay of the two rate conversions together, in samples at the callers' rate (0 at 16 kHz); the one-hop lag of ``enhance_hop``
        comes on top."""
        return int(self._lib.nutls_pcm_delay_samples(self._h))

    def set_pcm_channels(self, channels: int = 1) -> None:
        """The callers' frame layout of the ``_pcm`` methods (``nutls_set_pcm_channels``): 1, the default, is one row per stream; with 2
        or 4 the callers' buffers are interleaved frames, ``[rows / C, n * C]`` or, the same memory, ``[rows / C, n, C]`` -- channel ``c`` of
        frame row ``r`` is stream ``r * C + c`` -- and the methods return the shape they were given.  Masks, hop counts, limits and the
        16 kHz float sides of the halves stay per stream.  A setting, not stream state: ``reset`` and ``set_pcm_format`` keep it, it may
        change between any two calls and touches no history.  Synchronises the device.  ``ValueError``: a value other than 1, 2, 4, or one
        that does not divide the handle's rows -- nothing changes."""
        if int(channels) == self._pcm_channels:
            return      # (the value in force: a no-op in the library too)
        _check(self._lib, self._lib.nutls_set_pcm_channels(self._h, int(channels)))
        self._pcm_channels = int(channels)

    @property
    def pcm_channels(self) -> int:
        """Channels per frame of the callers' buffers (``nutls_pcm_channels``); 1: one row per stream."""
        return int(self._lib.nutls_pcm_channels(self._h)) if self._pcm_channels > 1 else 1

    _pcm_channels = 1      # what set_pcm_channels last set: the methods' shape checks cost no call into the library

    def _pcm_shapes(self, rows: int, cols: int):
        """The shapes the callers' side ``[rows, cols]`` of a ``_pcm`` method may have in the layout in force (the first: what the methods allocate)."""
        ch = self._pcm_channels
        return ((rows, cols),) if ch == 1 else ((rows // ch, cols * ch), (rows // ch, cols, ch))

    def _pcm_cols(self, x) -> int:
        """Samples per stream of the callers' buffer ``x`` in the layout in force; -1: not a shape of that layout."""
        shape, ch = tuple(getattr(x, "shape", ())), self._pcm_channels
        if ch > 1 and len(shape) == 3 and shape[2] == ch:
            return int(shape[1])
        return int(shape[1]) // ch if len(shape) == 2 and shape[1] % ch == 0 else -1

    def _pcm_tensor(self, x, rows: int, cols: int, name: str, dtype=None):
        """A contiguous CUDA tensor ``[rows, cols]`` of the handle's sample type (or ``dtype``: a 16 kHz float side, one row per stream
        whatever the layout); with channels, ``[rows / C, cols * C]`` or ``[rows / C, cols, C]``."""
        import torch
        want = dtype or getattr(torch, self.pcm_dtype)
        shapes = ((rows, cols),) if dtype is not None else self._pcm_shapes(rows, cols)
        if not (torch.is_tensor(x) and x.is_cuda and x.dtype == want and x.is_contiguous() and tuple(x.shape) in shapes):
            raise ValueError("%s must be a contiguous %s CUDA tensor %s" % (name, str(want).replace("torch.", ""), self._shapes_text(shapes)))
        return x

    def _pcm_array(self, x, rows: int, cols: int, name: str):
        shapes = self._pcm_shapes(rows, cols)
        if not (isinstance(x, np.ndarray) and x.dtype.name == self.pcm_dtype and x.flags.c_contiguous and x.shape in shapes):
            raise ValueError("%s must be a contiguous %s numpy array %s" % (name, self.pcm_dtype, self._shapes_text(shapes)))
        return x

    @staticmethod
    def _shapes_text(shapes) -> str:
        return " or ".join("[%s]" % ",".join("%d" % d for d in s) for s in shapes)


# the kinds of the per-layer conv kernels, in the library's order (csrc/nutls_internal.hpp ConvKind)
CONV_KINDS = ("el_c32", "el_c64", "el_c128", "dl_n64", "dl_n128", "in_c64", "in_c128", "down", "up_even", "up_odd")


def conv_dispatch(kind, batch: int, f_out: int, bf16: bool = True, ksplit: bool = True, tile_min: Optional[int] = None) -> Dict[str, int]:
    """Which instantiation of the per-layer conv kernels a launch runs and its launch shape (``nutls_conv_dispatch``: the function the
    library's launches dispatch on; no GPU needed).  ``kind``: a name of ``CONV_KINDS`` or its index; ``batch``: streams of the launch
    (block mode: utterances x frames); ``bf16``: the bf16-pipe kernel of the block mode, else the fp32-MFMA kernel; ``ksplit`` /
    ``tile_min``: the developer knobs ``NUTLS_OFFLINE_KSPLIT`` and ``NUTLS_CONV_TILE_MIN`` (None: the defaults) a handle would be created
    under.  Returns ``{"nw", "all", "tile", "grid", "lds"}``: template arguments NW and ALL, positions per workgroup, workgroups, LDS bytes."""
    lib = load_library()
    k = CONV_KINDS.index(kind) if isinstance(kind, str) else int(kind)
    nw, al, tile, grid, lds = ctypes.c_int(), ctypes.c_int(), ctypes.c_int(), ctypes.c_longlong(), ctypes.c_longlong()
    _check(lib, lib.nutls_conv_dispatch(k, int(batch), int(f_out), 1 if bf16 else 0, 1 if ksplit else 0, -1 if tile_min is None else int(tile_min),
                                        ctypes.byref(nw), ctypes.byref(al), ctypes.byref(tile), ctypes.byref(grid), ctypes.byref(lds)))
    return {"nw": nw.value, "all": al.value, "tile": tile.value, "grid": grid.value, "lds": lds.value}


def conv_launches(lib, handle) -> List[Tuple[str, str, int]]:
    """The conv launches of a handle's per-layer plan (``nutls_launch_conv_shape``): (layer name, kind name, f_out) in issue order."""
    res = []
    for i in range(lib.nutls_launches_per_step(handle)):
        layer, kind, f_out = ctypes.c_char_p(), ctypes.c_int(), ctypes.c_int()
        _check(lib, lib.nutls_launch_info(handle, i, ctypes.byref(layer), None, None, None))
        _check(lib, lib.nutls_launch_conv_shape(handle, i, ctypes.byref(kind), ctypes.byref(f_out)))
        if kind.value >= 0:
            res.append((layer.value.decode(), CONV_KINDS[kind.value], f_out.value))
    return res


class NutlsEngine(_PcmFormat):
    """B streams, device-resident state.  ``step`` takes/returns ``[B,256]`` magnitudes."""

    MODES = {"launches": 0, "graph": 1, "fused": 3}
    VARIANTS = {"lstm": 0, "baseline": 1}

    def __init__(self, weights=None, batch: int = 1, device: int = 0, mode: Optional[str] = None, variant: str = "lstm",
                 streams_per_workgroup: Optional[int] = None, hop_fusion: Optional[bool] = None):
        """``mode``: "fused" (the default when the container holds int8 conv kernels, as the reference's .tflite does:
        one launch per frame, one workgroup per one / two / four streams, every op its own specialised instruction stream),
        "graph" (one kernel per layer, hipGraph replay; the default for float containers) or "launches" (one kernel per layer).
        ``variant``: "lstm" (NUNet-TLS-LSTM, trained weights ship in weights/) or "baseline"
        (dilated-dense bottleneck; no trained weights exist -- pass a container, e.g.
        ``weights.write_blob(weights.synthetic_weights("baseline"), int8_convs=True)``).
        ``streams_per_workgroup``: which plan the fused kernel runs -- None: the library's choice (a packed plan, two or four streams
        per workgroup, where its cost model finds one faster: more streams than CUs), 1 / 2 / 4: that plan (``nutls_create_plan``; a batch
        that is not a multiple, or a variant without such a plan, raises).
        ``hop_fusion``: True / False: ``set_hop_fusion`` once the mode is set (``enhance_hop`` as ONE launch instead of three; raises where the
        handle has no hop build); None (default): the handle stays as the library created it -- off, or on under ``NUTLS_HOP_FUSION=1``."""
        self._lib = load_library()
        if variant not in self.VARIANTS:
            raise ValueError("variant must be one of %s" % sorted(self.VARIANTS))
        if weights is None and variant != "lstm":
            raise ValueError("the %s variant has no shipped weights: pass a .nutlsw container" % variant)
        self.variant = variant
        blob = read_blob(weights if weights is not None else DEFAULT_WEIGHTS)
        self._h = ctypes.c_void_p()
        buf = ctypes.create_string_buffer(blob, len(blob))
        _check(self._lib, self._lib.nutls_create_plan(buf, len(blob), self.VARIANTS[variant], int(batch), int(device),
                                                      int(streams_per_workgroup or 0), ctypes.byref(self._h)))
        self._blob = blob          # (kept for weight_blob_bytes() of the per-layer modes: parsed there, on demand)
        self._fp32_weight_bytes = None
        self.batch = int(batch)
        self.device = int(device)
        pin, pout = ctypes.c_void_p(), ctypes.c_void_p()
        _check(self._lib, self._lib.nutls_io_buffers(self._h, ctypes.byref(pin), ctypes.byref(pout)))
        self.io_in_ptr, self.io_out_ptr = pin.value, pout.value
        if mode is not None:
            self.set_mode(mode)
        else:       # fused when the container holds int8 conv kernels, else the per-layer kernels replayed as a hipGraph
            try:
                self.set_mode("fused")
            except ValueError:
                self.set_mode("graph")
        if hop_fusion is not None:
            self.set_hop_fusion(hop_fusion)

    # -- lifetime --------------------------------------------------------------------------
    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            self._lib.nutls_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    CTFA_MODES = {"frame": 0, "causal32": 1}

    def set_ctfa_mode(self, ctfa_mode: str):
        """"frame" (default): the frame-wise graph's CTFA, whose frequency branch sees TA/32; "causal32": the offline /
        training model's 32-frame causal mean of the time attention (models/proposed.py:143-147), history kept per stream inside
        the library -- fused mode only."""
        if ctfa_mode not in self.CTFA_MODES:
            raise ValueError("ctfa_mode must be one of %s" % sorted(self.CTFA_MODES))
        _check(self._lib, self._lib.nutls_set_ctfa_mode(self._h, self.CTFA_MODES[ctfa_mode]))
        self.ctfa_mode = ctfa_mode

    def set_mode(self, mode: str):
        if mode not in self.MODES:
            raise ValueError("mode must be one of %s" % sorted(self.MODES))
        _check(self._lib, self._lib.nutls_set_mode(self._h, self.MODES[mode]))
        self.mode = mode

    @property
    def streams_per_workgroup(self) -> int:
        """Streams one workgroup of the fused kernel steps: 1, or 2 / 4 (packed plans, chosen for handles with more streams than CUs)."""
        return int(self._lib.nutls_streams_per_workgroup(self._h))

    @property
    def launches_per_step(self) -> int:
        return self._lib.nutls_launches_per_step(self._h)

    def set_hop_fusion(self, enable: bool = True) -> None:
        """``enhance_hop`` as ONE launch: STFT analysis and inverse STFT / overlap-add run inside the fused step kernel (its hop build) instead
        of in a launch each in front of and behind it (``nutls_set_hop_fusion``).  Same per-stream state and buffers: it may be switched
        between any two hops.  LSTM variant, fused mode, one- or two-stream plan; raises ValueError elsewhere, and while it is on
        ``set_mode("graph" / "launches")``, ``debug_trace()`` and the profiling calls raise instead of quietly going back to three launches."""
        _check(self._lib, self._lib.nutls_set_hop_fusion(self._h, 1 if enable else 0))

    @property
    def launches_per_hop(self) -> int:
        """Launches one ``enhance_hop`` issues: 3 (analysis, step, synthesis), or 1 with hop fusion on."""
        return int(self._lib.nutls_launches_per_hop(self._h))

    # -- the hot path ----------------------------------------------------------------------
    def _host_mask(self, active) -> np.ndarray:
        """``active`` of a numpy call: a length-B bool / uint8 array -> contiguous uint8 (checked before the library is called)."""
        if not (isinstance(active, np.ndarray) and active.dtype in (np.bool_, np.uint8)):
            raise ValueError("active must be a bool / uint8 numpy array of length %d when the frames are a numpy array" % self.batch)
        if active.shape != (self.batch,):
            raise ValueError("active must have length %d (one flag per stream), got shape %s" % (self.batch, active.shape))
        return np.ascontiguousarray(active).view(np.uint8)

    def _device_mask(self, active, like):
        """``active`` of a tensor call: a length-B bool / uint8 CUDA tensor on the frames' device (read by the kernels: it must stay
        unmodified until the queued work has run)."""
        import torch
        if not (torch.is_tensor(active) and active.is_cuda and active.dtype in (torch.bool, torch.uint8) and active.is_contiguous()):
            raise ValueError("active must be a contiguous bool / uint8 CUDA tensor of length %d when the frames are a CUDA tensor" % self.batch)
        if tuple(active.shape) != (self.batch,):
            raise ValueError("active must have length %d (one flag per stream), got shape %s" % (self.batch, tuple(active.shape)))
        if active.device != like.device:
            raise ValueError("active lives on %s, the frames on %s" % (active.device, like.device))
        return active.data_ptr()

    def step(self, mag, out=None, active=None):
        """One frame for all B streams.  ``mag``: ``[B,256]`` float32, either a torch tensor on
        this engine's GPU (zero-copy, asynchronous on the current torch stream; ``out`` may be
        a preallocated tensor) or a numpy array (H2D + step + D2H, synchronous; ``out`` may be a preallocated
        array -- with arrays from ``host_alloc`` for both there are no copies, the kernel works on them over the link).
        ``active`` (length-B bool / uint8: a numpy array with numpy frames, a CUDA tensor with tensor frames): only the streams whose
        flag is nonzero take the frame, the others are HELD -- their state stays exactly as it was, their rows of ``mag`` are not used
        and their output rows are zero (``nutls_step_active``: fused mode, LSTM variant, frame-mode CTFA; anything else raises
        ``ValueError``).  A stream's results depend on the frames it took, not on the ticks it took them at."""
        if isinstance(mag, np.ndarray):
            m = np.ascontiguousarray(mag, dtype=np.float32)
            if m.shape != (self.batch, T.N_BINS):
                raise ValueError("mag must be [%d,%d], got %s" % (self.batch, T.N_BINS, m.shape))
            if out is None:
                o = np.empty_like(m)
            else:
                o = out
                if not (isinstance(o, np.ndarray) and o.dtype == np.float32 and o.flags.c_contiguous and o.shape == m.shape):
                    raise ValueError("out must be a contiguous float32 numpy array of mag's shape")
            if active is not None:
                a = self._host_mask(active)
                _check(self._lib, self._lib.nutls_step_host_active(self._h, _fptr(m), _fptr(o), a.ctypes.data))
                return o
            _check(self._lib, self._lib.nutls_step_host(self._h, _fptr(m), _fptr(o)))
            return o
        import torch
        if not (torch.is_tensor(mag) and mag.is_cuda and mag.dtype == torch.float32 and mag.is_contiguous()):
            raise ValueError("mag must be a contiguous float32 CUDA tensor or a numpy array")
        if tuple(mag.shape) != (self.batch, T.N_BINS):
            raise ValueError("mag must be [%d,%d], got %s" % (self.batch, T.N_BINS, tuple(mag.shape)))
        if out is None:
            out = torch.empty_like(mag)
        if mag.device.index != self.device or out.device != mag.device:
            raise ValueError("mag / out live on %s / %s, this engine on cuda:%d" % (mag.device, out.device, self.device))
        stream = torch.cuda.current_stream(mag.device).cuda_stream
        if active is not None:
            _check(self._lib, self._lib.nutls_step_active(self._h, mag.data_ptr(), out.data_ptr(), self._device_mask(active, mag), stream))
            return out
        _check(self._lib, self._lib.nutls_step(self._h, mag.data_ptr(), out.data_ptr(), stream))
        return out

    # -- STFT front end / inverse-STFT back end on the device ----------------
    _DC = {"edge": 0, "zero": 1}

    def enhance_hop(self, pcm, dc_mode: str = "edge", out=None, active=None):
        """One hop (256 samples) of every stream: analysis -> model step -> synthesis, all on the
        GPU (``interpreter_proposed.py:203-213, 352-365``).  ``pcm``: ``[B,256]`` float32 numpy array
        (synchronous) or CUDA tensor (asynchronous on the current torch stream).  The output lags the
        input by one hop, exactly like the reference loop.  ``active``: as in ``step`` -- a held stream's previous hop, overlap tail
        and model state stay as they are, its hop of the output is zero (``nutls_enhance_hop_active``)."""
        if dc_mode not in self._DC:
            raise ValueError("dc_mode must be 'edge' or 'zero'")
        if isinstance(pcm, np.ndarray):
            x = np.ascontiguousarray(pcm, dtype=np.float32)
            if x.shape != (self.batch, 256):
                raise ValueError("pcm must be [%d,256], got %s" % (self.batch, x.shape))
            if out is None:
                o = np.empty_like(x)
            else:       # (arrays from ``host_alloc`` for both ``pcm`` and ``out``: with hop fusion on the kernel works on them over the link, no copies)
                o = out
                if not (isinstance(o, np.ndarray) and o.dtype == np.float32 and o.flags.c_contiguous and o.shape == x.shape):
                    raise ValueError("out must be a contiguous float32 numpy array of pcm's shape")
            if active is not None:
                a = self._host_mask(active)
                _check(self._lib, self._lib.nutls_enhance_hop_host_active(self._h, _fptr(x), _fptr(o), a.ctypes.data, self._DC[dc_mode]))
                return o
            _check(self._lib, self._lib.nutls_enhance_hop_host(self._h, _fptr(x), _fptr(o), self._DC[dc_mode]))
            return o
        import torch
        if not (torch.is_tensor(pcm) and pcm.is_cuda and pcm.dtype == torch.float32 and pcm.is_contiguous()):
            raise ValueError("pcm must be a contiguous float32 CUDA tensor or a numpy array")
        if tuple(pcm.shape) != (self.batch, 256):
            raise ValueError("pcm must be [%d,256], got %s" % (self.batch, tuple(pcm.shape)))
        if out is None:
            out = torch.empty_like(pcm)
        stream = torch.cuda.current_stream(pcm.device).cuda_stream
        if active is not None:
            _check(self._lib, self._lib.nutls_enhance_hop_active(self._h, pcm.data_ptr(), out.data_ptr(), self._device_mask(active, pcm),
                                                                 self._DC[dc_mode], stream))
            return out
        _check(self._lib, self._lib.nutls_enhance_hop(self._h, pcm.data_ptr(), out.data_ptr(), self._DC[dc_mode], stream))
        return out

    def stft_hop(self, pcm):
        """Analysis half only: CUDA tensor ``[B,256]`` -> the library's ``mag_in`` buffer (phase kept inside)."""
        import torch
        stream = torch.cuda.current_stream(pcm.device).cuda_stream
        _check(self._lib, self._lib.nutls_stft_hop(self._h, pcm.data_ptr(), stream))

    def istft_hop(self, out, dc_mode: str = "edge"):
        """Synthesis half only: the library's ``mag_out`` buffer (+ the phase of the last ``stft_hop``) ->
        CUDA tensor ``out [B,256]``."""
        import torch
        stream = torch.cuda.current_stream(out.device).cuda_stream
        _check(self._lib, self._lib.nutls_istft_hop(self._h, out.data_ptr(), self._DC[dc_mode], stream))
        return out

    # -- PCM gateway: the callers' sample rate and type, converted on the device (csrc/pcm.hip) ---------------------------------
    def enhance_hop_pcm(self, pcm, dc_mode: str = "edge", out=None, active=None):
        """``enhance_hop`` in the format of ``set_pcm_format``: ``pcm [B, pcm_hop_samples]`` of the handle's sample type, a CUDA tensor
        (``nutls_enhance_hop_pcm``, asynchronous on the current torch stream) or a numpy array (``nutls_enhance_hop_pcm_host``, synchronous)
        -> the enhanced hop in the same format, ``pcm_delay_samples`` plus one hop late.  ``active``: as in ``enhance_hop`` -- a held
        stream's resampler history stays as it is too.  At 16000 / float32 this IS ``enhance_hop``."""
        if dc_mode not in self._DC:
            raise ValueError("dc_mode must be 'edge' or 'zero'")
        S = self.pcm_hop_samples
        if isinstance(pcm, np.ndarray):
            x = self._pcm_array(pcm, self.batch, S, "pcm")
            o = np.empty_like(x) if out is None else self._pcm_array(out, self.batch, S, "out")
            if active is not None:
                a = self._host_mask(active)
                _check(self._lib, self._lib.nutls_enhance_hop_pcm_host_active(self._h, x.ctypes.data, o.ctypes.data, a.ctypes.data, self._DC[dc_mode]))
            else:
                _check(self._lib, self._lib.nutls_enhance_hop_pcm_host(self._h, x.ctypes.data, o.ctypes.data, self._DC[dc_mode]))
            return o
        import torch
        x = self._pcm_tensor(pcm, self.batch, S, "pcm")
        o = torch.empty_like(x) if out is None else self._pcm_tensor(out, self.batch, S, "out")
        stream = torch.cuda.current_stream(x.device).cuda_stream
        if active is not None:
            _check(self._lib, self._lib.nutls_enhance_hop_pcm_active(self._h, x.data_ptr(), o.data_ptr(), self._device_mask(active, x),
                                                                     self._DC[dc_mode], stream))
        else:
            _check(self._lib, self._lib.nutls_enhance_hop_pcm(self._h, x.data_ptr(), o.data_ptr(), self._DC[dc_mode], stream))
        return o

    def pcm_decode_hop(self, pcm, out=None, active=None):
        """The decode half on its own: CUDA tensor ``[B, pcm_hop_samples]`` of the handle's sample type -> ``[B,256]`` float32 at 16 kHz
        (what ``enhance_hop`` takes).  ``active``: device mask; a held row of the result is zeros."""
        import torch
        x = self._pcm_tensor(pcm, self.batch, self.pcm_hop_samples, "pcm")
        o = torch.empty((self.batch, 256), dtype=torch.float32, device=x.device) if out is None else self._pcm_tensor(out, self.batch, 256, "out", torch.float32)
        a = None if active is None else self._device_mask(active, x)
        _check(self._lib, self._lib.nutls_pcm_decode_hop(self._h, x.data_ptr(), o.data_ptr(), a, torch.cuda.current_stream(x.device).cuda_stream))
        return o

    def pcm_encode_hop(self, hop, out=None, active=None):
        """The encode half on its own: ``[B,256]`` float32 CUDA tensor at 16 kHz -> ``[B, pcm_hop_samples]`` of the handle's sample type."""
        import torch
        x = self._pcm_tensor(hop, self.batch, 256, "hop", torch.float32)
        S = self.pcm_hop_samples
        o = torch.empty(self._pcm_shapes(self.batch, S)[0], dtype=getattr(torch, self.pcm_dtype), device=x.device) if out is None else self._pcm_tensor(out, self.batch, S, "out")
        a = None if active is None else self._device_mask(active, x)
        _check(self._lib, self._lib.nutls_pcm_encode_hop(self._h, x.data_ptr(), o.data_ptr(), a, torch.cuda.current_stream(x.device).cuda_stream))
        return o

    # -- packet mode: the callers' 10 / 20 ms packets re-framed into hops on the device (csrc/packet.hip) -------------------------
    def set_pcm_packet(self, samples=None, ms=None) -> None:
        """The callers' packet length for ``enhance_packet_pcm``: ``samples`` at the callers' rate, or ``ms`` milliseconds (``ms=20`` ->
        ``pcm_rate * 20 / 1000``, which must be a whole number); ``samples=0``, or neither, turns packet mode off
        (``nutls_set_pcm_packet``).  May be called between any two ticks: every stream's FIFOs start anew -- input empty, output
        ``pcm_packet_delay_samples`` samples of silence --, model state and resampler histories stay (nothing happens when the length is
        the one in force).  ``set_pcm_format`` turns packet mode off, so call this after it.  ``ValueError``: a length whose bytes are no
        multiple of 16 or that is outside 1 .. 4 hops, or a handle that cannot hold streams (see ``step``'s ``active``) with a length
        that is no multiple of the hop -- nothing changes."""
        if samples is not None and ms is not None:
            raise ValueError("give samples or ms, not both")
        if ms is not None:
            n = self.pcm_rate * ms / 1000.0
            if n != int(n):
                raise ValueError("%r ms are not a whole number of samples at %d Hz" % (ms, self.pcm_rate))
            samples = int(n)
        _check(self._lib, self._lib.nutls_set_pcm_packet(self._h, int(samples or 0)))

    @property
    def pcm_packet_samples(self) -> int:
        """Samples of a packet (``nutls_pcm_packet_samples``); 0: packet mode is off."""
        return int(self._lib.nutls_pcm_packet_samples(self._h))

    @property
    def pcm_packet_delay_samples(self) -> int:
        """``D = S - gcd(P, S)``: the samples of silence in front of every stream's packets; ``pcm_delay_samples`` and the one hop of
        ``enhance_hop`` come on top (``nutls_pcm_packet_delay_samples``)."""
        return int(self._lib.nutls_pcm_packet_delay_samples(self._h))

    @property
    def pcm_packet_last_rounds(self) -> int:
        """Hop rounds the last ``enhance_packet_pcm`` call issued (``nutls_pcm_packet_last_rounds``)."""
        return int(self._lib.nutls_pcm_packet_last_rounds(self._h))

    def pcm_packet_fill(self) -> np.ndarray:
        """``[B]`` int32: the samples waiting in each stream's input FIFO, read from the device (``nutls_pcm_packet_fill``; synchronises).
        ``ValueError`` while packet mode is off."""
        f = np.zeros(self.batch, np.int32)
        _check(self._lib, self._lib.nutls_pcm_packet_fill(self._h, f.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), len(f)))
        return f

    def enhance_packet_pcm(self, pcm, dc_mode: str = "edge", out=None, active=None):
        """One packet of every stream in, one packet out (``set_pcm_packet``): ``pcm [B, pcm_packet_samples]`` of the handle's sample type
        (``uint8`` in a G.711 format), a CUDA tensor (``nutls_enhance_packet_pcm``, asynchronous on the current torch stream) or a numpy
        array (``nutls_enhance_packet_pcm_host``, synchronous).  The concatenated packets of a stream are ``pcm_packet_delay_samples`` of
        silence, then what ``enhance_hop_pcm`` returns for the stream's concatenated input cut into hops, bit for bit.  ``active``: as in
        ``enhance_hop_pcm`` -- a held stream's FIFOs stay as they are too, its packet of the output is silence."""
        if dc_mode not in self._DC:
            raise ValueError("dc_mode must be 'edge' or 'zero'")
        P = self.pcm_packet_samples
        if P == 0:
            raise ValueError("packet mode is off (set_pcm_packet)")
        if isinstance(pcm, np.ndarray):
            x = self._pcm_array(pcm, self.batch, P, "pcm")
            o = np.empty_like(x) if out is None else self._pcm_array(out, self.batch, P, "out")
            a = None if active is None else self._host_mask(active)
            _check(self._lib, self._lib.nutls_enhance_packet_pcm_host(self._h, x.ctypes.data, o.ctypes.data, None if a is None else a.ctypes.data,
                                                                      self._DC[dc_mode]))
            return o
        import torch
        x = self._pcm_tensor(pcm, self.batch, P, "pcm")
        o = torch.empty_like(x) if out is None else self._pcm_tensor(out, self.batch, P, "out")
        a = None if active is None else self._device_mask(active, x)
        _check(self._lib, self._lib.nutls_enhance_packet_pcm(self._h, x.data_ptr(), o.data_ptr(), a, self._DC[dc_mode],
                                                            torch.cuda.current_stream(x.device).cuda_stream))
        return o

    def step_resident(self, stream: int = 0):
        """Step on the library-owned I/O buffers (``io_in_ptr`` / ``io_out_ptr``): no copies."""
        _check(self._lib, self._lib.nutls_step(self._h, self.io_in_ptr, self.io_out_ptr, stream))

    # -- state -----------------------------------------------------------------------------
    def state_specs(self) -> List[Tuple[str, Tuple[int, int]]]:
        n = self._lib.nutls_state_count(self._h)
        res = []
        for i in range(n):
            name, d0, d1 = ctypes.c_char_p(), ctypes.c_int(), ctypes.c_int()
            _check(self._lib, self._lib.nutls_state_info(self._h, i, ctypes.byref(name), ctypes.byref(d0), ctypes.byref(d1)))
            res.append((name.value.decode(), (d0.value, d1.value)))
        return res

    def _state_shape(self, name: str):
        if not hasattr(self, "_shapes"):
            self._shapes = {}
            for n, (d0, d1) in self.state_specs():
                self._shapes[n] = (d0, d1)
                self._shapes[n.replace("_prev", "_cur")] = (d0, d1)
        if name not in self._shapes:
            raise ValueError("unknown state tensor: %s" % name)
        return self._shapes[name]

    def state_get(self, name: str) -> np.ndarray:
        d0, d1 = self._state_shape(name)
        a = np.empty((self.batch, d0, d1), np.float32)
        _check(self._lib, self._lib.nutls_state_get(self._h, name.encode(), _fptr(a), a.size))
        return a.reshape(self.batch, d0) if d1 == 1 and d0 == T.LSTM_UNITS else a

    def state_get_all(self, stream_idx: int = 0) -> np.ndarray:
        """Every state tensor of one stream, concatenated in ``state_specs()`` order: ONE device-to-host copy."""
        if not hasattr(self, "_state_total"):
            self._state_total = sum(d0 * d1 for _, (d0, d1) in self.state_specs())
        a = np.empty(self._state_total, np.float32)
        _check(self._lib, self._lib.nutls_state_get_all(self._h, int(stream_idx), _fptr(a), a.size))
        return a

    def state_set(self, name: str, value) -> None:
        d0, d1 = self._state_shape(name)
        a = np.ascontiguousarray(value, dtype=np.float32)
        if a.size != self.batch * d0 * d1:
            raise ValueError("size mismatch for %s: expected %d floats, got %d" % (name, self.batch * d0 * d1, a.size))
        _check(self._lib, self._lib.nutls_state_set(self._h, name.encode(), _fptr(a), a.size))

    def reset(self, stream_idx: int = -1) -> None:
        _check(self._lib, self._lib.nutls_reset(self._h, int(stream_idx)))

    def debug_knob(self, name: str, value: int) -> None:
        """Developer knobs of the handle (include/nutls.h nutls_debug_knob): "skew"."""
        _check(self._lib, self._lib.nutls_debug_knob(self._h, name.encode(), int(value)))

    def debug_trace(self, enable: bool = True) -> None:
        """Fused mode: run every step on the profiling build of the step kernel, which also copies the tensors the kernel keeps in LDS
        ("<stage>.y", "<stage>.up", "input_layer") to a trace buffer that ``debug_get`` reads (one-stream plan, <= 64 streams)."""
        _check(self._lib, self._lib.nutls_debug_trace(self._h, 1 if enable else 0))

    def debug_get(self, name: str, per_stream_shape) -> np.ndarray:
        a = np.empty((self.batch,) + tuple(per_stream_shape), np.float32)
        _check(self._lib, self._lib.nutls_debug_get(self._h, name.encode(), _fptr(a), a.size))
        return a

    def launch_plan(self) -> List[Dict[str, object]]:
        """The per-frame launch list: layer name, kernel family, algorithmic flops / bytes."""
        res = []
        for i in range(self.launches_per_step):
            layer, fam = ctypes.c_char_p(), ctypes.c_char_p()
            fl, by = ctypes.c_double(), ctypes.c_double()
            _check(self._lib, self._lib.nutls_launch_info(self._h, i, ctypes.byref(layer), ctypes.byref(fam),
                                                          ctypes.byref(fl), ctypes.byref(by)))
            res.append({"layer": layer.value.decode(), "family": fam.value.decode(), "flops": fl.value, "bytes": by.value})
        return res

    def conv_launches(self) -> List[Tuple[str, str, int]]:
        """The conv launches of the per-layer plan: (layer name, kind of ``CONV_KINDS``, f_out) in issue order."""
        return conv_launches(self._lib, self._h)

    def fused_plan(self) -> List[Dict[str, object]]:
        """The fused kernel's static schedule: op name and algorithmic flops per stream."""
        res = []
        v, spw = self.VARIANTS[self.variant], self.streams_per_workgroup
        for i in range(self._lib.nutls_fused_plan_num_ops(v, spw)):
            name, fl = ctypes.c_char_p(), ctypes.c_double()
            _check(self._lib, self._lib.nutls_fused_plan_op_info(v, spw, i, ctypes.byref(name), ctypes.byref(fl)))
            res.append({"layer": name.value.decode(), "flops": fl.value})
        return res

    def weight_blob_bytes(self) -> int:
        """Bytes of weights one launch reads: the fused kernel's packed blob (conv kernels int8), else the fp32 tensors."""
        if self.mode == "fused":
            return 4 * int(self._lib.nutls_fused_plan_blob_floats(self.VARIANTS[self.variant], self.streams_per_workgroup))
        if self._fp32_weight_bytes is None:      # fp32 bytes of the container's tensors: what the modes that de-quantise on load keep on the device
            self._fp32_weight_bytes = 4 * sum(int(np.asarray(a).size) for a in parse_blob(self._blob).values())
        return self._fp32_weight_bytes      # (lstm: 11 460 668 B = SURVEY.md section 8(d)'s fp32 weights of the graph)

    def profile_fused(self) -> np.ndarray:
        """One fused-mode step with workgroup 0 time-stamping every op boundary; microseconds per op."""
        us = np.zeros(self._lib.nutls_fused_plan_num_ops(self.VARIANTS[self.variant], self.streams_per_workgroup), np.float64)
        _check(self._lib, self._lib.nutls_profile_fused(
            self._h, us.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), us.size))
        return us

    def profile_production(self, reps: int = 3, steps: int = 60) -> np.ndarray:
        """Per-op microseconds of the UN-instrumented step kernel (``nutls_profile_production``: launches of the library's stop twin that end
        in front of op N, differenced; one-stream plan of the LSTM variant).  Returns ``[n_ops + 1]``: element 0 is the launch floor, element
        ``i + 1`` what op ``i`` of ``fused_plan()`` adds.  Timing only -- every stream is reset afterwards."""
        n = self._lib.nutls_fused_plan_num_ops(self.VARIANTS[self.variant], 1) + 1
        cum = np.zeros(n, np.float64)
        _check(self._lib, self._lib.nutls_profile_production(self._h, cum.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), n, reps, steps))
        return np.concatenate([cum[:1], np.diff(cum)])

    def profile_step(self) -> np.ndarray:
        """One step with every launch bracketed by HIP events on the library's stream; returns
        milliseconds per launch (input: whatever the library's mag_in buffer holds)."""
        ms = np.zeros(self.launches_per_step, np.float32)
        _check(self._lib, self._lib.nutls_profile_step(self._h, _fptr(ms), ms.size))
        return ms


class NutlsRunner:
    """``runner(input=..., msfe6_ee_prev1=..., ..., msfe6_de_c=...) -> dict`` exactly like the
    reference's ``nutls_lstm_sm`` signature runner (interpreter_proposed.py:215-350), batch 1.

    The caller owns the state arrays, as in the reference, and gets fresh WRITABLE arrays back every
    frame (TF-Lite's signature runner does the same).  When it echoes back the very arrays this
    runner returned last frame, unchanged (what the reference loop does), the upload is skipped
    because the device already holds them: "unchanged" is checked against a private snapshot of
    what was handed out, so an in-place edit (zero h / c to reset a stream, ...) is noticed and
    uploaded like any foreign array."""

    signature_key = "nutls_lstm_sm"

    def __init__(self, weights=None, device: int = 0, mode: Optional[str] = None, variant: str = "lstm"):
        """``variant="baseline"`` mirrors the 'nutls' signature of converter_nunet_tls.py:1542 (208 states;
        interpreter_nunet_tls.py:549) -- weights must be supplied, none are shipped."""
        self.engine = NutlsEngine(weights, batch=1, device=device, mode=mode, variant=variant)
        self.signature_key = "nutls_lstm_sm" if variant == "lstm" else "nutls"
        self._in_names = T.input_names(variant)
        self._specs = T.state_specs(variant)
        self._last: Dict[str, np.ndarray] = {}
        self._snap: Dict[str, np.ndarray] = {}       # what the device holds, per output name (private, never handed out)

    @staticmethod
    def _io_shape(shp):
        """per-stream spec -> signature tensor shape: conv states (1,F,C) -> [1,1,F,C]; dilated-dense
        history (d,F,C) -> [1,d,F,C]; LSTM states (21,) -> [1,21]"""
        return (1, shp[0]) if len(shp) == 1 else (1,) + tuple(shp)

    def get_input_details(self) -> Dict[str, Tuple[int, ...]]:
        d = {"input": (1, 1, T.N_BINS, 1)}
        for base, shp in self._specs:
            d[base.format("prev")] = (1, shp[0]) if len(shp) == 1 else self._io_shape(shp)
        return d

    def __call__(self, **feeds) -> Dict[str, np.ndarray]:
        names = set(self._in_names)
        given = set(feeds)
        if given != names:
            raise ValueError("Invalid input names: unknown=%s missing=%s" % (sorted(given - names), sorted(names - given)))
        x = np.asarray(feeds["input"])
        if x.shape != (1, 1, T.N_BINS, 1) or x.dtype != np.float32:
            raise ValueError("input must be float32 [1,1,256,1], got %s %s" % (x.dtype, x.shape))
        eng = self.engine
        for base, shp in self._specs:
            k_in, k_out = base.format("prev"), base.format("cur")
            a = feeds[k_in]
            want = self._io_shape(shp)
            if not isinstance(a, np.ndarray) or a.dtype != np.float32 or a.shape != want:
                raise ValueError("%s must be float32 %s" % (k_in, want))
            # the echo of our own output, not edited since: the device already holds it
            if self._last.get(k_out) is a and np.array_equal(a.reshape(-1), self._snap[k_out]):
                continue
            eng.state_set(k_in, a)
        out = eng.step(x.reshape(1, T.N_BINS))
        res = {"model_out": out.reshape(1, 1, T.N_BINS, 1)}
        snap = eng.state_get_all(0)                 # one D2H copy for the 130 / 208 tensors
        pub = snap.copy()                           # the caller's arrays: writable, independent of the snapshot
        o = 0
        for base, shp in self._specs:
            n = int(np.prod(shp))
            res[base.format("cur")] = pub[o:o + n].reshape(self._io_shape(shp))
            self._snap[base.format("cur")] = snap[o:o + n]
            o += n
        self._last = res
        return res


def plan_ragged_blocks(lengths_in_hops, utterances: int, max_frames: int):
    """The schedule of :meth:`NutlsOffline.enhance_many`, a pure function: ``lengths_in_hops[i]`` hops (or frames) of item ``i`` through
    ``utterances`` slots in blocks of at most ``max_frames`` per slot.  Returns a list of blocks, each a list of
    ``(slot, item, first_hop, count, reset_before)`` in slot order: the block takes hops ``first_hop .. first_hop + count - 1`` of ``item`` in
    ``slot``; ``reset_before`` marks the first block of an item in its slot (the slot is reset in front of it).  An item stays in its slot
    until it ends and continues there block after block; a slot whose item has ended takes the next item of the queue in the next block;
    a slot with nothing to do is absent from the block (count 0: held).  The queue is served longest first, so that the blocks at the end of
    the run, which the last items have to themselves, are short ones.  Items of length 0 take no slot."""
    lengths = [int(n) for n in lengths_in_hops]
    utterances, max_frames = int(utterances), int(max_frames)
    if utterances < 1 or max_frames < 1 or any(n < 0 for n in lengths):
        raise ValueError("plan_ragged_blocks: utterances and max_frames must be >= 1, lengths >= 0")
    queue = sorted((i for i, n in enumerate(lengths) if n > 0), key=lambda i: (-lengths[i], i))
    slots = [None] * utterances          # per slot: [item, next hop]
    blocks, q = [], 0
    while True:
        for u in range(utterances):
            if slots[u] is None and q < len(queue):
                slots[u] = [queue[q], 0]
                q += 1
        block = []
        for u, cur in enumerate(slots):
            if cur is None:
                continue
            item, first = cur
            count = min(max_frames, lengths[item] - first)
            block.append((u, item, first, count, first == 0))
            cur[1] = first + count
            if cur[1] == lengths[item]:
                slots[u] = None
        if not block:
            return blocks
        blocks.append(block)


class NutlsOffline(_PcmFormat):
    """Offline / block mode: ``utterances`` independent utterances, up to ``max_frames`` consecutive frames of each
    per call -- every conv-like layer runs once per block over all frames of all utterances (the frame index takes the place of
    the stream index), only the LSTM recurrences are scanned (side by side for the utterances).  Same function as a streaming
    engine fed frame by frame (the offline forward of the reference, models/proposed.py:284-625, takes ``[B, T, ...]``); every
    utterance's state carries over between calls until :meth:`reset`."""

    CTFA_MODES = {"frame": 0, "causal32": 1}

    def __init__(self, weights=None, max_frames: int = 256, device: int = 0, ctfa_mode: str = "frame", pipeline: int = 0, utterances: int = 1):
        """``ctfa_mode``: "frame" (default; the frame-wise graph's TA/32, equal to the streaming result) or "causal32"
        (the offline model's true 32-frame causal average of the time attention, models/proposed.py:143-147).
        ``pipeline``: chunks of consecutive frames a block of ONE utterance is cut into, each on its own HIP stream one bottleneck
        behind the chunk before it (1..16; 0 = chosen from the block length).  The result does not depend on it.
        ``utterances``: the batch dimension (``nutls_create_offline_batch``); ``process`` then takes ``[utterances, N, 256]``."""
        if ctfa_mode not in self.CTFA_MODES:
            raise ValueError("ctfa_mode must be one of %s" % sorted(self.CTFA_MODES))
        self._lib = load_library()
        blob = read_blob(weights if weights is not None else DEFAULT_WEIGHTS)
        self._h = ctypes.c_void_p()
        self.max_frames = int(max_frames)
        self.utterances = int(utterances)
        _check(self._lib, self._lib.nutls_create_offline_batch(blob, len(blob), self.max_frames, self.utterances, int(device), ctypes.byref(self._h)))
        if ctfa_mode != "frame":
            _check(self._lib, self._lib.nutls_offline_set_ctfa_mode(self._h, self.CTFA_MODES[ctfa_mode]))
        self.ctfa_mode = ctfa_mode
        if pipeline:
            self.set_pipeline(pipeline)

    def set_pipeline(self, chunks: int):
        _check(self._lib, self._lib.nutls_offline_set_pipeline(self._h, int(chunks)))

    def process(self, mags) -> np.ndarray:
        """``mags [N,256]`` (one utterance) or ``[utterances,N,256]`` float32 (any N) -> enhanced magnitudes of the same shape; blocks of
        ``max_frames`` frames of every utterance."""
        m = np.ascontiguousarray(mags, dtype=np.float32)
        batched = m.ndim == 3
        if self.utterances == 1 and m.ndim == 2:
            m = m[None]
        if m.ndim != 3 or m.shape[0] != self.utterances or m.shape[2] != T.N_BINS:
            raise ValueError("mags must be [%s N,%d], got %s" % ("%d," % self.utterances if self.utterances > 1 else "", T.N_BINS, np.shape(mags)))
        out = np.empty_like(m)
        for a in range(0, m.shape[1], self.max_frames):
            blk = np.ascontiguousarray(m[:, a:a + self.max_frames])
            o = np.empty_like(blk)
            _check(self._lib, self._lib.nutls_process_block_host(self._h, _fptr(blk), _fptr(o), blk.shape[1]))
            out[:, a:a + blk.shape[1]] = o
        return out if batched else out[0]

    def _device_counts(self, counts, n: int, like, name: str):
        """Per-utterance counts of a device call -> device pointer.  An int32 CUDA tensor ``[utterances]`` is handed to the kernels as it is
        (it must stay unmodified until the queued work has run; the kernels clamp its values to ``0 .. n``); anything else array-like is
        checked here (``0 .. n``) and copied to the device."""
        import torch
        if torch.is_tensor(counts) and counts.is_cuda:
            if counts.dtype != torch.int32 or not counts.is_contiguous() or tuple(counts.shape) != (self.utterances,) or counts.device != like.device:
                raise ValueError("%s must be a contiguous int32 CUDA tensor of length %d on the block's device" % (name, self.utterances))
            return counts.data_ptr()
        host = self._host_counts(counts, n, name)
        self._counts_dev = torch.from_numpy(host).to(like.device)      # (kept until the next call: the queued kernels read it)
        return self._counts_dev.data_ptr()

    def _host_counts(self, counts, n: int, name: str) -> np.ndarray:
        a = np.asarray(counts.cpu() if hasattr(counts, "cpu") else counts)
        if a.shape != (self.utterances,) or a.dtype.kind not in "iu":
            raise ValueError("%s must be %d integers (one count per utterance), got %s %s" % (name, self.utterances, a.dtype, a.shape))
        if a.size and (int(a.min()) < 0 or int(a.max()) > n):
            raise ValueError("%s must lie in 0 .. %d (the block's row stride), got %s" % (name, n, a.tolist()))
        return np.ascontiguousarray(a, dtype=np.int32)

    def process_block_device(self, mag, out=None, frames=None):
        """One block on device tensors: ``mag [n,256]`` (one utterance) or ``[utterances,n,256]`` float32 CUDA tensor, n <= max_frames;
        asynchronous on the current torch stream.  ``frames`` (``nutls_process_block_ragged``): how many leading frames of every utterance
        are real -- an int32 CUDA tensor ``[utterances]`` or anything array-like; rows behind a count are zeros in ``out``, have no effect
        as input, and the utterance carries on from its own last real frame (count 0: the utterance is held).  ``None``: all ``n`` of all."""
        import torch
        if not (torch.is_tensor(mag) and mag.is_cuda and mag.dtype == torch.float32 and mag.is_contiguous()):
            raise ValueError("mag must be a contiguous float32 CUDA tensor")
        shape = tuple(mag.shape)
        want3 = mag.dim() == 3
        ok = (want3 and shape[0] == self.utterances) or (mag.dim() == 2 and self.utterances == 1)
        if not ok or shape[-1] != T.N_BINS or shape[-2] > self.max_frames:
            raise ValueError("mag must be [%sn<=%d,%d], got %s" % ("%d," % self.utterances if self.utterances > 1 else "", self.max_frames, T.N_BINS, shape))
        if out is None:
            out = torch.empty_like(mag)
        stream = torch.cuda.current_stream(mag.device).cuda_stream
        if frames is None:
            _check(self._lib, self._lib.nutls_process_block(self._h, mag.data_ptr(), out.data_ptr(), int(shape[-2]), stream))
        else:
            cnt = self._device_counts(frames, int(shape[-2]), mag, "frames")
            _check(self._lib, self._lib.nutls_process_block_ragged(self._h, mag.data_ptr(), out.data_ptr(), int(shape[-2]), cnt, stream))
        return out

    # -- waveform block mode: STFT / inverse STFT + overlap-add of whole blocks on the device (csrc/stft_block.hip) --------------
    _DC = {"edge": 0, "zero": 1}

    def _dc(self, dc_mode: str) -> int:
        if dc_mode not in self._DC:
            raise ValueError("dc_mode must be 'edge' or 'zero'")
        return self._DC[dc_mode]

    @staticmethod
    def _cuda_f32(x, name: str):
        import torch
        if not (torch.is_tensor(x) and x.is_cuda and x.dtype == torch.float32 and x.is_contiguous()):
            raise ValueError("%s must be a contiguous float32 CUDA tensor" % name)
        return x

    def _pcm_hops(self, pcm, name: str = "pcm") -> int:
        self._cuda_f32(pcm, name)
        shape = tuple(pcm.shape)
        ok = (pcm.dim() == 2 and shape[0] == self.utterances) or (pcm.dim() == 1 and self.utterances == 1)
        if not ok or shape[-1] % 256 or not 1 <= shape[-1] // 256 <= self.max_frames:
            raise ValueError("%s must be [%sn_hops*256] with 1 <= n_hops <= %d, got %s" % (
                name, "%d," % self.utterances if self.utterances > 1 else "", self.max_frames, shape))
        return shape[-1] // 256

    def _mag_hops(self, mag, name: str = "mag") -> int:
        self._cuda_f32(mag, name)
        shape = tuple(mag.shape)
        ok = (mag.dim() == 3 and shape[0] == self.utterances) or (mag.dim() == 2 and self.utterances == 1)
        if not ok or shape[-1] != T.N_BINS or not 1 <= shape[-2] <= self.max_frames:
            raise ValueError("%s must be [%s1<=n<=%d,%d], got %s" % (
                name, "%d," % self.utterances if self.utterances > 1 else "", self.max_frames, T.N_BINS, shape))
        return shape[-2]

    def enhance_block_device(self, pcm, out=None, dc_mode: str = "edge", hops=None):
        """One block of PCM on device tensors: ``pcm [n_hops*256]`` (one utterance) or ``[utterances, n_hops*256]`` float32 CUDA tensor,
        n_hops <= max_frames -> the enhanced PCM of the same shape, one hop late like ``NutlsEngine.enhance_hop``
        (``nutls_enhance_block``: analysis, ``process_block``, synthesis); asynchronous on the current torch stream.
        ``hops``: per-utterance counts as ``frames`` of :meth:`process_block_device` (``nutls_enhance_block_ragged``); the PCM rows behind a
        count are never read, the matching rows of ``out`` are zeros."""
        import torch
        dc = self._dc(dc_mode)
        n = self._pcm_hops(pcm)
        if out is None:
            out = torch.empty_like(pcm)
        elif self._cuda_f32(out, "out").shape != pcm.shape or out.device != pcm.device:
            raise ValueError("out must have pcm's shape and device")
        stream = torch.cuda.current_stream(pcm.device).cuda_stream
        if hops is None:
            _check(self._lib, self._lib.nutls_enhance_block(self._h, pcm.data_ptr(), out.data_ptr(), n, dc, stream))
        else:
            _check(self._lib, self._lib.nutls_enhance_block_ragged(self._h, pcm.data_ptr(), out.data_ptr(), n, self._device_counts(hops, n, pcm, "hops"), dc, stream))
        return out

    def stft_block_device(self, pcm, out=None, hops=None):
        """Analysis half only: ``pcm`` as in :meth:`enhance_block_device` -> magnitudes of bins 1..256, ``[n_hops,256]`` /
        ``[utterances,n_hops,256]`` (what :meth:`process_block_device` takes); the phase stays inside the handle
        (``debug_get("phasor_block", (n_hops, 257, 2))``).  ``hops``: per-utterance counts (``nutls_stft_block_ragged``)."""
        import torch
        n = self._pcm_hops(pcm)
        shape = tuple(pcm.shape[:-1]) + (n, T.N_BINS)
        if out is None:
            out = torch.empty(shape, dtype=torch.float32, device=pcm.device)
        elif tuple(self._cuda_f32(out, "out").shape) != shape or out.device != pcm.device:
            raise ValueError("out must be %s on pcm's device" % (shape,))
        stream = torch.cuda.current_stream(pcm.device).cuda_stream
        if hops is None:
            _check(self._lib, self._lib.nutls_stft_block(self._h, pcm.data_ptr(), out.data_ptr(), n, stream))
        else:
            _check(self._lib, self._lib.nutls_stft_block_ragged(self._h, pcm.data_ptr(), out.data_ptr(), n, self._device_counts(hops, n, pcm, "hops"), stream))
        return out

    def istft_block_device(self, mag, out=None, dc_mode: str = "edge", hops=None, noisy=None):
        """Synthesis half only: magnitudes ``[n_hops,256]`` / ``[utterances,n_hops,256]`` with the phase of the last
        :meth:`stft_block_device` of the same ``n_hops`` -> PCM ``[n_hops*256]`` / ``[utterances,n_hops*256]``, overlap-added.
        ``hops``: the counts that analysis was given (``nutls_istft_block_ragged``).  ``noisy``: the magnitudes that analysis returned, of
        ``mag``'s shape -- the half then honours the attenuation limit (``set_atten_limit``; ``nutls_istft_block_mix``); without it the
        limit is ignored."""
        import torch
        dc = self._dc(dc_mode)
        n = self._mag_hops(mag)
        if noisy is not None and (self._mag_hops(noisy, "noisy") != n or noisy.shape != mag.shape or noisy.device != mag.device):
            raise ValueError("noisy must have mag's shape and device")
        shape = tuple(mag.shape[:-2]) + (n * 256,)
        if out is None:
            out = torch.empty(shape, dtype=torch.float32, device=mag.device)
        elif tuple(self._cuda_f32(out, "out").shape) != shape or out.device != mag.device:
            raise ValueError("out must be %s on mag's device" % (shape,))
        stream = torch.cuda.current_stream(mag.device).cuda_stream
        if noisy is not None:
            counts = None if hops is None else self._device_counts(hops, n, mag, "hops")
            _check(self._lib, self._lib.nutls_istft_block_mix(self._h, mag.data_ptr(), noisy.data_ptr(), out.data_ptr(), n, counts, dc, stream))
        elif hops is None:
            _check(self._lib, self._lib.nutls_istft_block(self._h, mag.data_ptr(), out.data_ptr(), n, dc, stream))
        else:
            _check(self._lib, self._lib.nutls_istft_block_ragged(self._h, mag.data_ptr(), out.data_ptr(), n, self._device_counts(hops, n, mag, "hops"), dc, stream))
        return out

    def enhance_block_host(self, pcm: np.ndarray, out: Optional[np.ndarray] = None, dc_mode: str = "edge") -> np.ndarray:
        """One block on host arrays (pageable or from ``host_alloc``): ``pcm [utterances, n_hops*256]`` float32 contiguous,
        n_hops <= max_frames (``nutls_enhance_block_host``; synchronous)."""
        dc = self._dc(dc_mode)
        if not (isinstance(pcm, np.ndarray) and pcm.dtype == np.float32 and pcm.flags.c_contiguous and pcm.ndim == 2
                and pcm.shape[0] == self.utterances and pcm.shape[1] % 256 == 0):
            raise ValueError("pcm must be a contiguous float32 array [%d, n_hops*256], got %s" % (self.utterances, np.shape(pcm)))
        if out is None:
            out = np.empty_like(pcm)
        elif not (isinstance(out, np.ndarray) and out.dtype == np.float32 and out.flags.c_contiguous and out.shape == pcm.shape):
            raise ValueError("out must be a contiguous float32 numpy array of pcm's shape")
        _check(self._lib, self._lib.nutls_enhance_block_host(self._h, _fptr(pcm), _fptr(out), pcm.shape[1] // 256, dc))
        return out

    def enhance(self, wave, dc_mode: str = "edge", atten_lim_db=None) -> np.ndarray:
        """``wave [N]`` (one utterance) or ``[utterances, N]`` float, any N -> the enhanced waveform of the same shape, in the alignment
        of ``stream_enhance.enhance_batch_on_device`` / ``real_time_speech_enhancer`` (the first output hop, the leading half window,
        is dropped: interpreter_proposed.py:368).  ``(N - 256) // 256`` hops run in blocks of ``max_frames`` through
        ``nutls_enhance_block_host``; previous hop, overlap tail and model state carry on into the next call until :meth:`reset`.
        ``atten_lim_db``: a cap in dB on the noise removed, a scalar or one value per utterance (``set_atten_limit(db=...)``, which stays in
        force afterwards); ``None`` leaves the handle's limits as they are."""
        self._dc(dc_mode)
        if atten_lim_db is not None:
            self.set_atten_limit(db=atten_lim_db)
        x = np.asarray(wave, dtype=np.float32)
        batched = x.ndim == 2
        if x.ndim == 1 and self.utterances == 1:
            x = x[None]
        if x.ndim != 2 or x.shape[0] != self.utterances:
            raise ValueError("wave must be [%sN], got %s" % ("%d," % self.utterances if self.utterances > 1 else "", np.shape(wave)))
        n = x.shape[1]
        hops = max(0, (n - 256) // 256)
        out = np.zeros((self.utterances, n + 256), np.float64)
        for a in range(0, hops, self.max_frames):
            b = min(hops, a + self.max_frames)
            blk = np.ascontiguousarray(x[:, a * 256:b * 256])
            out[:, a * 256:b * 256] = self.enhance_block_host(blk, None, dc_mode)
        out = out[:, 256:]
        return out if batched else out[0]

    # -- PCM gateway: blocks in the callers' sample rate and type (csrc/pcm.hip) ---------------------------------------------------
    def _pcm_block_hops(self, cols: int, unit: int, name: str) -> int:
        if cols % unit or not 1 <= cols // unit <= self.max_frames:
            raise ValueError("%s must be [%d, n_hops*%d] with 1 <= n_hops <= %d" % (name, self.utterances, unit, self.max_frames))
        return cols // unit

    def enhance_block_pcm_device(self, pcm, out=None, dc_mode: str = "edge", hops=None):
        """``enhance_block_device`` in the format of ``set_pcm_format``: ``pcm [utterances, n_hops * pcm_hop_samples]`` CUDA tensor of the
        handle's sample type -> the enhanced block in the same format (``nutls_enhance_block_pcm``), ``pcm_delay_samples`` plus one hop late;
        the resampler histories carry from block to block.  ``hops``: per-utterance counts as in :meth:`enhance_block_device`
        (``nutls_enhance_block_pcm_ragged``): the hops behind a count are never read and come back as zeros, every history of the
        utterance carries on from its last real hop, a count of 0 holds it."""
        import torch
        dc = self._dc(dc_mode)
        S = self.pcm_hop_samples
        n = self._pcm_block_hops(self._pcm_cols(pcm), S, "pcm")
        x = self._pcm_tensor(pcm, self.utterances, n * S, "pcm")
        o = torch.empty_like(x) if out is None else self._pcm_tensor(out, self.utterances, n * S, "out")
        stream = torch.cuda.current_stream(x.device).cuda_stream
        if hops is None:
            _check(self._lib, self._lib.nutls_enhance_block_pcm(self._h, x.data_ptr(), o.data_ptr(), n, dc, stream))
        else:
            _check(self._lib, self._lib.nutls_enhance_block_pcm_ragged(self._h, x.data_ptr(), o.data_ptr(), n, self._device_counts(hops, n, x, "hops"), dc, stream))
        return o

    def enhance_block_pcm_host(self, pcm: np.ndarray, out: Optional[np.ndarray] = None, dc_mode: str = "edge") -> np.ndarray:
        """The same on host arrays (``nutls_enhance_block_pcm_host``; synchronous)."""
        dc = self._dc(dc_mode)
        S = self.pcm_hop_samples
        n = self._pcm_block_hops(self._pcm_cols(pcm) if isinstance(pcm, np.ndarray) else -1, S, "pcm")
        x = self._pcm_array(pcm, self.utterances, n * S, "pcm")
        o = np.empty_like(x) if out is None else self._pcm_array(out, self.utterances, n * S, "out")
        _check(self._lib, self._lib.nutls_enhance_block_pcm_host(self._h, x.ctypes.data, o.ctypes.data, n, dc))
        return o

    def pcm_decode_block_device(self, pcm, out=None, hops=None):
        """The decode half on its own: ``[utterances, n_hops * pcm_hop_samples]`` of the handle's sample type -> ``[utterances, n_hops*256]``
        float32 at 16 kHz (what ``enhance_block_device`` takes).  ``hops``: per-utterance counts (``nutls_pcm_decode_block_ragged``)."""
        import torch
        S = self.pcm_hop_samples
        n = self._pcm_block_hops(self._pcm_cols(pcm), S, "pcm")
        x = self._pcm_tensor(pcm, self.utterances, n * S, "pcm")
        o = (torch.empty((self.utterances, n * 256), dtype=torch.float32, device=x.device) if out is None
             else self._pcm_tensor(out, self.utterances, n * 256, "out", torch.float32))
        stream = torch.cuda.current_stream(x.device).cuda_stream
        if hops is None:
            _check(self._lib, self._lib.nutls_pcm_decode_block(self._h, x.data_ptr(), o.data_ptr(), n, stream))
        else:
            _check(self._lib, self._lib.nutls_pcm_decode_block_ragged(self._h, x.data_ptr(), o.data_ptr(), n, self._device_counts(hops, n, x, "hops"), stream))
        return o

    def pcm_encode_block_device(self, wave, out=None, hops=None):
        """The encode half on its own: ``[utterances, n_hops*256]`` float32 at 16 kHz -> the handle's format.  ``hops``: per-utterance counts
        (``nutls_pcm_encode_block_ragged``)."""
        import torch
        S = self.pcm_hop_samples
        n = self._pcm_block_hops(int(wave.shape[-1]) if hasattr(wave, "shape") and len(wave.shape) == 2 else -1, 256, "wave")
        x = self._pcm_tensor(wave, self.utterances, n * 256, "wave", torch.float32)
        o = (torch.empty(self._pcm_shapes(self.utterances, n * S)[0], dtype=getattr(torch, self.pcm_dtype), device=x.device) if out is None
             else self._pcm_tensor(out, self.utterances, n * S, "out"))
        stream = torch.cuda.current_stream(x.device).cuda_stream
        if hops is None:
            _check(self._lib, self._lib.nutls_pcm_encode_block(self._h, x.data_ptr(), o.data_ptr(), n, stream))
        else:
            _check(self._lib, self._lib.nutls_pcm_encode_block_ragged(self._h, x.data_ptr(), o.data_ptr(), n, self._device_counts(hops, n, x, "hops"), stream))
        return o

    def _wave_through_blocks(self, x: np.ndarray, lag: int, block) -> np.ndarray:
        """``x [utterances, N]`` (with channels: ``[utterances / C, N, C]``) of the handle's sample type, padded with zeros (G.711: the silence code) to whole hops that cover ``N + lag`` samples, through
        ``block`` (array ``[utterances, n_hops * pcm_hop_samples]`` -> array of the same shape, n_hops <= max_frames) in blocks of
        ``max_frames`` hops; the first ``lag`` samples of the result are dropped, so that sample i of what is returned belongs to ``x[:, i]``."""
        S = self.pcm_hop_samples
        n = x.shape[1]
        hops = max(1, -(-(n + lag) // S))
        padded = np.full((x.shape[0], hops * S) + x.shape[2:], self.pcm_silence, x.dtype)
        padded[:, :n] = x
        out = np.empty_like(padded)
        for a in range(0, hops, self.max_frames):
            b = min(hops, a + self.max_frames)
            out[:, a * S:b * S] = block(np.ascontiguousarray(padded[:, a * S:b * S]))
        return out[:, lag:lag + n]

    @staticmethod
    def _wave_format(dtype, rate, codec):
        """What ``set_pcm_format`` is told for recordings of ``dtype`` at ``rate`` with ``codec``; ``ValueError`` for what does not go together.
        A numpy dtype cannot say which law a byte array is in: uint8 needs ``codec``, and ``codec`` needs uint8 at 8000 Hz."""
        name = np.dtype(dtype).name
        if codec is None:
            if name == "uint8":
                raise ValueError("uint8 samples are G.711 codes: say which law with codec='ulaw' or codec='alaw'")
            if name not in ("float32", "int16"):
                raise ValueError("samples must be int16 or float32 (or uint8 with a codec), got %s" % name)
            return name
        _g711_format(codec)
        if name != "uint8":
            raise ValueError("codec=%r takes uint8 samples (G.711 codes), got %s" % (codec, name))
        if isinstance(rate, bool) or not isinstance(rate, (int, np.integer)) or int(rate) != 8000:
            raise ValueError("codec=%r is G.711, which is 8 kHz: rate must be 8000, got %r" % (codec, rate))
        return codec

    def enhance_wave(self, wave, rate: int, dc_mode: str = "edge", codec: Optional[str] = None, upper_gain: float = 0.0,
                     upper_follow: bool = False) -> np.ndarray:
        """A whole recording in its own format: ``wave [N]`` (one utterance) or ``[utterances, N]``, int16 or float32 numpy array of any
        length at ``rate`` (8000, 16000, 32000, 48000) -> the enhanced recording of the same shape and dtype, ALIGNED with the input:
        sample i of the result belongs to ``wave[i]`` (the input is padded with zeros to whole hops plus the total lag, one hop plus
        ``pcm_delay_samples``, and that lag is dropped from the front).  Sets the handle's format (``set_pcm_format``: the rate conversion
        starts from a zero history); the model state carries on from earlier calls until :meth:`reset`.  ``codec``: "ulaw" or "alaw" for a
        uint8 array of G.711 codes at 8000 Hz (a dtype cannot say which law: required for uint8, ``ValueError`` with any other dtype or
        rate); the padding is then the law's silence code, the result uint8 codes of the same law.  ``upper_gain``: the gain of the band
        above 8 kHz of a 32 or 48 kHz recording, passed around the model (``set_pcm_upper_band``, set after the format); 0.0: the result is
        band-limited to 8 kHz.  ``upper_follow``: that gain is the ceiling of one that follows the model's suppression
        (``set_pcm_upper_follow``, set after the gain).  One row per utterance: the handle's layout becomes 1 channel
        (``set_pcm_channels``); interleaved frames ``[N, C]``: :meth:`enhance_wave_channels`."""
        self._dc(dc_mode)
        x = np.asarray(wave)
        fmt = self._wave_format(x.dtype, rate, codec)
        self.set_pcm_channels(1)
        batched = x.ndim == 2
        if x.ndim == 1 and self.utterances == 1:
            x = x[None]
        if x.ndim != 2 or x.shape[0] != self.utterances:
            raise ValueError("wave must be [%sN], got %s" % ("%d," % self.utterances if self.utterances > 1 else "", np.shape(wave)))
        self.set_pcm_format(rate, fmt)
        self.set_pcm_upper_band(upper_gain)
        self.set_pcm_upper_follow(upper_follow)
        lag = self.pcm_hop_samples + self.pcm_delay_samples
        out = self._wave_through_blocks(x, lag, lambda blk: self.enhance_block_pcm_host(blk, None, dc_mode))
        return out if batched else out[0]

    def enhance_wave_channels(self, wave, rate: int, channels: int, dc_mode: str = "edge", codec: Optional[str] = None, upper_gain: float = 0.0,
                              upper_follow: bool = False) -> np.ndarray:
        """:meth:`enhance_wave` of interleaved frames: ``wave [N, C]``, the layout of ``scipy.io.wavfile`` / ``soundfile``, on a handle of
        ``utterances == C``, or ``[utterances / C, N, C]``, ``channels`` = C, 2 or 4.  Every channel is an utterance of its own
        (``set_pcm_channels``, which stays in force): channel c of recording r is utterance ``r * C + c``, and the result -- same shape and
        dtype, aligned like :meth:`enhance_wave`'s -- is bit for bit what :meth:`enhance_wave` returns for the transposed array on a
        1-channel handle of the same shape.  The split and the join happen on the device.  (A method of its own, like
        ``enhance_many_atten``: ``enhance_wave`` keeps the signature it has.)"""
        self._dc(dc_mode)
        x = np.asarray(wave)
        fmt = self._wave_format(x.dtype, rate, codec)
        if channels not in (2, 4):
            raise ValueError("channels must be 2 or 4, got %r (one row per utterance: enhance_wave)" % (channels,))
        self.set_pcm_channels(channels)      # (ValueError: the handle's utterances are no multiple of it)
        batched = x.ndim == 3
        if x.ndim == 2 and self.utterances == channels:
            x = x[None]
        if x.ndim != 3 or x.shape[0] * channels != self.utterances or x.shape[2] != channels:
            raise ValueError("with channels=%d wave must be [%sN,%d], got %s" % (
                channels, "%d," % (self.utterances // channels) if self.utterances > channels else "", channels, np.shape(x)))
        self.set_pcm_format(rate, fmt)
        self.set_pcm_upper_band(upper_gain)
        self.set_pcm_upper_follow(upper_follow)
        lag = self.pcm_hop_samples + self.pcm_delay_samples
        out = self._wave_through_blocks(x, lag, lambda blk: self.enhance_block_pcm_host(blk, None, dc_mode))
        return out if batched else out[0]

    # -- ragged blocks: per-utterance counts (nutls_process_block_ragged_host / nutls_enhance_block_ragged_host) ---------------------
    def _ragged_host(self, entry, chunks, unit: int, *tail, dtype=None, channels: int = 1):
        """One ragged block through a ``_host`` entry.  ``chunks[u]``: utterance u's piece of the block, ``k_u`` frames ``[k_u,256]``
        (``unit`` 1) or ``k_u`` hops of PCM ``[k_u * unit]`` (``unit`` 256: float32 at 16 kHz), k_u <= max_frames and at least one > 0; the
        row stride of the block is the longest count.  ``dtype``: the sample type of an entry that takes the callers' format (``unit`` =
        ``pcm_hop_samples``, buffers handed over as addresses); None: float32.  Returns each utterance's piece of the result.
        ``channels`` (``set_pcm_channels``): ``chunks[r]`` is frame row r's piece ``[k_r * unit, C]``, and each of its C utterances gets its count."""
        counts = np.array([c.shape[0] // unit for c in chunks], np.int32)
        n = int(counts.max())
        counts = np.ascontiguousarray(np.repeat(counts, channels))
        blk = np.zeros((len(chunks), n * unit) + chunks[0].shape[1:], dtype or np.float32)
        for u, c in enumerate(chunks):
            blk[u, :c.shape[0]] = c
        out = np.empty_like(blk)
        ptr = _fptr if dtype is None else (lambda a: a.ctypes.data)
        _check(self._lib, entry(self._h, ptr(blk), ptr(out), n, counts.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), *tail))
        return [out[u, :c.shape[0]] for u, c in enumerate(chunks)]

    def _ragged_list(self, items, what: str, ndim: int):
        items = [np.ascontiguousarray(x, dtype=np.float32) for x in items]
        if len(items) != self.utterances or any(x.ndim != ndim or (ndim == 2 and x.shape[1] != T.N_BINS) for x in items):
            raise ValueError("%s must be a list of %d arrays %s (one per utterance, any lengths)" % (
                what, self.utterances, "[N,%d]" % T.N_BINS if ndim == 2 else "[N]"))
        return items

    def process_ragged(self, mags_list) -> List[np.ndarray]:
        """``utterances`` magnitude arrays ``[N_u,256]`` of ANY lengths (0 included) -> the enhanced magnitudes, same lengths.  Blocks of
        ``max_frames``: utterance u takes ``min(max_frames, remaining)`` frames of each (``nutls_process_block_ragged_host``), an
        utterance that has ended is held.  State carries on into the next call until :meth:`reset` / :meth:`reset_utterance`."""
        mags = self._ragged_list(mags_list, "mags_list", 2)
        outs = [np.empty_like(m) for m in mags]
        for a in range(0, max([len(m) for m in mags] + [0]), self.max_frames):
            got = self._ragged_host(self._lib.nutls_process_block_ragged_host, [m[a:a + self.max_frames] for m in mags], 1)
            for o, g in zip(outs, got):
                o[a:a + len(g)] = g
        return outs

    def enhance_ragged(self, waves_list, dc_mode: str = "edge", atten_lim_db=None) -> List[np.ndarray]:
        """``utterances`` waveforms ``[N_u]`` of ANY lengths -> the enhanced waveforms, same lengths, each in the alignment of
        :meth:`enhance` (``(N_u - 256) // 256`` hops, the first output hop dropped); blocks of ``max_frames`` hops through
        ``nutls_enhance_block_ragged_host``.  Previous hop, overlap tail and model state of every utterance carry on until :meth:`reset`.
        ``atten_lim_db``: as in :meth:`enhance`."""
        dc = self._dc(dc_mode)
        if atten_lim_db is not None:
            self.set_atten_limit(db=atten_lim_db)
        waves = self._ragged_list(waves_list, "waves_list", 1)
        hops = [max(0, (len(w) - 256) // 256) for w in waves]
        outs = [np.zeros(len(w) + 256, np.float64) for w in waves]
        for a in range(0, max(hops), self.max_frames):
            chunks = [w[a * 256:min(h, a + self.max_frames) * 256] for w, h in zip(waves, hops)]
            got = self._ragged_host(self._lib.nutls_enhance_block_ragged_host, chunks, 256, dc)
            for o, g in zip(outs, got):
                o[a * 256:a * 256 + len(g)] = g
        return [o[256:] for o in outs]

    def enhance_many(self, waves, dc_mode: str = "edge", rate: Optional[int] = None) -> List[np.ndarray]:
        """ANY NUMBER of recordings ``[N_i]`` of any lengths through the handle's ``utterances`` slots (:func:`plan_ragged_blocks`: longest
        first; a recording longer than one block continues in its slot, a slot whose recording has ended is reset and takes the next one of
        the queue in the next block, the other slots are not disturbed) -> the enhanced recordings in input order, each what
        :meth:`enhance` of a fresh one-utterance handle returns for it.  Every slot that was used starts from a reset.
        ``rate`` (8000, 16000, 32000, 48000): the recordings are in the callers' format, int16 or float32 arrays at that rate, all of one
        dtype; each result then has its input's length and dtype and is ALIGNED with it, what :meth:`enhance_wave` of a fresh one-utterance
        handle returns (``nutls_enhance_block_pcm_ragged_host``).  Sets the handle's format, which turns the upper band
        (``set_pcm_upper_band``) and with it its following gain (``set_pcm_upper_follow``) off: the results are band-limited to 8 kHz.
        uint8 arrays of G.711 codes are refused here (a dtype cannot say which law): :meth:`enhance_many_codec`.  Recordings of
        interleaved frames ``[N_i, C]``: :meth:`enhance_many_channels`."""
        return self._enhance_many(waves, dc_mode, rate, None)

    def enhance_many_channels(self, waves, rate: int, channels: int, dc_mode: str = "edge", codec: Optional[str] = None,
                              atten_lim_db=None) -> List[np.ndarray]:
        """:meth:`enhance_many` for recordings of interleaved frames: each ``waves[i]`` is ``[N_i, C]``, ``channels`` = C, 2 or 4, at
        ``rate`` (int16 or float32; uint8 G.711 codes with ``codec``, as in :meth:`enhance_many_codec`).  The scheduler plans
        ``utterances // C`` frame rows (:func:`plan_ragged_blocks`); every channel of a row is an utterance of its own and gets the row's
        hop count, its reset and the recording's limit (``atten_lim_db``: as in :meth:`enhance_many_atten`).  Each result has its input's
        shape and dtype, aligned with it; ``set_pcm_channels`` stays in force.  The split and the join happen on the device
        (``nutls_enhance_block_pcm_ragged_host``).  (A method of its own, like ``enhance_many_atten``: ``enhance_many`` keeps the
        signature it has.)"""
        dc = self._dc(dc_mode)
        if channels not in (2, 4):
            raise ValueError("channels must be 2 or 4, got %r (one row per utterance: enhance_many)" % (channels,))
        waves = [np.asarray(w) for w in waves]
        if codec is not None:
            for w in waves:
                self._wave_format(w.dtype, rate, codec)
            self._wave_format(np.uint8, rate, codec)
        limits = None
        if atten_lim_db is not None:
            seq = list(atten_lim_db) if isinstance(atten_lim_db, (list, tuple, np.ndarray)) else [atten_lim_db] * len(waves)
            if len(seq) != len(waves):
                raise ValueError("atten_lim_db must be a scalar or one value per recording (%d), got %d" % (len(waves), len(seq)))
            limits = [atten_limit_from_db(d) for d in seq]
        return self._enhance_many_pcm(waves, dc, rate, limits, codec, channels)

    def enhance_many_atten(self, waves, atten_lim_db, dc_mode: str = "edge", rate: Optional[int] = None) -> List[np.ndarray]:
        """:meth:`enhance_many` with an attenuation limit per recording: ``atten_lim_db`` a cap in dB on the noise removed, a scalar for
        every recording or one value per recording, ``None`` entries for no cap (``set_atten_limit``).  The scheduler sets a slot's limit
        when it hands the slot a recording; each result is what :meth:`enhance` of a fresh one-utterance handle returns for that recording
        with its ``atten_lim_db``.  The limits of the last recordings stay in force on the slots afterwards.  (A method of its own:
        ``enhance_many`` keeps the signature it has.)"""
        n = len(waves)
        seq = list(atten_lim_db) if isinstance(atten_lim_db, (list, tuple, np.ndarray)) else [atten_lim_db] * n
        if len(seq) != n:
            raise ValueError("atten_lim_db must be a scalar or one value per recording (%d), got %d" % (n, len(seq)))
        return self._enhance_many(waves, dc_mode, rate, [atten_limit_from_db(d) for d in seq])

    def enhance_many_codec(self, waves, codec: str, dc_mode: str = "edge", rate: int = 8000, atten_lim_db=None) -> List[np.ndarray]:
        """:meth:`enhance_many` for an archive of G.711 recordings: ``waves`` uint8 arrays ``[N_i]`` of codes of ONE law, ``codec`` "ulaw" or
        "alaw" (a dtype cannot say which), ``rate`` 8000 -- the only rate G.711 has; anything else is a ``ValueError``, as is a dtype
        other than uint8.  Each result is uint8 codes of the same law, has its input's length and is ALIGNED with it: what
        ``enhance_wave(w, 8000, codec=codec)`` of a fresh one-utterance handle returns.  Recordings are padded with the law's silence code.
        ``atten_lim_db``: as in :meth:`enhance_many_atten`, None for no cap on any recording.  (A method of its own, like
        ``enhance_many_atten``: ``enhance_many`` keeps the signature it has, and refuses uint8 arrays.)  A stereo archive, ``[N_i, 2]``
        arrays: :meth:`enhance_many_channels` with ``codec``."""
        dc = self._dc(dc_mode)
        waves = [np.asarray(w) for w in waves]
        for w in waves:
            self._wave_format(w.dtype, rate, codec)
        self._wave_format(np.uint8, rate, codec)      # (an empty list: codec and rate are checked all the same)
        limits = None
        if atten_lim_db is not None:
            seq = list(atten_lim_db) if isinstance(atten_lim_db, (list, tuple, np.ndarray)) else [atten_lim_db] * len(waves)
            if len(seq) != len(waves):
                raise ValueError("atten_lim_db must be a scalar or one value per recording (%d), got %d" % (len(waves), len(seq)))
            limits = [atten_limit_from_db(d) for d in seq]
        return self._enhance_many_pcm(waves, dc, int(rate), limits, codec)

    def _slot_limits(self, block, limits, channels: int = 1):
        """The scheduler's hand-over of :meth:`enhance_many_atten`: the slots of ``block`` that take a new recording get its limit (with
        channels: every utterance of the slot's frame row)."""
        new = [] if limits is None else [(slot, limits[item]) for slot, item, _, _, reset_before in block if reset_before]
        if not new:
            return
        cur = self.atten_limit
        for slot, l in new:
            cur[slot * channels:(slot + 1) * channels] = l
        self.set_atten_limit(limit=cur)

    def _enhance_many(self, waves, dc_mode, rate, limits) -> List[np.ndarray]:
        dc = self._dc(dc_mode)
        if rate is not None:
            return self._enhance_many_pcm(waves, dc, rate, limits)
        waves = [np.ascontiguousarray(w, dtype=np.float32) for w in waves]
        if any(w.ndim != 1 for w in waves):
            raise ValueError("waves must be one-dimensional arrays")
        hops = [max(0, (len(w) - 256) // 256) for w in waves]
        outs = [np.zeros(len(w) + 256, np.float64) for w in waves]
        empty = np.zeros(0, np.float32)
        for block in plan_ragged_blocks(hops, self.utterances, self.max_frames):
            chunks = [empty] * self.utterances
            for slot, item, first, count, reset_before in block:
                if reset_before:
                    self.reset_utterance(slot)
                chunks[slot] = waves[item][first * 256:(first + count) * 256]
            self._slot_limits(block, limits)
            got = self._ragged_host(self._lib.nutls_enhance_block_ragged_host, chunks, 256, dc)
            for slot, item, first, count, _ in block:
                outs[item][first * 256:(first + count) * 256] = got[slot]
        return [o[256:] for o in outs]

    _PCM_RATES = (8000, 16000, 32000, 48000)

    def _enhance_many_pcm(self, waves, dc: int, rate, limits=None, codec=None, channels: int = 1) -> List[np.ndarray]:
        """:meth:`enhance_many` in the callers' format.  Every recording is padded with zeros to whole hops that cover ``N + lag`` samples,
        ``lag = pcm_hop_samples + pcm_delay_samples`` (the rule of :meth:`_wave_through_blocks`), and the lag is dropped from the front.
        ``codec`` (:meth:`enhance_many_codec`, which has checked dtype and rate): uint8 codes of that G.711 law, padded with its silence code."""
        waves = [np.asarray(w) for w in waves]
        if channels == 1:
            if any(w.ndim != 1 for w in waves):
                raise ValueError("waves must be one-dimensional arrays")
        elif any(w.ndim != 2 or w.shape[1] != channels for w in waves):
            raise ValueError("with channels=%r waves must be arrays [N,%r] of interleaved frames" % (channels, channels))
        names = {w.dtype.name for w in waves}
        if codec is None and (len(names) > 1 or not names <= {"float32", "int16"}):
            raise ValueError("with a rate, waves must all be int16 or all be float32 (uint8 G.711 codes: enhance_many_codec), got %s" % sorted(names))
        if isinstance(rate, bool) or not isinstance(rate, (int, np.integer)) or int(rate) not in self._PCM_RATES:
            raise ValueError("rate must be 8000, 16000, 32000 or 48000, got %r" % (rate,))
        if not waves:
            return []
        dtype = waves[0].dtype
        self.set_pcm_channels(channels)      # (ValueError: not 1, 2 or 4, or the handle's utterances are no multiple of it)
        self.set_pcm_format(int(rate), codec or dtype)
        S = self.pcm_hop_samples
        lag = S + self.pcm_delay_samples
        hops = [max(1, -(-(len(w) + lag) // S)) for w in waves]
        padded = []
        for w, n in zip(waves, hops):
            p = np.full((n * S,) + w.shape[1:], self.pcm_silence, dtype)
            p[:len(w)] = w
            padded.append(p)
        outs = [np.empty_like(p) for p in padded]
        empty = np.zeros((0,) + waves[0].shape[1:], dtype)
        rows = self.utterances // channels      # frame rows: the scheduler's slots
        for block in plan_ragged_blocks(hops, rows, self.max_frames):
            chunks = [empty] * rows
            for slot, item, first, count, reset_before in block:
                if reset_before:
                    for u in range(slot * channels, (slot + 1) * channels):
                        self.reset_utterance(u)
                chunks[slot] = padded[item][first * S:(first + count) * S]
            self._slot_limits(block, limits, channels)
            got = self._ragged_host(self._lib.nutls_enhance_block_pcm_ragged_host, chunks, S, dc, dtype=dtype, channels=channels)
            for slot, item, first, count, _ in block:
                outs[item][first * S:(first + count) * S] = got[slot]
        return [o[lag:lag + len(w)] for o, w in zip(outs, waves)]

    def debug_get(self, name: str, shape) -> np.ndarray:
        """Debug tensors of the handle, ``[utterances] + shape``: "phasor_block" (``shape = (n_hops, 257, 2)`` of the last analysed block)."""
        a = np.empty((self.utterances,) + tuple(shape), np.float32)
        _check(self._lib, self._lib.nutls_debug_get(self._h, name.encode(), _fptr(a), a.size))
        return a

    def state_get(self, name: str) -> np.ndarray:
        """Carried state tensor ``name`` of every utterance, ``[utterances, F, C]`` (``[utterances, 21]`` for h / c)."""
        d0, d1 = ctypes.c_int(), ctypes.c_int()
        for i in range(self._lib.nutls_state_count(self._h)):
            nm = ctypes.c_char_p()
            _check(self._lib, self._lib.nutls_state_info(self._h, i, ctypes.byref(nm), ctypes.byref(d0), ctypes.byref(d1)))
            if nm.value.decode() == name:
                a = np.empty((self.utterances, d0.value, d1.value), np.float32)
                _check(self._lib, self._lib.nutls_state_get(self._h, name.encode(), _fptr(a), a.size))
                return a.reshape(self.utterances, d0.value) if d1.value == 1 else a
        raise ValueError("unknown state tensor: %s" % name)

    def conv_launches(self) -> List[Tuple[str, str, int]]:
        """The conv launches of the block plan: (layer name, kind of ``CONV_KINDS``, f_out) in issue order; a block of n frames runs each
        with ``batch = utterances * n`` (``conv_dispatch``)."""
        return conv_launches(self._lib, self._h)

    def reset_utterance(self, u: int):
        """Zero the carried state (and the causal32 attention history) of utterance ``u``: a new utterance starts in that slot."""
        _check(self._lib, self._lib.nutls_reset(self._h, int(u)))

    def reset(self):
        _check(self._lib, self._lib.nutls_reset(self._h, -1))

    def close(self):
        if self._h:
            self._lib.nutls_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
