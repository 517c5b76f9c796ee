"""Builds the HIP library in-tree:  csrc/*.hip, csrc/*.cpp  ->  libnutls_hip.so  (gfx950 only).

    python -m nunet_amd.build        (or: from nunet_amd.build import build; build())

hipcc cross-compiles without a GPU.  Every source is compiled to its own object (in parallel; the fused
kernel's 154 specialised ops take minutes, everything else seconds) and only re-compiled when it or a header
changed; the objects and the .so are git-ignored, the .so travels to the GPU box with the working-tree snapshot.
"""
from __future__ import annotations

import os
import re
import shutil
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
OBJ = os.path.join(HERE, "build")
LIB = os.path.join(HERE, "libnutls_hip.so")
SOURCES = ["fused_step.hip", "fused_step_g2.hip", "fused_step_g4.hip", "fused_step_hop.hip", "fused_step_g2_hop.hip", "fused_step_prof.hip", "fused_step_stop.hip", "fused_base.hip", "fused_base_prof.hip", "kernels.hip", "stft.hip", "stft_block.hip", "ragged.hip", "pcm.hip", "packet.hip", "channels.hip", "offline.hip", "weights.cpp", "fused_host.cpp", "engine.cpp", "api_stream.cpp", "api_block.cpp", "api_state.cpp", "api_profile.cpp", "api_pcm.cpp"]
if os.environ.get("NUTLS_BUILD_G4_PROF") == "1":      # developer knob: the profiling twin of the 4-stream packed kernel (12 more minutes)
    SOURCES.insert(3, "fused_step_g4_prof.hip")
# (fused_step_hop.hip / fused_step_g2_hop.hip: the hop builds of the one- and two-stream kernels, nutls_set_hop_fusion)
# (ragged.hip: the stage-in / commit kernels of the ragged block calls, nutls_process_block_ragged)
# (pcm.hip + api_pcm.cpp: the PCM gateway -- the callers' sample rate and sample type converted on the device, nutls_set_pcm_format)
# (packet.hip: packet mode of the PCM gateway -- the callers' 10 / 20 ms packets re-framed into hops on the device, nutls_set_pcm_packet)
# (channels.hip: channels of the PCM gateway -- interleaved 2- and 4-channel frames split into one row per stream and joined back, nutls_set_pcm_channels)
# (engine.cpp + api_stream.cpp / api_block.cpp / api_state.cpp / api_profile.cpp: the host engine and the entry points of the C ABI by family; they share engine.hpp)
# (headers are found by scanning the #include "..." lines of every source: _deps)
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Wall", "-Wno-unused-function"]
# The 4-stream packed kernel is one very large function, and LLVM's SDWA peephole (which only re-encodes sub-dword operand
# selects) spent over a third of its compile time on it: 24 minutes with it, 12 without, and it alone sets the length of a clean
# build.  It is compiled without the pass; its results are bit-identical (its step at 1024 streams ~1 % slower; no default plan).
SOURCE_FLAGS = {"fused_step_g4.hip": ["-mllvm", "-amdgpu-sdwa-peephole=0"], "fused_step_g4_prof.hip": ["-mllvm", "-amdgpu-sdwa-peephole=0"]}
LAST_BUILD = None      # what the last build() call did: {"mode", "rebuilt": [...], "sources", "seconds", "linked"}


def _hipcc() -> str:
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        raise RuntimeError("hipcc not found: cannot build libnutls_hip.so")
    return hipcc


def _obj(src: str) -> str:
    return os.path.join(OBJ, os.path.splitext(src)[0] + ".o")


_INC = re.compile(r'^\s*#\s*include\s+"([^"]+)"', re.M)


def _deps(path: str, seen=None) -> set:
    """The file and everything it includes with quotes, transitively (paths relative to the including file)."""
    seen = set() if seen is None else seen
    path = os.path.normpath(path)
    if path in seen or not os.path.exists(path):
        return seen
    seen.add(path)
    with open(path, "r", errors="replace") as f:
        for inc in _INC.findall(f.read()):
            _deps(os.path.join(os.path.dirname(path), inc), seen)
    return seen


def _flags(src: str) -> list:
    return FLAGS + SOURCE_FLAGS.get(src, [])


def _flags_stamp(src: str) -> str:
    """The flags an object was compiled with, beside it: an object compiled with other flags is stale too."""
    return _obj(src) + ".flags"


def _stale_sources(force: bool):
    out = []
    for s in SOURCES:
        o = _obj(s)
        dep = max(os.path.getmtime(d) for d in _deps(os.path.join(CSRC, s)))
        stamp = _flags_stamp(s)
        same_flags = os.path.exists(stamp) and open(stamp).read() == " ".join(_flags(s))
        if force or not os.path.exists(o) or os.path.getmtime(o) < dep or not same_flags:
            out.append(s)
    return out


def _compile(hipcc: str, src: str, verbose: bool):
    _run([hipcc] + _flags(src) + ["-c", os.path.join(CSRC, src), "-o", _obj(src)], verbose)
    with open(_flags_stamp(src), "w") as f:
        f.write(" ".join(_flags(src)))


def _run(cmd, verbose):
    if verbose:
        print(" ".join(cmd), flush=True)
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        sys.stderr.write(r.stdout + r.stderr)
        raise RuntimeError("hipcc failed: " + " ".join(cmd[-3:]))
    if verbose and (r.stdout or r.stderr):
        print(r.stdout + r.stderr)


def build(force: bool = False, verbose: bool = False) -> str:
    hipcc = _hipcc()
    os.makedirs(OBJ, exist_ok=True)
    todo = _stale_sources(force)
    only = os.environ.get("NUTLS_BUILD_ONLY")      # developer knob while iterating on one kernel: re-compile just these (stale objects of the others are linked as they are)
    if only:
        todo = [s for s in todo if s in only.split(",")]
    global LAST_BUILD
    if not todo and not only and os.path.exists(LIB) and all(os.path.getmtime(LIB) >= os.path.getmtime(_obj(s)) for s in SOURCES):
        LAST_BUILD = {"mode": "force" if force else "incremental", "rebuilt": [], "sources": len(SOURCES), "seconds": 0.0, "linked": False}
        print("nutls build: rebuilt 0 of %d sources (every object is newer than its source and headers), library up to date" % len(SOURCES), flush=True)
        return LIB
    import time
    t0 = time.time()
    # (the longest compiles first: the 4-stream packed kernel alone is about 12 minutes, the pool must not start it last)
    order = sorted(todo, key=lambda s: {"fused_step_g4.hip": 0, "fused_step_g4_prof.hip": 0, "fused_step_g2.hip": 1, "fused_step_g2_hop.hip": 1}.get(s, 2))
    with ThreadPoolExecutor(max_workers=6) as ex:
        list(ex.map(lambda s: _compile(hipcc, s, verbose), order))
    _run([hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", LIB] + [_obj(s) for s in SOURCES], verbose)
    LAST_BUILD = {"mode": "force" if force else "incremental", "rebuilt": list(todo), "sources": len(SOURCES), "seconds": round(time.time() - t0, 1), "linked": True}
    print("nutls build: rebuilt %d of %d sources (%s) and linked in %.0f s" % (len(todo), len(SOURCES), ", ".join(todo) or "-", time.time() - t0), flush=True)
    return LIB


if __name__ == "__main__":
    print(build(force="--force" in sys.argv, verbose=True))
