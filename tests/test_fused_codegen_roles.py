"""CPU: wave roles in the one-stream fused step kernel (build/fused_step.o, disassembled with ROCm's llvm-objdump).

tests/test_fused_codegen.py holds the kernel's arithmetic, registers and instruction total.  Held here, as upper bounds, what the scalar wave
guards (fused_step.hip role_block / finish_op) and the 24-bit row x pitch products (row_x_pitch) took out of the instruction stream -- and the
two counts a wave branch must not raise: the waits, and the full drains of the memory counter behind a join.  The counts of the kernel before
that change: 68 916 instructions, 3 875 s_waitcnt, 58 s_waitcnt vmcnt(0), 678 s_and_saveexec_b64, 272 v_mul_lo_u32, 3 315 s_nop; now 67 518,
3 751, 57, 428, 127, 3 270.  Skips when the object or the tools are absent (nothing was built)."""
import os
import re
import subprocess

import pytest

from test_fused_codegen import BUILD, _count, _device_code, _llvm, _meta

# before the change (device assembly of that source)
PARENT = {"instructions": 68916, "s_waitcnt": 3875, "vmcnt0": 58, "saveexec": 678, "mul_lo": 272, "s_nop": 3315}
# the kernel as it is now: upper bounds
NOW = {"instructions": 67518, "s_waitcnt": 3751, "vmcnt0": 57, "saveexec": 428, "mul_lo": 127, "s_nop": 3270}
# The v_mul_lo_u32 that remain, by their constant operand (each but `21` also costs the s_movk that holds it):
#   x 0x190 (68), x 0x310 (28), x 0x110 (1)   a row x a pitch of (n + 4) * 4 bytes, n = 96 / 192 / 64 channels, in conv_x16b outside the row-wise
#       epilogues: the lane's row of the B image (lane_b) and `K slice * positions + position` of the exchange store, whose K slice comes from the
#       scalar wave index (no known range);
#   x 21 (26)     LSTM ops: `tid / 21 * 21` of the (unit, K slice) split of the thread index (prefetch_w, lstm_op);
#   x 0x60 (4)    a row x a 96-byte pitch (the gate-weight rows of an LSTM thread, a 24-float state row).
# Gone: the 146 `position x OPB` products (x 0x90, x 0x110, x 0x210: the exchange buffer's row pitch) of x_epilogue / x_epilogue1 / x_sums, now
# v_mul_u32_u24 with the pitch as a literal (fused_step.hip row_x_pitch).  The thread index's range (`__builtin_assume(0 <= tid < 512)` behind
# run_op's pin) would take 61 more but brings back the 64-bit vector addresses that tests/test_fused_codegen.py::test_loads_use_the_scalar_base_form
# forbids (76 -> 518 v_lshl_add_u64 / v_add_co / v_addc): it was left out.


@pytest.fixture(scope="module")
def step_kernel(tmp_path_factory):
    tmp = str(tmp_path_factory.mktemp("codegen_roles"))
    if None in [_llvm(t) for t in ("llvm-objdump", "llvm-readelf")]:
        pytest.skip("ROCm's llvm-objdump / llvm-readelf not found")
    co = _device_code(os.path.join(BUILD, "fused_step.o"), tmp)
    if co is None:
        pytest.skip("build/fused_step.o (or the tools to unpack it) not present: nothing was built")
    dis = subprocess.run([_llvm("llvm-objdump"), "-d", co], check=True, capture_output=True, text=True).stdout
    body, inside = [], False
    for line in dis.splitlines():
        m = re.match(r"^[0-9a-f]+ <(\S+)>:", line)
        if m:
            inside = "nutls_fused_step_kernel" in m.group(1)
            continue
        if inside and re.match(r"^\s+[a-z_0-9]+(\s|$)", line):
            body.append(re.sub(r"\s*//.*$", "", line).strip())
    assert body, "kernel symbol not found in the disassembly"
    last = max(i for i, l in enumerate(body) if l.startswith("s_endpgm"))      # (behind it: padding)
    return body[:last + 1], _meta(co)


def _counts(body):
    return {"instructions": len(body), "s_waitcnt": len(_count(body, r"^s_waitcnt")), "vmcnt0": len(_count(body, r"^s_waitcnt vmcnt\(0\)")),
            "saveexec": len(_count(body, r"^s_and_saveexec_b64")), "mul_lo": len(_count(body, r"^v_mul_lo_u32")), "s_nop": len(_count(body, r"^s_nop"))}


@pytest.mark.parametrize("what", ["s_waitcnt", "vmcnt0"])
def test_recorded_bounds_are_not_above_the_parent(what):
    assert NOW[what] <= PARENT[what]


@pytest.mark.parametrize("what", ["saveexec", "mul_lo", "s_nop", "instructions"])
def test_recorded_bounds_are_below_the_parent(what):
    """Strictly fewer than before the change."""
    assert NOW[what] < PARENT[what], (what, NOW[what], PARENT[what])


@pytest.mark.parametrize("what", sorted(NOW))
def test_count_stays_at_or_below_its_bound(step_kernel, what):
    body, _ = step_kernel
    got = _counts(body)[what]
    assert got <= NOW[what], (what, got)


def test_wave_guards_are_scalar_branches(step_kernel):
    """The blocks of an op that belong to some waves only are entered through s_cmp + s_cbranch_scc on the wave index (56 such branches and
    584 s_cbranch_execz before the change)."""
    body, _ = step_kernel
    assert len(_count(body, r"^s_cbranch_scc")) >= 200
    assert len(_count(body, r"^s_cbranch_execz")) <= 366
