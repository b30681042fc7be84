#!/usr/bin/env python3
"""Mandatory post-compile check of the pre-filter's gfx950 code object.

Usage:  check_isa.py <object>        exit code 0 = the object may be linked, 1 = it may not

The Makefile runs this right after ms_kernels.o is compiled and refuses to link the library from an object that fails;
tests/test_host_cabi.py calls check() on the object the shipped library was linked from.  Checked, for each of the three
instantiations of prefilter_f6_kernel (<2, parked>, <2, dense>, <4, parked>):

  * <= 128 vector registers (four waves per SIMD);
  * in the narrow kernels (<2, *>: every JASPAR-like set runs on them) no spilled register, scalar or vector, and no scratch memory at all
    (a spill in a pass's set-up is reloaded in front of the sequence prefetch, behind a wait that exposes the loads' latency; the rule
    from before, no scratch traffic between the first and the last matrix instruction, stays and follows from this one).
The wide kernel (<4, parked>) may spill.
"""
import os
import re
import shutil
import subprocess
import sys
import tempfile

OBJDUMP = "/opt/rocm/lib/llvm/bin/llvm-objdump"
READELF = "/opt/rocm/lib/llvm/bin/llvm-readelf"
N_KERNELS = 3


class IsaCheckError(AssertionError):
    pass


def tools_present():
    return os.path.exists(OBJDUMP) and os.path.exists(READELF)


def _need(cond, *what):
    if not cond:
        raise IsaCheckError(" ".join(str(w) for w in what))


def disassemble(obj):
    """-> (funcs: name -> [instruction lines], notes text) of the gfx950 code object inside the host object `obj`."""
    with tempfile.TemporaryDirectory() as tmp:
        shutil.copy(obj, os.path.join(tmp, "k.o"))
        subprocess.run([OBJDUMP, "--offloading", "k.o"], cwd=tmp, check=True, capture_output=True)
        co = [f for f in os.listdir(tmp) if "gfx950" in f]
        _need(len(co) == 1, "expected one gfx950 code object in", obj, "found", co)
        asm = subprocess.run([OBJDUMP, "-d", co[0]], cwd=tmp, check=True, capture_output=True, text=True).stdout
        notes = subprocess.run([READELF, "--notes", co[0]], cwd=tmp, check=True, capture_output=True, text=True).stdout
    funcs, name = {}, None
    for line in asm.splitlines():
        m = re.match(r"^[0-9a-f]+ <(\S+)>:", line)
        if m:
            name = m.group(1)
            funcs[name] = []
        elif name and line.startswith("\t"):
            funcs[name].append(line.split("//")[0].strip())
    return funcs, notes


def check_code(funcs, notes):
    """The rules on a disassembled object (disassemble's result).  Raises IsaCheckError with the first violated rule; returns a short
    summary string otherwise."""
    kernels = [k for k in funcs if "prefilter_f6_kernel" in k]
    _need(len(kernels) == N_KERNELS, f"expected {N_KERNELS} instantiations of prefilter_f6_kernel (<2|4 k-blocks> x <parked | dense>, no wide dense), found",
          len(kernels))
    summary = []
    for k in kernels:
        meta = notes[notes.index(".name:           " + k + "\n"):]
        meta = meta[:meta.index(".wavefront_size")]
        num = {f: int(re.search(rf"\.{f}:\s+(\d+)", meta).group(1)) for f in ("vgpr_count", "sgpr_spill_count", "vgpr_spill_count", "private_segment_fixed_size")}
        _need(num["vgpr_count"] <= 128, k, "uses more than 128 vector registers:", num)
        body = funcs[k]
        mf = [i for i, l in enumerate(body) if l.startswith("v_mfma")]
        _need(len(mf) >= 12, k, "holds only", len(mf), "matrix instructions")
        if "ILi2E" in k:                                            # the double-pass kernels (plans without a wide tile)
            _need(num["sgpr_spill_count"] == 0 and num["vgpr_spill_count"] == 0 and num["private_segment_fixed_size"] == 0, k, "spills:", num)
            _need(not [l for l in body[mf[0]:mf[-1] + 1] if l.startswith("scratch_")], k, "spill traffic inside the pass body")
        summary.append(f"{k[k.index('ILi'):][:8]}: {num['vgpr_count']} vgprs, {num['vgpr_spill_count']} spilled")
    return "; ".join(summary)


def check(obj):
    """check_code on the object file `obj`."""
    return check_code(*disassemble(obj))


def main(argv):
    if len(argv) < 2:
        print(__doc__)
        return 2
    if not tools_present():
        print(f"check_isa: {OBJDUMP} / {READELF} not found -- the object CANNOT be verified; refusing (set MS_SKIP_ISA_CHECK=1 to link anyway)", file=sys.stderr)
        return 0 if os.environ.get("MS_SKIP_ISA_CHECK") == "1" else 1
    try:
        print("check_isa:", os.path.basename(argv[1]), "ok --", check(argv[1]))
        return 0
    except IsaCheckError as e:
        print("check_isa: FAILED --", e, file=sys.stderr)
        return 1


if __name__ == "__main__":
    sys.exit(main(sys.argv))
