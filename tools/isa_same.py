#!/usr/bin/env python3
"""Has a change only MOVED kernels?  Compares the gfx950 machine code of two builds per mangled function name.

Usage:  isa_same.py <dir of the parent's *.o> <dir of the branch's *.o>        exit code 0 = the same code, 1 = not

Every device function of the parent must sit in exactly one object of the branch, with the same instruction stream -- after the padding
behind its end is dropped and the literal of a PC-relative address (s_getpc_b64, s_add_u32, s_addc_u32: the call of pf_flush) is masked --
and, for a kernel, the same registers, spills, scratch and static LDS in the code object's notes.
"""
import glob
import os
import re
import subprocess
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "motifscan_amd", "csrc"))
import check_isa  # noqa: E402

FIELDS = ("vgpr_count", "sgpr_spill_count", "vgpr_spill_count", "private_segment_fixed_size", "group_segment_fixed_size")


def normal(body):
    body = list(body)
    while body and (body[-1] == "..." or body[-1].startswith(("s_nop", "s_code_end"))):
        body.pop()
    for i, l in enumerate(body):
        if l.startswith(("s_add_u32", "s_addc_u32")) and any(p.startswith("s_getpc_b64") for p in body[max(i - 2, 0):i]):
            body[i] = re.sub(r"0x[0-9a-f]+$", "LIT", l)
    return body


def functions(objdir):
    """name -> [(object, normalised instructions, the notes' figures or None for a device function)]"""
    out = {}
    for obj in sorted(glob.glob(os.path.join(objdir, "*.o"))):
        try:
            funcs, notes = check_isa.disassemble(obj)
        except (check_isa.IsaCheckError, subprocess.CalledProcessError):
            continue                                                # host-only object
        for name, body in funcs.items():
            at = notes.find(".name:           " + name + "\n")
            num = None
            if at >= 0:                                             # a kernel's entry: .group_segment_fixed_size in front of .name, the rest behind it
                meta = notes[notes.rindex(".group_segment_fixed_size", 0, at):notes.index(".wavefront_size", at)]
                num = {f: int(re.search(rf"\.{f}:\s+(\d+)", meta).group(1)) for f in FIELDS}
            out.setdefault(name, []).append((os.path.basename(obj), normal(body), num))
    return out


def main(parent_dir, branch_dir):
    parent, branch = functions(parent_dir), functions(branch_dir)
    bad, library = 0, {}
    for name, was in sorted(parent.items(), key=lambda kv: (kv[1][0][0], kv[0])):
        now = branch.get(name, [])
        same = len(was) == 1 and len(now) == 1 and was[0][1:] == now[0][1:]
        bad += not same
        if same and "N2ms" not in name:                             # rocPRIM's kernels: one line per object
            library[was[0][0]] = library.get(was[0][0], 0) + 1
            continue
        figures = "/".join(str(v) for v in was[0][2].values()) if was[0][2] else "device function"
        print("same     " if same else "DIFFERENT", f"{was[0][0]:18s} -> {'+'.join(n[0] for n in now) or 'nowhere':18s} {len(was[0][1]):6d} instructions  {figures:18s}", name)
    for obj, n in sorted(library.items()):
        print("same     ", f"{obj:18s} -> {obj:18s} {n} functions outside namespace ms")
    print(f"{len(parent)} device functions of the parent, {bad} differ; {len(set(branch) - set(parent))} new in the branch  (figures: " + "/".join(FIELDS) + ")")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(*sys.argv[1:3]))
