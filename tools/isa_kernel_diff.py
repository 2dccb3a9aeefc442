#!/usr/bin/env python3
"""Compare two assembly listings of one kernel file, kernel by kernel.

    hipcc <the Makefile's flags> --cuda-device-only -S csrc/fa_mfma_kernel.hip -o new.s      (the same on the parent tree: old.s)
    python tools/isa_kernel_diff.py old.s new.s

For every kernel symbol present in both listings the instruction text (instructions, inline-asm markers and block labels without the function's index in the file; no comments,
no directives) must be identical; kernels present in one listing only are listed with their register and scratch figures. Exit status 1
if a shared kernel differs. A change that adds a compile-time mode to a shared body uses it to show that no existing kernel moved.
"""
import re
import sys


def kernels(path):
    text = open(path).read()
    meta = {}
    for m in re.finditer(r"\.name:\s+(\S+)\n(?:.*\n)*?.*?\.private_segment_fixed_size:\s+(\d+)\n(?:.*\n)*?.*?\.sgpr_count:\s+(\d+)\n(?:.*\n)*?"
                         r".*?\.vgpr_count:\s+(\d+)", text):
        meta[m.group(1)] = dict(scratch=int(m.group(2)), sgpr=int(m.group(3)), vgpr=int(m.group(4)))
    out = {}
    for name in meta:
        start = re.search(r"^" + re.escape(name) + r":", text, re.M).start()
        end = text.index(".Lfunc_end", start)
        body = []
        for line in text[start:end].splitlines()[1:]:
            code = line.split(";")[0].strip() if not line.strip().startswith(";;#ASM") else line.strip()
            code = re.sub(r"\.LBB\d+_", ".LBB_", code)  # block labels carry the function's index in the file: not part of the code
            if code and not code.startswith("."):
                body.append(code)
            elif code.startswith(".LBB"):
                body.append(code)
        out[name] = body
    return out, meta


def main():
    old, old_meta = kernels(sys.argv[1])
    new, new_meta = kernels(sys.argv[2])
    shared = sorted(set(old) & set(new))
    moved = [n for n in shared if old[n] != new[n]]
    print(f"kernels: {len(old)} before, {len(new)} after, {len(shared)} in both")
    print(f"identical instruction text: {len(shared) - len(moved)} of {len(shared)} ({sum(len(old[n]) for n in shared)} instructions compared)")
    for n in moved:
        print("DIFFERS", n, len(old[n]), "->", len(new[n]), "instructions")
    for n in sorted(set(old) - set(new)):
        print("removed", n)
    for n in sorted(set(new) - set(old)):
        m = new_meta[n]
        print(f"added   {n}: {len(new[n])} instructions, {m['vgpr']} VGPR, {m['sgpr']} SGPR, {m['scratch']} B scratch")
    return 1 if moved else 0


if __name__ == "__main__":
    sys.exit(main())
