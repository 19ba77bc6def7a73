#!/usr/bin/env python3
"""tools/asm_loops.py <file.s> <kernel symbol> [min instructions]: the loops of one kernel in the device assembly that
`hipcc -S --cuda-device-only` (with the flags of mvskit_amd/build.py) writes for a HIP source: for every backward branch the span from
its target label to the branch, with the instructions in it and how many of them are v_readlane / v_writelane (reloads and saves of
scalars spilled to vector lanes) or scratch accesses.  The refinement's step loops are the spans of ~1400 (one candidate) and ~1570
(two candidates) instructions; the loops nested in them (the view loops) are listed after them with a deeper indent."""
import re
import sys


def main():
    path, kernel = sys.argv[1], sys.argv[2]
    floor = int(sys.argv[3]) if len(sys.argv) > 3 else 300
    lines = open(path).read().splitlines()
    begin = next(k for k, ln in enumerate(lines) if ln.startswith(kernel + ":"))
    end = next(k for k in range(begin, len(lines)) if lines[k].startswith(".Lfunc_end"))
    body = lines[begin:end]
    labels, instr = {}, []  # label -> index of the next instruction; the instructions in order
    for ln in body:
        s = ln.split(";")[0].strip()
        m = re.match(r"^(\.LBB\w+):", s)
        if m:
            labels[m.group(1)] = len(instr)
        elif s and not s.startswith(".") and not s.endswith(":"):
            instr.append(s)
    loops = []
    for k, s in enumerate(instr):
        m = re.match(r"^s_c?branch\w*\s+(\.LBB\w+)", s)
        if m and m.group(1) in labels and labels[m.group(1)] <= k:
            loops.append((labels[m.group(1)], k, m.group(1)))
    loops.sort(key=lambda t: (t[0], -t[1]))
    print(f"{kernel}: {len(instr)} instructions, {sum('v_readlane' in s for s in instr)} v_readlane, {sum('v_writelane' in s for s in instr)} v_writelane")
    for a, b, name in loops:
        if b - a + 1 < floor:
            continue
        depth = sum(1 for a2, b2, _ in loops if a2 <= a and b <= b2 and (a2, b2) != (a, b))
        span = instr[a:b + 1]
        print(f"{'  ' * depth}{name:12s} {len(span):6d} instructions  v_readlane {sum('v_readlane' in s for s in span):4d}  v_writelane {sum('v_writelane' in s for s in span):4d}"
              f"  scratch {sum(s.startswith('scratch_') for s in span):3d}  ds_add {sum(s.startswith('ds_add') for s in span):3d}")


if __name__ == "__main__":
    main()
