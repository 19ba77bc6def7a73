#!/usr/bin/env python3
"""tools/asm_loops.py <file.s> <kernel symbol> [min instructions]: the loops of one kernel in the device assembly that
`hipcc -S --cuda-device-only` (with the flags of mvskit_amd/build.py) writes for a HIP source: for every backward branch the span from
its target label to the branch, with the instructions in it and how many of them are RELOADS of spilled scalars, the algorithm's own
lane BROADCASTS, v_writelane (saves of spilled scalars), scalar loads or scratch accesses.  A spill register is a VGPR that some
v_writelane_b32 of the kernel writes (the source has no writelane of its own: every one is the register allocator's); a v_readlane_b32
from such a register is a reload, from any other register a broadcast of the algorithm (rli / rlf, the wave butterflies).
The refinement's step loops are the spans of ~1400 (one candidate) and ~1570 (two candidates) instructions; the loops nested in them
(the view loops) are listed after them with a deeper indent.
tools/asm_loops.py --summary <file.s> <kernel symbol>: the kernel's totals alone, one line."""
import re
import sys


def kernel_instructions(path, kernel):
    """the instructions of a kernel in order, and label -> index of the next instruction"""
    lines = open(path).read().splitlines()
    begin = next(k for k, ln in enumerate(lines) if ln.startswith(kernel + ":"))
    end = next(k for k in range(begin, len(lines)) if lines[k].startswith(".Lfunc_end"))
    labels, instr = {}, []
    for ln in lines[begin:end]:
        s = ln.split(";")[0].strip()
        m = re.match(r"^(\.LBB\w+):", s)
        if m:
            labels[m.group(1)] = len(instr)
        elif s and not s.startswith(".") and not s.endswith(":"):
            instr.append(s)
    return instr, labels


def spill_registers(instr):
    """the VGPRs that hold spilled scalars: the destinations of the kernel's v_writelane_b32"""
    regs = set()
    for s in instr:
        m = re.match(r"^v_writelane_b32\s+(v\d+)", s)
        if m:
            regs.add(m.group(1))
    return regs


def counts(span, spill):
    c = {"n": len(span), "vector": 0, "reload": 0, "bcast": 0, "writelane": 0, "sload": 0, "scratch": 0, "ds_add": 0, "s_nop": 0}
    for s in span:
        if s.startswith(("v_", "ds_", "global_", "flat_", "scratch_", "buffer_")):
            c["vector"] += 1
        m = re.match(r"^v_readlane_b32\s+\S+\s+(v\d+)", s)
        if m:
            c["reload" if m.group(1) in spill else "bcast"] += 1
        elif s.startswith("v_writelane"):
            c["writelane"] += 1
        elif s.startswith(("s_load_", "s_buffer_load_")):
            c["sload"] += 1
        elif s.startswith("scratch_"):
            c["scratch"] += 1
        elif s.startswith("ds_add"):
            c["ds_add"] += 1
        elif s.startswith("s_nop"):
            c["s_nop"] += 1
    return c


def main():
    args = [a for a in sys.argv[1:] if a != "--summary"]
    path, kernel = args[0], args[1]
    floor = int(args[2]) if len(args) > 2 else 300
    instr, labels = kernel_instructions(path, kernel)
    spill = spill_registers(instr)
    t = counts(instr, spill)
    regs = " ".join(sorted(spill, key=lambda r: int(r[1:]))) or "none"
    print(f"{kernel}: {t['n']} instructions, {t['vector']} vector, {t['reload'] + t['bcast']} v_readlane ({t['reload']} reloads of spilled scalars, "
          f"{t['bcast']} broadcasts), {t['writelane']} v_writelane into {regs}, {t['sload']} scalar loads, {t['s_nop']} s_nop")
    if "--summary" in sys.argv[1:]:
        return
    loops = []
    for k, s in enumerate(instr):
        m = re.match(r"^s_c?branch\w*\s+(\.LBB\w+)", s)
        if m and m.group(1) in labels and labels[m.group(1)] <= k:
            loops.append((labels[m.group(1)], k, m.group(1)))
    loops.sort(key=lambda t: (t[0], -t[1]))
    for a, b, name in loops:
        if b - a + 1 < floor:
            continue
        depth = sum(1 for a2, b2, _ in loops if a2 <= a and b <= b2 and (a2, b2) != (a, b))
        c = counts(instr[a:b + 1], spill)
        print(f"{'  ' * depth}{name:12s} {c['n']:6d} instructions  reload {c['reload']:4d}  broadcast {c['bcast']:4d}  v_writelane {c['writelane']:4d}"
              f"  s_load {c['sload']:3d}  scratch {c['scratch']:3d}  ds_add {c['ds_add']:3d}")


if __name__ == "__main__":
    main()
