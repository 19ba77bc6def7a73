#!/usr/bin/env python3
"""tools/codeobj.py <lib.so> [kernel substring]: register / scratch / LDS figures of the gfx950 code objects inside an engine library
(the offload bundles are cut out by hand; llvm-readelf --notes prints the kernel descriptors' metadata).
tools/codeobj.py --sha256 <lib.so> [kernel substring]: one sha256 per gfx950 code object, in bundle order, and one per kernel's
machine code (the bytes of its symbol in .text) -- two builds with the same hashes run the same device code.  Reads nothing but <lib.so>."""
import hashlib
import re
import struct
import subprocess
import sys
import tempfile


def code_objects(data):
    """the gfx950 code objects of a library, one per HIP source (offload bundle), in bundle order"""
    i = data.find(b"__CLANG_OFFLOAD_BUNDLE__")
    while i >= 0:
        n = struct.unpack_from("<Q", data, i + 24)[0]
        off = i + 32
        for _ in range(n):
            o, s, tl = struct.unpack_from("<QQQ", data, off)
            off += 24
            if b"gfx950" in data[off:off + tl]:
                yield data[i + o:i + o + s]
            off += tl
        i = data.find(b"__CLANG_OFFLOAD_BUNDLE__", i + 24)


def kernel_text(co):
    """(name, machine code) of every kernel of a code object (ELF64, little endian): the functions that have a descriptor <name>.kd"""
    shoff, = struct.unpack_from("<Q", co, 0x28)
    shentsize, shnum = struct.unpack_from("<HH", co, 0x3A)
    sections = [struct.unpack_from("<IIQQQQIIQQ", co, shoff + k * shentsize) for k in range(shnum)]
    funcs, descriptors = [], set()
    for _, sh_type, _, _, sh_offset, sh_size, sh_link, _, _, sh_entsize in sections:
        if sh_type != 2:  # SHT_SYMTAB
            continue
        strtab = sections[sh_link][4]
        for p in range(sh_offset, sh_offset + sh_size, sh_entsize):
            st_name, st_info, _, st_shndx, st_value, st_size = struct.unpack_from("<IBBHQQ", co, p)
            name = co[strtab + st_name:co.index(b"\0", strtab + st_name)].decode()
            if name.endswith(".kd"):
                descriptors.add(name[:-3])
            elif st_info & 15 == 2 and 0 < st_shndx < shnum:  # STT_FUNC
                sec = sections[st_shndx]
                start = sec[4] + st_value - sec[3]
                funcs.append((name, co[start:start + st_size]))
    return [(name, code) for name, code in funcs if name in descriptors]


def print_sha256(data, want):
    for k, co in enumerate(code_objects(data)):
        print(f"code object {k}  {len(co):8d} B  {hashlib.sha256(co).hexdigest()}")
        for name, code in kernel_text(co):
            if want in name:
                print(f"  {name[:48]:48s} {len(code):7d} B  {hashlib.sha256(code).hexdigest()}")


def print_resources(data, want):
    out = ""
    for co in code_objects(data):
        with tempfile.NamedTemporaryFile(suffix=".co") as f:
            f.write(co)
            f.flush()
            out += subprocess.check_output(["/opt/rocm/lib/llvm/bin/llvm-readelf", "--notes", f.name], text=True)
    cur = {}
    rows = []
    for line in out.splitlines():
        m = re.match(r"\s*-?\s*\.(\w+):\s*(\S+)", line)
        if not m:
            continue
        k, v = m.groups()
        if k == "agpr_count" and cur.get("name"):
            rows.append(cur)
            cur = {}
        if k in ("agpr_count", "group_segment_fixed_size", "name", "private_segment_fixed_size", "sgpr_count", "sgpr_spill_count", "vgpr_count", "vgpr_spill_count"):
            cur[k] = v
    if cur.get("name"):
        rows.append(cur)
    for r in rows:
        if want in r.get("name", ""):
            print(f"{r['name'][:48]:48s} vgpr {r.get('vgpr_count'):>4s} (spill {r.get('vgpr_spill_count'):>3s})  sgpr {r.get('sgpr_count'):>4s} (spill {r.get('sgpr_spill_count'):>3s})  "
                  f"scratch {r.get('private_segment_fixed_size'):>4s} B  static LDS {r.get('group_segment_fixed_size'):>5s} B")


if __name__ == "__main__":
    args = [a for a in sys.argv[1:] if a != "--sha256"]
    data = open(args[0], "rb").read()
    want = args[1] if len(args) > 1 else ""
    (print_sha256 if "--sha256" in sys.argv[1:] else print_resources)(data, want)
