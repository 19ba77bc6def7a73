"""CPU-side checks of the C-ABI library: it loads, exports every symbol include/mvskit_engine.h declares,
and refuses to run without a GPU (no compute calls here)."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from mvskit_amd import abi, build, engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    build.build_engine()
    return engine.load_library()


def test_header_symbols_are_exported(lib):
    hdr = open(os.path.join(ROOT, "include", "mvskit_engine.h")).read()
    declared = set(re.findall(r"\b(mvs_[a-z_]+)\s*\(", hdr))
    declared -= {"mvs_engine"}  # the opaque struct name
    assert declared == set(engine.EXPORTS), declared ^ set(engine.EXPORTS)
    for name in declared:
        assert hasattr(lib, name), name
    status = {k: int(v) for k, v in re.findall(r"\b(MVS_OK|MVS_ERR_[A-Z_]+) = (-?\d+)", re.search(r"typedef enum mvs_status \{(.*?)\}", hdr, re.S).group(1))}
    assert len(status) == 6 and status == {k: getattr(engine, k) for k in status}, status


def test_record_layouts_match_header():
    assert engine.PATCH_DTYPE.itemsize == 128
    assert engine.PATCH_DTYPE.fields["images"][1] == 64 and engine.PATCH_DTYPE.fields["vimages"][1] == 96
    assert C.sizeof(engine.Counters) == 80
    assert C.sizeof(engine.Config) == 96


def test_default_config_follows_option_defaults(lib):
    c = engine.Config()
    lib.mvs_default_config(C.byref(c))
    # Option::Option, pmmvps/option.cpp:19-33
    assert (c.level, c.csize, c.wsize, c.minImageNum) == (1, 2, 7, 3)
    assert abs(c.nccThreshold - 0.7) < 1e-7 and abs(c.maxAngleThreshold - np.float32(10 * np.pi / 180)) < 1e-7
    assert abs(c.quadThreshold - 2.5) < 1e-7 and c.max_propag == 2


def test_create_rejects_bad_config_and_missing_gpu(lib):
    c = engine.Config()
    lib.mvs_default_config(C.byref(c))
    h = C.c_void_p()
    c.nviews = 0
    assert lib.mvs_engine_create(C.byref(c), C.byref(h)) == -1  # MVS_ERR_ARG
    c.nviews = 3
    c.wsize = 9
    assert lib.mvs_engine_create(C.byref(c), C.byref(h)) == -1
    if lib.mvs_device_count() == 0:
        c.wsize = 7
        assert lib.mvs_engine_create(C.byref(c), C.byref(h)) == -5  # MVS_ERR_NO_DEVICE: no CPU fallback
        assert b"no HIP device" in lib.mvs_last_error()
        with pytest.raises(engine.EngineError):
            engine.Engine(3)


@pytest.mark.parametrize("cap", [16, 32, 64])
def test_every_library_exports_the_same_abi(cap):
    """libmvskit_engine_cap32.so / _cap64.so = the same sources built with -DMVS_LISTCAP=32 / 64 (view lists of up to 32 / 64 entries):
    each exports every entry point, and load_library has given each the table's types."""
    build.build_engine(cap=cap)
    L = engine.load_library(cap=cap)
    for name, (restype, argtypes) in abi.SIGNATURES.items():
        assert hasattr(L, name), name
        fn = getattr(L, name)
        assert fn.restype is restype and fn.argtypes == argtypes, name
    assert L.mvs_list_cap() == cap and L.mvs_patch_bytes() == (192 if cap == 64 else 128)


def _header():
    """include/mvskit_engine.h without its comments"""
    return re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "mvskit_engine.h")).read(), flags=re.S)


def _header_structs():
    """{name: [field names]} of every `typedef struct name { ... } name;` of the header, in its order"""
    out = {}
    for name, body in re.findall(r"typedef\s+struct\s+(mvs_\w+)\s*\{(.*?)\}\s*\1\s*;", _header(), re.S):
        decls = [d for d in (d.strip() for d in body.split(";")) if d]  # `int32_t width, height`, `float P[12]`, `const uint8_t* rgb`
        out[name] = [re.search(r"(\w+)\s*(?:\[[^\]]*\])?$", part.strip()).group(1) for d in decls for part in d.split(",")]
    return out


def test_structs_table_covers_the_header():
    assert set(_header_structs()) - {"mvs_patch", "mvs_fused_point"} == set(abi.STRUCTS)  # those two are numpy dtypes
    assert len(set(abi.STRUCTS.values())) == len(abi.STRUCTS) == 18


def test_binding_signatures_match_header():
    """Every prototype of the header against abi.SIGNATURES: the same names in the same order, and at every position the ctypes class of
    the C type -- a count or a pointer in the wrong slot would corrupt memory, not fail a build."""
    protos = re.findall(r"\b(const\s+char\s*\*|int|void)\s+(mvs_\w+)\s*\(([^()]*)\)\s*;", _header())
    assert [name for _, name, _ in protos] == list(abi.SIGNATURES)
    assert len(protos) == 73 and engine.EXPORTS == list(abi.SIGNATURES)
    scalars = {"int": C.c_int, "int64_t": C.c_int64, "float": C.c_float}
    restypes = {"int": C.c_int, "void": None}
    pointees = {**scalars, **abi.STRUCTS, "mvs_engine*": C.c_void_p}
    for ret, name, params in protos:
        restype, argtypes = abi.SIGNATURES[name]
        assert restype is restypes.get(ret, C.c_char_p), name
        params = [" ".join(p.split()) for p in params.split(",")]
        if params == ["void"]:
            params = []
        assert len(params) == len(argtypes), name
        for k, (p, t) in enumerate(zip(params, argtypes)):
            where = f"{name}, parameter {k} ({p})"
            if "*" in p or "[" in p:  # `int64_t out[6]` is a pointer
                if isinstance(t, type) and issubclass(t, C._Pointer):  # a POINTER(...) points at what the header names
                    p = p.replace("const ", "")
                    pointee = p.split(" ")[0] if "[" in p else p[:p.rindex("*")].strip()
                    assert pointee in pointees and t._type_ is pointees[pointee], where
                else:
                    assert t in (C.c_void_p, C.c_char_p), where
            else:
                ctype, _ = p.rsplit(" ", 1)
                assert ctype in scalars and t is scalars[ctype], where


def test_struct_layouts_match_header(tmp_path):
    """sizeof and every offsetof of the header's structs, as the host C compiler lays them out, against the ctypes classes of abi.STRUCTS,
    position by position (names are not compared: the binding says `lam` where the header says `lambda`)."""
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    if cc is None:
        pytest.skip("no C compiler")
    fields = _header_structs()
    lines = ["#include <stddef.h>", "#include <stdio.h>", '#include "mvskit_engine.h"', "int main(void) {"]
    for name in abi.STRUCTS:
        lines.append(f'    printf("{name} %zu", sizeof({name}));')
        lines += [f'    printf(" %zu:%zu", offsetof({name}, {f}), sizeof((({name}*)0)->{f}));' for f in fields[name]]
        lines.append('    printf("\\n");')
    lines += ["    return 0;", "}"]
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines) + "\n")
    subprocess.check_call([cc, "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    seen = {}
    for line in subprocess.check_output([str(exe)], text=True).splitlines():
        name, size, *offs = line.split()
        seen[name] = (int(size), [tuple(int(x) for x in o.split(":")) for o in offs])
    assert list(seen) == list(abi.STRUCTS)
    for name, cls in abi.STRUCTS.items():
        mine = (C.sizeof(cls), [(getattr(cls, f).offset, getattr(cls, f).size) for f, _ in cls._fields_])
        assert len(mine[1]) == len(fields[name]), name
        assert mine == seen[name], (name, mine, seen[name])
    assert seen["mvs_config"][0] == 96 and seen["mvs_volume"][0] == seen["mvs_timing"][0] == 40 and seen["mvs_filter_stats"][0] == 104


def test_struct_sizes_of_the_binding():
    # mvs_timing: 3 floats, int32, float, (pad), 2 int64; mvs_filter_stats: 6 floats + 10 int64
    assert C.sizeof(engine.Timing) == 40
    assert C.sizeof(engine.FilterStats) == 24 + 10 * 8


def test_loopback_transport_exports_what_the_engine_binds():
    """tests/loopback_ccl (the shared-memory stand-in for RCCL that lets several engine ranks share the one GPU of a test box)
    must export exactly the eight entry points mvs_engine_comm.cpp binds through MVS_CCL_LIBRARY."""
    d = os.path.join(os.path.dirname(os.path.abspath(__file__)), "loopback_ccl")
    subprocess.check_call(["make", "-C", d, "-s"])
    out = subprocess.check_output(["nm", "-D", "--defined-only", os.path.join(d, "_build", "libloopback_ccl.so")], text=True)
    have = {line.split()[-1] for line in out.splitlines() if " T " in line}
    want = {"ncclGetUniqueId", "ncclCommInitRank", "ncclCommDestroy", "ncclAllGather", "ncclBroadcast", "ncclGroupStart", "ncclGroupEnd", "ncclGetErrorString"}
    assert want <= have
    src = open(os.path.join(os.path.dirname(d), "..", "mvskit_amd", "csrc", "mvs_engine_comm.cpp")).read()
    for name in want:
        assert f'"{name}"' in src, name
