#!/usr/bin/env python3
"""Compare the gfx950 device code of two builds of one object file, kernel by kernel (no GPU needed): the check of a refactor that is meant to
leave kernels alone.  The code object is unbundled from the .hip_fatbin section, the bytes of every function symbol are cut out of .text, and the
resources of the kernels that differ (VGPRs, LDS bytes, scratch bytes) are read from the code object's metadata note.

    python tools/kernel_bytes_diff.py PARENT/mpc_hip.o mpc_benchmark_amd/csrc/mpc_hip.o

Prints the counts, every kernel that differs, appears or disappears with its resources on both sides, and exits 0 (it judges nothing: which
kernels may differ is the reader's call).  Needs llvm-objcopy, clang-offload-bundler and llvm-readelf of the ROCm toolchain (ROCM_PATH, default /opt/rocm).
"""
import os
import re
import struct
import subprocess
import sys
import tempfile

LLVM = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin")
TARGET = "hipv4-amdgcn-amd-amdhsa--gfx950"


def code_object(obj, tmp, tag):
    fat, co = os.path.join(tmp, tag + ".fat"), os.path.join(tmp, tag + ".co")
    subprocess.run([os.path.join(LLVM, "llvm-objcopy"), "--dump-section", ".hip_fatbin=" + fat, obj], check=True)
    subprocess.run([os.path.join(LLVM, "clang-offload-bundler"), "--unbundle", "--type=o", "--targets=" + TARGET, "--input=" + fat, "--output=" + co], check=True)
    return co


def functions(co):
    """{symbol: bytes} of the STT_FUNC symbols of an ELF64 little-endian code object."""
    d = open(co, "rb").read()
    shoff, = struct.unpack_from("<Q", d, 0x28)
    shentsize, shnum, _ = struct.unpack_from("<HHH", d, 0x3A)
    sec = [struct.unpack_from("<IIQQQQIIQQ", d, shoff + i * shentsize) for i in range(shnum)]
    out = {}
    for s in sec:
        if s[1] != 2:  # SHT_SYMTAB
            continue
        stroff = sec[s[6]][4]
        for o in range(s[4], s[4] + s[5], s[9]):
            name, info, _, shndx, value, size = struct.unpack_from("<IBBHQQ", d, o)
            if info & 0xF != 2 or shndx == 0 or shndx >= shnum:  # STT_FUNC, defined
                continue
            end = d.index(b"\0", stroff + name)
            start = sec[shndx][4] + value - sec[shndx][3]
            out[d[stroff + name:end].decode()] = d[start:start + size]
    return out


def resources(co):
    """{kernel: (vgprs, lds bytes, scratch bytes)} from the AMDGPU metadata note."""
    txt = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", co], check=True, capture_output=True, text=True).stdout
    out = {}
    for blk in re.split(r"\n\s+- \.agpr_count:", txt)[1:]:
        get = lambda key: int(re.search(r"\n\s+\.%s:\s+(\d+)" % key, blk).group(1))
        out[re.search(r"\n\s+\.name:\s+(\S+)", blk).group(1)] = (get("vgpr_count"), get("group_segment_fixed_size"), get("private_segment_fixed_size"))
    return out


def main(parent, change):
    with tempfile.TemporaryDirectory() as tmp:
        cp, cc = code_object(parent, tmp, "parent"), code_object(change, tmp, "change")
        fp, fc, rp, rc = functions(cp), functions(cc), resources(cp), resources(cc)
    both = sorted(set(fp) & set(fc))
    differ = [n for n in both if fp[n] != fc[n]]
    only_p, only_c = sorted(set(fp) - set(fc)), sorted(set(fc) - set(fp))
    print("function symbols: parent %d, change %d ; in both %d, byte for byte equal %d, differ %d ; only in parent %d, only in change %d"
          % (len(fp), len(fc), len(both), len(both) - len(differ), len(differ), len(only_p), len(only_c)))
    print(".text bytes of the functions: parent %d, change %d" % (sum(map(len, fp.values())), sum(map(len, fc.values()))))
    fmt = lambda r, n: "vgpr %3d lds %6d scratch %3d" % r[n] if n in r else "(not a kernel)"
    for what, names in (("differs", differ), ("only in parent", only_p), ("only in change", only_c)):
        for n in names:
            print("%-15s %s\n%17s%6s bytes  %s\n%17s%6s bytes  %s" % (what, n, "parent ", len(fp[n]) if n in fp else "-", fmt(rp, n) if n in fp else "",
                                                                    "change ", len(fc[n]) if n in fc else "-", fmt(rc, n) if n in fc else ""))


if __name__ == "__main__":
    main(*sys.argv[1:3])
