#!/usr/bin/env python
"""Registers, scratch and LDS of every kernel of a built libslhip.so, read from the code objects themselves.

    python tools/kernel_resources.py [path/to/libslhip.so] [--json OUT]

hipcc embeds one offload bundle per translation unit in the library's ``.hip_fatbin`` section; every gfx950
code object in it carries the AMDGPU metadata note with, per kernel, ``.sgpr_count``, ``.vgpr_count``,
``.private_segment_fixed_size`` (scratch bytes per lane) and ``.group_segment_fixed_size`` (static LDS bytes
per workgroup) - what ``-Rpass-analysis=kernel-resource-usage`` reports at compile time
(``tools/resource_summary.sh``: TotalSGPRs, VGPRs, AGPRs, ScratchSize, LDS Size) as the code object records it,
without compiling anything again.  ``.vgpr_count`` is the kernel's share of the unified register file: the
remark's VGPRs rounded up to a multiple of four (where the AGPRs begin) plus ``.agpr_count``; with no AGPRs it
is the remark's VGPRs (137 VGPRs and 8 AGPRs read 148; 110 and 0 read 110).
Needs ``llvm-readelf`` and ``llvm-objcopy`` of the ROCm toolchain; no GPU.

``resources(lib)`` -> ``{mangled kernel name: {"sgpr": .., "vgpr": .., "agpr": .., "scratch": .., "lds": ..}}``; a kernel
name compiled into several translation units (the per-dimension units) must carry the same figures in all.
"""

import json
import os
import re
import struct
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LLVM = os.environ.get("SL_LLVM_BIN", "/opt/rocm/llvm/bin")
MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"
FIELDS = {".sgpr_count": "sgpr", ".vgpr_count": "vgpr", ".agpr_count": "agpr", ".private_segment_fixed_size": "scratch",
          ".group_segment_fixed_size": "lds"}


def _code_objects(fatbin):
    """The gfx950 code objects of every uncompressed offload bundle in a ``.hip_fatbin`` section."""
    at = fatbin.find(MAGIC)
    while at >= 0:
        (count,) = struct.unpack_from("<Q", fatbin, at + len(MAGIC))
        pos = at + len(MAGIC) + 8
        for _ in range(count):
            offset, size, triple_size = struct.unpack_from("<QQQ", fatbin, pos)
            triple = fatbin[pos + 24:pos + 24 + triple_size].decode()
            pos += 24 + triple_size
            if "gfx950" in triple and size:
                yield fatbin[at + offset:at + offset + size]
        at = fatbin.find(MAGIC, at + len(MAGIC))


def _kernels_of(code_object, tmp):
    path = os.path.join(tmp, "kernel.co")
    with open(path, "wb") as handle:
        handle.write(code_object)
    notes = subprocess.check_output([os.path.join(LLVM, "llvm-readelf"), "--notes", path], text=True)
    # one list item per kernel at two spaces of indent, its keys (sorted by name) at four
    out, entry = {}, None
    for line in notes.splitlines():
        match = re.match(r"  (- |  )(\.[a-z_]+):\s*(\S.*)?$", line)
        if not match:
            continue
        if match.group(1) == "- ":
            entry = {}
        if entry is None:
            continue
        key, value = match.group(2), (match.group(3) or "").strip()
        if key == ".symbol" and value.strip("'\"").endswith(".kd"):
            out[value.strip("'\"")[:-3]] = entry
        elif key in FIELDS and value.isdigit():
            entry[FIELDS[key]] = int(value)
    return {k: v for k, v in out.items() if len(v) == len(FIELDS)}


def resources(lib=None):
    lib = lib or os.path.join(ROOT, "safe_learning_amd", "libslhip.so")
    with tempfile.TemporaryDirectory() as tmp:
        section = os.path.join(tmp, "fatbin")
        subprocess.check_call([os.path.join(LLVM, "llvm-objcopy"), "-O", "binary", "--only-section=.hip_fatbin", lib,
                               section])
        with open(section, "rb") as handle:
            fatbin = handle.read()
        if MAGIC not in fatbin:
            raise RuntimeError("%s: no uncompressed offload bundle in .hip_fatbin" % lib)
        found = {}
        for code_object in _code_objects(fatbin):
            for name, entry in _kernels_of(code_object, tmp).items():
                if name in found and found[name] != entry:
                    raise RuntimeError("%s: two code objects disagree on %s: %r / %r" % (lib, name, found[name], entry))
                found[name] = entry
    return found


def main(argv):
    json_out = argv[argv.index("--json") + 1] if "--json" in argv else None
    args = [a for a in argv if not a.startswith("--") and a != json_out]
    table = resources(args[0] if args else None)
    if "--json" in argv:
        out = json_out
        with open(out, "w") as handle:
            json.dump(table, handle, indent=0, sort_keys=True)
            handle.write("\n")
        print("wrote %s: %d kernels" % (out, len(table)))
        return
    for name in sorted(table):
        e = table[name]
        print("%-100s SGPRs %3d  VGPRs %3d (AGPRs %3d)  scratch %5d  LDS %6d"
              % (name, e["sgpr"], e["vgpr"], e["agpr"], e["scratch"], e["lds"]))


if __name__ == "__main__":
    main(sys.argv[1:])
