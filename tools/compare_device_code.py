"""Is the device code of two builds the same, kernel by kernel?  (A host-side refactor must leave
every kernel's instructions and its kernel descriptor alone; whole listings differ anyway: the
kernels come out in another order, and the function ordinal n of the .LBBn_m labels moves with it.)

    python tools/compare_device_code.py --listings <source tree> <out dir>    # once per build
    python tools/compare_device_code.py <out dir A> <out dir B>

--listings compiles the gfx950 assembly of every translation unit of <source tree> (its
safe_learning_amd/_build.py names the units; the flags are those of _build.build) into
<out dir>/<unit>/<unit>.s.  The comparison keys every kernel on its mangled name and compares the
instruction text (';' comments dropped, the inline-asm markers kept, the function ordinal of local
labels replaced) and the .amdhsa_kernel ... .end_amdhsa_kernel block.  It prints per-unit counts and
every kernel that differs or exists on one side only; the exit status is 1 if there is one.
"""
import glob
import importlib.util
import os
import re
import subprocess
import sys

LOCAL_LABEL = re.compile(r'(\.L[A-Za-z_]*?)\d+(_\d+)?\b')


def emit_listings(tree, out, jobs=8):
    spec = importlib.util.spec_from_file_location("_sl_build", os.path.join(tree, "safe_learning_amd", "_build.py"))
    build = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(build)
    csrc = os.path.join(tree, "safe_learning_amd", "csrc")
    flags = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fPIC", "-fvisibility=hidden",
             "-I" + os.path.join(tree, "include"), "-I" + csrc, "--cuda-device-only", "-S"]
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    pending = [(stem, src, [f for f in extra if not f.startswith("-save-temps")]) for stem, src, extra in build.UNITS]
    running, failed = [], False
    while pending or running:
        while pending and len(running) < jobs:
            stem, src, extra = pending.pop(0)
            os.makedirs(os.path.join(out, stem), exist_ok=True)
            cmd = [hipcc] + flags + extra + [os.path.join(csrc, src), "-o", os.path.join(out, stem, stem + ".s")]
            running.append((stem, subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)))
        stem, proc = running.pop(0)
        text, _ = proc.communicate()
        if proc.returncode != 0:
            sys.stderr.write(text)
            failed = True
    if failed:
        raise SystemExit("hipcc failed")


def normalise(line):
    """One listing line as compared: None for a line that carries nothing."""
    if ";;#ASM" in line:                          # inline-asm markers: part of what the kernel is
        return line.strip()
    line = line.split(";", 1)[0].strip()
    return LOCAL_LABEL.sub(lambda m: m.group(1) + "n" + (m.group(2) or ""), line) or None


def kernels_of(listing):
    """{mangled name: (instruction lines, descriptor lines)} of the kernels of one listing.  (The
    descriptor block sits between a function's last instruction and its .Lfunc_end label.)"""
    bodies, descriptors, name, body, desc = {}, {}, None, None, None
    for line in open(listing):
        start = re.match(r'^([A-Za-z_$][\w$.]*):', line)
        if desc is not None:
            if line.strip() == ".end_amdhsa_kernel":
                descriptors[kernel], desc = desc, None
            elif normalise(line):
                desc.append(normalise(line))
        elif line.strip().startswith(".amdhsa_kernel "):
            kernel, desc = line.split()[1], []
        elif body is None and start:                                # a function's label
            name, body = start.group(1), []
        elif body is not None and re.match(r'^\.Lfunc_end\d+:', line):
            bodies[name], body = body, None
        elif body is not None and normalise(line):
            body.append(normalise(line))
    return {k: (bodies.get(k), descriptors[k]) for k in descriptors}


def compare(dir_a, dir_b):
    units = sorted(set(os.listdir(dir_a)) | set(os.listdir(dir_b)))
    total_a = total_b = bad = 0
    for unit in units:
        sides = []
        for d in (dir_a, dir_b):
            found = glob.glob(os.path.join(d, unit, "*.s"))
            found = [f for f in found if "gfx950" in f or os.path.basename(f) == unit + ".s"]
            sides.append(kernels_of(found[0]) if found else None)
        if sides[0] is None or sides[1] is None:
            print("%-18s listing missing in %s" % (unit, dir_a if sides[0] is None else dir_b))
            bad += 1
            continue
        a, b = sides
        total_a += len(a)
        total_b += len(b)
        differing = [k for k in sorted(set(a) & set(b)) if a[k] != b[k]]
        only_a, only_b = sorted(set(a) - set(b)), sorted(set(b) - set(a))
        print("%-18s %4d / %4d kernels, %d differ, %d / %d on one side only"
              % (unit, len(a), len(b), len(differing), len(only_a), len(only_b)))
        for k in differing:
            what = [w for w, i in (("instructions", 0), ("descriptor", 1)) if a[k][i] != b[k][i]]
            print("    differs (%s): %s" % (", ".join(what), k))
        for k in only_a:
            print("    only in %s: %s" % (dir_a, k))
        for k in only_b:
            print("    only in %s: %s" % (dir_b, k))
        bad += len(differing) + len(only_a) + len(only_b)
    print("total: %d / %d kernels, %s" % (total_a, total_b, "identical" if not bad else "%d problem(s)" % bad))
    return 1 if bad else 0


if __name__ == "__main__":
    if len(sys.argv) == 4 and sys.argv[1] == "--listings":
        emit_listings(sys.argv[2], sys.argv[3])
    elif len(sys.argv) == 3:
        sys.exit(compare(sys.argv[1], sys.argv[2]))
    else:
        sys.exit(__doc__)
