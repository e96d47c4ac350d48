"""g++ builds of the host sources under tests/hostsim, for the host tests: a stand-alone program (plain, or
under the address and undefined-behaviour sanitizers: a program of its own, run directly) or a shared library
for ctypes.  Every test passes the flags of its own compile line; the output goes where the test says
(pytest's temporary directories), never into the source tree."""

import ctypes
import os
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
API = "-I" + os.path.join(ROOT, "include")                                 # sl_hip.h
CSRC = "-I" + os.path.join(ROOT, "safe_learning_amd", "csrc")              # the engine's headers
SHIM_FLAGS = ["-O2", "-std=c++17", "-ffp-contract=off", API, CSRC]         # the per-cell / per-point shims
SIM_FLAGS = ["-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", CSRC]      # the bookkeeping simulators (+ -O1 / -O2)
SANITIZERS = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]


def _command(source, out, flags):
    return ["g++"] + list(flags) + ["-o", out, os.path.join(ROOT, "tests", "hostsim", source)]


def program(source, out_dir, flags, sanitize=False):
    """tests/hostsim/<source> as a program in ``out_dir`` -> its path."""
    out = os.path.join(str(out_dir), os.path.splitext(source)[0] + ("_san" if sanitize else ""))
    subprocess.check_call(_command(source, out, list(flags) + (SANITIZERS if sanitize else [])))
    return out


def sanitized_program_or_plain(source, out_dir, flags):
    """The program under the sanitizers where the toolchain has them; otherwise the plain program (the checks of
    the program itself remain)."""
    out = os.path.join(str(out_dir), os.path.splitext(source)[0])
    sanitized = subprocess.run(_command(source, out, list(flags) + SANITIZERS), stdout=subprocess.PIPE,
                               stderr=subprocess.STDOUT, text=True)
    if sanitized.returncode != 0:
        subprocess.check_call(_command(source, out, flags))
    return out


def shared(source, out_dir, flags):
    """tests/hostsim/<source> as a shared library in ``out_dir`` (None: a directory that goes away once the
    library is loaded) -> ``ctypes.CDLL``."""
    if out_dir is None:
        with tempfile.TemporaryDirectory() as tmp:
            return shared(source, tmp, flags)
    out = os.path.join(str(out_dir), "lib" + os.path.splitext(source)[0] + ".so")
    subprocess.check_call(_command(source, out, list(flags) + ["-fPIC", "-shared"]))
    return ctypes.CDLL(out)
