"""The one builder of what the tests compile: the stand-alone host check programs (tests/cpu_*_check.cpp, the "one source with
the host" headers of layout_dm_amd/csrc compiled for the CPU) and the gfx950 assembly of the kernel files.  Every product is built
once per session into one temporary directory that is removed at exit.  A failed build is a test failure carrying the compiler's
output: a sanitized build never falls back to a plain one and nothing here skips, except kernel_asm where hipcc does not exist."""
import atexit
import functools
import os
import shutil
import subprocess
import tempfile

import pytest

from layout_dm_amd import build

TESTS = os.path.dirname(os.path.abspath(__file__))
COMMON = ("-std=c++17", "-Wall", "-Werror", "-ffp-contract=off")   # x86-64 g++ contracts nothing without -march: written down
PLAIN = ("-O2",)
SANITIZED = ("-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all")
SANITIZER_ENV = {"ASAN_OPTIONS": "detect_leaks=0:abort_on_error=0", "UBSAN_OPTIONS": "halt_on_error=1"}


@functools.lru_cache(maxsize=None)
def _dir():
    tmp = tempfile.mkdtemp(prefix="ldm_hostbuild_")
    atexit.register(shutil.rmtree, tmp, ignore_errors=True)
    return tmp


@functools.lru_cache(maxsize=None)
def host_program(name, sanitize=False, extra=()):
    """tests/<name>.cpp (a cpu_*_check stem) as an executable -> its path.  sanitize: the ASan + UBSan build."""
    exe = os.path.join(_dir(), name + ("_san" if sanitize else "") + "".join(extra))
    cmd = ["g++", *COMMON, *(SANITIZED if sanitize else PLAIN), *extra, os.path.join(TESTS, name + ".cpp"), "-o", exe]
    try:
        r = subprocess.run(cmd, capture_output=True, text=True)
    except OSError as e:
        pytest.fail(f"{' '.join(cmd)}: {e}")
    if r.returncode != 0:
        pytest.fail(f"{' '.join(cmd)}\n{r.stderr}")
    return exe


def run_host(exe, *args, timeout=300):
    """The program as its own child process, in this environment plus the sanitizers' options (a plain build ignores them)."""
    return subprocess.run([exe, *map(str, args)], capture_output=True, text=True, timeout=timeout, env={**os.environ, **SANITIZER_ENV})


def run_host_io(exe, tmp, payload: bytes, *args):
    """`exe *args in.bin out.bin` on payload -> (exit code, the bytes it wrote: b"" if it wrote no file).  A sanitizer's report
    (it ends the run with an exit code no program here uses) is printed, so that it stands in the failing test's output."""
    inp, outp = os.path.join(str(tmp), "in.bin"), os.path.join(str(tmp), "out.bin")
    with open(inp, "wb") as f:
        f.write(payload)
    if os.path.exists(outp):
        os.unlink(outp)
    r = run_host(exe, *args, inp, outp)
    if r.stderr:
        print(r.stderr)
    if not os.path.exists(outp):
        return r.returncode, b""
    with open(outp, "rb") as f:
        return r.returncode, f.read()


@functools.lru_cache(maxsize=None)
def _kernel_asm(src, resource_report):
    path = os.path.join(_dir(), src + (".report.s" if resource_report else ".s"))
    asm, report = build.device_asm(src, path, resource_report)
    return asm, report, path


def kernel_asm(src, resource_report=False):
    """build.device_asm of one csrc/ file, once per session -> (assembly text, compiler output, path of the assembly)."""
    try:
        build.hipcc()
    except RuntimeError:
        pytest.skip("hipcc not available")
    return _kernel_asm(src, resource_report)
