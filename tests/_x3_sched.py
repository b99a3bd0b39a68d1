"""The schedule tables of layout_dm_amd/csrc/ldm_x3_sched.h, as tests/cpu_x3_sched_check.cpp prints them: the host program is
built (sanitizer build, plain build as fallback) and run ONCE per session, on the CPU, as its own process; the tests that replay
or compare the split kernels' protocols (test_lngemm_sched.py, test_attnout_layout.py, test_kernel_asm_lint.py) read them from
here instead of restating the header's formulas."""
import os
import shutil
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_cache = {}


def _dump():
    if "lines" not in _cache:
        cxx = shutil.which("g++") or shutil.which("c++")
        assert cxx is not None, "these tests need a host C++ compiler"
        src = os.path.join(ROOT, "tests", "cpu_x3_sched_check.cpp")
        with tempfile.TemporaryDirectory(prefix="x3_sched_") as tmp:
            exe = os.path.join(tmp, "cpu_x3_sched_check")
            r = subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", src, "-o", exe],
                               capture_output=True, text=True, cwd=ROOT)
            if r.returncode != 0 and "sanitize" in r.stderr:
                r = subprocess.run([cxx, "-O1", "-std=c++17", src, "-o", exe], capture_output=True, text=True, cwd=ROOT)
            assert r.returncode == 0, r.stderr
            out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
        assert out.returncode == 0 and "OK:" in out.stdout, out.stdout + out.stderr
        _cache["lines"] = [ln.split() for ln in out.stdout.splitlines() if "=" in ln]
    return _cache["lines"]


def rows(table, **where):
    """The lines of one table as dicts of ints, in the order printed, filtered by the given key = value pairs."""
    out = []
    for tok in _dump():
        if tok[0] == table:
            d = {k: int(v) for k, v in (t.split("=") for t in tok[1:])}
            if all(d[k] == v for k, v in where.items()):
                out.append(d)
    assert out, (table, where)
    return out


def row(table, **where):
    (r,) = rows(table, **where)
    return r
