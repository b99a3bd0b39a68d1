"""The schedule tables of layout_dm_amd/csrc/ldm_x3_sched.h, as tests/cpu_x3_sched_check.cpp prints them: the host program is
built (ASan + UBSan build) and run ONCE per session, on the CPU, as its own process; the tests that replay
or compare the split kernels' protocols (test_lngemm_sched.py, test_attnout_layout.py, test_kernel_asm_lint.py) read them from
here instead of restating the header's formulas."""
import functools

import _hostbuild as HB


@functools.lru_cache(maxsize=None)
def _dump():
    out = HB.run_host(HB.host_program("cpu_x3_sched_check", sanitize=True), timeout=120)
    assert out.returncode == 0 and "OK:" in out.stdout, out.stdout + out.stderr
    return [ln.split() for ln in out.stdout.splitlines() if "=" in ln]


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
