"""CPU: what ldm_sample_loop decides on the host before it launches anything (layout_dm_amd/csrc/ldm_loop_plan.h) compiled for the
host (tests/cpu_loop_plan_check.cpp).

  * the cut of a call into passes and lanes: every B in 1..600 at chunks {1, 7, 8, 128, 256}, 1..4 lanes, balanced on and off —
    the passes partition [0, B) in order, none empty, none above the chunk, ceil(B / chunk) of them, min(n_lanes, passes) lanes,
    lane l owning passes l, l + lanes, ...; and the cuts the rule's comments name, written down by hand;
  * the graph key: every field that decides a cache hit changed alone compares unequal, a copy compares equal;
  * the timestep range rule at the first, middle and last position of either array;
  * all of it again on the ASan + UBSan build of the program."""
import pytest

import _hostbuild as HB

# cases each mode counts: one per (B, chunk, lanes, balanced) | the cuts written down | the key's checks | the range rule's
CUT_CASES = 600 * 5 * 4 * 2
MODES = {"cut": CUT_CASES, "hand": 8, "key": 7 + 27 + 6 + 3, "timesteps": 2 + 2 * 3 * 2 + 1}


@pytest.fixture(scope="module")
def harness():
    return HB.host_program("cpu_loop_plan_check", extra=("-Wextra",))


def _run(exe, mode):
    r = HB.run_host(exe, mode)
    print(r.stdout[-2000:], r.stderr[-2000:])
    assert r.returncode == 0 and "FAIL" not in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
    assert r.stdout.split()[-2:] == [f"cases={MODES[mode]}", "failed=0"]


@pytest.mark.parametrize("mode", sorted(MODES))
def test_loop_plan(harness, mode):
    _run(harness, mode)


def test_loop_plan_under_address_and_undefined_sanitizers():
    exe = HB.host_program("cpu_loop_plan_check", sanitize=True, extra=("-Wextra",))
    for mode in sorted(MODES):
        _run(exe, mode)
