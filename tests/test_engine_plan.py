"""CPU: which engine a configuration runs (layout_dm_amd/csrc/ldm_engine_plan.h, the header ldm_create plans a handle with) compiled
for the host (tests/cpu_engine_plan_check.cpp).

  * the geometry -> engine table, its refusals (messages byte for byte, and which of them wait behind the device probe) and every
    buffer size against values written down by hand from the ldm_create the header replaced;
  * the eleven rows of tests/test_launch_sequence_gpu.py, knob rows included, from the plan alone: the `kernels=` string each of
    them pins on the GPU;
  * the workspace size rules as arithmetic: a panel holds the 128-row read of a chunk's last layout for every S in 1..128;
  * all of it again on the ASan + UBSan build of the program."""
import pytest

import _hostbuild as HB
import test_launch_sequence_gpu as LS

PRECISION = {"exact": 0, "fast": 1, "split": 2, "mixed": 3, "hybrid": 4}   # include/ldm_hip.h LDM_PREC_*
STRUCTURE = {LS.stack: "Stack", LS.hybrid_fused: "RowResident", LS.row_resident: "RowResident", LS.row_resident_tiled_attention: "RowResident"}


@pytest.fixture(scope="module")
def harness():
    return HB.host_program("cpu_engine_plan_check", extra=("-Wextra",))


def _fields(line):
    head, _, err = line.partition(" err=")   # (a refusal's message comes last and holds blanks)
    return {**dict(kv.split("=", 1) for kv in head.split()), "err": err}


def _table(exe):
    r = HB.run_host(exe, "table")
    print(r.stdout)
    assert r.returncode == 0 and "FAIL" not in r.stdout, r.stdout + r.stderr
    return {f["case"]: f for f in map(_fields, r.stdout.splitlines())}


def test_the_table_equals_the_values_written_down_from_the_replaced_create(harness):
    rows = _table(harness)
    assert set(LS.CASES) <= set(rows)
    for case, (_, precision, _, _, kernels) in LS.CASES.items():
        assert rows[case]["rc"] == "0" and rows[case]["kernels"] == kernels and rows[case]["precision"].startswith(precision), case
    # the refusal a test once meant to cover and missed at max_batch=8: hybrid below 64 tokens at the default batch
    assert rows["hybrid_S60"]["rc"] == "-1" and rows["hybrid_S60_batch8"]["rc"] == "0" and rows["hybrid_S65"]["rc"] == "0"
    assert rows["mixed_S60"]["rc"] == "0" and rows["mixed_S60"]["hid_panels"] == "0"


@pytest.mark.parametrize("case", sorted(LS.CASES))
def test_launch_sequence_row_from_the_plan_alone(harness, case):
    spec, precision, knobs, table, kernels = LS.CASES[case]
    r = HB.run_host(harness, "plan", spec.n_category, spec.n_bin, spec.max_elem, spec.d_model, spec.n_head, spec.d_ff, spec.n_layer,
                    spec.n_step, PRECISION[precision], 8, *(f"{k}={v}" for k, v in knobs.items()))
    assert r.returncode == 0, r.stderr
    f = _fields(r.stdout)
    print(r.stdout)
    assert f["rc"] == "0" and f["kernels"] == kernels
    # the launch table the GPU test pins follows from the structure and its two options
    want = STRUCTURE.get(table) or ("Generic16" if precision == "fast" else "Tiled")
    assert f["structure"] == want
    if table is LS.hybrid_fused:
        assert f["ffn_fused"] == "1" and f["attnout"] == "1"
    if table is LS.row_resident:
        assert f["ffn_fused"] == "0" and f["attnout"] == "1"
    if table is LS.row_resident_tiled_attention:
        assert f["ffn_fused"] == "0" and f["attnout"] == "0"
    assert f["plt"] == ("0" if table is LS.stack else "1")


def test_a_panel_holds_the_last_layouts_128_row_read(harness):
    r = HB.run_host(harness, "arith")
    print(r.stdout)
    assert r.returncode == 0 and "FAIL" not in r.stdout, r.stdout + r.stderr
    assert r.stdout.split()[-2:] == [f"cases={4 * 128 + 4 * 25 * 3}", "failed=0"]   # every (chunk, S) + the plans of the S a configuration reaches


def test_table_and_arithmetic_under_address_and_undefined_sanitizers():
    exe = HB.host_program("cpu_engine_plan_check", sanitize=True, extra=("-Wextra",))
    _table(exe)
    assert HB.run_host(exe, "arith").returncode == 0
