"""CPU: engine selection, replayed against a record of itself (tests/golden/selection_cases.json, tools/make_selection_golden.py).

Every scenario of tests/_selection_cases.py runs through HipMaskAndReplaceDiffusion on the fake engines of tests/_fake_engine.py and
must give what the file holds: the exception, or the selected name, report, INFO line, warnings, verifier check, calibration, which
engine runs and which pair verifies, the (precision, max_batch) of every engine built, in order, the largest number alive at once,
and none alive after close().  Strings and integers are compared exactly, floats to 1e-12 relative.  Then the name parser and the
two pure functions of layout_dm_amd/selection.py on records written by hand: no engine at all."""
import json
import math
import os

import pytest

import _selection_cases as SC

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "selection_cases.json")
with open(GOLDEN) as _f:
    RECORDED = json.load(_f)


def differences(got, want, path=""):
    """Where two JSON values differ: floats to 1e-12 relative (inf and nan as themselves), everything else exactly."""
    if isinstance(want, float) and isinstance(got, float):
        same = got == want or (math.isnan(got) and math.isnan(want)) or (math.isfinite(got) and math.isfinite(want)
                                                                         and abs(got - want) <= 1e-12 * abs(want))
        return [] if same else [f"{path}: {got!r} != {want!r}"]
    if type(got) is not type(want):
        return [f"{path}: {got!r} != {want!r}"]
    if isinstance(want, dict):
        out = [f"{path}: keys {sorted(got)} != {sorted(want)}"] if sorted(got) != sorted(want) else []
        return out + [d for k in want if k in got for d in differences(got[k], want[k], f"{path}/{k}")]
    if isinstance(want, list):
        out = [f"{path}: {len(got)} items != {len(want)}"] if len(got) != len(want) else []
        return out + [d for i, (g, w) in enumerate(zip(got, want)) for d in differences(g, w, f"{path}[{i}]")]
    return [] if got == want else [f"{path}: {got!r} != {want!r}"]


def test_the_file_holds_the_scenarios_as_they_are_written():
    assert differences({c["name"]: c for c in json.loads(json.dumps(SC.cases()))},
                       {n: {k: v for k, v in c.items() if k != "outcome"} for n, c in RECORDED.items()}) == []


@pytest.mark.parametrize("name", sorted(RECORDED))
def test_scenario_gives_what_was_recorded(name):
    import layout_dm_amd.diffusion as D

    case = RECORDED[name]
    got = json.loads(json.dumps(SC.run_case(D, case)))
    assert got["live_after_close"] == 0 and got["double_closes"] == 0
    assert differences(got, case["outcome"]) == []


def test_differences_is_exact_on_strings_and_integers_and_close_on_floats():
    assert differences({"a": [1, "x", 1.0, float("inf")]}, {"a": [1, "x", 1.0 + 1e-13, float("inf")]}) == []
    assert differences(1.0, 1.0 + 1e-11) and differences(1, 1.0) and differences("a", "b") and differences([1], [1, 2])
    assert differences({"a": 1}, {"b": 1}) and differences(float("inf"), 1e308) and differences(2, 3)


# -- selection.py alone ----------------------------------------------------------------------------------------------------
def test_selection_module_needs_no_gpu_library():
    import subprocess
    import sys

    code = ("import sys, layout_dm_amd.selection as S; bad = [m for m in sys.modules if m.endswith('.binding') or m == 'torch']; "
            "assert not bad, bad; print(S.parse_precision('auto'))")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd=os.path.dirname(os.path.dirname(os.path.dirname(GOLDEN))))
    assert r.returncode == 0, r.stderr
    assert r.stdout.strip() == "Request(engine='fast', verified=True, auto=True)"


def test_precision_names():
    import layout_dm_amd.diffusion as D
    import layout_dm_amd.selection as S

    assert S.parse_precision("fast_verified") == ("fast", True, False) and S.parse_precision("hybrid_verified") == ("hybrid", True, False)
    assert S.parse_precision("mixed_verified") == ("mixed", True, False) and S.parse_precision("auto") == ("fast", True, True)
    for name in ("exact", "split", "fast", "mixed", "hybrid", "f32", "f16", "f16x3", "f16x2", "split_verified", "_verified", 0, 3, None):
        assert S.parse_precision(name) == (name, False, False)
    assert D.RUNGS is S.RUNGS and D.THROUGHPUT_CLASS is S.THROUGHPUT_CLASS and D.FP16_MAX_CLASSES == S.FP16_MAX_CLASSES == 192
    assert D.HipMaskAndReplaceDiffusion.RUNGS == ("hybrid", "mixed")
    assert set(S.THROUGHPUT_CLASS) == {"exact", "split"} | {n + v for n in ("fast",) + S.RUNGS for v in ("", "_verified")}


class _Pair:
    def __init__(self, **calibration):
        self.calibration = calibration


def _selection(S, **kw):
    base = dict(requested="auto", auto=True, selected="fast_verified", engine=None, verified=None, calibration={}, rungs={},
                verifier="split", verifier_check={}, tolerance=1e-3, n_class=155, wide_vocab=False, instance_norm=None, reason=None)
    return S.Selection(**dict(base, **kw))


def test_report_and_message_of_a_record():
    import layout_dm_amd.selection as S

    T = S.THROUGHPUT_CLASS
    # an engine as requested
    sel = _selection(S, requested="split", auto=False, selected="split")
    assert S.selection_report(sel) == {"precision_requested": "split", "engine_selected": "split", "expected_throughput": T["split"]}
    assert S.selection_report(sel, "pos_emb=default")["denoiser_variant"] == "pos_emb=default"
    assert S.selection_message(sel) == f"layout_dm_amd: engine 'split' (as requested) — {T['split']}"
    assert S.selection_report(_selection(S, requested=7, auto=False, selected=7))["expected_throughput"] == "?"
    # auto down the ladder: hybrid unavailable, mixed inside
    fast = _Pair(err_rel=5e-3, err_abs=0.5, tie_abs=6.0)
    mixed = _Pair(err_rel=2e-4, err_abs=0.02, tie_abs=0.24)
    rungs = {"hybrid": {"unavailable": "no kernels"}, "mixed": {"err_rel": 2e-4, "err_abs": 0.02, "finite": True, "tie_abs": 0.24}}
    check = {"verifier": "split", "finite": True}
    sel = _selection(S, selected="mixed_verified", verified=mixed, calibration=fast.calibration, rungs=rungs, verifier_check=check)
    rep = S.selection_report(sel)
    assert rep == {"precision_requested": "auto", "engine_selected": "mixed_verified", "expected_throughput": T["mixed_verified"],
                   "fast_logits_err_rel": 5e-3, "fast_logits_err_abs": 0.5, "tolerance": 1e-3, "verifier": "split",
                   "verifier_check": check, "tie_abs": 0.24, "hybrid_unavailable": "no kernels", "mixed_logits_err_rel": 2e-4}
    assert rep["verifier_check"] is not check
    assert S.selection_message(sel) == (
        "layout_dm_amd: precision='auto' selected engine 'mixed_verified': the fp16 engine's logits error on this checkpoint is 5.00e-03 "
        "(relative, against the split reference-precision engine), OUTSIDE the 0.001 logits tolerance; no hybrid engine for this geometry; "
        f"the mixed engine's is 2.00e-04, inside — expect {T['mixed_verified']}")
    # auto, everything outside or non-finite: the verifier's name
    rungs = {"hybrid": {"err_rel": float("inf"), "finite": False}, "mixed": {"err_rel": 4e-3, "err_abs": 0.4, "finite": True, "tie_abs": 4.8}}
    sel = _selection(S, selected="exact", verifier="exact", verified=fast, calibration={"err_rel": float("inf"), "finite": False}, rungs=rungs)
    assert S.selection_message(sel) == (
        "layout_dm_amd: precision='auto' selected engine 'exact': the fp16 engine's logits error on this checkpoint is non-finite "
        "(relative, against the exact reference-precision engine), OUTSIDE the 0.001 logits tolerance; the hybrid engine's is non-finite, "
        f"OUTSIDE; the mixed engine's is 4.00e-03, OUTSIDE — expect {T['exact']}")
    # auto inside
    sel = _selection(S, verified=fast, calibration={"err_rel": 3e-4, "err_abs": 0.03})
    assert S.selection_message(sel).endswith("is 3.00e-04 (relative, against the split reference-precision engine), inside the 0.001 logits "
                                             f"tolerance — expect {T['fast_verified']}")
    # the verified names as requested
    sel = _selection(S, requested="fast_verified", auto=False, verified=fast, calibration=fast.calibration)
    assert S.selection_message(sel) == ("layout_dm_amd: engine 'fast_verified' (as requested); fp16 logits error on this checkpoint 5.00e-03 "
                                        f"(relative, against the split engine) — expect {T['fast_verified']}")
    sel = _selection(S, requested="hybrid_verified", auto=False, selected="hybrid_verified", verified=mixed, calibration=mixed.calibration)
    rep = S.selection_report(sel)
    assert rep["fast_logits_err_rel"] is None and rep["fast_logits_err_abs"] is None and rep["hybrid_logits_err_rel"] == 2e-4 and rep["tie_abs"] == 0.24
    assert S.selection_message(sel) == ("layout_dm_amd: engine 'hybrid_verified' (as requested); its logits error on this checkpoint 2.00e-04 "
                                        f"(relative, against the split engine) — expect {T['hybrid_verified']}")
    # auto without an fp16 engine: the vocabulary's reason comes before the norm's
    sel = _selection(S, selected="split", n_class=283, wide_vocab=True, instance_norm="adainnorm", reason="283 classes: ...")
    assert S.selection_report(sel) == {"precision_requested": "auto", "engine_selected": "split", "expected_throughput": T["split"],
                                       "n_class": 283, "fp16_max_classes": 192, "reason": "283 classes: ..."}
    assert S.selection_message(sel) == ("layout_dm_amd: precision='auto' selected engine 'split': the vocabulary has 283 classes and the fp16 "
                                        f"engines (fast / hybrid / mixed) serve at most 192 — no fp16 engine was built; expect {T['split']}")
    sel = _selection(S, selected="exact", verifier="exact", instance_norm="adainnorm_abs", reason="timestep_type=adainnorm_abs: ...")
    assert S.selection_report(sel, "timestep_type=adainnorm_abs") == {
        "precision_requested": "auto", "engine_selected": "exact", "expected_throughput": T["exact"],
        "denoiser_variant": "timestep_type=adainnorm_abs", "reason": "timestep_type=adainnorm_abs: ..."}
    assert S.selection_message(sel) == (
        "layout_dm_amd: precision='auto' selected engine 'exact': timestep_type=adainnorm_abs normalises per (layout, channel) over the "
        "sequence axis, which only the reference-precision engines (split / exact) serve — no fp16 engine was built; "
        f"expect less than {T['exact']} (its LayerNorm-fed GEMMs run as separate tiled launches)")
