"""The engine-selection scenarios of tests/golden/selection_cases.json and the one function that runs them: everything
`HipMaskAndReplaceDiffusion` decides per loaded checkpoint, on fake engines (tests/_fake_engine.py).  tools/make_selection_golden.py
records what run_case returns; tests/test_selection_cases.py replays it."""
import json
import logging
import warnings

from _fake_engine import FakeEngine

REFUSE_WIDE = "ldm_create: precision fast: at most 192 classes (n_category + 4 * n_bin + 2), got 283"
REFUSE_OTHER = "ldm_create: out of device memory"
REFUSE_NORM = "ldm_create: precision hybrid: timestep_type adainnorm runs on the exact / split engines only"
ERRS = {"fast_noise": 5e-3, "hybrid_noise": 6e-3, "mixed_noise": 5e-3}     # every fp16 engine outside the 1e-3 tolerance
INSIDE, OUTSIDE = {"fast_noise": 1e-4}, dict(ERRS, hybrid_noise=4e-4)      # a checkpoint for the fp16 engine, one for the hybrid rung


def _case(name, model, loads=({},), knobs=None):
    return {"name": name, "model": model, "knobs": knobs or {}, "loads": [dict(ld) for ld in loads]}


def cases():
    """[{name, model: constructor keywords, knobs: FakeEngine attributes set before the constructor, loads: the knobs set before each
    load_state_dict}]"""
    out = []
    for p in ("exact", "split", "fast", "mixed", "hybrid"):
        out.append(_case(p, {"precision": p, "max_batch": 8}))
    for verifier in ("split", "exact"):
        for p in ("fast_verified", "mixed_verified", "hybrid_verified"):
            out.append(_case(f"{p}-{verifier}", {"precision": p, "verifier": verifier, "max_batch": 8},
                             [{"fast_noise": 2e-4, "mixed_noise": 3e-4, "hybrid_noise": 4e-4}]))
        for i, (f, h, m) in enumerate([(1e-4, 6e-3, 5e-3), (5e-3, 6e-3, 4e-3), (5e-3, 6e-3, 2e-4), (5e-3, 4e-4, 2e-4), (5e-3, None, None)]):
            out.append(_case(f"auto-{verifier}-{i}", {"precision": "auto", "verifier": verifier, "max_batch": 8},
                             [{"fast_noise": f, "hybrid_noise": h or 0.0, "mixed_noise": m or 0.0}], {"mixed_available": m is not None}))
    auto = {"precision": "auto", "max_batch": 8}
    out += [
        _case("auto-fast-nonfinite", auto, [dict(ERRS, nonfinite=["fast"], mixed_noise=2e-4)]),
        _case("auto-rung-nonfinite", auto, [dict(ERRS, nonfinite=["hybrid"], mixed_noise=2e-4)]),
        _case("auto-all-fp16-nonfinite", auto, [dict(ERRS, nonfinite=["fast", "hybrid", "mixed"])]),
        _case("fast_verified-fast-nonfinite", {"precision": "fast_verified", "max_batch": 8}, [{"nonfinite": ["fast"]}]),
        _case("auto-split-fallback", auto, [dict(ERRS, split_noise=1e-3, mixed_noise=2e-4)]),
        _case("fast_verified-split-fallback", {"precision": "fast_verified", "max_batch": 8}, [{"fast_noise": 2e-4, "split_noise": 1e-3}]),
        _case("auto-split-nonfinite-fallback", auto, [dict(INSIDE, nonfinite=["split"])]),
        _case("auto-verifiers-nonfinite", auto, [dict(INSIDE, nonfinite=["split", "exact"])]),
        _case("auto-exact-verifier-nonfinite", dict(auto, verifier="exact"), [dict(INSIDE, nonfinite=["exact"])]),
        # a checkpoint that costs the split verifier its place, then two more on the same object: the fallback stays
        _case("auto-fallback-then-more", auto, [dict(OUTSIDE, split_noise=1e-3), dict(INSIDE, split_noise=0.0), dict(OUTSIDE, split_noise=0.0)]),
        _case("wide-auto", dict(auto, n_bin=64)),
        _case("wide-auto-exact", dict(auto, n_bin=64, verifier="exact")),
        _case("wide-split", {"precision": "split", "n_bin": 64, "max_batch": 8}),
        _case("wide-fast-refused", {"precision": "fast", "n_bin": 64, "max_batch": 8}, knobs={"refuse": {"fast": REFUSE_WIDE}}),
        _case("wide-fast_verified-refused", {"precision": "fast_verified", "n_bin": 64, "max_batch": 8}, knobs={"refuse": {"fast": REFUSE_WIDE}}),
        _case("wide-fast-other-error", {"precision": "fast", "n_bin": 64, "max_batch": 8}, knobs={"refuse": {"fast": REFUSE_OTHER}}),
        _case("narrow-fast-other-error", {"precision": "fast", "max_batch": 8}, knobs={"refuse": {"fast": REFUSE_WIDE}}),
        _case("adainnorm-auto", dict(auto, timestep_type="adainnorm")),
        _case("adainnorm_abs-auto-exact", dict(auto, timestep_type="adainnorm_abs", verifier="exact")),
        _case("adainnorm-exact", {"precision": "exact", "timestep_type": "adainnorm", "max_batch": 8}),
        _case("adainnorm-hybrid_verified-refused", {"precision": "hybrid_verified", "timestep_type": "adainnorm", "max_batch": 8},
              knobs={"refuse": {"hybrid": REFUSE_NORM}}),
        _case("adainnorm-mixed-other-error", {"precision": "mixed", "timestep_type": "adainnorm", "max_batch": 8},
              knobs={"refuse": {"mixed": REFUSE_OTHER}}),
        _case("wide-adainnorm-auto", dict(auto, n_bin=64, timestep_type="adainnorm")),
        _case("wide-adainnorm-fast-refused", {"precision": "fast", "n_bin": 64, "timestep_type": "adainnorm", "max_batch": 8},
              knobs={"refuse": {"fast": REFUSE_WIDE}}),
        _case("pos_emb-default-auto", dict(auto, pos_emb="default"), [INSIDE]),
        _case("pos_emb-default-abs-split", {"precision": "split", "pos_emb": "default", "timestep_type": "adalayernorm_abs", "max_batch": 8}),
        _case("timestep_type-none-fast_verified", {"precision": "fast_verified", "timestep_type": None, "max_batch": 8}, [{"fast_noise": 2e-4}]),
        _case("pos_emb-unknown", {"precision": "auto", "pos_emb": "sinusoidal"}),
        _case("timestep_type-mlp", {"precision": "auto", "timestep_type": "adainnorm_mlp"}),
        _case("alias-f16", {"precision": "f16", "max_batch": 8}),
        _case("alias-int", {"precision": 0, "max_batch": 8}),
        _case("vanilla-auto", dict(auto, q_type="vanilla"), [INSIDE]),
        # checkpoints in turn on one object: a rung's engine is built once, the fp16 engine is where every load starts
        _case("auto-out-in", auto, [OUTSIDE, INSIDE]),
        _case("auto-out-in-out", auto, [OUTSIDE, INSIDE, OUTSIDE]),
        _case("auto-hybrid-mixed-split", auto, [OUTSIDE, dict(ERRS, mixed_noise=2e-4), ERRS, OUTSIDE]),
        _case("auto-rungs-appear", auto, [dict(ERRS, mixed_available=False), dict(ERRS, mixed_available=True, mixed_noise=2e-4)]),
        _case("fast_verified-twice", {"precision": "fast_verified", "max_batch": 8}, [{"fast_noise": 2e-4}, {"fast_noise": 3e-4}]),
    ]
    for mb in (1, 2, 3):
        out.append(_case(f"auto-max_batch-{mb}", {"precision": "auto", "max_batch": mb}, [INSIDE]))
        out.append(_case(f"auto-max_batch-{mb}-ladder", {"precision": "auto", "max_batch": mb}, [dict(ERRS, mixed_noise=2e-4)]))
    assert len({c["name"] for c in out}) == len(out)
    return out


def _jsonable(x):
    return json.loads(json.dumps(x, default=str, sort_keys=True))


def _error(e):
    return {"type": type(e).__name__, "text": str(e)}


def _snapshot(m, messages, caught):
    prec = lambda e: None if e is None else e.precision   # noqa: E731
    v = m.verified
    return {"selected_precision": m.selected_precision, "selection_report": _jsonable(m.selection_report), "info": messages,
            "warnings": [[w.category.__name__, str(w.message)] for w in caught],
            "verifier": m.verifier, "verifier_check": _jsonable(m.verifier_check), "calibration": _jsonable(m.calibration),
            "engine": prec(m.engine), "verified_fast": prec(v and v.fast), "verified_exact": prec(v and v.exact),
            "verified_calibration": _jsonable(v.calibration) if v is not None else None,
            "rungs_built": sorted(m._v_rung), "fp16_pair": None if m._v_fast is None else [prec(m._v_fast.fast), prec(m._v_fast.exact)],
            "built": [list(b) for b in FakeEngine.built]}


class _Records(logging.Handler):
    def __init__(self):
        super().__init__(logging.INFO)
        self.messages = []

    def emit(self, record):
        if record.levelno == logging.INFO:
            self.messages.append(record.getMessage())


def run_case(D, case):
    """Runs one scenario through D.HipMaskAndReplaceDiffusion (D = layout_dm_amd.diffusion, whose Engine this replaces for the
    call) and returns what the golden file holds for it."""
    import layout_dm_amd.verified as V

    FakeEngine.reset()
    for k, v in case["knobs"].items():
        setattr(FakeEngine, k, v)
    keep = D.Engine, V.Engine
    D.Engine = V.Engine = FakeEngine
    log = logging.getLogger("layout_dm_amd")
    level, handler = log.level, _Records()
    log.addHandler(handler)
    log.setLevel(logging.INFO)
    out = {"loads": []}
    m = None
    try:
        try:
            m = D.HipMaskAndReplaceDiffusion(n_category=25, **case["model"])
        except Exception as e:   # noqa: BLE001  (the scenario's outcome)
            out["constructor_error"] = _error(e)
        else:
            out["constructed"] = {"selected_precision": m.selected_precision, "precision": m.precision, "auto": m.auto,
                                  "wide_vocab": m.wide_vocab, "instance_norm": m.instance_norm, "engine": m.engine.precision,
                                  "num_classes": m.num_classes, "built": [list(b) for b in FakeEngine.built]}
            for knobs in case["loads"]:
                for k, v in knobs.items():
                    setattr(FakeEngine, k, v)
                del handler.messages[:]
                with warnings.catch_warnings(record=True) as caught:
                    warnings.simplefilter("always")
                    try:
                        m.load_state_dict({})
                    except Exception as e:   # noqa: BLE001
                        out["loads"].append({"error": _error(e), "info": list(handler.messages), "built": [list(b) for b in FakeEngine.built]})
                        break
                out["loads"].append(_snapshot(m, list(handler.messages), caught))
            # what bench.py reads after close()
            m.close()
            out["after_close"] = {"auto_tolerance": m.auto_tolerance, "verifier_tolerance": m.verifier_tolerance,
                                  "selection_report": _jsonable(m.selection_report)}
    finally:
        log.removeHandler(handler)
        log.setLevel(level)
        D.Engine, V.Engine = keep
    out.update({"built": [list(b) for b in FakeEngine.built], "peak_live": FakeEngine.peak, "live_after_close": FakeEngine.live,
                "double_closes": FakeEngine.double_closes})
    FakeEngine.reset()
    return out
