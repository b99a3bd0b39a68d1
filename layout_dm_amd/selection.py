"""Which engine a checkpoint gets: the precision names, `precision="auto"`'s ladder and the report of what was selected.

Everything here works on engines it is handed (an `mk(precision, max_batch=None)` factory), so it runs without a GPU on stand-in
engines; neither the binding nor the library is imported (verified.py, which measures, is imported where a verifier is built).
precision "fast_verified": the fp16 engine for every sampler, plus a reference-precision engine of the same weights — the verifier:
"split" (fp16 x 3 on the fp16 matrix pipe: the exact mode's logits error at 1.7 x its speed) or "exact" (fp32 MFMA) — that re-decides
the near-tie layouts of DETERMINISTIC decoding (verified.py): greedy tokens are then the reference's, bit for bit.
precision "auto": load() measures the fp16 engine's logits error against the verifier ON THE CHECKPOINT (probe states over the whole
timestep range) and keeps it only inside the north star's 1e-3 relative tolerance.  (The fp16 mode's error is a property of the weights:
3e-4 on the reference's init, ~1e-3 at sigma = 0.06, percents once attention rows saturate: DESIGN.md section 3.5.)  Outside, the
ladder: "hybrid" (hi + lo fp16 activations x fp16 weights on the attention path, where the fp16 error lives; FFN and head in plain
fp16; 2.8e-4 on a fitted checkpoint whose fp16 error is 1.2e-3), then "mixed" (hi + lo x fp16 weights everywhere: two matrix passes
per weight product instead of split's three; 2e-4 there), each rung built on first need, measured the same way and kept — again with
verified greedy decoding — if inside; only then the reference-precision engine runs every call.  "hybrid(_verified)" /
"mixed(_verified)" select a rung unconditionally.
Wide vocabularies (64 / 128 bins per coordinate: more than FP16_MAX_CLASSES classes) and the adainnorm kinds of timestep_type
(instance norm over a layout's rows) run on the reference-precision engines only: auto then IS its verifier engine — no fp16 engine is
built or measured — and every name that needs an fp16 engine is refused with the library's own message.
"""
from __future__ import annotations

from typing import Callable, Dict, NamedTuple, Optional

FP16_MAX_CLASSES = 192   # ldm_create: fast / mixed / hybrid refuse wider vocabularies; exact / split take up to 576 classes, 128 bins
RUNGS = ("hybrid", "mixed")   # auto's ladder between the fp16 engine and the reference-precision engine, fastest first
# what each engine delivers on one MI355X (Rico25-shaped sequences, T = 100, batch 512; bench.py measures it on the box at hand)
THROUGHPUT_CLASS = {
    "fast": "~3 900 layouts/s (fp16 operands, one launch per sampling call)",
    "fast_verified": "~3 400 - 3 900 layouts/s (fp16 engine; greedy decoding re-checked by the reference-precision engine)",
    "hybrid": "~2 200 layouts/s (attention path: hi + lo fp16 activations x fp16 weights; FFN and head in plain fp16; per-step launches)",
    "hybrid_verified": "~2 200 layouts/s (attention path hi + lo x fp16, FFN / head plain fp16; greedy decoding re-checked by the reference-precision engine)",
    "mixed": "~1 500 layouts/s (hi + lo fp16 activations x fp16 weights: two matrix passes per weight product, per-step launches)",
    "mixed_verified": "~1 500 layouts/s (hi + lo fp16 activations x fp16 weights; greedy decoding re-checked by the reference-precision engine)",
    "split": "~1 150 - 1 200 layouts/s (reference precision on the fp16 matrix pipe, per-step launches)",
    "exact": "~420 layouts/s (fp32 MFMA)",
}
_VERIFIED = "_verified"


class Request(NamedTuple):
    engine: object    # the name the engine factory gets for the primary engine
    verified: bool    # a verifier engine beside it re-decides greedy decoding's near ties
    auto: bool        # load() measures the fp16 engine on the checkpoint and walks the ladder


def parse_precision(precision) -> Request:
    """"fast_verified" -> ("fast", True, False), "auto" -> ("fast", True, True), "split" -> ("split", False, False); what is not a
    name of this module (binding.PRECISIONS' aliases, an integer) goes to the engine factory as it is."""
    if precision == "auto":
        return Request("fast", True, True)
    if isinstance(precision, str) and precision.endswith(_VERIFIED) and precision[:-len(_VERIFIED)] in ("fast",) + RUNGS:
        return Request(precision[:-len(_VERIFIED)], True, False)
    return Request(precision, False, False)


class Selection(NamedTuple):
    """What load() decided for one checkpoint."""
    requested: object                      # the `precision` argument
    auto: bool
    selected: object                       # selected_precision: the name of what runs
    engine: object                         # the engine every call runs on
    verified: object                       # the VerifiedGreedy in force (greedy decoding goes through it while engine is its .fast), or None
    calibration: Dict[str, float]          # the primary engine's measured error against the verifier, {} without a verifier
    rungs: Dict[str, Dict[str, object]]    # auto, ladder order: rung -> {"unavailable": text} | {"err_rel", "finite"[, "err_abs", "tie_abs"]}
    verifier: str                          # the verifier engine's name ("exact" after the fallback)
    verifier_check: Dict[str, object]
    tolerance: float
    n_class: int
    wide_vocab: bool
    instance_norm: Optional[str]           # the timestep_type where it is an instance-norm kind
    reason: Optional[str]                  # auto: why no fp16 engine was built


class Selector:
    """Owns the engines of one model: builds them, loads every checkpoint into them, selects, and releases them."""

    def __init__(self, mk: Callable, requested, verifier: str = "split", auto_tolerance: float = 1e-3,
                 verifier_tolerance: float = 5e-4, wide_vocab: bool = False, instance_norm: Optional[str] = None):
        self.mk, self.requested, self.request = mk, requested, parse_precision(requested)
        self.verifier, self.auto_tolerance, self.verifier_tolerance = verifier, auto_tolerance, verifier_tolerance
        self.wide_vocab, self.instance_norm = wide_vocab, instance_norm
        self._built = []      # every engine alive, in build order
        self.v_fast = None    # VerifiedGreedy(primary engine, verifier)
        self.v_rung: Dict[str, object] = {}   # rung -> VerifiedGreedy(its engine, verifier), built on first need
        req, no_fp16 = self.request, wide_vocab or bool(instance_norm)
        assert not req.verified or verifier in ("split", "exact")
        self.selected = None if req.auto else requested    # (auto: not before the first load)
        self.reason = None
        if req.auto and no_fp16:
            self.primary = self._build(verifier)
            self.selected = verifier
            self.reason = (f"{self.primary.C} classes: the fp16 engines (fast / hybrid / mixed) serve at most {FP16_MAX_CLASSES}; no fp16 "
                           "engine was built or measured") if wide_vocab else (
                f"timestep_type={instance_norm}: instance norm over a layout's rows runs on the tiled kernels of the "
                "reference-precision engines (split / exact) only; no fp16 engine was built or measured")
            return
        try:
            self.primary = self._build(req.engine)
        except RuntimeError as e:
            refusals = ["192 classes"] * wide_vocab + ["adainnorm"] * bool(instance_norm)
            if req.engine in ("exact", "split") or not any(r in str(e) for r in refusals):
                raise
            raise NotImplementedError(str(e)) from e
        if req.verified:
            from .verified import VerifiedGreedy

            self.v_fast = VerifiedGreedy(self.primary, self._build(verifier))

    def _build(self, precision):
        self._built.append(self.mk(precision))
        return self._built[-1]

    def close(self) -> None:
        """Release every engine this object built (the handles own GBs of workspace)."""
        for e in self._built:
            e.close()
        self._built = []

    def _selection(self, selected, engine, verified=None, rungs=None, check=None) -> Selection:
        return Selection(self.requested, self.request.auto, selected, engine, verified,
                         dict(self.v_fast.calibration) if self.v_fast is not None else {}, rungs or {}, self.verifier, check or {},
                         self.auto_tolerance, self.primary.C, self.wide_vocab, self.instance_norm, self.reason)

    def load(self, state_dict) -> Selection:
        """Every engine in use gets the checkpoint; with a verifier: the verifier is checked, the primary engine's error measured
        (tie_abs <- 6 x safety x measured |logits error|), and auto selects — starting from the fp16 engine for every checkpoint."""
        v, tol = self.v_fast, self.auto_tolerance
        self.primary.load_state_dict(state_dict)
        if v is None:
            return self._selection(self.selected, self.primary)
        v.exact.load_state_dict(state_dict)
        check = self._check_verifier(state_dict)
        try:
            cal = v.calibrate()
        except FloatingPointError:
            if not self.request.auto:
                raise
            # the fp16 engine overflows on this checkpoint (the verifier was checked finite above): auto's answer
            cal = v.calibration = dict(v.calibration, err_rel=float("inf"), finite=False)
        if not self.request.auto:
            return self._selection(self.requested, v.fast, v, check=check)
        if cal["err_rel"] <= tol:                                # (NaN / inf compare False)
            return self._selection("fast_verified", v.fast, v, check=check)
        rungs = {}
        for rung in RUNGS:
            rungs[rung] = self._measure_rung(rung, state_dict)
            if rungs[rung].get("err_rel", float("inf")) <= tol:
                return self._selection(rung + _VERIFIED, self.v_rung[rung].fast, self.v_rung[rung], rungs, check)
        return self._selection(self.verifier, v.exact, v, rungs, check)

    def _check_verifier(self, state_dict) -> Dict[str, object]:
        """auto / fast_verified treat the verifier engine as ground truth: check THAT once per checkpoint.  The split engine rounds
        every operand to an fp16 hi part (overflow above 65 504) and an unscaled fp16 lo part, so it is compared with a small
        fp32-MFMA engine of the same weights on probe states; if its logits are non-finite or differ by more than
        `verifier_tolerance` the fp32-MFMA engine becomes the verifier — of every pair, from here on — and if that one is
        non-finite too the checkpoint is refused here, at load time — not at the first sampling call."""
        from .verified import measure_fast_error, probe_states

        v = self.v_fast
        n = max(1, min(4, int(v.exact.max_batch)))   # (the probe batch must fit an engine built with max_batch < 4)
        if self.verifier != "split":
            states = probe_states(v.exact, n_layouts=n, ts=[v.exact.T // 2])
            if not bool(v.exact.denoise_logits(*states[0]).isfinite().all()):
                raise FloatingPointError("reference-precision engine: non-finite logits on this checkpoint")
            return {"verifier": self.verifier, "finite": True}
        small = self.mk("exact", n)
        try:
            small.load_state_dict(state_dict)
            states = probe_states(small, n_layouts=n, ts=[small.T - 1, small.T // 2, 1])
            c = measure_fast_error(v.exact, small, states)
            lg_ok = bool(small.denoise_logits(*states[0]).isfinite().all())
        finally:
            small.close()
        check = {"verifier": "split", "err_rel_vs_fp32_mfma": c["err_rel"], "finite": c["finite"], "tolerance": self.verifier_tolerance}
        if c["finite"] and c["err_rel"] <= self.verifier_tolerance:
            return check
        if not lg_ok:
            raise FloatingPointError("reference-precision engines: non-finite logits on this checkpoint (fp32 MFMA too)")
        import warnings

        warnings.warn(f"split verifier outside {self.verifier_tolerance:g} of the fp32-MFMA engine on this checkpoint "
                      f"({c['err_rel']:.3g}, finite={c['finite']}): verifying with the fp32-MFMA engine instead",
                      RuntimeWarning)
        old, new = v.exact, self._build("exact")
        new.load_state_dict(state_dict)
        for pair in [v] + list(self.v_rung.values()):
            pair.exact = new
        self._built.remove(old)
        old.close()
        self.verifier = "exact"
        return dict(check, verifier="exact (fallback)")

    def _measure_rung(self, rung: str, state_dict) -> Dict[str, object]:
        """One rung of auto's ladder: the engine (built on first need; unavailable where the library has no such kernels for the
        model's geometry) measured against the verifier exactly like the fp16 engine was."""
        from .verified import VerifiedGreedy

        if rung not in self.v_rung:
            try:
                self.v_rung[rung] = VerifiedGreedy(self._build(rung), self.v_fast.exact)
            except RuntimeError as e:                            # (ldm_create: geometry without these kernels)
                return {"unavailable": str(e)}
        vm = self.v_rung[rung]
        vm.fast.load_state_dict(state_dict)
        try:
            cal = vm.calibrate()
        except FloatingPointError:
            return {"err_rel": float("inf"), "finite": False}
        return {"err_rel": cal["err_rel"], "err_abs": cal["err_abs"], "finite": True, "tie_abs": cal["tie_abs"]}


def selection_report(sel: Selection, variant: Optional[str] = None) -> Dict[str, object]:
    """`selection_report` (python -m layout_dm_amd.check_checkpoint prints it): which engine runs, the fp16 engine's measured logits
    error, the tolerance it was held against and the throughput class to expect.  variant: diffusion.variant_name's."""
    rep = {"precision_requested": sel.requested, "engine_selected": sel.selected,
           "expected_throughput": THROUGHPUT_CLASS.get(sel.selected, "?")}
    if variant:
        rep["denoiser_variant"] = variant
    if sel.verified is not None:
        rung_requested = not sel.auto and sel.requested != "fast_verified"      # mixed_verified / hybrid_verified
        cal = {} if rung_requested else sel.calibration
        rep.update({"fast_logits_err_rel": cal.get("err_rel"), "fast_logits_err_abs": cal.get("err_abs"),
                    "tolerance": sel.tolerance, "verifier": sel.verifier, "verifier_check": dict(sel.verifier_check),
                    "tie_abs": sel.verified.calibration.get("tie_abs")})
        if rung_requested:
            rep[parse_precision(sel.requested).engine + "_logits_err_rel"] = sel.verified.calibration.get("err_rel")
        for rung, err in sel.rungs.items():
            if "unavailable" in err:
                rep[rung + "_unavailable"] = err["unavailable"]
            else:
                rep[rung + "_logits_err_rel"] = err.get("err_rel")
    if sel.reason:
        if sel.wide_vocab:
            rep.update({"n_class": sel.n_class, "fp16_max_classes": FP16_MAX_CLASSES})
        rep["reason"] = sel.reason
    return rep


def selection_message(sel: Selection) -> str:
    """The one INFO line per loaded checkpoint: a user must be able to tell why a job runs at 1 200 instead of 3 900 layouts/s."""
    name, expect = sel.selected, THROUGHPUT_CLASS.get(sel.selected, "?")
    if sel.reason and sel.wide_vocab:
        return (f"layout_dm_amd: precision='auto' selected engine '{name}': the vocabulary has {sel.n_class:d} classes and the fp16 engines "
                f"(fast / hybrid / mixed) serve at most {FP16_MAX_CLASSES:d} — no fp16 engine was built; expect {expect}")
    if sel.reason:
        return (f"layout_dm_amd: precision='auto' selected engine '{name}': timestep_type={sel.instance_norm} normalises per (layout, channel) over the "
                "sequence axis, which only the reference-precision engines (split / exact) serve — no fp16 engine was built; "
                f"expect less than {expect} (its LayerNorm-fed GEMMs run as separate tiled launches)")
    if sel.verified is None:
        return f"layout_dm_amd: engine '{name}' (as requested) — {expect}"
    fmt = lambda e: "non-finite" if e is None or e != e or e == float("inf") else f"{e:.2e}"   # noqa: E731
    if sel.auto:
        why = ("inside" if name == "fast_verified" else "OUTSIDE") + f" the {sel.tolerance:g} logits tolerance"
        for rung, err in sel.rungs.items():
            if "unavailable" in err:
                why += f"; no {rung} engine for this geometry"
            else:
                why += f"; the {rung} engine's is {fmt(err.get('err_rel'))}, " + ("inside" if name == rung + _VERIFIED else "OUTSIDE")
        return (f"layout_dm_amd: precision='auto' selected engine '{name}': the fp16 engine's logits error on this checkpoint is "
                f"{fmt(sel.calibration.get('err_rel'))} (relative, against the {sel.verifier} reference-precision engine), {why} — expect {expect}")
    if sel.requested != "fast_verified":
        return (f"layout_dm_amd: engine '{sel.requested}' (as requested); its logits error on this checkpoint "
                f"{fmt(sel.verified.calibration.get('err_rel'))} (relative, against the {sel.verifier} engine) — expect {expect}")
    return (f"layout_dm_amd: engine '{name}' (as requested); fp16 logits error on this checkpoint {fmt(sel.calibration.get('err_rel'))} "
            f"(relative, against the {sel.verifier} engine) — expect {expect}")
