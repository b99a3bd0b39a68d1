"""CPU: what a checkpoint is to a handle (layout_dm_amd/csrc/ldm_weight_plan.h, the header ldm_finalize_weights plans with) compiled
for the host (tests/cpu_weight_plan_check.cpp).

  * accepted checkpoints, as name -> shape: every denoiser variant on the reference backbone and on the small geometry of
    tests/test_launch_sequence_gpu.py — the variant read from the key set and the keys the build reads, in order;
  * every refusal byte for byte (strings written down from the ldm_finalize_weights the header replaced), and which of two wrong
    things is reported;
  * the element count of every derived buffer for the eleven rows of tests/test_launch_sequence_gpu.py and a wide vocabulary, against
    the replaced allocation expressions;
  * the split mode's weight cast (scale, hi, lo) bit for bit against NumPy's float16, which rounds to nearest even;
  * all of it again on the ASan + UBSan build of the program."""
import numpy as np
import pytest

import _hostbuild as HB
import test_launch_sequence_gpu as LS


@pytest.fixture(scope="module")
def harness():
    return HB.host_program("cpu_weight_plan_check", extra=("-Wextra",))


@pytest.fixture(scope="module")
def sanitized():
    return HB.host_program("cpu_weight_plan_check", sanitize=True, extra=("-Wextra",))


def _fields(line):
    head, _, err = line.partition(" err=")   # (a refusal's message comes last and holds blanks)
    return {**dict(kv.split("=", 1) for kv in head.split()), "err": err}


def _table(exe):
    r = HB.run_host(exe, "table")
    print(r.stdout)
    assert r.returncode == 0 and "FAIL" not in r.stdout and r.stdout.splitlines()[-1] == "failed=0", r.stdout + r.stderr
    rows = [_fields(line) for line in r.stdout.splitlines()[:-1]]
    return {f["case"]: f for f in rows if "case" in f}, {f["counts"]: f for f in rows if "counts" in f}


# keys read per variant: 6 outside the layers with the elem / attr pair (5 with pos_emb=default), 13 per layer (12 without the learned
# timestep embedding), 8 schedule buffers per attribute (8 in all under q_type vanilla)
VARIANTS = {   # id: (pos_default, timestep_kind, keys outside the layers, keys per layer, schedule keys)
    "default": (0, 0, 6, 13, 40),
    "pos_default": (1, 0, 5, 13, 40),
    "pos_default_longer_table": (1, 0, 5, 13, 40),
    "abs": (0, 1, 6, 12, 40),
    "none": (0, 2, 6, 12, 40),
    "adainnorm": (0, 0, 6, 13, 40),
    "adainnorm_abs": (0, 1, 6, 12, 40),
    "vanilla": (0, 0, 6, 13, 8),
    "vanilla_pos_default": (1, 0, 5, 13, 8),
}
REFUSALS = {"missing_key", "wrong_shape", "scalar_shape", "pos_both", "pos_both_half_a_pair", "pos_neither", "pos_half_a_pair",
            "pos_default_shorter_table", "pos_default_wrong_width", "pos_default_flat", "mlp", "plain_and_linear", "none_on_instance_norm",
            "abs_layer_disagrees", "none_layer_disagrees", "abs_two_channels", "schedule_constrained", "schedule_length", "schedule_vanilla",
            "schedule_constrained_keys_on_vanilla", "schedule_vanilla_keys_on_constrained", "order_embedding_before_positions",
            "order_head_before_norm1", "order_mlp_before_both_before_layers", "order_layers_before_schedule", "order_layer_0_before_layer_1"}


def test_variants_refusals_and_counts(harness):
    cases, counts = _table(harness)
    for geo, n_layer in (("backbone", LS.REFERENCE.n_layer), ("small", LS.SMALL.n_layer)):
        for name, (pos_default, kind, outside, per_layer, sched) in VARIANTS.items():
            f = cases[f"{geo}/{name}"]
            assert (f["rc"], f["pos_default"], f["timestep_kind"]) == ("0", str(pos_default), str(kind)), f
            assert int(f["reads"]) == outside + n_layer * per_layer + sched, f
    assert REFUSALS <= set(cases)
    for name in REFUSALS:
        assert cases[name]["rc"] == "-4" and cases[name]["err"], name
    # one row of counts per launch-sequence configuration, and the wide vocabulary
    assert set(LS.CASES) | {"split_bins64", "split_abs"} == set(counts)
    assert all(f["rc"] == "0" for f in counts.values())


def test_the_same_under_address_and_undefined_sanitizers(sanitized):
    _table(sanitized)


def _cast_inputs():
    f32 = np.float32
    rng = np.random.default_rng(11)
    tie = 2.0 ** -10   # fp16 carries 11 significant bits: 1 + (2 k + 1) 2^-11 lies halfway between two fp16 values in [1, 2)
    edges = np.array([0.0, -0.0, 1.0, -1.0,
                      1 + tie / 2, 1 + 3 * tie / 2, -(1 + tie / 2), -(1 + 3 * tie / 2),       # ties: to the even neighbour below / above
                      1 + tie / 2 + 2.0 ** -23, 1 + 3 * tie / 2 - 2.0 ** -23,                 # ... and one fp32 ulp off the ties
                      1.9995117, 1.99975586, 1.9999999,                                       # rounding up into the next binade
                      2.0 ** -14, 2.0 ** -15, 3 * 2.0 ** -16, 2.0 ** -24, 2.0 ** -25, 1.5 * 2.0 ** -25, 2.0 ** -26,   # fp16 denormals on hi
                      2.0 ** -24 + 2.0 ** -25, 5 * 2.0 ** -25, 7 * 2.0 ** -25, -(2.0 ** -20) * (1 + 2.0 ** -5),
                      1 + 2.0 ** -12, 1 + 2.0 ** -13, 1 + 2.0 ** -20, 1.25 + 2.0 ** -23, 0.33333334, 1e-10, 1e-39], dtype=f32)   # ... and on lo
    return {
        "edges": edges,                                                     # max |w| = 1.99..: scale 1
        "edges_scaled_down": (edges * f32(2.0 ** -7)).astype(f32),          # scale 2^7
        "edges_scaled_up": (edges * f32(2.0 ** 9)).astype(f32),             # scale 2^-9 (hi reaches 65 504's neighbourhood without it)
        "largest_finite": np.array([np.finfo(f32).max, 1.0, -np.finfo(f32).max, 3e38, 65504.0, 65519.0, 65520.0, 70000.0], dtype=f32),
        "inf_and_nan": np.array([np.inf, np.nan, -np.inf, 1.0, 65519.0, 65520.0, 1e5, -0.0, 2.0 ** -25], dtype=f32),   # scale 1
        "nan_only": np.array([np.nan, 0.5, -0.25], dtype=f32),             # NaN does not take part in the maximum: scale 2
        "zeros": np.zeros(17, dtype=f32),
        "normal_sigma_0.02": rng.normal(0.0, 0.02, 100_000).astype(f32),
        "normal_sigma_20": rng.normal(0.0, 20.0, 100_000).astype(f32),
    }


def _expected(w):
    """scale = 2^-floor(log2(max |w|)), 1 where the maximum is 0 or not finite; hi = f16(f32(w s)), lo = f16(f32(w s) - f32(hi))"""
    f32 = np.float32
    with np.errstate(all="ignore"):
        mx = f32(0)
        for x in np.abs(w[~np.isnan(w)]):
            mx = max(mx, x)
        scale = f32(2.0) ** f32(-np.floor(np.log2(mx))) if mx > 0 and np.isfinite(mx) else f32(1)
        x = (w * scale).astype(f32)
        hi = x.astype(np.float16)
        lo = (x - hi.astype(f32)).astype(f32).astype(np.float16)
    return scale, hi, lo


def _same_bits(got, want):
    nan = np.isnan(want)
    return np.array_equal(np.isnan(got), nan) and np.array_equal(got.view(np.uint16)[~nan], want.view(np.uint16)[~nan])


@pytest.mark.parametrize("build", ["plain", "sanitized"])
def test_split_cast_is_numpys_float16_bit_for_bit(harness, sanitized, tmp_path, build):
    exe = harness if build == "plain" else sanitized
    for name, w in _cast_inputs().items():
        rc, out = HB.run_host_io(exe, tmp_path, w.tobytes(), "cast")
        assert rc == 0 and len(out) == 4 + 4 * w.size, name
        scale = np.frombuffer(out[:4], dtype=np.float32)[0]
        hi = np.frombuffer(out[4:4 + 2 * w.size], dtype=np.float16)
        lo = np.frombuffer(out[4 + 2 * w.size:], dtype=np.float16)
        want_scale, want_hi, want_lo = _expected(w)
        print(f"[{name}] n = {w.size}, scale {scale}, fp16 denormals: hi {int(((np.abs(hi) < 2.0 ** -14) & (hi != 0)).sum())}, "
              f"lo {int(((np.abs(lo) < 2.0 ** -14) & (lo != 0)).sum())}, NaN: hi {int(np.isnan(hi).sum())}, lo {int(np.isnan(lo).sum())}")
        assert scale.view(np.uint32) == np.float32(want_scale).view(np.uint32), (name, scale, want_scale)
        assert _same_bits(hi, want_hi), (name, np.flatnonzero(hi.view(np.uint16) != want_hi.view(np.uint16))[:5])
        assert _same_bits(lo, want_lo), (name, np.flatnonzero(lo.view(np.uint16) != want_lo.view(np.uint16))[:5])
    # the inputs do reach what they are here for
    _, hi, lo = _expected(_cast_inputs()["edges"])
    assert ((np.abs(hi) < 2.0 ** -14) & (hi != 0)).any() and ((np.abs(lo) < 2.0 ** -14) & (lo != 0)).any()
    assert _expected(_cast_inputs()["inf_and_nan"])[0] == 1 and _expected(_cast_inputs()["zeros"])[0] == 1
    assert _expected(_cast_inputs()["nan_only"])[0] == 2
