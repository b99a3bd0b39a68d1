"""CPU: the denoiser variants of the reference's LayoutDM class beyond its default — pos_emb=default, timestep_type
adalayernorm_abs / None / adainnorm / adainnorm_abs — against tests/golden/variants/*.npz (the real reference, written by
tools/make_denoiser_variant_golden.py):

  * layout_dm_amd.synthetic.synth_state_dict(pos_emb=, timestep_type=) has the key set and shapes of the reference's state_dict();
  * the restated sinusoid (every step in float64, rounded to float32 where the reference rounds) against the reference's own table;
  * layout_dm_amd/csrc/ldm_variant_core.h compiled for the host (tests/cpu_variant_check.cpp) gives the restatement bit for bit;
  * what ldm_engine_plan.h decides for the norm1 kind (tests/cpu_variant_plan_check.cpp): Tiled on exact / split, the three refusals
    byte for byte, every existing case unchanged;
  * what stays refused says why; and, where the reference can be imported, the tool writes the committed files again bit for bit."""
import importlib.util
import os

import numpy as np
import pytest

import _hostbuild as HB
from _stub_tokenizer import StubTokenizer
from layout_dm_amd import synthetic
from oracle import ref_harness

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def load_tool():
    spec = importlib.util.spec_from_file_location("make_denoiser_variant_golden", os.path.join(ROOT, "tools", "make_denoiser_variant_golden.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    return tool


TOOL = load_tool()
VARIANTS = sorted(TOOL.VARIANTS)


def fixture(golden_dir, name):
    with np.load(os.path.join(golden_dir, "variants", name + ".npz")) as z:
        return {k: z[k] for k in z.files}


# ----------------------------------------------------------------------------- fixtures and synthetic checkpoints
@pytest.mark.parametrize("name", VARIANTS)
def test_fixture_is_data_of_the_expected_shape(golden_dir, name):
    fx, spec = fixture(golden_dir, name), TOOL.SPEC
    assert os.path.getsize(os.path.join(golden_dir, "variants", name + ".npz")) < (1 << 20)
    assert all(v.dtype.kind in "fiubU" for v in fx.values())            # numbers and names only: nothing a loader could execute
    assert int(fx["weight_seed"]) == 1 and sorted(fx["ts"].tolist()) == [0, 1, 99]
    for t in fx["ts"]:
        B = fx[f"tokens_{t}"].shape[0]
        assert B == (1 if t == 0 else 2)
        assert fx[f"logits_{t}"].shape == (B, spec.seq_len, spec.n_class) and fx[f"post_{t}"].shape == (B, spec.n_class, spec.seq_len)
    assert fx["traj_states_after"].shape == (10, 2, spec.seq_len) and fx["traj_steps"].tolist() == list(range(90, -1, -10))
    assert len(fx["traj_chosen"]) >= 5 and (fx["traj_states_after"][-1] != spec.mask_id).all()
    assert ("sinusoid" in fx) == TOOL.VARIANTS[name].is_abs == ("logits_patched_99" in fx)


@pytest.mark.parametrize("name", VARIANTS)
def test_synthetic_state_dict_has_the_reference_key_set_and_shapes(golden_dir, name):
    fx, v = fixture(golden_dir, name), TOOL.VARIANTS[name]
    want = dict(zip(fx["manifest_names"].tolist(), fx["manifest_shapes"].tolist()))
    shape = lambda a: ",".join(str(n) for n in a.shape)   # noqa: E731
    got = {k: shape(a) for k, a in TOOL.state_dict(v).items()}
    assert got == want
    # synth_state_dict alone: everything but the schedule buffers, which belong to q_type (the un-prefixed set of vanilla.py:66-73)
    sched = tuple(synthetic.SCHEDULE_NAMES)
    plain = {k: shape(a) for k, a in synthetic.synth_state_dict(TOOL.SPEC, seed=1, perturb=True, prefix="", pos_emb=v.pos_emb,
                                                                 timestep_type=v.timestep_type).items() if not k.endswith(sched)}
    assert plain == {k: s for k, s in want.items() if not k.endswith(sched)}
    # the variant's own keys
    assert ("transformer.pos_emb.pos_emb" in want) == (v.pos_emb == "default") != ("transformer.pos_emb.elem_emb" in want)
    n1 = "transformer.backbone.layers.0.norm1."
    assert (n1 + "weight" in want) == (v.timestep_type is None)
    assert (n1 + "emb.weight" in want) == (v.timestep_type in ("adalayernorm", "adainnorm"))
    assert (n1 + "linear.weight" in want) == (v.timestep_type is not None)


def test_default_arguments_draw_what_they_always_drew():
    from oracle import spec as SP
    from oracle import synth

    a = synthetic.synth_state_dict(synthetic.RICO25, seed=3, perturb=True)
    b = synthetic.synth_state_dict(synthetic.RICO25, seed=3, perturb=True, pos_emb="elem_attr", timestep_type="adalayernorm")
    c = synth.synth_state_dict(SP.RICO25, seed=3, perturb=True)
    assert list(a) == list(b) == list(c) and all(np.array_equal(a[k], b[k]) and np.array_equal(a[k], c[k]) for k in a)
    with pytest.raises(ValueError):
        synthetic.synth_state_dict(synthetic.RICO25, pos_emb="sinusoidal")
    with pytest.raises(ValueError):
        synthetic.synth_state_dict(synthetic.RICO25, timestep_type="adalayernorm_mlp")


# ----------------------------------------------------------------------------- the sinusoid
def _table_error(golden_dir, name):
    fx = fixture(golden_dir, name)
    T, D = fx["sinusoid"].shape
    return np.abs(fx["sinusoid"].astype(np.float64) - TOOL.restated_sinusoid(T, D).astype(np.float64)), TOOL.sinusoid_args(T, D)


def _torch_sinusoid(T, D):
    """SinusoidalPosEmb(T, D)(arange(T)) (transformer_utils.py:34-49) in torch's own float32 arithmetic, operation for operation"""
    import math

    import torch

    x = torch.arange(T) / float(T) * 4000.0
    half = D // 2
    emb = torch.exp(torch.arange(half) * -(math.log(10000) / (half - 1)))
    arg = x[:, None] * emb[None, :]
    return torch.cat((arg.sin(), arg.cos()), dim=-1).numpy()


def test_restated_sinusoid_against_the_reference_table_within_the_bound_of_the_issue(golden_dir):
    """|restated - reference| <= 2^-23 |arg| + 2^-22 per entry, "one ulp of frequency times the argument, plus the output roundings":
    torch's float32 exp is not correctly rounded — at D = 464 the frequencies k = 3, 128, 137, 199 of the 232 come out one ulp off —
    every frequency is <= 1, so its ulp is at most 2^-23, and it is multiplied by x = t / T * 4000, the argument the embedding is
    evaluated at: `arg` is x.  Against the reference's stored [100][464] table (the same in both *_abs fixtures), and against torch's
    own float32 arithmetic at the other shapes the bound was stated for, (100, 64) and (10, 32): inside everywhere, as stated there.

    (Read with `arg` = x * f_k, what the sine is taken of, the bound would NOT hold for the chain as prescribed: 4 of the 46 400
    entries at (100, 464), all on k = 137 at |x f_k| = 10.4 - 12.7, differ by 1.49e-6 - 1.91e-6 against 1.47e-6 - 1.76e-6, because
    the float32 rounding of the product, 2^-20 there, has no term in it.  The next test holds every entry to the bound in |x f_k|
    with that term counted, which is the tighter of the two wherever f_k is below about 1 / 2.)  Largest difference: 2.44e-4."""
    for name in ("abs", "adainnorm_abs"):
        fx = fixture(golden_dir, name)
        T, D = fx["sinusoid"].shape
        assert (T, D) == (100, 464)
        d = np.abs(fx["sinusoid"].astype(np.float64) - TOOL.restated_sinusoid(T, D).astype(np.float64))
        bound = 2.0 ** -23 * TOOL.sinusoid_x(T, D) + 2.0 ** -22
        print(f"[{name}] max |restated - reference| = {d.max():.4e}; outside the bound: {int((d > bound).sum())} of {d.size} entries")
        assert np.array_equal(bound, TOOL.sinusoid_bound(T, D))
        assert (d <= bound).all()
    for T, D in ((100, 64), (10, 32)):
        d = np.abs(_torch_sinusoid(T, D).astype(np.float64) - TOOL.restated_sinusoid(T, D).astype(np.float64))
        print(f"[{T}, {D}] max |restated - torch| = {d.max():.4e}")
        assert (d <= TOOL.sinusoid_bound(T, D)).all()


@pytest.mark.parametrize("name", ["abs", "adainnorm_abs"])
def test_restated_sinusoid_against_the_reference_table_with_the_product_rounding(golden_dir, name):
    """The same comparison under the bound with every rounding of the chain counted, 2^-22 |arg| + 2^-23: the frequency's ulp moves the
    exact product by at most 2^-23 |arg|; each of the two chains rounds its product to float32, at most 2^-24 |arg| each; sin and cos
    have slope <= 1; each chain rounds its output, at most 2^-24 each.  Not vacuous: sin | cos swapped or a float32
    `t * (4000 / T)` miss it by orders of magnitude, and the differences must sit on a few frequencies only."""
    d, arg = _table_error(golden_dir, name)
    assert (d <= 2.0 ** -22 * arg + 2.0 ** -23).all()
    assert d.max() > 1e-5          # (the two tables do differ: the reference's exp)
    assert (d == 0).mean() > 0.9   # ... on the four frequencies only


@pytest.fixture(scope="module")
def variant_check():
    return HB.host_program("cpu_variant_check", extra=("-Wextra",))


@pytest.mark.parametrize("T,D", [(100, 464), (100, 64), (10, 32), (7, 16)])
def test_host_build_of_the_device_source_gives_the_restated_sinusoid(variant_check, tmp_path, T, D):
    for exe in (variant_check, HB.host_program("cpu_variant_check", sanitize=True, extra=("-Wextra",))):
        out = os.path.join(str(tmp_path), "sinus.bin")
        r = HB.run_host(exe, "sinus", T, D, out)
        assert r.returncode == 0, r.stderr
        got = np.fromfile(out, np.float32).reshape(T, D)
        want = TOOL.restated_sinusoid(T, D)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), int((got != want).sum())
    assert got[0, : D // 2].tolist() == [0.0] * (D // 2) and got[0, D // 2:].tolist() == [1.0] * (D // 2)   # t = 0: sin 0 | cos 0


def test_host_build_refuses_bad_sinusoid_arguments(variant_check, tmp_path):
    for T, D in ((0, 464), (100, 2), (100, 33)):
        assert HB.run_host(variant_check, "sinus", T, D, os.path.join(str(tmp_path), "x.bin")).returncode == 2


def test_timestep_type_none_row_is_weight_minus_one_and_bias(variant_check, tmp_path):
    D = 48
    rng = np.random.default_rng(5)
    w, b = (1.0 + 0.1 * rng.standard_normal(D)).astype(np.float32), (0.1 * rng.standard_normal(D)).astype(np.float32)
    w[:3] = [1.0, 0.0, -1.5]
    rc, out = HB.run_host_io(variant_check, tmp_path, np.concatenate([w, b]).tobytes(), "const", D)
    assert rc == 0
    row = np.frombuffer(out, np.float32)
    assert np.array_equal(row[:D], w - np.float32(1.0)) and np.array_equal(row[D:], b)
    assert row[0] == 0.0 and row[1] == -1.0
    # x_hat * (1 + scale) + shift against nn.LayerNorm's x_hat * w + b: 1 + (w - 1) is w up to one rounding of w - 1
    assert np.abs((np.float32(1.0) + row[:D]) - w).max() <= 2.0 ** -24 * 2


# ----------------------------------------------------------------------------- the plan
def test_plan_instance_norm_is_tiled_on_exact_and_split_and_refused_elsewhere():
    for sanitize in (False, True):
        exe = HB.host_program("cpu_variant_plan_check", sanitize=sanitize, extra=("-Wextra",))
        r = HB.run_host(exe, "instance")
        print(r.stdout)
        assert r.returncode == 0 and "FAIL" not in r.stdout, r.stdout + r.stderr
    lines = r.stdout.splitlines()
    assert sum(ln.startswith("case=instance_") and "rc=0" in ln and "kernels=tiled_gemm+attn+instance_norm" in ln for ln in lines) == 8
    for name in ("fast", "mixed", "hybrid"):
        assert any(ln.endswith(f"err=precision {name}: timestep_type adainnorm / adainnorm_abs (instance norm over a layout's rows) has no "
                               "kernel in the fp16 engines; use precision split or exact") for ln in lines), name


def test_plan_of_every_existing_case_is_unchanged_with_the_default_kind():
    for sanitize in (False, True):
        exe = HB.host_program("cpu_variant_plan_check", sanitize=sanitize, extra=("-Wextra",))
        r = HB.run_host(exe, "default")
        assert r.returncode == 0 and "FAIL" not in r.stdout, r.stdout + r.stderr
        assert r.stdout.split()[-2:] == ["cases=133", "failed=0"]


# ----------------------------------------------------------------------------- what stays refused
BACKBONE = {"encoder_layer": {"d_model": 512, "nhead": 8, "dim_feedforward": 2048, "timestep_type": "adalayernorm", "diffusion_step": 100},
            "num_layers": 4}


def _backbone(timestep_type):
    return {**BACKBONE, "encoder_layer": {**BACKBONE["encoder_layer"], "timestep_type": timestep_type}}


@pytest.mark.parametrize("timestep_type", ["adalayernorm_mlp", "adainnorm_mlp"])
def test_layoutdm_refuses_the_mlp_kinds_and_says_why(timestep_type):
    from layout_dm_amd.layoutdm import LayoutDM

    with pytest.raises(NotImplementedError) as e:
        LayoutDM(_backbone(timestep_type), StubTokenizer(synthetic.RICO25), q_type="constrained")
    assert str(e.value) == (f"timestep_type={timestep_type}: not supported, and the reference cannot run it either — its embedding MLP starts "
                            "with nn.Linear(1, d_model / 2) and is fed the integer (Long) timestep, which raises a dtype error on the first "
                            "forward pass")


def test_layoutdm_refuses_aggregated_and_says_why():
    from layout_dm_amd.layoutdm import LayoutDM

    with pytest.raises(NotImplementedError) as e:
        LayoutDM(_backbone("adalayernorm"), StubTokenizer(synthetic.RICO25), transformer_type="aggregated", q_type="constrained")
    assert str(e.value) == ("transformer_type=aggregated: not supported, and the reference cannot instantiate it either — base.py:85-93 calls "
                            "CategoricalAggregatedTransformer with arguments its constructor (nn_lib.py:408-415) does not take")


def test_unknown_values_are_refused_by_name():
    from layout_dm_amd.diffusion import HipMaskAndReplaceDiffusion
    from layout_dm_amd.layoutdm import LayoutDM

    with pytest.raises(NotImplementedError, match="pos_emb=sinusoidal"):
        LayoutDM(_backbone("adalayernorm"), StubTokenizer(synthetic.RICO25), pos_emb="sinusoidal", q_type="vanilla")
    with pytest.raises(NotImplementedError, match="timestep_type=adagroupnorm"):
        LayoutDM(_backbone("adagroupnorm"), StubTokenizer(synthetic.RICO25), q_type="constrained")
    with pytest.raises(NotImplementedError, match="pos_emb=sinusoidal"):
        HipMaskAndReplaceDiffusion(n_category=25, pos_emb="sinusoidal")
    with pytest.raises(NotImplementedError, match="timestep_type=adainnorm_mlp"):
        HipMaskAndReplaceDiffusion(n_category=25, timestep_type="adainnorm_mlp")


def test_variant_name_names_only_what_is_not_the_default():
    from layout_dm_amd.diffusion import variant_name

    assert variant_name("elem_attr", "adalayernorm") is None
    assert variant_name("default", "adalayernorm") == "pos_emb=default"
    assert variant_name("elem_attr", None) == "timestep_type=None"
    assert variant_name("default", "adainnorm_abs") == "pos_emb=default, timestep_type=adainnorm_abs"


# ----------------------------------------------------------------------------- the tool
@pytest.mark.skipif(not ref_harness.reference_importable(), reason="the reference implementation is not on this machine")
def test_tool_regenerates_the_fixtures_bit_for_bit(golden_dir, tmp_path):
    for path in TOOL.main(str(tmp_path)):
        name = os.path.basename(path)[:-len(".npz")]
        old = fixture(golden_dir, name)
        with np.load(path) as z:
            new = {k: z[k] for k in z.files}
        assert sorted(new) == sorted(old)
        for k in old:
            assert new[k].dtype == old[k].dtype and np.array_equal(new[k], old[k]), (name, k)
