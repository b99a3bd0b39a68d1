"""ldm_vb_core.h token_grad on the host (tests/cpu_vb_grad_check.cpp, the one-lane group) against the gradient the reference's own
autograd computed (tests/golden/vb_grad, tools/make_vb_grad_golden.py): every element within the bar of the reference's float64
gradient, the [MASK] column exactly 0, the sums with the bits of tests/cpu_vb_check.cpp.

Bar, per token row: 4 x that row's recorded float32-vs-float64 distance of the reference's own autograd (_vb_grad_cases.bars).
Worst share of the bar, measured on the host program (x86-64 g++ -O2 -ffp-contract=off, glibc libm): 0.250 on every model (t1,
t33, mixed, sharp; 0.247 - 0.250 at t99, 0.082 - 0.083 at t0) — a float64 evaluation rounded once is as far from the float64
reference as the nearest float32 is, which is at most the distance the reference's own float32 gradient keeps, a quarter of the bar.
"""
import numpy as np
import pytest

import _hostbuild
import _vb_cases
import _vb_grad_cases as G


@pytest.fixture(scope="module")
def exe():
    return _hostbuild.host_program("cpu_vb_grad_check")


def run_case(exe, tmp_path, model, case, mode="grad"):
    spec = G.spec_of(model)
    B, S = G.fixture()[f"{model}/{case}/xt"].shape
    rc, raw = _hostbuild.run_host_io(exe, tmp_path, G.case_payload(model, case), mode)
    assert rc == 0
    return G.parse(raw, B, S, spec.n_class, grad=mode == "grad")


@pytest.mark.parametrize("model", list(G.MODELS))
def test_gradient_within_bar_of_reference_float64(exe, tmp_path, model):
    worst = {}
    for case in G.CASES:
        err, grad, _, _ = run_case(exe, tmp_path, model, case)
        assert err == 0
        assert np.isfinite(grad).all()
        assert (grad[..., -1] == 0).all(), "the [MASK] column"
        worst[case] = G.share_of_bar(grad, model, case)
        print(f"{model}/{case}: worst share of the bar {worst[case]:.3f}")
    assert max(worst.values()) <= 1.0, worst


@pytest.mark.parametrize("model", list(G.MODELS))
def test_sums_have_the_forward_programs_bits(exe, tmp_path, model):
    """grad mode's terms and sums == the values-only path's (token_terms<true> alone); where tests/cpu_vb_check.cpp serves the
    vocabulary (C <= 192) also == that program's, run layout by layout at the layout's own t"""
    fx, spec = G.fixture(), G.spec_of(model)
    fwd = _hostbuild.host_program("cpu_vb_check") if spec.n_class <= 192 else None
    for case in G.CASES:
        _, _, tok, sums = run_case(exe, tmp_path, model, case)
        _, _, tok_v, sums_v = run_case(exe, tmp_path, model, case, "terms")
        assert np.array_equal(tok.view(np.uint32), tok_v.view(np.uint32)) and np.array_equal(sums.view(np.uint64), sums_v.view(np.uint64))
        if fwd is None:
            continue
        p = f"{model}/{case}/"
        x0, xt, t, logits = fx[f"{model}/x0"], fx[p + "xt"], fx[p + "t"], G.arrays(model, case)[0]
        for b in range(x0.shape[0]):
            raw = G.payload(model, x0[b:b + 1], xt[b:b + 1], logits[b:b + 1], t[b:b + 1], np.zeros((1, 2)), t=int(t[b]))
            n = len(raw) - 4 - 8       # cpu_vb_check's case file: without t_rows and coef
            rc, out = _hostbuild.run_host_io(fwd, tmp_path, raw[:n], "logits")
            assert rc == 0
            _, tok_f, sums_f = _vb_cases.parse_terms(out, 1, x0.shape[1])
            assert np.array_equal(tok_f[:, 0].view(np.uint32), tok[:, b].view(np.uint32)), (case, b)
            assert np.array_equal(sums_f[0].view(np.uint64), sums[b].view(np.uint64)), (case, b)


def test_refused_token_leaves_a_zero_row(exe, tmp_path):
    model, case = "rico25_constrained", "mixed"
    fx, spec = G.fixture(), G.spec_of(model)
    p = f"{model}/{case}/"
    x0 = fx[f"{model}/x0"].astype(np.int32).copy()
    x0[2, 3] = spec.mask_id
    raw = G.payload(model, x0, fx[p + "xt"], G.arrays(model, case)[0], fx[p + "t"], G.coefficients(model, case))
    rc, out = _hostbuild.run_host_io(exe, tmp_path, raw, "grad")
    assert rc == 0
    err, grad, tok, _ = G.parse(out, *x0.shape, spec.n_class)
    assert err == 2 and (grad[2, 3] == 0).all() and (tok[:, 2, 3] == 0).all()
    _, want, _, _ = run_case(exe, tmp_path, model, case)
    keep = np.ones(x0.shape, bool)
    keep[2, 3] = False
    assert np.array_equal(grad[keep].view(np.uint32), want[keep].view(np.uint32))


def test_sanitized_build_runs_clean(tmp_path):
    san = _hostbuild.host_program("cpu_vb_grad_check", sanitize=True)
    for model in G.MODELS:
        for mode in ("grad", "terms"):
            rc, raw = _hostbuild.run_host_io(san, tmp_path, G.case_payload(model, "sharp"), mode)
            assert rc == 0 and raw
    rc, _ = _hostbuild.run_host_io(san, tmp_path, G.case_payload("rico25_constrained", "t0")[:-9], "grad")
    assert rc == 2   # a short file
