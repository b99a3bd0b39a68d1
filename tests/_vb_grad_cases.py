"""Shared by tests/test_vb_grad_core.py, tests/test_training_host.py and tests/test_vb_grad_gpu.py: the fixture of
tools/make_vb_grad_golden.py (the reference's own autograd gradient of its training loss with respect to the logits), the host
check program's case files and the bar."""
import dataclasses
import functools
import os

import numpy as np

from oracle import spec as SP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "vb_grad")
# name -> (dataset, q_type, bins per coordinate), as tools/make_vb_grad_golden.py has them
MODELS = {"rico25_constrained": ("rico25", "constrained", 32), "publaynet_constrained": ("publaynet", "constrained", 32),
          "rico25_vanilla": ("rico25", "vanilla", 32), "rico25b64_constrained": ("rico25", "constrained", 64)}
CASES = ("t0", "t1", "t33", "t99", "mixed", "sharp")
AUX_WEIGHT = 0.1


@functools.lru_cache(maxsize=None)
def fixture():
    with np.load(os.path.join(GOLDEN, "reference.npz")) as z:
        return {k: z[k] for k in z.files}


@functools.lru_cache(maxsize=None)
def arrays(model, case):
    """-> (logits (B,S,C) float32, the reference's float64 gradient (B,S,C))"""
    with np.load(os.path.join(GOLDEN, f"{model}.{case}.npz")) as z:
        return z["logits"], z["grad64"]


def spec_of(model):
    ds, _, n_bin = MODELS[model]
    return dataclasses.replace(SP.SPECS[ds], max_elem=int(fixture()["max_elem"]), n_bin=n_bin)


def sub_vocab(spec, q_type, attr):
    """(start, count) of the attribute's body, as ldm_create lays the vocabulary out"""
    if q_type == "vanilla":
        return 0, spec.n_class - 2
    return (0, spec.n_category) if attr == 0 else (spec.n_category + (attr - 1) * spec.n_bin, spec.n_bin)


@functools.lru_cache(maxsize=None)
def schedule_table(model):
    """float32 [8][n_attr][T + 1]: the device table's layout (ldm_kernels.h ScheduleRow)"""
    spec, q_type = spec_of(model), MODELS[model][1]
    buf = SP.schedule_buffers(spec, q_type)
    out = np.zeros((8, spec.n_attr, spec.n_step + 1), np.float32)
    for r, n in enumerate(SP.SCHEDULE_NAMES):
        for a, key in enumerate(SP.VAR_NAMES):
            v = buf[n if q_type == "vanilla" else f"{key}_{n}"]
            out[r, a, :len(v)] = v
    return out


def coefficients(model, case):
    """(B,2) float64: what layout_dm_amd.training.loss_coefficients gives the case for kl_loss + aux_loss (both upstream gradients 1)"""
    from layout_dm_amd.training import loss_coefficients

    fx, spec = fixture(), spec_of(model)
    p = f"{model}/{case}/"
    B, S = fx[p + "xt"].shape
    return loss_coefficients(fx[p + "t"], fx[p + "pt"], spec.n_step, AUX_WEIGHT, True, 1.0, 1.0, B, S)


def payload(model, x0, xt, rows, t_rows, coef, t=0):
    """the case file of cpu_vb_check (header t: what THAT program runs the batch at), then what cpu_vb_grad_check reads on"""
    spec, q_type = spec_of(model), MODELS[model][1]
    x0 = np.ascontiguousarray(x0, np.int32)
    B, S = x0.shape
    sv = [sub_vocab(spec, q_type, a) for a in range(spec.n_attr)]
    hdr = [spec.n_class, spec.n_attr, spec.pad_id, spec.mask_id, spec.n_step, t, B, S, 1]
    hdr += [s for s, _ in sv] + [0] * (8 - len(sv)) + [c for _, c in sv] + [0] * (8 - len(sv))
    raw = np.array(hdr, np.int32).tobytes() + np.array([0, 0], np.uint64).tobytes()
    raw += schedule_table(model).tobytes() + x0.tobytes()
    raw += np.ascontiguousarray(xt, np.int32).tobytes() + np.ascontiguousarray(rows, np.float32).tobytes()
    return raw + np.ascontiguousarray(t_rows, np.int32).tobytes() + np.ascontiguousarray(coef, np.float64).tobytes()


def case_payload(model, case):
    fx = fixture()
    p = f"{model}/{case}/"
    return payload(model, fx[f"{model}/x0"], fx[p + "xt"], arrays(model, case)[0], fx[p + "t"], coefficients(model, case))


def parse(raw, B, S, C, grad=True):
    """-> (error word, (B,S,C) float32 gradient or None, (4,B,S) float32 kl / nll / aux / hit, (B,4) float64 sums)"""
    raw = np.frombuffer(raw, np.uint8)
    ng, nt = (B * S * C * 4 if grad else 0), 4 * B * S * 4
    g = raw[4:4 + ng].view(np.float32).reshape(B, S, C) if grad else None
    return (int(raw[:4].view(np.int32)[0]), g, raw[4 + ng:4 + ng + nt].view(np.float32).reshape(4, B, S),
            raw[4 + ng + nt:].view(np.float64).reshape(B, 4))


def bars(model, case):
    """(B,S,1): 4 x the row's recorded float32-vs-float64 distance of the reference's own autograd (the convention of
    _vb_cases.bar: our float32 evaluation makes the same kind and number of roundings); where that distance is exactly 0, the
    smallest positive recorded distance of the file."""
    fx = fixture()
    d = fx[f"{model}/{case}/row_dist"]
    return np.where(d > 0, 4.0 * d, float(fx["zero_floor"]))[..., None]


def share_of_bar(got, model, case):
    """max over the elements of |got - reference float64 gradient| / bar"""
    return float((np.abs(got.astype(np.float64) - arrays(model, case)[1]) / bars(model, case)).max())
