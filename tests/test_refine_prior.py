"""The cond=refinement prior on the device (ldm_refinement_prior, kernels_refine.hip) — CPU side.

The host build of the kernel's one source of index / bounds / broadcast arithmetic (csrc/ldm_refine_core.h, through
tests/cpu_refine_check.cpp, walking workgroups and threads like the kernel) against layoutdm.refinement_weak_logits, the
host function the product path used: BIT FOR BIT, compared as int32 (so that -0.0 under a negative weight counts).  Rico25
and PubLayNet; uniform / negative / gaussian tables; weights 3.0, 0.1, -3.0; every output misalignment a slice of a larger
buffer can have; the (1,S) -> B broadcast; int32 and int64 ids; the out-of-range ids -1 and C.  The same program built with
ASan + UBSan (tests/_hostbuild.py) runs the same cases.  Also: the export refusing bad arguments, the kernels' resource report
(no scratch, no atomics, 16-byte stores), and the Python functions raising without a GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import _hostbuild as HB
from _stub_tokenizer import StubTokenizer
from oracle import spec as SP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODES = ("uniform", "negative", "gaussian")
WEIGHTS = (3.0, 0.1, -3.0)


@pytest.fixture(scope="module")
def host_exe():
    return HB.host_program("cpu_refine_check")


@pytest.fixture(scope="module")
def san_exe():
    return HB.host_program("cpu_refine_check", sanitize=True)


def host_run(exe, tmp_path, seq, table, weight, B, mis=0):
    """-> (exit code, error word, (B,C,S) float32)"""
    seq = np.ascontiguousarray(seq)
    assert seq.dtype in (np.int32, np.int64) and seq.ndim == 2
    Cn, S = table.shape[0], seq.shape[1]
    rc, raw = HB.run_host_io(exe, tmp_path, np.array([seq.dtype == np.int64, seq.shape[0], B, S, Cn, mis], np.int32).tobytes() +
                             np.float32(weight).tobytes() + seq.tobytes() + np.ascontiguousarray(table, np.float32).tobytes())
    if rc != 0:
        return rc, None, None
    raw = np.frombuffer(raw, np.uint8)
    return rc, int(raw[:4].view(np.int32)[0]), raw[4:].view(np.float32).reshape(B, Cn, S)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.int32), b.view(np.int32))


def _seq_orig(spec, B, seed):
    """ids as get_cond leaves them in seq_orig: every attribute's own sub-vocabulary, [PAD] tails, ids 0 and C - 1 present"""
    g = np.random.default_rng(seed)
    seq = np.empty((B, spec.seq_len), np.int64)
    for a in range(spec.n_attr):
        ids = np.asarray(spec.full_ids(a))
        seq[:, a::spec.n_attr] = ids[g.integers(0, len(ids), (B, spec.max_elem))]
    for b in range(B):
        n = int(g.integers(1, spec.max_elem + 1))
        seq[b, n * spec.n_attr:] = spec.pad_id
    seq[0, 0], seq[-1, -1] = 0, spec.n_class - 1
    return seq


def _cases(exe, tmp_path):
    from layout_dm_amd.layoutdm import refinement_prior_table, refinement_weak_logits

    n = 0
    for spec in (SP.RICO25, SP.PUBLAYNET):
        tok = StubTokenizer(spec)
        seq = _seq_orig(spec, 3, seed=spec.n_category)
        for mode in MODES:
            table = refinement_prior_table(tok, mode, 0.1).numpy()
            for lam in WEIGHTS:
                # refinement_weak_logits negates refine_lambda for "negative"; the kernel is handed the signed weight
                cfg = {"refine_mode": mode, "refine_offset_ratio": 0.1, "refine_lambda": lam}
                signed = -lam if mode == "negative" else lam
                want = refinement_weak_logits(tok, torch.from_numpy(seq), cfg, cache={}).numpy()
                assert want.shape == (3, spec.n_class, spec.seq_len)
                if signed < 0:
                    assert np.signbit(want[want == 0]).any()          # -0.0 is in play
                for mis, dt in ((0, np.int64), (1, np.int32), (2, np.int64), (3, np.int32)):
                    rc, err, got = host_run(exe, tmp_path, seq.astype(dt), table, signed, 3, mis)
                    assert rc == 0 and err == 0, (spec.name, mode, lam, mis, rc, err)
                    assert same_bits(got, want), (spec.name, mode, lam, mis)
                    n += 1
                # duplicate_cond: one conditioning layout, five samples
                one = refinement_weak_logits(tok, torch.from_numpy(seq[1:2]), cfg, cache={}).numpy()
                for dt, mis in ((np.int64, 3), (np.int32, 0)):
                    rc, err, got = host_run(exe, tmp_path, seq[1:2].astype(dt), table, signed, 5, mis)
                    assert rc == 0 and err == 0 and same_bits(got, np.repeat(one, 5, 0)), (spec.name, mode, lam, "broadcast")
                    n += 1
        # out-of-range ids: the error word, +0.0 in their columns, every other column untouched by them
        table = refinement_prior_table(tok, "gaussian", 0.1).numpy()
        want = refinement_weak_logits(tok, torch.from_numpy(seq), {"refine_mode": "gaussian", "refine_lambda": -3.0}, cache={}).numpy()
        for bad in (-1, spec.n_class, 2 ** 32, -2 ** 40):
            for dt in (np.int32, np.int64):
                if dt == np.int32 and abs(bad) >= 2 ** 31:
                    continue
                s = seq.astype(dt)
                s[1, 7] = bad
                s[2, spec.seq_len - 1] = bad
                rc, err, got = host_run(exe, tmp_path, s, table, -3.0, 3, 1)
                assert rc == 0 and err == 1, (bad, dt, rc, err)
                w = want.copy()
                w[1, :, 7] = 0.0
                w[2, :, spec.seq_len - 1] = 0.0
                assert same_bits(got, w), (bad, dt)
                n += 1
    return n


def _geometry_cases(exe, tmp_path):
    """beyond the datasets: the smallest shapes, one float, slabs shorter than a group, several chunks per layout, and a
    sequence past kMaxStaged (tokens read in place, bad ids reported from there)"""
    g = np.random.default_rng(5)
    for Cn, S, B in ((1, 1, 1), (1, 1, 9), (2, 1, 3), (1, 3, 5), (7, 63, 3), (65, 150, 2), (192, 128, 2), (3, 1030, 2), (5, 4099, 1)):
        table = g.standard_normal((Cn, Cn)).astype(np.float32)
        seq = g.integers(0, Cn, (B, S))
        want = table[seq].transpose(0, 2, 1) * np.float32(-0.75)
        for mis in range(4):
            rc, err, got = host_run(exe, tmp_path, seq.astype(np.int64 if mis % 2 else np.int32), table, -0.75, B, mis)
            assert rc == 0 and err == 0 and same_bits(got, want), (Cn, S, B, mis, rc)
        bad = seq.copy()
        bad[B - 1, S - 1] = Cn
        rc, err, got = host_run(exe, tmp_path, bad, table, -0.75, B, 2)
        w = want.copy()
        w[B - 1, :, S - 1] = 0.0
        assert rc == 0 and err == 1 and same_bits(got, w), (Cn, S, B)
    # B = 0 writes nothing; refused arguments
    assert host_run(exe, tmp_path, np.zeros((1, 4), np.int32), np.eye(3, dtype=np.float32), 1.0, 0)[:2] == (0, 0)
    assert host_run(exe, tmp_path, np.zeros((2, 4), np.int32), np.eye(3, dtype=np.float32), 1.0, 3)[0] == 2    # B_seq not in {1, B}
    assert host_run(exe, tmp_path, np.zeros((1, 4), np.int32), np.eye(3, dtype=np.float32), 1.0, 1, mis=4)[0] == 2


def test_host_build_equals_refinement_weak_logits_bit_for_bit(host_exe, tmp_path):
    assert _cases(host_exe, tmp_path) >= 2 * (3 * 3 * 6 + 6)


def test_host_build_geometry_edges(host_exe, tmp_path):
    _geometry_cases(host_exe, tmp_path)


def test_host_build_under_address_and_undefined_sanitizers(san_exe, tmp_path):
    """the same cases, the stand-alone program as the ASan + UBSan build: a read past the ids or the table, a
    write past the output, signed overflow or a misaligned access in the index arithmetic ends the run with a non-zero code"""
    _cases(san_exe, tmp_path)
    _geometry_cases(san_exe, tmp_path)


def test_cabi_export_and_refuses_bad_arguments():
    from layout_dm_amd import binding, build

    assert "ldm_refinement_prior" in binding.EXPORTS and binding.ABI_VERSION == 5
    assert "kernels_refine.hip" in build.SOURCES
    hdr = open(os.path.join(ROOT, "include", "ldm_hip.h")).read()
    assert "#define LDM_ABI_VERSION 5" in hdr and "int ldm_refinement_prior(" in hdr
    lib = C.CDLL(build.build(verbose=False))
    vp, i32 = C.c_void_p, C.c_int
    lib.ldm_refinement_prior.argtypes = [vp, i32, i32, i32, i32, i32, vp, C.c_float, vp, vp, vp]
    d = C.c_void_p(64)   # never dereferenced: every call below is refused (or is B == 0) before it touches memory or launches

    def call(seq=d, i64=1, B_seq=4, B=4, S=125, Cn=155, table=d, w=3.0, out=d, err=d):
        return lib.ldm_refinement_prior(seq, i64, B_seq, B, S, Cn, table, w, out, err, None)

    for bad in ({"seq": None}, {"table": None}, {"out": None}, {"err": None}, {"i64": 2}, {"i64": -1}, {"B": -1}, {"S": 0},
                {"S": -5}, {"Cn": 0}, {"B_seq": 2}, {"B_seq": 0}, {"B_seq": 5}, {"out": C.c_void_p(66)}, {"seq": C.c_void_p(68)},
                {"B": 1 << 30, "B_seq": 1, "S": 1 << 20, "Cn": 1 << 20}):
        assert call(**bad) == -1, bad
    # B == 0: nothing launched, nothing touched (no device is needed), for either broadcast form
    assert call(B=0, B_seq=0, seq=None, out=None) == 0 and call(B=0, B_seq=1, out=None, err=None) == 0


def test_refine_kernels_use_no_scratch_no_atomics_and_store_16_bytes():
    asm, out, _ = HB.kernel_asm("kernels_refine.hip", resource_report=True)
    seen = 0
    for blk in re.split(r"Function Name: ", out)[1:]:
        if "refinement_prior_k" not in blk.split()[0]:
            continue
        seen += 1
        get = lambda pat: int(re.search(pat, blk).group(1))   # noqa: E731
        assert get(r"ScratchSize \[bytes/lane\]: (\d+)") == 0, blk
        assert get(r"VGPRs? Spill: (\d+)") == 0 and get(r"SGPRs? Spill: (\d+)") == 0, blk
        assert get(r"LDS Size \[bytes/block\]: (\d+)") <= 4096, blk       # kMaxStaged ids, or none
        assert get(r"Occupancy \[waves/SIMD\]: (\d+)") == 8, blk
    assert seen == 2
    bodies = re.findall(r"^(\S*refinement_prior_k\S*):[^\n]*$(.*?)^\.Lfunc_end", asm, flags=re.S | re.M)
    assert len(bodies) == 2
    for name, body in bodies:
        ins = [ln.split(";")[0].strip() for ln in body.splitlines()]
        assert any(i.startswith("global_store_dwordx4") for i in ins), name
        assert not [i for i in ins if "atomic" in i or i.startswith(("scratch_", "flat_"))], name


def test_python_api_and_no_silent_cpu_path():
    from layout_dm_amd import binding
    from layout_dm_amd.layoutdm import refinement_weak_logits, refinement_weak_logits_device

    spec = SP.RICO25
    tok = StubTokenizer(spec)
    seq = torch.from_numpy(_seq_orig(spec, 2, 0))
    cfg = {"refine_mode": "negative", "refine_offset_ratio": 0.1, "refine_lambda": 3.0}
    if torch.cuda.is_available():
        got = refinement_weak_logits_device(tok, seq, cfg, 2, {})
        assert got.is_cuda and same_bits(got.cpu().numpy(), refinement_weak_logits(tok, seq, cfg, {}).numpy())
    else:
        with pytest.raises(RuntimeError, match="no CPU path"):
            binding.refinement_prior(seq, torch.eye(spec.n_class), 3.0, 2)
        with pytest.raises(RuntimeError, match="no CPU path"):
            refinement_weak_logits_device(tok, seq, cfg, 2, {})
