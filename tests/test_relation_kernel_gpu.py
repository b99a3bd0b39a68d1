"""GPU: ONE relation_update_k launch (layout_dm_amd/csrc/kernels_relation.hip — the SGD of the cond=relation logit adjustment, whose arithmetic
csrc/ldm_relation_core.h shares with relation_step_k and the relation form of the one-launch loop kernel) on the test's buffers, through the
development hook ldm_dev_relation_run (csrc/ldm_dev.cpp), against the float64 restatement of the reference's update (tests/_relation_cases.py).
No engine is created, except for the window check at the end.  tests/test_relation_reference.py pins cases, margins and bars on the CPU.

  * metric: per row (layout, element, coordinate), max over bins |out - ref64| divided by the row's path length, max over bins of the sum
    over iterations of |delta| in float64 (net updates cancel); the worst row of the case is held to the bar;
  * bar: 4 x the same quantity of the float32 emulation of the case (the larger of its two evaluations: tests/_relation_cases.py bar);
    nothing is taken from the device; 0 where nothing moves;
  * the buffer holds one layout more than B and 64 words behind it, and every word the kernel must not touch — category positions, classes
    outside the body bins, all rows of non-node elements, the layout past B, the tail — holds a NaN pattern: all come back bit for bit,
    and no NaN remains inside a node's body bins; rows of nodes whose gradient is zero come back bit for bit as well;
  * logp_tm = 0 (B, C, S) and logp_tm = 1 (B, S, C) of the same case agree bit for bit;
  * 528 edges in one layout and the same graph as 512 + 16 edges in two layouts are each held to float64; 512 edges plus a 513th edge
    unknown | unknown (the scan path of the node sums) equals the 512-edge graph (the incidence lists) bit for bit;
  * Engine.relation_update: a plan of 6 layouts run as two windows of 3 equals the one call of 6 bit for bit; t = 9 changes nothing.

Measured on the MI355X, worst row of a case in path lengths (the printed table and every case: profiles/relation_alone_check.txt):

  family          cases (x 2 layouts)   measured              bar
  one edge           37                 0 .. 4.8e-5           0 .. 1.7e-4      (the 14 inactive-hinge cases: 0 of 0, the whole buffer bit for bit)
  zero argument       8                 0                     0 .. 1.8e-6      (a hinge argument of exactly 0: less() active by its eps, less_equal() not)
  geometry           10                 6.6e-7 .. 4.6e-5      3.7e-6 .. 4.0e-4
  node mapping        5                 1.1e-6 .. 4.6e-5      4.2e-6 .. 1.7e-4
  edges              10 + 1             0 .. 1.3e-5           0 .. 7.1e-5      (512 + 1 unknown edge == 512 edges bit for bit)
  iterations          3                 2.2e-6 .. 4.5e-5      1.1e-5 .. 1.2e-4 (num_update 0: the buffer bit for bit)
  windows             1                 1.5e-5                5.9e-5           (two windows of 3 == one call of 6 bit for bit)

Closest to a bar: iter-4 4.46e-5 of 8.67e-5, geo-E30-NB32 1.43e-5 of 3.59e-5, one-sm-canvas-on 3.44e-6 of 1.05e-5; the values are bit-repeatable.  No case
exposed a fault.  The emulation's figure is the larger of its two float32 evaluations (tests/_relation_cases.py bar says why); with the analytic one
alone one-sm-canvas-on is outside its bar, 3.44e-6 against 3.20e-6, and every other case inside.

Mutation check, by hand, in csrc/ldm_relation_core.h (figures in path lengths):
  1. the 0.5f on gs[2] removed: 31 cases fail at 0.94 .. 48 (1.5e4 .. 1.5e6 x their bars) — one-left-on, one-right-on, one-center-1-on, one-center-2-on,
     zero-center-1, zero-center-2, nine of the ten geometry cases, map-no-element, map-node-without-edge, map-all-32-nodes, edges-one .. edges-1056, iter-1 / 2 / 4 — and
     the scan-order and windows tests.  tests/test_hip_parity.py::test_relation_update_vs_reference_and_oracle fails too.
  2. the eps of `(l1 - r2) + eps > 0.f` dropped: zero-center-1 fails at 1.0 (bar 1.8e-6) and nothing else — a case with a margin cannot see 1e-8.
     test_relation_update_vs_reference_and_oracle passes.
  3. the incidence loop stopping one entry early: 51 cases fail at 1.0 .. 36 (5.9e3 .. 1.6e6 x their bars), every case with an active hinge and at most 512 edges per
     layout, and the scan-order and windows tests; edges-513, edges-528 and edges-1056 take the scan path and pass.  test_relation_update_vs_reference_and_oracle fails too.
"""
import ctypes
import dataclasses

import numpy as np
import pytest
import torch

import _relation_cases as RC

pytestmark = pytest.mark.gpu

VP, I32, I64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64


class RelIo(ctypes.Structure):     # csrc/ldm_dev.cpp ldm_dev_relation_io
    _fields_ = [(n, VP) for n in ("logp", "cond_seq", "edge_off", "edge_src", "edge_dst", "edge_attr", "centres")] + \
               [("canvas_bins", I32 * 4), ("step", ctypes.c_float)] + \
               [(n, I32) for n in ("num_update", "B", "C", "S", "A", "n_category", "n_bin", "pad_id", "logp_tm")] + \
               [(n, I64) for n in ("logp_floats", "n_cond", "n_edge_off", "n_edge", "n_centres")]


@pytest.fixture(scope="module")
def lib():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a ROCm device (no CPU fallback exists)")
    from layout_dm_amd import binding

    L = binding.load_library()
    L.ldm_dev_relation_run.argtypes, L.ldm_dev_relation_run.restype = [ctypes.POINTER(RelIo)], ctypes.c_int
    torch.cuda.set_device(0)
    return L


def _dev(a):
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint32:
        a = a.view(np.int32)
    return torch.from_numpy(a).cuda()


def guarded_input(case):
    """(B + 1, C, S) uint32: the NaN pattern everywhere but the body bins of the nodes' coordinate positions"""
    words = np.full((case.B + 1, case.C, case.S), RC.NAN32, np.uint32)
    m = RC.body_mask(case)
    words[:case.B][m] = RC.logp(case).view(np.uint32)[m]
    return words


def launch(lib, case, tm, expect=0, **override):
    """-> the whole buffer after the launch as (B + 1, C, S) uint32 words (token-major buffers transposed back), the tail's words"""
    words = guarded_input(case)
    flat = (words.transpose(0, 2, 1) if tm else words).reshape(-1)
    buf = _dev(np.concatenate([flat, np.full(RC.TAIL, RC.NAN32, np.uint32)]))
    off, src, dst, attr = RC.csr(case)
    keep = [_dev(RC.cond_seq(case)), _dev(off), _dev(src), _dev(dst), _dev(attr), _dev(RC.centres(case.NB).astype(np.float32))]
    ptr = lambda t: t.data_ptr() if t.numel() else None
    io = RelIo(logp=buf.data_ptr(), cond_seq=ptr(keep[0]), edge_off=ptr(keep[1]), edge_src=ptr(keep[2]), edge_dst=ptr(keep[3]), edge_attr=ptr(keep[4]),
               centres=ptr(keep[5]), canvas_bins=(I32 * 4)(*RC.canvas_bins(case.NB)), step=float(np.float32(case.lr) / (np.float32(14.0) * np.float32(case.graphs))),
               num_update=case.num_update, B=case.B, C=case.C, S=case.S, A=RC.A, n_category=case.n_category, n_bin=case.NB, pad_id=case.pad_id, logp_tm=tm,
               logp_floats=(case.B + 1) * case.C * case.S, n_cond=case.B * case.S, n_edge_off=case.B + 1, n_edge=len(src), n_centres=4 * case.NB)
    for k, v in override.items():
        setattr(io, k, v)
    torch.cuda.synchronize()
    rc = lib.ldm_dev_relation_run(ctypes.byref(io))
    if rc == -2:    # a HIP error: nothing more runs on this device from this module
        pytest.exit(f"{case.id}: HIP error", returncode=3)
    assert rc == expect, (case.id, rc)
    got = buf.cpu().numpy().view(np.uint32)
    body = got[:-RC.TAIL].reshape((case.B + 1, case.S, case.C) if tm else (case.B + 1, case.C, case.S))
    return (body.transpose(0, 2, 1) if tm else body).copy(), got[-RC.TAIL:]


MEASURED = {}   # case id -> (family, error, bar, where)


def check(case, words, tail, note=""):
    """Every figure printed before it is asserted"""
    start = guarded_input(case)
    m, still = RC.body_mask(case), RC.still_mask(case)
    out = words[:case.B].view(np.float32)
    err, where = RC.row_error(case, out.astype(np.float64))
    bar = RC.bar(case)
    bad = []
    if not np.array_equal(words[:case.B][~m], start[:case.B][~m]):
        bad.append("a word outside the nodes' body bins")
    if not (words[case.B] == RC.NAN32).all():
        bad.append("the layout past B")
    if not (tail == RC.NAN32).all():
        bad.append("the tail")
    if not np.array_equal(words[:case.B][still], start[:case.B][still]):
        bad.append("a row whose gradient is zero")
    if np.isnan(out[m]).any():
        bad.append("a NaN inside a node's body bins")
    MEASURED[case.id + note] = (case.family, err, bar, where)
    print(f"{case.id + note:34s} edges {str(case.n_edges):16s} worst row {err:.2e} at {where} (bar {bar:.2e})" + (f"  TOUCHED: {bad}" if bad else ""), flush=True)
    assert not bad, bad
    assert err <= bar, (case.id, err, bar)
    if not (RC.reference(case).path > 0).any():      # nothing moves: the whole buffer, bit for bit
        assert np.array_equal(words, start)


CASES = RC.cases()


@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_relation_update_against_float64(lib, case):
    a, tail_a = launch(lib, case, 0)
    b, tail_b = launch(lib, case, 1)
    check(case, a, tail_a)
    check(case, b, tail_b, note=" (token-major)")
    assert np.array_equal(a, b)        # the arithmetic is the same behind the load


def test_no_update_is_a_no_op(lib):
    case = RC.noop_case()
    for tm in (0, 1):
        words, tail = launch(lib, case, tm)
        assert np.array_equal(words, guarded_input(case)) and (tail == RC.NAN32).all()


def test_scan_path_sums_in_the_order_of_the_incidence_lists(lib):
    """513 edges take the scan of all edges per node, 512 the incidence lists; both sum a node's entries in ascending edge order"""
    c512, c513 = RC.case("edges-512"), RC.edge_513_with_dead_last()
    assert c513.n_edges == [513] and np.array_equal(RC.logp(c512), RC.logp(c513))
    a, _ = launch(lib, c512, 0)
    b, tail = launch(lib, c513, 0)
    check(c513, b, tail)
    assert np.array_equal(a, b)


def test_the_hook_refuses_what_the_kernel_forbids(lib):
    """-1 before any launch: the buffers are real, only the stated precondition is broken; the buffer comes back untouched"""
    case = RC.case("map-pad-between-nodes")
    start = guarded_input(case)

    def refused(**kw):
        words, tail = launch(lib, case, 0, expect=-1, **kw)
        return np.array_equal(words, start) and (tail == RC.NAN32).all()

    assert refused(S=case.S + 1) and refused(A=4) and refused(n_bin=33) and refused(C=case.n_category + 4 * case.NB - 1)
    assert refused(logp_floats=case.B * case.C * case.S - 1) and refused(n_cond=case.B * case.S - 1) and refused(n_edge_off=case.B)
    assert refused(n_edge=sum(case.n_edges) - 1) and refused(n_centres=4 * case.NB - 1) and refused(logp_tm=2) and refused(num_update=-1)
    assert refused(canvas_bins=(I32 * 4)(16, 16, 32, 31)) and refused(canvas_bins=(I32 * 4)(-1, 16, 31, 31))
    wide = dataclasses.replace(case, E=33, cats=tuple(c + (-1,) * 25 for c in case.cats))          # 33 elements
    launch(lib, wide, 0, expect=-1)
    n0 = len(RC.nodes_of(case, 0))
    for bad_edge in ((n0 + 1, 1, RC.UNKNOWN), (1, -1, RC.UNKNOWN)):                                 # a node id past the layout's nodes
        c = dataclasses.replace(case, edges=(case.edges[0] + (bad_edge,), case.edges[1]))
        launch(lib, c, 0, expect=-1)
    off = RC.csr(case)[0].copy()
    off[1] = off[2] + 1                                                                              # offsets that decrease
    t = _dev(off)
    assert refused(edge_off=t.data_ptr())
    assert lib.ldm_dev_relation_run(None) == -1
    launch(lib, case, 0)                                                                             # (and the unbroken arguments run)


def test_windows_of_a_plan_equal_the_whole_call(lib):
    """Engine.relation_update on layouts 0 .. 2 and 3 .. 5 of a plan of 6 == the one call of 6, bit for bit: the step is the plan's
    (relation_lambda / (14 x 6)) and the edge offsets of a window are absolute.  t = 9: no update (logit_adjustment.py:107)."""
    from layout_dm_amd.binding import Engine

    case = RC.windows_case()
    eng = Engine(n_category=25, n_bin=32, max_elem=25, d_model=64, n_head=2, d_ff=64, n_layer=1, n_step=100, precision="exact", max_batch=8)
    rel = eng.make_relation(RC.oracle_graph(case), RC.centres(32), RC.canvas_bins(32), case.lr, case.num_update, 6)
    seq = torch.from_numpy(RC.cond_seq(case).astype(np.int64))
    start = torch.from_numpy(RC.logp(case).copy()).cuda()
    whole = eng.relation_update(start.clone(), seq, rel, 40)
    parts = torch.cat([eng.relation_update(start[lo:lo + 3].clone().contiguous(), seq[lo:lo + 3], rel, 40, layout_offset=lo) for lo in (0, 3)])
    assert torch.equal(whole.view(torch.int32), parts.view(torch.int32)) and not torch.equal(whole, start)
    err, where = RC.row_error(case, whole.cpu().numpy().astype(np.float64))
    print(f"windows: worst row {err:.2e} at {where} (bar {RC.bar(case):.2e})")
    assert err <= RC.bar(case)
    assert torch.equal(eng.relation_update(start.clone(), seq, rel, 9).view(torch.int32), start.view(torch.int32))


def test_print_the_measured_table():
    """(last: what profiles/relation_alone_check.txt holds)"""
    print("\nfamily          cases   measured (worst row)    bar                     closest to its bar")
    fams = {}
    for cid, (fam, err, bar, where) in MEASURED.items():
        fams.setdefault(fam, {})[cid] = (err, bar)
    for fam, m in fams.items():
        errs, bars = [v[0] for v in m.values()], [v[1] for v in m.values()]
        worst = max(m, key=lambda k: m[k][0] / m[k][1] if m[k][1] else 0.0)
        print(f"{fam:14s}  {len(m):5d}   {min(errs):.1e} .. {max(errs):.1e}    {min(bars):.1e} .. {max(bars):.1e}    {worst} ({m[worst][0]:.2e} of {m[worst][1]:.2e})")
    assert MEASURED
