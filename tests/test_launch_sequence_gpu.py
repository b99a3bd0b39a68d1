"""The launch tables of one denoiser pass (layout_dm_amd/csrc/ldm_denoise.cpp), pinned through Engine.profile().

Every numerics mode strings its kernels together in its own order; bench.py keys its roofline on the profile entry names
(KERNEL_SYMBOL, SPLIT_ / MIXED_ / HYBRID_KERNEL_SYMBOL).  Each case builds a fresh engine, switches profiling on, runs ONE
denoise_logits call over one chunk and compares the (name, launches) rows — in the order the launches first appear — with a
table written out here in terms of L = n_layer.  A host-side change that moves, drops or renames a launch fails here before it
shows up as a number.
"""
import dataclasses

import pytest
import torch

from oracle import spec as SP
from oracle import synth

pytestmark = pytest.mark.gpu

KNOBS = ("LDM_DEV", "LDM_X3_LNGEMM", "LDM_X3_ATTNOUT", "LDM_X3_HIDPANEL", "LDM_HYB_FFN", "LDM_FUSED_ATTN")

REFERENCE = SP.SPECS["rico25"]   # d_model 464, 8 heads, d_ff 1856, S = 125: the layout-resident / row-resident kernels
SMALL = dataclasses.replace(REFERENCE, name="small", d_model=256, n_head=4, d_ff=1024, n_layer=2, n_step=20)   # none of them


def stack(L):      # fast on the reference backbone: every layer and the vocabulary head in one launch
    return [("embed_stats", 1), ("layers_fused", 1)]


def tiled(L):      # LayerNorm launch -> GEMM -> attention -> GEMM -> LayerNorm -> GEMM -> GEMM, head (fast generic, exact, split without the row-resident kernels)
    return [("embed_adaln", 1), ("gemm_qkv", L), ("attention", L), ("gemm_attn_out", L), ("layernorm2", L), ("gemm_ffn1", L),
            ("gemm_ffn2", L), ("adaln", L - 1), ("layernorm_head", 1), ("gemm_head", 1)]


def row_resident(L):   # in_proj (linear2 of the previous layer as its prologue) -> attention + out_proj -> linear1 -> head (+ the last linear2)
    return [("gemm_qkv_ln", 1), ("attn_out_fused", L), ("gemm_ffn1_ln", L), ("gemm_ffn2_qkv_ln", L - 1), ("gemm_ffn2_head_ln", 1)]


def row_resident_tiled_attention(L):   # LDM_X3_ATTNOUT=0: the tiled attention + out_proj pair in the middle
    return [("gemm_qkv_ln", 1), ("attention", L), ("gemm_attn_out", L), ("gemm_ffn1_ln", L), ("gemm_ffn2_qkv_ln", L - 1),
            ("gemm_ffn2_head_ln", 1)]


def hybrid_fused(L):   # the block's plain-fp16 FFN behind the attention: two launches per layer
    return [("gemm_qkv_ln", L), ("attn_out_ffn_fused", L), ("gemm_head_ln", 1)]


ROW = "row_resident_ln_gemm+linear2_prologue+attn_out_proj_fused"
CASES = {
    # id: (geometry, precision, knobs, table, ldm_describe's `kernels`)
    "fast": (REFERENCE, "fast", {}, stack, "stack"),
    "fast_generic_geometry": (SMALL, "fast", {}, tiled, "generic16"),
    "exact": (REFERENCE, "exact", {}, tiled, "tiled_gemm+attn"),
    "split": (REFERENCE, "split", {}, row_resident, ROW),
    "mixed": (REFERENCE, "mixed", {}, row_resident, ROW),
    "hybrid": (REFERENCE, "hybrid", {}, hybrid_fused, "row_resident_ln_gemm+attn_ffn_fused_fp16+attn_out_proj_fused"),
    "split_lngemm_0": (REFERENCE, "split", {"LDM_X3_LNGEMM": "0"}, tiled, "tiled_gemm+attn"),
    "split_attnout_0": (REFERENCE, "split", {"LDM_X3_ATTNOUT": "0"}, row_resident_tiled_attention,
                        "row_resident_ln_gemm+linear2_prologue+tiled_gemm+attn"),
    "split_hidpanel_0": (REFERENCE, "split", {"LDM_X3_HIDPANEL": "0"}, row_resident, ROW),
    "hybrid_ffn_0": (REFERENCE, "hybrid", {"LDM_HYB_FFN": "0"}, row_resident, ROW),
    "split_generic_geometry": (SMALL, "split", {}, tiled, "tiled_gemm+attn"),
}


@pytest.mark.parametrize("case", sorted(CASES))
def test_one_pass_issues_the_launches_of_its_table(monkeypatch, case):
    from layout_dm_amd.binding import Engine

    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a ROCm device (no CPU fallback exists)")
    spec, precision, knobs, table, kernels = CASES[case]
    for k in KNOBS:   # the knobs are read by ldm_create: set them before it, and only in dev mode (csrc/ldm_knobs.h)
        monkeypatch.delenv(k, raising=False)
    if knobs:
        monkeypatch.setenv("LDM_DEV", "1")
        for k, v in knobs.items():
            monkeypatch.setenv(k, v)
    e = Engine(n_category=spec.n_category, n_bin=spec.n_bin, max_elem=spec.max_elem, d_model=spec.d_model, n_head=spec.n_head,
               d_ff=spec.d_ff, n_layer=spec.n_layer, n_step=spec.n_step, precision=precision, max_batch=8)
    try:
        e.load_state_dict(synth.synth_state_dict(spec, seed=1, perturb=True))
        d = e.describe()
        for k, v in knobs.items():
            assert f"{k}={v}" in d["knobs"]
        assert d["kernels"] == kernels
        tokens = torch.randint(0, spec.n_class, (5, spec.seq_len), generator=torch.Generator().manual_seed(5))
        e.set_profiling(True)
        e.denoise_logits(tokens.int(), spec.n_step // 3)
        rows = [(r["name"], r["launches"]) for r in e.profile()]
    finally:
        e.close()
    want = [(name, n) for name, n in table(spec.n_layer) if n > 0]
    print(f"[{case}] L = {spec.n_layer}: {rows}")
    assert rows == want
