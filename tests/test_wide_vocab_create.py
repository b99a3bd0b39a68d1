"""CPU: ldm_create's vocabulary rule (include/ldm_hip.h).  The reference-precision engines (exact, split) accept up to 128
bins per coordinate and 576 classes; the fp16 engines (fast, mixed, hybrid) stop at 192 classes and say so by name.  Every
refusal happens before a device is probed; an accepted geometry then stops, on a machine without a GPU, at the device probe."""
import ctypes

import pytest

import _wide_vocab as WV


@pytest.fixture(scope="module")
def lib():
    from layout_dm_amd import binding, build

    build.build(verbose=False)
    return binding.load_library()


def _create(lib, *, n_category, n_bin, precision, max_elem=4, d_model=64, n_head=4, d_ff=128, n_layer=2, n_step=10):
    from layout_dm_amd import binding

    cfg = binding.LdmConfig(binding.ABI_VERSION, n_category, n_bin, max_elem, 5, d_model, n_head, d_ff, n_layer, n_step,
                            binding.PRECISIONS[precision], 4, 0, 0, 0)
    h = ctypes.c_void_p()
    rc = lib.ldm_create(ctypes.byref(cfg), 0, ctypes.byref(h))
    if rc == 0:
        lib.ldm_destroy(h)
        return 0, b""
    assert not h.value
    return rc, lib.ldm_last_error(None)


@pytest.mark.parametrize("precision", ["exact", "split"])
@pytest.mark.parametrize("n_category,n_bin", WV.VOCABS, ids=WV.VOCAB_IDS)
def test_reference_precision_engines_accept_wide_vocabularies(lib, precision, n_category, n_bin):
    import torch

    rc, msg = _create(lib, n_category=n_category, n_bin=n_bin, precision=precision)
    if torch.cuda.is_available():
        assert rc == 0, msg
    else:  # validation passed: the next stop is the device probe
        assert rc == -1 and b"no HIP device" in msg, msg


@pytest.mark.parametrize("precision", ["exact", "split"])
def test_reference_backbone_at_64_bins_passes_validation(lib, precision):
    import torch

    rc, msg = _create(lib, n_category=25, n_bin=64, precision=precision, max_elem=25, d_model=464, n_head=8, d_ff=1856,
                      n_layer=4, n_step=100)
    assert (rc == 0) if torch.cuda.is_available() else (rc == -1 and b"no HIP device" in msg), msg


@pytest.mark.parametrize("precision", ["exact", "split", "fast", "mixed", "hybrid"])
def test_more_than_128_bins_and_576_classes_are_refused_by_name(lib, precision):
    rc, msg = _create(lib, n_category=1, n_bin=129, precision=precision)        # 519 classes: only the bins are too many
    assert rc == -1 and b"n_bin" in msg and b"128" in msg, msg
    rc, msg = _create(lib, n_category=63, n_bin=128, precision=precision)       # 577 classes
    assert rc == -1 and b"577 classes" in msg and b"576" in msg and b"n_category" in msg, msg


@pytest.mark.parametrize("precision", ["fast", "mixed", "hybrid"])
def test_fp16_engines_refuse_wide_vocabularies_and_point_to_split(lib, precision):
    rc, msg = _create(lib, n_category=25, n_bin=64, precision=precision, max_elem=25, d_model=464, n_head=8, d_ff=1856,
                      n_layer=4, n_step=100)
    assert rc == -1 and b"192 classes" in msg, msg
    assert b"precision " + precision.encode() in msg and b"split" in msg and b"exact" in msg and b"283" in msg, msg
    # 192 classes exactly is not wide: the fp16 engines take it as before (and stop at the device probe or at their own geometry rule)
    rc, msg = _create(lib, n_category=62, n_bin=32, precision=precision)
    assert b"192 classes" not in msg, msg
