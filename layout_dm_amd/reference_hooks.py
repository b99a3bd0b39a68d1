"""What the drop-in model class brings along when it runs inside the reference's own `trainer.test.main()`.

`python -m layout_dm_amd.test_entry` swaps `trainer.models.layoutdm.LayoutDM` for `layout_dm_amd.layoutdm.LayoutDM` and
calls the reference's `main()`; hydra then builds the drop-in class (test.py:113-118).  Besides sampling, that `main()`
scores every cond=relation batch with `compute_violation` (trainer/helpers/metric.py:62-95, called at test.py:230-254), a
Python loop over the edges that costs more than drawing the batch.  `install_violation_dropin()` — called by the drop-in
class's constructor — puts `layout_dm_amd.metrics.compute_violation` (kernels_violation.hip, equal to the reference's
function bit for bit) in its place for that entry point.

Only where the class swap was made and a GPU is present: without the swap (`_target_: layout_dm_amd.layoutdm.LayoutDM` in a
user's own script) or without a device nothing is touched.  What is installed asks `torch.cuda.is_available()` again on
every call and hands the call to the reference's own function when there is no device, so a later run of the reference's
class on the host in the same process is scored by the reference."""
from __future__ import annotations

import sys

import torch


def install_violation_dropin(model_class) -> bool:
    """trainer.test.compute_violation -> the device drop-in, if `model_class` is what trainer.models.layoutdm.LayoutDM now
    names.  Returns whether trainer.test carries the drop-in afterwards."""
    ref_layoutdm, ref_test = sys.modules.get("trainer.models.layoutdm"), sys.modules.get("trainer.test")
    if ref_layoutdm is None or ref_test is None or getattr(ref_layoutdm, "LayoutDM", None) is not model_class:
        return False
    current = getattr(ref_test, "compute_violation", None)
    if current is None:
        return False
    if getattr(current, "reference", None) is not None:
        return True          # already installed
    if not torch.cuda.is_available():
        return False

    def compute_violation(bbox_flatten, data):
        if not torch.cuda.is_available():
            return current(bbox_flatten, data)
        from . import metrics

        return metrics.compute_violation(bbox_flatten, data)

    compute_violation.reference = current
    ref_test.compute_violation = compute_violation
    return True
