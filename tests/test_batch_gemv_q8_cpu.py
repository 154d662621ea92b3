"""CPU: the Q8 R-row GEMV batched step's public names, and the margin rule of every oracle
comparison tests/test_gpu_batch_gemv_q8.py makes (the rule and the method of
tests/test_batch_gemv_cpu.py: on the oracle alone, with no step left out, (top1 - top2) /
max|logit| is at least 4x the logit bar, 2e-4 for f32 rings and 4e-4 for fp16 rings).  The
worst gap of each case is printed."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests"))
import test_gpu_batch_gemv_q8 as q  # noqa: E402  (the cases and the oracle sessions; nothing runs on a GPU)

pytestmark = pytest.mark.cpu
NAMES = ["vox_hip_batch_set_gemv_rows_q8", "vox_hip_gemv_rows_q8", "vox_hip_gemv_q8"]


def test_header_library_and_binding_have_the_names():
    import vox_hip
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "voxtral_hip.h")).read(), flags=re.S)
    lib = ctypes.CDLL(vox_hip.LIB_PATH)
    for n in NAMES:
        assert re.search(r"\bint\s+%s\s*\(" % n, src), n
        assert hasattr(lib, n), n
        assert n in vox_hip.EXPORTS, n
    assert callable(vox_hip.Batch.set_gemv_rows_q8)
    assert callable(vox_hip.gemv_rows_q8) and callable(vox_hip.gemv_q8)
    host = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "vox_hip_host.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+vh_sched_set_gemv_rows_q8\s*\(", host)
    assert hasattr(ctypes.CDLL(os.path.join(os.path.dirname(vox_hip.LIB_PATH), "libvox_hip_host.so")),
                   "vh_sched_set_gemv_rows_q8")


@pytest.mark.parametrize("case", sorted(q.CASES))
def test_oracle_margin(case):
    _, sizes, _, kv16 = q.CASES[case]
    margin = q.MARGIN_KV16 if kv16 else q.MARGIN_F32
    ref = q._oracle(case)
    assert len(ref) == len(sizes)
    worst, steps = np.inf, 0
    for i, (ids, lg) in enumerate(ref):
        assert len(ids) == lg.shape[0] >= 6, (case, i, len(ids))   # six single steps are read
        top = np.partition(lg, -2, axis=1)[:, -2:]
        gap = (top[:, 1] - top[:, 0]) / np.max(np.abs(lg), axis=1)
        assert np.array_equal(np.argmax(lg, axis=1), np.asarray(ids)), (case, i)
        k = int(np.argmin(gap))
        assert gap[k] >= margin, (case, i, k, float(gap[k]), margin)
        worst = min(worst, float(gap[k]))
        steps += len(ids)
    print(f"{case}: oracle top-2 gap >= {worst:.2e} of the largest logit over {steps} steps "
          f"(rule: {margin:.0e}); tokens per stream {[len(ids) for ids, _ in ref]}")
