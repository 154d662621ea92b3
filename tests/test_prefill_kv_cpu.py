"""CPU: the public name of the stacked prefill's switch, and the margin rule of every oracle
comparison tests/test_gpu_prefill_kv.py makes over half rings.

An id comparison against the oracle only means something where the oracle's own top-2 gap
exceeds what the logit tolerance allows.  So for every half-ring case of that file (HALF: the
KV8, TINY and Q8 TINY batches; SERVED: the scheduler's audio sessions), on the oracle alone under
set_kv_fp16(True) and with no step left out: (top1 - top2) / max|logit| is at least 4 x 1e-4.
The FP8 cases replay RUNS of tests/kv8_ref.py, whose margin tests/test_kv8_cpu.py pins.  The
worst gap of each case is printed."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests"))
import test_gpu_prefill_kv as t  # noqa: E402  (the cases and the oracle sessions; nothing runs on a GPU)

pytestmark = pytest.mark.cpu


def test_header_library_and_binding_have_the_name():
    import vox_hip
    n = "vox_hip_batch_set_prefill_kv"
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "voxtral_hip.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+%s\s*\(\s*vox_hip_batch_t\s*\*\s*b\s*,\s*int\s+on\s*\)" % n, src)
    assert hasattr(ctypes.CDLL(vox_hip.LIB_PATH), n)
    assert n in vox_hip.EXPORTS
    assert callable(vox_hip.Batch.set_prefill_kv)


def test_bars():
    assert t.MARGIN_KV16 == 4e-4 and t.LOGIT_TOL16 == 1e-4 and t.LOGIT_TOL == 5e-5
    assert t.NP + 1 == 1 + 32 + 6      # the prompt: BOS, 32 pads, the 6 delay tokens


@pytest.mark.parametrize("case", sorted(t.HALF))
def test_half_oracle_margin(case):
    ref = t.half_oracle(case)
    assert [len(ids) for ids, _ in ref] == t.HALF[case][3]
    t._assert_margin(ref, f"half {case}")


def test_served_oracle_margin(jfk_samples):
    """the five audio sessions of the served test: the gap on every step, no EOS (the sessions
    stop at one), and prompts that complete two per tick, so that streams can share a pass"""
    audios = t.served_audios(jfk_samples)
    assert len(audios) == len(t.SERVED_STARTS) == 5
    om = t._oracle_model("TINY_LONG")
    try:
        ref = [t.served_oracle(om, a) for a in audios]
    finally:
        om.close()
    for ids, lg in ref:
        assert len(ids) == lg.shape[0] > 20 and 2 not in ids
    t._assert_margin(ref, "served half")
    assert sorted(t.SERVED_STARTS) == t.SERVED_STARTS and len(set(t.SERVED_STARTS)) < len(t.SERVED_STARTS)
    assert all(len(a) >= 2.5 * 16000 for a in audios)
    assert np.all(np.diff([o for o, _ in t.SERVED]) > 0)
