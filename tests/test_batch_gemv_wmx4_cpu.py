"""CPU: the public names of the R-row GEMV step's wmx4 switch, and the margin rule of every oracle
comparison tests/test_gpu_batch_gemv_wmx4.py makes.

An id comparison against the oracle only means something where the oracle's own top-2 gap
exceeds what the logit tolerance allows.  So for every case in that file's CASES, on the oracle
alone over the MXFP4-rounded weights and with no step left out: (top1 - top2) / max|logit| is at
least 4x the logit bar, 2e-4 for f32 rings and 4e-4 for half rings.  The FP8-ring case is held to
2e-4 on the reference session of tests/kv8_ref.py with the FP8 rounding at the K/V append (the
session the GPU test replays ring-conditioned, where it asserts the same rule on the replay
itself).  The worst gap of each case is printed."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests"))
import test_gpu_batch_gemv_wmx4 as t  # noqa: E402  (the cases and the oracle sessions; nothing runs on a GPU)

pytestmark = pytest.mark.cpu
NAMES = ["vox_hip_batch_set_gemv_wmx4", "vox_hip_batch_gemv_wmx4_stats"]


def test_header_library_and_binding_have_the_names():
    import vox_hip
    inc = os.path.join(ROOT, "include")
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(inc, "voxtral_hip.h")).read(), flags=re.S)
    lib = ctypes.CDLL(vox_hip.LIB_PATH)
    for n in NAMES:
        assert re.search(r"\bint\s+%s\s*\(" % n, src), n
        assert hasattr(lib, n), n
        assert n in vox_hip.EXPORTS, n
    assert callable(vox_hip.Batch.set_gemv_wmx4) and callable(vox_hip.Batch.gemv_wmx4_stats)
    # the C host's setters
    host = re.sub(r"/\*.*?\*/", "", open(os.path.join(inc, "vox_hip_host.h")).read(), flags=re.S)
    hlib = ctypes.CDLL(os.path.join(os.path.dirname(vox_hip.LIB_PATH), "libvox_hip_host.so"))
    for n in ("vh_sched_set_gemv_rows", "vh_sched_set_gemv_wmx4"):
        assert re.search(r"\bint\s+%s\s*\(" % n, host), n
        assert hasattr(hlib, n), n


def _gaps(lg):
    top = np.partition(lg, -2, axis=1)[:, -2:]
    return (top[:, 1] - top[:, 0]) / np.max(np.abs(lg), axis=1)


@pytest.mark.parametrize("case", sorted(c for c in t.CASES if t.CASES[c][4] != "fp8"))
def test_oracle_margin(case):
    _, kind, sizes, _, ring = t.CASES[case]
    margin = t.MARGIN_KV16 if ring == "f16" else t.MARGIN_F32
    ref = t._oracle(case)
    assert len(ref) == len(sizes)
    worst, steps = np.inf, 0
    for i, (ids, lg) in enumerate(ref):
        assert len(ids) == lg.shape[0] >= 6, (case, i, len(ids))   # six single steps are read
        gap = _gaps(lg)
        assert np.array_equal(np.argmax(lg, axis=1), np.asarray(ids)), (case, i)
        k = int(np.argmin(gap))
        assert gap[k] >= margin, (case, i, k, float(gap[k]), margin)
        worst = min(worst, float(gap[k]))
        steps += len(ids)
    print(f"{case}: oracle top-2 gap >= {worst:.2e} of the largest logit over {steps} steps "
          f"(rule: {margin:.0e}); tokens per stream {[len(ids) for ids, _ in ref]}")


def test_rounded_weights_differ_and_are_a_fixed_point():
    """the `rounded` weights are not the plain ones (the oracle comparisons are about the rounded
    model), rounding them again changes nothing, and `mixed` differs from them in one tensor"""
    from vox_weights import mxfp4_round, mxfp4_tensor_names
    plain, rounded, mixed = (t._weights("kv8", k) for k in ("plain", "rounded", "mixed"))
    names = mxfp4_tensor_names(t.KV8)
    assert t.UNROUNDED in names
    for n in names:
        assert not np.array_equal(plain.t[n], rounded.t[n]), n
        assert np.array_equal(mxfp4_round(rounded.t[n]), rounded.t[n]), n
        assert np.array_equal(mixed.t[n], rounded.t[n]) == (n != t.UNROUNDED), n


def test_fp8_reference_margin():
    """the FP8-ring case: the reference session with the E4M3 rounding at every K/V append, on the
    rounded weights, keeps 2e-4 on every step the GPU test takes"""
    import vox_oracle
    from kv8_ref import MARGIN, RefDecoder, kv8_hook, oracle_adapter, top2_margin
    assert MARGIN == t.MARGIN_F32 == 2e-4
    w = t._weights("kv8", "rounded")
    om = vox_oracle.OracleModel(t.KV8, w)
    try:
        worst = np.inf
        for mel, n in zip(t._case_mels("kv8_fp8_2"), t.FP8_STEPS):
            r = RefDecoder(t.KV8, w, oracle_adapter(om, mel), om.ada_scale(), round_fn=kv8_hook)
            ids, lg = r.decode(n)
            assert len(ids) == n
            m = top2_margin(lg)
            assert m >= MARGIN, (n, m)
            worst = min(worst, m)
    finally:
        om.close()
    print(f"kv8_fp8_2: FP8 reference top-2 gap >= {worst:.2e} over {sum(t.FP8_STEPS)} steps (rule: {MARGIN:.0e})")
