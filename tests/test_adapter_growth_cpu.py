"""CPU: what tests/test_gpu_adapter_growth.py relies on, pinned on the oracle and the host alone:
the capacity setter's contract (it needs no device), the top-2 margin rule on every oracle step the
GPU ids are held to, and the row schedules under which the adapter buffers grow where the GPU
tests assert that they did."""
import ctypes

import pytest

import adapter_growth_ref as R

pytestmark = pytest.mark.cpu


def test_new_symbols_are_exported():
    import vox_hip
    lib = ctypes.CDLL(vox_hip.LIB_PATH)
    for n in ("vox_hip_set_adapter_rows0", "vox_hip_stream_adapter_stats"):
        assert hasattr(lib, n) and n in vox_hip.EXPORTS, n
    host = ctypes.CDLL(vox_hip.HOST_LIB_PATH)
    for n in ("vh_sched_debug_fail_next_encode", "vh_stream_adapter_stats"):
        assert hasattr(host, n), n


def test_setter_takes_powers_of_two_from_16_to_1024_without_a_device():
    """0 (the default) and 16, 32, ..., 1024 are accepted; everything else is an error reported
    through vox_hip_last_error that names the value.  No GPU call: this runs on a CPU-only host."""
    import vox_hip
    L = vox_hip.lib()
    try:
        for ok in (0, 16, 32, 64, 128, 256, 512, 1024, 0):
            L.vox_hip_clear_error()
            assert L.vox_hip_set_adapter_rows0(ok) == 0, ok
            assert not L.vox_hip_last_error()
        for bad in (-1, 1, 8, 15, 17, 24, 48, 1000, 1023, 1025, 2048, 1 << 20, -1024):
            L.vox_hip_clear_error()
            assert L.vox_hip_set_adapter_rows0(bad) == -1, bad
            assert str(bad).encode() in L.vox_hip_last_error(), (bad, L.vox_hip_last_error())
            with pytest.raises(RuntimeError, match="adapter rows0"):
                vox_hip.set_adapter_rows0(bad)
        vox_hip.set_adapter_rows0(64)
        assert L.vox_hip_set_adapter_rows0(48) == -1   # a refused value leaves the setting alone ...
        assert L.vox_hip_set_adapter_rows0(64) == 0    # ... (read back on the GPU by the streams' stats)
    finally:
        assert L.vox_hip_set_adapter_rows0(0) == 0


def test_single_schedule_rows_and_margin():
    """the ragged schedule: 44 rows after the first chunk (more than 16, with no prompt row before
    it), 296 in the end, crossing 64, 128 and 256 on the way; 258 steps, each with a top-2 gap of
    at least 4 x the logit bar"""
    ref = R.single_oracle()
    rows = ref["rows"]
    assert rows[0] == 44 and rows[-1] == 296 and len(ref["ids"]) == 258
    caps, cap = [], 16
    for r in rows:
        if r > cap:
            while cap < r:
                cap *= 2
            caps.append(cap)
    assert caps == [64, 128, 256, 512]
    assert R.worst_margin(ref["logits"]) >= R.MARGIN, R.worst_margin(ref["logits"])


@pytest.mark.parametrize("name", list(R.BEGUN))
def test_begun_cases_rows_and_margin(name):
    """every member starts below 64 rows with more than 16 steps left (two chunks), the growing
    ones cross 64 with their next 10 rows, and every oracle step keeps the margin"""
    n, cap, grow, _, alts, _ = R.BEGUN[name]
    ref = R.begun_oracle(name)
    assert len(ref) == n <= cap and len(grow) == 2
    for i, x in enumerate(ref):
        rows = R.begun_rows(i)
        assert rows <= 64 and len(x["start"]) == 1
        assert len(x["call"]) == rows - (33 + R.begun_delay(name, i)) > R.STEP_BATCH
        assert len(x["call"]) <= R.BEGUN_STEPS
        assert len(x["drain"]) == (R.GROW_ROWS if i in grow else 0)
        assert (rows + R.GROW_ROWS > 64) and x["adapter"].shape[0] == rows + (R.GROW_ROWS if i in grow else 0)
    m = min(R.worst_margin(x["logits"]) for x in ref)
    assert m >= R.MARGIN, m
    if alts:
        import vox_oracle
        for i in alts:
            ids = ref[i]["start"] + ref[i]["call"] + ref[i]["drain"]
            acc = sum(vox_oracle.fill_alts(l, t, 3, 0.5)[0][1] >= 0 for l, t in zip(ref[i]["logits"], ids))
            assert acc >= 3, (i, acc)


def test_scheduler_row_schedule_grows_inside_begun_calls(jfk_samples):
    """the served case on the host: from the oracle sessions' rows after each 4 s feed, every
    stream has at least one run that begins more than 16 steps and whose pass then outgrows the
    buffer (128 -> 256 at the second feed)"""
    ref = R.sched_oracle(jfk_samples)
    hits = R.sched_row_schedule([rows for _, rows in ref])
    for k, h in enumerate(hits):
        assert h and all(steps > R.STEP_BATCH for steps, _, _ in h), (k, h)
        assert h[0] == (R.SCHED_STEP_CAP, 128, 256), (k, h)
    for ids, rows in ref:
        assert len(ids) > 100 and 2 not in ids and rows[0] > R.SCHED_CAP0
