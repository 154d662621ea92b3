"""The per-GPU scheduler past 32 streams (VH_SCHED_MAX 128): 64 streams on one vh_sched_t, their
deferred chunks encoded in groups of 32 (the library's per-pass limit) and their rows decoded by
the wide batched step."""
import numpy as np
import pytest

from test_gpu_sched import _serve, _single_stream_ids

pytestmark = pytest.mark.gpu


def test_scheduler_64_streams_match_single_stream(tiny_weights, jfk_samples):
    """64 TINY_LONG streams of 6-8 s on one Scheduler(ctx, 64): 16 start per tick, so all 64 are
    live together, a step cap of 8 as bench.py --stagger (as the 32-stream test of
    tests/test_gpu_sched.py).  Every stream's ids equal the same pieces through the
    single-stream path; the stats show batched encoder passes, stacked prefills and more than 32
    rows per batched step on average."""
    import vox_hip
    from vox_weights import TINY_LONG
    hm = vox_hip.Model(TINY_LONG, tiny_weights)
    long = np.concatenate([jfk_samples] * 2)
    audios = []
    for k in range(64):
        n = int(16000 * (6.0 + 0.5 * (k % 5)))
        off = (k * 7919) % (len(long) - n)
        audios.append(np.ascontiguousarray(long[off:off + n]))
    ids, st = _serve(hm, audios, [k // 16 for k in range(64)], 0.5, max_streams=64, step_cap=8)
    ctx = vox_hip.HostCtx(hm)
    for k, a in enumerate(audios):
        ref = _single_stream_ids(ctx, a, 0.5)
        assert len(ref) > 20, (k, len(ref))
        assert ids[k] == ref, (k, len(ids[k]), len(ref))
    ctx.close()
    hm.close()
    print("64-stream scheduler stats", st)
    assert st["enc_batches"] > 0 and st["prefill_passes"] >= 3, st
    assert st["tokens"] / max(1, st["steps"]) > 32, st
