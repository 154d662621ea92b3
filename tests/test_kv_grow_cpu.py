"""CPU: growing decoder K/V rings (vox_hip_model_set_kv_grow) -- the library
declares and exports the new entry points, the CLI takes --kv-grow, the numpy restatement of the
capacity schedule and of the prefix re-pitch copy (tests/kv_grow_ref.py) does what the issue
states, and the oracle sessions the GPU tests compare ids against keep the top-2 margin rule on
every step.  No GPU work here."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import kv_grow_ref as R
from conftest import ROOT
from vox_weights import TINY, TINY_LONG

pytestmark = pytest.mark.cpu

NEW = ["vox_hip_model_set_kv_grow", "vox_hip_stream_kv_slots", "vox_hip_stream_kv_bytes",
       "vox_hip_stream_kv_grow_stats", "vox_hip_stream_reserve_kv", "vox_hip_batch_kv_grow_stats"]


def test_abi_declares_and_exports_the_kv_grow_calls():
    import vox_hip
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "voxtral_hip.h")).read(), flags=re.S)
    lib = ctypes.CDLL(vox_hip.LIB_PATH)
    for n in NEW:
        assert re.search(r"\b%s\s*\(" % n, src), n
        assert hasattr(lib, n), n
        assert n in vox_hip.EXPORTS, n
    host = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "vox_hip_host.h")).read(), flags=re.S)
    hl = ctypes.CDLL(os.path.join(ROOT, "voxtral.c_amd", "libvox_hip_host.so"))
    for n in ["vh_set_kv_grow", "vh_stream_kv_slots"]:
        assert re.search(r"\b%s\s*\(" % n, host), n
        assert hasattr(hl, n), n
    assert hasattr(vox_hip.Model, "set_kv_grow")
    for name in ["kv_slots", "kv_bytes", "reserve_kv", "kv_grow_stats"]:
        assert hasattr(vox_hip.Stream, name), name
    assert hasattr(vox_hip.Batch, "kv_grow_stats") and hasattr(vox_hip.HostCtx, "set_kv_grow")


def test_cli_parses_kv_grow():
    """--kv-grow N is an option with a value: named in the usage text, refused (usage, status 2)
    without its value or with a negative one, and accepted with one -- the run then gets as far as
    opening the checkpoint, which does not exist (status 1, no usage text)."""
    exe = os.path.join(ROOT, "voxtral.c_amd", "vox_hip_transcribe")

    def run(*args):
        p = subprocess.run([exe, *args], capture_output=True, text=True, timeout=60)
        return p.returncode, p.stderr

    rc, err = run()
    assert rc == 2 and "--kv-grow slots" in err
    rc, err = run("-d", "/nonexistent/model", "-i", "/nonexistent/a.wav", "--kv-grow")
    assert rc == 2 and "usage" in err
    rc, err = run("-d", "/nonexistent/model", "-i", "/nonexistent/a.wav", "--kv-grow", "-3")
    assert rc == 2 and "usage" in err
    rc, err = run("-d", "/nonexistent/model", "-i", "/nonexistent/a.wav", "--kv-grow", "256")
    assert rc == 1 and "usage" not in err, (rc, err)


def test_schedule_doubles_from_slots0_and_stops_at_full():
    full = R.full_slots(TINY_LONG)
    assert full == 8256 and R.full_slots(TINY) == 112
    # clamp: 0 stays off, below the slack -> the slack, above the full ring -> the full ring
    assert [R.clamp_slots0(v, TINY_LONG) for v in (0, 1, 63, 64, 65, 256, 8256, 9000)] == \
        [0, 64, 64, 64, 65, 256, 8256, 8256]
    assert [R.clamp_slots0(v, TINY) for v in (0, 32, 100, 112, 4096)] == [0, 64, 100, 112, 112]
    # the smallest slots0 * 2^k that holds the need, never above the full size
    assert [R.grow_cap(64, full, n) for n in (0, 64, 65, 128, 129, 300, 4097, 8192, 8193, 8256)] == \
        [64, 64, 128, 128, 256, 512, 8192, 8192, 8256, 8256]
    assert [R.grow_cap(256, full, n) for n in (1, 256, 257, 513)] == [256, 256, 512, 1024]
    assert R.grow_cap(96, full, 200) == 384 and R.grow_cap(96, full, 8000) == 8256   # 96 * 128 > full
    assert [R.grow_cap(64, 112, n) for n in (64, 65, 102, 112)] == [64, 112, 112, 112]   # TINY: 112, not 128
    # the sessions of the GPU tests in calls of 64 steps: the last position + 1 of each call
    needs = [R.PROMPT + min(424, 64 * (k + 1)) for k in range(7)]
    assert R.schedule(256, TINY_LONG, needs) == ([256, 256, 256, 512, 512, 512, 512], 1)
    assert R.schedule(64, TINY_LONG, needs) == ([128, 256, 256, 512, 512, 512, 512], 3)
    assert R.schedule(0, TINY_LONG, needs) == ([8256] * 7, 0)
    # a need beyond the full ring (the ring wraps) asks for the full ring, once
    assert R.schedule(64, TINY, [102, 166, 238]) == ([112, 112, 112], 1)
    assert R.ring_bytes(TINY_LONG, 8256, 4) == 2 * 2 * 8256 * 256 * 4


@pytest.mark.parametrize("dtype", [np.float32, np.float16, np.uint8])
def test_repitch_moves_the_prefix_and_nothing_else(dtype):
    """[L][cap0][C] -> [L][cap1][C]: rows [0, pos) of every layer at the same slots, every other
    element of the new buffer untouched -- for a full prefix, a partial one, an empty one and the
    capped last step (64 -> 112)"""
    rng = np.random.default_rng(3)
    L, C = 3, 8
    for cap0, cap1, pos in [(64, 128, 64), (64, 128, 39), (64, 128, 0), (64, 112, 51), (128, 128, 100)]:
        old = rng.integers(1, 100, size=(L, cap0, C)).astype(dtype)
        new = np.full((L, cap1, C), 101, dtype)
        out = R.repitch(old, new.copy(), pos)
        assert out.shape == (L, cap1, C)
        assert np.array_equal(out[:, :pos], old[:, :pos])
        assert np.all(out[:, pos:] == 101)
        # as flat device buffers: layer l starts at l * cap * C, the pitch is all that changed
        for l in range(L):
            a = out.reshape(-1)[l * cap1 * C:][:pos * C]
            b = old.reshape(-1)[l * cap0 * C:][:pos * C]
            assert np.array_equal(a, b)
    with pytest.raises(AssertionError):
        R.repitch(np.zeros((1, 64, 8), dtype), np.zeros((1, 32, 8), dtype), 10)   # never shrinks


@pytest.mark.parametrize("name", list(R.SESSIONS))
def test_oracle_sessions_keep_the_margin_rule(name):
    """ids are compared with the oracle's only where every step's top-2 gap is 4 x the logit bar"""
    cfg, steps, _ = R.SESSIONS[name]
    ref = R.session_oracle(name)
    assert len(ref["ids"]) == steps and ref["logits"].shape == (steps, cfg.vocab)
    m = R.worst_margin(ref["logits"])
    print(f"{name}: worst top-2 gap over {steps} steps {m:.2e}")
    assert m >= R.MARGIN, (name, m)
    # the sessions reach where the tests say they do
    last = R.PROMPT + steps
    if name == "long":
        assert 256 < last <= 512
    else:
        assert last > R.full_slots(TINY) + TINY.dec_window
