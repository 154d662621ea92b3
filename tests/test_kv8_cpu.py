"""CPU tests of the FP8 E4M3 decoder KV ring's format (csrc/vox_kv8.h) and of the Python decoder
session the GPU tests replay (tests/kv8_ref.py)."""
import os

import numpy as np
import pytest

import kv8_ref
from kv8_ref import (CFGS, MARGIN, RUNS, RefDecoder, c_kv8_decode, c_kv8_encode, kv8_midpoints, np_kv8_decode,
                     np_kv8_encode, np_kv8_values, oracle_adapter, run_mels, top2_margin)

STEPS = 60


@pytest.fixture(scope="module")
def tiny(tiny_cfg, tiny_weights):
    import vox_oracle
    vox_oracle.set_threads(min(16, os.cpu_count() or 1))
    om = vox_oracle.OracleModel(tiny_cfg, tiny_weights)
    mel = np.random.default_rng(7).uniform(-0.6, 1.4, size=(8 * (39 + STEPS + 5), 128)).astype(np.float32)
    yield tiny_cfg, tiny_weights, om, mel
    vox_oracle.set_kv_fp16(False)
    om.close()


def _oracle_session(om, mel, kv16):
    import vox_oracle
    vox_oracle.set_kv_fp16(kv16)
    try:
        st = vox_oracle.OracleStream(om)
        st.encode_mel(mel)
        ids, lg = st.decode(max_steps=STEPS, stop_at_eos=False, want_logits=True)
        st.close()
    finally:
        vox_oracle.set_kv_fp16(False)
    return ids, lg


def test_ref_identity_equals_oracle(tiny):
    """identity hook: ids and logits over prefill + 60 steps (the 48-key window slides) are the
    oracle's, bit for bit"""
    cfg, w, om, mel = tiny
    ids, lg = _oracle_session(om, mel, False)
    assert len(ids) == STEPS
    r = RefDecoder(cfg, w, oracle_adapter(om, mel), om.ada_scale())
    rids, rlg = r.decode(STEPS)
    assert np.array_equal(rids, ids)
    assert np.array_equal(rlg, lg)


def test_ref_f16_hook_equals_oracle_kv_fp16(tiny):
    """vox_oracle.f16_round as the hook = the oracle under set_kv_fp16(True): the hook sits at the
    oracle's own rounding site"""
    cfg, w, om, mel = tiny
    ids, lg = _oracle_session(om, mel, True)
    _, lg32 = _oracle_session(om, mel, False)
    assert not np.array_equal(lg, lg32)     # the rounding changes the session
    r = RefDecoder(cfg, w, oracle_adapter(om, mel), om.ada_scale(), round_fn=kv8_ref.f16_hook)
    rids, rlg = r.decode(STEPS)
    assert np.array_equal(rids, ids)
    assert np.array_equal(rlg, lg)


def _bits(x):
    return np.asarray(x, np.float32).view(np.uint32)


def _check(x):
    """C rule == numpy rule over x: codes, and decoded values bit for bit"""
    x = np.asarray(x, np.float32)
    cc, cb = c_kv8_encode(x)
    nc = np_kv8_encode(x)
    bad = np.nonzero(cc != nc)[0]
    assert bad.size == 0, (x[bad[:4]], cc[bad[:4]], nc[bad[:4]])
    assert np.array_equal(_bits(cb), _bits(np_kv8_decode(nc)))
    return cc


def test_kv8_all_codes_round_trip():
    codes = np.arange(256, dtype=np.uint8)
    vals = c_kv8_decode(codes)
    assert np.array_equal(_bits(vals), _bits(np_kv8_decode(codes)))
    exp = np_kv8_values()
    fin = ~np.isnan(exp)
    assert np.array_equal(vals[fin].astype(np.float64), exp[fin]) and np.all(np.isnan(vals[~fin]))
    assert np.array_equal(np.nonzero(~fin)[0], [0x7f, 0xff])
    assert vals[0x7e] == 448.0 and vals[0x08] == 2.0 ** -6 and vals[0x01] == 2.0 ** -9
    assert np.signbit(vals[0x80]) and vals[0x80] == 0.0
    # every code encodes back to itself (NaN: 0x7f with the sign)
    assert np.array_equal(_check(vals), codes)
    # torch's e4m3fn agrees inside +-448 (beyond, it gives NaN where this rule saturates)
    torch = pytest.importorskip("torch")
    if hasattr(torch, "float8_e4m3fn"):
        x = np.random.default_rng(3).uniform(-448, 448, 20000).astype(np.float32)
        x = np.concatenate([x, x * 2.0 ** -10, kv8_midpoints(), -kv8_midpoints()])
        t = torch.from_numpy(x).to(torch.float8_e4m3fn)
        assert np.array_equal(t.view(torch.uint8).numpy(), c_kv8_encode(x)[0])
        assert np.array_equal(t.to(torch.float32).numpy(), c_kv8_encode(x)[1])


def test_kv8_midpoints_ties_to_even():
    mid = kv8_midpoints()                    # midpoint i lies between codes i and i + 1
    assert mid.size == 126
    lo = np.arange(126)
    even = np.where(lo % 2 == 0, lo, lo + 1).astype(np.uint8)
    for sgn, sb in ((1.0, 0), (-1.0, 0x80)):
        m = (sgn * mid).astype(np.float32)
        assert np.array_equal(_check(m), even | sb)
        toward0 = np.nextafter(m, np.float32(0), dtype=np.float32)
        away = np.nextafter(m, np.float32(sgn * np.inf), dtype=np.float32)
        assert np.array_equal(_check(toward0), lo.astype(np.uint8) | sb)
        assert np.array_equal(_check(away), (lo + 1).astype(np.uint8) | sb)


def test_kv8_saturation_zero_nan_subnormals():
    big = np.array([448, 463.99997, 464, 464.00003, 480, 1e9, 3.4e38, np.inf], np.float32)
    assert np.all(_check(big) == 0x7e) and np.all(_check(-big) == 0xfe)
    assert np.all(c_kv8_encode(big)[1] == 448.0)
    below = np.nextafter(np.float32(448), np.float32(0))
    assert _check([below])[0] == 0x7e and _check([np.float32(432)])[0] == 0x7e   # 432: tie 416 | 448 -> even mantissa
    assert _check([np.nextafter(np.float32(432), np.float32(0))])[0] == 0x7d
    z = _check(np.array([0.0, -0.0], np.float32))
    assert z.tolist() == [0x00, 0x80]
    nan = np.array([np.nan, -np.nan], np.float32)
    nan = np.concatenate([nan, np.array([0x7f800001, 0xffc12345], np.uint32).view(np.float32)])
    assert c_kv8_encode(nan)[0].tolist() == [0x7f, 0xff, 0x7f, 0xff]
    assert np.array_equal(np_kv8_encode(nan), c_kv8_encode(nan)[0])
    # subnormal range: multiples of 2^-9 below 2^-6, f32 denormals and tiny values to (signed) zero
    x = np.linspace(0, 2.0 ** -6, 4097).astype(np.float32)
    c = _check(x)
    assert c.max() == 8 and c.min() == 0 and set(np.unique(c)) == set(range(9))
    assert np.array_equal(c_kv8_encode(x)[1], (np.round(x.astype(np.float64) * 512) / 512).astype(np.float32))
    tiny = np.array([1e-45, 1e-38, 2.0 ** -10, np.nextafter(np.float32(2.0 ** -10), np.float32(1))], np.float32)
    assert _check(tiny).tolist() == [0, 0, 0, 1] and _check(-tiny).tolist() == [0x80, 0x80, 0x80, 0x81]


def test_kv8_random_and_idempotent():
    rng = np.random.default_rng(5)
    x = (rng.choice([-1.0, 1.0], 200000) * 2.0 ** rng.uniform(-12, 12, 200000)).astype(np.float32)
    _check(x)
    _, r = c_kv8_encode(x)
    _, rr = c_kv8_encode(r)
    assert np.array_equal(_bits(r), _bits(rr))
    lib = kv8_ref._synth()
    for v in (0.3, -17.25, 500.0, 2.0 ** -8):
        assert lib.vox_kv8_decode(lib.vox_kv8_encode(v)) == lib.vox_kv8_round(v) == float(np_kv8_decode(np_kv8_encode([v]))[0])


@pytest.mark.parametrize("name", sorted(RUNS))
def test_kv8_unforced_reference_margin(name, tiny_weights):
    """the FP8 reference on its own (kv8_round at the append, nothing forced): at the seeds the GPU
    tests use, the top-2 gap is at least MARGIN of the largest logit on every step of every stream"""
    import vox_oracle
    from vox_weights import synth_weights
    vox_oracle.set_threads(min(16, os.cpu_count() or 1))
    cfg = CFGS[RUNS[name][0]]
    w = tiny_weights if cfg.dec_dim == 256 else synth_weights(cfg, seed=1)
    om = vox_oracle.OracleModel(cfg, w)
    worst = np.inf
    for mel, n in zip(run_mels(name), RUNS[name][2]):
        r = RefDecoder(cfg, w, oracle_adapter(om, mel), om.ada_scale(), round_fn=kv8_ref.kv8_hook)
        ids, lg = r.decode(n)
        assert len(ids) == n
        worst = min(worst, top2_margin(lg))
    om.close()
    print(f"{name}: unforced FP8 reference top-2 margin {worst:.2e} (needs {MARGIN:.1e})")
    assert worst >= MARGIN, worst
