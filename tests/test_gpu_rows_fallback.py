"""The M > 1 transformer layers in both arithmetics, at TINY: k_gemmf over the fragment-major
copies (the default: TINY's shapes pass gemmf_ok) and the row-major launch_gemm (k_gemm2) layers
that VOX_HIP_GEMMF=0 (encoder and decoder) and VOX_HIP_PREFILL_GEMMF=0 (decoder only) select,
which no other test reaches with bf16 weights.

The switches are read once per process, so each mode runs in a fresh child, one after another,
each under its own timeout; the first that does not exit 0 stops the test.  Every child runs the
smallest case of every caller of the layers:
  A  a one-shot encode of 400 mel frames (200 encoder rows > enc_skinny_rows() = 80, so
     run_encoder_rows passes the skinny chain), then that stream's prefill and 4 steps
     (run_decoder_rows);
  B  one cross-stream encoder pass of 2 streams of 420 and 446 frames (run_encoder_rows_batch),
     then their stacked prefill through a Batch and 4 batched steps (batch_prefill);
  C  33 streams in one call of a Batch of capacity 64 (bucket 64: batch_step_wide, after two
     stacked prefill passes of 26 and 7 prompts) for 2 steps.
Per mode: every stream's ids equal its CPU-oracle session's; adapter rows (A, B) and the last
step's logits (every stream of A, B and C) within 5e-5 of the oracle's largest magnitude, the bar
of tests/test_gpu_tiny.py.  Across modes: the ids are identical.  As in tests/test_gpu_batch_kv8.py
the id comparison rests on the oracle's own top-2 gap, asserted first (4 x the logit bar, every
step used; mel seed 7300 is the first tried)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import test_gpu_batch_kv8 as g
from vox_weights import TINY

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

LOGIT_TOL = 5e-5     # of the largest logit magnitude, as tests/test_gpu_tiny.py
ADAPTER_TOL = 5e-5   # of the largest adapter magnitude, as tests/test_gpu_tiny.py
SEED = 7300
SIZES_A = [400]
SIZES_B = [420, 446]
SIZES_C = [400 + 2 * i for i in range(33)]
STEPS_AB, STEPS_C = 4, 2
KNOBS = ("VOX_HIP_GEMMF", "VOX_HIP_PREFILL_GEMMF")
MODES = (("default", {}), ("gemmf0", {"VOX_HIP_GEMMF": "0"}), ("prefill_gemmf0", {"VOX_HIP_PREFILL_GEMMF": "0"}))


def _mels():
    m = g._mels(TINY, SIZES_A + SIZES_B + SIZES_C, SEED)
    return m[:1], m[1:3], m[3:]


def _weights():
    from vox_weights import synth_weights
    return synth_weights(TINY, seed=1)


_REF = []


def _oracle():
    """[(adapter rows, ids, logits [steps, vocab])] for the streams of A, B and C, once"""
    import vox_oracle
    if not _REF:
        om = vox_oracle.OracleModel(TINY, _weights())
        out = []
        for mels, steps in zip(_mels(), (STEPS_AB, STEPS_AB, STEPS_C)):
            case = []
            for mel in mels:
                st = vox_oracle.OracleStream(om)
                st.encode_mel(mel)
                ad = st.read_adapter()
                ids, lg = st.decode(max_steps=steps, stop_at_eos=False, want_logits=True)
                st.close()
                for a in (ad, lg):
                    a.setflags(write=False)
                case.append((ad, ids.tolist(), lg))
            out.append(case)
        om.close()
        _REF.extend(out)
    return _REF


def _child_main(out_path):
    """in a fresh process, on the GPU only: cases A, B and C, to a file"""
    import vox_hip
    ma, mb, mc = _mels()
    hm = vox_hip.Model(TINY, _weights())
    z = {}
    # A: one-shot encode, single-stream prefill + steps
    s = vox_hip.Stream(hm)
    s.encode_mel(ma[0])
    z["a_adapter"] = s.read_adapter()
    ids, lg = s.decode(max_steps=STEPS_AB, stop_at_eos=False, want_logits=True)
    z["a_ids"], z["a_logits"] = ids[None, :], lg[-1:]
    s.close()
    # B: one encoder pass over both streams, stacked prefill + batched steps
    ss = [vox_hip.Stream(hm) for _ in mb]
    vox_hip.encode_mel_batch(ss, mb)
    for i, t in enumerate(ss):
        z[f"b_adapter{i}"] = t.read_adapter()
    b = vox_hip.Batch(hm, len(ss))
    z["b_ids"] = np.stack(b.decode(ss, max_steps=STEPS_AB, stop_at_eos=False))
    z["b_logits"] = np.stack([b.read_logits(t) for t in ss])
    assert b.stats()["prefill_passes"] == 1, b.stats()
    b.close()
    for t in ss:
        t.close()
    # C: 33 streams in a Batch of capacity 64
    ss = [vox_hip.Stream(hm) for _ in mc]
    for t, mel in zip(ss, mc):
        t.encode_mel(mel)
    b = vox_hip.Batch(hm, 64)
    z["c_ids"] = np.stack(b.decode(ss, max_steps=STEPS_C, stop_at_eos=False))
    z["c_logits"] = np.stack([b.read_logits(t) for t in ss])
    b.close()
    for t in ss:
        t.close()
    hm.close()
    np.savez(out_path, **z)


def _check(name, z, ref):
    worst_a, worst_l = 0.0, 0.0
    for case, key, n_ad in zip(ref, "abc", (1, 2, 0)):
        ids, lg = z[f"{key}_ids"], z[f"{key}_logits"]
        assert ids.shape[0] == lg.shape[0] == len(case), (name, key, ids.shape, lg.shape)
        for i, (ad, rids, rlg) in enumerate(case):
            assert ids[i].tolist() == rids, (name, key, i, ids[i].tolist(), rids)
            r = g.rel(lg[i], rlg[-1])
            print(f"{name} {key}{i}: last step's logit err {r:.2e}")
            worst_l = max(worst_l, r)
            assert r < LOGIT_TOL, (name, key, i, r)
            if i < n_ad:
                got = z["a_adapter"] if key == "a" else z[f"b_adapter{i}"]
                assert got.shape == ad.shape, (name, key, i, got.shape, ad.shape)
                ra = g.rel(got, ad)
                print(f"{name} {key}{i}: adapter err {ra:.2e}")
                worst_a = max(worst_a, ra)
                assert ra < ADAPTER_TOL, (name, key, i, ra)
    print(f"{name}: ids of {sum(len(c) for c in ref)} streams equal, worst adapter err {worst_a:.2e}, "
          f"worst logit err {worst_l:.2e}")


def test_rows_layers_in_both_arithmetics(tmp_path):
    ref = _oracle()
    for case, what, steps in zip(ref, ("A", "B", "C"), (STEPS_AB, STEPS_AB, STEPS_C)):
        assert all(len(ids) == steps for _, ids, _ in case), what
        g._assert_margin([(ids, lg) for _, ids, lg in case], 4 * LOGIT_TOL, f"rows fallback {what}")
    code = ("import sys; sys.path[:0] = [{!r}, {!r}, {!r}]; import test_gpu_rows_fallback as t; t._child_main(sys.argv[1])"
            .format(os.path.join(ROOT, "voxtral.c_amd"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")))
    runs = {}
    for name, knobs in MODES:
        env = {k: v for k, v in os.environ.items() if k not in KNOBS}
        env.update(knobs)
        out = str(tmp_path / f"{name}.npz")
        r = subprocess.run([sys.executable, "-c", code, out], env=env, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, (name, r.returncode, r.stdout[-2000:] + r.stderr[-4000:])   # stops the test
        runs[name] = dict(np.load(out))
        _check(name, runs[name], ref)
    for name, _ in MODES[1:]:
        for key in ("a_ids", "b_ids", "c_ids"):
            assert np.array_equal(runs["default"][key], runs[name][key]), (name, key)
        print(f"{name}: logits differ in bits from the default's: "
              f"{[not g._bits_equal(runs['default'][k], runs[name][k]) for k in ('a_logits', 'b_logits', 'c_logits')]}")
