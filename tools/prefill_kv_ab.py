#!/usr/bin/env python3
"""The batched prefill of joining streams per decoder KV ring element type: stacked passes on the
batch queue against one single-stream prefill per stream (vox_hip_batch_set_prefill_kv 1 / 0).

N fresh pre-encoded streams of the full-size model (seeded synthetic weights, synthetic log-mel:
nothing else is read) join a batch in one Batch.decode(max_steps=1): their prefills plus one
batched step.  That call is timed with the switch at 0 and at 1 in --pairs alternating pairs in
one process, for each element type in --dtypes (0 f32, which ignores the switch, 1 half, 2 FP8
E4M3); before every timed call the streams are reset and encoded again.  One untimed pair comes
first (fragment-major weight copies, plane buffers, step graphs).

Prints one JSON line per (element type, pair, variant) and a summary line per element type:
ms per call, prefill passes, and the decoder layer weight bytes the prefills of the call stream
(passes x the 26 layers' matrices; the step adds one more read for either variant)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "voxtral.c_amd"))

KV_NAMES = {0: "f32", 1: "half", 2: "fp8"}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--streams", type=int, default=16)
    ap.add_argument("--dtypes", type=int, nargs="+", default=[1, 2, 0])
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    import vox_hip
    from vox_weights import VOXTRAL_4B, synth_weights
    cfg = VOXTRAL_4B
    vox_hip.init(device=0)
    w = synth_weights(cfg, seed=args.seed)
    model = vox_hip.Model(cfg, w)
    del w
    n = args.streams
    rows = 39 + 9                      # the prompt and a few rows more
    rng = np.random.default_rng(77)
    mel = rng.uniform(-0.6, 1.4, size=(8 * rows, cfg.mel_bins)).astype(np.float32)
    mel_dev = vox_hip.DeviceArray(mel)
    dq, dkv = cfg.dec_heads * cfg.dec_head_dim, cfg.dec_kv_heads * cfg.dec_head_dim
    layer_w = 2 * (cfg.dec_dim * (dq + 2 * dkv) + dq * cfg.dec_dim + 3 * cfg.dec_dim * cfg.dec_hidden)
    pass_bytes = cfg.dec_layers * layer_w
    for t in args.dtypes:
        model.set_kv_dtype(t)
        ss = [vox_hip.Stream(model) for _ in range(n)]
        model.set_kv_dtype(0)
        b = vox_hip.Batch(model, max(4, n))
        ms = {0: [], 1: []}

        def call(on, timed, pair):
            for s in ss:
                s.reset()
                s.encode_mel_device(mel_dev.ptr, mel.shape[0])
            for s in ss:
                s.sync()
            assert b.set_prefill_kv(on) == 0
            p0 = b.stats()["prefill_passes"]
            t0 = time.perf_counter()
            out = b.decode(ss, max_steps=1, stop_at_eos=False)
            dt = (time.perf_counter() - t0) * 1e3
            assert all(len(o) == 1 for o in out)
            passes = b.stats()["prefill_passes"] - p0
            if timed:
                ms[on].append(dt)
                print(json.dumps({"kv_dtype": KV_NAMES[t], "streams": n, "pair": pair, "prefill_kv": on,
                                  "ms_per_call": round(dt, 3), "prefill_passes": passes,
                                  "prefill_weight_bytes": passes * pass_bytes}), flush=True)
            return passes

        for on in (0, 1):
            call(on, False, -1)
        for pair in range(args.pairs):
            for on in (0, 1):
                call(on, True, pair)
        # f32 streams take the stacked pass under either value: their two columns are one variant
        verdict = ({"switch_ignored": True} if t == 0 else
                   {"stacked_slower_in_every_pair": all(a < c for a, c in zip(ms[0], ms[1]))})
        print(json.dumps({"kv_dtype": KV_NAMES[t], "streams": n, "summary": True,
                          "ms_per_call_off": [round(v, 3) for v in ms[0]], "ms_per_call_on": [round(v, 3) for v in ms[1]],
                          "median_off": round(float(np.median(ms[0])), 3), "median_on": round(float(np.median(ms[1])), 3),
                          **verdict}), flush=True)
        b.close()
        for s in ss:
            s.close()
    mel_dev.free()
    model.close()


if __name__ == "__main__":
    main()
