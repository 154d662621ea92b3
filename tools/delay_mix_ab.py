#!/usr/bin/env python3
"""What a mixed batched call costs per step: N pre-encoded streams of the full-size model (seeded
synthetic weights, synthetic log-mel: nothing else is read) all following the model's delay (a
plain call: the shared-row norm kernels) against the same streams with delays of their own
alternating over five values (vox_hip_stream_set_delay: the per-slot instances
k_resid_xw_fplanes_slot / k_rmsnorm_fplanes_slot).

For each N in --streams and each variant, in one process and --rounds alternating rounds: the
streams are reset, given their delays and encoded again, one untimed Batch.decode(max_steps=1)
runs the prefills and the first step (and, the first time, the graph capture), then one
Batch.decode(max_steps=--steps) is timed: ms per batched step = its time / --steps.  One untimed
round comes first.  The contexts of the two variants differ by the prompt lengths (39 keys for the
model's delay of 6 against 34..63), all below one 256-key attention block.

Prints one JSON line per (N, round, variant) and a summary line per N."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "voxtral.c_amd"))

DELAYS = (1, 3, 6, 12, 30)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--streams", type=int, nargs="+", default=[16, 32, 64])
    ap.add_argument("--steps", type=int, default=32)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    import vox_hip
    from vox_weights import VOXTRAL_4B, synth_weights
    cfg = VOXTRAL_4B
    vox_hip.init(device=0)
    w = synth_weights(cfg, seed=args.seed)
    model = vox_hip.Model(cfg, w)
    del w
    rows = 1 + 32 + max(DELAYS) + 1 + args.steps + 2
    rng = np.random.default_rng(78)
    mel = rng.uniform(-0.6, 1.4, size=(8 * rows, cfg.mel_bins)).astype(np.float32)
    mel_dev = vox_hip.DeviceArray(mel)
    for n in args.streams:
        ss = [vox_hip.Stream(model) for _ in range(n)]
        b = vox_hip.Batch(model, n)
        ms = {"plain": [], "mixed": []}

        def call(variant, timed, rnd):
            for i, s in enumerate(ss):
                s.reset()
                s.set_delay(DELAYS[i % len(DELAYS)] if variant == "mixed" else None)
                s.encode_mel_device(mel_dev.ptr, mel.shape[0])
            for s in ss:
                s.sync()
            assert all(len(o) == 1 for o in b.decode(ss, max_steps=1, stop_at_eos=False))
            r0 = b.stats()["replays"]
            t0 = time.perf_counter()
            out = b.decode(ss, max_steps=args.steps, stop_at_eos=False)
            dt = (time.perf_counter() - t0) * 1e3
            assert all(len(o) == args.steps for o in out)
            assert b.stats()["replays"] - r0 == args.steps
            if timed:
                ms[variant].append(dt / args.steps)
                print(json.dumps({"streams": n, "round": rnd, "variant": variant,
                                  "ms_per_step": round(dt / args.steps, 4)}), flush=True)

        for variant in ("plain", "mixed"):
            call(variant, False, -1)
        for rnd in range(args.rounds):
            for variant in ("plain", "mixed"):
                call(variant, True, rnd)
        p, m = ms["plain"], ms["mixed"]
        print(json.dumps({"streams": n, "summary": True, "steps": args.steps,
                          "plain_ms_per_step": [round(v, 4) for v in p], "mixed_ms_per_step": [round(v, 4) for v in m],
                          "plain_spread_ms": round(max(p) - min(p), 4),
                          "mixed_minus_plain_median_ms": round(float(np.median(m) - np.median(p)), 4)}), flush=True)
        b.close()
        for s in ss:
            s.close()
    mel_dev.free()
    model.close()


if __name__ == "__main__":
    main()
