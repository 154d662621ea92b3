#!/usr/bin/env python3
"""Batched decode steps at a full 8192-key window per decoder KV ring element type.

N streams of the full-size model (seeded synthetic weights, synthetic log-mel: nothing else is
read) are primed with batched steps until every one holds --keys positions, then --steps batched
steps are timed, for each element type in --dtypes (0 f32, 1 half, 2 FP8 E4M3) and each stream
count in --streams (the largest is primed, the smaller counts time a prefix of the same streams).
Weights are read once per step for all rows, every row reads its own rings: the KV bytes per step
are streams x keys x 212,992 / 106,496 / 53,248 B.  VOX_HIP_WMX4=2 VOX_HIP_WMX4_BATCH=1 in the
environment selects the MXFP4 fragment planes for the weights (read at model creation).

Prints one JSON line per (element type, stream count)."""
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
    ap.add_argument("--streams", type=int, nargs="+", default=[16, 8])
    ap.add_argument("--dtypes", type=int, nargs="+", default=[0, 1, 2])
    ap.add_argument("--keys", type=int, default=8192)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    import vox_hip
    from vox_weights import VOXTRAL_4B, synth_weights
    cfg = VOXTRAL_4B
    vox_hip.init(device=0)
    w = synth_weights(cfg, seed=args.seed)
    model = vox_hip.Model(cfg, w)
    del w
    nmax = max(args.streams)
    rows = args.keys + args.steps * len(args.streams) + 64
    rng = np.random.default_rng(77)
    mel = rng.uniform(-0.6, 1.4, size=(8 * rows, cfg.mel_bins)).astype(np.float32)
    mel_dev = vox_hip.DeviceArray(mel)
    kvb = {t: 2 * cfg.dec_layers * cfg.dec_kv_heads * cfg.dec_head_dim * e for t, e in ((0, 4), (1, 2), (2, 1))}
    for t in args.dtypes:
        model.set_kv_dtype(t)
        ss = [vox_hip.Stream(model) for _ in range(nmax)]
        model.set_kv_dtype(0)
        for s in ss:
            for off in range(0, mel.shape[0], 4096):
                s.encode_mel_device(mel_dev.ptr + off * cfg.mel_bins * 4, min(4096, mel.shape[0] - off))
        b = vox_hip.Batch(model, max(4, nmax))
        b.decode(ss, max_steps=1, stop_at_eos=False)                 # prefills + first token
        prime = max(0, args.keys - ss[0].state()["kv_pos"])
        done = 0
        while done < prime:
            n = min(4096, prime - done)
            b.decode(ss, max_steps=n, stop_at_eos=False)
            done += n
        for n in sorted(args.streams, reverse=True):
            sub = ss[:n]
            b.decode(sub, max_steps=4, stop_at_eos=False)            # this bucket's graphs
            for s in sub:
                s.sync()
            t0 = time.perf_counter()
            out = b.decode(sub, max_steps=args.steps, stop_at_eos=False)
            for s in sub:
                s.sync()
            dt = time.perf_counter() - t0
            assert all(len(o) == args.steps for o in out)
            keys = min(sub[0].state()["kv_pos"], cfg.dec_window)
            kv_step = n * keys * kvb[t]
            print(json.dumps({
                "kv_dtype": KV_NAMES[t], "streams": n, "keys": keys, "steps": args.steps,
                "ms_per_step": round(dt * 1e3 / args.steps, 4), "tokens_per_s": round(n * args.steps / dt, 1),
                "kv_bytes_per_step": kv_step, "kv_gbs": round(kv_step / (dt / args.steps) / 1e9, 1),
                "ring_gb_per_stream": round((cfg.dec_window + 64) * kvb[t] / 1e9, 3),
                "wmx4": vox_hip.wmx4(), "wmx4_batch": vox_hip.wmx4_batch()}), flush=True)
        b.close()
        for s in ss:
            s.close()
    mel_dev.free()
    model.close()


if __name__ == "__main__":
    main()
