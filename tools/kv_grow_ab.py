#!/usr/bin/env python3
"""bench.py of this tree with full decoder K/V rings ("off") and with growing ones ("on",
VOX_HIP_KV_GROW=<--slots0>, default 64) against bench.py of a built copy of the parent commit
(--parent DIR), in --rounds alternating rounds of (parent, off, on) in one call on one GPU, for
each configuration in --configs:

    default     bench.py                  (single stream: decoder tokens/s, encoder RTF)
    streams16   bench.py --streams 16     (the <= 32 MFMA step; "on": its ragged instances)
    streams64   bench.py --streams 64     (the wide step; "on": its ragged instances)

Every run is a fresh child process under its own time limit; the first one that fails ends the
tool.  Prints one JSON line per run and a summary line per configuration: the figures per variant,
the parent's own spread (max - min over its rounds), whether "off" falls inside the parent's
measured range, and "on" against "off" as a ratio of the medians (for the batched configurations,
whose streams stay far below the full ring, that is the ragged step against the plain step).
"on" is reported, not gated.

--growth instead times one growth of a stream's rings at Voxtral's ring geometry (26 layers x
1024 K/V columns, f32) from 4096 to 8256 slots with 4064 rows to copy, in this tree only: the
host time of vox_hip_stream_reserve_kv (two allocations that are zeroed, two 2D copies, the wait,
two frees) over --rounds fresh streams."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONFIGS = {"default": [], "streams16": ["--streams", "16"], "streams64": ["--streams", "64"]}
KEYS = ("value", "encoder_rtf")


def run(tree, extra, slots0, steps, warmup, limit):
    env = dict(os.environ)
    env.pop("VOX_HIP_KV_GROW", None)
    if slots0:
        env["VOX_HIP_KV_GROW"] = str(slots0)
    cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.join(tree, "bench.py"), "--gpus", "1",
           "--steps", str(steps), "--warmup", str(warmup)] + extra
    p = subprocess.run(cmd, cwd=tree, env=env, capture_output=True, text=True)
    if p.returncode != 0:
        sys.stderr.write(p.stdout[-2000:] + p.stderr[-2000:])
        raise SystemExit(f"{' '.join(cmd)}: exit {p.returncode}")
    line = [l for l in p.stdout.splitlines() if l.startswith("{")][-1]
    return json.loads(line)


def growth(rounds):
    """one 4096 -> 8256 growth per fresh stream at the full ring geometry, small everywhere else"""
    sys.path.insert(0, os.path.join(ROOT, "voxtral.c_amd"))
    import dataclasses

    import numpy as np

    import vox_hip
    from vox_weights import TINY, synth_weights
    cfg = dataclasses.replace(TINY, dec_layers=26, dec_heads=32, dec_kv_heads=8, dec_window=8192, enc_window=750)
    m = vox_hip.Model(cfg, synth_weights(cfg, seed=1))
    rows = 64
    x = np.zeros((rows, cfg.dec_dim), np.float32)
    rope = np.zeros((rows, cfg.dec_head_dim), np.float32)
    rope[:, 0::2] = 1.0
    ms = []
    for _ in range(rounds):
        m.set_kv_grow(4096)
        s = vox_hip.Stream(m)
        m.set_kv_grow(0)
        # the ring is sized for positions [0, 4064): those rows are what the growth copies
        s.twin_decoder_prefill_step(x, rope, 4000)
        assert s.kv_slots == 4096
        t0 = time.perf_counter()
        s.reserve_kv(8256)
        ms.append((time.perf_counter() - t0) * 1e3)
        st = s.kv_grow_stats()
        assert st["slots"] == 8256 and st["grows"] == 1
        s.close()
    m.close()
    print(json.dumps({"growth": "4096 -> 8256 slots, 26 layers x 1024 columns f32", "copied_bytes": st["copied"],
                      "new_ring_bytes": 2 * 26 * 8256 * 1024 * 4, "ms": [round(v, 3) for v in ms],
                      "ms_median": round(statistics.median(ms), 3)}), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--parent", help="a built checkout of the parent commit")
    ap.add_argument("--configs", nargs="+", default=list(CONFIGS), choices=list(CONFIGS))
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--slots0", type=int, default=64, help="VOX_HIP_KV_GROW of the \"on\" runs")
    ap.add_argument("--limit", type=int, default=600, help="seconds per bench.py run")
    ap.add_argument("--growth", action="store_true", help="time one 4096 -> 8256 growth instead")
    args = ap.parse_args()
    if args.growth:
        growth(args.rounds)
        return
    if not args.parent:
        ap.error("--parent is required without --growth")
    for name in args.configs:
        res = {"parent": [], "off": [], "on": []}
        for rnd in range(args.rounds):
            for variant in ("parent", "off", "on"):
                tree = os.path.abspath(args.parent) if variant == "parent" else ROOT
                out = run(tree, CONFIGS[name], args.slots0 if variant == "on" else 0, args.steps, args.warmup, args.limit)
                rec = {k: out.get(k) for k in KEYS}
                res[variant].append(rec)
                print(json.dumps({"config": name, "round": rnd, "variant": variant, **rec}), flush=True)
        summary = {"config": name, "summary": True}
        for k in KEYS:
            vals = {v: [r[k] for r in res[v] if r[k] is not None] for v in res}
            if not vals["parent"]:
                continue
            lo, hi = min(vals["parent"]), max(vals["parent"])
            summary[k] = {v: vals[v] for v in vals}
            summary[k + "_parent_spread"] = round(hi - lo, 6)
            summary[k + "_off_within_parent_range"] = all(lo <= x <= hi for x in vals["off"])
            if vals["on"] and vals["off"]:
                summary[k + "_on_over_off"] = round(statistics.median(vals["on"]) / statistics.median(vals["off"]), 4)
        print(json.dumps(summary), flush=True)


if __name__ == "__main__":
    main()
