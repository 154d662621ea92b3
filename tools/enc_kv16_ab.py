#!/usr/bin/env python3
"""bench.py of this tree with the encoder K/V rings as f32 ("off") and as IEEE half ("on",
VOX_HIP_ENC_KV_FP16=1) against bench.py of a built copy of the parent commit (--parent DIR), in
--rounds alternating rounds of (parent, off, on) in one call on one GPU, for each configuration in
--configs:

    default     bench.py                         (encoder RTF, jfk)
    streaming   bench.py --streaming
    stagger32   bench.py --stagger --streams 32

Every run is a fresh child process under its own time limit; the first one that fails ends the
tool.  Prints one JSON line per run and a summary line per configuration: the figures per variant,
the parent's own spread (max - min over its rounds) and whether "off" falls inside the parent's
range widened by one such spread.  "on" is reported, not gated."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONFIGS = {"default": [], "streaming": ["--streaming"], "stagger32": ["--stagger", "--streams", "32"]}
KEYS = ("value", "encoder_rtf")


def run(tree, extra, on, steps, warmup, limit):
    env = dict(os.environ)
    env.pop("VOX_HIP_ENC_KV_FP16", None)
    if on:
        env["VOX_HIP_ENC_KV_FP16"] = "1"
    cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.join(tree, "bench.py"), "--gpus", "1",
           "--steps", str(steps), "--warmup", str(warmup)] + extra
    p = subprocess.run(cmd, cwd=tree, env=env, capture_output=True, text=True)
    if p.returncode != 0:
        sys.stderr.write(p.stdout[-2000:] + p.stderr[-2000:])
        raise SystemExit(f"{' '.join(cmd)}: exit {p.returncode}")
    line = [l for l in p.stdout.splitlines() if l.startswith("{")][-1]
    return json.loads(line)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--parent", required=True, help="a built checkout of the parent commit")
    ap.add_argument("--configs", nargs="+", default=list(CONFIGS), choices=list(CONFIGS))
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--limit", type=int, default=600, help="seconds per bench.py run")
    args = ap.parse_args()
    for name in args.configs:
        res = {"parent": [], "off": [], "on": []}
        for rnd in range(args.rounds):
            for variant in ("parent", "off", "on"):
                tree = os.path.abspath(args.parent) if variant == "parent" else ROOT
                out = run(tree, CONFIGS[name], variant == "on", args.steps, args.warmup, args.limit)
                rec = {k: out.get(k) for k in KEYS}
                res[variant].append(rec)
                print(json.dumps({"config": name, "round": rnd, "variant": variant, **rec}), flush=True)
        summary = {"config": name, "summary": True}
        for k in KEYS:
            vals = {v: [r[k] for r in res[v] if r[k] is not None] for v in res}
            if not vals["parent"]:
                continue
            lo, hi = min(vals["parent"]), max(vals["parent"])
            spread = hi - lo
            summary[k] = {v: vals[v] for v in vals}
            summary[k + "_parent_spread"] = round(spread, 6)
            summary[k + "_off_within_parent_range_plus_one_spread"] = all(lo - spread <= x <= hi + spread for x in vals["off"])
        print(json.dumps(summary), flush=True)


if __name__ == "__main__":
    main()
