#!/usr/bin/env python3
"""bench.py of this tree with the encoder K/V rings as f32 ("off"), as IEEE half ("half",
VOX_HIP_ENC_KV_FP16=1) and as FP8 E4M3 ("fp8", VOX_HIP_ENC_KV_FP8=1) against bench.py of a built
copy of the parent commit (--parent DIR), in --rounds alternating rounds of (parent, off, half,
fp8) in one call on one GPU, for each configuration in --configs:

    default     bench.py                         (encoder RTF, jfk)
    streaming   bench.py --streaming              (the short-chunk encoder: 25-row chunks)
    stagger32   bench.py --stagger --streams 32

Every run is a fresh child process under its own time limit; the first one that fails ends the
tool.  Prints one JSON line per run and a summary line per configuration.  The only gate is the
precedent of DESIGN.md 31.6: with the switch off, no run is slower than the parent's slowest run
of the same rounds (tokens/s not below the parent's lowest, encoder RTF not above its highest).
"half" and "fp8" are reported, not gated."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONFIGS = {"default": [], "streaming": ["--streaming"], "stagger32": ["--stagger", "--streams", "32"]}
VARIANTS = {"parent": {}, "off": {}, "half": {"VOX_HIP_ENC_KV_FP16": "1"}, "fp8": {"VOX_HIP_ENC_KV_FP8": "1"}}
KEYS = ("value", "encoder_rtf")      # decoder tokens/s (higher is better), encoder time / audio time (lower)


def run(tree, extra, setenv, steps, warmup, limit):
    env = dict(os.environ)
    for k in ("VOX_HIP_ENC_KV_FP16", "VOX_HIP_ENC_KV_FP8"):
        env.pop(k, None)
    env.update(setenv)
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
    ap.add_argument("--configs", nargs="+", default=["default", "streaming"], choices=list(CONFIGS))
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--limit", type=int, default=600, help="seconds per bench.py run")
    args = ap.parse_args()
    ok = True
    for name in args.configs:
        res = {v: [] for v in VARIANTS}
        for rnd in range(args.rounds):
            for variant, setenv in VARIANTS.items():
                tree = os.path.abspath(args.parent) if variant == "parent" else ROOT
                out = run(tree, CONFIGS[name], setenv, args.steps, args.warmup, args.limit)
                rec = {k: out.get(k) for k in KEYS}
                res[variant].append(rec)
                print(json.dumps({"config": name, "round": rnd, "variant": variant, **rec}), flush=True)
        summary = {"config": name, "summary": True}
        for k in KEYS:
            vals = {v: [r[k] for r in res[v] if r[k] is not None] for v in res}
            if not vals["parent"] or not vals["off"]:
                continue
            summary[k] = vals
            if k == "value":
                gate = min(vals["off"]) >= min(vals["parent"])
            else:
                gate = max(vals["off"]) <= max(vals["parent"])
            summary[k + "_off_not_slower_than_parents_slowest"] = gate
            ok = ok and gate
        print(json.dumps(summary), flush=True)
    return 0 if ok else 3


if __name__ == "__main__":
    sys.exit(main())
