#!/usr/bin/env python3
"""k_gemmf over int8 fragments against the row-major GEMM on a Q8 model (vox_hip_set_gemmf_q8 1 / 0),
both in one process: two models over one quantised weight set (seeded synthetic weights of the
full-size architecture, synthetic log-mel: nothing else is read), one created with the switch off
and one with it on, timed in --rounds alternating rounds, every timed pass after an untimed one.

Per round and variant, with bench.py's own phase timers (transcribe / transcribe_batch):
  single   one jfk-shaped one-shot transcription: encoder (677-row pass), prefill + first token,
           the greedy steps (the single-stream GEMV step: the switch does not reach it);
  streams  for each S of --streams (S > 64 with IEEE-half rings, as bench.py --kv-fp16): S
           jfk-shaped transcriptions, encoders and prefills per stream, the steps batched
           (S <= 32: the skinny step, which the switch does not reach; 33..128: the wide step).
Prints one JSON line per (case, round, variant) and a summary line per case with the medians."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "voxtral.c_amd"))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--streams", type=int, nargs="*", default=[64, 128, 32])
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    import bench
    import vox_hip
    from vox_weights import VOXTRAL_4B, quantize_q8, synth_weights
    cfg = VOXTRAL_4B
    vox_hip.init(device=0)
    w = quantize_q8(synth_weights(cfg, seed=args.seed))
    models = {}
    for on in (0, 1):
        vox_hip.set_gemmf_q8(bool(on))
        models[on] = vox_hip.Model(cfg, w)
    vox_hip.set_gemmf_q8(False)
    del w
    rng = np.random.default_rng(args.seed)
    n_mel = sum(bench.JFK_CHUNKS)

    def new_mel():
        return vox_hip.DeviceArray(rng.uniform(-0.6, 1.4, size=(n_mel, cfg.mel_bins)).astype(np.float32))

    def report(case, rows):
        keys = [k for k in rows[0][0] if k not in ("round", "gemmf_q8", "case")]
        med = {f"{k}_{('off', 'on')[on]}": round(float(np.median([r[k] for r in rows[on]])), 4) for k in keys for on in (0, 1)}
        print(json.dumps({"case": case, "summary": True, "rounds": args.rounds, **med,
                          "int8_launches_off": models[0].gemmf_q8_stats()[1],
                          "int8_launches_on": models[1].gemmf_q8_stats()[1]}), flush=True)

    # ---- one stream --------------------------------------------------------------------------------
    mel0 = new_mel()
    sts = {on: vox_hip.Stream(models[on]) for on in (0, 1)}
    rows = {0: [], 1: []}
    ids = {}
    for rnd in range(-1, args.rounds):
        for on in (0, 1):
            r = bench.transcribe(sts[on], mel0, cfg.mel_bins)
            ids[on] = r["tokens"]
            if rnd < 0:
                continue
            row = {"case": "single", "round": rnd, "gemmf_q8": on, "enc_ms": round(r["enc"] * 1e3, 3),
                   "encoder_rtf": round(r["enc"] / bench.AUDIO_SECONDS, 6), "prefill_ms": round(r["prefill"] * 1e3, 3),
                   "ms_per_step": round(r["step_s"] * 1e3 / max(1, r["steps"]), 4)}
            rows[on].append(row)
            print(json.dumps(row), flush=True)
    print(json.dumps({"case": "single", "ids_equal_off_on": bool(np.array_equal(ids[0], ids[1])), "tokens": int(len(ids[0]))}),
          flush=True)
    report("single", rows)
    for s in sts.values():
        s.close()

    # ---- S streams -----------------------------------------------------------------------------------
    # (the streams and batch of one variant at a time: two sets of 64 f32 or 128 half ring sets
    # would not fit beside each other; each timed pass follows an untimed one on the same batch)
    for S in args.streams:
        half = S > 64
        mels = [mel0] + [new_mel() for _ in range(S - 1)]
        rows = {0: [], 1: []}
        case = f"streams{S}" + ("_kv16" if half else "")
        same = True
        for rnd in range(args.rounds):
            toks = {}
            for on in (0, 1):
                models[on].set_kv_fp16(half)
                ss = [vox_hip.Stream(models[on]) for _ in range(S)]
                models[on].set_kv_fp16(False)
                b = vox_hip.Batch(models[on], S)
                bench.transcribe_batch(b, ss, mels, cfg.mel_bins)
                r = bench.transcribe_batch(b, ss, mels, cfg.mel_bins)
                toks[on] = r["tokens"]
                row = {"case": case, "round": rnd, "gemmf_q8": on, "enc_ms_per_stream": round(r["enc"] * 1e3 / S, 3),
                       "prefill_ms_per_stream": round(r["prefill"] * 1e3 / S, 3),
                       "ms_per_batched_step": round(r["step_s"] * 1e3 / max(1, r["steps"] / S), 4),
                       "tokens_per_s": round(r["steps"] / r["step_s"], 1)}
                rows[on].append(row)
                print(json.dumps(row), flush=True)
                b.close()
                for s_ in ss:
                    s_.close()
            same = same and all(np.array_equal(x, y) for x, y in zip(toks[0], toks[1]))
        print(json.dumps({"case": case, "ids_equal_off_on": bool(same)}), flush=True)
        report(case, rows)
        for m in mels[1:]:
            m.free()
    mel0.free()
    for m in models.values():
        m.close()


if __name__ == "__main__":
    main()
