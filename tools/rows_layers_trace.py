"""The launch sequence of every caller of the M > 1 layer walker (rows_layers), at
TINY, for a kernel trace of its own:

    rocprofv3 --kernel-trace -d DIR -o run --output-format csv -- python tools/rows_layers_trace.py
    python tools/rows_layers_trace.py --list DIR

The first form runs one encode, one prefill + 4 steps, one stacked prefill of 2 streams + 4
batched steps and 2 wide steps of 33 streams.  The second prints the sha256 of the ordered
(kernel name, grid) list of the trace under DIR, its length, and with --out FILE the list itself:
two trees launch the same kernels in the same order with the same grids when the hashes agree."""
import argparse
import csv
import glob
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "voxtral.c_amd"), os.path.join(ROOT, "oracle")]


def run():
    import numpy as np
    import vox_hip
    from vox_weights import TINY, synth_weights
    rng = np.random.default_rng(7300)
    mels = [rng.uniform(-0.6, 1.4, size=(n, TINY.mel_bins)).astype(np.float32)
            for n in [400, 420, 446] + [400 + 2 * i for i in range(33)]]
    hm = vox_hip.Model(TINY, synth_weights(TINY, seed=1))
    s = vox_hip.Stream(hm)
    s.encode_mel(mels[0])
    ids = [s.decode(max_steps=4, stop_at_eos=False).tolist()]
    s.close()
    for group, cap, steps in ((mels[1:3], 2, 4), (mels[3:], 64, 2)):
        ss = [vox_hip.Stream(hm) for _ in group]
        if cap == 2:
            vox_hip.encode_mel_batch(ss, group)
        else:
            for t, mel in zip(ss, group):
                t.encode_mel(mel)
        b = vox_hip.Batch(hm, cap)
        ids += [t.tolist() for t in b.decode(ss, max_steps=steps, stop_at_eos=False)]
        b.close()
        for t in ss:
            t.close()
    hm.close()
    print("ids sha256", hashlib.sha256(repr(ids).encode()).hexdigest())


def listing(d, out):
    rows = []
    for path in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
        with open(path, newline="") as f:
            rows += list(csv.DictReader(f))
    assert rows, f"no *kernel_trace.csv under {d}"
    rows.sort(key=lambda r: int(r["Dispatch_Id"]))
    lines = ["{} {}x{}x{}".format(r["Kernel_Name"], r["Grid_Size_X"], r["Grid_Size_Y"], r["Grid_Size_Z"]) for r in rows]
    text = "\n".join(lines) + "\n"
    if out:
        with open(out, "w") as f:
            f.write(text)
    print(f"{len(lines)} launches, sha256 {hashlib.sha256(text.encode()).hexdigest()}")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--list", metavar="DIR", default=None)
    ap.add_argument("--out", metavar="FILE", default=None)
    a = ap.parse_args()
    listing(a.list, a.out) if a.list else run()
