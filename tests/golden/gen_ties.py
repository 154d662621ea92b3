"""Weights whose LM head produces exact logit ties (tests/test_argmax_ties_cpu.py,
tests/test_gpu_argmax_ties.py).  Importable only: nothing is written to disk.

The reference picks the token and the --alt candidates by scanning ids in ascending order with a
strict '>' (voxtral_decoder.c:771-779, stream_fill_alts voxtral.c:955-1010): among equal logits
the lowest id wins and equal-probability alternatives come out in ascending id order.  Seeded
Gaussian rows never tie, so `tie_weights` copies a few synthetic rows of tok_embeddings.weight
over sets of ids ("positions") chosen to sit on every boundary of the device's reductions:

  p even: {f, f+1, f+256, f+V/2, f+3*(V/64)+5, V-1-p} -- the next row (the same GEMV row group
          when f is even), the same batched-argmax thread one stride later (vocab > 16384), the
          same GEMV block one grid-stride later, another batched slice, the last block / slice;
  p odd:  {f, f+V/2}; position 1 is {999, 1000}, straddling TOKEN_TEXT_MIN, so the chosen id is
          a control token and its twin the first id the alternatives may hold.

Eight classes of rows are written, class c to the members of position (c + rot) % 8: synthetic
row 3500 + c//2 scaled by 16 (4 added to every nonzero bf16 exponent field, exact), negated
when c is odd.  Of +-16 l_k, k = 0..3, the largest is 16 max|l_k|, so the winning logit always
falls in a tied class, and `rot` moves the winning class through all eight positions.

Vocab sizes: 4096, 8192 and 65536 select the 2-, 4- and 8-row groups of the LM-head GEMV and
64, 128 and 1024 ids per batched argmax slice (1024: 4 ids per thread).
"""
import dataclasses
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "voxtral.c_amd"))
import vox_weights as vw  # noqa: E402

VOCABS = (4096, 8192, 65536)
N_POS = 8
BASE_ROW = 3500                # classes 2k and 2k+1 come from the untouched row BASE_ROW + k
STEPS = 12                     # the 400-frame mel gives 50 adapter rows: 38 prefill + 12 steps
TEXT_MIN = 1000                # TOKEN_TEXT_MIN
RESERVED = (1, 2, 32)          # BOS, EOS, streaming pad
EMB = vw.EMB + ".tok_embeddings.weight"


def cfg_for(V):
    return dataclasses.replace(vw.TINY, vocab=V)


def smoke_mel(cfg):
    """the mel of __graft_entry__.smoke()"""
    return np.random.default_rng(0).uniform(-0.5, 1.5, size=(400, cfg.mel_bins)).astype(np.float32)


def first_ids(V):
    return [5, 999, 1002, 1023, V // 2 - 40, 1500, 2030, 3001]


def positions(V):
    """member ids of the eight positions, ascending (the first id is the lowest)"""
    out = []
    for p, f in enumerate(first_ids(V)):
        far = f + V // 2
        if p % 2 == 0:
            m = [f, f + 1, f + 256, far if far < V else f + 7, f + 3 * (V // 64) + 5, V - 1 - p]
        elif f == 999:
            m = [999, 1000]
        else:
            m = [f, far if far < V else f + V // 4]
        assert m[0] == min(m) and max(m) < V, (V, p, m)
        out.append(sorted(m))
    flat = [i for m in out for i in m]
    assert len(set(flat)) == len(flat), (V, out)
    assert not set(flat) & set(RESERVED), (V, out)
    assert not set(flat) & set(range(BASE_ROW, BASE_ROW + N_POS // 2)), (V, out)
    return out


def class_row(base_rows, c):
    """row of class c from the untouched rows BASE_ROW..BASE_ROW+3: x16, negated when c is odd"""
    r = base_rows[c // 2].astype(np.uint16).copy()
    e = (r >> 7) & 0xff
    assert int(e.max()) + 4 < 255
    r = np.where(e != 0, r + np.uint16(4 << 7), r).astype(np.uint16)
    if c & 1:
        r ^= np.uint16(0x8000)
    return r


def class_members(V, rot):
    """member ids of class c = 0..7 (position (c + rot) % 8)"""
    pos = positions(V)
    return [pos[(c + rot) % N_POS] for c in range(N_POS)]


def _with_embedding(base, emb):
    t = dict(base.t)
    t[EMB] = emb
    return vw.Weights(base.cfg, t, keep=base)


def tie_weights(cfg, rot, seed=1, base=None):
    """synth_weights(cfg, seed) with the rows of tok_embeddings.weight at the tie positions
    rewritten; base: an untouched synth_weights(cfg, seed) to share every other tensor with
    (it is left unchanged)"""
    if base is None:
        base = vw.synth_weights(cfg, seed=seed)
    src = base.t[EMB]
    emb = src.copy()
    rows = src[BASE_ROW:BASE_ROW + N_POS // 2]
    for c, members in enumerate(class_members(cfg.vocab, rot)):
        emb[members] = class_row(rows, c)
    return _with_embedding(base, emb)


def requantize_head(base_q8, w):
    """quantize_q8(w) for a w that differs from the bf16 weights behind base_q8 only in
    tok_embeddings.weight: that tensor alone goes through the quantiser again"""
    q = vw.quantize_q8(vw.Weights(w.cfg, {EMB: w.t[EMB]}))
    q8 = dict(base_q8.q8)
    q8[EMB] = q.q8[EMB]
    return vw.Weights(w.cfg, {}, q8=q8, f32=base_q8._stored_f32)


def tie_step(lg, V, rot):
    """What one step's logits [V] say about the fixture: (ids at the maximum, the position
    whose members they are or None, (max - next distinct logit) / max|logit|, whether the
    logits of every class are bit-identical)"""
    lg = np.ascontiguousarray(lg, np.float32)
    top = float(lg.max())
    at_max = np.flatnonzero(lg == top).tolist()
    pos = positions(V)
    which = next((p for p, m in enumerate(pos) if m == at_max), None)
    below = lg[lg < top]
    gap = (top - float(below.max())) / float(np.max(np.abs(lg))) if below.size else 0.0
    bits = lg.view(np.uint32)
    same = all(len(set(bits[m].tolist())) == 1 for m in class_members(V, rot))
    return at_max, which, gap, same


def zero_head(cfg, seed=1, base=None):
    """tok_embeddings.weight all zero, +0 on even rows and -0 on odd rows: every logit is +-0,
    so every block and every slice of the device's reductions ties"""
    if base is None:
        base = vw.synth_weights(cfg, seed=seed)
    emb = np.zeros_like(base.t[EMB])
    emb[1::2] = 0x8000
    return _with_embedding(base, emb)
