"""A Python restatement of the CPU oracle's decoder session (oracle/vox_oracle.c: dec_layers,
vo_decoder_prefill, vo_decoder_forward, step_embed and the prompt of vo_stream_decode), composed
only from the ops oracle/vox_oracle.py exports (rms_norm, linear_bf16, rope_freqs, apply_rope,
causal_attention, silu), with a hook at the K/V append:

    round_fn(k, v, layer, pos) -> (k, v)

k / v are the new rows [seq, kv_heads * head_dim] of logical positions pos .. pos + seq - 1 as the
oracle would append them; what the hook returns is what the cache holds and every later attention
reads.  The identity gives the oracle's f32 session bit for bit, vox_oracle.f16_round its fp16-KV
session (tests/test_kv8_cpu.py pins both), kv8_round an FP8 E4M3 ring, and a hook that returns a
GPU stream's stored rows makes the session *ring-conditioned*: both sides attend identical rings,
so the comparison stays at the f32 ring's bar however coarse the ring's element is
(tests/test_gpu_kv8.py).

Also here: a numpy statement of the FP8 E4M3 rule of csrc/vox_kv8.h written by hand (np_kv8_*),
the ctypes view of the C functions (c_kv8_*), and the per-element ring comparison rule.
"""
import ctypes

import numpy as np

import vox_oracle
from vox_weights import bf16_to_f32, synth_lib

TOKEN_BOS = 1
TOKEN_STREAMING_PAD = 32


# ---- the FP8 E4M3 rule, by hand in numpy (float64 arithmetic is exact for every step) ----------
def np_kv8_values():
    """the 256 codes' values (float64; NaN for S.1111.111)"""
    c = np.arange(256)
    e, m = (c >> 3) & 15, (c & 7).astype(np.float64)
    v = np.where(e == 0, m * 2.0 ** -9, (8.0 + m) * 2.0 ** (e - 10.0))
    v[(c & 0x7f) == 0x7f] = np.nan
    return np.where(c & 0x80, -v, v)


_POS = np_kv8_values()[:0x7f]          # the 127 finite non-negative values, ascending, code = index


def np_kv8_encode(x):
    """clamp to +-448, nearest value, ties to the even mantissa (= the even code), subnormals
    kept, sign of zero kept, NaN -> 0x7f with the sign"""
    x = np.asarray(x, np.float32)
    sign = ((x.view(np.uint32) >> 24) & 0x80).astype(np.uint8)
    with np.errstate(invalid="ignore"):                       # (signalling NaN inputs)
        a = np.minimum(np.abs(x.astype(np.float64)), 448.0)   # NaN stays NaN through np.minimum
    nan = np.isnan(a)
    a = np.where(nan, 0.0, a)
    hi = np.clip(np.searchsorted(_POS, a, side="left"), 1, 0x7e)   # _POS[hi - 1] <= a <= _POS[hi] (a > 0)
    lo = hi - 1
    dl, dh = a - _POS[lo], _POS[hi] - a
    code = np.where(dl < dh, lo, np.where(dh < dl, hi, np.where(lo % 2 == 0, lo, hi)))
    code = np.where(nan, 0x7f, code).astype(np.uint8)
    return code | sign


def np_kv8_decode(codes):
    return np_kv8_values().astype(np.float32)[np.asarray(codes, np.uint8)]


def np_kv8_round(x):
    return np_kv8_decode(np_kv8_encode(x))


def kv8_midpoints():
    """the 126 midpoints between adjacent non-negative values (all exact in f32), ascending,
    and 464, the midpoint between 448 and the value the NaN code's bits would have"""
    return ((_POS[:-1] + _POS[1:]) / 2).astype(np.float32)


# ---- csrc/vox_kv8.h through libvox_synth.so ----------------------------------------------------
def _synth():
    L = synth_lib()
    if not getattr(L, "_kv8_sig", False):
        L.vox_kv8_encode.argtypes = [ctypes.c_float]
        L.vox_kv8_encode.restype = ctypes.c_uint8
        L.vox_kv8_decode.argtypes = [ctypes.c_uint8]
        L.vox_kv8_decode.restype = ctypes.c_float
        L.vox_kv8_round.argtypes = [ctypes.c_float]
        L.vox_kv8_round.restype = ctypes.c_float
        L.vox_kv8_encode_n.argtypes = [ctypes.c_void_p, ctypes.c_longlong, ctypes.c_void_p, ctypes.c_void_p]
        L.vox_kv8_encode_n.restype = None
        L.vox_kv8_decode_n.argtypes = [ctypes.c_void_p, ctypes.c_longlong, ctypes.c_void_p]
        L.vox_kv8_decode_n.restype = None
        L._kv8_sig = True
    return L


def c_kv8_encode(x):
    """(codes, decoded) of csrc/vox_kv8.h over an array"""
    x = np.ascontiguousarray(x, np.float32)
    codes = np.empty(x.shape, np.uint8)
    back = np.empty(x.shape, np.float32)
    _synth().vox_kv8_encode_n(x.ctypes.data, x.size, codes.ctypes.data, back.ctypes.data)
    return codes, back


def c_kv8_decode(codes):
    codes = np.ascontiguousarray(codes, np.uint8)
    out = np.empty(codes.shape, np.float32)
    _synth().vox_kv8_decode_n(codes.ctypes.data, codes.size, out.ctypes.data)
    return out


def kv8_round(x):
    """decode(encode(x)) by the C rule, shape kept"""
    return c_kv8_encode(x)[1]


def kv8_hook(k, v, layer, pos):
    return kv8_round(k), kv8_round(v)


def identity_hook(k, v, layer, pos):
    return k, v


def f16_hook(k, v, layer, pos):
    return vox_oracle.f16_round(k).reshape(k.shape), vox_oracle.f16_round(v).reshape(v.shape)


# ---- the decoder session -----------------------------------------------------------------------
class RefDecoder:
    """One stream's decoder session over its adapter rows [n, dec_dim] (an OracleStream's
    read_adapter()).  ada = OracleModel.ada_scale().  decode() follows vo_stream_decode."""

    def __init__(self, cfg, weights, adapter, ada, round_fn=identity_hook, delay_tokens=6):
        assert not weights.is_q8
        self.c, self.w = cfg, weights
        self.adapter = np.ascontiguousarray(adapter, np.float32)
        self.ada = np.ascontiguousarray(ada, np.float32)
        self.round_fn = round_fn
        self.prompt_len = 1 + 32 + delay_tokens
        self.tok_emb_bits = weights.bf16("mm_streams_embeddings.embedding_module.tok_embeddings.weight")
        kvd = cfg.dec_kv_heads * cfg.dec_head_dim
        cap = self.adapter.shape[0] + 2
        # the whole history by logical position (the oracle's cache without its compaction, which
        # only moves rows: the attention's window picks the keys)
        self.K = np.zeros((cfg.dec_layers, cap, kvd), np.float32)
        self.V = np.zeros((cfg.dec_layers, cap, kvd), np.float32)
        self.pos = 0
        self.gen_pos = 0
        self.started = False
        self.prev_token = TOKEN_BOS

    def _mat(self, l, name):
        return self.w.bf16(f"layers.{l}.{name}.weight")

    def _norm(self, l, name):
        return self.w.f32(f"layers.{l}.{name}.weight")

    def embed(self, row, token):
        """step_embed: adapter row + the token's bf16 embedding"""
        return self.adapter[row] + bf16_to_f32(self.tok_emb_bits[token])

    def layers(self, x, pos0):
        """dec_layers over x [seq, dec_dim] at logical positions pos0 ..; returns the new x"""
        c = self.c
        H, KVH, hd = c.dec_heads, c.dec_kv_heads, c.dec_head_dim
        seq = x.shape[0]
        rope = vox_oracle.rope_freqs(np.arange(pos0, pos0 + seq), hd, c.rope_theta)
        x = np.array(x, np.float32, copy=True)
        for l in range(c.dec_layers):
            xn = vox_oracle.rms_norm(x, self._norm(l, "attention_norm"), c.dec_eps)
            q = vox_oracle.linear_bf16(xn, self._mat(l, "attention.wq"))
            k = vox_oracle.linear_bf16(xn, self._mat(l, "attention.wk"))
            v = vox_oracle.linear_bf16(xn, self._mat(l, "attention.wv"))
            q = vox_oracle.apply_rope(q, rope, H, hd)
            k = vox_oracle.apply_rope(k, rope, KVH, hd)
            k, v = self.round_fn(k, v, l, pos0)
            self.K[l, pos0:pos0 + seq] = k
            self.V[l, pos0:pos0 + seq] = v
            att = vox_oracle.causal_attention(q, self.K[l, :pos0 + seq], self.V[l, :pos0 + seq], H, KVH, hd,
                                              c.dec_window, pos0)
            x = x + vox_oracle.linear_bf16(att, self._mat(l, "attention.wo"))
            xn = vox_oracle.rms_norm(x, self._norm(l, "ffn_norm"), c.dec_eps)
            xn = xn * (np.float32(1.0) + self.ada[l])[None, :]
            gate = vox_oracle.silu(vox_oracle.linear_bf16(xn, self._mat(l, "feed_forward.w1")))
            gate = gate * vox_oracle.linear_bf16(xn, self._mat(l, "feed_forward.w3"))
            x = x + vox_oracle.linear_bf16(gate, self._mat(l, "feed_forward.w2"))
        return x

    def prefill(self, embeds):
        self.layers(embeds, self.pos)
        self.pos += embeds.shape[0]

    def forward(self, embed):
        """vo_decoder_forward: (first-max argmax id, logits)"""
        x = self.layers(embed[None, :], self.pos)
        self.pos += 1
        x = vox_oracle.rms_norm(x, self.w.f32("norm.weight"), self.c.dec_eps)
        logits = vox_oracle.linear_bf16(x, self.tok_emb_bits)[0]
        return int(np.argmax(logits)), logits

    def step(self, force_token=None):
        """one step of vo_stream_decode (the first call runs the prompt); force_token: the id the
        next embedding is built from instead of this session's own argmax.  Returns (id, logits),
        or None when the adapter rows are used up."""
        if not self.started:
            if self.adapter.shape[0] < self.prompt_len:
                return None
            pe = np.stack([self.embed(i, TOKEN_BOS if i == 0 else TOKEN_STREAMING_PAD)
                           for i in range(self.prompt_len)])
            self.pos = 0
            self.prefill(pe[:-1])
            tok, lg = self.forward(pe[-1])
            self.gen_pos = self.prompt_len
            self.started = True
        else:
            if self.gen_pos >= self.adapter.shape[0]:
                return None
            tok, lg = self.forward(self.embed(self.gen_pos, self.prev_token))
            self.gen_pos += 1
        self.prev_token = tok if force_token is None else int(force_token)
        return tok, lg

    def decode(self, max_steps):
        ids, lgs = [], []
        while len(ids) < max_steps:
            r = self.step()
            if r is None:
                break
            ids.append(r[0])
            lgs.append(r[1])
        return np.array(ids, np.int32), np.stack(lgs) if lgs else np.zeros((0, self.c.vocab), np.float32)


def top2_margin(logits):
    """min over steps of (top1 - top2) / max|logit|"""
    lg = np.asarray(logits, np.float32)
    s = np.sort(lg, axis=1)
    return float(np.min((s[:, -1] - s[:, -2]) / np.max(np.abs(lg), axis=1)))


# ---- the ring comparison rule ------------------------------------------------------------------
ACT_TOL = 5e-5    # the project's f32 activation bar (LOGIT_TOL of tests/test_gpu_batch.py), of max|row|


def check_fp8_rows(ref_unrounded, gpu_decoded, what=""):
    """The rule for the rows [n, kvd] of one layer's K (or V): a GPU element equals the
    reference's rounding (as decoded values), or is the adjacent code across a midpoint that lies
    within ACT_TOL * max|row| of the reference's unrounded value.  Returns the number of
    adjacent-code elements; raises AssertionError on anything else."""
    ref = np.asarray(ref_unrounded, np.float32)
    gpu = np.asarray(gpu_decoded, np.float32)
    rc, rv = c_kv8_encode(ref)
    diff = ~((rv == gpu) | (np.isnan(rv) & np.isnan(gpu)))
    if not diff.any():
        return 0
    gc, gv = c_kv8_encode(gpu)
    assert np.array_equal(gv[diff], gpu[diff]), f"{what}: ring holds values that are no E4M3 value"
    vals = np_kv8_values()
    # codes order by magnitude within a sign; across zero (+0 / -0 neighbours) the values are equal
    # as decoded, so a differing pair has one sign
    r_c, g_c = rc[diff].astype(np.int64), gc[diff].astype(np.int64)
    assert np.all((r_c & 0x80) == (g_c & 0x80)) and np.all(np.abs(r_c - g_c) == 1), \
        f"{what}: {int(np.sum(np.abs(r_c - g_c) != 1))} elements are not the adjacent code"
    mid = (vals[r_c] + vals[g_c]) / 2
    bar = ACT_TOL * np.max(np.abs(ref), axis=1, keepdims=True) * np.ones_like(ref)
    dist = np.abs(mid - ref[diff].astype(np.float64))
    worst = float(np.max(dist / bar[diff]))
    assert np.all(dist <= bar[diff]), f"{what}: adjacent code with the midpoint {worst:.2f} bars away"
    return int(diff.sum())


# ---- the runs tests/test_gpu_kv8.py replays (and tests/test_kv8_cpu.py checks the margin of) ----
def _cfgs():
    from dataclasses import replace

    from vox_weights import TINY, TINY_LONG
    kv8 = replace(TINY, dec_heads=32, dec_kv_heads=8, dec_dim=768, dec_hidden=1280)   # tests/test_gpu_batch_kv8.py's KV8
    return {"TINY": TINY, "TINY_LONG": TINY_LONG, "W320": replace(TINY, dec_window=320), "KV8": kv8}


CFGS = _cfgs()
FRAMES_PER_ROW = 8            # mel frames per adapter row
MARGIN = 4 * ACT_TOL          # the replay's top-2 gap every id comparison needs

# name -> (config, mel seed, [steps per stream]); a stream of n steps gets 39 + n + 5 adapter rows.
# The seeds are the first from the base on at which the unforced FP8 reference's top-2 margin is
# at least MARGIN on every step of every stream (scanned on the CPU, pinned by test_kv8_cpu.py).
RUNS = {
    "long300": ("TINY_LONG", 4100, [300]),
    "wrap320": ("W320", 4200, [450]),
    "tiny48": ("TINY", 4300, [120]),
    "batch3": ("TINY_LONG", 4400, [60, 290, 100]),
    "batch17": ("KV8", 4501, [10 + (i % 3) for i in range(17)]),
    "gemv2": ("TINY_LONG", 4600, [50, 70]),
}


def run_mels(name, seed=None):
    cfg_name, s, steps = RUNS[name]
    cfg = CFGS[cfg_name]
    rng = np.random.default_rng(s if seed is None else seed)
    return [rng.uniform(-0.6, 1.4, size=(FRAMES_PER_ROW * (39 + n + 5), cfg.mel_bins)).astype(np.float32)
            for n in steps]


def oracle_adapter(om, mel, chunk=4096):
    """an oracle stream's adapter rows for a mel"""
    st = vox_oracle.OracleStream(om)
    for i in range(0, mel.shape[0], chunk):
        st.encode_mel(mel[i:i + chunk])
    a = st.read_adapter()
    st.close()
    return a
