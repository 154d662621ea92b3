"""A Python restatement of the CPU oracle's incremental encoder (oracle/vox_oracle.c:
vo_conv_stem, vo_encoder_incremental, vo_adapter and the residual handling of
vo_stream_encode_mel), composed only from the ops oracle/vox_oracle.py exports (causal_conv1d,
gelu, rms_norm, linear_bf16 -- linear_q8 for a Q8 checkpoint's matrices, as the oracle's own lin()
picks it --, rope_freqs, apply_rope, causal_attention, silu), with a hook at the K/V append:

    round_fn(k, v, layer, pos) -> (k, v)

k / v are the new rows [n, enc_kv_heads * enc_head_dim] of logical encoder positions
pos .. pos + n - 1 as the oracle would append them; what the hook returns is what the cache
holds and every later attention reads.  The identity gives the oracle's f32 session bit for bit
(tests/test_enc_kv16_cpu.py pins it), f16_hook a session whose ring holds IEEE half values, and a
hook that returns a GPU stream's stored rows makes the session *ring-conditioned*: both sides
attend identical rings, so the comparison stays at the f32 ring's bar (tests/test_gpu_enc_kv16.py).
The precedent is tests/kv8_ref.py (the decoder's session).

The oracle compacts its cache to the window before a chunk that would overflow it; that only
moves rows.  Here the history is kept by logical position and each chunk's attention gets the
keys from the first one its first query can see.
"""
import numpy as np

import vox_oracle
from vox_weights import EMB, ENC

ACT_TOL = 5e-5    # the project's f32 activation bar, of the reference's largest magnitude


def identity_hook(k, v, layer, pos):
    return k, v


def f16_hook(k, v, layer, pos):
    return vox_oracle.f16_round(k).reshape(k.shape), vox_oracle.f16_round(v).reshape(v.shape)


def rel(got, ref):
    """max |got - ref| / max |ref|"""
    return float(np.max(np.abs(np.asarray(got, np.float32) - ref)) / max(1e-6, float(np.max(np.abs(ref)))))


class RefEncoder:
    """One stream's encoder session: encode_mel(mel chunk) -> adapter rows added; adapter()."""

    def __init__(self, cfg, weights, round_fn=identity_hook):
        self.c, self.w, self.round_fn = cfg, weights, round_fn
        c = cfg
        self.kvd = c.enc_kv_heads * c.enc_head_dim
        self.K = [np.zeros((0, self.kvd), np.float32) for _ in range(c.enc_layers)]
        self.V = [np.zeros((0, self.kvd), np.float32) for _ in range(c.enc_layers)]
        self.pos = 0                      # next logical encoder position
        self.conv_init = False
        self.mel_tail = np.zeros((c.mel_bins, 2), np.float32)
        self.conv0_tail = np.zeros((c.enc_dim, 2), np.float32)
        self.conv0_res = None             # the odd conv0 column kept for the next chunk
        self.enc_res = np.zeros((0, c.enc_dim), np.float32)
        self.rows = []                    # adapter rows

    # ---- weights -------------------------------------------------------------------------
    def _lin(self, x, name, bias=None):
        """the oracle's lin(): bf16 bits, or int8 rows with their scales"""
        d, sc = self.w.matrix(name)
        return vox_oracle.linear_bf16(x, d, bias) if sc is None else vox_oracle.linear_q8(x, d, sc, bias)

    def _proj(self, x, l, name, bias=None):
        b = None if bias is None else self._vec(l, bias)
        return self._lin(x, f"{ENC}.transformer.layers.{l}.{name}.weight", b)

    def _vec(self, l, name):
        return self.w.f32(f"{ENC}.transformer.layers.{l}.{name}")

    # ---- vo_conv_stem --------------------------------------------------------------------
    def conv_stem(self, mel):
        c, w = self.c, self.w
        mel = np.ascontiguousarray(mel, np.float32)
        n = mel.shape[0]
        if n <= 0:
            return np.zeros((0, c.enc_dim), np.float32)
        w0, b0 = w.f32(f"{ENC}.conv_layers.0.conv.weight"), w.f32(f"{ENC}.conv_layers.0.conv.bias")
        w1, b1 = w.f32(f"{ENC}.conv_layers.1.conv.weight"), w.f32(f"{ENC}.conv_layers.1.conv.bias")
        first = not self.conv_init
        if first:
            c0 = vox_oracle.gelu(vox_oracle.causal_conv1d(mel.T, w0, b0, 1), c.gelu_erf)
            self.conv_init = True
        else:
            cin = np.concatenate([self.mel_tail, mel.T], axis=1)
            c0 = vox_oracle.gelu(vox_oracle.causal_conv1d(cin, w0, b0, 1), c.gelu_erf)[:, 2:]
        tail = np.zeros((c.mel_bins, 2), np.float32)
        tc = min(n, 2)
        tail[:, 2 - tc:] = mel[n - tc:].T
        self.mel_tail = tail
        # stride alignment
        prev = 0 if self.conv0_res is None else 1
        new_res = (prev + n) & 1
        feed_new = n - new_res
        if prev + feed_new <= 0:
            if new_res:
                self.conv0_res = c0[:, -1].copy()
            return np.zeros((0, c.enc_dim), np.float32)
        parts = ([self.conv0_res[:, None]] if prev else []) + [c0[:, :feed_new]]
        feed = np.ascontiguousarray(np.concatenate(parts, axis=1))
        self.conv0_res = c0[:, -1].copy() if new_res else None
        c1_in = feed if first else np.concatenate([self.conv0_tail, feed], axis=1)
        self.conv0_tail = feed[:, -2:].copy()
        c1 = vox_oracle.gelu(vox_oracle.causal_conv1d(c1_in, w1, b1, 2)[:, :c1_in.shape[1] // 2], c.gelu_erf)
        return np.ascontiguousarray(c1[:, (0 if first else 1):].T)

    # ---- vo_encoder_incremental ----------------------------------------------------------
    def layers(self, x):
        c = self.c
        H, KVH, hd = c.enc_heads, c.enc_kv_heads, c.enc_head_dim
        n, pos0 = x.shape[0], self.pos
        if n <= 0:
            return x
        rope = vox_oracle.rope_freqs(np.arange(pos0, pos0 + n), hd, c.rope_theta)
        lo = max(0, pos0 - c.enc_window + 1)      # the first key any of these queries sees
        x = np.array(x, np.float32, copy=True)
        for l in range(c.enc_layers):
            xn = vox_oracle.rms_norm(x, self._vec(l, "attention_norm.weight"), c.enc_eps)
            q = self._proj(xn, l, "attention.wq", "attention.wq.bias")
            k = self._proj(xn, l, "attention.wk")
            v = self._proj(xn, l, "attention.wv", "attention.wv.bias")
            q = vox_oracle.apply_rope(q, rope, H, hd)
            k = vox_oracle.apply_rope(k, rope, KVH, hd)
            k, v = self.round_fn(k, v, l, pos0)
            self.K[l] = np.concatenate([self.K[l], np.asarray(k, np.float32)])
            self.V[l] = np.concatenate([self.V[l], np.asarray(v, np.float32)])
            att = vox_oracle.causal_attention(q, self.K[l][lo:], self.V[l][lo:], H, KVH, hd, c.enc_window, pos0 - lo)
            x = x + self._proj(att, l, "attention.wo", "attention.wo.bias")
            xn = vox_oracle.rms_norm(x, self._vec(l, "ffn_norm.weight"), c.enc_eps)
            gate = vox_oracle.silu(self._proj(xn, l, "feed_forward.w1"))
            gate = gate * self._proj(xn, l, "feed_forward.w3")
            x = x + self._proj(gate, l, "feed_forward.w2", "feed_forward.w2.bias")
        self.pos += n
        return vox_oracle.rms_norm(x, self.w.f32(f"{ENC}.transformer.norm.weight"), c.enc_eps)

    # ---- vo_adapter + the residual rows of vo_stream_encode_mel --------------------------
    def encode_mel(self, mel):
        c = self.c
        conv = self.conv_stem(mel)
        if conv.shape[0] <= 0:
            return 0
        enc = self.layers(conv)
        comb = np.concatenate([self.enc_res, enc])
        usable = comb.shape[0] // c.downsample * c.downsample
        added = 0
        if usable > 0:
            rows = np.ascontiguousarray(comb[:usable]).reshape(usable // c.downsample, c.downsample * c.enc_dim)
            mid = vox_oracle.gelu(self._lin(rows, f"{EMB}.audio_language_projection.0.weight"), c.gelu_erf)
            out = self._lin(mid, f"{EMB}.audio_language_projection.2.weight")
            self.rows.append(out)
            added = out.shape[0]
        self.enc_res = comb[usable:].copy()
        return added

    def adapter(self):
        if not self.rows:
            return np.zeros((0, self.c.dec_dim), np.float32)
        return np.concatenate(self.rows)


def gpu_ring_hook(stream):
    """The ring-conditioned hook: the rows the GPU stream stored for these positions (the stream
    must have encoded them already and still hold them), widened to f32."""
    def hook(k, v, layer, pos):
        gk, gv = stream.read_enc_kv(layer, pos, k.shape[0], decoded=True)
        return gk, gv
    return hook


def chunks(mel, sizes):
    """mel split into consecutive pieces of the given frame counts (the rest as a last piece)"""
    out, p = [], 0
    for n in sizes:
        out.append(mel[p:p + n])
        p += n
    if p < mel.shape[0]:
        out.append(mel[p:])
    return [m for m in out if m.shape[0] > 0]
