"""The opt-in FP8 (OCP E4M3, no scale, saturating at 448: csrc/vox_kv8.h) encoder K/V rings
(vox_hip_model_set_enc_kv_dtype(m, 2); no reference counterpart).  The test-for-test twin of
tests/test_gpu_enc_kv16.py at its shapes, with the one-byte format's rules.

The reference is tests/enc_kv_ref.py, the restatement of the oracle's incremental encoder with a
hook at the K/V append (pinned to the oracle by tests/test_enc_kv16_cpu.py).  The comparisons:

  exact      layer-0 K/V do not depend on the ring type, so every layer-0 code of an FP8 stream is
             vox_kv8_encode of the f32 stream's element, bit for bit.
  ring-conditioned   the hook first holds the GPU's stored row to the reference's own row: a code
             equals the reference's rounding, or is the adjacent code across a rounding boundary
             that lies within ACT_TOL x max|reference row| of the reference's unrounded value (the
             f32 bar on the values before the store: only then can the two sides round apart).
             Anything else fails; no share of elements is exempt.  The hook then returns the GPU's
             decoded rows, so both sides attend identical rings and the adapter rows sit within the
             project's f32 bar, 5e-5 of the largest magnitude.
  ring rule  two GPU runs whose kernels sum in different orders hold f32 K/V rows that agree
             within the f32 bar before the store; the stored rows a, b then obey
                 |a - b| <= ACT_TOL (16/15) max|row| + 2^-4 (|a| + |b|) + 2^-9
             -- the f32 bar taken on the stored row's maximum and corrected for its own rounding
             (a stored maximum is at least 15/16 of the value it came from), each store's half
             step, at most 2^-4 of the stored magnitude, and two half steps of a subnormal
             (2^-10 each).  Nothing in it is measured.  It holds only while nothing saturates,
             which test 3 asserts (largest stored magnitude far below 448).
"""
import ctypes
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ACT_TOL = 5e-5
F32, F16, FP8 = 0, 1, 2
NP_DT = {F32: np.float32, F16: np.float16, FP8: np.uint8}
_SETTER_CALLED = False


def _mel(cfg, seed, frames):
    return np.random.default_rng(seed).uniform(-0.6, 1.4, size=(frames, cfg.mel_bins)).astype(np.float32)


def _stream(hm, dtype):
    """a stream of the given encoder ring type; the model's switch is left off"""
    global _SETTER_CALLED
    import vox_hip
    _SETTER_CALLED = True
    hm.set_enc_kv_dtype(dtype)
    s = vox_hip.Stream(hm)
    hm.set_enc_kv_dtype(F32)
    assert s.enc_kv_dtype == dtype and s.enc_kv_fp16 == (dtype == F16)
    return s


# ---- csrc/vox_kv8.h through libvox_synth.so ---------------------------------------------------
def _synth():
    from vox_weights import synth_lib
    L = synth_lib()
    L.vox_kv8_encode_n.argtypes = [ctypes.c_void_p, ctypes.c_longlong, ctypes.c_void_p, ctypes.c_void_p]
    L.vox_kv8_encode_n.restype = None
    L.vox_kv8_decode_n.argtypes = [ctypes.c_void_p, ctypes.c_longlong, ctypes.c_void_p]
    L.vox_kv8_decode_n.restype = None
    return L


def _encode(x):
    """vox_kv8_encode_n: the codes of f32 values, shape kept"""
    x = np.ascontiguousarray(x, np.float32)
    codes = np.empty(x.shape, np.uint8)
    _synth().vox_kv8_encode_n(x.ctypes.data, x.size, codes.ctypes.data, None)
    return codes


def _decode(codes):
    codes = np.ascontiguousarray(codes, np.uint8)
    out = np.empty(codes.shape, np.float32)
    _synth().vox_kv8_decode_n(codes.ctypes.data, codes.size, out.ctypes.data)
    return out


_POS = None


def _pos_values():
    """the 127 finite non-negative values, ascending; code = index"""
    global _POS
    if _POS is None:
        _POS = _decode(np.arange(0x7f, dtype=np.uint8)).astype(np.float64)
        assert _POS[0] == 0 and _POS[-1] == 448 and np.all(np.diff(_POS) > 0)
    return _POS


def _signed_index(codes):
    """the codes' rank on the value axis: ... 0x81 -> -2, -0 -> -1, +0 -> 0, 0x01 -> 1 ..."""
    c = codes.astype(np.int64)
    mag = c & 0x7f
    return np.where(c & 0x80, -1 - mag, mag)


def _boundary_below(u):
    """the value at which the rounding passes from signed index u - 1 to u: the midpoint of the two
    values, 0 between the two zeros"""
    P = _pos_values()
    up = np.clip(u, 1, 126)
    dn = np.clip(-u, 1, 126)
    return np.where(u >= 1, (P[up - 1] + P[up]) / 2, np.where(u == 0, 0.0, -(P[dn] + P[dn - 1]) / 2))


def _check_codes(ref, codes, what):
    """The ring-conditioned rule of the module docstring for one block of rows: ref [n, kvd] the
    reference's unrounded f32 rows, codes the GPU's.  Returns the number of adjacent-code elements."""
    ref = np.ascontiguousarray(ref, np.float32)
    assert codes.dtype == np.uint8 and codes.shape == ref.shape
    assert not np.any((codes & 0x7f) == 0x7f), what + ": NaN code"
    want = _encode(ref)
    bad = codes != want
    if not bad.any():
        return 0
    gi, wi = _signed_index(codes), _signed_index(want)
    assert np.all(np.abs(gi - wi)[bad] == 1), f"{what}: {int(np.sum(np.abs(gi - wi) > 1))} codes further than one from the reference's"
    bnd = _boundary_below(np.maximum(gi, wi))
    tol = ACT_TOL * np.max(np.abs(ref.astype(np.float64)), axis=1, keepdims=True)
    dist = np.abs(bnd - ref.astype(np.float64))
    far = bad & (dist > tol)
    assert not far.any(), (f"{what}: {int(far.sum())} adjacent codes whose rounding boundary is further than the f32 bar "
                           f"from the reference's value, worst {float(np.max(np.where(far, dist / tol, 0))):.2f} bars")
    return int(bad.sum())


def _checking_ring_hook(stream, stats):
    """the ring-conditioned hook: check the GPU's stored rows, then adopt them"""
    def hook(k, v, layer, pos):
        gk, gv = stream.read_enc_kv(layer, pos, k.shape[0])
        stats["adjacent"] += _check_codes(k, gk, f"layer {layer} pos {pos} K")
        stats["adjacent"] += _check_codes(v, gv, f"layer {layer} pos {pos} V")
        stats["elements"] += gk.size + gv.size
        return _decode(gk), _decode(gv)
    return hook


def _assert_layer0_exact(s32, s8, first, n, what):
    k32, v32 = s32.read_enc_kv(0, first, n)
    k8, v8 = s8.read_enc_kv(0, first, n)
    assert k8.dtype == np.uint8 and k32.dtype == np.float32
    assert float(np.max(np.abs(k32))) > 0 and float(np.max(np.abs(v32))) > 0
    assert np.array_equal(k8, _encode(k32)), f"{what} K: {int(np.sum(k8 != _encode(k32)))} codes"
    assert np.array_equal(v8, _encode(v32)), f"{what} V: {int(np.sum(v8 != _encode(v32)))} codes"
    # decoded=True is the exact value of the codes
    kd, vd = s8.read_enc_kv(0, first, min(n, 8), decoded=True)
    assert kd.dtype == np.float32 and np.array_equal(kd, _decode(k8[:8])) and np.array_equal(vd, _decode(v8[:8]))


def _assert_ring_rule(a, b, what):
    """The ring rule of the module docstring over decoded rows a, b [n, kvd].  Returns the number
    of elements that differ."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    d = np.abs(a - b)
    rowmax = np.maximum(np.max(np.abs(a), axis=1, keepdims=True), np.max(np.abs(b), axis=1, keepdims=True))
    bar = ACT_TOL * (16.0 / 15.0) * rowmax + 2.0 ** -4 * (np.abs(a) + np.abs(b)) + 2.0 ** -9
    assert np.all(d <= bar), f"{what}: {int(np.sum(d > bar))} elements outside the ring rule, worst {float(np.max(d / bar)):.2f} bars"
    return int(np.count_nonzero(d))


def _smoke_run(hm, cfg):
    """the smoke inputs (TINY, 400 frames of rng(0), 8 greedy steps): adapter rows, ids"""
    import vox_hip
    mel = np.random.default_rng(0).uniform(-0.5, 1.5, size=(400, cfg.mel_bins)).astype(np.float32)
    s = vox_hip.Stream(hm)
    assert s.enc_kv_dtype == F32 and not s.enc_kv_fp16
    n = s.encode_mel(mel)
    rows = s.read_adapter()
    ids = np.asarray(s.decode(max_steps=8, stop_at_eos=False))
    s.close()
    assert n == rows.shape[0] > 0 and len(ids) == 8
    return rows, ids


@pytest.fixture(scope="module", autouse=True)
def pristine(tiny_cfg, tiny_weights):
    """Runs before the module's first test: a stream created before any setter call of this module."""
    import vox_hip
    assert not _SETTER_CALLED
    hm = vox_hip.Model(tiny_cfg, tiny_weights)
    out = _smoke_run(hm, tiny_cfg)
    hm.close()
    return out


@pytest.fixture(scope="module")
def models(tiny_cfg, tiny_weights):
    import vox_hip
    import vox_oracle
    from vox_weights import TINY_LONG
    vox_oracle.set_threads(min(16, os.cpu_count() or 1))
    hm, hl = vox_hip.Model(tiny_cfg, tiny_weights), vox_hip.Model(TINY_LONG, tiny_weights)
    yield {"TINY": hm, "TINY_LONG": hl}
    hm.close()
    hl.close()


# ---------------------------------------------------------------------------------------------
# 1. layer 0 is exact, before and after the ring wraps
# ---------------------------------------------------------------------------------------------
def test_layer0_ring_is_kv8_encode_of_the_f32_ring_through_the_wrap(models, tiny_cfg):
    """2400 frames = 1200 rows through every single-stream path (a 550-row pass, 25-row chunks,
    1-row chunks, a 60-row chunk) into rings of 24 + 1024 + 64 = 1112 slots: checked at 1000 rows
    (nothing overwritten) and at the end (slots 0..87 hold positions 1112..1199)."""
    import enc_kv_ref
    hm = models["TINY"]
    ecap = tiny_cfg.enc_window + 1024 + 64
    mel = _mel(tiny_cfg, 6100, 2400)
    sizes = [1100] + [50] * 8 + [2, 120, 2] + [50] * 7 + [26] + [50] * 100
    pieces = enc_kv_ref.chunks(mel, sizes)
    s32, s8 = _stream(hm, F32), _stream(hm, FP8)
    rows, checked_mid = 0, False
    for p in pieces:
        a, b = s32.encode_mel(p), s8.encode_mel(p)
        assert a == b
        rows += p.shape[0] // 2
        if not checked_mid and rows >= 1000:
            assert rows < ecap
            _assert_layer0_exact(s32, s8, 0, rows, "before the wrap")
            checked_mid = True
    assert checked_mid and rows == 1200 > ecap
    _assert_layer0_exact(s32, s8, rows - ecap, ecap, "after the wrap")
    with pytest.raises(RuntimeError):
        s8.read_enc_kv(0, rows - ecap - 1, 1)       # overwritten
    with pytest.raises(RuntimeError):
        s8.read_enc_kv(0, rows, 1)                  # not appended
    s32.close()
    s8.close()


# ---------------------------------------------------------------------------------------------
# 2. ring-conditioned parity, once per path
# ---------------------------------------------------------------------------------------------
def _ring_conditioned(hm, cfg, weights, mel, sizes):
    """GPU FP8 stream over the chunks, then the restatement checking and attending the GPU's stored
    rows; returns (rel err of the adapter rows, hook stats, the FP8 stream -- still open)"""
    import enc_kv_ref
    pieces = enc_kv_ref.chunks(mel, sizes)
    s = _stream(hm, FP8)
    added = [s.encode_mel(p) for p in pieces]
    assert sum(p.shape[0] for p in pieces) // 2 < cfg.enc_window + 1024 + 64      # every row still resident
    stats = {"adjacent": 0, "elements": 0}
    ref = enc_kv_ref.RefEncoder(cfg, weights, _checking_ring_hook(s, stats))
    assert [ref.encode_mel(p) for p in pieces] == added
    got, want = s.read_adapter(), ref.adapter()
    assert got.shape == want.shape and got.shape[0] > 0 and stats["elements"] > 0
    return enc_kv_ref.rel(got, want), stats, s


NO_PASSES = {"gemv_row": 0, "fused": 0, "slab": 0, "rows": 0, "fused_split": 0}
PATHS = {
    # name: (config, mel frames per chunk, the passes Stream.enc_paths() must report); rows = frames / 2
    "gemm_200_rows": ("TINY", [400], {"rows": 1}),
    "fused_25_row_chunks": ("TINY", [50] * 6, {"fused": 6}),
    "one_row_chunks": ("TINY", [50, 2, 2, 50, 2, 6], {"gemv_row": 3, "fused": 3}),
    # 25 rows against 325..375 keys: every fused chunk's attention on the split grid + combine
    "split_grid_and_combine": ("TINY_LONG", [600, 50, 50, 50], {"rows": 1, "fused": 3, "fused_split": 3}),
}


@pytest.mark.parametrize("name", list(PATHS))
def test_ring_conditioned_parity(models, tiny_weights, name):
    from vox_weights import TINY, TINY_LONG
    cfg_name, sizes, passes = PATHS[name]
    cfg = {"TINY": TINY, "TINY_LONG": TINY_LONG}[cfg_name]
    r, st, s = _ring_conditioned(models[cfg_name], cfg, tiny_weights, _mel(cfg, 6200 + len(sizes), sum(sizes)), sizes)
    took = s.enc_paths()
    s.close()
    assert took == {**NO_PASSES, **passes}, took      # the path the case is named after really ran
    print(f"ring-conditioned fp8 {name}: adapter rows rel {r:.2e}, {st['adjacent']} adjacent codes of {st['elements']}")
    assert r < ACT_TOL, r


def test_ring_conditioned_parity_slab_path(tiny_cfg, tiny_weights):
    """The split-K slab chain (k_skl + k_slabs_rope_kv) is what a Q8 model's chunks of up to 80
    rows take: 25-, 70- and 9-row chunks of a quantize_q8 TINY."""
    import vox_hip
    from vox_weights import quantize_q8
    w8 = quantize_q8(tiny_weights)
    hm = vox_hip.Model(tiny_cfg, w8)
    sizes = [50, 140, 18, 50]
    r, st, s = _ring_conditioned(hm, tiny_cfg, w8, _mel(tiny_cfg, 6300, sum(sizes)), sizes)
    took = s.enc_paths()
    s.close()
    hm.close()
    assert took == {**NO_PASSES, "slab": 4}, took
    print(f"ring-conditioned fp8 slab path (Q8): adapter rows rel {r:.2e}, {st['adjacent']} adjacent codes of {st['elements']}")
    assert r < ACT_TOL, r


# ---------------------------------------------------------------------------------------------
# 3. the rounding is applied
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg_name,sizes", [("TINY", [400]), ("TINY_LONG", [600, 50, 50, 50])])
def test_rounding_is_applied_and_nothing_saturates(models, tiny_weights, cfg_name, sizes):
    """The FP8 stream's adapter rows are far from the f32 oracle's: more than 1e-3 of the largest
    magnitude (the restatement with the host FP8 hook gives 2.9e-2 on TINY [400] and 3.2e-2 on
    TINY_LONG [600, 50, 50, 50] on the CPU; an f32 or half ring gives 2e-4 at the most).  And no
    stored element is near the format's limit (4.7 at the most on the CPU): the ring rule of the
    batched test and of the twin depends on nothing saturating at 448."""
    import enc_kv_ref
    import vox_oracle
    from vox_weights import TINY, TINY_LONG
    cfg = {"TINY": TINY, "TINY_LONG": TINY_LONG}[cfg_name]
    mel = _mel(cfg, 6400, sum(sizes))
    pieces = enc_kv_ref.chunks(mel, sizes)
    s = _stream(models[cfg_name], FP8)
    for p in pieces:
        s.encode_mel(p)
    got = s.read_adapter()
    rows = sum(sizes) // 2
    big = max(float(np.max(np.abs(x))) for l in range(cfg.enc_layers) for x in s.read_enc_kv(l, 0, rows, decoded=True))
    s.close()
    om = vox_oracle.OracleModel(cfg, tiny_weights)
    os_ = vox_oracle.OracleStream(om)
    for p in pieces:
        os_.encode_mel(p)
    f32 = os_.read_adapter()
    os_.close()
    om.close()
    d = enc_kv_ref.rel(got, f32)
    print(f"enc kv8 {cfg_name} {sizes}: adapter rows rel {d:.3e} to the f32 oracle, largest stored magnitude {big:.3g}")
    assert d > 1e-3, d
    assert big < 448, big


# ---------------------------------------------------------------------------------------------
# 4. the batched pass
# ---------------------------------------------------------------------------------------------
ROUNDS = [[50, 36, 120, 0], [50, 2, 50, 64], [30, 0, 50, 50]]      # mel frames per stream and round


def _rings(s, cfg, rows, decoded=False):
    return [s.read_enc_kv(l, 0, rows, decoded=decoded) for l in range(cfg.enc_layers)]


def test_batched_pass_of_fp8_streams_equals_single_streams(models, tiny_cfg):
    """4 FP8 streams, ragged chunks, one of them idle in two of the three rounds, through
    encode_mel_batch against the same chunks one stream at a time.  Adapter rows: within the f32
    bar.  Rings: the stacked rows go through the M > 1 GEMM, a single stream's chunk of up to 80
    rows through the skinny kernels, so the f32 K/V differ in summation order and the stored
    codes, decoded, obey the ring rule of the module docstring (every layer).  Bit-equal rings are
    asserted where the kernels are the same: a batched call in which only one stream has rows runs
    that stream's own path (fresh streams, so that the conv tails and the history are the same)."""
    import enc_kv_ref
    import vox_hip
    hm, cfg = models["TINY"], tiny_cfg
    mels = [_mel(cfg, 6500 + i, sum(r[i] for r in ROUNDS)) for i in range(4)]
    bs, ss = [_stream(hm, FP8) for _ in range(4)], [_stream(hm, FP8) for _ in range(4)]
    offs = [0] * 4
    for r in ROUNDS:
        chunk = [mels[i][offs[i]:offs[i] + r[i]] for i in range(4)]
        added = vox_hip.encode_mel_batch(bs, chunk)
        single = [ss[i].encode_mel(chunk[i]) if r[i] else 0 for i in range(4)]
        assert added == single, (added, single)
        offs = [o + n for o, n in zip(offs, r)]
    flips = 0
    for i in range(4):
        a, b = bs[i].read_adapter(), ss[i].read_adapter()
        assert a.shape == b.shape and a.shape[0] > 0
        assert enc_kv_ref.rel(a, b) < ACT_TOL, (i, enc_kv_ref.rel(a, b))
        rows = offs[i] // 2
        for l, ((ka, va), (kb, vb)) in enumerate(zip(_rings(bs[i], cfg, rows, True), _rings(ss[i], cfg, rows, True))):
            flips += _assert_ring_rule(ka, kb, f"stream {i} layer {l} K")
            flips += _assert_ring_rule(va, vb, f"stream {i} layer {l} V")
    print(f"batched fp8 pass: {flips} ring elements differ from the single streams'")
    for s in bs + ss:
        s.close()
    # one stream with rows: the same kernels, the same bits, every layer
    extra = _mel(cfg, 6510, 100)
    f1, f2, g = _stream(hm, FP8), _stream(hm, FP8), _stream(hm, FP8)
    for lo in (0, 50):
        piece = extra[lo:lo + 50]
        assert vox_hip.encode_mel_batch([f1, f2], [piece, piece[:0]])[0] == g.encode_mel(piece)
    assert np.array_equal(f1.read_adapter(), g.read_adapter())
    for (ka, va), (kb, vb) in zip(_rings(f1, cfg, 50), _rings(g, cfg, 50)):
        assert ka.dtype == np.uint8 and np.array_equal(ka, kb) and np.array_equal(va, vb)
    for s in (f1, f2, g):
        s.close()


# ---------------------------------------------------------------------------------------------
# 5. mixed lists
# ---------------------------------------------------------------------------------------------
def _mixed_against_own_groups(hm, cfg, types, frames, seed):
    """One call over streams of `types` against one call per type (in the order in which the list
    first names the types) on fresh streams: added[] in list order, adapter rows and every ring
    bit-equal.  Returns the mixed streams (open) and their mels."""
    import vox_hip
    B = len(types)
    mels = [_mel(cfg, seed + i, sum(f[i] for f in frames)) for i in range(B)]
    mixed = [_stream(hm, t) for t in types]
    own = [_stream(hm, t) for t in types]
    order = list(dict.fromkeys(types))
    offs = [0] * B
    for f in frames:
        chunk = [mels[i][offs[i]:offs[i] + f[i]] for i in range(B)]
        added = vox_hip.encode_mel_batch(mixed, chunk)
        want = [None] * B
        for t in order:
            idx = [i for i in range(B) if types[i] == t]
            for i, a in zip(idx, vox_hip.encode_mel_batch([own[i] for i in idx], [chunk[i] for i in idx])):
                want[i] = a
        assert added == want, (added, want)
        offs = [o + n for o, n in zip(offs, f)]
    for i in range(B):
        assert mixed[i].enc_kv_dtype == types[i]
        a, b = mixed[i].read_adapter(), own[i].read_adapter()
        assert a.shape[0] > 0 and a.tobytes() == b.tobytes(), i
        for (ka, va), (kb, vb) in zip(_rings(mixed[i], cfg, offs[i] // 2), _rings(own[i], cfg, offs[i] // 2)):
            assert ka.dtype == NP_DT[types[i]]
            assert ka.tobytes() == kb.tobytes() and va.tobytes() == vb.tobytes(), i
    for s in own:
        s.close()
    return mixed, mels


def test_mixed_list_of_three_types_gives_each_type_its_own_pass(models, tiny_cfg):
    """[fp8, f32, half, fp8, half, f32] in one call against three calls of one type each on fresh
    streams: the mixed call forms exactly those three passes."""
    hm, cfg = models["TINY"], tiny_cfg
    frames = [[50, 70, 36, 120, 50, 64], [50, 50, 64, 2, 36, 70]]
    mixed, mels = _mixed_against_own_groups(hm, cfg, [FP8, F32, F16, FP8, F16, F32], frames, 6600)
    # and the fp8 stream's deeper layer is not what an f32 ring would have given it
    s = _stream(hm, F32)
    off = 0
    for f in frames:
        s.encode_mel(mels[0][off:off + f[0]])
        off += f[0]
    assert not np.array_equal(mixed[0].read_enc_kv(1, 0, 8, decoded=True)[0], s.read_enc_kv(1, 0, 8)[0])
    s.close()
    for m in mixed:
        m.close()


def test_half_and_f32_list_on_a_model_that_never_selected_fp8(tiny_cfg, tiny_weights):
    """[half, f32, half, f32] on a fresh model on which FP8 is never selected: bit-equal to the
    same call's two groups run separately, as before the third type existed."""
    import vox_hip
    hm = vox_hip.Model(tiny_cfg, tiny_weights)
    mixed, _ = _mixed_against_own_groups(hm, tiny_cfg, [F16, F32, F16, F32], [[50, 70, 36, 120], [50, 50, 64, 2]], 6650)
    for m in mixed:
        m.close()
    hm.close()


# ---------------------------------------------------------------------------------------------
# 6. the scheduler
# ---------------------------------------------------------------------------------------------
PIECE = 8000


def test_scheduler_serves_all_three_ring_types(models, jfk_samples):
    """6 TINY streams on one vh_sched, f32, half and FP8 alternating (the scheduler's encoder pass
    gets a list of three types every tick): each stream's ids equal its own single-stream session
    of the same ring type on the same pieces."""
    import vox_hip
    global _SETTER_CALLED
    hm = models["TINY"]
    types = [F32, F16, FP8, F32, F16, FP8]
    audios = [np.ascontiguousarray(jfk_samples[int(k * 9000):][:int(sec * 16000)])
              for k, sec in enumerate([3.0, 4.5, 2.5, 4.0, 3.5, 2.0])]
    ctx = vox_hip.HostCtx(hm)
    _SETTER_CALLED = True

    def make(dtype, q=None):
        ctx.set_enc_kv_dtype(dtype)
        s = vox_hip.HostStream(ctx, interval_s=0.5)
        ctx.set_enc_kv_dtype(F32)
        if q is not None:
            q.attach(s)
        assert vox_hip.host_lib().vh_stream_enc_kv_dtype(s.h) == dtype
        assert bool(vox_hip.host_lib().vh_stream_enc_kv_fp16(s.h)) == (dtype == F16)
        return s

    ref = []
    for a, t in zip(audios, types):
        s = make(t)
        ids = []
        for i in range(0, len(a), PIECE):
            s.feed(a[i:i + PIECE])
            ids += s.get()
        s.finish()
        ids += s.get()
        s.close()
        assert len(ids) > 0
        ref.append(ids)
    n = len(types)
    q = vox_hip.Scheduler(ctx, n)
    ss = [make(t, q) for t in types]
    pos, done, ids = [0] * n, [False] * n, [[] for _ in range(n)]
    while not all(done) or any(s.pending() for s in ss):
        for k, (a, s) in enumerate(zip(audios, ss)):
            if done[k]:
                continue
            if pos[k] < len(a):
                s.feed(a[pos[k]:pos[k] + PIECE])
                pos[k] += PIECE
            else:
                s.finish()
                done[k] = True
        q.run()
        for k, s in enumerate(ss):
            ids[k] += s.get()
    st = q.stats()
    for s in ss:
        s.close()
    q.close()
    ctx.close()
    assert st["enc_batches"] > 0, st
    for k in range(n):
        assert ids[k] == ref[k], (k, len(ids[k]), len(ref[k]))


# ---------------------------------------------------------------------------------------------
# 7. the reference-boundary twin
# ---------------------------------------------------------------------------------------------
def test_encoder_full_step_twin_on_an_fp8_stream(models, tiny_cfg, tiny_weights):
    """vox_hip_encoder_full_step over the conv-stem rows of a 300-frame chunk (the CPU oracle's
    stem, as the reference's call site feeds it) on an FP8 stream.  Its layer-0 ring is
    vox_kv8_encode of an f32 stream's twin call bit for bit; against encode_mel's rings (device
    conv stem: f32 inputs that differ in summation order) every layer obeys the ring rule.  The
    twin does not advance the stream's encoder position, so each stream first encodes another mel
    of the same length, which the twin then overwrites (asserted)."""
    import vox_oracle
    hm, cfg = models["TINY"], tiny_cfg
    mel, other = _mel(cfg, 6700, 300), _mel(cfg, 6701, 300)
    om = vox_oracle.OracleModel(cfg, tiny_weights)
    stem = vox_oracle.OracleStream(om)
    x = stem.conv_stem(mel)
    stem.close()
    om.close()
    n = x.shape[0]
    assert n == 150
    rope = vox_oracle.rope_freqs(np.arange(n), cfg.enc_head_dim, cfg.rope_theta)
    t8, t32, e8 = _stream(hm, FP8), _stream(hm, F32), _stream(hm, FP8)
    for s in (t8, t32):
        s.encode_mel(other)
    before = _rings(t8, cfg, n)
    y8 = t8.twin_encoder_full_step(x, rope, 0)
    y32 = t32.twin_encoder_full_step(x, rope, 0)
    e8.encode_mel(mel)
    after = _rings(t8, cfg, n)
    assert not np.array_equal(before[0][0], after[0][0])
    _assert_layer0_exact(t32, t8, 0, n, "twin")
    assert y8.shape == y32.shape and not np.array_equal(y8, y32)      # deeper layers attend rounded rows
    for l, ((ka, va), (kb, vb)) in enumerate(zip(after, _rings(e8, cfg, n))):
        _assert_ring_rule(_decode(ka), _decode(kb), f"twin layer {l} K")
        _assert_ring_rule(_decode(va), _decode(vb), f"twin layer {l} V")
    for s in (t8, t32, e8):
        s.close()


# ---------------------------------------------------------------------------------------------
# 8. the real encoder geometry
# ---------------------------------------------------------------------------------------------
def test_full_encoder_geometry():
    """Voxtral's encoder dimensions (1280 wide, 32 heads of 64: ring rows of 2048 columns, 5120
    hidden, window 750) on two layers of synthetic weights and TINY's decoder: 105 rows (GEMM
    path) then 25 (fused chunk).  Layer-0 exactness and the ring-conditioned bar, once."""
    from dataclasses import replace

    import enc_kv_ref
    import vox_hip
    from vox_weights import TINY, synth_weights
    cfg = replace(TINY, enc_dim=1280, enc_heads=32, enc_kv_heads=32, enc_hidden=5120, enc_window=750)
    w = synth_weights(cfg, seed=3)
    hm = vox_hip.Model(cfg, w)
    sizes = [210, 50]
    mel = _mel(cfg, 6800, sum(sizes))
    r, st, s8 = _ring_conditioned(hm, cfg, w, mel, sizes)
    s32 = _stream(hm, F32)
    for p in enc_kv_ref.chunks(mel, sizes):
        s32.encode_mel(p)
    assert s8.read_enc_kv(0, 0, 130)[0].shape == (130, 2048)
    _assert_layer0_exact(s32, s8, 0, 130, "full geometry")
    assert s8.enc_kv_bytes * 4 == s32.enc_kv_bytes == 2 * 2 * (750 + 1024 + 64) * 2048 * 4
    s8.close()
    s32.close()
    hm.close()
    print(f"ring-conditioned fp8 full geometry: adapter rows rel {r:.2e}, {st['adjacent']} adjacent codes of {st['elements']}")
    assert r < ACT_TOL, r


# ---------------------------------------------------------------------------------------------
# 9. memory, the default, the switches
# ---------------------------------------------------------------------------------------------
def test_fp8_stream_takes_a_quarter_of_the_encoder_ring_bytes(models, tiny_cfg):
    import vox_hip
    hm, c = models["TINY"], tiny_cfg
    L = vox_hip.lib()
    m0 = L.vox_hip_memory_used()
    s32 = _stream(hm, F32)
    m1 = L.vox_hip_memory_used()
    s8 = _stream(hm, FP8)
    m2 = L.vox_hip_memory_used()
    ring32 = 2 * c.enc_layers * (c.enc_window + 1024 + 64) * c.enc_kv_heads * c.enc_head_dim * 4
    assert s32.enc_kv_bytes == ring32 and s8.enc_kv_bytes * 4 == ring32
    assert (m1 - m0) - (m2 - m1) == ring32 // 4 * 3, (m1 - m0, m2 - m1, ring32)
    s32.close()
    s8.close()


def test_default_is_untouched(pristine, models, tiny_cfg, tiny_weights):
    """Nothing set: enc_kv_dtype is 0 (asserted on every smoke stream), and adapter rows and ids on
    the smoke inputs are np.array_equal to those of a stream created before any setter call of this
    module -- on a model that has had FP8 on and off again and has an FP8 stream alive, and on a
    fresh model."""
    import vox_hip
    rows0, ids0 = pristine
    hm = models["TINY"]
    s8 = _stream(hm, FP8)
    s8.encode_mel(_mel(tiny_cfg, 6900, 100))
    assert _SETTER_CALLED
    rows, ids = _smoke_run(hm, tiny_cfg)
    assert np.array_equal(rows, rows0) and np.array_equal(ids, ids0)
    s8.close()
    fresh = vox_hip.Model(tiny_cfg, tiny_weights)
    rows, ids = _smoke_run(fresh, tiny_cfg)
    fresh.close()
    assert np.array_equal(rows, rows0) and np.array_equal(ids, ids0)


def test_setters_and_environment(tiny_cfg, tiny_weights):
    """set_enc_kv_fp16 keeps its meaning next to the dtype setter; a dtype outside 0..2 is refused;
    VOX_HIP_ENC_KV_FP8 is read at model creation and wins over VOX_HIP_ENC_KV_FP16; at an encoder
    head_dim other than 64 the variable is ignored and the setter refuses dtype 2, naming it."""
    from dataclasses import replace

    import vox_hip
    from vox_weights import synth_weights
    global _SETTER_CALLED
    _SETTER_CALLED = True
    saved = {k: os.environ.pop(k, None) for k in ("VOX_HIP_ENC_KV_FP8", "VOX_HIP_ENC_KV_FP16")}
    try:
        hm = vox_hip.Model(tiny_cfg, tiny_weights)
        for call, arg, want in ((hm.set_enc_kv_fp16, True, F16), (hm.set_enc_kv_dtype, FP8, FP8),
                                (hm.set_enc_kv_fp16, True, F16), (hm.set_enc_kv_fp16, False, F32),
                                (hm.set_enc_kv_dtype, F16, F16), (hm.set_enc_kv_dtype, F32, F32)):
            call(arg)
            s = vox_hip.Stream(hm)
            assert s.enc_kv_dtype == want and s.enc_kv_fp16 == (want == F16)
            s.close()
        with pytest.raises(RuntimeError):
            hm.set_enc_kv_dtype(3)
        hm.close()
        os.environ["VOX_HIP_ENC_KV_FP8"] = "1"
        os.environ["VOX_HIP_ENC_KV_FP16"] = "1"
        hm = vox_hip.Model(tiny_cfg, tiny_weights)
        s = vox_hip.Stream(hm)
        assert s.enc_kv_dtype == FP8 and not s.enc_kv_fp16
        s.close()
        hm.close()
        cfg128 = replace(tiny_cfg, enc_heads=tiny_cfg.enc_heads // 2, enc_kv_heads=tiny_cfg.enc_kv_heads // 2, enc_head_dim=128)
        hm = vox_hip.Model(cfg128, synth_weights(cfg128, seed=5))
        s = vox_hip.Stream(hm)
        assert s.enc_kv_dtype == F32
        s.close()
        with pytest.raises(RuntimeError, match="128"):
            hm.set_enc_kv_dtype(FP8)
        hm.close()
    finally:
        for k, v in saved.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v
