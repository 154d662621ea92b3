"""The opt-in 16-bit (IEEE half) encoder K/V rings (vox_hip_model_set_enc_kv_fp16; no reference
counterpart, the reference's VOX_DECODER_KV_FP16 is decoder-only).

The CPU oracle has no encoder-KV rounding switch.  The reference here is tests/enc_kv_ref.py, a
restatement of the oracle's incremental encoder with a hook at the K/V append, pinned bit for bit
to the oracle by tests/test_enc_kv16_cpu.py.  Three kinds of comparison:

  exact      layer-0 K/V do not depend on the ring type (conv stem and layer-0 projection only), so
             every layer-0 element of a half stream is f16_round of the f32 stream's, bit for bit.
  ring-conditioned   the restatement's hook returns the rows the GPU stream stored, so both sides
             attend identical rings and the adapter rows sit within the project's f32 bar, 5e-5 of
             the largest magnitude, whatever the ring's element is.
  ring rule  two GPU runs whose kernels sum in different orders (a stacked pass on the M > 1
             GEMM against single streams on the skinny kernels; the twin fed a CPU conv stem) hold
             f32 K/V rows x_a, x_b that agree within the f32 bar, ACT_TOL of the row's largest
             magnitude, before the store; each store then moves its element by at most half a
             half ulp, 2^-11 of its magnitude (2^-25 for a subnormal).  So the stored rows obey
             |a - b| <= ACT_TOL max|row| + 2^-11 (|a| + |b|) + 2^-24: the f32 bar plus the
             format's precision, nothing measured.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ACT_TOL = 5e-5
_SETTER_CALLED = False


def _mel(cfg, seed, frames):
    return np.random.default_rng(seed).uniform(-0.6, 1.4, size=(frames, cfg.mel_bins)).astype(np.float32)


def _stream(hm, half):
    """a stream of the given encoder ring type; the model's switch is left off"""
    global _SETTER_CALLED
    import vox_hip
    _SETTER_CALLED = True
    hm.set_enc_kv_fp16(half)
    s = vox_hip.Stream(hm)
    hm.set_enc_kv_fp16(False)
    assert s.enc_kv_fp16 == half
    return s


def _smoke_run(hm, cfg):
    """the smoke inputs (TINY, 400 frames of rng(0), 8 greedy steps): adapter rows, ids"""
    import vox_hip
    mel = np.random.default_rng(0).uniform(-0.5, 1.5, size=(400, cfg.mel_bins)).astype(np.float32)
    s = vox_hip.Stream(hm)
    assert not s.enc_kv_fp16
    n = s.encode_mel(mel)
    rows = s.read_adapter()
    ids = np.asarray(s.decode(max_steps=8, stop_at_eos=False))
    s.close()
    assert n == rows.shape[0] > 0 and len(ids) == 8
    return rows, ids


@pytest.fixture(scope="module", autouse=True)
def pristine(tiny_cfg, tiny_weights):
    """Runs before the module's first test: a stream created before the setter was ever called in
    this process (no other test file calls it)."""
    import vox_hip
    assert not _SETTER_CALLED
    hm = vox_hip.Model(tiny_cfg, tiny_weights)
    out = _smoke_run(hm, tiny_cfg)
    hm.close()
    return out


@pytest.fixture(scope="module")
def models(tiny_cfg, tiny_weights):
    import os

    import vox_hip
    import vox_oracle
    from vox_weights import TINY_LONG
    vox_oracle.set_threads(min(16, os.cpu_count() or 1))
    hm, hl = vox_hip.Model(tiny_cfg, tiny_weights), vox_hip.Model(TINY_LONG, tiny_weights)
    yield {"TINY": hm, "TINY_LONG": hl}
    hm.close()
    hl.close()


def _half_bits(x_f32):
    """f16_round of f32 values as half bit patterns"""
    import vox_oracle
    r = vox_oracle.f16_round(x_f32).reshape(np.shape(x_f32))
    h = r.astype(np.float16)
    assert np.array_equal(h.astype(np.float32), r, equal_nan=True)
    return h.view(np.uint16)


def _assert_layer0_exact(s32, s16, first, n, what):
    k32, v32 = s32.read_enc_kv(0, first, n)
    k16, v16 = s16.read_enc_kv(0, first, n)
    assert k16.dtype == np.float16 and k32.dtype == np.float32
    assert float(np.max(np.abs(k32))) > 0 and float(np.max(np.abs(v32))) > 0
    assert np.array_equal(k16.view(np.uint16), _half_bits(k32)), what + " K"
    assert np.array_equal(v16.view(np.uint16), _half_bits(v32)), what + " V"


def _assert_one_half_ulp(a, b, what):
    """The ring rule of the module docstring over rows a, b [n, kvd] widened to f32.  Returns the
    number of elements that differ."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    d = np.abs(a - b)
    rowmax = np.maximum(np.max(np.abs(a), axis=1, keepdims=True), np.max(np.abs(b), axis=1, keepdims=True))
    bar = ACT_TOL * rowmax + 2.0 ** -11 * (np.abs(a) + np.abs(b)) + 2.0 ** -24
    assert np.all(d <= bar), f"{what}: {int(np.sum(d > bar))} elements outside the ring rule, worst {float(np.max(d / bar)):.2f} bars"
    return int(np.count_nonzero(d))


# ---------------------------------------------------------------------------------------------
# 1. layer 0 is exact, before and after the ring wraps
# ---------------------------------------------------------------------------------------------
def test_layer0_ring_is_f16_round_of_the_f32_ring_through_the_wrap(models, tiny_cfg):
    """2400 frames = 1200 rows through every single-stream path (a 550-row pass, 25-row chunks,
    1-row chunks, a 60-row chunk) into rings of 24 + 1024 + 64 = 1112 slots: checked at 1000 rows
    (nothing overwritten) and at the end (slots 0..87 hold positions 1112..1199)."""
    hm = models["TINY"]
    ecap = tiny_cfg.enc_window + 1024 + 64
    mel = _mel(tiny_cfg, 6100, 2400)
    sizes = [1100] + [50] * 8 + [2, 120, 2] + [50] * 7 + [26] + [50] * 100
    import enc_kv_ref
    pieces = enc_kv_ref.chunks(mel, sizes)
    s32, s16 = _stream(hm, False), _stream(hm, True)
    rows, checked_mid = 0, False
    for p in pieces:
        a, b = s32.encode_mel(p), s16.encode_mel(p)
        assert a == b
        rows += p.shape[0] // 2
        if not checked_mid and rows >= 1000:
            assert rows < ecap
            _assert_layer0_exact(s32, s16, 0, rows, "before the wrap")
            checked_mid = True
    assert checked_mid and rows == 1200 > ecap
    _assert_layer0_exact(s32, s16, rows - ecap, ecap, "after the wrap")
    with pytest.raises(RuntimeError):
        s16.read_enc_kv(0, rows - ecap - 1, 1)       # overwritten
    with pytest.raises(RuntimeError):
        s16.read_enc_kv(0, rows, 1)                  # not appended
    s32.close()
    s16.close()


# ---------------------------------------------------------------------------------------------
# 2. ring-conditioned parity, once per path
# ---------------------------------------------------------------------------------------------
def _ring_conditioned(hm, cfg, weights, mel, sizes):
    """GPU half stream over the chunks, then the restatement attending the GPU's stored rows;
    returns (rel err of the adapter rows, GPU rows, the half stream -- still open)"""
    import enc_kv_ref
    pieces = enc_kv_ref.chunks(mel, sizes)
    s = _stream(hm, True)
    added = [s.encode_mel(p) for p in pieces]
    assert sum(p.shape[0] for p in pieces) // 2 < cfg.enc_window + 1024 + 64      # every row still resident
    ref = enc_kv_ref.RefEncoder(cfg, weights, enc_kv_ref.gpu_ring_hook(s))
    assert [ref.encode_mel(p) for p in pieces] == added
    got, want = s.read_adapter(), ref.adapter()
    assert got.shape == want.shape and got.shape[0] > 0
    return enc_kv_ref.rel(got, want), got, s


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
    r, _, s = _ring_conditioned(models[cfg_name], cfg, tiny_weights, _mel(cfg, 6200 + len(sizes), sum(sizes)), sizes)
    took = s.enc_paths()
    s.close()
    assert took == {**NO_PASSES, **passes}, took      # the path the case is named after really ran
    print(f"ring-conditioned {name}: adapter rows rel {r:.2e}")
    assert r < ACT_TOL, r


def test_ring_conditioned_parity_slab_path(tiny_cfg, tiny_weights):
    """The split-K slab chain (k_skl + k_slabs_rope_kv) is what a Q8 model's chunks of up to 80
    rows take: 25-, 70- and 9-row chunks of a quantize_q8 TINY."""
    import vox_hip
    from vox_weights import quantize_q8
    w8 = quantize_q8(tiny_weights)
    hm = vox_hip.Model(tiny_cfg, w8)
    sizes = [50, 140, 18, 50]
    r, _, s = _ring_conditioned(hm, tiny_cfg, w8, _mel(tiny_cfg, 6300, sum(sizes)), sizes)
    took = s.enc_paths()
    s.close()
    hm.close()
    assert took == {**NO_PASSES, "slab": 4}, took
    print(f"ring-conditioned slab path (Q8): adapter rows rel {r:.2e}")
    assert r < ACT_TOL, r


# ---------------------------------------------------------------------------------------------
# 3. the rounding is applied, and is the right one
# ---------------------------------------------------------------------------------------------
# distance of the GPU's adapter rows to the f16-hook restatement on the seeded inputs below
# (max |diff| / max |ref|): 2.735e-05 measured on an MI355X, against 2.291e-04 to the f32 oracle
# (profiles/enc_kv16_gputest.txt), and the margin over it
F16_MEASURED = 2.74e-5
F16_MARGIN = 3.0


def test_rounding_is_applied_and_is_f16_round(models, tiny_weights):
    """TINY_LONG, 300 rows then three 25-row chunks (up to 375 keys per query).  The GPU's adapter
    rows are closer to the restatement whose hook is f16_round than to the f32 oracle.  The
    distance to the f16 restatement is not at the f32 bar: the GPU rounds its own f32 K/V, which
    differ from the CPU's in summation order (~1e-7), so an element next to a rounding boundary
    lands one half ulp (2^-11 relative) away and every later row sees it; how many do is a
    property of the inputs.  The bar is therefore the value measured on these seeded inputs times
    F16_MARGIN, and it must stay below the distance to the f32 oracle (asserted), so a ring that
    rounds by another rule, or not at all, fails."""
    import enc_kv_ref
    import vox_oracle
    from vox_weights import TINY_LONG
    cfg, hm = TINY_LONG, models["TINY_LONG"]
    sizes = [600, 50, 50, 50]
    mel = _mel(cfg, 6400, sum(sizes))
    pieces = enc_kv_ref.chunks(mel, sizes)
    s = _stream(hm, True)
    for p in pieces:
        s.encode_mel(p)
    got = s.read_adapter()
    s.close()
    r16 = enc_kv_ref.RefEncoder(cfg, tiny_weights, enc_kv_ref.f16_hook)
    for p in pieces:
        r16.encode_mel(p)
    om = vox_oracle.OracleModel(cfg, tiny_weights)
    os_ = vox_oracle.OracleStream(om)
    for p in pieces:
        os_.encode_mel(p)
    f32 = os_.read_adapter()
    os_.close()
    om.close()
    d16, d32 = enc_kv_ref.rel(got, r16.adapter()), enc_kv_ref.rel(got, f32)
    print(f"enc kv16: adapter rows rel {d16:.3e} to the f16-hook restatement, {d32:.3e} to the f32 oracle")
    assert d16 < d32, (d16, d32)
    bar = F16_MEASURED * F16_MARGIN
    assert bar < d32, (bar, d32)
    assert d16 < bar, (d16, bar)


# ---------------------------------------------------------------------------------------------
# 4. the batched pass
# ---------------------------------------------------------------------------------------------
ROUNDS = [[50, 36, 120, 0], [50, 2, 50, 64], [30, 0, 50, 50]]      # mel frames per stream and round


def _rings(s, cfg, rows):
    return [s.read_enc_kv(l, 0, rows) for l in range(cfg.enc_layers)]


def test_batched_pass_of_half_streams_equals_single_streams(models, tiny_cfg):
    """4 half streams, ragged chunks, one of them idle in two of the three rounds, through
    encode_mel_batch against the same chunks one stream at a time.  Adapter rows: within the f32
    bar.  Rings: the stacked rows go through the M > 1 GEMM, a single stream's chunk of up to 80
    rows through the skinny kernels, so the f32 K/V differ in summation order and the stored
    halves obey the ring rule of the module docstring (every layer).  Bit-equal rings are asserted where the kernels
    are the same: a batched call in which only one stream has rows runs that stream's own path
    (fresh streams, so that the conv tails and the history are the same too)."""
    import enc_kv_ref
    import vox_hip
    hm, cfg = models["TINY"], tiny_cfg
    mels = [_mel(cfg, 6500 + i, sum(r[i] for r in ROUNDS)) for i in range(4)]
    bs, ss = [_stream(hm, True) for _ in range(4)], [_stream(hm, True) for _ in range(4)]
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
        for l, ((ka, va), (kb, vb)) in enumerate(zip(_rings(bs[i], cfg, rows), _rings(ss[i], cfg, rows))):
            flips += _assert_one_half_ulp(ka.astype(np.float32), kb.astype(np.float32), f"stream {i} layer {l} K")
            flips += _assert_one_half_ulp(va.astype(np.float32), vb.astype(np.float32), f"stream {i} layer {l} V")
    print(f"batched half pass: {flips} ring elements differ from the single streams'")
    for s in bs + ss:
        s.close()
    # one stream with rows: the same kernels, the same bits, every layer
    extra = _mel(cfg, 6510, 100)
    f1, f2, g = _stream(hm, True), _stream(hm, True), _stream(hm, True)
    for lo in (0, 50):
        piece = extra[lo:lo + 50]
        assert vox_hip.encode_mel_batch([f1, f2], [piece, piece[:0]])[0] == g.encode_mel(piece)
    assert np.array_equal(f1.read_adapter(), g.read_adapter())
    for (ka, va), (kb, vb) in zip(_rings(f1, cfg, 50), _rings(g, cfg, 50)):
        assert np.array_equal(ka.view(np.uint16), kb.view(np.uint16)) and np.array_equal(va.view(np.uint16), vb.view(np.uint16))
    for s in (f1, f2, g):
        s.close()


def test_mixed_list_gives_each_stream_its_own_types_pass(models, tiny_cfg):
    """[half, f32, half, f32] in one call against [half, half] and [f32, f32] in calls of their
    own on fresh streams: the mixed call forms exactly those two passes, so adapter rows and every
    ring are bit-equal, and added[] keeps the list's order."""
    import vox_hip
    hm, cfg = models["TINY"], tiny_cfg
    types = [True, False, True, False]
    frames = [[50, 70, 36, 120], [50, 50, 64, 2]]
    mels = [_mel(cfg, 6600 + i, sum(f[i] for f in frames)) for i in range(4)]
    mixed = [_stream(hm, t) for t in types]
    own = [_stream(hm, t) for t in types]
    offs = [0] * 4
    for f in frames:
        chunk = [mels[i][offs[i]:offs[i] + f[i]] for i in range(4)]
        added = vox_hip.encode_mel_batch(mixed, chunk)
        ah = vox_hip.encode_mel_batch([own[0], own[2]], [chunk[0], chunk[2]])
        af = vox_hip.encode_mel_batch([own[1], own[3]], [chunk[1], chunk[3]])
        assert added == [ah[0], af[0], ah[1], af[1]]
        offs = [o + n for o, n in zip(offs, f)]
    for i in range(4):
        assert mixed[i].enc_kv_fp16 == types[i]
        a, b = mixed[i].read_adapter(), own[i].read_adapter()
        assert a.shape[0] > 0 and np.array_equal(a, b), i
        for (ka, va), (kb, vb) in zip(_rings(mixed[i], cfg, offs[i] // 2), _rings(own[i], cfg, offs[i] // 2)):
            assert ka.dtype == (np.float16 if types[i] else np.float32)
            assert np.array_equal(ka, kb) and np.array_equal(va, vb), i
    # and the half streams differ from what an f32 ring would have given them
    assert not np.array_equal(mixed[0].read_enc_kv(1, 0, 8, decoded=True)[0],
                              _f32_rows_of(hm, mels[0], [f[0] for f in frames], 1, 8))
    for s in mixed + own:
        s.close()


def _f32_rows_of(hm, mel, sizes, layer, n):
    import enc_kv_ref
    s = _stream(hm, False)
    for p in enc_kv_ref.chunks(mel, sizes):
        s.encode_mel(p)
    k = s.read_enc_kv(layer, 0, n)[0]
    s.close()
    return k


# ---------------------------------------------------------------------------------------------
# 5. the scheduler
# ---------------------------------------------------------------------------------------------
PIECE = 8000


def test_scheduler_serves_both_ring_types(models, jfk_samples):
    """4 TINY streams on one vh_sched, half and f32 alternating (the scheduler's encoder pass gets
    a mixed list every tick): each stream's ids equal its own single-stream session of the same
    ring type on the same pieces."""
    import vox_hip
    global _SETTER_CALLED
    hm = models["TINY"]
    types = [True, False, True, False]
    audios = [np.ascontiguousarray(jfk_samples[int(k * 9000):][:int(sec * 16000)])
              for k, sec in enumerate([3.0, 4.5, 2.5, 4.0])]
    ctx = vox_hip.HostCtx(hm)
    _SETTER_CALLED = True

    def make(half, q=None):
        hm.set_enc_kv_fp16(half)
        s = vox_hip.HostStream(ctx, interval_s=0.5)
        hm.set_enc_kv_fp16(False)
        if q is not None:
            q.attach(s)
        assert bool(vox_hip.host_lib().vh_stream_enc_kv_fp16(s.h)) == half
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
    q = vox_hip.Scheduler(ctx, 4)
    ss = [make(t, q) for t in types]
    pos, done, ids = [0] * 4, [False] * 4, [[] for _ in range(4)]
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
    for k in range(4):
        assert ids[k] == ref[k], (k, len(ids[k]), len(ref[k]))


# ---------------------------------------------------------------------------------------------
# 6. the reference-boundary twin
# ---------------------------------------------------------------------------------------------
def test_encoder_full_step_twin_on_a_half_stream(models, tiny_cfg, tiny_weights):
    """vox_hip_encoder_full_step over the conv-stem rows of a 300-frame chunk (the CPU oracle's
    stem, as the reference's call site feeds it) on a half stream.  Its layer-0 ring is f16_round
    of an f32 stream's twin call bit for bit; against encode_mel's rings (device conv stem: f32
    inputs that differ in summation order) every layer obeys the ring rule.  The twin does not
    advance the stream's encoder position, so each stream first encodes another mel of the same
    length, which the twin then overwrites (asserted)."""
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
    t16, t32, e16 = _stream(hm, True), _stream(hm, False), _stream(hm, True)
    for s in (t16, t32):
        s.encode_mel(other)
    before = _rings(t16, cfg, n)
    y16 = t16.twin_encoder_full_step(x, rope, 0)
    y32 = t32.twin_encoder_full_step(x, rope, 0)
    e16.encode_mel(mel)
    after = _rings(t16, cfg, n)
    assert not np.array_equal(before[0][0], after[0][0])
    _assert_layer0_exact(t32, t16, 0, n, "twin")
    assert y16.shape == y32.shape and not np.array_equal(y16, y32)      # deeper layers attend rounded rows
    for l, ((ka, va), (kb, vb)) in enumerate(zip(after, _rings(e16, cfg, n))):
        _assert_one_half_ulp(ka.astype(np.float32), kb.astype(np.float32), f"twin layer {l} K")
        _assert_one_half_ulp(va.astype(np.float32), vb.astype(np.float32), f"twin layer {l} V")
    for s in (t16, t32, e16):
        s.close()


# ---------------------------------------------------------------------------------------------
# 7. the real encoder geometry
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
    r, _, s16 = _ring_conditioned(hm, cfg, w, mel, sizes)
    s32 = _stream(hm, False)
    for p in enc_kv_ref.chunks(mel, sizes):
        s32.encode_mel(p)
    assert s16.read_enc_kv(0, 0, 130)[0].shape == (130, 2048)
    _assert_layer0_exact(s32, s16, 0, 130, "full geometry")
    assert s16.enc_kv_bytes * 2 == s32.enc_kv_bytes == 2 * 2 * (750 + 1024 + 64) * 2048 * 4
    s16.close()
    s32.close()
    hm.close()
    print(f"ring-conditioned full geometry: adapter rows rel {r:.2e}")
    assert r < ACT_TOL, r


# ---------------------------------------------------------------------------------------------
# 8. memory, 9. the default
# ---------------------------------------------------------------------------------------------
def test_half_stream_takes_half_the_encoder_ring_bytes(models, tiny_cfg):
    import vox_hip
    hm, c = models["TINY"], tiny_cfg
    L = vox_hip.lib()
    m0 = L.vox_hip_memory_used()
    s32 = _stream(hm, False)
    m1 = L.vox_hip_memory_used()
    s16 = _stream(hm, True)
    m2 = L.vox_hip_memory_used()
    ring32 = 2 * c.enc_layers * (c.enc_window + 1024 + 64) * c.enc_kv_heads * c.enc_head_dim * 4
    assert s32.enc_kv_bytes == ring32 and s16.enc_kv_bytes * 2 == ring32
    assert (m1 - m0) - (m2 - m1) == ring32 // 2, (m1 - m0, m2 - m1, ring32)
    s32.close()
    s16.close()


def test_default_is_untouched(pristine, models, tiny_cfg, tiny_weights):
    """Switch off: adapter rows and ids on the smoke inputs are np.array_equal to those of a stream
    created before the setter was ever called in this process -- on a model that has had the
    switch on and off again and has a half stream alive, and on a fresh model."""
    import vox_hip
    rows0, ids0 = pristine
    hm = models["TINY"]
    s16 = _stream(hm, True)
    s16.encode_mel(_mel(tiny_cfg, 6900, 100))
    assert _SETTER_CALLED
    rows, ids = _smoke_run(hm, tiny_cfg)
    assert np.array_equal(rows, rows0) and np.array_equal(ids, ids0)
    s16.close()
    fresh = vox_hip.Model(tiny_cfg, tiny_weights)
    rows, ids = _smoke_run(fresh, tiny_cfg)
    fresh.close()
    assert np.array_equal(rows, rows0) and np.array_equal(ids, ids0)
