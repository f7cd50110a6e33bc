"""GPU: per-utterance start positions in one forward and one sampler call (echo_dit_forward_pos, echo_sample_euler_items_pos) and the
host scheduler on top of them (stream_batch.StreamBatcher).

Which kernel rotates in each case (engine.hip `plan_gemm`: the ping-pong kernel takes a bf16 GEMM once M x Npad >= 256 x 256 x 64):
  - tiny model (d = 256, QKVG N = 1024), bf16 AND fp32: the fused QKV tail of the TILE kernels (gemm_tile.h, its RoPE-modulus instantiation).
    The fp32 engine takes the fused tail too (d % 256 == 0); the unfused headnorm_rope path runs only for model sizes that are no multiple
    of 256, which no fixture has - it is the same kernel as before with other arguments (modulus B x S, gathered table);
  - WIDE1 (d = 2048, N = 8192) bf16 with M >= 512: gemm_pp_kernel's fused QKV tail (its RoPE-modulus instantiation).

Bit equality is asserted wherever the two sides run the same launches on the same geometry (same B, hence the same M and GEMM plans) and
rows are independent; distances to the reference's goldens use the suite's own bounds."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import echo_ref as R  # noqa: E402  (checker only)
from tests import gpu_util as U  # noqa: E402
from tests.golden_defs import SAMPLER_CASES, TINY, TINY_DAC, WIDE1  # noqa: E402

import echo_tts_amd as E  # noqa: E402
from echo_tts_amd import _lib as L  # noqa: E402
from echo_tts_amd import inference as inf  # noqa: E402
from echo_tts_amd import inference_blockwise as IB  # noqa: E402
from echo_tts_amd import stream_batch as SB  # noqa: E402

DEV = U.DEV
LAT_TOL = 1e-3      # the constant of tests/test_gpu_engine.py
ENGINES = ["f32", "bf16"]
DT = {"f32": torch.float32, "bf16": torch.bfloat16}


def rms(a, b):
    return float((a.float().cpu() - b.float().cpu()).pow(2).mean().sqrt())


@pytest.fixture(scope="module")
def tiny_models():
    w = R.make_dit_weights(TINY, seed=0)
    return {"f32": E.EchoDiT(TINY, w, dtype=torch.float32, device=DEV),
            "bf16": E.EchoDiT(TINY, {k: v.bfloat16() for k, v in w.items()}, dtype=torch.bfloat16, device=DEV)}


@pytest.fixture(scope="module")
def wide_model():
    w = R.make_dit_weights(WIDE1, seed=0)
    return E.EchoDiT(WIDE1, {k: v.bfloat16() for k, v in w.items()}, dtype=torch.bfloat16, device=DEV)


def _inputs(B, S, P, seed=11):
    """B utterances with different text lengths and voices, a latent prefix of P latents, CFG-layout rows (3 B)."""
    gen = torch.Generator().manual_seed(seed)
    ids = torch.randint(1, 256, (B, 24), generator=gen, dtype=torch.int32)
    tm = torch.zeros((B, 24), dtype=torch.bool)
    sm = torch.zeros((B, 16), dtype=torch.bool)
    for b in range(B):
        tm[b, :24 - 3 * b] = True
        sm[b, :16 - 4 * (b % 3)] = True
    spk = torch.randn((B, 16, 80), generator=gen)
    prefix = torch.randn((B, P, 80), generator=gen)
    x = torch.randn((3 * B, S, 80), generator=gen)
    tm3 = torch.cat([tm, torch.zeros_like(tm), tm], 0)
    sm3 = torch.cat([sm, sm, torch.zeros_like(sm)], 0)
    return ids, tm, spk, sm, prefix, x, tm3, sm3


def _caches(m, ids, tm, spk, sm, prefix):
    kvt = m.get_kv_cache_text(ids, tm)
    kvs = m.get_kv_cache_speaker(spk.to(m.dtype), sm)
    kvl = m.get_kv_cache_latent(prefix)
    return kvt, kvs, kvl


# ------------------------------------------------------------------------------------------------ 1. uniform == existing
@pytest.mark.parametrize("p", [0, 13])
@pytest.mark.parametrize("engine", ENGINES)
def test_uniform_positions_equal_the_existing_calls(golden, tiny_models, engine, p):
    """Every item at position p: echo_dit_forward_pos is echo_dit_forward_t(start_pos = p) and echo_sample_euler_items_pos is
    echo_sample_euler_items(start_pos = p), bit for bit (the gathered RoPE rows are copies of the rows the scalar form reads).  Latent prefix on:
    p = 0 sees no prefix key, p = 13 sees ceil(13 / 4) = 4."""
    _uniform_equals_existing(golden, tiny_models[engine], p)


def _uniform_equals_existing(g, m, p):
    B, S = 2, 32
    ids, tm, spk, sm, prefix, x, tm3, sm3 = _inputs(B, S, 16)
    kvt, kvs, kvl = _caches(m, ids, tm, spk, sm, prefix)
    t = torch.full((3 * B,), 0.7)
    a = m(x.to(m.dtype), t, tm3, sm3, kvt, kvs, start_pos=p, kv_cache_latent=kvl)
    b = m(x.to(m.dtype), t, tm3, sm3, kvt, kvs, start_pos=[p] * B, kv_cache_latent=kvl)
    assert float(a.abs().max()) > 0 and torch.equal(a, b)
    if p:   # the position matters at all: another position gives other bits
        assert not torch.equal(a, m(x.to(m.dtype), t, tm3, sm3, kvt, kvs, start_pos=[p, p - 1], kv_cache_latent=kvl))
    items = [dict(SAMPLER_CASES["cfg_default"]), dict(SAMPLER_CASES["cfg_default"], cfg_scale_text=2.0)]
    arr, temb, _keep = inf.build_sampler_items(m, [dict(it, rng_seed=0) for it in items])
    x0 = x[:B].to(DEV)
    sa = inf.run_euler_items(m, x0, arr, 6, temb, start_pos=p, use_latent=True)
    sb = inf.run_euler_items(m, x0, arr, 6, temb, start_pos=torch.tensor([p] * B), use_latent=True)
    assert bool(torch.isfinite(sa).all()) and torch.equal(sa, sb)


@pytest.mark.parametrize("engine", ENGINES)
def test_position_call_ending_on_the_last_rope_row(tiny_models, engine):
    """A position-only call reads its RoPE rows through the gather that clamps at an item's length, with every length S.  B = 2, S = 32, item 0 at
    0, item 1 at 13, and a RoPE table of exactly 13 + 32 rows (the model's own table, announced that short): item 1's last token reads the last
    row.  Each item of echo_dit_forward_pos / echo_sample_euler_items_pos has the bits of echo_dit_forward_t / echo_sample_euler_items with
    start_pos at that item's position (same B, caches and noise).  One position more is refused ("rope table") and writes nothing."""
    m = tiny_models[engine]
    B, S, P1 = 2, 32, 13
    positions = [0, P1]
    ids, tm, spk, sm, prefix, x, tm3, sm3 = _inputs(B, S, 16)
    kvt, kvs, kvl = _caches(m, ids, tm, spk, sm, prefix)
    t = torch.full((3 * B,), 0.7)
    xx = x.to(m.dtype)
    arr, temb, _keep = inf.build_sampler_items(m, [dict(SAMPLER_CASES["cfg_default"], rng_seed=0), dict(SAMPLER_CASES["cfg_default"], rng_seed=0, cfg_scale_text=2.0)])
    x0 = x[:B].to(DEV).contiguous()
    lib, ctx = m._lib, m._ctx
    L.check(lib.echo_set_rope_table(ctx, m._rope.data_ptr(), P1 + S), ctx)
    try:
        fwd = m(xx, t, tm3, sm3, kvt, kvs, start_pos=positions, kv_cache_latent=kvl)
        lat = inf.run_euler_items(m, x0, arr, 6, temb, start_pos=positions, use_latent=True)
        assert bool(torch.isfinite(fwd).all()) and bool(torch.isfinite(lat).all()) and float(lat.abs().max()) > 0
        for b, p in enumerate(positions):
            rows = [b, B + b, 2 * B + b]         # item b's cond / text-uncond / speaker-uncond rows
            uni = m(xx, t, tm3, sm3, kvt, kvs, start_pos=p, kv_cache_latent=kvl)
            assert torch.equal(fwd[rows], uni[rows]), (engine, "forward", b, p)
            assert not torch.equal(fwd[[1 - b]], uni[[1 - b]])         # teeth: the other item stands elsewhere
            ulat = inf.run_euler_items(m, x0, arr, 6, temb, start_pos=p, use_latent=True)
            assert torch.equal(lat[b], ulat[b]), (engine, "sampler", b, p)
            assert not torch.equal(lat[1 - b], ulat[1 - b])
        # one position more: refused before anything is queued
        past = (C.c_int32 * B)(0, P1 + 1)
        SENTINEL = 12345.0
        temb1 = torch.zeros((1, TINY.timestep_embed_size), dtype=m.dtype, device=DEV)
        out = torch.full((3 * B, S, 80), SENTINEL, dtype=torch.float32, device=DEV)
        on = (C.c_int32 * (3 * B))(*([1] * (3 * B)))
        xd = xx.to(DEV).contiguous()
        rc = lib.echo_dit_forward_pos(ctx, xd.data_ptr(), temb1.data_ptr(), 1, None, 3 * B, B, S, past, 1, on, on, out.data_ptr(), m._stream())
        assert rc != 0 and b"rope table" in lib.echo_last_error(ctx)
        p = L.EchoSamplerParams()
        p.B, p.S, p.num_steps, p.use_latent = B, S, 6, 1
        td = temb.to(DEV).contiguous()
        p.temb = td.data_ptr()
        o2 = torch.full_like(x0, SENTINEL)
        rc = lib.echo_sample_euler_items_pos(ctx, C.byref(p), arr, past, x0.data_ptr(), o2.data_ptr(), m._stream())
        assert rc != 0 and b"rope table" in lib.echo_last_error(ctx)
        torch.cuda.synchronize()
        assert bool((out == SENTINEL).all()) and bool((o2 == SENTINEL).all())
    finally:
        L.check(lib.echo_set_rope_table(ctx, m._rope.data_ptr(), m.MAX_POS), ctx)


# ------------------------------------------------------------------------------------------------ 2. staggered == uniform per item
def _staggered_equals_uniform(m, B, S, positions):
    assert len(positions) == B
    P = 28                                   # 7 prefix keys (patch 4): positions 0 / 5 / 16 / 27 see 0 / 2 / 4 / 7 of them
    ids, tm, spk, sm, prefix, x, tm3, sm3 = _inputs(B, S, P)
    kvt, kvs, kvl = _caches(m, ids, tm, spk, sm, prefix)
    t = torch.full((3 * B,), 0.7)
    xx = x.to(m.dtype)
    stag = m(xx, t, tm3, sm3, kvt, kvs, start_pos=list(positions), kv_cache_latent=kvl)
    assert bool(torch.isfinite(stag).all())
    uni, bad = {}, []
    for b, p in enumerate(positions):
        if p not in uni:
            uni[p] = m(xx, t, tm3, sm3, kvt, kvs, start_pos=int(p), kv_cache_latent=kvl)
        rows = [b, B + b, 2 * B + b]         # item b's cond / text-uncond / speaker-uncond rows
        d = float((stag[rows] - uni[p][rows]).abs().max())
        print(f"staggered vs uniform, {m.dtype} S={S} B={B}: item {b} at {p}: max |difference| {d:.3e}, bit-equal {torch.equal(stag[rows], uni[p][rows])}")
        if not torch.equal(stag[rows], uni[p][rows]):
            bad.append((b, p, d))
    assert not bad, bad
    # teeth: items at different positions differ from each other's uniform run
    ps = sorted(set(positions))
    if len(ps) > 1:
        b = list(positions).index(ps[0])
        assert not torch.equal(stag[b], uni[ps[1]][b])


@pytest.mark.parametrize("engine,S,B,positions", [
    ("bf16", 40, 5, [0, 5, 16, 27, 12]),     # M = 600: 128-row tiles and 32-row passes straddle the items (40 = 32 + 8)
    ("bf16", 20, 4, [0, 5, 16, 27]),         # S & 7 != 0: the element-wise transposed-V path next to the rotated q / k
    ("f32", 40, 5, [0, 5, 16, 27, 12]),      # fp32 engine: the fused tile tail as well (d % 256 == 0), fp32 instantiation
    ("f32", 20, 4, [0, 5, 16, 27]),
])
def test_staggered_equals_uniform_per_item_tiny(tiny_models, engine, S, B, positions):
    """Tile-kernel tail (see the module docstring for the path each engine takes).

    fp32: the parity engine's unfused attention lays a row's scores out as the concatenated columns of the active segments and sums a
    softmax row in column order, so a row's bits would depend on the widest prefix among its batch-mates (measured before the engine grouped
    the rows: the item at position 0 was 1 ulp, 5.96e-08, off the uniform call, which has no latent segment).  The engine therefore runs
    one attention pass per prefix width and keeps each row from the pass of its own width (engine.hip `attention_by_prefix_width`): the
    position-0 item here takes that path."""
    _staggered_equals_uniform(tiny_models[engine], B, S, positions)


@pytest.mark.parametrize("S,B,positions", [
    (96, 2, [27, 5]),                        # M = 576 >= 512: gemm_pp_kernel; a 256-row tile spans three rows
    (40, 5, [0, 5, 16, 27, 12]),             # M = 600: 16-token pieces straddle items, ragged last tile
])
def test_staggered_equals_uniform_per_item_wide_pingpong(wide_model, S, B, positions):
    """WIDE1 bf16: the ping-pong kernel's fused QKV tail."""
    _staggered_equals_uniform(wide_model, B, S, positions)


# ------------------------------------------------------------------------------------------------ 3. the reference, teacher-forced
@pytest.mark.parametrize("tag", ["tiny", "tinyb2"])
@pytest.mark.parametrize("engine", ENGINES)
def test_teacher_forced_blocks_against_the_reference_goldens(golden, tiny_models, engine, tag):
    """The golden `<tag>.*.blockwise.plain` was made by the reference with blocks [16, 8, 8].  ONE call of S = 8 carries, for every golden
    utterance, block 1 (start 16) and block 2 (start 24): items = [utterances at 16 | utterances at 24].  Each item's prefix is the golden's
    own latents before its start (zeros after), its noise the golden's blk_x1 / blk_x2.  fp32 engine: LAT_TOL.  bf16 engine: 1.5 x the RMS
    distance between the bf16 and the fp32 golden on that slice (the suite's budget rule, from the fixtures)."""
    g, m = golden, tiny_models[engine]
    gold, gold16 = g[f"{tag}.f32.blockwise.plain"], g[f"{tag}.bf16.blockwise.plain"]
    n = gold.shape[0]
    starts = [16] * n + [24] * n
    ids = torch.cat([g[f"{tag}.ids"]] * 2, 0)
    tm = torch.cat([g[f"{tag}.tmask"].bool()] * 2, 0)
    spk = torch.cat([g[f"{tag}.spk"]] * 2, 0)
    sm = torch.cat([g[f"{tag}.smask"].bool()] * 2, 0)
    prefix = torch.zeros((2 * n, 24, 80))
    for i, s in enumerate(starts):
        prefix[i, :s] = gold[i % n, :s]
    x0 = torch.cat([g[f"{tag}.blk_x1"], g[f"{tag}.blk_x2"]], 0)
    m.get_kv_cache_text(ids, tm)
    m.get_kv_cache_speaker(spk.to(m.dtype), sm)
    m.get_kv_cache_latent(prefix)
    arr, temb, _keep = inf.build_sampler_items(m, [dict(SAMPLER_CASES["cfg_default"], rng_seed=0)] * (2 * n))
    out = inf.run_euler_items(m, x0.to(DEV), arr, 6, temb, start_pos=starts, use_latent=True)
    for i, s in enumerate(starts):
        want = gold[i % n, s:s + 8]
        e = rms(out[i], want)
        bound = LAT_TOL if engine == "f32" else 1.5 * rms(gold16[i % n, s:s + 8], want)
        print(f"teacher-forced {tag} {engine}: item {i} (utterance {i % n}, start {s}) rms {e:.3e} bound {bound:.3e}")
        assert e < bound, (i, s, e, bound)


# ------------------------------------------------------------------------------------------------ 4. StreamBatcher end to end
def _stream_requests(g):
    """Three streams: two voices plus none, different guidance scales inside one CFG window, blocks [8, 8, 8], fixed noise."""
    gen = torch.Generator().manual_seed(21)
    base = dict(SAMPLER_CASES["cfg_default"])
    voices = {"a": (g["tinyb2.spk"][0:1], g["tinyb2.smask"].bool()[0:1]), "b": (g["tinyb2.spk"][1:2], g["tinyb2.smask"].bool()[1:2])}
    reqs = []
    for i, (voice, over) in enumerate((("a", {}), ("b", dict(cfg_scale_text=2.0, cfg_scale_speaker=5.0)), (None, dict(cfg_scale_text=4.0)))):
        row = i % 2
        reqs.append(dict(text_input_ids=g["tinyb2.ids"][row:row + 1], text_mask=g["tinyb2.tmask"].bool()[row:row + 1],
                         item_params=dict(base, **over), block_sizes=[8, 8, 8], rng_seed=i, speaker_voice=voice,
                         x_inits=[torch.randn((1, 8, 80), generator=gen) for _ in range(3)]))
    return voices, reqs


def _alone(m, voices, r):
    """The same stream alone through the existing blockwise sampler."""
    if r["speaker_voice"] is None:
        spk, sm = torch.zeros((1, 4, 80)), torch.zeros((1, 4), dtype=torch.bool)
    else:
        spk, sm = voices[r["speaker_voice"]]
    return IB.sample_blockwise_euler_cfg_independent_guidances(m, spk.to(m.dtype), sm, r["text_input_ids"], r["text_mask"], rng_seed=r["rng_seed"],
                                                               block_sizes=r["block_sizes"], x_inits=r["x_inits"], **r["item_params"])


def test_stream_batcher_end_to_end(golden, tiny_models):
    """Stream 2 is opened after stream 0's first block, so the calls carry items at different positions (and, in the first call, fewer
    items).  Every stream's latents against the same stream run alone through `sample_blockwise_stream` with the same noise: fp32 engine,
    LAT_TOL (the batch shape changes the GEMM plans, so no bit equality is claimed).  Then `step_audio`: the concatenated chunks of every
    stream equal `ae_decode` of its final latent, as tests/test_gpu_engine.py::test_blockwise_streaming_api asserts for one stream."""
    g, m = golden, tiny_models["f32"]
    voices, reqs = _stream_requests(g)
    want = [_alone(m, voices, r) for r in reqs]
    sb = SB.StreamBatcher(m, None, None, voices=voices, max_batch=8)
    sid = [sb.open(**reqs[0]), sb.open(**reqs[1])]
    got = {}
    seen_positions = []

    def take(out):
        seen_positions.append(sorted(p for _, p, _ in out))
        for i, p, blk in out:
            got.setdefault(i, []).append((p, blk.clone()))

    take(sb.step())
    sid.append(sb.open(**reqs[2]))
    while sb.open_ids:
        take(sb.step())
    assert seen_positions == [[0, 0], [0, 8, 8], [8, 16, 16], [16]]
    assert sb.step() == []
    for k, i in enumerate(sid):
        assert [p for p, _ in got[i]] == [0, 8, 16]
        lat = torch.cat([b for _, b in got[i]], dim=1)
        e = rms(lat, want[k])
        print(f"StreamBatcher stream {k}: rms vs the stream alone {e:.3e} (bound {LAT_TOL:.1e}, latent rms {U.rms(want[k]):.3f})")
        assert e < LAT_TOL, (k, e)
    # audio: one DACStream per stream
    dac = E.DAC(TINY_DAC, R.make_dac_weights(TINY_DAC, 0), device=DEV)
    pca = R.make_pca(TINY_DAC, 80, 0)
    st = E.PCAState(pca.pca_components, pca.pca_mean, pca.latent_scale)
    chunks = {}
    for k, chunk in IB.stream_audio_many(m, dac, st, reqs[:2], voices=voices, max_batch=8):
        chunks.setdefault(k, []).append(chunk)
    for k in range(2):
        assert [c.shape[-1] for c in chunks[k]] == [8 * 2048] * 3
        lat = torch.cat([b for _, b in got[sid[k]]], dim=1)
        e = rms(torch.cat(chunks[k], dim=-1), E.ae_decode(dac, st, lat))
        print(f"StreamBatcher stream {k}: audio chunks vs ae_decode of the final latent rms {e:.3e}")
        assert e < 1e-6, (k, e)


# ------------------------------------------------------------------------------------------------ 5. refusals
def test_bad_geometry_is_refused_and_the_context_survives(golden, tiny_models):
    """A position past the RoPE table, 3 B > 96 rows, a null table: each returns an error with a message, nothing is launched, and the
    context still runs case 1 afterwards."""
    g, m = golden, tiny_models["bf16"]
    B, S = 2, 32
    ids, tm, spk, sm, prefix, x, tm3, sm3 = _inputs(B, S, 16)
    kvt, kvs, kvl = _caches(m, ids, tm, spk, sm, prefix)
    t = torch.full((3 * B,), 0.7)
    xx = x.to(m.dtype)
    with pytest.raises(L.EchoHipError, match="rope table"):
        m(xx, t, tm3, sm3, kvt, kvs, start_pos=[0, m.MAX_POS - S + 1], kv_cache_latent=kvl)
    m(xx, t, tm3, sm3, kvt, kvs, start_pos=[0, m.MAX_POS - S], kv_cache_latent=kvl)          # the last legal position
    lib, ctx = m._lib, m._ctx
    temb = torch.zeros((1, TINY.timestep_embed_size), dtype=m.dtype, device=DEV)
    out = torch.empty((3 * B, S, 80), dtype=torch.float32, device=DEV)
    xd = xx.to(DEV).contiguous()
    on = (C.c_int32 * 96)(*([1] * 96))
    # null table
    rc = lib.echo_dit_forward_pos(ctx, xd.data_ptr(), temb.data_ptr(), 1, None, 3 * B, B, S, None, 1, on, on, out.data_ptr(), m._stream())
    assert rc != 0 and b"null position table" in lib.echo_last_error(ctx)
    # 33 items: 99 rows
    pos33 = (C.c_int32 * 33)(*([0] * 33))
    rc = lib.echo_dit_forward_pos(ctx, xd.data_ptr(), temb.data_ptr(), 1, None, 33, 33, S, pos33, 1, on, on, out.data_ptr(), m._stream())
    assert rc != 0 and b"96 rows" in lib.echo_last_error(ctx)
    # the sampler entry point: the same three
    arr, temb6, _keep = inf.build_sampler_items(m, [dict(SAMPLER_CASES["cfg_default"], rng_seed=0)] * B)
    with pytest.raises(L.EchoHipError, match="rope table"):
        inf.run_euler_items(m, x[:B].to(DEV), arr, 6, temb6, start_pos=[m.MAX_POS, 0], use_latent=True)
    p = L.EchoSamplerParams()
    p.B, p.S, p.num_steps, p.use_latent = B, S, 6, 1
    td = temb6.to(DEV).contiguous()
    p.temb = td.data_ptr()
    x0 = x[:B].to(DEV).contiguous()
    o2 = torch.empty_like(x0)
    rc = lib.echo_sample_euler_items_pos(ctx, C.byref(p), arr, None, x0.data_ptr(), o2.data_ptr(), m._stream())
    assert rc != 0 and b"null position table" in lib.echo_last_error(ctx)
    p.B = 33
    rc = lib.echo_sample_euler_items_pos(ctx, C.byref(p), arr, pos33, x0.data_ptr(), o2.data_ptr(), m._stream())
    assert rc != 0 and b"96 rows" in lib.echo_last_error(ctx)
    torch.cuda.synchronize()
    _uniform_equals_existing(g, m, 13)
