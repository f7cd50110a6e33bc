"""GPU: per-utterance lengths in one forward and one sampler call (echo_dit_forward_len, echo_sample_euler_items_len) and the host paths on
top of them (StreamBatcher(mix_block_sizes=True)).

A call has B items and a row length S; item b owns the first len[b] tokens of its rows, the rest is padding.  What is asserted:
  - full lengths give the bits of the position calls (the length forms of the kernels differ from the others only at padding tokens);
  - valid rows depend on nothing at a padding position - the caller's values there (NaN, 1e30), what an earlier call left in the workspace,
    the other items - bit for bit, since both sides run the same launches on the same geometry; padding rows of the result are exactly 0;
  - an item against the uniform call of its own length: other M, other plans, so the suite's tolerances, not equality.

Which attention kernel runs: the switch ECHO_ATTN is read once per process, at the first launch; this module runs under the default, so the
bf16 engine's joint attention is attn5_qlen_kernel (the length form of attn5_kernel) with attn_redo_kernel behind it.  attn_qlen_kernel (the
form behind ECHO_ATTN=1) runs the padding, stale-workspace and block-skipping tests of this module in a child process of
tests/test_gpu_attention_len.py, which also holds both forms to an fp64 reference at kernel level."""
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


def rms(a, b):
    return float((a.float().cpu() - b.float().cpu()).pow(2).mean().sqrt())


@pytest.fixture(scope="module")
def tiny_models():
    w = R.make_dit_weights(TINY, seed=0)
    return {"f32": E.EchoDiT(TINY, w, dtype=torch.float32, device=DEV),
            "bf16": E.EchoDiT(TINY, {k: v.bfloat16() for k, v in w.items()}, dtype=torch.bfloat16, device=DEV)}


@pytest.fixture(scope="module")
def wide_models():
    w = R.make_dit_weights(WIDE1, seed=0)
    return {"f32": E.EchoDiT(WIDE1, w, dtype=torch.float32, device=DEV),
            "bf16": E.EchoDiT(WIDE1, {k: v.bfloat16() for k, v in w.items()}, dtype=torch.bfloat16, device=DEV)}


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


class Case:
    """One geometry on one model: caches built once, forwards and 6-step sampler calls on them."""

    check_f32 = True

    def __init__(self, m, B, S, positions, P=28):
        self.m, self.B, self.S, self.positions = m, B, S, list(positions)
        self.ids, self.tm, self.spk, self.sm, self.prefix, self.x, self.tm3, self.sm3 = _inputs(B, S, P)
        self.t = torch.full((3 * B,), 0.7)
        base = dict(SAMPLER_CASES["cfg_default"])
        self.items = [dict(base) if b % 2 == 0 else dict(base, cfg_scale_text=2.0, cfg_scale_speaker=5.0) for b in range(B)]
        self.caches()

    def caches(self):
        m = self.m
        self.kvt = m.get_kv_cache_text(self.ids, self.tm)
        self.kvs = m.get_kv_cache_speaker(self.spk.to(m.dtype), self.sm)
        self.kvl = m.get_kv_cache_latent(self.prefix)
        self.arr, self.temb, self._keep = inf.build_sampler_items(m, [dict(it, rng_seed=0) for it in self.items])

    def forward(self, x=None, lengths=None, S=None, positions=None):
        x = self.x if x is None else x
        if S is not None:
            x = x[:, :S]
        return self.m(x.to(self.m.dtype), self.t, self.tm3, self.sm3, self.kvt, self.kvs, start_pos=list(positions or self.positions),
                      kv_cache_latent=self.kvl, lengths=lengths)

    def sample(self, x=None, lengths=None, S=None):
        x0 = (self.x if x is None else x)[:self.B]
        if S is not None:
            x0 = x0[:, :S]
        return inf.run_euler_items(self.m, x0.to(DEV), self.arr, 6, self.temb, start_pos=self.positions, use_latent=True, lengths=lengths)

    def item_rows(self, b):
        return [b, self.B + b, 2 * self.B + b]        # item b's cond / text-uncond / speaker-uncond rows


def _valid(rows, S, lengths, B):
    """(rows, S) bool: token s of row r belongs to item r % B."""
    return torch.tensor([[s < lengths[r % B] for s in range(S)] for r in range(rows)])


def _fill(x, lengths, B, value):
    out = x.clone()
    out[~_valid(x.shape[0], x.shape[1], lengths, B)] = value
    return out


# ------------------------------------------------------------------------------------------------ 1. symbols
def test_entry_points_are_bound():
    lib = L.load_library()
    for name in ("echo_dit_forward_len", "echo_sample_euler_items_len"):
        assert getattr(lib, name).argtypes == L.SIGNATURES[name][1]
    assert lib.echo_abi_version() == 8


# ------------------------------------------------------------------------------------------------ 2. full lengths == the position calls
def _full_lengths_equal_existing(m):
    c = Case(m, 2, 32, [0, 13], P=16)
    a = c.forward()
    b = c.forward(lengths=[32, 32])
    assert float(a.abs().max()) > 0 and bool(torch.isfinite(a).all()) and torch.equal(a, b)
    sa = c.sample()
    sb = c.sample(lengths=[32, 32])
    assert bool(torch.isfinite(sa).all()) and float(sa.abs().max()) > 0 and torch.equal(sa, sb)
    # a null position table: every item at p.start_pos, the bits of the scalar form
    s0 = inf.run_euler_items(m, c.x[:2].to(DEV), c.arr, 6, c.temb, start_pos=13, use_latent=True)
    s1 = inf.run_euler_items(m, c.x[:2].to(DEV), c.arr, 6, c.temb, start_pos=13, use_latent=True, lengths=[32, 32])
    assert torch.equal(s0, s1)
    # the lengths matter at all
    assert not torch.equal(a[:, :31], c.forward(lengths=[31, 32])[:, :31])


@pytest.mark.parametrize("engine", ENGINES)
def test_full_lengths_equal_the_existing_calls(tiny_models, engine):
    """B = 2, S = 32, P = 16, positions [0, 13]: forward(lengths=[32, 32]) and run_euler_items(lengths=[32, 32]) (6 steps, cfg_default and a
    second parameter set) against the same calls without lengths: torch.equal."""
    _full_lengths_equal_existing(tiny_models[engine])


# ------------------------------------------------------------------------------------------------ 3. padding independence, zero padding
def _padding_independence(c, lengths, what=("forward", "sample")):
    B, S = c.B, c.S
    for kind in what:
        run = c.forward if kind == "forward" else c.sample
        rows = 3 * B if kind == "forward" else B
        valid = _valid(rows, S, lengths, B)
        outs = [run(x=_fill(c.x, lengths, B, v), lengths=lengths).cpu() for v in (0.0, float("nan"), 1e30)]
        for o in outs:
            assert bool(torch.isfinite(o).all()), kind
            assert float(o[valid].abs().max()) > 0
            assert bool((o[~valid] == 0).all()), f"{kind}: padding rows of the result are not exactly 0"
        assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2]), f"{kind}: valid rows depend on the caller's padding"
        # teeth: one valid element of item 1 changes item 1's rows only
        x2 = _fill(c.x, lengths, B, 0.0)
        x2[1, 0, 0] += 1.0
        o2 = run(x=x2, lengths=lengths).cpu()
        others = [r for r in range(rows) if r != 1]         # (item 1's other CFG rows of a forward have their own x: they stay too)
        assert not torch.equal(o2[1], outs[0][1]), kind
        assert torch.equal(o2[others], outs[0][others]), f"{kind}: another row moved"


TINY_RAGGED = [
    (40, [40, 8, 33, 17], [0, 5, 16, 27]),       # 32 + 8: tiles and 32-row passes straddle items
    (20, [20, 5, 13, 1], [0, 5, 16, 27]),        # S & 7 != 0, a length of 1
]


@pytest.mark.parametrize("S,lengths,positions", TINY_RAGGED)
@pytest.mark.parametrize("engine", ENGINES)
def test_padding_independence_and_zero_padding(tiny_models, engine, S, lengths, positions):
    """One forward and a 6-step sampler call, with zeros, NaN and 1e30 in the padding of x: the valid rows of all three are torch.equal and
    finite, the padding rows of the result exactly 0; changing one valid element of item 1 changes that row only."""
    _padding_independence(Case(tiny_models[engine], 4, S, positions), lengths)


# ------------------------------------------------------------------------------------------------ 4. stale workspace
def _stale_workspace(c, lengths, what=("forward", "sample")):
    B, S = c.B, c.S
    for kind in what:
        run = c.forward if kind == "forward" else c.sample
        rows = 3 * B if kind == "forward" else B
        valid = _valid(rows, S, lengths, B)
        clean_x = _fill(c.x, lengths, B, 0.0)
        run(x=clean_x)                                              # a clean uniform call of the same geometry
        want = run(x=clean_x, lengths=lengths).cpu()
        dirty = run(x=_fill(c.x, lengths, B, float("inf"))).cpu()     # uniform: +Inf exactly where the next call has padding
        assert not bool(torch.isfinite(dirty[~valid]).all()), kind
        got = run(x=clean_x, lengths=lengths).cpu()
        assert bool(torch.isfinite(got).all()), f"{kind}: something stale reached a valid row"
        assert torch.equal(got, want), f"{kind}: the ragged call depends on what the call before left in the workspace"
        assert bool((got[~valid] == 0).all())


@pytest.mark.parametrize("S,lengths,positions", TINY_RAGGED)
@pytest.mark.parametrize("engine", ENGINES)
def test_stale_workspace_does_not_reach_valid_rows(tiny_models, engine, S, lengths, positions):
    """A uniform call whose x is +Inf at the next call's padding positions leaves non-finite values in every workspace there.  The ragged
    call behind it equals the ragged call behind a clean uniform call: a skipped attention block is written, not left as it was."""
    _stale_workspace(Case(tiny_models[engine], 4, S, positions), lengths)


# ------------------------------------------------------------------------------------------------ 5. against the uniform call of the item's length
def _against_uniform(c32, c16, lengths, what=("forward", "sample")):
    """c32 / c16: the same Case on the fp32 and the bf16 engine.  fp32: RMS over the item's rows below LAT_TOL.  bf16, items of at least 8
    tokens: rms(ragged_bf16 - uniform_fp32) < 1.5 x rms(uniform_bf16 - uniform_fp32) on that slice (the suite's budget rule; both uniform
    runs are the existing calls)."""
    B = c32.B
    for kind in what:
        rag = {}
        for tag, c in (("f32", c32), ("bf16", c16)):
            if c is not None:
                rag[tag] = (c.forward if kind == "forward" else c.sample)(x=_fill(c.x, lengths, B, 0.0), lengths=lengths).cpu()
        uni = {}
        for n in sorted(set(lengths)):
            for tag, c in (("f32", c32), ("bf16", c16)):
                if c is not None:
                    uni[tag, n] = (c.forward if kind == "forward" else c.sample)(S=n).cpu()
        for b, n in enumerate(lengths):
            rows = c32.item_rows(b) if kind == "forward" else [b]
            want = uni["f32", n][rows]
            if "f32" in rag and c32.check_f32:
                e = rms(rag["f32"][rows][:, :n], want)
                print(f"{kind} S={c32.S} item {b} len {n}: fp32 ragged vs uniform rms {e:.3e} (bound {LAT_TOL:.1e})")
                assert e < LAT_TOL, (kind, b, n, e)
            if "bf16" in rag and n >= 8:
                e = rms(rag["bf16"][rows][:, :n], want)
                budget = 1.5 * rms(uni["bf16", n][rows], want)
                print(f"{kind} S={c32.S} item {b} len {n}: bf16 ragged vs fp32 uniform rms {e:.3e} (bound {budget:.3e})")
                assert e < budget, (kind, b, n, e, budget)
        if B < 3:
            continue
        # teeth: item 1's ragged rows are not within the bound of item 2's uniform rows
        n = min(lengths[1], lengths[2])
        r1, r2 = (c32.item_rows(1), c32.item_rows(2)) if kind == "forward" else ([1], [2])
        other = uni["f32", lengths[2]][r2][:, :n]
        if "f32" in rag and c32.check_f32:
            assert rms(rag["f32"][r1][:, :n], other) > LAT_TOL
        if "bf16" in rag and lengths[1] >= 8 and lengths[2] >= 8:
            assert rms(rag["bf16"][r1][:, :n], other) > 1.5 * rms(uni["bf16", lengths[2]][r2][:, :n], other)


def _pair(models, B, S, positions, check_f32=True):
    c32, c16 = Case(models["f32"], B, S, positions), Case(models["bf16"], B, S, positions)
    c32.check_f32 = check_f32
    return c32, c16


def test_each_item_against_the_uniform_call_of_its_own_length(tiny_models):
    """B = 4, S = 40, lengths [40, 8, 33, 17]: item b against forward(start_pos=[...]) / the sampler call with S = len[b] on the same caches.
    Measured: fp32 about 1e-6 and below."""
    _against_uniform(*_pair(tiny_models, 4, 40, [0, 5, 16, 27]), [40, 8, 33, 17])


# ------------------------------------------------------------------------------------------------ 6. block skipping, tile-count classes
@pytest.mark.parametrize("lengths", [[300, 100, 128, 129, 257], [256, 40, 170, 230, 64]])
def test_attention_block_skipping_and_tile_classes(tiny_models, lengths):
    """Tiny, one forward, S = 300, B = 5: M = 4500, 15 rows x 2 heads x 3 blocks of 128 queries are 90 workgroups, one round, so the launcher
    takes 128-query blocks (attn5_qlen_kernel's one-stream body; see the module docstring for the kernel).  The lengths put the block
    boundary at, before and after the row's end (128, 129, 257, 100, 256) and walk the self key counts over the total_tiles % 3 classes next
    to 24 text and 16 speaker keys.  Per item: padding independence (test 3), the bounds of test 5 against its uniform call, and three
    launches bit-identical (the look-ahead-read bug class)."""
    positions = [0, 5, 16, 27, 12]
    c32, c16 = _pair(tiny_models, 5, 300, positions)
    _padding_independence(c16, lengths, what=("forward",))
    _padding_independence(c32, lengths, what=("forward",))
    _against_uniform(c32, c16, lengths, what=("forward",))
    # the skipped blocks are WRITTEN: +Inf left in the workspace at exactly those blocks by a uniform call does not reach a valid row
    _stale_workspace(c16, lengths, what=("forward",))
    x = _fill(c16.x, lengths, 5, 0.0)
    a = c16.forward(x=x, lengths=lengths)
    for _ in range(2):
        assert torch.equal(a, c16.forward(x=x, lengths=lengths))


def test_skipped_256_query_blocks_and_short_last_block(tiny_models):
    """Tiny bf16, one forward, S = 1100, B = 8: 24 rows x 2 heads x 9 blocks of 128 queries are 432 workgroups, more than one round, so the
    launcher takes 256-query blocks: four of them and the short last block [1024, 1100) (76 queries: the one-stream body).  The lengths
    end rows at, before and after block boundaries, so whole 256-query blocks and the short block are skipped, straddled and full.
    Padding independence (NaN / 1e30 in the caller's padding, zero result padding, teeth) and the stale +Inf workspace.  (B = 8: the
    largest batch whose items all keep a text key in `_inputs`.)"""
    lengths = [1100, 100, 256, 257, 1024, 1025, 600, 513]
    c = Case(tiny_models["bf16"], 8, 1100, [0, 5, 16, 27, 12, 3, 9, 20])
    _padding_independence(c, lengths, what=("forward",))
    _stale_workspace(c, lengths, what=("forward",))


# ------------------------------------------------------------------------------------------------ 7. ping-pong path
@pytest.mark.parametrize("S,B,lengths,positions", [
    (96, 2, [96, 50], [27, 5]),                               # M = 576: gemm_pp_kernel
    (40, 5, [40, 8, 33, 17, 24], [0, 5, 16, 27, 12]),
])
def test_wide_pingpong_path(wide_models, S, B, lengths, positions):
    """WIDE1 bf16 (the ping-pong kernel's fused QKV tail in front of the attention): tests 3 and 5.  The fp32 WIDE1 engine supplies the
    reference of the bf16 budget rule; its own ragged run is held to LAT_TOL as well."""
    c32, c16 = _pair(wide_models, B, S, positions)
    _padding_independence(c16, lengths)
    _against_uniform(c32, c16, lengths)          # (two items: the bounds without the teeth, which need a third)


# ------------------------------------------------------------------------------------------------ 8. StreamBatcher(mix_block_sizes=True)
def _stream_requests(g):
    gen = torch.Generator().manual_seed(21)
    base = dict(SAMPLER_CASES["cfg_default"])
    voices = {"a": (g["tinyb2.spk"][0:1], g["tinyb2.smask"].bool()[0:1]), "b": (g["tinyb2.spk"][1:2], g["tinyb2.smask"].bool()[1:2])}
    reqs = []
    for i, (voice, over, blocks) in enumerate((("a", {}, [8, 16, 16]), ("b", dict(cfg_scale_text=2.0, cfg_scale_speaker=5.0), [16, 16]),
                                               (None, dict(cfg_scale_text=4.0), [8, 8, 24]))):
        row = i % 2
        reqs.append(dict(text_input_ids=g["tinyb2.ids"][row:row + 1], text_mask=g["tinyb2.tmask"].bool()[row:row + 1],
                         item_params=dict(base, **over), block_sizes=blocks, rng_seed=i, speaker_voice=voice,
                         x_inits=[torch.randn((1, n, 80), generator=gen) for n in blocks]))
    return voices, reqs


def _alone(m, voices, r):
    if r["speaker_voice"] is None:
        spk, sm = torch.zeros((1, 4, 80)), torch.zeros((1, 4), dtype=torch.bool)
    else:
        spk, sm = voices[r["speaker_voice"]]
    return IB.sample_blockwise_euler_cfg_independent_guidances(m, spk.to(m.dtype), sm, r["text_input_ids"], r["text_mask"], rng_seed=r["rng_seed"],
                                                               block_sizes=r["block_sizes"], x_inits=r["x_inits"], **r["item_params"])


def _drive(sb, reqs, audio=False):
    """Streams opened one step apart; returns ({request index: [(start, block)]}, {request index: [chunk]}, calls)."""
    got, sid = {}, {}
    k = 0
    while k < len(reqs) or sb.open_ids:
        if k < len(reqs):
            sid[sb.open(**reqs[k])] = k
            k += 1
        if audio:
            for i, chunk in sb.step_audio():
                got.setdefault(sid[i], []).append(chunk)
        else:
            for i, p, blk in sb.step():
                got.setdefault(sid[i], []).append((p, blk.clone()))
    return got, sb.stats["calls"]


def test_stream_batcher_mixed_block_sizes_end_to_end(golden, tiny_models):
    """Three streams with block schedules [8, 16, 16], [16, 16], [8, 8, 24], opened one step apart, 6 steps, fp32 engine.  Each stream's latents
    against the same stream alone through the existing blockwise sampler (LAT_TOL: other batch shapes, other plans); step_audio's chunks
    against ae_decode of the final latent (1e-6, the bound of test_stream_batcher_end_to_end); fewer sampler calls than without mixing."""
    g, m = golden, tiny_models["f32"]
    voices, reqs = _stream_requests(g)
    want = [_alone(m, voices, r) for r in reqs]
    mixed, calls_mixed = _drive(SB.StreamBatcher(m, None, None, voices=voices, max_batch=8, mix_block_sizes=True), reqs)
    plain, calls_plain = _drive(SB.StreamBatcher(m, None, None, voices=voices, max_batch=8), reqs)
    print(f"sampler calls: {calls_mixed} mixed, {calls_plain} grouped by block size")
    assert calls_mixed < calls_plain
    for k, r in enumerate(reqs):
        for got in (mixed, plain):
            assert [b.shape[1] for _, b in got[k]] == r["block_sizes"]
            assert [p for p, _ in got[k]] == [sum(r["block_sizes"][:i]) for i in range(len(r["block_sizes"]))]
        lat = torch.cat([b for _, b in mixed[k]], dim=1)
        e = rms(lat, want[k])
        print(f"mixed StreamBatcher stream {k}: rms vs the stream alone {e:.3e} (bound {LAT_TOL:.1e}, latent rms {U.rms(want[k]):.3f})")
        assert e < LAT_TOL, (k, e)
    dac = E.DAC(TINY_DAC, R.make_dac_weights(TINY_DAC, 0), device=DEV)
    pca = R.make_pca(TINY_DAC, 80, 0)
    st = E.PCAState(pca.pca_components, pca.pca_mean, pca.latent_scale)
    chunks, _ = _drive(SB.StreamBatcher(m, dac, st, voices=voices, max_batch=8, mix_block_sizes=True), reqs, audio=True)
    for k, r in enumerate(reqs):
        assert [c.shape[-1] for c in chunks[k]] == [n * 2048 for n in r["block_sizes"]]
        lat = torch.cat([b for _, b in mixed[k]], dim=1)
        e = rms(torch.cat(chunks[k], dim=-1), E.ae_decode(dac, st, lat))
        print(f"mixed StreamBatcher stream {k}: audio chunks vs ae_decode of the final latent rms {e:.3e}")
        assert e < 1e-6, (k, e)


# ------------------------------------------------------------------------------------------------ 9. refusals
def test_bad_length_tables_are_refused_and_the_context_survives(tiny_models):
    """A length of 0, a length above S, start + length beyond the RoPE table: each an EchoHipError with the reason from the host check, and
    each a non-zero status with the engine's message through the C ABI; nothing is launched and the model then runs test 2's call."""
    m = tiny_models["bf16"]
    c = Case(m, 2, 32, [0, 13], P=16)
    with pytest.raises(L.EchoHipError, match="below 1"):
        c.forward(lengths=[32, 0])
    with pytest.raises(L.EchoHipError, match="above S"):
        c.forward(lengths=[33, 32])
    with pytest.raises(L.EchoHipError, match="rope table"):
        c.forward(lengths=[32, 32], positions=[0, m.MAX_POS - 31])
    c.forward(lengths=[32, 31], positions=[0, m.MAX_POS - 31])             # start + length fits: legal although start + S does not
    with pytest.raises(L.EchoHipError, match="below 1"):
        c.sample(lengths=[0, 32])
    lib, ctx = m._lib, m._ctx
    temb = torch.zeros((1, TINY.timestep_embed_size), dtype=m.dtype, device=DEV)
    out = torch.empty((6, 32, 80), dtype=torch.float32, device=DEV)
    xd = c.x.to(DEV, m.dtype).contiguous()
    on = (C.c_int32 * 96)(*([1] * 96))

    def fwd(pos, ln):
        return lib.echo_dit_forward_len(ctx, xd.data_ptr(), temb.data_ptr(), 1, None, 6, 2, 32, None if pos is None else (C.c_int32 * 2)(*pos),
                                        None if ln is None else (C.c_int32 * 2)(*ln), 1, on, on, out.data_ptr(), m._stream())

    for pos, ln, msg in ((None, None, b"null length table"), (None, [32, 0], b"a length is below 1"), ([0, 13], [33, 32], b"a length is above S"),
                         ([0, m.MAX_POS - 31], [32, 32], b"rope table")):
        assert fwd(pos, ln) != 0 and msg in lib.echo_last_error(ctx), msg
    p = L.EchoSamplerParams()
    p.B, p.S, p.num_steps, p.use_latent = 2, 32, 6, 1
    td = c.temb.to(DEV).contiguous()
    p.temb = td.data_ptr()
    x0 = c.x[:2].to(DEV).contiguous()
    o2 = torch.empty_like(x0)
    for pos, ln, msg in ((None, None, b"null length table"), (None, [32, 0], b"a length is below 1"), ([0, 13], [33, 32], b"a length is above S"),
                         ([0, m.MAX_POS - 31], [32, 32], b"rope table")):
        rc = lib.echo_sample_euler_items_len(ctx, C.byref(p), c.arr, None if pos is None else (C.c_int32 * 2)(*pos),
                                             None if ln is None else (C.c_int32 * 2)(*ln), x0.data_ptr(), o2.data_ptr(), m._stream())
        assert rc != 0 and msg in lib.echo_last_error(ctx), msg
    torch.cuda.synchronize()
    _full_lengths_equal_existing(m)


# ------------------------------------------------------------------------------------------------ 10. fp8
def test_fp8_engine_refuses_length_tables():
    """The fp8 engine (EchoDiT(fp8=True)) is not supported: its attention writes e4m3 bytes (O8) and that output has no length form.  It
    refuses a length table up front with the reason, in both calls, and goes on serving calls without one."""
    w = {k: v.bfloat16() for k, v in R.make_dit_weights(TINY, seed=0).items()}
    m8 = E.EchoDiT(TINY, w, dtype=torch.bfloat16, device=DEV, fp8=True)
    c = Case(m8, 2, 32, [0, 13], P=16)
    with pytest.raises(L.EchoHipError, match="not supported by the fp8 engine"):
        c.forward(lengths=[32, 20])
    with pytest.raises(L.EchoHipError, match="not supported by the fp8 engine"):
        c.sample(lengths=[32, 20])
    assert bool(torch.isfinite(c.forward()).all()) and bool(torch.isfinite(c.sample()).all())


# ------------------------------------------------------------------------------------------------ 11. biased caches
def test_caches_with_a_key_bias_are_refused_up_front(tiny_models):
    """A text mask that is not a prefix gives the cache a per-key bias and the joint attention its biased kernel, which has no length form:
    a length table is refused before anything is queued, with the reason; the same caches go on serving calls without one."""
    m = tiny_models["bf16"]
    c = Case(m, 2, 32, [0, 13], P=16)
    c.tm[0, 3] = False                              # a hole: not a prefix
    c.tm3 = torch.cat([c.tm, torch.zeros_like(c.tm), c.tm], 0)
    c.caches()
    with pytest.raises(L.EchoHipError, match="not a prefix"):
        c.forward(lengths=[32, 20])
    with pytest.raises(L.EchoHipError, match="not a prefix"):
        c.sample(lengths=[32, 20])
    assert bool(torch.isfinite(c.forward()).all()) and bool(torch.isfinite(c.sample()).all())


# ------------------------------------------------------------------------------------------------ 12. the host's list forms
def test_sample_euler_items_with_a_list_of_lengths(golden, tiny_models):
    """sample_euler_items(sequence_length=[32, 20, 9]) returns one (len[b], latent) tensor per item, equal to run_euler_items(lengths=) on the
    noise each item draws alone ((1, len[b], latent) from its own seed) placed in a zero tensor; a numpy integer is an int."""
    import numpy as np
    g, m = golden, tiny_models["f32"]
    n = [32, 20, 9]
    ids = torch.cat([g["tinyb2.ids"], g["tinyb2.ids"][:1]], 0)
    tm = torch.cat([g["tinyb2.tmask"].bool(), g["tinyb2.tmask"].bool()[:1]], 0)
    spk = torch.cat([g["tinyb2.spk"], g["tinyb2.spk"][:1]], 0)
    sm = torch.cat([g["tinyb2.smask"].bool(), g["tinyb2.smask"].bool()[:1]], 0)
    items = [dict(SAMPLER_CASES["cfg_default"], rng_seed=3 + b, cfg_scale_text=3.0 - 0.5 * b) for b in range(3)]
    got = inf.sample_euler_items(m, spk, sm, ids, tm, items, sequence_length=n)
    assert isinstance(got, list) and [tuple(x.shape) for x in got] == [(k, 80) for k in n]
    x0 = torch.zeros((3, 32, 80), device=DEV)
    for b in range(3):
        x0[b, :n[b]] = torch.randn((1, n[b], 80), device=DEV, dtype=torch.float32, generator=torch.Generator(device=DEV).manual_seed(3 + b))[0]
    arr, temb, _keep = inf.build_sampler_items(m, items)
    want = inf.run_euler_items(m, x0, arr, 6, temb, lengths=n)
    for b in range(3):
        assert bool(torch.isfinite(got[b]).all()) and torch.equal(got[b], want[b, :n[b]])
        assert bool((want[b, n[b]:] == 0).all())
    uni = inf.sample_euler_items(m, spk, sm, ids, tm, items, sequence_length=np.int64(32))
    assert tuple(uni.shape) == (3, 32, 80) and torch.equal(uni, inf.sample_euler_items(m, spk, sm, ids, tm, items, sequence_length=32))
    e = rms(got[0], uni[0])                          # item 0 has the call's length and its own noise: the uniform call's row up to the plans
    print(f"sample_euler_items list form, item 0 against the uniform call: rms {e:.3e} (bound {LAT_TOL:.1e})")
    assert e < LAT_TOL


def test_synthesize_many_mix_lengths_equals_the_jobs_run_alone(golden, tiny_models):
    """Three jobs with sequence lengths 32 / 24 / 16 and one num_steps: ONE sampler call with mix_lengths=True (three without), each job's
    audio against the job alone through `synthesize`: same shape, RMS <= 1e-4 (WAV_TOL of tests/test_gpu_sampler_items.py)."""
    from echo_tts_amd import handler as H
    m = tiny_models["f32"]
    dac = E.DAC(TINY_DAC, R.make_dac_weights(TINY_DAC, 0), device=DEV)
    pca = R.make_pca(TINY_DAC, 80, 0)
    st = E.PCAState(pca.pca_components, pca.pca_mean, pca.latent_scale)
    voices = {"alice": (golden["tiny.spk"], golden["tiny.smask"].bool())}
    jobs = [{"text": "The shortest of the three.", "speaker_voice": "alice", "parameters": dict(SAMPLER_CASES["cfg_default"], sequence_length=16, seed=5)},
            {"text": "A second request, the longest one.", "speaker_voice": "alice", "parameters": dict(SAMPLER_CASES["cfg_default"], sequence_length=32, seed=7)},
            {"text": "No voice, in between.", "parameters": dict(SAMPLER_CASES["cfg_default"], cfg_scale_text=2.0, sequence_length=24, seed=3)}]
    _, calls = H.plan_mixed_batches(jobs, 24, mix_lengths=True)
    assert len(calls) == 1 and calls[0]["lengths"] == [32, 24, 16] and len(H.plan_mixed_batches(jobs, 24)[1]) == 3
    got = H.synthesize_many(jobs, m, dac, st, voices=voices, mix_lengths=True)
    alone = [voices["alice"], voices["alice"], (None, None)]
    for j in range(3):
        assert "error" not in got[j], got[j].get("traceback")
        want = H.synthesize(jobs[j], m, dac, st, speaker_latent=alone[j][0], speaker_mask=alone[j][1])
        assert "error" not in want, want.get("traceback")
        a, b = want["audio"].float().cpu(), got[j]["audio"].float().cpu()
        assert a.shape == b.shape, (j, a.shape, b.shape)
        print(f"synthesize_many(mix_lengths) job {j}: rms vs alone {rms(a, b):.3e}")
        assert rms(a, b) <= 1e-4, (j, rms(a, b))
