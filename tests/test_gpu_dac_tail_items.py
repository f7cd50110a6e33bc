"""Batched streaming DAC decode: `echo_dac_decode_tail_items`, `DAC.decode_latent_tails`, `DACStream.push_many`,
`StreamBatcher(batch_decode=True)`.

Numerics contract.  fp32: an item of a batched call agrees with its own `echo_dac_decode_tail` call up to the fp32 summation order of the
row-wise GEMMs (other M, other tile plans): the bound of test_dac_decode_batch_equals_single_decodes, 3e-5 x rms + 1e-7.  bf16: the fixed plan
rule keeps one summation chain per output, but equal bits are NOT reached for ragged groups: `frun` picks the tile from the launch's M, and the
192- / 96-column tiles carry the branch-free conv tail whose Snake uses v_sin_f32 where the generic tail of the 128-column tiles calls sinf()
(gemm_nt_kernel, NTAIL 2..5 against NTAIL 1) - a slot of W frames and a single call of fewer frames can sit on different sides of that rule, and
the fp32 PCA inverse takes M-dependent plans.  The bf16 comparison is therefore held to the bound test_bf16_decode_batch uses:
0.5 x the reference's bf16-vs-fp32 floor x the item's RMS.  Same geometry gives the same plans: there, bits are equal (the isolation test)."""
from __future__ import annotations

import ctypes as C
import os

import pytest
import torch
from safetensors.torch import load_file

pytestmark = pytest.mark.gpu

from tests.golden_defs import GOLD, SAMPLER_CASES, TINY, TINY_DAC, R  # noqa: E402
from tests import gpu_util as U  # noqa: E402

import echo_tts_amd as E  # noqa: E402
from echo_tts_amd import _lib as L  # noqa: E402
from echo_tts_amd.autoencoder import DACStream  # noqa: E402

DEV = U.DEV
HOP = 2048
# (T, first_frame, drop): the shortest tail, a tail of one frame, a start at 0 next to starts > 0, ragged histories.  The issue behind this change
# lists item 2 as (40, 28, 12); that is drop_frames = T - first_frame, which the same issue has the call refuse (no sample would be left), so the
# item starts one frame earlier here and keeps one frame behind its 12 dropped ones.
GEOM = ((8, 0, 0), (24, 4, 4), (40, 27, 12), (33, 32, 0))


def rms(a, b=None):
    d = a.float().cpu() if b is None else a.float().cpu() - b.float().cpu()
    return float(d.pow(2).mean().sqrt())


def _is_bf16_valued(x: torch.Tensor) -> bool:
    return x.dtype == torch.float32 and torch.equal(x, x.bfloat16().float())


@pytest.fixture(scope="module")
def gold():
    g = {}
    for fn in ("dac_tiny.safetensors", "dac_full.safetensors", "dac_bf16.safetensors"):
        g.update(load_file(os.path.join(GOLD, fn)))
    return g


@pytest.fixture(scope="module")
def dacs():
    """One engine per (config, dtype), shared by the tests of this module."""
    out = {}
    for size, cfg in (("tiny", TINY_DAC), ("full", R.DacConfig())):
        w = R.make_dac_weights(cfg, 0)
        pca = R.make_pca(cfg, 80, 0)
        out[size] = dict(cfg=cfg, w=w, st=E.PCAState(pca.pca_components, pca.pca_mean, pca.latent_scale),
                         bf16=E.DAC(cfg, w, device=DEV, dtype=torch.bfloat16), f32=E.DAC(cfg, w, device=DEV))
        for k in ("bf16", "f32"):
            out[size][k].set_pca(out[size]["st"])
    return out


def _floor_rel(gold, size):
    tag = "dac_tiny" if size == "tiny" else "dac_full"
    return rms(gold[f"{tag}.bf16.wav"].float(), gold[f"{tag}.wav"]) / rms(gold[f"{tag}.wav"])


def _latents(seed=21, scale1=3.0):
    gen = torch.Generator().manual_seed(seed)
    lats = [torch.randn((T, 80), generator=gen) for T, _, _ in GEOM]
    lats[1] = lats[1] * scale1                                 # an item of another scale: a leak between items would show
    return [x.to(DEV) for x in lats]


def _singles(dac, lats, geom=GEOM):
    return [dac.decode_latent_tail(lat, f0)[drop * HOP:] for lat, (_, f0, drop) in zip(lats, geom)]


def _within(dtype, floor_rel, got, one):
    e, r = rms(got, one), rms(one)
    bound = 3e-5 * r + 1e-7 if dtype == "f32" else 0.5 * floor_rel * r
    return e, bound


def _raw(dac, items):
    """The C call itself: items = [(latent tensor, T, first_frame, drop, wav_out tensor)].  Returns (status, message)."""
    n = len(items)
    tab = (L.EchoDacTailItem * max(n, 1))()
    for i, (lat, T, f0, drop, out) in enumerate(items):
        tab[i].latent, tab[i].T, tab[i].first_frame, tab[i].drop_frames, tab[i].wav_out = lat.data_ptr(), T, f0, drop, out.data_ptr()
    rc = dac._lib.echo_dac_decode_tail_items(dac._ctx, tab, n, getattr(dac, "_latent_scale", 1.0), dac._stream())
    torch.cuda.synchronize()
    return rc, dac._lib.echo_last_error(dac._ctx).decode()


# ------------------------------------------------------------------ 1. symbol
def test_library_exports_the_tail_items_call():
    lib = L.load_library()
    assert hasattr(lib, "echo_dac_decode_tail_items")
    assert lib.echo_abi_version() == 8 and L.ABI_VERSION == 8


# ------------------------------------------------------------------ 2. equals the single calls
@pytest.mark.parametrize("size", ["tiny", "full"])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_items_equal_their_single_tail_calls(gold, dacs, size, dtype):
    """Every item against `decode_latent_tail` plus slicing.  Item 3 keeps the samples right behind first_frame = 32 (nothing dropped): there
    the single call's taps read, in front of its operands, the item's own front rows left in the buffer, and the batched call must place the
    same rows in front of the item's slot at every layer - zeros there differ by 1.2e-2 rms on a 1.4e-2 .. 2.3e-2 signal."""
    dac, fr = dacs[size][dtype], _floor_rel(gold, size)
    lats = _latents()
    got = dac.decode_latent_tails([(lat, f0, drop) for lat, (_, f0, drop) in zip(lats, GEOM)])
    again = dac.decode_latent_tails([(lat, f0, drop) for lat, (_, f0, drop) in zip(lats, GEOM)])
    ones = _singles(dac, lats)
    for i, (g, a, one, (T, f0, drop)) in enumerate(zip(got, again, ones, GEOM)):
        assert g.shape == one.shape == ((T - f0 - drop) * HOP,)
        assert bool(torch.isfinite(g).all()) and torch.equal(g, a)
        if dtype == "bf16":
            assert _is_bf16_valued(g)
        e, bound = _within(dtype, fr, g, one)
        print(f"tail items ({size}, {dtype}) item {i} {(T, f0, drop)}: rms difference to its single call {e:.3e} (item rms {rms(one):.3e}, "
              f"bound {bound:.3e}, bit-equal {torch.equal(g, one)})")
        assert e < bound, (i, e, bound)


# ------------------------------------------------------------------ 3. isolation
@pytest.mark.parametrize("size", ["tiny", "full"])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_an_item_does_not_see_its_neighbours(dacs, size, dtype):
    """Same geometry, same plans: items 1 and 3 must keep their BITS whatever items 0 and 2 hold - any difference is a leak across a slot
    boundary (a tap that read a neighbour's rows, a front that mixed items).  The check can fail: decoded as ONE item, items 0 and 1 do leak."""
    dac = dacs[size][dtype]
    lats = _latents()
    req = lambda ls: [(lat, f0, drop) for lat, (_, f0, drop) in zip(ls, GEOM)]      # noqa: E731
    base = dac.decode_latent_tails(req(lats))
    gen = torch.Generator().manual_seed(77)
    for k, mag in enumerate((1.0, 1e3)):
        other = list(lats)
        other[0] = (mag * torch.randn((GEOM[0][0], 80), generator=gen)).to(DEV)
        other[2] = (mag * torch.randn((GEOM[2][0], 80), generator=gen)).to(DEV)
        got = dac.decode_latent_tails(req(other))
        assert torch.equal(got[1], base[1]) and torch.equal(got[3], base[3]), f"neighbours x {mag:g} changed an item's bits"
        assert bool(torch.isfinite(got[1]).all()) and bool(torch.isfinite(got[3]).all())
        if k == 0:
            assert not torch.equal(got[0], base[0]) and not torch.equal(got[2], base[2])
    # teeth: items 0 and 1 given as one item of 8 + 24 frames; item 1's kept frames 8.. are frames 16.. of the merged item
    merged = dac.decode_latent_tails([(torch.cat([lats[0], lats[1]], 0), 0, 0)] + req(lats)[2:])[0]
    a = GEOM[0][0] + GEOM[1][1] + GEOM[1][2]
    leak = rms(merged[a * HOP:], base[1])
    print(f"tail items ({size}, {dtype}): items 0 and 1 decoded as one item differ from item 1 alone by rms {leak:.3e}")
    assert merged[a * HOP:].shape == base[1].shape and leak > 1e-5


# ------------------------------------------------------------------ 4. the caller's memory
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_callers_memory_is_respected(gold, dacs, dtype):
    """NaN behind row T of every latent allocation (never read), a guard pattern behind every wav_out (never written); the dropped context
    samples land nowhere: wav_out holds exactly the kept samples."""
    dac = dacs["tiny"][dtype]
    lats = _latents()
    ones = dac.decode_latent_tails([(lat, f0, drop) for lat, (_, f0, drop) in zip(lats, GEOM)])      # same geometry: same bits expected
    singles = _singles(dac, lats)
    GUARD, items, outs = 1234.5, [], []
    for lat, (T, f0, drop) in zip(lats, GEOM):
        big = torch.full((T + 9, 80), float("nan"), device=DEV)
        big[:T] = lat
        n = (T - f0 - drop) * HOP
        out = torch.full((n + 4096,), GUARD, device=DEV)
        items.append((big[:T], T, f0, drop, out))
        outs.append((out, n))
    rc, msg = _raw(dac, items)
    assert rc == 0, msg
    for i, ((out, n), one) in enumerate(zip(outs, ones)):
        assert bool((out[n:] == GUARD).all()), f"item {i}: wrote behind its wav_out"
        assert bool(torch.isfinite(out[:n]).all()) and torch.equal(out[:n], one)
        e, bound = _within(dtype, _floor_rel(gold, "tiny"), out[:n], singles[i])      # the single call WITHOUT its first drop * hop samples
        assert e < bound, (i, e, bound)


# ------------------------------------------------------------------ 5. groups
def test_groups_and_nothing_stale_between_geometries(dacs):
    """5 items x 200 frames: 1000 slot frames > 640, so at least two groups.  A call with small tails behind it must equal the same call made
    first in a fresh DAC: nothing the larger geometry left in the shared buffers may reach it."""
    d = dacs["tiny"]
    dac = d["f32"]
    gen = torch.Generator().manual_seed(5)
    longs = [torch.randn((200, 80), generator=gen).to(DEV) for _ in range(5)]
    shorts = [torch.randn((60 + 7 * i, 80), generator=gen).to(DEV) for i in range(5)]
    sreq = [(x, x.shape[0] - 44, 12) for x in shorts]
    got = dac.decode_latent_tails([(x, 0, 0) for x in longs])
    for i, (g, x) in enumerate(zip(got, longs)):
        one = dac.decode_latent_tail(x, 0)
        e = rms(g, one)
        assert g.shape == one.shape and e < 3e-5 * rms(one) + 1e-7, (i, e, rms(one))
    after = dac.decode_latent_tails(sreq)
    fresh_dac = E.DAC(d["cfg"], d["w"], device=DEV)
    fresh_dac.set_pca(d["st"])
    fresh = fresh_dac.decode_latent_tails(sreq)
    for i, (a, f) in enumerate(zip(after, fresh)):
        assert a.shape == (32 * HOP,) and torch.equal(a, f), f"item {i}: the earlier, larger call changed this one"


# ------------------------------------------------------------------ 6. refusals
def test_refusals_name_their_cause_and_leave_the_context_usable(dacs):
    dac = dacs["tiny"]["f32"]
    lat = torch.randn((300, 80), generator=torch.Generator().manual_seed(3)).to(DEV)
    SENT = -7.0
    out = torch.full((16 * HOP,), SENT, device=DEV)
    good = (lat[:16], 16, 4, 4, out)
    cases = [
        ([], "outside 1..32"),
        ([good] * 33, "outside 1..32"),
        ([good, (lat[:16], 16, 16, 0, out)], "first_frame"),
        ([good, (lat[:16], 16, 4, 12, out)], "drop_frames"),
        ([good, (lat[:257], 257, 250, 0, out)], "rope"),      # the tiny DAC's table has 256 positions
    ]
    for items, word in cases:
        rc, msg = _raw(dac, items)
        assert rc != 0 and word in msg, (word, rc, msg)
        assert bool((out == SENT).all()), f"a refused call ({word}) wrote to wav_out"
        rc, msg = _raw(dac, [good])
        assert rc == 0, msg
        want = dac.decode_latent_tail(lat[:16], 4)[4 * HOP:]
        assert rms(out[:8 * HOP], want) < 3e-5 * rms(want) + 1e-7 and bool((out[8 * HOP:] == SENT).all())
        out.fill_(SENT)
    # a context without PCA operands
    d = dacs["tiny"]
    bare = E.DAC(d["cfg"], d["w"], device=DEV)
    rc, msg = _raw(bare, [good])
    assert rc != 0 and "echo_set_pca" in msg and bool((out == SENT).all())


# ------------------------------------------------------------------ 7. DACStream.push_many
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_push_many_equals_whole_decode_and_push_state(gold, dacs, dtype):
    d = dacs["tiny"]
    dac, st, fr = d[dtype], d["st"], _floor_rel(gold, "tiny")
    schedules = ((8, 8, 4, 20), (16, 24), (40,))
    gen = torch.Generator().manual_seed(2)
    lats = [torch.randn((1, 40, 80), generator=gen) for _ in schedules]
    wholes = [E.ae_decode(dac, st, x) for x in lats]
    streams, twins = [DACStream(dac, st) for _ in schedules], [DACStream(dac, st) for _ in schedules]
    parts, pos = [[] for _ in schedules], [0] * len(schedules)
    for rnd in range(max(len(s) for s in schedules)):
        live = [i for i, s in enumerate(schedules) if rnd < len(s)]
        blocks = [lats[i][:, pos[i]:pos[i] + schedules[i][rnd]] for i in live]
        chunks = DACStream.push_many([streams[i] for i in live], blocks)
        for i, blk, ch in zip(live, blocks, chunks):
            assert ch.shape == (1, 1, schedules[i][rnd] * HOP)
            parts[i].append(ch)
            twins[i].push(blk)
            pos[i] += schedules[i][rnd]
            assert streams[i].emitted == twins[i].emitted == pos[i] and torch.equal(streams[i].latents, twins[i].latents)
    for i, whole in enumerate(wholes):
        got = torch.cat(parts[i], dim=-1)
        e = rms(got, whole)
        print(f"push_many ({dtype}) stream {i} {schedules[i]}: rms to the whole-utterance decode {e:.3e} (signal {rms(whole):.3e})")
        assert got.shape == whole.shape
        if dtype == "f32":
            assert e < 1e-6 and e < 1e-4 * rms(whole)
        else:
            assert e < 0.5 * fr * rms(whole) and _is_bf16_valued(got)


def test_push_many_refuses_what_it_cannot_do(dacs):
    d = dacs["tiny"]
    a, b = DACStream(d["f32"], d["st"]), DACStream(d["f32"], d["st"])
    blk = torch.randn((4, 80))
    with pytest.raises(ValueError, match="different DAC"):
        DACStream.push_many([a, DACStream(d["bf16"], d["st"])], [blk, blk])
    with pytest.raises(ValueError, match="32"):
        DACStream.push_many([DACStream(d["f32"], d["st"]) for _ in range(33)], [blk] * 33)
    with pytest.raises(ValueError, match="twice"):
        DACStream.push_many([a, a], [blk, blk])
    with pytest.raises(ValueError, match="empty"):
        DACStream.push_many([a, b], [blk, blk[:0]])
    assert a.latents is None and a.emitted == 0 and b.latents is None      # a refused call moves no state
    assert DACStream.push_many([a, b], [blk, blk])[1].shape == (1, 1, 4 * HOP)


# ------------------------------------------------------------------ 8. StreamBatcher(batch_decode=True)
@pytest.fixture(scope="module")
def tiny_stack(dacs):
    model = E.EchoDiT(TINY, R.make_dit_weights(TINY, seed=0), dtype=torch.float32, device=DEV)
    return model, dacs["tiny"]["f32"], dacs["tiny"]["st"]


def _requests(g):
    """Three streams as in test_stream_batcher_end_to_end (two voices plus none, fixed noise), other block schedules; stream 1 continues 12
    latents that exist already."""
    gen = torch.Generator().manual_seed(21)
    base = dict(SAMPLER_CASES["cfg_default"])
    voices = {"a": (g["tinyb2.spk"][0:1], g["tinyb2.smask"].bool()[0:1]), "b": (g["tinyb2.spk"][1:2], g["tinyb2.smask"].bool()[1:2])}
    reqs = []
    for i, (voice, blocks) in enumerate((("a", (8, 8, 16)), ("b", (8, 16)), (None, (16, 8, 8)))):
        row = i % 2
        reqs.append(dict(text_input_ids=g["tinyb2.ids"][row:row + 1], text_mask=g["tinyb2.tmask"].bool()[row:row + 1],
                         item_params=dict(base), block_sizes=list(blocks), rng_seed=i, speaker_voice=voice,
                         x_inits=[torch.randn((1, b, 80), generator=gen) for b in blocks]))
    reqs[1]["continuation_latent"] = torch.randn((1, 12, 80), generator=gen)
    return voices, reqs


def _run_batcher(stack, g, batch_decode, by_hand=False):
    """Three staggered streams (the third opens after the first step); returns ([(sid, chunk)] in order, the batcher's block latents)."""
    from echo_tts_amd.stream_batch import StreamBatcher
    model, dac, st = stack
    voices, reqs = _requests(g)
    sb = StreamBatcher(model, dac, st, voices=voices, max_batch=8, mix_block_sizes=True, batch_decode=batch_decode)
    out, decs = [], {}
    sb.open(**reqs[0]); sb.open(**reqs[1])
    opened = False
    while sb.open_ids or not opened:
        if by_hand:      # the parent's behaviour, spelled out: one DACStream per stream, driven by push
            for sid, start, block in sb.step():
                if sid not in decs:
                    decs[sid] = DACStream(dac, st)
                    if start > 0:
                        decs[sid].push(reqs[sid]["continuation_latent"][0])
                out.append((sid, decs[sid].push(block[0])))
        else:
            out.extend(sb.step_audio())
        if not opened:
            sb.open(**reqs[2])
            opened = True
    return out


def test_stream_batcher_batch_decode(golden, tiny_stack):
    from echo_tts_amd.stream_batch import stream_audio_many
    g = golden
    off = _run_batcher(tiny_stack, g, False)
    on = _run_batcher(tiny_stack, g, True)
    hand = _run_batcher(tiny_stack, g, False, by_hand=True)
    assert [s for s, _ in off] == [s for s, _ in on] == [s for s, _ in hand] and len({s for s, _ in off}) == 3
    for (sid, a), (_, b), (_, h) in zip(off, on, hand):
        assert torch.equal(a, h), "batch_decode=False must be the per-stream DACStream path, bit for bit"
        assert a.shape == b.shape and bool(torch.isfinite(b).all())
        e = rms(a, b)
        assert e < 3e-5 * rms(a) + 1e-7, (sid, e, rms(a))
    model, dac, st = tiny_stack
    voices, reqs = _requests(g)
    many_off = list(stream_audio_many(model, dac, st, reqs, voices=voices, max_batch=8, mix_block_sizes=True))
    many_on = list(stream_audio_many(model, dac, st, reqs, voices=voices, max_batch=8, mix_block_sizes=True, batch_decode=True))
    assert [i for i, _ in many_off] == [i for i, _ in many_on]
    for (i, a), (_, b) in zip(many_off, many_on):
        assert a.shape == b.shape and rms(a, b) < 3e-5 * rms(a) + 1e-7, i
