"""GPU: the sampler with compacted row sets (echo_sample_euler_items_compact) and the host paths on top of it.

TINY, S = 32, B = 4, at most 6 steps, parameter sets cfg_default / cfg_off / all_options of SAMPLER_CASES.  Iteration i of a compact call
runs the conditional row of every active item and the two un-conditional rows of those that have CFG at their own step i; a finished item
has no rows.  Bit for bit: one group with every item in CFG at the same steps equals the rectangular calls; an item does not depend on the
other items' contents while the row sets stay the same; a stale workspace changes nothing; a finished item's result is final.  Against the
uniform batch-1 call of each item (other M, other plans) the suite's constants of tests/test_gpu_item_steps.py hold: LAT_TOL on the fp32
engine, BUDGET x the uniform bf16 call's own distance on the bf16 engine."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import echo_ref as R  # noqa: E402  (checker only)
from tests import gpu_util as U  # noqa: E402
from tests import test_gpu_item_steps as IS  # noqa: E402  (its Call fixture class and its constants)
from tests.golden_defs import SAMPLER_CASES, TINY, TINY_DAC  # noqa: E402

import echo_tts_amd as E  # noqa: E402
from echo_tts_amd import _lib as L  # noqa: E402
from echo_tts_amd import inference as inf  # noqa: E402
from echo_tts_amd import stream_batch as SB  # noqa: E402

DEV = U.DEV
LAT_TOL, BUDGET, ENGINES, rms = IS.LAT_TOL, IS.BUDGET, IS.ENGINES, IS.rms
B = 4
COUNTS = [6, 2, 6, 4]


@pytest.fixture(scope="module")
def tiny_models():
    return IS._make_models()


def _params(counts):
    return IS._params(counts)       # item b: cfg_default / cfg_off / all_options by b % 3, at counts[b] steps


def _cfg_table(m, items):
    """has_cfg per (item, own step), read from the step tables the engine is given."""
    _arr, _t, keep = inf.build_sampler_items(m, items)
    return [[bool(keep[b][i].has_cfg) for i in range(int(it["num_steps"]))] for b, it in enumerate(items)]


class Call(IS.Call):
    def compact(self, items, counts, *, pos=None, lengths=None, start_pos=0, x=None, item_steps="counts", fill=None, expect_ok=True):
        """echo_sample_euler_items_compact through the C ABI: (latent_out, row-forwards of the call)."""
        m, n = self.m, self.B
        self.caches(items)
        arr, _t, keep = inf.build_sampler_items(m, items)
        N = max(counts)
        td = inf.step_groups_temb(m, counts, N).to(DEV).contiguous()
        p = L.EchoSamplerParams()
        p.B, p.S, p.num_steps, p.start_pos, p.use_latent = n, self.S, N, int(start_pos), 1
        p.temb = td.data_ptr()
        x0 = (self.x if x is None else x).to(DEV, torch.float32).contiguous()
        out = torch.empty_like(x0) if fill is None else torch.full_like(x0, fill)
        tab = (C.c_int32 * n)(*counts) if item_steps == "counts" else item_steps
        rc = m._lib.echo_sample_euler_items_compact(m._ctx, C.byref(p), arr, tab, None if pos is None else (C.c_int32 * n)(*pos),
                                                    None if lengths is None else (C.c_int32 * n)(*lengths), x0.data_ptr(), out.data_ptr(), m._stream())
        torch.cuda.synchronize()
        del keep
        if not expect_ok:
            return rc, out
        assert rc == 0, m._lib.echo_last_error(m._ctx)
        return out.cpu(), m.last_row_forwards()


# ------------------------------------------------------------------------------------------------ 5. one group, all in CFG == rectangular
@pytest.mark.parametrize("engine", ENGINES)
def test_one_group_all_in_cfg_equals_the_rectangular_calls(tiny_models, engine):
    """Four items of cfg_default (other scales per item), 6 steps: CFG at the same steps for all, one group - the 3 B layout while the window
    is open, B rows after it.  torch.equal with echo_sample_euler_items_steps / _len / plain, with and without positions and lengths; NULL
    item_steps means all N."""
    c = Call(tiny_models[engine], B)
    base = SAMPLER_CASES["cfg_default"]
    items = [dict(base, num_steps=6, rng_seed=b, cfg_scale_text=3.0 - 0.5 * b, cfg_scale_speaker=8.0 - b) for b in range(B)]
    for kw in (dict(), dict(pos=[0, 13, 5, 7], lengths=[32, 20, 9, 32]), dict(start_pos=13)):
        want = c.steps(items, [6] * B, **kw)
        got, nrf = c.compact(items, [6] * B, **kw)
        assert bool(torch.isfinite(want).all()) and float(want.abs().max()) > 0
        assert torch.equal(got, want), (engine, kw)
        got2, _ = c.compact(items, [6] * B, item_steps=None, **kw)
        assert torch.equal(got2, want)
        assert nrf == inf.row_forwards(_cfg_table(c.m, items), None, compact=False) == m_rect_count(c, items, [6] * B, **kw)
    assert torch.equal(c.compact(items, [6] * B)[0], c.existing(items))


def m_rect_count(c, items, counts, **kw):
    c.steps(items, counts, **kw)
    return c.m.last_row_forwards()


# ------------------------------------------------------------------------------------------------ mixed windows and counts
def _mixed(c, **kw):
    items = _params(COUNTS)
    got, nrf = c.compact(items, COUNTS, **kw)
    return items, got, nrf


def test_mixed_windows_and_counts_against_uniform_calls(tiny_models):
    """Counts (6, 2, 6, 4), cfg_default / cfg_off / all_options / cfg_default: each item against its uniform batch-1 call at its own count."""
    c32, c16 = Call(tiny_models["f32"], B), Call(tiny_models["bf16"], B)
    items, got32, _ = _mixed(c32)
    _, got16, _ = _mixed(c16)
    assert bool(torch.isfinite(got32).all()) and bool(torch.isfinite(got16).all())
    res = IS._check_against_uniform(c32, c16, items, got32, got16, lambda c, b: IS._uniform_alone(c, items, b), f"compact {tuple(COUNTS)}")
    for b, (e32, e16, own) in enumerate(res):
        assert e32 < LAT_TOL, (b, e32)
        assert e16 < BUDGET * own, (b, e16, own)


@pytest.mark.parametrize("engine", ENGINES)
def test_row_forward_counter(tiny_models, engine):
    """echo_debug_last_row_forwards of the compact call = inference.row_forwards(compact=True) = the sum over the grouped calls (one
    rectangular call per step count), strictly below the rectangular mixed call's count (= row_forwards(compact=False)).  Counts
    (6, 2, 6, 4); the two 6-step items share their CFG window (cfg_default with other scales), as grouping by step count needs for the
    equality: a grouped call is rectangular inside its group.  The 2-step item is cfg_off, the 4-step item all_options."""
    c = Call(tiny_models[engine], B)
    names = ("cfg_default", "cfg_off", "cfg_default", "all_options")
    items = [dict(SAMPLER_CASES[n], num_steps=k, rng_seed=b, cfg_scale_text=3.0 - 0.25 * b) for b, (n, k) in enumerate(zip(names, COUNTS))]
    _, nrf = c.compact(items, COUNTS)
    cfg = _cfg_table(c.m, items)
    assert any(any(row) for row in cfg) and not all(all(row) for row in cfg)
    assert nrf == inf.row_forwards(cfg, COUNTS, compact=True)
    rect = m_rect_count(c, items, COUNTS)
    assert rect == inf.row_forwards(cfg, COUNTS, compact=False)
    grouped = 0
    for n in dict.fromkeys(COUNTS):
        rows = [b for b in range(B) if COUNTS[b] == n]
        c.existing([items[b] for b in rows], rows=rows)
        grouped += c.m.last_row_forwards()
    assert nrf == grouped < rect, (nrf, grouped, rect)
    assert grouped == sum(inf.row_forwards([cfg[b] for b in range(B) if COUNTS[b] == n], None, compact=False) for n in dict.fromkeys(COUNTS))
    assert nrf < rect


# ------------------------------------------------------------------------------------------------ 6. independence of the others' contents
@pytest.mark.parametrize("engine", ENGINES)
def test_an_item_does_not_depend_on_the_other_items_contents(tiny_models, engine):
    """Same parameters (same row sets), item 0 unchanged; the others get another text, voice, prefix and noise: item 0's bits stay, theirs move."""
    m = tiny_models[engine]
    a, b = Call(m, B, seed=11), Call(m, B, seed=12)
    for t in ("ids", "tm", "sm", "spk", "prefix", "x"):
        getattr(b, t)[0] = getattr(a, t)[0]
    kw = dict(pos=[0, 13, 5, 7], lengths=[32, 20, 9, 27])
    _, ga, na = _mixed(a, **kw)
    _, gb, nb = _mixed(b, **kw)
    assert na == nb and float(ga[0].abs().max()) > 0
    assert torch.equal(ga[0], gb[0]), "item 0 changed with the other items' contents"
    for r in range(1, B):
        assert not torch.equal(ga[r], gb[r])


# ------------------------------------------------------------------------------------------------ 7. stale workspace
@pytest.mark.parametrize("engine", ENGINES)
def test_a_stale_workspace_changes_nothing(tiny_models, engine):
    """The same compact call after a clean run and after a rectangular call that left +Inf where the compact call has padding and in rows it
    does not run: the same bits, all finite."""
    c = Call(tiny_models[engine], B)
    kw = dict(pos=[0, 13, 5, 7], lengths=[32, 20, 9, 27])
    _, want, _ = _mixed(c, **kw)
    dirty = c.x.clone()
    for r, n in enumerate(kw["lengths"]):
        dirty[r, n:] = float("inf")
    items = _params([6] * B)
    c.existing(items, x=dirty, pos=kw["pos"])
    _, got, _ = _mixed(c, **kw)
    assert bool(torch.isfinite(got).all()) and torch.equal(got, want)


# ------------------------------------------------------------------------------------------------ a finished item is final
@pytest.mark.parametrize("engine", ENGINES)
def test_a_finished_item_is_final(tiny_models, engine):
    """Item 1 finishes after 2 steps, item 3 after 4.  What the longer items do afterwards (another noise for items 0 and 2: same row sets)
    leaves their latent_out bits alone; padding of the result is 0 and nothing is written behind the items."""
    c = Call(tiny_models[engine], B)
    items, got, _ = _mixed(c, lengths=[32, 20, 32, 27])
    x2 = c.x.clone()
    x2[0] += 1.0
    x2[2] -= 1.0
    got2, _ = c.compact(items, COUNTS, lengths=[32, 20, 32, 27], x=x2)
    assert torch.equal(got[1], got2[1]) and torch.equal(got[3], got2[3])
    assert not torch.equal(got[0], got2[0]) and not torch.equal(got[2], got2[2])
    assert bool((got[1, 20:] == 0).all()) and bool((got[3, 27:] == 0).all())


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals_and_the_context_survives(tiny_models):
    c = Call(tiny_models["bf16"], B)
    items = _params(COUNTS)
    lib, ctx = c.m._lib, c.m._ctx
    for counts, what in (([6, 0, 6, 4], b"below 1"), ([6, 7, 6, 4], b"above")):
        rc, out = c.compact(items, COUNTS, item_steps=(C.c_int32 * B)(*counts), fill=IS.SENTINEL, expect_ok=False)
        assert rc != 0 and what in lib.echo_last_error(ctx)
        assert bool((out == IS.SENTINEL).all()), "a refused call wrote latent_out"
    rc, _ = c.compact(items, COUNTS, pos=[0, 13, -1, 7], expect_ok=False)
    assert rc != 0 and b"negative" in lib.echo_last_error(ctx)
    got, _ = c.compact(items, COUNTS)
    assert bool(torch.isfinite(got).all())


def test_fp8_model_is_refused_before_anything_is_queued():
    w = {k: v.bfloat16() for k, v in R.make_dit_weights(TINY, seed=0).items()}
    m8 = E.EchoDiT(TINY, w, dtype=torch.bfloat16, device=DEV, fp8=True)
    c = Call(m8, 2)
    items = _params([6, 6])
    rc, _ = c.compact(items, [6, 6], expect_ok=False)
    assert rc != 0 and b"fp8 engine" in m8._lib.echo_last_error(m8._ctx)
    arr, temb, _k = inf.build_sampler_items(m8, items)
    with pytest.raises(L.EchoHipError, match="compact_rows"):
        inf.run_euler_items(m8, c.x.to(DEV), arr, 6, temb, compact_rows=True)
    with pytest.raises(L.EchoHipError, match="compact_rows"):
        inf.sample_euler_items(m8, c.spk.bfloat16(), c.sm, c.ids, c.tm, items, sequence_length=32, compact_rows=True)
    with pytest.raises(L.EchoHipError, match="compact_rows"):
        SB.StreamBatcher(m8, None, None, compact_rows=True)


# ------------------------------------------------------------------------------------------------ host paths
def test_sample_euler_items_compact_against_rectangular(tiny_models):
    """inference.sample_euler_items(num_steps=[6, 2, 6, 4], compact_rows=True) against compact_rows=False: fp32 rms < LAT_TOL per item; bf16
    distance to the fp32 rectangular result <= BUDGET x the bf16 rectangular result's own distance to it.  The counter falls."""
    c = IS.Call(tiny_models["f32"], B)
    items = _params(COUNTS)
    out = {}
    for engine in ENGINES:
        m = tiny_models[engine]
        for compact in (False, True):
            out[engine, compact] = inf.sample_euler_items(m, c.spk.to(m.dtype), c.sm, c.ids, c.tm, items, sequence_length=32, num_steps=COUNTS,
                                                          compact_rows=compact).cpu()
            out[engine, compact, "n"] = m.last_row_forwards()
        assert out[engine, True, "n"] < out[engine, False, "n"]
    for b in range(B):
        ref = out["f32", False][b]
        e32, e16, own = rms(out["f32", True][b], ref), rms(out["bf16", True][b], ref), rms(out["bf16", False][b], ref)
        print(f"item {b}: fp32 compact vs rectangular {e32:.3e} (bound {LAT_TOL:.1e}); bf16 compact vs fp32 {e16:.3e}, bf16 rectangular vs fp32 {own:.3e}")
        assert e32 < LAT_TOL, (b, e32)
        assert e16 < BUDGET * own, (b, e16, own)


def test_stream_batcher_compact_rows_three_staggered_streams(golden, tiny_models):
    """Three streams of 6 / 4 / 6 steps opened one step apart (tests/test_gpu_item_steps.py), mix_steps with compact_rows: as many calls as
    without it, every stream's latents against the stream alone inside LAT_TOL (fp32) / BUDGET (bf16); idle_steps stays 0 and row_forwards
    falls."""
    voices, reqs = IS._stream_requests(golden, (6, 4, 6))
    m32, m16 = tiny_models["f32"], tiny_models["bf16"]
    want32, want16 = [IS._alone(m32, voices, r) for r in reqs], [IS._alone(m16, voices, r) for r in reqs]
    lat, stats = {}, {}
    for tag, m in (("f32", m32), ("bf16", m16)):
        sb = SB.StreamBatcher(m, None, None, voices=voices, max_batch=8, mix_block_sizes=True, mix_steps=True, compact_rows=True)
        mixed, _ = IS._drive(sb, reqs)
        stats[tag] = dict(sb.stats)
        lat[tag] = [torch.cat([b for _, b in mixed[k]], dim=1).cpu() for k in range(len(reqs))]
    sb = SB.StreamBatcher(m32, None, None, voices=voices, max_batch=8, mix_block_sizes=True, mix_steps=True)
    IS._drive(sb, reqs)
    assert stats["f32"]["calls"] == sb.stats["calls"] and stats["f32"]["idle_steps"] == 0 and sb.stats["idle_steps"] > 0
    assert 0 < stats["f32"]["row_forwards"] < sb.stats["row_forwards"]
    for k in range(len(reqs)):
        e32, e16, own = rms(lat["f32"][k], want32[k]), rms(lat["bf16"][k], want32[k]), rms(want16[k], want32[k])
        print(f"compact stream {k}: fp32 vs alone {e32:.3e} (bound {LAT_TOL:.1e}); bf16 vs fp32 alone {e16:.3e}, bf16 alone {own:.3e}")
        assert e32 < LAT_TOL, (k, e32)
        assert e16 < BUDGET * own, (k, e16, own)


def test_synthesize_many_compact_rows_three_jobs(golden, tiny_models):
    """Three jobs in one call, one of them cfg_off: compact_rows=True against each job alone through `synthesize`: same shape, RMS <= 1e-3
    (LAT_TOL: the compacted call has other row counts than the job alone); the call ran fewer row-forwards than without compact_rows."""
    from echo_tts_amd import handler as H
    m = tiny_models["f32"]
    dac = E.DAC(TINY_DAC, R.make_dac_weights(TINY_DAC, 0), device=DEV)
    pca = R.make_pca(TINY_DAC, 80, 0)
    st = E.PCAState(pca.pca_components, pca.pca_mean, pca.latent_scale)
    voices = {"alice": (golden["tiny.spk"], golden["tiny.smask"].bool())}
    jobs = [{"text": "The first of the three.", "speaker_voice": "alice", "parameters": dict(SAMPLER_CASES["cfg_default"], sequence_length=32, seed=5)},
            {"text": "A second request, without guidance.", "speaker_voice": "alice", "parameters": dict(SAMPLER_CASES["cfg_off"], num_steps=6, sequence_length=32, seed=7)},
            {"text": "No voice, in between.", "parameters": dict(SAMPLER_CASES["cfg_default"], cfg_scale_text=2.0, sequence_length=32, seed=3)}]
    assert len(H.plan_mixed_batches(jobs, 24)[1]) == 1
    rect = H.synthesize_many(jobs, m, dac, st, voices=voices)
    n_rect = m.last_row_forwards()
    got = H.synthesize_many(jobs, m, dac, st, voices=voices, compact_rows=True)
    assert m.last_row_forwards() < n_rect
    alone = [voices["alice"], voices["alice"], (None, None)]
    for j in range(3):
        assert "error" not in got[j], got[j].get("traceback")
        assert "error" not in rect[j], rect[j].get("traceback")
        want = H.synthesize(jobs[j], m, dac, st, speaker_latent=alone[j][0], speaker_mask=alone[j][1])
        a, b = want["audio"].float().cpu(), got[j]["audio"].float().cpu()
        assert a.shape == b.shape, (j, a.shape, b.shape)
        print(f"synthesize_many(compact_rows) job {j}: rms vs alone {rms(a, b):.3e}")
        assert rms(a, b) <= LAT_TOL, (j, rms(a, b))
