"""GPU: per-utterance step counts in one sampler call (echo_sample_euler_items_steps) and the host paths on top of it
(sample_euler_items(num_steps=[...]), StreamBatcher(mix_steps=True), synthesize_many(mix_steps=True)).

A call has B items and N = the largest step count; item b runs item_steps[b] steps of its own schedule and is then left alone.  Asserted:
  - equal counts give the bits of echo_sample_euler_items_len (one group is one modulation segment: the same launches);
  - an item of a mixed call has, bit for bit, the result of the call in which every item runs that item's count: rows do not see each
    other and a finished row's state is not touched after its last step;
  - an item against the uniform batch-1 call of its own step count: other M, other plans, so the suite's tolerances, not equality;
  - teeth for both; a stale workspace; the CFG row set follows the active items only; lengths and positions on top; refusals; the host."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import echo_ref as R  # noqa: E402  (checker only)
from tests import gpu_util as U  # noqa: E402
from tests.golden_defs import SAMPLER_CASES, TINY, TINY_DAC, WIDE1  # noqa: E402

import echo_tts_amd as E  # noqa: E402
from echo_tts_amd import _lib as L  # noqa: E402
from echo_tts_amd import handler as H  # noqa: E402
from echo_tts_amd import inference as inf  # noqa: E402
from echo_tts_amd import inference_blockwise as IB  # noqa: E402
from echo_tts_amd import stream_batch as SB  # noqa: E402

DEV = U.DEV
LAT_TOL = 1e-3      # fp32 engine, other-geometry comparisons: the constant of tests/test_gpu_engine.py
BUDGET = 1.5        # bf16: distance to the fp32 uniform call <= BUDGET x the uniform bf16 call's own distance to it (the suite's rule)
ENGINES = ["f32", "bf16"]
SENTINEL = -7.25


def rms(a, b):
    return float((a.float().cpu() - b.float().cpu()).pow(2).mean().sqrt())


def _make_models():
    w = R.make_dit_weights(TINY, seed=0)
    return {"f32": E.EchoDiT(TINY, w, dtype=torch.float32, device=DEV),
            "bf16": E.EchoDiT(TINY, {k: v.bfloat16() for k, v in w.items()}, dtype=torch.bfloat16, device=DEV)}


@pytest.fixture(scope="module")
def tiny_models():
    return _make_models()


def _params(counts):
    """Distinct per-item request parameters (SAMPLER_CASES), item b at counts[b] steps."""
    names = ("cfg_default", "cfg_off", "all_options")
    return [dict(SAMPLER_CASES[names[b % 3]], num_steps=int(n), rng_seed=b) for b, n in enumerate(counts)]


class Call:
    """B utterances (own text, voice, latent prefix, noise) on one model; every run re-encodes the caches, because an item with
    speaker_kv_scale scales and un-scales its speaker KV inside the call (bf16: not an exact round trip)."""

    def __init__(self, m, B, S=32, P=16, seed=11):
        self.m, self.B, self.S = m, B, S
        gen = torch.Generator().manual_seed(seed)
        self.ids = torch.randint(1, 256, (B, 24), generator=gen, dtype=torch.int32)
        self.tm = torch.zeros((B, 24), dtype=torch.bool)
        self.sm = torch.zeros((B, 16), dtype=torch.bool)
        for b in range(B):
            self.tm[b, :24 - 3 * (b % 5)] = True
            self.sm[b, :16 - 4 * (b % 3)] = True
        self.spk = torch.randn((B, 16, 80), generator=gen)
        self.prefix = torch.randn((B, P, 80), generator=gen)
        self.x = torch.randn((B, S, 80), generator=gen)

    def caches(self, items, rows=None):
        m, rows = self.m, list(range(self.B)) if rows is None else rows
        m.get_kv_cache_text(self.ids[rows], self.tm[rows])
        kvs = m.get_kv_cache_speaker(self.spk[rows].to(m.dtype), self.sm[rows])
        m.get_kv_cache_latent(self.prefix[rows])
        if any(it["speaker_kv_scale"] is not None for it in items):
            inf._multiply_kv_cache_items(kvs, [1.0 if it["speaker_kv_scale"] is None else it["speaker_kv_scale"] for it in items],
                                         [it["speaker_kv_max_layers"] for it in items])

    def steps_abi(self, items, counts, *, pos=None, lengths=None, start_pos=0, N=None, temb=None, x=None, item_steps="counts", fill=None):
        """echo_sample_euler_items_steps through the C ABI.  Returns (status, latent_out)."""
        m, B = self.m, self.B
        self.caches(items)
        arr, _t, keep = inf.build_sampler_items(m, items)
        N = max(counts) if N is None else N
        if temb is None:
            temb = inf.step_groups_temb(m, counts, N)
        td = temb.to(DEV).contiguous()
        p = L.EchoSamplerParams()
        p.B, p.S, p.num_steps, p.start_pos, p.use_latent = B, self.S, N, int(start_pos), 1
        p.temb = td.data_ptr()
        x0 = (self.x if x is None else x).to(DEV, torch.float32).contiguous()
        out = torch.empty_like(x0) if fill is None else torch.full_like(x0, fill)
        tab = (C.c_int32 * B)(*counts) if item_steps == "counts" else item_steps
        rc = m._lib.echo_sample_euler_items_steps(m._ctx, C.byref(p), arr, tab, None if pos is None else (C.c_int32 * B)(*pos),
                                                  None if lengths is None else (C.c_int32 * B)(*lengths), x0.data_ptr(), out.data_ptr(), m._stream())
        torch.cuda.synchronize()
        del keep
        return rc, out

    def steps(self, items, counts, **kw):
        rc, out = self.steps_abi(items, counts, **kw)
        assert rc == 0, self.m._lib.echo_last_error(self.m._ctx)
        return out.cpu()

    def existing(self, items, *, pos=None, lengths=None, start_pos=0, x=None, rows=None):
        """The existing calls (echo_sample_euler_items / _pos / _len) for items that share num_steps; `rows`: a sub-batch of the utterances."""
        self.caches(items, rows)
        arr, temb, _keep = inf.build_sampler_items(self.m, items)
        x0 = (self.x if x is None else x)
        x0 = x0 if rows is None else x0[rows]
        return inf.run_euler_items(self.m, x0.to(DEV), arr, int(items[0]["num_steps"]), temb, start_pos=start_pos if pos is None else pos,
                                   use_latent=True, lengths=lengths).cpu()


def _same_count_reference(c, items, b, **kw):
    """The call of counts (n_b, ..., n_b): every other item's tables replaced by schedules of n_b steps (its own parameters otherwise)."""
    n = int(items[b]["num_steps"])
    return c.steps([dict(it, num_steps=n) for it in items], [n] * c.B, **kw)


# ------------------------------------------------------------------------------------------------ 0. symbol
def test_entry_point_is_bound():
    lib = L.load_library()
    assert lib.echo_sample_euler_items_steps.argtypes == L.SIGNATURES["echo_sample_euler_items_steps"][1]
    assert lib.echo_abi_version() == 8


# ------------------------------------------------------------------------------------------------ 1. equal counts
@pytest.mark.parametrize("positions", [False, True])
@pytest.mark.parametrize("engine", ENGINES)
def test_equal_counts_give_the_bits_of_the_length_call(tiny_models, engine, positions):
    """B = 3, S = 32, counts (6, 6, 6), three parameter sets: torch.equal with echo_sample_euler_items_len on the same inputs (full and ragged
    lengths), with a position table and with NULL (every item at p->start_pos); without a length table, with the plain / position call."""
    c = Call(tiny_models[engine], 3)
    items = _params([6, 6, 6])
    pos, sp = ([0, 13, 5], 0) if positions else (None, 13)
    for lengths in ([32, 32, 32], [32, 20, 9]):
        want = c.existing(items, pos=pos, lengths=lengths, start_pos=sp)
        got = c.steps(items, [6, 6, 6], pos=pos, lengths=lengths, start_pos=sp)
        assert bool(torch.isfinite(want).all()) and float(want.abs().max()) > 0
        assert torch.equal(got, want), (engine, positions, lengths)
    want = c.existing(items, pos=pos, start_pos=sp)
    assert torch.equal(c.steps(items, [6, 6, 6], pos=pos, start_pos=sp), want)


# ------------------------------------------------------------------------------------------------ 2. a finished item is frozen
FORMS = {"plain": dict(), "len_pos": dict(pos=[0, 13, 5], lengths=[32, 20, 27])}


def _frozen(c, counts, form):
    items = _params(counts)
    got = c.steps(items, counts, **FORMS[form])
    assert bool(torch.isfinite(got).all())
    for b in range(c.B):
        want = _same_count_reference(c, items, b, **FORMS[form])
        assert float(want[b].abs().max()) > 0
        assert torch.equal(got[b], want[b]), f"item {b} ({counts[b]} of {max(counts)} steps) differs from the call of its own count"
    return items, got


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("engine", ENGINES)
def test_a_finished_item_is_frozen(tiny_models, engine, form):
    """B = 3, S = 32, counts (6, 4, 2), parameter sets cfg_default / cfg_off / all_options (its speaker-KV un-scaling fires at its own step):
    latent_out of item b equals, bit for bit, its row in the call of counts (n_b, n_b, n_b) - same B, S, tables of b.  Both forms of the
    update (euler_items_kernel without a length table; with ragged lengths and a position table)."""
    _frozen(Call(tiny_models[engine], 3), [6, 4, 2], form)


# ------------------------------------------------------------------------------------------------ 3. against the uniform call of the item's count
def _uniform_alone(c, items, b, *, S=None, start_pos=0):
    """The existing echo_sample_euler_items(_pos) call with B = 1 at the item's own step count (and length / position)."""
    x = c.x if S is None else c.x[:, :S]
    return c.existing([items[b]], rows=[b], x=x, start_pos=start_pos)[0]


def _check_against_uniform(c32, c16, items, got32, got16, alone, label):
    """fp32: rms < LAT_TOL.  bf16: rms(mixed_bf16 - uniform_fp32) < BUDGET x rms(uniform_bf16 - uniform_fp32), both measured here."""
    out = []
    for b in range(c32.B):
        w32, w16 = alone(c32, b), alone(c16, b)
        n = w32.shape[0]
        e32, e16, own = rms(got32[b][:n], w32), rms(got16[b][:n], w32), rms(w16, w32)
        print(f"{label} item {b} ({items[b]['num_steps']} steps): fp32 mixed vs uniform rms {e32:.3e} (bound {LAT_TOL:.1e}); "
              f"bf16 mixed vs fp32 uniform {e16:.3e}, uniform bf16 vs fp32 uniform {own:.3e} (bound {BUDGET * own:.3e})")
        out.append((e32, e16, own))
    return out


@pytest.fixture(scope="module")
def wide_models():
    w = R.make_dit_weights(WIDE1, seed=0)
    return {"f32": E.EchoDiT(WIDE1, w, dtype=torch.float32, device=DEV),
            "bf16": E.EchoDiT(WIDE1, {k: v.bfloat16() for k, v in w.items()}, dtype=torch.bfloat16, device=DEV)}


def _against_uniform_and_swapped(models, counts):
    B = len(counts)
    c32, c16 = Call(models["f32"], B), Call(models["bf16"], B)
    items = _params(counts)
    got32, got16 = c32.steps(items, counts), c16.steps(items, counts)
    res = _check_against_uniform(c32, c16, items, got32, got16, lambda c, b: _uniform_alone(c, items, b), f"mixed {tuple(counts)}")
    for b, (e32, e16, own) in enumerate(res):
        assert e32 < LAT_TOL, (b, e32)
        assert e16 < BUDGET * own, (b, e16, own)
    bad, G, N = {}, len(set(counts)), max(counts)
    for tag, c in (("f32", c32), ("bf16", c16)):
        t = inf.step_groups_temb(c.m, counts, N).reshape(N, G, -1).clone()
        t[:, [0, 1]] = t[:, [1, 0]]
        bad[tag] = c.steps(items, counts, temb=t.reshape(N * G, -1))
    swapped = _check_against_uniform(c32, c16, items, bad["f32"], bad["bf16"], lambda c, b: _uniform_alone(c, items, b), "swapped columns")
    for b in range(2, B):                                # the columns that stayed: the same bits
        assert torch.equal(bad["f32"][b], got32[b]) and torch.equal(bad["bf16"][b], got16[b])
    return swapped


def test_each_item_against_the_uniform_call_of_its_own_step_count(tiny_models):
    """TINY, counts (6, 4, 2) against echo_sample_euler_items with B = 1 at n_b steps.  Measured (MI355X): fp32 0 (the plans coincide); bf16
    mixed exactly as far from the fp32 uniform call as the uniform bf16 call is (1.8e-3 / 6.6e-4 / 2.9e-3, bounds 1.5 x that).
    With the columns of the 6- and the 4-step group swapped in the [N][G] table both items move (asserted), but TINY's random weights make
    little of a timestep: 4.6e-4 and 3.0e-4 RMS in fp32 (the CPU oracle gives the same figures, and 8.7e-4 for the most different schedule
    there is), below the 1e-3 bound.  The teeth of the tolerance are therefore shown on WIDE1, next test."""
    swapped = _against_uniform_and_swapped(tiny_models, [6, 4, 2])
    for b in (0, 1):
        assert swapped[b][0] > 1e-4, (b, swapped[b])


def test_wrong_group_embeddings_leave_the_tolerance(wide_models):
    """WIDE1 (full widths, one layer), counts (6, 4), in the bounds of the test above; then the two columns of the [N][G] table swapped:
    each item gets the other group's embeddings and leaves both bounds (the CPU oracle puts the fp32 effect at 0.56 and 0.42 RMS)."""
    swapped = _against_uniform_and_swapped(wide_models, [6, 4])
    for b in (0, 1):
        e32, e16, own = swapped[b]
        assert e32 > LAT_TOL and e16 > BUDGET * own, (b, swapped[b])


# ------------------------------------------------------------------------------------------------ 4. teeth of test 2
@pytest.mark.parametrize("engine", ENGINES)
def test_ignoring_the_done_flag_is_caught(tiny_models, engine):
    """echo_debug_item_steps_ignore_done: the table is built without `done`, so a finished item is updated again with its last entry.  The
    two items that finish early differ from test 2's result; item 0, never finished, keeps its bits."""
    m = tiny_models[engine]
    c = Call(m, 3)
    items, good = _frozen(c, [6, 4, 2], "plain")
    assert m._lib.echo_debug_item_steps_ignore_done(m._ctx, 1) == 0
    try:
        bad = c.steps(items, [6, 4, 2])
        again = c.steps(items, [6, 4, 2])                                    # one-shot: the call above consumed the instrument
    finally:
        assert m._lib.echo_debug_item_steps_ignore_done(m._ctx, 0) == 0
    assert torch.equal(bad[0], good[0])
    assert not torch.equal(bad[1], good[1]) and not torch.equal(bad[2], good[2])
    assert torch.equal(again, good)


# ------------------------------------------------------------------------------------------------ 5. stale workspace
@pytest.mark.parametrize("engine", ENGINES)
def test_stale_workspace_of_a_uniform_call(engine):
    """A uniform 6-step call whose x_init holds 1e30 in the rows of the items that will finish early, then the mixed call (6, 4, 2) on the
    same context: bit-equal to the mixed call run first in a fresh context; every value finite."""
    items, counts = _params([6, 4, 2]), [6, 4, 2]
    fresh = Call(_make_models()[engine], 3)
    want = fresh.steps(items, counts)
    c = Call(_make_models()[engine], 3)
    x = c.x.clone()
    x[1:] = 1e30
    dirty = c.existing(_params([6, 6, 6]), x=x)
    assert not bool(torch.isfinite(dirty[1:]).all()) or float(dirty[1:].abs().max()) > 1e20
    got = c.steps(items, counts)
    assert bool(torch.isfinite(got).all())
    assert torch.equal(got, want)


# ------------------------------------------------------------------------------------------------ 6. CFG window over active items only
def _n_gemm(c, items, counts):
    m = c.m
    assert m._lib.echo_set_profiling(m._ctx, 1) == 0
    try:
        out = c.steps(items, counts)
        prof = L.EchoProfile()
        assert m._lib.echo_get_profile(m._ctx, C.byref(prof)) == 0
    finally:
        assert m._lib.echo_set_profiling(m._ctx, 0) == 0
    return out, int(prof.n_gemm)


@pytest.mark.parametrize("engine", ENGINES)
def test_cfg_rows_follow_the_active_items_only(tiny_models, engine):
    """Counts (6, 2): the 6-step item has CFG off (cfg_min_t 1.1), the 2-step item has it at both of its steps (cfg_min_t 0: its LAST
    entry, which a finished item's table slot repeats, has CFG too).  Iterations 0-1 must run 3 B rows, iterations 2-5 B rows.
    The GEMM launches of a forward depend on its row set alone, so two control calls with the same counts and segments give the unit:
    nobody has CFG (six forwards of B rows), and the 6-step item has CFG throughout (six forwards of 3 B rows).  The call under test must
    count two 3 B forwards and four B forwards.  bf16 engine (fused attention: no GEMM inside it) also by formula: a forward is
    in_proj + out_proj + L x (QKVG + w1|w3 + wo and w2 once per modulation segment), two interleaved groups over `rows` rows are `rows`
    segments, the modulation 5 launches."""
    c = Call(tiny_models[engine], 2)
    slow, fast = dict(SAMPLER_CASES["cfg_off"], num_steps=6, rng_seed=0), dict(SAMPLER_CASES["cfg_default"], num_steps=2, cfg_min_t=0.0, rng_seed=1)
    items, counts = [slow, fast], [6, 2]
    got, n = _n_gemm(c, items, counts)
    _, n_b = _n_gemm(c, [slow, dict(fast, cfg_min_t=1.1)], counts)
    _, n_3b = _n_gemm(c, [dict(slow, cfg_min_t=0.0), fast], counts)
    assert n_3b > n_b and (n_3b - n_b) % 6 == 0
    want_n = n_b + 2 * (n_3b - n_b) // 6
    print(f"GEMM launches of the (6, 2) call: {n} (B rows throughout: {n_b}; 3 B rows throughout: {n_3b}; 3 B rows in iterations 0-1 only: {want_n})")
    assert n == want_n
    if engine == "bf16":
        def fwd(segs):
            return 2 + TINY.num_layers * (2 + 2 * segs)
        assert (n_b, n, n_3b) == (5 + 6 * fwd(2), 5 + 2 * fwd(6) + 4 * fwd(2), 5 + 6 * fwd(6))
    for b in range(2):
        assert torch.equal(got[b], _same_count_reference(c, items, b)[b]), b


# ------------------------------------------------------------------------------------------------ 7. lengths and positions combined
def test_lengths_and_positions_combined(tiny_models):
    """Counts (6, 4), lengths (32, 20), positions (0, 13), a latent prefix of 16: each item against itself alone (B = 1, S = its length, its
    position, its step count) in the tolerances of test 3; the padding of the result is exactly 0."""
    c32, c16 = Call(tiny_models["f32"], 2), Call(tiny_models["bf16"], 2)
    counts, lengths, pos = [6, 4], [32, 20], [0, 13]
    items = _params(counts)
    got32 = c32.steps(items, counts, pos=pos, lengths=lengths)
    got16 = c16.steps(items, counts, pos=pos, lengths=lengths)
    for got in (got32, got16):
        assert bool(torch.isfinite(got).all()) and bool((got[1, 20:] == 0).all()) and float(got[1, :20].abs().max()) > 0
    res = _check_against_uniform(c32, c16, items, got32, got16, lambda c, b: _uniform_alone(c, items, b, S=lengths[b], start_pos=pos[b]),
                                 "lengths (32, 20) positions (0, 13)")
    for b, (e32, e16, own) in enumerate(res):
        assert e32 < LAT_TOL, (b, e32)
        assert e16 < BUDGET * own, (b, e16, own)


# ------------------------------------------------------------------------------------------------ 8. refusals
def test_bad_step_tables_are_refused_and_the_context_survives(tiny_models):
    """NULL table, a count of 0, a count above N, unequal dt inside a group, 9 groups: each a non-zero status with its message, nothing
    written to latent_out (pre-filled with a sentinel), and a valid call right behind each refusal gives the first valid call's bits."""
    m = tiny_models["bf16"]
    c = Call(m, 3)
    items, counts = _params([6, 4, 4]), [6, 4, 4]
    good = c.steps(items, counts)

    def refused(rc, out, msg):
        err = m._lib.echo_last_error(m._ctx)
        assert rc != 0 and msg in err, (msg, err)
        assert bool((out == SENTINEL).all()), msg
        assert torch.equal(c.steps(items, counts), good), msg

    refused(*c.steps_abi(items, counts, item_steps=None, fill=SENTINEL), b"null step-count table")
    refused(*c.steps_abi(items, counts, item_steps=(C.c_int32 * 3)(6, 0, 4), fill=SENTINEL), b"a step count is below 1")
    refused(*c.steps_abi(items, counts, item_steps=(C.c_int32 * 3)(6, 7, 4), fill=SENTINEL), b"a step count is above the call's num_steps")
    # two items of the 4-step group whose dt differ: item 2 gets a copy of its table with one dt moved
    c.caches(items)
    arr, _t, keep = inf.build_sampler_items(m, items)
    moved = (L.EchoStep * 4)()
    for i in range(4):
        C.memmove(C.byref(moved[i]), C.byref(arr[2].steps[i]), C.sizeof(L.EchoStep))
    moved[1].dt = moved[1].dt * 1.5
    arr[2].steps = moved
    p = L.EchoSamplerParams()
    p.B, p.S, p.num_steps, p.use_latent = 3, 32, 6, 1
    td = inf.step_groups_temb(m, counts, 6).to(DEV).contiguous()
    p.temb = td.data_ptr()
    x0 = c.x.to(DEV).contiguous()
    out = torch.full_like(x0, SENTINEL)
    rc = m._lib.echo_sample_euler_items_steps(m._ctx, C.byref(p), arr, (C.c_int32 * 3)(*counts), None, None, x0.data_ptr(), out.data_ptr(), m._stream())
    torch.cuda.synchronize()
    refused(rc, out.cpu(), b"differ in their schedules (dt)")
    del keep
    # 9 distinct counts need 9 items; 8 are served
    c9 = Call(m, 9)
    nine = list(range(10, 1, -1))
    refused(*c9.steps_abi(_params(nine), nine, fill=SENTINEL), b"more than 8 distinct step counts")
    eight = nine[:8] + [nine[7]]
    assert bool(torch.isfinite(c9.steps(_params(eight), eight)).all())
    # the host layer raises ValueError for the same tables before any device work
    arr, _t, keep = inf.build_sampler_items(m, items)
    for bad, msg in (([6, 0, 4], "below 1"), ([6, 7, 4], "above the call's num_steps"), ([6, 4], "one step count per item")):
        with pytest.raises(ValueError, match=msg):
            inf.run_euler_items(m, c.x.to(DEV), arr, 6, None, item_steps=bad)


def test_one_scaled_voice_at_different_step_counts_is_refused(tiny_models):
    """Three items share ONE voice (speaker cache of batch 1) and scale its KV (all_options): at counts (6, 4, 6) each would undo the scale in
    another iteration.  The engine refuses with its own message and writes nothing; the host raises ValueError before any device work; equal
    counts on the same shared voice are served."""
    m = tiny_models["bf16"]
    c = Call(m, 3)
    items = [dict(SAMPLER_CASES["all_options"], num_steps=n, rng_seed=b) for b, n in enumerate((6, 4, 6))]

    def shared_voice_call(its, counts):
        m.get_kv_cache_text(c.ids, c.tm)
        kvs = m.get_kv_cache_speaker(c.spk[:1].to(m.dtype), c.sm[:1])
        inf._multiply_kv_cache_items(kvs, [it["speaker_kv_scale"] for it in its], [it["speaker_kv_max_layers"] for it in its])
        arr, _t, keep = inf.build_sampler_items(m, its)
        p = L.EchoSamplerParams()
        p.B, p.S, p.num_steps = 3, 32, max(counts)
        td = inf.step_groups_temb(m, counts, max(counts)).to(DEV).contiguous()
        p.temb = td.data_ptr()
        x0 = c.x.to(DEV).contiguous()
        out = torch.full_like(x0, SENTINEL)
        rc = m._lib.echo_sample_euler_items_steps(m._ctx, C.byref(p), arr, (C.c_int32 * 3)(*counts), None, None, x0.data_ptr(), out.data_ptr(), m._stream())
        torch.cuda.synchronize()
        del keep
        return rc, out.cpu()

    rc, out = shared_voice_call(items, [6, 4, 6])
    assert rc != 0 and b"un-scale its speaker KV at different iterations" in m._lib.echo_last_error(m._ctx)
    assert bool((out == SENTINEL).all())
    with pytest.raises(ValueError, match="undone at different iterations"):
        inf.sample_euler_items(m, c.spk[:1].to(m.dtype), c.sm[:1], c.ids, c.tm, items, sequence_length=32, x_init=c.x, num_steps=[6, 4, 6])
    rc, out = shared_voice_call([dict(it, num_steps=6) for it in items], [6, 6, 6])
    assert rc == 0 and bool(torch.isfinite(out).all()) and not bool((out == SENTINEL).any())


def test_fp8_engine_refuses_step_tables():
    """The fp8 engine is not supported (the same reason as the length tables): refused up front, nothing written, and it goes on serving
    the calls it has."""
    w = {k: v.bfloat16() for k, v in R.make_dit_weights(TINY, seed=0).items()}
    m8 = E.EchoDiT(TINY, w, dtype=torch.bfloat16, device=DEV, fp8=True)
    c = Call(m8, 3)
    items, counts = _params([6, 4, 4]), [6, 4, 4]
    rc, out = c.steps_abi(items, counts, fill=SENTINEL)
    assert rc != 0 and b"not supported by the fp8 engine" in m8._lib.echo_last_error(m8._ctx)
    assert bool((out == SENTINEL).all())
    arr, _t, _keep = inf.build_sampler_items(m8, items)
    with pytest.raises(ValueError, match="not supported by the fp8 engine"):
        inf.run_euler_items(m8, c.x.to(DEV), arr, 6, None, item_steps=counts)
    assert bool(torch.isfinite(c.existing(_params([6, 6, 6]))).all())


# ------------------------------------------------------------------------------------------------ 9. host
def test_sample_euler_items_with_a_list_of_step_counts(tiny_models):
    """sample_euler_items(num_steps=[6, 4, 6]): results in the caller's order, torch.equal with run_euler_items(item_steps=[6, 6, 4]) on the
    rows sorted by step count (stable) with the same noise; a list of equal values gives the bits of today's call."""
    m = tiny_models["f32"]
    c = Call(m, 3)
    items = [dict(it, num_steps=6) for it in _params([6, 6, 6])]
    for it in items:
        it["speaker_kv_scale"] = it["speaker_kv_max_layers"] = it["speaker_kv_min_t"] = None
    got = inf.sample_euler_items(m, c.spk.to(m.dtype), c.sm, c.ids, c.tm, items, sequence_length=32, x_init=c.x, num_steps=[6, 4, 6]).cpu()
    order, counts = [0, 2, 1], [6, 6, 4]
    srt = [dict(items[b], num_steps=n) for b, n in zip(order, counts)]
    m.get_kv_cache_text(c.ids[order], c.tm[order])
    m.get_kv_cache_speaker(c.spk[order].to(m.dtype), c.sm[order])
    arr, _t, _keep = inf.build_sampler_items(m, srt)
    want = inf.run_euler_items(m, c.x[order].to(DEV), arr, 6, None, item_steps=counts).cpu()
    assert bool(torch.isfinite(got).all())
    for r, b in enumerate(order):
        assert torch.equal(got[b], want[r]), b
    today = inf.sample_euler_items(m, c.spk.to(m.dtype), c.sm, c.ids, c.tm, items, sequence_length=32, x_init=c.x).cpu()
    assert torch.equal(inf.sample_euler_items(m, c.spk.to(m.dtype), c.sm, c.ids, c.tm, items, sequence_length=32, x_init=c.x, num_steps=[6, 6, 6]).cpu(), today)
    assert torch.equal(inf.sample_euler_items(m, c.spk.to(m.dtype), c.sm, c.ids, c.tm, items, sequence_length=32, x_init=c.x, num_steps=6).cpu(), today)
    assert torch.equal(got[0], today[0]) or rms(got[0], today[0]) < LAT_TOL          # the 6-step rows: today's rows up to the launch geometry
    with pytest.raises(ValueError, match="share num_steps"):                         # without the new argument the old rule holds
        inf.sample_euler_items(m, c.spk.to(m.dtype), c.sm, c.ids, c.tm, [dict(it, num_steps=n) for it, n in zip(items, (6, 4, 6))],
                               sequence_length=32, x_init=c.x)


def _stream_requests(g, steps):
    gen = torch.Generator().manual_seed(21)
    base = dict(SAMPLER_CASES["cfg_default"])
    voices = {"a": (g["tinyb2.spk"][0:1], g["tinyb2.smask"].bool()[0:1]), "b": (g["tinyb2.spk"][1:2], g["tinyb2.smask"].bool()[1:2])}
    reqs = []
    for i, (voice, over, blocks) in enumerate((("a", {}, [8, 16, 16]), ("b", dict(cfg_scale_text=2.0, cfg_scale_speaker=5.0), [16, 16]),
                                               (None, dict(cfg_scale_text=4.0), [8, 8, 24]))):
        row = i % 2
        reqs.append(dict(text_input_ids=g["tinyb2.ids"][row:row + 1], text_mask=g["tinyb2.tmask"].bool()[row:row + 1],
                         item_params=dict(base, num_steps=steps[i], **over), block_sizes=blocks, rng_seed=i, speaker_voice=voice,
                         x_inits=[torch.randn((1, n, 80), generator=gen) for n in blocks]))
    return voices, reqs


def _alone(m, voices, r):
    if r["speaker_voice"] is None:
        spk, sm = torch.zeros((1, 4, 80)), torch.zeros((1, 4), dtype=torch.bool)
    else:
        spk, sm = voices[r["speaker_voice"]]
    return IB.sample_blockwise_euler_cfg_independent_guidances(m, spk.to(m.dtype), sm, r["text_input_ids"], r["text_mask"], rng_seed=r["rng_seed"],
                                                               block_sizes=r["block_sizes"], x_inits=r["x_inits"], **r["item_params"]).cpu()


def _drive(sb, reqs):
    """Streams opened one step apart; returns ({request index: [(start, block)]}, calls)."""
    got, sid = {}, {}
    k = 0
    while k < len(reqs) or sb.open_ids:
        if k < len(reqs):
            sid[sb.open(**reqs[k])] = k
            k += 1
        for i, p, blk in sb.step():
            got.setdefault(sid[i], []).append((p, blk.clone()))
    return got, sb.stats["calls"]


def test_stream_batcher_mix_steps_end_to_end(golden, tiny_models):
    """Three streams of 6 / 4 / 6 steps with block schedules [8, 16, 16], [16, 16], [8, 8, 24], opened one step apart:
    StreamBatcher(mix_block_sizes=True, mix_steps=True) makes fewer sampler calls than mix_steps=False; each stream's latents and their
    decoded audio against the same stream alone through the existing blockwise sampler, in the tolerances of test 3."""
    voices, reqs = _stream_requests(golden, (6, 4, 6))
    m32, m16 = tiny_models["f32"], tiny_models["bf16"]
    want32, want16 = [_alone(m32, voices, r) for r in reqs], [_alone(m16, voices, r) for r in reqs]
    lat, calls = {}, {}
    for tag, m in (("f32", m32), ("bf16", m16)):
        mixed, calls[tag] = _drive(SB.StreamBatcher(m, None, None, voices=voices, max_batch=8, mix_block_sizes=True, mix_steps=True), reqs)
        for k, r in enumerate(reqs):
            assert [b.shape[1] for _, b in mixed[k]] == r["block_sizes"]
            assert [p for p, _ in mixed[k]] == [sum(r["block_sizes"][:i]) for i in range(len(r["block_sizes"]))]
        lat[tag] = [torch.cat([b for _, b in mixed[k]], dim=1).cpu() for k in range(len(reqs))]
    _, calls_grouped = _drive(SB.StreamBatcher(m32, None, None, voices=voices, max_batch=8, mix_block_sizes=True), reqs)
    print(f"sampler calls: {calls['f32']} with mix_steps, {calls_grouped} grouped by step count")
    assert calls["f32"] < calls_grouped and calls["bf16"] == calls["f32"]
    dac = E.DAC(TINY_DAC, R.make_dac_weights(TINY_DAC, 0), device=DEV)
    pca = R.make_pca(TINY_DAC, 80, 0)
    st = E.PCAState(pca.pca_components, pca.pca_mean, pca.latent_scale)

    def audio(x):
        return E.ae_decode(dac, st, x.to(DEV)).cpu()

    for k in range(len(reqs)):
        for what, f in (("latents", lambda x: x), ("audio", audio)):
            w32, w16 = f(want32[k]), f(want16[k])
            e32, e16, own = rms(f(lat["f32"][k]), w32), rms(f(lat["bf16"][k]), w32), rms(w16, w32)
            print(f"mix_steps stream {k} {what}: fp32 vs alone {e32:.3e} (bound {LAT_TOL:.1e}); bf16 vs fp32 alone {e16:.3e}, "
                  f"bf16 alone vs fp32 alone {own:.3e} (bound {BUDGET * own:.3e})")
            assert e32 < LAT_TOL, (k, what, e32)
            assert e16 < BUDGET * own, (k, what, e16, own)


def test_synthesize_many_mix_steps_equals_the_jobs_run_alone(golden, tiny_models):
    """Three jobs of 6 / 4 / 4 steps (sequence lengths 32 / 24 / 16): ONE sampler call with mix_lengths=True, mix_steps=True (two with
    mix_lengths alone); each job's audio against the job alone through `synthesize`: same shape, RMS <= 1e-4 (the bound
    tests/test_gpu_item_lengths.py uses for mix_lengths)."""
    m = tiny_models["f32"]
    dac = E.DAC(TINY_DAC, R.make_dac_weights(TINY_DAC, 0), device=DEV)
    pca = R.make_pca(TINY_DAC, 80, 0)
    st = E.PCAState(pca.pca_components, pca.pca_mean, pca.latent_scale)
    voices = {"alice": (golden["tiny.spk"], golden["tiny.smask"].bool())}
    jobs = [{"text": "The shortest of the three.", "speaker_voice": "alice", "parameters": dict(SAMPLER_CASES["cfg_default"], num_steps=4, sequence_length=16, seed=5)},
            {"text": "A second request, the longest one.", "speaker_voice": "alice", "parameters": dict(SAMPLER_CASES["cfg_default"], num_steps=6, sequence_length=32, seed=7)},
            {"text": "No voice, in between.", "parameters": dict(SAMPLER_CASES["cfg_default"], num_steps=4, cfg_scale_text=2.0, sequence_length=24, seed=3)}]
    _, calls = H.plan_mixed_batches(jobs, 24, mix_lengths=True, mix_steps=True)
    assert len(calls) == 1 and calls[0]["item_steps"] == [6, 4, 4] and calls[0]["lengths"] == [32, 24, 16]
    assert len(H.plan_mixed_batches(jobs, 24, mix_lengths=True)[1]) == 2
    got = H.synthesize_many(jobs, m, dac, st, voices=voices, mix_lengths=True, mix_steps=True)
    alone = [voices["alice"], voices["alice"], (None, None)]
    for j in range(3):
        assert "error" not in got[j], got[j].get("traceback")
        want = H.synthesize(jobs[j], m, dac, st, speaker_latent=alone[j][0], speaker_mask=alone[j][1])
        assert "error" not in want, want.get("traceback")
        a, b = want["audio"].float().cpu(), got[j]["audio"].float().cpu()
        assert a.shape == b.shape, (j, a.shape, b.shape)
        print(f"synthesize_many(mix_steps) job {j}: rms vs alone {rms(a, b):.3e}")
        assert rms(a, b) <= 1e-4, (j, rms(a, b))
