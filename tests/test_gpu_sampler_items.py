"""GPU: mixed batches - one sampler call whose utterances bring their own request parameters and their own cached voice
(echo_sample_euler_items, echo_scale_speaker_kv_items, echo_voice_bind_items; inference.sample_euler_items, EchoDiT.bind_voices,
handler.synthesize_many).  Tiny model, S = 32, the committed goldens.

Tolerances are the suite's own: LAT_TOL / WAV_TOL on the fp32 engine, and for the bf16 engine the budget rule of
tests/test_gpu_engine.py (1.5 x the reference's own bf16-vs-fp32 distance + 1e-3), evaluated per row from the two goldens the row
comes from.  Where geometry and launches are the same and rows are independent in every kernel, bit equality is asserted."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import echo_ref as R  # noqa: E402  (checker only)
from tests import gpu_util as U  # noqa: E402
from tests.golden_defs import SAMPLER_CASES, TINY, TINY_DAC  # noqa: E402

import echo_tts_amd as E  # noqa: E402
from echo_tts_amd import _lib as L  # noqa: E402
from echo_tts_amd import inference as inf  # noqa: E402

DEV = U.DEV
LAT_TOL = 1e-3      # the constants of tests/test_gpu_engine.py
WAV_TOL = 1e-4
ENGINES = ["f32", "bf16"]


def rms(a, b):
    return float((a.float().cpu() - b.float().cpu()).pow(2).mean().sqrt())


def _bf16_row_budget(golden, case, row):
    """tests/test_gpu_engine.py `_bf16_budget`, for one row of the tinyb2 goldens"""
    return 1.5 * rms(golden[f"tinyb2.bf16.euler.{case}"][row], golden[f"tinyb2.f32.euler.{case}"][row]) + 1e-3


@pytest.fixture(scope="module")
def tiny_models():
    w = R.make_dit_weights(TINY, seed=0)
    return {"f32": E.EchoDiT(TINY, w, dtype=torch.float32, device=DEV),
            "bf16": E.EchoDiT(TINY, {k: v.bfloat16() for k, v in w.items()}, dtype=torch.bfloat16, device=DEV)}


def _b2(g, ts=32):
    """(speaker latent, speaker mask, ids, text mask) of the batch-2 fixture; ts < 32 truncates the speaker reference"""
    return g["tinyb2.spk"][:, :ts].contiguous(), g["tinyb2.smask"].bool()[:, :ts].contiguous(), g["tinyb2.ids"], g["tinyb2.tmask"].bool()


def _mixed(m, g, params, ts=32, **kw):
    items = [dict(p, rng_seed=0) for p in params]
    return inf.sample_euler_items(m, *_b2(g, ts), items, sequence_length=32, x_init=g["tinyb2.x0"], **kw)


def _uniform(m, g, p, ts=32):
    return E.sample_euler_cfg_independent_guidances(m, *_b2(g, ts), rng_seed=0, sequence_length=32, x_init=g["tinyb2.x0"], **p)


# ------------------------------------------------------------------------------------------------ 1. the reference's own goldens
@pytest.mark.parametrize("cases", [("cfg_default", "all_options"), ("all_options", "cfg_default")])
@pytest.mark.parametrize("engine", ENGINES)
def test_mixed_call_against_reference_goldens(golden, tiny_models, engine, cases):
    """Two utterances, different text lengths and voices, one call: one runs `cfg_default`, the other `all_options` (both 6 steps).
    Their CFG windows differ (steps 0-2 / 1-3), only one has truncation, rescale and a speaker-KV scale of 1.5 on one layer that is
    undone after step 2 - so every per-item path and the "any item has CFG" row rule are on.  Row b must be row b of the golden
    the reference produced with item b's parameters for the whole batch."""
    g, m = golden, tiny_models[engine]
    lat = _mixed(m, g, [SAMPLER_CASES[c] for c in cases])
    for b, case in enumerate(cases):
        e = rms(lat[b], g[f"tinyb2.f32.euler.{case}"][b])
        bound = LAT_TOL if engine == "f32" else _bf16_row_budget(g, case, b)
        print(f"mixed {cases} {engine}: row {b} ({case}) rms {e:.3e} bound {bound:.3e}")
        assert e < bound, (b, case, e, bound)


# ------------------------------------------------------------------------------------------------ 2. uniform items == existing call
@pytest.mark.parametrize("case,ts", [(c, 32) for c in SAMPLER_CASES] + [("all_options", 28)])
@pytest.mark.parametrize("engine", ENGINES)
def test_uniform_items_equal_the_existing_call_bit_for_bit(golden, tiny_models, engine, case, ts):
    """ts = 28: 7 speaker keys, not a multiple of a 16-byte vector of either type - the per-item KV scaling takes its row tails."""
    g, m = golden, tiny_models[engine]
    want = _uniform(m, g, SAMPLER_CASES[case], ts)
    got = _mixed(m, g, [SAMPLER_CASES[case]] * 2, ts)
    assert torch.equal(got, want)
    assert torch.equal(_uniform(m, g, SAMPLER_CASES[case], ts), want)     # and the mixed call left nothing behind


# ------------------------------------------------------------------------------------------------ 3. per-item independence
@pytest.mark.parametrize("engine", ENGINES)
def test_items_are_independent_bit_for_bit(golden, tiny_models, engine):
    """One CFG window, no KV scaling: same geometry and launches as a uniform call, and rows are independent in every kernel, so item b
    of the mixed call is item b of the uniform batch-2 call that carries item b's parameters."""
    g, m = golden, tiny_models[engine]
    a = dict(SAMPLER_CASES["cfg_default"])
    b = dict(a, cfg_scale_text=2.5, cfg_scale_speaker=5.0, truncation_factor=0.8, rescale_k=1.2, rescale_sigma=3.0)
    mixed = _mixed(m, g, [a, b])
    ua, ub = _uniform(m, g, a), _uniform(m, g, b)
    assert torch.equal(mixed[0], ua[0]) and torch.equal(mixed[1], ub[1])
    assert not torch.equal(ua[1], ub[1])          # the parameters do matter


# ------------------------------------------------------------------------------------------------ 4. per-item KV scale
@pytest.mark.parametrize("ts", [32, 28])
@pytest.mark.parametrize("engine", ENGINES)
def test_per_item_speaker_kv_scale(golden, tiny_models, engine, ts):
    g, m = golden, tiny_models[engine]
    spk, smask, _, _ = _b2(g, ts)
    kv = m.get_kv_cache_speaker(spk, smask)
    before = [tuple(t.clone() for t in kv.layer(i)) for i in range(TINY.num_layers)]
    assert before[0][0].shape[0] == 2 and before[0][0].shape[1] == ts // 4
    sc, ml = (C.c_float * 2)(1.0, 1.5), (C.c_int32 * 2)(-1, 1)
    L.check(m._lib.echo_scale_speaker_kv_items(m._ctx, sc, ml, 2, m._stream()), m._ctx)
    after = [kv.layer(i) for i in range(TINY.num_layers)]

    def rounded(x):      # the product in fp32, rounded to the cache type (bf16 x 1.5 is exact in fp32)
        y = x * 1.5
        return y.bfloat16().float() if engine == "bf16" else y
    for i in range(TINY.num_layers):
        for t0, t1 in zip(before[i], after[i]):
            assert torch.equal(t1[0], t0[0]), f"item 0 changed in layer {i}"
            assert torch.equal(t1[1], rounded(t0[1]) if i == 0 else t0[1]), f"item 1, layer {i}"
    assert float(before[0][0][1].abs().max()) > 0
    # entries that share a slot must agree: 4 entries on 2 slots
    bad = m._lib.echo_scale_speaker_kv_items(m._ctx, (C.c_float * 4)(1.0, 1.5, 1.0, 2.0), (C.c_int32 * 4)(-1, 1, -1, 1), 4, m._stream())
    assert bad != 0 and b"share a voice slot" in m._lib.echo_last_error(m._ctx)


# ------------------------------------------------------------------------------------------------ 5. bind_voices
@pytest.mark.parametrize("engine", ENGINES)
def test_bind_voices(golden, tiny_models, engine):
    """Two voices of 8 and 5 keys (32 / 20 latents; 5 is no multiple of the 64-key tile, nor of a 16-byte vector) captured alone and
    bound as one batch-2 speaker cache: own keys bit for bit, zeros beyond; a sampler run on them agrees with the same run on a
    stacked encode of the two padded latents.  The cache holds infinities first, so a tail that is not zero-filled shows as NaN."""
    g, m = golden, tiny_models[engine]
    spk = g["tinyb2.spk"]
    lat = [spk[:1], spk[1:, :20].contiguous()]
    voices, own = [], []
    for x in lat:
        kv = m.get_kv_cache_speaker(x, torch.ones(x.shape[:2], dtype=torch.bool))
        own.append([tuple(t.clone() for t in kv.layer(i)) for i in range(TINY.num_layers)])
        voices.append(m.capture_voice(kv))
    poison = m.get_kv_cache_speaker(spk, None)                   # batch 2, 8 keys: the buffers bind_voices is about to reuse ...
    inf._multiply_kv_cache(poison, float("inf"))                 # ... hold +-inf in K, V and V^T; 0 x inf is NaN
    assert not bool(torch.isfinite(poison.layer(0)[1]).any())
    bound = m.bind_voices(voices)
    assert bound.batch == 2 and bound.mask.tolist() == [[True] * 8, [True] * 5 + [False] * 3]
    for i in range(TINY.num_layers):
        k, v = bound.layer(i)
        assert k.shape[:2] == (2, 8)
        for got, (k0, k1) in ((k, (own[0][i][0], own[1][i][0])), (v, (own[0][i][1], own[1][i][1]))):
            assert torch.equal(got[0], k0[0]) and torch.equal(got[1, :5], k1[0])
            assert bool((got[1, 5:] == 0).all())
    items = [dict(SAMPLER_CASES["cfg_default"], rng_seed=0), dict(SAMPLER_CASES["all_options"], rng_seed=0)]
    ids, tmask, x0 = g["tinyb2.ids"], g["tinyb2.tmask"].bool(), g["tinyb2.x0"]
    got = inf.sample_euler_items(m, None, None, ids, tmask, items, sequence_length=32, x_init=x0, speaker_kv=voices)
    assert bool(torch.isfinite(got).all())
    if engine == "f32":
        pad = torch.zeros((2, 32, 80))
        pad[0], pad[1, :20] = lat[0][0], lat[1][0]
        smask = torch.ones((2, 32), dtype=torch.bool)
        smask[1, 20:] = False
        want = inf.sample_euler_items(m, pad, smask, ids, tmask, items, sequence_length=32, x_init=x0)
        e = rms(got, want)
        print(f"bound voices vs stacked encode, fp32: rms {e:.3e}")
        assert e < LAT_TOL, e
    for v in voices:
        v.close()


# ------------------------------------------------------------------------------------------------ 6. ABI errors
def test_abi_errors_return_a_status_and_a_message(golden, tiny_models):
    g, m = golden, tiny_models["f32"]
    lib, ctx, st = m._lib, m._ctx, m._stream()
    spk, smask, ids, tmask = _b2(g)
    items = [dict(SAMPLER_CASES["cfg_default"], rng_seed=0)] * 2
    arr, temb, keep = inf.build_sampler_items(m, items)
    m.get_kv_cache_text(ids, tmask)
    m.get_kv_cache_speaker(spk, smask)
    temb_dev = temb.to(DEV).contiguous()
    x0 = g["tinyb2.x0"].to(DEV).contiguous()
    out = torch.empty_like(x0)

    def call(B=2, item_arr=arr):
        p = L.EchoSamplerParams()
        p.B, p.S, p.num_steps, p.temb = B, 32, 6, temb_dev.data_ptr()
        return lib.echo_sample_euler_items(ctx, C.byref(p), item_arr, x0.data_ptr(), out.data_ptr(), st)

    def failed(status, text):
        msg = lib.echo_last_error(ctx)
        assert status != 0 and msg and text in msg, (status, msg)
    failed(call(B=1), b"batch size of the text cache")
    failed(call(item_arr=None), b"null")
    other = (L.EchoStep * 6)(*[keep[1][i] for i in range(6)])
    other[2].dt = keep[1][2].dt * 0.5
    arr2 = (L.EchoSamplerItem * 2)(arr[0], arr[1])
    arr2[1].steps = other
    failed(call(item_arr=arr2), b"dt")
    arr3 = (L.EchoSamplerItem * 2)(arr[0], arr[1])
    arr3[1].steps = None
    failed(call(item_arr=arr3), b"no step table")
    v32 = m.capture_voice(m.get_kv_cache_speaker(spk[:1], smask[:1]))
    mb = tiny_models["bf16"]
    ptrs = (C.c_void_p * 1)(v32._ptr)
    status = mb._lib.echo_voice_bind_items(mb._ctx, ptrs, 1, mb._stream())
    assert status != 0 and b"different model" in mb._lib.echo_last_error(mb._ctx)
    with pytest.raises(RuntimeError, match="different model"):
        mb.bind_voices([v32])
    v32.close()
    # the context survives: the same arguments, now valid
    m.get_kv_cache_speaker(spk, smask)
    assert call() == 0
    assert rms(out, g["tinyb2.f32.euler.cfg_default"]) < LAT_TOL


# ------------------------------------------------------------------------------------------------ 7. synthesize_many
def test_synthesize_many_equals_the_jobs_run_alone(golden, tiny_models):
    """Three jobs - different texts (one of several chunks), parameters, voices and num_steps (4 and 6: two groups) - plus one bad
    job.  Batched against sequential, as test_handler_batches_the_chunks_of_a_request compares them: same shape, RMS <= WAV_TOL."""
    from echo_tts_amd import handler as H
    m = tiny_models["f32"]
    dac = E.DAC(TINY_DAC, R.make_dac_weights(TINY_DAC, 0), device=DEV)
    pca = R.make_pca(TINY_DAC, 80, 0)
    st = E.PCAState(pca.pca_components, pca.pca_mean, pca.latent_scale)
    spk, sm = golden["tiny.spk"], golden["tiny.smask"].bool()
    bob = (golden["tinyb2.spk"][1:, :20].contiguous(), torch.ones((1, 20), dtype=torch.bool))
    voices = {"alice": (spk, sm), "bob": bob}
    long_text = ("The quick brown fox jumps over the lazy dog near the quiet river bank. " * 3 + "Then it rests for a while under the old oak tree. " * 3).strip()
    jobs = [
        {"text": long_text, "speaker_voice": "alice",
         "parameters": dict(SAMPLER_CASES["cfg_default"], sequence_length=32, seed=5, max_chars_per_chunk=90, normalize_boundaries=False)},
        {"text": "A second request, with every option set.", "speaker_voice": "bob", "seed": 7,
         "parameters": dict(SAMPLER_CASES["all_options"], sequence_length=32)},
        {"text": "No voice and fewer steps.", "parameters": dict(SAMPLER_CASES["cfg_default"], num_steps=4, cfg_scale_text=2.0, sequence_length=32, seed=3)},
        {"text": ""},
    ]
    alone_voice = [voices["alice"], voices["bob"], (None, None)]
    got = H.synthesize_many(jobs, m, dac, st, voices=voices)
    assert len(got) == 4
    assert got[3] == {"error": "Missing or invalid 'text' field (expected string)"}
    for j in range(3):
        assert "error" not in got[j], got[j].get("traceback")
        want = H.synthesize(jobs[j], m, dac, st, speaker_latent=alone_voice[j][0], speaker_mask=alone_voice[j][1])
        assert "error" not in want, want.get("traceback")
        a, b = want["audio"].float().cpu(), got[j]["audio"].float().cpu()
        assert a.shape == b.shape, (j, a.shape, b.shape)
        print(f"synthesize_many job {j}: {got[j]['chunks']} chunks, rms vs alone {rms(a, b):.3e}")
        assert rms(a, b) <= WAV_TOL, (j, rms(a, b))
        assert {k: got[j][k] for k in ("chunks", "seed", "text_length", "sample_rate")} == {k: want[k] for k in ("chunks", "seed", "text_length", "sample_rate")}
    assert got[0]["chunks"] >= 3 and got[0]["seed"] == 5 and got[1]["seed"] == 7
    unknown = H.synthesize_many([{"text": "Hi.", "speaker_voice": "carol", "parameters": {"num_steps": 4, "sequence_length": 32}}], m, dac, st, voices=voices)
    assert unknown == [{"error": "speaker_voice 'carol' not found"}]
