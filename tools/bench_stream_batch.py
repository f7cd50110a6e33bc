"""What does one start position per utterance cost, and what does batching staggered streams buy?  C4 shapes (full-size EchoDiT, random
bf16 weights, blockwise generation with blocks of 160 latents, four blocks per stream, 40 Euler steps, 768 text columns / 436 tokens).

(a) Cost of the table form.  One block at start_pos = 320 with a 320-latent prefix, B = 8 and 24, caches encoded once outside the timed
    region; one timed unit = one sampler call ending in a device synchronise; the two cases ALTERNATE inside every repeat:
      uniform   echo_sample_euler_items at start_pos = 320 (code that exists without this feature)
      table     echo_sample_euler_items_pos with every item at 320 (results must equal `uniform` bit for bit: checked)
    Reported: median / min / max per case, the uniform call's run-to-run spread, the overhead of the table form over it.
(b) Eight streams, each opened one block after the previous one, through StreamBatcher (timing on: it synchronises around the encode
    and the sampler part of every call), against the same eight streams run one after another through sample_blockwise_stream.
    Reported: audio-seconds per second (one latent = 2048 samples at 44.1 kHz), time to first block per stream (from the moment the
    stream was opened to the end of the call that produced its first block; sequential: from the start of the whole run, since stream k
    waits for the streams before it), and the share of StreamBatcher's time spent re-encoding texts and prefixes and binding voices.

    python tools/bench_stream_batch.py [--steps 40] [--repeats 5] [--warmup 1] [--streams 8] [--out FILE]

Prints one JSON record (and writes it to --out).  Needs the MI355X: there is no CPU path."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BLOCK, NBLOCKS, TT, TVALID, TS = 160, 4, 768, 436, 1280
BASE = dict(num_steps=40, cfg_scale_text=3.0, cfg_scale_speaker=8.0, cfg_min_t=0.5, cfg_max_t=1.0, truncation_factor=None,
            rescale_k=None, rescale_sigma=None, speaker_kv_scale=None, speaker_kv_max_layers=None, speaker_kv_min_t=None)
AUDIO_S_PER_LATENT = 2048 / 44100.0


def stats(ms):
    return {"median_ms": round(statistics.median(ms), 3), "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3), "n": len(ms)}


def note(msg: str) -> None:
    print(f"[bench_stream_batch] {msg}", file=sys.stderr, flush=True)


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0), r


def table_cost(model, inf, B, N, warmup, repeats, g):
    lz = model.config.latent_size
    start = 2 * BLOCK
    ids = torch.zeros((B, TT), dtype=torch.int32)
    ids[:, 1:TVALID] = torch.randint(32, 127, (B, TVALID - 1), generator=g, dtype=torch.int32)
    tmask = torch.zeros((B, TT), dtype=torch.bool)
    tmask[:, :TVALID] = True
    model.get_kv_cache_text(ids, tmask)
    model.get_kv_cache_speaker(torch.randn((B, TS, lz), generator=g), torch.ones((B, TS), dtype=torch.bool))
    model.get_kv_cache_latent(torch.randn((B, start, lz), generator=g))
    x0 = torch.randn((B, BLOCK, lz), generator=g).to(model.device)
    arr, temb, _keep = inf.build_sampler_items(model, [dict(BASE, num_steps=N, rng_seed=0)] * B)
    cases = {"uniform": lambda: inf.run_euler_items(model, x0, arr, N, temb, start_pos=start, use_latent=True),
             "table": lambda: inf.run_euler_items(model, x0, arr, N, temb, start_pos=[start] * B, use_latent=True)}
    times, last = {k: [] for k in cases}, {}
    for r in range(warmup + repeats):
        for name, fn in cases.items():
            ms, last[name] = timed(fn)
            note(f"(a) B={B} {name} run {r}: {ms:.1f} ms")
            if r >= warmup:
                times[name].append(ms)
    uni = stats(times["uniform"])
    spread = uni["max_ms"] - uni["min_ms"]
    d = statistics.median(times["table"]) - uni["median_ms"]
    return {"B": B, "start_pos": start, "uniform": uni, "table": stats(times["table"]), "uniform_spread_ms": round(spread, 3),
            "uniform_spread_pct": round(100 * spread / uni["median_ms"], 3), "table_overhead_ms": round(d, 3),
            "table_overhead_pct": round(100 * d / uni["median_ms"], 3), "table_overhead_within_uniform_spread": bool(abs(d) <= spread),
            "table_equals_uniform_bitwise": bool(torch.equal(last["table"], last["uniform"])),
            "finite": bool(torch.isfinite(last["table"]).all())}


def staggered(model, n_streams, N, warmup, repeats, g):
    from echo_tts_amd import inference_blockwise as IB
    from echo_tts_amd.stream_batch import StreamBatcher
    lz = model.config.latent_size
    item = dict(BASE, num_steps=N)
    reqs, voices = [], {}
    for k in range(n_streams):
        ids = torch.zeros((1, TT), dtype=torch.int32)
        ids[:, 1:TVALID] = torch.randint(32, 127, (1, TVALID - 1), generator=g, dtype=torch.int32)
        tmask = torch.zeros((1, TT), dtype=torch.bool)
        tmask[:, :TVALID] = True
        voices[f"v{k}"] = (torch.randn((1, TS, lz), generator=g), torch.ones((1, TS), dtype=torch.bool))
        reqs.append(dict(text_input_ids=ids, text_mask=tmask, item_params=item, block_sizes=[BLOCK] * NBLOCKS, rng_seed=k, speaker_voice=f"v{k}"))
    audio_s = n_streams * NBLOCKS * BLOCK * AUDIO_S_PER_LATENT

    def batched():
        sb = StreamBatcher(model, None, None, voices=voices, max_batch=24)
        sb.timing = True
        for k in range(n_streams):      # the voices are captured here, outside the timed region: a server has them cached
            sb._voice(f"v{k}")
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        opened, first, nopen = {}, {}, 0
        while nopen < n_streams or sb.open_ids:
            if nopen < n_streams:       # one new stream per block interval
                opened[sb.open(**reqs[nopen])] = time.perf_counter()
                nopen += 1
            out = sb.step()
            torch.cuda.synchronize()
            now = time.perf_counter()
            for sid, _start, _blk in out:
                first.setdefault(sid, 1e3 * (now - opened[sid]))
        total = 1e3 * (time.perf_counter() - t0)
        return total, sorted(first.values()), dict(sb.stats)

    def sequential():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        first = []
        for r in reqs:
            spk, sm = voices[r["speaker_voice"]]
            kw = dict(item)
            for bi, _ in enumerate(IB.sample_blockwise_stream(model, spk.to(model.dtype), sm, r["text_input_ids"], r["text_mask"], r["rng_seed"],
                                                              [BLOCK] * NBLOCKS, **kw)):
                if bi == 0:
                    torch.cuda.synchronize()
                    first.append(1e3 * (time.perf_counter() - t0))
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0), first

    tb, ts_, ftb, fts, st_last = [], [], None, None, None
    for r in range(warmup + repeats):
        total_b, first_b, st = batched()
        total_s, first_s = sequential()
        note(f"(b) run {r}: batcher {total_b:.0f} ms ({st['calls']} calls, encode {st['ms_encode']:.0f} ms, sample {st['ms_sample']:.0f} ms), sequential {total_s:.0f} ms")
        if r >= warmup:
            tb.append(total_b); ts_.append(total_s); ftb, fts, st_last = first_b, first_s, st
    mb, ms_ = statistics.median(tb), statistics.median(ts_)
    return {"streams": n_streams, "blocks": [BLOCK] * NBLOCKS, "audio_s": round(audio_s, 2),
            "batcher": dict(stats(tb), audio_s_per_s=round(audio_s / (mb * 1e-3), 2), calls=st_last["calls"], rows=st_last["rows"],
                            ms_encode_texts_prefixes_voices=round(st_last["ms_encode"], 1), ms_sampler=round(st_last["ms_sample"], 1),
                            encode_share_pct=round(100 * st_last["ms_encode"] / max(1e-9, st_last["ms_encode"] + st_last["ms_sample"]), 2),
                            first_block_ms_after_open=[round(v, 1) for v in ftb]),
            "sequential": dict(stats(ts_), audio_s_per_s=round(audio_s / (ms_ * 1e-3), 2), first_block_ms_after_run_start=[round(v, 1) for v in fts]),
            "speedup": round(ms_ / mb, 3)}


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--streams", type=int, default=8)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/bench_stream_batch.py needs an MI355X: the hot path has no CPU fallback")
    import echo_tts_amd as E
    from echo_tts_amd import inference as inf
    from echo_tts_amd.weights import random_dit_state
    device = torch.device("cuda:0")
    torch.cuda.set_device(device)
    cfg = E.EchoDiTConfig()
    model = E.EchoDiT(cfg, random_dit_state(cfg, device, torch.bfloat16, seed=0, with_blockwise=True), dtype=torch.bfloat16, device=device)
    torch.cuda.empty_cache()
    note("model ready")
    g = torch.Generator().manual_seed(1234)
    table = [table_cost(model, inf, B, args.steps, args.warmup, args.repeats, g) for B in (8, 24)]
    stag = staggered(model, args.streams, args.steps, args.warmup, args.repeats, g)
    rec = {"tool": "tools/bench_stream_batch.py", "device": torch.cuda.get_device_name(0),
           "workload": f"C4 shapes: full-size EchoDiT, random bf16 weights, blocks of {BLOCK} latents x {NBLOCKS}, {args.steps} Euler steps, {TVALID} of {TT} "
                       f"text tokens, speaker references of {TS} latents; {args.warmup} warm-up + {args.repeats} timed repeats, cases alternating inside a "
                       f"repeat, host clock around a device synchronise",
           "table_form_cost": table, "staggered_streams": stag}
    print(json.dumps(rec))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w", encoding="utf-8") as f:
            f.write(json.dumps(rec, indent=1) + "\n")


if __name__ == "__main__":
    main()
