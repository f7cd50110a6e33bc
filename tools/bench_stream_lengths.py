"""What does one length per utterance cost, and what does mixing block sizes in one sampler call buy?  Full-size EchoDiT, random bf16
weights, 40 Euler steps, 768 text columns / 436 tokens (the shapes of tools/bench_stream_batch.py).

(a) Overhead of the length form at full lengths.  One block of S = 160 at start_pos = 320 with a 320-latent prefix, B = 8 and 24, caches
    encoded once outside the timed region; one timed unit = one sampler call ending in a device synchronise; the cases ALTERNATE inside
    every repeat:
      pos       echo_sample_euler_items_pos, every item at 320 (code that exists without this feature)
      len       echo_sample_euler_items_len, every item at 320 with length 160 (results must equal `pos` bit for bit: checked)
    Reported: median / min / max per case, the `pos` call's run-to-run spread, the overhead of the length form and whether it is resolved.
(b) Staggered streams.  Eight streams with block_sizes [32, 64, 128, 160, 160] (a short first block for the time to first audio, long
    ones for throughput), each opened one block after the previous one, through StreamBatcher with mix_block_sizes off, and on at
    max_pad_fraction None / 0.5 / 0.25; the four settings alternate inside every repeat.  Reported per setting: audio-seconds per second
    (one latent = 2048 samples at 44.1 kHz), sampler calls, the time from `open` to the end of the call that produced each stream's first
    block, and the padded share of the token rows the calls carried.

    python tools/bench_stream_lengths.py [--steps 40] [--repeats 5] [--warmup 1] [--streams 8] [--out FILE]

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

BLOCK, BLOCKS, TT, TVALID, TS = 160, [32, 64, 128, 160, 160], 768, 436, 1280
BASE = dict(num_steps=40, cfg_scale_text=3.0, cfg_scale_speaker=8.0, cfg_min_t=0.5, cfg_max_t=1.0, truncation_factor=None,
            rescale_k=None, rescale_sigma=None, speaker_kv_scale=None, speaker_kv_max_layers=None, speaker_kv_min_t=None)
AUDIO_S_PER_LATENT = 2048 / 44100.0
SETTINGS = [("grouped", False, None), ("mixed", True, None), ("mixed_pad_0.5", True, 0.5), ("mixed_pad_0.25", True, 0.25)]


def stats(ms):
    return {"median_ms": round(statistics.median(ms), 3), "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3), "n": len(ms)}


def note(msg: str) -> None:
    print(f"[bench_stream_lengths] {msg}", file=sys.stderr, flush=True)


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0), r


def length_form_cost(model, inf, B, N, warmup, repeats, g):
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
    cases = {"pos": lambda: inf.run_euler_items(model, x0, arr, N, temb, start_pos=[start] * B, use_latent=True),
             "len": lambda: inf.run_euler_items(model, x0, arr, N, temb, start_pos=[start] * B, use_latent=True, lengths=[BLOCK] * B)}
    times, last = {k: [] for k in cases}, {}
    for r in range(warmup + repeats):
        for name, fn in cases.items():
            ms, last[name] = timed(fn)
            note(f"(a) B={B} {name} run {r}: {ms:.1f} ms")
            if r >= warmup:
                times[name].append(ms)
    pos = stats(times["pos"])
    spread = pos["max_ms"] - pos["min_ms"]
    d = statistics.median(times["len"]) - pos["median_ms"]
    return {"B": B, "S": BLOCK, "start_pos": start, "pos": pos, "len": stats(times["len"]), "pos_spread_ms": round(spread, 3),
            "pos_spread_pct": round(100 * spread / pos["median_ms"], 3), "len_overhead_ms": round(d, 3),
            "len_overhead_pct": round(100 * d / pos["median_ms"], 3), "len_overhead_resolved": bool(abs(d) > spread),
            "len_equals_pos_bitwise": bool(torch.equal(last["len"], last["pos"])), "finite": bool(torch.isfinite(last["len"]).all())}


def staggered(model, n_streams, N, warmup, repeats, g):
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
        reqs.append(dict(text_input_ids=ids, text_mask=tmask, item_params=item, block_sizes=list(BLOCKS), rng_seed=k, speaker_voice=f"v{k}"))
    audio_s = n_streams * sum(BLOCKS) * AUDIO_S_PER_LATENT

    def run(mix, pad):
        sb = StreamBatcher(model, None, None, voices=voices, max_batch=24, mix_block_sizes=mix, max_pad_fraction=pad)
        for k in range(n_streams):      # the voices are captured here, outside the timed region: a server has them cached
            sb._voice(f"v{k}")
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        opened, first, nopen = {}, {}, 0
        while nopen < n_streams or sb.open_ids:
            if nopen < n_streams:       # one new stream per call
                opened[sb.open(**reqs[nopen])] = time.perf_counter()
                nopen += 1
            out = sb.step()
            torch.cuda.synchronize()
            now = time.perf_counter()
            for sid, _start, _blk in out:
                first.setdefault(sid, 1e3 * (now - opened[sid]))
        return 1e3 * (time.perf_counter() - t0), [first[k] for k in sorted(first)], dict(sb.stats)

    totals, firsts, last = {n: [] for n, _, _ in SETTINGS}, {}, {}
    for r in range(warmup + repeats):
        for name, mix, pad in SETTINGS:
            total, first, st = run(mix, pad)
            note(f"(b) run {r} {name}: {total:.0f} ms, {st['calls']} calls, padded share {st['pad_tokens'] / max(1, st['tokens']):.3f}")
            if r >= warmup:
                totals[name].append(total); firsts[name] = first; last[name] = st
    out = {"streams": n_streams, "blocks": list(BLOCKS), "audio_s": round(audio_s, 2)}
    for name, mix, pad in SETTINGS:
        med, st = statistics.median(totals[name]), last[name]
        out[name] = dict(stats(totals[name]), mix_block_sizes=mix, max_pad_fraction=pad, audio_s_per_s=round(audio_s / (med * 1e-3), 2),
                         calls=st["calls"], rows=st["rows"], token_rows=st["tokens"], padded_share=round(st["pad_tokens"] / max(1, st["tokens"]), 4),
                         first_block_ms_after_open=[round(v, 1) for v in firsts[name]])
    return out


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--streams", type=int, default=8)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/bench_stream_lengths.py needs an MI355X: the hot path has no CPU fallback")
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
    cost = [length_form_cost(model, inf, B, args.steps, args.warmup, args.repeats, g) for B in (8, 24)]
    stag = staggered(model, args.streams, args.steps, args.warmup, args.repeats, g)
    rec = {"tool": "tools/bench_stream_lengths.py", "device": torch.cuda.get_device_name(0),
           "workload": f"full-size EchoDiT, random bf16 weights, {args.steps} Euler steps, {TVALID} of {TT} text tokens, speaker references of {TS} "
                       f"latents; (a) one block of {BLOCK} at start 320; (b) blocks {BLOCKS} per stream; {args.warmup} warm-up + {args.repeats} timed "
                       f"repeats, cases alternating inside a repeat, host clock around a device synchronise",
           "length_form_cost": cost, "staggered_streams": stag}
    print(json.dumps(rec))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w", encoding="utf-8") as f:
            f.write(json.dumps(rec, indent=1) + "\n")


if __name__ == "__main__":
    main()
