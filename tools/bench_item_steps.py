"""What does one step count per utterance cost, and does mixing step counts in one sampler call pay?  Full-size EchoDiT, random bf16
weights, S = 640, 768 text columns / 436 tokens, speaker references of 1280 latents (the shapes of tools/bench_stream_lengths.py).

(a) Overhead of the step-count form at equal counts.  B = 8 and 24, all items at 40 steps, caches encoded once outside the timed region;
    one timed unit = one sampler call ending in a device synchronise; the cases ALTERNATE inside every repeat:
      len       echo_sample_euler_items_len, every length 640 (code that exists without this feature)
      steps     echo_sample_euler_items_steps, every count 40, every length 640 (results must equal `len` bit for bit: checked)
    Reported: median / min / max per case, the `len` call's run-to-run spread, the difference and whether it is resolved.
(b) 4 items at 20 steps + 4 items at 40 steps:
      grouped   two calls of B = 4 (echo_sample_euler_items_len at 20 and at 40 steps), text and voices re-bound per call
      mixed     one call of B = 8 (echo_sample_euler_items_steps, counts 40 x 4 then 20 x 4)
    The timed unit includes binding the call's text and speaker caches, since the grouped form does that twice.  Reported: audio-seconds
    per second (one latent = 2048 samples at 44.1 kHz), the idle share of the mixed call, and the mixed call's 40-step rows against the
    grouped call's (other batch size: not equality; RMS).

    python tools/bench_item_steps.py [--steps 40] [--fast-steps 20] [--repeats 5] [--warmup 1] [--out FILE]

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

S, TT, TVALID, TS = 640, 768, 436, 1280
BASE = dict(num_steps=40, cfg_scale_text=3.0, cfg_scale_speaker=8.0, cfg_min_t=0.5, cfg_max_t=1.0, truncation_factor=None,
            rescale_k=None, rescale_sigma=None, speaker_kv_scale=None, speaker_kv_max_layers=None, speaker_kv_min_t=None)
AUDIO_S_PER_LATENT = 2048 / 44100.0


def stats(ms):
    return {"median_ms": round(statistics.median(ms), 3), "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3), "n": len(ms)}


def note(msg: str) -> None:
    print(f"[bench_item_steps] {msg}", file=sys.stderr, flush=True)


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0), r


def inputs(model, B, g):
    lz = model.config.latent_size
    ids = torch.zeros((B, TT), dtype=torch.int32)
    ids[:, 1:TVALID] = torch.randint(32, 127, (B, TVALID - 1), generator=g, dtype=torch.int32)
    tmask = torch.zeros((B, TT), dtype=torch.bool)
    tmask[:, :TVALID] = True
    spk = torch.randn((B, TS, lz), generator=g).to(model.device, model.dtype)
    smask = torch.ones((B, TS), dtype=torch.bool)
    x0 = torch.randn((B, S, lz), generator=g).to(model.device)
    return ids.to(model.device), tmask.to(model.device), spk, smask, x0


def steps_form_cost(model, inf, B, N, warmup, repeats, g):
    ids, tmask, spk, smask, x0 = inputs(model, B, g)
    model.get_kv_cache_text(ids, tmask)
    model.get_kv_cache_speaker(spk, smask)
    arr, temb, _keep = inf.build_sampler_items(model, [dict(BASE, num_steps=N, rng_seed=0)] * B)
    cases = {"len": lambda: inf.run_euler_items(model, x0, arr, N, temb, lengths=[S] * B),
             "steps": lambda: inf.run_euler_items(model, x0, arr, N, None, lengths=[S] * B, item_steps=[N] * B)}
    times, last = {k: [] for k in cases}, {}
    for r in range(warmup + repeats):
        for name, fn in cases.items():
            ms, last[name] = timed(fn)
            note(f"(a) B={B} {name} run {r}: {ms:.1f} ms")
            if r >= warmup:
                times[name].append(ms)
    ref = stats(times["len"])
    spread = ref["max_ms"] - ref["min_ms"]
    d = statistics.median(times["steps"]) - ref["median_ms"]
    return {"B": B, "S": S, "num_steps": N, "len": ref, "steps": stats(times["steps"]), "len_spread_ms": round(spread, 3),
            "len_spread_pct": round(100 * spread / ref["median_ms"], 3), "steps_minus_len_ms": round(d, 3),
            "steps_minus_len_pct": round(100 * d / ref["median_ms"], 3), "difference_resolved": bool(abs(d) > spread),
            "steps_equals_len_bitwise": bool(torch.equal(last["steps"], last["len"])), "finite": bool(torch.isfinite(last["steps"]).all()),
            "ms_per_item": round(ref["median_ms"] / B, 2)}


def mixed_vs_grouped(model, inf, n_each, N, n_fast, warmup, repeats, g):
    B = 2 * n_each
    ids, tmask, spk, smask, x0 = inputs(model, B, g)
    counts = [N] * n_each + [n_fast] * n_each            # longest first: equal counts adjacent
    items = [dict(BASE, num_steps=n, rng_seed=b) for b, n in enumerate(counts)]

    def call(rows, item_steps, compact=False):
        model.get_kv_cache_text(ids[rows], tmask[rows])
        model.get_kv_cache_speaker(spk[rows], smask[rows])
        its = [items[b] for b in rows]
        arr, temb, _keep = inf.build_sampler_items(model, its)
        if item_steps:
            return inf.run_euler_items(model, x0[rows], arr, max(counts[b] for b in rows), None, lengths=[S] * len(rows),
                                       item_steps=[counts[b] for b in rows], compact_rows=compact)
        return inf.run_euler_items(model, x0[rows], arr, counts[rows[0]], temb, lengths=[S] * len(rows))

    slow, fast = list(range(n_each)), list(range(n_each, B))
    cases = {"grouped": lambda: torch.cat([call(slow, False), call(fast, False)], 0),
             "mixed": lambda: call(slow + fast, True),
             "compact": lambda: call(slow + fast, True, compact=True)}      # the mixed call with compacted row sets
    times, last, row_forwards = {k: [] for k in cases}, {}, {}
    for r in range(warmup + repeats):
        for name, fn in cases.items():
            ms, last[name] = timed(fn)
            row_forwards[name] = model.last_row_forwards()       # grouped: of its second call only
            note(f"(b) {name} run {r}: {ms:.1f} ms")
            if r >= warmup:
                times[name].append(ms)
    audio_s = B * S * AUDIO_S_PER_LATENT
    out = {"items": f"{n_each} x {N} steps + {n_each} x {n_fast} steps", "S": S, "audio_s": round(audio_s, 2),
           "idle_share_mixed": round(sum(N - n for n in counts) / float(B * N), 4)}
    for name in cases:
        st = stats(times[name])
        out[name] = dict(st, audio_s_per_s=round(audio_s / (st["median_ms"] * 1e-3), 2))
    gm, mm = out["grouped"]["median_ms"], out["mixed"]["median_ms"]
    out["mixed_minus_grouped_ms"] = round(mm - gm, 3)
    out["mixed_minus_grouped_pct"] = round(100 * (mm - gm) / gm, 3)
    out["grouped_spread_ms"] = round(out["grouped"]["max_ms"] - out["grouped"]["min_ms"], 3)
    d = (last["mixed"].float() - last["grouped"].float())
    out["mixed_vs_grouped_rms"] = [round(float(d[b].pow(2).mean().sqrt()), 6) for b in range(B)]
    out["latent_rms"] = round(float(last["grouped"].float().pow(2).mean().sqrt()), 4)
    out["finite"] = bool(torch.isfinite(last["mixed"]).all())
    cm = out["compact"]["median_ms"]
    out["compact_minus_grouped_ms"] = round(cm - gm, 3)
    out["compact_minus_grouped_pct"] = round(100 * (cm - gm) / gm, 3)
    out["compact_minus_mixed_pct"] = round(100 * (cm - mm) / mm, 3)
    dc = (last["compact"].float() - last["grouped"].float())
    out["compact_vs_grouped_rms"] = [round(float(dc[b].pow(2).mean().sqrt()), 6) for b in range(B)]
    out["row_forwards"] = {"mixed": row_forwards["mixed"], "compact": row_forwards["compact"]}
    out["compact_finite"] = bool(torch.isfinite(last["compact"]).all())
    return out


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--fast-steps", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=None)
    ap.add_argument("--only-mixed", action="store_true", help="case (b) alone: grouped / mixed / compacted")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/bench_item_steps.py needs an MI355X: the hot path has no CPU fallback")
    import echo_tts_amd as E
    from echo_tts_amd import inference as inf
    from echo_tts_amd.weights import random_dit_state
    device = torch.device("cuda:0")
    torch.cuda.set_device(device)
    cfg = E.EchoDiTConfig()
    model = E.EchoDiT(cfg, random_dit_state(cfg, device, torch.bfloat16, seed=0, with_blockwise=False), dtype=torch.bfloat16, device=device)
    torch.cuda.empty_cache()
    note("model ready")
    g = torch.Generator().manual_seed(1234)
    cost = [] if args.only_mixed else [steps_form_cost(model, inf, B, args.steps, args.warmup, args.repeats, g) for B in (8, 24)]
    mix = mixed_vs_grouped(model, inf, 4, args.steps, args.fast_steps, args.warmup, args.repeats, g)
    rec = {"tool": "tools/bench_item_steps.py", "device": torch.cuda.get_device_name(0),
           "workload": f"full-size EchoDiT, random bf16 weights, S = {S}, {TVALID} of {TT} text tokens, speaker references of {TS} latents; "
                       f"{args.warmup} warm-up + {args.repeats} timed repeats, cases alternating inside a repeat, host clock around a device synchronise",
           "steps_form_cost": cost, "mixed_vs_grouped": mix}
    print(json.dumps(rec))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w", encoding="utf-8") as f:
            f.write(json.dumps(rec, indent=1) + "\n")


if __name__ == "__main__":
    main()
