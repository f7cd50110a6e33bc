"""What do per-utterance sampler parameters and per-utterance cached voices cost?  C2 shapes (full-size EchoDiT, random bf16
weights, S = 640, 40 Euler steps, 768 text columns / 436 tokens), B = 24 utterances per sampler call.

Sampler (the KV caches are encoded once, outside the timed region; one timed unit = one sampler call ending in a device
synchronise; the three cases ALTERNATE inside every repeat, so drift of the box hits them alike):
  uniform   echo_sample_euler, one parameter set per call (what bench.py times)
  items     echo_sample_euler_items, the same parameter set on every item (results must equal `uniform` bit for bit: checked)
  distinct  echo_sample_euler_items, 24 different parameter sets inside one CFG window (scales, truncation, rescale)
Reported: median / min / max per case, the uniform call's run-to-run spread, and the overhead of the two mixed cases over it.

cfg_off among CFG items: half of the items have no CFG window (cfg_min_t above 1), the others BASE's; the rectangular
echo_sample_euler_items call pays 3 rows for everybody while the window is open, the compacted call (compact_rows=True) 1 row for a cfg_off
item:
  cfgoff_rect     echo_sample_euler_items            cfgoff_compact  echo_sample_euler_items_compact
Reported with the row-forwards of both calls; `--only-cfg-off` runs this section alone.

Voices (24 voices of 1280..2560 speaker latents, captured once):
  bind      EchoDiT.bind_voices: one gather kernel into a batch-24 speaker cache
  encode    get_kv_cache_speaker on the 24 stacked, padded latents with masks (what a server without the per-voice cache runs)

    python tools/bench_mixed_batch.py [--batch 24] [--steps 40] [--repeats 5] [--warmup 1] [--out FILE]

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

S, TT, TVALID, TS = 640, 768, 436, 2560
BASE = dict(num_steps=40, cfg_scale_text=3.0, cfg_scale_speaker=8.0, cfg_min_t=0.5, cfg_max_t=1.0, truncation_factor=None,
            rescale_k=None, rescale_sigma=None, speaker_kv_scale=None, speaker_kv_max_layers=None, speaker_kv_min_t=None)


def distinct_items(n: int, num_steps: int):
    """n different parameter sets that share BASE's CFG window (so the row set per step is the uniform call's)"""
    out = []
    for b in range(n):
        it = dict(BASE, num_steps=num_steps, cfg_scale_text=1.5 + 0.125 * b, cfg_scale_speaker=4.0 + 0.25 * b, rng_seed=b)
        if b % 2:
            it["truncation_factor"] = 0.7 + 0.01 * b
        if b % 3:
            it.update(rescale_k=1.1 + 0.01 * b, rescale_sigma=3.0)
        out.append(it)
    return out


def stats(ms):
    return {"median_ms": round(statistics.median(ms), 3), "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3), "n": len(ms)}


def note(msg: str) -> None:
    print(f"[bench_mixed_batch] {msg}", file=sys.stderr, flush=True)


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0), r


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=24)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=None)
    ap.add_argument("--only-cfg-off", action="store_true", help="the cfg_off-among-CFG section alone")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/bench_mixed_batch.py needs an MI355X: the hot path has no CPU fallback")
    import echo_tts_amd as E
    from echo_tts_amd import inference as inf
    from echo_tts_amd.weights import random_dit_state
    device = torch.device("cuda:0")
    torch.cuda.set_device(device)
    B, N = args.batch, args.steps
    cfg = E.EchoDiTConfig()
    model = E.EchoDiT(cfg, random_dit_state(cfg, device, torch.bfloat16, seed=0), dtype=torch.bfloat16, device=device)
    torch.cuda.empty_cache()
    note("model ready")
    g = torch.Generator().manual_seed(1234)
    ids = torch.zeros((B, TT), dtype=torch.int32)
    ids[:, 1:TVALID] = torch.randint(32, 127, (B, TVALID - 1), generator=g, dtype=torch.int32)
    tmask = torch.zeros((B, TT), dtype=torch.bool)
    tmask[:, :TVALID] = True
    spk = torch.randn((B, TS, cfg.latent_size), generator=g)
    lens = [TS - 4 * (320 * b // max(1, B - 1)) for b in range(B)]          # 2560 .. 1280 latents, multiples of the patch
    smask = torch.zeros((B, TS), dtype=torch.bool)
    for b, n in enumerate(lens):
        smask[b, :n] = True
    x0 = torch.randn((B, S, cfg.latent_size), generator=g).to(device)

    # ------------------------------------------------------------------ cfg_off items among CFG items: rectangular vs compacted rows
    kw = dict(BASE, num_steps=N)
    model.get_kv_cache_text(ids, tmask)
    model.get_kv_cache_speaker(spk, smask)
    off_items = [dict(kw, rng_seed=b, cfg_min_t=1.1 if b % 2 else kw["cfg_min_t"]) for b in range(B)]
    off, off_temb, keep_off = inf.build_sampler_items(model, off_items)
    ocases = {"cfgoff_rect": lambda: inf.run_euler_items(model, x0, off, N, off_temb),
              "cfgoff_compact": lambda: inf.run_euler_items(model, x0, off, N, off_temb, compact_rows=True)}
    otimes, olast, orows = {k: [] for k in ocases}, {}, {}
    for r in range(args.warmup + args.repeats):
        for name, fn in ocases.items():
            ms, olast[name] = timed(fn)
            orows[name] = model.last_row_forwards()
            note(f"{name} run {r}: {ms:.1f} ms")
            if r >= args.warmup:
                otimes[name].append(ms)
    audio_s = B * S * 2048 / 44100.0
    cfg_off = {k: dict(stats(v), audio_s_per_s=round(audio_s / (statistics.median(v) * 1e-3), 2), row_forwards=orows[k]) for k, v in otimes.items()}
    cfg_off["items"] = f"{B - B // 2} x CFG window {kw['cfg_min_t']}..{kw['cfg_max_t']} + {B // 2} x cfg_off, {N} steps"
    cfg_off["compact_minus_rect_pct"] = round(100 * (cfg_off["cfgoff_compact"]["median_ms"] / cfg_off["cfgoff_rect"]["median_ms"] - 1), 3)
    d_off = olast["cfgoff_compact"].float() - olast["cfgoff_rect"].float()
    cfg_off["compact_vs_rect_rms_max"] = round(max(float(d_off[b].pow(2).mean().sqrt()) for b in range(B)), 6)
    cfg_off["finite"] = bool(torch.isfinite(olast["cfgoff_compact"]).all())
    if args.only_cfg_off:
        rec = {"tool": "tools/bench_mixed_batch.py", "device": torch.cuda.get_device_name(0), "cfg_off_among_cfg": cfg_off}
        print(json.dumps(rec))
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w", encoding="utf-8") as f:
                f.write(json.dumps(rec, indent=1) + "\n")
        return

    # ------------------------------------------------------------------ sampler: uniform call vs mixed call, caches in place
    steps, temb = inf.build_schedule(model, N, kw["cfg_min_t"], kw["cfg_max_t"], None, None, None, None)
    same, _, keep_same = inf.build_sampler_items(model, [dict(kw, rng_seed=0)] * B)
    dist_items = distinct_items(B, N)
    dist, _, keep_dist = inf.build_sampler_items(model, dist_items)
    cases = {
        "uniform": lambda: inf.run_euler(model, x0, steps, temb, kw["cfg_scale_text"], kw["cfg_scale_speaker"], None, None, None),
        "items": lambda: inf.run_euler_items(model, x0, same, N, temb),
        "distinct": lambda: inf.run_euler_items(model, x0, dist, N, temb),
    }
    times = {k: [] for k in cases}
    last = {}
    for r in range(args.warmup + args.repeats):
        for name, fn in cases.items():
            ms, lat = timed(fn)
            last[name] = lat
            note(f"sampler {name} run {r}: {ms:.1f} ms")
            if r >= args.warmup:
                times[name].append(ms)
    if not all(bool(torch.isfinite(v).all()) for v in last.values()):
        raise SystemExit("non-finite latents")
    uni = stats(times["uniform"])
    spread = uni["max_ms"] - uni["min_ms"]
    sampler = {"uniform": uni, "items": stats(times["items"]), "distinct": stats(times["distinct"]),
               "uniform_spread_ms": round(spread, 3), "uniform_spread_pct": round(100 * spread / uni["median_ms"], 3),
               "items_equal_uniform_bitwise": bool(torch.equal(last["items"], last["uniform"]))}
    for name in ("items", "distinct"):
        d = sampler[name]["median_ms"] - uni["median_ms"]
        sampler[f"{name}_overhead_ms"] = round(d, 3)
        sampler[f"{name}_overhead_pct"] = round(100 * d / uni["median_ms"], 3)
        sampler[f"{name}_overhead_within_uniform_spread"] = bool(abs(d) <= spread)

    # ------------------------------------------------------------------ voices: bind 24 cached voices vs encode the stacked batch
    voices = []
    for b, n in enumerate(lens):
        h = model.get_kv_cache_speaker(spk[b:b + 1, :n].contiguous(), torch.ones((1, n), dtype=torch.bool))
        voices.append(model.capture_voice(h))
    torch.cuda.synchronize()
    note(f"{len(voices)} voices captured")
    vt = {"bind": [], "encode": []}
    vcases = {"bind": lambda: model.bind_voices(voices), "encode": lambda: model.get_kv_cache_speaker(spk, smask)}
    for r in range(args.warmup + args.repeats):
        for name, fn in vcases.items():
            ms, _ = timed(fn)
            note(f"voices {name} run {r}: {ms:.2f} ms")
            if r >= args.warmup:
                vt[name].append(ms)
    # the bound cache serves a mixed call (24 parameter sets, 24 voices): finite output, timed once for the record
    model.bind_voices(voices)
    ms_bound, lat = timed(cases["distinct"])
    # bind_GB_per_s_read_plus_write counts the voices' bytes twice: a lower bound, the cache written is padded to the longest voice
    voice_bytes = sum(v.nbytes for v in voices)
    voice = {"bind": stats(vt["bind"]), "encode": stats(vt["encode"]), "voices": B, "speaker_latents": [min(lens), max(lens)],
             "voice_cache_bytes": voice_bytes,
             "bind_GB_per_s_read_plus_write": round(2 * voice_bytes / (statistics.median(vt["bind"]) * 1e-3) / 1e9, 1),
             "speedup_bind_over_encode": round(statistics.median(vt["encode"]) / statistics.median(vt["bind"]), 2),
             "distinct_call_on_bound_voices_ms": round(ms_bound, 3), "finite": bool(torch.isfinite(lat).all())}
    for v in voices:
        v.close()
    rec = {"tool": "tools/bench_mixed_batch.py", "device": torch.cuda.get_device_name(0),
           "workload": f"C2 shapes: full-size EchoDiT, random bf16 weights, B = {B} utterances per sampler call, S = {S}, {N} Euler steps, "
                       f"{TVALID} of {TT} text tokens, speaker references of {min(lens)}..{max(lens)} latents; {args.warmup} warm-up + {args.repeats} "
                       f"timed repeats, cases alternating inside a repeat, host clock around a device synchronise",
           "sampler": sampler, "voices": voice, "cfg_off_among_cfg": cfg_off}
    line = json.dumps(rec)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w", encoding="utf-8") as f:
            f.write(json.dumps(rec, indent=1) + "\n")


if __name__ == "__main__":
    main()
