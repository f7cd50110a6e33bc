#!/usr/bin/env python3
"""Fish S1-DAC decode A/B: the full-size seeded autoencoder, `ae_decode` of 640 latent frames, batch 1 and batch 24, in fp32 or bf16.

    python tools/bench_dac.py --dtype f32
    python tools/bench_dac.py --dtype bf16

Run both on the same box, back to back, fp32 first.  Per batch size: warm-up calls (plans, workspaces, code objects), then timed calls; prints
one JSON line with the median and the spread of the wall clock per utterance (host timer around a synchronised call) and the engine's own
HIP-event time per utterance (`get_profile().ms_total`, a separate profiled pass: profiling synchronises).  `peak_mib` is the device memory
the decode added on top of the loaded weights (torch does not see the engine's allocations: read from hipMemGetInfo).
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import echo_tts_amd as E  # noqa: E402
from echo_tts_amd.autoencoder import DACConfig  # noqa: E402
from echo_tts_amd.weights import random_dac_state  # noqa: E402


def used_mib() -> float:
    free, total = torch.cuda.mem_get_info()
    return (total - free) / 2 ** 20


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dtype", choices=("f32", "bf16"), default="f32")
    ap.add_argument("--frames", type=int, default=640)
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 24])
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--runs", type=int, default=10)
    a = ap.parse_args()
    dtype = torch.bfloat16 if a.dtype == "bf16" else torch.float32
    cfg = DACConfig()
    sd = {k: v.cpu() for k, v in random_dac_state(cfg, "cuda:0", seed=0).items()}       # the seeded checkpoint of bench.py
    dac = E.DAC(cfg, sd, device="cuda:0", dtype=dtype)
    g = torch.Generator().manual_seed(0)
    q, _ = torch.linalg.qr(torch.randn(cfg.latent_dim, cfg.latent_size, generator=g))
    st = E.PCAState(q.T.contiguous().to("cuda:0"), (0.1 * torch.randn(cfg.latent_dim, generator=g)).to("cuda:0"), 1.0)
    torch.cuda.synchronize()
    base = used_mib()
    for B in a.batches:
        lat = torch.randn((B, a.frames, 80), generator=torch.Generator().manual_seed(1)).to("cuda:0")
        for _ in range(a.warmup):
            wav = E.ae_decode(dac, st, lat)
        torch.cuda.synchronize()
        peak = used_mib() - base
        wall = []
        for _ in range(a.runs):
            t0 = time.perf_counter()
            wav = E.ae_decode(dac, st, lat)
            torch.cuda.synchronize()
            wall.append((time.perf_counter() - t0) * 1e3 / B)
        dac.set_profiling(True)
        prof = []
        for _ in range(max(3, a.runs // 2)):
            E.ae_decode(dac, st, lat)
            torch.cuda.synchronize()
            prof.append(dac.get_profile().ms_total)
        dac.set_profiling(False)
        print(json.dumps({"bench": "dac_decode", "dtype": a.dtype, "frames": a.frames, "B": B,
                          "ms_per_utt_wall_median": round(statistics.median(wall), 3), "ms_per_utt_wall_min": round(min(wall), 3),
                          "ms_per_utt_wall_max": round(max(wall), 3), "ms_per_utt_profile_median": round(statistics.median(prof), 3),
                          "runs": a.runs, "peak_mib": round(peak, 1), "wav_rms": round(float(wav.float().pow(2).mean().sqrt()), 6)}), flush=True)


if __name__ == "__main__":
    main()
