"""Streaming DAC decode: one `DACStream.push` per stream against one `DACStream.push_many` for all.

Full-size seeded Fish S1-DAC, fp32 and bf16.  Cases: n streams x new block x history; one step = every stream receives its block.  Both forms
run in ONE process and alternate inside every repeat (push loop, push_many, push loop, ...), each on fresh streams that already hold `history`
frames, so that drift of the box hits both alike.  Figures per case and form: ms per step (median and min..max over the repeats) and ms until
the FIRST stream's chunk is complete (the push loop: after its first push; push_many: the whole call).  `--shapes` reruns one case per form
under engine profiling with ECHO_PROFILE_SHAPES=1 (per-shape GEMM times on stderr).  Prints one JSON document.

    python tools/bench_stream_decode.py [--repeats 5] [--out profiles/pr_stream_decode_batch.json] [--shapes]"""
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

import echo_tts_amd as E  # noqa: E402
from echo_tts_amd.autoencoder import DACConfig, DACStream  # noqa: E402
from echo_tts_amd.weights import random_dac_state  # noqa: E402

DEV = "cuda:0"


def _streams(dac, st, n, history, gen):
    out = []
    for _ in range(n):
        s = DACStream(dac, st)
        if history:
            s.latents = torch.randn((history, 80), generator=gen).to(DEV)
            s.emitted = history
        out.append(s)
    return out


def _time_loop(streams, blocks):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    first = None
    for s, b in zip(streams, blocks):
        s.push(b)
        if first is None:
            torch.cuda.synchronize()
            first = time.perf_counter() - t0
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, first * 1e3


def _time_many(streams, blocks):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    DACStream.push_many(streams, blocks)
    torch.cuda.synchronize()
    t = (time.perf_counter() - t0) * 1e3
    return t, t


def _case(dac, st, n, block, history, repeats, gen):
    blocks = [torch.randn((block, 80), generator=gen).to(DEV) for _ in range(n)]
    res = {"loop": [], "many": []}
    for r in range(repeats + 1):                     # repeat 0 warms both forms (buffers, plans) and is dropped
        for form, fn in (("loop", _time_loop), ("many", _time_many)):
            t = fn(_streams(dac, st, n, history, gen), blocks)
            if r:
                res[form].append(t)
    out = {"n": n, "block": block, "history": history}
    for form, ts in res.items():
        step, first = [a for a, _ in ts], [b for _, b in ts]
        out[form] = {"ms_step_median": round(statistics.median(step), 3), "ms_step_min": round(min(step), 3), "ms_step_max": round(max(step), 3),
                     "ms_first_chunk_median": round(statistics.median(first), 3)}
    out["speedup_step"] = round(out["loop"]["ms_step_median"] / out["many"]["ms_step_median"], 3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--shapes", action="store_true")
    ap.add_argument("--dtypes", default="f32,bf16")
    a = ap.parse_args()
    cfg = DACConfig()
    w = {k: v.cpu() for k, v in random_dac_state(cfg, DEV, seed=0).items()}       # the seeded checkpoint of bench.py
    gen = torch.Generator().manual_seed(0)
    q, _ = torch.linalg.qr(torch.randn(cfg.latent_dim, cfg.latent_size, generator=gen))
    st = E.PCAState(q.T.contiguous().to(DEV), (0.1 * torch.randn(cfg.latent_dim, generator=gen)).to(DEV), 1.0)
    doc = {"what": "DACStream.push per stream (loop) vs DACStream.push_many (many), full-size seeded DAC, one process, forms alternate per repeat",
           "repeats": a.repeats, "cases": {}}
    for name in a.dtypes.split(","):
        dac = E.DAC(cfg, w, device=DEV, dtype=torch.bfloat16 if name == "bf16" else torch.float32)
        rows = []
        for n in (1, 8, 24):
            for block in (32, 160):
                for history in (0, 320):
                    rows.append(_case(dac, st, n, block, history, a.repeats, gen))
                    print(json.dumps(dict(rows[-1], dtype=name)), file=sys.stderr, flush=True)
        doc["cases"][name] = rows
        if a.shapes:
            os.environ["ECHO_PROFILE_SHAPES"] = "1"
            dac.set_profiling(True)
            blocks = [torch.randn((32, 80), generator=gen).to(DEV) for _ in range(8)]
            print(f"[shapes] {name}: n = 8, block 32, history 320 - one push (stream 0), then push_many", file=sys.stderr, flush=True)
            _streams(dac, st, 1, 320, gen)[0].push(blocks[0])
            print("[shapes] push_many", file=sys.stderr, flush=True)
            DACStream.push_many(_streams(dac, st, 8, 320, gen), blocks)
            dac.set_profiling(False)
            os.environ.pop("ECHO_PROFILE_SHAPES", None)
        del dac
    text = json.dumps(doc, indent=1)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
