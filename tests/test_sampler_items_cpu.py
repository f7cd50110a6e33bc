"""CPU: host side of the mixed batches (per-utterance sampler parameters and voices in one call): the ctypes layout of the new
item struct against the header's declaration, the argument checks of `sample_euler_items` (they run before any device work), and
the pure planning step of `handler.synthesize_many`."""
import ctypes
import os
import re

import pytest
import torch

from echo_tts_amd import _lib as L
from echo_tts_amd import handler as H
from echo_tts_amd import inference as inf
from tests.golden_defs import SAMPLER_CASES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _c_struct_size(body: str) -> int:
    """sizeof of a C struct of ints, floats and pointers from its declaration text (natural alignment, LP64)."""
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    off, align = 0, 1
    for decl in filter(None, (d.strip() for d in body.split(";"))):
        names = [n.strip() for n in decl.split(",")]
        first = names[0]
        pointer = "*" in first
        base = first.replace("const", "").replace("*", " ").split()[0]
        assert pointer or base in ("int", "float"), decl
        size = 8 if pointer else 4
        for _ in names:
            off = (off + size - 1) // size * size
            off += size
            align = max(align, size)
    return (off + align - 1) // align * align


def test_item_struct_size_matches_the_header():
    header = open(os.path.join(ROOT, "include", "echo_hip.h"), encoding="utf-8").read()
    m = re.search(r"typedef struct \{([^}]*)\}\s*echo_sampler_item;", header)
    assert m, "echo_sampler_item is not declared"
    assert ctypes.sizeof(L.EchoSamplerItem) == _c_struct_size(m.group(1)) == 6 * 4 + 8
    # the parser itself, on a struct whose size an existing test pins by hand (tests/test_host_cpu.py)
    m = re.search(r"typedef struct \{([^}]*)\}\s*echo_sampler_params;", header)
    assert _c_struct_size(m.group(1)) == ctypes.sizeof(L.EchoSamplerParams)
    assert "added under ABI 8" in header and "#define ECHO_ABI_VERSION 8" in header


def _items(n, **over):
    return [dict(SAMPLER_CASES["cfg_default"], rng_seed=b, **over) for b in range(n)]


def _call(items, batch=None, spk_batch=None, **kw):
    batch = len(items) if batch is None else batch
    ids = torch.zeros((batch, 8), dtype=torch.int32)
    spk = torch.zeros((batch if spk_batch is None else spk_batch, 8, 80))
    # model = None: every check below must fire before the model is touched
    return inf.sample_euler_items(None, spk, None, ids, torch.ones((batch, 8), dtype=torch.bool), items, sequence_length=32, **kw)


def test_sample_euler_items_argument_checks():
    items = _items(2)
    items[1]["num_steps"] = 4
    with pytest.raises(ValueError, match="share num_steps"):
        _call(items)
    with pytest.raises(ValueError, match="at most 32 items"):
        _call(_items(33))
    # two rows on ONE voice slot (speaker batch 1) with different speaker-KV scaling: the slot's K / V exist once
    items = _items(2)
    items[1].update(speaker_kv_scale=1.5, speaker_kv_max_layers=1, speaker_kv_min_t=0.6)
    with pytest.raises(ValueError, match="share one voice slot"):
        _call(items, spk_batch=1)
    with pytest.raises(ValueError, match="one item per text row"):
        _call(_items(2), batch=3, spk_batch=1)
    with pytest.raises(ValueError, match="unknown keys"):
        _call([dict(it, sequence_length=32) for it in _items(2)])
    with pytest.raises(ValueError, match="missing keys"):
        _call([{k: v for k, v in it.items() if k != "rng_seed"} for it in _items(2)])
    with pytest.raises(ValueError, match="one voice per text row"):
        _call(_items(2), speaker_kv=[object()])
    # what the checks accept: the same two items on two slots, and equal KV parameters on one slot
    inf.check_sampler_items(items, 2, 2)
    inf.check_sampler_items(_items(4, speaker_kv_scale=1.5, speaker_kv_max_layers=1, speaker_kv_min_t=0.6), 4, 2)
    assert set(inf.ITEM_KEYS) == set(SAMPLER_CASES["cfg_default"]) | {"rng_seed"}


LONG = ("The quick brown fox jumps over the lazy dog near the quiet river bank. " * 3 + "Then it rests for a while under the old oak tree. " * 3).strip()


def test_plan_mixed_batches():
    p6 = dict(SAMPLER_CASES["cfg_default"], sequence_length=32, max_chars_per_chunk=90)
    jobs_in = [
        {"text": LONG, "seed": 5, "parameters": dict(p6)},                                               # 6 steps, several chunks, top-level seed
        {"text": "Hello there.", "parameters": dict(p6, num_steps=4, seed=7), "speaker_voice": "alice"},  # 4 steps
        {"text": ""},                                                                                    # bad: isolated
        {"text": "Good morning to you all.", "parameters": dict(p6, seed=9, cfg_scale_text=2.0)},        # 6 steps again
        {"text": "Other length.", "parameters": dict(p6, sequence_length=48)},                            # 6 steps, other S
        {"text": "x" * 4001},
    ]
    jobs, calls = H.plan_mixed_batches(jobs_in, max_batch=3)
    assert len(jobs) == len(jobs_in)
    assert jobs[2] == {"error": "Missing or invalid 'text' field (expected string)"}
    assert jobs[5] == {"error": "Text too long: 4001 characters (max 4000)"}
    n0 = len(H.chunk_text_for_audio(LONG, 90, 10.0))
    assert n0 >= 3 and jobs[0]["pieces"] == H.chunk_text_for_audio(LONG, 90, 10.0)
    assert [j.get("seed") for j in jobs] == [5, 7, None, 9, 0, None]
    assert jobs[1]["speaker_voice"] == "alice" and jobs[0]["speaker_voice"] is None
    assert jobs[3]["item"]["cfg_scale_text"] == 2.0 and set(jobs[3]["item"]) | {"rng_seed"} == set(inf.ITEM_KEYS)
    # no call mixes num_steps or sequence_length, none exceeds max_batch, a bad job takes no row
    seen = []
    for c in calls:
        assert 1 <= len(c["rows"]) <= 3
        for r in c["rows"]:
            job = jobs[r["job"]]
            assert "error" not in job
            assert (job["item"]["num_steps"], job["sequence_length"]) == (c["num_steps"], c["sequence_length"])
            assert r["text"] == job["pieces"][r["chunk"]] and r["seed"] == job["seed"] + 1000 * r["chunk"]
            seen.append((c["num_steps"], c["sequence_length"], r["job"], r["chunk"]))
    # every chunk of every good job exactly once; inside a group: job order, then chunk order
    want = [(j, c) for j in (0, 1, 3, 4) for c in range(len(jobs[j]["pieces"]))]
    assert sorted((j, c) for _, _, j, c in seen) == want
    for key in {(a, b) for a, b, _, _ in seen}:
        rows = [(j, c) for a, b, j, c in seen if (a, b) == key]
        assert rows == sorted(rows)
    assert [(a, b) for a, b, _, _ in seen if (a, b) == (6, 32)] and {(a, b) for a, b, _, _ in seen} == {(6, 32), (4, 32), (6, 48)}
    assert len(calls) == -(-(n0 + 1) // 3) + 1 + 1
    # max_batch is clamped to what one sampler call can take
    assert all(len(c["rows"]) <= 32 for c in H.plan_mixed_batches([{"text": LONG, "parameters": {"max_chars_per_chunk": 20}}] * 8, 1000)[1])
