"""CPU: host side of per-utterance lengths: the validation of a `lengths` table, the pure planner for calls that mix block sizes
(`plan_stream_step_mixed`), `plan_mixed_batches(mix_lengths=True)`, and the declarations of the two entry points."""
import os
import re

import pytest
import torch

from echo_tts_amd import _lib as L
from echo_tts_amd import handler as H
from echo_tts_amd import model as M
from echo_tts_amd import stream_batch as SB
from tests.golden_defs import SAMPLER_CASES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _st(i, blocks, steps=6, nxt=0, since=0):
    return SB.StreamState(id=i, arrival=i, block_sizes=tuple(blocks), num_steps=steps, next_block=nxt, waiting_since=since)


def _advance(states, picked, tick):
    for s in states:
        if s.id in picked:
            s.next_block += 1
            s.waiting_since = tick


# ------------------------------------------------------------------------------------------------ validation
def test_length_table_validation():
    assert M.item_lengths(None, 3, 40) is None
    assert M.item_lengths([40, 8, 1], 3, 40) == [40, 8, 1]
    assert M.item_lengths(torch.tensor([40, 8, 1]), 3, 40) == [40, 8, 1]
    assert M.item_lengths([40.0, 8, 1], 3, 40) == [40, 8, 1]                    # integral floats are integers, as for start positions
    with pytest.raises(ValueError, match=r"one length per KV batch item expected \(3\), got 2"):
        M.item_lengths([40, 8], 3, 40)
    with pytest.raises(ValueError, match=r"one length per KV batch item expected \(3\)"):
        M.item_lengths(40, 3, 40)
    with pytest.raises(ValueError, match="must be integers"):
        M.item_lengths([40, 8.5, 1], 3, 40)
    with pytest.raises(ValueError, match="must be integers"):
        M.item_lengths(torch.tensor([40.0, 8.0, 1.0]), 3, 40)
    with pytest.raises(ValueError, match="must be integers"):
        M.item_lengths([40, True, 1], 3, 40)
    with pytest.raises(ValueError, match="a length is below 1"):
        M.item_lengths([40, 0, 1], 3, 40)
    with pytest.raises(ValueError, match="a length is above S"):
        M.item_lengths([40, 41, 1], 3, 40)
    with pytest.raises(ValueError, match="plus its length runs past the rope table"):
        M.item_lengths([40, 8, 2], 3, 40, start_positions=[0, 5, 4095], max_pos=4096)
    assert M.item_lengths([40, 8, 1], 3, 40, start_positions=[0, 5, 4095], max_pos=4096) == [40, 8, 1]     # the last legal position
    with pytest.raises(ValueError, match="plus its length runs past the rope table"):
        M.item_lengths([40, 8, 1], 3, 40, start_positions=4060, max_pos=4096)       # one int: every item starts there
    # the three refusals the engine repeats are EchoHipErrors as well: a caller that catches the engine's error catches these
    for bad, kw in (([0, 1, 1], {}), ([41, 1, 1], {}), ([2, 1, 1], dict(start_positions=[4095, 0, 0], max_pos=4096))):
        with pytest.raises(L.EchoHipError):
            M.item_lengths(bad, 3, 40, **kw)


def test_entry_points_are_declared():
    hdr = open(os.path.join(ROOT, "include", "echo_hip.h")).read()
    for name in ("echo_dit_forward_len", "echo_sample_euler_items_len"):
        assert re.search(r"\bint\s+%s\s*\(" % name, hdr), name
        assert name in L.SIGNATURES
    assert len(L.SIGNATURES["echo_dit_forward_len"][1]) == len(L.SIGNATURES["echo_dit_forward_pos"][1]) + 1
    assert len(L.SIGNATURES["echo_sample_euler_items_len"][1]) == len(L.SIGNATURES["echo_sample_euler_items_pos"][1]) + 1
    assert re.search(r"#define\s+ECHO_ABI_VERSION\s+8\b", hdr) and L.ABI_VERSION == 8


# ------------------------------------------------------------------------------------------------ plan_stream_step_mixed
def test_mixed_plan_equals_plain_plan_for_equal_block_sizes():
    for cap in (1, 2, 8, 1000):
        states = [_st(0, [8, 8], since=3), _st(1, [8, 8], since=1), _st(2, [8, 8], since=2), _st(3, [8, 8], steps=4), _st(4, [8], nxt=1)]
        assert SB.plan_stream_step_mixed(states, cap) == SB.plan_stream_step(states, cap)
        assert SB.plan_stream_step_mixed(states, cap, max_pad_fraction=0.0) == SB.plan_stream_step(states, cap)
    many = [_st(i, [8, 8]) for i in range(40)]
    assert SB.plan_stream_step_mixed(many, 1000) == SB.plan_stream_step(many, 1000) == list(range(32))
    assert SB.plan_stream_step_mixed([], 8) == []


def test_mixed_plan_shares_a_call_across_block_sizes():
    states = [_st(0, [32, 64], since=2), _st(1, [64, 128], since=1), _st(2, [160]), _st(3, [32], steps=4), _st(4, [8, 160], nxt=1, since=2)]
    # stream 2 has waited longest (since 0) and leads; 0, 1, 4 (its SECOND block, 160) follow in arrival order; other num_steps stays out
    assert SB.plan_stream_step_mixed(states, 8) == [2, 0, 1, 4]
    assert SB.plan_stream_step(states, 8) == [2, 4]                      # the plain planner: only the 160-blocks
    assert SB.plan_stream_step_mixed(states, 3) == [2, 0, 1]
    # the stream of the other step count gets its own call
    assert SB.plan_stream_step_mixed([states[3]], 8) == [3]


def test_max_pad_fraction_excludes_exactly_the_candidate_that_exceeds_it():
    def share(sizes):
        s_call = max(sizes)
        return sum(s_call - b for b in sizes) / (len(sizes) * s_call)

    states = [_st(0, [160]), _st(1, [128]), _st(2, [32]), _st(3, [64]), _st(4, [160])]
    assert SB.padded_share([160, 128, 32]) == share([160, 128, 32])
    # leader 160; +128 -> 0.1; +32 -> (0 + 32 + 128) / 480 = 0.333: over 0.3, skipped; +64 -> (32 + 96) / 480 = 0.267; +160 -> 0.2
    assert share([160, 128]) <= 0.3 < share([160, 128, 32])
    assert share([160, 128, 64]) <= 0.3 and share([160, 128, 64, 160]) <= 0.3
    assert SB.plan_stream_step_mixed(states, 8, max_pad_fraction=0.3) == [0, 1, 3, 4]
    assert SB.plan_stream_step_mixed(states, 8, max_pad_fraction=None) == [0, 1, 2, 3, 4]
    assert SB.plan_stream_step_mixed(states, 8, max_pad_fraction=0.0) == [0, 4]
    # a short leader: a long candidate would turn the LEADER's row into padding, and counts the same way
    short_first = [_st(0, [32]), _st(1, [160]), _st(2, [40])]
    assert share([32, 160]) > 0.3 >= share([32, 40])
    assert SB.plan_stream_step_mixed(short_first, 8, max_pad_fraction=0.3) == [0, 2]


def test_a_stream_skipped_twice_leads_the_third_call():
    # a pad limit of 0.15 keeps the 32- and the 64-block out of the 160s' call and out of each other's (32 / 128 = 0.25)
    states = [_st(0, [160, 160, 160]), _st(1, [160, 160, 160]), _st(2, [32, 32]), _st(3, [64, 64])]
    order = []
    for tick in range(1, 5):
        picked = SB.plan_stream_step_mixed(states, 8, max_pad_fraction=0.15)
        order.append(picked)
        _advance(states, picked, tick)
    assert order[0] == [0, 1]            # 2: 128 / 480 = 0.27, 3: 96 / 480 = 0.2: both skipped by the limit
    assert order[1] == [2]               # the earlier-arrived skipped stream leads; 3 is skipped a second time (0.25)
    assert order[2] == [3]               # skipped twice: the leader of the third call
    assert order[3] == [0, 1]            # then the streams that have run since


# ------------------------------------------------------------------------------------------------ plan_mixed_batches
def test_plan_mixed_batches_mix_lengths():
    base = dict(SAMPLER_CASES["cfg_default"])
    jobs_in = [
        {"text": "Short one.", "parameters": dict(base, sequence_length=64, seed=1)},
        {"text": "The long one.", "parameters": dict(base, sequence_length=640, seed=2)},
        {"text": "In between.", "parameters": dict(base, sequence_length=320, seed=3)},
        {"text": "Other steps.", "parameters": dict(base, sequence_length=640, num_steps=4, seed=4)},
    ]
    jobs, calls = H.plan_mixed_batches(jobs_in, max_batch=24, mix_lengths=True)
    assert [c["num_steps"] for c in calls] == [6, 4]
    assert calls[0]["lengths"] == [640, 320, 64] and calls[0]["sequence_length"] == 640         # one call, longest first
    assert [r["job"] for r in calls[0]["rows"]] == [1, 2, 0]
    assert calls[1]["lengths"] == [640] and [r["job"] for r in calls[1]["rows"]] == [3]
    # cut into calls after the ordering: close lengths share a call
    _, calls2 = H.plan_mixed_batches(jobs_in[:3] + [{"text": "Also short.", "parameters": dict(base, sequence_length=80)}], max_batch=2, mix_lengths=True)
    assert [c["lengths"] for c in calls2] == [[640, 320], [80, 64]]
    # the default is the grouping and the output as before: no "lengths" key, one call per (num_steps, sequence_length), job order
    jobs_d, calls_d = H.plan_mixed_batches(jobs_in, max_batch=24)
    assert jobs_d == jobs
    assert calls_d == [
        {"num_steps": 6, "sequence_length": 64, "rows": [{"job": 0, "chunk": 0, "text": "Short one.", "seed": 1}]},
        {"num_steps": 6, "sequence_length": 640, "rows": [{"job": 1, "chunk": 0, "text": "The long one.", "seed": 2}]},
        {"num_steps": 6, "sequence_length": 320, "rows": [{"job": 2, "chunk": 0, "text": "In between.", "seed": 3}]},
        {"num_steps": 4, "sequence_length": 640, "rows": [{"job": 3, "chunk": 0, "text": "Other steps.", "seed": 4}]},
    ]
    assert H.plan_mixed_batches(jobs_in, 24, mix_lengths=False) == (jobs_d, calls_d)
