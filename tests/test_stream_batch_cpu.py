"""CPU: host side of continuous batching for streaming (per-utterance start positions): the pure selection rule `plan_stream_step`,
the stated limits of a stream (ValueError before any device work), the declarations of the two new entry points in the header and
in the ctypes table, and the validation of a `start_pos` sequence."""
import os
import re

import pytest
import torch

from echo_tts_amd import _lib as L
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


def test_plan_oldest_first():
    states = [_st(0, [8, 8], since=3), _st(1, [8, 8], since=1), _st(2, [8, 8], since=2)]
    assert SB.plan_stream_step(states, 8) == [1, 0, 2]          # the longest-waiting stream leads, the rest in arrival order
    assert SB.plan_stream_step(states, 1) == [1]
    # ties on the waiting time go to the earlier arrival
    assert SB.plan_stream_step([_st(4, [8]), _st(2, [8]), _st(3, [8])], 8)[0] == 2
    assert SB.plan_stream_step([], 8) == []


def test_plan_groups_by_block_size_and_steps():
    states = [_st(0, [16, 8]), _st(1, [8, 8]), _st(2, [16, 8], steps=4), _st(3, [16, 16]), _st(4, [8, 16], nxt=1)]
    # leader 0 wants (16, 6): stream 1 (8), stream 2 (other num_steps) stay out; 3 and 4 (its SECOND block is 16) join
    assert SB.plan_stream_step(states, 8) == [0, 3, 4]
    for s in states:
        assert s.key == (s.block_sizes[s.next_block], s.num_steps)


def test_plan_max_batch_cap():
    states = [_st(i, [8, 8]) for i in range(40)]
    assert SB.plan_stream_step(states, 5) == [0, 1, 2, 3, 4]
    assert SB.plan_stream_step(states, 1000) == list(range(32))   # clamped to what one sampler call can take (3 rows per item, 96 rows)
    assert SB.plan_stream_step(states, 0) == [0]


def test_plan_finished_stream_takes_no_row():
    states = [_st(0, [8], nxt=1), _st(1, [8, 8], nxt=1, since=5), _st(2, [8, 8], nxt=2)]
    assert states[0].finished and states[2].finished and states[0].key is None
    assert SB.plan_stream_step(states, 8) == [1]
    assert SB.plan_stream_step([states[0], states[2]], 8) == []


def test_plan_skipped_stream_is_first_next_time():
    # three streams with 8-blocks and one with a 16-block, cap 2: whoever is left out leads the next call
    states = [_st(0, [8, 8, 8]), _st(1, [16, 16]), _st(2, [8, 8, 8]), _st(3, [8, 8, 8])]
    order = []
    for tick in range(1, 7):
        picked = SB.plan_stream_step(states, 2)
        order.append(picked)
        _advance(states, picked, tick)
    assert order[0] == [0, 2]            # 1 (other size) and 3 (no room) skipped
    assert order[1] == [1]               # the earlier-arrived skipped stream leads, alone in its group
    assert order[2] == [3, 0]            # then the other one, ahead of streams that have run since
    # the plan drains: every block of every stream exactly once
    while any(not s.finished for s in states):
        picked = SB.plan_stream_step(states, 2)
        assert picked
        _advance(states, picked, 100)
    assert all(s.next_block == len(s.block_sizes) for s in states)


def _item(**over):
    return {k: v for k, v in dict(SAMPLER_CASES["cfg_default"], **over).items()}


def test_stated_limits_raise_value_errors():
    ok = _item()
    SB.check_stream_request(ok, [8, 8], 0, 4096)
    # scale given, never undone inside a block: no speaker_kv_min_t at all, or one the schedule never crosses
    for bad in (_item(speaker_kv_scale=1.5, speaker_kv_max_layers=1, speaker_kv_min_t=None),
                _item(speaker_kv_scale=1.5, speaker_kv_max_layers=1, speaker_kv_min_t=-1.0),
                _item(speaker_kv_scale=1.5, speaker_kv_max_layers=1, speaker_kv_min_t=2.0)):
        with pytest.raises(ValueError, match="never undone inside a block"):
            SB.check_stream_request(bad, [8, 8], 0, 4096)
    SB.check_stream_request(_item(speaker_kv_scale=1.5, speaker_kv_max_layers=1, speaker_kv_min_t=0.6), [8, 8], 0, 4096)   # undone at the 0.6 crossing
    with pytest.raises(ValueError, match="longer than the RoPE table allows"):
        SB.check_stream_request(ok, [8, 8], 4096 - 15, 4096)
    SB.check_stream_request(ok, [8, 8], 4096 - 16, 4096)
    with pytest.raises(ValueError, match="unknown keys"):
        SB.check_stream_request(dict(ok, rng_seed=1), [8], 0, 4096)
    with pytest.raises(ValueError, match="at least one block"):
        SB.check_stream_request(ok, [], 0, 4096)
    # StreamBatcher.open runs the same checks before it touches the model (a stand-in without a device)
    class NoModel:
        MAX_POS = 64
    sb = SB.StreamBatcher(NoModel(), None, None)
    ids = torch.zeros((1, 8), dtype=torch.int32)
    with pytest.raises(ValueError, match="longer than the RoPE table allows"):
        sb.open(ids, None, ok, [8, 8], 0, continuation_latent=torch.zeros((1, 56, 80)))
    with pytest.raises(ValueError, match="never undone inside a block"):
        sb.open(ids, None, _item(speaker_kv_scale=2.0), [8], 0)
    assert sb.open_ids == [] and sb.step() == []


def test_new_entry_points_are_declared():
    header = open(os.path.join(ROOT, "include", "echo_hip.h"), encoding="utf-8").read()
    for name in ("echo_dit_forward_pos", "echo_sample_euler_items_pos"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
        assert name in L.SIGNATURES
    # the header's argument lists against the ctypes tables: same number of arguments, the position table where the header has it
    for name in ("echo_dit_forward_pos", "echo_sample_euler_items_pos"):
        args = re.search(name + r"\s*\(([^;]*)\)\s*;", header, flags=re.S).group(1)
        args = [a.strip() for a in re.sub(r"/\*.*?\*/", "", args, flags=re.S).split(",")]
        assert len(args) == len(L.SIGNATURES[name][1]), name
        k = [i for i, a in enumerate(args) if "item_start_pos" in a]
        assert len(k) == 1 and "const int32_t*" in args[k[0]]
        assert L.SIGNATURES[name][1][k[0]] is L.SIGNATURES["echo_dit_forward_t"][1][4]      # POINTER(c_int32)
    assert "inference_blockwise.py:59-121" in header
    m = re.search(r"#define\s+ECHO_ABI_VERSION\s+(\d+)", header)
    assert m and int(m.group(1)) == L.ABI_VERSION      # additive entry points: the version the library reports is the header's
    # existing declarations are untouched: echo_dit_forward_t still takes one scalar start_pos
    assert re.search(r"echo_dit_forward_t\(echo_ctx\* ctx, const void\* x, const void\* temb, int n_t, const int32_t\* row_t, int rows, int B, int S, int start_pos,", header)


def test_start_pos_sequence_validation():
    f = M.item_start_positions
    assert f(None, 3) is None and f(7, 3) is None and f(torch.tensor(5), 3) is None      # the reference's forms: one position per call
    assert f([0, 5, 16], 3) == [0, 5, 16]
    assert f((4,), 1) == [4]
    assert f(torch.tensor([3, 0]), 2) == [3, 0]
    assert f(torch.tensor([3, 0], dtype=torch.int32), 2) == [3, 0]
    with pytest.raises(ValueError, match="one start position per KV batch item"):
        f([0, 5], 3)
    with pytest.raises(ValueError, match="one start position per KV batch item"):
        f(torch.tensor([1, 2, 3, 4]), 3)
    with pytest.raises(ValueError, match="non-negative"):
        f([0, -1, 2], 3)
    with pytest.raises(ValueError, match="must be integers"):
        f([0, 1.5, 2], 3)
    with pytest.raises(ValueError, match="must be integers"):
        f(torch.tensor([0.0, 1.0]), 2)
