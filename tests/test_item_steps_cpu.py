"""CPU: host side of per-utterance step counts: the validation of a step-count table, the pure planners for calls that mix
step counts (`plan_stream_step_mixed(mix_steps=True)`, `plan_mixed_batches(mix_steps=True)`), and the declaration of the entry point."""
import os
import re

import pytest
import torch

from echo_tts_amd import _lib as L
from echo_tts_amd import handler as H
from echo_tts_amd import inference as I
from echo_tts_amd import model as M
from echo_tts_amd import stream_batch as SB
from tests.golden_defs import SAMPLER_CASES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _st(i, blocks, steps=6, nxt=0, since=0):
    return SB.StreamState(id=i, arrival=i, block_sizes=tuple(blocks), num_steps=steps, next_block=nxt, waiting_since=since)


def _items(steps):
    return [dict(SAMPLER_CASES["cfg_default"], num_steps=n, rng_seed=b) for b, n in enumerate(steps)]


# ------------------------------------------------------------------------------------------------ validation
def test_check_sampler_items_steps():
    assert I.check_sampler_items_steps(_items([6, 4, 6]), 3, 3) == [6, 4, 6]
    assert I.check_sampler_items_steps(_items([6, 6, 6]), 3, 1, num_steps=[6, 4, 6]) == [6, 4, 6]      # the list replaces the items' keys
    with pytest.raises(ValueError, match="share num_steps"):                                            # the old path keeps its rule
        I.check_sampler_items(_items([6, 4, 6]), 3, 3)
    with pytest.raises(ValueError, match="a step count is below 1"):
        I.check_sampler_items_steps(_items([6, 0, 6]), 3, 3)
    with pytest.raises(ValueError, match="a step count is below 1"):
        I.check_sampler_items_steps(_items([6, 6, 6]), 3, 3, num_steps=[6, 0, 6])
    with pytest.raises(ValueError, match="above the call's num_steps"):
        I.check_sampler_items_steps(_items([6, 7, 6]), 3, 3, max_steps=6)
    assert I.check_sampler_items_steps(_items([6, 7, 6]), 3, 3) == [6, 7, 6]                            # no maximum given: the largest count is it
    nine = list(range(2, 11))
    with pytest.raises(ValueError, match="more than 8 distinct step counts"):
        I.check_sampler_items_steps(_items(nine), 9, 9)
    assert I.check_sampler_items_steps(_items(nine[:8] + [2]), 9, 9) == nine[:8] + [2]                  # 8 distinct counts are fine
    # everything else the shared check refuses is still refused
    with pytest.raises(ValueError, match="one item per text row expected"):
        I.check_sampler_items_steps(_items([6, 4]), 3, 3)
    with pytest.raises(ValueError, match="share one voice slot"):
        I.check_sampler_items_steps([dict(it, speaker_kv_scale=1.5 if b else None) for b, it in enumerate(_items([6, 4]))], 2, 1)
    # one shared voice whose KV is scaled: every item would undo the scale at its own iteration; equal counts, or a voice each, are fine
    scaled = [dict(SAMPLER_CASES["all_options"], num_steps=n, rng_seed=b) for b, n in enumerate((6, 4, 6))]
    with pytest.raises(ValueError, match="undone at different iterations"):
        I.check_sampler_items_steps(scaled, 3, 1)
    assert I.check_sampler_items_steps(scaled, 3, 3) == [6, 4, 6]
    assert I.check_sampler_items_steps(scaled, 3, 1, num_steps=[6, 6, 6]) == [6, 6, 6]


def test_step_count_table_validation():
    assert M.item_step_counts(None, 3) is None
    assert M.item_step_counts([6, 4, 6], 3, 6) == [6, 4, 6]
    assert M.item_step_counts(torch.tensor([6, 4, 6]), 3, 6) == [6, 4, 6]
    with pytest.raises(ValueError, match=r"one step count per item expected \(3\), got 2"):
        M.item_step_counts([6, 4], 3, 6)
    with pytest.raises(ValueError, match=r"one step count per item expected \(3\)"):
        M.item_step_counts(6, 3, 6)
    with pytest.raises(ValueError, match="must be integers"):
        M.item_step_counts([6, 4.5, 6], 3, 6)
    with pytest.raises(ValueError, match="must be integers"):
        M.item_step_counts([6, True, 6], 3, 6)


def test_entry_point_is_declared():
    hdr = open(os.path.join(ROOT, "include", "echo_hip.h")).read()
    assert re.search(r"\bint\s+echo_sample_euler_items_steps\s*\(", hdr)
    assert len(L.SIGNATURES["echo_sample_euler_items_steps"][1]) == len(L.SIGNATURES["echo_sample_euler_items_len"][1]) + 1
    assert re.search(r"#define\s+ECHO_ABI_VERSION\s+8\b", hdr) and L.ABI_VERSION == 8


def test_step_groups_temb_layout():
    class _Cfg:
        timestep_embed_size = 16

    class _Model:
        dtype, config = torch.float32, _Cfg()

    t = I.step_groups_temb(_Model(), [6, 4, 6, 2], 6)          # groups in order of first appearance: 6, 4, 2
    assert t.shape == (6 * 3, 16)
    t = t.reshape(6, 3, 16)
    for g, n in enumerate((6, 4, 2)):
        ts = torch.linspace(1.0, 0.0, n + 1) * 0.999
        want = M.timestep_embedding(ts[:n], 16)
        assert torch.equal(t[:n, g], want)
        assert torch.equal(t[n:, g], want[-1:].expand(6 - n, 16))      # past the group's last step: its last embedding, finite


# ------------------------------------------------------------------------------------------------ plan_stream_step_mixed
def test_mix_steps_puts_every_step_count_in_one_call():
    states = [_st(i, [8, 8], steps=n) for i, n in enumerate((6, 6, 4, 6, 4))]
    assert SB.plan_stream_step_mixed(states, 8, mix_steps=True) == [0, 1, 2, 3, 4]           # leader first, then arrival order
    assert SB.plan_stream_step_mixed(states, 8) == [0, 1, 3]                                 # the default: the leader's step count only
    assert SB.plan_stream_step_mixed(states, 8, mix_steps=False) == SB.plan_stream_step(states, 8) == [0, 1, 3]
    late = [_st(0, [8], steps=6, since=2), _st(1, [8], steps=4, since=1), _st(2, [8], steps=6, since=2)]
    assert SB.plan_stream_step_mixed(late, 8, mix_steps=True) == [1, 0, 2]                   # the leader rule is unchanged
    assert SB.plan_stream_step_mixed(late, 2, mix_steps=True) == [1, 0]
    # the pad limit still applies
    sizes = [_st(0, [160], steps=6), _st(1, [32], steps=4), _st(2, [160], steps=4)]
    assert SB.plan_stream_step_mixed(sizes, 8, max_pad_fraction=0.3, mix_steps=True) == [0, 2]


def test_max_idle_fraction():
    assert SB.idle_share([6, 2, 2]) == (0 + 4 + 4) / (3 * 6)
    states = [_st(0, [8], steps=6), _st(1, [8], steps=2), _st(2, [8], steps=2)]
    assert SB.plan_stream_step_mixed(states, 8, mix_steps=True, max_idle_fraction=0.25) == [0]      # 4 / 12 = 0.33 each time
    assert SB.plan_stream_step_mixed(states, 8, mix_steps=True, max_idle_fraction=None) == [0, 1, 2]
    assert SB.plan_stream_step_mixed(states, 8, mix_steps=True, max_idle_fraction=0.5) == [0, 1, 2]  # 0.33, then 8 / 18 = 0.44
    # a short leader: a long candidate makes the LEADER idle, and counts the same way
    short_first = [_st(0, [8], steps=2), _st(1, [8], steps=6), _st(2, [8], steps=2)]
    assert SB.plan_stream_step_mixed(short_first, 8, mix_steps=True, max_idle_fraction=0.25) == [0, 2]
    # without mix_steps the limit has nothing to act on
    assert SB.plan_stream_step_mixed(states, 8, max_idle_fraction=0.0) == [0]


def test_stream_batcher_mix_steps_needs_mix_block_sizes():
    with pytest.raises(ValueError, match="mix_steps=True requires mix_block_sizes=True"):
        SB.StreamBatcher(None, None, None, mix_steps=True)


# ------------------------------------------------------------------------------------------------ plan_mixed_batches
def _jobs_in():
    base = dict(SAMPLER_CASES["cfg_default"])
    return [
        {"text": "Short one.", "parameters": dict(base, sequence_length=64, seed=1)},
        {"text": "The long one.", "parameters": dict(base, sequence_length=640, seed=2)},
        {"text": "In between.", "parameters": dict(base, sequence_length=320, seed=3)},
        {"text": "Other steps.", "parameters": dict(base, sequence_length=640, num_steps=4, seed=4)},
    ]


def test_plan_mixed_batches_mix_steps():
    jobs_in = _jobs_in()
    jobs, calls = H.plan_mixed_batches(jobs_in, max_batch=24, mix_lengths=True, mix_steps=True)
    assert len(calls) == 1
    c = calls[0]
    assert c["item_steps"] == [6, 6, 6, 4] and c["num_steps"] == 6                 # (steps, length) descending
    assert c["lengths"] == [640, 320, 64, 640] and c["sequence_length"] == 640
    assert [r["job"] for r in c["rows"]] == [1, 2, 0, 3]
    # cut into calls after the ordering
    _, calls2 = H.plan_mixed_batches(jobs_in, max_batch=3, mix_lengths=True, mix_steps=True)
    assert [c["item_steps"] for c in calls2] == [[6, 6, 6], [4]] and [c["num_steps"] for c in calls2] == [6, 4]
    with pytest.raises(ValueError, match="mix_steps=True requires mix_lengths=True"):
        H.plan_mixed_batches(jobs_in, max_batch=24, mix_steps=True)
    assert H.plan_mixed_batches(jobs_in, 24, mix_lengths=True)[0] == jobs


def test_plan_mixed_batches_defaults_are_unchanged():
    jobs_in = _jobs_in()
    jobs_d, calls_d = H.plan_mixed_batches(jobs_in, max_batch=24)
    assert calls_d == [
        {"num_steps": 6, "sequence_length": 64, "rows": [{"job": 0, "chunk": 0, "text": "Short one.", "seed": 1}]},
        {"num_steps": 6, "sequence_length": 640, "rows": [{"job": 1, "chunk": 0, "text": "The long one.", "seed": 2}]},
        {"num_steps": 6, "sequence_length": 320, "rows": [{"job": 2, "chunk": 0, "text": "In between.", "seed": 3}]},
        {"num_steps": 4, "sequence_length": 640, "rows": [{"job": 3, "chunk": 0, "text": "Other steps.", "seed": 4}]},
    ]
    assert H.plan_mixed_batches(jobs_in, 24, mix_lengths=False, mix_steps=False) == (jobs_d, calls_d)
    _, calls_l = H.plan_mixed_batches(jobs_in, max_batch=24, mix_lengths=True)
    assert [c["num_steps"] for c in calls_l] == [6, 4] and all("item_steps" not in c for c in calls_l)
    assert calls_l[0]["lengths"] == [640, 320, 64] and [r["job"] for r in calls_l[0]["rows"]] == [1, 2, 0]
    assert H.plan_mixed_batches(jobs_in, 24, mix_lengths=True, mix_steps=False)[1] == calls_l
