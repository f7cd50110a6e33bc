"""CPU: the host side of compacted row sets - row-forward arithmetic, planner behaviour, declarations, defaults."""
import ctypes as C
import inspect
import os
import re

import pytest

from echo_tts_amd import _lib as L
from echo_tts_amd import handler as H
from echo_tts_amd import inference as I
from echo_tts_amd import inference_blockwise as IB
from echo_tts_amd import model as M
from echo_tts_amd import stream_batch as SB

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("echo_op_attention_bf16_rows", "echo_dit_forward_rows", "echo_sample_euler_items_compact", "echo_debug_last_row_forwards")


def _window(n, first_half=True):
    """CFG in the first half of an n-step schedule."""
    return [i < n // 2 for i in range(n)] if first_half else [False] * n


def test_row_forwards_of_the_worked_example():
    """4 items at 40 steps + 4 at 20, CFG in the first half of each schedule: rectangular 20 x 24 + 20 x 8 = 640; two grouped calls
    4 x (10 x 3 + 10) + 4 x (20 x 3 + 20) = 480; compacted 10 x 24 + 10 x 16 + 20 x 4 = 480."""
    cfg = [_window(40)] * 4 + [_window(20)] * 4
    counts = [40] * 4 + [20] * 4
    assert I.row_forwards(cfg, counts, compact=False) == 20 * 24 + 20 * 8 == 640
    grouped = I.row_forwards(cfg[:4], counts[:4], compact=False) + I.row_forwards(cfg[4:], counts[4:], compact=False)
    assert grouped == 4 * (20 * 3 + 20) + 4 * (10 * 3 + 10) == 480
    assert I.row_forwards(cfg, counts, compact=True) == 10 * 24 + 10 * 16 + 20 * 4 == 480


def test_row_forwards_small_cases():
    assert I.row_forwards([[True, False]], None, compact=False) == 3 + 1
    assert I.row_forwards([[True, False]], None, compact=True) == 3 + 1
    # a cfg_off item among two CFG items, 2 steps, window = step 0: rectangular 9 + 3, compacted (3 + 3 + 1) + 3
    cfg = [[True, False], [True, False], [False, False]]
    assert I.row_forwards(cfg, None, compact=False) == 12
    assert I.row_forwards(cfg, None, compact=True) == 10
    # step counts: item 1 stops after one step; the listed steps beyond a count are ignored
    assert I.row_forwards(cfg, [2, 1, 2], compact=False) == 9 + 3
    assert I.row_forwards(cfg, [2, 1, 2], compact=True) == 7 + 2
    # a finished item's window does not open the CFG layout for the others
    assert I.row_forwards([[False, False, False], [False, True, True]], [3, 1], compact=False) == 2 * 3
    assert I.row_forwards([[False, False, False], [False, True, True]], [3, 1], compact=True) == 2 + 1 + 1
    with pytest.raises(ValueError):
        I.row_forwards(cfg, [2, 3, 2])
    with pytest.raises(ValueError):
        I.row_forwards(cfg, [2, 0, 2])


def _st(i, blocks, steps=6, since=0):
    return SB.StreamState(id=i, arrival=i, block_sizes=tuple(blocks), num_steps=steps, next_block=0, waiting_since=since)


def test_idle_share_and_the_planner_under_compact_rows():
    assert SB.idle_share([6, 2, 2]) == (0 + 4 + 4) / (3 * 6)
    assert SB.idle_share([6, 2, 2], compact=True) == 0
    states = [_st(0, [8], steps=6), _st(1, [8], steps=2), _st(2, [8], steps=2)]
    assert SB.plan_stream_step_mixed(states, 8, mix_steps=True, max_idle_fraction=0.25) == [0]                   # as before
    assert SB.plan_stream_step_mixed(states, 8, mix_steps=True, max_idle_fraction=0.25, compact=True) == [0, 1, 2]  # nothing rides along
    assert SB.plan_stream_step_mixed(states, 8, mix_steps=True, max_idle_fraction=0.0, compact=True) == [0, 1, 2]
    assert SB.plan_stream_step_mixed(states, 8, compact=True) == SB.plan_stream_step_mixed(states, 8) == [0]       # the key rule is unchanged
    sizes = [_st(0, [160], steps=6), _st(1, [32], steps=4), _st(2, [160], steps=4)]
    assert SB.plan_stream_step_mixed(sizes, 8, max_pad_fraction=0.3, mix_steps=True, compact=True) == [0, 2]       # the pad limit still applies


def test_new_symbols_are_declared_and_exported():
    hdr = open(os.path.join(ROOT, "include", "echo_hip.h")).read()
    assert re.search(r"#define\s+ECHO_ABI_VERSION\s+8\b", hdr) and L.ABI_VERSION == 8
    for name in NEW_SYMBOLS:
        assert re.search(r"\b(int|int64_t)\s+" + name + r"\s*\(", hdr), name
        assert name in L.SIGNATURES
    assert len(L.SIGNATURES["echo_sample_euler_items_compact"][1]) == len(L.SIGNATURES["echo_sample_euler_items_steps"][1])
    assert len(L.SIGNATURES["echo_dit_forward_rows"][1]) == len(L.SIGNATURES["echo_dit_forward_len"][1]) + 1
    assert len(L.SIGNATURES["echo_op_attention_bf16_rows"][1]) == len(L.SIGNATURES["echo_op_attention_bf16_len"][1]) + 1
    assert os.path.exists(L.LIB_PATH), "libechohip.so is not built (python echo-tts_amd/build.py)"
    lib = C.CDLL(L.LIB_PATH)          # dlopen alone: no device is touched
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), f"{name} is not exported by the built library"


def test_defaults_are_off_everywhere():
    for fn in (I.run_euler_items, I.sample_euler_items, SB.StreamBatcher.__init__, SB.stream_audio_many, IB.stream_audio_many, H.synthesize_many):
        assert inspect.signature(fn).parameters["compact_rows"].default is False, fn
    assert inspect.signature(M.EchoDiT.forward).parameters["row_item"].default is None
    assert inspect.signature(SB.idle_share).parameters["compact"].default is False
    assert inspect.signature(SB.plan_stream_step_mixed).parameters["compact"].default is False
    assert inspect.signature(I.row_forwards).parameters["compact"].default is False
    sb = SB.StreamBatcher(None, None, None)
    assert sb.compact_rows is False and sb.stats["row_forwards"] == 0


def test_compact_rows_on_an_fp8_model_is_refused_before_anything_is_queued():
    class _Fp8Model:
        fp8 = True

    with pytest.raises(L.EchoHipError, match="compact_rows.*fp8 engine"):
        SB.StreamBatcher(_Fp8Model(), None, None, compact_rows=True)
    with pytest.raises(L.EchoHipError, match="compact_rows.*fp8 engine"):
        H.synthesize_many([], _Fp8Model(), None, None, compact_rows=True)
    with pytest.raises(L.EchoHipError, match="compact_rows.*fp8 engine"):
        I.sample_euler_items(_Fp8Model(), None, None, None, None, [], compact_rows=True)
