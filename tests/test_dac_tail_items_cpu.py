"""Host side of the batched streaming DAC decode: `autoencoder.tail_requests` states `DACStream.push`'s arithmetic once, and
the ctypes struct of `echo_dac_decode_tail_items` must have the header's layout.  No GPU."""
from __future__ import annotations

import ctypes as C
import os
import random
import re

import pytest
import torch

from tests.golden_defs import ROOT

from echo_tts_amd import _lib as L
from echo_tts_amd.autoencoder import DACStream, tail_requests


def test_tail_requests_hand_worked_cases():
    # first block: nothing emitted, nothing to re-decode, nothing to drop
    assert tail_requests([0], [32], 12) == [(32, 0, 0)]
    # a block shorter than the context: 8 emitted < 12 context -> the tail starts at frame 0 and the 8 old frames are dropped
    assert tail_requests([8], [4], 12) == [(12, 0, 8)]
    # a continuation: 100 frames exist, 32 arrive, 12 frames of context are decoded again and dropped
    assert tail_requests([100], [32], 12) == [(132, 88, 12)]
    # context 0: the tail is exactly the new frames
    assert tail_requests([100], [32], 0) == [(132, 100, 0)]
    # several streams, one context each
    assert tail_requests([0, 8, 100], [8, 8, 1], [12, 12, 3]) == [(8, 0, 0), (16, 0, 8), (101, 97, 3)]
    for bad in (([0], [0], 12), ([-1], [4], 12), ([0], [4], -1), ([0, 1], [4], 12)):
        with pytest.raises(ValueError):
            tail_requests(*bad)


class _FakeAE:
    """Records what `DACStream.push` asks of `decode_latent_tail`; returns a waveform that numbers its samples."""
    device = "cpu"

    class config:
        hop = 4

    def __init__(self):
        self.calls = []

    def set_pca(self, st):
        pass

    def decode_latent_tail(self, latents, f0):
        self.calls.append((int(latents.shape[0]), int(f0)))
        return torch.arange((latents.shape[0] - f0) * 4, dtype=torch.float32)


def test_tail_requests_agree_with_push_over_random_schedules():
    rnd = random.Random(0)
    for _ in range(200):
        ctx = rnd.choice([0, 1, 3, 12, 40])
        ae = _FakeAE()
        s = DACStream(ae, None, context=ctx)
        for _ in range(rnd.randint(1, 6)):
            n, emitted = rnd.randint(1, 50), s.emitted
            (T, f0, drop), = tail_requests([emitted], [n], ctx)
            wav = s.push(torch.zeros((n, 2)))
            assert ae.calls[-1] == (T, f0)
            assert wav.shape == (1, 1, (T - f0 - drop) * 4) == (1, 1, n * 4)
            assert float(wav[0, 0, 0]) == drop * 4          # push dropped exactly drop_frames * hop samples
            assert 0 <= f0 < T and 0 <= drop < T - f0       # what the engine call accepts


def test_tail_item_struct_has_the_headers_layout():
    with open(os.path.join(ROOT, "include", "echo_hip.h")) as f:
        text = f.read()
    m = re.search(r"typedef struct \{([^}]*)\} echo_dac_tail_item;", text)
    assert m, "echo_dac_tail_item is not declared in the header"
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        ctype, names = ("ptr", decl.rsplit("*", 1)[1]) if "*" in decl else decl.split(None, 1)
        fields += [(n.strip(), ctype) for n in names.split(",")]
    assert fields == [("latent", "ptr"), ("T", "int32_t"), ("first_frame", "int32_t"), ("drop_frames", "int32_t"), ("wav_out", "ptr")]
    got = [(n, "ptr" if t is C.c_void_p else "int32_t") for n, t in L.EchoDacTailItem._fields_]
    assert got == fields
    S = L.EchoDacTailItem
    assert C.sizeof(S) == 32 and (S.latent.offset, S.T.offset, S.first_frame.offset, S.drop_frames.offset, S.wav_out.offset) == (0, 8, 12, 16, 24)
    assert all(t is C.c_int32 for n, t in S._fields_ if n in ("T", "first_frame", "drop_frames"))
    res, args = L.SIGNATURES["echo_dac_decode_tail_items"]
    assert res is C.c_int and len(args) == 5 and args[1]._type_ is S
    assert re.search(r"#define\s+ECHO_ABI_VERSION\s+8\b", text) and L.ABI_VERSION == 8
