"""CPU side of the bf16 Fish S1-DAC: the dtype switch never ignores its argument, the loader's bf16 weight preparation reproduces the
reference's bf16-folded weights bit for bit, and the Python binding and the header agree on the ABI version."""
from __future__ import annotations

import os
import re

import pytest
import torch
from safetensors.torch import load_file, save_file

from tests.golden_defs import GOLD, ROOT, TINY_DAC, R

import echo_tts_amd as E  # noqa: E402
from echo_tts_amd import _lib as L  # noqa: E402
from echo_tts_amd import autoencoder as A  # noqa: E402
from echo_tts_amd import inference as inf  # noqa: E402


def test_loader_refuses_other_dtypes_before_touching_anything(tmp_path):
    """`load_fish_ae_from_path(..., dtype=torch.float16)` used to ignore `dtype` and return the fp32 autoencoder.  It must raise ValueError
    before the file, a device or the library is touched: the path does not even exist here."""
    with pytest.raises(ValueError):
        inf.load_fish_ae_from_path(str(tmp_path / "missing.safetensors"), dtype=torch.float16, config=TINY_DAC)
    with pytest.raises(ValueError):
        inf.load_fish_ae_from_path(str(tmp_path / "missing.safetensors"), dtype=torch.int8, config=TINY_DAC)


def test_loader_refuses_float16_on_a_real_file(tmp_path):
    save_file(R.make_dac_weights(TINY_DAC, 0), str(tmp_path / "dac.safetensors"))
    with pytest.raises(ValueError):
        inf.load_fish_ae_from_path(str(tmp_path / "dac.safetensors"), dtype=torch.float16, config=TINY_DAC)


def test_dac_refuses_other_dtypes():
    with pytest.raises(ValueError):
        E.DAC(TINY_DAC, R.make_dac_weights(TINY_DAC, 0), device="cuda:0", dtype=torch.float16)
    assert A.check_ae_dtype(None) is torch.float32 and A.check_ae_dtype(torch.float32) is torch.float32
    assert A.check_ae_dtype(torch.bfloat16) is torch.bfloat16


def _undo_conv(w2d: torch.Tensor, co: int, ci: int, k: int, cop: int, cip: int) -> torch.Tensor:
    """(Co_pad, k * Ci_pad) tap-major GEMM form -> (Co, Ci, k); the padding must be zeros."""
    w = w2d.reshape(cop, k, cip).permute(0, 2, 1)
    assert not bool(w[co:].any()) and not bool(w[:, ci:].any())
    return w[:co, :ci]


def _undo_convT(w2d: torch.Tensor, ci: int, co: int, stride: int, cip: int, cop: int) -> torch.Tensor:
    """(stride * Co_pad, 2 * Ci_pad) -> (Ci, Co, 2 * stride): inverse of _convT_as_gemm for k = 2 * stride."""
    w = w2d.reshape(stride, cop, 2, cip).permute(3, 1, 2, 0).flip(2).reshape(cip, cop, 2 * stride)
    assert not bool(w[ci:].any()) and not bool(w[:, co:].any())
    return w[:ci, :co]


def test_bf16_weight_preparation_reproduces_the_reference_fold_bit_for_bit():
    """Round every checkpoint tensor to bf16 first, fold weight-norm from the rounded original0 / original1 in bf16, reshape last: the three
    effective weights the reference module's `.weight` property gave (fixture) come back bit for bit once the GEMM reshape and the channel
    padding (96 -> 128, zeros) are undone.  Folding in fp32 and rounding afterwards does not reproduce them."""
    g = load_file(os.path.join(GOLD, "dac_bf16.safetensors"))
    cfg = R.DacConfig()
    sd = R.make_dac_weights(cfg, 0)
    t = dict(A.decode_tensors(A.DACConfig.from_any(cfg), sd, torch.bfloat16))
    assert all(v.dtype == torch.bfloat16 for v in t.values())
    n = len(cfg.decoder_rates)
    k7 = _undo_conv(t["decoder.model.4.block.2.block.1.conv.weight"], 96, 96, 7, 128, 128)
    assert torch.equal(k7, g["fold.k7"])
    ct = _undo_convT(t["decoder.model.4.block.1.conv.weight"], 192, 96, cfg.decoder_rates[3], 192, 128)
    assert torch.equal(ct, g["fold.convT"])
    wo = t[f"decoder.model.{n + 2}.conv.weight"]                      # (7, 128)
    assert wo.shape == (7, 128) and not bool(wo[:, 96:].any())
    assert torch.equal(wo[:, :96].t().unsqueeze(0), g["fold.out"])
    # padded vectors: zeros behind the real channels
    a = t["decoder.model.4.block.2.block.0.alpha"]
    assert a.shape == (128,) and not bool(a[96:].any())
    assert torch.equal(a[:96], sd["decoder.model.4.block.2.block.0.alpha"].flatten().bfloat16())
    # the order of operations matters: fp32 fold, then rounding, gives other bits
    late = A._fold(sd, "decoder.model.4.block.2.block.1.conv").bfloat16()
    assert not torch.equal(late, g["fold.k7"])
    # fp32 preparation is what it was: no padding, fp32 values
    f = dict(A.decode_tensors(A.DACConfig.from_any(cfg), sd, torch.float32))
    assert f["decoder.model.4.block.2.block.1.conv.weight"].shape == (96, 7 * 96)
    assert torch.equal(f["decoder.model.4.block.2.block.1.conv.weight"], A._conv_as_gemm(A._fold(sd, "decoder.model.4.block.2.block.1.conv")))


def test_abi_version_matches_the_header():
    with open(os.path.join(ROOT, "include", "echo_hip.h"), encoding="utf-8") as f:
        m = re.search(r"#define\s+ECHO_ABI_VERSION\s+(\d+)", f.read())
    assert m and int(m.group(1)) == L.ABI_VERSION == 8
