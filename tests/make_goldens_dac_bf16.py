#!/usr/bin/env python3
"""Generate tests/golden/dac_bf16.safetensors by running the REFERENCE's Fish S1-DAC in bf16 (CPU), next to make_goldens.py.

    python tests/make_goldens_dac_bf16.py

The reference serves its autoencoder in bf16 (handler.py:345 -> load_fish_ae_from_hf(dtype=torch.bfloat16), inference.py:56-76): the state
dict is cast tensor by tensor, so the parameters - the weight-norm `original0` / `original1` included - end up bf16 and the effective conv
weights are folded from the rounded parameters in bf16.  This script builds the reference module the same way on the seeded weights of the
existing DAC fixtures and stores what the bf16 tests need:

* tiny config, T = 16 and full-size config, T = 8, on the EXISTING inputs `dac_tiny.z` / `.latent`, `dac_full.z` / `.latent`:
  `<tag>.bf16.post_module`, `.bf16.upsample`, `.bf16.wav`, `.bf16.ae_decode` (stored in the dtype the reference returns: bf16, `ae_decode` fp32; the tests read `.float()`);
* full-size config, T = 11 (conv rows 44 -> 352 -> 2 816 -> 11 264 -> 22 528: ragged edge tiles at every tile height in use), a new seeded z:
  `dac_full11.z`, `dac_full11.wav` (the reference's fp32 run), `dac_full11.bf16.wav`;
* the bf16-folded effective weight of three layers, read from the reference module's `.weight` property: `fold.k7` (a WNConv1d k7),
  `fold.convT` (a WNConvTranspose1d), `fold.out` (the output conv); `dac_bf16_meta.json` names the state-dict prefixes and records the floors.

`floor = rms(ref_bf16_wav - ref_f32_wav)` is the yardstick of the bf16 parity tests (1.5 x floor); the script asserts that it is usable at every
shape: 1e-3 < floor / rms(ref_f32_wav) < 5e-2.  Only tensors and JSON are written; no reference program text.
"""
from __future__ import annotations

import json
import os
import sys

import torch
from safetensors.torch import load_file, save_file

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests.make_goldens import GOLD, R, build_ref_dac, import_reference, sha  # noqa: E402
from tests.golden_defs import TINY_DAC  # noqa: E402

# the last decoder block (96 channels: the count the bf16 engine pads to its K step) - and the only one whose kernels fit a committed fixture
FOLD_LAYERS = {"fold.k7": "decoder.model.4.block.2.block.1.conv", "fold.convT": "decoder.model.4.block.1.conv"}
FULL11_SEED, FULL11_T = 17, 11


def rms(x: torch.Tensor) -> float:
    return float(x.float().pow(2).mean().sqrt())


def build_ref_dac_bf16(ref_ae, cfg, weights):
    """load_fish_ae_from_hf(dtype=torch.bfloat16): the state dict is cast tensor by tensor and assigned."""
    dac = build_ref_dac(ref_ae, cfg, weights)
    state = {k: v.to(dtype=torch.bfloat16) for k, v in weights.items()}
    dac.load_state_dict(state, strict=False, assign=True)
    # buffers that are not in the state dict (rope caches, masks) stay as the module built them: the rope cache is bf16 by construction
    # (autoencoder.py:805-813), the masks are bool
    for name, p in dac.named_parameters():
        if name in state:
            assert p.dtype == torch.bfloat16, (name, p.dtype)
    # the seeded decode-path weights carry no encoder: those (unused) parameters would stay fp32 and `DAC.dtype` - the first parameter's dtype
    # (autoencoder.py:1138), what ae_decode casts to - would read fp32.  The real checkpoint holds every parameter, so the module is bf16 throughout.
    return dac.to(torch.bfloat16).eval()


def check_floor(tag: str, wav_bf16: torch.Tensor, wav_f32: torch.Tensor, meta: dict) -> None:
    floor, level = rms(wav_bf16.float() - wav_f32), rms(wav_f32)
    meta[f"{tag}.bf16.floor"] = floor
    meta[f"{tag}.bf16.floor_rel"] = floor / level
    print(f"{tag}: floor {floor:.4e}  rms {level:.4e}  rel {floor / level:.4e}")
    assert 1e-3 < floor / level < 5e-2, (tag, floor, level)


def main():
    torch.manual_seed(0)
    torch.set_num_threads(8)
    _, ref_ae, ref_inf, _, _ = import_reference()
    meta_path = os.path.join(GOLD, "dac_bf16_meta.json")      # a file of its own: meta.json belongs to make_goldens.py and stays as it is
    meta = {}
    out = {}
    for tag, cfg, fixture in (("dac_tiny", TINY_DAC, "dac_tiny.safetensors"), ("dac_full", R.DacConfig(), "dac_full.safetensors")):
        g = load_file(os.path.join(GOLD, fixture))
        w = R.make_dac_weights(cfg, 0)
        dac = build_ref_dac_bf16(ref_ae, cfg, w)
        pca = R.make_pca(cfg, 80, seed=0)
        st = ref_inf.PCAState(pca_components=pca.pca_components, pca_mean=pca.pca_mean, latent_scale=pca.latent_scale)
        with torch.inference_mode():
            z = g[f"{tag}.z"].to(torch.bfloat16)
            zp = dac.quantizer.post_module(z)
            out[f"{tag}.bf16.post_module"] = zp.clone()
            out[f"{tag}.bf16.upsample"] = dac.quantizer.upsample(zp).clone()
            out[f"{tag}.bf16.wav"] = dac.decode_zq(z).clone()
            out[f"{tag}.bf16.ae_decode"] = ref_inf.ae_decode(dac, st, g[f"{tag}.latent"]).clone()
        check_floor(tag, out[f"{tag}.bf16.wav"], g[f"{tag}.wav"], meta)
        floor2 = rms(out[f"{tag}.bf16.ae_decode"].float() - g[f"{tag}.ae_decode"])
        meta[f"{tag}.bf16.ae_floor"] = floor2
        assert 1e-3 < floor2 / rms(g[f"{tag}.ae_decode"]) < 5e-2, (tag, floor2)
        if tag == "dac_full":
            # T = 11 on a new seeded input: fp32 and bf16 runs of the reference
            z11 = torch.randn((1, cfg.latent_dim, FULL11_T), generator=torch.Generator().manual_seed(FULL11_SEED))
            out["dac_full11.z"] = z11
            with torch.inference_mode():
                out["dac_full11.wav"] = build_ref_dac(ref_ae, cfg, w).decode_zq(z11).clone()
                out["dac_full11.bf16.wav"] = dac.decode_zq(z11.to(torch.bfloat16)).clone()
            check_floor("dac_full11", out["dac_full11.bf16.wav"], out["dac_full11.wav"], meta)
            meta["dac_full11.seed"], meta["dac_full11.T"] = FULL11_SEED, FULL11_T
            # bf16-folded effective weights, as the module's parametrization evaluates them
            n = len(cfg.decoder_rates)
            layers = dict(FOLD_LAYERS)
            layers["fold.out"] = f"decoder.model.{n + 2}.conv"
            mods = dict(dac.named_modules())
            for key, prefix in layers.items():
                wt = mods[prefix].weight.detach()
                assert wt.dtype == torch.bfloat16
                out[key] = wt.clone()
                meta[f"{key}.prefix"] = prefix
    save_file({k: v.contiguous() for k, v in out.items()}, os.path.join(GOLD, "dac_bf16.safetensors"))
    meta["dac_bf16.wav_sha"] = sha(out["dac_full11.bf16.wav"].float())
    with open(meta_path, "w", encoding="utf-8") as f:
        json.dump(meta, f, indent=1, ensure_ascii=False)
    print("dac_bf16.safetensors", os.path.getsize(os.path.join(GOLD, "dac_bf16.safetensors")))


if __name__ == "__main__":
    main()
