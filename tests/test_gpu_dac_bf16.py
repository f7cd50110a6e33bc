"""The bf16 Fish S1-DAC decoder (`DAC(..., dtype=torch.bfloat16)`, the reference's own AE dtype) on the GPU.

Numerics contract: the engine fuses what eager PyTorch rounds separately, so it is not bit-comparable to the reference's bf16
run; its output must be no farther from the reference's FP32 output than 1.5 x the reference's own bf16 run is (`floor`, from committed
fixtures; no absolute term: waveforms of the seeded weights have RMS ~1e-2)."""
from __future__ import annotations

import os
import subprocess
import sys

import pytest
import torch
from safetensors.torch import load_file

pytestmark = pytest.mark.gpu

from tests.golden_defs import GOLD, ROOT, TINY_DAC, R  # noqa: E402
from tests import gpu_util as U  # noqa: E402

import echo_tts_amd as E  # noqa: E402
from echo_tts_amd.autoencoder import DACStream  # noqa: E402

DEV = U.DEV
WAV_TOL = 1e-4


def rms(a, b=None):
    d = a.float().cpu() if b is None else a.float().cpu() - b.float().cpu()
    return float(d.pow(2).mean().sqrt())


@pytest.fixture(scope="module")
def gold():
    g = {}
    for fn in ("dac_tiny.safetensors", "dac_full.safetensors", "dac_bf16.safetensors"):
        g.update(load_file(os.path.join(GOLD, fn)))
    return g


@pytest.fixture(scope="module")
def dacs():
    """One engine per (config, dtype), shared by the tests of this module."""
    out = {}
    for size, cfg in (("tiny", TINY_DAC), ("full", R.DacConfig())):
        w = R.make_dac_weights(cfg, 0)
        pca = R.make_pca(cfg, 80, 0)
        out[size] = dict(cfg=cfg, w=w, st=E.PCAState(pca.pca_components, pca.pca_mean, pca.latent_scale),
                         bf16=E.DAC(cfg, w, device=DEV, dtype=torch.bfloat16), f32=E.DAC(cfg, w, device=DEV))
    return out


def _is_bf16_valued(x: torch.Tensor) -> bool:
    return x.dtype == torch.float32 and torch.equal(x, x.bfloat16().float())


# ------------------------------------------------------------------ 1. parity with the reference
@pytest.mark.parametrize("size, tag", [("tiny", "dac_tiny"), ("full", "dac_full")])
def test_bf16_decode_within_the_reference_bf16_floor(gold, dacs, size, tag):
    d, g = dacs[size], gold
    dac = d["bf16"]
    assert dac.dtype is torch.bfloat16 and d["f32"].dtype is torch.float32
    ref32, ref16 = g[f"{tag}.wav"], g[f"{tag}.bf16.wav"].float()
    floor = rms(ref16, ref32)
    wav = dac.decode_zq(g[f"{tag}.z"])
    assert wav.shape == ref32.shape and _is_bf16_valued(wav)
    e, e16 = rms(wav, ref32), rms(wav, ref16)
    f32 = d["f32"].decode_zq(g[f"{tag}.z"])
    apart = rms(wav, f32)
    print(f"bf16 DAC {size} decode_zq: floor {floor:.3e}  engine-vs-ref-fp32 {e:.3e}  engine-vs-ref-bf16 {e16:.3e}  engine bf16-vs-fp32 {apart:.3e}")
    assert e < 1.5 * floor, (e, floor)
    assert apart > 0.1 * floor, "the bf16 decoder must not be the fp32 decoder in disguise"
    # ae_decode: PCA inverse in fp32, rounded once
    a32, a16 = g[f"{tag}.ae_decode"], g[f"{tag}.bf16.ae_decode"].float()
    afloor = rms(a16, a32)
    out = E.ae_decode(dac, d["st"], g[f"{tag}.latent"])
    ea = rms(out, a32)
    print(f"bf16 DAC {size} ae_decode: floor {afloor:.3e}  engine-vs-ref-fp32 {ea:.3e}  engine-vs-ref-bf16 {rms(out, a16):.3e}")
    assert _is_bf16_valued(out) and ea < 1.5 * afloor, (ea, afloor)


def test_bf16_decode_full_size_11_frames_ragged_tiles(gold, dacs):
    """T = 11: conv rows 44 -> 352 -> 2 816 -> 11 264 -> 22 528, a ragged edge tile at every tile height in use."""
    g, dac = gold, dacs["full"]["bf16"]
    ref32, ref16 = g["dac_full11.wav"], g["dac_full11.bf16.wav"].float()
    floor = rms(ref16, ref32)
    wav = dac.decode_zq(g["dac_full11.z"])
    e = rms(wav, ref32)
    print(f"bf16 DAC full T=11: floor {floor:.3e}  engine-vs-ref-fp32 {e:.3e}  engine-vs-ref-bf16 {rms(wav, ref16):.3e}")
    assert _is_bf16_valued(wav) and e < 1.5 * floor, (e, floor)


# ------------------------------------------------------------------ 2. kernel-level exactness of the bf16 taps-GEMM
def _conv_case(M, N, K, taps, shift, cfg, ksplit=1, store_main=1, res=False, vec_mod=0, seed=0):
    """Conv form of the bf16 DAC through echo_op_gemm(ECHO_BF16): small-integer operands (exact in bf16 and in the fp32 accumulator), channel
    counts carried at a row pitch rounded up to the 64-element K step with zero columns (the engine's layout), zero rows in front of A."""
    gen = torch.Generator().manual_seed(seed)
    Kp, Np = (K + 63) // 64 * 64, (N + 127) // 128 * 128
    front = (taps - 1) * shift
    a = torch.randint(-2, 3, (M, K), generator=gen).double()
    w = torch.randint(-1, 2, (N, taps, K), generator=gen).double()
    nv = vec_mod or N
    bias = torch.randint(-3, 4, (nv,), generator=gen).double()
    alpha = torch.tensor([0.25, 0.5, 1.0, 1.5])[torch.randint(0, 4, (nv,), generator=gen)].double()
    r = torch.randint(-4, 5, (M, N), generator=gen).double() if res else None
    # float64 evaluation: y[m][n] = sum_j a[m - (taps-1-j) * shift] . w[n][j] + bias [+ res]
    y = torch.zeros((M, N), dtype=torch.float64)
    for j in range(taps):
        off = (taps - 1 - j) * shift
        src = torch.zeros((M, K), dtype=torch.float64)
        if off < M:
            src[off:] = a[: M - off]
        y += src @ w[:, j].t()
    col = torch.arange(N) % nv
    y = y + bias[col]
    if res:
        y = y + r
    al = alpha[col]
    snake = y + (1.0 / (al + 1e-9)) * torch.sin(al * y).pow(2)
    # device operands
    A = torch.zeros((front + M, Kp), dtype=torch.bfloat16)
    A[front:, :K] = a.bfloat16()
    W = torch.zeros((Np, taps * Kp), dtype=torch.bfloat16)
    W.view(Np, taps, Kp)[:N, :, :K] = w.bfloat16()
    A, W = A.to(DEV), W.to(DEV)
    Cm = torch.full((M, N), 7.0, dtype=torch.bfloat16, device=DEV)      # sentinel: must survive store_main = 0
    if res:
        Cm = r.bfloat16().to(DEV).contiguous()                           # residual in place
    C2 = torch.zeros((M, N), dtype=torch.bfloat16, device=DEV)
    U.gemm(A, W, Cm, M=M, N=N, K=Kp, lda=Kp, ldw=taps * Kp, ldc=N, C2=C2, taps=taps, tap_base=-front, tap_shift=shift,
           bias=bias.bfloat16().to(DEV), vec_mod=vec_mod, res=Cm if res else None, ldres=N, snake_alpha=alpha.bfloat16().to(DEV),
           store_main=store_main, a_offset_elems=front * Kp, cfg=cfg, ksplit=ksplit)
    torch.cuda.synchronize()
    if store_main:
        assert torch.equal(Cm.cpu(), y.bfloat16()), f"main output differs in {int((Cm.cpu() != y.bfloat16()).sum())} places"
    elif not res:
        assert bool((Cm == 7.0).all()), "store_main = 0 must not write C"
    want = snake.bfloat16().float()
    got = C2.float().cpu()
    ulp = torch.maximum(want.abs(), torch.tensor(2.0 ** -126)).log2().floor().exp2() * 2.0 ** -7
    assert bool(((got - want).abs() <= ulp).all()), f"snake output off by more than one bf16 ulp: {float(((got - want).abs() / ulp).max()):.2f}"


# cfg: 0 / 1 = 128 x 128 (2 / 4 stages), 2 = 256 x 256, 3 = 256 x 128, 8 = 256 x 192, 9 = 384 x 96 - every tile the bf16 DAC's plan rule can pick, split-K included
@pytest.mark.parametrize("cfg, ksplit", [(9, 1), (0, 1), (1, 3), (2, 1), (3, 1)])
def test_bf16_taps_gemm_exact_k96_store_main_0(cfg, ksplit):
    """K = 96 is no multiple of the bf16 K step: carried at pitch 128 with zero columns; M = 500 leaves a ragged 384-row tile; dilation 9."""
    _conv_case(500, 96, 96, 7, 9, cfg, ksplit, store_main=0)


@pytest.mark.parametrize("cfg, ksplit", [(8, 1), (6, 1), (0, 1), (1, 2), (2, 1)])
def test_bf16_taps_gemm_exact_k192_residual_in_place(cfg, ksplit):
    _conv_case(300, 192, 192, 7, 3, cfg, ksplit, store_main=1, res=True, seed=1)
    _conv_case(300, 192, 192, 1, 0, cfg, 1, store_main=0, res=True, seed=2)      # the 1-tap conv + residual whose main output is dropped


@pytest.mark.parametrize("cfg", [8, 2, 0])
def test_bf16_taps_gemm_exact_transposed_conv_form(cfg):
    _conv_case(130, 384, 192, 2, 1, cfg, store_main=1, vec_mod=192, seed=3)


@pytest.mark.parametrize("cfg", [0, 1])
def test_bf16_taps_gemm_exact_tiny_half_step(cfg):
    """The tiny config's 32 channels: half a K step, carried at pitch 64."""
    _conv_case(40, 32, 32, 7, 1, cfg, store_main=1, seed=4)


# ------------------------------------------------------------------ 3 / 4. conv tails and reproducibility (fresh processes)
_CHILD = (
    "import sys, torch\n"
    f"sys.path.insert(0, {ROOT!r})\n"
    "import echo_tts_amd as E\n"
    "from oracle import echo_ref as R\n"
    "cfg = R.DacConfig(); w = R.make_dac_weights(cfg, 0)\n"
    "z = torch.randn((1, cfg.latent_dim, 24), generator=torch.Generator().manual_seed(7))\n"
    "dac = E.DAC(cfg, w, device='cuda:0', dtype=torch.bfloat16)\n"
    "torch.save(dac.decode_zq(z).cpu(), sys.argv[1])\n")


def test_bf16_conv_tails_equal_the_generic_tail_and_runs_reproduce(tmp_path):
    """A bf16 full-size decode of 24 frames gives the same bits with the branch-free conv tails on and off (both with the sinf Snake), and the
    default configuration gives the same bits in two fresh processes (fixed plan rule, no timing-based tuning)."""
    script = tmp_path / "decode.py"
    script.write_text(_CHILD)
    outs = {}
    for name, env in (("conv", {"ECHO_NT_CONV_TAILS": "1", "ECHO_DAC_FAST_SIN": "0"}), ("generic", {"ECHO_NT_CONV_TAILS": "0", "ECHO_DAC_FAST_SIN": "0"}),
                      ("run1", {}), ("run2", {})):
        out = tmp_path / f"{name}.pt"
        r = subprocess.run([sys.executable, str(script), str(out)], env=dict(os.environ, **env), capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        outs[name] = torch.load(out, weights_only=True)
    assert torch.equal(outs["conv"], outs["generic"])
    assert torch.equal(outs["run1"], outs["run2"])
    assert bool(torch.isfinite(outs["run1"]).all()) and rms(outs["run1"]) > 1e-3


# ------------------------------------------------------------------ 5. batch
@pytest.mark.parametrize("size, tag, B, T", [("tiny", "dac_tiny", 3, 40), ("full", "dac_full", 3, 136)])
def test_bf16_decode_batch(gold, dacs, size, tag, B, T):
    d = dacs[size]
    floor_rel = rms(gold[f"{tag}.bf16.wav"].float(), gold[f"{tag}.wav"]) / rms(gold[f"{tag}.wav"])
    lat = torch.randn((B, T, 80), generator=torch.Generator().manual_seed(11))
    lat[1] *= 3.0                                            # items of different scale: a leak between items would show
    allb = E.ae_decode(d["bf16"], d["st"], lat)
    again = E.ae_decode(d["bf16"], d["st"], lat)
    assert torch.equal(allb, again) and bool(torch.isfinite(allb).all()) and _is_bf16_valued(allb)
    for b in range(B):
        one = E.ae_decode(d["bf16"], d["st"], lat[b:b + 1])
        e = rms(allb[b:b + 1], one)
        print(f"bf16 DAC batch ({size}) item {b}: rms difference to its single decode {e:.3e} (item rms {rms(one):.3e}, bound {0.5 * floor_rel * rms(one):.3e})")
        assert e < 0.5 * floor_rel * rms(one), (b, e, rms(one))


# ------------------------------------------------------------------ 6. causality and streaming
def test_bf16_decode_is_causal_and_streams(gold, dacs):
    d = dacs["tiny"]
    dac = d["bf16"]
    floor_rel = rms(gold["dac_tiny.bf16.wav"].float(), gold["dac_tiny.wav"]) / rms(gold["dac_tiny.wav"])
    z = torch.randn((1, TINY_DAC.latent_dim, 32), generator=torch.Generator().manual_seed(5))
    whole = dac.decode_zq(z)
    head = dac.decode_zq(z[..., :24])
    e = rms(head, whole[..., : head.shape[-1]])
    print(f"bf16 DAC causality: rms {e:.3e} (bound {0.5 * floor_rel * rms(head):.3e})")
    assert e < 0.5 * floor_rel * rms(head)
    lat = torch.randn((1, 32, 80), generator=torch.Generator().manual_seed(6))
    full = E.ae_decode(dac, d["st"], lat)
    s = DACStream(dac, d["st"])
    parts = [s.push(lat[0, a:b]) for a, b in ((0, 16), (16, 24), (24, 32))]
    got = torch.cat(parts, dim=-1)
    e = rms(got, full)
    print(f"bf16 DAC stream 16 + 8 + 8: rms {e:.3e} (bound {0.5 * floor_rel * rms(full):.3e})")
    assert got.shape == full.shape and e < 0.5 * floor_rel * rms(full)


# ------------------------------------------------------------------ 7. fp32 untouched
def test_fp32_default_is_untouched(gold, dacs):
    d = dacs["tiny"]
    z = gold["dac_tiny.z"]
    a = d["f32"].decode_zq(z)
    b = E.DAC(d["cfg"], d["w"], device=DEV, dtype=torch.float32).decode_zq(z)
    assert torch.equal(a, b)
    assert rms(a, gold["dac_tiny.wav"]) < WAV_TOL
    with pytest.raises(ValueError):
        E.DAC(d["cfg"], d["w"], device=DEV, dtype=torch.float16)
