"""GPU: the Fish S1-DAC's small hand-written kernels (csrc/dac.hip) and the two row softmaxes (csrc/elementwise.hip), one launch each through
the echo_op_dac_* / echo_op_softmax entry points, against an fp64 restatement of the same operation on the same operands (bf16: the bf16 values
widened to fp64, with the intermediate bf16 roundings the kernel documents).

Every output sits in a buffer whose row pitch is larger than its width and which has SPARE rows behind the last one, all pre-filled with
SENTINEL: whatever lies outside the documented output region must come back bit-unchanged.  Input memory the operation must not read - pad
columns, spare rows, rows of the previous batch item that the causal padding hides, masked score columns - holds NaN (always inside the tensor).

Tolerances (no case is bit-exact unless it says so):
  fp32 kernels  `_check_f32`: the same formula in plain fp32 torch on the CPU has the maximum absolute error e32 against fp64; the kernel may
                have 4 * e32 (another summation order, the device's sinf / expf / tanhf / rsqrtf) + one fp32 ulp of the largest |reference|.
  bf16 kernels  `_check_bf16`: against bf16(reference) through U.bf16_close; the allowed ulp distance is max(1, 2 x the worst distance of the
                fp32 torch restatement with the same rounding points), the share of exactly equal elements at least the restatement's - 0.01.
Each check prints one `DACK` line (profiles/pr_dac_kernel_tests.txt holds a run's table)."""
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from tests import gpu_util as U  # noqa: E402
from echo_tts_amd import _lib as L  # noqa: E402
from oracle import echo_ref as R  # noqa: E402

DEV = U.DEV
SENTINEL = 7.0
SPARE = 3              # sentinel / NaN rows behind the last row of every buffer
NAN = float("nan")
F32, BF16 = torch.float32, torch.bfloat16
DTYPES = [pytest.param(F32, id="f32"), pytest.param(BF16, id="bf16")]


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _wide(t, ct):
    """Operand values in the computing type ct (fp64 for the reference, fp32 for the restatement)."""
    return t.cpu().to(ct)


def _placed(data, rows, ld, fill):
    """data (r, c) in the top left corner of a (rows, ld) device buffer filled with `fill`."""
    buf = torch.full((rows, ld), fill, dtype=data.dtype, device=DEV)
    buf[:data.shape[0], :data.shape[1]] = data.to(DEV)
    return buf


def _assert_outside_untouched(buf, rows, cols=None):
    """Everything of a SENTINEL-filled buffer outside [:rows] (1-D) / [:rows, :cols] still holds SENTINEL."""
    t = buf.detach().cpu().float().clone()
    if cols is None:
        t[:rows] = SENTINEL
    else:
        t[:rows, :cols] = SENTINEL
    assert bool((t == SENTINEL).all()), f"{int((t != SENTINEL).sum())} elements outside the output region were written"


def _bits(t):
    t = t.detach().cpu().contiguous()
    return t.view(torch.int16 if t.element_size() == 2 else torch.int32)


def _ulp32(m):
    """One fp32 ulp at magnitude m."""
    return 2.0 ** (math.floor(math.log2(m)) - 23) if m > 0 else 2.0 ** -149


def _check_f32(name, got, ref64, f32):
    got, f32 = got.detach().cpu(), f32.cpu()
    assert got.dtype == F32 and f32.dtype == F32 and ref64.dtype == torch.float64
    assert bool(torch.isfinite(got).all()), f"{name}: non-finite output"
    e32 = float((f32.double() - ref64).abs().max())
    err = float((got.double() - ref64).abs().max())
    floor = _ulp32(float(ref64.abs().max()))
    bound = 4 * e32 + floor
    print(f"DACK {name:<46} f32  e32 {e32:.3e}  kernel {err:.3e}  kernel/e32 {err / e32 if e32 else float('inf'):7.2f}  bound {bound:.3e}")
    assert err <= bound, f"{name}: kernel error {err:.3e} > 4 * {e32:.3e} + {floor:.3e}"


def _check_bf16(name, got, ref_b, rest_b, atol=0.0):
    """got, ref_b = bf16(reference), rest_b = the fp32 restatement's bf16 result; all as fp32 values of bf16 numbers."""
    got, ref_b, rest_b = got.detach().cpu().float(), ref_b.float(), rest_b.float()
    assert bool(torch.isfinite(got).all()), f"{name}: non-finite output"

    def worst(o):
        d, den = (o - ref_b).abs(), (2.0 ** -7) * ref_b.abs()
        nz = den > 0
        return float((d[nz] / den[nz]).max()) if bool(nz.any()) else 0.0

    w_rest, share_rest = worst(rest_b), float((rest_b == ref_b).float().mean())
    ulps, share = max(1.0, 2.0 * w_rest), max(share_rest - 0.01, 0.0)
    print(f"DACK {name:<46} bf16 restatement {w_rest:.3f} ulp / {share_rest:.4f} exact  kernel {worst(got):.3f} ulp / "
          f"{float((got == ref_b).float().mean()):.4f} exact  allowed {ulps:.3f} ulp / {share:.4f}")
    U.bf16_close(got, ref_b, ulps=ulps, atol=atol, frac_exact=share)


# ------------------------------------------------------------------------------------------------ dwconv_ln
DW_EPS = float(torch.tensor(1e-6, dtype=F32))     # the fp32 value the kernel receives


def _dw_inputs(C, T, dt):
    g = _gen(1000 * C + T)
    x = torch.randn(T, C, generator=g).to(dt)
    w = (0.4 * torch.randn(C, 7, generator=g)).to(dt)
    b = (0.1 * torch.randn(C, generator=g)).to(dt)
    lnw = (1.0 + 0.2 * torch.randn(C, generator=g)).to(dt)
    lnb = (0.1 * torch.randn(C, generator=g)).to(dt)
    return x, w, b, lnw, lnb


def _dw_formula(x, w, b, lnw, lnb, T, S, ct, bf16):
    """autoencoder.py:362-364 (oracle/echo_ref.py:628-629): causal depthwise conv k7 whose padding restarts per item, LayerNorm over C.
    bf16: the conv output is the bf16 tensor the reference materialises between the two modules."""
    x, w, b, lnw, lnb = (_wide(t, ct) for t in (x, w, b, lnw, lnb))
    C, n = x.shape[1], T // S
    xp = F.pad(x.view(n, S, C), (0, 0, 6, 0))
    conv = b.expand(n, S, C)
    for k in range(7):
        conv = conv + w[:, k] * xp[:, k:k + S, :]
    if bf16:
        conv = conv.to(BF16).to(ct)
    mean = conv.mean(-1, keepdim=True)
    var = (conv - mean).pow(2).mean(-1, keepdim=True)
    return ((conv - mean) * torch.rsqrt(var + DW_EPS) * lnw + lnb).reshape(T, C)


def _dw_run(x, w, b, lnw, lnb, T, S, C):
    xb = _placed(x, T + SPARE, C + 8, NAN)
    yb = torch.full((T + SPARE, C + 4), SENTINEL, dtype=x.dtype, device=DEV)
    U.dac_dwconv_ln(xb, yb, T, S, C, w.to(DEV), b.to(DEV), lnw.to(DEV), lnb.to(DEV), DW_EPS)
    torch.cuda.synchronize()
    _assert_outside_untouched(yb, T, C)
    return yb[:T, :C].cpu()


@pytest.mark.parametrize("T,S", [(13, 13), (21, 7), (9, 3), (1, 1)])
@pytest.mark.parametrize("C", [32, 272, 1024])
@pytest.mark.parametrize("dt", DTYPES)
def test_dwconv_ln_matches_fp64(dt, C, T, S):
    """dwconv_ln_kernel against autoencoder.py:362-364.  C: 8 of 64 lanes busy / a second chunk on 4 lanes / the register maximum; (T, S): a
    ragged last block of 4 waves / three items / S < 7 (every row has truncated taps) / one row."""
    ins = _dw_inputs(C, T, dt)
    got = _dw_run(*ins, T, S, C)
    ref = _dw_formula(*ins, T, S, torch.float64, dt == BF16)
    rest = _dw_formula(*ins, T, S, F32, dt == BF16)
    name = f"dwconv_ln C={C} T={T} S={S}"
    if dt == F32:
        _check_f32(name, got, ref, rest)
    else:
        # (v - mean) * rs * g + be cancels: a result near zero keeps the absolute error of its addends, a few fp32 ulps of the largest one
        _check_bf16(name, got, ref.to(BF16), rest.to(BF16), atol=2.0 ** -21 * float(ref.abs().max()))


@pytest.mark.parametrize("C", [32, 272, 1024])
@pytest.mark.parametrize("dt", DTYPES)
def test_dwconv_ln_constant_conv_gives_the_ln_bias_exactly(dt, C):
    """w = 0 and b = 0.5 in every channel: the conv output is constant (sums of 0.5 and their mean are exact), v - mean = 0, y = lnb."""
    T, S = 21, 7
    x, w, b, lnw, lnb = _dw_inputs(C, T, dt)
    got = _dw_run(x, torch.zeros_like(w), torch.full_like(b, 0.5), lnw, lnb, T, S, C)
    assert torch.equal(_bits(got), _bits(lnb.expand(T, C)))


@pytest.mark.parametrize("C", [32, 272, 1024])
@pytest.mark.parametrize("dt", DTYPES)
def test_dwconv_ln_does_not_read_the_previous_items_rows(dt, C):
    """(T, S) = (21, 7): NaN in the last 6 rows of items 0 and 1.  Item 2 - and row 0 of items 0 and 1 - must have the bits of the clean call."""
    T, S = 21, 7
    x, w, b, lnw, lnb = _dw_inputs(C, T, dt)
    clean = _dw_run(x, w, b, lnw, lnb, T, S, C)
    xn = x.clone()
    xn[1:7] = NAN
    xn[8:14] = NAN
    got = _dw_run(xn, w, b, lnw, lnb, T, S, C)
    keep = [0, 7] + list(range(14, 21))
    assert bool(torch.isfinite(got[keep].float()).all())
    assert torch.equal(_bits(got[keep]), _bits(clean[keep]))


# ------------------------------------------------------------------------------------------------ conv_out_tanh
CO_CASES = ([(T, T, C, 7) for C in (4, 36, 128) for T in (1, 121, 122, 123, 250)] +
            [(T, S, C, 7) for C in (4, 36, 128) for (T, S) in ((183, 61), (150, 50))] +
            [(123, 123, 36, 1), (123, 123, 36, 8)])
CO_BIAS = float(torch.tensor(0.02, dtype=F32))


def _co_inputs(T, C, k, dt):
    """Pre-activations of standard deviation ~2.5; rows 40..55 are quiet (x 0.004: outputs in tanh's linear region), rows 60..75 loud (x 2:
    saturated outputs), so that a case of T >= 121 spans both by construction."""
    g = _gen(100000 * k + 1000 * C + T)
    x = torch.randn(T, C, generator=g)
    x[40:56] *= 0.004
    x[60:76] *= 2.0
    w = (2.5 / math.sqrt(k * C) * torch.randn(k, C, generator=g)).to(dt)
    return x.to(dt), w


def _co_formula(x, w, T, S, k, ct, bf16):
    """autoencoder.py:994 (oracle/echo_ref.py dac_decoder's last causal_conv1d + tanh): causal conv k, C -> 1, padding restarts per item.
    Returns (y, pre-activation).  bf16: the conv output and the tanh are bf16 tensors."""
    x, w = _wide(x, ct), _wide(w, ct)
    C, n = x.shape[1], T // S
    xp = F.pad(x.view(n, S, C), (0, 0, k - 1, 0))
    a = torch.full((n, S), CO_BIAS, dtype=ct)
    for kk in range(k):
        a = a + xp[:, kk:kk + S, :] @ w[kk]
    a = a.reshape(T)
    if bf16:
        a = a.to(BF16).to(ct)
    y = torch.tanh(a)
    return (y.to(BF16).to(ct) if bf16 else y), a


def _co_run(x, w, T, S, C, k):
    xb = _placed(x, T + SPARE, C + 4, NAN)
    yb = torch.full((T + 5,), SENTINEL, dtype=F32, device=DEV)
    U.dac_conv_out_tanh(xb, yb, T, S, C, k, w.to(DEV), CO_BIAS)
    torch.cuda.synchronize()
    _assert_outside_untouched(yb, T)
    return yb[:T].cpu()


@pytest.mark.parametrize("T,S,C,k", CO_CASES)
@pytest.mark.parametrize("dt", DTYPES)
def test_conv_out_tanh_matches_fp64(dt, T, S, C, k):
    """conv_out_tanh_kernel against autoencoder.py:994.  k = 7: a block owns 122 outputs, so T = 121 / 122 / 123 / 250 end inside, at and behind
    a block; (183, 61): an item boundary on the block boundary, (150, 50): inside a block.  S < T: a second call with NaN in the last k - 1 rows
    of every item but the last must leave every output that does not own those rows bit-equal."""
    x, w = _co_inputs(T, C, k, dt)
    got = _co_run(x, w, T, S, C, k)
    ref, a64 = _co_formula(x, w, T, S, k, torch.float64, dt == BF16)
    rest, _ = _co_formula(x, w, T, S, k, F32, dt == BF16)
    if T >= 121:          # (a single output cannot do both)
        assert bool((ref.abs() > 0.999).any()) and bool((ref.abs() < 0.05).any()), "inputs must span saturation and the linear region"
    name = f"conv_out_tanh C={C} k={k} T={T} S={S}"
    if dt == F32:
        _check_f32(name, got, ref, rest.float())
    else:
        assert torch.equal(got, got.bfloat16().float()), "the bf16 form must store bf16-representable samples"
        # a pre-activation near zero keeps the absolute error of its k * C fp32 additions (a few ulps of the largest partial sum); tanh' <= 1
        _check_bf16(name, got, ref.float(), rest.float(), atol=2.0 ** -21 * float(a64.abs().max()))
    if S < T and k > 1:
        xn = x.clone()
        own = torch.ones(T, dtype=torch.bool)
        for it in range(T // S - 1):
            xn[(it + 1) * S - (k - 1):(it + 1) * S] = NAN
            own[(it + 1) * S - (k - 1):(it + 1) * S] = False
        again = _co_run(xn, w, T, S, C, k)
        assert bool(torch.isfinite(again[own]).all())
        assert torch.equal(_bits(again[own]), _bits(got[own]))


# ------------------------------------------------------------------------------------------------ snake
def _snake(x, alpha):
    """autoencoder.py:96-102 (oracle/echo_ref.py:536)."""
    return x + (alpha + 1e-9).reciprocal() * torch.sin(alpha * x).pow(2)


def test_snake_matches_fp64():
    """snake_kernel: 37 x 20, ldx = 24, ldy = 28, alpha in [0.05, 3] and one column with alpha == 0 (y == x bit for bit), |x| up to 50."""
    rows, C, zero_col = 37, 20, 7
    g = _gen(37)
    x = (torch.rand(rows, C, generator=g) * 100 - 50)
    x[0, 0], x[1, 1] = 50.0, -50.0
    alpha = torch.rand(C, generator=g) * 2.95 + 0.05
    alpha[zero_col] = 0.0
    xb = _placed(x, rows + SPARE, C + 4, NAN)
    yb = torch.full((rows + SPARE, C + 8), SENTINEL, dtype=F32, device=DEV)
    U.dac_snake(xb, yb, rows, C, alpha.to(DEV))
    torch.cuda.synchronize()
    _assert_outside_untouched(yb, rows, C)
    got = yb[:rows, :C].cpu()
    _check_f32("snake 37x20", got, _snake(x.double(), alpha.double()), _snake(x, alpha))
    assert torch.equal(_bits(got[:, zero_col]), _bits(x[:, zero_col]))


# ------------------------------------------------------------------------------------------------ ae_rope
@pytest.mark.parametrize("HD", [64, 128])
@pytest.mark.parametrize("dt", DTYPES)
def test_ae_rope_is_the_separately_rounded_fp32_expression(dt, HD):
    """ae_rope_kernel against autoencoder.py:815-826 (oracle/echo_ref.py:578-579) on the q and k sections of a (rows, 3 * H * HD) qkv buffer:
    bit-equal to the fp32 torch expression a*c - b*s, b*c + a*s (bf16: its bf16 rounding).  Rows take position row % S of a 16-position cache
    (backed by 32, so that no wrong position leaves the tensor); v, and the rows behind the last one, stay as they were."""
    H, S, rows = 3, 11, 22
    D = H * HD
    g = _gen(HD)
    buf = torch.randn(rows + SPARE, 3 * D, generator=g).to(dt)
    cache = R.ae_rope_cache(32, HD).float()[:16]
    assert len({tuple(cache[p].flatten().tolist()) for p in range(16)}) == 16
    want = buf.clone()
    pos = torch.arange(rows) % S
    c, s = cache[pos][:, None, :, 0], cache[pos][:, None, :, 1]
    for off in (0, D):
        xs = buf[:rows, off:off + D].float().view(rows, H, HD // 2, 2)
        a, b = xs[..., 0], xs[..., 1]
        ac, bs, bc, as_ = a * c, b * s, b * c, a * s
        want[:rows, off:off + D] = torch.stack([ac - bs, bc + as_], -1).view(rows, D).to(dt)
    dev, cdev = buf.to(DEV), R.ae_rope_cache(32, HD).float().to(DEV)
    U.dac_rope(dev, rows, S, H, HD, cdev, col_off=0)
    U.dac_rope(dev, rows, S, H, HD, cdev, col_off=D)
    torch.cuda.synchronize()
    got = dev.cpu()
    assert torch.equal(_bits(got[:, 2 * D:]), _bits(buf[:, 2 * D:])) and torch.equal(_bits(got[rows:]), _bits(buf[rows:]))
    assert torch.equal(_bits(got), _bits(want)), f"{int((_bits(got) != _bits(want)).sum())} elements differ"


# ------------------------------------------------------------------------------------------------ softmax
def _softmax_formula(v, ct):
    """Row softmax of v (-inf = masked) in ct: exp(v - max) / sum."""
    v = v.to(ct)
    e = torch.exp(v - v.max(-1, keepdim=True)[0])
    return e / e.sum(-1, keepdim=True)


def test_softmax_f32_with_key_bias_and_shared_bias_rows():
    """softmax_f32_kernel in the layout of the parity attention (engine.hip: launch_softmax_f32(sc, ld, S, rows * H, tot, tot, biasrows, ld, H,
    ...)): B = 2 items x H = 3 heads x 5 queries, one bias row per item, -inf at irregular columns; scores span +-80.  The bias tensor has
    B * H rows of which the launch owns the first B, so that a wrong row index stays inside it."""
    B, H, rpb, ncols, ld = 2, 3, 5, 70, 72
    rows = B * H * rpb
    g = _gen(70)
    s = torch.rand(rows, ncols, generator=g) * 160 - 80
    bias = torch.where(torch.rand(B * H, ld, generator=g) < 0.4, float("-inf"), 0.0) + 0.5 * torch.randn(B * H, ld, generator=g)
    bias[:, 3] = 0.25                                     # at least one finite column per row
    assert bool((bias[:B, :ncols] == float("-inf")).any(1).all())
    assert not torch.equal(torch.isinf(bias[0]), torch.isinf(bias[1])) and not torch.equal(torch.isinf(bias[1]), torch.isinf(bias[2]))
    sb = _placed(s, rows + SPARE, ld, SENTINEL)
    U.softmax(sb, rpb, rows, ncols, ncols, bias=bias.to(DEV), bias_batch_stride=ld, heads_per_bias_row=H, causal=0, window=0)
    torch.cuda.synchronize()
    _assert_outside_untouched(sb, rows, ncols)
    got = sb[:rows, :ncols].cpu()
    v = s + bias[:B, :ncols].repeat_interleave(H * rpb, 0)            # fp32 sum, exactly the kernel's operand
    _check_f32("softmax_f32 bias B=2 H=3", got, _softmax_formula(v, torch.float64), _softmax_formula(v, F32))
    assert bool((_bits(got)[torch.isinf(v)] == 0).all()), "masked columns must be exactly +0"


@pytest.mark.parametrize("window", [0, 1, 8, 64, 200])
@pytest.mark.parametrize("Tn", [1, 37, 130])
@pytest.mark.parametrize("dt", DTYPES)
def test_softmax_causal_window_matches_fp64(dt, Tn, window):
    """softmax_f32_kernel / softmax_window_bf16_kernel as the post_module launches them (autoencoder.py:762-773, oracle/echo_ref.py:587: key j
    visible to query i iff max(0, i - window + 1) <= j <= i; window 0 = causal only): 2 batches of Tn queries, ncols = Tn.  Columns
    ncols..ncols_pad-1 hold NaN and come back as +0; bf16 also holds NaN in every masked column (the kernel reads its window only)."""
    nb, ncols = 2, Tn
    ncols_pad = (Tn + 31) // 32 * 32
    ld, rows = ncols_pad + 8, nb * Tn
    g = _gen(1000 * Tn + window)
    s = (torch.rand(rows, ncols, generator=g) * 10 - 5).to(dt)
    qi = (torch.arange(rows) % Tn)[:, None]
    j = torch.arange(ncols)[None]
    visible = (j <= qi) & ((j >= qi - window + 1) if window > 0 else torch.ones_like(j, dtype=torch.bool))
    fill = s.clone()
    if dt == BF16:
        fill[~visible] = NAN
    sb = _placed(fill, rows + SPARE, ld, SENTINEL)
    sb[:rows, ncols:ncols_pad] = NAN
    U.softmax(sb, Tn, rows, ncols, ncols_pad, causal=1, window=window)
    torch.cuda.synchronize()
    _assert_outside_untouched(sb, rows, ncols_pad)
    out = sb[:rows].cpu()
    assert bool((_bits(out[:, ncols:ncols_pad]) == 0).all()), "the K padding columns must come back as +0"
    got = out[:, :ncols]
    v = torch.where(visible, s.float(), float("-inf"))
    ref, rest = _softmax_formula(v, torch.float64), _softmax_formula(v, F32)
    name = f"softmax window Tn={Tn} window={window}"
    if dt == F32:
        _check_f32(name, got, ref, rest)
        assert float((got.double().sum(-1) - 1).abs().max()) < 1e-6
    else:
        _check_bf16(name, got, ref.to(BF16), rest.to(BF16))
    want_nz = torch.minimum(qi[:, 0] + 1, torch.full((rows,), window, dtype=torch.long)) if window else qi[:, 0] + 1
    assert torch.equal((got.float() != 0).sum(-1), want_nz)
    assert bool((_bits(got)[~visible] == 0).all()), "masked columns must be exactly +0"


# ------------------------------------------------------------------------------------------------ conv_in_snake
def _cis_formula(x, w, b, alpha, T, k, ct):
    """autoencoder.py:917 (oracle/echo_ref.py dac_encoder's first causal_conv1d) and the Snake of it (autoencoder.py:96-102)."""
    x, w, b, alpha = (t.to(ct) for t in (x, w, b, alpha))
    xp = F.pad(x, (k - 1, 0))
    y = b.expand(T, -1)
    for kk in range(k):
        y = y + xp[kk:kk + T, None] * w[:, kk]
    return y, _snake(y, alpha)


@pytest.mark.parametrize("pad", [0, 4])
@pytest.mark.parametrize("C", [4, 64])
@pytest.mark.parametrize("T", [1, 6, 7, 1000])
def test_conv_in_snake_matches_fp64(T, C, pad):
    """conv_in_snake_kernel, k = 7, ld = C and C + 4: both outputs.  The samples sit between NaNs: x[t < 0] is zero padding, not memory."""
    k, lead = 7, 8
    g = _gen(100 * T + C)
    x = torch.randn(T, generator=g)
    w, b = 0.5 * torch.randn(C, k, generator=g), 0.1 * torch.randn(C, generator=g)
    alpha = torch.rand(C, generator=g) * 2.95 + 0.05
    xb = torch.full((lead + T + 4,), NAN, dtype=F32, device=DEV)
    xb[lead:lead + T] = x.to(DEV)
    yb = torch.full((T + SPARE, C + pad), SENTINEL, dtype=F32, device=DEV)
    sb = yb.clone()
    U.dac_conv_in_snake(xb, T, C, k, w.to(DEV), b.to(DEV), alpha.to(DEV), yb, sb, x_off=lead)
    torch.cuda.synchronize()
    y64, s64 = _cis_formula(x, w, b, alpha, T, k, torch.float64)
    y32, s32 = _cis_formula(x, w, b, alpha, T, k, F32)
    for nm, buf, r64, r32 in (("y", yb, y64, y32), ("snake", sb, s64, s32)):
        _assert_outside_untouched(buf, T, C)
        _check_f32(f"conv_in_snake {nm} T={T} C={C} ld={C + pad}", buf[:T, :C].cpu(), r64, r32)


# ------------------------------------------------------------------------------------------------ vq_argmax
def _vq_run(e, cbn, cb, T, size, lde):
    eb = _placed(e, T + SPARE, lde, NAN)
    idx = torch.full((T + SPARE,), -7, dtype=torch.int32, device=DEV)
    zst = torch.full((T + SPARE, 32), SENTINEL, dtype=F32, device=DEV)
    gath = torch.full((T + SPARE, 40), SENTINEL, dtype=F32, device=DEV)
    U.dac_vq_argmax(eb, T, cbn.to(DEV), cb.to(DEV), size, idx, zst, gath)
    torch.cuda.synchronize()
    assert bool((idx[T:] == -7).all())
    _assert_outside_untouched(zst, T, 8)
    _assert_outside_untouched(gath, T, 8)
    idx = idx[:T].cpu().long()
    # copies: the raw code vector, and the straight-through value in the reference's fp32 order (autoencoder.py:157)
    assert torch.equal(_bits(gath[:T, :8]), _bits(cb[idx]))
    assert torch.equal(_bits(zst[:T, :8]), _bits(e + (cb[idx] - e)))
    return idx


def _vq_scores64(e, cbn):
    """autoencoder.py:145-158 (oracle/echo_ref.py:723-726) in fp64 on the fp32 operands."""
    en, c = F.normalize(e.double()), cbn.double()
    return -(en.pow(2).sum(1, keepdim=True) - 2 * en @ c.t() + c.pow(2).sum(1)[None])


@pytest.mark.parametrize("lde", [8, 32])
@pytest.mark.parametrize("T", [1, 203])
@pytest.mark.parametrize("size", [40, 100, 1024, 4096])
def test_vq_argmax_codes_match_fp64(size, T, lde):
    """vq_argmax_kernel: queries of a known code j, scaled by U(0.2, 5) plus noise; the fp64 margin between the best and the second score is at
    least 1.6e-2 (checked here), five orders above fp32 rounding, so every row must give the fp64 argmax - none is excluded."""
    g = _gen(size)
    cb = torch.randn(size, 8, generator=g)
    cbn = F.normalize(cb)
    j = torch.randint(0, size, (T,), generator=g)
    e = cbn[j] * (torch.rand(T, 1, generator=g) * 4.8 + 0.2) + 0.02 * torch.randn(T, 8, generator=g)
    score = _vq_scores64(e, cbn)
    top = score.topk(2, dim=1)[0]
    assert float((top[:, 0] - top[:, 1]).min()) >= 1.6e-2 and torch.equal(score.argmax(1), j)
    idx = _vq_run(e, cbn, cb, T, size, lde)
    assert torch.equal(idx, j), f"{int((idx != j).sum())} of {T} codes differ from the fp64 argmax"


def test_vq_argmax_ties_take_the_lowest_index():
    """Codebook rows a, a + 64 and a + 65 identical: a and a + 64 tie inside one lane's strided scan, a and a + 65 across lanes.  Queries aimed
    at them must give a, the reference's first argmax (autoencoder.py:152 `.max(1)[1]`)."""
    size, firsts = 300, [0, 5, 63, 100, 130, 191]
    g = _gen(300)
    cb = torch.randn(size, 8, generator=g)
    for a in firsts:
        cb[a + 64] = cb[a]
        cb[a + 65] = cb[a]
    cbn = F.normalize(cb)
    j = torch.tensor([a for a in firsts for _ in range(5)])
    T = len(j)
    e = cbn[j] * (torch.rand(T, 1, generator=g) * 4.8 + 0.2) + 0.02 * torch.randn(T, 8, generator=g)
    score = _vq_scores64(e, cbn)
    best = score.max(1, keepdim=True)[0]
    first = (score == best).float().argmax(1)            # lowest index among the equal maxima
    assert torch.equal(first, j) and bool(((score == best).sum(1) == 3).all())
    top = score.topk(4, dim=1)[0]
    assert float((top[:, 0] - top[:, 3]).min()) >= 1.6e-2
    assert torch.equal(_vq_run(e, cbn, cb, T, size, 8), j)


# ------------------------------------------------------------------------------------------------ refusals
def _refused(call, *outs):
    """The call raises through L.check (non-zero status) and leaves the SENTINEL-filled outputs untouched."""
    with pytest.raises(L.EchoHipError):
        call()
    torch.cuda.synchronize()
    for o in outs:
        assert bool((o.cpu().float() == SENTINEL).all())


@pytest.mark.parametrize("C", [1028, 30])
@pytest.mark.parametrize("dt", DTYPES)
def test_dwconv_ln_refuses_unsupported_widths(dt, C):
    T, ld = 4, 1040
    x = torch.zeros((T + SPARE, ld), dtype=dt, device=DEV)
    y = torch.full((T + SPARE, ld), SENTINEL, dtype=dt, device=DEV)
    w, v = torch.zeros((ld, 7), dtype=dt, device=DEV), torch.zeros((ld,), dtype=dt, device=DEV)
    _refused(lambda: U.dac_dwconv_ln(x, y, T, T, C, w, v, v, v), y)


@pytest.mark.parametrize("C,k", [(132, 7), (36, 9), (36, 0)])
@pytest.mark.parametrize("dt", DTYPES)
def test_conv_out_tanh_refuses_unsupported_shapes(dt, C, k):
    T = 8
    x = torch.zeros((T + SPARE, 136), dtype=dt, device=DEV)
    w = torch.zeros((9, 136), dtype=dt, device=DEV)
    y = torch.full((T + 5,), SENTINEL, dtype=F32, device=DEV)
    _refused(lambda: U.dac_conv_out_tanh(x, y, T, T, C, k, w, 0.0), y)


def test_conv_in_snake_refuses_a_width_that_is_no_multiple_of_4():
    T, C = 8, 6
    x = torch.zeros((T + 8,), dtype=F32, device=DEV)
    w, v = torch.zeros((8, 7), dtype=F32, device=DEV), torch.ones((8,), dtype=F32, device=DEV)
    y = torch.full((T + SPARE, 8), SENTINEL, dtype=F32, device=DEV)
    s = y.clone()
    _refused(lambda: U.dac_conv_in_snake(x, T, C, 7, w, v, v, y, s), y, s)


def test_softmax_bf16_refuses_a_bias_and_a_non_causal_call():
    s = torch.full((8 + SPARE, 40), SENTINEL, dtype=BF16, device=DEV)
    bias = torch.zeros((2, 40), dtype=F32, device=DEV)
    _refused(lambda: U.softmax(s, 4, 8, 32, 32, bias=bias, bias_batch_stride=40, causal=1), s)
    _refused(lambda: U.softmax(s, 4, 8, 32, 32, causal=0), s)


def test_wrappers_refuse_what_the_launchers_leave_unchecked():
    """T < 1, an odd HD, size < 1, ncols_pad < ncols, ld < ncols_pad, an unknown dtype, a NULL operand."""
    lib, st = U.lib(), U.stream()
    f = torch.full((16, 64), SENTINEL, dtype=F32, device=DEV)
    i = torch.full((16,), -7, dtype=torch.int32, device=DEV)
    p = f.data_ptr()
    assert lib.echo_op_dac_dwconv_ln(L.ECHO_F32, p, 64, p, 64, 0, 1, 32, p, p, p, p, 1e-6, st) != 0
    assert lib.echo_op_dac_dwconv_ln(2, p, 64, p, 64, 4, 4, 32, p, p, p, p, 1e-6, st) != 0
    assert lib.echo_op_dac_dwconv_ln(L.ECHO_F32, p, 64, None, 64, 4, 4, 32, p, p, p, p, 1e-6, st) != 0
    assert lib.echo_op_dac_conv_out_tanh(L.ECHO_F32, p, 64, p, 0, 1, 32, 7, p, 0.0, st) != 0
    assert lib.echo_op_dac_snake(p, 16, p, 64, 4, 32, p, st) != 0
    assert lib.echo_op_dac_rope(L.ECHO_F32, p, 64, 4, 4, 1, 33, p, st) != 0
    assert lib.echo_op_dac_rope(L.ECHO_F32, p, 32, 4, 4, 1, 64, p, st) != 0
    assert lib.echo_op_dac_conv_in_snake(p, 0, 4, 7, p, p, p, p, p, 64, st) != 0
    assert lib.echo_op_dac_vq_argmax(p, 8, 4, p, p, 0, i.data_ptr(), p, 32, p, 32, st) != 0
    assert lib.echo_op_dac_vq_argmax(p, 8, 0, p, p, 4, i.data_ptr(), p, 32, p, 32, st) != 0
    assert lib.echo_op_softmax(L.ECHO_F32, p, 64, 4, 8, 40, 32, None, 0, 1, 1, 0, st) != 0
    assert lib.echo_op_softmax(L.ECHO_F32, p, 32, 4, 8, 40, 64, None, 0, 1, 1, 0, st) != 0
    assert lib.echo_op_softmax(L.ECHO_F32, p, 64, 4, 7, 32, 32, None, 0, 1, 1, 0, st) != 0
    assert lib.echo_op_softmax(3, p, 64, 4, 8, 32, 32, None, 0, 1, 1, 0, st) != 0
    torch.cuda.synchronize()
    assert bool((f.cpu() == SENTINEL).all()) and bool((i.cpu() == -7).all())
