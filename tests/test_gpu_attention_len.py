"""GPU: the length forms of the joint attention (attn5_qlen_kernel, attn_qlen_kernel) at kernel level, through
echo_op_attention_bf16_len, against an fp64 softmax attention of the same bf16 operands.

A launch has R rows of S queries; row r owns its first qlen[r] queries and, as the engine sets it, nkeys_self[r] = qlen[r] self keys.  A
query block that starts at or beyond qlen[r] is not computed: its O block comes back as zeros and its range-report word as 0.

Which kernel runs is decided once per process by the switches ECHO_ATTN / ECHO_ATTN_Q128 (launch_attention_bf16); `_block_size` repeats
that decision so that the tests know which blocks are skipped:
  default / ECHO_ATTN=5   attn5_qlen_kernel, 128-query blocks when ceil(S / 128) * H * R <= 256, else 256 (ECHO_ATTN_Q128 forces either);
  ECHO_ATTN=1             attn_qlen_kernel: 128-query blocks, no report words - the redo-word assertions are dropped;
  ECHO_ATTN=4             attn4_kernel, which computes its padding blocks under the per-row key counts: "skipped blocks are exactly 0"
                          becomes "finite", and Q holds no NaN (every block is read).
test_length_forms_under_forced_kernels repeats this module in child processes under each switch and runs the engine-level length tests
under ECHO_ATTN=1.

Tolerance: the one of test_attention_bf16_joint_segments, per (row, head): max(err - |ref| * 2^-7) < 3e-2 and mean(err) < 2e-3."""
import ctypes as C
import math
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import gpu_util as U  # noqa: E402
from echo_tts_amd import _lib as L  # noqa: E402

DEV = U.DEV
HD = 128
SCALE = 1 / math.sqrt(HD)
PAD_COLS = 64          # sentinel columns behind every row of O (row pitch D + 64)
PAD_ROWS = 8           # sentinel rows behind the last row of O
SENTINEL = 7.0


def _variant():
    """The kernel the launcher takes for a call with a length table: 5, 4, or 1 (any other forced value falls through to attn_qlen_kernel)."""
    v = int(os.environ.get("ECHO_ATTN") or 0)
    return 5 if v == 0 else v if v in (4, 5) else 1


def _block_size(R, H, S):
    """Queries per workgroup of the kernel in play (launch_attention_bf16)."""
    v = _variant()
    if v == 1:
        return 128
    if v == 4:
        return 256
    forced = os.environ.get("ECHO_ATTN_Q128")
    q128 = int(forced) != 0 if forced else (S + 127) // 128 * H * R <= 256
    return 128 if q128 else 256


def _rnd(*shape, scale=1.0, seed=0):
    g = torch.Generator().manual_seed(seed + sum(shape))
    return (torch.randn(shape, generator=g) * scale).bfloat16().to(DEV)


class Geometry:
    """Operands of one joint-attention launch: self | text | speaker (Ls = 0: no speaker segment).  packed: Q, K and the gate are sections
    of one (R * S + 256, 4 D) buffer (the fused QKV GEMM's output); otherwise tensors of their own.  Every K / Vt element, padding
    included, is a finite random value.  plants: (row, head, query, key) - the key row becomes 20 x the query row."""

    def __init__(self, name, R, H, S, lens, Lt, nt, Ls, ns, packed, qscale, plants=()):
        self.name, self.R, self.H, self.S, self.lens, self.Lt, self.nt, self.Ls, self.ns = name, R, H, S, list(lens), Lt, list(nt), Ls, list(ns)
        self.plants = list(plants)
        D = self.D = H * HD
        self.blk = _block_size(R, H, S)
        self.nb = (S + self.blk - 1) // self.blk
        self.pS, pT, pSp = (S + 63) // 64 * 64, (Lt + 63) // 64 * 64, (max(Ls, 1) + 63) // 64 * 64
        if packed:
            self.buf = _rnd(R * S + 256, 4 * D, scale=qscale)
            self.ld = 4 * D
            self.q = self.buf[:R * S].view(R, S, 4 * D)[:, :, 0:D]
            self.k = self.buf[:R * S].view(R, S, 4 * D)[:, :, D:2 * D]
            self.g = self.buf[:R * S].view(R, S, 4 * D)[:, :, 3 * D:4 * D]
        else:
            self.ld = D
            self.q, self.k, self.g = _rnd(R, S, D, scale=qscale), _rnd(R, S, D, scale=qscale, seed=1), _rnd(R, S, D, seed=7)
        self.vt = _rnd(R, H, HD, self.pS, seed=2)                       # V^T of the self segment, (row, head, d, key)
        self.kt, self.vtt = _rnd(Lt + 64, D, seed=3), _rnd(1, H, HD, pT, seed=4)
        self.ksp, self.vtsp = _rnd(max(Ls, 1) + 64, D, seed=5), _rnd(1, H, HD, pSp, seed=6)
        self.pT, self.pSp = pT, pSp
        for (r, h, qi, kj) in self.plants:
            assert qi < self.lens[r] and kj < self.lens[r]
            self.k[r, kj, h * HD:(h + 1) * HD] = (20.0 * self.q[r, qi, h * HD:(h + 1) * HD].float()).bfloat16()
        self.o_ld = D + PAD_COLS
        self.o_fill = torch.full((R * S + PAD_ROWS, self.o_ld), SENTINEL, dtype=torch.bfloat16, device=DEV)
        self.o_fill[:R * S, :D] = float("nan")
        self._keep = []

    def first_skipped(self, r):
        """First query of row r's wholly skipped blocks (S: none)."""
        return min(self.S, (self.lens[r] + self.blk - 1) // self.blk * self.blk)

    def poison_q(self):
        """NaN into the Q rows of wholly skipped blocks: they must not be read.  (Not under ECHO_ATTN=4, whose kernel computes them.)"""
        if _variant() == 4:
            return
        for r in range(self.R):
            self.q[r, self.first_skipped(r):] = float("nan")

    def desc(self, out, self_keys, redo=None):
        R, H, S, D = self.R, self.H, self.S, self.D
        nk = torch.tensor([list(self_keys), self.nt, self.ns], dtype=torch.int32, device=DEV)
        self._keep.append(nk)
        d = L.EchoAttnDesc()
        d.Q, d.q_ld, d.q_row_stride = self.q.data_ptr(), self.ld, S * self.ld
        d.G, d.g_ld, d.g_row_stride = self.g.data_ptr(), self.ld, S * self.ld
        d.O, d.o_ld, d.o_row_stride = out.data_ptr(), self.o_ld, S * self.o_ld
        d.S, d.H, d.rows, d.nseg, d.causal, d.scale = S, H, R, 3 if self.Ls else 2, 0, SCALE
        segs = [(self.k.data_ptr(), self.ld, S * self.ld, self.vt, self.pS, False), (self.kt.data_ptr(), D, 0, self.vtt, self.pT, True),
                (self.ksp.data_ptr(), D, 0, self.vtsp, self.pSp, True)]
        for i, (kp, kld, krs, vt, pitch, shared) in enumerate(segs[:d.nseg]):
            sg = d.seg[i]
            sg.K, sg.k_ld, sg.k_head_stride, sg.k_row_stride = kp, kld, HD, krs
            sg.Vt, sg.vt_ld, sg.vt_head_stride = vt.data_ptr(), pitch, HD * pitch
            sg.vt_row_stride = 0 if shared else H * HD * pitch
            sg.nkeys = nk[i].data_ptr()
            sg.kv_mod = 1 if shared else 0
        if redo is not None:
            d.redo = redo.data_ptr()
        return d

    def launch(self, qlen=None, self_keys=None, redo=None):
        """One launch into a fresh NaN / sentinel filled O; qlen None: the plain entry point.  Returns the whole O buffer."""
        out = self.o_fill.clone()
        d = self.desc(out, self.lens if self_keys is None else self_keys, redo)
        if qlen is None:
            L.check(U.lib().echo_op_attention_bf16(C.byref(d), U.stream()))
        else:
            ql = torch.tensor(list(qlen), dtype=torch.int32, device=DEV)
            L.check(U.lib().echo_op_attention_bf16_len(C.byref(d), ql.data_ptr(), U.stream()))
        torch.cuda.synchronize()
        return out

    def view(self, out):
        """(R, S, D) view of the payload of an O buffer."""
        return out[:self.R * self.S].view(self.R, self.S, self.o_ld)[:, :, :self.D]

    def reference(self, r, extra_self_keys=0):
        """fp64 softmax attention of row r's queries below its length over lens[r] (+ extra) self keys and the row's text / speaker keys,
        rounded and gated at the kernels' rounding points (bf16(o), bf16(sigmoid(g)), bf16 of the product): (lens[r], H, 128) fp32."""
        n, H = self.lens[r], self.H
        nself = n + extra_self_keys
        q = self.q[r, :n].reshape(n, H, HD).permute(1, 0, 2).double()
        ks = [self.k[r, :nself].reshape(nself, H, HD).permute(1, 0, 2)]
        vs = [self.vt[r, :, :, :nself].permute(0, 2, 1)]
        if self.nt[r]:
            ks.append(self.kt[:self.nt[r]].reshape(-1, H, HD).permute(1, 0, 2))
            vs.append(self.vtt[0, :, :, :self.nt[r]].permute(0, 2, 1))
        if self.Ls and self.ns[r]:
            ks.append(self.ksp[:self.ns[r]].reshape(-1, H, HD).permute(1, 0, 2))
            vs.append(self.vtsp[0, :, :, :self.ns[r]].permute(0, 2, 1))
        k, v = torch.cat(ks, 1).double(), torch.cat(vs, 1).double()
        o = torch.softmax(q @ k.transpose(1, 2) * SCALE, -1) @ v                # (H, n, 128)
        o = o.permute(1, 0, 2).float().bfloat16().float()
        gate = torch.sigmoid(self.g[r, :n].reshape(n, H, HD).float()).bfloat16().float()
        return (o * gate).bfloat16().float()


def _tolerance_misses(got, ref):
    """got, ref (n, H, 128) fp32 -> the heads outside the tolerance, with their figures."""
    err = (got - ref).abs()
    worst = (err - ref.abs() * 2.0 ** -7).amax(dim=(0, 2))
    mean = err.mean(dim=(0, 2))
    return [(h, float(worst[h]), float(mean[h])) for h in range(got.shape[1]) if not (float(worst[h]) < 3e-2 and float(mean[h]) < 2e-3)]


def _check_parity(g, out, refs):
    o = g.view(out)
    for r in range(g.R):
        n = g.lens[r]
        bad = _tolerance_misses(o[r, :n].reshape(n, g.H, HD).float(), refs[r])
        assert not bad, f"{g.name} row {r} (length {n}): (head, max(err - |ref| 2^-7), mean err) outside 3e-2 / 2e-3: {bad[:4]}"


def _check_skipped_blocks(g, out):
    R, S, D = g.R, g.S, g.D
    assert bool((out[:, D:].float() == SENTINEL).all()), f"{g.name}: columns beyond the row of O were written"
    assert bool((out[R * S:].float() == SENTINEL).all()), f"{g.name}: rows beyond R * S of O were written"
    o = g.view(out)
    assert bool(torch.isfinite(o.float()).all()), f"{g.name}: NaN left in or written to O"
    nskipped = 0
    for r in range(R):
        q0 = g.first_skipped(r)
        nskipped += S - q0
        if _variant() != 4:          # attn4_kernel computes its padding blocks (launch_attention_bf16): finite, asserted above
            assert bool((o[r, q0:] == 0).all()), f"{g.name} row {r}: a block at or beyond the length {g.lens[r]} is not exactly 0"
    assert nskipped > 0, "the geometry skips no block"


# A: 128-query blocks (3 * 3 * 6 = 54 workgroups, one round), odd H; a row end before, at and after a block boundary and a length of 1;
#    rows 1 and 4 without text, row 2 without speaker; text 70 keys of which 65 are valid
# B: 5 * 16 * 6 = 480 > 256: 256-query blocks and the 88-query one-stream body [512, 600); Q, K, gate packed; rows 1 and 5 without text
def _geometry(name, plants=()):
    if name == "geoA":
        return Geometry("geoA", 6, 3, 300, [300, 100, 128, 129, 257, 1], 70, [65, 0, 65, 65, 0, 65], 33, [33, 33, 0, 33, 33, 33], False, 1.0, plants)
    return Geometry("geoB", 6, 16, 600, [600, 256, 257, 512, 513, 40], 70, [70, 0, 70, 70, 70, 0], 0, [0] * 6, True, 0.5, plants)


class Runs:
    """Every launch of one geometry, done once: full lengths (plain and length form) and the plain launch under the ragged key counts on
    the clean Q, then NaN into Q's skipped blocks and three launches of the length form."""

    def __init__(self, name):
        g = self.g = _geometry(name)
        full = [g.S] * g.R
        self.plain_full = g.launch(None, self_keys=full)
        self.len_full = g.launch(full, self_keys=full)
        self.plain = g.launch(None)
        g.poison_q()
        self.out = [g.launch(g.lens) for _ in range(3)]
        self.refs = [g.reference(r) for r in range(g.R)]


@pytest.fixture(scope="module", params=["geoA", "geoB"])
def runs(request):
    return Runs(request.param)


def test_entry_point_is_bound():
    lib = L.load_library()
    assert lib.echo_op_attention_bf16_len.argtypes == L.SIGNATURES["echo_op_attention_bf16_len"][1]
    assert lib.echo_abi_version() == 8


def test_parity_with_fp64_below_each_length(runs):
    """Every query below its row's length, every row and head, inside the tolerance of test_attention_bf16_joint_segments."""
    _check_parity(runs.g, runs.out[0], runs.refs)


def test_skipped_blocks_are_zero_and_nothing_else_is_touched(runs):
    """O starts as NaN, Q holds NaN in wholly skipped blocks: afterwards those blocks are exactly 0 (finite under ECHO_ATTN=4), O is finite
    inside R * S, and the sentinel columns and rows are untouched."""
    _check_skipped_blocks(runs.g, runs.out[0])


def test_bit_equal_with_the_plain_launch(runs):
    """The body is claimed unchanged: the plain launch under the same key counts gives the same bits at every query below its length, and
    with all lengths equal to S the whole O buffer is the same."""
    g = runs.g
    a, b = g.view(runs.out[0]), g.view(runs.plain)
    for r in range(g.R):
        assert torch.equal(a[r, :g.lens[r]], b[r, :g.lens[r]]), f"{g.name} row {r}"
    assert bool(torch.isfinite(runs.plain_full.float()).all())
    assert torch.equal(runs.len_full, runs.plain_full), g.name


def test_one_extra_self_key_is_seen(runs):
    """Teeth: the reference of a row with qlen[r] + 1 self keys (the finite padding key behind its end) is outside the tolerance for at
    least one ragged row, so the parity check can see a single key too many."""
    g = runs.g
    o = g.view(runs.out[0])
    seen = []
    for r in range(g.R):
        n = g.lens[r]
        if n < g.S and _tolerance_misses(o[r, :n].reshape(n, g.H, HD).float(), g.reference(r, extra_self_keys=1)):
            seen.append(r)
    assert seen, f"{g.name}: no ragged row tells qlen + 1 self keys from qlen"


def test_three_launches_are_bit_identical(runs):
    assert torch.equal(runs.out[0], runs.out[1]) and torch.equal(runs.out[0], runs.out[2]), runs.g.name


# (row, head, query, key), all below the row's length: a full block of a ragged row (row 3, length 512), straddling blocks (row 2, length
# 257: one valid query in [256, 512); row 5, length 40), and the short last block of row 0
PLANTS_B = [(3, 7, 300, 400), (2, 5, 256, 100), (5, 15, 10, 35), (0, 2, 580, 520)]


def test_range_fallback_under_lengths_geoB():
    """Geometry B with a caller-owned report buffer that starts as 1 in every word, and keys scoring 20 |q|^2.  A skipped block must write 0
    to its word: a stale flag would make attn_redo_kernel compute a padding block (from NaN queries here) into O.  The flagged set is the
    planted blocks (attn4_kernel, whose reference point a key in the first tile raises: a subset), each planted query returns its key's
    gated value row within 2e-2 (the bound of test_attention_range_fallback_many_blocks), and parity and the skipped blocks hold as above."""
    g = _geometry("geoB", PLANTS_B)
    g.poison_q()
    nwords = g.R * g.H * ((g.S + 127) // 128)
    redo = torch.ones((nwords,), dtype=torch.int32, device=DEV)
    out = g.launch(g.lens, redo=redo)
    if _variant() != 1:                                # attn_qlen_kernel writes no report words
        words = redo[:g.R * g.H * g.nb].view(g.R, g.H, g.nb)
        for r in range(g.R):
            assert not bool(words[r, :, (g.lens[r] + g.blk - 1) // g.blk:].any()), f"row {r}: the report word of a skipped block is not 0"
        planted = {(r, h, qi // g.blk) for (r, h, qi, _) in g.plants}
        seen = {tuple(int(x) for x in ix) for ix in torch.nonzero(words).tolist()}
        assert seen == planted if _variant() == 5 else seen <= planted, sorted(seen)
    _check_skipped_blocks(g, out)
    _check_parity(g, out, [g.reference(r) for r in range(g.R)])
    o = g.view(out)
    for (r, h, qi, kj) in g.plants:
        gate = torch.sigmoid(g.g[r, qi, h * HD:(h + 1) * HD].float()).bfloat16().float()
        want = (g.vt[r, h, :, kj].float() * gate).bfloat16().float()
        assert float((o[r, qi, h * HD:(h + 1) * HD].float() - want).abs().max()) < 2e-2, (r, h, qi)


def test_refusals_leave_a_valid_launch_working():
    """A length table together with causal, an e4m3 destination or a per-key bias, and a NULL table: each a non-zero status, nothing
    written; the plain entry point takes the causal / e4m3 / bias descriptors.  A valid launch afterwards gives the bits of one before."""
    g = _geometry("geoA")
    lib = U.lib()
    ql = torch.tensor(g.lens, dtype=torch.int32, device=DEV)
    before = g.launch(g.lens)
    out = g.o_fill.clone()
    o8 = torch.zeros((g.R * g.S, g.D), dtype=torch.uint8, device=DEV)
    bias = torch.zeros((1, g.Lt), device=DEV)

    def causal(d):
        d.nseg, d.causal = 1, 1

    def e4m3(d):
        d.O8, d.o8_ld, d.o8_row_stride, d.o8_inv = o8.data_ptr(), g.D, g.S * g.D, 16.0

    def seg_bias(d):
        d.seg[1].bias, d.seg[1].bias_row_stride = bias.data_ptr(), g.Lt

    for change in (causal, e4m3, seg_bias):
        d = g.desc(out, g.lens)
        change(d)
        assert lib.echo_op_attention_bf16_len(C.byref(d), ql.data_ptr(), U.stream()) != 0, change.__name__
        assert lib.echo_last_error(None), change.__name__
    d = g.desc(out, g.lens)
    assert lib.echo_op_attention_bf16_len(C.byref(d), None, U.stream()) != 0
    assert b"length table" in lib.echo_last_error(None)
    torch.cuda.synchronize()
    assert bool((out[:g.R * g.S, :g.D] != out[:g.R * g.S, :g.D]).all()) and not bool(o8.any()), "a refused launch wrote its output"
    scratch = g.o_fill.clone()
    for change in (causal, e4m3, seg_bias):            # the same descriptors without a table are legal: the table is what is refused
        d = g.desc(scratch, g.lens)
        change(d)
        L.check(lib.echo_op_attention_bf16(C.byref(d), U.stream()))
    torch.cuda.synchronize()
    assert torch.equal(g.launch(g.lens), before)


# ------------------------------------------------------------------------------------------------ the other kernels, in child processes
HERE = os.path.abspath(__file__)
ENGINE_LEVEL = os.path.join(os.path.dirname(HERE), "test_gpu_item_lengths.py")
VARIANTS = [
    # id, environment, module, -k
    ("attn1", dict(ECHO_ATTN="1"), HERE, None),                                  # attn_qlen_kernel
    ("attn4", dict(ECHO_ATTN="4"), HERE, None),                                  # attn4_kernel: computes its padding blocks
    ("attn5", dict(ECHO_ATTN="5"), HERE, None),
    ("attn5-256-geoA", dict(ECHO_ATTN="5", ECHO_ATTN_Q128="0"), HERE, "geoA"),   # both block sizes see both shapes
    ("attn5-128-geoB", dict(ECHO_ATTN="5", ECHO_ATTN_Q128="1"), HERE, "geoB"),
    # attn_qlen_kernel inside a forward
    ("attn1-engine", dict(ECHO_ATTN="1"), ENGINE_LEVEL, "padding_independence or stale_workspace or block_skipping or skipped_256"),
]


@pytest.mark.parametrize("env,module,select", [v[1:] for v in VARIANTS], ids=[v[0] for v in VARIANTS])
def test_length_forms_under_forced_kernels(env, module, select):
    """The switches are read once per process, at the first launch: every variant is a fresh pytest process."""
    if os.environ.get("ECHO_ATTN"):
        pytest.skip("already a variant run")
    root = os.path.dirname(os.path.dirname(HERE))
    cmd = [sys.executable, "-m", "pytest", module, "-m", "gpu", "-q", "-x"] + (["-k", select] if select else [])
    r = subprocess.run(cmd, env=dict(os.environ, **env), cwd=root, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and " passed" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]
