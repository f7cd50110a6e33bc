"""GPU: the joint attention under a row map (AttnArgs.row_item) at kernel level, through echo_op_attention_bf16_rows.

A launch has R = 6 rows; the shared segments (kv_mod > 0) hold one KV row per ITEM and row r reads the KV of item MAP[r] % kv_mod.  Segments:
self (kv_mod 0, per row) | latent (kv_mod 2) | text (kv_mod 3) | speaker (kv_mod 1), with unequal key counts per row.

The claim is bit equality, so the reference is the existing kernel itself: echo_op_attention_bf16 / _len run on KV that was physically
gathered for every row (kv_mod 0 in every segment, row r's K / V^T / bias = those of its item).  Both launches have the same grid, the
same key counts and the same values at every address the kernel reads.

The two geometries are those of tests/test_gpu_attention_len.py (128-query blocks of attn_kernel / attn5's one-stream body; attn5's 256-query
blocks and its short last block).  Which kernel runs is decided once per process by ECHO_ATTN; test_row_map_under_forced_kernels repeats the
module in child processes under ECHO_ATTN = 1, 4 and 5."""
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
MAP = [2, 0, 1, 1, 0, 2]
# (name, kv_mod, keys in the cache, key count per row); a count of 0 switches the segment off for that row
SHARED = [("latent", 2, 40, [40, 17, 0, 33, 40, 1]), ("text", 3, 70, [65, 0, 70, 64, 3, 70]), ("speaker", 1, 33, [33, 33, 0, 33, 20, 33])]


def _rnd(*shape, scale=1.0, seed=0):
    g = torch.Generator().manual_seed(seed + sum(shape))
    return (torch.randn(shape, generator=g) * scale).bfloat16().to(DEV)


class Geometry:
    def __init__(self, name, R, H, S, lens):
        self.name, self.R, self.H, self.S, self.lens = name, R, H, S, lens
        D = self.D = H * HD
        self.pS = (S + 63) // 64 * 64
        self.q, self.k, self.g = _rnd(R, S, D), _rnd(R, S, D, seed=1), _rnd(R, S, D, seed=7)
        self.vt = _rnd(R, H, HD, self.pS, seed=2)
        self.shared = []
        for i, (_, mod, n, _) in enumerate(SHARED):
            pitch = (n + 63) // 64 * 64
            k = _rnd(mod, n + 64, D, seed=10 + i)              # (item, key, D); 64 finite rows behind the last key
            vt = _rnd(mod, H, HD, pitch, seed=20 + i)          # (item, head, d, key)
            self.shared.append((k, vt, pitch))
        # per-key bias of the text segment: 0 / -inf, another pattern per item, key 0 always open
        gen = torch.Generator().manual_seed(5)
        open_ = torch.rand((3, 70), generator=gen) > 0.3
        open_[:, 0] = True
        self.text_bias = torch.where(open_, 0.0, float("-inf")).float().to(DEV)
        self._keep = []

    def desc(self, out, row_map, gathered, self_keys, bias=False):
        """gathered=False: the caches as they are, kv_mod per segment (the launch under a map).  True: row r's own copy of its item's K,
        V^T and bias, kv_mod 0 everywhere (the reference launch)."""
        R, H, S, D = self.R, self.H, self.S, self.D
        nk = torch.tensor([list(self_keys)] + [c for (_, _, _, c) in SHARED], dtype=torch.int32, device=DEV)
        self._keep.append(nk)
        d = L.EchoAttnDesc()
        d.Q, d.q_ld, d.q_row_stride = self.q.data_ptr(), D, S * D
        d.G, d.g_ld, d.g_row_stride = self.g.data_ptr(), D, S * D
        d.O, d.o_ld, d.o_row_stride = out.data_ptr(), D, S * D
        d.S, d.H, d.rows, d.nseg, d.causal, d.scale = S, H, R, 4, 0, SCALE
        sg = d.seg[0]
        sg.K, sg.k_ld, sg.k_head_stride, sg.k_row_stride = self.k.data_ptr(), D, HD, S * D
        sg.Vt, sg.vt_ld, sg.vt_head_stride, sg.vt_row_stride = self.vt.data_ptr(), self.pS, HD * self.pS, H * HD * self.pS
        sg.nkeys, sg.kv_mod = nk[0].data_ptr(), 0
        for i, ((name, mod, n, _), (k, vt, pitch)) in enumerate(zip(SHARED, self.shared)):
            b = self.text_bias if bias and name == "text" else None
            if gathered:
                idx = torch.tensor([m % mod for m in row_map], device=DEV)
                k, vt = k[idx].contiguous(), vt[idx].contiguous()
                b = b[idx].contiguous() if b is not None else None
                self._keep += [k, vt, b]
            sg = d.seg[1 + i]
            sg.K, sg.k_ld, sg.k_head_stride, sg.k_row_stride = k.data_ptr(), D, HD, (n + 64) * D
            sg.Vt, sg.vt_ld, sg.vt_head_stride, sg.vt_row_stride = vt.data_ptr(), pitch, HD * pitch, H * HD * pitch
            sg.nkeys, sg.kv_mod = nk[1 + i].data_ptr(), 0 if gathered else mod
            if b is not None:
                sg.bias, sg.bias_row_stride = b.data_ptr(), b.shape[1]
        return d

    def launch(self, row_map, gathered, qlen=None, bias=False):
        R, S, D = self.R, self.S, self.D
        out = torch.full((R, S, D), float("nan"), dtype=torch.bfloat16, device=DEV)
        self_keys = self.lens if qlen is not None else [S] * R
        d = self.desc(out, row_map, gathered, self_keys, bias)
        ql = torch.tensor(list(qlen), dtype=torch.int32, device=DEV) if qlen is not None else None
        lib = U.lib()
        if gathered:
            if ql is None:
                L.check(lib.echo_op_attention_bf16(C.byref(d), U.stream()))
            else:
                L.check(lib.echo_op_attention_bf16_len(C.byref(d), ql.data_ptr(), U.stream()))
        else:
            m = torch.tensor(list(row_map), dtype=torch.int32, device=DEV)
            L.check(lib.echo_op_attention_bf16_rows(C.byref(d), m.data_ptr(), ql.data_ptr() if ql is not None else None, U.stream()))
        torch.cuda.synchronize()
        return out


def _geometry(name):
    if name == "geoA":
        return Geometry("geoA", 6, 3, 300, [300, 100, 128, 129, 257, 1])
    return Geometry("geoB", 6, 16, 600, [600, 256, 257, 512, 513, 40])


@pytest.fixture(scope="module", params=["geoA", "geoB"])
def geo(request):
    return _geometry(request.param)


def test_entry_point_is_bound():
    lib = L.load_library()
    assert lib.echo_op_attention_bf16_rows.argtypes == L.SIGNATURES["echo_op_attention_bf16_rows"][1]
    assert lib.echo_abi_version() == 8


def test_bit_equal_with_gathered_kv(geo):
    """Without a length table: every row equals the existing kernel on KV gathered for that row; the result is finite everywhere."""
    got, want = geo.launch(MAP, False), geo.launch(MAP, True)
    assert bool(torch.isfinite(got.float()).all())
    for r in range(geo.R):
        assert torch.equal(got[r], want[r]), f"{geo.name} row {r}"


def test_bit_equal_with_gathered_kv_under_lengths(geo):
    """With a length table (qlen = the self key counts, as the engine sets them): equal to echo_op_attention_bf16_len on gathered KV, the
    skipped blocks included."""
    got, want = geo.launch(MAP, False, qlen=geo.lens), geo.launch(MAP, True, qlen=geo.lens)
    for r in range(geo.R):
        n = geo.lens[r]
        assert bool(torch.isfinite(got[r, :n].float()).all())
        assert torch.equal(got[r, :n], want[r, :n]), f"{geo.name} row {r}"
    assert torch.equal(got.view(torch.int16), want.view(torch.int16)), geo.name      # padding blocks too, bit for bit (NaN-safe compare)


def test_bit_equal_with_gathered_kv_and_bias(geo):
    """A per-key bias (the biased attn_kernel) is indexed by the item's KV row as well."""
    got, want = geo.launch(MAP, False, bias=True), geo.launch(MAP, True, bias=True)
    assert bool(torch.isfinite(got.float()).all())
    assert torch.equal(got, want), geo.name
    assert not torch.equal(got, geo.launch(MAP, False)), "the bias changed nothing: the check has no teeth"


def test_one_map_entry_changes_that_row_only(geo):
    """Control: row 3 moved from item 1 to item 0 - that row changes (its text and latent keys are another item's), no other row does."""
    other = list(MAP)
    other[3] = 0
    a, b = geo.launch(MAP, False), geo.launch(other, False)
    for r in range(geo.R):
        if r == 3:
            assert not torch.equal(a[r], b[r]), "row 3 did not notice its new item"
        else:
            assert torch.equal(a[r], b[r]), f"row {r} changed with another row's map entry"
    assert torch.equal(b[3], geo.launch(other, True)[3])


def test_identity_map_equals_the_plain_launch(geo):
    """row_item[r] = r is the arithmetic of a launch without a map (kvrow = r % kv_mod)."""
    ident = list(range(geo.R))
    out = torch.full((geo.R, geo.S, geo.D), float("nan"), dtype=torch.bfloat16, device=DEV)
    d = geo.desc(out, ident, False, [geo.S] * geo.R)
    L.check(U.lib().echo_op_attention_bf16(C.byref(d), U.stream()))
    torch.cuda.synchronize()
    assert torch.equal(out, geo.launch(ident, False))


def test_refusals_return_a_status_and_a_message():
    g = _geometry("geoA")
    lib = U.lib()
    m = torch.tensor(MAP, dtype=torch.int32, device=DEV)
    before = g.launch(MAP, False)
    out = torch.full((g.R, g.S, g.D), float("nan"), dtype=torch.bfloat16, device=DEV)
    o8 = torch.zeros((g.R * g.S, g.D), dtype=torch.uint8, device=DEV)
    prof = torch.zeros((1 << 16,), dtype=torch.int64, device=DEV)

    def causal(d):
        d.nseg, d.causal = 1, 1

    def e4m3(d):
        d.O8, d.o8_ld, d.o8_row_stride, d.o8_inv = o8.data_ptr(), g.D, g.S * g.D, 16.0

    def profiled(d):
        d.prof = prof.data_ptr()

    for change in (causal, e4m3, profiled):
        d = g.desc(out, MAP, False, [g.S] * g.R)
        change(d)
        assert lib.echo_op_attention_bf16_rows(C.byref(d), m.data_ptr(), None, U.stream()) != 0, change.__name__
        assert b"row map" in lib.echo_last_error(None), change.__name__
    d = g.desc(out, MAP, False, [g.S] * g.R)
    assert lib.echo_op_attention_bf16_rows(C.byref(d), None, None, U.stream()) != 0
    assert b"row map" in lib.echo_last_error(None)
    torch.cuda.synchronize()
    assert bool((out != out).all()) and not bool(o8.any()) and not bool(prof.any()), "a refused launch wrote something"
    assert torch.equal(g.launch(MAP, False), before)


HERE = os.path.abspath(__file__)


@pytest.mark.parametrize("variant", ["1", "4", "5"])
def test_row_map_under_forced_kernels(variant):
    """ECHO_ATTN is read once per process, at the first launch: every variant is a fresh pytest process."""
    if os.environ.get("ECHO_ATTN"):
        pytest.skip("already a variant run")
    root = os.path.dirname(os.path.dirname(HERE))
    cmd = [sys.executable, "-m", "pytest", HERE, "-m", "gpu", "-q", "-x"]
    r = subprocess.run(cmd, env=dict(os.environ, ECHO_ATTN=variant), cwd=root, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and " passed" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]
