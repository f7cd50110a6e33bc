"""GPU: a forward whose rows are described by a map (echo_dit_forward_rows, EchoDiT.forward(row_item=)).

TINY model, S = 32, B = 3 items, both engines.  Row r uses the position, length, text and speaker KV of item row_item[r]; the number of rows
is free.  Asserted:
  - the rectangular map (row_item[r] = r % B) gives the bits of echo_dit_forward_t / _pos / _len;
  - two 7-row forwards agree, bit for bit, on every row that has the same (item, flags, x), wherever it stands (item 1 owns three rows, item 2
    one); the launches are the same (same M), so this is row-permutation equivariance;
  - each row against the oracle's batch-1 forward of its item: fp32 engine rms < 1e-4 x max(1, rms(want)), bf16 engine < 1.5 x the bf16
    oracle's own distance to fp32 + 1e-3 (the constants of tests/test_gpu_engine.py::test_forward_with_per_row_timesteps);
  - positions and lengths on top, NaN in the padding of x; a wrong map entry is seen by the oracle check; the refusals."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import echo_ref as R  # noqa: E402  (checker only)
from tests import gpu_util as U  # noqa: E402
from tests.golden_defs import TINY  # noqa: E402

import echo_tts_amd as E  # noqa: E402
from echo_tts_amd import _lib as L  # noqa: E402

DEV = U.DEV
B, S = 3, 32
ENGINES = ["f32", "bf16"]
# (item, text on, speaker on): item 1 three times, item 2 once, item 0 three times; every flag pair occurs
ROWS_A = [(1, 1, 1), (0, 1, 1), (1, 0, 1), (2, 1, 1), (0, 1, 0), (1, 1, 0), (0, 0, 1)]
PERM = [3, 6, 0, 5, 1, 2, 4]          # arrangement two: row i of it is row PERM[i] of arrangement one
POSITIONS = [0, 5, 13]
LENGTHS = [32, 20, 7]


def rms(a, b):
    return float((a.float().cpu() - b.float().cpu()).pow(2).mean().sqrt())


class Setup:
    def __init__(self, dname):
        self.dt = torch.float32 if dname == "f32" else torch.bfloat16
        self.w = R.make_dit_weights(TINY, seed=0)
        self.wd = self.w if dname == "f32" else {k: v.bfloat16() for k, v in self.w.items()}
        self.m = E.EchoDiT(TINY, self.wd, dtype=self.dt, device=DEV)
        gen = torch.Generator().manual_seed(21)
        self.ids = torch.randint(1, 256, (B, 24), generator=gen, dtype=torch.int32)
        self.tm = torch.zeros((B, 24), dtype=torch.bool)
        self.sm = torch.zeros((B, 16), dtype=torch.bool)
        for b in range(B):
            self.tm[b, :24 - 5 * b] = True
            self.sm[b, :16 - 4 * b] = True
        self.spk = torch.randn((B, 16, 80), generator=gen)
        self.x = torch.randn((9, S, 80), generator=gen)          # one x per row; rows take x[id]
        self.kvt = self.m.get_kv_cache_text(self.ids, self.tm)
        self.kvs = self.m.get_kv_cache_speaker(self.spk.to(self.dt), self.sm)
        self._okv = {}

    def masks(self, rows):
        tm = torch.stack([self.tm[b] if ton else torch.zeros_like(self.tm[b]) for (b, ton, _) in rows])
        sm = torch.stack([self.sm[b] if son else torch.zeros_like(self.sm[b]) for (b, _, son) in rows])
        return tm, sm

    def forward(self, rows, xids, row_item="map", **kw):
        tm, sm = self.masks(rows)
        ri = [b for (b, _, _) in rows] if row_item == "map" else row_item
        t = torch.full((len(rows),), 0.75)
        return self.m(self.x[xids].to(self.dt), t.to(self.dt), tm, sm, self.kvt, self.kvs, row_item=ri, **kw).float().cpu()

    def oracle(self, w, row, xid, pos=0, n=S):
        """batch-1 oracle forward of one row: item `row[0]` alone, its flags, x[xid][:n] at start position pos."""
        b, ton, son = row
        dt = next(iter(w.values())).dtype
        key = (dt, b)
        if key not in self._okv:
            self._okv[key] = (R.kv_cache_text(w, TINY, self.ids[b:b + 1], self.tm[b:b + 1]), R.kv_cache_speaker(w, TINY, self.spk[b:b + 1].to(dt)))
        kvt, kvs = self._okv[key]
        tm = self.tm[b:b + 1] if ton else torch.zeros_like(self.tm[b:b + 1])
        sm = self.sm[b:b + 1] if son else torch.zeros_like(self.sm[b:b + 1])
        return R.dit_forward(w, TINY, self.x[xid:xid + 1, :n].to(dt), torch.full((1,), 0.75).to(dt), tm, sm, kvt, kvs, start_pos=pos)[0].float()

    def oracle_miss(self, got_row, row, xid, pos=0, n=S):
        """None when got_row is inside the engine's tolerance of the oracle, else the figures."""
        want = self.oracle(self.w, row, xid, pos, n)
        e = rms(got_row[:n], want)
        if self.dt == torch.float32:
            bound = 1e-4 * max(1.0, U.rms(want))
        else:
            bound = 1.5 * rms(self.oracle(self.wd, row, xid, pos, n), want) + 1e-3
        return None if e < bound else (e, bound)


@pytest.fixture(scope="module", params=ENGINES)
def su(request):
    return Setup(request.param)


def test_entry_points_are_bound():
    lib = L.load_library()
    for name in ("echo_dit_forward_rows", "echo_sample_euler_items_compact", "echo_debug_last_row_forwards"):
        assert getattr(lib, name).argtypes == L.SIGNATURES[name][1]
    assert lib.echo_abi_version() == 8


def test_rectangular_map_equals_the_existing_forwards(su):
    """rows = 2 B in the r % B layout (second copy text-uncond): without tables, with positions, with positions and lengths."""
    rows = [(b, 1, 1) for b in range(B)] + [(b, 0, 1) for b in range(B)]
    xids = list(range(6))
    for kw in (dict(), dict(start_pos=POSITIONS), dict(start_pos=POSITIONS, lengths=LENGTHS), dict(lengths=LENGTHS)):
        a = su.forward(rows, xids, row_item=None, **kw)
        b = su.forward(rows, xids, **kw)
        assert bool(torch.isfinite(a).all()) and float(a.abs().max()) > 0
        assert torch.equal(a, b), kw


def test_rows_agree_wherever_they_stand_and_with_the_oracle(su):
    """7 rows, two arrangements: bit-equal row by row; every row inside the tolerance of its item's batch-1 oracle forward."""
    xa = list(range(7))
    a = su.forward(ROWS_A, xa)
    b = su.forward([ROWS_A[i] for i in PERM], [xa[i] for i in PERM])
    assert bool(torch.isfinite(a).all())
    for i, src in enumerate(PERM):
        assert torch.equal(b[i], a[src]), f"row {src} of arrangement one moved to {i} and changed"
    for r, row in enumerate(ROWS_A):
        miss = su.oracle_miss(a[r], row, xa[r])
        assert miss is None, f"row {r} {row}: rms against the oracle, bound: {miss}"
    # rows of one item with different flags are different outputs (the flags reach the attention)
    assert not torch.equal(su.forward([(1, 1, 1), (1, 0, 1)], [0, 0])[0], su.forward([(1, 1, 1), (1, 0, 1)], [0, 0])[1])


def test_positions_and_lengths_with_nan_padding(su):
    """Per-item positions and lengths through the map; x holds NaN in the padding of every row.  Valid tokens: finite, bit-equal between the
    arrangements and inside the oracle's tolerance at (position, length) of the row's item; padding of the result: exactly 0."""
    x_keep = su.x.clone()
    try:
        for r, (b, _, _) in enumerate(ROWS_A):
            su.x[r, LENGTHS[b]:] = float("nan")
        xa = list(range(7))
        kw = dict(start_pos=POSITIONS, lengths=LENGTHS)
        a = su.forward(ROWS_A, xa, **kw)
        b2 = su.forward([ROWS_A[i] for i in PERM], [xa[i] for i in PERM], **kw)
        assert bool(torch.isfinite(a).all())
        for i, src in enumerate(PERM):
            assert torch.equal(b2[i], a[src]), f"row {src}"
        for r, row in enumerate(ROWS_A):
            n = LENGTHS[row[0]]
            assert bool((a[r, n:] == 0).all()), f"row {r}: padding of the result is not exactly 0"
            assert float(a[r, :n].abs().max()) > 0
            miss = su.oracle_miss(a[r], row, xa[r], POSITIONS[row[0]], n)
            assert miss is None, f"row {r} {row}: {miss}"
    finally:
        su.x.copy_(x_keep)


def test_a_wrong_map_entry_is_detected(su):
    """Row 3 belongs to item 2.  Mapped to item 0 (with item 0's masks, so that the host check passes) that row - and no other - leaves the
    bits of the right map, and it is item 0's row: inside the oracle's tolerance for item 0.  The fp32 engine's oracle check for item 2
    rejects it; the bf16 bound (1.5 x the bf16 oracle's own distance + 1e-3) is too wide to tell two texts apart on TINY's random weights
    (DESIGN.md 3.14 measured the same for timesteps), so there the figures are printed and the bit comparison is the detector.  With item
    2's masks the host refuses the mismatch between the row's mask and its item's cached mask."""
    xa = list(range(7))
    wrong = list(ROWS_A)
    wrong[3] = (0, 1, 1)
    right, got = su.forward(ROWS_A, xa), su.forward(wrong, xa)
    for r in range(7):
        assert torch.equal(got[r], right[r]) == (r != 3), f"row {r}"
    assert su.oracle_miss(got[3], wrong[3], xa[3]) is None
    miss = su.oracle_miss(got[3], ROWS_A[3], xa[3])
    print(f"wrong map entry, {su.dt}: rms of row 3 against item 2's oracle {rms(got[3], su.oracle(su.w, ROWS_A[3], xa[3])):.3e}, outside the bound: {miss}")
    if su.dt == torch.float32:
        assert miss is not None, "item 0's keys passed for item 2's"
    ri = [b for (b, _, _) in wrong]
    with pytest.raises(NotImplementedError):
        su.forward(ROWS_A, xa, row_item=ri)


def test_refusals(su):
    m = su.m
    off = [(b, 0, 0) for (b, _, _) in ROWS_A]          # all-False masks: the host has no cached mask to compare, the engine sees the map
    with pytest.raises(L.EchoHipError, match="row_item entry is out of range"):
        su.forward(off, list(range(7)), row_item=[0, 1, 2, 3, 0, 1, 2])
    with pytest.raises(L.EchoHipError, match="row_item entry is out of range"):
        su.forward(off, list(range(7)), row_item=[0, 1, 2, -1, 0, 1, 2])
    with pytest.raises(ValueError):
        su.forward(ROWS_A, list(range(7)), row_item=[0, 1, 2])
    rows97 = [(0, 1, 1)] * 97
    with pytest.raises(L.EchoHipError, match="rows <= 96"):
        su.forward(rows97, [0] * 97)
    # a NULL map at the C boundary
    i32 = C.c_int32
    st = m._lib.echo_dit_forward_rows(m._ctx, None, None, 1, None, 3, B, S, None, None, None, 0, (i32 * 3)(1, 1, 1), (i32 * 3)(1, 1, 1), None, m._stream())
    assert st != 0 and b"row_item" in m._lib.echo_last_error(m._ctx)
    # the context stays usable
    assert bool(torch.isfinite(su.forward(ROWS_A, list(range(7)))).all())


def test_non_prefix_mask_with_lengths_is_refused(su):
    """A text mask with a hole gives the cache a per-key bias: the length forms of the attention do not exist for it, under a map either;
    without lengths the map runs on the biased kernel."""
    m = su.m
    tm = su.tm.clone()
    tm[1, 3] = False
    try:
        kvt = m.get_kv_cache_text(su.ids, tm)
        rows = [(1, 1, 1), (0, 1, 1), (1, 1, 1)]
        tmr = torch.stack([tm[b] for (b, _, _) in rows])
        smr = torch.stack([su.sm[b] for (b, _, _) in rows])
        t = torch.full((3,), 0.75).to(su.dt)
        with pytest.raises(L.EchoHipError, match="not a prefix"):
            m(su.x[:3].to(su.dt), t, tmr, smr, kvt, su.kvs, row_item=[1, 0, 1], lengths=LENGTHS)
        out = m(su.x[[0, 1, 0]].to(su.dt), t, tmr, smr, kvt, su.kvs, row_item=[1, 0, 1]).float().cpu()
        assert bool(torch.isfinite(out).all()) and torch.equal(out[0], out[2])
    finally:
        su.kvt = m.get_kv_cache_text(su.ids, su.tm)


def test_fp8_context_is_refused():
    w = {k: v.bfloat16() for k, v in R.make_dit_weights(TINY, seed=0).items()}
    m8 = E.EchoDiT(TINY, w, dtype=torch.bfloat16, device=DEV, fp8=True)
    ids = torch.randint(1, 256, (1, 24), dtype=torch.int32)
    tm, sm = torch.ones((1, 24), dtype=torch.bool), torch.ones((1, 16), dtype=torch.bool)
    kvt, kvs = m8.get_kv_cache_text(ids, tm), m8.get_kv_cache_speaker(torch.randn((1, 16, 80)).bfloat16(), sm)
    x = torch.randn((2, S, 80)).bfloat16()
    with pytest.raises(L.EchoHipError, match="fp8 engine"):
        m8(x, torch.full((2,), 0.75).bfloat16(), tm.expand(2, -1), sm.expand(2, -1), kvt, kvs, row_item=[0, 0])
