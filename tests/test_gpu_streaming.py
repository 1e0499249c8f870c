"""-m gpu: the streaming and row-movement kernels (csrc/scn_elem.hip, scn_elem_bf16.hip, scn_segpool.hip, the column sum of
scn_conv.hip) on every launcher path, against the plain float64 restatement in tests/stream_restate.py (pinned on the CPU by
tests/test_stream_restate_cpu.py) or against torch on the same bits.

What the other files cannot reach and this one does:
  * the SCALAR bodies that `ew_launch`, both row gathers and both casts select from the pointer alignment (every torch
    allocation is 256-byte aligned; the executor's arena and the flat parameter buffer hand out interior pointers);
  * the second trip of the grid-stride loops (`scn::ew_grid` caps a grid at 2048 x 256 threads);
  * bf16 pooling, SparseToDense and the scalar bf16 gather;
  * the max-pool gradient at ties (every tied child receives the full dY) and at a -0 / +0 pair, in both storages;
  * column sums wider than 256 columns, n = 0 and n around 8 * COLSUM_BLOCKS;
  * per-sample pooling at 64-column passes, sample boundaries seen by each row lane, all-negative / tied / signed-zero maxima;
  * the casts at exact rounding ties, overflow, denormals, signed zeros and NaN.

Raw entry points run inside a larger buffer whose guard regions (sentinel bytes before and after each output) must come
back bit-unchanged; an output's own bytes start as sentinels too, so an element the kernel skips is seen.  Misaligned
pointers (one element off a 256-byte boundary: still naturally aligned for the element type) go ONLY to entry points whose
launcher inspects alignment.

Every tolerance is derived from the kernel's stated arithmetic (u = 2^-24, the fp32 unit roundoff; one bf16 rounding: 2^-8 relative);
each bounded test prints its worst measured error as a fraction of its bound (`[margin]` lines; DESIGN.md section 2 records them).
"""
import itertools

import numpy as np
import pytest
import torch

import stream_restate as R
from oracle import scn_oracle as O

pytestmark = pytest.mark.gpu

U32 = 2.0 ** -24                 # fp32 unit roundoff
UB16 = 2.0 ** -8                 # bf16 unit roundoff: 8 significant bits, half an ulp is at most 2^-8 of the value
EW_THREADS = 2048 * 256          # scn::ew_grid: at most 2048 blocks of 256 threads, then the loops stride
GUARD, SENT = 512, 0xA5


def _scn():
    import sparse_rcnn_amd as scn
    return scn


def _L():
    from sparse_rcnn_amd import _lib as L
    return L


class Buf:
    """`count` elements of `dtype` inside a sentinel-filled byte buffer; the data starts `off` elements past a 256-byte
    boundary.  `.t` views the data, `.ptr` is its address, `.intact()` says whether every byte outside it is untouched."""

    def __init__(self, dev, dtype, count, off=0, fill=None):
        isz = torch.empty((), dtype=dtype).element_size()
        self.lo = GUARD + off * isz
        self.hi = self.lo + int(count) * isz
        self.raw = torch.full((self.hi + GUARD,), SENT, dtype=torch.uint8, device=dev)
        assert self.raw.data_ptr() % 256 == 0
        self.t = self.raw[self.lo:self.hi].view(dtype)
        if fill is not None:
            self.t.copy_(fill.reshape(-1))
        self.ptr = self.raw.data_ptr() + self.lo

    def intact(self):
        return bool((self.raw[:self.lo] == SENT).all()) and bool((self.raw[self.hi:] == SENT).all())


_INT = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}


def _bits(t):
    return t.contiguous().view(_INT[t.element_size()])


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _np_bits(a):
    a = np.ascontiguousarray(a)
    return a.view({2: np.uint16, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def _bf16_np(t):
    """bf16 tensor -> numpy uint16 bit patterns."""
    return t.detach().contiguous().view(torch.int16).cpu().numpy().view(np.uint16)


# ------------------------------------------------------------------------------------------------------------------------
# ReLU forward / backward, add (fp32: k_ew, vector and scalar body), add (bf16)
# ------------------------------------------------------------------------------------------------------------------------
EW_COUNTS = [0, 1, 3, 4, 5, 255, 256, 257, 1023, 1024, 1025, 4 * EW_THREADS + 4 * 300 + 3]
_SPECIAL = [0.0, -0.0, float("inf"), -float("inf"), 1e-40, -1e-40, 1.4e-45]


def _with_specials(n, seed, shift):
    """randn with +-0, +-inf and denormals at the positions i with (i + shift) % 29 < 7 (two operands with shifts 0 and 10
    never hold a special at the same position: no inf - inf)."""
    x = torch.randn(n, generator=torch.Generator().manual_seed(seed))
    k = (torch.arange(n) + shift) % 29
    m = k < len(_SPECIAL)
    x[m] = torch.tensor(_SPECIAL)[k[m]]
    return x


@pytest.fixture(scope="module")
def ew_operands(gpu):
    n = EW_COUNTS[-1]
    return _with_specials(n, 1, 0).to(gpu), _with_specials(n, 2, 10).to(gpu)


@pytest.mark.parametrize("op", ["relu_fwd", "relu_bwd", "add"])
def test_relu_and_add_fp32_vector_and_scalar_bodies(gpu, ew_operands, op):
    """scn_relu_fwd / scn_relu_bwd / scn_add: all operands aligned (float4 body + scalar tail) and each operand in turn one
    float off (scalar body); counts around the float4 width, the block and one that sends both bodies round their loop more
    than once (with a remainder of 3).  relu_bwd and add bit-equal to torch; relu_fwd equal as values (sign of 0 not pinned)."""
    L = _L()
    lib = L.lib()
    A, B = ew_operands
    offs = [(0, 0, 0), (1, 0, 0), (0, 0, 1)] + ([] if op == "relu_fwd" else [(0, 1, 0)])
    for count, (oa, ob, oy) in itertools.product(EW_COUNTS, offs):
        a, b = Buf(gpu, torch.float32, count, oa, A[:count]), Buf(gpu, torch.float32, count, ob, B[:count])
        y = Buf(gpu, torch.float32, count, oy)
        if op == "relu_fwd":
            L.check(lib.scn_relu_fwd(a.ptr, count, y.ptr, L.stream()))
            assert torch.equal(y.t, torch.relu(a.t)), (op, count, oa, oy)
        elif op == "relu_bwd":
            L.check(lib.scn_relu_bwd(a.ptr, b.ptr, count, y.ptr, L.stream()))
            assert _same_bits(y.t, torch.where(a.t > 0, b.t, torch.zeros_like(b.t))), (op, count, oa, ob, oy)
        else:
            L.check(lib.scn_add(a.ptr, b.ptr, count, y.ptr, L.stream()))
            assert _same_bits(y.t, a.t + b.t), (op, count, oa, ob, oy)
        assert y.intact() and a.intact() and b.intact(), ("guard", op, count, oa, ob, oy)


def test_add_bf16_equals_torch_bit_for_bit(gpu, ew_operands):
    L = _L()
    lib = L.lib()
    A, B = (t.to(torch.bfloat16) for t in ew_operands)
    for count in EW_COUNTS:
        a, b = Buf(gpu, torch.bfloat16, count, 0, A[:count]), Buf(gpu, torch.bfloat16, count, 0, B[:count])
        y = Buf(gpu, torch.bfloat16, count)
        L.check(lib.scn_add_bf16(a.ptr, b.ptr, count, y.ptr, L.stream()))
        assert _same_bits(y.t, a.t + b.t), count
        assert y.intact(), count


# ------------------------------------------------------------------------------------------------------------------------
# row gather (fp32 / bf16): a byte copy of rows
# ------------------------------------------------------------------------------------------------------------------------
WIDTHS = [1, 3, 4, 7, 8, 12, 24, 33, 64]


@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("c", WIDTHS)
def test_row_gather_vector_and_scalar_bodies(gpu, c, bf16):
    """scn_gather_rows / scn_gather_rows_bf16: 16-byte pieces when c allows it and X, Y are 16-byte aligned, else one element
    per thread; m = 0, 1, around a block, and one m that sends the body taken round its loop twice; repeated, descending and
    random row lists; X or Y one element off.  The slab holds random BIT patterns (NaN payloads too): a gather copies bytes."""
    L = _L()
    lib = L.lib()
    dt = torch.int16 if bf16 else torch.int32
    entry = lib.scn_gather_rows_bf16 if bf16 else lib.scn_gather_rows
    V = 8 if bf16 else 4
    n_src = 257
    g = torch.Generator().manual_seed(c)
    src = torch.randint(-2 ** 15, 2 ** 15, (n_src, c), generator=g).to(dt) if bf16 else \
        torch.randint(-2 ** 31, 2 ** 31, (n_src, c), generator=g).to(dt)
    src = src.to(gpu)
    for ox, oy in [(0, 0), (1, 0), (0, 1)]:
        vec = c % V == 0 and ox == 0 and oy == 0
        m_twice = EW_THREADS // (c // V if vec else c) + 300
        X = Buf(gpu, dt, n_src * c, ox, src)
        for m in (0, 1, 255, 257, m_twice):
            i = torch.arange(m)
            lists = {"repeated": (i // 3) % n_src, "descending": n_src - 1 - i % n_src,
                     "random": torch.randint(0, n_src, (m,), generator=g)}
            for name, rows in lists.items():
                rows = Buf(gpu, torch.int32, m, 0, rows.to(torch.int32).to(gpu))
                Y = Buf(gpu, dt, m * c, oy)
                L.check(entry(X.ptr, rows.ptr, m, c, Y.ptr, L.stream()))
                assert torch.equal(Y.t.view(m, c), X.t.view(n_src, c)[rows.t.long()]), (c, m, name, ox, oy)
                assert Y.intact() and X.intact(), ("guard", c, m, name, ox, oy)


# ------------------------------------------------------------------------------------------------------------------------
# segment sum (fp32 / bf16)
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("c", WIDTHS)
def test_segment_sum_equals_the_float64_sum_rounded_once(gpu, c, bf16):
    """scn_segment_sum[_bf16]: n_items = 0 with rows -> exact +0; rows without items -> +0; one row receiving 10 000 items of
    mixed sign and magnitude (12 significant bits, resp. 8 for bf16, exponents -12..12: their float64 sum is exact, so the
    fp64 atomics' arrival order cannot show) next to rows with a handful of full-precision items.  Bit-equal to the
    restatement (float64 sum, ONE rounding to fp32, then to bf16); a second run is bit-identical."""
    L = _L()
    lib = L.lib()
    entry = lib.scn_segment_sum_bf16 if bf16 else lib.scn_segment_sum
    dt = torch.bfloat16 if bf16 else torch.float32
    # no items at all
    dX, acc = Buf(gpu, dt, 37 * c), Buf(gpu, torch.float64, 37 * c)
    L.check(entry(0, 0, 0, 37, c, dX.ptr, acc.ptr, L.stream()))
    assert int(_bits(dX.t).ne(0).sum()) == 0 and dX.intact() and acc.intact()
    # 10 000 items into row 5, 1200 into random EVEN rows of 300 (every other odd row stays without items)
    g = torch.Generator().manual_seed(100 + c)
    n_rows, n_big, n_small = 300, 10000, 1200
    mb = 8 if bf16 else 12
    mant = torch.randint(2 ** (mb - 1), 2 ** mb, (n_big, c), generator=g).double()
    expo = torch.randint(-12, 13, (n_big, c), generator=g).double()
    sign = torch.randint(0, 2, (n_big, c), generator=g).double() * 2 - 1
    big = (sign * mant * 2.0 ** (expo - (mb - 1))).float()
    small = torch.randn(n_small, c, generator=g)
    vals = torch.cat([big, small]).to(dt)
    assert torch.equal(vals[:n_big].double(), big.double())                          # representable: nothing was rounded away
    item_row = torch.cat([torch.full((n_big,), 5), torch.randint(0, n_rows // 2, (n_small,), generator=g) * 2])
    perm = torch.randperm(n_big + n_small, generator=g)
    vals, item_row = vals[perm].contiguous(), item_row[perm].to(torch.int32)
    n_items = len(item_row)
    V, IR = Buf(gpu, dt, n_items * c, 0, vals.to(gpu)), Buf(gpu, torch.int32, n_items, 0, item_row.to(gpu))
    want = R.segment_sum(_bf16_np(vals) if bf16 else vals.numpy(), item_row.numpy(), n_rows, bf16=bf16)
    runs = []
    for _ in range(2):
        dX, acc = Buf(gpu, dt, n_rows * c), Buf(gpu, torch.float64, n_rows * c)
        L.check(entry(V.ptr, IR.ptr, n_items, n_rows, c, dX.ptr, acc.ptr, L.stream()))
        assert dX.intact() and acc.intact() and V.intact() and IR.intact()
        runs.append((_bf16_np(dX.t) if bf16 else dX.t.cpu().numpy()).reshape(n_rows, c))
    assert np.array_equal(_np_bits(runs[0]), _np_bits(want))
    assert np.array_equal(_np_bits(runs[0]), _np_bits(runs[1]))
    empty = np.setdiff1d(np.arange(n_rows), item_row.numpy())
    assert len(empty) >= n_rows // 2 - 1 and not _np_bits(runs[0])[empty].any()      # rows without items: +0


# ------------------------------------------------------------------------------------------------------------------------
# storage casts
# ------------------------------------------------------------------------------------------------------------------------
CAST_COUNTS = list(range(1, 10)) + [1023, 1024, 1025, 4 * EW_THREADS + 4 * 100 + 3]


def _nan_aware_equal(got_bits, want_bits, nan_mask, is_nan_of_bits):
    """Bit-equal outside NaN; at a NaN of the expectation the result is some NaN."""
    ok = torch.equal(got_bits[~nan_mask], want_bits[~nan_mask])
    return ok and bool(is_nan_of_bits(got_bits[nan_mask]).all())


def _is_nan16(b):
    return (b.int() & 0x7FFF) > 0x7F80


def _is_nan32(b):
    return (b.long() & 0x7FFFFFFF) > 0x7F800000


def _f2b_values():
    """int32 bit patterns: every finite bf16 value widened, every exact midpoint between neighbouring bf16 values, the fp32
    values one ulp either side of each midpoint, the largest finite fp32, fp32 denormals, +-0, +-inf, NaNs."""
    h = np.arange(65536, dtype=np.uint32)
    h = h[(h & 0x7FFF) < 0x7F80] << 16                                                  # finite bf16, both signs
    extra = np.array([0x7F7FFFFF, 0xFF7FFFFF, 0x00000001, 0x80000001, 0x007FFFFF, 0x807FFFFF, 0x00000000, 0x80000000,
                      0x7F800000, 0xFF800000, 0x7FC00000, 0xFFC00000, 0x7F800001, 0x7FFFFFFF, 0xFF800001], dtype=np.uint32)
    return np.concatenate([h, h | 0x8000, h | 0x7FFF, h | 0x8001, extra]).view(np.int32)


def test_cast_bf16_to_f32_all_patterns_both_bodies(gpu):
    """scn_cast_bf16_to_f32: all 65 536 patterns (NaN compared as NaN), then shuffled patterns at counts 1-9, 1023-1025 and one
    above the grid cap, source off by 1, 2 (scalar body) and 4 elements (8-byte aligned: vector body), destination off by 1."""
    L = _L()
    lib = L.lib()
    pat = torch.arange(65536, dtype=torch.int32).to(torch.int16)
    g = torch.Generator().manual_seed(3)
    big_n = CAST_COUNTS[-1]
    src = torch.cat([pat, pat[torch.randint(0, 65536, (big_n - 65536,), generator=g)]])
    want = _bits(src.view(torch.bfloat16).float()).to(gpu)
    nan = _is_nan16(src).to(gpu)
    src = src.to(gpu)
    for count, (ox, oy) in itertools.product([65536] + CAST_COUNTS, [(0, 0), (1, 0), (2, 0), (4, 0), (0, 1)]):
        X, Y = Buf(gpu, torch.int16, count, ox, src[:count]), Buf(gpu, torch.float32, count, oy)
        L.check(lib.scn_cast_bf16_to_f32(X.ptr, count, Y.ptr, L.stream()))
        assert _nan_aware_equal(_bits(Y.t), want[:count], nan[:count], _is_nan32), (count, ox, oy)
        assert Y.intact() and X.intact(), ("guard", count, ox, oy)


def test_cast_f32_to_bf16_rounds_to_nearest_even_at_every_tie(gpu):
    """scn_cast_f32_to_bf16 bit-equal to torch's .to(torch.bfloat16) (NaN -> NaN) on `_f2b_values` -- ties to even at every
    exact midpoint, overflow to infinity above the largest bf16, denormals, signed zeros --, whole and at counts 1-9,
    1023-1025 and one above the grid cap; source one float off (scalar body), destination off by 1, 2 (scalar body) and 4
    elements (8-byte aligned: the vector body's 8-byte stores)."""
    L = _L()
    lib = L.lib()
    vals = torch.from_numpy(_f2b_values())
    g = torch.Generator().manual_seed(4)
    big_n = CAST_COUNTS[-1]
    src = torch.cat([vals, vals[torch.randint(0, len(vals), (big_n - len(vals),), generator=g)]])
    want16 = src.view(torch.float32).to(torch.bfloat16)
    assert np.array_equal(_bf16_np(want16)[~_is_nan32(src).numpy()],
                          R.f32_to_bf16_bits(src.view(torch.float32).numpy())[~_is_nan32(src).numpy()])   # torch == the restatement
    want = _bits(want16).to(gpu)
    nan = _is_nan32(src).to(gpu)
    assert bool(_is_nan16(want[nan]).all())
    src = src.to(gpu)
    for count, (ox, oy) in itertools.product([len(vals)] + CAST_COUNTS, [(0, 0), (1, 0), (0, 1), (0, 2), (0, 4), (1, 4)]):
        X, Y = Buf(gpu, torch.int32, count, ox, src[:count]), Buf(gpu, torch.int16, count, oy)
        L.check(lib.scn_cast_f32_to_bf16(X.ptr, count, Y.ptr, L.stream()))
        assert _nan_aware_equal(_bits(Y.t), want[:count], nan[:count], _is_nan16), (count, ox, oy)
        assert Y.intact() and X.intact(), ("guard", count, ox, oy)


# ------------------------------------------------------------------------------------------------------------------------
# MaxPooling / AveragePooling through the modules, fp32 and bf16 storage
# ------------------------------------------------------------------------------------------------------------------------
POOL_GRID, POOL_BATCH = (12, 12, 12), 2
POOL_STRIDES = [(2, 2, 2), (3, 3, 3), (2, 2, 1), (1, 2, 3), (4, 4, 4)]


def _pool_cloud(stride, seed):
    """About 600 points of a 12^3 grid, batch 2, chosen PER COARSE SITE: a few sites hold all n_off children, the others two
    or three -- so that cells whose maximum is shared (all children <= 0 after a ReLU, equal levels) are common at every
    stride (a uniform cloud gives a 4^3 cell eleven children and practically no all-zero cell)."""
    rng = np.random.default_rng(seed)
    st = np.asarray(stride)
    n_off = int(st.prod())
    cg = np.asarray(POOL_GRID) // st
    sites = np.stack(np.unravel_index(np.arange(int(cg.prod()) * POOL_BATCH), tuple(cg) + (POOL_BATCH,)), 1)
    rng.shuffle(sites)
    n_full = max(1, (200 if n_off <= 8 else 520) // n_off)
    rest = 600 - n_full * n_off
    n3 = rest // 10
    n2 = min((rest - 3 * n3) // 2, len(sites) - n_full - n3)
    ks = [n_off] * n_full + [3] * n3 + [2] * n2
    offs = np.stack(np.unravel_index(np.arange(n_off), tuple(st)), 1)
    pts = []
    for site, k in zip(sites, ks):
        for o in offs[rng.choice(n_off, size=min(k, n_off), replace=False)]:
            pts.append(np.concatenate([site[:3] * st + o, site[3:]]))
    pts = np.asarray(pts, dtype=np.int64)
    rng.shuffle(pts)
    return pts


def _pool_families(n, c, seed):
    g = torch.Generator().manual_seed(seed)
    levels = torch.tensor([-1.0, -0.5, 0.0, 0.5, 1.0])
    f3 = levels[torch.randint(0, 5, (n, c), generator=g)]
    f5 = f3.clone()
    zeros = (f3 == 0).nonzero()
    neg = zeros[torch.randperm(len(zeros), generator=g)[:len(zeros) // 2]]
    f5[neg[:, 0], neg[:, 1]] = -0.0
    return {"randn": torch.randn(n, c, generator=g), "relu": torch.relu(torch.randn(n, c, generator=g)), "levels": f3,
            "negative": -torch.randn(n, c, generator=g).abs() - 0.1, "levels_signed_zeros": f5}


def _tensor_on(gpu, coords, size, batch):
    """A SparseConvNetTensor factory over the Metadata of `coords` (unique; mode 0: slab row i is coords row i)."""
    scn = _scn()
    base = scn.InputLayer(3, torch.tensor(size), mode=0)((torch.from_numpy(coords), torch.zeros(len(coords), 1).to(gpu), batch))
    assert np.array_equal(base.get_spatial_locations().numpy(), coords)

    def make(features):
        return scn.SparseConvNetTensor(features=features, metadata=base.metadata, spatial_size=base.spatial_size)
    return make


def _run_pool(scn, make, slab, dY, average, stride):
    leaf = slab.clone().requires_grad_()
    y = (scn.AveragePooling if average else scn.MaxPooling)(3, stride, stride)(make(leaf)).features
    (dx,) = torch.autograd.grad(y, leaf, dY)
    return y.detach(), dx


@pytest.mark.parametrize("c", [1, 5, 8, 33])
@pytest.mark.parametrize("stride", POOL_STRIDES, ids=lambda s: "x".join(map(str, s)))
def test_pooling_both_kinds_both_storages_with_ties_and_signed_zeros(gpu, stride, c):
    """scn.MaxPooling / scn.AveragePooling (scn_pool_fwd / _bwd and their _bf16 forms) on five input families: randn,
    relu(randn) (all-zero cells), five levels (equal maxima), all negative (every output is the initial zero, no child gets a
    gradient), and the levels with half of the zeros made -0.0.
    max: forward and backward BIT-equal to the restatement in both storages (a maximum is not rounded, the gradient is a copy
    of dY or +0; every child that equals the cell's output AS A VALUE gets the full dY, -0 == +0 included).
    avg forward, fp32: <= (n_off + 1) u sum|children| / n_off  (n_off - 1 additions, the rounded reciprocal, the product);
    avg backward, fp32: exact for a power-of-two volume, else <= 2u |dY| / n_off  (rounded reciprocal, the product);
    bf16 storage: one bf16 rounding of that result on top (for the exact case: bit-equal to the rounded quotient).
    The signed-zero family in bf16 storage equals the fp32 kernels run on the widened slab, both kinds."""
    scn = _scn()
    coords = _pool_cloud(stride, 7)
    assert 560 <= len(coords) <= 640
    rb = O.strided_rulebook(coords, stride)
    child, parent = rb["child"], rb["parent"]
    n_off, nc = child.shape
    make = _tensor_on(gpu, coords, POOL_GRID, POOL_BATCH)
    fams = _pool_families(len(coords), c, 11 + c)
    pow2 = n_off & (n_off - 1) == 0
    worst = {}

    def note(key, err, bound):
        ok = bool((err <= bound).all())
        with np.errstate(divide="ignore", invalid="ignore"):
            r = np.where(bound > 0, err / bound, np.where(err > 0, np.inf, 0.0)).max()
        worst[key] = max(worst.get(key, 0.0), float(r))
        return ok

    for fam, x32 in fams.items():
        for bf16 in (False, True):
            slab = x32.to(gpu).to(torch.bfloat16) if bf16 else x32.to(gpu)
            Xw = slab.float().cpu().numpy()                                          # the stored values, widened exactly
            if fam in ("relu", "levels", "levels_signed_zeros"):
                assert R.pool_tie_cells(Xw, child).mean() >= 0.1, (fam, "too few cells with a tie for this test to mean anything")
            gen = torch.Generator().manual_seed(5)
            dY = torch.randn(nc, c, generator=gen).to(gpu)
            dY = dY.to(torch.bfloat16) if bf16 else dY
            dYw = dY.float().cpu().numpy()
            rnd = R.round_bf16 if bf16 else (lambda a: a)
            for average in (False, True):
                y, dx = _run_pool(scn, make, slab, dY, average, stride)
                assert y.dtype == slab.dtype and dx.dtype == slab.dtype
                yw, dxw = y.float().cpu().numpy(), dx.float().cpu().numpy()
                Y = R.pool_fwd(Xw, child, average)
                what = (fam, "bf16" if bf16 else "fp32", "avg" if average else "max")
                if not average:
                    assert np.array_equal(_np_bits(yw), _np_bits(Y.astype(np.float32))), what + ("forward",)
                    dX = R.pool_bwd(Xw, Y, dYw, parent, False, n_off)
                    assert np.array_equal(_np_bits(dxw), _np_bits(dX.astype(np.float32))), what + ("backward",)
                else:
                    b32 = (n_off + 1) * U32 * R.pool_fwd(np.abs(Xw), child, True)
                    bound = b32 + UB16 * (np.abs(Y) + b32) if bf16 else b32
                    assert note(what[1:] + ("forward",), np.abs(yw - Y), bound), what + ("forward",)
                    dX = R.pool_bwd(None, None, dYw, parent, True, n_off)
                    if pow2:
                        assert np.array_equal(_np_bits(dxw), _np_bits(rnd(dX).astype(np.float32))), what + ("backward",)
                    else:
                        b32 = 2 * U32 * np.abs(dX)
                        bound = b32 + UB16 * (np.abs(dX) + b32) if bf16 else b32
                        assert note(what[1:] + ("backward",), np.abs(dxw - dX), bound), what + ("backward",)
                if bf16 and fam == "levels_signed_zeros":
                    y32, dx32 = _run_pool(scn, make, slab.float(), dY.float(), average, stride)
                    assert _same_bits(y32.to(torch.bfloat16), y), what + ("forward vs fp32 on the widened slab",)
                    assert _same_bits(dx32.to(torch.bfloat16), dx), what + ("backward vs fp32 on the widened slab",)
                    if not average:
                        assert _same_bits(y.float(), y32) and _same_bits(dx.float(), dx32)
    for k, v in sorted(worst.items()):
        print(f"[margin] pooling {'x'.join(map(str, stride))} c={c} {' '.join(k)}: worst err/bound {v:.3g}")


# ------------------------------------------------------------------------------------------------------------------------
# SparseToDense through the module
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("size,c,per_sample", [((5, 7, 3), 1, 40), ((5, 7, 3), 6, 40), ((5, 7, 3), 33, 40),
                                               ((32, 32, 16), 64, 4500)])
def test_sparse_to_dense_put_and_get(gpu, size, c, per_sample, bf16):
    """scn.SparseToDense: batch 3 with the middle sample empty; forward bit-equal to an index put into +0 (inactive cells
    are +0), backward -- with a gradient that is non-zero at inactive cells too -- bit-equal to the index get.  The large
    case (9000 rows x 64 channels) sends the loop round twice."""
    scn = _scn()
    rng = np.random.default_rng(c)
    cells = size[0] * size[1] * size[2]
    cs = []
    for b in (0, 2):
        p = np.stack(np.unravel_index(rng.choice(cells, size=per_sample, replace=False), size), 1)
        cs.append(np.concatenate([p, np.full((per_sample, 1), b)], 1))
    coords = np.concatenate(cs).astype(np.int64)
    n = len(coords)
    assert (n * c > EW_THREADS) == (c == 64)
    make = _tensor_on(gpu, coords, size, 3)
    g = torch.Generator().manual_seed(1)
    dt = torch.bfloat16 if bf16 else torch.float32
    X = torch.randn(n, c, generator=g).to(dt)
    X[::5, 0] = -0.0
    leaf = X.to(gpu).requires_grad_()
    out = scn.SparseToDense(3, c)(make(leaf))
    assert out.dtype == dt and tuple(out.shape) == (3, c) + tuple(size)
    Xn = X.float().numpy()
    want = R.sparse_to_dense_fwd(Xn, coords, size, 3)
    assert np.array_equal(_np_bits(out.detach().float().cpu().numpy()), _np_bits(want))
    assert not _np_bits(out.detach().float().cpu().numpy())[1].any()                  # the empty sample: +0 everywhere
    dOut = (torch.randn(out.shape, generator=g) + 3.0).to(dt)
    assert bool((dOut.float() != 0).all())
    (dx,) = torch.autograd.grad(out, leaf, dOut.to(gpu))
    assert dx.dtype == dt
    assert np.array_equal(_np_bits(dx.float().cpu().numpy()), _np_bits(R.sparse_to_dense_bwd(dOut.float().numpy(), coords)))


# ------------------------------------------------------------------------------------------------------------------------
# OutputLayer on a bf16 slab with an odd width: scalar bf16 gather, bf16 segment sum through autograd
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", [7, 33])
def test_output_layer_on_a_bf16_slab_with_odd_width(gpu, c):
    scn = _scn()
    rng = np.random.default_rng(2)
    grid = (12, 10, 8)
    p = np.stack(np.unravel_index(rng.choice(grid[0] * grid[1] * grid[2], size=700, replace=False), grid), 1)
    p = np.concatenate([p, p[rng.integers(0, 700, size=900)]])                        # duplicates: rows with several items
    rng.shuffle(p)
    coords = np.concatenate([p, np.zeros((len(p), 1), dtype=p.dtype)], 1).astype(np.int64)
    scene = O.OracleScene(coords)
    x = scn.InputLayer(3, torch.tensor(grid), mode=4)((torch.from_numpy(coords), torch.zeros(len(coords), 1).to(gpu), 1))
    assert np.array_equal(x.metadata.item_row.cpu().numpy(), scene.prow)
    g = torch.Generator().manual_seed(c)
    slab = torch.randn(scene.n(0), c, generator=g).to(torch.bfloat16)
    leaf = slab.to(gpu).requires_grad_()
    y = scn.OutputLayer(3)(scn.SparseConvNetTensor(features=leaf, metadata=x.metadata, spatial_size=x.spatial_size))
    assert y.dtype == torch.bfloat16
    assert np.array_equal(_bf16_np(y), R.gather_rows(_bf16_np(slab), scene.prow))
    dY = torch.randn(len(coords), c, generator=g).to(torch.bfloat16)
    (dx,) = torch.autograd.grad(y, leaf, dY.to(gpu))
    assert dx.dtype == torch.bfloat16
    assert np.array_equal(_bf16_np(dx), R.segment_sum(_bf16_np(dY), scene.prow, scene.n(0), bf16=True))


# ------------------------------------------------------------------------------------------------------------------------
# column sum (bias gradient)
# ------------------------------------------------------------------------------------------------------------------------
def _colsum_chain(n, c, blocks):
    """Longest chain of fp32 additions behind each column of scn_colsum, from the launcher's constants: `nblk` blocks of 256
    threads share the rows (8 rows per block until `blocks` blocks are in use); inside a pass of `width` <= 256 columns a
    block runs 256 // width row lanes, each adding its share of the block's rows one by one; the lanes are added one by
    one; the final kernel adds ceil(nblk / 256) partials per thread, then 6 shuffle steps and 2 steps over the 4 waves."""
    nblk = max(1, -(-n // 8) if n < blocks * 8 else blocks)
    rows_per_block = -(-n // nblk)
    k = np.zeros(c, dtype=np.float64)
    for c0 in range(0, c, 256):
        width = min(256, c - c0)
        lanes = max(256 // width, 1)
        k[c0:c0 + width] = -(-rows_per_block // lanes) + lanes + -(-nblk // 256) + 6 + 2
    return k


@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("c", [1, 3, 64, 100, 255, 256, 257, 300, 513])
def test_colsum_beyond_256_columns_and_around_the_block_switch(gpu, c, bf16):
    """F.colsum (scn_colsum / scn_colsum_bf16) against float64: widths up to and past the 256-column pass, n = 0 (exact
    zeros), 1, around 8 rows (one block / two), around 8 * COLSUM_BLOCKS (where the block count stops growing) and 70 000.
    |db - exact| <= k u sum_r |dY[r][c]|, k = the longest chain of additions for that (n, c) (`_colsum_chain`); a second run is
    bit-identical (fixed order)."""
    from sparse_rcnn_amd import functional as F
    L = _L()
    worst = 0.0
    for n in (0, 1, 7, 8, 9, 4095, 4096, 4097, 70000):
        dY = torch.randn(n, c, generator=torch.Generator(device=gpu).manual_seed(n + c), device=gpu)
        dY = dY.to(torch.bfloat16) if bf16 else dY
        db = F.colsum(dY)
        db2 = F.colsum(dY)
        assert db.dtype == torch.float32 and db.shape == (c,)
        assert _same_bits(db, db2), (n, c)
        exact, sabs = dY.double().sum(0), dY.double().abs().sum(0)
        if n == 0:
            assert int(_bits(db).ne(0).sum()) == 0
            continue
        err = (db.double() - exact).abs().cpu().numpy()
        bound = _colsum_chain(n, c, L.COLSUM_BLOCKS) * U32 * sabs.cpu().numpy()
        assert (err <= bound).all(), (n, c, float((err / bound).max()))
        worst = max(worst, float((err / bound).max()))
    print(f"[margin] colsum c={c} {'bf16' if bf16 else 'fp32'}: worst err/bound {worst:.3g}")


# ------------------------------------------------------------------------------------------------------------------------
# SparseGlobalPool: mean / sum / amax per sample
# ------------------------------------------------------------------------------------------------------------------------
GP_SIZES = [0, 1, 1, 1, 252, 0, 1, 1, 256, 100, 0]         # rows per sample: boundaries at rows 1, 2, 3, 255, 256, 257, 513
GP_NEG, GP_TIED, GP_ZEROS = 4, 8, 9                        # samples: all negative / tied maxima / a -0, +0 pair above negatives


def _gp_scene(shuffled):
    rng = np.random.default_rng(17)
    cs = []
    for b, k in enumerate(GP_SIZES):
        p = np.stack(np.unravel_index(rng.choice(16 ** 3, size=k, replace=False), (16, 16, 16)), 1)
        cs.append(np.concatenate([p, np.full((k, 1), b)], 1))
    coords = np.concatenate(cs).astype(np.int64)
    assert np.cumsum(GP_SIZES)[[1, 2, 3, 4, 6, 7, 8]].tolist() == [1, 2, 3, 255, 256, 257, 513]
    if shuffled:
        rng.shuffle(coords)
    return coords


def _gp_features(coords, c, seed):
    X = torch.randn(len(coords), c, generator=torch.Generator().manual_seed(seed)).numpy()
    s = coords[:, 3]
    X[s == GP_NEG] = -np.abs(X[s == GP_NEG]) - 0.5
    tied = np.nonzero(s == GP_TIED)[0]
    X[tied[3], :] = 5.0                                                            # three rows share the maximum; two of them
    X[tied[7], :] = 5.0                                                            # (3, 7: the same row lane of their block when
    X[tied[130], :] = 5.0                                                          # sorted) meet inside one thread
    z = np.nonzero(s == GP_ZEROS)[0]
    X[z] = -np.abs(X[z]) - 0.5
    X[z[2], 0::2], X[z[6], 0::2] = -0.0, 0.0                                        # -0 before +0 (the same row lane when sorted)
    X[z[2], 1::2], X[z[6], 1::2] = 0.0, -0.0                                        # +0 before -0
    return X


@pytest.mark.parametrize("c", [1, 63, 64, 65, 130])
def test_global_pool_column_passes_sample_boundaries_and_maxima(gpu, c):
    """SparseGlobalPool(mean / sum / amax) (scn_segment_pool_*): 64-column passes (c below, at and past 64 and 128), sample
    boundaries at rows 1, 2, 3, 255, 256, 257 and 513 of the slab, an empty first, middle and last sample, rows grouped by
    sample and shuffled, a bf16-stored slab.  amax forward bit-equal to the true maximum: NEGATIVE for an all-negative
    sample, +0 for a -0 / +0 pair; mean and sum within u |y| + n 2^-53 sum|x| of float64 (float64 accumulation, one
    rounding to fp32); gradients bit-equal: mean dY / float(cnt), sum a copy, amax dY / ties (-0 and +0 tie)."""
    scn = _scn()
    ns = len(GP_SIZES)
    fns = {"mean": torch.mean, "sum": torch.sum, "amax": torch.amax}
    worst = 0.0
    for shuffled, bf16 in ((False, False), (True, False), (False, True)):
        coords = _gp_scene(shuffled)
        make = _tensor_on(gpu, coords, (16, 16, 16), ns)
        X = _gp_features(coords, c, 3 + c)
        Xt = torch.from_numpy(X).to(torch.bfloat16) if bf16 else torch.from_numpy(X)
        Xw = Xt.float().numpy()
        s = coords[:, 3]
        cnt = np.bincount(s, minlength=ns)
        for op, fn in fns.items():
            leaf = Xt.to(gpu).requires_grad_()
            y = scn.SparseGlobalPool(fn)(make(leaf))
            assert y.dtype == torch.float32 and tuple(y.shape) == (ns, c)
            yn = y.detach().cpu().numpy()
            Y = R.segment_pool_fwd(Xw, s, ns, op)
            what = (op, "shuffled" if shuffled else "sorted", "bf16" if bf16 else "fp32")
            assert not _np_bits(yn)[cnt == 0].any(), what                       # an empty sample pools to +0
            if op == "amax":
                assert np.array_equal(_np_bits(yn), _np_bits(Y.astype(np.float32))), what
                assert (yn[GP_NEG] < 0).all() and not _np_bits(yn[GP_ZEROS]).any()
            else:
                sabs = R.segment_pool_fwd(np.abs(Xw), s, ns, "sum")
                bound = U32 * np.abs(Y) + cnt[:, None] * 2.0 ** -53 * sabs
                err = np.abs(yn - Y)
                assert (err <= bound).all(), what
                worst = max(worst, float((err[cnt > 0] / bound[cnt > 0]).max()))
            dY = torch.randn(ns, c, generator=torch.Generator().manual_seed(8))
            (dx,) = torch.autograd.grad(y, leaf, dY.to(gpu))
            dX = R.segment_pool_bwd(Xw, yn, dY.numpy(), s, ns, op)
            if bf16:                                                            # the fp32 gradient, cast to the leaf's storage
                assert dx.dtype == torch.bfloat16
                assert np.array_equal(_bf16_np(dx), R.f32_to_bf16_bits(dX)), what
            else:
                assert np.array_equal(_np_bits(dx.cpu().numpy()), _np_bits(dX)), what
    print(f"[margin] global pool c={c} mean/sum: worst err/bound {worst:.3g}")
