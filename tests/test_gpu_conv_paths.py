"""-m gpu: the fp32 tile convolution (csrc/scn_conv_ts.hip with its two tile loops, k_conv_ts_sum, the opt-in stream kernel of
scn_conv_tss.hip) on every launcher path, through the C ABI, against the float64 restatement in tests/conv_restate.py (pinned
on the CPU by tests/test_conv_restate_cpu.py, which also holds the case table to the launcher's branches).

Every case
  * asks scn_conv_tiles_plan_describe, with the real pointer bits, which path the call takes and holds it to the path the table
    names; after the call scn_conv_tiles_path_counts and scn_conv_tiles_split_count say the same on their own;
  * runs inside guarded buffers: X, residual and relu_mask with 8 guard rows before and after, everything else with 4 KB, the
    scratch EXACTLY scn_conv_tiles_scratch_bytes long, the arrival array exactly max(1, scn_conv_tiles_arrival_counters) zeroed
    ints.  The guards of the float inputs hold the word 0x7FC00000: a gather that strays into one puts a NaN into the output for
    certain (a small sentinel would vanish next to an integer sum); so do the rows of X that no rule names (a fifth of them).  Y and its guards start as 0xA5 bytes.  The guards of the
    index arrays hold -1 ("no rule"): a stray index read there must not turn into a wild gather that faults the device; what
    their guards show is a write.  Afterwards every guard word is unchanged, every input and tile structure is unchanged, every arrival counter is
    zero, Y holds no sentinel word and no NaN;
  * `exact` operands (small integers: every summation order gives the float64 bits): bit-equal to the restatement; `gaussian`
    operands: every element within gamma_{N+2} S of it (N terms, S the sum of their absolute values -- the bound of a sum of N
    rounded products in ANY order; nothing in it is measured), the largest ratio to the bound printed per case (`[margin]`);
  * a second identical call into the same scratch and arrival buffers gives the same bits.

Misaligned pointers are one float off a 16-byte boundary.  The scratch is misaligned only without an arrival array (the fused
form stores 16-byte pieces to it).  scn_conv_tiles_bf16 has the same kind of file: tests/test_gpu_conv_bf16_paths.py.  Out of
scope: scn_conv_tiles_chain (tests/test_gpu_chain.py), the >= 2^23-row limits of the fast path.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import conv_restate as R

pytestmark = pytest.mark.gpu

NAN_WORD = 0x7FC00000
Y_WORD = int(np.array([0xA5A5A5A5], dtype=np.uint32).view(np.int32)[0])
IDX_WORD = -1
GUARD_ROWS, GUARD_BYTES = 8, 4096


@pytest.fixture(scope="module")
def L(gpu):
    from sparse_rcnn_amd import _lib
    _lib.lib()
    return _lib


class Buf:
    """`nbytes` of data `off` bytes past a 16-byte boundary, `guard` bytes (a multiple of 16) of the word `word` on both sides."""

    def __init__(self, dev, nbytes, guard, word, off=0, fill=None):
        assert guard % 16 == 0 and off % 4 == 0 and nbytes % 4 == 0
        self.word = word
        self.lo, self.hi = (guard + off) // 4, (guard + off + int(nbytes)) // 4
        self.raw = torch.full((self.hi + guard // 4,), word, dtype=torch.int32, device=dev)
        assert self.raw.data_ptr() % 256 == 0
        self.ptr = self.raw.data_ptr() + 4 * self.lo
        self.fill = None
        if fill is not None:
            self.fill = torch.from_numpy(np.ascontiguousarray(fill).reshape(-1).view(np.int32)).to(dev)
            assert self.fill.numel() == self.hi - self.lo
            self.data().copy_(self.fill)

    def data(self):
        return self.raw[self.lo:self.hi]

    def f32(self):
        return self.data().view(torch.float32).cpu().numpy()

    def reset(self, word=None):
        self.data().fill_(self.word if word is None else word)

    def intact(self):
        return bool((self.raw[:self.lo] == self.word).all()) and bool((self.raw[self.hi:] == self.word).all())

    def unchanged(self):
        return torch.equal(self.data(), self.fill)


_tables, _inputs, _refs, _margins, _draws = {}, {}, {}, {}, {}


def _table(gpu, n_off, rows):
    """The rule table of (n_off, rows), its tile structures from metadata.build_tiles -- checked against the table in numpy -- in
    guarded buffers.  Once per module."""
    key = (n_off, rows)
    if key not in _tables:
        from sparse_rcnn_amd import metadata
        table, n_in = R.rule_table(n_off, rows)
        t = metadata.build_tiles(torch.from_numpy(table).to(gpu), n_off, rows)
        torch.cuda.synchronize()
        arrs = dict(perm=t.perm.cpu().numpy(), tstab=t.tstab.cpu().numpy(), tile_mask=t.tile_mask.cpu().numpy(),
                    tile_order=t.tile_order.cpu().numpy())
        pop = R.check_tiles(table, arrs["perm"], arrs["tstab"], arrs["tile_mask"], arrs["tile_order"])
        assert set(R.group_counts(n_off)) <= set(pop.tolist())
        bufs = {k: Buf(gpu, v.size * 4, GUARD_BYTES, IDX_WORD, 0, v) for k, v in arrs.items()}
        unnamed = R.unnamed_rows(table, n_in)
        assert len(unnamed) >= n_in // 5 - 2                         # every row = 3 (mod 5) but, at most, the two forced ends
        _tables[key] = dict(table=table, n_in=n_in, bufs=bufs, unnamed=unnamed)
    return _tables[key]


def _drawn(kind, rows, cols, seed):
    key = (kind, rows, cols, seed)
    if key not in _draws:
        _draws[key] = R.mask_operand(rows, cols, seed) if kind == "mask" else R.operand(kind, rows, cols, seed)
    return _draws[key]


def _x(kind, c, T):
    """X of a case: the rows no rule names are NaN (the restatement never reads them either)."""
    key = (kind, "x", c.n_off, T["table"].shape[1], c.cin)
    if key not in _draws:
        x = R.operand(kind, T["n_in"], c.cin, 101)
        x[T["unnamed"]] = np.nan
        _draws[key] = x
    return _draws[key]


def _operands(kind, c, T, rows):
    """Host operands of a case: X [n_in, cin], W [n_off, cin, cout] (stored [n_off, cout, cin] under W_TRANSPOSED: the same
    numbers, another reading), bias, residual, relu_mask."""
    wr = c.cout if c.flags & R.F_W_TRANSPOSED else c.cin
    wc = c.cin if c.flags & R.F_W_TRANSPOSED else c.cout
    ops = dict(x=_x(kind, c, T), w=_drawn(kind, c.n_off * wr, wc, 102).reshape(c.n_off, wr, wc))
    if "bias" in c.operands:
        ops["bias"] = _drawn(kind, 1, c.cout, 103)[0]
    if "residual" in c.operands:
        ops["residual"] = _drawn(kind, rows, c.cout, 104)
    if "relu_mask" in c.operands:
        ops["relu_mask"] = _drawn("mask" if kind == "exact" else kind, rows, c.cout, 105)
    return ops


def _reference(kind, c, T, rows):
    """exact: Y as float32 (cached: shared by every path that runs the operands); gaussian: (Y, bound) in float64."""
    key = (kind, c.cin, c.cout, c.n_off, rows, c.flagset)
    if key in _refs:
        return _refs[key]
    ops = _operands(kind, c, T, rows)
    Y, S, N = R.conv(ops["x"], ops["w"], T["table"], ops.get("bias"), ops.get("residual"), ops.get("relu_mask"),
                     c.flags & ~R.F_SPLIT_SUM)
    if kind == "exact":
        R.assert_exact(S)
        ref = Y.astype(np.float32)
        assert np.array_equal(ref.astype(np.float64), Y)
        _refs[key] = ref
        return ref
    return Y, R.bound(N[:, None], S)


def _input(gpu, kind, c, name, arr, off):
    """A guarded device copy of an input operand, shared by the cases that read the same numbers at the same alignment."""
    key = (kind, name, arr.shape, c.flags & R.F_W_TRANSPOSED if name == "w" else 0, c.n_off if name == "x" else 0, off)
    if key not in _inputs:
        guard = GUARD_ROWS * arr.shape[-1] * 4 if name in ("x", "residual", "relu_mask") else GUARD_BYTES
        guard = -(-guard // 16) * 16
        _inputs[key] = Buf(gpu, arr.size * 4, guard, NAN_WORD, off, arr)
    return _inputs[key]


def run(gpu, L, c, kind):
    """One case of conv_restate.CASES under the discipline of the module docstring."""
    lib = L.lib()
    what = f"{c.id()} {kind}"
    with R.switches(L, c.sw):
        rows = R.table_rows(L, c)
        T = _table(gpu, c.n_off, rows)
        n_in, tb = T["n_in"], T["bufs"]
        ops = _operands(kind, c, T, rows)
        ref = _reference(kind, c, T, rows)
        ins = {k: _input(gpu, kind, c, k, v, 4 if k in c.off else 0) for k, v in ops.items()}
        nbytes = lib.scn_conv_tiles_scratch_bytes(c.cin, rows, c.cout)
        n_arr = lib.scn_conv_tiles_arrival_counters(c.cin, rows, c.cout)
        assert nbytes >= 256 and n_arr >= 0
        Y = Buf(gpu, rows * c.cout * 4, GUARD_BYTES, Y_WORD, 4 if "y" in c.off else 0)
        scratch = Buf(gpu, nbytes, GUARD_BYTES, Y_WORD, 4 if "scratch" in c.off else 0)
        arrival = Buf(gpu, 4 * max(1, n_arr), GUARD_BYTES, Y_WORD, 0, np.zeros(max(1, n_arr), np.int32)) if c.arrival else None
        bufs = list(ins.values()) + list(tb.values()) + [Y, scratch] + ([arrival] if arrival else [])
        opt = lambda k: ins[k].ptr if k in ins else None

        x_bits, w_bits = ins["x"].ptr & 15, ins["w"].ptr & 15
        epi_bits = (Y.ptr | scratch.ptr | (opt("bias") or 0) | (opt("residual") or 0) | (opt("relu_mask") or 0)) & 15
        assert (x_bits, w_bits, epi_bits) == c.ptr_bits(), what
        rc, d = R.describe(L, n_in, c.cin, c.n_off, rows, c.cout, c.flags, c.arrival, x_bits, w_bits, epi_bits)
        assert rc == 0 and {k: d[k] for k in c.expect} == c.expect, (what, d)

        def call():
            st = L.stream()
            rc = lib.scn_conv_tiles(ins["x"].ptr, n_in, c.cin, tb["tstab"].ptr, tb["tile_mask"].ptr, tb["perm"].ptr,
                                    tb["tile_order"].ptr, c.n_off, rows, ins["w"].ptr, opt("bias"), opt("residual"),
                                    opt("relu_mask"), Y.ptr, c.cout, c.flags, scratch.ptr, arrival.ptr if arrival else None, st)
            if rc == 0 and c.split_sum:
                rc = lib.scn_conv_tiles_finish(c.cin, rows, opt("bias"), opt("residual"), opt("relu_mask"), Y.ptr, c.cout,
                                               c.flags, scratch.ptr, st)
            return rc

        def after(tag):
            torch.cuda.current_stream().synchronize()
            for b in bufs:
                assert b.intact(), ("guard", tag, what, bufs.index(b))
            for k, b in list(ins.items()) + list(tb.items()):
                assert b.unchanged(), ("input written", tag, what, k)
            assert arrival is None or not bool(arrival.data().any()), ("arrival counters not zero", tag, what)
            y = Y.data()
            assert not bool((y == Y_WORD).any()), ("element not written", tag, what)
            assert not bool(torch.isnan(y.view(torch.float32)).any()), ("NaN: a gather strayed", tag, what)

        paths = (C.c_int64 * 4)()
        lib.scn_conv_tiles_path_counts(paths, 1)
        lib.scn_conv_tiles_split_count(1)
        L.check(call())
        lib.scn_conv_tiles_path_counts(paths, 1)
        ksplit = d["n_kc"] > 1
        if d["stream"]:
            assert list(paths) == [1, 0, 1, 0] and lib.scn_conv_tiles_split_count(1) == 0, (what, list(paths))
        else:
            assert list(paths) == [d["fullk"], 1 - d["fullk"], int(ksplit and d["fused"]), int(ksplit and not d["fused"])], \
                (what, list(paths))
            assert lib.scn_conv_tiles_split_count(1) == d["split4"], what
        after("first call")
        got = Y.f32().reshape(rows, c.cout)
        Y.reset()
        L.check(call())
        after("second call")
        assert np.array_equal(got.view(np.uint32), Y.f32().view(np.uint32).reshape(got.shape)), ("not reproducible", what)

    if kind == "exact":
        assert np.array_equal(got.view(np.uint32), ref.view(np.uint32)), \
            (what, float(np.abs(got.astype(np.float64) - ref).max()), int((got.view(np.uint32) != ref.view(np.uint32)).sum()))
    else:
        want, lim = ref
        err = np.abs(got.astype(np.float64) - want)
        ratio = float(np.max(np.where(lim > 0, err / np.where(lim > 0, lim, 1.0), np.where(err > 0, np.inf, 0.0))))
        _margins[c.group] = max(_margins.get(c.group, 0.0), ratio)
        print(f"[margin] {c.group}: {what} {ratio:.3f} of the bound")
        assert ratio <= 1.0, (what, ratio)
    return d


GROUP_SHAPES = sorted({(c.group, c.cin, c.cout) for c in R.CASES})


@pytest.mark.parametrize("group,cin,cout", GROUP_SHAPES, ids=[f"{g.replace(' ', '_')}-{a}x{b}" for g, a, b in GROUP_SHAPES])
def test_every_case_of_the_table(gpu, L, group, cin, cout):
    """The rows of conv_restate.CASES of one group and shape: every loop, K-reduction form, flag / epilogue set, switch and
    pointer offset the table names for it -- exact operands everywhere, gaussian once per distinct expected path."""
    cases = [c for c in R.CASES if (c.group, c.cin, c.cout) == (group, cin, cout)]
    assert cases
    for c in cases:
        run(gpu, L, c, "exact")
        if c.gaussian:
            run(gpu, L, c, "gaussian")


def test_bad_arguments_are_refused_without_a_launch_and_no_rows_touch_nothing(gpu, L):
    lib = L.lib()
    c = next(c for c in R.CASES if (c.cin, c.cout, c.n_off, c.table, c.flagset) == (64, 64, 27, "small", "fwd") and c.arrival)
    rows = R.small_rows(27)
    T = _table(gpu, 27, rows)
    tb = T["bufs"]
    ops = _operands("exact", c, T, rows)
    ins = {k: _input(gpu, "exact", c, k, v, 0) for k, v in ops.items()}
    Y = Buf(gpu, rows * 64 * 4, GUARD_BYTES, Y_WORD)
    scratch = Buf(gpu, lib.scn_conv_tiles_scratch_bytes(64, rows, 64), GUARD_BYTES, Y_WORD)
    n_arr = lib.scn_conv_tiles_arrival_counters(64, rows, 64)
    arrival = Buf(gpu, 4 * n_arr, GUARD_BYTES, Y_WORD, 0, np.zeros(n_arr, np.int32))

    def call(x=ins["x"].ptr, cin=64, n_off=27, n_out=rows, sc=scratch.ptr):
        return lib.scn_conv_tiles(x, T["n_in"], cin, tb["tstab"].ptr, tb["tile_mask"].ptr, tb["perm"].ptr, tb["tile_order"].ptr,
                                  n_off, n_out, ins["w"].ptr, ins["bias"].ptr, None, None, Y.ptr, 64, 0, sc, arrival.ptr,
                                  L.stream())

    paths = (C.c_int64 * 4)()
    lib.scn_conv_tiles_path_counts(paths, 1)
    lib.scn_conv_tiles_split_count(1)
    assert call(n_off=28) == L.EINVAL and call(n_off=0) == L.EINVAL
    assert call(cin=0) == L.EINVAL
    assert call(x=None) == L.EINVAL
    assert call(sc=None) == L.EINVAL
    assert call(n_out=-1) == L.EINVAL
    assert call(n_out=0) == L.OK and call(x=None, n_out=0) == L.OK
    assert lib.scn_conv_tiles_finish(0, rows, None, None, None, Y.ptr, 64, 0, scratch.ptr, L.stream()) == L.EINVAL
    assert lib.scn_conv_tiles_finish(64, rows, None, None, None, None, 64, 0, scratch.ptr, L.stream()) == L.EINVAL
    assert lib.scn_conv_tiles_finish(64, 0, None, None, None, None, 64, 0, None, L.stream()) == L.OK
    torch.cuda.synchronize()
    lib.scn_conv_tiles_path_counts(paths, 1)
    assert list(paths) == [0, 0, 0, 0] and lib.scn_conv_tiles_split_count(1) == 0
    for b in (Y, scratch, arrival):
        assert b.intact()
    assert bool((Y.data() == Y_WORD).all()) and bool((scratch.data() == Y_WORD).all()) and not bool(arrival.data().any())


def test_zz_largest_ratio_to_the_bound_per_group(gpu):
    """(Runs last in the file: the summary line of the [margin] prints above.)"""
    for g in sorted(_margins):
        print(f"[margin] group {g}: largest |error| / bound {_margins[g]:.3f}")
    assert all(v <= 1.0 for v in _margins.values())
