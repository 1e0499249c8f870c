"""-m gpu: the bf16 tile convolution (csrc/scn_conv_ts_bf16.hip: k_conv_tb, the weight-streaming k_conv_tbs, k_conv_tb_sum, the
pack behind scn_conv_tiles_bf16) on every launcher path, through the C ABI, against the restatement in
tests/conv_bf16_restate.py (pinned on the CPU by tests/test_conv_bf16_restate_cpu.py, which also holds the case table to the
launcher's branches).  The discipline of tests/test_gpu_conv_paths.py, in halfwords:

Every case
  * asks scn_conv_tiles_bf16_plan_describe, with the real pointer bits, which path the call takes and holds it to the path the
    table names;
  * packs the weight image UNDER THE CASE'S SWITCHES with scn_conv_tiles_bf16_pack into a guarded buffer of exactly
    scn_conv_tiles_bf16_image_bytes (SCN_F_W_TRANSPOSED / SCN_F_OFF_REVERSE go to the pack);
  * runs inside guarded buffers: X, residual and relu_mask with 8 guard rows before and after, everything else with 4 KB, the
    scratch EXACTLY scn_conv_tiles_bf16_scratch_bytes long, the arrival array exactly max(1,
    scn_conv_tiles_bf16_arrival_counters) zeroed ints, the tile order exactly scn_tiles_order_ints(n, 1) ints.  The guards of
    the inputs hold the bf16 quiet NaN 0x7FC0 -- positive: it survives the packed-integer input ReLU, a negative NaN would be
    zeroed by it and hide a stray gather -- and so do the rows of X that no rule names (a fifth of them).  Y, the scratch and
    their guards start as 0xA5 bytes, the guards of the index arrays hold -1 ("no rule").  Afterwards every guard halfword is
    unchanged, every input, the image and the tile structures are unchanged, every arrival counter is zero, Y holds no 0xA5A5
    halfword and no NaN;
  * `exact` operands: bit-equal to the restatement's rounded float64 sums; `gaussian` operands: every element inside the
    interval the rigorous fp32 bound and the monotone rounding leave (conv_bf16_restate.check_interval), elements the mask
    zeroes exactly +0 or exactly the residual; the largest |error| / (bound + half an ulp) is printed per case (`[margin]`)
    with the share of elements whose interval admits two bf16 values (information only);
  * a second identical call into the same scratch and counters gives the same bits; the fused and the two-launch forms of a case
    give the same bits (same association); SCN_F_TILE_ORDER_X gives the bits of the plain call.

Misaligned pointers are 2, 4 or 8 bytes past a 16-byte boundary, one buffer at a time.  The scratch is misaligned only without
an arrival array (the fused form stores 16-byte pieces to it).  Nothing here is meant to fault: the refused-argument test only
checks return codes.  Out of scope: the >= 2^23-row limits, cout > 4096, scn_conv_tiles_chain (tests/test_gpu_chain.py), the
step executor (tests/test_gpu_exec.py).
"""
import numpy as np
import pytest
import torch

import conv_bf16_restate as B
import conv_restate as R

pytestmark = pytest.mark.gpu

NAN_HALF, Y_HALF, IDX_HALF = B.NAN_BF16, 0xA5A5, 0xFFFF
GUARD_ROWS, GUARD_BYTES = 8, 4096


@pytest.fixture(scope="module")
def L(gpu):
    from sparse_rcnn_amd import _lib
    _lib.lib()
    return _lib


class Buf:
    """`nbytes` of data `off` bytes past a 16-byte boundary, `guard` bytes (a multiple of 16) of the halfword `half` on both
    sides (test_gpu_conv_paths.Buf with 2-byte granularity)."""

    def __init__(self, dev, nbytes, guard, half, off=0, fill=None):
        assert guard % 16 == 0 and off % 2 == 0 and nbytes % 2 == 0
        self.half = int(np.array([half], dtype=np.uint16).view(np.int16)[0])
        self.lo, self.hi = (guard + off) // 2, (guard + off + int(nbytes)) // 2
        self.raw = torch.full((self.hi + guard // 2,), self.half, dtype=torch.int16, device=dev)
        assert self.raw.data_ptr() % 256 == 0
        self.ptr = self.raw.data_ptr() + 2 * self.lo
        self.fill = None
        if fill is not None:
            self.fill = torch.from_numpy(np.ascontiguousarray(fill).reshape(-1).view(np.int16)).to(dev)
            assert self.fill.numel() == self.hi - self.lo
            self.data().copy_(self.fill)

    def data(self):
        return self.raw[self.lo:self.hi]

    def u16(self):
        return self.data().cpu().numpy().view(np.uint16)

    def reset(self):
        self.data().fill_(self.half)

    def keep(self):
        """The current contents are what `unchanged` compares with from now on."""
        self.fill = self.data().clone()

    def intact(self):
        return bool((self.raw[:self.lo] == self.half).all()) and bool((self.raw[self.hi:] == self.half).all())

    def unchanged(self):
        return torch.equal(self.data(), self.fill)


_tables, _inputs, _images, _bits, _margins, _shares = {}, {}, {}, {}, {}, {}


def _table(gpu, L, n_off, rows):
    """The tile structures of the rule table (n_off, rows) from metadata.build_tiles(with_x=True) -- checked against the table in
    numpy -- in guarded buffers; the order buffer whole (LPT order, order by XCD bin, bin starts).  Once per module."""
    key = (n_off, rows)
    if key not in _tables:
        from sparse_rcnn_amd import metadata
        table, n_in, unnamed = B.table_of(n_off, rows)
        t = metadata.build_tiles(torch.from_numpy(table).to(gpu), n_off, rows, with_x=True)
        torch.cuda.synchronize()
        order = t.tile_order._base
        assert order is not None and order.numel() == L.lib().scn_tiles_order_ints(rows, 1)
        arrs = dict(perm=t.perm.cpu().numpy(), tstab=t.tstab.cpu().numpy(), tile_mask=t.tile_mask.cpu().numpy(),
                    tile_order=order.cpu().numpy())
        nt = -(-rows // 16)
        pop = B.check_tiles(table, arrs["perm"], arrs["tstab"], arrs["tile_mask"], arrs["tile_order"])
        assert set(R.group_counts(n_off)) <= set(pop.tolist())
        ox, bs = arrs["tile_order"][nt:2 * nt], arrs["tile_order"][2 * nt:2 * nt + 9]
        assert np.array_equal(np.sort(ox), np.arange(nt)) and bs[0] == 0 and bs[8] == nt and np.all(np.diff(bs) >= 0)
        assert len(unnamed) >= n_in // 5 - 2
        _tables[key] = dict(table=table, n_in=n_in, bufs={k: Buf(gpu, v.size * 4, GUARD_BYTES, IDX_HALF, 0, v) for k, v in arrs.items()})
    return _tables[key]


def _input(gpu, kind, c, name, arr, off):
    """A guarded device copy of an input operand (bf16 bits; bias fp32), shared by the cases that read the same numbers at the same
    alignment."""
    key = (kind, name, arr.shape, c.n_off if name == "x" else 0, off)
    if key not in _inputs:
        host = arr if name == "bias" else B.to_bf16_bits(arr)
        if name != "bias":
            assert np.array_equal(B.from_bf16_bits(host).view(np.uint32), arr.view(np.uint32))      # the operands ARE bf16
        guard = -(-(GUARD_ROWS * arr.shape[-1] * 2 if name != "bias" else GUARD_BYTES) // 16) * 16
        _inputs[key] = Buf(gpu, host.nbytes, guard, NAN_HALF, off, host)
    return _inputs[key]


def _image(gpu, L, kind, c, w):
    """The packed weight image of the case, packed under the switches in force (the caller holds them).  -> (W buffer, image)"""
    lib = L.lib()
    key = (kind, c.cin, c.cout, c.n_off, c.flags & (R.F_W_TRANSPOSED | R.F_OFF_REVERSE), c.variant)
    if key not in _images:
        wb = Buf(gpu, w.nbytes, GUARD_BYTES, NAN_HALF, 0, w)
        nbytes = lib.scn_conv_tiles_bf16_image_bytes(c.cin, c.cout, c.n_off)
        s = B.SHAPES[(c.cin, c.cout, c.variant)]
        assert nbytes == s["n_chunks"] * s["n_kc"] * c.n_off * 16 * s["nb"] * 32 * s["kh"] * 2
        img = Buf(gpu, nbytes, GUARD_BYTES, Y_HALF)
        L.check(lib.scn_conv_tiles_bf16_pack(wb.ptr, c.cin, c.cout, c.n_off, c.flags, img.ptr, L.stream()))
        torch.cuda.current_stream().synchronize()
        assert img.intact() and wb.intact() and wb.unchanged()
        assert not bool((img.data() == img.half).any()), "image halfword not written"
        img.keep()
        _images[key] = (wb, img)
    return _images[key]


def path_name(d, n_off):
    epi = "vec" if d["vec_ok"] else "elem"
    if d["stream"]:
        return f"k_conv_tbs<{d['ks']},{n_off},{d['nw']}> {epi}"
    return f"k_conv_tb<{d['nb']},{d['kh']},{'F' if d['fused'] else '-'},{'P' if d['part'] else '-'}> {epi}" + \
        (f" + sum<{d['sum_v']}>" if d["sum"] else "")


def run(gpu, L, c, kind):
    """One case of conv_bf16_restate.CASES under the discipline of the module docstring."""
    lib = L.lib()
    what = f"{c.id()} {kind}"
    with R.switches(L, c.sw):
        rows = B.table_rows(L, c)
        T = _table(gpu, L, c.n_off, rows)
        n_in, tb = T["n_in"], T["bufs"]
        ops = B.operands(kind, c, rows)
        ref = B.reference(kind, c, rows)
        ins = {k: _input(gpu, kind, c, k, v, c.off.get(k, 0)) for k, v in ops.items() if k != "w"}
        wb, img = _image(gpu, L, kind, c, ops["w"])
        nbytes = lib.scn_conv_tiles_bf16_scratch_bytes(c.cin, rows, c.cout)
        n_arr = lib.scn_conv_tiles_bf16_arrival_counters(c.cin, rows, c.cout)
        assert nbytes >= 256 and n_arr >= 0
        Y = Buf(gpu, rows * c.cout * 2, GUARD_BYTES, Y_HALF, c.off.get("y", 0))
        scratch = Buf(gpu, nbytes, GUARD_BYTES, Y_HALF, c.off.get("scratch", 0))
        arrival = Buf(gpu, 4 * max(1, n_arr), GUARD_BYTES, Y_HALF, 0, np.zeros(max(1, n_arr), np.int32)) if c.arrival else None
        bufs = list(ins.values()) + list(tb.values()) + [wb, img, Y, scratch] + ([arrival] if arrival else [])
        opt = lambda k: ins[k].ptr if k in ins else None

        assert ins["x"].ptr % 16 == 0 and img.ptr % 16 == 0
        y_bits = (Y.ptr | (opt("residual") or 0) | (opt("relu_mask") or 0)) & 15
        s_bits = (scratch.ptr | (opt("bias") or 0)) & 15
        assert (y_bits, s_bits) == c.ptr_bits(), what
        rc, d = B.describe(L, n_in, c.cin, c.n_off, rows, c.cout, c.flags, c.arrival, y_bits, s_bits)
        assert rc == 0 and {k: d[k] for k in c.expect} == c.expect, (what, d)

        def call(flags=c.flags):
            return lib.scn_conv_tiles_bf16(ins["x"].ptr, n_in, c.cin, tb["tstab"].ptr, tb["tile_mask"].ptr, tb["perm"].ptr,
                                           tb["tile_order"].ptr, c.n_off, rows, img.ptr, opt("bias"), opt("residual"),
                                           opt("relu_mask"), Y.ptr, c.cout, flags, scratch.ptr, arrival.ptr if arrival else None,
                                           L.stream())

        def after(tag):
            torch.cuda.current_stream().synchronize()
            for b in bufs:
                assert b.intact(), ("guard", tag, what, bufs.index(b))
            for k, b in list(ins.items()) + list(tb.items()) + [("w", wb), ("image", img)]:
                assert b.unchanged(), ("input written", tag, what, k)
            assert arrival is None or not bool(arrival.data().any()), ("arrival counters not zero", tag, what)
            y = Y.data()
            assert not bool((y == Y.half).any()), ("element not written", tag, what)
            assert not bool(torch.isnan(y.view(torch.bfloat16)).any()), ("NaN: a gather strayed", tag, what)
            return Y.u16().reshape(rows, c.cout)

        L.check(call())
        got = after("first call")
        Y.reset()
        L.check(call())
        assert np.array_equal(got, after("second call")), ("not reproducible", what)
        if c.xorder:                                                 # placement only decides the speed
            Y.reset()
            L.check(call(c.flags & ~B.F_TILE_ORDER_X))
            assert np.array_equal(got, after("plain order")), ("the hand-out by XCD changes the bits", what)

    # the forms of the K reduction (fused, arrival == NULL, SPLIT_SUM) of the same kernel and numbers: the same bits
    key = (kind, c.cin, c.cout, c.n_off, rows, c.flagset, c.variant, d["stream"])
    if key in _bits:
        assert np.array_equal(got, _bits[key][1]), ("K-reduction forms differ", what, _bits[key][0])
    else:
        _bits[key] = (what, got)

    if kind == "exact":
        want = ref[0]
        assert np.array_equal(got, want), (what, int((got != want).sum()),
                                           float(np.abs(B.from_bf16_bits(got).astype(np.float64) - ref[1]).max()))
    else:
        bad, margin, share = B.check_interval(got, *ref)
        name = path_name(d, c.n_off)
        _margins[name] = max(_margins.get(name, 0.0), margin)
        _shares[name] = max(_shares.get(name, 0.0), share)
        print(f"[margin] {name}: {what} {margin:.3f} of bound + half ulp; two-valued intervals {100 * share:.2f} %")
        assert bad == 0, (what, bad, margin)
    return d


GROUP_SHAPES = sorted({(c.group, c.cin, c.cout) for c in B.CASES})


@pytest.mark.parametrize("group,cin,cout", GROUP_SHAPES, ids=[f"{g.replace(' ', '_')}-{a}x{b}" for g, a, b in GROUP_SHAPES])
def test_every_case_of_the_table(gpu, L, group, cin, cout):
    """The rows of conv_bf16_restate.CASES of one group and shape: every kernel, K-reduction form, flag / epilogue set, switch,
    table and pointer offset the table names for it -- exact operands everywhere, gaussian once per distinct expected path."""
    cases = [c for c in B.CASES if (c.group, c.cin, c.cout) == (group, cin, cout)]
    assert cases
    for c in cases:
        run(gpu, L, c, "exact")
        if c.gaussian:
            run(gpu, L, c, "gaussian")


def test_bad_arguments_are_refused_without_a_launch_and_no_rows_touch_nothing(gpu, L):
    """X or the image off their 16-byte boundary, cin no multiple of 8, offset counts outside 1..27, missing buffers: SCN_EINVAL
    and an untouched Y (return codes only: nothing is launched)."""
    lib = L.lib()
    c = next(c for c in B.CASES if (c.cin, c.cout, c.n_off, c.table, c.flagset) == (64, 32, 27, "small", "fwd") and c.arrival
             and not c.off and not c.sw)
    rows = R.small_rows(27)
    T = _table(gpu, L, 27, rows)
    tb = T["bufs"]
    ops = B.operands("exact", c, rows)
    x, bias = _input(gpu, "exact", c, "x", ops["x"], 0), _input(gpu, "exact", c, "bias", ops["bias"], 0)
    _, img = _image(gpu, L, "exact", c, ops["w"])
    Y = Buf(gpu, rows * 32 * 2, GUARD_BYTES, Y_HALF)
    scratch = Buf(gpu, lib.scn_conv_tiles_bf16_scratch_bytes(64, rows, 32), GUARD_BYTES, Y_HALF)
    n_arr = lib.scn_conv_tiles_bf16_arrival_counters(64, rows, 32)
    arrival = Buf(gpu, 4 * n_arr, GUARD_BYTES, Y_HALF, 0, np.zeros(n_arr, np.int32))

    def call(xp=x.ptr, ip=img.ptr, cin=64, n_off=27, n_out=rows, sc=scratch.ptr, yp=Y.ptr):
        return lib.scn_conv_tiles_bf16(xp, T["n_in"], cin, tb["tstab"].ptr, tb["tile_mask"].ptr, tb["perm"].ptr,
                                       tb["tile_order"].ptr, n_off, n_out, ip, bias.ptr, None, None, yp, 32, 0, sc, arrival.ptr,
                                       L.stream())

    for off in (2, 4, 8):
        assert call(xp=x.ptr + off) == L.EINVAL and call(ip=img.ptr + off) == L.EINVAL
    assert call(n_off=28) == L.EINVAL and call(n_off=0) == L.EINVAL
    assert call(cin=0) == L.EINVAL and call(cin=4) == L.EINVAL and call(cin=60) == L.EINVAL
    assert call(xp=None) == L.EINVAL and call(ip=None) == L.EINVAL and call(sc=None) == L.EINVAL and call(yp=None) == L.EINVAL
    assert call(n_out=-1) == L.EINVAL and call(n_out=1 << 23) == L.EINVAL
    assert call(n_out=0) == L.OK and call(xp=None, n_out=0) == L.OK
    torch.cuda.synchronize()
    for b in (Y, scratch, arrival):
        assert b.intact()
    assert bool((Y.data() == Y.half).all()) and bool((scratch.data() == scratch.half).all()) and not bool(arrival.data().any())


def test_zz_largest_margin_per_path(gpu):
    """(Runs last in the file: the summary of the [margin] prints above, per launcher path.)"""
    for name in sorted(_margins):
        print(f"[margin] path {name}: largest |error| / (bound + half ulp) {_margins[name]:.3f}; "
              f"two-valued intervals at most {100 * _shares[name]:.2f} %")
    assert all(np.isfinite(v) for v in _margins.values())            # (the assertion is the interval, case by case)
