"""-m gpu: the weight gradient (csrc/scn_wgrad.hip, scn_wgrad_unit.inc, scn_wgrad_tiles.hip) on every launcher path, through
the C ABI, against the float64 restatement in tests/wgrad_restate.py (pinned on the CPU by tests/test_wgrad_restate_cpu.py).

Every case
  * asks scn_wgrad_plan_describe which path the call takes and holds it to the path the table names (coverage cannot move
    silently when pick_shape / make_dplan change);
  * runs inside sentinel-filled buffers: X, dY with 8 guard rows before and after, dW, db and the scratch with 4 KB on both
    sides, the scratch EXACTLY scn_wgrad_scratch_bytes* long; afterwards every guard byte is unchanged, X and dY are
    unchanged, dW and db hold no sentinel word;
  * `exact` operands (small integers: every summation order and bf16 storage give the float64 bits): bit-equal to the
    restatement; `gaussian` operands: every element within gamma_{N+2} S of it (N rules of the offset, S the sum of the
    absolute terms -- the bound of a sum of N rounded products in ANY order; nothing in it is measured), the largest
    ratio to the bound printed per case (`[margin]` lines);
  * a second identical call gives the same bits.

A rule that reads a guard row (sentinel 0xA5A5A5A5 = -2.9e-16, bf16 0xA5A5 = -1.8e-16) breaks the exact comparison.
Misaligned pointers are one element off a 16-byte boundary: still naturally aligned for their element type.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import wgrad_restate as R

pytestmark = pytest.mark.gpu

SENT = 0xA5
SENT_WORD = int(np.array([0xA5A5A5A5], dtype=np.uint32).view(np.int32)[0])
GUARD_ROWS, GUARD_BYTES = 8, 4096
F_RELU_IN = 1


@pytest.fixture(scope="module")
def L(gpu):
    from sparse_rcnn_amd import _lib
    _lib.lib()
    return _lib


class Buf:
    """`nbytes` of data `off` bytes past a 16-byte boundary, `guard` sentinel bytes (a multiple of 16) on both sides."""

    def __init__(self, dev, nbytes, guard, off=0, fill=None):
        assert guard % 16 == 0
        self.lo, self.hi = guard + off, guard + off + int(nbytes)
        self.raw = torch.full((self.hi + guard,), SENT, dtype=torch.uint8, device=dev)
        assert self.raw.data_ptr() % 256 == 0
        self.ptr = self.raw.data_ptr() + self.lo
        self.fill = None
        if fill is not None:
            self.fill = torch.from_numpy(np.ascontiguousarray(fill).view(np.uint8).reshape(-1)).to(dev)
            assert self.fill.numel() == nbytes
            self.data().copy_(self.fill)

    def data(self):
        return self.raw[self.lo:self.hi]

    def f32(self):
        return self.data().view(torch.float32).cpu().numpy()

    def reset(self):
        self.data().fill_(SENT)

    def intact(self):
        return bool((self.raw[:self.lo] == SENT).all()) and bool((self.raw[self.hi:] == SENT).all())

    def unchanged(self):
        return torch.equal(self.data(), self.fill)

    def has_sentinel(self):
        return bool((self.data().view(torch.int32) == SENT_WORD).any())


_refs, _margins = {}, {}


def _aligned(cin, cout, bf16):
    """Path of a shape with 16-byte-aligned pointers and no switch: the shape table's, or (bf16 shapes it does not list) the
    k_wgrad_tb form: 1 / 2 / 4 tiles per wave for up to 32 / 64 / more channels, workgroup blocks of 32 tiles."""
    for s in R.SHAPES:
        if s[:4] == (cin, cout, bf16, {}):
            return s[4]
    assert bf16 and cin % 8 == 0 and cout % 8 == 0
    tiles = lambda c: 1 if c <= 32 else (2 if c <= 64 else 4)
    return R.mk_path("t", tiles(cin), tiles(cout), nbi=-(-cin // (32 * tiles(cin))), nbj=-(-cout // (32 * tiles(cout))))


def _problem(kind, cin, cout, bf16, lst, relu, n_prob):
    """Operands, rule list and restatement of a case -- computed once per module, shared by every path that runs them."""
    key = (kind, cin, cout, bool(bf16) and kind != "exact", lst, relu, n_prob)
    if key not in _refs:
        if isinstance(lst, int):                                     # the identity list of `lst` rows
            in_rows = out_rows = None
            prefix, mask, rows_in, rows_out = np.array([0, lst], dtype=np.int64), 1, lst, lst
        else:
            in_rows, out_rows, prefix, mask = R.make_list(lst)
            rows_in, rows_out = R.N_IN, R.N_OUT
        Xs = [R.operand(kind, rows_in, cin, 10 + p, key[3]) for p in range(n_prob)]
        dYs = [R.operand(kind, rows_out, cout, 20 + p, key[3]) for p in range(n_prob)]
        res = [R.wgrad(Xs[p], dYs[p], in_rows, out_rows, prefix, relu, mask) for p in range(n_prob)]
        sdb = [R.db_abs(dYs[p], out_rows, prefix, mask) for p in range(n_prob)]
        if kind == "exact":
            for p in range(n_prob):
                R.assert_exact(res[p][2], sdb[p][0])
        _refs[key] = dict(Xs=Xs, dYs=dYs, in_rows=in_rows, out_rows=out_rows, prefix=prefix, mask=mask,
                          dW=np.stack([r[0] for r in res]), db=np.stack([r[1] for r in res]),
                          S=np.stack([r[2] for r in res]), S_db=np.stack([s[0] for s in sdb]), n_db=sdb[0][1])
    return _refs[key]


def run(gpu, L, cin, cout, bf16, lst, kind, relu=0, *, n_prob=1, with_db=True, expect=None, x_off=0, dy_off=0, dw_off=0,
        sc_off=0, pair=0, force_n=False, what=""):
    """One call of the entry point that (n_prob, bf16, with_db) selects, under the discipline of the module docstring.
    x_off / dy_off: elements the X / dY pointer of operand pair `pair` sits past a 16-byte boundary; dw_off: floats;
    sc_off: bytes.  Returns the path report."""
    lib = L.lib()
    P = _problem(kind, cin, cout, bf16, lst, relu, n_prob)
    isz = 2 if bf16 else 4
    enc = R.to_bf16_bits if bf16 else (lambda a: a)
    n_off = len(P["prefix"]) - 1
    X = [Buf(gpu, P["Xs"][p].size * isz, GUARD_ROWS * cin * isz, x_off * isz if p == pair else 0, enc(P["Xs"][p]))
         for p in range(n_prob)]
    dY = [Buf(gpu, P["dYs"][p].size * isz, GUARD_ROWS * cout * isz, dy_off * isz if p == pair else 0, enc(P["dYs"][p]))
          for p in range(n_prob)]
    rows = None
    if P["in_rows"] is not None:
        rows = [Buf(gpu, 4 * max(len(r), 1), 256, 0, r if len(r) else np.zeros(1, np.int32)) for r in (P["in_rows"], P["out_rows"])]
    ph = (C.c_int64 * (n_off + 1))(*[int(v) for v in P["prefix"]])
    if n_prob == 1:
        nbytes = lib.scn_wgrad_scratch_bytes(cin, cout, ph, n_off)
    elif n_prob == 2 and not force_n:
        nbytes = lib.scn_wgrad_scratch_bytes2(cin, cout, ph, n_off)
    else:
        nbytes = lib.scn_wgrad_scratch_bytes_n(cin, cout, ph, n_off, n_prob)
    assert nbytes > 0
    dW = Buf(gpu, 4 * n_prob * n_off * cin * cout, GUARD_BYTES, 4 * dw_off)
    db = Buf(gpu, 4 * n_prob * cout, GUARD_BYTES) if with_db else None
    scratch = Buf(gpu, nbytes, GUARD_BYTES, sc_off)
    bufs = X + dY + [dW, scratch] + ([db] if db else []) + (rows or [])

    ptr_bits = 0
    for b in X + dY:
        ptr_bits |= b.ptr & 15
    rc, d = R.describe(L, cin, cout, P["prefix"], n_prob, bf16, ptr_bits, (dW.ptr | scratch.ptr) & 15)
    assert rc == 0
    if expect is not None:
        assert {k: d[k] for k in expect} == expect, (what, d)
    assert d["bytes_db"] <= nbytes                                   # what this plan writes fits what the caller was told
    mask = P["mask"] if with_db else 0
    rin, rout = (rows[0].ptr, rows[1].ptr) if rows else (None, None)
    flags = F_RELU_IN if relu else 0
    sfx = "_bf16" if bf16 else ""

    def call():
        st = L.stream()
        if n_prob == 1 and with_db:
            fn = getattr(lib, "scn_wgrad_bias_rules" + sfx)
            return fn(X[0].ptr, cin, dY[0].ptr, cout, rin, rout, ph, n_off, dW.ptr, db.ptr, mask, scratch.ptr, flags, st)
        if n_prob == 1:
            fn = getattr(lib, "scn_wgrad_rules" + sfx)
            return fn(X[0].ptr, cin, dY[0].ptr, cout, rin, rout, ph, n_off, dW.ptr, scratch.ptr, flags, st)
        dbp = db.ptr if with_db else None
        if n_prob == 2 and not force_n:
            fn = getattr(lib, "scn_wgrad_bias_rules2" + sfx)
            return fn(X[0].ptr, dY[0].ptr, X[1].ptr, dY[1].ptr, cin, cout, rin, rout, ph, n_off, dW.ptr, dbp, mask,
                      scratch.ptr, flags, st)
        fn = getattr(lib, "scn_wgrad_bias_rules_n" + sfx)
        xs, ys = (C.c_void_p * n_prob)(*[b.ptr for b in X]), (C.c_void_p * n_prob)(*[b.ptr for b in dY])
        return fn(xs, ys, n_prob, cin, cout, rin, rout, ph, n_off, dW.ptr, dbp, mask, scratch.ptr, flags, st)

    L.check(call())
    torch.cuda.current_stream().synchronize()
    for b in bufs:
        assert b.intact(), ("guard", what, bufs.index(b))
    for b in X + dY:
        assert b.unchanged(), ("operand written", what)
    assert not dW.has_sentinel() and not (db and db.has_sentinel()), ("element not written", what)
    got_w = dW.f32().reshape(n_prob, n_off, cin, cout)
    got_b = db.f32().reshape(n_prob, cout) if db else None
    dW.reset()
    if db:
        db.reset()
    L.check(call())
    torch.cuda.current_stream().synchronize()
    assert np.array_equal(got_w.view(np.uint32), dW.f32().view(np.uint32).reshape(got_w.shape)), ("not reproducible", what)
    assert db is None or np.array_equal(got_b.view(np.uint32), db.f32().view(np.uint32).reshape(got_b.shape))
    for b in bufs:
        assert b.intact(), ("guard, second call", what)

    if kind == "exact":
        assert np.array_equal(got_w, P["dW"].astype(np.float32)), (what, "dW", float(np.abs(got_w - P["dW"]).max()))
        assert db is None or np.array_equal(got_b, P["db"].astype(np.float32)), (what, "db")
    else:
        counts = np.diff(P["prefix"]).astype(np.float64)
        lim = R.bound(counts[None, :, None, None], P["S"])
        err = np.abs(got_w.astype(np.float64) - P["dW"])
        ratio = float(np.max(np.where(lim > 0, err / np.where(lim > 0, lim, 1.0), np.where(err > 0, np.inf, 0.0))))
        ratio_b = 0.0
        if db:
            limb = R.bound(P["n_db"], P["S_db"])
            errb = np.abs(got_b.astype(np.float64) - P["db"])
            ratio_b = float(np.max(np.where(limb > 0, errb / np.where(limb > 0, limb, 1.0), np.where(errb > 0, np.inf, 0.0))))
        fam = R.family(d)
        _margins[fam] = max(_margins.get(fam, 0.0), ratio, ratio_b)
        print(f"[margin] {fam}: {what} dW {ratio:.3f} db {ratio_b:.3f} of the bound")
        assert ratio <= 1.0 and ratio_b <= 1.0, (what, ratio, ratio_b)
    return d


# ------------------------------------------------------------------------------------------------------------------------
# the shape table x the unit plans, on list (a)
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", R.SHAPES, ids=R.shape_id)
def test_every_shape_on_the_edge_count_list_under_every_unit_plan(gpu, L, shape):
    """List (a) (27 offsets, counts around 4 / 64 / 128 / 256 / 512 / 1025 rules, empty offsets first, last and side by side)
    under the chip's own unit plan (exact and gaussian), one unit per offset, two units for the 1025-rule offset, `per` on its
    floor (3 / 9 / 5 units) and a 32-CU budget: bias gradient over an empty, the centre, the longest and a one-rule offset."""
    cin, cout, bf16, sw, path = shape
    sid = R.shape_id(shape)
    for plan in R.PLANS:
        with R.switches(L, {**sw, **plan}):
            exp = dict(path)
            if plan.get("SCN_WGRAD_SPLITS") == "4096":
                exp["per"] = R.floor_per(path)
            d = run(gpu, L, cin, cout, bf16, "A", "exact", relu=1, expect=exp, what=f"{sid} {plan} exact")
            if plan.get("SCN_WGRAD_SPLITS") == "1":
                assert d["units"] == sum(c > 0 for c in R.COUNTS_A)
            if plan.get("SCN_WGRAD_SPLITS") == "5":
                assert d["per"] > R.floor_per(path) and -(-1025 // d["per"]) == 2
            if plan.get("SCN_WGRAD_SPLITS") in (None, "4096"):
                run(gpu, L, cin, cout, bf16, "A", "gaussian", relu=0, expect=exp, what=f"{sid} {plan} gaussian")


@pytest.mark.parametrize("fam", R.FAMILIES, ids=R.shape_id)
def test_every_rule_list_on_one_shape_per_kernel_family(gpu, L, fam):
    """(c) no rules at all (memsets: exactly zero), (d) one offset; eight offsets all in the bias gradient with rows repeated
    ~40 times (a Deconvolution); 32 offsets with bit 31 in the bias mask; prefix_host[0] = 7, (e) the identity list of 1, 4, 500
    and 513 rows, (f) with and without the input ReLU; without a bias gradient too."""
    cin, cout, bf16, sw = fam
    path = next(s[4] for s in R.SHAPES if s[:4] == fam)
    sid = R.shape_id(fam)
    with R.switches(L, sw):
        for relu in (0, 1):
            run(gpu, L, cin, cout, bf16, "empty", "exact", relu, expect={"memset": 1, "units": 0}, what=f"{sid} empty")
            for lst in ("one", "deconv8", "wide32", "A7"):
                run(gpu, L, cin, cout, bf16, lst, "exact", relu, expect=path, what=f"{sid} {lst} relu {relu}")
            for n in R.IDENT_ROWS:
                run(gpu, L, cin, cout, bf16, n, "exact", relu, expect=path, what=f"{sid} identity {n} relu {relu}")
        run(gpu, L, cin, cout, bf16, "deconv8", "gaussian", 1, expect=path, what=f"{sid} deconv8 gaussian")
        run(gpu, L, cin, cout, bf16, 513, "gaussian", 0, expect=path, what=f"{sid} identity 513 gaussian")
        run(gpu, L, cin, cout, bf16, "A", "exact", 0, with_db=False, expect=path, what=f"{sid} no db")
        run(gpu, L, cin, cout, bf16, "empty", "exact", 0, with_db=False, expect={"memset": 1}, what=f"{sid} empty, no db")


# ------------------------------------------------------------------------------------------------------------------------
# alignment
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("c", [32, 64, 128, 48])
def test_pointers_one_element_off_take_the_element_and_scalar_routes(gpu, L, c, bf16):
    """X, then dY, one element past a 16-byte boundary: fp32 rows go EDGE without vector pieces (the 48-wide blocks read
    three-dword pieces and stay), bf16 rows leave k_wgrad_tb for k_wgrad_direct<..., HB>, element loads.  dW one float off,
    then the scratch four bytes off: the unit sum runs one channel per thread; the unit kernel stays."""
    sid = f"{c}x{c} {'bf16' if bf16 else 'fp32'}"
    aligned = _aligned(c, c, bf16)
    if bf16:
        off_path = R.mk_path("d", 4 if c > 32 else 2, 4 if c > 32 else 2, quad=int(c > 64), edge=1, hb=1)
    elif c == 48:
        off_path = aligned
    else:
        off_path = dict(aligned, edge=1, evec=0)
    for kw in ({"x_off": 1}, {"dy_off": 1}):
        run(gpu, L, c, c, bf16, "A", "exact", 1, expect=off_path, what=f"{sid} {kw}", **kw)
    run(gpu, L, c, c, bf16, "A", "gaussian", 0, expect=off_path, what=f"{sid} x_off gaussian", x_off=1)
    for kw in ({"dw_off": 1}, {"sc_off": 4}):
        run(gpu, L, c, c, bf16, "A", "exact", 1, expect=dict(aligned, V=1), what=f"{sid} {kw}", **kw)
        run(gpu, L, c, c, bf16, "deconv8", "gaussian", 0, expect=dict(aligned, V=1), what=f"{sid} {kw} gaussian", **kw)


def test_operands_not_aligned_to_their_element_are_refused_without_a_launch(gpu, L):
    lib = L.lib()
    _, _, prefix, _ = R.make_list("A")
    ph = (C.c_int64 * 28)(*[int(v) for v in prefix])
    x = torch.zeros(R.N_IN * 32 + 8, device=gpu)
    y = torch.zeros(R.N_OUT * 32 + 8, device=gpu)
    rows = torch.zeros(int(prefix[-1]), dtype=torch.int32, device=gpu)
    dW = torch.full((27 * 32 * 32,), 7.0, device=gpu)
    sc = torch.empty(lib.scn_wgrad_scratch_bytes(32, 32, ph, 27), dtype=torch.uint8, device=gpu)
    before = (C.c_int64 * 4)()
    lib.scn_wgrad_group_counts(before, 0)
    assert lib.scn_wgrad_rules(x.data_ptr() + 2, 32, y.data_ptr(), 32, rows.data_ptr(), rows.data_ptr(), ph, 27,
                               dW.data_ptr(), sc.data_ptr(), 0, L.stream()) == L.EINVAL
    assert lib.scn_wgrad_rules_bf16(x.data_ptr(), 32, y.data_ptr() + 1, 32, rows.data_ptr(), rows.data_ptr(), ph, 27,
                                    dW.data_ptr(), sc.data_ptr(), 0, L.stream()) == L.EINVAL
    after = (C.c_int64 * 4)()
    lib.scn_wgrad_group_counts(after, 0)
    assert list(before) == list(after) and bool((dW == 7.0).all())
    assert R.describe(L, 32, 32, prefix, 1, False, 2, 0)[0] == L.EINVAL


# ------------------------------------------------------------------------------------------------------------------------
# entry points
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("n_prob", [1, 2, 3, 4])
def test_every_entry_point_with_and_without_the_bias_gradient(gpu, L, n_prob, bf16):
    """scn_wgrad_rules / _bias_rules (n_prob 1), _bias_rules2 and _bias_rules_n with 2, 3 and 4 operand pairs, fp32 and bf16,
    db given and NULL (db_offsets 0); one call in which the second operand pair alone is misaligned (the whole launch takes
    the element route)."""
    for cin, cout in [(32, 32), (64, 64), (128, 128)]:
        aligned = _aligned(cin, cout, bf16)
        sid = f"{cin}x{cout} {'bf16' if bf16 else 'fp32'} n_prob {n_prob}"
        for with_db in (True, False):
            run(gpu, L, cin, cout, bf16, "A", "exact", 1, n_prob=n_prob, with_db=with_db, expect=aligned,
                what=f"{sid} db {with_db}")
        run(gpu, L, cin, cout, bf16, "A", "gaussian", 0, n_prob=n_prob, expect=aligned, what=f"{sid} gaussian")
    if n_prob == 2:
        run(gpu, L, 64, 64, bf16, "deconv8", "exact", 0, n_prob=2, force_n=True, expect=_aligned(64, 64, bf16),
            what="rules_n with two pairs")
    if n_prob > 1:
        exp = R.mk_path("d", 4, 4, edge=1, hb=1) if bf16 else R.mk_path("d", 4, 4, edge=1)
        run(gpu, L, 64, 64, bf16, "A", "exact", 1, n_prob=n_prob, expect=exp, x_off=1, pair=1, what=f"pair 1 of {n_prob} off")
        run(gpu, L, 64, 64, bf16, "A", "exact", 1, n_prob=n_prob, with_db=False, expect=exp, dy_off=1, pair=n_prob - 1,
            what=f"last pair of {n_prob} off, no db")


def test_a_call_on_a_side_stream(gpu, L):
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        assert L.stream() != 0 and L.stream() == s.cuda_stream
        run(gpu, L, 64, 64, False, "A", "exact", 1, expect=R.mk_path("d", 4, 4), what="side stream fp32")
        run(gpu, L, 64, 64, True, "A", "exact", 1, expect=R.mk_path("t", 2, 2), what="side stream bf16")
        s.synchronize()


def test_tile_major_weight_gradient_is_exact_on_integer_operands(gpu, L):
    """scn_wgrad_tiles32 (32 -> 32 SubM 3^3 from the forward kernel's tile tables) on a 900-voxel scene: bit-equal to the
    restatement on the exact operands, with and without the input ReLU, as scn_wgrad_rules is on the same rule list."""
    import sparse_rcnn_amd as scn
    from sparse_rcnn_amd.synthetic import make_batch
    lib = L.lib()
    coords, feats, size, bs, _ = make_batch(1, (24, 24, 16), 900, seed=3, cin=3)
    x = scn.InputLayer(3, size, mode=4)((coords, feats.to(gpu), bs))
    rb = x.metadata.subm_rulebook(tuple(int(v) for v in size), 3)
    n, r, t = rb.n, rb.rules, rb.tiles
    prefix = np.asarray(r.prefix_list(), dtype=np.int64)
    in_rows, out_rows = r.in_rows.cpu().numpy(), r.out_rows.cpu().numpy()
    assert n > 100 and len(prefix) == 28 and int(prefix[-1]) == len(in_rows)
    Xh, dYh = R.operand("exact", n, 32, 31), R.operand("exact", n, 32, 32)
    X = Buf(gpu, Xh.size * 4, GUARD_ROWS * 128, 0, Xh)
    dY = Buf(gpu, dYh.size * 4, GUARD_ROWS * 128, 0, dYh)
    s1 = Buf(gpu, lib.scn_wgrad_tiles32_scratch_bytes(), GUARD_BYTES)
    s0 = Buf(gpu, lib.scn_wgrad_scratch_bytes(32, 32, r.prefix_host, 27), GUARD_BYTES)
    for relu in (0, 1):
        ref, _, S = R.wgrad(Xh, dYh, in_rows, out_rows, prefix, relu, 0)
        R.assert_exact(S)
        dW0, dW1 = Buf(gpu, 4 * 27 * 32 * 32, GUARD_BYTES), Buf(gpu, 4 * 27 * 32 * 32, GUARD_BYTES)
        L.check(lib.scn_wgrad_tiles32(X.ptr, n, dY.ptr, n, L.ptr(t.tstab), L.ptr(t.tile_mask), L.ptr(t.perm), r.prefix_host,
                                      dW1.ptr, s1.ptr, relu, L.stream()))
        L.check(lib.scn_wgrad_rules(X.ptr, 32, dY.ptr, 32, L.ptr(r.in_rows), L.ptr(r.out_rows), r.prefix_host, 27, dW0.ptr,
                                    s0.ptr, relu, L.stream()))
        torch.cuda.synchronize()
        for b in (X, dY, s0, s1, dW0, dW1):
            assert b.intact()
        assert X.unchanged() and dY.unchanged() and not dW0.has_sentinel() and not dW1.has_sentinel()
        assert np.array_equal(dW1.f32().reshape(27, 32, 32), ref.astype(np.float32)), ("tiles32", relu)
        assert np.array_equal(dW0.f32().reshape(27, 32, 32), ref.astype(np.float32)), ("rules", relu)


def test_zz_largest_ratio_to_the_bound_per_kernel_family(gpu):
    """(Runs last in the file: the summary line of the [margin] prints above.)"""
    for fam in sorted(_margins):
        print(f"[margin] family {fam}: largest |error| / bound {_margins[fam]:.3f}")
    assert all(v <= 1.0 for v in _margins.values())
