"""Pins tests/conv_bf16_restate.py (what the bf16 tile-convolution path tests compare against) on the CPU: the bf16 rounding
against torch, the interval check of the gaussian kind on fp32 accumulations in two orders (and that it rejects an output two
bf16 ulps away), the exactness precondition, the representability cap and the rounding ties of the exact kind for every
tabulated case -- and, without a GPU, that every row of the case table names the path scn_conv_tiles_bf16_plan_describe reports
(the entry point is host-only) and that the table reaches exactly the branches of the launcher."""
import ctypes as C

import numpy as np
import pytest
import torch

import conv_bf16_restate as B
import conv_restate as R


def test_bf16_rounding_equals_torch():
    """Ties of both parities, negative values, the subnormal edge, -0.0 -- and a few thousand ordinary numbers."""
    bits = np.array([0x3F808000, 0x3F818000, 0x3F807FFF, 0x3F808001, 0xBF808000, 0xBF818000, 0x437F8000, 0x43808000,   # ties ...
                     0x00800000, 0x007FFFFF, 0x00808000, 0x00008000, 0x00018000, 0x80008000, 0x00000001,               # the edge
                     0x80000000, 0x00000000, 0x7F7F0000, 0xC3808000, 0x43818000], dtype=np.uint32)
    v = np.concatenate([bits.view(np.float32), np.arange(-600, 600, dtype=np.float32) / 2,
                        R.operand("gaussian", 50, 64, 9).reshape(-1) * 40.0])
    want = torch.from_numpy(v).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    got = B.to_bf16_bits(v)
    assert np.array_equal(got, want)
    assert got[15] == 0x8000 and got[0] == 0x3F80 and got[1] == 0x3F82          # -0.0 stays; ties go to the even neighbour
    assert np.array_equal(B.from_bf16_bits(got).view(np.uint32), got.astype(np.uint32) << 16)
    # odd integers in 257..511 are exact ties, the even neighbour wins
    odd = np.arange(257, 512, 2, dtype=np.float32)
    r = B.bf16_round(odd)
    assert np.all(np.abs(r - odd) == 1) and np.all((r / 2) % 2 == 0)
    assert np.array_equal(B.bf16_round(np.arange(-256, 257, dtype=np.float32)), np.arange(-256, 257, dtype=np.float32))
    # outward roundings to fp32
    x = np.array([0.1, -0.1, 1.0, 1.0 + 2.0 ** -30, -(1.0 + 2.0 ** -30)])
    assert np.all(B.down32(x).astype(np.float64) <= x) and np.all(B.up32(x).astype(np.float64) >= x)
    assert B.down32(x)[2] == 1.0 == B.up32(x)[2] and B.up32(x)[3] == np.float32(1.0 + 2.0 ** -23) and B.down32(x)[3] == 1.0
    assert B.half_ulp_bf16(np.array([1.0, 1.99, 2.0, -300.0])).tolist() == [2.0 ** -8, 2.0 ** -8, 2.0 ** -7, 1.0]


class _C:
    """(what `operands` / `reference` read of a case)"""

    def __init__(self, cin, cout, n_off, flagset):
        self.cin, self.cout, self.n_off, self.flagset = cin, cout, n_off, flagset
        self.flags, self.operands = R.FLAGSETS[flagset]


def test_the_interval_accepts_fp32_accumulation_in_two_orders_and_rejects_two_ulps():
    """The restatement's own terms of a row, summed in fp32 front to back and as a pairwise tree from the far end, rounded to
    bf16 once: inside.  The same output moved by two bf16 ulps in any one element: outside.  Zeroed elements: exactly +0, or
    exactly the residual's bits."""
    c = _C(32, 4, 27, "bwd_res_last")
    rows = R.small_rows(27)
    ops = B.operands("gaussian", c, rows)
    Y, E, zeroed, res_bits = B.reference("gaussian", c, rows)
    table = B.table_of(27, rows)[0]
    W = B.bf16_round(ops["w"])                                       # [o][cout][cin], offsets reversed
    pick = (0, 17, 400, rows - 1)
    outs = {"fwd": np.zeros((len(pick), c.cout), np.float32), "tree": np.zeros((len(pick), c.cout), np.float32)}
    for a, row in enumerate(pick):
        for n in range(c.cout):
            terms = [np.float32(ops["x"][table[o][row]][k] * W[26 - o][n][k]) for o in range(27) if table[o][row] >= 0
                     for k in range(c.cin)]
            fwd = np.float32(0)
            for t in terms:
                fwd = np.float32(fwd + t)
            parts = list(reversed(terms))
            while len(parts) > 1:
                parts = [np.float32(parts[k] + parts[k + 1]) if k + 1 < len(parts) else parts[k] for k in range(0, len(parts), 2)]
            for name, v in (("fwd", fwd), ("tree", parts[0])):
                v = np.float32(0) if zeroed[row][n] else v
                outs[name][a][n] = np.float32(v + ops["residual"][row][n])
    sel = np.array(pick)
    args = (Y[sel], E[sel], zeroed[sel], res_bits[sel])
    assert zeroed[sel].any() and not zeroed[sel].all()
    for name, o in outs.items():
        bits = B.to_bf16_bits(o)
        bad, margin, share = B.check_interval(bits, *args)
        assert bad == 0 and margin <= 1.0 and 0.0 <= share <= 1.0, (name, bad, margin)
        for idx in np.ndindex(*bits.shape):
            for step in (2, -2):
                moved = bits.copy()
                # two ulps: the neighbour after next in the ordered bf16 numbers (sign-magnitude: step the magnitude, across
                # zero flip the sign)
                m = int(moved[idx] & 0x7FFF) + (step if not moved[idx] & 0x8000 else -step)
                moved[idx] = (moved[idx] & 0x8000) | m if m >= 0 else (~moved[idx] & 0x8000) | (-m)
                assert B.check_interval(moved, *args)[0] == 1, (name, idx, step)
    # a zeroed element must be exactly +0 without a residual
    z = np.array([[True, False]])
    y, e = np.array([[0.0, 1.0]]), np.array([[1e-6, 1e-6]])
    assert B.check_interval(np.array([[0x0000, 0x3F80]], np.uint16), y, e, z)[0] == 0
    assert B.check_interval(np.array([[0x8000, 0x3F80]], np.uint16), y, e, z)[0] == 1       # -0
    assert B.check_interval(np.array([[0x0001, 0x3F80]], np.uint16), y, e, z)[0] == 1
    assert B.check_interval(np.array([[0x0000, 0x7FC0]], np.uint16), y, e, z)[0] == 1       # NaN is outside
    assert B.check_interval(np.array([[0x4000, 0x3F80]], np.uint16), y, e, z, np.array([[0x4000, 0]], np.uint16))[0] == 0


# ------------------------------------------------------------------------------------------------------------------------
# the path report (host only)
# ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def L():
    import __graft_entry__
    __graft_entry__.build()
    from sparse_rcnn_amd import _lib
    return _lib


def _report(L, c):
    rows = B.table_rows(L, c)
    with R.switches(L, c.sw):
        rc, d = B.describe(L, R.N_IN_FACTOR[c.n_off] * rows, c.cin, c.n_off, rows, c.cout, c.flags, c.arrival, *c.ptr_bits())
        lib = L.load()                                               # (the sizes follow the shape switches too)
        d["sizes"] = (lib.scn_conv_tiles_bf16_arrival_counters(c.cin, rows, c.cout),
                      lib.scn_conv_tiles_bf16_scratch_bytes(c.cin, rows, c.cout),
                      lib.scn_conv_tiles_bf16_image_bytes(c.cin, c.cout, c.n_off))
    assert rc == 0
    return rows, d


def cdiv(a, b):
    return -(-a // b)


@pytest.mark.parametrize("group", B.GROUPS)
def test_exact_cases_are_representable_and_hit_ties(L, group):
    """The exactness precondition (through |x|, |w| <= 3 and on the operands: `reference` asserts it), and the condition that
    keeps the exact kind sharp: at least three quarters of the compared elements are integers bf16 holds."""
    seen, ties = set(), 0
    for c in [c for c in B.CASES if c.group == group]:
        assert c.cin <= 256 and c.n_off <= 27 and 9 * c.cin * c.n_off + 6 < R.EXACT_LIMIT
        rows = B.table_rows(L, c)
        key = (c.cin, c.cout, c.n_off, rows, c.flagset)
        if key in seen:
            continue
        seen.add(key)
        bits, Y = B.reference("exact", c, rows)
        assert np.array_equal(Y, np.round(Y)) and bits.shape == (rows, c.cout)
        share = float((np.abs(Y) <= 256).mean())
        assert share >= 0.75, (c.id(), share)
        ties += int(((np.abs(Y) > 256) & (np.abs(Y) < 512) & (Y % 2 == 1)).sum())
    assert ties > 0 or group in ("NB forced", "single chunk NB2", "single chunk NB4"), group      # (32 input channels: none)


@pytest.mark.parametrize("group", B.GROUPS)
def test_every_case_names_the_reported_path(L, group):
    for c in [c for c in B.CASES if c.group == group]:
        rows, d = _report(L, c)
        assert {k: d[k] for k in c.expect} == c.expect, (c.id(), d)
        nt = cdiv(rows, 16)
        assert d["nt"] == nt and rows % 16 != 0 and rows <= R.MAX_ROWS
        ct = 16 * d["nb"]
        assert d["sizes"] == ((nt * d["n_chunks"] if d["n_kc"] > 1 else 0),
                              256 + (d["n_kc"] * nt * 16 * d["n_chunks"] * ct * 4 if d["n_kc"] > 1 else 0),
                              d["n_chunks"] * d["n_kc"] * c.n_off * ct * 32 * d["kh"] * 2), (c.id(), d)
        if d["stream"]:
            batches = cdiv(nt, d["nw"])
            assert nt % d["nw"] != 0 and 1 <= d["n_wgb"] <= batches and d["grid_x"] == cdiv(d["n_wgb"], 8) * 8 * d["n_chunks"]
            assert (cdiv(nt, 8) * d["n_chunks"] < 224) == (d["nw"] == 4)
            assert (d["n_wgb"] < batches) == (c.table == "s8cap")    # only there a workgroup walks more than one batch
        else:
            assert 1 <= d["n_tg"] <= cdiv(nt, 16) and d["grid_x"] == d["n_tg"] * d["n_kc"] * d["n_chunks"]
            if c.table == "long":                                    # ~4 tiles per wave
                assert 3.5 <= nt / (16 * d["n_tg"]) <= 4.5, (c.id(), d)
            if c.table == "xcd":
                assert d["n_tg"] >= 8


def _features(c, d):
    """What a case covers beyond its kernel instantiation: the instantiation with the live / dead parts of its shape, the
    K-chunk count up to the combiner's second flush round, the hand-out, each misaligned buffer by kernel."""
    s = B.SHAPES[(c.cin, c.cout, c.variant)]
    f = set(B.branches_of(d, c.n_off))
    if d["stream"]:
        f.add(("tbs", d["ks"], c.n_off, d["nw"], d["vec_ok"], s["dead_cols"] > 0, d["n_wgb"] < cdiv(d["nt"], d["nw"])))
    else:
        f.add(("tb", d["nb"], d["kh"], d["fused"], d["part"], min(d["n_kc"], 5), d["n_chunks"] > 1, s["dead_cols"] > 0,
               s["dead_plane"], d["vec_ok"], c.n_off))
        f.add(("xbins", d["xbins"]))
    f |= {("off", o, b, d["stream"], d["nb"], d["sum_v"]) for o, b in c.off.items()}
    return f


def test_the_case_table_reaches_exactly_the_branches_of_the_launcher(L):
    """Over the reports, not over the table's own expectations.  And no case group can be deleted: each is the only one to
    cover something (a deleted group fails here)."""
    reached, per_group = set(), {}
    for c in B.CASES:
        _, d = _report(L, c)
        reached |= B.branches_of(d, c.n_off)
        per_group.setdefault(c.group, set()).update(_features(c, d))
    assert reached == B.LAUNCH_BRANCHES_BF16, (B.LAUNCH_BRANCHES_BF16 - reached, reached - B.LAUNCH_BRANCHES_BF16)
    assert set(per_group) == {"single chunk NB2", "single chunk NB4", "K split", "KH2", "NB forced", "stream", "alignment",
                              "xcd order"}
    only = {g: f - set().union(*(v for h, v in per_group.items() if h != g)) for g, f in per_group.items()}
    assert all(only.values()), [g for g, v in only.items() if not v]
    assert only["stream"] >= {("tbs", ks, no, nw) for ks in (2, 4, 8) for no in (27, 8) for nw in (8, 4)} - {("tbs", 2, 27, 4)}
    assert only["KH2"] >= {("tb", 2, 2, fu, pt) for fu in (0, 1) for pt in (0, 1)} - {("tb", 2, 2, 0, 0)}
    assert {f for f in only["xcd order"] if f[0] == "xbins"} == {("xbins", 2), ("xbins", 4), ("xbins", 8)}
    assert any(f[0] == "tbs" and len(f) > 4 and f[6] for f in only["stream"])              # n_wgb capped: two batches
    assert any(f[0] == "tb" and len(f) > 5 and f[5] == 5 and f[3] for f in only["K split"])  # a second R4 flush round
    # and what the table names beyond that
    e = [c.expect for c in B.CASES]
    assert {x["xbins"] for x in e} == {0, 1, 2, 4, 8}
    assert {c.table for c in B.CASES} == set(B.TABLES)
    assert {(x["stream"], x["vec_ok"]) for x in e} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    assert any(c.gaussian and c.expect["fused"] for c in B.CASES) and any(c.gaussian and c.expect["sum"] for c in B.CASES)
    assert sum(c.gaussian for c in B.CASES) >= 24                    # 12 + 12 instantiations


def test_switches_and_pointer_bits_move_the_reported_path(L):
    def d(cin, cout, flags=0, arrival=True, n=889, n_off=27, **bits):
        rc, out = B.describe(L, n, cin, n_off, n, cout, flags, arrival, **bits)
        assert rc == 0
        return out

    base = d(64, 32)
    assert (base["nb"], base["kh"], base["n_kc"], base["fused"], base["vec_ok"], base["sum"], base["stream"]) == (2, 1, 2, 1, 1, 0, 0)
    assert d(64, 32, y_bits=2)["vec_ok"] == 0 and d(64, 32, y_bits=4)["vec_ok"] == 1 and d(64, 31)["vec_ok"] == 0
    assert d(32, 64, y_bits=4)["vec_ok"] == 0 and d(32, 64, y_bits=8)["vec_ok"] == 1 and d(32, 70)["vec_ok"] == 0
    assert d(64, 32, arrival=False)["sum_v"] == 4 and d(64, 32, R.F_SPLIT_SUM)["sum_v"] == 4 and d(64, 32)["sum_v"] == 0
    for bits, v in ((dict(y_bits=2), 1), (dict(y_bits=4), 1), (dict(y_bits=8), 4), (dict(s_bits=4), 1), (dict(s_bits=8), 1)):
        assert d(64, 32, arrival=False, **bits)["sum_v"] == v, bits
    assert d(64, 30, arrival=False)["sum_v"] == 1 and d(64, 30, arrival=False)["vec_ok"] == 1
    assert d(32, 32, arrival=False)["sum"] == 0                      # one K-chunk: no K reduction
    # the stream kernel: by default only two K-chunks with 27 offsets
    s = d(64, 64)
    assert (s["stream"], s["ks"], s["nw"], s["n_wgb"], s["fused"], s["sum"], s["n_tg"], s["xbins"]) == (1, 2, 4, 14, 0, 0, 0, 0)
    assert d(64, 64, arrival=False)["stream"] == 1 and d(64, 64, R.F_SPLIT_SUM)["stream"] == 0
    assert d(64, 64, n_off=8)["stream"] == 0 and d(128, 64)["stream"] == 0 and d(64, 32)["stream"] == 0
    with L.debug_switch("SCN_TB_STREAM", 1):
        assert d(64, 64, n_off=8)["stream"] == 1 and d(128, 64)["ks"] == 4 and d(256, 64)["ks"] == 8
        assert d(96, 64)["stream"] == 0 and d(64, 32)["stream"] == 0 and d(72, 64)["stream"] == 0 and d(64, 64, n_off=12)["stream"] == 0
        assert d(512, 64)["stream"] == 0
        big = d(128, 128, n=16389)
        assert (big["nw"], big["n_wgb"], big["grid_x"]) == (8, 128, 256) and d(128, 128, n=16389 - 16)["n_wgb"] == 128
        assert d(64, 64, n=16 * 8 * 223)["nw"] == 4 and d(64, 64, n=16 * 8 * 223 + 1)["nw"] == 8
        with L.debug_switch("SCN_TB_KH", 2):
            assert d(64, 64)["stream"] == 0
        with L.debug_switch("SCN_TB_NB", 2):
            assert d(64, 64)["stream"] == 0
    with L.debug_switch("SCN_TB_STREAM", 0):
        t = d(64, 64)
        assert (t["stream"], t["fused"], t["nb"], t["n_kc"]) == (0, 1, 4, 2)
    with L.debug_switch("SCN_TB_KH", 2):
        k = d(96, 32)
        assert (k["kh"], k["nb"], k["n_kc"], k["part"]) == (2, 2, 2, 1) and d(32, 64)["kh"] == 1 and d(128, 64)["nb"] == 2
    with L.debug_switch("SCN_TB_NB", 4):
        assert d(32, 16)["nb"] == 4 and d(32, 16)["n_chunks"] == 1
    with L.debug_switch("SCN_CU_BUDGET", 32):
        assert d(32, 32, n=40000)["n_tg"] == 64 and d(64, 32, n=40000)["n_tg"] == 32 and d(32, 64, n=40000)["n_tg"] == 32
    assert d(32, 32, n=40000)["n_tg"] == cdiv(cdiv(40000, 16), 16)
    # XCD-local hand-out
    X = B.F_TILE_ORDER_X
    assert d(32, 32, X, n=4101)["xbins"] == 8 and d(64, 32, X, n=4101)["xbins"] == 4 and d(32, 32, n=4101)["xbins"] == 1
    assert d(32, 32, X)["xbins"] == 1                                # 4 workgroups per slice: fewer than 8
    with L.debug_switch("SCN_TB_NO_XORDER", 1):
        assert d(32, 32, X, n=4101)["xbins"] == 1
    zero = d(64, 64, n=0)
    assert all(v == 0 for v in zero.values())


def test_bad_arguments_and_odd_pointer_bits_are_refused(L):
    lib = L.load()
    out = (C.c_int64 * 18)()
    ok = (889, 32, 27, 889, 32, 0, 1, 0, 0)
    assert lib.scn_conv_tiles_bf16_plan_describe(*ok, out) == L.OK
    for pos, bad in ((2, 28), (2, 0), (1, 0), (1, 4), (1, 12), (1, 36), (4, 0), (0, -1), (3, -1), (7, 1), (7, 3), (7, 16), (7, -2),
                     (8, 2), (8, 1), (8, 16), (0, 1 << 23), (3, 1 << 23)):
        args = list(ok)
        args[pos] = bad
        assert lib.scn_conv_tiles_bf16_plan_describe(*args, out) == L.EINVAL, (pos, bad)
    assert lib.scn_conv_tiles_bf16_plan_describe(*ok, None) == L.EINVAL
    for pos, good in ((7, 2), (7, 6), (7, 14), (8, 4), (8, 12), (4, 1), (4, 23), (1, 8)):
        args = list(ok)
        args[pos] = good
        assert lib.scn_conv_tiles_bf16_plan_describe(*args, out) == L.OK, (pos, good)
