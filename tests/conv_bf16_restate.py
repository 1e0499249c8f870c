"""The bf16 tile convolution (csrc/scn_conv_ts_bf16.hip: scn_conv_tiles_bf16 with k_conv_tb, the weight-streaming k_conv_tbs,
k_conv_tb_sum and the pack behind it) restated on top of tests/conv_restate.py: the same float64 `conv`, rule tables, bound and
flag sets, on operands that already ARE bf16 numbers, with the one rounding of the output stated on its own, and the case table
of the launcher's paths.  tests/test_conv_bf16_restate_cpu.py pins it and holds every case to the path
scn_conv_tiles_bf16_plan_describe reports; tests/test_gpu_conv_bf16_paths.py compares every launcher path of the HIP kernels
with it.

    Y[r] = bf16_rne( epi( bias + sum_o in(X[table[o][r]]) . bf16_rne(Wo(o)), residual[r], relu_mask[r] ) )

X, residual and relu_mask are bf16 (rounded with to_bf16_bits), W is rounded the same way (what the pack stores; the pack's
layout is pinned by test_bf16_weight_image_layout_bit_for_bit), bias stays fp32.  SCN_F_W_TRANSPOSED / SCN_F_OFF_REVERSE are
properties of the packed image: the pack gets them, the convolution ignores them.

  exact     integers in [-3, 3] (mask values from MASK_VALUES): the fp32 accumulation is exact in every order (assert_exact), the
            kernel's one rounding is round-to-nearest-even, so the expected BITS are to_bf16_bits(float32(Y64)).  bf16 holds
            integers exactly only up to 256 (above, the final rounding can swallow a wrong term of 1): in every exact case at
            least three quarters of the compared elements have |Y64| <= 256 (the worst shape, 256 input channels with 27
            offsets, has 87 %), and odd integers in 257..511 -- exact ties of the rounding -- occur.
  gaussian  standard normal rounded to bf16.  The fp32 value the kernel rounds lies within E = bound(N, S) of Y64 (gamma_{N+2} S,
            u = 2^-24: a sum of N rounded products in ANY order; nothing in it is measured), and rounding is monotone, so
                bf16_rne(down32(Y64 - E)) <= out <= bf16_rne(up32(Y64 + E))        (down32 / up32: outward to fp32)
            as real numbers.  Elements the mask zeroes are exactly +0 -- under SCN_F_RESIDUAL_LAST exactly the residual's bits.

Out of scope: the >= 2^23-row limits, cout > 4096 (the stream kernel's workgroup cap below 8), scn_conv_tiles_chain
(tests/test_gpu_chain.py), the step executor (tests/test_gpu_exec.py).
No project import: the library handle (sparse_rcnn_amd._lib) is passed in where the path report is asked for.
"""
import ctypes as C

import numpy as np

from conv_restate import (BWD, F_OFF_REVERSE, F_RELU_IN, F_RESIDUAL_LAST, F_SPLIT_SUM, F_W_TRANSPOSED, FLAGSETS, FOUR,  # noqa: F401
                          MASK_VALUES, MAX_ROWS, N_IN_FACTOR, assert_exact, bound, check_tiles, conv, mask_operand, operand,
                          rule_table, small_rows, switches, unnamed_rows)
from wgrad_restate import from_bf16_bits, to_bf16_bits

F_TILE_ORDER_X = 64
NAN_BF16 = 0x7FC0                # the quiet NaN of the guards: positive, so the packed-integer input ReLU (a max against 0 on
                                 # int16) keeps it -- a negative NaN would be zeroed and hide a stray gather


# ------------------------------------------------------------------------------------------------------------------------
# The one rounding of the output, and the interval of the gaussian kind
# ------------------------------------------------------------------------------------------------------------------------
def bf16_round(a):
    """float32 -> the float32 value of its bf16 rounding (nearest even)."""
    return from_bf16_bits(to_bf16_bits(a))


def down32(v):
    """float64 -> the largest float32 <= v."""
    v = np.asarray(v, dtype=np.float64)
    f = v.astype(np.float32)
    return np.where(f.astype(np.float64) > v, np.nextafter(f, np.float32(-np.inf)), f).astype(np.float32)


def up32(v):
    """float64 -> the smallest float32 >= v."""
    v = np.asarray(v, dtype=np.float64)
    f = v.astype(np.float32)
    return np.where(f.astype(np.float64) < v, np.nextafter(f, np.float32(np.inf)), f).astype(np.float32)


def half_ulp_bf16(v):
    """Half a bf16 ulp (8 significand bits) at |v|, float64; at zero that of the smallest normal."""
    a = np.maximum(np.abs(np.asarray(v, dtype=np.float64)), 2.0 ** -126)
    return np.exp2(np.floor(np.log2(a)) - 8.0)


def check_interval(out_bits, Y64, E, zeroed=None, res_bits=None):
    """The gaussian kind's check of an output (uint16 bits) against (Y64, E).  zeroed: bool array, the elements the ReLU mask
    zeroes (None: no mask); res_bits: under SCN_F_RESIDUAL_LAST the residual's bits -- what a zeroed element must hold instead
    of +0.  -> (number of elements outside, margin, share): margin = the largest |out - Y64| / (E + half a bf16 ulp of Y64)
    over the elements the mask lets through, share = the fraction of them whose interval admits more than one bf16 value."""
    out_bits = np.asarray(out_bits, dtype=np.uint16)
    live = np.ones(Y64.shape, dtype=bool) if zeroed is None else ~zeroed
    lo = bf16_round(down32(Y64 - E)).astype(np.float64)
    hi = bf16_round(up32(Y64 + E)).astype(np.float64)
    out = from_bf16_bits(out_bits).astype(np.float64)
    with np.errstate(invalid="ignore"):
        bad = live & ~((lo <= out) & (out <= hi))                   # (a NaN output is outside)
    if zeroed is not None:
        want = np.zeros(Y64.shape, dtype=np.uint16) if res_bits is None else np.asarray(res_bits, dtype=np.uint16)
        bad |= zeroed & (out_bits != want)
    if not live.any():
        return int(bad.sum()), 0.0, 0.0
    with np.errstate(invalid="ignore"):
        ratio = np.abs(out - Y64)[live] / (E + half_ulp_bf16(Y64))[live]
    margin = float(np.nanmax(ratio)) if not np.isnan(ratio).all() else float("inf")
    return int(bad.sum()), margin, float((lo != hi)[live].mean())


# ------------------------------------------------------------------------------------------------------------------------
# Operands and references (cached: the CPU and the GPU test see the same numbers)
# ------------------------------------------------------------------------------------------------------------------------
_tables, _ops, _refs = {}, {}, {}


def table_of(n_off, rows):
    key = (n_off, rows)
    if key not in _tables:
        table, n_in = rule_table(n_off, rows)
        _tables[key] = (table, n_in, unnamed_rows(table, n_in))
    return _tables[key]


def _draw(kind, rows, c, seed, bf16=True):
    key = (kind, rows, c, seed, bf16)
    if key not in _ops:
        a = mask_operand(rows, c, seed) if kind == "mask" else operand(kind, rows, c, seed)
        _ops[key] = bf16_round(a) if bf16 else a
    return _ops[key]


def operands(kind, c, rows):
    """Host operands of a case as float32 arrays.  x, residual, relu_mask: bf16 numbers (the rows of x no rule names are NaN);
    w: the layer's fp32 master weights [n_off, cin, cout] ([n_off, cout, cin] under W_TRANSPOSED: the same numbers, another
    reading), NOT rounded -- the pack rounds them; bias: fp32."""
    table, n_in, unnamed = table_of(c.n_off, rows)
    key = (kind, "x", c.n_off, rows, c.cin)
    if key not in _ops:
        x = _draw(kind, n_in, c.cin, 101).copy()
        x[unnamed] = np.nan
        _ops[key] = x
    wr = c.cout if c.flags & F_W_TRANSPOSED else c.cin
    wc = c.cin if c.flags & F_W_TRANSPOSED else c.cout
    ops = dict(x=_ops[key], w=_draw(kind, c.n_off * wr, wc, 102, bf16=False).reshape(c.n_off, wr, wc))
    if "bias" in c.operands:
        ops["bias"] = _draw(kind, 1, c.cout, 103, bf16=False)[0]
    if "residual" in c.operands:
        ops["residual"] = _draw(kind, rows, c.cout, 104)
    if "relu_mask" in c.operands:
        ops["relu_mask"] = _draw("mask" if kind == "exact" else kind, rows, c.cout, 105)
    return ops


def reference(kind, c, rows):
    """exact: (expected bits uint16, Y64);  gaussian: (Y64, E, zeroed or None, residual bits under RESIDUAL_LAST or None).
    Shared by every path that runs the same numbers, never changed."""
    key = (kind, c.cin, c.cout, c.n_off, rows, c.flagset)
    if key not in _refs:
        ops = operands(kind, c, rows)
        table = table_of(c.n_off, rows)[0]
        Y, S, N = conv(ops["x"], bf16_round(ops["w"]), table, ops.get("bias"), ops.get("residual"), ops.get("relu_mask"),
                       c.flags & (F_RELU_IN | F_W_TRANSPOSED | F_OFF_REVERSE | F_RESIDUAL_LAST))
        if kind == "exact":
            assert_exact(S)
            y32 = Y.astype(np.float32)
            assert np.array_equal(y32.astype(np.float64), Y)
            ref = (to_bf16_bits(y32), Y)
        else:
            zeroed = None if "relu_mask" not in ops else ~(ops["relu_mask"] > 0)
            res_last = "residual" in ops and bool(c.flags & F_RESIDUAL_LAST)
            ref = (Y, bound(N[:, None], S), zeroed, to_bf16_bits(ops["residual"]) if res_last and zeroed is not None else None)
        for a in ref:
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _refs[key] = ref
    return _refs[key]


# ------------------------------------------------------------------------------------------------------------------------
# The path report of the library (scn_conv_tiles_bf16_plan_describe: host only); L = sparse_rcnn_amd._lib
# ------------------------------------------------------------------------------------------------------------------------
FIELDS = ["stream", "ks", "nw", "n_wgb", "nb", "kh", "fused", "part", "n_kc", "n_chunks", "n_tg", "grid_x", "xbins", "vec_ok",
          "sum", "sum_v", "nt", "lds"]


def describe(L, n_in, cin, n_off, n_out, cout, flags, with_arrival, y_bits=0, s_bits=0):
    """(rc, dict over FIELDS).  y_bits: the low 4 bits of Y | residual | relu_mask; s_bits: of scratch | bias."""
    out = (C.c_int64 * 18)()
    rc = L.load().scn_conv_tiles_bf16_plan_describe(n_in, cin, n_off, n_out, cout, flags, int(bool(with_arrival)), y_bits, s_bits,
                                                    out)
    return rc, (dict(zip(FIELDS, [int(v) for v in out])) if rc == 0 else None)


# ------------------------------------------------------------------------------------------------------------------------
# Shapes: (cin, cout, variant) -> what follows from tb_shape; variant: "" the default, "kh2" under SCN_TB_KH=2, "nb2" / "nb4"
# under SCN_TB_NB.
#   nb: 16-column blocks per workgroup (ct = 16 nb columns);  kh: 32-channel planes per K-chunk;  n_kc / n_chunks: K-chunks of
#   32 kh channels / column chunks of ct;  part: cin no multiple of the K-chunk;  dead_plane: KH = 2 and the last K-chunk's second
#   plane is empty (cin % 64 <= 32);  dead_cols: columns of the last chunk past cout;  vec: cout % nb == 0 (the vector epilogue by
#   shape);  v4: cout % 4 == 0 (the K-chunk sum's width by shape);  ks: K-chunks of the stream kernel where the shape admits it
# ------------------------------------------------------------------------------------------------------------------------
def shape(nb, kh=1, n_kc=1, n_chunks=1, part=0, dead_plane=0, dead_cols=0, vec=1, v4=1, ks=0):
    return dict(nb=nb, kh=kh, n_kc=n_kc, n_chunks=n_chunks, part=part, dead_plane=dead_plane, dead_cols=dead_cols, vec=vec,
                v4=v4, ks=ks)


SHAPES = {
    # single K-chunk, NB = 2
    (32, 32, ""): shape(2),
    (8, 16, ""): shape(2, part=1, dead_cols=16),
    (24, 24, ""): shape(2, part=1, dead_cols=8),
    (32, 23, ""): shape(2, dead_cols=9, vec=0, v4=0),
    # single K-chunk, NB = 4
    (32, 64, ""): shape(4),
    (32, 37, ""): shape(4, dead_cols=27, vec=0, v4=0),
    (32, 96, ""): shape(4, n_chunks=2, dead_cols=32),                # half-dead last chunk
    (32, 70, ""): shape(4, n_chunks=2, dead_cols=58, vec=0, v4=0),
    # K split
    (64, 32, ""): shape(2, n_kc=2),
    (40, 24, ""): shape(2, n_kc=2, part=1, dead_cols=8),
    (48, 80, ""): shape(4, n_kc=2, n_chunks=2, part=1, dead_cols=48),
    (128, 64, ""): shape(4, n_kc=4, ks=4),
    (160, 32, ""): shape(2, n_kc=5),                                 # two R4 flush rounds, the last partial
    (64, 64, ""): shape(4, n_kc=2, ks=2),
    (64, 23, ""): shape(2, n_kc=2, dead_cols=9, vec=0, v4=0),        # sum V = 1 by shape
    (96, 64, ""): shape(4, n_kc=3),                                  # three K-chunks: no stream kernel
    (128, 128, ""): shape(4, n_kc=4, n_chunks=2, ks=4),
    (256, 64, ""): shape(4, n_kc=8, ks=8),
    (256, 128, ""): shape(4, n_kc=8, n_chunks=2, ks=8),
    (64, 96, ""): shape(4, n_kc=2, n_chunks=2, dead_cols=32, ks=2),  # dead half chunk
    (64, 70, ""): shape(4, n_kc=2, n_chunks=2, dead_cols=58, vec=0, v4=0, ks=2),
    # SCN_TB_KH=2 (NB = 2)
    (64, 64, "kh2"): shape(2, kh=2, n_chunks=2),                     # one 64-channel chunk
    (96, 32, "kh2"): shape(2, kh=2, n_kc=2, part=1, dead_plane=1),
    (72, 48, "kh2"): shape(2, kh=2, n_kc=2, n_chunks=2, part=1, dead_plane=1, dead_cols=16),
    (128, 32, "kh2"): shape(2, kh=2, n_kc=2),
    # SCN_TB_NB
    (32, 64, "nb2"): shape(2, n_chunks=2),
    (32, 16, "nb4"): shape(4, dead_cols=48),                         # three of the four column blocks are dead
}
VARIANT_SW = {"": {}, "kh2": {"SCN_TB_KH": "2"}, "nb2": {"SCN_TB_NB": "2"}, "nb4": {"SCN_TB_NB": "4"}}


def tb_shape(cin, cout, variant):
    """tb_shape of the library, restated: (nb, kh)."""
    kh = 2 if variant == "kh2" and cin > 32 else 1
    nb = {"nb2": 2, "nb4": 4}.get(variant, 4 if cout > 32 else 2)
    return (2 if kh == 2 else nb), kh


for (_ci, _co, _v), _s in SHAPES.items():                            # the table above, held to its own definitions
    _nb, _kh = tb_shape(_ci, _co, _v)
    _nkc, _nch = -(-_ci // (32 * _kh)), -(-_co // (16 * _nb))
    assert _ci % 8 == 0 and _s == shape(
        _nb, _kh, _nkc, _nch, int(_ci % (32 * _kh) != 0), int(_kh == 2 and 0 < _ci % 64 <= 32), _nch * 16 * _nb - _co,
        int(_co % _nb == 0), int(_co % 4 == 0),
        _nkc if (_kh == 1 and _nb == 4 and _ci % 32 == 0 and _nkc in (2, 4, 8)) else 0), (_ci, _co, _v)

STREAM0, STREAM1, BUDGET32, NO_XORDER = {"SCN_TB_STREAM": "0"}, {"SCN_TB_STREAM": "1"}, {"SCN_CU_BUDGET": "32"}, \
    {"SCN_TB_NO_XORDER": "1"}
OFFSETS = ("y", "residual", "relu_mask", "bias", "scratch")          # buffers a case may put off a 16-byte boundary
TABLES = ("small", "long", "xcd", "s4", "s8", "s8cap")


class Case:
    """One call.  variant: of SHAPES;  table: "small"; "long" (k_conv_tb under SCN_CU_BUDGET=32, ~4 tiles per wave); "xcd" (at
    least 8 workgroups per slice: the XCD-local hand-out); "s4" / "s8" (k_conv_tbs with 4- / 8-wave workgroups whose last batch
    has waves without a tile); "s8cap" (n_wgb capped: a workgroup walks two batches);  arrival: the call passes an arrival
    array;  split_sum: SCN_F_SPLIT_SUM;  off: {buffer: bytes past a 16-byte boundary};  xorder: SCN_F_TILE_ORDER_X;
    expect: the path, over fields of `describe`."""

    def __init__(self, group, cin, cout, n_off, flagset, variant="", table="small", arrival=True, split_sum=False, sw=None,
                 off=None, xorder=False):
        self.group, self.cin, self.cout, self.n_off, self.flagset, self.variant = group, cin, cout, n_off, flagset, variant
        self.table, self.arrival, self.split_sum, self.xorder = table, arrival, split_sum, xorder
        self.sw, self.off = {**VARIANT_SW[variant], **(sw or {})}, dict(off or {})
        assert table in TABLES and flagset in FLAGSETS and all(o in OFFSETS and b in (2, 4, 8) for o, b in self.off.items())
        assert not ("scratch" in self.off and arrival), "the fused form stores 16-byte pieces to the scratch"
        self.flags, self.operands = FLAGSETS[flagset]
        assert all(o in self.operands for o in self.off if o in ("bias", "residual", "relu_mask"))
        assert all(b % 4 == 0 for o, b in self.off.items() if o in ("bias", "scratch"))
        self.flags |= (F_SPLIT_SUM if split_sum else 0) | (F_TILE_ORDER_X if xorder else 0)
        self.gaussian = False                                        # set below: once per distinct expected path
        self.expect = self._expect()

    def ptr_bits(self):
        """(y_bits, s_bits) of the case's buffers (a missing operand is a NULL pointer: no bits)."""
        y = s = 0
        for o, b in self.off.items():
            if o in ("bias", "scratch"):
                s |= b
            else:
                y |= b
        return y, s

    def _expect(self):
        s = SHAPES[(self.cin, self.cout, self.variant)]
        y_bits, s_bits = self.ptr_bits()
        mode = self.sw.get("SCN_TB_STREAM")
        stream = int(bool(s["ks"]) and self.n_off in (27, 8) and not self.split_sum and mode != "0"
                     and (mode == "1" or (s["ks"] == 2 and self.n_off == 27)))
        vec_ok = int(s["vec"] and y_bits & (2 * s["nb"] - 1) == 0)
        e = dict(stream=stream, nb=s["nb"], kh=s["kh"], n_kc=s["n_kc"], n_chunks=s["n_chunks"], vec_ok=vec_ok)
        if stream:
            return dict(e, ks=s["ks"], nw=4 if self.table in ("small", "s4") else 8, fused=0, part=0, xbins=0, sum=0, sum_v=0)
        fused = int(s["n_kc"] > 1 and self.arrival and not self.split_sum)
        ksum = int(s["n_kc"] > 1 and not fused)
        slices = s["n_kc"] * s["n_chunks"]
        xbins = 8 // slices if (self.xorder and "SCN_TB_NO_XORDER" not in self.sw and slices in (1, 2, 4)) else 1
        return dict(e, ks=0, nw=0, n_wgb=0, fused=fused, part=s["part"], xbins=xbins, sum=ksum,
                    sum_v=(4 if s["v4"] and s_bits & 15 == 0 and y_bits & 7 == 0 else 1) if ksum else 0)

    def branch(self):
        return branches_of(self.expect, self.n_off)

    def id(self):
        sw = "".join("-" + k[4:].lower() + str(v) for k, v in sorted(self.sw.items()))
        mode = ("" if self.arrival else "-noarrival") + ("-splitsum" if self.split_sum else "") + ("-xorder" if self.xorder else "")
        off = "".join(f"-{o}off{b}" for o, b in sorted(self.off.items()))
        return f"{self.cin}x{self.cout}-o{self.n_off}-{self.table}-{self.flagset}{mode}{sw}{off}"


def branches_of(d, n_off):
    """A reported path -> the launcher branches it takes (keys of LAUNCH_BRANCHES_BF16)."""
    if d["stream"]:
        return {("tbs", d["ks"], n_off, d["nw"]), ("tbs-epilogue", "vec" if d["vec_ok"] else "elem")}
    b = {("tb", d["nb"], d["kh"], d["fused"], d["part"]), ("tb-epilogue", "vec" if d["vec_ok"] else "elem")}
    if d["sum"]:
        b.add(("sum", d["sum_v"]))
    return b


# every branch the launcher can take below 2^23 rows: 12 k_conv_tb and 12 k_conv_tbs instantiations, both k_conv_tb_sum widths,
# both epilogue forms of each of the two tile kernels
LAUNCH_BRANCHES_BF16 = ({("tb", nb, kh, fu, pt) for nb, kh in ((2, 1), (4, 1), (2, 2)) for fu in (0, 1) for pt in (0, 1)}
                        | {("tbs", ks, no, nw) for ks in (2, 4, 8) for no in (27, 8) for nw in (8, 4)}
                        | {("sum", 4), ("sum", 1)}
                        | {(k, e) for k in ("tb-epilogue", "tbs-epilogue") for e in ("vec", "elem")})
assert len(LAUNCH_BRANCHES_BF16) == 30

MODES = ((True, False), (False, False), (True, True))               # (arrival, split_sum): fused, arrival == NULL, SPLIT_SUM
EIGHT = ("fwd", "wt_only", "rev_only")                               # the 8-offset table: the pack's flags one at a time


def _build_cases():
    cases = []

    def add(group, cin, cout, n_off, fs, **kw):
        cases.append(Case(group, cin, cout, n_off, fs, **kw))

    # ---- single K-chunk: k_conv_tb<2 | 4, 1, false, PART>, no K reduction (the arrival array is not looked at)
    for group, shapes in (("single chunk NB2", ((32, 32), (8, 16), (24, 24), (32, 23))),
                          ("single chunk NB4", ((32, 64), (32, 37), (32, 96), (32, 70)))):
        for cin, cout in shapes:
            for fs in FOUR:
                add(group, cin, cout, 27, fs)
            add(group, cin, cout, 27, "bwd_res_last", arrival=False)
            for fs in EIGHT:
                add(group, cin, cout, 8, fs)
    # ---- K split on k_conv_tb: the three forms of the K reduction; long tables for the pipelined hand-off
    for cin, cout, sw in ((64, 32, {}), (40, 24, {}), (48, 80, {}), (128, 64, STREAM0), (160, 32, {}), (64, 23, {})):
        for arrival, split_sum in MODES:
            for fs in FOUR:
                add("K split", cin, cout, 27, fs, arrival=arrival, split_sum=split_sum, sw=sw)
    for arrival, split_sum in MODES:                                 # 8 offsets: the default is not the stream kernel
        for fs in EIGHT:
            add("K split", 64, 64, 8, fs, arrival=arrival, split_sum=split_sum)
    for cin, cout in ((64, 32), (40, 24), (48, 80), (160, 32)):
        for fs in ("fwd_relu_res", "bwd_res_last"):
            add("K split", cin, cout, 27, fs, table="long", sw=BUDGET32)
        add("K split", cin, cout, 27, "bwd", table="long", arrival=False, sw=BUDGET32)
    # ---- SCN_TB_KH=2: k_conv_tb<2, 2, *, *>
    for fs in FOUR:
        add("KH2", 64, 64, 27, fs, variant="kh2")
    add("KH2", 64, 64, 8, "wt_only", variant="kh2", arrival=False)
    for cin, cout in ((96, 32), (72, 48), (128, 32)):
        for arrival, split_sum in MODES:
            for fs in FOUR:
                add("KH2", cin, cout, 27, fs, variant="kh2", arrival=arrival, split_sum=split_sum)
    for cin, cout in ((96, 32), (128, 32)):
        for fs in ("fwd_relu_res", "bwd_res_last"):
            add("KH2", cin, cout, 27, fs, variant="kh2", table="long", sw=BUDGET32)
    # ---- SCN_TB_NB against the default
    for cin, cout, v in ((32, 64, "nb2"), (32, 16, "nb4")):
        for fs in FOUR:
            add("NB forced", cin, cout, 27, fs, variant=v)
        add("NB forced", cin, cout, 8, "wt_only", variant=v)
    # ---- the stream kernel k_conv_tbs<KS, 27 | 8, 4 | 8>
    for fs in FOUR:
        add("stream", 64, 64, 27, fs, table="s4")                    # by default
        add("stream", 64, 70, 27, fs, table="s4")                    # element epilogue
        add("stream", 128, 128, 27, fs, table="s4", sw=STREAM1)
        add("stream", 256, 64, 27, fs, table="s4", sw=STREAM1)
    add("stream", 64, 64, 27, "fwd", table="s4", arrival=False)      # the stream kernel needs no arrival array
    for fs in ("fwd_relu_res", "bwd_res_last"):
        add("stream", 64, 96, 27, fs, table="s8")                    # dead half chunk, 8-wave workgroups
        add("stream", 128, 128, 27, fs, table="s8cap", sw=STREAM1)   # n_wgb capped: two batches per workgroup
    add("stream", 256, 128, 27, "bwd_res_last", table="s8", sw=STREAM1)
    for cin, cout in ((64, 64), (128, 128), (256, 64)):
        for fs in EIGHT:
            add("stream", cin, cout, 8, fs, table="s4", sw=STREAM1)
    for cin, cout in ((64, 96), (128, 128), (256, 128)):
        add("stream", cin, cout, 8, "wt_only", table="s8", sw=STREAM1)
    add("stream", 64, 70, 8, "wt_only", table="s4", sw=STREAM1)
    # not taken: the two-launch form, three K-chunks, the narrow tile
    add("stream", 64, 64, 27, "fwd", split_sum=True)
    add("stream", 128, 128, 27, "bwd", split_sum=True, sw=STREAM1)
    for fs in ("fwd", "bwd"):
        add("stream", 96, 64, 27, fs, sw=STREAM1)
        add("stream", 64, 32, 27, fs, sw=STREAM1)
    # ---- alignment, one buffer at a time
    fs_of = {"y": "bwd", "residual": "bwd_res_last", "relu_mask": "bwd_res_last", "bias": "fwd_relu_res"}
    for o in ("y", "residual", "relu_mask"):
        for b in (2, 4):                                             # NB = 2: 2 bytes off breaks vec_ok, 4 keeps it
            add("alignment", 32, 32, 27, fs_of[o], off={o: b})
            for arrival, split_sum in MODES:
                add("alignment", 64, 32, 27, fs_of[o], arrival=arrival, split_sum=split_sum, off={o: b})
        for b in (4, 8):                                             # NB = 4: 4 bytes off breaks vec_ok, 8 keeps it
            add("alignment", 32, 64, 27, fs_of[o], off={o: b})
            for arrival, split_sum in MODES[:2]:
                add("alignment", 128, 64, 27, fs_of[o], arrival=arrival, split_sum=split_sum, sw=STREAM0, off={o: b})
            add("alignment", 64, 64, 27, fs_of[o], table="s4", off={o: b})                 # the stream kernel's epilogue
        add("alignment", 64, 64, 27, fs_of[o], table="s4", off={o: 2})
        add("alignment", 64, 64, 27, fs_of[o], variant="kh2", off={o: 2})
    for cin, cout, sw in ((64, 32, {}), (128, 64, STREAM0)):         # bias / scratch one float off: the sum one element a thread
        add("alignment", cin, cout, 27, "fwd_relu_res", arrival=False, sw=sw, off={"bias": 4})
        add("alignment", cin, cout, 27, "fwd_relu_res", sw=sw, off={"bias": 4})
        add("alignment", cin, cout, 27, "fwd_relu_res", arrival=False, sw=sw, off={"scratch": 4})
        add("alignment", cin, cout, 27, "bwd_res_last", arrival=False, sw=sw, off={"scratch": 8})
    add("alignment", 64, 64, 27, "fwd_relu_res", table="s4", off={"bias": 4})
    # ---- XCD-local hand-out: 1, 2, 4 slices -> xbins 8, 4, 2; 8 slices and SCN_TB_NO_XORDER -> 1
    for cin, cout, sw in ((32, 32, {}), (64, 32, {}), (128, 64, STREAM0), (128, 128, STREAM0), (64, 32, NO_XORDER)):
        for fs in ("fwd_relu_res", "bwd_res_last"):
            add("xcd order", cin, cout, 27, fs, table="xcd", sw=sw, xorder=True)
    add("xcd order", 32, 64, 27, "fwd", table="xcd", xorder=True)
    seen = set()
    for c in cases:                                                  # the gaussian kind: once per distinct expected path
        key = (tuple(sorted(c.expect.items())), c.table, c.n_off != 27)
        if key not in seen:
            seen.add(key)
            c.gaussian = True
    ids = [c.id() for c in cases]
    assert len(ids) == len(set(ids))
    return cases


CASES = _build_cases()
GROUPS = sorted({c.group for c in CASES})

_rows = {}


def table_rows(L, case):
    """Rows of the case's table, chosen from the path report under the case's switches (n_out % 16 != 0 everywhere):
      long   16 * 64 * n_tg + 5, n_tg = the workgroups per slice at any large row count: ~4 tiles per wave of k_conv_tb;
      xcd    4101: 257 tiles, 17 workgroups per slice (the hand-out by XCD needs 8);
      s4     the first table past the small one whose tile count is no multiple of 4 (4-wave workgroups);
      s8     the shortest table the launcher gives 8-wave workgroups (cdiv(nt, 8) * n_chunks >= 224), nt no multiple of 8;
      s8cap  the shortest such table whose n_wgb is capped below its batches: a workgroup walks two."""
    if case.table == "small":
        return small_rows(case.n_off)
    key = (case.table, case.cin, case.cout, case.n_off, tuple(sorted(case.sw.items())))
    if key in _rows:
        return _rows[key]
    rows_of = lambda nt: 16 * (nt - 1) + 5

    def rep(rows):
        rc, d = describe(L, N_IN_FACTOR[case.n_off] * rows, case.cin, case.n_off, rows, case.cout, case.flags, case.arrival,
                         *case.ptr_bits())
        assert rc == 0
        return d

    with switches(L, case.sw):
        if case.table == "long":
            assert case.sw.get("SCN_CU_BUDGET") == "32"
            rows = 16 * 64 * rep(MAX_ROWS)["n_tg"] + 5
        elif case.table == "xcd":
            rows = 4101
        elif case.table == "s4":
            nt = -(-small_rows(case.n_off) // 16) + 1
            while nt % 4 == 0 or rep(rows_of(nt))["nw"] != 4:
                nt += 1
            rows = rows_of(nt)
        else:
            nt = 1
            while True:
                d = rep(rows_of(nt))
                if nt % 8 != 0 and d["nw"] == 8 and (case.table == "s8" or d["n_wgb"] < -(-nt // 8)):
                    break
                nt += 1
            rows = rows_of(nt)
    assert small_rows(case.n_off) <= rows <= MAX_ROWS and rows % 16 != 0, (case.id(), rows)
    _rows[key] = rows
    return rows
