"""Plain numpy / float64 restatement of the fp32 tile convolution (csrc/scn_conv_ts.hip: scn_conv_tiles, scn_conv_tiles_finish,
the opt-in stream kernel of scn_conv_tss.hip), the synthetic rule tables and operands the path tests run it on, and their case
table.  tests/test_conv_restate_cpu.py pins it against torch and holds every case to the path scn_conv_tiles_plan_describe
reports; tests/test_gpu_conv_paths.py compares every launcher path of the HIP kernels with it.

    Y[r]    = epi( bias + sum_{o: table[o][r] >= 0} in(X[table[o][r]]) . Wo(o), residual[r], relu_mask[r] )
    S[r][n] = the same sum with the absolute value of every term (|bias| and |residual| among them)
    N[r]    = number of terms (cin products per rule, one per epilogue addend)

    in = ReLU under SCN_F_RELU_IN;  Wo(o) = W[o'], o' = n_off-1-o under SCN_F_OFF_REVERSE, used transposed under
    SCN_F_W_TRANSPOSED;  epi adds the residual, then zeroes where !(mask > 0) -- under SCN_F_RESIDUAL_LAST it zeroes first.

Two operand kinds (those of wgrad_restate.py):
  exact     integers in [-3, 3] (mask values from {-2, -0.0, 0.0, 1, 3}): S <= 27 * 160 * 9 + 6 < 2^24, so every summation
            order -- the four-wave shares, the K-chunk slabs -- gives the float64 bits;
  gaussian  standard normal, every element held to gamma_{N+2} S: the bound of a sum of N rounded products in ANY order.
No project import: the library handle (sparse_rcnn_amd._lib) is passed in where the path report is asked for.
"""
import contextlib
import ctypes as C

import numpy as np

from wgrad_restate import EXACT_LIMIT, U32, bound, operand          # noqa: F401  (re-exported: one bound, one operand recipe)

F_RELU_IN, F_W_TRANSPOSED, F_OFF_REVERSE, F_RESIDUAL_LAST, F_SPLIT_SUM = 1, 2, 4, 8, 16
MASK_VALUES = np.array([-2.0, -0.0, 0.0, 1.0, 3.0], dtype=np.float32)
MAX_ROWS = 40000                 # no table of this file is longer


def conv(X, W, table, bias, residual, relu_mask, flags):
    """(Y, S [n_out, cout], N [n_out]) in float64.  W is [n_off, cin, cout], or [n_off, cout, cin] under SCN_F_W_TRANSPOSED."""
    X = np.asarray(X, dtype=np.float64)
    W = np.asarray(W, dtype=np.float64)
    table = np.asarray(table)
    n_off, n_out = table.shape
    if flags & F_RELU_IN:
        X = np.maximum(X, 0.0)
    cout = W.shape[1] if flags & F_W_TRANSPOSED else W.shape[2]
    Y = np.zeros((n_out, cout))
    S = np.zeros((n_out, cout))
    N = np.zeros(n_out, dtype=np.int64)
    if bias is not None:
        Y += np.asarray(bias, dtype=np.float64)[None, :]
        S += np.abs(np.asarray(bias, dtype=np.float64))[None, :]
        N += 1
    for o in range(n_off):
        Wo = W[n_off - 1 - o] if flags & F_OFF_REVERSE else W[o]
        if flags & F_W_TRANSPOSED:
            Wo = Wo.T
        rows = np.nonzero(table[o] >= 0)[0]
        if len(rows):
            xg = X[table[o][rows].astype(np.int64)]
            Y[rows] += xg @ Wo
            S[rows] += np.abs(xg) @ np.abs(Wo)
            N[rows] += X.shape[1]
    res = None if residual is None else np.asarray(residual, dtype=np.float64)
    if res is not None:
        S += np.abs(res)
        N += 1
        if not flags & F_RESIDUAL_LAST:
            Y += res
    if relu_mask is not None:
        Y = np.where(np.asarray(relu_mask) > 0, Y, 0.0)
    if res is not None and flags & F_RESIDUAL_LAST:
        Y += res
    return Y, S, N


def mask_operand(rows, c, seed):
    return MASK_VALUES[np.random.default_rng(seed).integers(0, len(MASK_VALUES), size=(rows, c))]


def assert_exact(S):
    """The precondition of the exact kind: no partial sum of any subset of the terms can leave the integers of fp32."""
    assert float(S.max(initial=0.0)) < EXACT_LIMIT


# ------------------------------------------------------------------------------------------------------------------------
# Synthetic rule tables: int32 [n_off][n_out], -1 = no rule
# ------------------------------------------------------------------------------------------------------------------------
GROUP_COUNTS = [1, 2, 3, 4, 5, 6, 7, 8, 9, 13, 26, 27]   # offset counts that get a block of rows with ONE shared mask
GROUP_ROWS = 32                  # rows per block: a run of >= 31 rows with one mask holds a whole tile wherever the sort puts it
N_RANDOM, N_RAGGED = 500, 5
N_IN_FACTOR = {27: 1, 8: 3, 12: 2, 1: 1}                 # SubM 3^3; a Convolution child table; a 2x2x3 stride; one offset


def group_counts(n_off):
    return [p for p in GROUP_COUNTS if p <= n_off]


def small_rows(n_off):
    return GROUP_ROWS * len(group_counts(n_off)) + N_RANDOM + N_RAGGED


def rule_table(n_off, n_out=None, seed=0):
    """(table, n_in).  For every offset count p of GROUP_COUNTS 32 rows share one mask of p bits (the mask sort keeps them
    together: at least one tile has exactly that mask); the other rows draw every bit with probability 1/2; with 27 offsets the
    centre bit is always set.  Entries are random input rows (repeats allowed; every fifth row is left out, see unnamed_rows);
    row 0 and row n_in - 1 occur in the first and in the last offset.  The rows are shuffled, and n_out is no multiple of 16 (a
    ragged last tile)."""
    n_out = small_rows(n_off) if n_out is None else int(n_out)
    assert small_rows(n_off) <= n_out <= MAX_ROWS and n_out % 16 != 0
    rng = np.random.default_rng(7000 + 100 * n_off + seed)
    n_in = N_IN_FACTOR[n_off] * n_out
    bits = rng.random((n_out, n_off)) < 0.5
    r = 0
    for p in group_counts(n_off):
        on = np.zeros(n_off, dtype=bool)
        pool = [o for o in range(n_off) if not (n_off == 27 and o == 13)]
        k = p - 1 if n_off == 27 else p
        on[rng.choice(pool, size=k, replace=False)] = True
        if n_off == 27:
            on[13] = True
        assert int(on.sum()) == p
        bits[r:r + GROUP_ROWS] = on[None, :]
        r += GROUP_ROWS
    if n_off == 27:
        bits[:, 13] = True
    bits = bits[rng.permutation(n_out)]
    pool = np.nonzero(np.arange(n_in) % 5 != 3)[0]                   # a fifth of the input rows is named by no rule
    table = np.where(bits.T, pool[rng.integers(0, len(pool), size=(n_off, n_out))], -1).astype(np.int32)
    for o in (0, n_off - 1):                                         # the two ends of X, in the first and in the last offset
        have = np.nonzero(table[o] >= 0)[0]
        assert len(have) >= 2
        table[o][have[0]] = 0
        table[o][have[-1]] = n_in - 1
    return table, n_in


def unnamed_rows(table, n_in):
    """Input rows no rule names.  The path tests fill them with NaN: the convolution never reads them, so a gather that runs past
    the channels of the row before (a K tail multiplied by the zero weights of the padding: NaN . 0) or takes a wrong row shows."""
    return np.setdiff1d(np.arange(n_in), table[table >= 0])


def check_tiles(table, perm, tstab, tile_mask, tile_order):
    """The tile structures of a table (metadata.build_tiles / scn_tiles_build), as numpy arrays, against the table itself."""
    n_off, n_out = table.shape
    nt = (n_out + 15) // 16
    assert perm.shape == (nt * 16,) and tstab.shape == (nt, n_off, 16) and tile_mask.shape == (nt,)
    assert np.array_equal(np.sort(perm[perm >= 0]), np.arange(n_out)) and int((perm == -1).sum()) == nt * 16 - n_out
    assert int(perm.min()) >= -1
    padded = np.concatenate([table, np.full((n_off, 1), -1, dtype=np.int32)], axis=1)      # perm -1 -> a row without rules
    want = padded[:, perm].reshape(n_off, nt, 16).transpose(1, 0, 2)
    assert np.array_equal(tstab, want)
    row_mask = ((want >= 0).astype(np.uint32) << np.arange(n_off, dtype=np.uint32)[None, :, None]).sum(axis=1, dtype=np.uint32)
    assert np.array_equal(tile_mask.view(np.uint32), np.bitwise_or.reduce(row_mask, axis=1))
    assert np.array_equal(np.sort(tile_order[:nt]), np.arange(nt))
    pop = np.array([bin(int(m)).count("1") for m in tile_mask.view(np.uint32)])
    assert set(group_counts(n_off)) - {13, 26} <= set(pop.tolist()), sorted(set(pop.tolist()))
    assert np.all(np.diff(pop[tile_order[:nt]]) <= 0)               # hand-out order: offset count descending
    return pop


# ------------------------------------------------------------------------------------------------------------------------
# The path report of the library (scn_conv_tiles_plan_describe: host only) and its developer switches; L = sparse_rcnn_amd._lib
# ------------------------------------------------------------------------------------------------------------------------
FIELDS = ["stream", "fullk", "wt", "vecn", "part", "tail", "k_tail", "n_tail", "fused", "split4", "prog_g0", "n_kc", "n_chunks",
          "n_tg", "grid_x", "finish_v4"]


def describe(L, n_in, cin, n_off, n_out, cout, flags, with_arrival, x_bits=0, w_bits=0, epi_bits=0):
    """(rc, dict over FIELDS).  x_bits / w_bits: the low 4 bits of the X / W pointer."""
    out = (C.c_int64 * 16)()
    rc = L.load().scn_conv_tiles_plan_describe(n_in, cin, n_off, n_out, cout, flags, int(bool(with_arrival)),
                                               ((x_bits | w_bits) & 15) | ((w_bits & 15) << 4), epi_bits, out)
    return rc, (dict(zip(FIELDS, [int(v) for v in out])) if rc == 0 else None)


@contextlib.contextmanager
def switches(L, sw):
    with contextlib.ExitStack() as st:
        for k, v in sw.items():
            st.enter_context(L.debug_switch(k, v))
        yield


# ------------------------------------------------------------------------------------------------------------------------
# Flag and epilogue sets
# ------------------------------------------------------------------------------------------------------------------------
BWD = F_W_TRANSPOSED | F_OFF_REVERSE
FLAGSETS = {
    "fwd": (0, ("bias",)),
    "fwd_relu_res": (F_RELU_IN, ("bias", "residual")),
    "bwd": (BWD, ("relu_mask",)),
    "bwd_res_last": (BWD | F_RESIDUAL_LAST, ("relu_mask", "residual")),
    "wt_only": (F_W_TRANSPOSED, ("relu_mask", "residual")),         # Deconvolution backward-data (child tables)
    "rev_only": (F_OFF_REVERSE, ("bias",)),
}
FOUR = ("fwd", "fwd_relu_res", "bwd", "bwd_res_last")

# ------------------------------------------------------------------------------------------------------------------------
# Shapes: (cin, cout) -> what follows from the channel counts alone, for 16-byte-aligned pointers and small row counts.
#   fullk: cin % 4 == 0;  vecn: cout % 4 == 0;  part: cin % 32 != 0;  k_tail / n_tail: 1 ... 16 channels / columns in the last
#   K-chunk / column chunk;  n_kc, n_chunks: chunks of 32
# ------------------------------------------------------------------------------------------------------------------------
def shape(fullk=1, vecn=1, part=0, k_tail=0, n_tail=0, n_kc=1, n_chunks=1):
    return dict(fullk=fullk, vecn=vecn, part=part, k_tail=k_tail, n_tail=n_tail, n_kc=n_kc, n_chunks=n_chunks)


SHAPES = {
    # fullk, one K-chunk
    (32, 32): shape(),
    (4, 4): shape(part=1, k_tail=1, n_tail=1),                       # only the "both" slice class exists
    (16, 16): shape(part=1, k_tail=1, n_tail=1),
    (8, 32): shape(part=1, k_tail=1),
    (12, 32): shape(part=1, k_tail=1),                               # (a K tail of 12 channels; 4 and 8 above)
    (20, 36): shape(part=1, n_tail=1, n_chunks=2),                   # PART without a K tail
    (32, 23): shape(vecn=0),
    (32, 35): shape(vecn=0, n_tail=1, n_chunks=2),
    # fullk, K split over workgroups
    (48, 35): shape(vecn=0, part=1, k_tail=1, n_tail=1, n_kc=2, n_chunks=2),
    (64, 64): shape(n_kc=2, n_chunks=2),
    (128, 64): shape(n_kc=4, n_chunks=2),
    (128, 96): shape(n_kc=4, n_chunks=3),
    (160, 32): shape(n_kc=5),                                        # the combiner's second pass of four K-chunks
    (48, 48): shape(part=1, k_tail=1, n_tail=1, n_kc=2, n_chunks=2),  # all four slice classes
    (80, 112): shape(part=1, k_tail=1, n_tail=1, n_kc=3, n_chunks=4),
    (40, 24): shape(part=1, k_tail=1, n_kc=2),
    (64, 23): shape(vecn=0, n_kc=2),
    (64, 40): shape(n_tail=1, n_kc=2, n_chunks=2),                   # TAIL without PART
    (64, 35): shape(vecn=0, n_tail=1, n_kc=2, n_chunks=2),           # TAIL without PART, element staging
    # the general kernel: cin % 4 != 0
    (7, 32): shape(fullk=0, part=1, k_tail=1),
    (7, 16): shape(fullk=0, part=1, k_tail=1, n_tail=1),
    (3, 5): shape(fullk=0, vecn=0, part=1, k_tail=1, n_tail=1),
    (23, 32): shape(fullk=0, part=1),
    (33, 32): shape(fullk=0, part=1, k_tail=1, n_kc=2),
    (70, 64): shape(fullk=0, part=1, k_tail=1, n_kc=3, n_chunks=2),
}
for (_ci, _co), _s in SHAPES.items():                                # the table above, held to its own definitions
    assert _s == shape(int(_ci % 4 == 0), int(_co % 4 == 0), int(_ci % 32 != 0), int(0 < _ci % 32 <= 16),
                       int(0 < _co % 32 <= 16), -(-_ci // 32), -(-_co // 32)), (_ci, _co)

NO_SPLIT, BUDGET32, NO_TAIL, STREAM = {"SCN_TS_SPLIT": "0"}, {"SCN_CU_BUDGET": "32"}, {"SCN_TS_NO_TAIL": "1"}, {"SCN_TS_STREAM": "1"}
OFFSETS = ("x", "w", "y", "bias", "residual", "relu_mask", "scratch")     # buffers a case may put 4 bytes past a 16-byte boundary


class Case:
    """One call.  table: "small", "long" (the plain loop with ~4 tiles per wave) or "long4" (the four-waves-per-tile loop over >= 3
    rounds); arrival: the call passes an arrival array; split_sum: SCN_F_SPLIT_SUM + scn_conv_tiles_finish; off: buffers one
    float past a 16-byte boundary; expect: the path, over the fields of `describe`."""

    def __init__(self, group, cin, cout, n_off, flagset, table="small", arrival=True, split_sum=False, sw=None, off=()):
        self.group, self.cin, self.cout, self.n_off, self.flagset, self.table = group, cin, cout, n_off, flagset, table
        self.arrival, self.split_sum, self.sw, self.off = arrival, split_sum, dict(sw or {}), tuple(off)
        assert all(o in OFFSETS for o in self.off) and flagset in FLAGSETS
        assert not ("scratch" in self.off and arrival), "the fused form stores 16-byte pieces to the scratch"
        self.flags, self.operands = FLAGSETS[flagset]
        assert all(o in self.operands for o in self.off if o in ("bias", "residual", "relu_mask"))
        if split_sum:
            self.flags |= F_SPLIT_SUM
        self.gaussian = False                                        # set below: once per distinct expected path
        self.expect = self._expect()

    def _expect(self):
        s = SHAPES[(self.cin, self.cout)]
        x_off, w_off = "x" in self.off, "w" in self.off
        fullk = int(s["fullk"] and not x_off and not w_off)
        vecn = int(s["vecn"] and not w_off)
        wt = int(bool(self.flags & F_W_TRANSPOSED))
        tail = int(fullk and (s["k_tail"] or s["n_tail"]) and "SCN_TS_NO_TAIL" not in self.sw)
        fused = int(s["n_kc"] > 1 and self.arrival and not self.split_sum)
        # the four-waves-per-tile loop: the fast path's, for up to 2048 (tile, slice) pairs -- every table of this file
        # but the plain-loop long ones, which run under SCN_TS_SPLIT=0
        split4 = int(fullk and self.sw.get("SCN_TS_SPLIT") != "0")
        prog = 0
        if fullk and not wt and vecn and not s["part"] and not tail and not split4 and self.n_off == 27 and self.cout % 32 == 0:
            prog = int(self.sw.get("SCN_TS_PROG", 0))
        stream = int(self.sw.get("SCN_TS_STREAM") == "1" and self.arrival and not self.split_sum and fullk
                     and self.cin in (64, 128) and self.cout % 64 == 0 and self.n_off in (27, 8))
        epi_off = any(o in self.off for o in ("y", "bias", "residual", "relu_mask", "scratch"))
        return dict(stream=stream, fullk=fullk, wt=wt, vecn=vecn, part=s["part"], tail=tail, k_tail=s["k_tail"],
                    n_tail=s["n_tail"], fused=fused, split4=split4, prog_g0=prog, n_kc=s["n_kc"], n_chunks=s["n_chunks"],
                    finish_v4=int(self.cout % 4 == 0 and not epi_off))

    def ptr_bits(self):
        """(x_bits, w_bits, epi_bits) of the case's buffers (a missing operand is a NULL pointer: no bits)."""
        epi = any(o not in ("x", "w") for o in self.off)
        return (4 if "x" in self.off else 0), (4 if "w" in self.off else 0), (4 if epi else 0)

    def branch(self):
        """The k_conv_ts instantiation family the case launches: a key of LAUNCH_BRANCHES (None: the stream kernel)."""
        return branch_of(self.expect)

    def id(self):
        sw = "".join("-" + k[4:].lower() + str(v) for k, v in sorted(self.sw.items()))
        mode = ("" if self.arrival else "-noarrival") + ("-splitsum" if self.split_sum else "")
        off = "".join("-" + o + "off" for o in self.off)
        return f"{self.cin}x{self.cout}-o{self.n_off}-{self.table}-{self.flagset}{mode}{sw}{off}"


def branch_of(d):
    """A reported path -> the launcher branch it takes.  k_conv_ts<WT, VEC, VECN, FULLK, PART, FUSED, TAIL, SPLIT>: with WT
    the staging never looks at VECN (the three `!vecn && wt` combinations are folded into the WT instantiations), the general
    kernel has neither PART nor TAIL nor the four-wave loop."""
    if d["stream"]:
        return None
    stage = "wt" if d["wt"] else ("vecn" if d["vecn"] else "elem")
    if not d["fullk"]:
        return ("general", stage, 0, 0, d["fused"], 0)
    return ("fullk", stage, d["part"], d["tail"], d["fused"], d["split4"])


# every branch the launcher can take for cin <= 160 (row counts below 2^23): 3 stagings x PART x TAIL x FUSED x SPLIT on the
# fast path, 3 stagings x FUSED on the general kernel
LAUNCH_BRANCHES = {("fullk", st, pt, tl, fu, sp) for st in ("wt", "vecn", "elem") for pt in (0, 1) for tl in (0, 1)
                   for fu in (0, 1) for sp in (0, 1)} | {("general", st, 0, 0, fu, 0) for st in ("wt", "vecn", "elem") for fu in (0, 1)}
assert len(LAUNCH_BRANCHES) == 54


def _modes(cin, cout, long_tables):
    """The loops and K-reduction forms a shape runs in: (table, arrival, split_sum, switches)."""
    s = SHAPES[(cin, cout)]
    ksplit, tails = s["n_kc"] > 1, s["fullk"] and (s["k_tail"] or s["n_tail"])
    m = [("small", True, False, {}), ("small", True, False, NO_SPLIT)]
    if ksplit:
        m += [("small", False, False, {}), ("small", True, True, {}), ("small", False, False, NO_SPLIT)]
    if long_tables:
        m += [("long", True, False, {**BUDGET32, **NO_SPLIT})]
        if s["fullk"]:
            m += [("long4", True, False, BUDGET32)]
        if ksplit:
            m += [("long", False, False, {**BUDGET32, **NO_SPLIT})]
    if tails:
        m += [("small", True, False, NO_TAIL), ("small", True, False, {**NO_TAIL, **NO_SPLIT})]
        if ksplit:
            m += [("small", False, False, NO_TAIL), ("small", False, False, {**NO_TAIL, **NO_SPLIT})]
    return m


def _build_cases():
    cases = []
    single = [(32, 32), (4, 4), (16, 16), (8, 32), (12, 32), (20, 36), (32, 23), (32, 35)]
    ksplit = [(48, 35), (64, 64), (128, 96), (160, 32), (48, 48), (80, 112), (40, 24), (64, 23), (64, 40), (64, 35)]
    general = [(7, 32), (7, 16), (3, 5), (23, 32), (33, 32), (70, 64)]
    for group, shapes in (("fullk single chunk", single), ("fullk K-split", ksplit), ("general kernel", general)):
        for cin, cout in shapes:
            long_tables = group == "fullk K-split" or (cin, cout) in ((32, 32), (7, 32), (33, 32))
            for table, arrival, split_sum, sw in _modes(cin, cout, long_tables):
                for fs in FOUR:
                    cases.append(Case(group, cin, cout, 27, fs, table, arrival, split_sum, sw))
    # other offset counts: a Convolution child table forward and as Deconvolution backward-data, a 2x2x3 stride, one offset
    for cin, cout in ((32, 32), (64, 64), (48, 48), (20, 36), (7, 16)):
        for sw in ({}, NO_SPLIT) + (({**NO_TAIL, **NO_SPLIT},) if (cin, cout) == (48, 48) else ()):
            for fs in ("fwd", "wt_only"):
                cases.append(Case("offset counts", cin, cout, 8, fs, sw=sw))
            for n_off in (12, 1):
                for fs in ("fwd_relu_res", "bwd_res_last"):
                    cases.append(Case("offset counts", cin, cout, n_off, fs, sw=sw))
    cases.append(Case("offset counts", 32, 32, 27, "rev_only"))
    cases.append(Case("offset counts", 64, 64, 27, "rev_only", sw=NO_SPLIT))
    # general by alignment: X one float off (the weight staging keeps its 16-byte reads), W one float off
    for cin, cout in ((32, 32), (64, 64)):
        for off in (("x",), ("w",)):
            for fs in FOUR:
                cases.append(Case("general by alignment", cin, cout, 27, fs, off=off))
            if cin == 64:
                cases.append(Case("general by alignment", cin, cout, 27, "fwd", arrival=False, off=off))
                cases.append(Case("general by alignment", cin, cout, 27, "bwd", table="long", sw={**BUDGET32, **NO_SPLIT}, off=off))
    # epilogue alignment: one buffer at a time (the K-chunk sum one element per thread; the tile kernel stores by element)
    for off in ("y", "bias", "residual", "relu_mask"):
        fs = {"y": "bwd", "bias": "fwd_relu_res", "residual": "bwd_res_last", "relu_mask": "bwd_res_last"}[off]
        cases.append(Case("epilogue alignment", 64, 64, 27, fs, arrival=False, off=(off,)))
        cases.append(Case("epilogue alignment", 64, 64, 27, fs, split_sum=True, off=(off,)))
        cases.append(Case("epilogue alignment", 64, 64, 27, fs, off=(off,)))               # fused: element stores
        cases.append(Case("epilogue alignment", 32, 32, 27, fs, off=(off,)))
        cases.append(Case("epilogue alignment", 32, 32, 27, fs, sw=NO_SPLIT, off=(off,)))
    # scratch alignment: only without an arrival array
    for fs in FOUR:
        cases.append(Case("scratch alignment", 64, 64, 27, fs, arrival=False, off=("scratch",)))
    cases.append(Case("scratch alignment", 64, 64, 27, "fwd", arrival=False, sw=NO_SPLIT, off=("scratch",)))
    # progressive staging of the forward slice
    for cin, cout in ((32, 32), (64, 64)):
        for g0 in (4, 8, 12):
            sw = {**NO_SPLIT, "SCN_TS_PROG": str(g0)}
            for fs in ("fwd", "fwd_relu_res"):
                cases.append(Case("progressive staging", cin, cout, 27, fs, sw=sw))
                cases.append(Case("progressive staging", cin, cout, 27, fs, table="long", sw={**sw, **BUDGET32}))
            cases.append(Case("progressive staging", cin, cout, 27, "bwd", sw=sw))         # transposed weights: classic staging
    # the opt-in stream kernel
    for cin, cout in ((64, 64), (128, 64)):
        for fs in FOUR:
            cases.append(Case("stream", cin, cout, 27, fs, sw=STREAM))
        for fs in ("fwd", "wt_only"):
            cases.append(Case("stream", cin, cout, 8, fs, sw=STREAM))
        cases.append(Case("stream", cin, cout, 27, "fwd", split_sum=True, sw=STREAM))      # not taken: k_conv_ts + finish
        cases.append(Case("stream", cin, cout, 27, "bwd", arrival=False, sw=STREAM))       # not taken: no arrival array
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


def table_rows(L, case):
    """Rows of the case's table.  long: 16 * 64 * n_tg_max + 5, n_tg_max = the workgroups per slice the path report names for
    the case under its switches (SCN_CU_BUDGET=32) at any large row count -- four tiles per wave of the plain loop on average;
    long4: at least 16 * 12 * n_tg_max + 5 -- three rounds of the four-waves-per-tile loop."""
    if case.table == "small":
        return small_rows(case.n_off)
    assert case.n_off == 27 and case.sw.get("SCN_CU_BUDGET") == "32"
    x, w, e = case.ptr_bits()
    with switches(L, case.sw):
        # (long4: the longest table that still takes the four-waves-per-tile loop, 2048 (tile, slice) pairs)
        probe = 2048 // (case.expect["n_kc"] * case.expect["n_chunks"]) * 16 if case.table == "long4" else MAX_ROWS
        rc, d = describe(L, probe, case.cin, 27, probe, case.cout, case.flags, case.arrival, x, w, e)
    assert rc == 0 and d["split4"] == case.expect["split4"]
    per_wg = 64 if case.table == "long" else 12
    rows = max(16 * per_wg * d["n_tg"] + 5, small_rows(27))
    assert rows < MAX_ROWS and rows % 16 != 0
    return rows
