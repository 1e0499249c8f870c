"""Plain numpy / float64 restatement of the weight (and bias) gradient of every conv-type layer (csrc/scn_wgrad.hip), the
rule lists and operands the path tests run it on, and their case tables.  tests/test_wgrad_restate_cpu.py pins it against
torch; tests/test_gpu_wgrad_paths.py compares every launcher path of the HIP kernels with it.

    dW[o] = sum_{p in [prefix[o], prefix[o+1])} relu?(X[in_rows[p]])^T dY[out_rows[p]]
    db    = sum over the rules of the offsets named in db_mask of dY[out_rows[p]]
    S[o]  = the sum of dW[o] with absolute values taken term by term (the scale of its rounding-error bound)

Two operand kinds:
  exact     integers in [-3, 3] (a third zeros, half of the rest negative): every product and every partial sum of any subset
            of the terms is an integer below 2^24, so every fp32 summation order, and bf16 storage, gives the float64 bits;
  gaussian  standard normal (rounded to bf16 first for bf16-stored cases, so the restatement sees what the kernel reads),
            held to the bound of a sum of N rounded products in any order: gamma_{N+2} * S.
"""
import contextlib
import ctypes as C

import numpy as np

U32 = 2.0 ** -24                 # fp32 unit roundoff
EXACT_LIMIT = 2 ** 24            # integers below it are fp32 numbers
N_IN, N_OUT = 600, 500           # rows of X / dY in every rule-list case


def wgrad(X, dY, in_rows, out_rows, prefix, relu_in, db_mask):
    """(dW [n_off, cin, cout], db [cout], S [n_off, cin, cout]) in float64.  in_rows is None: the identity list."""
    X = np.asarray(X, dtype=np.float64)
    dY = np.asarray(dY, dtype=np.float64)
    prefix = [int(v) for v in prefix]
    n_off = len(prefix) - 1
    if relu_in:
        X = np.maximum(X, 0.0)
    dW = np.zeros((n_off, X.shape[1], dY.shape[1]))
    S = np.zeros_like(dW)
    db = np.zeros(dY.shape[1])
    for o in range(n_off):
        a, b = prefix[o], prefix[o + 1]
        if b <= a:
            continue
        if in_rows is None:
            xi, yo = X[a:b], dY[a:b]
        else:
            xi, yo = X[np.asarray(in_rows[a:b], dtype=np.int64)], dY[np.asarray(out_rows[a:b], dtype=np.int64)]
        dW[o] = xi.T @ yo
        S[o] = np.abs(xi).T @ np.abs(yo)
        if (int(db_mask) >> o) & 1:
            db += yo.sum(0)
    return dW, db, S


def db_abs(dY, out_rows, prefix, db_mask):
    """(S_db [cout], N_db): the term-by-term absolute sum of db and the number of rules it adds."""
    dY = np.abs(np.asarray(dY, dtype=np.float64))
    s, n = np.zeros(dY.shape[1]), 0
    for o in range(len(prefix) - 1):
        a, b = int(prefix[o]), int(prefix[o + 1])
        if b > a and (int(db_mask) >> o) & 1:
            s += (dY[a:b] if out_rows is None else dY[np.asarray(out_rows[a:b], dtype=np.int64)]).sum(0)
            n += b - a
    return s, n


def bound(n_terms, S):
    """|fl(sum of n rounded products, any order) - exact| <= gamma_{n+2} * S, gamma_k = k u / (1 - k u)."""
    g = (np.asarray(n_terms, dtype=np.float64) + 2.0) * U32
    return g * S / (1.0 - g)


def rule_list(counts, n_in=N_IN, n_out=N_OUT, seed=0, first=0, pool=None):
    """(in_rows int32, out_rows int32, prefix int64) with counts[o] rules for offset o, rows drawn WITH repeats (the weight
    gradient is defined for any list; Deconvolution rules repeat rows).  `first` unused leading entries (prefix[0] = first);
    pool: draw from that many distinct rows only (many repeats)."""
    rng = np.random.default_rng(1000 + seed)
    total = int(first + sum(counts))
    in_rows = rng.integers(0, pool or n_in, size=total).astype(np.int32)
    out_rows = rng.integers(0, pool or n_out, size=total).astype(np.int32)
    prefix = np.concatenate([[first], first + np.cumsum(np.asarray(counts, dtype=np.int64))]).astype(np.int64)
    return in_rows, out_rows, prefix


def to_bf16_bits(a):
    """float32 -> bf16 bit patterns (uint16), round to nearest even (finite inputs)."""
    u = np.ascontiguousarray(a, dtype=np.float32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def from_bf16_bits(b):
    return (np.asarray(b, dtype=np.uint16).astype(np.uint32) << 16).view(np.float32)


def operand(kind, rows, c, seed, bf16=False):
    """float32 [rows, c]; with bf16 every value is a bf16 number."""
    rng = np.random.default_rng(seed)
    if kind == "exact":
        mag = rng.integers(1, 4, size=(rows, c))
        sign = np.where(rng.random((rows, c)) < 0.5, -1, 1)
        return np.where(rng.random((rows, c)) < 1.0 / 3.0, 0, mag * sign).astype(np.float32)
    x = rng.standard_normal((rows, c)).astype(np.float32)
    return from_bf16_bits(to_bf16_bits(x)) if bf16 else x


def assert_exact(S, S_db=None):
    """The precondition of the exact kind: no partial sum of any subset of the terms can leave the integers of fp32."""
    assert float(S.max(initial=0.0)) < EXACT_LIMIT
    assert S_db is None or float(S_db.max(initial=0.0)) < EXACT_LIMIT


# ------------------------------------------------------------------------------------------------------------------------
# Rule lists of the path tests: name -> (counts, keyword arguments of rule_list, db_mask)
# ------------------------------------------------------------------------------------------------------------------------
# (a) 27 offsets, counts around the MFMA step (4), the wave block of rules (16 / 64), the unit granularities (16 / 32 / 64)
# and the unit floors (128 / 256 / 512); first and last offset empty, two empty offsets side by side (9, 10)
COUNTS_A = [0, 1, 3, 4, 5, 63, 64, 65, 127, 0, 0, 128, 129, 255, 256, 257, 511, 512, 513, 1025, 1, 5, 64, 3, 65, 4, 0]
COUNTS_32 = [0, 1, 3, 4, 5, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512] * 2
MASK_A = (1 << 0) | (1 << 13) | (1 << 19) | (1 << 20)          # an empty offset, the centre, the 1025-rule offset, one rule
LISTS = {
    "A": (COUNTS_A, {}, MASK_A),
    "A7": (COUNTS_A, {"first": 7}, MASK_A),                      # prefix_host[0] = 7 (single-problem calls only)
    "empty": ([0] * 27, {}, 1 << 13),                            # no rules at all: the memset path
    "one": ([777], {}, 1),
    "deconv8": ([300, 512, 1, 0, 64, 129, 700, 65], {"pool": 40}, 0xFF),     # every offset in db, rows repeat ~40 times
    "wide32": (COUNTS_32, {}, (1 << 31) | (1 << 15) | 2),
}
IDENT_ROWS = [1, 4, 500, 513]                                    # (e) the identity list: NULL row arrays, n_off = 1
assert len(COUNTS_A) == 27 and sum(COUNTS_A) < 6000 and sum(COUNTS_32) < 6000


def make_list(name):
    counts, kw, mask = LISTS[name]
    in_rows, out_rows, prefix = rule_list(counts, seed=sorted(LISTS).index(name), **kw)
    return in_rows, out_rows, prefix, mask


# ------------------------------------------------------------------------------------------------------------------------
# Shape table: (cin, cout, bf16 storage, switches, expected path).  Path = (kernel, ta, tb, quad, edge, evec, hb, V, nbi, nbj)
# as scn_wgrad_plan_describe reports it for 16-byte-aligned pointers; kernel "d" = k_wgrad_direct, "t" = k_wgrad_tb.
# ------------------------------------------------------------------------------------------------------------------------
def mk_path(kernel, ta, tb, quad=0, edge=0, evec=0, hb=0, V=4, nbi=1, nbj=1):
    return dict(kernel=kernel, ta=ta, tb=tb, quad=quad, edge=edge, evec=evec, hb=hb, V=V, nbi=nbi, nbj=nbj)


NO_T3, NO_EVEC, NO_TB = {"SCN_WD_NO_T3": "1"}, {"SCN_WD_NO_EVEC": "1"}, {"SCN_WGRAD_BF16_MFMA": "0"}
SHAPES = [
    # direct 2x2 whole / EVEC edge / element edge with the V = 1 sum
    (32, 32, False, {}, mk_path("d", 2, 2)),
    (16, 32, False, {}, mk_path("d", 2, 2, edge=1, evec=1)),
    (8, 24, False, {}, mk_path("d", 2, 2, edge=1, evec=1)),
    (5, 7, False, {}, mk_path("d", 2, 2, edge=1, V=1)),
    (1, 1, False, {}, mk_path("d", 2, 2, edge=1, V=1)),
    (33, 3, False, {}, mk_path("d", 4, 2, edge=1, V=1)),              # (Cin > 32: the 4 x 2 block, element edge)
    # direct 4x2 / 2x4 / 4x4
    (64, 32, False, {}, mk_path("d", 4, 2)),
    (32, 64, False, {}, mk_path("d", 2, 4)),
    (64, 64, False, {}, mk_path("d", 4, 4)),
    # QUAD whole (one block, two blocks), QUAD edge (vector pieces, element loads)
    (128, 128, False, {}, mk_path("d", 4, 4, quad=1)),
    (256, 128, False, {}, mk_path("d", 4, 4, quad=1, nbi=2)),
    (80, 112, False, {}, mk_path("d", 4, 4, quad=1, edge=1, evec=1)),
    (80, 112, False, NO_T3, mk_path("d", 4, 4, quad=1, edge=1, evec=1)),
    (130, 65, False, {}, mk_path("d", 4, 4, quad=1, edge=1, V=1, nbi=2)),
    # 48-wide wave blocks, and the padded blocks they replace
    (48, 48, False, {}, mk_path("d", 3, 3)),
    (96, 48, False, {}, mk_path("d", 3, 3, nbi=2)),
    (96, 96, False, {}, mk_path("d", 3, 3, nbi=2, nbj=2)),
    (48, 48, False, NO_T3, mk_path("d", 4, 4, edge=1, evec=1)),
    (96, 48, False, NO_T3, mk_path("d", 4, 4, edge=1, evec=1, nbi=2)),
    (96, 96, False, NO_T3, mk_path("d", 4, 4, quad=1, edge=1, evec=1)),
    # EDGE with vector row pieces against element loads
    (48, 80, False, {}, mk_path("d", 4, 4, edge=1, evec=1, nbj=2)),
    (48, 80, False, NO_EVEC, mk_path("d", 4, 4, edge=1, nbj=2)),
    (112, 112, False, {}, mk_path("d", 4, 4, quad=1, edge=1, evec=1)),
    (112, 112, False, NO_EVEC, mk_path("d", 4, 4, quad=1, edge=1)),
    # k_wgrad_tb: every (tiles_in, tiles_out)
    (8, 8, True, {}, mk_path("t", 1, 1)),
    (32, 64, True, {}, mk_path("t", 1, 2)),
    (32, 128, True, {}, mk_path("t", 1, 4)),
    (64, 32, True, {}, mk_path("t", 2, 1)),
    (64, 64, True, {}, mk_path("t", 2, 2)),
    (40, 24, True, {}, mk_path("t", 2, 1)),
    (64, 128, True, {}, mk_path("t", 2, 4)),
    (128, 32, True, {}, mk_path("t", 4, 1)),
    (128, 64, True, {}, mk_path("t", 4, 2)),
    (128, 128, True, {}, mk_path("t", 4, 4)),
    (72, 200, True, {}, mk_path("t", 4, 4, nbj=2)),
    # bf16 rows on the fp32-MFMA kernel (HB)
    (23, 7, True, {}, mk_path("d", 2, 2, edge=1, hb=1, V=1)),
    (12, 20, True, {}, mk_path("d", 2, 2, edge=1, hb=1)),
    (64, 64, True, NO_TB, mk_path("d", 4, 4, hb=1)),
    (48, 48, True, NO_TB, mk_path("d", 4, 4, edge=1, hb=1)),          # (no 48-wide blocks for bf16 rows)
]
# one shape per kernel family runs every rule list, with and without the input ReLU
FAMILIES = [(32, 32, False, {}), (64, 64, False, {}), (128, 128, False, {}), (48, 48, False, {}), (5, 7, False, {}),
            (80, 112, False, {}), (64, 64, True, {}), (12, 20, True, {}), (64, 64, True, NO_TB)]
# unit plans of list (b): switch values, and the units the 1025-rule offset is cut into at SCN_WGRAD_SPLITS = 4096, where
# `per` sits on its floor (512 rules: k_wgrad_direct in K mode; 128: QUAD; 256: k_wgrad_tb)
PLANS = [{}, {"SCN_WGRAD_SPLITS": "1"}, {"SCN_WGRAD_SPLITS": "5"}, {"SCN_WGRAD_SPLITS": "4096"}, {"SCN_CU_BUDGET": "32"}]


def floor_per(path):
    return 256 if path["kernel"] == "t" else (128 if path["quad"] else 512)


def shape_id(s):
    cin, cout, bf16, sw = s[:4]
    return f"{cin}x{cout}-{'bf16' if bf16 else 'fp32'}" + "".join("-" + k[4:].lower() + v for k, v in sorted(sw.items()))


def family(path):
    """Kernel family of a reported path (the summary's grouping of the error ratios)."""
    if path["kernel"] == "t":
        return "k_wgrad_tb"
    name = "quad" if path["quad"] else ("t3" if path["ta"] == 3 else f"{path['ta']}x{path['tb']}")
    return "k_wgrad_direct " + name + (" edge" if path["edge"] else "") + (" hb" if path["hb"] else "")


# ------------------------------------------------------------------------------------------------------------------------
# The path report of the library (scn_wgrad_plan_describe: host only) and its developer switches; L = sparse_rcnn_amd._lib
# ------------------------------------------------------------------------------------------------------------------------
def describe(L, cin, cout, prefix, n_prob, bf16, ptr_bits, out_bits):
    lib = L.load()
    ph = (C.c_int64 * len(prefix))(*[int(v) for v in prefix])
    out = (C.c_int64 * 16)()
    rc = lib.scn_wgrad_plan_describe(cin, cout, ph, len(prefix) - 1, n_prob, int(bf16), ptr_bits, out_bits, out)
    if rc != 0:
        return rc, None
    keys = ["kernel", "ta", "tb", "quad", "edge", "evec", "hb", "per", "units", "nbi", "nbj", "V", "G", "bytes", "bytes_db",
            "memset"]
    d = dict(zip(keys, [int(v) for v in out]))
    d["kernel"] = "t" if d["kernel"] else "d"
    return 0, d


@contextlib.contextmanager
def switches(L, sw):
    with contextlib.ExitStack() as st:
        for k, v in sw.items():
            st.enter_context(L.debug_switch(k, v))
        yield
