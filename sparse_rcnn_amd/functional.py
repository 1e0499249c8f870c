"""Autograd functions of the sparse operator set, each a thin host wrapper over the C ABI.

Forward / backward definitions follow SURVEY.md Appendix B; each function names the reference call site it serves.
No function here falls back to PyTorch arithmetic: feature math runs in libscn_mi355x kernels only.

The convolution-type nodes (SubmanifoldConvolution, Convolution, Deconvolution, NetworkInNetwork and its joined form, the residual
unit) differ in their forward and backward-data kernels; what they do for their parameters is one decision, held once in
`_param_grads`, and every weight-gradient launch goes through one launcher, `_wgrad`.  The residual unit is ONE node for both
storage types, `ResidualBlockFunction`.
"""
from __future__ import annotations

import os

import ctypes as C

import torch

from . import _lib as L
from . import profiling
from .metadata import Metadata, Rules


def _f32(t: torch.Tensor) -> torch.Tensor:
    if t.dtype != torch.float32:
        raise TypeError(f"sparse_rcnn_amd operators compute in fp32; got {t.dtype}")
    if not t.is_cuda:
        raise L.ScnError("feature tensors must live on the MI355X (no CPU fallback)")
    return t.contiguous()


def _new(shape, like, dtype=torch.float32):
    return torch.empty(shape, dtype=dtype, device=like.device)


def _feat(t: torch.Tensor) -> torch.Tensor:
    """Feature slab of a conv-type layer: fp32, or bf16 STORAGE (BASELINE configs 3-5: the bf16 entry points of the
    library; parameters and their gradients stay fp32)."""
    if t.dtype == torch.bfloat16:
        if not t.is_cuda:
            raise L.ScnError("feature tensors must live on the MI355X (no CPU fallback)")
        return t.contiguous()
    return _f32(t)


def _is_bf16(t):
    return t.dtype == torch.bfloat16


# Debug hook for the parity tests: when a list, every FORWARD that applies a ReLU to a stored slab
# (the fused input ReLU of a convolution, scn.ReLU) appends that slab's sign mask (x > 0, bool, on the host) in call order.
# An oracle that takes these masks instead of its own `relu` decisions differentiates the same piecewise-linear function,
# so ReLU inputs within rounding of zero no longer separate the two gradients.  None (default): nothing is recorded.
RELU_RECORD = None


def _rec_relu(X):
    if RELU_RECORD is not None:
        RELU_RECORD.append((X.detach() > 0).cpu())


# ------------------------------------------------------------------------------------------------------
# raw kernels (no autograd)
# ------------------------------------------------------------------------------------------------------

def _conv_bytes(n_in, cin, n_out, cout, n_off, n_rules):
    """Compulsory HBM bytes of one conv-type launch: X once, Y once, W, int32 rule pairs."""
    return 4.0 * (n_in * cin + n_out * cout + n_off * cin * cout) + 8.0 * n_rules


def _count(n_rules):
    """n_rules: an int or a metadata.RuleCount (whose total is read lazily; it holds no device buffers)."""
    return n_rules if isinstance(n_rules, int) else n_rules.total


def gemm_table(X, table, n_off, n_out, W, bias, cout, flags=0, residual=None, relu_mask=None, n_rules=None):
    """n_rules: number of (in,out) rules the table holds (int or RuleCount) -- only used for the algorithmic-FLOP
    accounting, evaluated when a profile is summarised."""
    lib = L.lib()
    cin = X.shape[1]
    Y = _new((n_out, cout), X, X.dtype)
    n_in = X.shape[0]
    P = (lambda: n_out) if n_rules is None else (lambda: _count(n_rules))
    entry = lib.scn_gemm_table_bf16 if _is_bf16(X) else lib.scn_gemm_table       # bf16 storage: same arithmetic

    def run():
        L.check(entry(L.ptr(X), X.shape[0], cin, L.ptr(table), n_off, n_out, L.ptr(W), L.ptr(bias),
                      L.ptr(residual), L.ptr(relu_mask), L.ptr(Y), cout, flags, L.stream()))
    profiling.timed("k_gemm_table", lambda: 2.0 * P() * cin * cout,
                    lambda: _conv_bytes(n_in, cin, n_out, cout, n_off, P()), run)
    return Y


_ts_scratch_cache = {}
_tb_sizes = {}
FUSED_K = True      # scn_conv_tiles adds its K-chunk partial sums inside the launch (False: second launch k_conv_ts_sum)


def _cache_put(cache, key, value):
    """A miss of one of the size caches: they are bounded -- one that holds more than 4096 keys starts again empty."""
    if len(cache) > 4096:
        cache.clear()
    cache[key] = value
    return value


def _conv_tiles_scratch_bytes(cin, n_out, cout):
    key = (cin, n_out, cout)
    v = _ts_scratch_cache.get(key)
    return v if v is not None else _cache_put(_ts_scratch_cache, key, L.lib().scn_conv_tiles_scratch_bytes(cin, n_out, cout))


def conv_rules(X, tiles, n_out, W, bias, cout, flags=0, residual=None, relu_mask=None, n_rules=0, image=None):
    """The hot kernel: output-stationary convolution over mask-sorted tiles (scn_conv_tiles).  image: bf16 storage only,
    a packed weight image for these flags."""
    if _is_bf16(X):
        return conv_rules_bf16(X, tiles, n_out, W, bias, cout, flags, residual, relu_mask, image=image, n_rules=n_rules)
    lib = L.lib()
    cin = X.shape[1]
    Y = _new((n_out, cout), X)
    n_in, n_off = X.shape[0], tiles.n_off      # the profiling closures below must not keep device buffers alive
    P = lambda: _count(n_rules)
    scratch = L.scratch(_conv_tiles_scratch_bytes(cin, n_out, cout), X.device)
    n_kc = (cin + 31) // 32
    # layers with more than 32 input channels: the K-chunk partial sums are added inside the launch (zeroed arrival
    # counters, left zero by the kernel); FUSED_K = False is the two-launch form (cross-check in the tests)
    arr = L.arrival(((n_out + 15) // 16) * ((cout + 31) // 32), X.device) if (n_kc > 1 and FUSED_K) else None

    def run(fl=flags):
        L.check(lib.scn_conv_tiles(L.ptr(X), n_in, cin, L.ptr(tiles.tstab), L.ptr(tiles.tile_mask), L.ptr(tiles.perm),
                                   L.ptr(tiles.tile_order), tiles.n_off, n_out, L.ptr(W), L.ptr(bias), L.ptr(residual), L.ptr(relu_mask),
                                   L.ptr(Y), cout, fl, L.ptr(scratch), L.ptr(arr), L.stream()))
    if profiling.TIMER is None:
        run()
        return Y
    if arr is not None or n_kc == 1:
        # one launch per convolution: the timing events bracket exactly the production kernel
        profiling.timed("k_conv_ts", lambda: 2.0 * P() * cin * cout,
                        lambda: _conv_bytes(n_in, cin, n_out, cout, n_off, P()), run)
        return Y
    # two-launch form, timed: the events bracket the tile kernel alone; the K-chunk slab sum is launched -- and timed -- apart
    profiling.timed("k_conv_ts", lambda: 2.0 * P() * cin * cout,
                    lambda: _conv_bytes(n_in, cin, n_out, cout, n_off, P()), lambda: run(flags | L.F_SPLIT_SUM))
    profiling.timed("k_conv_ts_sum", 0.0, 4.0 * n_out * cout * (n_kc + 1) if n_kc > 1 else 0.0,
                    lambda: L.check(lib.scn_conv_tiles_finish(cin, n_out, L.ptr(bias), L.ptr(residual), L.ptr(relu_mask),
                                                              L.ptr(Y), cout, flags, L.ptr(scratch), L.stream())))
    return Y


def pack_weights_bf16(W, cin, cout, n_off, flags=0):
    """scn_conv_tiles_bf16_pack: the layer's fp32 master weights -> the bf16 image the tile kernel stages (one rounding per
    weight).  flags: F_W_TRANSPOSED | F_OFF_REVERSE select the backward-data image.  Valid until W changes: callers pack
    per use (forward / backward of one step) and never cache across steps."""
    lib = L.lib()
    img = torch.empty(lib.scn_conv_tiles_bf16_image_bytes(cin, cout, n_off), dtype=torch.uint8, device=W.device)
    L.check(lib.scn_conv_tiles_bf16_pack(L.ptr(W), cin, cout, n_off, flags & (L.F_W_TRANSPOSED | L.F_OFF_REVERSE),
                                         L.ptr(img), L.stream()))
    return img


# ---- channel-padded parameters of a network, one launch each way -----------------------------------------------------------
# modules._ConvBase / NetworkInNetwork hand the kernels zero-padded copies of their logical parameters where a level runs on
# padded slabs (unet.SparseUNet.phys0: the mask network's 23 -> 24 columns).  Through torch.nn.functional.pad that is a fill +
# a copy per tensor forward and a slice copy backward -- ~50 launches of ~4.5 us per detection + mask step.  `padded_params`
# pads every tensor of a fixed list with ONE scn_pad_params_many launch (its backward: one launch slices all gradients);
# `_wb` of the modules picks its tensors up from PADDED while the block is open.
PADDED = {}
PAD_MANY = os.environ.get("SCN_PAD_MANY", "1") != "0"      # 0: tensor-by-tensor torch pads (A/B, cross-check in the tests)
PAD_RECORD = None        # a list while a network records which (module, cin_phys) its forward asks `_wb` for


class PadPlan:
    """jobs: [(key, module, attribute, padded shape, segments)] -- key: what `_wb` asks PADDED for ((id(module), cin_phys,
    "w" | "b")); getattr(module, attribute): the logical parameter, [fv, rows, cols] / [rows, cols] / [cols] (fetched at every
    use: module.to(...) replaces the tensors); padded shape: same rank; segments: up to two (src row, count, dst row) triples
    (None: all rows at row 0)."""

    @classmethod
    def from_requests(cls, requests):
        """requests: the (module, cin_phys) pairs a forward recorded (PAD_RECORD) -> plan, or False when there are none."""
        jobs, seen = [], set()
        for m, cin_phys in requests:
            if (id(m), cin_phys) not in seen:
                seen.add((id(m), cin_phys))
                jobs += m._pad_jobs(cin_phys)
        return cls(jobs) if jobs else False

    def fetch(self):
        return [getattr(m, a) for _, m, a, _, _ in self.jobs]

    def __init__(self, jobs):
        self.jobs = list(jobs)
        self.n = len(self.jobs)
        self.params = self.fetch()
        desc, self.out_shapes, self.out_offs, self.in_offs = [], [], [], []
        tot_out = tot_in = 0
        for (key, _, _, shape, segs), t in zip(self.jobs, self.params):
            s3 = (1,) * (3 - t.dim()) + tuple(t.shape)
            d3 = (1,) * (3 - len(shape)) + tuple(int(v) for v in shape)
            segs = list(segs) if segs else [(0, s3[1], 0)]
            segs += [(0, 0, 0)] * (2 - len(segs))
            desc += [s3[0], s3[1], s3[2], d3[1], d3[2], *segs[0], *segs[1]]
            if d3[0] != s3[0]:
                raise ValueError("PadPlan: the leading dimension is never padded")
            self.out_shapes.append(tuple(int(v) for v in shape))
            self.out_offs.append(tot_out); self.in_offs.append(tot_in)
            tot_out += (d3[0] * d3[1] * d3[2] + 3) & ~3                       # 16-byte aligned tensors
            tot_in += (t.numel() + 3) & ~3
        self.total_out, self.total_in = tot_out, tot_in
        self.desc = (C.c_int32 * len(desc))(*desc)
        self.src = (C.c_void_p * self.n)()
        self.dst = (C.c_void_p * self.n)()
        self.keys = [j[0] for j in self.jobs]


class _PadMany(torch.autograd.Function):
    @staticmethod
    def forward(ctx, plan, *params):
        buf = torch.empty(plan.total_out, dtype=torch.float32, device=params[0].device)
        base = buf.data_ptr()
        for i, p in enumerate(params):
            if p.dtype != torch.float32 or not p.is_contiguous():
                raise TypeError("padded_params: contiguous fp32 parameters")
            plan.src[i] = p.data_ptr()
            plan.dst[i] = base + 4 * plan.out_offs[i]
        L.check(L.lib().scn_pad_params_many(plan.n, plan.src, plan.dst, plan.desc, 0, L.stream()))
        ctx.plan = plan
        outs = []
        for off, shape in zip(plan.out_offs, plan.out_shapes):
            n = 1
            for v in shape:
                n *= v
            outs.append(buf[off:off + n].view(shape))
        return tuple(outs)

    @staticmethod
    def backward(ctx, *grads):
        plan = ctx.plan
        dev = next(g.device for g in grads if g is not None)
        buf = torch.empty(plan.total_in, dtype=torch.float32, device=dev)
        base, keep = buf.data_ptr(), []
        src, dst = (C.c_void_p * plan.n)(), (C.c_void_p * plan.n)()      # (own tables: backward runs on autograd's thread)
        for i, g in enumerate(grads):
            if g is not None and (g.dtype != torch.float32 or not g.is_contiguous()):
                g = g.float().contiguous()
            keep.append(g)
            src[i] = g.data_ptr() if g is not None else None
            dst[i] = base + 4 * plan.in_offs[i]
        L.check(L.lib().scn_pad_params_many(plan.n, src, dst, plan.desc, 1, L.stream()))
        return (None,) + tuple(buf[off:off + p.numel()].view(p.shape) for off, p in zip(plan.in_offs, plan.params))


class padded_params:
    """Context manager: the padded tensors of `plan` are in PADDED until the block ends (nested blocks of other networks keep
    theirs).  Outside a CUDA device or with no jobs it does nothing -- `_wb` then pads tensor by tensor as before."""

    def __init__(self, plan):
        self.plan, self.keys = plan, []

    def __enter__(self):
        pl = self.plan
        if not pl or not pl.n:
            return self
        pl.params = pl.fetch()
        if not pl.params[0].is_cuda:
            return self
        outs = _PadMany.apply(pl, *pl.params)
        for key, t in zip(pl.keys, outs):
            PADDED[key] = t
        self.keys = pl.keys
        return self

    def __exit__(self, *exc):
        for k in self.keys:
            PADDED.pop(k, None)
        return False


# Weight images packed for the forward pass that is running (packed_weights below): (data_ptr, cin, cout, n_off, flags & 6)
# -> image.  Filled by ONE launch for a whole network, emptied when its forward ends; a backward-data image is handed to the
# autograd node during the forward (ctx) -- nothing here outlives a step, so an optimizer update can never meet a stale image.
PACKED = {}
_BACK = L.F_W_TRANSPOSED | L.F_OFF_REVERSE


def packed_image(W, cin, cout, n_off, flags):
    """The packed bf16 image of a layer's weight as a tensor (a view of the pack buffer), or None."""
    e = PACKED.get((W.data_ptr(), cin, cout, n_off, flags & _BACK))
    if e is None or torch.is_tensor(e):
        return e
    buf, o, b, _ = e
    return buf[o:o + b]


def packed_entry(W, cin, cout, n_off, flags):
    """(pack buffer, device address of the image) or None -- what the step executor needs (an address for its table and ONE
    tensor to keep alive); slicing a view per image cost the host ~2.5 us each, 124 per step."""
    e = PACKED.get((W.data_ptr(), cin, cout, n_off, flags & _BACK))
    if e is None:
        return None
    if torch.is_tensor(e):
        return e, e.data_ptr()
    return e[0], e[3]


class PackPlan:
    """Host-side argument tables of one scn_conv_tiles_bf16_pack_many call for a fixed list of layers."""

    def __init__(self, jobs):
        self.jobs = list(jobs)
        self.n = len(self.jobs)
        self.weights = [j[0] for j in self.jobs]
        if self.n:
            self.rebuild()

    def rebuild(self):
        lib = L.lib()
        jobs, n = self.jobs, self.n
        self.ptrs = [W.data_ptr() for W in self.weights]
        self.sizes = [lib.scn_conv_tiles_bf16_image_bytes(ci, co, no) for (_, ci, co, no, _) in jobs]
        self.offs, tot = [], 0
        for b in self.sizes:
            self.offs.append(tot)
            tot += (b + 255) & ~255
        self.total = tot
        self.Wp = (C.c_void_p * n)(*self.ptrs)
        self.Ip = (C.c_void_p * n)()
        self.ci = (C.c_int32 * n)(*[j[1] for j in jobs]); self.co = (C.c_int32 * n)(*[j[2] for j in jobs])
        self.no = (C.c_int32 * n)(*[j[3] for j in jobs]); self.fl = (C.c_int32 * n)(*[j[4] & _BACK for j in jobs])
        self.keys = [(W.data_ptr(), cin, cout, n_off, flags & _BACK) for (W, cin, cout, n_off, flags) in jobs]


class packed_weights:
    """Context manager: pack the bf16 weight images (forward and backward-data) of `jobs` = [(W, cin, cout, n_off, flags)]
    with one scn_conv_tiles_bf16_pack_many launch; they are visible through packed_image() until the block ends."""

    def __init__(self, jobs):
        """jobs: a list, or a `PackPlan` (the host-side tables of a fixed list, built once and re-used every step)."""
        self.plan = jobs if isinstance(jobs, PackPlan) else PackPlan(jobs)
        self.keys = []

    def __enter__(self):
        pl = self.plan
        if not pl.n:
            return self
        if pl.ptrs != [W.data_ptr() for W in pl.weights]:          # a parameter moved (module.to(...), load): rebuild
            pl.rebuild()
        buf = torch.empty(pl.total, dtype=torch.uint8, device=pl.weights[0].device)
        base = buf.data_ptr()
        for i, o in enumerate(pl.offs):
            pl.Ip[i] = base + o
        L.check(L.lib().scn_conv_tiles_bf16_pack_many(pl.n, pl.Wp, pl.ci, pl.co, pl.no, pl.fl, pl.Ip, L.stream()))
        for key, o, b in zip(pl.keys, pl.offs, pl.sizes):
            PACKED[key] = (buf, o, b, base + o)           # (views are cut on demand: packed_image)
        self.keys = pl.keys
        return self

    def __exit__(self, *exc):
        for k in self.keys:
            PACKED.pop(k, None)
        return False


def conv_rules_bf16(X, tiles, n_out, W, bias, cout, flags=0, residual=None, relu_mask=None, image=None, n_rules=0):
    """scn_conv_tiles_bf16: the tile convolution for bf16-stored features (X, residual, relu_mask, result: torch.bfloat16;
    W, bias: the layer's fp32 parameters).  Forward and, with F_W_TRANSPOSED | F_OFF_REVERSE, backward-data.
    image: a packed weight image of W for these flags (pack_weights_bf16); None: packed here."""
    lib = L.lib()
    for t in (X, residual, relu_mask):
        if t is not None and (t.dtype != torch.bfloat16 or not t.is_contiguous()):
            raise L.ScnError("conv_rules_bf16 takes contiguous torch.bfloat16 features")
    if W.dtype != torch.float32 or (bias is not None and bias.dtype != torch.float32):
        raise L.ScnError("conv_rules_bf16 takes the fp32 master weights")
    cin = X.shape[1]
    if cin % 8:
        raise L.ScnError("bf16 storage needs input channel counts that are multiples of 8 (16-byte row pieces)")
    n_in, n_off = X.shape[0], tiles.n_off
    if image is None:
        image = packed_image(W, cin, cout, n_off, flags)
    if image is None:
        image = pack_weights_bf16(W, cin, cout, n_off, flags)
    Y = torch.empty((n_out, cout), dtype=torch.bfloat16, device=X.device)
    if getattr(tiles, "has_x", False):
        flags |= L.F_TILE_ORDER_X               # tile_order continues with the XCD-local hand-out order (scn_tiles_build_x)
    key = (cin, n_out, cout)
    sz = _tb_sizes.get(key)
    if sz is None:
        sz = _cache_put(_tb_sizes, key, (lib.scn_conv_tiles_bf16_scratch_bytes(cin, n_out, cout),
                                         lib.scn_conv_tiles_bf16_arrival_counters(cin, n_out, cout)))
    scratch = L.scratch(sz[0], X.device)
    arr = L.arrival(sz[1], X.device) if (sz[1] and FUSED_K) else None

    def run():
        L.check(lib.scn_conv_tiles_bf16(
            L.ptr(X), n_in, cin, L.ptr(tiles.tstab), L.ptr(tiles.tile_mask), L.ptr(tiles.perm),
            L.ptr(tiles.tile_order), n_off, n_out, L.ptr(image), L.ptr(bias), L.ptr(residual), L.ptr(relu_mask),
            L.ptr(Y), cout, flags, L.ptr(scratch), L.ptr(arr), L.stream()))
    if profiling.TIMER is None:
        run()
        return Y
    P = lambda: _count(n_rules)
    profiling.timed("k_conv_tb", lambda: 2.0 * P() * cin * cout,
                    lambda: 2.0 * (n_in * cin + n_out * cout + n_off * cin * cout) + 8.0 * P(), run)
    return Y


# The 3^3 / 2^3 table convolutions run on the tile kernel (scn_conv_tiles); USE_TILES = False routes them through the
# plain table GEMM (scn_gemm_table: no mask sorting, 2-3x wasted matrix work) -- kept as a cross-check of the two kernels.
USE_TILES = True


def gemm_rules(X, in_rows, out_rows, prefix_host, n_off, n_out, W, bias, cout, flags=0, relu_mask=None):
    lib = L.lib()
    Y = _new((n_out, cout), X, X.dtype)
    cin = X.shape[1]
    P = int(prefix_host[n_off] - prefix_host[0])
    entry = lib.scn_gemm_rules_bf16 if _is_bf16(X) else lib.scn_gemm_rules

    def run():
        # the entry point takes up to 32 offsets per call; every output row occurs in exactly one rule (the callers: Deconvolution
        # forward, Convolution backward-data), so the chunks of a larger filter (a 4^3 stride: 64) write disjoint rows of one Y
        for o0 in range(0, n_off, 32):
            k = min(32, n_off - o0)
            ph = _offset_chunk(prefix_host, o0)
            Wp = L.ptr(W) + 4 * o0 * W.shape[1] * W.shape[2] if o0 else L.ptr(W)
            L.check(entry(L.ptr(X), cin, L.ptr(in_rows), L.ptr(out_rows), ph, k, Wp,
                          L.ptr(bias), L.ptr(relu_mask), L.ptr(Y), cout, flags, L.stream()))
    profiling.timed("k_gemm_rules", 2.0 * P * cin * cout, _conv_bytes(X.shape[0], cin, n_out, cout, n_off, P), run)
    return Y


def _offset_chunk(prefix_host, o0):
    """`prefix_host` advanced by o0 offsets (the rule-list entry points take up to 32 offsets per call; rule rows are addressed
    through the absolute prefix, so a chunk is the same arrays with a later prefix pointer)."""
    return prefix_host if o0 == 0 else C.cast(C.addressof(prefix_host.contents) + 8 * o0, C.POINTER(C.c_int64))


def _wgrad(Xs, dYs, in_rows, out_rows, prefix_host, n_off, db_offsets, flags, want_db):
    """The one weight-gradient launcher; the public forms below are fronts of it.  Xs, dYs: ONE operand pair (two tensors) or a
    sequence of 2 ... 4 pairs that share the rule list and their channel counts; fp32 or bf16-stored, of one storage type,
    contiguous (checked where it was always checked: bf16-stored operands and the several-pair form).  At most 32 offsets.
    The entry point follows from (storage type, one pair or several, want_db):
        one pair, no db     scn_wgrad_rules / _bf16
        one pair, db        scn_wgrad_bias_rules / _bf16           (db over the rule lists of the offsets in `db_offsets`)
        several pairs       scn_wgrad_bias_rules_n / _n_bf16       (db where want_db, else a NULL db)
    -> fp32 (dW [n_off, cin, cout], db [cout] or None); several pairs: (dW [n_prob, n_off, cin, cout], db [n_prob, cout] or None)."""
    lib = L.lib()
    one = torch.is_tensor(Xs)
    X, dY = (Xs, dYs) if one else (Xs[0], dYs[0])
    hb = X.dtype == torch.bfloat16
    cin, cout = X.shape[1], dY.shape[1]
    dev = X.device
    if one:
        if hb and (dY.dtype != torch.bfloat16 or not (X.is_contiguous() and dY.is_contiguous())):
            raise L.ScnError("the weight gradient takes contiguous operands of one storage type")
        n_prob = 1
        nbytes = lib.scn_wgrad_scratch_bytes(cin, cout, prefix_host, n_off)
        w_shape, b_shape = (n_off, cin, cout), (cout,)
    else:
        n_prob = len(Xs)
        if any(t.dtype != X.dtype or not t.is_contiguous() for t in Xs + dYs):
            raise L.ScnError("the weight gradient takes contiguous operands of one storage type")
        nbytes = lib.scn_wgrad_scratch_bytes_n(cin, cout, prefix_host, n_off, n_prob)
        w_shape, b_shape = (n_prob, n_off, cin, cout), (n_prob, cout)
    if nbytes < 0:
        raise L.ScnError("scn_wgrad_scratch_bytes" + ("" if one else "_n") + ": bad arguments")
    scratch = L.scratch(nbytes, dev)
    dW = torch.empty(w_shape, dtype=torch.float32, device=dev)
    db = torch.empty(b_shape, dtype=torch.float32, device=dev) if want_db else None
    if not one:
        entry = lib.scn_wgrad_bias_rules_n_bf16 if hb else lib.scn_wgrad_bias_rules_n
        xp = (C.c_void_p * n_prob)(*[t.data_ptr() for t in Xs])
        yp = (C.c_void_p * n_prob)(*[t.data_ptr() for t in dYs])

        def run():
            L.check(entry(xp, yp, n_prob, cin, cout, L.ptr(in_rows), L.ptr(out_rows), prefix_host, n_off, L.ptr(dW), L.ptr(db),
                          db_offsets, L.ptr(scratch), flags, L.stream()))
    elif want_db:
        entry = lib.scn_wgrad_bias_rules_bf16 if hb else lib.scn_wgrad_bias_rules

        def run():
            L.check(entry(L.ptr(X), cin, L.ptr(dY), cout, L.ptr(in_rows), L.ptr(out_rows), prefix_host, n_off, L.ptr(dW),
                          L.ptr(db), db_offsets, L.ptr(scratch), flags, L.stream()))
    else:
        entry = lib.scn_wgrad_rules_bf16 if hb else lib.scn_wgrad_rules

        def run():
            L.check(entry(L.ptr(X), cin, L.ptr(dY), cout, L.ptr(in_rows), L.ptr(out_rows), prefix_host, n_off, L.ptr(dW),
                          L.ptr(scratch), flags, L.stream()))
    if hb and one and not want_db:
        flops = moved = 0.0             # (a reporting gap as old as the bf16 no-bias form: it tells the timer nothing)
    else:
        P = int(prefix_host[n_off] - prefix_host[0])
        flops = 2.0 * n_prob * P * cin * cout
        moved = n_prob * ((2.0 if hb else 4.0) * (X.shape[0] * cin + dY.shape[0] * cout) + 4.0 * n_off * cin * cout + 8.0 * P)
    profiling.timed("k_wgrad_rules_bf16" if hb else "k_wgrad_rules", flops, moved, run)
    return dW, db


def wgrad_rules(X, dY, in_rows, out_rows, prefix_host, n_off, flags=0):
    """dW alone (scn_wgrad_rules; bf16-stored operands: scn_wgrad_rules_bf16, fp32 result)."""
    if n_off > 32:          # (a 4^3 stride, a 5^3 filter: chunks of 32 offsets)
        return torch.cat([wgrad_rules(X, dY, in_rows, out_rows, _offset_chunk(prefix_host, o0), min(32, n_off - o0), flags)
                          for o0 in range(0, n_off, 32)], 0)
    return _wgrad(X, dY, in_rows, out_rows, prefix_host, n_off, 0, flags, False)[0]


def wgrad_rules_bf16(X, dY, in_rows, out_rows, prefix_host, n_off, flags=0):
    """`wgrad_rules` that refuses anything but bf16-stored operands -- the weight gradient of the bf16 storage path."""
    if not (_is_bf16(X) and _is_bf16(dY)):
        raise L.ScnError("wgrad_rules_bf16 takes contiguous torch.bfloat16 operands")
    return wgrad_rules(X, dY, in_rows, out_rows, prefix_host, n_off, flags)


def wgrad_bias_rules(X, dY, in_rows, out_rows, prefix_host, n_off, db_offsets, flags=0):
    """dW and db in one pass (scn_wgrad_bias_rules; bf16-stored operands: scn_wgrad_bias_rules_bf16, fp32 results)."""
    return _wgrad(X, dY, in_rows, out_rows, prefix_host, n_off, db_offsets, flags, True)


# residual units: both weight gradients in one launch (False / SCN_WGRAD_PAIR=0: one call each -- cross-check, A/B)
WGRAD_PAIR = os.environ.get("SCN_WGRAD_PAIR", "1") != "0"


def wgrad_bias_rules_n(Xs, dYs, in_rows, out_rows, prefix_host, n_off, db_offsets, flags=0):
    """The weight (and, db_offsets != 0, bias) gradients of 2 ... 4 convolutions that share a rule list and their channel
    counts -- the two of a residual unit, the four of two stacked units -- in one launch + one sum
    (scn_wgrad_bias_rules_n / _bf16): operand pairs (Xs[p], dYs[p]) of one storage type.
    -> fp32 dW [n_prob, n_off, cin, cout], db [n_prob, cout] or None."""
    return _wgrad(tuple(Xs), tuple(dYs), in_rows, out_rows, prefix_host, n_off, db_offsets, flags, bool(db_offsets))


def wgrad_bias_rules2(X0, dY0, X1, dY1, in_rows, out_rows, prefix_host, n_off, db_offsets, flags=0):
    return _wgrad((X0, X1), (dY0, dY1), in_rows, out_rows, prefix_host, n_off, db_offsets, flags, bool(db_offsets))


def colsum(dY):
    """Bias gradient db[c] = sum_r dY[r][c] (fp32 result; dY fp32 or bf16-stored), two-stage, fixed order."""
    lib = L.lib()
    c = dY.shape[1]
    scratch = torch.empty(L.COLSUM_BLOCKS * c, dtype=torch.float32, device=dY.device)
    db = torch.empty(c, dtype=torch.float32, device=dY.device)
    entry = lib.scn_colsum_bf16 if _is_bf16(dY) else lib.scn_colsum
    L.check(entry(L.ptr(dY), dY.shape[0], c, L.ptr(db), L.ptr(scratch), L.stream()))
    return db


def _identity_prefix(n):
    h = L.host_i64(2)
    h[0], h[1] = 0, n
    return h


def _param_grads(X, dY, rules, n_off, shape, want_w, want_b, bias_offsets=0, flags=0, swap=False):
    """The parameter gradients of a convolution-type layer, Y[out] += X[in] . W[offset] over a rule list -- the one place that
    decides how they are computed:
        dW and db wanted, and the node names `bias_offsets`     one pass (scn_wgrad_bias_rules)
        dW wanted                                               the weight gradient alone (scn_wgrad_rules, chunked above 32 offsets)
        db wanted and not yet there                             colsum(dY)
    rules: the layer's `metadata.Rules`, or None for a 1x1 layer (an identity prefix over the rows of dY, no row arrays); swap: the
    rule list with its row roles exchanged (a Deconvolution runs its Convolution's).  The rows are asked for only where a weight
    gradient is wanted: a `Rules` object compacts its lists at the first request, one launch a frozen layer must not cause.
    bias_offsets: the mask of offsets whose rule lists together name every row of dY exactly once (the centre of a submanifold
    filter, every offset of a Deconvolution, the one offset of a 1x1 layer); 0 where the node never takes the one-pass form (a
    strided Convolution: a coarse row occurs once per child it has, and no set of offsets sorts that out) or has more offsets than
    that form is used for.
    -> (dW viewed as `shape`, db), each None where not wanted.  (Called with positional arguments: it runs once per layer and step.)
    These are leaves of the backward graph and run on the main stream (a second stream for them was measured in round 1: no gain)."""
    dW = db = None
    if want_w:
        if rules is None:
            in_rows = out_rows = None
            prefix_host = _identity_prefix(dY.shape[0])
        elif swap:
            in_rows, out_rows, prefix_host = rules.out_rows, rules.in_rows, rules.prefix_host
        else:
            in_rows, out_rows, prefix_host = rules.in_rows, rules.out_rows, rules.prefix_host
        if want_b and bias_offsets:
            dW, db = _wgrad(X, dY, in_rows, out_rows, prefix_host, n_off, bias_offsets, flags, True)
        elif n_off > 32:
            dW = wgrad_rules(X, dY, in_rows, out_rows, prefix_host, n_off, flags)
        else:
            dW = _wgrad(X, dY, in_rows, out_rows, prefix_host, n_off, 0, flags, False)[0]
        dW = dW.view(shape)
    if want_b and db is None:
        db = colsum(dY)
    return dW, db


# ------------------------------------------------------------------------------------------------------
# A5 SubmanifoldConvolution  (module_factory.py:383-385 k=1, 404-406 k=3)
# ------------------------------------------------------------------------------------------------------
class SubmanifoldConvolutionFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, features, weight, bias, metadata: Metadata, spatial_size, k, relu_in=False, residual=None):
        """residual (optional, [N, Cout]): added in the kernel epilogue -- the AddTable of a residual block fused
        (module_factory.py:51-57: Sequential(ConcatTable(Identity, inner), AddTable))."""
        X, W = _feat(features), _f32(weight)
        rb = metadata.subm_rulebook(spatial_size, k)
        n_off = k ** 3
        cout = W.shape[-1]
        b = _f32(bias) if bias is not None else None
        R = _feat(residual) if residual is not None else None
        if relu_in:
            _rec_relu(X)
        if USE_TILES and rb.rules is not None and rb.tiles is not None:
            Y = conv_rules(X, rb.tiles, rb.n, W, b, cout, L.F_RELU_IN if relu_in else 0, residual=R,
                           n_rules=rb.rules.count)
        else:
            Y = gemm_table(X, rb.table, n_off, rb.n, W, b, cout, L.F_RELU_IN if relu_in else 0, residual=R,
                           n_rules=rb.rules.count if rb.rules is not None else rb.n)
        ctx.save_for_backward(X, W)
        ctx.rb, ctx.has_bias, ctx.relu_in = rb, bias is not None, relu_in
        ctx.bwd_image = packed_image(W, cout, X.shape[1], n_off, _BACK) if _is_bf16(X) else None
        return Y

    @staticmethod
    def backward(ctx, dY):
        X, W = ctx.saved_tensors
        rb = ctx.rb
        dY = _feat(dY)
        n_off = rb.k ** 3
        cin = X.shape[1]
        fl = L.F_RELU_IN if ctx.relu_in else 0
        dX = None
        if ctx.needs_input_grad[0]:
            if USE_TILES and rb.rules is not None and rb.tiles is not None:
                dX = conv_rules(dY, rb.tiles, rb.n, W, None, cin, L.F_W_TRANSPOSED | L.F_OFF_REVERSE,
                                relu_mask=X if ctx.relu_in else None, n_rules=rb.rules.count, image=ctx.bwd_image)
            else:
                dX = gemm_table(dY, rb.table, n_off, rb.n, W, None, cin, L.F_W_TRANSPOSED | L.F_OFF_REVERSE,
                                relu_mask=X if ctx.relu_in else None,
                                n_rules=rb.rules.count if rb.rules is not None else rb.n)
        # the centre offset lists every row once (filters of up to 32 offsets: one call of the one-pass form)
        dW, db = _param_grads(X, dY, None if rb.k == 1 else rb.rules, n_off, W.shape, ctx.needs_input_grad[1],
                              ctx.has_bias and ctx.needs_input_grad[2], 1 << (n_off // 2) if n_off <= 32 else 0, fl)
        dR = dY if (len(ctx.needs_input_grad) > 7 and ctx.needs_input_grad[7]) else None
        return dX, dW, db, None, None, None, None, dR


# ------------------------------------------------------------------------------------------------------
# Residual block  x + SubM3(ReLU(SubM3(ReLU(x))))  as ONE autograd node  (module_factory.py:127-183 get_residual_block
# with relu_first, two units; custom_container.py: Sequential(ConcatTable(Identity, inner), AddTable))
# ------------------------------------------------------------------------------------------------------
class ResidualBlockFunction(torch.autograd.Function):
    """Same kernels as the layer-by-layer path; what the fusion removes is the glue: the AddTable runs in the epilogue
    of the second convolution (forward) and the sum of the two gradient paths of x in the epilogue of the first
    convolution's backward-data kernel (SCN_F_RESIDUAL_LAST: dX = mask(conv1^T dY1) + dY) -- no elementwise launches, one
    autograd node instead of two.

    One node for both storage types, told apart by `features.dtype`.  bf16-STORED features (BASELINE configs 3-5): x,
    the intermediate h, the result and every gradient tensor of the block are torch.bfloat16; the parameters stay fp32 (rounded to
    bf16 as they are staged into LDS) and their gradients come back fp32.  Six launches either way: the tile convolution x 4
    (two forward, two backward-data with the ReLU mask / the skip gradient in the epilogue) and the weight gradients."""

    @staticmethod
    def forward(ctx, features, w1, b1, w2, b2, metadata: Metadata, spatial_size):
        hb = _is_bf16(features)
        if hb:
            if features.shape[1] % 8 != 0 or w1.shape[-1] % 8 != 0:
                raise L.ScnError("bf16 storage needs channel counts that are multiples of 8 (16-byte row pieces)")
            X = features.contiguous()
        else:
            X = _f32(features)
        W1, W2 = _f32(w1), _f32(w2)
        rb = metadata.subm_rulebook(spatial_size, 3)
        B1 = _f32(b1) if b1 is not None else None
        B2 = _f32(b2) if b2 is not None else None
        Y1 = conv_rules(X, rb.tiles, rb.n, W1, B1, W1.shape[-1], L.F_RELU_IN, n_rules=rb.rules.count)
        Y = conv_rules(Y1, rb.tiles, rb.n, W2, B2, W2.shape[-1], L.F_RELU_IN, residual=X, n_rules=rb.rules.count)
        _rec_relu(X); _rec_relu(Y1)
        ctx.save_for_backward(X, Y1, W1, W2)
        ctx.rb, ctx.has_b1, ctx.has_b2 = rb, b1 is not None, b2 is not None
        # the packed backward-data images of the forward that is running (bf16 storage alone has any)
        ctx.bwd_images = (packed_image(W1, W1.shape[-1], W1.shape[1], 27, _BACK),
                          packed_image(W2, W2.shape[-1], W2.shape[1], 27, _BACK)) if hb else (None, None)
        return Y

    @staticmethod
    def backward(ctx, dY):
        X, Y1, W1, W2 = ctx.saved_tensors
        rb, r = ctx.rb, ctx.rb.rules
        dY = dY.to(torch.bfloat16).contiguous() if _is_bf16(X) else _f32(dY)
        need = ctx.needs_input_grad
        centre = 1 << 13                # the centre offset lists every row once
        dY1 = conv_rules(dY, rb.tiles, rb.n, W2, None, W2.shape[1], _BACK, relu_mask=Y1, n_rules=r.count, image=ctx.bwd_images[1])
        want_b1, want_b2 = ctx.has_b1 and need[2], ctx.has_b2 and need[4]
        # both weight gradients in one launch (same rule list, same channel counts; bias gradients both or neither).  The launch
        # wants contiguous operands, and all four are by construction in both storage types: X left the forward's `_f32` /
        # `.contiguous()`, dY the line above, Y1 and dY1 are slabs `conv_rules` allocated
        pair = (WGRAD_PAIR and need[1] and need[3] and want_b1 == want_b2 and W1.shape == W2.shape
                and W1.shape[1] == W1.shape[2] and r.prefix_host[0] == 0)
        if not pair:
            dW2, db2 = _param_grads(Y1, dY, r, 27, W2.shape, need[3], want_b2, centre, L.F_RELU_IN)
        dX = None
        if need[0]:
            dX = conv_rules(dY1, rb.tiles, rb.n, W1, None, W1.shape[1], _BACK | L.F_RESIDUAL_LAST, relu_mask=X,
                            residual=dY, n_rules=r.count, image=ctx.bwd_images[0])
        if pair:
            dWp, dbp = wgrad_bias_rules2(X, dY1, Y1, dY, r.in_rows, r.out_rows, r.prefix_host, 27, centre if want_b1 else 0,
                                         L.F_RELU_IN)
            dW1, dW2 = dWp[0].view_as(W1), dWp[1].view_as(W2)
            db1, db2 = (dbp[0], dbp[1]) if dbp is not None else (None, None)
        else:
            dW1, db1 = _param_grads(X, dY1, r, 27, W1.shape, need[1], want_b1, centre, L.F_RELU_IN)
        return dX, dW1, db1, dW2, db2, None, None


class ResidualBlockFunctionBF16(ResidualBlockFunction):
    """`ResidualBlockFunction` under the name the bf16 storage path had: it refuses anything but bf16-stored features."""

    @staticmethod
    def forward(ctx, features, *rest):
        if features.dtype != torch.bfloat16:
            raise L.ScnError("ResidualBlockFunctionBF16 takes torch.bfloat16 features")
        return ResidualBlockFunction.forward(ctx, features, *rest)


# ------------------------------------------------------------------------------------------------------
# A6 Convolution size=stride=2  (module_factory.py:232-234)
# ------------------------------------------------------------------------------------------------------
class ConvolutionFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, features, weight, bias, metadata: Metadata, in_size, relu_in=False, stride=(2, 2, 2)):
        X, W = _feat(features), _f32(weight)
        rb = metadata.strided_rulebook(in_size, stride)
        b = _f32(bias) if bias is not None else None
        if relu_in:
            _rec_relu(X)
        if USE_TILES and rb.tiles is not None:
            Y = conv_rules(X, rb.tiles, rb.n_coarse, W, b, W.shape[-1], L.F_RELU_IN if relu_in else 0,
                           n_rules=rb.n_fine)
        else:                   # (more than 27 offsets -- a 4^3 filter -- : the table-walk GEMM; fp32 rows)
            Y = gemm_table(X, rb.child, rb.n_off, rb.n_coarse, W, b, W.shape[-1], L.F_RELU_IN if relu_in else 0,
                           n_rules=rb.n_fine)
        ctx.save_for_backward(X, W)
        ctx.rb, ctx.has_bias, ctx.relu_in = rb, bias is not None, relu_in
        return Y

    @staticmethod
    def backward(ctx, dY):
        X, W = ctx.saved_tensors
        rb, r = ctx.rb, ctx.rb.rules
        dY = _feat(dY)
        fl = L.F_RELU_IN if ctx.relu_in else 0
        dX = None
        if ctx.needs_input_grad[0]:      # dX[f] = dY[parent f] . W[off f]^T : rule list with roles swapped
            dX = gemm_rules(dY, r.out_rows, r.in_rows, r.prefix_host, rb.n_off, rb.n_fine, W, None, X.shape[1],
                            L.F_W_TRANSPOSED, relu_mask=X if ctx.relu_in else None)
        # (no bias_offsets: a coarse row is named once per child, so db is always the column sum)
        dW, db = _param_grads(X, dY, r, rb.n_off, W.shape, ctx.needs_input_grad[1], ctx.has_bias and ctx.needs_input_grad[2], 0, fl)
        return dX, dW, db, None, None, None, None


# ------------------------------------------------------------------------------------------------------
# A7 Deconvolution size=stride back to the cached fine level  (module_factory.py:256-258)
# ------------------------------------------------------------------------------------------------------
class DeconvolutionFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, features, weight, bias, metadata: Metadata, out_size, relu_in=False, stride=(2, 2, 2)):
        X, W = _feat(features), _f32(weight)
        out_size = tuple(int(s) for s in out_size)
        rb = metadata.cached_strided_rulebook(out_size, stride)
        if rb is None:
            raise L.ScnError(f"Deconvolution: no cached Convolution rulebook from spatial size {out_size}; the "
                             "reference only deconvolves back to an encoder level (custom_container.py:70-83)")
        r = rb.rules
        b = _f32(bias) if bias is not None else None
        if relu_in:
            _rec_relu(X)
        Y = gemm_rules(X, r.out_rows, r.in_rows, r.prefix_host, rb.n_off, rb.n_fine, W, b, W.shape[-1],
                       L.F_RELU_IN if relu_in else 0)
        ctx.save_for_backward(X, W)
        ctx.rb, ctx.has_bias, ctx.relu_in = rb, bias is not None, relu_in
        ctx.bwd_image = packed_image(W, W.shape[-1], X.shape[1], rb.n_off, L.F_W_TRANSPOSED) if _is_bf16(X) else None
        return Y

    @staticmethod
    def backward(ctx, dY):
        X, W = ctx.saved_tensors
        rb, r = ctx.rb, ctx.rb.rules
        dY = _feat(dY)
        fl = L.F_RELU_IN if ctx.relu_in else 0
        dX = None
        if ctx.needs_input_grad[0]:      # dX[c] = sum_o dY[child[o][c]] . W[o]^T
            if USE_TILES and rb.tiles is not None:
                dX = conv_rules(dY, rb.tiles, rb.n_coarse, W, None, X.shape[1], L.F_W_TRANSPOSED,
                                relu_mask=X if ctx.relu_in else None, n_rules=rb.n_fine, image=ctx.bwd_image)
            else:
                dX = gemm_table(dY, rb.child, rb.n_off, rb.n_coarse, W, None, X.shape[1], L.F_W_TRANSPOSED,
                                relu_mask=X if ctx.relu_in else None, n_rules=rb.n_fine)
        # the Convolution's rule list with its roles swapped; every fine (output) row occurs in exactly one of the rule lists, so
        # all offsets together carry the bias pass (filters of up to 27 offsets)
        dW, db = _param_grads(X, dY, r, rb.n_off, W.shape, ctx.needs_input_grad[1], ctx.has_bias and ctx.needs_input_grad[2],
                              (1 << rb.n_off) - 1 if rb.n_off <= 27 else 0, fl, True)
        return dX, dW, db, None, None, None, None


# ------------------------------------------------------------------------------------------------------
# A9 NetworkInNetwork (module_factory.py:366-367), ReLU (:88), AddTable (:52-54,308)
# ------------------------------------------------------------------------------------------------------
class NetworkInNetworkFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, features, weight, bias):
        X, W = _feat(features), _f32(weight)
        b = _f32(bias) if bias is not None else None
        n = X.shape[0]
        Y = gemm_table(X, None, 1, n, W, b, W.shape[-1])
        ctx.save_for_backward(X, W)
        ctx.has_bias = bias is not None
        return Y

    @staticmethod
    def backward(ctx, dY):
        X, W = ctx.saved_tensors
        dY = _feat(dY)
        n = X.shape[0]
        dX = None
        if ctx.needs_input_grad[0]:
            dX = gemm_table(dY, None, 1, n, W, None, X.shape[1], L.F_W_TRANSPOSED)
        dW, db = _param_grads(X, dY, None, 1, W.shape, ctx.needs_input_grad[1], ctx.has_bias and ctx.needs_input_grad[2], 1)
        return dX, dW, db


FUSED_JOIN = True   # NetworkInNetwork over two JoinTable parts: one two-source launch (False: one GEMM per part, chained)


def gemm_rows2(X0, X1, W, bias, cout, flags=0):
    """scn_gemm_rows2 with two sources: Y = bias + [X0 | X1] . W (W is the layer's [c0 + c1][cout] weight)."""
    n, c0, c1 = X0.shape[0], X0.shape[1], X1.shape[1]
    Y = _new((n, cout), X0, X0.dtype)

    def run():
        L.check(L.lib().scn_gemm_rows2(L.ptr(X0), c0, L.ptr(X1), c1, n, L.ptr(W), L.ptr(bias), 0, 0, L.ptr(Y), cout, 0, 0,
                                       flags, int(_is_bf16(X0)), L.stream()))
    eb = X0.element_size()
    profiling.timed("k_gemm_table", 2.0 * n * (c0 + c1) * cout, eb * n * (c0 + c1 + cout) + 4.0 * (c0 + c1) * cout, run)
    return Y


def gemm_rows2_bwd(dY, W, c0, c1):
    """scn_gemm_rows2 with two destinations: dX0 = dY . W[:c0]^T, dX1 = dY . W[c0:]^T from one read of dY."""
    n, cout = dY.shape
    d0, d1 = _new((n, c0), dY, dY.dtype), _new((n, c1), dY, dY.dtype)

    def run():
        L.check(L.lib().scn_gemm_rows2(L.ptr(dY), cout, 0, 0, n, L.ptr(W), 0, 0, 0, L.ptr(d0), c0, L.ptr(d1), c1,
                                       L.F_W_TRANSPOSED, int(_is_bf16(dY)), L.stream()))
    eb = dY.element_size()
    profiling.timed("k_gemm_table", 2.0 * n * (c0 + c1) * cout, eb * n * (c0 + c1 + cout) + 4.0 * (c0 + c1) * cout, run)
    return d0, d1


class JoinedNetworkInNetworkFunction(torch.autograd.Function):
    """NetworkInNetwork over a JoinTable without the concatenated slab: Y = b + sum_k X_k . W[rows of part k].
    Two parts in 8-channel groups (every decoder level): ONE launch reads both slabs (scn_gemm_rows2) and one launch writes
    both gradients.  Otherwise one identity-table GEMM per part, the running sum carried through the kernel's residual
    operand, and dX_k = dY . W[rows k]^T per part.  dW[rows k] = X_k^T dY (db with the first)."""

    @staticmethod
    def forward(ctx, weight, bias, *parts):
        W = _f32(weight)
        b = _f32(bias) if bias is not None else None
        Xs = [_feat(p) for p in parts]
        n, cout = Xs[0].shape[0], W.shape[-1]
        if sum(X.shape[1] for X in Xs) != W.shape[0]:
            raise L.ScnError("JoinTable parts do not add up to the NetworkInNetwork's input width")
        c0, c1 = (Xs[0].shape[1], Xs[1].shape[1]) if len(Xs) == 2 else (0, 0)
        ctx.fused = (FUSED_JOIN and len(Xs) == 2 and Xs[0].dtype == Xs[1].dtype and c0 >= 8 and c1 >= 8 and c0 % 8 == 0
                     and c1 % 8 == 0 and n > 0)
        if ctx.fused:
            y = gemm_rows2(Xs[0], Xs[1], W, b, cout)
        else:
            y, r0 = None, 0
            for k, X in enumerate(Xs):
                c = X.shape[1]
                y = gemm_table(X, None, 1, n, W[r0:r0 + c], b if k == 0 else None, cout, residual=y)
                r0 += c
        ctx.save_for_backward(W, *Xs)
        ctx.has_bias = bias is not None
        return y

    @staticmethod
    def backward(ctx, dY):
        W, *Xs = ctx.saved_tensors
        dY = _feat(dY)
        n = dY.shape[0]
        need = ctx.needs_input_grad
        dW = torch.empty_like(W) if need[0] else None
        db, dXs, r0 = None, [], 0
        if ctx.fused and need[2] and need[3] and dY.shape[1] % 8 == 0:       # (the kernel stages dY in 8-channel groups)
            dXs = list(gemm_rows2_bwd(dY, W, Xs[0].shape[1], Xs[1].shape[1]))
        for k, X in enumerate(Xs):
            c = X.shape[1]
            if len(dXs) <= k:
                dXs.append(gemm_table(dY, None, 1, n, W[r0:r0 + c], None, c, L.F_W_TRANSPOSED) if need[2 + k] else None)
            if need[0]:                 # (db in the first part's pass)
                dW[r0:r0 + c], dbk = _param_grads(X, dY, None, 1, (c, -1), True, k == 0 and ctx.has_bias and need[1], 1)
                db = dbk if k == 0 else db
            r0 += c
        if db is None and ctx.has_bias and need[1]:
            db = colsum(dY)
        return (dW, db, *dXs)


class ReLUFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, features):
        """fp32, or a bf16-STORED slab (scn_relu_fwd_bf16 / _bwd_bf16: result and gradient stay bf16, and widening either gives
        the fp32 function's result on the widened input bit for bit)."""
        X = _feat(features)
        _rec_relu(X)
        Y = torch.empty_like(X)
        fwd = L.lib().scn_relu_fwd_bf16 if _is_bf16(X) else L.lib().scn_relu_fwd
        L.check(fwd(L.ptr(X), X.numel(), L.ptr(Y), L.stream()))
        ctx.save_for_backward(X)
        return Y

    @staticmethod
    def backward(ctx, dY):
        (X,) = ctx.saved_tensors
        dX = torch.empty_like(X)
        if _is_bf16(X):
            dY = dY.to(torch.bfloat16).contiguous()
            L.check(L.lib().scn_relu_bwd_bf16(L.ptr(X), L.ptr(dY), X.numel(), L.ptr(dX), L.stream()))
            return dX
        dY = _f32(dY)
        L.check(L.lib().scn_relu_bwd(L.ptr(X), L.ptr(dY), X.numel(), L.ptr(dX), L.stream()))
        return dX


class AddFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a, b):
        A, B = _f32(a), _f32(b)
        if A.shape != B.shape:
            raise ValueError("AddTable: shape mismatch")
        Y = torch.empty_like(A)
        L.check(L.lib().scn_add(L.ptr(A), L.ptr(B), A.numel(), L.ptr(Y), L.stream()))
        return Y

    @staticmethod
    def backward(ctx, dY):
        return dY, dY


class AddStoredFunction(torch.autograd.Function):
    """AddTable on two bf16-STORED slabs (modules.AddTable(stored=True)): scn_add_bf16, the result stays stored."""

    @staticmethod
    def forward(ctx, a, b):
        A, B = _feat(a), _feat(b)
        if A.shape != B.shape or not (_is_bf16(A) and _is_bf16(B)):
            raise ValueError("AddTable(stored): two bf16 slabs of one shape required")
        Y = torch.empty_like(A)
        L.check(L.lib().scn_add_bf16(L.ptr(A), L.ptr(B), A.numel(), L.ptr(Y), L.stream()))
        return Y

    @staticmethod
    def backward(ctx, dY):
        return dY, dY


# ------------------------------------------------------------------------------------------------------
# A8 BatchNorm(Leaky)ReLU (module_factory.py:92-102)
# ------------------------------------------------------------------------------------------------------
def _sync_group(sync):
    """The process group SyncBN reduces over, or None (single process / not requested)."""
    import torch.distributed as dist
    if not sync or not (dist.is_available() and dist.is_initialized()) or dist.get_world_size() < 2:
        return None
    return dist.group.WORLD


class BatchNormReLUFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, features, weight, bias, running_mean, running_var, eps, momentum, leak, training, sync=False):
        lib = L.lib()
        X = _f32(features)
        n, c = X.shape
        g, b = _f32(weight), _f32(bias)
        if not (g.numel() == b.numel() == running_mean.numel() == running_var.numel() == c):
            # a channel-padded slab (modules._ConvBase.pad_out_to) is wider than the layer: the kernels would normalise the
            # pad columns with statistics and parameters read past the layer's, and the pad would stop being zero
            raise ValueError(f"batch norm over a {c}-column slab with {g.numel()} planes: the slab must be exactly as wide "
                             "as the layer (no channel padding)")
        scratch = torch.empty(lib.scn_bn_scratch_bytes(c), dtype=torch.uint8, device=X.device)
        group = _sync_group(sync) if training else None
        n_stat = n
        if group is not None:
            # batch statistics over the scenes of ALL ranks (module_factory.py:92-102: one feature matrix per batch):
            # one all-reduce of (sum x, sum x^2, rows) per layer, float64
            import torch.distributed as dist
            pack = torch.empty(2 * c + 1, dtype=torch.float64, device=X.device)
            L.check(lib.scn_bn_sums(L.ptr(X), n, c, L.ptr(pack), L.ptr(scratch), L.stream()))
            pack[2 * c] = float(n)
            dist.all_reduce(pack, group=group)
            n_stat = int(round(pack[2 * c].item()))
            mu = pack[:c] / max(n_stat, 1)
            mean = mu.float()
            var = (pack[c:2 * c] / max(n_stat, 1) - mu * mu).clamp_(min=0).float()
            running_mean.mul_(momentum).add_(mean, alpha=1 - momentum)
            running_var.mul_(momentum).add_(var, alpha=(1 - momentum) * (n_stat / (n_stat - 1) if n_stat > 1 else 1.0))
        elif training:
            mean, var = _new((c,), X), _new((c,), X)
            L.check(lib.scn_bn_stats(L.ptr(X), n, c, L.ptr(mean), L.ptr(var), L.ptr(scratch), L.stream()))
            # momentum is the RETAIN fraction (SparseConvNet convention; SURVEY.md §4.1 caveat).  The running variance
            # takes the UNBIASED batch estimate (sum of squared differences / (n - 1)), the normalisation the biased
            # one -- SparseConvNet's BatchNormalization forward as recalled [UPSTREAM-SCN], and torch.nn.BatchNorm's
            # convention too; n = 1 keeps the (zero) biased value instead of dividing by zero
            running_mean.mul_(momentum).add_(mean, alpha=1 - momentum)
            running_var.mul_(momentum).add_(var, alpha=(1 - momentum) * (n / (n - 1) if n > 1 else 1.0))
        else:
            mean, var = _f32(running_mean), _f32(running_var)
        Y = torch.empty_like(X)
        L.check(lib.scn_bn_fwd(L.ptr(X), n, c, L.ptr(mean), L.ptr(var), eps, L.ptr(g), L.ptr(b), leak, L.ptr(Y),
                               L.stream()))
        # the layer's ReLU decisions for RELU_RECORD: Y > 0 exactly where the normalised pre-activation the kernels compute
        # (forward and backward alike: ((x - mean) * rsqrt(var + eps)) * gamma + beta) is > 0 -- leak * pre is never > 0
        _rec_relu(Y)
        ctx.save_for_backward(X, g, b, mean, var)
        ctx.cfg = (eps, leak, training)
        ctx.sync = (group, n_stat)
        return Y

    @staticmethod
    def backward(ctx, dY):
        lib = L.lib()
        X, g, b, mean, var = ctx.saved_tensors
        eps, leak, training = ctx.cfg
        dY = _f32(dY)
        n, c = X.shape
        scratch = torch.empty(lib.scn_bn_scratch_bytes(c), dtype=torch.uint8, device=X.device)
        dX, dg, db = torch.empty_like(X), _new((c,), X), _new((c,), X)
        group, n_stat = ctx.sync
        if group is not None:
            # (sum g, sum g x^) over all ranks; dgamma / dbeta stay this rank's share (the gradient all-reduce adds them)
            import torch.distributed as dist
            sums = torch.empty(2 * c, dtype=torch.float64, device=X.device)
            L.check(lib.scn_bn_bwd_reduce(L.ptr(X), L.ptr(dY), n, c, L.ptr(mean), L.ptr(var), eps, L.ptr(g), L.ptr(b), leak,
                                          L.ptr(dg), L.ptr(db), L.ptr(sums), L.ptr(scratch), L.stream()))
            dist.all_reduce(sums, group=group)
            L.check(lib.scn_bn_bwd_apply(L.ptr(X), L.ptr(dY), n, c, L.ptr(mean), L.ptr(var), eps, L.ptr(g), L.ptr(b), leak,
                                         L.ptr(sums), n_stat, L.ptr(dX), L.stream()))
            return dX, dg, db, None, None, None, None, None, None, None
        L.check(lib.scn_bn_bwd(L.ptr(X), L.ptr(dY), n, c, L.ptr(mean), L.ptr(var), eps, L.ptr(g), L.ptr(b), leak,
                               1 if training else 0, L.ptr(dX), L.ptr(dg), L.ptr(db), L.ptr(scratch), L.stream()))
        return dX, dg, db, None, None, None, None, None, None, None


# ------------------------------------------------------------------------------------------------------
# A3 / A10 ioLayers  (custom_operations.py:7-10, 67-86; roi_select_sparse.py:79-81,117-119)
# ------------------------------------------------------------------------------------------------------
class InputLayerFunction(torch.autograd.Function):
    """``scn.ioLayers.InputLayerFunction.apply(dimension, metadata, spatial_size, coords, features, batch_size, mode)``"""

    @staticmethod
    def forward(ctx, dimension, metadata, spatial_size, coords, input_features, batch_size, mode):
        lib = L.lib()
        if int(dimension) != 3:
            raise NotImplementedError("only dimension 3")
        mode = int(mode)
        dev = torch.device("cuda", torch.cuda.current_device())
        F = input_features.to(dev)
        if F.dtype == torch.bfloat16:           # bf16-stored point features (the ROI crop of a bf16 slab): widened exactly;
            F = F.float()                       # the mean over a voxel's points accumulates in fp32 / fp64
        F = _f32(F)
        if coords.shape[0] != F.shape[0]:
            raise ValueError("coords / features row mismatch")
        if metadata.input_size is None:
            grid = metadata.set_input(spatial_size, coords, int(batch_size), mode)
        else:                                   # prepared ahead of time (Metadata.prepare_async) for these coords
            if metadata.n_items != coords.shape[0] or metadata.input_size != tuple(int(s) for s in spatial_size):
                raise L.ScnError("InputLayer: this Metadata was prepared for different coordinates")
            metadata.handover()
            if not metadata.prepared_for(coords):        # same point count, other coordinates (fixed-size sampling)
                raise L.ScnError("InputLayer: this Metadata was prepared for different coordinates")
            grid = metadata.grid(metadata.input_size)
        n_items, c = F.shape
        Y = _new((grid.n, c), F)
        acc = torch.empty((grid.n, c), dtype=torch.float64, device=dev) if mode in (3, 4) else None
        if mode == 1:
            metadata.row_last = torch.empty(grid.n, dtype=torch.int32, device=dev)
        L.check(lib.scn_input_fwd(L.ptr(F), L.ptr(metadata.item_row), L.ptr(metadata.row_count),
                                  L.ptr(metadata.row_first), n_items, grid.n, c, mode, L.ptr(Y), L.ptr(acc),
                                  L.ptr(metadata.row_last), L.stream()))
        ctx.md, ctx.mode, ctx.shape, ctx.in_device, ctx.in_dtype = metadata, mode, (n_items, c), input_features.device, \
            input_features.dtype
        return Y

    @staticmethod
    def backward(ctx, dY):
        md = ctx.md
        dY = _f32(dY)
        n_items, c = ctx.shape
        dF = _new((n_items, c), dY)
        L.check(L.lib().scn_input_bwd(L.ptr(dY), L.ptr(md.item_row), L.ptr(md.row_count), L.ptr(md.row_first),
                                      L.ptr(md.row_last), n_items, c, ctx.mode, L.ptr(dF), L.stream()))
        return None, None, None, None, dF.to(device=ctx.in_device, dtype=ctx.in_dtype), None, None


class OutputLayerFunction(torch.autograd.Function):
    """``scn.ioLayers.OutputLayerFunction.apply(dimension, metadata, features)`` -> one row per ORIGINAL input point."""

    @staticmethod
    def forward(ctx, dimension, metadata, input_features):
        X = _feat(input_features)               # fp32, or bf16 storage (a row copy either way)
        if metadata.item_row is None:
            raise L.ScnError("OutputLayer: this Metadata has no InputLayer rules")
        c = X.shape[1]
        Y = _new((metadata.n_items, c), X, X.dtype)
        gather = L.lib().scn_gather_rows_bf16 if _is_bf16(X) else L.lib().scn_gather_rows
        L.check(gather(L.ptr(X), L.ptr(metadata.item_row), metadata.n_items, c, L.ptr(Y), L.stream()))
        ctx.md, ctx.n_rows, ctx.hb = metadata, X.shape[0], _is_bf16(X)
        return Y

    @staticmethod
    def backward(ctx, dY):
        md = ctx.md
        dY = dY.to(torch.bfloat16).contiguous() if ctx.hb else _f32(dY)
        c = dY.shape[1]
        dX = _new((ctx.n_rows, c), dY, dY.dtype)
        acc = torch.empty((ctx.n_rows, c), dtype=torch.float64, device=dY.device)
        seg = L.lib().scn_segment_sum_bf16 if ctx.hb else L.lib().scn_segment_sum
        L.check(seg(L.ptr(dY), L.ptr(md.item_row), md.n_items, ctx.n_rows, c, L.ptr(dX), L.ptr(acc), L.stream()))
        return None, None, dX


# ------------------------------------------------------------------------------------------------------
# A13 SparseToDense (module_factory.py:429-435)
# ------------------------------------------------------------------------------------------------------
class SparseToDenseFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, features, metadata, spatial_size):
        X = _feat(features)                     # fp32, or bf16 storage (the dense volume then is bf16 too)
        size = tuple(int(s) for s in spatial_size)
        g = metadata.grid(size)
        n, c = X.shape
        out = torch.zeros((metadata.n_samples, c) + size, dtype=X.dtype, device=X.device)
        hs = L.host_i64(3)
        hs[0], hs[1], hs[2] = size
        fwd = L.lib().scn_sparse_to_dense_fwd_bf16 if _is_bf16(X) else L.lib().scn_sparse_to_dense_fwd
        L.check(fwd(L.ptr(X), L.ptr(g.coords), n, c, hs, L.ptr(out), L.stream()))
        ctx.g, ctx.size, ctx.shape, ctx.hb = g, size, (n, c), _is_bf16(X)
        return out

    @staticmethod
    def backward(ctx, dOut):
        dOut = dOut.to(torch.bfloat16).contiguous() if ctx.hb else _f32(dOut)
        n, c = ctx.shape
        dX = _new((n, c), dOut, dOut.dtype)
        hs = L.host_i64(3)
        hs[0], hs[1], hs[2] = ctx.size
        bwd = L.lib().scn_sparse_to_dense_bwd_bf16 if ctx.hb else L.lib().scn_sparse_to_dense_bwd
        L.check(bwd(L.ptr(dOut), L.ptr(ctx.g.coords), n, c, hs, L.ptr(dX), L.stream()))
        return dX, None, None


# ------------------------------------------------------------------------------------------------------
# MaxPooling / AveragePooling 2^3 stride 2 (module_factory.py:315-354)
# ------------------------------------------------------------------------------------------------------
class PoolingFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, features, metadata: Metadata, in_size, average, stride=(2, 2, 2)):
        X = _feat(features)                     # fp32, or bf16 storage
        rb = metadata.strided_rulebook(in_size, stride)
        c = X.shape[1]
        Y = _new((rb.n_coarse, c), X, X.dtype)
        mode = int(bool(average)) | ((rb.n_off << 8) if rb.n_off != 8 else 0)     # pool volume above bit 8 (0: the 2^3 default)
        fwd = L.lib().scn_pool_fwd_bf16 if _is_bf16(X) else L.lib().scn_pool_fwd
        L.check(fwd(L.ptr(X), L.ptr(rb.child), rb.n_coarse, c, mode, L.ptr(Y), L.stream()))
        ctx.save_for_backward(X, Y)
        ctx.rb, ctx.average = rb, mode
        return Y

    @staticmethod
    def backward(ctx, dY):
        X, Y = ctx.saved_tensors
        hb = _is_bf16(X)
        dY = dY.to(torch.bfloat16).contiguous() if hb else _f32(dY)
        dX = torch.empty_like(X)
        bwd = L.lib().scn_pool_bwd_bf16 if hb else L.lib().scn_pool_bwd
        L.check(bwd(L.ptr(X), L.ptr(Y), L.ptr(dY), L.ptr(ctx.rb.parent), X.shape[0], X.shape[1], ctx.average, L.ptr(dX),
                    L.stream()))
        return dX, None, None, None, None


# ------------------------------------------------------------------------------------------------------
# Dense RoiAlign + the unclamped dense max pool behind it (roi_select_dense.py:28-141; nn.MaxPool3d(2); scn_roialign.hip)
# ------------------------------------------------------------------------------------------------------
def _host3(v):
    h = L.host_i64(3)
    h[0], h[1], h[2] = (int(s) for s in v)
    return h


def _slab16(features, what):
    """The slab of the two dense operators: fp32, or bf16 STORAGE -- 16-byte lanes of 8 channels, so a bf16 slab's width is a
    multiple of 8 (modules.py stores no other width in bf16)."""
    X = _feat(features)
    if _is_bf16(X) and X.shape[1] % 8:
        raise ValueError(f"{what}: a bf16-stored slab needs a width that is a multiple of 8, got {X.shape[1]}")
    return X


class RoiAlignFunction(torch.autograd.Function):
    """forward(F [B X Y Z, C] channels-last slab, boxes fp32 [R, 2, 3] transformed and clipped to the volume (cells),
    sample_of_box int32 [R] ascending, batch, size (X, Y, Z), extract (ex, ey, ez)) -> [R ex ey ez, C], the slab of the fully
    active grid `extract` with batch R.  The backward is the library's ordered gather (no atomics): dF covers every cell.
    A bf16-stored slab (C a multiple of 8) gives a bf16 slab and a bf16 dF: the fp32 arithmetic on exactly widened values,
    rounded once at the store; boxes and the table are the same."""

    @staticmethod
    def forward(ctx, features, boxes, sample_of_box, batch, size, extract):
        X = _slab16(features, "RoiAlign")
        hb = _is_bf16(X)
        size, extract = tuple(int(s) for s in size), tuple(int(s) for s in extract)
        batch, r, c = int(batch), int(boxes.shape[0]), X.shape[1]
        if X.shape[0] != batch * size[0] * size[1] * size[2]:
            raise ValueError(f"RoiAlign: {X.shape[0]} rows are not a [{batch}, {size[0]}, {size[1]}, {size[2]}] volume")
        if tuple(boxes.shape) != (r, 2, 3) or sample_of_box.shape[0] != r or sample_of_box.dtype != torch.int32:
            raise ValueError("RoiAlign: boxes fp32 [R, 2, 3] and sample_of_box int32 [R] required")
        boxes = _f32(boxes)
        out = _new((r * extract[0] * extract[1] * extract[2], c), X, X.dtype)
        table = torch.empty(max(r, 1) * (3 * sum(extract) + 2 * sum(size)), dtype=torch.int32, device=X.device)
        fwd = L.lib().scn_roialign_fwd_bf16 if hb else L.lib().scn_roialign_fwd
        L.check(fwd(L.ptr(X), batch, _host3(size), c, L.ptr(boxes), L.ptr(sample_of_box), r, _host3(extract), L.ptr(table),
                    L.ptr(out), L.stream()))
        ctx.save_for_backward(table, sample_of_box)
        ctx.cfg = (batch, size, extract, r, c, hb)
        return out

    @staticmethod
    def backward(ctx, dOut):
        table, sample_of_box = ctx.saved_tensors
        batch, size, extract, r, c, hb = ctx.cfg
        dOut = dOut.to(torch.bfloat16).contiguous() if hb else _f32(dOut)
        dF = _new((batch * size[0] * size[1] * size[2], c), dOut, dOut.dtype)
        bwd = L.lib().scn_roialign_bwd_bf16 if hb else L.lib().scn_roialign_bwd
        L.check(bwd(L.ptr(dOut), L.ptr(table), L.ptr(sample_of_box), r, batch, _host3(size), c, _host3(extract), L.ptr(dF),
                    L.stream()))
        return dF, None, None, None, None, None


class DenseMaxPoolFunction(torch.autograd.Function):
    """forward(X [R ex ey ez, C], n_boxes R, extent (ex, ey, ez) even, pad_boxes=0) -> [max(R, pad_boxes) ex/2 ey/2 ez/2, C]:
    the plain maximum of the 8 children (no clamp at 0, the first child on a tie: nn.MaxPool3d(2)); the rows of the boxes
    R .. pad_boxes - 1 are zero and take no gradient (the class branch's box-count bucket).  fp32, or a bf16-stored slab (C a
    multiple of 8) in and out: the maximum of bf16 values is one of them, so nothing is rounded."""

    @staticmethod
    def forward(ctx, features, n_boxes, extent, pad_boxes=0):
        X = _slab16(features, "DenseMaxPool")
        hb = _is_bf16(X)
        extent = tuple(int(s) for s in extent)
        r, c = int(n_boxes), X.shape[1]
        if any(e % 2 or e < 2 for e in extent):
            raise ValueError(f"DenseMaxPool: even extents required, got {extent}")
        if X.shape[0] != r * extent[0] * extent[1] * extent[2]:
            raise ValueError(f"DenseMaxPool: {X.shape[0]} rows are not {r} boxes of {extent}")
        per = (extent[0] // 2) * (extent[1] // 2) * (extent[2] // 2)
        rows = max(r, int(pad_boxes)) * per
        Y = _new((rows, c), X, X.dtype)
        arg = torch.empty((r * per, c), dtype=torch.uint8, device=X.device)
        fwd = L.lib().scn_dense_maxpool_fwd_bf16 if hb else L.lib().scn_dense_maxpool_fwd
        L.check(fwd(L.ptr(X), r, _host3(extent), c, L.ptr(Y), L.ptr(arg), L.stream()))
        if rows > r * per:
            Y[r * per:].zero_()
        ctx.save_for_backward(arg)
        ctx.cfg = (r, extent, c, per, hb)
        return Y

    @staticmethod
    def backward(ctx, dY):
        (arg,) = ctx.saved_tensors
        r, extent, c, per, hb = ctx.cfg
        dY = dY.to(torch.bfloat16).contiguous() if hb else _f32(dY)
        dX = _new((r * per * 8, c), dY, dY.dtype)
        bwd = L.lib().scn_dense_maxpool_bwd_bf16 if hb else L.lib().scn_dense_maxpool_bwd
        L.check(bwd(L.ptr(dY), L.ptr(arg), r, _host3(extent), c, L.ptr(dX), L.stream()))
        return dX, None, None, None


class RoiAlignPoolFunction(torch.autograd.Function):
    """RoiAlignFunction then DenseMaxPoolFunction in one pass (scn_roialign_pool_fwd / _bwd): forward(F [B X Y Z, C], boxes,
    sample_of_box, batch, size, extract (even), pad_boxes=0) -> [max(R, pad_boxes) ex/2 ey/2 ez/2, C].  The forward equals the
    pair bit for bit, the backward as numbers; the [R ex ey ez, C] samples and their gradient are never written.  The rows of
    the boxes R .. pad_boxes - 1 are zero and take no gradient, as in DenseMaxPoolFunction.  fp32 or a bf16-stored slab."""

    @staticmethod
    def forward(ctx, features, boxes, sample_of_box, batch, size, extract, pad_boxes=0):
        X = _slab16(features, "RoiAlignPool")
        hb = _is_bf16(X)
        size, extract = tuple(int(s) for s in size), tuple(int(s) for s in extract)
        batch, r, c = int(batch), int(boxes.shape[0]), X.shape[1]
        if any(e % 2 or e < 2 for e in extract):
            raise ValueError(f"RoiAlignPool: even extents required, got {extract}")
        if X.shape[0] != batch * size[0] * size[1] * size[2]:
            raise ValueError(f"RoiAlignPool: {X.shape[0]} rows are not a [{batch}, {size[0]}, {size[1]}, {size[2]}] volume")
        if tuple(boxes.shape) != (r, 2, 3) or sample_of_box.shape[0] != r or sample_of_box.dtype != torch.int32:
            raise ValueError("RoiAlignPool: boxes fp32 [R, 2, 3] and sample_of_box int32 [R] required")
        boxes = _f32(boxes)
        per = (extract[0] // 2) * (extract[1] // 2) * (extract[2] // 2)
        rows = max(r, int(pad_boxes)) * per
        Y = _new((rows, c), X, X.dtype)
        arg = torch.empty((r * per, c), dtype=torch.uint8, device=X.device)
        table = torch.empty(max(r, 1) * (3 * sum(extract) + 2 * sum(size)), dtype=torch.int32, device=X.device)
        fwd = L.lib().scn_roialign_pool_fwd_bf16 if hb else L.lib().scn_roialign_pool_fwd
        L.check(fwd(L.ptr(X), batch, _host3(size), c, L.ptr(boxes), L.ptr(sample_of_box), r, _host3(extract), L.ptr(table),
                    L.ptr(Y), L.ptr(arg), L.stream()))
        if rows > r * per:
            Y[r * per:].zero_()
        ctx.save_for_backward(table, sample_of_box, arg)
        ctx.cfg = (batch, size, extract, r, c, per, hb)
        return Y

    @staticmethod
    def backward(ctx, dY):
        table, sample_of_box, arg = ctx.saved_tensors
        batch, size, extract, r, c, per, hb = ctx.cfg
        dY = dY.to(torch.bfloat16).contiguous() if hb else _f32(dY)          # (the padding boxes' rows lie behind r * per)
        dF = _new((batch * size[0] * size[1] * size[2], c), dY, dY.dtype)
        bwd = L.lib().scn_roialign_pool_bwd_bf16 if hb else L.lib().scn_roialign_pool_bwd
        L.check(bwd(L.ptr(dY), L.ptr(arg), L.ptr(table), L.ptr(sample_of_box), r, batch, _host3(size), c, _host3(extract),
                    L.ptr(dF), L.stream()))
        return dF, None, None, None, None, None, None


class BoxFlattenFunction(torch.autograd.Function):
    """forward(X fp32 [R V, C], n_boxes R, relu=False) -> [R, C V], channel-major (column ch V + s: the reference's
    `Reshaper` on [R, C, x, y, z]), with the ReLU that follows it folded in when `relu` (scn_box_flatten_fwd / _bwd)."""

    @staticmethod
    def forward(ctx, features, n_boxes, relu=False):
        X = _f32(_feat(features))
        r, c = int(n_boxes), X.shape[1]
        if r < 0 or (r == 0 and X.shape[0]) or (r and X.shape[0] % r):
            raise ValueError(f"BoxFlatten: {X.shape[0]} rows are not {r} boxes")
        v = X.shape[0] // r if r else 1
        Y = _new((r, c * v), X)
        L.check(L.lib().scn_box_flatten_fwd(L.ptr(X), r, v, c, int(bool(relu)), L.ptr(Y), L.stream()))
        ctx.save_for_backward(X if relu else None)
        ctx.cfg = (r, v, c, bool(relu))
        return Y

    @staticmethod
    def backward(ctx, dY):
        (X,) = ctx.saved_tensors
        r, v, c, relu = ctx.cfg
        dY = _f32(dY)
        dX = _new((r * v, c), dY)
        L.check(L.lib().scn_box_flatten_bwd(L.ptr(X) if relu else None, L.ptr(dY), r, v, c, int(relu), L.ptr(dX), L.stream()))
        return dX, None, None


# ------------------------------------------------------------------------------------------------------
# The permutation half of the reference's up-sampling RPN heads (anchor_network.py:127-219; scn_anchor_up.hip)
# ------------------------------------------------------------------------------------------------------
class AnchorUpFunction(torch.autograd.Function):
    """forward(plan, batch, P_0, ..., P_{L-1}) -> (rpn_bbox [B, N_in, 2, 3], rpn_score [B, N_in]) over the inside anchors of all
    levels: P_l [B X_l Y_l Z_l, Ncol_l] is level l's slab times its packed head weights; one scn_anchor_up_fwd per level writes
    the level's records straight into the two outputs (every inside anchor belongs to exactly one level).  `plan`
    (rpn.AnchorNetworkUpsample builds and keeps it per scene shape): .n_all, .n_inside, .dest int32 [n_all] on the
    device, .levels = [(size (X, Y, Z), ncol, group table int64 [G][6] on the host, G)].  The backward is one
    scn_anchor_up_bwd per level: dP_l written once everywhere, 0 at the anchors outside the scene, an absent gradient is zeros."""

    @staticmethod
    def forward(ctx, plan, batch, *Ps):
        if len(Ps) != len(plan.levels):
            raise ValueError(f"AnchorUp: {len(plan.levels)} levels planned, {len(Ps)} given")
        Ps = [_f32(P) for P in Ps]
        B = int(batch)
        for P, (size, ncol, _, _) in zip(Ps, plan.levels):
            if tuple(P.shape) != (B * size[0] * size[1] * size[2], ncol):
                raise ValueError(f"AnchorUp: P {tuple(P.shape)} is not [{B} x {size[0]} x {size[1]} x {size[2]}, {ncol}]")
        if plan.dest.dtype != torch.int32 or plan.dest.shape[0] != plan.n_all or plan.dest.device != Ps[0].device:
            raise ValueError("AnchorUp: dest int32 [n_all] on the slabs' device required")
        rpn_bbox = _new((B, plan.n_inside, 2, 3), Ps[0])
        rpn_score = _new((B, plan.n_inside), Ps[0])
        for P, (size, ncol, groups, n_groups) in zip(Ps, plan.levels):
            L.check(L.lib().scn_anchor_up_fwd(L.ptr(P), B, _host3(size), ncol, groups, n_groups, L.ptr(plan.dest), plan.n_all,
                                              plan.n_inside, L.ptr(rpn_bbox), L.ptr(rpn_score), L.stream()))
        ctx.plan, ctx.batch = plan, B
        ctx.set_materialize_grads(False)
        return rpn_bbox, rpn_score

    @staticmethod
    def backward(ctx, d_bbox, d_score):
        plan = ctx.plan
        d_bbox = None if d_bbox is None else _f32(d_bbox)
        d_score = None if d_score is None else _f32(d_score)
        B = ctx.batch
        out = []
        for i, (size, ncol, groups, n_groups) in enumerate(plan.levels):
            if not ctx.needs_input_grad[2 + i]:
                out.append(None)
                continue
            dP = torch.empty((B * size[0] * size[1] * size[2], ncol), dtype=torch.float32, device=plan.dest.device)
            L.check(L.lib().scn_anchor_up_bwd(L.ptr(d_bbox), L.ptr(d_score), B, _host3(size), ncol, groups, n_groups,
                                              L.ptr(plan.dest), plan.n_all, plan.n_inside, L.ptr(dP), L.stream()))
            out.append(dP)
        return (None, None, *out)
