"""Host side of the step executor (csrc/scn_exec.hip, include/scn_mi355x.h "Step executor").

The reference drives the scn surface one layer at a time from Python (module_factory.py builds nested scn.Sequential trees,
model.py:414-431 / 758-782 run them), and so did this package's autograd functions: ~330 launches per backbone step, ~760
with the mask branch, ~13 us of host time each.  Here a U-Net LEVEL runs as one autograd node whose forward and backward are
one C call each: the node's launch plan (a flat list of `scn_exec_op`) is compiled ONCE per network from the module tree,
and a step only fills three pointer tables (feature slabs carved out of one workspace tensor, parameters / bf16 weight
images, parameter gradients).  Every op is one of the library's own entry points with the arguments the layer-by-layer
path passes, so both paths produce the same bits (tests/test_gpu_exec.py).

One node per LEVEL rather than per network: the parameter gradients of a level leave its node when that level's backward
ends, so the bucketed gradient all-reduce of dp.py still overlaps with the rest of backward, skip connections stay ordinary
autograd edges, and the encoder outputs (`SparseUNet.interims`, the RPN's inputs in the reference) stay differentiable.

Units: the plain pre-activation residual unit, the reference's bottleneck / main-path-ReLU forms, its post-activation units
(relu_first=False) and its plain convolution blocks (use_residuals=False) (`_unit_blocks`); input stages with the ReLU in front
of the layer, behind it, or dropped (`_stage_relus`).  Batch-norm networks (`SparseUNet(batchnorm=True, bn_stages=True)`, or
SCN_EXEC_BN=1): every one of those units and input stages with BatchNorm(Leaky)ReLU where the ReLU stood (`_bn_blocks`).  A
batch-norm activation is never folded into the consuming convolution: it is SCN_OP_BN_STATS + SCN_OP_BN_FWD writing a slab
of its own, SCN_OP_BN_BWD on the way back; its batch mean / variance live in the stage workspace and the host applies the
running-statistics update after the forward call (`run_stage`), with the statements functional.BatchNormReLUFunction uses.

Not covered (the layer-by-layer path runs instead): batch norm without `bn_stages`, `bf16_blocks=True` (casts around every
run of units), channel plans the two-source NetworkInNetwork kernel does not take, empty levels, and any step in which
`profiling.TIMER` brackets single launches with events.  A batch-norm network also steps aside while `modules._BatchNorm.SYNC`
is on with an initialised process group (the all-reduce sits between two kernels of a layer), while
`functional.RELU_RECORD` records activation masks, and when its batch-norm layers are not all in the network's own
training / evaluation mode.
"""
from __future__ import annotations

import contextlib
import ctypes as C
import os
import struct
import threading

import torch

from . import _lib as L
from . import functional as F
from . import modules as M

ENABLED = os.environ.get("SCN_EXEC", "1") != "0"
# parameter-gradient ops of a backward pass on a second stream beside the backward-data chain (scn_exec_run_streams)
SIDE_LEAVES = os.environ.get("SCN_EXEC_SIDE", "0") != "0"
# developer switch: batch-norm networks built WITHOUT `bn_stages=True` compile stage plans too (A/B of an unmodified bench.py)
BN_STAGES = os.environ.get("SCN_EXEC_BN", "0") != "0"
_side_streams, _side_scratch = {}, {}

i32, i64, vp = C.c_int32, C.c_int64, C.c_void_p

OP_GEMM_IDENT, OP_CONV_SUBM, OP_CONV_CHILD, OP_RULES_CHILD, OP_ROWS2 = 1, 2, 3, 4, 5
OP_WGRAD_SUBM, OP_WGRAD2_SUBM, OP_WGRAD_DOWN, OP_WGRAD_UP, OP_WGRAD_IDENT, OP_COLSUM, OP_ADD, OP_CAST = 6, 7, 8, 9, 10, 11, 12, 13
OP_RELU, OP_RELU_BWD, OP_ADD_RELU = 14, 15, 16
OP_BN_STATS, OP_BN_FWD, OP_BN_BWD = 17, 18, 19
XF_BF16, XF_COARSE_ROWS, XF_BN_TRAINING = 1 << 16, 1 << 17, 1 << 18
VEC = -1                                # `level` of a buffer that is one row whatever the level sizes are (batch mean | variance)
BACK = L.F_W_TRANSPOSED | L.F_OFF_REVERSE


class ExecOp(C.Structure):
    _fields_ = [(n, i32) for n in ("op", "flags", "level", "cin", "cout", "x", "y", "r", "m", "x1", "y1", "c1", "w", "b", "aux",
                                   "reserved")]


class ExecLevel(C.Structure):
    _fields_ = [("n", i64), ("tstab", vp), ("tile_mask", vp), ("perm", vp), ("tile_order", vp), ("in_rows", vp),
                ("out_rows", vp), ("prefix_host", vp), ("n_coarse", i64), ("c_tstab", vp), ("c_tile_mask", vp),
                ("c_perm", vp), ("c_tile_order", vp), ("c_in_rows", vp), ("c_out_rows", vp), ("c_prefix_host", vp),
                ("flags", i64)]


def _addr(prefix_host):
    return C.cast(prefix_host, vp).value


def _f32_bits(v):
    """The int32 that holds float(v) rounded to fp32 -- how eps / leakiness travel in an ExecOp (ctypes rounds the same way when
    the layer-by-layer path hands them to a `float` argument)."""
    return struct.unpack("<i", struct.pack("<f", float(v)))[0]


def _rows(ns, lv):
    return 1 if lv < 0 else ns[lv]


def build_levels(md, size, n_levels):
    """The index structures of `n_levels` U-Net levels below spatial size `size`, as the executor's level table.
    -> (ctypes array, objects kept alive, rows per level), cached on the Metadata; None when a level is empty."""
    size = tuple(int(s) for s in size)
    cache = md.__dict__.setdefault("_exec_levels", {})
    hit = cache.get((size, n_levels))
    if hit is not None:
        return hit or None
    nat = md.__dict__.get("_native")
    if nat is not None and nat[0] == size and nat[1] >= n_levels and nat[2] == 3:
        out = _levels_from_native(md, nat, n_levels)
        if out is not None:
            cache[(size, n_levels)] = out
            return out or None
    arr = (ExecLevel * n_levels)()
    keep, ns = [], []
    sz = size
    for l in range(n_levels):
        rb = md.subm_rulebook(sz, 3)
        if rb.n == 0 or rb.rules is None or rb.tiles is None:
            cache[(size, n_levels)] = False
            return None
        e, t, r = arr[l], rb.tiles, rb.rules
        e.n = rb.n
        e.flags = 1 if getattr(t, "has_x", False) else 0           # SCN_XL_TILE_ORDER_X
        # (`ptr`: addresses straight from the build workspace's layout -- no tensor view is created for the executor)
        e.tstab, e.tile_mask, e.perm, e.tile_order = t.ptr("tstab"), t.ptr("tile_mask"), t.ptr("perm"), t.ptr("tile_order")
        ph = r.prefix_host
        e.in_rows, e.out_rows, e.prefix_host = r.ptr("in_rows"), r.ptr("out_rows"), _addr(ph)
        keep += [rb, ph]
        ns.append(rb.n)
        if l + 1 < n_levels:
            sb = md.strided_rulebook(sz)
            if sb.n_coarse == 0:
                cache[(size, n_levels)] = False
                return None
            ct, cr = sb.tiles, sb.rules
            cph = cr.prefix_host
            e.n_coarse = sb.n_coarse
            e.c_tstab, e.c_tile_mask, e.c_perm, e.c_tile_order = ct.ptr("tstab"), ct.ptr("tile_mask"), ct.ptr("perm"), ct.ptr("tile_order")
            e.c_in_rows, e.c_out_rows, e.c_prefix_host = cr.ptr("in_rows"), cr.ptr("out_rows"), _addr(cph)
            keep += [sb, cph]
            sz = sb.coarse_size
    out = cache[(size, n_levels)] = (arr, keep, ns)
    return out


def _levels_from_native(md, nat, n_levels):
    """build_levels for a Metadata that ONE native call built (Metadata.build_native): every address is workspace base +
    descriptor offset (include/scn_mi355x.h: scn_pyramid_build descriptor), the rule prefixes are the host arrays the rule
    objects already own -- ~15 integer operations per level instead of ~40 attribute chains / view lookups (round 5: the
    detection + mask step follows the host; two Metadata objects per step).  False: a level is empty (layer-by-layer path);
    None: something is not as a native build leaves it (the general path decides)."""
    size, _, _, wsp, per_level, has_x = nat
    arr = (ExecLevel * n_levels)()
    keep, ns = [getattr(md, "_workspace", None)], []
    sz = size
    for l in range(n_levels):
        D = per_level[l]
        rb = md.subm.get((sz, 3))
        if D[0] == 0 or rb is None:
            return False
        rules = rb.__dict__.get("rules")
        ph = None if rules is None else rules.__dict__.get("_prefix_host")
        if ph is None or "_specs" not in rules.__dict__:
            return None
        e = arr[l]
        e.n = D[0]
        e.flags = 1 if has_x else 0
        e.tstab, e.tile_mask, e.perm, e.tile_order = wsp + D[10], wsp + D[11], wsp + D[9], wsp + D[12]
        e.in_rows, e.out_rows, e.prefix_host = wsp + D[64], wsp + D[65], _addr(ph)
        keep.append(ph)
        ns.append(D[0])
        md._note_levels(sz, 1)                           # (the depth hint of the drop-in path, as Metadata.subm_rulebook)
        if l + 1 < n_levels:
            sb = md.strided.get(sz)
            if sb is None or per_level[l + 1][0] == 0:
                return False
            md._unrequested.discard(sz)                 # (as Metadata.strided_rulebook: a layer of this forward asked for it)
            md._note_levels(sz, 2)
            crules = sb.__dict__.get("rules")
            cph = None if crules is None else crules.__dict__.get("_prefix_host")
            if cph is None or "_specs" not in crules.__dict__:
                return None
            e.n_coarse = per_level[l + 1][0]
            e.c_tstab, e.c_tile_mask, e.c_perm, e.c_tile_order = wsp + D[21], wsp + D[22], wsp + D[20], wsp + D[23]
            e.c_in_rows, e.c_out_rows, e.c_prefix_host = wsp + D[66], wsp + D[67], _addr(cph)
            keep.append(cph)
            sz = sb.coarse_size
    return arr, keep, ns


# ----------------------------------------------------------------------------------------------------------------------
# plan compiler
# ----------------------------------------------------------------------------------------------------------------------
class Stage:
    """The launch plan of one autograd node: forward and backward op lists over symbolic buffer / parameter / gradient ids."""

    def __init__(self, bf16, n_inputs, bn_training=True):
        self.bn_training = bool(bn_training)     # batch-norm layers of the plan: batch statistics | the running buffers
        self.bn_layers = []             # training: (mod idx, buffer id of [mean | var], level) per batch-norm layer, module order
        self.bf16 = bool(bf16)
        self.hb = XF_BF16 if bf16 else 0
        self.es = 2 if bf16 else 4
        self.n_inputs = n_inputs
        self.fwd, self.bwd = [], []
        self.bufs = []                  # id -> (level, channels, elem bytes, kind)   kind: "f" fwd ws | "b" bwd ws | "x" external
        self.mods = []                  # modules whose (W, b) the node takes: (module, cin_phys)
        self.params = []                # params-table descriptors: ("w", mod idx) | ("b", mod idx) | ("img", mod idx, cin, cout, n_off, flags)
                                        # | ("rm", mod idx) | ("rv", mod idx): a batch-norm layer's running buffers (evaluation)
        self.gregions = []              # gradient regions: list of [(mod idx, "w"|"b"), ...] laid out back to back
        self.in_ids, self.din_ids = [], []
        self.out_id = self.dout_id = None

    # ---- symbols ----------------------------------------------------------------------------------------------------
    def buf(self, level, ch, es=None, kind="f"):
        self.bufs.append((level, int(ch), self.es if es is None else es, kind))
        return len(self.bufs) - 1

    def mod(self, module, cin_phys):
        for i, (m, c) in enumerate(self.mods):
            if m is module:
                return i
        self.mods.append((module, int(cin_phys)))
        return len(self.mods) - 1

    def param(self, *desc):
        if desc not in self.params:
            self.params.append(desc)
        return self.params.index(desc)

    def weight(self, mi, cin, cout, n_off, flags, tile_kernel):
        """params id of the weight operand of a data op: the fp32 weight, or (bf16 storage, tile kernel) its packed image."""
        if self.bf16 and tile_kernel:
            return self.param("img", mi, cin, cout, n_off, flags & BACK)
        return self.param("w", mi)

    def gregion(self, *members):
        self.gregions.append(list(members))
        return len(self.gregions) - 1

    def op(self, lst, op, level, cin, cout, x=-1, y=-1, r=-1, m=-1, x1=-1, y1=-1, c1=0, w=-1, b=-1, aux=0, flags=0):
        lst.append(ExecOp(op, flags, level, cin, cout, x, y, r, m, x1, y1, c1, w, b, aux, 0))

    # ---- residual units ----------------------------------------------------------------------------------------------
    def units_fwd(self, level, c, x, blocks, out_id=None):
        """blocks (`_unit_blocks`): (conv1, conv2) of x + SubM3(ReLU(SubM3(ReLU(x)))) at `c` physical channels, or a tagged tuple of
        one of the other unit forms (`_form_fwd`).  -> (output id, saved)"""
        saved = []
        for k, blk in enumerate(blocks):
            if isinstance(blk[0], str):                      # a bottleneck / main-path-ReLU unit (_unit_blocks)
                y = out_id if (out_id is not None and k == len(blocks) - 1) else self.buf(level, c)
                saved.append((self._bn_fwd if blk[0] == "bn" else self._form_fwd)(level, c, x, y, blk))
                x = y
                continue
            c1, c2 = blk
            m1, m2 = self.mod(c1, c), self.mod(c2, c)
            y1 = self.buf(level, c)
            y = out_id if (out_id is not None and k == len(blocks) - 1) else self.buf(level, c)
            fl = L.F_RELU_IN | self.hb
            self.op(self.fwd, OP_CONV_SUBM, level, c, c, x=x, y=y1, w=self.weight(m1, c, c, 27, 0, True), b=self.param("b", m1), flags=fl)
            self.op(self.fwd, OP_CONV_SUBM, level, c, c, x=y1, y=y, r=x, w=self.weight(m2, c, c, 27, 0, True), b=self.param("b", m2), flags=fl)
            saved.append((x, y1, m1, m2))
            x = y
        return x, saved

    def units_bwd(self, level, c, g, saved, din_id=None):
        """Backward of units_fwd: g = gradient of the last block's output -> id of the gradient of the first block's input."""
        for k, sv in enumerate(reversed(saved)):
            if isinstance(sv[0], str):
                dx = din_id if (din_id is not None and k == len(saved) - 1) else self.buf(level, c, kind="b")
                (self._bn_bwd if sv[0] == "bn" else self._form_bwd)(level, c, g, dx, sv)
                g = dx
                continue
            x, y1, m1, m2 = sv
            dy1 = self.buf(level, c, kind="b")
            dx = din_id if (din_id is not None and k == len(saved) - 1) else self.buf(level, c, kind="b")
            self.op(self.bwd, OP_CONV_SUBM, level, c, c, x=g, y=dy1, m=y1, w=self.weight(m2, c, c, 27, BACK, True), flags=BACK | self.hb)
            self.op(self.bwd, OP_CONV_SUBM, level, c, c, x=dy1, y=dx, m=x, r=g, w=self.weight(m1, c, c, 27, BACK, True),
                    flags=BACK | L.F_RESIDUAL_LAST | self.hb)
            gw, gb = self.gregion((m1, "w"), (m2, "w")), self.gregion((m1, "b"), (m2, "b"))
            self.op(self.bwd, OP_WGRAD2_SUBM, level, c, c, x=x, y=dy1, x1=y1, y1=g, w=gw, b=gb, flags=L.F_RELU_IN | self.hb)
            g = dx
        return g

    # ---- the reference's other unit forms (unet.py header; module_factory.py:127-183) ----------------------------------------
    # Each op is the call the layer-by-layer path makes for that layer (modules.Sequential: ReLU fused into the next
    # convolution's gather, the AddTable into the last convolution's epilogue).  Backward, the two gradient paths of x meet in
    # an SCN_OP_ADD -- layer by layer autograd adds them -- because the row GEMM has no "residual after the mask" epilogue and
    # a bf16 slab must be rounded before the add to give autograd's bits.  The closing ReLU of a main-path unit is one
    # SCN_OP_RELU in place on the unit's result; its backward masks by that result (y > 0 exactly where the sum was).
    #
    # Post-activation units (relu_first=False, "post" / "post_bottleneck"): y = x + act(t), t the branch's last convolution.  No
    # activation on the way in, no residual in the last convolution's epilogue; ONE SCN_OP_ADD_RELU ends the unit and leaves t
    # as it is, which is the mask of the backward's SCN_OP_RELU_BWD.  The skip's gradient is dy itself, the branch's is masked.
    # Plain blocks (use_residuals=False): "plain_pre" = K(ReLU(x)), the ReLU in the gather; "plain_post" = ReLU(K(x)), the ReLU
    # one in-place SCN_OP_RELU on the block's result, its backward masked by that result.
    def _form_fwd(self, level, c, x, y, blk):
        hb, relu = self.hb, L.F_RELU_IN | self.hb
        form, main = blk[0], blk[0] in ("main", "both")
        post = form in ("post", "post_bottleneck")
        if form in ("plain_pre", "plain_post"):
            m1 = self.mod(blk[1], c)
            self.op(self.fwd, OP_CONV_SUBM, level, c, c, x=x, y=y, w=self.weight(m1, c, c, 27, 0, True), b=self.param("b", m1),
                    flags=relu if form == "plain_pre" else hb)
            if form == "plain_post":
                self.op(self.fwd, OP_RELU, level, c, 0, x=y, y=y, flags=hb)
            return (form, x, y, m1)
        first = hb if (main or post) else relu              # main_path_relu / post-activation: no activation on the way in
        t = self.buf(level, c) if post else y               # post-activation: the branch's result, kept for the backward mask
        r = -1 if post else x
        if form in ("main", "post"):
            _, c1, c2 = blk
            m1, m2 = self.mod(c1, c), self.mod(c2, c)
            y1 = self.buf(level, c)
            self.op(self.fwd, OP_CONV_SUBM, level, c, c, x=x, y=y1, w=self.weight(m1, c, c, 27, 0, True), b=self.param("b", m1), flags=first)
            self.op(self.fwd, OP_CONV_SUBM, level, c, c, x=y1, y=t, r=r, w=self.weight(m2, c, c, 27, 0, True), b=self.param("b", m2), flags=relu)
            sv = (form, x, y, y1, m1, m2)
        else:
            _, n1, kk, n2 = blk
            ci = n1.nOut
            m1, mk, m2 = self.mod(n1, c), self.mod(kk, ci), self.mod(n2, ci)
            a, b = self.buf(level, ci), self.buf(level, ci)
            self.op(self.fwd, OP_GEMM_IDENT, level, c, ci, x=x, y=a, w=self.param("w", m1), b=self.param("b", m1), flags=first)
            self.op(self.fwd, OP_CONV_SUBM, level, ci, ci, x=a, y=b, w=self.weight(mk, ci, ci, 27, 0, True), b=self.param("b", mk), flags=relu)
            self.op(self.fwd, OP_GEMM_IDENT, level, ci, c, x=b, y=t, r=r, w=self.param("w", m2), b=self.param("b", m2), flags=relu)
            sv = (form, x, y, a, b, ci, m1, mk, m2)
        if main:
            self.op(self.fwd, OP_RELU, level, c, 0, x=y, y=y, flags=hb)
        if post:
            self.op(self.fwd, OP_ADD_RELU, level, c, 0, x=x, x1=t, y=y, flags=hb)
            sv = sv + (t,)
        return sv

    def _form_bwd(self, level, c, g, dx, sv):
        hb, relu = self.hb, L.F_RELU_IN | self.hb
        form, x, y = sv[:3]
        if form in ("plain_pre", "plain_post"):
            m1 = sv[3]
            if form == "plain_post":
                gs = self.buf(level, c, kind="b")
                self.op(self.bwd, OP_RELU_BWD, level, c, 0, m=y, x1=g, y=gs, flags=hb)
                g = gs
            pre = form == "plain_pre"
            self.op(self.bwd, OP_CONV_SUBM, level, c, c, x=g, y=dx, m=x if pre else -1, w=self.weight(m1, c, c, 27, BACK, True),
                    flags=BACK | hb)
            self.op(self.bwd, OP_WGRAD_SUBM, level, c, c, x=x, y=g, w=self.gregion((m1, "w")), b=self.gregion((m1, "b")),
                    flags=relu if pre else hb)
            return
        main = form in ("main", "both")
        post = form in ("post", "post_bottleneck")
        first = hb if (main or post) else relu
        g_skip = g                                          # what the skip hands back to x
        if main:
            gs = self.buf(level, c, kind="b")
            self.op(self.bwd, OP_RELU_BWD, level, c, 0, m=y, x1=g, y=gs, flags=hb)
            g = g_skip = gs
        if post:                                            # only the branch passes the closing activation
            gs = self.buf(level, c, kind="b")
            self.op(self.bwd, OP_RELU_BWD, level, c, 0, m=sv[-1], x1=g, y=gs, flags=hb)
            g, sv = gs, sv[:-1]
        t = self.buf(level, c, kind="b")                    # the branch's gradient of x, before the skip's is added
        if form in ("main", "post"):
            y1, m1, m2 = sv[3:]
            dy1 = self.buf(level, c, kind="b")
            self.op(self.bwd, OP_CONV_SUBM, level, c, c, x=g, y=dy1, m=y1, w=self.weight(m2, c, c, 27, BACK, True), flags=BACK | hb)
            self.op(self.bwd, OP_CONV_SUBM, level, c, c, x=dy1, y=t, w=self.weight(m1, c, c, 27, BACK, True), flags=BACK | hb)
            self.op(self.bwd, OP_ADD, level, c, 0, x=t, x1=g_skip, y=dx, flags=hb)
            self.op(self.bwd, OP_WGRAD_SUBM, level, c, c, x=y1, y=g, w=self.gregion((m2, "w")), b=self.gregion((m2, "b")), flags=relu)
            self.op(self.bwd, OP_WGRAD_SUBM, level, c, c, x=x, y=dy1, w=self.gregion((m1, "w")), b=self.gregion((m1, "b")), flags=first)
            return
        a, b, ci, m1, mk, m2 = sv[3:]
        db, da = self.buf(level, ci, kind="b"), self.buf(level, ci, kind="b")
        self.op(self.bwd, OP_GEMM_IDENT, level, c, ci, x=g, y=db, m=b, w=self.param("w", m2), flags=BACK | hb)
        self.op(self.bwd, OP_CONV_SUBM, level, ci, ci, x=db, y=da, m=a, w=self.weight(mk, ci, ci, 27, BACK, True), flags=BACK | hb)
        self.op(self.bwd, OP_GEMM_IDENT, level, ci, c, x=da, y=t, m=-1 if (main or post) else x, w=self.param("w", m1), flags=BACK | hb)
        self.op(self.bwd, OP_ADD, level, c, 0, x=t, x1=g_skip, y=dx, flags=hb)
        self.op(self.bwd, OP_WGRAD_IDENT, level, ci, c, x=b, y=g, w=self.gregion((m2, "w")), b=self.gregion((m2, "b")), flags=relu)
        self.op(self.bwd, OP_WGRAD_SUBM, level, ci, ci, x=a, y=db, w=self.gregion((mk, "w")), b=self.gregion((mk, "b")), flags=relu)
        self.op(self.bwd, OP_WGRAD_IDENT, level, c, ci, x=x, y=da, w=self.gregion((m1, "w")), b=self.gregion((m1, "b")), flags=first)

    # ---- batch-norm activations and units (bn_stages) ---------------------------------------------------------------------
    # A BatchNorm(Leaky)ReLU layer is SCN_OP_BN_STATS (training mode: batch mean | biased variance -> ONE 2c-float vector of the
    # stage workspace) + SCN_OP_BN_FWD reading slab x and writing a slab y of its own -- never a flag of the consuming
    # convolution --, and SCN_OP_BN_BWD (x, dy -> dx and dgamma | dbeta in ONE gradient region) on the way back: scn_bn_stats /
    # scn_bn_fwd / scn_bn_bwd with the arguments functional.BatchNormReLUFunction passes.  gamma and beta sit next to each other
    # in the params table (`w` names gamma); evaluation mode: the running buffers follow them, no statistics op is planned.
    def bn_layer(self, level, m, x, y):
        c = int(m.nPlanes)
        mi = self.mod(m, c)
        if ("w", mi) in self.params:
            raise RuntimeError("executor plan: a batch-norm layer stands twice in one stage")
        gp = self.param("w", mi)
        self.param("b", mi)
        mv, fl = -1, 0
        if self.bn_training:
            mv, fl = self.buf(VEC, 2 * c, 4), XF_BN_TRAINING
            self.op(self.fwd, OP_BN_STATS, level, c, 0, x=x, y=mv)
            self.bn_layers.append((mi, mv, level))
        else:
            self.param("rm", mi)
            self.param("rv", mi)
        eps, leak = _f32_bits(m.eps), _f32_bits(m.leakiness)
        self.op(self.fwd, OP_BN_FWD, level, c, 0, x=x, y=y, x1=mv, w=gp, aux=eps, c1=leak, flags=fl)
        return (level, c, mi, x, mv, gp, eps, leak, fl)

    def bn_layer_bwd(self, rec, g, dx):
        level, c, mi, x, mv, gp, eps, leak, fl = rec
        self.op(self.bwd, OP_BN_BWD, level, c, 0, x=x, m=g, y=dx, x1=mv, w=gp, b=self.gregion((mi, "w"), (mi, "b")), aux=eps,
                c1=leak, flags=fl)

    def _chain_conv(self, level, m, cin, x, y, r=-1):
        """A SubM 3^3 / 1^3 layer of a batch-norm unit: no activation in its gather, its bias (None beside batch norm) as it is."""
        mi, cout = self.mod(m, cin), int(m.nOut)
        b = self.param("b", mi) if m.bias is not None else -1
        if m.filter_size == 3:
            self.op(self.fwd, OP_CONV_SUBM, level, cin, cout, x=x, y=y, r=r, w=self.weight(mi, cin, cout, 27, 0, True), b=b, flags=self.hb)
        else:
            self.op(self.fwd, OP_GEMM_IDENT, level, cin, cout, x=x, y=y, r=r, w=self.param("w", mi), b=b, flags=self.hb)
        return (mi, m.filter_size, cin, cout, x, m.bias is not None)

    def _chain_conv_bwd(self, level, rec, g, dx):
        mi, k, cin, cout, x, has_b = rec
        if k == 3:
            self.op(self.bwd, OP_CONV_SUBM, level, cout, cin, x=g, y=dx, w=self.weight(mi, cout, cin, 27, BACK, True), flags=BACK | self.hb)
        else:
            self.op(self.bwd, OP_GEMM_IDENT, level, cout, cin, x=g, y=dx, w=self.param("w", mi), flags=BACK | self.hb)
        gw = self.gregion((mi, "w"))
        gb = self.gregion((mi, "b")) if has_b else -1      # (no bias: scn_wgrad_rules, as the layer's own backward)
        self.op(self.bwd, OP_WGRAD_SUBM if k == 3 else OP_WGRAD_IDENT, level, cin, cout, x=x, y=g, w=gw, b=gb, flags=self.hb)

    def _bn_fwd(self, level, c, x, y, blk):
        """A unit of `_bn_blocks`: the branch layer by layer, every layer writing a slab of its own.  skip "res": x joins in the
        last convolution's epilogue (modules.Sequential hands it the residual); "add": one SCN_OP_ADD behind a branch that ends
        in its activation (post-activation); None: a flat run of plain blocks.  closing: the activation of a main-path unit."""
        _, _, skip, mods, closing = blk
        end = y if closing is None else self.buf(level, c)
        t, w, tape = x, c, []
        for i, m in enumerate(mods):
            last = i == len(mods) - 1
            bn = isinstance(m, M._BatchNorm)
            cout = int(m.nPlanes) if bn else int(m.nOut)
            dst = end if (last and skip != "add") else self.buf(level, cout)
            if bn:
                tape.append(("a", self.bn_layer(level, m, t, dst)))
            else:
                tape.append(("k", self._chain_conv(level, m, w, t, dst, r=x if (last and skip == "res") else -1)))
            t, w = dst, cout
        if skip == "add":
            self.op(self.fwd, OP_ADD, level, c, 0, x=x, x1=t, y=end, flags=self.hb)
        crec = self.bn_layer(level, closing, end, y) if closing is not None else None
        return ("bn", skip, tape, crec)

    def _bn_bwd(self, level, c, g, dx, sv):
        _, skip, tape, crec = sv
        if crec is not None:
            gs = self.buf(level, c, kind="b")
            self.bn_layer_bwd(crec, g, gs)
            g = gs
        t = g
        for i in range(len(tape) - 1, -1, -1):
            kind, rec = tape[i]
            cin = rec[1] if kind == "a" else rec[2]
            dst = dx if (i == 0 and skip is None) else self.buf(level, cin, kind="b")
            if kind == "a":
                self.bn_layer_bwd(rec, t, dst)
            else:
                self._chain_conv_bwd(level, rec, t, dst)
            t = dst
        if skip is not None:                                # the two gradient paths of x: layer by layer autograd adds them
            self.op(self.bwd, OP_ADD, level, c, 0, x=t, x1=g, y=dx, flags=self.hb)

    # ---- finish -----------------------------------------------------------------------------------------------------
    def freeze(self):
        self.fwd_arr = (ExecOp * len(self.fwd))(*self.fwd)
        self.bwd_arr = (ExecOp * len(self.bwd))(*self.bwd)
        self.fwd_ws = [i for i, b in enumerate(self.bufs) if b[3] == "f"]
        self.bwd_ws = [i for i, b in enumerate(self.bufs) if b[3] == "b"]
        # host-side tables of a call, built once (the per-call Python is what a host-bound step feels: DESIGN.md section 5)
        self.fwd_specs = [(self.bufs[i][0], self.bufs[i][1] * self.bufs[i][2]) for i in self.fwd_ws]     # (level, row bytes)
        self.bwd_specs = [(self.bufs[i][0], self.bufs[i][1] * self.bufs[i][2]) for i in self.bwd_ws]
        self.w_entries = [(k, 2 * d[1]) for k, d in enumerate(self.params) if d[0] == "w"]
        self.b_entries = [(k, 2 * d[1] + 1) for k, d in enumerate(self.params) if d[0] == "b"]
        self.img_entries = [(k, 2 * d[1]) + tuple(d[2:]) for k, d in enumerate(self.params) if d[0] == "img"]
        # batch norm: the running buffers an evaluation-mode plan reads, the positions of gamma / beta among the node's parameters
        self.stat_entries = [(k, d[1], "running_mean" if d[0] == "rm" else "running_var") for k, d in enumerate(self.params)
                             if d[0] in ("rm", "rv")]
        self.bn_phys = frozenset(2 * i + j for i, (m, _) in enumerate(self.mods) if isinstance(m, M._BatchNorm) for j in (0, 1))
        self.grad_views = {}                              # tuple of parameter shapes -> (region offsets, total, views)
        # a main-path unit that ends the stage: its backward masks by the stage's OUTPUT slab, which then is saved for backward
        self.bwd_reads_out = any(getattr(op, f) == self.out_id for op in self.bwd for f in ("x", "y", "r", "m", "x1", "y1"))
        self._lean_slots()
        covered = sorted(m for reg in self.gregions for m in reg)
        want = sorted((i, k) for i, (m, _) in enumerate(self.mods) for k in ("w", "b")
                      if k == "w" or getattr(m, "bias", None) is not None or not self.bn_phys)
        if covered != want:
            raise RuntimeError("executor plan: every parameter must sit in exactly one gradient region")
        return self


def _lean_slots(self):
    """Forward-only plan (evaluation: `eval_model`, ndsis/training/training.py:244-304, and `SparseMaskPredictor`,
    model.py:826-882, run the forward under torch.no_grad()): nothing is kept for a backward pass, so a forward slab's
    storage is handed on as soon as its last reader has been queued.  Slots per (level, row bytes) class by liveness over the
    forward op list; an op's output never shares a slot with one of its own operands (a slot is released AFTER the op)."""
    last = {}
    for t, op in enumerate(self.fwd):
        for v in (op.x, op.r, op.m, op.x1, op.y, op.y1):
            if v >= 0:
                last[v] = t
    ws = set(i for i, b in enumerate(self.bufs) if b[3] == "f")
    free, n_slots, slot_of = {}, {}, {}
    for t, op in enumerate(self.fwd):
        for v in (op.y, op.y1):
            if v in ws and v not in slot_of:
                cls = (self.bufs[v][0], self.bufs[v][1] * self.bufs[v][2])
                if free.get(cls):
                    slot_of[v] = (cls, free[cls].pop())
                else:
                    slot_of[v] = (cls, n_slots.get(cls, 0))
                    n_slots[cls] = n_slots.get(cls, 0) + 1
        for v in (op.x, op.r, op.m, op.x1, op.y, op.y1):
            if v in slot_of and last[v] == t and slot_of[v] is not None and self.bufs[v][0] != VEC:   # (VEC: the host reads it after the pass)
                cls, k = slot_of[v]
                if k not in free.setdefault(cls, []):
                    free[cls].append(k)
    for v in ws:                                          # (a declared slab no forward op writes: give it a slot of its own)
        if v not in slot_of:
            cls = (self.bufs[v][0], self.bufs[v][1] * self.bufs[v][2])
            slot_of[v] = (cls, n_slots.get(cls, 0))
            n_slots[cls] = n_slots.get(cls, 0) + 1
    self.lean_classes = sorted(n_slots.items())            # [((level, row bytes), slots)]
    self.lean_slot_of = [slot_of[i] for i in self.fwd_ws]


Stage._lean_slots = _lean_slots


def run_add_relu(x_ptr, x1_ptr, y_ptr, rows, c, bf16, scratch):
    """y = x + max(x1, 0) over [rows, c] slabs as a plan of ONE SCN_OP_ADD_RELU through scn_exec_run: the fused end of a
    post-activation unit has no entry point of its own.  Raw addresses; scratch: a device tensor of at least 256 bytes (the
    executor asks for one whatever the ops are).  For the kernel tests and tools/post_act_bench.py."""
    lib = L.lib()
    levels = (ExecLevel * 1)()
    levels[0].n = int(rows)
    ops = (ExecOp * 1)(ExecOp(OP_ADD_RELU, XF_BF16 if bf16 else 0, 0, int(c), 0, 0, 2, -1, -1, 1, -1, 0, -1, -1, 0, 0))
    table = (vp * 3)(x_ptr, x1_ptr, y_ptr)
    L.check(lib.scn_exec_run(ops, 1, levels, 1, table, None, None, scratch.data_ptr(), scratch.numel(), None, L.stream()))


def _lean_layout(stage, ns):
    """-> (offset per forward workspace buffer, total bytes) of the forward-only plan."""
    base, tot = {}, 0
    for (lv, row_bytes), k in stage.lean_classes:
        size = (_rows(ns, lv) * row_bytes + 255) & ~255
        base[(lv, row_bytes)] = (tot, size)
        tot += size * k
    return [base[cls][0] + k * base[cls][1] for cls, k in stage.lean_slot_of], tot


def _plain_blocks(unit_seq):
    """[(conv1, conv2)] of a `units(...)` Sequential, or None when a block is not the plain pre-activation unit."""
    out = []
    for block in unit_seq:
        if not (type(block) is M.Sequential and len(block) == 2 and type(block[0]) is M.ConcatTable and type(block[1]) is M.AddTable):
            return None
        a, inner = list(block[0]._modules.values()) if len(block[0]._modules) == 2 else (None, None)
        if type(a) is not M.Identity or type(inner) is not M.Sequential or len(inner) != 4:
            return None
        r0, c1, r1, c2 = list(inner._modules.values())
        if not (type(r0) is M.ReLU and type(r1) is M.ReLU and type(c1) is M.SubmanifoldConvolution
                and type(c2) is M.SubmanifoldConvolution and c1.filter_size == 3 and c2.filter_size == 3
                and c1.bias is not None and c2.bias is not None and c1.nIn == c2.nOut and c1.nOut == c2.nIn == c1.nIn
                and c1.groups == 1 and c2.groups == 1):
            return None
        out.append((c1, c2))
    return out


def _bn_chain(mods, c):
    """Channels behind a run of BatchNorm(Leaky)ReLU / SubM 3^3 / SubM 1^3 layers that starts at c channels; None: not such a run."""
    for m in mods:
        if isinstance(m, M._BatchNorm):
            if int(m.nPlanes) != c:
                return None
        elif (type(m) is M.SubmanifoldConvolution and m.filter_size in (1, 3) and m.groups == 1 and not m.pad_out_to
                and m.nIn == c):
            c = m.nOut
        else:
            return None
    return c


def _bn_blocks(unit_seq):
    """`_unit_blocks` of a batch-norm network: every unit form of unet.residual_block / plain_blocks with BatchNorm(Leaky)ReLU where
    the ReLU stands, as ("bn", channels, skip, branch layers, closing activation | None) -- skip "res": the branch ends in a
    convolution that adds x in its epilogue (pre-activation, bottleneck, main-path units); "add": the branch ends in its
    activation and an AddTable follows (post-activation); None: one flat run [act, K] * n | [K, act] * n.  A ReLU that batch
    norm replaced never appears: a unit that still holds one is none of these (None)."""
    mods = list(unit_seq._modules.values()) if isinstance(unit_seq, torch.nn.Sequential) else list(unit_seq)
    if mods and all(isinstance(m, (M._BatchNorm, M.SubmanifoldConvolution)) for m in mods):
        c = int(mods[0].nPlanes) if isinstance(mods[0], M._BatchNorm) else mods[0].nIn
        kinds = [isinstance(m, M._BatchNorm) for m in mods]
        if len(mods) % 2 or kinds != [kinds[0], not kinds[0]] * (len(mods) // 2) or _bn_chain(mods, c) != c:
            return None
        return [("bn", c, None, mods, None)]
    out = []
    for block in mods:
        if not (type(block) is M.Sequential and len(block) in (2, 3) and type(block[0]) is M.ConcatTable
                and type(block[1]) is M.AddTable and len(block[0]._modules) == 2):
            return None
        closing = block[2] if len(block) == 3 else None
        a, inner = list(block[0]._modules.values())
        if type(a) is not M.Identity or type(inner) is not M.Sequential or not len(inner):
            return None
        branch = list(inner._modules.values())
        c = int(branch[0].nPlanes) if isinstance(branch[0], M._BatchNorm) else getattr(branch[0], "nIn", None)
        if c is None or _bn_chain(branch, c) != c or not any(isinstance(m, M._BatchNorm) for m in branch):
            return None
        if closing is not None and not (isinstance(closing, M._BatchNorm) and int(closing.nPlanes) == c):
            return None
        out.append(("bn", c, "add" if isinstance(branch[-1], M._BatchNorm) else "res", branch, closing))
    return out


def _unit_blocks(unit_seq, bn=False):
    """_plain_blocks with the reference's other unit forms: a plain unit stays (conv1, conv2); the others come as
    ("bottleneck" | "both", N1, K, N2) and ("main", K1, K2) -- "both" and "main" close with a ReLU (main_path_relu).  None when
    a block is none of them (batch norm, a layer without bias, channel padding, groups).
    bn: a batch-norm layer may stand wherever a ReLU may (`_bn_blocks`)."""
    if bn and any(isinstance(m, M._BatchNorm) for m in (unit_seq.modules() if isinstance(unit_seq, torch.nn.Module) else unit_seq)):
        return _bn_blocks(unit_seq)
    out = []
    mods = list(unit_seq._modules.values()) if isinstance(unit_seq, torch.nn.Sequential) else list(unit_seq)
    if mods and len(mods) % 2 == 0 and all(type(m) in (M.ReLU, M.SubmanifoldConvolution) for m in mods):
        # use_residuals=False: a flat [ReLU, K] * n | [K, ReLU] * n (module_factory.py:186-218)
        pre = type(mods[0]) is M.ReLU
        convs, relus = (mods[1::2], mods[0::2]) if pre else (mods[0::2], mods[1::2])
        if any(type(m) is not M.ReLU for m in relus):
            return None
        for m in convs:
            if (type(m) is not M.SubmanifoldConvolution or m.filter_size != 3 or m.bias is None or m.groups != 1 or m.pad_out_to
                    or m.nIn != m.nOut):
                return None
            out.append(("plain_pre" if pre else "plain_post", m))
        return out
    for block in unit_seq:
        plain = _plain_blocks([block])
        if plain is not None:
            out += plain
            continue
        if not (type(block) is M.Sequential and len(block) in (2, 3) and type(block[0]) is M.ConcatTable
                and type(block[1]) is M.AddTable and len(block[0]._modules) == 2):
            return None
        main = len(block) == 3
        if main and type(block[2]) is not M.ReLU:
            return None
        a, inner = list(block[0]._modules.values())
        if type(a) is not M.Identity or type(inner) is not M.Sequential:
            return None
        mods = list(inner._modules.values())
        post = False
        if not main:                                         # relu_first: the branch opens with the activation ...
            if not mods:
                return None
            if type(mods[0]) is M.ReLU:
                mods = mods[1:]
            elif type(mods[-1]) is M.ReLU:                   # ... without it the activation closes the branch (post-activation)
                mods, post = mods[:-1], True
            else:
                return None
        if len(mods) not in (3, 5) or any(type(m) is not M.ReLU for m in mods[1::2]):
            return None
        convs = mods[0::2]
        if any(type(m) is not M.SubmanifoldConvolution or m.bias is None or m.groups != 1 or m.pad_out_to for m in convs):
            return None
        sizes = tuple(m.filter_size for m in convs)
        c = convs[0].nIn
        if sizes == (3, 3):
            if not (main or post) or any((m.nIn, m.nOut) != (c, c) for m in convs):
                return None
            out.append(("post" if post else "main", *convs))
        elif sizes == (1, 3, 1):
            ci = convs[0].nOut
            if (convs[1].nIn, convs[1].nOut, convs[2].nIn, convs[2].nOut) != (ci, ci, ci, c):
                return None
            out.append(("both" if main else ("post_bottleneck" if post else "bottleneck"), *convs))
        else:
            return None
    return out


def _block_width(blk):
    """Channels a unit of `_unit_blocks` takes and gives."""
    if blk[0] == "bn":
        return blk[1]
    return (blk[1] if isinstance(blk[0], str) else blk[0]).nIn


def _phys(m):
    return int(getattr(m, "pad_out_to", None) or m.nOut)


def _stage_relus(stage, bn=False):
    """(a ReLU leads the layer, a ReLU follows it) of an input stage (module_factory.py:438-486): the conv-type layer itself or a
    Sequential of just it -- (False, False) --, Sequential(ReLU, layer), Sequential(layer, ReLU).  None: anything else.
    bn: a batch-norm layer may stand where the ReLU does; the pair then holds that MODULE in place of True."""
    if isinstance(stage, M._ConvBase):
        return (False, False)
    if type(stage) is not M.Sequential:
        return None
    mods = list(stage._modules.values())
    kinds = tuple("r" if (type(m) is M.ReLU or (bn and isinstance(m, M._BatchNorm))) else ("c" if isinstance(m, M._ConvBase) else "?")
                  for m in mods)
    out = {("c",): (False, False), ("r", "c"): (True, False), ("c", "r"): (False, True)}.get(kinds)
    if out is None or not bn:
        return out
    act = mods[0] if out[0] else (mods[1] if out[1] else None)
    if isinstance(act, M._BatchNorm):
        return (act, False) if out[0] else (False, act)
    return out


def _bn_of(flag):
    """The batch-norm layer a `_stage_relus` entry names, or None (no activation there, or a ReLU)."""
    return flag if isinstance(flag, M._BatchNorm) else None


def compile_encoder_stage(level, head, blocks, cin_phys, bf16, cast_first=False, cast_last=False, in_bf16=False,
                          relus=(False, False), bn_training=True):
    """Encoder level: head (SubM 1^3 at level 0 | Convolution 2^3/2 from level-1) + residual units.
    level 0 in bf16 storage: the head runs in fp32 on the fp32 input and its result is cast (SparseUNet), or -- cast_first,
    the mask branch's input stage -- the input is cast first and the head runs on bf16 rows, or -- in_bf16 -- the input
    slab is bf16-stored already (a SubM 1^3 stage behind a bf16 network in a module tree); cast_last: fp32 output.
    relus (`_stage_relus`): a ReLU in front of the head is fused into its gather; one behind it is an in-place SCN_OP_RELU on the
    head's result, whose backward masks by that slab.  A batch-norm layer in either place (`_stage_relus(bn=True)`; fp32 slabs
    only) reads one slab and writes another: in front, the head gathers the normalised slab; behind, the units start from it.
    bn_training: the batch-norm layers of the stage take batch statistics (False: their running buffers)."""
    lead, trail = relus
    lead_bn, trail_bn = _bn_of(lead), _bn_of(trail)
    if bf16 and (lead_bn or trail_bn or any(b[0] == "bn" for b in blocks)):
        raise NotImplementedError("executor: batch norm runs on fp32 slabs")
    lead, trail = bool(lead) and lead_bn is None, bool(trail) and trail_bn is None
    lead_fl = L.F_RELU_IN if lead else 0
    st = Stage(bf16, 1, bn_training)
    in_bf16 = bool(bf16 and in_bf16 and level == 0)
    es_in = (2 if in_bf16 else 4) if (level == 0) else st.es
    c = _phys(head)
    IN = st.buf(level if level == 0 else level - 1, cin_phys, es_in, "x")
    st.in_ids = [IN]
    mh = st.mod(head, cin_phys)
    out_es = 4 if (cast_last or not bf16) else 2
    OUT = st.buf(level, c, out_es, "x")
    st.out_id = OUT
    if level == 0:
        if bf16 and (cast_first or in_bf16):
            if lead or trail:
                raise NotImplementedError("executor: a level-0 head on bf16 rows takes no input-stage ReLU")
            xin = IN
            if not in_bf16:
                xin = st.buf(0, cin_phys)
                st.op(st.fwd, OP_CAST, 0, cin_phys, 0, x=IN, y=xin, flags=XF_BF16)
            h = st.buf(0, c)
            st.op(st.fwd, OP_GEMM_IDENT, 0, cin_phys, c, x=xin, y=h, w=st.param("w", mh), b=st.param("b", mh), flags=XF_BF16)
            x, head_in, head_hb = h, xin, XF_BF16
        else:
            h = st.buf(0, c, 4)
            head_in = IN
            if lead_bn is not None:
                head_in = st.buf(0, cin_phys, 4)
                lead_rec = st.bn_layer(0, lead_bn, IN, head_in)
            st.op(st.fwd, OP_GEMM_IDENT, 0, cin_phys, c, x=head_in, y=h, w=st.param("w", mh), b=st.param("b", mh), flags=lead_fl)
            if trail:
                st.op(st.fwd, OP_RELU, 0, c, 0, x=h, y=h, flags=0)
            x, head_hb = h, 0
            if trail_bn is not None:
                x = st.buf(0, c, 4)
                trail_rec = st.bn_layer(0, trail_bn, h, x)
            if bf16:
                x = st.buf(0, c)
                st.op(st.fwd, OP_CAST, 0, c, 0, x=h, y=x, flags=XF_BF16)
    else:
        x = st.buf(level, c)
        head_in = IN
        if lead_bn is not None:
            head_in = st.buf(level - 1, cin_phys)
            lead_rec = st.bn_layer(level - 1, lead_bn, IN, head_in)
        st.op(st.fwd, OP_CONV_CHILD, level - 1, cin_phys, c, x=head_in, y=x, w=st.weight(mh, cin_phys, c, 8, 0, True),
              b=st.param("b", mh), flags=lead_fl | st.hb)
        h = x
        if trail:
            st.op(st.fwd, OP_RELU, level, c, 0, x=x, y=x, flags=st.hb)
        if trail_bn is not None:
            x = st.buf(level, c)
            trail_rec = st.bn_layer(level, trail_bn, h, x)
    if bf16 and cast_last:
        last, saved = st.units_fwd(level, c, x, blocks)
        st.op(st.fwd, OP_CAST, level, c, 0, x=last, y=OUT, flags=0)
    else:
        last, saved = st.units_fwd(level, c, x, blocks, out_id=OUT)
    # ---- backward
    DOUT = st.buf(level, c, out_es, "x")
    st.dout_id = DOUT
    g = DOUT
    if bf16 and cast_last:
        g = st.buf(level, c, kind="b")
        st.op(st.bwd, OP_CAST, level, c, 0, x=DOUT, y=g, flags=XF_BF16)
    g = st.units_bwd(level, c, g, saved)
    DIN = st.buf(level if level == 0 else level - 1, cin_phys, es_in, "x")
    st.din_ids = [DIN]
    gw, gb = st.gregion((mh, "w")), st.gregion((mh, "b"))
    if level == 0:
        if head_hb:                                           # head ran on bf16 rows: its input gradient is cast back at the end
            dinb = DIN if in_bf16 else st.buf(0, cin_phys, kind="b")
            st.op(st.bwd, OP_GEMM_IDENT, 0, c, cin_phys, x=g, y=dinb, w=st.param("w", mh), flags=BACK | XF_BF16)
            st.op(st.bwd, OP_WGRAD_IDENT, 0, cin_phys, c, x=head_in, y=g, w=gw, b=gb, flags=XF_BF16)
            if not in_bf16:
                st.op(st.bwd, OP_CAST, 0, cin_phys, 0, x=dinb, y=DIN, flags=0)
        else:
            gf = g
            if bf16:
                gf = st.buf(0, c, 4, "b")
                st.op(st.bwd, OP_CAST, 0, c, 0, x=g, y=gf, flags=0)
            if trail:
                gm = st.buf(0, c, 4, "b")
                st.op(st.bwd, OP_RELU_BWD, 0, c, 0, m=h, x1=gf, y=gm, flags=0)
                gf = gm
            if trail_bn is not None:
                gm = st.buf(0, c, 4, "b")
                st.bn_layer_bwd(trail_rec, gf, gm)
                gf = gm
            dhead = DIN if lead_bn is None else st.buf(0, cin_phys, 4, "b")
            st.op(st.bwd, OP_GEMM_IDENT, 0, c, cin_phys, x=gf, y=dhead, m=IN if lead else -1, w=st.param("w", mh), flags=BACK)
            st.op(st.bwd, OP_WGRAD_IDENT, 0, cin_phys, c, x=head_in, y=gf, w=gw, b=gb, flags=lead_fl)
            if lead_bn is not None:
                st.bn_layer_bwd(lead_rec, dhead, DIN)
    else:
        if trail:
            gm = st.buf(level, c, kind="b")
            st.op(st.bwd, OP_RELU_BWD, level, c, 0, m=h, x1=g, y=gm, flags=st.hb)
            g = gm
        if trail_bn is not None:
            gm = st.buf(level, c, kind="b")
            st.bn_layer_bwd(trail_rec, g, gm)
            g = gm
        dhead = DIN if lead_bn is None else st.buf(level - 1, cin_phys, kind="b")
        st.op(st.bwd, OP_RULES_CHILD, level - 1, c, cin_phys, x=g, y=dhead, m=IN if lead else -1, w=st.param("w", mh),
              flags=L.F_W_TRANSPOSED | st.hb)
        st.op(st.bwd, OP_WGRAD_DOWN, level - 1, cin_phys, c, x=head_in, y=g, w=gw, flags=lead_fl | st.hb)
        st.op(st.bwd, OP_COLSUM, level, c, 0, x=g, b=gb, flags=st.hb)
        if lead_bn is not None:
            st.bn_layer_bwd(lead_rec, dhead, DIN)
    return st.freeze()


def compile_decoder_stage(level, up, nin, blocks, c_coarse, bf16, relus=(True, False), bn_training=True):
    """Decoder level: ReLU -> Deconvolution 2^3/2 (coarse level+1 -> level) -> JoinTable([up, skip]) -> NetworkInNetwork ->
    residual units.  Inputs: (coarse slab, skip slab).  relus (`_stage_relus`): (True, False) is that form; (False, True) the
    relu_first=False one, Deconvolution -> ReLU, the ReLU in place on the deconvolution's result.  A batch-norm layer behind
    the deconvolution (fp32 slabs only) writes the slab the NetworkInNetwork reads; in front of it: not a form the network
    builder makes (NotImplementedError)."""
    lead, trail = relus
    trail_bn = _bn_of(trail)
    if _bn_of(lead) is not None or (bf16 and (trail_bn is not None or any(b[0] == "bn" for b in blocks))):
        raise NotImplementedError("executor: a decoder level takes batch norm behind its deconvolution, on fp32 slabs")
    trail = bool(trail) and trail_bn is None
    lead_fl = L.F_RELU_IN if lead else 0
    st = Stage(bf16, 2, bn_training)
    c = _phys(up)
    IN0 = st.buf(level + 1, c_coarse, None, "x")
    IN1 = st.buf(level, c, None, "x")
    st.in_ids = [IN0, IN1]
    OUT = st.buf(level, c, None, "x")
    st.out_id = OUT
    mu, mn = st.mod(up, c_coarse), st.mod(nin, 2 * c)
    upb = st.buf(level, c)
    st.op(st.fwd, OP_RULES_CHILD, level, c_coarse, c, x=IN0, y=upb, w=st.param("w", mu), b=st.param("b", mu),
          flags=lead_fl | st.hb)
    if trail:
        st.op(st.fwd, OP_RELU, level, c, 0, x=upb, y=upb, flags=st.hb)
    upa = upb                                              # what the NetworkInNetwork reads
    if trail_bn is not None:
        upa = st.buf(level, c)
        trail_rec = st.bn_layer(level, trail_bn, upb, upa)
    h = st.buf(level, c)
    st.op(st.fwd, OP_ROWS2, level, c, c, x=upa, x1=IN1, c1=c, y=h, w=st.param("w", mn), b=st.param("b", mn), flags=st.hb)
    last, saved = st.units_fwd(level, c, h, blocks, out_id=OUT)
    # ---- backward
    DOUT = st.buf(level, c, None, "x")
    st.dout_id = DOUT
    g = st.units_bwd(level, c, DOUT, saved)
    DIN0 = st.buf(level + 1, c_coarse, None, "x")
    DIN1 = st.buf(level, c, None, "x")
    st.din_ids = [DIN0, DIN1]
    dup = st.buf(level, c, kind="b")
    st.op(st.bwd, OP_ROWS2, level, c, c, x=g, y=dup, y1=DIN1, c1=c, w=st.param("w", mn), flags=L.F_W_TRANSPOSED | st.hb)
    gwn, gbn = st.gregion((mn, "w")), st.gregion((mn, "b"))
    st.op(st.bwd, OP_WGRAD_IDENT, level, c, c, x=upa, y=g, w=gwn, b=gbn, aux=0, flags=st.hb)
    st.op(st.bwd, OP_WGRAD_IDENT, level, c, c, x=IN1, y=g, w=gwn, b=-1, aux=c * c, flags=st.hb)
    if trail:
        dm = st.buf(level, c, kind="b")
        st.op(st.bwd, OP_RELU_BWD, level, c, 0, m=upb, x1=dup, y=dm, flags=st.hb)
        dup = dm
    if trail_bn is not None:
        dm = st.buf(level, c, kind="b")
        st.bn_layer_bwd(trail_rec, dup, dm)
        dup = dm
    st.op(st.bwd, OP_CONV_CHILD, level, c, c_coarse, x=dup, y=DIN0, m=IN0 if lead else -1,
          w=st.weight(mu, c, c_coarse, 8, L.F_W_TRANSPOSED, True), flags=L.F_W_TRANSPOSED | st.hb)
    gwu, gbu = st.gregion((mu, "w")), st.gregion((mu, "b"))
    st.op(st.bwd, OP_WGRAD_UP, level, c_coarse, c, x=IN0, y=dup, w=gwu, b=gbu, flags=lead_fl | st.hb)
    return st.freeze()


# ----------------------------------------------------------------------------------------------------------------------
# run time
# ----------------------------------------------------------------------------------------------------------------------
def _layout(specs, ns):
    offs, tot = [], 0
    for lv, row_bytes in specs:
        offs.append(tot)
        tot += (_rows(ns, lv) * row_bytes + 255) & ~255
    return offs, tot


def _run(stage, ops, levels, table, ptab, gtab, dev, side=False, own_scratch=None):
    if own_scratch is not None:                # a pass inside `step_weight_gradients` (never a timed or a side-stream one)
        return _run_plain(stage, ops, levels, table, ptab, gtab, dev, False, own_scratch)
    from . import profiling
    t = profiling.TIMER
    if t is not None and t.exec_timing():      # a sampled step of bench.py: the C call brackets its tile-convolution launches
        lib = L.lib()
        lib.scn_exec_timing_enable(1)
        try:
            return _run_plain(stage, ops, levels, table, ptab, gtab, dev, side)
        finally:
            lib.scn_exec_timing_enable(0)
    return _run_plain(stage, ops, levels, table, ptab, gtab, dev, side)


def _run_plain(stage, ops, levels, table, ptab, gtab, dev, side=False, own_scratch=None):
    lib = L.lib()
    arr, _, ns = levels
    sb, ac = i64(0), i64(0)
    L.check(lib.scn_exec_requirements(ops, len(ops), arr, len(ns), C.byref(sb), C.byref(ac)))
    if own_scratch is not None:                # the unit slabs of this pass live until the step's flush: its own allocation
        scratch = torch.empty(max(sb.value, 256), dtype=torch.uint8, device=dev)
        own_scratch.append(scratch)
    else:
        scratch = L.scratch(sb.value, dev)
    arrival = L.arrival(max(ac.value, 1), dev)
    if side and SIDE_LEAVES:
        key = (dev.index, L.stream())
        st = _side_streams.get(key)
        if st is None:
            st = _side_streams[key] = torch.cuda.Stream(device=dev)
        ss = _side_scratch.get(key)
        if ss is None or ss.numel() < scratch.numel():
            ss = _side_scratch[key] = torch.empty(scratch.numel(), dtype=torch.uint8, device=dev)
        L.check(lib.scn_exec_run_streams(ops, len(ops), arr, len(ns), table, ptab, gtab, scratch.data_ptr(), scratch.numel(),
                                         arrival.data_ptr(), L.stream(), st.cuda_stream, ss.data_ptr(), ss.numel()))
        return
    L.check(lib.scn_exec_run(ops, len(ops), arr, len(ns), table, ptab, gtab, scratch.data_ptr(), scratch.numel(),
                             arrival.data_ptr(), L.stream()))


# ----------------------------------------------------------------------------------------------------------------------
# step scope of the weight gradients
# ----------------------------------------------------------------------------------------------------------------------
_step_scope = threading.local()
LAST_STEP_SCOPE = {"passes": 0, "delivered": 0}    # what the last scope that closed held back (tests)


class _StepScope:
    def __init__(self):
        self.deliver = []           # (parameter, view of the flat gradient buffer of its pass)
        self.pending = set()        # id of every parameter in `deliver`: a second pass that uses it runs in place
        self.keep = []              # everything the held-back launches read or write, until the flush has been queued
        self.passes = 0             # backward passes whose weight gradients were held back


def step_scope_passes():
    """Passes held back by the scope open on this thread (None: no scope is open)."""
    sc = getattr(_step_scope, "scope", None)
    return None if sc is None else sc.passes


@contextlib.contextmanager
def step_weight_gradients():
    """Run the weight gradients of every compiled stage whose backward falls inside the block as ONE grid per kernel variant
    and one sum launch, after the last backward pass (scn_wgrad_step_begin / _flush): no consumer reads
    a parameter gradient before the optimizer step.  Inside the block the backward of an eligible stage (`_step_eligible`)
    returns None for its parameters; at exit, once the flush has been queued on the current stream, `p.grad` is assigned for
    each of them.  Every other stage runs as without the block.  For `loss.backward()` / `torch.autograd.backward` callers that
    read `.grad` afterwards -- `torch.autograd.grad` would see None.  Not under torch's DistributedDataParallel or anything else
    that hooks the AccumulateGrad nodes themselves: such hooks are invisible here and would never fire for a held-back parameter.  Per thread (a backward that autograd runs on another
    thread sees no scope and runs in place), not nestable; an exception inside drops what was recorded and is re-raised."""
    if getattr(_step_scope, "scope", None) is not None:
        raise RuntimeError("executor.step_weight_gradients is not nestable")
    lib = L.lib()
    L.check(lib.scn_wgrad_step_begin())
    sc = _step_scope.scope = _StepScope()
    try:
        yield sc
    except BaseException:
        _step_scope.scope = None
        lib.scn_wgrad_step_discard()
        raise
    _step_scope.scope = None
    try:
        L.check(lib.scn_wgrad_step_flush(L.stream()))
    except BaseException:
        lib.scn_wgrad_step_discard()
        raise
    LAST_STEP_SCOPE["passes"], LAST_STEP_SCOPE["delivered"] = sc.passes, len(sc.deliver)
    with torch.no_grad():
        for p, view in sc.deliver:              # (the flush is queued: on this stream every later reader sees them written)
            if p.grad is None:
                p.grad = view
            else:
                # a later pass of the block that ran in place (the same parameter used twice, or reached through another
                # path) has put its gradient there meanwhile: add, as AccumulateGrad would have -- two terms, same bits
                p.grad.add_(view)
    # one stream: what the held-back launches read may go back to the caching allocator now that they are queued
    sc.keep.clear()
    sc.deliver.clear()


def _step_eligible(stage, kept, needs, pending=()):
    """The parameters of a backward pass inside `step_weight_gradients` whose gradients can be delivered at its exit:
    [(position in the returned gradients, parameter)], or None when the stage has to run in place -- bf16 storage, the
    executor's launch timing or the side stream on, gradient mode on (a double backward), a W or b that is not the module's own
    leaf tensor (a channel-padded stage sees padded views from `_wb`), a parameter that has a `.grad` already (a later
    micro-batch: autograd accumulates), one that a pass held back earlier in the same block will deliver (`pending`: one
    network applied twice in a graph, two backward calls in one block -- the second use runs in place and the exit adds the
    two) or one that carries hooks (the bucketed all-reduce needs its gradients during backward)."""
    if stage.bf16 or SIDE_LEAVES or torch.is_grad_enabled():
        return None
    from . import profiling
    t = profiling.TIMER
    if t is not None and t.exec_timing():
        return None
    out, k = [], 0
    for mi, (m, _) in enumerate(stage.mods):
        for which, p in ((0, m.weight), (1, m.bias)):
            j = 2 * mi + which
            if p is None:                       # (phys[j] was None as well: save_for_backward skipped it)
                if stage.bn_phys:               # a batch-norm stage: its units' convolutions have no bias, nothing to deliver
                    continue
                return None
            if kept[k] is not p or not p.is_leaf:
                return None
            k += 1
            if not needs[j] or j in stage.bn_phys:      # (gamma / beta: scn_bn_bwd writes them inside the pass -- never held back)
                continue
            if p.grad is not None or id(p) in pending or p._backward_hooks or getattr(p, "_post_accumulate_grad_hooks", None):
                return None
            out.append((j, p))
    return out


LAST_FORWARD = {"lean": False, "ws_bytes": 0}      # what the last stage forward did (tests)


def _lean(inputs, phys):
    return not torch.is_grad_enabled() or not any(t is not None and t.requires_grad for t in (*inputs, *phys))


class StageFunction(torch.autograd.Function):
    """forward(stage, levels, lean, *inputs, *(W, b per module of the stage)) -> the stage's output slab.
    lean: nothing will ask for a backward pass (torch.no_grad(), or no operand requires a gradient): the forward-only slab
    plan (`_lean_layout`: storage re-used along the op list) and nothing saved."""

    @staticmethod
    def forward(ctx, stage, levels, lean, *ts):
        n_in = stage.n_inputs
        inputs = [F._feat(t) for t in ts[:n_in]]
        phys = ts[n_in:]
        dev = inputs[0].device
        ns = levels[2]
        lean = bool(lean) and F.RELU_RECORD is None
        offs, total = _lean_layout(stage, ns) if lean else _layout(stage.fwd_specs, ns)
        LAST_FORWARD["lean"], LAST_FORWARD["ws_bytes"] = lean, total
        ws = torch.empty(max(total, 256), dtype=torch.uint8, device=dev)
        lv, ch, es, _ = stage.bufs[stage.out_id]
        out = torch.empty((ns[lv], ch), dtype=torch.float32 if es == 4 else torch.bfloat16, device=dev)
        table = (vp * len(stage.bufs))()
        base = ws.data_ptr()
        for i, o in zip(stage.fwd_ws, offs):
            table[i] = base + o
        for i, t in zip(stage.in_ids, inputs):
            blv, bch, bes, _ = stage.bufs[i]
            if t.shape != (ns[blv], bch) or t.element_size() != bes:
                raise L.ScnError(f"executor: input slab {tuple(t.shape)} {t.dtype} where the plan expects {(ns[blv], bch)} x {bes} B")
            table[i] = t.data_ptr()
        table[stage.out_id] = out.data_ptr()
        ptab = (vp * max(len(stage.params), 1))()
        images = []
        f32 = torch.float32
        for k, j in stage.w_entries:
            t = phys[j]
            ptab[k] = (t if (t.dtype is f32 and t.is_contiguous()) else F._f32(t)).data_ptr()
        for k, j in stage.b_entries:
            t = phys[j]
            ptab[k] = 0 if t is None else (t if (t.dtype is f32 and t.is_contiguous()) else F._f32(t)).data_ptr()
        stats = [getattr(stage.mods[mi][0], name) for _, mi, name in stage.stat_entries]
        for (k, _, _), t in zip(stage.stat_entries, stats):
            if t.dtype is not f32 or not t.is_contiguous() or t.device != dev:
                raise L.ScnError("executor: the running statistics of a batch-norm layer must be contiguous fp32 on the slabs' device")
            ptab[k] = t.data_ptr()
        for k, j, cin, cout, n_off, fl in stage.img_entries:
            if lean and fl:                      # a backward-data image: only a backward pass reads it
                continue
            W = phys[j]
            ent = F.packed_entry(W, cin, cout, n_off, fl)
            if ent is None:
                img = F.pack_weights_bf16(W.detach(), cin, cout, n_off, fl)
                ent = (img, img.data_ptr())
            if not images or images[-1] is not ent[0]:
                images.append(ent[0])                # (the pack buffer of a network: one tensor for all its images)
            ptab[k] = ent[1]
        _run(stage, stage.fwd_arr, levels, table, ptab, None, dev)
        if F.RELU_RECORD is not None:
            _record_relu_masks(stage, ns, ws, offs, inputs, out)
        if stage.bn_layers:                      # batch mean / variance of every batch-norm layer, for `run_stage`
            where = dict(zip(stage.fwd_ws, offs))
            handed = []
            for mi, mv, blv in stage.bn_layers:
                c = stage.bufs[mv][1] // 2
                both = ws[where[mv]:where[mv] + 8 * c].view(f32)
                handed.append((stage.mods[mi][0], both[:c], both[c:], ns[blv]))
            _bn_handed.stats = handed
        if lean:
            return out
        ctx.stage, ctx.levels, ctx.table, ctx.ptab = stage, levels, table, ptab
        ctx.stats = stats                        # (evaluation-mode batch norm: the backward reads the running buffers through ptab)
        ctx.phys_shapes = tuple(None if t is None else tuple(t.shape) for t in phys)
        # Everything the pointer tables name travels through save_for_backward: the parameter tensors, the forward workspace,
        # the packed weight images and the input slabs.  They stay alive exactly as long as autograd keeps the graph
        # (retain_graph=True: a second backward reads the same slabs; otherwise they are released when backward ends and a
        # second backward raises autograd's own "backward through the graph a second time" error).
        ctx.save_for_backward(*[t for t in phys if t is not None], ws, *images, *inputs, *([out] if stage.bwd_reads_out else []))
        return out

    @staticmethod
    def backward(ctx, dout):
        kept = ctx.saved_tensors                 # (raises when the graph's buffers have been freed)
        stage, levels, ptab = ctx.stage, ctx.levels, ctx.ptab
        table = type(ctx.table).from_buffer_copy(ctx.table)      # a fresh table per pass: the forward's entries stay as they were
        ns = levels[2]
        dev = dout.device
        lv, ch, es, _ = stage.bufs[stage.dout_id]
        dout = dout.contiguous()
        if dout.element_size() != es:
            dout = dout.to(torch.float32 if es == 4 else torch.bfloat16)
        offs, total = _layout(stage.bwd_specs, ns)
        ws = torch.empty(max(total, 256), dtype=torch.uint8, device=dev)
        base = ws.data_ptr()
        for i, o in zip(stage.bwd_ws, offs):
            table[i] = base + o
        table[stage.dout_id] = dout.data_ptr()
        dins = []
        for i in stage.din_ids:
            blv, bch, bes, _ = stage.bufs[i]
            t = torch.empty((ns[blv], bch), dtype=torch.float32 if bes == 4 else torch.bfloat16, device=dev)
            dins.append(t)
            table[i] = t.data_ptr()
        # gradient regions back to back in one fp32 buffer; the returned gradients are views of it
        shapes = ctx.phys_shapes
        cached = stage.grad_views.get(shapes)
        if cached is None:
            goffs, gtot, views = [], 0, [None] * len(shapes)
            for reg in stage.gregions:
                goffs.append(gtot)
                start = gtot
                for mi, kind in reg:
                    sh = shapes[2 * mi + (kind == "b")]
                    if sh is not None:
                        n = 1
                        for v in sh:
                            n *= v
                        views[2 * mi + (kind == "b")] = (gtot, n, sh)
                        gtot += n
                if gtot == start:                    # (plans are only compiled for layers WITH bias: _require_bias)
                    raise L.ScnError("executor: a gradient region without a tensor (bias=None layer in a compiled stage)")
                gtot = (gtot + 63) & ~63
            cached = stage.grad_views[shapes] = (goffs, gtot, views)
        goffs, gtot, views = cached
        flat = torch.empty(max(gtot, 1), dtype=torch.float32, device=dev)
        gtab = (vp * max(len(stage.gregions), 1))()
        gb = flat.data_ptr()
        for k, o in enumerate(goffs):
            gtab[k] = gb + 4 * o
        scope = getattr(_step_scope, "scope", None)
        late = None
        if scope is not None:
            late = _step_eligible(stage, kept, ctx.needs_input_grad[3 + stage.n_inputs:], scope.pending)
        if late is not None and L.lib().scn_wgrad_step_hold(1) == 1:
            # the C side holds this pass's weight-gradient launches and sums back until the scope's flush: the pass gets a
            # scratch allocation of its own, and the scope keeps what those launches touch
            own = []
            try:
                _run(stage, stage.bwd_arr, levels, table, ptab, gtab, dev, own_scratch=own)
            finally:
                L.lib().scn_wgrad_step_hold(0)
            scope.keep.append((kept, ws, dout, flat, own, levels, table, gtab))
            for j, p in late:
                v = views[j]
                scope.deliver.append((p, flat[v[0]:v[0] + v[1]].view(v[2])))
                scope.pending.add(id(p))
            scope.passes += 1
            return (None, None, None, *dins,
                    *[flat[v[0]:v[0] + v[1]].view(v[2]) if (j in stage.bn_phys and v is not None) else None for j, v in enumerate(views)])
        _run(stage, stage.bwd_arr, levels, table, ptab, gtab, dev, side=True)
        grads = [None if v is None else flat[v[0]:v[0] + v[1]].view(v[2]) for v in views]
        del kept
        return (None, None, None, *dins, *grads)


def _record_relu_masks(stage, ns, ws, offs, inputs, out):
    """functional.RELU_RECORD for a stage (the parity tests' frozen ReLU masks): the sign mask of every slab a forward op of
    the plan applies its fused input ReLU to, in op order -- the order the layer-by-layer path records them in (a residual
    unit: x, then y1; a decoder level: the coarse input of its deconvolution first).  Read from the slabs the executor
    keeps for backward, after the forward launches have been queued."""
    where = dict(zip(stage.fwd_ws, offs))
    ext = dict(zip(stage.in_ids, inputs))
    ext[stage.out_id] = out
    for op in stage.fwd:
        if op.op == OP_RELU:                             # in place: the result has the sign mask of what the ReLU read
            src = op.y
        elif op.op == OP_ADD_RELU:                       # the branch slab the closing activation read
            src = op.x1
        elif op.flags & L.F_RELU_IN:
            src = op.x
        else:
            continue
        lv, ch, es, kind = stage.bufs[src]
        if src in ext:
            t = ext[src]
        else:
            nb = ns[lv] * ch * es
            t = ws[where[src]:where[src] + nb].view(torch.float32 if es == 4 else torch.bfloat16).view(ns[lv], ch)
        F._rec_relu(t)


_bn_handed = threading.local()


def _update_running_stats():
    """The running-statistics update of every batch-norm layer of the stage that just ran, in module order: the statements of
    functional.BatchNormReLUFunction.forward on the batch mean / biased variance the stage computed (views of its workspace)
    and the level's row count -- same operands, same torch kernels, same bits."""
    handed, _bn_handed.stats = getattr(_bn_handed, "stats", None) or (), None
    with torch.no_grad():
        for m, mean, var, n in handed:
            momentum = float(m.momentum)
            m.running_mean.mul_(momentum).add_(mean, alpha=1 - momentum)
            m.running_var.mul_(momentum).add_(var, alpha=(1 - momentum) * (n / (n - 1) if n > 1 else 1.0))


def _require_bias(*mods):
    """Plans write a bias gradient for every conv-type layer they cover (COLSUM / the b region of the WGRAD ops): a layer
    built with bias=False keeps the layer-by-layer path."""
    return all(getattr(m, "bias", None) is not None for m in mods)


def run_stage(stage, levels, inputs, pack=False):
    """Apply a compiled stage: the physical (W, b) of its modules are fetched through `_wb` (zero-padded views of the logical
    parameters where a layer is channel-padded -- autograd carries their gradients back through the pad).
    pack: bf16 storage outside a network-wide `packed_weights` block (a stage of a module tree somebody else built): the
    stage's weight images are packed by ONE launch of its own instead of one per image."""
    phys = []
    for m, cin_phys in stage.mods:
        W, b = (m.weight, m.bias) if isinstance(m, M._BatchNorm) else m._wb(cin_phys)
        phys += [W, b]
    if stage.bn_layers:
        y = StageFunction.apply(stage, levels, _lean(inputs, phys), *inputs, *phys)
        _update_running_stats()
        return y
    if pack and stage.bf16:
        lean = _lean(inputs, phys)
        attr = "_pack_plan_fwd" if lean else "_pack_plan"
        plan = stage.__dict__.get(attr)
        if plan is None:
            jobs = []
            for d in stage.params:
                if d[0] == "img":
                    _, mi, cin, cout, n_off, fl = d
                    if lean and fl:
                        continue
                    m, cin_phys = stage.mods[mi]
                    if getattr(m, "pad_out_to", None) or cin_phys != m.nIn:
                        jobs = None                      # padded layers see fresh padded weight tensors: packed per call
                        break
                    jobs.append((m.weight, cin, cout, n_off, fl))
            plan = F.PackPlan(jobs) if jobs else False
            setattr(stage, attr, plan)
        if plan:
            with F.packed_weights(plan):
                return StageFunction.apply(stage, levels, lean, *inputs, *phys)
    return StageFunction.apply(stage, levels, _lean(inputs, phys), *inputs, *phys)
