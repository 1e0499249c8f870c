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

Units: every unit of a level is ONE description (`Unit`: a skip around a short branch of activations and SubM convolutions,
optionally closed by an activation), read off the module tree by ONE recogniser (`_units`) and compiled by ONE emitter pair
(`Stage.units_fwd` / `units_bwd`, a walk over the branch's layers).  That covers the plain pre-activation residual unit, the
reference's bottleneck / main-path-ReLU forms, its post-activation units (relu_first=False) and its plain convolution blocks
(use_residuals=False); which of them a ReLU network may compile is `Unit.accepted`.  Input stages come with the activation in
front of the layer, behind it, or dropped (`_stage_relus`; `Stage.act` / `act_bwd`).  Batch-norm networks
(`SparseUNet(batchnorm=True, bn_stages=True)`, or SCN_EXEC_BN=1): the same units and input stages with BatchNorm(Leaky)ReLU
where the ReLU stood.  A batch-norm activation is never folded into the consuming convolution: it is SCN_OP_BN_STATS +
SCN_OP_BN_FWD writing a slab of its own, SCN_OP_BN_BWD on the way back; its batch mean / variance live in the stage workspace
and the host applies the running-statistics update after the forward call (`run_stage`), with the statements
functional.BatchNormReLUFunction uses.

Frozen parts (trainstep.SceneStep(train=...), or any caller that sets requires_grad False): a stage none of whose operands
requires a gradient runs the forward-only slab plan (`_lean`), and a backward pass runs only the ops of the stored list that
what autograd asks for needs (`Stage.backward_pass`: frozen parameters drop the weight-gradient ops, inputs that need no gradient
the backward-data ops nothing else reads); what still runs gives the same bits.

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
from typing import NamedTuple, Optional

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
OP_GRAD_NORM, OP_GRAD_SCALE = 20, 21
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
def _is_relu(m):
    return type(m) is M.ReLU


def _is_bn(m):
    return isinstance(m, M._BatchNorm)


def _is_subm(m):
    return type(m) is M.SubmanifoldConvolution


class Unit(NamedTuple):
    """One unit of a level (unet.py header; module_factory.py:127-218): a skip around a short branch, optionally closed by an
    activation.  Everything the plan compiler and its callers know about a unit is read from these fields."""
    c: int                      # channels the unit takes and gives
    skip: Optional[str]         # None: no skip (a plain block) | "res": x joins in the last convolution's epilogue |
                                # "add": x joins after a branch that ends in its activation (post-activation)
    layers: tuple               # the branch in order: ReLU, BatchNorm(Leaky)ReLU, SubmanifoldConvolution 1^3 | 3^3
    closing: object = None      # the activation behind the join (a plain block: behind its convolution), or None

    @property
    def convs(self):
        return [m for m in self.layers if _is_subm(m)]

    @property
    def has_bn(self):
        return any(_is_bn(m) for m in (*self.layers, self.closing))

    @property
    def is_default(self):
        """x + K2(ReLU(K1(ReLU(x)))), K 3^3: the pre-activation unit every network had before the other forms existed."""
        return (self.skip == "res" and self.closing is None and len(self.layers) == 4 and _is_relu(self.layers[0])
                and _is_relu(self.layers[2]) and len(self.convs) == 2 and all(m.filter_size == 3 for m in self.convs))

    @property
    def tree_form(self):
        """A form the stages of a module tree somebody else built take (modules.py): the default unit, the post-activation
        units and the plain blocks.  The bottleneck / main-path-ReLU units stay layer by layer there."""
        return self.is_default or self.skip != "res"

    def _width_behind(self):
        """Channels behind the branch when c go in; None when a layer does not take what the one before it gives."""
        w = self.c
        for m in self.layers:
            if _is_bn(m) and int(m.nPlanes) != w:
                return None
            if _is_subm(m):
                if m.nIn != w:
                    return None
                w = m.nOut
        return w

    def accepted(self):
        """May a plan be compiled for this unit?  The rules, one place each; a unit that fails one keeps the layer-by-layer path."""
        convs, closing = self.convs, self.closing
        if self._width_behind() != self.c or any(m.filter_size not in (1, 3) or m.groups != 1 for m in convs):
            return False
        if not (closing is None or _is_relu(closing) or (_is_bn(closing) and int(closing.nPlanes) == self.c)):
            return False
        if self.has_bn:
            # batch norm wherever an activation stands (no ReLU left over), at least once inside the branch; any 1^3 / 3^3 chain
            # that returns to c, its convolutions with or without bias, none of them channel-padded
            return (all(_is_bn(m) or _is_subm(m) for m in self.layers) and any(map(_is_bn, self.layers)) and not _is_relu(closing)
                    and not any(m.pad_out_to for m in convs))
        # ReLU networks: the branch is K (ReLU K)* with exactly ONE more ReLU -- in front of it, behind it ("add") or closing the unit
        lead, tail = _is_relu(self.layers[0]), _is_relu(self.layers[-1])
        inner = self.layers[lead:len(self.layers) - tail]
        if not (all(_is_relu(m) or _is_subm(m) for m in self.layers) and len(inner) == 2 * len(convs) - 1
                and all(map(_is_subm, inner[0::2])) and lead + tail + (closing is not None) == 1 and tail == (self.skip == "add")):
            return False
        # branch shapes (3, 3) and (1, 3, 1), a plain block one 3^3 layer; a 3^3 layer keeps its width; every layer with bias
        sizes = tuple(m.filter_size for m in convs)
        if sizes not in (((3,),) if self.skip is None else ((3, 3), (1, 3, 1))):
            return False
        if any(m.bias is None or (m.filter_size == 3 and m.nIn != m.nOut) for m in convs):
            return False
        # channel padding: only the default unit (the mask head's level 0 runs it on zero-padded slabs)
        return self.is_default or not any(m.pad_out_to for m in convs)


def _width_in(layers):
    """Channels the first layer of a branch takes (a ReLU takes any); None: it holds no batch-norm or SubM layer to say so."""
    m = next((m for m in layers if not _is_relu(m)), None)
    return int(m.nPlanes) if _is_bn(m) else (m.nIn if _is_subm(m) else None)


def _units(unit_seq, bn=False):
    """The units of a level as [Unit], or None when one of them is no form a plan is compiled for (`Unit.accepted`).
    unit_seq: a Sequential (or list) of residual units  Sequential(ConcatTable(Identity, Sequential(branch)), AddTable [, act]),
    or use_residuals=False's flat run  [act, K] * n | [K, act] * n  (module_factory.py:186-218).  A flat ReLU run is cut into
    one plain block per convolution; a flat batch-norm run stays one unit (its widths need only return to c at its end).
    bn: batch norm may stand wherever a ReLU may -- then in every unit; without it a batch-norm layer is no form at all."""
    mods = list(unit_seq._modules.values()) if isinstance(unit_seq, torch.nn.Sequential) else list(unit_seq)
    units = []
    if mods and all(_is_relu(m) or _is_bn(m) or _is_subm(m) for m in mods):
        is_act = [not _is_subm(m) for m in mods]
        if len(mods) % 2 or is_act != [is_act[0], not is_act[0]] * (len(mods) // 2):
            return None
        if any(map(_is_bn, mods)):
            units.append(Unit(_width_in(mods), None, tuple(mods)))
        elif is_act[0]:
            units += [Unit(k.nIn, None, (a, k)) for a, k in zip(mods[0::2], mods[1::2])]
        else:
            units += [Unit(k.nIn, None, (k,), a) for k, a in zip(mods[0::2], mods[1::2])]
        mods = []
    for block in mods:
        if not (type(block) is M.Sequential and len(block) in (2, 3) and type(block[0]) is M.ConcatTable
                and type(block[1]) is M.AddTable and len(block[0]._modules) == 2):
            return None
        a, inner = block[0]._modules.values()
        if type(a) is not M.Identity or type(inner) is not M.Sequential:
            return None
        branch = tuple(inner._modules.values())
        if _width_in(branch) is None:
            return None
        units.append(Unit(_width_in(branch), "res" if _is_subm(branch[-1]) else "add", branch, block[2] if len(block) == 3 else None))
    with_bn = [u.has_bn for u in units]
    if (any(with_bn) and not (bn and all(with_bn))) or not all(u.accepted() for u in units):
        return None
    return units


class _Conv(NamedTuple):
    """What the backward walk needs of a branch convolution: its module index, filter size, widths, input slab, whether a ReLU
    sits in its gather, whether it has a bias."""
    mi: int
    k: int
    cin: int
    cout: int
    x: int
    relu_in: bool
    has_b: bool


class _Relu(NamedTuple):
    """A ReLU with an op of its own: slab x holds the mask of its backward (hb: XF_BF16 when that slab is bf16-stored)."""
    level: int
    c: int
    x: int
    hb: int


class _BN(NamedTuple):
    """A batch-norm layer: input slab x, [mean | var] vector mv (training), gamma's params id gp, eps / leakiness as ExecOp bits."""
    level: int
    c: int
    mi: int
    x: int
    mv: int
    gp: int
    eps: int
    leak: int
    fl: int


class _UnitRec(NamedTuple):
    """A compiled unit: its description, its input slab, one record per branch layer that has an op, the closing activation's."""
    unit: Unit
    x: int
    tape: list
    closing: object


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

    # ---- free-standing activations ---------------------------------------------------------------------------------------
    # An activation no convolution's gather absorbs: behind the head of a level, closing a unit or a plain block.  A ReLU is one
    # SCN_OP_RELU in place; its backward (SCN_OP_RELU_BWD) masks by that slab -- y > 0 exactly where the ReLU's input was.  A
    # BatchNorm(Leaky)ReLU layer is SCN_OP_BN_STATS (training mode: batch mean | biased variance -> ONE 2c-float vector of the
    # stage workspace) + SCN_OP_BN_FWD reading slab x and writing a slab of its own, and SCN_OP_BN_BWD (x, dy -> dx and
    # dgamma | dbeta in ONE gradient region) on the way back: scn_bn_stats / scn_bn_fwd / scn_bn_bwd with the arguments
    # functional.BatchNormReLUFunction passes.  gamma and beta sit next to each other in the params table (`w` names gamma);
    # evaluation mode: the running buffers follow them, no statistics op is planned.
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
        return _BN(level, c, mi, x, mv, gp, eps, leak, fl)

    def act(self, level, c, m, x, out=None, fp32=False):
        """The free-standing activation m on slab x -> (slab that holds the result, record for `act_bwd`).  A ReLU works in place
        (x must be `out` where one is asked for); batch norm writes `out`, or a slab of its own.
        fp32: x is an fp32 slab whatever the plan's storage is (the level-0 head of a bf16 network runs in fp32)."""
        if _is_bn(m):
            y = self.buf(level, c, 4) if out is None else out
            return y, self.bn_layer(level, m, x, y)
        hb = 0 if fp32 else self.hb
        self.op(self.fwd, OP_RELU, level, c, 0, x=x, y=x, flags=hb)
        return x, _Relu(level, c, x, hb)

    def act_bwd(self, rec, g, dx=None):
        """Backward of `act` (and of the ReLU that ends a post-activation branch): gradient slab g -> dx, or a slab of its own."""
        hb = 0 if isinstance(rec, _BN) else rec.hb
        if dx is None:
            dx = self.buf(rec.level, rec.c, 2 if hb else 4, "b")
        if isinstance(rec, _BN):
            self.op(self.bwd, OP_BN_BWD, rec.level, rec.c, 0, x=rec.x, m=g, y=dx, x1=rec.mv, w=rec.gp,
                    b=self.gregion((rec.mi, "w"), (rec.mi, "b")), aux=rec.eps, c1=rec.leak, flags=rec.fl)
        else:
            self.op(self.bwd, OP_RELU_BWD, rec.level, rec.c, 0, m=rec.x, x1=g, y=dx, flags=hb)
        return dx

    # ---- units -----------------------------------------------------------------------------------------------------------
    # A unit (`Unit`) compiles by one walk over its branch, forward, and one over the records of that walk, in reverse.  Each op
    # is the call the layer-by-layer path makes for that layer (modules.Sequential), so both paths give the same bits:
    #   ReLU directly in front of a convolution   F_RELU_IN on that convolution -- no slab, no op.  The backward-data op masks by
    #                                             the convolution's input slab (m=), the weight gradient carries F_RELU_IN.
    #   BatchNorm(Leaky)ReLU                      `bn_layer`, a slab of its own, never a flag of the consuming convolution.
    #   last convolution, skip "res"              x joins in its epilogue (r=x).
    #   activation that ends a branch, skip "add" y = x + act(t): a ReLU is ONE SCN_OP_ADD_RELU that leaves the branch slab t as
    #                                             it is -- the mask of the backward; batch norm writes a slab, SCN_OP_ADD joins.
    #   closing activation                        `act` on the unit's result.
    # Backward, the two gradient paths of x meet in an SCN_OP_ADD -- layer by layer autograd adds them -- because the row GEMM has
    # no "residual after the mask" epilogue and a bf16 slab must be rounded before the add to give autograd's bits.  The default
    # pre-activation unit alone does without it (`_unit_bwd`).
    def units_fwd(self, level, c, x, units, out_id=None):
        """units (`_units`) at `c` physical channels on slab x; the last one writes `out_id` when given.  -> (output id, records)"""
        saved = []
        for k, u in enumerate(units):
            x, rec = self._unit_fwd(level, c, x, out_id if k == len(units) - 1 else None, u)
            saved.append(rec)
        return x, saved

    def units_bwd(self, level, c, g, saved, din_id=None):
        """Backward of units_fwd: g = gradient of the last unit's output -> id of the gradient of the first unit's input."""
        for k, rec in enumerate(reversed(saved)):
            g = self._unit_bwd(level, c, g, din_id if k == len(saved) - 1 else None, rec)
        return g

    # (out / dx = None: a slab of the unit's own, asked for where the walk first writes it -- the symbol order plans always had)
    def _unit_fwd(self, level, c, x, out, u):
        def joined():                   # what the join writes: the unit's result, or what a closing batch norm reads
            return self.buf(level, c) if (out is None or _is_bn(u.closing)) else out

        t, w, relu_in, tape = x, c, False, []
        for i, m in enumerate(u.layers):
            last = i == len(u.layers) - 1
            if _is_relu(m) and not last:
                relu_in = True
                continue
            if _is_relu(m):
                end = joined()
                self.op(self.fwd, OP_ADD_RELU, level, c, 0, x=x, x1=t, y=end, flags=self.hb)
                tape.append(_Relu(level, c, t, self.hb))
                t = end
                break
            cout = w if _is_bn(m) else _phys(m)
            dst = joined() if (last and u.skip != "add") else self.buf(level, cout)
            if _is_bn(m):
                tape.append(self.bn_layer(level, m, t, dst))
            else:
                mi = self.mod(m, w)
                wp = self.weight(mi, w, cout, 27, 0, True) if m.filter_size == 3 else self.param("w", mi)
                b = self.param("b", mi) if m.bias is not None else -1       # (None beside batch norm)
                self.op(self.fwd, OP_CONV_SUBM if m.filter_size == 3 else OP_GEMM_IDENT, level, w, cout, x=t, y=dst,
                        r=x if (last and u.skip == "res") else -1, w=wp, b=b, flags=(L.F_RELU_IN if relu_in else 0) | self.hb)
                tape.append(_Conv(mi, m.filter_size, w, cout, t, relu_in, m.bias is not None))
            t, w, relu_in = dst, cout, False
        if u.skip == "add" and _is_bn(u.layers[-1]):
            end = joined()
            self.op(self.fwd, OP_ADD, level, c, 0, x=x, x1=t, y=end, flags=self.hb)
            t = end
        closing = None
        if u.closing is not None:
            t, closing = self.act(level, c, u.closing, t, out=out)
        return t, _UnitRec(u, x, tape, closing)

    def _unit_bwd(self, level, c, g, dx, rec):
        u, x, tape, hb = rec.unit, rec.x, rec.tape, self.hb
        if u.is_default:
            # The benchmarked unit keeps two fusions the general walk has no place for: the skip's gradient enters through the
            # first convolution's backward-data epilogue (F_RESIDUAL_LAST: fp32 accumulators, one rounding -- no SCN_OP_ADD), and
            # both weight gradients leave as ONE SCN_OP_WGRAD2_SUBM whose weight and bias regions hold the pair.
            k1, k2 = tape
            dy1 = self.buf(level, c, kind="b")
            dx = self.buf(level, c, kind="b") if dx is None else dx
            self.op(self.bwd, OP_CONV_SUBM, level, c, c, x=g, y=dy1, m=k2.x, w=self.weight(k2.mi, c, c, 27, BACK, True), flags=BACK | hb)
            self.op(self.bwd, OP_CONV_SUBM, level, c, c, x=dy1, y=dx, m=x, r=g, w=self.weight(k1.mi, c, c, 27, BACK, True),
                    flags=BACK | L.F_RESIDUAL_LAST | hb)
            gw, gb = self.gregion((k1.mi, "w"), (k2.mi, "w")), self.gregion((k1.mi, "b"), (k2.mi, "b"))
            self.op(self.bwd, OP_WGRAD2_SUBM, level, c, c, x=x, y=dy1, x1=k2.x, y1=g, w=gw, b=gb, flags=L.F_RELU_IN | hb)
            return dx
        if rec.closing is not None:
            g = self.act_bwd(rec.closing, g)
        # parameter-gradient ops: a batch-norm unit queues each right behind its backward-data op, a ReLU unit behind the unit's
        # data chain and add (the orders the two kinds of unit always had; the grouped weight-gradient launch sees them as queued)
        t, leaves = g, []
        for i in range(len(tape) - 1, -1, -1):
            r = tape[i]
            dst = dx if (i == 0 and u.skip is None) else None      # (None: a slab of the op's own)
            if not isinstance(r, _Conv):
                t = self.act_bwd(r, t, dst)
                continue
            if dst is None:
                dst = self.buf(level, r.cin, kind="b")
            wp = self.weight(r.mi, r.cout, r.cin, 27, BACK, True) if r.k == 3 else self.param("w", r.mi)
            self.op(self.bwd, OP_CONV_SUBM if r.k == 3 else OP_GEMM_IDENT, level, r.cout, r.cin, x=t, y=dst,
                    m=r.x if r.relu_in else -1, w=wp, flags=BACK | hb)
            if u.has_bn:
                self._conv_wgrad(level, r, t)
            else:
                leaves.append((r, t))
            t = dst
        if u.skip is not None:                              # the two gradient paths of x
            dx = self.buf(level, c, kind="b") if dx is None else dx
            self.op(self.bwd, OP_ADD, level, c, 0, x=t, x1=g, y=dx, flags=hb)
            t = dx
        for leaf in leaves:
            self._conv_wgrad(level, *leaf)
        return t

    def _conv_wgrad(self, level, r, g):
        gw = self.gregion((r.mi, "w"))
        gb = self.gregion((r.mi, "b")) if r.has_b else -1    # (no bias: scn_wgrad_rules, as the layer's own backward)
        self.op(self.bwd, OP_WGRAD_SUBM if r.k == 3 else OP_WGRAD_IDENT, level, r.cin, r.cout, x=r.x, y=g, w=gw, b=gb,
                flags=(L.F_RELU_IN if r.relu_in else 0) | self.hb)

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
        self.grad_views = {}                              # (parameter shapes, regions of the pass) -> (region offsets, total, views)
        self._bwd_passes = {}                             # (inputs need a gradient, parameters need one) -> _BackwardPass
        # a main-path unit that ends the stage: its backward masks by the stage's OUTPUT slab, which then is saved for backward
        self.bwd_reads_out = any(getattr(op, f) == self.out_id for op in self.bwd for f in ("x", "y", "r", "m", "x1", "y1"))
        self._lean_slots()
        covered = sorted(m for reg in self.gregions for m in reg)
        want = sorted((i, k) for i, (m, _) in enumerate(self.mods) for k in ("w", "b")
                      if k == "w" or getattr(m, "bias", None) is not None or not self.bn_phys)
        if covered != want:
            raise RuntimeError("executor plan: every parameter must sit in exactly one gradient region")
        return self


_BUF_FIELDS = ("x", "y", "r", "m", "x1", "y1")
_WGRAD_OPS = (OP_WGRAD_SUBM, OP_WGRAD_DOWN, OP_WGRAD_UP, OP_WGRAD_IDENT)


def _op_io(op):
    """(buffer ids read, buffer ids written, gradient regions written) of one op, as run_op in csrc/scn_exec.hip uses its fields."""
    k = op.op
    if k in (OP_GEMM_IDENT, OP_CONV_SUBM, OP_CONV_CHILD):
        io = (op.x, op.r, op.m), (op.y,), ()
    elif k == OP_RULES_CHILD:
        io = (op.x, op.m), (op.y,), ()
    elif k == OP_ROWS2:                       # y1 >= 0: one source, two destinations (backward-data of the NiN over a JoinTable)
        io = ((op.x,), (op.y, op.y1), ()) if op.y1 >= 0 else ((op.x, op.x1), (op.y,), ())
    elif k in _WGRAD_OPS:
        io = (op.x, op.y), (), (op.w, op.b)
    elif k == OP_WGRAD2_SUBM:
        io = (op.x, op.y, op.x1, op.y1), (), (op.w, op.b)
    elif k == OP_COLSUM:
        io = (op.x,), (), (op.b,)
    elif k in (OP_ADD, OP_ADD_RELU):
        io = (op.x, op.x1), (op.y,), ()
    elif k in (OP_CAST, OP_RELU, OP_BN_STATS):
        io = (op.x,), (op.y,), ()
    elif k == OP_RELU_BWD:
        io = (op.m, op.x1), (op.y,), ()
    elif k == OP_BN_FWD:
        io = (op.x, op.x1), (op.y,), ()
    elif k == OP_BN_BWD:                      # dx and dgamma | dbeta leave one launch
        io = (op.x, op.m, op.x1), (op.y,), (op.b,)
    else:
        raise RuntimeError(f"executor plan: unknown op {k}")
    return tuple(tuple(v for v in part if v >= 0) for part in io)


class _BackwardPass(NamedTuple):
    """What one backward call runs: the stored list, or the part of it that autograd's request needs (`Stage.backward_pass`)."""
    ops: list                   # ExecOp, in the order of `Stage.bwd`
    arr: object                 # the same as a ctypes array
    ws: list                    # ids of the backward workspace slabs a kept op names
    specs: list                 # their (level, row bytes)
    dins: frozenset             # input-gradient ids a kept op writes
    regions: frozenset          # gradient regions a kept op writes


def _backward_pass(self, inputs=True, params=True):
    """The backward pass for a request (do the inputs need a gradient, do the parameters), derived once from the unchanged
    `bwd` list by a reverse liveness pass over WHOLE ops: an op stays when it writes a needed input-gradient slab, a needed
    gradient region or a slab a later kept op reads; an op with several outputs stays whole when any of them is live.  Kept ops
    keep every field and their order, so what still runs gives the bits of the full pass.  (Every slab of a backward list is
    written by one op, so a write ends no liveness here: the pass only ever adds to the live set.)"""
    key = (bool(inputs), bool(params))
    got = self._bwd_passes.get(key)
    if got is not None:
        return got
    if key == (True, True):
        got = _BackwardPass(self.bwd, self.bwd_arr, self.bwd_ws, self.bwd_specs, frozenset(self.din_ids),
                            frozenset(range(len(self.gregions))))
    else:
        live = set(self.din_ids) if key[0] else set()
        keep = [False] * len(self.bwd)
        for t in range(len(self.bwd) - 1, -1, -1):
            reads, writes, regions = _op_io(self.bwd[t])
            if (key[1] and regions) or any(v in live for v in writes):
                keep[t] = True
                live.update(reads)
        ops = [op for op, k in zip(self.bwd, keep) if k]
        named, written, regions = set(), set(), set()
        for op in ops:
            r, w, g = _op_io(op)
            named.update(r, w)
            written.update(w)
            regions.update(g)
        ws = [i for i in self.bwd_ws if i in named]
        got = _BackwardPass(ops, (ExecOp * len(ops))(*ops), ws, [(self.bufs[i][0], self.bufs[i][1] * self.bufs[i][2]) for i in ws],
                            frozenset(i for i in self.din_ids if i in written), frozenset(regions))
    self._bwd_passes[key] = got
    return got


def _backward_ops(self, inputs=True, params=True):
    """The ops a backward pass runs when the stage's inputs / its parameters need a gradient (`backward_pass`), for inspection."""
    return list(self.backward_pass(inputs, params).ops)


Stage.backward_pass = _backward_pass
Stage.backward_ops = _backward_ops


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


CLIP_MAX_SEGS = 80                      # segments per launch of the clip kernels (include/scn_mi355x.h: SCN_OP_GRAD_NORM)


def clip_plan(counts, max_norm, grad_scale):
    """The pseudo-level and the two-op plan of a global-norm clip over segments of `counts` elements: SCN_OP_GRAD_NORM writes
    the record (buffer 0), SCN_OP_GRAD_SCALE reads its coefficient.  -> (ops, levels, prefix): `prefix` is the host int64 array
    the level points to, the caller keeps it alive until the call has returned."""
    counts = [int(n) for n in counts]
    prefix = (i64 * (len(counts) + 1))()
    for i, n in enumerate(counts):
        prefix[i + 1] = prefix[i] + n
    levels = (ExecLevel * 1)()
    levels[0].n = len(counts)
    levels[0].prefix_host = _addr(prefix)
    ops = (ExecOp * 2)(
        ExecOp(OP_GRAD_NORM, 0, 0, 0, 0, -1, 0, -1, -1, -1, -1, _f32_bits(grad_scale), 0, -1, _f32_bits(max_norm), 0),
        ExecOp(OP_GRAD_SCALE, 0, 0, 0, 0, -1, -1, -1, -1, 0, -1, 0, 0, -1, 0, 0))
    return ops, levels, prefix


def clip_scratch_bytes(counts):
    """Scratch of clip_segments, as the library counts it: scn_exec_requirements on the plan (8 bytes per workgroup of the
    partial-sum launches, never less than the executor's 256).  No GPU needed."""
    ops, levels, prefix = clip_plan(counts, 1.0, 1.0)
    scratch, arrival = C.c_int64(0), C.c_int64(0)
    L.check(L.load().scn_exec_requirements(ops, 2, levels, 1, C.byref(scratch), C.byref(arrival)))
    return scratch.value


def clip_launches(counts):
    """Kernel launches of one clip_segments call: the partial sums and the scale take one launch per CLIP_MAX_SEGS non-empty
    segments each, the record one."""
    return 2 * -(-sum(1 for n in counts if n) // CLIP_MAX_SEGS) + 1


def clip_segments(grad_ptrs, counts, max_norm, grad_scale, record, scratch):
    """torch.nn.utils.clip_grad_norm_ (norm_type 2) over fp32 segments as ONE scn_exec_run call on torch's current stream:
    record[0:4] = (|grad_scale| x the L2 norm of all elements, min(1, max_norm / (that + 1e-6)), 1.0 if the sum of squares is not
    finite, 0), then every element is multiplied by record[1] unless it is 1.  Raw addresses and element counts; record: a device
    fp32 tensor of at least 4 elements; scratch: a device uint8 tensor of at least clip_scratch_bytes(counts).  No host wait."""
    ops, levels, prefix = clip_plan(counts, max_norm, grad_scale)
    n = len(counts)
    grads = (vp * max(n, 1))(*[int(p) for p in grad_ptrs])
    table = (vp * 1)(record.data_ptr())
    L.check(L.lib().scn_exec_run(ops, 2, levels, 1, table, None, grads, scratch.data_ptr(), scratch.numel() * scratch.element_size(),
                                 None, L.stream()))


def _lean_layout(stage, ns):
    """-> (offset per forward workspace buffer, total bytes) of the forward-only plan."""
    base, tot = {}, 0
    for (lv, row_bytes), k in stage.lean_classes:
        size = (_rows(ns, lv) * row_bytes + 255) & ~255
        base[(lv, row_bytes)] = (tot, size)
        tot += size * k
    return [base[cls][0] + k * base[cls][1] for cls, k in stage.lean_slot_of], tot


def _phys(m):
    return int(getattr(m, "pad_out_to", None) or m.nOut)


def _stage_relus(stage, bn=False):
    """(lead, trail): the activation MODULE in front of and behind the layer of an input stage (module_factory.py:438-486), each
    None, a ReLU or -- bn -- a batch-norm layer: the conv-type layer itself or a Sequential of just it -- (None, None) --,
    Sequential(act, layer), Sequential(layer, act).  None: anything else."""
    if isinstance(stage, M._ConvBase):
        return (None, None)
    if type(stage) is not M.Sequential:
        return None
    mods = list(stage._modules.values())
    is_layer = [isinstance(m, M._ConvBase) for m in mods]
    if is_layer == [True]:
        return (None, None)
    act = mods[is_layer.index(False)] if sorted(is_layer) == [False, True] else None
    if not (_is_relu(act) or (bn and _is_bn(act))):
        return None
    return (None, act) if is_layer[0] else (act, None)


def compile_encoder_stage(level, head, blocks, cin_phys, bf16, cast_first=False, cast_last=False, in_bf16=False,
                          relus=(None, None), bn_training=True):
    """Encoder level: head (SubM 1^3 at level 0 | Convolution 2^3/2 from level-1) + residual units.
    level 0 in bf16 storage: the head runs in fp32 on the fp32 input and its result is cast (SparseUNet), or -- cast_first,
    the mask branch's input stage -- the input is cast first and the head runs on bf16 rows, or -- in_bf16 -- the input
    slab is bf16-stored already (a SubM 1^3 stage behind a bf16 network in a module tree); cast_last: fp32 output.
    blocks: the level's units (`_units`).  relus (`_stage_relus`): a ReLU in front of the head is a flag of its gather; every
    other activation is free-standing (`Stage.act`) -- a ReLU behind the head works in place on its result, a batch-norm layer
    (fp32 slabs only) reads one slab and writes another: in front, the head gathers the normalised slab; behind, the units
    start from it.
    bn_training: the batch-norm layers of the stage take batch statistics (False: their running buffers)."""
    lead, trail = relus
    if bf16 and (_is_bn(lead) or _is_bn(trail) or any(u.has_bn for u in blocks)):
        raise NotImplementedError("executor: batch norm runs on fp32 slabs")
    lead_fl = L.F_RELU_IN if _is_relu(lead) else 0
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
            if lead is not None or trail is not None:
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
            if _is_bn(lead):
                head_in, lead_rec = st.act(0, cin_phys, lead, IN, fp32=True)
            st.op(st.fwd, OP_GEMM_IDENT, 0, cin_phys, c, x=head_in, y=h, w=st.param("w", mh), b=st.param("b", mh), flags=lead_fl)
            x, head_hb = h, 0
            if trail is not None:
                x, trail_rec = st.act(0, c, trail, h, fp32=True)
            if bf16:
                x = st.buf(0, c)
                st.op(st.fwd, OP_CAST, 0, c, 0, x=h, y=x, flags=XF_BF16)
    else:
        x = st.buf(level, c)
        head_in = IN
        if _is_bn(lead):
            head_in, lead_rec = st.act(level - 1, cin_phys, lead, IN)
        st.op(st.fwd, OP_CONV_CHILD, level - 1, cin_phys, c, x=head_in, y=x, w=st.weight(mh, cin_phys, c, 8, 0, True),
              b=st.param("b", mh), flags=lead_fl | st.hb)
        if trail is not None:
            x, trail_rec = st.act(level, c, trail, x)
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
            if trail is not None:
                gf = st.act_bwd(trail_rec, gf)
            dhead = st.buf(0, cin_phys, 4, "b") if _is_bn(lead) else DIN
            st.op(st.bwd, OP_GEMM_IDENT, 0, c, cin_phys, x=gf, y=dhead, m=IN if lead_fl else -1, w=st.param("w", mh), flags=BACK)
            st.op(st.bwd, OP_WGRAD_IDENT, 0, cin_phys, c, x=head_in, y=gf, w=gw, b=gb, flags=lead_fl)
            if _is_bn(lead):
                st.act_bwd(lead_rec, dhead, DIN)
    else:
        if trail is not None:
            g = st.act_bwd(trail_rec, g)
        dhead = st.buf(level - 1, cin_phys, kind="b") if _is_bn(lead) else DIN
        st.op(st.bwd, OP_RULES_CHILD, level - 1, c, cin_phys, x=g, y=dhead, m=IN if lead_fl else -1, w=st.param("w", mh),
              flags=L.F_W_TRANSPOSED | st.hb)
        st.op(st.bwd, OP_WGRAD_DOWN, level - 1, cin_phys, c, x=head_in, y=g, w=gw, flags=lead_fl | st.hb)
        st.op(st.bwd, OP_COLSUM, level, c, 0, x=g, b=gb, flags=st.hb)
        if _is_bn(lead):
            st.act_bwd(lead_rec, dhead, DIN)
    return st.freeze()


def compile_decoder_stage(level, up, nin, blocks, c_coarse, bf16, *, relus, bn_training=True):
    """Decoder level: ReLU -> Deconvolution 2^3/2 (coarse level+1 -> level) -> JoinTable([up, skip]) -> NetworkInNetwork ->
    units (`_units`).  Inputs: (coarse slab, skip slab).  relus (`_stage_relus`): (ReLU, None) is that form, the ReLU a flag of
    the deconvolution's gather; (None, act) the relu_first=False one, Deconvolution -> act, free-standing (`Stage.act`): a ReLU in
    place on the deconvolution's result, a batch-norm layer (fp32 slabs only) writing the slab the NetworkInNetwork reads.
    Batch norm in front of the deconvolution: not a form the network builder makes (NotImplementedError)."""
    lead, trail = relus
    if _is_bn(lead) or (bf16 and (_is_bn(trail) or any(u.has_bn for u in blocks))):
        raise NotImplementedError("executor: a decoder level takes batch norm behind its deconvolution, on fp32 slabs")
    lead_fl = L.F_RELU_IN if lead is not None else 0
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
    upa = upb                                              # what the NetworkInNetwork reads
    if trail is not None:
        upa, trail_rec = st.act(level, c, trail, upb)
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
    if trail is not None:
        dup = st.act_bwd(trail_rec, dup)
    st.op(st.bwd, OP_CONV_CHILD, level, c, c_coarse, x=dup, y=DIN0, m=IN0 if lead_fl else -1,
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
LAST_BACKWARD = {"ops": 0, "of": 0}                # ops the last stage backward ran, out of the stage's stored list (tests)


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
        n_in = stage.n_inputs
        needs_in, needs_p = ctx.needs_input_grad[3:3 + n_in], ctx.needs_input_grad[3 + n_in:]
        # what autograd asked for decides what runs: frozen parameters drop the weight-gradient ops, inputs that need no gradient
        # the backward-data ops nothing else reads (`Stage.backward_pass`; everything needed: the stored list itself)
        bp = stage.backward_pass(any(needs_in), any(needs_p))
        LAST_BACKWARD["ops"], LAST_BACKWARD["of"] = len(bp.ops), len(stage.bwd)
        if not bp.ops:
            return (None,) * (3 + n_in + len(needs_p))
        table = type(ctx.table).from_buffer_copy(ctx.table)      # a fresh table per pass: the forward's entries stay as they were
        ns = levels[2]
        dev = dout.device
        lv, ch, es, _ = stage.bufs[stage.dout_id]
        dout = dout.contiguous()
        if dout.element_size() != es:
            dout = dout.to(torch.float32 if es == 4 else torch.bfloat16)
        offs, total = _layout(bp.specs, ns)
        ws = torch.empty(max(total, 256), dtype=torch.uint8, device=dev)
        base = ws.data_ptr()
        for i, o in zip(bp.ws, offs):
            table[i] = base + o
        table[stage.dout_id] = dout.data_ptr()
        dins, unasked = [], []
        for i, need in zip(stage.din_ids, needs_in):
            if i not in bp.dins:                 # no kept op writes it (and nobody asked for it)
                dins.append(None)
                continue
            blv, bch, bes, _ = stage.bufs[i]
            t = torch.empty((ns[blv], bch), dtype=torch.float32 if bes == 4 else torch.bfloat16, device=dev)
            dins.append(t if need else None)     # (a slab a kept op writes beside a needed one: it lives until the pass is queued)
            if not need:
                unasked.append(t)
            table[i] = t.data_ptr()
        # the gradient regions of the pass back to back in one fp32 buffer; the returned gradients are views of it
        shapes = ctx.phys_shapes
        all_regions = len(bp.regions) == len(stage.gregions)
        cached = stage.grad_views.get((shapes, None if all_regions else bp.regions))
        if cached is None:
            goffs, gtot, views = [], 0, [None] * len(shapes)
            for k, reg in enumerate(stage.gregions):
                if k not in bp.regions:
                    goffs.append(None)
                    continue
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
            cached = stage.grad_views[(shapes, None if all_regions else bp.regions)] = (goffs, gtot, views)
        goffs, gtot, views = cached
        if not any(needs_p):                     # (a batch-norm backward-data op still writes its dgamma | dbeta: nobody reads them)
            views = [None] * len(shapes)
        flat = torch.empty(max(gtot, 1), dtype=torch.float32, device=dev)
        gtab = (vp * max(len(stage.gregions), 1))()
        gb = flat.data_ptr()
        for k, o in enumerate(goffs):
            if o is not None:
                gtab[k] = gb + 4 * o
        scope = getattr(_step_scope, "scope", None)
        late = None
        if scope is not None and any(needs_p):
            late = _step_eligible(stage, kept, needs_p, scope.pending)
        if late is not None and L.lib().scn_wgrad_step_hold(1) == 1:
            # the C side holds this pass's weight-gradient launches and sums back until the scope's flush: the pass gets a
            # scratch allocation of its own, and the scope keeps what those launches touch
            own = []
            try:
                _run(stage, bp.arr, levels, table, ptab, gtab, dev, own_scratch=own)
            finally:
                L.lib().scn_wgrad_step_hold(0)
            scope.keep.append((kept, ws, dout, flat, own, levels, table, gtab, unasked))
            for j, p in late:
                v = views[j]
                scope.deliver.append((p, flat[v[0]:v[0] + v[1]].view(v[2])))
                scope.pending.add(id(p))
            scope.passes += 1
            return (None, None, None, *dins,
                    *[flat[v[0]:v[0] + v[1]].view(v[2]) if (j in stage.bn_phys and v is not None) else None for j, v in enumerate(views)])
        _run(stage, bp.arr, levels, table, ptab, gtab, dev, side=True)
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
