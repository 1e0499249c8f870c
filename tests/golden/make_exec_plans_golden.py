"""Writes tests/golden/exec_plans.json: what the step executor's plan compiler (sparse_rcnn_amd/executor.py) emits for every
unit form, storage mode and caller, as one SHA-256 per stage -- the file tests/test_exec_plans_cpu.py holds the compiler to.

    python tests/golden/make_exec_plans_golden.py            # rewrite the file
    python tests/golden/make_exec_plans_golden.py --full     # print the records themselves (to diff two commits' output)

The file was written by the commit BEFORE the unit description (`executor.Unit`) replaced the tagged tuples; it is never
regenerated from later code -- running this script on that commit reproduces it byte for byte.  No GPU: plans are compiled from
the module tree alone, and the callers that compile on first use (maskhead.py, modules.py) are driven with slab stand-ins up to
the point where they would build index structures.

A stage's record is its plan with the numbering taken out, so that a compiler may hand out its symbols in another order but
may not change anything the C side acts on:
  buffers      ranked by first appearance over in_ids, out_id, the forward ops (x, y, r, m, x1, y1 in op order), dout_id,
               din_ids, the backward ops; each written as (rank, level, channels, elem bytes, kind)
  parameters   the descriptor instead of the id, its module index replaced by (module rank by first appearance, type name,
               cin_phys); a batch-norm op also lists the descriptors that follow its `w` (scn_exec.hip reads w + 1 .. w + 3)
  regions      the member list instead of the id; which of an op's w / b name a parameter and which a region follows
               scn_exec.hip: both are regions in the weight-gradient ops and SCN_OP_COLSUM, `b` alone in SCN_OP_BN_BWD
  the rest     op, flags, level, cin, cout, c1, aux and the op order verbatim; the sorted (level, row bytes) lists of the two
               workspaces, lean_classes, bwd_reads_out, the number of batch-norm layers
"""
import argparse
import contextlib
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import torch                                                    # noqa: E402

from sparse_rcnn_amd import executor as EX                     # noqa: E402
from sparse_rcnn_amd import modules as M                       # noqa: E402
from sparse_rcnn_amd import unet as U                          # noqa: E402
from sparse_rcnn_amd.maskhead import MaskBranch                # noqa: E402
from sparse_rcnn_amd.tensor import DeferredTensor, SparseConvNetTensor   # noqa: E402

PATH = os.path.join(HERE, "exec_plans.json")
CHANNELS = (32, 64, 96, 128)
FLAGS = [dict(), dict(bottleneck_divisor=4), dict(main_path_relu=True), dict(bottleneck_divisor=4, main_path_relu=True),
         dict(relu_first=False), dict(relu_first=False, bottleneck_divisor=4), dict(drop_input_relu=False),
         dict(use_residuals=False), dict(use_residuals=False, relu_first=False), dict(num_units=1),
         dict(relu_first=False, drop_input_relu=False)]
MODES = {"fp32": (dict(), None), "bf16": (dict(bf16_blocks="all"), None),
         "bn_train": (dict(batchnorm=True, bn_stages=True), True), "bn_eval": (dict(batchnorm=True, bn_stages=True), False)}
BUF_FIELDS = ("x", "y", "r", "m", "x1", "y1")
REGION_OPS = (EX.OP_WGRAD_SUBM, EX.OP_WGRAD2_SUBM, EX.OP_WGRAD_DOWN, EX.OP_WGRAD_UP, EX.OP_WGRAD_IDENT, EX.OP_COLSUM)
BN_OPS = (EX.OP_BN_FWD, EX.OP_BN_BWD)


# ---- the record ------------------------------------------------------------------------------------------------------------
def stage_record(st):
    buf_rank, mod_rank = {}, {}

    def buf(i):
        if i < 0:
            return None
        if i not in buf_rank:
            buf_rank[i] = len(buf_rank)
        return buf_rank[i]

    def mod(mi):
        if mi not in mod_rank:
            mod_rank[mi] = len(mod_rank)
        m, cin_phys = st.mods[mi]
        return [mod_rank[mi], type(m).__name__, cin_phys]

    def param(k):
        if k < 0:
            return None
        d = st.params[k]
        return [d[0], mod(d[1]), *d[2:]]

    def region(k):
        return None if k < 0 else [[mod(mi), which] for mi, which in st.gregions[k]]

    def op_record(op):
        rec = dict(op=op.op, flags=op.flags, level=op.level, cin=op.cin, cout=op.cout, c1=op.c1, aux=op.aux)
        for f in BUF_FIELDS:
            rec[f] = buf(getattr(op, f))
        if op.op in REGION_OPS:
            rec["w"], rec["b"] = region(op.w), region(op.b)
        elif op.op in BN_OPS:                       # gamma; beta and (evaluation mode) the running buffers follow it
            rec["w"] = [param(op.w + k) for k in range(2 if op.x1 >= 0 else 4)]
            rec["b"] = region(op.b) if op.op == EX.OP_BN_BWD else param(op.b)
        else:
            rec["w"], rec["b"] = param(op.w), param(op.b)
        return rec

    ins = [buf(i) for i in st.in_ids]
    out = buf(st.out_id)
    fwd = [op_record(op) for op in st.fwd]
    dout = buf(st.dout_id)
    dins = [buf(i) for i in st.din_ids]
    bwd = [op_record(op) for op in st.bwd]
    return dict(bf16=st.bf16, n_inputs=st.n_inputs, in_ids=ins, out_id=out, dout_id=dout, din_ids=dins,
                bufs=[[r, *st.bufs[i]] for i, r in sorted(buf_rank.items(), key=lambda kv: kv[1])], fwd=fwd, bwd=bwd,
                fwd_ws=sorted(list(s) for s in st.fwd_specs), bwd_ws=sorted(list(s) for s in st.bwd_specs),
                lean_classes=[[list(cls), k] for cls, k in st.lean_classes], bwd_reads_out=bool(st.bwd_reads_out),
                bn_layers=len(st.bn_layers))


def digest(rec):
    sha = hashlib.sha256(json.dumps(rec, sort_keys=True, separators=(",", ":")).encode()).hexdigest()
    return dict(sha256=sha, fwd=len(rec["fwd"]), bwd=len(rec["bwd"]))


# ---- SparseUNet ------------------------------------------------------------------------------------------------------------
def _name(flags):
    return ",".join(f"{k}={v}" for k, v in flags.items()) or "default"


def unet_stages(net, training=None):
    """The stages of a network's plan in level order (encoder, then decoder), or None when the network takes no plan."""
    plan = net._exec_plan(training) if training is not None else net._exec_plan()
    if not plan:
        return None
    return [s for s in plan["enc"] + plan["dec"] if s is not None]


def unet_cases():
    for mode, (kw, training) in MODES.items():
        for flags in FLAGS:
            stages = unet_stages(U.SparseUNet(7, CHANNELS, **kw, **flags), training)
            assert stages, (mode, flags)
            yield f"unet/{mode}/{_name(flags)}", stages
    for mode in ("fp32", "bf16"):                 # the mask head's internal U-Net: level 0 zero-padded from 23 to 24 channels
        yield f"unet_padded/{mode}", unet_stages(U.SparseUNet(23, (23, 32, 48), identity_first=True, **MODES[mode][0]))


def _first_unit(net):
    """(unit, its branch) of the first residual unit of encoder level 1."""
    unit = net.encoder[1][1][0]
    return unit, unit[0][1]


def refused_cases():
    """Trees the plan compiler must leave to the layer-by-layer path: recorded as null."""
    def conv_at(branch):
        return next(i for i, m in enumerate(branch) if isinstance(m, M.SubmanifoldConvolution))

    net = U.SparseUNet(7, (32, 64))
    _, branch = _first_unit(net)
    branch[conv_at(branch)].bias = None
    yield "refused/bias_free_convolution", unet_stages(net)

    net = U.SparseUNet(7, (32, 64))
    _, branch = _first_unit(net)
    branch[conv_at(branch)] = M.SubmanifoldConvolution(3, 64, 64, 3, True, groups=2)
    yield "refused/groups", unet_stages(net)

    net = U.SparseUNet(7, (32, 64), bottleneck_divisor=4)
    _, branch = _first_unit(net)
    [m for m in branch if isinstance(m, M.SubmanifoldConvolution)][-1].pad_out_to = 72
    yield "refused/pad_out_to", unet_stages(net)

    net = U.SparseUNet(7, (32, 64))
    unit, branch = _first_unit(net)
    i = [k for k, m in enumerate(branch) if isinstance(m, M.SubmanifoldConvolution)][-1]
    branch[i] = M.SubmanifoldConvolution(3, 64, 64, 1, True)
    yield "refused/branch_3_1", unet_stages(net)

    net = U.SparseUNet(7, (32, 64), batchnorm=True, bn_stages=True)
    _, branch = _first_unit(net)
    branch[[k for k, m in enumerate(branch) if isinstance(m, M._BatchNorm)][-1]] = M.ReLU()
    yield "refused/relu_in_batchnorm_unit", unet_stages(net, True)


# ---- callers that compile on first use ----------------------------------------------------------------------------------------
class _Slab:
    """Stands where a device slab does while a caller decides whether and what to compile."""
    is_cuda = True

    def __init__(self, rows, channels, dtype):
        self.shape, self.dtype = (rows, channels), dtype

    def dim(self):
        return 2


class _Metadata:
    def cached_strided_rulebook(self, size):
        return True


@contextlib.contextmanager
def _no_levels():
    """The callers compile, then ask for the index structures of their levels: none here, so they stop right behind the plan."""
    orig = EX.build_levels
    EX.build_levels = lambda *a, **k: None
    try:
        yield
    finally:
        EX.build_levels = orig


def mask_input_cases():
    for mode, bf16 in (("fp32", False), ("bf16", True)):
        branch = MaskBranch(32, 7, bf16_blocks=bf16)
        fmap = SparseConvNetTensor(features=_Slab(64, 32, torch.float32), metadata=_Metadata(), spatial_size=torch.tensor([8, 8, 8]))
        with _no_levels():
            assert branch._input_stage_exec(fmap) is None
        yield f"mask_input/{mode}", [branch.__dict__["_input_stage"]]


TREE_FORMS = {"default": dict(), "post": dict(relu_first=False), "post_bottleneck": dict(relu_first=False, bottleneck_divisor=4),
              "plain_pre": dict(use_residuals=False), "plain_post": dict(use_residuals=False, relu_first=False)}


def _tree_units(c, form):
    return U.units(c, 2, **TREE_FORMS[form])


def tree_cases():
    """Encoder and decoder levels of a module tree somebody else built (modules._enc_stage / _dec_stage)."""
    size = torch.tensor([8, 8, 8])
    for form in TREE_FORMS:
        relu_first = TREE_FORMS[form].get("relu_first", True)
        for level, head in ((0, lambda: M.SubmanifoldConvolution(3, 16, 32, 1, True)),
                            (1, lambda: M.Convolution(3, 16, 32, (2, 2, 2), (2, 2, 2), True))):
            for in16 in ((False, True) if form == "default" else (False,)):
                stages = {"bare": lambda: M.Sequential(head())}
                if not in16:                        # the input stage with its ReLU on the side relu_first puts it (fp32 slabs only)
                    stages["act"] = lambda: U.input_stage(head(), False, relu_first)
                for stage_name, make in stages.items():
                    seq = M.Sequential(make(), _tree_units(32, form))
                    assert M._kind(seq) == "enc"
                    x = SparseConvNetTensor(features=_Slab(64, 16, torch.bfloat16 if in16 else torch.float32),
                                            metadata=_Metadata(), spatial_size=size)
                    with _no_levels():
                        assert M._enc_stage(seq, x) is NotImplemented
                    (st,) = seq.__dict__["_stages"].values()
                    yield f"tree_enc/{form}/level{level}/{stage_name}/{'bf16' if in16 else 'fp32'}_in", [st]
        for in16 in ((False, True) if form == "default" else (False,)):
            dtype = torch.bfloat16 if in16 else torch.float32
            md = _Metadata()
            deconv, nin = M.Deconvolution(3, 64, 32, (2, 2, 2), (2, 2, 2), True), M.NetworkInNetwork(64, 32, True)
            coarse = SparseConvNetTensor(features=_Slab(8, 64, dtype), metadata=md, spatial_size=size // 2)
            skip = SparseConvNetTensor(features=_Slab(64, 32, dtype), metadata=md, spatial_size=size)
            # the calls of the reference's reuniter: input stage and channel changer stay pending, the units compile the level
            x = nin(M.JoinTable()([U.input_stage(deconv, False, relu_first)(coarse), skip]))
            seq = _tree_units(32, form)
            assert M._kind(seq) == "units" and isinstance(x, DeferredTensor) and x.pending
            with _no_levels():
                assert M._dec_stage(seq, x) is NotImplemented
            (st,) = seq.__dict__["_stages"].values()
            yield f"tree_dec/{form}/{'bf16' if in16 else 'fp32'}", [st]


def all_cases():
    for gen in (unet_cases, mask_input_cases, tree_cases, refused_cases):
        for name, stages in gen():
            yield name, None if stages is None else [stage_record(st) for st in stages]


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--full", action="store_true", help="print every record instead of writing the digests")
    args = ap.parse_args()
    if args.full:
        for name, recs in all_cases():
            for k, rec in enumerate(recs or [None]):
                print(json.dumps({"case": name, "stage": k, "record": rec}, sort_keys=True))
        return
    out = {name: None if recs is None else [digest(r) for r in recs] for name, recs in all_cases()}
    with open(PATH, "w") as f:
        json.dump(out, f, indent=0, sort_keys=True, separators=(",", ":"))
        f.write("\n")
    print(f"{PATH}: {len(out)} cases, {sum(len(v) for v in out.values() if v)} stages")


if __name__ == "__main__":
    main()
