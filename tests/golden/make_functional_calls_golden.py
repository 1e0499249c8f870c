"""Writes tests/golden/functional_calls.json: the ordered library calls the convolution-type autograd nodes of
`sparse_rcnn_amd/functional.py` make from Python -- forward, then `torch.autograd.grad` for a chosen subset of the inputs -- for every
node, storage type, bias, switch setting and subset of requested gradients.  tests/test_gpu_functional_calls.py holds the nodes to
the file.  Needs the MI355X: the calls are recorded around real launches.

    python tests/golden/make_functional_calls_golden.py                      # rewrite the file
    python tests/golden/make_functional_calls_golden.py --values --out F     # the calls + a SHA-256 of every output and gradient, to F
    python tests/golden/make_functional_calls_golden.py --compare A B        # every case that differs; exit status 1 if any does

Per call: the entry point's name, every integer argument, and for every pointer argument whether it is NULL
(tools/call_count.py `describe_call`); the size queries `scn_wgrad_scratch_bytes*` are kept, the other quiet names of
tools/call_count.py are not.  Where a call goes through `profiling.timed`, the kernel name and the FLOP and byte figures handed to
the timer stand in front of it.  Entry names, flags, offset counts and `db_offsets` masks do not depend on the toolchain or on the
device, and the row counts follow from the seeded scene, so the file is a committed golden.  `--values` adds digests that do depend
on both: for comparing two commits on ONE machine.

The file was written by the commit BEFORE the parameter-gradient decision of the seven nodes moved into one helper and the two
residual nodes became one; it is never regenerated from later code.

Shapes: two samples on a 24 x 20 x 16 grid with 1500 active voxels each (the cloud of tests/test_gpu_parity.py), 16 channels,
16 -> 32 down and 32 -> 16 up.  The nodes are applied directly, so every case runs layer by layer whatever the step executor's
switches say; they are switched off all the same."""
import argparse
import contextlib
import hashlib
import itertools
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np                                              # noqa: E402
import torch                                                    # noqa: E402

PATH = os.path.join(HERE, "functional_calls.json")
HEADER = ("Written once by tests/golden/make_functional_calls_golden.py on the MI355X, on the commit before functional.py's seven "
          "parameter-gradient sites moved into one helper; never regenerated from later code.")
GRID, N_ACTIVE, BATCH, DUP, C, C2 = (24, 20, 16), 1500, 2, 200, 16, 32
STORAGE = {"f32": torch.float32, "bf16": torch.bfloat16}
# the parametrisation of the test: every case name starts with one of these
GROUPS = [f"{node}/{st}" for node in ("subm3", "subm1", "conv2", "deconv2", "conv4", "deconv4", "nin", "join2", "join2-chained", "join3",
                                       "residual") for st in STORAGE]


def cloud(seed):
    """`_cloud` of tests/test_gpu_parity.py at its default shape."""
    rng = np.random.default_rng(seed)
    cs = []
    for b in range(BATCH):
        lin = rng.choice(GRID[0] * GRID[1] * GRID[2], size=N_ACTIVE, replace=False)
        p = np.stack(np.unravel_index(lin, GRID), 1)
        p = np.concatenate([p, p[rng.integers(0, N_ACTIVE, size=DUP)]])
        rng.shuffle(p)
        cs.append(np.concatenate([p, np.full((len(p), 1), b)], 1))
    return torch.from_numpy(np.concatenate(cs).astype(np.int64)), torch.tensor(GRID), BATCH


class Scene:
    """The one input every case shares, with its rulebooks built before anything is recorded."""

    def __init__(self, device):
        import sparse_rcnn_amd as scn
        coords, size, batch = cloud(5)
        feats = torch.randn(len(coords), 3, generator=torch.Generator().manual_seed(105)).to(device)
        from sparse_rcnn_amd.metadata import Metadata
        # (a depth hint that an earlier forward on this grid size left would build the index structures another way)
        was, Metadata.AUTO_NATIVE = Metadata.AUTO_NATIVE, False
        try:
            x = scn.InputLayer(3, size, mode=4)((coords, feats, batch))
        finally:
            Metadata.AUTO_NATIVE = was
        self.device, self.md, self.size = device, x.metadata, tuple(int(s) for s in size)
        self.n = x.features.shape[0]
        self.md.subm_rulebook(self.size, 1)
        books = [self.md.subm_rulebook(self.size, 3), self.md.strided_rulebook(self.size, (2, 2, 2)),
                 self.md.strided_rulebook(self.size, (4, 4, 4))]
        for rb in books:                    # (rule lists are compacted at their first use: here, not inside whichever case is first)
            rb.rules.in_rows, rb.rules.prefix_host
        self.n_coarse = {2: books[1].n_coarse, 4: books[2].n_coarse}
        torch.cuda.synchronize()

    def leaf(self, seed, shape, dtype=torch.float32, scale=1.0):
        t = torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * scale
        return t.to(self.device).to(dtype)


def subsets(names):
    return [s for k in range(1, len(names) + 1) for s in itertools.combinations(names, k)]


def all_cases(scene):
    """name -> (switches {attribute of functional: value}, inputs {name: tensor}, forward(inputs) -> Y, the inputs that require a
    gradient)."""
    from sparse_rcnn_amd import functional as F
    md, size = scene.md, scene.size
    cases = {}

    def add(group, variant, switches, inputs, forward):
        for want in subsets(list(inputs)):
            cases[f"{group}/{variant}/{'+'.join(want)}"] = (switches, inputs, forward, want)

    for st, dt in STORAGE.items():
        for bias in (True, False):
            bn = "bias" if bias else "nobias"

            def wb(seed, n_off, cin, cout):
                d = {"w": scene.leaf(seed, (n_off, cin, cout) if n_off else (cin, cout), scale=0.1)}
                if bias:
                    d["b"] = scene.leaf(seed + 1, (cout,), scale=0.1)
                return d

            fine, fine2 = scene.leaf(1, (scene.n, C), dt), scene.leaf(2, (scene.n, C2), dt)
            for tiles in (True, False):
                tn = f"{bn}-tiles{int(tiles)}"
                add(f"subm3/{st}", tn, {"USE_TILES": tiles}, dict(x=fine, **wb(10, 27, C, C)),
                    lambda i: F.SubmanifoldConvolutionFunction.apply(i["x"], i["w"], i.get("b"), md, size, 3, True))
                add(f"conv2/{st}", tn, {"USE_TILES": tiles}, dict(x=fine, **wb(20, 8, C, C2)),
                    lambda i: F.ConvolutionFunction.apply(i["x"], i["w"], i.get("b"), md, size, True, (2, 2, 2)))
                add(f"deconv2/{st}", tn, {"USE_TILES": tiles}, dict(x=scene.leaf(3, (scene.n_coarse[2], C2), dt), **wb(30, 8, C2, C)),
                    lambda i: F.DeconvolutionFunction.apply(i["x"], i["w"], i.get("b"), md, size, True, (2, 2, 2)))
            add(f"subm1/{st}", bn, {}, dict(x=fine, **wb(40, 1, C, C)),
                lambda i: F.SubmanifoldConvolutionFunction.apply(i["x"], i["w"], i.get("b"), md, size, 1, False))
            # the 4^3 filter: 64 offsets, the chunked calls
            add(f"conv4/{st}", bn, {}, dict(x=fine, **wb(50, 64, C, C2)),
                lambda i: F.ConvolutionFunction.apply(i["x"], i["w"], i.get("b"), md, size, False, (4, 4, 4)))
            add(f"deconv4/{st}", bn, {}, dict(x=scene.leaf(4, (scene.n_coarse[4], C2), dt), **wb(60, 64, C2, C)),
                lambda i: F.DeconvolutionFunction.apply(i["x"], i["w"], i.get("b"), md, size, False, (4, 4, 4)))
            add(f"nin/{st}", bn, {}, dict(x=fine, **wb(70, 0, C, C2)),
                lambda i: F.NetworkInNetworkFunction.apply(i["x"], i["w"], i.get("b")))
            join = lambda i: F.JoinedNetworkInNetworkFunction.apply(i["w"], i.get("b"), *[i[k] for k in i if k[0] == "x"])
            add(f"join2/{st}", bn, {"FUSED_JOIN": True}, dict(x0=fine, x1=fine2, **wb(80, 0, C + C2, C)), join)
            add(f"join2-chained/{st}", bn, {"FUSED_JOIN": False}, dict(x0=fine, x1=fine2, **wb(80, 0, C + C2, C)), join)
            three = dict(x0=fine, x1=fine2, x2=scene.leaf(5, (scene.n, 8), dt), **wb(90, 0, C + C2 + 8, C))
            xs = tuple(k for k in three if k[0] == "x")
            for want in subsets(["x"] + [k for k in three if k[0] != "x"]):      # the three parts requested together
                cases[f"join3/{st}/{bn}/{'+'.join(want)}"] = ({}, three, join, tuple(k for w in want for k in (xs if w == "x" else (w,))))
            unit = dict(x=fine, w1=scene.leaf(100, (27, C, C), scale=0.1), w2=scene.leaf(102, (27, C, C), scale=0.1))
            if bias:
                unit = dict(x=fine, w1=unit["w1"], b1=scene.leaf(101, (C,), scale=0.1), w2=unit["w2"], b2=scene.leaf(103, (C,), scale=0.1))
            node = F.ResidualBlockFunctionBF16 if st == "bf16" else F.ResidualBlockFunction
            for pair in (True, False):
                add(f"residual/{st}", f"{bn}-pair{int(pair)}", {"WGRAD_PAIR": pair}, unit,
                    lambda i, node=node: node.apply(i["x"], i["w1"], i.get("b1"), i["w2"], i.get("b2"), md, size))
    return cases


@contextlib.contextmanager
def recording(log):
    """Every library call from Python inside the block, and every `profiling.timed`, appended to `log` in order."""
    from call_count import _Counting
    from sparse_rcnn_amd import _lib as L, profiling
    lib, timed = L.lib(), profiling.timed
    value = lambda v: float(v() if callable(v) else v)

    def logging_timed(name, flops, nbytes, fn):
        log.append(f"timed:{name}:{value(flops)!r}:{value(nbytes)!r}")
        return timed(name, flops, nbytes, fn)
    L._lib, profiling.timed = _Counting(lib, log, ("scn_wgrad_scratch_bytes",)), logging_timed
    try:
        yield
    finally:
        L._lib, profiling.timed = lib, timed


@contextlib.contextmanager
def layer_by_layer(switches=()):
    """The step executor's switches off, and the switches of `functional` a case names set, for the block."""
    from sparse_rcnn_amd import functional as F, modules, unet
    held = [(unet.SparseUNet, "EXEC", False), (modules, "TREE_STAGES", False)] + [(F, k, v) for k, v in dict(switches).items()]
    was = [getattr(o, k) for o, k, _ in held]
    for o, k, v in held:
        setattr(o, k, v)
    try:
        yield
    finally:
        for (o, k, _), v in zip(held, was):
            setattr(o, k, v)


def _digest(t):
    t = t.detach().to("cpu").contiguous()
    return hashlib.sha256(f"{t.dtype}{tuple(t.shape)}".encode() + t.reshape(-1).view(torch.uint8).numpy().tobytes()).hexdigest()


def run_case(case, values=False):
    """-> the ordered call list, or with `values` {"calls": the list, "values": {output or gradient: SHA-256}}."""
    switches, inputs, forward, want = case
    # (a node's `needs_input_grad` follows `requires_grad` of what it is handed, not the list `autograd.grad` is given)
    inputs = {k: v.detach().requires_grad_(k in want) for k, v in inputs.items()}
    log = []
    with layer_by_layer(switches), recording(log):
        y = forward(inputs)
        gy = torch.randn(y.shape, generator=torch.Generator().manual_seed(7)).to(y.device).to(y.dtype)
        grads = torch.autograd.grad(y, [inputs[k] for k in want], gy)
        torch.cuda.synchronize()
    if not values:
        return log
    return {"calls": log, "values": {"y": _digest(y), **{"d" + k: _digest(g) for k, g in zip(want, grads)}}}


def compare(a_path, b_path):
    with open(a_path) as f:
        a = json.load(f)["cases"]
    with open(b_path) as f:
        b = json.load(f)["cases"]
    differ = 0
    for name in sorted(set(a) | set(b)):
        if a.get(name) != b.get(name):
            print(f"{name} differs\n    {json.dumps(a.get(name))[:400]}\n    {json.dumps(b.get(name))[:400]}")
            differ += 1
    print(f"{len(set(a) | set(b))} cases, {differ} differing keys")
    return 1 if differ else 0


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--values", action="store_true", help="add a SHA-256 of every output and returned gradient (one machine only)")
    ap.add_argument("--out", default=None, help="write there instead of tests/golden/functional_calls.json (required with --values)")
    ap.add_argument("--compare", nargs=2, metavar=("A.json", "B.json"), default=None)
    args = ap.parse_args()
    if args.compare:
        sys.exit(compare(*args.compare))
    if args.values and not args.out:
        ap.error("--values is for comparing two commits: give --out, the committed file holds no digests")
    scene = Scene(torch.device("cuda", 0))
    done = {name: run_case(case, args.values) for name, case in all_cases(scene).items()}
    with open(args.out or PATH, "w") as f:                      # one line per case
        f.write('{"_header": ' + json.dumps(HEADER) + ',\n"cases": {\n')
        f.write(",\n".join(f" {json.dumps(name)}: {json.dumps(done[name], sort_keys=True)}" for name in sorted(done)))
        f.write("\n}}\n")
    print(f"{len(done)} cases -> {args.out or PATH}")


if __name__ == "__main__":
    main()
