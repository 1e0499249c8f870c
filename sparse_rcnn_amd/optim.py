"""Adam on the library's fused update (scn_adam_many, csrc/scn_optim.hip): the reference's optimizer,
`optim.Adam(learnable_parameter, lr=4e-4, weight_decay=0)` over three parameter groups (scannet_config/run.py:403-416,
1441-1449), stepped once per `batches_per_step` micro-batches (ndsis/training/training.py:458-460) and decayed by
`StepLR(step_size=1, gamma=0.992)` once per epoch (run.py:418,1452).

    from sparse_rcnn_amd.optim import Adam          # in place of torch.optim.Adam: same constructor, same state_dict

The per-element arithmetic is torch.optim.Adam's single-tensor step (include/scn_mi355x.h: scn_adam_many).  All parameters
of a device are updated by one launch per <= 80 tensors; the moments live in ONE flat `exp_avg` and ONE flat `exp_avg_sq`
allocation per device (the per-parameter state tensors are views into them).
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib as L

# one scn_adam_segment record (include/scn_mi355x.h)
SEGMENT = np.dtype([("p", "<u8"), ("g", "<u8"), ("m", "<u8"), ("v", "<u8"), ("n", "<i8"), ("step_size", "<f4"),
                    ("inv_bc2_sqrt", "<f4"), ("weight_decay", "<f4"), ("decay", "<f4")])
ALIGN = 4                               # floats: every parameter's moment slice starts 16-byte aligned


def constants(lr, beta1, beta2, weight_decay, decoupled, step):
    """(step_size, inv_bc2_sqrt, weight_decay, decay) of one segment at step count `step` (after the increment), in double as
    torch.optim.Adam computes them (the table rounds them to float).  torch divides by bias_correction2_sqrt, a host scalar,
    as a multiplication by its reciprocal: the reciprocal is taken here, in double."""
    bias_correction1 = 1 - beta1 ** step
    bias_correction2 = 1 - beta2 ** step
    step_size = lr / bias_correction1
    inv_bc2_sqrt = 1 / bias_correction2 ** 0.5
    if weight_decay != 0 and decoupled:
        return step_size, inv_bc2_sqrt, 0.0, 1 - lr * weight_decay
    return step_size, inv_bc2_sqrt, float(weight_decay), 1.0


def launch(table: np.ndarray, grad_scale: float, beta1: float, beta2: float, eps: float) -> None:
    """scn_adam_many over a SEGMENT table on torch's current stream (the table is copied into the kernel arguments: it may
    be reused as soon as this returns)."""
    if len(table):
        L.check(L.lib().scn_adam_many(table.ctypes.data, len(table), float(grad_scale), float(beta1), float(beta2),
                                      float(eps), L.stream()))


def launches(table: np.ndarray) -> int:
    """Kernel launches scn_adam_many makes for this table."""
    n = C.c_int(0)
    L.check(L.load().scn_adam_launches(table.ctypes.data, len(table), C.byref(n)))
    return n.value


def _check_param(p):
    if not isinstance(p, torch.Tensor):
        raise TypeError("sparse_rcnn_amd.optim.Adam: parameters must be tensors")
    if p.device.type != "cuda":
        raise ValueError("sparse_rcnn_amd.optim.Adam: parameter on %s -- the update runs on the MI355X only (no CPU "
                         "fallback); move the model to the GPU first" % p.device)
    if p.dtype != torch.float32:
        raise ValueError("sparse_rcnn_amd.optim.Adam: fp32 parameters only (got %s)" % p.dtype)
    if not p.is_contiguous():
        raise ValueError("sparse_rcnn_amd.optim.Adam: parameters must be contiguous")


_clip_cache = {}                         # (device index, stream handle) -> [record, scratch]


def clip_buffers(device, scratch_bytes):
    """The record (4 floats) and the scratch of a clip on `device` and torch's current stream there, kept per (device, stream):
    the scratch is allocated again only when a longer table asks for more."""
    with torch.cuda.device(device):
        key = (torch.cuda.current_device(), L.stream())
        hit = _clip_cache.get(key)
        if hit is None:
            hit = _clip_cache[key] = [torch.zeros(4, dtype=torch.float32, device=device), None]
        if hit[1] is None or hit[1].numel() < scratch_bytes:
            hit[1] = torch.empty(max(int(scratch_bytes), 256), dtype=torch.uint8, device=device)
    return hit[0], hit[1]


def clip_grad_norm_(parameters, max_norm, norm_type=2.0, error_if_nonfinite=False, foreach=None):
    """torch.nn.utils.clip_grad_norm_ on the library's two clip kernels (SCN_OP_GRAD_NORM + SCN_OP_GRAD_SCALE, one executor
    call over the gradients where autograd left them): the L2 norm over every `.grad` that is not None, accumulated in double
    in a fixed order, and `grad *= min(1, max_norm / (norm + 1e-6))` in place.  -> the total norm as a 0-dim device tensor, a
    view of the call's record (valid until the next clip on this device and stream); no host wait unless error_if_nonfinite.
    `foreach` is accepted and ignored.  Gradients: fp32, contiguous, on the GPU (ValueError otherwise); L2 only."""
    from . import executor as EX
    if isinstance(parameters, torch.Tensor):
        parameters = [parameters]
    parameters = list(parameters)
    if float(norm_type) != 2.0:
        raise ValueError("sparse_rcnn_amd.optim.clip_grad_norm_: norm_type %r is not implemented, only the L2 norm "
                         "(norm_type=2)" % (norm_type,))
    grads = [p.grad for p in parameters if p.grad is not None]
    if not grads:
        return torch.tensor(0.0)
    dev = grads[0].device
    for g in grads:
        if g.device.type != "cuda":
            raise ValueError("sparse_rcnn_amd.optim.clip_grad_norm_: gradient on %s -- the clip runs on the MI355X only (no CPU "
                             "fallback); move the model to the GPU first" % g.device)
        if g.is_sparse or g.dtype != torch.float32 or g.device != dev or not g.is_contiguous():
            raise ValueError("sparse_rcnn_amd.optim.clip_grad_norm_: gradients must be contiguous fp32 on one device")
    counts = [g.numel() for g in grads]
    record, scratch = clip_buffers(dev, EX.clip_scratch_bytes(counts))
    with torch.cuda.device(dev):
        EX.clip_segments([g.data_ptr() for g in grads], counts, float(max_norm), 1.0, record, scratch)
    if error_if_nonfinite and record[2].item() != 0.0:
        raise RuntimeError(f"The total norm of order {float(norm_type)} for gradients from `parameters` is non-finite, so it "
                           "cannot be clipped. To disable this error and scale the gradients by the non-finite norm anyway, "
                           "set `error_if_nonfinite=False`")
    return record[0]


class _DeviceState:
    """The flat moments of the parameters of one device: slot i = params[i], moments at [off[i], off[i] + n[i])."""

    def __init__(self, params):
        self.params = list(params)
        self.index = {id(p): i for i, p in enumerate(self.params)}
        n = np.array([p.numel() for p in self.params], dtype=np.int64)
        off = np.zeros(len(n), dtype=np.int64)
        if len(n) > 1:
            off[1:] = np.cumsum((n + ALIGN - 1) // ALIGN * ALIGN)[:-1]
        total = int(off[-1] + n[-1]) if len(n) else 0
        dev = self.params[0].device
        self.exp_avg = torch.zeros(total, dtype=torch.float32, device=dev)
        self.exp_avg_sq = torch.zeros(total, dtype=torch.float32, device=dev)
        self.steps = torch.zeros(len(n), dtype=torch.float32)          # `state[p]["step"]` are 0-dim views of this
        self.steps_np = self.steps.numpy()
        self.n, self.off = n, off
        self.m_views = [self.exp_avg[o:o + k].view_as(p) for p, o, k in zip(self.params, off.tolist(), n.tolist())]
        self.v_views = [self.exp_avg_sq[o:o + k].view_as(p) for p, o, k in zip(self.params, off.tolist(), n.tolist())]
        self.table = np.zeros(len(n), dtype=SEGMENT)
        self.table["n"] = n
        self.table["m"] = self.exp_avg.data_ptr() + 4 * off
        self.table["v"] = self.exp_avg_sq.data_ptr() + 4 * off


class Adam(torch.optim.Optimizer):
    """torch.optim.Adam's constructor, state_dict layout and step semantics on the library's fused update.

    Not implemented (ValueError): amsgrad, maximize, capturable, differentiable.  `foreach` and `fused` are accepted and
    recorded (every step is the fused launch).  Parameters: fp32, contiguous, on the GPU."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, amsgrad=False, *, foreach=None,
                 maximize=False, capturable=False, differentiable=False, fused=None, decoupled_weight_decay=False):
        if isinstance(lr, torch.Tensor):
            if lr.numel() != 1:
                raise ValueError("Tensor lr must be 1-element")
            lr = lr.item()
        if not 0.0 <= lr:
            raise ValueError(f"Invalid learning rate: {lr}")
        if not 0.0 <= eps:
            raise ValueError(f"Invalid epsilon value: {eps}")
        betas = tuple(b.item() if isinstance(b, torch.Tensor) else b for b in betas)
        if not 0.0 <= betas[0] < 1.0:
            raise ValueError(f"Invalid beta parameter at index 0: {betas[0]}")
        if not 0.0 <= betas[1] < 1.0:
            raise ValueError(f"Invalid beta parameter at index 1: {betas[1]}")
        if not 0.0 <= weight_decay:
            raise ValueError(f"Invalid weight_decay value: {weight_decay}")
        for name, on in (("amsgrad", amsgrad), ("maximize", maximize), ("capturable", capturable),
                         ("differentiable", differentiable)):
            if on:
                raise ValueError(f"sparse_rcnn_amd.optim.Adam does not implement {name}=True")
        if fused and foreach:
            raise RuntimeError("`fused` and `foreach` cannot be `True` together.")
        defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=amsgrad, maximize=maximize,
                        foreach=foreach, capturable=capturable, differentiable=differentiable, fused=fused,
                        decoupled_weight_decay=decoupled_weight_decay)
        self._dev = {}                                                  # device -> _DeviceState
        super().__init__(params, defaults)

    def add_param_group(self, param_group):
        super().add_param_group(param_group)
        group = self.param_groups[-1]
        try:
            for p in group["params"]:
                _check_param(p)
            for k in ("amsgrad", "maximize", "capturable", "differentiable"):
                if group.get(k):
                    raise ValueError(f"sparse_rcnn_amd.optim.Adam does not implement {k}=True")
        except Exception:
            self.param_groups.pop()
            raise
        if self._dev:                          # parameters added after the moments were laid out: lay them out again
            self._layout()

    def __setstate__(self, state):
        super().__setstate__(state)
        for group in self.param_groups:
            for k, v in (("amsgrad", False), ("maximize", False), ("foreach", None), ("capturable", False),
                         ("differentiable", False), ("decoupled_weight_decay", False), ("fused", None)):
                group.setdefault(k, v)

    # ---- flat moments ----------------------------------------------------------------------------------------
    def _layout(self):
        """(Re)build the flat moments of every device, keeping the state that exists."""
        by_dev = {}
        for g in self.param_groups:
            for p in g["params"]:
                by_dev.setdefault(p.device, []).append(p)
        new = {dev: _DeviceState(ps) for dev, ps in by_dev.items()}
        self._dev = new
        self._adopt()

    def _adopt(self):
        """Make every state entry a view of the flat buffers (copying values in) and zero the slots without state."""
        for ds in self._dev.values():
            ds.exp_avg.zero_()
            ds.exp_avg_sq.zero_()
            for i, p in enumerate(ds.params):
                st = self.state.get(p)
                if not st:
                    ds.steps_np[i] = 0.0
                    continue
                m, v = ds.m_views[i], ds.v_views[i]
                if st["exp_avg"] is not m:
                    m.copy_(st["exp_avg"])
                if st["exp_avg_sq"] is not v:
                    v.copy_(st["exp_avg_sq"])
                step = st["step"]
                ds.steps_np[i] = float(step.item() if isinstance(step, torch.Tensor) else step)
                st["exp_avg"], st["exp_avg_sq"], st["step"] = m, v, ds.steps[i]

    def load_state_dict(self, state_dict):
        """torch's load, then COPY the moments into the flat buffers (torch's default would rebind the state tensors)."""
        super().load_state_dict(state_dict)
        self._layout()

    def state_dict(self):
        """torch.optim.Adam's layout; `step` is a float32 CPU tensor of its own per parameter (a copy)."""
        sd = super().state_dict()
        sd["state"] = {k: dict(v, step=v["step"].clone()) if "step" in v else dict(v) for k, v in sd["state"].items()}
        return sd

    # ---- step ------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def step(self, closure=None):
        """One update of every parameter whose `.grad` is not None (the others, and their step counts, stay as they are)."""
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        if sum(len(ds.params) for ds in self._dev.values()) != sum(len(g["params"]) for g in self.param_groups):
            self._layout()
        rows = {dev: [] for dev in self._dev}
        for group in self.param_groups:
            beta1, beta2 = group["betas"]
            lr = float(group["lr"])
            launch_key = (group["eps"], beta1, beta2)
            consts = {}
            for p in group["params"]:
                g = p.grad
                if g is None:
                    continue
                if g.is_sparse:
                    raise RuntimeError("Adam does not support sparse gradients, please consider SparseAdam instead")
                if g.dtype != torch.float32 or g.device != p.device or not g.is_contiguous() or not p.is_contiguous():
                    raise ValueError("sparse_rcnn_amd.optim.Adam: gradients and parameters must be contiguous fp32 on "
                                     "the parameter's device")
                ds = self._dev.get(p.device)
                i = ds.index.get(id(p)) if ds is not None else None
                if i is None:
                    raise RuntimeError("sparse_rcnn_amd.optim.Adam: a parameter changed device or was added without "
                                       "add_param_group()")
                st = self.state[p]
                if not st:
                    ds.steps_np[i] = 0.0
                    st["step"], st["exp_avg"], st["exp_avg_sq"] = ds.steps[i], ds.m_views[i], ds.v_views[i]
                ds.steps_np[i] += 1.0
                t = float(ds.steps_np[i])
                c = consts.get(t)
                if c is None:
                    c = consts[t] = constants(lr, beta1, beta2, group["weight_decay"], group["decoupled_weight_decay"], t)
                rows[p.device].append((launch_key, i, p.data_ptr(), g.data_ptr(), c))
        for dev, rs in rows.items():
            if not rs:
                continue
            ds = self._dev[dev]
            for key in sorted({r[0] for r in rs}):         # one table per launch-wide (eps, beta1, beta2): usually one
                sel = [r for r in rs if r[0] == key]
                tab = ds.table[np.fromiter((r[1] for r in sel), dtype=np.int64, count=len(sel))]
                tab["p"] = [r[2] for r in sel]
                tab["g"] = [r[3] for r in sel]
                cs = np.array([r[4] for r in sel], dtype=np.float64)
                tab["step_size"], tab["inv_bc2_sqrt"], tab["weight_decay"], tab["decay"] = cs[:, 0], cs[:, 1], cs[:, 2], cs[:, 3]
                with torch.cuda.device(dev):
                    launch(tab, 1.0, key[1], key[2], key[0])
        return loss


class FlatAdam:
    """Adam state of a `dp.FlatParams` (one parameter group): flat moments `exp_avg` / `exp_avg_sq` aligned element for element
    with `FlatParams.flat`, and one step count per parameter.  Driven by `FlatParams.adam_step` (the packed / all-reduced
    gradient: segments over the flat buffers) and `FlatParams.adam_step_single_rank` (one rank: the gradients where autograd
    left them, one segment per parameter).
    Over a CPU buffer the state is laid out and the object constructs -- a step built to be inspected or described without a GPU,
    as an SGD step can be -- and every update (`step_flat`, `step_params`) raises ValueError: there is no CPU fallback."""

    def __init__(self, fp, lr=4e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, decoupled_weight_decay=False):
        if fp.flat.dtype != torch.float32:
            raise ValueError("FlatAdam: fp32 parameters only (got %s)" % fp.flat.dtype)
        if not (0.0 <= lr and 0.0 <= eps and 0.0 <= betas[0] < 1.0 and 0.0 <= betas[1] < 1.0 and 0.0 <= weight_decay):
            raise ValueError("FlatAdam: invalid hyperparameters")
        self.lr, self.betas, self.eps = float(lr), (float(betas[0]), float(betas[1])), float(eps)
        self.weight_decay, self.decoupled_weight_decay = float(weight_decay), bool(decoupled_weight_decay)
        self.exp_avg = torch.zeros_like(fp.flat)
        self.exp_avg_sq = torch.zeros_like(fp.flat)
        self.steps = np.zeros(len(fp.params), dtype=np.float64)      # per parameter, as torch's state["step"]
        self.n = np.array([p.numel() for p in fp.params], dtype=np.int64)
        self.off = np.concatenate([[0], np.cumsum(self.n)[:-1]]).astype(np.int64)
        self.table = np.zeros(len(self.n), dtype=SEGMENT)             # per-parameter segments (the one-rank fast path)
        self.table["n"] = self.n
        self.table["m"] = self.exp_avg.data_ptr() + 4 * self.off
        self.table["v"] = self.exp_avg_sq.data_ptr() + 4 * self.off
        self._p0 = None

    @staticmethod
    def _require_gpu(t):
        if not t.is_cuda:
            raise ValueError("FlatAdam: fp32 parameters on the GPU only (no CPU fallback)")

    def _consts(self, step):
        return constants(self.lr, self.betas[0], self.betas[1], self.weight_decay, self.decoupled_weight_decay, float(step))

    def _fill(self, tab, steps):
        if steps.min() == steps.max():
            tab["step_size"], tab["inv_bc2_sqrt"], tab["weight_decay"], tab["decay"] = self._consts(steps[0])
            return
        cs = np.array([self._consts(t) for t in steps], dtype=np.float64)
        tab["step_size"], tab["inv_bc2_sqrt"], tab["weight_decay"], tab["decay"] = cs[:, 0], cs[:, 1], cs[:, 2], cs[:, 3]

    def step_flat(self, fp):
        """Every parameter advances (the packed gradient holds zeros where no rank produced one): one segment per run of
        parameters with equal step counts over flat / flat_grad -- one segment while all counts agree."""
        self._require_gpu(fp.flat)
        self.steps += 1.0
        cut = np.flatnonzero(np.diff(self.steps)) + 1
        starts = np.concatenate([[0], cut]).astype(np.int64)
        ends = np.concatenate([cut, [len(self.steps)]]).astype(np.int64)
        tab = np.zeros(len(starts), dtype=SEGMENT)
        byte_off = 4 * self.off[starts]
        tab["p"] = fp.flat.data_ptr() + byte_off
        tab["g"] = fp.flat_grad.data_ptr() + byte_off
        tab["m"] = self.exp_avg.data_ptr() + byte_off
        tab["v"] = self.exp_avg_sq.data_ptr() + byte_off
        tab["n"] = self.off[ends - 1] + self.n[ends - 1] - self.off[starts]
        self._fill(tab, self.steps[starts])
        launch(tab, fp.grad_scale, self.betas[0], self.betas[1], self.eps)

    def step_params(self, datas, grads):
        """Parameters whose gradient is None are skipped, their step counts stay (torch.optim.Adam's rule)."""
        self._require_gpu(self.exp_avg)
        if self._p0 != datas[0].data_ptr():
            self.table["p"] = [d.data_ptr() for d in datas]
            self._p0 = datas[0].data_ptr()
        if not all(g.is_contiguous() and g.dtype == torch.float32 for g in grads if g is not None):
            raise ValueError("FlatAdam: gradients must be contiguous fp32")
        if any(g is None for g in grads):
            have = np.array([g is not None for g in grads])
            if not have.any():
                return
            self.steps[have] += 1.0
            tab = self.table[have]
            tab["g"] = [g.data_ptr() for g in grads if g is not None]
            self._fill(tab, self.steps[have])
        else:
            self.steps += 1.0
            tab = self.table
            tab["g"] = [g.data_ptr() for g in grads]
            self._fill(tab, self.steps)
        launch(tab, 1.0, self.betas[0], self.betas[1], self.eps)
