"""Adam update bandwidth on the MI355X (profiles/adam_bw.txt).

On the parameter lists of cfg 2 and cfg 5 (built by trainstep.SceneStep) times, with HIP events after warm-up:
  scn_adam_many on the per-parameter list (FlatParams.adam_step_single_rank's fast path), the flat single-segment form
  (FlatParams.adam_step), torch.optim.Adam(foreach=True) and torch.optim.Adam(fused=True) on the same tensors;
then one full cfg 2 fp32 SceneStep with each optimizer.  Effective bandwidth counts 28 B per parameter (p, g, m, v read;
p, m, v written).

    python tools/adam_bw.py [--iters 50] [--steps 30]
"""
from __future__ import annotations

import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402


def _events_us(fn, iters, warmup=10):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    host = (time.perf_counter() - t0) / iters * 1e6
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters * 1e3, host


def _kernels(fn):
    """GPU kernels one call launches (torch profiler), or None."""
    try:
        from torch.autograd import DeviceType
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        return sum(1 for e in prof.events() if e.device_type == DeviceType.CUDA)
    except Exception:                                   # noqa: BLE001  (a profiler that cannot start: not counted)
        return None


def update_table(workload, iters):
    from sparse_rcnn_amd import optim
    from sparse_rcnn_amd.trainstep import SceneStep
    job = SceneStep(workload, prefetch=False, optimizer="adam")
    fp, adam = job.flat, job.adam
    n = fp.flat.numel()
    gen = torch.Generator(device=fp.flat.device).manual_seed(0)
    grads = [torch.randn(p.shape, generator=gen, device=p.device) for p in fp.params]
    fp.flat_grad.normal_(generator=gen)
    for p, g in zip(fp.params, grads):
        p.grad = g
    adam.lr = 1e-12                                    # the timed updates leave the parameters where they are (almost)
    rows = []

    def per_param():
        adam.step_params(fp._datas, grads)

    def flat():
        adam.step_flat(fp)
    per_param()                                        # (fills the gradient pointers of the table)
    tab = adam.table.copy()
    rows.append(("scn_adam_many, per-parameter list", per_param, optim.launches(tab)))
    one = tab[:1].copy()
    one["n"] = n
    rows.append(("scn_adam_many, flat single segment", flat, optim.launches(one)))
    params = [p for p in fp.params]
    for kind, kw in (("torch.optim.Adam(foreach=True)", dict(foreach=True)), ("torch.optim.Adam(fused=True)", dict(fused=True))):
        opt = torch.optim.Adam(params, lr=1e-12, **kw)
        opt.step()
        rows.append((kind, opt.step, None))
    out = [f"{workload}: {len(fp.params)} parameter tensors, {n} parameters ({28 * n / 1e6:.1f} MB moved per update)"]
    for name, fn, launches in rows:
        us, host = _events_us(fn, iters)
        k = launches if launches is not None else _kernels(fn)
        out.append(f"  {name:<40s} {us:9.1f} us  {28 * n / us / 1e6:6.2f} TB/s  launches {k if k is not None else '?':>4}  "
                   f"(host {host:7.1f} us per call)")
    for p in fp.params:
        p.grad = None
    del job, fp, adam, grads, params
    torch.cuda.empty_cache()
    return out


def scene_steps(steps):
    from sparse_rcnn_amd.trainstep import SceneStep
    out = ["cfg2 fp32 SceneStep (rulebooks + fwd + bwd + update), mean over %d steps after 5 warm-up steps:" % steps]
    for opt in ("sgd", "adam"):
        job = SceneStep("cfg2", optimizer=opt)
        for _ in range(5):
            job.step()
        job.finish()
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(steps):
            job.step()
        job.finish()
        b.record()
        torch.cuda.synchronize()
        ok = bool(torch.isfinite(job.flat.flat).all())
        out.append(f"  optimizer={opt:<5s} {a.elapsed_time(b) / steps:7.3f} ms per step  (lr {job.lr:g}, parameters finite: {ok})")
        del job
        torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--workloads", default="cfg2,cfg5")
    a = ap.parse_args()
    lines = [f"# tools/adam_bw.py on {torch.cuda.get_device_name(0)}, torch {torch.__version__}"]
    for w in a.workloads.split(","):
        lines += update_table(w, a.iters)
    lines += scene_steps(a.steps)
    print("\n".join(lines), flush=True)


if __name__ == "__main__":
    main()
