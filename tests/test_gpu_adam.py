"""GPU: the fused Adam (csrc/scn_optim.hip, sparse_rcnn_amd.optim, FlatParams.adam_step*, SceneStep(optimizer="adam"))
against torch.optim.Adam(foreach=False) on fp32 copies -- the reference's optimizer (scannet_config/run.py:403-416,1449)."""
import gc
import io

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SIZES = (1, 3, 5, 4096, 1_000_003)


def _key(x):
    """Float bits -> an integer order in which neighbouring floats differ by 1."""
    i = x.contiguous().view(torch.int32).to(torch.int64)
    return torch.where(i < 0, -(i & 0x7FFFFFFF), i)


def _ulps(a, b):
    return (_key(a.float()) - _key(b.float())).abs().max().item() if a.numel() else 0


def _rel_l2(a, b):
    return ((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-30)).item()


def _grads(shapes, step, device, seed=0):
    g = torch.Generator(device=device).manual_seed(seed * 1000 + step)
    return [torch.randn(s, generator=g, device=device) for s in shapes]


def _make(device, with_views=True, seed=0):
    """Parameters of every size of SIZES plus three views into one buffer at float offsets 1, 2, 3."""
    g = torch.Generator(device=device).manual_seed(seed)
    ps = [torch.randn(n, generator=g, device=device) for n in SIZES]
    if with_views:
        buf = torch.randn(4 + 997 + 1000 + 5 + 8, generator=g, device=device)
        ps += [buf[1:998], buf[1002:2002], buf[2003:2008]]          # float offsets 1, 2 and 3 (mod 4): unaligned
    return ps


def _pair(device, groups_lr=(1e-3, 3e-3), with_views=True, **kw):
    """(ours, torch's, our params, torch's params): two groups with different lr, identical initial values."""
    from sparse_rcnn_amd.optim import Adam
    base = _make(device, with_views)
    ours = [torch.nn.Parameter(t) for t in base]                    # (views stay views: Parameter aliases its data)
    ref = [torch.nn.Parameter(t.detach().clone()) for t in base]
    half = len(ours) // 2

    def groups(ps):
        return [{"params": ps[:half], "lr": groups_lr[0]}, {"params": ps[half:], "lr": groups_lr[1]}]
    return Adam(groups(ours), **kw), torch.optim.Adam(groups(ref), foreach=False, **kw), ours, ref


def _compare_rel(oa, ra, ours, ref):
    for p, q in zip(ours, ref):
        sp, sq = oa.state.get(p, {}), ra.state.get(q, {})
        assert bool(sp) == bool(sq)
        assert _rel_l2(p.detach(), q.detach()) <= 1e-6
        if sp:
            assert sp["step"].item() == sq["step"].item()
            assert _rel_l2(sp["exp_avg"], sq["exp_avg"]) <= 1e-6 and _rel_l2(sp["exp_avg_sq"], sq["exp_avg_sq"]) <= 1e-6


def _compare_state(oa, ra, ours, ref, ulp=2):
    for p, q in zip(ours, ref):
        sp, sq = oa.state.get(p, {}), ra.state.get(q, {})
        assert bool(sp) == bool(sq)
        assert _ulps(p.detach(), q.detach()) <= ulp, ("p", p.numel(), _ulps(p.detach(), q.detach()))
        if sp:
            assert sp["step"].item() == sq["step"].item()
            assert _ulps(sp["exp_avg"], sq["exp_avg"]) <= ulp, ("m", p.numel())
            assert _ulps(sp["exp_avg_sq"], sq["exp_avg_sq"]) <= ulp, ("v", p.numel())


@pytest.mark.parametrize("wd,decoupled", [(0.0, False), (0.01, False), (0.0, True), (0.01, True)])
def test_one_step_then_25_steps_match_torch(gpu, wd, decoupled):
    oa, ra, ours, ref = _pair(gpu, weight_decay=wd, decoupled_weight_decay=decoupled)
    shapes = [p.shape for p in ours]
    for step in range(25):
        for p, q, g in zip(ours, ref, _grads(shapes, step, gpu)):
            p.grad, q.grad = g, g.clone()
        oa.step()
        ra.step()
        if step == 0:
            torch.cuda.synchronize()
            _compare_state(oa, ra, ours, ref)
    for p, q in zip(ours, ref):
        assert _rel_l2(p.detach(), q.detach()) <= 1e-6
        assert _rel_l2(oa.state[p]["exp_avg"], ra.state[q]["exp_avg"]) <= 1e-6
        assert _rel_l2(oa.state[p]["exp_avg_sq"], ra.state[q]["exp_avg_sq"]) <= 1e-6


@pytest.mark.parametrize("offset", [0, 1, 2, 3])
def test_kernel_segments_at_float_offsets(gpu, offset):
    """scn_adam_many on raw segments whose four pointers share a float offset (scalar head, 16-byte body, scalar tail) and
    on segments where only p is offset (scalar path), against torch's single-tensor arithmetic."""
    from sparse_rcnn_amd import optim
    sizes = SIZES + (4097, 4099, 8191)
    g0 = torch.Generator(device=gpu).manual_seed(7 + offset)
    bufs = {k: torch.randn(offset + sum(sizes) + 4 * len(sizes), generator=g0, device=gpu) for k in "pgmv"}
    bufs["v"] = bufs["v"].abs()
    shifted = torch.randn(offset + sum(sizes) + 4 * len(sizes), generator=g0, device=gpu)      # p of the mixed segments
    ref = {k: b.clone() for k, b in bufs.items()}
    t = np.zeros(2 * len(sizes), dtype=optim.SEGMENT)
    ref_mixed = []
    off = offset
    lr, b1, b2, eps, step = 2e-3, 0.9, 0.999, 1e-8, 3
    c = optim.constants(lr, b1, b2, 0.0, False, step)
    for j, n in enumerate(sizes):
        for k in "pgmv":
            t[k][j] = bufs[k].data_ptr() + 4 * off
        t["n"][j] = n
        # mixed alignment: p at offset+1 of its own buffer, g / m / v shared with nothing (fresh copies)
        g2 = bufs["g"][off:off + n].clone()
        m2 = bufs["m"][off:off + n].clone()
        v2 = bufs["v"][off:off + n].clone()
        p2 = shifted[off + 1:off + 1 + n]                            # disjoint: off advances by n + 3
        ref_mixed.append((p2.clone(), g2, m2.clone(), v2.clone(), p2, m2, v2))
        t["p"][len(sizes) + j], t["g"][len(sizes) + j] = p2.data_ptr(), g2.data_ptr()
        t["m"][len(sizes) + j], t["v"][len(sizes) + j] = m2.data_ptr(), v2.data_ptr()
        t["n"][len(sizes) + j] = n
        off += n + 3
    t["step_size"], t["inv_bc2_sqrt"], t["weight_decay"], t["decay"] = c
    optim.launch(t, 1.0, b1, b2, eps)
    torch.cuda.synchronize()

    def torch_adam(p, g, m, v):
        m.lerp_(g, 1 - b1)
        v.mul_(b2).addcmul_(g, g, value=1 - b2)
        bc1, bc2 = 1 - b1 ** step, 1 - b2 ** step
        denom = (v.sqrt() / (bc2 ** 0.5)).add_(eps)
        p.addcdiv_(m, denom, value=-(lr / bc1))

    off = offset
    for j, n in enumerate(sizes):
        sl = slice(off, off + n)
        p, g, m, v = (ref[k][sl] for k in "pgmv")
        torch_adam(p, g, m, v)
        for k, want in zip("pmv", (p, m, v)):
            assert _ulps(bufs[k][sl], want) <= 2, (k, n, offset)
        off += n + 3
    assert torch.equal(bufs["g"], ref["g"])                        # g is read only
    for p0, g2, m0, v0, p2, m2, v2 in ref_mixed:
        torch_adam(p0, g2, m0, v0)
        assert _ulps(p2, p0) <= 2 and _ulps(m2, m0) <= 2 and _ulps(v2, v0) <= 2


def test_sparse_gradients_skip_like_torch(gpu):
    oa, ra, ours, ref = _pair(gpu)
    shapes = [p.shape for p in ours]
    for step in range(6):
        grads = _grads(shapes, step, gpu, seed=3)
        before = [p.detach().clone() for p in ours]
        skipped = [i for i in range(len(ours)) if (i + step) % 3 == 0]
        for i, (p, q, g) in enumerate(zip(ours, ref, grads)):
            p.grad, q.grad = (None, None) if i in skipped else (g, g.clone())
        oa.step()
        ra.step()
        torch.cuda.synchronize()
        for i in skipped:
            assert torch.equal(ours[i].detach(), before[i])
        if step == 0:
            _compare_state(oa, ra, ours, ref)
        _compare_rel(oa, ra, ours, ref)
    assert sorted(oa.state[p]["step"].item() for p in ours) == sorted(ra.state[q]["step"].item() for q in ref)


def test_step_lr_schedule_matches_torch(gpu):
    oa, ra, ours, ref = _pair(gpu, with_views=False)
    so = torch.optim.lr_scheduler.StepLR(oa, step_size=1, gamma=0.992)
    sr = torch.optim.lr_scheduler.StepLR(ra, step_size=1, gamma=0.992)
    shapes = [p.shape for p in ours]
    k = 0
    for epoch in range(5):
        for _ in range(3):
            for p, q, g in zip(ours, ref, _grads(shapes, k, gpu, seed=5)):
                p.grad, q.grad = g, g.clone()
            oa.step()
            ra.step()
            k += 1
        so.step()
        sr.step()
        assert so.get_last_lr() == sr.get_last_lr()
        assert [g["lr"] for g in oa.param_groups] == [g["lr"] for g in ra.param_groups]
    for p, q in zip(ours, ref):
        assert _rel_l2(p.detach(), q.detach()) <= 1e-6


def _roundtrip(sd):
    b = io.BytesIO()
    torch.save(sd, b)
    b.seek(0)
    return torch.load(b, weights_only=False)


def _run(opt, ps, steps, start, gpu):
    shapes = [p.shape for p in ps]
    for k in range(start, start + steps):
        for p, g in zip(ps, _grads(shapes, k, gpu, seed=9)):
            p.grad = g
        opt.step()


def test_checkpoints_load_both_ways(gpu):
    from sparse_rcnn_amd.optim import Adam
    base = [t.detach().clone() for t in _make(gpu, with_views=False)]

    def fresh(cls, **kw):
        ps = [torch.nn.Parameter(t.clone()) for t in base]
        return cls([{"params": ps[:2]}, {"params": ps[2:], "lr": 2e-3}], lr=1e-3, weight_decay=0.01, **kw), ps

    stay, ps_stay = fresh(Adam)
    _run(stay, ps_stay, 5, 0, gpu)
    # ours -> torch
    a, pa = fresh(Adam)
    _run(a, pa, 3, 0, gpu)
    sd = a.state_dict()
    assert set(sd["state"][0].keys()) == {"step", "exp_avg", "exp_avg_sq"}
    assert sd["state"][0]["step"].dtype == torch.float32 and sd["state"][0]["step"].device.type == "cpu"
    t, pt = fresh(torch.optim.Adam, foreach=False)
    with torch.no_grad():
        for p, q in zip(pt, pa):
            p.copy_(q)
    t.load_state_dict(_roundtrip(sd))
    _run(t, pt, 2, 3, gpu)
    _run(a, pa, 2, 3, gpu)
    for p, q, r in zip(pt, pa, ps_stay):
        assert torch.equal(q.detach(), r.detach())
        assert _rel_l2(p.detach(), r.detach()) <= 1e-6
    # torch -> ours
    tt, ptt = fresh(torch.optim.Adam, foreach=False)
    _run(tt, ptt, 3, 0, gpu)
    b, pb = fresh(Adam)
    with torch.no_grad():
        for p, q in zip(pb, ptt):
            p.copy_(q)
    b.load_state_dict(_roundtrip(tt.state_dict()))
    ds = b._dev[gpu]
    for i, p in enumerate(pb):
        st = b.state[p]
        assert st["exp_avg"].data_ptr() == ds.m_views[i].data_ptr()
        assert st["exp_avg"].untyped_storage().data_ptr() == ds.exp_avg.untyped_storage().data_ptr()
        assert st["exp_avg_sq"].untyped_storage().data_ptr() == ds.exp_avg_sq.untyped_storage().data_ptr()
        assert st["step"].item() == 3.0
    _run(b, pb, 2, 3, gpu)
    _run(tt, ptt, 2, 3, gpu)
    for p, q in zip(pb, ptt):
        assert _rel_l2(p.detach(), q.detach()) <= 1e-6
        assert _rel_l2(b.state[p]["exp_avg"], tt.state[q]["exp_avg"]) <= 1e-6


class _Net(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.a = torch.nn.Linear(33, 5)          # 165 + 5: odd offsets into the flat buffer
        self.b = torch.nn.Linear(5, 3)
        self.c = torch.nn.Linear(3, 1000)
        self.d = torch.nn.Linear(1000, 7)


def _flat(gpu, seed=0):
    from sparse_rcnn_amd.dp import FlatParams
    from sparse_rcnn_amd.optim import FlatAdam
    torch.manual_seed(seed)
    fp = FlatParams(_Net().to(gpu), n_buckets=0)
    return fp, FlatAdam(fp, lr=1e-3, weight_decay=0.01)


def _flat_run(fp, adam, steps, gpu, drop=None):
    shapes = [p.shape for p in fp.params]
    for k in range(steps):
        fp.zero_grad()
        for i, (p, g) in enumerate(zip(fp.params, _grads(shapes, k, gpu, seed=11))):
            p.grad = None if (drop is not None and i == drop and k == steps - 1) else g
        fp.adam_step_single_rank(adam)
    torch.cuda.synchronize()


def test_flat_packed_and_fast_paths_are_bit_equal(gpu, monkeypatch):
    fa, aa = _flat(gpu)
    _flat_run(fa, aa, 3, gpu)
    assert not fa.flat_grad_valid                                        # the fast path ran
    monkeypatch.setenv("SCN_STEP_PACKED", "1")
    fb, ab = _flat(gpu)
    _flat_run(fb, ab, 3, gpu)
    assert fb.flat_grad_valid                                            # the packed path ran
    assert torch.equal(fa.flat, fb.flat)
    assert torch.equal(aa.exp_avg, ab.exp_avg) and torch.equal(aa.exp_avg_sq, ab.exp_avg_sq)
    assert (aa.steps == 3).all() and (ab.steps == 3).all()


def test_flat_paths_on_a_missing_gradient(gpu, monkeypatch):
    """Packed path: the parameter without a gradient counts as a zero gradient (its step advances, it keeps moving on its
    momentum); fast path: it is skipped (step and value stay), as torch.optim.Adam does."""
    drop = 2
    fa, aa = _flat(gpu)
    _flat_run(fa, aa, 2, gpu)
    before = fa.params[drop].detach().clone()
    fa.zero_grad()
    shapes = [p.shape for p in fa.params]
    for i, (p, g) in enumerate(zip(fa.params, _grads(shapes, 2, gpu, seed=11))):
        p.grad = None if i == drop else g
    fa.adam_step_single_rank(aa)
    torch.cuda.synchronize()
    assert aa.steps[drop] == 2 and (np.delete(aa.steps, drop) == 3).all()
    assert torch.equal(fa.params[drop].detach(), before)
    monkeypatch.setenv("SCN_STEP_PACKED", "1")
    fb, ab = _flat(gpu)
    _flat_run(fb, ab, 3, gpu, drop=drop)
    assert (ab.steps == 3).all()
    assert not torch.equal(fb.params[drop].detach(), before)
    # a step after the fast path skipped one parameter: the packed path runs one segment per run of equal step counts
    for i, (p, g) in enumerate(zip(fa.params, _grads(shapes, 3, gpu, seed=11))):
        p.grad = g
    fa.gather_grads()
    fa.adam_step(aa)
    torch.cuda.synchronize()
    assert aa.steps[drop] == 3 and (np.delete(aa.steps, drop) == 4).all()
    assert torch.isfinite(fa.flat).all()


@pytest.mark.parametrize("how", ["rank_weight", "total_weight"])
def test_flat_grad_scale_matches_torch_on_half_the_gradient(gpu, how):
    fp, adam = _flat(gpu)
    ref = [torch.nn.Parameter(p.detach().clone()) for p in fp.params]
    ta = torch.optim.Adam(ref, lr=1e-3, weight_decay=0.01, foreach=False)
    shapes = [p.shape for p in fp.params]
    for k in range(3):
        fp.zero_grad()
        grads = _grads(shapes, k, gpu, seed=13)
        for p, q, g in zip(fp.params, ref, grads):
            p.grad, q.grad = g, 0.5 * g
        if how == "rank_weight":
            fp.rank_weight = 0.5
            fp.adam_step_single_rank(adam)
        else:
            fp.all_reduce_mean(total_weight=2.0)
            assert fp.grad_scale == 0.5
            fp.adam_step(adam)
        ta.step()
        if k == 0:
            torch.cuda.synchronize()
            for p, q in zip(fp.params, ref):
                assert _ulps(p.detach(), q.detach()) <= 2
    torch.cuda.synchronize()
    for p, q in zip(fp.params, ref):
        assert _rel_l2(p.detach(), q.detach()) <= 1e-6


def _free():
    gc.collect()
    torch.cuda.empty_cache()


def test_cfg2_adam_replays_through_torch_and_is_deterministic(gpu, monkeypatch):
    """(lr 1e-5: the synthetic step feeds the SAME upstream gradient every step, a steady push -- at the reference's 4e-4 the
    features, and with them the squared gradients in exp_avg_sq, overflow within the 35 steps, for torch's Adam alike)"""
    from sparse_rcnn_amd.trainstep import SceneStep
    monkeypatch.setenv("SCN_STEP_PACKED", "1")
    lr = 1e-5

    def run(steps, collect):
        job = SceneStep("cfg2", gpu, prefetch=False, optimizer="adam", lr=lr)
        init = [p.detach().clone() for p in job.flat.params]
        grads = []
        for _ in range(steps):
            job.step()
            if collect:
                grads.append([g.clone() for g in job.flat.mean_grad_views()])
        torch.cuda.synchronize()
        return job, init, grads

    job, init, grads = run(3, True)
    assert "Adam" in job.describe() and "plain SGD" not in job.describe()
    ref = [torch.nn.Parameter(t.clone()) for t in init]
    ta = torch.optim.Adam(ref, lr=lr, foreach=False)
    for gs in grads:
        for q, g in zip(ref, gs):
            q.grad = g
        ta.step()
    for p, q in zip(job.flat.params, ref):
        assert _rel_l2(p.detach(), q.detach()) <= 1e-6
    first = job.flat.flat.clone()
    del job, grads
    _free()
    job2, _, _ = run(3, False)
    assert torch.equal(job2.flat.flat, first)
    for _ in range(32):
        job2.step()
    torch.cuda.synchronize()
    assert torch.isfinite(job2.flat.flat).all() and torch.isfinite(job2.adam.exp_avg_sq).all()
    assert torch.isfinite(job2.out.features).all()
    del job2
    _free()


def test_cfg2_bf16_adam_update_reaches_the_next_forward(gpu):
    from sparse_rcnn_amd.trainstep import SceneStep
    job = SceneStep("cfg2", gpu, dtype="bf16", prefetch=False, optimizer="adam")
    job.step()
    updated = job.flat.flat.clone()
    job.step()
    second = job.out.features.detach().clone()
    torch.cuda.synchronize()
    del job
    _free()
    fresh = SceneStep("cfg2", gpu, dtype="bf16", prefetch=False, optimizer="adam")
    assert not torch.equal(fresh.flat.flat, updated)                    # the update moved the parameters
    with torch.no_grad():
        fresh.flat.flat.copy_(updated)
    fresh.forward_backward(0)
    torch.cuda.synchronize()
    assert torch.equal(fresh.out.features.detach(), second)
    del fresh
    _free()


def test_cfg2_default_is_still_plain_sgd(gpu):
    from sparse_rcnn_amd.trainstep import SceneStep
    a = SceneStep("cfg2", gpu, prefetch=False)
    b = SceneStep("cfg2", gpu, prefetch=False, optimizer="sgd")
    assert a.adam is None and a.lr == b.lr == 1e-6
    a.step()
    b.step()
    torch.cuda.synchronize()
    assert a.describe() == b.describe() and "plain SGD" in a.describe()
    assert torch.equal(a.flat.flat, b.flat.flat)
    del a, b
    _free()
