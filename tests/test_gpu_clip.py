"""-m gpu: global-norm gradient clipping on the device -- the executor ops SCN_OP_GRAD_NORM and SCN_OP_GRAD_SCALE (csrc/scn_clip.hip)
as raw two-op plans on guarded buffers, optim.clip_grad_norm_ against torch's on the same tensors, FlatParams.clip_grad_norm on the
per-parameter and the packed path, SceneStep(max_grad_norm=) against a step whose gradients torch scaled, and two gloo ranks.

The reference of the raw ops is the float64 restatement in tests/clip_restate.py (pinned to torch on the CPU by
tests/test_clip_cpu.py).

The bound on total_norm, derived (not measured): the kernel squares every fp32 element in double -- exact, 48 significant bits --
and adds the squares in double, so S carries a relative error of at most n * 2^-53 (2^-33 for the largest n here, 2^20) whatever
the order; sqrt halves it and rounds once (2^-53); what remains is the double product with |gs| (one rounding, far below 2^-24)
and ONE rounding of the result to fp32, at most 2^-24 relative.  The restatement's own float64 error is of the size of the
kernel's double error.  NORM_REL = 2^-22 = 4 x 2^-24 holds all of it with a factor 4 of margin.  Everything else is compared
bit for bit: the coefficient against the fp32 expression on the record's own norm, every scaled element against one fp32 multiply.
"""
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))          # tests/clip_restate.py
import clip_restate as R                                                 # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NORM_REL = 2.0 ** -22
GUARD, SENT = 512, 0xA5
COUNTS = [1, 3, 4, 5, 255, 256, 257, 4095, 4096, 4097, 8192 + 3, (1 << 20) + 3]
TINY = dict(channels=(16, 32), target=500, grid=(32, 32, 16), prefetch=False)


class Buf:
    """`count` elements of `dtype` inside a sentinel-filled byte buffer; the data starts `off` elements past a 256-byte boundary."""

    def __init__(self, dev, dtype, count, off=0, fill=None):
        isz = torch.empty((), dtype=dtype).element_size()
        self.lo = GUARD + off * isz
        self.hi = self.lo + int(count) * isz
        self.raw = torch.full((self.hi + GUARD,), SENT, dtype=torch.uint8, device=dev)
        assert self.raw.data_ptr() % 256 == 0
        self.t = self.raw[self.lo:self.hi].view(dtype)
        if fill is not None:
            self.t.copy_(fill.reshape(-1))
        self.ptr = self.raw.data_ptr() + self.lo
        self.count = int(count)

    def intact(self):
        return bool((self.raw[:self.lo] == SENT).all()) and bool((self.raw[self.hi:] == SENT).all())


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _data(n, seed):
    return torch.randn(n, generator=torch.Generator().manual_seed(seed))


def _clip(dev, segs, max_norm, gs=1.0):
    """One clip_segments call over guarded segments with a guarded record and a guarded scratch of exactly the documented size.
    -> the record (numpy, 4 floats); asserts every guard."""
    from sparse_rcnn_amd import executor as EX
    counts = [s.count for s in segs]
    rec = Buf(dev, torch.float32, 4)
    scratch = Buf(dev, torch.uint8, EX.clip_scratch_bytes(counts))
    EX.clip_segments([s.ptr for s in segs], counts, max_norm, gs, rec.t, scratch.t)
    torch.cuda.synchronize()
    assert rec.intact() and scratch.intact() and all(s.intact() for s in segs)
    return rec.t.cpu().numpy()


def _check(dev, hosts, offs, gs=1.0):
    """Segments `hosts` (fp32 CPU tensors) at pointer offsets `offs`: a bound above the norm, then one below it, then the latter
    again.  -> the clipping run's record."""
    ref = [h.numpy() for h in hosts]
    want_total = R.total_norm(ref, gs)
    segs = [Buf(dev, torch.float32, h.numel(), off=o, fill=h) for h, o in zip(hosts, offs)]
    # a bound above the norm: the buffers come back bit-identical
    rec = _clip(dev, segs, 2.0 * want_total + 1.0, gs)
    print(f"[margin] n={[h.numel() for h in hosts][:4]} total_norm rel err {abs(float(rec[0]) - want_total) / want_total / NORM_REL:.3f} of the bound")
    assert abs(float(rec[0]) - want_total) <= NORM_REL * want_total
    assert rec[1] == np.float32(1.0) and rec[2] == 0.0 and rec[3] == 0.0
    for s, r in zip(segs, ref):
        assert np.array_equal(_bits(s.t.cpu().numpy()), _bits(r))
    # a bound below it
    bound = 0.37 * want_total
    rec = _clip(dev, segs, bound, gs)
    assert abs(float(rec[0]) - want_total) <= NORM_REL * want_total
    coef = rec[1]
    assert _bits(coef) == _bits(R.coef_f32(rec[0], bound)) and coef < 1.0 and rec[2] == 0.0
    for s, r in zip(segs, ref):
        assert np.array_equal(_bits(s.t.cpu().numpy()), _bits(R.scaled_f32(r, coef)))
    # again, from the same input: same bits
    segs2 = [Buf(dev, torch.float32, h.numel(), off=o, fill=h) for h, o in zip(hosts, offs)]
    rec2 = _clip(dev, segs2, bound, gs)
    assert np.array_equal(_bits(rec), _bits(rec2))
    for a, b in zip(segs, segs2):
        assert torch.equal(a.t.view(torch.int32), b.t.view(torch.int32))
    return rec


@pytest.mark.parametrize("off", [0, 1, 2, 3])
def test_single_segments_at_every_alignment(gpu, off):
    for i, n in enumerate(COUNTS):
        _check(gpu, [_data(n, 100 + i)], [off])


@pytest.mark.parametrize("table", ["three", "eighty_one", "zeros", "mixed"])
def test_segment_tables(gpu, table):
    if table == "three":
        counts, offs = [5, 4097, 300], [0, 0, 0]
    elif table == "eighty_one":                                  # crosses the 80-segment launch split
        counts, offs = [1 + (7 * i) % 23 + (4096 if i in (3, 80) else 0) for i in range(81)], [i % 4 for i in range(81)]
    elif table == "zeros":
        counts, offs = [0, 17, 0, 0, 4100, 0], [0, 1, 2, 3, 0, 1]
    else:
        counts, offs = [4096, 4095, 9000, 2, 1025], [3, 2, 1, 0, 1]
    _check(gpu, [_data(n, 200 + i) for i, n in enumerate(counts)], offs)


def test_an_empty_table_writes_a_zero_norm(gpu):
    rec = _clip(gpu, [Buf(gpu, torch.float32, 0), Buf(gpu, torch.float32, 0)], 2.0)
    assert rec.tolist() == [0.0, 1.0, 0.0, 0.0]


@pytest.mark.parametrize("bad", ["nan", "inf"])
def test_non_finite_gradients_set_the_flag(gpu, bad):
    h = _data(5000, 7)
    h[4321] = float(bad)
    s = Buf(gpu, torch.float32, h.numel(), off=1, fill=h)
    rec = _clip(gpu, [s], 1.0)
    assert rec[2] == 1.0 and rec[3] == 0.0
    got = s.t.cpu().numpy()
    if bad == "nan":                                              # torch.clamp leaves the NaN: every element becomes NaN
        assert np.isnan(rec[0]) and np.isnan(rec[1]) and np.isnan(got).all()
    else:                                                         # 1 / inf: the coefficient is 0
        assert np.isinf(rec[0]) and rec[1] == 0.0
        want = R.scaled_f32(h.numpy(), np.float32(0.0))
        assert np.isnan(got[4321]) and np.isnan(want[4321])
        keep = np.arange(h.numel()) != 4321
        assert np.array_equal(_bits(got[keep]), _bits(want[keep]))


def test_values_whose_fp32_squares_overflow(gpu):
    h = torch.full((4099,), 1e25)
    h[::3] = -1e25
    s = Buf(gpu, torch.float32, h.numel(), fill=h)
    rec = _clip(gpu, [s], 1.0)
    want = R.total_norm([h.numpy()])
    assert np.isfinite(rec[0]) and abs(float(rec[0]) - want) <= NORM_REL * want and rec[2] == 0.0
    assert _bits(rec[1]) == _bits(R.coef_f32(rec[0], 1.0))
    assert np.array_equal(_bits(s.t.cpu().numpy()), _bits(R.scaled_f32(h.numpy(), rec[1])))


def test_grad_scale_scales_the_norm_and_not_the_buffer(gpu):
    h = _data(10_001, 9)
    one = _check(gpu, [h], [0])
    quarter = _check(gpu, [h], [0], gs=0.25)                     # (inside: every element x coef only)
    assert abs(float(quarter[0]) - 0.25 * float(one[0])) <= 2 * NORM_REL * float(quarter[0])
    s = Buf(gpu, torch.float32, h.numel(), fill=h)
    rec = _clip(gpu, [s], 1e30, gs=-0.25)                        # the sign of the scale does not matter to a norm
    assert _bits(rec[0]) == _bits(_clip(gpu, [Buf(gpu, torch.float32, h.numel(), fill=h)], 1e30, gs=0.25)[0])
    assert np.array_equal(_bits(s.t.cpu().numpy()), _bits(h.numpy()))
    inf = _clip(gpu, [s], float("inf"))                           # +inf as the bound: measure only
    assert inf[1] == 1.0 and np.array_equal(_bits(s.t.cpu().numpy()), _bits(h.numpy()))


def test_bad_tables_are_refused_before_anything_runs(gpu):
    import ctypes as C
    from sparse_rcnn_amd import _lib as L, executor as EX
    lib = L.lib()
    s = Buf(gpu, torch.float32, 64, fill=_data(64, 1))
    rec, scratch = Buf(gpu, torch.float32, 4), Buf(gpu, torch.uint8, 256)

    def run(ptrs, counts, y=0, x1=0, rec_ptr=None):
        ops, levels, prefix = EX.clip_plan(counts, 1.0, 1.0)
        ops[0].y, ops[1].x1 = y, x1
        grads = (C.c_void_p * len(ptrs))(*ptrs)
        table = (C.c_void_p * 1)(rec.ptr if rec_ptr is None else rec_ptr)
        rc = lib.scn_exec_run(ops, 2, levels, 1, table, None, grads, scratch.ptr, 256, None, L.stream())
        return rc, lib.scn_last_error_string().decode()
    for ptrs, counts, kw, op in (([0], [8], {}, "SCN_OP_GRAD_NORM"),                      # NULL with a positive count
                                 ([s.ptr + 2], [8], {}, "SCN_OP_GRAD_NORM"),              # not 4-byte aligned
                                 ([s.ptr, s.ptr], [8, -3], {}, "SCN_OP_GRAD_NORM"),       # a negative count
                                 ([s.ptr], [8], dict(y=-1), "SCN_OP_GRAD_NORM")):
        rc, msg = run(ptrs, counts, **kw)
        assert rc == L.EINVAL and op in msg, (rc, msg)
    torch.cuda.synchronize()
    assert bool((rec.t.view(torch.uint8) == SENT).all())         # a refused norm op: nothing ran
    rc, msg = run([s.ptr], [8], x1=-1)                           # the scale op's record id (the norm op before it has run)
    assert rc == L.EINVAL and "SCN_OP_GRAD_SCALE" in msg, (rc, msg)
    torch.cuda.synchronize()
    assert s.intact() and rec.intact() and scratch.intact()
    assert np.array_equal(_bits(s.t.cpu().numpy()), _bits(_data(64, 1).numpy()))


# ---- optim.clip_grad_norm_ ----------------------------------------------------------------------------------------------------
def _params(dev, seed=3):
    g = torch.Generator().manual_seed(seed)
    shapes = [(3, 3, 3, 7, 16), (16,), (27, 16, 16), (1,), (16, 32), (5000,), (33, 3)] * 6          # 42 tensors
    ps = []
    for i, sh in enumerate(shapes[:40]):
        p = torch.nn.Parameter(torch.zeros(sh, device=dev))
        if i % 7 != 5:                                            # some parameters received no gradient
            p.grad = (torch.randn(sh, generator=g) * (1.0 + i % 3)).to(dev)
        ps.append(p)
    return ps


@pytest.mark.parametrize("clipped", [True, False])
def test_clip_grad_norm_is_torchs(gpu, clipped):
    from sparse_rcnn_amd.optim import clip_grad_norm_
    ours, theirs = _params(gpu), _params(gpu)
    before = [None if p.grad is None else p.grad.cpu().numpy().copy() for p in ours]
    have = [b for b in before if b is not None]
    assert len(have) < len(ours) == 40
    bound = R.total_norm(have) * (0.5 if clipped else 3.0)
    total = clip_grad_norm_(ours, bound, foreach=True)
    ref_total = torch.nn.utils.clip_grad_norm_(theirs, bound)
    assert total.dim() == 0 and total.is_cuda
    assert abs(float(total) - R.total_norm(have)) <= NORM_REL * R.total_norm(have)
    assert abs(float(total) - float(ref_total)) <= 1e-5 * float(ref_total)               # torch sums in fp32
    coef = R.coef_f32(np.float32(float(total)), bound)
    for p, q, b in zip(ours, theirs, before):
        if b is None:
            assert p.grad is None and q.grad is None
            continue
        got = p.grad.cpu().numpy()
        assert np.array_equal(_bits(got), _bits(R.scaled_f32(b, coef)))
        ref = q.grad.cpu().numpy()
        assert np.abs(got - ref).max() <= 1e-5 * np.abs(ref).max()
    # no allocation in steady state: the record and the scratch are the cached ones
    again = clip_grad_norm_(ours, bound)
    assert again.data_ptr() == total.data_ptr()
    with pytest.raises(RuntimeError, match="non-finite"):
        ours[0].grad[0, 0, 0, 0, 0] = float("nan")
        clip_grad_norm_(ours, bound, error_if_nonfinite=True)
    with pytest.raises(ValueError, match="contiguous fp32"):
        ours[4].grad = torch.zeros((32, 16), device=gpu).t()     # [16, 32], not contiguous
        clip_grad_norm_(ours, bound)


# ---- FlatParams: the per-parameter and the packed path ---------------------------------------------------------------------
def test_flat_params_packed_and_per_parameter_paths(gpu):
    from sparse_rcnn_amd.dp import FlatParams
    torch.manual_seed(0)
    net = torch.nn.Sequential(torch.nn.Linear(37, 129), torch.nn.Linear(129, 64), torch.nn.Linear(64, 3)).to(gpu)
    fp = FlatParams(net, n_buckets=2)
    g = torch.Generator().manual_seed(11)
    grads = [torch.randn(p.shape, generator=g).to(gpu) for p in fp.params]
    want = R.total_norm([x.cpu().numpy() for x in grads])
    bound = 0.25 * want

    def arm():
        for p, x in zip(fp.params, grads):
            p.grad = x.clone()
    arm()
    rec_pp = fp.clip_grad_norm(bound).cpu().numpy().copy()       # flat_grad_valid False: the gradients where they are
    assert abs(float(rec_pp[0]) - want) <= NORM_REL * want
    for p, x in zip(fp.params, grads):
        assert np.array_equal(_bits(p.grad.cpu().numpy()), _bits(R.scaled_f32(x.cpu().numpy(), rec_pp[1])))
    arm()
    fp.all_reduce_mean()                                         # one rank: packs flat_grad, grad_scale 1
    assert fp.flat_grad_valid and fp.grad_scale == 1.0
    flat0 = fp.flat_grad.cpu().numpy().copy()
    rec = fp.clip_grad_norm(bound).cpu().numpy().copy()
    assert abs(float(rec[0]) - float(rec_pp[0])) <= NORM_REL * float(rec[0])              # the two layouts chunk differently
    assert abs(float(rec[0]) - want) <= NORM_REL * want and _bits(rec[1]) == _bits(R.coef_f32(rec[0], bound))
    assert np.array_equal(_bits(fp.flat_grad.cpu().numpy()), _bits(R.scaled_f32(flat0, rec[1])))
    # the mean over 4 ranks' worth of weight: the norm is that of flat_grad x grad_scale, the buffer is scaled by the coefficient only
    arm()
    fp.all_reduce_mean(total_weight=4.0)
    rec4 = fp.clip_grad_norm(0.25 * bound).cpu().numpy().copy()
    assert abs(float(rec4[0]) - 0.25 * want) <= NORM_REL * 0.25 * want
    assert np.array_equal(_bits(fp.flat_grad.cpu().numpy()), _bits(R.scaled_f32(flat0, rec4[1])))


# ---- SceneStep(max_grad_norm=) -------------------------------------------------------------------------------------------------
def _step(gpu, **kw):
    from sparse_rcnn_amd.trainstep import SceneStep
    return SceneStep("cfg2", gpu, **{**TINY, **kw})


def _backward_only(st):
    """The micro-batches of SceneStep.step() without its update -> the gradients, where autograd left them."""
    n = st.batches_per_step
    for k in range(n - 1):
        with st.flat.accumulate():
            st.forward_backward(k, zero=(k == 0))
    st.forward_backward(n - 1, zero=(n == 1))
    assert all(p.grad is not None for p in st.flat.params)
    return [p.grad for p in st.flat.params]


def _update_only(st):
    """The update of SceneStep.step() on one rank."""
    if st.adam is not None:
        st.adam.lr = st.lr
        st.flat.adam_step_single_rank(st.adam)
    else:
        st.flat.step_single_rank(st.lr)


def _params_of(st):
    torch.cuda.synchronize()
    return st.flat.flat.cpu().numpy().copy()


def test_a_bound_never_reached_changes_nothing(gpu):
    plain, wide = _step(gpu, optimizer="adam"), _step(gpu, optimizer="adam", max_grad_norm=1e30)
    assert np.array_equal(_bits(_params_of(plain)), _bits(_params_of(wide)))
    plain.step(); plain.finish()
    wide.step(); wide.finish()
    assert np.array_equal(_bits(_params_of(plain)), _bits(_params_of(wide)))
    total, coef, bad = wide.grad_norm
    want = R.total_norm([p.grad.cpu().numpy() for p in wide.flat.params])
    assert coef == 1.0 and bad is False and abs(total - want) <= NORM_REL * want and plain.grad_norm is None


@pytest.mark.parametrize("kw", [dict(optimizer="adam"), dict(optimizer="adam", batches_per_step=2), dict(optimizer="sgd", lr=1e-3)],
                         ids=["adam", "adam-2-micro-batches", "sgd"])
def test_a_clipped_step_is_the_step_on_scaled_gradients(gpu, kw):
    manual = _step(gpu, **kw)
    grads = _backward_only(manual)                               # with batches_per_step=2: the accumulated gradient
    want = R.total_norm([g.cpu().numpy() for g in grads])
    clipped = _step(gpu, max_grad_norm=0.5 * want, **kw)
    assert np.array_equal(_bits(_params_of(manual)), _bits(_params_of(clipped)))
    calls = []
    inner = clipped.flat.clip_grad_norm
    clipped.flat.clip_grad_norm = lambda *a, **k: (calls.append(a), inner(*a, **k))[1]
    clipped.step(); clipped.finish()
    total, coef, bad = clipped.grad_norm
    assert len(calls) == 1                                       # once per optimizer step, after the last micro-batch
    assert abs(total - want) <= NORM_REL * want and bad is False
    assert _bits(np.float32(coef)) == _bits(R.coef_f32(np.float32(total), 0.5 * want)) and 0.49 < coef < 0.51
    torch._foreach_mul_(grads, coef)                             # torch scales the second step's gradients, then its plain update
    _update_only(manual)
    assert np.array_equal(_bits(_params_of(manual)), _bits(_params_of(clipped)))
    for a, b in zip(manual.flat.params, clipped.flat.params):
        assert torch.equal(a.grad.view(torch.int32), b.grad.view(torch.int32))


def test_two_clipping_steps_on_one_stream_keep_their_own_records(gpu):
    """Two step objects (staged training) and a caller's clip_grad_norm_ share the stream and the scratch, not the record:
    each `grad_norm` is that object's last clip, whatever ran after it."""
    from sparse_rcnn_amd.optim import clip_grad_norm_
    probe = _step(gpu, optimizer="adam")
    want = R.total_norm([g.cpu().numpy() for g in _backward_only(probe)])
    wide = _step(gpu, optimizer="adam", lr=0.0, max_grad_norm=1e30)
    tight = _step(gpu, optimizer="adam", lr=0.0, max_grad_norm=0.5 * want)
    for _ in range(2):                                           # alternately; lr 0: every step sees the same gradient
        wide.step(); wide.finish()
        tight.step(); tight.finish()
    other = _params(gpu)
    clip_grad_norm_(other, 1e-3)                                 # a third clip on the stream, with a coefficient of its own
    assert wide.flat.clip_record.data_ptr() != tight.flat.clip_record.data_ptr()
    w, t = wide.grad_norm, tight.grad_norm
    assert w[1] == 1.0 and abs(w[0] - want) <= NORM_REL * want and w[2] is False
    assert 0.49 < t[1] < 0.51 and abs(t[0] - want) <= NORM_REL * want and t[2] is False
    assert _bits(np.float32(t[1])) == _bits(R.coef_f32(np.float32(t[0]), 0.5 * want))


# ---- two ranks ----------------------------------------------------------------------------------------------------------------
def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def test_two_ranks_clip_the_mean_gradient_alike(gpu, tmp_path):
    """Two fresh gloo processes on cuda:0 (tests/clip_rank_worker.py), one scene each, one Adam step with a bound below the norm:
    both ranks write the same record bits and end with the same parameters, the norm is that of the mean gradient and the packed
    buffer is scaled by the one coefficient."""
    port = _free_port()
    procs, outs = [], []
    for r in range(2):
        out = str(tmp_path / f"rank{r}.npz")
        outs.append(out)
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE="2", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        procs.append(subprocess.Popen(["timeout", "-k", "10", "150", sys.executable, os.path.join(ROOT, "tests", "clip_rank_worker.py"),
                                       out, "0.5"], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT))
    logs = [p.communicate(timeout=200)[0].decode() for p in procs]
    assert all(p.returncode == 0 for p in procs), logs
    z = [np.load(o) for o in outs]
    assert np.array_equal(_bits(z[0]["record"]), _bits(z[1]["record"]))
    assert np.array_equal(_bits(z[0]["params"]), _bits(z[1]["params"]))
    assert not np.array_equal(_bits(z[0]["params"]), _bits(z[0]["params0"]))              # the update ran
    assert int(z[0]["clips"]) == int(z[1]["clips"]) == 1 and float(z[0]["grad_scale"]) == 0.5
    for r in range(2):
        total, coef = z[r]["record"][0], z[r]["record"][1]
        want = R.total_norm([z[r]["reduced"]], 0.5)               # the mean gradient: the summed buffer x grad_scale
        assert abs(float(total) - want) <= NORM_REL * want
        assert _bits(coef) == _bits(R.coef_f32(total, float(z[r]["bound"]))) and coef < 1.0
        assert np.array_equal(_bits(z[r]["scaled"]), _bits(R.scaled_f32(z[r]["reduced"], coef)))
    assert np.array_equal(_bits(z[0]["reduced"]), _bits(z[1]["reduced"]))
