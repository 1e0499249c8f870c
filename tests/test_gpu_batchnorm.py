"""-m gpu: BatchNorm(Leaky)ReLU -- the kernels of csrc/scn_elem.hip through the C ABI, and scn.BatchNormReLU /
scn.BatchNormLeakyReLU -- against float64 references, at the widths and row counts where k_bn_partial's thread map and
fixed grid change behaviour: widths that leave idle threads (48, 100, 112), exactly one row per thread (256), a second
256-column pass (257, 300, 512), row counts with empty blocks (< 256 rows over BN_BLOCKS = 256 blocks), at and just past
256-row boundaries, and the cfg2-bn sizes (32 .. 256 planes on 150 k rows).

Bounds are element-wise and derived from the kernels' arithmetic (u = 2^-24, the fp32 unit roundoff; rsqrtf is taken
within 2 ulp, 4u relative):
  statistics  float64 column sums over chains of at most L = ceil(n / 256) + 512 additions, then one rounding to fp32:
              |mean - m| <= ulp(m) + L 2^-53 mean|x|,  |var - v| <= ulp(v) + 4 (L + 1) 2^-53 mean(x^2)
  forward     y = ((x - m) * rsqrtf(v + eps)) * gamma + beta: the product term carries (x - m) u, (v + eps) u/2, rsqrtf 4u,
              two multiplies 2u -> 7.5u; the sum u |y|; the leak multiply u |out|, and the (leaky) ReLU is 1-Lipschitz:
              |out - ref| <= 10u |xhat gamma| + 3u |y|
  backward    xh = (x - m) * is is within 6.5u of xhat; A = sum g / n and B = sum g xh / n carry 2u mean|g| + u |A| and
              8u mean|g xhat| + u |B|; inner = g - A - xh B adds u (|g| + |A|), 8.5u |xhat B| and u |inner|; gamma * is and
              the last multiply 6.5u |inner|:
              |dX - ref| <= |gamma| is (8u |inner| + 4u (|g| + |A|) + 10u |xhat| (|B| + mean|g xhat|) + 2u mean|g|)
              evaluation mode (dX = gamma is g): 8u |gamma is g|
  dgamma      ulp(ref) + (8u + L 2^-53) sum|g xhat|;  dbeta  ulp(ref) + (u [leak not 0] + L 2^-53) sum|g|
Rows whose normalised pre-activation lies within 64u (|xhat gamma| + |beta|) of zero get dY = 0, so that a decision the
rounding may flip cannot move a gradient.  Every output buffer is followed by canary values that must survive, and every
entry point is called twice with bit-identical results.  The `wrong_reference` tests hand the same checks deliberately wrong
references and assert that each misses its bound by a wide margin."""
import numpy as np
import pytest
import torch

from oracle import scn_oracle as O

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
U64 = 2.0 ** -53
BN_BLOCKS = 256          # scn_elem.hip: the fixed grid of k_bn_partial
EPS = 1e-4
CANARY = 64
SENTINEL = -1234.5
TINY = 1e-37             # below it, fp32 results may be denormal or flushed


def _L():
    from sparse_rcnn_amd import _lib as L
    return L, L.lib()


def _chain(n):
    """Upper bound on the float64 additions behind one column sum: a thread's rows, its block's rows_par partials, the
    BN_BLOCKS block partials."""
    return -(-n // BN_BLOCKS) + 2 * 256


def _ulp(ref):
    return torch.from_numpy(np.spacing(np.abs(ref.numpy()).astype(np.float32)).astype(np.float64))


def _buf(numel, dtype, gpu):
    """(whole buffer, its first numel entries): the CANARY entries after them hold SENTINEL."""
    full = torch.full((numel + CANARY,), SENTINEL, dtype=dtype, device=gpu)
    return full, full[:numel]


def _untouched(full, numel, what):
    tail = full[numel:].cpu()
    assert bool((tail == SENTINEL).all()), f"{what}: the canary after the buffer was overwritten"


def _ratio(err, bound):
    """max over elements of |err| / bound (0 for no elements)."""
    return float((err.abs() / bound).max()) if err.numel() else 0.0


def _inputs(n, c, offset, seed):
    """[n, c] fp32, column std in [0.25, 2.25]; offset: column means of 1, 30 and 1000 std (signs alternating)."""
    g = torch.Generator().manual_seed(seed)
    std = torch.rand(c, generator=g, dtype=torch.float64) * 2 + 0.25
    ratio = torch.zeros(c, dtype=torch.float64)
    if offset:
        ratio = torch.tensor([1e3, -1.0, 30.0, -1e3, 0.0], dtype=torch.float64).repeat(c // 5 + 1)[:c]
    X = torch.randn(n, c, generator=g, dtype=torch.float64) * std + ratio * std
    return X.float()


def _affine(c, seed):
    g = torch.Generator().manual_seed(seed + 1000)
    gamma = (torch.rand(c, generator=g) * 1.5 + 0.25) * torch.where(torch.rand(c, generator=g) < 0.2, -1.0, 1.0)
    beta = torch.randn(c, generator=g) * 0.5
    return gamma.float(), beta.float()


# ------------------------------------------------------------------------------------------------ float64 references
def ref_stats(X):
    """(mean, biased variance) of the columns of X in float64, two passes; zero for no rows (what the kernel writes)."""
    Xd = X.double()
    if Xd.shape[0] == 0:
        return torch.zeros(Xd.shape[1], dtype=torch.float64), torch.zeros(Xd.shape[1], dtype=torch.float64)
    m = Xd.mean(0)
    return m, ((Xd - m) ** 2).mean(0)


def stats_ratio(X, mean, var, m_ref, v_ref):
    """Worst |kernel - reference| / bound over the mean and the variance."""
    Xd = X.double()
    n = X.shape[0]
    L = _chain(n)
    ax = Xd.abs().mean(0) if n else torch.zeros(X.shape[1], dtype=torch.float64)
    x2 = (Xd ** 2).mean(0) if n else torch.zeros(X.shape[1], dtype=torch.float64)
    bm = _ulp(m_ref) + L * U64 * ax + TINY
    bv = _ulp(v_ref) + 4 * (L + 1) * U64 * x2 + TINY
    return max(_ratio(mean.cpu().double() - m_ref, bm), _ratio(var.cpu().double() - v_ref, bv))


def _xhat(X, m, v, eps=EPS):
    """float64 x^ and 1/sqrt(v + eps) from the fp32 values the kernel was given."""
    is_ = 1.0 / torch.sqrt(v.double() + float(np.float32(eps)))
    return (X.double() - m.double()) * is_, is_


def ref_fwd(X, m, v, gamma, beta, leak):
    """-> (out, pre, bound) in float64."""
    xh, _ = _xhat(X, m, v)
    xg = xh * gamma.double()
    pre = xg + beta.double()
    lk = float(np.float32(leak))
    out = torch.where(pre > 0, pre, pre * lk)
    return out, pre, 10 * U * xg.abs() + 3 * U * pre.abs() + TINY


def safe_dy(X, m, v, gamma, beta, dY):
    """dY with zeros where the normalised pre-activation is within rounding of zero."""
    xh, _ = _xhat(X, m, v)
    xg = xh * gamma.double()
    pre = xg + beta.double()
    amb = pre.abs() <= 64 * U * (xg.abs() + beta.double().abs()) + 1e-30
    return torch.where(amb, torch.zeros_like(dY), dY)


def ref_bwd(X, dY, m, v, gamma, beta, leak, training, n_stat=None, rows=None, drop_mean_g=False):
    """-> (dX, dgamma, dbeta, bound dX, bound dgamma, bound dbeta) in float64.  The statistics terms A = sum g / n_stat,
    B = sum g x^ / n_stat are taken over all rows of X; dX, dgamma, dbeta over rows[0]:rows[1] (default: all) -- a rank's
    share in SyncBN.  drop_mean_g: leave out A (a deliberately wrong reference)."""
    xh, is_ = _xhat(X, m, v)
    ga = gamma.double()
    pre = xh * ga + beta.double()
    lk = float(np.float32(leak))
    g = dY.double() * torch.where(pre > 0, 1.0, lk)
    N = X.shape[0]
    n_stat = N if n_stat is None else n_stat
    r0, r1 = (0, N) if rows is None else rows
    inv = 1.0 / n_stat if n_stat else 0.0
    A = g.sum(0) * inv
    B = (g * xh).sum(0) * inv
    if drop_mean_g:
        A = torch.zeros_like(A)
    gl, xl = g[r0:r1], xh[r0:r1]
    if training:
        inner = gl - A - xl * B
        dX = ga * is_ * inner
        mg = g.abs().sum(0) * inv
        mgx = (g * xh).abs().sum(0) * inv
        bX = ga.abs() * is_ * (8 * U * inner.abs() + 4 * U * (gl.abs() + A.abs()) + 10 * U * xl.abs() * (B.abs() + mgx)
                               + 2 * U * mg) + TINY
    else:
        dX = ga * is_ * gl
        bX = 8 * U * dX.abs() + TINY
    L = _chain(r1 - r0)
    db = gl.sum(0)
    dg = (gl * xl).sum(0)
    bdb = _ulp(db) + ((U if leak else 0.0) + L * U64) * gl.abs().sum(0) + TINY
    bdg = _ulp(dg) + (8 * U + L * U64) * (gl * xl).abs().sum(0) + TINY
    return dX, dg, db, bX, bdg, bdb


# ------------------------------------------------------------------------------------------------ kernel calls
class _Kernels:
    def __init__(self, gpu, c):
        self.L, self.lib = _L()
        self.gpu, self.c = gpu, c
        self.scratch = torch.empty(self.lib.scn_bn_scratch_bytes(c), dtype=torch.uint8, device=gpu)

    def _go(self, rc):
        self.L.check(rc)

    def stats(self, Xg):
        n, c, P = Xg.shape[0], self.c, self.L.ptr
        mf, m = _buf(c, torch.float32, self.gpu)
        vf, v = _buf(c, torch.float32, self.gpu)
        self._go(self.lib.scn_bn_stats(P(Xg), n, c, P(m), P(v), P(self.scratch), self.L.stream()))
        torch.cuda.synchronize()
        _untouched(mf, c, "mean"), _untouched(vf, c, "var_biased")
        return m.clone(), v.clone()

    def sums(self, Xg):
        n, c, P = Xg.shape[0], self.c, self.L.ptr
        sf, s = _buf(2 * c, torch.float64, self.gpu)
        self._go(self.lib.scn_bn_sums(P(Xg), n, c, P(s), P(self.scratch), self.L.stream()))
        torch.cuda.synchronize()
        _untouched(sf, 2 * c, "sums")
        return s.clone()

    def fwd(self, Xg, m, v, ga, be, leak):
        n, c, P = Xg.shape[0], self.c, self.L.ptr
        yf, y = _buf(n * c, torch.float32, self.gpu)
        self._go(self.lib.scn_bn_fwd(P(Xg), n, c, P(m), P(v), EPS, P(ga), P(be), leak, P(y), self.L.stream()))
        torch.cuda.synchronize()
        _untouched(yf, n * c, "Y")
        return y.view(n, c).clone()

    def _grads(self):
        n, c = self.n, self.c
        xf, dx = _buf(n * c, torch.float32, self.gpu)
        gf, dg = _buf(c, torch.float32, self.gpu)
        bf, db = _buf(c, torch.float32, self.gpu)
        return (xf, dx), (gf, dg), (bf, db)

    def bwd(self, Xg, dYg, m, v, ga, be, leak, training):
        self.n = n = Xg.shape[0]
        c, P = self.c, self.L.ptr
        (xf, dx), (gf, dg), (bf, db) = self._grads()
        self._go(self.lib.scn_bn_bwd(P(Xg), P(dYg), n, c, P(m), P(v), EPS, P(ga), P(be), leak, int(training), P(dx),
                                     P(dg), P(db), P(self.scratch), self.L.stream()))
        torch.cuda.synchronize()
        _untouched(xf, n * c, "dX"), _untouched(gf, c, "dgamma"), _untouched(bf, c, "dbeta")
        return dx.view(n, c).clone(), dg.clone(), db.clone()

    def reduce(self, Xg, dYg, m, v, ga, be, leak):
        self.n = n = Xg.shape[0]
        c, P = self.c, self.L.ptr
        _, (gf, dg), (bf, db) = self._grads()
        sf, s = _buf(2 * c, torch.float64, self.gpu)
        self._go(self.lib.scn_bn_bwd_reduce(P(Xg), P(dYg), n, c, P(m), P(v), EPS, P(ga), P(be), leak, P(dg), P(db),
                                            P(s), P(self.scratch), self.L.stream()))
        torch.cuda.synchronize()
        _untouched(gf, c, "dgamma"), _untouched(bf, c, "dbeta"), _untouched(sf, 2 * c, "sums")
        return dg.clone(), db.clone(), s.clone()

    def apply(self, Xg, dYg, m, v, ga, be, leak, sums, n_stat):
        self.n = n = Xg.shape[0]
        c, P = self.c, self.L.ptr
        (xf, dx), _, _ = self._grads()
        self._go(self.lib.scn_bn_bwd_apply(P(Xg), P(dYg), n, c, P(m), P(v), EPS, P(ga), P(be), leak, P(sums), n_stat,
                                           P(dx), self.L.stream()))
        torch.cuda.synchronize()
        _untouched(xf, n * c, "dX")
        return dx.view(n, c).clone()


def _same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b)) if isinstance(a, tuple) else torch.equal(a, b)


def _case(gpu, n, c, offset, leak, seed):
    """Every entry point on one [n, c] input; -> the worst error / bound of each check (all must be <= 1)."""
    K = _Kernels(gpu, c)
    X = _inputs(n, c, offset, seed)
    Xg = X.to(gpu).contiguous()
    gamma, beta = _affine(c, seed)
    ga, be = gamma.to(gpu), beta.to(gpu)
    r = {}
    m, v = K.stats(Xg)
    assert _same((m, v), K.stats(Xg))
    m_ref, v_ref = ref_stats(X)
    r["stats"] = stats_ratio(X, m, v, m_ref, v_ref)
    s = K.sums(Xg)
    assert _same(s, K.sums(Xg))
    Xd = X.double()
    s_ref = torch.cat([Xd.sum(0), (Xd ** 2).sum(0)])
    Ls = _chain(n) + 64
    bs = torch.cat([Ls * U64 * Xd.abs().sum(0), (Ls + 1) * U64 * (Xd ** 2).sum(0)]) + 1e-300
    r["sums"] = _ratio(s.cpu() - s_ref, bs)
    # evaluation mode reads running statistics: near the batch's, not equal to them
    gr = torch.Generator().manual_seed(seed + 7)
    rm = (m_ref + 0.1 * torch.randn(c, generator=gr, dtype=torch.float64) * v_ref.sqrt()).float()
    rv = (v_ref * (0.5 + torch.rand(c, generator=gr, dtype=torch.float64)) + 0.01).float()
    dY = torch.randn(n, c, generator=gr)
    for training in (True, False):
        mm, vv = (m.cpu(), v.cpu()) if training else (rm, rv)
        mg, vg = mm.to(gpu), vv.to(gpu)
        y = K.fwd(Xg, mg, vg, ga, be, leak)
        assert _same(y, K.fwd(Xg, mg, vg, ga, be, leak))
        out, _, bY = ref_fwd(X, mm, vv, gamma, beta, leak)
        r[f"Y training={training}"] = _ratio(y.cpu().double() - out, bY)
        dYs = safe_dy(X, mm, vv, gamma, beta, dY)
        dYg = dYs.to(gpu)
        got = K.bwd(Xg, dYg, mg, vg, ga, be, leak, training)
        assert _same(got, K.bwd(Xg, dYg, mg, vg, ga, be, leak, training))
        dX, dg, db, bX, bdg, bdb = ref_bwd(X, dYs, mm, vv, gamma, beta, leak, training)
        r[f"dX training={training}"] = _ratio(got[0].cpu().double() - dX, bX)
        r[f"dgamma training={training}"] = _ratio(got[1].cpu().double() - dg, bdg)
        r[f"dbeta training={training}"] = _ratio(got[2].cpu().double() - db, bdb)
        if training:
            # the SyncBN halves with n_stat == n: bit for bit what the one-call backward computes
            dg2, db2, sums = K.reduce(Xg, dYg, mg, vg, ga, be, leak)
            assert _same((dg2, db2, sums), K.reduce(Xg, dYg, mg, vg, ga, be, leak))
            dx2 = K.apply(Xg, dYg, mg, vg, ga, be, leak, sums, n)
            assert _same(dx2, K.apply(Xg, dYg, mg, vg, ga, be, leak, sums, n))
            assert torch.equal(dx2, got[0]) and torch.equal(dg2, got[1]) and torch.equal(db2, got[2])
    return r


SMALL_C = (1, 3, 24, 48, 100, 112, 256, 257, 300, 512)
SMALL_N = (0, 1, 2, 255, 256, 257)
LEAKS = (0.0, 0.2, 0.333)
CASES = [(c, n, i % 2 == 1, LEAKS[i % 3]) for i, (c, n) in enumerate((c, n) for c in SMALL_C for n in SMALL_N)]
# large n: 65 537 rows (257 rows per block, the last block short) at widths with idle threads / a second column pass, and
# the cfg2-bn widths on 150 k rows (586 rows per block, 570 in the last)
CASES += [(3, 65_537, True, 0.2), (100, 65_537, False, 0.333), (257, 65_537, True, 0.0), (300, 65_537, False, 0.2),
          (32, 150_000, False, 0.0), (64, 150_000, True, 0.333), (128, 150_000, True, 0.0), (256, 150_000, False, 0.2),
          (256, 150_000, True, 0.0)]


@pytest.mark.parametrize("c,n,offset,leak", CASES)
def test_bn_kernels_vs_float64(gpu, c, n, offset, leak):
    r = _case(gpu, n, c, offset, leak, seed=c * 7 + n)
    bad = {k: x for k, x in r.items() if not x <= 1.0}
    assert not bad, (bad, r)


@pytest.mark.parametrize("c,n0,n1,leak", [(24, 100, 157, 0.2), (48, 255, 1, 0.0), (300, 257, 256, 0.333),
                                          (256, 75_000, 75_000, 0.0)])
def test_bn_bwd_apply_with_statistics_over_more_rows(gpu, c, n0, n1, leak):
    """SyncBN on one process: the statistics and (sum g, sum g x^) are over the rows of two 'ranks', rank 0 applies them to
    its own n0 rows (scn_bn_bwd_apply with n_stat = n0 + n1 > n); dgamma / dbeta of scn_bn_bwd_reduce are rank 0's share."""
    K = _Kernels(gpu, c)
    N = n0 + n1
    X = _inputs(N, c, True, seed=c + N)
    gamma, beta = _affine(c, c)
    ga, be = gamma.to(gpu), beta.to(gpu)
    m_ref, v_ref = ref_stats(X)
    m, v = m_ref.float(), v_ref.float()
    mg, vg = m.to(gpu), v.to(gpu)
    dY = safe_dy(X, m, v, gamma, beta, torch.randn(N, c, generator=torch.Generator().manual_seed(3)))
    X0, X1 = X[:n0].to(gpu).contiguous(), X[n0:].to(gpu).contiguous()
    d0, d1 = dY[:n0].to(gpu).contiguous(), dY[n0:].to(gpu).contiguous()
    dg0, db0, s0 = K.reduce(X0, d0, mg, vg, ga, be, leak)
    _, _, s1 = K.reduce(X1, d1, mg, vg, ga, be, leak)
    sums = s0 + s1                                     # the all-reduce
    dx = K.apply(X0, d0, mg, vg, ga, be, leak, sums, N)
    assert _same(dx, K.apply(X0, d0, mg, vg, ga, be, leak, sums, N))
    dX, dg, db, bX, bdg, bdb = ref_bwd(X, dY, m, v, gamma, beta, leak, True, rows=(0, n0))
    r = dict(dX=_ratio(dx.cpu().double() - dX, bX), dgamma=_ratio(dg0.cpu().double() - dg, bdg),
             dbeta=_ratio(db0.cpu().double() - db, bdb))
    assert all(x <= 1.0 for x in r.values()), r
    # n_stat must not be smaller than n
    L, lib = _L()
    rc = lib.scn_bn_bwd_apply(L.ptr(X0), L.ptr(d0), n0, c, L.ptr(mg), L.ptr(vg), EPS, L.ptr(ga), L.ptr(be), leak,
                              L.ptr(sums), n0 - 1, L.ptr(dx), L.stream())
    assert rc != 0


# ------------------------------------------------------------------------------------------------ modules
def _module(planes, leak, gpu, seed):
    import sparse_rcnn_amd as scn
    bn = (scn.BatchNormLeakyReLU(planes, EPS, 0.9, leak) if leak else scn.BatchNormReLU(planes, EPS, 0.9)).to(gpu)
    gamma, beta = _affine(planes, seed)
    with torch.no_grad():
        bn.weight.copy_(gamma), bn.bias.copy_(beta)
    return bn


def _module_step(bn, X, gpu, dY_seed):
    """Forward + backward of the module on X; against O.batchnorm_relu_fwd in float64 with autograd (running statistics
    cloned before).  -> dict of worst error / bound, the reference's running statistics after the step."""
    import sparse_rcnn_amd as scn
    training = bn.training
    n, c = X.shape
    rm0 = bn.running_mean.detach().cpu().double().clone()
    rv0 = bn.running_var.detach().cpu().double().clone()
    xg = X.to(gpu).requires_grad_()
    y = bn(scn.SparseConvNetTensor(xg)).features
    Xo = X.double().requires_grad_()
    ga = bn.weight.detach().cpu().double().requires_grad_()
    be = bn.bias.detach().cpu().double().requires_grad_()
    rm, rv = rm0.clone(), rv0.clone()
    yo = O.batchnorm_relu_fwd(Xo, ga, be, rm, rv, EPS, 0.9, bn.leakiness, training)
    m_ref, v_ref = ref_stats(X) if training else (rm0, rv0)
    # the module normalises with fp32 statistics: |dm| <= ulp(m) + L 2^-53 mean|x|, |dv| the same with 4 mean(x^2); they move
    # the pre-activation by |dm| is |gamma| + |xhat gamma| |dv| / (2 (v + eps)) on top of the kernel's own bound
    L = _chain(n)
    xh, is_ = _xhat(X, m_ref, v_ref)
    gd = ga.detach()
    dm = (_ulp(m_ref) + L * U64 * X.double().abs().mean(0)) if training else torch.zeros(c, dtype=torch.float64)
    dv = (_ulp(v_ref) + 4 * (L + 1) * U64 * (X.double() ** 2).mean(0)) if training else torch.zeros(c, dtype=torch.float64)
    srel = dm * is_ + xh.abs() * dv * is_ ** 2 / 2          # relative to |gamma|: the statistics' share of |pre - ref|
    xg_ = (xh * gd).abs()
    bY = 10 * U * xg_ + 3 * U * (xh * gd + be.detach()).abs() + gd.abs() * srel + TINY
    r = {"Y": _ratio(y.detach().cpu().double() - yo.detach(), bY)}
    dY = torch.randn(n, c, generator=torch.Generator().manual_seed(dY_seed), dtype=torch.float64)
    pre = xh * gd + be.detach()
    dY = torch.where(pre.abs() <= 64 * U * (xg_ + be.detach().abs()) + gd.abs() * 4 * srel + 1e-30, 0.0, dY).float()
    gx, gg, gb = torch.autograd.grad(y, (xg, bn.weight, bn.bias), dY.to(gpu))
    ox, og, ob = torch.autograd.grad(yo, (Xo, ga, be), dY.double())
    # the kernel's element bounds, widened by the statistics' relative error (srel) on every term
    dXr, dgr, dbr, bX, bdg, bdb = ref_bwd(X, dY, m_ref.float(), v_ref.float(), gd.float(), be.detach().float(),
                                          bn.leakiness, training)
    wid = 1 + srel.max() / (8 * U)
    r["dX"] = _ratio(gx.cpu().double() - ox, bX * wid + (ox - dXr).abs())
    r["dgamma"] = _ratio(gg.cpu().double() - og, bdg * wid + (og - dgr).abs())
    r["dbeta"] = _ratio(gb.cpu().double() - ob, bdb * wid + (ob - dbr).abs())
    return r, rm, rv


@pytest.mark.parametrize("planes", [32, 64, 128, 256])
@pytest.mark.parametrize("leak", [0.0, 0.333], ids=["BatchNormReLU", "BatchNormLeakyReLU"])
def test_bn_module_vs_float64_autograd_at_150k(gpu, planes, leak):
    """Three training steps (150 000 rows, one row, 257 rows with a mean offset), the running statistics after each, then an
    evaluation-mode forward and backward with them."""
    bn = _module(planes, leak, gpu, seed=planes)
    bn.train()
    for step, (n, offset) in enumerate([(150_000, False), (1, False), (257, True)]):
        X = _inputs(n, planes, offset, seed=planes + step)
        rm0, rv0 = bn.running_mean.cpu().double(), bn.running_var.cpu().double()
        r, rm, rv = _module_step(bn, X, gpu, dY_seed=step)
        assert all(x <= 1.0 for x in r.values()), (step, r)
        r = running_stats_ratio(bn, X, rm0, rv0, rm, rv)
        assert r <= 1.0, (step, r)
    bn.eval()
    rm0, rv0 = bn.running_mean.clone(), bn.running_var.clone()
    X = _inputs(20_000, planes, False, seed=planes + 9)
    r, _, _ = _module_step(bn, X, gpu, dY_seed=9)
    assert all(x <= 1.0 for x in r.values()), ("eval", r)
    assert torch.equal(bn.running_mean, rm0) and torch.equal(bn.running_var, rv0)   # evaluation leaves them alone


def running_stats_ratio(bn, X, rm0, rv0, rm, rv):
    """Worst error / bound of the module's running statistics after one training step that started from (rm0, rv0), against
    the reference's (rm, rv).  The update 0.9 r0 + 0.1 f s (f = n / (n - 1) for the variance, 1 for n = 1) rounds three times
    in fp32 (4u on each term and the result); s itself is the kernel's statistic (its bound above)."""
    n = X.shape[0]
    m_ref, v_ref = ref_stats(X)
    f = n / (n - 1) if n > 1 else 1.0
    L = _chain(n)
    em = _ulp(m_ref) + L * U64 * X.double().abs().mean(0)
    ev = _ulp(v_ref) + 4 * (L + 1) * U64 * (X.double() ** 2).mean(0)
    bm = 0.1 * em + 4 * U * (0.9 * rm0.abs() + 0.1 * m_ref.abs() + rm.abs()) + TINY
    bv = 0.1 * f * ev + 4 * U * (0.9 * rv0.abs() + 0.1 * f * v_ref + rv.abs()) + TINY
    return max(_ratio(bn.running_mean.cpu().double() - rm, bm), _ratio(bn.running_var.cpu().double() - rv, bv))


# ------------------------------------------------------------------------------------------------ the checks can fail
def test_bn_checks_reject_wrong_references(gpu):
    """Each check above, handed a deliberately wrong reference, misses its bound by far (the factors are printed):
    a running variance without the n / (n - 1) factor, a training dX without the mean-of-g term, and statistics that leave
    out the last of the BN_BLOCKS row blocks (the kernel's own partition, 586 rows per block at 150 k rows)."""
    found = {}
    # running variance without n / (n - 1), after a 257-row step
    bn = _module(64, 0.0, gpu, seed=3)
    bn.train()
    X = _inputs(257, 64, False, seed=4)
    rm0, rv0 = bn.running_mean.cpu().double(), bn.running_var.cpu().double()
    _, rm, rv = _module_step(bn, X, gpu, dY_seed=1)
    assert running_stats_ratio(bn, X, rm0, rv0, rm, rv) <= 1.0
    v_ref = ref_stats(X)[1]
    rv_wrong = 0.9 * rv0 + 0.1 * v_ref                          # the biased batch variance
    found["running_var without n/(n-1)"] = running_stats_ratio(bn, X, rm0, rv0, rm, rv_wrong)
    # dX without the mean-of-g term, and statistics without the last row block, on a cfg2-bn slab
    n, c = 150_000, 32
    K = _Kernels(gpu, c)
    X = _inputs(n, c, False, seed=5)
    Xg = X.to(gpu)
    m, v = K.stats(Xg)
    m_ref, v_ref = ref_stats(X)
    assert stats_ratio(X, m, v, m_ref, v_ref) <= 1.0
    rows_per_block = -(-n // BN_BLOCKS)
    mw, vw = ref_stats(X[:(BN_BLOCKS - 1) * rows_per_block])
    found["statistics without the last row block"] = stats_ratio(X, m, v, mw, vw)
    gamma, beta = _affine(c, 5)
    mc, vc = m.cpu(), v.cpu()
    dY = safe_dy(X, mc, vc, gamma, beta, torch.randn(n, c, generator=torch.Generator().manual_seed(6)))
    dx, _, _ = K.bwd(Xg, dY.to(gpu), m, v, gamma.to(gpu), beta.to(gpu), 0.0, True)
    dX, _, _, bX, _, _ = ref_bwd(X, dY, mc, vc, gamma, beta, 0.0, True)
    assert _ratio(dx.cpu().double() - dX, bX) <= 1.0
    dXw = ref_bwd(X, dY, mc, vc, gamma, beta, 0.0, True, drop_mean_g=True)[0]
    found["dX without the mean of g"] = _ratio(dx.cpu().double() - dXw, bX)
    print("[bn wrong references] worst error / bound: " + ", ".join(f"{k} {x:.3g}" for k, x in found.items()))
    assert all(x > 10.0 for x in found.values()), found


# ------------------------------------------------------------------------------------------------ slab width != nPlanes
@pytest.mark.parametrize("training", [True, False])
def test_bn_refuses_a_slab_wider_than_its_planes(gpu, training):
    """A channel-padded slab (24 columns: the mask head's 23-channel level padded to 16-byte rows) handed to
    BatchNormReLU(23) is refused before any kernel runs: normalising 24 columns with 23 statistics would read past
    mean / var / gamma / beta and make the zero pad column non-zero."""
    import sparse_rcnn_amd as scn
    bn = scn.BatchNormReLU(23).to(gpu)
    bn.train(training)
    X = torch.nn.functional.pad(torch.randn(300, 23, generator=torch.Generator().manual_seed(0)), (0, 1)).to(gpu)
    rm, rv = bn.running_mean.clone(), bn.running_var.clone()
    with pytest.raises(ValueError, match="23"):
        bn(scn.SparseConvNetTensor(X))
    assert torch.equal(bn.running_mean, rm) and torch.equal(bn.running_var, rv)
