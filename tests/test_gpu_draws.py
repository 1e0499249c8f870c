"""The sample conversion's device-side draws on the MI355X: scn_philox_fill's words bit-equal to the independent restatement
(tests/philox_restate.py) and its normals within 16 ulp of the float64 evaluation of the same words; the fused pack kernel
(scn_sample_pack_drawn) bit-equal to scn_sample_pack fed the materialised noise; scn_sample_cut_start equal to the restated
random cut-out in all eight outputs; convert_sample with PhiloxDraws bit-equal to convert_sample given the same values as a plain
Draws -- the path the reference's fixtures pin; one SceneStep step on a batch converted that way."""
import math
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import philox_restate as P                                     # noqa: E402
import sample_restate as R                                     # noqa: E402

pytestmark = pytest.mark.gpu

SEEDS = [(2 ** 63 + 5, 2 ** 40 + 1), (0xFFFFFFFF00000001, 0x8000000080000000)]
GUARD = 64


def _fill(gpu, seed, counter, stream, first, n, mode, sigma=1.0):
    """scn_philox_fill into a buffer prefilled with a pattern that is a NaN as fp32, with guards on both sides.
    -> (the written part as int32 [n][4 or 3], the whole buffer)."""
    from sparse_rcnn_amd import _lib as L
    width = 4 if mode == 0 else 3
    whole = torch.full((GUARD + n * width + GUARD,), 0x7FC12345, dtype=torch.int32, device=gpu)
    body = whole[GUARD:GUARD + n * width]
    L.check(L.lib().scn_philox_fill(seed, counter, stream, first, n, mode, sigma, L.ptr(body), L.stream()))
    torch.cuda.synchronize()
    return body.view(n, width), whole


def _guards_intact(whole):
    return bool((whole[:GUARD] == 0x7FC12345).all()) and bool((whole[-GUARD:] == 0x7FC12345).all())


@pytest.mark.parametrize("seed,counter", SEEDS)
@pytest.mark.parametrize("first", [0, 5])
def test_fill_words_equal_the_restatement(gpu, seed, counter, first):
    fills = {}
    for n in (1, 3, 64, 1000, 4099):
        body, whole = _fill(gpu, seed, counter, 2, first, n, 0)
        got = body.cpu().numpy().view(np.uint32)
        want = P.words_array(seed, counter, 2, first, n)
        assert np.array_equal(got, want), n                     # every element written (none is the prefill), bit-equal
        assert tuple(int(v) for v in got[n - 1]) == P.words(seed, counter, 2, first + n - 1)
        assert _guards_intact(whole), n
        fills[n] = got
    assert np.array_equal(fills[4099][:1000], fills[1000])       # a value does not depend on the launch shape
    other, _ = _fill(gpu, seed, counter, 3, first, 64, 0)
    assert not np.array_equal(other.cpu().numpy().view(np.uint32), fills[64])       # another stream, other words


@pytest.mark.parametrize("seed,counter", SEEDS)
def test_fill_normals_within_16_ulp_of_float64(gpu, seed, counter):
    """|sigma z - float64| <= 16 * 2^-21: 16 ulp at the largest possible |z| = sqrt(48 ln 2) = 5.77 (logf, sqrtf, sincospif are
    documented at 1-2 ulp each, two multiplies follow).  Measured on the MI355X: see DESIGN 4.12."""
    bound = 16 * 2.0 ** -21
    worst = 0.0
    for stream, first, n, sigma in ((2, 0, 4099, 1.0), (3, 5, 1000, 1.0), (4, 0, 1, 1.0), (2, 0, 1 << 16, 1.0)):
        body, whole = _fill(gpu, seed, counter, stream, first, n, 1, sigma)
        got = body.view(torch.float32).cpu().numpy().astype(np.float64)
        assert _guards_intact(whole) and np.isfinite(got).all()  # every element written: the prefill is a NaN
        want = P.normals_array(P.words_array(seed, counter, stream, first, n))
        worst = max(worst, float(np.abs(got - want).max()))
    print(f"[fill] worst |fp32 - float64| of a normal: {worst:.3e} (bound {bound:.3e})")
    assert worst <= bound
    # sigma scales with one rounding: sigma * z of the sigma = 1 fill
    one, _ = _fill(gpu, seed, counter, 2, 0, 1000, 1, 1.0)
    tenth, _ = _fill(gpu, seed, counter, 2, 0, 1000, 1, 0.1)
    assert torch.equal(tenth.view(torch.float32), one.view(torch.float32) * torch.tensor(0.1, device=gpu))
    a, _ = _fill(gpu, seed, counter, 2, 0, 4099, 1, 0.1)
    assert torch.equal(a[:1000], tenth)


VARIANTS = [                                                    # (name, colour sigma, common, normal sigma, common, use_color, use_normal)
    ("per-point both", 0.1, 0, 0.05, 0, 1, 1),
    ("common both", 0.1, 1, 0.05, 1, 1, 1),
    ("colour only", 0.1, 0, 0.0, 0, 1, 1),
    ("normals only, rotated", 0.0, 0, 0.05, 0, 1, 1),
    ("colour common, normals per point", 0.2, 1, 0.3, 0, 1, 1),
    ("sigma 0", 0.0, 0, 0.0, 0, 1, 1),
    ("no colour channel", 0.1, 0, 0.05, 1, 0, 1),
    ("no normal channel", 0.1, 1, 0.05, 0, 1, 0),
]


@pytest.mark.parametrize("m", [0, 1, 63, 64, 65, 1000])
def test_fused_pack_equals_pack_fed_the_materialised_noise(gpu, m):
    from sparse_rcnn_amd import _lib as L
    from sparse_rcnn_amd.sample import PhiloxDraws
    from sparse_rcnn_amd.voxelize import _f32xn
    lib = L.lib()
    gen = torch.Generator().manual_seed(100 + m)
    n, n_inst = 1500, 5
    rows = torch.sort(torch.randperm(n, generator=gen)[:m]).values.to(torch.int32).to(gpu)
    colors = (torch.rand((n, 3), generator=gen) * 2 - 1).to(gpu)
    normals = torch.nn.functional.normalize(torch.randn((n, 3), generator=gen), dim=1).to(gpu)
    ids = torch.randint(0, n_inst + 1, (n,), generator=gen).to(gpu)
    angle = 0.7
    rot = (torch.eye(3) + 0.1 * torch.randn((3, 3), generator=gen)) @ torch.tensor(
        [[math.cos(angle), math.sin(angle), 0.], [-math.sin(angle), math.cos(angle), 0.], [0., 0., 1.]])
    slot = torch.tensor([0, -1, 1, -1, 2, -1], dtype=torch.int32).to(gpu)
    g, w = 3, (m + 31) // 32
    seg_table = torch.tensor([3, 1, 4, 1, 5, -100]).to(gpu)
    seed, counter = SEEDS[0]
    draws = PhiloxDraws(seed, counter)
    for name, cs, cc, ns, nc, use_c, use_n in VARIANTS:
        c = 3 * use_c + 1 + 3 * use_n
        outs = []
        for fused in (True, False):
            feats = torch.full((max(m, 1), c), float("nan"), device=gpu)
            seg = torch.full((max(m, 1),), -7, dtype=torch.int64, device=gpu)
            words = torch.full((max(g * w, 1),), 0x55555555, dtype=torch.int32, device=gpu)
            head = (L.ptr(rows), m, L.ptr(colors), L.ptr(normals), L.ptr(ids), n_inst, _f32xn(rot, 9))
            tail = (use_c, 1, use_n, L.ptr(feats), L.ptr(seg_table), L.ptr(seg), L.ptr(slot), g, L.ptr(words), L.stream())
            if fused:
                L.check(lib.scn_sample_pack_drawn(*head, seed, counter, cs, cc, ns, nc, *tail))
            else:
                cn = draws.noise_tensor("color", m, cs, cc, device=gpu) if (cs and use_c and m) else None
                nn_ = draws.noise_tensor("normal", m, ns, nc, device=gpu) if (ns and use_n and m) else None
                assert cn is None or tuple(cn.shape) == ((3,) if cc else (m, 3))
                L.check(lib.scn_sample_pack(*head, L.ptr(cn), int(not cc), L.ptr(nn_), int(not nc), *tail))
            torch.cuda.synchronize()
            outs.append((feats.view(torch.int32), seg, words))
        for what, a, b in zip(("features", "labels", "mask words"), *outs):
            assert torch.equal(a, b), (name, what)
        feats = outs[0][0].view(torch.float32)
        if m:
            assert bool(torch.isfinite(feats).all()), name       # every feature written
            plain = colors[rows.long()]
            if use_c:
                assert torch.equal(feats[:, :3], plain) == (cs == 0.0), name    # noise where asked for, none at sigma 0
        else:
            assert bool(torch.isnan(feats).all()) and int(outs[0][2][0]) == 0x55555555      # M = 0: nothing is touched


def _cut(gpu, pts, size, border, seed, counter):
    from sparse_rcnn_amd import _lib as L
    from sparse_rcnn_amd.voxelize import _i32x3
    whole = torch.full((GUARD + 8 + GUARD,), 0x7FC12345, dtype=torch.int32, device=gpu)
    d = torch.as_tensor(pts, dtype=torch.int32).to(gpu).contiguous()
    L.check(L.lib().scn_sample_cut_start(L.ptr(d), d.shape[0], _i32x3(size), _i32x3(border), seed, counter,
                                         L.ptr(whole[GUARD:GUARD + 8]), L.stream()))
    torch.cuda.synchronize()
    assert _guards_intact(whole)
    return whole[GUARD:GUARD + 8].cpu().tolist()


def _cut_want(pts, size, border, seed, counter):
    start, order, alive, dims, _ = P.random_cut_out(pts, size, border, seed, counter)
    return start + order + [alive, dims]


@pytest.mark.parametrize("n", [1, 63, 1025, 5000])
@pytest.mark.parametrize("border", [(0, 0, 0), (8, 8, 4)])
def test_cut_start_equals_the_restatement(gpu, n, border):
    rng = np.random.default_rng(n)
    pts = rng.integers(0, 100, size=(n, 3))
    size = (32, 32, 16)
    orders = set()
    for seed, counter in SEEDS + [(1234, k) for k in range(6)]:
        want = _cut_want(pts, list(size), list(border), seed, counter)
        got = _cut(gpu, pts, size, border, seed, counter)
        assert got == want, (seed, counter)
        assert _cut(gpu, pts, size, border, seed, counter) == got           # a rerun gives the same eight values
        orders.add(tuple(got[3:6]))
    assert len(orders) >= 3                                      # the dimension order does vary with the counter


def test_cut_start_axis_shorter_than_the_size_and_window_in_a_gap(gpu):
    rng = np.random.default_rng(7)
    # z spans 6 voxels, the size is 16 and the border at most 4: max_start = hi + 1 - 16 + border <= lo - border whatever
    # subset is alive, so no draw is made on z, its start is (lowest alive z) - border and nothing is cut along z
    pts = np.concatenate([rng.integers(0, 100, size=(2000, 2)), rng.integers(20, 26, size=(2000, 1))], 1)
    for border in ((0, 0, 0), (8, 8, 4)):
        for counter in range(4):
            start, order, alive, dims, inside = P.random_cut_out(pts, [32, 32, 16], list(border), 99, counter)
            moved = pts[:, :2] - np.array(start[:2])
            in_xy = ((moved >= 0) & (moved < 32)).all(1)
            assert np.array_equal(inside, in_xy) and alive == int(in_xy.sum())
            if alive:
                assert dims == 3 and 20 - border[2] <= start[2] <= 25 - border[2]
            assert _cut(gpu, pts, (32, 32, 16), border, 99, counter) == start + order + [alive, dims]
    # two clusters 80 voxels apart in x, y and z 8 wide from 3: a window in the gap leaves nothing alive and ends the loop
    one = np.concatenate([rng.integers(0, 8, size=(300, 1)), rng.integers(3, 11, size=(300, 2))], 1)
    pts = np.concatenate([one, one + np.array([88, 0, 0])])
    size, border = [16, 16, 16], [0, 0, 0]
    stopped = [k for k in range(200) if _cut_want(pts, size, border, 5, k)[6] == 0 and _cut_want(pts, size, border, 5, k)[7] < 3]
    filled = [k for k in range(200) if _cut_want(pts, size, border, 5, k)[6] > 0]
    assert stopped and filled
    for counter in stopped[:3] + filled[:2]:
        want = _cut_want(pts, size, border, 5, counter)
        got = _cut(gpu, pts, size, border, 5, counter)
        assert got == want, counter
        if counter in stopped:                                   # the dimensions after x were not processed: their starts stay 0
            later = want[3:6][want[7]:]
            assert later and all(want[d] == 0 for d in later) and 8 <= want[0] <= 72


def _crop_kw():
    from test_gpu_sample import _training_mappers
    inst, seg = _training_mappers()
    return dict(spatial_size=(64, 64, 32), instance_cutoff_threshold=0.5, color_noise_sigma=0.1, common_color_noise=False,
                normal_noise_sigma=0.05, common_normal_noise=True, use_color=True, use_ones=True, use_normal=True,
                additional_bbox_pixel=0, background_label=-100, scale=1 / 0.02, instance_label_mapper=inst,
                segmentation_label_mapper=seg, shift=None)


def _same(a, b):
    """Two convert_sample 9-tuples (the noise entries of the augmentation dict apart): every output, bits and dtypes."""
    assert a[0] == b[0]
    for k in (1, 2, 3, 5, 6, 8):
        assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape, k
        x, y = a[k].contiguous(), b[k].contiguous()
        if x.dtype == torch.float32:
            x, y = x.view(torch.int32), y.view(torch.int32)
        assert torch.equal(x, y), k
    assert a[4].n_gt == b[4].n_gt and a[4].n_points == b[4].n_points and torch.equal(a[4].words, b[4].words)
    for k in ("coords_projection", "coords_shift", "remaining_points"):
        assert torch.equal(a[7][k], b[7][k]), k


def test_convert_sample_with_philox_draws_equals_the_given_draws_path(gpu, monkeypatch):
    from sparse_rcnn_amd import sample as S
    from sparse_rcnn_amd.synthetic import make_raw_sample
    sample = ("scene",) + make_raw_sample(15_000, 12, seed=21)
    kw = _crop_kw()
    seed, counter = 2 ** 63 + 5, 2 ** 40 + 1

    def refuse(*a, **k):
        raise AssertionError("the PhiloxDraws path draws nothing on the host")

    def convert(cnt):
        d = S.PhiloxDraws(seed, cnt, coord_noise_sigma=0.1)
        with monkeypatch.context() as mp:
            mp.setattr(torch, "randn", refuse)
            mp.setattr(S, "random_cut_start", refuse)
            out = S.convert_sample(sample, draws=d, required_size_factor=16, **kw)
        return d, out

    d, out = convert(counter)
    m = out[1].shape[0]
    print(f"[philox convert] start {d.start_positions.tolist()} order {d.cut_order} alive {d.cut_alive} M {m} kept {out[4].n_gt}")
    assert m > 500 and out[4].n_gt[0] >= 1 and d.cut_dims == 3 and d.cut_alive == m
    # the start is the restated random cut-out's, on the voxels the fixtures pin
    aug = R.matmul3(sample[1], d.almost_orthonormal * kw["scale"])
    discrete = (aug + (-aug.min(0).values + d.sub_pixel_offset)).long().numpy()
    start, order, alive, dims, inside = P.random_cut_out(discrete, [64, 64, 32], [0, 0, 0], seed, counter)
    assert d.start_positions.tolist() == start and d.cut_order == order and (alive, dims) == (m, 3)
    assert np.array_equal(out[7]["remaining_points"].cpu().numpy(), inside)
    # the same conversion given everything as a plain Draws: the path the reference's fixtures pin
    color, normal = out[7]["color_shift"].tensor(), out[7]["normals_shift"].tensor()
    assert color.is_cuda and tuple(color.shape) == (m, 3) and tuple(normal.shape) == (3,)
    given = S.Draws(d.almost_orthonormal, d.sub_pixel_offset, start_positions=d.start_positions, color_noise=color,
                    normal_noise=normal)
    twin = S.convert_sample(sample, draws=given, required_size_factor=16, **kw)
    _same(out, twin)
    assert torch.equal(twin[7]["color_shift"], color) and torch.equal(twin[7]["normals_shift"], normal)
    assert not torch.equal(out[2][:, :3], sample[2].to(gpu)[out[7]["remaining_points"]])        # the noise was added
    # the same (seed, counter) again: equal; the next counter: another sample
    d2, again = convert(counter)
    _same(out, again)
    assert torch.equal(d2.start_positions, d.start_positions)
    d3, other = convert(counter + 1)
    assert (not torch.equal(d3.start_positions, d.start_positions)) or other[2].shape != out[2].shape \
        or not torch.equal(other[2], out[2])
    # without noise the entries are the zero-dim zeros of the host-generator path
    quiet = S.convert_sample(sample, draws=S.PhiloxDraws(seed, counter, coord_noise_sigma=0.1), required_size_factor=16,
                             **dict(kw, color_noise_sigma=0, normal_noise_sigma=0))
    assert torch.equal(quiet[7]["color_shift"], torch.zeros(())) and torch.equal(quiet[7]["normals_shift"], torch.zeros(()))
    assert torch.equal(quiet[2][:, :3], sample[2].to(gpu)[quiet[7]["remaining_points"]])


def test_scene_step_on_a_batch_converted_with_philox_draws(gpu):
    """Two such samples (15 000 points, 12 instances) collated with required_size_factor=32 and one cfg3-rpn step with the RPN and
    the mask loss on them.  The crop here is 128 x 128 x 64 voxels at 1 cm (the reference's training crop) and not the 64 x 64 x 32
    of the test above: the step's proposal selection takes the top 1024 anchors inside the scene, and a 64 x 64 x 32 scene holds
    fewer than that (torch.topk raises, as the reference's would)."""
    from sparse_rcnn_amd.sample import PhiloxDraws, collate, convert_sample
    from sparse_rcnn_amd.synthetic import make_raw_sample
    from sparse_rcnn_amd.trainstep import SceneStep
    kw = dict(_crop_kw(), spatial_size=(128, 128, 64), scale=1 / 0.01)
    outs = []
    for i in range(2):
        sample = (f"s{i}",) + make_raw_sample(15_000, 12, seed=21 + i)
        outs.append(convert_sample(sample, draws=PhiloxDraws(2 ** 63 + 5, 2 ** 40 + 1 + i, coord_noise_sigma=0.1), batch_index=i,
                                   required_size_factor=32, **kw))
    batch = collate(outs)
    print(f"[philox step] rows {batch['batch_splits']} instances {batch['gt_mask'].n_gt} size {batch['data'][2].tolist()}")
    assert min(batch["batch_splits"]) > 1000 and min(batch["gt_mask"].n_gt) >= 1
    assert [int(v) % 32 for v in batch["data"][2]] == [0, 0, 0]
    st = SceneStep("cfg3-rpn", batches=[batch], optimizer="adam", rpn_loss=True, mask_loss=True, prefetch=False, lr=1e-4)
    st.step()
    st.finish()
    for v in (st.rpn_losses[0], st.rpn_losses[1], st.mask_losses):
        assert bool(torch.isfinite(v.detach()).all())
