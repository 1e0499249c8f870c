"""Deterministic synthetic ScanNet-shaped voxel clouds (SURVEY.md §8d "Synthetic inputs").

Produces the reference's input contract (ndsis/data/data.py:88-115 ``collate_fn``):
``coords`` int64 CPU ``[Npts,4]`` = (x,y,z,batch), sample-major, duplicates allowed;
``feats`` fp32 ``[Npts,7]`` (3 colour in [-1,1], 1 ones, 3 unit normal); ``spatial_size`` int64 [3].
"""
from __future__ import annotations

import numpy as np
import torch


def _surface_voxels(rng, grid, n_cuboids=20, n_planes=3, scale=0.9):
    """Room shell + furniture shells + tilted planes, 1 voxel thick with +-1 jitter.  `scale` = room extent as a
    fraction of the grid (the room sits in the grid centre), chosen by the caller so that the raw surface has about
    the target number of voxels -- surfaces stay dense (ScanNet-like ~9-10 rules per voxel), not thinned noise."""
    gx, gy, gz = grid
    pts = []
    x0, x1 = int(gx * (0.5 - scale / 2)), int(gx * (0.5 + scale / 2))
    y0, y1 = int(gy * (0.5 - scale / 2)), int(gy * (0.5 + scale / 2))
    z0, z1 = int(gz * (0.5 - scale / 2)), int(gz * (0.5 + scale / 2))
    gx, gy, gz = max(x1 - x0, 8), max(y1 - y0, 8), max(z1 - z0, 8)        # furniture sizes relative to the room
    xs, ys = np.meshgrid(np.arange(x0, x1), np.arange(y0, y1), indexing="ij")
    pts.append(np.stack([xs.ravel(), ys.ravel(), np.full(xs.size, z0)], 1))
    xs, zs = np.meshgrid(np.arange(x0, x1), np.arange(z0, z1), indexing="ij")
    for y in (y0, y1 - 1):
        pts.append(np.stack([xs.ravel(), np.full(xs.size, y), zs.ravel()], 1))
    ys, zs = np.meshgrid(np.arange(y0, y1), np.arange(z0, z1), indexing="ij")
    for x in (x0, x1 - 1):
        pts.append(np.stack([np.full(ys.size, x), ys.ravel(), zs.ravel()], 1))
    # furniture: cuboid shells standing on the floor
    for _ in range(n_cuboids):
        ex = rng.integers(max(4, gx // 32), max(6, gx // 6), size=3)
        ex[2] = min(ex[2], (z1 - z0) // 2)
        cx = rng.integers(x0 + 1, max(x0 + 2, x1 - ex[0] - 1))
        cy = rng.integers(y0 + 1, max(y0 + 2, y1 - ex[1] - 1))
        lo = np.array([cx, cy, z0 + 1]); hi = lo + ex
        a, b = np.meshgrid(np.arange(lo[0], hi[0]), np.arange(lo[1], hi[1]), indexing="ij")
        pts.append(np.stack([a.ravel(), b.ravel(), np.full(a.size, hi[2])], 1))            # top
        a, c = np.meshgrid(np.arange(lo[0], hi[0]), np.arange(lo[2], hi[2]), indexing="ij")
        for y in (lo[1], hi[1] - 1):
            pts.append(np.stack([a.ravel(), np.full(a.size, y), c.ravel()], 1))
        b, c = np.meshgrid(np.arange(lo[1], hi[1]), np.arange(lo[2], hi[2]), indexing="ij")
        for x in (lo[0], hi[0] - 1):
            pts.append(np.stack([np.full(b.size, x), b.ravel(), c.ravel()], 1))
    # a few tilted planes
    for _ in range(n_planes):
        w = rng.integers(gx // 8, gx // 3); h = rng.integers(gy // 8, gy // 3)
        ox = rng.integers(x0, max(x0 + 1, x1 - w)); oy = rng.integers(y0, max(y0 + 1, y1 - h))
        sx, sy = rng.uniform(-0.4, 0.4, 2)
        a, b = np.meshgrid(np.arange(w), np.arange(h), indexing="ij")
        z = (z0 + (z1 - z0) * 0.4 + sx * a + sy * b).astype(np.int64)
        pts.append(np.stack([ox + a.ravel(), oy + b.ravel(), z.ravel()], 1))
    p = np.concatenate(pts).astype(np.int64)
    p += rng.integers(-1, 2, size=p.shape) * (rng.random(p.shape) < 0.15)                    # +-1 voxel jitter
    p = np.clip(p, 0, np.array(grid) - 1)
    p = np.unique(p, axis=0)
    return p[(p[:, 0] >= x0) & (p[:, 0] < x1) & (p[:, 1] >= y0) & (p[:, 1] < y1)]


def make_scene(grid=(512, 512, 256), target_active=150_000, dup=1.15, seed=1, uniform=False):
    """One sample.  Returns (coords int64 [Npts,3], feats fp32 [Npts,7], n_active)."""
    rng = np.random.default_rng(seed)
    grid = tuple(int(g) for g in grid)
    if uniform:
        lin = rng.choice(grid[0] * grid[1] * grid[2], size=target_active, replace=False)
        vox = np.stack(np.unravel_index(lin, grid), 1).astype(np.int64)
    else:
        lo, hi = 0.05, 0.98                                          # bisect the room scale for ~1.04 x target voxels
        state = rng.bit_generator.state
        for _ in range(14):
            mid = 0.5 * (lo + hi)
            rng.bit_generator.state = state
            vox = _surface_voxels(rng, grid, scale=mid)
            if len(vox) < 1.04 * target_active:
                lo = mid
            else:
                hi = mid
        rng.bit_generator.state = state
        vox = _surface_voxels(rng, grid, scale=hi)
        tries = 0
        while len(vox) < target_active and tries < 8:                                       # grid too small: densify
            extra = _surface_voxels(rng, grid, n_cuboids=40, n_planes=6, scale=0.98)
            vox = np.unique(np.concatenate([vox, extra]), axis=0)
            tries += 1
        if len(vox) > target_active:
            vox = vox[np.sort(rng.choice(len(vox), size=target_active, replace=False))]
    n_active = len(vox)
    n_dup = int(round(n_active * (dup - 1.0)))
    pts = np.concatenate([vox, vox[rng.integers(0, n_active, size=n_dup)]]) if n_dup else vox
    # mesh-vertex-like order: spatially coherent blocks, shuffled inside a block
    key = (pts[:, 0] // 16) * 1_000_000 + (pts[:, 1] // 16) * 1000 + pts[:, 2] // 16
    pts = pts[np.lexsort((rng.random(len(pts)), key))]
    colour = rng.uniform(-1, 1, size=(len(pts), 3))
    normal = rng.normal(size=(len(pts), 3)); normal /= np.linalg.norm(normal, axis=1, keepdims=True)
    feats = np.concatenate([colour, np.ones((len(pts), 1)), normal], 1).astype(np.float32)
    return pts, feats, n_active


def make_batch(n_scenes=1, grid=(512, 512, 256), target_active=150_000, dup=1.15, seed=1, uniform=False,
               cin=7):
    """collate_fn-shaped batch: (coords [Npts,4] int64 CPU, feats [Npts,cin] fp32, spatial_size [3] int64,
    batch_size, batch_splits)."""
    cs, fs, splits = [], [], []
    for b in range(n_scenes):
        p, f, _ = make_scene(grid, target_active, dup, seed + b, uniform)
        cs.append(np.concatenate([p, np.full((len(p), 1), b, np.int64)], 1))
        fs.append(f[:, :cin] if cin <= 7 else np.tile(f, (1, (cin + 6) // 7))[:, :cin])
        splits.append(len(p))
    coords = torch.from_numpy(np.concatenate(cs))
    feats = torch.from_numpy(np.ascontiguousarray(np.concatenate(fs)))
    return coords, feats, torch.tensor(grid, dtype=torch.long), n_scenes, splits


def make_boxes(coords, n_boxes=64, seed=3, lo=8.0, hi=96.0):
    """cfg-3 boxes: centres on random points, edge lengths log-uniform lo..hi voxels, fp32 non-integer corners.
    Returns a list (one per sample) of fp32 [n,2,3] tensors (start, stop)."""
    rng = np.random.default_rng(seed)
    c = coords.numpy() if isinstance(coords, torch.Tensor) else np.asarray(coords)
    out = []
    for b in range(int(c[:, 3].max()) + 1 if len(c) else 0):
        pts = c[c[:, 3] == b][:, :3]
        ctr = pts[rng.integers(0, len(pts), size=n_boxes)].astype(np.float64)
        edge = np.exp(rng.uniform(np.log(lo), np.log(hi), size=(n_boxes, 3)))
        start = ctr - edge / 2 + rng.uniform(0, 1, size=(n_boxes, 3))
        stop = start + edge
        out.append(torch.from_numpy(np.stack([start, stop], 1).astype(np.float32)))
    return out


def make_instances(coords, boxes, n_classes=18, seed=5):
    """Synthetic ground-truth instances for the scene's boxes: per sample, (labels int64 [G_s] uniform over n_classes,
    masks bool [G_s, N_s] over the sample's point rows, duplicates included -- the reference's batch['gt_label'] /
    batch['gt_mask']).  Point p belongs to instance g if it lies inside box g under the ROI crop's own rule (floor(start)
    <= x < ceil(stop) per axis, as scn_roi_boxes / the reference's BBoxTransformerSlice + get_inside_indicator apply it) AND
    its voxel centre lies inside the ellipsoid inscribed in the box: some of a box's points, not all of them.
    Deterministic, on the host.  -> (labels list, masks list) of CPU tensors."""
    rng = np.random.default_rng(seed)
    c = coords.numpy() if isinstance(coords, torch.Tensor) else np.asarray(coords)
    labels, masks = [], []
    for b, bx in enumerate(boxes):
        pts = c[c[:, 3] == b][:, :3]
        bx = (bx.numpy() if isinstance(bx, torch.Tensor) else np.asarray(bx)).astype(np.float32).reshape(-1, 2, 3)
        g = len(bx)
        labels.append(torch.from_numpy(rng.integers(0, n_classes, size=g).astype(np.int64)))
        lo, hi = np.floor(bx[:, 0]).astype(np.int64), np.ceil(bx[:, 1]).astype(np.int64)
        ctr = (bx[:, 0].astype(np.float64) + bx[:, 1]) / 2
        rad = (bx[:, 1].astype(np.float64) - bx[:, 0]) / 2
        m = np.zeros((g, len(pts)), dtype=bool)
        centre = pts.astype(np.float64) + 0.5
        for i in range(g):
            inside = ((pts >= lo[i]) & (pts < hi[i])).all(1)
            r = np.where(rad[i] > 0, rad[i], 1.0)
            m[i] = inside & ((((centre - ctr[i]) / r) ** 2).sum(1) <= 1.0)
        masks.append(torch.from_numpy(m))
    return labels, masks


def make_segmentation(labels, masks, offset=2):
    """Per-point semantic labels of a scene from its `make_instances` output: list (one per sample) of int64 [N_s] CPU
    tensors, `offset + label` of the lowest-numbered instance that holds the point and -100 (the reference's
    `background_label`, scannet_config/run.py:401: ignored by the segmentation loss) where none does."""
    out = []
    for lab, m in zip(labels, masks):
        lab = torch.as_tensor(lab, dtype=torch.int64)
        m = torch.as_tensor(m, dtype=torch.bool)
        seg = torch.full((m.shape[1],), -100, dtype=torch.int64)
        if m.shape[0]:
            first = torch.argmax(m.to(torch.uint8), dim=0)       # the first True of the column (0 if none)
            held = m.any(0)
            seg[held] = offset + lab[first[held]]
        out.append(seg)
    return out


def make_raw_sample(n_points=200_000, n_instances=40, voxel_size=0.02, grid=None, seed=1, n_raw_labels=41):
    """One scene in the reference's STORED format (what `sample.convert_sample` takes, ndsis/data/data.py:6-8 without the
    scene id): (coords fp32 [N,3] in metres, colors fp32 [N,3] in [-1,1], normals fp32 [N,3] unit, instance_ids int64 [N] with
    values 0 .. n_instances (n_instances = no instance), semantic_instance_labels_raw int64 [n_instances] in
    0 .. n_raw_labels-1), CPU tensors.  The surfaces are `make_scene`'s (about n_points points, 1.15 per voxel, mesh order), each
    point moved to a random place inside its voxel and scaled by voxel_size; instance g = the points inside a box around a
    random point (edges log-uniform grid/32 .. grid/5 voxels), the lowest-numbered box winning where boxes meet.  An instance
    may have no point."""
    rng = np.random.default_rng(seed + 77)
    target = max(int(n_points / 1.15), 64)
    if grid is None:
        side = 64
        while side < 1.6 * (target / 3) ** 0.5:
            side *= 2
        grid = (side, side, side // 2)
    pts, feats, _ = make_scene(grid, target, dup=1.15, seed=seed)
    coords = ((pts + rng.random(pts.shape)) * voxel_size).astype(np.float32)
    ids = np.full(len(pts), n_instances, np.int64)
    ctr = pts[rng.integers(0, len(pts), size=n_instances)].astype(np.float64)
    edge = np.exp(rng.uniform(np.log(grid[0] / 32), np.log(grid[0] / 5), size=(n_instances, 3)))
    for g in reversed(range(n_instances)):
        ids[(np.abs(pts - ctr[g]) <= edge[g] / 2).all(1)] = g
    labels_raw = rng.integers(0, n_raw_labels, size=n_instances).astype(np.int64)
    return (torch.from_numpy(coords), torch.from_numpy(np.ascontiguousarray(feats[:, :3])),
            torch.from_numpy(np.ascontiguousarray(feats[:, 4:7])), torch.from_numpy(ids), torch.from_numpy(labels_raw))
