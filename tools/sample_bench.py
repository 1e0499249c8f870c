"""Time of one sample conversion (stored scene -> training sample) three ways, on one MI355X:

  (a) sparse_rcnn_amd.sample.convert_sample: scn_vox_* + scn_sample_stats + scn_sample_pack;
  (b) the same operations as torch operators on device tensors -- what the reference's `load_using_gpu` mode runs
      (scannet_config/run.py:951: convert_sample on device tensors), restated with the draws given: tests/sample_restate.py
      `convert` on device inputs, with its Python loop and host wait per instance;
  (c) the same restatement on the CPU with 16 torch threads (what a DataLoader worker runs).

Two shapes: one scene of ~200 000 points / 40 instances with a fixed cut-out that keeps most of it, and the reference's training
batch, 12 random crops of 128 x 128 x 64 voxels (run.py:364,485-488), converted and collated.  Inputs are resident on the device
for (a) and (b), as a training run that keeps its scenes in HBM has them; the draws are made on the host beforehand.  Every
timed window ends in a device synchronise; each variant is warmed up, then the variants alternate for `--repeats` rounds and the
median and the range over the rounds are printed.  Launches are counted with torch's profiler in a separate, untimed call.

`--draws` says where the random numbers of (a) come from.  `given` (default): made on the host beforehand and handed in, the
measurement above.  `host`: `convert_sample(draws=None)` -- the matrix, the random cut-out's start (random_cut_start: three small
reads) and the per-point noise (torch.randn on the CPU, copied from pageable memory) are drawn inside the timed call, which is
what a training loop on the host generator pays.  `device`: `PhiloxDraws` -- the start from scn_sample_cut_start, the noise
inside scn_sample_pack_drawn.  `host` and `device` time (a) alone; every round draws afresh (round r: torch.manual_seed(r) /
sample counters from r * samples), so the kept-row counts differ a little from round to round and between the two.

    python tools/sample_bench.py [--repeats 15] [--draws given|host|device] [--out profiles/sample_convert.txt]
"""
import argparse
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import sample_restate as R                                                      # noqa: E402
from test_gpu_sample import _device_convert, _training_kw, _training_mappers                      # noqa: E402


def timed(fn, sync):
    t = time.perf_counter()
    fn()
    if sync:
        torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3


def count_launches(fn):
    """(kernel launches, memsets, memcpys) of one call, from torch's profiler; None where the profiler gives no device events."""
    try:
        from torch.profiler import ProfilerActivity, profile
        fn()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        k = ms = mc = 0
        for e in prof.events():
            if str(getattr(e, "device_type", "")).endswith("CUDA"):
                name = e.name.lower()
                if "memset" in name:
                    ms += 1
                elif "memcpy" in name:
                    mc += 1
                else:
                    k += 1
        return (k, ms, mc) if (k or ms or mc) else None
    except Exception as e:                                                      # noqa: BLE001
        return f"profiler failed: {type(e).__name__}"


def drawn_cases(args, cases, say):
    """(a) with its draws made inside the timed call: on the host (draws=None) or on the device (PhiloxDraws)."""
    from sparse_rcnn_amd.sample import PhiloxDraws, collate, convert_sample
    kept = []

    def run(items, r):
        if args.draws == "host":
            torch.manual_seed(r)
        outs = []
        for i, (_, d, k) in enumerate(items):
            draws = PhiloxDraws(1234, r * len(items) + i, coord_noise_sigma=0.1) if args.draws == "device" else None
            outs.append(convert_sample(
                d, spatial_size=k["spatial_size"], shift=k["shift"], instance_cutoff_threshold=0.8, color_noise_sigma=0.1,
                common_color_noise=False, normal_noise_sigma=0, common_normal_noise=False, use_color=True, use_ones=True,
                use_normal=True, additional_bbox_pixel=0, background_label=-100, scale=k["scale"],
                instance_label_mapper=k["instance_label_mapper"], segmentation_label_mapper=k["segmentation_label_mapper"],
                coord_noise_sigma=0.1, draws=draws))
        kept.append(sum(int(o[1].shape[0]) for o in outs))
        return collate(outs) if len(outs) > 1 else outs

    for title, items in cases.items():
        n = sum(s[0].shape[0] for s, _, _ in items)
        for r in range(3):
            run(items, 1000 + r)
        torch.cuda.synchronize()
        del kept[:]
        t = [timed(lambda: run(items, r), True) for r in range(args.repeats)]
        say(f"== {title}: {len(items)} sample(s), {n} stored points, kept per round {min(kept)} .. {max(kept)}, 40 instances each ==")
        say(f"  (a) device path, draws = {args.draws:6s}                median {statistics.median(t):8.3f} ms   min {min(t):8.3f}   "
            f"max {max(t):8.3f}   per sample {statistics.median(t) / len(items):8.3f} ms   ({len(t)} rounds)")
        say(f"  device activities of one call (kernels, memsets, memcpys): {count_launches(lambda: run(items, 0))}")
    say("host waits per sample, by construction: the kept-row count and the shift/extent copy of augment_coords + ONE copy of the "
        "(I + 1) x 8 instance table; the random cut-out: + 3 reads in random_cut_start (host) or + 1 read of 32 bytes (device)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--points", type=int, default=200_000)
    ap.add_argument("--draws", choices=("given", "host", "device"), default="given")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("sample_bench needs an MI355X: there is no CPU timing of the device path")
    torch.set_num_threads(16)
    from sparse_rcnn_amd.sample import collate
    from sparse_rcnn_amd.synthetic import make_raw_sample
    dev = torch.device("cuda", 0)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    scene = make_raw_sample(args.points, 40, seed=1)
    crops_raw = [make_raw_sample(args.points, 40, seed=2 + i) for i in range(3)]
    on_dev = lambda s: tuple(t.to(dev) for t in s[:4]) + (s[4],)               # noqa: E731
    cases = {}
    if args.draws != "given":                                                   # no draws to prepare: the shapes and the mappers
        inst, seg = _training_mappers()
        light = lambda size, shift: dict(spatial_size=size, shift=shift, scale=1 / 0.02, instance_label_mapper=inst,   # noqa: E731
                                         segmentation_label_mapper=seg)
        cases["one scene, fixed cut-out 320x320x160"] = [(scene, on_dev(scene), light((320, 320, 160), 0))]
        cases["12 random crops 128x128x64, collated"] = [(crops_raw[i % 3], on_dev(crops_raw[i % 3]), light((128, 128, 64), None))
                                                         for i in range(12)]
        drawn_cases(args, cases, say)
        if args.out:
            with open(args.out, "w") as f:
                f.write("\n".join(lines) + "\n")
        return
    kw = _training_kw(scene, seed=5, spatial_size=(320, 320, 160), shift=0)
    cases["one scene, fixed cut-out 320x320x160"] = [(scene, on_dev(scene), kw)]
    crops = []
    for i in range(12):
        s = crops_raw[i % 3]
        crops.append((s, on_dev(s), _training_kw(s, seed=30 + i, spatial_size=(128, 128, 64), random_cut=True)))
    cases["12 random crops 128x128x64, collated"] = crops

    for title, items in cases.items():
        n = sum(s[0].shape[0] for s, _, _ in items)
        m = sum(int(R.convert(*s, **k)["coords"].shape[0]) for s, _, k in items)

        def run_a():
            outs = [_device_convert(d, k) for _, d, k in items]
            return collate(outs) if len(outs) > 1 else outs

        def run_b():
            outs = [R.convert(*d[:4], d[4], **k) for _, d, k in items]
            return R.collate(outs) if len(outs) > 1 else outs

        def run_c():
            outs = [R.convert(*s, **k) for s, _, k in items]
            return R.collate(outs) if len(outs) > 1 else outs

        for _ in range(3):
            run_a(); run_b()
        run_c()
        torch.cuda.synchronize()
        ta, tb, tc = [], [], []
        for r in range(args.repeats):
            ta.append(timed(run_a, True))
            tb.append(timed(run_b, True))
            if r < 5:
                tc.append(timed(run_c, False))
        say(f"== {title}: {len(items)} sample(s), {n} stored points, {m} kept, 40 instances each ==")
        for name, t in (("(a) device path (scn_vox_* + scn_sample_*)", ta), ("(b) torch operators on device tensors", tb),
                        ("(c) restatement on the CPU, 16 threads", tc)):
            say(f"  {name:44s} median {statistics.median(t):8.3f} ms   min {min(t):8.3f}   max {max(t):8.3f}   "
                f"per sample {statistics.median(t) / len(items):8.3f} ms   ({len(t)} rounds)")
        la, lb = count_launches(run_a), count_launches(run_b)
        say(f"  device activities of one call (kernels, memsets, memcpys): (a) {la}   (b) {lb}")
    say("host waits per sample, by construction: (a) the kept-row count and the shift/extent copy of augment_coords + ONE copy of the "
        "(I + 1) x 8 instance table (the random cut-out: + 3 reads in random_cut_start when the start is not given); "
        "(b) one per instance for the ratio, one per boolean-mask index, one for the labels: > 40")
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
