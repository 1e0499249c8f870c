"""CPU: bench.py --dump-outputs writes what the last timed step handed its caller -- float32 .npy files within the 64 MB
budget, a fixed sample of the same positions for an array above its share, the parameter gradients from wherever the
step left them.  A stand-in step object on CPU tensors (the GPU run of the option: tests/test_gpu_atsize.py)."""
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
import bench  # noqa: E402


def _job(n_rows, packed, logits=True):
    g = torch.Generator().manual_seed(0)
    params = [torch.randn(64, 7, generator=g, requires_grad=True), torch.randn(5000, generator=g, requires_grad=True)]
    for p in params:
        p.grad = torch.randn(p.shape, generator=g)
    params[1].grad = None if not packed else params[1].grad          # a parameter the step left without a gradient
    flat = types.SimpleNamespace(params=params, flat=torch.cat([p.detach().reshape(-1) for p in params]),
                                 flat_grad_valid=packed)
    flat.mean_grad = lambda: torch.cat([p.grad.reshape(-1) for p in params])
    fin = torch.randn(n_rows, 7, generator=g).requires_grad_()
    fin.grad = torch.randn(n_rows, 7, generator=g)
    out = types.SimpleNamespace(features=torch.randn(n_rows, 32, generator=g).to(torch.bfloat16))
    return types.SimpleNamespace(out=out, fin=fin, flat=flat, rpn_out=None,
                                 logits=torch.randn(100, 18, generator=g) if logits else None)


def test_dump_writes_float32_arrays_whole_when_small(tmp_path):
    job = _job(1000, packed=False)
    info = bench.dump_outputs(job, str(tmp_path / "d"), torch)["arrays"]
    assert set(info) == {"output_features", "mask_logits", "input_features_grad", "param_grads", "params"}
    for name, meta in info.items():
        a = np.load(tmp_path / "d" / f"{name}.npy")
        assert a.dtype == np.float32 and not meta["sampled"] and list(a.shape) == meta["shape"]
    np.testing.assert_array_equal(np.load(tmp_path / "d" / "output_features.npy"), job.out.features.float().numpy())
    np.testing.assert_array_equal(np.load(tmp_path / "d" / "input_features_grad.npy"), job.fin.grad.numpy())
    g = np.load(tmp_path / "d" / "param_grads.npy")
    np.testing.assert_array_equal(g[:448], job.flat.params[0].grad.reshape(-1).numpy())
    assert not g[448:].any()                                            # no gradient: zeros, in FlatParams order
    np.testing.assert_array_equal(np.load(tmp_path / "d" / "params.npy"), job.flat.flat.numpy())


def test_dump_takes_the_packed_mean_gradient(tmp_path):
    job = _job(10, packed=True, logits=False)
    info = bench.dump_outputs(job, str(tmp_path), torch)["arrays"]
    assert "mask_logits" not in info
    np.testing.assert_array_equal(np.load(tmp_path / "param_grads.npy"), job.flat.mean_grad().numpy())


def test_dump_samples_large_arrays_at_fixed_positions_within_the_budget(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_ELEMS_PER_ARRAY", 4096)
    job = _job(1000, packed=False)
    info = bench.dump_outputs(job, str(tmp_path / "a"), torch)["arrays"]
    assert info["output_features"] == {"shape": [1000, 32], "sampled": True}
    assert info["mask_logits"]["sampled"] is False
    a = np.load(tmp_path / "a" / "output_features.npy")
    assert a.shape == (4096,) and a.dtype == np.float32
    full = job.out.features.float().numpy().reshape(-1)
    assert np.isin(a, full).all()
    bench.dump_outputs(job, str(tmp_path / "b"), torch)
    for name in info:
        np.testing.assert_array_equal(np.load(tmp_path / "a" / f"{name}.npy"), np.load(tmp_path / "b" / f"{name}.npy"))


def test_dump_budget_of_the_real_sizes_is_64_mb():
    # at most seven arrays (output, logits, rpn_bbox, rpn_score, input grad, parameter grads, parameters), float32
    assert 7 * bench.DUMP_ELEMS_PER_ARRAY * 4 <= 64 * 2 ** 20


def test_bench_accepts_the_option():
    a = bench.parse_args(["--steps", "7", "--dump-outputs", "out"])
    assert a.steps == 7 and a.dump_outputs == "out"
    d = bench.parse_args([])
    assert d.dump_outputs is None and d.lr == 0.0


def test_a_plain_run_takes_no_side_leg_and_full_takes_them_all(monkeypatch):
    """`--full` is off by default; without it no leg beyond the timed steps runs, whatever the --no-... options say, and the
    evaluation-only child is not started; with it every leg runs unless its own --no-... option leaves it out."""
    none = {"gpu": False, "fresh_child": False, "cpu_baseline": False}
    assert bench.parse_args([]).full is False
    for argv in ([], ["--gpus", "1", "--steps", "5", "--warmup", "2"], ["--no-extras"], ["--no-cpu-baseline"], ["--dropin"],
                 ["--gpus", "2"], ["--dump-outputs", "d"]):
        assert bench.side_legs(bench.parse_args(argv)) == none, argv
    assert bench.side_legs(bench.parse_args(["--full"])) == {"gpu": True, "fresh_child": True, "cpu_baseline": True}
    assert bench.side_legs(bench.parse_args(["--full", "--no-extras"])) == {"gpu": False, "fresh_child": False, "cpu_baseline": True}
    assert bench.side_legs(bench.parse_args(["--full", "--no-cpu-baseline"])) == {"gpu": True, "fresh_child": True, "cpu_baseline": False}
    # N ranks: every rank takes the GPU legs (their collectives stay matched); no child process, no CPU baseline
    assert bench.side_legs(bench.parse_args(["--full", "--gpus", "2"]), world=2) == {"gpu": True, "fresh_child": False, "cpu_baseline": False}

    started = []
    monkeypatch.setattr(bench, "_FRESH", None)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    monkeypatch.setattr(bench, "forward_only_fresh", lambda args: started.append("child") or {"ms_per_step": 1.0})
    monkeypatch.setattr(bench, "run", lambda args: started.append("run") or 0)
    for argv, want in ((["--gpus", "1", "--steps", "5", "--warmup", "2"], ["run"]), (["--full"], ["child", "run"])):
        del started[:]
        monkeypatch.setattr(sys, "argv", ["bench.py"] + argv)
        try:
            bench.main()
        except SystemExit as e:
            assert e.code == 0
        assert started == want, (argv, started)
