"""Helper of tests/test_gpu_clip.py::test_two_ranks_clip_the_mean_gradient_alike -- ONE rank of a data-parallel Adam step of the
cfg2 backbone at the tests' tiny shape with gradient clipping on, run as a fresh process (RANK / WORLD_SIZE / MASTER_* in the
environment, gloo collective so that two ranks may share one GPU).  Writes the clip's record, the packed gradient buffer as the
clip found it (the sum over ranks) and as it left it, and the parameters before and after the update.

argv: out.npz max_grad_norm"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np
import torch
import torch.distributed as dist


def main():
    out_path, bound = sys.argv[1], float(sys.argv[2])
    rank = int(os.environ["RANK"])
    torch.cuda.set_device(0)
    dist.init_process_group("gloo")
    from sparse_rcnn_amd.trainstep import SceneStep
    job = SceneStep("cfg2", torch.device("cuda", 0), prefetch=False, seed=10 + rank, grad_seed=100 + rank, n_buckets=2,
                    channels=(16, 32), target=500, grid=(32, 32, 16), optimizer="adam", max_grad_norm=bound)
    assert job.flat.buckets, "the bucketed, overlapped all-reduce must be active with 2 ranks"
    params0 = job.flat.flat.cpu().numpy().copy()
    seen = {"clips": 0}
    inner = job.flat.clip_grad_norm

    def spy(*a, **k):                           # the packed buffer as the clip finds it: after the reduction, before the update
        seen["clips"] += 1
        seen["reduced"] = job.flat.flat_grad.clone()
        seen["grad_scale"] = job.flat.grad_scale
        return inner(*a, **k)
    job.flat.clip_grad_norm = spy
    job.step()
    job.finish()
    torch.cuda.synchronize()
    np.savez(out_path, record=job.flat.clip_record.cpu().numpy(), reduced=seen["reduced"].cpu().numpy(),
             scaled=job.flat.flat_grad.cpu().numpy(), params0=params0, params=job.flat.flat.cpu().numpy(),
             clips=seen["clips"], grad_scale=seen["grad_scale"], bound=bound)
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
