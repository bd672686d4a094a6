"""One rank of the sharded InversionEngine with precondition="illumination" on the smoke geometry
(tests/test_gpu_illumination.py launches it with torch.distributed.run).  Every rank uses cuda:0 of the one-GPU test
box and the gloo backend, as tests/dist_engine_worker.py.

Usage: python -m torch.distributed.run --nproc-per-node N tests/illum_engine_worker.py OUT.npz
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (HERE, ROOT, os.path.join(ROOT, "red-diffeq_amd")):
    sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402


def main(out):
    import test_gpu_illumination as T
    from red_diffeq.core import inversion as inv
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    dist.init_process_group("gloo")
    rank, world = dist.get_rank(), dist.get_world_size()
    ns = int(T.SMOKE["ns"])
    shots = (rank * ns // world, (rank + 1) * ns // world)
    mu0, vt, y = T.engine_inputs({"fwi": T.make_fwi()}, dev)          # the full survey's data, made on every rank
    fwi = T.make_fwi(shots=shots)
    sharded = [False]
    orig = inv._GradAllReduce.backward

    def backward(ctx, g):
        sharded[0] = True
        return orig(ctx, g)
    inv._GradAllReduce.backward = staticmethod(backward)
    trace = T.run_engine(dev, fwi, mu0, vt, y, precondition="illumination", precondition_every=2)
    mu = trace[-1].cpu().numpy()
    gathered = [torch.zeros(mu.size, dtype=torch.float64) for _ in range(world)]
    dist.all_gather(gathered, torch.from_numpy(mu.astype(np.float64).ravel()))
    if rank == 0:
        np.savez(out, mu=mu, same=np.array(all(torch.equal(g, gathered[0]) for g in gathered)),
                 sharded=np.array(bool(sharded[0])))
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main(sys.argv[1])
