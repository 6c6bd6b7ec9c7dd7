"""Worker of tests/test_cabi_eval.py::test_metrics_two_ranks_gloo: RegressionMetrics.compute() over gloo with uneven
shards (rank 0 holds 3 batches, rank 1 holds 1), records made with numpy."""
import os
import sys

import numpy as np
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def worker(rank, world, port, tmpdir):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from eval_np import check_metrics, metrics, offset_pair, record
    from gan_danet_amd import kern as K
    from gan_danet_amd.evaluate import RegressionMetrics

    x, y = offset_pair(4000, seed=3)
    cuts = {0: [(0, 1000), (1000, 2000), (2000, 2900)], 1: [(2900, 4000)]}      # 3 + 1 batches, uneven counts
    m = RegressionMetrics("cpu", capacity=1)                                     # capacity 1: the store has to grow
    m.add_records([record(y[a:b], x[a:b]) for a, b in cuts[rank]])
    got = m.compute()
    single = K.eval_merge_host([record(y[a:b], x[a:b]) for r in range(world) for a, b in cuts[r]])[1]
    assert got == single, (rank, got, single)                                    # rank-major merge, bit for bit
    check_metrics(got, metrics(y, x), f"rank {rank}")
    both = [None] * world
    dist.all_gather_object(both, got)
    assert both[0] == both[1], both
    got2 = RegressionMetrics("cpu")                                              # a rank without any record
    if rank == 0:
        got2.add_records([record(y, x)])
    assert got2.compute(pad_to=1) == K.eval_merge_host([record(y, x)])[1]
    np.save(os.path.join(tmpdir, f"eval_ok{rank}.npy"), np.array([got[k] for k in ("n", "mse", "mae", "r2", "cc")]))
    dist.destroy_process_group()
