"""LAMB under data parallel: two gloo ranks on the one GPU of the test box (as tests/test_gpu_dp_ranks.py runs the kinds before
it), the all-reduce form - the sharded update is refused under a trust kind.  Every rank runs the norms pass, the finish and the
update on the same reduced gradient, so the replicas stay bit-identical and hold the same ratios after three steps."""
import os
import sys

import numpy as np
import pytest
import torch

from test_gpu_dp_ranks import B, HERE, STEPS, _free_port, _problem

pytestmark = pytest.mark.gpu
WORLD = 2


def _trainer(distributed):
    from codae.tool import Optimizer
    from codae.train import HipEmbeddingTrainer
    sched, params, data, bm, mtu, order = _problem()
    tr = HipEmbeddingTrainer(sched, torch.tensor(data), torch.tensor(bm).to(torch.uint8), torch.tensor(mtu), 1e-3, 1e-4, 1.0,
                             max_batch=B, precision="bf16", device="cuda:0", distributed=distributed, n_buckets=4,
                             sharded_update=False, optimizer=Optimizer("lamb"))
    tr.load_params(params)
    return tr, order


def _worker(rank, world, port, out_dir):
    for p in (os.path.dirname(HERE), os.path.join(os.path.dirname(HERE), "mui-deepautoencoder_amd"), HERE):
        if p not in sys.path:
            sys.path.insert(0, p)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    os.environ["CODAE_NO_CHAIN"] = "1"
    import torch.distributed as dist
    from codae.train import shard_batch
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        tr, order = _trainer(True)
        assert tr.dp.world == world and not tr.dp.sharded
        for idx in order:
            mine = shard_batch(torch.tensor(idx, dtype=torch.int32), rank, world)
            tr.train_batch(mine.to("cuda:0"), run=0, global_rows=len(idx))
        torch.cuda.synchronize()
        agree = tr.dp.replicas_agree()
        np.save(os.path.join(out_dir, "agree_%d.npy" % rank), np.asarray([bool(agree)]))
        np.save(os.path.join(out_dir, "params_%d.npy" % rank), tr.engine.params.cpu().numpy())
        np.save(os.path.join(out_dir, "m_%d.npy" % rank), tr.engine.adam_m.cpu().numpy())
        np.save(os.path.join(out_dir, "shadow_%d.npy" % rank), tr.engine.shadow.view(torch.int16).cpu().numpy())
        np.save(os.path.join(out_dir, "ratios_%d.npy" % rank), tr.trust_ratios().cpu().numpy())
    finally:
        dist.destroy_process_group()


def test_two_ranks_under_lamb_stay_bit_identical_with_equal_ratios(tmp_path):
    import torch.multiprocessing as mp
    mp.spawn(_worker, args=(WORLD, _free_port(), str(tmp_path)), nprocs=WORLD, join=True)
    load = lambda name: [np.load(tmp_path / ("%s_%d.npy" % (name, r))) for r in range(WORLD)]
    for name in ("params", "m", "shadow", "ratios"):
        a, b = load(name)
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), "%s differs between the replicas" % name
    assert all(bool(x[0]) for x in load("agree")), "replicas_agree() is false"
    ratios = load("ratios")[0]
    assert ratios.dtype == np.float32 and ratios.shape == (len(_problem()[0]),) and np.isfinite(ratios).all() and (ratios > 0).all(), ratios
    assert STEPS == 3
