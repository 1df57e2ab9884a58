"""world_size-2 `gloo` test of StreamMeter.all_reduce on CPU: each rank feeds its shard of the videos; afterwards both ranks
hold the state of the unsharded run, bit for bit."""
import os
import socket
import sys

import numpy as np
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import _metrics_ref as mr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K, V, N, TOPK = 65, 3, 23, (1, 5)


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _inputs():
    x, y = mr.make_case(77, N, V, K, 2.0 ** -6)
    y[2], y[20] = -1, K                  # one bad label in each shard
    x[5, 1, 3], x[15, 0, 64] = np.nan, np.inf
    return torch.from_numpy(x).float(), torch.from_numpy(y)


def _feed(meter, x, y, lo, hi, step=4):
    for a in range(lo, hi, step):
        b = min(a + step, hi)
        meter.update(x[a:b], y[a:b])


def _worker(rank, world, port, out):
    sys.path.insert(0, ROOT)
    os.environ.update(RANK=str(rank), LOCAL_RANK=str(rank), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1",
                      MASTER_PORT=str(port))
    torch.set_num_threads(1)
    from rubiksnet_amd import dp
    from rubiksnet_amd.metrics import StreamMeter
    env = dp.init_distributed(prefer_gpu=False)
    x, y = _inputs()
    lo, hi = dp.shard_range(N, rank, world)
    meter = StreamMeter(K, topk=TOPK, views=V)
    _feed(meter, x, y, lo, hi)
    meter.all_reduce()
    idle = StreamMeter(K, topk=TOPK, views=V)          # a rank-local meter that saw nothing joins with zeros
    if rank == 0:
        _feed(idle, x, y, 0, N)
    idle.all_reduce()
    torch.save({"state": meter.state.clone(), "idle": idle.state.clone(), "range": (lo, hi), "backend": env.backend},
               os.path.join(out, "rank%d.pt" % rank))
    dist.barrier()
    dist.destroy_process_group()


def test_all_reduce_gives_every_rank_the_unsharded_state(tmp_path):
    from rubiksnet_amd.metrics import StreamMeter

    mp.spawn(_worker, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=True)
    r0 = torch.load(tmp_path / "rank0.pt")
    r1 = torch.load(tmp_path / "rank1.pt")
    assert r0["range"] == (0, 12) and r1["range"] == (12, 23) and r0["backend"] == "gloo"
    x, y = _inputs()
    whole = StreamMeter(K, topk=TOPK, views=V)
    _feed(whole, x, y, 0, N, step=7)
    for r in (r0, r1):
        assert torch.equal(r["state"], whole.state) and torch.equal(r["idle"], whole.state)
    ref = mr.reference(x.double().numpy(), y.numpy(), TOPK, True, 2.0 ** -6)
    assert ref["state"][0] == 21 and ref["state"][2] == 2 and ref["state"][3] == 2
    mr.check_state(r0["state"].numpy(), ref)
