"""One process per rank over gloo on this host, for the tests of the sharded front ends (test_dist_gloo.py on the CPU,
test_gpu_dist.py with the ranks sharing one device)."""
import os
import socket

import torch.distributed as dist
import torch.multiprocessing as mp


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def init_gloo(rank, world, port):
    """A worker's first call: joins the test's process group."""
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)


def run_ranks(worker, world, args=(), get_timeout=120, join_timeout=60):
    """Spawns ``worker(rank, world, port, q, *args)`` for every rank, takes one item -- a tuple that starts with the rank
    -- from each off the queue, joins them and asserts that every one exited with 0.  Returns the items in rank order."""
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=worker, args=(r, world, port, q) + tuple(args)) for r in range(world)]
    for p in procs:
        p.start()
    res = sorted((q.get(timeout=get_timeout) for _ in range(world)), key=lambda item: item[0])
    for p in procs:
        p.join(timeout=join_timeout)
        assert p.exitcode == 0
    return res
