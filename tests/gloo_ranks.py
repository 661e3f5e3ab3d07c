"""Multi-process gloo runs for the sharding tests: ``run(worker, world, args, n_results, timeout)`` starts ``world`` spawned
ranks in one gloo process group, each calling ``worker(rank, world, *args, q)``, and returns the ``n_results`` items the
ranks put on ``q``.  TEST INFRASTRUCTURE ONLY."""
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


def _rank_main(worker, rank, world, port, args, q):
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        worker(rank, world, *args, q)
    finally:
        dist.destroy_process_group()


def run(worker, world, args, n_results, timeout):
    """-> the ``n_results`` items put on the queue (each awaited ``timeout`` s), after every rank has exited with 0."""
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_rank_main, args=(worker, r, world, port, args, q)) for r in range(world)]
    for p in procs:
        p.start()
    got = [q.get(timeout=timeout) for _ in range(n_results)]
    for r, p in enumerate(procs):
        p.join(timeout=60)
        assert p.exitcode == 0, f"rank {r} exited with {p.exitcode}"
    return got
