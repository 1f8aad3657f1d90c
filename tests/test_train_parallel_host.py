"""Host side of the accumulated / data-parallel training step, no GPU: the batch plan as a pure function, the self-launcher with
stand-in children, reduce_flat over a two-rank gloo group, and the command line's argument errors."""
import os
import socket
import subprocess
import sys
import time

import pytest
import torch
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _env():
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_PORT")}
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    return env


def test_micro_batch_mapping_and_divisibility_errors():
    from etch_amd.train import micro_batch_size, micro_batches
    assert micro_batch_size(8, 2, 2) == 2 and micro_batch_size(1) == 1
    # micro-batch m = rank * K + k covers items [m * mb, (m + 1) * mb): together the ranks tile the global batch in order
    for batch, gpus, K in ((8, 2, 2), (6, 3, 1), (4, 1, 4), (12, 2, 3), (2, 2, 1), (2, 1, 2)):
        mb = batch // (gpus * K)
        spans = [s for r in range(gpus) for s in micro_batches(batch, gpus, K, r)]
        assert spans == [(m * mb, (m + 1) * mb) for m in range(gpus * K)]
        assert micro_batches(batch, gpus, K, gpus - 1)[0] == ((gpus - 1) * K * mb, (gpus - 1) * K * mb + mb)
    for bad in ((3, 2, 1), (4, 1, 3), (2, 2, 2), (0, 1, 1), (4, 0, 1), (4, 1, 0)):
        with pytest.raises(ValueError):
            micro_batch_size(*bad)
    with pytest.raises(ValueError):
        micro_batches(4, 2, 1, 2)


class _Items:
    """A stand-in dataset: items are their index; records what precompute was asked for."""

    def __init__(self, n):
        self.id_list = [f"id{i:02d}" for i in range(n)]
        self.asked = []

    def __len__(self):
        return len(self.id_list)

    def precompute(self, batch_size=8, ids=None):
        self.asked.append(list(ids))

    def __getitem__(self, i):
        return {"hitpts": torch.full((2, 3), float(i)), "id": self.id_list[i]}


def test_plan_depends_on_seed_and_batch_size_only():
    """The global batches are DataLoader(shuffle=True, drop_last=True)'s own for the seed, epoch after epoch and with the generator left in the same
    state; every (gpus, accumulate) split of them, ranks joined in order, gives the global batch back; a rank solves its own ids only."""
    from torch.utils.data import DataLoader

    from etch_amd.train import PlannedLoader, batch_plan
    n, batch = 13, 4
    g_ref, g_plan = torch.Generator().manual_seed(5), torch.Generator().manual_seed(5)
    ref_loader = DataLoader(range(n), batch_size=batch, shuffle=True, drop_last=True, generator=g_ref)
    epochs = []
    for _ in range(3):
        want = [b.tolist() for b in ref_loader]
        assert batch_plan(n, batch, g_plan) == want and len(want) == n // batch
        epochs.append(want)
    assert torch.equal(g_ref.get_state(), g_plan.get_state())
    assert epochs[0] != epochs[1]
    for gpus, K in ((1, 2), (2, 1), (2, 2), (4, 1), (1, 4)):
        per_rank = []
        for rank in range(gpus):
            ds, g = _Items(n), torch.Generator().manual_seed(5)
            loader = PlannedLoader(ds, batch, gpus, K, rank, g)
            raw = [list(loader) for _ in range(3)]
            assert all(b["local"] and len(b["id"]) == batch // gpus for ep in raw for b in ep)
            got = [[b["hitpts"][:, 0, 0].long().tolist() for b in ep] for ep in raw]
            assert torch.equal(g.get_state(), g_ref.get_state())
            for e, asked in enumerate(ds.asked):
                assert asked == sorted({ds.id_list[i] for b in got[e] for i in b})
            per_rank.append(got)
        for e in range(3):
            joined = [sum((per_rank[r][e][k] for r in range(gpus)), []) for k in range(n // batch)]
            assert joined == epochs[e], (gpus, K, e)


CHILD = "import os, sys, time\nr = int(os.environ['RANK'])\nprint('rank', r, 'of', os.environ['WORLD_SIZE'], os.environ['LOCAL_RANK'], flush=True)\n"


def test_launch_ranks_passes_success_and_relays_rank_0(capsys):
    from etch_amd.parallel import launch_ranks
    assert launch_ranks([sys.executable, "-c", CHILD + "assert os.environ['MASTER_ADDR'] and int(os.environ['MASTER_PORT'])\n"], 3, timeout=60) == 0
    out = capsys.readouterr().out
    assert out == "rank 0 of 3 0\n"


def test_launch_ranks_stops_the_peers_of_a_failed_rank():
    from etch_amd.parallel import launch_ranks
    t0 = time.monotonic()
    rc = launch_ranks([sys.executable, "-c", CHILD + "sys.exit(3) if r == 1 else time.sleep(120)\n"], 2, timeout=60)
    assert rc == 3
    assert time.monotonic() - t0 < 30               # neither the peer's 120 s nor the 60 s limit was waited for


def test_launch_ranks_time_limit_and_world_bounds():
    from etch_amd.parallel import launch_ranks
    t0 = time.monotonic()
    assert launch_ranks([sys.executable, "-c", "import time\ntime.sleep(120)\n"], 2, timeout=0) == 124        # a limit already over: stopped at once
    assert time.monotonic() - t0 < 30
    for world in (0, 17):
        with pytest.raises(ValueError):
            launch_ranks([sys.executable, "-c", "pass"], world)


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _reduce_worker(rank, world, port, q):
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    from etch_amd import parallel as P
    P.init("gloo")
    t = torch.arange(11, dtype=torch.float32) * (0.5 if rank == 0 else 0.25) + rank
    t[3] = float("inf") if rank == 0 else 1.0
    out = P.reduce_flat(t)
    q.put((rank, out is t, t.tolist()))
    torch.distributed.destroy_process_group()


def test_reduce_flat_is_the_exact_sum_over_a_two_rank_gloo_group():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_reduce_worker, args=(r, 2, port, q)) for r in range(2)]
    [p.start() for p in procs]
    res = sorted(q.get(timeout=120) for _ in range(2))
    [p.join(timeout=60) for p in procs]
    want = (torch.arange(11, dtype=torch.float32) * 0.5 + (torch.arange(11, dtype=torch.float32) * 0.25 + 1)).tolist()
    want[3] = float("inf")
    assert all(in_place for _, in_place, _ in res)
    assert res[0][2] == want and res[1][2] == want


def test_reduce_flat_without_a_group_is_a_no_op():
    from etch_amd import parallel as P
    t = torch.arange(5, dtype=torch.float32)
    assert P.reduce_flat(t) is t and t.tolist() == [0.0, 1.0, 2.0, 3.0, 4.0]


@pytest.mark.parametrize("argv, needle", [
    (["--gpus", "2", "--batch_size", "3"], "multiple of gpus * accumulate"),
    (["--accumulate", "2", "--batch_size", "3"], "multiple of gpus * accumulate"),
    (["--gpus", "32", "--batch_size", "32"], "at most 16"),
    (["--reference_step", "--accumulate", "2", "--batch_size", "2"], "literal single-device step"),
])
def test_command_line_argument_errors_come_before_any_gpu_work(argv, needle):
    r = subprocess.run([sys.executable, "-m", "etch_amd.train", *argv], env=_env(), cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 2, (r.returncode, r.stderr[-400:])
    assert needle in r.stderr and "error:" in r.stderr
    assert "needs a GPU" not in r.stderr and "Traceback" not in r.stderr
