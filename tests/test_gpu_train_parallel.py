"""Accumulated and data-parallel training steps: the pack kernel (csrc/train_step.hip: etch_grad_pack / etch_grad_unpack_tail) against
torch bit for bit, GuardedAdam stepping from the flat buffer, what `--accumulate` computes, two ranks against two micro-batches, the forced
world-size-1 RCCL group, the guards on the combined step, and --resume across modes.  Child processes run under a subprocess time limit; at most
two ranks have the GPU open."""
import json
import os
import socket
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

import _train_data as TD

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = (1, 3, 4, 5, 8191, 8192, 8193, 2 * 8192 + 3)          # the chunk is 8192
POISON = 0x5A5A5A5A
STAT_BUFFERS = ("running_mean", "running_var", "num_batches_tracked")


def _bits(t):
    return t.contiguous().view(torch.int32)


# ------------------------------------------------------------------------------------------------------------------ 1. the pack kernel
def _pack_case():
    from etch_amd.optim import GuardedAdam
    gen = torch.Generator().manual_seed(11)
    params = [torch.nn.Parameter(torch.randn(n, generator=gen).to(DEV)) for n in SIZES]
    opt = GuardedAdam(params)
    _, layout = opt.flat_gradients()
    g = opt._tables()[0]

    def grads(seed, none_at):
        gen = torch.Generator().manual_seed(seed)
        out = []
        for k, n in enumerate(SIZES):
            if k == none_at:
                out.append(None)
            elif n == 8193:                                   # a view one element into its storage: not 16-byte aligned
                store = torch.randn(n + 1, generator=gen).to(DEV)
                out.append(store[1:])
                assert out[-1].data_ptr() % 16 == 4 and out[-1].is_contiguous()
            else:
                out.append(torch.randn(n, generator=gen).to(DEV))
        nf = out[SIZES.index(8191)]
        nf[5], nf[4000], nf[8190] = float("nan"), float("inf"), float("-inf")
        return out
    return opt, g, layout, grads


def _table(grads):
    return torch.tensor([0 if x is None else x.data_ptr() for x in grads], dtype=torch.int64, device=DEV)


@pytest.mark.parametrize("scale", [1.0, 0.5, 1.0 / 3.0])
def test_pack_kernel_against_torch_bitwise(scale):
    """mode 0 is g * s, mode 1 is flat + g * s with the product and the sum rounded SEPARATELY -- torch's two kernels -- and not a fused multiply-add:
    for s = 1/3 the two differ in some element of these gradients, which the test checks, so it tells the two apart."""
    from etch_amd import ops
    opt, g, layout, grads = _pack_case()
    off, numel, tail, size = layout["offsets"], layout["numel"], layout["tail"], layout["size"]
    assert size == tail + ops.grad_tail_floats() and ops.guarded_adam_chunk() == 8192
    assert all(o % 4 == 0 for o in off) and tail % 4 == 0 and list(numel) == list(SIZES)
    assert all(off[k + 1] == off[k] + (numel[k] + 3) // 4 * 4 for k in range(len(SIZES) - 1))
    beyond = 16
    buf = torch.full((size + beyond,), POISON, dtype=torch.int32, device=DEV).view(torch.float32)
    s32 = torch.tensor(scale, dtype=torch.float32, device=DEV)
    none0, none1 = SIZES.index(5), SIZES.index(3)
    ga, gb = grads(1, none0), grads(2, none1)
    la, lb = torch.tensor([0.3, 1.7, 0.01, 4.2, 6.21], device=DEV), torch.tensor([0.9, 0.2, 7.0, 0.5, 8.6], device=DEV)
    sa, sb = torch.tensor([ops.TRAIN_STATUS_BAD_LABEL], dtype=torch.int32, device=DEV), torch.tensor([0], dtype=torch.int32, device=DEV)

    def pack(gr, mode, losses, status):
        ops.grad_pack(g["T"], g["C"], g["chunk_tensor"], g["first_chunk"], g["numel"], _table(gr), g["off"], buf, scale, mode, losses, status, tail,
                      layout=(off, numel))

    # mode 0
    want = buf.clone()
    for k, x in enumerate(ga):
        want[off[k]:off[k] + numel[k]] = 0.0 if x is None else x * s32
    want[tail:tail + 5] = la * s32
    want[tail + 5:tail + 8] = torch.tensor([0.0, 1.0, 0.0], device=DEV)
    pack(ga, 0, la, sa)
    assert torch.equal(_bits(buf), _bits(want))               # slots, zeros of the None slot, tail; padding and the region beyond still poison
    assert bool((_bits(buf[off[none0]:off[none0] + 5]) == 0).all())
    pad = torch.ones(size + beyond, dtype=torch.bool)
    for k in range(len(SIZES)):
        pad[off[k]:off[k] + numel[k]] = False
    pad[tail:size] = False
    assert int(pad.sum()) == beyond + sum((-n) % 4 for n in SIZES)
    assert bool((_bits(buf)[pad.to(DEV)] == POISON).all())
    # mode 1
    want1 = want.clone()
    fused, fma_differs = want.clone(), False
    for k, x in enumerate(gb):
        if x is None:
            continue                                           # untouched: the slot keeps mode 0's values
        sl = slice(off[k], off[k] + numel[k])
        prod = x * s32
        want1[sl] = want[sl] + prod
        fused[sl] = (want[sl].double() + x.double() * s32.double()).float()       # one rounding (up to fp64's own)
    want1[tail:tail + 5] = want[tail:tail + 5] + lb * s32
    sb[0] = ops.TRAIN_STATUS_NAN
    want1[tail + 5] += 1.0
    fused[tail:size] = want1[tail:size]                        # the FMA question is asked of the gradients
    pack(gb, 1, lb, sb)
    assert torch.equal(_bits(buf), _bits(want1))
    assert torch.equal(_bits(buf[off[none1]:off[none1] + 3]), _bits(want[off[none1]:off[none1] + 3]))
    finite = torch.isfinite(want1) & torch.isfinite(fused)
    fma_differs = bool((want1[finite] != fused[finite]).any())
    if scale == 1.0 / 3.0:
        assert fma_differs                                     # separate rounding is what the kernel defines, and these inputs tell it from an FMA
    else:
        assert not fma_differs                                 # s = 1, 0.5: the product is exact, both are the same sum
    nf = off[SIZES.index(8191)]
    assert bool(torch.isnan(buf[nf + 5])) and float(buf[nf + 4000]) == float("inf") and float(buf[nf + 8190]) == float("-inf")
    # the tail's round trip
    losses, status = ops.grad_unpack_tail(buf[tail:size])
    assert torch.equal(losses, la * s32 + lb * s32)
    assert int(status[0]) == ops.TRAIN_STATUS_NAN | ops.TRAIN_STATUS_BAD_LABEL
    clean = buf[tail:size].clone()
    clean[5:7] = 0.0
    assert int(ops.grad_unpack_tail(clean)[1][0]) == 0
    # no tail asked for: the tail is left alone
    before = buf.clone()
    ops.grad_pack(g["T"], g["C"], g["chunk_tensor"], g["first_chunk"], g["numel"], _table(ga), g["off"], buf, scale, 0, layout=(off, numel))
    assert torch.equal(_bits(buf[tail:]), _bits(before[tail:]))
    # the wrapper refuses, on the host, a layout the buffer does not hold: a short buffer, a slot into the tail, an offset that is no multiple of 4
    from etch_amd._lib import EtchHipError
    shifted = off.copy()
    shifted[-1] += 4
    before = buf.clone()
    for kw in (dict(flat=buf[:tail - 4], tail_offset=-1, layout=(off, numel)), dict(flat=buf, tail_offset=tail, layout=(shifted, numel)),
               dict(flat=buf, tail_offset=-1, layout=(off + 1, numel)), dict(flat=buf, tail_offset=-1, layout=(off[:-1], numel[:-1]))):
        with pytest.raises(EtchHipError):
            ops.grad_pack(g["T"], g["C"], g["chunk_tensor"], g["first_chunk"], g["numel"], _table(ga), g["off"], kw["flat"], scale, 0, None, None,
                          kw["tail_offset"], layout=kw["layout"])
    assert torch.equal(_bits(buf), _bits(before))


# ------------------------------------------------------------------------------------------------------------------ 2. Adam from the flat buffer
def test_guarded_adam_from_the_flat_buffer_is_the_step_from_grad():
    from etch_amd.optim import GuardedAdam
    gen = torch.Generator().manual_seed(21)
    start = [torch.randn(n, generator=gen) for n in SIZES]
    twins = []
    for _ in range(2):
        params = [torch.nn.Parameter(t.clone().to(DEV)) for t in start]
        twins.append((params, GuardedAdam(params, lr=1e-2)))
    none_at, nan_at = SIZES.index(4), SIZES.index(8193)
    for step in range(3):
        gen = torch.Generator().manual_seed(100 + step)
        gr = [torch.randn(n, generator=gen).to(DEV) for n in SIZES]
        gr[nan_at][77] = float("nan")
        for params, _ in twins:
            for k, p in enumerate(params):
                p.grad = None if k == none_at else gr[k].clone()
        twins[0][1].step()
        twins[1][1].accumulate(1.0, first=True)
        twins[1][1].step()
    (pa, oa), (pb, ob) = twins
    for k in range(len(SIZES)):
        assert torch.equal(_bits(pa[k]), _bits(pb[k])), k
        if k == none_at:
            assert "exp_avg" not in oa.state.get(pa[k], {}) and "exp_avg" not in ob.state.get(pb[k], {})
            assert torch.equal(pa[k].detach().cpu(), start[k])
            continue
        for name in ("exp_avg", "exp_avg_sq", "step"):
            assert torch.equal(_bits(oa.state[pa[k]][name]), _bits(ob.state[pb[k]][name])), (k, name)
        assert float(ob.state[pb[k]]["step"]) == 3.0
    assert oa.report() == ob.report() and ob.report()["tensors_zeroed"] == 3
    assert not torch.equal(pb[0].detach().cpu(), start[0])
    sa, sb = oa.state_dict(), ob.state_dict()
    assert sa["param_groups"] == sb["param_groups"] and list(sa["state"]) == list(sb["state"])


# ------------------------------------------------------------------------------------------------------------------ the program
@pytest.fixture(scope="module")
def data(tmp_path_factory):
    return TD.build(tmp_path_factory.mktemp("train_parallel_data"), DEV)


@pytest.fixture(scope="module")
def setup(data):
    """The parsed arguments and the one global batch of the dataset, for the tests that drive train() themselves."""
    from etch_amd import train
    from etch_amd.datasets import GTDataset
    args = train.build_parser().parse_args(data.flags + ["--output_root", os.path.join(data.root, "direct")])
    args.pred_items = args.pred_items.split(",")
    args.device = torch.device("cuda:0")
    args.output_folder = os.path.join(data.root, "direct")
    with open(args.markerset_path) as fh:
        args.markerset = json.load(fh)
    ds = GTDataset(args, device=args.device, verbose=False)
    items = [ds[0], ds[1]]
    batch = {k: torch.stack([it[k] for it in items]) for k in ("hitpts", "vectors", "confidences", "labels")}
    return types.SimpleNamespace(args=args, batch=batch)


def _fresh(setup, **over):
    from etch_amd import train
    args = types.SimpleNamespace(**vars(setup.args))
    for k, v in over.items():
        setattr(args, k, v)
    train.default_stuff(args.seed)
    model = train.make_model(args)
    return args, model, train.make_optimizer(args, model)


def test_accumulation_is_half_of_each_micro_batch_gradient(setup):
    """accumulate = 2 on one global batch of 2: the combined flat gradient is g0 * 0.5 + g1 * 0.5 bit for bit, g0 and g1 being what the plain path
    leaves in .grad for each item alone from the same start.  The losses are the mean of the two runs': each loss * 0.5 is exact and their fp32 sum
    rounds once, against a mean formed in fp64 from two fp32 values -- within 2^-22 relative, as one rounding per contribution plus one for the
    sum of non-negative terms bounds it."""
    from etch_amd import train
    seen = []
    args, model, opt = _fresh(setup, accumulate=2, on_step=seen.append)
    start = {k: v.detach().clone() for k, v in model.named_parameters()}
    train.train(args, model, opt, [setup.batch])
    flat, layout = seen[0]["flat_gradients"]
    assert any(not torch.equal(start[k], v) for k, v in model.named_parameters())
    slot = {id(p): (int(o), int(n)) for p, o, n in zip(layout["params"], layout["offsets"], layout["numel"])}
    combined = {k: flat[slot[id(p)][0]:slot[id(p)][0] + slot[id(p)][1]].clone() for k, p in model.named_parameters()}
    assert seen[0]["hitpts"].shape[0] == 2 and seen[0]["results"]["magnitude"].shape[0] == 1     # the last micro-batch's results
    single, losses = [], []
    for b in range(2):
        one = []
        args1, model1, opt1 = _fresh(setup, on_step=one.append)
        assert all(torch.equal(start[k], v) for k, v in model1.named_parameters())
        train.train(args1, model1, opt1, [{k: v[b:b + 1] for k, v in setup.batch.items()}])
        single.append({k: None if p.grad is None else p.grad.detach().clone() for k, p in model1.named_parameters()})
        losses.append(one[0]["losses"])
    bad = []
    for k, got in combined.items():
        g0, g1 = single[0][k], single[1][k]
        assert (g0 is None) == (g1 is None)
        want = torch.zeros_like(got) if g0 is None else (g0 * 0.5 + g1 * 0.5).reshape(-1)
        if not torch.equal(_bits(got), _bits(want)):
            bad.append(k)
    assert not bad, (len(bad), bad[:5])
    for key, v in seen[0]["losses"].items():
        want = (losses[0][key] + losses[1][key]) / 2
        print(key, v, want, abs(v - want) / want)
        assert abs(v - want) <= 2.0 ** -22 * want, key


def test_guards_act_on_the_combined_step(setup):
    """A NaN in micro-batch 1's target vectors only: the whole step changes nothing.  A clean step goes first so that moments and step counts exist to
    be compared, and one follows to show the optimizer goes on."""
    from etch_amd import train
    args, model, opt = _fresh(setup, accumulate=2)
    train.train(args, model, opt, [setup.batch])

    def snapshot():
        out = {k: v.detach().clone() for k, v in model.named_parameters()}
        for k, p in model.named_parameters():
            for name in ("exp_avg", "exp_avg_sq", "step"):
                if name in opt.state.get(p, {}):                 # a parameter no loss reaches has no state
                    out[k + "/" + name] = opt.state[p][name].detach().clone()
        return out
    before = snapshot()
    batch = dict(setup.batch)
    batch["vectors"] = batch["vectors"].clone()
    batch["vectors"][1, 17, 2] = float("nan")
    train.train(args, model, opt, [batch])
    after = snapshot()
    assert all(torch.equal(_bits(before[k]), _bits(after[k])) for k in before)
    rep = opt.report()
    assert rep["skipped_steps"] == 1 and rep["tensors_zeroed"] == 0
    train.train(args, model, opt, [setup.batch])
    moved = snapshot()
    assert any(not torch.equal(before[k], moved[k]) for k, _ in model.named_parameters())
    steps = [float(v) for k, v in moved.items() if k.endswith("/step")]
    assert len(steps) > 100 and all(v == 2.0 for v in steps)
    assert opt.report()["skipped_steps"] == 1


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _program(argv, **extra_env):
    """python -m etch_amd.train as a child process of its own."""
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "ETCH_FORCE_DIST", "ETCH_DIST_BACKEND")}
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    env["MASTER_PORT"] = str(_free_port())
    env.update(extra_env)
    r = subprocess.run([sys.executable, "-m", "etch_amd.train", *argv], env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.returncode, r.stdout[-1500:], r.stderr[-3000:])
    return r


def _two_ranks(argv):
    """--gpus 2 from a plain interpreter on the one GPU: both ranks on device 0, the reduction through gloo."""
    return _program(["--gpus", "2", *argv], ETCH_ALL_RANKS_DEVICE0="1", ETCH_DIST_BACKEND="gloo")


def _load(path):
    return torch.load(path, map_location="cpu")


def _same(folder_a, folder_b, epoch, buffers):
    want = _load(os.path.join(folder_a, f"model_epochs_{epoch:08d}.pth"))
    got = _load(os.path.join(folder_b, f"model_epochs_{epoch:08d}.pth"))
    assert list(want) == list(got)
    keys = [k for k in want if buffers or not k.endswith(STAT_BUFFERS)]
    assert len(keys) > 100 and (buffers or len(keys) < len(want))
    bad = [k for k in keys if not torch.equal(want[k], got[k])]
    assert not bad, (epoch, len(bad), bad[:5])


def _losses(folder):
    with open(os.path.join(folder, "log_all", "train", "losses.json")) as fh:
        return json.load(fh)


@pytest.fixture(scope="module")
def accumulated(data):
    from etch_amd import train
    out = os.path.join(data.root, "accumulated")
    train.main(data.flags + ["--accumulate", "2", "--epochs", "2", "--output_root", out])
    return TD.folder(out)


def test_two_ranks_equal_two_micro_batches(data, accumulated):
    """Parameters are compared bit for bit; the BatchNorm buffers running_mean / running_var / num_batches_tracked are left out by name: a rank's
    running statistics see its own micro-batches only (rank 0's one per step here, the accumulating process's two), as DataParallel's replicas do,
    and no parameter depends on them in train() mode."""
    out = os.path.join(data.root, "two_ranks")
    r = _two_ranks(data.flags + ["--epochs", "2", "--output_root", out])
    assert "Flat gradient path: 2 contribution(s) per step, all-reduce backend gloo, world 2" in r.stdout
    assert "Running on 2 GPUs" in r.stdout and r.stdout.count("Epoch 0 start") == 1          # rank 0 alone prints
    for epoch in (0, 1):
        _same(accumulated, TD.folder(out), epoch, buffers=False)
    assert _losses(TD.folder(out)) == _losses(accumulated)
    assert os.listdir(out) == [os.path.basename(TD.folder(out))]
    assert sorted(os.listdir(TD.folder(out))) == ["EPN_model_setting_json", "log_all", "model_epochs_00000000.pth", "model_epochs_00000001.pth", "train_state_00000000.pth",
                                                  "train_state_00000001.pth", "training_args.json"]
    assert os.listdir(os.path.join(TD.folder(out), "log_all", "train")) == ["losses.json"]


def test_two_ranks_equal_two_micro_batches_with_aug(data):
    from etch_amd import train
    out_a, out_b = os.path.join(data.root, "aug_accumulated"), os.path.join(data.root, "aug_two_ranks")
    train.main(data.flags + ["--aug", "true", "--accumulate", "2", "--epochs", "1", "--output_root", out_a])
    _two_ranks(data.flags + ["--aug", "true", "--epochs", "1", "--output_root", out_b])
    _same(TD.folder(out_a), TD.folder(out_b), 0, buffers=False)
    assert _losses(TD.folder(out_a)) == _losses(TD.folder(out_b))


def test_forced_world_size_1_rccl_group_equals_the_plain_run(data):
    """ETCH_FORCE_DIST=1: pack, an RCCL all-reduce over one rank, unpack and Adam from the flat buffer, against the plain step from .grad -- every
    tensor of the checkpoint, the statistics too (one micro-batch per step in both)."""
    from etch_amd import train
    out_a, out_b = os.path.join(data.root, "plain"), os.path.join(data.root, "forced")
    train.main(data.flags + ["--epochs", "1", "--output_root", out_a])
    r = _program(data.flags + ["--gpus", "1", "--accumulate", "1", "--epochs", "1", "--output_root", out_b], ETCH_FORCE_DIST="1")
    assert "Flat gradient path: 1 contribution(s) per step, all-reduce backend nccl, world 1" in r.stdout       # the forced group and the flat path ran
    _same(TD.folder(out_a), TD.folder(out_b), 0, buffers=True)
    assert _losses(TD.folder(out_a)) == _losses(TD.folder(out_b))


def test_resume_across_modes(data, accumulated):
    """The state --accumulate 2 wrote after epoch 0, resumed with --gpus 2, gives that run's epoch-1 parameters."""
    out = os.path.join(data.root, "resumed")
    _two_ranks(data.flags + ["--epochs", "2", "--output_root", out, "--resume", os.path.join(accumulated, "train_state_00000000.pth")])
    _same(accumulated, TD.folder(out), 1, buffers=False)
    assert not os.path.exists(os.path.join(TD.folder(out), "model_epochs_00000000.pth"))
    assert _losses(TD.folder(out)) == _losses(accumulated)
