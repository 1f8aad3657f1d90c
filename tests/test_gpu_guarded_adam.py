"""etch_amd.optim.GuardedAdam (csrc/train_step.hip: etch_guarded_adam_step) against the reference's guard loop (train.py:119-125) written out
literally in front of torch.optim.Adam(foreach=False), and against an fp64 numpy Adam fed the same fp32 inputs.

Bounds (derived, not tuned): at lr = 1e-4 the update's own error is orders below an ulp of p, so a parameter is within 1 ulp (np.spacing) of the fp64
result -- only the final rounding can differ; a moment is b m + (1 - b) g after three roundings: within 4 ulp of the larger addend.  NaN patterns and
step counts are identical to torch's."""
import copy

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SIZES = (1, 3, 63, 64, 65, 1000, 70001)
MISALIGNED = 5          # SIZES[5]: a contiguous view of a non-contiguous origin whose first element is only 4-byte aligned
LR, B1, B2, EPS = 1e-4, 0.9, 0.999, 1e-8
f32 = np.float32


def make_params(seed=0):
    rng = np.random.default_rng(seed)
    ps = []
    for k, n in enumerate(SIZES):
        # |p| in [0.25, 2): the premise of the 1-ulp bound (an update of ~lr carries an error of ~1e-11, orders below ulp(p) >= 3e-8)
        v = torch.from_numpy((rng.uniform(0.25, 2.0, n) * rng.choice([-1.0, 1.0], n)).astype(f32)).cuda()
        if k == MISALIGNED:
            origin = torch.zeros((4, n + 1), device="cuda").t()            # (n+1, 4), strides (1, n+1): not contiguous
            view = origin[1:, 2]                                           # contiguous, storage offset 2 (n+1) + 1
            assert view.is_contiguous() and not origin.is_contiguous() and view.data_ptr() % 16 != 0 and view.data_ptr() % 4 == 0
            view.copy_(v)
            v = view
        ps.append(torch.nn.Parameter(v))
    return ps


def make_grads(seed=1):
    """Three steps of gradients: [step][tensor] -> fp32 array or None."""
    rng = np.random.default_rng(seed)
    gs = [[rng.standard_normal(n).astype(f32) * f32(10.0 ** rng.integers(-3, 2)) for n in SIZES] for _ in range(3)]
    gs[0][4][7] = np.nan                        # size 65: a NaN on steps 1 and 3
    gs[2][4][64] = np.nan
    gs[1][5][3], gs[1][5][900] = np.inf, -np.inf    # the misaligned 1000: +inf and -inf on step 2
    gs[0][3][10] = np.inf                       # size 64: +inf only (not flagged, as in the reference)
    gs[1][6] = None                             # size 70001: no gradient on step 2 only
    gs[2][6][69000] = np.nan                    # ... and a NaN in its last chunk on step 3 (every chunk of the tensor must see it)
    gs[2][2][5], gs[2][2][6] = -np.inf, -np.inf     # size 63: -inf only
    return gs


def set_grads(ps, gs):
    for p, g in zip(ps, gs):
        p.grad = None if g is None else torch.from_numpy(g).cuda()


def guard_loop(ps):
    """train.py:119-123."""
    for param in ps:
        if param.grad is None:
            pass
        elif param.grad.sum().isnan():
            param.grad = torch.zeros_like(param.grad)


def state_of(opt, p):
    st = opt.state.get(p, {})
    if "exp_avg" not in st:
        return None
    return st["exp_avg"].detach().cpu().numpy().copy(), st["exp_avg_sq"].detach().cpu().numpy().copy(), float(st["step"])


def adam64(p, g, m, v, step):
    """One fp64 Adam step (step = the count after this step) from fp32 inputs; returns p, m, v and the larger addend of each moment."""
    p, g, m, v = (x.astype(np.float64) for x in (p, g, m, v))
    with np.errstate(all="ignore"):
        a1, a2 = np.maximum(np.abs(B1 * m), np.abs((1 - B1) * g)), np.maximum(B2 * v, (1 - B2) * g * g)
        m = B1 * m + (1 - B1) * g
        v = B2 * v + (1 - B2) * g * g
        p = p - LR / (1 - B1 ** step) * m / (np.sqrt(v) / np.sqrt(1 - B2 ** step) + EPS)
    return p, m, v, a1, a2


def guarded(g):
    """The guard's definition: a NaN, or infinities of both signs -> a zero gradient."""
    if np.isnan(g).any() or (np.isposinf(g).any() and np.isneginf(g).any()):
        return np.zeros_like(g)
    return g


def check_step_against_fp64(before, after, g, tag):
    """before / after: (p, m, v, step) fp32 snapshots around one step with gradient g (None: the tensor must be untouched)."""
    p0, m0, v0, s0 = before
    p1, m1, v1, s1 = after
    if g is None:
        assert np.array_equal(p0, p1, equal_nan=True) and np.array_equal(m0, m1, equal_nan=True) and np.array_equal(v0, v1, equal_nan=True) and s0 == s1, tag
        return
    assert s1 == s0 + 1, tag
    p, m, v, a1, a2 = adam64(p0, guarded(g), m0, v0, s1)
    with np.errstate(all="ignore"):
        ok = np.isfinite(p) & np.isfinite(m) & np.isfinite(v) & (np.abs(g.astype(np.float64)) < 1e18)      # g^2 stays inside fp32
        dp = np.abs(p1.astype(np.float64) - p)[ok]
        dm = np.abs(m1.astype(np.float64) - m)[ok]
        dv = np.abs(v1.astype(np.float64) - v)[ok]
        up = np.spacing(np.abs(p).astype(f32)).astype(np.float64)[ok]
        um = 4 * np.spacing(a1.astype(f32)).astype(np.float64)[ok]
        uv = 4 * np.spacing(a2.astype(f32)).astype(np.float64)[ok]
    print(tag, "max error in bounds: p", float((dp / up).max(initial=0)), "m", float((dm / um).max(initial=0)), "v", float((dv / uv).max(initial=0)))
    assert np.all(dp <= up), (tag, float((dp / up).max()))
    assert np.all(dm <= um), (tag, float((dm / um).max()))
    assert np.all(dv <= uv), (tag, float((dv / uv).max()))


def snapshot(opt, ps):
    out = []
    for p in ps:
        st = state_of(opt, p)
        n = p.numel()
        out.append((p.detach().cpu().numpy().copy(),) + (st if st is not None else (np.zeros(n, f32), np.zeros(n, f32), 0.0)))
    return out


def test_three_guarded_steps_against_the_literal_loop_and_fp64():
    from etch_amd.optim import GuardedAdam
    ps, qs = make_params(), make_params()
    opt, ref = GuardedAdam(ps, lr=LR, betas=(B1, B2), eps=EPS), torch.optim.Adam(qs, lr=LR, betas=(B1, B2), eps=EPS, foreach=False)
    gs = make_grads()
    zeroed = 0
    for s in range(3):
        before = snapshot(opt, ps)
        set_grads(ps, gs[s])
        set_grads(qs, gs[s])
        opt.step()
        guard_loop(qs)
        ref.step()
        after = snapshot(opt, ps)
        for k in range(len(SIZES)):
            check_step_against_fp64(before[k], after[k], gs[s][k], f"step {s + 1} size {SIZES[k]}")
            # torch on the same device, its own trajectory from the same start: the same NaN pattern and step counts
            tp, tst = qs[k].detach().cpu().numpy(), state_of(ref, qs[k])
            assert np.array_equal(np.isnan(after[k][0]), np.isnan(tp)), (s, k)
            if tst is None:
                assert state_of(opt, ps[k]) is None
            else:
                assert np.array_equal(np.isnan(after[k][1]), np.isnan(tst[0])) and np.array_equal(np.isnan(after[k][2]), np.isnan(tst[1])), (s, k)
                assert after[k][3] == tst[2], (s, k)
            if gs[s][k] is not None and guarded(gs[s][k]) is not gs[s][k]:
                zeroed += 1
    assert np.isnan(ps[3].detach().cpu().numpy()[10]) and np.isfinite(ps[4].detach().cpu().numpy()).all()      # +inf only reaches p; a NaN does not
    rep = opt.report()
    assert rep["tensors_zeroed"] == zeroed == 4 and rep["skipped_steps"] == 0 and not rep["bad_label"]


def test_nan_loss_status_word_makes_the_step_a_no_op():
    from etch_amd import ops
    from etch_amd.optim import GuardedAdam
    ps = make_params()
    opt = GuardedAdam(ps, lr=LR)
    gs = make_grads(5)
    set_grads(ps, [g if g is None else np.nan_to_num(g, nan=0.0, posinf=0.0, neginf=0.0) for g in gs[0]])
    opt.step()
    before = snapshot(opt, ps)
    opt.status.fill_(ops.TRAIN_STATUS_NAN)
    opt.step()
    after = snapshot(opt, ps)
    for b, a in zip(before, after):
        assert all(np.array_equal(x, y) for x, y in zip(b[:3], a[:3])) and b[3] == a[3] == 1.0
    assert opt.report()["skipped_steps"] == 1
    opt.status.zero_()
    opt.step()
    assert all(s[3] == 2.0 for s in snapshot(opt, ps)) and opt.report()["skipped_steps"] == 1


def test_state_dict_round_trip_with_torch_adam():
    from etch_amd.optim import GuardedAdam
    ps, qs = make_params(), make_params()
    opt = GuardedAdam(ps, lr=LR)
    gs = make_grads(7)
    clean = [[np.nan_to_num(g, nan=0.0, posinf=0.0, neginf=0.0) for g in step] for step in (gs[0], gs[2])]
    for g in clean:
        set_grads(ps, g)
        opt.step()
    sd = opt.state_dict()
    assert set(sd["param_groups"][0]) == set(torch.optim.Adam([torch.nn.Parameter(torch.zeros(1))]).state_dict()["param_groups"][0])
    assert all(set(st) == {"step", "exp_avg", "exp_avg_sq"} and st["step"].device.type == "cpu" and float(st["step"]) == 2.0 for st in sd["state"].values())
    with torch.no_grad():
        for p, q in zip(ps, qs):
            q.copy_(p)
    ref = torch.optim.Adam(qs, lr=LR, foreach=False)
    ref.load_state_dict(copy.deepcopy(sd))          # load_state_dict keeps the tensors it is given: without the copy both optimizers would own one state
    g3 = [g * f32(0.5) for g in clean[0]]
    b_opt, b_ref = snapshot(opt, ps), snapshot(ref, qs)
    set_grads(ps, g3), set_grads(qs, g3)
    opt.step(), ref.step()
    a_opt, a_ref = snapshot(opt, ps), snapshot(ref, qs)
    for k in range(len(SIZES)):
        assert all(np.array_equal(x, y) for x, y in zip(b_opt[k][:3], b_ref[k][:3])) and b_opt[k][3] == b_ref[k][3] == 2.0
        check_step_against_fp64(b_opt[k], a_opt[k], g3[k], f"ours after save, size {SIZES[k]}")
        check_step_against_fp64(b_ref[k], a_ref[k], g3[k], f"torch after load, size {SIZES[k]}")
    # and back: torch's state into a fresh GuardedAdam over parameters equal to torch's
    rs = make_params()
    with torch.no_grad():
        for r, q in zip(rs, qs):
            r.copy_(q)
    back = GuardedAdam(rs, lr=LR)
    back.load_state_dict(copy.deepcopy(ref.state_dict()))
    b_back = snapshot(back, rs)
    for k in range(len(SIZES)):
        assert all(np.array_equal(x, y) for x, y in zip(b_back[k][:3], a_ref[k][:3])) and b_back[k][3] == 3.0
    g4 = [g * f32(-2.0) for g in clean[1]]
    set_grads(rs, g4), set_grads(qs, g4)
    back.step(), ref.step()
    a_back, a_ref2 = snapshot(back, rs), snapshot(ref, qs)
    for k in range(len(SIZES)):
        check_step_against_fp64(b_back[k], a_back[k], g4[k], f"ours after load, size {SIZES[k]}")
        check_step_against_fp64(a_ref[k], a_ref2[k], g4[k], f"torch, size {SIZES[k]}")
        assert a_back[k][3] == a_ref2[k][3] == 4.0


def test_unsupported_options_raise():
    from etch_amd.optim import GuardedAdam
    p = [torch.nn.Parameter(torch.zeros(3, device="cuda"))]
    for kw in (dict(weight_decay=0.1), dict(amsgrad=True), dict(maximize=True)):
        with pytest.raises(ValueError):
            GuardedAdam(p, **kw)
