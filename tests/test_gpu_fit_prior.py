"""The LM fit kernel's warm start (x_init) and diagonal Gaussian prior against the committed oracle, unmodified
(tests/_fit_prior_oracle.py builds the augmented residual that oracle.stage2.lm minimises), on SyntheticSMPL(7) / SyntheticSMPLX(7) with the
default marker set: default equivalence, parity for both instantiations, the stage-0-free schedule, the split fit, a scan without markers,
and the argument checks."""
import pytest
import torch

import _fit_prior_oracle as O

pytestmark = pytest.mark.gpu


def _db(bm, mv):
    from etch_amd.models.fit_SMPL import _device_body
    return _device_body(bm, mv, torch.device("cuda"))


def _noisy(x_gt, seed, model="smpl"):
    """init = generating parameters + seeded noise; mu = another noisy copy; w mixed: positive on the pose, zero on some DoFs (a block of the
    pose, the global orientation), large on the betas."""
    g = torch.Generator().manual_seed(seed)
    B, dof = x_gt.shape
    npose, nb = (69, 10) if model == "smpl" else (162, 20)
    init = x_gt + torch.randn(B, dof, generator=g) * 0.03
    mu = x_gt + torch.randn(B, dof, generator=g) * 0.03
    w = torch.zeros(B, dof)
    w[:, :npose] = 0.1 + 0.2 * torch.rand(B, npose, generator=g)
    w[:, 9:21] = 0.0
    w[:, npose:npose + nb] = 50.0
    w[:, npose + nb + 3:] = 2.0
    return init.contiguous(), mu.contiguous(), w.contiguous()


def _run(db, tgt, valid, it0, it1, init=None, prior=None, **kw):
    from etch_amd import ops
    c = lambda t: None if t is None else t.cuda().contiguous()
    return ops.smpl_lm_fit(db.lm_consts, c(tgt), c(valid.float()), it0, 0.5, 0.01, it1, 0.2, 1e-3, True, nj=db.nj, nb=db.nb, x_init=c(init),
                           prior=None if prior is None else (c(prior[0]), c(prior[1])), **kw)


@pytest.fixture(scope="module")
def smpl():
    bm, ms, mv, tgt, valid, x_gt = O.problem(3)
    assert valid.sum(1).tolist() == [85, 86, 82]                 # one scan misses 1 marker, one misses 4
    return bm, mv, tgt, valid, x_gt, _db(bm, mv)


def test_zero_init_and_zero_prior_equal_the_default_fit_bitwise(smpl):
    """smpl_lm_fit(...) against smpl_lm_fit(..., x_init=zeros, prior=(zeros, zeros)) on the full 30 + 50 schedule: x, x_stage0 and the trace
    are equal under == (a -0 may become +0, nothing else)."""
    bm, mv, tgt, valid, x_gt, db = smpl
    z = torch.zeros(3, 85)
    x, x0, tr = _run(db, tgt, valid, 30, 50)
    xp, x0p, trp = _run(db, tgt, valid, 30, 50, init=z, prior=(z, z))
    assert torch.isfinite(x).all() and tr.shape == (3, 82)
    assert bool((xp == x).all()) and bool((x0p == x0).all()) and bool((trp == tr).all())


def test_init_and_prior_vs_oracle(smpl):
    bm, mv, tgt, valid, x_gt, db = smpl
    init, mu, w = _noisy(x_gt, 31)
    assert (w == 0).any() and (w > 10).any()
    x, x0, tr = _run(db, tgt, valid, 5, 10, init=init, prior=(mu, w))
    ref = O.fit(bm, mv, tgt, valid, 5, 10, init=init, prior=(mu, w))
    O.assert_fit_parity(x, x0, tr, ref, lambda: O.fit(bm, mv, tgt, valid, 5, 10, init=init, prior=(mu, w), dtype=torch.float64))
    # stage 0 leaves its inactive betas where x_init put them
    assert torch.equal(x0[:, 71:79].cpu(), init[:, 71:79])
    # and the prior did something: the same fit without it lands elsewhere
    xn, _, _ = _run(db, tgt, valid, 5, 10, init=init)
    assert float((xn - x).abs().max()) > 1e-3


def test_no_stage0_starts_stage1_at_init(smpl):
    """it0 = 0: x_stage0 is x_init bitwise, the trace has it1 + 2 entries, stage 1 is the oracle's from `init`."""
    bm, mv, tgt, valid, x_gt, db = smpl
    init, mu, w = _noisy(x_gt, 32)
    x, x0, tr = _run(db, tgt, valid, 0, 10, init=init, prior=(mu, w))
    assert torch.equal(x0.cpu(), init)
    assert tr.shape == (3, 12)
    ref = O.fit(bm, mv, tgt, valid, 0, 10, init=init, prior=(mu, w))
    O.assert_fit_parity(x, x0, tr, ref, lambda: O.fit(bm, mv, tgt, valid, 0, 10, init=init, prior=(mu, w), dtype=torch.float64))


def test_188_dof_model_vs_oracle():
    bm, ms, mv, tgt, valid, x_gt = O.problem(2, seed=2, model="smplx")
    db = _db(bm, mv)
    init, mu, w = _noisy(x_gt, 33, "smplx")
    x, x0, tr = _run(db, tgt, valid, 2, 3, init=init, prior=(mu, w))
    assert x.shape == (2, 188) and tr.shape == (2, 7)
    ref = O.fit(bm, mv, tgt, valid, 2, 3, init=init, prior=(mu, w))
    O.assert_fit_parity(x, x0, tr, ref, lambda: O.fit(bm, mv, tgt, valid, 2, 3, init=init, prior=(mu, w), dtype=torch.float64),
                        groups=O.DOF_GROUPS_X, npose=162)
    assert torch.equal(x0[:, 164:182].cpu(), init[:, 164:182])


def test_split_fit_with_init_and_prior_matches_one_workgroup_per_scan(smpl):
    """split = 3 against split = 1 (the bars of the existing split test: trace <= 1e-6 of its maximum, parameters < 2e-6); the prior is added
    after the exchange by every workgroup in the same order, so two runs at split = 3 are bitwise equal."""
    bm, mv, tgt, valid, x_gt, db = smpl
    init, mu, w = _noisy(x_gt, 34)
    tgt, valid, init, mu, w = tgt[:2], valid[:2], init[:2].contiguous(), mu[:2].contiguous(), w[:2].contiguous()
    x1, x01, tr1 = _run(db, tgt, valid, 5, 10, init=init, prior=(mu, w), split=1)
    x3, x03, tr3 = _run(db, tgt, valid, 5, 10, init=init, prior=(mu, w), split=3)
    assert torch.isfinite(x3).all()
    assert float((tr3 - tr1).abs().max()) <= 1e-6 * float(tr1.max())
    assert float((x3 - x1).abs().max()) < 2e-6 and float((x03 - x01).abs().max()) < 2e-6
    x3b, x03b, tr3b = _run(db, tgt, valid, 5, 10, init=init, prior=(mu, w), split=3)
    assert torch.equal(x3b, x3) and torch.equal(x03b, x03) and torch.equal(tr3b, tr3)


def test_scan_without_markers_is_held_by_its_prior(smpl):
    """A scan with no valid marker and w > 0 everywhere (its neighbour in the batch is an ordinary scan): started at mu it stays at mu, bit
    for bit; started elsewhere (it0 = 0) it follows the oracle's run of the prior-only objective."""
    bm, mv, tgt, valid, x_gt, db = smpl
    tgt, valid = tgt[:2], valid[:2].clone()
    valid[0] = False
    g = torch.Generator().manual_seed(35)
    mu = (x_gt[:2] + torch.randn(2, 85, generator=g) * 0.03).contiguous()
    w = (0.5 + torch.rand(2, 85, generator=g)).contiguous()
    x, x0, tr = _run(db, tgt, valid, 3, 3, init=mu, prior=(mu, w))
    assert torch.isfinite(x).all() and torch.equal(x[0].cpu(), mu[0]) and torch.equal(x0[0].cpu(), mu[0])
    assert float(tr[0].abs().max()) == 0.0
    init = (mu + torch.randn(2, 85, generator=g) * 0.05).contiguous()
    x, x0, tr = _run(db, tgt, valid, 0, 10, init=init, prior=(mu, w))
    ref = O.fit(bm, mv, tgt, valid, 0, 10, init=init, prior=(mu, w))
    O.assert_fit_parity(x, x0, tr, ref, lambda: O.fit(bm, mv, tgt, valid, 0, 10, init=init, prior=(mu, w), dtype=torch.float64))
    assert float((x[0].cpu() - mu[0]).abs().max()) < float((init[0] - mu[0]).abs().max())       # it moved towards mu


def test_argument_errors_raise_before_any_launch(smpl, monkeypatch):
    from etch_amd import _lib, ops
    bm, mv, tgt, valid, x_gt, db = smpl
    init, mu, w = _noisy(x_gt, 36)
    mk, vf = tgt.cuda(), valid.float().cuda()
    init, mu, w = init.cuda(), mu.cuda(), w.cuda()
    neg = w.clone()
    neg[1, 4] = -1e-3
    nan = w.clone()
    nan[0, 0] = float("nan")
    strided = torch.zeros(3, 170, device="cuda")[:, ::2]
    torch.cuda.synchronize()
    monkeypatch.setattr(_lib, "lib", lambda: pytest.fail("the library was reached"))
    for kw in (dict(prior=(mu, neg)), dict(prior=(mu, nan)), dict(prior=(mu, None)), dict(prior=(None, w)), dict(prior=(mu[:, :84].contiguous(), w)),
               dict(prior=(mu, w[:2])), dict(x_init=init[:2]), dict(x_init=init.double()), dict(prior=(mu, strided)), dict(x_init=init.cpu()),
               dict(prior=mu)):
        with pytest.raises(_lib.EtchHipError):
            ops.smpl_lm_fit(db.lm_consts, mk, vf, 2, 0.5, 0.01, 2, 0.2, 1e-3, nj=db.nj, nb=db.nb, **kw)
