"""The step kernel's row-local node chains (M1/M2 forward, M12 backward) and the row
reductions behind them (M13, dV1) vs the CPU oracle, at the node counts that sit on the edges
of their MFMA tiles.  GPU only, but for the CPU guard of the regime cases at the end.

In split mode a block owns K = ceil(Ne / 2) or floor(Ne / 2) nodes: K is the reduction
length of M13's tiles (16-step bodies with all operand reads in front, 4-steps, a K % 4 tail)
and decides which 16-row blocks of the chains are full, shared by masking or empty:

  Ne   2   1 | 1     K < 4: the tail alone
       7   4 | 3     one 4-step | the tail alone
       8   4 | 4     4-steps only;     16  8 | 8 (one block: a single full row block)
      17   9 | 8     nlo = 9: the row block is shared by both halves
      31  16 | 15    exactly one body | 4-steps and tail
      33  17 | 16    body and tail | exactly one body; nlo = 17
      34  17 | 17    nlo = 17
      40  20 | 20    body, 4-step (no tail)
      66  33 | 33    two bodies and the tail; nlo = 33

Nc = 9 and B = 9: the split grid has padding commits.  Ne 33 and 66 also run at the
"trained" and "degenerate" parameters of tests/_regimes.py: dead first-layer units (h == 0
exactly) are what the select in the chain's dq guards.  One model_4 hybrid case, one wide-form
case (Nc = 81) and a run-to-run bitwise check.  Both split modes; the tolerances are
test_gpu_parity's, unchanged.
"""
import functools

import numpy as np
import pytest
import torch

from hdgnn import _lib, layout
from hdgnn.synth import synth_commits
from oracle import model_ref
from tests import _regimes as R
from tests.test_cgrad_defer_gpu import _grad_close4, _oracle, _reg_grad4
from tests.test_gpu_parity import _grad_close, _reg_grad
from tests.test_param_regimes import CE_RTOL, GUARD_DRAWS, GUARD_FRACTION, check_well_conditioned

gpu = pytest.mark.gpu

B = 9
NES = (2, 7, 8, 16, 17, 31, 33, 34, 40, 66)
STEPS = 3
# (regime, Ne) -> (data seed, parameter seed); each pair is held to the kink guard, the logit
# range and the CE conditions by test_regime_cases_are_well_conditioned below.  A pair that
# fails moves to the next parameter seed, as _regimes.MOVED does; the seeds left behind stay
# in the comment.
REGIME_SEEDS = {
    ("trained", 33): (133, 2001),
    ("degenerate", 33): (133, 2011),
    # pseed 2002, 2003: CE halves per step (10.1 -> 5.8 -> 2.66), and float32 rounding of the
    # parameters alone moves the third step's CE by 5.4e-6 resp. 7.0e-6 of it
    ("trained", 66): (166, 2004),
    ("degenerate", 66): (166, 2012),
}


@pytest.fixture(params=["1", "0"], ids=["split", "one_block"])
def split_mode(request, monkeypatch):
    monkeypatch.setenv("HDG_FUSED_SPLIT", request.param)
    return request.param


def _inputs(ne, nc, v, regime):
    if regime is None:
        return synth_commits(B, ne, nc, 100 + ne), layout.init_flat(ne, v)
    dseed, pseed = REGIME_SEEDS[(regime, ne)]
    return synth_commits(B, ne, nc, dseed), R.regime_flat(regime, pseed, v)


@functools.lru_cache(maxsize=None)
def _case(ne, nc=9, v=2, regime=None):
    """(batch, initial parameters, oracle trajectory [(out, g_ref, theta after the step)]),
    computed once per case and shared by the tests and both split modes"""
    cb, flat = _inputs(ne, nc, v, regime)
    theta = flat.astype(np.float64)
    opt = model_ref.AdamTF(len(flat))
    traj = []
    for _ in range(STEPS):
        out, g_ref = _oracle(theta.astype(np.float32), cb, v)
        theta = opt.step(theta, g_ref)
        traj.append((out, g_ref, theta.copy()))
    return cb, flat, traj


def _engine(ne, nc, v):
    from hdgnn.engine import Engine
    eng = Engine(ne, nc, B, variant=v, path=_lib.PATH_FUSED)
    assert eng.path == _lib.PATH_FUSED
    return eng


def _check_gradients(ne, nc=9, v=2, regime=None):
    cb, flat, traj = _case(ne, nc, v, regime)
    out, g_ref, _ = traj[0]
    eng = _engine(ne, nc, v)
    eng.set_params(flat)
    eng.fwd_bwd(eng.upload(cb))
    torch.cuda.synchronize()
    eng.check_status()
    g = eng.grad.cpu().numpy().astype(np.float64)
    n = len(flat)
    if v == 2:
        _grad_close(g[:n] + _reg_grad(flat), g_ref)
    else:
        _grad_close4(g[:n] + _reg_grad4(flat), g_ref)
    np.testing.assert_allclose(g[n] / (B * nc * (nc - 1)), float(out["ce"]), rtol=1e-5)


def _check_adam(ne, nc=9, v=2, regime=None):
    cb, flat, traj = _case(ne, nc, v, regime)
    eng = _engine(ne, nc, v)
    eng.set_params(flat)
    db = eng.upload(cb)
    for out, _, theta in traj:
        eng.train_step(db)
        torch.cuda.synchronize()
        stats = eng.stats.cpu().numpy()
        for i, k in enumerate(("ce", "loss_map", "loss_para", "total")):
            np.testing.assert_allclose(stats[i], float(out[k]), rtol=1e-5)
        np.testing.assert_allclose(eng.get_params(), theta, rtol=0, atol=2e-6)


@gpu
@pytest.mark.parametrize("ne", NES)
def test_gradients_match_oracle(ne, split_mode):
    _check_gradients(ne)


@gpu
@pytest.mark.parametrize("ne", NES)
def test_adam_steps_match_oracle(ne, split_mode):
    _check_adam(ne)


@gpu
@pytest.mark.parametrize("regime,ne", sorted(REGIME_SEEDS))
def test_dead_units_match_oracle(regime, ne, split_mode):
    """first-layer units that are off for every node (degenerate: z == 0 exactly, -0.0
    weights): h == 0 there, dq is the selected 0.f, and M13 sums those columns"""
    _check_gradients(ne, regime=regime)
    _check_adam(ne, regime=regime)


@gpu
def test_model4_hybrid_matches_oracle(split_mode):
    _check_gradients(33, 17, 4)
    _check_adam(33, 17, 4)


@gpu
def test_wide_form_matches_oracle(split_mode):
    """Nc = 81: the wide form of the hunk stage around the same node chains"""
    _check_gradients(17, 81)
    _check_adam(17, 81)


@gpu
def test_deterministic_bitwise(split_mode):
    ne = 66
    cb, flat, _ = _case(ne)
    eng = _engine(ne, 9, 2)
    eng.set_params(flat)
    db = eng.upload(cb)
    eng.fwd_bwd(db)
    g1, p1 = eng.grad.clone(), eng.probs.clone()
    eng.fwd_bwd(db)
    assert torch.equal(g1, eng.grad) and torch.equal(p1, eng.probs)


@pytest.mark.parametrize("regime,ne", sorted(REGIME_SEEDS))
def test_regime_cases_are_well_conditioned(regime, ne):
    """CPU: the guards of test_param_regimes.test_table_entry_is_well_conditioned on the
    regime cases above (kink guard at half the fused tolerance, max |logit| <= 1e4, CE in
    float32 to half the GPU check's relative tolerance), and the CE condition of the later
    steps.  The engine's parameters are float32 variables, so after s steps they may differ
    from the float64 trajectory by s roundings, theta (1 +- s 2^-24); where CE falls by half
    per step that alone moves CE by more than the check's 1e-5, and the comparison would
    measure the rounding of the parameters, not a kernel.  The oracle's CE at the perturbed
    parameters (three sign draws) has to stay within half the tolerance."""
    cb, flat = _inputs(ne, 9, 2, regime)
    check_well_conditioned(flat, cb, 2, True)
    _, _, traj = _case(ne, 9, 2, regime)
    for s in range(1, STEPS):
        theta, ce = traj[s - 1][2], float(traj[s][0]["ce"])
        for draw in range(GUARD_DRAWS):
            sg = np.random.default_rng(7100 + draw).choice([-1.0, 1.0], len(theta))
            out, _ = _oracle(theta * (1 + s * 2.0 ** -24 * sg), cb, 2)
            dev = abs(float(out["ce"]) / ce - 1)
            print("step %d draw %d: CE moves by %.3g" % (s, draw, dev))
            assert dev <= GUARD_FRACTION * CE_RTOL
