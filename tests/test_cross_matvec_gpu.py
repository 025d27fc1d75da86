"""The step kernel's cross-graph matvecs (M3: n = [ks x', kt x'] forward, M11: dx' = ks^T dn0 +
kt^T dn1 backward) vs the CPU oracle, at the hunk and node counts that sit on the edges of
their load schedules.  GPU only, but for the CPU guard of the cases at the end.

M11 walks a hunk range per thread group (8 ranges of cq = ceil(Nc / 8) hunks in split mode,
4 of ceil(Nc / 4) in the one-block form) in chunks of 10 hunks whose loads are all issued
before the first product; hunks past a range's end are clamped and dropped by select:

  Nc (Ne = 33)   7   cq = 1: fewer hunks than ranges, one range empty
                 9   cq = 2: one range of a single hunk, three empty
                17   cq = 3: the last non-empty range is short, two are empty
                80   cq = 10: exactly one full chunk
                81   the wide form, two chunks
               160   cq = 20, and the one-block form's 40

M3 reads a node range in lane groups of 64 (a half of the nodes in split mode):

  Ne (Nc = 9)    2   1 | 1          3   2 | 1
                65   33 | 32        129  65 | 64      a lane group boundary
               255, 256             four lane groups exactly full; a half of 128 nodes is the
                                    whole width of an M11 range

B = 9: the split grid has padding commits.  synth_commits draws n < Ne for about half the
commits and 20 % null hid, so short node lists and empty hunks are in every case.  One model_4
hybrid case (the entity-edge aggregate in M3, dn's class parts beside M11's exchange), two
forward-only cases (hdg_forward runs the same M3) and a run-to-run bitwise check.  Both split
modes; the tolerances are test_gpu_parity's, unchanged.
"""
import functools

import numpy as np
import pytest
import torch

from hdgnn import _lib, layout
from hdgnn.synth import synth_commits
from oracle import model_ref
from tests.test_cgrad_defer_gpu import _grad_close4, _oracle, _reg_grad4
from tests.test_gpu_parity import _check_outputs, _grad_close, _reg_grad
from tests.test_param_regimes import CE_RTOL, GUARD_DRAWS, GUARD_FRACTION

gpu = pytest.mark.gpu

B = 9
NCS = (7, 9, 17, 80, 81, 160)       # at Ne = 33
NES = (2, 3, 65, 129, 255, 256)     # at Nc = 9
STEPS = 3
# (Ne, Nc) -> seed offset of the cases that left offset 0: the first multiple of 1000 at which
# the float64 oracle's own three-step trajectory meets test_cases_are_well_conditioned below
# (CE falls in every step; rounding the parameters to float32 moves CE by at most a quarter
# of the GPU check's 1e-5).  What offset 0 gives for them: 33 x 9 CE 0.3916, 0.3831, 0.3866
# and 129 x 9 CE 3.83, 2.41, 5.85 (Adam overshoots in the third step); 65 x 17 CE 1.18, 0.73,
# 0.91 and the rounding moves it by 5.1e-6; 256 x 9 CE 381, 249, 134 and 2.8e-6.  The third
# step's CE of 129 x 9 and 256 x 9 is then off by 3.5e-5 and 1.1e-5 on the GPU in both block
# forms alike, and with the library of the commit before this file as with the one after it.
MOVED = {(33, 9): 2000, (129, 9): 1000, (256, 9): 1000, (65, 17): 1000}
CASES = ([(33, nc, 2) for nc in NCS] + [(ne, 9, 2) for ne in NES] +
         [(33, 17, 4), (66, 17, 2), (65, 17, 2)])


@pytest.fixture(params=["1", "0"], ids=["split", "one_block"])
def split_mode(request, monkeypatch):
    monkeypatch.setenv("HDG_FUSED_SPLIT", request.param)
    return request.param


@functools.lru_cache(maxsize=None)
def _case(ne, nc, v=2):
    """(batch, initial parameters, oracle trajectory [(out, g_ref, theta after the step)]),
    computed once per case and shared by the tests and both split modes"""
    k = MOVED.get((ne, nc), 0)
    cb, flat = synth_commits(B, ne, nc, 300 + ne + nc + k), layout.init_flat(ne + nc + k, v)
    theta = flat.astype(np.float64)
    opt = model_ref.AdamTF(len(flat))
    traj = []
    for _ in range(STEPS):
        out, g_ref = _oracle(theta.astype(np.float32), cb, v)
        theta = opt.step(theta, g_ref)
        traj.append((out, g_ref, theta.copy()))
    return cb, flat, traj


def _engine(ne, nc, v=2):
    from hdgnn.engine import Engine
    eng = Engine(ne, nc, B, variant=v, path=_lib.PATH_FUSED)
    assert eng.path == _lib.PATH_FUSED
    return eng


def _check_gradients(ne, nc, v=2):
    cb, flat, traj = _case(ne, nc, v)
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


def _check_adam(ne, nc, v=2):
    cb, flat, traj = _case(ne, nc, v)
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
@pytest.mark.parametrize("nc", NCS)
def test_hunk_counts_match_oracle(nc, split_mode):
    _check_gradients(33, nc)
    _check_adam(33, nc)


@gpu
@pytest.mark.parametrize("ne", NES)
def test_node_counts_match_oracle(ne, split_mode):
    _check_gradients(ne, 9)
    _check_adam(ne, 9)


@gpu
def test_model4_hybrid_matches_oracle(split_mode):
    _check_gradients(33, 17, 4)
    _check_adam(33, 17, 4)


@gpu
@pytest.mark.parametrize("ne,nc", [(33, 9), (66, 17)])
def test_forward_only_matches_oracle(ne, nc, monkeypatch):
    """Engine.forward in split mode: probs and logits of the forward-only launch"""
    monkeypatch.setenv("HDG_FUSED_SPLIT", "1")
    cb, flat, traj = _case(ne, nc)
    out = traj[0][0]
    eng = _engine(ne, nc)
    eng.set_params(flat)
    probs, logits, ce_sum = eng.forward(eng.upload(cb))
    torch.cuda.synchronize()
    eng.check_status()
    _check_outputs(logits.cpu().numpy(), probs.cpu().numpy(), out)
    np.testing.assert_allclose(ce_sum.item() / (B * nc * (nc - 1)), float(out["ce"]), rtol=1e-5)


@gpu
def test_deterministic_bitwise(split_mode):
    """the step twice from the same state: gradients, probs and parameters bit for bit"""
    ne, nc = 65, 17
    cb, flat, _ = _case(ne, nc)
    res = []
    for _ in range(2):                       # a fresh engine each: the same Adam state
        eng = _engine(ne, nc)
        eng.set_params(flat)
        db = eng.upload(cb)
        eng.fwd_bwd(db)
        g, p = eng.grad.clone(), eng.probs.clone()
        eng.train_step(db)
        torch.cuda.synchronize()
        eng.check_status()
        res.append((g, p, eng.params.clone()))
    for a, b in zip(*res):
        assert torch.equal(a, b)


@pytest.mark.parametrize("ne,nc,v", CASES)
def test_cases_are_well_conditioned(ne, nc, v):
    """CPU: the CE condition of tests/test_node_chain_gpu.py on every case above, at half its
    bound.  After s steps the engine's float32 parameters may differ from the float64
    trajectory by s roundings; the oracle's CE at parameters perturbed that much (three sign
    draws) has to stay within a quarter of the GPU check's tolerance, and CE has to fall from
    step to step: where Adam overshoots, CE is far more sensitive to the parameters than the
    rounding draws show."""
    cb, _, traj = _case(ne, nc, v)
    ces = [float(out["ce"]) for out, _, _ in traj]
    assert all(b < a for a, b in zip(ces, ces[1:])), ces
    for s in range(1, STEPS):
        theta = traj[s - 1][2]
        for draw in range(GUARD_DRAWS):
            sg = np.random.default_rng(7100 + draw).choice([-1.0, 1.0], len(theta))
            out, _ = _oracle(theta * (1 + s * 2.0 ** -24 * sg), cb, v)
            dev = abs(float(out["ce"]) / ces[s] - 1)
            print("step %d draw %d: CE moves by %.3g" % (s, draw, dev))
            assert dev <= 0.5 * GUARD_FRACTION * CE_RTOL
