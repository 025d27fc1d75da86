"""Engine vs the float64 oracle at trained-regime parameters (tests/_regimes.py).  GPU only.

Every other one-shot parity test runs at layout.init_flat: all biases exactly 0, no
degenerate first-layer unit.  The cases here are the explicit table _regimes.CASES, each
held by the CPU suite to the kink guard and the logit range (tests/test_param_regimes.py):

  A  general path, every variant, three shapes, three regimes
  B  fused path, model_2 / model_4, split and one-block, three shapes ((1,120,100) runs
     pair_tile32), three regimes
  C  sorted / tiled / sorted-group hunk forms at two shapes that cross both tile edges
  D  the entity-edge gam-only LDS table (Ne = 401)
  E  one TF-Adam step from the regime's parameters (loss_para now includes biases)
  F  the XCD block map with both of its branches in one grid (B = 11, 19)

Tolerances are the suite's own, unchanged: test_general_gpu._run_and_check (logits
2e-5 |ref| + 2e-6 max, gradients 8e-5 |ref| + 8e-6 max|ref| per variable, CE rel 1e-5) for
every case; the fused-path cases are held to test_gpu_parity's numbers as well (logits
1.5e-5 / 1.5e-6, gradients 1.5e-4 / 3e-6); stats rel 1e-5 and weights atol 2e-6 after the
Adam step.
"""
import numpy as np
import pytest
import torch

from hdgnn import _lib, layout
from hdgnn.synth import synth_commits
from oracle import model_ref
from tests import _errlog
from tests import _regimes as R
from tests import test_general_gpu as G
from tests import test_gpu_parity as FP

pytestmark = pytest.mark.gpu

PATHS = {"general": _lib.PATH_GENERAL, "fused": _lib.PATH_FUSED}
FORMS = {None: 0, "sorted": _lib.FLAG_HUNK_SORTED, "tiled": _lib.FLAG_HUNK_TILED,
         "sorted_group": _lib.FLAG_HUNK_SORTED | _lib.FLAG_HUNK_GROUP}


def _group(g):
    cs = [c for c in R.CASES if c.group == g]
    return pytest.mark.parametrize("case", cs, ids=[R.case_id(c) for c in cs])


def _inputs(c):
    cb = synth_commits(c.B, c.ne, c.nc, c.dseed)
    return cb, R.regime_flat(c.regime, c.pseed, c.variant, data=cb)


def _run(c):
    cb, flat = _inputs(c)
    eng = G._run_and_check(cb, c.variant, c.pseed, PATHS[c.path], FORMS[c.form], flat=flat)
    assert eng.path == PATHS[c.path]
    return eng, cb, flat


@pytest.fixture
def split_env(request, monkeypatch):
    """HDG_FUSED_SPLIT of the case ("1" two blocks per commit, "0" one), set before the
    engine is built."""
    split = request.node.callspec.params["case"].split
    monkeypatch.setenv("HDG_FUSED_SPLIT", split)
    return split


@_group("A")
def test_general_path(case):
    _run(case)


def _fused_grad_close(g_eng, g_ref, v):
    bad = []
    for name, (o, shape) in layout.offsets(v).items():
        n = int(np.prod(shape))
        a, r = g_eng[o:o + n], g_ref[o:o + n]
        scale = max(np.abs(r).max(), 1e-12)
        tol = R.FUS_GRAD[0] * np.abs(r) + R.FUS_GRAD[1] * scale + 1e-9
        err = np.abs(a - r)
        _errlog.record("grad_fused_tol:" + name, err.max() / scale, (err / tol).max())
        if not np.all(err <= tol):
            bad.append("%s: max err %.3g, scale %.3g" % (name, np.nanmax(err), scale))
    assert not bad, "gradient mismatch (fused tolerances):\n  " + "\n  ".join(bad)


@_group("B")
def test_fused_path(case, split_env):
    """_run_and_check's checks, then the same launch against test_gpu_parity's tolerances
    (its _check_outputs also compares the probabilities with the oracle's)."""
    eng, cb, flat = _run(case)
    eng.fwd_bwd(eng.upload(cb))
    torch.cuda.synchronize()
    eng.check_status()
    out, g_ref = G._oracle(flat, cb, case.variant)
    FP._check_outputs(eng.logits.cpu().numpy(), eng.probs.cpu().numpy(), out)
    g = eng.grad.cpu().numpy().astype(np.float64)[:len(flat)]
    _fused_grad_close(g + G._reg_grad(flat), g_ref, case.variant)


@_group("C")
def test_hunk_forms(case):
    _run(case)


@_group("D")
def test_ee_gamma_table(case):
    _run(case)


@_group("E")
def test_one_adam_step(case):
    """stats[0..3] rel 1e-5 and the weights after one TF-Adam step atol 2e-6, as
    test_model4_train_steps_match_oracle_adam checks them from the initialiser.

    The weights are float32 variables (in TF as in the engine).  A saturated first-layer bias
    reaches |b| = 3.3e4 in these cases, where neighbouring float32 values lie 3.9e-3 apart and
    the whole Adam step (3e-4) is below half of that: no float32 result can meet an absolute
    2e-6 there (the first GPU run read 1.9e-4 and 3.0e-4 on exactly those biases, 3.4e-8 of
    their size).  So an element's bound is 2e-6 or, where that is larger, one float32 spacing
    at the oracle's value; below |w| = 16, that is for every weight of the other two regimes
    and every saturated one but those biases, it is the 2e-6 of the suite unchanged."""
    c = case
    cb, flat = _inputs(c)
    eng = G._engine(c.B, c.ne, c.nc, c.variant, PATHS[c.path])
    assert eng.path == PATHS[c.path]
    eng.set_params(flat)
    eng.train_step(eng.upload(cb))
    torch.cuda.synchronize()
    out, g_ref = G._oracle(flat, cb, c.variant)
    stats = eng.stats.cpu().numpy()
    for i, k in enumerate(("ce", "loss_map", "loss_para", "total")):
        _errlog.record("stats:" + k, abs(stats[i] / float(out[k]) - 1),
                       abs(stats[i] / float(out[k]) - 1) / 1e-5)
        np.testing.assert_allclose(stats[i], float(out[k]), rtol=1e-5, err_msg=k)
    theta = model_ref.AdamTF(len(flat)).step(flat.astype(np.float64), g_ref)
    err = np.abs(eng.get_params() - theta)
    tol = np.maximum(2e-6, np.spacing(np.abs(theta).astype(np.float32)).astype(np.float64))
    assert (tol[np.abs(theta) < 16] == 2e-6).all()
    _errlog.record("weights@1", err.max(), (err / tol).max())
    bad = np.nonzero(~(err <= tol))[0]
    assert bad.size == 0, "weights after the step: %d off, worst %.3g at %d (bound %.3g)" % (
        bad.size, err[bad].max(), bad[err[bad].argmax()], tol[bad[err[bad].argmax()]])


@_group("F")
def test_block_map_both_branches(case):
    """xcd_commit_map (csrc/wide.hip) deals commits [0, B & ~7) across the XCDs and takes the
    last B % 8 in id order.  B = 11: commits 0-7 in the first branch, 8-10 in the second;
    B = 19: commits 0-15 in the first, 16-18 in the second.  The logits check is per commit
    (its scale is the commit's own max |logit|) and every commit's data differ, so a commit
    mapped to the wrong blocks fails it."""
    assert 0 < (case.B & ~7) < case.B
    _run(case)
