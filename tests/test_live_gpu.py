"""Engine vs the float64 oracle off the initialiser with a live entity stage, up to the
benchmark shapes (tests/_live.py).  GPU only.

At `trained` parameters mlp2_entity_B1 often leaves x' = 0 on every node; then no gradient
reaches the entity stage and no entity bias moves a logit, and the engine passes the check of
its entity backward by multiplying with rho = 0 (_live.KNOWN_DEAD lists those entries of the
earlier tables).  At layout.init_flat, where the larger shapes ran so far, every bias is 0, so
a term proportional to a bias -- 2 (Ne - 1) b5, c0 = W1[2] + b1, the classifier offsets -- or a
padded node or hunk row that leaks relu(b) is multiplied by zero.  The cases here are the
explicit table _live.CASES at the `live` regime: biases nonzero, x' > 0, every variable with a
data gradient >= 1e-3 and every entity bias visible in the logits (tests/test_live.py).

  A  fused path, model_2, split and one-block, B = 2, 28 shapes (Ne, Nc) at the step kernel's
     own edges: the split halves ceil(Ne / 2) at 16 | 17; the 16-row chain blocks up to all 16
     waves of the one-block mode at Ne >= 241; E1's 102-node pass edge, 102 | 103 in one-block
     mode and 204 | 205 in split mode; NE4 residues 0-3; the label words at Nc 32 | 33, 64 | 65,
     96 | 97, 128 | 129; smax_c 5 | 8 | 10 at 80 | 81 and 128 | 129 and with them gam_lds /
     defer_cgrad and pair_tile32; odd Nc, where the two blocks own different row counts; the
     benchmark shapes 200 x 74, 250 x 114, 250 x 150, 256 x 160.  Attributes alternate int10 /
     real; edensity 0.5 at (103, 64), (205, 81) and (256, 128), where the x-lists are read from
     the prepared buffer, not LDS.
  B  model_4 on the fused path: every third shape of A and the benchmark shapes
  C  general path, variants 1-4, four shapes; sorted and tiled hunk forms at 2 x 65 x 70
  D  `degenerate` on top of `live` at 200 x 74 and 256 x 160, fused, variants 2 and 4
  E  one TF-Adam step from `live` parameters at 2 x 200 x 74 and 1 x 256 x 160
  S  model_2 at the general path's stress shape 1 x 1024 x 512 (slow)

Tolerances are the suites' own, unchanged: test_general_gpu._run_and_check for every case
(fwd_bwd, the forward-only launch, CE, ehr), test_gpu_parity._check_outputs and its gradient
numbers as well for the fused path; stats rel 1e-5 and weights atol max(2e-6, one float32
spacing) after the Adam step.  The oracle runs once per entry and is shared by both block
modes.
"""
import numpy as np
import pytest
import torch

from oracle import model_ref
from tests import _errlog
from tests import _live as LV
from tests import test_general_gpu as G
from tests import test_gpu_parity as FP
from tests.test_labels_gpu import FORMS
from tests.test_param_regimes_gpu import PATHS, _fused_grad_close, split_env  # noqa: F401

pytestmark = pytest.mark.gpu


def _group(g):
    cs = [c for c in LV.CASES if c.group == g]
    return pytest.mark.parametrize("case", cs, ids=[LV.case_id(c) for c in cs])


def _run(c):
    cb, flat = LV.inputs(c)
    eng = G._run_and_check(cb, c.variant, c.pseed, PATHS[c.path], FORMS[c.form],
                           flat=flat.copy(), ref=LV.reference(c))
    assert eng.path == PATHS[c.path]
    eng.check_status()
    return eng, cb, flat


def _fused(case):
    """_run_and_check's checks, then the same launch against test_gpu_parity's tolerances (its
    _check_outputs also compares the probabilities with the oracle's)."""
    eng, cb, flat = _run(case)
    eng.fwd_bwd(eng.upload(cb))
    torch.cuda.synchronize()
    eng.check_status()
    out, g_ref = LV.reference(case)
    FP._check_outputs(eng.logits.cpu().numpy(), eng.probs.cpu().numpy(), out)
    g = eng.grad.cpu().numpy().astype(np.float64)[:len(flat)]
    _fused_grad_close(g + G._reg_grad(flat), g_ref, case.variant)


@_group("A")
def test_fused_lattice(case, split_env):
    _fused(case)


@_group("B")
def test_fused_model4(case, split_env):
    _fused(case)


@_group("C")
def test_general_path(case):
    _run(case)


@_group("D")
def test_fused_degenerate(case, split_env):
    _fused(case)


@_group("E")
def test_one_adam_step(case, monkeypatch):
    """stats[0..3] rel 1e-5 and the weights after one TF-Adam step: atol 2e-6 or, where that
    is larger, one float32 spacing at the oracle's value (test_param_regimes_gpu's bound)."""
    c = case
    if c.split is not None:
        monkeypatch.setenv("HDG_FUSED_SPLIT", c.split)
    cb, flat = LV.inputs(c)
    eng = G._engine(c.B, c.ne, c.nc, c.variant, PATHS[c.path])
    assert eng.path == PATHS[c.path]
    eng.set_params(flat.copy())
    eng.train_step(eng.upload(cb))
    torch.cuda.synchronize()
    eng.check_status()
    out, g_ref = LV.reference(c)
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


@pytest.mark.slow
@_group("S")
def test_stress_shape(case):
    _run(case)
