"""Engine vs the float64 oracle under asymmetric hunk labels (tests/_labels.py).  GPU only.

Every other parity test draws its labels from synth_commits, whose y is symmetric: there a
transposed read of y (yT a copy of ybits, a swapped `z ? yT : ybits`, the label lists' sides,
the fused pair pass' row / column roles, row counts for column counts, the label of relation
(q, p) for that of (p, q)) leaves every output bit as it was.  The cases here are the explicit
table _labels.CASES; the CPU suite (tests/test_labels.py) holds each entry to the bite
condition -- y against y^T moves the oracle's logits and gradients by at least 50 x the
tolerances below -- and to the regimes table's guards.

  A  general path, every variant, six shapes from the ABI minimum 2 x 2 to one past a tile,
     init and trained parameters
  B  fused path, model_2 / model_4, split and one-block; nc > ne up to the fused limit
     (30 x 160), ne = nc = 2, pair_tile32 (120 x 100)
  C  dense / sorted / tiled / sorted-group hunk forms (the sorted forms walk the label lists)
  D  the trailer's correct-count and hdg_eval's confusion counts against the host's
  and on each path: diagonal bits set in the host grid change no output bit.

Tolerances are the suites' own, imported: test_general_gpu._run_and_check for every case,
test_gpu_parity._check_outputs and its gradient numbers as well for the fused path.
"""
import numpy as np
import pytest
import torch

from hdgnn import _lib, metrics
from hdgnn.data import CommitBatch, onehot_relations, pair_index
from tests import _labels as L
from tests import test_general_gpu as G
from tests import test_gpu_parity as FP
from tests.test_param_regimes_gpu import PATHS, _fused_grad_close, split_env  # noqa: F401

pytestmark = pytest.mark.gpu

FORMS = {None: 0, "dense": _lib.FLAG_HUNK_DENSE, "sorted": _lib.FLAG_HUNK_SORTED,
         "tiled": _lib.FLAG_HUNK_TILED,
         "sorted_group": _lib.FLAG_HUNK_SORTED | _lib.FLAG_HUNK_GROUP}


def _group(g):
    cs = [c for c in L.CASES if c.group == g]
    return pytest.mark.parametrize("case", cs, ids=[L.case_id(c) for c in cs])


def _run(c):
    """fwd_bwd, then forward, each against the oracle (logits, probs = softmax, CE, loss_E_HR,
    per-variable gradients), as every case of the general suite."""
    cb, flat = L.inputs(c)
    eng = G._run_and_check(cb, c.variant, c.pseed, PATHS[c.path], FORMS[c.form], flat=flat,
                           ref=L.reference(c))
    assert eng.path == PATHS[c.path]
    return eng, cb, flat


@_group("A")
def test_general_path(case):
    _run(case)


@_group("B")
def test_fused_path(case, split_env):
    """_run_and_check's checks, then the same launch against test_gpu_parity's tolerances
    (its _check_outputs also compares the probabilities with the oracle's)."""
    eng, cb, flat = _run(case)
    eng.fwd_bwd(eng.upload(cb))
    torch.cuda.synchronize()
    eng.check_status()
    out, g_ref = L.reference(case)
    FP._check_outputs(eng.logits.cpu().numpy(), eng.probs.cpu().numpy(), out)
    g = eng.grad.cpu().numpy().astype(np.float64)[:len(flat)]
    _fused_grad_close(g + G._reg_grad(flat), g_ref, case.variant)


@_group("C")
def test_hunk_forms(case):
    _run(case)


@_group("D")
def test_counts(case):
    """HDG_TR_COUNT of the gradient trailer == the host count of argmax(probs) == y[:, I, J]
    on the engine's own probabilities (np.argmax: a tie picks class 0); hdg_eval on the same
    probabilities gives that count as TP + TN, and the host's four confusion slots."""
    c = case
    cb, flat = L.inputs(c)
    eng = G._engine(c.B, c.ne, c.nc, c.variant, PATHS[c.path])
    assert eng.path == PATHS[c.path]
    eng.set_params(flat)
    db = eng.upload(cb)
    eng.fwd_bwd(db)
    torch.cuda.synchronize()
    eng.check_status()
    probs = eng.probs.cpu().numpy()
    I, J = pair_index(c.nc)
    lab = cb.y[:, I, J]
    want = int((np.argmax(probs, axis=1) == lab).sum())
    assert _lib.trailer_count(eng.grad.cpu().numpy()[eng.np:]) == want
    ev = eng.evaluate(db).cpu().numpy()
    host = metrics.eval_counts(onehot_relations(cb.y), probs)
    four = [_lib.EV_TP, _lib.EV_FP, _lib.EV_FN, _lib.EV_TN]
    np.testing.assert_array_equal(ev[:, four], host[:, four])
    assert int(ev[:, [_lib.EV_TP, _lib.EV_TN]].sum()) == want
    assert (ev[:, four].sum(1) == c.nc * (c.nc - 1)).all()


@pytest.mark.parametrize("path", ["general", "fused"])
def test_diagonal_bits_are_cleared(path):
    """hdg_batch.ybits is 'diag 0': a host grid with y_pp = 1 packs to the same bit rows and
    prepared tables, and the step's outputs are the same bits."""
    c = next(c for c in L.CASES if c.group == "D" and c.path == path and c.variant == 4)
    cb, flat = L.inputs(c)
    yd = cb.y.copy()
    idx = np.arange(c.nc)
    yd[:, idx, idx] = 1
    eng = G._engine(c.B, c.ne, c.nc, c.variant, PATHS[path])
    eng.set_params(flat)
    got = []
    for y in (cb.y, yd):
        db = eng.upload(CommitBatch(cb.x, cb.a, y, cb.hid, cb.nlen))
        eng.grad.zero_()
        eng.fwd_bwd(db)
        torch.cuda.synchronize()
        got.append((db.ybits.clone(), db.prep.clone(), eng.grad.clone(), eng.probs.clone(),
                    eng.logits.clone()))
    for a, b in zip(*got):
        assert torch.equal(a, b)
    assert got[0][2][:eng.np].abs().max() > 0
