"""The asymmetric-label case table (tests/_labels.py) on the CPU: the generators' properties,
the table against the matrix it was written from, and every entry against its guards with
the float64 oracle alone.  No engine."""
import numpy as np
import pytest

from hdgnn import layout
from tests import _labels as L
from tests import _regimes as R
from tests import test_general_gpu as G
from tests import test_gpu_parity as FP
from tests.test_param_regimes import check_well_conditioned

BITE = 50.0     # y vs y^T moves the oracle by at least this many GPU tolerances


# ----------------------------------------------------------------------------
# generators
# ----------------------------------------------------------------------------
@pytest.mark.parametrize("kind", L.KINDS)
def test_label_kinds(kind):
    B, nc = 4, 61
    y = L.label_grid(kind, B, nc, 3)
    assert y.dtype == np.uint8 and y.shape == (B, nc, nc) and y.max() == 1
    assert not y[:, np.arange(nc), np.arange(nc)].any()
    off = ~np.eye(nc, dtype=bool)
    yt = y.transpose(0, 2, 1)
    if kind == "directed":
        assert 0.07 < y[:, off].mean() < 0.13
        assert ((y != yt).reshape(B, -1).sum(1) > nc).all()
    elif kind == "upper":
        assert not np.tril(y).any() and 0.15 < y[:, np.triu(off)].mean() < 0.25
        rows, cols = y.sum(2), y.sum(1)
        assert (rows[:, -1] == 0).all() and (cols[:, 0] == 0).all()
        assert (rows != cols).any(1).all()
    else:
        assert ((y + yt)[:, off] == 1).all()              # exactly one of y_pq, y_qp
        assert y[:, off].mean() == 0.5
    assert np.array_equal(y, L.label_grid(kind, B, nc, 3))
    assert not np.array_equal(y, L.label_grid(kind, B, nc, 4))


def test_commits_keep_the_synthetic_rest():
    from hdgnn.synth import synth_commits
    cb, ref = L.commits("upper", 3, 7, 5, 107, 9), synth_commits(3, 7, 5, 107)
    for k in ("x", "a", "hid", "nlen"):
        assert np.array_equal(getattr(cb, k), getattr(ref, k))
    assert np.array_equal(ref.y, ref.y.transpose(0, 2, 1))           # what the table replaces
    assert np.array_equal(cb.y, L.label_grid("upper", 3, 5, 9))
    cb.validate()


def test_tolerances_are_the_suites():
    assert R.GEN_GRAD == (G.GRAD_RTOL, G.GRAD_ATOL)
    assert R.FUS_GRAD == FP._grad_close.__defaults__
    ref = np.random.default_rng(0).standard_normal((2, 2, 20)) * 50
    assert np.array_equal(L.logit_tol(ref, False),
                          G.LOGIT_RTOL * np.abs(ref) + G.LOGIT_ATOL * np.abs(ref).reshape(2, -1)
                          .max(1)[:, None, None])
    assert np.array_equal(L.logit_tol(ref, True), FP._logit_tol(ref))    # the smaller of the two


# ----------------------------------------------------------------------------
# case table
# ----------------------------------------------------------------------------
def test_case_table_is_the_issue_matrix():
    n = {}
    for c in L.CASES:
        n[c.group] = n.get(c.group, 0) + 1
    # A: 4 variants x (6 directed + 2 x 2 upper / tournament) x 2 parameter sets
    # B: 2 variants x 2 block modes x (6 directed + 1 upper) x 2;  C: 2 shapes x 2 variants x
    # 4 forms x 2 kinds;  D: 2 paths x 2 variants
    assert n == {"A": 80, "B": 56, "C": 32, "D": 4}
    assert len({L.case_id(c) for c in L.CASES}) == len(L.CASES)
    for c in L.CASES:
        assert c.path == {"A": "general", "B": "fused", "C": "general"}.get(c.group, c.path)
        assert (c.split in ("1", "0")) if c.group == "B" else c.split is None
        if c.path == "fused":
            assert c.variant in (2, 4) and c.ne <= 256 and c.nc <= 160
        if c.group == "C":
            assert c.param == "trained" and c.form in L.C_FORMS
    fused_shapes = {(c.ne, c.nc) for c in L.CASES if c.group == "B"}
    assert (2, 2) in fused_shapes                                   # the ABI minimum
    assert any(nc > ne and nc == 160 for ne, nc in fused_shapes)    # nc > ne at the fused limit
    keys = {(c.kind, c.param, c.variant, c.B, c.ne, c.nc) for c in L.CASES}
    assert set(L.MOVED) <= keys
    assert set(L.LABEL_SEED) <= {(c.kind, c.B, c.ne, c.nc) for c in L.CASES}


def _flat_tol(g0, v, fused):
    tol = np.empty_like(g0)
    for name, (o, shape) in layout.offsets(v).items():
        n = int(np.prod(shape))
        tol[o:o + n] = L.grad_tol(g0[o:o + n], fused)
    return tol


@pytest.mark.parametrize("entry", L.oracle_entries(), ids=L.entry_id)
def test_table_entry_guards(entry):
    """Asymmetry: every commit has a bit with y_pq != y_qp.  Bite: the oracle on y and on y^T
    differ by at least 50 x the entry's GPU logit tolerance at the worst logit and by at least
    50 x the gradient tolerance on the worst variable -- a condition on the inputs: a kernel
    that reads y transposed somewhere cannot hide inside the tolerance.  Then the regimes
    table's three guards, unchanged (test_param_regimes.check_well_conditioned: kink guard 0.5
    of the tolerance under the 2e-7 perturbation, max |logit| <= 1e4, the float32 oracle's CE
    to 5e-6 relative).  An entry that fails moves to the next seed in _labels.MOVED; none is
    waived."""
    e = entry
    cb, flat = L.inputs(e)
    asym = (cb.y != cb.y.transpose(0, 2, 1)).reshape(e.B, -1).sum(1)
    assert (asym > 0).all(), asym
    out, g0 = check_well_conditioned(flat, cb, e.variant, e.fused)
    outT, gT = G._oracle(flat, L.transposed(cb), e.variant)
    lref = out["logits"].transpose(0, 2, 1)
    lbite = (np.abs(outT["logits"].transpose(0, 2, 1) - lref) / L.logit_tol(lref, e.fused)).max()
    gbite = (np.abs(gT - g0) / _flat_tol(g0, e.variant, e.fused)).max()
    print("bite: logits %.3g x tol, gradient %.3g x tol; CE %.4g" % (lbite, gbite,
                                                                      float(out["ce"])))
    assert lbite >= BITE and gbite >= BITE


@pytest.mark.parametrize("case", [c for c in L.CASES if c.group == "D" and c.path == "general"],
                         ids=L.case_id)
def test_count_cases_tell_the_orientation(case):
    """Group D: on the oracle's probabilities the correct-count against y[:, I, J] differs from
    the count against y[:, J, I], and the four confusion slots differ too -- a count that took
    the label of (q, p) for that of (p, q) cannot give the right number by accident.  (With
    every prediction class 0 the two counts would be equal: both are the number of 0 labels.)"""
    from hdgnn import metrics
    from hdgnn.data import onehot_relations, pair_index
    cb, _ = L.inputs(case)
    probs = L.reference(case)[0]["probs"].transpose(0, 2, 1)
    I, J = pair_index(case.nc)
    pred = np.argmax(probs, axis=1)
    assert 0 < pred.sum() < pred.size
    assert int((pred == cb.y[:, I, J]).sum()) != int((pred == cb.y[:, J, I]).sum())
    ev = metrics.eval_counts(onehot_relations(cb.y), probs)
    evT = metrics.eval_counts(onehot_relations(cb.y.transpose(0, 2, 1)), probs)
    assert (ev[:, :4] != evT[:, :4]).any(1).all()
