"""Engine vs the float64 oracle at exact relu ties (tests/_ties.py).  GPU only.

Every first layer decides which pairs are on by a strict z > 0, and no forward output can see
that rule: a tie adds 0 to a relu sum and u_i + w1 x_j = 0 to the count / prefix-sum form.
Only the backward counts and masks move.  The cases here are the explicit table _ties.CASES:
lattice parameters whose pre-activations are exact in fp32 and in float64 alike, with the
biases solved so that interior pairs tie beside pairs that are on and pairs that are off.  The
CPU suite (tests/test_ties.py) holds each entry to exactness, tie coverage, the bite (the
ties turned on move the layer's own gradient by >= 50 x the tolerances below), one-sidedness
and the regimes' guards.

  A  general path, every variant, three shapes, integer and half-integer attributes
  B  fused path, model_2 / model_4, split and one-block ((1, 120, 100) runs pair_tile32); the
     x-lists read from the prepared buffer (2 x 256 x 9, edensity 0.5); the wide form (nc = 81)
  C  dense / sorted / tiled / sorted-group hunk forms at two shapes that cross both tile edges
  D  the entity-edge gam-only LDS table (Ne = 401; integer attributes only, see _ties._table)
  E  one TF-Adam step from the lattice parameters
  F  every attribute equal (x = 3, x = 0: nd = 1), a whole a = 0 set tied beside a = 1 pairs on
  and two run-to-run bitwise checks (fused, sorted form).

Tolerances are the suites' own, unchanged: test_general_gpu._run_and_check for every case,
test_gpu_parity._check_outputs and its gradient numbers as well for the fused path; stats rel
1e-5 and weights atol max(2e-6, one float32 spacing) after the Adam step.  The lattice layers'
own variables are compared first and by name, so a failure says which tie rule broke.
"""
import numpy as np
import pytest
import torch

from hdgnn import layout
from oracle import model_ref
from tests import _errlog
from tests import _ties as T
from tests import test_general_gpu as G
from tests import test_gpu_parity as FP
from tests.test_labels_gpu import FORMS
from tests.test_param_regimes_gpu import PATHS, _fused_grad_close, split_env  # noqa: F401

pytestmark = pytest.mark.gpu


def _group(g):
    cs = [c for c in T.CASES if c.group == g]
    return pytest.mark.parametrize("case", cs, ids=[T.case_id(c) for c in cs])


def _lattice_first(g_eng, g_ref, c):
    """The lattice layers' own weight and bias gradients, by name, at the case's tolerance."""
    v, fused = c.variant, c.path == "fused"
    offs = layout.offsets(v)
    bad = []
    for layer in T.lattice_layers(v):
        ws, b = T.layer_vars(v, layer)
        for name in ws + (b,):
            o, shape = offs[name]
            n = int(np.prod(shape))
            err = np.abs(g_eng[o:o + n] - g_ref[o:o + n])
            tol = T.grad_tol(g_ref[o:o + n], fused)
            _errlog.record("tie:%s:%s" % (layer, name), err.max() / max(np.abs(g_ref[o:o + n]).max(),
                                                                        1e-12), (err / tol).max())
            if not np.all(err <= tol):
                units = sorted(set(np.nonzero(~(err <= tol).reshape(shape))[-1].tolist()))
                bad.append("%s %s: %.3g x tol, hidden units %s (lattice units %s)" % (
                    layer, name, (err / tol).max(), units, list(T.LU)))
    assert not bad, "tie rule (mask = [z > 0]) broken at an exact tie:\n  " + "\n  ".join(bad)


def _run(c):
    cb, flat = T.inputs(c)
    ref = T.reference(c)
    eng = G._engine(c.B, c.ne, c.nc, c.variant, PATHS[c.path], FORMS[c.form])
    assert eng.path == PATHS[c.path]
    eng.set_params(flat.copy())
    eng.fwd_bwd(eng.upload(cb))
    torch.cuda.synchronize()
    g = eng.grad.cpu().numpy().astype(np.float64)[:len(flat)] + G._reg_grad(flat)
    _lattice_first(g, ref[1], c)
    eng = G._run_and_check(cb, c.variant, c.pseed, PATHS[c.path], FORMS[c.form], flat=flat.copy(),
                           ref=ref)
    assert eng.path == PATHS[c.path]
    return eng, cb, flat


@_group("A")
def test_general_path(case):
    _run(case)


def _fused(case):
    eng, cb, flat = _run(case)
    eng.fwd_bwd(eng.upload(cb))
    torch.cuda.synchronize()
    eng.check_status()
    out, g_ref = T.reference(case)
    FP._check_outputs(eng.logits.cpu().numpy(), eng.probs.cpu().numpy(), out)
    g = eng.grad.cpu().numpy().astype(np.float64)[:len(flat)]
    _fused_grad_close(g + G._reg_grad(flat), g_ref, case.variant)


@_group("B")
def test_fused_path(case, split_env):
    """_run_and_check's checks, then the same launch against test_gpu_parity's tolerances."""
    _fused(case)


@_group("C")
def test_hunk_forms(case):
    _run(case)


@_group("D")
def test_ee_gamma_table(case):
    _run(case)


@_group("E")
def test_one_adam_step(case):
    """stats[0..3] rel 1e-5 and the weights after one TF-Adam step: atol 2e-6 or, where that
    is larger, one float32 spacing at the oracle's value (test_param_regimes_gpu's bound)."""
    c = case
    cb, flat = T.inputs(c)
    eng = G._engine(c.B, c.ne, c.nc, c.variant, PATHS[c.path])
    assert eng.path == PATHS[c.path]
    eng.set_params(flat.copy())
    eng.train_step(eng.upload(cb))
    torch.cuda.synchronize()
    out, g_ref = T.reference(c)
    stats = eng.stats.cpu().numpy()
    for i, k in enumerate(("ce", "loss_map", "loss_para", "total")):
        _errlog.record("stats:" + k, abs(stats[i] / float(out[k]) - 1),
                       abs(stats[i] / float(out[k]) - 1) / 1e-5)
        np.testing.assert_allclose(stats[i], float(out[k]), rtol=1e-5, err_msg=k)
    theta = model_ref.AdamTF(len(flat)).step(flat.astype(np.float64), g_ref)
    err = np.abs(eng.get_params() - theta)
    tol = np.maximum(2e-6, np.spacing(np.abs(theta).astype(np.float32)).astype(np.float64))
    _errlog.record("weights@1", err.max(), (err / tol).max())
    bad = np.nonzero(~(err <= tol))[0]
    assert bad.size == 0, "weights after the step: %d off, worst %.3g at %d (bound %.3g)" % (
        bad.size, err[bad].max(), bad[err[bad].argmax()], tol[bad[err[bad].argmax()]])


@_group("F")
def test_all_attributes_equal(case):
    """nd = 1: the set boundary of every E1 / EE unit is 0 or 1 of one distinct value, and the
    unit ties a whole class set"""
    if case.path == "fused":
        _fused(case)
    else:
        _run(case)


def _pick(**want):
    return next(c for c in T.CASES if all(getattr(c, k) == v for k, v in want.items()))


@pytest.mark.parametrize("case", [
    _pick(group="B", variant=4, ne=37, xkind="half", split="1"),
    _pick(group="C", variant=1, ne=37, xkind="half", form="sorted"),
], ids=T.case_id)
def test_deterministic_bitwise(case, monkeypatch):
    c = case
    if c.split is not None:
        monkeypatch.setenv("HDG_FUSED_SPLIT", c.split)
    cb, flat = T.inputs(c)
    eng = G._engine(c.B, c.ne, c.nc, c.variant, PATHS[c.path], FORMS[c.form])
    assert eng.path == PATHS[c.path]
    eng.set_params(flat.copy())
    db = eng.upload(cb)
    eng.fwd_bwd(db)
    g1, p1 = eng.grad.clone(), eng.probs.clone()
    eng.fwd_bwd(db)
    assert torch.equal(g1, eng.grad) and torch.equal(p1, eng.probs)
    assert g1[:eng.np].abs().max() > 0
