"""Parameter regimes off the initialiser, on the CPU: the oracle itself is pinned there
(pair-explicit vs literal restatement, every variant), the regime generator's properties,
and every entry of the GPU case table (tests/_regimes.py) against the kink guard and the
logit range.  Float64 oracle only; no engine."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from hdgnn import layout
from hdgnn.synth import synth_commits
from oracle import layout as olayout
from oracle import literal, model_ref
from tests import _regimes as R
from tests.test_oracle import _rand_case

STATES = ("init",) + R.REGIMES


def _params(state, seed, v, case):
    if state == "init":
        return model_ref.init_params(seed, v)
    x, a, y, hid, nlen = case
    data = SimpleNamespace(x=x, a=a, y=y, hid=hid, nlen=nlen)
    return model_ref.unflatten(R.regime_flat(state, seed, v, data=data), v)


def _pair_explicit_vs_literal(state, seed, v):
    case = _rand_case(seed)
    x, a, y, hid, nlen = case
    params = _params(state, seed, v, case)
    B, ne = x.shape
    nc = y.shape[1]
    P1 = model_ref.to_torch_params(params)
    out1 = model_ref.forward(P1, x, a, y, hid, nlen, variant=v)
    out1["total"].backward()
    P2 = model_ref.to_torch_params(params)
    D = literal.build_dense(x, a, y, hid, nlen, dtype=torch.float64)
    out2 = literal.forward(P2, D, B, ne, nc, variant=v)
    out2["total"].backward()
    np.testing.assert_allclose(out1["logits"].detach().numpy(),
                               out2["logits"].transpose(1, 2).detach().numpy(),
                               rtol=1e-12, atol=1e-12)
    for k in ("ce", "loss_map", "loss_para", "total"):
        np.testing.assert_allclose(float(out1[k]), float(out2[k]), rtol=1e-12)
    assert set(P1) == {k for k, _, _ in olayout.keyed_specs(v)}
    for k in P1:
        np.testing.assert_allclose(P1[k].grad.numpy(), P2[k].grad.numpy(),
                                   rtol=1e-10, atol=1e-12)


@pytest.mark.parametrize("seed", [0, 1, 2])
@pytest.mark.parametrize("regime", R.REGIMES)
def test_pair_explicit_equals_literal_at_regimes(regime, seed):
    """model_2 off the init point (the committed check in test_oracle.py is at init only)."""
    _pair_explicit_vs_literal(regime, seed, 2)


@pytest.mark.parametrize("seed", [0, 1, 2])
@pytest.mark.parametrize("state", STATES)
@pytest.mark.parametrize("v", [1, 3, 4])
def test_pair_explicit_equals_literal_other_variants(v, state, seed):
    """model_1 / model_3 / model_4: the oracle against the dense op sequence of that
    variant's build_model, at the initialiser and at the three regimes."""
    _pair_explicit_vs_literal(state, seed, v)


def test_literal_default_is_model2():
    """bench.py's CPU baseline calls literal.forward without a variant."""
    x, a, y, hid, nlen = _rand_case(0)
    P = model_ref.to_torch_params(model_ref.init_params(0), requires_grad=False)
    D = literal.build_dense(x, a, y, hid, nlen, dtype=torch.float64)
    o1 = literal.forward(P, D, 3, 7, 5)
    o2 = literal.forward(P, D, 3, 7, 5, variant=2)
    assert torch.equal(o1["logits"], o2["logits"]) and float(o1["total"]) == float(o2["total"])


# ----------------------------------------------------------------------------
# generator properties
# ----------------------------------------------------------------------------
@pytest.mark.parametrize("v", [1, 2, 3, 4])
def test_trained_has_no_zero(v):
    flat = R.regime_flat("trained", 5, v)
    assert flat.dtype == np.float32 and flat.shape == (layout.n_params(v),)
    assert (flat != 0).all()
    for name, view in R.views(flat, v).items():
        if name.split("/")[-1].split(":")[0] in layout.BIASES:
            assert (view != 0).all(), name
    assert 0.05 < flat.std() < 0.15


@pytest.mark.parametrize("v", [1, 2, 3, 4])
def test_degenerate_features_are_bit_exact(v):
    flat = R.regime_flat("degenerate", 5, v)
    base = R.regime_flat("trained", 5, v)
    V, U = R.views(flat, v), R.UNITS
    have = R.first_layers(v)
    assert set(have) == {1: {"H1", "H2"}, 2: {"E1", "E3", "H1", "H2"},
                         3: {"EE", "EC", "H1", "H2"},
                         4: {"E1", "E3", "EE", "EC", "H1", "H2"}}[v]
    touched = np.zeros(len(flat), bool)
    for key, (w, b) in have.items():
        if key == "EE":
            w11, w12, bias = V[w[0]], V[w[1]], V[b]
            for u in ("xj_zero", "xi_zero", "all_zero"):
                assert w11[0, U[u]] == 0 and not np.signbit(w11[0, U[u]])
            assert (w12[:, U["all_zero"]] == 0).all() and bias[U["all_zero"]] == 0
            assert w12[0, U["cls_equal"]] == w12[1, U["cls_equal"]] != 0
            assert w12[0, U["cls_tiny"]] == 0 and w12[1, U["cls_tiny"]] == np.float32(1e-33)
            assert w11[0, U["xj_negzero"]] == 0 and np.signbit(w11[0, U["xj_negzero"]])
            continue
        L, W, bias = R.LAYERS[key], V[w], V[b]
        assert (W[L.xj, U["xj_zero"]] == 0).all()
        assert (W[sorted(set(L.xi) - set(L.xj)), U["xj_zero"]] != 0).all()
        assert (W[L.xi, U["xi_zero"]] == 0).all()
        assert (W[:, U["all_zero"]] == 0).all() and bias[U["all_zero"]] == 0
        if L.cls is not None:
            assert W[L.cls[0], U["cls_equal"]] == W[L.cls[1], U["cls_equal"]] != 0
            assert W[L.cls[0], U["cls_tiny"]] == 0
            assert 0 < W[L.cls[1], U["cls_tiny"]] == np.float32(1e-33) < 2.0 ** -100
        assert (W[L.xj, U["xj_negzero"]] == 0).all() and np.signbit(W[L.xj, U["xj_negzero"]]).all()
    # nothing but the named units of the first layers moved, and only those hold zeros
    changed = flat.view(np.uint32) != base.view(np.uint32)
    for key, (w, b) in have.items():
        for name in (w if isinstance(w, tuple) else (w,)) + (b,):
            o, shape = layout.offsets(v)[name]
            m = np.zeros(shape, bool)
            m[..., sorted(U.values())] = True
            touched[o:o + m.size] = m.reshape(-1)
    assert not (changed & ~touched).any()
    assert (flat[~touched] != 0).all()
    # theta (1 +- eps) keeps every exact zero and the sign of -0.0 (the kink guard's step)
    pert = flat.astype(np.float64) * (1 + 2e-7)
    assert ((pert == 0) == (flat == 0)).all()
    assert (np.signbit(pert) == np.signbit(flat)).all()


def _saturated_entries():
    return [e for e in R.oracle_entries() if e[0] == "saturated"]


@pytest.mark.parametrize("entry", _saturated_entries(), ids=lambda e: "v%d-%dx%dx%d" % e[1:5])
def test_saturated_units_are_all_on_or_all_off(entry):
    """Even units on for every pair (node), odd units off for every one, in every first layer
    of the variant, at the table's own batch; every other parameter is the trained one."""
    reg, v, B, ne, nc, dseed, pseed, _ = entry
    cb = synth_commits(B, ne, nc, dseed)
    flat = R.regime_flat(reg, pseed, v, data=cb)
    trace = {}
    P = model_ref.to_torch_params(model_ref.unflatten(flat.astype(np.float64), v),
                                  requires_grad=False)
    model_ref.forward(P, cb.x.astype(np.float64), cb.a, cb.y, cb.hid, cb.nlen, v, trace=trace)
    have = R.first_layers(v)
    assert set(trace) == set(have)
    base = R.regime_flat("trained", pseed, v)
    same = np.ones(len(flat), bool)
    for key, (_, b) in have.items():
        z = trace[key].reshape(-1, 20).numpy()
        zmax = np.abs(z).max()
        assert (z[:, 0::2] > 0.04 * zmax).all(), key      # on, and far from the kink
        assert (z[:, 1::2] < -0.04 * zmax).all(), key
        o, shape = layout.offsets(v)[b]
        same[o:o + 20] = False
        bias = flat[o:o + 20]
        assert (bias[0::2] > 0).all() and (bias[1::2] == -bias[0]).all()
    assert np.array_equal(flat[same], base[same])


# ----------------------------------------------------------------------------
# case table
# ----------------------------------------------------------------------------
def test_case_table_is_the_issue_matrix():
    n = {}
    for c in R.CASES:
        n[c.group] = n.get(c.group, 0) + 1
    assert n == {"A": 36, "B": 36, "C": 36, "D": 2, "E": 18, "F": 4}
    assert len({R.case_id(c) for c in R.CASES}) == len(R.CASES)
    for c in R.CASES:
        if c.group in ("C", "D"):
            assert c.regime in ("trained", "degenerate")
        if c.group == "F":   # both branches of the block map in one grid
            assert c.B >= 8 and c.B % 8 != 0
    assert set(R.MOVED) <= {(c.regime, c.variant, c.B, c.ne, c.nc) for c in R.CASES}


def _oracle_grad(flat, cb, v):
    params = model_ref.unflatten(np.asarray(flat, np.float64), v)
    out, g = model_ref.loss_and_grads(params, cb.x.astype(np.float64), cb.a, cb.y, cb.hid,
                                      cb.nlen, variant=v)
    return out, np.concatenate([g[k].reshape(-1) for k, _, _ in olayout.keyed_specs(v)])


GUARD_EPS, GUARD_DRAWS, GUARD_FRACTION, LOGIT_MAX = 2e-7, 3, 0.5, 1e4
CE_RTOL = 1e-5          # the GPU cases' relative CE tolerance


def check_well_conditioned(flat, cb, v, fused):
    """The three guards of test_table_entry_is_well_conditioned on one (parameters, batch);
    -> the float64 oracle's (out, flat gradient).  tests/test_labels.py applies them to its
    own table."""
    out, g0 = _oracle_grad(flat, cb, v)
    assert np.isfinite(g0).all()
    assert np.abs(out["logits"]).max() <= LOGIT_MAX
    P32 = model_ref.to_torch_params(model_ref.unflatten(flat, v), torch.float32, False)
    ce32 = float(model_ref.forward(P32, cb.x, cb.a, cb.y, cb.hid, cb.nlen, v, torch.float32)["ce"])
    assert abs(ce32 - float(out["ce"])) <= GUARD_FRACTION * CE_RTOL * float(out["ce"])
    worst = 0.0
    for draw in range(GUARD_DRAWS):
        s = np.random.default_rng(7000 + draw).choice([-1.0, 1.0], len(flat))
        _, g1 = _oracle_grad(flat.astype(np.float64) * (1 + GUARD_EPS * s), cb, v)
        for name, (o, shape) in layout.offsets(v).items():
            n = int(np.prod(shape))
            frac = (np.abs(g1[o:o + n] - g0[o:o + n]) / R.grad_tol(g0[o:o + n], fused)).max()
            worst = max(worst, frac)
            assert frac <= GUARD_FRACTION, "%s: %.3g of the tolerance" % (name, frac)
    print("guard %.3g of tol, max|logit| %.4g" % (worst, np.abs(out["logits"]).max()))
    return out, g0


@pytest.mark.parametrize("entry", R.oracle_entries(),
                         ids=lambda e: "%s-v%d-%dx%dx%d" % e[:5])
def test_table_entry_is_well_conditioned(entry):
    """Kink guard: the oracle's own gradient at theta and at theta (1 + 2e-7 s), three sign
    draws s, differ by at most half the tolerance the entry's GPU cases are held to -- a relu
    crossing within fp32 rounding of the parameters moves it by more than the whole tolerance,
    and then a mismatch says nothing about a kernel.  Logit range: max |logit| <= 1e4, the
    range the tolerances were set for.  CE condition: the oracle run in float32 gives the
    float64 CE to half the relative tolerance of the GPU check -- when the labels are
    separated completely CE falls to 1e-4 or to 0 and a relative check of it in fp32 measures
    nothing.  An entry that fails moves to the next seed in _regimes.MOVED; it is never
    waived."""
    reg, v, B, ne, nc, dseed, pseed, fused = entry
    cb = synth_commits(B, ne, nc, dseed)
    flat = R.regime_flat(reg, pseed, v, data=cb)
    check_well_conditioned(flat, cb, v, fused)
