"""The exact-tie case table (tests/_ties.py) on the CPU: the generator's properties, the table
against the matrix it was written from, and every distinct oracle input against exactness, tie
coverage, bite, one-sidedness and the regimes' guards, with the oracle alone.  No engine."""
import numpy as np
import pytest
import torch

from hdgnn import layout
from oracle import layout as olayout
from oracle import model_ref
from tests import _regimes as R
from tests import _ties as T
from tests.test_param_regimes import (CE_RTOL, GUARD_DRAWS, GUARD_EPS, GUARD_FRACTION,
                                      LOGIT_MAX)

BITE = 50.0          # the asymmetric-labels table's bite factor
EPS = 2.0 ** -40     # bias shift that turns the ties on (+) or leaves them off (-)
ONE_SIDED = 1e-6     # of the tolerance
TIE_SHARE = 0.30
Z_MAX = 2.0 ** 20


# ----------------------------------------------------------------------------
# generator
# ----------------------------------------------------------------------------
def test_attribute_kinds():
    from hdgnn.synth import synth_commits
    ref = synth_commits(3, 37, 19, 137)
    for kind in T.XKINDS:
        cb = T.commits(kind, 3, 37, 19, 137)
        cb.validate()
        for k in ("a", "y", "hid", "nlen"):
            assert np.array_equal(getattr(cb, k), getattr(ref, k))
        assert cb.x.dtype == np.float32
    assert np.array_equal(T.commits("int10", 3, 37, 19, 137).x, ref.x)
    x = T.commits("half", 3, 37, 19, 137).x
    want = (np.arange(37) - 18) / 2.0
    for row in x:
        assert np.array_equal(np.sort(row), want)           # Ne distinct half-integers: nd = Ne
    assert not np.array_equal(x[0], x[1])
    assert (T.commits("eq3", 3, 37, 19, 137).x == 3).all()
    assert (T.commits("eq0", 3, 37, 19, 137).x == 0).all()


def test_roles_cover_signs_and_classes():
    for roles, signs in ((T.ROLES, 4), (T.EE_ROLES, 2)):
        for cls in (0, 1):
            assert len({(r.si, r.sj) for r in roles if r.cls == cls and not r.d0}) >= signs - 1
        assert len({(r.si, r.sj) for r in roles}) == signs
        assert sum(r.d0 for r in roles) == 1
    assert T.WHOLE_ROLES[0] == (0, True)
    assert {w for w in T.WHOLE_ROLES[1:]} == {(1, True), (1, False)}


@pytest.mark.parametrize("v", [1, 2, 3, 4])
def test_lattice_touches_only_the_lattice(v):
    cb = T.commits("half", 2, 37, 19, 137)
    flat, info = T.lattice_build(5, v, cb)
    base = R.regime_flat("trained", 5, v)
    mask = T.lattice_mask(v)
    assert flat.dtype == np.float32 and set(info) == set(T.lattice_layers(v))
    assert np.array_equal(flat[~mask], base[~mask])
    lat = flat[mask].astype(np.float64) * 64
    assert np.array_equal(lat, np.round(lat))                # multiples of the lattice unit
    assert set(T.lattice_layers(v)) == {1: {"H1"}, 2: {"E1", "H1"}, 3: {"EE", "H1"},
                                        4: {"E1", "EE", "H1"}}[v]
    V = R.views(flat, v)
    W = V[T.layer_vars(v, "H1")[0][0]][:, list(T.LU)]
    zero_rows = {1: [], 3: [], 2: [0, 1, 4, 5], 4: list(range(8))}[v]
    assert (W[zero_rows] == 0).all()
    assert (W[[r for r in range(10) if r not in zero_rows]] != 0).sum() >= 8 * (9 - len(zero_rows))
    assert np.array_equal(flat, T.lattice_flat(5, v, cb))    # a pure function of its inputs
    # the kink guard's step keeps the zero rows zero
    assert ((flat.astype(np.float64) * (1 + 2e-7) == 0) == (flat == 0)).all()


# ----------------------------------------------------------------------------
# case table
# ----------------------------------------------------------------------------
def test_case_table_is_the_issue_matrix():
    n = {}
    for c in T.CASES:
        n[c.group] = n.get(c.group, 0) + 1
    # A: 3 shapes x 4 variants x 2 x kinds;  B: 3 shapes x 2 variants x 2 block modes x 2 kinds
    # + the prepared-buffer case + the wide form;  C: 2 shapes x 3 variants x 4 forms x 2 kinds;
    # D: integer x;  E: 6 runs x 2 kinds;  F: 2 variants x {x = 3, x = 0} x 2 paths
    assert n == {"A": 24, "B": 26, "C": 48, "D": 1, "E": 12, "F": 8}
    assert len({T.case_id(c) for c in T.CASES}) == len(T.CASES)
    for c in T.CASES:
        assert c.path == {"A": "general", "B": "fused", "C": "general", "D": "general"}.get(
            c.group, c.path)
        assert (c.split in ("1", "0")) if c.group == "B" else c.split is None
        if c.path == "fused":
            assert c.variant in (2, 4) and c.ne <= 256 and c.nc <= 160
        assert (c.form in T.C_FORMS) if c.group == "C" else c.form is None
        assert (c.xkind in ("eq3", "eq0")) == (c.group == "F")
        assert (c.edensity == 0.5) == ((c.B, c.ne, c.nc) == T.B_HBM)
    assert sum((c.B, c.ne, c.nc) == T.B_HBM for c in T.CASES) == 1
    assert sum(c.nc == 81 for c in T.CASES) == 1
    assert any(c.group == "C" and c.variant == 1 and c.xkind == "half" and c.form == "sorted"
               for c in T.CASES)
    keys = {T._key(c) for c in T.CASES}
    assert set(T.MOVED) <= keys and T.ALIVE <= keys


# ----------------------------------------------------------------------------
# every distinct oracle input
# ----------------------------------------------------------------------------
def _oracle(flat64, cb, v, dtype=torch.float64, trace=None):
    out, g = model_ref.loss_and_grads(model_ref.unflatten(flat64, v),
                                      cb.x.astype(np.float64), cb.a, cb.y, cb.hid, cb.nlen,
                                      v, dtype, trace=trace)
    return out, np.concatenate([np.asarray(g[k], np.float64).reshape(-1)
                                for k, _, _ in olayout.keyed_specs(v)])


def _frac(g1, g0, v, fused, names=None):
    """max |g1 - g0| / tolerance over the variables (names: only those)."""
    worst = 0.0
    for name, (o, shape) in layout.offsets(v).items():
        if names is not None and name not in names:
            continue
        n = int(np.prod(shape))
        worst = max(worst, (np.abs(g1[o:o + n] - g0[o:o + n])
                            / T.grad_tol(g0[o:o + n], fused)).max())
    return worst


def _classes(cb):
    I, J = model_ref.pair_index(cb.Ne)
    Ip, Jq = model_ref.pair_index(cb.Nc)
    return {"E1": cb.a[:, I, J], "EE": cb.a[:, I, J], "H1": cb.y[:, Ip, Jq]}


def _check_ties(e, cb, flat, tr):
    """Ties exist where they must, from the oracle's own trace."""
    v = e.variant
    cls, V, lu = _classes(cb), R.views(flat, v), list(T.LU)
    for layer in T.lattice_layers(v):
        z = tr[layer][..., lu].numpy()                                   # (B, P, 8)
        two = T.two_valued(layer, v, cb)
        tie, on, off = z == 0, z > 0, z < 0
        assert tie.any(1).all(), "%s: a unit without a tie in a commit" % layer
        if two:
            assert (on | off).any(1).all(), layer
        else:
            assert on.any(1).all() and off.any(1).all(), "%s: no pair on / off" % layer
        share = tie.mean()
        assert share <= TIE_SHARE, "%s: tie share %.3f" % (layer, share)
        c = cls[layer][..., None]
        assert (tie & (c == 0)).any() and (tie & (c == 1)).any(), layer  # both z0 and fl(z0 + d)
        ws, _ = T.layer_vars(v, layer)
        if layer == "EE":
            signs = {(float(s),) for s in np.sign(V[ws[0]][0, lu])}
            d = V[ws[1]][1, lu] - V[ws[1]][0, lu]
            assert signs == {(1.0,), (-1.0,)}
        else:
            W = V[ws[0]][:, lu]
            ri, rj, rc = {"E1": (0, 1, 2), "H1": (2, 6, 8)}[layer]
            d = W[rc + 1] - W[rc]
            signs = {(float(a), float(b)) for a, b in zip(np.sign(W[ri]), np.sign(W[rj]))}
            if not (layer == "H1" and v == 4):
                assert len(signs) == 4, "%s: sign pairs %s" % (layer, signs)
        if two:     # a whole class-0 set tied beside class-1 pairs that are on
            assert any((tie[..., u] == (c[..., 0] == 0)).all() and d[u] > 0 for u in range(8))
            assert (d != 0).all()
        else:
            assert (d == 0).sum() == 1
        print("%s: tie share %.4f" % (layer, share))


def _check_sorted_duplicates(cb, tr):
    """Group C, variant 1, half x: a tied pair whose row hunk and whose column hunk share their
    neighbourhood sums with another hunk -- the threshold of the sorted form's slot search lies
    exactly on a run of equal alpha resp. beta values."""
    B3, _ = T.features(cb)["H"]
    Ip, Jq = model_ref.pair_index(cb.Nc)
    z = tr["H1"][..., list(T.LU)].numpy()
    found = [False, False]
    for b in range(cb.x.shape[0]):
        nbr = np.zeros((cb.Nc, 4))
        nbr[Ip] = B3[b, :, 0:4]
        nbr[Jq] = B3[b, :, 4:8]
        _, inv, cnt = np.unique(nbr, axis=0, return_inverse=True, return_counts=True)
        dup = cnt[inv.reshape(-1)] > 1                                   # (Nc,)
        tied = (z[b] == 0).any(1)                                        # (Pc,)
        found[0] |= bool((tied & dup[Ip]).any())
        found[1] |= bool((tied & dup[Jq]).any())
    assert all(found), found


@pytest.mark.parametrize("entry", T.oracle_entries(), ids=T.entry_id)
def test_table_entry(entry):
    """Exactness: the float32 oracle's lattice pre-activations are the float64 oracle's bits,
    |z| < 2^20.  Ties: every lattice unit has in every commit a tie, a pair on and a pair off
    (a two-valued layer: a tie and the other class), ties fall on class-0 and on class-1 pairs,
    the sign pairs and the d = 0 unit are there, and at most 30 % of a layer's lattice
    pre-activations tie.  Bite: raising one layer's lattice biases by 2^-40, which is what a
    `>=` would see, moves that layer's own weight or bias gradient by >= 50 x the entry's GPU
    tolerance.  One-sidedness: lowering all of them by 2^-40 moves no gradient by more than
    1e-6 of it.  Then the regimes' guards with the lattice parameters held: kink guard (the
    other parameters x (1 + 2e-7 s), three draws, <= 0.5 of the tolerance), max |logit| <=
    1e4, float32 CE within 5e-6 relative.  An entry that fails moves to the next seed in
    _ties.MOVED; none is waived."""
    e = entry
    v = e.variant
    cb, flat = T.inputs(e)
    f64 = flat.astype(np.float64)
    tr, tr32 = {}, {}
    out, g0 = _oracle(f64, cb, v, trace=tr)
    assert np.isfinite(g0).all()
    P32 = model_ref.to_torch_params(model_ref.unflatten(flat, v), torch.float32, False)
    ce32 = float(model_ref.forward(P32, cb.x, cb.a, cb.y, cb.hid, cb.nlen, v, torch.float32,
                                   trace=tr32)["ce"])
    lu = list(T.LU)
    for layer in T.lattice_layers(v):
        z, z32 = tr[layer][..., lu].numpy(), tr32[layer][..., lu].numpy()
        assert z32.dtype == np.float32 and np.array_equal(z, z32.astype(np.float64)), layer
        assert np.abs(z).max() < Z_MAX
    _check_ties(e, cb, flat, tr)
    if v == 1 and e.xkind == "half" and any(c.form == "sorted" and T.entry_of(c)[:-1] == e[:-1]
                                            for c in T.CASES):
        _check_sorted_duplicates(cb, tr)

    low = f64.copy()
    for layer in T.lattice_layers(v):
        up = f64.copy()
        up[T.bias_index(v, layer)] += EPS
        low[T.bias_index(v, layer)] -= EPS
        if layer == "EE" and v == 3:
            continue        # model_3 computes the entity-edge stage and never uses it (B2 = B1):
            #                 EE's gradient is the regulariser's alone, nothing there can bite
        ws, b = T.layer_vars(v, layer)
        bite = _frac(_oracle(up, cb, v)[1], g0, v, e.fused, set(ws) | {b})
        print("%s: bite %.3g x tol" % (layer, bite))
        assert bite >= BITE, "%s: bite %.3g x tol" % (layer, bite)
    minus = _frac(_oracle(low, cb, v)[1], g0, v, e.fused)
    print("minus side %.3g of tol" % minus)
    assert minus <= ONE_SIDED

    assert np.abs(out["logits"]).max() <= LOGIT_MAX
    assert abs(ce32 - float(out["ce"])) <= GUARD_FRACTION * CE_RTOL * float(out["ce"])
    free = ~T.lattice_mask(v)
    worst = 0.0
    for draw in range(GUARD_DRAWS):
        s = np.random.default_rng(7000 + draw).choice([-1.0, 1.0], len(flat))
        worst = max(worst, _frac(_oracle(f64 * (1 + GUARD_EPS * s * free), cb, v)[1], g0, v,
                                 e.fused))
    print("guard %.3g of tol, max|logit| %.4g, CE %.4g" % (worst, np.abs(out["logits"]).max(),
                                                            float(out["ce"])))
    assert worst <= GUARD_FRACTION
