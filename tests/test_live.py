"""Liveness on the CPU (tests/_live.py): the `live` regime's properties, the entries of the four
earlier tables that miss the gradient-reach condition pinned to _live.KNOWN_DEAD, the new
table against the matrix it was written from, and every entry of it against the regimes'
guards and the three liveness conditions.  Float64 oracle only; no engine."""
import numpy as np
import pytest

from hdgnn import layout
from tests import _live as LV
from tests import _regimes as R
from tests import _ties as T
from tests.test_general_gpu import _oracle
from tests.test_param_regimes import check_well_conditioned


# ----------------------------------------------------------------------------
# the regime
# ----------------------------------------------------------------------------
@pytest.mark.parametrize("v", [1, 2, 3, 4])
@pytest.mark.parametrize("ne,nc", [(7, 5), (16, 16), (37, 19), (256, 160)])
def test_live_flat_is_trained_alive_scaled(v, ne, nc):
    """Step by step against its three sources, bit for bit; only the named second layers and
    E3's three edited variables differ from `trained`; no exact zero; a pure function."""
    flat = LV.live_flat(5, v, ne, nc)
    base = R.regime_flat("trained", 5, v)
    assert flat.dtype == np.float32 and flat.shape == (layout.n_params(v),)
    assert (flat != 0).all()
    assert np.array_equal(flat, LV.live_flat(5, v, ne, nc))
    want = base.copy()
    have = R.first_layers(v)
    if "E3" in have:
        want = T._alive(want, v)
    V = R.views(want, v)
    se, sc = np.float32(min(1, 16 / ne)), np.float32(min(1, 16 / nc))
    scaled = []
    if "E1" in have:
        scaled += [("phi_E_O1/r1_w5o:0", se), ("phi_E_O1/r1_b5o:0", se)]
    if "EE" in have:
        scaled += [("phi_E_R1/r1_w2r:0", se), ("phi_E_R1/r1_b2r:0", se)]
    scaled += [("mlp_hunk_B2/r1_w2r:0", sc), ("mlp_hunk_B2/b2:0", sc)]
    for name, s in scaled:
        V[name][...] = V[name] * s
    assert np.array_equal(flat, want)
    assert {n for n, _ in scaled} == {n for key in LV.PAIR_SCALE if key in have
                                      for n in LV.second_layer(v, key)}
    if ne <= 16 and nc <= 16 and "E3" not in have:
        assert np.array_equal(flat, base)          # nothing to scale, nothing to revive
    deg = LV.regime_flat("degenerate", 5, v, ne, nc)
    assert np.array_equal(deg, R._degenerate(flat.copy(), v))


# ----------------------------------------------------------------------------
# the earlier tables, pinned as they are
# ----------------------------------------------------------------------------
EARLIER = LV.earlier_tables()


@pytest.mark.parametrize("table", sorted(EARLIER))
def test_known_dead_is_pinned(table):
    """The gradient-reach condition (every variable that can reach the loss has max |g_data|
    >= 1e-3) over the table's oracle inputs: the entries that miss it are exactly
    _live.KNOWN_DEAD[table], of the kind recorded there.  The earlier suites stay as they are;
    a new entry of one of them cannot be dead unnoticed."""
    ents = EARLIER[table]
    assert len({eid for eid, _, _ in ents}) == len(ents)
    found = {}
    for eid, v, make in ents:
        cb, flat = make()
        _, g = _oracle(flat, cb, v)
        dead = LV.dead_variables(flat, g, v)
        if dead:
            found[eid] = LV.dead_kind(dead)
        if v == 3:      # the exemption itself: model_3's entity-edge stage has no data gradient
            gd = LV.data_grad(flat, g)
            for n in LV.exempt(3):
                o, s = layout.offsets(3)[n]
                if not n.startswith("map_conv/"):
                    assert not gd[o:o + int(np.prod(s))].any(), (eid, n)
    print("%s: %d of %d entries dead (%d of them exactly 0 on E1 / E3)" % (
        table, len(found), len(ents), sum(k == "zero" for k in found.values())))
    assert found == {k: kind for k, (kind, _) in LV.KNOWN_DEAD[table].items()}


def test_known_dead_counts():
    n = {t: len(d) for t, d in LV.KNOWN_DEAD.items()}
    assert n == {"regimes": 19, "labels": 16, "ties": 3, "tails": 0}
    # the issue's count for _regimes: of the 50 entries with Ne <= 300, 16 compare E1 / E3 with
    # exact zeros and the 9 model_3 entries their entity-edge stage (exempt): 25
    reg = LV.KNOWN_DEAD["regimes"]
    zero = [k for k, (kind, _) in reg.items() if kind == "zero" and "401" not in k]
    m3 = [e for e in R.oracle_entries() if e[1] == 3]
    assert len(zero) == 16 and len(m3) == 9 and len(R.oracle_entries()) == 52
    for d in LV.KNOWN_DEAD.values():
        assert all(kind in ("zero", "weak") and reason for kind, reason in d.values())


# ----------------------------------------------------------------------------
# the new table
# ----------------------------------------------------------------------------
def test_case_table_is_the_issue_matrix():
    n = {}
    for c in LV.CASES:
        n[c.group] = n.get(c.group, 0) + 1
    # A: 28 shapes x 2 block modes;  B: (8 + 4) shapes x 2;  C: 4 shapes x 4 variants + 2 forms
    # x 2 variants;  D: 2 shapes x 2 variants x 2;  E: 2 shapes x 5 runs;  S: the slow one
    assert n == {"A": 56, "B": 24, "C": 20, "D": 8, "E": 10, "S": 1}
    assert len({LV.case_id(c) for c in LV.CASES}) == len(LV.CASES)
    assert len(LV.A_SHAPES) == len(set(LV.A_SHAPES)) == 28
    for c in LV.CASES:
        assert c.path == {"A": "fused", "B": "fused", "C": "general", "D": "fused",
                          "S": "general"}.get(c.group, c.path)
        assert c.variant == {"A": 2, "B": 4, "S": 2}.get(c.group, c.variant)
        assert c.regime == ("degenerate" if c.group == "D" else "live")
        if c.path == "fused":
            assert c.variant in (2, 4) and c.ne <= 256 and c.nc <= 160
            assert (c.split in ("1", "0")) or (c.group == "E" and c.variant == 4)
        else:
            assert c.split is None
        if c.group in "ABD":
            assert c.B == 2
            i = LV.A_SHAPES.index((c.ne, c.nc))
            assert c.xkind == ("int10", "real")[i % 2]
            assert c.edensity == (0.5 if (c.ne, c.nc) in LV.DENSE_EDGES else 0.05)
        assert (c.form is not None) == (c.group == "C" and c.form in ("sorted", "tiled"))
        assert (c.dseed, c.pseed) in LV.seed_walk(c.regime, c.variant, c.ne, c.nc)
    a = {(c.ne, c.nc) for c in LV.CASES if c.group == "A"}
    assert a == set(LV.A_SHAPES) and set(LV.BENCH_SHAPES) <= a
    assert {(c.ne, c.nc) for c in LV.CASES if c.group == "B"} == set(LV.B_SHAPES)
    assert len(LV.B_SHAPES) == 12 and set(LV.BENCH_SHAPES) <= set(LV.B_SHAPES)
    # gaps 1-3 of the issue: a live fused entity stage past Ne 120, an own half past 102
    # nodes in split mode, the four benchmark shapes
    assert any(c.ne >= 205 and c.split == "1" for c in LV.CASES if c.group == "A")
    assert {(200, 74), (250, 114), (250, 150), (256, 160)} == set(LV.BENCH_SHAPES)
    keys = {LV._key(c.regime, c.variant, c.B, c.ne, c.nc, c.xkind) for c in LV.CASES}
    assert set(LV.MOVED) <= keys
    for k, seeds in LV.MOVED.items():
        walk = LV.seed_walk(k[0], k[1], k[3], k[4])
        assert seeds in walk[1:]


def _entry_params():
    return [pytest.param(e, id=LV.entry_id(e),
                         marks=[pytest.mark.slow] if (e.B, e.ne, e.nc) == LV.S_SHAPE else [])
            for e in LV.oracle_entries()]


@pytest.mark.parametrize("entry", _entry_params())
def test_table_entry_is_well_conditioned_and_live(entry):
    """The regimes' three guards, unchanged (test_param_regimes.check_well_conditioned: kink
    <= 0.5 of the tolerance under the 2e-7 perturbation, max |logit| <= 1e4, the float32
    oracle's CE to 5e-6 relative), then _live.check_live: every variable that can reach the
    loss has max |g_data| >= 1e-3, every 20-column first-layer weight has >= 8 hidden units
    with a gradient, and zeroing r1_b1o, r1_b5o, o1_b1o or o1_b2o (variants 2, 4) moves the
    worst logit by >= 50 x the entry's logit tolerance.  An entry that fails moves along
    _live.seed_walk and is recorded in _live.MOVED; none is waived."""
    e = entry
    cb, flat = LV.inputs(e)
    ref = check_well_conditioned(flat, cb, e.variant, e.fused)
    LV.check_live(flat, cb, e.variant, e.fused, ref=ref)
