"""Refinement on the host (CPU): hdgnn.metrics.refine, the restatement hdg_refine is compared
with on the GPU, against the definitions of include/hdgnn.h themselves -- a planted family
whose highest score is a wrong pair between two groups (no tree at any threshold recovers
the groups, refinement from any tree's cut does), the objective recomputed pair by pair, a
brute-force search for an improving move after convergence, a sweep written as plain loops
-- the Python mirrors of HDG_RF_* and the host-side argument checks of hdg_refine.
Every comparison is integer equality.
"""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from hdgnn import _lib, data, metrics

RULES = ("mean", "any", "both")
METHODS = ("single", "complete", "average")


def _onehot(y):
    return np.stack([1 - y, y], 1).astype(np.float32)


def _probs(p1):
    return np.ascontiguousarray(np.stack([1.0 - p1, p1], 1), np.float32)


def _canon(g):
    """Dense ids ordered by each group's smallest member."""
    g = np.asarray(g)
    _, first, inv = np.unique(g, return_index=True, return_inverse=True)
    return np.argsort(np.argsort(first))[inv].astype(np.int32)


def _tprime(thr, rule):
    thr = np.float32(thr)
    return thr + thr if rule == "mean" else thr


# ---------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------
def wrong_first_merge(seed=11, nc=18, B=5):
    """Three planted groups, same-group scores 0.7 .. 0.8, others 0 .. 0.2, and one
    cross-group pair per commit at 0.95 in both directions: every tree merges it first.
    -> (labels (B, R) uint8, scores (B, R) float32, planted groups (B, nc) in dense ids)."""
    rng = np.random.default_rng(seed)
    I, J = data.pair_index(nc)
    y = np.zeros((B, len(I)), np.uint8)
    p1 = np.zeros((B, len(I)), np.float32)
    planted = np.zeros((B, nc), np.int32)
    for b in range(B):
        grp = rng.permutation(np.arange(nc) % 3)
        same = grp[I] == grp[J]
        p1[b] = np.where(same, 0.7 + 0.1 * rng.random(len(I)), 0.2 * rng.random(len(I)))
        u, v = int(np.flatnonzero(grp == 0)[0]), int(np.flatnonzero(grp == 1)[0])
        p1[b, ((I == u) & (J == v)) | ((I == v) & (J == u))] = 0.95
        y[b] = same
        planted[b] = _canon(grp)
    return y, p1, planted


def noisy_planted(nc, seed, B=2, k=4):
    """k planted groups, scores 0.65 inside and 0.35 across, + 0.25 sigma noise, clipped."""
    rng = np.random.default_rng(seed)
    I, J = data.pair_index(nc)
    grp = rng.integers(0, k, (B, nc))
    same = grp[:, I] == grp[:, J]
    p1 = np.clip(np.where(same, 0.65, 0.35) + 0.25 * rng.standard_normal(same.shape), 0.0, 1.0)
    return same.astype(np.uint8), p1.astype(np.float32)


def uniform(nc, seed, B=2):
    rng = np.random.default_rng(seed)
    y = (rng.random((B, nc * (nc - 1))) < 0.3).astype(np.uint8)
    return y, rng.random((B, nc * (nc - 1)), dtype=np.float32)


def grid(nc, seed, B=2):
    """Scores on the 1/256 grid: many exact ties, and pairs exactly at the bound."""
    rng = np.random.default_rng(seed)
    y = (rng.random((B, nc * (nc - 1))) < 0.3).astype(np.uint8)
    return y, (rng.integers(96, 161, (B, nc * (nc - 1))) / 256.0).astype(np.float32)


FAMILIES = {"uniform": uniform, "grid": grid, "noisy": noisy_planted}


# ---------------------------------------------------------------------------------------
# the definitions, pair by pair and step by step
# ---------------------------------------------------------------------------------------
def _gains(p1, nc, tp, rule):
    """include/hdgnn.h's a_pq, one pair at a time in numpy float32 scalars."""
    I, J = data.pair_index(nc)
    S = np.zeros((nc, nc), np.float32)
    S[I, J] = p1
    A = np.zeros((nc, nc), np.int64)
    two, scale = np.float32(2), np.float32(262144)
    for p in range(nc):
        for q in range(p + 1, nc):
            a, c = S[p, q], S[q, p]
            with np.errstate(invalid="ignore", over="ignore"):
                w = a + c if rule == "mean" else (max(a, c) if rule == "any" else min(a, c))
            if np.isnan(a) or np.isnan(c) or np.isnan(w):
                continue
            d = np.float32(w) - np.float32(tp)
            A[p, q] = A[q, p] = int(np.rint(min(max(d, -two), two) * scale))
    return A


def _objective(A, g):
    iu, ju = np.triu_indices(len(g), 1)
    return int(A[iu, ju][g[iu] == g[ju]].sum())


def _start_slots(ids, nc):
    slot = list(range(nc))
    if ids is not None:
        for i in range(nc):
            if 0 <= ids[i] < nc:
                slot[i] = min(j for j in range(nc) if ids[j] == ids[i])
    return slot


def _slow_sweeps(A, slot, max_sweeps):
    """The sweep of include/hdgnn.h as plain loops -> the slots after every sweep run."""
    nc = len(slot)
    slot = list(slot)
    states = []
    for _ in range(max_sweeps):
        moved = False
        for p in range(nc):
            g = slot[p]
            S = [0] * nc
            size = [0] * nc
            for q in range(nc):
                size[slot[q]] += 1
                if q != p:
                    S[slot[q]] += int(A[p, q])
            best, to = S[g], g
            for h in range(nc):                      # ascending: a tie keeps the lower slot
                if h != g and size[h] > 0 and S[h] > best:
                    best, to = S[h], h
            if size[g] > 1 and 0 > best:             # strictly: a non-empty slot wins a tie
                best, to = 0, min(h for h in range(nc) if size[h] == 0)
            if to != g:
                slot[p] = to
                moved = True
        states.append(list(slot))
        if not moved:
            break
    return states


# ---------------------------------------------------------------------------------------
# the wrong-first-merge family
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("rule", RULES)
def test_refinement_repairs_a_wrong_first_merge(rule, method):
    y, p1, planted = wrong_first_merge()
    label, probs = _onehot(y), _probs(p1)
    m, lv, cv, _, lk = metrics.agglomerate(label, probs, rule, method)
    _, best, best_tp = metrics.best_threshold(lv, cv, lk, rule, "f1")
    print(rule, method, "best tree f1", best, "at bound", best_tp)
    assert best < 1.0                                 # no cut of the tree is the planted partition
    for tp in (_tprime(0.5, rule), np.float32(best_tp)):
        start = metrics.cut_groups(m, lv, tp)
        assert not np.array_equal(start, planted)
        ut, g, rq = metrics.refine(label, probs, start, 0.5, rule, max_sweeps=4)
        print(rule, method, float(tp), "ut", ut.tolist(), "rq", rq.tolist())
        np.testing.assert_array_equal(g, planted)
        assert (ut[:, metrics.UT_SD] == 0).all() and (ut[:, metrics.UT_DS] == 0).all()
        assert (rq[:, metrics.RF_Q_CONVERGED] == 1).all()
        assert (rq[:, metrics.RF_Q_SWEEPS] <= 4).all() and (ut[:, metrics.RF_MOVES] > 0).all()
        assert metrics.scores_from_untangle(ut)["exact"] == 1.0


def test_refinement_from_singletons_also_finds_the_planted_groups():
    y, p1, planted = wrong_first_merge()
    ut, g, rq = metrics.refine(_onehot(y), _probs(p1), None, 0.5, "mean", max_sweeps=8)
    np.testing.assert_array_equal(g, planted)
    assert (rq[:, metrics.RF_Q_START] == 0).all() and (rq[:, metrics.RF_Q_CONVERGED] == 1).all()


# ---------------------------------------------------------------------------------------
# properties
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", sorted(FAMILIES))
@pytest.mark.parametrize("nc", [2, 3, 7, 33])
def test_properties(nc, family):
    B = 2
    y, p1 = FAMILIES[family](nc, seed=500 + nc)
    label, probs = _onehot(y), _probs(p1)
    rng = np.random.default_rng(nc)
    for rule in RULES:
        tp = _tprime(0.5, rule)
        A = [_gains(p1[b], nc, tp, rule) for b in range(B)]
        for b in range(B):
            np.testing.assert_array_equal(metrics.refine_gains(p1[b], tp, rule)[0], A[b])
        starts = [None, np.zeros((B, nc), np.int64), rng.integers(0, max(2, nc // 3), (B, nc)),
                  metrics.untangle_counts(label, probs, 0.5, rule)[1]]
        for start in starts:
            ut, g, rq = metrics.refine(label, probs, start, 0.5, rule, max_sweeps=64)
            assert (rq[:, metrics.RF_Q_CONVERGED] == 1).all()          # the cap is far away
            assert (rq[:, metrics.RF_Q_END] >= rq[:, metrics.RF_Q_START]).all()
            assert (rq[:, metrics.RF_Q_END] - rq[:, metrics.RF_Q_START] >= ut[:, metrics.RF_MOVES]).all()
            four = [metrics.UT_SS, metrics.UT_SD, metrics.UT_DS, metrics.UT_DD]
            assert (ut[:, four].sum(1) == nc * (nc - 1) // 2).all()
            for b in range(B):
                s0 = _start_slots(None if start is None else start[b], nc)
                assert rq[b, metrics.RF_Q_START] == _objective(A[b], np.asarray(s0))
                assert rq[b, metrics.RF_Q_END] == _objective(A[b], g[b])
                np.testing.assert_array_equal(g[b], _canon(g[b]))
                assert ut[b, metrics.UT_GROUPS] == g[b].max() + 1
                # the plain loops reach the same partition, sweep for sweep
                states = _slow_sweeps(A[b], s0, 64)
                assert len(states) == rq[b, metrics.RF_Q_SWEEPS]
                np.testing.assert_array_equal(g[b], _canon(states[-1]))
                one = metrics.refine(label[b:b + 1], probs[b:b + 1],
                                     None if start is None else start[b:b + 1], 0.5, rule,
                                     max_sweeps=1)
                np.testing.assert_array_equal(one[1][0], _canon(states[0]))
                assert one[2][0, metrics.RF_Q_SWEEPS] == 1
                assert one[2][0, metrics.RF_Q_CONVERGED] == int(len(states) == 1)
                assert one[2][0, metrics.RF_Q_END] == _objective(A[b], one[1][0])
                # converged: no single move to a group or to a new one raises Q
                for p in range(nc):
                    S = np.bincount(g[b], weights=A[b][p], minlength=nc + 1)
                    assert S.max() <= S[g[b, p]], (b, p)               # S[nc] = 0: a new group
                    if np.count_nonzero(g[b] == g[b, p]) == 1:
                        assert S[g[b, p]] == 0
            again = metrics.refine(label, probs, g, 0.5, rule, max_sweeps=8)
            np.testing.assert_array_equal(again[1], g)
            assert (again[0][:, metrics.RF_MOVES] == 0).all()
            assert (again[2][:, metrics.RF_Q_SWEEPS] == 1).all()
            np.testing.assert_array_equal(again[2][:, :2], rq[:, [1, 1]])
            if start is not None:                  # the numbering of the input does not matter
                perm = rng.permutation(nc)
                other = metrics.refine(label, probs, perm[np.asarray(start)], 0.5, rule, 64)
                for a, c in zip(other, (ut, g, rq)):
                    np.testing.assert_array_equal(a, c)


@pytest.mark.parametrize("nc", [3, 7, 33])
def test_out_of_range_ids_start_alone(nc):
    y, p1 = noisy_planted(nc, seed=700 + nc)
    label, probs = _onehot(y), _probs(p1)
    rng = np.random.default_rng(nc)
    k = max(1, nc // 4)
    start = rng.integers(0, k, (2, nc))
    alone = np.zeros((2, nc), bool)
    alone[:, [0, nc - 1]] = True
    wild, fresh = start.copy(), start.copy()
    wild[:, 0], wild[:, nc - 1] = -7, nc + 5
    fresh[:, 0], fresh[:, nc - 1] = nc - 1, nc - 2           # ids nobody else holds (k <= nc - 2)
    assert k <= nc - 2
    for ms in (1, 8):
        a = metrics.refine(label, probs, wild, 0.5, "mean", ms)
        c = metrics.refine(label, probs, fresh, 0.5, "mean", ms)
        for x, z in zip(a, c):
            np.testing.assert_array_equal(x, z)
    big = np.full((2, nc), 2 ** 31 - 1, np.int64)              # every id out of range: singletons
    for x, z in zip(metrics.refine(label, probs, big, 0.5, "any", 8),
                    metrics.refine(label, probs, None, 0.5, "any", 8)):
        np.testing.assert_array_equal(x, z)


def test_no_edge_pairs_and_infinite_scores():
    nc = 7
    y, p1 = noisy_planted(nc, seed=9, B=1)
    I, J = data.pair_index(nc)
    p1[0, (I == 0) & (J == 1)] = np.nan                     # one direction only
    p1[0, (I == 2) & (J == 3)] = np.inf
    p1[0, (I == 3) & (J == 2)] = -np.inf                    # NaN under mean, an edge otherwise
    p1[0, (I == 4) & (J == 5)] = np.inf
    for rule, nans in (("mean", 2), ("any", 1), ("both", 1)):
        A, n = metrics.refine_gains(p1[0], _tprime(0.5, rule), rule)
        np.testing.assert_array_equal(A, _gains(p1[0], nc, _tprime(0.5, rule), rule))
        assert n == nans and A[0, 1] == 0 and (A == A.T).all()
        assert A[4, 5] == (2 << 18 if rule != "both" else A[5, 4])      # the clamp at +2
        assert A[2, 3] == {"mean": 0, "any": 2 << 18, "both": -(2 << 18)}[rule]
        ut = metrics.refine(_onehot(y), _probs(p1), None, 0.5, rule)[0]
        assert ut[0, metrics.RF_NAN] == nans


# ---------------------------------------------------------------------------------------
# errors, mirrors, the library's host-side checks
# ---------------------------------------------------------------------------------------
def test_errors():
    y, p1 = uniform(5, 1)
    label, probs = _onehot(y), _probs(p1)
    for thr in (float("nan"), float("inf"), float("-inf")):
        for rule in RULES:
            with pytest.raises(ValueError):
                metrics.refine(label, probs, None, thr, rule)
    with pytest.raises(ValueError):
        metrics.refine(label, probs, None, 2e38, "mean")          # t' = inf
    metrics.refine(label, probs, None, 2e38, "any")
    for ms in (0, -1, 65):
        with pytest.raises(ValueError):
            metrics.refine(label, probs, None, 0.5, "mean", ms)
    with pytest.raises(ValueError):
        metrics.refine(label, probs, None, 0.5, "most")
    with pytest.raises(ValueError):
        metrics.refine(label, probs[:, :, :-1], None)


def test_python_mirrors_match_the_header():
    with open(os.path.join(ROOT, "include", "hdgnn.h")) as f:
        defs = dict(re.findall(r"#define\s+(HDG_RF_[A-Z_0-9]+)\s+(\d+)", f.read()))
    assert sorted(defs) == ["HDG_RF_MAX_SWEEPS", "HDG_RF_MOVES", "HDG_RF_NAN", "HDG_RF_Q_CONVERGED",
                            "HDG_RF_Q_END", "HDG_RF_Q_SLOTS", "HDG_RF_Q_START", "HDG_RF_Q_SWEEPS",
                            "HDG_RF_SLOTS"]
    for name, v in defs.items():
        assert getattr(_lib, name[4:]) == int(v), name
        assert getattr(metrics, name[4:]) == int(v), name
    assert _lib.RF_SLOTS == _lib.UT_SLOTS and _lib.ABI_VERSION == 9


def test_library_argument_checks_on_the_host():
    lib = _lib.load()
    ok = _lib.Shape(4, 200, 74, 2, 4, 0)
    for b, nc in ((1, 2), (3, 64), (4, 74), (2, 2048)):
        t = -(-nc // 64)
        words = nc * nc + t * (t + 1) // 2
        assert lib.hdg_refine_workspace_bytes(ctypes.byref(_lib.Shape(b, 2, nc, 2, b, 0)),
                                              0) == b * (words + words % 2) * 4
    for b, nc in ((0, 74), (65536, 74), (4, 1), (4, 2049)):
        assert lib.hdg_refine_workspace_bytes(ctypes.byref(_lib.Shape(b, 200, nc, 2, 4, 0)), 0) == 0
        assert b"must be in" in lib.hdg_last_error()
    one = ctypes.c_void_p(64)                       # never dereferenced: the checks come first
    bt = _lib.Batch(None, None, one, None, None, None)
    args = dict(shape=ok, bt=bt, probs=one, thr=0.5, rule=0, ms=8, flags=0, gin=None, groups=one,
                ut=one, rq=one, ws=one)

    def call(**kw):
        a = dict(args, **kw)
        return lib.hdg_refine(ctypes.byref(a["shape"]), ctypes.byref(a["bt"]), a["probs"],
                              ctypes.c_float(a["thr"]), a["rule"], a["ms"], a["flags"], a["gin"],
                              a["groups"], a["ut"], a["rq"], a["ws"], None)

    einval = 1000
    for kw, word in ((dict(rule=3), b"rule"), (dict(rule=-1), b"rule"), (dict(ms=0), b"max_sweeps"),
                     (dict(ms=65), b"max_sweeps"), (dict(ms=-3), b"max_sweeps"),
                     (dict(flags=1), b"flag"), (dict(flags=-1), b"flag"),
                     (dict(thr=float("nan")), b"finite"), (dict(thr=float("inf")), b"finite"),
                     (dict(thr=float("-inf"), rule=1), b"finite"), (dict(thr=2e38), b"finite"),
                     (dict(ws=ctypes.c_void_p(68)), b"aligned")):
        assert call(**kw) == einval and word in lib.hdg_last_error(), kw
        assert lib.hdg_last_error().startswith(b"hdg_refine:")
    for k in ("probs", "groups", "ut", "rq", "ws"):
        assert call(**{k: None}) == einval and b"NULL" in lib.hdg_last_error(), k
    assert call(bt=_lib.Batch(None, None, None, None, None, None)) == einval
    assert call(shape=_lib.Shape(0, 200, 74, 2, 1, 0)) == einval
    assert call(shape=_lib.Shape(4, 200, 2049, 2, 4, 0)) == einval
    assert lib.hdg_last_error().startswith(b"hdg_refine: nc must be")
