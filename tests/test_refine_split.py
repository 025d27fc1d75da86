"""Refinement with split sweeps on the host (CPU): hdgnn.metrics.refine_split and
refine_split_ladder, the restatements hdg_refine_split and hdg_refine_split_ladder are compared
with on the GPU, against the definitions of include/hdgnn.h themselves -- the family of fused
groups that neither node moves nor merges can cut and a split sweep does, rounds written as
plain loops, the consequences (A) to (D), a split gain past int32, two hand-made cases of the
sweep's skipping rules, the ladder against the loop it stands for -- the Python mirrors of
HDG_RS_*, the host-side argument checks of the two library calls, and main.py's --link-split
against a recorder.  Every comparison is integer equality.
"""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

from _ladder import DEFAULT_LADDER, LADDERS, tprime
from _split import BIG_NC, BIG_Q_END, BIG_Q_START, BIG_SPLIT_GAIN, KINDS, big_split, two_fused
from conftest import ROOT
from hdgnn import _lib, data, metrics
from test_refine import (FAMILIES, RULES, _canon, _gains, _objective, _onehot, _probs, _slow_sweeps,
                         _start_slots, noisy_planted)
from test_refine_merge import _Recorder, _runs, _slow_group_sweep

SPLITS = metrics.RS_Q_SPLITS


# ---------------------------------------------------------------------------------------
# the family of fused groups
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("rule", RULES)
@pytest.mark.parametrize("nc", [24, 66, 132])
def test_split_sweeps_cut_the_fused_groups_nothing_else_can(nc, rule):
    y, p1, halves, fused = two_fused(nc)
    label, probs = _onehot(y), _probs(p1)
    # single linkage chains the halves through the one wrong pair
    m, lv = metrics.agglomerate(label, probs, rule, "single")[:2]
    np.testing.assert_array_equal(metrics.cut_groups(m, lv, tprime(0.5, rule)), fused)
    ut0, g0, rq0 = metrics.refine(label, probs, fused, 0.5, rule, 8)
    utm, gm, rqm = metrics.refine_merge(label, probs, fused, 0.5, rule, 8, 4)
    np.testing.assert_array_equal(g0, fused)                     # "converged", and wrong
    np.testing.assert_array_equal(gm, fused)
    assert (ut0[:, metrics.RF_MOVES] == 0).all() and (utm[:, metrics.RF_MOVES] == 0).all()
    assert (rqm[:, metrics.RM_Q_MERGES] == 0).all() and (rqm[:, metrics.RF_Q_CONVERGED] == 1).all()
    f1 = {24: 0.6, 66: 20 / 31, 132: 0.65625}[nc]
    assert metrics.scores_from_untangle(utm)["f1"] == pytest.approx(f1, abs=1e-12)
    for kinds in ("split", "both"):
        ut, g, rq = metrics.refine_split(label, probs, fused, 0.5, rule, 8, 4, KINDS[kinds])
        print(nc, rule, kinds, rq.tolist())
        np.testing.assert_array_equal(g, halves)
        assert (ut[:, metrics.UT_SD] == 0).all() and (ut[:, metrics.UT_DS] == 0).all()
        assert (rq[:, SPLITS] == 3).all() and (rq[:, metrics.RM_Q_ROUNDS] == 2).all()
        assert (rq[:, metrics.RM_Q_MERGES] == 0).all() and (ut[:, metrics.RF_MOVES] == 0).all()
        assert (rq[:, metrics.RF_Q_CONVERGED] == 1).all()
        np.testing.assert_array_equal(rq[:, metrics.RM_Q_NODE], rq0[:, metrics.RF_Q_END])
        assert (rq[:, metrics.RF_Q_END] > rq[:, metrics.RM_Q_NODE]).all()
        assert metrics.scores_from_untangle(ut)["f1"] == 1.0


# ---------------------------------------------------------------------------------------
# the rounds, step by step in plain loops
# ---------------------------------------------------------------------------------------
def _slow_split_sweep(A, slot):
    """The split sweep of include/hdgnn.h as plain loops -> (the slots after it, its splits)."""
    nc = len(slot)
    slot = list(slot)
    filled, splits = set(), 0
    for g in range(nc):
        mem = [p for p in range(nc) if slot[p] == g]
        if len(mem) < 2 or g in filled:
            continue
        best = None
        for i, p in enumerate(mem):                  # ascending p, then q: a tie keeps the first
            for q in mem[i + 1:]:
                if best is None or int(A[p, q]) < best[0]:
                    best = (int(A[p, q]), p, q)
        if best[0] >= 0:
            continue
        _, s1, s2 = best
        G, E = [s1], [s2]
        rest = [m for m in mem if m != s1 and m != s2]
        for m in rest:
            tg = sum(int(A[m, x]) for x in G)
            te = sum(int(A[m, x]) for x in E)
            (E if te > tg else G).append(m)
        for _ in range(metrics.RS_PASSES - 1):
            changed = False
            for m in rest:
                X, O = (G, E) if m in G else (E, G)
                own = sum(int(A[m, x]) for x in X if x != m)
                other = sum(int(A[m, x]) for x in O)
                if other > own:
                    X.remove(m)
                    O.append(m)
                    changed = True
            if not changed:
                break
        if sum(int(A[x, z]) for x in G for z in E) < 0:
            e = min(h for h in range(nc) if h not in slot)
            for z in E:
                slot[z] = e
            filled.add(e)
            splits += 1
    return slot, splits


def _slow_rounds(A, slot, max_sweeps, max_rounds, kinds):
    """-> (final slots, node moves, rq row of 8) by the header's rounds."""
    slot = list(slot)
    q_start = _objective(A, np.asarray(slot))
    sweeps = rounds = merges = splits = moves = 0
    q_node = None
    while True:
        states = _slow_sweeps(A, slot, max_sweeps - sweeps)
        prev = slot
        for s in states:                             # a hunk moves at most once per sweep
            moves += sum(a != c for a, c in zip(prev, s))
            prev = s
        conv = int(states[-1] == (states[-2] if len(states) > 1 else slot))
        sweeps += len(states)
        slot = states[-1]
        if q_node is None:
            q_node = _objective(A, np.asarray(slot))
        merged = split = 0
        if kinds & metrics.RS_MERGE:
            slot, merged = _slow_group_sweep(A, slot)
        if kinds & metrics.RS_SPLIT:
            slot, split = _slow_split_sweep(A, slot)
        rounds += 1
        merges += merged
        splits += split
        if merged + split == 0 or rounds >= max_rounds or sweeps >= max_sweeps:
            break
    q_end = _objective(A, np.asarray(slot))
    return slot, moves, [q_start, q_end, sweeps, int(conv and merged + split == 0), rounds,
                         merges, q_node, splits]


@pytest.mark.parametrize("family", sorted(FAMILIES))
@pytest.mark.parametrize("nc", [2, 3, 7, 33])
def test_rounds_step_by_step(nc, family):
    B = 2
    y, p1 = FAMILIES[family](nc, seed=900 + nc)
    label, probs = _onehot(y), _probs(p1)
    rng = np.random.default_rng(nc)
    wild = rng.integers(0, max(2, nc // 3), (B, nc))
    wild[:, 0], wild[:, nc - 1] = -7, nc + 5
    split_somewhere = 0
    for rule in RULES:
        A = [_gains(p1[b], nc, tprime(0.5, rule), rule) for b in range(B)]
        for start in (None, np.zeros((B, nc), np.int64), wild):
            for ms, mr in ((1, 1), (2, 16), (8, 4)):
                for kinds in (1, 2, 3):
                    ut, g, rq = metrics.refine_split(label, probs, start, 0.5, rule, ms, mr, kinds)
                    assert rq.shape == (B, metrics.RS_Q_SLOTS) and g.dtype == np.int32
                    for b in range(B):
                        s0 = _start_slots(None if start is None else start[b], nc)
                        slot, moves, row = _slow_rounds(A[b], s0, ms, mr, kinds)
                        what = (family, nc, rule, ms, mr, kinds, b)
                        assert rq[b].tolist() == row, what
                        np.testing.assert_array_equal(g[b], _canon(slot), str(what))
                        assert ut[b, metrics.RF_MOVES] == moves, what
                        assert ut[b, metrics.UT_GROUPS] == g[b].max() + 1
                        assert 1 <= rq[b, metrics.RM_Q_ROUNDS] <= mr
                        assert 1 <= rq[b, metrics.RF_Q_SWEEPS] <= ms
                    split_somewhere += int(rq[:, SPLITS].sum())
    if nc >= 7:
        assert split_somewhere > 0                   # the split sweep did act on this family


# ---------------------------------------------------------------------------------------
# the consequences (A) to (D)
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_consequences_a_to_d(family):
    nc, B = 33, 2
    y, p1 = FAMILIES[family](nc, seed=1200)
    label, probs = _onehot(y), _probs(p1)
    start = np.random.default_rng(3).integers(0, 9, (B, nc))
    for rule in RULES:
        gains = [metrics.refine_gains(probs[b, 1], tprime(0.5, rule), rule)[0] for b in range(B)]
        for st in (None, start, np.zeros((B, nc), np.int64)):
            for ms, mr in ((1, 1), (2, 2), (8, 4), (64, 16)):
                ut0, g0, rq0 = metrics.refine(label, probs, st, 0.5, rule, ms)
                merged = metrics.refine_merge(label, probs, st, 0.5, rule, ms, mr)
                as_merge = metrics.refine_split(label, probs, st, 0.5, rule, ms, mr, 1)
                for a, c in zip(as_merge, merged):                                     # (A)
                    np.testing.assert_array_equal(a, c)
                assert (merged[2][:, SPLITS] == 0).all()
                for kinds in (1, 2, 3):
                    ut, g, rq = metrics.refine_split(label, probs, st, 0.5, rule, ms, mr, kinds)
                    np.testing.assert_array_equal(rq[:, metrics.RM_Q_NODE],
                                                  rq0[:, metrics.RF_Q_END])            # (B)
                    np.testing.assert_array_equal(rq[:, metrics.RF_Q_START],
                                                  rq0[:, metrics.RF_Q_START])
                    assert (rq[:, metrics.RF_Q_END] - rq[:, metrics.RM_Q_NODE]
                            >= rq[:, metrics.RM_Q_MERGES] + rq[:, SPLITS]).all()       # (C)
                    for b in range(B):                                                 # (D)
                        assert rq[b, metrics.RF_Q_END] == _objective(gains[b], g[b])
                    if not kinds & metrics.RS_SPLIT:
                        assert (rq[:, SPLITS] == 0).all()
                    if not kinds & metrics.RS_MERGE:
                        assert (rq[:, metrics.RM_Q_MERGES] == 0).all()


def test_noisy_components_start_splits_and_never_lowers_q():
    """noisy_planted(74, ..) from the link graph's components at 0.55: the input the GPU test
    names for "the split sweeps did act"."""
    y, p1 = noisy_planted(74, seed=5, B=4, k=8)
    label, probs = _onehot(y), _probs(p1)
    start = metrics.untangle_counts(label, probs, 0.55, "mean")[1]
    _, _, rqm = metrics.refine_merge(label, probs, start, 0.55, "mean", 8, 4)
    _, _, rq = metrics.refine_split(label, probs, start, 0.55, "mean", 8, 4, 3)
    print("merge", rqm.tolist(), "merge + split", rq.tolist())
    assert rq[:, SPLITS].sum() > 0
    assert (rq[:, metrics.RF_Q_END] >= rqm[:, metrics.RF_Q_END]).all()
    assert rq[:, metrics.RF_Q_END].sum() > rqm[:, metrics.RF_Q_END].sum()


# ---------------------------------------------------------------------------------------
# a split gain past int32
# ---------------------------------------------------------------------------------------
def test_a_split_gain_past_int32():
    y, p1, start = big_split()
    label, probs = _onehot(y), _probs(p1)
    ut0, g0, rq0 = metrics.refine(label, probs, start, 0.5, "mean", 8)
    assert ut0[0, metrics.RF_MOVES] == 0 and rq0[0, metrics.RF_Q_CONVERGED] == 1
    assert rq0[0].tolist() == [BIG_Q_START, BIG_Q_START, 1, 1]
    parity = (np.arange(BIG_NC) % 2).astype(np.int32)[None]
    for kinds in (2, 3):
        ut, g, rq = metrics.refine_split(label, probs, start, 0.5, "mean", 8, 4, kinds)
        gain = int(rq[0, metrics.RF_Q_END] - rq[0, metrics.RM_Q_NODE])
        assert BIG_SPLIT_GAIN > 2 ** 31 and gain == BIG_SPLIT_GAIN == 66 * 66 * 498074
        assert rq[0].tolist() == [BIG_Q_START, BIG_Q_END, 2, 1, 2, 0, BIG_Q_START, 1]
        assert (BIG_Q_START, BIG_Q_END) == (79585176, 2249195520)
        np.testing.assert_array_equal(g, parity)         # the seeds are (0, 1): side E is odd
        assert ut[0, metrics.UT_GROUPS] == 2 and ut[0, metrics.RF_MOVES] == 0


# ---------------------------------------------------------------------------------------
# hand-made cases of the sweep's rules
# ---------------------------------------------------------------------------------------
def _scores(nc, w):
    """Symmetric scores s with s_pq + s_qp = w[p][q] -> (labels, scores) of one commit."""
    I, J = data.pair_index(nc)
    p1 = (np.asarray(w, np.float64)[I, J] / 2).astype(np.float32)[None]
    return np.zeros_like(p1, dtype=np.uint8), p1


def test_a_group_without_a_negative_pair_is_never_touched():
    # X = {0, 1, 2}: gains 0, +, + (the smallest is exactly 0); Y = {3, 4} + {5, 6} fused
    nc = 7
    w = np.full((nc, nc), 0.2)                       # across X and Y: far below the bound 1.0
    w[:3, :3] = 1.2
    w[0, 1] = w[1, 0] = 1.0                          # exactly on the bound: gain 0
    w[3:, 3:] = 0.7
    for a, b in ((3, 4), (5, 6)):
        w[a, b] = w[b, a] = 2.0
    y, p1 = _scores(nc, w)
    label, probs = _onehot(y), _probs(p1)
    A = metrics.refine_gains(probs[0, 1], tprime(0.5, "mean"))[0]
    assert A[0, 1] == 0 and (A[:3, :3] >= 0).all() and A[3, 5] < 0
    start = np.array([[0, 0, 0, 1, 1, 1, 1]])
    slot, size = np.array([0, 0, 0, 3, 3, 3, 3]), np.array([3, 0, 0, 4, 0, 0, 0])
    assert metrics._split_sweep(A, slot, size) == (1, -int(A[3:5, 5:].sum()))
    assert slot.tolist() == [0, 0, 0, 3, 3, 1, 1] and size.tolist() == [3, 2, 0, 2, 0, 0, 0]
    for kinds in (2, 3):
        ut, g, rq = metrics.refine_split(label, probs, start, 0.5, "mean", 8, 4, kinds)
        assert g[0].tolist() == [0, 0, 0, 1, 1, 2, 2]
        assert rq[0, SPLITS] == 1 and ut[0, metrics.RF_MOVES] == 0 and rq[0, metrics.RM_Q_MERGES] == 0
    # X alone: the sweep changes nothing at all
    slot, size = np.array([0, 0, 0, 3, 4, 5, 6]), np.array([3, 0, 0, 1, 1, 1, 1])
    assert metrics._split_sweep(A, slot, size) == (0, 0)
    assert slot.tolist() == [0, 0, 0, 3, 4, 5, 6] and size.tolist() == [3, 0, 0, 1, 1, 1, 1]


def test_a_slot_filled_by_a_split_waits_for_the_next_sweep():
    # three tight clusters in one group: a | b far apart, a | c far apart, b | c less so.  The
    # first visit cuts a from b + c, which lands in slot 1 -- itself worth cutting, but filled
    # by this sweep: one split per sweep, the second in the next round
    nc = 9
    w = np.full((nc, nc), 0.7)                       # a | b and a | c: gain -0.3
    w[3:6, 6:] = w[6:, 3:6] = 0.9                    # b | c: -0.1
    for k in (0, 3, 6):
        w[k:k + 3, k:k + 3] = 2.0                    # within: +1.0
    y, p1 = _scores(nc, w)
    label, probs = _onehot(y), _probs(p1)
    A = metrics.refine_gains(probs[0, 1], tprime(0.5, "mean"))[0]
    slot, size = np.zeros(nc, np.int64), np.bincount(np.zeros(nc, np.int64), minlength=nc)
    assert metrics._split_sweep(A, slot, size) == (1, -int(A[:3, 3:].sum()))
    assert slot.tolist() == [0] * 3 + [1] * 6 and size.tolist() == [3, 6] + [0] * 7
    assert metrics._split_sweep(A, slot, size) == (1, -int(A[3:6, 6:].sum()))
    assert slot.tolist() == [0] * 3 + [1] * 3 + [2] * 3
    start = np.zeros((1, nc), np.int64)
    ut, g, rq = metrics.refine_split(label, probs, start, 0.5, "mean", 8, 1, 2)
    assert g[0].tolist() == [0] * 3 + [1] * 6 and rq[0, SPLITS] == 1
    assert rq[0, metrics.RF_Q_CONVERGED] == 0 and rq[0, metrics.RM_Q_ROUNDS] == 1
    ut, g, rq = metrics.refine_split(label, probs, start, 0.5, "mean", 8, 4, 2)
    assert g[0].tolist() == [0] * 3 + [1] * 3 + [2] * 3 and ut[0, metrics.RF_MOVES] == 0
    assert rq[0, 2:].tolist() == [3, 1, 3, 0, rq[0, 0], 2]


def test_refine_merge_is_what_it_was_and_errors():
    y, p1 = FAMILIES["noisy"](9, seed=1)
    label, probs = _onehot(y), _probs(p1)
    assert metrics.refine_merge(label, probs, None)[2].shape == (2, metrics.RM_Q_SLOTS)
    assert inspect.signature(metrics.refine_split).parameters["kinds"].default == 3
    assert inspect.signature(metrics.refine_split).parameters["max_rounds"].default == 4
    for kinds in (0, 4, -1, None, "both"):
        with pytest.raises(ValueError):
            metrics.refine_split(label, probs, None, 0.5, "mean", 8, 4, kinds)
    for kw in (dict(max_rounds=0), dict(max_rounds=17), dict(max_rounds=None),
               dict(threshold=float("nan")), dict(rule="most"), dict(max_sweeps=0),
               dict(max_sweeps=65)):
        with pytest.raises(ValueError):
            metrics.refine_split(label, probs, None, **kw)
    with pytest.raises(ValueError):
        metrics.refine_split_ladder(label, probs, [])
    with pytest.raises(ValueError):
        metrics.refine_split_ladder(label, probs, [0.5], kinds=0)


# ---------------------------------------------------------------------------------------
# the ladder is the loop
# ---------------------------------------------------------------------------------------
def _loop(label, probs, thresholds, tree, rule, ms, mr, kinds):
    out = []
    for t in np.asarray(thresholds, np.float32):
        start = None if tree is None else metrics.cut_groups(tree[0], tree[1], tprime(t, rule))
        out.append(metrics.refine_split(label, probs, start, t, rule, ms, mr, kinds))
    return tuple(np.stack([o[i] for o in out]) for i in range(3))


@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_refine_split_ladder_is_the_loop(family):
    nc = 17
    y, p1 = FAMILIES[family](nc, seed=60 + nc)
    label, probs = _onehot(y), _probs(p1)
    k = 0
    for rule in RULES:
        trees = [None] + [metrics.agglomerate(label, probs, rule, m)[:2]
                          for m in ("single", "average")]
        for tree in trees:
            thr, ms, mr = LADDERS[k % len(LADDERS)], (1, 8)[k % 2], (1, 4, 16)[k % 3]
            kinds = (3, 2, 3, 1)[k % 4]
            k += 1
            got = metrics.refine_split_ladder(label, probs, thr, tree, rule, ms, mr, kinds)
            assert got[0].shape == (len(thr), 2, metrics.RF_SLOTS)
            assert got[1].shape == (len(thr), 2, nc) and got[1].dtype == np.int32
            assert got[2].shape == (len(thr), 2, metrics.RS_Q_SLOTS)
            for a, c in zip(got, _loop(label, probs, thr, tree, rule, ms, mr, kinds)):
                np.testing.assert_array_equal(a, c)
    # the merge ladder is what it was, and is the split ladder with kinds merge
    for a, c in zip(metrics.refine_merge_ladder(label, probs, [0.4, 0.6], trees[1], "both", 8, 2),
                    metrics.refine_split_ladder(label, probs, [0.4, 0.6], trees[1], "both", 8, 2, 1)):
        np.testing.assert_array_equal(a, c)
    # on the fused groups single linkage's tree gives the fused start at 0.5, and the rung cuts it
    y, p1, halves, fused = two_fused()
    label, probs = _onehot(y), _probs(p1)
    tree = metrics.agglomerate(label, probs, "mean", "single")[:2]
    ut, g, rq = metrics.refine_split_ladder(label, probs, [0.5], tree)
    np.testing.assert_array_equal(g[0], halves)
    assert (rq[0][:, SPLITS] == 3).all()


# ---------------------------------------------------------------------------------------
# mirrors, exports, the library's host-side checks
# ---------------------------------------------------------------------------------------
def test_python_mirrors_and_exports():
    with open(os.path.join(ROOT, "include", "hdgnn.h")) as f:
        txt = f.read()
    defs = dict(re.findall(r"#define\s+(HDG_RS_[A-Z_0-9]+)\s+(\d+)", txt))
    assert defs == {"HDG_RS_MERGE": "1", "HDG_RS_SPLIT": "2", "HDG_RS_PASSES": "4",
                    "HDG_RS_Q_SLOTS": "8", "HDG_RS_Q_SPLITS": "7"}
    for name, v in defs.items():
        assert getattr(_lib, name[4:]) == int(v), name
        assert getattr(metrics, name[4:]) == int(v), name
    declared = set(re.findall(r"\b(hdg_[a-z_0-9]+)\s*\(", txt))
    assert {"hdg_refine_split", "hdg_refine_split_ladder"} <= declared
    assert {"hdg_refine_split", "hdg_refine_split_ladder"} <= set(_lib.EXPORTS)
    assert "hdg_refine_split_workspace_bytes" not in declared      # no new sizing function
    assert _lib.ABI_VERSION == 9 and _lib.load().hdg_version() == 9
    assert _lib.RS_Q_SLOTS == _lib.RM_Q_SLOTS and _lib.RS_KINDS == KINDS


def test_library_argument_checks_on_the_host():
    lib = _lib.load()
    ok = _lib.Shape(4, 200, 74, 2, 4, 0)
    one = ctypes.c_void_p(64)                       # never dereferenced: the checks come first
    bt = _lib.Batch(None, None, one, None, None, None)
    args = dict(shape=ok, bt=bt, probs=one, thr=0.5, rule=0, ms=8, mr=4, kinds=3, flags=0,
                gin=None, groups=one, ut=one, rq=one, ws=one)

    def call(**kw):
        a = dict(args, **kw)
        return lib.hdg_refine_split(ctypes.byref(a["shape"]), ctypes.byref(a["bt"]), a["probs"],
                                    ctypes.c_float(a["thr"]), a["rule"], a["ms"], a["mr"],
                                    a["kinds"], a["flags"], a["gin"], a["groups"], a["ut"],
                                    a["rq"], a["ws"], None)

    einval = 1000
    nan, inf = float("nan"), float("inf")
    for kw, word in ((dict(kinds=0), b"kinds"), (dict(kinds=4), b"kinds"), (dict(kinds=-1), b"kinds"),
                     (dict(flags=1), b"flag"), (dict(flags=-1), b"flag"),
                     (dict(mr=0), b"max_rounds"), (dict(mr=17), b"max_rounds"),
                     (dict(rule=3), b"rule"), (dict(ms=0), b"max_sweeps"),
                     (dict(ms=65), b"max_sweeps"), (dict(thr=nan), b"finite"),
                     (dict(thr=inf), b"finite"), (dict(thr=2e38), b"finite"),
                     (dict(ws=ctypes.c_void_p(68)), b"aligned")):
        assert call(**kw) == einval and word in lib.hdg_last_error(), kw
        assert lib.hdg_last_error().startswith(b"hdg_refine_split:")
    for k in ("probs", "groups", "ut", "rq", "ws"):
        assert call(**{k: None}) == einval and b"NULL" in lib.hdg_last_error(), k
        assert lib.hdg_last_error().startswith(b"hdg_refine_split:")
    assert call(bt=_lib.Batch(None, None, None, None, None, None)) == einval
    assert call(shape=_lib.Shape(4, 200, 2049, 2, 4, 0)) == einval
    assert lib.hdg_last_error().startswith(b"hdg_refine_split: nc must be")

    largs = dict(shape=ok, bt=bt, probs=one, thr=[0.5, 0.25], n=None, rule=0, ms=8, mr=4, kinds=3,
                 flags=0, merges=one, levels=one, groups=one, ut=one, rq=one, ws=one)

    def lcall(**kw):
        a = dict(largs, **kw)
        thr = a["thr"]
        n = a["n"] if a["n"] is not None else len(thr)
        arr = None if thr is None else (ctypes.c_float * max(1, len(thr)))(*thr)
        return lib.hdg_refine_split_ladder(ctypes.byref(a["shape"]), ctypes.byref(a["bt"]),
                                           a["probs"], arr, n, a["rule"], a["ms"], a["mr"],
                                           a["kinds"], a["flags"], a["merges"], a["levels"],
                                           a["groups"], a["ut"], a["rq"], a["ws"], None)

    for kw, word in ((dict(kinds=0), b"kinds"), (dict(kinds=4), b"kinds"), (dict(flags=1), b"flag"),
                     (dict(flags=-1), b"flag"), (dict(mr=0), b"max_rounds"),
                     (dict(mr=17), b"max_rounds"), (dict(rule=3), b"rule"),
                     (dict(ms=0), b"max_sweeps"), (dict(n=0), b"n_rungs"),
                     (dict(thr=[0.5] * 65), b"n_rungs"), (dict(thr=None, n=2), b"thresholds"),
                     (dict(thr=[0.5, inf]), b"rung 1"), (dict(levels=None), b"merges and levels"),
                     (dict(merges=None), b"merges and levels"),
                     (dict(ws=ctypes.c_void_p(68)), b"aligned")):
        assert lcall(**kw) == einval and word in lib.hdg_last_error(), (kw, lib.hdg_last_error())
        assert lib.hdg_last_error().startswith(b"hdg_refine_split_ladder:")
    for k in ("probs", "ut", "rq", "ws"):
        assert lcall(**{k: None}) == einval and b"NULL" in lib.hdg_last_error(), k
        assert lib.hdg_last_error().startswith(b"hdg_refine_split_ladder:")
    assert lcall(shape=_lib.Shape(4, 200, 2049, 2, 4, 0)) == einval
    assert lib.hdg_last_error().startswith(b"hdg_refine_split_ladder: nc must be")
    # the four earlier calls keep rejecting every flag bit under their own names
    assert lib.hdg_refine(ctypes.byref(ok), ctypes.byref(bt), one, ctypes.c_float(0.5), 0, 8, 2,
                          None, one, one, one, one, None) == einval
    assert lib.hdg_last_error().startswith(b"hdg_refine: unknown flag")
    assert lib.hdg_refine_merge(ctypes.byref(ok), ctypes.byref(bt), one, ctypes.c_float(0.5), 0, 8,
                                4, 2, None, one, one, one, one, None) == einval
    assert lib.hdg_last_error().startswith(b"hdg_refine_merge: unknown flag")
    arr = (ctypes.c_float * 2)(0.5, 0.25)
    assert lib.hdg_refine_ladder(ctypes.byref(ok), ctypes.byref(bt), one, arr, 2, 0, 8, 2, one,
                                 one, one, one, one, one, None) == einval
    assert lib.hdg_last_error().startswith(b"hdg_refine_ladder: unknown flag")
    assert lib.hdg_refine_merge_ladder(ctypes.byref(ok), ctypes.byref(bt), one, arr, 2, 0, 8, 4, 2,
                                       one, one, one, one, one, one, None) == einval
    assert lib.hdg_last_error().startswith(b"hdg_refine_merge_ladder: unknown flag")


# ---------------------------------------------------------------------------------------
# model.py's arguments and main.py --link-split (a recorder)
# ---------------------------------------------------------------------------------------
def test_model_arguments():
    from hdgnn.model import graph2graph
    for fn in (graph2graph.untangle, graph2graph.calibrate_refined):
        par = inspect.signature(fn).parameters
        assert par["split"].default is False and par["merge"].default == 0
    graph2graph._check_split(False, 0)
    graph2graph._check_split(True, 1)
    for split, merge in ((True, 0), (1, 4), ("yes", 4), (None, 4)):
        with pytest.raises(ValueError):
            graph2graph._check_split(split, merge)


def test_main_link_split(tmp_path):
    import importlib.util
    spec = importlib.util.spec_from_file_location("hdg_main_rs",
                                                  os.path.join(ROOT, "hd-gnn_amd", "main.py"))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    runs = _runs(cli, ["--Type", "untangle", "--link-threshold", "refined", "--link-refine", "8",
                       "--link-merge", "3", "--link-split"], tmp_path)
    want = []
    for s in cli.STEPS:
        want += [("calibrate_refined", s, "train", "mean", "f1",
                  {"refine": 8, "ladder": DEFAULT_LADDER, "merge": 3, "split": True}),
                 ("untangle", s, "test", 0.0625 * s, "mean",
                  {"refine": 8, "merge": 3, "split": True})]
    assert runs == want
    assert _runs(cli, ["--Type", "calibrate", "--link-threshold", "refined", "--link-refine", "2",
                       "--link-merge", "16", "--link-split", "--link-method", "average"],
                 tmp_path) == \
        [("calibrate_refined", s, "train", "mean", "f1",
          {"refine": 2, "ladder": DEFAULT_LADDER, "method": "average", "merge": 16, "split": True})
         for s in cli.STEPS]
    assert _runs(cli, ["--Type", "untangle", "--link-refine", "4", "--link-merge", "1",
                       "--link-split"], tmp_path) == \
        [("untangle", s, "test", 0.5, "mean", {"refine": 4, "merge": 1, "split": True})
         for s in cli.STEPS]
    # without the flag the calls are exactly today's
    assert _runs(cli, ["--Type", "untangle", "--link-refine", "4", "--link-merge", "1"],
                 tmp_path) == [("untangle", s, "test", 0.5, "mean", {"refine": 4, "merge": 1})
                               for s in cli.STEPS]
    assert _runs(cli, ["--Type", "untangle", "--link-refine", "8"], tmp_path) == \
        [("untangle", s, "test", 0.5, "mean", {"refine": 8}) for s in cli.STEPS]
    assert _runs(cli, ["--Type", "untangle"], tmp_path) == \
        [("untangle", s, "test", 0.5, "mean", {}) for s in cli.STEPS]
    assert _runs(cli, ["--Type", "calibrate"], tmp_path) == \
        [("calibrate", s, "train", "mean", "f1", {}) for s in cli.STEPS]
    # splitting happens in the rounds: it needs --link-merge R >= 1 (and that, --link-refine)
    for argv in (["--link-split"], ["--link-split", "--link-refine", "8"],
                 ["--link-split", "--link-refine", "8", "--link-merge", "0"],
                 ["--link-split", "--link-merge", "3"],
                 ["--link-split", "yes", "--link-refine", "8", "--link-merge", "3"]):
        for typ in ("untangle", "calibrate"):
            with pytest.raises(SystemExit):
                cli.main(["--Type", typ] + argv + ["--checkpoint_dir", str(tmp_path)],
                         model_cls=_Recorder)
