"""hdg_match's host side: the integer assignment solver of hdgnn.metrics against brute force
(and scipy where it is installed), the planted fixtures of _match.py, the header's
consequences, the certificate of `mate`, renumbering, the scores, the CLI, and the library's
argument checks on the host.  No GPU.
"""
import ctypes
import itertools
import os
import re
import types

import numpy as np
import pytest

from _match import (PLANTED, check_consequences, check_mate, noisy_sets, relabeled_truth,
                    renumbered, table_of, wild_ids)
from conftest import ROOT
from hdgnn import _lib, metrics
from test_refine import FAMILIES, _onehot, _probs, noisy_planted

MATCHED, PURITY, COVER = _lib.MT_MATCHED, _lib.MT_PURITY, _lib.MT_COVER


def _brute(a):
    a = a if a.shape[0] <= a.shape[1] else a.T
    K, M = a.shape
    return max(sum(int(a[i, p[i]]) for i in range(K)) for p in itertools.permutations(range(M), K))


def _check_assignment(a, value, col):
    K, M = a.shape
    hit = col >= 0
    assert hit.sum() == min(K, M) and len(set(col[hit])) == hit.sum()
    assert ((col[hit] >= 0) & (col[hit] < M)).all()
    assert value == int(a[np.flatnonzero(hit), col[hit]].sum())


def test_solver_against_brute_force():
    rng = np.random.default_rng(0)
    shapes = set()
    for k in range(300):
        K, M = (int(x) for x in rng.integers(1, 7, 2))
        a = rng.integers(0, int(rng.integers(1, 9)), (K, M))
        if k % 5 == 0:
            a[rng.random((K, M)) < 0.5] = 0                       # sparse: many ties at 0
        value, col = metrics.assign_max(a)
        assert value == _brute(a), a
        _check_assignment(a, value, col)
        shapes.add((K, M))
    assert {(6, 6), (1, 6), (6, 1), (2, 5), (5, 2)} <= shapes
    assert metrics.assign_max(np.zeros((0, 3), np.int64))[0] == 0
    assert metrics.assign_max(np.zeros((3, 0), np.int64))[0] == 0
    for bad in (np.zeros((2, 2)), np.zeros(3, np.int64), -np.ones((2, 2), np.int64)):
        with pytest.raises(ValueError):
            metrics.assign_max(bad)


def test_solver_against_scipy():
    opt = pytest.importorskip("scipy.optimize")
    rng = np.random.default_rng(1)
    for K, M, top in ((129, 129, 5), (129, 64, 9), (40, 129, 3), (77, 77, 2), (100, 100, 2048)):
        a = rng.integers(0, top, (K, M))
        a[rng.random((K, M)) < 0.7] = 0
        value, col = metrics.assign_max(a)
        r, c = opt.linear_sum_assignment(a, maximize=True)
        assert value == int(a[r, c].sum()), (K, M)
        _check_assignment(a, value, col)
    for name, make in PLANTED.items():                            # the planted numbers, again
        y, g, planted = make()
        gd, td = g[0], metrics.match_counts(_onehot(y), g)[2][0]
        table = np.zeros((gd.max() + 1, td.max() + 1), np.int64)
        np.add.at(table, (gd, td), 1)
        r, c = opt.linear_sum_assignment(table, maximize=True)
        assert int(table[r, c].sum()) == planted[MATCHED], name


def _independent(groups, tg, mt):
    """MATCHED of every row against solvers that share nothing with match_counts' reduction: the
    full table from the definition (table_of), brute force over all permutations where it is at
    most 7 x 7, scipy where it is installed."""
    try:
        from scipy.optimize import linear_sum_assignment
    except ImportError:
        linear_sum_assignment = None
    for s, b in np.ndindex(groups.shape[:2]):
        table = table_of(groups[s, b], tg[b])
        if max(table.shape) <= 7:
            assert _brute(table) == mt[s, b, MATCHED], (s, b)
        if linear_sum_assignment is not None:
            r, c = linear_sum_assignment(table, maximize=True)
            assert int(table[r, c].sum()) == mt[s, b, MATCHED], (s, b)


@pytest.mark.parametrize("name", sorted(PLANTED))
def test_planted_values(name):
    y, g, planted = PLANTED[name]()
    mt, mate, tg = metrics.match_counts(_onehot(y), g)
    assert mt.shape == (1, 1, _lib.MT_SLOTS) and mt.dtype == np.int64
    assert mate.shape == (1,) + g.shape and mate.dtype == np.int32 and tg.dtype == np.int32
    for slot, value in planted.items():
        assert mt[0, 0, slot] == value, (name, slot, mt[0, 0])
    check_mate(mate, g[None], tg, mt)
    check_consequences(mt, g[None], tg)


def test_what_the_planted_fixtures_rule_out():
    """three_ways_wrong: greedy by largest cell, purity and cover all miss; the contender-last
    staircase: arg-max greedy per row misses by one cell."""
    y, g, planted = PLANTED["three_ways_wrong"]()
    mt = metrics.match_counts(_onehot(y), g)[0][0, 0]
    table = np.array([[3, 2], [2, 0]])
    assert mt[MATCHED] == 4 == table[0, 1] + table[1, 0] and table[0, 0] + table[1, 1] == 3
    assert mt[PURITY] == 5 != mt[MATCHED] and mt[COVER] == 5
    for K in (3, 32, 64):
        y, g, planted = PLANTED["staircase%d_last" % K]()
        tg = metrics.match_counts(_onehot(y), g)[2][0]
        table = np.zeros((K + 1, K + 1), np.int64)
        np.add.at(table, (g[0], tg), 1)
        taken, greedy = set(), 0
        for i in range(K + 1):                                    # rows in id order, first arg-max
            free = [c for c in range(K + 1) if c not in taken and table[i, c] > 0]
            if free:
                c = max(free, key=lambda c: (table[i, c], -c))
                taken.add(c)
                greedy += int(table[i, c])
        assert greedy == 2 * K and planted[MATCHED] == 2 * K + 2
        assert g.shape[-1] == 2 * (2 * K + 1)


@pytest.mark.parametrize("family", ["noisy", "uniform", "grid"])
@pytest.mark.parametrize("nc", [2, 3, 5, 6, 7, 33, 74, 130])
def test_consequences_certificate_and_renumbering(nc, family):
    y, p1 = FAMILIES[family](nc, seed=nc, B=3)
    label = _onehot(y)
    groups = noisy_sets(y, p1, seed=nc, n_sets=3)
    rng = np.random.default_rng(nc)
    for g in (groups, wild_ids(groups, rng)):
        mt, mate, tg = metrics.match_counts(label, g)
        check_consequences(mt, g, tg)
        check_mate(mate, g, tg, mt)
        np.testing.assert_array_equal(tg, metrics.untangle_counts(label, _probs(p1))[2])
        np.testing.assert_array_equal(metrics.match_counts(label, renumbered(g, rng))[0], mt)
        np.testing.assert_array_equal(metrics.match_counts(label, g[1])[0][0], mt[1])   # (B, nc)
        _independent(g, tg, mt)


def test_matched_all_iff_the_partitions_are_equal():
    nc = 33
    y, p1 = noisy_planted(nc, seed=4, B=4)
    label, probs = _onehot(y), _probs(p1)
    ut, g, tg = metrics.untangle_counts(label, probs, 0.5)
    rng = np.random.default_rng(4)
    sets = np.stack([g, tg, renumbered(tg[None], rng)[0], relabeled_truth(tg, rng)])
    mt = metrics.match_counts(label, sets)[0]
    assert (mt[1:3, :, MATCHED] == nc).all()
    for k in (1, 2):
        for slot in (_lib.MT_ISOLATED, _lib.MT_GROUPS, _lib.MT_TGROUPS):
            np.testing.assert_array_equal(mt[k, :, slot], mt[k, :, _lib.MT_CELLS])
    exact = (ut[:, _lib.UT_SD] == 0) & (ut[:, _lib.UT_DS] == 0)
    np.testing.assert_array_equal(mt[0, :, MATCHED] == nc, exact)
    for k in (0, 3):                                              # SD = DS = 0, by pair counts
        for b in range(4):
            same = np.array_equal(sets[k, b][:, None] == sets[k, b][None, :],
                                  tg[b][:, None] == tg[b][None, :])
            assert (mt[k, b, MATCHED] == nc) == same


def test_match_counts_errors():
    y, p1 = noisy_planted(5, seed=1, B=2)
    label = _onehot(y)
    g = np.zeros((2, 5), np.int32)
    for bad in (g[:1], g[:, :4], np.zeros((65, 2, 5), np.int32), np.zeros((0, 2, 5), np.int32),
                np.zeros(5, np.int32)):
        with pytest.raises(ValueError):
            metrics.match_counts(label, bad)
    with pytest.raises(ValueError):
        metrics.match_counts(label[:, :, :-1], g)
    assert metrics.match_counts(label, np.zeros((64, 2, 5), np.int32))[0].shape == (64, 2, 8)


def test_scores_from_match_and_best_rung_match():
    nc = 10
    mt = np.zeros((3, _lib.MT_SLOTS), np.int64)
    mt[:, _lib.MT_GROUPS], mt[:, _lib.MT_TGROUPS] = (2, 3, 4), (3, 3, 6)
    mt[:, MATCHED], mt[:, PURITY], mt[:, COVER] = (10, 5, 6), (10, 8, 7), (10, 6, 9)
    s = metrics.scores_from_match(mt, nc)
    assert s == {"accuracy": 21 / 30, "accuracy_mean": np.mean([1.0, 0.5, 0.6]),
                 "purity": 25 / 30, "cover": 25 / 30, "exact": 1 / 3, "groups_mean": 3.0,
                 "tgroups_mean": 4.0}
    empty = metrics.scores_from_match(np.zeros((0, _lib.MT_SLOTS), np.int64), nc)
    assert set(empty) == set(s) and all(np.isnan(v) for v in empty.values())
    with pytest.raises(ValueError):
        metrics.scores_from_match(mt, 0)
    lad = np.zeros((4, 2, _lib.MT_SLOTS), np.int64)
    lad[:, :, MATCHED] = ((3, 4), (5, 4), (4, 5), (1, 1))
    thr = [0.2, 0.4, 0.6, 0.8]
    k, t, best, vals = metrics.best_rung_match(lad, thr, nc)
    assert (k, t, best) == (1, float(np.float32(0.4)), 9 / 20)           # ties: the lowest index
    np.testing.assert_array_equal(vals, np.array([7, 9, 9, 2]) / 20)
    k, t, best, vals = metrics.best_rung_match(np.zeros((4, 0, _lib.MT_SLOTS), np.int64), thr, nc)
    assert k == 0 and t == float(np.float32(0.2)) and np.isnan(best) and np.isnan(vals).all()
    for bad in (lad[:3], lad[..., :7], lad[0]):
        with pytest.raises(ValueError):
            metrics.best_rung_match(bad, thr, nc)
    with pytest.raises(ValueError):
        metrics.best_rung_match(np.zeros((65, 1, 8), np.int64), [0.5] * 65, nc)
    # best_rung is what it was: "acc" is not one of its scores
    with pytest.raises(ValueError):
        metrics.best_rung(np.zeros((4, 2, 8), np.int64), thr, "acc")


def test_python_mirrors_match_the_header():
    with open(os.path.join(ROOT, "include", "hdgnn.h")) as f:
        defs = dict(re.findall(r"#define\s+(HDG_MT_[A-Z_0-9]+)\s+(\d+)", f.read()))
    assert sorted(defs) == ["HDG_MT_CELLS", "HDG_MT_COVER", "HDG_MT_GROUPS", "HDG_MT_ISOLATED",
                            "HDG_MT_MATCHED", "HDG_MT_MAX_SETS", "HDG_MT_PURITY", "HDG_MT_SLOTS",
                            "HDG_MT_TGROUPS"]
    for name, v in defs.items():
        assert getattr(_lib, name[4:]) == int(v), name
        assert getattr(metrics, name[4:]) == int(v), name
    assert _lib.MT_MAX_SETS == _lib.RL_MAX_RUNGS and _lib.ABI_VERSION == 9
    assert "match.hip" in __import__("hdgnn.build", fromlist=["SOURCES"]).SOURCES


def test_engine_match_argument_checks():
    """Engine.match checks `groups` and `mate` before anything else: no device is needed."""
    import torch
    from hdgnn.engine import Engine
    eng = Engine.__new__(Engine)
    eng.device, eng.batch, eng.nc = torch.device("cpu"), 3, 5
    ok = torch.zeros(2, 3, 5, dtype=torch.int32)
    g, S = eng._match_args(ok, False)
    assert S == 2 and g.data_ptr() == ok.data_ptr()
    g, S = eng._match_args(ok[0], True)
    assert S == 1 and tuple(g.shape) == (1, 3, 5)
    assert eng._match_args(torch.zeros(64, 3, 5, dtype=torch.int32), False)[1] == 64
    for bad in (ok.long(), ok[:, :2], ok[:, :, :4], ok.transpose(1, 2), ok.numpy(), None,
                torch.zeros(65, 3, 5, dtype=torch.int32), torch.zeros(0, 3, 5, dtype=torch.int32),
                torch.zeros(5, dtype=torch.int32), torch.zeros(1, 2, 3, 5, dtype=torch.int32)):
        with pytest.raises(ValueError, match="groups must be"):
            eng.match(None, bad)
    for bad in (1, None, "yes"):
        with pytest.raises(ValueError, match="mate must be"):
            eng.match(None, ok, mate=bad)


# ---------------------------------------------------------------------------------------
# graph2graph and the CLI
# ---------------------------------------------------------------------------------------
def test_calibrate_rejects_acc_and_untangle_checks_match():
    from hdgnn.model import graph2graph
    m = graph2graph.__new__(graph2graph)
    args = types.SimpleNamespace(Repo="tiny", checkpoint_dir=".")
    with pytest.raises(ValueError, match="calibrate_refined"):
        m.calibrate(args, score="acc")
    for bad in (1, None, "yes"):
        with pytest.raises(ValueError, match="match must be a bool"):
            m.untangle(args, match=bad)


class _Recorder:
    log = []

    def __init__(self, sess, **kw):
        assert sess is None

    def untangle(self, args, part="test", threshold=0.5, rule="mean", **kw):
        _Recorder.log.append(("untangle", args.Step, part, threshold, rule, kw))

    def calibrate(self, args, part="train", rule="mean", score="f1", **kw):
        _Recorder.log.append(("calibrate", args.Step, part, rule, score, kw))
        return 0.125 * args.Step, {}, None, None, None

    def calibrate_refined(self, args, part="train", rule="mean", score="f1", **kw):
        _Recorder.log.append(("calibrate_refined", args.Step, part, rule, score, kw))
        return 0.0625 * args.Step, {}, None, None, None


def _runs(cli, argv, tmp_path):
    _Recorder.log = []
    cli.main(argv + ["--checkpoint_dir", str(tmp_path)], model_cls=_Recorder)
    return _Recorder.log


def test_main_link_match_and_link_score_acc(tmp_path):
    import importlib.util
    spec = importlib.util.spec_from_file_location("hdg_main_mt",
                                                  os.path.join(ROOT, "hd-gnn_amd", "main.py"))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    ladder = (0.05, 0.95, 19)
    assert _runs(cli, ["--Type", "untangle", "--link-match"], tmp_path) == \
        [("untangle", s, "test", 0.5, "mean", {"match": True}) for s in cli.STEPS]
    runs = _runs(cli, ["--Type", "untangle", "--link-threshold", "refined", "--link-refine", "8",
                       "--link-score", "acc", "--link-match", "--link-merge", "2",
                       "--link-split"], tmp_path)
    want = []
    for s in cli.STEPS:
        want += [("calibrate_refined", s, "train", "mean", "acc",
                  {"refine": 8, "ladder": ladder, "merge": 2, "split": True}),
                 ("untangle", s, "test", 0.0625 * s, "mean",
                  {"refine": 8, "match": True, "merge": 2, "split": True})]
    assert runs == want
    assert _runs(cli, ["--Type", "calibrate", "--link-threshold", "refined", "--link-refine", "4",
                       "--link-score", "acc"], tmp_path) == \
        [("calibrate_refined", s, "train", "mean", "acc", {"refine": 4, "ladder": ladder})
         for s in cli.STEPS]
    # --link-match does not reach the calibration, and acc needs the ladder
    assert _runs(cli, ["--Type", "calibrate", "--link-match"], tmp_path) == \
        [("calibrate", s, "train", "mean", "f1", {}) for s in cli.STEPS]
    for bad in (["--link-score", "acc"], ["--link-score", "acc", "--link-threshold", "auto"],
                ["--link-score", "acc", "--link-threshold", "0.4"], ["--link-score", "auc"],
                ["--link-score", "acc", "--link-threshold", "refined"]):
        for kind in ("untangle", "calibrate"):
            with pytest.raises(SystemExit):
                cli.main(["--Type", kind, "--checkpoint_dir", str(tmp_path)] + bad,
                         model_cls=_Recorder)
    # without the new flags every invocation records exactly the old calls
    assert _runs(cli, ["--Type", "untangle"], tmp_path) == \
        [("untangle", s, "test", 0.5, "mean", {}) for s in cli.STEPS]
    runs = _runs(cli, ["--Type", "untangle", "--link-threshold", "refined", "--link-refine", "8"],
                 tmp_path)
    want = []
    for s in cli.STEPS:
        want += [("calibrate_refined", s, "train", "mean", "f1", {"refine": 8, "ladder": ladder}),
                 ("untangle", s, "test", 0.0625 * s, "mean", {"refine": 8})]
    assert runs == want
    assert _runs(cli, ["--Type", "untangle", "--link-threshold", "auto"], tmp_path)[:2] == \
        [("calibrate", 2, "train", "mean", "f1", {}), ("untangle", 2, "test", 0.25, "mean", {})]


# ---------------------------------------------------------------------------------------
# the library's checks on the host: nothing is launched
# ---------------------------------------------------------------------------------------
def test_library_argument_checks_on_the_host():
    lib = _lib.load()
    ok = _lib.Shape(4, 200, 74, 2, 4, 0)
    for b, nc, sets in ((1, 2, 1), (3, 65, 64), (4, 74, 19), (2, 2048, 1), (65535, 3, 2)):
        nbytes = lib.hdg_match_workspace_bytes(ctypes.byref(_lib.Shape(b, 2, nc, 2, b, 0)), sets)
        assert nbytes == -(-b * nc * 4 // 8) * 8
    for b, nc, sets in ((0, 74, 1), (65536, 74, 1), (4, 1, 1), (4, 2049, 1), (4, 74, 0),
                        (4, 74, 65), (4, 74, -1)):
        assert lib.hdg_match_workspace_bytes(ctypes.byref(_lib.Shape(b, 200, nc, 2, 4, 0)),
                                             sets) == 0
        assert b"must be in" in lib.hdg_last_error()
        assert lib.hdg_last_error().startswith(b"hdg_match_workspace_bytes:")
    one = ctypes.c_void_p(64)                       # never dereferenced: the checks come first
    bt = _lib.Batch(None, None, one, None, None, None)
    args = dict(shape=ok, bt=bt, groups=one, sets=3, mate=one, tg=one, mt=one, ws=one)

    def call(**kw):
        a = dict(args, **kw)
        return lib.hdg_match(ctypes.byref(a["shape"]), ctypes.byref(a["bt"]), a["groups"],
                             a["sets"], a["mate"], a["tg"], a["mt"], a["ws"], None)

    einval = 1000
    for kw, word in ((dict(sets=0), b"n_sets"), (dict(sets=65), b"n_sets"), (dict(sets=-2), b"n_sets"),
                     (dict(ws=ctypes.c_void_p(68)), b"aligned"),
                     (dict(shape=_lib.Shape(0, 200, 74, 2, 1, 0)), b"batch"),
                     (dict(shape=_lib.Shape(65536, 200, 74, 2, 1, 0)), b"batch"),
                     (dict(shape=_lib.Shape(4, 200, 1, 2, 4, 0)), b"nc must be"),
                     (dict(shape=_lib.Shape(4, 200, 2049, 2, 4, 0)), b"nc must be")):
        assert call(**kw) == einval and word in lib.hdg_last_error(), kw
        assert lib.hdg_last_error().startswith(b"hdg_match:"), kw
    for k in ("groups", "mt", "ws"):
        assert call(**{k: None}) == einval and b"NULL" in lib.hdg_last_error(), k
        assert lib.hdg_last_error().startswith(b"hdg_match:")
    assert call(bt=_lib.Batch(None, None, None, None, None, None)) == einval
    assert b"NULL" in lib.hdg_last_error() and lib.hdg_last_error().startswith(b"hdg_match:")
    assert lib.hdg_match(ctypes.byref(ok), None, one, 3, one, one, one, one, None) == einval   # batch
    assert b"NULL" in lib.hdg_last_error() and lib.hdg_last_error().startswith(b"hdg_match:")
