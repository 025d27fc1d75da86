"""The refinement ladder on the host (CPU): hdgnn.metrics.refine_ladder, the restatement
hdg_refine_ladder is compared with on the GPU, against the loop it stands for; best_rung's
choice; ladder()'s rungs; the family that motivates the call, pinned by computation; the
Python mirror of HDG_RL_*; the host-side argument checks of hdg_refine_ladder; and main.py's
--link-threshold refined / --link-ladder against a recorder.  Every comparison of results is
integer equality.
"""
import ctypes
import os
import re

import numpy as np
import pytest

from _ladder import DEFAULT_LADDER, LADDERS, loop, motivating_family
from conftest import ROOT
from hdgnn import _lib, metrics
from test_refine import _onehot, _probs, grid, noisy_planted, uniform

RULES = ("mean", "any", "both")


# ---------------------------------------------------------------------------------------
# refine_ladder is the loop
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", (noisy_planted, uniform, grid))
def test_refine_ladder_is_the_loop_over_cut_groups_and_refine(family):
    nc = 17
    y, p1 = family(nc, seed=40 + nc)
    label, probs = _onehot(y), _probs(p1)
    k = 0
    for rule in RULES:
        trees = [None] + [metrics.agglomerate(label, probs, rule, m)[:2]
                          for m in ("single", "average")]
        for tree in trees:
            thr, ms = LADDERS[k % len(LADDERS)], (1, 8)[k % 2]
            k += 1
            got = metrics.refine_ladder(label, probs, thr, tree, rule, ms)
            want = loop(label, probs, thr, tree, rule, ms)
            assert got[0].shape == (len(thr), 2, metrics.RF_SLOTS)
            assert got[1].shape == (len(thr), 2, nc) and got[1].dtype == np.int32
            assert got[2].shape == (len(thr), 2, metrics.RF_Q_SLOTS)
            for a, c in zip(got, want):
                np.testing.assert_array_equal(a, c)
            if tree is None:
                assert (got[2][..., metrics.RF_Q_START] == 0).all()
    # equal rungs give equal rows; a rung is what refine gives alone
    ut, g, rq = metrics.refine_ladder(label, probs, [0.4, 0.4], None, "mean", 8)
    np.testing.assert_array_equal(ut[0], ut[1])
    np.testing.assert_array_equal(g[0], g[1])
    one = metrics.refine(label, probs, None, 0.4, "mean", 8)
    for a, c in zip((ut[1], g[1], rq[1]), one):
        np.testing.assert_array_equal(a, c)


def test_refine_ladder_errors():
    y, p1 = uniform(5, 1)
    label, probs = _onehot(y), _probs(p1)
    for thr in ([], [0.5] * 65, [0.5, float("nan")], [float("inf")]):
        with pytest.raises(ValueError):
            metrics.refine_ladder(label, probs, thr)
    with pytest.raises(ValueError):
        metrics.refine_ladder(label, probs, [0.5], rule="most")
    with pytest.raises(ValueError):
        metrics.refine_ladder(label, probs, [0.5], max_sweeps=0)
    metrics.refine_ladder(label, probs, [0.5] * 64, max_sweeps=1)


# ---------------------------------------------------------------------------------------
# best_rung
# ---------------------------------------------------------------------------------------
def _table(rows):
    """Per rung one commit with the given (SS, SD, DS, DD)."""
    ut = np.zeros((len(rows), 1, metrics.RF_SLOTS), np.int64)
    for k, (ss, sd, ds, dd) in enumerate(rows):
        ut[k, 0, [metrics.UT_SS, metrics.UT_SD, metrics.UT_DS, metrics.UT_DD]] = ss, sd, ds, dd
    return ut


def test_best_rung():
    thr = [0.2, 0.4, 0.6, 0.8]
    # f1: 0.5, 0.8, 0.8, nan -> the tie goes to the lower index
    ut = _table([(1, 1, 1, 3), (4, 1, 1, 0), (4, 2, 0, 0), (0, 0, 0, 6)])
    i, t, s, vals = metrics.best_rung(ut, thr)
    assert (i, t) == (1, float(np.float32(0.4))) and s == 0.8
    np.testing.assert_array_equal(vals[:3], [0.5, 0.8, 0.8])
    assert np.isnan(vals[3]) and vals.dtype == np.float64
    # a nan never wins, even first
    i, t, s, _ = metrics.best_rung(ut[::-1], thr)
    assert i == 1 and s == 0.8
    # rand is defined where f1 is not: all pairs apart, all truly apart
    i, t, s, vals = metrics.best_rung(ut, thr, "rand")
    assert i == 3 and s == 1.0
    # all nan: index 0 with nan
    i, t, s, vals = metrics.best_rung(_table([(0, 0, 0, 6)] * 3), thr[:3])
    assert i == 0 and t == float(np.float32(0.2)) and np.isnan(s) and np.isnan(vals).all()
    # pooled over the commits of a rung, not averaged
    two = np.concatenate([_table([(1, 0, 0, 0), (1, 0, 0, 0)]), _table([(0, 9, 0, 0), (0, 0, 0, 1)])], 1)
    assert metrics.best_rung(two, [0.1, 0.2])[3].tolist() == [2 / 11, 1.0]
    for bad in (dict(score="auc"), dict(thresholds=thr[:3])):
        with pytest.raises(ValueError):
            metrics.best_rung(ut, **dict(dict(thresholds=thr), **bad))


# ---------------------------------------------------------------------------------------
# ladder()
# ---------------------------------------------------------------------------------------
def test_ladder():
    L = metrics.ladder(*DEFAULT_LADDER)
    assert L.dtype == np.float32 and L.shape == (19,)
    want = [np.float32(0.05 + (0.95 - 0.05) * k / 18) for k in range(19)]      # float64, rounded once
    np.testing.assert_array_equal(L, np.array(want, np.float32))
    assert L[0] == np.float32(0.05) and L[18] == np.float32(0.95) and L[8] == np.float32(0.45)
    np.testing.assert_array_equal(metrics.ladder(0.3, 0.9, 1), np.array([0.3], np.float32))
    np.testing.assert_array_equal(metrics.ladder(1.0, -1.0, 3), np.array([1, 0, -1], np.float32))
    assert len(metrics.ladder(0, 1, 64)) == 64
    for bad in ((0, 1, 0), (0, 1, 65), (0, 1, -1), (0, 1, 2.0), (float("nan"), 1, 3),
                (0, float("inf"), 3), (float("-inf"), 0, 1)):
        with pytest.raises(ValueError):
            metrics.ladder(*bad)


# ---------------------------------------------------------------------------------------
# the motivating family: the tree's best threshold is the wrong one for the objective
# ---------------------------------------------------------------------------------------
def test_the_trees_best_threshold_is_not_the_refined_one():
    y, p1 = motivating_family()
    label, probs = _onehot(y), _probs(p1)
    m, lv, cv, _, lk = metrics.linkage(label, probs, "mean")
    thr, tree_f1, tp = metrics.best_threshold(lv, cv, lk, "mean", "f1")
    at_tree = metrics.refine(label, probs, metrics.cut_groups(m, lv, np.float32(tp)), thr, "mean", 8)
    f1_at_tree = metrics.scores_from_untangle(at_tree[0])["f1"]
    rungs = metrics.ladder(*DEFAULT_LADDER)
    ut, g, rq = metrics.refine_ladder(label, probs, rungs, (m, lv), "mean", 8)
    k, best_thr, f1, vals = metrics.best_rung(ut, rungs, "f1")
    print("tree", thr, tree_f1, "refined there", f1_at_tree, "best rung", k, best_thr, f1)
    assert f1_at_tree < tree_f1 < f1
    assert k == 8 and best_thr == float(np.float32(0.45)) and f1 == 1.0
    assert (ut[8][:, metrics.UT_SD] == 0).all() and (ut[8][:, metrics.UT_DS] == 0).all()


# ---------------------------------------------------------------------------------------
# mirrors, the header, the library's host-side checks
# ---------------------------------------------------------------------------------------
def test_python_mirror_and_declarations():
    with open(os.path.join(ROOT, "include", "hdgnn.h")) as f:
        txt = f.read()
    defs = dict(re.findall(r"#define\s+(HDG_RL_[A-Z_0-9]+)\s+(\d+)", txt))
    assert defs == {"HDG_RL_MAX_RUNGS": "64"}
    assert _lib.RL_MAX_RUNGS == metrics.RL_MAX_RUNGS == int(defs["HDG_RL_MAX_RUNGS"])
    declared = set(re.findall(r"\b(hdg_[a-z_0-9]+)\s*\(", txt))
    assert {"hdg_refine_ladder", "hdg_refine_ladder_workspace_bytes"} <= declared
    assert {"hdg_refine_ladder", "hdg_refine_ladder_workspace_bytes"} <= set(_lib.EXPORTS)
    assert _lib.ABI_VERSION == 9


def test_library_argument_checks_on_the_host():
    lib = _lib.load()
    ok = _lib.Shape(4, 200, 74, 2, 4, 0)
    for b, nc in ((1, 2), (3, 64), (4, 74), (2, 2048)):
        s = _lib.Shape(b, 2, nc, 2, b, 0)
        assert lib.hdg_refine_ladder_workspace_bytes(ctypes.byref(s), 0) == \
            lib.hdg_refine_workspace_bytes(ctypes.byref(s), 0) > 0
    for b, nc in ((0, 74), (65536, 74), (4, 1), (4, 2049)):
        s = _lib.Shape(b, 200, nc, 2, 4, 0)
        assert lib.hdg_refine_ladder_workspace_bytes(ctypes.byref(s), 0) == 0
        assert lib.hdg_last_error().startswith(b"hdg_refine_ladder_workspace_bytes:")
    one = ctypes.c_void_p(64)                       # never dereferenced: the checks come first
    bt = _lib.Batch(None, None, one, None, None, None)
    args = dict(shape=ok, bt=bt, probs=one, thr=[0.5, 0.25], n=None, rule=0, ms=8, flags=0,
                merges=one, levels=one, groups=one, ut=one, rq=one, ws=one)

    def call(**kw):
        a = dict(args, **kw)
        thr = a["thr"]
        n = a["n"] if a["n"] is not None else len(thr)
        arr = None if thr is None else (ctypes.c_float * max(1, len(thr)))(*thr)
        return lib.hdg_refine_ladder(ctypes.byref(a["shape"]), ctypes.byref(a["bt"]), a["probs"],
                                     arr, n, a["rule"], a["ms"], a["flags"], a["merges"],
                                     a["levels"], a["groups"], a["ut"], a["rq"], a["ws"], None)

    einval = 1000
    nan, inf = float("nan"), float("inf")
    for kw, word in ((dict(rule=3), b"rule"), (dict(rule=-1), b"rule"), (dict(ms=0), b"max_sweeps"),
                     (dict(ms=65), b"max_sweeps"), (dict(flags=1), b"flag"),
                     (dict(flags=-1), b"flag"), (dict(n=0), b"n_rungs"), (dict(n=-1), b"n_rungs"),
                     (dict(thr=[0.5] * 65), b"n_rungs"), (dict(thr=None, n=2), b"thresholds"),
                     (dict(thr=[nan]), b"rung 0"), (dict(thr=[0.5, inf]), b"rung 1"),
                     (dict(thr=[0.1, 0.2, 0.3, nan, 0.5]), b"rung 3"),
                     (dict(thr=[0.5, 0.5, 2e38]), b"rung 2"), (dict(thr=[-inf], rule=1), b"rung 0"),
                     (dict(levels=None), b"merges and levels"),
                     (dict(merges=None), b"merges and levels"),
                     (dict(ws=ctypes.c_void_p(68)), b"aligned")):
        assert call(**kw) == einval and word in lib.hdg_last_error(), (kw, lib.hdg_last_error())
        assert lib.hdg_last_error().startswith(b"hdg_refine_ladder:")
    for k in ("probs", "ut", "rq", "ws"):
        assert call(**{k: None}) == einval and b"NULL" in lib.hdg_last_error(), k
    assert call(bt=_lib.Batch(None, None, None, None, None, None)) == einval
    assert call(shape=_lib.Shape(0, 200, 74, 2, 1, 0)) == einval
    assert call(shape=_lib.Shape(4, 200, 2049, 2, 4, 0)) == einval
    assert lib.hdg_last_error().startswith(b"hdg_refine_ladder: nc must be")
    assert call(thr=[0.5, 0.5, 2e38], rule=1, ws=None) == einval      # 2e38 is finite under any
    assert b"NULL" in lib.hdg_last_error()


# ---------------------------------------------------------------------------------------
# main.py --link-threshold refined, --link-ladder (a recorder)
# ---------------------------------------------------------------------------------------
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


def test_main_link_threshold_refined(tmp_path):
    import importlib.util
    spec = importlib.util.spec_from_file_location("hdg_main_rl",
                                                  os.path.join(ROOT, "hd-gnn_amd", "main.py"))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    default = {"refine": 8, "ladder": DEFAULT_LADDER}
    runs = _runs(cli, ["--Type", "untangle", "--link-threshold", "refined", "--link-refine", "8"],
                 tmp_path)
    want = []
    for s in cli.STEPS:                             # its threshold is the one untangle refines at
        want += [("calibrate_refined", s, "train", "mean", "f1", default),
                 ("untangle", s, "test", 0.0625 * s, "mean", {"refine": 8})]
    assert runs == want
    runs = _runs(cli, ["--Type", "untangle", "--link-threshold", "refined", "--link-refine", "3",
                       "--link-method", "average", "--link-rule", "any", "--link-score", "rand",
                       "--link-ladder", "0.2:0.6:5"], tmp_path)
    want = []
    for s in cli.STEPS:
        want += [("calibrate_refined", s, "train", "any", "rand",
                  {"refine": 3, "ladder": (0.2, 0.6, 5), "method": "average"}),
                 ("untangle", s, "test", 0.0625 * s, "any", {"method": "average", "refine": 3})]
    assert runs == want
    assert _runs(cli, ["--Type", "calibrate", "--link-threshold", "refined", "--link-refine", "8",
                       "--link-ladder=-1:1:1"], tmp_path) == \
        [("calibrate_refined", s, "train", "mean", "f1", {"refine": 8, "ladder": (-1.0, 1.0, 1)})
         for s in cli.STEPS]
    # every earlier invocation makes the calls it made: --link-ladder alone changes nothing
    assert _runs(cli, ["--Type", "calibrate", "--link-refine", "8", "--link-ladder", "0:1:3"],
                 tmp_path) == [("calibrate", s, "train", "mean", "f1", {}) for s in cli.STEPS]
    assert _runs(cli, ["--Type", "untangle", "--link-threshold", "auto"], tmp_path) == \
        [x for s in cli.STEPS for x in (("calibrate", s, "train", "mean", "f1", {}),
                                        ("untangle", s, "test", 0.125 * s, "mean", {}))]
    assert _runs(cli, ["--Type", "untangle"], tmp_path) == \
        [("untangle", s, "test", 0.5, "mean", {}) for s in cli.STEPS]
    # refined needs sweeps to refine with; a ladder needs LO:HI:N
    for argv in (["--link-threshold", "refined"],
                 ["--link-threshold", "refined", "--link-refine", "0"],
                 ["--link-threshold", "refined", "--link-refine", "8", "--link-ladder", "0.1:0.9"],
                 ["--link-threshold", "refined", "--link-refine", "8", "--link-ladder", "0:1:65"],
                 ["--link-threshold", "refined", "--link-refine", "8", "--link-ladder", "0:x:3"],
                 ["--link-threshold", "refined", "--link-refine", "8", "--link-ladder", "0:inf:3"]):
        for typ in ("untangle", "calibrate"):
            with pytest.raises(SystemExit):
                cli.main(["--Type", typ] + argv + ["--checkpoint_dir", str(tmp_path)],
                         model_cls=_Recorder)
    assert cli._ladder("0.05:0.95:19") == DEFAULT_LADDER
    np.testing.assert_array_equal(metrics.ladder(*cli._ladder("0.05:0.95:19")),
                                  metrics.ladder(*DEFAULT_LADDER))
