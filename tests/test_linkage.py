"""Linkage on the host (CPU): hdgnn.metrics.linkage (plain Kruskal) against brute force --
every reachable cut of the merge tree must be the partition and the counts
hdgnn.metrics.untangle_counts gives at that cut's threshold -- the edge order, -0, the
infinities, NaN pairs that disconnect a hunk, best_threshold against an evaluation of every
candidate, a planted case that 0.5 gets wrong and the calibrated threshold gets right, the
header constants against their Python mirrors, the host side of the C entry points, and
main.py --Type calibrate / --link-threshold auto through test_cli's recorder pattern.

Every comparison is integer or bit equality.
"""
import ctypes
import math
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from hdgnn import _lib, data, metrics

RULES = ("mean", "any", "both")


def _onehot(y):
    return np.stack([1 - y, y], 1).astype(np.float32)


def _probs(p1):
    return np.ascontiguousarray(np.stack([1.0 - p1, p1], 1), np.float32)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _grid_scores(rng, B, nc, nan=0.0):
    """Scores on a 1/8 grid (ties dominate), labels from three planted groups."""
    I, J = data.pair_index(nc)
    p1 = (rng.integers(0, 9, (B, len(I))) / 8.0).astype(np.float32)
    if nan:
        p1[rng.random(p1.shape) < nan] = np.nan
    gt = rng.integers(0, 3, (B, nc))
    y = ((gt[:, I] == gt[:, J]) & (rng.random((B, len(I))) < 0.6)).astype(np.uint8)
    return y, p1


def _cut_groups(nc, merges, k):
    """Dense ids (ordered by smallest member) of the merge tree cut after merges 0 .. k."""
    lab = list(range(nc))
    for p, q in merges[:k + 1]:
        a, c = lab[p], lab[q]
        assert a != c                                   # a forest: no merge inside a cluster
        lo, hi = min(a, c), max(a, c)
        lab = [lo if v == hi else v for v in lab]
    first = sorted(set(lab))
    return [first.index(v) for v in lab]


def _check_against_untangle(y, p1, rule, nan_scores_only=True):
    """Every reachable cut of every commit against untangle_counts at its threshold;
    -> the linkage.  nan_scores_only: no pair has a NaN weight from two non-NaN scores
    (inf + -inf under the mean rule), so LK_NAN is UT_NAN."""
    B, R = p1.shape
    nc = int(round((1 + math.sqrt(1 + 4 * R)) / 2))
    label, probs = _onehot(y), _probs(p1)
    merges, levels, curve, tgroups, lk = metrics.linkage(label, probs, rule)
    assert merges.dtype == np.int32 and merges.shape == (B, nc - 1, 2)
    assert levels.dtype == np.float32 and levels.shape == (B, nc - 1)
    assert curve.dtype == np.int64 and curve.shape == (B, nc - 1, 2)
    assert tgroups.dtype == np.int32 and lk.dtype == np.int64 and lk.shape == (B, metrics.LK_SLOTS)
    for b in range(B):
        M = int(lk[b, metrics.LK_MERGES])
        assert (merges[b, M:] == -1).all() and np.isnan(levels[b, M:]).all()
        assert not np.isnan(levels[b, :M]).any()
        assert (merges[b, :M, 0] < merges[b, :M, 1]).all()
        lv = levels[b, :M].astype(np.float64)
        assert (lv[1:] <= lv[:-1]).all()                # Kruskal's order
        for k in range(M - 1):                          # ties: (p, q) ascending
            if lv[k] == lv[k + 1]:
                assert tuple(merges[b, k]) < tuple(merges[b, k + 1])
        last = curve[b, M - 1] if M else (0, 0)
        assert (curve[b, M:] == last).all()
        assert lk[b, metrics.LK_PAIRS] == nc * (nc - 1) // 2 and (lk[b, 5:] == 0).all()
        for k in range(M):
            tp = lv[k + 1] if k + 1 < M else -np.inf    # the bound this cut is reached at
            if not tp < lv[k]:
                continue                                # reached by no threshold
            thr = np.float32(tp) / np.float32(2) if rule == "mean" else np.float32(tp)
            ut, g, t = metrics.untangle_counts(label[b:b + 1], probs[b:b + 1], thr, rule)
            assert ut[0, metrics.UT_GROUPS] == nc - (k + 1), (b, k)
            assert ut[0, metrics.UT_SS] == curve[b, k, 1], (b, k)
            assert ut[0, metrics.UT_SS] + ut[0, metrics.UT_SD] == curve[b, k, 0], (b, k)
            assert g[0].tolist() == _cut_groups(nc, merges[b], k), (b, k)
            assert ut[0, metrics.UT_TGROUPS] == lk[b, metrics.LK_TGROUPS]
            assert ut[0, metrics.UT_SS] + ut[0, metrics.UT_DS] == lk[b, metrics.LK_ST]
            assert ut[0, metrics.UT_NAN] <= lk[b, metrics.LK_NAN]
            assert ut[0, metrics.UT_NAN] == lk[b, metrics.LK_NAN] or not nan_scores_only
            np.testing.assert_array_equal(t[0], tgroups[b])
    return merges, levels, curve, tgroups, lk


@pytest.mark.parametrize("rule", RULES)
@pytest.mark.parametrize("nc", [2, 3, 4, 5, 8, 13, 21, 32, 33])
def test_every_reachable_cut_is_untangles_partition(nc, rule):
    rng = np.random.default_rng(1000 + nc)
    y, p1 = _grid_scores(rng, 3, nc)
    _check_against_untangle(y, p1, rule)
    y, p1 = _grid_scores(rng, 3, nc, nan=0.3)
    _, _, _, _, lk = _check_against_untangle(y, p1, rule)
    if nc >= 8:
        assert (lk[:, metrics.LK_NAN] > 0).all()


@pytest.mark.parametrize("rule", RULES)
def test_all_scores_equal_gives_the_lexicographic_star(rule):
    nc = 19
    p1 = np.full((1, nc * (nc - 1)), 0.375, np.float32)
    y = np.zeros(p1.shape, np.uint8)
    merges, levels, curve, _, lk = metrics.linkage(_onehot(y), _probs(p1), rule)
    assert merges[0].tolist() == [[0, q] for q in range(1, nc)]
    want = np.float32(0.75 if rule == "mean" else 0.375)
    assert (_bits(levels[0]) == _bits(want)).all()
    assert curve[0, :, 0].tolist() == [(k + 1) * (k + 2) // 2 for k in range(nc - 1)]
    assert (curve[0, :, 1] == 0).all() and lk[0, metrics.LK_ST] == 0
    assert lk[0, metrics.LK_MERGES] == nc - 1 and lk[0, metrics.LK_TGROUPS] == nc


@pytest.mark.parametrize("rule", RULES)
def test_minus_zero_is_plus_zero(rule):
    nc = 9
    rng = np.random.default_rng(5)
    I, J = data.pair_index(nc)
    zero = np.zeros((2, len(I)), np.float32)
    mixed = np.where(rng.random(zero.shape) < 0.5, np.float32(-0.0), np.float32(0.0))
    assert np.signbit(mixed).any() and not np.signbit(mixed).all()
    y, _ = _grid_scores(rng, 2, nc)
    a = metrics.linkage(_onehot(y), np.stack([zero, zero], 1), rule)
    c = metrics.linkage(_onehot(y), np.ascontiguousarray(np.stack([zero, mixed], 1)), rule)
    for x, z in zip(a, c):
        np.testing.assert_array_equal(x, z)
    assert (_bits(c[1]) == 0).all()                     # +0 bit for bit
    assert c[0][0].tolist() == [[0, q] for q in range(1, nc)]


@pytest.mark.parametrize("rule", RULES)
def test_infinite_scores(rule):
    nc = 7
    rng = np.random.default_rng(6)
    I, J = data.pair_index(nc)
    p1 = rng.choice(np.array([-np.inf, -1.0, 0.25, 0.5, np.inf], np.float32), (3, len(I)))
    for p, q in ((0, 1), (1, 0), (2, 3), (3, 2)):       # an edge at +inf, one at -inf
        p1[:, (I == p) & (J == q)] = np.inf if p + q == 1 else -np.inf
    if rule == "mean":                                  # inf + -inf is NaN: not an edge
        p1[1] = np.where(np.isinf(p1[1]) & (p1[1] < 0), np.float32(-2.0), p1[1])
    y, _ = _grid_scores(rng, 3, nc)
    merges, levels, _, _, lk = _check_against_untangle(y, p1, rule, nan_scores_only=False)
    assert np.isposinf(levels[:, 0]).all() and merges[:, 0].tolist() == [[0, 1]] * 3
    # a merge at -inf is in the tree but reached by no threshold (the check above skips it)
    p1 = np.full((1, len(I)), -np.inf, np.float32)
    merges, levels, curve, _, lk = metrics.linkage(_onehot(y[:1]), _probs(p1), rule)
    assert lk[0, metrics.LK_MERGES] == nc - 1 and np.isneginf(levels[0]).all()
    assert merges[0].tolist() == [[0, q] for q in range(1, nc)]


@pytest.mark.parametrize("rule", RULES)
def test_nan_pairs_disconnect_a_hunk(rule):
    nc = 12
    rng = np.random.default_rng(7)
    I, J = data.pair_index(nc)
    y, p1 = _grid_scores(rng, 2, nc)
    p1[0, I == 5] = np.nan                              # hunk 5: one direction of every pair
    p1[1, (I == 5) | (I == 8)] = np.nan
    p1[1, (J == 8) & (I == 2)] = np.nan                 # both directions of one pair
    merges, levels, curve, _, lk = _check_against_untangle(y, p1, rule)
    assert lk[:, metrics.LK_MERGES].tolist() == [nc - 2, nc - 3]
    assert lk[:, metrics.LK_NAN].tolist() == [nc - 1, 2 * (nc - 1) - 1]
    assert not (merges[0] == 5).any() and not np.isin(merges[1], (5, 8)).any()
    assert (merges[0, nc - 2:] == -1).all() and np.isnan(levels[0, nc - 2:]).all()
    assert (curve[0, nc - 2:] == curve[0, nc - 3]).all()
    assert curve[0, -1, 0] == (nc - 1) * (nc - 2) // 2
    # no edge at all: M = 0 and the curve holds 0
    p1[:] = np.nan
    merges, levels, curve, _, lk = metrics.linkage(_onehot(y), _probs(p1), rule)
    assert (lk[:, metrics.LK_MERGES] == 0).all() and (merges == -1).all() and not curve.any()
    assert np.isnan(levels).all() and (lk[:, metrics.LK_NAN] == nc * (nc - 1) // 2).all()


def test_argument_checks():
    z = np.zeros((1, 2, 12), np.float32)
    with pytest.raises(ValueError):
        metrics.linkage(z, z, "most")
    with pytest.raises(ValueError):
        metrics.linkage(z[:, :, :-1], z[:, :, :-1])
    _, levels, curve, _, lk = metrics.linkage(z, z)
    with pytest.raises(ValueError):
        metrics.best_threshold(levels, curve, lk, "mean", "auc")
    with pytest.raises(ValueError):
        metrics.best_threshold(levels, curve, lk, "most")


# ---------------------------------------------------------------------------------------
# curve_scores and best_threshold
# ---------------------------------------------------------------------------------------
def test_curve_scores_are_the_untangle_scores_of_each_cut():
    rng = np.random.default_rng(8)
    nc = 14
    y, p1 = _grid_scores(rng, 4, nc, nan=0.05)
    _, levels, curve, _, lk = metrics.linkage(_onehot(y), _probs(p1), "any")
    cs = metrics.curve_scores(levels, curve, lk)
    for b in range(4):
        for k in range(nc - 1):
            sp, ss = (int(v) for v in curve[b, k])
            st, pairs = int(lk[b, metrics.LK_ST]), int(lk[b, metrics.LK_PAIRS])
            row = [0, 0, ss, sp - ss, st - ss, pairs - sp - st + ss, 0, 0]
            want = metrics.scores_from_untangle([row])
            for name in ("rand", "precision", "recall", "f1"):
                np.testing.assert_equal(cs[name][b, k], want[name])


@pytest.mark.parametrize("score", ["f1", "rand"])
@pytest.mark.parametrize("rule", RULES)
def test_best_threshold_against_every_candidate(rule, score):
    rng = np.random.default_rng(9)
    nc, B = 11, 5
    y, p1 = _grid_scores(rng, B, nc, nan=0.1)
    p1[0, :4] = -np.inf
    label, probs = _onehot(y), _probs(p1)
    _, levels, curve, _, lk = metrics.linkage(label, probs, rule)
    thr, best, tp = metrics.best_threshold(levels, curve, lk, rule, score)
    cands = sorted(set(levels[~np.isnan(levels)].astype(np.float64).tolist()) | {-np.inf},
                   reverse=True)
    vals = []
    for c in cands:
        t = np.float32(c) / np.float32(2) if rule == "mean" else np.float32(c)
        ut, _, _ = metrics.untangle_counts(label, probs, t, rule)
        vals.append(metrics.scores_from_untangle(ut)[score])
        # the table read off the tree is the one untangle gives there (LINKS aside)
        table = metrics.cut_table(levels, curve, lk, c)
        keep = [k for k in range(metrics.UT_SLOTS) if k != metrics.UT_LINKS]
        np.testing.assert_array_equal(table[:, keep], ut[:, keep])
    finite = [v for v in vals if not math.isnan(v)]
    assert best == max(finite)
    assert tp == cands[[i for i, v in enumerate(vals) if v == best][0]]      # largest t' of a tie
    assert thr == (np.float32(tp) / np.float32(2) if rule == "mean" else tp)


def test_best_threshold_ties_go_to_the_largest_bound():
    # two commits of three hunks: all of commit 0 in one true group, none of commit 1
    levels = np.array([[0.75, 0.5], [0.25, 0.125]], np.float32)
    curve = np.array([[[1, 1], [3, 3]], [[1, 0], [3, 0]]], np.int64)
    lk = np.zeros((2, metrics.LK_SLOTS), np.int64)
    lk[:, metrics.LK_MERGES], lk[:, metrics.LK_PAIRS] = 2, 3
    lk[0, metrics.LK_ST], lk[0, metrics.LK_TGROUPS], lk[1, metrics.LK_TGROUPS] = 3, 1, 3
    thr, best, tp = metrics.best_threshold(levels, curve, lk, "any", "f1")
    assert (thr, best, tp) == (0.25, 1.0, 0.25)         # level > 0.25: both of commit 0, none of 1
    thr, best, tp = metrics.best_threshold(levels, curve, lk, "mean", "rand")
    assert (thr, best, tp) == (0.125, 1.0, 0.25)
    # a tie: SS 1, SD 0, DS 1 after the first merge and SS 2, SD 2, DS 0 after the second
    # are both f1 = 2/3; the third cut and no merge at all are worse
    levels = np.array([[0.75, 0.5, 0.25]], np.float32)
    curve = np.array([[[1, 1], [4, 2], [6, 2]]], np.int64)
    lk = np.zeros((1, metrics.LK_SLOTS), np.int64)
    lk[0, :5] = (3, 3, 2, 0, 6)
    thr, best, tp = metrics.best_threshold(levels, curve, lk, "both", "f1")
    assert (thr, best, tp) == (0.5, 2 / 3, 0.5)
    # no score defined anywhere (no same pair on either side): nan, at the only candidate
    lk[0, :5] = (0, 4, 0, 6, 6)
    nothing = np.full((1, 3), np.nan, np.float32)
    thr, best, tp = metrics.best_threshold(nothing, np.zeros((1, 3, 2), np.int64), lk, "both", "f1")
    assert math.isnan(best) and tp == -np.inf and thr == -np.inf


def test_calibration_fixes_a_planted_case():
    """Within-group scores 0.30 .. 0.40, cross-group scores <= 0.20: nothing links at 0.5."""
    rng = np.random.default_rng(10)
    nc, B = 24, 6
    I, J = data.pair_index(nc)
    grp = rng.integers(0, 4, (B, nc))
    same = grp[:, I] == grp[:, J]
    p1 = np.where(same, 0.30 + 0.10 * rng.random(same.shape), 0.20 * rng.random(same.shape))
    p1 = p1.astype(np.float32)
    y = same.astype(np.uint8)
    label, probs = _onehot(y), _probs(p1)
    for rule in RULES:
        at_half = metrics.scores_from_untangle(metrics.untangle_counts(label, probs, 0.5, rule)[0])
        assert at_half["exact"] == 0.0
        _, levels, curve, _, lk = metrics.linkage(label, probs, rule)
        thr, best, _ = metrics.best_threshold(levels, curve, lk, rule, "f1")
        assert best == 1.0
        tuned = metrics.scores_from_untangle(metrics.untangle_counts(label, probs, thr, rule)[0])
        assert tuned["exact"] == 1.0 and tuned["f1"] == 1.0


# ---------------------------------------------------------------------------------------
# header, binding, entry points
# ---------------------------------------------------------------------------------------
def test_python_mirrors_match_the_header():
    with open(os.path.join(ROOT, "include", "hdgnn.h")) as f:
        txt = f.read()
    val = {k[len("HDG_"):]: int(v) for k, v in re.findall(r"#define\s+(HDG_LK_[A-Z_0-9]+)\s+(\d+)", txt)}
    names = ["LK_SLOTS", "LK_MERGES", "LK_TGROUPS", "LK_ST", "LK_NAN", "LK_PAIRS"]
    for n in names:
        assert val[n] == getattr(_lib, n) == getattr(metrics, n), n
    assert len(val) == len(names)                   # nothing in the header without a mirror
    assert "hdg_linkage" in _lib.EXPORTS and "hdg_linkage_workspace_bytes" in _lib.EXPORTS
    assert re.search(r"#define\s+HDG_ABI_VERSION\s+9\b", txt)


def test_library_entry_points_reject_bad_arguments():
    """Host side of the C entry points (no device call is reached)."""
    lib = _lib.load()
    ok = _lib.Shape(100, 200, 74, 2, 100, 0)
    assert lib.hdg_linkage_workspace_bytes(ctypes.byref(ok)) == 100 * 1 * 74 * 8
    big = _lib.Shape(32, 1024, 512, 2, 32, 0)
    assert lib.hdg_linkage_workspace_bytes(ctypes.byref(big)) == \
        32 * _lib.untangle_blocks(512) * 512 * 8
    for b, nc in ((0, 74), (65536, 74), (4, 1), (4, 2049)):
        bad = _lib.Shape(b, 200, nc, 2, 4, 0)
        assert lib.hdg_linkage_workspace_bytes(ctypes.byref(bad)) == 0
        assert b"must be in" in lib.hdg_last_error()
    one = ctypes.c_void_p(64)                       # never dereferenced: the checks come first
    bt = _lib.Batch(None, None, one, None, None, None)
    args = dict(probs=one, rule=0, merges=one, levels=one, curve=one, lk=one, ws=one, shape=ok,
                bt=bt)

    def call(**kw):
        a = dict(args, **kw)
        return lib.hdg_linkage(ctypes.byref(a["shape"]), ctypes.byref(a["bt"]), a["probs"],
                               a["rule"], a["merges"], a["levels"], a["curve"], None, a["lk"],
                               a["ws"], None)

    einval = 1000
    assert call(rule=3) == einval and b"rule" in lib.hdg_last_error()
    assert lib.hdg_last_error().startswith(b"hdg_linkage:")
    assert call(rule=-1) == einval
    for k in ("probs", "merges", "levels", "curve", "lk", "ws"):
        assert call(**{k: None}) == einval and b"NULL" in lib.hdg_last_error(), k
        assert lib.hdg_last_error().startswith(b"hdg_linkage:")
    assert call(bt=_lib.Batch(None, None, None, None, None, None)) == einval
    assert call(ws=ctypes.c_void_p(68)) == einval and b"aligned" in lib.hdg_last_error()
    assert call(shape=_lib.Shape(0, 200, 74, 2, 1, 0)) == einval
    assert call(shape=_lib.Shape(4, 200, 2049, 2, 4, 0)) == einval
    assert lib.hdg_last_error().startswith(b"hdg_linkage: nc must be")


# ---------------------------------------------------------------------------------------
# main.py --Type calibrate, --link-threshold auto (test_cli's recorder pattern)
# ---------------------------------------------------------------------------------------
class _Recorder:
    log = []

    def __init__(self, sess, **kw):
        assert sess is None
        _Recorder.log.append(("init", kw))

    def train(self, args):
        _Recorder.log.append(("train",))

    def test(self, args):
        _Recorder.log.append(("test",))

    def evaluate(self, args):
        _Recorder.log.append(("eval",))

    def untangle(self, args, part="test", threshold=0.5, rule="mean"):
        _Recorder.log.append(("untangle", args.Step, part, threshold, rule))

    def calibrate(self, args, part="train", rule="mean", score="f1"):
        _Recorder.log.append(("calibrate", args.Step, part, rule, score))
        return 0.125 * args.Step, {}, None, None, None


def _main():
    import importlib.util
    spec = importlib.util.spec_from_file_location("hdg_main_lk",
                                                  os.path.join(ROOT, "hd-gnn_amd", "main.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _runs(cli, argv, tmp_path):
    _Recorder.log = []
    cli.main(argv + ["--checkpoint_dir", str(tmp_path)], model_cls=_Recorder)
    return [e for e in _Recorder.log if e[0] != "init"]


def test_main_calibrate_and_auto_threshold(tmp_path):
    cli = _main()
    assert _runs(cli, ["--Type", "calibrate"], tmp_path) == \
        [("calibrate", s, "train", "mean", "f1") for s in cli.STEPS]
    assert _runs(cli, ["--Type", "calibrate", "--link-rule", "both", "--link-score", "rand"],
                 tmp_path) == [("calibrate", s, "train", "both", "rand") for s in cli.STEPS]
    # auto: calibrate on the train split, then untangle with the float it returned
    runs = _runs(cli, ["--Type", "untangle", "--link-threshold", "auto", "--link-rule", "any"],
                 tmp_path)
    want = []
    for s in cli.STEPS:
        want += [("calibrate", s, "train", "any", "f1"), ("untangle", s, "test", 0.125 * s, "any")]
    assert runs == want
    assert all(isinstance(r[3], float) for r in runs if r[0] == "untangle")
    # a number: untangle alone, as before
    assert _runs(cli, ["--Type", "untangle", "--link-threshold", "0.25"], tmp_path) == \
        [("untangle", s, "test", 0.25, "mean") for s in cli.STEPS]
    assert _runs(cli, ["--Type", "untangle"], tmp_path) == \
        [("untangle", s, "test", 0.5, "mean") for s in cli.STEPS]
    assert [e[0] for e in _runs(cli, ["--Type", "eval"], tmp_path)] == ["eval"] * 3
    for bad in (["--link-score", "auc"], ["--link-threshold", "best"]):
        with pytest.raises(SystemExit):
            cli.main(["--Type", "untangle", "--checkpoint_dir", str(tmp_path)] + bad,
                     model_cls=_Recorder)
    parser = cli.build_parser(2, 200, 74, 39800, 5402)
    assert not [a for a in parser._actions if "link" in a.dest]
