"""Agglomeration on the host (CPU): hdgnn.metrics.agglomerate, the restatement hdg_agglomerate
is compared with on the GPU, against the definitions of include/hdgnn.h themselves --
single linkage against metrics.linkage, single and complete linkage against the max / min
over the raw pair weights of each merge's members, average linkage against the exactly
rounded float64 mean where the fp32 sums are exact, the running minimum on a pinned raw
inversion -- metrics.cut_groups against metrics.untangle_counts, a planted chaining case
that only complete and average linkage untangle, the Python mirrors of HDG_AG_* / HDG_CUT_*,
the host-side argument checks of hdg_agglomerate and hdg_cut, and main.py --link-method.
Every comparison is integer or bit equality.
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


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _labels(rng, B, nc, k=3):
    I, J = data.pair_index(nc)
    gt = rng.integers(0, k, (B, nc))
    return ((gt[:, I] == gt[:, J]) & (rng.random((B, len(I))) < 0.6)).astype(np.uint8)


def _planted(rng, B, nc):
    """Scores on the 1/256 grid (many ties): high inside planted groups, low across."""
    I, J = data.pair_index(nc)
    gp = rng.integers(0, max(2, nc // 12), (B, nc))
    same = gp[:, I] == gp[:, J]
    p1 = np.where(same, rng.integers(160, 257, same.shape), rng.integers(0, 96, same.shape)) / 256.0
    return _labels(rng, B, nc), p1.astype(np.float32)


def _uniform(rng, B, nc):
    return _labels(rng, B, nc), rng.random((B, nc * (nc - 1)), dtype=np.float32)


def _ulp_family(rng, B, nc):
    """Scores 0.75 + {0 .. 3} ulps: fp32 sums of them round, so raw average levels invert."""
    base = np.float32(0.75).view(np.uint32)
    p1 = (base + rng.integers(0, 4, (B, nc * (nc - 1))).astype(np.uint32)).view(np.float32)
    return _labels(rng, B, nc), p1


def _weights(p1, nc, rule):
    """(nc, nc) float32 pair weights of one commit under the rule, NaN: no edge; -0 -> +0."""
    I, J = data.pair_index(nc)
    S = np.zeros((nc, nc), np.float32)
    S[I, J] = p1
    with np.errstate(invalid="ignore", over="ignore"):
        if rule == "mean":
            W = S + S.T
        else:
            W = np.where(np.isnan(S) | np.isnan(S.T), np.float32(np.nan),
                         np.maximum(S, S.T) if rule == "any" else np.minimum(S, S.T))
    W = np.where(W == 0, np.float32(0), W).astype(np.float32)
    np.fill_diagonal(W, np.nan)
    return W


def _members(nc, merges, upto):
    """Clusters (by smallest member) after merges[:upto] -> dict name -> member list."""
    cl = {i: [i] for i in range(nc)}
    for a, c in merges[:upto]:
        assert a < c and a in cl and c in cl          # names are the clusters' smallest members
        cl[a] = cl[a] + cl.pop(c)
    return cl


# ---------------------------------------------------------------------------------------
# single linkage against metrics.linkage
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("rule", RULES)
@pytest.mark.parametrize("nc", [2, 3, 33, 65, 74])
def test_single_matches_linkage(nc, rule):
    rng = np.random.default_rng(1000 + nc)
    for what, (y, p1) in (("planted", _planted(rng, 2, nc)), ("uniform", _uniform(rng, 2, nc))):
        label, probs = _onehot(y), _probs(p1)
        m, lv, cv, t, lk = metrics.agglomerate(label, probs, rule, "single")
        hm, hlv, hcv, ht, hlk = metrics.linkage(label, probs, rule)
        np.testing.assert_array_equal(_bits(lv), _bits(hlv), what)
        np.testing.assert_array_equal(lk, hlk, what)
        np.testing.assert_array_equal(t, ht, what)
        for b in range(len(lv)):
            M = int(lk[b, metrics.LK_MERGES])
            nxt = np.append(lv[b, 1:M], -np.inf)
            reach = np.flatnonzero(nxt < lv[b, :M])
            assert len(reach) > 0
            np.testing.assert_array_equal(cv[b, reach], hcv[b, reach], what)
            # and the partitions there are the same: cluster minima here, edge ends there
            for k in reach[[0, len(reach) // 2, -1]]:
                tp = nxt[k]
                np.testing.assert_array_equal(metrics.cut_groups(m[b:b + 1], lv[b:b + 1], tp),
                                              metrics.cut_groups(hm[b:b + 1], hlv[b:b + 1], tp))


# ---------------------------------------------------------------------------------------
# against the definition: levels from the raw pair weights and the membership
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("rule", RULES)
@pytest.mark.parametrize("method", ["single", "complete"])
def test_single_and_complete_levels_are_the_max_and_min_over_member_pairs(method, rule):
    rng = np.random.default_rng(7)
    nc, B = 21, 3
    y, p1 = _planted(rng, B, nc)
    p1[rng.random(p1.shape) < 0.03] = np.nan
    m, lv, _, _, lk, raw = metrics.agglomerate(_onehot(y), _probs(p1), rule, method, raw=True)
    np.testing.assert_array_equal(_bits(lv), _bits(raw))         # already non-increasing
    for b in range(B):
        W = _weights(p1[b], nc, rule)
        for k in range(int(lk[b, metrics.LK_MERGES])):
            cl = _members(nc, m[b], k)
            a, c = m[b, k]
            w = W[np.ix_(cl[a], cl[c])]
            if method == "single":
                assert not np.isnan(w).all()
                want = np.nanmax(w)
            else:
                assert not np.isnan(w).any()
                want = w.min()
            assert _bits(lv[b, k]) == _bits(want), (b, k)
            # and no cluster pair before (a, c) in the order has a larger or equal similarity
            names = sorted(cl)
            for i, x in enumerate(names):
                for z in names[i + 1:]:
                    ww = W[np.ix_(cl[x], cl[z])]
                    if method == "single":
                        d = np.nanmax(ww) if not np.isnan(ww).all() else None
                    else:
                        d = ww.min() if not np.isnan(ww).any() else None
                    if d is None:
                        continue
                    assert d < want or (d == want and (x, z) >= (a, c)), (b, k, x, z)


@pytest.mark.parametrize("rule", RULES)
@pytest.mark.parametrize("nc", [9, 40, 129])
def test_average_level_is_the_exact_mean_on_the_grid(nc, rule):
    """Scores k / 256: every fp32 sum of at most 129^2 / 4 weights is exact, so S is the true
    sum and the level is the float64 mean rounded once."""
    rng = np.random.default_rng(50 + nc)
    B = 2 if nc < 100 else 1
    y, p1 = _planted(rng, B, nc)
    m, lv, _, _, lk, raw = metrics.agglomerate(_onehot(y), _probs(p1), rule, "average", raw=True)
    for b in range(B):
        W = _weights(p1[b], nc, rule).astype(np.float64)
        assert lk[b, metrics.LK_MERGES] == nc - 1
        for k in range(nc - 1):
            cl = _members(nc, m[b], k)
            a, c = m[b, k]
            mean = W[np.ix_(cl[a], cl[c])].sum() / (len(cl[a]) * len(cl[c]))
            assert _bits(raw[b, k]) == _bits(np.float32(mean)), (b, k)
    np.testing.assert_array_equal(_bits(lv), _bits(np.minimum.accumulate(raw, axis=1)))


@pytest.mark.parametrize("method", METHODS)
def test_levels_never_increase(method):
    rng = np.random.default_rng(3)
    for y, p1 in (_planted(rng, 3, 33), _uniform(rng, 3, 33), _ulp_family(rng, 8, 8)):
        for rule in RULES:
            _, lv, cv, _, lk = metrics.agglomerate(_onehot(y), _probs(p1), rule, method)
            assert (np.diff(lv, axis=1) <= 0).all()
            assert (np.diff(cv, axis=1) >= 0).all()
            assert (lk[:, metrics.LK_MERGES] == lv.shape[1]).all()


def test_raw_average_levels_invert_and_levels_are_their_running_minimum():
    rng = np.random.default_rng(2024)
    y, p1 = _ulp_family(rng, 300, 8)
    _, lv, _, _, _, raw = metrics.agglomerate(_onehot(y), _probs(p1), "any", "average", raw=True)
    inverted = (np.diff(raw, axis=1) > 0).any(1)
    print("commits with a raw inversion:", int(inverted.sum()), "of", len(raw))
    assert inverted.any()                   # or this test stopped covering the running minimum
    np.testing.assert_array_equal(_bits(lv), _bits(np.minimum.accumulate(raw, axis=1)))
    assert (np.diff(lv, axis=1) <= 0).all()


# ---------------------------------------------------------------------------------------
# order, special values
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("rule", RULES)
@pytest.mark.parametrize("method", METHODS)
def test_all_scores_equal_gives_the_lexicographic_star(method, rule):
    nc = 9
    p1 = np.full((1, nc * (nc - 1)), 0.75, np.float32)
    y = np.zeros(p1.shape, np.uint8)
    m, lv, cv, _, lk = metrics.agglomerate(_onehot(y), _probs(p1), rule, method)
    assert m[0].tolist() == [[0, q] for q in range(1, nc)]
    assert (lv == (1.5 if rule == "mean" else 0.75)).all()
    assert cv[0, :, 0].tolist() == [(k + 1) * (k + 2) // 2 for k in range(nc - 1)]


@pytest.mark.parametrize("rule", RULES)
@pytest.mark.parametrize("method", METHODS)
def test_infinite_and_minus_zero_scores(method, rule):
    nc = 5
    I, J = data.pair_index(nc)
    p1 = np.full((2, nc * (nc - 1)), 0.25, np.float32)
    p1[0, (I == 0) | (J == 0)] = -0.0
    p1[0, ((I == 0) & (J == 1)) | ((I == 1) & (J == 0))] = np.inf
    p1[0, ((I == 2) & (J == 3)) | ((I == 3) & (J == 2))] = -np.inf
    p1[1, :] = -0.0                                   # every weight -0 -> +0
    y = np.zeros(p1.shape, np.uint8)
    m, lv, _, _, lk = metrics.agglomerate(_onehot(y), _probs(p1), rule, method)
    assert m[0, 0].tolist() == [0, 1] and lv[0, 0] == np.inf
    assert (lk[:, metrics.LK_MERGES] == nc - 1).all() and (lk[:, metrics.LK_NAN] == 0).all()
    assert not np.signbit(lv[np.isfinite(lv) & (lv == 0)]).any()
    assert m[1].tolist() == [[0, q] for q in range(1, nc)] and (_bits(lv[1]) == 0).all()
    if method != "single":                            # 2 and 3 meet in the last merge only
        assert np.isneginf(lv[0, -1]) and np.isfinite(lv[0, -2])
    # +inf against -inf under "mean" is no edge, and counts
    p2 = np.full((1, nc * (nc - 1)), 0.25, np.float32)
    p2[0, (I == 0) & (J == 1)] = np.inf
    p2[0, (I == 1) & (J == 0)] = -np.inf
    _, _, _, _, lk2 = metrics.agglomerate(_onehot(y[:1]), _probs(p2), rule, method)
    assert lk2[0, metrics.LK_NAN] == (1 if rule == "mean" else 0)


@pytest.mark.parametrize("rule", RULES)
@pytest.mark.parametrize("method", METHODS)
def test_nan_pairs(method, rule):
    nc = 8
    I, J = data.pair_index(nc)
    rng = np.random.default_rng(5)
    y, p1 = _uniform(rng, 1, nc)
    p1[0, I == 3] = np.nan                            # hunk 3: no edge reaches it
    m, lv, cv, _, lk = metrics.agglomerate(_onehot(y), _probs(p1), rule, method)
    assert lk[0, metrics.LK_MERGES] == nc - 2 and lk[0, metrics.LK_NAN] == nc - 1
    assert (m[0, -1] == -1).all() and np.isnan(lv[0, -1]) and not (m[0, :-1] == 3).any()
    assert (cv[0, -1] == cv[0, -2]).all()
    # two cliques {0..3}, {4..7} at 0.75, every pair between them 0.5, one of those a NaN:
    # complete and average linkage never join them, single linkage does through another pair
    same = (I < 4) == (J < 4)
    p1 = np.where(same, 0.75, 0.5).astype(np.float32)[None]
    p1[0, (I == 1) & (J == 6)] = np.nan
    m, lv, _, _, lk = metrics.agglomerate(_onehot(y), _probs(p1), rule, method)
    assert lk[0, metrics.LK_NAN] == 1
    assert lk[0, metrics.LK_MERGES] == (nc - 1 if method == "single" else nc - 2)
    if method == "single":
        assert m[0, -1].tolist() == [0, 4] and lv[0, -1] == (1.0 if rule == "mean" else 0.5)


def test_argument_checks():
    y = np.zeros((1, 6), np.uint8)
    p1 = np.zeros((1, 6), np.float32)
    with pytest.raises(ValueError):
        metrics.agglomerate(_onehot(y), _probs(p1), "most", "average")
    with pytest.raises(ValueError):
        metrics.agglomerate(_onehot(y), _probs(p1), "mean", "ward")
    with pytest.raises(ValueError):
        metrics.agglomerate(_onehot(y[:, :5]), _probs(p1[:, :5]), "mean", "average")
    assert len(metrics.agglomerate(_onehot(y), _probs(p1))) == 5
    assert len(metrics.agglomerate(_onehot(y), _probs(p1), raw=True)) == 6


# ---------------------------------------------------------------------------------------
# chaining: what single linkage cannot untangle at any threshold
# ---------------------------------------------------------------------------------------
def test_a_bridge_chains_single_linkage_only():
    """Three true groups, each a clique of two tight halves: 0.7 inside a half, 0.4 between
    the halves of a group, <= 0.2 across groups -- except one bridge pair per commit between
    two groups at 0.5, above what holds any group together.  Single linkage has fused the two
    groups through the bridge before either is whole, at every threshold; the worst or the mean
    pair of the bridged halves stays below 0.4."""
    rng = np.random.default_rng(11)
    nc, B = 18, 5
    I, J = data.pair_index(nc)
    grp, half = np.zeros((B, nc), np.int64), np.zeros((B, nc), np.int64)
    for b in range(B):
        perm = rng.permutation(nc)
        grp[b, perm], half[b, perm] = np.arange(nc) % 3, (np.arange(nc) // 3) % 2
    same = grp[:, I] == grp[:, J]
    tight = same & (half[:, I] == half[:, J])
    p1 = np.where(tight, 0.7, np.where(same, 0.4, 0.2 * rng.random(same.shape)))
    p1 = p1.astype(np.float32)
    for b in range(B):
        p = int(np.flatnonzero(grp[b] == 0)[0])
        q = int(np.flatnonzero(grp[b] == 1)[0])
        p1[b, ((I == p) & (J == q)) | ((I == q) & (J == p))] = 0.5
    y = same.astype(np.uint8)
    label, probs = _onehot(y), _probs(p1)
    planted = metrics.untangle_counts(label, probs, 0.5, "mean")[2]      # the true groups' ids
    for rule in RULES:
        for method in METHODS:
            m, lv, cv, t, lk = metrics.agglomerate(label, probs, rule, method)
            np.testing.assert_array_equal(t, planted)
            thr, best, tp = metrics.best_threshold(lv, cv, lk, rule, "f1")
            print(rule, method, "best f1", best, "at", thr)
            if method == "single":
                assert best < 1.0
                continue
            assert best == 1.0
            np.testing.assert_array_equal(metrics.cut_groups(m, lv, tp), planted)
            table = metrics.cut_table(lv, cv, lk, tp)
            assert (table[:, metrics.UT_SD] == 0).all() and (table[:, metrics.UT_DS] == 0).all()


# ---------------------------------------------------------------------------------------
# cut_groups
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("rule", RULES)
def test_cut_groups_of_the_linkage_tree_are_untangles_groups(rule):
    rng = np.random.default_rng(21)
    nc, B = 33, 3
    y, p1 = _uniform(rng, B, nc)
    p1[rng.random(p1.shape) < 0.02] = np.nan
    label, probs = _onehot(y), _probs(p1)
    m, lv, cv, _, lk = metrics.linkage(label, probs, rule)
    for b in range(B):
        M = int(lk[b, metrics.LK_MERGES])
        nxt = np.append(lv[b, 1:M], -np.inf)
        reach = np.flatnonzero(nxt < lv[b, :M])
        for k in reach[[0, len(reach) // 3, 2 * len(reach) // 3, -1]]:
            tp = np.float32(nxt[k])
            thr = float(tp / np.float32(2)) if rule == "mean" else float(tp)
            ut, g, _ = metrics.untangle_counts(label, probs, thr, rule)
            np.testing.assert_array_equal(metrics.cut_groups(m, lv, tp)[b], g[b])
            assert ut[b, metrics.UT_GROUPS] == nc - (k + 1)
    # above every level: singletons; rows of -1 / NaN are skipped
    np.testing.assert_array_equal(metrics.cut_groups(m, lv, np.inf),
                                  np.tile(np.arange(nc, dtype=np.int32), (B, 1)))
    pad_m = np.concatenate([m, np.full((B, 2, 2), -1, np.int32)], 1)
    pad_l = np.concatenate([lv, np.full((B, 2), np.nan, np.float32)], 1)
    assert metrics.cut_groups(pad_m, pad_l, -np.inf).shape == (B, nc + 2)


# ---------------------------------------------------------------------------------------
# header, binding, entry points
# ---------------------------------------------------------------------------------------
def test_python_mirrors_match_the_header():
    with open(os.path.join(ROOT, "include", "hdgnn.h")) as f:
        txt = f.read()
    val = {k[len("HDG_"):]: int(v)
           for k, v in re.findall(r"#define\s+(HDG_(?:AG|CUT)_[A-Z_0-9]+)\s+(\d+)", txt)}
    names = ["AG_SINGLE", "AG_COMPLETE", "AG_AVERAGE", "AG_FLAG_GLOBAL", "AG_LDS_MAX_NC",
             "CUT_SLOTS", "CUT_GROUPS", "CUT_TGROUPS", "CUT_SS", "CUT_SD", "CUT_DS", "CUT_DD",
             "CUT_MERGES", "CUT_NAN"]
    for n in names:
        assert val[n] == getattr(_lib, n), n
    assert len(val) == len(names)                   # nothing in the header without a mirror
    assert _lib.AG_METHODS == {"single": val["AG_SINGLE"], "complete": val["AG_COMPLETE"],
                               "average": val["AG_AVERAGE"]}
    assert tuple(_lib.AG_METHODS) == metrics.AG_METHODS
    assert _lib.AG_LDS_MAX_NC >= 160                # every fused-path shape is LDS-resident
    # hdg_cut's row is hdg_untangle's but for slot 6
    for n in ("SLOTS", "GROUPS", "TGROUPS", "SS", "SD", "DS", "DD", "NAN"):
        assert getattr(_lib, "CUT_" + n) == getattr(_lib, "UT_" + n), n
    assert _lib.CUT_MERGES == _lib.UT_LINKS
    for name in ("hdg_agglomerate", "hdg_agglomerate_workspace_bytes", "hdg_cut"):
        assert name in _lib.EXPORTS
    assert re.search(r"#define\s+HDG_ABI_VERSION\s+9\b", txt)


def test_library_entry_points_reject_bad_arguments():
    """Host side of the C entry points (no device call is reached)."""
    lib = _lib.load()
    ok = _lib.Shape(100, 200, 74, 2, 100, 0)
    for flags in (0, _lib.AG_FLAG_GLOBAL):
        assert lib.hdg_agglomerate_workspace_bytes(ctypes.byref(ok), flags) == 100 * 74 * 74 * 4
    assert lib.hdg_agglomerate_workspace_bytes(ctypes.byref(_lib.Shape(1, 2, 2, 2, 1, 0)), 0) == 16
    for b, nc in ((1, 2), (1, 2048), (65535, 2)):   # never 0 for a valid shape
        assert lib.hdg_agglomerate_workspace_bytes(ctypes.byref(_lib.Shape(b, 2, nc, 2, b, 0)),
                                                   0) == b * nc * nc * 4
    for b, nc in ((0, 74), (65536, 74), (4, 1), (4, 2049)):
        bad = _lib.Shape(b, 200, nc, 2, 4, 0)
        assert lib.hdg_agglomerate_workspace_bytes(ctypes.byref(bad), 0) == 0
        assert b"must be in" in lib.hdg_last_error()
    one = ctypes.c_void_p(64)                       # never dereferenced: the checks come first
    bt = _lib.Batch(None, None, one, None, None, None)
    args = dict(probs=one, rule=0, method=2, flags=0, merges=one, levels=one, curve=one, lk=one,
                ws=one, shape=ok, bt=bt)

    def call(**kw):
        a = dict(args, **kw)
        return lib.hdg_agglomerate(ctypes.byref(a["shape"]), ctypes.byref(a["bt"]), a["probs"],
                                   a["rule"], a["method"], a["flags"], a["merges"], a["levels"],
                                   a["curve"], None, a["lk"], a["ws"], None)

    einval = 1000
    for kw, word in ((dict(rule=3), b"rule"), (dict(rule=-1), b"rule"), (dict(method=3), b"method"),
                     (dict(method=-1), b"method"), (dict(flags=2), b"flag"),
                     (dict(flags=-1), b"flag")):
        assert call(**kw) == einval and word in lib.hdg_last_error(), kw
        assert lib.hdg_last_error().startswith(b"hdg_agglomerate:")
    for k in ("probs", "merges", "levels", "curve", "lk", "ws"):
        assert call(**{k: None}) == einval and b"NULL" in lib.hdg_last_error(), k
        assert lib.hdg_last_error().startswith(b"hdg_agglomerate:")
    assert call(bt=_lib.Batch(None, None, None, None, None, None)) == einval
    assert call(ws=ctypes.c_void_p(68)) == einval and b"aligned" in lib.hdg_last_error()
    assert call(shape=_lib.Shape(0, 200, 74, 2, 1, 0)) == einval
    assert call(shape=_lib.Shape(4, 200, 2049, 2, 4, 0)) == einval
    assert lib.hdg_last_error().startswith(b"hdg_agglomerate: nc must be")

    cargs = dict(shape=ok, merges=one, levels=one, curve=one, lk=one, thr=0.5, rule=0, groups=one,
                 ut=one)

    def cut(**kw):
        a = dict(cargs, **kw)
        return lib.hdg_cut(ctypes.byref(a["shape"]), a["merges"], a["levels"], a["curve"], a["lk"],
                           ctypes.c_float(a["thr"]), a["rule"], a["groups"], a["ut"], None)

    assert cut(thr=float("nan")) == einval and b"NaN" in lib.hdg_last_error()
    assert lib.hdg_last_error().startswith(b"hdg_cut:")
    assert cut(rule=3) == einval and b"rule" in lib.hdg_last_error()
    assert cut(rule=-1) == einval
    for k in ("merges", "levels", "groups"):
        assert cut(**{k: None}) == einval and b"NULL" in lib.hdg_last_error(), k
    for k in ("curve", "lk"):                       # required once ut is given
        assert cut(**{k: None}) == einval and b"ut needs" in lib.hdg_last_error(), k
    assert cut(shape=_lib.Shape(4, 200, 1, 2, 4, 0)) == einval
    assert lib.hdg_last_error().startswith(b"hdg_cut: nc must be")


# ---------------------------------------------------------------------------------------
# main.py --link-method (a recorder of this file's own: it takes `method`)
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


def _main():
    import importlib.util
    spec = importlib.util.spec_from_file_location("hdg_main_ag",
                                                  os.path.join(ROOT, "hd-gnn_amd", "main.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _runs(cli, argv, tmp_path):
    _Recorder.log = []
    cli.main(argv + ["--checkpoint_dir", str(tmp_path)], model_cls=_Recorder)
    return _Recorder.log


def test_main_link_method(tmp_path):
    cli = _main()
    assert _runs(cli, ["--Type", "calibrate", "--link-method", "average"], tmp_path) == \
        [("calibrate", s, "train", "mean", "f1", {"method": "average"}) for s in cli.STEPS]
    runs = _runs(cli, ["--Type", "untangle", "--link-threshold", "auto", "--link-method",
                       "complete", "--link-rule", "both"], tmp_path)
    want = []
    for s in cli.STEPS:
        want += [("calibrate", s, "train", "both", "f1", {"method": "complete"}),
                 ("untangle", s, "test", 0.125 * s, "both", {"method": "complete"})]
    assert runs == want
    assert _runs(cli, ["--Type", "untangle", "--link-method", "average", "--link-threshold",
                       "0.25"], tmp_path) == \
        [("untangle", s, "test", 0.25, "mean", {"method": "average"}) for s in cli.STEPS]
    # single, given or by default, passes no method: the call as it always was
    for argv in (["--link-method", "single"], []):
        assert _runs(cli, ["--Type", "calibrate"] + argv, tmp_path) == \
            [("calibrate", s, "train", "mean", "f1", {}) for s in cli.STEPS]
        assert _runs(cli, ["--Type", "untangle"] + argv, tmp_path) == \
            [("untangle", s, "test", 0.5, "mean", {}) for s in cli.STEPS]
    with pytest.raises(SystemExit):
        cli.main(["--Type", "untangle", "--link-method", "ward", "--checkpoint_dir", str(tmp_path)],
                 model_cls=_Recorder)
