"""Untangling on the host (CPU): hdgnn.metrics.untangle_counts against an independent
statement of the definition in include/hdgnn.h (scipy's connected_components when it is
importable, else a plain Python union-find), the group-id order rule, the table's
invariants, scores_from_untangle on hand-made rows, the header constants against their
Python mirrors, and main.py --Type untangle through test_cli's recorder pattern.
"""
import math
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from hdgnn import _lib, data, metrics


# ---------------------------------------------------------------------------------------
# the independent statement
# ---------------------------------------------------------------------------------------
def _components_ref(n, edges):
    """Component label per node (any labels) of the undirected edges on n nodes."""
    try:
        from scipy.sparse import coo_matrix
        from scipy.sparse.csgraph import connected_components
    except ImportError:
        parent = list(range(n))

        def find(x):
            while parent[x] != x:
                x = parent[x]
            return x

        for a, b in edges:
            ra, rb = find(a), find(b)
            if ra != rb:
                parent[rb] = ra
        return [find(i) for i in range(n)]
    a = [e[0] for e in edges]
    b = [e[1] for e in edges]
    m = coo_matrix((np.ones(len(edges)), (a, b)), shape=(n, n))
    return list(connected_components(m, directed=False)[1])


def _dense_by_min_member(raw):
    """Relabel: the id of a group = the number of groups whose smallest member is smaller."""
    first = {}
    for i, r in enumerate(raw):
        first.setdefault(r, i)                      # smallest member of each group
    order = {r: k for k, r in enumerate(sorted(first, key=first.get))}
    return [order[r] for r in raw]


def _reference(y_rel, p1, nc, threshold, rule):
    """One commit, pair by pair in Python: y_rel / p1 (R,) in relation order."""
    thr = np.float32(threshold)

    def r(p, q):
        return p * (nc - 1) + q - (1 if q > p else 0)

    links, ylinks, nan = [], [], 0
    for p in range(nc):
        for q in range(p + 1, nc):
            spq, sqp = np.float32(p1[r(p, q)]), np.float32(p1[r(q, p)])
            if y_rel[r(p, q)] or y_rel[r(q, p)]:
                ylinks.append((p, q))
            if math.isnan(spq) or math.isnan(sqp):
                nan += 1
                continue
            if rule == "mean":
                hit = np.float32(spq + sqp) > np.float32(thr + thr)
            elif rule == "any":
                hit = spq > thr or sqp > thr
            else:
                hit = spq > thr and sqp > thr
            if hit:
                links.append((p, q))
    g = _dense_by_min_member(_components_ref(nc, links))
    t = _dense_by_min_member(_components_ref(nc, ylinks))
    ss = sd = ds = dd = 0
    for p in range(nc):
        for q in range(p + 1, nc):
            sp, st = g[p] == g[q], t[p] == t[q]
            ss += sp and st
            sd += sp and not st
            ds += (not sp) and st
            dd += (not sp) and (not st)
    return [max(g) + 1, max(t) + 1, ss, sd, ds, dd, len(links), nan], g, t


def _planted(rng, B, nc, k_pred, k_true, noise=0.0, keep=1.0):
    """Scores on a 1/256 grid from planted groups (within-group pairs high, `keep` of them),
    labels from other planted groups -> (y (B, R) u8, p1 (B, R) f32)."""
    I, J = data.pair_index(nc)
    gp = rng.integers(0, k_pred, (B, nc))
    gt = rng.integers(0, k_true, (B, nc))
    same = gp[:, I] == gp[:, J]
    lo = rng.integers(0, 100, same.shape)
    hi = rng.integers(160, 257, same.shape)
    on = same & (rng.random(same.shape) < keep)
    flip = rng.random(same.shape) < noise
    p1 = (np.where(on ^ flip, hi, lo) / 256.0).astype(np.float32)
    y = ((gt[:, I] == gt[:, J]) & (rng.random(same.shape) < 0.6)).astype(np.uint8)
    return y, p1


def _onehot(y):
    return np.stack([1 - y, y], 1).astype(np.float32)


def _probs(p1):
    return np.stack([1.0 - p1, p1], 1).astype(np.float32)


CASES = [(2, 1), (3, 2), (5, 3), (8, 4), (13, 5), (21, 6), (33, 7), (40, 8)]


@pytest.mark.parametrize("rule", ["mean", "any", "both"])
@pytest.mark.parametrize("nc,seed", CASES)
def test_host_counts_match_the_definition(nc, seed, rule):
    rng = np.random.default_rng(seed)
    B = 3
    y, p1 = _planted(rng, B, nc, 3, 2, noise=0.02, keep=0.5)
    p1[1] = rng.random(p1.shape[1], dtype=np.float32)          # one commit of plain noise
    y[1] = rng.random(y.shape[1]) < 1.5 / nc
    p1[2, rng.random(p1.shape[1]) < 0.05] = np.nan             # and one with NaNs
    p1[2, -1] = np.nan
    p1[0, 0] = 0.5                                             # exactly at the threshold
    ut, g, t = metrics.untangle_counts(_onehot(y), _probs(p1), 0.5, rule)
    assert ut.dtype == np.int64 and ut.shape == (B, metrics.UT_SLOTS)
    assert g.dtype == np.int32 and t.dtype == np.int32 and g.shape == t.shape == (B, nc)
    for b in range(B):
        row, gr, tr = _reference(y[b], p1[b], nc, 0.5, rule)
        assert ut[b].tolist() == row
        assert g[b].tolist() == gr and t[b].tolist() == tr
    assert (ut[:, [metrics.UT_SS, metrics.UT_SD, metrics.UT_DS, metrics.UT_DD]].sum(1)
            == nc * (nc - 1) // 2).all()
    assert ut[2, metrics.UT_NAN] > 0


def test_structured_graphs():
    nc = 17
    I, J = data.pair_index(nc)
    z = np.zeros((1, nc * (nc - 1)), np.uint8)

    def run(edges, directed=True):
        p1 = np.zeros((1, nc * (nc - 1)), np.float32)
        for p, q in edges:
            p1[0, (I == p) & (J == q)] = 1.0
            if not directed:
                p1[0, (I == q) & (J == p)] = 1.0
        return metrics.untangle_counts(_onehot(z), _probs(p1), 0.5, "any")

    ut, g, _ = run([(i, i + 1) for i in range(nc - 1)])                 # a path: one group
    assert ut[0, metrics.UT_GROUPS] == 1 and ut[0, metrics.UT_LINKS] == nc - 1
    assert not g.any()
    ut, g, t = run([])                                                  # no links
    assert ut[0, metrics.UT_GROUPS] == nc and g[0].tolist() == list(range(nc))
    assert ut[0, metrics.UT_TGROUPS] == nc and t[0].tolist() == list(range(nc))
    assert ut[0, metrics.UT_DD] == nc * (nc - 1) // 2
    ut, g, _ = run([(nc - 1, i) for i in range(3, nc - 1)])             # a star on the last hunk
    assert ut[0, metrics.UT_GROUPS] == 4
    assert g[0].tolist() == [0, 1, 2] + [3] * (nc - 3)
    # a one-directional score links under "any", not under "both"; "mean" follows the sum
    p1 = np.zeros((1, nc * (nc - 1)), np.float32)
    p1[0, (I == 2) & (J == 9)] = 0.75
    p1[0, (I == 9) & (J == 2)] = 0.25                                   # sum = 1.0: not > 1.0
    p1[0, (I == 3) & (J == 4)] = 0.75
    p1[0, (I == 4) & (J == 3)] = 0.375                                  # sum 1.125 > 1.0
    for rule, links in (("any", 2), ("both", 0), ("mean", 1)):
        ut, _, _ = metrics.untangle_counts(_onehot(z), _probs(p1), 0.5, rule)
        assert ut[0, metrics.UT_LINKS] == links, rule


def test_group_ids_are_ordered_by_smallest_member():
    rng = np.random.default_rng(11)
    nc = 30
    y, p1 = _planted(rng, 4, nc, 5, 4)
    _, g, t = metrics.untangle_counts(_onehot(y), _probs(p1))
    for ids in list(g) + list(t):
        assert ids[0] == 0
        seen = -1
        for i, v in enumerate(ids):                 # a new id is always the next integer
            assert v <= seen + 1
            seen = max(seen, v)
        firsts = [int(np.flatnonzero(ids == k)[0]) for k in range(seen + 1)]
        assert firsts == sorted(firsts)


def test_relabelling_the_hunks_permutes_the_groups_and_keeps_the_table():
    rng = np.random.default_rng(12)
    nc, B = 23, 3
    y, p1 = _planted(rng, B, nc, 4, 3, noise=0.01, keep=0.4)
    ut, g, t = metrics.untangle_counts(_onehot(y), _probs(p1))
    perm = rng.permutation(nc)                      # new hunk k is old hunk perm[k]
    I, J = data.pair_index(nc)
    S = np.zeros((B, nc, nc), np.float32)
    Y = np.zeros((B, nc, nc), np.uint8)
    S[:, I, J], Y[:, I, J] = p1, y
    S2, Y2 = S[:, perm][:, :, perm], Y[:, perm][:, :, perm]
    ut2, g2, t2 = metrics.untangle_counts(_onehot(Y2[:, I, J]), _probs(S2[:, I, J]))
    np.testing.assert_array_equal(ut2, ut)
    for b in range(B):                              # the same partition of the same hunks
        for old, new in ((g[b], g2[b]), (t[b], t2[b])):
            moved = old[perm]
            assert _dense_by_min_member(list(moved)) == new.tolist()


def test_strict_comparisons_and_argument_checks():
    nc = 4
    R = nc * (nc - 1)
    z = np.zeros((1, R), np.uint8)
    thr = np.float32(0.3)
    up = np.nextafter(thr, np.float32(1.0))
    for rule in ("mean", "any", "both"):
        at = np.full((1, R), thr, np.float32)
        assert metrics.untangle_counts(_onehot(z), _probs(at), thr, rule)[0][0, metrics.UT_LINKS] == 0
        above = np.full((1, R), up, np.float32)
        assert (metrics.untangle_counts(_onehot(z), _probs(above), thr, rule)[0][0, metrics.UT_LINKS]
                == nc * (nc - 1) // 2)
    with pytest.raises(ValueError):
        metrics.untangle_counts(_onehot(z), _probs(np.zeros((1, R), np.float32)), 0.5, "most")
    with pytest.raises(ValueError):
        metrics.untangle_counts(_onehot(z), _probs(np.zeros((1, R), np.float32)), float("nan"))
    with pytest.raises(ValueError):
        metrics.untangle_counts(_onehot(z[:, :-1]), _probs(np.zeros((1, R - 1), np.float32)))


def test_scores_from_untangle():
    #        G  TG  SS SD DS DD  L  NAN
    rows = [[2, 2, 3, 0, 0, 3, 3, 0],        # exact
            [1, 3, 2, 4, 0, 0, 5, 1],        # one big predicted group: recall 1, precision 1/3
            [6, 6, 0, 0, 0, 15, 0, 0],       # all singletons on both sides: P / R / F1 undefined
            [3, 2, 1, 1, 2, 6, 2, 0]]
    s = metrics.scores_from_untangle(rows)
    assert s["rand"] == (3 + 3 + 2 + 0 + 0 + 15 + 1 + 6) / (6 + 6 + 15 + 10)
    assert s["precision"] == 6 / 11 and s["recall"] == 6 / 8
    assert s["f1"] == 12 / (12 + 5 + 2)
    assert s["rand_mean"] == pytest.approx((1.0 + 2 / 6 + 1.0 + 0.7) / 4)
    assert s["precision_mean"] == pytest.approx((1.0 + 1 / 3 + 0.5) / 3)       # row 2 left out
    assert s["recall_mean"] == pytest.approx((1.0 + 1.0 + 1 / 3) / 3)
    assert s["f1_mean"] == pytest.approx((1.0 + 0.5 + 0.4) / 3)
    assert s["exact"] == 0.5 and s["group_count_match"] == 0.5 and s["nan_pairs"] == 1
    only = metrics.scores_from_untangle([rows[2]])
    assert only["rand"] == 1.0 and only["exact"] == 1.0
    for k in ("precision", "recall", "f1", "precision_mean", "recall_mean", "f1_mean"):
        assert math.isnan(only[k]), k
    empty = metrics.scores_from_untangle(np.zeros((0, 8), np.int64))
    assert math.isnan(empty["rand"]) and math.isnan(empty["exact"]) and empty["nan_pairs"] == 0


def test_python_mirrors_match_the_header():
    with open(os.path.join(ROOT, "include", "hdgnn.h")) as f:
        defs = dict(re.findall(r"#define\s+(HDG_UT_[A-Z_0-9]+)\s+(\d+)", f.read()))
    val = {k[len("HDG_"):]: int(v) for k, v in defs.items()}
    names = ["UT_SLOTS", "UT_GROUPS", "UT_TGROUPS", "UT_SS", "UT_SD", "UT_DS", "UT_DD", "UT_LINKS",
             "UT_NAN"]
    for n in names:
        assert val[n] == getattr(_lib, n) == getattr(metrics, n), n
    for n in ("UT_RULE_MEAN", "UT_RULE_ANY", "UT_RULE_BOTH", "UT_TILE", "UT_TILES_PER_BLOCK",
              "UT_MAX_BLOCKS"):
        assert val[n] == getattr(_lib, n), n
    assert len(val) == len(names) + 6               # nothing in the header without a mirror
    assert _lib.UT_RULES == {"mean": val["UT_RULE_MEAN"], "any": val["UT_RULE_ANY"],
                             "both": val["UT_RULE_BOTH"]}
    assert tuple(_lib.UT_RULES) == metrics.UT_RULES
    # blocks per commit, from the constants: the shapes the header comment names
    assert [_lib.untangle_blocks(n) for n in (2, 64, 74, 128, 129, 192, 193, 705, 2048)] == \
        [1, 1, 1, 1, 2, 2, 3, 16, 16]


def test_library_entry_points_reject_bad_arguments():
    """Host side of the C entry points (no device call is reached)."""
    import ctypes
    lib = _lib.load()
    ok = _lib.Shape(100, 200, 74, 2, 100, 0)
    assert lib.hdg_untangle_workspace_bytes(ctypes.byref(ok)) == 100 * 1 * (74 + 2) * 4
    big = _lib.Shape(32, 1024, 512, 2, 32, 0)
    assert lib.hdg_untangle_workspace_bytes(ctypes.byref(big)) == \
        32 * _lib.untangle_blocks(512) * (512 + 2) * 4
    for b, nc in ((0, 74), (65536, 74), (4, 1), (4, 2049)):
        bad = _lib.Shape(b, 200, nc, 2, 4, 0)
        assert lib.hdg_untangle_workspace_bytes(ctypes.byref(bad)) == 0
        assert b"must be in" in lib.hdg_last_error()
    one = ctypes.c_void_p(64)                       # never dereferenced: the checks come first
    bt = _lib.Batch(None, None, one, None, None, None)
    args = dict(probs=one, thr=0.5, rule=0, groups=one, ut=one, ws=one, shape=ok, bt=bt)

    def call(**kw):
        a = dict(args, **kw)
        return lib.hdg_untangle(ctypes.byref(a["shape"]), ctypes.byref(a["bt"]), a["probs"],
                                ctypes.c_float(a["thr"]), a["rule"], a["groups"], None, a["ut"],
                                a["ws"], None)

    einval = 1000
    assert call(rule=3) == einval and b"rule" in lib.hdg_last_error()
    assert call(rule=-1) == einval
    assert call(thr=float("nan")) == einval and b"NaN" in lib.hdg_last_error()
    for k in ("probs", "groups", "ut", "ws"):
        assert call(**{k: None}) == einval and b"NULL" in lib.hdg_last_error(), k
    assert call(bt=_lib.Batch(None, None, None, None, None, None)) == einval
    assert call(shape=_lib.Shape(0, 200, 74, 2, 1, 0)) == einval
    assert call(shape=_lib.Shape(4, 200, 2049, 2, 4, 0)) == einval
    assert b"nc must be" in lib.hdg_last_error()


# ---------------------------------------------------------------------------------------
# main.py --Type untangle (test_cli's recorder pattern)
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
        _Recorder.log.append(("untangle", args.Step, args.Nc, part, threshold, rule))


def _main():
    import importlib.util
    spec = importlib.util.spec_from_file_location("hdg_main_ut",
                                                  os.path.join(ROOT, "hd-gnn_amd", "main.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_main_type_untangle_reaches_model_untangle(tmp_path):
    cli = _main()
    _Recorder.log = []
    cli.main(["--Type", "untangle", "--checkpoint_dir", str(tmp_path)], model_cls=_Recorder)
    runs = [e for e in _Recorder.log if e[0] != "init"]
    assert runs == [("untangle", s, n, "test", 0.5, "mean")
                    for s, n in zip(cli.STEPS, cli.HUNK_NODES)]
    _Recorder.log = []
    cli.main(["--link-rule", "both", "--Type", "untangle", "--link-threshold", "0.25", "--model",
              "4", "--checkpoint_dir", str(tmp_path)], model_cls=_Recorder)
    runs = [e for e in _Recorder.log if e[0] != "init"]
    assert [r[4:] for r in runs] == [(0.25, "both")] * 3
    with pytest.raises(SystemExit):
        cli.main(["--Type", "untangle", "--link-rule", "most", "--checkpoint_dir", str(tmp_path)],
                 model_cls=_Recorder)
    # the other modes do not call it, and the reference parser does not know the new flags
    _Recorder.log = []
    cli.main(["--Type", "eval", "--checkpoint_dir", str(tmp_path)], model_cls=_Recorder)
    assert [e[0] for e in _Recorder.log if e[0] != "init"] == ["eval"] * 3
    parser = cli.build_parser(2, 200, 74, 39800, 5402)
    assert not [a for a in parser._actions if "link" in a.dest]
