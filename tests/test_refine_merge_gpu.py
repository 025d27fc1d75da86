"""hdg_refine_merge and hdg_refine_merge_ladder on the GPU: groups, ut and rq compared with the
host restatements (hdgnn.metrics.refine_merge, refine_merge_ladder) for integer equality, with
hdg_refine's own outputs where consequence (A) of include/hdgnn.h says they agree, and rung by
rung with hdg_cut then hdg_refine_merge.  No tolerances.  Buffers are poisoned before every
call and no poison may survive.

Shapes: nc 2 and 3, 33 (the label row crosses a word), the tile edges 64 / 65, 74 (the glide
shape), 129 (three tile rows; more slots than two waves own), B = 3 and all three rules; 1025,
the first nc at which a thread owns two hunks, B = 1, rule "mean".  Families: noisy planted
groups, uniform scores, the 1/256 grid (exact ties, pairs exactly on the bound), NaN in one
direction, infinite scores.  Starts: none, all zeros, the link graph's components at the same
threshold, and random ids with -7 and nc + 5 among them.  Budgets (max_sweeps, max_rounds):
(1, 1), (8, 1), (8, 4), (64, 16).
"""
import ctypes
import math
import types

import numpy as np
import pytest
import torch

from _decode import (B, T, _agglomerate_run, _cut, _linkage_run, _onehot, _planted, _probs,
                     _refine_run, _uniform, _with_infs, _with_nans)
from _ladder import LADDERS, ladder_run
from _merge import (BIG_MERGE_GAIN, BIG_NC, BIG_Q_END, MergeBufs, big_sums, merge_ladder_run,
                    merge_run, two_halves)
from hdgnn import _lib, data, layout, metrics
from hdgnn.synth import synth_commits
from test_refine import noisy_planted

pytestmark = pytest.mark.gpu

RULES = ("mean", "any", "both")
SHAPES = [2, 3, 33, T, T + 1, 74, 2 * T + 1]
TWO_PER_THREAD = 1025
BUDGETS = ((1, 1), (8, 1), (8, 4), (64, 16))
STARTS = ("none", "zeros", "untangle", "wild")
Q4 = [_lib.RF_Q_START, _lib.RF_Q_END, _lib.RF_Q_SWEEPS, _lib.RF_Q_CONVERGED]


def _noisy(nc):
    return noisy_planted(nc, seed=nc, B=B)


def _unif(nc):
    return _uniform(nc, seed=nc)


def _grid(nc):
    return _planted(nc, seed=nc)


def _nans(nc):
    return _with_nans(nc, B)[:2]


def _infs(nc):
    return _with_infs(*noisy_planted(nc, seed=50 + nc, B=B), seed=50 + nc)


FAMILIES = {"noisy": _noisy, "uniform": _unif, "grid": _grid, "nan": _nans, "inf": _infs}


def test_shapes_follow_from_the_header_constants():
    if T == 64:
        assert SHAPES == [2, 3, 33, 64, 65, 74, 129]
    assert TWO_PER_THREAD == 1024 + 1 and _lib.RM_MAX_ROUNDS == 16 and _lib.RM_Q_SLOTS == 8


def _start(which, y, p1, rule, rng):
    nb = len(p1)
    nc = int(round((1 + math.sqrt(1 + 4 * p1.shape[1])) / 2))
    if which == "none":
        return None
    if which == "zeros":
        return np.zeros((nb, nc), np.int32)
    if which == "untangle":
        return metrics.untangle_counts(_onehot(y), _probs(p1), 0.5, rule)[1].astype(np.int32)
    wild = rng.integers(0, max(2, nc // 3), (nb, nc)).astype(np.int32)
    wild[:, 0], wild[:, nc - 1] = -7, nc + 5
    return wild


def _same(dev, host, what=""):
    """(groups, ut, rq) of the device against (ut, groups, rq) of the host."""
    g, ut, rq = dev
    hut, hg, hrq = host
    np.testing.assert_array_equal(rq, hrq, what)
    np.testing.assert_array_equal(ut, hut, what)
    np.testing.assert_array_equal(g, hg, what)
    assert g.dtype == np.int32


def _one(what, y, p1, start, rule, ms, mr, thr=0.5):
    host = metrics.refine_merge(_onehot(y), _probs(p1), start, thr, rule, ms, mr)
    bufs, *dev = merge_run(y, p1, start, thr, rule, ms, mr)
    print(what, "device rq", dev[2].tolist())
    assert not bufs.any_poison(), what
    _same(dev, host, what)
    return host


# ---------------------------------------------------------------------------------------
# device == host
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", sorted(FAMILIES))
@pytest.mark.parametrize("nc", SHAPES)
def test_device_is_the_host_restatement(nc, family):
    y, p1 = FAMILIES[family](nc)
    rng = np.random.default_rng(nc)
    merges = 0
    for rule in RULES:
        for which in STARTS:
            start = _start(which, y, p1, rule, rng)
            for ms, mr in BUDGETS:
                host = _one("%s %d %s %s (%d, %d)" % (family, nc, rule, which, ms, mr), y, p1,
                            start, rule, ms, mr)
                merges += int(host[2][:, _lib.RM_Q_MERGES].sum())
    if nc >= 33:
        assert merges > 0                            # the group sweeps did act


@pytest.mark.parametrize("which", STARTS)
def test_two_hunks_per_thread(which):
    nc = TWO_PER_THREAD
    y, p1 = noisy_planted(nc, seed=nc, B=1, k=12)
    start = _start(which, y, p1, "mean", np.random.default_rng(nc))
    merges = 0
    for ms, mr in BUDGETS:
        host = _one("1025 %s (%d, %d)" % (which, ms, mr), y, p1, start, "mean", ms, mr)
        merges += int(host[2][:, _lib.RM_Q_MERGES].sum())
    assert merges > 0


# ---------------------------------------------------------------------------------------
# the two families of the definition
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("rule", RULES)
def test_tight_halves_merge_on_the_device(rule):
    y, p1, halves, planted = two_halves()
    _, g0, ut0, rq0 = _refine_run(y, p1, halves, 0.5, rule, 8)
    assert (ut0[:, _lib.RF_MOVES] == 0).all() and (rq0[:, _lib.RF_Q_CONVERGED] == 1).all()
    np.testing.assert_array_equal(g0, halves)
    host = _one("two_halves %s" % rule, y, p1, halves, rule, 8, 4)
    _, g, ut, rq = merge_run(y, p1, halves, 0.5, rule, 8, 4)
    np.testing.assert_array_equal(g, planted)
    assert (ut[:, _lib.UT_SD] == 0).all() and (ut[:, _lib.UT_DS] == 0).all()
    assert (rq[:, _lib.RF_Q_CONVERGED] == 1).all() and (rq[:, _lib.RM_Q_MERGES] == 3).all()
    assert (rq[:, _lib.RM_Q_ROUNDS] == 2).all()
    np.testing.assert_array_equal(rq[:, _lib.RM_Q_NODE], rq0[:, _lib.RF_Q_END])
    # from the device's own trees, cut above the threshold the objective is climbed at
    for method in ("single", "complete", "average"):
        _, (m, lv, cv, _, lk) = _agglomerate_run(y, p1, rule, method)
        start, _ = _cut(24, m, lv, cv, lk, 0.7, rule, ut=False)
        np.testing.assert_array_equal(start, halves)
    assert host[2].tolist() == rq.tolist()


def test_a_merge_gain_past_int32_on_the_device():
    y, p1, start = big_sums()
    _, g0, ut0, rq0 = _refine_run(y, p1, start, 0.5, "mean", 8)
    assert ut0[0, _lib.RF_MOVES] == 0 and rq0[0, _lib.RF_Q_CONVERGED] == 1
    _one("big sums", y, p1, start, "mean", 8, 4)
    _, g, ut, rq = merge_run(y, p1, start, 0.5, "mean", 8, 4)
    assert int(rq[0, _lib.RF_Q_END] - rq[0, _lib.RM_Q_NODE]) == BIG_MERGE_GAIN > 2 ** 31
    assert rq[0, _lib.RF_Q_END] == BIG_Q_END and rq[0, _lib.RM_Q_MERGES] == 1
    assert (g == 0).all() and g.shape == (1, BIG_NC) and rq[0, _lib.RM_Q_NODE] == rq0[0, 1]


# ---------------------------------------------------------------------------------------
# (A): the first node phase is hdg_refine's run, on the device's own outputs
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("nc", [33, 74, 2 * T + 1])
def test_first_node_phase_is_hdg_refine(nc):
    y, p1 = noisy_planted(nc, seed=300 + nc, B=B)
    rng = np.random.default_rng(nc)
    quiet = 0
    for rule in RULES:
        for which in STARTS:
            start = _start(which, y, p1, rule, rng)
            for thr in (0.5, 0.8):                   # at 0.8 few merges gain: quiet commits
                for ms in (1, 8):
                    _, g0, ut0, rq0 = _refine_run(y, p1, start, thr, rule, ms)
                    _, g, ut, rq = merge_run(y, p1, start, thr, rule, ms, 4)
                    np.testing.assert_array_equal(rq[:, _lib.RM_Q_NODE], rq0[:, _lib.RF_Q_END])
                    np.testing.assert_array_equal(rq[:, _lib.RF_Q_START], rq0[:, _lib.RF_Q_START])
                    assert (rq[:, _lib.RF_Q_END] - rq[:, _lib.RM_Q_NODE]
                            >= rq[:, _lib.RM_Q_MERGES]).all()                      # (B)
                    np.testing.assert_array_equal(ut[:, _lib.RF_NAN], ut0[:, _lib.RF_NAN])
                    for b in range(B):
                        if rq[b, _lib.RM_Q_MERGES] == 0:
                            quiet += 1
                            assert rq[b, _lib.RM_Q_ROUNDS] == 1
                            np.testing.assert_array_equal(g[b], g0[b])
                            np.testing.assert_array_equal(ut[b], ut0[b])
                            np.testing.assert_array_equal(rq[b, Q4], rq0[b])
    assert quiet > 0


# ---------------------------------------------------------------------------------------
# buffers and calls
# ---------------------------------------------------------------------------------------
def test_groups_may_be_groups_in_and_buffers_are_reused():
    nc = 74
    y, p1 = noisy_planted(nc, seed=901, B=B)
    start = _start("wild", y, p1, "mean", np.random.default_rng(1))
    host = metrics.refine_merge(_onehot(y), _probs(p1), start, 0.5, "mean", 8, 4)
    bufs, *first = merge_run(y, p1, start, 0.5, "mean", 8, 4)
    _same(first, host)
    _, *again = merge_run(y, p1, start, 0.5, "mean", 8, 4, bufs=bufs, alias=True)
    _same(again, host, "groups is groups_in")
    y3, p3 = _uniform(nc, seed=902)                              # other inputs, same buffers
    p3[0, :nc - 1] = np.nan
    _, *other = merge_run(y3, p3, None, 0.4, "both", 2, 16, bufs=bufs)
    _same(other, metrics.refine_merge(_onehot(y3), _probs(p3), None, 0.4, "both", 2, 16))


def test_argument_errors_launch_nothing():
    lib = _lib.load()
    dev = torch.device("cuda")
    nc, n = 10, 5
    one, lad = MergeBufs(B, nc, dev), MergeBufs(B, nc, dev, rungs=n)
    ybits = torch.zeros(B, nc, 1, dtype=torch.int32, device=dev)
    pt = torch.rand(B, 2, nc * (nc - 1), device=dev)
    tm = torch.full((B, nc - 1, 2), -1, dtype=torch.int32, device=dev)
    tl = torch.full((B, nc - 1), float("nan"), device=dev)
    vp = ctypes.c_void_p
    base = dict(shape=_lib.Shape(B, 20, nc, 2, B, 0),
                bt=_lib.Batch(None, None, ybits.data_ptr(), None, None, None),
                probs=vp(pt.data_ptr()), rule=0, ms=8, mr=4, flags=0)

    def stream():
        return vp(torch.cuda.current_stream(dev).cuda_stream)

    def call(**kw):
        a = dict(base, thr=0.5, gin=None, groups=vp(one.groups.data_ptr()),
                 ut=vp(one.ut.data_ptr()), rq=vp(one.rq.data_ptr()), ws=vp(one.ws.data_ptr()))
        a.update(kw)
        return lib.hdg_refine_merge(ctypes.byref(a["shape"]), ctypes.byref(a["bt"]), a["probs"],
                                    ctypes.c_float(a["thr"]), a["rule"], a["ms"], a["mr"],
                                    a["flags"], a["gin"], a["groups"], a["ut"], a["rq"], a["ws"],
                                    stream())

    def lcall(**kw):
        a = dict(base, thr=[0.1, 0.3, 0.5, 0.7, 0.9], n=None, merges=vp(tm.data_ptr()),
                 levels=vp(tl.data_ptr()), groups=vp(lad.groups.data_ptr()),
                 ut=vp(lad.ut.data_ptr()), rq=vp(lad.rq.data_ptr()), ws=vp(lad.ws.data_ptr()))
        a.update(kw)
        thr = a["thr"]
        k = a["n"] if a["n"] is not None else len(thr)
        arr = None if thr is None else (ctypes.c_float * max(1, len(thr)))(*thr)
        return lib.hdg_refine_merge_ladder(ctypes.byref(a["shape"]), ctypes.byref(a["bt"]),
                                           a["probs"], arr, k, a["rule"], a["ms"], a["mr"],
                                           a["flags"], a["merges"], a["levels"], a["groups"],
                                           a["ut"], a["rq"], a["ws"], stream())

    nan, inf = float("nan"), float("inf")
    both = [dict(rule=3), dict(rule=-1), dict(ms=0), dict(ms=65), dict(mr=0), dict(mr=17),
            dict(mr=-1), dict(flags=1), dict(flags=-1), dict(probs=None), dict(ut=None),
            dict(rq=None), dict(ws=None),
            dict(bt=_lib.Batch(None, None, None, None, None, None)),
            dict(shape=_lib.Shape(0, 20, nc, 2, B, 0)), dict(shape=_lib.Shape(B, 20, 1, 2, B, 0)),
            dict(shape=_lib.Shape(B, 20, 2049, 2, B, 0))]
    for kw in both + [dict(thr=nan), dict(thr=inf), dict(thr=3e38), dict(groups=None),
                      dict(ws=vp(one.ws.data_ptr() + 4))]:
        assert call(**kw) == 1000, kw
        assert lib.hdg_last_error().startswith(b"hdg_refine_merge:"), kw
    for kw in both + [dict(n=0), dict(n=65, thr=[0.5] * 65), dict(thr=None, n=5),
                      dict(thr=[0.1, 0.3, 0.5, nan, 0.9]), dict(thr=[0.1, 3e38, 0.5, 0.7, 0.9]),
                      dict(levels=None), dict(merges=None), dict(ws=vp(lad.ws.data_ptr() + 4))]:
        assert lcall(**kw) == 1000, kw
        assert lib.hdg_last_error().startswith(b"hdg_refine_merge_ladder:"), kw
    assert lcall(thr=[0.1, 0.3, 0.5, nan, 0.9]) == 1000 and b"rung 3" in lib.hdg_last_error()
    torch.cuda.synchronize(dev)
    assert one.poisoned() and lad.poisoned()
    assert call() == 0 and lcall() == 0 and lcall(merges=None, levels=None, groups=None) == 0
    torch.cuda.synchronize(dev)
    assert not one.any_poison() and not lad.any_poison()
    assert (one.rq[..., _lib.RM_Q_ROUNDS] >= 1).all() and (lad.rq[..., 7] == 0).all()


# ---------------------------------------------------------------------------------------
# the ladder: device == host loop == hdg_cut + hdg_refine_merge per rung
# ---------------------------------------------------------------------------------------
def _tree(y, p1, rule, start):
    if start == "none":
        return None
    if start == "linkage":
        _, (m, lv, cv, _, lk) = _linkage_run(y, p1, rule)
    else:
        _, (m, lv, cv, _, lk) = _agglomerate_run(y, p1, rule, start)
    return m, lv, cv, lk


def _sequences(y, p1, thresholds, tree, rule, ms, mr):
    nc = int(round((1 + math.sqrt(1 + 4 * p1.shape[1])) / 2))
    out = []
    for t in thresholds:
        start = None
        if tree is not None:
            start, _ = _cut(nc, tree[0], tree[1], tree[2], tree[3], float(t), rule, ut=False)
        out.append(merge_run(y, p1, start, float(t), rule, ms, mr)[1:])
    return tuple(np.stack([o[i] for o in out]) for i in range(3))


@pytest.mark.parametrize("nc", [3, 33, T + 1, 74])
def test_ladder_is_cut_then_refine_merge_per_rung(nc):
    y, p1 = noisy_planted(nc, seed=nc, B=B)
    k = 0
    for rule in RULES:
        for start in ("none", "linkage", "complete", "average"):
            thr = LADDERS[k % len(LADDERS)]
            ms, mr = BUDGETS[(k + k // 4) % len(BUDGETS)]
            k += 1
            tree = _tree(y, p1, rule, start)
            what = "%d %s %s T=%d (%d, %d)" % (nc, rule, start, len(thr), ms, mr)
            host = metrics.refine_merge_ladder(_onehot(y), _probs(p1), thr,
                                               None if tree is None else tree[:2], rule, ms, mr)
            bufs, *dev = merge_ladder_run(y, p1, thr, None if tree is None else tree[:2], rule,
                                          ms, mr)
            assert not bufs.any_poison(), what
            _same(dev, host, what)
            for x, z in zip(dev, _sequences(y, p1, thr, tree, rule, ms, mr)):
                np.testing.assert_array_equal(x, z, what)
            bufs, g0, ut0, rq0 = merge_ladder_run(y, p1, thr, None if tree is None else tree[:2],
                                                  rule, ms, mr, groups=False)
            assert (g0 == -7).all() and not bool((bufs.ut == -1).any() or (bufs.rq == -99).any())
            np.testing.assert_array_equal(ut0, dev[1], what)
            np.testing.assert_array_equal(rq0, dev[2], what)


def test_ladder_on_the_tight_halves():
    """From singletons the node moves build the halves at every rung and stop there
    (hdg_refine_ladder); with rounds the rung at 0.5 joins them."""
    y, p1, halves, planted = two_halves()
    thr = [0.7, 0.5, 0.6]
    _, g0, _, _ = ladder_run(y, p1, thr, None, "mean", 8)
    for k in range(3):
        np.testing.assert_array_equal(g0[k], halves)
    _, g, ut, rq = merge_ladder_run(y, p1, thr, None, "mean", 8, 4)
    _same((g, ut, rq), metrics.refine_merge_ladder(_onehot(y), _probs(p1), thr, None))
    np.testing.assert_array_equal(g[0], halves)          # at 0.7 the halves do not attract
    np.testing.assert_array_equal(g[1], planted)
    assert (rq[1][:, _lib.RM_Q_MERGES] == 3).all() and (rq[0][:, _lib.RM_Q_MERGES] == 0).all()


# ---------------------------------------------------------------------------------------
# Engine
# ---------------------------------------------------------------------------------------
def _engine(seed):
    from hdgnn.engine import Engine
    ne, nc, b = 20, 10, 4
    cb = synth_commits(b, ne, nc, seed)
    eng = Engine(ne, nc, b, variant=2)
    eng.set_params(layout.init_flat(5, 2))
    return eng, eng.upload(cb), data.onehot_relations(cb.y), nc, b


def test_engine_refine_merge_end_to_end():
    eng, db, label, nc, b = _engine(43)
    probs, _, _ = eng.forward(db)
    g0, _ = eng.untangle(db)
    out = eng.refine_merge(db, g0, max_sweeps=8, max_rounds=4)
    g, ut, rq = out
    assert all(x.is_cuda for x in out)
    assert g.dtype == torch.int32 and tuple(g.shape) == (b, nc)
    assert ut.dtype == torch.int64 and tuple(ut.shape) == (b, _lib.RF_SLOTS)
    assert rq.dtype == torch.int64 and tuple(rq.shape) == (b, _lib.RM_Q_SLOTS)
    host = metrics.refine_merge(label, probs.cpu().numpy(), g0.cpu().numpy(), 0.5, "mean", 8, 4)
    _same((g.cpu().numpy(), ut.cpu().numpy(), rq.cpu().numpy()), host)
    ws = eng._rf_workspace
    fake = torch.rand_like(probs)
    for rule in RULES:
        for start in (None, g0):
            g, ut, rq = eng.refine_merge(db, start, fake, threshold=0.45, rule=rule,
                                         max_sweeps=2, max_rounds=16)
            host = metrics.refine_merge(label, fake.cpu().numpy(),
                                        None if start is None else start.cpu().numpy(), 0.45,
                                        rule, 2, 16)
            _same((g.cpu().numpy(), ut.cpu().numpy(), rq.cpu().numpy()), host)
    plain = eng.refine(db, g0, fake)                              # refine() is what it was
    assert tuple(plain[2].shape) == (b, _lib.RF_Q_SLOTS) and eng._rf_workspace is ws
    thr = [0.3, 0.6]
    tree = eng.agglomerate(db, fake, "mean", "average")[:2]
    lut, lrq, lg = eng.refine_merge_ladder(db, thr, tree, fake, max_sweeps=4, max_rounds=2,
                                           groups=True)
    assert tuple(lrq.shape) == (2, b, _lib.RM_Q_SLOTS) and tuple(lg.shape) == (2, b, nc)
    host = metrics.refine_merge_ladder(label, fake.cpu().numpy(), thr,
                                       (tree[0].cpu().numpy(), tree[1].cpu().numpy()), "mean", 4, 2)
    _same((lg.cpu().numpy(), lut.cpu().numpy(), lrq.cpu().numpy()), host)
    assert eng.refine_merge_ladder(db, thr, tree, fake)[2] is None
    for kw in (dict(max_rounds=0), dict(max_rounds=17), dict(max_rounds=2.0), dict(max_sweeps=0),
               dict(max_sweeps=65), dict(rule="most"), dict(groups=g0.long()),
               dict(groups=g0[:, :-1]), dict(groups=g0.cpu()), dict(probs=fake[:, :, :-1])):
        with pytest.raises(ValueError):
            eng.refine_merge(db, **kw)
    for kw in (dict(max_rounds=0), dict(max_rounds=17), dict(thresholds=[]), dict(tree=(tree[0],))):
        with pytest.raises(ValueError):
            eng.refine_merge_ladder(db, **dict(dict(thresholds=thr), **kw))
    eng.check_status()


def test_merge_ladder_is_graph_capturable():
    """Tree and ladder replay from a captured graph on new scores, with the captured rungs."""
    eng, db, label, nc, b = _engine(44)
    scores = torch.rand(b, 2, nc * (nc - 1), device=eng.device)
    thr = [0.6, 0.3, 0.45]

    def np3(out):
        ut, rq, g = out
        return g.cpu().numpy(), ut.cpu().numpy(), rq.cpu().numpy()

    tree = eng.agglomerate(db, scores, "any", "average")[:2]     # warm: workspaces allocated
    eng.refine_merge_ladder(db, thr, tree, scores, rule="any", groups=True)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        tree = eng.agglomerate(db, scores, "any", "average")[:2]
        out = eng.refine_merge_ladder(db, thr, tree, scores, rule="any", groups=True)
    for _ in range(2):
        scores.copy_(torch.rand_like(scores))
        graph.replay()
        torch.cuda.synchronize()
        replayed = np3(out)
        eager = np3(eng.refine_merge_ladder(db, thr,
                                            eng.agglomerate(db, scores, "any", "average")[:2],
                                            scores, rule="any", groups=True))
        for x, z in zip(replayed, eager):
            np.testing.assert_array_equal(x, z)
        host = metrics.refine_merge_ladder(label, scores.cpu().numpy(), thr,
                                           (tree[0].cpu().numpy(), tree[1].cpu().numpy()), "any")
        _same(replayed, host)


def test_graph2graph_untangle_and_calibrate_with_merge(golden_dir, tmp_path, monkeypatch, capsys):
    from hdgnn.model import graph2graph
    from test_model_gpu import _tuple
    tup, meta = _tuple(golden_dir)
    ne, nc, mb = meta["Ne"], meta["Nc"], 25
    monkeypatch.chdir(tmp_path)
    args = types.SimpleNamespace(Repo="tiny", checkpoint_dir=str(tmp_path / "ckpt"))
    m = graph2graph(None, Ds=1, Ne=ne, Nc=nc, Ner=ne * (ne - 1), Ncr=nc * (nc - 1), Dr=2,
                    De_e=20, De_er=20, Mini_batch=mb, checkpoint_dir=args.checkpoint_dir,
                    epoch=2, Ds_inter=1, Dr_inter=2, Step=2, Repo="tiny",
                    reader=lambda mm, step: tup, seed=7)
    m.train(args)
    capsys.readouterr()
    d = tmp_path / "outputSelf" / "tiny" / "model_2" / "2"
    lad, sweeps, rounds = (0.3, 0.7, 5), 4, 3
    thr, scores, rungs, table, rq = m.calibrate_refined(args, part="train", method="average",
                                                        refine=sweeps, ladder=lad, merge=rounds)
    out = capsys.readouterr().out
    n = table.shape[1]
    assert n > 0 and table.shape == (5, n, 8) and rq.shape == (5, n, _lib.RM_Q_SLOTS)
    train, _, maps = data.compact_from_read_data(tup, ne, nc, mb)
    want = []
    for j, db in enumerate(m._device_batches(train, maps)):
        label = data.onehot_relations(train.y[j * mb:(j + 1) * mb])
        probs = m.engine.forward(db)[0].cpu().numpy()
        tree = metrics.agglomerate(label, probs, "mean", "average")
        want.append(metrics.refine_merge_ladder(label, probs, rungs, tree[:2], "mean", sweeps,
                                                rounds))
    hut = np.concatenate([w[0] for w in want], 1)
    hrq = np.concatenate([w[2] for w in want], 1)
    np.testing.assert_array_equal(table, hut)
    np.testing.assert_array_equal(rq, hrq)
    np.testing.assert_array_equal(np.load(d / ("refine_ladder_objective%d.npy" % ne)), rq)
    for j in range(5):
        assert ("calibrate refined rung %d merge: %d rounds, %d merges, objective after the first "
                "node phase %d -> %d at the end"
                % (j, hrq[j, :, _lib.RM_Q_ROUNDS].sum(), hrq[j, :, _lib.RM_Q_MERGES].sum(),
                   hrq[j, :, _lib.RM_Q_NODE].sum(), hrq[j, :, _lib.RF_Q_END].sum())) in out
    k = metrics.best_rung(hut, rungs, "f1")[0]
    _, t1, _ = m.untangle(args, part="train", threshold=thr, method="average", refine=sweeps,
                          merge=rounds)
    out = capsys.readouterr().out
    np.testing.assert_array_equal(t1, table[k])
    q = np.load(d / ("untangle_refine%d.npy" % ne))
    np.testing.assert_array_equal(q, rq[k])
    assert ("untangle merge: %d rounds at most, %d rounds, %d merges, objective after the first "
            "node phase %d -> %d at the end"
            % (rounds, q[:, _lib.RM_Q_ROUNDS].sum(), q[:, _lib.RM_Q_MERGES].sum(),
               q[:, _lib.RM_Q_NODE].sum(), q[:, _lib.RF_Q_END].sum())) in out
    # without merge both are what they were: four columns, no line about merges
    _, t0, _ = m.untangle(args, part="train", threshold=thr, method="average", refine=sweeps)
    assert "merge" not in capsys.readouterr().out
    assert np.load(d / ("untangle_refine%d.npy" % ne)).shape == (n, _lib.RF_Q_SLOTS)
    for kw in (dict(merge=17), dict(merge=-1), dict(merge=1.0), dict(merge=2, refine=0)):
        with pytest.raises(ValueError):
            m.untangle(args, **kw)
    for kw in (dict(merge=17), dict(merge=-1)):
        with pytest.raises(ValueError):
            m.calibrate_refined(args, **kw)
