"""hdg_refine_split and hdg_refine_split_ladder on the GPU: groups, ut and rq compared with the
host restatements (hdgnn.metrics.refine_split, refine_split_ladder) for integer equality, with
hdg_refine_merge's own outputs where consequence (A) of include/hdgnn.h says they agree, and
rung by rung with hdg_cut then hdg_refine_split.  No tolerances.  Buffers are poisoned before
every call and no poison may survive.

Shapes, families and starts are test_refine_merge_gpu.py's: nc 2 and 3, 33, the tile edges 64 /
65, 74, 129 (more slots than two waves own), B = 3 and all three rules; 1025, the first nc at
which a thread owns two hunks, B = 1, rule "mean".  kinds split and both; budgets (max_sweeps,
max_rounds): (1, 1), (8, 4), (64, 16).  The fused groups of _split.py at nc 24, 66 (a group of
22 hunks spans the slots of two waves), 132 and 1026 (a group's members on both of a thread's
hunks), and the split whose gain is past int32.

"The split sweeps did act" is asserted only where the host restatement alone shows a split
(test_refine_split.py checks these on the CPU): two_fused, always (test_split_sweeps_cut_the_
fused_groups_nothing_else_can), and noisy_planted(74, seed=5, B=4, k=8) from the link graph's
components at 0.55 (test_noisy_components_start_splits_and_never_lowers_q).
"""
import ctypes
import math
import types

import numpy as np
import pytest
import torch

from _decode import B, T, _cut, _onehot, _probs, _refine_run, _uniform
from _ladder import LADDERS
from _merge import MergeBufs, merge_ladder_run, merge_run
from _split import (BIG_NC, BIG_Q_END, BIG_Q_START, BIG_SPLIT_GAIN, KINDS, big_split, split_ladder_run,
                    split_run, two_fused)
from hdgnn import _lib, data, metrics
from test_refine import noisy_planted
from test_refine_merge_gpu import (FAMILIES, RULES, SHAPES, STARTS, TWO_PER_THREAD, _engine, _same,
                                   _start, _tree)

pytestmark = pytest.mark.gpu

BUDGETS = ((1, 1), (8, 4), (64, 16))
SPLITS = _lib.RS_Q_SPLITS


def test_shapes_follow_from_the_header_constants():
    if T == 64:
        assert SHAPES == [2, 3, 33, 64, 65, 74, 129]
    assert TWO_PER_THREAD == 1024 + 1 and _lib.RS_PASSES == 4 and _lib.RS_Q_SLOTS == 8
    assert KINDS == {"merge": 1, "split": 2, "both": 3}


def _one(what, y, p1, start, rule, ms, mr, kinds, thr=0.5):
    host = metrics.refine_split(_onehot(y), _probs(p1), start, thr, rule, ms, mr, kinds)
    bufs, *dev = split_run(y, p1, start, thr, rule, ms, mr, kinds)
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
    for rule in RULES:
        for which in STARTS:
            start = _start(which, y, p1, rule, rng)
            for ms, mr in BUDGETS:
                for kinds in ("split", "both"):
                    _one("%s %d %s %s (%d, %d) %s" % (family, nc, rule, which, ms, mr, kinds), y,
                         p1, start, rule, ms, mr, KINDS[kinds])


@pytest.mark.parametrize("which", STARTS)
def test_two_hunks_per_thread(which):
    nc = TWO_PER_THREAD
    y, p1 = noisy_planted(nc, seed=nc, B=1, k=12)
    start = _start(which, y, p1, "mean", np.random.default_rng(nc))
    for ms, mr in BUDGETS:
        _one("1025 %s (%d, %d) both" % (which, ms, mr), y, p1, start, "mean", ms, mr, 3)
    _one("1025 %s (8, 4) split" % which, y, p1, start, "mean", 8, 4, 2)


def test_the_noisy_components_start_splits_on_the_device():
    y, p1 = noisy_planted(74, seed=5, B=4, k=8)
    start = metrics.untangle_counts(_onehot(y), _probs(p1), 0.55, "mean")[1].astype(np.int32)
    host = _one("noisy 74 components 0.55", y, p1, start, "mean", 8, 4, 3, thr=0.55)
    assert host[2][:, SPLITS].sum() > 0              # the host alone shows it (see the docstring)


# ---------------------------------------------------------------------------------------
# the two families of the definition
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("nc", [24, 66, 132, 1026])
def test_fused_groups_are_cut_on_the_device(nc):
    nb = 1 if nc > 1024 else 4
    y, p1, halves, fused = two_fused(nc, B=nb)
    for rule in RULES if nc <= 1024 else ("mean",):
        _, g0, ut0, rq0 = _refine_run(y, p1, fused, 0.5, rule, 8)
        assert (ut0[:, _lib.RF_MOVES] == 0).all() and (rq0[:, _lib.RF_Q_CONVERGED] == 1).all()
        np.testing.assert_array_equal(g0, fused)
        _, gm, utm, rqm = merge_run(y, p1, fused, 0.5, rule, 8, 4)
        np.testing.assert_array_equal(gm, fused)
        assert (rqm[:, _lib.RM_Q_MERGES] == 0).all() and (rqm[:, SPLITS] == 0).all()
        for kinds in ("split", "both"):
            host = _one("two_fused %d %s %s" % (nc, rule, kinds), y, p1, fused, rule, 8, 4,
                        KINDS[kinds])
            g, rq = host[1], host[2]                 # the device's, integer for integer
            np.testing.assert_array_equal(g, halves)
            assert (host[0][:, _lib.UT_SD] == 0).all() and (host[0][:, _lib.UT_DS] == 0).all()
            assert (rq[:, SPLITS] == 3).all() and (rq[:, _lib.RM_Q_ROUNDS] == 2).all()
            assert (rq[:, _lib.RF_Q_CONVERGED] == 1).all()
            np.testing.assert_array_equal(rq[:, _lib.RM_Q_NODE], rq0[:, _lib.RF_Q_END])


def test_a_split_gain_past_int32_on_the_device():
    y, p1, start = big_split()
    _, g0, ut0, rq0 = _refine_run(y, p1, start, 0.5, "mean", 8)
    assert ut0[0, _lib.RF_MOVES] == 0 and rq0[0].tolist() == [BIG_Q_START, BIG_Q_START, 1, 1]
    for kinds in (2, 3):
        _one("big split", y, p1, start, "mean", 8, 4, kinds)
        _, g, ut, rq = split_run(y, p1, start, 0.5, "mean", 8, 4, kinds)
        assert int(rq[0, _lib.RF_Q_END] - rq[0, _lib.RM_Q_NODE]) == BIG_SPLIT_GAIN > 2 ** 31
        assert rq[0].tolist() == [BIG_Q_START, BIG_Q_END, 2, 1, 2, 0, BIG_Q_START, 1]
        np.testing.assert_array_equal(g[0], np.arange(BIG_NC) % 2)


# ---------------------------------------------------------------------------------------
# (A): kinds merge is hdg_refine_merge, on the device's own outputs
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("nc", [33, 74, 2 * T + 1])
def test_kinds_merge_is_hdg_refine_merge(nc):
    y, p1 = noisy_planted(nc, seed=300 + nc, B=B)
    rng = np.random.default_rng(nc)
    for rule in RULES:
        for which in STARTS:
            start = _start(which, y, p1, rule, rng)
            for ms, mr in ((1, 1), (8, 4)):
                _, g0, ut0, rq0 = _refine_run(y, p1, start, 0.5, rule, ms)
                bm, *merged = merge_run(y, p1, start, 0.5, rule, ms, mr)
                bs, *as_merge = split_run(y, p1, start, 0.5, rule, ms, mr, 1)
                assert not bs.any_poison()
                for a, c in zip(as_merge, merged):
                    np.testing.assert_array_equal(a, c)
                assert (as_merge[2][:, SPLITS] == 0).all()
                for kinds in (2, 3):                                       # (B), (C)
                    _, g, ut, rq = split_run(y, p1, start, 0.5, rule, ms, mr, kinds)
                    np.testing.assert_array_equal(rq[:, _lib.RM_Q_NODE], rq0[:, _lib.RF_Q_END])
                    assert (rq[:, _lib.RF_Q_END] - rq[:, _lib.RM_Q_NODE]
                            >= rq[:, _lib.RM_Q_MERGES] + rq[:, SPLITS]).all()
                    np.testing.assert_array_equal(ut[:, _lib.RF_NAN], ut0[:, _lib.RF_NAN])


# ---------------------------------------------------------------------------------------
# buffers and calls
# ---------------------------------------------------------------------------------------
def test_groups_may_be_groups_in_and_buffers_are_reused():
    y, p1, halves, fused = two_fused(66, B=B)
    host = metrics.refine_split(_onehot(y), _probs(p1), fused, 0.5, "mean", 8, 4, 3)
    bufs, *first = split_run(y, p1, fused, 0.5, "mean", 8, 4, 3)
    _same(first, host)
    _, *again = split_run(y, p1, fused, 0.5, "mean", 8, 4, 3, bufs=bufs, alias=True)
    _same(again, host, "groups is groups_in")
    np.testing.assert_array_equal(again[0], halves)
    nc = 66
    y3, p3 = _uniform(nc, seed=902)                              # other inputs, same buffers
    p3[0, :nc - 1] = np.nan
    start = _start("wild", y3, p3, "both", np.random.default_rng(1))
    _, *other = split_run(y3, p3, start, 0.4, "both", 2, 16, 2, bufs=bufs, alias=True)
    _same(other, metrics.refine_split(_onehot(y3), _probs(p3), start, 0.4, "both", 2, 16, 2))


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
                probs=vp(pt.data_ptr()), rule=0, ms=8, mr=4, kinds=3, flags=0)

    def stream():
        return vp(torch.cuda.current_stream(dev).cuda_stream)

    def call(**kw):
        a = dict(base, thr=0.5, gin=None, groups=vp(one.groups.data_ptr()),
                 ut=vp(one.ut.data_ptr()), rq=vp(one.rq.data_ptr()), ws=vp(one.ws.data_ptr()))
        a.update(kw)
        return lib.hdg_refine_split(ctypes.byref(a["shape"]), ctypes.byref(a["bt"]), a["probs"],
                                    ctypes.c_float(a["thr"]), a["rule"], a["ms"], a["mr"],
                                    a["kinds"], a["flags"], a["gin"], a["groups"], a["ut"],
                                    a["rq"], a["ws"], stream())

    def lcall(**kw):
        a = dict(base, thr=[0.1, 0.3, 0.5, 0.7, 0.9], n=None, merges=vp(tm.data_ptr()),
                 levels=vp(tl.data_ptr()), groups=vp(lad.groups.data_ptr()),
                 ut=vp(lad.ut.data_ptr()), rq=vp(lad.rq.data_ptr()), ws=vp(lad.ws.data_ptr()))
        a.update(kw)
        thr = a["thr"]
        k = a["n"] if a["n"] is not None else len(thr)
        arr = None if thr is None else (ctypes.c_float * max(1, len(thr)))(*thr)
        return lib.hdg_refine_split_ladder(ctypes.byref(a["shape"]), ctypes.byref(a["bt"]),
                                           a["probs"], arr, k, a["rule"], a["ms"], a["mr"],
                                           a["kinds"], a["flags"], a["merges"], a["levels"],
                                           a["groups"], a["ut"], a["rq"], a["ws"], stream())

    nan = float("nan")
    both = [dict(kinds=0), dict(kinds=4), dict(kinds=-1), dict(flags=1), dict(flags=-1),
            dict(mr=0), dict(mr=17), dict(rule=3), dict(ms=0), dict(ms=65), dict(probs=None),
            dict(ut=None), dict(rq=None), dict(ws=None),
            dict(bt=_lib.Batch(None, None, None, None, None, None)),
            dict(shape=_lib.Shape(B, 20, 1, 2, B, 0)), dict(shape=_lib.Shape(B, 20, 2049, 2, B, 0))]
    for kw in both + [dict(thr=nan), dict(thr=3e38), dict(groups=None),
                      dict(ws=vp(one.ws.data_ptr() + 4))]:
        assert call(**kw) == 1000, kw
        assert lib.hdg_last_error().startswith(b"hdg_refine_split:"), kw
    for kw in both + [dict(n=0), dict(n=65, thr=[0.5] * 65), dict(thr=None, n=5),
                      dict(thr=[0.1, 0.3, 0.5, nan, 0.9]), dict(levels=None), dict(merges=None),
                      dict(ws=vp(lad.ws.data_ptr() + 4))]:
        assert lcall(**kw) == 1000, kw
        assert lib.hdg_last_error().startswith(b"hdg_refine_split_ladder:"), kw
    torch.cuda.synchronize(dev)
    assert one.poisoned() and lad.poisoned()
    assert call() == 0 and lcall() == 0 and lcall(merges=None, levels=None, groups=None) == 0
    torch.cuda.synchronize(dev)
    assert not one.any_poison() and not lad.any_poison()
    assert (one.rq[..., _lib.RM_Q_ROUNDS] >= 1).all() and (lad.rq[..., SPLITS] >= 0).all()


# ---------------------------------------------------------------------------------------
# the ladder: device == host loop == hdg_cut + hdg_refine_split per rung
# ---------------------------------------------------------------------------------------
def _sequences(y, p1, thresholds, tree, rule, ms, mr, kinds):
    nc = int(round((1 + math.sqrt(1 + 4 * p1.shape[1])) / 2))
    out = []
    for t in thresholds:
        start = None
        if tree is not None:
            start, _ = _cut(nc, tree[0], tree[1], tree[2], tree[3], float(t), rule, ut=False)
        out.append(split_run(y, p1, start, float(t), rule, ms, mr, kinds)[1:])
    return tuple(np.stack([o[i] for o in out]) for i in range(3))


@pytest.mark.parametrize("nc", [3, 33, T + 1, 74])
def test_ladder_is_cut_then_refine_split_per_rung(nc):
    y, p1 = noisy_planted(nc, seed=nc, B=B)
    k = 0
    for rule in RULES:
        for start in ("none", "linkage", "complete", "average"):
            thr = LADDERS[k % len(LADDERS)]
            ms, mr = BUDGETS[(k + k // 4) % len(BUDGETS)]
            kinds = (3, 2)[k % 2]
            k += 1
            tree = _tree(y, p1, rule, start)
            what = "%d %s %s T=%d (%d, %d) %d" % (nc, rule, start, len(thr), ms, mr, kinds)
            host = metrics.refine_split_ladder(_onehot(y), _probs(p1), thr,
                                               None if tree is None else tree[:2], rule, ms, mr,
                                               kinds)
            bufs, *dev = split_ladder_run(y, p1, thr, None if tree is None else tree[:2], rule,
                                          ms, mr, kinds)
            assert not bufs.any_poison(), what
            _same(dev, host, what)
            for x, z in zip(dev, _sequences(y, p1, thr, tree, rule, ms, mr, kinds)):
                np.testing.assert_array_equal(x, z, what)
            bufs, g0, ut0, rq0 = split_ladder_run(y, p1, thr, None if tree is None else tree[:2],
                                                  rule, ms, mr, kinds, groups=False)
            assert (g0 == -7).all() and not bool((bufs.ut == -1).any() or (bufs.rq == -99).any())
            np.testing.assert_array_equal(ut0, dev[1], what)
            np.testing.assert_array_equal(rq0, dev[2], what)
    # kinds merge is the merge ladder, on the device's own outputs
    tree = _tree(y, p1, "mean", "linkage")
    for x, z in zip(split_ladder_run(y, p1, LADDERS[0], tree[:2], "mean", 8, 4, 1)[1:],
                    merge_ladder_run(y, p1, LADDERS[0], tree[:2], "mean", 8, 4)[1:]):
        np.testing.assert_array_equal(x, z)


def test_ladder_on_the_fused_groups():
    """Single linkage's tree fuses the halves at every rung below the wrong pair's level; the
    rung at 0.5 cuts them again, and only split sweeps can."""
    y, p1, halves, fused = two_fused()
    tree = _tree(y, p1, "mean", "linkage")
    thr = [0.5, 0.3]
    _, gm, _, rqm = merge_ladder_run(y, p1, thr, tree[:2], "mean", 8, 4)
    np.testing.assert_array_equal(gm[0], fused)
    _, g, ut, rq = split_ladder_run(y, p1, thr, tree[:2], "mean", 8, 4, 3)
    _same((g, ut, rq), metrics.refine_split_ladder(_onehot(y), _probs(p1), thr, tree[:2]))
    np.testing.assert_array_equal(g[0], halves)
    assert (rq[0][:, SPLITS] == 3).all() and (rqm[0][:, SPLITS] == 0).all()


# ---------------------------------------------------------------------------------------
# Engine
# ---------------------------------------------------------------------------------------
def test_engine_refine_split_end_to_end():
    eng, db, label, nc, b = _engine(43)
    probs, _, _ = eng.forward(db)
    g0, _ = eng.untangle(db)
    out = eng.refine_split(db, g0, max_sweeps=8, max_rounds=4)
    g, ut, rq = out
    assert all(x.is_cuda for x in out)
    assert g.dtype == torch.int32 and tuple(g.shape) == (b, nc)
    assert ut.dtype == torch.int64 and tuple(ut.shape) == (b, _lib.RF_SLOTS)
    assert rq.dtype == torch.int64 and tuple(rq.shape) == (b, _lib.RS_Q_SLOTS)
    host = metrics.refine_split(label, probs.cpu().numpy(), g0.cpu().numpy(), 0.5, "mean", 8, 4, 3)
    _same((g.cpu().numpy(), ut.cpu().numpy(), rq.cpu().numpy()), host)
    ws = eng._rf_workspace
    fake = torch.rand_like(probs)
    zeros = torch.zeros_like(g0)
    for rule in RULES:
        for start in (None, g0, zeros):
            for kinds in KINDS:
                g, ut, rq = eng.refine_split(db, start, fake, threshold=0.45, rule=rule,
                                             max_sweeps=2, max_rounds=16, kinds=kinds)
                host = metrics.refine_split(label, fake.cpu().numpy(),
                                            None if start is None else start.cpu().numpy(), 0.45,
                                            rule, 2, 16, KINDS[kinds])
                _same((g.cpu().numpy(), ut.cpu().numpy(), rq.cpu().numpy()), host)
    merged = eng.refine_merge(db, g0, fake)                       # refine_merge() is what it was
    as_merge = eng.refine_split(db, g0, fake, kinds="merge")
    for x, z in zip(merged, as_merge):
        assert torch.equal(x, z)
    assert eng._rf_workspace is ws
    thr = [0.3, 0.6]
    tree = eng.agglomerate(db, fake, "mean", "single")[:2]
    lut, lrq, lg = eng.refine_split_ladder(db, thr, tree, fake, max_sweeps=4, max_rounds=2,
                                           kinds="both", groups=True)
    assert tuple(lrq.shape) == (2, b, _lib.RS_Q_SLOTS) and tuple(lg.shape) == (2, b, nc)
    host = metrics.refine_split_ladder(label, fake.cpu().numpy(), thr,
                                       (tree[0].cpu().numpy(), tree[1].cpu().numpy()), "mean", 4, 2,
                                       3)
    _same((lg.cpu().numpy(), lut.cpu().numpy(), lrq.cpu().numpy()), host)
    assert eng.refine_split_ladder(db, thr, tree, fake)[2] is None
    for kw in (dict(kinds="all"), dict(kinds=3), dict(kinds=None), dict(max_rounds=0),
               dict(max_rounds=17), dict(max_rounds=2.0), dict(max_sweeps=0), dict(max_sweeps=65),
               dict(rule="most"), dict(groups=g0.long()), dict(groups=g0.cpu())):
        with pytest.raises(ValueError):
            eng.refine_split(db, **kw)
    for kw in (dict(kinds="none"), dict(max_rounds=0), dict(thresholds=[]), dict(tree=(tree[0],))):
        with pytest.raises(ValueError):
            eng.refine_split_ladder(db, **dict(dict(thresholds=thr), **kw))
    eng.check_status()


def test_split_ladder_is_graph_capturable():
    """Tree and ladder replay from a captured graph on new scores, with the captured rungs."""
    eng, db, label, nc, b = _engine(44)
    scores = torch.rand(b, 2, nc * (nc - 1), device=eng.device)
    thr = [0.6, 0.3, 0.45]

    def np3(out):
        ut, rq, g = out
        return g.cpu().numpy(), ut.cpu().numpy(), rq.cpu().numpy()

    tree = eng.agglomerate(db, scores, "any", "single")[:2]      # warm: workspaces allocated
    eng.refine_split_ladder(db, thr, tree, scores, rule="any", groups=True)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        tree = eng.agglomerate(db, scores, "any", "single")[:2]
        out = eng.refine_split_ladder(db, thr, tree, scores, rule="any", groups=True)
    for _ in range(2):
        scores.copy_(torch.rand_like(scores))
        graph.replay()
        torch.cuda.synchronize()
        replayed = np3(out)
        eager = np3(eng.refine_split_ladder(db, thr,
                                            eng.agglomerate(db, scores, "any", "single")[:2],
                                            scores, rule="any", groups=True))
        for x, z in zip(replayed, eager):
            np.testing.assert_array_equal(x, z)
        host = metrics.refine_split_ladder(label, scores.cpu().numpy(), thr,
                                           (tree[0].cpu().numpy(), tree[1].cpu().numpy()), "any")
        _same(replayed, host)


def test_graph2graph_untangle_and_calibrate_with_split(golden_dir, tmp_path, monkeypatch, capsys):
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
    thr, scores, rungs, table, rq = m.calibrate_refined(args, part="train", refine=sweeps,
                                                        ladder=lad, merge=rounds, split=True)
    out = capsys.readouterr().out
    n = table.shape[1]
    assert n > 0 and table.shape == (5, n, 8) and rq.shape == (5, n, _lib.RS_Q_SLOTS)
    train, _, maps = data.compact_from_read_data(tup, ne, nc, mb)
    want = []
    for j, db in enumerate(m._device_batches(train, maps)):
        label = data.onehot_relations(train.y[j * mb:(j + 1) * mb])
        probs = m.engine.forward(db)[0].cpu().numpy()
        tree = metrics.linkage(label, probs, "mean")
        want.append(metrics.refine_split_ladder(label, probs, rungs, tree[:2], "mean", sweeps,
                                                rounds, 3))
    hut = np.concatenate([w[0] for w in want], 1)
    hrq = np.concatenate([w[2] for w in want], 1)
    np.testing.assert_array_equal(table, hut)
    np.testing.assert_array_equal(rq, hrq)
    for j in range(5):
        assert ("calibrate refined rung %d split: %d splits in %d of %d commits"
                % (j, hrq[j, :, SPLITS].sum(), np.count_nonzero(hrq[j, :, SPLITS]), n)) in out
    k = metrics.best_rung(hut, rungs, "f1")[0]
    _, t1, _ = m.untangle(args, part="train", threshold=thr, refine=sweeps, merge=rounds,
                          split=True)
    out = capsys.readouterr().out
    np.testing.assert_array_equal(t1, table[k])
    q = np.load(d / ("untangle_refine%d.npy" % ne))
    np.testing.assert_array_equal(q, rq[k])
    assert ("untangle split: %d splits in %d of %d commits"
            % (q[:, SPLITS].sum(), np.count_nonzero(q[:, SPLITS]), n)) in out
    # without split both are what they were: no line about splits, the last column 0
    m.untangle(args, part="train", threshold=thr, refine=sweeps, merge=rounds)
    assert "split" not in capsys.readouterr().out
    assert (np.load(d / ("untangle_refine%d.npy" % ne))[:, SPLITS] == 0).all()
    for kw in (dict(split=True), dict(split=True, refine=4), dict(split=1, refine=4, merge=2)):
        with pytest.raises(ValueError):
            m.untangle(args, **kw)
    with pytest.raises(ValueError):
        m.calibrate_refined(args, split=True)
