"""hdg_refine_ladder on the GPU: every rung of groups, ut and rq compared with the host
restatement (hdgnn.metrics.refine_ladder) and with the existing entry points run rung by rung
(hdg_cut then hdg_refine on the same tree) for integer equality.  No tolerances.  Buffers are
poisoned before every call and no poison may survive in any rung.

Shapes: nc 2 and 3, 33 (the label row crosses a word), the tile edges 64 / 65, 74 (the glide
shape), 129 (three tile rows, two blocks in the weights grid), B = 3 and all three rules;
1025, the first nc at which a thread owns two hunks, B = 1, two rungs, two sweeps, rule
"mean".  Ladders: one rung; two equal rungs; five unsorted rungs with -1.5 and 3.0 among
them; 64 rungs at nc = 33.  Starts: no tree, hdg_linkage's tree, hdg_agglomerate's complete
and average trees (the trees are the device's: those entry points have their own tests).
"""
import ctypes
import math
import types

import numpy as np
import pytest
import torch

from _decode import (B, T, _agglomerate_run, _cut, _linkage_run, _onehot, _planted, _probs,
                     _refine_run, _uniform, _with_infs, _with_nans)
from _ladder import (DEFAULT_LADDER, LADDERS, LadderBufs, ladder_run, motivating_family, same,
                     tprime)
from hdgnn import _lib, data, layout, metrics
from hdgnn.synth import synth_commits
from test_refine import noisy_planted

pytestmark = pytest.mark.gpu

RULES = ("mean", "any", "both")
SHAPES = [2, 3, 33, T, T + 1, 74, 2 * T + 1]
TWO_PER_THREAD = 1025
STARTS = ("none", "linkage", "complete", "average")


def test_shapes_follow_from_the_header_constants():
    if T == 64:
        assert SHAPES == [2, 3, 33, 64, 65, 74, 129]
    assert TWO_PER_THREAD == 1024 + 1 and _lib.RL_MAX_RUNGS == 64
    assert [len(x) for x in LADDERS] == [1, 2, 5] and LADDERS[1][0] == LADDERS[1][1]
    assert -1.5 in LADDERS[2] and 3.0 in LADDERS[2] and LADDERS[2] != sorted(LADDERS[2])


# ---------------------------------------------------------------------------------------
# running the library and the host
# ---------------------------------------------------------------------------------------
def _tree(y, p1, rule, start):
    """The device's tree for a start -> (merges, levels, curve, lk) or None."""
    if start == "none":
        return None
    if start == "linkage":
        _, (m, lv, cv, _, lk) = _linkage_run(y, p1, rule)
    else:
        _, (m, lv, cv, _, lk) = _agglomerate_run(y, p1, rule, start)
    return m, lv, cv, lk


def _sequences(y, p1, thresholds, tree, rule, ms):
    """What the call replaces: per rung hdg_cut then hdg_refine -> (groups, ut, rq) stacked."""
    nc = int(round((1 + math.sqrt(1 + 4 * p1.shape[1])) / 2))
    out = []
    for t in thresholds:
        start = None
        if tree is not None:
            start, _ = _cut(nc, tree[0], tree[1], tree[2], tree[3], float(t), rule, ut=False)
        out.append(_refine_run(y, p1, start, float(t), rule, ms)[1:])
    return tuple(np.stack([o[i] for o in out]) for i in range(3))


def _one(what, y, p1, thresholds, tree, rule, ms=8):
    """One call against the host and against the sequences -> the host's (ut, groups, rq)."""
    host = metrics.refine_ladder(_onehot(y), _probs(p1), thresholds,
                                 None if tree is None else tree[:2], rule, ms)
    bufs, *dev = ladder_run(y, p1, thresholds, None if tree is None else tree[:2], rule, ms)
    print(what, "device ut", dev[1].tolist(), "rq", dev[2].tolist())
    assert not bufs.any_poison(), what
    same(dev, host, what)
    seq = _sequences(y, p1, thresholds, tree, rule, ms)
    for x, z in zip(dev, seq):
        np.testing.assert_array_equal(x, z, what)
    return host


def _check(what, y, p1, extra=()):
    """Every rule and start; the ladders cycle so that every (start, ladder) pair is run."""
    ladders = list(LADDERS) + list(extra)
    k = 0
    for rule in RULES:
        for start in STARTS:
            thr = ladders[k % len(ladders)]
            k += 1
            tree = _tree(y, p1, rule, start)
            _one("%s %s %s T=%d" % (what, rule, start, len(thr)), y, p1, thr, tree, rule)


def test_every_start_meets_every_ladder():
    pairs = {(k % len(STARTS), k % len(LADDERS)) for k in range(len(RULES) * len(STARTS))}
    assert len(pairs) == len(STARTS) * len(LADDERS)


# ---------------------------------------------------------------------------------------
# device == host, device == hdg_cut + hdg_refine
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("nc", SHAPES)
def test_noisy_planted_scores(nc):
    y, p1 = noisy_planted(nc, seed=nc, B=B)
    _check("noisy %d" % nc, y, p1)


@pytest.mark.parametrize("nc", SHAPES)
def test_uniform_scores(nc):
    y, p1 = _uniform(nc, seed=nc)
    _check("uniform %d" % nc, y, p1)


@pytest.mark.parametrize("nc", SHAPES)
def test_scores_on_the_grid(nc):
    y, p1 = _planted(nc, seed=nc)                            # the 1/256 grid: many exact ties
    _check("planted %d" % nc, y, p1)


@pytest.mark.parametrize("nc", SHAPES)
def test_nan_in_one_direction_and_an_isolated_hunk(nc):
    y, p1, nans = _with_nans(nc, B)
    _check("nan %d" % nc, y, p1)
    _, _, ut, _ = ladder_run(y, p1, [0.5, 0.2], None, "mean", 1)
    np.testing.assert_array_equal(ut[:, :, _lib.RF_NAN], np.stack([nans, nans]))


@pytest.mark.parametrize("nc", [3, 33, T + 1, 2 * T + 1])
def test_infinite_scores(nc):
    y, p1 = _with_infs(*noisy_planted(nc, seed=50 + nc, B=B), seed=50 + nc)
    _check("inf %d" % nc, y, p1)
    _, _, mean, _ = ladder_run(y, p1, [0.5], None, "mean", 1)
    _, _, both, _ = ladder_run(y, p1, [0.5], None, "both", 1)
    assert (mean[..., _lib.RF_NAN] >= 1).all() and (both[..., _lib.RF_NAN] == 0).all()


def test_sixty_four_rungs():
    nc = 33
    y, p1 = noisy_planted(nc, seed=64, B=B)
    rng = np.random.default_rng(64)
    thr = rng.permutation(metrics.ladder(-0.2, 1.2, 64)).tolist()
    for rule, start in (("mean", "average"), ("any", "linkage"), ("both", "none")):
        host = _one("64 rungs %s %s" % (rule, start), y, p1, thr, _tree(y, p1, rule, start), rule)
        assert len({tuple(r.ravel()) for r in host[1]}) > 3          # the rungs do differ


def test_two_hunks_per_thread():
    nc = TWO_PER_THREAD
    y, p1 = noisy_planted(nc, seed=nc, B=1, k=12)
    tree = _tree(y, p1, "mean", "linkage")
    host = _one("1025", y, p1, [0.5, 0.45], tree, "mean", ms=2)
    assert (host[0][..., _lib.RF_MOVES] > 0).all() and (host[2][..., _lib.RF_Q_START] != 0).all()


# ---------------------------------------------------------------------------------------
# exact ties at both places a bound is compared
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("nc", [33, T + 1, 74])
def test_a_level_and_a_weight_exactly_on_a_rung(nc):
    rng = np.random.default_rng(nc)
    y, _ = _planted(nc, seed=nc)
    p1 = (rng.integers(96, 161, y.shape) / 256.0).astype(np.float32)
    on_grid = [0.625, 0.375, 0.5]
    for rule in ("any", "both"):
        for start in ("linkage", "complete"):
            tree = _tree(y, p1, rule, start)
            lv = tree[1]
            # single linkage keeps its levels near the top of the grid, so two more rungs are
            # levels of the tree itself: the middle merge of commit 0 and of commit 1
            thr = on_grid + [float(lv[0, (nc - 1) // 2]), float(lv[1, (nc - 1) // 2])]
            W = np.stack([metrics.refine_gains(p1[b], np.float32(0), rule)[0] for b in range(B)])
            # a pair weight exactly on a rung (gain 0): the maximum of two scores reaches the
            # top of the grid and not its bottom, the minimum the other way round
            for t in thr:
                assert t * 256 == int(t * 256)
                if t != {"any": 0.375, "both": 0.625}[rule]:
                    assert (W == int(t * 262144)).any(), (rule, t)
            assert sum(int((lv == np.float32(t)).sum()) for t in thr) >= 2    # strict: not united
            _one("ties %d %s %s" % (nc, rule, start), y, p1, thr, tree, rule)


# ---------------------------------------------------------------------------------------
# caps and outputs
# ---------------------------------------------------------------------------------------
def test_max_sweeps_and_the_converged_flag():
    """Uniform scores at nc = 129 under mean take several sweeps: the cap cuts rungs short."""
    nc = 2 * T + 1
    y, p1 = _uniform(nc, seed=nc)
    thr = [0.5, 0.3, 0.9]
    flags = {}
    for ms in (1, 2, 8, 64):
        host = _one("cap %d" % ms, y, p1, thr, None, "mean", ms)
        flags[ms] = host[2][..., _lib.RF_Q_CONVERGED]
        assert (host[2][..., _lib.RF_Q_SWEEPS] <= ms).all()
    every = np.concatenate([f.ravel() for f in flags.values()])
    assert (every == 0).any() and (every == 1).any()            # the host's flags, both values
    assert (flags[64] == 1).all()


def test_without_groups_the_same_table():
    nc = 74
    y, p1 = noisy_planted(nc, seed=74, B=B)
    tree = _tree(y, p1, "mean", "average")
    thr = LADDERS[2]
    _, g, ut, rq = ladder_run(y, p1, thr, tree[:2], "mean", 8)
    bufs, g0, ut0, rq0 = ladder_run(y, p1, thr, tree[:2], "mean", 8, groups=False)
    assert (g0 == -7).all() and not bool((bufs.ut == -1).any() or (bufs.rq == -99).any())
    np.testing.assert_array_equal(ut0, ut)
    np.testing.assert_array_equal(rq0, rq)


# ---------------------------------------------------------------------------------------
# calls
# ---------------------------------------------------------------------------------------
def test_repeat_launch_other_inputs_same_buffers():
    nc = 74
    y, p1 = noisy_planted(nc, seed=901, B=B)
    tree = _tree(y, p1, "mean", "linkage")
    thr = LADDERS[2]
    host = metrics.refine_ladder(_onehot(y), _probs(p1), thr, tree[:2])
    bufs, *first = ladder_run(y, p1, thr, tree[:2])
    same(first, host)
    _, *again = ladder_run(y, p1, thr, tree[:2], bufs=bufs)        # into the used buffers
    for x, z in zip(first, again):
        np.testing.assert_array_equal(x, z)
    y3, p3 = _uniform(nc, seed=902)                                # other inputs, same buffers
    p3[0, :nc - 1] = np.nan
    thr3 = [0.4, 0.1, 0.6, 0.4, 0.9]
    _, *other = ladder_run(y3, p3, thr3, None, "both", 2, bufs=bufs)
    same(other, metrics.refine_ladder(_onehot(y3), _probs(p3), thr3, None, "both", 2))


def test_argument_errors_launch_nothing():
    lib = _lib.load()
    dev = torch.device("cuda")
    nc, n = 10, 5
    bufs = LadderBufs(n, B, nc, dev)
    ybits = torch.zeros(B, nc, 1, dtype=torch.int32, device=dev)
    pt = torch.rand(B, 2, nc * (nc - 1), device=dev)
    tm = torch.full((B, nc - 1, 2), -1, dtype=torch.int32, device=dev)
    tl = torch.full((B, nc - 1), float("nan"), device=dev)
    vp = ctypes.c_void_p
    base = dict(shape=_lib.Shape(B, 20, nc, 2, B, 0),
                bt=_lib.Batch(None, None, ybits.data_ptr(), None, None, None),
                probs=vp(pt.data_ptr()), thr=[0.1, 0.3, 0.5, 0.7, 0.9], n=None, rule=0, ms=8,
                flags=0, merges=vp(tm.data_ptr()), levels=vp(tl.data_ptr()),
                groups=vp(bufs.groups.data_ptr()), ut=vp(bufs.ut.data_ptr()),
                rq=vp(bufs.rq.data_ptr()), ws=vp(bufs.ws.data_ptr()))

    def call(**kw):
        a = dict(base, **kw)
        thr = a["thr"]
        k = a["n"] if a["n"] is not None else len(thr)
        arr = None if thr is None else (ctypes.c_float * max(1, len(thr)))(*thr)
        stream = vp(torch.cuda.current_stream(dev).cuda_stream)
        return lib.hdg_refine_ladder(ctypes.byref(a["shape"]), ctypes.byref(a["bt"]), a["probs"],
                                     arr, k, a["rule"], a["ms"], a["flags"], a["merges"],
                                     a["levels"], a["groups"], a["ut"], a["rq"], a["ws"], stream)

    nan, inf = float("nan"), float("inf")
    bad = [dict(rule=3), dict(rule=-1), dict(ms=0), dict(ms=65), dict(ms=-1), dict(flags=1),
           dict(flags=2), dict(n=0), dict(n=-1), dict(n=65, thr=[0.5] * 65), dict(thr=None, n=5),
           dict(thr=[0.1, 0.3, 0.5, nan, 0.9]), dict(thr=[inf, 0.3, 0.5, 0.7, 0.9]),
           dict(thr=[0.1, 0.3, 0.5, 0.7, -inf], rule=1), dict(thr=[0.1, 3e38, 0.5, 0.7, 0.9]),
           dict(levels=None), dict(merges=None), dict(probs=None), dict(ut=None), dict(rq=None),
           dict(ws=None), dict(ws=vp(bufs.ws.data_ptr() + 4)),
           dict(bt=_lib.Batch(None, None, None, None, None, None)),
           dict(shape=_lib.Shape(0, 20, nc, 2, B, 0)), dict(shape=_lib.Shape(65536, 20, nc, 2, B, 0)),
           dict(shape=_lib.Shape(B, 20, 1, 2, B, 0)), dict(shape=_lib.Shape(B, 20, 2049, 2, B, 0))]
    for kw in bad:
        assert call(**kw) == 1000, kw
        assert lib.hdg_last_error().startswith(b"hdg_refine_ladder:"), kw
    assert call(thr=[0.1, 0.3, 0.5, nan, 0.9]) == 1000 and b"rung 3" in lib.hdg_last_error()
    torch.cuda.synchronize(dev)
    assert bufs.poisoned()
    assert call() == 0 and call(merges=None, levels=None) == 0 and call(groups=None) == 0
    torch.cuda.synchronize(dev)
    assert (bufs.groups >= 0).all() and (bufs.ut >= 0).all() and (bufs.rq[..., 2] >= 1).all()


# ---------------------------------------------------------------------------------------
# the motivating family, on the device from the tree to the chosen rung
# ---------------------------------------------------------------------------------------
def test_device_picks_the_rung_that_recovers_the_planted_groups():
    y, p1 = motivating_family()
    nc = 40
    _, (m, lv, cv, _, lk) = _linkage_run(y, p1, "mean")
    thr, tree_f1, tp = metrics.best_threshold(lv, cv.astype(np.int64), lk, "mean", "f1")
    rungs = metrics.ladder(*DEFAULT_LADDER)
    _, g, ut, rq = ladder_run(y, p1, rungs.tolist(), (m, lv), "mean", 8)
    k, best, f1, vals = metrics.best_rung(ut, rungs, "f1")
    print("tree", thr, tree_f1, "rungs", vals.tolist())
    assert k == 8 and best == float(np.float32(0.45)) and f1 == 1.0 and tree_f1 < 1.0
    assert (ut[8][:, _lib.UT_SD] == 0).all() and (ut[8][:, _lib.UT_DS] == 0).all()
    planted = metrics.untangle_counts(_onehot(y), _probs(p1))[2]      # the true groups
    np.testing.assert_array_equal(g[8], planted)
    # refining at the tree's own best threshold is the path that loses
    start, _ = _cut(nc, m, lv, cv, lk, thr, "mean", ut=False)
    at_tree = _refine_run(y, p1, start, thr, "mean", 8)[2]
    assert metrics.scores_from_untangle(at_tree)["f1"] < tree_f1


# ---------------------------------------------------------------------------------------
# Engine and graph2graph
# ---------------------------------------------------------------------------------------
def _engine(seed):
    from hdgnn.engine import Engine
    ne, nc, b = 20, 10, 4
    cb = synth_commits(b, ne, nc, seed)
    eng = Engine(ne, nc, b, variant=2)
    eng.set_params(layout.init_flat(5, 2))
    return eng, eng.upload(cb), data.onehot_relations(cb.y), nc, b


def _np(out):
    """Engine.refine_ladder's (ut, rq, groups) -> (groups, ut, rq) on the host."""
    ut, rq, g = out
    return g.cpu().numpy(), ut.cpu().numpy(), rq.cpu().numpy()


def _host(label, probs, thr, tree, rule="mean", ms=8):
    tree = None if tree is None else (tree[0].cpu().numpy(), tree[1].cpu().numpy())
    return metrics.refine_ladder(label, probs.cpu().numpy(), thr, tree, rule, ms)


def test_engine_forward_then_tree_then_ladder():
    eng, db, label, nc, b = _engine(41)
    probs, _, _ = eng.forward(db)
    m, lv, _, _, _ = eng.linkage(db)
    thr = metrics.ladder(0.2, 0.8, 4).tolist()
    out = eng.refine_ladder(db, thr, tree=(m, lv), groups=True)
    ut, rq, groups = out
    assert all(x.is_cuda for x in out)
    assert groups.dtype == torch.int32 and tuple(groups.shape) == (4, b, nc)
    assert ut.dtype == torch.int64 and tuple(ut.shape) == (4, b, _lib.RF_SLOTS)
    assert rq.dtype == torch.int64 and tuple(rq.shape) == (4, b, _lib.RF_Q_SLOTS)
    same(_np(out), _host(label, probs, thr, (m, lv)))
    ws = eng._rl_workspace
    ut2, rq2, none = eng.refine_ladder(db, thr, tree=(m, lv))
    assert none is None and torch.equal(ut2, ut) and torch.equal(rq2, rq)
    fake = torch.rand_like(probs)
    for rule in RULES:
        for method in (None, "complete"):
            tree = None if method is None else eng.agglomerate(db, fake, rule, method)[:2]
            out = eng.refine_ladder(db, LADDERS[2], tree, fake, rule=rule, max_sweeps=2,
                                    groups=True)
            same(_np(out), _host(label, fake, LADDERS[2], tree, rule, 2))
    assert eng._rl_workspace is ws                               # allocated once
    for kw in (dict(thresholds=[]), dict(thresholds=[0.5] * 65), dict(thresholds=[0.5, float("nan")]),
               dict(thresholds=[float("inf")]), dict(thresholds=0.5), dict(probs=fake[:, :, :-1]),
               dict(rule="most"), dict(max_sweeps=0), dict(max_sweeps=65), dict(max_sweeps=2.0),
               dict(tree=(m,)), dict(tree=(m, lv.double())), dict(tree=(m.long(), lv)),
               dict(tree=(m[:, :-1], lv)), dict(tree=(m.cpu(), lv.cpu())), dict(tree=(lv, m))):
        with pytest.raises(ValueError):
            eng.refine_ladder(db, **dict(dict(thresholds=thr), **kw))
    with pytest.raises(RuntimeError):
        eng.refine_ladder(db, [3e38])                            # finite, but t' = inf under mean
    eng.check_status()


def test_ladder_is_graph_capturable():
    """Tree and ladder replay from a captured graph on new scores, with the captured rungs."""
    eng, db, label, nc, b = _engine(42)
    scores = torch.rand(b, 2, nc * (nc - 1), device=eng.device)
    thr = [0.6, 0.3, 0.45]
    tree = eng.agglomerate(db, scores, "any", "average")[:2]     # warm: workspaces allocated
    eng.refine_ladder(db, thr, tree, scores, rule="any", groups=True)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        tree = eng.agglomerate(db, scores, "any", "average")[:2]
        out = eng.refine_ladder(db, thr, tree, scores, rule="any", groups=True)
    for _ in range(2):
        scores.copy_(torch.rand_like(scores))
        graph.replay()
        torch.cuda.synchronize()
        replayed = _np(out)
        eager = _np(eng.refine_ladder(db, thr, eng.agglomerate(db, scores, "any", "average")[:2],
                                      scores, rule="any", groups=True))
        for x, z in zip(replayed, eager):
            np.testing.assert_array_equal(x, z)
        same(replayed, _host(label, scores, thr, tree, "any"))


def test_graph2graph_calibrate_refined(golden_dir, tmp_path, monkeypatch, capsys):
    from hdgnn.model import graph2graph
    from test_model_gpu import _tuple
    tup, meta = _tuple(golden_dir)
    ne, nc, mb = meta["Ne"], meta["Nc"], 25
    monkeypatch.chdir(tmp_path)
    args = types.SimpleNamespace(Repo="tiny", checkpoint_dir=str(tmp_path / "ckpt"))

    def model(seed):
        return graph2graph(None, Ds=1, Ne=ne, Nc=nc, Ner=ne * (ne - 1), Ncr=nc * (nc - 1), Dr=2,
                           De_e=20, De_er=20, Mini_batch=mb, checkpoint_dir=args.checkpoint_dir,
                           epoch=2, Ds_inter=1, Dr_inter=2, Step=2, Repo="tiny",
                           reader=lambda m, step: tup, seed=seed)

    m = model(7)
    m.train(args)
    capsys.readouterr()
    m2 = model(99)                                  # another initialiser: the load must win
    d = tmp_path / "outputSelf" / "tiny" / "model_2" / "2"
    lad, sweeps = (0.3, 0.7, 5), 4
    thr, scores, rungs, table, rq = m2.calibrate_refined(args, part="train", method="average",
                                                         refine=sweeps, ladder=lad)
    out = capsys.readouterr().out
    assert " [*] Load SUCCESS" in out
    np.testing.assert_array_equal(rungs, metrics.ladder(*lad))
    n = table.shape[1]
    assert n > 0 and n % mb == 0 and table.shape == (5, n, 8) and rq.shape == (5, n, 4)
    assert table.dtype == np.int64 and rq.dtype == np.int64
    # the host, from the probabilities a forward of the same batches returns
    train, _, maps = data.compact_from_read_data(tup, ne, nc, mb)
    want, trees = [], []
    for j, db in enumerate(m2._device_batches(train, maps)):
        label = data.onehot_relations(train.y[j * mb:(j + 1) * mb])
        probs = m2.engine.forward(db)[0].cpu().numpy()
        tree = metrics.agglomerate(label, probs, "mean", "average")
        trees.append(tree)
        want.append(metrics.refine_ladder(label, probs, rungs, tree[:2], "mean", sweeps))
    hut = np.concatenate([w[0] for w in want], 1)
    hrq = np.concatenate([w[2] for w in want], 1)
    np.testing.assert_array_equal(table, hut)
    np.testing.assert_array_equal(rq, hrq)
    k, best_thr, best, vals = metrics.best_rung(hut, rungs, "f1")
    assert thr == best_thr
    np.testing.assert_equal(scores, metrics.scores_from_untangle(hut[k]))
    np.testing.assert_array_equal(np.load(d / ("refine_ladder_thresholds%d.npy" % ne)), rungs)
    np.testing.assert_array_equal(np.load(d / ("refine_ladder_counts%d.npy" % ne)), table)
    np.testing.assert_array_equal(np.load(d / ("refine_ladder_objective%d.npy" % ne)), rq)
    assert ("calibrate refined threshold: %r (rung %d), f1 = %s" % (best_thr, k, best)) in out
    for j in range(5):
        assert ("calibrate refined rung %d: threshold %r, f1 = %s, %d moves, %d of %d commits "
                "converged" % (j, float(rungs[j]), vals[j], hut[j, :, _lib.RF_MOVES].sum(),
                               hrq[j, :, _lib.RF_Q_CONVERGED].sum(), n)) in out
    lv, cv, lk = (np.concatenate([t[i] for t in trees]) for i in (1, 2, 4))
    tree_thr, tree_best, _ = metrics.best_threshold(lv, cv, lk, "mean", "f1")
    assert ("calibrate refined tree alone: threshold %r, f1 = %s" % (tree_thr, tree_best)) in out
    verdict = ("the refined rung scores higher than the tree alone" if best > tree_best else
               "the tree alone scores higher than every refined rung" if tree_best > best else
               "neither scores higher")
    assert verdict in out
    # untangle at that threshold with the same sweeps gives that rung's table
    _, t1, _ = m2.untangle(args, part="train", threshold=thr, method="average", refine=sweeps)
    capsys.readouterr()
    np.testing.assert_array_equal(t1, table[k])
    # calibrate() is what it was: it neither prints nor writes anything of the ladder's
    for f in d.glob("refine_ladder_*"):
        f.unlink()
    m2.calibrate(args, part="train", method="average")
    assert "refined" not in capsys.readouterr().out and not list(d.glob("refine_ladder_*"))
    for kw in (dict(refine=0), dict(refine=65), dict(ladder=(0, 1, 65)), dict(method="ward"),
               dict(part="all")):
        with pytest.raises(ValueError):
            m2.calibrate_refined(args, **kw)
