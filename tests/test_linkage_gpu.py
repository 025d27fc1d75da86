"""hdg_linkage on the GPU: merges, levels, curve, true groups and the lk row compared with
the host implementation (hdgnn.metrics.linkage: plain Kruskal, no shared algorithm) for
integer equality, levels bit for bit (NaN padding by isnan) -- no tolerances.

The forest kernel tiles as hdg_untangle's link kernel does, so the shapes are the block
edges test_untangle_gpu derives from the header constants: nc 2, 33, 64, 65, 74, 128, 129,
193 at B = 3, and nc 705 at B = 1 for the 16-block cap.
"""
import ctypes
import types

import numpy as np
import pytest
import torch

from _decode import (B, BIG, NC_CAPPED, NC_THREE, NC_TWO, SHAPES, T, _bridged_groups, _onehot,
                     _owner, _pairs, _planted, _planted_labels, _probs, _same, _scores_of, _sym,
                     _uniform, _untangle_run, _with_infs)
from _decode import _LinkageBufs as _Bufs
from _decode import _linkage_run as _run
from hdgnn import _lib, data, layout, metrics
from hdgnn.synth import synth_commits

pytestmark = pytest.mark.gpu

RULES = ("mean", "any", "both")


def test_shapes_are_the_block_edges():
    assert SHAPES == [2, 33, T, T + 1, 74, NC_TWO - 1, NC_TWO, NC_THREE]
    assert _lib.untangle_blocks(NC_TWO - 1) == 1 and _lib.untangle_blocks(NC_TWO) == 2
    assert _lib.untangle_blocks(NC_THREE - 1) == 2 and _lib.untangle_blocks(NC_THREE) == 3
    assert _lib.untangle_blocks(NC_CAPPED) == _lib.UT_MAX_BLOCKS
    if (T, _lib.UT_TILES_PER_BLOCK, _lib.UT_MAX_BLOCKS) == (64, 4, 16):
        assert SHAPES == [2, 33, 64, 65, 74, 128, 129, 193]


# ---------------------------------------------------------------------------------------
# running the library and the host
# ---------------------------------------------------------------------------------------
def _check(y, p1, rule="mean", what=""):
    """Device == host, all five outputs; -> the host's."""
    _, dev = _run(y, p1, rule)
    host = metrics.linkage(_onehot(y), _probs(p1), rule)
    print(what, rule, "device lk", dev[4].tolist(), "host lk", host[4].tolist())
    _same(dev, host, "%s %s" % (what, rule))
    return host


# ---------------------------------------------------------------------------------------
# shapes x score sets
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("nc", SHAPES)
def test_planted_groups(nc):
    y, p1 = _planted(nc, seed=nc)                     # the 1/256 grid: many ties
    for rule in RULES:
        _, levels, _, _, lk = _check(y, p1, rule, "planted nc %d" % nc)
        assert (lk[:, _lib.LK_MERGES] == nc - 1).all()
    if nc >= T + 1:
        assert (np.diff(levels, axis=1) == 0).any()


@pytest.mark.parametrize("nc", SHAPES)
def test_uniform_scores(nc):
    y, p1 = _uniform(nc, seed=nc)                     # nearly all weights distinct
    for rule in RULES:
        _check(y, p1, rule, "uniform nc %d" % nc)


@pytest.mark.parametrize("nc", SHAPES)
def test_nan_in_one_direction(nc):
    y, p1 = _planted(nc, seed=300 + nc)
    rng = np.random.default_rng(300 + nc)
    I, J = _pairs(nc)
    hit = _sym(nc, rng, B, 0.05)
    hit[:, (I == 0) & (J == 1)] = hit[:, (I == 1) & (J == 0)] = True
    first = _sym(nc, rng, B, 0.5) ^ (I < J)           # which direction carries the NaN
    p1 = p1.copy()
    p1[hit & first] = np.nan
    if nc >= 33:                                      # and a hunk that no edge reaches
        p1[1, I == 7] = np.nan
        hit[1, (I == 7) | (J == 7)] = True
    for rule in RULES:
        _, _, _, _, lk = _check(y, p1, rule, "nan nc %d" % nc)
        np.testing.assert_array_equal(lk[:, _lib.LK_NAN], hit.sum(1) // 2)
        if nc >= 33:
            assert lk[1, _lib.LK_MERGES] == nc - 2


@pytest.mark.parametrize("nc", [3, T + 1])
def test_infinite_scores(nc):
    """Under mean a pair of +inf and -inf is no edge and counts in LK_NAN; hdg_untangle's
    UT_NAN, which counts NaN scores, stays 0 on the same input."""
    y, p1 = _with_infs(*_planted(nc, seed=50 + nc), seed=50 + nc)
    nan = {rule: _check(y, p1, rule, "inf nc %d" % nc)[4][:, _lib.LK_NAN] for rule in RULES}
    assert (nan["mean"] >= 1).all() and (nan["both"] == 0).all()
    ut = metrics.untangle_counts(_onehot(y), _probs(p1), 0.5, "mean")[0]
    assert (ut[:, _lib.UT_NAN] == 0).all()


@pytest.mark.parametrize("nc", [33, T + 1, NC_TWO, NC_THREE])
def test_scores_that_encode_their_relation(nc):
    """s_pq is a function of (p, q) that is neither symmetric nor smooth: reading a
    neighbouring relation (a wrong [q > p] shift) or the wrong mirror tile changes the tree."""
    I, J = _pairs(nc)
    rng = np.random.default_rng(700 + nc)
    y = _planted_labels(nc, rng, B)
    M = 128
    while M < 2 * nc:
        M *= 2
    p1 = np.stack([((I * (37 + 2 * b) + J * 101 + (I * J) % 7 + 11 * b) % M) / float(M)
                   for b in range(B)]).astype(np.float32)
    for rule in RULES:
        _check(y, p1, rule, "encoded nc %d" % nc)


def test_capped_shape_sixteen_blocks():
    nc = NC_CAPPED
    y, p1 = _planted(nc, seed=7, nb=1)
    _check(y, p1, "mean", "capped planted")
    y, p1 = _uniform(nc, seed=7, nb=1)
    _check(y, p1, "both", "capped uniform")


# ---------------------------------------------------------------------------------------
# against the existing kernel: a cut of the tree is hdg_untangle's partition there
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("nc", [T + 1, NC_TWO])
def test_cuts_are_hdg_untangles_partitions(nc):
    y, p1 = _uniform(nc, seed=40 + nc)
    for rule in RULES:
        _, (merges, levels, curve, _, lk) = _run(y, p1, rule)
        for b in range(B):
            M = int(lk[b, _lib.LK_MERGES])
            lv = levels[b, :M].astype(np.float64)
            nxt = np.append(lv[1:], -np.inf)
            reach = np.flatnonzero(nxt < lv)
            assert len(reach) >= 4
            for k in reach[[0, len(reach) // 3, 2 * len(reach) // 3, -1]]:
                tp = np.float32(nxt[k])
                thr = float(tp / np.float32(2)) if rule == "mean" else float(tp)
                _, _, _, ut = _untangle_run(y, p1, thr, rule)
                print(nc, rule, b, k, "curve", curve[b, k].tolist(), "ut", ut[b].tolist())
                assert ut[b, _lib.UT_GROUPS] == nc - (k + 1)
                assert ut[b, _lib.UT_SS] == curve[b, k, 1]
                assert ut[b, _lib.UT_SS] + ut[b, _lib.UT_SD] == curve[b, k, 0]
                assert ut[b, _lib.UT_SS] + ut[b, _lib.UT_DS] == lk[b, _lib.LK_ST]


# ---------------------------------------------------------------------------------------
# structures
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("nc", BIG)
def test_paths_stars_cliques(nc):
    rng = np.random.default_rng(400 + nc)
    y = _planted_labels(nc, rng, B)
    path = [[i, i + 1] for i in range(nc - 1)]
    star0 = [[0, q] for q in range(1, nc)]
    last = [[i, nc - 1] for i in range(nc - 1)]
    # a path; the same seen only from the top down; a star on the last hunk
    p1 = np.stack([_scores_of(nc, path), _scores_of(nc, path, "down"), _scores_of(nc, last)])
    merges, levels, _, _, _ = _check(y, p1, "any", "path / down / star nc %d" % nc)
    assert merges[0].tolist() == path and merges[1].tolist() == path and merges[2].tolist() == last
    assert (levels == 0.75).all()
    merges, levels, _, _, _ = _check(y, p1, "both", "path / down / star nc %d" % nc)
    assert merges[0].tolist() == path and merges[2].tolist() == last
    assert merges[1].tolist() == star0 and (levels[1] == 0.125).all()      # nothing is high both ways
    # the complete graph at one level: the lexicographic star on hunk 0
    full = np.full((1, nc * (nc - 1)), 0.75, np.float32)
    for rule in RULES:
        merges, levels, curve, _, _ = _check(y[:1], full, rule, "complete nc %d" % nc)
        assert merges[0].tolist() == star0
        assert (levels == (1.5 if rule == "mean" else 0.75)).all()
        assert curve[0, :, 0].tolist() == [(k + 1) * (k + 2) // 2 for k in range(nc - 1)]


@pytest.mark.parametrize("nc", BIG)
def test_groups_joined_by_another_blocks_link(nc):
    own = _owner(nc)
    edges, A, Bm, bridge = _bridged_groups(nc)
    assert all(own[p, q] == 0 for p, q in edges) and own[bridge] != 0
    rng = np.random.default_rng(500 + nc)
    y = _planted_labels(nc, rng, 1)
    I, J = _pairs(nc)
    p1 = _scores_of(nc, edges + [bridge])
    lo, hi = min(bridge), max(bridge)
    p1[((I == lo) & (J == hi)) | ((I == hi) & (J == lo))] = 0.5       # below the groups' links
    p1[p1 == np.float32(0.125)] = np.nan                              # every other pair: no edge
    members = len(set(A) | set(Bm))
    for rule in RULES:
        merges, levels, _, _, lk = _check(y, p1[None], rule, "bridge nc %d" % nc)
        M = int(lk[0, _lib.LK_MERGES])
        assert M == members - 1
        assert merges[0, M - 1].tolist() == [lo, hi]                  # the bridge comes last
        assert levels[0, M - 1] == (1.0 if rule == "mean" else 0.5)
        assert (levels[0, :M - 1] == (1.5 if rule == "mean" else 0.75)).all()


@pytest.mark.parametrize("nc", [T + 1, NC_TWO])
def test_directed_scores(nc):
    """s_pq 0.875 or 0.625 against s_qp 0.25 (p < q): which of the two each rule reads."""
    rng = np.random.default_rng(600 + nc)
    I, J = _pairs(nc)
    y = _planted_labels(nc, rng, B)
    a = _sym(nc, rng, B, 3.0 / nc)
    b = _sym(nc, rng, B, 3.0 / nc) & ~a
    p1 = np.full(a.shape, 0.25, np.float32)
    p1[a & (I < J)] = 0.875
    p1[b & (I < J)] = 0.625
    top = {"mean": 1.125, "any": 0.875, "both": 0.25}
    for rule in RULES:
        _, levels, _, _, _ = _check(y, p1, rule, "directed nc %d" % nc)
        assert (levels[:, 0] == top[rule]).all()
    # and the other way round
    p1 = np.full(a.shape, 0.25, np.float32)
    p1[a & (I > J)] = 0.875
    for rule in RULES:
        _, levels, _, _, _ = _check(y, p1, rule, "directed down nc %d" % nc)
        assert (levels[:, 0] == top[rule]).all()


# ---------------------------------------------------------------------------------------
# outputs and arguments
# ---------------------------------------------------------------------------------------
def test_repeat_launch_other_inputs_and_null_tgroups():
    nc = NC_THREE
    y, p1 = _planted(nc, seed=901)
    host = metrics.linkage(_onehot(y), _probs(p1))
    bufs, first = _run(y, p1)
    _same(first, host)
    _, again = _run(y, p1, bufs=bufs)                           # into the used buffers
    for x, z in zip(first, again):
        np.testing.assert_array_equal(x.view(np.uint8), z.view(np.uint8))     # the same bits
    y3, p3 = _uniform(nc, seed=902)                             # other inputs, same buffers
    p3[0, :nc - 1] = np.nan                                     # fewer merges than before
    _, other = _run(y3, p3, "any", bufs=bufs)
    _same(other, metrics.linkage(_onehot(y3), _probs(p3), "any"))
    fresh, nul = _run(y, p1, tgroups=False)                     # tgroups = NULL
    assert (nul[3] == -7).all()                                 # untouched
    _same(nul[:3] + (host[3],) + nul[4:], host)


def test_argument_errors_launch_nothing():
    lib = _lib.load()
    dev = torch.device("cuda")
    nc = 10
    bufs = _Bufs(B, nc, dev)
    ybits = torch.zeros(B, nc, 1, dtype=torch.int32, device=dev)
    pt = torch.rand(B, 2, nc * (nc - 1), device=dev)
    ok_shape = _lib.Shape(B, 20, nc, 2, B, 0)
    ok_bt = _lib.Batch(None, None, ybits.data_ptr(), None, None, None)
    vp = ctypes.c_void_p
    base = dict(shape=ok_shape, bt=ok_bt, probs=vp(pt.data_ptr()), rule=0,
                merges=vp(bufs.merges.data_ptr()), levels=vp(bufs.levels.data_ptr()),
                curve=vp(bufs.curve.data_ptr()), lk=vp(bufs.lk.data_ptr()),
                ws=vp(bufs.ws.data_ptr()))

    def call(**kw):
        a = dict(base, **kw)
        stream = vp(torch.cuda.current_stream(dev).cuda_stream)
        return lib.hdg_linkage(ctypes.byref(a["shape"]), ctypes.byref(a["bt"]), a["probs"],
                               a["rule"], a["merges"], a["levels"], a["curve"], None, a["lk"],
                               a["ws"], stream)

    bad = [dict(rule=3), dict(rule=-1), dict(probs=None), dict(merges=None), dict(levels=None),
           dict(curve=None), dict(lk=None), dict(ws=None),
           dict(bt=_lib.Batch(None, None, None, None, None, None)),
           dict(shape=_lib.Shape(0, 20, nc, 2, B, 0)), dict(shape=_lib.Shape(65536, 20, nc, 2, B, 0)),
           dict(shape=_lib.Shape(B, 20, 1, 2, B, 0)), dict(shape=_lib.Shape(B, 20, 2049, 2, B, 0))]
    for kw in bad:
        assert call(**kw) == 1000, kw
        assert lib.hdg_last_error().startswith(b"hdg_linkage:"), kw
    torch.cuda.synchronize(dev)
    assert bufs.poisoned()
    assert call() == 0
    torch.cuda.synchronize(dev)
    assert (bufs.lk >= 0).all() and (bufs.lk[:, _lib.LK_MERGES] == nc - 1).all()


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


def test_engine_forward_then_linkage():
    eng, db, label, nc, b = _engine(21)
    probs, _, _ = eng.forward(db)
    out = eng.linkage(db)
    merges, levels, curve, tgroups, lk = out
    assert all(x.is_cuda for x in out)
    assert merges.dtype == torch.int32 and tuple(merges.shape) == (b, nc - 1, 2)
    assert levels.dtype == torch.float32 and tuple(levels.shape) == (b, nc - 1)
    assert curve.dtype == torch.int32 and tuple(curve.shape) == (b, nc - 1, 2)
    assert tgroups.dtype == torch.int32 and tuple(tgroups.shape) == (b, nc)
    assert lk.dtype == torch.int64 and tuple(lk.shape) == (b, _lib.LK_SLOTS)
    _same(tuple(x.cpu().numpy() for x in out), metrics.linkage(label, probs.cpu().numpy()))
    ws = eng._lk_workspace
    fake = torch.rand_like(probs)
    for rule in RULES:
        out = eng.linkage(db, fake, rule=rule)
        _same(tuple(x.cpu().numpy() for x in out), metrics.linkage(label, fake.cpu().numpy(), rule))
    assert eng._lk_workspace is ws                               # allocated once
    with pytest.raises(ValueError):
        eng.linkage(db, fake[:, :, :-1])
    with pytest.raises(ValueError):
        eng.linkage(db, fake, rule="most")
    eng.check_status()


def test_linkage_is_graph_capturable():
    """Both launches replay from a captured graph on new scores."""
    eng, db, label, nc, b = _engine(22)
    scores = torch.rand(b, 2, nc * (nc - 1), device=eng.device)
    eng.linkage(db, scores, rule="any")             # warm: module loaded, workspace allocated
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = eng.linkage(db, scores, rule="any")
    for _ in range(2):
        scores.copy_(torch.rand_like(scores))
        g.replay()
        torch.cuda.synchronize()
        _same(tuple(x.cpu().numpy() for x in out),
              metrics.linkage(label, scores.cpu().numpy(), "any"))


def test_graph2graph_calibrate_finds_the_train_splits_threshold(golden_dir, tmp_path, monkeypatch,
                                                                capsys):
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
    thr, scores, levels, curve, lk = m2.calibrate(args, part="train", rule="mean", score="f1")
    out = capsys.readouterr().out
    assert " [*] Load SUCCESS" in out and "Load failed" not in out
    for line in ("calibrate rule: mean", "calibrate score: f1 = ", "calibrate threshold: "):
        assert line in out, line
    n = len(lk)
    assert n > 0 and n % mb == 0
    assert levels.shape == (n, nc - 1) and levels.dtype == np.float32
    assert curve.shape == (n, nc - 1, 2) and curve.dtype == np.int64
    assert lk.shape == (n, _lib.LK_SLOTS) and lk.dtype == np.int64
    d = tmp_path / "outputSelf" / "tiny" / "model_2" / "2"
    np.testing.assert_array_equal(np.load(d / ("linkage_levels%d.npy" % ne)).view(np.uint32),
                                  levels.view(np.uint32))
    np.testing.assert_array_equal(np.load(d / ("linkage_curve%d.npy" % ne)), curve)
    np.testing.assert_array_equal(np.load(d / ("linkage_counts%d.npy" % ne)), lk)
    saved = np.load(d / ("linkage_merges%d.npy" % ne))
    assert saved.shape == (n, nc - 1, 2) and saved.dtype == np.int32
    # the host linkages of the probabilities a forward of the same batches returns
    train, _, maps = data.compact_from_read_data(tup, ne, nc, mb)
    dbs = m2._device_batches(train, maps)
    want = [metrics.linkage(data.onehot_relations(train.y[j * mb:(j + 1) * mb]),
                            m2.engine.forward(db)[0].cpu().numpy(), "mean")
            for j, db in enumerate(dbs)]
    host = tuple(np.concatenate([w[i] for w in want]) for i in range(5))
    _same((saved, levels, curve, host[3], lk), host)
    hthr, hbest, htp = metrics.best_threshold(host[1], host[2], host[4], "mean", "f1")
    assert thr == hthr and scores["f1"] == hbest
    print("calibrated threshold", thr, "f1", hbest, "bound", htp)
    # untangling the same split at that threshold scores what the calibration promised
    uscores, table, _ = m2.untangle(args, part="train", threshold=thr)
    assert uscores["f1"] == hbest
    np.testing.assert_equal({k: v for k, v in uscores.items()},
                            {k: v for k, v in scores.items()})
