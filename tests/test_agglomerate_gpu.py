"""hdg_agglomerate and hdg_cut on the GPU: all five outputs compared with the host restatement
(hdgnn.metrics.agglomerate: a plain arg-max over the whole matrix per step, no shared
algorithm) for integer equality, levels bit for bit (NaN padding by isnan); the workspace
home of the matrix against the LDS home; single linkage against hdg_linkage; hdg_cut against
hdg_untangle on hdg_linkage's tree and against metrics.cut_groups / cut_table on the others.
No tolerances.

Shapes: nc 2 and 3 (one and two merges), 33, the tile edges 64 / 65, 74 (the glide shape), 129
(three tile rows), and HDG_AG_LDS_MAX_NC and the next nc, where the matrix moves from LDS to
the workspace; B = 3, but B = 1 and rule "mean" only at the two largest.
"""
import ctypes
import types

import numpy as np
import pytest
import torch

from _decode import (B, T, _cut, _linkage_run, _onehot, _pairs, _planted, _planted_labels, _probs,
                     _same, _uniform, _untangle_run, _with_infs, _with_nans)
from _decode import _AgglomerateBufs as _Bufs
from _decode import _agglomerate_run as _run
from hdgnn import _lib, data, layout, metrics
from hdgnn.synth import synth_commits

pytestmark = pytest.mark.gpu

RULES = ("mean", "any", "both")
METHODS = ("single", "complete", "average")
LDS_MAX = _lib.AG_LDS_MAX_NC
SMALL = [2, 3, 33, T, T + 1, 74, 2 * T + 1]
LARGE = [LDS_MAX, LDS_MAX + 1]
SHAPES = SMALL + LARGE


def test_shapes_follow_from_the_header_constants():
    assert SHAPES == [2, 3, 33, T, T + 1, 74, 2 * T + 1, LDS_MAX, LDS_MAX + 1]
    assert max(SMALL) < LDS_MAX and LDS_MAX >= 160
    if (T, LDS_MAX) == (64, 256):
        assert SHAPES == [2, 3, 33, 64, 65, 74, 129, 256, 257]


def _nb(nc):
    return B if nc in SMALL else 1


def _rules(nc):
    return RULES if nc in SMALL else ("mean",)


# ---------------------------------------------------------------------------------------
# running the library and the host
# ---------------------------------------------------------------------------------------
_HOST = {}


def _host(key, y, p1, rule, method):
    """The host restatement, computed once per input set and shared."""
    k = (key, rule, method)
    if k not in _HOST:
        out = metrics.agglomerate(_onehot(y), _probs(p1), rule, method)
        for a in out:
            a.setflags(write=False)
        _HOST[k] = out
    return _HOST[k]


def _check(key, y, p1, rules=RULES, methods=METHODS, flags=0):
    for rule in rules:
        for method in methods:
            _, dev = _run(y, p1, rule, method, flags)
            host = _host(key, y, p1, rule, method)
            print(key, rule, method, "device lk", dev[4].tolist(), "host lk", host[4].tolist())
            _same(dev, host, "%s %s %s" % (key, rule, method))
            assert (np.diff(dev[1], axis=1) > 0).sum() == 0


# ---------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------
def _encoded(nc, nb):
    """test_scores_that_encode_their_relation's scores: neither symmetric nor smooth in (p, q)."""
    I, J = _pairs(nc)
    y = _planted_labels(nc, np.random.default_rng(700 + nc), nb)
    M = 128
    while M < 2 * nc:
        M *= 2
    p1 = np.stack([((I * (37 + 2 * b) + J * 101 + (I * J) % 7 + 11 * b) % M) / float(M)
                   for b in range(nb)]).astype(np.float32)
    return y, p1


def _ulps(nc, nb):
    """0.75 + {0 .. 3} ulps: the fp32 sums of average linkage round, raw levels invert."""
    rng = np.random.default_rng(800 + nc)
    base = np.float32(0.75).view(np.uint32)
    p1 = (base + rng.integers(0, 4, (nb, nc * (nc - 1))).astype(np.uint32)).view(np.float32)
    return _planted_labels(nc, rng, nb), p1


# ---------------------------------------------------------------------------------------
# device == host
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("nc", SHAPES)
def test_planted_groups(nc):
    y, p1 = _planted(nc, seed=nc, nb=_nb(nc))         # the 1/256 grid: many ties
    _check("planted %d" % nc, y, p1, _rules(nc))


@pytest.mark.parametrize("nc", SHAPES)
def test_uniform_scores(nc):
    y, p1 = _uniform(nc, seed=nc, nb=_nb(nc))
    _check("uniform %d" % nc, y, p1, _rules(nc))


@pytest.mark.parametrize("nc", SMALL)
def test_nan_in_one_direction_and_an_isolated_hunk(nc):
    y, p1, nans = _with_nans(nc, B)
    _check("nan %d" % nc, y, p1)
    for method in METHODS:
        lk = _host("nan %d" % nc, y, p1, "mean", method)[4]
        np.testing.assert_array_equal(lk[:, _lib.LK_NAN], nans)
        if nc >= 33:
            assert lk[1, _lib.LK_MERGES] <= nc - 2


@pytest.mark.parametrize("nc", [3, T + 1])
def test_infinite_scores(nc):
    """Under mean a pair of +inf and -inf is no edge and counts in LK_NAN; hdg_untangle's
    UT_NAN, which counts NaN scores, stays 0 on the same input."""
    y, p1 = _with_infs(*_planted(nc, seed=50 + nc), seed=50 + nc)
    key, methods = "inf %d" % nc, METHODS if nc == 3 else ("average",)
    with np.errstate(invalid="ignore"):             # _check's np.diff of two infinite levels
        _check(key, y, p1, methods=methods)
        if nc == 3:
            _check(key, y, p1, flags=_lib.AG_FLAG_GLOBAL)
    for method in methods:
        mean = _host(key, y, p1, "mean", method)[4][:, _lib.LK_NAN]
        both = _host(key, y, p1, "both", method)[4][:, _lib.LK_NAN]
        assert (mean >= 1).all() and (both == 0).all()
    ut = metrics.untangle_counts(_onehot(y), _probs(p1), 0.5, "mean")[0]
    assert (ut[:, _lib.UT_NAN] == 0).all()


@pytest.mark.parametrize("nc", [33, T + 1, 2 * T + 1])
def test_scores_that_encode_their_relation(nc):
    y, p1 = _encoded(nc, B)
    _check("encoded %d" % nc, y, p1)


@pytest.mark.parametrize("nc", [8, 33, 74])
def test_scores_an_ulp_apart(nc):
    y, p1 = _ulps(nc, 8 if nc == 8 else B)
    _check("ulps %d" % nc, y, p1)


def test_the_ulp_family_inverts_raw_levels():
    """... so the family above does exercise the running minimum on the device."""
    y, p1 = _ulps(8, 8)
    raw = metrics.agglomerate(_onehot(y), _probs(p1), "any", "average", raw=True)[5]
    assert (np.diff(raw, axis=1) > 0).any()


@pytest.mark.parametrize("nc", [33, 74])
def test_the_workspace_home_gives_the_lds_homes_bits(nc):
    for (y, p1) in (_planted(nc, seed=nc), _ulps(nc, B), _with_nans(nc, B)[:2]):
        for rule in RULES:
            for method in METHODS:
                _, lds = _run(y, p1, rule, method, 0)
                _, glb = _run(y, p1, rule, method, _lib.AG_FLAG_GLOBAL)
                for a, c in zip(lds, glb):
                    np.testing.assert_array_equal(a.view(np.uint8), c.view(np.uint8))
    y, p1 = _uniform(nc, seed=nc)
    _check("uniform %d" % nc, y, p1, flags=_lib.AG_FLAG_GLOBAL)


# ---------------------------------------------------------------------------------------
# against the existing kernels
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("nc", [T + 1, 74, 2 * T + 1, LDS_MAX + 1])
def test_single_is_hdg_linkages_tree(nc):
    nb = _nb(nc)
    for y, p1 in (_planted(nc, seed=40 + nc, nb=nb), _uniform(nc, seed=40 + nc, nb=nb)):
        for rule in _rules(nc):
            _, (m, lv, cv, t, lk) = _run(y, p1, rule, "single")
            _, (hm, hlv, hcv, ht, hlk) = _linkage_run(y, p1, rule)
            np.testing.assert_array_equal(lv.view(np.uint32), hlv.view(np.uint32))
            np.testing.assert_array_equal(lk, hlk)
            np.testing.assert_array_equal(t, ht)
            for b in range(nb):
                M = int(lk[b, _lib.LK_MERGES])
                reach = np.flatnonzero(np.append(lv[b, 1:M], -np.inf) < lv[b, :M])
                np.testing.assert_array_equal(cv[b, reach], hcv[b, reach])


def _reachable(lv, M):
    nxt = np.append(lv[1:M].astype(np.float64), -np.inf)
    reach = np.flatnonzero(nxt < lv[:M])
    assert len(reach) >= 4
    return [(int(k), np.float32(nxt[k])) for k in reach[[0, len(reach) // 3, 2 * len(reach) // 3, -1]]]


@pytest.mark.parametrize("nc", [T + 1, 2 * T + 1])
def test_cut_of_hdg_linkages_tree_is_hdg_untangle(nc):
    y, p1 = _uniform(nc, seed=60 + nc)
    for rule in RULES:
        _, (m, lv, cv, _, lk) = _linkage_run(y, p1, rule)
        for k, tp in _reachable(lv[0], int(lk[0, _lib.LK_MERGES])):
            thr = float(tp / np.float32(2)) if rule == "mean" else float(tp)
            _, ug, _, ut = _untangle_run(y, p1, thr, rule)
            g, row = _cut(nc, m, lv, cv, lk, thr, rule)
            print(nc, rule, k, "cut", row.tolist(), "untangle", ut.tolist())
            np.testing.assert_array_equal(g, ug)
            keep = [s for s in range(_lib.CUT_SLOTS) if s != _lib.CUT_MERGES]
            np.testing.assert_array_equal(row[:, keep], ut[:, keep])
            assert row[0, _lib.CUT_MERGES] == k + 1
            np.testing.assert_array_equal(row[:, _lib.CUT_MERGES], nc - ut[:, _lib.UT_GROUPS])


@pytest.mark.parametrize("nc", [33, 74])
def test_cut_of_agglomerate_trees(nc):
    y, p1, _ = _with_nans(nc, B)
    for rule in RULES:
        for method in METHODS:
            _, (m, lv, cv, _, lk) = _run(y, p1, rule, method)
            bounds = _reachable(lv[0], int(lk[0, _lib.LK_MERGES])) + [(0, np.float32(np.inf)),
                                                                      (0, np.float32(-np.inf))]
            for _, tp in bounds:
                thr = float(tp / np.float32(2)) if rule == "mean" else float(tp)
                g, row = _cut(nc, m, lv, cv, lk, thr, rule)
                np.testing.assert_array_equal(g, metrics.cut_groups(m, lv, tp))
                want = metrics.cut_table(lv, cv, lk, tp)
                want[:, _lib.CUT_MERGES] = nc - want[:, _lib.CUT_GROUPS]
                np.testing.assert_array_equal(row, want)
                g2, row2 = _cut(nc, m, lv, cv, lk, thr, rule, ut=False)     # ut = NULL
                np.testing.assert_array_equal(g2, g)
                assert (row2 == -1).all()


# ---------------------------------------------------------------------------------------
# outputs and arguments
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", [0, _lib.AG_FLAG_GLOBAL])
def test_repeat_launch_other_inputs_and_null_tgroups(flags):
    nc = 74
    y, p1 = _planted(nc, seed=901)
    host = metrics.agglomerate(_onehot(y), _probs(p1))
    bufs, first = _run(y, p1, flags=flags)
    _same(first, host)
    assert not any(bool((x == v).any()) for x, v in zip(bufs.outputs(), (-7, 12345.0, -7, -7, -1)))
    _, again = _run(y, p1, flags=flags, bufs=bufs)              # into the used buffers
    for x, z in zip(first, again):
        np.testing.assert_array_equal(x.view(np.uint8), z.view(np.uint8))     # the same bits
    y3, p3 = _uniform(nc, seed=902)                             # other inputs, same buffers
    p3[0, :nc - 1] = np.nan                                     # fewer merges than before
    _, other = _run(y3, p3, "any", "complete", flags=flags, bufs=bufs)
    _same(other, metrics.agglomerate(_onehot(y3), _probs(p3), "any", "complete"))
    fresh, nul = _run(y, p1, flags=flags, tgroups=False)        # tgroups = NULL
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
    base = dict(shape=ok_shape, bt=ok_bt, probs=vp(pt.data_ptr()), rule=0, method=2, flags=0,
                merges=vp(bufs.merges.data_ptr()), levels=vp(bufs.levels.data_ptr()),
                curve=vp(bufs.curve.data_ptr()), lk=vp(bufs.lk.data_ptr()),
                ws=vp(bufs.ws.data_ptr()))

    def call(**kw):
        a = dict(base, **kw)
        stream = vp(torch.cuda.current_stream(dev).cuda_stream)
        return lib.hdg_agglomerate(ctypes.byref(a["shape"]), ctypes.byref(a["bt"]), a["probs"],
                                   a["rule"], a["method"], a["flags"], a["merges"], a["levels"],
                                   a["curve"], None, a["lk"], a["ws"], stream)

    bad = [dict(rule=3), dict(rule=-1), dict(method=3), dict(method=-1), dict(flags=2),
           dict(flags=4 | _lib.AG_FLAG_GLOBAL), dict(probs=None), dict(merges=None),
           dict(levels=None), dict(curve=None), dict(lk=None), dict(ws=None),
           dict(ws=vp(bufs.ws.data_ptr() + 4)),
           dict(bt=_lib.Batch(None, None, None, None, None, None)),
           dict(shape=_lib.Shape(0, 20, nc, 2, B, 0)), dict(shape=_lib.Shape(65536, 20, nc, 2, B, 0)),
           dict(shape=_lib.Shape(B, 20, 1, 2, B, 0)), dict(shape=_lib.Shape(B, 20, 2049, 2, B, 0))]
    for kw in bad:
        assert call(**kw) == 1000, kw
        assert lib.hdg_last_error().startswith(b"hdg_agglomerate:"), kw
    groups = torch.full((B, nc), -7, dtype=torch.int32, device=dev)
    row = torch.full((B, _lib.CUT_SLOTS), -1, dtype=torch.int64, device=dev)

    def cut(thr=0.5, rule=0, curve=base["curve"], lk=base["lk"], merges=base["merges"]):
        stream = vp(torch.cuda.current_stream(dev).cuda_stream)
        return lib.hdg_cut(ctypes.byref(ok_shape), merges, base["levels"], curve, lk,
                           ctypes.c_float(thr), rule, vp(groups.data_ptr()), vp(row.data_ptr()),
                           stream)

    for kw in (dict(thr=float("nan")), dict(rule=3), dict(curve=None), dict(lk=None),
               dict(merges=None)):
        assert cut(**kw) == 1000, kw
        assert lib.hdg_last_error().startswith(b"hdg_cut:"), kw
    torch.cuda.synchronize(dev)
    assert bufs.poisoned() and (groups == -7).all() and (row == -1).all()
    assert call() == 0
    assert cut() == 0
    torch.cuda.synchronize(dev)
    assert (bufs.lk >= 0).all() and (bufs.lk[:, _lib.LK_MERGES] == nc - 1).all()
    assert (groups >= 0).all() and (row >= 0).all()


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
    return tuple(x.cpu().numpy() for x in out)


def test_engine_forward_then_agglomerate_then_cut():
    eng, db, label, nc, b = _engine(21)
    probs, _, _ = eng.forward(db)
    out = eng.agglomerate(db)
    merges, levels, curve, tgroups, lk = out
    assert all(x.is_cuda for x in out)
    assert merges.dtype == torch.int32 and tuple(merges.shape) == (b, nc - 1, 2)
    assert levels.dtype == torch.float32 and tuple(levels.shape) == (b, nc - 1)
    assert curve.dtype == torch.int32 and tuple(curve.shape) == (b, nc - 1, 2)
    assert tgroups.dtype == torch.int32 and tuple(tgroups.shape) == (b, nc)
    assert lk.dtype == torch.int64 and tuple(lk.shape) == (b, _lib.LK_SLOTS)
    _same(_np(out), metrics.agglomerate(label, probs.cpu().numpy()))
    ws = eng._ag_workspace
    fake = torch.rand_like(probs)
    for rule in RULES:
        for method in METHODS:
            out = eng.agglomerate(db, fake, rule=rule, method=method)
            host = metrics.agglomerate(label, fake.cpu().numpy(), rule, method)
            _same(_np(out), host)
            thr = 0.6
            groups, ut = eng.cut(out[0], out[1], out[2], out[4], threshold=thr, rule=rule)
            assert groups.dtype == torch.int32 and tuple(groups.shape) == (b, nc) and groups.is_cuda
            assert ut.dtype == torch.int64 and tuple(ut.shape) == (b, _lib.CUT_SLOTS)
            tp = np.float32(thr) + np.float32(thr) if rule == "mean" else np.float32(thr)
            np.testing.assert_array_equal(groups.cpu().numpy(),
                                          metrics.cut_groups(host[0], host[1], tp))
            want = metrics.cut_table(host[1], host[2], host[4], tp)
            want[:, _lib.CUT_MERGES] = nc - want[:, _lib.CUT_GROUPS]
            np.testing.assert_array_equal(ut.cpu().numpy(), want)
    assert eng._ag_workspace is ws                               # allocated once
    with pytest.raises(ValueError):
        eng.agglomerate(db, fake[:, :, :-1])
    with pytest.raises(ValueError):
        eng.agglomerate(db, fake, rule="most")
    with pytest.raises(ValueError):
        eng.agglomerate(db, fake, method="ward")
    with pytest.raises(ValueError):
        eng.cut(out[0], out[1].double(), out[2], out[4])
    eng.check_status()


def test_agglomerate_and_cut_are_graph_capturable():
    """All four launches replay from a captured graph on new scores."""
    eng, db, label, nc, b = _engine(22)
    scores = torch.rand(b, 2, nc * (nc - 1), device=eng.device)
    warm = eng.agglomerate(db, scores, rule="any")  # warm: module loaded, workspace allocated
    eng.cut(warm[0], warm[1], warm[2], warm[4])
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = eng.agglomerate(db, scores, rule="any", method="average")
        groups, ut = eng.cut(out[0], out[1], out[2], out[4], threshold=0.7, rule="any")
    for _ in range(2):
        scores.copy_(torch.rand_like(scores))
        g.replay()
        torch.cuda.synchronize()
        host = metrics.agglomerate(label, scores.cpu().numpy(), "any", "average")
        _same(_np(out), host)
        np.testing.assert_array_equal(groups.cpu().numpy(),
                                      metrics.cut_groups(host[0], host[1], np.float32(0.7)))


def test_graph2graph_calibrate_then_untangle_with_average_linkage(golden_dir, tmp_path,
                                                                  monkeypatch, capsys):
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
    thr, scores, levels, curve, lk = m2.calibrate(args, part="train", rule="mean", score="f1",
                                                  method="average")
    out = capsys.readouterr().out
    assert " [*] Load SUCCESS" in out and "Load failed" not in out
    for line in ("calibrate rule: mean", "calibrate method: average", "calibrate score: f1 = ",
                 "calibrate threshold: "):
        assert line in out, line
    n = len(lk)
    assert n > 0 and n % mb == 0
    d = tmp_path / "outputSelf" / "tiny" / "model_2" / "2"
    np.testing.assert_array_equal(np.load(d / ("agglo_average_levels%d.npy" % ne)).view(np.uint32),
                                  levels.view(np.uint32))
    np.testing.assert_array_equal(np.load(d / ("agglo_average_curve%d.npy" % ne)), curve)
    np.testing.assert_array_equal(np.load(d / ("agglo_average_counts%d.npy" % ne)), lk)
    saved = np.load(d / ("agglo_average_merges%d.npy" % ne))
    assert not (d / ("linkage_levels%d.npy" % ne)).exists()
    # the host trees of the probabilities a forward of the same batches returns
    train, _, maps = data.compact_from_read_data(tup, ne, nc, mb)
    dbs = m2._device_batches(train, maps)
    want = [metrics.agglomerate(data.onehot_relations(train.y[j * mb:(j + 1) * mb]),
                                m2.engine.forward(db)[0].cpu().numpy(), "mean", "average")
            for j, db in enumerate(dbs)]
    host = tuple(np.concatenate([w[i] for w in want]) for i in range(5))
    _same((saved, levels, curve, host[3], lk), host)
    hthr, hbest, htp = metrics.best_threshold(host[1], host[2], host[4], "mean", "f1")
    assert thr == hthr and scores["f1"] == hbest
    print("calibrated threshold", thr, "f1", hbest, "bound", htp)
    # untangling the same split at that threshold scores what the calibration promised
    uscores, table, groups = m2.untangle(args, part="train", threshold=thr, method="average")
    out = capsys.readouterr().out
    assert "untangle method: average" in out
    assert uscores["f1"] == hbest
    np.testing.assert_equal({k: v for k, v in uscores.items()},
                            {k: v for k, v in scores.items()})
    np.testing.assert_array_equal(groups, metrics.cut_groups(host[0], host[1], htp))
    np.testing.assert_array_equal(np.load(d / ("untangle_groups%d.npy" % ne)), groups)
    # "single" is the path it always was
    s_single, t_single, _ = m2.untangle(args, part="train", threshold=thr, method="single")
    s_default, t_default, _ = m2.untangle(args, part="train", threshold=thr)
    np.testing.assert_array_equal(t_single, t_default)
    assert "untangle method" not in capsys.readouterr().out
