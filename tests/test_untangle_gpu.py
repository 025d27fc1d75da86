"""hdg_untangle on the GPU: groups, true groups and every table row compared for integer
equality with the host implementation (hdgnn.metrics.untangle_counts) -- no tolerances.

Shapes are the smallest at which each piece of the kernels can break, derived from the
header constants (written here for HDG_UT_TILE = 64, 4 tile pairs per block), B = 3 each:
    nc   2   one pair
    nc  33   label rows cross one 32-bit word, a tile that is mostly padding
    nc  64   one full tile
    nc  65   a one-wide edge tile and its mirror
    nc  74   the glide shape: 3 tile pairs on one block
    nc 128   two full tile rows, still one block
    nc 129   6 tile pairs on two blocks
    nc 193   10 tile pairs on three blocks, dealt 4 / 3 / 3
and nc 705 at B = 1: 78 tile pairs on the 16 blocks the cap allows (4 or 5 per block).
"""
import ctypes
import math
import types

import numpy as np
import pytest
import torch

from _decode import (B, BIG, MAXB, NC_CAPPED, NC_THREE, NC_TWO, SHAPES, T, TPB, _bridged_groups,
                     _onehot, _owner, _pairs, _planted, _planted_labels, _probs, _scores_of,
                     _sym, _tile_pairs, _uniform, _with_infs)
from _decode import _UntangleBufs as _Bufs
from _decode import _untangle_run as _run
from hdgnn import _lib, data, layout, metrics
from hdgnn.synth import synth_commits

pytestmark = pytest.mark.gpu


def test_shapes_are_the_block_edges():
    assert _lib.untangle_blocks(T) == 1 and _tile_pairs(T) == 1 and _tile_pairs(T + 1) == 3
    assert _lib.untangle_blocks(NC_TWO - 1) == 1 and _lib.untangle_blocks(NC_TWO) == 2
    assert (NC_TWO - 1) % T == 0                                   # full tiles only, then an edge
    assert _lib.untangle_blocks(NC_THREE - 1) == 2 and _lib.untangle_blocks(NC_THREE) == 3
    assert _tile_pairs(NC_THREE) % 3 != 0                          # an uneven deal
    assert _lib.untangle_blocks(NC_CAPPED) == MAXB < -(-_tile_pairs(NC_CAPPED) // TPB)
    if (T, TPB, MAXB) == (64, 4, 16):
        assert SHAPES == [2, 33, 64, 65, 74, 128, 129, 193]


# ---------------------------------------------------------------------------------------
# running the library and the host
# ---------------------------------------------------------------------------------------
def _host(y, p1, thr=0.5, rule="mean"):
    return metrics.untangle_counts(_onehot(y), _probs(p1), thr, rule)


def _check(y, p1, thr=0.5, rule="mean", what=""):
    """Device == host, all three outputs; -> the host's (ut, groups, tgroups)."""
    _, g, t, ut = _run(y, p1, thr, rule)
    hut, hg, ht = _host(y, p1, thr, rule)
    print(what, rule, thr, "device", ut.tolist(), "host", hut.tolist())
    np.testing.assert_array_equal(ut, hut)
    np.testing.assert_array_equal(g, hg)
    np.testing.assert_array_equal(t, ht)
    nc = g.shape[1]
    four = [_lib.UT_SS, _lib.UT_SD, _lib.UT_DS, _lib.UT_DD]
    assert (ut[:, four].sum(1) == nc * (nc - 1) // 2).all()
    return hut, hg, ht


# ---------------------------------------------------------------------------------------
# shapes x score sets
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("nc", SHAPES)
def test_planted_groups(nc):
    y, p1 = _planted(nc, seed=nc)
    ut, g, t = _check(y, p1, 0.5, "mean", "planted nc %d" % nc)
    if nc >= T + 1:      # a real partition on both sides, and every kind of pair present
        assert ((ut[:, _lib.UT_GROUPS] > 1) & (ut[:, _lib.UT_GROUPS] < nc)).all()
        for k in (_lib.UT_SS, _lib.UT_SD, _lib.UT_DS, _lib.UT_DD):
            assert (ut[:, k] > 0).all(), k
    _check(y, p1, 0.5, "any", "planted nc %d" % nc)
    _check(y, p1, 0.5, "both", "planted nc %d" % nc)


@pytest.mark.parametrize("nc", SHAPES)
def test_uniform_scores(nc):
    y, p1 = _uniform(nc, seed=nc)
    _check(y, p1, 0.5, "mean", "uniform nc %d" % nc)            # dense: one group
    # near the point where the giant component forms: many groups of many sizes
    ut, _, _ = _check(y, p1, 1.0 - 0.7 / math.sqrt(nc), "both", "uniform nc %d" % nc)
    _check(y, p1, 0.9, "mean", "uniform nc %d" % nc)
    _check(y, p1, 0.995, "any", "uniform nc %d" % nc)
    if nc >= T + 1:
        assert (ut[:, _lib.UT_GROUPS] > 1).all() and (ut[:, _lib.UT_LINKS] > 0).all()


@pytest.mark.parametrize("nc", SHAPES)
def test_scores_at_the_threshold_and_one_ulp_above(nc):
    """Strict comparisons: a score equal to the threshold does not link, the next float does;
    under the mean rule the sum of the two is rounded once, as the host does it in float32."""
    rng = np.random.default_rng(200 + nc)
    thr = np.float32(0.3)
    up = np.nextafter(thr, np.float32(1))
    I, J = _pairs(nc)
    R = len(I)
    for density in (1.0, 2.0 / nc):
        a = _sym(nc, rng, B, density)                         # pairs with s_pq one ulp up ...
        b = _sym(nc, rng, B, density)                         # ... and, on their own, s_qp
        upper = I < J
        p1 = np.where((a & upper) | (b & ~upper), up, thr).astype(np.float32)
        y = _planted_labels(nc, rng, B)
        for rule in ("mean", "any", "both"):
            ut, _, _ = _check(y, p1, float(thr), rule, "ulp nc %d" % nc)
            if density == 1.0:
                assert (ut[:, _lib.UT_LINKS] == nc * (nc - 1) // 2).all()
    at = np.full((B, R), thr, np.float32)
    for rule in ("mean", "any", "both"):
        ut, g, _ = _check(_planted_labels(nc, rng, B), at, float(thr), rule, "at nc %d" % nc)
        assert (ut[:, _lib.UT_LINKS] == 0).all() and (ut[:, _lib.UT_GROUPS] == nc).all()


@pytest.mark.parametrize("nc", SHAPES)
def test_nan_in_one_direction(nc):
    y, p1 = _planted(nc, seed=300 + nc)
    rng = np.random.default_rng(300 + nc)
    I, J = _pairs(nc)
    hit = _sym(nc, rng, B, 0.05)
    hit[:, (I == 0) & (J == 1)] = hit[:, (I == 1) & (J == 0)] = True
    first = _sym(nc, rng, B, 0.5) ^ (I < J)                   # which direction carries the NaN
    p1 = p1.copy()
    p1[hit & first] = np.nan
    n_hit = hit.sum(1) // 2
    for rule in ("mean", "any", "both"):
        ut, _, _ = _check(y, p1, 0.5, rule, "nan nc %d" % nc)
        np.testing.assert_array_equal(ut[:, _lib.UT_NAN], n_hit)
    # exactly one direction of every hit pair is NaN
    S = np.zeros((B, nc, nc), np.float32)
    S[:, I, J] = p1
    nan = np.isnan(S)
    assert not (nan & nan.transpose(0, 2, 1)).any() and nan.sum() == n_hit.sum()


@pytest.mark.parametrize("nc", [3, T + 1])
def test_infinite_scores(nc):
    """Under mean a pair of +inf and -inf has a NaN weight: it does not link, and it is not in
    UT_NAN, which counts NaN scores -- though hdg_linkage counts it as no edge."""
    y, p1 = _with_infs(*_planted(nc, seed=50 + nc), seed=50 + nc)
    for rule in ("mean", "any", "both"):
        ut, _, _ = _check(y, p1, 0.5, rule, "inf nc %d" % nc)
        assert (ut[:, _lib.UT_NAN] == 0).all()
    lk = metrics.linkage(_onehot(y), _probs(p1), "mean")[4]
    assert (lk[:, _lib.LK_NAN] >= 1).all()


def test_capped_shape_sixteen_blocks():
    """nc 705, one commit: two interleaved paths (even hunks, odd hunks) whose links lie in
    every tile pair near the diagonal, a star across all tile rows on hunk 3, and a clique."""
    nc = NC_CAPPED
    assert _tile_pairs(nc) > TPB * MAXB
    rng = np.random.default_rng(7)
    I, J = _pairs(nc)
    link = (np.abs(I - J) == 2)                                # evens | odds
    link |= ((I == 3) | (J == 3)) & ((I + J) % 64 == 3) & ((I + J) % 2 == 0)
    clique = (I >= 600) & (I < 640) & (J >= 600) & (J < 640) & ((I + J) % 2 == 1)
    p1 = np.where(link, 0.75, 0.125).astype(np.float32)[None]
    y = _planted_labels(nc, rng, 1, k=4)
    ut, g, _ = _check(y, p1, 0.5, "mean", "capped")
    assert ut[0, _lib.UT_GROUPS] == 2 and g[0, :4].tolist() == [0, 1, 0, 1]
    p1 = np.where(link | clique, 0.75, 0.125).astype(np.float32)[None]
    ut, _, _ = _check(y, p1, 0.5, "mean", "capped + clique")
    assert ut[0, _lib.UT_GROUPS] == 1


# ---------------------------------------------------------------------------------------
# structures that break a wrong union-find or a wrong merge of the blocks' forests
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("nc", BIG)
def test_paths_stars_cliques(nc):
    rng = np.random.default_rng(400 + nc)
    y = _planted_labels(nc, rng, B)
    path = [(i, i + 1) for i in range(nc - 1)]
    star = [(i, nc - 1) for i in range(nc - 1)]
    # the path, plain; seen only from the top down (the score from the higher hunk to the
    # lower one alone is high: every link comes out of the mirror tile); and with the links
    # of the two ends alternating, so that the roots keep being lowered from far away
    zig = []
    for k in range(nc // 2):
        zig += [(nc - 1 - k, k), (k, nc - 2 - k)]
    zig = [e for e in zig if e[0] != e[1]]
    p1 = np.stack([_scores_of(nc, path), _scores_of(nc, path, "down"), _scores_of(nc, zig, "up")])
    ut, g, _ = _check(y, p1, 0.5, "any", "paths nc %d" % nc)
    assert (ut[:, _lib.UT_GROUPS] == 1).all() and not g.any()
    assert ut[:, _lib.UT_LINKS].tolist() == [nc - 1, nc - 1, len(set(map(frozenset, zig)))]
    ut, _, _ = _check(y, p1, 0.5, "both", "paths nc %d" % nc)
    assert ut[:, _lib.UT_GROUPS].tolist() == [1, nc, nc]
    # a star on the last hunk, the complete graph, no links at all
    full = np.full(nc * (nc - 1), 0.75, np.float32)
    none = np.full(nc * (nc - 1), 0.125, np.float32)
    p1 = np.stack([_scores_of(nc, star), full, none])
    ut, g, _ = _check(y, p1, 0.5, "mean", "star / complete / empty nc %d" % nc)
    assert ut[:, _lib.UT_GROUPS].tolist() == [1, 1, nc]
    assert ut[:, _lib.UT_LINKS].tolist() == [nc - 1, nc * (nc - 1) // 2, 0]
    assert g[2].tolist() == list(range(nc))


@pytest.mark.parametrize("nc", BIG)
def test_groups_joined_by_another_blocks_link(nc):
    own = _owner(nc)
    edges, A, Bm, bridge = _bridged_groups(nc)
    assert all(own[p, q] == 0 for p, q in edges) and own[bridge] != 0
    rng = np.random.default_rng(500 + nc)
    y = _planted_labels(nc, rng, 2)
    p1 = np.stack([_scores_of(nc, edges), _scores_of(nc, edges + [bridge])])
    ut, g, _ = _check(y, p1, 0.5, "mean", "bridge nc %d" % nc)
    members = len(set(A) | set(Bm))
    assert ut[:, _lib.UT_GROUPS].tolist() == [nc - members + 2, nc - members + 1]
    assert g[0, Bm[0]] != g[0, 0] and len(set(g[0, Bm])) == 1
    assert len(set(g[1, A + Bm])) == 1


# ---------------------------------------------------------------------------------------
# orientation: which score is s_pq and which s_qp
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("nc", [T + 1, NC_TWO])
def test_directed_scores(nc):
    rng = np.random.default_rng(600 + nc)
    I, J = _pairs(nc)
    y = _planted_labels(nc, rng, B)
    a = _sym(nc, rng, B, 3.0 / nc)              # s_pq 0.875, s_qp 0.25 (p < q): sum 1.125
    b = _sym(nc, rng, B, 3.0 / nc) & ~a         # s_pq 0.625, s_qp 0.25: sum 0.875
    p1 = np.full(a.shape, 0.25, np.float32)
    p1[a & (I < J)] = 0.875
    p1[b & (I < J)] = 0.625
    na, nb_ = a.sum(1) // 2, b.sum(1) // 2
    ut, _, _ = _check(y, p1, 0.5, "any", "directed nc %d" % nc)
    np.testing.assert_array_equal(ut[:, _lib.UT_LINKS], na + nb_)
    ut, _, _ = _check(y, p1, 0.5, "both", "directed nc %d" % nc)
    assert (ut[:, _lib.UT_LINKS] == 0).all()
    ut, _, _ = _check(y, p1, 0.5, "mean", "directed nc %d" % nc)
    np.testing.assert_array_equal(ut[:, _lib.UT_LINKS], na)
    assert (na > 0).all() and (nb_ > 0).all()


@pytest.mark.parametrize("nc", [33, T + 1, NC_TWO, NC_THREE])
def test_scores_that_encode_their_relation(nc):
    """s_pq is a function of (p, q) that is neither symmetric nor smooth: reading a
    neighbouring relation (a wrong [q > p] shift) or the wrong mirror tile changes the links."""
    I, J = _pairs(nc)
    rng = np.random.default_rng(700 + nc)
    y = _planted_labels(nc, rng, B)
    M = 128
    while M < 2 * nc:
        M *= 2
    p1 = np.stack([((I * (37 + 2 * b) + J * 101 + (I * J) % 7 + 11 * b) % M) / float(M)
                   for b in range(B)]).astype(np.float32)
    # thresholds that link a pair with probability about 1 / M under each rule: a mean degree
    # below one, so many groups of several sizes
    k = math.sqrt(M)
    for rule, thr in (("mean", 1.0 - k / (1.4 * M)), ("any", 1.0 - 1.5 / M),
                      ("both", 1.0 - (k + 0.5) / M)):
        ut, _, _ = _check(y, p1, thr, rule, "encoded nc %d" % nc)
        assert ((ut[:, _lib.UT_LINKS] > 0) & (ut[:, _lib.UT_GROUPS] > 1)).all(), rule


@pytest.mark.parametrize("nc", [T + 1, NC_TWO])
def test_antisymmetric_labels_give_the_same_true_groups(nc):
    rng = np.random.default_rng(800 + nc)
    I, J = _pairs(nc)
    gt = rng.integers(0, 5, (B, nc))
    within = (gt[:, I] == gt[:, J]) & _sym(nc, rng, B, 4.0 / nc)
    y_sym = within.astype(np.uint8)
    y_up = (within & (I < J)).astype(np.uint8)                  # only y_pq, p < q
    y_down = (within & (I > J)).astype(np.uint8)
    _, p1 = _planted(nc, seed=nc)
    _, _, t_sym = _check(y_sym, p1, 0.5, "mean", "labels sym")
    _, _, t_up = _check(y_up, p1, 0.5, "mean", "labels up")
    _, _, t_down = _check(y_down, p1, 0.5, "mean", "labels down")
    np.testing.assert_array_equal(t_up, t_sym)
    np.testing.assert_array_equal(t_down, t_sym)
    assert (t_sym.max(1) > 0).all()


# ---------------------------------------------------------------------------------------
# outputs and arguments
# ---------------------------------------------------------------------------------------
def test_repeat_launch_and_null_tgroups():
    nc = NC_THREE
    y, p1 = _planted(nc, seed=901)
    bufs, g1, t1, ut1 = _run(y, p1)
    hut, hg, ht = _host(y, p1)
    np.testing.assert_array_equal(ut1, hut)
    np.testing.assert_array_equal(g1, hg)
    np.testing.assert_array_equal(t1, ht)
    _, g2, t2, ut2 = _run(y, p1, bufs=bufs)                    # into the used buffers
    np.testing.assert_array_equal(ut2, ut1)
    np.testing.assert_array_equal(g2, g1)
    np.testing.assert_array_equal(t2, t1)
    y3, p3 = _planted(nc, seed=902)                             # other inputs, same buffers
    _, g3, _, ut3 = _run(y3, p3, bufs=bufs)
    np.testing.assert_array_equal(ut3, _host(y3, p3)[0])
    np.testing.assert_array_equal(g3, _host(y3, p3)[1])
    fresh, g4, t4, ut4 = _run(y, p1, tgroups=False)            # tgroups = NULL
    np.testing.assert_array_equal(ut4, ut1)
    np.testing.assert_array_equal(g4, g1)
    assert (t4 == -7).all()                                    # untouched


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
    base = dict(shape=ok_shape, bt=ok_bt, probs=vp(pt.data_ptr()), thr=0.5, rule=0,
                groups=vp(bufs.groups.data_ptr()), ut=vp(bufs.ut.data_ptr()),
                ws=vp(bufs.ws.data_ptr()))

    def call(**kw):
        a = dict(base, **kw)
        stream = vp(torch.cuda.current_stream(dev).cuda_stream)
        return lib.hdg_untangle(ctypes.byref(a["shape"]), ctypes.byref(a["bt"]), a["probs"],
                                ctypes.c_float(a["thr"]), a["rule"], a["groups"], None, a["ut"],
                                a["ws"], stream)

    bad = [dict(rule=3), dict(rule=-1), dict(thr=float("nan")), dict(probs=None),
           dict(groups=None), dict(ut=None), dict(ws=None),
           dict(bt=_lib.Batch(None, None, None, None, None, None)),
           dict(shape=_lib.Shape(0, 20, nc, 2, B, 0)), dict(shape=_lib.Shape(65536, 20, nc, 2, B, 0)),
           dict(shape=_lib.Shape(B, 20, 1, 2, B, 0)), dict(shape=_lib.Shape(B, 20, 2049, 2, B, 0))]
    for kw in bad:
        assert call(**kw) == 1000, kw
        assert lib.hdg_last_error().startswith(b"hdg_untangle:"), kw
    torch.cuda.synchronize(dev)
    assert (bufs.groups == -7).all() and (bufs.ut == -1).all() and (bufs.ws == 0x7F7F7F7F).all()
    assert call() == 0
    torch.cuda.synchronize(dev)
    assert (bufs.ut >= 0).all()


# ---------------------------------------------------------------------------------------
# Engine and graph2graph
# ---------------------------------------------------------------------------------------
def test_engine_forward_then_untangle():
    from hdgnn.engine import Engine
    ne, nc, b = 20, 10, 4
    cb = synth_commits(b, ne, nc, 21)
    eng = Engine(ne, nc, b, variant=2)
    eng.set_params(layout.init_flat(5, 2))
    db = eng.upload(cb)
    label = data.onehot_relations(cb.y)
    probs, _, _ = eng.forward(db)
    groups, ut = eng.untangle(db)
    assert groups.dtype == torch.int32 and tuple(groups.shape) == (b, nc) and groups.is_cuda
    assert ut.dtype == torch.int64 and tuple(ut.shape) == (b, _lib.UT_SLOTS) and ut.is_cuda
    hut, hg, _ = metrics.untangle_counts(label, probs.cpu().numpy())
    np.testing.assert_array_equal(ut.cpu().numpy(), hut)
    np.testing.assert_array_equal(groups.cpu().numpy(), hg)
    ws = eng._ut_workspace
    # an explicit array of the same shape, another rule and threshold
    fake = torch.rand_like(probs)
    for rule, thr in (("mean", 0.7), ("any", 0.9), ("both", 0.6)):
        groups, ut = eng.untangle(db, fake, threshold=thr, rule=rule)
        hut, hg, _ = metrics.untangle_counts(label, fake.cpu().numpy(), thr, rule)
        np.testing.assert_array_equal(ut.cpu().numpy(), hut)
        np.testing.assert_array_equal(groups.cpu().numpy(), hg)
    assert eng._ut_workspace is ws                               # allocated once
    with pytest.raises(ValueError):
        eng.untangle(db, fake[:, :, :-1])
    with pytest.raises(ValueError):
        eng.untangle(db, fake, rule="most")
    eng.check_status()


def test_untangle_is_graph_capturable():
    """Both launches replay from a captured graph on new scores."""
    from hdgnn.engine import Engine
    ne, nc, b = 20, 10, 4
    cb = synth_commits(b, ne, nc, 22)
    eng = Engine(ne, nc, b, variant=2)
    db = eng.upload(cb)
    label = data.onehot_relations(cb.y)
    scores = torch.rand(b, 2, nc * (nc - 1), device=eng.device)
    eng.untangle(db, scores, threshold=0.7)         # warm: module loaded, workspace allocated
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        groups, ut = eng.untangle(db, scores, threshold=0.7)
    for _ in range(2):
        scores.copy_(torch.rand_like(scores))
        g.replay()
        torch.cuda.synchronize()
        hut, hg, _ = metrics.untangle_counts(label, scores.cpu().numpy(), 0.7)
        np.testing.assert_array_equal(ut.cpu().numpy(), hut)
        np.testing.assert_array_equal(groups.cpu().numpy(), hg)


def test_graph2graph_untangle_groups_the_test_commits(golden_dir, tmp_path, monkeypatch, capsys):
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
    trained = m.engine.get_params()
    capsys.readouterr()

    m2 = model(99)                                  # another initialiser: the load must win
    scores, table, groups = m2.untangle(args)
    out = capsys.readouterr().out
    assert " [*] Load SUCCESS" in out and "Load failed" not in out
    assert "untangle rand:" in out and "untangle f1:" in out
    np.testing.assert_array_equal(m2.engine.get_params(), trained)
    assert table.shape == (50, _lib.UT_SLOTS) and table.dtype == np.int64
    assert groups.shape == (50, nc) and groups.dtype == np.int32
    d = tmp_path / "outputSelf" / "tiny" / "model_2" / "2"
    np.testing.assert_array_equal(np.load(d / ("untangle_counts%d.npy" % ne)), table)
    saved = np.load(d / ("untangle_groups%d.npy" % ne))
    assert saved.dtype == np.int32
    np.testing.assert_array_equal(saved, groups)
    four = [_lib.UT_SS, _lib.UT_SD, _lib.UT_DS, _lib.UT_DD]
    assert (table[:, four].sum(1) == nc * (nc - 1) // 2).all()
    assert (groups[:, 0] == 0).all() and (groups.max(1) + 1 == table[:, _lib.UT_GROUPS]).all()
    np.testing.assert_equal(scores, metrics.scores_from_untangle(table))
    # the rows are those of the probabilities a forward of the same batches returns
    _, test, maps = data.compact_from_read_data(tup, ne, nc, mb)
    dbs = m2._device_batches(test, maps)
    want = [metrics.untangle_counts(data.onehot_relations(test.y[j * mb:(j + 1) * mb]),
                                    m2.engine.forward(db)[0].cpu().numpy())
            for j, db in enumerate(dbs)]
    np.testing.assert_array_equal(table, np.concatenate([w[0] for w in want]))
    np.testing.assert_array_equal(groups, np.concatenate([w[1] for w in want]))
    # another rule and threshold, the train part: other commits, another table
    _, ttable, tgroups = m2.untangle(args, part="train", threshold=0.4, rule="any")
    assert ttable.shape == (50, _lib.UT_SLOTS) and tgroups.shape == (50, nc)
