"""hdg_match on the device against hdgnn.metrics.match_counts, integer for integer: mt and
tgroups are compared for equality, `mate` (one optimum, not unique under ties) by its
certificate against the device's own mt and tgroups.  Every output buffer is poisoned before
every call and no poison may survive.

Shapes are the smallest at which each piece can break: nc 2, 3, 7, 14 (one thread row), 33
(label rows cross a word), 64, 65 (a wave and one hunk past it), 74 (glide), 129, 130 (the
128-hunk instance gives way to the 512-hunk one, more than 128 cells) at B = 3; 257 and 258
(past the block's 256 threads: two hunks per thread) at B = 1; 1025 (the 2048-hunk instance,
two hunks per thread in the 1024-thread truth kernel) at B = 1, noisy family only.
"""
import os

import numpy as np
import pytest
import torch

from _decode import B, _untangle_run
from _match import (PLANTED, check_consequences, check_mate, match_run, noisy_sets,
                    relabeled_truth, renumbered, wild_ids)
from hdgnn import _lib, data, layout, metrics
from hdgnn.synth import synth_commits
from test_refine import _onehot, noisy_planted
from test_refine_merge_gpu import FAMILIES

pytestmark = pytest.mark.gpu

SHAPES = [2, 3, 7, 14, 33, 64, 65, 74, 129, 130]
SHAPES_B1 = [257, 258]
TWO_PER_THREAD = 1025


def _same(y, groups, mate=True, tgroups=True):
    """The call on poisoned buffers == the host, no poison left; the certificate of mate."""
    groups = np.asarray(groups, np.int32)
    if groups.ndim == 2:
        groups = groups[None]
    bufs, mt, mt_mate, tg = match_run(y, groups, mate=mate, tgroups=tgroups)
    hmt, hmate, htg = metrics.match_counts(_onehot(y), groups)
    assert not (mt == -1).any()
    np.testing.assert_array_equal(mt, hmt)
    if tgroups:
        np.testing.assert_array_equal(tg, htg)
    else:
        assert (tg == -7).all()
    if mate:
        assert not (mt_mate == -7).any()
        check_mate(mt_mate, groups, htg, mt)
    else:
        assert (mt_mate == -7).all()
    check_mate(hmate, groups, htg, hmt)
    check_consequences(mt, groups, htg)
    return mt


@pytest.mark.parametrize("name", sorted(PLANTED))
def test_planted_values_on_the_device(name):
    y, g, planted = PLANTED[name]()
    mt = _same(y, g)
    for slot, value in planted.items():
        assert mt[0, 0, slot] == value, (name, slot, mt[0, 0])


@pytest.mark.parametrize("family", sorted(FAMILIES))
@pytest.mark.parametrize("nc", SHAPES)
def test_device_is_the_host_restatement(nc, family):
    y, p1 = FAMILIES[family](nc)
    groups = noisy_sets(y, p1, seed=nc, n_sets=3)
    _same(y, groups)
    rng = np.random.default_rng(nc)
    wild = wild_ids(groups, rng)
    mt = _same(y, wild)
    np.testing.assert_array_equal(_same(y, renumbered(wild, rng)), mt)


@pytest.mark.parametrize("nc", SHAPES_B1)
def test_two_hunks_per_thread_of_the_match_block(nc):
    y, p1 = noisy_planted(nc, seed=nc, B=1)
    groups = noisy_sets(y, p1, seed=nc, n_sets=3)
    _same(y, groups)
    _same(y, wild_ids(groups, np.random.default_rng(nc))[:1], mate=False)


def test_two_hunks_per_thread_of_the_truth_block():
    nc = TWO_PER_THREAD
    y, p1 = noisy_planted(nc, seed=nc, B=1)
    groups = noisy_sets(y, p1, seed=nc, n_sets=3)
    _same(y, wild_ids(groups, np.random.default_rng(nc), share=0.02))


def test_sixty_four_sets_each_its_own_relabeling():
    nc = 33
    y, p1 = noisy_planted(nc, seed=64, B=B)
    groups = noisy_sets(y, p1, seed=64, n_sets=_lib.MT_MAX_SETS)
    assert len(groups) == 64 and len({g.tobytes() for g in groups}) == 64
    mt = _same(y, groups)
    assert len({r.tobytes() for r in mt}) > 8
    _same(y, groups[:1], mate=False, tgroups=False)


def test_renumbering_and_out_of_range_ids():
    nc = 74
    y, p1 = noisy_planted(nc, seed=9, B=B)
    tg = metrics.untangle_counts(_onehot(y), np.stack([1 - p1, p1], 1), 0.5)[2]
    rng = np.random.default_rng(9)
    g = relabeled_truth(tg, rng)[None]
    mt = _same(y, g)
    for _ in range(3):
        np.testing.assert_array_equal(_same(y, renumbered(g, rng)), mt)
    alone = np.array([-1, nc, -2 ** 31, 2 ** 31 - 1] * 19, np.int64)[:nc].astype(np.int32)
    mt = _same(y, np.broadcast_to(alone, (1, B, nc)))
    assert (mt[..., _lib.MT_GROUPS] == nc).all() and (mt[..., _lib.MT_PURITY] == nc).all()
    assert (mt[..., _lib.MT_MATCHED] == mt[..., _lib.MT_TGROUPS]).all()


def test_matched_all_iff_untangle_counts_no_wrong_pair():
    """MATCHED == nc exactly where hdg_untangle's row of the same groups has SD = DS = 0."""
    nc = 74
    y, p1 = noisy_planted(nc, seed=21, B=B)
    p1 = p1.copy()
    p1[0] = np.where(y[0] > 0, 0.9, 0.1)                 # commit 0: the scores give the truth
    _, groups, _, ut = _untangle_run(y, p1)
    _, mt, _, _ = match_run(y, groups)
    exact = (ut[:, _lib.UT_SD] == 0) & (ut[:, _lib.UT_DS] == 0)
    np.testing.assert_array_equal(mt[0, :, _lib.MT_MATCHED] == nc, exact)
    assert exact[0] and not exact.all()
    np.testing.assert_array_equal(mt[0, :, _lib.MT_GROUPS], ut[:, _lib.UT_GROUPS])
    np.testing.assert_array_equal(mt[0, :, _lib.MT_TGROUPS], ut[:, _lib.UT_TGROUPS])


def test_buffers_are_reused_and_the_call_repeats_its_bits():
    nc = 130
    y, p1 = noisy_planted(nc, seed=5, B=B)
    groups = noisy_sets(y, p1, seed=5, n_sets=3)
    bufs, mt, mate, tg = match_run(y, groups)
    for _ in range(2):
        _, mt2, mate2, tg2 = match_run(y, groups, bufs=bufs)
        for a, z in ((mt, mt2), (mate, mate2), (tg, tg2)):
            np.testing.assert_array_equal(a, z)


# ---------------------------------------------------------------------------------------
# Engine
# ---------------------------------------------------------------------------------------
def _engine(seed, nc=10):
    from hdgnn.engine import Engine
    ne, b = 20, 4
    cb = synth_commits(b, ne, nc, seed)
    eng = Engine(ne, nc, b, variant=2)
    eng.set_params(layout.init_flat(5, 2))
    return eng, eng.upload(cb), data.onehot_relations(cb.y), nc, b


def test_engine_match_takes_a_split_ladders_groups():
    eng, db, label, nc, b = _engine(51)
    scores = torch.rand(b, 2, nc * (nc - 1), device=eng.device)
    thr = [0.3, 0.45, 0.6]
    tree = eng.agglomerate(db, scores, "mean", "single")[:2]
    _, _, lg = eng.refine_split_ladder(db, thr, tree, scores, max_sweeps=4, max_rounds=2,
                                       kinds="both", groups=True)
    out = eng.match(db, lg, mate=True)
    mt, mate, tg = out
    assert all(x.is_cuda for x in out)
    assert mt.dtype == torch.int64 and tuple(mt.shape) == (3, b, _lib.MT_SLOTS)
    assert mate.dtype == torch.int32 and tuple(mate.shape) == (3, b, nc)
    assert tg.dtype == torch.int32 and tuple(tg.shape) == (b, nc)
    hg = metrics.refine_split_ladder(label, scores.cpu().numpy(), thr,
                                     (tree[0].cpu().numpy(), tree[1].cpu().numpy()), "mean", 4, 2,
                                     3)[1]
    np.testing.assert_array_equal(lg.cpu().numpy(), hg)
    hmt, _, htg = metrics.match_counts(label, hg)
    np.testing.assert_array_equal(mt.cpu().numpy(), hmt)
    np.testing.assert_array_equal(tg.cpu().numpy(), htg)
    check_mate(mate.cpu().numpy(), hg, htg, hmt)
    ws = eng._mt_workspace
    one = eng.match(db, lg[1])                               # [B][nc]: one set
    assert one[1] is None and tuple(one[0].shape) == (1, b, _lib.MT_SLOTS)
    assert torch.equal(one[0][0], mt[1]) and torch.equal(one[2], tg)
    assert eng._mt_workspace is ws
    k, t, acc, vals = metrics.best_rung_match(hmt, thr, nc)
    assert acc == hmt[k, :, _lib.MT_MATCHED].sum() / (b * nc) and t == np.float32(thr[k])
    for bad in (lg.long(), lg.cpu(), lg[:, :, :-1], lg[:, :-1], lg.transpose(0, 1), None):
        with pytest.raises(ValueError):
            eng.match(db, bad)
    with pytest.raises(ValueError):
        eng.match(db, lg, mate=1)
    eng.check_status()


def test_match_is_graph_capturable():
    eng, db, label, nc, b = _engine(52)
    groups = torch.randint(0, 3, (2, b, nc), dtype=torch.int32, device=eng.device)
    eng.match(db, groups, mate=True)                         # warm: the workspace is allocated
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = eng.match(db, groups, mate=True)
    for k in range(2):
        groups.copy_(torch.randint(-1, 4 + k, (2, b, nc), dtype=torch.int32,
                                   device=eng.device))
        graph.replay()
        torch.cuda.synchronize()
        replayed = [x.cpu().numpy() for x in out]
        eager = [x.cpu().numpy() for x in eng.match(db, groups, mate=True)]
        for x, z in zip(replayed, eager):
            np.testing.assert_array_equal(x, z)
        hmt, _, htg = metrics.match_counts(label, groups.cpu().numpy())
        np.testing.assert_array_equal(replayed[0], hmt)
        np.testing.assert_array_equal(replayed[2], htg)
        check_mate(replayed[1], groups.cpu().numpy(), htg, hmt)


def test_graph2graph_untangle_and_calibrate_by_matching(golden_dir, tmp_path, monkeypatch, capsys):
    import types
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
    thr, scores, rungs, table, rq = m.calibrate_refined(args, part="train", score="acc",
                                                        refine=sweeps, ladder=lad, merge=rounds,
                                                        split=True)
    out = capsys.readouterr().out
    n = table.shape[1]
    train, _, maps = data.compact_from_read_data(tup, ne, nc, mb)
    want, cuts = [], []
    for j, db in enumerate(m._device_batches(train, maps)):
        label = data.onehot_relations(train.y[j * mb:(j + 1) * mb])
        probs = m.engine.forward(db)[0].cpu().numpy()
        tree = metrics.linkage(label, probs, "mean")
        hg = metrics.refine_split_ladder(label, probs, rungs, tree[:2], "mean", sweeps, rounds, 3)[1]
        want.append(metrics.match_counts(label, hg)[0])
        plain = np.stack([metrics.cut_groups(tree[0], tree[1], np.float32(t) + np.float32(t))
                          for t in rungs])
        cuts.append(metrics.match_counts(label, plain)[0])
    hmt, hcut = np.concatenate(want, 1), np.concatenate(cuts, 1)
    assert n > 0 and hmt.shape == (5, n, 8)
    np.testing.assert_array_equal(np.load(d / ("refine_ladder_match%d.npy" % ne)), hmt)
    k, t, best, vals = metrics.best_rung_match(hmt, rungs, nc)
    assert thr == t and scores["match"] == metrics.scores_from_match(hmt[k], nc)
    assert "calibrate refined threshold: %r (rung %d), acc = %s" % (t, k, best) in out
    _, tt, tbest, _ = metrics.best_rung_match(hcut, rungs, nc)
    assert "calibrate refined tree alone: threshold %r, acc = %s" % (tt, tbest) in out
    for j in range(5):
        assert "calibrate refined rung %d: threshold %r, acc = %s," % (j, float(rungs[j]),
                                                                      vals[j]) in out
    # untangle with the matching: the chosen rung's rows, one more line, one more file
    s1, t1, g1 = m.untangle(args, part="train", threshold=thr, refine=sweeps, merge=rounds,
                            split=True, match=True)
    out = capsys.readouterr().out
    np.testing.assert_array_equal(t1, table[k])
    np.testing.assert_array_equal(np.load(d / ("match_counts%d.npy" % ne)), hmt[k])
    sm = metrics.scores_from_match(hmt[k], nc)
    assert s1["match"] == sm
    assert ("untangle match: accuracy %s (per-commit mean %s), purity %s, cover %s"
            % (sm["accuracy"], sm["accuracy_mean"], sm["purity"], sm["cover"])) in out
    # without match everything is what it was: no line, no key, the file untouched
    os.remove(d / ("match_counts%d.npy" % ne))
    s0, t0, g0 = m.untangle(args, part="train", threshold=thr, refine=sweeps, merge=rounds,
                            split=True)
    assert "untangle match:" not in capsys.readouterr().out and "match" not in s0
    assert not (d / ("match_counts%d.npy" % ne)).exists()
    np.testing.assert_array_equal(t0, t1)
    np.testing.assert_array_equal(g0, g1)
    with pytest.raises(ValueError):
        m.calibrate(args, score="acc")
