"""hdg_refine on the GPU: groups, ut and rq compared with the host restatement
(hdgnn.metrics.refine: one np.bincount per visit, no shared algorithm) for integer equality.
No tolerances.

Shapes: nc 2 and 3, 33, the tile edges 64 / 65, 74 (the glide shape), 129 (three tile rows),
B = 3 and all three rules; 1025, the first nc at which a thread owns two hunks, B = 1, rule
"mean", two sweeps.  The matrix of gains has one home (the workspace), so there is no second
path to compare.  Starts: NULL, all zeros, hdg_untangle's groups at 0.5, arbitrary ids with
-7 and nc + 5 among them.  max_sweeps 1, 2, 8 and 64.
"""
import ctypes
import math
import os
import types

import numpy as np
import pytest
import torch

from _decode import (B, T, _agglomerate_run, _cut, _onehot, _pairs, _planted, _probs, _uniform,
                     _with_nans)
from _decode import _RefineBufs as _Bufs
from _decode import _refine_run as _run
from conftest import ROOT
from hdgnn import _lib, data, layout, metrics
from hdgnn.synth import synth_commits
from test_refine import noisy_planted, wrong_first_merge

pytestmark = pytest.mark.gpu

RULES = ("mean", "any", "both")
SHAPES = [2, 3, 33, T, T + 1, 74, 2 * T + 1]
TWO_PER_THREAD = 1025
SWEEPS = (1, 2, 8, 64)


def test_shapes_follow_from_the_header_constants():
    if T == 64:
        assert SHAPES == [2, 3, 33, 64, 65, 74, 129]
    assert TWO_PER_THREAD == 1024 + 1 and _lib.RF_MAX_SWEEPS == max(SWEEPS)


# ---------------------------------------------------------------------------------------
# running the library and the host
# ---------------------------------------------------------------------------------------
def _same(dev, host, what=""):
    """(groups, ut, rq) of the device against (ut, groups, rq) of the host."""
    g, ut, rq = dev
    hut, hg, hrq = host
    np.testing.assert_array_equal(rq, hrq, what)
    np.testing.assert_array_equal(ut, hut, what)
    np.testing.assert_array_equal(g, hg, what)
    assert g.dtype == np.int32


def _starts(y, p1, rule, nc, seed):
    """name -> starting ids (b, nc) or None."""
    rng = np.random.default_rng(seed)
    nb = len(p1)
    wild = rng.integers(0, max(2, nc // 5), (nb, nc))
    wild[:, 0] = -7
    wild[:, nc - 1] = nc + 5
    if nc > 4:
        wild[:, nc // 2] = nc - 1                           # the largest id in range
        wild[-1, 1] = -(2 ** 31)
        wild[0, 2] = 2 ** 31 - 1
    return {"null": None, "zeros": np.zeros((nb, nc), np.int32),
            "untangle": metrics.untangle_counts(_onehot(y), _probs(p1), 0.5, rule)[1],
            "wild": wild}


def _check(what, y, p1, rules=RULES, thr=0.5):
    """Every rule and start, max_sweeps cycling through SWEEPS -> the host's rq rows."""
    nc = int(round((1 + math.sqrt(1 + 4 * p1.shape[1])) / 2))
    label, probs = _onehot(y), _probs(p1)
    k, rows = 0, []
    for rule in rules:
        for name, start in _starts(y, p1, rule, nc, nc).items():
            ms = SWEEPS[k % len(SWEEPS)]
            k += 5                                          # every (start, max_sweeps) pair
            host = metrics.refine(label, probs, start, thr, rule, ms)
            bufs, *dev = _run(y, p1, start, thr, rule, ms)
            print(what, rule, name, ms, "device ut", dev[1].tolist(), "rq", dev[2].tolist())
            _same(dev, host, "%s %s %s %d" % (what, rule, name, ms))
            assert not bool((bufs.groups == -7).any() or (bufs.ut == -1).any()
                            or (bufs.rq == -99).any())
            rows.append(host[2])
    return np.concatenate(rows)


# ---------------------------------------------------------------------------------------
# device == host
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("nc", SHAPES)
def test_noisy_planted_scores(nc):
    y, p1 = noisy_planted(nc, seed=nc, B=B)
    _check("noisy %d" % nc, y, p1)


@pytest.mark.parametrize("nc", SHAPES)
def test_uniform_scores(nc):
    y, p1 = _uniform(nc, seed=nc)
    rq = _check("uniform %d" % nc, y, p1)
    if nc == 2 * T + 1:                                     # the cap did cut some runs short
        assert (rq[:, _lib.RF_Q_CONVERGED] == 0).any() and (rq[:, _lib.RF_Q_CONVERGED] == 1).any()


@pytest.mark.parametrize("nc", SHAPES)
def test_scores_on_the_grid(nc):
    y, p1 = _planted(nc, seed=nc)                            # the 1/256 grid: many exact ties
    _check("planted %d" % nc, y, p1)
    rng = np.random.default_rng(nc)                          # ... and pairs exactly at the bound
    p2 = (rng.integers(96, 161, p1.shape) / 256.0).astype(np.float32)
    _check("grid %d" % nc, y, p2)


@pytest.mark.parametrize("nc", SHAPES)
def test_nan_in_one_direction_and_an_isolated_hunk(nc):
    y, p1, nans = _with_nans(nc, B)
    _check("nan %d" % nc, y, p1)
    ut = metrics.refine(_onehot(y), _probs(p1), None, 0.5, "mean", 1)[0]
    np.testing.assert_array_equal(ut[:, _lib.RF_NAN], nans)


@pytest.mark.parametrize("nc", [3, 33, T + 1, 2 * T + 1])
def test_infinite_scores(nc):
    y, p1 = noisy_planted(nc, seed=50 + nc, B=B)
    rng = np.random.default_rng(50 + nc)
    p1 = p1.copy()
    r = rng.random(p1.shape)
    p1[r < 0.04] = np.inf
    p1[(r >= 0.04) & (r < 0.08)] = -np.inf
    I, J = _pairs(nc)
    p1[:, (I == 0) & (J == 1)] = np.inf                      # inf and -inf: no edge under mean
    p1[:, (I == 1) & (J == 0)] = -np.inf
    _check("inf %d" % nc, y, p1)
    mean = metrics.refine(_onehot(y), _probs(p1), None, 0.5, "mean", 1)[0]
    both = metrics.refine(_onehot(y), _probs(p1), None, 0.5, "both", 1)[0]
    assert (mean[:, _lib.RF_NAN] >= 1).all() and (both[:, _lib.RF_NAN] == 0).all()


@pytest.mark.parametrize("thr", [0.0, 0.3, 0.9, -1.5, 3.0])
def test_other_thresholds(thr):
    nc = 74
    y, p1 = noisy_planted(nc, seed=int(thr * 10) + 20, B=B)
    _check("thr %s" % thr, y, p1, thr=thr)


def test_two_hunks_per_thread():
    nc = TWO_PER_THREAD
    y, p1 = noisy_planted(nc, seed=nc, B=1, k=12)
    label, probs = _onehot(y), _probs(p1)
    start = _starts(y, p1, "mean", nc, nc)["wild"]
    host = metrics.refine(label, probs, start, 0.5, "mean", 2)
    _, *dev = _run(y, p1, start, 0.5, "mean", 2)
    print("device ut", dev[1].tolist(), "rq", dev[2].tolist())
    _same(dev, host)
    assert host[0][0, _lib.RF_MOVES] > 0 and host[2][0, _lib.RF_Q_START] != 0


def test_max_sweeps_and_the_converged_flag():
    """Uniform scores at nc = 129 under mean take several sweeps: the cap cuts them short."""
    nc = 2 * T + 1
    y, p1 = _uniform(nc, seed=nc)
    label, probs = _onehot(y), _probs(p1)
    flags = {}
    for ms in SWEEPS:
        host = metrics.refine(label, probs, None, 0.5, "mean", ms)
        _, *dev = _run(y, p1, None, 0.5, "mean", ms)
        print(ms, "rq", dev[2].tolist())
        _same(dev, host, str(ms))
        flags[ms] = host[2][:, _lib.RF_Q_CONVERGED]
        assert (host[2][:, _lib.RF_Q_SWEEPS] <= ms).all()
    assert (flags[1] == 0).all() and (flags[2] == 0).all()      # the host's flags, not a guess
    assert (flags[64] == 1).all()


# ---------------------------------------------------------------------------------------
# calls
# ---------------------------------------------------------------------------------------
def test_groups_may_be_groups_in():
    for nc in (33, 74, 2 * T + 1):
        y, p1 = noisy_planted(nc, seed=80 + nc, B=B)
        for name, start in _starts(y, p1, "any", nc, 3).items():
            if start is None:
                continue
            host = metrics.refine(_onehot(y), _probs(p1), start, 0.5, "any", 8)
            _, *dev = _run(y, p1, start, 0.5, "any", 8, alias=True)
            _same(dev, host, "%d %s" % (nc, name))


def test_repeat_launch_other_inputs_same_buffers():
    nc = 74
    y, p1 = noisy_planted(nc, seed=901, B=B)
    start = _starts(y, p1, "mean", nc, 9)["untangle"]
    host = metrics.refine(_onehot(y), _probs(p1), start)
    bufs, *first = _run(y, p1, start)
    _same(first, host)
    _, *again = _run(y, p1, start, bufs=bufs)                   # into the used buffers
    for x, z in zip(first, again):
        np.testing.assert_array_equal(x, z)
    y3, p3 = _uniform(nc, seed=902)                             # other inputs, same buffers
    p3[0, :nc - 1] = np.nan
    _, *other = _run(y3, p3, None, 0.4, "both", 2, bufs=bufs)
    _same(other, metrics.refine(_onehot(y3), _probs(p3), None, 0.4, "both", 2))


def test_argument_errors_launch_nothing():
    lib = _lib.load()
    dev = torch.device("cuda")
    nc = 10
    bufs = _Bufs(B, nc, dev)
    ybits = torch.zeros(B, nc, 1, dtype=torch.int32, device=dev)
    pt = torch.rand(B, 2, nc * (nc - 1), device=dev)
    gin = torch.zeros(B, nc, dtype=torch.int32, device=dev)
    vp = ctypes.c_void_p
    base = dict(shape=_lib.Shape(B, 20, nc, 2, B, 0),
                bt=_lib.Batch(None, None, ybits.data_ptr(), None, None, None),
                probs=vp(pt.data_ptr()), thr=0.5, rule=0, ms=8, flags=0, gin=vp(gin.data_ptr()),
                groups=vp(bufs.groups.data_ptr()), ut=vp(bufs.ut.data_ptr()),
                rq=vp(bufs.rq.data_ptr()), ws=vp(bufs.ws.data_ptr()))

    def call(**kw):
        a = dict(base, **kw)
        stream = vp(torch.cuda.current_stream(dev).cuda_stream)
        return lib.hdg_refine(ctypes.byref(a["shape"]), ctypes.byref(a["bt"]), a["probs"],
                              ctypes.c_float(a["thr"]), a["rule"], a["ms"], a["flags"], a["gin"],
                              a["groups"], a["ut"], a["rq"], a["ws"], stream)

    bad = [dict(rule=3), dict(rule=-1), dict(ms=0), dict(ms=65), dict(ms=-1), dict(flags=1),
           dict(flags=2), dict(thr=float("nan")), dict(thr=float("inf")), dict(thr=float("-inf")),
           dict(thr=3e38), dict(thr=float("inf"), rule=1), dict(probs=None), dict(groups=None),
           dict(ut=None), dict(rq=None), dict(ws=None), dict(ws=vp(bufs.ws.data_ptr() + 4)),
           dict(bt=_lib.Batch(None, None, None, None, None, None)),
           dict(shape=_lib.Shape(0, 20, nc, 2, B, 0)), dict(shape=_lib.Shape(65536, 20, nc, 2, B, 0)),
           dict(shape=_lib.Shape(B, 20, 1, 2, B, 0)), dict(shape=_lib.Shape(B, 20, 2049, 2, B, 0))]
    for kw in bad:
        assert call(**kw) == 1000, kw
        assert lib.hdg_last_error().startswith(b"hdg_refine:"), kw
    torch.cuda.synchronize(dev)
    assert bufs.poisoned()
    assert call() == 0 and call(gin=None) == 0
    torch.cuda.synchronize(dev)
    assert (bufs.groups >= 0).all() and (bufs.ut >= 0).all() and (bufs.rq[:, 2] >= 1).all()


# ---------------------------------------------------------------------------------------
# the wrong-first-merge family, on the device from the tree to the refined groups
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", ("single", "complete", "average"))
def test_device_repairs_a_wrong_first_merge(method):
    y, p1, planted = wrong_first_merge()
    nc = planted.shape[1]
    for rule in RULES:
        _, (m, lv, cv, _, lk) = _agglomerate_run(y, p1, rule, method)
        _, best, _ = metrics.best_threshold(lv, cv.astype(np.int64), lk, rule, "f1")
        assert best < 1.0
        cut, row = _cut(nc, m, lv, cv, lk, 0.5, rule)
        assert not np.array_equal(cut, planted)
        _, g, ut, rq = _run(y, p1, cut, 0.5, rule, 4)
        print(rule, method, "cut", row.tolist(), "refined", ut.tolist(), "rq", rq.tolist())
        np.testing.assert_array_equal(g, planted)
        assert (ut[:, _lib.UT_SD] == 0).all() and (ut[:, _lib.UT_DS] == 0).all()
        assert (rq[:, _lib.RF_Q_CONVERGED] == 1).all() and (rq[:, 1] > rq[:, 0]).all()
        _same((g, ut, rq), metrics.refine(_onehot(y), _probs(p1), cut, 0.5, rule, 4))


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


def test_engine_forward_then_untangle_then_refine():
    eng, db, label, nc, b = _engine(31)
    probs, _, _ = eng.forward(db)
    g0, _ = eng.untangle(db)
    out = eng.refine(db, g0)
    groups, ut, rq = out
    assert all(x.is_cuda for x in out) and groups.data_ptr() != g0.data_ptr()
    assert groups.dtype == torch.int32 and tuple(groups.shape) == (b, nc)
    assert ut.dtype == torch.int64 and tuple(ut.shape) == (b, _lib.RF_SLOTS)
    assert rq.dtype == torch.int64 and tuple(rq.shape) == (b, _lib.RF_Q_SLOTS)
    _same(_np(out), metrics.refine(label, probs.cpu().numpy(), g0.cpu().numpy()))
    ws = eng._rf_workspace
    fake = torch.rand_like(probs)
    for rule in RULES:
        for ms in (1, 8):
            g1, _ = eng.untangle(db, fake, threshold=0.6, rule=rule)
            for start in (None, g1):
                out = eng.refine(db, start, fake, threshold=0.6, rule=rule, max_sweeps=ms)
                host = metrics.refine(label, fake.cpu().numpy(),
                                      None if start is None else start.cpu().numpy(), 0.6, rule, ms)
                _same(_np(out), host)
    assert eng._rf_workspace is ws                               # allocated once
    for kw in (dict(probs=fake[:, :, :-1]), dict(rule="most"), dict(max_sweeps=0),
               dict(max_sweeps=65), dict(max_sweeps=2.0), dict(groups=g0.long()),
               dict(groups=g0[:, :-1]), dict(groups=g0.cpu())):
        with pytest.raises(ValueError):
            eng.refine(db, **kw)
    with pytest.raises(RuntimeError):
        eng.refine(db, threshold=float("nan"))
    eng.check_status()


def test_refine_is_graph_capturable():
    """Both launches replay from a captured graph on new scores, with the eager bits."""
    eng, db, label, nc, b = _engine(32)
    scores = torch.rand(b, 2, nc * (nc - 1), device=eng.device)
    g0, _ = eng.untangle(db, scores, rule="any")    # warm: module loaded, workspaces allocated
    eng.refine(db, g0, scores, rule="any")
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        g0, _ = eng.untangle(db, scores, threshold=0.7, rule="any")
        out = eng.refine(db, g0, scores, threshold=0.7, rule="any", max_sweeps=8)
    for _ in range(2):
        scores.copy_(torch.rand_like(scores))
        graph.replay()
        torch.cuda.synchronize()
        replayed = _np(out)
        eager = _np(eng.refine(db, eng.untangle(db, scores, threshold=0.7, rule="any")[0], scores,
                               threshold=0.7, rule="any", max_sweeps=8))
        for x, z in zip(replayed, eager):
            np.testing.assert_array_equal(x, z)
        _same(replayed, metrics.refine(label, scores.cpu().numpy(), g0.cpu().numpy(), 0.7,
                                       "any", 8))


def test_graph2graph_untangle_with_refinement(golden_dir, tmp_path, monkeypatch, capsys):
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
    thr = 0.5
    # without refinement: what it always printed and wrote
    s0, t0, g0 = m2.untangle(args, part="train", threshold=thr, method="average")
    out = capsys.readouterr().out
    assert " [*] Load SUCCESS" in out and "refine" not in out
    assert not (d / ("untangle_refine%d.npy" % ne)).exists()
    scores, table, groups = m2.untangle(args, part="train", threshold=thr, method="average",
                                        refine=8)
    out = capsys.readouterr().out
    for line in ("untangle method: average", "untangle refine: 8 sweeps at most, ",
                 "untangle refine objective: "):
        assert line in out, line
    n = len(table)
    assert n > 0 and n % mb == 0
    saved = np.load(d / ("untangle_refine%d.npy" % ne))
    # the host, from the probabilities a forward of the same batches returns
    train, _, maps = data.compact_from_read_data(tup, ne, nc, mb)
    want = []
    for j, db in enumerate(m2._device_batches(train, maps)):
        label = data.onehot_relations(train.y[j * mb:(j + 1) * mb])
        probs = m2.engine.forward(db)[0].cpu().numpy()
        tree = metrics.agglomerate(label, probs, "mean", "average")
        start = metrics.cut_groups(tree[0], tree[1], np.float32(thr) + np.float32(thr))
        np.testing.assert_array_equal(start, g0[j * mb:(j + 1) * mb])
        want.append(metrics.refine(label, probs, start, thr, "mean", 8))
    hut, hg, hrq = (np.concatenate([w[i] for w in want]) for i in range(3))
    _same((groups, table, saved), (hut, hg, hrq))
    np.testing.assert_array_equal(np.load(d / ("untangle_groups%d.npy" % ne)), groups)
    np.testing.assert_array_equal(np.load(d / ("untangle_counts%d.npy" % ne)), table)
    np.testing.assert_equal(scores, metrics.scores_from_untangle(hut))
    assert ("%d moves, %d of %d commits converged"
            % (hut[:, _lib.RF_MOVES].sum(), hrq[:, _lib.RF_Q_CONVERGED].sum(), n)) in out
    assert ("objective: %d -> %d" % (hrq[:, 0].sum(), hrq[:, 1].sum())) in out
    assert (hrq[:, 1] >= hrq[:, 0]).all()
    # the single-linkage path takes it too
    _, t1, g1 = m2.untangle(args, part="train", threshold=thr, refine=2)
    capsys.readouterr()
    assert np.load(d / ("untangle_refine%d.npy" % ne)).shape == (n, _lib.RF_Q_SLOTS)
    with pytest.raises(ValueError):
        m2.untangle(args, part="train", refine=-1)
    with pytest.raises(ValueError):
        m2.untangle(args, part="train", refine=65)


# ---------------------------------------------------------------------------------------
# main.py --link-refine (a recorder: it takes `method` and `refine`)
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


def _runs(cli, argv, tmp_path):
    _Recorder.log = []
    cli.main(argv + ["--checkpoint_dir", str(tmp_path)], model_cls=_Recorder)
    return _Recorder.log


def test_main_link_refine(tmp_path):
    import importlib.util
    spec = importlib.util.spec_from_file_location("hdg_main_rf",
                                                  os.path.join(ROOT, "hd-gnn_amd", "main.py"))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    assert _runs(cli, ["--Type", "untangle", "--link-refine", "8"], tmp_path) == \
        [("untangle", s, "test", 0.5, "mean", {"refine": 8}) for s in cli.STEPS]
    runs = _runs(cli, ["--Type", "untangle", "--link-threshold", "auto", "--link-method",
                       "average", "--link-refine", "3", "--link-rule", "any"], tmp_path)
    want = []
    for s in cli.STEPS:                             # calibrate is untouched; its threshold is used
        want += [("calibrate", s, "train", "any", "f1", {"method": "average"}),
                 ("untangle", s, "test", 0.125 * s, "any", {"method": "average", "refine": 3})]
    assert runs == want
    assert _runs(cli, ["--Type", "calibrate", "--link-refine", "8"], tmp_path) == \
        [("calibrate", s, "train", "mean", "f1", {}) for s in cli.STEPS]
    # 0, given or by default, passes nothing: the call as it always was
    for argv in (["--link-refine", "0"], []):
        assert _runs(cli, ["--Type", "untangle"] + argv, tmp_path) == \
            [("untangle", s, "test", 0.5, "mean", {}) for s in cli.STEPS]
    with pytest.raises(SystemExit):
        cli.main(["--Type", "untangle", "--link-refine", "many", "--checkpoint_dir", str(tmp_path)],
                 model_cls=_Recorder)
