"""hdg_eval on the GPU: every row compared for integer equality with the host
implementation (hdgnn.metrics.eval_counts) on the same arrays -- no tolerances.

Shapes are the smallest at which each piece of the kernel can break, derived from the
chunk size (written here for HDG_EVAL_CHUNK = 16384), B = 3 each:
    nc   2  Ncr     2  a chunk that is almost all padding
    nc  33  Ncr  1056  label rows cross one 32-bit word
    nc  65  Ncr  4160  two-word label rows, the j >= i skip on both sides of a word edge
    nc 128  Ncr 16256  one chunk, just not full
    nc 129  Ncr 16512  two chunks, the second with 128 relations
    nc 182  Ncr 32942  three chunks
"""
import ctypes
import math
import types

import numpy as np
import pytest
import torch

from hdgnn import _lib, data, layout, metrics
from hdgnn.synth import synth_commits

pytestmark = pytest.mark.gpu

B = 3
C = _lib.EVAL_CHUNK


def _nc_chunks(k):
    """Smallest nc whose nc (nc - 1) relations need k chunks."""
    nc = 2
    while nc * (nc - 1) <= (k - 1) * C:
        nc += 1
    return nc


NC_ONE = _nc_chunks(2) - 1           # 128: the largest single-chunk shape
NC_TWO = _nc_chunks(2)               # 129
NC_THREE = _nc_chunks(3)             # 182
SHAPES = [2, 33, 65, NC_ONE, NC_TWO, NC_THREE]


def test_shapes_are_the_chunk_edges():
    assert (NC_ONE * (NC_ONE - 1) <= C < NC_TWO * (NC_TWO - 1) <= 2 * C
            < NC_THREE * (NC_THREE - 1) <= 3 * C)
    if C == 16384:
        assert SHAPES == [2, 33, 65, 128, 129, 182]


def _labels(nc, seed):
    """(B, R) random relation labels (not symmetric: every bit of ybits is its own)."""
    rng = np.random.default_rng(seed)
    return (rng.random((B, nc * (nc - 1))) < 0.3).astype(np.uint8)


def _scores(kind, nc, seed):
    """-> (labels (B, R) u8, probs (B, 2, R) f32) of one score set."""
    rng = np.random.default_rng(1000 + seed)
    R = nc * (nc - 1)
    y = _labels(nc, seed)
    if kind == "uniform":
        p1 = rng.random((B, R), dtype=np.float32)
        return y, np.stack([1.0 - p1, p1], 1).astype(np.float32)
    if kind == "quantised":            # multiples of 1/8: ties between relations, p1 == p0
        p1 = (rng.integers(0, 9, (B, R)) / 8.0).astype(np.float32)      # ties, exact 0 and 1
        p1[:, 0], p1[:, -1] = 0.0, 1.0
        if R > 2:
            p1[:, 1] = 0.5
        return y, np.stack([1.0 - p1, p1], 1).astype(np.float32)
    if kind == "one_class":            # all positives, all negatives, mixed
        y[0], y[1] = 1, 0
        p1 = rng.random((B, R), dtype=np.float32)
        return y, np.stack([1.0 - p1, p1], 1).astype(np.float32)
    if kind == "nan":                  # 5 % of the relations with a NaN in channel 0 or 1
        p1 = (rng.integers(0, 65, (B, R)) / 64.0).astype(np.float32)
        probs = np.stack([1.0 - p1, p1], 1).astype(np.float32)
        hit = rng.random((B, R)) < 0.05
        hit[:, 0] = True
        ch = rng.integers(0, 2, (B, R))
        probs[:, 0][hit & (ch == 0)] = np.nan
        probs[:, 1][hit & (ch == 1)] = np.nan
        return y, probs
    raise ValueError(kind)


def _run(nc, y, probs, ev=None):
    """hdg_eval on relation labels y (B, R) and probs (B, 2, R) -> (device ev, host rows)."""
    lib = _lib.load()
    dev = torch.device("cuda")
    ybits = torch.from_numpy(data.pack_bits(data._grid(y, nc)).view(np.int32)).to(dev)
    pt = torch.from_numpy(np.ascontiguousarray(probs, np.float32)).to(dev)
    if ev is None:                     # poisoned: the call zeroes every slot itself
        ev = torch.full((B, _lib.EV_SLOTS), -1, dtype=torch.int64, device=dev)
    shape = _lib.Shape(B, 20, nc, 2, B, 0)
    bt = _lib.Batch(None, None, ybits.data_ptr(), None, None, None)
    stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    _lib.check(lib.hdg_eval(ctypes.byref(shape), ctypes.byref(bt), ctypes.c_void_p(pt.data_ptr()),
                            ctypes.c_void_p(ev.data_ptr()), stream))
    torch.cuda.synchronize(dev)
    return ev, ev.cpu().numpy()


def _host(y, probs):
    return metrics.eval_counts(np.stack([1 - y, y], 1), probs)


@pytest.mark.parametrize("nc", SHAPES)
@pytest.mark.parametrize("kind", ["uniform", "quantised", "one_class", "nan"])
def test_rows_equal_host_counts(kind, nc):
    y, probs = _scores(kind, nc, seed=nc)
    _, got = _run(nc, y, probs)
    want = _host(y, probs)
    print(kind, nc, got.tolist(), want.tolist())
    np.testing.assert_array_equal(got, want)
    R = nc * (nc - 1)
    five = [_lib.EV_TP, _lib.EV_FP, _lib.EV_FN, _lib.EV_TN, _lib.EV_NAN]
    assert (got[:, five].sum(1) == R).all()
    if kind == "one_class":
        assert got[0, _lib.EV_U2] == 0 and got[1, _lib.EV_U2] == 0
        assert got[0, _lib.EV_FP] + got[0, _lib.EV_TN] == 0
        assert got[1, _lib.EV_TP] + got[1, _lib.EV_FN] == 0
    if kind == "nan":
        assert (got[:, _lib.EV_NAN] > 0).all()
        # U2 is the host's over the relations without NaN
        for b in range(B):
            keep = ~np.isnan(probs[b]).any(0)
            sub = _host(y[b:b + 1, keep], probs[b:b + 1][:, :, keep])
            assert got[b, _lib.EV_U2] == sub[0, _lib.EV_U2]
    if kind == "quantised" and nc > 2:
        assert (probs[:, 0] == probs[:, 1]).any()


def test_negatives_and_positives_in_different_chunks():
    """A block's sorted negatives must meet the positives of the other chunks."""
    nc = NC_THREE
    R = nc * (nc - 1)
    rng = np.random.default_rng(5)
    p1 = (rng.integers(0, 257, (B, R)) / 256.0).astype(np.float32)
    probs = np.stack([1.0 - p1, p1], 1).astype(np.float32)
    chunk = np.arange(R) // C
    y = np.zeros((B, R), np.uint8)
    y[0, chunk == 0] = 1               # positives in chunk 0 only, negatives in chunk 1 only,
    probs[0][:, chunk == 2] = np.nan   # the third chunk's relations out of play
    y[1, chunk != 1] = 1               # negatives in the middle chunk, positives around it
    y[2, chunk != 2] = 1               # negatives in the short last chunk only
    _, got = _run(nc, y, probs)
    want = _host(y, probs)
    print(got.tolist(), want.tolist())
    np.testing.assert_array_equal(got, want)
    assert (got[:, _lib.EV_U2] > 0).all()
    assert got[0, _lib.EV_NAN] == R - 2 * C


def test_repeat_launch_gives_identical_rows():
    """ev is zeroed per call (the second launch reuses the filled buffer) and the integer
    sums do not depend on the order the blocks ran in."""
    y, probs = _scores("quantised", NC_TWO, seed=77)
    ev, first = _run(NC_TWO, y, probs)
    _, second = _run(NC_TWO, y, probs, ev=ev)
    np.testing.assert_array_equal(first, second)
    np.testing.assert_array_equal(first, _host(y, probs))


def test_engine_forward_then_evaluate():
    from hdgnn.engine import Engine
    ne, nc, b = 20, 10, 4
    cb = synth_commits(b, ne, nc, 21)
    eng = Engine(ne, nc, b, variant=2)
    eng.set_params(layout.init_flat(5, 2))
    db = eng.upload(cb)
    label = data.onehot_relations(cb.y)
    probs, _, _ = eng.forward(db)
    ev = eng.evaluate(db)
    assert ev.dtype == torch.int64 and tuple(ev.shape) == (b, _lib.EV_SLOTS) and ev.is_cuda
    np.testing.assert_array_equal(ev.cpu().numpy(), metrics.eval_counts(label, probs.cpu().numpy()))
    # an explicit array of the same shape: synthetic scores
    fake = torch.rand_like(probs)
    np.testing.assert_array_equal(eng.evaluate(db, fake).cpu().numpy(),
                                  metrics.eval_counts(label, fake.cpu().numpy()))
    with pytest.raises(ValueError):
        eng.evaluate(db, fake[:, :, :-1])
    # the training launch's own count (gradient trailer) is TP + TN of its probabilities
    eng.fwd_bwd(db)
    ev = eng.evaluate(db).cpu().numpy()
    assert ev[:, _lib.EV_NAN].sum() == 0
    assert int(ev[:, _lib.EV_TP].sum() + ev[:, _lib.EV_TN].sum()) == eng.correct_count()
    eng.check_status()


def test_graph2graph_evaluate_scores_the_trained_checkpoint(golden_dir, tmp_path, monkeypatch,
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
    trained = m.engine.get_params()
    assert not np.array_equal(trained, layout.init_flat(7, 2))
    capsys.readouterr()

    m2 = model(99)                                  # another initialiser: the load must win
    scores, table = m2.evaluate(args)
    out = capsys.readouterr().out
    assert " [*] Load SUCCESS" in out and "Load failed" not in out
    assert "eval acc:" in out and "eval auc:" in out and "topol_acc" not in out
    np.testing.assert_array_equal(m2.engine.get_params(), trained)
    assert table.shape == (50, _lib.EV_SLOTS) and table.dtype == np.int64
    saved = np.load(tmp_path / "outputSelf" / "tiny" / "model_2" / "2" / ("eval_counts%d.npy" % ne))
    np.testing.assert_array_equal(saved, table)
    five = [_lib.EV_TP, _lib.EV_FP, _lib.EV_FN, _lib.EV_TN, _lib.EV_NAN]
    assert (table[:, five].sum(1) == nc * (nc - 1)).all()
    assert math.isfinite(scores["acc"]) and 0.0 <= scores["acc"] <= 1.0
    np.testing.assert_equal(scores, metrics.scores_from_counts(table))
    # the rows are those of the probabilities a forward of the same batches returns
    _, test, maps = data.compact_from_read_data(tup, ne, nc, mb)
    dbs = m2._device_batches(test, maps)
    want = [metrics.eval_counts(data.onehot_relations(test.y[j * mb:(j + 1) * mb]),
                                m2.engine.forward(db)[0].cpu().numpy())
            for j, db in enumerate(dbs)]
    np.testing.assert_array_equal(table, np.concatenate(want))
    # the train part: other commits, another table
    _, ttable = m2.evaluate(args, part="train")
    assert ttable.shape == (50, _lib.EV_SLOTS)


def test_evaluate_is_graph_capturable():
    """The memset node and the kernel replay from a captured graph on new scores."""
    from hdgnn.engine import Engine
    ne, nc, b = 20, 10, 4
    cb = synth_commits(b, ne, nc, 22)
    eng = Engine(ne, nc, b, variant=2)
    db = eng.upload(cb)
    label = data.onehot_relations(cb.y)
    scores = torch.rand(b, 2, nc * (nc - 1), device=eng.device)
    eng.evaluate(db, scores)                        # warm: module loaded before the capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        ev = eng.evaluate(db, scores)
    for _ in range(2):
        scores.copy_(torch.rand_like(scores))
        g.replay()
        torch.cuda.synchronize()
        np.testing.assert_array_equal(ev.cpu().numpy(),
                                      metrics.eval_counts(label, scores.cpu().numpy()))
