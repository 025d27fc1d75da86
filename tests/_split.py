"""What the tests of hdg_refine_split and hdg_refine_split_ladder share (test_refine_split.py,
test_refine_split_gpu.py): the two families that motivate the calls, and the calls on poisoned
buffers.  The buffers are _merge.py's (the rq rows have the same 8 slots), the generators and
the other entry points' runs are _decode.py's, _ladder.py's, _merge.py's and test_refine.py's.

Nothing here touches the GPU at import; the runs load the library when they are called.
"""
import ctypes

import numpy as np
import torch

from _decode import _call_args
from _merge import MergeBufs
from hdgnn import _lib, data

KINDS = {"merge": 1, "split": 2, "both": 3}


def two_fused(nc=24, B=4, seed=5):
    """Three fused groups of nc / 3 hunks, each made of two halves that are the TRUE groups:
    scores 0.9 + 0.1 u within a half, 0.25 + 0.05 u between the halves of a group, 0.2 u
    elsewhere (u uniform on [0, 1)); the two directed scores between the first hunks of a
    group's two halves are 0.97, the wrong pair that chains single linkage.  At 0.5 every hunk
    keeps a positive sum towards its fused group, so no node moves and nothing merges, while
    the sum between the halves is far below 0.
    -> (labels (B, R) uint8, scores (B, R) float32, the halves (B, nc), the fused groups (B, nc))."""
    assert nc % 6 == 0 and nc >= 24
    rng = np.random.default_rng(seed)
    I, J = data.pair_index(nc)
    h = nc // 6
    half = np.arange(nc) // h
    group = half // 2
    u = rng.random((B, len(I)))
    p1 = np.where(half[I] == half[J], 0.9 + 0.1 * u,
                  np.where(group[I] == group[J], 0.25 + 0.05 * u, 0.2 * u)).astype(np.float32)
    wrong = (group[I] == group[J]) & (half[I] != half[J]) & (I % h == 0) & (J % h == 0)
    p1[:, wrong] = np.float32(0.97)
    y = np.broadcast_to(half[I] == half[J], p1.shape).astype(np.uint8)
    return (y, p1, np.broadcast_to(half, (B, nc)).astype(np.int32),
            np.broadcast_to(group, (B, nc)).astype(np.int32))


BIG_NC, BIG_SPLIT_GAIN, BIG_Q_START, BIG_Q_END = 132, 2169610344, 79585176, 2249195520


def big_split():
    """One commit, nc = 132, all in one group, the even hunks against the odd ones: scores 5.0
    inside a parity (the gain clamps at 2^19) and -0.45 across (gain -498074 under mean at
    0.5).  A hunk keeps 65 * 2^19 - 66 * 498074 > 0 where it is, so no node moves; the seeds
    are (0, 1) and the one split gains 66 * 66 * 498074 = 2 169 610 344, above 2^31.
    -> (labels (1, R), scores (1, R), the all-zeros start (1, nc))."""
    nc = BIG_NC
    I, J = data.pair_index(nc)
    same = (I % 2) == (J % 2)
    p1 = np.where(same, 5.0, -0.45).astype(np.float32)[None]
    return same.astype(np.uint8)[None], p1, np.zeros((1, nc), np.int32)


def split_run(y, p1, start=None, thr=0.5, rule="mean", max_sweeps=8, max_rounds=4, kinds=3,
              bufs=None, alias=False):
    """hdg_refine_split on relation labels y (b, R), scores p1 (b, R) and starting ids (b, nc)
    or None -> (bufs, groups, ut, rq) read back.  alias: groups_in is the output array."""
    lib = _lib.load()
    dev, nb, nc, shape, bt, probs, stream, _keep = _call_args(y, p1)
    bufs = bufs or MergeBufs(nb, nc, dev)
    gin = None
    if start is not None:
        gin = torch.from_numpy(np.ascontiguousarray(start, np.int32)).to(dev)
        if alias:
            bufs.groups.copy_(gin)
            gin = bufs.groups
    vp = ctypes.c_void_p
    _lib.check(lib.hdg_refine_split(ctypes.byref(shape), ctypes.byref(bt), probs,
                                    ctypes.c_float(thr), _lib.UT_RULES[rule], max_sweeps,
                                    max_rounds, kinds, 0,
                                    None if gin is None else vp(gin.data_ptr()),
                                    vp(bufs.groups.data_ptr()), vp(bufs.ut.data_ptr()),
                                    vp(bufs.rq.data_ptr()), vp(bufs.ws.data_ptr()), stream))
    torch.cuda.synchronize(dev)
    return (bufs,) + bufs.read()


def split_ladder_run(y, p1, thresholds, tree=None, rule="mean", max_sweeps=8, max_rounds=4,
                     kinds=3, bufs=None, groups=True):
    """hdg_refine_split_ladder on relation labels y (b, R), scores p1 (b, R), the thresholds
    and tree = (merges, levels) numpy arrays or None -> (bufs, groups, ut, rq) read back."""
    lib = _lib.load()
    dev, nb, nc, shape, bt, probs, stream, _keep = _call_args(y, p1)
    n = len(thresholds)
    bufs = bufs or MergeBufs(nb, nc, dev, rungs=n)
    vp = ctypes.c_void_p
    tm = tl = None
    if tree is not None:
        tm = torch.from_numpy(np.ascontiguousarray(tree[0], np.int32)).to(dev)
        tl = torch.from_numpy(np.ascontiguousarray(tree[1], np.float32)).to(dev)
    _lib.check(lib.hdg_refine_split_ladder(
        ctypes.byref(shape), ctypes.byref(bt), probs,
        (ctypes.c_float * n)(*[float(t) for t in thresholds]), n, _lib.UT_RULES[rule], max_sweeps,
        max_rounds, kinds, 0, None if tm is None else vp(tm.data_ptr()),
        None if tl is None else vp(tl.data_ptr()), vp(bufs.groups.data_ptr()) if groups else None,
        vp(bufs.ut.data_ptr()), vp(bufs.rq.data_ptr()), vp(bufs.ws.data_ptr()), stream))
    torch.cuda.synchronize(dev)
    return (bufs,) + bufs.read()
