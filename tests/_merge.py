"""What the tests of hdg_refine_merge and hdg_refine_merge_ladder share (test_refine_merge.py,
test_refine_merge_gpu.py): the two families that motivate the calls, and poisoned buffers with
the calls that fill them.  Generators and the other entry points' runs are _decode.py's,
_ladder.py's and test_refine.py's.

Nothing here touches the GPU at import; the runs load the library when they are called.
"""
import ctypes

import numpy as np
import torch

from _decode import POISON_WS, T, _call_args
from hdgnn import _lib, data


def two_halves(nc=24, B=4, seed=5):
    """Three planted groups of nc / 3 hunks, each made of two halves: scores 0.85 + 0.1 u
    within a half, 0.55 + 0.05 u between the halves of a group, 0.2 u elsewhere (u uniform on
    [0, 1)).  At 0.5 every half is tight and the two halves of a group attract each other as
    wholes, while no single hunk gains by crossing.
    -> (labels (B, R) uint8, scores (B, R) float32, the halves (B, nc), the groups (B, nc))."""
    assert nc % 6 == 0
    rng = np.random.default_rng(seed)
    I, J = data.pair_index(nc)
    half = np.arange(nc) // (nc // 6)
    group = half // 2
    u = rng.random((B, len(I)))
    p1 = np.where(half[I] == half[J], 0.85 + 0.1 * u,
                  np.where(group[I] == group[J], 0.55 + 0.05 * u, 0.2 * u)).astype(np.float32)
    y = np.broadcast_to(group[I] == group[J], p1.shape).astype(np.uint8)
    return (y, p1, np.broadcast_to(half, (B, nc)).astype(np.int32),
            np.broadcast_to(group, (B, nc)).astype(np.int32))


BIG_NC, BIG_MERGE_GAIN, BIG_Q_END = 132, 2169610344, 4418805864


def big_sums():
    """One commit, nc = 132, the even hunks against the odd ones: scores 5.0 inside (the gain
    clamps at 2^19) and 1.45 across (gain 498074 under mean at 0.5).  A hunk keeps
    65 * 2^19 where it is against 66 * 498074 across, so no node moves; the merge of the two
    groups gains 66 * 66 * 498074 = 2 169 610 344, above 2^31.
    -> (labels (1, R), scores (1, R), the even / odd start (1, nc))."""
    nc = BIG_NC
    I, J = data.pair_index(nc)
    same = (I % 2) == (J % 2)
    p1 = np.where(same, 5.0, 1.45).astype(np.float32)[None]
    return same.astype(np.uint8)[None], p1, (np.arange(nc) % 2).astype(np.int32)[None]


class MergeBufs:
    """Poisoned outputs and workspace of hdg_refine_merge (rungs None) or of
    hdg_refine_merge_ladder: the call writes every slot itself."""

    def __init__(self, nb, nc, dev, rungs=None):
        shape = _lib.Shape(nb, 20, nc, 2, nb, 0)
        lib = _lib.load()
        size = (lib.hdg_refine_workspace_bytes if rungs is None
                else lib.hdg_refine_ladder_workspace_bytes)
        nbytes = size(ctypes.byref(shape), 0)
        t = -(-nc // T)
        assert nbytes % 8 == 0 and nbytes >= nb * (nc * nc + t * (t + 1) // 2) * 4
        lead = () if rungs is None else (rungs,)
        self.groups = torch.full(lead + (nb, nc), -7, dtype=torch.int32, device=dev)
        self.ut = torch.full(lead + (nb, _lib.RF_SLOTS), -1, dtype=torch.int64, device=dev)
        self.rq = torch.full(lead + (nb, _lib.RM_Q_SLOTS), -99, dtype=torch.int64, device=dev)
        self.ws = torch.full((nbytes // 8,), POISON_WS, dtype=torch.int64, device=dev)

    def poisoned(self):
        return bool((self.groups == -7).all() and (self.ut == -1).all() and (self.rq == -99).all()
                    and (self.ws == POISON_WS).all())

    def any_poison(self):
        return bool((self.groups == -7).any() or (self.ut == -1).any() or (self.rq == -99).any())

    def read(self):
        return self.groups.cpu().numpy(), self.ut.cpu().numpy(), self.rq.cpu().numpy()


def merge_run(y, p1, start=None, thr=0.5, rule="mean", max_sweeps=8, max_rounds=4, bufs=None,
              alias=False):
    """hdg_refine_merge on relation labels y (b, R), scores p1 (b, R) and starting ids (b, nc)
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
    _lib.check(lib.hdg_refine_merge(ctypes.byref(shape), ctypes.byref(bt), probs,
                                    ctypes.c_float(thr), _lib.UT_RULES[rule], max_sweeps,
                                    max_rounds, 0, None if gin is None else vp(gin.data_ptr()),
                                    vp(bufs.groups.data_ptr()), vp(bufs.ut.data_ptr()),
                                    vp(bufs.rq.data_ptr()), vp(bufs.ws.data_ptr()), stream))
    torch.cuda.synchronize(dev)
    return (bufs,) + bufs.read()


def merge_ladder_run(y, p1, thresholds, tree=None, rule="mean", max_sweeps=8, max_rounds=4,
                     bufs=None, groups=True):
    """hdg_refine_merge_ladder on relation labels y (b, R), scores p1 (b, R), the thresholds
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
    _lib.check(lib.hdg_refine_merge_ladder(
        ctypes.byref(shape), ctypes.byref(bt), probs,
        (ctypes.c_float * n)(*[float(t) for t in thresholds]), n, _lib.UT_RULES[rule], max_sweeps,
        max_rounds, 0, None if tm is None else vp(tm.data_ptr()),
        None if tl is None else vp(tl.data_ptr()), vp(bufs.groups.data_ptr()) if groups else None,
        vp(bufs.ut.data_ptr()), vp(bufs.rq.data_ptr()), vp(bufs.ws.data_ptr()), stream))
    torch.cuda.synchronize(dev)
    return (bufs,) + bufs.read()
