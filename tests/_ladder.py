"""What the tests of hdg_refine_ladder share (test_refine_ladder.py, test_refine_ladder_gpu.py):
the motivating family, the ladders, and a set of poisoned buffers with the call that fills
them.  Generators and the other entry points' runs are _decode.py's and test_refine.py's.

Nothing here touches the GPU at import; the runs load the library when they are called.
"""
import ctypes

import numpy as np
import torch

from _decode import POISON_WS, T, _call_args
from hdgnn import _lib, metrics
from test_refine import noisy_planted

DEFAULT_LADDER = (0.05, 0.95, 19)
# T = 1; T = 2 with equal rungs; T = 5, unsorted, with bounds below every weight and above
LADDERS = ([0.5], [0.4, 0.4], [0.7, -1.5, 0.5, 3.0, 0.3])


def motivating_family():
    """The family on which refining at the tree's best threshold loses and the right rung
    recovers every planted group -> (labels (6, R), scores (6, R))."""
    return noisy_planted(40, seed=7, B=6)


def tprime(thr, rule):
    thr = np.float32(thr)
    return thr + thr if rule == "mean" else thr


class LadderBufs:
    """Poisoned outputs and workspace: the call writes every slot of every rung itself."""

    def __init__(self, rungs, nb, nc, dev):
        shape = _lib.Shape(nb, 20, nc, 2, nb, 0)
        lib = _lib.load()
        nbytes = lib.hdg_refine_ladder_workspace_bytes(ctypes.byref(shape), 0)
        assert nbytes == lib.hdg_refine_workspace_bytes(ctypes.byref(shape), 0)   # no factor T
        t = -(-nc // T)
        assert nbytes % 8 == 0 and nbytes >= nb * (nc * nc + t * (t + 1) // 2) * 4
        self.groups = torch.full((rungs, nb, nc), -7, dtype=torch.int32, device=dev)
        self.ut = torch.full((rungs, nb, _lib.RF_SLOTS), -1, dtype=torch.int64, device=dev)
        self.rq = torch.full((rungs, nb, _lib.RF_Q_SLOTS), -99, dtype=torch.int64, device=dev)
        self.ws = torch.full((nbytes // 8,), POISON_WS, dtype=torch.int64, device=dev)

    def poisoned(self):
        return bool((self.groups == -7).all() and (self.ut == -1).all() and (self.rq == -99).all()
                    and (self.ws == POISON_WS).all())

    def any_poison(self):
        return bool((self.groups == -7).any() or (self.ut == -1).any() or (self.rq == -99).any())


def ladder_run(y, p1, thresholds, tree=None, rule="mean", max_sweeps=8, bufs=None, groups=True):
    """hdg_refine_ladder on relation labels y (b, R), scores p1 (b, R), the thresholds and
    tree = (merges, levels) numpy arrays or None -> (bufs, groups, ut, rq) read back."""
    lib = _lib.load()
    dev, nb, nc, shape, bt, probs, stream, _keep = _call_args(y, p1)
    n = len(thresholds)
    bufs = bufs or LadderBufs(n, nb, nc, dev)
    vp = ctypes.c_void_p
    tm = tl = None
    if tree is not None:
        tm = torch.from_numpy(np.ascontiguousarray(tree[0], np.int32)).to(dev)
        tl = torch.from_numpy(np.ascontiguousarray(tree[1], np.float32)).to(dev)
    _lib.check(lib.hdg_refine_ladder(ctypes.byref(shape), ctypes.byref(bt), probs,
                                     (ctypes.c_float * n)(*[float(t) for t in thresholds]), n,
                                     _lib.UT_RULES[rule], max_sweeps, 0,
                                     None if tm is None else vp(tm.data_ptr()),
                                     None if tl is None else vp(tl.data_ptr()),
                                     vp(bufs.groups.data_ptr()) if groups else None,
                                     vp(bufs.ut.data_ptr()), vp(bufs.rq.data_ptr()),
                                     vp(bufs.ws.data_ptr()), stream))
    torch.cuda.synchronize(dev)
    return bufs, bufs.groups.cpu().numpy(), bufs.ut.cpu().numpy(), bufs.rq.cpu().numpy()


def same(dev, host, what=""):
    """(groups, ut, rq) of the device against (ut, groups, rq) of the host, every rung."""
    g, ut, rq = dev
    hut, hg, hrq = host
    np.testing.assert_array_equal(rq, hrq, what)
    np.testing.assert_array_equal(ut, hut, what)
    np.testing.assert_array_equal(g, hg, what)
    assert g.dtype == np.int32


def loop(label, probs, thresholds, tree, rule, max_sweeps):
    """The explicit loop metrics.refine_ladder stands for: cut_groups then refine, per rung."""
    out = []
    for t in np.asarray(thresholds, np.float32):
        start = None if tree is None else metrics.cut_groups(tree[0], tree[1], tprime(t, rule))
        out.append(metrics.refine(label, probs, start, t, rule, max_sweeps))
    return tuple(np.stack([o[i] for o in out]) for i in range(3))
