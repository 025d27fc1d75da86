"""What the tests of hdg_match share (test_match.py, test_match_gpu.py): fixtures with planted
values, the noisy families, the certificate of `mate`, and the call on poisoned buffers.

A fixture is (labels y (b, R) uint8, predicted ids (b, nc) int32, planted slots or None): the
labels are those of the true groups, y_pq = [t_p == t_q].  The planted numbers were checked
with scipy.optimize.linear_sum_assignment where it is installed (test_match.py does it again
under importorskip); the ones that need no solver follow from the construction.

Nothing here touches the GPU at import; the run loads the library when it is called.
"""
import ctypes
import math

import numpy as np

from hdgnn import _lib, data, metrics

INT32_MIN, INT32_MAX = -2 ** 31, 2 ** 31 - 1
POISON_MT, POISON_ID, POISON_WS = -1, -7, 0x7F7F7F7F7F7F7F7F


def labels_of(tg):
    """True ids (b, nc) -> relation labels (b, R) uint8."""
    tg = np.atleast_2d(np.asarray(tg))
    I, J = data.pair_index(tg.shape[1])
    return (tg[:, I] == tg[:, J]).astype(np.uint8)


def canon(g):
    """Dense ids ordered by each group's smallest member."""
    _, first, inv = np.unique(np.asarray(g), return_index=True, return_inverse=True)
    return np.argsort(np.argsort(first))[inv].astype(np.int32)


def _fixture(pred, true, **slots):
    pred, true = np.asarray(pred, np.int32)[None], np.asarray(true, np.int32)[None]
    return labels_of(true), pred, {getattr(_lib, "MT_" + k.upper()): v for k, v in slots.items()}


def three_ways_wrong():
    """nc = 7, table [[3, 2], [2, 0]]: the optimum 4 takes the two 2s; largest-cell-first
    greedy gives 3, purity and cover both 5."""
    return _fixture([0, 0, 0, 0, 0, 1, 1], [0, 0, 0, 1, 1, 0, 0],
                    groups=2, tgroups=2, matched=4, purity=5, cover=5, cells=3, isolated=0)


def staircase(K, contender_first):
    """Two hunks per cell; rows i < K hold the cells (i, i) and (i, i+1), a last row (the
    contender) the single cell (K, 0).  nc = 2 (2K + 1); the optimum 2 (K + 1) moves every row
    i to column i + 1 and needs an augmenting path through all K rows, arg-max greedy gives
    2K when the contender comes last.  Ids are dense by smallest member: the contender's two
    hunks are placed first or last, so it is the lowest or the highest predicted group."""
    rows, cols = [], []
    for i in range(K):
        rows += [i, i, i, i]
        cols += [i, i, i + 1, i + 1]
    if contender_first:
        rows, cols = [K, K] + rows, [0, 0] + cols
    else:
        rows, cols = rows + [K, K], cols + [0, 0]
    assert len(rows) == 2 * (2 * K + 1)
    return _fixture(canon(rows), canon(cols), groups=K + 1, tgroups=K + 1, matched=2 * (K + 1),
                    purity=2 * (K + 1), cover=2 * (K + 1), cells=2 * K + 1, isolated=0)


def singletons_vs_one(nc=74):
    return _fixture(np.arange(nc), np.zeros(nc), groups=nc, tgroups=1, matched=1, purity=nc,
                    cover=1, cells=nc, isolated=0)


def one_vs_singletons(nc=74):
    return _fixture(np.zeros(nc), np.arange(nc), groups=1, tgroups=nc, matched=1, purity=1,
                    cover=nc, cells=nc, isolated=0)


def equal_partitions(nc=74, k=5, seed=3):
    t = canon(np.random.default_rng(seed).integers(0, k, nc))
    n = int(t.max()) + 1
    return _fixture(t, t, groups=n, tgroups=n, matched=nc, purity=nc, cover=nc, cells=n,
                    isolated=n)


def chain(nc):
    """Predicted pairs {2i, 2i+1} against true pairs {2i+1, 2i+2} (hunk 0 alone on the true
    side, the last hunk alone on one side or both): one path through every cell."""
    pred = np.arange(nc) // 2
    true = (np.arange(nc) + 1) // 2
    planted = {8: (4, 4, 5), 66: (33, 33, 34), 257: (129, 129, 129)}[nc]
    return _fixture(pred, true, groups=(nc + 1) // 2, tgroups=nc // 2 + 1, matched=planted[0],
                    purity=planted[1], cover=planted[2], cells=nc, isolated=0)


PLANTED = {
    "three_ways_wrong": three_ways_wrong,
    "staircase3_first": lambda: staircase(3, True), "staircase3_last": lambda: staircase(3, False),
    "staircase32_first": lambda: staircase(32, True),
    "staircase32_last": lambda: staircase(32, False),
    "staircase64_first": lambda: staircase(64, True),
    "staircase64_last": lambda: staircase(64, False),
    "singletons_vs_one": singletons_vs_one, "one_vs_singletons": one_vs_singletons,
    "equal": equal_partitions,
    "chain8": lambda: chain(8), "chain66": lambda: chain(66), "chain257": lambda: chain(257),
}


def relabeled_truth(tg, rng, moved=0.1):
    """A random renumbering of the true ids (non-dense, any order) with `moved` of the hunks
    put into another, random group."""
    tg = np.asarray(tg)
    nc = tg.shape[-1]
    out = np.empty_like(tg, dtype=np.int32)
    for idx in np.ndindex(tg.shape[:-1]):
        perm = rng.permutation(nc)
        g = perm[tg[idx]]
        hit = rng.random(nc) < moved
        g[hit] = perm[rng.integers(0, int(tg[idx].max()) + 1, int(hit.sum()))]
        out[idx] = g
    return out


def noisy_sets(y, p1, seed, n_sets=3):
    """`n_sets` sets of predicted ids for the family's commits (y, p1) -> (n_sets, b, nc) int32.
    1: untangle_counts' groups at 0.5; 3: those at 0.45 and 0.55 and a relabeling of the truth
    with 10 % of the hunks moved; more: relabelings alone, a different one in every set."""
    from test_refine import _onehot, _probs
    label, probs = _onehot(y), _probs(p1)
    rng = np.random.default_rng(seed)
    sets = []
    tg = metrics.untangle_counts(label, probs, 0.5, "mean")[2]
    for thr in {1: (0.5,), 3: (0.45, 0.55)}.get(n_sets, ()):
        sets.append(metrics.untangle_counts(label, probs, thr, "mean")[1])
    while len(sets) < n_sets:
        sets.append(relabeled_truth(tg, rng))
    return np.stack(sets).astype(np.int32)


def wild_ids(groups, rng, share=0.15):
    """`share` of the ids replaced by -1, nc, INT32_MIN and INT32_MAX: those hunks are alone."""
    g = np.array(groups, np.int64)
    nc = g.shape[-1]
    hit = rng.random(g.shape) < share
    g[hit] = rng.choice([-1, nc, INT32_MIN, INT32_MAX, nc + 5, -nc], int(hit.sum()))
    return g.astype(np.int32)


def renumbered(groups, rng):
    """The in-range ids permuted over [0, nc) (non-dense): the same partition."""
    g = np.array(groups, np.int64)
    nc = g.shape[-1]
    out = g.copy()
    for idx in np.ndindex(g.shape[:-1]):
        perm = rng.permutation(nc)
        ok = (g[idx] >= 0) & (g[idx] < nc)
        out[idx][ok] = perm[g[idx][ok]]
    return out.astype(np.int32)


def table_of(ids, tg):
    """Predicted ids (nc,) -- equal ids in [0, nc) together, any other id alone -- and dense true
    ids (nc,) -> the dense contingency table, straight from the definition (np.add.at)."""
    ids = np.asarray(ids, np.int64).copy()
    nc = len(ids)
    alone = (ids < 0) | (ids >= nc)
    ids[alone] = nc + np.flatnonzero(alone)
    g = np.unique(ids, return_inverse=True)[1]
    table = np.zeros((int(g.max()) + 1, int(np.max(tg)) + 1), np.int64)
    np.add.at(table, (g, np.asarray(tg, np.int64)), 1)
    return table


def check_consequences(mt, groups, tgroups):
    """The header's consequences on the rows mt ((S, b, 8)) of the ids groups ((S, b, nc)) and
    tgroups ((b, nc)), against the table built from the definition: the counts, PURITY, COVER,
    (A) max cell <= MATCHED <= min(PURITY, COVER) <= nc, (B) MATCHED == nc iff the table has one
    cell per row and per column, and then CELLS == ISOLATED == GROUPS == TGROUPS, (C) MATCHED >=
    the sum of the isolated cells; slot 7 is 0."""
    mt, groups = np.asarray(mt), np.asarray(groups)
    nc = groups.shape[-1]
    assert mt.shape == groups.shape[:2] + (_lib.MT_SLOTS,)
    for s, b in np.ndindex(groups.shape[:2]):
        table = table_of(groups[s, b], tgroups[b])
        on = table > 0
        iso = on & (on.sum(1, keepdims=True) == 1) & (on.sum(0, keepdims=True) == 1)
        row = mt[s, b]
        m = row[_lib.MT_MATCHED]
        assert row[_lib.MT_GROUPS] == table.shape[0] and row[_lib.MT_TGROUPS] == table.shape[1]
        assert row[_lib.MT_CELLS] == on.sum() and row[_lib.MT_ISOLATED] == iso.sum(), (s, b)
        assert row[_lib.MT_PURITY] == table.max(1).sum() and row[_lib.MT_COVER] == table.max(0).sum()
        assert table.max() <= m <= min(row[_lib.MT_PURITY], row[_lib.MT_COVER]) <= nc, (s, b)
        assert m >= table[iso].sum(), (s, b)
        assert (m == nc) == bool(iso.sum() == on.sum()), (s, b)
        if m == nc:
            assert (row[_lib.MT_CELLS] == row[_lib.MT_ISOLATED] == row[_lib.MT_GROUPS]
                    == row[_lib.MT_TGROUPS])
        assert row[7] == 0


def check_mate(mate, groups, tgroups, mt):
    """The certificate of `mate` ((S, b, nc)) against mt ((S, b, 8)) and tgroups ((b, nc)):
    constant on each predicted group, injective over the groups where it is not -1, and it
    matches exactly MATCHED hunks."""
    mate, groups = np.asarray(mate), np.asarray(groups)
    nc = groups.shape[-1]
    for s, b in np.ndindex(mate.shape[:2]):
        ids = groups[s, b].astype(np.int64)
        alone = (ids < 0) | (ids >= nc)
        ids[alone] = nc + np.flatnonzero(alone)              # a hunk alone is its own group
        m = mate[s, b]
        assert ((m >= -1) & (m <= tgroups[b].max())).all()
        image = {}
        for g in np.unique(ids):
            vals = np.unique(m[ids == g])
            assert len(vals) == 1, (s, b, g)
            if vals[0] >= 0:
                assert vals[0] not in image, (s, b, g)
                image[vals[0]] = g
        assert np.count_nonzero(m == tgroups[b]) == mt[s, b, _lib.MT_MATCHED], (s, b)


class MatchBufs:
    """Poisoned outputs and workspace of hdg_match: the call writes every slot itself."""

    def __init__(self, n_sets, nb, nc, dev):
        import torch
        shape = _lib.Shape(nb, 20, nc, 2, nb, 0)
        nbytes = _lib.load().hdg_match_workspace_bytes(ctypes.byref(shape), n_sets)
        assert nbytes % 8 == 0 and nbytes >= nb * nc * 4
        self.mt = torch.full((n_sets, nb, _lib.MT_SLOTS), POISON_MT, dtype=torch.int64, device=dev)
        self.mate = torch.full((n_sets, nb, nc), POISON_ID, dtype=torch.int32, device=dev)
        self.tgroups = torch.full((nb, nc), POISON_ID, dtype=torch.int32, device=dev)
        self.ws = torch.full((nbytes // 8,), POISON_WS, dtype=torch.int64, device=dev)

    def any_poison(self):
        return bool((self.mt == POISON_MT).any() or (self.mate == POISON_ID).any()
                    or (self.tgroups == POISON_ID).any())

    def read(self):
        return self.mt.cpu().numpy(), self.mate.cpu().numpy(), self.tgroups.cpu().numpy()


def match_run(y, groups, bufs=None, mate=True, tgroups=True):
    """hdg_match on relation labels y (b, R) and predicted ids (S, b, nc) or (b, nc) ->
    (bufs, mt, mate, tgroups) read back."""
    import torch
    lib = _lib.load()
    dev = torch.device("cuda")
    groups = np.asarray(groups, np.int32)
    if groups.ndim == 2:
        groups = groups[None]
    S, nb, nc = groups.shape
    assert y.shape == (nb, nc * (nc - 1))
    ybits = torch.from_numpy(data.pack_bits(data._grid(y, nc)).view(np.int32)).to(dev)
    shape = _lib.Shape(nb, 20, nc, 2, nb, 0)
    bt = _lib.Batch(None, None, ybits.data_ptr(), None, None, None)
    stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    gin = torch.from_numpy(np.ascontiguousarray(groups)).to(dev)
    bufs = bufs or MatchBufs(S, nb, nc, dev)
    vp = ctypes.c_void_p
    _lib.check(lib.hdg_match(ctypes.byref(shape), ctypes.byref(bt), vp(gin.data_ptr()), S,
                             vp(bufs.mate.data_ptr()) if mate else None,
                             vp(bufs.tgroups.data_ptr()) if tgroups else None,
                             vp(bufs.mt.data_ptr()), vp(bufs.ws.data_ptr()), stream))
    torch.cuda.synchronize(dev)
    return (bufs,) + bufs.read()


def nc_of(R):
    return int(round((1 + math.sqrt(1 + 4 * R)) / 2))
