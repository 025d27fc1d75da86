"""What the GPU tests of the four decoders of the pair scores share (test_untangle_gpu.py,
test_linkage_gpu.py, test_agglomerate_gpu.py, test_refine_gpu.py): the shapes derived from
the header constants, the score and label generators, and per entry point a set of poisoned
buffers with the call that fills them.

Shapes are the smallest at which each piece of the tiled kernels can break (written here for
HDG_UT_TILE = 64, 4 tile pairs per block), B = 3 each:
    nc   2   one pair
    nc  33   label rows cross one 32-bit word, a tile that is mostly padding
    nc  64   one full tile
    nc  65   a one-wide edge tile and its mirror
    nc  74   the glide shape: 3 tile pairs on one block
    nc 128   two full tile rows, still one block
    nc 129   6 tile pairs on two blocks
    nc 193   10 tile pairs on three blocks, dealt 4 / 3 / 3
and nc 705 at B = 1: 78 tile pairs on the 16 blocks the cap allows (4 or 5 per block).

Nothing here touches the GPU at import; the runs load the library when they are called.
"""
import ctypes
import math

import numpy as np
import torch

from hdgnn import _lib, data

B = 3
T, TPB, MAXB = _lib.UT_TILE, _lib.UT_TILES_PER_BLOCK, _lib.UT_MAX_BLOCKS
POISON_WS = 0x7F7F7F7F7F7F7F7F


def _tile_pairs(nc):
    t = -(-nc // T)
    return t * (t + 1) // 2


def _nc_blocks(k):
    """Smallest nc whose commit runs on k blocks."""
    nc = 2
    while _lib.untangle_blocks(nc) < k:
        nc += 1
    return nc


NC_TWO, NC_THREE, NC_CAPPED = _nc_blocks(2), _nc_blocks(3), 705
SHAPES = [2, 33, T, T + 1, 74, NC_TWO - 1, NC_TWO, NC_THREE]
BIG = [NC_TWO, NC_THREE]


# ---------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------
def _probs(p1):
    """(b, R) scores -> C-contiguous (b, 2, R) float32 (fancy-indexed inputs may be F-ordered)."""
    return np.ascontiguousarray(np.stack([1.0 - p1, p1], 1), np.float32)


def _onehot(y):
    return np.stack([1 - y, y], 1).astype(np.float32)


def _pairs(nc):
    return data.pair_index(nc)


def _sym(nc, rng, nb, prob):
    """(nb, R) bool: a random symmetric choice of unordered pairs, each with probability prob."""
    I, J = _pairs(nc)
    m = rng.random((nb, nc, nc)) < prob
    m = np.triu(m, 1)
    m = m | m.transpose(0, 2, 1)
    return m[:, I, J]


def _planted_labels(nc, rng, nb, k=3, pad=2):
    """Labels from k planted groups, each direction of a within-group pair set with
    probability 0.5 on its own (not symmetric); the last `pad` hunks are padding: no labels."""
    I, J = _pairs(nc)
    gt = rng.integers(0, k, (nb, nc))
    y = (gt[:, I] == gt[:, J]) & (rng.random((nb, len(I))) < 0.5)
    y &= (I < nc - pad) & (J < nc - pad)
    return y.astype(np.uint8)


def _planted(nc, seed, nb=B):
    """Planted predicted groups of about 12 hunks with sparse within-group links (a pair of
    the same group is linked with probability 0.25: both directions high), a handful of
    cross-group pairs high in ONE direction only, everything on a 1/256 grid; labels from
    three other planted groups."""
    rng = np.random.default_rng(seed)
    I, J = _pairs(nc)
    R = len(I)
    kp = max(2, nc // 12)
    gp = rng.integers(0, kp, (nb, nc))
    same = gp[:, I] == gp[:, J]
    on = same & _sym(nc, rng, nb, 0.25)
    lo = rng.integers(0, 96, (nb, R))
    hi = rng.integers(160, 257, (nb, R))
    # about 1.5 per group; high + low = 160 .. 351 of 256, so about a quarter of them link
    one_way = ~same & (rng.random((nb, R)) < 1.5 * kp / R)
    p1 = (np.where(on | one_way, hi, lo) / 256.0).astype(np.float32)
    pad = (I >= nc - 2) | (J >= nc - 2)
    p1[:, pad] = 0.0
    return _planted_labels(nc, rng, nb), p1


def _uniform(nc, seed, nb=B):
    rng = np.random.default_rng(100 + seed)
    return _planted_labels(nc, rng, nb), rng.random((nb, nc * (nc - 1)), dtype=np.float32)


def _with_nans(nc, nb):
    """NaN in one direction of about 5% of the pairs, and in commit 1 a hunk no edge reaches."""
    y, p1 = _planted(nc, seed=300 + nc, nb=nb)
    rng = np.random.default_rng(300 + nc)
    I, J = _pairs(nc)
    hit = _sym(nc, rng, nb, 0.05)
    hit[:, (I == 0) & (J == 1)] = hit[:, (I == 1) & (J == 0)] = True
    first = _sym(nc, rng, nb, 0.5) ^ (I < J)
    p1 = p1.copy()
    p1[hit & first] = np.nan
    if nc >= 33 and nb > 1:
        p1[1, I == 7] = np.nan
        hit[1, (I == 7) | (J == 7)] = True
    return y, p1, hit.sum(1) // 2


def _with_infs(y, p1, seed):
    """test_infinite_scores' scores from a family's (y, p1): 4 % of the scores +inf, 4 % -inf,
    and the pair (0, 1) = +inf, (1, 0) = -inf: no edge under mean, NaN in no direction."""
    nc = int(round((1 + math.sqrt(1 + 4 * p1.shape[1])) / 2))
    rng = np.random.default_rng(seed)
    p1 = p1.copy()
    r = rng.random(p1.shape)
    p1[r < 0.04] = np.inf
    p1[(r >= 0.04) & (r < 0.08)] = -np.inf
    I, J = _pairs(nc)
    p1[:, (I == 0) & (J == 1)] = np.inf                      # inf and -inf: no edge under mean
    p1[:, (I == 1) & (J == 0)] = -np.inf
    return y, p1


def _scores_of(nc, edges, directed=None):
    """(R,) scores: 0.75 on the listed pairs (both directions; directed='down': only from
    the higher hunk to the lower, 'up': only from the lower to the higher), 0.125 elsewhere."""
    S = np.full((nc, nc), 0.125, np.float32)
    e = np.asarray(edges, np.int64).reshape(-1, 2)
    lo, hi = e.min(1), e.max(1)
    if directed != "down":
        S[lo, hi] = 0.75
    if directed != "up":
        S[hi, lo] = 0.75
    I, J = _pairs(nc)
    return S[I, J]


def _owner(nc):
    """(nc, nc) block that owns the tile pair of the unordered pair {p, q}."""
    t = -(-nc // T)
    k_of = np.zeros((t, t), np.int64)
    k = 0
    for i in range(t):
        for j in range(i, t):
            k_of[i, j] = k_of[j, i] = k
            k += 1
    tile = np.arange(nc) // T
    return k_of[tile[:, None], tile[None, :]] % _lib.untangle_blocks(nc)


def _bridged_groups(nc):
    """Two groups whose links all lie in tile pairs of block 0 and whose only connecting link
    lies in a tile pair of another block -> (edges, members of A, members of B, bridge)."""
    own = _owner(nc)
    A = list(range(10))                                        # a clique in tile pair (0, 0)
    assert (own[:10, :10] == 0).all()
    for q in range(10, nc):                                    # B's end of the bridge
        if own[A[4], q] == 0:
            continue
        for h in range(nc - 1, 9, -1):                         # B is a star on h, q one of its rays
            if h == q or own[q, h] != 0:
                continue
            rest = [r for r in range(10, nc) if r not in (q, h) and own[h, r] == 0]
            if len(rest) >= 5:
                Bm = [q, h] + rest[::max(1, len(rest) // 5)][:5]    # spread over the tiles
                edges = [(a, b) for a in A for b in A if a < b] + [(h, r) for r in Bm if r != h]
                return edges, A, Bm, (A[4], q)
    raise AssertionError("no bridge at nc %d" % nc)


# ---------------------------------------------------------------------------------------
# running the library: the arguments every entry point takes
# ---------------------------------------------------------------------------------------
def _call_args(y, p1):
    """-> (dev, nb, nc, shape, bt, probs pointer, stream, what must stay alive)."""
    dev = torch.device("cuda")
    nb, R = p1.shape
    nc = int(round((1 + math.sqrt(1 + 4 * R)) / 2))
    ybits = torch.from_numpy(data.pack_bits(data._grid(y, nc)).view(np.int32)).to(dev)
    pt = torch.from_numpy(_probs(p1)).to(dev).contiguous()
    shape = _lib.Shape(nb, 20, nc, 2, nb, 0)
    bt = _lib.Batch(None, None, ybits.data_ptr(), None, None, None)
    stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    return dev, nb, nc, shape, bt, ctypes.c_void_p(pt.data_ptr()), stream, (ybits, pt)


# ---- hdg_untangle -------------------------------------------------------------------------
class _UntangleBufs:
    """Poisoned outputs and workspace: the call writes every slot itself."""

    def __init__(self, nb, nc, dev):
        shape = _lib.Shape(nb, 20, nc, 2, nb, 0)
        nbytes = _lib.load().hdg_untangle_workspace_bytes(ctypes.byref(shape))
        assert nbytes == nb * _lib.untangle_blocks(nc) * (nc + 2) * 4
        self.groups = torch.full((nb, nc), -7, dtype=torch.int32, device=dev)
        self.tgroups = torch.full((nb, nc), -7, dtype=torch.int32, device=dev)
        self.ut = torch.full((nb, _lib.UT_SLOTS), -1, dtype=torch.int64, device=dev)
        self.ws = torch.full((nbytes // 4,), 0x7F7F7F7F, dtype=torch.int32, device=dev)


def _untangle_run(y, p1, thr=0.5, rule="mean", bufs=None, tgroups=True):
    """hdg_untangle on relation labels y (b, R) and scores p1 (b, R) -> (bufs, groups,
    tgroups, ut) as numpy arrays read back from the device."""
    lib = _lib.load()
    dev, nb, nc, shape, bt, probs, stream, _keep = _call_args(y, p1)
    bufs = bufs or _UntangleBufs(nb, nc, dev)
    _lib.check(lib.hdg_untangle(ctypes.byref(shape), ctypes.byref(bt), probs, ctypes.c_float(thr),
                                _lib.UT_RULES[rule], ctypes.c_void_p(bufs.groups.data_ptr()),
                                ctypes.c_void_p(bufs.tgroups.data_ptr()) if tgroups else None,
                                ctypes.c_void_p(bufs.ut.data_ptr()),
                                ctypes.c_void_p(bufs.ws.data_ptr()), stream))
    torch.cuda.synchronize(dev)
    return bufs, bufs.groups.cpu().numpy(), bufs.tgroups.cpu().numpy(), bufs.ut.cpu().numpy()


# ---- hdg_linkage, hdg_agglomerate: the five outputs of a merge tree ------------------------
class _TreeBufs:
    """Poisoned outputs and workspace: the call writes every slot itself."""

    def __init__(self, nb, nc, dev, ws_words, ws_dtype, ws_poison):
        self.merges = torch.full((nb, nc - 1, 2), -7, dtype=torch.int32, device=dev)
        self.levels = torch.full((nb, nc - 1), 12345.0, dtype=torch.float32, device=dev)
        self.curve = torch.full((nb, nc - 1, 2), -7, dtype=torch.int32, device=dev)
        self.tgroups = torch.full((nb, nc), -7, dtype=torch.int32, device=dev)
        self.lk = torch.full((nb, _lib.LK_SLOTS), -1, dtype=torch.int64, device=dev)
        self.ws = torch.full((ws_words,), ws_poison, dtype=ws_dtype, device=dev)
        self.ws_poison = ws_poison

    def outputs(self):
        return (self.merges, self.levels, self.curve, self.tgroups, self.lk)

    def poisoned(self):
        return bool((self.merges == -7).all() and (self.levels == 12345.0).all()
                    and (self.curve == -7).all() and (self.tgroups == -7).all()
                    and (self.lk == -1).all() and (self.ws == self.ws_poison).all())

    def read(self):
        return tuple(x.cpu().numpy() for x in self.outputs())


class _LinkageBufs(_TreeBufs):
    def __init__(self, nb, nc, dev):
        shape = _lib.Shape(nb, 20, nc, 2, nb, 0)
        nbytes = _lib.load().hdg_linkage_workspace_bytes(ctypes.byref(shape))
        assert nbytes == nb * _lib.untangle_blocks(nc) * nc * 8
        super().__init__(nb, nc, dev, nbytes // 8, torch.int64, POISON_WS)


class _AgglomerateBufs(_TreeBufs):
    def __init__(self, nb, nc, dev, flags=0):
        shape = _lib.Shape(nb, 20, nc, 2, nb, 0)
        nbytes = _lib.load().hdg_agglomerate_workspace_bytes(ctypes.byref(shape), flags)
        assert nbytes == nb * nc * nc * 4
        super().__init__(nb, nc, dev, nbytes // 4, torch.int32, 0x7F7F7F7F)


def _linkage_run(y, p1, rule="mean", bufs=None, tgroups=True):
    """hdg_linkage on relation labels y (b, R) and scores p1 (b, R) -> (bufs, the five outputs
    as numpy arrays read back from the device)."""
    lib = _lib.load()
    dev, nb, nc, shape, bt, probs, stream, _keep = _call_args(y, p1)
    bufs = bufs or _LinkageBufs(nb, nc, dev)
    vp = ctypes.c_void_p
    _lib.check(lib.hdg_linkage(ctypes.byref(shape), ctypes.byref(bt), probs,
                               _lib.UT_RULES[rule], vp(bufs.merges.data_ptr()),
                               vp(bufs.levels.data_ptr()), vp(bufs.curve.data_ptr()),
                               vp(bufs.tgroups.data_ptr()) if tgroups else None,
                               vp(bufs.lk.data_ptr()), vp(bufs.ws.data_ptr()), stream))
    torch.cuda.synchronize(dev)
    return bufs, bufs.read()


def _agglomerate_run(y, p1, rule="mean", method="average", flags=0, bufs=None, tgroups=True):
    """hdg_agglomerate on relation labels y (b, R) and scores p1 (b, R) -> (bufs, the five
    outputs as numpy arrays read back from the device)."""
    lib = _lib.load()
    dev, nb, nc, shape, bt, probs, stream, _keep = _call_args(y, p1)
    bufs = bufs or _AgglomerateBufs(nb, nc, dev, flags)
    vp = ctypes.c_void_p
    _lib.check(lib.hdg_agglomerate(ctypes.byref(shape), ctypes.byref(bt), probs,
                                   _lib.UT_RULES[rule], _lib.AG_METHODS[method], flags,
                                   vp(bufs.merges.data_ptr()), vp(bufs.levels.data_ptr()),
                                   vp(bufs.curve.data_ptr()),
                                   vp(bufs.tgroups.data_ptr()) if tgroups else None,
                                   vp(bufs.lk.data_ptr()), vp(bufs.ws.data_ptr()), stream))
    torch.cuda.synchronize(dev)
    return bufs, bufs.read()


def _same(dev, host, what=""):
    """The five device outputs of a merge tree == the host's."""
    (m, lv, cv, t, lk), (hm, hlv, hcv, ht, hlk) = dev, host
    np.testing.assert_array_equal(lk, hlk, what)
    np.testing.assert_array_equal(m, hm, what)
    pad = np.isnan(hlv)
    np.testing.assert_array_equal(np.isnan(lv), pad, what)
    np.testing.assert_array_equal(lv.view(np.uint32)[~pad], hlv.view(np.uint32)[~pad], what)
    np.testing.assert_array_equal(cv, hcv, what)
    np.testing.assert_array_equal(t, ht, what)


def _cut(nc, merges, levels, curve, lk, thr, rule, ut=True):
    """hdg_cut on numpy trees -> (groups, ut) read back; buffers poisoned before the call."""
    lib = _lib.load()
    dev = torch.device("cuda")
    nb = len(levels)
    vp = ctypes.c_void_p
    tm = torch.from_numpy(np.ascontiguousarray(merges, np.int32)).to(dev)
    tl = torch.from_numpy(np.ascontiguousarray(levels, np.float32)).to(dev)
    tc = torch.from_numpy(np.ascontiguousarray(curve).astype(np.int32)).to(dev)
    tk = torch.from_numpy(np.ascontiguousarray(lk, np.int64)).to(dev)
    groups = torch.full((nb, nc), -7, dtype=torch.int32, device=dev)
    row = torch.full((nb, _lib.CUT_SLOTS), -1, dtype=torch.int64, device=dev)
    shape = _lib.Shape(nb, 20, nc, 2, nb, 0)
    stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    _lib.check(lib.hdg_cut(ctypes.byref(shape), vp(tm.data_ptr()), vp(tl.data_ptr()),
                           vp(tc.data_ptr()) if ut else None, vp(tk.data_ptr()) if ut else None,
                           ctypes.c_float(thr), _lib.UT_RULES[rule], vp(groups.data_ptr()),
                           vp(row.data_ptr()) if ut else None, stream))
    torch.cuda.synchronize(dev)
    return groups.cpu().numpy(), row.cpu().numpy()


# ---- hdg_refine ---------------------------------------------------------------------------
class _RefineBufs:
    """Poisoned outputs and workspace: the call writes every slot itself."""

    def __init__(self, nb, nc, dev):
        shape = _lib.Shape(nb, 20, nc, 2, nb, 0)
        nbytes = _lib.load().hdg_refine_workspace_bytes(ctypes.byref(shape), 0)
        t = -(-nc // T)
        assert nbytes % 8 == 0 and nbytes >= nb * (nc * nc + t * (t + 1) // 2) * 4
        self.groups = torch.full((nb, nc), -7, dtype=torch.int32, device=dev)
        self.ut = torch.full((nb, _lib.RF_SLOTS), -1, dtype=torch.int64, device=dev)
        self.rq = torch.full((nb, _lib.RF_Q_SLOTS), -99, dtype=torch.int64, device=dev)
        self.ws = torch.full((nbytes // 8,), POISON_WS, dtype=torch.int64, device=dev)

    def poisoned(self):
        return bool((self.groups == -7).all() and (self.ut == -1).all() and (self.rq == -99).all()
                    and (self.ws == POISON_WS).all())


def _refine_run(y, p1, start=None, thr=0.5, rule="mean", max_sweeps=8, bufs=None, alias=False):
    """hdg_refine on relation labels y (b, R), scores p1 (b, R) and starting ids (b, nc) or
    None -> (bufs, groups, ut, rq) read back.  alias: groups_in is the output array itself."""
    lib = _lib.load()
    dev, nb, nc, shape, bt, probs, stream, _keep = _call_args(y, p1)
    bufs = bufs or _RefineBufs(nb, nc, dev)
    gin = None
    if start is not None:
        gin = torch.from_numpy(np.ascontiguousarray(start, np.int32)).to(dev)
        if alias:
            bufs.groups.copy_(gin)
            gin = bufs.groups
    vp = ctypes.c_void_p
    _lib.check(lib.hdg_refine(ctypes.byref(shape), ctypes.byref(bt), probs,
                              ctypes.c_float(thr), _lib.UT_RULES[rule], max_sweeps, 0,
                              None if gin is None else vp(gin.data_ptr()),
                              vp(bufs.groups.data_ptr()), vp(bufs.ut.data_ptr()),
                              vp(bufs.rq.data_ptr()), vp(bufs.ws.data_ptr()), stream))
    torch.cuda.synchronize(dev)
    return bufs, bufs.groups.cpu().numpy(), bufs.ut.cpu().numpy(), bufs.rq.cpu().numpy()
