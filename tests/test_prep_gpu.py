"""hdg_prepare's cross-graph count tables against the oracle's relation maps, bit-exact.

K_s[c][I] = #{relations r in Ne-row I : s_r = c} + #{... : t_r = c}, K_t over Ne-columns,
ncst[c][a] = the same counts split by the relation's class a (utils2.py:111-137, the
marshalling_B2 maps of model_2.py:146-150; s_r, t_r walk the n-grid: oracle.model_ref.
relation_maps).  Cases: n in {0, 1, 2, Ne}, unmapped nodes, every node mapped, both
engine paths, the stress shape.

Also read back bit-exact: the entity neighbour lists; the tables built from the hunk labels
(yT and the label id lists, under labels with y != y^T); the entity-edge dispatch orders."""
import ctypes

import numpy as np
import pytest

from hdgnn import _lib
from hdgnn.synth import synth_commits
from oracle import model_ref

pytestmark = pytest.mark.gpu


def expected_counts(cb):
    B, ne = cb.x.shape
    nc = cb.y.shape[1]
    s, t = model_ref.relation_maps(cb.hid, cb.nlen, ne, nc)
    I, J = model_ref.pair_index(ne)
    ks = np.zeros((B, nc, ne), np.int64)
    kt = np.zeros((B, nc, ne), np.int64)
    ncst = np.zeros((B, nc, 2), np.int64)
    for b in range(B):
        a = cb.a[b, I, J].astype(np.int64)
        for h in (s[b], t[b]):
            m = h >= 0
            np.add.at(ks[b], (h[m], I[m]), 1)
            np.add.at(kt[b], (h[m], J[m]), 1)
            np.add.at(ncst[b], (h[m], a[m]), 1)
    return ks, kt, ncst


def device_counts(db, ne, nc, variant, path):
    lib = _lib.load()
    sh = _lib.Shape(db.B, ne, nc, variant, db.B, path)
    st, ks, kt, nco = (ctypes.c_int64() for _ in range(4))
    _lib.check(lib.hdg_prep_counts_layout(ctypes.byref(sh), ctypes.byref(st), ctypes.byref(ks),
                                          ctypes.byref(kt), ctypes.byref(nco)))
    words = db.prep.cpu().numpy().view(np.uint32)[:db.B * st.value].reshape(db.B, st.value)
    u16 = lambda o: words[:, o:o + (nc * ne + 1) // 2].copy().view(np.uint16)[:, :nc * ne]
    return (u16(ks.value).reshape(db.B, nc, ne), u16(kt.value).reshape(db.B, nc, ne),
            words[:, nco.value:nco.value + 2 * nc].copy().view(np.float32).reshape(db.B, nc, 2))


@pytest.mark.parametrize("B,ne,nc,variant,path", [
    (5, 24, 10, 2, _lib.PATH_FUSED), (5, 24, 10, 2, _lib.PATH_GENERAL),
    (6, 200, 74, 2, _lib.PATH_FUSED), (6, 200, 74, 4, _lib.PATH_GENERAL),
    (5, 250, 150, 2, _lib.PATH_FUSED), (5, 300, 33, 1, _lib.PATH_GENERAL),
    (2, 1024, 512, 2, _lib.PATH_GENERAL)])
def test_count_tables_bit_exact(B, ne, nc, variant, path):
    cb = synth_commits(B, ne, nc, 11 + ne + nc)
    for i, n in enumerate([0, 1, 2, ne][:B - 1]):
        cb.nlen[i] = n
    cb.nlen[-1] = ne
    cb.hid[-1] = np.random.default_rng(ne).integers(0, nc, ne)   # every node mapped
    db = cb.to_device("cuda:0", variant, path)
    ks, kt, ncst = device_counts(db, ne, nc, variant, path)
    eks, ekt, encst = expected_counts(cb)
    np.testing.assert_array_equal(ks, eks)
    np.testing.assert_array_equal(kt, ekt)
    np.testing.assert_array_equal(ncst, encst.astype(np.float32))


@pytest.mark.parametrize("B,ne,nc,variant", [
    (3, 24, 10, 2), (3, 37, 12, 4), (4, 200, 74, 4), (2, 1024, 512, 2), (3, 5, 3, 2)])
def test_neighbour_lists_bit_exact(B, ne, nc, variant):
    """The general path's per-node neighbour id lists (wide.hip kw_prep_lists: side 0 the
    j != i with a_ij = 1, side 1 the j with a_ji = 1, ascending, padded to 4 with the
    sentinel ne) against the adjacency, including a full and an empty commit."""
    cb = synth_commits(B, ne, nc, 5 + ne)
    cb.a[0] = 1                      # full adjacency, diagonal included (lists skip j == i)
    cb.a[1] = 0
    db = cb.to_device("cuda:0", variant, _lib.PATH_GENERAL)
    lib = _lib.load()
    sh = _lib.Shape(B, ne, nc, variant, B, _lib.PATH_GENERAL)
    st, ks, kt, nco = (ctypes.c_int64() for _ in range(4))
    _lib.check(lib.hdg_prep_counts_layout(ctypes.byref(sh), ctypes.byref(st), ctypes.byref(ks),
                                          ctypes.byref(kt), ctypes.byref(nco)))
    we, wc, ls = (ne + 31) // 32, (nc + 31) // 32, (ne + 3) & ~3
    c0 = (B * st.value + B * ne * we + B * nc * wc + 3) & ~3
    i0 = c0 + ((2 * B * ne + 3) & ~3)
    words = db.prep.cpu().numpy().view(np.uint32)
    assert words.size >= i0 + B * ne * ls
    cnt = words[c0:c0 + 2 * B * ne].reshape(2, B, ne)
    ids = words[i0:i0 + B * ne * ls].copy().view(np.uint16).reshape(2, B, ne, ls)
    for side, adj in ((0, cb.a), (1, cb.a.transpose(0, 2, 1))):
        for b in range(B):
            for i in range(ne):
                exp = np.flatnonzero(adj[b, i])
                exp = exp[exp != i]
                n = len(exp)
                assert cnt[side, b, i] == n, (side, b, i)
                np.testing.assert_array_equal(ids[side, b, i, :n], exp)
                assert (ids[side, b, i, n:(n + 3) & ~3] == ne).all()


@pytest.mark.parametrize("B,n", [(3, 7), (2, 33), (4, 200), (1, 1100)])
def test_pack_classes_matches_host(B, n):
    """hdg_pack_classes (the upload's device-side bit packing) == data.pack_bits."""
    import ctypes
    import torch
    from hdgnn import _lib
    from hdgnn.data import pack_bits
    rng = np.random.default_rng(n)
    grid = (rng.random((B, n, n)) < 0.3).astype(np.uint8)
    g = torch.from_numpy(grid).cuda()
    out = torch.full((B, n, (n + 31) // 32), -1, dtype=torch.int32, device="cuda")
    lib = _lib.load()
    _lib.check(lib.hdg_pack_classes(ctypes.c_void_p(g.data_ptr()), B, n,
                                    ctypes.c_void_p(out.data_ptr()),
                                    ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)))
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy().view(np.uint32), pack_bits(grid))


# ----------------------------------------------------------------------------
# the tables built from the hunk labels, and the entity-edge dispatch orders
# ----------------------------------------------------------------------------
def _gen_layout(B, ne, nc, ent):
    """Word offsets inside a general-path prep (csrc/wide.hip: gen_prep's stride through
    hdg_prep_counts_layout, then aT, yT, list_layout, ylist_layout restated)."""
    lib = _lib.load()
    sh = _lib.Shape(B, ne, nc, 2 if ent else 1, B, _lib.PATH_GENERAL)
    st, ks, kt, nco = (ctypes.c_int64() for _ in range(4))
    _lib.check(lib.hdg_prep_counts_layout(ctypes.byref(sh), ctypes.byref(st), ctypes.byref(ks),
                                          ctypes.byref(kt), ctypes.byref(nco)))
    we, wc = (ne + 31) // 32, (nc + 31) // 32
    L = {"aT": B * st.value}
    L["yT"] = L["aT"] + B * ne * we
    L["cnt"] = (L["yT"] + B * nc * wc + 3) & ~3
    L["ids"] = L["cnt"] + ((2 * B * ne + 3) & ~3)
    L["end"] = L["ids"] + B * ne * ((ne + 3) & ~3)
    L["ycnt"] = ((L["end"] if ent else L["cnt"]) + 3) & ~3
    L["yids"] = L["ycnt"] + ((2 * B * nc + 3) & ~3)
    L["yend"] = L["yids"] + B * nc * ((nc + 3) & ~3)
    return L


def _check_label_tables(cb, variant):
    from hdgnn.data import pack_bits
    B, ne, nc = cb.B, cb.Ne, cb.Nc
    db = cb.to_device("cuda:0", variant, _lib.PATH_GENERAL)
    L = _gen_layout(B, ne, nc, variant in (2, 4))
    wc, ls = (nc + 31) // 32, (nc + 3) & ~3
    words = db.prep.cpu().numpy().view(np.uint32)
    assert words.size == L["yend"]                # model_1 / model_2: the lists end the prep
    yT = words[L["yT"]:L["yT"] + B * nc * wc].reshape(B, nc, wc)
    np.testing.assert_array_equal(yT, pack_bits(cb.y.transpose(0, 2, 1)))
    np.testing.assert_array_equal(db.ybits.cpu().numpy().view(np.uint32), pack_bits(cb.y))
    cnt = words[L["ycnt"]:L["ycnt"] + 2 * B * nc].reshape(2, B, nc)
    ids = words[L["yids"]:L["yend"]].copy().view(np.uint16).reshape(2, B, nc, ls)
    for side, adj in ((0, cb.y), (1, cb.y.transpose(0, 2, 1))):
        for b in range(B):
            for p in range(nc):
                exp = np.flatnonzero(adj[b, p])
                exp = exp[exp != p]
                n = len(exp)
                assert cnt[side, b, p] == n, (side, b, p)
                np.testing.assert_array_equal(ids[side, b, p, :n], exp)
                assert (ids[side, b, p, n:(n + 3) & ~3] == nc).all()


@pytest.mark.parametrize("variant", [2, 1], ids=["entity_lists", "no_entity_lists"])
@pytest.mark.parametrize("kind", ["directed", "upper"])
@pytest.mark.parametrize("B,ne,nc,lseed", [(3, 5, 3, 73), (3, 37, 12, 52), (2, 40, 257, 297),
                                           (4, 200, 74, 114)])
def test_label_tables_bit_exact(B, ne, nc, lseed, kind, variant):
    """yT = the words of pack_bits(y^T), and the hunk label id lists (kw_prep_lists on ybits /
    yT at ylist_layout: side 0 the q != p with y_pq = 1, side 1 the p with y_pq = 1, ascending,
    padded to 4 with the sentinel Nc) under labels with y != y^T -- with a symmetric y, yT could
    be a copy of ybits and the two sides each other's.  Once with the labels as drawn (every
    commit asymmetric; 73 is the first label seed from 40 + Nc at which all three 3 x 3 commits
    of both kinds are), once with commit 0 full (diagonal set in the host grid, which the
    packer and the lists drop) and commit 1 empty.  model_2 has the entity lists in front of
    the label lists, model_1 has not: the lists sit at different offsets."""
    from tests._labels import commits
    cb = commits(kind, B, ne, nc, 5 + ne, lseed)
    assert (cb.y != cb.y.transpose(0, 2, 1)).any(axis=(1, 2)).all()
    _check_label_tables(cb, variant)
    cb.y[0] = 1
    cb.y[1] = 0
    _check_label_tables(cb, variant)


# csrc/wide.hip, restated: TF index rows per kw_ee_fwd block, its tiles per commit, a commit's
# relation rows ceil(n (n - 1) / (Ne - 1)) for n = nlen clamped to [0, Ne]
EE_TF = 32


def _ee_fwd_tiles(ne):
    return (ne + EE_TF - 1) // EE_TF


def _ee_rows(n, ne):
    n = np.clip(np.asarray(n, np.int64), 0, ne)
    return np.where(n < 2, 0, np.minimum((n * (n - 1) + ne - 2) // (ne - 1), ne))


def _rank_desc(key):
    """ids by decreasing key, ties by index"""
    return np.argsort(-np.asarray(key, np.int64), kind="stable")


@pytest.mark.parametrize("path", [_lib.PATH_GENERAL, _lib.PATH_FUSED], ids=["general", "fused"])
def test_ee_dispatch_orders_bit_exact(path):
    """kw_prep_order's table (model_4; the dispatch orders of kw_ee_clsb / kw_ee_fwd): the first
    B words are the commits by decreasing relation rows, after the rounding of B to 4 the te B
    words are the (commit, tile) ids b te + T by decreasing key (n where n >= 2 and the tile
    holds index rows, T TF < n; else 0), ties by index; both are permutations -- a table that
    is not skips or repeats blocks.  nlen holds 0, 1, 2, Ne, equal values and values on both
    sides of the 32-row tile edges; B = 11 is no multiple of 4, Ne = 70 has three tiles.  On
    the fused path the general-path tables follow the fused prep, without label lists."""
    B, ne, nc, v = 11, 70, 9, 4
    cb = synth_commits(B, ne, nc, 77)
    cb.nlen[:] = [0, 1, 2, ne, 33, 33, 32, 64, 65, 33, ne]
    db = cb.to_device("cuda:0", v, path)
    words = db.prep.cpu().numpy().view(np.uint32)
    L = _gen_layout(B, ne, nc, True)
    if path == _lib.PATH_GENERAL:
        off = L["yend"]
    else:
        lib = _lib.load()
        sh = _lib.Shape(B, ne, nc, v, B, path)
        st, ks, kt, nco = (ctypes.c_int64() for _ in range(4))
        _lib.check(lib.hdg_prep_counts_layout(ctypes.byref(sh), ctypes.byref(st),
                                              ctypes.byref(ks), ctypes.byref(kt),
                                              ctypes.byref(nco)))
        off = B * st.value + L["end"]
    te, B4 = _ee_fwd_tiles(ne), (B + 3) & ~3
    assert te == 3 and B4 != B
    assert words.size == off + B4 + te * B
    first = words[off:off + B]
    assert sorted(first.tolist()) == list(range(B))
    np.testing.assert_array_equal(first, _rank_desc(_ee_rows(cb.nlen, ne)))
    n = np.clip(cb.nlen.astype(np.int64), 0, ne)
    bb, T = np.divmod(np.arange(te * B), te)
    key = np.where((n[bb] >= 2) & (T * EE_TF < n[bb]), n[bb], 0)
    second = words[off + B4:off + B4 + te * B]
    assert sorted(second.tolist()) == list(range(te * B))
    np.testing.assert_array_equal(second, _rank_desc(key))
    assert len(set(_ee_rows(cb.nlen, ne).tolist())) < B      # ties among the commits
