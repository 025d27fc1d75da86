"""The node-local entity backward (phase E2 of the step kernel) vs the CPU oracle.  GPU only.

E2 forms dW1[0:4] and db1 of mlp_entity_B1 from each own node's rho times rho-free counts and
x sums over its row set and its column set (the forward's set boundaries, kept per node and
unit, and the static prefix tables) plus the a = 1 corrections over the node's row and column
x-lists (tests/test_e2_algebra.py pins the algebra on the CPU).  Every gradient slot of one
hdg_fwd_bwd is compared with the oracle at test_gpu_parity's tolerances (rtol 1.5e-4, atol
3e-6 max|ref| per variable, copied in _slots_close), the 100 slots of E2 first and on their
own so that a failure names them.  Both block forms through Engine.set_split.  B = 9 and
Nc = 9 (the split grid has padding commits) unless a case says otherwise.
"""
import functools

import numpy as np
import pytest
import torch

from hdgnn import _lib, layout
from hdgnn.data import CommitBatch
from hdgnn.synth import synth_commits
from oracle import model_ref
from tests.test_cgrad_defer_gpu import _grad_close4, _oracle, _reg_grad4
from tests.test_gpu_parity import _grad_close, _reg_grad

pytestmark = pytest.mark.gpu

HS = 20
W1_NAME, B1_NAME = "phi_E_O1/r1_w1o:0", "phi_E_O1/r1_b1o:0"


@pytest.fixture(params=[True, False], ids=["split", "one_block"])
def split(request):
    return request.param


def _slots_close(g_eng, g_ref, v, name, reg):
    """test_gpu_parity._grad_close's bound on one variable.  The reference must carry a data
    gradient far above the L2 term's (reg, the regulariser's part of g_ref): with rho = 0, E2
    returns 0 whatever it does, and the case would compare zero with zero.  The floors: 10
    times the L2 term, so that an E2 that returned 0 would miss the bound (about 1.5e-4 of the
    slot) by three orders of magnitude, and 1e-4, which is 1e5 times the bound's absolute term
    1e-9, so the relative terms decide.  The smallest case, Ne = 2, has 1.3e-2 in W1 (67 times
    its L2 term) and 2.9e-3 in b1; from Ne = 16 on the data part is above 1."""
    o, shape = layout.offsets(v)[name]
    n = int(np.prod(shape))
    a, r = g_eng[o:o + n], g_ref[o:o + n]
    data = np.abs(r - reg[o:o + n]).max()
    assert data >= 1e-4 and data >= 10 * np.abs(reg[o:o + n]).max(), \
        "%s: the case carries no gradient to E2 (data part %.3g)" % (name, data)
    scale = max(np.abs(r).max(), 1e-12)
    tol = 1.5e-4 * np.abs(r) + 3e-6 * scale + 1e-9
    err = np.abs(a - r)
    print("%s: max err %.3g of scale %.3g, worst err / tol %.3g" % (
        name, np.nanmax(err), scale, np.nanmax(err / tol)))
    assert np.all(err <= tol), "%s: max err %.3g, scale %.3g, %d/%d bad" % (
        name, np.nanmax(err), scale, int((~(err <= tol)).sum()), n)


# ---- cases: name -> (batch, initial parameters), built once ---------------------------
def _w1_regime(flat, kind, seed):
    """mlp_entity_B1's W1 rows set explicitly.  Rows 0, 1 (w0, w1: which side of the sorted
    order the column and row sets are): all >= 0, all < 0, or all four sign combinations over
    the units.  Rows 2, 3 (d = W1[3] - W1[2]): d > 0, d < 0, d = 0 and 0 < |d| < 2^-100 in turn,
    a unit dead for every pair and one live for every pair (set boundaries 0 and nd).  b1 is
    nonzero so that no pre-activation is exactly 0 at x = 0."""
    rng = np.random.default_rng(seed)
    W = np.abs(rng.standard_normal((4, HS)) * 0.1 + 0.02).astype(np.float32)
    k = np.arange(HS)
    if kind == "neg":
        W[0], W[1] = -W[0], -W[1]
    elif kind == "mixed":
        W[0] = np.where(k & 1, -W[0], W[0])
        W[1] = np.where(k & 2, -W[1], W[1])
    W[2] = (rng.standard_normal(HS) * 0.3).astype(np.float32)
    dsel = (k >> 2) % 4
    W[3] = W[2] + np.select([dsel == 0, dsel == 1, dsel == 2], [0.25, -0.25, 0.0], 0.0).astype(np.float32)
    tiny = dsel == 3
    W[2, tiny] = 0.0
    W[3, tiny] = np.where(k[tiny] & 1, 2.0 ** -110, -2.0 ** -110)
    W[2, 16] = W[3, 16] = -100.0                 # dead for every pair
    W[2, 17] = W[3, 17] = 100.0                  # live for every pair
    flat = flat.copy()
    flat[0:4 * HS] = W.reshape(-1)
    flat[4 * HS:5 * HS] = (rng.uniform(0.05, 0.3, HS) * rng.choice([-1, 1], HS)).astype(np.float32)
    return flat


def _tri(cb, upper):
    ne = cb.Ne
    m = np.random.default_rng(ne).random((cb.x.shape[0], ne, ne)) < 0.4
    m = np.triu(m, 1) if upper else np.tril(m, -1)
    assert m.any()
    return CommitBatch(cb.x, m.astype(np.uint8), cb.y, cb.hid, cb.nlen)


def _alive(flat, v):
    """mlp2_entity_B1 with positive biases and w2' >= 0: o = h w2' + b2' > 0 on every node, so
    x' = relu(o) is alive and a gradient reaches the entity stage in every case (at the zero
    initial biases a small graph can have o <= 0 throughout: rho = 0, and E2 is not tested).
    _slots_close asserts that it did."""
    flat, offs = flat.copy(), layout.offsets(v)
    for name, val in (("phi_U_O1/o1_b1o:0", 0.2), ("phi_U_O1/o1_b2o:0", 0.5)):
        o, shape = offs[name]
        flat[o:o + int(np.prod(shape))] = val
    o, shape = offs["phi_U_O1/o1_w2o:0"]
    flat[o:o + int(np.prod(shape))] = np.abs(flat[o:o + int(np.prod(shape))])
    return flat


def _build(name):
    cb, flat, v = _build0(name)
    return cb, _alive(flat, v), v


def _build0(name):
    B, nc, v = 9, 9, 2
    kind, _, arg = name.partition(":")
    if kind == "ne":
        ne = int(arg)
        return synth_commits(B, ne, nc, 100 + ne), layout.init_flat(ne), v
    if kind == "tri":
        return _tri(synth_commits(B, 33, nc, 133), arg == "upper"), layout.init_flat(33), v
    if kind == "a":
        cb = synth_commits(B, 17, nc, 117)
        a = 0 * cb.a if arg == "empty" else 1 - np.eye(17, dtype=np.uint8)[None] + 0 * cb.a
        return CommitBatch(cb.x, a, cb.y, cb.hid, cb.nlen), layout.init_flat(17), v
    if kind == "w1":
        return synth_commits(B, 33, nc, 133), _w1_regime(layout.init_flat(33), arg, 7), v
    if kind == "x":
        if arg == "equal":
            cb = synth_commits(B, 33, nc, 133)
            return CommitBatch(0 * cb.x + 3, cb.a, cb.y, cb.hid, cb.nlen), layout.init_flat(33), v
        return synth_commits(B, 33, nc, 133, xkind="real"), layout.init_flat(33), v
    if kind == "nlen":                           # 1 < nlen < Ne index lines per commit
        cb = synth_commits(B, 33, nc, 133)
        nlen = np.minimum(cb.nlen, 20)
        assert (nlen > 1).all() and (nlen < 33).all()
        return CommitBatch(cb.x, cb.a, cb.y, cb.hid, nlen), layout.init_flat(33), v
    if kind == "hbm":                            # x-lists of 2 * 256 * ~128 words: not in LDS
        return synth_commits(2, 256, nc, 256, edensity=0.5), layout.init_flat(256), v
    if kind == "model4":
        return synth_commits(B, 33, 17, 133), layout.init_flat(33, 4), 4
    if kind == "wide":
        return synth_commits(B, 33, 81, 133), layout.init_flat(33), v
    raise KeyError(name)


STEPS = 3


@functools.lru_cache(maxsize=None)
def _case(name, steps=1):
    """(batch, parameters, variant, oracle trajectory [(out, g_ref, theta after)]), shared by
    both block forms"""
    cb, flat, v = _build(name)
    theta = flat.astype(np.float64)
    opt = model_ref.AdamTF(len(flat))
    traj = []
    for _ in range(steps):
        out, g_ref = _oracle(theta.astype(np.float32), cb, v)
        theta = opt.step(theta, g_ref)
        traj.append((out, g_ref, theta.copy()))
    return cb, flat, v, traj


def _engine(cb, v, split):
    from hdgnn.engine import Engine
    eng = Engine(cb.Ne, cb.Nc, cb.x.shape[0], variant=v, path=_lib.PATH_FUSED)
    assert eng.path == _lib.PATH_FUSED
    eng.set_split(split)
    return eng


def _check_gradients(name, split):
    cb, flat, v, traj = _case(name)
    out, g_ref, _ = traj[0]
    eng = _engine(cb, v, split)
    eng.set_params(flat)
    eng.fwd_bwd(eng.upload(cb))
    torch.cuda.synchronize()
    eng.check_status()
    g = eng.grad.cpu().numpy().astype(np.float64)
    n = len(flat)
    reg = _reg_grad(flat) if v == 2 else _reg_grad4(flat)
    g_eng = g[:n] + reg
    _slots_close(g_eng, g_ref, v, W1_NAME, reg)
    _slots_close(g_eng, g_ref, v, B1_NAME, reg)
    (_grad_close if v == 2 else _grad_close4)(g_eng, g_ref)
    B, nc = cb.x.shape[0], cb.Nc
    np.testing.assert_allclose(g[n] / (B * nc * (nc - 1)), float(out["ce"]), rtol=1e-5)


def _check_steps(eng, db, traj):
    for out, _, theta in traj:
        eng.train_step(db)
        torch.cuda.synchronize()
        eng.check_status()
        stats = eng.stats.cpu().numpy()
        for i, k in enumerate(("ce", "loss_map", "loss_para", "total")):
            np.testing.assert_allclose(stats[i], float(out[k]), rtol=1e-5)
        np.testing.assert_allclose(eng.get_params(), theta, rtol=0, atol=2e-6)


@pytest.mark.parametrize("ne", [2, 3, 7, 16, 17, 33, 66, 200])
def test_node_counts(ne, split):
    """odd Ne: the halves' boundary is (Ne + 1) / 2.  A wave's round covers 96 nodes: Ne = 200
    (lists staged in LDS) takes a second, partial round of 4 nodes per half in split mode and
    two full rounds and one of 8 nodes in one block; the smaller Ne stay within one round."""
    _check_gradients("ne:%d" % ne, split)


@pytest.mark.parametrize("side", ["upper", "lower"])
def test_triangular_adjacency(side, split):
    """row and column lists differ: a swapped list or a swapped x role fails"""
    _check_gradients("tri:" + side, split)


@pytest.mark.parametrize("fill", ["empty", "full"])
def test_empty_and_full_adjacency(fill, split):
    _check_gradients("a:" + fill, split)


@pytest.mark.parametrize("kind", ["pos", "neg", "mixed"])
def test_first_layer_regimes(kind, split):
    _check_gradients("w1:" + kind, split)


@pytest.mark.parametrize("kind", ["equal", "real"])
def test_attribute_kinds(kind, split):
    """all x equal: nd = 1; real x: nd = Ne distinct values"""
    _check_gradients("x:" + kind, split)


def test_short_index_lists(split):
    _check_gradients("nlen:20", split)


def test_lists_beyond_lds(split):
    """Ne = 256 at density 0.5: both walks read their lists from the prepared buffer"""
    _check_gradients("hbm:", split)


def test_model4_hybrid(split):
    _check_gradients("model4:", split)


def test_wide_form(split):
    _check_gradients("wide:", split)


def test_adam_steps_match_oracle(split):
    cb, flat, v, traj = _case("ne:33", STEPS)
    eng = _engine(cb, v, split)
    eng.set_params(flat)
    _check_steps(eng, eng.upload(cb), traj)


def test_deterministic_bitwise(split):
    cb, flat, v, _ = _case("ne:66")
    eng = _engine(cb, v, split)
    eng.set_params(flat)
    db = eng.upload(cb)
    eng.fwd_bwd(db)
    g1, p1 = eng.grad.cpu().numpy().copy(), eng.probs.cpu().numpy().copy()
    eng.fwd_bwd(db)
    assert np.array_equal(g1, eng.grad.cpu().numpy())
    assert np.array_equal(p1, eng.probs.cpu().numpy())


def test_steps_after_exchange_timeout(monkeypatch):
    """The pair's epoch now advances after the dn exchange.  A step whose exchanges timed out
    (the debug knob; its update is skipped) must leave the engine able to run: the next two
    steps, on the same engine, follow the oracle trajectory from the initial parameters -- a
    stale tag accepted in either would not."""
    cb, flat, v, traj = _case("ne:33", STEPS)
    eng = _engine(cb, v, True)
    eng.set_params(flat)
    db = eng.upload(cb)
    monkeypatch.setenv("HDG_DEBUG_XCH_FAULT", "1")
    eng.train_step(db)
    torch.cuda.synchronize()
    assert int(eng.status.item()) == _lib.STATUS_XCH_TIMEOUT
    np.testing.assert_array_equal(eng.get_params(), flat)
    monkeypatch.delenv("HDG_DEBUG_XCH_FAULT")
    eng.clear_status()
    _check_steps(eng, db, traj[:2])
