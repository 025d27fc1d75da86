"""What ends a training step -- the partial-row reduction, TF1 ApplyAdam (csrc/adam_tf.h), the
loss stats, the correct-prediction count -- off a fresh start.  GPU only.  Tables, reference
and bounds: tests/_tails.py; their guards and that the bounds bite: tests/test_tails.py.

  A  ApplyAdam of a chosen gradient on a chosen state (36 cases: every variant x step counts
     1 .. 120000, three learning rates, three theta norms; eight slot populations in every
     16-slot group) through hdg_adam_tf (k_adam_tf) and the world-of-one hdg_adam_dp with
     flags 0 (k_dp_aux + k_dp_tail<GRAD>) and HDG_DP_SHARED (k_dp_tail_shared<GRAD>),
     against the TF-exact reference within the counted rounding bound; the two hdg_adam_dp
     runs bit-equal, hdg_adam_tf within the lr_t association width of them; a set fault slot
     leaves the state bit-unchanged.
  B  two teacher-forced steps from a trained state (t = 200 / 1000) through hdg_train_step
     (k_reduce_adam split and one-block, kw_reduce_adam with and without fused rows),
     hdg_fwd_bwd + hdg_adam_tf, and the world-of-one hdg_train_step_dp (k_dp_tail<PART>, the
     shared-device tail, the general path), within the gradient tolerance pushed through the
     reference plus the operator bound.
  C  counts above 2^16: the trailer's and the stats' 16-bit parts against the host's count
     on the returned probabilities and hdg_eval's TP + TN; one two-rank case whose low parts
     carry.
Achieved error / bound goes to the parity report (tests/_errlog.py).
"""
import ctypes
import functools
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from hdgnn import _lib, metrics
from hdgnn.data import onehot_relations
from hdgnn.synth import synth_commits
from tests import _errlog
from tests import _regimes as R
from tests import _tails as T
from tests import test_general_gpu as G
from tests.test_xgmi_gpu import _init, _port

pytestmark = pytest.mark.gpu

PATHS = {"general": _lib.PATH_GENERAL, "fused": _lib.PATH_FUSED}
FLT_MIN = np.finfo(np.float32).tiny


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ----------------------------------------------------------------------------
# a data-parallel world of one: its own mailbox, no peer, nothing waits
# ----------------------------------------------------------------------------
@pytest.fixture(scope="module")
def world_one():
    lib = _lib.load()
    own = ctypes.c_void_p()
    handle = (ctypes.c_ubyte * _lib.DP_HANDLE_BYTES)()
    _lib.check(lib.hdg_dp_mailbox_alloc(ctypes.byref(own), handle))

    def make(flags):
        dp = _lib.Dp()
        dp.rank, dp.world, dp.flags = 0, 1, flags
        dp.mailbox[0] = own.value
        dp.wait_ticks = 100_000_000
        return dp
    yield make
    torch.cuda.synchronize()
    _lib.check(lib.hdg_dp_mailbox_free(own))


def _attach(eng, dp):
    """Engine.train_step / adam through the data-parallel entry points of this world."""
    eng.xgmi = SimpleNamespace(dp=dp)
    eng.grad_local = torch.zeros_like(eng.grad)


def _state(eng):
    torch.cuda.synchronize()
    eng.check_status()
    return SimpleNamespace(w=eng.params.cpu().numpy(), m=eng.m.cpu().numpy(),
                           v=eng.v.cpu().numpy(), bpow=eng.beta_pow.cpu().numpy(),
                           stats=eng.stats.cpu().numpy(), grad=eng.grad.cpu().numpy())


def _put(eng, w, m, v, bpow):
    eng.params.copy_(torch.from_numpy(np.ascontiguousarray(w, np.float32)))
    eng.m.copy_(torch.from_numpy(np.ascontiguousarray(m, np.float32)))
    eng.v.copy_(torch.from_numpy(np.ascontiguousarray(v, np.float32)))
    eng.beta_pow.copy_(torch.from_numpy(np.asarray(bpow, np.float32)))
    eng.stats.fill_(float("nan"))


def _check_powers(got, b1p, b2p, what):
    """Bit-equal to the float32 products; a product below FLT_MIN may come out flushed."""
    for k, (p, c) in enumerate(((b1p, 0.9), (b2p, 0.999))):
        want = np.float32(np.float32(p) * np.float32(c))
        ok = got[k] == want or (want < FLT_MIN and got[k] == 0)
        assert ok, "%s: beta power %d is %r, the float32 product %r" % (what, k, got[k], want)


def _check_update(tag, got, ref, bound, pop=None):
    """theta', m', v' within the bound; the worst error / bound to the report."""
    for k, name in enumerate(("theta", "m", "v")):
        a = (got.w, got.m, got.v)[k].astype(np.float64)
        assert np.isfinite(a).all(), "%s %s: non-finite slots %s" % (
            tag, name, np.nonzero(~np.isfinite(a))[0][:8])
        err = np.abs(a - ref[k])
        with np.errstate(divide="ignore", invalid="ignore"):
            ratio = np.where(err > 0, err / bound[k], 0.0)
        worst = int(ratio.argmax())
        _errlog.record("%s:%s" % (tag, name), err[worst], ratio[worst], slot=worst,
                       population=None if pop is None else str(pop[worst]))
        print("%s %s: worst %.3g of the bound at slot %d" % (tag, name, ratio[worst], worst))
        assert (err <= bound[k]).all(), "%s %s: %.3g of the bound at slot %d%s (%d off)" % (
            tag, name, ratio[worst], worst, "" if pop is None else " (%s)" % pop[worst],
            int((err > bound[k]).sum()))


# ----------------------------------------------------------------------------
# A: the operator on a chosen gradient
# ----------------------------------------------------------------------------
A_SHAPE = (2, 8, 5)               # the engine's shape only sets 1 / pairs for the CE stat
ENTRIES = ("adam_tf", "adam_dp", "adam_dp_shared")


@functools.lru_cache(maxsize=None)
def _a_engine(variant):
    from hdgnn.engine import Engine
    B, ne, nc = A_SHAPE
    eng = Engine(ne, nc, B, variant=variant, path=_lib.PATH_GENERAL)
    eng.a_local = torch.zeros_like(eng.grad)
    return eng


def _a_run(eng, entry, d, grad, make):
    """One call of the entry point on the case's state -> the state it leaves."""
    _put(eng, d["w"], d["m"], d["v"], d["bpow"])
    eng.lr = d["lr"]
    g = torch.from_numpy(grad)
    if entry == "adam_tf":
        eng.grad.copy_(g)
        eng.adam()
        return _state(eng)
    dp = make(_lib.DP_SHARED if entry == "adam_dp_shared" else 0)
    eng.a_local.copy_(g)
    eng.grad.fill_(float("nan"))                       # grad_out: disjoint from grad_local
    _lib.check(eng.lib.hdg_adam_dp(ctypes.byref(eng.shape), ctypes.byref(eng._state),
                                   ctypes.c_void_p(eng.a_local.data_ptr()),
                                   ctypes.c_void_p(eng.grad.data_ptr()), ctypes.c_float(eng.lr),
                                   ctypes.c_void_p(eng.stats.data_ptr()),
                                   ctypes.c_void_p(eng.status.data_ptr()), ctypes.byref(dp),
                                   eng._stream()))
    return _state(eng)


@pytest.mark.parametrize("case", T.A_CASES, ids=T.a_id)
def test_adam_operator(case, world_one):
    d = T.build_a(case)
    n, pop = d["n"], d["pop"]
    eng = _a_engine(case.variant)
    assert eng.np == n and eng.xgmi is None
    ref = T.a_reference(case, d)
    bound = T.a_bound(case, d)
    grad = np.concatenate([d["g"], d["trailer"]])
    B, _, nc = A_SHAPE
    w64 = d["w"].astype(np.float64)
    n1, n2 = T.theta_norms(w64)
    ce = float(d["trailer"][0]) / (B * nc * (nc - 1))
    lmap, lpara = 0.01 * (n1 + n2), 0.0005 * float((w64 * w64).sum())
    want_stats = [ce, lmap, lpara, 10 * ce + 0.1 * lmap + lpara]
    out = {}
    for entry in ENTRIES:
        s = out[entry] = _a_run(eng, entry, d, grad, world_one)
        tag = "A:" + entry
        _check_update(tag, s, ref, bound, pop)
        zero = pop == "zero"
        for a in (s.w, s.m, s.v):                              # 0 / (0 + eps) is 0
            assert (a[zero] == 0).all(), tag
        if d["lr"] == 0:                                        # parameters bit-unchanged
            assert np.array_equal(bits(s.w), bits(d["w"])), tag
            assert not np.array_equal(bits(s.m), bits(d["m"]))  # the moments still move
        _check_powers(s.bpow, d["bpow"][0], d["bpow"][1], tag)
        assert np.isfinite(s.stats).all(), tag
        np.testing.assert_allclose(s.stats[:4], want_stats, rtol=1e-5, err_msg=tag)
        assert np.array_equal(s.stats[4:8], d["trailer"][1:5]), tag
        if entry != "adam_tf":                                  # the world's sum: this rank's
            assert np.array_equal(s.grad, grad), tag
        den = pop == "denormal"     # what the runtime does with denormal moments: recorded
        _errlog.record(tag + ":denormal_moments_kept",
                       float((s.m[den] != 0).mean()), 0.0,
                       v_kept=float((s.v[den] != 0).mean()),
                       power_kept=bool(s.bpow[0] != 0 and s.bpow[1] != 0))
    # the two hdg_adam_dp tails: the same bits in every output (include/hdgnn.h)
    a, b = out["adam_dp"], out["adam_dp_shared"]
    for name in ("w", "m", "v", "bpow", "stats", "grad"):
        assert np.array_equal(bits(getattr(a, name)), bits(getattr(b, name))), name
    # hdg_adam_tf: the one statement on the same norms (adam_sq_sums) gives the same moments
    # and powers; theta' differs by the association of lr_t alone.  k_adam_tf rounds
    # lr sqrt(1 - b2p) / (1 - b1p) left to right, the other sites lr (sqrt(1 - b2p) / (1 - b1p));
    # either lies within 6.5u of the exact factor, the step's product and quotient add 3u to
    # each: 19u of the step, held as ASSOC_REL = 20u, plus one spacing of the stored result.
    t = out["adam_tf"]
    for name in ("m", "v", "bpow"):
        assert np.array_equal(bits(getattr(a, name)), bits(getattr(t, name))), name
    step = np.abs(w64 - ref[0])
    width = T.ASSOC_REL * step + T.spacing32(ref[0])
    diff = np.abs(t.w.astype(np.float64) - a.w)
    _errlog.record("A:adam_tf_vs_adam_dp:theta", diff.max(), (diff / width).max())
    assert (diff <= width).all(), "%.3g of the association width" % (diff / width).max()
    # a faulted step (the trailer's fault slot set): no entry point touches the state
    grad_f = grad.copy()
    grad_f[n + _lib.TR_FAULT] = 1.0
    for entry in ENTRIES:
        s = _a_run(eng, entry, d, grad_f, world_one)
        for name, src in (("w", d["w"]), ("m", d["m"]), ("v", d["v"]), ("bpow", d["bpow"])):
            assert np.array_equal(bits(getattr(s, name)), bits(src)), (entry, name)
        assert s.stats[7] == 1.0, entry


# ----------------------------------------------------------------------------
# B: the tails that take their gradient from the step
# ----------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _b_first(variant, B, ne, nc, dseed, pseed):
    """The entry's batch, parameters and the oracle's gradient there (computed once)."""
    cb = synth_commits(B, ne, nc, dseed)
    flat = R.regime_flat("trained", pseed, variant)
    out, g = G._oracle(flat, cb, variant)
    return cb, flat, out, g


@pytest.fixture
def b_split_env(request, monkeypatch):
    split = request.node.callspec.params["case"].split
    if split is not None:
        monkeypatch.setenv("HDG_FUSED_SPLIT", split)
    return split


@pytest.mark.parametrize("case", T.B_CASES, ids=T.b_id)
def test_step_tails_at_trained_state(case, world_one, b_split_env):
    from hdgnn.engine import Engine
    c = case
    fused = c.path == "fused"
    cb, flat, out0, g0 = _b_first(c.variant, c.B, c.ne, c.nc, c.dseed, c.pseed)
    eng = Engine(c.ne, c.nc, c.B, variant=c.variant, path=PATHS[c.path], lr=c.lr)
    assert eng.path == PATHS[c.path]
    if c.route in ("dp", "dps"):
        _attach(eng, world_one(_lib.DP_SHARED if c.route == "dps" else 0))
    m0, v0 = T.b_state(g0, c.variant, c.pseed)
    _put(eng, flat, m0, v0, T.beta_powers(c.t))
    db = eng.upload(cb)
    tag = "B:%s:%s:v%d" % (c.route, c.path, c.variant)
    for step in (1, 2):
        s0 = _state(eng)
        out, g = (out0, g0) if step == 1 else G._oracle(s0.w, cb, c.variant)
        if c.route == "calls":
            eng.fwd_bwd(db)
            eng.adam()
        else:
            eng.train_step(db)
        s1 = _state(eng)
        assert s1.stats[7] == 0
        w64 = s0.w.astype(np.float64)
        g_red = g - G._reg_grad(s0.w)
        tol = T.b_grad_tol(g, c.variant, fused)
        ref = T.ref_step(s0.w, g_red, s0.m, s0.v, s0.bpow[0], s0.bpow[1], c.lr)
        bound = T.grad_bound(w64, g_red, tol, s0.m, s0.v, s0.bpow[0], s0.bpow[1], c.lr)
        _check_update("%s:step%d" % (tag, step), s1, ref, bound)
        _check_powers(s1.bpow, s0.bpow[0], s0.bpow[1], tag)
        for i, k in enumerate(("ce", "loss_map", "loss_para", "total")):
            rel = abs(s1.stats[i] / float(out[k]) - 1)
            _errlog.record("%s:stats:%s" % (tag, k), rel, rel / 1e-5)
            np.testing.assert_allclose(s1.stats[i], float(out[k]), rtol=1e-5, err_msg=k)
        assert np.array_equal(s1.stats[4:8], s1.grad[eng.np + 1:eng.np + 5])
    assert not np.array_equal(bits(s1.bpow), bits(np.asarray(T.beta_powers(c.t))))


# ----------------------------------------------------------------------------
# C: counts with a second 16-bit part
# ----------------------------------------------------------------------------
def _c_params():
    P = []
    for c in T.C_CASES:
        routes = ["fwd_bwd", "train_step"]
        if c.path == "fused" and c.variant == 2 and c.split == "1":
            routes += ["dp", "dps"]
        P += [pytest.param(c, r, id="%s-%s" % (T.c_id(c), r)) for r in routes]
    return P


def _stats_count(st, one_rank=True):
    for x in st[4:7]:              # a world's low parts may sum past 2^16: that is the carry
        assert x == np.floor(x) and 0 <= x < (65536 if one_rank else 65536 * 256)
    return int(st[4]) + (int(st[5]) << 16) + (int(st[6]) << 32)


@pytest.mark.parametrize("case,route", _c_params())
def test_count_second_part(case, route, world_one, b_split_env):
    from hdgnn.engine import Engine
    c = case
    cb, flat = T.c_inputs(c)
    eng = Engine(c.ne, c.nc, c.B, variant=c.variant, path=PATHS[c.path])
    assert eng.path == PATHS[c.path]
    if route in ("dp", "dps"):
        _attach(eng, world_one(_lib.DP_SHARED if route == "dps" else 0))
    eng.set_params(flat)
    db = eng.upload(cb)
    eng.stats.fill_(float("nan"))
    if route == "fwd_bwd":
        eng.fwd_bwd(db)
    else:
        eng.train_step(db)
    s = _state(eng)
    probs = eng.probs.cpu().numpy()
    want = metrics.top_acc_count(onehot_relations(cb.y), probs)
    tr = s.grad[eng.np:]
    lo, hi, top = (float(tr[_lib.TR_COUNT + k]) for k in range(3))
    print("count %d: parts %g %g %g" % (want, lo, hi, top))
    assert want >= T.COUNT_MIN
    for x in (lo, hi):
        assert x == np.floor(x) and 0 <= x < 65536
    assert hi >= 1 and top == 0
    assert _lib.trailer_count(tr) == want
    if route != "fwd_bwd":
        assert _stats_count(s.stats) == want
        assert np.array_equal(s.stats[4:7], tr[_lib.TR_COUNT:_lib.TR_COUNT + 3])
    ev = eng.evaluate(db).cpu().numpy()
    assert int(ev[:, _lib.EV_TP].sum() + ev[:, _lib.EV_TN].sum()) == want
    _errlog.record("C:%s:count" % route, want, 0.0, parts=[lo, hi, top])


def _count_main(rank, world, port, out_dir):
    from hdgnn.engine import Engine
    _init(rank, world, port)
    c = T.C_CASES[0]
    cb, flat = T.c_inputs(c)
    bl = c.B // world
    eng = Engine(c.ne, c.nc, bl, variant=c.variant, batch_global=c.B,
                 process_group=torch.distributed.group.WORLD, allreduce="xgmi")
    assert eng.allreduce_kind == "xgmi"
    eng.set_params(flat)
    db = eng.upload(cb.slice(rank * bl, (rank + 1) * bl))
    eng.fwd_bwd(db)                                   # this rank's own count (grad_local)
    torch.cuda.synchronize()
    local = _lib.trailer_count(eng.grad_local[eng.np:].cpu().numpy())
    eng.train_step(db)
    torch.cuda.synchronize()
    eng.check_status()
    np.savez(os.path.join(out_dir, "count%d.npz" % rank), local=local,
             trailer=eng.grad[eng.np:].cpu().numpy(), stats=eng.stats.cpu().numpy())
    eng.xgmi.close()
    torch.distributed.destroy_process_group()


def test_count_two_ranks_carry(tmp_path):
    """Each rank takes 4 of the 8 commits; the ranks' low parts sum past 2^16, so putting the
    world's count together carries from the first part into the second."""
    from hdgnn.engine import Engine
    world = 2
    mp.spawn(_count_main, args=(world, _port(), str(tmp_path)), nprocs=world, join=True)
    r = [np.load(os.path.join(tmp_path, "count%d.npz" % k)) for k in range(world)]
    c = T.C_CASES[0]
    cb, flat = T.c_inputs(c)
    eng = Engine(c.ne, c.nc, c.B, variant=c.variant, path=PATHS[c.path])
    eng.set_params(flat)
    eng.train_step(eng.upload(cb))
    torch.cuda.synchronize()
    want = eng.correct_count()
    assert want == metrics.top_acc_count(onehot_relations(cb.y), eng.probs.cpu().numpy())
    locals_ = [int(x["local"]) for x in r]
    assert sum(locals_) == want
    assert sum(x & 0xFFFF for x in locals_) >= 1 << 16
    for x in r:
        assert _lib.trailer_count(x["trailer"]) == want
        assert _stats_count(x["stats"], one_rank=False) == want
        assert np.array_equal(x["trailer"], r[0]["trailer"])
