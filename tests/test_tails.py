"""The step tails' tables and bounds (tests/_tails.py) on the CPU, reference only: the TF-exact
mode of oracle.model_ref.AdamTF, the float32 beta-power recurrence, every group A population
against its definition, every table entry against its guards, and that the bounds bite --
each mutation of the reference moves a result by >= 50 bounds where it is meant to.  A
float32 emulation of the kernel's statement (both lr_t associations) stays inside the bound.
No engine."""
import math

import numpy as np
import pytest

from hdgnn import layout, metrics
from hdgnn.data import onehot_relations
from hdgnn.synth import synth_commits
from oracle import model_ref
from tests import _regimes as R
from tests import _tails as T
from tests.test_general_gpu import _reg_grad
from tests.test_param_regimes import check_well_conditioned

f32 = np.float32


# ----------------------------------------------------------------------------
# the reference
# ----------------------------------------------------------------------------
def test_default_mode_is_unchanged():
    """The other suites' AdamTF: the default arithmetic, bit for bit, over three steps."""
    rng = np.random.default_rng(0)
    n = 64
    theta, opt = rng.standard_normal(n), model_ref.AdamTF(n)
    th, m, v, p1, p2 = theta.copy(), np.zeros(n), np.zeros(n), f32(0.9), f32(0.999)
    for _ in range(3):
        g = rng.standard_normal(n)
        theta = opt.step(theta, g)
        lr_t = 3e-4 * math.sqrt(1 - float(p2)) / (1 - float(p1))
        m = 0.9 * m + (1 - 0.9) * g
        v = 0.999 * v + (1 - 0.999) * g * g
        th = th - lr_t * m / (np.sqrt(v) + 1e-8)
        p1, p2 = f32(p1 * f32(0.9)), f32(p2 * f32(0.999))
        assert np.array_equal(theta, th) and np.array_equal(opt.m, m)
        assert np.array_equal(opt.v, v) and (opt.b1p, opt.b2p) == (p1, p2)
    assert not opt.exact


def test_exact_mode_constants():
    opt = model_ref.AdamTF(4, lr=1e-3, exact=True)
    assert opt.lr == float(f32(1e-3)) and opt.b1 == float(f32(0.9))
    assert opt.b2 == float(f32(0.999)) and opt.eps == float(f32(1e-8))
    assert opt.omb1 == 1 - float(f32(0.9)) == T.OMB1         # exact in float32 (Sterbenz)
    assert opt.omb2 == 1 - float(f32(0.999)) == T.OMB2
    assert 1.28e-8 < 0.001 - opt.omb2 < 1.30e-8               # 1.3e-5 of 0.001
    assert T.REG_W == float(f32(0.001)) != 0.001


@pytest.mark.parametrize("case", T.A_CASES[::5], ids=T.a_id)
def test_ref_step_is_adamtf_exact(case):
    d = T.build_a(case)
    opt = model_ref.AdamTF(d["n"], lr=case.lr, exact=True)
    opt.m, opt.v = d["m"].astype(np.float64), d["v"].astype(np.float64)
    opt.b1p, opt.b2p = d["bpow"]
    got = opt.step_raw(d["w"].astype(np.float64), d["g"].astype(np.float64))
    want = T.a_reference(case, d)
    for a, b in zip(got, want):
        assert np.array_equal(a, b)


def test_beta_power_recurrence():
    tiny = np.finfo(f32).tiny
    p = {t: T.beta_powers(t) for t in T.STATES}
    assert p[1] == (f32(0.9), f32(0.999)) and p[2] == (f32(f32(0.9) * f32(0.9)),
                                                       f32(f32(0.999) * f32(0.999)))
    q1, q2 = f32(0.9), f32(0.999)
    for _ in range(49):
        q1, q2 = f32(q1 * f32(0.9)), f32(q2 * f32(0.999))
    assert p[50] == (q1, q2)
    for t in T.STATES:
        assert p[t][0].dtype == np.float32 and p[t][1].dtype == np.float32
        assert p[t][0] > 0 and p[t][1] > 0                   # never 0, as 0.9 ** t would say
    assert p[200][0] > tiny and 0 < p[830][0] < tiny          # b1p denormal at 830
    assert f32(p[830][0] * f32(0.9)) != p[830][0]             # ... and still moving
    assert f32(p[1000][0] * f32(0.9)) == p[1000][0] < 1e-44   # stuck
    assert p[1000][1] > 0.3
    assert tiny < p[87000][1] < 1.4 * tiny                    # the last normal values
    assert 0 < p[87400][1] < tiny and f32(p[87400][1] * f32(0.999)) != p[87400][1]
    assert f32(p[120000][1] * f32(0.999)) == p[120000][1]     # both stuck
    assert p[120000][0] == p[1000][0] != p[120000][1]
    assert T.lr_factor(*p[120000]) == 1.0                     # lr_t = lr exactly
    assert T.lr_factor(*p[87000]) == 1.0
    assert abs(T.lr_factor(*p[1]) - 0.3162) < 1e-3


# ----------------------------------------------------------------------------
# group A
# ----------------------------------------------------------------------------
def test_a_table_is_the_issue_matrix():
    assert [layout.n_params(v) for v in (1, 2, 3, 4)] == [1146, 2127, 2148, 3129]
    assert len(T.A_CASES) == 36 and len({T.a_id(c) for c in T.A_CASES}) == 36
    assert {(c.variant, c.t) for c in T.A_CASES} == {(v, t) for v in (1, 2, 3, 4)
                                                     for t in T.STATES}
    # every variant and every state meets every learning rate; every norm is used
    for v in (1, 2, 3, 4):
        assert {c.lr for c in T.A_CASES if c.variant == v} == set(T.LRS)
    for t in T.STATES:
        assert {c.lr for c in T.A_CASES if c.t == t} == set(T.LRS)
    assert {c.norm for c in T.A_CASES} == set(T.NORMS)
    assert set(T.MOVED) <= {(c.variant, c.t) for c in T.A_CASES}
    # every 16-slot group, wave and 1024-stride holds every population
    pop = T.pops_of(3129)
    for lo in range(0, 3104, 16):
        assert set(pop[lo:lo + 16]) == set(T.POPS)
    assert (pop[-4:] == T.THETA).all()


@pytest.mark.parametrize("case", T.A_CASES, ids=T.a_id)
def test_a_populations_are_what_they_claim(case):
    d = T.build_a(case)
    pop, w, g, m, v = d["pop"], d["w"], d["g"], d["m"], d["v"]
    for a in (w, g, m, v):
        assert a.dtype == np.float32 and np.isfinite(a).all()
    assert (v >= 0).all()
    w1, m1, v1, p1, p2 = T.a_reference(case, d)
    for a in (w1, m1, v1):                       # no result leaves float32's range
        assert np.isfinite(a.astype(np.float32)).all()
    if case.t < 830:
        assert (p1, p2) == T.beta_powers(case.t + 1)
    k = pop == "fresh"
    assert (m[k] == 0).all() and (v[k] == 0).all() and (g[k] != 0).all()
    assert (w[k] == 0).any() and (w[k] != 0).any()
    k = pop == "typical"
    assert (np.abs(g[k]) >= 0.99e-6).all() and (np.abs(g[k]) <= 1).all()
    assert (m[k] != 0).all() and (v[k] > 0).all()
    k = pop == "eps"
    s = np.sqrt(v1[k])
    assert (w[k] == 0).all() and (s >= 0.99e-9).all() and (s <= 1.01e-7).all()
    assert s.min() < T.EPS < s.max()                          # both sides of eps
    k = pop == "zero"
    for a in (w, g, m, v, w1, m1, v1):
        assert (a[k] == 0).all()
    k = pop == "cancel"
    gg = g[k].astype(np.float64) + T.REG_W * w[k]
    assert (np.sign(gg) == -np.sign(m[k])).all()
    assert (np.abs(m1[k]) <= 1e-3 * np.abs(m[k])).all()
    k = pop == "large"
    gg = g[k].astype(np.float64) + T.REG_W * w[k]
    assert np.abs(g[k]).max() > 1e13 and np.abs(g[k]).max() <= 1e15
    assert np.abs(w[k]).max() <= 3e4 and (gg * gg).max() < 1e31
    k = pop == "denormal"
    tiny = np.finfo(f32).tiny
    assert (np.abs(m[k]) < tiny).all() and (m[k] != 0).all()
    assert (v[k] < tiny).all() and (v[k] > 0).all()
    n1, n2 = T.theta_norms(w)
    assert abs(n1 / case.norm - 0.8) < 1e-3 and abs(n2 / case.norm - 1.3) < 1e-3
    assert {np.sign(x) for x in w[-4:-2]} == {-1.0, 1.0} == {np.sign(x) for x in w[-2:]}
    assert d["trailer"][2] >= 1 and d["trailer"][4] == 0


def _emulate32(d, left_to_right):
    """adam_tf.h's statement in float32 on the host, lr_t in either association."""
    w, g, m0, v0 = d["w"], d["g"], d["m"], d["v"]
    n = d["n"]
    c, lr = f32(0.001), f32(d["lr"])
    n1 = np.sqrt(f32(w[n - 4] * w[n - 4]) + f32(w[n - 3] * w[n - 3]))
    n2 = np.sqrt(f32(w[n - 2] * w[n - 2]) + f32(w[n - 1] * w[n - 1]))
    gg = g + c * w
    gg[n - 4:n - 2] += c * w[n - 4:n - 2] / n1
    gg[n - 2:] += c * w[n - 2:] / n2
    m = m0 + (gg - m0) * (f32(1) - f32(0.9))
    v = v0 + (gg * gg - v0) * (f32(1) - f32(0.999))
    b1p, b2p = d["bpow"]
    if left_to_right:
        lr_t = f32(lr * np.sqrt(f32(1) - b2p)) / (f32(1) - b1p)
    else:
        lr_t = lr * f32(np.sqrt(f32(1) - b2p) / (f32(1) - b1p))
    w1 = w - lr_t * m / (np.sqrt(v) + f32(1e-8))
    for a in (w1, m, v):
        assert a.dtype == np.float32
    return w1, m, v


@pytest.mark.parametrize("case", T.A_CASES, ids=T.a_id)
def test_a_bound_holds_float32_statement_and_bites(case):
    d = T.build_a(case)
    ref = T.a_reference(case, d)
    bound = T.a_bound(case, d)
    for b in bound:
        assert np.isfinite(b).all() and (b[d["pop"] != "zero"] > 0).all()
        assert (b[d["pop"] == "zero"] <= 2 * np.finfo(f32).smallest_subnormal).all()
    # the statement itself, rounded to float32 at every operation, is inside the bound
    got = [_emulate32(d, ltr) for ltr in (True, False)]
    for out in got:
        for k in range(3):
            err = np.abs(out[k].astype(np.float64) - ref[k])
            assert (err <= bound[k]).all(), "%s: %.3g bounds" % ("wmv"[k], (err / bound[k]).max())
    # ... and the two associations within the stated width of each other
    step = np.abs(d["w"].astype(np.float64) - ref[0])
    width = T.ASSOC_REL * step + T.spacing32(ref[0])
    assert (np.abs(got[0][0].astype(np.float64) - got[1][0]) <= width).all()
    # every mutation the case claims moves a result by >= BITE bounds on its population
    for mut in T.MUTATIONS:
        if not T.claims(mut, case.t, d["lr"]):
            continue
        mutd = T.a_reference(case, d, mut)
        if not T.MUT_POPS[mut]:
            assert (mutd[3], mutd[4]) != (ref[3], ref[4]), mut
            continue
        slots = np.isin(d["pop"], T.MUT_POPS[mut])
        r = T.bite(ref, mutd, bound, slots)
        assert r >= T.BITE, "%s moves %s by only %.3g bounds" % (mut, T.MUT_POPS[mut], r)
    if d["lr"] == 0:
        assert np.array_equal(ref[0], d["w"].astype(np.float64))   # parameters frozen


# ----------------------------------------------------------------------------
# group B
# ----------------------------------------------------------------------------
def test_b_table_is_the_issue_matrix():
    assert len(T.B_CASES) == 24 and len({T.b_id(c) for c in T.B_CASES}) == 24
    for sh in T.B_SHAPES:
        cs = [c for c in T.B_CASES if (c.B, c.ne, c.nc) == sh]
        assert {(c.route, c.path, c.variant) for c in cs} == {
            ("step", "fused", 2), ("step", "fused", 4), ("step", "general", 1),
            ("step", "general", 2), ("step", "general", 3), ("step", "general", 4),
            ("calls", "fused", 2), ("calls", "general", 4), ("dp", "fused", 2),
            ("dps", "fused", 2), ("dp", "general", 2)}
        assert {c.split for c in cs if (c.route, c.path, c.variant) == ("step", "fused", 2)} \
            == {"0", "1"}
    assert {(c.t, c.lr) for c in T.B_CASES} == {(t, lr) for t in (200, 1000)
                                                for lr in (3e-4, 1e-3)}


@pytest.mark.parametrize("entry", T.b_entries(), ids=lambda e: "v%d-%dx%dx%d" % e[:4])
def test_b_entry_is_well_conditioned_and_bites(entry):
    """The regimes' three guards (kink <= 0.5 of the tolerance, max |logit| <= 1e4, float32 CE
    to 5e-6) at the case's parameters and at the parameters its first step leaves, and
    mutations 2-5 at >= 50 propagated bounds, on both steps of every case of the entry."""
    v, B, ne, nc, dseed, pseed, fused = entry
    cb = synth_commits(B, ne, nc, dseed)
    flat = R.regime_flat("trained", pseed, v)
    cases = [c for c in T.B_CASES if (c.variant, c.B, c.ne, c.nc) == (v, B, ne, nc)]
    assert cases
    _, g0 = check_well_conditioned(flat, cb, v, fused)
    m0, v0 = T.b_state(g0, v, pseed)
    for t, lr in sorted({(c.t, c.lr) for c in cases}):
        w, m, vv, (p1, p2), g = flat, m0, v0, T.beta_powers(t), g0
        for step in (1, 2):
            g_red = g - _reg_grad(w)
            tol = T.b_grad_tol(g, v, fused)
            ref = T.ref_step(w, g_red, m, vv, p1, p2, lr)
            bound = T.grad_bound(w.astype(np.float64), g_red, tol, m, vv, p1, p2, lr)
            every = np.ones(len(w), bool)
            for mut in ("lr_fresh", "lr_plain", "m0_zero", "v0_zero"):
                r = T.bite(ref, T.ref_step(w, g_red, m, vv, p1, p2, lr, mut), bound, every)
                assert r >= T.BITE, "t=%d lr=%g step %d: %s only %.3g bounds" % (t, lr, step,
                                                                                 mut, r)
            if step == 1:          # the state the second step starts from
                w, m, vv = (a.astype(np.float32) for a in ref[:3])
                p1, p2 = ref[3], ref[4]
                _, g = check_well_conditioned(w, cb, v, fused)


# ----------------------------------------------------------------------------
# group C
# ----------------------------------------------------------------------------
def c_oracle(c):
    """-> (count, relations, near ties) of the float64 oracle on the case's inputs."""
    cb, flat = T.c_inputs(c)
    P = model_ref.to_torch_params(model_ref.unflatten(flat.astype(np.float64), c.variant),
                                  requires_grad=False)
    out = model_ref.forward(P, cb.x.astype(np.float64), cb.a, cb.y, cb.hid, cb.nlen, c.variant)
    z = out["logits"].numpy()
    p = out["probs"].numpy().transpose(0, 2, 1)
    scale = np.abs(z).reshape(c.B, -1).max(1)[:, None]
    near = int((np.abs(z[..., 1] - z[..., 0]) < T.NEAR_TIE * scale).sum())
    return metrics.top_acc_count(onehot_relations(cb.y), p), z.shape[0] * z.shape[1], near


@pytest.mark.parametrize("case", T.C_CASES, ids=T.c_id)
def test_c_count_needs_its_second_part(case):
    count, nrel, near = c_oracle(case)
    assert nrel == case.B * case.nc * (case.nc - 1)
    lo, hi, top = T.count_parts(count)
    assert count >= T.COUNT_MIN and hi >= 1 and lo != 0 and top == 0
    assert near <= T.NEAR_MAX * nrel
    assert count + near < nrel            # not everything right: a real count, not the total


def test_c_two_rank_halves_carry():
    """The two-rank case: commits 0-3 and 4-7 of the fused model_2 entry; the ranks' low
    parts must sum to >= 2^16 so that reassembling the world's count carries."""
    c = T.C_CASES[0]
    cb, flat = T.c_inputs(c)
    lows = []
    for r in range(2):
        sh = cb.slice(4 * r, 4 * r + 4)
        P = model_ref.to_torch_params(model_ref.unflatten(flat.astype(np.float64), 2),
                                      requires_grad=False)
        out = model_ref.forward(P, sh.x.astype(np.float64), sh.a, sh.y, sh.hid, sh.nlen, 2)
        p = out["probs"].numpy().transpose(0, 2, 1)
        lows.append(metrics.top_acc_count(onehot_relations(sh.y), p) & 0xFFFF)
    assert sum(lows) >= 1 << 16, lows
