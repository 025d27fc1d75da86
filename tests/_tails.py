"""What ends a training step, off a fresh start: case tables, state and gradient builders, the
TF-exact reference and the bounds of tests/test_tails.py (CPU) and tests/test_tails_gpu.py.

Three groups:

  A  TF1 ApplyAdam (csrc/adam_tf.h) on a chosen gradient and a chosen state, through
     hdg_adam_tf and the world-of-one hdg_adam_dp (both flag values), against
     oracle.model_ref.AdamTF(exact=True).  Inputs are exact float32, so only the kernel's
     own roundings separate the two: op_bound() below counts them.
  B  the tails that take their gradient from the step (hdg_train_step, hdg_fwd_bwd +
     hdg_adam_tf, the world-of-one hdg_train_step_dp) at a trained state; the gradient
     carries the parity suites' tolerance, pushed through the reference by corners.
  C  correct-prediction counts above 2^16, so the trailer's second 16-bit part is used.

No tolerance here comes from a GPU run.  u = 2^-24 is float32's unit roundoff; an operation
the device may round to 1 ulp instead of correctly (sqrtf, the division) is counted as 2u.
"""
import functools
import math
from collections import namedtuple

import numpy as np

from hdgnn import layout
from oracle import model_ref

U = 2.0 ** -24
FLT_MIN = float(np.finfo(np.float32).tiny)
BITE = 50.0                       # a mutation must move a result by this many bounds

# ----------------------------------------------------------------------------
# the reference: TF's kernel to the letter, with optional mutations
# ----------------------------------------------------------------------------
B1, B2, EPS = (float(np.float32(c)) for c in (0.9, 0.999, 1e-8))
OMB1 = float(np.float32(1) - np.float32(0.9))       # T(1) - beta1, formed in float32
OMB2 = float(np.float32(1) - np.float32(0.999))     # 1.29e-8 below 0.001
REG_W, REG_TH = float(model_ref.AdamTF.REG_W), float(model_ref.AdamTF.REG_TH)

MUTATIONS = (
    "eps_in_root",     # 1. sqrt(v + eps)           in place of sqrt(v) + eps
    "eps2_in_root",    # 1. sqrt(v + eps^2)
    "lr_fresh",        # 2. lr_t from the fresh powers (0.9, 0.999) instead of the state's
    "lr_plain",        # 3. lr_t = lr
    "m0_zero",         # 4. m0 read as 0
    "v0_zero",         # 5. v0 read as 0
    "v_no_reg",        # 6. v fed g without the regulariser terms
    "no_l2",           # 7. the 0.001 w term missing
    "no_theta",        # 8. the theta term missing
    "theta_shift",     # 8. the theta term on slots shifted by one pair (TH1 taking |theta2|)
    "pow_stay",        # 9. beta powers not advanced
    "pow_swap",        # 9. the two beta powers written to each other's slot
    "omb2_double",     # 10. 1 - beta2 taken as the double 0.001
)


@functools.lru_cache(maxsize=None)
def beta_powers(t):
    return model_ref.AdamTF.beta_powers(t)


def lr_factor(b1p, b2p):
    return math.sqrt(1 - float(b2p)) / (1 - float(b1p))


def theta_norms(w):
    n = len(w)
    return (math.sqrt(float(w[n - 4]) ** 2 + float(w[n - 3]) ** 2),
            math.sqrt(float(w[n - 2]) ** 2 + float(w[n - 1]) ** 2))


def theta_term(w, swap=False):
    """0.001f theta / |theta| on the last four slots, 0 elsewhere."""
    w = np.asarray(w, np.float64)
    n = len(w)
    n1, n2 = theta_norms(w)
    if swap:
        n1, n2 = n2, n1
    t = np.zeros(n)
    t[n - 4:n - 2] = REG_TH * w[n - 4:n - 2] / n1
    t[n - 2:] = REG_TH * w[n - 2:] / n2
    return t


def ref_step(w, g, m0, v0, b1p, b2p, lr, mut=None):
    """TF1 ApplyAdam of the reduced gradient g (without the regularisers, as the tail gets
    it) in float64 on float32 inputs -> (w', m', v', b1p', b2p').  mut: one of MUTATIONS.
    mut=None is oracle.model_ref.AdamTF(exact=True).step_raw bit for bit
    (tests/test_tails.py)."""
    assert mut is None or mut in MUTATIONS
    w, g, m0, v0 = (np.asarray(a, np.float64) for a in (w, g, m0, v0))
    lr = float(np.float32(lr))
    reg = (0.0 if mut == "no_l2" else REG_W * w)
    if mut != "no_theta":
        reg = reg + theta_term(w, swap=mut == "theta_shift")
    gg = g + reg
    if mut == "m0_zero":
        m0 = np.zeros_like(m0)
    if mut == "v0_zero":
        v0 = np.zeros_like(v0)
    p1, p2 = (B1, B2) if mut == "lr_fresh" else (float(b1p), float(b2p))
    lr_t = lr if mut == "lr_plain" else lr * math.sqrt(1 - p2) / (1 - p1)
    gv = g if mut == "v_no_reg" else gg
    m = m0 + (gg - m0) * OMB1
    v = v0 + (gv * gv - v0) * (0.001 if mut == "omb2_double" else OMB2)
    if mut == "eps_in_root":
        den = np.sqrt(v + EPS)
    elif mut == "eps2_in_root":
        den = np.sqrt(v + EPS * EPS)
    else:
        den = np.sqrt(v) + EPS
    w1 = w - lr_t * m / den
    n1p = np.float32(np.float32(b1p) * np.float32(0.9))
    n2p = np.float32(np.float32(b2p) * np.float32(0.999))
    if mut == "pow_stay":
        n1p, n2p = np.float32(b1p), np.float32(b2p)
    if mut == "pow_swap":
        n1p, n2p = n2p, n1p
    return w1, m, v, n1p, n2p


# ----------------------------------------------------------------------------
# the operator's forward error bound
# ----------------------------------------------------------------------------
# lr_t.  k_adam_tf: fl(fl(lr fl(sqrt(fl(1 - b2p)))) / fl(1 - b1p)): the difference u, halved by
# the root (u/2), the root 2u, the product u, the other difference u, the quotient 2u: 6.5u.
# Every other site: lr fl(fl(sqrt(fl(1 - b2p))) / fl(1 - b1p)): u/2 + 2u + u + 2u, then the
# product u: 6.5u as well.  Both fit 7u.
LRT_REL = 7 * U
# so the two associations lie within 13u of each other.  The step fl(fl(lr_t m) / D) adds 3u
# to either (product u, quotient 2u): the steps differ by <= 19u, rounded up to 20u, and the
# stored parameters fl(w - step) by that plus one spacing (each rounds by half of one).
ASSOC_REL = 20 * U
# |theta|: two squares (u each) and their sum (u) leave the sum within 2u, its root within u,
# and the root itself rounds by <= 2u: 3u, taken as 4u for the second-order terms.
NORM_REL = 4 * U
# theta term fl(fl(0.001f w) / n): product u, quotient 2u, n NORM_REL: 7u, taken as 8u.
THETA_REL = 8 * U
# the step's own operations: fl(sqrt) 2u, + eps u, lr_t m u, the quotient 2u
STEP_REL = 6 * U


def spacing32(x):
    return np.spacing(np.abs(np.asarray(x, np.float64)).astype(np.float32)).astype(np.float64)


def op_bound(w, g, m0, v0, b1p, b2p, lr, dg=0.0, floor=None):
    """Bounds (bw, bm, bv) on |kernel - ref_step| for float32 inputs; dg: an uncertainty of
    the gradient itself on top (group B: the parity suites' tolerance); floor: slots whose
    moments get FLT_MIN on top (a runtime that flushes denormals)."""
    w, g, m0, v0 = (np.asarray(a, np.float64) for a in (w, g, m0, v0))
    lr = float(np.float32(lr))
    cw = REG_W * w
    term = theta_term(w)
    gg = g + cw + term
    # gg: fl(c w) (u |cw|), fl(g + .) (u |sum|); a theta slot adds the term's own error and
    # one more sum.  |sum| <= sum of the magnitudes; adding an exact 0 (w = 0) rounds nothing.
    dgg = dg + U * np.abs(cw) + np.where(cw != 0, U * (np.abs(g) + np.abs(cw)), 0.0)
    dgg = dgg + np.where(term != 0, THETA_REL * np.abs(term)
                         + U * (np.abs(g) + np.abs(cw) + np.abs(term)), 0.0)
    # m' = fl(m0 + fl(fl(gg - m0) c1))
    d = gg - m0
    dd = dgg + U * np.abs(d)
    dx = dd * OMB1 + U * np.abs(d) * OMB1
    m1 = m0 + d * OMB1
    bm = dx + U * np.abs(m1)
    # v' = fl(v0 + fl(fl(fl(gg gg) - v0) c2))
    q = gg * gg
    dq = 2 * np.abs(gg) * dgg + dgg * dgg + U * q
    e = q - v0
    de = dq + U * np.abs(e)
    dy = de * OMB2 + U * np.abs(e) * OMB2
    v1 = v0 + e * OMB2
    bv = dy + U * np.abs(v1)
    if floor is not None:
        bm = bm + np.where(floor, FLT_MIN, 0.0)
        bv = bv + np.where(floor, FLT_MIN, 0.0)
    # the step by corners: sqrt near 0 and the eps regime are where derivatives lie
    lr_t = lr * lr_factor(b1p, b2p)
    f0 = lr_t * m1 / (np.sqrt(v1) + EPS)
    dev = np.zeros_like(f0)
    fmax = np.abs(f0)
    for mm in (m1 - bm, m1 + bm):
        for vv in (np.maximum(v1 - bv, 0.0), v1 + bv):
            for ll in (lr_t * (1 - LRT_REL), lr_t * (1 + LRT_REL)):
                f = ll * mm / (np.sqrt(vv) + EPS)
                dev = np.maximum(dev, np.abs(f - f0))
                fmax = np.maximum(fmax, np.abs(f))
    bw = dev + STEP_REL * fmax + 2 * spacing32(w - f0)
    return bw, bm, bv


def grad_bound(w, g, dg, m0, v0, b1p, b2p, lr):
    """Group B: the reference at g - dg, g, g + dg (corners of the gradient's tolerance) and
    op_bound at each; the largest deviation from the centre plus the largest operator bound."""
    c = ref_step(w, g, m0, v0, b1p, b2p, lr)
    out = [np.zeros_like(c[0]) for _ in range(3)]
    ops = [np.zeros_like(c[0]) for _ in range(3)]
    for gc in (g - dg, g, g + dg):
        r = ref_step(w, gc, m0, v0, b1p, b2p, lr)
        ob = op_bound(w, gc, m0, v0, b1p, b2p, lr)
        for k in range(3):
            out[k] = np.maximum(out[k], np.abs(r[k] - c[k]))
            ops[k] = np.maximum(ops[k], ob[k])
    return tuple(o + p for o, p in zip(out, ops))


# ----------------------------------------------------------------------------
# group A: states, populations, cases
# ----------------------------------------------------------------------------
# step counts: fresh, second, the trajectories' end, trained; b1p denormal (830), b1p stuck
# (1000), b2p at the edge of the normal range (87000: 1.6e-38, its products stay normal for
# another 294 steps) and inside the denormal range (87400), both stuck and lr_t = lr exactly
# (120000)
STATES = (1, 2, 50, 200, 830, 1000, 87000, 87400, 120000)
LRS = (3e-4, 1e-3, 0.0)
NORMS = (3e-3, 0.2, 40.0)
# population of slot p: POPS[p % 8] (every 16-slot group, wave and 1024-stride holds them
# all); the last four slots are thetas
POPS = ("fresh", "typical", "eps", "zero", "cancel", "large", "denormal", "typical")
THETA = "theta"

ACase = namedtuple("ACase", "variant t lr norm seed")

# Entries whose first seed failed a condition of tests/test_tails.py and moved to the next:
# (variant, t) -> seed, the reason in the comment.  None so far: every guard and every
# mutation held at the first seed of every entry.
MOVED = {}


def _a_table():
    T = []
    for vi, v in enumerate((1, 2, 3, 4)):
        for ti, t in enumerate(STATES):
            seed = MOVED.get((v, t), 9000 + 100 * v + ti)
            T.append(ACase(v, t, LRS[(vi + ti) % 3], NORMS[(vi + 2 * ti) % 3], seed))
    return T


A_CASES = _a_table()


def a_id(c):
    return "v%d-t%d-lr%g-n%g" % (c.variant, c.t, c.lr, c.norm)


def pops_of(n):
    """Population name of every slot of an n-parameter vector."""
    pop = np.array([POPS[p % 8] for p in range(n)], dtype=object)
    pop[n - 4:] = THETA
    return pop


def _logu(rng, lo, hi, n):
    return np.exp(rng.uniform(math.log(lo), math.log(hi), n))


def build_a(c):
    """The float32 inputs of a group A case: dict(w, g, m, v, bpow, pop, trailer, lr)."""
    n = layout.n_params(c.variant)
    rng = np.random.default_rng(c.seed)
    pop = pops_of(n)
    sign = lambda: rng.choice([-1.0, 1.0], n)                 # noqa: E731
    xi, xj = rng.standard_normal(n), rng.standard_normal(n)
    g = sign() * _logu(rng, 1e-6, 1.0, n)
    w = 0.1 * rng.standard_normal(n)
    m = g * (1 + 0.3 * xi)
    v = g * g * (1 + 0.3 * np.abs(xj))
    k = pop == "fresh"
    m[k], v[k] = 0.0, 0.0
    w[k & (np.arange(n) % 16 == 0)] = 0.0      # a fresh start's biases are exactly 0
    k = pop == "eps"           # sqrt(v') = s in [0.1, 10] x 1e-8, g^2 of v's own size
    s = _logu(rng, 1e-9, 1e-7, n)
    ge = sign() * s * rng.uniform(0.5, 1.5, n)
    w[k] = 0.0
    g[k] = ge[k]
    m[k] = (ge * (1 + 0.3 * xi))[k]
    v[k] = ((s * s - OMB2 * ge * ge) / (1 - OMB2))[k]
    k = pop == "zero"
    g[k] = w[k] = m[k] = v[k] = 0.0
    k = pop == "large"
    gl = sign() * _logu(rng, 1e3, 1e15, n)
    g[k] = gl[k]
    w[k] = (sign() * _logu(rng, 1.0, 3e4, n))[k]
    m[k] = (gl * (1 + 0.3 * xi))[k]
    v[k] = (gl * gl * (1 + 0.3 * np.abs(xj)))[k]
    k = pop == "denormal"
    g[k] = w[k] = 0.0
    m[k] = (sign() * _logu(rng, 1e-45, 1e-39, n))[k]
    v[k] = _logu(rng, 1e-45, 1e-39, n)[k]
    # thetas: |theta1| = 0.8 norm, |theta2| = 1.3 norm, mixed signs; small gradients
    a1, a2 = rng.uniform(0.3, 1.2, 2)
    w[n - 4:] = [0.8 * c.norm * math.cos(a1), -0.8 * c.norm * math.sin(a1),
                 -1.3 * c.norm * math.cos(a2), 1.3 * c.norm * math.sin(a2)]
    gt = sign()[:4] * _logu(rng, 1e-5, 1e-2, 4)
    g[n - 4:] = gt
    m[n - 4:] = gt * (1 + 0.3 * xi[:4])
    v[n - 4:] = gt * gt * (1 + 0.3 * np.abs(xj[:4]))
    w, g, v = w.astype(np.float32), g.astype(np.float32), v.astype(np.float32)
    # cancel: m' = m0 (1 - c1) + gg c1 = 0 up to m0's own rounding
    k = pop == "cancel"
    gg = g.astype(np.float64) + REG_W * w.astype(np.float64)
    m[k] = (-gg * OMB1 / (1 - OMB1))[k]
    m = m.astype(np.float32)
    b1p, b2p = beta_powers(c.t)
    # trailer: CE sum, a count above 2^16 in its parts, no fault
    trailer = np.zeros(8, np.float32)
    trailer[0] = np.float32(rng.uniform(5.0, 500.0))
    trailer[1], trailer[2] = 4321.0 + c.t % 7, 3.0
    return dict(w=w, g=g, m=m, v=v, bpow=np.array([b1p, b2p], np.float32), pop=pop,
                trailer=trailer, lr=float(np.float32(c.lr)), n=n)


def a_reference(c, d=None, mut=None):
    d = d or build_a(c)
    return ref_step(d["w"], d["g"], d["m"], d["v"], d["bpow"][0], d["bpow"][1], d["lr"], mut)


def a_bound(c, d=None):
    d = d or build_a(c)
    return op_bound(d["w"], d["g"], d["m"], d["v"], d["bpow"][0], d["bpow"][1], d["lr"],
                    floor=d["pop"] == "denormal")


# which populations a mutation is meant for, and which cases claim it.  lr = 0 freezes the
# parameters, so the mutations that only move theta' claim lr > 0; lr_plain equals the truth
# once both powers are denormal (sqrt(1 - b2p) / (1 - b1p) = 1 exactly, t >= 87000);
# lr_fresh equals it at t = 1; pow_stay equals it once both powers are stuck (t = 120000).
MUT_POPS = {
    "eps_in_root": ("eps",), "eps2_in_root": ("eps",),
    "lr_fresh": ("typical",), "lr_plain": ("typical",),
    "m0_zero": ("typical",), "v0_zero": ("typical",),
    "v_no_reg": ("typical",), "no_l2": ("typical",),
    "no_theta": (THETA,), "theta_shift": (THETA,),
    "pow_stay": (), "pow_swap": (),            # the powers themselves: any change bites
    "omb2_double": ("fresh",),
}


def claims(mut, t, lr):
    if mut in ("eps_in_root", "eps2_in_root"):
        return lr > 0
    if mut == "lr_fresh":
        return lr > 0 and t > 1
    if mut == "lr_plain":
        return lr > 0 and t <= 1000
    if mut == "pow_stay":
        return t < 120000
    return True


def bite(ref, mutd, bound, slots):
    """Largest |mutated - reference| / bound over theta', m', v' on the given slots."""
    worst = 0.0
    for k in range(3):
        dlt = np.abs(mutd[k] - ref[k])[slots]
        b = bound[k][slots]
        ok = dlt > 0
        if ok.any():
            with np.errstate(divide="ignore"):
                worst = max(worst, float((dlt[ok] / b[ok]).max()))
    return worst


# ----------------------------------------------------------------------------
# group B: the tails behind a step
# ----------------------------------------------------------------------------
# route: which entry points end the step
#   step        hdg_train_step
#   calls       hdg_fwd_bwd then hdg_adam_tf
#   dp / dps    world-of-one hdg_train_step_dp, flags 0 / HDG_DP_SHARED
BCase = namedtuple("BCase", "route path variant split B ne nc t lr dseed pseed")
B_SHAPES = ((3, 7, 5), (2, 37, 19))
B_MOVED = {}          # (path, variant, B, ne, nc) -> (dseed, pseed); none moved so far


def _b_table():
    T = []

    def add(route, path, v, split, sh, k):
        key = (path, v) + sh
        d, p = B_MOVED.get(key, (300 + sh[1], 2000 + 10 * v + sh[1] % 7))
        T.append(BCase(route, path, v, split, sh[0], sh[1], sh[2], (200, 1000)[k % 2],
                       (3e-4, 1e-3)[(k // 2 + k) % 2], d, p))
    k = 0
    for sh in B_SHAPES:
        for split in ("1", "0"):
            add("step", "fused", 2, split, sh, k); k += 1          # k_reduce_adam
        add("step", "fused", 4, None, sh, k); k += 1               # kw_reduce_adam, fused rows
        for v in (1, 2, 3, 4):
            add("step", "general", v, None, sh, k); k += 1         # kw_reduce_adam
        add("calls", "fused", 2, None, sh, k); k += 1              # k_grad_reduce -> k_adam_tf
        add("calls", "general", 4, None, sh, k); k += 1            # kw_grad_reduce -> k_adam_tf
        add("dp", "fused", 2, None, sh, k); k += 1                 # k_dp_tail<PART>
        add("dps", "fused", 2, None, sh, k); k += 1                # k_dp_tail_shared<GRAD>
        add("dp", "general", 2, None, sh, k); k += 1               # wide_run -> hdg_adam_dp
    return T


B_CASES = _b_table()


def b_id(c):
    s = "%s-%s-v%d-%dx%dx%d-t%d-lr%g" % (c.route, c.path, c.variant, c.B, c.ne, c.nc, c.t, c.lr)
    return s + ("-split" + c.split if c.split is not None else "")


def b_entries():
    """Distinct (path is fused?, variant, B, ne, nc, dseed, pseed) the table needs from the
    oracle."""
    seen = {}
    for c in B_CASES:
        k = (c.variant, c.B, c.ne, c.nc, c.dseed, c.pseed)
        seen[k] = seen.get(k, False) or c.path == "fused"
    return [k + (f,) for k, f in seen.items()]


def b_state(g_ref, variant, seed):
    """Trained-state moments around the oracle's full gradient: m = g (1 + 0.3 xi),
    v = max(g^2, (1e-3 max|g| of the variable)^2) (1 + 0.3 |xi|), float32.  The floor keeps
    the step's sensitivity to the gradient tolerance bounded, as an accumulated v does."""
    rng = np.random.default_rng(seed)
    n = len(g_ref)
    m = g_ref * (1 + 0.3 * rng.standard_normal(n))
    fl = np.zeros(n)
    for _, (o, shape) in layout.offsets(variant).items():
        k = int(np.prod(shape))
        fl[o:o + k] = 1e-3 * np.abs(g_ref[o:o + k]).max()
    v = np.maximum(g_ref * g_ref, fl * fl) * (1 + 0.3 * np.abs(rng.standard_normal(n)))
    return m.astype(np.float32), v.astype(np.float32)


def b_grad_tol(g_ref, variant, fused):
    """The suites' gradient tolerance per element of the flat vector (tests/_regimes.grad_tol
    per variable)."""
    from tests import _regimes as R
    tol = np.zeros(len(g_ref))
    for _, (o, shape) in layout.offsets(variant).items():
        k = int(np.prod(shape))
        tol[o:o + k] = R.grad_tol(g_ref[o:o + k], fused)
    return tol


def reg_exact(w):
    """The regularisers' gradient with adam_tf.h's float32 factors (what ref_step adds)."""
    w = np.asarray(w, np.float64)
    return REG_W * w + theta_term(w)


# ----------------------------------------------------------------------------
# group C: counts with a second 16-bit part
# ----------------------------------------------------------------------------
CCase = namedtuple("CCase", "path variant split B ne nc dseed pseed")
C_MOVED = {}          # (path, variant, B, ne, nc) -> (dseed, pseed); none moved so far
COUNT_MIN = (1 << 16) + 1000
NEAR_TIE = 1e-5       # of the commit's largest |logit|: the suites' logit tolerance
NEAR_MAX = 0.01       # at most this share of the relations that close to a tie


def _c_table():
    T = []

    def add(path, v, split, sh):
        d, p = C_MOVED.get((path, v) + sh, (1, 1))
        T.append(CCase(path, v, split, sh[0], sh[1], sh[2], d, p))
    add("fused", 2, "1", (8, 8, 160))
    add("fused", 2, "0", (8, 8, 160))
    add("fused", 4, None, (8, 8, 160))
    add("general", 1, None, (3, 8, 257))
    add("general", 4, None, (3, 8, 257))
    return T


C_CASES = _c_table()


def c_id(c):
    s = "%s-v%d-%dx%dx%d" % (c.path, c.variant, c.B, c.ne, c.nc)
    return s + ("-split" + c.split if c.split is not None else "")


def c_inputs(c):
    from hdgnn.synth import synth_commits
    cb = synth_commits(c.B, c.ne, c.nc, c.dseed, hdensity=0.5)
    return cb, layout.init_flat(c.pseed, c.variant)


def count_parts(count):
    return count & 0xFFFF, (count >> 16) & 0xFFFF, count >> 32
