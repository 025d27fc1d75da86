"""Parameters off the initialiser at which every stage of the model reaches the loss, the
guard that says so, and the parity case table built on them.

The `trained` regime of tests/_regimes.py (N(0, 0.1) on every variable) leaves the entity
stage dead on a third of that table: mlp2_entity_B1 ends in a relu, and where its trained
parameters put x' = 0 on every node (rho = 0, tests/_ties.py ALIVE) no gradient reaches the
entity pair MLP and no entity bias moves a logit.  The engine then passes the gradient check
of the entity backward by multiplying with 0.  KNOWN_DEAD below pins those entries of the
four earlier tables; tests/test_live.py recomputes the set.

live_flat() is a regime that keeps the entity stage alive up to the fused path's largest
shapes:

  1. _regimes._trained(seed, variant);
  2. the E3 edit of _ties._alive (o1_b1o = 0.2, o1_b2o = 0.5, o1_w2o = |o1_w2o|): x' > 0;
  3. the second layer (weight and bias) of every pair MLP scaled in float32: E1's and, where
     the variant has it, EE's by s_e = min(1, 16 / Ne), H1's by s_c = min(1, 16 / Nc).  A node
     sums its pair MLP over 2 (Ne - 1) relations; without the scale a live x' at Ne >= 200
     drives max |logit| past the 1e4 the tolerances were set for.

A pure function of (seed, variant, Ne, Nc); it never produces an exact zero.  `degenerate` on
top of it is _regimes._degenerate(live_flat(...)).

check_live() holds an entry to three conditions with the float64 oracle alone (gradient
reach, unit reach, forward reach); CASES is the explicit list tests/test_live_gpu.py runs,
and tests/test_live.py holds every entry of it to check_live and to
test_param_regimes.check_well_conditioned.  Nothing here is searched at test time.
"""
import functools
from collections import namedtuple

import numpy as np

from hdgnn import layout
from hdgnn.synth import synth_commits
from oracle import model_ref
from tests import _regimes as R
from tests import _ties as T

REGIMES = ("live", "degenerate")
SCALE_AT = 16.0                      # s = min(1, SCALE_AT / N)

# ----------------------------------------------------------------------------
# the regime
# ----------------------------------------------------------------------------
# pair MLP -> which node count scales its second layer
PAIR_SCALE = {"E1": "ne", "EE": "ne", "H1": "nc"}


def second_layer(variant, key):
    """(weight, bias) names of the second layer of first layer `key` (a key of
    _regimes.first_layers): the two variables that follow its bias in layout order."""
    names = list(layout.offsets(variant))
    i = names.index(R.first_layers(variant)[key][1])
    w2, b2 = names[i + 1], names[i + 2]
    shapes = layout.offsets(variant)
    assert shapes[w2][1][0] == 20 and len(shapes[b2][1]) == 1, (w2, b2)
    return w2, b2


def scales(ne, nc):
    return (np.float32(min(1.0, SCALE_AT / ne)), np.float32(min(1.0, SCALE_AT / nc)))


def live_flat(seed, variant, ne, nc):
    """float32 flat parameter vector of the `live` regime (layout.offsets(variant) order)."""
    flat = R._trained(seed, variant)
    have = R.first_layers(variant)
    if "E3" in have:
        flat = T._alive(flat, variant)
    V = R.views(flat, variant)
    s = dict(zip(("ne", "nc"), scales(ne, nc)))
    for key, which in PAIR_SCALE.items():
        if key in have:
            for name in second_layer(variant, key):
                V[name][...] = V[name] * s[which]
    assert flat.dtype == np.float32 and (flat != 0).all()
    return flat


def regime_flat(name, seed, variant, ne, nc):
    flat = live_flat(seed, variant, ne, nc)
    if name == "degenerate":
        flat = R._degenerate(flat, variant)
    elif name != "live":
        raise ValueError("unknown regime %r" % (name,))
    return flat


# ----------------------------------------------------------------------------
# the liveness guard
# ----------------------------------------------------------------------------
GRAD_REACH = 1e-3        # max |g_data| of every variable
UNIT_REACH = 8           # hidden units of a first layer whose column carries a gradient
UNIT_FLOOR = 1e-6        # ... of at least this share of the variable's maximum
FORWARD_REACH = 50.0     # zeroing an entity bias moves the worst logit by this many tolerances
ENTITY_BIASES = ("phi_E_O1/r1_b1o:0", "phi_E_O1/r1_b5o:0", "phi_U_O1/o1_b1o:0",
                 "phi_U_O1/o1_b2o:0")
HUNK_BIASES = ("mlp_hunk_B2/b1:0", "mlp_hunk_B2/b2:0", "/C_edge_b1:0")     # reported only


def exempt(variant):
    """Variables that never reach the loss: the two thetas (the regulariser's alone), and
    model_3's entity-edge stage, computed and unused (B2 = B1)."""
    out = {n for n in layout.offsets(variant) if n.startswith("map_conv/")}
    if variant == 3:
        out |= {n for n in layout.offsets(variant)
                if n.startswith("phi_E_R1/") or n.startswith("phi_U_R1/")}
    return out


def data_grad(flat, g):
    """The oracle's gradient without the regularisers' part."""
    from tests.test_general_gpu import _reg_grad
    return np.asarray(g, np.float64) - _reg_grad(np.asarray(flat, np.float32))


def grad_reach(flat, g, variant):
    """{variable: max |g_data|} of the variables that have to reach the loss."""
    gd = data_grad(flat, g)
    skip = exempt(variant)
    return {n: float(np.abs(gd[o:o + int(np.prod(s))]).max())
            for n, (o, s) in layout.offsets(variant).items() if n not in skip}


def dead_variables(flat, g, variant):
    """The variables that miss the gradient-reach condition, with their max |g_data|."""
    return {n: m for n, m in grad_reach(flat, g, variant).items() if not m >= GRAD_REACH}


def unit_reach(flat, g, variant):
    """{first-layer weight: hidden units whose column maximum is >= UNIT_FLOOR of the
    variable's maximum}."""
    gd = data_grad(flat, g)
    skip = exempt(variant)
    offs = layout.offsets(variant)
    out = {}
    for key, (w, _) in R.first_layers(variant).items():
        for name in (w if isinstance(w, tuple) else (w,)):
            if name in skip:
                continue
            o, shape = offs[name]
            a = np.abs(gd[o:o + int(np.prod(shape))]).reshape(shape)
            assert shape[-1] == 20
            out[name] = int((a.max(0) >= UNIT_FLOOR * a.max()).sum()) if a.max() > 0 else 0
    return out


def _logits(flat64, cb, variant):
    P = model_ref.to_torch_params(model_ref.unflatten(flat64, variant), requires_grad=False)
    out = model_ref.forward(P, cb.x.astype(np.float64), cb.a, cb.y, cb.hid, cb.nlen, variant)
    return out["logits"].numpy().transpose(0, 2, 1)


def forward_reach(flat, cb, variant, fused, ref_logits, names):
    """{bias: worst |logit move| / logit tolerance when the bias is zeroed}.  ref_logits:
    the oracle's (B, Pc, 2)."""
    from tests._labels import logit_tol
    ref = np.asarray(ref_logits).transpose(0, 2, 1)
    tol = logit_tol(ref, fused)
    offs = layout.offsets(variant)
    out = {}
    for suffix in names:
        name = R._find(offs, suffix)
        if name is None:
            continue
        o, shape = offs[name]
        z = np.asarray(flat, np.float64).copy()
        z[o:o + int(np.prod(shape))] = 0.0
        out[name] = float((np.abs(_logits(z, cb, variant) - ref) / tol).max())
    return out


def check_live(flat, cb, variant, fused, ref=None):
    """The three liveness conditions on one (parameters, batch), float64 oracle only.
    ref: the (out, flat gradient) of the oracle where the caller has it.  -> a dict of the
    figures (printed too)."""
    from tests.test_general_gpu import _oracle
    out, g = ref if ref is not None else _oracle(flat, cb, variant)
    reach = grad_reach(flat, g, variant)
    low = min(reach, key=reach.get)
    print("gradient reach: smallest max|g_data| %.3g (%s)" % (reach[low], low))
    dead = dead_variables(flat, g, variant)
    assert not dead, "variables without a data gradient: %s" % dead
    units = unit_reach(flat, g, variant)
    print("unit reach: %s" % units)
    assert all(n >= UNIT_REACH for n in units.values()), units
    fwd = {}
    if variant in (2, 4):
        fwd = forward_reach(flat, cb, variant, fused, out["logits"], ENTITY_BIASES)
        print("forward reach (x logit tol): %s" % {k: "%.3g" % v for k, v in fwd.items()})
        assert len(fwd) == 4 and all(v >= FORWARD_REACH for v in fwd.values()), fwd
    hunk = forward_reach(flat, cb, variant, fused, out["logits"], HUNK_BIASES)
    print("hunk-side biases, no condition (x logit tol): %s"
          % {k: "%.3g" % v for k, v in hunk.items()})
    return dict(grad_reach=reach[low], units=min(units.values()), forward=fwd, hunk=hunk)


# ----------------------------------------------------------------------------
# entries of the earlier tables that miss the gradient-reach condition
# ----------------------------------------------------------------------------
def earlier_tables():
    """{table: [(id, variant, thunk -> (CommitBatch, flat))]} of the four earlier tables'
    oracle inputs."""
    from tests import _labels as L
    from tests import _tails as TL
    out = {"regimes": [], "labels": [], "ties": [], "tails": []}
    def regimes_inputs(e):
        reg, v, B, ne, nc, dseed, pseed, _ = e
        cb = synth_commits(B, ne, nc, dseed)
        return cb, R.regime_flat(reg, pseed, v, data=cb)

    for e in R.oracle_entries():
        out["regimes"].append(("%s-v%d-%dx%dx%d" % e[:5], e[1], lambda e=e: regimes_inputs(e)))
    for e in L.oracle_entries():
        out["labels"].append((L.entry_id(e), e.variant, lambda e=e: L.inputs(e)))
    for e in T.oracle_entries():
        out["ties"].append((T.entry_id(e), e.variant, lambda e=e: T.inputs(e)))
    for e in TL.b_entries():              # (variant, B, ne, nc, dseed, pseed, fused)
        out["tails"].append(("v%d-%dx%dx%d" % e[:4], e[0],
                             lambda e=e: (synth_commits(e[1], e[2], e[3], e[4]),
                                          R.regime_flat("trained", e[5], e[0]))))
    return out


def dead_kind(dead):
    """"zero": the data gradient of both entity first layers is exactly 0 (x' = 0 on every
    node, rho = 0); "weak": some variable lies below GRAD_REACH without that."""
    e1, e3 = "phi_E_O1/r1_w1o:0", "phi_U_O1/o1_w1o:0"
    return "zero" if dead.get(e1) == 0.0 and dead.get(e3) == 0.0 else "weak"


_RHO0 = "x' = 0 on every node: E1 and E3 (all eight variables) exactly 0"

# table -> {entry id: (kind, reason)}: the entries of the four earlier tables that miss the
# gradient-reach condition.  Their suites are unchanged; this is the record of what they
# compare with zeros (kind "zero") or with a gradient so small that the absolute floor of the
# tolerance carries the check (kind "weak").  model_3's entity-edge variables are exactly 0 in
# every entry of every table and exempt (exempt()): with them _regimes has 16 + 9 = 25 entries
# of its 50 with Ne <= 300 that compare an entity first layer with zeros.
KNOWN_DEAD = {
    "regimes": {
        "trained-v2-3x7x5": ("zero", _RHO0),
        "saturated-v2-3x7x5": ("zero", _RHO0),
        "trained-v4-2x37x19": ("zero", _RHO0),
        "saturated-v4-2x37x19": ("weak", "EE and EC <= 1.7e-7: the EC softmax saturates"),
        "trained-v2-2x65x70": ("zero", _RHO0),
        "degenerate-v2-2x65x70": ("zero", _RHO0),
        "saturated-v2-2x65x70": ("zero", _RHO0),
        "degenerate-v4-2x65x70": ("zero", _RHO0),
        "saturated-v4-2x65x70": ("zero", _RHO0 + "; EE and EC <= 1e-14"),
        "trained-v2-1x120x100": ("zero", _RHO0),
        "saturated-v2-1x120x100": ("zero", _RHO0),
        "trained-v4-1x120x100": ("zero", _RHO0),
        "degenerate-v4-1x120x100": ("zero", _RHO0),
        "saturated-v4-1x120x100": ("zero", _RHO0 + "; EE and EC exactly 0 too"),
        "trained-v2-1x40x257": ("zero", _RHO0),
        "trained-v4-1x40x257": ("zero", _RHO0),
        "degenerate-v4-1x40x257": ("zero", _RHO0),
        "trained-v4-2x401x50": ("zero", _RHO0 + "; EC b1 2.9e-4"),
        "degenerate-v4-2x401x50": ("zero", _RHO0),
    },
    "labels": {
        "directed-init-v2-2x2x2": ("weak", "E1 b1 7.6e-4: one relation per commit"),
        "directed-trained-v2-2x2x2": ("weak", "E1 b1 8.8e-4: one relation per commit"),
        "directed-init-v2-2x5x33": ("zero", _RHO0),
        "directed-trained-v2-2x37x19": ("zero", _RHO0),
        "upper-trained-v2-2x21x40": ("zero", _RHO0),
        "tournament-trained-v2-2x21x40": ("zero", _RHO0),
        "directed-trained-v2-2x65x70": ("zero", _RHO0),
        "directed-init-v4-2x2x2": ("zero", _RHO0 + "; EE <= 9.6e-4"),
        "directed-trained-v4-2x2x2": ("weak", "E1 b1 7.2e-4, EE and EC <= 2.1e-4"),
        "directed-trained-v4-2x5x33": ("weak", "E1 b1 8.1e-4, E3 b1 7.8e-4"),
        "directed-init-v4-2x65x70": ("zero", _RHO0),
        "directed-trained-v2-1x30x160": ("zero", _RHO0),
        "directed-init-v2-2x120x100": ("zero", _RHO0),
        "directed-init-v4-1x30x160": ("zero", _RHO0),
        "directed-init-v4-2x120x100": ("zero", _RHO0 + "; EC b1 5.7e-4"),
        "upper-trained-v4-2x37x19": ("zero", _RHO0),
    },
    "ties": {
        "v4-2x65x70-int10": ("weak", "EE and EC <= 6.3e-4 (E1 / E3 alive by the _alive edit)"),
        "v4-1x120x100-int10": ("weak", "EC b1 7.9e-5, EC b2 4.1e-4"),
        "v4-2x37x19-eq0": ("weak", "EE w11 exactly 0: every attribute of the batch is 0"),
    },
    "tails": {},
}


# ----------------------------------------------------------------------------
# case table
# ----------------------------------------------------------------------------
Case = namedtuple("Case", R.Case._fields + ("xkind", "edensity"))

# (Ne, Nc) of group A, at the fused kernel's own edges (tests/test_live_gpu.py names them);
# attributes alternate int10 / real down the list
A_SHAPES = [
    (16, 2), (17, 3), (32, 15), (33, 16), (63, 17), (64, 31), (65, 32), (102, 33), (103, 64),
    (128, 65), (129, 79), (204, 80), (205, 81), (240, 96),
    (241, 97), (255, 127), (256, 128), (256, 129), (205, 159), (103, 160), (17, 160), (255, 3),
    (33, 129), (129, 33),
    (200, 74), (250, 114), (250, 150), (256, 160),
]
BENCH_SHAPES = A_SHAPES[-4:]
DENSE_EDGES = {(103, 64), (205, 81), (256, 128)}          # edensity 0.5
B_SHAPES = A_SHAPES[0:24:3] + BENCH_SHAPES
C_SHAPES = [(2, 64, 64), (2, 65, 70), (2, 200, 74), (1, 257, 161)]
C_FORMS_AT = (2, 65, 70)
D_SHAPES = [(200, 74), (256, 160)]
E_SHAPES = [(2, 200, 74), (1, 256, 160)]
S_SHAPE = (1, 1024, 512)        # the general path's stress shape; marked slow
E_RUNS = [(2, "fused", "1"), (2, "fused", "0"), (4, "fused", None), (2, "general", None),
          (4, "general", None)]

_REG_IDX = {r: i for i, r in enumerate(REGIMES)}

# Entries that missed a condition of tests/test_live.py at their first seeds and moved on, a
# pseed at a time and after four of those to the next dseed: key -> (dseed, pseed), the
# conditions of the seeds left behind in the comment.
# "kink": the kink guard's worst fraction of the tolerance (limit 0.5) and the variable; "CE":
# the float32 oracle's CE off by more than 5e-6 relative -- with Nc = 3 a commit has 6
# relations, the labels separate and CE falls to where a relative check measures nothing.
MOVED = {
    ("live", 2, 2, 256, 160, "real"): (356, 1024),    # pseed 1023: kink 0.778 (H1 w1)
    # dseed 355: CE x4; dseed 356: CE (1026); 1027: labels separated completely, every data
    # gradient exactly 0
    ("live", 2, 2, 255, 3, "real"): (356, 1028),
    ("live", 2, 2, 241, 97, "int10"): (341, 1023),    # pseed 1022: kink 0.517 (E1 w1)
    ("live", 4, 2, 255, 127, "real"): (355, 1045),    # pseed 1044: kink 0.776 (H1 w1)
    ("live", 2, 2, 205, 81, "int10"): (305, 1027),    # pseed 1026: kink 0.502 (H1 b2)
    ("live", 4, 2, 255, 3, "real"): (355, 1049),      # pseed 1046: kink 0.829 (E1 w1); CE x2
    ("live", 1, 1, 257, 161, "int10"): (357, 1016),   # pseed 1015: kink 3.96 (H1 w1)
    ("live", 2, 2, 103, 160, "real"): (203, 1025),    # pseed 1024: kink 0.573 (H1 w1)
    ("live", 2, 1, 1024, 512, "int10"): (1124, 1024),  # pseed 1023: max |logit| > 1e4
}


def _attrs(ne, nc):
    i = A_SHAPES.index((ne, nc))
    return ("int10", "real")[i % 2], (0.5 if (ne, nc) in DENSE_EDGES else 0.05)


def first_seeds(regime, variant, ne, nc):
    return 100 + ne, 1000 + 100 * _REG_IDX[regime] + 10 * variant + (ne + nc) % 7


def seed_walk(regime, variant, ne, nc):
    """The 12 seed pairs an entry may take, in order."""
    d, p = first_seeds(regime, variant, ne, nc)
    return [(d + i, p + j) for i in range(3) for j in range(4)]


def _key(regime, variant, B, ne, nc, xkind):
    return (regime, variant, B, ne, nc, xkind)


def _case(group, regime, variant, shape, xkind="int10", edensity=0.05, path="general",
          form=None, split=None):
    B, ne, nc = shape
    d, p = MOVED.get(_key(regime, variant, B, ne, nc, xkind),
                     first_seeds(regime, variant, ne, nc))
    return Case(group, regime, variant, B, ne, nc, d, p, path, form, split, xkind, edensity)


def _table():
    T_ = []
    for ne, nc in A_SHAPES:                                                # A fused lattice
        xk, ed = _attrs(ne, nc)
        T_ += [_case("A", "live", 2, (2, ne, nc), xk, ed, "fused", None, s) for s in ("1", "0")]
    for ne, nc in B_SHAPES:                                                # B model_4, fused
        xk, ed = _attrs(ne, nc)
        T_ += [_case("B", "live", 4, (2, ne, nc), xk, ed, "fused", None, s) for s in ("1", "0")]
    for sh in C_SHAPES:                                                    # C general path
        T_ += [_case("C", "live", v, sh) for v in (1, 2, 3, 4)]
    T_ += [_case("C", "live", v, C_FORMS_AT, form=f) for v in (2, 4) for f in ("sorted", "tiled")]
    for ne, nc in D_SHAPES:                                                # D degenerate
        xk, ed = _attrs(ne, nc)
        T_ += [_case("D", "degenerate", v, (2, ne, nc), xk, ed, "fused", None, s)
               for v in (2, 4) for s in ("1", "0")]
    for sh in E_SHAPES:                                                    # E one Adam step
        T_ += [_case("E", "live", v, sh, path=path, split=s) for v, path, s in E_RUNS]
    T_.append(_case("S", "live", 2, S_SHAPE))                              # S slow: stress shape
    return T_


CASES = _table()


def case_id(c):
    s = "%s-%s-v%d-%dx%dx%d-%s-%s" % (c.group, c.regime, c.variant, c.B, c.ne, c.nc, c.xkind,
                                      c.path)
    if c.form:
        s += "-" + c.form
    if c.split is not None:
        s += "-split" + c.split
    return s


Entry = namedtuple("Entry", "regime variant B ne nc dseed pseed xkind edensity fused")


def entry_of(c, fused=None):
    if isinstance(c, Entry):
        return c
    return Entry(c.regime, c.variant, c.B, c.ne, c.nc, c.dseed, c.pseed, c.xkind, c.edensity,
                 c.path == "fused" if fused is None else fused)


def oracle_entries():
    """The distinct inputs the table needs from the oracle; fused is True when any case of
    the entry runs the fused path (its tolerances are then the smaller ones)."""
    seen = {}
    for c in CASES:
        k = entry_of(c)[:-1]
        seen[k] = seen.get(k, False) or c.path == "fused"
    return [Entry(*(k + (f,))) for k, f in seen.items()]


def entry_id(e):
    return "%s-v%d-%dx%dx%d-%s" % (e.regime, e.variant, e.B, e.ne, e.nc, e.xkind)


@functools.lru_cache(maxsize=None)
def _inputs(key):
    e = Entry(*(key + (False,)))
    cb = synth_commits(e.B, e.ne, e.nc, e.dseed, edensity=e.edensity, xkind=e.xkind)
    flat = regime_flat(e.regime, e.pseed, e.variant, e.ne, e.nc)
    flat.setflags(write=False)
    return cb, flat


def inputs(c):
    """(CommitBatch, read-only float32 flat parameters) of a case or an entry."""
    return _inputs(entry_of(c)[:-1])


@functools.lru_cache(maxsize=None)
def _reference(key):
    from tests import test_general_gpu as G
    cb, flat = _inputs(key)
    out, g = G._oracle(flat, cb, key[1])
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    g.setflags(write=False)
    return out, g


def reference(c):
    """The float64 oracle's (out, flat gradient) of a case, computed once per distinct input
    and shared, read-only, among the cases that need it (both block modes of a shape)."""
    return _reference(entry_of(c)[:-1])
