"""Exact relu ties at interior positions: lattice parameters, and the parity case table on them.

Every first layer of the engine decides which pairs are on by a strict z > 0 (TF's ReluGrad is
g * (z > 0)).  The forward cannot see that rule: a tie adds relu(0) = 0 to a relu sum and
u_i + w1 x_j = 0 to the count / prefix-sum form, so `>=` for `>`, or an upper bound for a
lower bound on a run of equal sorted values, leaves every logit, probability and loss bit as
it was.  Only the backward counts and masks move.  The other tables never hold a partial tie:
their parameters are floats (z is never 0), or a whole unit is zero (the set boundary is 0 or
nd, never beside pairs that are on and pairs that are off).

lattice_flat() is the `trained` regime with the hidden units LU of every pair first layer put
on a dyadic lattice, where the layer reads raw data, so that z is exactly representable: the
engine's fp32 z is the exact value under any association, fma or not, and the float64
oracle's is the same number.

  E1 (variants 2, 4)  rows [x_i, x_j, 1-a, a] and b1: x rows k/16, class rows k/4
  EE (variants 3, 4)  w11 (shared by both sides) k/16, both w12 rows k/4, and b1
  H1, variants 1, 3   B2 = B1, nbr holds integer counts x raw x: x rows k/32, count rows k/16,
                      label rows k/4
  H1, variant 2       x' rows (0, 1, 4, 5) = 0; count rows k/16, label rows k/4
  H1, variant 4       E_edge2 is a softmax: rows 0..7 = 0, label rows k/4 (a class-only tie)
  E3 / EC / H2        stay trained (no search, float inputs); where the trained E3 leaves
                      x' = 0 on every node (rho = 0: no gradient reaches E1 and its ties
                      cannot move anything) the entry is in ALIVE and E3 takes the _alive
                      edit of tests/test_e2_local_gpu.py, or the entry moves to the next seed

with k = +-1..+-4 drawn from the seed, the signs fixed by the unit's role (ROLES), and the bias
solved, as a multiple of the lattice unit, so that one data pair of the case's own batch ties.
The pair is the first of the role's class, in (commit, relation) order, whose bias gives
every commit a tie, a pair on and a pair off and ties at most UNIT_SHARE of the unit's pairs;
where no pair does, the magnitudes are redrawn (attempt 1, 2, ...; from attempt SHARED on H1's
two count rows of a side share a magnitude, from attempt TWO_CLASS on the other class row is
solved on a pair of a second commit, _solve_two).  That is a fixed rule, a
pure function of (seed, variant, batch); tests/test_ties.py checks its outcome from the
oracle's own trace, and an entry that misses a condition moves to the next seed in MOVED.

A layer whose z takes two values per unit (H1 of variant 4; E1 / EE where every attribute of
the batch is equal) cannot have a tie, a pair on and a pair off in one unit: there the tie is a
whole class set beside the other class on or off (WHOLE_ROLES), and there is no d = 0 unit
(d = 0 ties every pair or none: the `degenerate` regime's all_zero unit).

Two attribute kinds beside the generator's integers 0..9: `half`, Ne distinct signed
half-integers per commit (nd = Ne: the binary searches meet the tie at an interior slot after
log2(Ne) levels), and `eq3` / `eq0`, every attribute 3 resp. 0 (nd = 1).

CASES is the explicit list the GPU tests run (tests/test_ties_gpu.py).
"""
import functools
from collections import namedtuple

import numpy as np

from hdgnn import layout
from hdgnn.data import CommitBatch
from hdgnn.synth import synth_commits
from oracle import model_ref
from tests import _regimes as R

LU = (0, 2, 3, 5, 6, 8, 9, 11)          # the lattice units of every lattice layer
LAYERS = ("E1", "EE", "H1")
XKINDS = ("int10", "half", "eq3", "eq0")
UNIT_SHARE = 0.25                       # a unit's ties: at most this share of its pairs
ATTEMPTS = 32
SHARED = 8
TWO_CLASS = 16

# role of lattice unit u = 0..7: sign of the x_i-side and of the x_j-side weight (prefix and
# suffix sets on the row and on the column side), class of the pair the bias is solved on,
# d = 0 (both class rows equal).  Every sign pair occurs with a class-0 and a class-1 tie.
Role = namedtuple("Role", "si sj cls d0")
ROLES = [Role(1 if u & 2 == 0 else -1, 1 if u & 1 == 0 else -1, (u ^ (u >> 2)) & 1, u == 7)
         for u in range(8)]
# EE has one weight for both sides: its sign alternates, the class every second unit
EE_ROLES = [Role(1 if u & 1 == 0 else -1, 1 if u & 1 == 0 else -1, (u >> 1) & 1, u == 7)
            for u in range(8)]
# two-valued layers: (tie class, other class on): unit 0 ties the whole class-0 set beside
# class-1 pairs that are on; the others tie the (small) class-1 set, class 0 on / off in turn
WHOLE_ROLES = [(0, True)] + [(1, u & 1 == 1) for u in range(1, 8)]

H1_ROWS = {1: "full", 3: "full", 2: "counts", 4: "labels"}


def _alive(flat, variant):
    """tests/test_e2_local_gpu._alive: mlp2_entity_B1 with positive biases and w2' >= 0, so
    x' > 0 on every node and a gradient reaches the entity stage (rho != 0)."""
    V = R.views(flat, variant)
    V["phi_U_O1/o1_b1o:0"][:] = 0.2
    V["phi_U_O1/o1_b2o:0"][:] = 0.5
    w2 = V["phi_U_O1/o1_w2o:0"]
    w2[:] = np.abs(w2)
    return flat


# ----------------------------------------------------------------------------
# data
# ----------------------------------------------------------------------------
def commits(xkind, B, ne, nc, dseed, edensity=0.05):
    """synth_commits(B, ne, nc, dseed, edensity) with x of the kind; a, y, hid, nlen stay."""
    cb = synth_commits(B, ne, nc, dseed, edensity=edensity)
    if xkind == "int10":
        return cb
    if xkind == "half":
        rng = np.random.default_rng([dseed, 77])
        base = (np.arange(ne) - ne // 2) / 2.0
        x = np.stack([rng.permutation(base) for _ in range(B)]).astype(np.float32)
    elif xkind in ("eq3", "eq0"):
        x = np.full((B, ne), 3.0 if xkind == "eq3" else 0.0, np.float32)
    else:
        raise ValueError("unknown attribute kind %r" % (xkind,))
    return CommitBatch(x, cb.a, cb.y, cb.hid, cb.nlen)


def features(data):
    """The raw inputs of the pair first layers in float64, exact: {"E": (B1 (B, Pe, 4), class
    (B, Pe)), "H": (B3 (B, Pc, 10) of variants 1 / 3, class (B, Pc))}.  B3's count columns
    (2, 3, 6, 7) and label columns are those of every variant."""
    x = np.asarray(data.x, np.float64)
    a, y = np.asarray(data.a), np.asarray(data.y)
    B, ne = x.shape
    nc = y.shape[1]
    I, J = model_ref.pair_index(ne)
    acls = a[:, I, J].astype(np.int64)
    B1 = np.stack([x[:, I], x[:, J], acls == 0, acls == 1], -1).astype(np.float64)
    s, t = model_ref.relation_maps(data.hid, data.nlen, ne, nc)
    nbr = np.zeros((B, nc + 1, 4))
    for b in range(B):
        np.add.at(nbr[b], np.where(s[b] < 0, nc, s[b]), B1[b])
        np.add.at(nbr[b], np.where(t[b] < 0, nc, t[b]), B1[b])
    nbr = nbr[:, :nc]
    Ip, Jq = model_ref.pair_index(nc)
    ycls = y[:, Ip, Jq].astype(np.int64)
    B3 = np.concatenate([nbr[:, Ip], nbr[:, Jq], (ycls == 0)[..., None], (ycls == 1)[..., None]],
                        -1).astype(np.float64)
    return {"E": (B1, acls), "H": (B3, ycls)}


def two_valued(layer, variant, data):
    """The layer's lattice z takes two values per unit on this batch (one per class)."""
    if layer == "H1":
        return variant == 4
    return bool((np.ptp(np.asarray(data.x), axis=1) == 0).all())


# ----------------------------------------------------------------------------
# the lattice
# ----------------------------------------------------------------------------
def _column(rng, layer, variant, role, whole, attempt=0):
    """One lattice unit's input rows, (nrows,) float64 in the layer's B1 / B3 row order.  From
    attempt SHARED on, the two count rows of a side of H1 share one magnitude: the side's sum
    then depends on the number of relations at the hunk alone, and commits with few hunks
    (2 x 256 x 9, 3 x 7 x 5) get a value that all of them hold."""
    def k(den):
        return float(rng.integers(1, 5)) / den
    c0 = float(rng.choice([-1.0, 1.0])) * k(4)
    if whole is not None:
        tie, other_on = whole          # tie on class 1: z0 = -d; tie on class 0: z1 = d
        d = k(4) if (tie == 0) == other_on else -k(4)
    else:
        d = 0.0 if role.d0 else float(rng.choice([-1.0, 1.0])) * k(4)
    c1 = c0 + d
    if layer in ("E1", "EE"):
        wi = role.si * k(16)
        wj = wi if layer == "EE" else role.sj * k(16)
        return np.array([wi, wj, c0, c1])
    rows = H1_ROWS[variant]
    col = np.zeros(10)
    for base, s in ((0, role.si), (4, role.sj)):
        xr = [s * k(32), s * k(32)]
        cr = [s * k(16), s * k(16)]
        if attempt >= SHARED:
            cr[1] = cr[0]
        if rows == "full":
            col[base:base + 2] = xr
        if rows in ("full", "counts"):
            col[base + 2:base + 4] = cr
    col[8:10] = c0, c1
    return col


def _solve(zb, cls, role, whole):
    """The threshold v = -bias of one unit: zb (B, P) its z without the bias, cls (B, P) the
    pairs' classes.  -> (v, (commit, relation)) or None."""
    if whole is not None:
        hit = np.argwhere(cls == whole[0])
        return (float(zb[tuple(hit[0])]), tuple(hit[0])) if len(hit) else None
    ok = None
    for c in range(zb.shape[0]):
        u = np.unique(zb[c])
        u = u[(u > u[0]) & (u < u[-1])]              # a pair off and a pair on beside the tie
        ok = u if ok is None else np.intersect1d(ok, u)
    vals, counts = np.unique(zb, return_counts=True)
    ok = np.intersect1d(ok, vals[counts <= UNIT_SHARE * zb.size])
    cand = np.argwhere(np.ones_like(cls, bool) if role.d0 else cls == role.cls)
    good = np.isin(zb[cand[:, 0], cand[:, 1]], ok)
    if not good.any():
        return None
    at = tuple(cand[np.argmax(good)])
    return float(zb[at]), at


def _solve_two(feat, col, cls, role):
    """The second rule (attempts TWO_CLASS on): one commit's tie fixes bias + class row of the
    role's class on a pair A of that class, another commit's tie the other class row on a pair
    B of the other class; a third commit has to hold one of the two values by itself.  The
    solved class row is a multiple of the lattice unit like the bias, no longer k/4.
    -> (column, v, A) or None."""
    base = feat[..., :-2] @ col[:-2]
    t = role.cls
    ct = col[-2 + t]
    A_all = np.argwhere(cls == t)[:24]
    for A in map(tuple, A_all):
        b = -(base[A] + ct)
        miss = [c for c in range(cls.shape[0])
                if not ((cls[c] == t) & (base[c] == base[A])).any()]
        if not miss:
            continue
        B_all = np.argwhere(cls[miss[0]] == 1 - t)[:64]
        for r in B_all[:, 0]:
            col2 = col.copy()
            col2[-2 + (1 - t)] = -(base[miss[0], r] + b)
            if abs(col2[-2 + (1 - t)]) > 64 or col2[-1] == col2[-2]:
                continue
            zb = feat @ col2
            if _meets(zb, -b):
                return col2, -b, A
    return None


def _meets(zb, v):
    tie = zb == v
    return bool(tie.any(1).all() and (zb > v).any(1).all() and (zb < v).any(1).all()
                and tie.mean() <= UNIT_SHARE)


Unit = namedtuple("Unit", "unit role whole column bias pair attempt")


def lattice_build(seed, variant, data, alive=False):
    """-> (flat, {layer: [Unit] * 8}): the trained regime at `seed` with the lattice units of
    the variant's pair first layers edited as the module text says."""
    flat = R.regime_flat("trained", seed, variant)
    if alive:
        flat = _alive(flat, variant)
    V = R.views(flat, variant)
    F = features(data)
    have = R.first_layers(variant)
    info = {}
    for li, layer in enumerate(LAYERS):
        if layer not in have:
            continue
        w, b = have[layer]
        feat, cls = F["H" if layer == "H1" else "E"]
        tv = two_valued(layer, variant, data)
        units = []
        for u, unit in enumerate(LU):
            role = (EE_ROLES if layer == "EE" else ROLES)[u]
            whole = WHOLE_ROLES[u] if tv else None
            first = None
            for attempt in range(ATTEMPTS):
                rng = np.random.default_rng([seed, li, u, attempt])
                col = _column(rng, layer, variant, role, whole, attempt)
                got = _solve(feat @ col, cls, role, whole)
                if first is None:
                    first = col
                if got is None and attempt >= TWO_CLASS and whole is None and not role.d0:
                    two = _solve_two(feat, col, cls, role)
                    if two is not None:
                        col, got = two[0], two[1:]
                if got is not None:
                    break
            else:                     # no attempt met the rule: tests/test_ties.py will say so
                col, attempt = first, -1
                zb = feat @ col
                hit = np.argwhere(cls == role.cls)
                at = tuple(hit[0]) if len(hit) else (0, 0)
                got = (float(zb[at]), at)
            bias = np.float32(-got[0])
            assert float(bias) == -got[0], "bias off the float32 lattice"
            if layer == "EE":
                V[w[0]][0, unit] = col[0]
                V[w[1]][:, unit] = col[2:4]
            else:
                V[w][:, unit] = col
            V[b][unit] = bias
            units.append(Unit(unit, role, whole, col, float(bias), got[1], attempt))
        info[layer] = units
    return flat, info


def lattice_flat(seed, variant, data, alive=False):
    """float32 flat parameter vector: `trained` with the lattice units' rows and biases;
    alive: the _alive edit on the (non-lattice) E3 parameters as well."""
    return lattice_build(seed, variant, data, alive)[0]


def lattice_layers(variant):
    return [l for l in LAYERS if l in R.first_layers(variant)]


def layer_vars(variant, layer):
    """(weight variable names, bias name) of a lattice layer."""
    w, b = R.first_layers(variant)[layer]
    return (w if isinstance(w, tuple) else (w,)), b


def lattice_mask(variant):
    """bool (n_params,): the lattice parameters (LU columns of the lattice layers' first
    weights and biases)."""
    m = np.zeros(layout.n_params(variant), bool)
    offs = layout.offsets(variant)
    for layer in lattice_layers(variant):
        ws, b = layer_vars(variant, layer)
        for name in ws + (b,):
            o, shape = offs[name]
            sel = np.zeros(shape, bool)
            sel[..., list(LU)] = True
            m[o:o + sel.size] = sel.reshape(-1)
    return m


def bias_index(variant, layer):
    """flat indices of the layer's lattice biases."""
    o, _ = layout.offsets(variant)[layer_vars(variant, layer)[1]]
    return o + np.array(LU)


grad_tol = R.grad_tol


# ----------------------------------------------------------------------------
# case table
# ----------------------------------------------------------------------------
Case = namedtuple("Case", R.Case._fields + ("xkind", "edensity"))

# Entries that failed a condition of tests/test_ties.py with their first seeds and moved to the
# next: key -> (dseed, pseed), the condition of the seeds left behind in the comment.
# Both seeds + 1 per move; (variant, B, ne, nc, xkind) -> (dseed, pseed).  "no tie": a lattice
# unit of H1 without a tie, or without a pair on and a pair off, in one of the commits -- with 5
# hunks a commit has 20 relations, and three commits have to hold the unit's threshold.
MOVED = {
    (1, 3, 7, 5, "int10"): (139, 3047),     # no tie x32
    (1, 3, 7, 5, "half"): (111, 3119),      # no tie x4
    (2, 3, 7, 5, "int10"): (115, 3033),     # no tie x8
    (2, 3, 7, 5, "half"): (117, 3135),      # no tie x10
    (3, 3, 7, 5, "int10"): (148, 3076),     # no tie x40, EE ties on one class only x1
    (3, 3, 7, 5, "half"): (111, 3139),      # no tie x4
    (4, 3, 7, 5, "int10"): (110, 3048),     # no y = 1 relation in the batch x1, no tie x2
    (4, 3, 7, 5, "half"): (111, 3149),      # the same x1 + x2; E1 bite 2.6e-8 (rho = 0), alive: kink
    (2, 2, 37, 19, "int10"): (138, 3021),   # E1 bite 3.5e-8 (rho = 0), alive: kink
    (1, 2, 65, 70, "int10"): (166, 3013),   # kink
    (2, 2, 65, 70, "int10"): (166, 3023),   # E1 bite 4.4e-8 (rho = 0), alive: kink
    (2, 1, 120, 100, "int10"): (221, 3024),  # E1 bite 7.1e-8 (rho = 0), alive: max |logit| > 1e4
    # E1 bite <= 1.2e-8 (rho = 0) x10, alive: max |logit| > 1e4 x4, EE bite <= 4.6 x6
    (4, 1, 120, 100, "half"): (230, 3153),
    (1, 1, 40, 257, "half"): (141, 3114),   # no tied pair on a run of equal alpha (sorted form)
    (2, 2, 256, 9, "half"): (369, 3139),    # no tie x9, max |logit| > 1e4 x4
    # EE bite <= 10.5 x4 (the EC softmax saturates), E1 bite <= 4.1e-8, max |logit| > 1e4
    (4, 2, 401, 50, "int10"): (510, 3052),
}

# Entries whose E3 takes the _alive edit (rho = 0 at the trained E3, E1's bite <= 7e-8; two
# missed the kink guard without it).
ALIVE = {
    (2, 2, 65, 70, "int10"), (4, 2, 65, 70, "int10"), (2, 1, 120, 100, "int10"),
    (4, 1, 120, 100, "int10"), (2, 2, 37, 19, "eq0"), (2, 1, 40, 257, "int10"),
    (4, 2, 37, 19, "eq3"),
}


def _key(c):
    return (c.variant, c.B, c.ne, c.nc, c.xkind)


def _seeds(variant, B, ne, nc, xkind):
    key = (variant, B, ne, nc, xkind)
    if key in MOVED:
        return MOVED[key]
    return 100 + ne, 3000 + 100 * XKINDS.index(xkind) + 10 * variant + (ne + nc) % 7


def _case(group, variant, shape, xkind, path="general", form=None, split=None, edensity=0.05):
    B, ne, nc = shape
    d, p = _seeds(variant, B, ne, nc, xkind)
    return Case(group, "lattice", variant, B, ne, nc, d, p, path, form, split, xkind, edensity)


A_SHAPES = [(3, 7, 5), (2, 37, 19), (2, 65, 70)]
B_SHAPES = [(2, 37, 19), (2, 65, 70), (1, 120, 100)]
B_HBM, B_WIDE = (2, 256, 9), (2, 33, 81)
C_SHAPES = [(2, 37, 19), (1, 40, 257)]
C_FORMS = ("dense", "sorted", "tiled", "sorted_group")
D_SHAPE = (2, 401, 50)
EF_SHAPE = (2, 37, 19)
E_RUNS = [(1, "general"), (2, "general"), (3, "general"), (4, "general"), (2, "fused"),
          (4, "fused")]


def _table():
    T = []
    both = XKINDS[:2]
    for sh in A_SHAPES:                                                    # A general
        T += [_case("A", v, sh, k) for v in (1, 2, 3, 4) for k in both]
    for sh in B_SHAPES:                                                    # B fused
        T += [_case("B", v, sh, k, "fused", None, split)
              for v in (2, 4) for split in ("1", "0") for k in both]
    # x-lists of 2 x 256 x ~128 words: E1 / E2 read them from the prepared buffer, not LDS
    T.append(_case("B", 2, B_HBM, "half", "fused", None, "1", edensity=0.5))
    T.append(_case("B", 2, B_WIDE, "half", "fused", None, "1"))           # nc = 81: wide form
    for sh in C_SHAPES:                                                    # C hunk forms
        T += [_case("C", v, sh, k, "general", form)
              for v in (1, 2, 4) for form in C_FORMS for k in both]
    # D EE gam-only table.  Integer attributes only: with Ne = 401 half-integers reach +-100,
    # and of 30 seeds none met the bite of E1 and EE and max |logit| <= 1e4 together (rho = 0
    # at the trained E3; with the _alive edit max |logit| = 3.6e7 or the EC softmax saturates)
    T += [_case("D", 4, D_SHAPE, "int10")]
    T += [_case("E", v, EF_SHAPE, k, path) for v, path in E_RUNS for k in both]   # E Adam step
    T += [_case("F", v, EF_SHAPE, k, path)                                 # F all x equal
          for v in (2, 4) for k in XKINDS[2:] for path in ("general", "fused")]
    return T


CASES = _table()


def case_id(c):
    s = "%s-v%d-%dx%dx%d-%s-%s" % (c.group, c.variant, c.B, c.ne, c.nc, c.xkind, c.path)
    if c.form:
        s += "-" + c.form
    if c.split is not None:
        s += "-split" + c.split
    return s


Entry = namedtuple("Entry", "variant B ne nc dseed pseed xkind edensity alive fused")


def entry_of(c, fused=None):
    if isinstance(c, Entry):
        return c
    return Entry(c.variant, c.B, c.ne, c.nc, c.dseed, c.pseed, c.xkind, c.edensity,
                 _key(c) in ALIVE,
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
    return "v%d-%dx%dx%d-%s" % (e.variant, e.B, e.ne, e.nc, e.xkind)


@functools.lru_cache(maxsize=None)
def _inputs(key):
    e = Entry(*(key + (False,)))
    cb = commits(e.xkind, e.B, e.ne, e.nc, e.dseed, e.edensity)
    flat, info = lattice_build(e.pseed, e.variant, cb, e.alive)
    flat.setflags(write=False)
    return cb, flat, info


def inputs(c):
    """(CommitBatch, read-only float32 flat parameters) of a case or an entry."""
    return _inputs(entry_of(c)[:-1])[:2]


def build_info(c):
    return _inputs(entry_of(c)[:-1])[2]


@functools.lru_cache(maxsize=None)
def _reference(key):
    from tests import test_general_gpu as G
    cb, flat, _ = _inputs(key)
    out, g = G._oracle(flat, cb, key[0])
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    g.setflags(write=False)
    return out, g


def reference(c):
    """The float64 oracle's (out, flat gradient) of a case, computed once per distinct input
    and shared, read-only, among the cases that need it."""
    return _reference(entry_of(c)[:-1])
