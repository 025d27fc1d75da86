"""Asymmetric hunk labels, and the parity case table built on them.

hdgnn.synth.synth_commits draws the hunk label matrix symmetric (y = up | up^T), and every
edit the other suites make to it (0 * y, the full matrix) is symmetric too.  The engine's
contract is wider: bit j of ybits row i is the class of the ordered relation (i, j)
(include/hdgnn.h), as the reference fills C_edge from y_label[k, i, j] per ordered pair.
With y == y^T a transposed read of y, a swapped side of the label lists, a row sum taken for
a column sum or a count of the wrong side leave every output bit unchanged.  The three label
kinds here take that cover away (the diagonal is 0 in all of them):

  directed     Bernoulli(0.10), independent per ordered pair.
  upper        Bernoulli(0.20) for p < q, 0 for p > q: a row has labels only to its right, a
               column only above it, so the row lists and the column lists are disjoint in
               content and differ in length.
  tournament   exactly one of y_pq, y_qp is 1 for every pair: every bit disagrees with its
               transpose; label density 50 %.

x, a, hid and nlen stay those of synth_commits(B, ne, nc, dseed).  The parameter sets are
"init" (layout.init_flat: every bias 0, so the per-node label counts, which the biases
multiply, drop out) and "trained" (tests/_regimes.py's trained regime: no exact zero).

CASES is the explicit list the GPU tests run (tests/test_labels_gpu.py); the CPU test
(tests/test_labels.py) holds every entry to the asymmetry, bite, kink, range and CE guards
with the float64 oracle alone.  Nothing here is searched at test time.
"""
import functools
from collections import namedtuple

import numpy as np

from hdgnn import layout
from hdgnn.data import CommitBatch
from hdgnn.synth import synth_commits
from tests import _regimes as R
from tests import test_general_gpu as G
from tests import test_gpu_parity as FP

KINDS = ("directed", "upper", "tournament")
PARAMS = ("init", "trained")


def label_grid(kind, B, nc, seed):
    """(B, nc, nc) u8 labels of the kind, diagonal 0."""
    rng = np.random.default_rng(seed)
    u = rng.random((B, nc, nc))
    if kind == "directed":
        y = u < 0.10
    elif kind == "upper":
        y = np.triu(u < 0.20, 1)
    elif kind == "tournament":
        w = np.triu(u < 0.5, 1)
        y = w | np.tril(~w.transpose(0, 2, 1), -1)
    else:
        raise ValueError("unknown label kind %r" % (kind,))
    y = y.astype(np.uint8)
    idx = np.arange(nc)
    y[:, idx, idx] = 0
    return y


def commits(kind, B, ne, nc, dseed, lseed):
    """synth_commits(B, ne, nc, dseed) with y replaced by label_grid(kind, B, nc, lseed)."""
    cb = synth_commits(B, ne, nc, dseed)
    return CommitBatch(cb.x, cb.a, label_grid(kind, B, nc, lseed), cb.hid, cb.nlen)


def transposed(cb):
    return CommitBatch(cb.x, cb.a, np.ascontiguousarray(cb.y.transpose(0, 2, 1)), cb.hid, cb.nlen)


def param_flat(param, pseed, variant):
    if param == "init":
        return layout.init_flat(pseed, variant)
    if param == "trained":
        return R.regime_flat("trained", pseed, variant)
    raise ValueError("unknown parameter set %r" % (param,))


# ----------------------------------------------------------------------------
# tolerances the GPU cases are held to: the suites' own, imported
# ----------------------------------------------------------------------------
def logit_tol(ref, fused):
    """Elementwise logit tolerance, ref (B, 2, Pc): test_general_gpu._check_outputs' for every
    case, the smaller of that and test_gpu_parity._logit_tol for a fused-path case."""
    ref = np.asarray(ref, np.float64)
    scale = np.maximum(1.0, np.abs(ref).reshape(ref.shape[0], -1).max(1))[:, None, None]
    tol = G.LOGIT_RTOL * np.abs(ref) + G.LOGIT_ATOL * scale
    return np.minimum(tol, FP._logit_tol(ref)) if fused else tol


grad_tol = R.grad_tol     # (ref, fused): the regimes table's, = the two suites' numbers


# ----------------------------------------------------------------------------
# case table
# ----------------------------------------------------------------------------
Case = namedtuple("Case", "group kind param variant B ne nc dseed lseed pseed path form split")

_KIND_IDX = {k: i for i, k in enumerate(KINDS)}
_PAR_IDX = {p: i for i, p in enumerate(PARAMS)}

# Label seeds that are not the formula's.  directed at 2x2 has one pair per commit and needs
# y_01 != y_10 in both commits (probability 0.03 per draw): the first seed from 0 that has it.
LABEL_SEED = {
    ("directed", 2, 2, 2): 16,
}

# Entries that failed a guard of tests/test_labels.py with their first seeds and moved to the
# next (all three seeds + 1 per move): key -> (dseed, lseed, pseed), the failed condition of
# the seeds left behind in the comment.  Six missed the logit bite: at init-scale logits of
# 600 .. 6000 the absolute part of the logit tolerance (x max |logit| of the commit) grows
# with the largest logit while the label-dependent part of a logit does not.  Four missed the
# kink guard, one the logit range.  The gradient bite held at every seed tried (>= 104 x).
MOVED = {
    # logit bite 37, 41.5, 13.9, 48.3, 19.5, 18.9 x tol (6 moves; max |logit| 770 .. 1750)
    ("directed", "init", 1, 2, 65, 70): (171, 5271, 2018),
    ("directed", "trained", 1, 2, 65, 70): (166, 5266, 2113),    # logit bite 49.1
    ("upper", "trained", 2, 2, 21, 40): (122, 6104, 2126),       # kink 0.624 (E1 w1)
    ("tournament", "init", 2, 2, 21, 40): (122, 7104, 2026),     # kink 0.646 (E1 w1)
    ("tournament", "trained", 2, 2, 21, 40): (122, 7104, 2126),  # kink 0.557 (H2 w1)
    ("directed", "init", 3, 2, 65, 70): (166, 5266, 2033),       # logit bite 29.3
    ("directed", "trained", 3, 2, 65, 70): (166, 5266, 2133),    # logit bite 25.3
    ("directed", "init", 2, 1, 30, 160): (131, 5251, 2022),      # kink 0.745 (H1 b1)
    ("directed", "init", 2, 2, 120, 100): (221, 5461, 2024),     # logit bite 35.2
    ("directed", "trained", 2, 2, 120, 100): (221, 5461, 2124),  # max |logit| 1.15e4
    # logit bite 45.4, 32.6; kink 12.5 (EE w11); logit bite 7.29 (max |logit| 5966) (4 moves)
    ("directed", "init", 4, 2, 120, 100): (224, 5464, 2047),
    # group D's count guard (test_count_cases_tell_the_orientation): at the first two seeds the
    # oracle predicts one class for all 684 relations, and then the correct-count is the number
    # of 0 (or 1) labels whichever way y is read (2 moves each)
    ("directed", "trained", 2, 2, 37, 19): (139, 5132, 2122),
    ("directed", "trained", 4, 2, 37, 19): (139, 5132, 2142),
}


def _seeds(kind, param, variant, B, ne, nc):
    key = (kind, param, variant, B, ne, nc)
    if key in MOVED:
        return MOVED[key]
    lseed = LABEL_SEED.get((kind, B, ne, nc), 5000 + 1000 * _KIND_IDX[kind] + 3 * ne + nc)
    return 100 + ne, lseed, 2000 + 100 * _PAR_IDX[param] + 10 * variant + (ne + nc) % 7


def _case(group, kind, param, variant, shape, path="general", form=None, split=None):
    B, ne, nc = shape
    d, l, p = _seeds(kind, param, variant, B, ne, nc)
    return Case(group, kind, param, variant, B, ne, nc, d, l, p, path, form, split)


A_SHAPES = [(2, 2, 2), (3, 7, 5), (2, 5, 33), (2, 37, 19), (2, 21, 40), (2, 65, 70)]
A_ALL_KINDS = [(3, 7, 5), (2, 21, 40)]
B_SHAPES = [(2, 2, 2), (3, 7, 5), (2, 37, 19), (2, 21, 40), (1, 30, 160), (2, 120, 100)]
C_SHAPES = [(2, 37, 19), (1, 40, 257)]
C_FORMS = ("dense", "sorted", "tiled", "sorted_group")
D_SHAPE = (2, 37, 19)


def _table():
    """The whole matrix: no entry was dropped.  (Entries of different groups that agree in
    kind, parameter set, variant and shape share one oracle run, oracle_entries().)"""
    T = []
    for v in (1, 2, 3, 4):                                                 # A general
        for sh in A_SHAPES:
            kinds = KINDS if sh in A_ALL_KINDS else KINDS[:1]
            T += [_case("A", k, p, v, sh) for k in kinds for p in PARAMS]
    for v in (2, 4):                                                       # B fused
        for split in ("1", "0"):
            for sh in B_SHAPES:
                kinds = ("directed", "upper") if sh == (2, 21, 40) else ("directed",)
                T += [_case("B", k, p, v, sh, "fused", None, split) for k in kinds for p in PARAMS]
    for sh in C_SHAPES:                                                    # C hunk forms
        for v in (1, 4):
            for form in C_FORMS:
                T += [_case("C", k, "trained", v, sh, "general", form) for k in KINDS[:2]]
    for path in ("general", "fused"):                                      # D counts
        T += [_case("D", "directed", "trained", v, D_SHAPE, path) for v in (2, 4)]
    return T


CASES = _table()


def case_id(c):
    s = "%s-%s-%s-v%d-%dx%dx%d-%s" % (c.group, c.kind, c.param, c.variant, c.B, c.ne, c.nc, c.path)
    if c.form:
        s += "-" + c.form
    if c.split is not None:
        s += "-split" + c.split
    return s


Entry = namedtuple("Entry", "kind param variant B ne nc dseed lseed pseed fused")


def entry_of(c, fused=None):
    return Entry(c.kind, c.param, c.variant, c.B, c.ne, c.nc, c.dseed, c.lseed, c.pseed,
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
    return "%s-%s-v%d-%dx%dx%d" % e[:6]


def inputs(c):
    """(CommitBatch, float32 flat parameters) of a case or an entry."""
    return (commits(c.kind, c.B, c.ne, c.nc, c.dseed, c.lseed),
            param_flat(c.param, c.pseed, c.variant))


@functools.lru_cache(maxsize=None)
def _reference(key):
    e = Entry(*(key + (False,)))
    cb, flat = inputs(e)
    out, g = G._oracle(flat, cb, e.variant)
    for k, v in out.items():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    g.setflags(write=False)
    return out, g


def reference(c):
    """The float64 oracle's (out, flat gradient) of a case, computed once per distinct input
    and shared, read-only, among the cases that need it."""
    return _reference(entry_of(c)[:-1])
