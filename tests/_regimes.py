"""Parameter regimes away from the initialiser, and the parity case table built on them.

layout.init_flat is the state before the first training step: every bias exactly 0 and no
first-layer unit degenerate.  Every bias-proportional term of the kernels is multiplied by
zero there, and the branches for w == 0, d == 0, |d| < 2^-100 and for units that are on
for every pair or for none never run.  regime_flat() builds three states that reach them:

  trained      every weight, theta and bias N(0, 0.1); no exact zero anywhere.
  degenerate   trained, then fixed hidden units of every first layer edited (UNITS below).
  saturated    trained, then every first-layer bias set to +B / -B alternating per unit, B per
               layer just large enough that each unit is on for every pair or for none on the
               batch it runs on (SAT_MARGIN).

CASES is the explicit list the GPU tests run (tests/test_param_regimes_gpu.py); the CPU test
(tests/test_param_regimes.py) holds every entry to the kink guard and the logit range with
the float64 oracle alone.  Nothing here is searched at test time.
"""
from collections import namedtuple

import numpy as np

from hdgnn import layout

REGIMES = ("trained", "degenerate", "saturated")

# Hidden-unit index of each degenerate feature, the same in every first layer.
UNITS = {
    "xj_zero": 1,      # x_j-side input rows = 0
    "xi_zero": 4,      # x_i-side input rows = 0
    "all_zero": 7,     # every input row and the bias = 0: z == 0 exactly (strict > 0 mask)
    "cls_equal": 10,   # the two class rows equal: d / delta / epsilon == 0 exactly
    "cls_tiny": 13,    # class row 0 = 0, class row 1 = 1e-33 (below the 2^-100 cut)
    "xj_negzero": 16,  # x_j-side weight = -0.0
}
TINY = np.float32(1e-33)

# First layers: weight / bias variable (suffix of the layout name), x_i-side rows, x_j-side
# rows, class rows.  E3 has no pair and no class rows: its "x_j" row is the node's own
# attribute, its "x_i" rows the 20 aggregated ones.  The classifiers EC / H2 see
# [class(2), effects(20)] with no i / j split: their "x_i" unit drops every effect row (a
# class-only unit), their "x_j" unit the upper half.
# EE shares one weight w11 between both sides (model_4.py:221), so both side edits hit it.
Layer = namedtuple("Layer", "w b xi xj cls")
LAYERS = {
    "E1": Layer("phi_E_O1/r1_w1o:0", "phi_E_O1/r1_b1o:0", [0], [1], [2, 3]),
    "E3": Layer("phi_U_O1/o1_w1o:0", "phi_U_O1/o1_b1o:0", list(range(1, 21)), [0], None),
    "EC": Layer("phi_U_R1/o1_w1r:0", "phi_U_R1/o1_b1r:0", list(range(2, 22)),
                list(range(12, 22)), [0, 1]),
    "H1": Layer("mlp_hunk_B2/w1:0", "mlp_hunk_B2/b1:0", [0, 1, 2, 3], [4, 5, 6, 7], [8, 9]),
    "H2": Layer("/C_edge_w1:0", "/C_edge_b1:0", list(range(2, 22)), list(range(12, 22)), [0, 1]),
}
EE_W11, EE_W12, EE_B1 = "phi_E_R1/r1_w1r1:0", "phi_E_R1/r1_w1r2:0", "phi_E_R1/r1_b1r:0"

# saturated: |bias| of a first layer = SAT_MARGIN x the largest |z - b| the float64 oracle
# shows for that layer on the case's own batch, layer by layer in data-flow order (a later
# layer's input depends on the earlier biases).  One constant per layer over all shapes would
# have to fit the largest shape and drives the small shapes' logits to 1e7; a margin much
# above 1 does the same through the four-layer cascade (every on unit passes about B on).
# At 1.1 a unit's pre-activation stays at least 0.09 max|z| away from zero, five orders above
# fp32 rounding, so "on for every pair or for none" holds for the engine as for the oracle.
SAT_MARGIN = 1.1
SAT_ORDER = ("E1", "EE", "E3", "EC", "H1", "H2")


def _find(offs, suffix):
    hit = [n for n in offs if n.endswith(suffix)]
    return hit[0] if len(hit) == 1 else None


def first_layers(variant):
    """{layer: (weight view name(s), bias name)} of the first layers this variant has."""
    offs = layout.offsets(variant)
    out = {}
    for key, L in LAYERS.items():
        w, b = _find(offs, L.w), _find(offs, L.b)
        if w is not None:
            out[key] = (w, b)
    if EE_W11 in offs:
        out["EE"] = ((EE_W11, EE_W12), EE_B1)
    return out


def views(flat, variant):
    """name -> writable array view of the variable inside flat."""
    return {n: flat[o:o + int(np.prod(s))].reshape(s)
            for n, (o, s) in layout.offsets(variant).items()}


def _trained(seed, variant):
    rng = np.random.default_rng(seed)
    flat = (0.1 * rng.standard_normal(layout.n_params(variant))).astype(np.float32)
    while (flat == 0).any():                       # never at float32 resolution; kept exact
        z = flat == 0
        flat[z] = (0.1 * rng.standard_normal(int(z.sum()))).astype(np.float32)
    return flat


def _degenerate(flat, variant):
    V = views(flat, variant)
    U = UNITS
    for key, (w, b) in first_layers(variant).items():
        if key == "EE":
            w11, w12, bias = V[w[0]], V[w[1]], V[b]
            w11[0, U["xj_zero"]] = 0.0
            w11[0, U["xi_zero"]] = 0.0
            w11[0, U["all_zero"]] = 0.0
            w12[:, U["all_zero"]] = 0.0
            bias[U["all_zero"]] = 0.0
            w12[1, U["cls_equal"]] = w12[0, U["cls_equal"]]
            w12[0, U["cls_tiny"]] = 0.0
            w12[1, U["cls_tiny"]] = TINY
            w11[0, U["xj_negzero"]] = -0.0
            continue
        L, W, bias = LAYERS[key], V[w], V[b]
        W[L.xj, U["xj_zero"]] = 0.0
        W[L.xi, U["xi_zero"]] = 0.0
        W[:, U["all_zero"]] = 0.0
        bias[U["all_zero"]] = 0.0
        if L.cls is not None:
            W[L.cls[1], U["cls_equal"]] = W[L.cls[0], U["cls_equal"]]
            W[L.cls[0], U["cls_tiny"]] = 0.0
            W[L.cls[1], U["cls_tiny"]] = TINY
        W[L.xj, U["xj_negzero"]] = -0.0
    return flat


def _saturated(flat, variant, data):
    from oracle import model_ref
    V = views(flat, variant)
    sign = np.where(np.arange(20) % 2 == 0, 1.0, -1.0)
    have = first_layers(variant)
    x = np.asarray(data.x, np.float64)
    for key in SAT_ORDER:
        if key not in have:
            continue
        bias = V[have[key][1]]
        bias[:] = 0.0
        trace = {}
        P = model_ref.to_torch_params(model_ref.unflatten(flat.astype(np.float64), variant),
                                      requires_grad=False)
        model_ref.forward(P, x, data.a, data.y, data.hid, data.nlen, variant, trace=trace)
        bias[:] = (SAT_MARGIN * float(trace[key].abs().max()) * sign).astype(np.float32)
    return flat


def regime_flat(name, seed, variant, data=None):
    """float32 flat parameter vector of the regime (layout.offsets(variant) order).
    data: the CommitBatch the parameters will run on; "saturated" needs it (SAT_MARGIN)."""
    flat = _trained(seed, variant)
    if name == "degenerate":
        flat = _degenerate(flat, variant)
    elif name == "saturated":
        if data is None:
            raise ValueError("the saturated regime is sized on a batch: pass data")
        flat = _saturated(flat, variant, data)
    elif name != "trained":
        raise ValueError("unknown regime %r" % (name,))
    return flat


# ----------------------------------------------------------------------------
# tolerances the GPU cases are held to (unchanged from the suite's own numbers)
# ----------------------------------------------------------------------------
GEN_GRAD = (8e-5, 8e-6)       # tests/test_general_gpu.py: x |ref|, x max|ref| of the variable
FUS_GRAD = (1.5e-4, 3e-6)     # tests/test_gpu_parity.py
FUS_LOGIT = (1.5e-5, 1.5e-6)  # tests/test_gpu_parity.py: x |ref|, x max(1, max|ref|) per commit


def grad_tol(ref, fused):
    """Elementwise gradient tolerance of one variable.  A fused-path case runs through
    test_general_gpu._run_and_check (its numbers) and is held to the fused suite's numbers
    as well, so its tolerance is the smaller of the two."""
    ref = np.abs(np.asarray(ref, np.float64))
    scale = max(ref.max(), 1e-12)
    tol = GEN_GRAD[0] * ref + GEN_GRAD[1] * scale + 1e-9
    if fused:
        tol = np.minimum(tol, FUS_GRAD[0] * ref + FUS_GRAD[1] * scale + 1e-9)
    return tol


# ----------------------------------------------------------------------------
# case table
# ----------------------------------------------------------------------------
Case = namedtuple("Case", "group regime variant B ne nc dseed pseed path form split")

_REG_IDX = {r: i for i, r in enumerate(REGIMES)}

# Entries that failed a condition of the CPU check with their first seeds and moved to the
# next seed: key -> (dseed, pseed).  The kink guard held at every seed tried.  Three failed the
# logit range (max |logit| of the seeds left behind in the comment).  Two failed the CE
# condition: a saturated model_2 / model_3 at 3x7x5 separates the labels completely (they
# are an input of the classifier), CE is 2e-4 resp. 0, and the relative CE check then measures
# nothing -- the float32 oracle itself is off by 5e-5 resp. all of it.
MOVED = {
    ("saturated", 2, 1, 120, 100): (220, 1224),   # pseed 1223: 1.45e5
    ("saturated", 4, 1, 120, 100): (220, 1244),   # pseed 1243: 1.61e6
    ("saturated", 1, 2, 65, 70): (165, 1214),     # pseed 1212: 1.52e4, 1213: 1.10e4 (2nd move)
    ("saturated", 2, 3, 7, 5): (108, 1225),       # dseed 107: CE 2.0e-4
    ("saturated", 3, 3, 7, 5): (107, 1236),       # pseed 1235: CE 0
}


def _seeds(regime, variant, B, ne, nc):
    key = (regime, variant, B, ne, nc)
    if key in MOVED:
        return MOVED[key]
    return 100 + ne, 1000 + 100 * _REG_IDX[regime] + 10 * variant + (ne + nc) % 7


def _case(group, regime, variant, shape, path="general", form=None, split=None):
    B, ne, nc = shape
    d, p = _seeds(regime, variant, B, ne, nc)
    return Case(group, regime, variant, B, ne, nc, d, p, path, form, split)


def _table():
    T = []
    for sh in [(3, 7, 5), (2, 37, 19), (2, 65, 70)]:                       # A general
        for v in (1, 2, 3, 4):
            T += [_case("A", r, v, sh) for r in REGIMES]
    for sh in [(2, 37, 19), (2, 65, 70), (1, 120, 100)]:                   # B fused
        for v in (2, 4):
            for split in ("1", "0"):
                T += [_case("B", r, v, sh, "fused", None, split) for r in REGIMES]
    for sh in [(2, 37, 19), (1, 40, 257)]:                                 # C hunk forms
        for v in (1, 2, 4):
            for form in ("sorted", "tiled", "sorted_group"):
                T += [_case("C", r, v, sh, "general", form) for r in REGIMES[:2]]
    T += [_case("D", r, 4, (2, 401, 50)) for r in REGIMES[:2]]             # D EE gam-only table
    for v, path in [(1, "general"), (2, "general"), (3, "general"), (4, "general"),
                    (2, "fused"), (4, "fused")]:                           # E one Adam step
        T += [_case("E", r, v, (2, 37, 19), path) for r in REGIMES]
    for sh in [(11, 12, 9), (19, 12, 9)]:                                  # F block map
        T += [_case("F", "trained", 2, sh, "general", form) for form in ("sorted", "tiled")]
    return T


CASES = _table()


def case_id(c):
    s = "%s-%s-v%d-%dx%dx%d-%s" % (c.group, c.regime, c.variant, c.B, c.ne, c.nc, c.path)
    if c.form:
        s += "-" + c.form
    if c.split is not None:
        s += "-split" + c.split
    return s


def oracle_entries():
    """The distinct (regime, variant, B, ne, nc, dseed, pseed, fused) the table needs from the
    oracle; fused is True when any case of the entry runs the fused path."""
    seen = {}
    for c in CASES:
        k = (c.regime, c.variant, c.B, c.ne, c.nc, c.dseed, c.pseed)
        seen[k] = seen.get(k, False) or c.path == "fused"
    return [k + (f,) for k, f in seen.items()]
