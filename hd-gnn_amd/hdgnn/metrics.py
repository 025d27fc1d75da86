"""Host-side evaluation with the semantics of the reference's EvaluationFuncs.py.

These run on the probabilities the engine returns (B, 2, Ncr) against the one-hot
labels (B, 2, Ncr), exactly as model_2.train/test call them, quirks included
(SURVEY Appendix B.9):
  * top_ACC        EvaluationFuncs.py:27-37   argmax agreement over all relations
                   (np.argmax: ties pick class 0)
  * prec/recall/f1 EvaluationFuncs.py:79-106  np.ceil of labels AND probabilities,
                   then sklearn on channel 0 (so every prediction is 1)
  * AUC            EvaluationFuncs.py:108-153 resets auc inside the graph loop and
                   returns the LAST graph's AUC over the number of scored graphs
  * process_edge   EvaluationFuncs.py:11-16   identity
The correct-count of top_ACC is also exposed (top_acc_count) so data-parallel ranks
can all-reduce it instead of gathering probabilities.
"""
import numpy as np


def process_edge(Ra):
    return Ra


def top_acc_count(label, probs):
    """Number of relations whose argmax class agrees (numpy argmax tie rule)."""
    label = np.asarray(label)
    probs = np.asarray(probs)
    return int((np.argmax(probs, axis=1) == np.argmax(label, axis=1)).sum())


def top_ACC(label, probs):
    label = np.asarray(label)
    return float(top_acc_count(label, probs) / (label.shape[0] * label.shape[2]))


def _per_graph(score_fn, label, real):
    labelz = np.ceil(np.asarray(label))
    realz = np.ceil(np.asarray(real))
    acc = 0.0
    for i in range(labelz.shape[0]):
        acc += score_fn(labelz[i, 0, :], realz[i, 0, :])
    return acc / labelz.shape[0]


def prec(label, real):
    from sklearn.metrics import precision_score
    return _per_graph(precision_score, label, real)


def recall(label, real):
    from sklearn.metrics import recall_score
    return _per_graph(recall_score, label, real)


def f1(label, real):
    from sklearn.metrics import f1_score
    return _per_graph(f1_score, label, real)


def AUC(label, real):
    from sklearn.metrics import roc_auc_score
    label = np.asarray(label)
    real = np.asarray(real)
    auc, count = 0.0, 0
    for i in range(label.shape[0]):
        auc, count = 0.0, 0                      # reset per graph (reference behaviour)
        lab_idx = np.argmax(label[i], axis=0)    # class index of each relation
        pos = np.argmin(label[i], axis=0)        # channel whose score is used
        score = np.where(pos == 0, real[i, 0], real[i, 1])
        try:
            s = roc_auc_score(lab_idx, score)
        except ValueError:
            print("ValueError: Only one class present in y_true. ROC AUC score is not "
                  "defined in that case.")
        else:
            auc += s
            count += 1
    return auc / count


# ---------------------------------------------------------------------------------------
# Counts-based evaluation of the trained classifier (not the reference's quirks above):
# the integer table hdg_eval computes on the device (include/hdgnn.h, HDG_EV_*), its host
# implementation, and the scores that follow from it.
# ---------------------------------------------------------------------------------------
EV_SLOTS, EV_TP, EV_FP, EV_FN, EV_TN, EV_U2, EV_NAN = 8, 0, 1, 2, 3, 4, 5


def eval_counts(label_onehot, probs):
    """(B, 2, R) one-hot labels and probabilities -> int64 (B, EV_SLOTS): per commit TP, FP,
    FN, TN of the argmax prediction (class 1 when p1 > p0: np.argmax's tie rule), U2 = sum
    over (positive, negative) pairs of 2 [s_p > s_n] + [s_p == s_n] with s = probs[:, 1], and
    the number of relations with a NaN in either channel (counted in no other slot and in no
    pair).  The host implementation of hdg_eval: the negatives' scores sorted once per commit,
    np.searchsorted left and right for each positive."""
    label = np.asarray(label_onehot)
    probs = np.asarray(probs)
    B = label.shape[0]
    ev = np.zeros((B, EV_SLOTS), np.int64)
    for b in range(B):
        y = label[b, 1] > label[b, 0]
        p0, p1 = probs[b, 0], probs[b, 1]
        nan = np.isnan(p0) | np.isnan(p1)
        ok = ~nan
        pred = np.zeros(y.shape, bool)
        pred[ok] = p1[ok] > p0[ok]
        ev[b, EV_TP] = np.count_nonzero(ok & y & pred)
        ev[b, EV_FP] = np.count_nonzero(ok & ~y & pred)
        ev[b, EV_FN] = np.count_nonzero(ok & y & ~pred)
        ev[b, EV_TN] = np.count_nonzero(ok & ~y & ~pred)
        ev[b, EV_NAN] = np.count_nonzero(nan)
        neg = np.sort(p1[ok & ~y])
        pos = p1[ok & y]
        lb = np.searchsorted(neg, pos, side="left").astype(np.int64)
        ub = np.searchsorted(neg, pos, side="right").astype(np.int64)
        ev[b, EV_U2] = int((2 * lb + (ub - lb)).sum())
    return ev


def _ratio(num, den):
    """num / den in float64, nan where den == 0 (no warning)."""
    num = np.asarray(num, np.float64)
    den = np.asarray(den, np.float64)
    out = np.full(np.broadcast(num, den).shape, np.nan)
    np.divide(num, den, out=out, where=den != 0)
    return out


def _nanmean(v):
    v = np.asarray(v, np.float64).reshape(-1)
    v = v[~np.isnan(v)]
    return float(v.mean()) if v.size else float("nan")


def scores_from_counts(ev):
    """(n_commits, EV_SLOTS) integer table -> dict of scores.

    acc / precision / recall / f1: pooled over all relations of all commits;
    acc_mean / precision_mean / recall_mean / f1_mean: the mean of the per-commit ratios over
    the commits where the ratio is defined.  A ratio with a zero denominator is nan.
    auc: mean over commits with both classes (P = TP + FN > 0 and N = FP + TN > 0) of
    U2 / (2 P N) in float64, nan when there is no such commit; auc_commits: how many were
    scored; nan_relations: relations left out because a probability was NaN."""
    ev = np.asarray(ev).reshape(-1, EV_SLOTS).astype(np.int64)
    tp, fp, fn, tn = (ev[:, k] for k in (EV_TP, EV_FP, EV_FN, EV_TN))

    def four(tp, fp, fn, tn):
        return (_ratio(tp + tn, tp + fp + fn + tn), _ratio(tp, tp + fp), _ratio(tp, tp + fn),
                _ratio(2 * tp, 2 * tp + fp + fn))

    names = ("acc", "precision", "recall", "f1")
    out = {}
    for n, pooled, per in zip(names, four(tp.sum(), fp.sum(), fn.sum(), tn.sum()),
                              four(tp, fp, fn, tn)):
        out[n] = float(pooled)
        out[n + "_mean"] = _nanmean(per)
    P, N = tp + fn, fp + tn
    both = (P > 0) & (N > 0)
    auc = ev[both, EV_U2].astype(np.float64) / (2.0 * P[both].astype(np.float64)
                                                * N[both].astype(np.float64))
    out["auc"] = float(auc.mean()) if auc.size else float("nan")
    out["auc_commits"] = int(both.sum())
    out["nan_relations"] = int(ev[:, EV_NAN].sum())
    return out


# ---------------------------------------------------------------------------------------
# Untangling: the hunk groups a threshold on the pair scores gives (connected components of
# the link graph) against the true groups (components of the label graph), as the integer
# table hdg_untangle computes on the device (include/hdgnn.h, HDG_UT_*), its host
# implementation, and the partition scores that follow from it.
# ---------------------------------------------------------------------------------------
UT_SLOTS = 8
UT_GROUPS, UT_TGROUPS, UT_SS, UT_SD, UT_DS, UT_DD, UT_LINKS, UT_NAN = range(8)
UT_RULES = ("mean", "any", "both")


def _components(n, a, b):
    """Connected components of the undirected edges (a[k], b[k]) on nodes 0..n-1 -> int32 (n,)
    dense ids ordered by each component's smallest member.  Min-label propagation over the
    edge list with one pointer jump per round, until a fixed point: then every node carries
    its component's smallest member, and the id of a component is the number of smaller ones."""
    lab = np.arange(n, dtype=np.int64)
    while a.size:
        new = lab.copy()
        m = np.minimum(lab[a], lab[b])
        np.minimum.at(new, a, m)
        np.minimum.at(new, b, m)
        new = new[new]
        if np.array_equal(new, lab):
            break
        lab = new
    ids = np.cumsum(lab == np.arange(n)) - 1
    return ids[lab].astype(np.int32)


def untangle_counts(label_onehot, probs, threshold=0.5, rule="mean"):
    """(B, 2, R) one-hot labels and probabilities, R = Nc (Nc - 1) -> (ut int64 (B, UT_SLOTS),
    groups int32 (B, Nc), tgroups int32 (B, Nc)): the host implementation of hdg_untangle,
    definitions as in include/hdgnn.h.  With s_pq = probs[b, 1, r(p, q)] in float32, the pair
    {p, q} is linked iff  mean: s_pq + s_qp > threshold + threshold (both sums in float32),
    any: s_pq > threshold or s_qp > threshold,  both: and  -- strict comparisons, and never
    when either score is NaN (such pairs count in UT_NAN).  groups: components of the link
    graph; tgroups: components of y_pq | y_qp; ids dense, ordered by smallest member."""
    from .data import pair_index
    if rule not in UT_RULES:
        raise ValueError("rule must be one of %s (got %r)" % (", ".join(UT_RULES), rule))
    thr = np.float32(threshold)
    if np.isnan(thr):
        raise ValueError("threshold is NaN")
    label = np.asarray(label_onehot)
    probs = np.asarray(probs, np.float32)
    B, R = probs.shape[0], probs.shape[2]
    nc = int(round((1.0 + np.sqrt(1.0 + 4.0 * R)) / 2.0))
    if nc < 2 or nc * (nc - 1) != R:
        raise ValueError("R = %d is not Nc (Nc - 1)" % R)
    I, J = pair_index(nc)
    iu, ju = np.triu_indices(nc, 1)
    ut = np.zeros((B, UT_SLOTS), np.int64)
    groups = np.zeros((B, nc), np.int32)
    tgroups = np.zeros((B, nc), np.int32)
    S = np.zeros((nc, nc), np.float32)
    Y = np.zeros((nc, nc), bool)
    for b in range(B):
        S[I, J] = probs[b, 1]
        Y[I, J] = label[b, 1] > label[b, 0]
        spq, sqp = S[iu, ju], S[ju, iu]
        nan = np.isnan(spq) | np.isnan(sqp)
        with np.errstate(invalid="ignore", over="ignore"):
            if rule == "mean":
                link = (spq + sqp) > (thr + thr)
            elif rule == "any":
                link = (spq > thr) | (sqp > thr)
            else:
                link = (spq > thr) & (sqp > thr)
        link &= ~nan
        ylink = Y[iu, ju] | Y[ju, iu]
        g = _components(nc, iu[link], ju[link])
        t = _components(nc, iu[ylink], ju[ylink])
        sp, st = g[iu] == g[ju], t[iu] == t[ju]
        groups[b], tgroups[b] = g, t
        ut[b] = (int(g.max()) + 1, int(t.max()) + 1, np.count_nonzero(sp & st),
                 np.count_nonzero(sp & ~st), np.count_nonzero(~sp & st),
                 np.count_nonzero(~sp & ~st), np.count_nonzero(link), np.count_nonzero(nan))
    return ut, groups, tgroups


def scores_from_untangle(ut):
    """(n_commits, UT_SLOTS) integer table -> dict of partition scores.

    rand = (SS + DD) / all pairs, precision = SS / (SS + SD), recall = SS / (SS + DS),
    f1 = 2 SS / (2 SS + SD + DS): pooled over the pairs of all commits; rand_mean /
    precision_mean / recall_mean / f1_mean: the mean of the per-commit ratios over the commits
    where the ratio is defined.  A ratio with a zero denominator is nan (scores_from_counts'
    rule).  exact: share of commits whose predicted partition is the true one (SD = DS = 0);
    group_count_match: share with as many predicted as true groups (both nan without
    commits); nan_pairs: pairs never linked because a score was NaN."""
    ut = np.asarray(ut).reshape(-1, UT_SLOTS).astype(np.int64)
    ss, sd, ds, dd = (ut[:, k] for k in (UT_SS, UT_SD, UT_DS, UT_DD))

    def four(ss, sd, ds, dd):
        return (_ratio(ss + dd, ss + sd + ds + dd), _ratio(ss, ss + sd), _ratio(ss, ss + ds),
                _ratio(2 * ss, 2 * ss + sd + ds))

    out = {}
    for n, pooled, per in zip(("rand", "precision", "recall", "f1"),
                              four(ss.sum(), sd.sum(), ds.sum(), dd.sum()), four(ss, sd, ds, dd)):
        out[n] = float(pooled)
        out[n + "_mean"] = _nanmean(per)
    n = len(ut)
    out["exact"] = float(((sd == 0) & (ds == 0)).mean()) if n else float("nan")
    out["group_count_match"] = (float((ut[:, UT_GROUPS] == ut[:, UT_TGROUPS]).mean()) if n
                                else float("nan"))
    out["nan_pairs"] = int(ut[:, UT_NAN].sum())
    return out


# ---------------------------------------------------------------------------------------
# Linkage: every partition a threshold can give, at once -- the single-linkage merge tree of
# a commit's pair weights and the pair counts of each of its cuts, as hdg_linkage computes
# them on the device (include/hdgnn.h, HDG_LK_*), its host implementation, and the exactly
# optimal threshold of a set of commits that follows from them.
# ---------------------------------------------------------------------------------------
LK_SLOTS = 8
LK_MERGES, LK_TGROUPS, LK_ST, LK_NAN, LK_PAIRS = range(5)


def _nc_of(R):
    nc = int(round((1.0 + np.sqrt(1.0 + 4.0 * R)) / 2.0))
    if nc < 2 or nc * (nc - 1) != R:
        raise ValueError("R = %d is not Nc (Nc - 1)" % R)
    return nc


def linkage(label_onehot, probs, rule="mean"):
    """(B, 2, R) one-hot labels and probabilities, R = Nc (Nc - 1) -> (merges int32
    (B, Nc-1, 2), levels float32 (B, Nc-1), curve int64 (B, Nc-1, 2), tgroups int32 (B, Nc),
    lk int64 (B, LK_SLOTS)): the host implementation of hdg_linkage, definitions as in
    include/hdgnn.h.  Plain Kruskal: every edge {p, q}, p < q, with its weight under the rule
    (mean: s_pq + s_qp in float32, any: the larger, both: the smaller; no edge when the
    weight is NaN; -0 counts as +0) sorted by (weight descending, p, q), then one sequential
    pass of unions.  The curve comes from the clusters' true-group histograms: a merge of A
    and B adds |A| |B| same-predicted pairs, sum_g A_g B_g of them in one true group."""
    from .data import pair_index
    if rule not in UT_RULES:
        raise ValueError("rule must be one of %s (got %r)" % (", ".join(UT_RULES), rule))
    label = np.asarray(label_onehot)
    probs = np.asarray(probs, np.float32)
    B, R = probs.shape[0], probs.shape[2]
    nc = _nc_of(R)
    I, J = pair_index(nc)
    iu, ju = np.triu_indices(nc, 1)
    merges = np.full((B, nc - 1, 2), -1, np.int32)
    levels = np.full((B, nc - 1), np.nan, np.float32)
    curve = np.zeros((B, nc - 1, 2), np.int64)
    tgroups = np.zeros((B, nc), np.int32)
    lk = np.zeros((B, LK_SLOTS), np.int64)
    S = np.zeros((nc, nc), np.float32)
    Y = np.zeros((nc, nc), bool)
    for b in range(B):
        S[I, J] = probs[b, 1]
        Y[I, J] = label[b, 1] > label[b, 0]
        spq, sqp = S[iu, ju], S[ju, iu]
        with np.errstate(invalid="ignore", over="ignore"):
            if rule == "mean":
                w = spq + sqp
            elif rule == "any":
                w = np.maximum(spq, sqp)
            else:
                w = np.minimum(spq, sqp)
        nan = np.isnan(w)                          # either score, or inf + -inf under "mean"
        w = np.where(w == 0, np.float32(0), w).astype(np.float32)       # -0 -> +0
        ylink = Y[iu, ju] | Y[ju, iu]
        t = _components(nc, iu[ylink], ju[ylink])
        ntg = int(t.max()) + 1
        ok = np.flatnonzero(~nan)
        # (w descending, p ascending, q ascending); iu, ju are already in (p, q) order
        order = ok[np.argsort(-w[ok].astype(np.float64), kind="stable")]
        ep, eq, ew = iu[order], ju[order], w[order]
        lab = np.arange(nc)                        # a cluster's label is its smallest member
        hist = np.zeros((nc, ntg), np.int64)       # per cluster: members of each true group
        hist[np.arange(nc), t] = 1
        m = sp = ss = pos = 0
        chunk = 4 * nc
        while pos < len(order) and m < nc - 1:
            # the sequential pass, with the edges already inside one cluster sieved out a
            # chunk at a time (an edge inside a cluster stays inside it)
            sel = np.flatnonzero(lab[ep[pos:pos + chunk]] != lab[eq[pos:pos + chunk]]) + pos
            for e in sel:
                a, c = lab[ep[e]], lab[eq[e]]
                if a == c:
                    continue
                lo, hi = (a, c) if a < c else (c, a)
                sp += int(hist[lo].sum() * hist[hi].sum())
                ss += int(hist[lo] @ hist[hi])
                hist[lo] += hist[hi]
                lab[lab == hi] = lo
                merges[b, m] = (ep[e], eq[e])
                levels[b, m] = ew[e]
                curve[b, m] = (sp, ss)
                m += 1
            pos += chunk
            chunk *= 2
        curve[b, m:] = (sp, ss)
        tgroups[b] = t
        lk[b, :5] = (m, ntg, np.count_nonzero(t[iu] == t[ju]), np.count_nonzero(nan),
                     nc * (nc - 1) // 2)
    return merges, levels, curve, tgroups, lk


def _lk_arrays(levels, curve, lk):
    levels = np.asarray(levels, np.float32)
    levels = levels.reshape(-1, levels.shape[-1])
    curve = np.asarray(curve).astype(np.int64).reshape(levels.shape + (2,))
    lk = np.asarray(lk).astype(np.int64).reshape(-1, LK_SLOTS)
    if len(lk) != len(levels):
        raise ValueError("levels, curve and lk describe different numbers of commits")
    return levels, curve, lk


def curve_scores(levels, curve, lk):
    """Per commit and per cut k (the partition after merges 0 .. k) -> dict of float64
    (n_commits, Nc-1) arrays rand / precision / recall / f1, scores_from_untangle's ratios of
    SS = SS_k, SD = SP_k - SS_k, DS = ST - SS_k, DD = PAIRS - SP_k - ST + SS_k (nan on a zero
    denominator).  Rows k >= M repeat the last cut's scores."""
    levels, curve, lk = _lk_arrays(levels, curve, lk)
    sp, ss = curve[..., 0], curve[..., 1]
    st, pairs = lk[:, LK_ST, None], lk[:, LK_PAIRS, None]
    sd, ds = sp - ss, st - ss
    dd = pairs - sp - st + ss
    return {"rand": _ratio(ss + dd, ss + sd + ds + dd), "precision": _ratio(ss, ss + sd),
            "recall": _ratio(ss, ss + ds), "f1": _ratio(2 * ss, 2 * ss + sd + ds)}


def cut_table(levels, curve, lk, tprime):
    """The (n_commits, UT_SLOTS) table hdg_untangle would give at the link bound t' (a pair
    links iff its weight > t'), read off the linkage: per commit the merges with level > t'
    are done.  UT_LINKS is -1: the tree does not know how many pairs link."""
    levels, curve, lk = _lk_arrays(levels, curve, lk)
    nc = levels.shape[1] + 1
    with np.errstate(invalid="ignore"):
        k = (levels > np.float32(tprime)).sum(1)              # NaN padding compares false
    rows = np.arange(len(levels))
    done = np.where(k[:, None] > 0, curve[rows, np.maximum(k, 1) - 1], 0)
    sp, ss = done[:, 0], done[:, 1]
    st, pairs = lk[:, LK_ST], lk[:, LK_PAIRS]
    ut = np.zeros((len(levels), UT_SLOTS), np.int64)
    ut[:, UT_GROUPS], ut[:, UT_TGROUPS] = nc - k, lk[:, LK_TGROUPS]
    ut[:, UT_SS], ut[:, UT_SD], ut[:, UT_DS] = ss, sp - ss, st - ss
    ut[:, UT_DD] = pairs - sp - st + ss
    ut[:, UT_LINKS], ut[:, UT_NAN] = -1, lk[:, LK_NAN]
    return ut


def best_threshold(levels, curve, lk, rule, score="f1"):
    """The link threshold with the best pooled score over the given commits, exactly:
    -> (threshold, score, t').  The candidates for the link bound t' are every level of every
    commit, and -inf; a candidate does, in each commit, the merges with level > t' (so the
    largest level of all does none, and -inf does every merge above -inf).  The score is
    scores_from_untangle's pooled `score` ("f1" or "rand") of the resulting tables, evaluated
    at every candidate from one sort of all (level, dSP, dSS) events and their running sums.
    A nan score never wins; ties go to the largest t' (if every score is nan: the largest
    candidate, with a nan score).  threshold is what hdg_untangle takes: t' under "any" and
    "both", 0.5 t' under "mean" (its bound is fl32(threshold + threshold)) -- exact unless t'
    is an odd multiple of the smallest denormal: no float32 threshold doubles to such a
    bound, 0.5 t' rounds, and hdg_untangle then cuts at a neighbouring denormal."""
    if rule not in UT_RULES:
        raise ValueError("rule must be one of %s (got %r)" % (", ".join(UT_RULES), rule))
    if score not in ("f1", "rand"):
        raise ValueError("score must be 'f1' or 'rand' (got %r)" % (score,))
    levels, curve, lk = _lk_arrays(levels, curve, lk)
    real = ~np.isnan(levels)
    d = np.diff(curve, axis=1, prepend=0)                      # what merge k adds
    lv = levels[real].astype(np.float64)
    order = np.argsort(-lv, kind="stable")
    lv = lv[order]
    csp = np.concatenate([[0], np.cumsum(d[..., 0][real][order])])
    css = np.concatenate([[0], np.cumsum(d[..., 1][real][order])])
    # candidates, descending: each distinct level (done: the events before its first
    # occurrence), then -inf (done: the events above -inf)
    first = np.flatnonzero(np.concatenate([[True], lv[1:] != lv[:-1]])) if lv.size else \
        np.zeros(0, np.int64)
    cand = lv[first]
    if not (cand.size and cand[-1] == -np.inf):
        cand = np.concatenate([cand, [-np.inf]])
        first = np.concatenate([first, [np.count_nonzero(lv > -np.inf)]])
    sp, ss = csp[first], css[first]
    st, pairs = int(lk[:, LK_ST].sum()), int(lk[:, LK_PAIRS].sum())
    sd, ds = sp - ss, st - ss
    dd = pairs - sp - st + ss
    val = (_ratio(2 * ss, 2 * ss + sd + ds) if score == "f1"
           else _ratio(ss + dd, ss + sd + ds + dd))
    good = ~np.isnan(val)
    i = int(np.flatnonzero(good & (val == val[good].max()))[0]) if good.any() else 0
    tprime = np.float32(cand[i])
    thr = np.float32(0.5) * tprime if rule == "mean" else tprime
    return float(thr), float(val[i]), float(tprime)


# ---------------------------------------------------------------------------------------
# Agglomeration: the merge tree of a commit under single, complete or average linkage, as
# hdg_agglomerate computes it on the device (include/hdgnn.h, HDG_AG_*), its host
# restatement, and the groups any merge tree gives at a link bound (hdg_cut).
# ---------------------------------------------------------------------------------------
AG_METHODS = ("single", "complete", "average")


def agglomerate(label_onehot, probs, rule="mean", method="average", raw=False):
    """(B, 2, R) one-hot labels and probabilities -> linkage()'s five outputs for the merge
    tree under `method` ("single" | "complete" | "average"), the host restatement of
    hdg_agglomerate, definitions as in include/hdgnn.h; with raw=True a sixth, the raw levels
    float32 (B, Nc-1) before the running minimum.  Plain: the full cluster-pair matrix (float32
    weights, or sums under "average"; NaN is no edge), and per step one arg-max over the whole
    matrix in the order (D descending, a, c) -- under "average" over the float64 quotients
    S / (|A| |C|) -- then row and column a are recombined (max ignoring NaN / min keeping NaN /
    one float32 addition) and c is retired.  The curve comes from the clusters' true-group
    histograms as in linkage()."""
    from .data import pair_index
    if rule not in UT_RULES:
        raise ValueError("rule must be one of %s (got %r)" % (", ".join(UT_RULES), rule))
    if method not in AG_METHODS:
        raise ValueError("method must be one of %s (got %r)" % (", ".join(AG_METHODS), method))
    label = np.asarray(label_onehot)
    probs = np.asarray(probs, np.float32)
    B, R = probs.shape[0], probs.shape[2]
    nc = _nc_of(R)
    I, J = pair_index(nc)
    iu, ju = np.triu_indices(nc, 1)
    merges = np.full((B, nc - 1, 2), -1, np.int32)
    levels = np.full((B, nc - 1), np.nan, np.float32)
    rawlv = np.full((B, nc - 1), np.nan, np.float32)
    curve = np.zeros((B, nc - 1, 2), np.int64)
    tgroups = np.zeros((B, nc), np.int32)
    lk = np.zeros((B, LK_SLOTS), np.int64)
    S = np.zeros((nc, nc), np.float32)
    Y = np.zeros((nc, nc), bool)
    upper = np.triu(np.ones((nc, nc), bool), 1)
    for b in range(B):
        S[I, J] = probs[b, 1]
        Y[I, J] = label[b, 1] > label[b, 0]
        with np.errstate(invalid="ignore", over="ignore"):
            if rule == "mean":
                W = S + S.T
            elif rule == "any":
                W = np.maximum(S, S.T)                 # NaN when either is
            else:
                W = np.minimum(S, S.T)
        W = np.where(W == 0, np.float32(0), W).astype(np.float32)       # -0 -> +0
        np.fill_diagonal(W, np.nan)
        nans = int(np.count_nonzero(np.isnan(W[iu, ju])))
        ylink = Y[iu, ju] | Y[ju, iu]
        t = _components(nc, iu[ylink], ju[ylink])
        ntg = int(t.max()) + 1
        hist = np.zeros((nc, ntg), np.int64)
        hist[np.arange(nc), t] = 1
        size = np.ones(nc, np.int64)
        live = np.ones(nc, bool)
        m = sp = ss = 0
        low = None
        while m < nc - 1:
            with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
                V = (W.astype(np.float64) / np.outer(size, size).astype(np.float64)
                     if method == "average" else W.astype(np.float64))
            ok = upper & live[:, None] & live[None, :] & ~np.isnan(V)
            cand = np.flatnonzero(ok.ravel())          # row-major: (a, c) ascending
            if not cand.size:
                break
            j = int(cand[np.argmax(V.ravel()[cand])])  # the first of the largest
            a, c = divmod(j, nc)
            r = np.float32(V[a, c])
            low = r if low is None or r < low else low
            merges[b, m] = (a, c)
            rawlv[b, m], levels[b, m] = r, low
            sp += int(size[a] * size[c])
            ss += int(hist[a] @ hist[c])
            curve[b, m] = (sp, ss)
            with np.errstate(invalid="ignore", over="ignore"):
                if method == "average":
                    n = W[a] + W[c]
                elif method == "single":
                    n = np.fmax(W[a], W[c])
                else:
                    n = np.minimum(W[a], W[c])
            W[a, :] = W[:, a] = n
            W[c, :] = W[:, c] = np.nan
            W[a, a] = np.nan
            hist[a] += hist[c]
            size[a] += size[c]
            live[c] = False
            m += 1
        curve[b, m:] = (sp, ss)
        tgroups[b] = t
        lk[b, :5] = (m, ntg, np.count_nonzero(t[iu] == t[ju]), nans, nc * (nc - 1) // 2)
    out = (merges, levels, curve, tgroups, lk)
    return out + (rawlv,) if raw else out


def cut_groups(merges, levels, tprime):
    """Merges int (n, Nc-1, 2) and levels float32 (n, Nc-1) of any merge tree -> int32
    (n, Nc) groups at the link bound t': per commit the merges with level > t' are united
    (rows of -1 / NaN are skipped); ids dense, ordered by smallest member -- what hdg_cut
    writes."""
    merges = np.asarray(merges)
    levels = np.asarray(levels, np.float32)
    levels = levels.reshape(-1, levels.shape[-1])
    merges = merges.reshape(levels.shape + (2,)).astype(np.int64)
    nc = levels.shape[1] + 1
    groups = np.zeros((len(levels), nc), np.int32)
    with np.errstate(invalid="ignore"):
        take = (levels > np.float32(tprime)) & (merges >= 0).all(-1)
    for b in range(len(levels)):
        groups[b] = _components(nc, merges[b, take[b], 0], merges[b, take[b], 1])
    return groups


# ---------------------------------------------------------------------------------------
# Refinement: best-move sweeps on the correlation-clustering objective from any starting
# partition, as hdg_refine runs them on the device (include/hdgnn.h, HDG_RF_*), its host
# restatement.
# ---------------------------------------------------------------------------------------
RF_SLOTS, RF_MOVES, RF_NAN = 8, 6, 7
RF_Q_SLOTS = 4
RF_Q_START, RF_Q_END, RF_Q_SWEEPS, RF_Q_CONVERGED = range(4)
RF_MAX_SWEEPS = 64


def refine_gains(probs_b, tprime, rule="mean"):
    """One commit's scores (R,) float32 and the link bound t' -> (A int64 (Nc, Nc), no-edge
    pairs): the fixed-point gains a_pq of include/hdgnn.h, symmetric, 0 on the diagonal and
    for a pair that is no edge."""
    from .data import pair_index
    nc = _nc_of(len(probs_b))
    I, J = pair_index(nc)
    S = np.zeros((nc, nc), np.float32)
    S[I, J] = np.asarray(probs_b, np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        if rule == "mean":
            W = S + S.T
        elif rule == "any":
            W = np.maximum(S, S.T)                     # NaN when either is
        else:
            W = np.minimum(S, S.T)
        W = np.where(W == 0, np.float32(0), W).astype(np.float32)       # -0 -> +0
        none = np.isnan(W)
        np.fill_diagonal(none, False)
        d = np.where(none, np.float32(0), W) - np.float32(tprime)       # one float32 subtraction
        A = np.rint(np.clip(d, np.float32(-2), np.float32(2)) * np.float32(262144)).astype(np.int64)
    A[none] = 0
    np.fill_diagonal(A, 0)
    return A, int(np.count_nonzero(none)) // 2


def refine(label_onehot, probs, groups, threshold=0.5, rule="mean", max_sweeps=8):
    """(B, 2, R) one-hot labels and probabilities and starting groups int (B, Nc) or None
    (every hunk alone) -> (ut int64 (B, RF_SLOTS), groups int32 (B, Nc), rq int64
    (B, RF_Q_SLOTS)): the host restatement of hdg_refine, definitions as in include/hdgnn.h.
    Plain: per visit of p one np.bincount of row p of the gains over the slots, then the
    choice among stay, the other non-empty slots and the smallest empty slot (strictly above
    stay; the largest; a non-empty slot before the empty one, then the lowest slot)."""
    return _refine(label_onehot, probs, groups, threshold, rule, max_sweeps, None)


def _node_phase(A, slot, size, budget):
    """hdg_refine's sweeps on one commit's gains A, in place on slot and size: until a sweep
    makes no move or `budget` sweeps have run -> (moves, sweeps, converged, gain in Q)."""
    nc = len(slot)
    moves = sweeps = conv = gain = 0
    while sweeps < budget and not conv:
        moved = 0
        for p in range(nc):
            s = np.bincount(slot, weights=A[p], minlength=nc).astype(np.int64)   # exact
            g = int(slot[p])
            stay, best, to = int(s[g]), None, -1
            cand = size > 0
            cand[g] = False
            if cand.any():
                m = int(s[cand].max())
                if m > stay:
                    best, to = m, int(np.flatnonzero(cand & (s == m))[0])
            if size[g] > 1 and 0 > stay and (best is None or 0 > best):
                best, to = 0, int(np.flatnonzero(size == 0)[0])
            if best is not None:
                slot[p] = to
                size[g] -= 1
                size[to] += 1
                gain += best - stay
                moved += 1
        sweeps += 1
        moves += moved
        conv = int(moved == 0)
    return moves, sweeps, conv, gain


def _group_sweep(A, slot, size):
    """One group sweep of hdg_refine_merge (include/hdgnn.h) on one commit's gains A, in place
    on slot and size -> (merges, gain in Q).  Per visit of a non-empty slot g: C[h] = the sum
    of the gains between g's members and slot h's, one exact integer sum per slot; the largest
    C[h] over the other non-empty slots, strictly above 0, the lowest h among equals; the
    members of max(g, h) move into min(g, h)."""
    nc = len(slot)
    merges = gain = 0
    for g in range(nc):
        if size[g] == 0:
            continue
        c = A[slot == g].sum(0)                            # int64: per hunk q, over g's members
        C = np.zeros(nc, np.int64)
        np.add.at(C, slot, c)
        cand = size > 0
        cand[g] = False
        if not cand.any():
            continue
        m = int(C[cand].max())
        if m <= 0:
            continue
        h = int(np.flatnonzero(cand & (C == m))[0])
        to, frm = min(g, h), max(g, h)
        slot[slot == frm] = to
        size[to] += size[frm]
        size[frm] = 0
        gain += m
        merges += 1
    return merges, gain


def _split_sweep(A, slot, size):
    """One split sweep of hdg_refine_split (include/hdgnn.h) on one commit's gains A, in place
    on slot and size -> (splits, gain in Q).  Per visit of a slot g of at least 2 hunks that no
    split of this sweep filled: the seeds (the pair of g with the smallest gain, the lowest p
    then the lowest q among equals; nothing happens unless it is below 0), the assignment pass,
    at most RS_PASSES - 1 correction passes, and the cut is taken iff the sum between the two
    sides is below 0: side E moves to the smallest empty slot."""
    nc = len(slot)
    splits = gain = 0
    filled = np.zeros(nc, bool)
    for g in range(nc):
        if size[g] < 2 or filled[g]:
            continue
        mem = np.flatnonzero(slot == g)                    # index order
        n = len(mem)
        sub = A[np.ix_(mem, mem)]                          # int64, 0 on the diagonal
        iu, ju = np.triu_indices(n, 1)                     # p ascending, then q ascending
        k = int(np.argmin(sub[iu, ju]))                    # the first among equals
        s1, s2 = int(iu[k]), int(ju[k])
        if sub[s1, s2] >= 0:
            continue
        side = np.zeros(n, np.int64)                       # 0 not assigned, 1 side G, 2 side E
        side[s1], side[s2] = 1, 2
        others = [m for m in range(n) if m != s1 and m != s2]
        for m in others:
            side[m] = 2 if sub[m, side == 2].sum() > sub[m, side == 1].sum() else 1
        for _ in range(RS_PASSES - 1):
            changed = False
            for m in others:
                x = side[m]
                if sub[m, side == 3 - x].sum() > sub[m, side == x].sum():      # a_mm is 0
                    side[m] = 3 - x
                    changed = True
            if not changed:
                break
        C = int(sub[np.ix_(side == 1, side == 2)].sum())
        if C >= 0:
            continue
        e = int(np.flatnonzero(size == 0)[0])
        moved = mem[side == 2]
        slot[moved] = e
        size[e] = len(moved)
        size[g] -= len(moved)
        filled[e] = True
        gain -= C
        splits += 1
    return splits, gain


def _refine(label_onehot, probs, groups, threshold, rule, max_sweeps, max_rounds, kinds=1):
    """refine (max_rounds None), refine_merge and refine_split: the checks, the start, the node
    phase -- alone, or in rounds with the sweeps of `kinds` (1 a group sweep, 2 a split sweep,
    3 both) after each -- and the rows."""
    from .data import pair_index
    if rule not in UT_RULES:
        raise ValueError("rule must be one of %s (got %r)" % (", ".join(UT_RULES), rule))
    thr = np.float32(threshold)
    with np.errstate(over="ignore"):
        tp = thr + thr if rule == "mean" else thr
    if not (np.isfinite(thr) and np.isfinite(tp)):
        raise ValueError("threshold %r gives no finite link bound" % (threshold,))
    if not 1 <= int(max_sweeps) <= RF_MAX_SWEEPS:
        raise ValueError("max_sweeps must be in [1, %d] (got %r)" % (RF_MAX_SWEEPS, max_sweeps))
    if max_rounds is not None and not 1 <= int(max_rounds) <= RM_MAX_ROUNDS:
        raise ValueError("max_rounds must be in [1, %d] (got %r)" % (RM_MAX_ROUNDS, max_rounds))
    if kinds not in (RS_MERGE, RS_SPLIT, RS_MERGE | RS_SPLIT):
        raise ValueError("kinds must be 1 (merge), 2 (split) or 3 (both) (got %r)" % (kinds,))
    label = np.asarray(label_onehot)
    probs = np.asarray(probs, np.float32)
    B, R = probs.shape[0], probs.shape[2]
    nc = _nc_of(R)
    if groups is not None:
        groups = np.asarray(groups).astype(np.int64).reshape(B, nc)
    I, J = pair_index(nc)
    iu, ju = np.triu_indices(nc, 1)
    ut = np.zeros((B, RF_SLOTS), np.int64)
    out = np.zeros((B, nc), np.int32)
    rq = np.zeros((B, RF_Q_SLOTS if max_rounds is None else RM_Q_SLOTS), np.int64)
    Y = np.zeros((nc, nc), bool)
    every = np.arange(nc)
    for b in range(B):
        A, nans = refine_gains(probs[b, 1], tp, rule)
        slot = every.copy()
        if groups is not None:                     # a group sits at its smallest member
            ok = (groups[b] >= 0) & (groups[b] < nc)
            low = np.full(nc, nc, np.int64)
            np.minimum.at(low, groups[b][ok], every[ok])
            slot[ok] = low[groups[b][ok]]
        size = np.bincount(slot, minlength=nc)
        q0 = int(A[iu, ju][slot[iu] == slot[ju]].sum())
        moves, sweeps, conv, gain = _node_phase(A, slot, size, int(max_sweeps))
        q1 = q0 + gain
        if max_rounds is not None:
            rounds, merges, splits, qn = 0, 0, 0, q1
            while True:
                merged = split = 0
                if kinds & RS_MERGE:
                    merged, gain = _group_sweep(A, slot, size)
                    q1 += gain
                if kinds & RS_SPLIT:
                    split, gain = _split_sweep(A, slot, size)
                    q1 += gain
                rounds += 1
                merges += merged
                splits += split
                acted = merged + split
                conv = int(conv and not acted)
                if not acted or rounds >= int(max_rounds) or sweeps >= int(max_sweeps):
                    break
                m, s, conv, gain = _node_phase(A, slot, size, int(max_sweeps) - sweeps)
                moves, sweeps, q1 = moves + m, sweeps + s, q1 + gain
        low = np.full(nc, nc, np.int64)
        np.minimum.at(low, slot, every)
        lab = low[slot]                            # every hunk's smallest group member
        g = (np.cumsum(lab == every) - 1)[lab].astype(np.int32)
        Y[I, J] = label[b, 1] > label[b, 0]
        ylink = Y[iu, ju] | Y[ju, iu]
        t = _components(nc, iu[ylink], ju[ylink])
        sp, st = g[iu] == g[ju], t[iu] == t[ju]
        out[b] = g
        ut[b] = (int(g.max()) + 1, int(t.max()) + 1, np.count_nonzero(sp & st),
                 np.count_nonzero(sp & ~st), np.count_nonzero(~sp & st),
                 np.count_nonzero(~sp & ~st), moves, nans)
        rq[b, :RF_Q_SLOTS] = (q0, q1, sweeps, conv)
        if max_rounds is not None:
            rq[b, RF_Q_SLOTS:] = (rounds, merges, qn, splits)
    return ut, out, rq


# ---------------------------------------------------------------------------------------
# Refinement with rounds: after every node phase one group sweep, in which whole groups merge,
# as hdg_refine_merge and hdg_refine_merge_ladder run them on the device (include/hdgnn.h,
# HDG_RM_*), their host restatements.
# ---------------------------------------------------------------------------------------
RM_Q_SLOTS = 8
RM_Q_ROUNDS, RM_Q_MERGES, RM_Q_NODE = 4, 5, 6
RM_MAX_ROUNDS = 16
# hdg_refine_split: the kinds of sweep of a round, the passes of a split attempt, the rq row
RS_MERGE, RS_SPLIT = 1, 2
RS_PASSES = 4
RS_Q_SLOTS, RS_Q_SPLITS = 8, 7


def refine_merge(label_onehot, probs, groups, threshold=0.5, rule="mean", max_sweeps=8,
                 max_rounds=4):
    """refine() with rounds -> (ut int64 (B, RF_SLOTS), groups int32 (B, Nc), rq int64
    (B, RM_Q_SLOTS)): the host restatement of hdg_refine_merge, definitions as in
    include/hdgnn.h.  A round is refine's node phase, then one group sweep (per visit of a
    non-empty slot one exact sum per slot of the gains between the two slots' members, and
    the best merge strictly above 0); until a group sweep merges nothing, `max_rounds` rounds
    have run or the node sweeps of all rounds reach `max_sweeps`.  RF_MOVES counts node moves
    only; rq adds the rounds, the merges and Q after the first node phase."""
    if max_rounds is None:
        raise ValueError("max_rounds must be in [1, %d] (got None)" % RM_MAX_ROUNDS)
    return _refine(label_onehot, probs, groups, threshold, rule, max_sweeps, max_rounds)


def refine_split(label_onehot, probs, groups, threshold=0.5, rule="mean", max_sweeps=8,
                 max_rounds=4, kinds=3):
    """refine_merge() with split sweeps -> (ut int64 (B, RF_SLOTS), groups int32 (B, Nc), rq
    int64 (B, RS_Q_SLOTS)): the host restatement of hdg_refine_split, definitions as in
    include/hdgnn.h.  A round is refine's node phase, then with kinds & RS_MERGE one group sweep
    and with kinds & RS_SPLIT one split sweep (_split_sweep: seeded bisection of a slot, taken
    iff the sum between the two sides is below 0); until a round merges nothing and splits
    nothing, `max_rounds` rounds have run or the node sweeps reach `max_sweeps`.  rq is
    refine_merge's row with the accepted splits in RS_Q_SPLITS."""
    if max_rounds is None:
        raise ValueError("max_rounds must be in [1, %d] (got None)" % RM_MAX_ROUNDS)
    return _refine(label_onehot, probs, groups, threshold, rule, max_sweeps, max_rounds, kinds)


# ---------------------------------------------------------------------------------------
# Refinement ladder: refine at every rung of a ladder of thresholds, each rung from the cut
# of a merge tree at that rung, as hdg_refine_ladder runs it on the device (include/hdgnn.h,
# HDG_RL_*), its host restatement, and the rung with the best pooled score -- the threshold
# calibrated for the refined result, which is not the tree's best cut.
# ---------------------------------------------------------------------------------------
RL_MAX_RUNGS = 64


def ladder(lo, hi, n):
    """The n rungs float32(lo + (hi - lo) k / (n - 1)), k = 0 .. n-1, the arithmetic in
    float64; n == 1 gives lo.  1 <= n <= RL_MAX_RUNGS, finite ends."""
    if not (isinstance(n, (int, np.integer)) and not isinstance(n, bool)
            and 1 <= n <= RL_MAX_RUNGS):
        raise ValueError("a ladder has 1 to %d rungs (got %r)" % (RL_MAX_RUNGS, n))
    lo, hi = float(lo), float(hi)
    if not (np.isfinite(lo) and np.isfinite(hi)):
        raise ValueError("a ladder's ends must be finite (got %r, %r)" % (lo, hi))
    if n == 1:
        return np.array([lo], np.float32)
    return (lo + (hi - lo) * np.arange(n, dtype=np.float64) / (n - 1)).astype(np.float32)


def _rungs(thresholds):
    thr = np.asarray(thresholds, np.float32).reshape(-1)
    if not 1 <= len(thr) <= RL_MAX_RUNGS:
        raise ValueError("a ladder has 1 to %d rungs (got %d)" % (RL_MAX_RUNGS, len(thr)))
    return thr


def refine_ladder(label_onehot, probs, thresholds, tree=None, rule="mean", max_sweeps=8):
    """(B, 2, R) one-hot labels and probabilities, T thresholds and tree = (merges, levels) of
    any merge tree or None -> (ut int64 (T, B, RF_SLOTS), groups int32 (T, B, Nc), rq int64
    (T, B, RF_Q_SLOTS)): the host restatement of hdg_refine_ladder.  A loop: per rung
    cut_groups at the rung's link bound (None: every hunk alone), then refine at the rung."""
    return _ladder_of(lambda start, t: refine(label_onehot, probs, start, t, rule, max_sweeps),
                      thresholds, tree, rule)


def refine_merge_ladder(label_onehot, probs, thresholds, tree=None, rule="mean", max_sweeps=8,
                        max_rounds=4):
    """refine_ladder() with rounds -> (ut int64 (T, B, RF_SLOTS), groups int32 (T, B, Nc), rq
    int64 (T, B, RM_Q_SLOTS)): the host restatement of hdg_refine_merge_ladder.  A loop: per
    rung cut_groups at the rung's link bound (None: every hunk alone), then refine_merge at
    the rung."""
    return _ladder_of(lambda start, t: refine_merge(label_onehot, probs, start, t, rule,
                                                    max_sweeps, max_rounds),
                      thresholds, tree, rule)


def refine_split_ladder(label_onehot, probs, thresholds, tree=None, rule="mean", max_sweeps=8,
                        max_rounds=4, kinds=3):
    """refine_merge_ladder() with refine_split()'s rounds -> (ut int64 (T, B, RF_SLOTS), groups
    int32 (T, B, Nc), rq int64 (T, B, RS_Q_SLOTS)): the host restatement of
    hdg_refine_split_ladder.  A loop: per rung cut_groups at the rung's link bound (None: every
    hunk alone), then refine_split at the rung."""
    return _ladder_of(lambda start, t: refine_split(label_onehot, probs, start, t, rule,
                                                    max_sweeps, max_rounds, kinds),
                      thresholds, tree, rule)


def _ladder_of(run, thresholds, tree, rule):
    """The loop of every ladder: per rung the cut of `tree` at the rung's link bound
    (None: every hunk alone), then run(start, threshold); the rungs stacked."""
    thr = _rungs(thresholds)
    if rule not in UT_RULES:
        raise ValueError("rule must be one of %s (got %r)" % (", ".join(UT_RULES), rule))
    out = []
    for t in thr:
        start = None
        if tree is not None:
            with np.errstate(over="ignore"):
                start = cut_groups(tree[0], tree[1], t + t if rule == "mean" else t)
        out.append(run(start, t))
    return tuple(np.stack([o[i] for o in out]) for i in range(3))


def best_rung(ut_ladder, thresholds, score="f1"):
    """ut_ladder int (T, n_commits, RF_SLOTS) and the T thresholds -> (index, threshold, score,
    per-rung scores float64 (T,)): the rung with the best pooled `score` ("f1" | "rand",
    scores_from_untangle's) over the commits.  A nan score never wins; ties go to the lowest
    index; if every score is nan: index 0, with a nan score."""
    if score not in ("f1", "rand"):
        raise ValueError("score must be 'f1' or 'rand' (got %r)" % (score,))
    thr = _rungs(thresholds)
    ut = np.asarray(ut_ladder)
    if ut.shape[0] != len(thr) or ut.shape[-1] != RF_SLOTS:
        raise ValueError("ut_ladder must be (%d, n_commits, %d) (got %r)"
                         % (len(thr), RF_SLOTS, ut.shape))
    vals = np.array([scores_from_untangle(ut[k])[score] for k in range(len(thr))], np.float64)
    good = ~np.isnan(vals)
    i = int(np.flatnonzero(good & (vals == vals[good].max()))[0]) if good.any() else 0
    return i, float(thr[i]), float(vals[i]), vals


# ---------------------------------------------------------------------------------------
# Matching: how many hunks are in the right group under the best one-to-one assignment of
# predicted to true groups, as hdg_match computes it on the device (include/hdgnn.h,
# HDG_MT_*), its host restatement with an integer assignment solver, the scores that follow
# and the rung of a ladder with the best pooled accuracy.
# ---------------------------------------------------------------------------------------
MT_SLOTS = 8
MT_GROUPS, MT_TGROUPS, MT_MATCHED, MT_PURITY, MT_COVER, MT_CELLS, MT_ISOLATED = range(7)
MT_MAX_SETS = 64


def assign_max(table):
    """Integer table (K, M) of non-negative weights -> (value, col int64 (K,)): the largest
    sum of table[i, col[i]] over one-to-one assignments that assign the smaller side fully
    (col[i] = -1 for a row left out when K > M), an empty cell counting 0.  Shortest
    augmenting paths with integer potentials on the negated table (Kuhn-Munkres in
    Jonker-Volgenant's form), rows on the smaller side, every scan a numpy operation over the
    columns, ties between equal slacks to the lowest column.  The value is unique, the
    assignment one optimum."""
    a = np.asarray(table)
    if a.ndim != 2 or not np.issubdtype(a.dtype, np.integer):
        raise ValueError("table must be a 2-d integer array (got %r, %s)" % (a.shape, a.dtype))
    if a.size and a.min() < 0:
        raise ValueError("table must be non-negative")
    K, M = a.shape
    if K > M:
        value, row = assign_max(a.T)
        col = np.full(K, -1, np.int64)
        col[row] = np.arange(M)
        return value, col
    cost = -a.astype(np.int64)
    inf = np.int64(1) << 60
    u, v = np.zeros(K, np.int64), np.zeros(M, np.int64)
    pcol = np.full(M, -1, np.int64)               # the row assigned to a column
    for i in range(K):
        minv = np.full(M, inf, np.int64)
        way = np.full(M, -1, np.int64)
        used = np.zeros(M, bool)
        i0, j0 = i, -1
        while True:
            cur = cost[i0] - u[i0] - v
            better = ~used & (cur < minv)
            minv[better] = cur[better]
            way[better] = j0
            j1 = int(np.argmin(np.where(used, inf, minv)))      # the first of equals
            delta = minv[j1]
            u[pcol[used]] += delta
            u[i] += delta
            v[used] -= delta
            minv[~used] -= delta
            used[j1] = True
            j0 = j1
            if pcol[j1] < 0:
                break
            i0 = pcol[j1]
        while j0 >= 0:
            j1 = way[j0]
            pcol[j0] = i if j1 < 0 else pcol[j1]
            j0 = j1
    col = np.full(K, -1, np.int64)
    hit = pcol >= 0
    col[pcol[hit]] = np.flatnonzero(hit)
    return int(a[np.arange(K), col].sum()) if K else 0, col


def _match_one(g, t):
    """Predicted ids g (by smallest member) and dense true ids t of one commit -> (mt row,
    mate): the table with np.add.at, the isolated cells taken as they are, assign_max on the
    residual graph."""
    nc = len(g)
    gd = (np.cumsum(g == np.arange(nc)) - 1)[g]                 # dense, by smallest member
    G, TG = int(gd.max()) + 1, int(t.max()) + 1
    keys, first, w = np.unique(gd.astype(np.int64) * TG + t, return_index=True,
                               return_counts=True)
    cg, ct = keys // TG, keys % TG                                # the non-zero cells
    rmax, cmax = np.zeros(G, np.int64), np.zeros(TG, np.int64)
    np.maximum.at(rmax, cg, w)
    np.maximum.at(cmax, ct, w)
    rdeg, cdeg = np.bincount(cg, minlength=G), np.bincount(ct, minlength=TG)
    iso = (rdeg[cg] == 1) & (cdeg[ct] == 1)
    gm = np.full(G, -1, np.int64)
    gm[cg[iso]] = ct[iso]
    matched = int(w[iso].sum())
    if not iso.all():
        rows, ri = np.unique(cg[~iso], return_inverse=True)
        cols, ci = np.unique(ct[~iso], return_inverse=True)
        table = np.zeros((len(rows), len(cols)), np.int64)
        np.add.at(table, (ri, ci), w[~iso])
        value, col = assign_max(table)
        matched += value
        hit = col >= 0
        hit[hit] = table[np.flatnonzero(hit), col[hit]] > 0       # not through an empty cell
        gm[rows[hit]] = cols[col[hit]]
    row = (G, TG, matched, int(rmax.sum()), int(cmax.sum()), len(keys), int(iso.sum()), 0)
    return row, gm[gd].astype(np.int32)


def match_counts(label_onehot, groups):
    """(B, 2, R) one-hot labels, R = Nc (Nc - 1), and group ids int (S, B, Nc) or (B, Nc) ->
    (mt int64 (S, B, MT_SLOTS), mate int32 (S, B, Nc), tgroups int32 (B, Nc)): the host
    restatement of hdg_match, definitions as in include/hdgnn.h.  Predicted groups by
    refine()'s start rule (equal ids in [0, Nc) together, any other id alone), true groups
    untangle_counts()'s.  mate is one optimal assignment: under ties the device may return
    another; both satisfy #{p : mate[p] == tgroups[p]} == MATCHED."""
    from .data import pair_index
    label = np.asarray(label_onehot)
    B, R = label.shape[0], label.shape[2]
    nc = _nc_of(R)
    groups = np.asarray(groups)
    if groups.ndim == 2:
        groups = groups[None]
    if groups.ndim != 3 or groups.shape[1:] != (B, nc) or not 1 <= len(groups) <= MT_MAX_SETS:
        raise ValueError("groups must be (S, %d, %d) or (%d, %d) with 1 <= S <= %d (got %r)"
                         % (B, nc, B, nc, MT_MAX_SETS, groups.shape))
    groups = groups.astype(np.int64)
    S = len(groups)
    I, J = pair_index(nc)
    iu, ju = np.triu_indices(nc, 1)
    Y = np.zeros((nc, nc), bool)
    every = np.arange(nc)
    mt = np.zeros((S, B, MT_SLOTS), np.int64)
    mate = np.zeros((S, B, nc), np.int32)
    tgroups = np.zeros((B, nc), np.int32)
    for b in range(B):
        Y[I, J] = label[b, 1] > label[b, 0]
        ylink = Y[iu, ju] | Y[ju, iu]
        tgroups[b] = _components(nc, iu[ylink], ju[ylink])
        for s in range(S):
            ids = groups[s, b]
            ok = (ids >= 0) & (ids < nc)
            low = np.full(nc, nc, np.int64)
            np.minimum.at(low, ids[ok], every[ok])
            g = every.copy()
            g[ok] = low[ids[ok]]
            mt[s, b], mate[s, b] = _match_one(g, tgroups[b].astype(np.int64))
    return mt, mate, tgroups


def scores_from_match(mt, nc):
    """(n_commits, MT_SLOTS) integer table and nc, the hunks per commit (the length of the
    group ids) -> dict.  accuracy: matched hunks pooled over all commits, sum MATCHED /
    (n_commits nc); accuracy_mean: the mean of the per-commit MATCHED / nc (equal to the
    pooled value, every commit having nc hunks; kept beside it as the other score dicts keep
    theirs); purity, cover: pooled likewise; exact: share of commits with MATCHED == nc (the
    predicted partition is the true one); groups_mean, tgroups_mean.  Without commits every
    value is nan (_ratio's rule)."""
    mt = np.asarray(mt).reshape(-1, MT_SLOTS).astype(np.int64)
    nc = int(nc)
    if nc < 1:
        raise ValueError("nc must be positive (got %r)" % (nc,))
    n = len(mt)
    out = {"accuracy": float(_ratio(mt[:, MT_MATCHED].sum(), n * nc)),
           "accuracy_mean": _nanmean(_ratio(mt[:, MT_MATCHED], np.full(n, nc))),
           "purity": float(_ratio(mt[:, MT_PURITY].sum(), n * nc)),
           "cover": float(_ratio(mt[:, MT_COVER].sum(), n * nc))}
    nan = float("nan")
    out["exact"] = float((mt[:, MT_MATCHED] == nc).mean()) if n else nan
    out["groups_mean"] = float(mt[:, MT_GROUPS].mean()) if n else nan
    out["tgroups_mean"] = float(mt[:, MT_TGROUPS].mean()) if n else nan
    return out


def best_rung_match(mt_ladder, thresholds, nc):
    """mt_ladder int (T, n_commits, MT_SLOTS), the T thresholds and nc -> (index, threshold,
    accuracy, per-rung accuracies float64 (T,)): best_rung's contract on the pooled accuracy
    of scores_from_match.  A nan score never wins; ties go to the lowest index; if every
    score is nan: index 0, with a nan score."""
    thr = _rungs(thresholds)
    mt = np.asarray(mt_ladder)
    if mt.ndim != 3 or mt.shape[0] != len(thr) or mt.shape[-1] != MT_SLOTS:
        raise ValueError("mt_ladder must be (%d, n_commits, %d) (got %r)"
                         % (len(thr), MT_SLOTS, mt.shape))
    vals = np.array([scores_from_match(mt[k], nc)["accuracy"] for k in range(len(thr))],
                    np.float64)
    good = ~np.isnan(vals)
    i = int(np.flatnonzero(good & (vals == vals[good].max()))[0]) if good.any() else 0
    return i, float(thr[i]), float(vals[i]), vals
