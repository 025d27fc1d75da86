"""GPU box: time of hdg_refine_split (kinds both) against hdg_refine_merge, and of
hdg_refine_split_ladder against hdg_refine_merge_ladder (19 rungs), on the same inputs in the
same process, at the glide shape (200x74, B=100) and the stress shape (1024x512, B=32), at most
8 node sweeps and 4 rounds.

Three sets of scores per shape:
  sparse  tools/refine_time.py's scores, the start hdg_untangle's groups (the ladder: the cut of
          hdg_agglomerate's AVERAGE tree): few splits are expected, so the difference is mostly
          the price of the seed walks and of futile attempts
  noisy   planted groups, 0.65 inside and 0.35 across + 0.25 sigma noise, every hunk alone at
          the start (the ladder: no tree)
  fused   tests/_split.py's two_fused at any nc: six runs of hunks, the true groups, fused in
          pairs through one wrong pair at 0.97; the start is the fused groups (the ladder: the
          cut of hdg_agglomerate's SINGLE tree, which chains them): every fused group is cut

Events around --launches (20) calls after --warmup (5), --pairs (3) interleaved pairs (merge,
split) per case; the medians and their ratio are in the row, with the splits and rounds per
commit.  Before anything is timed the outputs of all four calls are compared with
hdgnn.metrics on the host.  Prints one JSON line per case and writes them to --out (default
bench_out/refine_split_time.json).

  python tools/refine_split_time.py [--launches 20] [--warmup 5] [--pairs 3] [--out PATH]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "hd-gnn_amd")]

SHAPES = [("glide", 200, 74, 100), ("stress", 1024, 512, 32)]
LADDER = (0.05, 0.95, 19)
SWEEPS, ROUNDS, THR, KINDS = 8, 4, 0.5, 3


def scores(kind, nc, B, np, data):
    """-> (labels (B, nc, nc) uint8, scores (B, R) float32)."""
    R = nc * (nc - 1)
    rng = np.random.default_rng(nc)
    I, J = data.pair_index(nc)
    grp = rng.integers(0, max(2, nc // 12), (B, nc))
    y = (grp[:, :, None] == grp[:, None, :]).astype(np.uint8)     # pack_bits clears the diagonal
    same = grp[:, I] == grp[:, J]
    if kind == "fused":
        half = np.arange(nc) * 6 // nc
        first = np.flatnonzero(np.diff(half, prepend=-1))           # the first hunk of a half
        group = half // 2
        u = rng.random((B, R))
        p1 = np.where(half[I] == half[J], 0.9 + 0.1 * u,
                      np.where(group[I] == group[J], 0.25 + 0.05 * u, 0.2 * u))
        wrong = (group[I] == group[J]) & (half[I] != half[J]) & np.isin(I, first) & np.isin(J, first)
        p1[:, wrong] = 0.97
        y = np.broadcast_to((half[:, None] == half[None, :]).astype(np.uint8), (B, nc, nc)).copy()
        start = np.ascontiguousarray(np.broadcast_to(group, (B, nc)), np.int32)
        return y, p1.astype(np.float32), start
    if kind == "sparse":
        on = np.triu(rng.random((B, nc, nc)) < 0.25, 1)
        on = (on | on.transpose(0, 2, 1))[:, I, J] & same
        p1 = np.where(on, 0.75, 0.0).astype(np.float32) + 0.25 * rng.random((B, R), dtype=np.float32)
    else:
        p1 = np.clip(np.where(same, 0.65, 0.35) + 0.25 * rng.standard_normal((B, R)), 0.0, 1.0)
    return y, p1.astype(np.float32), None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--rule", default="mean", choices=("mean", "any", "both"))
    ap.add_argument("--out", default=os.path.join(ROOT, "bench_out", "refine_split_time.json"))
    a = ap.parse_args()
    import numpy as np
    import torch
    from hdgnn import _lib, data, metrics
    lib = _lib.load()
    dev = torch.device("cuda", torch.cuda.current_device())
    stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    vp = ctypes.c_void_p
    rule = _lib.UT_RULES[a.rule]
    rungs = metrics.ladder(*LADDER)
    T = len(rungs)
    carr = (ctypes.c_float * T)(*[float(t) for t in rungs])
    rows = []

    def per_call(fn):
        for _ in range(a.warmup):
            fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.launches):
            fn()
        e1.record()
        torch.cuda.synchronize(dev)
        return e0.elapsed_time(e1) / a.launches

    def pairs(merge, split):
        m, s = [], []
        for _ in range(a.pairs):                    # interleaved
            m.append(per_call(merge))
            s.append(per_call(split))
        return m, s

    for name, ne, nc, B in SHAPES:
        for kind in ("sparse", "noisy", "fused"):
            y, p1, fused = scores(kind, nc, B, np, data)
            label = data.onehot_relations(y)
            ybits = torch.from_numpy(data.pack_bits(y).view(np.int32)).to(dev)
            host_probs = np.ascontiguousarray(np.stack([1.0 - p1, p1], 1), np.float32)
            probs = torch.from_numpy(host_probs).to(dev)
            shape = _lib.Shape(B, ne, nc, 2, B, 0)
            bt = _lib.Batch(None, None, ybits.data_ptr(), None, None, None)

            def empty(*shp, dtype=torch.int32):
                return torch.empty(*shp, dtype=dtype, device=dev)

            sh, pb = ctypes.byref(shape), ctypes.byref(bt)
            ws = empty(lib.hdg_refine_workspace_bytes(sh, 0) // 8, dtype=torch.int64)
            start = tree = None
            if kind == "sparse":                    # the starts of refine_time / refine_ladder_time
                start, sut = empty(B, nc), empty(B, _lib.UT_SLOTS, dtype=torch.int64)
                uws = empty(lib.hdg_untangle_workspace_bytes(sh) // 4)
                _lib.check(lib.hdg_untangle(sh, pb, vp(probs.data_ptr()), ctypes.c_float(THR), rule,
                                            vp(start.data_ptr()), None, vp(sut.data_ptr()),
                                            vp(uws.data_ptr()), stream))
            if kind == "fused":
                start = torch.from_numpy(fused).to(dev).contiguous()
            if kind != "noisy":
                method = "average" if kind == "sparse" else "single"
                tree = (empty(B, nc - 1, 2), empty(B, nc - 1, dtype=torch.float32))
                curve, lk = empty(B, nc - 1, 2), empty(B, _lib.LK_SLOTS, dtype=torch.int64)
                aws = empty(lib.hdg_agglomerate_workspace_bytes(sh, 0) // 4)
                _lib.check(lib.hdg_agglomerate(sh, pb, vp(probs.data_ptr()), rule,
                                               _lib.AG_METHODS[method], 0,
                                               vp(tree[0].data_ptr()), vp(tree[1].data_ptr()),
                                               vp(curve.data_ptr()), None, vp(lk.data_ptr()),
                                               vp(aws.data_ptr()), stream))
            gin = None if start is None else vp(start.data_ptr())
            tm = None if tree is None else vp(tree[0].data_ptr())
            tl = None if tree is None else vp(tree[1].data_ptr())
            g, ut = empty(B, nc), empty(B, _lib.RF_SLOTS, dtype=torch.int64)
            mrq, srq = (empty(B, n, dtype=torch.int64) for n in (_lib.RM_Q_SLOTS, _lib.RS_Q_SLOTS))
            lg, lut = empty(T, B, nc), empty(T, B, _lib.RF_SLOTS, dtype=torch.int64)
            lmrq, lsrq = (empty(T, B, n, dtype=torch.int64)
                          for n in (_lib.RM_Q_SLOTS, _lib.RS_Q_SLOTS))

            def refine_split():
                _lib.check(lib.hdg_refine_split(sh, pb, vp(probs.data_ptr()), ctypes.c_float(THR),
                                                rule, SWEEPS, ROUNDS, KINDS, 0, gin,
                                                vp(g.data_ptr()), vp(ut.data_ptr()),
                                                vp(srq.data_ptr()), vp(ws.data_ptr()), stream))

            def refine_merge():
                _lib.check(lib.hdg_refine_merge(sh, pb, vp(probs.data_ptr()), ctypes.c_float(THR),
                                                rule, SWEEPS, ROUNDS, 0, gin, vp(g.data_ptr()),
                                                vp(ut.data_ptr()), vp(mrq.data_ptr()),
                                                vp(ws.data_ptr()), stream))

            def split_ladder():
                _lib.check(lib.hdg_refine_split_ladder(sh, pb, vp(probs.data_ptr()), carr, T, rule,
                                                       SWEEPS, ROUNDS, KINDS, 0, tm, tl,
                                                       vp(lg.data_ptr()), vp(lut.data_ptr()),
                                                       vp(lsrq.data_ptr()), vp(ws.data_ptr()),
                                                       stream))

            def merge_ladder():
                _lib.check(lib.hdg_refine_merge_ladder(sh, pb, vp(probs.data_ptr()), carr, T, rule,
                                                       SWEEPS, ROUNDS, 0, tm, tl,
                                                       vp(lg.data_ptr()), vp(lut.data_ptr()),
                                                       vp(lmrq.data_ptr()), vp(ws.data_ptr()),
                                                       stream))

            def read(fn, *outs):
                fn()
                torch.cuda.synchronize(dev)
                return [x.cpu().numpy() for x in outs]

            hstart = None if start is None else start.cpu().numpy()
            htree = None if tree is None else (tree[0].cpu().numpy(), tree[1].cpu().numpy())
            checks = (
                (read(refine_merge, ut, g, mrq),
                 metrics.refine_merge(label, host_probs, hstart, THR, a.rule, SWEEPS, ROUNDS)),
                (read(refine_split, ut, g, srq),
                 metrics.refine_split(label, host_probs, hstart, THR, a.rule, SWEEPS, ROUNDS,
                                      KINDS)),
                (read(merge_ladder, lut, lg, lmrq),
                 metrics.refine_merge_ladder(label, host_probs, rungs, htree, a.rule, SWEEPS,
                                             ROUNDS)),
                (read(split_ladder, lut, lg, lsrq),
                 metrics.refine_split_ladder(label, host_probs, rungs, htree, a.rule, SWEEPS,
                                             ROUNDS, KINDS)))
            for k, (d, h) in enumerate(checks):
                for x, z in zip(d, h):
                    if not np.array_equal(x, z):
                        raise SystemExit("%s %s: device and host results differ (call %d)"
                                         % (name, kind, k))
            (mut, _, mq), (sut, _, sq), (mlut, _, _), (slut, _, slq) = (c[0] for c in checks)
            one_m, one_s = pairs(refine_merge, refine_split)
            lad_m, lad_s = pairs(merge_ladder, split_ladder)
            starts = {"sparse": ("hdg_untangle", "hdg_agglomerate average"),
                      "noisy": ("singletons", "singletons"),
                      "fused": ("the fused groups", "hdg_agglomerate single")}[kind]
            row = {"shape": name, "ne": ne, "nc": nc, "batch": B, "rule": a.rule, "scores": kind,
                   "threshold": THR, "max_sweeps": SWEEPS, "max_rounds": ROUNDS, "kinds": KINDS,
                   "start": starts[0], "ladder_start": starts[1],
                   "rungs": T, "ladder": list(LADDER), "checked_against": "host",
                   "launches": a.launches, "warmup": a.warmup,
                   "refine_merge_ms_per_call": one_m, "refine_split_ms_per_call": one_s,
                   "refine_merge_ms_median": statistics.median(one_m),
                   "refine_split_ms_median": statistics.median(one_s),
                   "split_over_merge": statistics.median(one_s) / statistics.median(one_m),
                   "merge_ladder_ms_per_call": lad_m, "split_ladder_ms_per_call": lad_s,
                   "merge_ladder_ms_median": statistics.median(lad_m),
                   "split_ladder_ms_median": statistics.median(lad_s),
                   "split_ladder_over_merge_ladder":
                       statistics.median(lad_s) / statistics.median(lad_m),
                   "splits_per_commit": float(sq[:, _lib.RS_Q_SPLITS].mean()),
                   "rounds_per_commit": [float(mq[:, _lib.RM_Q_ROUNDS].mean()),
                                         float(sq[:, _lib.RM_Q_ROUNDS].mean())],
                   "merges_per_commit": [float(mq[:, _lib.RM_Q_MERGES].mean()),
                                         float(sq[:, _lib.RM_Q_MERGES].mean())],
                   "node_sweeps_per_commit": [float(mq[:, _lib.RF_Q_SWEEPS].mean()),
                                              float(sq[:, _lib.RF_Q_SWEEPS].mean())],
                   "q_end": [int(mq[:, _lib.RF_Q_END].sum()), int(sq[:, _lib.RF_Q_END].sum())],
                   "f1": [metrics.scores_from_untangle(mut)["f1"],
                          metrics.scores_from_untangle(sut)["f1"]],
                   "ladder_splits_per_rung": slq[:, :, _lib.RS_Q_SPLITS].sum(1).tolist(),
                   "ladder_rounds_mean_per_rung": slq[:, :, _lib.RM_Q_ROUNDS].mean(1).tolist(),
                   "ladder_best_f1": [metrics.best_rung(mlut, rungs, "f1")[2],
                                      metrics.best_rung(slut, rungs, "f1")[2]]}
            print(json.dumps(row), flush=True)
            rows.append(row)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
