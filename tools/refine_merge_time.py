"""GPU box: time of hdg_refine_merge against hdg_refine, and of hdg_refine_merge_ladder against
hdg_refine_ladder (19 rungs), on the same inputs in the same process, at the glide shape
(200x74, B=100) and the stress shape (1024x512, B=32), at most 8 node sweeps and 4 rounds.

Two sets of scores per shape:
  sparse  tools/refine_time.py's scores, the start hdg_untangle's groups (the ladder: the cut of
          hdg_agglomerate's AVERAGE tree): no merge is expected, so the difference is the
          price of one futile group sweep
  noisy   planted groups, 0.65 inside and 0.35 across + 0.25 sigma noise, every hunk alone at
          the start (the ladder: no tree): merges happen; the row carries the rounds and the
          merges per commit

Events around --launches (20) calls after --warmup (5), --pairs (3) interleaved pairs (plain,
merge) per case; the medians and their ratio are in the row.  Before anything is timed the
outputs of all four calls are compared with hdgnn.metrics on the host.  Prints one JSON line
per case and writes them to --out (default bench_out/refine_merge_time.json).

  python tools/refine_merge_time.py [--launches 20] [--warmup 5] [--pairs 3] [--out PATH]
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
SWEEPS, ROUNDS, THR = 8, 4, 0.5


def scores(kind, nc, B, np, data):
    """-> (labels (B, nc, nc) uint8, scores (B, R) float32)."""
    R = nc * (nc - 1)
    rng = np.random.default_rng(nc)
    I, J = data.pair_index(nc)
    grp = rng.integers(0, max(2, nc // 12), (B, nc))
    y = (grp[:, :, None] == grp[:, None, :]).astype(np.uint8)     # pack_bits clears the diagonal
    same = grp[:, I] == grp[:, J]
    if kind == "sparse":
        on = np.triu(rng.random((B, nc, nc)) < 0.25, 1)
        on = (on | on.transpose(0, 2, 1))[:, I, J] & same
        p1 = np.where(on, 0.75, 0.0).astype(np.float32) + 0.25 * rng.random((B, R), dtype=np.float32)
    else:
        p1 = np.clip(np.where(same, 0.65, 0.35) + 0.25 * rng.standard_normal((B, R)), 0.0, 1.0)
    return y, p1.astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--rule", default="mean", choices=("mean", "any", "both"))
    ap.add_argument("--out", default=os.path.join(ROOT, "bench_out", "refine_merge_time.json"))
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

    def pairs(plain, merge):
        p, m = [], []
        for _ in range(a.pairs):                    # interleaved
            p.append(per_call(plain))
            m.append(per_call(merge))
        return p, m

    for name, ne, nc, B in SHAPES:
        for kind in ("sparse", "noisy"):
            y, p1 = scores(kind, nc, B, np, data)
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
                tree = (empty(B, nc - 1, 2), empty(B, nc - 1, dtype=torch.float32))
                curve, lk = empty(B, nc - 1, 2), empty(B, _lib.LK_SLOTS, dtype=torch.int64)
                aws = empty(lib.hdg_agglomerate_workspace_bytes(sh, 0) // 4)
                _lib.check(lib.hdg_agglomerate(sh, pb, vp(probs.data_ptr()), rule,
                                               _lib.AG_METHODS["average"], 0,
                                               vp(tree[0].data_ptr()), vp(tree[1].data_ptr()),
                                               vp(curve.data_ptr()), None, vp(lk.data_ptr()),
                                               vp(aws.data_ptr()), stream))
            gin = None if start is None else vp(start.data_ptr())
            tm = None if tree is None else vp(tree[0].data_ptr())
            tl = None if tree is None else vp(tree[1].data_ptr())
            g, ut = empty(B, nc), empty(B, _lib.RF_SLOTS, dtype=torch.int64)
            rq, mrq = (empty(B, n, dtype=torch.int64) for n in (_lib.RF_Q_SLOTS, _lib.RM_Q_SLOTS))
            lg, lut = empty(T, B, nc), empty(T, B, _lib.RF_SLOTS, dtype=torch.int64)
            lrq, lmrq = (empty(T, B, n, dtype=torch.int64)
                         for n in (_lib.RF_Q_SLOTS, _lib.RM_Q_SLOTS))

            def refine():
                _lib.check(lib.hdg_refine(sh, pb, vp(probs.data_ptr()), ctypes.c_float(THR), rule,
                                          SWEEPS, 0, gin, vp(g.data_ptr()), vp(ut.data_ptr()),
                                          vp(rq.data_ptr()), vp(ws.data_ptr()), stream))

            def refine_merge():
                _lib.check(lib.hdg_refine_merge(sh, pb, vp(probs.data_ptr()), ctypes.c_float(THR),
                                                rule, SWEEPS, ROUNDS, 0, gin, vp(g.data_ptr()),
                                                vp(ut.data_ptr()), vp(mrq.data_ptr()),
                                                vp(ws.data_ptr()), stream))

            def ladder():
                _lib.check(lib.hdg_refine_ladder(sh, pb, vp(probs.data_ptr()), carr, T, rule,
                                                 SWEEPS, 0, tm, tl, vp(lg.data_ptr()),
                                                 vp(lut.data_ptr()), vp(lrq.data_ptr()),
                                                 vp(ws.data_ptr()), stream))

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
                (read(refine, ut, g, rq),
                 metrics.refine(label, host_probs, hstart, THR, a.rule, SWEEPS)),
                (read(refine_merge, ut, g, mrq),
                 metrics.refine_merge(label, host_probs, hstart, THR, a.rule, SWEEPS, ROUNDS)),
                (read(ladder, lut, lg, lrq),
                 metrics.refine_ladder(label, host_probs, rungs, htree, a.rule, SWEEPS)),
                (read(merge_ladder, lut, lg, lmrq),
                 metrics.refine_merge_ladder(label, host_probs, rungs, htree, a.rule, SWEEPS,
                                             ROUNDS)))
            for k, (d, h) in enumerate(checks):
                for x, z in zip(d, h):
                    if not np.array_equal(x, z):
                        raise SystemExit("%s %s: device and host results differ (call %d)"
                                         % (name, kind, k))
            (put, _, prq), (mut, _, mq), (plut, _, _), (mlut, _, mlq) = (c[0] for c in checks)
            one_p, one_m = pairs(refine, refine_merge)
            lad_p, lad_m = pairs(ladder, merge_ladder)
            row = {"shape": name, "ne": ne, "nc": nc, "batch": B, "rule": a.rule, "scores": kind,
                   "threshold": THR, "max_sweeps": SWEEPS, "max_rounds": ROUNDS,
                   "start": "hdg_untangle" if start is not None else "singletons",
                   "ladder_start": "hdg_agglomerate average" if tree is not None else "singletons",
                   "rungs": T, "ladder": list(LADDER), "checked_against": "host",
                   "launches": a.launches, "warmup": a.warmup,
                   "refine_ms_per_call": one_p, "refine_merge_ms_per_call": one_m,
                   "refine_ms_median": statistics.median(one_p),
                   "refine_merge_ms_median": statistics.median(one_m),
                   "merge_over_refine": statistics.median(one_m) / statistics.median(one_p),
                   "ladder_ms_per_call": lad_p, "merge_ladder_ms_per_call": lad_m,
                   "ladder_ms_median": statistics.median(lad_p),
                   "merge_ladder_ms_median": statistics.median(lad_m),
                   "merge_ladder_over_ladder": statistics.median(lad_m) / statistics.median(lad_p),
                   "rounds_per_commit": float(mq[:, _lib.RM_Q_ROUNDS].mean()),
                   "merges_per_commit": float(mq[:, _lib.RM_Q_MERGES].mean()),
                   "node_sweeps_per_commit": [float(prq[:, _lib.RF_Q_SWEEPS].mean()),
                                              float(mq[:, _lib.RF_Q_SWEEPS].mean())],
                   "q_end": [int(prq[:, _lib.RF_Q_END].sum()), int(mq[:, _lib.RF_Q_END].sum())],
                   "f1": [metrics.scores_from_untangle(put)["f1"],
                          metrics.scores_from_untangle(mut)["f1"]],
                   "ladder_merges_per_rung": mlq[:, :, _lib.RM_Q_MERGES].sum(1).tolist(),
                   "ladder_rounds_mean_per_rung": mlq[:, :, _lib.RM_Q_ROUNDS].mean(1).tolist(),
                   "ladder_best_f1": [metrics.best_rung(plut, rungs, "f1")[2],
                                      metrics.best_rung(mlut, rungs, "f1")[2]]}
            print(json.dumps(row), flush=True)
            rows.append(row)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
