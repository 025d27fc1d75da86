"""GPU box: time of hdg_match against the path it replaces -- the device-to-host copy of the
group ids followed by hdgnn.metrics.match_counts in numpy.

Cases (noisy planted scores: 0.65 inside and 0.35 across + 0.25 sigma noise, every hunk alone
at the start, at most 8 node sweeps and 4 rounds, kinds both):
  glide 200x74, B=100   the 19 rungs hdg_refine_split_ladder leaves on the device, in one call
                        (S = 19), and the rung at 0.5 alone (S = 1)
  stress 1024x512, B=32 hdg_refine_split's groups at 0.5 (S = 1)
  worst                 the staircase of the tests (K = 64, the contender row last), one commit
                        (nc = 258), timed ONCE after one warm-up call: 65 rows of the
                        residual graph, the last one's path through all of them; the row
                        holds the iteration counts the header's bounds give for it

Events around --launches (20) calls after --warmup (5); the copy and the host time are single
wall-clock readings.  Before anything is timed mt and tgroups are compared with the host's and
mate must match exactly MATCHED hunks.  Prints one JSON line per case and writes them to --out
(default bench_out/match_time.json).

  python tools/match_time.py [--launches 20] [--warmup 5] [--out PATH]
"""
import argparse
import ctypes
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "hd-gnn_amd")]

LADDER = (0.05, 0.95, 19)
SWEEPS, ROUNDS, THR, KINDS = 8, 4, 0.5, 3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "bench_out", "match_time.json"))
    a = ap.parse_args()
    import numpy as np
    import torch
    from hdgnn import _lib, data, metrics
    lib = _lib.load()
    dev = torch.device("cuda", torch.cuda.current_device())
    stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    vp = ctypes.c_void_p
    rungs = metrics.ladder(*LADDER)
    T = len(rungs)
    carr = (ctypes.c_float * T)(*[float(t) for t in rungs])
    rows = []

    def empty(*shp, dtype=torch.int32):
        return torch.empty(*shp, dtype=dtype, device=dev)

    def per_call(fn, launches, warmup):
        for _ in range(warmup):
            fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(launches):
            fn()
        e1.record()
        torch.cuda.synchronize(dev)
        return e0.elapsed_time(e1) / launches

    def case(name, ne, y, groups, launches, warmup, **more):
        """y (B, nc, nc) uint8 labels, groups int32 [S][B][nc] on the device."""
        S, B, nc = groups.shape
        label = data.onehot_relations(y)
        ybits = torch.from_numpy(data.pack_bits(y).view(np.int32)).to(dev)
        shape = _lib.Shape(B, ne, nc, 2, B, 0)
        bt = _lib.Batch(None, None, ybits.data_ptr(), None, None, None)
        sh, pb = ctypes.byref(shape), ctypes.byref(bt)
        ws = empty(lib.hdg_match_workspace_bytes(sh, S) // 8, dtype=torch.int64)
        mt, mate, tg = empty(S, B, _lib.MT_SLOTS, dtype=torch.int64), empty(S, B, nc), empty(B, nc)

        def match():
            _lib.check(lib.hdg_match(sh, pb, vp(groups.data_ptr()), S, vp(mate.data_ptr()),
                                     vp(tg.data_ptr()), vp(mt.data_ptr()), vp(ws.data_ptr()),
                                     stream))

        match()
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        hg = groups.cpu().numpy()
        t1 = time.perf_counter()
        hmt, _, htg = metrics.match_counts(label, hg)
        t2 = time.perf_counter()
        dmt, dtg, dmate = mt.cpu().numpy(), tg.cpu().numpy(), mate.cpu().numpy()
        if not (np.array_equal(dmt, hmt) and np.array_equal(dtg, htg)):
            raise SystemExit("%s: device and host results differ" % name)
        if not np.array_equal((dmate == dtg[None]).sum(-1), dmt[..., _lib.MT_MATCHED]):
            raise SystemExit("%s: mate does not match MATCHED hunks" % name)
        ms = per_call(match, launches, warmup)
        sc = [metrics.scores_from_match(hmt[k], nc) for k in range(S)]
        row = {"case": name, "ne": ne, "nc": nc, "batch": B, "sets": S, "checked_against": "host",
               "launches": launches, "warmup": warmup, "match_ms_per_call": ms,
               "copy_ids_ms": (t1 - t0) * 1e3, "host_match_counts_ms": (t2 - t1) * 1e3,
               "cells_per_commit": float(hmt[..., _lib.MT_CELLS].mean()),
               "isolated_per_commit": float(hmt[..., _lib.MT_ISOLATED].mean()),
               "accuracy_per_set": [s["accuracy"] for s in sc],
               "purity_per_set": [s["purity"] for s in sc],
               "cover_per_set": [s["cover"] for s in sc]}
        row.update(more)
        print(json.dumps(row), flush=True)
        rows.append(row)

    def noisy(nc, B):
        rng = np.random.default_rng(nc)
        I, J = data.pair_index(nc)
        grp = rng.integers(0, max(2, nc // 12), (B, nc))
        y = (grp[:, :, None] == grp[:, None, :]).astype(np.uint8)     # pack_bits clears the diagonal
        same = grp[:, I] == grp[:, J]
        p1 = np.clip(np.where(same, 0.65, 0.35) + 0.25 * rng.standard_normal(same.shape), 0.0, 1.0)
        return y, np.ascontiguousarray(np.stack([1.0 - p1, p1], 1), np.float32)

    for name, ne, nc, B, ladder in (("glide", 200, 74, 100, True), ("stress", 1024, 512, 32, False)):
        y, host_probs = noisy(nc, B)
        probs = torch.from_numpy(host_probs).to(dev)
        ybits = torch.from_numpy(data.pack_bits(y).view(np.int32)).to(dev)
        shape = _lib.Shape(B, ne, nc, 2, B, 0)
        bt = _lib.Batch(None, None, ybits.data_ptr(), None, None, None)
        sh, pb = ctypes.byref(shape), ctypes.byref(bt)
        size = lib.hdg_refine_ladder_workspace_bytes if ladder else lib.hdg_refine_workspace_bytes
        rws = empty(size(sh, 0) // 8, dtype=torch.int64)
        if ladder:
            lg, lut = empty(T, B, nc), empty(T, B, _lib.RF_SLOTS, dtype=torch.int64)
            lrq = empty(T, B, _lib.RS_Q_SLOTS, dtype=torch.int64)
            _lib.check(lib.hdg_refine_split_ladder(sh, pb, vp(probs.data_ptr()), carr, T, 0, SWEEPS,
                                                   ROUNDS, KINDS, 0, None, None, vp(lg.data_ptr()),
                                                   vp(lut.data_ptr()), vp(lrq.data_ptr()),
                                                   vp(rws.data_ptr()), stream))
            torch.cuda.synchronize(dev)
            case(name + " ladder", ne, y, lg, a.launches, a.warmup,
                 groups_from="hdg_refine_split_ladder, 19 rungs")
            case(name + " one rung", ne, y, lg[T // 2:T // 2 + 1].contiguous(), a.launches,
                 a.warmup, groups_from="the rung at %r" % float(rungs[T // 2]))
        else:
            g, ut = empty(1, B, nc), empty(B, _lib.RF_SLOTS, dtype=torch.int64)
            rq = empty(B, _lib.RS_Q_SLOTS, dtype=torch.int64)
            _lib.check(lib.hdg_refine_split(sh, pb, vp(probs.data_ptr()), ctypes.c_float(THR), 0,
                                            SWEEPS, ROUNDS, KINDS, 0, None, vp(g.data_ptr()),
                                            vp(ut.data_ptr()), vp(rq.data_ptr()),
                                            vp(rws.data_ptr()), stream))
            torch.cuda.synchronize(dev)
            case(name, ne, y, g, a.launches, a.warmup, groups_from="hdg_refine_split at 0.5")

    # the staircase: two hunks per cell, rows i < K with the cells (i, i) and (i, i + 1), then the
    # row K with the single cell (K, 0) as the highest group id
    K = 64
    pred = np.array([i for i in range(K) for _ in range(4)] + [K, K], np.int32)
    true = np.array([i + j for i in range(K) for j in (0, 0, 1, 1)] + [0, 0], np.int32)
    grid = (true[:, None] == true[None, :]).astype(np.uint8)[None]
    case("worst: staircase(64, last)", 20, grid,
         torch.from_numpy(pred[None, None]).to(dev).contiguous(),
         1, 1, residual_rows=K + 1, augmentations_at_most=K + 1,
         columns_per_path_at_most=K + 2, steps_at_most=(K + 1) * (K + 2),
         barriers_per_step=2)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
