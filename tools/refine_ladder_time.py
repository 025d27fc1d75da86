"""GPU box: time of one hdg_refine_ladder call (two launches: 19 rungs, at most 8 sweeps, the
start cut from hdg_agglomerate's AVERAGE tree) against the 19 hdg_cut + hdg_refine sequences it
replaces (57 launches) on the same inputs in the same process, at the glide shape (200x74,
B=100) and the stress shape (1024x512, B=32).

  ladder     events around --launches (20) hdg_refine_ladder calls after --warmup (5), per call
  sequences  the same around 20 x (19 x (hdg_cut, hdg_refine)), per 19 sequences

--pairs (3) interleaved pairs (ladder, sequences) per shape; the medians and their ratio are
in the row.  Scores as tools/linkage_time.py, rule mean, rungs metrics.ladder(0.05, 0.95, 19).
Before anything is timed the ladder's ut, groups and rq are compared with
hdgnn.metrics.refine_ladder on the host (from the device's tree) and with the sequences'
outputs.  The rows also carry, per rung, the pooled f1, the moves and the sweeps run.  Prints
one JSON line per shape and writes them to --out (default bench_out/refine_ladder_time.json).

  python tools/refine_ladder_time.py [--launches 20] [--warmup 5] [--pairs 3] [--out PATH]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "hd-gnn_amd")]

SHAPES = [("glide", 200, 74, 100), ("stress", 1024, 512, 32)]
LADDER = (0.05, 0.95, 19)
SWEEPS = 8


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--rule", default="mean", choices=("mean", "any", "both"))
    ap.add_argument("--out", default=os.path.join(ROOT, "bench_out", "refine_ladder_time.json"))
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
    thr = [float(t) for t in rungs]
    carr = (ctypes.c_float * T)(*thr)
    rows = []
    for name, ne, nc, B in SHAPES:
        R = nc * (nc - 1)
        rng = np.random.default_rng(nc)
        I, J = data.pair_index(nc)
        grp = rng.integers(0, max(2, nc // 12), (B, nc))
        y = (grp[:, :, None] == grp[:, None, :]).astype(np.uint8)     # pack_bits clears the diagonal
        label = data.onehot_relations(y)
        ybits = torch.from_numpy(data.pack_bits(y).view(np.int32)).to(dev)
        on = np.triu(rng.random((B, nc, nc)) < 0.25, 1)
        on = (on | on.transpose(0, 2, 1))[:, I, J] & (grp[:, I] == grp[:, J])
        p1 = np.where(on, 0.75, 0.0).astype(np.float32) + 0.25 * rng.random((B, R), dtype=np.float32)
        probs = torch.from_numpy(np.ascontiguousarray(np.stack([1.0 - p1, p1], 1), np.float32)).to(dev)
        shape = _lib.Shape(B, ne, nc, 2, B, 0)
        bt = _lib.Batch(None, None, ybits.data_ptr(), None, None, None)

        def empty(*shp, dtype=torch.int32):
            return torch.empty(*shp, dtype=dtype, device=dev)

        merges, levels = empty(B, nc - 1, 2), empty(B, nc - 1, dtype=torch.float32)
        curve, lk = empty(B, nc - 1, 2), empty(B, _lib.LK_SLOTS, dtype=torch.int64)
        aws = empty(lib.hdg_agglomerate_workspace_bytes(ctypes.byref(shape), 0) // 4)
        # the ladder's outputs, and the sequences': one slice per rung, so both can be compared
        lg, sg = empty(T, B, nc), empty(T, B, nc)
        lut, sut = (empty(T, B, _lib.RF_SLOTS, dtype=torch.int64) for _ in range(2))
        lrq, srq = (empty(T, B, _lib.RF_Q_SLOTS, dtype=torch.int64) for _ in range(2))
        start = empty(B, nc)
        lws = empty(lib.hdg_refine_ladder_workspace_bytes(ctypes.byref(shape), 0) // 8,
                    dtype=torch.int64)
        rws = empty(lib.hdg_refine_workspace_bytes(ctypes.byref(shape), 0) // 8, dtype=torch.int64)
        _lib.check(lib.hdg_agglomerate(ctypes.byref(shape), ctypes.byref(bt), vp(probs.data_ptr()),
                                       rule, _lib.AG_METHODS["average"], 0, vp(merges.data_ptr()),
                                       vp(levels.data_ptr()), vp(curve.data_ptr()), None,
                                       vp(lk.data_ptr()), vp(aws.data_ptr()), stream))

        def ladder():
            _lib.check(lib.hdg_refine_ladder(ctypes.byref(shape), ctypes.byref(bt),
                                             vp(probs.data_ptr()), carr, T, rule, SWEEPS, 0,
                                             vp(merges.data_ptr()), vp(levels.data_ptr()),
                                             vp(lg.data_ptr()), vp(lut.data_ptr()),
                                             vp(lrq.data_ptr()), vp(lws.data_ptr()), stream))

        def sequences():
            for k in range(T):
                _lib.check(lib.hdg_cut(ctypes.byref(shape), vp(merges.data_ptr()),
                                       vp(levels.data_ptr()), None, None, ctypes.c_float(thr[k]),
                                       rule, vp(start.data_ptr()), None, stream))
                _lib.check(lib.hdg_refine(ctypes.byref(shape), ctypes.byref(bt),
                                          vp(probs.data_ptr()), ctypes.c_float(thr[k]), rule, SWEEPS,
                                          0, vp(start.data_ptr()), vp(sg[k].data_ptr()),
                                          vp(sut[k].data_ptr()), vp(srq[k].data_ptr()),
                                          vp(rws.data_ptr()), stream))

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

        ladder()
        sequences()
        torch.cuda.synchronize(dev)
        dev_out = [x.cpu().numpy() for x in (lut, lg, lrq)]
        for x, z in zip(dev_out, (sut, sg, srq)):
            if not np.array_equal(x, z.cpu().numpy()):
                raise SystemExit("%s: the ladder and the sequences differ" % name)
        t0 = time.perf_counter()
        host = metrics.refine_ladder(label, probs.cpu().numpy(), rungs,
                                     (merges.cpu().numpy(), levels.cpu().numpy()), a.rule, SWEEPS)
        host_ms = (time.perf_counter() - t0) * 1e3
        for x, z in zip(dev_out, host):
            if not np.array_equal(x, z):
                raise SystemExit("%s: device and host results differ" % name)
        lad, seq = [], []
        for _ in range(a.pairs):                    # interleaved
            lad.append(per_call(ladder))
            seq.append(per_call(sequences))
        dut, _, drq = dev_out
        k, best_thr, best, vals = metrics.best_rung(dut, rungs, "f1")
        row = {"shape": name, "ne": ne, "nc": nc, "batch": B, "rule": a.rule, "rungs": T,
               "ladder": list(LADDER), "max_sweeps": SWEEPS, "start": "hdg_agglomerate average",
               "checked_against": "host and sequences", "launches": a.launches, "warmup": a.warmup,
               "ladder_ms_per_call": lad, "sequences_ms_per_call": seq,
               "ladder_ms_median": statistics.median(lad),
               "sequences_ms_median": statistics.median(seq),
               "ladder_over_sequences": statistics.median(lad) / statistics.median(seq),
               "sweep_blocks": T * B, "host_ladder_ms": host_ms,
               "workspace_mbytes": lws.numel() * 8 / 1e6,
               "best_rung": k, "best_threshold": best_thr, "best_f1": best,
               "f1_per_rung": [float(v) for v in vals],
               "moves_per_rung": dut[:, :, _lib.RF_MOVES].sum(1).tolist(),
               "sweeps_mean_per_rung": drq[:, :, _lib.RF_Q_SWEEPS].mean(1).tolist(),
               "sweeps_max_per_rung": drq[:, :, _lib.RF_Q_SWEEPS].max(1).tolist(),
               "converged_per_rung": drq[:, :, _lib.RF_Q_CONVERGED].sum(1).tolist()}
        print(json.dumps(row), flush=True)
        rows.append(row)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
