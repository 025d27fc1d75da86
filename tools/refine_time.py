"""GPU box: time of one hdg_refine call (two launches) from hdg_untangle's groups at threshold
0.5, with max_sweeps 1 and 8, next to the device-to-host copy of probs and the host
restatement, at the glide shape (200x74, B=100) and the stress shape (1024x512, B=32).

  device    events around --launches (20) hdg_refine calls after --warmup (5), per call
  untangle  the same around the hdg_untangle call that gives the starting groups
  host      the device-to-host copy of probs, then hdgnn.metrics.refine on it (once each, wall
            clock)

Scores as tools/linkage_time.py, rule mean.  Before anything is timed groups, ut and rq are
compared with the host's.  The rows also carry the sweeps the commits actually ran, the moves
made, the commits converged and the pooled f1 before and after.  Prints one JSON line per
shape and max_sweeps and writes them to --out (default bench_out/refine_time.json).

  python tools/refine_time.py [--launches 20] [--warmup 5] [--out PATH]
"""
import argparse
import ctypes
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "hd-gnn_amd")]

SHAPES = [("glide", 200, 74, 100), ("stress", 1024, 512, 32)]
SWEEPS = (1, 8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rule", default="mean", choices=("mean", "any", "both"))
    ap.add_argument("--out", default=os.path.join(ROOT, "bench_out", "refine_time.json"))
    a = ap.parse_args()
    import numpy as np
    import torch
    from hdgnn import _lib, data, metrics
    lib = _lib.load()
    dev = torch.device("cuda", torch.cuda.current_device())
    stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    vp = ctypes.c_void_p
    thr = 0.5
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
        start = torch.empty(B, nc, dtype=torch.int32, device=dev)
        sut = torch.empty(B, _lib.UT_SLOTS, dtype=torch.int64, device=dev)
        groups = torch.empty(B, nc, dtype=torch.int32, device=dev)
        ut = torch.empty(B, _lib.RF_SLOTS, dtype=torch.int64, device=dev)
        rq = torch.empty(B, _lib.RF_Q_SLOTS, dtype=torch.int64, device=dev)
        uws = torch.empty(lib.hdg_untangle_workspace_bytes(ctypes.byref(shape)) // 4,
                          dtype=torch.int32, device=dev)
        ws = torch.empty(lib.hdg_refine_workspace_bytes(ctypes.byref(shape), 0) // 8,
                         dtype=torch.int64, device=dev)

        def untangle():
            _lib.check(lib.hdg_untangle(ctypes.byref(shape), ctypes.byref(bt), vp(probs.data_ptr()),
                                        ctypes.c_float(thr), _lib.UT_RULES[a.rule],
                                        vp(start.data_ptr()), None, vp(sut.data_ptr()),
                                        vp(uws.data_ptr()), stream))

        def refine(ms):
            _lib.check(lib.hdg_refine(ctypes.byref(shape), ctypes.byref(bt), vp(probs.data_ptr()),
                                      ctypes.c_float(thr), _lib.UT_RULES[a.rule], ms, 0,
                                      vp(start.data_ptr()), vp(groups.data_ptr()),
                                      vp(ut.data_ptr()), vp(rq.data_ptr()), vp(ws.data_ptr()),
                                      stream))

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

        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        host_probs = probs.cpu().numpy()
        copy_ms = (time.perf_counter() - t0) * 1e3
        untangle()
        torch.cuda.synchronize(dev)
        host_start, before = start.cpu().numpy(), sut.cpu().numpy()
        untangle_ms = per_call(untangle)
        for ms in SWEEPS:
            refine(ms)
            torch.cuda.synchronize(dev)
            dg, dut, drq = groups.cpu().numpy(), ut.cpu().numpy(), rq.cpu().numpy()
            t1 = time.perf_counter()
            hut, hg, hrq = metrics.refine(label, host_probs, host_start, thr, a.rule, ms)
            host_ms = (time.perf_counter() - t1) * 1e3
            if not (np.array_equal(dg, hg) and np.array_equal(dut, hut) and np.array_equal(drq, hrq)):
                raise SystemExit("%s max_sweeps %d: device and host results differ" % (name, ms))
            row = {"shape": name, "ne": ne, "nc": nc, "batch": B, "rule": a.rule, "threshold": thr,
                   "start": "hdg_untangle", "max_sweeps": ms, "checked_against": "host",
                   "refine_ms_per_call": per_call(lambda: refine(ms)),
                   "untangle_ms_per_call": untangle_ms, "launches": a.launches, "warmup": a.warmup,
                   "host_copy_ms": copy_ms, "host_refine_ms": host_ms,
                   "probs_mbytes": B * 2 * R * 4 / 1e6, "workspace_mbytes": ws.numel() * 8 / 1e6,
                   "sweeps_mean": float(drq[:, _lib.RF_Q_SWEEPS].mean()),
                   "sweeps_max": int(drq[:, _lib.RF_Q_SWEEPS].max()),
                   "moves": int(dut[:, _lib.RF_MOVES].sum()),
                   "converged": int(drq[:, _lib.RF_Q_CONVERGED].sum()),
                   "q_start": int(drq[:, _lib.RF_Q_START].sum()),
                   "q_end": int(drq[:, _lib.RF_Q_END].sum()),
                   "f1_start": metrics.scores_from_untangle(before)["f1"],
                   "f1_end": metrics.scores_from_untangle(dut)["f1"]}
            print(json.dumps(row), flush=True)
            rows.append(row)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
