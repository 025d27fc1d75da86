"""GPU box: time of one hdg_linkage call (two launches) against the host path it replaces and
against one hdg_untangle call (which answers one threshold), at the glide shape (200x74,
B=100) and the stress shape (1024x512, B=32); --nc2048 adds the largest nc (B=8).

  device    events around --launches (20) hdg_linkage calls after --warmup (5), per call
  untangle  the same around hdg_untangle calls at threshold 0.5
  host      the device-to-host copy of probs, then hdgnn.metrics.linkage on it (once each,
            wall clock)

Scores as tools/untangle_time.py: planted groups of about 12 hunks with sparse links (0.75
to 1.0) on a uniform background below 0.25; the labels are the planted groups, so the rows
also show what calibration buys: the pooled f1 at the default 0.5 and at the threshold
hdgnn.metrics.best_threshold finds.  All five outputs are compared with the host's before
anything is timed.  With a diagnostic library built with -DHDG_LK_STAMP_WALK
(HDG_HIPCC_FLAGS for hdgnn/build.py, loaded through HDG_LIB_PATH) the closing kernel stamps
its serial list walk with the 100 MHz clock into lk slot 7 (0 in the real library); the rows
then carry walk_us_mean / walk_us_max over the commits.  Prints one JSON line per shape and
writes them to --out (default bench_out/linkage_time.json).

  python tools/linkage_time.py [--launches 20] [--warmup 5] [--nc2048] [--out PATH]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--nc2048", action="store_true")
    ap.add_argument("--rule", default="mean", choices=("mean", "any", "both"))
    ap.add_argument("--out", default=os.path.join(ROOT, "bench_out", "linkage_time.json"))
    a = ap.parse_args()
    import numpy as np
    import torch
    from hdgnn import _lib, data, metrics
    lib = _lib.load()
    dev = torch.device("cuda", torch.cuda.current_device())
    stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    vp = ctypes.c_void_p
    rows = []
    for name, ne, nc, B in SHAPES + ([("nc2048", 1024, 2048, 8)] if a.nc2048 else []):
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
        merges = torch.empty(B, nc - 1, 2, dtype=torch.int32, device=dev)
        levels = torch.empty(B, nc - 1, dtype=torch.float32, device=dev)
        curve = torch.empty(B, nc - 1, 2, dtype=torch.int32, device=dev)
        tgroups = torch.empty(B, nc, dtype=torch.int32, device=dev)
        lk = torch.empty(B, _lib.LK_SLOTS, dtype=torch.int64, device=dev)
        ws = torch.empty(lib.hdg_linkage_workspace_bytes(ctypes.byref(shape)) // 8,
                         dtype=torch.int64, device=dev)
        groups = torch.empty(B, nc, dtype=torch.int32, device=dev)
        ut = torch.empty(B, _lib.UT_SLOTS, dtype=torch.int64, device=dev)
        uws = torch.empty(lib.hdg_untangle_workspace_bytes(ctypes.byref(shape)) // 4,
                          dtype=torch.int32, device=dev)

        def launch():
            _lib.check(lib.hdg_linkage(ctypes.byref(shape), ctypes.byref(bt), vp(probs.data_ptr()),
                                       _lib.UT_RULES[a.rule], vp(merges.data_ptr()),
                                       vp(levels.data_ptr()), vp(curve.data_ptr()),
                                       vp(tgroups.data_ptr()), vp(lk.data_ptr()),
                                       vp(ws.data_ptr()), stream))

        def launch_untangle():
            _lib.check(lib.hdg_untangle(ctypes.byref(shape), ctypes.byref(bt), vp(probs.data_ptr()),
                                        ctypes.c_float(0.5), _lib.UT_RULES[a.rule],
                                        vp(groups.data_ptr()), None, vp(ut.data_ptr()),
                                        vp(uws.data_ptr()), stream))

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

        launch()
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        host_probs = probs.cpu().numpy()
        t1 = time.perf_counter()
        hm, hl, hc, ht, hk = metrics.linkage(label, host_probs, a.rule)
        t2 = time.perf_counter()
        real = ~np.isnan(hl)
        dl, dk = levels.cpu().numpy(), lk.cpu().numpy()
        ticks = dk[:, 7].copy()                      # the walk's stamp in a diagnostic build
        dk[:, 7] = 0
        if not (np.array_equal(merges.cpu().numpy(), hm) and np.array_equal(curve.cpu().numpy(), hc)
                and np.array_equal(tgroups.cpu().numpy(), ht) and np.array_equal(dk, hk)
                and np.array_equal(np.isnan(dl), ~real)
                and np.array_equal(dl.view(np.uint32)[real], hl.view(np.uint32)[real])):
            raise SystemExit("%s: device and host results differ" % name)
        thr, best, tprime = metrics.best_threshold(hl, hc, hk, a.rule, "f1")
        at_half = metrics.scores_from_untangle(metrics.cut_table(hl, hc, hk, 1.0 if a.rule == "mean"
                                                                 else 0.5))
        row = {"shape": name, "ne": ne, "nc": nc, "batch": B, "rule": a.rule, "pairs": B * R // 2,
               "blocks_per_commit": _lib.untangle_blocks(nc),
               "linkage_ms_per_call": per_call(launch),
               "untangle_ms_per_call": per_call(launch_untangle),
               "launches": a.launches, "warmup": a.warmup,
               "host_copy_ms": (t1 - t0) * 1e3, "host_linkage_ms": (t2 - t1) * 1e3,
               "probs_mbytes": B * 2 * R * 4 / 1e6,
               "rows_to_host_kbytes": B * ((nc - 1) * 12 + _lib.LK_SLOTS * 8) / 1e3,
               "merges_mean": float(hk[:, _lib.LK_MERGES].mean()),
               "f1_at_0.5": at_half["f1"], "best_threshold": thr, "best_f1": best}
        if ticks.any():
            row["walk_us_mean"], row["walk_us_max"] = float(ticks.mean()) / 100.0, float(ticks.max()) / 100.0
        print(json.dumps(row), flush=True)
        rows.append(row)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
