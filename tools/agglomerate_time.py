"""GPU box: time of one hdg_agglomerate call (three launches) per linkage method, next to one
hdg_linkage call, the device-to-host copy of probs and the host restatement, at the glide
shape (200x74, B=100), the stress shape (1024x512, B=32) and the largest nc (2048, B=8).

  device    events around --launches (20) hdg_agglomerate calls after --warmup (5), per call
  linkage   the same around hdg_linkage calls (single linkage by Boruvka rounds, many blocks)
  host      the device-to-host copy of probs, then hdgnn.metrics.agglomerate on it (once each,
            wall clock) where the host is affordable: not at nc = 2048

Scores as tools/linkage_time.py.  Before anything is timed all five outputs of every method
are compared with the host's; at nc = 2048 single linkage is compared with hdg_linkage
instead (levels, lk, and the curve at reachable cuts) and the other methods are only checked
for non-increasing levels.  --global adds the workspace home of the matrix at the shapes that
fit LDS.  Prints one JSON line per shape and method and writes them to --out (default
bench_out/agglomerate_time.json).

  python tools/agglomerate_time.py [--launches 20] [--warmup 5] [--global] [--out PATH]
"""
import argparse
import ctypes
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "hd-gnn_amd")]

SHAPES = [("glide", 200, 74, 100, True), ("stress", 1024, 512, 32, True),
          ("nc2048", 1024, 2048, 8, False)]
METHODS = ("single", "complete", "average")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--global", dest="glob", action="store_true")
    ap.add_argument("--rule", default="mean", choices=("mean", "any", "both"))
    ap.add_argument("--out", default=os.path.join(ROOT, "bench_out", "agglomerate_time.json"))
    a = ap.parse_args()
    import numpy as np
    import torch
    from hdgnn import _lib, data, metrics
    lib = _lib.load()
    dev = torch.device("cuda", torch.cuda.current_device())
    stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    vp = ctypes.c_void_p
    rows = []
    for name, ne, nc, B, host_ok in SHAPES:
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

        def outputs():
            return (torch.empty(B, nc - 1, 2, dtype=torch.int32, device=dev),
                    torch.empty(B, nc - 1, dtype=torch.float32, device=dev),
                    torch.empty(B, nc - 1, 2, dtype=torch.int32, device=dev),
                    torch.empty(B, nc, dtype=torch.int32, device=dev),
                    torch.empty(B, _lib.LK_SLOTS, dtype=torch.int64, device=dev))

        out, lout = outputs(), outputs()
        ws = torch.empty(lib.hdg_agglomerate_workspace_bytes(ctypes.byref(shape), 0) // 4,
                         dtype=torch.float32, device=dev)
        lws = torch.empty(lib.hdg_linkage_workspace_bytes(ctypes.byref(shape)) // 8,
                          dtype=torch.int64, device=dev)

        def launch(method, flags=0):
            _lib.check(lib.hdg_agglomerate(ctypes.byref(shape), ctypes.byref(bt),
                                           vp(probs.data_ptr()), _lib.UT_RULES[a.rule],
                                           _lib.AG_METHODS[method], flags,
                                           *[vp(x.data_ptr()) for x in out], vp(ws.data_ptr()),
                                           stream))

        def launch_linkage():
            _lib.check(lib.hdg_linkage(ctypes.byref(shape), ctypes.byref(bt), vp(probs.data_ptr()),
                                       _lib.UT_RULES[a.rule], *[vp(x.data_ptr()) for x in lout],
                                       vp(lws.data_ptr()), stream))

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

        def read(bufs):
            torch.cuda.synchronize(dev)
            return tuple(x.cpu().numpy() for x in bufs)

        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        host_probs = probs.cpu().numpy()
        copy_ms = (time.perf_counter() - t0) * 1e3
        launch_linkage()
        lm, ll, lc, lt, lkk = read(lout)
        linkage_ms = per_call(launch_linkage)
        homes = [0] + ([_lib.AG_FLAG_GLOBAL] if a.glob and nc <= _lib.AG_LDS_MAX_NC else [])
        for method in METHODS:
            host_ms = None
            launch(method)
            dm, dl, dc, dt, dk = read(out)
            if host_ok:
                t1 = time.perf_counter()
                hm, hl, hc, ht, hk = metrics.agglomerate(label, host_probs, a.rule, method)
                host_ms = (time.perf_counter() - t1) * 1e3
                real = ~np.isnan(hl)
                if not (np.array_equal(dm, hm) and np.array_equal(dc, hc) and np.array_equal(dt, ht)
                        and np.array_equal(dk, hk) and np.array_equal(np.isnan(dl), ~real)
                        and np.array_equal(dl.view(np.uint32)[real], hl.view(np.uint32)[real])):
                    raise SystemExit("%s %s: device and host results differ" % (name, method))
                checked = "host"
            elif method == "single":
                same = (np.array_equal(dl.view(np.uint32), ll.view(np.uint32))
                        and np.array_equal(dk, lkk) and np.array_equal(dt, lt))
                for b in range(B):
                    M = int(dk[b, _lib.LK_MERGES])
                    reach = np.flatnonzero(np.append(dl[b, 1:M], -np.inf) < dl[b, :M])
                    same = same and np.array_equal(dc[b, reach], lc[b, reach])
                if not same:
                    raise SystemExit("%s single: hdg_agglomerate and hdg_linkage differ" % name)
                checked = "hdg_linkage"
            else:
                if (np.diff(dl, axis=1) > 0).any() or (dk[:, _lib.LK_TGROUPS] != lkk[:, _lib.LK_TGROUPS]).any():
                    raise SystemExit("%s %s: levels increase" % (name, method))
                checked = "levels only"
            thr, best, _ = metrics.best_threshold(dl, dc.astype(np.int64), dk, a.rule, "f1")
            for flags in homes:
                row = {"shape": name, "ne": ne, "nc": nc, "batch": B, "rule": a.rule,
                       "method": method,
                       "home": "lds" if nc <= _lib.AG_LDS_MAX_NC and not flags else "workspace",
                       "checked_against": checked,
                       "agglomerate_ms_per_call": per_call(lambda: launch(method, flags)),
                       "linkage_ms_per_call": linkage_ms, "launches": a.launches,
                       "warmup": a.warmup, "host_copy_ms": copy_ms, "host_agglomerate_ms": host_ms,
                       "probs_mbytes": B * 2 * R * 4 / 1e6,
                       "workspace_mbytes": B * nc * nc * 4 / 1e6,
                       "merges_mean": float(dk[:, _lib.LK_MERGES].mean()),
                       "best_threshold": thr, "best_f1": best}
                print(json.dumps(row), flush=True)
                rows.append(row)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
