"""GPU box: time of one hdg_untangle call (two launches) against the host path it replaces,
at the glide shape (200x74, B=100) and the stress shape (1024x512, B=32).

  device   events around --launches (20) hdg_untangle calls after --warmup (5), per call
  host     the device-to-host copy of probs, then hdgnn.metrics.untangle_counts on it (once)
  step     for scale: events around the same number of Engine.train_step calls on synthetic
           commits of the same shape (--no-step skips it)

Scores are planted groups of about 12 hunks with sparse links (a within-group pair is linked
with probability 0.25, both directions high) on a uniform background below the threshold,
labels hdgnn.synth's (symmetric, 10 % density); groups, true groups and the table are
compared with the host's before anything is timed.  Prints one JSON line per shape and
writes them to --out (default bench_out/untangle_time.json).

  python tools/untangle_time.py [--launches 20] [--warmup 5] [--no-step] [--out PATH]
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
    ap.add_argument("--no-step", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "bench_out", "untangle_time.json"))
    a = ap.parse_args()
    import numpy as np
    import torch
    from hdgnn import _lib, data, metrics
    from hdgnn.synth import synth_commits
    lib = _lib.load()
    dev = torch.device("cuda", torch.cuda.current_device())
    stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    rows = []
    for name, ne, nc, B in SHAPES:
        R = nc * (nc - 1)
        rng = np.random.default_rng(nc)
        y = synth_commits(B, 4, nc, 3).y             # only the hunk labels are used
        label = data.onehot_relations(y)
        ybits = torch.from_numpy(data.pack_bits(y).view(np.int32)).to(dev)
        I, J = data.pair_index(nc)
        grp = rng.integers(0, max(2, nc // 12), (B, nc))
        on = np.triu(rng.random((B, nc, nc)) < 0.25, 1)
        on = (on | on.transpose(0, 2, 1))[:, I, J] & (grp[:, I] == grp[:, J])
        p1 = np.where(on, 0.75, 0.0).astype(np.float32) + 0.25 * rng.random((B, R), dtype=np.float32)
        probs = torch.from_numpy(np.ascontiguousarray(np.stack([1.0 - p1, p1], 1), np.float32)).to(dev)
        shape = _lib.Shape(B, ne, nc, 2, B, 0)
        bt = _lib.Batch(None, None, ybits.data_ptr(), None, None, None)
        groups = torch.empty(B, nc, dtype=torch.int32, device=dev)
        tgroups = torch.empty(B, nc, dtype=torch.int32, device=dev)
        ut = torch.empty(B, _lib.UT_SLOTS, dtype=torch.int64, device=dev)
        ws = torch.empty(lib.hdg_untangle_workspace_bytes(ctypes.byref(shape)) // 4,
                         dtype=torch.int32, device=dev)

        def launch():
            _lib.check(lib.hdg_untangle(ctypes.byref(shape), ctypes.byref(bt),
                                        ctypes.c_void_p(probs.data_ptr()), ctypes.c_float(0.5),
                                        _lib.UT_RULE_MEAN, ctypes.c_void_p(groups.data_ptr()),
                                        ctypes.c_void_p(tgroups.data_ptr()),
                                        ctypes.c_void_p(ut.data_ptr()),
                                        ctypes.c_void_p(ws.data_ptr()), stream))

        launch()
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        host_probs = probs.cpu().numpy()
        t1 = time.perf_counter()
        want, hg, ht = metrics.untangle_counts(label, host_probs)
        t2 = time.perf_counter()
        if not (np.array_equal(ut.cpu().numpy(), want) and np.array_equal(groups.cpu().numpy(), hg)
                and np.array_equal(tgroups.cpu().numpy(), ht)):
            raise SystemExit("%s: device and host results differ" % name)
        for _ in range(a.warmup):
            launch()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.launches):
            launch()
        e1.record()
        torch.cuda.synchronize(dev)
        sc = metrics.scores_from_untangle(want)
        row = {"shape": name, "ne": ne, "nc": nc, "batch": B, "pairs": B * R // 2,
               "blocks_per_commit": _lib.untangle_blocks(nc),
               "device_ms_per_call": e0.elapsed_time(e1) / a.launches,
               "launches": a.launches, "warmup": a.warmup,
               "host_copy_ms": (t1 - t0) * 1e3, "host_untangle_counts_ms": (t2 - t1) * 1e3,
               "probs_mbytes": B * 2 * R * 4 / 1e6,
               "groups_mean": float(want[:, _lib.UT_GROUPS].mean()),
               "links_mean": float(want[:, _lib.UT_LINKS].mean()), "rand": sc["rand"], "f1": sc["f1"]}
        if not a.no_step:
            from hdgnn.engine import Engine
            from hdgnn import layout
            eng = Engine(ne, nc, B, variant=2)
            eng.set_params(layout.init_flat(5, 2))
            db =eng.upload(synth_commits(B, ne, nc, 3))
            for _ in range(a.warmup):
                eng.train_step(db)
            e0.record()
            for _ in range(a.launches):
                eng.train_step(db)
            e1.record()
            torch.cuda.synchronize(dev)
            eng.check_status()
            row["train_step_ms"] = e0.elapsed_time(e1) / a.launches
            del eng, db
        print(json.dumps(row), flush=True)
        rows.append(row)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
