"""GPU box: time of one hdg_eval launch against the host path it replaces, at the glide
shape (200x74, B=100) and the stress shape (1024x512, B=32).

  device   events around --launches (20) hdg_eval calls after --warmup (5), per launch
  host     the device-to-host copy of probs, then hdgnn.metrics.eval_counts on it (once)

Scores are uniform random with p0 = 1 - p1, labels hdgnn.synth's (symmetric, 10 % density);
the two tables are compared before anything is timed.  Prints one JSON line per shape and
writes them to --out (default bench_out/eval_time.json).

  python tools/eval_time.py [--launches 20] [--warmup 5] [--out PATH]
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
    ap.add_argument("--out", default=os.path.join(ROOT, "bench_out", "eval_time.json"))
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
        y = synth_commits(B, 4, nc, 3).y             # only the hunk labels are used
        label = data.onehot_relations(y)
        ybits = torch.from_numpy(data.pack_bits(y).view(np.int32)).to(dev)
        p1 = torch.rand(B, R, device=dev)
        probs = torch.stack([1.0 - p1, p1], 1).contiguous()
        ev = torch.empty(B, _lib.EV_SLOTS, dtype=torch.int64, device=dev)
        shape = _lib.Shape(B, ne, nc, 2, B, 0)
        bt = _lib.Batch(None, None, ybits.data_ptr(), None, None, None)

        def launch():
            _lib.check(lib.hdg_eval(ctypes.byref(shape), ctypes.byref(bt),
                                    ctypes.c_void_p(probs.data_ptr()),
                                    ctypes.c_void_p(ev.data_ptr()), stream))

        launch()
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        host_probs = probs.cpu().numpy()
        t1 = time.perf_counter()
        want = metrics.eval_counts(label, host_probs)
        t2 = time.perf_counter()
        if not np.array_equal(ev.cpu().numpy(), want):
            raise SystemExit("%s: device and host tables differ" % name)
        for _ in range(a.warmup):
            launch()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.launches):
            launch()
        e1.record()
        torch.cuda.synchronize(dev)
        row = {"shape": name, "ne": ne, "nc": nc, "batch": B, "relations": B * R,
               "chunks_per_commit": -(-R // _lib.EVAL_CHUNK),
               "device_ms_per_launch": e0.elapsed_time(e1) / a.launches,
               "launches": a.launches, "warmup": a.warmup,
               "host_copy_ms": (t1 - t0) * 1e3, "host_eval_counts_ms": (t2 - t1) * 1e3,
               "probs_mbytes": B * 2 * R * 4 / 1e6,
               "auc": metrics.scores_from_counts(want)["auc"]}
        print(json.dumps(row), flush=True)
        rows.append(row)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
