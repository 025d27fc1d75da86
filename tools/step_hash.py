"""Hash what three training steps leave behind, per shape and split mode: run once per
library build (HDG_LIB_PATH, as tools/gpu_ab.sh loads variants) and compare the outputs
line by line; any differing line is a differing bit.
    python tools/step_hash.py [B:Ne:Nc:variant ...] > OUT.txt
Per line: shape, HDG_FUSED_SPLIT, then sha256 prefixes of grad (every slot), probs, stats and
the training state (params, Adam m, v) after the third train_step.  After the fused rows the
other ways a step ends: the general path (kw_reduce_adam) for every variant, and the
fwd_bwd + adam() decomposition (k_grad_reduce + k_adam_tf); with explicit shapes only those
shapes' fused rows are printed."""
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "hd-gnn_amd"))

import torch  # noqa: E402
from hdgnn import _lib, layout  # noqa: E402
from hdgnn.engine import Engine  # noqa: E402
from hdgnn.synth import synth_commits  # noqa: E402

# glide, the tile and K-quarter edges of the hunk stage, padding commits (B = 9), the wide
# forms (NC16 = 128, 160), model_4 on the step kernel
SHAPES = ["100:200:74:2", "9:21:9:2", "9:12:15:2", "9:13:16:2", "9:16:17:2", "9:19:79:2",
          "9:21:80:2", "9:14:81:2", "8:256:80:2", "6:250:150:2", "2:256:160:2", "9:16:17:4",
          "8:200:74:4"]
GENERAL = ["%s:%d" % (s, v) for v in (1, 2, 3, 4) for s in ("9:21:9", "9:16:17")]
SPLIT_CALLS = ["9:21:9:2"]     # fwd_bwd, then adam()


def h(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()[:16]


def run(spec, split, path=_lib.PATH_FUSED, calls=False):
    B, ne, nc, v = (int(s) for s in spec.split(":"))
    os.environ["HDG_FUSED_SPLIT"] = split
    cb = synth_commits(B, ne, nc, 7)
    eng = Engine(ne, nc, B, variant=v, path=path)
    eng.set_params(layout.init_flat(3, v))
    db = eng.upload(cb)
    for _ in range(3):
        if calls:
            eng.fwd_bwd(db)
            eng.adam()
        else:
            eng.train_step(db)
    torch.cuda.synchronize()
    tag = "calls" if calls else ("general" if path == _lib.PATH_GENERAL else "split=" + split)
    print("%-14s %s grad %s probs %s stats %s params %s m %s v %s" % (
        spec, tag, h(eng.grad), h(eng.probs), h(eng.stats), h(eng.params), h(eng.m), h(eng.v)),
        flush=True)


if __name__ == "__main__":
    for spec in sys.argv[1:] or SHAPES:
        for split in ("1", "0"):
            run(spec, split)
    if not sys.argv[1:]:
        for spec in GENERAL:
            run(spec, "1", path=_lib.PATH_GENERAL)
        for spec in SPLIT_CALLS:
            run(spec, "1", calls=True)
