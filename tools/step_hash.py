"""Hash what three training steps leave behind, per shape and split mode: run once per
library build (HDG_LIB_PATH, as tools/gpu_ab.sh loads variants) and compare the outputs
line by line; any differing line is a differing bit.
    python tools/step_hash.py [B:Ne:Nc:variant ...] > OUT.txt
Per line: shape, HDG_FUSED_SPLIT, then sha256 prefixes of grad (every slot), probs, stats and
the training state (params, Adam m, v) after the third train_step, then the kernel names one
traced fwd_bwd records (hdg_fwd_bwd_kernel_events), in launch order.  After the fused rows
the other ways a step runs and ends; with explicit shapes only those shapes' fused rows are
printed:
  general   the general path (kw_reduce_adam) for every variant; under each forced hunk form
            at the forms' smallest tested shapes; and at 800 commits, where the entity kernels'
            grids pass 2 and 3 blocks per CU and take their 4-wave forms (also on the fused
            path, around the step kernel)
  calls     the fwd_bwd + adam() decomposition (k_grad_reduce + k_adam_tf; model_4 on the fused
            path: k_grad_reduce, then the entity-edge rows' kw_grad_reduce)
  forward   what Engine.forward leaves on either path: probs, logits, the CE sum, loss_E_HR"""
import ctypes
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
SPLIT_CALLS = ["9:21:9:2", "9:16:17:4"]     # fwd_bwd, then adam()
FORMS = [("dense", _lib.FLAG_HUNK_DENSE), ("sorted", _lib.FLAG_HUNK_SORTED),
         ("group", _lib.FLAG_HUNK_SORTED | _lib.FLAG_HUNK_GROUP), ("tiled", _lib.FLAG_HUNK_TILED)]
FORM_SHAPES = ["%s:%d" % (s, v) for v in (1, 4) for s in ("2:37:19", "1:40:257")]
MANY = "800:16:9:4"
FORWARD = [("9:16:17:%d" % v, p) for p, vs in ((_lib.PATH_FUSED, (2, 4)),
                                               (_lib.PATH_GENERAL, (1, 2, 3, 4))) for v in vs]


def h(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()[:16]


def kernels(eng, db):
    """the kernel names of one traced fwd_bwd (it overwrites grad and probs: hash first)"""
    nev = 40
    ev = _lib.HipEvents(nev)
    names = (ctypes.c_char_p * (nev - 1))()
    nk = ctypes.c_int32()
    b = db.struct()
    _lib.check(eng.lib.hdg_fwd_bwd_kernel_events(
        ctypes.byref(eng.shape), ctypes.byref(b), ctypes.c_void_p(eng.params.data_ptr()),
        ctypes.c_void_p(eng.grad_local.data_ptr()), ctypes.byref(eng._outputs(True, False)),
        ctypes.c_void_p(eng.workspace.data_ptr()), eng._stream(), ev.ev, nev, names,
        ctypes.byref(nk)))
    torch.cuda.synchronize()
    return " ".join(names[i].decode() for i in range(nk.value))


def run(spec, split, path=_lib.PATH_FUSED, calls=False, flags=0, form=None, forward=False):
    B, ne, nc, v = (int(s) for s in spec.split(":"))
    os.environ["HDG_FUSED_SPLIT"] = split
    cb = synth_commits(B, ne, nc, 7)
    eng = Engine(ne, nc, B, variant=v, path=path, flags=flags)
    eng.set_params(layout.init_flat(3, v))
    db = eng.upload(cb)
    tag = "general" if path == _lib.PATH_GENERAL else "split=" + split
    if form:
        tag += "/" + form
    if forward:
        eng.forward(db)
        torch.cuda.synchronize()
        sums = "forward probs %s logits %s ce %s ehr %s" % (
            h(eng.probs), h(eng.logits), h(eng.ce_sum), h(eng.ehr))
    else:
        for _ in range(3):
            if calls:
                eng.fwd_bwd(db)
                eng.adam()
            else:
                eng.train_step(db)
        torch.cuda.synchronize()
        sums = "%sgrad %s probs %s stats %s params %s m %s v %s" % (
            "calls " if calls else "", h(eng.grad), h(eng.probs), h(eng.stats), h(eng.params),
            h(eng.m), h(eng.v))
    print("%-14s %s %s | %s" % (spec, tag, sums, kernels(eng, db)), flush=True)


if __name__ == "__main__":
    for spec in sys.argv[1:] or SHAPES:
        for split in ("1", "0"):
            run(spec, split)
    if not sys.argv[1:]:
        for spec in GENERAL:
            run(spec, "1", path=_lib.PATH_GENERAL)
        for spec in FORM_SHAPES:
            for form, flags in FORMS:
                run(spec, "1", path=_lib.PATH_GENERAL, flags=flags, form=form)
        run(MANY, "1", path=_lib.PATH_GENERAL)
        run(MANY, "1")
        for spec in SPLIT_CALLS:
            run(spec, "1", calls=True)
        for spec, path in FORWARD:
            run(spec, "1", path=path, forward=True)
