"""Counts-based evaluation, host side: hdgnn.metrics.eval_counts / scores_from_counts
against sklearn, the Python mirror of the HDG_EV_* constants, hdg_eval's argument checks
(host only: they return before any HIP call) and main.py --Type eval."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from hdgnn import metrics
from test_cli import _load_main


def _quantised_commits(B=6, nc=9, seed=11):
    """Random labels and scores on the 1/8 grid (ties are common), p0 = 1 - p1."""
    rng = np.random.default_rng(seed)
    R = nc * (nc - 1)
    y = rng.random((B, R)) < 0.3
    y[:, 0], y[:, 1] = True, False                      # both classes in every commit
    p1 = rng.integers(0, 9, (B, R)) / 8.0
    label = np.stack([~y, y], 1).astype(np.float32)
    probs = np.stack([1.0 - p1, p1], 1).astype(np.float32)
    return y, label, probs


def test_eval_counts_against_sklearn():
    from sklearn.metrics import confusion_matrix, roc_auc_score
    y, label, probs = _quantised_commits()
    ev = metrics.eval_counts(label, probs)
    assert ev.shape == (6, metrics.EV_SLOTS) and ev.dtype == np.int64
    assert (probs[:, 1] == probs[:, 0]).any()           # p1 == p0 ties: predicted 0
    for b in range(6):
        tn, fp, fn, tp = confusion_matrix(y[b], np.argmax(probs[b], axis=0), labels=[0, 1]).ravel()
        assert (ev[b, metrics.EV_TP], ev[b, metrics.EV_FP], ev[b, metrics.EV_FN],
                ev[b, metrics.EV_TN]) == (tp, fp, fn, tn)
        P, N = tp + fn, fp + tn
        auc = ev[b, metrics.EV_U2] / (2.0 * P * N)
        # float64 on at most 72 terms on both sides: rounding only
        assert abs(auc - roc_auc_score(y[b], probs[b, 1])) <= 1e-9
        assert ev[b, metrics.EV_NAN] == 0 and not ev[b, 6:].any()


def test_eval_counts_nan_relations_leave_every_other_slot():
    y, label, probs = _quantised_commits(B=2)
    clean = metrics.eval_counts(label, probs)
    probs[0, 0, 3] = np.nan                             # a positive or negative, channel 0
    probs[0, 1, 0] = np.nan                             # the forced positive, channel 1
    ev = metrics.eval_counts(label, probs)
    assert ev[0, metrics.EV_NAN] == 2 and ev[0, :4].sum() == 72 - 2
    np.testing.assert_array_equal(ev[1], clean[1])
    keep = np.ones(72, bool)
    keep[[0, 3]] = False
    np.testing.assert_array_equal(
        metrics.eval_counts(label[:1][:, :, keep], probs[:1][:, :, keep])[0, :5], ev[0, :5])


def test_scores_from_counts_hand_table():
    #            TP FP FN TN  U2 NAN
    ev = np.array([[2, 1, 2, 5, 36, 0, 0, 0],     # P = 4, N = 6: auc 36 / 48
                   [0, 0, 0, 10, 0, 0, 0, 0],     # P = 0: no auc, precision / recall / f1 undefined
                   [3, 3, 0, 2, 30, 2, 0, 0]],    # P = 3, N = 5: auc 30 / 30
                  np.int64)
    s = metrics.scores_from_counts(ev)
    assert s["acc"] == pytest.approx(22 / 28) and s["acc_mean"] == pytest.approx((0.7 + 1 + 5 / 8) / 3)
    assert s["precision"] == pytest.approx(5 / 9)
    assert s["precision_mean"] == pytest.approx((2 / 3 + 1 / 2) / 2)      # commit 1 skipped
    assert s["recall"] == pytest.approx(5 / 7) and s["recall_mean"] == pytest.approx((0.5 + 1) / 2)
    assert s["f1"] == pytest.approx(10 / 16)
    assert s["f1_mean"] == pytest.approx((4 / 7 + 6 / 9) / 2)
    assert s["auc"] == pytest.approx((0.75 + 1.0) / 2) and s["auc_commits"] == 2
    assert s["nan_relations"] == 2
    # pooled and per-commit means differ on this table
    assert s["precision"] != pytest.approx(s["precision_mean"])


def test_scores_from_counts_undefined_ratios_are_nan():
    import warnings
    ev = np.array([[0, 0, 3, 7, 0, 0, 0, 0]], np.int64)      # nothing predicted positive
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        s = metrics.scores_from_counts(ev)
        none = metrics.scores_from_counts(np.zeros((0, 8), np.int64))
    assert math.isnan(s["precision"]) and math.isnan(s["precision_mean"])
    assert s["recall"] == 0.0 and s["acc"] == 0.7 and s["auc"] == 0.0 and s["auc_commits"] == 1
    assert math.isnan(none["acc"]) and math.isnan(none["auc"]) and none["auc_commits"] == 0


def test_python_mirror_matches_header_eval_constants():
    from hdgnn import _lib
    with open(os.path.join(ROOT, "include", "hdgnn.h")) as f:
        defs = dict(re.findall(r"#define\s+(HDG_[A-Z_0-9]+)\s+(0x[0-9a-fA-F]+|\d+)", f.read()))
    val = {k: int(v, 0) for k, v in defs.items()}
    for mod in (_lib, metrics):
        assert val["HDG_EV_SLOTS"] == mod.EV_SLOTS
        for n in ("TP", "FP", "FN", "TN", "U2", "NAN"):
            assert val["HDG_EV_" + n] == getattr(mod, "EV_" + n), n
    assert val["HDG_EVAL_CHUNK"] == _lib.EVAL_CHUNK
    assert val["HDG_ABI_VERSION"] == _lib.ABI_VERSION == 9      # a compatible addition


def test_hdg_eval_argument_errors_host_only():
    """NULL pointers and a bad shape are refused before any HIP call."""
    from hdgnn import _lib
    lib = _lib.load()
    bt = _lib.Batch(None, None, 64, None, None, None)             # never dereferenced
    assert lib.hdg_eval(None, ctypes.byref(bt), 64, 64, None) == 1000
    assert b"shape" in lib.hdg_last_error()
    bad = _lib.Shape(3, 20, 1, 2, 3, 0)
    assert lib.hdg_eval(ctypes.byref(bad), ctypes.byref(bt), 64, 64, None) == 1000
    assert b"nc" in lib.hdg_last_error()
    ok = _lib.Shape(3, 20, 10, 2, 3, 0)
    assert lib.hdg_eval(ctypes.byref(ok), None, 64, 64, None) == 1000
    assert b"NULL" in lib.hdg_last_error()
    assert lib.hdg_eval(ctypes.byref(ok), ctypes.byref(bt), None, 64, None) == 1000
    assert lib.hdg_eval(ctypes.byref(ok), ctypes.byref(bt), 64, None, None) == 1000
    nolab = _lib.Batch(None, None, None, None, None, None)
    assert lib.hdg_eval(ctypes.byref(ok), ctypes.byref(nolab), 64, 64, None) == 1000
    assert lib.hdg_eval(ctypes.byref(_lib.Shape(0, 20, 10, 2, 3, 0)), ctypes.byref(bt), 64, 64,
                        None) == 1000
    assert b"batch" in lib.hdg_last_error()


class _Recorder:
    log = []

    def __init__(self, sess, **kw):
        _Recorder.log.append(("init", kw["Step"]))

    def train(self, args):
        _Recorder.log.append(("train", args.Step))

    def test(self, args):
        _Recorder.log.append(("test", args.Step))

    def evaluate(self, args):
        _Recorder.log.append(("evaluate", args.Step, args.Ne, args.Nc))


def test_main_type_eval_calls_evaluate_per_step(tmp_path):
    cli = _load_main()
    _Recorder.log = []
    cli.main(["--Type", "eval", "--checkpoint_dir", str(tmp_path / "ck") + "/"],
             model_cls=_Recorder)
    runs = [e for e in _Recorder.log if e[0] != "init"]
    assert runs == [("evaluate", s, ne, nc) for s, ne, nc in
                    zip(cli.STEPS, cli.ENTITY_NODES, cli.HUNK_NODES)]
    assert [e[1] for e in _Recorder.log if e[0] == "init"] == cli.STEPS
