"""Device-side step runner over libhdgnn.so.

Owns the fp32 parameter vector, TF-Adam state, gradient buffer, workspace and
per-step outputs on one GPU.  One training step = hdg_fwd_bwd -> (all-reduce of
the flat gradient + CE-sum trailer when distributed) -> hdg_adam_tf, all enqueued
on torch's current stream (so a torch.cuda.CUDAGraph can capture it).  The
all-reduce is the in-kernel xGMI exchange (hdgnn/xgmi.py, hdg_train_step_dp) when
every rank is on this node, else torch.distributed (RCCL); HDG_DP_ALLREDUCE or the
`allreduce` argument ("auto" | "xgmi" | "rccl") overrides the choice.
"""
import ctypes
import math
import os
import warnings

import numpy as np
import torch

from . import _lib
from .layout import n_params, state_offsets


class Engine:
    def __init__(self, ne, nc, batch, variant=2, device="cuda", batch_global=None, lr=3e-4,
                 process_group=None, path=_lib.PATH_AUTO, allreduce=None, flags=0,
                 dp_shared=None):
        """variant: model_<variant>.py (1 HD-GNN/ES, 2 HD-GNN/S, 3 HD-GNN/E, 4 HD-GNN).
        path: PATH_AUTO (fused kernel when it applies, else the general path),
        PATH_FUSED or PATH_GENERAL (include/hdgnn.h).  flags: HDG_FLAG_* bits
        (FLAG_HUNK_DENSE / FLAG_HUNK_SORTED force the general path's hunk-sum form).
        dp_shared: the xGMI ranks share devices (HDG_DP_SHARED); None detects it."""
        self.lib = _lib.load()
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("Engine needs a HIP device (got %s)" % self.device)
        if self.device.index is None:          # "cuda" -> the current device, explicitly,
            self.device = torch.device("cuda", torch.cuda.current_device())  # as tensors report
        self.ne, self.nc, self.batch, self.variant = ne, nc, batch, variant
        self.batch_global = batch_global or batch
        self.lr = lr
        self.pg = process_group
        self.shape = _lib.Shape(batch, ne, nc, variant, self.batch_global, path, flags)
        self.path = self.lib.hdg_resolve_path(ctypes.byref(self.shape))
        if self.path < 0:
            raise ValueError(self.lib.hdg_last_error().decode())
        self.np = self.lib.hdg_param_count(variant)
        assert self.np == n_params(variant)
        self.glen = self.lib.hdg_grad_len(variant)
        wsb = self.lib.hdg_workspace_bytes(ctypes.byref(self.shape))
        if wsb == 0:
            raise RuntimeError(self.lib.hdg_last_error().decode())
        dev = self.device
        f32 = torch.float32
        self.workspace = torch.zeros(wsb // 4, dtype=f32, device=dev)   # block-pair inboxes start at 0
        # the training state as one flat buffer [params | adam_m | adam_v | beta_pow]: one
        # copy snapshots, restores or reads it (the checkpoint's host copy)
        # (each slice 64-byte aligned, layout.state_offsets; the pads stay zero)
        P, so = self.np, state_offsets(variant)
        self.state = torch.zeros(so["len"], dtype=f32, device=dev)
        self.params, self.m, self.v, self.beta_pow = (
            self.state[:P], self.state[so["m"]:so["m"] + P], self.state[so["v"]:so["v"] + P],
            self.state[so["beta_pow"]:so["beta_pow"] + 2])
        for t in (self.params, self.m, self.v, self.beta_pow):
            assert t.data_ptr() % 64 == 0, "training-state slice not 64-byte aligned"
        self.beta_pow.copy_(torch.tensor([0.9, 0.999]))
        self.grad = torch.zeros(self.glen, dtype=f32, device=dev)
        # ce, loss_map, loss_para, train_loss, count parts (3), fault count (hdg_outputs.stats)
        self.stats = torch.zeros(_lib.STATS_LEN, dtype=f32, device=dev)
        # sticky status word (HDG_STATUS_* bits); check_status() reads it
        self.status = torch.zeros(1, dtype=torch.int32, device=dev)
        self.ce_sum = torch.zeros(1, dtype=f32, device=dev)
        self.ehr = torch.zeros(1, dtype=f32, device=dev)     # loss_E_HR of the last forward
        pc = nc * (nc - 1)
        self.probs = torch.zeros(batch, 2, pc, dtype=f32, device=dev)
        self.logits = torch.zeros(batch, 2, pc, dtype=f32, device=dev)
        self._state = _lib.State(self.params.data_ptr(), self.m.data_ptr(), self.v.data_ptr(),
                                 self.beta_pow.data_ptr())
        st = self.status.data_ptr()
        self._out = _lib.Outputs(self.probs.data_ptr(), self.logits.data_ptr(),
                                 self.stats.data_ptr(), st, self.ehr.data_ptr())
        # a training sess.run fetches C_edge_output2 (the probabilities), not the logits
        self._out_train = _lib.Outputs(self.probs.data_ptr(), None, self.stats.data_ptr(), st,
                                       None)
        self._out_none = _lib.Outputs(None, None, None, st, None)   # status only
        # data parallelism: which all-reduce joins the ranks' gradients
        self.xgmi, self.allreduce_kind, self.allreduce_selftest = None, None, None
        if self._distributed():
            mode = allreduce or os.environ.get("HDG_DP_ALLREDUCE", "auto")
            if mode not in ("auto", "xgmi", "rccl"):
                raise ValueError("allreduce must be auto, xgmi or rccl (got %r)" % mode)
            if mode != "rccl":
                from .xgmi import XgmiGroup
                self.xgmi = XgmiGroup.create(self.lib, self.pg or torch.distributed.group.WORLD,
                                             dev, required=mode == "xgmi", shared=dp_shared)
                self.allreduce_selftest = XgmiGroup.verdict
            else:
                self.allreduce_selftest = "xGMI not tried (HDG_DP_ALLREDUCE=rccl)"
            self.allreduce_kind = "xgmi" if self.xgmi else "rccl"
        # hdg_fwd_bwd's own (local) gradient: the xGMI tail reads it while writing the
        # world sum into self.grad, so the two must not overlap
        self.grad_local = (torch.zeros(self.glen, dtype=f32, device=dev) if self.xgmi
                           else self.grad)

    # ---- parameters ---------------------------------------------------------
    def set_params(self, flat):
        flat = np.asarray(flat, np.float32).reshape(-1)
        assert flat.size == self.np
        self.params.copy_(torch.from_numpy(flat))
        self.m.zero_()
        self.v.zero_()
        self.beta_pow.copy_(torch.tensor([0.9, 0.999]))

    def get_params(self):
        return self.params.detach().cpu().numpy().copy()

    # ---- steps --------------------------------------------------------------
    def _stream(self):
        return ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def upload(self, cb):
        """Host CommitBatch -> DeviceBatch prepared for this engine's path."""
        return cb.to_device(self.device, self.variant, self.path)

    def _check(self, dbatch):
        assert dbatch.B == self.batch and dbatch.Ne == self.ne and dbatch.Nc == self.nc
        if dbatch.path != self.path or getattr(dbatch, "variant", self.variant) != self.variant:
            raise ValueError("batch prepared for model_%s path %d, engine runs model_%d path %d "
                             "(use Engine.upload)" % (getattr(dbatch, "variant", "?"), dbatch.path,
                                                      self.variant, self.path))

    def _outputs(self, outputs, logits, stats=None):
        if not outputs:
            return self._out_none
        out = self._out if logits else self._out_train
        if stats is None:
            return out
        # a caller-provided stats row (a training loop's per-step row of an epoch buffer)
        assert stats.device == self.device and stats.dtype == torch.float32 and \
            stats.is_contiguous() and stats.numel() >= _lib.STATS_LEN
        return _lib.Outputs(out.probs, out.logits, stats.data_ptr(), out.status, out.ehr)

    # ---- split mode (fused path: two co-resident blocks per commit) -------------------
    @property
    def split(self):
        """False once set_split(False) forced one block per commit (HDG_FLAG_NO_SPLIT)."""
        return not (self.shape.flags & _lib.FLAG_NO_SPLIT)

    def set_split(self, on):
        self.shape.flags = (self.shape.flags & ~_lib.FLAG_NO_SPLIT) | (0 if on else
                                                                       _lib.FLAG_NO_SPLIT)

    def snapshot(self):
        """A device copy of the training state (parameters, Adam moments, beta powers)."""
        return self.state.clone()

    def restore(self, snap):
        """Set the training state from a snapshot() (device) or a host copy of self.state."""
        if isinstance(snap, np.ndarray):
            snap = torch.from_numpy(np.ascontiguousarray(snap, np.float32))
        self.state.copy_(snap)

    def split_fault_retry(self):
        """After a step whose block-pair exchange timed out (HDG_STATUS_XCH_TIMEOUT; its
        update was skipped on every rank, the fault count travels in the all-reduced
        gradient trailer): switch to one block per commit for the rest of the run and
        clear the status, so the caller re-runs the step.  Returns False when already in
        one-block mode (the fault is then not a residency problem)."""
        if not self.split:
            return False
        warnings.warn("libhdgnn: a split-mode block-pair exchange timed out (the two blocks "
                      "of a commit were not co-resident); re-running in one-block-per-commit "
                      "mode for the rest of this run", RuntimeWarning, stacklevel=2)
        self.set_split(False)
        self.clear_status()
        return True

    def train_step_checked(self, dbatch, outputs=True, logits=False, stats=None):
        """train_step that survives a split-mode pair timeout: on a faulted step (read from
        the gradient trailer, identical on every rank) the state is restored and the step
        re-run with one block per commit.

        A per-step diagnostic / test helper, not a loop body: it snapshots the whole state
        and synchronises with the device on every call.  Training loops use the epoch-buffer
        pattern of graph2graph.train (every step's stats into its own device row, one read
        per epoch, the retry decided from those rows)."""
        snap = self.snapshot() if self.split else None
        self.train_step(dbatch, outputs, logits, stats)
        fault = float(self.grad[self.np + _lib.TR_FAULT].item())
        if fault != 0.0 and snap is not None and self.split_fault_retry():
            self.restore(snap)
            self.train_step(dbatch, outputs, logits, stats)
            fault = float(self.grad[self.np + _lib.TR_FAULT].item())
        if fault != 0.0 or int(self.status.item()):
            self.check_status()

    # ---- status / trailer -----------------------------------------------------
    def check_status(self):
        """Raise if any launch since the last clear_status() failed on the device (the
        sticky status word, include/hdgnn.h).  Synchronises with the device."""
        st = int(self.status.item())
        if st & _lib.STATUS_DP_TIMEOUT:
            raise RuntimeError(
                "libhdgnn: a peer rank's gradient words did not arrive over xGMI in time (a "
                "rank stopped or issued a different sequence of steps); that step's loss is "
                "NaN and its update was skipped on the waiting blocks.")
        if st & _lib.STATUS_XCH_TIMEOUT:
            raise RuntimeError(
                "libhdgnn: a block-pair exchange of the fused split path timed out (the two "
                "blocks of a commit were not resident together: another process holding "
                "CUs?); that step's outputs are NaN and its Adam update was skipped. "
                "HDG_FUSED_SPLIT=0 runs one block per commit.")
        if st:
            raise RuntimeError("libhdgnn: device status 0x%x" % st)

    def clear_status(self):
        self.status.zero_()

    def correct_count(self, trailer=None):
        """top_ACC numerator of the last fwd_bwd / train step (summed over ranks when the
        gradient was all-reduced) from the gradient trailer."""
        tr = (self.grad[self.np:] if trailer is None else trailer)
        return _lib.trailer_count(tr.cpu().numpy() if hasattr(tr, "cpu") else tr)

    def fwd_bwd(self, dbatch, outputs=True, logits=True):
        self._reduced = False
        self._check(dbatch)
        b = dbatch.struct()
        out = self._outputs(outputs, logits)
        _lib.check(self.lib.hdg_fwd_bwd(ctypes.byref(self.shape), ctypes.byref(b),
                                        ctypes.c_void_p(self.params.data_ptr()),
                                        ctypes.c_void_p(self.grad_local.data_ptr()),
                                        ctypes.byref(out),
                                        ctypes.c_void_p(self.workspace.data_ptr()),
                                        self._stream()))

    def allreduce(self):
        """All-reduce the flat gradient: RCCL in place on self.grad; xGMI from the local
        gradient fwd_bwd wrote (grad_local) into self.grad (hdg_dp_allreduce).  Either way
        self.grad then holds the world sum, and adam() applies TF Adam to it."""
        if not self._distributed():
            return
        if self.xgmi:
            _lib.check(self.lib.hdg_dp_allreduce(ctypes.byref(self.xgmi.dp),
                                                 ctypes.c_void_p(self.grad_local.data_ptr()),
                                                 ctypes.c_void_p(self.grad.data_ptr()),
                                                 ctypes.c_int32(self.glen),
                                                 ctypes.c_void_p(self.status.data_ptr()),
                                                 self._stream()))
            self._reduced = True
            return
        torch.distributed.all_reduce(self.grad, group=self.pg)

    def adam(self):
        """TF Adam on the world gradient.  xGMI: when allreduce() already summed it into
        self.grad, a local update of that sum (every rank holds the same bits); otherwise
        the exchange and the update in one kernel (hdg_adam_dp, from grad_local)."""
        if self.xgmi and not getattr(self, "_reduced", False):
            _lib.check(self.lib.hdg_adam_dp(ctypes.byref(self.shape), ctypes.byref(self._state),
                                            ctypes.c_void_p(self.grad_local.data_ptr()),
                                            ctypes.c_void_p(self.grad.data_ptr()),
                                            ctypes.c_float(self.lr),
                                            ctypes.c_void_p(self.stats.data_ptr()),
                                            ctypes.c_void_p(self.status.data_ptr()),
                                            ctypes.byref(self.xgmi.dp), self._stream()))
            return
        self._reduced = False
        _lib.check(self.lib.hdg_adam_tf(ctypes.byref(self.shape), ctypes.byref(self._state),
                                        ctypes.c_void_p(self.grad.data_ptr()),
                                        ctypes.c_float(self.lr),
                                        ctypes.c_void_p(self.stats.data_ptr()), self._stream()))

    def _distributed(self):
        return self.pg is not None or (torch.distributed.is_available()
                                       and torch.distributed.is_initialized()
                                       and torch.distributed.get_world_size() > 1)

    def train_step(self, dbatch, outputs=True, logits=False, stats=None):
        """sess.run([C_edge_output2, loss_Hedge_mse, loss_map, theta, trainer]) equivalent:
        outputs land in self.probs / self.stats (pre-update), params updated in place;
        self.logits only with logits=True (the reference's training run does not fetch them);
        stats: a device row of >= 8 floats for this step's hdg_outputs.stats instead of
        self.stats (so a loop can keep every step's values and read them once).
        Single process: hdg_train_step (step kernel + fused reduce/Adam).  Data parallel
        over xGMI: hdg_train_step_dp (the same two kernels, the exchange inside the second).
        Over RCCL: hdg_fwd_bwd -> all-reduce of the flat gradient -> hdg_adam_tf."""
        if self.xgmi:
            self._check(dbatch)
            b = dbatch.struct()
            out = self._outputs(outputs, logits, stats)
            _lib.check(self.lib.hdg_train_step_dp(ctypes.byref(self.shape), ctypes.byref(b),
                                                  ctypes.byref(self._state),
                                                  ctypes.c_float(self.lr), ctypes.byref(out),
                                                  ctypes.c_void_p(self.grad.data_ptr()),
                                                  ctypes.c_void_p(self.workspace.data_ptr()),
                                                  ctypes.byref(self.xgmi.dp), self._stream()))
            return
        if self._distributed():
            self.fwd_bwd(dbatch, outputs, logits)
            self.allreduce()
            self.adam()
            if stats is not None:
                stats[:_lib.STATS_LEN].copy_(self.stats)
            return
        self._check(dbatch)
        b = dbatch.struct()
        out = self._outputs(outputs, logits, stats)
        _lib.check(self.lib.hdg_train_step(ctypes.byref(self.shape), ctypes.byref(b),
                                           ctypes.byref(self._state), ctypes.c_float(self.lr),
                                           ctypes.byref(out),
                                           ctypes.c_void_p(self.grad.data_ptr()),
                                           ctypes.c_void_p(self.workspace.data_ptr()),
                                           self._stream()))

    def step_call(self, dbatch, stats=None, logits=False):
        """A zero-argument callable that enqueues train_step(dbatch, logits=logits,
        stats=stats) on the current stream, its ctypes arguments built once (a training
        loop's per-step host cost).  Single process only; data parallel: train_step itself."""
        if self.xgmi or self._distributed():
            return lambda: self.train_step(dbatch, True, logits, stats)
        self._check(dbatch)
        b = dbatch.struct()
        out = self._outputs(True, logits, stats)
        fn, check = self.lib.hdg_train_step, _lib.check
        args = (ctypes.byref(self.shape), ctypes.byref(b), ctypes.byref(self._state),
                ctypes.c_float(self.lr), ctypes.byref(out),
                ctypes.c_void_p(self.grad.data_ptr()),
                ctypes.c_void_p(self.workspace.data_ptr()), self._stream())

        def call():
            check(fn(*args))
        return call

    # ---- HIP graph of one training step ----------------------------------------
    def capture(self, dbatch, outputs=True, logits=False, steps=1):
        """Capture `steps` consecutive train_step(dbatch) calls (fwd_bwd [+ RCCL all-reduce]
        + Adam each) into one HIP graph; replay() then runs that many training steps with a
        single launch (no per-step graph launch gap).  dbatch must stay alive."""
        saved = self.snapshot()
        self.train_step(dbatch, outputs, logits)  # warm: attributes set, RCCL comm built
        self.restore(saved)                       # the warm-up step leaves no trace
        torch.cuda.synchronize(self.device)
        self._graph_batch = dbatch
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            for _ in range(steps):
                self.train_step(dbatch, outputs, logits)
        torch.cuda.synchronize(self.device)
        self._graph = g
        self.graph_steps = steps
        return g

    def replay(self):
        self._graph.replay()

    def forward(self, dbatch):
        """sess.run([loss_Hedge_mse, loss_map, C_edge_output2]) equivalent (test path);
        also fills self.ehr with the batch's loss_E_HR (model_2.py:122)."""
        self._check(dbatch)
        b = dbatch.struct()
        _lib.check(self.lib.hdg_forward(ctypes.byref(self.shape), ctypes.byref(b),
                                        ctypes.c_void_p(self.params.data_ptr()),
                                        ctypes.byref(self._out),
                                        ctypes.c_void_p(self.ce_sum.data_ptr()),
                                        ctypes.c_void_p(self.workspace.data_ptr()),
                                        self._stream()))
        return self.probs, self.logits, self.ce_sum

    # ---- what the decoders of the pair scores share --------------------------------
    def _decode_probs(self, probs):
        """`probs`, default self.probs, checked: contiguous fp32 [B][2][nc(nc-1)] on this device."""
        probs = self.probs if probs is None else probs
        if (probs.device != self.device or probs.dtype != torch.float32
                or not probs.is_contiguous()
                or tuple(probs.shape) != (self.batch, 2, self.nc * (self.nc - 1))):
            raise ValueError("probs must be a contiguous float32 [%d][2][%d] tensor on %s"
                             % (self.batch, self.nc * (self.nc - 1), self.device))
        return probs

    @staticmethod
    def _rule(rule):
        """The library's number of the link rule `rule`."""
        if rule not in _lib.UT_RULES:
            raise ValueError("rule must be one of %s (got %r)" % (", ".join(_lib.UT_RULES), rule))
        return _lib.UT_RULES[rule]

    def _workspace(self, attr, nbytes_fn, dtype):
        """The workspace kept in self.<attr>: nbytes_fn() bytes of `dtype`, allocated on the
        first call."""
        ws = getattr(self, attr, None)
        if ws is None:
            nbytes = nbytes_fn()
            if nbytes == 0:
                raise RuntimeError(self.lib.hdg_last_error().decode())
            ws = torch.empty(nbytes // dtype.itemsize, dtype=dtype, device=self.device)
            setattr(self, attr, ws)
        return ws

    def _tree_outputs(self):
        """Fresh (merges, levels, curve, tgroups, lk) of a merge tree.  curve and lk hold u32 /
        u64 counts, every value < 2^31 (at most nc (nc-1) / 2 pairs): int32 and int64 read
        them as they are."""
        n1 = self.nc - 1
        return (torch.empty(self.batch, n1, 2, dtype=torch.int32, device=self.device),
                torch.empty(self.batch, n1, dtype=torch.float32, device=self.device),
                torch.empty(self.batch, n1, 2, dtype=torch.int32, device=self.device),
                torch.empty(self.batch, self.nc, dtype=torch.int32, device=self.device),
                torch.empty(self.batch, _lib.LK_SLOTS, dtype=torch.int64, device=self.device))

    def evaluate(self, dbatch, probs=None):
        """hdg_eval: the per-commit evaluation table of `probs` ([B][2][nc(nc-1)] fp32 on
        this device; default self.probs as the last forward / fwd_bwd / train step left it)
        against the batch's labels -> a fresh int64 device tensor [B][EV_SLOTS] (TP, FP,
        FN, TN, U2, NAN; hdgnn.metrics.scores_from_counts turns it into scores).  Enqueued on
        the current stream; nothing is copied to the host."""
        self._check(dbatch)
        probs = self._decode_probs(probs)
        # the library writes u64 counts; every value is < 2^63, so int64 reads them as they are
        ev = torch.empty(self.batch, _lib.EV_SLOTS, dtype=torch.int64, device=self.device)
        b = dbatch.struct()
        _lib.check(self.lib.hdg_eval(ctypes.byref(self.shape), ctypes.byref(b),
                                     ctypes.c_void_p(probs.data_ptr()),
                                     ctypes.c_void_p(ev.data_ptr()), self._stream()))
        return ev

    def untangle(self, dbatch, probs=None, threshold=0.5, rule="mean"):
        """hdg_untangle: the hunk groups `probs` ([B][2][nc(nc-1)] fp32 on this device; default
        self.probs as the last forward / fwd_bwd / train step left it) gives under the link
        rule ("mean" | "any" | "both" against `threshold`, strict comparisons; include/hdgnn.h)
        and their pair counts against the batch's true groups -> (groups int32 [B][nc], ut
        int64 [B][UT_SLOTS]) as fresh device tensors (hdgnn.metrics.scores_from_untangle turns
        ut into scores).  Enqueued on the current stream; nothing is copied to the host.  The
        workspace is allocated on the first call and kept."""
        self._check(dbatch)
        probs = self._decode_probs(probs)
        rule = self._rule(rule)
        ws = self._workspace("_ut_workspace", lambda: self.lib.hdg_untangle_workspace_bytes(
            ctypes.byref(self.shape)), torch.int32)
        groups = torch.empty(self.batch, self.nc, dtype=torch.int32, device=self.device)
        # u64 counts, every value < 2^63: int64 reads them as they are
        ut = torch.empty(self.batch, _lib.UT_SLOTS, dtype=torch.int64, device=self.device)
        b = dbatch.struct()
        _lib.check(self.lib.hdg_untangle(ctypes.byref(self.shape), ctypes.byref(b),
                                         ctypes.c_void_p(probs.data_ptr()),
                                         ctypes.c_float(threshold), rule,
                                         ctypes.c_void_p(groups.data_ptr()), None,
                                         ctypes.c_void_p(ut.data_ptr()),
                                         ctypes.c_void_p(ws.data_ptr()),
                                         self._stream()))
        return groups, ut

    def linkage(self, dbatch, probs=None, rule="mean"):
        """hdg_linkage: the single-linkage merge tree of every commit's pair weights under
        `rule` ("mean" | "any" | "both"; include/hdgnn.h) -- every partition untangle() can
        give, at every threshold at once -- and the pair counts of each cut against the
        batch's true groups.  `probs` as untangle()'s.  -> (merges int32 [B][nc-1][2], levels
        float32 [B][nc-1], curve int32 [B][nc-1][2], tgroups int32 [B][nc], lk int64
        [B][LK_SLOTS]) as fresh device tensors (hdgnn.metrics.best_threshold turns levels,
        curve and lk into the best threshold).  Enqueued on the current stream; nothing is
        copied to the host.  The workspace is allocated on the first call and kept."""
        self._check(dbatch)
        probs = self._decode_probs(probs)
        rule = self._rule(rule)
        ws = self._workspace("_lk_workspace", lambda: self.lib.hdg_linkage_workspace_bytes(
            ctypes.byref(self.shape)), torch.int64)
        merges, levels, curve, tgroups, lk = self._tree_outputs()
        b = dbatch.struct()
        _lib.check(self.lib.hdg_linkage(ctypes.byref(self.shape), ctypes.byref(b),
                                        ctypes.c_void_p(probs.data_ptr()), rule,
                                        ctypes.c_void_p(merges.data_ptr()),
                                        ctypes.c_void_p(levels.data_ptr()),
                                        ctypes.c_void_p(curve.data_ptr()),
                                        ctypes.c_void_p(tgroups.data_ptr()),
                                        ctypes.c_void_p(lk.data_ptr()),
                                        ctypes.c_void_p(ws.data_ptr()),
                                        self._stream()))
        return merges, levels, curve, tgroups, lk

    def agglomerate(self, dbatch, probs=None, rule="mean", method="average"):
        """hdg_agglomerate: the merge tree of every commit under `method` ("single" |
        "complete" | "average" linkage of the pair weights `rule` gives; include/hdgnn.h), in
        linkage()'s format -> the same five fresh device tensors, so
        hdgnn.metrics.best_threshold and cut() apply to them as they are.  `probs` as
        untangle()'s.  Enqueued on the current stream; nothing is copied to the host.  The
        workspace is allocated on the first call and kept."""
        self._check(dbatch)
        probs = self._decode_probs(probs)
        rule = self._rule(rule)
        if method not in _lib.AG_METHODS:
            raise ValueError("method must be one of %s (got %r)"
                             % (", ".join(_lib.AG_METHODS), method))
        ws = self._workspace("_ag_workspace", lambda: self.lib.hdg_agglomerate_workspace_bytes(
            ctypes.byref(self.shape), 0), torch.float32)
        merges, levels, curve, tgroups, lk = self._tree_outputs()
        b = dbatch.struct()
        _lib.check(self.lib.hdg_agglomerate(ctypes.byref(self.shape), ctypes.byref(b),
                                            ctypes.c_void_p(probs.data_ptr()),
                                            rule, _lib.AG_METHODS[method], 0,
                                            ctypes.c_void_p(merges.data_ptr()),
                                            ctypes.c_void_p(levels.data_ptr()),
                                            ctypes.c_void_p(curve.data_ptr()),
                                            ctypes.c_void_p(tgroups.data_ptr()),
                                            ctypes.c_void_p(lk.data_ptr()),
                                            ctypes.c_void_p(ws.data_ptr()),
                                            self._stream()))
        return merges, levels, curve, tgroups, lk

    def cut(self, merges, levels, curve, lk, threshold=0.5, rule="mean"):
        """hdg_cut: the groups the merge tree (merges, levels, curve, lk as linkage() or
        agglomerate() returned them) gives at `threshold` under `rule`, the threshold meaning
        what it means to untangle() -> (groups int32 [B][nc], ut int64 [B][CUT_SLOTS]) as
        fresh device tensors; ut has untangle()'s slots except CUT_MERGES, the merges done
        (hdgnn.metrics.scores_from_untangle reads it as it is).  Enqueued on the current
        stream; nothing is copied to the host."""
        n1 = self.nc - 1
        want = ((merges, torch.int32, (self.batch, n1, 2)), (levels, torch.float32, (self.batch, n1)),
                (curve, torch.int32, (self.batch, n1, 2)), (lk, torch.int64, (self.batch, _lib.LK_SLOTS)))
        for x, dt, shp in want:
            if (x.device != self.device or x.dtype != dt or not x.is_contiguous()
                    or tuple(x.shape) != shp):
                raise ValueError("merges, levels, curve and lk must be the contiguous tensors "
                                 "linkage() / agglomerate() return for this engine")
        rule = self._rule(rule)
        groups = torch.empty(self.batch, self.nc, dtype=torch.int32, device=self.device)
        ut = torch.empty(self.batch, _lib.CUT_SLOTS, dtype=torch.int64, device=self.device)
        _lib.check(self.lib.hdg_cut(ctypes.byref(self.shape), ctypes.c_void_p(merges.data_ptr()),
                                    ctypes.c_void_p(levels.data_ptr()),
                                    ctypes.c_void_p(curve.data_ptr()),
                                    ctypes.c_void_p(lk.data_ptr()), ctypes.c_float(threshold),
                                    rule, ctypes.c_void_p(groups.data_ptr()),
                                    ctypes.c_void_p(ut.data_ptr()), self._stream()))
        return groups, ut

    def refine(self, dbatch, groups=None, probs=None, threshold=0.5, rule="mean", max_sweeps=8):
        """hdg_refine: best-move sweeps on the correlation-clustering objective of `probs`
        under `rule` at `threshold` (the threshold meaning what it means to untangle();
        include/hdgnn.h), starting from `groups` (int32 [B][nc] on this device, as untangle()
        or cut() returned them; None: every hunk alone), at most `max_sweeps` sweeps ->
        (groups int32 [B][nc], ut int64 [B][RF_SLOTS], rq int64 [B][RF_Q_SLOTS]) as fresh
        device tensors; ut has untangle()'s slots except RF_MOVES, the moves made
        (hdgnn.metrics.scores_from_untangle reads it as it is), rq holds the objective at the
        start and the end, the sweeps run and whether the last one made no move.  `probs` as
        untangle()'s.  Enqueued on the current stream; nothing is copied to the host.  The
        workspace is allocated on the first call and kept."""
        return self._refine(dbatch, groups, probs, threshold, rule, max_sweeps, None)

    def refine_merge(self, dbatch, groups=None, probs=None, threshold=0.5, rule="mean",
                     max_sweeps=8, max_rounds=4):
        """hdg_refine_merge: refine() in at most `max_rounds` rounds (1 to RM_MAX_ROUNDS), a
        round being refine()'s node sweeps followed by one group sweep in which whole groups
        merge (include/hdgnn.h); `max_sweeps` is the total of node sweeps -> (groups int32
        [B][nc], ut int64 [B][RF_SLOTS], rq int64 [B][RM_Q_SLOTS]) as fresh device tensors: as
        refine()'s, RF_MOVES counting node moves only and rq holding four more slots (the
        rounds run, the merges made, the objective after the first node phase, 0).  Arguments,
        stream and workspace as refine()'s."""
        if not (isinstance(max_rounds, int) and 1 <= max_rounds <= _lib.RM_MAX_ROUNDS):
            raise ValueError("max_rounds must be an int in [1, %d] (got %r)"
                             % (_lib.RM_MAX_ROUNDS, max_rounds))
        return self._refine(dbatch, groups, probs, threshold, rule, max_sweeps, max_rounds)

    def refine_split(self, dbatch, groups=None, probs=None, threshold=0.5, rule="mean",
                     max_sweeps=8, max_rounds=4, kinds="both"):
        """hdg_refine_split: refine_merge()'s rounds with the sweeps `kinds` names after every
        node phase -- "merge": the group sweep alone (refine_merge() itself), "split": one split
        sweep, in which a group is cut in two from two seeds if the sum between the two sides is
        below 0 (include/hdgnn.h), "both": the group sweep, then the split sweep -> (groups
        int32 [B][nc], ut int64 [B][RF_SLOTS], rq int64 [B][RS_Q_SLOTS]) as fresh device
        tensors: refine_merge()'s, with the accepted splits in rq's last slot.  Arguments,
        stream and workspace as refine()'s."""
        return self._refine(dbatch, groups, probs, threshold, rule, max_sweeps,
                            self._rounds(max_rounds), self._kinds(kinds))

    @staticmethod
    def _rounds(max_rounds):
        if not (isinstance(max_rounds, int) and 1 <= max_rounds <= _lib.RM_MAX_ROUNDS):
            raise ValueError("max_rounds must be an int in [1, %d] (got %r)"
                             % (_lib.RM_MAX_ROUNDS, max_rounds))
        return max_rounds

    @staticmethod
    def _kinds(kinds):
        if not (isinstance(kinds, str) and kinds in _lib.RS_KINDS):
            raise ValueError("kinds must be one of %s (got %r)"
                             % (", ".join(_lib.RS_KINDS), kinds))
        return _lib.RS_KINDS[kinds]

    def _refine(self, dbatch, groups, probs, threshold, rule, max_sweeps, max_rounds, kinds=None):
        """refine() (max_rounds None), refine_merge() (kinds None) and refine_split(): the
        checks, the outputs, the call."""
        self._check(dbatch)
        probs = self._decode_probs(probs)
        rule = self._rule(rule)
        if not (isinstance(max_sweeps, int) and 1 <= max_sweeps <= _lib.RF_MAX_SWEEPS):
            raise ValueError("max_sweeps must be an int in [1, %d] (got %r)"
                             % (_lib.RF_MAX_SWEEPS, max_sweeps))
        if groups is not None and (groups.device != self.device or groups.dtype != torch.int32
                                   or not groups.is_contiguous()
                                   or tuple(groups.shape) != (self.batch, self.nc)):
            raise ValueError("groups must be a contiguous int32 [%d][%d] tensor on %s"
                             % (self.batch, self.nc, self.device))
        ws = self._workspace("_rf_workspace", lambda: self.lib.hdg_refine_workspace_bytes(
            ctypes.byref(self.shape), 0), torch.int64)
        out = torch.empty(self.batch, self.nc, dtype=torch.int32, device=self.device)
        # u64 counts, every value < 2^63: int64 reads them as they are
        ut = torch.empty(self.batch, _lib.RF_SLOTS, dtype=torch.int64, device=self.device)
        rq = torch.empty(self.batch, _lib.RF_Q_SLOTS if max_rounds is None else _lib.RM_Q_SLOTS,
                         dtype=torch.int64, device=self.device)
        b = dbatch.struct()
        call, budget = ((self.lib.hdg_refine, (max_sweeps,)) if max_rounds is None
                        else (self.lib.hdg_refine_merge, (max_sweeps, max_rounds)) if kinds is None
                        else (self.lib.hdg_refine_split, (max_sweeps, max_rounds, kinds)))
        _lib.check(call(ctypes.byref(self.shape), ctypes.byref(b),
                        ctypes.c_void_p(probs.data_ptr()), ctypes.c_float(threshold), rule,
                        *budget, 0,
                        None if groups is None else ctypes.c_void_p(groups.data_ptr()),
                        ctypes.c_void_p(out.data_ptr()), ctypes.c_void_p(ut.data_ptr()),
                        ctypes.c_void_p(rq.data_ptr()), ctypes.c_void_p(ws.data_ptr()),
                        self._stream()))
        return out, ut, rq

    def refine_ladder(self, dbatch, thresholds, tree=None, probs=None, rule="mean", max_sweeps=8,
                      groups=False):
        """hdg_refine_ladder: refine() at every one of the T `thresholds` (a host sequence of 1
        to RL_MAX_RUNGS finite floats, in any order) in one call, rung k starting from the cut
        at thresholds[k] of `tree` = (merges, levels) as linkage() or agglomerate() returned
        them (None: every hunk alone) -> (ut int64 [T][B][RF_SLOTS], rq int64
        [T][B][RF_Q_SLOTS], groups int32 [T][B][nc] or None unless `groups`) as fresh device
        tensors: rung k holds what cut() then refine() at thresholds[k] return
        (hdgnn.metrics.best_rung picks the rung).  `probs` as untangle()'s.  Enqueued on the
        current stream; nothing is copied to the host; a captured graph replays the captured
        thresholds.  The workspace is allocated on the first call and kept."""
        return self._refine_ladder(dbatch, thresholds, tree, probs, rule, max_sweeps, None, groups)

    def refine_merge_ladder(self, dbatch, thresholds, tree=None, probs=None, rule="mean",
                            max_sweeps=8, max_rounds=4, groups=False):
        """hdg_refine_merge_ladder: refine_ladder() with refine_merge()'s rounds at every rung
        -> (ut int64 [T][B][RF_SLOTS], rq int64 [T][B][RM_Q_SLOTS], groups int32 [T][B][nc] or
        None unless `groups`): rung k holds what cut() then refine_merge() at thresholds[k]
        return.  Arguments, stream and workspace as refine_ladder()'s."""
        if not (isinstance(max_rounds, int) and 1 <= max_rounds <= _lib.RM_MAX_ROUNDS):
            raise ValueError("max_rounds must be an int in [1, %d] (got %r)"
                             % (_lib.RM_MAX_ROUNDS, max_rounds))
        return self._refine_ladder(dbatch, thresholds, tree, probs, rule, max_sweeps, max_rounds,
                                   groups)

    def refine_split_ladder(self, dbatch, thresholds, tree=None, probs=None, rule="mean",
                            max_sweeps=8, max_rounds=4, kinds="both", groups=False):
        """hdg_refine_split_ladder: refine_merge_ladder() with refine_split()'s rounds at every
        rung -> (ut int64 [T][B][RF_SLOTS], rq int64 [T][B][RS_Q_SLOTS], groups int32
        [T][B][nc] or None unless `groups`): rung k holds what cut() then refine_split() at
        thresholds[k] return.  Arguments, stream and workspace as refine_ladder()'s."""
        return self._refine_ladder(dbatch, thresholds, tree, probs, rule, max_sweeps,
                                   self._rounds(max_rounds), groups, self._kinds(kinds))

    def _refine_ladder(self, dbatch, thresholds, tree, probs, rule, max_sweeps, max_rounds, groups,
                       kinds=None):
        """refine_ladder() (max_rounds None), refine_merge_ladder() (kinds None) and
        refine_split_ladder(): the checks, the outputs, the call."""
        self._check(dbatch)
        probs = self._decode_probs(probs)
        rule = self._rule(rule)
        if not (isinstance(max_sweeps, int) and 1 <= max_sweeps <= _lib.RF_MAX_SWEEPS):
            raise ValueError("max_sweeps must be an int in [1, %d] (got %r)"
                             % (_lib.RF_MAX_SWEEPS, max_sweeps))
        try:
            thr = [float(t) for t in thresholds]
        except TypeError:
            raise ValueError("thresholds must be a sequence of floats (got %r)" % (thresholds,))
        if not 1 <= len(thr) <= _lib.RL_MAX_RUNGS or not all(math.isfinite(t) for t in thr):
            raise ValueError("thresholds must be 1 to %d finite floats (got %r)"
                             % (_lib.RL_MAX_RUNGS, thr))
        merges = levels = None
        if tree is not None:
            n1 = self.nc - 1
            try:
                merges, levels = tree
            except (TypeError, ValueError):
                raise ValueError("tree must be (merges, levels)")
            for x, dt, shp in ((merges, torch.int32, (self.batch, n1, 2)),
                               (levels, torch.float32, (self.batch, n1))):
                if (not isinstance(x, torch.Tensor) or x.device != self.device or x.dtype != dt
                        or not x.is_contiguous() or tuple(x.shape) != shp):
                    raise ValueError("tree must be the contiguous (merges, levels) linkage() / "
                                     "agglomerate() return for this engine")
        ws = self._workspace("_rl_workspace", lambda: self.lib.hdg_refine_ladder_workspace_bytes(
            ctypes.byref(self.shape), 0), torch.int64)
        T = len(thr)
        out = (torch.empty(T, self.batch, self.nc, dtype=torch.int32, device=self.device)
               if groups else None)
        # u64 counts, every value < 2^63: int64 reads them as they are
        ut = torch.empty(T, self.batch, _lib.RF_SLOTS, dtype=torch.int64, device=self.device)
        rq = torch.empty(T, self.batch, _lib.RF_Q_SLOTS if max_rounds is None else _lib.RM_Q_SLOTS,
                         dtype=torch.int64, device=self.device)
        b = dbatch.struct()
        call, budget = ((self.lib.hdg_refine_ladder, (max_sweeps,)) if max_rounds is None
                        else (self.lib.hdg_refine_merge_ladder, (max_sweeps, max_rounds))
                        if kinds is None
                        else (self.lib.hdg_refine_split_ladder, (max_sweeps, max_rounds, kinds)))
        _lib.check(call(
            ctypes.byref(self.shape), ctypes.byref(b), ctypes.c_void_p(probs.data_ptr()),
            (ctypes.c_float * T)(*thr), T, rule, *budget, 0,
            None if merges is None else ctypes.c_void_p(merges.data_ptr()),
            None if levels is None else ctypes.c_void_p(levels.data_ptr()),
            None if out is None else ctypes.c_void_p(out.data_ptr()),
            ctypes.c_void_p(ut.data_ptr()), ctypes.c_void_p(rq.data_ptr()),
            ctypes.c_void_p(ws.data_ptr()), self._stream()))
        return ut, rq, out

    def _match_args(self, groups, mate):
        """match()'s `groups` and `mate`, checked as _refine() checks its groups -> the ids as
        [S][B][nc] (a view) and S."""
        if not isinstance(mate, bool):
            raise ValueError("mate must be a bool (got %r)" % (mate,))
        ok = (isinstance(groups, torch.Tensor) and groups.device == self.device
              and groups.dtype == torch.int32 and groups.is_contiguous())
        if ok and groups.dim() == 2:
            groups = groups.unsqueeze(0)
        if not (ok and groups.dim() == 3 and tuple(groups.shape[1:]) == (self.batch, self.nc)
                and 1 <= groups.shape[0] <= _lib.MT_MAX_SETS):
            raise ValueError("groups must be a contiguous int32 [%d][%d] or [S][%d][%d] tensor on "
                             "%s, 1 <= S <= %d" % (self.batch, self.nc, self.batch, self.nc,
                                                   self.device, _lib.MT_MAX_SETS))
        return groups, int(groups.shape[0])

    def match(self, dbatch, groups, mate=False):
        """hdg_match: how many hunks are in the right group -- per set of `groups` (int32
        [B][nc] or [S][B][nc] on this device, 1 <= S <= MT_MAX_SETS: what untangle(), cut(), a
        refine call or a ladder with groups=True returned; equal ids in [0, nc) are together,
        any other id is alone) and commit the best one-to-one assignment of predicted to true
        groups (include/hdgnn.h) -> (mt int64 [S][B][MT_SLOTS], mate int32 [S][B][nc] or None
        unless `mate`, tgroups int32 [B][nc]) as fresh device tensors
        (hdgnn.metrics.scores_from_match turns mt into scores, best_rung_match picks a ladder's
        rung).  Enqueued on the current stream; nothing is copied to the host.  The workspace is
        allocated on the first call and kept."""
        groups, S = self._match_args(groups, mate)
        self._check(dbatch)
        ws = self._workspace("_mt_workspace", lambda: self.lib.hdg_match_workspace_bytes(
            ctypes.byref(self.shape), _lib.MT_MAX_SETS), torch.int64)
        # u64 counts, every value < 2^63: int64 reads them as they are
        mt = torch.empty(S, self.batch, _lib.MT_SLOTS, dtype=torch.int64, device=self.device)
        out = (torch.empty(S, self.batch, self.nc, dtype=torch.int32, device=self.device)
               if mate else None)
        tgroups = torch.empty(self.batch, self.nc, dtype=torch.int32, device=self.device)
        b = dbatch.struct()
        _lib.check(self.lib.hdg_match(ctypes.byref(self.shape), ctypes.byref(b),
                                      ctypes.c_void_p(groups.data_ptr()), S,
                                      None if out is None else ctypes.c_void_p(out.data_ptr()),
                                      ctypes.c_void_p(tgroups.data_ptr()),
                                      ctypes.c_void_p(mt.data_ptr()),
                                      ctypes.c_void_p(ws.data_ptr()), self._stream()))
        return mt, out, tgroups
