"""Drop-in for the reference's model_N.graph2graph, backed by libhdgnn.so.

graph2graph here is model_2 (HD-GNN/S, the reference main.py's import); hdgnn.model_1 /
model_3 / model_4 export the same class for the other variants (variant attribute).

Same constructor (model_2.py:16-33), same train(args) / test(args) flow, files and
printed lines (model_2.py:336-407, 434-548); the TF graph + sess.run are replaced by
the engine (hdgnn.engine.Engine -> C ABI -> k_commit_step on MI355X):

    reference                                         here
    sess.run([..., trainer], feed_dict) (369-383)     Engine.train_step(DeviceBatch)
    sess.run([loss, loss_map, C_edge_output2]) (486)  Engine.forward(DeviceBatch)
    read_data(self, Step) -> 12 dense arrays          reader(self, Step) -> the same tuple,
                                                      then data.compact_from_read_data
    saver.save / restore (427-451)                    TF V2 bundle, TF variable names

Reference behaviours kept on purpose: every batch feeds the maps
of the first Mini_batch commits (B.2, also in test); remainder commits are dropped
(B.3); test() looks for its checkpoint under checkpoint_dir/Repo/Repo/model_2/Step and
so normally evaluates freshly initialised weights (B.8).

Data parallel: when torch.distributed is initialised with world W > 1, every batch of
Mini_batch commits is split into W contiguous shards (Mini_batch % W == 0); the flat
gradient is all-reduced once per step (Engine.allreduce).  The epoch accuracy's correct
count is computed on the device and travels in the gradient trailer, so the same
all-reduce sums it.  Outputs written to disk are gathered on rank 0.
"""
import ctypes
import os
import time

import numpy as np

from . import _lib, layout, metrics, tfckpt
from .data import compact_from_read_data, onehot_relations

HS = 20   # De_e = De_er = h_size compiled into the engine
FAULT_POLL = 16   # train(): steps between fault polls inside a long epoch


def shard_plan(n_commits, mini_batch, world=1, rank=0):
    """Per reference batch j (floor division, model_2.py:364): this rank's commit range and
    the batch positions whose maps it feeds (Esc/Etc/..[:Mini_batch], model_2.py:376-381)
    -> list of ((commit_lo, commit_hi), (pos_lo, pos_hi))."""
    if mini_batch % world:
        raise ValueError("Mini_batch=%d is not divisible by world=%d" % (mini_batch, world))
    lb = mini_batch // world
    lo = rank * lb
    return [((j * mini_batch + lo, j * mini_batch + lo + lb), (lo, lo + lb))
            for j in range(n_commits // mini_batch)]


def _default_reader(model, step):
    """The reference's own loader (utils2.read_data), imported from the caller's path the
    way model_2.py does (`from utils2 import read_data`)."""
    try:
        from utils2 import read_data
    except ImportError as e:       # no silent fallback: the dataset loader is the caller's
        raise ImportError("graph2graph needs a reader: pass reader=... or put the reference's "
                          "utils2.py on sys.path") from e
    return read_data(model, step)


def _evaluation_funcs():
    """The reference's metrics module, imported from the caller's path the way model_2.py
    does (`from EvaluationFuncs import *`, model_2.py:12; the north star keeps it as-is);
    hdgnn.metrics (the same functions restated, pinned by the reference's own outputs in
    tests/golden/metrics_tiny.*) only when EvaluationFuncs is not importable."""
    try:
        import EvaluationFuncs
        return EvaluationFuncs
    except ImportError:
        return metrics


_COUNT_W = np.array([1, 1 << 16, 1 << 32], dtype=np.int64)   # trailer count parts


class Saver(object):
    """tf.train.Saver() of build_model (model_2.py:139): every variable of the graph
    (tf.global_variables() at that point: the model's weights) saved
    as a TF V2 bundle under the TF variable names (hdgnn.tfckpt), plus this engine's TF1
    Adam slots and beta powers so a restore resumes training.  save() keeps the newest
    max_to_keep bundles (TF's default 5) and rewrites the 'checkpoint' state file, as
    Saver.save does; restore() reads a TF-written bundle too (no Adam slots: the
    optimizer state is then left as it is).  The bundle bytes are assembled and written
    by libhdgnn (tfckpt.BundleTemplate -> hdg_bundle_write); background saves go to its
    native writer thread (tfckpt.BundleWriter), which also takes the training loop's
    result-file lines, so their file writes never run on the training thread."""

    def __init__(self, model, max_to_keep=5):
        self._model = model
        self.max_to_keep = max_to_keep
        self._last = []              # prefixes saved by this Saver, oldest first
        self._dropped = []           # prefixes whose removal is queued on the writer
        self._splits = {}            # prefix -> (directory, basename)
        self._tmpl = None
        self._writer = None
        self._dirs = set()           # directories known to exist

    def _template(self):
        if self._tmpl is None:
            self._tmpl = tfckpt.BundleTemplate(self._model.variant)
        return self._tmpl

    def writer(self):
        """The native background writer (created on first use)."""
        if self._writer is None:
            self._writer = tfckpt.BundleWriter(self._template())
        return self._writer

    def _host_state(self):
        """[params | adam_m | adam_v | beta_pow] (layout.state_offsets) in one device->host
        copy."""
        return self._model.engine.state.detach().cpu().numpy().copy()

    def _mkdir(self, d):
        if d not in self._dirs:
            os.makedirs(d, exist_ok=True)
            self._dirs.add(d)

    def _split(self, prefix):
        """(directory, basename) of a prefix, memoised (the training loop books one save
        per epoch against the same few prefixes)."""
        r = self._splits.get(prefix)
        if r is None:
            if len(self._splits) > 4096:
                self._splits.clear()
            d, base = os.path.split(prefix)
            r = self._splits[prefix] = (d or ".", base)
        return r

    def _book(self, prefix):
        """max_to_keep bookkeeping of a save at prefix: (paths to delete, state-file path,
        state-file text)."""
        d, base = self._split(prefix)
        if prefix in self._last:
            self._last.remove(prefix)
        self._last.append(prefix)
        removes = []
        while self.max_to_keep and len(self._last) > self.max_to_keep:
            old = self._last.pop(0)
            self._dropped.append(old)
            removes += [old + ".index", old + ".data-00000-of-00001"]
        kept = [b for dq, b in map(self._split, self._last) if dq == d]
        return removes, os.path.join(d, "checkpoint"), tfckpt.state_file_text(base, kept)

    def save(self, sess, save_path, global_step=None, background=False, state=None):
        """background=True: the writer thread writes the bundle of this state (a host copy
        taken now, so it holds exactly this step's values) while the caller's next steps
        run; flush() waits for it and raises its error.  state: a host copy of the flat
        training state the caller already holds (graph2graph.train reads it with the epoch's
        statistics), instead of a fresh device read."""
        prefix = save_path if global_step is None else "%s-%d" % (save_path, int(global_step))
        state = self._host_state() if state is None else state
        self._mkdir(self._split(prefix)[0])
        if not background:
            self.flush()
            return self._write(prefix, state)
        self._check(self.writer().poll)    # an earlier background save failed: raise now
        removes, spath, text = self._book(prefix)
        self.writer().submit(prefix, state, removes, spath, text)
        return prefix

    def flush(self):
        if self._writer is not None:
            self._check(self._writer.flush)
            self._dropped = []           # every queued removal has run

    def _check(self, op):
        """Run the writer's flush / poll; on a failed background job re-book the keep-list
        from the files on disk before raising: the failed prefix (no index file: bundles
        are written under .tmp and renamed) leaves it, and the older bundles that job
        would have removed (it stopped before its removals) come back, oldest first, so
        the next save's max_to_keep bookkeeping deletes them and no state file lists a
        bundle that was never written."""
        try:
            op()
        except tfckpt.CheckpointError:
            def there(q):
                return os.path.exists(q + ".index")
            back = [q for q in self._dropped if there(q) and q not in self._last]
            self._last = back + [q for q in self._last if there(q)]
            self._dropped = []
            raise

    def _write(self, prefix, state):
        self._template().write(prefix, state)
        removes, spath, text = self._book(prefix)
        for f in removes:
            if os.path.exists(f):
                os.remove(f)
        with open(spath, "w") as f:
            f.write(text)
        return prefix

    def restore(self, sess, save_path):
        import torch
        self.flush()
        eng = self._model.engine
        flat, m, v, bp = tfckpt.engine_state(tfckpt.read(save_path), self._model.variant)
        eng.set_params(flat)
        if m is not None:
            eng.m.copy_(torch.from_numpy(np.asarray(m, np.float32)))
            eng.v.copy_(torch.from_numpy(np.asarray(v, np.float32)))
            eng.beta_pow.copy_(torch.from_numpy(np.asarray(bp, np.float32)))


class graph2graph(object):
    variant = 2        # model_<variant>.py

    def __init__(self, sess, Ds, Ne, Nc, Ner, Ncr, Dr, De_e, De_er, Mini_batch, checkpoint_dir,
                 epoch, Ds_inter, Dr_inter, Step, Repo, *, reader=None, device=None, seed=0,
                 lr=3e-4, process_group=None, loader="utils2", data_root=".", compact=None):
        self.sess = sess                       # accepted and ignored (no TF session)
        self.Ds, self.Ne, self.Nc, self.Ner, self.Ncr, self.Dr = Ds, Ne, Nc, Ner, Ncr, Dr
        self.Ds_inter, self.Dr_inter = Ds_inter, Dr_inter
        self.De_e, self.De_er = De_e, De_er
        self.mini_batch_num = Mini_batch
        self.epoch = epoch
        self.checkpoint_dir = checkpoint_dir
        self.Step, self.Repo = Step, Repo
        self.reader = reader or _default_reader
        if loader not in ("utils2", "fast"):
            raise ValueError("loader must be 'utils2' (the reference read_data) or 'fast'")
        self.loader, self.data_root = loader, data_root
        # (train, test, maps) CommitBatches already in compact form (hdgnn.loader.read_compact,
        # a synthetic generator): used instead of reading the dataset
        self._given = compact
        self.seed, self.lr, self.pg = seed, lr, process_group
        self.device = device
        if (Ds, Dr, De_e, De_er) != (1, 2, HS, HS):
            raise ValueError("the engine is built for Ds=1, Dr=2, De_e=De_er=20 (got %s)"
                             % ((Ds, Dr, De_e, De_er),))
        if Ner != Ne * (Ne - 1) or Ncr != Nc * (Nc - 1):
            raise ValueError("Ner/Ncr must be Ne(Ne-1)/Nc(Nc-1) (complete relation digraphs)")
        self.build_model()

    # ------------------------------------------------------------------ model
    def build_model(self):
        import torch
        from .engine import Engine
        dist = torch.distributed
        self.world = dist.get_world_size(self.pg) if dist.is_available() and dist.is_initialized() else 1
        self.rank = dist.get_rank(self.pg) if self.world > 1 else 0
        if self.mini_batch_num % self.world:
            raise ValueError("Mini_batch=%d is not divisible by world=%d"
                             % (self.mini_batch_num, self.world))
        self.local_batch = self.mini_batch_num // self.world
        dev = self.device or torch.device("cuda", torch.cuda.current_device())
        self.engine = Engine(self.Ne, self.Nc, self.local_batch, variant=self.variant,
                             device=dev, batch_global=self.mini_batch_num, lr=self.lr,
                             process_group=self.pg)
        self._initialize()
        # fetchable attributes (filled by the last step, like sess.run results)
        self.C_edge_output2 = None
        self.C_edge_output2_logits = None
        self.loss_Hedge_mse = None
        self.loss_map = None
        self.loss_para = None
        # 0.001 * l2_loss(C_edge_output) (model_2.py:122): computed by the graph but fetched
        # by neither train nor test; here filled by test()'s forward launches
        self.loss_E_HR = None
        # the training sess.run fetches C_edge_output2 only (model_2.py:369-371); set True
        # to have train() also fill C_edge_output2_logits every step
        self.fetch_logits = False
        self.saver = Saver(self)

    def _initialize(self):
        """tf.global_variables_initializer(): truncated_normal(0.1) weights, zero biases,
        fresh Adam slots and beta powers."""
        self.engine.set_params(layout.init_flat(self.seed, self.variant))

    @property
    def vars(self):
        return layout.split(self.engine.get_params(), self.variant)

    @property
    def theta(self):
        return self.vars["map_conv/map_theta2:0"]

    # ------------------------------------------------------------------ data
    def _compact(self):
        """-> (C_edge_train, C_edge_test, train, test, maps).  'utils2': the reference's
        read_data 12-tuple through the bit-exact adapter; 'fast': hdgnn.loader reads the same
        files straight into the compact form (no dense arrays, no progress-bar sleeps)."""
        if self._given is not None:
            train, test, maps = self._given
            return onehot_relations(train.y), onehot_relations(test.y), train, test, maps
        if self.loader == "fast":
            from .loader import read_compact
            train, test, maps = read_compact(self.Repo, self.Step, self.Ne, self.Nc,
                                             self.mini_batch_num, root=self.data_root)
            return onehot_relations(train.y), onehot_relations(test.y), train, test, maps
        tup = self.reader(self, self.Step)
        train, test, maps = compact_from_read_data(tup, self.Ne, self.Nc, self.mini_batch_num)
        return np.asarray(tup[4]), np.asarray(tup[5]), train, test, maps

    def _device_batches(self, part, maps):
        """Per reference batch j: this rank's shard of commits j*mb .. (j+1)*mb with the
        maps of batch positions (model_2.py:365-381: Esc/Etc/..[:Mini_batch])."""
        out = []
        for (c0, c1), (p0, p1) in shard_plan(part.B, self.mini_batch_num, self.world, self.rank):
            sh = part.slice(c0, c1).with_maps(maps.slice(p0, p1))
            out.append(self.engine.upload(sh))
        return out

    def _gather(self, arr):
        """Concatenate a per-rank (lb, ...) array over ranks on every rank."""
        if self.world == 1:
            return arr
        import torch
        t = torch.from_numpy(np.ascontiguousarray(arr)).to(self.engine.device)
        parts = [torch.empty_like(t) for _ in range(self.world)]
        torch.distributed.all_gather(parts, t, group=self.pg)
        return torch.cat(parts).cpu().numpy()

    def _allsum(self, v):
        if self.world == 1:
            return v
        import torch
        t = torch.tensor([float(v)], dtype=torch.float64, device=self.engine.device)
        torch.distributed.all_reduce(t, group=self.pg)
        return t.item()

    # ------------------------------------------------------------------ train
    def _barrier(self):
        """Ranks meet before the first step and after rank 0's host work of an epoch, so no
        rank enters a data-parallel step far behind its peers (the xGMI exchange waits a
        bounded time for peer words)."""
        if self.world > 1:
            import torch
            torch.distributed.barrier(group=self.pg)

    def train(self, args):
        """model_2.py:335-424.  Every step's pre-update losses and top_ACC count land in its
        own row of an epoch buffer on the device (hdg_outputs.stats); at the epoch's end that
        buffer and the flat training state go to pinned host memory in two stream-ordered
        copies.  Epochs are pipelined one deep: epoch i+1 is enqueued before the host waits
        for epoch i, so epoch i's result line, result file and checkpoint (written by the
        saver thread through libhdgnn) overlap epoch i+1 on the GPU.  A split-mode exchange
        timeout (a step's update skipped, the fault count in every rank's stats) re-runs
        epoch i from the host copy of the state before it, with one block per commit
        (Engine.split_fault_retry); epochs of more than FAULT_POLL steps poll the fault
        slots every FAULT_POLL steps and stop a faulted epoch early."""
        import torch
        self._initialize()
        _, _, train, _, maps = self._compact()
        batches = self._device_batches(train, maps)
        nb = len(batches)
        counter = 1
        start_time1 = time.time()
        eng = self.engine
        S, dev = eng.state.numel(), eng.device
        th_off = layout.offsets(self.variant)["map_conv/map_theta2:0"][0]
        nr = max(nb, 1)
        # device stats rows and pinned host slots per epoch parity; host state slots mod 3
        # (a retry of epoch i needs the state after i-1 while i+1 is in flight)
        es = [torch.zeros(nr, _lib.STATS_LEN, dtype=torch.float32, device=dev) for _ in range(2)]
        hs = [torch.zeros(nr, _lib.STATS_LEN, dtype=torch.float32).pin_memory() for _ in range(2)]
        hst = [torch.zeros(S, dtype=torch.float32).pin_memory() for _ in range(3)]
        hst[2].copy_(eng.state)                          # "after epoch -1": the initial state
        outs = {}
        pflag = torch.zeros(2, dtype=torch.float32).pin_memory()   # fault-poll slots
        pdone = [torch.cuda.Event() for _ in range(2)]
        # per step row and epoch parity: the step with its ctypes arguments built once; the
        # epoch's host reads and completion events through libhdgnn (hipMemcpyAsync /
        # hipEvent: no dispatcher round per epoch)
        lib = eng.lib
        steps = [[eng.step_call(db, stats=es[p][j], logits=self.fetch_logits)
                  for j, db in enumerate(batches)] for p in range(2)]
        stream = eng._stream()
        done = [ctypes.c_void_p() for _ in range(2)]
        for ev in done:
            _lib.check(lib.hdg_event_create(ctypes.byref(ev)))
        rows_bytes, state_bytes = nr * _lib.STATS_LEN * 4, S * 4
        filepath = None
        if self.rank == 0:
            filepath = r'outputSelf/{}/model_{}/{}/result_{}.npy'.format(
                args.Repo, self.variant, self.Step, self.Step)
            os.makedirs(os.path.dirname(filepath), exist_ok=True)

        def launch(i):
            """Enqueue epoch i: its steps, then the host copies of its stats and end state.
            Split fused epochs of more than FAULT_POLL steps poll the fault slots every
            FAULT_POLL steps: the poll at step j copies the fault column so far to pinned
            memory, and waits only for the previous poll's copy (FAULT_POLL steps older), so
            the GPU keeps FAULT_POLL steps queued and the host is never in lockstep with it;
            a fault stops the epoch at the next poll after the one that saw it."""
            rows = es[i % 2]
            npoll = 0
            for j, step in enumerate(steps[i % 2]):
                step()
                if nb > FAULT_POLL and (j + 1) % FAULT_POLL == 0 and j + 1 < nb and \
                        eng.split and eng.path == _lib.PATH_FUSED:
                    if npoll:
                        pdone[(npoll - 1) % 2].synchronize()
                        if pflag[(npoll - 1) % 2].item() != 0.0:   # stop a faulted epoch early
                            rows[j + 1:].zero_()
                            rows[j + 1:, 7] = 1.0
                            break
                    pflag[npoll % 2:npoll % 2 + 1].copy_(rows[:j + 1, 7].amax().reshape(1),
                                                         non_blocking=True)
                    pdone[npoll % 2].record()
                    npoll += 1
            if nb and i == self.epoch - 1:              # the fetched outputs of the last step
                outs[i] = (eng.probs.clone(), eng.logits.clone() if self.fetch_logits else None)
            _lib.check(lib.hdg_memcpy_async(ctypes.c_void_p(hs[i % 2].data_ptr()),
                                            ctypes.c_void_p(rows.data_ptr()), rows_bytes, stream))
            _lib.check(lib.hdg_memcpy_async(ctypes.c_void_p(hst[i % 3].data_ptr()),
                                            ctypes.c_void_p(eng.state.data_ptr()), state_bytes,
                                            stream))
            _lib.check(lib.hdg_event_record(done[i % 2], stream))

        try:
            self._train_epochs(args, launch, done, hs, hst, outs, nb, th_off, counter, filepath)
        finally:
            for ev in done:
                lib.hdg_event_destroy(ev)
        end_time1 = time.time()
        if self.rank == 0:
            print('test time:' + str(end_time1 - start_time1))

    def _train_epochs(self, args, launch, done, hs, hst, outs, nb, th_off, counter, filepath):
        """train()'s epoch loop: epoch i+1 enqueued before the host waits for epoch i."""
        import torch
        eng, lib, dev = self.engine, self.engine.lib, self.engine.device
        self._barrier()
        if self.epoch > 0:
            launch(0)
        i = 0
        while i < self.epoch:
            if i + 1 < self.epoch and self.world == 1:
                launch(i + 1)
            _lib.check(lib.hdg_event_synchronize(done[i % 2]))
            host = hs[i % 2].numpy().astype(np.float64)
            if host[:nb, 7].any():                       # a split-mode exchange timed out
                torch.cuda.synchronize(dev)              # epoch i+1 (if launched) drained
                if eng.split and eng.path == _lib.PATH_FUSED and eng.split_fault_retry():
                    eng.restore(hst[(i - 1) % 3].numpy())
                    outs.pop(i + 1, None)
                    launch(i)
                    continue
                eng.check_status()
                raise RuntimeError("libhdgnn: a training step faulted (stats %s)" % host[:nb])
            if not np.isfinite(host[:nb, 0]).all():      # a NaN loss: a device fault (DP
                eng.check_status()                       # timeout) raises, a diverged run
                                                         # prints nan as the reference would
            tr_loss_Hedge = float(host[:nb, 0].sum())
            tr_loss_map = float(host[:nb, 1].sum())
            # the trailer's three 16-bit count parts per step, summed exactly in int64
            correct = int((np.rint(host[:nb, 4:7]).astype(np.int64) * _COUNT_W).sum())
            state = hst[i % 3].numpy()
            if nb:
                self.loss_Hedge_mse, self.loss_map, self.loss_para = (float(host[nb - 1, 0]),
                                                                      float(host[nb - 1, 1]),
                                                                      float(host[nb - 1, 2]))
                if i in outs:
                    self.C_edge_output2, self.C_edge_output2_logits = outs.pop(i)
            acc_top = correct / (nb * self.mini_batch_num * self.Ncr) if nb else 0.0
            # theta (model_2.py:369-371, 392): map_theta2 in the state after epoch i, as
            # self.theta reads it at this point
            theta = state[th_off:th_off + 2].astype(np.float32)
            resultString = "Epoch " + str(i + 1) + \
                           " acc: " + str(acc_top)[0:6] + \
                           " Hedge loss: " + str(tr_loss_Hedge / nb if nb else 0.0)[0:6] + \
                           " map MSE: " + str(tr_loss_map / nb if nb else 0.0)[0:6] + \
                           " theta: " + str(theta[0]) + ' ' + str(theta[1]) + '\n'
            if self.rank == 0:
                # appended by the writer thread, in order with the checkpoints (same bytes
                # as the reference's open(..., "a") + write per epoch)
                self.saver.writer().submit(text_path=filepath, text=resultString, append=True)
                print(resultString)
            counter += 1
            self.save(args.checkpoint_dir, counter, background=True, state=state)
            self._barrier()
            if self.world > 1 and i + 1 < self.epoch:   # DP: ranks launch in step after the barrier
                launch(i + 1)
            i += 1
        self.saver.flush()          # every epoch's files on disk before train() returns

    # sess.run's fetched C_edge_output2 / C_edge_output2_logits.  Training keeps the last
    # step's device output as a fresh tensor per epoch (later steps never change it) and
    # hands out a host numpy copy on first access, as sess.run returns one.
    def _fetched(self, key):
        f = self.__dict__.setdefault("_fetch", {})
        v = f.get(key)
        if v is not None and not isinstance(v, np.ndarray):
            v = f[key] = v.detach().cpu().numpy()
        return v

    @property
    def C_edge_output2(self):
        return self._fetched("probs")

    @C_edge_output2.setter
    def C_edge_output2(self, v):
        self.__dict__.setdefault("_fetch", {})["probs"] = v

    @property
    def C_edge_output2_logits(self):
        return self._fetched("logits")

    @C_edge_output2_logits.setter
    def C_edge_output2_logits(self, v):
        self.__dict__.setdefault("_fetch", {})["logits"] = v

    # ------------------------------------------------------------------ checkpoints
    def _model_dir(self, checkpoint_dir):
        return os.path.join(checkpoint_dir, "%s/model_%d/%s" % (self.Repo, self.variant, self.Step))

    def save(self, checkpoint_dir, step, background=False, state=None):
        """saver.save(sess, <dir>/g2g.model, global_step=step) (model_2.py:427-437): a TF V2
        bundle g2g.model-<step>.index / .data-00000-of-00001 under the TF variable names
        (hdgnn.tfckpt), plus TF1 Adam's slots and beta powers so training can resume, and
        the 'checkpoint' state file tf.train.get_checkpoint_state reads.  train() saves in
        the background (Saver.save(background=True)): the state is read at the epoch's end,
        the files are written while the next epoch runs, and train() flushes before it
        returns."""
        if self.rank != 0:
            return
        self.saver.save(self.sess, os.path.join(self._model_dir(checkpoint_dir), "g2g.model"),
                        global_step=step, background=background, state=state)

    def load(self, checkpoint_dir):
        """get_checkpoint_state + saver.restore (model_2.py:439-451).  Reads TF V2 bundles
        (this framework's or the reference's own; the latter carry no Adam slots, so the
        optimizer state is left as initialised) and this framework's older .npz files."""
        print(" [*] Reading checkpoint...")
        self.saver.flush()
        d = self._model_dir(checkpoint_dir)
        name = tfckpt.latest(d)
        if not name:
            return False
        path = os.path.join(d, name)
        if os.path.exists(path + ".index"):
            self.saver.restore(self.sess, path)
            return True
        if os.path.exists(path + ".npz"):
            z = np.load(path + ".npz", allow_pickle=False)
            flat = np.concatenate([np.asarray(z[n], np.float32).reshape(-1)
                                   for n, _ in layout.specs(self.variant)])
            m, v, bp = ((z["_adam_m"], z["_adam_v"], z["_beta_pow"]) if "_adam_m" in z
                        else (None, None, None))
        else:
            return False
        import torch
        eng = self.engine
        eng.set_params(flat)
        if m is not None:
            eng.m.copy_(torch.from_numpy(np.asarray(m, np.float32)))
            eng.v.copy_(torch.from_numpy(np.asarray(v, np.float32)))
            eng.beta_pow.copy_(torch.from_numpy(np.asarray(bp, np.float32)))
        return True

    # ------------------------------------------------------------------ evaluate
    def evaluate(self, args, part="test"):
        """Score the trained classifier on the test (or train) split without moving the
        probabilities: per batch Engine.forward then Engine.evaluate (hdg_eval), and only the
        per-commit integer rows (include/hdgnn.h, HDG_EV_*) come to the host.  Not a reference
        flow: unlike test() it restores the checkpoint from where train() saves it, and its
        scores are the usual ones (metrics.scores_from_counts), not EvaluationFuncs' quirks.
        Same batches as test(): shard_plan over the part, the maps of the first Mini_batch
        commits, remainder commits dropped.  -> (scores dict, int64 table [n_commits][8]);
        rank 0 prints the scores and writes the table to
        outputSelf/<Repo>/model_<v>/<Step>/eval_counts<Ne>.npy."""
        import torch
        if part not in ("train", "test"):
            raise ValueError("part must be 'train' or 'test' (got %r)" % (part,))
        _, _, train, test, maps = self._compact()
        if self.load(self.checkpoint_dir):
            print(" [*] Load SUCCESS")
        else:
            print(" [!] Load failed...")
        eng = self.engine
        rows = []
        for db in self._device_batches(train if part == "train" else test, maps):
            eng.forward(db)
            rows.append(eng.evaluate(db))
        nb = len(rows)
        table = (torch.stack(rows).cpu().numpy() if nb
                 else np.zeros((0, self.local_batch, _lib.EV_SLOTS), np.int64))
        eng.check_status()
        if self.world > 1 and nb:      # rank-major (W nb, lb, 8) -> batch-major commit order
            table = self._gather(table).reshape(self.world, nb, self.local_batch, _lib.EV_SLOTS)
            table = table.transpose(1, 0, 2, 3)
        table = np.ascontiguousarray(table.reshape(-1, _lib.EV_SLOTS)).astype(np.int64)
        scores = metrics.scores_from_counts(table)
        if self.rank == 0:
            step_dir = 'outputSelf/%s/model_%d/%s/' % (args.Repo, self.variant, self.Step)
            os.makedirs(step_dir, exist_ok=True)
            np.save(step_dir + 'eval_counts' + str(self.Ne) + '.npy', table)
            for name in ("acc", "precision", "recall", "f1"):
                print('eval %s: %s (per-commit mean %s)' % (name, scores[name],
                                                            scores[name + "_mean"]))
            print('eval auc: %s (%d of %d commits)' % (scores["auc"], scores["auc_commits"],
                                                       len(table)))
            print('eval nan relations: %d' % scores["nan_relations"])
        return scores, table

    @staticmethod
    def _check_merge(merge, refine):
        """untangle()'s and calibrate_refined()'s `merge`: the rounds of hdg_refine_merge."""
        if not (isinstance(merge, int) and 0 <= merge <= _lib.RM_MAX_ROUNDS):
            raise ValueError("merge must be an int in [0, %d] (got %r)"
                             % (_lib.RM_MAX_ROUNDS, merge))
        if merge and refine < 1:
            raise ValueError("merge > 0 needs refine >= 1 (got refine = %r)" % (refine,))

    @staticmethod
    def _check_split(split, merge):
        """untangle()'s and calibrate_refined()'s `split`: hdg_refine_split's split sweeps in
        the rounds that `merge` counts."""
        if not isinstance(split, bool):
            raise ValueError("split must be a bool (got %r)" % (split,))
        if split and merge < 1:
            raise ValueError("split needs merge >= 1, the rounds (got merge = %r)" % (merge,))

    # ------------------------------------------------------------------ untangle
    def untangle(self, args, part="test", threshold=0.5, rule="mean", method="single", refine=0,
                 merge=0, split=False, match=False):
        """Untangle the commits of the test (or train) split with the trained classifier: per
        batch Engine.forward then Engine.untangle (hdg_untangle), so only each commit's hunk
        group ids and its integer row (include/hdgnn.h, HDG_UT_*) come to the host, never the
        probabilities.  Not a reference flow (the reference stops at the pair scores).  As
        evaluate(): the checkpoint from where train() saves it, the batches of test().
        -> (scores dict, int64 table [n_commits][8], int32 groups [n_commits][Nc]); rank 0
        prints the scores (metrics.scores_from_untangle) and writes untangle_groups<Ne>.npy
        and untangle_counts<Ne>.npy under outputSelf/<Repo>/model_<v>/<Step>/.
        method "complete" | "average": the groups are the cut at `threshold` of each commit's
        merge tree under that linkage instead (Engine.agglomerate then Engine.cut: hdg_cut's
        row, whose slot 6 holds the merges done, not the linked pairs); "single" is
        hdg_untangle, the link graph's components.
        refine > 0: the groups of either path go through Engine.refine (hdg_refine: at most
        `refine` best-move sweeps at the same threshold and rule); the refined groups and
        table (slot 6: the moves made) are what is returned and saved, and
        untangle_refine<Ne>.npy holds each commit's objective row (HDG_RF_Q_*).
        merge > 0 (needs refine >= 1): the refinement is Engine.refine_merge (hdg_refine_merge:
        at most `merge` rounds of node sweeps and one group sweep, `refine` the total of node
        sweeps); the objective rows have 8 columns, the first four with their meaning
        (HDG_RM_Q_*), and one more line reports rounds, merges and the objective.
        split (needs merge >= 1): the refinement is Engine.refine_split with kinds "both"
        (hdg_refine_split: every round also runs a split sweep, in which a group is cut in
        two); the objective rows keep 8 columns, the last the accepted splits, and one more
        line reports them.
        match: after the groups are final, whatever produced them, one Engine.match call per
        batch (hdg_match: the hunks in the right group under the best one-to-one assignment of
        predicted to true groups); one more line reports accuracy, its per-commit mean, purity
        and cover (metrics.scores_from_match), match_counts<Ne>.npy holds each commit's row
        (HDG_MT_*), and the scores dict gains "match", that dict."""
        import torch
        if not isinstance(match, bool):
            raise ValueError("match must be a bool (got %r)" % (match,))
        if part not in ("train", "test"):
            raise ValueError("part must be 'train' or 'test' (got %r)" % (part,))
        if method not in _lib.AG_METHODS:
            raise ValueError("method must be one of %s (got %r)"
                             % (", ".join(_lib.AG_METHODS), method))
        if not (isinstance(refine, int) and 0 <= refine <= _lib.RF_MAX_SWEEPS):
            raise ValueError("refine must be an int in [0, %d] (got %r)"
                             % (_lib.RF_MAX_SWEEPS, refine))
        self._check_merge(merge, refine)
        self._check_split(split, merge)
        qslots = _lib.RM_Q_SLOTS if merge else _lib.RF_Q_SLOTS
        _, _, train, test, maps = self._compact()
        if self.load(self.checkpoint_dir):
            print(" [*] Load SUCCESS")
        else:
            print(" [!] Load failed...")
        eng = self.engine
        rows, ids, qs, ms = [], [], [], []
        for db in self._device_batches(train if part == "train" else test, maps):
            eng.forward(db)
            if method == "single":
                g, ut = eng.untangle(db, threshold=threshold, rule=rule)
            else:
                m, lv, cv, _, lk = eng.agglomerate(db, rule=rule, method=method)
                g, ut = eng.cut(m, lv, cv, lk, threshold=threshold, rule=rule)
            if split:
                g, ut, rq = eng.refine_split(db, g, threshold=threshold, rule=rule,
                                             max_sweeps=refine, max_rounds=merge, kinds="both")
                qs.append(rq)
            elif merge:
                g, ut, rq = eng.refine_merge(db, g, threshold=threshold, rule=rule,
                                             max_sweeps=refine, max_rounds=merge)
                qs.append(rq)
            elif refine:
                g, ut, rq = eng.refine(db, g, threshold=threshold, rule=rule, max_sweeps=refine)
                qs.append(rq)
            if match:
                ms.append(eng.match(db, g)[0][0])
            ids.append(g)
            rows.append(ut)
        nb, lb = len(rows), self.local_batch
        table = (torch.stack(rows).cpu().numpy() if nb
                 else np.zeros((0, lb, _lib.UT_SLOTS), np.int64))
        groups = (torch.stack(ids).cpu().numpy() if nb else np.zeros((0, lb, self.Nc), np.int32))
        eng.check_status()
        if self.world > 1 and nb:      # rank-major (W nb, lb, ..) -> batch-major commit order
            table = self._gather(table).reshape(self.world, nb, lb, _lib.UT_SLOTS)
            table = table.transpose(1, 0, 2, 3)
            groups = self._gather(groups).reshape(self.world, nb, lb, self.Nc)
            groups = groups.transpose(1, 0, 2, 3)
        if refine:
            qrows = (torch.stack(qs).cpu().numpy() if nb
                     else np.zeros((0, lb, qslots), np.int64))
            if self.world > 1 and nb:
                qrows = self._gather(qrows).reshape(self.world, nb, lb, qslots)
                qrows = qrows.transpose(1, 0, 2, 3)
            qrows = np.ascontiguousarray(qrows.reshape(-1, qslots)).astype(np.int64)
        if match:
            mrows = (torch.stack(ms).cpu().numpy() if nb
                     else np.zeros((0, lb, _lib.MT_SLOTS), np.int64))
            if self.world > 1 and nb:
                mrows = self._gather(mrows).reshape(self.world, nb, lb, _lib.MT_SLOTS)
                mrows = mrows.transpose(1, 0, 2, 3)
            mrows = np.ascontiguousarray(mrows.reshape(-1, _lib.MT_SLOTS)).astype(np.int64)
        table = np.ascontiguousarray(table.reshape(-1, _lib.UT_SLOTS)).astype(np.int64)
        groups = np.ascontiguousarray(groups.reshape(-1, self.Nc)).astype(np.int32)
        scores = metrics.scores_from_untangle(table)
        if match:
            scores["match"] = metrics.scores_from_match(mrows, self.Nc)
        if self.rank == 0:
            step_dir = 'outputSelf/%s/model_%d/%s/' % (args.Repo, self.variant, self.Step)
            os.makedirs(step_dir, exist_ok=True)
            np.save(step_dir + 'untangle_groups' + str(self.Ne) + '.npy', groups)
            np.save(step_dir + 'untangle_counts' + str(self.Ne) + '.npy', table)
            print('untangle rule: %s, threshold %s' % (rule, threshold))
            if method != "single":
                print('untangle method: %s' % method)
            if refine:
                np.save(step_dir + 'untangle_refine' + str(self.Ne) + '.npy', qrows)
                print('untangle refine: %d sweeps at most, %d moves, %d of %d commits converged'
                      % (refine, int(table[:, _lib.RF_MOVES].sum()),
                         int(qrows[:, _lib.RF_Q_CONVERGED].sum()), len(qrows)))
                print('untangle refine objective: %d -> %d'
                      % (int(qrows[:, _lib.RF_Q_START].sum()), int(qrows[:, _lib.RF_Q_END].sum())))
            if merge:
                print('untangle merge: %d rounds at most, %d rounds, %d merges, objective after '
                      'the first node phase %d -> %d at the end'
                      % (merge, int(qrows[:, _lib.RM_Q_ROUNDS].sum()),
                         int(qrows[:, _lib.RM_Q_MERGES].sum()),
                         int(qrows[:, _lib.RM_Q_NODE].sum()), int(qrows[:, _lib.RF_Q_END].sum())))
            if split:
                print('untangle split: %d splits in %d of %d commits'
                      % (int(qrows[:, _lib.RS_Q_SPLITS].sum()),
                         int(np.count_nonzero(qrows[:, _lib.RS_Q_SPLITS])), len(qrows)))
            for name in ("rand", "precision", "recall", "f1"):
                print('untangle %s: %s (per-commit mean %s)' % (name, scores[name],
                                                                scores[name + "_mean"]))
            print('untangle exact partitions: %s, group count match: %s (%d commits)'
                  % (scores["exact"], scores["group_count_match"], len(table)))
            print('untangle nan pairs: %d' % scores["nan_pairs"])
            if match:
                np.save(step_dir + 'match_counts' + str(self.Ne) + '.npy', mrows)
                sm = scores["match"]
                print('untangle match: accuracy %s (per-commit mean %s), purity %s, cover %s'
                      % (sm["accuracy"], sm["accuracy_mean"], sm["purity"], sm["cover"]))
        return scores, table, groups

    # ------------------------------------------------------------------ calibrate
    def calibrate(self, args, part="train", rule="mean", score="f1", method="single"):
        """The link threshold untangle() should use: the one with the best pooled `score`
        ("f1" | "rand") over the commits of the train (or test) split, exactly.  Per batch
        Engine.forward then Engine.linkage (hdg_linkage), so only each commit's merge tree
        and its integer curve (include/hdgnn.h, HDG_LK_*: Nc - 1 rows) come to the host,
        never the probabilities; metrics.best_threshold does the rest.  Checkpoint, batches
        and multi-rank gather as untangle().  -> (threshold, scores dict at that threshold
        (metrics.scores_from_untangle of metrics.cut_table), levels float32 [n_commits][Nc-1],
        curve int64 [n_commits][Nc-1][2], lk int64 [n_commits][8]); rank 0 prints the result
        and writes linkage_levels<Ne>.npy, linkage_curve<Ne>.npy, linkage_merges<Ne>.npy and
        linkage_counts<Ne>.npy under outputSelf/<Repo>/model_<v>/<Step>/.
        method "complete" | "average": the trees are Engine.agglomerate's under that linkage
        (hdg_agglomerate) and the threshold is the one untangle(method=...) should use; the
        files are agglo_<method>_levels<Ne>.npy, _curve, _merges and _counts."""
        import torch
        if score == "acc":
            raise ValueError("score 'acc' needs a matching per cut: use calibrate_refined, which "
                             "scores the rungs of a ladder with hdg_match")
        if part not in ("train", "test"):
            raise ValueError("part must be 'train' or 'test' (got %r)" % (part,))
        if method not in _lib.AG_METHODS:
            raise ValueError("method must be one of %s (got %r)"
                             % (", ".join(_lib.AG_METHODS), method))
        _, _, train, test, maps = self._compact()
        if self.load(self.checkpoint_dir):
            print(" [*] Load SUCCESS")
        else:
            print(" [!] Load failed...")
        eng = self.engine
        outs = []
        for db in self._device_batches(train if part == "train" else test, maps):
            eng.forward(db)
            m, lv, cv, _, lk = (eng.linkage(db, rule=rule) if method == "single"
                                else eng.agglomerate(db, rule=rule, method=method))
            outs.append((m, lv, cv, lk))
        nb, lb, n1 = len(outs), self.local_batch, self.Nc - 1
        tails = ((n1, 2), (n1,), (n1, 2), (_lib.LK_SLOTS,))
        dtypes = (np.int32, np.float32, np.int32, np.int64)
        arrs = [(torch.stack([o[i] for o in outs]).cpu().numpy() if nb
                 else np.zeros((0, lb) + tails[i], dtypes[i])) for i in range(4)]
        eng.check_status()
        if self.world > 1 and nb:      # rank-major (W nb, lb, ..) -> batch-major commit order
            arrs = [self._gather(a).reshape((self.world, nb, lb) + tails[i])
                    .transpose((1, 0, 2) + tuple(range(3, 3 + len(tails[i]))))
                    for i, a in enumerate(arrs)]
        merges, levels, curve, lk = (np.ascontiguousarray(a.reshape((-1,) + tails[i]))
                                     for i, a in enumerate(arrs))
        curve, lk = curve.astype(np.int64), lk.astype(np.int64)
        threshold, best, tprime = metrics.best_threshold(levels, curve, lk, rule, score)
        scores = metrics.scores_from_untangle(metrics.cut_table(levels, curve, lk, tprime))
        if self.rank == 0:
            step_dir = 'outputSelf/%s/model_%d/%s/' % (args.Repo, self.variant, self.Step)
            os.makedirs(step_dir, exist_ok=True)
            stem = step_dir + ('linkage_' if method == "single" else 'agglo_%s_' % method)
            np.save(stem + 'levels' + str(self.Ne) + '.npy', levels)
            np.save(stem + 'curve' + str(self.Ne) + '.npy', curve)
            np.save(stem + 'merges' + str(self.Ne) + '.npy', merges)
            np.save(stem + 'counts' + str(self.Ne) + '.npy', lk)
            print('calibrate rule: %s, part %s (%d commits)' % (rule, part, len(lk)))
            if method != "single":
                print('calibrate method: %s' % method)
            print('calibrate score: %s = %s' % (score, best))
            print('calibrate threshold: %r (link bound %r)' % (threshold, tprime))
        return threshold, scores, levels, curve, lk

    # ------------------------------------------------------------------ calibrate_refined
    def calibrate_refined(self, args, part="train", rule="mean", score="f1", method="single",
                          refine=8, ladder=(0.05, 0.95, 19), merge=0, split=False):
        """The link threshold untangle(refine=N) should use: the rung of `ladder` = (lo, hi, n)
        (metrics.ladder) with the best pooled `score` of the REFINED groups over the commits of
        the train (or test) split -- the objective's threshold is not the tree's best cut,
        which calibrate() returns.  Per batch Engine.forward, then the merge tree as
        calibrate() builds it (Engine.linkage, or Engine.agglomerate under `method`), then
        Engine.refine_ladder from that tree (hdg_refine_ladder: every rung cut from the tree
        and refined with at most `refine` sweeps, in one call); only the integer rows of each
        commit and rung and the trees come to the host.  Checkpoint, batches and multi-rank
        gather as untangle().  -> (threshold, scores dict at it (metrics.scores_from_untangle
        of that rung's table), thresholds float32 [T], table int64 [T][n_commits][8], rq int64
        [T][n_commits][4]); rank 0 prints one line per rung, the chosen rung and the tree's
        own best (metrics.best_threshold on the same trees) beside it, and writes
        refine_ladder_thresholds<Ne>.npy, refine_ladder_counts<Ne>.npy and
        refine_ladder_objective<Ne>.npy under outputSelf/<Repo>/model_<v>/<Step>/.
        merge > 0: the threshold untangle(refine=N, merge=R) should use -- the ladder is
        Engine.refine_merge_ladder (hdg_refine_merge_ladder), every rung refined in at most
        `merge` rounds; rq has 8 columns, the first four with their meaning, and each rung's
        line is followed by one with its rounds, merges and objective.
        split (needs merge >= 1): the threshold untangle(refine=N, merge=R, split=True) should
        use -- the ladder is Engine.refine_split_ladder with kinds "both"
        (hdg_refine_split_ladder); rq keeps 8 columns, the last the accepted splits, and each
        rung gets one more line with them.
        score "acc": the rung is chosen by the pooled matching accuracy -- the hunks in the right
        group under the best one-to-one assignment of predicted to true groups, over all hunks
        (metrics.best_rung_match).  The ladder leaves its groups on the device and one
        Engine.match call per batch (hdg_match) scores the T rungs there; the "tree alone" lines
        compare with the tree's plain cuts at the same T thresholds (Engine.cut per rung,
        stacked, one more Engine.match call), the exactly best cut over all Nc - 1 cuts not being
        available for this score.  The scores dict gains "match" (metrics.scores_from_match of
        the chosen rung) and refine_ladder_match<Ne>.npy holds the rows [T][n_commits][8]."""
        import torch
        acc = score == "acc"
        if part not in ("train", "test"):
            raise ValueError("part must be 'train' or 'test' (got %r)" % (part,))
        if method not in _lib.AG_METHODS:
            raise ValueError("method must be one of %s (got %r)"
                             % (", ".join(_lib.AG_METHODS), method))
        if not (isinstance(refine, int) and 1 <= refine <= _lib.RF_MAX_SWEEPS):
            raise ValueError("refine must be an int in [1, %d] (got %r)"
                             % (_lib.RF_MAX_SWEEPS, refine))
        self._check_merge(merge, refine)
        self._check_split(split, merge)
        qslots = _lib.RM_Q_SLOTS if merge else _lib.RF_Q_SLOTS
        thresholds = metrics.ladder(*ladder)
        T = len(thresholds)
        _, _, train, test, maps = self._compact()
        if self.load(self.checkpoint_dir):
            print(" [*] Load SUCCESS")
        else:
            print(" [!] Load failed...")
        eng = self.engine
        outs = []
        more = {"groups": True} if acc else {}     # without "acc" every call is as it was
        for db in self._device_batches(train if part == "train" else test, maps):
            eng.forward(db)
            m, lv, cv, _, lk = (eng.linkage(db, rule=rule) if method == "single"
                                else eng.agglomerate(db, rule=rule, method=method))
            if split:
                ut, rq, lg = eng.refine_split_ladder(db, thresholds.tolist(), tree=(m, lv),
                                                     rule=rule, max_sweeps=refine,
                                                     max_rounds=merge, kinds="both", **more)
            elif merge:
                ut, rq, lg = eng.refine_merge_ladder(db, thresholds.tolist(), tree=(m, lv),
                                                     rule=rule, max_sweeps=refine,
                                                     max_rounds=merge, **more)
            else:
                ut, rq, lg = eng.refine_ladder(db, thresholds.tolist(), tree=(m, lv), rule=rule,
                                               max_sweeps=refine, **more)
            # batch-major like the tree's arrays, the rungs inside: [lb][T][slots]
            outs.append((lv, cv, lk, ut.transpose(0, 1).contiguous(),
                         rq.transpose(0, 1).contiguous()))
            if acc:                    # the rungs' groups and the tree's plain cuts, matched
                cuts = torch.stack([eng.cut(m, lv, cv, lk, threshold=float(t), rule=rule)[0]
                                    for t in thresholds])
                outs[-1] += (eng.match(db, lg)[0].transpose(0, 1).contiguous(),
                             eng.match(db, cuts)[0].transpose(0, 1).contiguous())
        nb, lb, n1 = len(outs), self.local_batch, self.Nc - 1
        tails = ((n1,), (n1, 2), (_lib.LK_SLOTS,), (T, _lib.RF_SLOTS), (T, qslots))
        dtypes = (np.float32, np.int32, np.int64, np.int64, np.int64)
        if acc:
            tails += ((T, _lib.MT_SLOTS),) * 2
            dtypes += (np.int64,) * 2
        arrs = [(torch.stack([o[i] for o in outs]).cpu().numpy() if nb
                 else np.zeros((0, lb) + tails[i], dtypes[i])) for i in range(len(tails))]
        eng.check_status()
        if self.world > 1 and nb:      # rank-major (W nb, lb, ..) -> batch-major commit order
            arrs = [self._gather(a).reshape((self.world, nb, lb) + tails[i])
                    .transpose((1, 0, 2) + tuple(range(3, 3 + len(tails[i]))))
                    for i, a in enumerate(arrs)]
        levels, curve, lk, table, qrows = (np.ascontiguousarray(a.reshape((-1,) + tails[i]))
                                           for i, a in enumerate(arrs[:5]))
        curve, lk = curve.astype(np.int64), lk.astype(np.int64)
        table = np.ascontiguousarray(table.transpose(1, 0, 2)).astype(np.int64)    # [T][n][8]
        qrows = np.ascontiguousarray(qrows.transpose(1, 0, 2)).astype(np.int64)
        if acc:
            mrows, trows = (np.ascontiguousarray(a.reshape((-1,) + tails[5]).transpose(1, 0, 2))
                            .astype(np.int64) for a in arrs[5:])
            k, threshold, best, vals = metrics.best_rung_match(mrows, thresholds, self.Nc)
            scores = metrics.scores_from_untangle(table[k])
            scores["match"] = metrics.scores_from_match(mrows[k], self.Nc)
            _, tree_thr, tree_best, _ = metrics.best_rung_match(trows, thresholds, self.Nc)
        else:
            k, threshold, best, vals = metrics.best_rung(table, thresholds, score)
            scores = metrics.scores_from_untangle(table[k])
            tree_thr, tree_best, _ = metrics.best_threshold(levels, curve, lk, rule, score)
        if self.rank == 0:
            step_dir = 'outputSelf/%s/model_%d/%s/' % (args.Repo, self.variant, self.Step)
            os.makedirs(step_dir, exist_ok=True)
            np.save(step_dir + 'refine_ladder_thresholds' + str(self.Ne) + '.npy', thresholds)
            np.save(step_dir + 'refine_ladder_counts' + str(self.Ne) + '.npy', table)
            np.save(step_dir + 'refine_ladder_objective' + str(self.Ne) + '.npy', qrows)
            if acc:
                np.save(step_dir + 'refine_ladder_match' + str(self.Ne) + '.npy', mrows)
            n = table.shape[1]
            print('calibrate refined rule: %s, part %s (%d commits), method %s, %d sweeps at most'
                  % (rule, part, n, method, refine))
            for j in range(T):
                print('calibrate refined rung %d: threshold %r, %s = %s, %d moves, %d of %d '
                      'commits converged'
                      % (j, float(thresholds[j]), score, vals[j],
                         int(table[j, :, _lib.RF_MOVES].sum()),
                         int(qrows[j, :, _lib.RF_Q_CONVERGED].sum()), n))
                if merge:
                    print('calibrate refined rung %d merge: %d rounds, %d merges, objective '
                          'after the first node phase %d -> %d at the end'
                          % (j, int(qrows[j, :, _lib.RM_Q_ROUNDS].sum()),
                             int(qrows[j, :, _lib.RM_Q_MERGES].sum()),
                             int(qrows[j, :, _lib.RM_Q_NODE].sum()),
                             int(qrows[j, :, _lib.RF_Q_END].sum())))
                if split:
                    print('calibrate refined rung %d split: %d splits in %d of %d commits'
                          % (j, int(qrows[j, :, _lib.RS_Q_SPLITS].sum()),
                             int(np.count_nonzero(qrows[j, :, _lib.RS_Q_SPLITS])), n))
            print('calibrate refined threshold: %r (rung %d), %s = %s' % (threshold, k, score, best))
            print('calibrate refined tree alone: threshold %r, %s = %s' % (tree_thr, score,
                                                                          tree_best))
            if best > tree_best:
                print('calibrate refined: the refined rung scores higher than the tree alone')
            elif tree_best > best:
                print('calibrate refined: the tree alone scores higher than every refined rung')
            else:
                print('calibrate refined: neither scores higher (equal, or no score defined)')
        return threshold, scores, thresholds, table, qrows

    # ------------------------------------------------------------------ test
    def test(self, args):
        _, C_edge_test, _, test, maps = self._compact()
        self._initialize()
        checkpoint_dir = os.path.join(self.checkpoint_dir, self.Repo)
        if self.load(checkpoint_dir):
            print(" [*] Load SUCCESS")
        else:
            print(" [!] Load failed...")
        te_loss_Hedge = 0.0
        te_loss_map = 0.0
        C_edge_t = []
        eng = self.engine
        start_time = time.time()
        end_time = start_time
        for db in self._device_batches(test, maps):
            probs, logits, ce_sum = eng.forward(db)
            p = probs.cpu().numpy()
            self.C_edge_output2_logits = logits.clone()     # not overwritten by later batches
            self.loss_E_HR = self._allsum(float(eng.ehr.item()))
            eng.check_status()
            ce = self._allsum(float(ce_sum.item())) / (self.mini_batch_num * self.Ncr)
            th1 = self.vars["map_conv/map_theta1:0"].reshape(-1).astype(np.float64)
            th2 = self.vars["map_conv/map_theta2:0"].reshape(-1).astype(np.float64)
            lmap = 0.01 * (np.sqrt((th2 ** 2).sum()) + np.sqrt((th1 ** 2).sum()))
            end_time = time.time()
            te_loss_Hedge += ce
            te_loss_map += lmap
            self.C_edge_output2 = p
            C_edge_t.append(self._gather(p))
        n_used = len(C_edge_t) * self.mini_batch_num
        C_edge_t1 = (np.array(C_edge_t).reshape(n_used, self.Dr, self.Ncr) if C_edge_t
                     else np.zeros((0, self.Dr, self.Ncr), np.float32))
        if self.rank != 0:
            return
        step_dir = 'outputSelf/%s/model_%d/%s/' % (args.Repo, self.variant, self.Step)
        os.makedirs(step_dir, exist_ok=True)
        np.save(step_dir + 'C_edge_t' + str(self.Ne) + '.npy', C_edge_t1)
        np.save(step_dir + 'C_edge_y' + str(self.Ne) + '.npy',
                C_edge_test.reshape(len(C_edge_test), self.Dr, self.Ncr))
        ev = _evaluation_funcs()
        C_edge_t2 = ev.process_edge(C_edge_t1)
        C_edge_y = C_edge_test[:n_used]
        print('topol_acc: ' + str(ev.top_ACC(C_edge_y, C_edge_t2)))
        print('prec: ' + str(ev.prec(C_edge_y, C_edge_t2)))
        print('recall: ' + str(ev.recall(C_edge_y, C_edge_t2)))
        print('F1-score: ' + str(ev.f1(C_edge_y, C_edge_t2)))
        print('AUC-score: ' + str(ev.AUC(C_edge_y, C_edge_t2)))
        print('test time:' + str(end_time - start_time))
