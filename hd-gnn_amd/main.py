# -*- coding: utf-8 -*-
"""Drop-in for the reference's main.py: the same argparse surface and the same loop over
the three glide step configurations (main.py:10-73), running hdgnn.model.graph2graph on
MI355X instead of a TF1 session.

    python hd-gnn_amd/main.py --Type train [--epoch 50 --Mini_batch 50 ...]
    python -m torch.distributed.run --nproc-per-node N --master-addr 127.0.0.1 \\
        hd-gnn_amd/main.py --Type train          # data parallel over N GPUs (RCCL)
    python hd-gnn_amd/main.py --Type eval      # accuracy / precision / recall / F1 / ROC-AUC
                                               # of the trained model, computed on the device
    python hd-gnn_amd/main.py --Type untangle [--link-threshold 0.5 --link-rule mean]
                                               # hunk groups per commit and partition scores
    python hd-gnn_amd/main.py --Type untangle --link-threshold auto [--link-score f1]
                                               # ... at the threshold calibrated on the train split
    python hd-gnn_amd/main.py --Type calibrate # that threshold alone (merge trees on the device)
    python hd-gnn_amd/main.py --Type calibrate --link-method average
    python hd-gnn_amd/main.py --Type untangle --link-threshold auto --link-method complete
                                               # groups from complete / average linkage trees
    python hd-gnn_amd/main.py --Type untangle --link-method average --link-refine 8
                                               # ... then up to 8 best-move sweeps over them
    python hd-gnn_amd/main.py --Type untangle --link-threshold refined --link-refine 8 \\
        [--link-ladder 0.05:0.95:19]           # ... at the threshold calibrated for the REFINED
                                               # groups: the best rung of the ladder LO:HI:N
    python hd-gnn_amd/main.py --Type calibrate --link-threshold refined --link-refine 8
                                               # that threshold alone (one ladder call per batch)
    python hd-gnn_amd/main.py --Type untangle --link-threshold refined --link-refine 8 \\
        --link-merge 4                         # ... whole groups may merge between the sweeps:
                                               # up to 4 rounds of node sweeps + one group sweep
    python hd-gnn_amd/main.py --Type untangle --link-threshold refined --link-refine 8 \\
        --link-merge 4 --link-split            # ... and a fused group may be cut in two: every
                                               # round also runs one split sweep
    python hd-gnn_amd/main.py --Type untangle --link-match
                                               # ... and how many hunks are in the right group
                                               # (best assignment of predicted to true groups)
    python hd-gnn_amd/main.py --Type untangle --link-threshold refined --link-refine 8 \\
        --link-score acc --link-match          # the ladder's rung chosen by that accuracy

The dataset loader is the reference's utils2.read_data (put its directory on
PYTHONPATH, as the reference's own main.py expects it next to itself).
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def _init_distributed():
    import torch
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world > 1 and not torch.distributed.is_initialized():
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        local = int(os.environ.get("LOCAL_RANK", "0"))
        torch.cuda.set_device(local)
        torch.distributed.init_process_group("nccl", device_id=torch.device("cuda", local))


def _threshold(text):
    return text if text in ('auto', 'refined') else float(text)


def _ladder(text):
    """LO:HI:N -> (lo, hi, n), checked as hdgnn.metrics.ladder checks it."""
    import math
    try:
        lo, hi, n = text.split(':')
        lo, hi, n = float(lo), float(hi), int(n)
    except ValueError:
        raise argparse.ArgumentTypeError("expected LO:HI:N (got %r)" % (text,))
    if not (math.isfinite(lo) and math.isfinite(hi) and 1 <= n <= 64):
        raise argparse.ArgumentTypeError("LO:HI:N needs finite ends and 1 <= N <= 64 (got %r)"
                                         % (text,))
    return lo, hi, n


def _variant(argv):
    """Additions to the reference's flags (every reference flag is unchanged):
    --model N (1..4, default 2 = the reference main.py's `from model_2 import`): which
    model_N.graph2graph to run; --loader utils2|fast: the reference's read_data (default)
    or hdgnn.loader reading the same dataset files straight into the compact form;
    --link-threshold T (default 0.5) and --link-rule mean|any|both (default mean): how
    --Type untangle turns pair scores into links (include/hdgnn.h, hdg_untangle);
    --link-threshold auto: the threshold with the best pooled --link-score f1|rand (default
    f1) on the train split, from the commits' merge trees (hdg_linkage), which --Type
    calibrate computes alone; --link-method single|complete|average (default single: the link
    graph's components): the linkage whose merge tree both cut (hdg_agglomerate, hdg_cut);
    --link-refine N (default 0: none): --Type untangle passes its groups through at most N
    best-move sweeps (hdg_refine) at the same threshold and rule -- with --link-threshold auto
    the one calibrated for the tree; --Type calibrate does not look at it, except with
    --link-threshold refined: the threshold with the best pooled --link-score of the groups
    REFINED with at most --link-refine N sweeps (N >= 1 is required), among the rungs of
    --link-ladder LO:HI:N (default 0.05:0.95:19), every rung cut from the commits' merge trees
    and refined in one call (hdg_refine_ladder); --Type calibrate computes it alone, --Type
    untangle uses it;
    --link-merge R (default 0: none; at most 16; needs --link-refine N >= 1): the refinement
    runs in at most R rounds, each the node sweeps followed by one group sweep in which whole
    groups merge, N the total of node sweeps (hdg_refine_merge, hdg_refine_merge_ladder), in
    --Type untangle and in the ladder of --link-threshold refined alike;
    --link-split (needs --link-merge R >= 1): every round also runs one split sweep, in which a
    group is cut in two from two seeds if that raises the objective (hdg_refine_split,
    hdg_refine_split_ladder);
    --link-match: --Type untangle also reports how many hunks are in the right group under the
    best one-to-one assignment of predicted to true groups (hdg_match): accuracy, purity, cover;
    --link-score acc (needs --link-threshold refined): the ladder's rung is chosen by that
    accuracy, pooled, every rung matched on the device."""
    p = argparse.ArgumentParser(add_help=False)
    p.add_argument('--model', type=int, default=2, choices=(1, 2, 3, 4))
    p.add_argument('--loader', default='utils2', choices=('utils2', 'fast'))
    p.add_argument('--link-threshold', type=_threshold, default=0.5)
    p.add_argument('--link-rule', default='mean', choices=('mean', 'any', 'both'))
    p.add_argument('--link-score', default='f1', choices=('f1', 'rand', 'acc'))
    p.add_argument('--link-method', default='single', choices=('single', 'complete', 'average'))
    p.add_argument('--link-refine', type=int, default=0)
    p.add_argument('--link-ladder', type=_ladder, default=(0.05, 0.95, 19))
    p.add_argument('--link-merge', type=int, default=0)
    p.add_argument('--link-split', action='store_true')
    p.add_argument('--link-match', action='store_true')
    a, rest = p.parse_known_args(argv)
    if a.link_score == 'acc' and a.link_threshold != 'refined':
        p.error("--link-score acc needs --link-threshold refined")
    if a.link_threshold == 'refined' and a.link_refine < 1:
        p.error("--link-threshold refined needs --link-refine N with N >= 1")
    if not 0 <= a.link_merge <= 16:
        p.error("--link-merge R needs 0 <= R <= 16")
    if a.link_merge and a.link_refine < 1:
        p.error("--link-merge needs --link-refine N with N >= 1")
    if a.link_split and a.link_merge < 1:
        p.error("--link-split needs --link-merge R with R >= 1")
    return a, rest


# the reference's per-step tables (main.py:11-15): glide steps 2, 3, 5
STEPS = [2, 3, 5]
ENTITY_NODES = [200, 250, 250]
HUNK_NODES = [74, 114, 150]
ENTITY_EDGES = [39800, 62250, 62250]
HUNK_EDGES = [5402, 12882, 22350]


def build_parser(step, entity_node, hunk_node, entity_edge, hunk_edge):
    """The reference's per-step parser (main.py:24-48): same flags, types, defaults, help."""
    parser = argparse.ArgumentParser(description='')
    parser.add_argument('--epoch', type=int, default=50, help='number of training epochs')
    parser.add_argument('--Ds', type=int, default=1, help='The State Dimention')
    parser.add_argument('--Ds_inter', type=int, default=1, help='The State Dimention of inter state')
    parser.add_argument('--Dr', type=int, default=2, help='The Relationship Dimension')
    parser.add_argument('--Dr_inter', type=int, default=2, help='The Relationship Dimension of inter state')
    parser.add_argument('--De_e', type=int, default=20, help='The Effect Dimension on entity')
    parser.add_argument('--De_er', type=int, default=20, help='The Effect Dimension on entity Relations')
    parser.add_argument('--Mini_batch', type=int, default=50, help='The training mini_batch')
    parser.add_argument('--checkpoint_dir', dest='checkpoint_dir', default='./checkpoint40/',
                        help='models are saved here')
    parser.add_argument('--Ne', type=int, default=entity_node, help='The Number of entities')
    parser.add_argument('--Nc', type=int, default=hunk_node, help='The Number of code changes')
    parser.add_argument('--Ner', type=int, default=entity_edge, help='The Number of entity Relations')
    parser.add_argument('--Ncr', type=int, default=hunk_edge, help='The Number of code change Relations')
    parser.add_argument('--Step', type=int, default=step, help='the number of commits/groups')
    parser.add_argument('--Repo', type=str, default='glide', help='the name of repository')
    parser.add_argument('--Type', dest='Type', default='train', help='train or test')
    return parser


def main(argv=None, model_cls=None):
    """model_cls: the graph2graph class to run (tests inject a recorder); default
    hdgnn.model[_N].graph2graph for --model N."""
    import importlib
    extra, argv = _variant(sys.argv[1:] if argv is None else argv)
    variant, loader = extra.model, extra.loader
    graph2graph = model_cls or importlib.import_module(
        "hdgnn.model" + ("" if variant == 2 else "_%d" % variant)).graph2graph
    if model_cls is None:
        _init_distributed()

    for step, entity_node, hunk_node, entity_edge, hunk_edge in zip(
            STEPS, ENTITY_NODES, HUNK_NODES, ENTITY_EDGES, HUNK_EDGES):
        print(step, entity_node, hunk_node, entity_edge, hunk_edge)
        args = build_parser(step, entity_node, hunk_node, entity_edge, hunk_edge).parse_args(argv)

        if not os.path.exists(args.checkpoint_dir):
            os.makedirs(args.checkpoint_dir)
        model = graph2graph(None,
                            Ds=args.Ds,
                            Ne=args.Ne, Nc=args.Nc,
                            Ner=args.Ner, Ncr=args.Ncr,
                            Dr=args.Dr,
                            De_e=args.De_e, De_er=args.De_er,
                            Mini_batch=args.Mini_batch,
                            checkpoint_dir=args.checkpoint_dir,
                            epoch=args.epoch,
                            Ds_inter=args.Ds_inter, Dr_inter=args.Dr_inter,
                            Step=args.Step,
                            Repo=args.Repo, loader=loader)
        if args.Type == 'train':
            model.train(args)
        if args.Type == 'test':
            model.test(args)
        if args.Type == 'eval':      # not in the reference: on-device scores of the trained model
            model.evaluate(args)
        # single linkage is the call as it always was; another method is passed on
        how = {} if extra.link_method == 'single' else {'method': extra.link_method}
        # the threshold calibrated for the refined groups: the best rung of the ladder
        refined = dict(rule=extra.link_rule, score=extra.link_score, refine=extra.link_refine,
                       ladder=extra.link_ladder, **how)
        # rounds with group sweeps only when asked for: without the flag every call is as it was
        rounds = {'merge': extra.link_merge} if extra.link_merge else {}
        if extra.link_split:         # split sweeps in those rounds, only when asked for
            rounds['split'] = True
        refined.update(rounds)
        if args.Type == 'untangle':  # not in the reference: hunk groups per commit, on the device
            threshold = extra.link_threshold
            if threshold == 'refined':
                threshold = model.calibrate_refined(args, part="train", **refined)[0]
            elif threshold == 'auto':
                threshold = model.calibrate(args, part="train", rule=extra.link_rule,
                                            score=extra.link_score, **how)[0]
            # without refinement the call is the one it always was
            more = {'refine': extra.link_refine} if extra.link_refine else {}
            if extra.link_match:     # the matching accuracy, only when asked for
                more['match'] = True
            model.untangle(args, threshold=threshold, rule=extra.link_rule, **how, **more,
                           **rounds)
        if args.Type == 'calibrate':  # not in the reference: the best link threshold, on the device
            if extra.link_threshold == 'refined':
                model.calibrate_refined(args, part="train", **refined)
            else:
                model.calibrate(args, part="train", rule=extra.link_rule, score=extra.link_score,
                                **how)


if __name__ == '__main__':
    main()
