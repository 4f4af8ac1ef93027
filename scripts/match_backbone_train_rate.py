"""Rate of ``match_main.py --mode train --scene_cache device`` at 768 x 768 with --train_backbone 0 and 1, and of the parent
commit's command line beside --train_backbone 0 -- every configuration twice, in turn, in one session on one card -- then the
parts of one --train_backbone 1 iteration between device events.

    python scripts/match_backbone_train_rate.py --parent /path/to/a/built/checkout/of/the/parent --out profiles/match_backbone_train.txt

The data is that of scripts/match_cache_rate.py (synthetic 768 x 768 scenes written into a temporary directory, a random backbone of
the released shape), and so are the runs: processes of their own under their own time limit, ms per iteration of every window of
--window iterations, the first window left out of the mean; a run that fails ends the session.  This is a record: there is no
earlier number for a step that trains the backbone.  The one comparison is --train_backbone 0 against the parent, which must
agree within the run-to-run spread of the two."""
import argparse
import os
import shutil
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import match_cache_rate as R        # noqa: E402


def worker(args):
    """One process: --reps iterations of the trainer with an event behind every part; the mean of each part without the first
    two iterations."""
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    from sketchyscenecolorization_amd import match_backbone_train, match_train, matching
    cfg = matching.MatchConfig()
    model = matching.MatchModel(cfg)
    model.init_random(1)
    act, scratch, slots = match_backbone_train.check_budget(cfg, torch.cuda.mem_get_info()[0])
    print('kept activations %d bytes, gradient scratch %d, gradient and Adam slots %d' % (act, scratch, slots))
    trainer = match_backbone_train.BackboneMatchTrainer(model)
    trainer.reserve()
    rng = np.random.RandomState(0)
    sk = np.full((cfg.size, cfg.size, 3), 255, np.uint8)
    sk[rng.rand(cfg.size, cfg.size) < 0.1] = 0
    labels = np.zeros((cfg.size, cfg.size), np.uint8)
    labels[100:400, 80:500] = 1
    skd, labels_d = torch.from_numpy(sk).cuda(), trainer.upload_scene(labels)
    tok = torch.zeros(cfg.max_len, dtype=torch.int32, device='cuda')
    tok[:5] = torch.tensor([5, 9, 3, 7, 11], dtype=torch.int32)
    lut = torch.from_numpy(match_train.caption_lut([1])).cuda()
    order = ['forward: backbone, everything kept', 'forward: head', 'loss', 'backward: head, d feat', 'group_5', 'group_4', 'group_3',
             'group_2', 'pool and conv1', 'update: head', 'update: backbone (l2, Adam, planes)']
    total = {k: 0.0 for k in order}
    for rep in range(args.reps):
        ev = [torch.cuda.Event(enable_timing=True)]
        ev[0].record()
        names = []

        def part(name):
            e = torch.cuda.Event(enable_timing=True)
            e.record()
            ev.append(e)
            names.append(name)
        trainer.on_part = part
        feat = trainer._features(skd)
        part(order[0])
        pred = trainer.head_train(feat, tok, 5)
        part(order[1])
        dpred = trainer.loss_and_grad(pred, skd, labels_d, lut)
        part(order[2])
        dfeat = trainer._bbuf('bb/dfeat', (1, cfg.feat, cfg.feat, cfg.filters[4]))
        match_train.MatchTrainer.backward(trainer, dpred, dfeat)
        part(order[3])
        trainer.backbone_backward(dfeat)
        match_train.MatchTrainer.apply(trainer, 2.5e-4)
        part(order[9])
        trainer.step_count -= 1
        trainer.on_part = None
        trainer.apply(2.5e-4)           # the head's update once more beside the backbone's: its share is taken off below
        part('both')
        torch.cuda.synchronize()
        if rep >= 2:
            ms = {n: a.elapsed_time(b) for n, a, b in zip(names, ev[:-1], ev[1:])}
            for k in order[:-1]:
                total[k] += ms[k]
            total[order[-1]] += ms['both'] - ms[order[9]]
    n = args.reps - 2
    for k in order:
        print('%-40s %8.3f ms' % (k, total[k] / n))
    print('%-40s %8.3f ms  (mean of %d iterations between device events, one stream)' % ('sum', sum(total.values()) / n, n))
    model.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--parent', default='', help='a built checkout of the parent commit (timed beside --train_backbone 0)')
    ap.add_argument('--scenes', type=int, default=32)
    ap.add_argument('--captions', type=int, default=4)
    ap.add_argument('--iters', type=int, default=301)
    ap.add_argument('--window', type=int, default=50)
    ap.add_argument('--repeats', type=int, default=2)
    ap.add_argument('--timeout', type=int, default=240)
    ap.add_argument('--out', default='')
    ap.add_argument('--worker', action='store_true')
    ap.add_argument('--reps', type=int, default=12)
    args = ap.parse_args()
    if args.worker:
        return worker(args)
    base = tempfile.mkdtemp()
    t0 = time.time()
    R.write_data(base, args.scenes, args.captions)
    lines = ['match_main.py --mode train --scene_cache device at 768 x 768, %d iterations: %d synthetic scenes (png + mat) with %d captions '
             'each and a random backbone, written in %.1f s; ms per iteration of each window of %d (first window: start-up, not in the '
             'mean); %d CPUs' % (args.iters, args.scenes, args.captions, time.time() - t0, args.window, len(os.sched_getaffinity(0)))]
    dev = ['--scene_cache', 'device']
    plan = ([('parent', os.path.abspath(args.parent), dev)] if args.parent else []) + \
        [('backbone 0', ROOT, dev + ['--train_backbone', '0']), ('backbone 1', ROOT, dev + ['--train_backbone', '1'])]
    res = {name: [] for name, _, _ in plan}
    for rep in range(args.repeats):
        for name, tree, extra in plan:
            ms, _said = R.run(tree, base, '%s_%d' % (name.replace(' ', ''), rep), args, extra)
            res[name].append(sum(ms[1:]) / max(1, len(ms[1:])))
            lines.append('[%-10s run %d] %s  -> %.2f' % (name, rep + 1, ' '.join('%.2f' % m for m in ms), res[name][-1]))
            print(lines[-1], flush=True)
    mean = {k: sum(v) / len(v) for k, v in res.items()}
    spread = {k: max(v) - min(v) for k, v in res.items()}
    lines.append('mean of the runs (run-to-run spread): ' + ', '.join('%s %.2f (%.2f)' % (k, mean[k], spread[k]) for k in res))
    if args.parent:
        s, d = max(spread['backbone 0'], spread['parent']), mean['backbone 0'] - mean['parent']
        lines.append('--train_backbone 0 %.2f ms against the parent %.2f ms: %+.2f ms (%+.1f %%), %s the run-to-run spread of %.2f ms'
                     % (mean['backbone 0'], mean['parent'], d, 100 * d / mean['parent'], 'within' if abs(d) <= s else 'OUTSIDE', s))
    lines.append('--train_backbone 1 costs %.2f ms per iteration more than --train_backbone 0 (x %.2f)'
                 % (mean['backbone 1'] - mean['backbone 0'], mean['backbone 1'] / mean['backbone 0']))
    r = subprocess.run([sys.executable, os.path.abspath(__file__), '--worker', '--reps', str(args.reps)], cwd=base,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True, timeout=args.timeout)
    if r.returncode != 0:
        sys.stderr.write(r.stderr[-4000:])
        raise SystemExit('the worker failed: exit status %d' % r.returncode)
    lines.append('the parts of one --train_backbone 1 iteration:')
    lines += r.stdout.strip().split('\n')
    shutil.rmtree(base, ignore_errors=True)
    text = '\n'.join(lines) + '\n'
    print(text)
    if args.out:
        with open(args.out, 'w') as fp:
            fp.write(text)


if __name__ == '__main__':
    main()
