"""Rate of ``bg_colorization_main.py --mode train --image_size 768`` on synthetic scenes at several --batch_size values, and of
the same command line of another tree (the parent commit) at batch 1, in one session on one card.

    python scripts/bg_cli_batch_rate.py --parent /path/to/a/built/checkout/of/the/parent --out profiles/bg_cli_batch_rate.txt

Every run is a process of its own.  A step is timed where the command line itself waits for the device: each progress print
reads the losses (BGTrainer.loss_values), so the wall clock between two prints is ``--window`` whole steps, host work included.
The first ``--warm`` windows (allocation, graph capture, first launches) are dropped; reported are the median, the fastest and
the slowest window per run.  Runs of the two trees alternate (parent, this tree, parent, this tree) so that a drift of the box
shows as a spread within a tree, not as a difference between them."""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPREAD = 0.04       # box-to-box spread of the step time this project records (12.20-13.26 ms on six boxes)


def worker(tree, batch, steps, window):
    sys.path.insert(0, tree)
    os.chdir(tempfile.mkdtemp())
    import bg_colorization_main as cli
    from sketchyscenecolorization_amd import bg_colorization
    stamps = []
    real = bg_colorization.BGTrainer.loss_values

    def stamped(self):
        v = real(self)          # reads the device: every step issued so far has run
        stamps.append(time.time())
        return v

    bg_colorization.BGTrainer.loss_values = stamped
    cli.main(['--mode', 'train', '--image_size', '768', '--batch_size', str(batch), '--max_steps', str(steps), '--save_freq', '0',
              '--summary_freq', '0', '--progress_freq', str(window)])
    print('WINDOWS ' + json.dumps([b - a for a, b in zip(stamps, stamps[1:])]))


def run(tree, batch, args):
    cmd = [sys.executable, os.path.abspath(__file__), '--worker', '--tree', tree, '--batch', str(batch), '--steps', str(args.steps),
           '--window', str(args.window)]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True, timeout=args.timeout)
    if r.returncode != 0:
        sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
        raise SystemExit('run failed (%s, batch %d): exit status %d -- nothing more is started' % (tree, batch, r.returncode))
    win = [json.loads(l[8:]) for l in r.stdout.splitlines() if l.startswith('WINDOWS ')][0][args.warm:]
    ms = sorted(1e3 * w / args.window for w in win)
    return {'batch': batch, 'windows': len(ms), 'ms': ms[len(ms) // 2], 'fast': ms[0], 'slow': ms[-1]}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--parent', default='', help='a built checkout of the parent commit (its batch 1 is timed beside this tree)')
    ap.add_argument('--batches', default='1,2,4')
    ap.add_argument('--steps', type=int, default=320)
    ap.add_argument('--window', type=int, default=20)
    ap.add_argument('--warm', type=int, default=3)
    ap.add_argument('--timeout', type=int, default=420)
    ap.add_argument('--out', default='')
    ap.add_argument('--worker', action='store_true')
    ap.add_argument('--tree', default=ROOT)
    ap.add_argument('--batch', type=int, default=1)
    args = ap.parse_args()
    if args.worker:
        return worker(args.tree, args.batch, args.steps, args.window)
    rows = []
    plan = [('this', ROOT, int(b)) for b in args.batches.split(',')]
    if args.parent:
        parent = os.path.abspath(args.parent)
        plan = [('parent', parent, 1), ('this', ROOT, 1), ('parent', parent, 1)] + plan
    for name, tree, batch in plan:
        r = dict(run(tree, batch, args), tree=name)
        r['images_s'] = 1e3 * batch / r['ms']
        rows.append(r)
        print(json.dumps(r), flush=True)
    lines = ['bg_colorization_main.py --mode train --image_size 768, synthetic scenes, %d steps a run, windows of %d steps, first %d '
             'windows dropped' % (args.steps, args.window, args.warm),
             'tree    batch  ms/step (median  fastest  slowest window)  images/s']
    for r in rows:
        lines.append('%-7s %5d  %15.2f %8.2f %8.2f  %16.1f' % (r['tree'], r['batch'], r['ms'], r['fast'], r['slow'], r['images_s']))
    best = lambda name, b: min([r['ms'] for r in rows if r['tree'] == name and r['batch'] == b] or [None])      # noqa: E731
    if args.parent:
        new, old = best('this', 1), best('parent', 1)
        lines.append('batch 1, this tree against the parent: %.2f ms against %.2f ms (%+.1f %%): %s'
                     % (new, old, 100 * (new / old - 1), 'within' if new <= old * (1 + SPREAD) else 'SLOWER than'
                        ) + ' the %d %% box-to-box spread' % round(100 * SPREAD))
    if best('this', 1) and best('this', 4):
        r1, r4 = 1e3 / best('this', 1), 4e3 / best('this', 4)
        lines.append('images/s at batch 4 against batch 1: %.1f against %.1f: %s' % (r4, r1, 'not below' if r4 >= r1 else 'BELOW'))
    text = '\n'.join(lines) + '\n'
    print(text)
    if args.out:
        with open(args.out, 'w') as fp:
            fp.write(text)


if __name__ == '__main__':
    main()
