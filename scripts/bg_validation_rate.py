"""What ``bg_colorization_main.py --val_freq`` costs at 768 x 768, trained from files: ms per step of the steps that take no
held-out pass, with --val_freq 0 and with passes, beside the --val_freq 0 run of another tree (the parent commit), each run twice
in turn; the seconds of a pass; and the two kernels of a pass under rocprofv3.

    python scripts/bg_validation_rate.py --parent /path/to/a/built/checkout/of/the/parent --out profiles/bg_validation.txt

The datasets are written here, into a temporary directory: flat-coloured 768 x 768 scenes as png files (train and val), their
captions and a vocabulary file.  Every run is a process of its own under its own time limit.  A step is timed where the command
line waits for the device (each progress print reads the losses); a window of ``--window`` steps that holds a pass is reported
apart from the windows that hold none, with the pass's own time (taken around bg_validation.run_pass) beside it.  The first
``--warm`` windows are dropped.  A run that fails ends the session: nothing more is started.  The last run goes under
``rocprofv3 --kernel-trace --stats`` (kernel trace only, no counters) for the rows of the two new kernels."""
import argparse
import csv
import glob
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = ('image_metrics_bg_f32_kernel', 'seg_confusion_kernel', 'image_metrics_sum_kernel', 'seg_confusion_sum_kernel')
VOCAB = ('<pad>', '<unk>', 'sky', 'is', 'blue', 'and', 'grass', 'green', 'ground', 'gray', 'purple', 'black', 'yellow', 'brown',
         'cyan', 'pink', 'orange', 'red')


def write_dataset(base, mode, scenes, seed, size=768):
    import numpy as np
    from PIL import Image
    sys.path.insert(0, ROOT)
    from sketchyscenecolorization_amd.data_processing import bg_palette as pal
    rng = np.random.RandomState(seed)
    for kind in ('foreground', 'background', 'segment'):
        os.makedirs(os.path.join(base, kind, mode))
    os.makedirs(os.path.join(base, 'captions'), exist_ok=True)
    recs = []
    for i in range(scenes):
        name = '%s_%03d.png' % (mode, i)
        horizon = size // 2 + int(rng.randint(-60, 60))
        seg = np.zeros((size, size), np.uint8)
        seg[:horizon - 2] = pal.SEG_SKY
        seg[horizon + 2:] = pal.SEG_GROUND
        y0, x0, h, w = [int(v) for v in (rng.randint(100, 300), rng.randint(50, 300), rng.randint(200, 350), rng.randint(200, 400))]
        seg[y0:y0 + h, x0:x0 + w] = 0
        fg = np.full((size, size, 3), 255, np.uint8)
        fg[y0:y0 + h, x0:x0 + w] = rng.randint(0, 256, (h, w, 3))
        bg = np.full((size, size, 3), 40, np.uint8)
        bg[y0:y0 + h, x0:x0 + w] = fg[y0:y0 + h, x0:x0 + w]
        sky, ground = pal.PAIRS[int(rng.randint(0, len(pal.PAIRS)))]
        Image.fromarray(fg, 'RGB').save(os.path.join(base, 'foreground', mode, name))
        Image.fromarray(seg, 'L').save(os.path.join(base, 'segment', mode, name))
        Image.fromarray(pal.recolor(bg, seg, sky, ground), 'RGB').save(os.path.join(base, 'background', mode, name))
        recs.append({'fg_name': name, 'bg_name': name, 'color_text': pal.caption(sky, ground)})
    with open(os.path.join(base, 'captions', mode + '.json'), 'w') as fp:
        json.dump(recs, fp, indent=4)
    with open(os.path.join(base, 'bg_vocab.txt'), 'w') as fp:
        fp.write('\n'.join(VOCAB) + '\n')


def worker(args):
    sys.path.insert(0, args.tree)
    os.chdir(tempfile.mkdtemp())
    import bg_colorization_main as cli
    from sketchyscenecolorization_amd import bg_colorization
    events, state = [], {'in_pass': False}
    real = bg_colorization.BGTrainer.loss_values

    def stamped(self):
        v = real(self)          # reads the device: every step issued so far has run
        if not state['in_pass']:
            events.append(('loss', time.time()))
        return v

    bg_colorization.BGTrainer.loss_values = stamped
    argv = ['--mode', 'train', '--image_size', '768', '--batch_size', str(args.batch), '--max_steps', str(args.steps), '--save_freq', '0',
            '--summary_freq', '0', '--progress_freq', str(args.window), '--data_base_dir', args.data,
            '--vocab_file', os.path.join(args.data, 'bg_vocab.txt')]
    if args.val_freq:           # (the parent has no such flag)
        from sketchyscenecolorization_amd import bg_validation
        real_pass = bg_validation.run_pass

        def timed_pass(*a, **k):
            state['in_pass'] = True
            t0 = time.time()
            line = real_pass(*a, **k)
            events.append(('pass', t0, time.time(), line['seconds'], line['images']))
            state['in_pass'] = False
            return line

        bg_validation.run_pass = timed_pass
        argv += ['--val_freq', str(args.val_freq)]
    cli.main(argv)
    print('EVENTS ' + json.dumps(events))


def worker_cmd(tree, val_freq, args, steps=None):
    return [sys.executable, os.path.abspath(__file__), '--worker', '--tree', tree, '--batch', str(args.batch), '--val-freq', str(val_freq),
            '--steps', str(steps or args.steps), '--window', str(args.window), '--data', args.data]


def windows(events, args):
    """-> (ms per step of the windows without a pass, of the windows with one after its time is taken out, the passes)."""
    plain, holed, passes, last, inside = [], [], [], None, []
    for e in events:
        if e[0] == 'pass':
            inside.append(e)
            passes.append({'wall': e[2] - e[1], 'seconds': e[3], 'images': e[4]})
            continue
        if last is not None:
            ms = 1e3 * (e[1] - last - sum(p[2] - p[1] for p in inside)) / args.window
            (holed if inside else plain).append(ms)
        last, inside = e[1], []
    return plain[args.warm:], holed, passes


def run(tree, val_freq, args):
    r = subprocess.run(worker_cmd(tree, val_freq, args), stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True,
                       timeout=args.timeout)
    if r.returncode != 0:
        sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
        raise SystemExit('run failed (%s, --val_freq %d): exit status %d -- nothing more is started' % (tree, val_freq, r.returncode))
    events = [json.loads(l[7:]) for l in r.stdout.splitlines() if l.startswith('EVENTS ')][0]
    plain, holed, passes = windows(events, args)
    ms = sorted(plain)
    return {'ms': ms[len(ms) // 2], 'fast': ms[0], 'slow': ms[-1], 'windows': len(ms), 'holed': holed, 'passes': passes,
            'cache': [l for l in r.stdout.splitlines() if l.startswith('held-out cache:')]}


def kernel_rows(args):
    out = tempfile.mkdtemp()
    cmd = ['rocprofv3', '--kernel-trace', '--stats', '--output-format', 'csv', '-d', out, '-o', 'p', '--'] + \
        worker_cmd(ROOT, args.window, args, steps=3 * args.window)
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True, timeout=args.timeout)
    if r.returncode != 0:       # the last run of the session: the timings above are reported all the same
        sys.stderr.write(r.stdout[-4000:])
        return ['the profiled run failed: exit status %d' % r.returncode]
    rows = []
    for path in glob.glob(os.path.join(out, '**', '*kernel_stats.csv'), recursive=True):
        with open(path) as fp:
            for row in csv.DictReader(fp):
                if any(k in row.get('Name', '') for k in KERNELS):
                    rows.append('%s: %s' % (row['Name'].split('(')[0], json.dumps({k: row[k] for k in ('Calls', 'AverageNs', 'MinNs', 'MaxNs', 'Percentage') if k in row})))
    shutil.rmtree(out, ignore_errors=True)
    return rows or ['no row of the two kernels found']


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--parent', default='', help='a built checkout of the parent commit (timed at --val_freq 0 beside this tree)')
    ap.add_argument('--scenes', type=int, default=16)
    ap.add_argument('--val-scenes', type=int, default=8)
    ap.add_argument('--steps', type=int, default=240)
    ap.add_argument('--window', type=int, default=20)
    ap.add_argument('--warm', type=int, default=3)
    ap.add_argument('--passes-every', type=int, default=3, help='--val_freq of the run with passes, in windows')
    ap.add_argument('--repeats', type=int, default=2)
    ap.add_argument('--timeout', type=int, default=420)
    ap.add_argument('--no-profile', action='store_true')
    ap.add_argument('--out', default='')
    ap.add_argument('--worker', action='store_true')
    ap.add_argument('--tree', default=ROOT)
    ap.add_argument('--batch', type=int, default=1)
    ap.add_argument('--val-freq', type=int, default=0)
    ap.add_argument('--data', default='')
    args = ap.parse_args()
    if args.worker:
        return worker(args)
    args.data = os.path.join(tempfile.mkdtemp(), 'data')
    t0 = time.time()
    write_dataset(args.data, 'train', args.scenes, 7)
    write_dataset(args.data, 'val', args.val_scenes, 8)
    vf = args.passes_every * args.window
    lines = ['bg_colorization_main.py --mode train --image_size 768 --batch_size %d from files: %d train and %d val scenes (written in %.1f s); '
             '%d steps a run, windows of %d steps, first %d windows dropped; median (fastest, slowest) window in ms per step; %d CPUs'
             % (args.batch, args.scenes, args.val_scenes, time.time() - t0, args.steps, args.window, args.warm, len(os.sched_getaffinity(0)))]
    plan = ([('parent', os.path.abspath(args.parent), 0)] if args.parent else []) + [('--val_freq 0', ROOT, 0), ('--val_freq %d' % vf, ROOT, vf)]
    res = {name: [] for name, _, _ in plan}
    for rep in range(args.repeats):
        for name, tree, freq in plan:
            r = run(tree, freq, args)
            res[name].append(r)
            lines.append('[%-14s run %d] steps without a pass: %.2f (%.2f, %.2f) over %d windows' % (name, rep + 1, r['ms'], r['fast'], r['slow'], r['windows'])
                         + ('; windows with a pass, its time taken out: %s; passes of %d images: %s s (wall, the line\'s own: %s)'
                            % (' '.join('%.2f' % m for m in r['holed']), r['passes'][-1]['images'], ' '.join('%.3f' % p['wall'] for p in r['passes']),
                               ' '.join('%.3f' % p['seconds'] for p in r['passes'])) if r['passes'] else ''))
            print(lines[-1], flush=True)
    mean = {k: sum(r['ms'] for r in v) / len(v) for k, v in res.items()}
    spread = {k: max(r['ms'] for r in v) - min(r['ms'] for r in v) for k, v in res.items()}
    lines.append('mean of the runs (run-to-run spread): ' + ', '.join('%s %.2f (%.2f)' % (k, mean[k], spread[k]) for k in res))
    if args.parent:
        for k in list(res)[1:]:
            d = mean[k] - mean['parent']
            lines.append('%s: steps without a pass %.2f ms against the parent %.2f ms: %+.2f ms (%+.1f %%), %s the parent\'s run-to-run spread of %.2f ms'
                         % (k, mean[k], mean['parent'], d, 100 * d / mean['parent'],
                            'inside' if abs(d) <= spread['parent'] else ('OUTSIDE (slower than)' if d > 0 else 'outside (faster than)'), spread['parent']))
    lines += sorted({l for v in res.values() for r in v for l in r['cache']})
    if not args.no_profile:
        lines.append('under rocprofv3 --kernel-trace --stats, %d steps with --val_freq %d:' % (3 * args.window, args.window))
        lines += kernel_rows(args)
    shutil.rmtree(os.path.dirname(args.data), ignore_errors=True)
    text = '\n'.join(lines) + '\n'
    print(text)
    if args.out:
        with open(args.out, 'w') as fp:
            fp.write(text)


if __name__ == '__main__':
    main()
