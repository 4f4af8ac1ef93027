"""Rate of ``bg_colorization_main.py --mode train --image_size 768`` trained FROM FILES, with --scene_cache off and device, at
several --batch_size values, and of the same command line of another tree (the parent commit) at off, in one session on one card.

    python scripts/bg_scene_cache_rate.py --parent /path/to/a/built/checkout/of/the/parent --out profiles/bg_scene_cache_rate.txt

The dataset is written here, into a temporary directory: --scenes base scenes of 768 x 768 (flat sky and ground, a textured
foreground patch, a dark separating line) and three recoloured records each, as the reference's generator lays a training set
out -- png files, captions/train.json and a vocabulary file.  Timing follows scripts/bg_cli_batch_rate.py: every run is a
process of its own under its own time limit, a step is timed where the command line waits for the device (each progress print
reads the losses), the first ``--warm`` windows are dropped and the median, fastest and slowest window are reported.  One
further run under ``rocprofv3 --kernel-trace --stats`` gives the stage kernel's own time."""
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
SPREAD = 0.04       # box-to-box spread of the step time this project records
KERNEL = 'bg_stage_cached_u8_kernel'
VOCAB = ('<pad>', '<unk>', 'sky', 'is', 'blue', 'and', 'grass', 'green', 'ground', 'gray', 'purple', 'black', 'yellow', 'brown',
         'cyan', 'pink', 'orange', 'red')


def write_dataset(base, scenes, size=768):
    import numpy as np
    from PIL import Image
    sys.path.insert(0, ROOT)
    from sketchyscenecolorization_amd.data_processing import bg_palette as pal
    rng = np.random.RandomState(7)
    for kind in ('foreground', 'background', 'segment'):
        os.makedirs(os.path.join(base, kind, 'train'))
    os.makedirs(os.path.join(base, 'captions'))
    recs, nbytes = [], 0
    for i in range(scenes):
        name = 'scene_%03d.png' % i
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
        bg = pal.recolor(bg, seg, *pal.BASE_PAIR)
        Image.fromarray(fg, 'RGB').save(os.path.join(base, 'foreground', 'train', name))
        Image.fromarray(seg, 'L').save(os.path.join(base, 'segment', 'train', name))
        pairs = [pal.BASE_PAIR] + [pal.PAIRS[int(k)] for k in rng.choice([k for k in range(len(pal.PAIRS)) if k != 1], 3, replace=False)]
        for a, (sky, ground) in enumerate(pairs):
            bg_name = name if a == 0 else name[:-4] + '_%d.png' % a
            Image.fromarray(pal.recolor(bg, seg, sky, ground), 'RGB').save(os.path.join(base, 'background', 'train', bg_name))
            recs.append({'fg_name': name, 'bg_name': bg_name, 'color_text': pal.caption(sky, ground)})
    with open(os.path.join(base, 'captions', 'train.json'), 'w') as fp:
        json.dump(recs, fp, indent=4)
    with open(os.path.join(base, 'bg_vocab.txt'), 'w') as fp:
        fp.write('\n'.join(VOCAB) + '\n')
    for b, _, fs in os.walk(base):
        nbytes += sum(os.path.getsize(os.path.join(b, f)) for f in fs)
    return len(recs), nbytes


def worker(args):
    sys.path.insert(0, args.tree)
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
    argv = ['--mode', 'train', '--image_size', '768', '--batch_size', str(args.batch), '--max_steps', str(args.steps), '--save_freq', '0',
            '--summary_freq', '0', '--progress_freq', str(args.window), '--data_base_dir', args.data,
            '--vocab_file', os.path.join(args.data, 'bg_vocab.txt')]
    cli.main(argv + (['--scene_cache', args.cache] if args.cache != 'off' else []))       # (the parent has no such flag)
    print('WINDOWS ' + json.dumps([b - a for a, b in zip(stamps, stamps[1:])]))


def worker_cmd(tree, batch, cache, args, steps=None):
    return [sys.executable, os.path.abspath(__file__), '--worker', '--tree', tree, '--batch', str(batch), '--cache', cache,
            '--steps', str(steps or args.steps), '--window', str(args.window), '--data', args.data]


def run(tree, batch, cache, args):
    r = subprocess.run(worker_cmd(tree, batch, cache, args), stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True,
                       timeout=args.timeout)
    if r.returncode != 0:
        sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
        raise SystemExit('run failed (%s, batch %d, cache %s): exit status %d -- nothing more is started' % (tree, batch, cache, r.returncode))
    win = [json.loads(l[8:]) for l in r.stdout.splitlines() if l.startswith('WINDOWS ')][0][args.warm:]
    ms = sorted(1e3 * w / args.window for w in win)
    built = [l for l in r.stdout.splitlines() if l.startswith('scene cache:')]
    return {'batch': batch, 'cache': cache, 'windows': len(ms), 'ms': ms[len(ms) // 2], 'fast': ms[0], 'slow': ms[-1],
            'built': built[0] if built else ''}


def kernel_time(args):
    """One run at the largest batch under rocprofv3 --kernel-trace --stats (the program after --): the stage kernel's row."""
    out = tempfile.mkdtemp()
    batch = max(int(b) for b in args.batches.split(','))
    cmd = ['rocprofv3', '--kernel-trace', '--stats', '--output-format', 'csv', '-d', out, '-o', 'p', '--'] + \
        worker_cmd(ROOT, batch, 'device', args, steps=3 * args.window)
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True, timeout=args.timeout)
    if r.returncode != 0:       # the last run of the session: the timings above are reported all the same
        sys.stderr.write(r.stdout[-4000:])
        return batch, 'the profiled run failed: exit status %d' % r.returncode
    for path in glob.glob(os.path.join(out, '**', '*kernel_stats.csv'), recursive=True):
        with open(path) as fp:
            for row in csv.DictReader(fp):
                if KERNEL in row.get('Name', ''):
                    return batch, {k: row[k] for k in ('Calls', 'AverageNs', 'MinNs', 'MaxNs', 'Percentage') if k in row}
    return batch, None


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--parent', default='', help='a built checkout of the parent commit (timed at --scene_cache off beside this tree)')
    ap.add_argument('--batches', default='1,2,4')
    ap.add_argument('--scenes', type=int, default=16, help='base scenes of the dataset (4 records each)')
    ap.add_argument('--steps', type=int, default=200)
    ap.add_argument('--window', type=int, default=20)
    ap.add_argument('--warm', type=int, default=3)
    ap.add_argument('--timeout', type=int, default=420)
    ap.add_argument('--no-profile', action='store_true')
    ap.add_argument('--out', default='')
    ap.add_argument('--worker', action='store_true')
    ap.add_argument('--tree', default=ROOT)
    ap.add_argument('--batch', type=int, default=1)
    ap.add_argument('--cache', default='off')
    ap.add_argument('--data', default='')
    args = ap.parse_args()
    if args.worker:
        return worker(args)
    args.data = os.path.join(tempfile.mkdtemp(), 'data')
    t0 = time.time()
    nrec, nbytes = write_dataset(args.data, args.scenes)
    lines = ['bg_colorization_main.py --mode train --image_size 768 from files: %d base scenes, %d records (%d png files, %.1f MB on disk, '
             'written in %.1f s); %d steps a run, windows of %d steps, first %d windows dropped; %d CPUs'
             % (args.scenes, nrec, 2 * args.scenes + nrec, nbytes / 1e6, time.time() - t0, args.steps, args.window, args.warm,
                len(os.sched_getaffinity(0)))]
    plan = []
    for b in (int(b) for b in args.batches.split(',')):
        if args.parent:
            plan.append(('parent', os.path.abspath(args.parent), b, 'off'))
        plan += [('this', ROOT, b, 'off'), ('this', ROOT, b, 'device')]
    rows = []
    for name, tree, batch, cache in plan:
        r = dict(run(tree, batch, cache, args), tree=name)
        r['images_s'] = 1e3 * batch / r['ms']
        rows.append(r)
        print(json.dumps(r), flush=True)
    lines.append('tree    cache   batch  ms/step (median  fastest  slowest window)  images/s')
    for r in rows:
        lines.append('%-7s %-7s %5d  %15.2f %8.2f %8.2f  %16.1f' % (r['tree'], r['cache'], r['batch'], r['ms'], r['fast'], r['slow'], r['images_s']))
    lines += sorted({r['built'] for r in rows if r['built']})
    get = lambda name, cache, b: [r['ms'] for r in rows if (r['tree'], r['cache'], r['batch']) == (name, cache, b)]      # noqa: E731
    for b in (int(b) for b in args.batches.split(',')):
        off, dev = get('this', 'off', b)[0], get('this', 'device', b)[0]
        lines.append('batch %d: device %.2f ms against off %.2f ms (%+.1f %%): %s' % (
            b, dev, off, 100 * (dev / off - 1), 'device SLOWER than off by more than' if dev > off * (1 + SPREAD) else 'device not slower than off beyond')
            + ' the %d %% box-to-box spread' % round(100 * SPREAD))
        for old in get('parent', 'off', b):
            lines.append('batch %d, off: this tree %.2f ms against the parent %.2f ms (%+.1f %%)' % (b, off, old, 100 * (off / old - 1)))
    if not args.no_profile:
        batch, row = kernel_time(args)
        lines.append('%s at batch %d under rocprofv3 --kernel-trace --stats: %s' % (KERNEL, batch, (row if isinstance(row, str) else json.dumps(row)) if row else 'no row found'))
    shutil.rmtree(os.path.dirname(args.data), ignore_errors=True)
    text = '\n'.join(lines) + '\n'
    print(text)
    if args.out:
        with open(args.out, 'w') as fp:
            fp.write(text)


if __name__ == '__main__':
    main()
