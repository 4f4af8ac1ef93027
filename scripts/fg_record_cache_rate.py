"""Rate of ``obj_colorization_main.py --mode train -bt Pix2Pix -bs 32`` at 192 x 192 trained from data/tfrecord/train with
--record_cache off and device, on the synthetic queue, and of the same command line of another tree (the parent commit) at
off -- every configuration twice, in turn, in one session on one card.

    python scripts/fg_record_cache_rate.py --parent /path/to/a/built/checkout/of/the/parent --out profiles/fg_record_cache_rate.txt

The dataset is the one of scripts/cli_train_rate_records.py (synthetic content in the reference's record format: --records
records of two 384 x 384 x 3 images in four files), written here into a temporary directory.  Every run is a process of its own
under its own time limit and reports the command line's own "Average time" per window of 100 iterations; the first window
(start-up, graph capture) is shown and left out of the mean.  A run that fails ends the session: nothing more is started.
Two further runs under ``rocprofv3 --kernel-trace --stats``: the ``-rc device`` command line (where the step's time goes), and
one batch decoded by the cache kernel and by the two launches of ssc_decode_paired_u8 (``--kernels``)."""
import argparse
import csv
import glob
import os
import shutil
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = ('decode_cached_kernel', 'decode_minmax_kernel', 'decode_write_kernel')


def write_dataset(base, n):
    import numpy as np
    sys.path.insert(0, ROOT)
    from sketchyscenecolorization_amd import tfrecord as tf
    d = os.path.join(base, 'data', 'tfrecord', 'train')
    os.makedirs(d)
    rng = np.random.RandomState(0)
    for f in range(4):
        recs = []
        for i in range(n // 4):
            sk = np.full((384, 384, 3), 255, np.uint8)
            sk[(7 * i) % 370:(7 * i) % 370 + 6, 40:340] = 0
            text = np.zeros(15, np.uint8)
            text[11:] = rng.randint(2, 58, 4)
            recs.append(tf.make_example({'ImageName': b'x.png', 'cartoon_data': rng.randint(0, 256, (384, 384, 3)).astype(np.uint8).tobytes(),
                                         'sketch_data': sk.tobytes(), 'Category': b'car', 'Category_id': i % 25,
                                         'Color_text': b'the car is red', 'Text_vocab_indices': text.tobytes()}))
        tf.write_records(os.path.join(d, '%d.tfrecord' % f), recs)
    return d


def cli_cmd(tree, args, cache, iters):
    cmd = [sys.executable, os.path.join(tree, 'obj_colorization_main.py'), '--mode', 'train', '-bt', 'Pix2Pix', '-si', '0', '-bs', str(args.batch),
           '-mi', str(iters), '-smf', '100000', '-swf', '100', '-clt', '100']
    return cmd + (['-rc', 'device'] if cache == 'device' else [])       # (the parent has no such flag)


def run(tree, cwd, cache, args):
    r = subprocess.run(cli_cmd(tree, args, cache, args.iters), cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       universal_newlines=True, timeout=args.timeout)
    if r.returncode != 0:
        sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
        raise SystemExit('run failed (%s, %s): exit status %d -- nothing more is started' % (tree, cache, r.returncode))
    ms = [1e3 * float(l.split('Average time: ')[1].split('s/iter')[0]) for l in r.stdout.splitlines() if 'Average time' in l and 'inf' not in l]
    built = [l for l in r.stdout.splitlines() if l.startswith('record cache:')]
    return ms, (built[0] if built else '')


def stats_rows(out_dir, names=None, top=0):
    rows = []
    for path in glob.glob(os.path.join(out_dir, '**', '*kernel_stats.csv'), recursive=True):
        with open(path) as fp:
            rows += list(csv.DictReader(fp))
    rows.sort(key=lambda r: -float(r.get('TotalDurationNs', 0) or 0))
    keep = [r for k, r in enumerate(rows) if k < top or (names and any(n in r.get('Name', '') for n in names))]
    return ['%10s calls  %12.1f ns avg  %6s %%  %s' % (r['Calls'], float(r['AverageNs']), r.get('Percentage', '?'), r['Name'][:110]) for r in keep]


def split_rows(out_dir, reps):
    """The cache kernel's dispatches in launch order from the kernel trace: the first ``reps`` decode the sketch, the rest do not."""
    ns = []
    for path in glob.glob(os.path.join(out_dir, '**', '*kernel_trace.csv'), recursive=True):
        with open(path) as fp:
            for r in csv.DictReader(fp):
                if 'decode_cached_kernel' in r.get('Kernel_Name', '') and 'Start_Timestamp' in r:
                    ns.append((int(r['Start_Timestamp']), int(r['End_Timestamp']) - int(r['Start_Timestamp'])))
    ns = [d for _, d in sorted(ns)]
    if len(ns) != 2 * reps:
        return ['decode_cached_kernel: %d dispatches in the kernel trace, %d expected: not split' % (len(ns), 2 * reps)]
    return ['decode_cached_kernel %-18s %10d calls  %12.1f ns avg  %d min  %d max' % (w, len(v), sum(v) / len(v), min(v), max(v))
            for w, v in (('with the sketch', ns[:reps]), ('without the sketch', ns[reps:]))]


def profiled(cmd, cwd, args, reps=0, **kw):
    out = tempfile.mkdtemp()
    r = subprocess.run(['rocprofv3', '--kernel-trace', '--stats', '--output-format', 'csv', '-d', out, '-o', 'p', '--'] + cmd, cwd=cwd,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True, timeout=args.timeout)
    if r.returncode != 0:
        sys.stderr.write(r.stdout[-4000:])
        raise SystemExit('the profiled run failed: exit status %d -- nothing more is started' % r.returncode)
    rows = stats_rows(out, **kw) + (split_rows(out, reps) if reps else [])
    shutil.rmtree(out, ignore_errors=True)
    return rows or ['no kernel_stats.csv row found']


def kernels_worker(args):
    """One batch of --batch records of the dataset, decoded ``--reps`` times by the cache kernel (sketch and no sketch) and by
    hip.decode_paired_u8 on the gathered bytes: the rows of one trace."""
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    from sketchyscenecolorization_amd import hip, record_cache as rc
    cache = rc.RecordCache(rc.list_record_files(os.path.join(args.data, 'data', 'tfrecord', 'train')), 192, device='cuda')
    numbers = np.random.RandomState(1).randint(0, len(cache), args.batch)
    idx = torch.from_numpy(numbers.astype(np.int32)).cuda()
    img, sk = cache.img[idx.long()].contiguous(), cache.sk[idx.long()].contiguous()
    noise = torch.rand((args.batch, 192, 192, 3), device='cuda') * (1.0 / 256)
    for _ in range(args.reps):
        a = hip.decode_paired_cached_u8(cache, idx, 192, noise=noise)
        b = hip.decode_paired_u8(img, sk, 192, noise=noise)
    for _ in range(args.reps):
        hip.decode_paired_cached_u8(cache, idx, 192, noise=noise, want_sketch=False)
    torch.cuda.synchronize()
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    print('kernels: %d x (cached with sketch, cached without, uncached) at batch %d, outputs equal' % (args.reps, args.batch))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--parent', default='', help='a built checkout of the parent commit (timed at off beside this tree)')
    ap.add_argument('--records', type=int, default=192)
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--iters', type=int, default=400)
    ap.add_argument('--repeats', type=int, default=2)
    ap.add_argument('--timeout', type=int, default=300)
    ap.add_argument('--no-profile', action='store_true')
    ap.add_argument('--out', default='')
    ap.add_argument('--kernels', action='store_true')
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--data', default='')
    args = ap.parse_args()
    if args.kernels:
        return kernels_worker(args)
    base, empty = tempfile.mkdtemp(), tempfile.mkdtemp()
    t0 = time.time()
    write_dataset(base, args.records)
    lines = ['obj_colorization_main.py --mode train -bt Pix2Pix -si 0 -bs %d -mi %d: %d records in 4 files, written in %.1f s; ms per '
             'iteration of each window of 100 as the command line prints it (first window: start-up, not in the mean); %d CPUs'
             % (args.batch, args.iters, args.records, time.time() - t0, len(os.sched_getaffinity(0)))]
    plan = ([('parent off', os.path.abspath(args.parent), base, 'off')] if args.parent else []) + \
        [('off', ROOT, base, 'off'), ('device', ROOT, base, 'device'), ('synthetic', ROOT, empty, 'off')]
    res, built = {name: [] for name, _, _, _ in plan}, set()
    for rep in range(args.repeats):
        for name, tree, cwd, cache in plan:
            ms, line = run(tree, cwd, cache, args)
            res[name].append(sum(ms[1:]) / max(1, len(ms[1:])))
            built |= {line} - {''}
            lines.append('[%-10s run %d] %s  -> %.2f' % (name, rep + 1, ' '.join('%.2f' % m for m in ms), res[name][-1]))
            print(lines[-1], flush=True)
    lines += sorted(built)
    mean = {k: sum(v) / len(v) for k, v in res.items()}
    spread = {k: max(v) - min(v) for k, v in res.items()}
    lines.append('mean of the runs (run-to-run spread): ' + ', '.join('%s %.2f (%.2f)' % (k, mean[k], spread[k]) for k in res))

    def compare(a, b, what):
        s = max(spread[a], spread[b])
        d = mean[a] - mean[b]
        lines.append('%s %.2f ms against %s %.2f ms: %+.2f ms (%+.1f %%), %s the run-to-run spread of %.2f ms'
                     % (a, mean[a], b, mean[b], d, 100 * d / mean[b], what[0] if d <= s else what[1], s))
    if args.parent:
        compare('off', 'parent off', ('not slower beyond', 'SLOWER by more than'))
    compare('device', 'off', ('not slower beyond', 'SLOWER by more than'))
    compare('device', 'synthetic', ('at the synthetic rate within', 'a gap beyond'))
    if not args.no_profile:
        lines.append('rocprofv3 --kernel-trace --stats of the -rc device command line (%d iterations): the ten largest rows and the decode kernels'
                     % min(args.iters, 200))
        lines += profiled(cli_cmd(ROOT, args, 'device', min(args.iters, 200)), base, args, names=KERNELS, top=10)
        lines.append('rocprofv3 --kernel-trace --stats of one batch of %d decoded %d times by the cache kernel (with and without the sketch) and by '
                     'ssc_decode_paired_u8 (decode_minmax_kernel + decode_write_kernel); decode_minmax_kernel also runs once per %d records '
                     'while the cache is built' % (args.batch, args.reps, args.batch))
        lines += profiled([sys.executable, os.path.abspath(__file__), '--kernels', '--data', base, '--batch', str(args.batch), '--reps',
                           str(args.reps)], base, args, reps=args.reps, names=KERNELS)
    shutil.rmtree(base, ignore_errors=True)
    shutil.rmtree(empty, ignore_errors=True)
    text = '\n'.join(lines) + '\n'
    print(text)
    if args.out:
        with open(args.out, 'w') as fp:
            fp.write(text)


if __name__ == '__main__':
    main()
