"""What --val_freq costs: ``obj_colorization_main.py --mode train -bt Pix2Pix -bs 32`` at 192 x 192 from 192 training records
with -vf 0, this tree and another tree (the parent commit) side by side, each twice in turn; the seconds of a held-out pass over
64 records; and the new kernel against the route it replaces on the same tensors.

    python scripts/train_validation_rate.py --parent /path/to/a/built/checkout/of/the/parent --out profiles/train_validation.txt

The datasets are synthetic content in the reference's record format (scripts/fg_record_cache_rate.py), written into a temporary
directory.  Every run is a process of its own under its own time limit and reports the command line's own "Average time" per
window of 100 iterations; the first window (start-up, graph capture) is shown and left out of the mean.  A run that fails ends
the session: nothing more is started.  ``--kernels``: one batch scored --reps times by hip.image_metrics_f32 and by
image_postprocess_u8 x 2 + image_metrics_u8, timed with events around each loop."""
import argparse
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def write_dataset(base, mode, n, seed):
    import numpy as np
    sys.path.insert(0, ROOT)
    from sketchyscenecolorization_amd import tfrecord as tf
    d = os.path.join(base, 'data', 'tfrecord', mode)
    os.makedirs(d)
    rng = np.random.RandomState(seed)
    for f in range(4):
        recs = []
        for i in range(n // 4):
            sk = np.full((384, 384, 3), 255, np.uint8)
            sk[(7 * i) % 370:(7 * i) % 370 + 6, 40:340] = 0
            text = np.zeros(15, np.uint8)
            text[11:] = rng.randint(2, 58, 4)
            recs.append(tf.make_example({'ImageName': ('%s%d_%d.png' % (mode, f, i)).encode(),
                                         'cartoon_data': rng.randint(0, 256, (384, 384, 3)).astype(np.uint8).tobytes(),
                                         'sketch_data': sk.tobytes(), 'Category': (b'car', b'tree', b'sun')[i % 3], 'Category_id': i % 25,
                                         'Color_text': b'the car is red', 'Text_vocab_indices': text.tobytes()}))
        tf.write_records(os.path.join(d, '%d.tfrecord' % f), recs)
    return d


def cli_cmd(tree, args, iters, extra=()):
    return [sys.executable, os.path.join(tree, 'obj_colorization_main.py'), '--mode', 'train', '-bt', 'Pix2Pix', '-si', '0', '-bs', str(args.batch),
            '-mi', str(iters), '-smf', '100000', '-swf', '100', '-clt', '100'] + list(extra)


def run(tree, cwd, args, iters, extra=()):
    before = set(os.listdir(os.path.join(cwd, 'outputs'))) if os.path.isdir(os.path.join(cwd, 'outputs')) else set()
    r = subprocess.run(cli_cmd(tree, args, iters, extra), cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       universal_newlines=True, timeout=args.timeout)
    if r.returncode != 0:
        sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
        raise SystemExit('run failed (%s, %s): exit status %d -- nothing more is started' % (tree, ' '.join(extra), r.returncode))
    ms = [1e3 * float(l.split('Average time: ')[1].split('s/iter')[0]) for l in r.stdout.splitlines() if 'Average time' in l and 'inf' not in l]
    new = sorted(set(os.listdir(os.path.join(cwd, 'outputs'))) - before)
    return ms, r.stdout, (os.path.join(cwd, 'outputs', new[0]) if new else None)


def kernels_worker(args):
    sys.path.insert(0, ROOT)
    import torch
    from sketchyscenecolorization_amd import hip
    n, s = args.batch, 192
    g = torch.Generator(device='cuda')
    g.manual_seed(1)
    a = torch.rand((n, s, s, 4), device='cuda', generator=g) * 2 - 1            # the generator's output buffer
    b = torch.rand((n, 3, s, s), device='cuda', generator=g) * 2 - 1            # a decoded target
    b4 = torch.zeros((n, s, s, 4), device='cuda')
    hip.nchw_to_nhwc(b, b4, 0)
    out = torch.empty((n, 5), dtype=torch.float64, device='cuda')
    ua, ub = hip.image_postprocess_u8(a, 0), hip.image_postprocess_u8(b4, 0)

    def timed(fn):
        for _ in range(3):
            fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.reps):
            fn()
        e1.record()
        e1.synchronize()
        return 1e3 * e0.elapsed_time(e1) / args.reps

    def composed():
        hip.image_postprocess_u8(a, 0, out=ua)
        hip.image_postprocess_u8(b4, 0, out=ub)
        hip.image_metrics_u8(ua, ub, out=out)

    t_new = timed(lambda: hip.image_metrics_f32(a, 0, b, out=out))
    t_nhwc = timed(lambda: hip.image_metrics_f32(a, 0, b4, 0, out=out))
    t_old = timed(composed)
    t_u8 = timed(lambda: hip.image_metrics_u8(ua, ub, out=out))
    same = torch.equal(hip.image_metrics_f32(a, 0, b), hip.image_metrics_u8(ua, ub))
    print('kernels: batch %d at %d x %d, %d calls each (events around the loop, launches back to back): image_metrics_f32 planar target '
          '%.1f us, NHWC target %.1f us; image_postprocess_u8 x 2 + image_metrics_u8 %.1f us (image_metrics_u8 alone %.1f us); rows %s'
          % (n, s, s, args.reps, t_new, t_nhwc, t_old, t_u8, 'equal' if same else 'DIFFERENT'))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--parent', default='', help='a built checkout of the parent commit (timed beside this tree)')
    ap.add_argument('--records', type=int, default=192)
    ap.add_argument('--val-records', type=int, default=64)
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--iters', type=int, default=400)
    ap.add_argument('--repeats', type=int, default=2)
    ap.add_argument('--timeout', type=int, default=300)
    ap.add_argument('--out', default='')
    ap.add_argument('--kernels', action='store_true')
    ap.add_argument('--reps', type=int, default=50)
    args = ap.parse_args()
    if args.kernels:
        return kernels_worker(args)
    base = tempfile.mkdtemp()
    t0 = time.time()
    write_dataset(base, 'train', args.records, 0)
    write_dataset(base, 'val', args.val_records, 1)
    lines = ['obj_colorization_main.py --mode train -bt Pix2Pix -si 0 -bs %d -mi %d: %d training and %d held-out records in 4 files each, '
             'written in %.1f s; ms per iteration of each window of 100 as the command line prints it (first window: start-up, not in '
             'the mean); %d CPUs' % (args.batch, args.iters, args.records, args.val_records, time.time() - t0, len(os.sched_getaffinity(0)))]
    plan = ([('parent', os.path.abspath(args.parent), ())] if args.parent else []) + [('-vf 0', ROOT, ('-vf', '0'))]
    res = {name: [] for name, _, _ in plan}
    for rep in range(args.repeats):
        for name, tree, extra in plan:
            ms, _, _ = run(tree, base, args, args.iters, extra)
            res[name].append(sum(ms[1:]) / max(1, len(ms[1:])))
            lines.append('[%-7s run %d] %s  -> %.2f' % (name, rep + 1, ' '.join('%.2f' % m for m in ms), res[name][-1]))
            print(lines[-1], flush=True)
    mean = {k: sum(v) / len(v) for k, v in res.items()}
    spread = {k: max(v) - min(v) for k, v in res.items()}
    lines.append('mean of the runs (run-to-run spread): ' + ', '.join('%s %.2f (%.2f)' % (k, mean[k], spread[k]) for k in res))
    if args.parent:
        d = mean['-vf 0'] - mean['parent']
        lines.append('-vf 0 %.2f ms against the parent %.2f ms: %+.2f ms (%+.1f %%), %s the parent\'s run-to-run spread of %.2f ms'
                     % (mean['-vf 0'], mean['parent'], d, 100 * d / mean['parent'],
                        'inside' if abs(d) <= spread['parent'] else ('OUTSIDE (slower than)' if d > 0 else 'outside (faster than)'), spread['parent']))
    # the held-out passes: -vf 100 over the same iterations, from the training cache and from the host queue
    for extra in (('-vf', '100', '-rc', 'device'), ('-vf', '100')):
        ms, out, run_dir = run(ROOT, base, args, args.iters, extra)
        with open(os.path.join(run_dir, 'log', 'validation.jsonl')) as fp:
            passes = [json.loads(l) for l in fp]
        lines.append('[%s] %s; held-out passes of %d images (%d batches) at steps %s: %s s (the first two run eagerly and capture the '
                     'inference graphs); last line: mae %.3f psnr %.3f ssim %.5f'
                     % (' '.join(extra), ' '.join('%.2f' % m for m in ms), passes[-1]['images'], -(-passes[-1]['images'] // args.batch),
                        [p['step'] for p in passes], ' '.join('%.3f' % p['seconds'] for p in passes), passes[-1]['all']['mae'],
                        passes[-1]['all']['psnr'], passes[-1]['all']['ssim']))
        lines += [l for l in out.splitlines() if l.startswith('held-out cache:')]
        print(lines[-2], flush=True)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), '--kernels', '--batch', str(args.batch), '--reps', str(args.reps)],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True, timeout=args.timeout)
    if r.returncode != 0:
        sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
        raise SystemExit('the kernel timing failed: exit status %d' % r.returncode)
    lines += [l for l in r.stdout.splitlines() if l.startswith('kernels:')]
    shutil.rmtree(base, ignore_errors=True)
    text = '\n'.join(lines) + '\n'
    print(text)
    if args.out:
        with open(args.out, 'w') as fp:
            fp.write(text)


if __name__ == '__main__':
    main()
