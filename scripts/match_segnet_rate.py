"""What the matcher's two backbones (match_main.py --weights deeplab | segnet; DESIGN.md sections 8.6 and 8.12) cost at 768 x 768,
on this tree and on another one (the parent commit), in one session on one card:

  * the two backbones' forward passes (MatchModel.backbone) between device events, a process per tree, --repeats times in turn;
  * ssc_max_pool2_argmax at the five pool sizes and ssc_unpool2 at the two unpool sizes of SegNet's pass, between device events,
    with the bytes each moves (this tree's first process only);
  * one iteration of ``match_main.py --mode train`` with --scene_cache device and features, --weights deeplab and --weights segnet,
    of this tree and of the other one -- every configuration --repeats times, in turn;
  * scripts/match_forward_digest.py on this tree against the other tree: the lines must be equal.

    python scripts/match_segnet_rate.py --parent /path/to/a/built/checkout/of/the/parent --out profiles/match_backbones.txt

The synthetic scenes, the random backbones, the processes under their own time limits and the windows are those of
scripts/match_cache_rate.py.  A run that fails ends the session: nothing more is started.  The bar for every figure is the
parent's figure for the same configuration within the session's run-to-run spread."""
import argparse
import os
import re
import shutil
import subprocess
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import match_cache_rate as base_rate       # noqa: E402

ROOT = base_rate.ROOT
POOLS = [(768, 64), (384, 128), (192, 256), (96, 512), (48, 512)]       # (side, channels) of what enc_1 .. enc_5 pool
UNPOOLS = [(24, 512), (48, 512)]                                       # (side, channels) of what dec_5 and dec_4 unpool


def _timed(fn, reps, warm=3):
    """-> ms per call between two device events, after ``warm`` calls."""
    import torch
    for _ in range(warm):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def worker(args):
    """One process: the two backbones' forward passes of the tree --tree and, with --kernels, the two kernels at the sizes of
    SegNet's pass."""
    sys.path.insert(0, os.path.abspath(args.tree))
    import numpy as np
    import torch
    from sketchyscenecolorization_amd import hip, matching
    sk = np.full((768, 768, 3), 255, np.uint8)
    sk[np.random.RandomState(0).rand(768, 768) < 0.1] = 0
    for backbone in ('segnet', 'deeplab'):
        cfg = matching.MatchConfig(backbone=backbone)
        model = matching.MatchModel(cfg)
        model.init_random(1)
        x4, _stroke = hip.match_preprocess_u8(model.put_sketch(sk), out=model._buf('x4', (1, 768, 768, 4)))
        ms = [_timed(lambda: model.backbone(x4), args.reps) for _ in range(3)]
        print('%s backbone forward at 768 x 768, random weights: %s ms per pass (three windows of %d passes between two device events)'
              % (backbone, ' '.join('%.3f' % m for m in ms), args.reps))
        model.close()
        del model
        torch.cuda.empty_cache()
    if not args.kernels:
        return
    print('the two kernels at the sizes of that pass, %d calls between two device events on the same buffers (repeated calls find '
          'much of a tensor in the last-level cache, so the rates are not those of the memory; the small sizes are bounded by the '
          'launch):' % (10 * args.reps))
    for side, c in POOLS:
        x = torch.randn(1, side, side, c, device='cuda')
        ab = torch.cat([torch.rand(c, device='cuda') + 0.5, torch.randn(c, device='cuda')])
        out = torch.empty(1, side // 2, side // 2, c, device='cuda')
        code = torch.empty(1, side // 2, side // 2, c, dtype=torch.uint8, device='cuda')
        ms = _timed(lambda: hip.max_pool2_argmax(x, ab, out=out, code=code), 10 * args.reps)
        nbytes = x.numel() * 4 + out.numel() * 5
        print('ssc_max_pool2_argmax %4d x %4d x %3d: %8.1f us, %6.1f MB read and written, %7.1f GB/s'
              % (side, side, c, 1e3 * ms, nbytes / 1e6, nbytes / ms / 1e6))
    for side, c in UNPOOLS:
        x = torch.randn(1, side, side, c, device='cuda')
        code = torch.randint(0, 4, (1, side, side, c), dtype=torch.uint8, device='cuda')
        out = torch.empty(1, 2 * side, 2 * side, c, device='cuda')
        ms = _timed(lambda: hip.unpool2(x, code, out=out), 10 * args.reps)
        nbytes = x.numel() * 5 + out.numel() * 4
        print('ssc_unpool2          %4d x %4d x %3d: %8.1f us, %6.1f MB read and written, %7.1f GB/s'
              % (side, side, c, 1e3 * ms, nbytes / 1e6, nbytes / ms / 1e6))


def digests(tree, timeout):
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'scripts', 'match_forward_digest.py'), '--tree', tree, '--tag', 'x'],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True, timeout=timeout, cwd=tree)
    if r.returncode != 0:
        sys.stderr.write(r.stderr[-4000:])
        raise SystemExit('match_forward_digest.py failed on %s: exit status %d -- nothing more is started' % (tree, r.returncode))
    return [line.split(' ', 3)[2:] for line in r.stdout.strip().split('\n') if line.startswith('x sha256 ')]


def forwards(tree, args, kernels):
    """The worker on ``tree`` in a process of its own -> ({backbone: mean ms of its three windows}, the lines it printed)."""
    r = subprocess.run([sys.executable, os.path.abspath(__file__), '--worker', '--reps', str(args.reps), '--tree', tree] +
                       (['--kernels'] if kernels else []), stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True,
                       timeout=args.timeout)
    if r.returncode != 0:
        sys.stderr.write(r.stderr[-4000:])
        raise SystemExit('the worker failed on %s: exit status %d -- nothing more is started' % (tree, r.returncode))
    said, ms = r.stdout.strip().split('\n'), {}
    for line in said:
        m = re.match(r'(\w+) backbone forward .*?: ([0-9. ]+) ms per pass', line)
        if m:
            w = [float(v) for v in m.group(2).split()]
            ms[m.group(1)] = sum(w) / len(w)
    return ms, said


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--parent', default='', help='a built checkout of the parent commit (timed and digested beside this tree)')
    ap.add_argument('--scenes', type=int, default=16)
    ap.add_argument('--captions', type=int, default=4)
    ap.add_argument('--iters', type=int, default=201)
    ap.add_argument('--window', type=int, default=50)
    ap.add_argument('--repeats', type=int, default=4, help='runs per configuration; the spread of two runs alone came out at 0.01 ms '
                                                           'once and called a 0.02 ms difference slower')
    ap.add_argument('--timeout', type=int, default=240)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--out', default='')
    ap.add_argument('--worker', action='store_true')
    ap.add_argument('--tree', default=ROOT, help='worker: the tree whose package it imports')
    ap.add_argument('--kernels', action='store_true', help='worker: the two kernels as well')
    args = ap.parse_args()
    if args.worker:
        return worker(args)
    trees = [('tree', ROOT)] + ([('parent', os.path.abspath(args.parent))] if args.parent else [])
    lines, res = [], {}
    for rep in range(args.repeats):
        for who, tree in trees:
            ms, said = forwards(tree, args, kernels=rep == 0 and tree == ROOT)
            for backbone, v in ms.items():
                res.setdefault('%s %s forward' % (who, backbone), []).append(v)
            lines += ['[%-6s run %d] %s' % (who, rep + 1, s) for s in said]
            print('\n'.join(lines[-len(said):]), flush=True)
    base = tempfile.mkdtemp()
    t0 = time.time()
    base_rate.write_data(base, args.scenes, args.captions)
    sys.path.insert(0, ROOT)
    from sketchyscenecolorization_amd import matching, tf_checkpoint
    segnet = os.path.join(base, 'segnet-1')
    tf_checkpoint.write_checkpoint(segnet, {k: a for k, a in matching.random_variables(matching.MatchConfig(backbone='segnet'), 1).items()
                                            if k.startswith('SegNet/')})
    lines.append('match_main.py --mode train at 768 x 768, %d iterations: %d synthetic scenes (png + mat) with %d captions each and random '
                 'backbones, written in %.1f s; ms per iteration of each window of %d (first window: start-up, not in the mean); %d CPUs'
                 % (args.iters, args.scenes, args.captions, time.time() - t0, args.window, len(os.sched_getaffinity(0))))
    seg = ['--weights', 'segnet', '--backbone_snapshot', segnet]
    plan = []
    for cache in ('device', 'features'):
        for who, tree in trees:
            plan.append(('%s deeplab %s' % (who, cache), tree, ['--scene_cache', cache, '--weights', 'deeplab']))
            plan.append(('%s segnet %s' % (who, cache), tree, ['--scene_cache', cache] + seg))
    res.update({name: [] for name, _, _ in plan})
    for rep in range(args.repeats):
        for name, tree, extra in plan:
            ms, said = base_rate.run(tree, base, '%s_%d' % (name.replace(' ', '_'), rep), args, extra)
            res[name].append(sum(ms[1:]) / max(1, len(ms[1:])))
            lines.append('[%-22s run %d] %s  -> %.2f' % (name, rep + 1, ' '.join('%.2f' % m for m in ms), res[name][-1]))
            if rep == 0:
                lines += ['[%-22s run 1] %s' % (name, s) for s in said if s.startswith('scene cache:')]
            print(lines[-1], flush=True)
    mean = {k: sum(v) / len(v) for k, v in res.items()}
    spread = {k: max(v) - min(v) for k, v in res.items()}
    lines.append('mean of the runs (run-to-run spread), ms: ' + ', '.join('%s %.3f (%.3f)' % (k, mean[k], spread[k]) for k in res))
    if args.parent:
        for what in [k[len('tree '):] for k in res if k.startswith('tree ')]:
            a, b = 'tree ' + what, 'parent ' + what
            sp, d = max(spread[a], spread[b]), mean[a] - mean[b]
            lines.append('%s: this tree %.3f ms against the parent %.3f ms: %+.3f ms (%+.1f %%), %s the run-to-run spread of %.3f ms'
                         % (what, mean[a], mean[b], d, 100 * d / mean[b], 'not slower beyond' if d <= sp else 'SLOWER by more than', sp))
    shutil.rmtree(base, ignore_errors=True)
    if args.parent:
        here, there = digests(ROOT, args.timeout), digests(os.path.abspath(args.parent), args.timeout)
        differ = [what for (sha, what), (sha2, what2) in zip(here, there) if (sha, what) != (sha2, what2)]
        lines.append('scripts/match_forward_digest.py (--weights deeplab: inference, both trainers, snapshots, launch names) on this tree '
                     'and on the parent: %d and %d lines, %s' % (len(here), len(there), 'all equal' if not differ and len(here) == len(there)
                                                                 else 'DIFFERENT: ' + '; '.join(differ[:8])))
    text = '\n'.join(lines) + '\n'
    print(text)
    if args.out:
        with open(args.out, 'w') as fp:
            fp.write(text)


if __name__ == '__main__':
    main()
