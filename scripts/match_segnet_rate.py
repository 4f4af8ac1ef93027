"""What the matcher's SegNet backbone (match_main.py --weights segnet) costs at 768 x 768, in one session on
one card:

  * the backbone's forward pass (MatchModel.segnet) between device events, beside the DeepLab-ResNet's (MatchModel.backbone);
  * ssc_max_pool2_argmax at the five pool sizes and ssc_unpool2 at the two unpool sizes of that pass, between device events, with
    the bytes each moves;
  * one iteration of ``match_main.py --mode train`` with --scene_cache device and features, --weights segnet and --weights deeplab,
    and the --weights deeplab command line of another tree (the parent commit, which reads no such flag in these modes) -- every
    configuration --repeats times, in turn;
  * scripts/match_forward_digest.py on this tree against the other tree: the lines must be equal.

    python scripts/match_segnet_rate.py --parent /path/to/a/built/checkout/of/the/parent --out profiles/match_segnet.txt

The synthetic scenes, the random backbones, the processes under their own time limits and the windows are those of
scripts/match_cache_rate.py.  A run that fails ends the session: nothing more is started.  No threshold is set for SegNet: there
is no earlier figure; the bar for --weights deeplab is the parent's figure within the session's run-to-run spread."""
import argparse
import os
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
    """One process: the two backbones' forward passes and the two kernels at the pass's sizes."""
    sys.path.insert(0, ROOT)
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
        extra = ', %d bytes of scratch memory' % cfg.segnet_scratch_bytes() if backbone == 'segnet' else ''
        print('%s backbone forward at 768 x 768, random weights: %s ms per pass (three windows of %d passes between two device events)%s'
              % (backbone, ' '.join('%.3f' % m for m in ms), args.reps, extra))
        model.close()
        del model
        torch.cuda.empty_cache()
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
    args = ap.parse_args()
    if args.worker:
        return worker(args)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), '--worker', '--reps', str(args.reps)], stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, universal_newlines=True, timeout=args.timeout)
    if r.returncode != 0:
        sys.stderr.write(r.stderr[-4000:])
        raise SystemExit('the worker failed: exit status %d -- nothing more is started' % r.returncode)
    lines = r.stdout.strip().split('\n')
    print('\n'.join(lines), flush=True)
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
        if args.parent:
            plan.append(('parent ' + cache, os.path.abspath(args.parent), ['--scene_cache', cache]))
        plan.append(('deeplab ' + cache, ROOT, ['--scene_cache', cache, '--weights', 'deeplab']))
        plan.append(('segnet ' + cache, ROOT, ['--scene_cache', cache] + seg))
    res = {name: [] for name, _, _ in plan}
    for rep in range(args.repeats):
        for name, tree, extra in plan:
            ms, said = base_rate.run(tree, base, '%s_%d' % (name.replace(' ', '_'), rep), args, extra)
            res[name].append(sum(ms[1:]) / max(1, len(ms[1:])))
            lines.append('[%-16s run %d] %s  -> %.2f' % (name, rep + 1, ' '.join('%.2f' % m for m in ms), res[name][-1]))
            if rep == 0:
                lines += ['[%-16s run 1] %s' % (name, s) for s in said if s.startswith('scene cache:')]
            print(lines[-1], flush=True)
    mean = {k: sum(v) / len(v) for k, v in res.items()}
    spread = {k: max(v) - min(v) for k, v in res.items()}
    lines.append('mean of the runs (run-to-run spread): ' + ', '.join('%s %.2f (%.2f)' % (k, mean[k], spread[k]) for k in res))
    for cache in ('device', 'features'):
        if args.parent:
            a, b = 'deeplab ' + cache, 'parent ' + cache
            s, d = max(spread[a], spread[b]), mean[a] - mean[b]
            lines.append('--weights deeplab --scene_cache %s %.2f ms against the parent %.2f ms: %+.2f ms (%+.1f %%), %s the run-to-run '
                         'spread of %.2f ms' % (cache, mean[a], mean[b], d, 100 * d / mean[b],
                                                'not slower beyond' if d <= s else 'SLOWER by more than', s))
        d = mean['segnet ' + cache] - mean['deeplab ' + cache]
        lines.append('--weights segnet --scene_cache %s %.2f ms against --weights deeplab %.2f ms: %+.2f ms (recorded, not bounded)'
                     % (cache, mean['segnet ' + cache], mean['deeplab ' + cache], d))
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
