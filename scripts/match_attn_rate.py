"""Rate of ``match_main.py --mode train --scene_cache features`` at 768 x 768 with --use_attn 0 and --use_attn 1, and of the same
command line of another tree (the parent commit, which has no such flag) -- every configuration twice, in turn, in one session on
one card.

    python scripts/match_attn_rate.py --parent /path/to/a/built/checkout/of/the/parent --out profiles/match_attn.txt

The synthetic scenes, the random backbone, the processes under their own time limits and the windows are those of
scripts/match_cache_rate.py: the time between two printed lines over --window is the ms per iteration of that window, the first
window (start-up, the first launches) is shown and left out of the mean.  A run that fails ends the session: nothing more is
started.  The bar for --use_attn 0 is the parent's figure within the session's run-to-run spread; what --use_attn 1 adds is
recorded, not bounded."""
import argparse
import os
import shutil
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import match_cache_rate as base_rate       # noqa: E402

ROOT = base_rate.ROOT


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--parent', default='', help='a built checkout of the parent commit (timed beside this tree)')
    ap.add_argument('--scenes', type=int, default=16)
    ap.add_argument('--captions', type=int, default=4)
    ap.add_argument('--iters', type=int, default=301)
    ap.add_argument('--window', type=int, default=50)
    ap.add_argument('--repeats', type=int, default=2)
    ap.add_argument('--timeout', type=int, default=240)
    ap.add_argument('--out', default='')
    args = ap.parse_args()
    base = tempfile.mkdtemp()
    t0 = time.time()
    base_rate.write_data(base, args.scenes, args.captions)
    lines = ['match_main.py --mode train --scene_cache features at 768 x 768, %d iterations: %d synthetic scenes (png + mat) with %d '
             'captions each and a random backbone, written in %.1f s; ms per iteration of each window of %d (first window: start-up, '
             'not in the mean); %d CPUs' % (args.iters, args.scenes, args.captions, time.time() - t0, args.window,
                                           len(os.sched_getaffinity(0)))]
    cache = ['--scene_cache', 'features']
    plan = ([('parent', os.path.abspath(args.parent), cache)] if args.parent else []) + \
        [('attn0', ROOT, cache + ['--use_attn', '0']), ('attn1', ROOT, cache + ['--use_attn', '1'])]
    res = {name: [] for name, _, _ in plan}
    for rep in range(args.repeats):
        for name, tree, extra in plan:
            ms, _said = base_rate.run(tree, base, '%s_%d' % (name, rep), args, extra)
            res[name].append(sum(ms[1:]) / max(1, len(ms[1:])))
            lines.append('[%-6s run %d] %s  -> %.2f' % (name, rep + 1, ' '.join('%.2f' % m for m in ms), res[name][-1]))
            print(lines[-1], flush=True)
    mean = {k: sum(v) / len(v) for k, v in res.items()}
    spread = {k: max(v) - min(v) for k, v in res.items()}
    lines.append('mean of the runs (run-to-run spread): ' + ', '.join('%s %.2f (%.2f)' % (k, mean[k], spread[k]) for k in res))
    if args.parent:
        s = max(spread['attn0'], spread['parent'])
        d = mean['attn0'] - mean['parent']
        lines.append('--use_attn 0 %.2f ms against the parent %.2f ms: %+.2f ms (%+.1f %%), %s the run-to-run spread of %.2f ms'
                     % (mean['attn0'], mean['parent'], d, 100 * d / mean['parent'], 'not slower beyond' if d <= s else 'SLOWER by more than', s))
    d = mean['attn1'] - mean['attn0']
    lines.append('--use_attn 1 %.2f ms against --use_attn 0 %.2f ms: %+.2f ms (%+.1f %%) for the attention (recorded, not bounded)'
                 % (mean['attn1'], mean['attn0'], d, 100 * d / mean['attn0']))
    shutil.rmtree(base, ignore_errors=True)
    text = '\n'.join(lines) + '\n'
    print(text)
    if args.out:
        with open(args.out, 'w') as fp:
            fp.write(text)


if __name__ == '__main__':
    main()
