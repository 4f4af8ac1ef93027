"""Rate of ``match_main.py --mode train`` at 768 x 768 trained from png and mat files with --scene_cache off, device and features,
and of the same command line of another tree (the parent commit) -- every configuration twice, in turn, in one session on one
card -- then the time of one held-out pass and of one ssc_match_score launch.

    python scripts/match_cache_rate.py --parent /path/to/a/built/checkout/of/the/parent --out profiles/match_cache.txt

The data is synthetic and written here into a temporary directory: --scenes scenes (a 768 x 768 sketch png, a 750 x 750 INSTANCE_GT
with five instances, so that the label map is zoomed as the real ones are) with --captions captions each, as the train split and
again as the val split, and a random backbone of the released shape as a TensorFlow checkpoint.  Every run is a process of its
own under its own time limit, started with unbuffered output; the command line prints a line every --window iterations after it
has read that iteration's loss (it waits for the device there), and the time between two such lines over --window is the ms per
iteration of that window.  The first window (start-up, the first launches) is shown and left out of the mean.  A run that fails
ends the session: nothing more is started."""
import argparse
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VOCAB = os.path.join(ROOT, 'tests', 'golden', 'match', 'vocab.txt')
CAPTIONS = [('the house on the left', [0]), ('two trees on the right', [1, 3]), ('all the people near the bus', [2, 4, 2]),
            ('the car in the middle', [2]), ('the dog near the tree', [4]), ('the cloud on the top', [1])]


def write_data(base, n_scenes, n_captions, size=768, size_gt=750):
    import numpy as np
    import scipy.io
    from PIL import Image
    sys.path.insert(0, ROOT)
    from sketchyscenecolorization_amd import matching, tf_checkpoint
    rng = np.random.RandomState(0)
    data, caps = os.path.join(base, 'data'), os.path.join(base, 'captions')
    os.makedirs(caps)
    for split in ('train', 'val'):
        for d in ('INSTANCE_GT', 'DRAWING_GT'):
            os.makedirs(os.path.join(data, split, d))
        entries = []
        for key in range(100, 100 + n_scenes):
            gt = np.zeros((size_gt, size_gt), np.uint8)
            for k in range(5):
                y, x = int(rng.randint(0, size_gt - 260)), int(k * 140 + rng.randint(0, 20))
                gt[y:y + 250, x:x + 120] = (k + 1) * 5
            scipy.io.savemat(os.path.join(data, split, 'INSTANCE_GT', 'sample_%d_instance.mat' % key), {'INSTANCE_GT': gt})
            sk = np.full((size, size, 3), 255, np.uint8)
            sk[rng.rand(size, size) < 0.1] = 0
            Image.fromarray(sk).save(os.path.join(data, split, 'DRAWING_GT', 'L0_sample%d.png' % key))
            entries.append({'key': key, 'sen_instIdx_map': {c: idx for c, idx in CAPTIONS[:n_captions]}})
        with open(os.path.join(caps, 'sentence_instance_%s.json' % split), 'w') as f:
            json.dump(entries, f)
    cfg = matching.MatchConfig()
    backbone = os.path.join(base, 'backbone-1')
    tf_checkpoint.write_checkpoint(backbone, {k: a for k, a in matching.random_variables(cfg, 1).items() if k.startswith('ResNet/')})
    return data, caps, backbone


def cli_cmd(tree, base, tag, iters, window, extra):
    root = os.path.join(base, 'runs', tag)
    return [sys.executable, '-u', os.path.join(tree, 'match_main.py'), '--mode', 'train', '--backbone_snapshot', os.path.join(base, 'backbone-1'),
            '--vocab_file', VOCAB, '--data_base_dir', os.path.join(base, 'data'), '--captions_base_dir', os.path.join(base, 'captions'),
            '--snapshot_root', root, '--log_root', root + '_log', '--max_iteration', str(iters), '--save_model_freq', '1000000',
            '--log_freq', str(window), '--seed', '1'] + extra


def run(tree, base, tag, args, extra):
    """-> (ms per iteration of every window, the lines the command line printed about its caches and its passes)."""
    errors = open(os.path.join(base, 'stderr_%s.txt' % tag), 'w+')
    p = subprocess.Popen(cli_cmd(tree, base, tag, args.iters, args.window, extra), cwd=base, stdout=subprocess.PIPE, stderr=errors,
                         universal_newlines=True)
    deadline = time.time() + args.timeout
    stamps, notes = [], []
    for line in p.stdout:
        now = time.time()
        if line.startswith('start_iter') or line.startswith('iter = '):
            stamps.append(now)
        elif line.startswith(('scene cache:', 'validation cache:', 'val: ')):
            notes.append(line.strip())
        if now > deadline:
            p.kill()
            raise SystemExit('run %s ran into its time limit of %d s -- nothing more is started' % (tag, args.timeout))
    if p.wait() != 0:
        errors.seek(0)
        sys.stderr.write(errors.read()[-4000:])
        raise SystemExit('run failed (%s): exit status %d -- nothing more is started' % (tag, p.returncode))
    errors.close()
    shutil.rmtree(os.path.join(base, 'runs', tag), ignore_errors=True)
    return [1e3 * (b - a) / args.window for a, b in zip(stamps[:-1], stamps[1:])], notes


def worker(args):
    """One process: the val cache, one held-out pass (after a first one that pays for the first launches), and ssc_match_score
    between device events."""
    sys.path.insert(0, ROOT)
    import torch
    from sketchyscenecolorization_amd import hip, match_validation, matching
    cfg = matching.MatchConfig()
    model = matching.MatchModel(cfg)
    model.init_random(1)
    vocab = matching.load_vocab(VOCAB)
    scenes = match_validation.validation_scenes(os.path.join(args.data, 'captions'), os.path.join(args.data, 'data'))
    t0 = time.time()
    val = match_validation.MatchValidation(model, vocab, scenes, os.path.join(args.data, 'data'))
    print('val cache: %d scenes, %d captions, %d bytes, built in %.2f s' % (len(val.cache), val.captions, val.nbytes, time.time() - t0))
    for k in range(3):
        rec = val.run(k)
        print('held-out pass %d: %d scenes, %d captions, %.3f s (%.2f ms per caption)' % (k + 1, rec['scenes'], rec['captions'], rec['seconds'],
                                                                                       1e3 * rec['seconds'] / rec['captions']))
    pred = torch.randn((cfg.feat, cfg.feat), device='cuda')
    out = torch.zeros(5, dtype=torch.int64, device='cuda')
    ws = hip.workspace()
    for _ in range(5):
        hip.match_score(pred, val.cache.sketch[0], val.cache.labels[0], val.lut[0], out=out, ws=ws)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(args.reps):
        hip.match_score(pred, val.cache.sketch[0], val.cache.labels[0], val.lut[0], out=out, ws=ws)
    b.record()
    torch.cuda.synchronize()
    print('ssc_match_score at %d x %d: %.1f us per call (both launches), %d calls between two device events'
          % (cfg.size, cfg.size, 1e3 * a.elapsed_time(b) / args.reps, args.reps))
    model.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--parent', default='', help='a built checkout of the parent commit (timed beside this tree)')
    ap.add_argument('--scenes', type=int, default=32)
    ap.add_argument('--captions', type=int, default=4)
    ap.add_argument('--iters', type=int, default=301)
    ap.add_argument('--window', type=int, default=50)
    ap.add_argument('--repeats', type=int, default=2)
    ap.add_argument('--timeout', type=int, default=240)
    ap.add_argument('--out', default='')
    ap.add_argument('--worker', action='store_true')
    ap.add_argument('--reps', type=int, default=200)
    ap.add_argument('--data', default='')
    args = ap.parse_args()
    if args.worker:
        return worker(args)
    base = tempfile.mkdtemp()
    t0 = time.time()
    write_data(base, args.scenes, args.captions)
    lines = ['match_main.py --mode train at 768 x 768, %d iterations: %d synthetic scenes (png + mat) with %d captions each and a random '
             'backbone, written in %.1f s; ms per iteration of each window of %d (first window: start-up, not in the mean); %d CPUs'
             % (args.iters, args.scenes, args.captions, time.time() - t0, args.window, len(os.sched_getaffinity(0)))]
    plan = ([('parent', os.path.abspath(args.parent), [])] if args.parent else []) + \
        [('off', ROOT, ['--scene_cache', 'off']), ('device', ROOT, ['--scene_cache', 'device']), ('features', ROOT, ['--scene_cache', 'features'])]
    res, notes = {name: [] for name, _, _ in plan}, []
    for rep in range(args.repeats):
        for name, tree, extra in plan:
            ms, said = run(tree, base, '%s_%d' % (name, rep), args, extra)
            res[name].append(sum(ms[1:]) / max(1, len(ms[1:])))
            notes += ['[%-8s run %d] %s' % (name, rep + 1, s) for s in said]
            lines.append('[%-8s run %d] %s  -> %.2f' % (name, rep + 1, ' '.join('%.2f' % m for m in ms), res[name][-1]))
            print(lines[-1], flush=True)
    lines += notes
    mean = {k: sum(v) / len(v) for k, v in res.items()}
    spread = {k: max(v) - min(v) for k, v in res.items()}
    lines.append('mean of the runs (run-to-run spread): ' + ', '.join('%s %.2f (%.2f)' % (k, mean[k], spread[k]) for k in res))

    def compare(a, b):
        s = max(spread[a], spread[b])
        d = mean[a] - mean[b]
        lines.append('%s %.2f ms against %s %.2f ms: %+.2f ms (%+.1f %%), %s the run-to-run spread of %.2f ms'
                     % (a, mean[a], b, mean[b], d, 100 * d / mean[b], 'not slower beyond' if d <= s else 'SLOWER by more than', s))
    if args.parent:
        compare('off', 'parent')
    compare('device', 'off')
    compare('features', 'off')
    lines.append('the drop from device to features: %.2f ms (profiles/match_train.txt gives the backbone 6.9 ms of the step)'
                 % (mean['device'] - mean['features']))
    # a run with a pass every window, for the cost of a pass inside the command line
    ms, said = run(ROOT, base, 'val', args, ['--scene_cache', 'features', '--val_freq', str(args.window), '--val_scenes', str(min(8, args.scenes))])
    lines.append('[features + --val_freq %d --val_scenes %d] %s  -> %.2f' % (args.window, min(8, args.scenes), ' '.join('%.2f' % m for m in ms),
                                                                             sum(ms[1:]) / max(1, len(ms[1:]))))
    lines += said[:3]
    r = subprocess.run([sys.executable, os.path.abspath(__file__), '--worker', '--data', base, '--reps', str(args.reps)], cwd=base,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True, timeout=args.timeout)
    if r.returncode != 0:
        sys.stderr.write(r.stderr[-4000:])
        raise SystemExit('the worker failed: exit status %d' % r.returncode)
    lines += r.stdout.strip().split('\n')
    shutil.rmtree(base, ignore_errors=True)
    text = '\n'.join(lines) + '\n'
    print(text)
    if args.out:
        with open(args.out, 'w') as fp:
            fp.write(text)


if __name__ == '__main__':
    main()
