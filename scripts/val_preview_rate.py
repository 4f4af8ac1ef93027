"""What the preview sheets cost (--val_preview K): the two kernels of csrc/preview.hip alone, the held-out
pass of each trainer with K = 0 and K = 8, and the training iteration with every flag at 0 beside another tree (the parent commit).

    python scripts/val_preview_rate.py --parent /path/to/a/built/checkout/of/the/parent --out profiles/val_preview.txt

One box, one session.  Every part is a process of its own under its own time limit; a part that fails ends the session: nothing
more is started.  Times are medians between two device events, and every configuration is measured twice in turn (A B A B), so
that the difference of two runs of one configuration stands beside the difference of two configurations.
  kernels     ssc_sheet_tiles_u8 and ssc_sheet_overlay_u8 at 768 x 768 (s = 2) and 192 x 192 (s = 1), one launch between events
  foreground  train_validation.HeldOutEvaluator.run over 64 synthetic records at 192 x 192, batch 32, Pix2Pix (the set of
              scripts/train_validation_rate.py)
  background  bg_validation.HeldOutEvaluator.run over 8 synthetic scenes at 768 x 768 (the set of scripts/bg_validation_rate.py)
  matcher     match_validation.MatchValidation.run over 4 scenes of 4 captions at 768 x 768 (the set of scripts/match_cache_rate.py)
  iteration   bench.py --gpus 1 (the Foreground train step, no flag of this change given) in this tree and in --parent
A pass is timed from before its first launch to behind the copy of its sheet (or, with K = 0, of its rows) to the host."""
import argparse
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))
K = 8


def median(v):
    v = sorted(v)
    return v[len(v) // 2]


def timed(fn, reps, warm=3):
    """The median, fastest and slowest of ``reps`` calls, each between two device events, in microseconds."""
    import torch
    for _ in range(warm):
        fn()
    us = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        us.append(1e3 * e0.elapsed_time(e1))
    return median(us), min(us), max(us)


def in_turn(configs, reps, fmt='%s: %.1f us (%.1f .. %.1f)'):
    """configs: [(name, fn)]: each timed twice, in turn.  -> lines."""
    lines, got = [], {}
    for turn in (1, 2):
        for name, fn in configs:
            m, lo, hi = timed(fn, reps)
            got.setdefault(name, []).append(m)
            lines.append(('[turn %d] ' % turn) + fmt % (name, m, lo, hi))
    for name, _fn in configs:
        a, b = got[name]
        lines.append('%s: mean of the two turns %.1f us, they differ by %.1f us' % (name, (a + b) / 2, abs(a - b)))
    return lines, {name: sum(v) / 2 for name, v in got.items()}, {name: abs(v[0] - v[1]) for name, v in got.items()}


# ---------------------------------------------------------------------------------------------------------------------------
def part_kernels(args):
    import torch
    from sketchyscenecolorization_amd import hip, preview
    g = torch.Generator(device='cuda')
    g.manual_seed(1)
    configs = []
    for side, s in ((768, 2), (192, 1)):
        tile = side // s
        sheet = preview.Sheet(1, 2, tile, tile, 'cuda')
        src = torch.randint(0, 256, (1, side, side, 3), device='cuda', generator=g, dtype=torch.uint8)
        pred = (torch.rand((side, side), device='cuda', generator=g) < 0.4).to(torch.uint8)
        labels = torch.randint(0, 6, (side, side), device='cuda', generator=g, dtype=torch.uint8)
        lut = torch.zeros(256, dtype=torch.uint8, device='cuda')
        lut[1] = lut[4] = 1
        configs.append(('ssc_sheet_tiles_u8 %d^2 s=%d' % (side, s), lambda src=src, s=s, sheet=sheet: sheet.tiles(src, s, 0, 0)))
        configs.append(('ssc_sheet_overlay_u8 %d^2 s=%d' % (side, s),
                        lambda src=src, s=s, sheet=sheet, pred=pred, labels=labels, lut=lut: sheet.overlay(src[0], pred, labels, lut, s, 0, 1)))
    lines, mean, _d = in_turn(configs, args.reps)
    for (side, s), name in zip(((768, 2), (768, 2), (192, 1), (192, 1)), [c[0] for c in configs]):
        moved = side * side * (3 if 'tiles' in name else 5) + (side // s) ** 2 * 3
        lines.append('%s: %d bytes read and written, %.0f GB/s' % (name, moved, moved / (mean[name] * 1e-6) / 1e9))
    print('\n'.join(lines))


def passes(name, make, run, args):
    """make(K) -> an evaluator; run(evaluator) is one pass, the sheet's copy to the host included."""
    evs = {k: make(k) for k in (0, K)}
    lines, mean, diff = in_turn([('%s pass, --val_preview %d' % (name, k), lambda k=k: run(evs[k])) for k in (0, K)], args.pass_reps,
                                fmt='%s: %.0f us (%.0f .. %.0f)')
    a, b = mean['%s pass, --val_preview 0' % name], mean['%s pass, --val_preview %d' % (name, K)]
    lines.append('%s: the preview of %d rows adds %.0f us to a pass of %.0f us (%+.1f %%); two turns of one configuration differ by up to %.0f us'
                 % (name, K, b - a, a, 100 * (b - a) / a, max(diff.values())))
    print('\n'.join(lines))


def part_foreground(args):
    sys.path.insert(0, HERE)
    import train_validation_rate as TVR
    from sketchyscenecolorization_amd import record_cache, train_validation
    from sketchyscenecolorization_amd.obj_lib import models_collection as models
    base = tempfile.mkdtemp()
    d = TVR.write_dataset(base, 'val', 64, 2)
    cache = record_cache.RecordCache(record_cache.list_record_files(d), 192, device='cuda')
    tower = models.get_trainer('Pix2Pix', 58, 192)
    tower.G.lstm_hybrid = True

    def run(ev):
        ev.run(tower)
        if ev.preview is not None:
            ev.preview.sheet.host()
    passes('foreground (64 records at 192^2, batch 32)', lambda k: train_validation.HeldOutEvaluator(cache, 32, preview=k), run, args)
    shutil.rmtree(base, ignore_errors=True)


def part_background(args):
    sys.path.insert(0, HERE)
    import bg_validation_rate as BVR
    import bg_colorization_main as cli
    from sketchyscenecolorization_amd import bg_validation
    from sketchyscenecolorization_amd.bg_colorization import BGTrainer
    base = os.path.join(tempfile.mkdtemp(), 'data')
    BVR.write_dataset(base, 'val', 8, 8)
    tr = BGTrainer(image_size=768, seed=1)
    p = {'data_base_dir': base, 'image_size': 768, 'text_len': 8, 'vocab_size': 18, 'vocab_file': os.path.join(base, 'bg_vocab.txt'),
         'val_freq': 1, 'val_records': 0, 'seg_classes': 3}

    def run(ev):
        ev.run(tr)
        if ev.preview is not None:
            ev.preview.sheet.host()
    passes('background (8 scenes at 768^2)', lambda k: bg_validation.open_held_out(dict(p, val_preview=k), cli.Scenes, tr), run, args)
    shutil.rmtree(os.path.dirname(base), ignore_errors=True)


def part_matcher(args):
    sys.path.insert(0, HERE)
    import match_cache_rate as MCR
    from sketchyscenecolorization_amd import match_validation, matching
    base = tempfile.mkdtemp()
    MCR.write_data(base, 4, 4)
    cfg = matching.MatchConfig()
    model = matching.MatchModel(cfg)
    model.init_random(1)
    vocab = matching.load_vocab(MCR.VOCAB)
    scenes = match_validation.validation_scenes(os.path.join(base, 'captions'), os.path.join(base, 'data'))

    def run(ev):
        ev.run(0)
        if ev.preview is not None:
            ev.preview.sheet.host()
    passes('matcher (4 scenes, 16 captions at 768^2)',
           lambda k: match_validation.MatchValidation(model, vocab, scenes, os.path.join(base, 'data'), preview=k), run, args)
    model.close()
    shutil.rmtree(base, ignore_errors=True)


PARTS = {'kernels': part_kernels, 'foreground': part_foreground, 'background': part_background, 'matcher': part_matcher}


def child(cmd, what, args, cwd=None):
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True, timeout=args.timeout, cwd=cwd)
    if r.returncode != 0:
        sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
        raise SystemExit('%s failed: exit status %d -- nothing more is started' % (what, r.returncode))
    return r.stdout


def iteration(args):
    """bench.py in this tree and in the parent's, twice in turn: the value of its JSON line."""
    trees = [('this tree', ROOT)] + ([('parent', os.path.abspath(args.parent))] if args.parent else [])
    got, lines = {}, []
    for turn in (1, 2):
        for name, tree in trees:
            out = child([sys.executable, os.path.join(tree, 'bench.py'), '--gpus', '1', '--steps', str(args.bench_steps), '--warmup',
                         str(args.bench_warmup)], 'bench.py of %s' % name, args, cwd=tree)
            rec = [json.loads(l) for l in out.splitlines() if l.startswith('{')][-1]
            value = float(rec.get('value', rec.get('images_per_sec', 0.0)))
            got.setdefault(name, []).append(value)
            lines.append('[turn %d] bench.py --gpus 1 --steps %d --warmup %d, %s: %s %.1f %s' % (turn, args.bench_steps, args.bench_warmup, name,
                                                                                              rec.get('metric', 'value'), value, rec.get('unit', '')))
    mean = {k: sum(v) / len(v) for k, v in got.items()}
    spread = {k: max(v) - min(v) for k, v in got.items()}
    lines.append('mean of the two turns (their difference): ' + ', '.join('%s %.1f (%.1f)' % (k, mean[k], spread[k]) for k in got))
    if args.parent:
        d, s = mean['this tree'] - mean['parent'], max(spread.values())
        lines.append('this tree against the parent: %+.1f (%+.2f %%), %s the run-to-run spread of %.1f'
                     % (d, 100 * d / mean['parent'], 'inside' if abs(d) <= s else 'OUTSIDE', s))
    else:
        lines.append('no --parent given: the iteration time of the parent commit was not measured')
    return lines


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--parent', default='', help='a built checkout of the parent commit (its bench.py is run beside this tree\'s)')
    ap.add_argument('--reps', type=int, default=200, help='launches of a kernel per turn')
    ap.add_argument('--pass-reps', type=int, default=7, help='passes per turn')
    ap.add_argument('--bench-steps', type=int, default=60)
    ap.add_argument('--bench-warmup', type=int, default=10)
    ap.add_argument('--timeout', type=int, default=420)
    ap.add_argument('--only', default='', help='comma-separated parts (kernels, foreground, background, matcher, iteration); default: all')
    ap.add_argument('--out', default='')
    ap.add_argument('--part', default='', help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.part:
        sys.path.insert(0, ROOT)
        return PARTS[args.part](args)
    only = [p for p in args.only.split(',') if p] or list(PARTS) + ['iteration']
    lines = ['preview sheets: medians between device events, every configuration twice in turn; %d CPUs; %s'
             % (len(os.sched_getaffinity(0)), time.strftime('%Y-%m-%d', time.gmtime()))]
    for part in only:
        if part == 'iteration':
            lines += iteration(args)
        else:
            out = child([sys.executable, os.path.abspath(__file__), '--part', part, '--reps', str(args.reps), '--pass-reps', str(args.pass_reps)],
                        'the part %r' % part, args)
            lines += [l for l in out.splitlines() if ': ' in l and ('[turn' in l or 'mean of' in l or 'adds' in l or 'GB/s' in l)]
        print('\n'.join(lines[-12:]), flush=True)
    text = '\n'.join(lines) + '\n'
    if args.out:
        with open(args.out, 'w') as fp:
            fp.write(text)
    print(text)


if __name__ == '__main__':
    main()
