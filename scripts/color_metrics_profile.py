"""What the colour scores cost (--color_metrics 1): the three kernels of csrc/color_metrics.hip beside the
three of csrc/metrics.hip at the same shapes, the held-out pass of both trainers with the flag at 0 and at 1, and the flag-0 pass
beside the same pass in another tree (the parent commit).

    python scripts/color_metrics_profile.py --parent /path/to/a/built/checkout/of/the/parent --out profiles/color_metrics.txt

One box, one session.  Every part is a process of its own under its own time limit; a part that fails ends the session: nothing
more is started.  Times are medians between two device events, and every configuration is measured twice in turn (A B A B), so
that the difference of two runs of one configuration stands beside the difference of two configurations.
  kernels     (32,192,192): ssc_color_metrics_u8 and _f32 (NHWC of 4 floats against a planar target: the Foreground pass's call)
              beside ssc_image_metrics_u8 and _f32; (1,768,768): ssc_color_metrics_bg_f32 under a mask beside
              ssc_image_metrics_bg_f32; both launches of an entry between the events
  foreground  train_validation.HeldOutEvaluator.run over 64 synthetic records at 192 x 192, batch 32, Pix2Pix (the set of
              scripts/train_validation_rate.py)
  background  bg_validation.HeldOutEvaluator.run over 8 synthetic scenes at 768 x 768 (the set of scripts/bg_validation_rate.py)
  parent      the two passes with the code of --parent, which has no flag
A pass is timed from before its first launch to behind the copy of its rows to the host."""
import argparse
import os
import shutil
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from val_preview_rate import child, in_turn      # noqa: E402


def part_kernels(args):
    import torch
    from sketchyscenecolorization_amd import hip
    g = torch.Generator(device='cuda')
    g.manual_seed(1)
    n, s = 32, 192
    a8 = torch.randint(0, 256, (n, s, s, 3), device='cuda', generator=g, dtype=torch.uint8)
    b8 = torch.randint(0, 256, (n, s, s, 3), device='cuda', generator=g, dtype=torch.uint8)
    af = torch.rand((n, s, s, 4), device='cuda', generator=g) * 2 - 1
    bp = torch.rand((n, 3, s, s), device='cuda', generator=g) * 2 - 1
    S = 768
    img = torch.rand((1, S, S, 4), device='cuda', generator=g) * 2 - 1
    fg = torch.randint(0, 256, (1, S, S, 3), device='cuda', generator=g, dtype=torch.uint8)
    tg = torch.randint(0, 256, (1, S, S, 3), device='cuda', generator=g, dtype=torch.uint8)
    mask = (torch.rand((1, S, S), device='cuda', generator=g) < 0.7).to(torch.uint8) * 255
    oc, om = torch.empty((n, 13), dtype=torch.float64, device='cuda'), torch.empty((n, 5), dtype=torch.float64, device='cuda')
    configs = [
        ('ssc_color_metrics_u8 (32,192,192)', lambda: hip.color_metrics_u8(a8, b8, out=oc)),
        ('ssc_image_metrics_u8 (32,192,192)', lambda: hip.image_metrics_u8(a8, b8, out=om)),
        ('ssc_color_metrics_f32 (32,192,192)', lambda: hip.color_metrics_f32(af, 0, bp, out=oc)),
        ('ssc_image_metrics_f32 (32,192,192)', lambda: hip.image_metrics_f32(af, 0, bp, out=om)),
        ('ssc_color_metrics_bg_f32 (1,768,768) masked', lambda: hip.color_metrics_bg_f32(img, fg, tg, mask, out=oc[:1])),
        ('ssc_image_metrics_bg_f32 (1,768,768) masked', lambda: hip.image_metrics_bg_f32(img, fg, tg, mask, out=om[:1])),
    ]
    lines, mean, _d = in_turn(configs, args.reps)
    for name, pixels in zip([c[0] for c in configs], [n * s * s] * 4 + [S * S] * 2):
        lines.append('%s: %.2f ns per pixel' % (name, mean[name] * 1e3 / pixels))
    print('\n'.join(lines))


def passes(name, make, run, args, flags):
    """make(flag) -> an evaluator; run(evaluator) is one pass."""
    evs = {k: make(k) for k in flags}
    lines, mean, diff = in_turn([('%s pass, --color_metrics %d' % (name, k), lambda k=k: run(evs[k])) for k in flags], args.pass_reps,
                                fmt='%s: %.0f us (%.0f .. %.0f)')
    if len(flags) == 2:
        a, b = mean['%s pass, --color_metrics 0' % name], mean['%s pass, --color_metrics 1' % name]
        lines.append('%s: the colour scores add %.0f us to a pass of %.0f us (%+.2f %%); two turns of one configuration differ by up to %.0f us'
                     % (name, b - a, a, 100 * (b - a) / a, max(diff.values())))
    print('\n'.join(lines))


def part_foreground(args):
    import train_validation_rate as TVR
    from sketchyscenecolorization_amd import record_cache, train_validation
    from sketchyscenecolorization_amd.obj_lib import models_collection as models
    base = tempfile.mkdtemp()
    d = TVR.write_dataset(base, 'val', 64, 2)
    cache = record_cache.RecordCache(record_cache.list_record_files(d), 192, device='cuda')
    tower = models.get_trainer('Pix2Pix', 58, 192)
    tower.G.lstm_hybrid = True
    flags = (0,) if args.tree else (0, 1)       # (the parent's evaluator takes no flag)
    make = lambda k: train_validation.HeldOutEvaluator(cache, 32, **({'color': True} if k else {}))      # noqa: E731
    passes('foreground (64 records at 192^2, batch 32)' + (' [parent]' if args.tree else ''), make, lambda ev: ev.run(tower), args, flags)
    shutil.rmtree(base, ignore_errors=True)


def part_background(args):
    import bg_validation_rate as BVR
    import bg_colorization_main as cli
    from sketchyscenecolorization_amd import bg_validation
    from sketchyscenecolorization_amd.bg_colorization import BGTrainer
    base = os.path.join(tempfile.mkdtemp(), 'data')
    BVR.write_dataset(base, 'val', 8, 8)
    tr = BGTrainer(image_size=768, seed=1)
    p = {'data_base_dir': base, 'image_size': 768, 'text_len': 8, 'vocab_size': 18, 'vocab_file': os.path.join(base, 'bg_vocab.txt'),
         'val_freq': 1, 'val_records': 0, 'seg_classes': 3}
    flags = (0,) if args.tree else (0, 1)
    make = lambda k: bg_validation.open_held_out(dict(p, **({'color_metrics': 1} if k else {})), cli.Scenes, tr)      # noqa: E731
    passes('background (8 scenes at 768^2)' + (' [parent]' if args.tree else ''), make, lambda ev: ev.run(tr), args, flags)
    shutil.rmtree(os.path.dirname(base), ignore_errors=True)


PARTS = {'kernels': part_kernels, 'foreground': part_foreground, 'background': part_background}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--parent', default='', help='a built checkout of the parent commit: its passes are timed beside the flag-0 passes')
    ap.add_argument('--reps', type=int, default=200, help='calls of an entry point per turn')
    ap.add_argument('--pass-reps', type=int, default=7, help='passes per turn')
    ap.add_argument('--timeout', type=int, default=420)
    ap.add_argument('--only', default='', help='comma-separated parts (kernels, foreground, background, parent); default: all')
    ap.add_argument('--out', default='')
    ap.add_argument('--part', default='', help=argparse.SUPPRESS)
    ap.add_argument('--tree', default='', help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.part:       # a part runs the package and the data-set writers of one tree: this one, or the parent's
        tree = os.path.abspath(args.tree) if args.tree else ROOT
        sys.path.insert(0, os.path.join(tree, 'scripts'))
        sys.path.insert(0, tree)
        return PARTS[args.part](args)
    only = [p for p in args.only.split(',') if p] or list(PARTS) + ['parent']
    lines = ['colour scores: medians between device events, every configuration twice in turn, %d calls of a kernel entry and %d passes '
             'per turn; %d CPUs; %s' % (args.reps, args.pass_reps, len(os.sched_getaffinity(0)), time.strftime('%Y-%m-%d', time.gmtime()))]
    me = [sys.executable, os.path.abspath(__file__), '--reps', str(args.reps), '--pass-reps', str(args.pass_reps)]
    keep = lambda out: [l for l in out.splitlines() if ': ' in l and ('[turn' in l or 'mean of' in l or ' add ' in l or 'per pixel' in l)]      # noqa: E731
    for part in only:
        if part == 'parent':
            if not args.parent:
                lines.append('no --parent given: the passes of the parent commit were not measured')
                continue
            for p in ('foreground', 'background'):
                lines += keep(child(me + ['--part', p, '--tree', os.path.abspath(args.parent)], 'the part %r of the parent' % p, args, cwd=os.path.abspath(args.parent)))
        else:
            lines += keep(child(me + ['--part', part], 'the part %r' % part, args))
        print('\n'.join(lines[-14:]), flush=True)
    text = '\n'.join(lines) + '\n'
    if args.out:
        with open(args.out, 'w') as fp:
            fp.write(text)
    print(text)


if __name__ == '__main__':
    main()
