"""Time of the --metrics 1 kernels (csrc/metrics.hip) inside the two command lines, from rocprofv3 --kernel-trace --stats:

    python scripts/image_metrics_profile.py --out profiles/image_metrics.txt

1. ``obj_colorization_main.py --mode val -bt Pix2Pix -bs 32 -mt 1`` at 192 x 192 on a run trained here for two iterations (the
   synthetic validation batch: one call on 32 images), and
2. ``bg_colorization_main.py --mode test --image_size 768 --metrics 1`` on a run trained here for one step (the eight synthetic
   scenes: eight calls on one image, no mask).

Every command is a process of its own under its own time limit, in a temporary directory; the first one that fails ends the
script.  The file is a record of what was measured, not a threshold."""
import argparse
import csv
import glob
import os
import shutil
import socket
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = ('image_metrics_u8_kernel', 'image_metrics_sum_kernel')


def run(cmd, cwd, limit):
    r = subprocess.run(cmd, cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True, timeout=limit,
                       env=dict(os.environ, PYTHONPATH=ROOT))
    if r.returncode != 0:
        sys.stderr.write(r.stdout[-4000:])
        raise SystemExit('%s: exit status %d -- nothing more is started' % (' '.join(cmd[:6]), r.returncode))
    return r.stdout


def profiled(argv, cwd, limit):
    """The command under rocprofv3 (the program after --): its printed metrics line and the rows of the two kernels."""
    out = tempfile.mkdtemp()
    cmd = ['rocprofv3', '--kernel-trace', '--stats', '--output-format', 'csv', '-d', out, '-o', 'p', '--', sys.executable] + argv
    text = run(cmd, cwd, limit)
    rows = {}
    for path in glob.glob(os.path.join(out, '**', '*kernel_stats.csv'), recursive=True):
        with open(path) as fp:
            for row in csv.DictReader(fp):
                for k in KERNELS:
                    if k in row.get('Name', ''):
                        rows[k] = {c: row[c] for c in ('Calls', 'TotalDurationNs', 'AverageNs', 'MinNs', 'MaxNs', 'Percentage') if c in row}
    shutil.rmtree(out, ignore_errors=True)
    line = [l for l in text.splitlines() if l.startswith('metrics:')]
    return 'rocprofv3 --kernel-trace --stats -- python ' + ' '.join(argv), (line[0] if line else 'no metrics line'), rows


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--out', default='')
    ap.add_argument('--timeout', type=int, default=300)
    args = ap.parse_args()
    work = tempfile.mkdtemp()
    fg, bg = os.path.join(ROOT, 'obj_colorization_main.py'), os.path.join(ROOT, 'bg_colorization_main.py')
    name = run([sys.executable, '-c', 'import torch; print(torch.cuda.get_device_name(0))'], work, args.timeout).strip().splitlines()[-1]
    lines = ['box %s, %s; kernel times from one rocprofv3 --kernel-trace --stats run each (a record, not a threshold)'
             % (socket.gethostname(), name)]
    run([sys.executable, fg, '--mode', 'train', '-bt', 'Pix2Pix', '-bs', '32', '-mi', '2', '-smf', '1'], work, args.timeout)
    stamp = sorted(os.listdir(os.path.join(work, 'outputs')))[0]
    jobs = [('validation pass, Pix2Pix, batch 32, 192 x 192 (one call on 32 images)',
             [fg, '--mode', 'val', '-rf', stamp, '-bt', 'Pix2Pix', '-bs', '32', '-mt', '1'], work)]
    work_bg = tempfile.mkdtemp()
    run([sys.executable, bg, '--mode', 'train', '--image_size', '768', '--max_steps', '1', '--save_freq', '1', '--progress_freq', '0',
         '--summary_freq', '0'], work_bg, args.timeout)
    stamp_bg = sorted(os.listdir(os.path.join(work_bg, 'outputs')))[0]
    jobs.append(('Background test mode, 768 x 768 (eight synthetic scenes: one call on one image each, no mask)',
                 [bg, '--mode', 'test', '--resume_from', stamp_bg, '--image_size', '768', '--metrics', '1'], work_bg))
    for what, argv, cwd in jobs:
        cmd, line, rows = profiled(argv, cwd, args.timeout)
        lines += ['', what, '  ' + cmd.replace(ROOT + os.sep, ''), '  ' + line]
        for k in KERNELS:
            r = rows.get(k)
            lines.append('  %-26s %s' % (k, 'no row found' if r is None else
                                         'calls %s  average %.1f us  min %.1f us  max %.1f us  (%s %% of the kernel time of the run)'
                                         % (r['Calls'], float(r['AverageNs']) / 1e3, float(r['MinNs']) / 1e3, float(r['MaxNs']) / 1e3,
                                            r.get('Percentage', '?'))))
    shutil.rmtree(work, ignore_errors=True)
    shutil.rmtree(work_bg, ignore_errors=True)
    text = '\n'.join(lines) + '\n'
    print(text)
    if args.out:
        with open(args.out, 'w') as fp:
            fp.write(text)


if __name__ == '__main__':
    main()
