"""--metrics 1 of both command lines, end to end on the GPU: the PNG files are those of --metrics 0 byte for byte, metrics.json
exists only with the flag, and every entry of it is what the float64 oracle (tests/metrics_oracle.py) gives for the PNG pair
read back from disk -- mae exactly, psnr to 1e-12 relative, ssim to 1e-9 (the bound of tests/test_gpu_image_metrics.py).

Every GPU command is a fresh child process under its own time limit."""
import faulthandler
import glob
import json
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest
from PIL import Image

import metrics_oracle as MO

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIX = os.path.join(ROOT, 'tests', 'golden', 'bg_aug')
CHILD_LIMIT = 180       # seconds a command-line child may take (start-up of a fresh process included)
# The validation queue seeds its dequantisation noise (input_pipeline.py, < 1/256 on the target images) from the operating
# system's entropy when it is given no seed: the child pins that, and torch's generator, so that two runs can be compared.
PIN = ('import random, sys, torch\n'
       'class _Pinned(random.Random):\n'
       '    def __init__(self, x=None):\n'
       '        super().__init__(20241 if x is None else x)\n'
       'random.Random = _Pinned\n'
       'random.seed(%d); torch.manual_seed(%d); sys.path.insert(0, %r)\n')


@pytest.fixture(autouse=True)
def _time_limit():
    """A test that hangs ends the process (with every thread's traceback) instead of holding the card."""
    faulthandler.dump_traceback_later(900, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


def _cli(module, cwd, argv, seed=5):
    code = PIN % (seed, seed, ROOT) + 'import %s as m; m.main(%r)' % (module, list(argv))
    os.makedirs(str(cwd), exist_ok=True)
    r = subprocess.run([sys.executable, '-c', code], cwd=str(cwd), stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       universal_newlines=True, timeout=CHILD_LIMIT)
    assert r.returncode == 0, r.stdout[-4000:]
    return r.stdout


def _pngs(d):
    out = {}
    for f in sorted(glob.glob(os.path.join(d, '*.png'))):
        with open(f, 'rb') as fp:
            out[os.path.basename(f)] = fp.read()
    return out


def _rgb(path):
    return np.array(Image.open(path).convert('RGB'), dtype=np.uint8)


def _close(got, want, tol, relative, what):
    if want is None or got is None:
        assert got is None and want is None, (what, got, want)
        return
    print('%s: %.17g, oracle %.17g' % (what, got, want))
    assert abs(got - want) <= (tol * abs(want) if relative else tol), (what, got, want)


def _assert_is_the_oracle(path, pairs, groups, masks=None):
    """metrics.json at path against the oracle on the PNG pairs {name: (output file, target file)}."""
    from sketchyscenecolorization_amd import metrics as M
    with open(path) as fp:
        text = fp.read()
    got = json.loads(text)
    names = sorted(pairs)
    win = M.ssim_window()
    rows = np.concatenate([MO.rows(_rgb(pairs[n][0])[None], _rgb(pairs[n][1])[None], win,
                                   None if masks is None or masks[n] is None else masks[n][None]) for n in names], 0)
    want = M.summarise(names, [groups[n] for n in names], rows)
    assert text == M.dumps(got), 'metrics.json is not in its canonical form (sorted keys)'
    assert sorted(got) == ['all', 'groups', 'images'] and sorted(got['images']) == names
    assert sorted(got['groups']) == sorted(want['groups'])
    entries = [('images/' + n, got['images'][n], want['images'][n]) for n in names]
    entries += [('groups/' + g, got['groups'][g], want['groups'][g]) for g in want['groups']] + [('all', got['all'], want['all'])]
    for what, g, w in entries:
        assert sorted(g) == sorted(w), (what, g, w)
        for k in ('n', 'psnr_infinite'):
            if k in w:
                assert g[k] == w[k], (what, k)
        assert g['mae'] == w['mae'], (what, g['mae'], w['mae'])         # integer sums divided alike: exact
        _close(g['psnr'], w['psnr'], 1e-12, True, what + ' psnr')
        _close(g['ssim'], w['ssim'], 1e-9, False, what + ' ssim')
    return got


def test_foreground_validation_metrics(tmp_path):
    """A two-iteration Pix2Pix run at 64 x 64, then --mode val with -mt 0 and -mt 1: over the synthetic batch, and over a
    two-record data/tfrecord/val."""
    from test_gpu_record_cache import _write_records
    cwd = tmp_path / 'run'
    _cli('obj_colorization_main', cwd, ['--mode', 'train', '-bt', 'Pix2Pix', '-si', '1', '-bs', '2', '-mi', '2', '-smf', '1',
                                        '-swf', '1'])
    stamp = sorted(os.listdir(str(cwd / 'outputs')))[0]
    res = str(cwd / 'outputs' / stamp / 'validation_results')
    val = ['--mode', 'val', '-rf', stamp, '-bt', 'Pix2Pix', '-si', '1', '-bs', '2']
    for source in ('synthetic', 'records'):
        if source == 'records':
            _write_records(str(cwd), 2, 3)
            os.rename(str(cwd / 'data' / 'tfrecord' / 'train'), str(cwd / 'data' / 'tfrecord' / 'val'))
        text0 = _cli('obj_colorization_main', cwd, val + ['-mt', '0'])
        d = os.path.join(res, 'with_text')
        plain = _pngs(d)
        assert len(plain) == 6 and not os.path.exists(os.path.join(d, 'metrics.json')) and 'metrics:' not in text0
        shutil.rmtree(res)
        text1 = _cli('obj_colorization_main', cwd, val + ['-mt', '1'])
        scored = _pngs(d)
        assert sorted(scored) == sorted(plain) and all(scored[k] == plain[k] for k in plain), source
        stems = sorted(f[:-len('_output.png')] for f in scored if f.endswith('_output.png'))
        assert len(stems) == 2 and (source == 'synthetic' or stems == ['car_n0', 'car_n1'])
        pairs = {s: (os.path.join(d, s + '_output.png'), os.path.join(d, s + '_target.png')) for s in stems}
        got = _assert_is_the_oracle(os.path.join(d, 'metrics.json'), pairs, {s: s.rsplit('_', 1)[0] for s in stems})
        assert got['all']['n'] == 2 and got['all']['ssim'] is not None and 'metrics: n 2' in text1
        shutil.rmtree(res)


def _bg_dataset(base, size):
    """The two scenes of tests/golden/bg_aug (16 x 16 and 12 x 20) as a test-mode dataset of size x size files: each png cut to
    its top-left 12 x 12 corner, as tests/test_bg_scene_cache.py cuts them, then enlarged without interpolation (the segment
    maps keep their three values).  scene_b is paired with a recoloured background."""
    for kind in ('foreground', 'background', 'segment'):
        os.makedirs(os.path.join(base, kind, 'test'))
        for name in sorted(os.listdir(os.path.join(FIX, kind, 'train'))):
            im = Image.open(os.path.join(FIX, kind, 'train', name))
            im.crop((0, 0, 12, 12)).resize((size, size), resample=Image.NEAREST).save(os.path.join(base, kind, 'test', name))
    os.makedirs(os.path.join(base, 'captions'))
    with open(os.path.join(FIX, 'captions', 'train.json')) as fp:
        recs = json.load(fp)
    keep = [[r for r in recs if r['bg_name'] == n][0] for n in ('scene_a.png', 'scene_b_1.png')]
    assert [r['fg_name'] for r in keep] == ['scene_a.png', 'scene_b.png']
    with open(os.path.join(base, 'captions', 'test.json'), 'w') as fp:
        json.dump(keep, fp)
    return keep


def test_background_test_mode_metrics(tmp_path):
    """Two training steps at 64 x 64, then --mode test with --metrics 0 and 1: on the synthetic scenes (no segment file: no
    mask) and on the two fixture scenes (the segment map's red channel is the mask: the pasted-back foreground is not
    counted)."""
    size = 64
    cwd = tmp_path / 'run'
    _cli('bg_colorization_main', cwd, ['--mode', 'train', '--image_size', str(size), '--max_steps', '2', '--save_freq', '1',
                                       '--progress_freq', '0', '--summary_freq', '0'])
    stamp = sorted(os.listdir(str(cwd / 'outputs')))[0]
    res = str(cwd / 'outputs' / stamp / 'results')
    base = str(tmp_path / 'data')
    recs = _bg_dataset(base, size)
    test = ['--mode', 'test', '--resume_from', stamp, '--image_size', str(size)]
    for source in ('synthetic', 'files'):
        argv = test + (['--data_base_dir', base, '--vocab_file', os.path.join(FIX, 'bg_vocab.txt')] if source == 'files' else [])
        text0 = _cli('bg_colorization_main', cwd, argv + ['--metrics', '0'])
        plain = _pngs(res)
        assert len(plain) == (6 if source == 'files' else 24) and 'metrics:' not in text0
        assert not os.path.exists(os.path.join(res, 'metrics.json'))
        shutil.rmtree(res)
        text1 = _cli('bg_colorization_main', cwd, argv + ['--metrics', '1'])
        scored = _pngs(res)
        assert sorted(scored) == sorted(plain) and all(scored[k] == plain[k] for k in plain), source
        stems = sorted(f[:-len('_outputs.png')] for f in scored if f.endswith('_outputs.png'))
        pairs = {s: (os.path.join(res, s + '_outputs.png'), os.path.join(res, s + '_targets.png')) for s in stems}
        masks = None
        if source == 'files':
            assert stems == ['scene_a', 'scene_b_1']
            masks = {r['bg_name'][:-4]: _rgb(os.path.join(base, 'segment', 'test', r['fg_name']))[:, :, 0] for r in recs}
            assert all(0 < (m != 0).sum() < m.size for m in masks.values())
        got = _assert_is_the_oracle(os.path.join(res, 'metrics.json'), pairs, {s: 'all' for s in stems}, masks)
        assert list(got['groups']) == ['all'] and got['groups']['all'] == got['all'] and got['all']['n'] == len(stems)
        assert 'metrics: n %d' % len(stems) in text1
        if source == 'files':       # the mask matters: without it the pasted-back pixels (difference 0) would be counted too
            from sketchyscenecolorization_amd import metrics as M
            for s in stems:
                a, b = _rgb(pairs[s][0]), _rgb(pairs[s][1])
                unmasked = M.scores(MO.rows(a[None], b[None], M.ssim_window()))[0]
                assert unmasked['mae'] != got['images'][s]['mae']
        shutil.rmtree(res)
