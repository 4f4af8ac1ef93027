"""--color_metrics 1 of both command lines, end to end on the GPU, at the sizes of tests/test_gpu_preview.py: training with the
flag writes the snapshots and every other key of every log/validation.jsonl line of a run without it; the "color" key is what
the float64 oracle (tests/color_metrics_oracle.py) gives for the pass's own output, read by a hook around the scoring call; the
evaluation modes write the metrics.json and the PNG files of a run without the flag, and a color_metrics.json that is the oracle
on the PNG files read back from disk.

The integer-made scores (hist_intersection, colourfulness) must be equal; the three error means are compared under the bound of
tests/test_gpu_color_metrics.py divided by the pixel count: 4e-12 + |ref| * pixels * 2^-52 (a mean over images does not grow it)."""
import faulthandler
import json
import os
import random
import shutil

import numpy as np
import pytest
import torch

import color_metrics_oracle as CO
from test_gpu_metrics_cli import _cli, _rgb
from test_gpu_preview import BG_VOCAB, SIZE_BG, _without_seconds, _write_bg_scenes

pytestmark = pytest.mark.gpu

ERRORS = ('de76', 'dab', 'dl')


@pytest.fixture(autouse=True)
def _time_limit():
    """A test that hangs ends the process (with every thread's traceback) instead of holding the card."""
    faulthandler.dump_traceback_later(900, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


@pytest.fixture
def scratch(tmp_path):
    """The test's directory, emptied behind the test: a Background snapshot is 0.7 GB, and pytest keeps the directories of its
    last sessions."""
    yield tmp_path
    shutil.rmtree(str(tmp_path), ignore_errors=True)


def _assert_level(got, want, pixels, what):
    from sketchyscenecolorization_amd import metrics as M
    assert sorted(got) == sorted(want), (what, got, want)
    for k in want:
        if k not in ERRORS or want[k] is None:
            assert got[k] == want[k], (what, k, got[k], want[k])
        else:
            bound = 4e-12 + abs(want[k]) * pixels * 2.0 ** -52
            print('%s %s: %.17g, oracle %.17g, bound %.3e' % (what, k, got[k], want[k], bound))
            assert abs(got[k] - want[k]) <= bound, (what, k, got[k], want[k])
    assert set(M.COLOR_KEYS) <= set(want)


def _assert_summary(got, names, groups, a, b, masks, pixels, levels=('all', 'groups', 'images')):
    """A colour summary against the oracle on the uint8 images a[i], b[i] (and masks[i])."""
    from sketchyscenecolorization_amd import metrics as M
    rows = np.concatenate([CO.rows(a[i][None], b[i][None], None if masks is None or masks[i] is None else masks[i][None])[0]
                           for i in range(len(names))], 0)
    want = M.summarise_color(names, groups, rows)
    assert sorted(got) == sorted(levels)
    _assert_level(got['all'], want['all'], pixels, 'all')
    assert sorted(got['groups']) == sorted(want['groups'])
    for g in want['groups']:
        _assert_level(got['groups'][g], want['groups'][g], pixels, 'groups/' + g)
    if 'images' in levels:
        assert sorted(got['images']) == sorted(want['images'])
        for n in want['images']:
            _assert_level(got['images'][n], want['images'][n], pixels, 'images/' + n)
        # the scores from the pixels, not from the sums: colourfulness's host formula
        for i, n in enumerate(names):
            s = CO.scores(a[i][None], b[i][None], None if masks is None or masks[i] is None else masks[i][None])[0]
            for k in ('colourfulness', 'colourfulness_target'):
                assert abs(got['images'][n][k] - s[k]) <= 1e-9 * max(1.0, s[k]), (n, k)
    return want


def _same_snapshots(a_path, b_path, at_least):
    a, b = torch.load(a_path, map_location='cpu'), torch.load(b_path, map_location='cpu')
    assert list(a) == list(b) and len(a) > at_least
    assert not [k for k in a if not torch.equal(torch.as_tensor(a[k]), torch.as_tensor(b[k]))]


def _lines_without_color(path):
    lines = _without_seconds(path)
    return [{k: v for k, v in l.items() if k != 'color'} for l in lines], [l.get('color') for l in lines]


def test_foreground(scratch, monkeypatch):
    """Pix2Pix at 64 x 64 (-si 1), batch 2, 3 held-out records, 2 iterations, -rc device -vf 1, with -cm 0 and -cm 1; then
    --mode val -mt 1 on the run, with -cm 0 and -cm 1."""
    import obj_colorization_main as cli
    from test_gpu_train_validation import _write_records
    from sketchyscenecolorization_amd import hip as H, record_cache as rcache, train_validation as TV
    from sketchyscenecolorization_amd.obj_lib import main_procedure as mp, models_collection as models
    base = mp.RecordQueue

    class SeededQueue(base):        # (tests/train_validation_child.py: the command line seeds one GPU's queues from the system)
        def __init__(self, batch_size, small, which, data_base_dir='data', seed=None, record_cache=None):
            base.__init__(self, batch_size, small, which, data_base_dir=data_base_dir, seed=4000 + which, record_cache=record_cache)
    monkeypatch.setattr(mp, 'RecordQueue', SeededQueue)
    real = H.color_metrics_f32
    seen = []

    def spy(a, coff, b, *args, **kw):
        assert b.dim() == 4 and b.shape[1] == 3         # the decoded planar target
        seen.append((H.image_postprocess_u8(a, coff).cpu().numpy(),
                     H.image_postprocess_u8(b.permute(0, 2, 3, 1).contiguous(), 0).cpu().numpy()))
        return real(a, coff, b, *args, **kw)

    def run(tag, cm):
        cwd = scratch / tag
        cwd.mkdir()
        _write_records(str(cwd), 'train', 3, 11)
        _write_records(str(cwd), 'val', 3, 12)
        monkeypatch.chdir(str(cwd))
        models.reset_default_graph()
        torch.manual_seed(7)
        try:
            cli.main(['--mode', 'train', '-si', '1', '-bs', '2', '-mi', '2', '-smf', '2', '-swf', '100', '-bt', 'Pix2Pix', '-rc', 'device',
                      '-vf', '1', '-cm', str(cm)])
            torch.cuda.synchronize()
        finally:
            models.reset_default_graph()
        runs = sorted(os.listdir(str(cwd / 'outputs')))
        assert len(runs) == 1
        return os.path.join(str(cwd), 'outputs', runs[0])
    try:
        plain = run('cm0', 0)
        monkeypatch.setattr(H, 'color_metrics_f32', spy)
        scored = run('cm1', 1)
        monkeypatch.setattr(H, 'color_metrics_f32', real)
        _same_snapshots(os.path.join(plain, 'snapshot', 'model_1.ckpt-1'), os.path.join(scored, 'snapshot', 'model_1.ckpt-1'), 20)
        lines0, color0 = _lines_without_color(os.path.join(plain, 'log', 'validation.jsonl'))
        lines1, color1 = _lines_without_color(os.path.join(scored, 'log', 'validation.jsonl'))
        assert lines1 == lines0 and [l['step'] for l in lines1] == [0, 1] and color0 == [None, None]
        assert len(seen) == 4                       # two batches per pass: records (0, 1) and (2)
        cache = rcache.RecordCache(rcache.list_record_files(os.path.join(os.path.dirname(os.path.dirname(scored)), 'data', 'tfrecord', 'val')),
                                   64, device='cuda')
        names, groups = TV.record_names(cache)
        for i in range(2):
            out = np.concatenate([seen[2 * i][0], seen[2 * i + 1][0]], 0)
            target = np.concatenate([seen[2 * i][1], seen[2 * i + 1][1]], 0)
            assert out.shape == (3, 64, 64, 3)
            _assert_summary(color1[i], names, groups, out, target, None, 64 * 64, levels=('all', 'groups'))
        assert color1[0] != color1[1]           # the weights of the moment
    finally:
        rcache._MEMO.clear()
    # --mode val on the run: the held-out records through the validation queue
    cwd = os.path.dirname(os.path.dirname(scored))
    stamp = os.path.basename(scored)
    d = os.path.join(scored, 'validation_results', 'with_text')
    val = ['--mode', 'val', '-rf', stamp, '-bt', 'Pix2Pix', '-si', '1', '-bs', '2', '-mt', '1']
    text0 = _cli('obj_colorization_main', cwd, val)
    files0 = {f: open(os.path.join(d, f), 'rb').read() for f in sorted(os.listdir(d))}
    assert 'metrics.json' in files0 and 'color_metrics.json' not in files0 and 'colour:' not in text0
    for f in files0:
        os.remove(os.path.join(d, f))
    text1 = _cli('obj_colorization_main', cwd, val + ['-cm', '1'])
    files1 = {f: open(os.path.join(d, f), 'rb').read() for f in sorted(os.listdir(d))}
    assert sorted(files1) == sorted(list(files0) + ['color_metrics.json'])
    assert all(files1[f] == files0[f] for f in files0)         # metrics.json and every PNG
    assert 'colour: n 2' in text1
    stems = sorted(f[:-len('_output.png')] for f in files1 if f.endswith('_output.png'))
    assert len(stems) == 2          # (the validation queue drops the incomplete last batch)
    text = files1['color_metrics.json'].decode()
    from sketchyscenecolorization_amd import metrics as M
    got = json.loads(text)
    assert text == M.dumps(got)
    _assert_summary(got, stems, [s.rsplit('_', 1)[0] for s in stems], [_rgb(os.path.join(d, s + '_output.png')) for s in stems],
                    [_rgb(os.path.join(d, s + '_target.png')) for s in stems], None, 64 * 64)


def test_background(scratch, monkeypatch):
    """Background at 64 x 64, batch 1, 2 held-out scenes, 2 steps, --val_freq 1, with --color_metrics 0 and 1; then --mode test
    --metrics 1 on the run with --color_metrics 0 and 1, scored under the segment map's mask.  One snapshot per run, behind the
    last step (it holds what both steps did to every parameter and optimizer slot); the run without the flag is removed once it
    has been compared."""
    import bg_colorization_main as bgcli
    from sketchyscenecolorization_amd import hip as H, metrics as M
    real = H.color_metrics_bg_f32
    seen = []

    def spy(image, fg, target, mask=None, **kw):
        seen.append((H.bg_finish_u8(image, fg, mask).cpu().numpy()[0], target.cpu().numpy()[0], mask.cpu().numpy()[0]))
        return real(image, fg, target, mask, **kw)

    def run(tag, cm):
        cwd = scratch / tag
        cwd.mkdir()
        _write_bg_scenes(str(cwd / 'data'), 'train', 3, 0)
        _write_bg_scenes(str(cwd / 'data'), 'val', 2, 3)
        monkeypatch.chdir(str(cwd))
        random.seed(23)
        torch.manual_seed(23)
        bgcli.main(['--mode', 'train', '--image_size', str(SIZE_BG), '--max_steps', '2', '--save_freq', '2', '--progress_freq', '0',
                    '--summary_freq', '0', '--data_base_dir', 'data', '--vocab_file', BG_VOCAB, '--batch_size', '1', '--val_freq', '1',
                    '--color_metrics', str(cm)])
        torch.cuda.synchronize()
        runs = sorted(os.listdir(str(cwd / 'outputs')))
        assert len(runs) == 1
        return os.path.join(str(cwd), 'outputs', runs[0])
    plain = run('cm0', 0)
    monkeypatch.setattr(H, 'color_metrics_bg_f32', spy)
    scored = run('cm1', 1)
    monkeypatch.setattr(H, 'color_metrics_bg_f32', real)
    assert sorted(os.listdir(os.path.join(plain, 'snapshot'))) == sorted(os.listdir(os.path.join(scored, 'snapshot'))) == ['checkpoint', 'snapshot-2']
    _same_snapshots(os.path.join(plain, 'snapshot', 'snapshot-2'), os.path.join(scored, 'snapshot', 'snapshot-2'), 50)
    lines0, color0 = _lines_without_color(os.path.join(plain, 'log', 'validation.jsonl'))
    lines1, color1 = _lines_without_color(os.path.join(scored, 'log', 'validation.jsonl'))
    shutil.rmtree(str(scratch / 'cm0'))
    assert lines1 == lines0 and [l['step'] for l in lines1] == [1, 2] and color0 == [None, None] and len(seen) == 4
    names = ['val_scene_0', 'val_scene_1']
    for n in range(2):
        out, target, mask = ([seen[2 * n + r][k] for r in range(2)] for k in range(3))
        assert all(0 < (m != 0).sum() < m.size for m in mask)
        _assert_summary(color1[n], names, ['all', 'all'], out, target, mask, SIZE_BG * SIZE_BG, levels=('all', 'groups'))
    # --mode test on the run
    cwd = os.path.dirname(os.path.dirname(scored))
    stamp = os.path.basename(scored)
    _write_bg_scenes(os.path.join(cwd, 'data'), 'test', 2, 1)
    res = os.path.join(scored, 'results')
    test = ['--mode', 'test', '--resume_from', stamp, '--image_size', str(SIZE_BG), '--data_base_dir', 'data', '--vocab_file', BG_VOCAB,
            '--metrics', '1']
    text0 = _cli('bg_colorization_main', cwd, test)
    files0 = {f: open(os.path.join(res, f), 'rb').read() for f in sorted(os.listdir(res))}
    assert 'metrics.json' in files0 and 'color_metrics.json' not in files0 and 'colour:' not in text0
    for f in files0:
        os.remove(os.path.join(res, f))
    text1 = _cli('bg_colorization_main', cwd, test + ['--color_metrics', '1'])
    files1 = {f: open(os.path.join(res, f), 'rb').read() for f in sorted(os.listdir(res))}
    assert sorted(files1) == sorted(list(files0) + ['color_metrics.json']) and all(files1[f] == files0[f] for f in files0)
    assert 'colour: n 2' in text1
    stems = ['test_scene_0', 'test_scene_1']
    masks = [_rgb(os.path.join(cwd, 'data', 'segment', 'test', s + '.png'))[:, :, 0] for s in stems]
    text = files1['color_metrics.json'].decode()
    got = json.loads(text)
    assert text == M.dumps(got)
    want = _assert_summary(got, stems, ['all', 'all'], [_rgb(os.path.join(res, s + '_outputs.png')) for s in stems],
                           [_rgb(os.path.join(res, s + '_targets.png')) for s in stems], masks, SIZE_BG * SIZE_BG)
    # the mask matters: the pasted-back foreground (difference 0) is not counted
    unmasked = M.color_scores(CO.rows(_rgb(os.path.join(res, 'test_scene_0_outputs.png'))[None],
                                      _rgb(os.path.join(res, 'test_scene_0_targets.png'))[None])[0])[0]
    assert unmasked['de76'] != want['images']['test_scene_0']['de76']
