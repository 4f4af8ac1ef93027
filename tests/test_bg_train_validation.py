"""bg_colorization_main.py --val_freq / --val_records, the host side (no GPU): metrics.region_scores against a second float64
formulation, the flags up to the point where the held-out cache is built, and the text of a log/validation.jsonl line."""
import json
import os
import types

import numpy as np
import pytest
import torch
from PIL import Image


VOCAB = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'bg_aug', 'bg_vocab.txt')


# ---------------------------------------------------------------------------------------------------------------
# region scores
# ---------------------------------------------------------------------------------------------------------------
def _scores_from_pixels(conf, k):
    """The second formulation: the counts are expanded into one (label, prediction) pair per pixel and the scores are taken
    from boolean arrays over those pixels, in float64."""
    cells = np.asarray(conf, np.int64).reshape(-1, k * k + 1).sum(0)
    lab = np.repeat(np.arange(k * k) // k, cells[:-1])
    pred = np.repeat(np.arange(k * k) % k, cells[:-1])
    acc = float(np.mean((lab == pred).astype(np.float64))) if lab.size else None
    iou = []
    for c in range(k):
        union = np.count_nonzero((lab == c) | (pred == c))
        iou.append(np.count_nonzero((lab == c) & (pred == c)) / np.float64(union) if union else None)
    have = [v for v in iou if v is not None]
    return acc, iou, (float(np.mean(np.array(have, np.float64))) if have else None), int(cells[-1])


def _close(a, b):
    return (a is None and b is None) or (a is not None and b is not None and abs(a - b) <= 1e-12)


@pytest.mark.parametrize('case', ['k3', 'k4-samples', 'empty-class', 'ignored', 'nothing', 'k1'])
def test_region_scores_against_a_second_formulation(case):
    from sketchyscenecolorization_amd import metrics as M
    rng = np.random.RandomState(len(case))
    k = {'k4-samples': 4, 'k1': 1}.get(case, 3)
    conf = rng.randint(0, 500, (3 if case == 'k4-samples' else 1, k * k + 1)).astype(np.int64)
    conf[:, -1] = 0
    if case == 'empty-class':           # class 1 never labelled and never predicted
        m = conf[0, :9].reshape(3, 3)
        m[1, :] = 0
        m[:, 1] = 0
    if case == 'ignored':
        conf[0, -1] = 777
    if case == 'nothing':
        conf[:] = 0
        conf[0, -1] = 5
    got = M.region_scores(conf if case != 'k3' else conf[0])
    acc, iou, miou, ignored = _scores_from_pixels(conf, k)
    assert sorted(got) == ['accuracy', 'ignored', 'iou', 'miou']
    assert _close(got['accuracy'], acc) and _close(got['miou'], miou) and got['ignored'] == ignored, (got, acc, miou, ignored)
    assert len(got['iou']) == k and all(_close(g, w) for g, w in zip(got['iou'], iou)), (got['iou'], iou)
    if case == 'empty-class':
        assert got['iou'][1] is None and got['iou'][0] is not None and got['iou'][2] is not None
        assert _close(got['miou'], (got['iou'][0] + got['iou'][2]) / 2.0)
    if case == 'ignored':
        assert got['ignored'] == 777
        conf[0, -1] = 0             # ignored pixels are in no score
        clean = M.region_scores(conf)
        assert clean['accuracy'] == got['accuracy'] and clean['iou'] == got['iou'] and clean['ignored'] == 0
    if case == 'nothing':
        assert got == {'accuracy': None, 'iou': [None, None, None], 'miou': None, 'ignored': 5}
    assert json.loads(json.dumps(got)) == got


def test_region_scores_by_hand():
    from sketchyscenecolorization_amd import metrics as M
    #            pred 0  1  2
    conf = [5, 1, 0,     # label 0
            2, 6, 0,     # label 1
            0, 0, 0,     # label 2: never labelled, never predicted
            3]
    got = M.region_scores(conf)
    assert got['accuracy'] == 11 / 14 and got['iou'] == [5 / 8, 6 / 9, None] and got['miou'] == (5 / 8 + 6 / 9) / 2
    assert got['ignored'] == 3


# ---------------------------------------------------------------------------------------------------------------
# flags
# ---------------------------------------------------------------------------------------------------------------
class _Reached(Exception):
    pass


def _fake_trainer(fed):
    class FakeScope(object):
        name = 'x'

    class FakeStore(object):
        generator = discriminator = FakeScope()

        def parameter_count(self, scope):
            return 0

    class FakeTrainer(object):
        def __init__(self, **kw):
            self.store, self.global_step = FakeStore(), 0
            self.losses = types.SimpleNamespace(device=torch.device('cpu'))

        def train_step_u8(self, fg, bg, tok, lab):
            fed.append(tuple(fg.shape))
            self.global_step += 1

    return FakeTrainer


class _FakeEvent(object):
    def synchronize(self):
        pass

    def record(self):
        pass


def _patch_loop(monkeypatch, fed):
    from sketchyscenecolorization_amd import bg_colorization
    monkeypatch.setattr(bg_colorization, 'BGTrainer', _fake_trainer(fed))
    monkeypatch.setattr(torch.cuda, 'Event', _FakeEvent)
    monkeypatch.setattr(torch.Tensor, 'pin_memory', lambda self: self)


def _val_set(base, n=3, size=32, segment=True):
    """n flat scenes under <base>/{foreground,background,segment}/val and captions/val.json -> the vocabulary file."""
    for kind in ('foreground', 'background', 'segment'):
        os.makedirs(os.path.join(base, kind, 'val'))
    os.makedirs(os.path.join(base, 'captions'))
    recs = []
    for i in range(n):
        name = 'held_%d.png' % i
        Image.fromarray(np.full((size, size, 3), 40 * i, np.uint8), 'RGB').save(os.path.join(base, 'foreground', 'val', name))
        Image.fromarray(np.full((size, size, 3), 200 - 40 * i, np.uint8), 'RGB').save(os.path.join(base, 'background', 'val', name))
        if segment:
            Image.fromarray(np.full((size, size), 128, np.uint8), 'L').save(os.path.join(base, 'segment', 'val', name))
        recs.append({'fg_name': name, 'bg_name': name, 'color_text': 'the sky is blue and the ground is green'})
    with open(os.path.join(base, 'captions', 'val.json'), 'w') as fp:
        json.dump(recs, fp)
    return VOCAB


TRAIN = ['--mode', 'train', '--image_size', '32', '--max_steps', '3', '--save_freq', '0', '--progress_freq', '0',
         '--summary_freq', '0']


def test_flags_and_their_defaults(tmp_path, monkeypatch):
    import bg_colorization_main as bgcli
    args = bgcli.build_parser().parse_args([])
    assert args.val_freq == 0 and args.val_records == 0
    args = bgcli.build_parser().parse_args(['--val_freq', '500', '--val_records', '16'])
    assert args.val_freq == 500 and args.val_records == 16
    names = [f[0] for f in bgcli.FLAGS]
    assert 'val_freq' in names and 'val_records' in names
    built = []
    _patch_loop(monkeypatch, built)
    monkeypatch.chdir(tmp_path)
    os.makedirs(os.path.join('outputs', 'stamp', 'snapshot'))
    with pytest.raises(ValueError, match='val_freq'):
        bgcli.main(['--mode', 'test', '--resume_from', 'stamp', '--val_freq', '2'])
    with pytest.raises(ValueError, match='negative'):
        bgcli.main(TRAIN + ['--val_freq', '-1'])
    assert not built


def test_without_the_caption_file_training_goes_on(tmp_path, monkeypatch, capsys):
    """--val_freq 2 without captions/val.json: one line says so, no cache is built, no synthetic scenes stand in, and the
    training loop is fed exactly as with --val_freq 0."""
    import bg_colorization_main as bgcli
    from sketchyscenecolorization_amd import scene_cache
    monkeypatch.chdir(tmp_path)
    monkeypatch.setattr(scene_cache, 'SceneCache', lambda *a, **k: pytest.fail('a cache was built without a held-out set'))
    import random
    runs = []
    for vf in ('0', '2'):
        fed = []
        _patch_loop(monkeypatch, fed)
        random.seed(3)
        bgcli.main(TRAIN + ['--val_freq', vf])
        runs.append((fed, random.random(), capsys.readouterr().out))
    assert runs[0][0] == runs[1][0] == [(1, 32, 32, 3)] * 3
    assert runs[0][1] == runs[1][1], 'the draws of the run moved'
    assert 'not found' not in runs[0][2]
    assert runs[1][2].count(os.path.join('data', 'captions', 'val.json') + ' not found') == 1
    assert runs[1][2].count('## nImgs') == 1, 'a second Scenes was built without a caption file'
    stamp = os.listdir('outputs')[0]
    assert not os.path.exists(os.path.join('outputs', stamp, 'log', 'validation.jsonl'))


@pytest.mark.parametrize('records', [0, 2, 7])
def test_val_records_reaches_the_cache_as_keep(tmp_path, monkeypatch, records):
    import bg_colorization_main as bgcli
    from sketchyscenecolorization_amd import scene_cache
    vocab = _val_set(str(tmp_path / 'data'))
    seen = {}

    def fake_cache(scenes, device='cuda', keep=None, **kw):
        seen.update(scenes=scenes, device=device, keep=keep, kw=kw)
        raise _Reached()

    _patch_loop(monkeypatch, [])
    monkeypatch.setattr(scene_cache, 'SceneCache', fake_cache)
    monkeypatch.chdir(tmp_path)
    with pytest.raises(_Reached):
        bgcli.main(TRAIN + ['--val_freq', '2', '--val_records', str(records), '--vocab_file', vocab])
    assert seen['keep'] == range(min(records, 3) if records else 3)
    assert seen['scenes'].dirs['segment'] == os.path.join('data', 'segment', 'val') and len(seen['scenes'].records) == 3
    assert seen['device'] == torch.device('cpu')        # the trainer's device
    assert seen['kw']['beside'] == 0 and '--val_records' in seen['kw']['remedy']


def test_a_missing_segment_file_is_refused_by_name(tmp_path, monkeypatch):
    import bg_colorization_main as bgcli
    from sketchyscenecolorization_amd import scene_cache
    vocab = _val_set(str(tmp_path / 'data'))
    os.remove(str(tmp_path / 'data' / 'segment' / 'val' / 'held_1.png'))
    _patch_loop(monkeypatch, [])
    monkeypatch.setattr(scene_cache, 'SceneCache', lambda *a, **k: pytest.fail('the cache was built'))
    monkeypatch.chdir(tmp_path)
    with pytest.raises(ValueError, match=r'segment.val.held_1\.png'):
        bgcli.main(TRAIN + ['--val_freq', '2', '--vocab_file', vocab])
    # the record behind the cap is not looked at
    monkeypatch.setattr(scene_cache, 'SceneCache', lambda *a, **k: (_ for _ in ()).throw(_Reached()))
    with pytest.raises(_Reached):
        bgcli.main(TRAIN + ['--val_freq', '2', '--val_records', '1', '--vocab_file', vocab])


def test_both_caches_share_the_memory_limit(tmp_path, monkeypatch):
    """The held-out cache beside a training cache: refused when the two together exceed half of what was free before either was
    built, with --val_records in the message; alone, the same cache fits."""
    import bg_colorization_main as bgcli
    from sketchyscenecolorization_amd import bg_validation, scene_cache
    vocab = _val_set(str(tmp_path / 'data'))
    p = {'image_size': 32, 'text_len': 8, 'data_base_dir': str(tmp_path / 'data'), 'mode': 'train', 'vocab_size': 18,
         'vocab_file': vocab, 'val_freq': 2, 'val_records': 0, 'seg_classes': 3}
    scenes, keep = bg_validation.held_out_scenes(p, bgcli.Scenes)
    need = 3 * 32 * 32 * 7
    train = 10 * need
    # free now = what is left beside the training cache
    monkeypatch.setattr(torch.cuda, 'mem_get_info', lambda device=None: (2 * need + train - 2, 100 * need))
    real_empty = torch.empty
    monkeypatch.setattr(torch, 'empty', lambda *a, **k: pytest.fail('allocated although the caches do not fit'))
    with pytest.raises(RuntimeError, match='--val_records') as e:
        bg_validation.build_cache(scenes, keep, 'cuda', beside=train)
    assert str(need) in str(e.value) and str(train) in str(e.value)
    monkeypatch.setattr(torch.cuda, 'mem_get_info', lambda device=None: (2 * need + train, 100 * need))
    monkeypatch.setattr(torch, 'empty', lambda *a, **k: (_ for _ in ()).throw(_Reached()))
    with pytest.raises(_Reached):       # (need + train) * 2 <= free + train: it fits, and goes on to allocate
        scene_cache.SceneCache(scenes, 'cuda', keep=keep, beside=train)
    monkeypatch.setattr(torch, 'empty', real_empty)


# ---------------------------------------------------------------------------------------------------------------
# the line
# ---------------------------------------------------------------------------------------------------------------
def test_validation_line_is_sorted_and_stable():
    from sketchyscenecolorization_amd import bg_validation as BV, metrics as M
    rows = np.array([[300.0, 5000.0, 100.0, 250.5, 90.0], [0.0, 0.0, 100.0, 270.0, 90.0]])
    conf = np.array([[50, 10, 0, 5, 30, 0, 0, 0, 0, 5], [40, 0, 0, 0, 60, 0, 0, 0, 0, 0]], np.int64)
    line, summary = BV.validation_line(12, ['b_scene', 'a_scene'], rows, conf, 0.25)
    text = BV.dumps_line(line)
    assert text.endswith('\n') and text.count('\n') == 1
    assert text == json.dumps(json.loads(text), sort_keys=True) + '\n'
    back = json.loads(text)
    assert list(back) == ['all', 'groups', 'images', 'region', 'seconds', 'step']
    assert back['step'] == 12 and back['images'] == 2 and back['seconds'] == 0.25 and list(back['groups']) == ['all']
    assert back['all'] == back['groups']['all'] == M.summarise(['a', 'b'], ['all'] * 2, rows[::-1])['all']
    assert back['all']['psnr_infinite'] == 1 and back['all']['n'] == 2
    assert back['region'] == M.region_scores(conf) and back['region']['iou'][2] is None and back['region']['ignored'] == 5
    assert back['region']['accuracy'] == 180 / 195
    # the order the scenes came in does not show, and a second call writes the same text
    swapped, _ = BV.validation_line(12, ['a_scene', 'b_scene'], rows[::-1], conf[::-1], 0.25)
    assert BV.dumps_line(swapped) == text == BV.dumps_line(BV.validation_line(12, ['b_scene', 'a_scene'], rows, conf, 0.25)[0])
    shown = BV.printed_line(line, summary)
    assert shown.startswith('held-out pass at step 12: metrics: n 2') and 'region miou' in shown and '\n' not in shown
