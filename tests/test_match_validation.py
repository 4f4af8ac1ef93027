"""The host side of scoring val while the matcher trains (sketchyscenecolorization_amd/match_validation.py, match_main.py --mode
train --val_freq / --val_scenes), without a GPU: the flags and the files they ask for, the record of a pass from rows of
(I, P, A, live, loss) against match_eval.Totals on the I and U of tests/golden/match_eval/, and the NumPy restatement of
ssc_match_score (tests/match_score_oracle.py) on that golden scene."""
import json
import os

import numpy as np
import pytest

import match_eval_oracle as EO
import match_score_oracle as SO
from sketchyscenecolorization_amd import match_eval, match_validation as V, matching as M, tf_checkpoint

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, 'tests', 'golden', 'match_eval')
VOCAB = os.path.join(ROOT, 'tests', 'golden', 'match', 'vocab.txt')
SMALL = dict(size=64, units=(1, 1, 1, 1), filters=(8, 16, 32, 64, 128))


def golden():
    with np.load(os.path.join(GOLD, 'metrics.npz')) as z:
        caps = [{k: z['c%d/%s' % (c, k)] for k in ('predicts', 'inst_indices', 'I', 'U')} for c in range(int(z['n_captions']))]
        return z['labels'], caps


# ------------------------------------------------------------------ the flags
def test_validation_flags_and_the_files_they_ask_for(tmp_path):
    import match_main
    cfg = M.MatchConfig(**SMALL)
    backbone = str(tmp_path / 'backbone-1')
    tf_checkpoint.write_checkpoint(backbone, {k: v for k, v in M.random_variables(cfg, 0).items() if k.startswith('ResNet/')})
    flags = EO.write_split(str(tmp_path), 'train')[:4]
    snaps, logs = str(tmp_path / 'snapshots'), str(tmp_path / 'log')
    good = ['--mode', 'train', '--backbone_snapshot', backbone, '--vocab_file', VOCAB, '--scene_size', '64', '--snapshot_root', snaps,
            '--log_root', logs, '--max_iteration', '4'] + flags
    parse = lambda extra: match_main.build_parser().parse_args(good + extra)

    def bad(extra, match):
        with pytest.raises(ValueError, match=match):
            match_main.main(good + extra)
        assert not os.path.exists(snaps) and not os.path.exists(logs)
    # there is no val split yet: F = 0 does not look for one, F > 0 refuses before any weight is read
    assert not os.path.exists(str(tmp_path / 'captions' / 'sentence_instance_val.json'))
    match_main.checked_train_arguments(parse([]))
    match_main.checked_train_arguments(parse(['--val_freq', '0', '--val_scenes', '1']))
    assert match_main.validation_scenes(parse([])) is None
    bad(['--val_freq', '-1'], 'val_freq')
    bad(['--val_scenes', '-1'], 'val_scenes')
    bad(['--val_freq', '2'], 'sentence_instance_val.json')
    EO.write_split(str(tmp_path), 'val')
    match_main.checked_train_arguments(parse(['--val_freq', '2']))
    scenes = match_main.validation_scenes(parse(['--val_freq', '2']))
    assert [s[0] for s in scenes] == ['11', '12'] and sum(len(p) for _i, p in scenes) == 6
    one = match_main.validation_scenes(parse(['--val_freq', '2', '--val_scenes', '1']))
    assert [s[0] for s in one] == ['11'] and len(one[0][1]) == 3
    # the segmentation output is not read: the pass computes no mask AP
    match_main.checked_train_arguments(parse(['--val_freq', '2', '--seg_data_dir', str(tmp_path / 'no_seg')]))
    # a missing ground-truth file of a scene that is scored, and only of such a scene
    os.remove(str(tmp_path / 'data' / 'val' / 'INSTANCE_GT' / 'sample_12_instance.mat'))
    bad(['--val_freq', '2'], 'sample_12_instance')
    match_main.checked_train_arguments(parse(['--val_freq', '2', '--val_scenes', '1']))
    match_main.checked_train_arguments(parse([]))
    # a caption without a word
    path = str(tmp_path / 'captions' / 'sentence_instance_val.json')
    data = json.load(open(path))
    data[0]['sen_instIdx_map'][' - '] = [0]
    json.dump(data, open(path, 'w'))
    bad(['--val_freq', '2', '--val_scenes', '1'], 'holds no word')
    json.dump([], open(path, 'w'))
    bad(['--val_freq', '2'], 'no scene')


# ------------------------------------------------------------------ the record
def test_record_is_totals_arithmetic_on_the_golden_counts():
    labels, caps = golden()
    area = np.bincount(labels.reshape(-1), minlength=256)
    totals = match_eval.Totals(mask_ap=False)
    rows = []
    for k, c in enumerate(caps):
        I, U = int(c['I']), int(c['U'])
        totals.add(I, U)
        A = int(area[sorted(set(int(i) + 1 for i in c['inst_indices']))].sum())
        P = U - A + I                                   # U = P + A - I
        assert P == int((c['predicts'] != 0).sum())
        rows.append((I, P, A, 100 + k, 0.5 * (k + 1)))
    rec = V.validation_record(4000, 1, rows, 1.25)
    assert rec['iter'] == 4000 and rec['scenes'] == 1 and rec['captions'] == len(caps) and rec['seconds'] == 1.25
    assert rec['overall_iou'] == totals.overall_iou() == totals.cum_I / totals.cum_U
    assert rec['precision'] == {str(t): p for t, p in zip(match_eval.IOU_LEVELS, totals.precision())}
    assert list(rec['precision']) == ['0.5', '0.6', '0.7', '0.8', '0.9']
    assert rec['precision'] == totals.record()['precision'] and rec['overall_iou'] == totals.record()['overall_IoU']
    assert rec['live_pixels'] == sum(100 + k for k in range(len(caps)))
    assert rec['class_loss_mean'] == sum(0.5 * (k + 1) for k in range(len(caps))) / len(caps)
    assert set(rec) == {'iter', 'scenes', 'captions', 'overall_iou', 'precision', 'class_loss_mean', 'live_pixels', 'seconds'}
    assert json.loads(json.dumps(rec)) == rec
    line = V.validation_line(rec)
    assert line == 'val: iter = 4000, overall IoU = %f, precision@0.5 = %f, loss = %f' % (rec['overall_iou'], rec['precision']['0.5'],
                                                                                         rec['class_loss_mean'])
    # I / U >= t is decided in float64, at the threshold itself too
    rec = V.validation_record(1, 1, [(5, 10, 5, 0, 0.0), (3, 5, 3, 0, 0.0)], 0.0)          # 5 / 10 and 3 / 5
    assert rec['precision'] == {'0.5': 1.0, '0.6': 0.5, '0.7': 0.0, '0.8': 0.0, '0.9': 0.0} and rec['overall_iou'] == 8 / 15
    with pytest.raises(ValueError):
        V.validation_record(1, 0, [], 0.0)


# ------------------------------------------------------------------ the oracle of the kernel
@pytest.mark.parametrize('dtype', [np.float64, np.float32])
def test_score_oracle_gives_the_golden_I_and_U(dtype):
    """The fixture's predicts as a +-1 map at full resolution (h = S: the up-sampling is the identity), every pixel a stroke."""
    labels, caps = golden()
    S = labels.shape[0]
    sketch = np.zeros((S, S, 3), np.uint8)
    for c in caps:
        pred = np.where(c['predicts'] != 0, 1.0, -1.0).astype(np.float32)
        lut = np.zeros(256, np.uint8)
        lut[[int(i) + 1 for i in c['inst_indices']]] = 1
        got = SO.score(pred, sketch, labels, lut, dtype)
        assert np.array_equal(got['up'], pred) and np.array_equal(got['predicts'], (c['predicts'] != 0).astype(np.uint8))
        assert (got['I'], got['U']) == (int(c['I']), int(c['U']))
        assert got['live'] == S * S and got['P'] == int((c['predicts'] != 0).sum())
        # u = +-1: a hit costs log1p(exp(-1)), a miss 1 + log1p(exp(-1))
        z = lut[labels] != 0
        misses = int(((pred > 0) != z).sum())
        assert got['loss'] == pytest.approx(S * S * np.log1p(np.exp(-1.0)) + misses, rel=1e-6)


def test_score_oracle_strokes_and_threshold():
    S = 8
    labels = np.zeros((S, S), np.uint8)
    labels[:, 4:] = 255
    lut = np.zeros(256, np.uint8)
    lut[255] = 3
    sketch = np.full((S, S, 3), 255, np.uint8)
    sketch[0, :, 0] = 0
    sketch[1, :, 0] = 104
    sketch[2, :, 0] = 105
    sketch[3, :, 0] = 254
    sketch[:, :, 1:] = 7                                # only the first byte decides
    for value, on in ((0.0, 0), (5e-10, 0), (-5e-10, 0), (1e-9, 1), (2.0, 1)):
        pred = np.full((2, 2), value, np.float32)
        for dt in (np.float64, np.float32):
            got = SO.score(pred, sketch, labels, lut, dt)
            assert (got['P'], got['I'], got['A'], got['live']) == (32 * on, 16 * on, 32, 16), (value, dt)
    blank = SO.score(np.full((2, 2), 2.0, np.float32), np.full((S, S, 3), 255, np.uint8), labels, np.zeros(256, np.uint8))
    assert (blank['I'], blank['P'], blank['A'], blank['live'], blank['loss'], blank['U']) == (0, 0, 0, 0, 0.0, 0)
