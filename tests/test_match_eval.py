"""The host side of the matcher's evaluation (sketchyscenecolorization_amd/match_eval.py, match_main.py --mode eval), without a
GPU: the metric functions fed integer histograms made in NumPy against what the reference's compute_mask_IU,
get_pred_instance_mask, compute_overlaps_masks and compute_ap returned (tests/golden/match_eval/, recorded by
tests/golden/make_match_eval_goldens.py) and against the mask-based restatement tests/match_eval_oracle.py; the label map;
augment_caption against the reference's captions; the refusals; the command line's checks."""
import json
import os
import random

import numpy as np
import pytest

import match_eval_oracle as O
from sketchyscenecolorization_amd import match_eval as E
from sketchyscenecolorization_amd import matching as M
from sketchyscenecolorization_amd import tf_checkpoint

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, 'tests', 'golden', 'match_eval')
VOCAB = os.path.join(ROOT, 'tests', 'golden', 'match', 'vocab.txt')
SMALL = dict(size=64, units=(1, 1, 1, 1), filters=(8, 16, 32, 64, 128))


def fixture():
    """-> (labels, boxes, masks, [caption dicts]) of metrics.npz."""
    with np.load(os.path.join(GOLD, 'metrics.npz')) as z:
        masks = [z['mask_%d' % k] for k in range(int(z['n']))]
        caps = [{k: z['c%d/%s' % (c, k)] for k in ('predicts', 'inst_indices', 'I', 'U', 'matched', 'scores', 'overlaps', 'ap')}
                for c in range(int(z['n_captions']))]
        return z['labels'], z['boxes'], masks, caps, float(z['mAP']), z['mAP_list'], z['thresholds']


def histograms(labels, boxes, masks, predicts=None):
    """What the two kernels and ssc_instance_occupancy give, in NumPy: area [256], H [N,256] (and P [256], counts [N,2])."""
    full = O.expand(boxes, masks, labels.shape[0])
    area = np.bincount(labels.reshape(-1), minlength=256).astype(np.int64)
    H = np.stack([np.bincount(labels[f != 0], minlength=256) for f in full]).astype(np.int64)
    if predicts is None:
        return area, H
    P = np.bincount(labels[predicts != 0], minlength=256).astype(np.int64)
    counts = np.array([[((predicts != 0) & (f != 0)).sum(), f.astype(np.int64).sum()] for f in full], np.int64)
    return area, H, P, counts


# ------------------------------------------------------------------ metrics against the reference's results
def test_fixture_holds_the_cases():
    labels, boxes, masks, caps, _, _, th = fixture()
    assert labels.shape == (40, 40) and np.array_equal(th, E.AP_THRESHOLDS) and th.dtype == np.float64
    assert any(len(c['matched']) == 0 for c in caps)                                            # no prediction
    assert any(len(c['scores']) > 1 and len(set(c['scores'].tolist())) < len(c['scores']) for c in caps)    # equal scores
    assert any(len(set(c['inst_indices'].tolist())) < len(c['inst_indices']) for c in caps)     # a duplicate: equal columns
    assert any(c['overlaps'].size and (c['overlaps'] == np.float32(0.5)).sum() >= 2 for c in caps)  # 0.5 with two instances
    ov = np.concatenate([c['overlaps'].reshape(-1) for c in caps])
    assert (ov == np.float32(0.7)).any() and (ov == np.float32(0.6)).any()                      # at a threshold
    assert np.float64(np.float32(0.7)) < th[4] and np.float64(np.float32(0.6)) > th[2]
    assert any((m == 2).any() for m in masks) and any((m == 3).any() for m in masks)
    assert any(c['predicts'].max() > 1 for c in caps)
    y1, x1, y2, x2 = boxes[0]
    Y1, X1, Y2, X2 = boxes[5]
    assert Y1 <= y1 and X1 <= x1 and Y2 >= y2 and X2 >= x2                                      # overlapping predicted instances


def test_metrics_from_histograms_equal_the_reference():
    labels, boxes, masks, caps, mAP32, mAP_list32, _ = fixture()
    tot = E.Totals(True)
    for c in caps:
        area, H, P, counts = histograms(labels, boxes, masks, c['predicts'])
        lab = E.caption_labels('s', c['inst_indices'].tolist(), 7, area)
        assert lab == [int(i) + 1 for i in c['inst_indices']]
        assert E.mask_iu(P, area, lab) == (int(c['I']), int(c['U']))
        matched, scores, ap = E.caption_ap(counts, H, area, lab)
        assert matched == c['matched'].tolist()
        assert scores.dtype == np.float64 and np.array_equal(scores, c['scores'])
        assert ap.dtype == np.float32 and np.array_equal(ap, c['ap'])
        if matched:
            ov = E.overlaps_f32(H[matched], area, lab)
            assert ov.dtype == np.float32 and np.array_equal(ov[E.descending(scores)], c['overlaps'])
        tot.add(int(c['I']), int(c['U']), ap)
    m, ml = tot.mean_ap()
    assert abs(m - mAP32) <= 1e-6 and np.abs(ml - mAP_list32).max() <= 1e-6
    assert (tot.cum_I, tot.cum_U) == (sum(int(c['I']) for c in caps), sum(int(c['U']) for c in caps))
    assert tot.correct == [sum(int(int(c['I']) / int(c['U']) >= t) for c in caps) for t in E.IOU_LEVELS]


def test_oracle_equals_the_reference_and_the_block():
    labels, boxes, masks, caps, mAP32, _, _ = fixture()
    full = O.expand(boxes, masks, 40)
    results, tot = [], E.Totals(True)
    for c in caps:
        r = O.caption(c['predicts'], labels, full, c['inst_indices'].tolist())
        assert (r['I'], r['U'], r['matched']) == (int(c['I']), int(c['U']), c['matched'].tolist())
        assert np.array_equal(r['scores'], c['scores']) and np.array_equal(r['ap'], c['ap'])
        results.append(r)
        tot.add(r['I'], r['U'], r['ap'])
    t = O.totals(results)
    assert abs(t['mAP'] - mAP32) <= 1e-6
    block = tot.block('snap/model-1')
    assert block == O.block('snap/model-1', t)
    lines = block.split('\n')
    assert lines[:3] == ['', 'snap/model-1', 'Segmentation evaluation (without DenseCRF):']
    assert [ln.split(' = ')[0] for ln in lines[3:11]] == ['precision@0.5', 'precision@0.6', 'precision@0.7', 'precision@0.8',
                                                          'precision@0.9', 'overall IoU', 'iou_threshold @[0.5:0.95],  mAP', 'mAP_list']
    assert lines[8] == 'overall IoU = %f' % (t['cum_I'] / t['cum_U'])
    assert 'mAP' not in _no_ap(results).block('x')
    rec = tot.record()
    assert rec['cum_I'] == t['cum_I'] and rec['precision']['0.5'] == t['precision'][0] and len(rec['mAP_list']) == 10


def _no_ap(results):
    tot = E.Totals(False)
    for r in results:
        tot.add(r['I'], r['U'])
    return tot


def test_average_precision_widens_the_overlap_before_it_compares():
    ov = np.array([[0.7]], np.float32)
    assert E.average_precision(np.array([0.9]), ov, np.float64(0.7)) == 0.0            # float32(0.7) < 0.7
    assert E.average_precision(np.array([0.9]), np.array([[0.6]], np.float32), AP_T(2)) == 1.0
    assert E.average_precision(np.array([0.9]), np.array([[0.5]], np.float32), 0.5) == 1.0


def AP_T(k):
    return E.AP_THRESHOLDS[k]


def test_descending_is_a_reversed_stable_sort():
    assert E.descending(np.array([1.0, 0.5, 1.0, 0.5])).tolist() == [2, 0, 3, 1]


# ------------------------------------------------------------------ the label map
@pytest.mark.parametrize('src,dst', [(30, 32), (60, 64)])
def test_label_map_zoom_equals_per_mask_zoom(src, dst):
    import scipy.ndimage
    rng = np.random.RandomState(src)
    gt = np.zeros((src, src), np.int32)
    for k in range(1, 9):
        y, x = rng.randint(0, src - 6, 2)
        gt[y:y + rng.randint(2, 12), x:x + rng.randint(2, 12)] = k * 3
    labels, ids = E.label_map(gt)
    zoomed = E.zoom_labels(labels, dst)
    assert zoomed.shape == (dst, dst) and zoomed.dtype == np.uint8
    stack = np.stack([(gt == i).astype(np.uint8) for i in ids], axis=2)                # load_mask's mask_set [H, W, nInst]
    scale = dst / src
    per_mask = np.array(scipy.ndimage.zoom(stack, zoom=[scale, scale, 1], order=0), dtype=np.uint8)
    assert per_mask.shape == (dst, dst, len(ids))
    for k in range(len(ids)):
        assert np.array_equal(zoomed == k + 1, per_mask[:, :, k] != 0), k
    assert np.array_equal(zoomed == 0, per_mask.sum(axis=2) == 0)
    assert E.zoom_labels(zoomed, dst) is not None and np.array_equal(E.zoom_labels(zoomed, dst), zoomed)


def test_compaction_follows_ascending_ids_with_gaps():
    gt = np.zeros((6, 6), np.uint8)
    gt[0, 0], gt[1, :3], gt[3, 3], gt[5, 5] = 101, 7, 40, 9
    labels, ids = E.label_map(gt)
    assert ids == [7, 9, 40, 101]
    assert labels[1, 0] == 1 and labels[5, 5] == 2 and labels[3, 3] == 3 and labels[0, 0] == 4 and labels[2, 2] == 0
    assert labels.dtype == np.uint8 and int((labels != 0).sum()) == 6


def test_label_map_refusals():
    many = np.arange(1, 257, dtype=np.int32).reshape(16, 16)
    with pytest.raises(ValueError, match='255'):
        E.label_map(many)
    assert len(E.label_map(np.arange(0, 256, dtype=np.int32).reshape(16, 16))[1]) == 255
    with pytest.raises(ValueError):
        E.label_map(np.zeros((4, 4), np.float32))
    with pytest.raises(ValueError):
        E.label_map(np.zeros((4, 4, 2), np.uint8))
    with pytest.raises(ValueError):
        E.zoom_labels(np.zeros((4, 6), np.uint8), 8)


def test_caption_labels_refusals():
    area = np.zeros(256, np.int64)
    area[[0, 1, 3]] = [10, 5, 2]
    assert E.caption_labels('77', [0, 2, 0], 3, area) == [1, 3, 1]
    with pytest.raises(ValueError, match='scene 77.*no pixel left'):
        E.caption_labels('77', [1], 3, area)
    with pytest.raises(ValueError, match='scene 77'):
        E.caption_labels('77', [3], 3, area)
    with pytest.raises(ValueError, match='scene 77'):
        E.caption_labels('77', [-1], 3, area)


# ------------------------------------------------------------------ files
def test_ground_truth_and_predictions_load(tmp_path):
    O.write_split(str(tmp_path))
    gt = E.load_ground_truth(str(tmp_path / 'data'), 'val', '11', 64)
    assert gt['sketch'].shape == (64, 64, 3) and gt['sketch'].dtype == np.uint8 and gt['n_inst'] == 5
    assert gt['labels'].shape == (64, 64) and set(np.unique(gt['labels']).tolist()) == {0, 1, 2, 3, 4, 5}
    pred = E.load_pred_instances(str(tmp_path / 'seg'), 'val', '11', 64)
    assert len(pred['masks']) == 7 and pred['boxes'].dtype == np.int32 and pred['offsets'].dtype == np.int64
    assert len(pred['buf']) == sum(m.size for m in pred['masks'])
    scenes = E.read_captions(str(tmp_path / 'captions'), 'val')
    assert [k for k, _ in scenes] == ['11', '12'] and scenes[0][1][2] == ('all the people near the bus', [2, 4, 2])
    with pytest.raises(ValueError, match='scene 13'):
        E.load_ground_truth(str(tmp_path / 'data'), 'val', '13', 64)
    with pytest.raises(ValueError, match='scene 13'):
        E.load_pred_instances(str(tmp_path / 'seg'), 'val', '13', 64)
    with pytest.raises(ValueError):
        E.read_captions(str(tmp_path / 'captions'), 'test')
    with pytest.raises(ValueError, match='scene 11'):            # a box that leaves a 32 x 32 image
        E.load_pred_instances(str(tmp_path / 'seg'), 'val', '11', 32)


# ------------------------------------------------------------------ captions
def test_augment_caption_equals_the_reference():
    cases = json.load(open(os.path.join(GOLD, 'augment.json')))
    assert len(cases) >= 6
    seen = set()
    for caption, want in cases.items():
        assert len(want) == 20
        got = [E.augment_caption(caption, random.Random(seed)) for seed in range(20)]
        assert got == want, caption
        seen.add(E.caption_category(caption))
    cats = {c for c, _ in seen}
    assert {'person', 'bus', 'house', 'bird', 'butterfly', 'dog'} <= cats and any(s for _, s in seen)
    with pytest.raises(ValueError):
        E.augment_caption('the thing on the left', random.Random(0))
    # the module-level generator is consumed the same way
    random.seed(3)
    assert E.augment_caption('the person on the left', random) == cases['the person on the left'][3]


# ------------------------------------------------------------------ the command line
def test_eval_mode_checks_its_arguments_before_anything_is_read(tmp_path):
    import match_main
    cfg = M.MatchConfig(**SMALL)
    prefix = str(tmp_path / 'model-1')
    tf_checkpoint.write_checkpoint(prefix, M.random_variables(cfg, 0))
    flags = O.write_split(str(tmp_path))
    results = str(tmp_path / 'results')
    good = ['--mode', 'eval', '--snapshot', prefix, '--vocab_file', VOCAB, '--scene_size', '64', '--vocab_size', '76', '--text_len', '15',
            '--mask_ap', '1', '--max_scenes', '0', '--eval_result_root', results] + flags
    args = match_main.build_parser().parse_args(good)
    cfg2, pre, vocab, scenes = match_main.checked_eval_arguments(args)
    assert (cfg2.size, pre, len(vocab), len(scenes)) == (64, prefix, 76, 2)
    assert len(match_main.checked_eval_arguments(match_main.build_parser().parse_args(good + ['--max_scenes', '1']))[3]) == 1

    def bad(extra=(), **change):
        argv = list(good) + list(extra)
        for k, val in change.items():
            i = argv.index('--' + k)
            if val is None:
                del argv[i:i + 2]
            else:
                argv[i + 1] = val
        with pytest.raises(ValueError):
            match_main.main(argv)
        assert not os.path.exists(results)
    bad(snapshot=None)
    bad(snapshot=str(tmp_path / 'nothing'))
    bad(mode='train')
    bad(dataset='train')
    bad(dataset='test')                                         # no caption file of that split
    bad(mask_ap='2')
    bad(max_scenes='-1')
    bad(scene_size='72')
    bad(text_len='0')
    bad(vocab_size='75')
    bad(vocab_file=str(tmp_path / 'no_vocab.txt'))
    bad(data_base_dir=str(tmp_path / 'no_data'))
    bad(captions_base_dir=str(tmp_path / 'no_captions'))
    bad(seg_data_dir=str(tmp_path / 'no_seg'))
    bad(eval_result_root='')
    os.remove(str(tmp_path / 'seg' / 'val' / 'seg_data' / '12_datas.npz'))
    bad()                                                       # the second scene's file is missed before the first is scored
    match_main.checked_eval_arguments(match_main.build_parser().parse_args(good + ['--max_scenes', '1']))


def test_augment_seed_needs_a_category_in_every_caption(tmp_path):
    import match_main
    cfg = M.MatchConfig(**SMALL)
    prefix = str(tmp_path / 'model-1')
    tf_checkpoint.write_checkpoint(prefix, M.random_variables(cfg, 0))
    flags = O.write_split(str(tmp_path))
    path = str(tmp_path / 'captions' / 'sentence_instance_val.json')
    data = json.load(open(path))
    data[1]['sen_instIdx_map']['the thing on the left'] = [0]
    json.dump(data, open(path, 'w'))
    good = ['--mode', 'eval', '--snapshot', prefix, '--vocab_file', VOCAB, '--scene_size', '64'] + flags
    match_main.checked_eval_arguments(match_main.build_parser().parse_args(good))
    with pytest.raises(ValueError, match='category'):
        match_main.checked_eval_arguments(match_main.build_parser().parse_args(good + ['--augment_seed', '4']))


def test_mode_absent_parses_as_before():
    import match_main
    d = match_main.build_parser().parse_args([])
    assert d.mode == 'match' and d.augment_seed is None and d.mask_ap == 1 and d.max_scenes == 0 and d.dataset == 'val'
    assert d.eval_result_root == 'outputs/eval_results'
    assert (d.vocab_file, d.vocab_size, d.text_len, d.scene_dir, d.scene_size, d.results_dir, d.snapshot, d.image_id, d.instruction) == \
        ('data/match_vocab.txt', 76, 15, 'examples', 768, 'outputs/match_results', '', None, '')
    with pytest.raises(ValueError, match='--snapshot'):         # the present behaviour: the match mode's own check
        match_main.main([])
