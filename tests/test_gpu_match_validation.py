"""Scoring val while the matcher trains, on the device (csrc/match_val.hip, sketchyscenecolorization_amd/match_validation.py,
match_main.py --mode train --val_freq): hip.match_score (ssc_match_score) against the NumPy restatement
tests/match_score_oracle.py, against the two-kernel path hip.match_finish -> hip.label_hist_u8 exactly, and against
ssc_match_loss_grad's own loss; then the command line in fresh processes: the trajectory with --val_freq is that without it, and
the lines of match_validation.jsonl are what --mode eval gives for the snapshots of those iterations.

Bounds.  The four counts are integers: compared exactly with the two-kernel path (the up-sampled value comes from one inline
function in both).  Against the float64 oracle a pixel whose float64 value lies within 16 * 2^-24 * max|pred| of the threshold
(three fp32 interpolations, each a few roundings of a corner) may fall on either side; every other pixel must agree.  The loss
against float64: 1e-5 relative, the bound tests/test_gpu_match_train.py::test_match_loss_grad holds the same fp32 terms to.  The
loss against ssc_match_loss_grad's: the same fp32 terms added in double in two orders, n_live * 2^-52 * sum |term|."""
import faulthandler
import json
import os

import numpy as np
import pytest
import torch

import match_eval_oracle as EO
import match_score_oracle as SO
from kernel_check import rc
from test_gpu_match_cache import _child, _second_scene_gets_other_labels, _snapshot_bytes

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VOCAB = os.path.join(ROOT, 'tests', 'golden', 'match', 'vocab.txt')
SMALL = dict(size=64, units=(1, 1, 1, 1), filters=(8, 16, 32, 64, 128))
NARROW = dict(v_emb=24, w_emb=24, w_rnn=40, m_rnn=20)
BYTES = np.array([0, 104, 105, 254, 255], np.uint8)


@pytest.fixture(autouse=True)
def _time_limit():
    """A test that hangs on the device ends the process (with every thread's traceback) instead of holding the card."""
    faulthandler.dump_traceback_later(400, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


def hip():
    from sketchyscenecolorization_amd import hip as h
    return h


def _dev(a, offset=0):
    """The array on the device, its first byte ``offset`` bytes past a 16-byte boundary."""
    a = np.ascontiguousarray(a)
    if offset == 0:
        return torch.from_numpy(a).cuda()
    assert a.dtype == np.uint8
    base = torch.zeros(a.size + 32, dtype=torch.uint8, device='cuda')
    start = (16 - base.data_ptr() % 16) % 16 + offset
    view = base[start:start + a.size].view(a.shape)
    view.copy_(torch.from_numpy(a))
    assert view.data_ptr() % 16 == offset % 16 and view.is_contiguous()
    return view


def _case(h, w, S, seed, scale=2.0, lut_kind='sparse', blank=False):
    rng = np.random.RandomState(seed)
    pred = (rng.randn(h, w) * scale).astype(np.float32)
    sk = rng.randint(0, 256, (S, S, 3)).astype(np.uint8)                # only the first byte decides
    sk[:, :, 0] = 255 if blank else rng.choice(BYTES, (S, S))
    labels = rng.randint(0, 6, (S, S)).astype(np.uint8)
    labels[rng.rand(S, S) < 0.1] = 255
    lut = {'zero': np.zeros(256, np.uint8), 'one': np.ones(256, np.uint8), 'sparse': np.zeros(256, np.uint8)}[lut_kind]
    if lut_kind == 'sparse':
        lut[[1, 4, 255]] = (1, 7, 255)
    return pred, sk, labels, lut


def _score(pred, sk, labels, lut, sk_off=0, lab_off=0):
    """-> (loss, I, P, A, live) of two runs, which must agree in every bit."""
    pred_d, sk_d, lab_d, lut_d = _dev(pred), _dev(sk, sk_off), _dev(labels, lab_off), _dev(lut)
    got = []
    for _ in range(2):
        out = torch.full((5,), -3, dtype=torch.int64, device='cuda')
        hip().match_score(pred_d, sk_d, lab_d, lut_d, out=out)
        host = out.cpu().numpy()
        got.append(host.tobytes())
    assert got[0] == got[1]                                             # the same bits on every run
    return (float(host[:1].view(np.float64)[0]),) + tuple(int(v) for v in host[1:])


def _two_kernels(pred, sk, labels, lut):
    """(I, P, A, live) the way --mode eval counts them: ssc_match_finish -> predicts, ssc_label_hist_u8 gated by it, the lut."""
    stroke = _dev((sk[:, :, 0] != 255).astype(np.uint8))
    lab_d = _dev(labels)
    _up, predicts = hip().match_finish(_dev(pred), stroke)
    P = hip().label_hist_u8(lab_d, predicts).cpu().numpy()
    area = hip().label_hist_u8(lab_d).cpu().numpy()
    on = lut != 0
    return int(P[on].sum()), int(P.sum()), int(area[on].sum()), int((sk[:, :, 0] <= 104).sum())


def _check(tag, pred, sk, labels, lut, got, loss_grad=True):
    loss, I, P, A, live = got
    assert (I, P, A, live) == _two_kernels(pred, sk, labels, lut), tag
    o = SO.score(pred, sk, labels, lut)
    assert (A, live) == (o['A'], o['live']), tag
    margin = 16 * 2.0 ** -24 * float(np.abs(pred).max())
    unsure = (np.abs(o['up'] - np.float64(SO.THRESHOLD)) <= margin) & (sk[:, :, 0] != 255)
    z = lut[labels] != 0
    print('%s: I %d P %d A %d live %d; float64 oracle I %d P %d, %d pixels within %.3e of the threshold'
          % (tag, I, P, A, live, o['I'], o['P'], int(unsure.sum()), margin))
    assert abs(P - o['P']) <= int(unsure.sum()) and abs(I - o['I']) <= int((unsure & z).sum()), tag
    print('%s: loss %.17g, float64 %.17g, rel %.3e' % (tag, loss, o['loss'], abs(loss - o['loss']) / max(o['loss'], 1e-300)))
    assert abs(loss - o['loss']) <= 1e-5 * o['loss'], tag
    h, w = pred.shape
    S = labels.shape[0]
    if loss_grad and S % h == 0 and h == w:
        acc = torch.zeros(1, dtype=torch.float64, device='cuda')
        _dp, n = hip().match_loss_grad(_dev(pred), _dev(sk), _dev(labels), _dev(lut), acc)
        other = float(acc.cpu()[0])
        bound = live * 2.0 ** -52 * o['abs_terms']
        print('%s: loss of ssc_match_loss_grad %.17g, difference %.3e, bound %.3e' % (tag, other, abs(loss - other), bound))
        assert int(n.cpu()[0]) == live and abs(loss - other) <= bound, tag
    return o


# ------------------------------------------------------------------ ssc_match_score
@pytest.mark.parametrize('lut_kind', ['sparse', 'zero', 'one'])
@pytest.mark.parametrize('h,w,S', [(3, 3, 24), (8, 8, 64), (5, 5, 40), (4, 8, 32), (7, 3, 36)])
def test_match_score(h, w, S, lut_kind):
    """(3, 24): every pixel of the last 8 rows and columns is in the clamp band; 64 and 40: more than one workgroup; h != w twice,
    once with sizes that divide nothing."""
    pred, sk, labels, lut = _case(h, w, S, 7 * h + w + len(lut_kind), lut_kind=lut_kind)
    assert all((sk[:, :, 0] == b).any() for b in BYTES) and (labels == 255).any()
    got = _score(pred, sk, labels, lut)
    o = _check('match_score %s %dx%d -> %d' % (lut_kind, h, w, S), pred, sk, labels, lut, got)
    assert 0 < got[4] < int((sk[:, :, 0] != 255).sum()) < S * S and 0 < got[2] < S * S
    if lut_kind == 'zero':
        assert got[1] == got[3] == 0 and o['I'] == 0
    if lut_kind == 'one':
        assert got[3] == S * S and got[1] == got[2]


def test_match_score_at_the_size_of_a_scene():
    pred, sk, labels, lut = _case(96, 96, 768, 11)
    assert hip().match_score_workspace_bytes(768) == 23040
    _check('match_score 96 -> 768', pred, sk, labels, lut, _score(pred, sk, labels, lut))


def test_match_score_of_a_blank_sketch_is_zero():
    pred, sk, labels, lut = _case(8, 8, 64, 3, blank=True)
    lut[:] = 0
    assert _score(pred, sk, labels, lut) == (0.0, 0, 0, 0, 0)
    lut[:] = 1                                           # the area of the target does not ask for a stroke
    assert _score(pred, sk, labels, lut) == (0.0, 0, 0, 64 * 64, 0)


@pytest.mark.parametrize('value,on', [(0.0, False), (5e-10, False), (-5e-10, False), (1e-9, True)])
def test_match_score_of_constant_maps_at_the_threshold(value, on):
    """A constant map is up-sampled exactly: every stroke pixel is predicted from 1e-9f on, none below."""
    _p, sk, labels, lut = _case(8, 8, 64, 5)
    pred = np.full((8, 8), value, np.float32)
    loss, I, P, A, live = _score(pred, sk, labels, lut)
    stroke, z = sk[:, :, 0] != 255, lut[labels] != 0
    assert (I, P, A, live) == _two_kernels(pred, sk, labels, lut)
    assert (I, P) == ((int((stroke & z).sum()), int(stroke.sum())) if on else (0, 0))
    assert (A, live) == (int(z.sum()), int((sk[:, :, 0] <= 104).sum()))
    assert abs(loss - live * np.log(2.0)) <= 1e-5 * live * np.log(2.0)


@pytest.mark.parametrize('h,S,seed', [(8, 64, 1), (5, 40, 2), (3, 24, 3)])
def test_match_score_near_the_threshold_counts_what_match_finish_predicts(h, S, seed):
    """Values of the size of the threshold itself, so that rounding decides pixels: the counts are those of ssc_match_finish's
    predicts, exactly -- the value is one inline function in both kernels."""
    _p, sk, labels, lut = _case(h, h, S, seed)
    rng = np.random.RandomState(seed)
    pred = (1e-9 + rng.randn(h, h) * 2e-9).astype(np.float32)
    pred[rng.rand(h, h) < 0.3] = np.float32(1e-9)
    got = _score(pred, sk, labels, lut)
    assert got[1:] == _two_kernels(pred, sk, labels, lut)
    up = SO.score(pred, sk, labels, lut)['up']
    assert 0 < got[2] < int((sk[:, :, 0] != 255).sum()) and (np.abs(up - 1e-9) < 1e-10).any()


def test_match_score_of_large_logits():
    """|u| up to 80: exp(-|u|) leaves float32's normal range, the terms stay finite and the sum is the float64 one."""
    pred, sk, labels, lut = _case(8, 8, 64, 9)
    pred = np.linspace(-80, 80, 64).astype(np.float32).reshape(8, 8)
    np.random.RandomState(4).shuffle(pred.reshape(-1))
    got = _score(pred, sk, labels, lut)
    assert np.isfinite(got[0]) and got[0] > 100
    _check('match_score |u| <= 80', pred, sk, labels, lut, got)


@pytest.mark.parametrize('sk_off,lab_off', [(0, 4), (4, 8), (1, 0), (0, 3), (2, 2), (7, 13), (15, 1), (5, 10), (9, 6), (11, 12), (14, 0)])
def test_match_score_takes_any_base_address(sk_off, lab_off):
    """Both bases on a 4-byte boundary: the 4-byte loads; any other: the byte-wise path.  Every offset 1 .. 15 occurs."""
    pred, sk, labels, lut = _case(5, 5, 40, 21)
    want = _score(pred, sk, labels, lut)
    assert _score(pred, sk, labels, lut, sk_off, lab_off) == want
    _check('match_score offsets %d %d' % (sk_off, lab_off), pred, sk, labels, lut, want, loss_grad=False)


def test_every_offset_is_covered():
    offs = [(0, 4), (4, 8), (1, 0), (0, 3), (2, 2), (7, 13), (15, 1), (5, 10), (9, 6), (11, 12), (14, 0)]
    assert {a for a, _b in offs} | {b for _a, b in offs} >= set(range(1, 16))


def test_match_score_refusals():
    pred, sk, labels, lut = _case(4, 4, 32, 1)
    p, s, l, t = _dev(pred), _dev(sk), _dev(labels), _dev(lut)
    out = torch.full((5,), -7, dtype=torch.int64, device='cuda')
    ws = torch.zeros(4096, device='cuda')
    big = ws.numel() * 4
    need = hip().match_score_workspace_bytes(32)
    assert need == 40 and hip().match_score_workspace_bytes(24) == 40 and hip().match_score_workspace_bytes(64) == 160
    assert hip().match_score_workspace_bytes(4096) == 40 * 2048
    for h, w, S in ((0, 4, 32), (4, 0, 32), (4, 4, 0), (4, 4, 2), (4, 4, 30), (33, 4, 32), (4, 33, 32), (4, 4, 4100)):
        assert rc('ssc_match_score', p, h, w, s, l, t, S, out, ws, big) == -1, (h, w, S)
    for k in range(4):
        args = [p, s, l, t]
        args[k] = None
        assert rc('ssc_match_score', args[0], 4, 4, args[1], args[2], args[3], 32, out, ws, big) == -1
    assert rc('ssc_match_score', p, 4, 4, s, l, t, 32, None, ws, big) == -1
    assert rc('ssc_match_score', p, 4, 4, s, l, t, 32, out, None, big) == -1
    assert rc('ssc_match_score', p, 4, 4, s, l, t, 32, out, ws, need - 1) == -1           # a workspace that is too small
    odd = torch.zeros(64, dtype=torch.uint8, device='cuda')[4:44]
    assert rc('ssc_match_score', p, 4, 4, s, l, t, 32, odd, ws, big) == -3
    assert rc('ssc_match_score', p, 4, 4, s, l, t, 32, out, ws[1:], big - 4) == -3
    assert bool((out == -7).all()) and not ws.any() and not odd.any()                       # a refusal writes nothing
    assert rc('ssc_match_score', p, 4, 4, s, l, t, 32, out, ws, need) == 0
    host = out.cpu().numpy()
    assert tuple(int(v) for v in host[1:]) == _two_kernels(pred, sk, labels, lut)


# ------------------------------------------------------------------ the command line
def test_validation_through_the_command_line(tmp_path):
    """4 iterations, a snapshot and a pass every 2: the snapshots are those of a run without passes, and each line of
    match_validation.jsonl is what --mode eval --mask_ap 0 gives for the snapshot of its iteration."""
    from sketchyscenecolorization_amd import match_eval, matching as m, tf_checkpoint
    import matching_oracle as MO
    cfg = m.MatchConfig(**dict(SMALL, **NARROW))
    backbone = str(tmp_path / 'backbone-1')
    tf_checkpoint.write_checkpoint(backbone, {k: a for k, a in m.random_variables(cfg, 31).items() if k.startswith('ResNet/')})
    flags = EO.write_split(str(tmp_path), 'train')[:4]
    eval_flags = EO.write_split(str(tmp_path), 'val', seed=3)
    _second_scene_gets_other_labels(str(tmp_path), 'train')
    _second_scene_gets_other_labels(str(tmp_path), 'val')
    common = ['--mode', 'train', '--backbone_snapshot', backbone, '--vocab_file', VOCAB, '--scene_size', '64', '--save_model_freq', '2',
              '--log_freq', '1', '--seed', '5', '--max_iteration', '4'] + flags

    def run(tag, extra):
        root = str(tmp_path / tag)
        return root, _child(common + ['--snapshot_root', root, '--log_root', root + '_log'] + extra, str(tmp_path))
    plain, printed0 = run('plain', [])
    scored, printed = run('scored', ['--val_freq', '2'])
    assert not os.path.exists(os.path.join(plain + '_log', 'match_validation.jsonl')) and 'val:' not in printed0
    for n in (2, 4):
        assert _snapshot_bytes(plain, n) == _snapshot_bytes(scored, n)
    assert [l for l in printed.split('\n') if l.startswith('iter = ')] == [l for l in printed0.split('\n') if l.startswith('iter = ')]
    records = [json.loads(l) for l in open(os.path.join(scored + '_log', 'match_validation.jsonl'))]
    assert [r['iter'] for r in records] == [2, 4] and all(r['scenes'] == 2 and r['captions'] == 6 for r in records)
    lines = [l for l in printed.split('\n') if l.startswith('val: ')]
    assert len(lines) == 2 and printed.strip().split('\n')[-1].startswith('model saved to ')
    vocab = m.load_vocab(VOCAB)
    scenes = match_eval.read_captions(eval_flags[3], 'val')
    for r, line in zip(records, lines):
        snap = os.path.join(scored, 'deeplab_RMI_iter_%d.tfmodel' % r['iter'])
        out_dir = str(tmp_path / ('eval_%d' % r['iter']))
        _child(['--mode', 'eval', '--mask_ap', '0', '--snapshot', snap, '--vocab_file', VOCAB, '--scene_size', '64',
                '--eval_result_root', out_dir] + eval_flags, str(tmp_path))
        ev = json.load(open(os.path.join(out_dir, 'eval_val.json')))
        I, U = [c['I'] for c in ev['per_caption']], [c['U'] for c in ev['per_caption']]
        assert len(I) == 6 and r['overall_iou'] == sum(I) / sum(U) == ev['overall_IoU']
        assert r['precision'] == {str(t): sum(int(i / u >= t) for i, u in zip(I, U)) / 6.0 for t in match_eval.IOU_LEVELS}
        assert r['precision'] == ev['precision']
        assert line == 'val: iter = %d, overall IoU = %f, precision@0.5 = %f, loss = %f' % (r['iter'], r['overall_iou'],
                                                                                            r['precision']['0.5'], r['class_loss_mean'])
        # the class loss of those captions: the float64 oracle on the head's map of the snapshot's weights
        model = m.MatchModel(cfg)
        model.load_tf_checkpoint(snap)
        losses, live = [], 0
        for image_id, pairs in scenes:
            gt = match_eval.load_ground_truth(eval_flags[1], 'val', image_id, 64)
            feat, _stroke = model.features(gt['sketch'])
            for caption, idx in pairs:
                indices, seq_len = m.preprocess_sentence(caption, vocab, cfg.max_len)
                tok = torch.from_numpy(np.asarray(indices, np.int32)).cuda()
                pred = model.head(feat, tok, seq_len).cpu().numpy()
                lut = np.zeros(256, np.uint8)
                lut[[i + 1 for i in idx]] = 1
                o = SO.score(pred, gt['sketch'], gt['labels'], lut)
                losses.append(o['loss'])
                live += o['live']
        model.close()
        want = float(np.mean(losses))
        print('iter %d: class_loss_mean %.17g, float64 oracle %.17g, rel %.3e' % (r['iter'], r['class_loss_mean'], want,
                                                                                 abs(r['class_loss_mean'] - want) / want))
        assert abs(r['class_loss_mean'] - want) <= 1e-5 * want and r['live_pixels'] == live and r['seconds'] > 0
    assert records[0]['class_loss_mean'] != records[1]['class_loss_mean']          # the weights of the moment
    # --val_scenes 1: the three captions of the first scene
    one, _ = run('one', ['--val_freq', '4', '--val_scenes', '1'])
    recs = [json.loads(l) for l in open(os.path.join(one + '_log', 'match_validation.jsonl'))]
    assert [(r['iter'], r['scenes'], r['captions']) for r in recs] == [(4, 1, 3)]
    assert _snapshot_bytes(one, 4) == _snapshot_bytes(plain, 4)
