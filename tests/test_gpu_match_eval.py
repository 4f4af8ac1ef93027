"""The matcher's evaluation on the device (csrc/match_eval.hip, sketchyscenecolorization_amd/match_eval.py, match_main.py --mode
eval): hip.label_hist_u8 and hip.instance_label_hist against NumPy, exactly (integer counts); score_caption on the crafted
predictions of tests/golden/match_eval/ against what the reference's functions returned; the backbone run once and the head per
caption against MatchModel.forward per caption, bit for bit; the command line in a fresh process on a synthetic split against the
mask-based restatement tests/match_eval_oracle.py fed the device's own predicts.

Outputs sit inside buffers with a guard band on either side that must come back untouched."""
import faulthandler
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import match_eval_oracle as O
from kernel_check import rc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, 'tests', 'golden', 'match_eval')
VOCAB = os.path.join(ROOT, 'tests', 'golden', 'match', 'vocab.txt')
GUARD = 64
CHILD_LIMIT = 180
SMALL = dict(size=64, units=(1, 1, 1, 1), filters=(8, 16, 32, 64, 128))
CAPTIONS = ['the house on the left', 'two trees on the right', 'all the people near the bus']


@pytest.fixture(autouse=True)
def _time_limit():
    """A test that hangs on the device ends the process (with every thread's traceback) instead of holding the card."""
    faulthandler.dump_traceback_later(400, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


def hip():
    from sketchyscenecolorization_amd import hip as h
    return h


def E():
    from sketchyscenecolorization_amd import match_eval
    return match_eval


def M():
    from sketchyscenecolorization_amd import matching
    return matching


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


class GuardedI64(object):
    """An int64 output of this shape in the middle of a buffer filled with a sentinel."""
    FILL = -(1 << 40)

    def __init__(self, shape):
        n = int(np.prod(shape))
        self.raw = torch.full((n + 2 * GUARD,), self.FILL, dtype=torch.int64, device='cuda')
        self.t = self.raw[GUARD:GUARD + n].view(*shape)

    def get(self):
        g = torch.cat([self.raw[:GUARD], self.raw[-GUARD:]]).cpu()
        assert bool((g == self.FILL).all()), 'the kernel wrote outside its output'
        return self.t.cpu().numpy()


def _at_offset(a, off):
    """The bytes of ``a`` on the device, ``off`` bytes behind a 256-byte boundary."""
    base = torch.zeros(a.size + 64, dtype=torch.uint8, device='cuda')
    assert base.data_ptr() % 256 == 0
    view = base[off:off + a.size]
    view.copy_(torch.from_numpy(np.ascontiguousarray(a).reshape(-1)))
    return view, base


# ------------------------------------------------------------------ ssc_label_hist_u8
def _labels(n, seed):
    """Runs of equal labels (a label map is made of them) with single pixels strewn in; every value 0 .. 255 where n allows."""
    rng = np.random.RandomState(seed)
    a = np.repeat(rng.randint(0, 256, n // 7 + 1), 7)[:n].astype(np.uint8)
    pick = rng.rand(n) < 0.2
    a[pick] = rng.randint(0, 256, int(pick.sum()))
    if n >= 256:
        a[rng.permutation(n)[:256]] = np.arange(256)
    return a


@pytest.mark.parametrize('off_labels,off_gate', [(0, 0), (1, 1), (1, 0), (0, 3), (5, 13)])
@pytest.mark.parametrize('n', [1, 255, 4099, 64 * 64])
def test_label_hist(n, off_labels, off_gate):
    rng = np.random.RandomState(n + off_labels)
    lab = _labels(n, n)
    if n >= 256:
        assert len(np.unique(lab)) == 256
    lab_d, keep1 = _at_offset(lab, off_labels)
    assert lab_d.data_ptr() % 16 == off_labels
    gates = {'none': None, 'zero': np.zeros(n, np.uint8),
             'random': rng.choice(np.array([0, 0, 1, 2, 7, 128, 255], np.uint8), n)}
    assert n < 16 or (gates['random'] > 1).any()
    for name, g in gates.items():
        g_d, keep2 = (None, None) if g is None else _at_offset(g, off_gate)
        want = np.bincount(lab if g is None else lab[g != 0], minlength=256).astype(np.int64)
        out = GuardedI64((256,))
        hip().label_hist_u8(lab_d, g_d, out=out.t)
        first = out.get().copy()
        hip().label_hist_u8(lab_d, g_d, out=out.t)          # the entry point zeroes out itself; the same bits again
        assert np.array_equal(first, want), (n, name)
        assert np.array_equal(out.get(), first), (n, name)
        assert int(first.sum()) == (n if g is None else int((g != 0).sum()))


def test_label_hist_at_the_size_of_a_scene_and_two_shapes():
    """768 x 768: more than one workgroup (144 of them), long runs of one label as a real label map has."""
    lab = np.zeros((768, 768), np.uint8)
    rng = np.random.RandomState(1)
    for k in range(1, 40):
        y, x = rng.randint(0, 700, 2)
        lab[y:y + rng.randint(5, 68), x:x + rng.randint(5, 68)] = k
    gate = (rng.rand(768, 768) < 0.3).astype(np.uint8) * 3
    out = GuardedI64((256,))
    hip().label_hist_u8(_dev(lab), None, out=out.t)
    assert np.array_equal(out.get(), np.bincount(lab.reshape(-1), minlength=256))
    hip().label_hist_u8(_dev(lab), _dev(gate), out=out.t)
    assert np.array_equal(out.get(), np.bincount(lab[gate != 0], minlength=256))


def test_label_hist_refusals():
    lab, out = torch.zeros(64, dtype=torch.uint8, device='cuda'), GuardedI64((256,))
    assert rc('ssc_label_hist_u8', lab, None, 0, out.t) == -1
    assert rc('ssc_label_hist_u8', lab, None, (1 << 24) + 1, out.t) == -1
    assert rc('ssc_label_hist_u8', None, None, 64, out.t) == -1
    assert rc('ssc_label_hist_u8', lab, None, 64, None) == -1
    odd = torch.zeros(4096, dtype=torch.uint8, device='cuda')[4:]           # an output that is not on an 8-byte boundary
    assert rc('ssc_label_hist_u8', lab, None, 64, odd) == -3
    assert not odd.any()
    assert (out.get() == GuardedI64.FILL).all()


# ------------------------------------------------------------------ ssc_instance_label_hist
def _fixture():
    with np.load(os.path.join(GOLD, 'metrics.npz')) as z:
        masks = [z['mask_%d' % k] for k in range(int(z['n']))]
        caps = [{k: z['c%d/%s' % (c, k)] for k in ('predicts', 'inst_indices', 'I', 'U', 'matched', 'scores', 'overlaps', 'ap')}
                for c in range(int(z['n_captions']))]
        return z['labels'], z['boxes'], masks, caps


def _instance_hist(labels, boxes, masks):
    full = O.expand(boxes, masks, labels.shape[0])
    return np.stack([np.bincount(labels[f != 0], minlength=256) for f in full]).astype(np.int64)


def _scene40():
    """The fixture's scene (overlapping boxes, bytes of 2 and 3) with a 1 x 1 box and a box on the last row and column."""
    labels, boxes, masks, _ = _fixture()
    labels = labels.copy()
    labels[39, 39], labels[39, 30:39] = 9, 8
    boxes = np.concatenate([boxes, np.array([[5, 5, 5, 5], [35, 33, 39, 39], [0, 0, 39, 39]], np.int32)])
    rng = np.random.RandomState(2)
    masks = masks + [np.array([[3]], np.uint8), rng.randint(0, 3, (5, 7)).astype(np.uint8), rng.randint(0, 2, (40, 40)).astype(np.uint8)]
    masks[-2][4, 6] = 2
    return labels, boxes, masks


def test_instance_label_hist():
    labels, boxes, masks = _scene40()
    buf, offsets = M().pack_masks(boxes, masks, 40)
    want = _instance_hist(labels, boxes, masks)
    assert want[7].sum() == 1 and want[7][labels[5, 5]] == 1 and want[8][9] == 1 and want[8][8] > 0
    assert any((m == 2).any() for m in masks) and any((m == 3).any() for m in masks)
    out = GuardedI64((len(masks), 256))
    for _ in range(2):
        hip().instance_label_hist(_dev(labels), _dev(buf), _dev(boxes), _dev(offsets), out=out.t)
        assert np.array_equal(out.get(), want)


def test_instance_label_hist_refuses_what_leaves_its_buffers():
    labels, boxes, masks = _scene40()
    buf, offsets = M().pack_masks(boxes, masks, 40)
    want = _instance_hist(labels, boxes, masks)
    bad, off = boxes.copy(), offsets.copy()
    bad[1] = [36, 36, 40, 39]           # leaves the image
    off[3] = len(buf) - 3               # the mask leaves the buffer
    out = GuardedI64((len(masks), 256))
    hip().instance_label_hist(_dev(labels), _dev(buf), _dev(bad), _dev(off), out=out.t)
    got = out.get()
    assert (got[[1, 3]] == -1).all()
    keep = [k for k in range(len(masks)) if k not in (1, 3)]
    assert np.array_equal(got[keep], want[keep])
    empty = boxes.copy()
    empty[2] = [5, 5, 4, 9]
    hip().instance_label_hist(_dev(labels), _dev(buf), _dev(empty), _dev(offsets), out=out.t)
    got = out.get()
    assert (got[2] == -1).all() and np.array_equal(np.delete(got, 2, 0), np.delete(want, 2, 0))
    l, b, o, m = _dev(labels), _dev(boxes), _dev(offsets), _dev(buf)
    assert rc('ssc_instance_label_hist', l, 0, m, len(buf), b, o, len(masks), out.t) == -1
    assert rc('ssc_instance_label_hist', l, 40, m, len(buf), b, o, 0, out.t) == -1
    assert rc('ssc_instance_label_hist', l, 40, m, 0, b, o, len(masks), out.t) == -1
    assert rc('ssc_instance_label_hist', l, 40, None, len(buf), b, o, len(masks), out.t) == -1


# ------------------------------------------------------------------ score_caption on the reference's cases
def test_score_caption_equals_the_reference():
    labels, boxes, masks, caps = _fixture()
    buf, offsets = M().pack_masks(boxes, masks, 40)
    scene = E().SceneOnDevice('fixture', labels, boxes, buf, offsets, 7)
    assert np.array_equal(scene.area, np.bincount(labels.reshape(-1), minlength=256))
    assert np.array_equal(scene.H, _instance_hist(labels, boxes, masks))
    tot = E().Totals(True)
    for c in caps:
        got = E().score_caption(_dev(c['predicts']), scene, c['inst_indices'].tolist())
        assert (got['I'], got['U']) == (int(c['I']), int(c['U']))
        assert got['matched'] == c['matched'].tolist() and np.array_equal(got['scores'], c['scores'])
        assert got['ap'].dtype == np.float32 and np.array_equal(got['ap'], c['ap'])
        tot.add(got['I'], got['U'], got['ap'])
        only_iu = E().score_caption(_dev(c['predicts']), scene, c['inst_indices'].tolist(), mask_ap=False)
        assert (only_iu['I'], only_iu['U']) == (got['I'], got['U']) and 'ap' not in only_iu
    with np.load(os.path.join(GOLD, 'metrics.npz')) as z:
        m, ml = tot.mean_ap()
        assert abs(m - float(z['mAP'])) <= 1e-6 and np.abs(ml - z['mAP_list']).max() <= 1e-6
    with pytest.raises(ValueError, match='scene fixture'):
        E().score_caption(_dev(caps[0]['predicts']), scene, [7])


# ------------------------------------------------------------------ the backbone once, the head per caption
@pytest.fixture(scope='module')
def small_model():
    m = M()
    cfg = m.MatchConfig(**SMALL)
    v = m.random_variables(cfg, 31)
    model = m.MatchModel(cfg)
    model.load_dict(v)
    model.test_vars = v
    yield model
    model.close()


def _sketch(size, seed):
    rng = np.random.RandomState(seed)
    sk = np.full((size, size, 3), 255, np.uint8)
    sk[rng.rand(size, size) < 0.5] = 0
    return sk


@pytest.mark.parametrize('order', [(0, 1, 2), (2, 1, 0)])
def test_features_once_and_head_per_caption_equal_forward(small_model, order):
    model, vocab = small_model, M().load_vocab(VOCAB)
    assert len(vocab) == 76
    sk = _sketch(64, 5)
    sentences = [M().preprocess_sentence(c, vocab, 15) for c in CAPTIONS]
    want = []
    for idx, n in sentences:
        up, pr = model.forward(sk, idx, n)
        want.append((up.clone(), pr.clone()))
    assert not torch.equal(want[0][0], want[1][0])          # the captions do change the output
    model.forward(_sketch(64, 6), *sentences[0])            # another scene in between: nothing of it may stay
    feat, stroke = model.features(sk)
    kept = feat.clone()
    for k in order:
        up, pr = model.predict(feat, stroke, *sentences[k])
        assert torch.equal(up, want[k][0]) and torch.equal(pr, want[k][1]), k
        assert up.dtype == torch.float32 and pr.dtype == torch.uint8
    assert torch.equal(feat, kept)                          # the head left the cached feature map alone
    model.forward(_sketch(64, 6), *sentences[1])            # and so does a whole forward pass
    assert torch.equal(feat, kept)


# ------------------------------------------------------------------ the command line
def test_eval_mode_through_the_command_line(tmp_path, small_model):
    """A synthetic split (two scenes, 60 x 60 label images, 64 x 64 sketches, three captions each), the small model as a
    TensorFlow checkpoint, match_main --mode eval in a fresh process, twice.  The final bias is set so that ``up`` straddles 0
    (minus the median of up without it, taken on the device here): the prediction covers about half of the strokes."""
    from sketchyscenecolorization_amd import tf_checkpoint
    model, vocab = small_model, M().load_vocab(VOCAB)
    flags = O.write_split(str(tmp_path))
    gts = [E().load_ground_truth(str(tmp_path / 'data'), 'val', k, 64) for k in ('11', '12')]
    v = {k: a.copy() for k, a in model.test_vars.items()}
    bias = 'text_sketchyscene/m_lstm_output_projection/biases'
    v[bias][:] = 0
    model.load_dict(v)
    up, _ = model.forward(gts[0]['sketch'], *M().preprocess_sentence(CAPTIONS[0], vocab, 15))
    v[bias][:] = -float(up.median())
    model.load_dict(model.test_vars)
    snap = tmp_path / 'snapshot'
    snap.mkdir()
    tf_checkpoint.write_checkpoint(str(snap / 'model-3'), v)
    (snap / 'checkpoint').write_text('model_checkpoint_path: "model-3"\n')
    results, dump = tmp_path / 'results', tmp_path / 'predicts.npy'
    code = ('import json, sys; sys.path.insert(0, %r); import match_main; '
            'from sketchyscenecolorization_amd.matching import MatchConfig; '
            'match_main.main(sys.argv[3:], config=MatchConfig(**json.loads(sys.argv[1])), predicts_out=sys.argv[2])' % ROOT)
    argv = [sys.executable, '-c', code, json.dumps(SMALL), str(dump), '--mode', 'eval', '--snapshot', str(snap), '--vocab_file', VOCAB,
            '--scene_size', '64', '--eval_result_root', str(results)] + flags

    def run():
        r = subprocess.run(argv, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=CHILD_LIMIT, cwd=str(tmp_path))
        assert r.returncode == 0, r.stderr.decode()[-2000:]
        return r.stdout.decode(), open(str(results / 'eval_val.json')).read()
    printed, text = run()
    rec = json.loads(text)
    predicts = np.load(str(dump))
    assert predicts.shape == (6, 64, 64) and predicts.dtype == np.uint8 and len(rec['per_caption']) == 6
    want = []
    for n, cap in enumerate(rec['per_caption']):
        scene = 0 if n < 3 else 1
        assert cap['image_id'] == ('11', '12')[scene] and cap['caption'] == CAPTIONS[n % 3] == cap['text']
        assert cap['inst_indices'] == [[0], [1, 3], [2, 4, 2]][n % 3]
        with np.load(str(tmp_path / 'seg' / 'val' / 'seg_data' / ('%s_datas.npz' % cap['image_id'])), allow_pickle=True) as z:
            full = O.expand(z['pred_boxes'], list(z['pred_masks']), 64)
        r = O.caption(predicts[n], gts[scene]['labels'], full, cap['inst_indices'])
        assert (cap['I'], cap['U'], cap['matched_inst_indices']) == (r['I'], r['U'], r['matched']), n
        assert np.array_equal(np.asarray(cap['AP'], np.float32), r['ap']) and [float(a) for a in r['ap']] == cap['AP'], n
        want.append(r)
    tot = O.totals(want)
    print('eval through the command line: cum_I %d cum_U %d, matched %s' % (tot['cum_I'], tot['cum_U'], [r['matched'] for r in want]))
    assert 0 < tot['cum_I'] < tot['cum_U']
    assert (rec['cum_I'], rec['cum_U'], rec['overall_IoU'], rec['captions'], rec['scenes']) == \
        (tot['cum_I'], tot['cum_U'], tot['overall_IoU'], 6, 2)
    assert [rec['precision'][str(t)] for t in O.LEVELS] == tot['precision']
    assert rec['mAP'] == tot['mAP'] and rec['mAP_list'] == [float(a) for a in tot['mAP_list']]
    assert rec['split'] == 'val' and rec['snapshot'] == str(snap / 'model-3') and rec['augment_seed'] is None
    block = O.block(str(snap / 'model-3'), tot)
    assert block in printed
    assert open(str(results / 'deeplab_RMI_val_result.txt')).read() == block
    printed2, text2 = run()
    assert text2 == text and block in printed2
    assert open(str(results / 'deeplab_RMI_val_result.txt')).read() == block + block     # the result file is appended to
