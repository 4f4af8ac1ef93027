"""The scene session and the system command line on the device (scene_session.py, sketchyscene_colorization_main.py; DESIGN.md
section 8.14): hip.scene_change_hist_u8 (ssc_scene_change_hist_u8) against NumPy, exactly; a session of four turns against the
chain made by hand -- matching.match_instances, then fg_scene.colorize_instances or bg_scene.colorize_background, with the
previous image and text handed over on the host -- byte for byte; withdraw; the command line in fresh processes; refusals.

The models are the small ones of tests/test_gpu_matching.py, test_gpu_fg_scene.py and test_gpu_bg_scene.py at a 64 x 64 scene,
the smallest size all three accept."""
import faulthandler
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
from PIL import Image

import fg_scene_oracle as FO
from kernel_check import rc
from test_gpu_matching import BIAS, GOLD as MATCH_GOLD, HEAD_SMALL, SMALL, Guarded, _dev, _model, _sketch, _vocab

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BG_VOCAB = os.path.join(ROOT, 'tests', 'golden', 'bg_aug', 'bg_vocab.txt')
CHILD_LIMIT = 180               # seconds a command-line child may take (start-up of a fresh process included)
S = 64
ID = '9996'
NOISE_SEED = 3
FG_A = 'the bus on the left is yellow with blue windows'
FG_B = 'the house has a red roof'
BG_A = 'the sky is red and the ground is yellow'
BG_B = 'the sky is pink'


@pytest.fixture(autouse=True)
def _time_limit():
    """A test that hangs on the device ends the process (with every thread's traceback) instead of holding the card."""
    faulthandler.dump_traceback_later(400, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


def hip():
    from sketchyscenecolorization_amd import hip as h
    return h


# ---------------------------------------------------------------------------------------------------------------
# ssc_scene_change_hist_u8
# ---------------------------------------------------------------------------------------------------------------
def _at_offset(a, off):
    """The array on the device, its first byte ``off`` bytes past a 16-byte boundary -> (tensor, what keeps it alive)."""
    raw = torch.zeros(a.size + 32, dtype=torch.uint8, device='cuda')
    start = (16 - raw.data_ptr() % 16) % 16 + off
    t = raw[start:start + a.size].view(a.shape)
    t.copy_(torch.from_numpy(np.ascontiguousarray(a)))
    assert t.data_ptr() % 16 == off % 16
    return t, raw


def _inner(h, w, seed):
    """Runs of one instance, as an inner mask is made, with single pixels strewn in; 0 and 255 among the values."""
    rng = np.random.RandomState(seed)
    n = h * w
    a = np.repeat(rng.choice(np.array([0, 0, 1, 2, 3, 17, 254, 255], np.uint8), n // 5 + 1), 5)[:n].copy()
    pick = rng.rand(n) < 0.1
    a[pick] = rng.randint(0, 256, int(pick.sum()))
    a[0] = 0
    a[-1] = 255
    return a.reshape(h, w)


def _want(prev, new, inner):
    return np.bincount(inner[(prev != new).any(-1)].reshape(-1), minlength=256).astype(np.int64)


def _pairs(h, w, seed):
    """{case: (prev, new)}: identical images; exactly one channel of every pixel differs; random differences, among them pixels
    that differ in the last channel only and in all three."""
    rng = np.random.RandomState(seed)
    prev = rng.randint(0, 256, (h, w, 3)).astype(np.uint8)
    one = prev.copy()
    ch = rng.randint(0, 3, (h, w))
    yy, xx = np.mgrid[0:h, 0:w]
    one[yy, xx, ch] ^= rng.randint(1, 256, (h, w)).astype(np.uint8)
    some = prev.copy()
    pick = rng.rand(h, w) < 0.35
    some[pick] = rng.randint(0, 256, (int(pick.sum()), 3))
    last = rng.rand(h, w) < 0.1
    some[last, 2] ^= 1
    return {'identical': (prev, prev.copy()), 'one_channel': (prev, one), 'random': (prev, some)}


@pytest.mark.parametrize('off', [0, 5], ids=['aligned', 'off_by_5'])
@pytest.mark.parametrize('shape', [(1, 1), (37, 29), (64, 64), (768, 768)], ids=lambda s: '%dx%d' % s)
def test_change_hist(shape, off):
    """Exact against NumPy: 1 x 1 and 37 x 29 (1073 pixels: 67 groups of 16 and a rest of 1), one workgroup and many; pointers on
    a 16-byte boundary (the 16-byte loads) and 5 bytes past one (the bytewise loads)."""
    h, w = shape
    inner = _inner(h, w, h + w)
    assert h * w == 1 or (inner.reshape(-1)[0] == 0 and inner.reshape(-1)[-1] == 255)
    inner_d, k0 = _at_offset(inner, off)
    for name, (prev, new) in _pairs(h, w, h * w + off).items():
        prev_d, k1 = _at_offset(prev, off)
        new_d, k2 = _at_offset(new, off)
        want = _want(prev, new, inner)
        if name == 'identical':
            assert not want.any()
        if name == 'one_channel':
            assert np.array_equal(want, np.bincount(inner.reshape(-1), minlength=256)) and ((prev != new).sum(-1) == 1).all()
        out = Guarded((256,), torch.int64)
        hip().scene_change_hist_u8(prev_d, new_d, inner_d, out=out.t)
        first = out.get().copy()
        hip().scene_change_hist_u8(prev_d, new_d, inner_d, out=out.t)       # the entry point zeroes out itself; the same bits again
        assert np.array_equal(first, want), (shape, name, int(np.abs(first - want).sum()))
        assert np.array_equal(out.get(), first), (shape, name)
        assert np.array_equal(prev_d.cpu().numpy(), prev) and np.array_equal(new_d.cpu().numpy(), new)    # the inputs are only read


def test_change_hist_refuses_bad_arguments_without_launching():
    h = hip()
    img, inner, out = torch.zeros((8, 8, 3), dtype=torch.uint8, device='cuda'), torch.zeros((8, 8), dtype=torch.uint8, device='cuda'), \
        Guarded((256,), torch.int64)
    before = h.LAUNCHES
    assert rc('ssc_scene_change_hist_u8', None, img, inner, 8, 8, out.t) == -1
    assert rc('ssc_scene_change_hist_u8', img, None, inner, 8, 8, out.t) == -1
    assert rc('ssc_scene_change_hist_u8', img, img, None, 8, 8, out.t) == -1
    assert rc('ssc_scene_change_hist_u8', img, img, inner, 8, 8, None) == -1
    assert rc('ssc_scene_change_hist_u8', img, img, inner, 0, 8, out.t) == -1
    assert rc('ssc_scene_change_hist_u8', img, img, inner, 8, -1, out.t) == -1
    assert rc('ssc_scene_change_hist_u8', img, img, inner, 4097, 4096, out.t) == -1
    odd = torch.zeros(4096, dtype=torch.uint8, device='cuda')[4:]           # an output that is not on an 8-byte boundary
    assert rc('ssc_scene_change_hist_u8', img, img, inner, 8, 8, odd) == -3
    assert not odd.any()
    bad = [(img[:4], img, inner), (img, img[:, :4], inner), (img, img, inner[:4]), (img.float(), img, inner), (img, img, inner.int()),
           (img.cpu(), img, inner), (img, img, inner.view(64)), (img.permute(1, 0, 2), img, inner)]
    for prev, new, lab in bad:
        with pytest.raises(ValueError):
            h.scene_change_hist_u8(prev, new, lab, out=out.t)
    for wrong in (torch.zeros(256, dtype=torch.int32, device='cuda'), torch.zeros(255, dtype=torch.int64, device='cuda')):
        with pytest.raises(ValueError):
            h.scene_change_hist_u8(img, img, inner, out=wrong)
    with pytest.raises(ValueError):
        h.scene_change_hist_u8(img[:0], img[:0], inner[:0], out=out.t)
    assert h.LAUNCHES == before and out.untouched()


# ---------------------------------------------------------------------------------------------------------------
# the models and the scene
# ---------------------------------------------------------------------------------------------------------------
BOXES = np.array([[8, 4, 30, 28], [34, 30, 58, 60], [44, 2, 62, 26], [10, 40, 28, 60]], np.int32)
CLASSES = np.array([15, 9, 27, 40], np.int32)          # house, bus, grass, and a class the instance generator does not colour
_SHARED = {}


def _predicts(model, text):
    from sketchyscenecolorization_amd import matching
    idx, n = matching.preprocess_sentence(text, _vocab(), 15)
    return model.forward(model.test_sketch, idx, n)[1].cpu().numpy()


def _shared():
    """The three small models with random weights and a 64 x 64 scene whose masks follow the matcher's own predictions, so that
    FG_A matches the instances built for it: the mask of an instance among 0, 1, 2 in whose box FG_A predicts something is that
    prediction (``followers``), every other mask lies where no sentence predicts anything.  Scene '7' is the same with the first
    follower of class 40, scene '8' the same without a background pixel in rows 5 and 6."""
    if not _SHARED:
        from sketchyscenecolorization_amd import matching
        from sketchyscenecolorization_amd.bg_colorization import BGTrainer
        from sketchyscenecolorization_amd.data_processing.default_vocab import default_vocab_dict
        from sketchyscenecolorization_amd.data_processing.text_processing import load_vocab_dict_from_file
        from sketchyscenecolorization_amd.trainer import GanTrainer
        sketch = _sketch(S, 64)
        model, v = _model(S, SMALL['units'], SMALL['filters'], HEAD_SMALL, 11)
        model.test_vars, model.test_sketch = v, sketch
        idx, n = matching.preprocess_sentence(FG_A, _vocab(), 15)
        v[BIAS][:] = 0                      # the projection's bias at minus the median of up: the prediction straddles 0
        model.load_dict(v)
        v[BIAS][:] = -float(np.median(model.forward(sketch, idx, n)[0].cpu().numpy()))
        model.load_dict(v)
        pr = {t: _predicts(model, t) != 0 for t in (FG_A, FG_B)}
        inner = np.zeros((S, S), np.uint8)
        masks, followers = [], []
        for k, (y1, x1, y2, x2) in enumerate(BOXES.tolist()):
            inner[y1 + 1:y2 - 1, x1 + 1:x2 - 1] = k + 1
            box = (slice(y1, y2 + 1), slice(x1, x2 + 1))
            m = ~(pr[FG_A][box] | pr[FG_B][box])            # where no sentence predicts anything: never matched
            if k < 3 and pr[FG_A][box].sum() >= 4:         # where FG_A predicts: matched by it (occupancy 1)
                m = pr[FG_A][box]
                followers.append(k)
            assert m.sum() >= 4, (k, int(m.sum()))
            masks.append(np.ascontiguousarray(m.astype(np.uint8)))
        assert followers, 'the prediction of %r is empty in every box' % FG_A
        assert not inner[5:7].all()         # the sky colour is sought in rows 5 and 6
        scene = {'image_id': ID, 'sketch': sketch, 'inner': inner, 'class_ids': CLASSES.copy(), 'boxes': BOXES.copy(), 'masks': masks}
        full = dict(scene, image_id='8', inner=inner.copy())
        full['inner'][5:7, :] = 1            # no background pixel where the sky colour is sought: the gradient has no answer
        unknown = dict(scene, image_id='7', class_ids=CLASSES.copy())
        unknown['class_ids'][followers[0]] = 40
        _SHARED.update(matcher=model, variables=v, followers=followers, fg=GanTrainer(img=S, seed=2, block_type='Pix2Pix'),
                       bg=BGTrainer(image_size=S, max_steps=2, seed=1), scene=scene, full=full, unknown=unknown,
                       vocabs={'match': _vocab(), 'fg': default_vocab_dict(), 'bg': load_vocab_dict_from_file(BG_VOCAB)})
    return _SHARED


def _session(base, noise_seed=NOISE_SEED):
    from sketchyscenecolorization_amd import scene_session
    sh = _shared()
    return scene_session.SceneSession(sh['matcher'], sh['fg'], sh['bg'], sh['vocabs'], os.path.join(base, 'data'),
                                      os.path.join(base, 'out'), S, noise_seed=noise_seed)


def _noise(n):
    return torch.cat([torch.randn(1, 256, generator=torch.Generator().manual_seed(NOISE_SEED + p)) for p in range(n)]) if n else None


def _by_hand(scene, text, previous, previous_text):
    """One turn of the chain made by hand, the previous image and text on the host -> (kind, image, matched, bg text, fg image)."""
    from sketchyscenecolorization_amd import bg_scene, fg_scene, matching, scene_records
    sh = _shared()
    if scene_records.colorize_type(text) == 'FG':
        matched, _scores, _info = matching.match_instances(sh['matcher'], scene, text, sh['vocabs']['match'])
        image, _ = fg_scene.colorize_instances(sh['fg'], scene, text, matched, previous, vocab=sh['vocabs']['fg'], noise=_noise(len(matched)))
        return 'FG', image, matched, previous_text, None
    image, marked, processed = bg_scene.colorize_background(sh['bg'], scene, text, previous, previous_text, True, vocab=sh['vocabs']['bg'],
                                                            text_len=8)
    return 'BG', image, [], processed, marked


def _png(path):
    return np.array(Image.open(path).convert('RGB'), dtype=np.uint8)


def _records_bytes(records):
    return json.dumps([dict(zip(('colorization_type', 'result_name', 'input_text', 'proc_bg_text'), r)) for r in records], indent=4)


def _read(path):
    with open(path) as fp:
        return fp.read()


# ---------------------------------------------------------------------------------------------------------------
# the session
# ---------------------------------------------------------------------------------------------------------------
def test_session_equals_the_chain_made_by_hand(tmp_path):
    from sketchyscenecolorization_amd import scene_records, scene_session
    sh = _shared()
    scene, base = sh['scene'], str(tmp_path)
    FO.write_scene(os.path.join(base, 'data'), ID, scene)
    session = _session(base).open(ID)
    res = os.path.join(base, 'out', 'results', ID)
    rec_path = os.path.join(base, 'out', 'update_records', ID + '_records.json')
    previous, previous_text, records, images = scene['sketch'], '', [], []
    matched_any = []
    for k, text in enumerate((FG_A, BG_A, FG_B, BG_B), 1):
        report = session.color(text)
        got = _png(os.path.join(res, '%s_%d.png' % (ID, k)))
        kind, want, matched, bg_text, marked = _by_hand(scene, text, previous, previous_text)
        assert np.array_equal(got, want), (k, int((got != want).any(-1).sum()))
        assert (want != previous).any() or (kind == 'FG' and not matched), k
        records.append((kind, '%s_%d.png' % (ID, k), text, bg_text))
        assert _read(rec_path) == _records_bytes(records), k
        assert report == json.loads(_read(os.path.join(res, '%s_%d.json' % (ID, k))))
        assert report['colorization_type'] == kind and report['input_text'] == text and report['matched_inst_indices'] == matched
        assert report['matched_classes'] == [int(CLASSES[i]) for i in matched]
        assert report['changed'] == scene_session.changed_counts(_want(previous, want, scene['inner'])), k
        if kind == 'BG':
            assert np.array_equal(_png(os.path.join(res, ID + '_fg.png')), marked)
            assert report['processed_text'] == bg_text and report['sky_color'] is not None
        else:
            matched_any.append(matched)
        assert np.array_equal(session.current.cpu().numpy(), want)
        previous, previous_text = want, bg_text
        images.append(want)
    assert set(sh['followers']) <= set(matched_any[0]) and 3 not in matched_any[0] + matched_any[1]    # the scene was built for it
    assert previous_text == 'the sky is pink and the ground is yellow'
    assert sorted(os.listdir(res)) == sorted(['%s_%d.%s' % (ID, k, e) for k in (1, 2, 3, 4) for e in ('png', 'json')] + [ID + '_fg.png'])
    # two steps back, then a new instruction: it is number 3 and starts from the image of turn 2
    assert len(session.withdraw()) == 3 and len(session.withdraw()) == 2
    assert sorted(os.listdir(res)) == sorted(['%s_%d.%s' % (ID, k, e) for k in (1, 2) for e in ('png', 'json')] + [ID + '_fg.png'])
    assert _read(rec_path) == _records_bytes(records[:2])
    assert np.array_equal(session.current.cpu().numpy(), images[1])
    report = session.color(FG_B)
    assert report['result_name'] == ID + '_3.png'
    kind, want, matched, bg_text, _ = _by_hand(scene, FG_B, images[1], records[1][3])
    assert np.array_equal(_png(os.path.join(res, ID + '_3.png')), want) and report['matched_inst_indices'] == matched
    assert _read(rec_path) == _records_bytes(records[:2] + [('FG', ID + '_3.png', FG_B, records[1][3])])
    assert scene_records.fetch(ID, os.path.join(base, 'out'))[0] == ID + '_4.png'
    # a session opened on these records goes on from the last PNG
    again = _session(base).open(ID)
    assert np.array_equal(again.current.cpu().numpy(), want)


def test_refused_turns_leave_nothing_behind(tmp_path):
    """A scene the gradient has no answer for, and an instruction whose match holds a class the instance generator does not
    colour: no PNG, no report, no record; the next turn runs."""
    sh = _shared()
    base = str(tmp_path)
    FO.write_scene(os.path.join(base, 'data'), '8', sh['full'])
    FO.write_scene(os.path.join(base, 'data'), '7', sh['unknown'])
    FO.write_scene(os.path.join(base, 'data'), ID, sh['scene'])
    out = os.path.join(base, 'out')
    session = _session(base).open('8')
    with pytest.raises(ValueError) as e:
        session.color(BG_A)
    assert 'colour gradient status 1' in str(e.value)
    assert not os.path.exists(out)
    session.open('7')
    with pytest.raises(ValueError) as e:
        session.color(FG_A)
    assert 'instance %d has class 40' % sh['followers'][0] in str(e.value)
    assert not os.path.exists(out)
    session.open(ID)
    with pytest.raises(ValueError):
        session.withdraw()
    assert np.array_equal(session.current.cpu().numpy(), sh['scene']['sketch'])
    report = session.color(FG_A)
    _kind, want, matched, _t, _m = _by_hand(sh['scene'], FG_A, sh['scene']['sketch'], '')
    assert report['matched_inst_indices'] == matched and report['result_name'] == ID + '_1.png'
    assert np.array_equal(_png(os.path.join(out, 'results', ID, ID + '_1.png')), want)
    assert sorted(os.listdir(os.path.join(out, 'results', ID))) == [ID + '_1.json', ID + '_1.png']


# ---------------------------------------------------------------------------------------------------------------
# the command line
# ---------------------------------------------------------------------------------------------------------------
def _child(cwd, argv):
    code = ('import json, sys; sys.path.insert(0, %r); import sketchyscene_colorization_main as m; '
            'from sketchyscenecolorization_amd.matching import MatchConfig; '
            'm.main(%r, match_config=MatchConfig(**json.loads(%r)))' % (ROOT, list(argv), json.dumps(dict(SMALL, size=S))))
    r = subprocess.run([sys.executable, '-c', code], cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       universal_newlines=True, timeout=CHILD_LIMIT)
    assert r.returncode == 0, r.stdout[-4000:]
    return r.stdout


def test_command_line_in_fresh_processes(tmp_path):
    """Two --command color processes one after the other, and one --script process with the same two lines, leave the same PNG
    bytes and the same records file; --command withdraw removes the second."""
    from sketchyscenecolorization_amd import tf_checkpoint
    from sketchyscenecolorization_amd.obj_lib.main_procedure import save_checkpoint
    from sketchyscenecolorization_amd.params import ParamStore
    sh = _shared()
    cwd = str(tmp_path)
    FO.write_scene(os.path.join(cwd, 'data'), ID, sh['scene'])
    os.makedirs(os.path.join(cwd, 'match'))
    tf_checkpoint.write_checkpoint(os.path.join(cwd, 'match', 'model-3'), sh['variables'])
    with open(os.path.join(cwd, 'match', 'checkpoint'), 'w') as fp:
        fp.write('model_checkpoint_path: "model-3"\n')
    save_checkpoint(ParamStore('Pix2Pix', 58, S, 'cuda', seed=3), os.path.join(cwd, 'fg'), 'model_9.ckpt', 9)
    os.makedirs(os.path.join(cwd, 'bg'))
    torch.save(sh['bg'].store.state_dict(), os.path.join(cwd, 'bg', 'snapshot-2'))
    with open(os.path.join(cwd, 'bg', 'checkpoint'), 'w') as fp:
        fp.write('model_checkpoint_path: "snapshot-2"\n')
    vocab = sh['vocabs']['fg']
    with open(os.path.join(cwd, 'fg_vocab.txt'), 'w') as fp:
        fp.write('\n'.join(sorted(vocab, key=vocab.get)))
    with open(os.path.join(cwd, 'turns.txt'), 'w') as fp:
        fp.write('# two turns\n%s\n\n%s\n' % (FG_A, BG_A))
    common = ['--image_id', ID, '--data_base_dir', 'data', '--match_snapshot_root', 'match', '--match_vocab_path',
              os.path.join(MATCH_GOLD, 'vocab.txt'), '--fgcolor_snapshot_root', 'fg', '--fgcolor_vocab_path', 'fg_vocab.txt',
              '--fgcolor_image_size', str(S), '--fgcolor_block_type', 'Pix2Pix', '--bg_snapshot_root', 'bg', '--bg_vocab_path', BG_VOCAB,
              '--scene_size', str(S), '--noise_seed', str(NOISE_SEED)]
    out1 = _child(cwd, common + ['--results_base_dir', 'one', '--instruction', FG_A])
    out2 = _child(cwd, common + ['--results_base_dir', 'one', '-c', 'color', '-it', BG_A])
    out3 = _child(cwd, common + ['--results_base_dir', 'two', '--script', 'turns.txt'])
    lines = [ln for ln in (out1 + out2).splitlines() if ln.startswith(('FG ', 'BG '))]
    assert len(lines) == 2 and lines == [ln for ln in out3.splitlines() if ln.startswith(('FG ', 'BG '))]
    assert lines[0].startswith('FG matched_inst_indices ') and ' result %s_1.png changed ' % ID in lines[0]
    names = sorted(os.listdir(os.path.join(cwd, 'one', 'results', ID)))
    assert names == sorted([ID + '_1.png', ID + '_1.json', ID + '_2.png', ID + '_2.json', ID + '_fg.png'])
    assert names == sorted(os.listdir(os.path.join(cwd, 'two', 'results', ID)))
    for name in names:
        with open(os.path.join(cwd, 'one', 'results', ID, name), 'rb') as a, open(os.path.join(cwd, 'two', 'results', ID, name), 'rb') as b:
            assert a.read() == b.read(), name
    rec = os.path.join('update_records', ID + '_records.json')
    assert _read(os.path.join(cwd, 'one', rec)) == _read(os.path.join(cwd, 'two', rec))
    assert _read(os.path.join(cwd, 'one', rec)) == _records_bytes([('FG', ID + '_1.png', FG_A, ''), ('BG', ID + '_2.png', BG_A, BG_A)])
    first = _png(os.path.join(cwd, 'one', 'results', ID, ID + '_1.png'))
    assert (first != sh['scene']['sketch']).any() and (_png(os.path.join(cwd, 'one', 'results', ID, ID + '_2.png')) != first).any()
    _child(cwd, ['--command', 'withdraw', '--image_id', ID, '--results_base_dir', 'one'])
    assert sorted(os.listdir(os.path.join(cwd, 'one', 'results', ID))) == sorted([ID + '_1.png', ID + '_1.json', ID + '_fg.png'])
    assert _read(os.path.join(cwd, 'one', rec)) == _records_bytes([('FG', ID + '_1.png', FG_A, '')])
