"""The scene's instances on the device: ssc_fg_scene_mask_u8 (hip.fg_scene_mask_u8), ssc_road_parallel_u8 (hip.road_parallel_u8),
ssc_fg_scene_paste_u8 (hip.fg_scene_paste_u8), fg_scene.colorize_instances over them and obj_colorization_main.py --mode scene,
against the NumPy + PIL oracle tests/fg_scene_oracle.py.

Every comparison is byte-exact, and that is derived, not measured: the three kernels hold integer compares and copies only, the
two resizes are Pillow's 8-bit fixed-point resampler (held bit for bit by tests/test_gpu_edge_cases.py), and the generator's
image enters the oracle as the bytes the device made.  Outputs sit inside buffers filled with a sentinel; every launch runs twice.

The chain runs a Pix2Pix generator at 64 x 64 with seeded weights over the fixture tests/golden/fg_scene/scenes.npz."""
import faulthandler
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
from PIL import Image

import bg_scene_oracle as B
import fg_scene_oracle as O

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL = 0xA5
PAD = 16
CHILD_LIMIT = 180               # seconds a command-line child may take (start-up of a fresh process included)
S = 64
TEXT = 'the bus on the left is yellow with blue windows'
PROCESSED = 'the bus is yellow with blue windows'


@pytest.fixture(autouse=True)
def _time_limit():
    """A test that hangs on the device ends the process (with every thread's traceback) instead of holding the card."""
    faulthandler.dump_traceback_later(400, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _out(*shape):
    """A uint8 output of this shape inside a sentinel-filled buffer -> (the view, the buffer)."""
    n = int(np.prod(shape))
    raw = torch.full((n + 2 * PAD,), SENTINEL, dtype=torch.uint8, device='cuda')
    return raw[PAD:PAD + n].view(*shape), raw


def _around_intact(raw):
    g = raw.cpu().numpy()
    return (g[:PAD] == SENTINEL).all() and (g[-PAD:] == SENTINEL).all()


def _untouched(raw):
    return (raw.cpu().numpy() == SENTINEL).all()


# ---------------------------------------------------------------------------------------------------------------
# the mask image
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('box', [(1, 1), (3, 5), (7, 4), (29, 90)], ids=lambda b: '%dx%d' % b)
def test_mask_image(box):
    """Bytes 0, 1 and 2 everywhere, each of them once in the first pixel; the mask's last row and column are all 1 and must not
    show; the bytes around the output stay."""
    from sketchyscenecolorization_amd import hip
    bh, bw = box
    rng = np.random.RandomState(bh * 100 + bw)
    for first in (0, 1, 2):
        small = rng.randint(0, 3, (bh + 1, bw + 1)).astype(np.uint8)
        small[0, 0] = first
        small[bh, :] = 1
        small[:, bw] = 1
        want = O.mask_image(small)
        assert want.shape == (bh, bw, 3) and want[0, 0, 0] == (0 if first == 1 else 255)
        if bh * bw > 8:
            assert {0, 1, 2} <= set(small[:bh, :bw].reshape(-1).tolist()) and {0, 255} == set(want.reshape(-1).tolist())
        for again in range(2):
            out, raw = _out(bh, bw, 1)
            got = hip.fg_scene_mask_u8(_dev(small), out=out)
            assert got is out and np.array_equal(out.cpu().numpy()[:, :, 0], want[:, :, 0]) and _around_intact(raw), (box, first, again)
        assert np.array_equal(hip.fg_scene_mask_u8(_dev(small)).cpu().numpy()[:, :, 0], want[:, :, 0])


# ---------------------------------------------------------------------------------------------------------------
# the paste
# ---------------------------------------------------------------------------------------------------------------
# (H, W) -> boxes (y1, x1, bh, bw): odd and even x1, boxes that touch the last row and the last column, bh * bw no multiple of 4
PASTE_BOXES = {(9, 7): [(0, 1, 3, 3), (4, 2, 5, 5), (8, 6, 1, 1), (0, 0, 9, 7)],
               (16, 16): [(1, 3, 5, 7), (6, 0, 10, 16), (15, 15, 1, 1), (3, 8, 13, 8), (2, 5, 3, 3)]}


@pytest.mark.parametrize('value', [1, 255])
@pytest.mark.parametrize('shape', sorted(PASTE_BOXES), ids=lambda s: '%dx%d' % s)
def test_paste(shape, value):
    """The whole image is compared: a write outside the mask, outside the box or into another instance's pixels shows."""
    from sketchyscenecolorization_amd import hip
    h, w = shape
    rng = np.random.RandomState(h * 1000 + w + value)
    other = 2 if value == 1 else 254
    assert any(x1 % 2 for _, x1, _, _ in PASTE_BOXES[shape]) and any(x1 % 2 == 0 for _, x1, _, _ in PASTE_BOXES[shape])
    assert any(y1 + bh == h for y1, _, bh, _ in PASTE_BOXES[shape]) and any(x1 + bw == w for _, x1, _, bw in PASTE_BOXES[shape])
    assert any((bh * bw) % 4 for _, _, bh, bw in PASTE_BOXES[shape])
    for y1, x1, bh, bw in PASTE_BOXES[shape]:
        inner = rng.choice(np.array([0, value, other], np.uint8), (h, w))
        inner[y1, x1] = value                           # at least one pixel is pasted
        if bh * bw > 1:
            inner[y1 + bh - 1, x1 + bw - 1] = other     # and another instance's pixel lies inside the box
        result = rng.randint(0, 256, (h, w, 3)).astype(np.uint8)
        inst = rng.randint(0, 256, (bh, bw, 3)).astype(np.uint8)
        want = O.paste(result, inner, inst, (y1, x1, y1 + bh, x1 + bw), value)
        changed = (want != result).any(-1)
        assert changed.any() and not changed[inner != value].any()
        if bh * bw < h * w:
            outside = np.ones((h, w), bool)
            outside[y1:y1 + bh, x1:x1 + bw] = False
            assert (inner[outside] == value).any()      # pixels of the instance outside its box: not written
        for again in range(2):
            out, raw = _out(h, w, 3)
            out.copy_(_dev(result))
            got = hip.fg_scene_paste_u8(out, _dev(inner), _dev(inst), y1, x1, value)
            assert got is out and np.array_equal(out.cpu().numpy(), want) and _around_intact(raw), (shape, (y1, x1, bh, bw), again)


# ---------------------------------------------------------------------------------------------------------------
# the road test
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('pw', [2, 25])
@pytest.mark.parametrize('s', [8, 33, 192])
def test_road_parallel(s, pw):
    """White, one line, two lines over pw and pw - 1 columns (over the whole width where s < pw), two vertical lines, strokes
    two thick, strokes in the last row and column, grey levels 234 and 235, random sketches: verdict, V and Hc are the
    oracle's closed form, which tests/test_fg_scene.py holds against the reference's loop."""
    from sketchyscenecolorization_amd import hip
    cases = O.road_cases(s, pw)
    rng = np.random.RandomState(s * 100 + pw)
    for i in range(4):
        a = np.where(rng.rand(s, s) < rng.choice([0.02, 0.3]), rng.choice([0, 100, 234], (s, s)), rng.choice([235, 255], (s, s)))
        cases['random_%d' % i] = O.grey(a)
    if s <= 33:
        for name, sk in cases.items():
            assert O.road_counts(sk) == O.road_loop(sk, pw, counts=True) and O.road_closed(sk, pw) == O.road_loop(sk, pw), name
    if pw <= s - 2:
        assert O.road_counts(cases['two_lines_%d' % pw]) == (pw, 0) and O.road_counts(cases['two_lines_%d' % (pw - 1)]) == (pw - 1, 0)
    assert O.road_counts(cases['two_vertical']) == (0, s) and O.road_counts(cases['grey_234_235']) == (0, 0)
    seen = set()
    for name, sk in cases.items():
        v, hc = O.road_counts(sk)
        want = [int(v >= pw or hc >= pw), v, hc]
        seen.add(want[0])
        for again in range(2):
            buf = torch.full((5,), -77, dtype=torch.int32, device='cuda')
            got = hip.road_parallel_u8(_dev(sk), pw, out=buf[1:4])
            assert got.data_ptr() == buf[1:4].data_ptr()
            assert buf.cpu().tolist() == [-77] + want + [-77], (name, s, pw, again, buf.cpu().tolist(), want)
    assert seen == ({0, 1} if pw <= s else {0})
    assert hip.road_parallel_u8(_dev(cases['thick'])).cpu().tolist() == [int(s >= 25), s, 0]      # the default width is 25


# ---------------------------------------------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------------------------------------------
def test_entry_points_refuse_bad_arguments_without_launching():
    from sketchyscenecolorization_amd import hip
    L, st = hip.lib(), hip.stream_ptr
    h, w, bh, bw = 12, 10, 4, 5
    small = _dev(np.ones((bh + 1, bw + 1), np.uint8))
    inner = _dev(np.full((h, w), 3, np.uint8))
    inst = _dev(np.zeros((bh, bw, 3), np.uint8))
    sketch = _dev(np.zeros((8, 8, 3), np.uint8))
    (mask_out, raw_m), (result, raw_r) = _out(bh, bw), _out(h, w, 3)
    verdict = torch.full((8,), -77, dtype=torch.int32, device='cuda')
    off = lambda t, nbytes: hip.ptr(t.view(-1).view(torch.uint8)[nbytes:])      # noqa: E731
    mask = lambda small_=hip.ptr(small), bh_=bh, bw_=bw, out_=hip.ptr(mask_out): L.ssc_fg_scene_mask_u8(small_, bh_, bw_, out_, st())   # noqa: E731
    assert mask(bh_=0) == -1 and mask(bw_=0) == -1 and mask(bh_=-3) == -1 and mask(bh_=4096, bw_=4096) == -1
    assert mask(small_=None) == -1 and mask(out_=None) == -1
    road = lambda sk=hip.ptr(sketch), s=8, pw=25, out_=hip.ptr(verdict): L.ssc_road_parallel_u8(sk, s, pw, out_, st())      # noqa: E731
    assert road(s=0) == -1 and road(s=-8) == -1 and road(s=4097) == -1 and road(pw=0) == -1 and road(pw=-1) == -1
    assert road(sk=None) == -1 and road(out_=None) == -1 and road(out_=off(verdict, 2)) == -3 and road(out_=off(verdict, 1)) == -3
    names = ('result', 'inner', 'H', 'W', 'inst', 'y1', 'x1', 'bh', 'bw', 'value')
    base = dict(result=hip.ptr(result), inner=hip.ptr(inner), H=h, W=w, inst=hip.ptr(inst), y1=2, x1=3, bh=bh, bw=bw, value=3)
    paste = lambda **kw: L.ssc_fg_scene_paste_u8(*([kw.get(k, base[k]) for k in names] + [st()]))       # noqa: E731
    assert paste(y1=-1) == -1 and paste(x1=-1) == -1 and paste(y1=h - bh + 1) == -1 and paste(x1=w - bw + 1) == -1
    assert paste(bh=0) == -1 and paste(bw=0) == -1 and paste(bh=-2) == -1 and paste(bh=h + 1, y1=0) == -1 and paste(bw=w + 1, x1=0) == -1
    assert paste(value=0) == -1 and paste(value=256) == -1 and paste(value=-1) == -1
    assert paste(H=0) == -1 and paste(W=0) == -1 and paste(H=5000, W=5000) == -1 and paste(y1=2 ** 31 - 2) == -1
    assert paste(result=None) == -1 and paste(inner=None) == -1 and paste(inst=None) == -1
    torch.cuda.synchronize()
    assert _untouched(raw_m) and _untouched(raw_r) and (verdict.cpu().numpy() == -77).all()
    # and the same calls go through once the argument is right (a box in the last row and column included)
    assert mask() == 0 and road() == 0 and paste() == 0 and paste(y1=h - bh, x1=w - bw) == 0
    torch.cuda.synchronize()
    assert _around_intact(raw_m) and _around_intact(raw_r) and (mask_out.cpu().numpy() == 0).all()
    assert verdict.cpu().tolist() == [0, 0, 0] + [-77] * 5      # an all-black sketch: one run everywhere
    assert (result.cpu().numpy()[2:2 + bh, 3:3 + bw] == 0).all() and (result.cpu().numpy()[:2] == SENTINEL).all()
    # the wrappers refuse what the entry points would
    with pytest.raises(RuntimeError):
        hip.fg_scene_paste_u8(result, inner, inst, h - bh + 1, 0, 3)
    with pytest.raises(RuntimeError):
        hip.fg_scene_paste_u8(result, inner, inst, 0, 0, 256)


# ---------------------------------------------------------------------------------------------------------------
# the chain
# ---------------------------------------------------------------------------------------------------------------
_SHARED = {}


def _shared():
    if not _SHARED:
        from sketchyscenecolorization_amd.data_processing.default_vocab import default_vocab_dict
        from sketchyscenecolorization_amd.trainer import GanTrainer
        _SHARED.update(scenes=O.load_scenes(), vocab=default_vocab_dict(), trainer=GanTrainer(img=S, seed=2, block_type='Pix2Pix'))
    return _SHARED


def _noise(n, seed):
    return torch.cat([torch.randn(1, 256, generator=torch.Generator().manual_seed(seed + p)) for p in range(n)])


def _tokens(text, vocab):
    from sketchyscenecolorization_amd.data_processing.text_processing import preprocess_sentence
    return np.array(preprocess_sentence(text, vocab, 15), dtype=np.int32)[None]


def _generate_alone(tr, scene, indices, noise, vocab, text=PROCESSED):
    """A forward pass per instance on the oracle's Pillow-built sketch, outside colorize_instances -> (sketches, images)."""
    from sketchyscenecolorization_amd import fg_scene
    sketches, images = [], []
    for p, k in enumerate(indices):
        cls = int(scene['class_ids'][k])
        sk = O.instance_sketch(scene, k, S)
        label = torch.tensor([fg_scene.CLASS_TO_COLOR_ID[cls]], dtype=torch.int32, device='cuda')
        gen = tr.generate_u8(_dev(sk[None]), _tokens(text, vocab), noise[p:p + 1].cuda(), labels=label, thicken=(cls == O.GRASS_LABEL))
        sketches.append(sk)
        images.append(gen[0].cpu().numpy())
    return sketches, images


@pytest.mark.parametrize('name, indices', [('example', [4, 7, 8]), ('synthetic', [0, 1, 2])], ids=['example', 'synthetic'])
def test_colorize_instances_equals_the_oracle_chain(name, indices):
    from sketchyscenecolorization_amd import fg_scene
    sh = _shared()
    scene, tr, vocab = sh['scenes'][name], sh['trainer'], sh['vocab']
    noise = _noise(len(indices), 11)
    info = {}
    result, text = fg_scene.colorize_instances(tr, scene, TEXT, indices, vocab=vocab, noise=noise, info=info)
    assert text == PROCESSED and result.dtype == np.uint8 and result.shape == scene['sketch'].shape
    assert [i['index'] for i in info['instances']] == indices
    sketches, images = _generate_alone(tr, scene, indices, noise, vocab)
    for p, k in enumerate(indices):
        got = info['instances'][p]
        assert got['class'] == int(scene['class_ids'][k])
        assert np.array_equal(got['sketch'], sketches[p]), (name, k)
        assert (got['sketch'][:, :, 0] < 235).any() and (got['sketch'] == 255).any()
        assert np.array_equal(got['generated'], images[p]), (name, k, int((got['generated'] != images[p]).sum()))
        assert got['generated'].std() > 0
    want = O.finish(scene, indices, [i['generated'] for i in info['instances']])
    # the fixture makes every step show before the comparison means anything
    grass = B.grass_table(scene['class_ids'])
    drawn = B.drawn_region(scene['sketch'], scene['inner'], grass)
    moved = B.moved(scene['sketch'])[:, :, 0] == 0
    pasted_not_grass = np.zeros(scene['inner'].shape, bool)
    step = scene['sketch'].copy()
    for p, k in enumerate(indices):
        y1, x1, y2, x2 = [int(v) for v in scene['boxes'][k]]
        own = np.zeros(scene['inner'].shape, bool)
        own[y1:y2, x1:x2] = scene['inner'][y1:y2, x1:x2] == k + 1
        assert own.sum() >= 1, k
        after = O.finish(dict(scene, sketch=np.full_like(scene['sketch'], 255)), [k], [info['instances'][p]['generated']], previous=step)
        assert (after != step).any(), k         # the paste changes the image (the blank sketch keeps the strokes out of this)
        if int(scene['class_ids'][k]) == O.GRASS_LABEL:
            kept = own & moved
            assert kept.sum() >= 1 and not drawn[kept].any()
            inst = O.reverse_resize_image(info['instances'][p]['generated'], y2 - y1, x2 - x1, margin_size=10)
            assert np.array_equal(result[kept], inst[kept[y1:y2, x1:x2]])       # grass keeps its generated pixels under the strokes
        else:
            pasted_not_grass |= own
    assert (drawn & pasted_not_grass).sum() >= 1
    assert np.array_equal(result[drawn], B.moved(scene['sketch'])[drawn])
    roads = [i['road'] for i in info['instances']]
    if name == 'synthetic':
        assert roads[0] is None and roads[2] is None and roads[1] == dict(zip(('V', 'Hc'), O.road_counts(sketches[1]))) and roads[1]['V'] >= 25
        assert np.array_equal(sketches[2], O.mask_image(scene['masks'][2]))       # the exact-size box: no resize
    else:
        assert roads == [None] * 3
    bad = np.argwhere((result != want).any(-1))
    assert bad.size == 0, (name, len(bad), bad[:4].tolist())
    # a second call, on top of the first result, with the same noise: the same instances again
    again, _ = fg_scene.colorize_instances(tr, scene, TEXT, indices, previous_image=result, vocab=vocab, noise=noise)
    assert np.array_equal(again, O.finish(scene, indices, images, previous=result))


def test_a_single_line_road_is_refused():
    """Instance 0 of the example scene: a road whose mask is one line.  The counts are read with the image, at the end."""
    from sketchyscenecolorization_amd import fg_scene
    sh = _shared()
    scene = sh['scenes']['example']
    info = {}
    with pytest.raises(ValueError) as e:
        fg_scene.colorize_instances(sh['trainer'], scene, 'the road is black', [7, 0], vocab=sh['vocab'], noise=_noise(2, 5), info=info)
    assert 'road is a single line' in str(e.value) and 'instance 0' in str(e.value)
    assert info['instances'][1]['road'] == {'V': 0, 'Hc': 1} and info['instances'][0]['road'] is None
    assert np.array_equal(info['instances'][1]['sketch'], O.instance_sketch(scene, 0, S))
    assert not O.road_loop(O.instance_sketch(scene, 0, S))


def test_an_unknown_class_is_refused_before_any_launch():
    from sketchyscenecolorization_amd import fg_scene, hip
    sh = _shared()
    scene = sh['scenes']['synthetic']
    assert int(scene['class_ids'][3]) == 40 and 40 not in fg_scene.CLASS_TO_COLOR_ID
    before = hip.LAUNCHES
    for indices in ([3], [0, 3], [0, 5], [-1]):
        with pytest.raises(ValueError):
            fg_scene.colorize_instances(sh['trainer'], scene, TEXT, indices, vocab=sh['vocab'])
    with pytest.raises(ValueError):
        fg_scene.colorize_instances(sh['trainer'], scene, TEXT, [0], vocab=sh['vocab'], noise=_noise(2, 1))
    with pytest.raises(ValueError):
        fg_scene.colorize_instances(sh['trainer'], scene, 'this bus with blue windows', [0], vocab=sh['vocab'])
    assert hip.LAUNCHES == before


# ---------------------------------------------------------------------------------------------------------------
# the command line
# ---------------------------------------------------------------------------------------------------------------
STAMP = '2018-01-02-03-04-05'
ID = '5'


def _child(cwd, argv):
    code = 'import sys; sys.path.insert(0, %r); import obj_colorization_main as m; m.main(%r)' % (ROOT, list(argv))
    return subprocess.run([sys.executable, '-c', code], cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                          universal_newlines=True, timeout=CHILD_LIMIT)


def test_command_line(tmp_path):
    """A snapshot of seeded weights, the synthetic scene on disk, --mode scene --noise_seed 3 in a process of its own: the png is
    what a fresh trainer with that snapshot, the same noise vectors and the oracle make; a call that fails leaves no file."""
    from sketchyscenecolorization_amd.obj_lib.main_procedure import latest_checkpoint, restore_checkpoint, save_checkpoint
    from sketchyscenecolorization_amd.params import ParamStore
    from sketchyscenecolorization_amd.trainer import GanTrainer
    sh = _shared()
    scene = sh['scenes']['synthetic']
    cwd = str(tmp_path)
    run = os.path.join(cwd, 'outputs', STAMP)
    save_checkpoint(ParamStore('Pix2Pix', 58, S, 'cuda', seed=3), os.path.join(run, 'snapshot'), 'model_9.ckpt', 9)
    O.write_scene(os.path.join(cwd, 'scene'), ID, scene)
    common = ['--mode', 'scene', '-rf', STAMP, '-bt', 'Pix2Pix', '-si', '1', '--scene_dir', 'scene', '--scene_size', '96',
              '--image_id', ID, '--instruction', TEXT, '--noise_seed', '3']
    res = os.path.join(run, 'scene_results', ID)
    failed = _child(cwd, common + ['--inst_indices', '0,3'])
    assert failed.returncode != 0 and 'class 40' in failed.stdout, failed.stdout[-3000:]
    assert not os.path.exists(os.path.join(run, 'scene_results'))
    indices = [2, 0, 1]
    done = _child(cwd, common + ['--inst_indices', '2,0,1'])
    assert done.returncode == 0, done.stdout[-4000:]
    assert '## segment_user_input_text:  ' + PROCESSED in done.stdout and 'model_9.ckpt-9' in done.stdout
    assert sorted(os.listdir(res)) == [ID + '_inst.png', 'scene.json']
    got = np.array(Image.open(os.path.join(res, ID + '_inst.png')).convert('RGB'))
    tr = GanTrainer(img=S, seed=1, block_type='Pix2Pix')
    restore_checkpoint(tr.store, latest_checkpoint(os.path.join(run, 'snapshot')))
    sketches, images = _generate_alone(tr, scene, indices, _noise(3, 3), sh['vocab'])
    want = O.finish(scene, indices, images)
    assert (want != scene['sketch']).any() and np.array_equal(got, want)
    with open(os.path.join(res, 'scene.json')) as fp:
        facts = json.load(fp)
    v, hc = O.road_counts(sketches[2])
    assert facts == {'text': PROCESSED, 'instances': indices, 'classes': [15, 27, 36], 'boxes': [scene['boxes'][k].tolist() for k in indices],
                     'roads': [None, None, {'V': v, 'Hc': hc}]}
