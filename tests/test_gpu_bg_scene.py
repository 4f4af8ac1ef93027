"""The scene background on the device: ssc_bg_scene_crop_u8 (hip.bg_scene_crop_u8), ssc_bg_scene_compose_u8
(hip.bg_scene_compose_u8, hip.bg_scene_overlay_u8), ssc_bg_sky_gradient_u8 (hip.bg_sky_gradient_u8) and bg_colorization_main.py
--mode scene on top of them, against the float64 NumPy oracle tests/bg_scene_oracle.py.

Every comparison is byte-exact: the kernels' arithmetic is IEEE basic operations in fp32 (the cast, each rounded on its own)
and float64 (the gradient, contraction off), a floor, compares and integer steps, the same operations in the same order as the
oracle's NumPy.  Outputs sit inside buffers filled with a sentinel byte; every launch runs twice.

Shapes: 16 x 16; 40 x 52 (M a multiple of 4, rows not 16-byte aligned after the one-pixel shift); 37 x 29 (M % 4 = 1: the short
last group); 768 x 768 once.  The gradient at 32 x 32 and 40 x 52 and once at 768 x 768."""
import faulthandler
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
from PIL import Image

import bg_scene_oracle as O

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VOCAB = os.path.join(ROOT, 'tests', 'golden', 'bg_aug', 'bg_vocab.txt')
F = np.float32
SENTINEL = 0xA5
PAD = 16
CHILD_LIMIT = 180               # seconds a command-line child may take (start-up of a fresh process included)
SHAPES = [(16, 16), (40, 52), (37, 29), (768, 768)]


@pytest.fixture(autouse=True)
def _time_limit():
    """A test that hangs on the device ends the process (with every thread's traceback) instead of holding the card."""
    faulthandler.dump_traceback_later(400, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _out(h, w):
    """A uint8 [h,w,3] output inside a sentinel-filled buffer -> (the view, the buffer)."""
    raw = torch.full((h * w * 3 + 2 * PAD,), SENTINEL, dtype=torch.uint8, device='cuda')
    return raw[PAD:PAD + h * w * 3].view(h, w, 3), raw


def _around_intact(raw):
    g = raw.cpu().numpy()
    return (g[:PAD] == SENTINEL).all() and (g[-PAD:] == SENTINEL).all()


def _untouched(raw):
    return (raw.cpu().numpy() == SENTINEL).all()


def _scene(rng, h, w):
    """inner with background, instances 1, 2 (grass), 3 and 255; a sketch with random strokes (red byte 0, other bytes anything),
    grey pixels (red byte not 0), and strokes in row 0, column 0, the last row and the last column; 255 class ids."""
    inner = np.zeros((h, w), np.uint8)
    inner[h // 4:h // 2, w // 8:w // 2] = 1
    inner[h // 2:h - 1, w // 3:w] = 2
    inner[1:h // 4, w // 2:w - 2] = 3
    inner[h - 3:h, 0:w // 4] = 255
    inner[rng.rand(h, w) < 0.03] = 0
    ids = np.full(255, 15, np.int32)
    ids[1] = O.GRASS_LABEL
    sketch = rng.randint(1, 256, (h, w, 3)).astype(np.uint8)
    strokes = rng.rand(h, w) < 0.25
    sketch[strokes, 0] = 0
    sketch[0, ::2, 0] = 0
    sketch[::3, 0, 0] = 0
    sketch[h - 1, :, 0] = 0
    sketch[:, w - 1, 0] = 0
    return inner, ids, sketch


def _generator_image(rng, h, w, ld):
    """[1,h,w,ld] with the image in channels 0..2: uniform values, some below -1, above 1 and NaN; 1e3 in the padding."""
    img = rng.uniform(-1.1, 1.1, (h, w, 3)).astype(F)
    flat = img.reshape(-1)
    where = rng.choice(flat.size, max(8, flat.size // 10), replace=False)
    flat[where] = np.array([-1.0, 1.0, -1.5, 1.5, np.nan, 3.0, -3.0, np.inf], F)[np.arange(where.size) % 8]
    buf = np.full((1, h, w, ld), 1.0e3, F)
    buf[0, ..., :3] = img
    return buf


@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: '%dx%d' % s)
def test_crop(shape):
    from sketchyscenecolorization_amd import hip
    h, w = shape
    rng = np.random.RandomState(h * 1000 + w)
    inner, _, _ = _scene(rng, h, w)
    prev = rng.randint(0, 256, (h, w, 3)).astype(np.uint8)
    want = O.crop(prev, inner)
    assert (inner == 255).any() and (inner == 0).any()
    out, raw = _out(h, w)
    got = hip.bg_scene_crop_u8(_dev(prev), _dev(inner), out=out)
    assert got is out and np.array_equal(out.cpu().numpy(), want) and _around_intact(raw)
    assert np.array_equal(hip.bg_scene_crop_u8(_dev(prev), _dev(inner)).cpu().numpy(), want), 'the second launch differs'


@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: '%dx%d' % s)
def test_compose(shape):
    """Rows of 3, 4 and 8 floats (768 x 768: 4 only), and rows of 3 from a base off the 16-byte boundary: out and fg_marked are
    the oracle's bytes.  The scene holds every case by construction: strokes in row 0 and column 0 (not moved), on the last row
    and column (their move falls off), over a grass instance (not drawn) and a non-grass one (drawn), inner value 255."""
    from sketchyscenecolorization_amd import hip
    h, w = shape
    rng = np.random.RandomState(h * 1000 + w + 1)
    inner, ids, sketch = _scene(rng, h, w)
    grass = O.grass_table(ids)
    fg = O.crop(rng.randint(0, 256, (h, w, 3)).astype(np.uint8), inner)
    moved_red = O.moved(sketch)[:, :, 0]
    assert grass[2] == 1 and grass.sum() == 1
    assert ((moved_red == 0) & (inner == 2)).any() and ((moved_red == 0) & (inner == 1)).any() and ((moved_red == 0) & (inner == 255)).any()
    assert (moved_red[0] == 0).any() and (moved_red[:, 0] == 0).any() and (moved_red[0] == sketch[0, :, 0]).all()
    assert (moved_red[1:, 1:] != sketch[1:, 1:, 0]).any()
    region = O.drawn_region(sketch, inner, grass)
    assert not region[inner == 2].any() and region[inner == 255].any()
    inner_d, grass_d, sketch_d, fg_d = _dev(inner), _dev(grass), _dev(sketch), _dev(fg)
    for ld, shift in ((4, 0),) if h == 768 else ((3, 0), (3, 1), (4, 0), (4, 1), (8, 0)):
        img = _generator_image(rng, h, w, ld)
        assert np.isnan(img).any() and (img[..., :3] > 1).any() and (img[..., :3] < -1).any()
        want, want_marked = O.compose(img[0], fg, inner, grass, sketch)
        rawf = torch.full((img.size + 8,), float('nan'), dtype=torch.float32, device='cuda')
        t = rawf[shift:shift + img.size].view(img.shape)
        t.copy_(torch.from_numpy(img))
        for again in range(2):
            (out, raw), (marked, raw_m) = _out(h, w), _out(h, w)
            a, b = hip.bg_scene_compose_u8(t, fg_d, inner_d, grass_d, sketch_d, out=out, fg_marked=marked)
            assert a is out and b is marked
            assert np.array_equal(out.cpu().numpy(), want), (shape, ld, shift, again)
            assert np.array_equal(marked.cpu().numpy(), want_marked), (shape, ld, shift, again)
            assert _around_intact(raw) and _around_intact(raw_m)
    assert np.array_equal(want_marked[~region], fg[~region]) and (want[region][:, 0] == 0).all()


@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: '%dx%d' % s)
def test_overlay_alone(shape):
    """The pass behind the gradient: only the drawn pixels of the image change."""
    from sketchyscenecolorization_amd import hip
    h, w = shape
    rng = np.random.RandomState(h * 1000 + w + 2)
    inner, ids, sketch = _scene(rng, h, w)
    grass = O.grass_table(ids)
    image = rng.randint(0, 256, (h, w, 3)).astype(np.uint8)
    want = O.overlay(image, sketch, inner, grass)
    for again in range(2):
        out, raw = _out(h, w)
        out.copy_(_dev(image))
        got = hip.bg_scene_overlay_u8(out, _dev(inner), _dev(grass), _dev(sketch))
        assert got is out and np.array_equal(out.cpu().numpy(), want) and _around_intact(raw), (shape, again)
    # no stroke at all (and a short last group): nothing changes
    blank = np.full((h, w, 3), 255, np.uint8)
    out, raw = _out(h, w)
    out.copy_(_dev(image))
    hip.bg_scene_overlay_u8(out, _dev(inner), _dev(grass), _dev(blank))
    assert np.array_equal(out.cpu().numpy(), image) and _around_intact(raw)


# ---------------------------------------------------------------------------------------------------------------
# the gradient
# ---------------------------------------------------------------------------------------------------------------
SKY, GROUND, OTHER, THIRD = (60, 120, 200), (30, 150, 40), (200, 90, 30), (9, 8, 7)


def _two_bands(h, w, sky, rows, ground=GROUND):
    color = np.empty((h, w, 3), np.uint8)
    color[:rows] = sky
    color[rows:] = ground
    return color


def _some_instances(h, w):
    inner = np.zeros((h, w), np.uint8)
    inner[3:9, 2:w // 3] = 1
    inner[h // 3:h // 3 + 5, w // 2:w - 1] = 7
    inner[h - 4:h - 1, 1:w - 3] = 255
    return inner


def gradient_case(name, h, w):
    """-> (color, inner, search_from, search_height, what the case must show: a dict compared with the oracle's facts)."""
    rng = np.random.RandomState(h * 7 + w + sum(map(ord, name)))
    inner = _some_instances(h, w)
    sf, sh_, show = 5, 2, {'status': 0}
    color = _two_bands(h, w, SKY, h // 2 - 2)
    color[inner != 0] = OTHER
    if name in ('tie', 'tie_reversed'):
        # SKY and OTHER cover as many background pixels of rows 5 and 6; THIRD is met first but is rarer
        inner[5:7] = 0
        first, second = (SKY, OTHER) if name == 'tie' else (OTHER, SKY)
        color[5], color[6] = first, second
        color[5, 0] = color[6, 0] = THIRD
        color[h // 2 - 3] = SKY
        show['sky_color'] = list(first)
    elif name == 'partly_foreground':
        # counted with the instance pixels OTHER would win rows 5 and 6; without them SKY does
        inner[5:7] = 0
        inner[5:7, :w // 2 + 2] = 1
        color[5:7, :w // 2 + 2] = OTHER
        show['sky_color'] = list(SKY)
    elif name == 'all_foreground':
        inner[5:7] = 3
        show['status'] = 1
    elif name == 'sky_in_row_0_only':
        sf, sh_ = 0, 1
        inner[:] = 0
        color = _two_bands(h, w, SKY, 1)
        show.update(status=2, sky_bottom=0)
    elif name in ('bottom_2', 'bottom_3'):
        sf, sh_ = 2, 1
        rows = 3 if name == 'bottom_2' else 4
        inner[:rows + 1] = 0
        color = _two_bands(h, w, SKY, rows)
        color[inner != 0] = OTHER
        show.update(sky_bottom=rows - 1, start_height=rows - 2)
    elif name == 'grey':
        color[color[..., 0] == SKY[0]] = (120, 120, 120)
        show['sky_color'] = [120, 120, 120]
    elif name == 'black':
        color[color[..., 0] == SKY[0]] = (0, 0, 0)
        show['sky_color'] = [0, 0, 0]
    elif name == 'white':
        # the sky band ends at row 7; the white-filled instance pixels below it match the sky colour down to row h/2
        color = _two_bands(h, w, (255, 255, 255), 8)
        inner[:] = 0
        inner[7:h // 2 + 3, 1:4] = 2
        color[inner != 0] = OTHER
        show.update(sky_color=[255, 255, 255], sky_bottom=h // 2)
    elif name == 'bright':
        color[color[..., 0] == SKY[0]] = (100, 150, 230)        # 1.5 * 230 / 255 > 1
        show['sky_color'] = [100, 150, 230]
    elif name == 'equal_maxima':
        a, b = rng.randint(1, 256, (2, h, w))
        hi, lo = np.maximum(a, b), np.minimum(a, b) - 1
        kinds = rng.randint(0, 5, (h, w))
        tied = np.stack([np.where(kinds == 1, lo, hi), np.where(kinds == 2, lo, hi), np.where(kinds == 0, lo, hi)], -1)
        tied[kinds == 3] = hi[kinds == 3][:, None]          # r == g == b
        keep = kinds == 4                                   # the bands as they are
        color = np.where(keep[..., None], color, tied).astype(np.uint8)
        color[5:7] = np.where(inner[5:7, :, None] == 0, np.array(SKY, np.uint8), color[5:7])
        show['sky_color'] = list(SKY)
    elif name == 'random':
        color = rng.randint(0, 256, (h, w, 3)).astype(np.uint8)
        inner = (rng.rand(h, w) < 0.3).astype(np.uint8) * rng.randint(1, 256, (h, w)).astype(np.uint8)
    else:
        raise KeyError(name)
    return np.ascontiguousarray(color), inner, sf, sh_, show


CASES = ['tie', 'tie_reversed', 'partly_foreground', 'all_foreground', 'sky_in_row_0_only', 'bottom_2', 'bottom_3', 'grey',
         'black', 'white', 'bright', 'equal_maxima', 'random']


def _check_gradient(name, h, w):
    from sketchyscenecolorization_amd import hip
    color, inner, sf, sh_, show = gradient_case(name, h, w)
    want, status, facts = O.sky_gradient(color, inner, sf, sh_)
    assert status == show['status'], (name, status, facts)
    for k in ('sky_color', 'sky_bottom', 'start_height'):
        if k in show:
            assert facts[k] == show[k], (name, k, facts)
    if status != 0:
        assert np.array_equal(want, color)
    elif name != 'black':       # a black sky stays black: v = 0 at both ends of the gradient
        assert (want != color).any()
    color_d, inner_d = _dev(color), _dev(inner)
    results = []
    for again in range(2):
        out, raw = _out(h, w)
        st = torch.full((3,), -77, dtype=torch.int32, device='cuda')
        got, got_st, info = hip.bg_sky_gradient_u8(color_d, inner_d, sf, sh_, out=out, status=st[1:2])
        assert got is out
        assert st.cpu().tolist() == [-77, status, -77], (name, st.cpu().tolist())
        got_np = out.cpu().numpy()
        bad = np.argwhere((got_np != want).any(-1))
        assert bad.size == 0, (name, (h, w), again, len(bad), bad[:4].tolist(),
                               [(got_np[tuple(i)].tolist(), want[tuple(i)].tolist(), color[tuple(i)].tolist()) for i in bad[:4]])
        assert _around_intact(raw)
        info = info.cpu().numpy()
        if status == 0:
            c = int(info[0])
            assert [c & 255, (c >> 8) & 255, (c >> 16) & 255] == facts['sky_color']
            assert (int(info[1]), int(info[2])) == (facts['sky_bottom'], facts['start_height'])
        results.append(got_np)
    assert np.array_equal(results[0], results[1])
    return want, color, inner, facts


@pytest.mark.parametrize('shape', [(32, 32), (40, 52)], ids=lambda s: '%dx%d' % s)
@pytest.mark.parametrize('name', CASES)
def test_gradient(name, shape):
    want, color, inner, facts = _check_gradient(name, *shape)
    assert np.array_equal(want[inner != 0], color[inner != 0])
    if name == 'equal_maxima':
        c = color[inner == 0].astype(int)
        r, g, b = c[:, 0], c[:, 1], c[:, 2]
        assert ((r == g) & (g > b)).any() and ((g == b) & (b > r)).any() and ((r == b) & (b > g)).any() and ((r == g) & (g == b)).any()
    if name == 'bright':
        assert want[0, 0].max() == 255


def test_gradient_768():
    """One full-size image: the bands of a scene with instances, the lower half random bytes, equal-channel colours sprinkled in."""
    h = w = 768
    rng = np.random.RandomState(768)
    from sketchyscenecolorization_amd import hip
    color = _two_bands(h, w, SKY, 300)
    color[400:] = rng.randint(0, 256, (h - 400, w, 3))
    grey = rng.rand(h, w) < 0.05
    color[grey] = color[grey][:, :1]
    inner = np.zeros((h, w), np.uint8)
    inner[100:260, 50:300] = 1
    inner[340:700, 400:760] = 2
    inner[4:8, 0:700] = 9
    color[inner != 0] = rng.randint(0, 256, (int((inner != 0).sum()), 3))
    want, status, facts = O.sky_gradient(color, inner)
    assert status == 0 and facts == {'sky_color': list(SKY), 'sky_bottom': 299, 'start_height': 224}
    for again in range(2):
        out, raw = _out(h, w)
        _, st, info = hip.bg_sky_gradient_u8(_dev(color), _dev(inner), out=out)
        assert int(st.cpu()[0]) == 0 and info.cpu().tolist()[1:] == [299, 224, 0]
        assert np.array_equal(out.cpu().numpy(), want) and _around_intact(raw), again


def test_entry_points_refuse_bad_arguments_without_launching():
    from sketchyscenecolorization_amd import hip
    h, w = 32, 40
    rng = np.random.RandomState(3)
    color, inner = _dev(rng.randint(0, 256, (h, w, 3)).astype(np.uint8)), _dev(np.zeros((h, w), np.uint8))
    sketch, grass = _dev(np.zeros((h, w, 3), np.uint8)), _dev(np.zeros(256, np.uint8))
    img = _dev(rng.uniform(-1, 1, (h, w, 4)).astype(F))
    (out, raw), (marked, raw_m) = _out(h, w), _out(h, w)
    status = torch.full((4,), -77, dtype=torch.int32, device='cuda')
    ws = torch.full((64,), -5, dtype=torch.int32, device='cuda')
    off = lambda t, nbytes: hip.ptr(t.view(-1).view(torch.uint8)[nbytes:])      # noqa: E731
    L = hip.lib()
    names = ('color', 'inner', 'H', 'W', 'search_from', 'search_height', 'out', 'status', 'ws', 'ws_bytes')
    base = dict(color=hip.ptr(color), inner=hip.ptr(inner), H=h, W=w, search_from=5, search_height=2, out=hip.ptr(out),
                status=hip.ptr(status), ws=hip.ptr(ws), ws_bytes=256)
    grad = lambda **kw: L.ssc_bg_sky_gradient_u8(*([kw.get(k, base[k]) for k in names] + [hip.stream_ptr()]))    # noqa: E731
    assert grad(search_height=0) == -1 and grad(search_height=-1) == -1 and grad(search_from=-1) == -1
    assert grad(search_from=16, search_height=2) == -1 and grad(search_from=17, search_height=1) == -1      # past row H/2 = 16
    assert grad(search_from=0, search_height=18) == -1
    assert grad(H=0) == -1 and grad(W=0) == -1 and grad(W=5000, search_height=2) == -1
    assert grad(color=None) == -1 and grad(inner=None) == -1 and grad(out=None) == -1 and grad(status=None) == -1
    assert grad(ws_bytes=15) == -2 and grad(ws_bytes=0) == -2 and grad(ws=None) == -2 and grad(ws=off(ws, 2)) == -2
    assert grad(color=off(color, 1)) == -3 and grad(inner=off(inner, 2)) == -3 and grad(out=off(raw, PAD + 1)) == -3
    assert grad(status=off(status, 2)) == -3
    cnames = ('img', 'ldc', 'fg', 'inner', 'grass', 'sketch', 'H', 'W', 'out', 'marked', 'overlay')
    cbase = dict(img=hip.ptr(img), ldc=4, fg=hip.ptr(color), inner=hip.ptr(inner), grass=hip.ptr(grass), sketch=hip.ptr(sketch),
                 H=h, W=w, out=hip.ptr(out), marked=hip.ptr(marked), overlay=0)
    comp = lambda **kw: L.ssc_bg_scene_compose_u8(*([kw.get(k, cbase[k]) for k in cnames] + [hip.stream_ptr()]))     # noqa: E731
    assert comp(H=0) == -1 and comp(W=-1) == -1 and comp(ldc=2) == -1 and comp(img=None) == -1 and comp(fg=None) == -1
    assert comp(marked=None) == -1 and comp(grass=None) == -1 and comp(sketch=None) == -1 and comp(out=None, overlay=1) == -1
    assert comp(out=off(raw, PAD + 2)) == -3 and comp(marked=off(raw_m, PAD + 1)) == -3 and comp(inner=off(inner, 1)) == -3
    assert comp(fg=off(color, 3)) == -3 and comp(img=off(img, 2)) == -3 and comp(out=off(raw, PAD + 2), overlay=1) == -3
    crop = lambda prev, inn, m, o: L.ssc_bg_scene_crop_u8(prev, inn, m, o, hip.stream_ptr())      # noqa: E731
    assert crop(hip.ptr(color), hip.ptr(inner), 0, hip.ptr(out)) == -1 and crop(None, hip.ptr(inner), h * w, hip.ptr(out)) == -1
    assert crop(hip.ptr(color), hip.ptr(inner), (1 << 24) + 1, hip.ptr(out)) == -1
    assert crop(off(color, 1), hip.ptr(inner), h * w, hip.ptr(out)) == -3 and crop(hip.ptr(color), off(inner, 2), h * w, hip.ptr(out)) == -3
    assert crop(hip.ptr(color), hip.ptr(inner), h * w, off(raw, PAD + 3)) == -3
    torch.cuda.synchronize()
    assert _untouched(raw) and _untouched(raw_m) and (status.cpu().numpy() == -77).all() and (ws.cpu().numpy() == -5).all()
    # and the same calls go through once the argument is right
    assert grad() == 0 and comp() == 0 and comp(img=None, fg=None, marked=None, ldc=0, overlay=1) == 0
    assert crop(hip.ptr(color), hip.ptr(inner), h * w, hip.ptr(out)) == 0
    torch.cuda.synchronize()
    assert status.cpu().tolist()[1:] == [-77] * 3 and status.cpu().tolist()[0] in (0, 1, 2) and _around_intact(raw)


# ---------------------------------------------------------------------------------------------------------------
# the command line
# ---------------------------------------------------------------------------------------------------------------
SIZE = 32
ID = '4711'
FIRST = 'the sky is red and the ground is yellow'
SECOND = 'the sky is pink'


def _cli_scene():
    """A 32 x 32 scene: a house (class 15) that reaches into rows 5 and 6, grass (class 27) along the bottom, strokes on both."""
    inner = np.zeros((SIZE, SIZE), np.uint8)
    inner[4:14, 3:12] = 1
    inner[24:SIZE, 6:SIZE] = 2
    inner[16:22, 20:30] = 3
    sketch = np.full((SIZE, SIZE, 3), 255, np.uint8)
    sketch[4, 3:12] = sketch[13, 3:12] = 0
    sketch[4:14, 3] = sketch[4:14, 11] = 0
    sketch[26, 8:30] = 0
    sketch[16:22, 20] = sketch[16, 20:30] = 0
    sketch[0, 5:9] = 0
    sketch[10:20, 0] = 0
    sketch[SIZE - 1, :] = 0
    sketch[2, 15:25] = (90, 90, 90)
    return sketch, inner, np.array([15, O.GRASS_LABEL, 3], np.int32)


def _child(cwd, argv):
    code = ('import random, sys; sys.path.insert(0, %r); random.seed(31); import bg_colorization_main as m; m.main(%r)'
            % (ROOT, list(argv)))
    r = subprocess.run([sys.executable, '-c', code], cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       universal_newlines=True, timeout=CHILD_LIMIT)
    assert r.returncode == 0, r.stdout[-4000:]
    return r.stdout


def _read(res_dir):
    with open(os.path.join(res_dir, 'scene.json')) as fp:
        facts = json.load(fp)
    return (np.array(Image.open(os.path.join(res_dir, ID + '_bg.png')).convert('RGB')),
            np.array(Image.open(os.path.join(res_dir, ID + '_fg.png')).convert('RGB')), facts, sorted(os.listdir(res_dir)))


_RUNS = {}


def _runs(tmp_path_factory):
    """Two training steps at 32 x 32 on the synthetic scenes, then three --mode scene runs, each a process of its own under its
    own time limit; a failing one ends the chain (its assert raises)."""
    if not _RUNS:
        import scipy.io
        cwd = str(tmp_path_factory.mktemp('bg-scene-cli'))
        sketch, inner, ids = _cli_scene()
        for d in ('sketches', 'inner_masks', 'seg_data'):
            os.makedirs(os.path.join(cwd, 'scene', d))
        Image.fromarray(sketch, 'RGB').save(os.path.join(cwd, 'scene', 'sketches', ID + '.png'))
        scipy.io.savemat(os.path.join(cwd, 'scene', 'inner_masks', ID + '.mat'), {'inner_masks': inner})
        np.savez(os.path.join(cwd, 'scene', 'seg_data', ID + '_datas.npz'), pred_class_ids=ids)
        common = ['--image_size', str(SIZE), '--vocab_file', VOCAB]
        _child(cwd, ['--mode', 'train', '--max_steps', '2', '--save_freq', '2', '--progress_freq', '0', '--summary_freq', '0',
                     '--data_base_dir', 'data'] + common)
        stamps = sorted(os.listdir(os.path.join(cwd, 'outputs')))
        assert len(stamps) == 1
        run = os.path.join(cwd, 'outputs', stamps[0])
        res = os.path.join(run, 'scene_results', ID)
        scene = ['--mode', 'scene', '--resume_from', stamps[0], '--scene_dir', 'scene', '--image_id', ID] + common
        out1 = _child(cwd, scene + ['--instruction', FIRST])
        first = _read(res)
        prev = os.path.join(cwd, 'first_bg.png')
        os.replace(os.path.join(res, ID + '_bg.png'), prev)
        out2 = _child(cwd, scene + ['--instruction', SECOND, '--previous_image', prev, '--previous_text', first[2]['text']])
        second = _read(res)
        out3 = _child(cwd, scene + ['--instruction', FIRST, '--color_gradient', '0'])
        flat = _read(res)
        _RUNS.update(run=run, first=first, second=second, flat=flat, out=(out1, out2, out3), scene=(sketch, inner, ids))
    return _RUNS


def _independent(run, text, prev, gradient):
    """The snapshot in a fresh trainer, the oracle's crop, one forward pass under another tag, the oracle's finishing."""
    from sketchyscenecolorization_amd import hip
    from sketchyscenecolorization_amd.bg_colorization import BGTrainer
    from sketchyscenecolorization_amd.data_processing.text_processing import load_vocab_dict_from_file, preprocess_sentence
    sketch, inner, ids = _RUNS['scene']
    if 'trainer' not in _RUNS:
        tr = BGTrainer(image_size=SIZE, max_steps=2, seed=1)
        tr.store.load_state_dict(torch.load(os.path.join(run, 'snapshot', 'snapshot-2'), map_location='cpu'))
        _RUNS['trainer'] = tr
    tr = _RUNS['trainer']
    fg = _dev(O.crop(prev, inner)[None])
    x = torch.empty((1, SIZE, SIZE, 3), dtype=torch.float32, device='cuda')
    y, xd, cnt = torch.empty_like(x), torch.empty((1, SIZE, SIZE, 8), dtype=torch.float32, device='cuda'), torch.empty(1, device='cuda')
    hip.bg_stage_u8(fg, fg, torch.zeros((1, SIZE, SIZE), dtype=torch.int32, device='cuda'), x, y, xd, cnt)
    tok = np.array(preprocess_sentence(text, load_vocab_dict_from_file(VOCAB), 8), dtype=np.int32)[None]
    img = tr.G.forward(x, tok, None, 'independent')['image'].cpu().numpy()[0]
    return O.finish(img, prev, inner, ids, sketch, gradient)


def test_command_line_first_instruction(tmp_path_factory):
    r = _runs(tmp_path_factory)
    sketch, inner, ids = r['scene']
    bg, fg, facts, files = r['first']
    assert files == sorted([ID + '_bg.png', ID + '_fg.png', 'scene.json'])
    want_bg, want_fg, status, info = _independent(r['run'], FIRST, sketch, True)
    assert status == 0
    assert np.array_equal(fg, want_fg) and np.array_equal(bg, want_bg)
    assert facts == {'text': FIRST, 'color_gradient': 1, 'sky_color': info['sky_color'], 'sky_bottom': info['sky_bottom'],
                     'start_height': info['start_height']}
    assert 'proc_input_text: ' + FIRST in r['out'][0] and 'iter_from 2' in r['out'][0]
    # strokes over the house are drawn, the ones over the grass are not; the instances carry the previous image (the sketch)
    assert bg[5, 4].tolist() == [0, 0, 0] and bg[27, 9].tolist() == sketch[27, 9].tolist() == [255, 255, 255]
    assert fg[27, 9].tolist() == [255, 255, 255] and fg[0, 5].tolist() == [0, 0, 0]


def test_command_line_second_instruction_splices_the_text(tmp_path_factory):
    r = _runs(tmp_path_factory)
    bg, fg, facts, _ = r['second']
    text = 'the sky is pink and the ground is yellow'
    want_bg, want_fg, status, info = _independent(r['run'], text, r['first'][0], True)
    assert status == 0 and facts['text'] == text and 'proc_input_text: ' + text in r['out'][1]
    assert np.array_equal(fg, want_fg) and np.array_equal(bg, want_bg)
    assert facts['sky_color'] == info['sky_color'] and facts['start_height'] == info['start_height']
    sketch, inner, ids = r['scene']
    kept = (inner != 0) & ~O.drawn_region(sketch, inner, O.grass_table(ids))
    assert np.array_equal(fg[kept], r['first'][0][kept])        # the instances carry the previous result


def test_command_line_without_the_gradient(tmp_path_factory):
    r = _runs(tmp_path_factory)
    bg, fg, facts, _ = r['flat']
    want_bg, want_fg, _, _ = _independent(r['run'], FIRST, r['scene'][0], False)
    assert np.array_equal(fg, want_fg) and np.array_equal(bg, want_bg)
    assert facts == {'text': FIRST, 'color_gradient': 0, 'sky_color': None, 'sky_bottom': None, 'start_height': None}
    assert np.array_equal(fg, r['first'][1]) and (bg != r['first'][0]).any()
