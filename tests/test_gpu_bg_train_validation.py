"""Scoring a held-out set during Background training: the two kernels of the pass -- ssc_image_metrics_bg_f32
(hip.image_metrics_bg_f32) and ssc_seg_confusion (hip.seg_confusion) -- and bg_colorization_main.py --val_freq on top of them.

The image kernel is DEFINED by a composition: its five sums are the bits of image_metrics_u8(bg_finish_u8(img, fg, mask), target,
mask).  So its tests compare 64-bit patterns; the oracle test takes its tolerances from tests/test_gpu_image_metrics.py (the
four integer rows exact, the SSIM mean to 1e-9: derived there).  The tile is 24 x 32 pixels with a 5-pixel halo: 10 x 13 has no
window, 11 x 11 exactly one, 24 x 32 is one full tile, 25 x 33 four tiles of which three hold one row or column, 50 x 70 is 3 x 3
tiles.  The confusion kernel counts integers: equality with NumPy is exact.  A workgroup takes 1024 pixels before a sample gets
a second one, so P = 4097 runs five workgroups per sample whose threads loop, the last one over a single pixel.

The training tests run the command line in child processes at 32 x 32 on three flat-coloured train scenes and three val scenes
written as PNG files."""
import faulthandler
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
from PIL import Image

import metrics_oracle as MO

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VOCAB = os.path.join(ROOT, 'tests', 'golden', 'bg_aug', 'bg_vocab.txt')
F = np.float32
SSIM_TOL = 1e-9                 # tests/test_gpu_image_metrics.py
EXACT = [0, 1, 2, 4]
SHAPES = [(10, 13), (11, 11), (24, 32), (25, 33), (50, 70)]
SENTINEL = -7.25
CHILD_LIMIT = 180               # seconds a command-line child may take (start-up of a fresh process included)


@pytest.fixture(autouse=True)
def _time_limit():
    """A test that hangs on the device ends the process (with every thread's traceback) instead of holding the card."""
    faulthandler.dump_traceback_later(400, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


# ---------------------------------------------------------------------------------------------------------------
# (a) the image kernel
# ---------------------------------------------------------------------------------------------------------------
def _sprinkle(rng, x):
    """-1, 1, +-1.5, +-3, NaN and +-inf at random places (about one value in 12)."""
    flat = x.reshape(-1)
    special = np.array([-1.0, 1.0, 1.5, -1.5, np.nan, np.inf, -np.inf, 3.0, -3.0], F)
    where = rng.choice(flat.size, max(9, flat.size // 12), replace=False)
    flat[where] = special[np.arange(where.size) % special.size]
    return x


def _uniform(rng, shape):
    return _sprinkle(rng, rng.uniform(-1.2, 1.2, shape).astype(F))


def _rounding_points(rng, shape, sprinkle=True):
    """The x at which (x + 1) / 2 * 255 + 0.5 lands on an integer -- x = (k - 0.5) / 255 * 2 - 1, k = 0 .. 256 -- and at which
    (x + 1) / 2 * 255 does (k / 255 * 2 - 1), with their fp32 neighbours on both sides: another rounding of one of the five
    operations, or a fused multiply-add, shows here."""
    k = np.arange(257, dtype=np.float64)
    pts = np.concatenate([(k - 0.5) / 255.0 * 2.0 - 1.0, k[:256] / 255.0 * 2.0 - 1.0]).astype(F)
    pts = np.concatenate([pts, np.nextafter(pts, F(-4)), np.nextafter(pts, F(4))]).astype(F)
    x = np.resize(pts, int(np.prod(shape)))
    rng.shuffle(x)
    x = x.reshape(shape)
    return _sprinkle(rng, x) if sprinkle else x


def _rows_of(img, ld, shift=0):
    """img [N,H,W,3] in channels 0..2 of rows of ld floats (1.0e3 in the padding channels), on the device, its base ``shift``
    floats behind a 16-byte boundary, NaN in front of it and behind it."""
    buf = np.full(img.shape[:3] + (ld,), 1.0e3, F)
    buf[..., :3] = img
    raw = torch.full((buf.size + 8,), float('nan'), dtype=torch.float32, device='cuda')
    t = raw[shift:shift + buf.size].view(buf.shape)
    t.copy_(torch.from_numpy(buf))
    assert t.is_contiguous() and t.data_ptr() % 16 == 4 * shift
    return t


def _masks(rng, n, h, w):
    mixed = rng.choice(np.array([0, 128, 255, 1], np.uint8), (n, h, w), p=[.35, .3, .3, .05])
    mixed.reshape(n, -1)[:, :2] = (0, 255)
    return {'null': None, 'zero': np.zeros((n, h, w), np.uint8), 'nonzero': rng.randint(1, 256, (n, h, w)).astype(np.uint8),
            'mixed': mixed}


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _bits(t):
    return t.cpu().numpy().view(np.int64)


def _out(n, width=5, dtype=torch.float64, fill=SENTINEL):
    """An [n, width] output inside a sentinel-filled buffer -> (the view, the buffer)."""
    raw = torch.full((n * width + 16,), fill, dtype=dtype, device='cuda')
    return raw[8:8 + n * width].view(n, width), raw


def _around_intact(raw, count):
    g = raw.cpu().numpy()
    return (g[:8] == SENTINEL).all() and (g[8 + count:] == SENTINEL).all()


@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: '%dx%d' % s)
def test_image_kernel_is_the_composed_route_bit_for_bit(shape):
    """N = 1 and 3; rows of 3, 4 and 8 floats, and each of them again from a base one float off the 16-byte boundary; no mask,
    an all-zero, an all-non-zero and a mixed one; uniform values and the rounding points, both with NaN, infinities and values
    outside [-1, 1]: the rows are the bits of the uint8 kernel on bg_finish_u8's image, a second call gives them again, and
    nothing around the output is written."""
    from sketchyscenecolorization_amd import hip
    h, w = shape
    for n in (1, 3):
        rng = np.random.RandomState(1000 * h + 10 * w + n)
        fg, target = [_dev(rng.randint(0, 256, (n, h, w, 3)).astype(np.uint8)) for _ in range(2)]
        masks = _masks(rng, n, h, w)
        for make in (_uniform, _rounding_points):
            img = make(rng, (n, h, w, 3))
            aligned3 = _rows_of(img, 3)
            for mname, mask in masks.items():
                m = _dev(mask)
                want = hip.image_metrics_u8(hip.bg_finish_u8(aligned3, fg if m is not None else None, m), target, m)
                for ld in (3, 4, 8):
                    for shift in (0, 1):
                        what = (shape, n, make.__name__, mname, ld, shift)
                        t = _rows_of(img, ld, shift)
                        out, raw = _out(n)
                        got = hip.image_metrics_bg_f32(t, fg if (m is not None or ld == 4) else None, target, m, out=out)
                        assert got is out and np.isfinite(out.cpu().numpy()).all(), what
                        assert np.array_equal(_bits(out), _bits(want)), (what, out.cpu().numpy(), want.cpu().numpy())
                        assert _around_intact(raw, n * 5), what
                        assert np.array_equal(_bits(hip.image_metrics_bg_f32(t, fg, target, m)), _bits(want)), what
                rows = want.cpu().numpy()
                counted = h * w if mask is None else np.count_nonzero(mask.reshape(n, -1), axis=1)
                assert (rows[:, 2] == counted).all(), (mname, rows)
                if mname == 'zero':
                    assert not rows.any()
                if mname in ('null', 'nonzero'):
                    assert (rows[:, 4] == (max(h - 10, 0) * max(w - 10, 0))).all()
        # the composed route itself takes rows of 4 and 8 floats to the same image (the kernel's reference is not one layout's)
        assert torch.equal(hip.bg_finish_u8(_rows_of(img, 4), fg, _dev(masks['mixed'])),
                           hip.bg_finish_u8(aligned3, fg, _dev(masks['mixed'])))


def test_image_kernel_pastes_and_rounds_as_stated():
    """Spelt out in NumPy on a case small enough to read: the rounded value floor(clamp((x+1)/2, 0, 1)*255 + 0.5) in fp32, NaN
    to 0, the foreground byte where the mask is 0 -- and the sums over the counted pixels only."""
    from sketchyscenecolorization_amd import hip
    rng = np.random.RandomState(5)
    n, h, w = 2, 10, 13
    img = _rounding_points(rng, (n, h, w, 3))
    fg = rng.randint(0, 256, (n, h, w, 3)).astype(np.uint8)
    target = rng.randint(0, 256, (n, h, w, 3)).astype(np.uint8)
    mask = _masks(rng, n, h, w)['mixed']
    with np.errstate(invalid='ignore'):
        y = np.minimum(np.maximum((img + F(1)) / F(2), F(0)), F(1)) * F(255)
        q = np.floor(y + F(0.5))
    q = np.where(np.isnan(img), 0, np.where(img > 1, 255, np.where(img < -1, 0, q))).astype(np.uint8)
    a = np.where((mask == 0)[..., None], fg, q)
    d = a.astype(np.int64) - target.astype(np.int64)
    keep = mask != 0
    got = hip.image_metrics_bg_f32(_rows_of(img, 4), _dev(fg), _dev(target), _dev(mask)).cpu().numpy()
    assert np.array_equal(hip.bg_finish_u8(_rows_of(img, 4), _dev(fg), _dev(mask)).cpu().numpy(), a)
    for i in range(n):
        assert got[i, 0] == np.abs(d[i])[keep[i]].sum() and got[i, 1] == (d[i] ** 2)[keep[i]].sum()
        assert got[i, 2] == keep[i].sum() and got[i, 3] == 0 and got[i, 4] == 0


@pytest.mark.parametrize('shape', [(25, 33), (50, 70)], ids=lambda s: '%dx%d' % s)
def test_image_kernel_against_the_float64_oracle(shape):
    """The uint8 images of the composed route read back and scored by tests/metrics_oracle.py in float64, with and without a
    mask: integers exact, the SSIM mean within 1e-9."""
    from sketchyscenecolorization_amd import hip, metrics as M
    h, w = shape
    rng = np.random.RandomState(7 * h + w)
    n = 3
    target = rng.randint(0, 256, (n, h, w, 3)).astype(np.uint8)
    img = np.stack([rng.uniform(-1, 1, (h, w, 3)).astype(F), _rounding_points(rng, (h, w, 3)),
                    np.clip(target[2].astype(F) / F(127.5) - F(1) + rng.uniform(-0.02, 0.02, (h, w, 3)).astype(F), -1, 1)])
    fg = rng.randint(0, 256, (n, h, w, 3)).astype(np.uint8)
    for mname, mask in _masks(rng, n, h, w).items():
        if mname == 'zero':
            continue
        m = _dev(mask)
        u8 = hip.bg_finish_u8(_rows_of(img, 3), _dev(fg) if m is not None else None, m).cpu().numpy()
        want = MO.rows(u8, target, M.ssim_window(), mask)
        for ld, shift in ((3, 0), (4, 0), (4, 1), (8, 0)):
            got = hip.image_metrics_bg_f32(_rows_of(img, ld, shift), _dev(fg), _dev(target), m).cpu().numpy()
            print('%dx%d mask %s ld %d shift %d: rows\n%r\noracle\n%r' % (h, w, mname, ld, shift, got, want))
            assert np.isfinite(got).all()
            assert np.array_equal(got[:, EXACT], want[:, EXACT]), (got[:, EXACT], want[:, EXACT])
            for i in range(n):
                assert want[i, 4] > 0
                err = abs(got[i, 3] - want[i, 3]) / (3.0 * want[i, 4])
                print('image %d: ssim %.15f, error %.3e (bound %.0e)' % (i, want[i, 3] / (3.0 * want[i, 4]), err, SSIM_TOL))
                assert err <= SSIM_TOL, (i, err)
        if mask is None:
            assert want[2, 3] / (3 * want[2, 4]) > 0.9 > want[0, 3] / (3 * want[0, 4])


def test_image_kernel_refuses_bad_arguments_without_launching():
    from sketchyscenecolorization_amd import hip, metrics as M
    n, h, w = 3, 25, 33
    rng = np.random.RandomState(1)
    img = _rows_of(_uniform(rng, (n, h, w, 3)), 4)
    fg, target = [_dev(rng.randint(0, 256, (n, h, w, 3)).astype(np.uint8)) for _ in range(2)]
    mask = _dev(_masks(rng, n, h, w)['mixed'])
    need = hip.image_metrics_workspace_bytes(n, h, w)
    assert need == n * 2 * 2 * 5 * 8
    win = torch.from_numpy(M.ssim_window()).cuda()
    ws = torch.zeros(need // 8, dtype=torch.float64, device='cuda')
    out, raw = _out(n)
    names = ('img', 'ldc', 'fg', 'target', 'mask', 'N', 'H', 'W', 'win', 'out', 'ws', 'ws_bytes')
    base = dict(img=hip.ptr(img), ldc=4, fg=hip.ptr(fg), target=hip.ptr(target), mask=hip.ptr(mask), N=n, H=h, W=w,
                win=hip.ptr(win), out=hip.ptr(out), ws=hip.ptr(ws), ws_bytes=need)
    call = lambda **kw: hip.lib().ssc_image_metrics_bg_f32(*([kw.get(k, base[k]) for k in names] + [hip.stream_ptr()]))  # noqa: E731
    off = lambda t, nbytes: hip.ptr(t.view(-1).view(torch.uint8)[nbytes:])      # noqa: E731
    assert call(ws_bytes=need - 1) == -2 and call(ws_bytes=0) == -2 and call(ws=None) == -2 and call(ws=off(ws, 4)) == -2
    assert call(out=off(raw, 8 * 8 + 4)) == -3 and call(win=off(win, 4)) == -3 and call(img=off(img, 2)) == -3
    assert call(ldc=2) == -1 and call(ldc=0) == -1 and call(ldc=-4) == -1
    assert call(N=0) == -1 and call(N=-2) == -1 and call(H=0) == -1 and call(W=0) == -1
    assert call(img=None) == -1 and call(target=None) == -1 and call(out=None) == -1 and call(fg=None) == -1
    torch.cuda.synchronize()
    assert (raw.cpu().numpy() == SENTINEL).all() and not ws.cpu().numpy().any()
    assert call(fg=None, mask=None) == 0        # without a mask nothing is pasted: no foreground needed
    torch.cuda.synchronize()
    assert np.array_equal(_bits(out), _bits(hip.image_metrics_u8(hip.bg_finish_u8(img), target)))
    assert call() == 0
    torch.cuda.synchronize()
    assert np.array_equal(_bits(out), _bits(hip.image_metrics_u8(hip.bg_finish_u8(img, fg, mask), target, mask)))
    assert _around_intact(raw, n * 5)


# ---------------------------------------------------------------------------------------------------------------
# (b) the confusion kernel
# ---------------------------------------------------------------------------------------------------------------
def confusion_np(logits, k, labels):
    """logits [N,P,ld], labels [N,P] -> int64 [N, k*k+1].  The prediction is the first index of the largest logit with NaN
    read as -inf (so a NaN never wins and a row of NaN predicts 0); labels outside [0, k) go to the last slot."""
    z = logits[..., :k].astype(np.float64)
    pred = np.argmax(np.where(np.isnan(z), -np.inf, z), axis=-1)
    out = np.zeros((logits.shape[0], k * k + 1), np.int64)
    lab = labels.astype(np.int64)
    cell = np.where((lab >= 0) & (lab < k), lab * k + pred, k * k)
    for n in range(logits.shape[0]):
        np.add.at(out[n], cell[n], 1)
    return out


def _confusion_inputs(rng, n, p, k, ld):
    """Logits from a handful of values (ties in most rows, NaN in many, some rows NaN throughout, +-inf), 1e9 in the padding
    column; labels from -1 .. k and two far values."""
    values = np.array([0.0, 0.5, 0.5, 1.0, -1.0, np.nan, np.inf, -np.inf, 2.25], F)
    logits = np.full((n, p, ld), 1.0e9, F)
    logits[..., :k] = values[rng.randint(0, values.size, (n, p, k))]
    logits[:, ::7, :k] = np.nan
    if p > 3:
        logits[:, 1, :k] = 0.5                      # all equal: index 0
        logits[:, 2, :k] = -np.inf
        logits[:, 3, :k] = [np.nan, 1.0, 1.0, 1.0][:k] if k > 1 else [np.nan]
    labels = rng.choice(np.array(list(range(-1, k + 1)) + [7, -2 ** 31], np.int64), (n, p)).astype(np.int32)
    return logits, labels


@pytest.mark.parametrize('kld', [(3, 3), (3, 4), (4, 4)], ids=lambda v: 'K%d-ld%d' % v)
@pytest.mark.parametrize('p', [1, 63, 64, 65, 4097])
def test_confusion_kernel_counts_what_numpy_counts(p, kld):
    from sketchyscenecolorization_amd import hip
    k, ld = kld
    for n in (1, 3):
        rng = np.random.RandomState(100 * p + 10 * k + ld + n)
        logits, labels = _confusion_inputs(rng, n, p, k, ld)
        want = confusion_np(logits, k, labels)
        assert want.sum() == n * p and (p < 63 or (want[:, -1] > 0).all())
        for shift in (0, 1):        # rows of 4 floats go as one 16-byte load on an aligned base, float by float elsewhere
            raw_l = torch.full((logits.size + 8,), float('nan'), dtype=torch.float32, device='cuda')
            t = raw_l[shift:shift + logits.size].view(logits.shape)
            t.copy_(torch.from_numpy(logits))
            out, raw = _out(n, k * k + 1, torch.int64, -7)
            got = hip.seg_confusion(t, _dev(labels), k, out=out)
            assert got is out and np.array_equal(out.cpu().numpy(), want), (p, k, ld, n, shift, out.cpu().numpy(), want)
            g = raw.cpu().numpy()
            assert (g[:8] == -7).all() and (g[8 + n * (k * k + 1):] == -7).all()
            assert np.array_equal(hip.seg_confusion(t, _dev(labels), k).cpu().numpy(), want), 'the second launch differs'


def test_confusion_kernel_on_the_shapes_of_the_pass():
    """[1, 32, 32, 3] logits and [1, 32, 32] labels as the generator and the stage kernel leave them; all classes by default."""
    from sketchyscenecolorization_amd import hip
    rng = np.random.RandomState(2)
    logits = np.maximum(rng.normal(0, 1, (1, 32, 32, 3)), 0).astype(F)      # after the relu: many zeros, many ties at 0
    labels = rng.randint(0, 3, (1, 32, 32)).astype(np.int32)
    want = confusion_np(logits.reshape(1, -1, 3), 3, labels.reshape(1, -1))
    assert np.array_equal(hip.seg_confusion(_dev(logits), _dev(labels)).cpu().numpy(), want) and want[0, -1] == 0


def test_confusion_kernel_refuses_bad_arguments_without_launching():
    from sketchyscenecolorization_amd import hip
    n, p, k = 3, 4097, 3
    rng = np.random.RandomState(4)
    logits, labels = _confusion_inputs(rng, n, p, k, 4)
    tl, tb = _dev(logits), _dev(labels)
    need = hip.seg_confusion_workspace_bytes(n, p, k)
    assert need == n * 5 * 10 * 8
    assert hip.seg_confusion_workspace_bytes(1, 1, 4) == 17 * 8 and hip.seg_confusion_workspace_bytes(1, 1 << 30, 1) == 256 * 2 * 8
    ws = torch.zeros(need // 8 + 1, dtype=torch.int64, device='cuda')
    out, raw = _out(n, k * k + 1, torch.int64, -7)
    names = ('logits', 'ld', 'K', 'labels', 'N', 'P', 'out', 'ws', 'ws_bytes')
    base = dict(logits=hip.ptr(tl), ld=4, K=k, labels=hip.ptr(tb), N=n, P=p, out=hip.ptr(out), ws=hip.ptr(ws), ws_bytes=need)
    call = lambda **kw: hip.lib().ssc_seg_confusion(*([kw.get(x, base[x]) for x in names] + [hip.stream_ptr()]))  # noqa: E731
    off = lambda t, nbytes: hip.ptr(t.view(-1).view(torch.uint8)[nbytes:])      # noqa: E731
    assert call(ws_bytes=need - 1) == -2 and call(ws_bytes=0) == -2 and call(ws=None) == -2 and call(ws=off(ws, 4)) == -2
    assert call(K=0) == -1 and call(K=5) == -1 and call(ld=2) == -1 and call(N=0) == -1 and call(P=0) == -1 and call(P=1 << 31) == -1
    assert call(N=65536) == -1 and call(logits=None) == -1 and call(labels=None) == -1 and call(out=None) == -1
    assert call(out=off(raw, 8 * 8 + 4)) == -3 and call(logits=off(tl, 2)) == -3 and call(labels=off(tb, 2)) == -3
    torch.cuda.synchronize()
    assert (raw.cpu().numpy() == -7).all() and not ws.cpu().numpy().any()
    assert call() == 0
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), confusion_np(logits, k, labels))


# ---------------------------------------------------------------------------------------------------------------
# training, through the command line
# ---------------------------------------------------------------------------------------------------------------
SIZE = 32
COLOURS = [(153, 217, 234), (181, 230, 29), (200, 30, 40), (20, 20, 90), (250, 250, 250), (90, 60, 10)]


def _write_scenes(base, mode, n, first):
    """n flat-coloured scenes: sky (128) over ground (255) and a foreground rectangle (0) of one colour; in scene 1 of a
    mode the rectangle reaches the left and the bottom border."""
    for kind in ('foreground', 'background', 'segment'):
        os.makedirs(os.path.join(base, kind, mode))
    os.makedirs(os.path.join(base, 'captions'), exist_ok=True)
    recs = []
    for i in range(n):
        name = '%s_scene_%d.png' % (mode, i)
        c = first + i
        seg = np.zeros((SIZE, SIZE), np.uint8)
        seg[:14 + 2 * i] = 128
        seg[14 + 2 * i:] = 255
        box = (slice(18, SIZE), slice(0, 12)) if i == 1 else (slice(8 + i, 22 + i), slice(10 + 3 * i, 24 + 3 * i))
        seg[box] = 0
        fg = np.full((SIZE, SIZE, 3), 255, np.uint8)
        fg[box] = COLOURS[(c + 2) % 6]
        bg = np.where((seg == 128)[..., None], np.array(COLOURS[c % 6], np.uint8),
                      np.where((seg == 255)[..., None], np.array(COLOURS[(c + 1) % 6], np.uint8), fg)).astype(np.uint8)
        assert set(np.unique(seg)) == {0, 128, 255}
        Image.fromarray(fg, 'RGB').save(os.path.join(base, 'foreground', mode, name))
        Image.fromarray(bg, 'RGB').save(os.path.join(base, 'background', mode, name))
        Image.fromarray(seg, 'L').save(os.path.join(base, 'segment', mode, name))
        recs.append({'fg_name': name, 'bg_name': name, 'color_text': 'the sky is %s and the ground is %s'
                     % (('blue', 'green', 'red')[c % 3], ('green', 'yellow', 'gray')[c % 3])})
    with open(os.path.join(base, 'captions', mode + '.json'), 'w') as fp:
        json.dump(recs, fp)


def _cli(cwd, argv):
    """bg_colorization_main.py --mode train at 32 x 32, four steps, a snapshot behind every one, in a process of its own under
    its own time limit, after random.seed(23) -> (run directory, output)."""
    argv = ['--mode', 'train', '--image_size', str(SIZE), '--max_steps', '4', '--save_freq', '1', '--progress_freq', '0',
            '--summary_freq', '2', '--data_base_dir', 'data', '--vocab_file', VOCAB] + list(argv)
    code = ('import random, sys; sys.path.insert(0, %r); random.seed(23); import bg_colorization_main as m; m.main(%r)'
            % (ROOT, argv))
    r = subprocess.run([sys.executable, '-c', code], cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       universal_newlines=True, timeout=CHILD_LIMIT)
    assert r.returncode == 0, r.stdout[-4000:]
    runs = sorted(os.listdir(os.path.join(cwd, 'outputs')))
    assert len(runs) == 1, runs
    return os.path.join(cwd, 'outputs', runs[0]), r.stdout


CONFIGS = {'b1': ['--batch_size', '1'], 'b2': ['--batch_size', '2'],
           'device-cap1': ['--batch_size', '2', '--scene_cache', 'device', '--val_records', '1']}
_RUNS = {}


def _run(tmp_path_factory, config, vf, val=True, again=''):
    """The run of a configuration with --val_freq vf, made once per session, in a working directory of its own."""
    key = (config, vf, val, again)
    if key not in _RUNS:
        cwd = str(tmp_path_factory.mktemp('%s-vf%s%s%s' % (config, vf, '' if val else '-noval', again)))
        _write_scenes(os.path.join(cwd, 'data'), 'train', 3, 0)
        if val:
            _write_scenes(os.path.join(cwd, 'data'), 'val', 3, 3)
        _RUNS[key] = (cwd,) + _cli(cwd, CONFIGS[config] + ['--val_freq', vf])
    return _RUNS[key]


def _lines(run):
    with open(os.path.join(run, 'log', 'validation.jsonl')) as f:
        return [json.loads(l) for l in f]


def _snapshot(run, step=4):
    return torch.load(os.path.join(run, 'snapshot', 'snapshot-%d' % step), map_location='cpu')


def _differing(a, b):
    assert list(a) == list(b) and len(a) > 50 and '__adam_m__/generator' in a
    return [k for k in a if not torch.equal(torch.as_tensor(a[k]), torch.as_tensor(b[k]))]


def test_two_runs_without_passes_are_the_same_run(tmp_path_factory):
    """The ground the trajectory test stands on: the same command with --val_freq 0 twice leaves the same snapshot bits."""
    a = _snapshot(_run(tmp_path_factory, 'b1', '0')[1])
    b = _snapshot(_run(tmp_path_factory, 'b1', '0', again='-again')[1])
    assert not _differing(a, b)


@pytest.mark.parametrize('config', sorted(CONFIGS))
def test_run_writes_a_line_per_pass(tmp_path_factory, config):
    """--max_steps 4 --val_freq 2: lines at global steps 2 and 4 and nowhere else; three images, or one under --val_records 1;
    the run without the flag writes no such file and says nothing about it."""
    cwd, run, out = _run(tmp_path_factory, config, '2')
    lines = _lines(run)
    images = 1 if 'cap1' in config else 3
    assert [l['step'] for l in lines] == [2, 4] and all(l['images'] == images for l in lines), lines
    for l in lines:
        assert sorted(l) == ['all', 'groups', 'images', 'region', 'seconds', 'step'] and sorted(l['groups']) == ['all']
        assert l['all'] == l['groups']['all'] and l['all']['n'] == images and l['seconds'] > 0
        assert all(np.isfinite(l['all'][k]) for k in ('mae', 'psnr', 'ssim')), l
        assert 0 < l['all']['mae'] < 255 and -1 <= l['all']['ssim'] <= 1
        r = l['region']
        assert sorted(r) == ['accuracy', 'ignored', 'iou', 'miou'] and r['ignored'] == 0 and len(r['iou']) == 3
        assert 0 <= r['accuracy'] <= 1 and 0 <= r['miou'] <= 1
    assert out.count('held-out pass at step') == 2 and 'held-out cache: %d scenes' % images in out
    assert 'metrics: n %d' % images in out and 'region miou' in out
    assert ('scene cache: 3 scenes' in out) == ('device' in config)
    assert sorted(os.listdir(os.path.join(run, 'snapshot'))) == ['checkpoint'] + ['snapshot-%d' % s for s in (1, 2, 3, 4)]
    _, run0, out0 = _run(tmp_path_factory, config, '0')
    assert not os.path.exists(os.path.join(run0, 'log', 'validation.jsonl')) and 'held-out' not in out0
    # scalars.jsonl is what --summary_freq 2 makes of it, with and without the passes: the same steps and keys, and the same
    # averages as far as two runs agree on them at all -- a loss word is a sum of per-workgroup partials added atomically in
    # double, equal from run to run to double rounding and not bitwise (tests/test_gpu_residual.py holds it to 1e-9 as well)
    with open(os.path.join(run, 'log', 'scalars.jsonl')) as fa, open(os.path.join(run0, 'log', 'scalars.jsonl')) as fb:
        sa, sb = [json.loads(l) for l in fa], [json.loads(l) for l in fb]
    assert [r['step'] for r in sa] == [2, 4] == [r['step'] for r in sb]
    for ra, rb in zip(sa, sb):
        assert sorted(ra) == sorted(rb) and len(ra) == 6
        assert all(abs(ra[k] - rb[k]) <= 1e-9 * max(1.0, abs(rb[k])) for k in ra), (ra, rb)


@pytest.mark.parametrize('config', sorted(CONFIGS))
def test_passes_leave_the_training_trajectory_alone(tmp_path_factory, config):
    """snapshot-4 (and snapshot-2, the one behind the first pass) with and without the passes: the same tensors bit for bit,
    Adam's first moments included."""
    run2, run0 = _run(tmp_path_factory, config, '2')[1], _run(tmp_path_factory, config, '0')[1]
    for step in (2, 4):
        a, b = _snapshot(run2, step), _snapshot(run0, step)
        differ = _differing(a, b)
        assert not differ, (step, differ[:5])
    assert not torch.isnan(a['__adam_m__/generator']).any() and float(a['__adam_m__/generator'].abs().sum()) > 0


@pytest.mark.parametrize('config', sorted(CONFIGS))
def test_the_last_line_is_the_score_of_the_snapshot(tmp_path_factory, config):
    """snapshot-4 in a fresh trainer; per val scene the files decoded on the host, staged by hip.bg_stage_u8, one forward pass
    under another tag, hip.bg_finish_u8 with the paste-back, hip.image_metrics_u8 under the segment mask, and a NumPy argmax
    confusion of the logits: through the line builder these rows give the step-4 line exactly."""
    import bg_colorization_main as bgcli
    from sketchyscenecolorization_amd import bg_validation as BV, hip
    from sketchyscenecolorization_amd.bg_colorization import BGTrainer
    cwd, run, _ = _run(tmp_path_factory, config, '2')
    line = _lines(run)[-1]
    assert line['step'] == 4
    tr = BGTrainer(image_size=SIZE, max_steps=4, seed=1)
    tr.store.load_state_dict(_snapshot(run))
    scenes = bgcli.Scenes({'image_size': SIZE, 'text_len': 8, 'data_base_dir': os.path.join(cwd, 'data'), 'mode': 'val',
                           'vocab_size': 18, 'vocab_file': VOCAB})
    count = 1 if 'cap1' in config else 3
    x = torch.empty((1, SIZE, SIZE, 3), dtype=torch.float32, device='cuda')
    y, xd, cnt = torch.empty_like(x), torch.empty((1, SIZE, SIZE, 8), dtype=torch.float32, device='cuda'), torch.empty(1, device='cuda')
    rows, conf, names, touches = [], [], [], False
    for i in range(count):
        fg, bg, tok, lab, fg_name, bg_name = scenes.get(i)
        seg = np.ascontiguousarray(np.array(Image.open(os.path.join(scenes.dirs['segment'], fg_name)).convert('RGB'), np.uint8)[:, :, 0])
        touches = touches or (seg[:, 0] == 0).any()
        fg_d, bg_d, seg_d, lab_d = _dev(fg), _dev(bg), _dev(seg[None]), _dev(lab)
        hip.bg_stage_u8(fg_d, bg_d, lab_d, x, y, xd, cnt)
        gctx = tr.G.forward(x, tok, None, 'independent')
        u8 = hip.bg_finish_u8(gctx['image'], fg_d, seg_d)
        assert torch.equal(u8[0][seg_d[0] == 0], fg_d[0][seg_d[0] == 0])
        rows.append(hip.image_metrics_u8(u8, bg_d, seg_d).cpu().numpy())
        logits = gctx['region_logits'].cpu().numpy().reshape(1, -1, 3)
        conf.append(confusion_np(logits, 3, lab.reshape(1, -1)))
        names.append(bg_name[:-4])
    assert touches or count == 1, 'no val scene whose foreground touches the border'
    mine, _ = BV.validation_line(4, names, np.concatenate(rows, 0), np.concatenate(conf, 0), line['seconds'])
    print('line of the run: %r\nindependent:     %r' % (line, mine))
    assert json.loads(BV.dumps_line(mine)) == line
    assert np.concatenate(rows, 0)[:, 2].tolist() == [float(np.count_nonzero(scenes.get(i)[3])) for i in range(count)]


def test_without_the_val_files_training_goes_on(tmp_path_factory):
    """--val_freq 2 without captions/val.json: one line says so, the run trains to its end, writes no validation.jsonl and
    leaves the snapshot of --val_freq 0."""
    _, run, out = _run(tmp_path_factory, 'b1', '2', val=False)
    assert out.count(os.path.join('data', 'captions', 'val.json') + ' not found') == 1 and 'held-out' not in out.replace('without held-out passes', '')
    assert not os.path.exists(os.path.join(run, 'log', 'validation.jsonl'))
    assert not _differing(_snapshot(run), _snapshot(_run(tmp_path_factory, 'b1', '0')[1]))
