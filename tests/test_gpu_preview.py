"""The preview sheets on the device (csrc/preview.hip, sketchyscenecolorization_amd/preview.py).

The two kernels against the NumPy restatement tests/preview_oracle.py, byte for byte (they work on integers: nothing to allow
for): tile rows that start on every byte offset mod 4 (left 0..4 with the sheet's base 5 bytes off a 16-byte boundary, and on one,
where the 4-byte path runs), a sheet pre-filled with a pattern of which every byte outside the tiles must survive, guard bytes
around the sheet, a second run with the same bits, sources of all 255 and all 0; every refusal with the destination untouched.

Then the flags: each trainer at its smallest size once with --val_preview 0 and once with K -- the snapshots are the same bytes
and the validation lines the same apart from ``seconds`` -- and what the sheets hold, against the pass's own outputs; and
match_main.py --mode eval --visualized 1 in a fresh process."""
import faulthandler
import json
import os
import random
import subprocess
import sys

import numpy as np
import pytest
import torch
from PIL import Image

import match_eval_oracle as EO
import preview_oracle as PO
from kernel_check import rc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VOCAB = os.path.join(ROOT, 'tests', 'golden', 'match', 'vocab.txt')
BG_VOCAB = os.path.join(ROOT, 'tests', 'golden', 'bg_aug', 'bg_vocab.txt')
GUARD = 64
FILL = 0xA5
CHILD_LIMIT = 180
SMALL = dict(size=64, units=(1, 1, 1, 1), filters=(8, 16, 32, 64, 128))
NARROW = dict(v_emb=24, w_emb=24, w_rnn=40, m_rnn=20)


@pytest.fixture(autouse=True)
def _time_limit():
    """A test that hangs on the device ends the process (with every thread's traceback) instead of holding the card."""
    faulthandler.dump_traceback_later(400, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


def hip():
    from sketchyscenecolorization_amd import hip as h
    return h


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


class GuardedSheet(object):
    """A sheet [SH,SW,3] whose first byte lies ``offset`` bytes past a 16-byte boundary, pre-filled with a pattern, between guard
    bytes (as ``Guarded`` of tests/test_gpu_matching.py)."""

    def __init__(self, SH, SW, offset):
        n = SH * SW * 3
        self.raw = torch.full((n + 2 * GUARD + 32,), FILL, dtype=torch.uint8, device='cuda')
        self.start = GUARD + (16 - (self.raw.data_ptr() + GUARD) % 16) % 16 + offset
        self.t = self.raw[self.start:self.start + n].view(SH, SW, 3)
        assert self.t.data_ptr() % 16 == offset % 16 and self.t.is_contiguous()
        self.pattern = ((np.arange(n) * 7 + 3) % 251).astype(np.uint8).reshape(SH, SW, 3)
        self.n = n
        self.reset()

    def reset(self):
        self.t.copy_(torch.from_numpy(self.pattern))

    def get(self):
        raw = self.raw.cpu().numpy()
        assert (raw[:self.start] == FILL).all() and (raw[self.start + self.n:] == FILL).all(), 'the kernel wrote outside the sheet'
        return raw[self.start:self.start + self.n].reshape(self.pattern.shape)


def _sheet_dims(N, th, tw):
    pitch = th + 1
    SW = (tw + 4 + 3 + 3) // 4 * 4              # room for left 0..4 and a margin; a multiple of 4: the 4-byte path can run
    SH = 1 + (N - 1) * pitch + th + 2
    return SH, SW, pitch


# ------------------------------------------------------------------ ssc_sheet_tiles_u8
TILE_CASES = [(1, 2, 2, 1), (1, 2, 2, 2), (3, 8, 12, 2), (2, 64, 64, 4), (1, 16, 16, 8), (1, 768, 768, 2), (2, 12, 24, 6), (1, 8, 20, 1)]


@pytest.mark.parametrize('offset', [5, 0])
@pytest.mark.parametrize('N,H,W,s', TILE_CASES, ids=lambda v: str(v))
def test_sheet_tiles_against_the_oracle(N, H, W, s, offset):
    """(1,2,2,2): a tile of one pixel; (3,8,12,2): H != W, a whole group of four pixels and a rest of two; (2,64,64,4) and 768: more
    than one workgroup; (2,12,24,6): the reduction of a 384-pixel record for a 64-pixel generator; (1,8,20,1): s = 1 with W % 4 == 0."""
    rng = np.random.RandomState(N * 1000 + H + W + s)
    th, tw = H // s, W // s
    SH, SW, pitch = _sheet_dims(N, th, tw)
    sheet = GuardedSheet(SH, SW, offset)
    sources = {'random': rng.randint(0, 256, (N, H, W, 3)).astype(np.uint8), '255': np.full((N, H, W, 3), 255, np.uint8),
               '0': np.zeros((N, H, W, 3), np.uint8)}
    for kind, src in sources.items():
        src_d = _dev(src)
        for left in range(5):
            want = PO.tiles(sheet.pattern, src, s, 1, left, pitch)
            runs = []
            for _ in range(2):
                sheet.reset()
                hip().sheet_tiles_u8(src_d, s, sheet.t, 1, left, pitch)
                runs.append(sheet.get().copy())
            assert np.array_equal(runs[0], runs[1]), (kind, left)                   # the same bits on every run
            bad = np.argwhere(runs[0] != want)
            assert bad.size == 0, (kind, left, bad[:4], runs[0][tuple(bad[0])], want[tuple(bad[0])])
            if kind != 'random':        # the rounding never leaves 0..255: a constant image stays that constant
                assert (runs[0][1:1 + th, left:left + tw] == int(kind)).all()


def test_sheet_tiles_source_off_its_boundary():
    """A source that starts 1, 2 and 3 bytes past a 4-byte boundary takes the bytewise path and gives the same tiles."""
    rng = np.random.RandomState(4)
    src = rng.randint(0, 256, (2, 8, 16, 3)).astype(np.uint8)
    SH, SW, pitch = _sheet_dims(2, 4, 8)
    sheet = GuardedSheet(SH, SW, 0)
    want = PO.tiles(sheet.pattern, src, 2, 1, 4, pitch)
    for off in range(4):
        base = torch.zeros(src.size + 32, dtype=torch.uint8, device='cuda')
        start = (16 - base.data_ptr() % 16) % 16 + off
        view = base[start:start + src.size].view(src.shape)
        view.copy_(torch.from_numpy(src))
        sheet.reset()
        hip().sheet_tiles_u8(view, 2, sheet.t, 1, 4, pitch)
        assert np.array_equal(sheet.get(), want), off


# ------------------------------------------------------------------ ssc_sheet_overlay_u8
def _overlay_case(S, seed, lut_kind):
    if S == 4:
        sketch, pred, labels, lut = PO.hand_scene()
    else:
        rng = np.random.RandomState(seed)
        sketch = rng.randint(0, 256, (S, S, 3)).astype(np.uint8)
        pred = (rng.rand(S, S) < 0.4).astype(np.uint8) * rng.choice(np.array([1, 2, 255], np.uint8), (S, S))
        labels = rng.randint(0, 6, (S, S)).astype(np.uint8)
        labels[rng.rand(S, S) < 0.1] = 255
        lut = np.zeros(256, np.uint8)
        lut[[1, 4, 255]] = (1, 7, 255)
    if lut_kind == 'zero':
        lut = np.zeros(256, np.uint8)
    return sketch, pred, labels, lut


@pytest.mark.parametrize('offset', [5, 0])
@pytest.mark.parametrize('S,s,lut_kind', [(4, 1, 'sparse'), (4, 2, 'sparse'), (64, 1, 'sparse'), (64, 2, 'sparse'), (64, 2, 'zero'),
                                          (768, 2, 'sparse'), (24, 6, 'sparse')])
def test_sheet_overlay_against_the_oracle(S, s, lut_kind, offset):
    sketch, pred, labels, lut = _overlay_case(S, 3 * S + s, lut_kind)
    tile = S // s
    SH, SW, _pitch = _sheet_dims(1, tile, tile)
    sheet = GuardedSheet(SH, SW, offset)
    sk_d, pred_d, lab_d, lut_d = _dev(sketch), _dev(pred), _dev(labels), _dev(lut)
    modes = {'gt': (None, labels, lut, None, lab_d, lut_d), 'out': (pred, None, None, pred_d, None, None),
             'both': (pred, labels, lut, pred_d, lab_d, lut_d)}
    for mode, (p, l, t, p_d, l_d, t_d) in modes.items():
        for left in range(5):
            want = PO.overlay(sheet.pattern, sketch, p, l, t, s, 1, left)
            runs = []
            for _ in range(2):
                sheet.reset()
                hip().sheet_overlay_u8(sk_d, p_d, l_d, t_d, s, sheet.t, 1, left)
                runs.append(sheet.get().copy())
            assert np.array_equal(runs[0], runs[1]), (mode, left)
            bad = np.argwhere(runs[0] != want)
            assert bad.size == 0, (mode, left, bad[:4], runs[0][tuple(bad[0])], want[tuple(bad[0])])
    if s == 1 and S == 64:      # the colours themselves, at full size
        sheet.reset()
        hip().sheet_overlay_u8(sk_d, pred_d, lab_d, lut_d, 1, sheet.t, 1, 0)
        got = sheet.get()[1:1 + S, :S]
        pm, tm = pred != 0, lut[labels] != 0
        assert (got[pm & tm] == (0, 170, 0)).all() and (got[pm & ~tm] == (230, 0, 0)).all() and (got[tm & ~pm] == (0, 90, 255)).all()
        assert np.array_equal(got[~pm & ~tm], sketch[~pm & ~tm])


def test_overlay_without_pred_and_labels_is_the_tile_of_the_sketch():
    sketch = _overlay_case(64, 1, 'sparse')[0]
    SH, SW, _p = _sheet_dims(1, 32, 32)
    a, b = GuardedSheet(SH, SW, 0), GuardedSheet(SH, SW, 0)
    hip().sheet_overlay_u8(_dev(sketch), None, None, None, 2, a.t, 1, 2)
    hip().sheet_tiles_u8(_dev(sketch[None]), 2, b.t, 1, 2)
    assert np.array_equal(a.get(), b.get()) and np.array_equal(a.get(), PO.tiles(a.pattern, sketch[None], 2, 1, 2, 0))


# ------------------------------------------------------------------ refusals
def test_sheet_tiles_refusals():
    src = torch.zeros((2, 8, 8, 3), dtype=torch.uint8, device='cuda')
    sheet = GuardedSheet(20, 16, 0)
    good = dict(N=2, H=8, W=8, s=2, SH=20, SW=16, top=1, left=2, pitch=5)

    def call(src_t=src, sheet_t=sheet.t, **kw):
        a = dict(good, **kw)
        return rc('ssc_sheet_tiles_u8', src_t, a['N'], a['H'], a['W'], a['s'], sheet_t, a['SH'], a['SW'], a['top'], a['left'], a['pitch'])
    assert call(src_t=None) == -1 and call(sheet_t=None) == -1                      # null pointers
    assert call(N=0) == -1 and call(N=-1) == -1
    for s in (0, 3, 5, 7, 16, -2):                                                  # an s that is not allowed
        assert call(s=s) == -1, s
    assert call(H=6, s=4) == -1 and call(W=6, s=4) == -1 and call(H=9, s=2) == -1   # an s that does not divide
    assert call(left=13) == -1 and call(left=-1) == -1 and call(top=-1) == -1       # a tile that leaves the sheet
    assert call(top=12) == -1 and call(SH=9) == -1 and call(SW=5) == -1
    assert call(top=20) == -1 and call(left=16) == -1
    assert call(pitch=3) == -1 and call(pitch=-1) == -1                             # pitch < H/s with N > 1
    assert call(N=1, pitch=0) == 0                                                  # (one tile needs no pitch)
    sheet.reset()
    assert call(H=0) == -1 and call(W=0) == -1 and call(SH=0) == -1 and call(SW=0) == -1
    # src overlapping sheet: the sheet's own bytes as the source, and a source that ends inside the sheet
    inside = sheet.t.reshape(-1)[:2 * 8 * 8 * 3].view(2, 8, 8, 3)
    assert call(src_t=inside) == -1
    before = sheet.raw[sheet.start - 8:sheet.start - 8 + 384].view(2, 8, 8, 3)
    assert call(src_t=before) == -1
    assert np.array_equal(sheet.get(), sheet.pattern)                               # a refusal writes nothing
    assert call() == 0 and not np.array_equal(sheet.get(), sheet.pattern)
    with pytest.raises(ValueError):
        hip().sheet_tiles_u8(src.to(torch.int32), 2, sheet.t, 1, 2, 5)
    with pytest.raises(ValueError):
        hip().sheet_tiles_u8(src, 2, sheet.t[:, :, :2], 1, 2, 5)
    with pytest.raises(RuntimeError, match='code -1'):
        hip().sheet_tiles_u8(src, 3, sheet.t, 1, 2, 5)


def test_sheet_overlay_refusals():
    S = 8
    sk = torch.zeros((S, S, 3), dtype=torch.uint8, device='cuda')
    pred, labels = (torch.ones((S, S), dtype=torch.uint8, device='cuda') for _ in range(2))
    lut = torch.ones(256, dtype=torch.uint8, device='cuda')
    sheet = GuardedSheet(12, 12, 0)
    good = dict(S=S, s=2, SH=12, SW=12, top=1, left=2)

    def call(sk_t=sk, pred_t=pred, labels_t=labels, lut_t=lut, sheet_t=sheet.t, **kw):
        a = dict(good, **kw)
        return rc('ssc_sheet_overlay_u8', sk_t, pred_t, labels_t, lut_t, a['S'], a['s'], sheet_t, a['SH'], a['SW'], a['top'], a['left'])
    assert call(sk_t=None) == -1 and call(sheet_t=None) == -1
    assert call(labels_t=None) == -1 and call(lut_t=None) == -1                     # labels and lut go together
    for s in (0, 3, 5, 16):
        assert call(s=s) == -1, s
    assert call(S=0) == -1 and call(S=6, s=4) == -1
    assert call(left=9) == -1 and call(top=9) == -1 and call(left=-1) == -1 and call(top=-1) == -1 and call(SH=4) == -1 and call(SW=5) == -1
    flat = sheet.t.reshape(-1)
    assert call(sk_t=flat[:S * S * 3].view(S, S, 3)) == -1                          # every input overlapping the sheet
    assert call(pred_t=flat[:S * S].view(S, S)) == -1 and call(labels_t=flat[8:8 + S * S].view(S, S)) == -1
    assert call(lut_t=flat[-256:]) == -1
    assert np.array_equal(sheet.get(), sheet.pattern)
    assert call() == 0 and call(pred_t=None) == 0 and call(labels_t=None, lut_t=None) == 0
    with pytest.raises(ValueError, match='go together'):
        hip().sheet_overlay_u8(sk, pred, labels, None, 2, sheet.t, 1, 2)
    with pytest.raises(ValueError):
        hip().sheet_overlay_u8(sk, pred[:4], labels, lut, 2, sheet.t, 1, 2)


# ---------------------------------------------------------------------------------------------------------------
# the flags: requirement A and what the sheets hold, in this process
# ---------------------------------------------------------------------------------------------------------------
def _without_seconds(path):
    out = []
    for l in open(path):
        rec = json.loads(l)
        assert rec.pop('seconds') > 0
        out.append(rec)
    return out


def _png(path):
    return np.array(Image.open(path).convert('RGB'))


def _tile(sheet, row, column, th, tw):
    top, left = PO.tile_origin(row, column, th, tw)
    return sheet[top:top + th, left:left + tw]


def _outside_tiles_is_white(sheet, rows, columns, th, tw):
    mask = np.ones(sheet.shape[:2], bool)
    for r in range(rows):
        for c in range(columns):
            top, left = PO.tile_origin(r, c, th, tw)
            mask[top:top + th, left:left + tw] = False
    return sheet.shape[:2] == (4 + rows * (th + 4), 4 + columns * (tw + 4)) and bool((sheet[mask] == 255).all())


def test_foreground_preview_leaves_the_run_alone_and_shows_the_pass(tmp_path, monkeypatch):
    """Pix2Pix at 64 x 64 (-si 1), batch 2, 3 held-out records, 3 iterations, -vf 1: with -vp 2 the snapshot and the lines are
    those of -vp 0; the sheet of every pass holds image_postprocess_u8 of the pass's own tower.infer_nhwc rows (read by a hook
    around the pass's scoring call), between the records' sketches and targets reduced by 6."""
    import obj_colorization_main as cli
    from test_gpu_train_validation import _write_records
    from sketchyscenecolorization_amd import hip as H, record_cache as rcache, train_validation as TV
    from sketchyscenecolorization_amd.obj_lib import main_procedure as mp, models_collection as models
    base = mp.RecordQueue

    class SeededQueue(base):        # (tests/train_validation_child.py: the command line seeds one GPU's queues from the system)
        def __init__(self, batch_size, small, which, data_base_dir='data', seed=None, record_cache=None):
            base.__init__(self, batch_size, small, which, data_base_dir=data_base_dir, seed=4000 + which, record_cache=record_cache)
    monkeypatch.setattr(mp, 'RecordQueue', SeededQueue)
    real = H.image_metrics_f32
    seen = []

    def spy(a, coff, b, *args, **kw):
        seen.append(H.image_postprocess_u8(a, coff).cpu().numpy())
        return real(a, coff, b, *args, **kw)

    def run(tag, vp):
        cwd = tmp_path / tag
        cwd.mkdir()
        _write_records(str(cwd), 'train', 3, 11)
        _write_records(str(cwd), 'val', 3, 12)
        monkeypatch.chdir(str(cwd))
        models.reset_default_graph()
        torch.manual_seed(7)
        try:
            cli.main(['--mode', 'train', '-si', '1', '-bs', '2', '-mi', '3', '-smf', '3', '-swf', '100', '-bt', 'Pix2Pix', '-vf', '1',
                      '-vp', str(vp)])
            torch.cuda.synchronize()
        finally:
            models.reset_default_graph()
        runs = sorted(os.listdir(str(cwd / 'outputs')))
        assert len(runs) == 1
        return os.path.join(str(cwd), 'outputs', runs[0])
    try:
        plain = run('vp0', 0)
        monkeypatch.setattr(H, 'image_metrics_f32', spy)
        shown = run('vp2', 2)
        monkeypatch.setattr(H, 'image_metrics_f32', real)
        a = torch.load(os.path.join(plain, 'snapshot', 'model_2.ckpt-2'), map_location='cpu')
        b = torch.load(os.path.join(shown, 'snapshot', 'model_2.ckpt-2'), map_location='cpu')
        assert list(a) == list(b) and len(a) > 20
        assert not [k for k in a if not torch.equal(torch.as_tensor(a[k]), torch.as_tensor(b[k]))]
        lines = _without_seconds(os.path.join(shown, 'log', 'validation.jsonl'))
        assert lines == _without_seconds(os.path.join(plain, 'log', 'validation.jsonl')) and [l['step'] for l in lines] == [0, 1, 2]
        assert not os.path.exists(os.path.join(plain, 'log', 'previews'))
        assert sorted(os.listdir(os.path.join(shown, 'log', 'previews'))) == sorted('step_%d.%s' % (i, e) for i in range(3) for e in ('json', 'png'))
        assert len(seen) == 6                       # two batches per pass: records (0, 1) and (2)
        cache = rcache.RecordCache(rcache.list_record_files(os.path.join(os.path.dirname(os.path.dirname(shown)), 'data', 'tfrecord', 'val')),
                                   64, device='cuda')
        sk, img = cache.sk.cpu().numpy(), cache.img.cpu().numpy()
        names, groups = TV.record_names(cache)
        sheets = []
        for i in range(3):
            sheet = _png(os.path.join(shown, 'log', 'previews', 'step_%d.png' % i))
            assert _outside_tiles_is_white(sheet, 2, 3, 64, 64)
            for r in range(2):
                assert np.array_equal(_tile(sheet, r, 0, 64, 64), PO.box_mean(sk[r], 6))
                assert np.array_equal(_tile(sheet, r, 1, 64, 64), seen[2 * i][r])
                assert np.array_equal(_tile(sheet, r, 2, 64, 64), PO.box_mean(img[r], 6))
            rec = json.load(open(os.path.join(shown, 'log', 'previews', 'step_%d.json' % i)))
            assert rec['kind'] == 'foreground' and rec['step'] == i and rec['columns'] == ['sketch', 'output', 'target']
            assert rec['tile'] == [64, 64] and rec['scale'] == 6
            assert rec['rows'] == [{'name': names[r], 'category': groups[r], 'caption_indices': [int(v) for v in cache.text[r]]} for r in range(2)]
            sheets.append(sheet)
        assert not np.array_equal(sheets[0], sheets[2])         # the weights of the moment
    finally:
        rcache._MEMO.clear()


SIZE_BG = 64
COLOURS = [(153, 217, 234), (181, 230, 29), (200, 30, 40), (20, 20, 90), (250, 250, 250), (90, 60, 10)]


def _write_bg_scenes(base, mode, n, first):
    """n flat-coloured scenes of 64 x 64: sky (128) over ground (255) and a foreground rectangle (0)."""
    for kind in ('foreground', 'background', 'segment'):
        os.makedirs(os.path.join(base, kind, mode))
    os.makedirs(os.path.join(base, 'captions'), exist_ok=True)
    recs, arrays = [], []
    for i in range(n):
        name = '%s_scene_%d.png' % (mode, i)
        c = first + i
        seg = np.zeros((SIZE_BG, SIZE_BG), np.uint8)
        seg[:28 + 4 * i] = 128
        seg[28 + 4 * i:] = 255
        box = (slice(16 + 2 * i, 44 + 2 * i), slice(20 + 6 * i, 48 + 6 * i))
        seg[box] = 0
        fg = np.full((SIZE_BG, SIZE_BG, 3), 255, np.uint8)
        fg[box] = COLOURS[(c + 2) % 6]
        bg = np.where((seg == 128)[..., None], np.array(COLOURS[c % 6], np.uint8),
                      np.where((seg == 255)[..., None], np.array(COLOURS[(c + 1) % 6], np.uint8), fg)).astype(np.uint8)
        Image.fromarray(fg, 'RGB').save(os.path.join(base, 'foreground', mode, name))
        Image.fromarray(bg, 'RGB').save(os.path.join(base, 'background', mode, name))
        Image.fromarray(seg, 'L').save(os.path.join(base, 'segment', mode, name))
        recs.append({'fg_name': name, 'bg_name': name, 'color_text': 'the sky is %s and the ground is %s'
                     % (('blue', 'green', 'red')[c % 3], ('green', 'yellow', 'gray')[c % 3])})
        arrays.append((fg, bg))
    with open(os.path.join(base, 'captions', mode + '.json'), 'w') as fp:
        json.dump(recs, fp)
    return arrays


def test_background_preview_leaves_the_run_alone_and_shows_the_pass(tmp_path, monkeypatch):
    """Background at 64 x 64, batch 1, 2 held-out scenes, 2 steps, --val_freq 1: with --val_preview 2 the snapshots and the lines
    are those of --val_preview 0; the output tile is bg_finish_u8 of the pass's image (read by a hook around the scoring call)."""
    import bg_colorization_main as bgcli
    from sketchyscenecolorization_amd import hip as H
    real = H.image_metrics_bg_f32
    seen = []

    def spy(image, fg, target, mask=None, **kw):
        seen.append(H.bg_finish_u8(image, fg, mask).cpu().numpy()[0])
        return real(image, fg, target, mask, **kw)

    def run(tag, vp):
        cwd = tmp_path / tag
        cwd.mkdir()
        _write_bg_scenes(str(cwd / 'data'), 'train', 3, 0)
        val = _write_bg_scenes(str(cwd / 'data'), 'val', 2, 3)
        monkeypatch.chdir(str(cwd))
        random.seed(23)
        torch.manual_seed(23)
        bgcli.main(['--mode', 'train', '--image_size', str(SIZE_BG), '--max_steps', '2', '--save_freq', '1', '--progress_freq', '0',
                    '--summary_freq', '0', '--data_base_dir', 'data', '--vocab_file', BG_VOCAB, '--batch_size', '1', '--val_freq', '1',
                    '--val_preview', str(vp)])
        torch.cuda.synchronize()
        runs = sorted(os.listdir(str(cwd / 'outputs')))
        assert len(runs) == 1
        return os.path.join(str(cwd), 'outputs', runs[0]), val
    plain, _val = run('vp0', 0)
    monkeypatch.setattr(H, 'image_metrics_bg_f32', spy)
    shown, val = run('vp2', 2)
    monkeypatch.setattr(H, 'image_metrics_bg_f32', real)
    for step in (1, 2):
        a = torch.load(os.path.join(plain, 'snapshot', 'snapshot-%d' % step), map_location='cpu')
        b = torch.load(os.path.join(shown, 'snapshot', 'snapshot-%d' % step), map_location='cpu')
        assert list(a) == list(b) and len(a) > 50
        assert not [k for k in a if not torch.equal(torch.as_tensor(a[k]), torch.as_tensor(b[k]))]
    lines = _without_seconds(os.path.join(shown, 'log', 'validation.jsonl'))
    assert lines == _without_seconds(os.path.join(plain, 'log', 'validation.jsonl')) and [l['step'] for l in lines] == [1, 2]
    assert not os.path.exists(os.path.join(plain, 'log', 'previews')) and len(seen) == 4
    for n, step in enumerate((1, 2)):
        sheet = _png(os.path.join(shown, 'log', 'previews', 'step_%d.png' % step))
        assert _outside_tiles_is_white(sheet, 2, 3, SIZE_BG, SIZE_BG)
        for r in range(2):
            assert np.array_equal(_tile(sheet, r, 0, SIZE_BG, SIZE_BG), val[r][0])
            assert np.array_equal(_tile(sheet, r, 1, SIZE_BG, SIZE_BG), seen[2 * n + r])
            assert np.array_equal(_tile(sheet, r, 2, SIZE_BG, SIZE_BG), val[r][1])
        rec = json.load(open(os.path.join(shown, 'log', 'previews', 'step_%d.json' % step)))
        assert rec['kind'] == 'background' and rec['step'] == step and rec['columns'] == ['foreground', 'output', 'background']
        assert rec['scale'] == 1 and [r['name'] for r in rec['rows']] == ['val_scene_0', 'val_scene_1']
        assert all(len(r['caption_indices']) == 8 for r in rec['rows'])


def _match_setup(tmp_path):
    from test_gpu_match_cache import _second_scene_gets_other_labels
    from sketchyscenecolorization_amd import matching as m, tf_checkpoint
    cfg = m.MatchConfig(**dict(SMALL, **NARROW))
    backbone = str(tmp_path / 'backbone-1')
    tf_checkpoint.write_checkpoint(backbone, {k: a for k, a in m.random_variables(cfg, 31).items() if k.startswith('ResNet/')})
    flags = EO.write_split(str(tmp_path), 'train')[:4]
    eval_flags = EO.write_split(str(tmp_path), 'val', seed=3)
    _second_scene_gets_other_labels(str(tmp_path), 'train')
    _second_scene_gets_other_labels(str(tmp_path), 'val')
    return cfg, backbone, flags, eval_flags


def test_matcher_preview_leaves_the_run_alone_and_shows_the_pass(tmp_path):
    """The matcher at size 64 with the small head: 4 iterations, a snapshot and a pass every 2.  With --val_preview 4 the snapshots
    and the lines are those of --val_preview 0; tile k of the sheet of iteration n is the oracle's overlay of what model.predict
    gives for that scene and caption with the snapshot of iteration n."""
    import match_main
    from test_gpu_match_cache import _snapshot_bytes
    from sketchyscenecolorization_amd import match_eval, matching as m
    cfg, backbone, flags, eval_flags = _match_setup(tmp_path)
    common = ['--mode', 'train', '--backbone_snapshot', backbone, '--vocab_file', VOCAB, '--scene_size', '64', '--save_model_freq', '2',
              '--log_freq', '1', '--seed', '5', '--max_iteration', '4', '--val_freq', '2'] + flags

    def run(tag, vp):
        root = str(tmp_path / tag)
        match_main.main(common + ['--snapshot_root', root, '--log_root', root + '_log', '--val_preview', str(vp)], config=cfg)
        torch.cuda.synchronize()
        return root
    plain, shown = run('vp0', 0), run('vp4', 4)
    for n in (2, 4):
        assert _snapshot_bytes(plain, n) == _snapshot_bytes(shown, n)
    lines = _without_seconds(os.path.join(shown + '_log', 'match_validation.jsonl'))
    assert lines == _without_seconds(os.path.join(plain + '_log', 'match_validation.jsonl')) and [l['iter'] for l in lines] == [2, 4]
    assert not os.path.exists(os.path.join(plain + '_log', 'match_previews'))
    vocab = m.load_vocab(VOCAB)
    scenes = match_eval.read_captions(eval_flags[3], 'val')
    captions = [(image_id, caption, idx) for image_id, pairs in scenes for caption, idx in pairs]
    assert len(captions) == 6
    gts = {image_id: match_eval.load_ground_truth(eval_flags[1], 'val', image_id, 64) for image_id, _p in scenes}
    sheets = []
    for n in (2, 4):
        sheet = _png(os.path.join(shown + '_log', 'match_previews', 'iter_%d.png' % n))
        rec = json.load(open(os.path.join(shown + '_log', 'match_previews', 'iter_%d.json' % n)))
        assert _outside_tiles_is_white(sheet, 1, 4, 64, 64) and rec['grid'] == [1, 4] and rec['scale'] == 1 and rec['step'] == n
        model = m.MatchModel(cfg)
        model.load_tf_checkpoint(os.path.join(shown, 'deeplab_RMI_iter_%d.tfmodel' % n))
        covered = []
        for k, (image_id, caption, idx) in enumerate(captions[:4]):
            gt = gts[image_id]
            feat, stroke = model.features(gt['sketch'])
            indices, seq_len = m.preprocess_sentence(caption, vocab, cfg.max_len)
            _up, predicts = model.predict(feat, stroke, indices, seq_len)
            predicts = predicts.cpu().numpy()
            lut = np.zeros(256, np.uint8)
            lut[[i + 1 for i in idx]] = 1
            want = PO.coloured(gt['sketch'], predicts, gt['labels'], lut)
            assert np.array_equal(_tile(sheet, 0, k, 64, 64), want), (n, k)
            t = lut[gt['labels']] != 0
            assert rec['rows'][k] == {'scene': image_id, 'caption': caption, 'I': int(((predicts != 0) & t).sum()),
                                      'P': int((predicts != 0).sum()), 'A': int(t.sum())}
            covered.append(float((predicts != 0).mean()))
        model.close()
        print('iter %d: predicted share of the pixels per caption %s' % (n, covered))
        assert len(rec['rows']) == 4
        sheets.append(sheet)


def test_eval_visualized_in_a_fresh_process(tmp_path):
    """match_main.py --mode eval --visualized 1 on the synthetic split: <k>_gt.png and <k>_out.png for every caption and a
    captions.json per scene; _out.png is the oracle's overlay of the device's own predicts, _gt.png that of the target; the
    printed block and eval_val.json are those of a run without the flag."""
    from sketchyscenecolorization_amd import match_eval, matching as m, tf_checkpoint
    cfg = m.MatchConfig(**SMALL)
    vocab = m.load_vocab(VOCAB)
    flags = EO.write_split(str(tmp_path))
    scenes = match_eval.read_captions(flags[3], 'val')
    gts = {image_id: match_eval.load_ground_truth(flags[1], 'val', image_id, 64) for image_id, _p in scenes}
    v = m.random_variables(cfg, 17)
    bias = 'text_sketchyscene/m_lstm_output_projection/biases'
    v[bias][:] = 0
    model = m.MatchModel(cfg)
    model.load_dict(v)
    up, _ = model.forward(gts['11']['sketch'], *m.preprocess_sentence('the house on the left', vocab, 15))
    v[bias][:] = -float(up.median())            # up straddles 0: about half of the strokes are predicted
    model.close()
    snap = tmp_path / 'snapshot'
    snap.mkdir()
    tf_checkpoint.write_checkpoint(str(snap / 'model-3'), v)
    (snap / 'checkpoint').write_text('model_checkpoint_path: "model-3"\n')
    code = ('import json, sys; sys.path.insert(0, %r); import match_main; '
            'from sketchyscenecolorization_amd.matching import MatchConfig; '
            'match_main.main(sys.argv[3:], config=MatchConfig(**json.loads(sys.argv[1])), predicts_out=sys.argv[2])' % ROOT)

    def run(tag, extra):
        results, dump = tmp_path / ('results_' + tag), tmp_path / ('predicts_%s.npy' % tag)
        argv = [sys.executable, '-c', code, json.dumps(SMALL), str(dump), '--mode', 'eval', '--snapshot', str(snap), '--vocab_file', VOCAB,
                '--scene_size', '64', '--eval_result_root', str(results)] + flags + extra
        r = subprocess.run(argv, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=CHILD_LIMIT, cwd=str(tmp_path))
        assert r.returncode == 0, r.stderr.decode()[-2000:]
        return (r.stdout.decode(), open(str(results / 'deeplab_RMI_val_result.txt')).read(),
                json.load(open(str(results / 'eval_val.json'))), np.load(str(dump)))
    vis = tmp_path / 'vis'
    printed0, block0, rec0, pred0 = run('plain', [])
    assert not vis.exists() and not (tmp_path / 'outputs').exists()
    printed, block, rec, pred = run('vis', ['--visualized', '1', '--visualize_pred_base_dir', str(vis)])
    assert block == block0 and block in printed and block0 in printed0 and rec == rec0 and np.array_equal(pred, pred0)
    assert pred.shape == (6, 64, 64) and 0 < (pred != 0).mean() < 1
    n = 0
    for image_id, pairs in scenes:
        d = vis / 'val' / image_id
        assert sorted(os.listdir(str(d))) == sorted(['captions.json'] + ['%d_%s.png' % (k, e) for k in range(3) for e in ('gt', 'out')])
        caps = json.load(open(str(d / 'captions.json')))
        assert caps['image_id'] == image_id and [c['caption'] for c in caps['captions']] == [c for c, _i in pairs]
        gt = gts[image_id]
        for k, (caption, idx) in enumerate(pairs):
            lut = np.zeros(256, np.uint8)
            lut[[i + 1 for i in idx]] = 1
            assert np.array_equal(_png(str(d / ('%d_out.png' % k))), PO.coloured(gt['sketch'], pred[n], None, None)), (image_id, k)
            assert np.array_equal(_png(str(d / ('%d_gt.png' % k))), PO.coloured(gt['sketch'], None, gt['labels'], lut)), (image_id, k)
            n += 1
