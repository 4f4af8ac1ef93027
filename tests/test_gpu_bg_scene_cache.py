"""Background training from a device scene cache: the gathering stage kernel (ssc_bg_stage_cached_u8) with its on-device
recolouring, BGTrainer.train_step_cached and bg_colorization_main.py --scene_cache device / --recolor 1 on top of them.

Every comparison is bit for bit: the kernel does the fp32 operations of u8 / 255 * 2 - 1 one by one on bytes it gathers, the
NumPy reference below does the same on the same bytes, and a train step fed by it launches the kernels of one fed by
hip.bg_stage_u8 on the same values."""
import faulthandler
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
from PIL import Image

pytestmark = pytest.mark.gpu

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIX = os.path.join(ROOT, 'tests', 'golden', 'bg_aug')
BLUE, GREEN = (153, 217, 234), (181, 230, 29)
CHILD_LIMIT = 180       # seconds a command-line child may take (start-up of a fresh process included)


@pytest.fixture(autouse=True)
def _time_limit():
    """A test that hangs on the device ends the process (with every thread's traceback) instead of holding the card."""
    faulthandler.dump_traceback_later(400, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


def unit_np(u8):
    return (u8.astype(F) / F(255)) * F(2) - F(1)


def labels_np(seg):
    return np.where(seg == 128, 1, np.where(seg == 255, 2, 0)).astype(np.int32)


def recolor_np(bg, seg, rec):
    """rec uint8 [8] = {enable, sky rgb, ground rgb, 0}: seg == 128 ? sky : seg == 255 ? ground : bg."""
    out = bg.copy()
    if rec is not None and rec[0]:
        out[seg == 128] = rec[1:4]
        out[seg == 255] = rec[4:7]
    return out


def ref_stage(fgc, bgc, segc, slots, recolor):
    """What ssc_bg_stage_cached_u8 writes: inputs, targets [N,H,W,3], xd [N,H,W,8], labels [N,H,W], count."""
    N, (H, W) = len(slots), segc.shape[1:]
    inputs, targets = np.empty((N, H, W, 3), F), np.empty((N, H, W, 3), F)
    labels = np.zeros((N, H, W), np.int32)
    bad = False
    for n, (sf, sb, ss) in enumerate(slots):
        if not (0 <= sf < len(fgc) and 0 <= sb < len(bgc) and 0 <= ss < len(segc)):
            inputs[n], targets[n], bad = np.nan, np.nan, True
            continue
        labels[n] = labels_np(segc[ss])
        inputs[n] = unit_np(fgc[sf])
        targets[n] = unit_np(recolor_np(bgc[sb], segc[ss], None if recolor is None else recolor[n]))
    xd = np.concatenate([inputs, targets, np.zeros((N, H, W, 2), F)], -1)
    return inputs, targets, xd, labels, (float('nan') if bad else float(np.count_nonzero(labels)))


def make_caches(rng, S, H, W):
    """S entries of each kind.  seg holds the three label values and values beside them (127, 129, 254, 1) that are label 0;
    bg entry e is a base scene over seg entry e (sky blue where it is 128, ground green where it is 255, any bytes elsewhere)."""
    seg = rng.choice(np.array([0, 128, 255, 127, 129, 254, 1], np.uint8), (S, H, W), p=[.2, .25, .25, .075, .075, .075, .075])
    fg = rng.randint(0, 256, (S, H, W, 3)).astype(np.uint8)
    bg = rng.randint(0, 256, (S, H, W, 3)).astype(np.uint8)
    bg[seg == 128] = BLUE
    bg[seg == 255] = GREEN
    fg.reshape(-1)[:2] = (0, 255)
    return fg, bg, seg


class Outputs(object):
    """The five outputs, each inside a larger allocation whose margins (16 bytes either side, so that the 16-byte alignment
    holds) must come back untouched; filled with values the kernel never writes."""

    def __init__(self, N, H, W):
        self.shapes = {'inputs': (N, H, W, 3), 'targets': (N, H, W, 3), 'xd': (N, H, W, 8), 'labels': (N, H, W), 'count': (1,)}
        self.raw, self.t = {}, {}
        for k, s in self.shapes.items():
            n = int(np.prod(s))
            if k == 'labels':
                self.raw[k] = torch.full((n + 8,), -7, dtype=torch.int32, device='cuda')
            else:
                self.raw[k] = torch.full((n + 8,), 7.5, dtype=torch.float32, device='cuda')
            self.t[k] = self.raw[k][4:4 + n].view(s)

    def check_margins(self):
        for k, r in self.raw.items():
            fill = -7 if k == 'labels' else 7.5
            assert bool((r[:4] == fill).all()) and bool((r[-4:] == fill).all()), k + ': written outside the array'


def run_stage(fgc, bgc, segc, slots, recolor):
    from sketchyscenecolorization_amd import hip
    N, (H, W) = len(slots), segc.shape[1:]
    o = Outputs(N, H, W)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()      # noqa: E731
    hip.bg_stage_cached_u8(dev(fgc), dev(bgc), dev(segc), dev(np.asarray(slots, np.int32)),
                           None if recolor is None else dev(recolor), o.t['inputs'], o.t['targets'], o.t['xd'], o.t['labels'],
                           o.t['count'])
    torch.cuda.synchronize()
    o.check_margins()
    return o


def assert_stage(o, want):
    for k, w in zip(('inputs', 'targets', 'xd', 'labels'), want[:4]):
        got = o.t[k].cpu().numpy()
        assert got.dtype == w.dtype and np.array_equal(got, w, equal_nan=True), k
    assert float(o.t['xd'][..., 6:].abs().max()) == 0.0
    c = float(o.t['count'].item())
    assert (np.isnan(c) and np.isnan(want[4])) or c == want[4], (c, want[4])


def pair_record(sky, ground, enable=1):
    return np.array((enable,) + tuple(sky) + tuple(ground) + (0,), np.uint8)


# N = 3 from caches of 4: a repeated entry, descending order, different fg, bg and seg entries per sample
SLOTS = [[3, 1, 2], [3, 0, 0], [1, 2, 3]]
# P = 35: entries and float rows start off every alignment; 36: aligned throughout; 4160: 5 workgroups of 4-pixel groups
SHAPES = [(5, 7), (6, 6), (64, 65)]


def recolor_case(name, N):
    if name == 'null':
        return None
    rec = np.stack([pair_record((163, 73, 164), (255, 242, 0)), pair_record((1, 2, 3), (4, 5, 6), enable=0),
                    pair_record((30, 30, 30), (127, 127, 127)), pair_record((255, 174, 201), (185, 122, 87))][:N])
    if name == 'identity':
        rec[:] = pair_record(BLUE, GREEN)
    return rec


@pytest.mark.parametrize('recolor', ['null', 'some', 'identity'])
@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_cached_stage_kernel(shape, recolor):
    """Against NumPy, and against hip.bg_stage_u8 on the arrays the slots gather."""
    from sketchyscenecolorization_amd import hip
    H, W = shape
    fgc, bgc, segc = make_caches(np.random.RandomState(H * 100 + W), 4, H, W)
    # the identity needs each background over its own segment map: (blue, green) on a base scene changes nothing
    slots = [[3, 1, 1], [3, 0, 0], [1, 2, 2]] if recolor == 'identity' else SLOTS
    rec = recolor_case(recolor, 3)
    want = ref_stage(fgc, bgc, segc, slots, rec)
    assert 0 < want[4] < 3 * H * W
    if recolor == 'identity':
        assert all(np.array_equal(w, n) for w, n in zip(want[:4], ref_stage(fgc, bgc, segc, slots, None)[:4]))
    if recolor == 'some':
        plain = ref_stage(fgc, bgc, segc, slots, None)
        assert not np.array_equal(want[1][0], plain[1][0]) and np.array_equal(want[1][1], plain[1][1])       # sample 1: enable = 0
    o = run_stage(fgc, bgc, segc, slots, rec)
    assert_stage(o, want)
    # the uncached kernel on the gathered (and, on the host, recoloured) scenes
    s = np.array(slots)
    g_bg = np.stack([recolor_np(bgc[sb], segc[ss], None if rec is None else rec[n]) for n, (sf, sb, ss) in enumerate(slots)])
    u = Outputs(3, H, W)
    hip.bg_stage_u8(torch.from_numpy(fgc[s[:, 0]]).cuda(), torch.from_numpy(g_bg).cuda(),
                    torch.from_numpy(labels_np(segc[s[:, 2]])).cuda(), u.t['inputs'], u.t['targets'], u.t['xd'], u.t['count'])
    torch.cuda.synchronize()
    for k in ('inputs', 'targets', 'xd', 'count'):
        assert torch.equal(o.t[k], u.t[k]), k


def test_cached_stage_kernel_flagship_shape():
    """N = 4 at 768 x 768: more 4-pixel groups than the 2048 workgroups the launcher caps the grid at have threads."""
    H = W = 768
    fgc, bgc, segc = make_caches(np.random.RandomState(768), 4, H, W)
    slots = SLOTS + [[0, 3, 1]]
    rec = recolor_case('some', 4)
    assert_stage(run_stage(fgc, bgc, segc, slots, rec), ref_stage(fgc, bgc, segc, slots, rec))


@pytest.mark.parametrize('bad', [[3, 1, 4], [-1, 0, 0], [3, 2 ** 30, 0]], ids=['seg-past-end', 'fg-negative', 'bg-huge'])
def test_cached_stage_kernel_slot_out_of_range(bad):
    """The sample with the bad slot: NaN floats (pad lanes 0), labels 0; the count NaN; the other samples exact.  The kernel
    tests the slot before it forms an address, so nothing is read."""
    H, W = 5, 7
    fgc, bgc, segc = make_caches(np.random.RandomState(3), 4, H, W)
    slots = [SLOTS[0], bad, SLOTS[2]]
    rec = recolor_case('some', 3)
    rec[1, 0] = 1
    want = ref_stage(fgc, bgc, segc, slots, rec)
    assert np.isnan(want[4]) and np.isnan(want[0][1]).all() and not np.isnan(want[0][0]).any()
    o = run_stage(fgc, bgc, segc, slots, rec)
    assert_stage(o, want)
    assert bool(torch.isnan(o.t['xd'][1, ..., :6]).all()) and int(o.t['labels'][1].abs().sum()) == 0
    # a good launch afterwards finds the state word as this one left it
    assert_stage(run_stage(fgc, bgc, segc, SLOTS, rec), ref_stage(fgc, bgc, segc, SLOTS, rec))


def test_cached_stage_kernel_refuses_bad_arguments():
    from sketchyscenecolorization_amd import hip
    z = lambda shape, dt: torch.zeros(shape, dtype=dt, device='cuda')      # noqa: E731
    c3, c1 = z((2, 8, 8, 3), torch.uint8), z((2, 8, 8), torch.uint8)
    slot, rec = z((1, 3), torch.int32), z((2, 8), torch.uint8)
    f3, f8, lab, cnt = z((1, 8, 8, 3), torch.float32), z((1, 8, 8, 8), torch.float32), z((1, 8, 8), torch.int32), z((1,), torch.float32)
    ws = hip.workspace()
    names = ('fg', 'S_fg', 'bg', 'S_bg', 'seg', 'S_seg', 'slot', 'rec', 'N', 'P', 'i', 't', 'xd', 'lab', 'c', 'ws', 'wsb')
    base = dict(fg=hip.ptr(c3), S_fg=2, bg=hip.ptr(c3), S_bg=2, seg=hip.ptr(c1), S_seg=2, slot=hip.ptr(slot), rec=hip.ptr(rec), N=1,
                P=64, i=hip.ptr(f3), t=hip.ptr(f3), xd=hip.ptr(f8), lab=hip.ptr(lab), c=hip.ptr(cnt), ws=hip.ptr(ws),
                wsb=ws.numel() * 4)
    call = lambda **kw: hip.lib().ssc_bg_stage_cached_u8(*([kw.get(k, base[k]) for k in names] + [hip.stream_ptr()]))      # noqa: E731
    off = lambda t, n=1: hip.ptr(t.view(-1)[n:])      # noqa: E731
    assert call() == 0 and call(rec=None) == 0
    assert call(N=0) == -1 and call(P=0) == -1 and call(N=-1) == -1
    assert call(N=1 << 12, P=(1 << 12) + 1) == -1 and call(N=(1 << 24) + 1, P=1) == -1 and call(N=1 << 40, P=1 << 40) == -1
    assert call(S_fg=0) == -1 and call(S_seg=1 << 31) == -1
    assert call(wsb=4) == -2 and call(ws=off(ws)) == -2
    for k, t in (('fg', c3), ('bg', c3), ('seg', c1)):
        assert call(**{k: off(t)}) == -3, k
    assert call(slot=off(slot.view(torch.uint8), 2)) == -3 and call(rec=off(rec, 4)) == -3
    for k, t in (('i', f3), ('t', f3), ('xd', f8), ('lab', lab)):
        assert call(**{k: off(t)}) == -3, k
    torch.cuda.synchronize()


def _fix_png(kind, name):
    return np.array(Image.open(os.path.join(FIX, kind, 'train', name)).convert('RGB'), dtype=np.uint8)


@pytest.mark.parametrize('scene', ['scene_a.png', 'scene_b.png'])
def test_cached_stage_kernel_makes_the_reference_generators_backgrounds(scene):
    """The base scene of the fixture cached, recolor = the pair of each record the reference's generator wrote for it (the
    base one included): targets is u8 / 255 * 2 - 1 of that record's own background png, labels what load_region_mask reads."""
    from sketchyscenecolorization_amd.data_processing import bg_palette as pal
    from sketchyscenecolorization_amd.data_processing.image_processing import load_region_mask
    with open(os.path.join(FIX, 'captions', 'train.json')) as fp:
        recs = [r for r in json.load(fp) if r['fg_name'] == scene]
    assert len(recs) == 4
    fg, bg, seg = _fix_png('foreground', scene), _fix_png('background', scene), _fix_png('segment', scene)[:, :, 0]
    rec = np.stack([pal.recolor_record(r['color_text'].split()[3], r['color_text'].split()[-1]) for r in recs])
    o = run_stage(fg[None], bg[None], seg[None], [[0, 0, 0]] * 4, rec)
    lab = load_region_mask(os.path.join(FIX, 'segment', 'train', scene), 0)
    for n, r in enumerate(recs):
        want = unit_np(_fix_png('background', r['bg_name']))
        assert np.array_equal(o.t['targets'][n].cpu().numpy(), want), r
        assert np.array_equal(o.t['inputs'][n].cpu().numpy(), unit_np(fg))
        assert np.array_equal(o.t['labels'][n].cpu().numpy(), lab[0])
    assert not np.array_equal(o.t['targets'][1].cpu().numpy(), o.t['targets'][0].cpu().numpy())
    assert float(o.t['count'].item()) == 4.0 * np.count_nonzero(lab)


def _assert_same_state(a, b):
    for sa, sb in ((a.store.generator, b.store.generator), (a.store.discriminator, b.store.discriminator)):
        assert sa.adam_t == sb.adam_t
        for name in ('flat', 'adam_m', 'adam_v'):
            assert torch.equal(getattr(sa, name), getattr(sb, name)), (sa.name, name)
    assert a.global_step == b.global_step


@pytest.mark.parametrize('use_graphs', [False, True], ids=['eager', 'graph'])
def test_train_step_cached_is_the_u8_step(use_graphs):
    """Three steps at N = 2, 64 x 64 (with graphs: one eager, one captured, one replayed): every weight and both Adam states
    as from train_step_u8 fed the same scenes; with graphs also as from an eager trainer fed from the cache.  The second step
    recolours one sample (the uint8 trainer gets that background painted on the host), the third none again."""
    import bg_colorization_main as bgcli
    from sketchyscenecolorization_amd.bg_colorization import BGTrainer
    from sketchyscenecolorization_amd.scene_cache import SceneCache
    p = {'image_size': 64, 'text_len': 8, 'data_base_dir': 'no_such_dir', 'mode': 'train', 'vocab_size': 18}
    scenes = bgcli.Scenes(p)
    cache = SceneCache(scenes, device='cuda')
    assert cache.fg.is_cuda and cache.fg.shape == (8, 64, 64, 3) and cache.nbytes == 8 * 64 * 64 * 7
    a = BGTrainer(image_size=64, max_steps=10, seed=4, use_graphs=use_graphs)
    b = BGTrainer(image_size=64, max_steps=10, seed=4, use_graphs=use_graphs)
    c = BGTrainer(image_size=64, max_steps=10, seed=4, use_graphs=False) if use_graphs else None
    paint = np.stack([pair_record((1, 2, 3), (4, 5, 6), enable=0), pair_record((163, 73, 164), (255, 242, 0))])
    for idxs, rec in (((0, 5), None), ((3, 3), paint), ((7, 1), None)):
        got = [scenes.get(i) for i in idxs]
        fg, tok, lab = [np.concatenate([g[k] for g in got], 0) for k in (0, 2, 3)]
        bg = np.stack([recolor_np(g[1][0], cache.seg[i].cpu().numpy(), None if rec is None else rec[n])
                       for n, (i, g) in enumerate(zip(idxs, got))])
        if rec is not None:
            assert not np.array_equal(bg[1], got[1][1][0]) and np.array_equal(bg[0], got[0][1][0])
        a.train_step_cached(cache, cache.slots[list(idxs)], rec, tok)
        b.train_step_u8(fg, bg, tok, lab)
        if c is not None:
            c.train_step_cached(cache, cache.slots[list(idxs)], rec, tok)
        torch.cuda.synchronize()
        _assert_same_state(a, b)
        if c is not None:
            _assert_same_state(a, c)
    if use_graphs:
        assert len(a._graphs) == 1 and a.use_graphs, 'the cached step was not captured'
    la, lb = a.loss_values(), b.loss_values()
    assert all(np.isfinite(la)) and all(abs(x - y) <= 1e-9 * max(1.0, abs(y)) for x, y in zip(la, lb)), (la, lb)


def test_entry_points_taken_in_turn_share_one_runner_and_its_buffers():
    """Six steps at N = 2, 64 x 64 that alternate train_step_u8 and train_step_cached on one trainer with graphs: each of the
    two keys goes eager, captured, replayed, between steps of the other that write the same named buffers ('xd_real',
    'l1_count', the gradient scratch).  Weights and all four Adam moments are those of an eager trainer fed train_step_u8 six
    times on the same scenes, bit for bit; the loss words agree to the 1e-9 of atomically summed doubles."""
    import bg_colorization_main as bgcli
    from sketchyscenecolorization_amd.bg_colorization import BGTrainer
    from sketchyscenecolorization_amd.scene_cache import SceneCache
    p = {'image_size': 64, 'text_len': 8, 'data_base_dir': 'no_such_dir', 'mode': 'train', 'vocab_size': 18}
    scenes = bgcli.Scenes(p)
    cache = SceneCache(scenes, device='cuda')
    a = BGTrainer(image_size=64, max_steps=10, seed=4, use_graphs=True)
    b = BGTrainer(image_size=64, max_steps=10, seed=4, use_graphs=False)
    for step, idxs in enumerate(((0, 5), (3, 3), (7, 1), (2, 6), (4, 0), (1, 7))):
        got = [scenes.get(i) for i in idxs]
        fg, bg, tok, lab = [np.concatenate([g[k] for g in got], 0) for k in (0, 1, 2, 3)]
        if step % 2 == 0:
            a.train_step_u8(fg, bg, tok, lab)
        else:
            a.train_step_cached(cache, cache.slots[list(idxs)], None, tok)
        b.train_step_u8(fg, bg, tok, lab)
        torch.cuda.synchronize()
        _assert_same_state(a, b)
        la, lb = a.losses.cpu(), b.losses.cpu()
        assert bool(torch.isfinite(la).all()) and la.shape == (5,)
        assert float((la - lb).abs().max()) <= 1e-9 * max(1.0, float(lb.abs().max())), (step, la.tolist(), lb.tolist())
    assert len(a._graphs) == 2 and a.use_graphs


def _cli(cwd, seed, argv):
    """bg_colorization_main.py in a process of its own, under its own time limit, after random.seed(seed)."""
    code = ('import random, sys; sys.path.insert(0, %r); random.seed(%d); import bg_colorization_main as m; m.main(%r)'
            % (ROOT, seed, list(argv)))
    os.makedirs(str(cwd), exist_ok=True)
    r = subprocess.run([sys.executable, '-c', code], cwd=str(cwd), stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       universal_newlines=True, timeout=CHILD_LIMIT)
    assert r.returncode == 0, r.stdout[-4000:]
    stamp = sorted(os.listdir(os.path.join(str(cwd), 'outputs')))[0]
    return os.path.join(str(cwd), 'outputs', stamp), r.stdout


@pytest.mark.parametrize('nb', [1, 2])
def test_cli_scene_cache_is_the_uncached_run(tmp_path, nb):
    """64 x 64 synthetic scenes, same seed: snapshot-3 of --scene_cache device holds the bits of --scene_cache off."""
    argv = ['--mode', 'train', '--batch_size', str(nb), '--image_size', '64', '--max_steps', '3', '--save_freq', '3',
            '--progress_freq', '1', '--summary_freq', '1']
    snaps = []
    for mode in ('off', 'device'):
        out, text = _cli(tmp_path / mode, 31, argv + ['--scene_cache', mode])
        assert ('scene cache: 8 scenes' in text) == (mode == 'device'), text[-2000:]
        snaps.append(torch.load(os.path.join(out, 'snapshot', 'snapshot-3'), map_location='cpu'))
    assert snaps[0].keys() == snaps[1].keys() and len(snaps[0]) > 50
    for k in snaps[0]:
        assert torch.equal(torch.as_tensor(snaps[0][k]), torch.as_tensor(snaps[1][k])), k


def test_cli_recolor_trains_from_png_files(tmp_path):
    """--recolor 1 on a dataset of three 64 x 64 base scenes (and one augmented record, which it leaves out): three steps at
    batch 2 with finite losses."""
    rng = np.random.RandomState(9)
    base = tmp_path / 'data'
    for kind in ('foreground', 'background', 'segment', 'captions'):
        os.makedirs(str(base / kind / ('train' if kind != 'captions' else '')))
    recs = []
    for i in range(3):
        name = 'scene_%d.png' % i
        seg = np.zeros((64, 64), np.uint8)
        seg[:30 + 2 * i] = 128
        seg[34 + 2 * i:] = 255
        seg[20:44, 10 + 5 * i:30 + 5 * i] = 0
        fg = np.full((64, 64, 3), 255, np.uint8)
        fg[20:44, 10 + 5 * i:30 + 5 * i] = rng.randint(0, 256, (24, 20, 3))
        bg = np.where((seg == 128)[..., None], np.array(BLUE, np.uint8), np.where((seg == 255)[..., None], np.array(GREEN, np.uint8), fg))
        bg[30 + 2 * i:34 + 2 * i] = 40
        Image.fromarray(fg, 'RGB').save(str(base / 'foreground' / 'train' / name))
        Image.fromarray(bg.astype(np.uint8), 'RGB').save(str(base / 'background' / 'train' / name))
        Image.fromarray(seg, 'L').save(str(base / 'segment' / 'train' / name))
        recs.append({'fg_name': name, 'bg_name': name, 'color_text': 'the sky is blue and the ground is green'})
    recs.insert(1, {'fg_name': 'scene_0.png', 'bg_name': 'no_such_file_1.png', 'color_text': 'the sky is red and the ground is gray'})
    with open(str(base / 'captions' / 'train.json'), 'w') as fp:
        json.dump(recs, fp)
    out, text = _cli(tmp_path / 'run', 7, ['--mode', 'train', '--batch_size', '2', '--image_size', '64', '--max_steps', '3', '--save_freq', '0',
                                           '--progress_freq', '1', '--summary_freq', '1', '--scene_cache', 'device', '--recolor', '1',
                                           '--data_base_dir', str(base), '--vocab_file', os.path.join(FIX, 'bg_vocab.txt')])
    assert 'scene cache: 3 scenes from 3 foregrounds, 3 backgrounds, 3 segment maps' in text, text[-2000:]
    with open(os.path.join(out, 'log', 'scalars.jsonl')) as fp:
        rows = [json.loads(l) for l in fp]
    assert [r['step'] for r in rows] == [1, 2, 3]
    for r in rows:
        assert all(np.isfinite(v) for v in r.values()), r
