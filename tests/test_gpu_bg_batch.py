"""Background training at --batch_size N from the loader's uint8 arrays: the fused stage kernel (ssc_bg_stage_u8), the device
post-process of test mode (ssc_bg_finish_u8), BGTrainer.train_step_u8 and the command line on top of them.

Every comparison here is bit for bit: the kernels do the fp32 operations of bg_colorization_main.to_unit / to_u8 one by one,
and a train step fed by the stage kernel launches the same arithmetic kernels on the same values as one fed with floats."""
import faulthandler
import glob
import os
import random
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

F = np.float32


@pytest.fixture(autouse=True)
def _time_limit():
    """A test that hangs on the device ends the process (with every thread's traceback) instead of holding the card."""
    faulthandler.dump_traceback_later(120, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


def unit_np(u8):
    return (u8.astype(F) / F(255)) * F(2) - F(1)


def to_u8_np(x):
    y = np.minimum(np.maximum((x + F(1)) / F(2), F(0)), F(1)) * F(255)
    return np.clip(np.floor(y + F(0.5)), 0, 255).astype(np.uint8)


def _bytes(rng, shape):
    """Random bytes that hold 0, 255 and every value between them (when there is room for 256 of them)."""
    a = rng.randint(0, 256, shape).astype(np.uint8)
    flat = a.reshape(-1)
    if flat.size >= 256:
        flat[rng.permutation(flat.size)[:256]] = np.arange(256, dtype=np.uint8)
        assert len(np.unique(a)) == 256
    return a


def test_to_unit_divides():
    """to_unit is the formula the stage kernel is held to, for every byte value (torch evaluates ``x / 255.0`` with a Python
    divisor as x * fl(1 / 255), one ulp off for 111 of them: the divisor is a device tensor for that reason)."""
    import bg_colorization_main as bgcli
    u8 = np.arange(256, dtype=np.uint8)
    assert np.array_equal(bgcli.to_unit(u8).cpu().numpy(), unit_np(u8))


# (N, H, W): the last two have N*H*W not a multiple of the 4 pixels a thread owns; 4 x 768^2 is the shape of the flagship step
# and more groups than the grid has threads
STAGE_SHAPES = [(1, 64, 64), (3, 64, 64), (1, 96, 96), (3, 96, 96), (1, 31, 33), (3, 5, 7), (4, 768, 768)]


@pytest.mark.parametrize('labels', ['mixed', 'all_zero', 'all_nonzero'])
@pytest.mark.parametrize('shape', STAGE_SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_stage_kernel(shape, labels):
    from sketchyscenecolorization_amd import hip
    from sketchyscenecolorization_amd.bg_colorization import BGTrainer
    from sketchyscenecolorization_amd.params import Buffers
    N, H, W = shape
    rng = np.random.RandomState(N * 1000 + H)
    fg, bg = _bytes(rng, (N, H, W, 3)), _bytes(rng, (N, H, W, 3))
    lab = {'mixed': rng.randint(0, 3, (N, H, W)), 'all_zero': np.zeros((N, H, W)),
           'all_nonzero': rng.randint(1, 3, (N, H, W))}[labels].astype(np.int32)
    garbage = lambda *s: torch.full(s, float('nan'), device='cuda')      # noqa: E731
    inputs, targets, xd, count = garbage(N, H, W, 3), garbage(N, H, W, 3), garbage(N, H, W, 8), garbage(1)
    hip.bg_stage_u8(torch.from_numpy(fg).cuda(), torch.from_numpy(bg).cuda(), torch.from_numpy(lab).cuda(), inputs, targets, xd,
                    count)
    torch.cuda.synchronize()
    assert np.array_equal(inputs.cpu().numpy(), unit_np(fg))
    assert np.array_equal(targets.cpu().numpy(), unit_np(bg))
    # the pair BGTrainer._pack builds from the same images (it needs the trainer's buffers only)
    packed = BGTrainer._pack(types.SimpleNamespace(bufs=Buffers('cuda')), 'xd_real', inputs, targets)
    assert torch.equal(xd, packed) and float(xd[..., 6:].abs().max()) == 0.0
    assert float(count.item()) == float(np.count_nonzero(lab))
    # a second launch finds the state word as the first left it
    count.fill_(-1.0)
    hip.bg_stage_u8(torch.from_numpy(fg).cuda(), torch.from_numpy(bg).cuda(), torch.from_numpy(lab).cuda(), inputs, targets, xd,
                    count)
    assert float(count.item()) == float(np.count_nonzero(lab))


def test_stage_kernel_refuses_bad_arguments():
    from sketchyscenecolorization_amd import hip
    u8 = torch.zeros((1, 8, 8, 3), dtype=torch.uint8, device='cuda')
    lab = torch.zeros((1, 8, 8), dtype=torch.int32, device='cuda')
    f3, f8, cnt = torch.zeros((1, 8, 8, 3), device='cuda'), torch.zeros((1, 8, 8, 8), device='cuda'), torch.zeros(1, device='cuda')
    ws = hip.workspace()
    args = lambda **kw: [kw.get(k, v) for k, v in (('fg', hip.ptr(u8)), ('bg', hip.ptr(u8)), ('lab', hip.ptr(lab)), ('M', 64),     # noqa: E731
                                                   ('i', hip.ptr(f3)), ('t', hip.ptr(f3)), ('xd', hip.ptr(f8)), ('c', hip.ptr(cnt)),
                                                   ('ws', hip.ptr(ws)), ('wsb', ws.numel() * 4))] + [hip.stream_ptr()]
    lib = hip.lib()
    assert lib.ssc_bg_stage_u8(*args()) == 0
    assert lib.ssc_bg_stage_u8(*args(M=0)) == -1 and lib.ssc_bg_stage_u8(*args(M=(1 << 24) + 1)) == -1
    assert lib.ssc_bg_stage_u8(*args(wsb=4)) == -2
    assert lib.ssc_bg_stage_u8(*args(fg=hip.ptr(u8.view(-1)[1:]))) == -3
    assert lib.ssc_bg_stage_u8(*args(xd=hip.ptr(f8.view(-1)[1:]))) == -3
    torch.cuda.synchronize()


def _finish_images(rng, shape, ldc):
    """Floats in [-1.2, 1.2] (both saturations), among them values x for which clamp((x + 1) / 2) * 255 + 0.5 is an exact
    integer in fp32 -- the ties of floor(. + 0.5), where a truncating or round-to-even cast gives another byte -- and their two
    neighbours."""
    N, H, W = shape
    x = rng.uniform(-1.2, 1.2, (N, H, W, ldc)).astype(F)
    k = np.arange(1, 256, dtype=np.float64)
    ties = (2.0 * (k - 0.5) / 255.0 - 1.0).astype(F)
    ties = np.concatenate([ties, np.nextafter(ties, F(2)), np.nextafter(ties, F(-2)), np.array([-1.0, 1.0, -1.2, 1.2, 0.0], F)])
    y = np.minimum(np.maximum((ties + F(1)) / F(2), F(0)), F(1)) * F(255) + F(0.5)
    exact = int((y == np.floor(y)).sum())
    flat = x.reshape(-1, ldc)
    n = min(len(ties), flat.shape[0] * 3)
    rows = rng.permutation(flat.shape[0] * 3)[:n]
    flat[rows // 3, rows % 3] = ties[:n]
    return x, exact


@pytest.mark.parametrize('masked', [False, True])
@pytest.mark.parametrize('ldc', [3, 4, 8])       # 16-byte loads over dense rows, one per 4-float row, and the float-at-a-time path
@pytest.mark.parametrize('shape', [(1, 64, 64), (2, 31, 33), (1, 768, 768)], ids=lambda s: 'x'.join(map(str, s)))
def test_finish_kernel(shape, ldc, masked):
    from sketchyscenecolorization_amd import hip
    N, H, W = shape
    rng = np.random.RandomState(H + ldc)
    x, exact = _finish_images(rng, shape, ldc)
    assert exact >= 100, exact        # the constructed ties are ties in fp32
    fg = _bytes(rng, (N, H, W, 3))
    mask = rng.choice(np.array([0, 0, 1, 128, 255], np.uint8), (N, H, W))
    want = to_u8_np(x[..., :3])
    if masked:
        want[mask == 0] = fg[mask == 0]
    out = torch.full((N, H, W, 3), 77, dtype=torch.uint8, device='cuda')
    got = hip.bg_finish_u8(torch.from_numpy(x).cuda(), torch.from_numpy(fg).cuda() if masked else None,
                           torch.from_numpy(mask).cuda() if masked else None, out=out)
    assert got is out
    assert np.array_equal(got.cpu().numpy(), want)
    assert want.min() == 0 and want.max() == 255


def _scene_batch(scenes, idxs):
    got = [scenes.get(i) for i in idxs]
    return [np.concatenate([g[k] for g in got], 0) for k in range(4)]      # fg, bg, tok, lab


def _assert_same_state(a, b):
    for sa, sb in ((a.store.generator, b.store.generator), (a.store.discriminator, b.store.discriminator)):
        assert sa.adam_t == sb.adam_t
        for name in ('flat', 'adam_m', 'adam_v'):
            assert torch.equal(getattr(sa, name), getattr(sb, name)), (sa.name, name)
    assert a.global_step == b.global_step


@pytest.mark.parametrize('use_graphs', [False, True], ids=['eager', 'graph'])
def test_train_step_u8_is_the_float_step(use_graphs):
    """Three steps at N = 2, 64 x 64 (with graphs: one eager, one captured, one replayed): every weight and both Adam
    states as from train_step fed with to_unit of the same arrays."""
    import bg_colorization_main as bgcli
    from sketchyscenecolorization_amd.bg_colorization import BGTrainer
    p = {'image_size': 64, 'text_len': 8, 'data_base_dir': 'no_such_dir', 'mode': 'train', 'vocab_size': 18}
    scenes = bgcli.Scenes(p)
    a = BGTrainer(image_size=64, max_steps=10, seed=4, use_graphs=use_graphs)
    b = BGTrainer(image_size=64, max_steps=10, seed=4, use_graphs=use_graphs)
    for idxs in ((0, 5), (3, 3), (7, 1)):
        fg, bg, tok, lab = _scene_batch(scenes, idxs)
        a.train_step_u8(fg, bg, tok, lab)
        b.train_step(bgcli.to_unit(fg), bgcli.to_unit(bg), tok, torch.from_numpy(lab).cuda())
        torch.cuda.synchronize()
        _assert_same_state(a, b)
    if use_graphs:
        assert len(a._graphs) == 1 and a.use_graphs, 'the uint8 step was not captured'
    la, lb = a.loss_values(), b.loss_values()
    assert all(np.isfinite(la)) and all(abs(x - y) <= 1e-9 * max(1.0, abs(y)) for x, y in zip(la, lb)), (la, lb)


def _filter_with_planes(hip, scope, name=None):
    """(name, plane entries) of one filter of ``scope`` that owns persistent bf16 planes: the first by name, or ``name``."""
    lo, hi = scope.flat.data_ptr(), scope.flat.data_ptr() + scope.flat.numel() * scope.flat.element_size()
    at = {v.data_ptr(): n for n, v in scope.p.items()}
    owned = {}
    for e in hip._SPLITS.values():
        if e.param and lo <= e.key[0] < hi and e.key[0] in at:
            owned.setdefault(at[e.key[0]], []).append(e)
    if name is None:
        assert owned, 'no generator filter owns persistent planes at this size'
        name = sorted(owned)[0]
    assert name in owned, (name, 'owns no planes on this trainer')
    return name, owned[name]


def test_replayed_step_follows_a_filter_written_through_torch():
    """A replayed Background step launches into the ADDRESSES of the filters' bf16 planes: a filter scaled in place through its
    store view between two replays must reach its planes in front of the next one (hip.resplit_stale), or the step would train
    on with the old weights in its bf16 layers.  Three uint8 steps at N = 2, 64 x 64 (eager, captured, replayed) on a trainer
    with graphs and on one without, one generator filter halved on both, a fourth step: every weight and both Adam states
    stay bit for bit the eager trainer's.  64 x 64 at N = 2 is the size used: generator filters own planes there (the test
    fails, it does not pass, where none does)."""
    import bg_colorization_main as bgcli
    from sketchyscenecolorization_amd import hip
    from sketchyscenecolorization_amd.bg_colorization import BGTrainer
    if not hip.ARITH_BF16:
        pytest.skip('SSC_ARITH=fp32: no planes')
    scenes = bgcli.Scenes({'image_size': 64, 'text_len': 8, 'data_base_dir': 'no_such_dir', 'mode': 'train', 'vocab_size': 18})
    a = BGTrainer(image_size=64, max_steps=10, seed=4, use_graphs=True)
    b = BGTrainer(image_size=64, max_steps=10, seed=4, use_graphs=False)

    def step(idxs):
        fg, bg, tok, lab = _scene_batch(scenes, idxs)
        for tr in (a, b):
            tr.train_step_u8(fg, bg, tok, lab)
        torch.cuda.synchronize()
        _assert_same_state(a, b)

    for idxs in ((0, 5), (3, 3), (7, 1)):
        step(idxs)
    assert len(a._graphs) == 1 and a.use_graphs and not b._graphs, 'the uint8 step was not captured'
    name, planes_a = _filter_with_planes(hip, a.store.generator)
    _, planes_b = _filter_with_planes(hip, b.store.generator, name)
    before = a.store.generator.flat.clone()
    for tr in (a, b):
        tr.store.generator.p[name].mul_(0.5)
    assert all(e.version != e.w._version for e in planes_a + planes_b), 'the planes do not know their filter was written'
    step((2, 6))
    assert all(e.version == e.w._version for e in planes_a + planes_b), (name, 'a plane was not split again')
    assert not torch.equal(a.store.generator.flat, before)


def _hand_trained(bgcli, nb, steps, seed):
    """The trainer the command line builds after random.seed(seed), stepped on the float path over the scenes it draws."""
    from sketchyscenecolorization_amd.bg_colorization import BGTrainer
    p = {'image_size': 64, 'text_len': 8, 'data_base_dir': 'data', 'mode': 'train', 'vocab_size': 18}
    scenes = bgcli.Scenes(p)
    random.seed(seed)
    tr = BGTrainer(image_size=64, max_steps=steps, seed=random.randint(0, 2 ** 31 - 1))
    for _ in range(steps):
        fg, bg, tok, lab = _scene_batch(scenes, [random.randint(0, len(scenes) - 1) for _ in range(nb)])
        tr.train_step(bgcli.to_unit(fg), bgcli.to_unit(bg), tok, torch.from_numpy(lab).cuda())
    torch.cuda.synchronize()
    sd = tr.store.state_dict()
    for sc in (tr.store.generator, tr.store.discriminator):
        sd['__adam_m__/' + sc.name] = sc.adam_m.detach().cpu()
    return sd


def _assert_same_snapshot(got, want):
    assert got.keys() == want.keys() and len(got) > 50
    for k in want:
        assert torch.equal(torch.as_tensor(got[k]), torch.as_tensor(want[k])), k


@pytest.mark.parametrize('nb,prefetch', [(2, '4'), (1, '4'), (2, '0')], ids=['batch2', 'batch1', 'batch2-no-prefetch'])
def test_cli_trains_at_batch_size(tmp_path, monkeypatch, nb, prefetch):
    """--batch_size 2 (refused before this feature) and 1: snapshot-3 holds, bit for bit, the weights and Adam states of a
    BGTrainer stepped by hand on the float path over the same scenes in draw order (to_unit: at batch 1 the step the command
    line made before, up to the one ulp by which to_unit's division differs from the earlier multiplication by 1/255).  With
    SSC_BG_PREFETCH=0 the loader draws and loads a batch where it is used: the same scenes in the same order."""
    import bg_colorization_main as bgcli
    monkeypatch.chdir(tmp_path)
    monkeypatch.setenv('SSC_BG_PREFETCH', prefetch)
    random.seed(31)
    bgcli.main(['--mode', 'train', '--batch_size', str(nb), '--image_size', '64', '--max_steps', '3', '--save_freq', '3',
                '--progress_freq', '1', '--summary_freq', '1'])
    stamp = sorted(os.listdir('outputs'))[0]
    snap = os.path.join('outputs', stamp, 'snapshot', 'snapshot-3')
    assert os.path.exists(snap) and not os.path.exists(snap[:-1] + '2')
    _assert_same_snapshot(torch.load(snap, map_location='cpu'), _hand_trained(bgcli, nb, 3, 31))
    if (nb, prefetch) != (2, '4'):
        return
    # test mode on that snapshot: one image per pass whatever --batch_size says, the saturating cast and the paste-back on
    # the device.  Scenes 0 and 5 get a segment map (0 = foreground), so that the paste-back runs.
    from PIL import Image
    from sketchyscenecolorization_amd.bg_colorization import BGTrainer
    os.makedirs(os.path.join('data', 'segment', 'test'))
    rng = np.random.RandomState(2)
    segs = {}
    for i in (0, 5):
        segs[i] = rng.choice(np.array([0, 128, 255], np.uint8), (64, 64))
        Image.fromarray(segs[i], 'L').save(os.path.join('data', 'segment', 'test', 'synthetic_%d.png' % i))
    bgcli.main(['--mode', 'test', '--resume_from', stamp, '--image_size', '64', '--batch_size', '2'])
    res = os.path.join('outputs', stamp, 'results')
    assert len(glob.glob(os.path.join(res, '*.png'))) == 24
    tr = BGTrainer(image_size=64, seed=0)
    tr.store.load_state_dict(torch.load(snap, map_location='cpu'))
    scenes = bgcli.Scenes({'image_size': 64, 'text_len': 8, 'data_base_dir': 'data', 'mode': 'test', 'vocab_size': 18})
    pasted = 0
    for i in range(len(scenes)):
        fg, bg, tok, lab, fg_name, bg_name = scenes.get(i, is_test=True)
        out = bgcli.to_u8(tr.G.forward(bgcli.to_unit(fg), tok, None, 'bg')['image'])
        if i in segs:
            out[0][segs[i] == 0] = fg[0][segs[i] == 0]
            pasted += int((segs[i] == 0).sum())
        for kind, arr in (('inputs', fg), ('outputs', out), ('targets', bg)):
            png = np.array(Image.open(os.path.join(res, bg_name[:-4] + '_' + kind + '.png')))
            assert np.array_equal(png, arr[0]), (i, kind)
    assert pasted > 1000
