"""Scoring a held-out set during Foreground training: the kernel that scores two float images without their uint8 forms
(ssc_image_metrics_f32, hip.image_metrics_f32) and obj_colorization_main.py --val_freq on top of it.

The kernel is DEFINED by a composition: its five sums are the bits of image_metrics_u8(image_postprocess_u8(a),
image_postprocess_u8(b)).  So the kernel tests compare 64-bit patterns, and the oracle test takes its tolerances from
tests/test_gpu_image_metrics.py (the four integer rows exact, the SSIM mean to 1e-9: derived there).

The tile is 24 x 32 pixels with a 5-pixel halo: 10 x 10 has no window at all, 11 x 11 exactly one, 24 x 32 is one full tile,
25 x 33 four tiles of which three hold one row or column, 50 x 70 is 3 x 3 tiles with planar rows of 280 bytes (every second one
starts 8 bytes off the 16-byte boundary), 64 x 64 the small network's image.

The training tests run the command line in child processes (tests/train_validation_child.py pins what a run draws at random),
Pix2Pix and MRU at 64 x 64, batch 2, three records each in data/tfrecord/train and data/tfrecord/val: the last held-out batch
holds one record."""
import faulthandler
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import metrics_oracle as MO

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
SSIM_TOL = 1e-9                 # tests/test_gpu_image_metrics.py
EXACT = [0, 1, 2, 4]
SHAPES = [(10, 10), (11, 11), (24, 32), (25, 33), (50, 70), (64, 64)]
A_LAYOUTS = [(4, 0), (8, 3)]    # (lda, coff)
GUARD = 64                      # floats of NaN on both sides of every input (a multiple of 4: the views stay 16-byte aligned)


@pytest.fixture(autouse=True)
def _time_limit():
    """A test that hangs on the device ends the process (with every thread's traceback) instead of holding the card."""
    faulthandler.dump_traceback_later(400, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


# ---------------------------------------------------------------------------------------------------------------
# the kernel
# ---------------------------------------------------------------------------------------------------------------
def _sprinkle(rng, x):
    """-1, 1, +-1.5, NaN and +-inf at random places (about one value in 12)."""
    flat = x.reshape(-1)
    special = np.array([-1.0, 1.0, 1.5, -1.5, np.nan, np.inf, -np.inf], F)
    where = rng.choice(flat.size, max(7, flat.size // 12), replace=False)
    flat[where] = special[np.arange(where.size) % special.size]
    return x


def _uniform(rng, shape):
    return _sprinkle(rng, rng.uniform(-1.0, 1.0, shape).astype(F))


def _quantisation_points(rng, shape, sprinkle=True):
    """The points k / 255 * 2 - 1, k = 0..255, where (x + 1) / 2 * 255 steps to the next integer, and their neighbours in fp32
    on both sides: a different rounding of the three operations shows here.  All 768 of them when the shape holds as many."""
    k = np.arange(256, dtype=F)
    pts = k / F(255) * F(2) - F(1)
    pts = np.concatenate([pts, np.nextafter(pts, F(-2)), np.nextafter(pts, F(2))]).astype(F)
    n = int(np.prod(shape))
    x = np.resize(pts, n)
    rng.shuffle(x)
    x = x.reshape(shape)
    return _sprinkle(rng, x) if sprinkle else x


def _guarded(values):
    """A contiguous device tensor of ``values`` with GUARD floats of NaN in front of it and behind it."""
    raw = torch.full((values.size + 2 * GUARD,), float('nan'), dtype=torch.float32, device='cuda')
    t = raw[GUARD:GUARD + values.size].view(values.shape)
    t.copy_(torch.from_numpy(np.ascontiguousarray(values)))
    assert t.is_contiguous() and t.data_ptr() % 16 == 0
    return t, raw


def _nhwc(img, ld, coff):
    """img [N,H,W,3] in channels [coff, coff + 3) of rows of ld floats, 1.0e3 in the padding channels."""
    buf = np.full(img.shape[:3] + (ld,), 1.0e3, F)
    buf[..., coff:coff + 3] = img
    return _guarded(buf)


def _guards_intact(raw, n):
    g = raw.cpu().numpy()
    return np.isnan(g[:GUARD]).all() and np.isnan(g[GUARD + n:]).all()


def _bits(t):
    return t.cpu().numpy().view(np.int64)


@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: '%dx%d' % s)
def test_kernel_is_the_composed_route_bit_for_bit(shape):
    """N = 1 and 3, a in a 4-channel buffer at channel 0 and in an 8-channel buffer at channel 3, b NHWC (4 channels) and
    planar, uniform values and the quantisation points, both with the special values: the rows are the bits of the uint8 kernel
    on the two postprocessed images; a second call gives them again."""
    from sketchyscenecolorization_amd import hip
    h, w = shape
    for n in (1, 3):
        rng = np.random.RandomState(1000 * h + 10 * w + n)
        for make in (_uniform, _quantisation_points):
            a, b = make(rng, (n, h, w, 3)), make(rng, (n, h, w, 3))
            b4, b4_raw = _nhwc(b, 4, 0)
            bp, bp_raw = _guarded(np.transpose(b, (0, 3, 1, 2)))
            ub = hip.image_postprocess_u8(b4, 0)
            for lda, coff in A_LAYOUTS:
                ta, ta_raw = _nhwc(a, lda, coff)
                want = hip.image_metrics_u8(hip.image_postprocess_u8(ta, coff), ub)
                for tb, coff_b in ((b4, 0), (bp, None)):
                    what = (shape, n, make.__name__, lda, coff, 'planar' if coff_b is None else 'nhwc')
                    out = torch.full((n, 5), float('nan'), dtype=torch.float64, device='cuda')
                    got = hip.image_metrics_f32(ta, coff, tb, coff_b, out=out)
                    assert got is out and np.isfinite(out.cpu().numpy()).all(), what
                    assert np.array_equal(_bits(out), _bits(want)), (what, out.cpu().numpy(), want.cpu().numpy())
                    again = hip.image_metrics_f32(ta, coff, tb, coff_b)
                    assert np.array_equal(_bits(again), _bits(want)), what
                assert _guards_intact(ta_raw, ta.numel())
            assert _guards_intact(b4_raw, b4.numel()) and _guards_intact(bp_raw, bp.numel())
            rows = want.cpu().numpy()
            assert (rows[:, 2] == h * w).all()
            if h < 11 or w < 11:
                assert (rows[:, 3] == 0).all() and (rows[:, 4] == 0).all()
            else:
                assert (rows[:, 4] == (h - 10) * (w - 10)).all()


def test_kernel_with_bases_off_the_16_byte_boundary():
    """Both NHWC bases 4 bytes and the planar base 8 bytes into their allocations: every load goes float by float (NHWC) or
    meets other fronts and ends (planar), the bits are those of the aligned call."""
    from sketchyscenecolorization_amd import hip
    rng = np.random.RandomState(3)
    n, h, w = 2, 25, 33
    a, b = _uniform(rng, (n, h, w, 3)), _quantisation_points(rng, (n, h, w, 3))

    def shifted(t, floats):
        raw = torch.full((t.numel() + 8,), float('nan'), dtype=torch.float32, device='cuda')
        v = raw[floats:floats + t.numel()].view(t.shape)
        v.copy_(t)
        assert v.data_ptr() % 16 == 4 * floats
        return v

    ta, b8, bp = _nhwc(a, 8, 3)[0], _nhwc(b, 8, 5)[0], _guarded(np.transpose(b, (0, 3, 1, 2)))[0]
    want = hip.image_metrics_u8(hip.image_postprocess_u8(ta, 3), hip.image_postprocess_u8(b8, 5))
    for tb, coff_b in ((b8, 5), (bp, None)):
        assert np.array_equal(_bits(hip.image_metrics_f32(ta, 3, tb, coff_b)), _bits(want))
        sb = shifted(tb, 1 if coff_b is not None else 2)
        assert np.array_equal(_bits(hip.image_metrics_f32(shifted(ta, 1), 3, sb, coff_b)), _bits(want))


@pytest.mark.parametrize('shape', [(25, 33), (50, 70)], ids=lambda s: '%dx%d' % s)
def test_kernel_against_the_float64_oracle(shape):
    """The same arrays postprocessed on the host by main_procedure._postprocess (which has no clamp: the values stay inside
    [-1, 1] and finite here) and scored by tests/metrics_oracle.py, with the uint8 kernel's tolerances."""
    from sketchyscenecolorization_amd import hip, metrics as M
    from sketchyscenecolorization_amd.obj_lib.main_procedure import _postprocess
    h, w = shape
    rng = np.random.RandomState(7 * h + w)
    n = 3
    a = np.stack([rng.uniform(-1, 1, (h, w, 3)).astype(F), _quantisation_points(rng, (h, w, 3), sprinkle=False),
                  rng.uniform(-1, 1, (h, w, 3)).astype(F)])
    b = np.stack([rng.uniform(-1, 1, (h, w, 3)).astype(F), _quantisation_points(rng, (h, w, 3), sprinkle=False),
                  np.clip(a[2] + rng.uniform(-0.02, 0.02, (h, w, 3)).astype(F), -1, 1).astype(F)])     # a near pair: SSIM near 1
    a_nchw, b_nchw = np.ascontiguousarray(np.transpose(a, (0, 3, 1, 2))), np.ascontiguousarray(np.transpose(b, (0, 3, 1, 2)))
    want = MO.rows(_postprocess(a_nchw), _postprocess(b_nchw), M.ssim_window(), None)
    for lda, coff in A_LAYOUTS:
        for tb, coff_b in ((_nhwc(b, 4, 0)[0], 0), (_guarded(b_nchw)[0], None)):
            got = hip.image_metrics_f32(_nhwc(a, lda, coff)[0], coff, tb, coff_b).cpu().numpy()
            print('%dx%d lda %d coff %d %s: rows\n%r\noracle\n%r' % (h, w, lda, coff, 'planar' if coff_b is None else 'nhwc', got, want))
            assert np.isfinite(got).all()
            assert np.array_equal(got[:, EXACT], want[:, EXACT]), (got[:, EXACT], want[:, EXACT])
            for i in range(n):
                err = abs(got[i, 3] - want[i, 3]) / (3.0 * want[i, 4])
                print('image %d: ssim %.15f, error %.3e (bound %.0e)' % (i, want[i, 3] / (3.0 * want[i, 4]), err, SSIM_TOL))
                assert err <= SSIM_TOL, (i, err)
    assert want[2, 3] / (3 * want[2, 4]) > 0.9 > want[0, 3] / (3 * want[0, 4])


def test_kernel_refuses_bad_arguments_without_launching():
    from sketchyscenecolorization_amd import hip, metrics as M
    n, h, w = 3, 25, 33
    rng = np.random.RandomState(1)
    a4 = _nhwc(_uniform(rng, (n, h, w, 3)), 4, 0)[0]
    b4 = _nhwc(_uniform(rng, (n, h, w, 3)), 4, 0)[0]
    need = hip.image_metrics_workspace_bytes(n, h, w)
    assert need == n * 2 * 2 * 5 * 8
    win = torch.from_numpy(M.ssim_window()).cuda()
    ws = torch.zeros(need // 8, dtype=torch.float64, device='cuda')
    out = torch.full((n, 5), float('nan'), dtype=torch.float64, device='cuda')
    names = ('a', 'lda', 'coff_a', 'b', 'ldb', 'coff_b', 'planar', 'N', 'H', 'W', 'win', 'out', 'ws', 'ws_bytes')
    base = dict(a=hip.ptr(a4), lda=4, coff_a=0, b=hip.ptr(b4), ldb=4, coff_b=0, planar=0, N=n, H=h, W=w, win=hip.ptr(win),
                out=hip.ptr(out), ws=hip.ptr(ws), ws_bytes=need)
    call = lambda **kw: hip.lib().ssc_image_metrics_f32(*([kw.get(k, base[k]) for k in names] + [hip.stream_ptr()]))     # noqa: E731
    assert call(N=0) == -1 and call(N=-2) == -1 and call(H=0) == -1
    assert call(coff_a=2) == -1 and call(lda=8, coff_a=6) == -1 and call(coff_a=-1) == -1 and call(lda=2) == -1
    assert call(coff_b=2) == -1 and call(ldb=8, coff_b=6) == -1
    assert call(ws_bytes=need - 1) == -2 and call(ws_bytes=0) == -2 and call(ws=None) == -2
    assert call(a=None) == -1 and call(out=None) == -1
    torch.cuda.synchronize()
    assert np.isnan(out.cpu().numpy()).all() and not ws.cpu().numpy().any()
    # a planar b has no pitch and no offset: they are not looked at
    bp = torch.zeros((n, 3, h, w), device='cuda')
    assert call(b=hip.ptr(bp), planar=1, ldb=0, coff_b=99) == 0
    assert call() == 0
    torch.cuda.synchronize()
    want = hip.image_metrics_u8(hip.image_postprocess_u8(a4, 0), hip.image_postprocess_u8(b4, 0))
    assert np.array_equal(_bits(out), _bits(want))


# ---------------------------------------------------------------------------------------------------------------
# training, through the command line
# ---------------------------------------------------------------------------------------------------------------
def _write_records(base, mode, n, seed):
    from sketchyscenecolorization_amd import tfrecord as tf
    rng = np.random.RandomState(seed)
    d = os.path.join(base, 'data', 'tfrecord', mode)
    os.makedirs(d)
    cats = ['car', 'tree', 'car']
    recs = []
    for i in range(n):
        sk = np.full((384, 384, 3), 255, np.uint8)
        sk[60 * i + 40:60 * i + 46, 30:350] = 0
        sk[30:350, 100 * i + 50:100 * i + 54] = 0
        text = np.zeros(15, np.uint8)
        text[-3:] = [5, 7 + i, 9]
        img = np.clip(rng.randint(0, 256, (384, 384, 3)) // 2 + 60 * i, 0, 255).astype(np.uint8)
        recs.append(tf.make_example({'ImageName': ('%s%d.png' % (mode, i)).encode(), 'cartoon_data': img.tobytes(),
                                     'sketch_data': sk.tobytes(), 'Category': cats[i % 3].encode(), 'Category_id': 3 + 7 * i,
                                     'Color_text': b'the car is red', 'Text_vocab_indices': text.tobytes()}))
    tf.write_records(os.path.join(d, 'a.tfrecord'), recs[:1])
    tf.write_records(os.path.join(d, 'b.tfrecord'), recs[1:])
    return d


def _child(cwd, *flags):
    """obj_colorization_main.py --mode train -si 1 -bs 2 -mi 4 -smf 4 -swf 100 + flags in a fresh process -> (run directory,
    stdout, the caches it held, caches built)."""
    env = dict(os.environ, PYTHONPATH=ROOT)
    argv = ['--mode', 'train', '-si', '1', '-bs', '2', '-mi', '4', '-smf', '4', '-swf', '100'] + list(flags)
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'tests', 'train_validation_child.py')] + argv, cwd=cwd, env=env,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True, timeout=380)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    tail = [l for l in r.stdout.splitlines() if l.startswith('CHILD_CACHES ')][-1]
    caches, builds = tail[len('CHILD_CACHES '):].rsplit(' ', 1)
    runs = sorted(os.listdir(os.path.join(cwd, 'outputs')))
    assert len(runs) == 1, runs
    return os.path.join(cwd, 'outputs', runs[0]), r.stdout, json.loads(caches), int(builds)


def _workdir(tmp_path_factory, name, val=True):
    base = str(tmp_path_factory.mktemp(name))
    _write_records(base, 'train', 3, 11)
    if val:
        _write_records(base, 'val', 3, 12)
    return base


@pytest.fixture(scope='module', params=['Pix2Pix', 'MRU'])
def runs(request, tmp_path_factory):
    """The run with -vf 2 and the same command with -vf 0, each in a working directory of its own with the same records."""
    bt = request.param
    with_vf = _workdir(tmp_path_factory, bt + '-vf2')
    without = _workdir(tmp_path_factory, bt + '-vf0')
    return {'bt': bt, 'cwd': with_vf, 'vf2': _child(with_vf, '-bt', bt, '-vf', '2'), 'vf0': _child(without, '-bt', bt, '-vf', '0')}


def _lines(run):
    with open(os.path.join(run, 'log', 'validation.jsonl')) as f:
        return [json.loads(l) for l in f]


def test_run_writes_a_line_per_pass(runs):
    """(a) -vf 2 over four iterations: passes behind iterations 1 and 3 (the last one is also the last iteration: one pass),
    three images each, finite scores, the two categories; the run without the flag writes no such file."""
    run, out, caches, builds = runs['vf2']
    lines = _lines(run)
    assert [l['step'] for l in lines] == [1, 3] and all(l['images'] == 3 for l in lines), lines
    for l in lines:
        assert sorted(l['groups']) == ['car', 'tree'] and l['groups']['car']['n'] == 2 and l['all']['n'] == 3
        assert all(np.isfinite(l['all'][k]) for k in ('mae', 'psnr', 'ssim')) and l['seconds'] > 0
        assert 0 < l['all']['mae'] < 255 and -1 <= l['all']['ssim'] <= 1
    assert out.count('held-out pass at iteration') == 2 and 'held-out cache: 3 records' in out and 'metrics: n 3' in out
    # -rc off: the held-out cache is the only one, built once, with the sketches as bytes
    assert builds == 1 and len(caches) == 1 and caches[0]['records'] == 3 and caches[0]['size'] == 64
    assert caches[0]['dir'].endswith(os.path.join('tfrecord', 'val')) and caches[0]['sk'] and not caches[0]['skf']
    assert json.load(open(os.path.join(run, 'log', 'param_0.json')))['val_freq'] == 2
    scal = [json.loads(l) for l in open(os.path.join(run, 'log', 'scalars.jsonl'))]
    assert [s['step'] for s in scal] == [0]         # scalars.jsonl is what -swf 100 makes of it, nothing else
    run0, out0, caches0, builds0 = runs['vf0']
    assert not os.path.exists(os.path.join(run0, 'log', 'validation.jsonl')) and 'held-out' not in out0 and builds0 == 0


def test_passes_leave_the_training_trajectory_alone(runs):
    """(b) model_3.ckpt with and without the passes: the same tensors bit for bit, the optimizer's slots and step counts
    included."""
    a = torch.load(os.path.join(runs['vf2'][0], 'snapshot', 'model_3.ckpt-3'), map_location='cpu')
    b = torch.load(os.path.join(runs['vf0'][0], 'snapshot', 'model_3.ckpt-3'), map_location='cpu')
    assert list(a) == list(b) and any(k.startswith('__adam_v__/') for k in a) and len(a) > 20
    differ = [k for k in a if not torch.equal(a[k], b[k])]
    assert not differ, differ[:5]
    assert not torch.isnan(a['__adam_v__/generator']).any() and float(a['__adam_v__/generator'].abs().sum()) > 0


def test_the_last_line_is_the_score_of_the_snapshot(runs):
    """(c) model_3.ckpt in a fresh tower, ``generate`` over the same batches (2 + 1 records, cache order) with the same seeded
    noise, the outputs and targets postprocessed on the host and scored by the uint8 kernel: through metrics.summarise these
    rows give the numbers of the step-3 line exactly."""
    from sketchyscenecolorization_amd import hip, record_cache as rc, train_validation as TV
    from sketchyscenecolorization_amd.obj_lib import main_procedure as mp, models_collection as models
    run = runs['vf2'][0]
    line = _lines(run)[-1]
    assert line['step'] == 3
    models.reset_default_graph()
    try:
        tower = models.get_trainer(runs['bt'], 58, 64)
        tower.G.lstm_hybrid = True
        mp.restore_checkpoint(tower.store, os.path.join(run, 'snapshot', 'model_3.ckpt-3'))
        cache = rc.RecordCache(rc.list_record_files(os.path.join(runs['cwd'], 'data', 'tfrecord', 'val')), 64, device='cuda')
        numbers = torch.arange(3, dtype=torch.int32, device='cuda')
        labels = torch.from_numpy(cache.class_id).cuda()
        gen = torch.Generator(device='cuda')
        gen.manual_seed(TV.NOISE_SEED)
        rows = []
        plan = TV.batch_plan(len(cache), 2)
        assert plan == [(0, 2), (2, 3)]
        for a, b in plan:
            target, sketch = hip.decode_paired_cached_u8(cache, numbers[a:b], 64)
            noise_vec = TV.pass_noise(gen, b - a, 'cuda')
            out = tower.generate(sketch, cache.text[a:b], noise_vec, labels=labels[a:b])
            dev = lambda u8: torch.from_numpy(np.ascontiguousarray(u8)).cuda()      # noqa: E731
            rows.append(hip.image_metrics_u8(dev(mp._postprocess(out)), dev(mp._postprocess(target))).cpu().numpy())
        names, groups = TV.record_names(cache)
        assert names == ['car_val0', 'tree_val1', 'car_val2']
        mine, _ = TV.validation_line(3, names, groups, np.concatenate(rows, 0), line['seconds'])
        print('line of the run: %r\nindependent:     %r' % (line, mine))
        assert json.loads(json.dumps(mine, sort_keys=True)) == line
    finally:
        models.reset_default_graph()


def test_distance_maps_reach_the_held_out_pass(tmp_path_factory):
    """(d) -dm 1: the run finishes with its two lines, and the held-out cache holds distance maps in place of the sketches."""
    run, out, caches, builds = _child(_workdir(tmp_path_factory, 'dm'), '-bt', 'Pix2Pix', '-vf', '2', '-dm', '1')
    lines = _lines(run)
    assert [l['step'] for l in lines] == [1, 3] and all(l['images'] == 3 and np.isfinite(l['all']['ssim']) for l in lines)
    assert len(caches) == 1 and caches[0]['skf'] and not caches[0]['sk'] and 'distance maps included' in out
    assert os.path.exists(os.path.join(run, 'snapshot', 'model_3.ckpt-3'))


def test_both_caches_live_on_the_device_and_the_cap_holds(tmp_path_factory):
    """-rc device -vf 2 -vn 2: the training cache and the held-out cache side by side, each built once; the pass takes the first
    two held-out records."""
    run, out, caches, builds = _child(_workdir(tmp_path_factory, 'two-caches'), '-bt', 'Pix2Pix', '-vf', '2', '-vn', '2',
                                      '-rc', 'device')
    assert builds == 2 and sorted((os.path.basename(c['dir']), c['records']) for c in caches) == [('train', 3), ('val', 2)]
    assert all(c['device'].startswith('cuda') for c in caches)
    lines = _lines(run)
    assert [l['step'] for l in lines] == [1, 3] and all(l['images'] == 2 for l in lines)
    assert 'record cache: 3 records' in out and 'held-out cache: 2 records' in out


def test_without_the_directory_training_goes_on(tmp_path_factory):
    """-vf 2 without data/tfrecord/val: one line says so, the run trains to its end and writes no validation.jsonl."""
    run, out, caches, builds = _child(_workdir(tmp_path_factory, 'no-val', val=False), '-bt', 'Pix2Pix', '-vf', '2')
    assert out.count('data/tfrecord/val not found') == 1 and 'held-out' not in out
    assert not os.path.exists(os.path.join(run, 'log', 'validation.jsonl')) and builds == 0
    assert os.path.exists(os.path.join(run, 'snapshot', 'model_3.ckpt-3'))
    scal = [json.loads(l) for l in open(os.path.join(run, 'log', 'scalars.jsonl'))]
    assert [s['step'] for s in scal] == [0] and np.isfinite(scal[0]['total_loss/g'])
