"""Foreground training from a device record cache: the gather-decode kernel (ssc_decode_paired_cached_u8) and the min / max
pass that feeds it (ssc_decode_minmax_u8), record_cache.RecordCache, PairedQueue(record_cache=...) and
obj_colorization_main.py --record_cache device on top of them.

Every comparison is bit for bit: the kernel does the fp32 operations of the oracle's decode_paired_example one by one on the
bytes it gathers, and the operations of hip.decode_paired_u8 in its order."""
import faulthandler
import json
import os
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

F = np.float32
S = 5
IDX = [3, 0, 3, 4, 1, 1, 2]             # repeats, out of order
# (R, size): factor 2 / 6 (16-bit loads) / 1 and 3 (one element at a time); (48,24): 576 pixels an image, so the 256-thread
# workgroups straddle images
SHAPES = [(12, 6), (12, 2), (12, 12), (48, 24), (12, 4)]


@pytest.fixture(autouse=True)
def _time_limit():
    """A test that hangs on the device ends the process (with every thread's traceback) instead of holding the card."""
    faulthandler.dump_traceback_later(400, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def make_records(rng, s, r):
    """s records of r x r: image 1 has a narrow value range (the min / max normalisation matters), the sketches hold any
    byte (the block means are not just 0 and 255)."""
    img = rng.randint(0, 256, (s, r, r, 3)).astype(np.uint8)
    img[1] = rng.randint(40, 200, (r, r, 3))
    sk = rng.randint(0, 256, (s, r, r, 3)).astype(np.uint8)
    return img, sk


def as_cache(img, sk, size, skf=None, offset=0):
    """What hip.decode_paired_cached_u8 reads of a RecordCache.  offset: the uint8 arrays start that many bytes into their
    allocations (1: off the 2-byte alignment the 16-bit loads need)."""
    from sketchyscenecolorization_amd import hip

    def put(a):
        if a is None:
            return None
        raw = torch.empty(a.size + 8, dtype=torch.uint8, device='cuda')
        t = raw[offset:offset + a.size].view(a.shape)
        t.copy_(torch.from_numpy(a))
        return t

    c = types.SimpleNamespace(img=put(img), sk=put(sk), skf=skf, size=size)
    c.mnmx = hip.decode_minmax_u8(c.img, size)
    return c


def oracle_batch(img, sk, idx, size, noise, distance_map=False):
    from oracle import image_ops as I
    out = [I.decode_paired_example(img[s], sk[s], size, None if noise is None else noise[n], distance_map=distance_map)
           for n, s in enumerate(idx)]
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out])


def test_minmax_kernel_alone():
    """ssc_decode_minmax_u8 = the first launch of ssc_decode_paired_u8: per record, the extremes of the pixels (f*y, f*x)."""
    from sketchyscenecolorization_amd import hip
    img, _ = make_records(np.random.RandomState(1), S, 48)
    img[2, ::2, ::2] = np.clip(img[2, ::2, ::2], 17, 230)      # the extremes of the resized image are not those of the record
    img[2, 1, 1] = (0, 255, 0)
    for size in (48, 24, 8):
        f = 48 // size
        got = hip.decode_minmax_u8(dev(img), size).cpu().numpy()
        sub = img[:, ::f, ::f].reshape(S, -1).astype(F)
        assert got.dtype == F and np.array_equal(got, np.stack([sub.min(1), sub.max(1)], 1)), size
    assert tuple(hip.decode_minmax_u8(dev(img[:0]), 24).shape) == (0, 2)
    lib = hip.lib()
    out = torch.zeros((S, 2), device='cuda')
    assert lib.ssc_decode_minmax_u8(hip.ptr(dev(img)), S, 48, 7, hip.ptr(out), hip.stream_ptr()) == -1
    assert lib.ssc_decode_minmax_u8(hip.ptr(dev(img)), -1, 48, 24, hip.ptr(out), hip.stream_ptr()) == -1


@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: '%dto%d' % s)
def test_cached_decode_kernel(shape):
    """Against the oracle on the indexed records, and against hip.decode_paired_u8 on the gathered batch; then the variants
    on the same records: no noise, no sketch, caches off the 2-byte alignment."""
    from sketchyscenecolorization_amd import hip
    r, size = shape
    rng = np.random.RandomState(100 * r + size)
    img, sk = make_records(rng, S, r)
    noise = rng.uniform(0.0, 1.0 / 256, size=(len(IDX), size, size, 3)).astype(F)
    cache, idx = as_cache(img, sk, size), dev(np.array(IDX, np.int32))
    want_i, want_s = oracle_batch(img, sk, IDX, size, noise)
    gi, gs = hip.decode_paired_cached_u8(cache, idx, size, noise=dev(noise))
    assert gi.shape == gs.shape == (len(IDX), 3, size, size)
    assert np.array_equal(gi.cpu().numpy(), want_i) and np.array_equal(gs.cpu().numpy(), want_s)
    ui, us = hip.decode_paired_u8(dev(img[IDX]), dev(sk[IDX]), size, noise=dev(noise))
    assert torch.equal(gi, ui) and torch.equal(gs, us)
    # noise=None
    ni, ns = hip.decode_paired_cached_u8(cache, idx, size)
    want_n = oracle_batch(img, sk, IDX, size, None)
    assert np.array_equal(ni.cpu().numpy(), want_n[0]) and np.array_equal(ns.cpu().numpy(), want_n[1])
    # want_sketch=False: the image alone, into a caller's buffer; a sketch buffer handed in stays as it was
    sentinel = torch.full((len(IDX), 3, size, size), 7.5, device='cuda')
    buf = torch.empty((len(IDX), 3, size, size), device='cuda')
    oi, none = hip.decode_paired_cached_u8(cache, idx, size, noise=dev(noise), img_out=buf, want_sketch=False, sk_out=sentinel)
    assert none is None and oi is buf and torch.equal(oi, gi) and bool((sentinel == 7.5).all())
    # the same records one byte into their allocations: the element-wise kernel at every factor
    odd = as_cache(img, sk, size, offset=1)
    assert odd.img.data_ptr() % 2 == 1 and torch.equal(odd.mnmx, cache.mnmx)
    xi, xs = hip.decode_paired_cached_u8(odd, idx, size, noise=dev(noise))
    assert torch.equal(xi, gi) and torch.equal(xs, gs)


def test_cached_decode_kernel_real_shape():
    """384 -> 192, N = 3 of 4 records: 108 workgroups an image."""
    from sketchyscenecolorization_amd import hip
    rng = np.random.RandomState(384)
    img, sk = make_records(rng, 4, 384)
    pick = [2, 0, 1]
    noise = rng.uniform(0.0, 1.0 / 256, size=(3, 192, 192, 3)).astype(F)
    gi, gs = hip.decode_paired_cached_u8(as_cache(img, sk, 192), dev(np.array(pick, np.int32)), 192, noise=dev(noise))
    want_i, want_s = oracle_batch(img, sk, pick, 192, noise)
    assert np.array_equal(gi.cpu().numpy(), want_i) and np.array_equal(gs.cpu().numpy(), want_s)


def test_cached_decode_kernel_distance_maps():
    """skf_cache from hip.distance_map_u8, no sk_cache: the oracle's distance_map=True decode of the indexed records, at
    384 -> 192 with N = 2 of 3 records, and what hip.decode_paired_u8(distance_map=True) gives for the gathered batch."""
    from sketchyscenecolorization_amd import hip
    rng = np.random.RandomState(5)
    img, _ = make_records(rng, 3, 384)
    sk = np.full((3, 384, 384, 3), 255, np.uint8)
    sk[0, 100:104, 50:300] = 0
    pts = rng.randint(0, 384, (60, 2))
    sk[1, pts[:, 0], pts[:, 1], :] = 0
    sk[1, 20:24, 20:24, 1] = 100            # a stroke in one channel only
    sk[2, 200:330, 250:252] = 30
    pick = [2, 1]
    cache = as_cache(img, None, 192, skf=hip.distance_map_u8(dev(sk)))
    gi, gs = hip.decode_paired_cached_u8(cache, dev(np.array(pick, np.int32)), 192)
    want_i, want_s = oracle_batch(img, sk, pick, 192, None, distance_map=True)
    assert np.array_equal(gs.cpu().numpy(), want_s) and np.array_equal(gi.cpu().numpy(), want_i)
    ui, us = hip.decode_paired_u8(dev(img[pick]), dev(sk[pick]), 192, distance_map=True)
    assert torch.equal(gi, ui) and torch.equal(gs, us)
    # the float cache 4 bytes off the 8-byte alignment of the float2 loads
    raw = torch.empty(cache.skf.numel() + 2, device='cuda')
    cache.skf = raw[1:1 + cache.skf.numel()].view(cache.skf.shape).copy_(cache.skf)
    assert cache.skf.data_ptr() % 8 == 4
    xi, xs = hip.decode_paired_cached_u8(cache, dev(np.array(pick, np.int32)), 192)
    assert torch.equal(xi, gi) and torch.equal(xs, gs)


@pytest.mark.parametrize('shape', [(12, 6), (12, 4)], ids=lambda s: '%dto%d' % s)
def test_cached_decode_kernel_record_number_out_of_range(shape):
    """-1 and S beside valid numbers: those samples all NaN, the others exact, nothing read (the number is tested before an
    address is formed) and no error from the runtime."""
    from sketchyscenecolorization_amd import hip
    r, size = shape
    rng = np.random.RandomState(9)
    img, sk = make_records(rng, S, r)
    numbers = [2, -1, 4, S, 0]
    noise = rng.uniform(0.0, 1.0 / 256, size=(5, size, size, 3)).astype(F)
    gi, gs = hip.decode_paired_cached_u8(as_cache(img, sk, size), dev(np.array(numbers, np.int32)), size, noise=dev(noise))
    torch.cuda.synchronize()
    gi, gs = gi.cpu().numpy(), gs.cpu().numpy()
    good = [0, 2, 4]
    want_i, want_s = oracle_batch(img, sk, [numbers[n] for n in good], size, noise[good])
    assert np.array_equal(gi[good], want_i) and np.array_equal(gs[good], want_s)
    assert np.isnan(gi[[1, 3]]).all() and np.isnan(gs[[1, 3]]).all()


def test_cached_decode_kernel_refuses_bad_arguments():
    from sketchyscenecolorization_amd import hip
    img, sk = make_records(np.random.RandomState(2), 2, 12)
    c = as_cache(img, sk, 6)
    idx = torch.zeros(1, dtype=torch.int32, device='cuda')
    oi, os_ = torch.full((1, 3, 6, 6), 7.5, device='cuda'), torch.full((1, 3, 6, 6), 7.5, device='cuda')
    names = ('img', 'sk', 'skf', 'mnmx', 'S', 'idx', 'N', 'R', 'size', 'noise', 'oi', 'os')
    base = dict(img=hip.ptr(c.img), sk=hip.ptr(c.sk), skf=None, mnmx=hip.ptr(c.mnmx), S=2, idx=hip.ptr(idx), N=1, R=12, size=6,
                noise=None, oi=hip.ptr(oi), os=hip.ptr(os_))
    call = lambda **kw: hip.lib().ssc_decode_paired_cached_u8(*([kw.get(k, base[k]) for k in names] + [hip.stream_ptr()]))      # noqa: E731
    assert call(size=5) == -1 and call(N=-1) == -1 and call(S=0) == -1 and call(S=-3) == -1 and call(S=1 << 31) == -1
    assert call(size=0) == -1 and call(sk=None) == -2
    assert call(N=0) == 0
    torch.cuda.synchronize()
    assert bool((oi == 7.5).all()) and bool((os_ == 7.5).all())
    assert call() == 0 and call(sk=None, os=None) == 0
    torch.cuda.synchronize()
    assert not bool((oi == 7.5).any())


# ---------------------------------------------------------------------------------------------------------------
# the cache and the queue on records of the real size
# ---------------------------------------------------------------------------------------------------------------
def _write_records(base, n, seed):
    from sketchyscenecolorization_amd import tfrecord as tf
    rng = np.random.RandomState(seed)
    d = os.path.join(base, 'data', 'tfrecord', 'train')
    os.makedirs(d)
    recs = []
    for i in range(n):
        sk = np.full((384, 384, 3), 255, np.uint8)
        sk[50 * i:50 * i + 5, 30:350] = 0
        text = np.zeros(15, np.uint8)
        text[-2:] = [7 + i, 9]
        recs.append(tf.make_example({'ImageName': ('n%d.png' % i).encode(), 'cartoon_data': rng.randint(0, 256, (384, 384, 3)).astype(np.uint8).tobytes(),
                                     'sketch_data': sk.tobytes(), 'Category': b'car', 'Category_id': i,
                                     'Color_text': b'the car is red', 'Text_vocab_indices': text.tobytes()}))
    tf.write_records(os.path.join(d, 'a.tfrecord'), recs[:n // 2])
    tf.write_records(os.path.join(d, 'b.tfrecord'), recs[n // 2:])
    return os.path.join(base, 'data')


@pytest.fixture(scope='module')
def seven_records(tmp_path_factory):
    return _write_records(str(tmp_path_factory.mktemp('records')), 7, 5)


@pytest.mark.parametrize('distance_map', [False, True], ids=['sketch', 'distance-map'])
def test_cached_queue_is_the_device_decoding_queue(seven_records, distance_map):
    """Same seed: images and sketches torch.equal, class ids and captions equal, over 8 dequeues of 3 from 7 records (2 with
    the distance maps: each uncached dequeue runs the exhaustive transform).  The cached queue starts no thread and has
    no image staging ring, only the ring of record numbers."""
    from sketchyscenecolorization_amd import record_cache as rc
    from sketchyscenecolorization_amd.obj_lib.input_pipeline import PairedQueue
    files = rc.list_record_files(os.path.join(seven_records, 'tfrecord', 'train'))
    cache = rc.RecordCache(files, 192, distance_map=distance_map, device='cuda')
    assert len(cache) == 7 and cache.img.is_cuda and tuple(cache.mnmx.shape) == (7, 2) and cache.build_seconds > 0
    if distance_map:
        assert cache.sk is None and cache.skf.shape == (7, 384, 384, 3) and cache.nbytes == 7 * (5 * 384 * 384 * 3 + 8)
    else:
        assert cache.skf is None and cache.sk.shape == (7, 384, 384, 3) and cache.nbytes == 7 * (2 * 384 * 384 * 3 + 8)
    kw = dict(min_after_dequeue=2, data_base_dir=seven_records, seed=11, distance_map=distance_map)
    qc = PairedQueue('train', 3, record_cache=cache, **kw)
    qu = PairedQueue('train', 3, **kw)
    assert qu.device_decode and qu.cache is None
    for _ in range(2 if distance_map else 8):
        a, b = qc.dequeue(with_names=True), qu.dequeue(with_names=True)
        torch.cuda.synchronize()
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
        assert a[2].dtype == b[2].dtype and (a[2] == b[2]).all() and a[3].dtype == b[3].dtype and (a[3] == b[3]).all()
        assert a[4] == b[4] and a[5] == b[5]
    assert qc._thread is None and qc._q is None
    assert len(qc._ring) == qc._RING and all(s[0].dtype == torch.int32 and s[0].numel() == 3 for s in qc._ring)
    # queue 2's form: the same images, no sketches
    q2, q2u = PairedQueue('train', 3, record_cache=cache, want_sketch=False, **kw), PairedQueue('train', 3, **kw)
    a, b = q2.dequeue(), q2u.dequeue()
    assert a[1] is None and torch.equal(a[0], b[0]) and (a[2] == b[2]).all()


def test_cli_trains_from_the_record_cache_and_builds_it_once(tmp_path, monkeypatch, capsys):
    """-rc device from 6 records: three finite scalar lines and the cache line; a second train() in the same process (the
    path of a restart: resumed from the snapshot of iteration 2) finds the cache it built."""
    import obj_colorization_main as cli
    from sketchyscenecolorization_amd import record_cache as rc
    _write_records(str(tmp_path), 6, 0)
    monkeypatch.chdir(tmp_path)
    rc._MEMO.clear()
    n0 = rc.BUILDS
    argv = ['--mode', 'train', '-bt', 'Pix2Pix', '-si', '1', '-bs', '2', '-swf', '1', '-smf', '3', '-rc', 'device']
    cli.main(argv + ['-mi', '3'])
    text = capsys.readouterr().out
    assert 'record cache: 6 records, %d bytes' % (6 * (2 * 384 * 384 * 3 + 8)) in text, text[-2000:]
    stamp = sorted(os.listdir('outputs'))[0]
    run = os.path.join('outputs', stamp)
    scal = [json.loads(l) for l in open(os.path.join(run, 'log', 'scalars.jsonl'))]
    assert [s['step'] for s in scal] == [0, 1, 2] and all(np.isfinite(s['total_loss/g']) and np.isfinite(s['total_loss/d']) for s in scal)
    assert json.load(open(os.path.join(run, 'log', 'param_0.json')))['record_cache'] == 'device'
    assert rc.BUILDS == n0 + 1 and len(rc._MEMO) == 1
    cache = list(rc._MEMO.values())[0]
    assert len(cache) == 6 and cache.size == 64 and cache.img.is_cuda
    cli.main(argv + ['-mi', '4', '-rf', stamp])
    text = capsys.readouterr().out
    assert 'record cache: 6 records' in text and rc.BUILDS == n0 + 1 and list(rc._MEMO.values())[0] is cache
    scal = [json.loads(l) for l in open(os.path.join(run, 'log', 'scalars.jsonl'))]
    assert [s['step'] for s in scal] == [0, 1, 2, 3] and np.isfinite(scal[3]['total_loss/g'])
    rc._MEMO.clear()
