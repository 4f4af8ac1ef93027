"""ssc_image_metrics_u8 (csrc/metrics.hip) against the float64 oracle of tests/metrics_oracle.py: per image the sum of absolute
and of squared differences, the counted pixels, the SSIM sum over the counted 11 x 11 windows and their number.

The kernel's tile is 24 rows x 32 columns of pixels per workgroup (hip.METRICS_TILE); neither side exceeds 32, so 37 x 70 spans
2 x 3 tiles with a ragged last tile in both directions, and 13 x 17 has rows of 51 bytes: no multiple of 4 or 16, and every
row but the first starts off the 16-byte alignment the wide loads need.

Rows 0, 1, 2 and 4 are integers and must equal the oracle exactly.  Row 3 is compared after division by 3 * row 4, to 1e-9
absolute per image.  That bound is derived, not measured: a window's moments carry at most 22 roundings of 1.1e-16 on terms
<= 65025, that is <= 1.6e-10 absolute against denominators >= C2 = 58.5, about 3e-12 per window; a mean does not grow it; 1e-9
leaves about 300 x for another summation order and fused multiply-adds."""
import faulthandler

import numpy as np
import pytest
import torch

import metrics_oracle as MO

pytestmark = pytest.mark.gpu

SSIM_TOL = 1e-9
EXACT = [0, 1, 2, 4]


@pytest.fixture(autouse=True)
def _time_limit():
    """A test that hangs on the device ends the process (with every thread's traceback) instead of holding the card."""
    faulthandler.dump_traceback_later(400, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


def dev(a):
    return None if a is None else torch.from_numpy(np.array(a)).cuda()      # a copy: the cases are read-only


def _bytes(rng, shape):
    return rng.randint(0, 256, shape).astype(np.uint8)


def _near(rng, a, amp=2):
    """a with small noise: SSIM near 1, where the variances are differences of large, nearly equal terms."""
    return np.clip(a.astype(np.int32) + rng.randint(-amp, amp + 1, a.shape), 0, 255).astype(np.uint8)


def _cases():
    rng = np.random.RandomState(17)
    c = {}
    a = _bytes(rng, (2, 13, 17, 3))
    c['13x17'] = (a, np.stack([_bytes(rng, (13, 17, 3)), _near(rng, a[1])]), None)
    # three images of different content (random pair, near pair, a smooth ramp against noise): the rows must not mix
    a = _bytes(rng, (3, 37, 70, 3))
    ramp = (np.add.outer(np.arange(37) * 3, np.arange(70) * 2)[..., None] + np.array([0, 40, 90])).astype(np.uint8)
    a[2] = ramp
    b = np.stack([_bytes(rng, (37, 70, 3)), _near(rng, a[1]), _near(rng, ramp, 30)])
    c['37x70'] = (a, b, None)
    c['11x11'] = (_bytes(rng, (1, 11, 11, 3)), _bytes(rng, (1, 11, 11, 3)), None)
    c['10x40'] = (_bytes(rng, (1, 10, 40, 3)), _bytes(rng, (1, 10, 40, 3)), None)
    c['40x10'] = (_bytes(rng, (1, 40, 10, 3)), _bytes(rng, (1, 40, 10, 3)), None)
    m = ((rng.randint(0, 4, (3, 37, 70)) != 0) * rng.randint(1, 256, (3, 37, 70))).astype(np.uint8)
    m[1, 5:20, 30:60] = 0          # a hole wider than a window
    c['37x70-mask'] = (a, b, m)
    c['37x70-mask-zero'] = (a, b, np.zeros((3, 37, 70), np.uint8))
    c['37x70-mask-full'] = (a, b, rng.randint(1, 256, (3, 37, 70)).astype(np.uint8))
    return c


@pytest.fixture(scope='module')
def cases():
    """name -> (a, b, mask, oracle rows), computed once and read only."""
    from sketchyscenecolorization_amd import metrics as M
    win = M.ssim_window()
    out = {}
    for name, (a, b, m) in _cases().items():
        want = MO.rows(a, b, win, m)
        for t in (a, b, m, want):
            if t is not None:
                t.setflags(write=False)
        out[name] = (a, b, m, want)
    return out


def run(a, b, m=None):
    from sketchyscenecolorization_amd import hip
    got = hip.image_metrics_u8(dev(a), dev(b), dev(m))
    assert got.dtype == torch.float64 and tuple(got.shape) == (a.shape[0], 5) and got.is_cuda
    return got.cpu().numpy()


def assert_rows(got, want, what):
    print('%s: rows\n%r\noracle\n%r' % (what, got, want))
    assert np.isfinite(got).all(), what
    assert np.array_equal(got[:, EXACT], want[:, EXACT]), (what, got[:, EXACT], want[:, EXACT])
    for n in range(got.shape[0]):
        if want[n, 4] == 0:
            assert got[n, 3] == 0.0, (what, n, got[n, 3])
        else:
            err = abs(got[n, 3] - want[n, 3]) / (3.0 * want[n, 4])
            print('%s image %d: ssim %.15f, error %.3e (bound %.0e)' % (what, n, want[n, 3] / (3.0 * want[n, 4]), err, SSIM_TOL))
            assert err <= SSIM_TOL, (what, n, err)


@pytest.mark.parametrize('name', ['13x17', '37x70', '11x11', '10x40', '40x10', '37x70-mask', '37x70-mask-zero',
                                  '37x70-mask-full'])
def test_kernel_against_the_oracle(cases, name):
    a, b, m, want = cases[name]
    assert_rows(run(a, b, m), want, name)


def test_shapes_of_the_cases(cases):
    """What the cases are there for: window counts, no window at all, the per-image rows differ, SSIM near 1 is among them."""
    assert cases['13x17'][3][:, 4].tolist() == [3 * 7] * 2 and cases['11x11'][3][0, 4] == 1
    assert cases['37x70'][3][:, 4].tolist() == [27 * 60] * 3
    for name in ('10x40', '40x10'):
        want = cases[name][3]
        assert want[0, 3] == 0 and want[0, 4] == 0 and want[0, 2] == 400 and want[0, 0] > 0 and want[0, 1] > 0
    w = cases['37x70'][3]
    ssim = w[:, 3] / (3 * w[:, 4])
    assert ssim[0] < 0.1 and ssim[1] > 0.99 and len({tuple(r) for r in w}) == 3
    z = cases['37x70-mask-zero'][3]
    assert not z.any()
    wm = cases['37x70-mask'][3]
    assert (0 < wm[:, 4]).all() and (wm[:, 4] < 27 * 60).all() and (wm[:, 2] < 37 * 70).all()


def test_all_nonzero_mask_is_no_mask_bit_for_bit(cases):
    a, b, m, _ = cases['37x70-mask-full']
    assert np.array_equal(run(a, b, m).view(np.int64), run(a, b, None).view(np.int64))


def test_all_zero_mask_counts_nothing(cases):
    a, b, m, _ = cases['37x70-mask-zero']
    got = run(a, b, m)
    assert not np.isnan(got).any() and (got == 0).all()


def test_an_image_against_itself(cases):
    """a is b: no difference at all, and every window's SSIM is 1 up to the rounding of its moments."""
    from sketchyscenecolorization_amd import hip, metrics as M
    a = cases['37x70'][0]
    t = dev(a)
    got = hip.image_metrics_u8(t, t).cpu().numpy()
    assert (got[:, 0] == 0).all() and (got[:, 1] == 0).all() and (got[:, 2] == 37 * 70).all()
    assert_rows(got, MO.rows(a, a, M.ssim_window()), 'a is b')
    assert (np.abs(got[:, 3] / (3 * got[:, 4]) - 1.0) <= SSIM_TOL).all()


@pytest.mark.parametrize('shape', [(2, 13, 17), (1, 37, 70)])
def test_extremes(shape):
    """All 0 against all 255: the largest sums a pixel can give, exactly."""
    from sketchyscenecolorization_amd import metrics as M
    n, h, w = shape
    a, b = np.zeros((n, h, w, 3), np.uint8), np.full((n, h, w, 3), 255, np.uint8)
    got = run(a, b)
    assert (got[:, 0] == 255 * 3 * h * w).all() and (got[:, 1] == 255 ** 2 * 3 * h * w).all() and (got[:, 2] == h * w).all()
    assert_rows(got, MO.rows(a, b, M.ssim_window()), 'extremes')
    assert np.array_equal(run(b, a)[:, EXACT], got[:, EXACT])


def test_bases_off_the_16_byte_alignment(cases):
    """The images start 1 and 7 bytes into their allocations, the mask 3: the result is that of aligned copies, bit for bit."""
    from sketchyscenecolorization_amd import hip
    a, b, m, want = cases['37x70-mask']

    def put(x, offset):
        raw = torch.zeros(x.size + 32, dtype=torch.uint8, device='cuda')
        t = raw[offset:offset + x.size].view(x.shape)
        t.copy_(torch.from_numpy(np.array(x)))
        assert t.data_ptr() % 16 == offset and t.is_contiguous()
        return t

    got = hip.image_metrics_u8(put(a, 1), put(b, 7), put(m, 3)).cpu().numpy()
    assert_rows(got, want, 'unaligned bases')
    assert np.array_equal(got.view(np.int64), run(a, b, m).view(np.int64))


def test_two_calls_give_the_same_bits(cases):
    for name in ('37x70', '37x70-mask', '13x17'):
        a, b, m, _ = cases[name]
        first = run(a, b, m)
        for _ in range(3):
            assert np.array_equal(run(a, b, m).view(np.int64), first.view(np.int64)), name


def test_the_out_argument_is_filled_in_place(cases):
    from sketchyscenecolorization_amd import hip
    a, b, m, want = cases['13x17']
    out = torch.full((2, 5), -7.0, dtype=torch.float64, device='cuda')
    assert hip.image_metrics_u8(dev(a), dev(b), out=out) is out
    assert_rows(out.cpu().numpy(), want, 'out=')


def test_workspace_too_small_is_refused_and_out_stays_unwritten(cases):
    """One byte short of N * tiles * 5 doubles: a non-zero return code, nothing launched -- never a partial sum."""
    from sketchyscenecolorization_amd import hip, metrics as M
    a, b, _, want = cases['37x70']
    need = hip.image_metrics_workspace_bytes(3, 37, 70)
    assert need == 3 * 2 * 3 * 5 * 8
    ta, tb, win = dev(a), dev(b), dev(M.ssim_window())
    ws = torch.zeros(need // 8, dtype=torch.float64, device='cuda')
    out = torch.full((3, 5), -7.0, dtype=torch.float64, device='cuda')
    call = lambda nbytes: hip.lib().ssc_image_metrics_u8(hip.ptr(ta), hip.ptr(tb), None, 3, 37, 70, hip.ptr(win), hip.ptr(out),     # noqa: E731
                                                         hip.ptr(ws), nbytes, hip.stream_ptr())
    for nbytes in (need - 1, 8, 0):
        assert call(nbytes) != 0
        torch.cuda.synchronize()
        assert (out.cpu().numpy() == -7.0).all() and not ws.cpu().numpy().any()
    assert hip.lib().ssc_image_metrics_u8(hip.ptr(ta), hip.ptr(tb), None, 3, 0, 70, hip.ptr(win), hip.ptr(out), hip.ptr(ws), need,
                                          hip.stream_ptr()) != 0
    assert call(need) == 0
    assert_rows(out.cpu().numpy(), want, 'exact workspace')
