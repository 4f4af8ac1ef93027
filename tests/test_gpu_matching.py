"""The instance matcher on the device against the float64 oracle tests/matching_oracle.py: the kernels of csrc/matching.hip one
by one (hip.match_preprocess_u8, hip.max_pool3s2, hip.space_to_batch, hip.batch_to_space, hip.squash_project, hip.match_finish,
hip.instance_occupancy), MatchModel's unit and head code at the released widths, whole small models, the command line, and one
pass at the released size.

Outputs sit inside buffers with a guard band on either side that must come back untouched.  Bounds:
  * moves, integer counts, the stroke map: exact;
  * one multiply-add: 2 * 2^-24 * (|a*x| + |b|); the upsampling: 4 * 2^-24 * max|corner| (three nested two-term mixes);
  * dot products: kernel_check.check_dot;
  * a whole model: 4 x the distance of the float32 oracle from the float64 one, recomputed here at run time."""
import faulthandler
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import matching_oracle as O
from conftest import parity_log
from kernel_check import U_FP32, check_dot, check_fp32

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, 'tests', 'golden', 'match')
GUARD = 64
CHILD_LIMIT = 180
HEAD_SMALL = dict(v_emb=24, w_emb=16, w_rnn=20, m_rnn=12)
SMALL = dict(units=(2, 1, 2, 2), filters=(8, 16, 32, 64, 128), **HEAD_SMALL)
SENTENCES = [('sun', 1), ('the bus on the left', 5),
             ('the two sheep on the right of the road , near the big tree , are light gray and dark brown', 15)]


@pytest.fixture(autouse=True)
def _time_limit():
    """A test that hangs on the device ends the process (with every thread's traceback) instead of holding the card."""
    faulthandler.dump_traceback_later(400, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


def hip():
    from sketchyscenecolorization_amd import hip as h
    return h


def M():
    from sketchyscenecolorization_amd import matching
    return matching


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


class Guarded(object):
    """An output of this shape in the middle of a buffer filled with a sentinel (NaN for floats)."""

    def __init__(self, shape, dtype=torch.float32):
        n = int(np.prod(shape))
        self.fill = float('nan') if dtype == torch.float32 else (0xA5 if dtype == torch.uint8 else -(1 << 40))
        self.raw = torch.full((n + 2 * GUARD,), self.fill, dtype=dtype, device='cuda')
        self.t = self.raw[GUARD:GUARD + n].view(*shape)

    def intact(self):
        g = torch.cat([self.raw[:GUARD], self.raw[-GUARD:]]).cpu()
        return bool(torch.isnan(g).all()) if self.fill != self.fill else bool((g == self.fill).all())

    def untouched(self):
        g = self.raw.cpu()
        return bool(torch.isnan(g).all()) if self.fill != self.fill else bool((g == self.fill).all())

    def get(self):
        assert self.intact(), 'the kernel wrote outside its output'
        return self.t.cpu().numpy()


def _vocab():
    return M().load_vocab(os.path.join(GOLD, 'vocab.txt'))


def _sketch(size, seed):
    """Strokes (0), grey strokes (128 and other bytes) and paper (255)."""
    rng = np.random.RandomState(seed)
    sk = np.full((size, size, 3), 255, np.uint8)
    sk[rng.rand(size, size) < 0.3] = 0
    grey = rng.rand(size, size) < 0.05
    sk[grey] = rng.randint(1, 255, (int(grey.sum()), 1)).astype(np.uint8)
    sk[0, :5] = [[0] * 3, [1] * 3, [254] * 3, [255] * 3, [128] * 3]
    return sk


# ------------------------------------------------------------------ preprocess
def test_preprocess():
    rng = np.random.RandomState(0)
    sk = rng.randint(0, 256, (32, 32, 3)).astype(np.uint8)
    sk[0, :4] = [[0, 1, 254], [1, 254, 255], [254, 255, 0], [255, 0, 1]]
    sk[5, 5] = [255, 0, 0]
    sk[5, 6] = [0, 255, 255]
    out, stroke = Guarded((1, 32, 32, 4)), Guarded((32, 32), torch.uint8)
    for _ in range(2):
        hip().match_preprocess_u8(_dev(sk), out=out.t, stroke=stroke.t)
    got = out.get()[0]
    ref = sk.astype(np.float32) - np.asarray(O.MU, dtype=np.float32)
    assert ref.dtype == np.float32
    err, ulp = np.abs(got[..., :3].astype(np.float64) - ref.astype(np.float64)), np.spacing(np.abs(ref)).astype(np.float64)
    print('preprocess: worst err / ulp %.3f' % float((err / ulp).max()))
    assert (err <= ulp).all()
    assert np.array_equal(got[..., 3], np.zeros((32, 32), np.float32))
    assert np.array_equal(stroke.get(), O.preprocess(sk)[1]) and stroke.get()[5, 5] == 0 and stroke.get()[5, 6] == 1
    x64, _ = O.preprocess(sk)
    assert np.abs(got[..., :3] - x64).max() < 2.0 ** -16         # float32(mu) is within 2^-18 of mu, the difference within 2^-17


# ------------------------------------------------------------------ space <-> batch
def _s2b(x, r):
    n, h, w, c = x.shape
    return np.ascontiguousarray(x.reshape(n, h // r, r, w // r, r, c).transpose(0, 2, 4, 1, 3, 5).reshape(n * r * r, h // r, w // r, c))


@pytest.mark.parametrize('C', [4, 36])
@pytest.mark.parametrize('r', [2, 4])
def test_space_to_batch_and_back(r, C):
    for n in (1, 2):
        for h, w in ((8, 8), (12, 8), (4, 4)):
            x = np.random.RandomState(h * w + n).randn(n, h, w, C).astype(np.float32)
            ref = _s2b(x, r)
            assert np.array_equal(ref[(n - 1) * r * r + 1 * r + 1], x[n - 1, 1::r, 1::r])       # sub-image (1, 1) of the last image
            out = Guarded(ref.shape)
            hip().space_to_batch(_dev(x), r, out=out.t)
            assert np.array_equal(out.get(), ref), (r, C, n, h, w)
            back = Guarded(x.shape)
            hip().batch_to_space(out.t, r, out=back.t)
            assert np.array_equal(back.get(), x), (r, C, n, h, w)
            back2 = Guarded(x.shape)
            hip().batch_to_space(_dev(ref), r, out=back2.t)
            assert np.array_equal(back2.get(), x)


def test_space_to_batch_refusals():
    from kernel_check import rc
    x, o = torch.zeros(1, 6, 8, 4, device='cuda'), Guarded((4, 3, 4, 4))
    assert rc('ssc_space_to_batch', x, 1, 6, 8, 4, 4, o.t) == -1            # 6 is no multiple of 4
    assert rc('ssc_space_to_batch', x, 1, 6, 8, 4, 3, o.t) == -1            # rate 3
    assert rc('ssc_batch_to_space', x, 1, 6, 8, 6, 2, o.t) == -1            # 6 channels
    assert rc('ssc_space_to_batch', x, 1, 6, 8, 4, 2, x) == -1              # in place
    assert o.untouched()


def test_regrouping_from_rate_2_to_rate_4(small_model_64):
    """What MatchModel does between group 4 and group 5: space_to_batch(2) on the rate-2 layout; every sub-image is one residue
    class mod 4 (y % 4 == 2*i2 + i1), and two batch_to_space(2) lead back."""
    m = small_model_64
    x = np.random.RandomState(3).randn(1, 8, 12, 8).astype(np.float32)
    a = m.cfg.net.regroup(m, _dev(x), 1, 2)
    assert np.array_equal(a.cpu().numpy(), _s2b(x, 2))
    b = m.cfg.net.regroup(m, a, 2, 4)
    got = b.cpu().numpy()
    assert np.array_equal(got, _s2b(_s2b(x, 2), 2))
    for i1 in range(2):
        for j1 in range(2):
            for i2 in range(2):
                for j2 in range(2):
                    assert np.array_equal(got[(i1 * 2 + j1) * 4 + i2 * 2 + j2], x[0, 2 * i2 + i1::4, 2 * j2 + j1::4])
    assert np.array_equal(m.cfg.net.ungroup(m, b, 4).cpu().numpy(), x)


# ------------------------------------------------------------------ max-pool
@pytest.mark.parametrize('with_ab', [False, True])
@pytest.mark.parametrize('C', [4, 64])
@pytest.mark.parametrize('size', [8, 10, 6, 7])
def test_max_pool(size, C, with_ab):
    rng = np.random.RandomState(size * C)
    x = (-1.0 - np.abs(rng.randn(2, size, size, C))).astype(np.float32)         # every maximum is negative: a padded tap read as 0 shows
    oh = (size + 1) // 2
    out = Guarded((2, oh, oh, C))
    if not with_ab:
        for _ in range(2):
            hip().max_pool3s2(_dev(x), None, out=out.t)
        assert np.array_equal(out.get(), O.max_pool(x))
        assert (out.get() < 0).all()
        return
    a = (rng.uniform(0.5, 1.5, C) * rng.choice([-1.0, 1.0], C)).astype(np.float32)
    b = rng.randn(C).astype(np.float32)
    hip().max_pool3s2(_dev(x), _dev(np.concatenate([a, b])), out=out.t)
    x64, a64, b64 = x.astype(np.float64), a.astype(np.float64), b.astype(np.float64)
    ref = O.max_pool(O.relu(a64 * x64 + b64))
    bound = O.max_pool(2 * U_FP32 * (np.abs(a64 * x64) + np.abs(b64)))         # |max f' - max f| <= max |f' - f| over the taps
    err = np.abs(out.get() - ref)
    print('max_pool size %d C %d: worst err / bound %.3f' % (size, C, float((err / bound).max())))
    assert (err <= bound).all()


# ------------------------------------------------------------------ squash + projection
@pytest.mark.parametrize('C', [12, 500])
def test_squash_project(C):
    """The constant 1 + 1e-3 is a float32 constant of the reference's graph (and of ssc_squash_fwd): the oracle takes it as that
    float32 value, so that what is left is the rounding of the logs, the products and the sum -- check_dot's (K + 8) * 2^-24 * S."""
    rows, ld = 64, -(-C // 32) * 32
    rng = np.random.RandomState(C)
    h = np.zeros((rows, ld), np.float32)
    h[:, :C] = np.tanh(rng.randn(rows, C) * 1.5)
    h[:, C:] = 0.75                                         # the padding is not read
    edge = np.array([1 - 2.0 ** -11, -(1 - 2.0 ** -11), 1 - 2.0 ** -14, 0.9995, -0.9995, 0.0, 1 - 2.0 ** -24], np.float32)
    h[:len(edge), 0] = edge
    h[1, :len(edge)] = edge
    assert (np.abs(h[:, :C]) < 1).all() and (1 - np.abs(h[:, :C]) < 1e-3).any()
    w = np.zeros(ld, np.float32)
    w[:C] = rng.randn(C)
    w[C:] = 7.0
    bias = np.array([0.3], np.float32)
    c = np.float64(np.float32(1.0 + 1e-3))
    hd = h[:, :C].astype(np.float64)
    sq = O.relu(0.5 * (np.log(c + hd) - np.log(c - hd)))
    ref = sq @ w[:C].astype(np.float64) + float(bias[0])
    S = np.abs(sq) @ np.abs(w[:C].astype(np.float64)) + abs(float(bias[0]))
    out = Guarded((rows,))
    for _ in range(2):
        hip().squash_project(_dev(h), _dev(w), _dev(bias), C=C, out=out.t)
    check_dot('squash_project', dict(rows=rows, C=C), torch.from_numpy(out.get()), torch.from_numpy(ref), torch.from_numpy(S), C)


# ------------------------------------------------------------------ finish
def _finish_case(h, S, seed):
    pred = np.random.RandomState(seed).randn(h, h).astype(np.float32)
    sk = _sketch(S, seed + 1)
    stroke = O.preprocess(sk)[1]
    up_ref, pr_ref = O.finish(pred.astype(np.float64), stroke, S)
    bound = 4 * U_FP32 * O.corner_max(pred.astype(np.float64), S)
    sure = np.abs(up_ref - 1e-9) > bound
    return pred, sk, stroke, up_ref, pr_ref, bound, sure


@pytest.mark.parametrize('h,S', [(8, 64), (12, 96)])
def test_finish(h, S):
    pred, sk, stroke, up_ref, pr_ref, bound, sure = _finish_case(h, S, 10 + h)
    assert (~sure).mean() <= 0.005                      # a condition on the seed, checked on the CPU
    assert (sk[:, :, 0] == 128).any() or ((sk[:, :, 0] > 1) & (sk[:, :, 0] < 254)).any()
    _, stroke_d = hip().match_preprocess_u8(_dev(sk))
    assert np.array_equal(stroke_d.cpu().numpy(), stroke)
    up, pr = Guarded((S, S)), Guarded((S, S), torch.uint8)
    for _ in range(2):
        hip().match_finish(_dev(pred), stroke_d, up=up.t, predicts=pr.t)
    err = np.abs(up.get() - up_ref)
    print('finish %d -> %d: worst err / bound %.3f, %d pixels left out' % (h, S, float((err / np.maximum(bound, 1e-300)).max()), int((~sure).sum())))
    assert (err <= bound).all()
    assert np.array_equal(pr.get()[sure], pr_ref[sure])
    grey = (sk[:, :, 0] != 0) & (sk[:, :, 0] != 255)
    assert grey.any() and (pr.get()[grey & sure & (up_ref >= 1e-9)] == 1).all()       # grey bytes are strokes
    # the >= and the stroke rule, exactly
    hip().match_finish(_dev(np.zeros((h, h), np.float32)), stroke_d, up=up.t, predicts=pr.t)
    assert not pr.get().any() and not up.get().any()
    hip().match_finish(_dev(np.full((h, h), 1e-9, np.float32)), stroke_d, up=up.t, predicts=pr.t)
    assert np.array_equal(pr.get(), stroke) and (up.get() == np.float32(1e-9)).all()
    hip().match_finish(_dev(np.full((h, h), np.nextafter(np.float32(1e-9), np.float32(0)), np.float32)), stroke_d, up=up.t, predicts=pr.t)
    assert not pr.get().any()


# ------------------------------------------------------------------ occupancy
def _selection(size):
    with np.load(os.path.join(GOLD, 'selection.npz')) as z:
        tag = 's%d/' % size
        n = int(z[tag + 'n'])
        return (z[tag + 'predicts'], z[tag + 'boxes'], [z[tag + 'mask_%d' % k] for k in range(n)], z[tag + 'matched'].tolist(),
                z[tag + 'scores'])


@pytest.mark.parametrize('size', [64, 96])
def test_occupancy_equals_the_recorded_selection(size):
    predicts, boxes, masks, matched, scores = _selection(size)
    p8 = predicts.astype(np.uint8)
    assert p8.max() == 128 and np.array_equal(p8 != 0, predicts != 0)
    buf, offsets = M().pack_masks(boxes, masks, size)
    out = Guarded((len(masks), 2), torch.int64)
    for _ in range(2):
        hip().instance_occupancy(_dev(p8), _dev(buf), _dev(boxes), _dev(offsets), out=out.t)
    assert np.array_equal(out.get(), O.occupancy(predicts, boxes, masks))
    got, got_scores = M().select_instances(out.get())
    assert got == matched and np.array_equal(got_scores, scores, equal_nan=True)
    assert np.array_equal(M().instance_counts(_dev(p8), boxes, masks), out.get())


def test_occupancy_refuses_what_leaves_its_buffers():
    predicts, boxes, masks, _, _ = _selection(64)
    buf, offsets = M().pack_masks(boxes, masks, 64)
    ref = O.occupancy(predicts, boxes, masks)
    bad = boxes.copy()
    bad[1] = [60, 60, 64, 63]           # leaves the image
    bad[2] = [5, 5, 4, 9]               # empty
    off = offsets.copy()
    off[3] = len(buf) - 3               # the mask leaves the buffer
    out = Guarded((len(masks), 2), torch.int64)
    hip().instance_occupancy(_dev(predicts.astype(np.uint8)), _dev(buf), _dev(bad), _dev(off), out=out.t)
    got = out.get()
    assert (got[[1, 2, 3]] == -1).all()
    keep = [k for k in range(len(masks)) if k not in (1, 2, 3)]
    assert np.array_equal(got[keep], ref[keep])


# ------------------------------------------------------------------ models
def _model(size, units, filters, head, seed):
    """(model, variables) with random weights."""
    m = M()
    cfg = m.MatchConfig(size=size, units=units, filters=filters, **head)
    v = m.random_variables(cfg, seed)
    model = m.MatchModel(cfg)
    model.load_dict(v)
    return model, v


BIAS = 'text_sketchyscene/m_lstm_output_projection/biases'


def _straddle(model, idx, n):
    """Set the final projection's bias to minus the median of the oracle's prediction without it, so that up straddles 0 for
    this sentence, and load the model again.  -> the variables."""
    cfg, v = model.cfg, model.test_vars
    v[BIAS][:] = 0
    pred = O.forward(model.test_sketch, v, idx, n, cfg.units, cfg.filters, cfg.max_len)[2]
    v[BIAS][:] = -np.median(pred)
    model.load_dict(v)
    return v


@pytest.fixture(scope='module')
def small_model_64():
    sk = _sketch(64, 64)
    model, v = _model(64, SMALL['units'], SMALL['filters'], HEAD_SMALL, 11)
    model.test_vars, model.test_sketch = v, sk
    yield model
    model.close()


@pytest.fixture(scope='module')
def small_model_96():
    sk = _sketch(96, 96)
    model, v = _model(96, SMALL['units'], SMALL['filters'], HEAD_SMALL, 12)
    model.test_vars, model.test_sketch = v, sk
    yield model
    model.close()


@pytest.fixture(scope='module')
def wide_model():
    """The released widths on a 64 x 64 image (an 8 x 8 map), one unit per group and a second one in group 5."""
    model, v = _model(64, (1, 1, 1, 2), (64, 256, 512, 1024, 2048), HEAD_SMALL, 13)
    model.test_vars = v
    yield model
    model.close()


def _unit_abs_sum(x, v, scope, stride, rate):
    """S of the unit's last contraction and its shortcut: |a3| (|relu(norm(block_2))| * |w3|) + |b3| + the shortcut's own sum."""
    y = O.relu(O.norm(O.conv(x, v[scope + '/block_1/conv/DW'], stride), v, scope + '/block_1/bn'))
    y = O.relu(O.norm(O.conv(y, v[scope + '/block_2/conv/DW'], 1, rate), v, scope + '/block_2/bn'))

    def absnorm(t, name):
        zero = dict(v)
        zero[name + '/mean'] = np.zeros_like(v[name + '/mean'])
        zero[name + '/beta'] = np.zeros_like(v[name + '/beta'])
        a = np.abs(O.norm(np.ones((1, 1, 1, v[name + '/gamma'].shape[0])), zero, name))
        b = np.abs(O.norm(np.zeros((1, 1, 1, v[name + '/gamma'].shape[0])), v, name))
        return a * t + b
    s = absnorm(O.conv(np.abs(y), np.abs(v[scope + '/block_3/conv/DW'])), scope + '/block_3/bn')
    if scope + '/block_add/conv/DW' in v:
        return s + absnorm(O.conv(np.abs(x), np.abs(v[scope + '/block_add/conv/DW']), stride), scope + '/block_add/bn')
    return s + np.abs(x)


@pytest.mark.parametrize('scope,cin,rate', [('ResNet/group_5_1', 2048, 4), ('ResNet/group_4_0', 512, 2)])
def test_unit_at_real_widths(wide_model, scope, cin, rate):
    """One bottleneck of the released widths through MatchModel.unit in the space-to-batch layout, against the oracle's direct
    dilated conv.  group_5_1: 2048 -> 512 -> 512 (rate 4) -> 2048 with the identity shortcut; group_4_0: 512 -> 256 -> 256 (rate 2)
    -> 1024 with the block_add conv.  Bound: check_dot's for the deepest contraction of the unit (K = 9 * cout / 4, or cin where
    that is deeper) over S of the last contraction plus the shortcut."""
    m = wide_model
    v = {k: a.astype(np.float64) for k, a in m.test_vars.items() if k.startswith(scope + '/')}
    x = np.abs(np.random.RandomState(rate).randn(1, 8, 8, cin)).astype(np.float32)          # what a unit reads went through a relu
    ref = O.unit(x.astype(np.float64), v, scope, 1, rate)
    S = _unit_abs_sum(x.astype(np.float64), v, scope, 1, rate)
    xd, cur = _dev(x), 1
    while cur < rate:
        xd = m.cfg.net.regroup(m, xd, cur, cur * 2).clone()
        cur *= 2
    assert tuple(xd.shape) == (rate * rate, 8 // rate, 8 // rate, cin)
    got = m.cfg.net.ungroup(m, m.cfg.net.unit(m, xd, scope, 1), rate)
    cout = ref.shape[3]
    K = max(9 * cout // 4, cin)
    assert (ref > 0).any() and (ref == 0).any()
    check_dot('match_unit', dict(scope=scope, rate=rate), got, torch.from_numpy(ref), torch.from_numpy(S), K)


def test_head_at_real_widths():
    """64 rows, 1000 / 1000 / 500 units padded to 1024 / 512, seven words.  Per element max(1e-5 * max|ref|, 4 x the float32 oracle's
    own distance from the float64 one): kernel_check.check_fp32, the rule for formulas that lose digits in float32 the same way
    in the reference (the logs of the squash near |h| = 1, the l2 norms)."""
    m = M()
    cfg = m.MatchConfig(size=64, units=(1, 1, 1, 1), filters=(8, 16, 32, 64, 128))
    v = m.random_variables(cfg, 21)
    model = m.MatchModel(cfg)
    model.load_dict(v)
    feat = np.abs(np.random.RandomState(5).randn(1, 8, 8, 128)).astype(np.float32)
    idx, n = m.preprocess_sentence('the bus on the left is yellow', _vocab(), 15)
    assert n == 7
    head = {k: a for k, a in v.items() if k.startswith('text_sketchyscene/')}
    ref64 = O.head(feat.astype(np.float64), {k: a.astype(np.float64) for k, a in head.items()}, idx, n, 15)
    ref32 = O.head(feat, head, idx, n, 15)
    assert ref32.dtype == np.float32
    tok = _dev(np.asarray(idx, np.int32))
    got = model.head(_dev(feat), tok, n).clone()
    again = model.head(_dev(feat), tok, n)
    assert torch.equal(got, again)
    check_fp32('match_head', dict(rows=64, seq_len=n), got, torch.from_numpy(ref64), torch.from_numpy(ref32.astype(np.float64)))
    model.close()


def _scene_for(predicts, size, seed):
    """Random boxes and masks whose oracle occupancy lies outside [0.45, 0.55], some matched and some not."""
    rng = np.random.RandomState(seed)
    boxes, masks = [], []
    for _ in range(60):
        y1, x1 = rng.randint(0, size - 8, 2)
        y2, x2 = min(size - 1, y1 + rng.randint(3, size // 2)), min(size - 1, x1 + rng.randint(3, size // 2))
        m = rng.rand(y2 - y1 + 1, x2 - x1 + 1) < 0.5
        if len(boxes) % 2:          # every other one follows the prediction, so that some are matched
            m = ((predicts[y1:y2 + 1, x1:x2 + 1] != 0) & (rng.rand(*m.shape) < 0.9)) | (rng.rand(*m.shape) < 0.05)
        m = m.astype(np.uint8)
        c = O.occupancy(predicts, [[y1, x1, y2, x2]], [m])[0]
        if c[1] > 0 and not 0.45 <= c[0] / c[1] <= 0.55:
            boxes.append([y1, x1, y2, x2])
            masks.append(m)
    return np.array(boxes, np.int32), masks


@pytest.mark.parametrize('which', [64, 96])
def test_whole_small_model(which, small_model_64, small_model_96):
    """up against the float64 oracle: the device may be 4 x as far from it as the float32 oracle is (relative to max|up|), a
    yardstick recomputed here; predicts wherever the oracle's up is further from the threshold than that; the matched instances of
    a scene whose occupancies the oracle puts outside [0.45, 0.55]."""
    model = small_model_64 if which == 64 else small_model_96
    cfg, sk = model.cfg, model.test_sketch
    vocab = _vocab()
    for text, want_len in SENTENCES:
        idx, n = M().preprocess_sentence(text, vocab, 15)
        assert n == want_len
        v = _straddle(model, idx, n)
        up64, pr64, _ = O.forward(sk, v, idx, n, cfg.units, cfg.filters, 15)
        up32, _, _ = O.forward(sk, v, idx, n, cfg.units, cfg.filters, 15, np.float32)
        assert up32.dtype == np.float32 and (up64 > 1e-9).any() and (up64 < 0).any()       # up straddles 0
        scale = np.abs(up64).max()
        yard = np.abs(up32.astype(np.float64) - up64).max()
        bound = 4 * yard
        sure = np.abs(up64 - 1e-9) > bound
        assert (~sure).mean() <= 0.005
        up, pr = model.forward(sk, idx, n)
        # inference keeps nothing for a backward pass: no buffer of the training passes (t_*, bt/*, bb/*) is allocated
        assert model._bufs and not [k for k in model._bufs if str(k[0]).startswith(('t_', 'bt/', 'bb/'))]
        up, pr = up.cpu().numpy().astype(np.float64), pr.cpu().numpy()
        err = np.abs(up - up64).max()
        print('whole model size %d seq_len %d: device %.3e, float32 oracle %.3e (relative to max|up| = %.3e: %.3e and %.3e), bound %.3e'
              % (which, n, err, yard, scale, err / scale, yard / scale, bound))
        parity_log('match_whole_model', dict(size=which, seq_len=n), err, bound, variant='kernel', cpu_fp32_vs_f64=yard, scale=scale)
        assert np.isfinite(up).all() and err <= bound
        assert np.array_equal(pr[sure], pr64[sure])
        boxes, masks = _scene_for(pr64, which, n)
        counts64 = O.occupancy(pr64, boxes, masks)
        want = O.select(counts64)[0]
        assert 0 < len(want) < len(masks)
        scene = {'sketch': sk, 'boxes': boxes, 'masks': masks, 'class_ids': np.zeros(len(masks), np.int32)}
        matched, scores, info = M().match_instances(model, scene, text, vocab)
        assert matched == want and info['seq_len'] == n and info['indices'] == idx
        assert np.array_equal(info['predicts'], pr)


def test_checkpoint_to_indices_through_the_command_line(tmp_path, small_model_64):
    """The small model written as a TensorFlow checkpoint under the reference's names, match_main.main in a fresh process on a
    scene directory: the printed line, match.json and the png are what match_instances gives in this process."""
    import scipy.io
    from PIL import Image
    from sketchyscenecolorization_amd import fg_scene, tf_checkpoint
    model = small_model_64
    cfg, sk = model.cfg, model.test_sketch
    text, vocab = SENTENCES[1][0], _vocab()
    idx, n = M().preprocess_sentence(text, vocab, 15)
    v = _straddle(model, idx, n)
    snap = tmp_path / 'snapshot'
    snap.mkdir()
    tf_checkpoint.write_checkpoint(str(snap / 'model-3'), v)
    (snap / 'checkpoint').write_text('model_checkpoint_path: "model-3"\n')
    pr64 = O.forward(sk, v, idx, n, cfg.units, cfg.filters, 15)[1]
    boxes, masks = _scene_for(pr64, 64, 7)
    boxes, masks = boxes[:12], masks[:12]
    d = tmp_path / 'scene'
    for sub in ('sketches', 'inner_masks', 'seg_data'):
        (d / sub).mkdir(parents=True)
    Image.fromarray(sk).save(str(d / 'sketches' / '42.png'))
    scipy.io.savemat(str(d / 'inner_masks' / '42.mat'), {'inner_masks': np.zeros((64, 64), np.uint8)})
    obj = np.empty(len(masks), dtype=object)
    for k, mk in enumerate(masks):
        obj[k] = mk
    np.savez(str(d / 'seg_data' / '42_datas.npz'), pred_masks=obj, pred_boxes=boxes, pred_class_ids=np.arange(len(masks)) + 7)
    scene = fg_scene.load_instances(str(d), '42', 64)
    matched, scores, info = M().match_instances(model, scene, text, vocab)
    assert 0 < len(matched) < len(masks)
    results = tmp_path / 'results'
    code = ('import json, sys; sys.path.insert(0, %r); import match_main; '
            'from sketchyscenecolorization_amd.matching import MatchConfig; '
            'match_main.main(sys.argv[2:], config=MatchConfig(**json.loads(sys.argv[1])))' % ROOT)
    small = dict(SMALL, size=64)
    run = subprocess.run([sys.executable, '-c', code, json.dumps(small), '--snapshot', str(snap), '--vocab_file', os.path.join(GOLD, 'vocab.txt'),
                          '--scene_dir', str(d), '--scene_size', '64', '--image_id', '42', '--instruction', text,
                          '--results_dir', str(results)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=CHILD_LIMIT, cwd=str(tmp_path))
    assert run.returncode == 0, run.stderr.decode()[-2000:]
    lines = [ln for ln in run.stdout.decode().splitlines() if ln.startswith('matched_inst_indices')]
    assert lines == ['matched_inst_indices ' + ','.join(str(k) for k in matched)]
    rec = json.load(open(str(results / '42' / 'match.json')))
    assert rec['matched_inst_indices'] == matched and rec['instruction'] == text and rec['seq_len'] == n
    assert rec['tokens'] == info['tokens'] and rec['class_ids'] == (np.arange(len(masks)) + 7).tolist()
    assert rec['occupancy'] == [float(s) for s in scores] and rec['snapshot'] == str(snap / 'model-3')
    png = np.array(Image.open(str(results / '42' / '42_match.png')))
    assert np.array_equal(png, info['predicts'] * 255)


def test_real_size_runs_and_repeats():
    """The released configuration (768 x 768, units 3 / 4 / 23 / 3, 2048 channels, 1000 / 1000 / 500) with random weights, one
    forward pass run twice: shapes, a finite up, the same bits both times.  No oracle here: the float64 network at 768 x 768 takes
    minutes on the CPU; the arithmetic is held by the tests above, through the same code at the same widths."""
    m = M()
    cfg = m.MatchConfig()
    model = m.MatchModel(cfg)
    model.init_random(1)
    sk = _sketch(768, 768)
    idx, n = m.preprocess_sentence('the bus on the left is yellow', _vocab(), 15)
    up, pr = model.forward(sk, idx, n)
    up1, pr1 = up.clone(), pr.clone()
    up, pr = model.forward(sk, idx, n)
    assert tuple(up.shape) == (768, 768) and up.dtype == torch.float32 and tuple(pr.shape) == (768, 768) and pr.dtype == torch.uint8
    assert bool(torch.isfinite(up).all())
    assert torch.equal(up, up1) and torch.equal(pr, pr1)
    stroke = torch.from_numpy(O.preprocess(sk)[1]).cuda()
    assert torch.equal(pr, ((up >= 1e-9) & (stroke != 0)).to(torch.uint8))
    model.close()
