"""The matcher's SegNet backbone on the device against the float64 oracle tests/segnet_oracle.py: the two kernels of
csrc/match_segnet.hip (hip.max_pool2_argmax, hip.unpool2) one by one, whole small models, one stage at the released widths, the
pass in two halves and head training on cached features, the command line in fresh processes, and one pass at the released size.

Bounds:
  * the pool's values: the max over the window's taps of 2 * 2^-24 * (|a*x| + |b|), the bound of tests/test_gpu_matching.py::
    test_max_pool (one multiply-add per tap; |max f' - max f| <= max |f' - f|); without ab the pool moves floats: exact;
  * a code: wherever the window's float64 margin (largest minus second-largest tap) exceeds twice that bound and its maximum is
    above it -- two taps that are further apart than both their errors cannot change places;
  * the unpool moves floats: exact, bit for bit;
  * a whole model: the device's codes must be the float64 oracle's in every sure window (margin more than 4 x the float32
    oracle's distance from the float64 one among the window's taps); then, on the device's codes, up within 4 x the float32
    oracle's distance from the float64 one -- the yardstick of test_whole_small_model."""
import faulthandler
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import match_eval_oracle as EO
import matching_oracle as O
import segnet_oracle as SO
from conftest import parity_log
from kernel_check import U_FP32, rc
from test_gpu_matching import GOLD, Guarded, SENTENCES, _dev, _scene_for, _sketch, _vocab

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VOCAB = os.path.join(GOLD, 'vocab.txt')
CHILD_LIMIT = 180
HEAD_SMALL = dict(v_emb=24, w_emb=16, w_rnn=20, m_rnn=12)       # the small head of tests/test_gpu_matching.py
FILTERS = (8, 16, 32, 32, 32)
SHAPES = [(1, 2, 2, 4), (2, 6, 10, 12), (1, 8, 8, 512), (1, 64, 64, 8)]
BIAS = 'text_sketchyscene/m_lstm_output_projection/biases'
# The seeds of the small models' weights, chosen on the CPU: with them the float32 oracle alone leaves no window of any pool
# unsure against the float64 one (seeds 11 and 17 leave one each), so the 0.5 % the device is allowed is all the device's.
SEEDS = {64: 12, 96: 13}


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


# ------------------------------------------------------------------ the pool kernel
def _pool_input(shape, seed):
    """Floats of both signs with planted exact ties: a four-way one, one between the last two taps, one between taps 1 and 2 below
    which tap 0 lies, and a window whose every tap is negative."""
    n, h, w, c = shape
    rng = np.random.RandomState(seed)
    x = rng.randn(*shape).astype(np.float32)
    x[0, 0:2, 0:2, 0] = 0.75
    x[0, 0:2, 0:2, 1] = [[-0.5, -0.25], [1.5, 1.5]]
    x[0, 0:2, 0:2, 2] = [[0.125, 2.0], [2.0, -3.0]]
    x[0, 0:2, 0:2, 3] = [[-1.0, -2.0], [-0.5, -4.0]]
    if h > 2:
        x[n - 1, h - 2:, w - 2:, c - 1] = 0.3125        # the last window of the last image, the last channel
    return x


def _tie_codes(shape):
    n, h, w, c = shape
    want = {(0, 0, 0, 0): 0, (0, 0, 0, 1): 2, (0, 0, 0, 2): 1, (0, 0, 0, 3): 2}
    if h > 2:
        want[(n - 1, h // 2 - 1, w // 2 - 1, c - 1)] = 0
    return want


@pytest.mark.parametrize('shape', SHAPES)
def test_pool_without_ab_is_exact(shape):
    """No arithmetic: the values and every code are the oracle's on the same float32 taps, ties included."""
    n, h, w, c = shape
    x = _pool_input(shape, sum(shape))
    ref, ind, code_ref, _margin = SO.max_pool_with_argmax(x)
    out, code = Guarded((n, h // 2, w // 2, c)), Guarded((n, h // 2, w // 2, c), torch.uint8)
    hip().max_pool2_argmax(_dev(x), None, out=out.t, code=code.t)
    first = out.get().copy(), code.get().copy()
    hip().max_pool2_argmax(_dev(x), None, out=out.t, code=code.t)
    assert np.array_equal(out.get(), first[0]) and np.array_equal(code.get(), first[1])        # two runs, the same bits
    assert np.array_equal(out.get(), ref) and (out.get() < 0).any()
    assert np.array_equal(code.get(), code_ref) and code.get().max() <= 3
    for at, k in _tie_codes(shape).items():
        assert code.get()[at] == k, at
    assert np.array_equal(x.reshape(n, -1)[np.arange(n)[:, None], ind.reshape(n, -1)].reshape(ref.shape), out.get())     # TF's flat index


@pytest.mark.parametrize('shape', SHAPES)
def test_pool_with_ab(shape):
    n, h, w, c = shape
    rng = np.random.RandomState(sum(shape) + 1)
    x = _pool_input(shape, sum(shape))
    a = (rng.uniform(0.5, 1.5, c) * rng.choice([-1.0, 1.0], c)).astype(np.float32)
    a[:4] = [1.25, 0.5, 1.0, 0.75]                          # the channels of the planted ties keep their order
    if c > 4:
        a[4] = -1.0
    b = (rng.randn(c) * 0.5).astype(np.float32)
    b[:4] = [0.25, -0.125, 0.5, 0.25]
    assert (a < 0).any() or c == 4
    x64, a64, b64 = x.astype(np.float64), a.astype(np.float64), b.astype(np.float64)
    f = O.relu(a64 * x64 + b64)
    ref, _ind, code_ref, margin = SO.max_pool_with_argmax(f)
    bound = SO.window_taps(2 * U_FP32 * (np.abs(a64 * x64) + np.abs(b64))).max(axis=0)
    out, code = Guarded((n, h // 2, w // 2, c)), Guarded((n, h // 2, w // 2, c), torch.uint8)
    hip().max_pool2_argmax(_dev(x), _dev(np.concatenate([a, b])), out=out.t, code=code.t)
    first = out.get().copy(), code.get().copy()
    hip().max_pool2_argmax(_dev(x), _dev(np.concatenate([a, b])), out=out.t, code=code.t)
    assert np.array_equal(out.get(), first[0]) and np.array_equal(code.get(), first[1])
    err = np.abs(out.get() - ref)
    checked = (margin > 2 * bound) & (ref > bound)
    print('max_pool2_argmax %s: worst err / bound %.3f, %d of %d codes checked' % (shape, float((err / bound).max()), int(checked.sum()),
                                                                              checked.size))
    parity_log('max_pool2_argmax', dict(shape=list(shape)), float((err / bound).max()), 1.0, variant='kernel')
    assert (err <= bound).all() and (out.get() >= 0).all() and code.get().max() <= 3
    assert np.array_equal(code.get()[checked], code_ref[checked]) and (h == 2 or checked.mean() > 0.5)
    dead = SO.window_taps(a64 * x64 + b64).max(axis=0) < -bound             # every tap <= 0: the value is 0, the code is not checked
    assert dead[0, 0, 0, 3] and (out.get()[dead] == 0).all()
    # the planted ties are exact in float32 too (the same a, b on equal taps): the first tap in row-major order wins.  Channel 3's
    # window is the dead one; the four-way tie of the last window gives code 0 whatever its channel's a
    for at, k in _tie_codes(shape).items():
        if at != (0, 0, 0, 3):
            assert code.get()[at] == k and margin[at] == 0, at


def test_pool_and_unpool_refusals():
    x = torch.zeros(1, 6, 8, 8, device='cuda')
    out, code = Guarded((1, 3, 4, 8)), Guarded((1, 3, 4, 8), torch.uint8)
    assert rc('ssc_max_pool2_argmax', x, None, 1, 5, 8, 8, out.t, code.t) == -1         # odd H
    assert rc('ssc_max_pool2_argmax', x, None, 1, 6, 7, 8, out.t, code.t) == -1         # odd W
    assert rc('ssc_max_pool2_argmax', x, None, 1, 6, 8, 6, out.t, code.t) == -1         # C % 4
    assert rc('ssc_max_pool2_argmax', x, None, 0, 6, 8, 8, out.t, code.t) == -1
    assert rc('ssc_max_pool2_argmax', x, None, 1, 6, 8, 8, out.t, None) == -1
    assert rc('ssc_max_pool2_argmax', x, None, 1, 6, 8, 8, x, code.t) == -1             # in place
    assert rc('ssc_max_pool2_argmax', x, None, 1, 6, 8, 8, out.raw[1:], code.t) == -3   # off a 16-byte boundary
    assert rc('ssc_max_pool2_argmax', x, None, 1, 6, 8, 8, out.t, code.raw[1:]) == -3   # the codes off a 4-byte one
    assert out.untouched() and code.untouched()
    big = Guarded((1, 12, 16, 8))
    c8 = torch.zeros(1, 6, 8, 8, dtype=torch.uint8, device='cuda')
    assert rc('ssc_unpool2', x, c8, 1, 6, 8, 6, big.t) == -1
    assert rc('ssc_unpool2', x, c8, 1, 0, 8, 8, big.t) == -1
    assert rc('ssc_unpool2', x, None, 1, 6, 8, 8, big.t) == -1
    assert rc('ssc_unpool2', x, c8, 1, 6, 8, 8, x) == -1
    assert rc('ssc_unpool2', x, c8, 1, 6, 8, 8, big.raw[1:]) == -3
    assert big.untouched()
    assert rc('ssc_max_pool2_argmax', x, None, 1, 6, 8, 8, out.t, code.t) == 0 and rc('ssc_unpool2', x, c8, 1, 6, 8, 8, big.t) == 0
    with pytest.raises(AssertionError):
        hip().max_pool2_argmax(torch.zeros(1, 5, 8, 8, device='cuda'))
    with pytest.raises(AssertionError):
        hip().unpool2(x, c8.to(torch.int32))


# ------------------------------------------------------------------ the unpool kernel
def _unpool_ref(x, code):
    n, h, w, c = x.shape
    out = np.zeros((n, 2 * h, 2 * w, c), x.dtype)
    k = code & 3
    for dy in (0, 1):
        for dx in (0, 1):
            out[:, dy::2, dx::2] = np.where(k == 2 * dy + dx, x, 0)
    return out


@pytest.mark.parametrize('shape', SHAPES)
def test_unpool_is_exact(shape):
    """Against NumPy bit for bit, in a buffer filled with NaN beforehand (every element is written); a code above 3 counts as its
    low two bits; and against the oracle's scatter_nd by TF's flat index."""
    n, H, W, c = shape
    h, w = H // 2, W // 2
    rng = np.random.RandomState(sum(shape))
    x = rng.randn(n, h, w, c).astype(np.float32)
    x[0, 0, 0, 0] = 0.0
    code = rng.randint(0, 4, (n, h, w, c)).astype(np.uint8)
    out = Guarded(shape)
    assert bool(torch.isnan(out.t).all())
    hip().unpool2(_dev(x), _dev(code), out=out.t)
    got = out.get()
    assert not np.isnan(got).any() and np.array_equal(got.view(np.uint32), _unpool_ref(x, code).view(np.uint32))
    assert np.array_equal(got, SO.unpool_2d(x, SO.flat_index(code, W), (H, W)))
    assert (SO.window_taps(got != 0).sum(axis=0) <= 1).all()
    high = (code | (rng.randint(0, 64, code.shape) << 2)).astype(np.uint8)
    assert high.max() > 3
    again = Guarded(shape)
    hip().unpool2(_dev(x), _dev(high), out=again.t)
    assert np.array_equal(again.get().view(np.uint32), got.view(np.uint32))
    # the unpool of the pool keeps the windows' maxima where they were
    y = _pool_input(shape, 3)
    pooled, codes = hip().max_pool2_argmax(_dev(y))
    back = hip().unpool2(pooled, codes).cpu().numpy()
    assert np.array_equal(back[back != 0], y[back != 0]) and np.array_equal(SO.window_taps(back).sum(axis=0), pooled.cpu().numpy())


# ------------------------------------------------------------------ whole small models
def _segnet_model(size, seed, filters=FILTERS, **more):
    m = M()
    cfg = m.MatchConfig(size=size, filters=filters, backbone='segnet', **dict(HEAD_SMALL, **more))
    v = m.random_variables(cfg, seed)
    model = m.MatchModel(cfg)
    model.load_dict(v)
    return model, v


@pytest.fixture(scope='module')
def small_segnets():
    made = {}
    for size, seed in SEEDS.items():
        model, v = _segnet_model(size, seed)
        model.test_vars, model.test_sketch = v, _sketch(size, size)
        made[size] = model
    yield made
    for model in made.values():
        model.close()


@pytest.fixture(scope='module')
def small_references(small_segnets):
    """Per size, computed once and left unchanged: the records of the float64 and the float32 oracle's own passes (they do not
    depend on the sentence) and which windows are sure."""
    out = {}
    for size, model in small_segnets.items():
        r64, r32 = {}, {}
        idx, n = M().preprocess_sentence(SENTENCES[0][0], _vocab(), 15)
        SO.forward(model.test_sketch, model.test_vars, idx, n, FILTERS, 15, record=r64)
        SO.forward(model.test_sketch, model.test_vars, idx, n, FILTERS, 15, np.float32, record=r32)
        out[size] = dict(r64=r64, sure=SO.sure_windows(r64, r32))
    return out


@pytest.mark.parametrize('which', [64, 96])
def test_whole_small_model(which, small_segnets, small_references):
    model, ref = small_segnets[which], small_references[which]
    cfg, sk, v = model.cfg, model.test_sketch, model.test_vars
    vocab = _vocab()
    alone = SO.unsure_share(ref['sure'])
    assert alone <= 0.005                       # the condition on the seed, checked on the CPU
    # the device's codes: the float64 oracle's in every sure window
    model.features(sk)
    codes = {k[0][len('sn/code/'):]: b.cpu().numpy() for k, b in model._bufs.items() if str(k[0]).startswith('sn/code/')}
    assert sorted(codes) == ['enc_1', 'enc_2', 'enc_3', 'enc_4', 'enc_5']
    other = 0
    for stage, (sure, positive) in ref['sure'].items():
        r = ref['r64'][stage]
        assert codes[stage].shape == r['code'].shape and codes[stage].max() <= 3
        wrong = (codes[stage] != r['code']) & sure & positive
        other += int(((codes[stage] != r['code']) & positive).sum())
        print('segnet size %d %s: %d windows, %d positive, %d of them unsure, %d sure ones with another code'
              % (which, stage, sure.size, int(positive.sum()), int((positive & ~sure).sum()), int(wrong.sum())))
        assert not wrong.any(), stage
    print('segnet size %d: unsure share of the oracles alone %.5f; %d positive windows with a code other than the float64 oracle\'s'
          % (which, alone, other))
    for text, want_len in SENTENCES[1:]:                    # two sentence lengths: 5 and 15
        idx, n = M().preprocess_sentence(text, vocab, 15)
        assert n == want_len
        v[BIAS][:] = 0
        v[BIAS][:] = -np.median(SO.forward(sk, v, idx, n, FILTERS, 15, codes=codes)[2])        # up straddles 0 for this sentence
        model.load_dict(v)
        up64, pr64, _p, _f = SO.forward(sk, v, idx, n, FILTERS, 15, codes=codes)
        up32 = SO.forward(sk, v, idx, n, FILTERS, 15, np.float32, codes=codes)[0]
        assert up32.dtype == np.float32 and (up64 > 1e-9).any() and (up64 < 0).any()
        scale = np.abs(up64).max()
        yard = np.abs(up32.astype(np.float64) - up64).max()
        bound = 4 * yard
        sure = np.abs(up64 - 1e-9) > bound
        assert (~sure).mean() <= 0.005
        up, pr = model.forward(sk, idx, n)
        up, pr = up.cpu().numpy().astype(np.float64), pr.cpu().numpy()
        err = np.abs(up - up64).max()
        print('segnet whole model size %d seq_len %d: device %.3e, float32 oracle %.3e (relative to max|up| = %.3e: %.3e and %.3e), '
              'ratio %.3f of 4' % (which, n, err, yard, scale, err / scale, yard / scale, err / yard))
        parity_log('match_segnet_whole_model', dict(size=which, seq_len=n), err, bound, variant='kernel', cpu_fp32_vs_f64=yard,
                   scale=scale, codes_other_than_f64=other)
        assert np.isfinite(up).all() and err <= bound
        assert np.array_equal(pr[sure], pr64[sure])
        boxes, masks = _scene_for(pr64, which, n)
        want = O.select(O.occupancy(pr64, boxes, masks))[0]
        assert 0 < len(want) < len(masks)
        scene = {'sketch': sk, 'boxes': boxes, 'masks': masks, 'class_ids': np.zeros(len(masks), np.int32)}
        matched, _scores, info = M().match_instances(model, scene, text, vocab)
        assert matched == want and info['seq_len'] == n and np.array_equal(info['predicts'], pr)
    # inference keeps nothing for a backward pass
    assert not [k for k in model._bufs if str(k[0]).startswith(('t_', 'bt/', 'bb/'))]


# ------------------------------------------------------------------ one stage at the released widths
def test_stage_at_real_widths():
    """enc_4 -> pool -> unpool -> dec_4 at 8 x 8 x 512 through the kernels MatchModel.segnet calls, in its order: three convs
    256 -> 512 -> 512 -> 512 with the statistics of the 64 pixels, the pool with their last [a | b], the unpool by its codes, two
    convs 512 -> 512 and the materialised relu.  The codes against the float64 oracle's in every sure window, then the output
    against the oracle on the device's codes: 4 x the float32 oracle's own distance from the float64 one."""
    h = hip()
    rng = np.random.RandomState(8)
    x = np.abs(rng.randn(1, 8, 8, 256)).astype(np.float32)
    widths = [('enc_4', 0, 256, 512), ('enc_4', 1, 512, 512), ('enc_4', 2, 512, 512), ('dec_4', 0, 512, 512), ('dec_4', 1, 512, 512)]
    v = {}
    for stage, k, cin, cout in widths:
        v['SegNet/%s/conv%d/DW' % (stage, k + 1)] = (rng.randn(3, 3, cin, cout) * np.sqrt(2.0 / (9 * cout))).astype(np.float32)
        v['SegNet/%s/conv%d/biases' % (stage, k + 1)] = (rng.randn(cout) * 0.1).astype(np.float32)
        v[SO.norm_scope(stage, k) + '/beta'] = (rng.randn(cout) * 0.1).astype(np.float32)
    ones = torch.ones(512, device='cuda')

    def convs(stage, t, n_convs, ab=None):
        for k in range(n_convs):
            out = torch.empty(1, t.shape[1], t.shape[2], 512, device='cuda')
            ab_new, stats = torch.empty(1024, device='cuda'), torch.empty(1024, device='cuda')
            h.conv_forward(h.View(t, None, ab, h.ACT_RELU if ab is not None else h.ACT_NONE), _dev(v['SegNet/%s/conv%d/DW' % (stage, k + 1)]),
                           1, 0, out, same=True, bn=(ones, _dev(v[SO.norm_scope(stage, k) + '/beta']), ab_new, stats, 1e-3))
            t, ab = out, ab_new
        return t, ab
    raw, ab = convs('enc_4', _dev(x), 3)
    pooled, code = h.max_pool2_argmax(raw, ab)
    up = h.unpool2(pooled, code)
    raw, ab = convs('dec_4', up, 2)
    got = torch.empty(1, 8, 8, 512, device='cuda')
    h.call('ssc_affine_act', raw, 512, ab, 512, h.ACT_RELU, got, 512, 64, 512)
    code = code.cpu().numpy()

    def oracle(dtype):
        vv = {k: a.astype(dtype) for k, a in v.items()}
        t = x.astype(dtype)
        for k in range(3):
            t = SO.conv_bn_relu(t, vv, 'enc_4', k)
        taps = SO.window_taps(t)
        p, ind, own, margin = SO.max_pool_with_argmax(t, code)
        t = SO.unpool_2d(p, ind, (8, 8))
        for k in range(2):
            t = SO.conv_bn_relu(t, vv, 'dec_4', k)
        return t, taps, own, margin, p
    ref64, taps64, _own, margin, p64 = oracle(np.float64)
    ref32, taps32, _o, _m, _p = oracle(np.float32)
    own = np.argmax(taps64, axis=0)
    diff = np.abs(taps32.astype(np.float64) - taps64).max(axis=0)
    positive = taps64.max(axis=0) > 0
    sure = (margin > 4 * diff) & (taps64.max(axis=0) > diff)
    unsure = float((positive & ~sure).sum()) / float(positive.sum())
    print('stage at real widths: %d windows, %d positive, unsure share %.5f, %d codes other than the float64 oracle\'s'
          % (sure.size, int(positive.sum()), unsure, int(((code != own) & positive).sum())))
    assert unsure <= 0.005                      # a condition on the seed, checked on the CPU
    assert np.array_equal(code[sure & positive], own[sure & positive])
    assert (ref64 > 0).any() and (ref64 == 0).any()
    got = got.cpu().numpy().astype(np.float64)
    err, yard = np.abs(got - ref64).max(), np.abs(ref32.astype(np.float64) - ref64).max()
    print('stage at real widths: device %.3e, float32 oracle %.3e, max|ref| %.3e, ratio %.3f of 4' % (err, yard, np.abs(ref64).max(), err / yard))
    parity_log('match_segnet_stage', dict(stage='enc_4/dec_4', hw=8, C=512), err, 4 * yard, variant='kernel', cpu_fp32_vs_f64=yard)
    assert np.isfinite(got).all() and err <= 4 * yard


# ------------------------------------------------------------------ the pass in two halves; head training on cached features
def test_features_and_predict_equal_forward(small_segnets):
    model = small_segnets[64]
    model.load_dict(model.test_vars)
    sk, vocab = model.test_sketch, _vocab()
    idx, n = M().preprocess_sentence(SENTENCES[1][0], vocab, 15)
    up, pr = model.forward(sk, idx, n)
    up, pr = up.clone(), pr.clone()
    feat, stroke = model.features(sk)
    assert tuple(feat.shape) == (1, 8, 8, 32) and float(feat.max()) > 0 and float(feat.min()) == 0
    other = M().preprocess_sentence(SENTENCES[2][0], vocab, 15)
    model.predict(feat, stroke, *other)
    up2, pr2 = model.predict(feat, stroke, idx, n)
    assert torch.equal(up2, up) and torch.equal(pr2, pr)
    with pytest.raises(ValueError, match='SegNet backward is not built'):
        model.features(sk, keep={})


def _digest_script():
    sys.path.insert(0, os.path.join(ROOT, 'scripts'))
    try:
        import match_forward_digest as D
    finally:
        sys.path.pop(0)
    return D


@pytest.mark.parametrize('widths,use_attn,size', _digest_script().SEGNET_CASES)
def test_segnet_gives_the_parents_bits(widths, use_attn, size):
    """profiles/match_backbones_once.txt keeps the digests scripts/match_forward_digest.py --segnet 1 printed on the parent commit's
    tree, where the SegNet pass was a method of MatchModel behind an ``if``: head at L = 15, 3, 1, forward, features, predict, and
    at size 64 three steps of the head trainer on the frozen backbone (one from a device-resident scene with its feature map), the
    snapshot's bytes, a resumed step; with each the names that went through hip.call in order.  Size 96 (an odd 3 x 3 map behind
    the last pool) is inference alone.  This tree's are the same, every line."""
    D = _digest_script()
    tag = D.segnet_case_name(widths, use_attn, size) + ' '
    want = {k: v for k, v in D.recorded(os.path.join(ROOT, 'profiles', 'match_backbones_once.txt')).items()
            if k.startswith(tag) and ' host ' not in k}
    got = {k: v for k, v in D.segnet_digests(widths, use_attn, size) if ' host ' not in k}
    assert len(want) == (20 if size == 64 else 10) and set(got) == set(want), set(got) ^ set(want)
    for what, sha in got.items():
        print('%s: %s' % (what, sha))
        assert sha == want[what], what


@pytest.fixture(scope='module')
def split(tmp_path_factory):
    base = str(tmp_path_factory.mktemp('match_segnet'))
    flags = EO.write_split(base, 'train')
    val = EO.write_split(base, 'val')
    return dict(base=base, flags=flags[:4], val=val)


def _child(argv, cwd, ok=True):
    code = ('import json, sys; sys.path.insert(0, %r); import match_main; '
            'from sketchyscenecolorization_amd.matching import MatchConfig; '
            'match_main.main(sys.argv[2:], config=MatchConfig(**json.loads(sys.argv[1])))' % ROOT)
    cfg = dict(size=64, filters=FILTERS, backbone='segnet', **HEAD_SMALL)
    r = subprocess.run([sys.executable, '-c', code, json.dumps(cfg)] + argv, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       timeout=CHILD_LIMIT, cwd=cwd)
    assert (r.returncode == 0) == ok, r.stderr.decode()[-3000:]
    return r.stdout.decode() if ok else r.stderr.decode()


def test_training_on_cached_features_writes_the_same_bytes(split, tmp_path):
    """3 iterations at size 64 in this process, from the scenes' files and from the feature cache: the same snapshot bytes."""
    import match_main
    from sketchyscenecolorization_amd import tf_checkpoint
    cfg = M().MatchConfig(size=64, filters=FILTERS, backbone='segnet', **HEAD_SMALL)
    backbone = str(tmp_path / 'segnet-1')
    tf_checkpoint.write_checkpoint(backbone, {k: a for k, a in M().random_variables(cfg, 31).items() if k.startswith('SegNet/')})
    data = {}
    for mode in ('off', 'features'):
        root = str(tmp_path / mode)
        saved = match_main.main(['--mode', 'train', '--weights', 'segnet', '--backbone_snapshot', backbone, '--vocab_file', VOCAB,
                                 '--scene_size', '64', '--max_iteration', '3', '--log_freq', '1', '--seed', '5', '--snapshot_root', root,
                                 '--log_root', root + '_log', '--scene_cache', mode] + split['flags'], config=cfg)
        assert saved == os.path.join(root, 'segnet_RMI_iter_3.tfmodel')
        data[mode] = open(saved + '.data-00000-of-00001', 'rb').read()
        tensors = tf_checkpoint.read_checkpoint(saved)
    assert len(data['off']) > 0 and data['features'] == data['off']
    have = tf_checkpoint.read_checkpoint(backbone)
    assert all(np.array_equal(tensors[k], have[k]) for k in have)           # the frozen backbone, its moving moments included
    assert 'text_sketchyscene/embedding/Adam' in tensors and not [k for k in tensors if k.startswith('SegNet/') and 'Adam' in k]


def test_command_line_in_fresh_processes(split, tmp_path):
    """Train 2 iterations, then --mode eval and --mode match read segnet_RMI_iter_2.tfmodel; --weights deeplab on it is refused."""
    import scipy.io
    from PIL import Image
    from sketchyscenecolorization_amd import tf_checkpoint
    cfg = M().MatchConfig(size=64, filters=FILTERS, backbone='segnet', **HEAD_SMALL)
    backbone = str(tmp_path / 'segnet-1')
    tf_checkpoint.write_checkpoint(backbone, {k: a for k, a in M().random_variables(cfg, 31).items() if k.startswith('SegNet/')})
    root = str(tmp_path / 'snaps')
    printed = _child(['--mode', 'train', '--weights', 'segnet', '--backbone_snapshot', backbone, '--vocab_file', VOCAB, '--scene_size', '64',
                      '--max_iteration', '2', '--log_freq', '1', '--snapshot_root', root, '--log_root', root + '_log',
                      '--scene_cache', 'device', '--val_freq', '2'] + split['flags'], str(tmp_path))
    prefix = os.path.join(root, 'segnet_RMI_iter_2.tfmodel')
    assert 'model saved to ' + prefix in printed and 'segnet backbone: %d bytes of scratch memory' % cfg.net.scratch_bytes() in printed
    assert 'firstly train, loaded ' + backbone in printed and os.path.exists(prefix + '.index')
    assert os.path.exists(os.path.join(root + '_log', 'match_validation.jsonl'))
    results = str(tmp_path / 'results')
    printed = _child(['--mode', 'eval', '--weights', 'segnet', '--snapshot', root, '--vocab_file', VOCAB, '--scene_size', '64',
                      '--eval_result_root', results] + split['val'], str(tmp_path))
    block = open(os.path.join(results, 'segnet_RMI_val_result.txt')).read()
    assert len(block) > 0 and block in printed and not os.path.exists(os.path.join(results, 'deeplab_RMI_val_result.txt'))
    assert json.load(open(os.path.join(results, 'eval_val.json')))['captions'] == 6
    # --mode match on a scene directory made of the val split's first scene
    d = tmp_path / 'scene'
    for sub in ('sketches', 'inner_masks', 'seg_data'):
        (d / sub).mkdir(parents=True)
    sk = np.array(Image.open(os.path.join(split['base'], 'data', 'val', 'DRAWING_GT', 'L0_sample11.png')))
    Image.fromarray(sk).save(str(d / 'sketches' / '11.png'))
    scipy.io.savemat(str(d / 'inner_masks' / '11.mat'), {'inner_masks': np.zeros((64, 64), np.uint8)})
    with open(os.path.join(split['base'], 'seg', 'val', 'seg_data', '11_datas.npz'), 'rb') as f:
        (d / 'seg_data' / '11_datas.npz').write_bytes(f.read())
    match_argv = ['--snapshot', prefix, '--vocab_file', VOCAB, '--scene_dir', str(d), '--scene_size', '64', '--image_id', '11',
                  '--instruction', 'the house on the left', '--results_dir', str(tmp_path / 'match')]
    printed = _child(match_argv + ['--weights', 'segnet'], str(tmp_path))
    lines = [ln for ln in printed.splitlines() if ln.startswith('matched_inst_indices')]
    rec = json.load(open(str(tmp_path / 'match' / '11' / 'match.json')))
    assert len(lines) == 1 and rec['snapshot'] == prefix and lines[0] == 'matched_inst_indices ' + ','.join(str(k) for k in rec['matched_inst_indices'])
    err = _child(match_argv, str(tmp_path), ok=False)                   # --weights deeplab, the default
    assert 'ValueError' in err and 'SegNet/' in err and '--weights segnet' in err


# ------------------------------------------------------------------ the released size
def test_released_size_runs_and_repeats():
    """768 x 768 at the released widths with random weights, one forward pass run twice: shapes, a finite up, the same bits both
    times.  No oracle here, as in test_real_size_runs_and_repeats: the arithmetic is held by the tests above."""
    m = M()
    cfg = m.MatchConfig(backbone='segnet')
    need = cfg.net.check_scratch(torch.cuda.mem_get_info()[0])
    model = m.MatchModel(cfg)
    model.init_random(1)
    sk = _sketch(768, 768)
    idx, n = m.preprocess_sentence('the bus on the left is yellow', _vocab(), 15)
    up, pr = model.forward(sk, idx, n)
    up1, pr1 = up.clone(), pr.clone()
    up, pr = model.forward(sk, idx, n)
    assert tuple(up.shape) == (768, 768) and up.dtype == torch.float32 and tuple(pr.shape) == (768, 768) and pr.dtype == torch.uint8
    assert bool(torch.isfinite(up).all()) and float(up.abs().max()) > 0
    assert torch.equal(up, up1) and torch.equal(pr, pr1)
    assert tuple(model._buf('sn/feat', (1, 96, 96, 512)).shape) == (1, 96, 96, 512)
    held = sum(b.numel() * b.element_size() for k, b in model._bufs.items() if str(k[0]).startswith(('sn/scratch', 'sn/code', 'sn/feat', 'x4')))
    print('segnet at 768: %d bytes of scratch reckoned, %d held' % (need, held))
    assert held == need
    stroke = torch.from_numpy(O.preprocess(sk)[1]).cuda()
    assert torch.equal(pr, ((up >= 1e-9) & (stroke != 0)).to(torch.uint8))
    model.close()
