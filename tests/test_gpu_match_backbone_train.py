"""Training the matcher's backbone on the device (csrc/match_backbone_train.hip, sketchyscenecolorization_amd/match_backbone_train.py,
match_main.py --train_backbone 1): hip.frozen_act_bwd (ssc_frozen_act_bwd), hip.unit_merge_bwd
(ssc_unit_merge_bwd), hip.zero_stuff2 (ssc_zero_stuff2) and hip.max_pool3s2_bwd (ssc_max_pool3s2_bwd) against float64 formulas,
backbone_train against MatchModel.backbone bit for bit, every trained tensor's gradient against autograd
(tests/match_backbone_oracle.py), the update against float64 Adam + l2 fed the device's own gradients, learning on one tuple with
and without the backbone, the untouched trajectory of --train_backbone 0, the command line in fresh processes, and one step at the
released size.

Tolerance of the gradients: the rule of tests/test_gpu_match_train.py -- per tensor max|g - g64| / max|g64| within 4 x the float32
oracle's own distance from the float64 one, floor 1e-6; the ratios are printed before they are asserted.  The cases are those of
tests/test_match_backbone_train.py, whose seed gives the float32 and the float64 oracle the same sign at every relu and the same
argmax in every pool window (asserted there on the CPU and again here), so the margin is not spent on a flipped mask.  The update
has the tolerance of test_gpu_match_train.py::test_update_rule_is_tf_adam_on_the_devices_own_gradients: 1e-6 of the tensor's
largest entry."""
import faulthandler
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import match_backbone_oracle as BO
import match_eval_oracle as EO
import match_train_oracle as TO
from kernel_check import rc
from test_gpu_match_train import close_to
from test_match_backbone_train import DESCENT, FILTERS, NARROW, UNITS, gradient_case, oracle_descent, oracle_gradients, small_config

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VOCAB = os.path.join(ROOT, 'tests', 'golden', 'match', 'vocab.txt')
CHILD_LIMIT = 180


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


def T():
    from sketchyscenecolorization_amd import match_train
    return match_train


def B():
    from sketchyscenecolorization_amd import match_backbone_train
    return match_backbone_train


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _nan(*shape):
    return torch.full(shape, float('nan'), device='cuda')


# ------------------------------------------------------------------ the kernels
# h != w, odd sizes, C = 4 and a C that is no multiple of 32, and two shapes of more than one workgroup (256 threads x 4 channels)
SHAPES = [(1, 5, 7, 4), (2, 9, 6, 36), (1, 1, 1, 4), (3, 33, 20, 36), (1, 64, 48, 64)]


def _affine(C, seed):
    """[a | b] with negative and positive a, none near 0."""
    rng = np.random.RandomState(seed)
    a = rng.uniform(0.5, 1.5, C) * np.where(rng.rand(C) < 0.4, -1, 1)
    a[0], a[-1] = -abs(a[0]), abs(a[-1])
    return np.concatenate([a, rng.randn(C)]).astype(np.float32)


def _raw_with_clear_signs(shape, ab, seed):
    """r with |a*r + b| >= 0.05 at every entry, both signs present: float32 and float64 agree on every mask."""
    rng = np.random.RandomState(seed)
    C = shape[-1]
    pre = rng.randn(*shape)
    pre = np.sign(pre) * (0.05 + np.abs(pre))
    r = ((pre - ab[C:].astype(np.float64)) / ab[:C].astype(np.float64)).astype(np.float32)
    assert (np.abs(ab[:C].astype(np.float64) * r + ab[C:]) > 0.04).all()
    return r


@pytest.mark.parametrize('shape', SHAPES)
def test_frozen_act_bwd(shape):
    C = shape[-1]
    ab = _affine(C, C + shape[1])
    r = _raw_with_clear_signs(shape, ab, 3)
    g = np.random.RandomState(4).randn(*shape).astype(np.float32)
    a64, b64 = ab[:C].astype(np.float64), ab[C:].astype(np.float64)
    want = g.astype(np.float64) * a64 * (a64 * r + b64 > 0)
    assert (ab[:C] < 0).any() and (ab[:C] > 0).any() and (shape[1] * shape[2] == 1 or (0 < (want != 0).mean() < 1))
    outs = [hip().frozen_act_bwd(_dev(g), _dev(r), _dev(ab), out=_nan(*shape)).cpu().numpy() for _ in range(2)]
    assert np.array_equal(outs[0], outs[1])                                            # the same bits on every run
    err = np.abs(outs[0] - want).max()
    print('frozen_act_bwd %s: err %.3e of %.3e' % (shape, err, np.abs(want).max()))
    assert err <= 2.0 ** -23 * np.abs(want).max()                                       # one rounded product
    assert np.array_equal((outs[0] != 0), (want != 0))
    gd = _dev(g)
    assert hip().frozen_act_bwd(gd, _dev(r), _dev(ab), out=gd) is gd and np.array_equal(gd.cpu().numpy(), outs[0])     # in place


@pytest.mark.parametrize('proj', [False, True])
@pytest.mark.parametrize('shape', SHAPES)
def test_unit_merge_bwd(shape, proj):
    C = shape[-1]
    rng = np.random.RandomState(C + shape[2])
    ab3, abadd = _affine(C, 5), _affine(C, 6)
    out = np.maximum(rng.randn(*shape), 0).astype(np.float32)                           # exact zeros: the mask is 0 there
    g = rng.randn(*shape).astype(np.float32)
    m = out > 0
    assert shape[1] * shape[2] == 1 or (0 < m.mean() < 1)
    want3 = g.astype(np.float64) * m * ab3[:C].astype(np.float64)
    want2 = g.astype(np.float64) * m * (abadd[:C].astype(np.float64) if proj else 1.0)
    outs = []
    for _ in range(2):
        dr3, d2 = hip().unit_merge_bwd(_dev(g), _dev(out), _dev(ab3), _dev(abadd) if proj else None, dr3=_nan(*shape), d2=_nan(*shape))
        outs.append((dr3.cpu().numpy(), d2.cpu().numpy()))
    assert all(np.array_equal(a, b) for a, b in zip(*outs))
    for what, got, want in (('dr3', outs[0][0], want3), ('d2', outs[0][1], want2)):
        err = np.abs(got - want).max()
        print('unit_merge_bwd %s proj %d %s: err %.3e of %.3e' % (shape, proj, what, err, np.abs(want).max()))
        assert err <= 2.0 ** -23 * max(np.abs(want).max(), 1e-30) and not got[~m].any()
    if not proj:
        assert np.array_equal(outs[0][1], np.where(m, g, 0))                            # the identity's share is g itself


@pytest.mark.parametrize('n,H,W,C', [(1, 5, 7, 4), (2, 9, 6, 36), (1, 6, 8, 4), (1, 1, 1, 4), (2, 33, 39, 36)])
def test_zero_stuff2(n, H, W, C):
    h, w = (H + 1) // 2, (W + 1) // 2
    src = np.random.RandomState(H + W).randn(n, h, w, C).astype(np.float32)
    want = np.zeros((n, H, W, C), np.float32)
    want[:, ::2, ::2] = src
    got = hip().zero_stuff2(_dev(src), _nan(n, H, W, C)).cpu().numpy()
    assert np.array_equal(got, want)
    assert np.array_equal(hip().zero_stuff2(_dev(src), _nan(n, H, W, C)).cpu().numpy(), got)


def _pool_ref(r, ab, g, dt):
    """autograd through F.max_pool2d of relu(a*r + b) padded with -inf after (torch: the first maximum in row-major order)."""
    C = r.shape[-1]
    x = torch.tensor(r.transpose(0, 3, 1, 2), dtype=dt, requires_grad=True)
    a, b = (torch.tensor(v.astype(np.float64), dtype=dt).view(1, C, 1, 1) for v in (ab[:C], ab[C:]))
    H, W = r.shape[1:3]
    ph, pw = max((-(-H // 2) - 1) * 2 + 3 - H, 0), max((-(-W // 2) - 1) * 2 + 3 - W, 0)
    y = F.max_pool2d(F.pad(torch.relu(a * x + b), (pw // 2, pw - pw // 2, ph // 2, ph - ph // 2), value=float('-inf')), 3, 2)
    assert tuple(y.shape[2:]) == (-(-H // 2), -(-W // 2))
    (y * torch.tensor(g.transpose(0, 3, 1, 2), dtype=dt)).sum().backward()
    return y.detach().numpy().transpose(0, 2, 3, 1), x.grad.numpy().transpose(0, 2, 3, 1)


def _pool_planes(kind, shape, rng):
    n, H, W, C = shape
    if kind == 'ties':                  # a small set of integers: ties are exact in both precisions
        return rng.randint(-2, 3, shape).astype(np.float32)
    if kind == 'flat':                  # every window is one value: its first real tap takes the gradient
        return np.full(shape, 2, np.float32)
    r = rng.randint(-2, 2, shape).astype(np.float32)
    if kind == 'last_row':              # the maximum of the bottom windows sits only in the last row, next to the padding
        r[:, -1] = 3
    else:                               # .. and only in the last column
        r[:, :, -1] = 3
    return r


@pytest.mark.parametrize('kind', ['ties', 'flat', 'last_row', 'last_col'])
@pytest.mark.parametrize('shape', [(1, 5, 7, 4), (2, 9, 6, 36), (1, 8, 8, 4), (1, 1, 1, 4), (2, 33, 20, 36)])
def test_max_pool3s2_bwd_on_exact_ties(shape, kind):
    """Integer planes, integer gradients and an affine of powers of two and integers: every value is exact in float32 and in
    float64, so the device has to give the oracle's numbers themselves."""
    n, H, W, C = shape
    rng = np.random.RandomState(H * W + len(kind))
    r = _pool_planes(kind, shape, rng)
    a = np.tile(np.array([1, -1, 2, 0.5]), C // 4)
    ab = np.concatenate([a, np.tile(np.array([0, 1, -1, 0.5]), C // 4)]).astype(np.float32)
    g = rng.randint(-3, 4, (n, (H + 1) // 2, (W + 1) // 2, C)).astype(np.float32)
    pooled, want = _pool_ref(r, ab, g, torch.float64)
    assert np.array_equal(hip().max_pool3s2(_dev(r), _dev(ab)).cpu().numpy(), pooled)
    got = hip().max_pool3s2_bwd(_dev(g), _dev(r), _dev(ab), out=_nan(*shape)).cpu().numpy()
    assert np.array_equal(got, hip().max_pool3s2_bwd(_dev(g), _dev(r), _dev(ab), out=_nan(*shape)).cpu().numpy())
    assert np.array_equal(got, want), np.argwhere(got != want)[:5]
    if kind == 'flat' and H > 1:
        # channel 0 (a = 1, b = 0, the plane is 2 > 0): the gradient of window (oy, ox) lands on its first real tap
        py, px = (((H + 1) // 2 - 1) * 2 + 3 - H) // 2, (((W + 1) // 2 - 1) * 2 + 3 - W) // 2
        exp = np.zeros((n, H, W))
        for oy in range((H + 1) // 2):
            for ox in range((W + 1) // 2):
                exp[:, max(oy * 2 - py, 0), max(ox * 2 - px, 0)] += g[:, oy, ox, 0]
        assert np.array_equal(got[..., 0], exp)


@pytest.mark.parametrize('shape', [(1, 5, 7, 4), (2, 9, 6, 36), (1, 64, 48, 64)])
def test_max_pool3s2_bwd_on_floats(shape):
    n, H, W, C = shape
    ab = _affine(C, H)
    r = _raw_with_clear_signs(shape, ab, 8)
    g = np.random.RandomState(9).randn(n, (H + 1) // 2, (W + 1) // 2, C).astype(np.float32)
    _p, w64 = _pool_ref(r, ab, g, torch.float64)
    _p, w32 = _pool_ref(r, ab, g, torch.float32)
    assert np.array_equal(w64 != 0, w32 != 0)
    got = hip().max_pool3s2_bwd(_dev(g), _dev(r), _dev(ab)).cpu().numpy()
    close_to('max_pool3s2_bwd %s' % (shape,), got, w64, w32)
    assert np.array_equal(got != 0, w64 != 0)


def test_refusals_of_the_backbone_kernels():
    z = lambda *s: torch.zeros(s, device='cuda')
    g, r, ab, dr = z(2, 3, 8), z(2, 3, 8), z(16), torch.full((2, 3, 8), 3.0, device='cuda')
    odd = torch.zeros(6 * 8 + 4, device='cuda')[1:]            # 4 bytes off a 16-byte boundary
    assert rc('ssc_frozen_act_bwd', g, r, ab, 6, 6, dr) == -1               # C no multiple of 4
    assert rc('ssc_frozen_act_bwd', g, r, ab, 6, 0, dr) == -1
    assert rc('ssc_frozen_act_bwd', g, r, ab, 0, 8, dr) == -1
    assert rc('ssc_frozen_act_bwd', g, r, None, 6, 8, dr) == -1
    assert rc('ssc_frozen_act_bwd', g, r, ab, 6, 8, r) == -1                # dr may be g, never r
    assert rc('ssc_frozen_act_bwd', g, odd, ab, 6, 8, dr) == -3
    d2 = torch.full((2, 3, 8), 3.0, device='cuda')
    assert rc('ssc_unit_merge_bwd', g, r, ab, None, 6, 6, dr, d2) == -1
    assert rc('ssc_unit_merge_bwd', g, r, ab, None, 0, 8, dr, d2) == -1
    assert rc('ssc_unit_merge_bwd', g, r, None, None, 6, 8, dr, d2) == -1
    assert rc('ssc_unit_merge_bwd', g, r, ab, None, 6, 8, dr, dr) == -1     # the two outputs are distinct
    assert rc('ssc_unit_merge_bwd', g, r, ab, None, 6, 8, g, d2) == -1
    assert rc('ssc_unit_merge_bwd', g, r, ab, odd, 6, 8, dr, d2) == -3
    src, out = z(1, 3, 4, 8), torch.full((1, 5, 7, 8), 3.0, device='cuda')
    assert rc('ssc_zero_stuff2', src, 1, 3, 4, 8, 5, 9, out) == -1          # ceil(9 / 2) is not 4
    assert rc('ssc_zero_stuff2', src, 1, 3, 4, 8, 7, 7, out) == -1
    assert rc('ssc_zero_stuff2', src, 1, 3, 4, 6, 5, 7, out) == -1
    assert rc('ssc_zero_stuff2', src, 0, 3, 4, 8, 5, 7, out) == -1
    assert rc('ssc_zero_stuff2', src, 1, 3, 4, 8, 5, 7, None) == -1
    assert rc('ssc_zero_stuff2', odd, 1, 3, 4, 8, 5, 7, out) == -3
    gp, r0, dr0 = z(1, 3, 4, 8), z(1, 5, 7, 8), torch.full((1, 5, 7, 8), 3.0, device='cuda')
    assert rc('ssc_max_pool3s2_bwd', gp, r0, ab, 1, 5, 7, 6, dr0) == -1
    assert rc('ssc_max_pool3s2_bwd', gp, r0, ab, 1, 0, 7, 8, dr0) == -1
    assert rc('ssc_max_pool3s2_bwd', gp, r0, None, 1, 5, 7, 8, dr0) == -1   # the fused relu needs its affine
    assert rc('ssc_max_pool3s2_bwd', gp, r0, ab, 1, 5, 7, 8, r0) == -1
    assert rc('ssc_max_pool3s2_bwd', gp, odd, ab, 1, 5, 7, 8, dr0) == -3
    assert bool((dr == 3.0).all()) and bool((d2 == 3.0).all()) and bool((out == 3.0).all()) and bool((dr0 == 3.0).all())
    assert rc('ssc_frozen_act_bwd', g, r, ab, 6, 8, dr) == 0 and rc('ssc_unit_merge_bwd', g, r, ab, None, 6, 8, dr, d2) == 0
    assert rc('ssc_zero_stuff2', src, 1, 3, 4, 8, 5, 7, out) == 0 and rc('ssc_max_pool3s2_bwd', gp, r0, ab, 1, 5, 7, 8, dr0) == 0


# ------------------------------------------------------------------ the model: forward bits, gradients
_MODELS = {}


def _model(size):
    """One model and its trainer per size for the module, on gradient_case(size)'s variables."""
    if size not in _MODELS:
        cfg, v, _sk, _labels, _idx, _L, _label = gradient_case(size)
        model = M().MatchModel(cfg)
        model.load_dict(v)
        _MODELS[size] = (model, B().BackboneMatchTrainer(model), v)
    return _MODELS[size]


@pytest.fixture(scope='module', autouse=True)
def _close_models():
    yield
    for model, _t, _v in _MODELS.values():
        model.close()
    _MODELS.clear()


def _x4(model, sk):
    c = model.cfg
    skd = model._buf('sketch', (c.size, c.size, 3), torch.uint8)
    skd.copy_(torch.from_numpy(sk))
    return hip().match_preprocess_u8(skd, out=model._buf('x4', (1, c.size, c.size, 4)),
                                     stroke=model._buf('stroke', (c.size, c.size), torch.uint8))[0]


@pytest.mark.parametrize('size', [64, 96])
def test_backbone_train_has_the_bits_of_backbone(size):
    model, trainer, _v = _model(size)
    sk = gradient_case(size)[2]
    want = model.backbone(_x4(model, sk)).clone()
    got = trainer.backbone_train(_x4(model, sk)).clone()
    assert got.shape == want.shape == (1, size // 8, size // 8, FILTERS[4]) and float(want.max()) > 0
    assert torch.equal(got, want)
    assert torch.equal(trainer._features(sk), want) and torch.equal(model.features(sk)[0], want)
    # every buffer the pass keeps is one of the plan, with the plan's shape
    plan = B().forward_buffer_shapes(model.cfg)
    kept = {k[0]: k[1:] for k in model._bufs if isinstance(k[0], str) and k[0].startswith('bt/')}
    assert kept == {tag: tuple(shape) for tag, shape in plan.items()}
    assert len({model._bufs[(tag,) + tuple(shape)].data_ptr() for tag, shape in plan.items()}) == len(plan)


@pytest.mark.parametrize('size', [64, 96])
def test_every_gradient_equals_autograd(size):
    model, trainer, v = _model(size)
    cfg, _v, sk, labels, idx, L, label = gradient_case(size)
    o = oracle_gradients(size)
    ok, what = BO.records_agree(o[torch.float32][4], o[torch.float64][4])
    assert ok, what
    (l64, g64, p64, f64, _r), (l32, g32, p32, f32, _r2) = o[torch.float64], o[torch.float32]
    feat = trainer._features(sk)
    tok = _dev(idx.astype(np.int32))
    pred = trainer.head_train(feat, tok, L)
    dpred = trainer.loss_and_grad(pred, model._buf('sketch', (size, size, 3), torch.uint8), trainer.upload_scene(labels),
                                  _dev(T().caption_lut([label])))
    trainer.b_grad.fill_(float('nan'))          # every entry of every filter's span is written by backward ..
    real = np.zeros(trainer.b_grad.numel(), bool)
    for name, (off, n, _p, _s) in trainer.b_spans.items():
        real[off:off + n] = True
    trainer.b_grad[_dev(~real)] = 0             # .. and nothing outside the spans: the norm tables' and the padding's entries stay 0
    trainer.backward(dpred)
    flat = trainer.b_grad.cpu().numpy()
    assert np.isfinite(flat).all() and not flat[~real].any()
    loss = float(trainer._loss[0].cpu())
    print('size %d: class loss %.9g, float64 %.9g' % (size, loss, l64))
    assert abs(loss - l64) <= 1e-5 * l64
    close_to('size %d feat' % size, feat.cpu().numpy(), f64, f32)
    close_to('size %d pred' % size, pred.cpu().numpy(), p64, p32)
    got = trainer.export_backbone_gradients()
    got.update(trainer.export_gradients())
    assert set(got) == set(g64) and len(got) == 1 + 3 * sum(UNITS) + 4 + 9
    failed = []
    for name in BO.trained_names(v):
        try:
            close_to('size %d d %s' % (size, name), got[name], g64[name], g32[name])
        except AssertionError as e:
            failed.append(str(e))
    assert not failed, failed
    # the scratch of the backward is the plan's
    plan = B().backward_buffer_shapes(cfg)
    used = {k[0]: k[1:] for k in model._bufs if isinstance(k[0], str) and k[0].startswith('bb/')}
    assert used == {tag: tuple(shape) for tag, shape in plan.items()}
    # and the same bits on a second pass
    trainer.backward(dpred)
    assert np.array_equal(trainer.b_grad.cpu().numpy(), flat)


# ------------------------------------------------------------------ the update
def test_update_is_adam_and_l2_on_the_devices_own_gradients_and_leaves_the_norm_tables():
    cfg, v, sk, labels, idx, L, label = gradient_case(64, seed=23)
    model = M().MatchModel(cfg)
    model.load_dict(v)
    trainer = B().BackboneMatchTrainer(model, weight_decay=5e-4)
    lr = 2.5e-4
    tables = {n: (o, int(np.prod(s))) for n, (o, s) in model._layout.items() if n.startswith('ResNet/') and not n.endswith('/DW')}
    assert len(tables) == len(trainer.b_names)
    tables_before = {n: model.flat[o:o + k].cpu().numpy().tobytes() for n, (o, k) in tables.items()}
    state = {'m': np.zeros(trainer.b_hi), 'v': np.zeros(trainer.b_hi)}
    scene = {'sketch': sk, 'labels_d': trainer.upload_scene(labels)}
    for t in (1, 2, 3):
        before = trainer.b_params.cpu().numpy().astype(np.float64)
        feat = trainer._features(sk)
        pred = trainer.head_train(feat, _dev(idx.astype(np.int32)), L)
        dpred = trainer.loss_and_grad(pred, model._buf('sketch', (64, 64, 3), torch.uint8), scene['labels_d'], _dev(T().caption_lut([label])))
        trainer.backward(dpred)
        grads = trainer.b_grad.cpu().numpy().astype(np.float64)         # the device's own gradients of the class loss
        head_before = trainer.params.clone()
        trainer.apply(lr)
        after = trainer.b_params.cpu().numpy().astype(np.float64)
        assert trainer.step_count == t and not torch.equal(trainer.params, head_before)
        for name, (o, size, padded, _shape) in trainer.b_spans.items():
            sl = slice(o, o + padded)
            w, state['m'][sl], state['v'][sl] = TO.update(name, before[sl], grads[sl], state['m'][sl], state['v'][sl], lr, t, 5e-4)
            err = np.abs(after[sl] - w).max() / np.abs(w).max()
            assert err <= 1e-6, (t, name, err)
            assert np.abs(after[sl] - before[sl]).max() > 0, name
            assert not after[o + size:o + padded].any()
        print('step %d: %d filters within 1e-6 of float64 Adam + l2' % (t, len(trainer.b_spans)))
        for n, (o, k) in tables.items():
            assert model.flat[o:o + k].cpu().numpy().tobytes() == tables_before[n], n       # the norm tables: the bytes they had
    # the next forward pass reads the new filters (the bf16 planes were refreshed): a fresh model loaded from the export
    up, predicts = model.forward(sk, idx, L)
    fresh = M().MatchModel(cfg)
    fresh.load_dict(trainer.export_variables())
    assert torch.equal(fresh.flat, model.flat)
    up2, predicts2 = fresh.forward(sk, idx, L)
    assert torch.equal(up, up2) and torch.equal(predicts, predicts2)
    model.close()
    fresh.close()


# ------------------------------------------------------------------ learning
def _descend(train_backbone):
    cfg, v, sk, labels, idx, L, label = gradient_case(64, fresh_head=True)
    model = M().MatchModel(cfg)
    model.load_dict(v)
    trainer = (B().BackboneMatchTrainer if train_backbone else T().MatchTrainer)(model, DESCENT['weight_decay'])
    scene = {'sketch': sk, 'labels_d': trainer.upload_scene(labels)}
    losses = []
    for n in range(DESCENT['steps']):
        prev = trainer.step(scene, T().caption_lut([label]), idx, L, DESCENT['lr'])
        if prev is not None:
            losses.append(prev)
    losses.append(trainer.last_loss())
    model.close()
    return losses


def test_the_class_loss_falls_further_with_the_backbone():
    """DESCENT['steps'] iterations on one tuple from the same start.  The float64 oracle brings the class loss to 0.47 of the first
    with the backbone and to 0.59 without (tests/test_match_backbone_train.py holds the gap); the device has to follow either
    trajectory: its last loss within 4 x the float32 oracle's distance from the float64 one, with a floor of steps x 4e-6 of the
    loss -- the gradient test allows every step's gradients 4e-6 of their largest entry (4 x a float32 yardstick of 1e-6), Adam's
    update m / (sqrt(v) + eps) is homogeneous of degree 0 in the gradient, so it is off by no more than the gradient is, and the
    steps' errors add up at most linearly over a trajectory whose loss moves by less than itself."""
    got = {tb: _descend(tb) for tb in (True, False)}
    for tb in (True, False):
        o64, o32 = oracle_descent(tb)[torch.float64], oracle_descent(tb)[torch.float32]
        l = got[tb]
        yard = abs(o32[-1] - o64[-1]) / o64[-1]
        err = abs(l[-1] - o64[-1]) / o64[-1]
        print('backbone %d: device %.6g -> %.6g, float64 %.6g -> %.6g; last: device %.3e, float32 oracle %.3e off' %
              (tb, l[0], l[-1], o64[0], o64[-1], err, yard))
        assert len(l) == DESCENT['steps'] and np.isfinite(l).all()
        assert abs(l[0] - o64[0]) <= 1e-5 * o64[0] and l[-1] < l[0]
        assert err <= max(4 * yard, DESCENT['steps'] * 4e-6), (tb, err, yard)
    assert got[True][-1] < 0.85 * got[False][-1]


def test_train_backbone_0_is_the_trajectory_it_was():
    """Three iterations of ``step`` -- what match_main runs without --train_backbone -- beside three of a MatchTrainer driven piece
    by piece as tests/test_gpu_match_train.py drives it (MatchModel.features, head_train, loss_and_grad, backward, apply):
    parameters, Adam slots and losses equal bit for bit, no buffer of the backbone's backward allocated, the backbone's stretch of
    the flat buffer what was loaded."""
    cfg, v, sk, labels, idx, L, label = gradient_case(64, fresh_head=True)
    lut, lr, outs = T().caption_lut([label]), 1e-3, []
    for by_step in (True, False):
        model = M().MatchModel(cfg)
        model.load_dict(v)
        before = model.flat.clone()
        trainer = T().MatchTrainer(model)
        for _ in range(3):
            if by_step:
                trainer.step({'sketch': sk, 'labels': labels}, lut, idx, L, lr)
            else:
                feat, _ = model.features(sk)
                pred = trainer.head_train(feat, _dev(idx.astype(np.int32)), L)
                dpred = trainer.loss_and_grad(pred, model._buf('sketch', (64, 64, 3), torch.uint8), trainer.upload_scene(labels), _dev(lut))
                trainer.backward(dpred)
                trainer.apply(lr)
        loss = trainer.last_loss() if by_step else float(trainer._loss[0].cpu())
        outs.append((model.flat.clone(), trainer.adam_m.clone(), trainer.adam_v.clone(), loss))
        assert not any(isinstance(k[0], str) and k[0].startswith(('bt/', 'bb/')) for k in model._bufs)
        assert torch.equal(model.flat[:trainer.lo], before[:trainer.lo]) and not torch.equal(model.flat, before)
        model.close()
    assert all(torch.equal(a, b) for a, b in zip(outs[0][:3], outs[1][:3])) and outs[0][3] == outs[1][3]


# ------------------------------------------------------------------ the command line
def _child(argv, cwd, ok=True):
    code = ('import json, sys; sys.path.insert(0, %r); import match_main; '
            'from sketchyscenecolorization_amd.matching import MatchConfig; '
            'match_main.main(sys.argv[2:], config=MatchConfig(**json.loads(sys.argv[1])))' % ROOT)
    r = subprocess.run([sys.executable, '-c', code, json.dumps(dict(size=64, units=UNITS, filters=FILTERS, **NARROW))] + argv,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=CHILD_LIMIT, cwd=cwd)
    if ok:
        assert r.returncode == 0, r.stderr.decode()[-3000:]
        return r.stdout.decode()
    assert r.returncode != 0
    return r.stderr.decode()


def test_train_backbone_through_the_command_line(tmp_path):
    """Fresh child processes on the synthetic split of the matcher's tests: 4 iterations with --train_backbone 1 --scene_cache
    device --val_freq 2 and a snapshot every 2; --mode eval reads the snapshot; a run with --scene_cache off, stopped at 2 and
    resumed, ends with the bytes of the uninterrupted one; a snapshot without the backbone's slots is refused; --train_backbone 0 resumes one that has them."""
    from sketchyscenecolorization_amd import tf_checkpoint
    cfg = small_config()
    start = {k: a for k, a in M().random_variables(cfg, 31).items() if k.startswith('ResNet/')}
    backbone = str(tmp_path / 'backbone-1')
    tf_checkpoint.write_checkpoint(backbone, start)
    flags = EO.write_split(str(tmp_path), 'train')[:4]
    eval_flags = EO.write_split(str(tmp_path), 'val', seed=3)
    common = ['--mode', 'train', '--backbone_snapshot', backbone, '--vocab_file', VOCAB, '--scene_size', '64', '--save_model_freq', '2',
              '--log_freq', '1', '--seed', '5'] + flags

    def run(tag, iterations, extra=('--train_backbone', '1', '--scene_cache', 'device', '--val_freq', '2'), ok=True):
        root = str(tmp_path / tag)
        return root, _child(common + list(extra) + ['--snapshot_root', root, '--log_root', root + '_log', '--max_iteration', str(iterations)],
                            str(tmp_path), ok)
    whole, printed = run('whole', 4)
    final = os.path.join(whole, 'deeplab_RMI_iter_4.tfmodel')
    assert printed.strip().split('\n')[-1] == 'model saved to ' + final
    act, scratch, slots = B().training_bytes(cfg)
    assert 'backbone training: %d bytes of kept activations, %d of gradient scratch, %d of gradient and Adam slots' % (act, scratch, slots) in printed
    val = [json.loads(l) for l in open(os.path.join(whole + '_log', 'match_validation.jsonl'))]
    assert [r['iter'] for r in val] == [2, 4]
    assert val[0] != dict(val[1], iter=2)               # scored with the weights of the moment
    tensors = tf_checkpoint.read_checkpoint(final)
    names = B().backbone_variable_names(cfg)
    for name, shape in cfg.variable_shapes().items():
        assert tensors[name].shape == tuple(shape), name
    for name in names:
        assert tensors[name + '/Adam'].shape == tensors[name + '/Adam_1'].shape == tensors[name].shape, name
        assert np.abs(tensors[name] - start[name]).max() > 0 and np.abs(tensors[name + '/Adam_1']).max() > 0, name
    for name in start:
        if name not in names:
            assert np.array_equal(tensors[name], start[name]), name                    # the norms are what the backbone delivered
    assert int(tensors['Variable']) == 4
    out = _child(['--mode', 'eval', '--snapshot', whole, '--vocab_file', VOCAB, '--scene_size', '64',
                  '--eval_result_root', str(tmp_path / 'eval')] + eval_flags, str(tmp_path))
    assert final in out and 'overall IoU = ' in out
    # stopped at 2, resumed to 4, and with --scene_cache off: the bytes of the uninterrupted run from the device cache
    off = ('--train_backbone', '1', '--scene_cache', 'off', '--val_freq', '2')
    parts, _ = run('parts', 2, extra=off)
    _, printed2 = run('parts', 4, extra=off)
    assert 'start_iter 2' in printed2
    a = open(final + '.data-00000-of-00001', 'rb').read()
    b = open(os.path.join(parts, 'deeplab_RMI_iter_4.tfmodel.data-00000-of-00001'), 'rb').read()
    assert len(a) > 0 and a == b
    # a run of the head alone writes no slots of the backbone: --train_backbone 1 cannot resume it, and says which run wrote it
    plain, _ = run('plain', 2, extra=())
    err = run('plain', 4, ok=False)[1]
    assert 'ValueError' in err and 'ResNet/group_1/conv1/DW/Adam' in err and '--train_backbone 0' in err
    assert not os.path.exists(os.path.join(plain, 'deeplab_RMI_iter_4.tfmodel.index'))
    # --train_backbone 0 resumes a snapshot that has them and ignores them
    _, printed3 = run('whole', 6, extra=())
    assert 'start_iter 4' in printed3
    t6 = tf_checkpoint.read_checkpoint(os.path.join(whole, 'deeplab_RMI_iter_6.tfmodel'))
    assert names[0] + '/Adam' not in t6 and all(np.array_equal(t6[n], tensors[n]) for n in names)
    assert np.abs(t6[TO.P + 'embedding'] - tensors[TO.P + 'embedding']).max() > 0


# ------------------------------------------------------------------ the released size
def test_one_step_at_the_released_size_twice_for_the_same_bits():
    """768 x 768, units (3, 4, 23, 3), the released widths, random weights: one whole step, then the same step from the same
    start on the same buffers; parameters and slots equal bit for bit, every filter moved, the norm tables not."""
    cfg = M().MatchConfig()
    v = M().random_variables(cfg, 5)
    rng = np.random.RandomState(6)
    sk = np.full((768, 768, 3), 255, np.uint8)
    sk[rng.rand(768, 768) < 0.1] = 0
    labels = np.zeros((768, 768), np.uint8)
    labels[100:400, 80:500] = 1
    idx = np.zeros(cfg.max_len, np.int64)
    idx[:4] = (5, 9, 3, 7)
    act, scratch, slots = B().check_budget(cfg, torch.cuda.mem_get_info()[0])
    outs = []
    for _ in range(2):
        model = M().MatchModel(cfg)
        model.load_dict(v)
        start = model.flat.clone()
        trainer = B().BackboneMatchTrainer(model)
        trainer.step({'sketch': sk, 'labels_d': trainer.upload_scene(labels)}, T().caption_lut([1]), idx, 4, 2.5e-4)
        loss = trainer.last_loss()
        outs.append((model.flat.clone(), trainer.b_adam_m.clone(), trainer.b_adam_v.clone(), loss))
        kept = 4 * sum(b.numel() for k, b in model._bufs.items() if isinstance(k[0], str) and k[0].startswith('bt/'))
        used = 4 * sum(b.numel() for k, b in model._bufs.items() if isinstance(k[0], str) and k[0].startswith('bb/'))
        assert (kept, used, 12 * trainer.b_hi) == (act, scratch, slots)
        spans, layout = dict(trainer.b_spans), dict(model._layout)
        model.close()
        del model, trainer
        torch.cuda.empty_cache()
    print('released size: %d bytes of activations kept, %d of scratch, %d of gradient and slots; loss %.6g' % (act, scratch, slots, outs[0][3]))
    assert np.isfinite(outs[0][3]) and outs[0][3] > 0 and bool(torch.isfinite(outs[0][0]).all())
    assert all(torch.equal(a, b) for a, b in zip(outs[0][:3], outs[1][:3])) and outs[0][3] == outs[1][3]
    moved = outs[0][0] != start
    for name, (o, size, _p, _s) in spans.items():
        assert bool(moved[o:o + size].any()), name
    for n, (o, s) in layout.items():
        if n.startswith('ResNet/') and not n.endswith('/DW'):
            assert not bool(moved[o:o + int(np.prod(s))].any()), n
