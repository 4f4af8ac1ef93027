"""The matcher's word attention on the device (csrc/match_attn.hip, MatchConfig(use_attn=True), match_main.py --use_attn 1;
DESIGN.md section 8.11): hip.attn_scores_fwd (ssc_attn_scores_fwd), hip.dev_scaled_add (ssc_dev_scaled_add), hip.attn_plane_dots
(ssc_attn_plane_dots) and hip.attn_scores_bwd (ssc_attn_scores_bwd) against float64; ``head`` after a longer sentence; head_train
against head bit for bit; the free bias; every trained tensor's gradient against autograd (tests/match_attn_oracle.py); the update
rule; --train_backbone 1; the command line in fresh processes; and the flag-off path against the parent commit's digests.

Kernel bounds are derived, not tuned: an output is held within (the roundings on its path) x 2^-24 x (the sum of the absolute
terms that make it), each test says which.  Network-level tolerances are tests/test_gpu_match_train.py's ``close_to``: 4 x the
float32 oracle's own distance from the float64 one, floor 1e-6.  Every figure is printed before it is asserted."""
import faulthandler
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import match_attn_oracle as AO
import match_eval_oracle as EO
import match_train_oracle as TO
from kernel_check import rc
from test_gpu_match_train import BF, NARROW, SMALL, _dev, _feat, _scene, _sentence, close_to

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VOCAB = os.path.join(ROOT, 'tests', 'golden', 'match', 'vocab.txt')
PARITY = os.path.join(ROOT, 'profiles', 'match_attn_parity.txt')
CHILD_LIMIT = 180
U = 2.0 ** -24
T15 = 15
DW, B = AO.ATTN_NAMES
NAN = float('nan')


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


def held(what, got, ref64, bound):
    """|got - ref64| <= bound, element by element; prints the worst ratio first."""
    got, ref64, bound = (np.asarray(a, np.float64) for a in (got, ref64, bound))
    assert got.shape == ref64.shape == bound.shape, (what, got.shape, ref64.shape, bound.shape)
    assert np.isfinite(got).all(), what
    err = np.abs(got - ref64)
    ratio = float(np.max(np.where(err > 0, err / np.maximum(bound, 1e-300), 0.0))) if err.size else 0.0
    print('%s: worst err / bound %.3e (max err %.3e)' % (what, ratio, float(err.max()) if err.size else 0.0))
    assert (err <= bound).all(), (what, ratio)


# ------------------------------------------------------------------ ssc_attn_scores_fwd
def _scores_case(C, ld, L, seed):
    """hs with NaN in the rows >= L (an earlier sentence's leftovers must not be read) and in the pad columns."""
    rng = np.random.RandomState(seed)
    hs = np.full((T15, ld), NAN, np.float32)
    hs[:L, :C] = rng.uniform(-1, 1, (L, C))
    w = np.full(ld, NAN, np.float32)
    w[:C] = rng.uniform(-1, 1, C) * np.sqrt(3.0 / C) * 4            # logits a few units apart
    b = np.array([0.3], np.float32)
    return hs, w, b


def _softmax64(hs, w, b, C, L):
    logit = np.full(T15, float(b[0]), np.float64)
    logit[:L] += hs[:L, :C].astype(np.float64) @ w[:C].astype(np.float64)
    e = np.exp(logit - logit.max())
    return logit, e / e.sum()


@pytest.mark.parametrize('L', [1, 3, T15])
@pytest.mark.parametrize('C,ld', [(40, 64), (1000, 1024)])
def test_attn_scores_fwd(C, ld, L):
    """The bound: a logit is ceil(C / 64) fused multiply-adds in a lane, six additions of the butterfly and the bias -- K =
    ceil(C / 64) + 7 roundings on A[t] = sum |hs w| + |b|, so |d logit| <= D = K u max A.  exp(logit[t] - m) carries the errors of
    both logits, the rounded difference (u |logit - m|) and expf (2 u); the sum runs in double; the quotient is rounded once:
    |d attn[t]| <= attn[t] * expm1(4 D + 2 u max|logit - m| + 5 u)."""
    hs, w, b = _scores_case(C, ld, L, 100 + C + L)
    out = torch.full((T15 + 3,), NAN, device='cuda')
    got = hip().attn_scores_fwd(_dev(hs), _dev(w), _dev(b), C, L, out=out[:T15]).cpu().numpy()
    again = hip().attn_scores_fwd(_dev(hs), _dev(w), _dev(b), C, L).cpu().numpy()
    assert np.array_equal(got, again) and bool(torch.isnan(out[T15:]).all())
    logit, want = _softmax64(hs, w, b, C, L)
    A = np.abs(hs[:L, :C].astype(np.float64) * w[:C].astype(np.float64)).sum(axis=1).max() + abs(float(b[0]))
    D = (-(-C // 64) + 7) * U * A
    held('attn_scores_fwd C %d L %d' % (C, L), got, want, want * np.expm1(4 * D + 2 * U * np.ptp(logit) + 5 * U))
    assert abs(float(got.astype(np.float64).sum()) - 1) <= (T15 + 1) * U
    if L < T15:     # the padded positions weigh exp(b) each: equal among themselves, and the real ones sum to less than 1
        assert np.ptp(got[L:]) == 0 and got[L] > 0 and got[:L].sum() < 1 - 1e-3


def test_attn_scores_refusals():
    hs, w, b = (_dev(a) for a in _scores_case(40, 64, 3, 1))
    out = torch.full((T15,), 7.0, device='cuda')
    for L in (0, -1, T15 + 1):
        with pytest.raises(ValueError, match='attn_scores_fwd'):
            hip().attn_scores_fwd(hs, w, b, 40, L, out=out)
    big = torch.zeros((65, 64), device='cuda')
    with pytest.raises(ValueError, match='attn_scores_fwd'):
        hip().attn_scores_fwd(big, w, b, 40, 3, out=torch.zeros(65, device='cuda'))
    hip().attn_scores_fwd(big, torch.zeros(64, device='cuda'), b, 40, 64, out=torch.zeros(64, device='cuda'))     # 64 words: held
    assert rc('ssc_attn_scores_fwd', hs, 32, w, b, 40, 3, T15, out) == -1             # ld < C
    assert rc('ssc_attn_scores_fwd', hs, 64, w, None, 40, 3, T15, out) == -1
    assert bool((out == 7.0).all())
    attn, dattn = torch.full((T15,), 1 / 15.0, device='cuda'), torch.zeros(T15, device='cuda')
    dhs = torch.full((T15, 64), 5.0, device='cuda')
    for L in (0, T15 + 1):
        with pytest.raises(ValueError, match='attn_scores_bwd'):
            hip().attn_scores_bwd(attn, dattn, hs, w, 40, L, dhs=dhs)
    with pytest.raises(ValueError, match='attn_scores_bwd'):
        hip().attn_scores_bwd(torch.zeros(65, device='cuda'), torch.zeros(65, device='cuda'), big, w, 40, 3, dhs=torch.zeros((65, 64), device='cuda'))
    assert bool((dhs == 5.0).all())


# ------------------------------------------------------------------ ssc_dev_scaled_add
@pytest.mark.parametrize('overwrite', [False, True])
@pytest.mark.parametrize('n,shift', [(1, 0), (31, 0), (65, 0), (65, 1), (9216 * 512, 0)])
def test_dev_scaled_add(n, shift, overwrite):
    """One fmaf per element, correctly rounded: |err| <= u * (|s x| + |y|).  shift 1: both operands 4 bytes off a 16-byte
    boundary (the scalar form).  With overwrite y is not read (it holds NaN); only s[k] of s is read (the others hold NaN)."""
    rng = np.random.RandomState(n + shift)
    x = rng.randn(n + shift).astype(np.float32)
    y0 = rng.randn(n + shift).astype(np.float32)
    s = np.full(5, NAN, np.float32)
    s[3] = 0.37
    yd = torch.full((n + shift + 8,), NAN, device='cuda')
    if not overwrite:
        yd[:n + shift] = _dev(y0)
    xd = _dev(x)
    hip().dev_scaled_add(yd[shift:shift + n], xd[shift:], _dev(s), 3, overwrite=overwrite)
    got = yd.cpu().numpy()
    assert np.isnan(got[shift + n:]).all() and (shift == 0 or (np.isnan(got[0]) if overwrite else got[0] == y0[0]))
    sx = np.float64(s[3]) * x[shift:].astype(np.float64)
    base = np.zeros(n) if overwrite else y0[shift:].astype(np.float64)
    held('dev_scaled_add n %d shift %d overwrite %d' % (n, shift, overwrite), got[shift:shift + n], sx + base, U * (np.abs(sx) + np.abs(base)))


def test_dev_scaled_add_refusals():
    x, y, s = torch.ones(8, device='cuda'), torch.full((8,), 2.0, device='cuda'), torch.ones(3, device='cuda')
    for k in (-1, 3):
        with pytest.raises(ValueError, match='dev_scaled_add'):
            hip().dev_scaled_add(y, x, s, k)
    assert rc('ssc_dev_scaled_add', y, x, s, 3, 0, 0, 0) == -1 and rc('ssc_dev_scaled_add', y, None, s, 3, 0, 8, 0) == -1
    assert bool((y == 2.0).all())


# ------------------------------------------------------------------ ssc_attn_plane_dots
@pytest.mark.parametrize('L', [1, T15])
@pytest.mark.parametrize('n', [32, 65 * 32, 9216 * 512])
def test_attn_plane_dots(n, L):
    """A product of two floats is exact in double and the double sum's own error is below 2^-40 of the absolute terms; the sum is
    rounded to float once: |err| <= 2^-22 * sum |dacc h| holds that with room (the issue's bound)."""
    g = torch.Generator().manual_seed(n + L)
    dacc = torch.randn(n, generator=g)
    planes = torch.randn(L, n, generator=g)
    dd, pd = dacc.cuda(), planes.cuda()
    out = torch.full((L + 2,), NAN, device='cuda')
    got = hip().attn_plane_dots(dd, pd, L, out=out).cpu().numpy()
    again = hip().attn_plane_dots(dd, pd, L).cpu().numpy()
    assert np.array_equal(got[:L], again[:L]) and np.isnan(got[L:]).all()          # the same bits on every run
    want = (planes.double() @ dacc.double()).numpy()
    mag = (planes.double().abs() @ dacc.double().abs()).numpy()
    held('attn_plane_dots n %d L %d' % (n, L), got[:L], want, 2.0 ** -22 * mag)


def test_attn_plane_dots_strides_and_refusals():
    """A stride beyond n (the gap holds NaN), an odd stride (the scalar form), and every refusal."""
    n, L = 65 * 32, 3
    g = torch.Generator().manual_seed(5)
    dacc = torch.randn(n, generator=g)
    ws = hip().workspace()
    for stride in (n + 4, n + 1):
        planes = torch.full((L, stride), NAN)
        planes[:, :n] = torch.randn(L, n, generator=g)
        out = torch.full((L,), NAN, device='cuda')
        assert rc('ssc_attn_plane_dots', dacc.cuda(), planes.cuda(), stride, n, L, out, ws, ws.numel() * 4) == 0
        want = (planes[:, :n].double() @ dacc.double()).numpy()
        held('attn_plane_dots stride n + %d' % (stride - n), out.cpu().numpy(), want, 2.0 ** -22 * (planes[:, :n].double().abs() @ dacc.double().abs()).numpy())
    dd, pd = dacc.cuda(), torch.zeros((65, n), device='cuda')
    out = torch.full((65,), 9.0, device='cuda')
    for bad in (0, 65):
        with pytest.raises(ValueError, match='attn_plane_dots'):
            hip().attn_plane_dots(dd, pd, bad, out=out)
    need = hip().attn_plane_dots_workspace_bytes(n, L)
    assert need == 8 * 3 and hip().attn_plane_dots_workspace_bytes(9216 * 512, 15) == 8 * 15 * 512
    assert rc('ssc_attn_plane_dots', dd, pd, n, n, L, out, ws, need - 1) == -1
    assert rc('ssc_attn_plane_dots', dd, pd, n - 1, n, L, out, ws, need) == -1
    assert rc('ssc_attn_plane_dots', dd, pd, n, n, L, out, None, need) == -1
    assert bool((out == 9.0).all())
    assert rc('ssc_attn_plane_dots', dd, pd, n, n, L, out, ws, need) == 0


# ------------------------------------------------------------------ ssc_attn_scores_bwd
@pytest.mark.parametrize('L', [1, 3, T15])
@pytest.mark.parametrize('C,ld', [(40, 64), (1000, 1024)])
def test_attn_scores_bwd(C, ld, L):
    """dot = sum attn dattn runs in double; dlogit[t] = attn[t] * (dattn[t] - dot) is the rounded difference times attn: 2
    roundings on A[t] = attn[t] * (|dattn[t]| + sum |attn dattn|).  dw[c]: L fused multiply-adds more, (L + 2) u sum_t A[t] |hs|.
    dhs: one more, 3 u (A[t] |w| + |dhs before|).  db: the plain float sum of the T values, whose exact value is 0:
    |db| <= 16 u sum |dlogit| (T = 15 additions and one rounding of the weights' own sum)."""
    hs, w, b = _scores_case(C, ld, L, 200 + C + L)
    rng = np.random.RandomState(L)
    _logit, attn64 = _softmax64(hs, w, b, C, L)
    attn = attn64.astype(np.float32)
    dattn = np.full(T15, NAN, np.float32)
    dattn[:L] = rng.randn(L)
    dhs0 = np.full((T15, ld), NAN, np.float32)
    dhs0[:L, :C] = rng.randn(L, C)
    outs = []
    for _ in range(2):
        dhs = _dev(dhs0)
        dw, db, dl = torch.full((ld,), NAN, device='cuda'), torch.full((2,), NAN, device='cuda'), torch.full((T15 + 1,), NAN, device='cuda')
        hip().attn_scores_bwd(_dev(attn), _dev(dattn), _dev(hs), _dev(w), C, L, dhs=dhs, dw=dw, db=db, dlogit=dl[:T15])
        outs.append([a.cpu().numpy() for a in (dl, dw, db, dhs)])
    (dl, dw, db, dhs), second = outs
    assert all(np.array_equal(a, c, equal_nan=True) for a, c in zip(outs[0], second))
    assert np.isnan(dl[T15:]).all() and np.isnan(dw[C:]).all() and np.isnan(db[1:]).all()
    assert np.isnan(dhs[L:]).all() and np.isnan(dhs[:L, C:]).all()                    # nothing touched beyond L rows and C columns
    a64, d64 = attn.astype(np.float64), np.zeros(T15)
    d64[:L] = dattn[:L]
    mag = np.abs(a64 * d64).sum()
    dl64 = a64 * (d64 - (a64 * d64).sum())
    A = a64 * (np.abs(d64) + mag)
    tag = 'attn_scores_bwd C %d L %d ' % (C, L)
    held(tag + 'dlogit', dl[:T15], dl64, 2 * U * A)
    h64, w64 = hs[:L, :C].astype(np.float64), w[:C].astype(np.float64)
    held(tag + 'dw', dw[:C], dl64[:L] @ h64, (L + 2) * U * (A[:L] @ np.abs(h64)))
    held(tag + 'dhs', dhs[:L, :C], dhs0[:L, :C] + np.outer(dl64[:L], w64), 3 * U * (np.outer(A[:L], np.abs(w64)) + np.abs(dhs0[:L, :C])))
    bound = 16 * U * np.abs(dl64).sum()
    print(tag + 'db %.3e, bound %.3e' % (float(db[0]), bound))
    assert abs(float(db[0])) <= bound
    assert float(db[0]) == float(np.cumsum(dl[:T15], dtype=np.float32)[-1])            # the plain sum in index order


# ------------------------------------------------------------------ the head: forward bits, the free bias, gradients
_MODELS = {}
KW = {'narrow': dict(SMALL, **NARROW), 'bf': dict(SMALL, **BF), 'released': dict(size=32, units=(1, 1, 1, 1), filters=(8, 16, 32, 64, 2048))}


def _model(key):
    """One model with the attention per configuration for the module: (model, trainer, its variables)."""
    if key not in _MODELS:
        m = M()
        cfg = m.MatchConfig(use_attn=True, **KW[key])
        v = m.random_variables(cfg, 17)
        v[DW] = (v[DW] * 4).astype(np.float32)            # weights that are visibly not uniform
        model = m.MatchModel(cfg)
        model.load_dict(v)
        _MODELS[key] = (model, T().MatchTrainer(model), v)
    return _MODELS[key]


@pytest.fixture(scope='module', autouse=True)
def _close_models():
    yield
    for model, _t, _v in _MODELS.values():
        model.close()
    _MODELS.clear()


def test_head_after_a_longer_sentence():
    """The rows 3 .. 14 of the word LSTM's buffers hold the longer sentence's states: the second result must not see them."""
    model, _trainer, v = _model('narrow')
    feat = _dev(_feat(model.cfg, 3))
    long_tok, short_tok = (_dev(_sentence(model.cfg, L, 4 + L).astype(np.int32)) for L in (T15, 3))
    model.head(feat, long_tok, T15)
    got = model.head(feat, short_tok, 3).clone()
    attn = model._buf('attn', (T15,)).clone()
    fresh = M().MatchModel(model.cfg)
    fresh.load_dict(v)
    want = fresh.head(feat, short_tok, 3)
    assert float(want.abs().max()) > 0 and torch.equal(got, want) and torch.equal(attn, fresh._buf('attn', (T15,)))
    assert float(attn[3:].max()) == float(attn[3:].min()) and abs(float(attn.double().sum()) - 1) <= 16 * U
    fresh.close()


@pytest.mark.parametrize('key,seq_len', [('narrow', 1), ('narrow', T15), ('bf', 4)])
def test_head_train_has_the_bits_of_head(key, seq_len):
    model, trainer, _v = _model(key)
    assert hip().lstm_bf(model.cm, 4 * model.cm) == (key == 'bf')
    feat = _dev(_feat(model.cfg, 3))
    tok = _dev(_sentence(model.cfg, seq_len, 4).astype(np.int32))
    want = model.head(feat, tok, seq_len).clone()
    got = trainer.head_train(feat, tok, seq_len).clone()
    assert got.shape == want.shape == (model.cfg.feat, model.cfg.feat) and float(want.abs().max()) > 0
    assert torch.equal(got, want)
    assert torch.equal(model.head(feat, tok, seq_len), want)
    # and the attention changes the result: the same weights read through the last state give something else
    plain = M().MatchModel(M().MatchConfig(**KW[key]))
    plain.load_dict({k: a for k, a in _v.items() if k not in AO.ATTN_NAMES})
    assert not torch.equal(plain.head(feat, tok, seq_len), want)
    plain.close()


def test_pred_does_not_move_with_the_bias():
    """The bias shifts all T logits alike.  With b = 3 the logits are rounded at the scale of 4, half a float32 ulp there each;
    the bar is 4 ulp of that scale, passed on to pred relatively: 4 * spacing(max |logit|) * max |pred|."""
    model, _trainer, v = _model('narrow')
    feat, tok = _dev(_feat(model.cfg, 8)), _dev(_sentence(model.cfg, 4, 9).astype(np.int32))
    preds = []
    for b in (0.0, 3.0):
        model.d['attn/b'].fill_(b)
        preds.append(model.head(feat, tok, 4).clone().cpu().numpy().astype(np.float64))
    hs = model._buf('hw', (T15 + 1, model.cw))[1:5, :model.cfg.w_rnn].cpu().numpy().astype(np.float64)
    scale = float(np.abs(hs @ v[DW].reshape(-1).astype(np.float64)).max()) + 3.0
    model.d['attn/b'].copy_(_dev(v[B]))
    tol = 4 * float(np.spacing(np.float32(scale))) * float(np.abs(preds[0]).max())
    err = float(np.abs(preds[0] - preds[1]).max())
    print('pred with attn/b 0 against 3: max |difference| %.3e, bar %.3e (logits up to %.3f)' % (err, tol, scale))
    assert np.abs(preds[0]).max() > 0 and err <= tol


def _real_entries(trainer):
    """1 where the flat head buffer holds an entry of a variable, 0 on the padding."""
    ones = {n: np.ones(s, np.float32) for n, s in trainer.cfg.variable_shapes().items() if n.startswith(TO.P)}
    mask = np.zeros(trainer.grad.numel(), np.float32)
    for name, a in T().pack_head(trainer.cfg, ones).items():
        o, size, _padded, _shape = trainer.spans[name]
        mask[o:o + size] = a.reshape(-1)
    return mask


@pytest.mark.parametrize('key,seq_len,repeat', [('narrow', 1, False), ('narrow', 3, True), ('narrow', T15, True), ('bf', 3, True),
                                                ('released', 3, False)])
def test_head_gradients_equal_autograd(key, seq_len, repeat):
    model, trainer, v = _model(key)
    cfg = model.cfg
    feat, idx = _feat(cfg, 5 + seq_len), _sentence(cfg, seq_len, 6 + seq_len, repeat)
    if repeat:
        assert (idx[:seq_len] == idx[0]).sum() == 3
    dpred = np.random.RandomState(7).randn(cfg.feat, cfg.feat).astype(np.float32)
    flats = []
    for _ in range(2):
        pred = trainer.head_train(_dev(feat), _dev(idx.astype(np.int32)), seq_len)
        trainer.grad.fill_(NAN)                     # every entry of every tensor is written by backward ..
        mask = _real_entries(trainer)
        trainer.grad[_dev(mask == 0)] = 0           # .. except the padding, which nobody writes and which stays zero
        trainer.backward(_dev(dpred))
        flats.append(trainer.grad.cpu().numpy())
    flat = flats[0]
    assert np.array_equal(flat, flats[1])                                # a second backward gives the same bits
    assert np.isfinite(flat).all() and mask.sum() < mask.size
    assert not flat[mask == 0].any()                                    # the padded entries of the device gradient are exactly 0
    o, size, _p, _s = trainer.spans['attn/w']
    assert size == model.cw and (mask[o:o + size] == 1).sum() == cfg.w_rnn
    got = trainer.export_gradients()
    g64, p64 = AO.head_gradients(feat, v, idx, seq_len, cfg.max_len, dpred)
    g32, p32 = AO.head_gradients(feat, v, idx, seq_len, cfg.max_len, dpred, torch.float32)
    tag = 'attn %s L %d ' % (key, seq_len)
    close_to(tag + 'pred', pred.cpu().numpy(), p64, p32)
    for name in AO.HEAD_NAMES:
        if name != B:
            close_to(tag + 'd ' + name[len(TO.P):], got[name], g64[name], g32[name])
    assert np.abs(g64[DW]).max() > 0
    # the bias: its exact gradient is 0 (float64 autograd gives rounding noise); the device's is the float sum of the T logit gradients
    dlogit = model._buf('b_dlogit', (cfg.max_len,)).cpu().numpy().astype(np.float64)
    bound = 16 * U * np.abs(dlogit).sum()
    print(tag + 'd attn_fc/biases: device %.3e, bound %.3e, float64 autograd %.3e, float32 autograd %.3e'
          % (float(got[B][0]), bound, float(g64[B][0]), float(g32[B][0])))
    assert np.abs(dlogit).sum() > 0 and abs(float(got[B][0])) <= bound


# ------------------------------------------------------------------ the optimiser, the backbone
def test_three_steps_are_tf_adam_on_the_devices_own_gradients():
    """tests/test_gpu_match_train.py::test_update_rule_is_tf_adam_on_the_devices_own_gradients with the attention: the same
    procedure and the same bar (1e-6 relative per tensor), and the two new tensors move under their own rules."""
    m = M()
    cfg = m.MatchConfig(use_attn=True, **dict(SMALL, **NARROW))
    v = m.random_variables(cfg, 23)
    model = m.MatchModel(cfg)
    model.load_dict(v)
    trainer = T().MatchTrainer(model, weight_decay=5e-4)
    assert trainer.dev_to_var['attn/w'] == 'attn_fc/DW' and trainer.dev_to_var['attn/b'] == 'attn_fc/biases'
    scene, lut, idx, L, lr = _scene(cfg, 1), T().caption_lut([2]), _sentence(cfg, 5, 2), 5, 2.5e-4
    mask = _real_entries(trainer)
    state = {'m': np.zeros_like(mask, np.float64), 'v': np.zeros_like(mask, np.float64)}
    for t in (1, 2, 3):
        before = trainer.params.cpu().numpy().astype(np.float64)
        feat, _ = model.features(scene['sketch'])
        pred = trainer.head_train(feat, _dev(idx.astype(np.int32)), L)
        dpred = trainer.loss_and_grad(pred, model._buf('sketch', (64, 64, 3), torch.uint8), trainer.upload_scene(scene['labels']), _dev(lut))
        trainer.backward(dpred)
        grads = trainer.grad.cpu().numpy().astype(np.float64)
        trainer.apply(lr)
        after = trainer.params.cpu().numpy().astype(np.float64)
        for name, (o, size, padded, _shape) in trainer.spans.items():
            sl = slice(o, o + padded)
            w, state['m'][sl], state['v'][sl] = TO.update(TO.P + trainer.dev_to_var[name], before[sl], grads[sl], state['m'][sl],
                                                          state['v'][sl], lr, t, 5e-4)
            err = np.abs(after[sl] - w).max() / np.abs(w).max()
            print('attn step %d %s: rel %.3e' % (t, name, err))
            assert err <= 1e-6, (t, name, err)
            if name != 'attn/b':        # the free parameter's gradient is rounding noise, it may or may not move
                assert np.abs(after[sl] - before[sl]).max() > 0, name
        assert not after[mask == 0].any()
    up, predicts = model.forward(scene['sketch'], idx, L)
    fresh = m.MatchModel(cfg)
    fresh.load_dict(trainer.export_variables())
    assert torch.equal(fresh.flat, model.flat)
    up2, predicts2 = fresh.forward(scene['sketch'], idx, L)
    assert torch.equal(up, up2) and torch.equal(predicts, predicts2)
    model.close()
    fresh.close()


def test_backbone_training_with_the_flag():
    """--train_backbone 1 goes through head_train and backward: one step with the attention runs, the filters' gradients are
    finite, and they are not those of the step without it."""
    from sketchyscenecolorization_amd import match_backbone_train as BT
    m = M()
    grads = {}
    for flag in (False, True):
        cfg = m.MatchConfig(use_attn=flag, **dict(SMALL, **NARROW))
        model = m.MatchModel(cfg)
        model.load_dict(m.random_variables(cfg, 31))
        trainer = BT.BackboneMatchTrainer(model)
        trainer.step(_scene(cfg, 1), T().caption_lut([2]), _sentence(cfg, 5, 2), 5, 2.5e-4)
        loss = trainer.last_loss()
        grads[flag] = trainer.b_grad.cpu().numpy()
        assert np.isfinite(loss) and np.isfinite(grads[flag]).all() and np.abs(grads[flag]).max() > 0
        if flag:
            assert np.isfinite(trainer.grad.cpu().numpy()).all() and float(trainer.g['attn/w'].abs().max()) > 0
        model.close()
    assert grads[False].shape == grads[True].shape and not np.array_equal(grads[False], grads[True])


# ------------------------------------------------------------------ the command line
def _child(argv, cwd, use_attn, ok=True):
    code = ('import json, sys; sys.path.insert(0, %r); import match_main; '
            'from sketchyscenecolorization_amd.matching import MatchConfig; '
            'match_main.main(sys.argv[2:], config=MatchConfig(**json.loads(sys.argv[1])))' % ROOT)
    r = subprocess.run([sys.executable, '-c', code, json.dumps(dict(SMALL, use_attn=use_attn, **NARROW))] + argv, stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, timeout=CHILD_LIMIT, cwd=cwd)
    if ok:
        assert r.returncode == 0, r.stderr.decode()[-3000:]
        return r.stdout.decode()
    assert r.returncode != 0
    return r.stderr.decode()


def _scene_dir(base, S=64):
    """A scene for --mode match, in the files fg_scene.load_instances reads."""
    import scipy.io
    from PIL import Image
    rng = np.random.RandomState(3)
    for sub in ('sketches', 'inner_masks', 'seg_data'):
        os.makedirs(os.path.join(base, sub))
    sk = np.full((S, S, 3), 255, np.uint8)
    sk[rng.rand(S, S) < 0.4] = 0
    Image.fromarray(sk).save(os.path.join(base, 'sketches', '7.png'))
    scipy.io.savemat(os.path.join(base, 'inner_masks', '7.mat'), {'inner_masks': np.zeros((S, S), np.uint8)})
    boxes = np.array([[4, 6, 29, 39], [34, 20, 59, 61]], np.int32)
    masks = np.empty(2, dtype=object)
    masks[0], masks[1] = np.ones((26, 34), np.uint8), np.ones((26, 42), np.uint8)
    np.savez(os.path.join(base, 'seg_data', '7_datas.npz'), pred_boxes=boxes, pred_masks=masks, pred_class_ids=np.array([1, 2]))
    return base


def test_use_attn_through_the_command_line(tmp_path):
    """Fresh child processes on the small configuration: 3 iterations with the attention, what the snapshot holds, a run stopped at
    2 and resumed to the uninterrupted run's bytes, --mode match with its "attention", and the refusal without the flag."""
    from sketchyscenecolorization_amd import tf_checkpoint
    m = M()
    cfg = m.MatchConfig(use_attn=True, **dict(SMALL, **NARROW))
    backbone = str(tmp_path / 'backbone-1')
    tf_checkpoint.write_checkpoint(backbone, {k: a for k, a in m.random_variables(cfg, 31).items() if k.startswith('ResNet/')})
    flags = EO.write_split(str(tmp_path), 'train')[:4]
    common = ['--mode', 'train', '--use_attn', '1', '--backbone_snapshot', backbone, '--vocab_file', VOCAB, '--scene_size', '64',
              '--save_model_freq', '2', '--log_freq', '1', '--seed', '5'] + flags

    def run(tag, iterations):
        root = str(tmp_path / tag)
        return root, _child(common + ['--snapshot_root', root, '--log_root', root + '_log', '--max_iteration', str(iterations)], str(tmp_path), True)
    whole, printed = run('whole', 3)
    final = os.path.join(whole, 'deeplab_RMI_iter_3.tfmodel')
    assert printed.strip().split('\n')[-1] == 'model saved to ' + final
    tensors = tf_checkpoint.read_checkpoint(final)
    fresh = T().init_head(cfg, 5)
    for name, shape in ((DW, (40, 1)), (B, (1,))):
        assert tensors[name].shape == tensors[name + '/Adam'].shape == tensors[name + '/Adam_1'].shape == shape, name
    assert np.abs(tensors[DW] - fresh[DW]).max() > 0 and np.abs(tensors[DW + '/Adam']).max() > 0 and int(tensors['Variable']) == 3
    for name in cfg.variable_shapes():
        assert name in tensors and (not name.startswith(TO.P) or name + '/Adam' in tensors), name
    parts, _ = run('parts', 2)
    _, printed2 = run('parts', 3)
    assert 'start_iter 2' in printed2
    a = open(final + '.data-00000-of-00001', 'rb').read()
    b = open(os.path.join(parts, 'deeplab_RMI_iter_3.tfmodel.data-00000-of-00001'), 'rb').read()
    assert len(a) > 0 and a == b
    # --mode match reads it and writes the T weights
    scene = _scene_dir(str(tmp_path / 'scene'))
    match = ['--snapshot', whole, '--vocab_file', VOCAB, '--scene_size', '64', '--scene_dir', scene, '--image_id', '7',
             '--instruction', 'the bus on the left', '--results_dir', str(tmp_path / 'results')]
    out = _child(match + ['--use_attn', '1'], str(tmp_path), True)
    assert 'matched_inst_indices' in out
    record = json.load(open(str(tmp_path / 'results' / '7' / 'match.json')))
    attn = record['attention']
    assert len(attn) == T15 and record['seq_len'] == 5 and all(a > 0 for a in attn) and abs(sum(attn) - 1) <= 1e-6
    assert len(set(attn[5:])) == 1 and sum(attn[:5]) < 1
    # the same snapshot without the flag: refused, naming the variable and the flag
    err = _child(match, str(tmp_path), False, ok=False)
    assert 'ValueError' in err and 'attn_fc/DW' in err and '--use_attn 1' in err


# ------------------------------------------------------------------ with the flag off: the parent commit's bits
def test_flag_off_gives_the_parents_bits():
    """profiles/match_attn_parity.txt keeps the digests scripts/match_attn_digest.py printed on the parent commit's tree (one
    head pass at L = 15 and at L = 3, two steps, the snapshot's bytes): this tree's are the same."""
    sys.path.insert(0, os.path.join(ROOT, 'scripts'))
    try:
        import match_attn_digest
    finally:
        sys.path.pop(0)
    want = {}
    for line in open(PARITY):
        part = line.rstrip('\n').split(' ', 3)
        if len(part) == 4 and part[0] == 'parent' and part[1] == 'sha256':
            want[part[3]] = part[2]
    got = dict(match_attn_digest.digests())
    assert len(want) >= 9 and set(got) == set(want), set(got) ^ set(want)
    for what, sha in got.items():
        print('%s: %s' % (what, sha))
        assert sha == want[what], what
