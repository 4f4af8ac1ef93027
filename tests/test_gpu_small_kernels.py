"""The loss, optimizer, spectral-norm and small dense-head kernels (csrc/losses_optim.hip) one by one against float64
references written from the oracle (oracle/tf_ops.py, oracle/pix2pix.py get_losses, oracle/residual.py bg_losses), at the sizes
where such kernels go wrong: below and far above every launch's block cap (so that every thread strides more than once), sizes
that are no multiple of 256 or 4, both sides of every optional pointer / flag, saturated inputs, and the argument checks.

Bounds (well-conditioned inputs): elementwise outputs and gradients 1e-5 * max(1, max|ref|); loss scalars 1e-5 relative;
reductions over more than 1e4 terms 1e-4.  Saturated inputs whose float32 formula loses digits by construction are bounded by
max(floor, 4 x the float32 oracle's own distance to float64) per element (kernel_check.check_fp32)."""
import math

import pytest
import torch

from kernel_check import NAN, acc, all_nan, check, check_fp32, check_scalar, hip, nan, randint, rc, rnd
from oracle import pix2pix as O
from oracle import residual as R
from oracle import tf_ops as T

pytestmark = pytest.mark.gpu


def _no_reg(p, scope):
    return 0.0


def _pix_parts(images, image_gens, real_logit, fake_logit, labels, real_disc, fake_disc):
    return O.get_losses({}, images, image_gens, labels, labels, real_disc, fake_disc, real_logit, fake_logit, reg=_no_reg)[2]


Z1 = torch.zeros(1, dtype=torch.float64)
L1 = torch.zeros(1, dtype=torch.int32)


# ------------------------------------------------------------------ ssc_softplus_loss (graph_single.py:401-402)
@pytest.mark.parametrize('rows', [100, 16384 + 37, 3 * 64 * 256 + 37])      # cap: 64 blocks of 256
@pytest.mark.parametrize('ld,sign,with_grad', [(1, 1.0, True), (4, -1.0, True), (4, 1.0, False)])
def test_softplus_loss(rows, ld, sign, with_grad):
    h = hip()
    cfg = dict(rows=rows, ld=ld, sign=sign, grad=with_grad)
    x = rnd(rows, ld, seed=1, std=3.0)
    x64 = x[:, 0].double().requires_grad_(True)
    scale, gscale = 1.0 / rows, 0.37
    # GAN_loss_g = mean softplus(-fake_disc), GAN_loss_d = mean softplus(fake) + mean softplus(-real)  (oracle get_losses)
    parts = _pix_parts(Z1, Z1, Z1.reshape(1, 1), Z1.reshape(1, 1), L1, Z1, -sign * x64)
    ref = parts['GAN_loss_g']
    (gscale * rows * ref).backward()
    a = acc(0.75, 7.0)
    grad = nan(rows, ld) if with_grad else None
    h.call('ssc_softplus_loss', x.cuda(), ld, rows, sign, scale, a[0:1], grad, gscale)
    check_scalar('softplus_loss', cfg, float(a[0]) - 0.75, ref)
    assert float(a[1]) == 7.0
    if with_grad:
        check('softplus_loss', cfg, grad[:, 0], x64.grad, what='grad')
        assert ld == 1 or all_nan(grad[:, 1:])       # only column 0 of a row is the patch logit


def test_softplus_loss_saturated():
    h = hip()
    x = torch.tensor([30.0, -30.0, 100.0, -100.0, 0.0, 88.0, -88.0, 17.0, -17.0, 104.0, -104.0])
    for sign in (1.0, -1.0):
        outs = {}
        for dt in (torch.float64, torch.float32):
            xs = x.detach().clone().to(dt).requires_grad_(True)
            loss = T.softplus(sign * xs)
            loss.sum().backward()
            outs[dt] = (loss.detach(), xs.grad)
        grad = nan(x.numel())
        per = []
        for i in range(x.numel()):           # one element per launch: the per-element loss
            a = acc(0.0)
            h.call('ssc_softplus_loss', x[i:i + 1].cuda(), 1, 1, sign, 1.0, a, grad[i:i + 1], 1.0)
            per.append(float(a[0]))
        cfg = dict(sign=sign, x='+-30,+-100')
        check_fp32('softplus_loss_saturated', cfg, torch.tensor(per), outs[torch.float64][0], outs[torch.float32][0], what='loss')
        check_fp32('softplus_loss_saturated', cfg, grad, outs[torch.float64][1], outs[torch.float32][1], what='grad')


# ------------------------------------------------------------------ ssc_acgan_loss (graph_single.py:340-353)
def _acgan_ref(logits, labels, focal, coef, dtype=torch.float64):
    z = logits.detach().clone().to(dtype).requires_grad_(True)
    parts = _pix_parts(Z1, Z1, z, z, labels, Z1, Z1)
    # the oracle's generator term carries its own 0.5 (loss_ac_g = 0.5 * mean CE); the discriminator term is the focal form
    loss = coef * (parts['ACGAN_loss_d'] if focal else parts['ACGAN_loss_g'] / 0.5)
    loss.backward()
    return loss.detach(), z.grad


@pytest.mark.parametrize('N,K', [(1, 25), (7, 1), (7, 3), (300, 25), (33, 64)])
@pytest.mark.parametrize('focal,with_grad', [(0, True), (1, True), (1, False)])
def test_acgan_loss(N, K, focal, with_grad):
    h = hip()
    cfg = dict(N=N, K=K, focal=focal, grad=with_grad)
    logits = rnd(N, K, seed=2, std=2.0)
    labels = randint(0, K, N, seed=3)
    coef = 0.5 * N          # gradients of order 1 whatever N is: the 1e-5 bound then sees every term
    ref, gref = _acgan_ref(logits, labels, focal, coef)
    a = acc(3.0, -2.0, 5.0)
    dl = nan(N, K) if with_grad else None
    h.call('ssc_acgan_loss', logits.cuda(), labels.cuda(), N, K, focal, coef, a[1:2], dl)
    if K > 1:
        check_scalar('acgan_loss', cfg, float(a[1]) + 2.0, ref)
    else:
        assert abs(float(a[1]) + 2.0) <= 1e-6 * coef       # one class: CE == 0
    assert float(a[0]) == 3.0 and float(a[2]) == 5.0
    if with_grad:
        check('acgan_loss', cfg, dl, gref, what='dlogits')


@pytest.mark.parametrize('focal', [0, 1])
def test_acgan_loss_saturated_and_clamped_labels(focal):
    h = hip()
    K = 25
    rows, labels = [], []
    for gap in (0.0, 20.0, 100.0, -20.0, -100.0):        # true logit above (+) / below (-) all the others by |gap|
        for t in (0, 7, K - 1):
            r = torch.zeros(K)
            r[t] = gap
            rows.append(r)
            labels.append(t)
    logits, labels = torch.stack(rows), torch.tensor(labels, dtype=torch.int32)
    N = logits.shape[0]
    cfg = dict(focal=focal, gaps='0,+-20,+-100')
    per = {}
    for dt in (torch.float64, torch.float32):
        ls, gs = [], []
        for i in range(N):
            l, g = _acgan_ref(logits[i:i + 1], labels[i:i + 1], focal, 1.0, dt)
            ls.append(l.reshape(()))
            gs.append(g[0])
        per[dt] = (torch.stack(ls), torch.stack(gs))
    got_l, got_g = [], nan(N, K)
    for i in range(N):
        a = acc(0.0)
        h.call('ssc_acgan_loss', logits[i:i + 1].cuda(), labels[i:i + 1].cuda(), 1, K, focal, 1.0, a, got_g[i:i + 1])
        got_l.append(float(a[0]))
    check_fp32('acgan_loss_saturated', cfg, torch.tensor(got_l), per[torch.float64][0], per[torch.float32][0], what='loss')
    check_fp32('acgan_loss_saturated', cfg, got_g, per[torch.float64][1], per[torch.float32][1], what='dlogits')
    # labels outside [0, K) are clamped: -1 behaves as 0, K as K - 1, bit for bit
    lg = rnd(4, K, seed=5).cuda()
    outs = []
    for lab in ([-1, K, -7, K + 9], [0, K - 1, 0, K - 1]):
        a, d = acc(0.0), nan(4, K)
        h.call('ssc_acgan_loss', lg, torch.tensor(lab, dtype=torch.int32).cuda(), 4, K, focal, 1.0, a, d)
        outs.append((float(a[0]), d.cpu()))
    assert math.isfinite(outs[0][0]) and torch.equal(outs[0][1], outs[1][1])
    assert abs(outs[0][0] - outs[1][0]) <= 1e-12 * abs(outs[1][0])      # the four atomic adds may arrive in another order


# ------------------------------------------------------------------ ssc_gen_output_grad (graph_single.py:551-555)
@pytest.mark.parametrize('npix', [100, 2 * 1024 * 256 + 37])     # cap: 1024 blocks of 256
@pytest.mark.parametrize('ldg,ldi,with_gd,with_dpre', [(3, 3, True, True), (4, 4, False, True), (4, 3, True, False)])
def test_gen_output_grad(npix, ldg, ldi, with_gd, with_dpre):
    h = hip()
    cfg = dict(npix=npix, ldg=ldg, ldi=ldi, gd=with_gd, dpre=with_dpre)
    gen = torch.tanh(rnd(npix, ldg, seed=6, std=1.5))
    img = torch.where(rnd(npix, ldi, seed=7) > 0.8, torch.sign(rnd(npix, ldi, seed=8)) * 0.99, torch.tanh(rnd(npix, ldi, seed=9)))
    gd = rnd(npix, 4, seed=10) if with_gd else None
    coef = 3.0 * npix * 0.5         # coef / (3 npix) = 0.5: the smooth-L1 gradient is of order 1 beside gd
    g64 = gen[:, :3].double().requires_grad_(True)
    smooth = _pix_parts(img[:, :3].double(), g64, Z1.reshape(1, 1), Z1.reshape(1, 1), L1, Z1, Z1)['l1_perceptual_loss']
    loss = coef * smooth
    (loss + ((gd[:, :3].double() * g64).sum() if with_gd else 0.0)).backward()
    dref = g64.grad * (1.0 - g64.detach() ** 2)         # through gen = tanh(pre)
    a = acc(1.0, 2.0, 3.0)
    dpre = nan(npix, 4) if with_dpre else None
    h.call('ssc_gen_output_grad', gen.cuda(), ldg, img.cuda(), ldi, gd.cuda() if with_gd else None, 4, npix, coef, a[1:2], dpre)
    check_scalar('gen_output_grad', cfg, float(a[1]) - 2.0, loss)
    assert float(a[0]) == 1.0 and float(a[2]) == 3.0
    if with_dpre:
        check('gen_output_grad', cfg, dpre[:, :3], dref, what='dpre')
        assert bool((dpre[:, 3] == 0).all())


# ------------------------------------------------------------------ ssc_l2_reg (mru.py:55,60)
@pytest.mark.parametrize('n', [100, 65536 + 1, 3 * 65536 + 5])       # cap: 256 blocks of 256
@pytest.mark.parametrize('with_grad,with_loss', [(True, True), (False, True), (True, False)])
def test_l2_reg(n, with_grad, with_loss):
    h = hip()
    cfg = dict(n=n, grad=with_grad, loss=with_loss)
    w = rnd(n, seed=11)
    w64 = w.double().requires_grad_(True)
    ref = O.regularization_loss({'s/fully_connected/weights': w64}, 's')       # rate 1e-6
    a = acc(0.5, 0.25)
    prior = rnd(n, seed=12)
    # the loss at the reference's rate; the gradient at rate 0.5 so that rate * w is of the order of what it is added to
    if with_loss:
        h.call('ssc_l2_reg', w.cuda(), n, 1e-6, a[0:1], None)
        check_scalar('l2_reg', cfg, float(a[0]) - 0.5, ref, tol=1e-4 if n > 10000 else 1e-5)
        assert float(a[1]) == 0.25
    if with_grad:
        (ref * (0.5 / 1e-6)).backward()
        g = prior.cuda()
        a2 = acc(0.0)
        h.call('ssc_l2_reg', w.cuda(), n, 0.5, a2 if with_loss else None, g)
        check('l2_reg', cfg, g, prior.double() + w64.grad, what='grad')
        if with_loss:
            check_scalar('l2_reg', cfg, float(a2[0]), ref.detach() * (0.5 / 1e-6), tol=1e-4 if n > 10000 else 1e-5, what='loss_rate_0.5')


# ------------------------------------------------------------------ ssc_bg_gan_loss (bg_colorization_main.py:596-627; oracle/residual.py:321-322)
def _bg_gan_ref(z, mode, dtype=torch.float64):
    zz = z.detach().clone().to(dtype).requires_grad_(True)
    p = torch.sigmoid(zz)
    per = -torch.log(p + R.BG_EPS) if mode == 0 else -torch.log(1 - p + R.BG_EPS)
    per.sum().backward()
    return per.detach(), zz.grad


@pytest.mark.parametrize('n', [100, 3 * 512 * 256 + 37])         # cap: 512 blocks of 256
@pytest.mark.parametrize('mode,with_dz', [(0, True), (1, True), (1, False)])
def test_bg_gan_loss(n, mode, with_dz):
    h = hip()
    cfg = dict(n=n, mode=mode, dz=with_dz)
    z = rnd(n, seed=13, std=2.0)
    per, gref = _bg_gan_ref(z, mode)
    a = acc(0.5, 0.25)
    dz = nan(n) if with_dz else None
    h.call('ssc_bg_gan_loss', z.cuda(), n, mode, 1.0 / n, a[1:2], dz, 0.7)
    check_scalar('bg_gan_loss', cfg, float(a[1]) - 0.25, per.mean())
    assert float(a[0]) == 0.5
    if with_dz:
        check('bg_gan_loss', cfg, dz, 0.7 * gref, what='dz')


def test_bg_gan_loss_is_the_oracle_discriminator_and_generator_loss():
    """discrim_loss = mode 0 on D(real) + mode 1 on D(fake) into one slot, gen_loss_GAN = mode 0 on D(fake): oracle bg_losses."""
    h = hip()
    n = 1000
    zr, zf = rnd(n, seed=14, std=2.0), rnd(n, seed=15, std=2.0)
    one = torch.zeros(1, 1, 1, 3, dtype=torch.float64)
    d_loss, _, parts = R.bg_losses(one, one, torch.sigmoid(zr.double()), torch.sigmoid(zf.double()), one + 1.0,
                                   torch.ones(1, 1, 1, dtype=torch.int32))
    a = acc(0.0, 0.0)
    h.call('ssc_bg_gan_loss', zr.cuda(), n, 0, 1.0 / n, a[0:1], None, 0.0)
    h.call('ssc_bg_gan_loss', zf.cuda(), n, 1, 1.0 / n, a[0:1], None, 0.0)
    h.call('ssc_bg_gan_loss', zf.cuda(), n, 0, 1.0 / n, a[1:2], None, 0.0)
    check_scalar('bg_gan_loss_oracle', dict(n=n), a[0], d_loss, what='discrim_loss')
    check_scalar('bg_gan_loss_oracle', dict(n=n), a[1], parts['gen_loss_GAN'], what='gen_loss_GAN')


@pytest.mark.parametrize('mode', [0, 1])
def test_bg_gan_loss_saturated(mode):
    h = hip()
    z = torch.tensor([5.0, -5.0, 20.0, -20.0, 100.0, -100.0, 0.0])
    (p64, g64), (p32, g32) = _bg_gan_ref(z, mode), _bg_gan_ref(z, mode, torch.float32)
    dz, per = nan(z.numel()), []
    for i in range(z.numel()):
        a = acc(0.0)
        h.call('ssc_bg_gan_loss', z[i:i + 1].cuda(), 1, mode, 1.0, a, dz[i:i + 1], 1.0)
        per.append(float(a[0]))
    cfg = dict(mode=mode, z='+-5,+-20,+-100')
    check_fp32('bg_gan_loss_saturated', cfg, torch.tensor(per), p64, p32, what='loss')
    check_fp32('bg_gan_loss_saturated', cfg, dz, g64, g32, what='dz')


# ------------------------------------------------------------------ ssc_count_nonzero_i32 / ssc_bg_output_grad (:612-616)
def test_count_nonzero_is_exact():
    h = hip()
    ws = h.workspace()
    M = 768 * 768 * 4        # the real size (batch 4 of 768^2); the float count is exact up to 2^24
    lab = torch.ones(M, dtype=torch.int32, device='cuda')
    cnt = nan(1)
    h.call('ssc_count_nonzero_i32', lab, M, cnt, ws, ws.numel() * 4)
    assert float(cnt[0]) == float(M)
    lab2 = randint(0, 3, 100003, seed=16)
    h.call('ssc_count_nonzero_i32', lab2.cuda(), lab2.numel(), cnt, ws, ws.numel() * 4)
    assert float(cnt[0]) == float((lab2 != 0).sum())
    cnt2 = nan(1)
    assert rc('ssc_count_nonzero_i32', lab, M, cnt2, ws, 256 * 4 - 1) == -2 and all_nan(cnt2)


@pytest.mark.parametrize('M', [100, 2 * 1024 * 256 + 37])        # cap: 1024 blocks of 256
@pytest.mark.parametrize('with_dgan', [True, False])
def test_bg_output_grad(M, with_dgan):
    h = hip()
    cfg = dict(M=M, dgan=with_dgan)
    img = torch.tanh(rnd(M, 3, seed=17))
    tgt = torch.tanh(rnd(M, 3, seed=18))
    tgt[5] = img[5]          # ties: |t - o| has gradient 0 there
    lab = randint(0, 3, M, seed=19)
    dgan = rnd(M, 4, seed=20) if with_dgan else None
    ws = h.workspace()
    cnt = nan(1)
    h.call('ssc_count_nonzero_i32', lab.cuda(), M, cnt, ws, ws.numel() * 4)
    l1w = 0.5 * 3.0 * float(cnt[0])      # l1w / (3 count) = 0.5: the L1 gradient is of order 1 beside dgan
    o64 = img.double().requires_grad_(True)
    logits = torch.zeros(1, M, 1, 3, dtype=torch.float64)
    half = torch.full((1,), 0.5, dtype=torch.float64)
    parts = R.bg_losses(o64.reshape(1, M, 1, 3), logits, half, half, tgt.double().reshape(1, M, 1, 3), lab.reshape(1, M, 1))[2]
    loss = l1w * parts['gen_loss_L1']
    (loss + ((dgan[:, :3].double() * o64).sum() if with_dgan else 0.0)).backward()
    dref = o64.grad * (1.0 - o64.detach() ** 2)
    a = acc(1.0, 2.0)
    dpre = nan(M, 4)
    h.call('ssc_bg_output_grad', img.cuda(), tgt.cuda(), lab.cuda(), cnt, l1w, dgan.cuda() if with_dgan else None, a[0:1], dpre, M)
    check_scalar('bg_output_grad', cfg, float(a[0]) - 1.0, loss)
    assert float(a[1]) == 2.0
    check('bg_output_grad', cfg, dpre[:, :3], dref, what='dpre')
    assert bool((dpre[:, 3] == 0).all())


# ------------------------------------------------------------------ ssc_seg_ce_loss (bg_colorization_main.py:589-591)
@pytest.mark.parametrize('M', [100, 2 * 1024 * 256 + 37])        # cap: 1024 blocks of 256
@pytest.mark.parametrize('K', [1, 2, 3, 4])
def test_seg_ce_loss(M, K):
    h = hip()
    cfg = dict(M=M, K=K)
    logits = rnd(M, K, seed=21, std=2.0)
    logits[:6] = 0.0
    for i, gap in enumerate((20.0, 100.0, -20.0, -100.0, 60.0, 0.0)):       # saturated rows: the label's logit +-gap off the others
        logits[i, 0] = gap
    lab = randint(0, K, M, seed=22)
    lab[:6] = 0
    w = 0.5 * M          # w / M = 0.5: gradients of order 1
    z = logits.double().requires_grad_(True)
    loss = w * T.sparse_softmax_ce(z, lab).mean()
    loss.backward()
    a = acc(1.0, 2.0)
    dl = nan(M, 4)
    h.call('ssc_seg_ce_loss', logits.cuda(), K, lab.cuda(), M, w, a[1:2], dl, 4)
    if K > 1:
        check_scalar('seg_ce_loss', cfg, float(a[1]) - 2.0, loss)
    else:
        assert abs(float(a[1]) - 2.0) <= 1e-6 * w
    assert float(a[0]) == 1.0
    check('seg_ce_loss', cfg, dl[:, :K], z.grad, what='dlogits')
    assert bool((dl[:, K:] == 0).all())          # pad columns


def test_seg_ce_loss_label_outside_the_logits_reads_nothing_and_answers_nan():
    """A label outside [0, K) (--seg_classes below the mask's class count) must not index the logits row: the kernel answers
    NaN for that row's loss and gradient, as tf.nn.sparse_softmax_cross_entropy_with_logits does on a GPU; every other row
    is untouched by it.  (The trainer refuses such a class count on the host: tests/test_host_logic.py.)"""
    h = hip()
    M, K = 64, 2
    logits = rnd(M, K, seed=23)
    lab = randint(0, K, M, seed=24)
    bad = [3, 17, 40]
    lab[3], lab[17], lab[40] = 2, -1, 1 << 30
    good = torch.ones(M, dtype=torch.bool)
    good[bad] = False
    z = logits.double().requires_grad_(True)
    (0.5 * M * T.sparse_softmax_ce(z[good], lab[good]).sum() / M).backward()
    a = acc(0.0, 2.0)
    dl = nan(M, 4)
    h.call('ssc_seg_ce_loss', logits.cuda(), K, lab.cuda(), M, 0.5 * M, a[0:1], dl, 4)
    assert math.isnan(float(a[0])) and float(a[1]) == 2.0
    assert all_nan(dl[bad][:, :K]) and bool((dl[:, K:] == 0).all())
    check('seg_ce_loss_bad_label', dict(M=M, K=K), dl[good][:, :K], z.grad[good], what='dlogits of the other rows')


# ------------------------------------------------------------------ ssc_adam_tf (graph_single.py:588)
@pytest.mark.parametrize('n', [4, 1028, 2048 * 256 * 4 * 2 + 8])     # cap: 2048 blocks of 256 threads x 4 elements
@pytest.mark.parametrize('with_m,lr_on_device', [(False, False), (True, True), (True, False), (False, True)])
def test_adam_tf(n, with_m, lr_on_device):
    h = hip()
    cfg = dict(n=n, m=with_m, lr_dev=lr_on_device)
    b1, b2, eps, lr, gscale = (0.5 if with_m else 0.0), 0.999, 1e-8, 0.1, 0.25
    w = rnd(n, seed=25)
    grads = [rnd(n, seed=26 + t, std=1.2) for t in range(3)]
    grads[1][::7] = 0.0
    w64, v64 = w.double(), torch.zeros(n, dtype=torch.float64)
    m64 = torch.zeros(n, dtype=torch.float64) if with_m else None
    wd, vd = w.cuda(), torch.zeros(n, device='cuda')
    md = torch.zeros(n, device='cuda') if with_m else None
    lr_dev = torch.zeros(1, device='cuda')
    for t, g in enumerate(grads, start=1):
        T.tf_adam_update(w64, gscale * g.double(), v64, t, lr, b1, b2, eps, m=m64)
        lr_t = lr * math.sqrt(1.0 - b2 ** t) / (1.0 - b1 ** t)
        lr_dev.fill_(lr_t)
        if lr_on_device:
            h.call('ssc_adam_tf', wd, g.cuda(), md, vd, n, NAN, lr_dev, b1, b2, eps, gscale)      # the argument is then ignored
        else:
            h.call('ssc_adam_tf', wd, g.cuda(), md, vd, n, lr_t, None, b1, b2, eps, gscale)
    check('adam_tf', cfg, wd, w64, what='var after 3 steps')
    check('adam_tf', cfg, vd, v64, what='v')
    if with_m:
        check('adam_tf', cfg, md, m64, what='m')


# ------------------------------------------------------------------ spectral norm (sn.py:12-52)
def _sn_ref(W, u, G):
    w64 = W.double().requires_grad_(True)
    u64 = u.double().reshape(1, -1)
    wbar, u_new = T.spectral_normed_weight(w64, u64)
    a = u64 @ w64.detach().t()
    v = T.sn_l2normalize(a)
    b = v @ w64.detach()
    aux = torch.stack([(v @ w64.detach() @ u_new.detach().t())[0, 0], (a * a).sum() ** 0.5, (b * b).sum() ** 0.5])
    (G.double() * wbar).sum().backward()
    return v.reshape(-1), u_new.detach().reshape(-1), wbar.detach(), aux, w64.grad


def _sn_inputs(m, n):
    W = rnd(m, n, seed=30, std=0.05)
    u = rnd(n, seed=31)
    G = rnd(m, n, seed=32) + 20.0 * W        # <G, W> far from 0: the terms through sigma and the power iteration count
    return W, u, G


def _sn_run(any_form, W, u, G, accumulate, prior):
    h = hip()
    m, n = W.shape
    Wd, ud, Gd = W.cuda(), u.cuda(), G.cuda()
    v, un, wbar, aux = nan(m), nan(n), nan(m, n), nan(3)
    dW = prior.cuda() if accumulate else nan(m, n)
    scratch = nan(m)
    if any_form:
        ws = nan(max(64 * n, 1024 + n))
        h.call('ssc_sn_forward_any', Wd, ud, m, n, v, un, wbar, aux, ws, ws.numel() * 4)
        h.call('ssc_sn_backward_any', Wd, ud, v, un, aux, Gd, m, n, dW, accumulate, scratch, ws, ws.numel() * 4)
    else:
        h.call('ssc_sn_forward', Wd, ud, m, n, v, un, wbar, aux)
        h.call('ssc_sn_backward', Wd, ud, v, un, aux, Gd, m, n, dW, accumulate, scratch)
    return v, un, wbar, aux, dW


SN_SMALL = [(64 * 16, 25), (512, 25), (3, 1), (300, 64)]
SN_ANY = SN_SMALL + [(6912, 768), (100, 65), (4 * 4 * 8, 200)]


@pytest.mark.parametrize('m,n', SN_ANY)
@pytest.mark.parametrize('accumulate', [0, 1])
def test_spectral_norm_forward_and_backward(m, n, accumulate):
    W, u, G = _sn_inputs(m, n)
    prior = rnd(m, n, seed=33)
    refs = _sn_ref(W, u, G)
    refs = refs[:4] + (refs[4] + (prior.double() if accumulate else 0.0),)
    names = ('v', 'u_new', 'wbar', 'aux', 'dW')
    outs = {}
    for any_form in ((False, True) if n <= 64 else (True,)):
        outs[any_form] = _sn_run(any_form, W, u, G, accumulate, prior)
        for name, got, ref in zip(names, outs[any_form], refs):
            check('sn_any' if any_form else 'sn', dict(m=m, n=n, accumulate=accumulate), got, ref, what=name)
    if len(outs) == 2:       # the one-workgroup form and the five-launch form claim the same math
        for name, a, b in zip(names, outs[False], outs[True]):
            check('sn_vs_sn_any', dict(m=m, n=n, accumulate=accumulate), a, b, what=name)


def test_spectral_norm_argument_checks():
    m, n = 10, 65
    W, u, G = _sn_inputs(m, n)
    Wd, ud, Gd = W.cuda(), u.cuda(), G.cuda()
    v, un, wbar, aux, dW, scratch = nan(m), nan(n), nan(m, n), nan(3), nan(m, n), nan(m)
    assert rc('ssc_sn_forward', Wd, ud, m, n, v, un, wbar, aux) == -1
    assert rc('ssc_sn_backward', Wd, ud, v, un, aux, Gd, m, n, dW, 0, scratch) == -1
    ws = nan(2048)
    assert rc('ssc_sn_forward_any', Wd, ud, m, n, v, un, wbar, aux, ws, n * 4 - 1) == -2         # nsplit = 1: n floats
    assert rc('ssc_sn_backward_any', Wd, ud, v, un, aux, Gd, m, n, dW, 0, scratch, ws, (1024 + n) * 4 - 1) == -2
    for t in (v, un, wbar, aux, dW, scratch, ws):
        assert all_nan(t)


# ------------------------------------------------------------------ ssc_fc_small_fwd / _bwd (models_collection.py:839)
@pytest.mark.parametrize('K', [1, 3, 31, 32, 33, 512])       # the unrolled-by-32 loop and its remainder loop
@pytest.mark.parametrize('J', [1, 25, 64])
def test_fc_small(K, J):
    h = hip()
    N = 5
    x, W, b, dy = rnd(N, K, seed=34), rnd(K, J, seed=35, std=0.3), rnd(J, seed=36), rnd(N, J, seed=37)
    x64, W64, b64 = (t.double().requires_grad_(True) for t in (x, W, b))
    y64 = x64 @ W64 + b64
    (y64 * dy.double()).sum().backward()
    xd, Wd, bd, dyd = x.cuda(), W.cuda(), b.cuda(), dy.cuda()
    cfg = dict(N=N, K=K, J=J)
    y = nan(N, J)
    h.call('ssc_fc_small_fwd', xd, Wd, bd, N, K, J, y)
    check('fc_small_fwd', cfg, y, y64, what='y')
    y0 = nan(N, J)
    h.call('ssc_fc_small_fwd', xd, Wd, None, N, K, J, y0)
    check('fc_small_fwd', cfg, y0, y64 - b64, what='y without bias')
    dx, dW, db = nan(N, K), nan(K, J), nan(J)
    h.call('ssc_fc_small_bwd', xd, Wd, dyd, N, K, J, dx, dW, db, 0)
    check('fc_small_bwd', cfg, dx, x64.grad, what='dx')
    check('fc_small_bwd', cfg, dW, W64.grad, what='dW')
    check('fc_small_bwd', cfg, db, b64.grad, what='db')
    pW, pb = rnd(K, J, seed=38), rnd(J, seed=39)
    dW2, db2 = pW.cuda(), pb.cuda()
    h.call('ssc_fc_small_bwd', xd, Wd, dyd, N, K, J, None, dW2, db2, 1)        # accumulate, no dx
    check('fc_small_bwd', cfg, dW2, pW.double() + W64.grad, what='dW accumulated')
    check('fc_small_bwd', cfg, db2, pb.double() + b64.grad, what='db accumulated')
    dW3 = nan(K, J)
    h.call('ssc_fc_small_bwd', xd, Wd, dyd, N, K, J, None, dW3, None, 0)          # no db
    check('fc_small_bwd', cfg, dW3, W64.grad, what='dW without db')


def test_argument_checks_of_the_loss_and_optimizer_kernels():
    """K > 64 (acgan), K > 4 (seg_ce), n & 3 (adam), J > 64 (fc_small): the documented non-zero code, nothing launched."""
    a = acc(0.0)
    dl = nan(2, 65)
    assert rc('ssc_acgan_loss', torch.zeros(2, 65, device='cuda'), torch.zeros(2, dtype=torch.int32, device='cuda'), 2, 65, 0, 1.0,
              a, dl) == -1 and all_nan(dl)
    dl = nan(8, 5)
    assert rc('ssc_seg_ce_loss', torch.zeros(8, 5, device='cuda'), 5, torch.zeros(8, dtype=torch.int32, device='cuda'), 8, 1.0, a,
              dl, 5) == -1 and all_nan(dl)
    assert float(a[0]) == 0.0
    w, v = nan(1026), nan(1026)
    assert rc('ssc_adam_tf', w, torch.ones(1026, device='cuda'), None, v, 1026, 0.1, None, 0.0, 0.9, 1e-8, 1.0) == -1
    assert all_nan(w) and all_nan(v)
    y = nan(2, 65)
    assert rc('ssc_fc_small_fwd', torch.ones(2, 8, device='cuda'), torch.ones(8, 65, device='cuda'), None, 2, 8, 65, y) == -1
    assert all_nan(y)
