"""The MRU pointwise / per-sample reduction kernels (csrc/mru_ops.hip) one by one against plain torch restatements
(float64 on the CPU) of the expressions in Foreground_Instance_Colorization/obj_lib/mru.py:15-28, 405-422, 560-591 and
models_collection.py:56-65.  Every op runs at a channel count that takes the 16-byte forms (`*_v4`, C % 4 == 0) and at one
that takes the scalar forms (C = 6): the two code paths must agree with the same reference."""
import pytest
import torch

from kernel_check import check

pytestmark = pytest.mark.gpu

TOL = 2e-5


def _hip():
    from sketchyscenecolorization_amd import hip
    hip.lib()
    return hip


def rnd(*shape, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g, dtype=torch.float32)


def close(a, b, tol=TOL):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    err = float((a - b).abs().max()) / max(1.0, float(b.abs().max()))
    assert err < tol, err


def miu(v):
    return 0.5 * (v + torch.sqrt(0.09 + v * v))


def up2(x):      # nearest 2x upsample of NHWC
    return x.repeat_interleave(2, dim=1).repeat_interleave(2, dim=2)


def minmax(x):   # [N,H,W,C] -> [N,2,C]
    return torch.stack([x.amin(dim=(1, 2)), x.amax(dim=(1, 2))], 1).contiguous()


def norm01(g, mm):
    mn, mx = mm[:, 0][:, None, None, :], mm[:, 1][:, None, None, :]
    return (g - mn) / (mx - mn)


# 16-byte form with one group per row, scalar form, 16-byte form with 9 groups, 65 groups (no power of two; the reductions'
# second workgroup along the channels holds one group)
CS = [8, 6, 36, 260]


@pytest.mark.parametrize('C', CS)
def test_pools_and_minmax(C):
    hip = _hip()
    N, H, W = 3, 10, 6
    x = rnd(N, H, W, C, seed=1)
    ref = 0.25 * (x[:, 0::2, 0::2] + x[:, 1::2, 0::2] + x[:, 0::2, 1::2] + x[:, 1::2, 1::2])
    xd = x.cuda()
    out = torch.full((N, H // 2, W // 2, C), float('nan'), device='cuda')
    hip.call('ssc_mean_pool2', xd, C, out, C, N, H, W, C)
    close(out, ref)
    # pool2: scale and accumulate, a channel slice of a wider source into a wider destination
    wide = rnd(N, H, W, C + 4, seed=2).cuda()
    dst = rnd(N, H // 2, W // 2, C + 8, seed=3).cuda()
    ref2 = dst.cpu().clone()
    ref2[..., :C] += 4.0 * 0.5 * (wide.cpu()[..., :C][:, 0::2, 0::2] + wide.cpu()[..., :C][:, 1::2, 0::2] +
                                  wide.cpu()[..., :C][:, 0::2, 1::2] + wide.cpu()[..., :C][:, 1::2, 1::2]) / 4.0
    hip.call('ssc_pool2', wide, C + 4, dst, C + 8, N, H, W, C, 0.5, 1)
    close(dst, ref2)
    mm = torch.empty(N, 2, C, device='cuda')
    hip.minmax_hw(xd, mm)
    assert torch.equal(mm.cpu(), minmax(x))


@pytest.mark.parametrize('C', CS)
def test_concat_parts_forms(C):
    """[gate * up(ht) | image (3 of 4) | act(a[n]*skip + b[n])]: upsample, min-max gate, the 3-channel part that shifts everything
    behind it off the 16-byte grid, per-sample norm tables + miu_relu; then the prelu and the plain single-part forms."""
    hip = _hip()
    N, H, W = 2, 8, 6
    ht, z, skip, rg = rnd(N, H // 2, W // 2, C, seed=4), rnd(N, H, W, 4, seed=5), rnd(N, H, W, C, seed=6), rnd(N, H, W, C, seed=7)
    abn = torch.cat([1.0 + 0.1 * rnd(N, C, seed=8), 0.2 * rnd(N, C, seed=9)], 1).contiguous()
    mm = minmax(rg)
    ct = 2 * C + 3
    ld = (ct + 3) // 4 * 4
    ref = torch.zeros(N, H, W, ld)
    ref[..., :C] = up2(ht) * norm01(rg, mm)
    ref[..., C:C + 3] = z[..., :3]
    a, b = abn[:, :C][:, None, None, :], abn[:, C:][:, None, None, :]
    ref[..., C + 3:ct] = miu(a * skip + b)
    out = torch.zeros(N, H, W, ld, device='cuda')
    hip.concat_parts(out, [dict(x=ht.cuda(), upsample=True, gate=(rg.cuda(), mm.cuda())), dict(x=z.cuda(), C=3),
                           dict(x=skip.cuda(), ab=abn.cuda(), act=hip.ACT_MIU)])
    close(out, ref)
    leak = torch.tensor([0.25])
    o2 = torch.empty(N, H, W, C, device='cuda')
    hip.concat_parts(o2, [dict(x=skip.cuda(), ab=leak.cuda(), act=hip.ACT_PRELU)])
    close(o2, torch.maximum(0.25 * skip, skip))


@pytest.mark.parametrize('C', CS)
@pytest.mark.parametrize('proj', [True, False])
def test_gate_merge_blend_and_their_backward(C, proj):
    hip = _hip()
    N, H, W = 2, 8, 6
    # ht_plus = ht + r * img (mru.py:422) and its backward
    ht, rg, img = (rnd(N, H, W, C, seed=s).double().requires_grad_(True) for s in (10, 11, 12))
    mm = minmax(rg.detach().float())
    r = norm01(rg, mm.double())
    htp = ht + r.detach() * img                  # the kernels take r as given: its gradient is the gate backward's business
    out = torch.empty(N, H, W, C, device='cuda')
    f = lambda t: t.detach().float().cuda()
    hip.call('ssc_mru_gate_merge', f(ht), f(rg), mm.cuda(), f(img), out, N, H * W, C)
    close(out, htp)
    g = rnd(N, H, W, C, seed=13)
    gr, gimg = torch.empty_like(out), torch.empty_like(out)
    hip.call('ssc_mru_gate_merge_backward', g.cuda(), f(rg), mm.cuda(), f(img), gr, gimg, N, H * W, C)
    close(gr, g.double() * img.detach())
    close(gimg, g.double() * r.detach())
    # the min-max gate's backward: r = (lrelu(pre) - min) / (max - min), reduce_min / reduce_max included
    pre = rnd(N, H, W, C, seed=14).double().requires_grad_(True)
    gv = torch.maximum(pre, 0.2 * pre)
    rr = (gv - gv.amin(dim=(1, 2), keepdim=True)) / (gv.amax(dim=(1, 2), keepdim=True) - gv.amin(dim=(1, 2), keepdim=True))
    (rr * g.double()).sum().backward()
    dpre = torch.empty_like(out)
    ws = hip.workspace()
    hip.call('ssc_minmax_gate_backward', f(gv), minmax(gv.detach().float()).cuda(), g.cuda(), N, H * W, C, dpre, ws,
             ws.numel() * 4)
    close(dpre, pre.grad, tol=2e-4)
    # blend (mru.py:583-589): out = hp * (1 - z) + h * z, ht at half resolution, with / without the projected + normed ht
    htl, h2, zg = rnd(N, H // 2, W // 2, C, seed=15), rnd(N, H, W, C, seed=16), rnd(N, H, W, C, seed=17)
    ab1 = torch.cat([1.0 + 0.1 * rnd(N, C, seed=18), 0.2 * rnd(N, C, seed=19)], 1).contiguous()
    ab2 = torch.cat([1.0 + 0.1 * rnd(N, C, seed=20), 0.2 * rnd(N, C, seed=21)], 1).contiguous()
    mz = minmax(zg)
    bc = lambda t, lo, hi: t[:, lo:hi][:, None, None, :]
    hp = up2(htl)
    if proj:
        hp = miu(bc(ab1, 0, C) * hp + bc(ab1, C, 2 * C))
    h = miu(bc(ab2, 0, C) * h2 + bc(ab2, C, 2 * C))
    zz = norm01(zg, mz)
    bo = torch.empty_like(out)
    hip.call('ssc_mru_blend', htl.cuda(), ab1.cuda() if proj else None, 1, h2.cuda(), ab2.cuda(), zg.cuda(), mz.cuda(), bo,
             N, H, W, C)
    close(bo, hp * (1 - zz) + h * zz)
    ghp, gh, gz = torch.empty_like(out), torch.empty_like(out), torch.empty_like(out)
    hip.call('ssc_mru_blend_backward', g.cuda(), htl.cuda(), ab1.cuda() if proj else None, 1, h2.cuda(), ab2.cuda(), zg.cuda(),
             mz.cuda(), ghp, gh, gz, N, H, W, C)
    close(ghp, g * (1 - zz))
    close(gh, g * zz)
    close(gz, g * (h - hp))
    # [r * up(ht) | ...] backward: gr = G * up(ht), G[:, :C] *= r in place
    ldG = C + 8
    G = rnd(N, H, W, ldG, seed=22)
    Gd = G.cuda()
    gr2 = torch.empty_like(out)
    hip.call('ssc_mru_in2_gate_backward', Gd, ldG, zg.cuda(), mz.cuda(), htl.cuda(), gr2, N, H, W, C)
    close(gr2, G[..., :C] * up2(htl))
    refG = G.clone()
    refG[..., :C] = G[..., :C] * zz
    close(Gd, refG)


@pytest.mark.parametrize('C', CS)
def test_prelu_backward_and_strided_copy(C):
    hip = _hip()
    M = 77
    x, gy = rnd(M, C + 2, seed=30), rnd(M, C + 4, seed=31)
    leak = torch.tensor([0.3])
    first = 0.3 * x[:, :C] >= x[:, :C]
    ref_dx = gy[:, :C] * torch.where(first, torch.tensor(0.3), torch.tensor(1.0))
    ref_dl = (gy[:, :C] * x[:, :C])[first].double().sum()
    dx = rnd(M, C, seed=32).cuda()
    base = dx.cpu().clone()
    dleak = torch.zeros(1, device='cuda')
    ws = hip.workspace()
    hip.call('ssc_prelu_backward', x.cuda(), C + 2, leak.cuda(), gy.cuda(), C + 4, M, C, dx, C, 1, dleak, 0, ws, ws.numel() * 4)
    close(dx, base + ref_dx)
    close(dleak, ref_dl.reshape(1), tol=2e-4)
    # a slice that starts at an odd column (a concat gradient behind the 3-channel image part), added to the destination
    src = rnd(M, 2 * C + 3, seed=33)
    dst = rnd(M, C, seed=34).cuda()
    ref = dst.cpu() + src[:, C + 3:]
    hip.call('ssc_strided_copy', src.cuda().view(-1)[C + 3:], 2 * C + 3, dst, C, M, C, 1)
    close(dst, ref)


@pytest.mark.parametrize('C', CS)
def test_cond_norm_backward(C):
    """Backward of y = miu_relu(cond_batchnorm(x)) (models_collection.py:22-35, 63-65): dx through the batch statistics and the
    per-class scale / offset table gradients, against autograd; gy is a channel slice of a wider gradient (row stride ldg)."""
    hip = _hip()
    N, P, L = 4, 35, 5
    x = rnd(N, P, C, seed=40).double().requires_grad_(True)
    scale_m = (1.0 + 0.1 * rnd(L, C, seed=41)).double().requires_grad_(True)
    offset_m = (0.2 * rnd(L, C, seed=42)).double().requires_grad_(True)
    labels = torch.tensor([1, 3, 1, 0], dtype=torch.int32)
    mean = x.mean(dim=(0, 1))
    var = ((x - mean) ** 2).mean(dim=(0, 1))
    rstd = torch.rsqrt(var + 1e-5)
    lab = labels.long()
    y = miu(scale_m[lab][:, None, :] * ((x - mean) * rstd) + offset_m[lab][:, None, :])
    gy = rnd(N, P, C + 3, seed=43)
    (y * gy[..., :C].double()).sum().backward()
    xd = x.detach().float().cuda()
    one, zero = torch.ones(C, device='cuda'), torch.zeros(C, device='cuda')
    ab0, st = torch.empty(2 * C, device='cuda'), torch.empty(2 * C, device='cuda')
    if C % 4 == 0:
        hip.bn_stats(xd.view(-1, C), one, zero, ab0, st)
    else:           # ssc_bn_stats takes multiples of 4 channels: the statistics from the reference
        st = torch.cat([mean.detach().float(), rstd.detach().float()]).cuda()
    abn = torch.empty(N, 2 * C, device='cuda')
    sm, om = scale_m.detach().float().cuda(), offset_m.detach().float().cuda()
    hip.call('ssc_cbn_fold', st, sm, om, labels.cuda(), N, C, abn)
    dx = torch.full((N, P, C), float('nan'), device='cuda')
    ds, do = torch.full((L, C), float('nan'), device='cuda'), torch.full((L, C), float('nan'), device='cuda')
    ws = hip.workspace()
    hip.call('ssc_cbn_act_backward', xd, abn, st, sm, labels.cuda(), L, gy.cuda(), C + 3, hip.ACT_MIU, N, P, C, dx, C, 0, ds, do,
             0, ws, ws.numel() * 4)
    close(dx, x.grad, tol=2e-4)
    close(ds, scale_m.grad, tol=2e-4)
    close(do, offset_m.grad, tol=2e-4)


# =====================================================================================================================
# The per-(sample, channel) reductions at sizes where their structure engages.  nsplit = min(64, ceil(P / 256)) row splits
# whose partial results a second kernel folds; the 16-byte forms put at most 64 channel groups (256 channels) in a
# workgroup, so C > 256 adds workgroups along the channels; the pointwise passes are grid-stride loops under a block cap.
#   P = 257    2 splits of 129 and 128 rows
#   P = 700    3 splits of 234, 234, 232 rows (no multiple of the row lanes)
#   P = 16640  65 -> the 64-split cap, 260 rows per split
#   C = 132    33 groups in one workgroup;  C = 260: 65 groups, the second workgroup holds one;  C = 512: two full ones
#   C = 6, 130 the scalar forms (one and three 64-channel chunks)
# =====================================================================================================================
FWD_TOL, RED_TOL = 2e-5, 2e-4
N2 = 2


def _nsplit(P):
    return min(64, (P + 255) // 256)


def _nan(*shape):
    return torch.full(shape, float('nan'), device='cuda')


@pytest.mark.parametrize('P,C,ld,off', [
    pytest.param(257, 8, 8, 0, id='P257-2splits-C8'),
    pytest.param(257, 6, 6, 0, id='P257-2splits-C6-scalar'),
    pytest.param(257, 6, 9, 2, id='P257-2splits-C6-scalar-ld9'),
    pytest.param(257, 512, 512, 0, id='P257-2splits-C512-2blocks'),
    pytest.param(700, 132, 132, 0, id='P700-3splits-C132-33groups'),
    pytest.param(700, 260, 272, 4, id='P700-3splits-C260-2ndblock1group-ld272'),
    pytest.param(16640, 8, 8, 0, id='P16640-64splitcap-C8'),
    pytest.param(16640, 8, 12, 4, id='P16640-64splitcap-C8-ld12'),
])
def test_minmax_hw_splits_blocks_and_row_stride(P, C, ld, off):
    """ssc_minmax_hw through its partial -> fold path (2, 3 and the capped 64 splits), with one and two workgroups along the
    channels, on a channel slice [off, off + C) of rows of stride ld: the bits of amin / amax."""
    hip = _hip()
    wide = rnd(N2, P, ld, seed=50)
    x = wide[..., off:off + C]
    ref = torch.stack([x.amin(1), x.amax(1)], 1)
    mm = _nan(N2, 2, C)
    ws = hip.workspace()
    hip.call('ssc_minmax_hw', wide.cuda().view(-1)[off:], ld, N2, P, C, mm, ws, ws.numel() * 4)
    assert torch.equal(mm.cpu(), ref), (P, C, ld, _nsplit(P))


@pytest.mark.parametrize('nsplit', [1, 3, 64])
@pytest.mark.parametrize('C', [6, 132])
def test_minmax_finalize_on_hand_built_partials(nsplit, C):
    """ssc_minmax_finalize alone on partial rows [N][nsplit][2][C] (the layout the conv epilogue and the partial kernels write):
    nsplit = 1 (nothing to fold), 3 (fewer splits than the fold's 8 thread groups), 64 (every group walks 8 splits); C = 132 is
    five 32-channel workgroups, the last one holding 4 channels.  Expected: the exact min of the min rows, max of the max rows."""
    hip = _hip()
    part = rnd(N2, nsplit, 2, C, seed=51)
    mm = _nan(N2, 2, C)
    hip.call('ssc_minmax_finalize', part.cuda(), nsplit, N2, C, mm)
    assert torch.equal(mm.cpu(), torch.stack([part[:, :, 0].amin(1), part[:, :, 1].amax(1)], 1))


def _lrelu_tf(pre):
    """tf.maximum(0.2 * x, x) with TensorFlow's gradient rule: the first argument (the leak branch) takes it where the two are
    equal, i.e. at x == 0 (torch.maximum would split it)."""
    return torch.where(pre > 0, pre, 0.2 * pre)


def _gate_backward_case(name, config, pre32, seed):
    """ssc_minmax_gate_backward on g = lrelu(pre) (fp32, as the conv epilogue stores it) and its exact extrema, against float64
    autograd through amin / amax of r = (g - min) / (max - min) (torch divides the gradient evenly over tied positions, as
    TensorFlow's reduce_min / reduce_max do)."""
    hip = _hip()
    N, P, C = pre32.shape
    gr = rnd(N, P, C, seed=seed)
    gv32 = _lrelu_tf(pre32)
    pre = pre32.double().requires_grad_(True)
    gv = _lrelu_tf(pre)
    mn, mx = gv.amin(1, keepdim=True), gv.amax(1, keepdim=True)
    assert bool((mx > mn).all()), 'a constant plane: the reference divides by zero too'
    (((gv - mn) / (mx - mn)) * gr.double()).sum().backward()
    mm = torch.stack([gv32.amin(1), gv32.amax(1)], 1).contiguous()
    dpre = _nan(N, P, C)
    ws = hip.workspace()
    hip.call('ssc_minmax_gate_backward', gv32.cuda(), mm.cuda(), gr.cuda(), N, P, C, dpre, ws, ws.numel() * 4)
    check(name, config, dpre, pre.grad, tol=RED_TOL, what='dpre')


GATE_SHAPES = [
    pytest.param(257, 8, id='P257-2splits-C8'),
    pytest.param(257, 6, id='P257-2splits-C6-scalar'),
    pytest.param(700, 132, id='P700-3splits-C132-33groups'),
    pytest.param(700, 260, id='P700-3splits-C260-2ndblock1group'),
    pytest.param(257, 512, id='P257-2splits-C512-2blocks'),
    pytest.param(16640, 8, id='P16640-64splitcap-C8'),
    pytest.param(16640, 260, id='P16640-64splitcap-C260-2blocks-applycap8192blocks'),
    pytest.param(16640, 130, id='P16640-64splitcap-C130-scalar-3chunks-applycap16384blocks'),
]


@pytest.mark.parametrize('P,C', GATE_SHAPES)
def test_minmax_gate_backward_splits_and_blocks(P, C):
    """Tie-free planes (randn) through the multi-split partial -> fold -> apply path; the two largest shapes also pass the
    block caps of the apply pass (N * P * C / 4 > 8192 * 256 groups in the 16-byte form, N * P * C > 16384 * 256 elements in
    the scalar form), so its grid-stride loop takes more than one trip."""
    _gate_backward_case('minmax_gate_backward', dict(P=P, C=C, nsplit=_nsplit(P)), rnd(N2, P, C, seed=60), 61)


def _tied_pre(P, C, shift, seed):
    """Pre-activations on a grid of 1/4, clamped to +-1.5 so that ~7 % of a plane sit on each end: many exactly tied minima and
    maxima (equal inputs give equal lrelu outputs in any arithmetic), and exact zeros, where lrelu's own tie rule applies."""
    return torch.clamp(torch.round(rnd(N2, P, C, seed=seed) * 4) / 4, -1.5, 1.5) + shift


@pytest.mark.parametrize('shift', [pytest.param(0.0, id='min-on-leak-branch'), pytest.param(-2.0, id='whole-plane-negative'),
                                   pytest.param(2.0, id='whole-plane-positive')])
@pytest.mark.parametrize('P,C', [
    pytest.param(257, 6, id='P257-2splits-C6-scalar'),
    pytest.param(257, 8, id='P257-2splits-C8'),
    pytest.param(700, 132, id='P700-3splits-C132-ties-across-splits'),
    pytest.param(700, 260, id='P700-3splits-C260-2ndblock-ties-across-splits'),
    pytest.param(16640, 8, id='P16640-64splitcap-C8-ties-across-splits'),
])
def test_minmax_gate_backward_tied_extrema(P, C, shift):
    """The TF tie rule: the gradient of reduce_min / reduce_max is divided evenly over every position that attains the extremum,
    the tie counts being summed (as floats) over the row splits.  Every plane has >= 2 tied minima and maxima; from P = 700 on
    the ties of a plane lie in different splits.  shift = 0: the minimum (-1.5 -> -0.3) is on the 0.2 leak branch, the maximum on
    the unit branch; -2: the whole plane is negative (both extrema on the leak branch); +2: the whole plane positive."""
    pre = _tied_pre(P, C, shift, 70)
    gv = _lrelu_tf(pre)                          # the fp32 gate the kernel is fed: the ties must have survived it
    tmin, tmax = gv == gv.amin(1, keepdim=True), gv == gv.amax(1, keepdim=True)
    assert int(tmin.sum(1).min()) >= 2 and int(tmax.sum(1).min()) >= 2
    gv64 = _lrelu_tf(pre.double())               # ... and be the reference's ties as well
    assert torch.equal(gv64 == gv64.amin(1, keepdim=True), tmin) and torch.equal(gv64 == gv64.amax(1, keepdim=True), tmax)
    if shift == 0.0:
        assert float(gv.amin()) < 0 < float(gv.amax()) and bool((pre == 0).any())
    else:
        assert bool((gv < 0).all()) if shift < 0 else bool((gv > 0).all())
    ns = _nsplit(P)
    if ns > 2:
        rows = -(-P // ns)
        split = (torch.arange(P) // rows)[None, :, None].expand_as(tmin)
        spread = lambda t: ((torch.where(t, split, ns).amin(1) != torch.where(t, split, -1).amax(1))).any()
        assert bool(spread(tmin)) and bool(spread(tmax)), 'no plane has its ties in different splits'
    _gate_backward_case('minmax_gate_backward_ties', dict(P=P, C=C, nsplit=ns, shift=shift), pre, 71)


@pytest.mark.parametrize('P,C', [
    pytest.param(257, 6, id='P257-2splits-C6-scalar'),
    pytest.param(257, 8, id='P257-2splits-C8'),
    pytest.param(700, 132, id='P700-3splits-C132-33groups'),
    pytest.param(700, 260, id='P700-3splits-C260-2ndblock1group'),
    pytest.param(257, 512, id='P257-2splits-C512-2blocks'),
    pytest.param(16640, 8, id='P16640-64splitcap-C8'),
])
def test_cond_norm_backward_splits_blocks_and_unused_labels(P, C):
    """ssc_cbn_act_backward through its multi-split partial -> fold path and with more than one workgroup along the channels:
    dx (written into the first C columns of rows of stride C + 4, the rest untouched) and both table gradients against
    float64 autograd; gy is a channel slice of a wider gradient.  Labels 0, 2 and 4 occur in no sample: their rows of both
    table gradients are exactly zero."""
    hip = _hip()
    N, L = 3, 5
    labels = torch.tensor([1, 3, 1], dtype=torch.int32)
    x = rnd(N, P, C, seed=80).double().requires_grad_(True)
    scale_m = (1.0 + 0.1 * rnd(L, C, seed=81)).double().requires_grad_(True)
    offset_m = (0.2 * rnd(L, C, seed=82)).double().requires_grad_(True)
    mean = x.mean(dim=(0, 1))
    rstd = torch.rsqrt(((x - mean) ** 2).mean(dim=(0, 1)) + 1e-5)
    lab = labels.long()
    y = miu(scale_m[lab][:, None, :] * ((x - mean) * rstd) + offset_m[lab][:, None, :])
    ldg, lddx = C + 4, C + 4
    gy = rnd(N, P, ldg, seed=83)
    (y * gy[..., :C].double()).sum().backward()
    xd = x.detach().float().cuda()
    st = torch.cat([mean.detach().float(), rstd.detach().float()]).cuda()
    if C % 4 == 0:          # (ssc_bn_stats takes multiples of 4 channels; C = 6 keeps the reference's statistics)
        hip.bn_stats(xd.view(-1, C), torch.ones(C, device='cuda'), torch.zeros(C, device='cuda'), torch.empty(2 * C, device='cuda'), st)
    sm, om = scale_m.detach().float().cuda(), offset_m.detach().float().cuda()
    abn = _nan(N, 2 * C)
    hip.call('ssc_cbn_fold', st, sm, om, labels.cuda(), N, C, abn)
    dx, ds, do = _nan(N, P, lddx), _nan(L, C), _nan(L, C)
    ws = hip.workspace()
    hip.call('ssc_cbn_act_backward', xd, abn, st, sm, labels.cuda(), L, gy.cuda(), ldg, hip.ACT_MIU, N, P, C, dx, lddx, 0, ds, do,
             0, ws, ws.numel() * 4)
    cfg = dict(P=P, C=C, nsplit=_nsplit(P))
    check('cbn_act_backward', cfg, dx[..., :C], x.grad, tol=RED_TOL, what='dx')
    assert bool(torch.isnan(dx[..., C:]).all()), 'columns past C of the dx rows were written'
    check('cbn_act_backward', cfg, ds, scale_m.grad, tol=RED_TOL, what='dscale')
    check('cbn_act_backward', cfg, do, offset_m.grad, tol=RED_TOL, what='doffset')
    unused = [0, 2, 4]
    assert bool((ds[unused] == 0).all()) and bool((do[unused] == 0).all())
    assert bool((scale_m.grad[unused] == 0).all())


@pytest.mark.parametrize('accumulate', [0, 1])
@pytest.mark.parametrize('M,C,ld', [
    pytest.param(2 * 257, 6, 8, id='M514-C6-ld8'),
    pytest.param(2 * 700, 132, 136, id='M1400-C132-ld136'),
    pytest.param(2 * 700, 260, 264, id='M1400-C260-ld264'),
    pytest.param(2 * 257, 512, 512, id='M514-C512'),
    pytest.param(2 * 16640, 8, 12, id='M33280-C8-ld12'),
])
def test_colsum_bias_gradients(M, C, ld, accumulate):
    """ssc_colsum (the bias gradients of every MRU conv): the first C columns of rows of stride ld, written or added."""
    hip = _hip()
    x = rnd(M, ld, seed=90)
    base = rnd(C, seed=91)
    out = base.cuda() if accumulate else _nan(C)
    ws = hip.workspace()
    hip.call('ssc_colsum', x.cuda(), ld, M, C, out, accumulate, ws, ws.numel() * 4)
    ref = x[:, :C].double().sum(0) + (base.double() if accumulate else 0.0)
    check('colsum', dict(M=M, C=C, ld=ld, accumulate=accumulate), out, ref, tol=RED_TOL)


@pytest.mark.parametrize('M,C', [
    pytest.param(9000, 64, id='M9000-C64-16byte-563blocks'),
    pytest.param(9000, 256, id='M9000-C256-16byte-2250blocks-cap2048-gridstride'),
    pytest.param(90000, 6, id='M90000-C6-scalar-2110blocks-cap2048-gridstride'),
])
def test_prelu_backward_grid_stride(M, C):
    """ssc_prelu_backward past its 2048-block cap (M * C > 2048 * 256 elements in the scalar form, M * C / 4 > 2048 * 256 groups
    in the 16-byte form): workgroups take more than one trip of the grid-stride loop and the leak gradient folds 2048 partial
    sums.  dx is added to its destination; x and gy are channel slices of wider rows."""
    hip = _hip()
    x, gy = rnd(M, C + 4, seed=95), rnd(M, C + 8, seed=96)
    leak = torch.tensor([0.3])
    first = 0.3 * x[:, :C] >= x[:, :C]
    ref_dx = gy[:, :C] * torch.where(first, torch.tensor(0.3), torch.tensor(1.0))
    ref_dl = (gy[:, :C] * x[:, :C])[first].double().sum()       # fp32 products (as TensorFlow forms them), summed in double
    base = rnd(M, C, seed=97)
    dx = base.cuda()
    dleak = _nan(1)
    ws = hip.workspace()
    hip.call('ssc_prelu_backward', x.cuda(), C + 4, leak.cuda(), gy.cuda(), C + 8, M, C, dx, C, 1, dleak, 0, ws, ws.numel() * 4)
    cfg = dict(M=M, C=C)
    check('prelu_backward', cfg, dx, base.double() + ref_dx.double(), tol=FWD_TOL, what='dx')
    check('prelu_backward', cfg, dleak, ref_dl.reshape(1), tol=RED_TOL, what='dleak')
