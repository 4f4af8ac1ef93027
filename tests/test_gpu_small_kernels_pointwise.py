"""The pointwise / reduction kernels of the caption branch (csrc/text_lstm.hip), the elementwise helpers and the batch
statistics (csrc/elementwise.hip) one by one against float64 references written from the oracle (oracle/tf_ops.py), with the
rules of tests/test_gpu_small_kernels.py: elementwise 1e-5 * max(1, max|ref|), reductions over more than 1e4 terms 1e-4, and
max(floor, 4 x float32-oracle distance) per element where the float32 formula loses digits by construction.

The batch-statistics sweep (test_bn_stats_ill_conditioned*) measures mean, 1/std, the normalised output and dx on
x = mean + std * noise up to mean/std = 5000 against float64, and the float32 two-pass oracle (T.batchnorm, the stand-in for
tf.nn.moments in float32) against float64 on the same input; bound max(2e-4, 1.5 x that) relative to the output scale."""
import pytest
import torch

from kernel_check import all_nan, check, check_fp32, hip, nan, randint, rc, rnd
from conftest import parity_log
from oracle import tf_ops as T

pytestmark = pytest.mark.gpu

ACT = {0: lambda t: t, 1: torch.relu, 2: lambda t: T.lrelu(t, 0.2), 3: torch.tanh}


# ------------------------------------------------------------------ embedding (models_collection.py:182)
@pytest.mark.parametrize('C', [4, 512])
def test_embedding_gather_and_scatter_add(C):
    h = hip()
    vocab, rows = 58, 45
    table = rnd(vocab, C, seed=1)
    tok = randint(1, vocab, rows, seed=2)
    tok[::4] = 0                 # pad tokens
    tok[1], tok[2], tok[5], tok[6] = 7, 7, 7, vocab - 1        # repeated tokens, the last row of the table
    out = nan(rows, C)
    h.call('ssc_embedding_gather', table.cuda(), tok.cuda(), rows, C, out)
    assert torch.equal(out.cpu(), table[tok.long()])             # tf.nn.embedding_lookup: a copy
    # gradient: rows of pad tokens never reach the table (tf.cond skips the lookup's consumer, :235)
    g = rnd(rows, C, seed=3)
    t64 = table.double().requires_grad_(True)
    (t64[tok.long()] * (g.double() * (tok != 0).double().reshape(-1, 1))).sum().backward()
    prior = rnd(vocab, C, seed=4)
    runs = []
    for _ in range(2):
        d = prior.cuda()
        h.call('ssc_embedding_scatter_add', d, vocab, tok.cuda(), rows, C, g.cuda())
        runs.append(d.cpu())
    check('embedding_scatter_add', dict(C=C), runs[0], prior.double() + t64.grad, what='dtable')
    assert torch.equal(runs[0][0], prior[0])         # id 0 leaves row 0 untouched
    assert torch.equal(runs[0], runs[1])             # fixed summation order: bitwise run to run


# ------------------------------------------------------------------ row l2-normalise (:202,216)
@pytest.mark.parametrize('C', [4, 1024])
@pytest.mark.parametrize('pad,with_ab', [(0, False), (8, False), (8, True), (0, True)])
def test_row_l2norm(C, pad, with_ab):
    h = hip()
    M, ldx = 7, C + pad
    cfg = dict(C=C, ldx=ldx, ab=with_ab)
    xbuf = rnd(M, ldx, seed=5)
    xbuf[2, :C] = 0.0                # sum of squares 0: the clamped branch (without ab)
    xbuf[4, :C] *= 1e-8              # ... and below 1e-12 without being 0
    ab = torch.cat([1.0 + 0.1 * rnd(C, seed=6), 0.2 * rnd(C, seed=7)]) if with_ab else None
    x64 = xbuf[:, :C].double().requires_grad_(True)
    z64 = x64 * ab[:C].double() + ab[C:].double() if with_ab else x64
    if with_ab:
        z64.retain_grad()
    y64 = T.l2_normalize(z64, 1)
    dy = rnd(M, C, seed=8)
    (y64 * dy.double()).sum().backward()
    dz_ref = z64.grad if with_ab else x64.grad
    y, ss = nan(M, C), nan(M)
    h.call('ssc_row_l2norm_fwd', xbuf.cuda(), ldx, ab.cuda() if with_ab else None, M, C, y, ss)
    prior = rnd(M, C, seed=9)
    dz, dz_acc = nan(M, C), prior.cuda()
    h.call('ssc_row_l2norm_bwd', y, ss, dy.cuda(), M, C, dz, 0)
    h.call('ssc_row_l2norm_bwd', y, ss, dy.cuda(), M, C, dz_acc, 1)
    check('row_l2norm', cfg, ss, (z64.detach() ** 2).sum(1), what='ss')
    # the rows whose sum of squares is clamped have 1/sqrt(1e-12) = 1e6 as their scale: compared apart from the ordinary ones
    small = (z64.detach() ** 2).sum(1) < 1e-12
    assert with_ab or int(small.sum()) == 2
    for rows, tag in ((~small, ''), (small, ' (clamped rows)')):
        if int(rows.sum()):
            check('row_l2norm', cfg, y[rows], y64[rows], what='y' + tag)
            check('row_l2norm', cfg, dz[rows], dz_ref[rows], what='dz' + tag)
            check('row_l2norm', cfg, dz_acc[rows], prior.double()[rows] + dz_ref[rows], what='dz accumulated' + tag)


def test_caption_kernels_argument_checks():
    o = nan(4, 6)
    x = torch.ones(4, 8, device='cuda')
    tok = torch.zeros(4, dtype=torch.int32, device='cuda')
    assert rc('ssc_embedding_gather', x, tok, 4, 6, o) == -1 and all_nan(o)
    ss = nan(4)
    assert rc('ssc_row_l2norm_fwd', x, 8, None, 4, 6, o, ss) == -1 and all_nan(o) and all_nan(ss)
    assert rc('ssc_row_l2norm_fwd', x, 6, None, 4, 4, o, ss) == -1 and all_nan(o)       # ldx & 3
    assert rc('ssc_row_l2norm_bwd', x, torch.ones(4, device='cuda'), x, 4, 6, o, 0) == -1 and all_nan(o)


# ------------------------------------------------------------------ BasicLSTMCell gate math (:230-236)
@pytest.mark.parametrize('N,div,C', [(5, 1, 8), (2, 36, 130)])           # rows = N * div; div2 = mdiv = div
@pytest.mark.parametrize('with_g1,with_g2,with_gacc', [(True, True, True), (False, False, False), (False, True, False)])
def test_lstm_pointwise(N, div, C, with_g1, with_g2, with_gacc):
    h = hip()
    rows = N * div
    cfg = dict(rows=rows, div=div, C=C, g1=with_g1, g2=with_g2, gacc=with_gacc)
    g0, g1, g2 = rnd(rows, 4 * C, seed=10), rnd(rows, 4 * C, seed=11), rnd(N, 4 * C, seed=12)
    c_in, h_in = rnd(rows, C, seed=13), torch.tanh(rnd(rows, C, seed=14))
    mask = torch.ones(N, dtype=torch.int32)
    mask[::2] = 0                # skipped steps (pad tokens)
    dh, dc = rnd(rows, C, seed=15), rnd(rows, C, seed=16)
    live = mask.bool().repeat_interleave(div)
    gates = g0.double()
    if with_g1:
        gates = gates + g1.double()
    if with_g2:
        gates = gates + g2.double().repeat_interleave(div, 0)
    gates = gates.requires_grad_(True)
    c64, h64 = c_in.double().requires_grad_(True), h_in.double().requires_grad_(True)
    # the oracle's cell with the gate pre-activations handed in: kernel = [I; 0] makes [x, h] @ kernel + 0 the gates themselves
    kern = torch.cat([torch.eye(4 * C, dtype=torch.float64), torch.zeros(C, 4 * C, dtype=torch.float64)])
    h1, state = T.basic_lstm_cell(gates, torch.cat([c64, h64], 1), kern, torch.zeros(4 * C, dtype=torch.float64))
    c1 = state[:, :C]
    lv = live.reshape(-1, 1)
    c_ref, h_ref = torch.where(lv, c1, c64), torch.where(lv, h1, h64)        # tf.cond: a pad token copies the state through
    ((h_ref * dh.double()).sum() + (c_ref * dc.double()).sum()).backward()
    gd = gates.detach()
    acts_ref = torch.cat([torch.sigmoid(gd[:, :C]), torch.tanh(gd[:, C:2 * C]), torch.sigmoid(gd[:, 2 * C:3 * C] + 1.0),
                          torch.sigmoid(gd[:, 3 * C:])], 1)
    c_out, h_out, acts = nan(rows, C), nan(rows, C), nan(rows, 4 * C)
    md = mask.cuda()
    h.call('ssc_lstm_pointwise_fwd', g0.cuda(), g1.cuda() if with_g1 else None, g2.cuda() if with_g2 else None, div, md, div,
           c_in.cuda(), h_in.cuda(), rows, C, c_out, h_out, acts)
    check('lstm_pointwise_fwd', cfg, c_out, c_ref, what='c_out')
    check('lstm_pointwise_fwd', cfg, h_out, h_ref, what='h_out')
    check('lstm_pointwise_fwd', cfg, acts[live], acts_ref[live], what='acts')
    assert all_nan(acts[~live])          # never written (nor read) for skipped steps
    dg, dc_in, dh_pass = nan(rows, 4 * C), nan(rows, C), nan(rows, C)
    prior = rnd(rows, 4 * C, seed=17)
    gacc = prior.cuda() if with_gacc else None
    h.call('ssc_lstm_pointwise_bwd', dh.cuda(), dc.cuda(), acts, c_in.cuda(), c_out, md, div, rows, C, dg, dc_in, dh_pass, gacc)
    check('lstm_pointwise_bwd', cfg, dg, gates.grad, what='dg')
    check('lstm_pointwise_bwd', cfg, dc_in, c64.grad, what='dc_in')
    check('lstm_pointwise_bwd', cfg, dh_pass, h64.grad, what='dh_pass')
    if with_gacc:
        check('lstm_pointwise_bwd', cfg, gacc, prior.double() + gates.grad, what='gacc')


# ------------------------------------------------------------------ squash (:238-242; oracle/pix2pix.py:150-151)
def _squash(hh):
    return torch.relu((torch.log(1.0 + 1e-3 + hh) - torch.log(1.0 + 1e-3 - hh)) * 0.5)


def test_squash():
    h = hip()
    n = 1000 + 11
    hv = torch.tanh(rnd(n, seed=18, std=1.5))
    edge = torch.tensor([0.0, 0.5, -0.5, 0.999, -0.999, 1.0, -1.0])          # the LSTM output range, ends included
    hv[:edge.numel()] = edge
    go = rnd(n, seed=19)
    refs = {}
    for dt in (torch.float64, torch.float32):
        x = hv.detach().clone().to(dt).requires_grad_(True)
        o = _squash(x)
        (o * go.to(dt)).sum().backward()
        refs[dt] = (o.detach(), x.grad)
    o, dh = nan(n), nan(n)
    h.call('ssc_squash_fwd', hv.cuda(), n, o)
    h.call('ssc_squash_bwd', hv.cuda(), o, go.cuda(), n, dh)
    check_fp32('squash', dict(n=n), o, refs[torch.float64][0], refs[torch.float32][0], what='o')
    check_fp32('squash', dict(n=n), dh, refs[torch.float64][1], refs[torch.float32][1], what='dh')


# ------------------------------------------------------------------ small reductions
@pytest.mark.parametrize('groups,G,C,pad', [(300, 1, 130, 0), (1, 300, 3, 5), (7, 36, 130, 6), (2, 20001, 64, 4)])
@pytest.mark.parametrize('accumulate', [0, 1])
def test_group_rowsum(groups, G, C, pad, accumulate):
    h = hip()
    ldx = C + pad
    x = rnd(groups * G, ldx, seed=20)
    prior = rnd(groups, C, seed=21)
    ref = x[:, :C].double().reshape(groups, G, C).sum(1) + (prior.double() if accumulate else 0.0)
    out = prior.cuda() if accumulate else nan(groups, C)
    h.call('ssc_group_rowsum', x.cuda(), ldx, groups, G, C, out, accumulate)
    check('group_rowsum', dict(groups=groups, G=G, C=C, ldx=ldx, accumulate=accumulate), out, ref, tol=1e-4 if G > 10000 else 1e-5)


@pytest.mark.parametrize('P', [1, 29, 32, 36, 577])      # the unrolled-by-32 loop and its remainder loop
@pytest.mark.parametrize('C', [3, 64, 130])
@pytest.mark.parametrize('act,with_ab', [(0, False), (1, True), (2, True), (2, False)])
def test_act_mean_hw(P, C, act, with_ab):
    h = hip()
    N = 2
    x = rnd(N, P, C, seed=22)
    ab = torch.cat([1.0 + 0.2 * rnd(C, seed=23), 0.3 * rnd(C, seed=24)]) if with_ab else None
    z = x.double() * ab[:C].double() + ab[C:].double() if with_ab else x.double()
    out = nan(N, C)
    h.call('ssc_act_mean_hw', x.cuda(), ab.cuda() if with_ab else None, act, N, P, C, out)
    check('act_mean_hw', dict(P=P, C=C, act=act, ab=with_ab), out, ACT[act](z).mean(1))


def test_act_mean_hw_long_reduction():
    h = hip()
    N, P, C = 2, 20003, 64
    x = rnd(N, P, C, seed=25)
    out = nan(N, C)
    h.call('ssc_act_mean_hw', x.cuda(), None, 2, N, P, C, out)
    check('act_mean_hw', dict(P=P, C=C, act=2, ab=False), out, T.lrelu(x.double(), 0.2).mean(1), tol=1e-4)


@pytest.mark.parametrize('N,P,C,offset', [(2, 9, 512, 0), (3, 7, 6, 0), (2, 9, 8, 1), (2, 8300, 512, 0)])
def test_add_row_bcast(N, P, C, offset):
    """C = 512: the float4 path (the last case far above its 4096-block cap); C = 6 and a `v` sliced to a 4-byte offset: the
    scalar path."""
    h = hip()
    g = rnd(N, P, C, seed=26)
    vbuf = rnd(N * C + offset, seed=27)
    v = vbuf[offset:].reshape(N, C)
    ref = g.double() + 0.37 * v.double().reshape(N, 1, C)
    gd = g.cuda()
    vd = vbuf.cuda()[offset:]
    assert (vd.data_ptr() % 16 == 0) == (offset == 0)
    h.call('ssc_add_row_bcast', gd, vd, 0.37, N, P, C)
    check('add_row_bcast', dict(N=N, P=P, C=C, offset=offset), gd, ref)


# ------------------------------------------------------------------ noise head (:63-65, 493-499)
def test_miu_permute():
    h = hip()
    N, Cc, P = 2, 5, 37          # Cc * P = 185: no multiple of 256
    pre = rnd(N, Cc * P, seed=28, std=2.0)
    edge = torch.tensor([-100.0, -30.0, -3.0, -0.3, 0.0, 0.3, 3.0, 30.0, 100.0])
    pre[0, :edge.numel()] = edge
    pre[1, -edge.numel():] = edge
    g = rnd(N, P, Cc, seed=29)
    refs = {}
    for dt in (torch.float64, torch.float32):
        x = pre.detach().clone().to(dt).requires_grad_(True)
        o = T.miu_relu(x).reshape(N, Cc, P).permute(0, 2, 1)
        (o * g.to(dt)).sum().backward()
        refs[dt] = (o.detach().contiguous(), x.grad)
    out, dpre = nan(N, P, Cc), nan(N, Cc * P)
    h.call('ssc_miu_permute_fwd', pre.cuda(), N, Cc, P, out)
    h.call('ssc_miu_permute_bwd', pre.cuda(), g.cuda(), N, Cc, P, dpre)
    check_fp32('miu_permute', dict(N=N, Cc=Cc, P=P), out, refs[torch.float64][0], refs[torch.float32][0], what='out')
    check_fp32('miu_permute', dict(N=N, Cc=Cc, P=P), dpre, refs[torch.float64][1], refs[torch.float32][1], what='dpre')


# ------------------------------------------------------------------ elementwise helpers
@pytest.mark.parametrize('M,C', [(100, 3), (100, 130), (33000, 130)])        # the last: every thread of the 8192-block cap strides
@pytest.mark.parametrize('act', [0, 1, 2, 3])
@pytest.mark.parametrize('with_ab', [True, False])
def test_affine_act(M, C, act, with_ab):
    h = hip()
    ldx, ldo, ldab = C + 5, C + 2, C + 3
    x = rnd(M, ldx, seed=30, std=1.5)
    ab = torch.cat([1.0 + 0.2 * rnd(ldab, seed=31), 0.3 * rnd(ldab, seed=32)]) if with_ab else None
    z = x[:, :C].double()
    if with_ab:
        z = z * ab[:C].double() + ab[ldab:ldab + C].double()
    out = nan(M, ldo)
    h.call('ssc_affine_act', x.cuda(), ldx, ab.cuda() if with_ab else None, ldab, act, out, ldo, M, C)
    check('affine_act', dict(M=M, C=C, act=act, ab=with_ab), out[:, :C], ACT[act](z))
    assert all_nan(out[:, C:])           # the pad columns of the output rows are not written


@pytest.mark.parametrize('M,C', [(100, 4), (100, 132), (130000, 132)])      # the last: every thread of the 8192-block cap strides
@pytest.mark.parametrize('act', [0, 1, 2, 3])
@pytest.mark.parametrize('with_ab2', [True, False])
def test_residual_merge(M, C, act, with_ab2):
    """residual_util.py:103-109, 138-146, 165-167.  The kernel works on float4 channel groups: C = 3 and C = 130 are refused
    (test_elementwise_argument_checks), the odd sizes here are 4 and 132."""
    h = hip()
    x1, x2 = rnd(M, C, seed=33), rnd(M, C, seed=34)
    ab1 = torch.cat([1.0 + 0.2 * rnd(C, seed=35), 0.3 * rnd(C, seed=36)])
    ab2 = torch.cat([1.0 + 0.2 * rnd(C, seed=37), 0.3 * rnd(C, seed=38)]) if with_ab2 else None
    s = x1.double() * ab1[:C].double() + ab1[C:].double()
    s = s + (x2.double() * ab2[:C].double() + ab2[C:].double() if with_ab2 else x2.double())
    out = nan(M, C)
    h.call('ssc_residual_merge', x1.cuda(), ab1.cuda(), x2.cuda(), ab2.cuda() if with_ab2 else None, act, out, M, C)
    check('residual_merge', dict(M=M, C=C, act=act, ab2=with_ab2), out, ACT[act](s))


@pytest.mark.parametrize('M,C,ld', [(100, 3, 4), (100, 130, 136), (70001, 130, 132), (70001, 64, 64)])
@pytest.mark.parametrize('accumulate', [0, 1])
def test_colsum(M, C, ld, accumulate):
    h = hip()
    x = rnd(M, ld, seed=39)
    prior = rnd(C, seed=40)
    out = prior.cuda() if accumulate else nan(C)
    ws = h.workspace()
    h.call('ssc_colsum', x.cuda(), ld, M, C, out, accumulate, ws, ws.numel() * 4)
    ref = x[:, :C].double().sum(0) + (prior.double() if accumulate else 0.0)
    check('colsum', dict(M=M, C=C, ld=ld, accumulate=accumulate), out, ref, tol=1e-4 if M > 10000 else 1e-5)


@pytest.mark.parametrize('nblk,C', [(3, 5), (600, 64)])      # 600 rows: the four-wavefronts-per-channel fold
def test_bn_finalize(nblk, C):
    """Rows of partial column sums / sums of squares -> the folded norm of T.batchnorm."""
    h = hip()
    rows = 8
    x = rnd(nblk * rows, C, seed=41) * 2.0 + 0.5
    scale, offset = 1.0 + 0.1 * rnd(C, seed=42), 0.1 * rnd(C, seed=43)
    xb = x.double().reshape(nblk, rows, C)
    partial = torch.stack([xb.sum(1), (xb * xb).sum(1)], 1).float()      # [nblk][2][C]
    ab, st = nan(2 * C), nan(2 * C)
    h.call('ssc_bn_finalize', partial.cuda(), nblk, C, nblk * rows, scale.cuda(), offset.cuda(), 1e-5, ab, st)
    x4 = x.double().t().reshape(1, C, -1, 1)
    y64 = T.batchnorm(x4, scale.double(), offset.double()).reshape(C, -1).t()
    a64, b64 = ab.cpu().double()[:C], ab.cpu().double()[C:]
    check('bn_finalize', dict(nblk=nblk, C=C), x.double() * a64 + b64, y64, what='a * x + b')
    check('bn_finalize', dict(nblk=nblk, C=C), st[:C], x.double().mean(0), what='mean')
    check('bn_finalize', dict(nblk=nblk, C=C), st[C:], 1.0 / torch.sqrt(x.double().var(0, unbiased=False) + 1e-5), what='rstd')


@pytest.mark.parametrize('n', [1, 1003, 2 * 4096 * 256 + 5])         # cap: 4096 blocks of 256
def test_fill(n):
    h = hip()
    buf = nan(n + 8)
    h.call('ssc_fill', buf[4:], 1.5, n)
    assert bool((buf[4:4 + n] == 1.5).all()) and all_nan(buf[:4]) and all_nan(buf[4 + n:])
    assert rc('ssc_fill', buf, 2.5, 0) == 0 and all_nan(buf[:4])     # nothing to do, nothing launched


def test_elementwise_argument_checks():
    x = torch.ones(8, 136, device='cuda')
    ab = torch.ones(2 * 136, device='cuda')
    o = nan(8, 136)
    assert rc('ssc_residual_merge', x, ab, x, None, 0, o, 8, 3) == -1 and all_nan(o)
    assert rc('ssc_residual_merge', x, ab, x, None, 0, o, 8, 130) == -1 and all_nan(o)
    ws = nan(4096)
    out = nan(130)
    assert rc('ssc_colsum', x, 134, 8, 130, out, 0, ws, ws.numel() * 4) == -1       # ld & 3
    assert rc('ssc_colsum', x, 128, 8, 130, out, 0, ws, ws.numel() * 4) == -1       # padded C > ld
    assert rc('ssc_colsum', x, 136, 8, 130, out, 0, ws, 2 * 132 * 4 - 1) == -2      # one row block of [2][132] partials
    assert all_nan(out) and all_nan(ws)
    st = nan(2 * 130)
    assert rc('ssc_bn_stats', x, 8, 130, 136, ab, ab, 1e-5, st, st, ws, ws.numel() * 4) == -1 and all_nan(st)      # C & 3


# ------------------------------------------------------------------ batch statistics on ill-conditioned inputs
BN_CASES = [(0.0, 1.0), (10.0, 1.0), (100.0, 1.0), (1000.0, 1.0), (50.0, 0.01)]
BN_TOL = 2e-4


def _rel(got, ref):
    got, ref = got.detach().cpu().double(), ref.detach().cpu().double()
    return float((got - ref).abs().max()) / max(1.0, float(ref.abs().max()))


def _bn_oracle(x, scale, offset, g, dtype):
    """mean, 1/std, y = batchnorm(x) and (g given) dx of <g, y> in ``dtype`` (T.batchnorm: the two-pass form of
    tf.nn.moments).  No activation sits between the norm and g: at mean/std = 5000 the float32 y is off by ~5e-4 on either side,
    an activation's derivative then flips on the elements with |y| below that, and the max-norm distance of dx would measure
    which elements flipped, not the statistics (test_gpu_igemm.py::test_bn_stats_and_backward holds the activation forms)."""
    M, C = x.shape
    xx = x.detach().clone().to(dtype).requires_grad_(g is not None)
    x4 = xx.t().reshape(1, C, M, 1)
    y = T.batchnorm(x4, scale.to(dtype), offset.to(dtype))
    out = {}
    if g is not None:
        (y.reshape(C, M).t() * g.to(dtype)).sum().backward()
        out['dx'] = xx.grad
    xv = xx.detach()
    mean = xv.mean(0)
    out.update(mean=mean, rstd=torch.rsqrt(((xv - mean) ** 2).mean(0) + 1e-5), y=y.detach().reshape(C, M).t())
    return out


def _bn_refs(x, scale, offset, g):
    return _bn_oracle(x, scale, offset, g, torch.float64), _bn_oracle(x, scale, offset, g, torch.float32)


def _bn_judge(test, cfg, dev, refs):
    r64, r32 = refs
    bad = []
    for k in sorted(dev):
        e, c = _rel(dev[k], r64[k]), _rel(r32[k], r64[k])
        bound = max(BN_TOL, 1.5 * c)
        print('%s %s %s: device %.3e  fp32 oracle %.3e  bound %.3e' % (test, cfg, k, e, c, bound))
        parity_log(test, dict(cfg, what=k), e, bound, variant='kernel', cpu_fp32_vs_f64=c)
        if not e <= bound:
            bad.append((k, e, c, bound))
    assert not bad, (test, cfg, bad)


def _bn_input(mean, std, M, C):
    x = mean + std * rnd(M, C, seed=50)
    return x, 1.0 + 0.1 * rnd(C, seed=51), 0.1 * rnd(C, seed=52), rnd(M, C, seed=53)


@pytest.mark.parametrize('mean,std', BN_CASES)
@pytest.mark.parametrize('M', [333, 70000, 768 * 768])
@pytest.mark.parametrize('C', [16, 128])
def test_bn_stats_ill_conditioned(mean, std, M, C):
    """hip.bn_stats + hip.bn_act_backward, dense rows and (through hip.bn_stats_view of a channel slice) ldx > C."""
    h = hip()
    x, scale, offset, g = _bn_input(mean, std, M, C)
    gd, sd, od = g.cuda(), scale.cuda(), offset.cuda()
    refs = _bn_refs(x, scale, offset, g)
    for ldx in (C, C + 8):
        buf = torch.zeros(1, M, 1, ldx, device='cuda')
        buf[..., :C] = x.cuda().reshape(1, M, 1, C)
        xd = buf[..., :C]
        ab, st = nan(2 * C), nan(2 * C)
        if ldx == C:
            h.bn_stats(xd.reshape(M, C), sd, od, ab, st)
        else:
            h.bn_stats_view(xd, sd, od, ab, st)          # a channel slice: its rows keep the parent's stride
        y = nan(M, C)
        h.call('ssc_affine_act', buf, ldx, ab, C, 0, y, C, M, C)
        dx = nan(M, C)
        h.bn_act_backward(buf.view(M, ldx)[:, :C], ab, st, gd, 0, dx)
        _bn_judge('bn_stats_ill_conditioned', dict(mean=mean, std=std, M=M, C=C, ldx=ldx),
                  dict(mean=st[:C], rstd=st[C:], y=y, dx=dx), refs)


def test_bn_stats_view_is_bn_stats_of_the_rows():
    h = hip()
    x = (100.0 + rnd(2, 5, 7, 16, seed=54)).cuda()
    s, o = torch.ones(16, device='cuda'), torch.zeros(16, device='cuda')
    ab1, st1, ab2, st2 = nan(32), nan(32), nan(32), nan(32)
    h.bn_stats_view(x, s, o, ab1, st1)
    h.bn_stats(x.view(70, 16), s, o, ab2, st2)
    assert torch.equal(ab1, ab2) and torch.equal(st1, st2)


BN_EPI_SHAPES = {333: (1, 9, 37), 70000: (2, 175, 200), 768 * 768: (1, 768, 768)}


# The column sums that the conv epilogues deliver are still raw float32 sums folded as q/M - mean^2 (fold_rows has no shift to add
# back): measured |1/std error| / bound of the cases that miss, (C, M, mean, std) -> ratio.  ssc_bn_stats itself (the sweep above)
# takes its sums around row 0 of the channel and holds the bound everywhere.
EPILOGUE_MISSES = {
    (16, 333, 100.0, 1.0): 4.3, (16, 333, 1000.0, 1.0): 889, (16, 333, 50.0, 0.01): 10870, (16, 70000, 1000.0, 1.0): 36,
    (16, 70000, 50.0, 0.01): 1063, (16, 589824, 1000.0, 1.0): 15, (16, 589824, 50.0, 0.01): 470,
    (128, 333, 100.0, 1.0): 4.5, (128, 333, 1000.0, 1.0): 378, (128, 333, 50.0, 0.01): 10825, (128, 70000, 1000.0, 1.0): 51,
    (128, 70000, 50.0, 0.01): 3538, (128, 589824, 100.0, 1.0): 1.6, (128, 589824, 1000.0, 1.0): 163,
    (128, 589824, 50.0, 0.01): 11560,
}


def _epilogue_cases():
    out = []
    for C in (16, 128):
        for M in (333, 70000, 768 * 768):
            for mean, std in BN_CASES:
                r = EPILOGUE_MISSES.get((C, M, mean, std))
                marks = [pytest.mark.xfail(strict=True, reason='epilogue-delivered sums are not shifted yet: 1/std error %s x the '
                                                                 'bound max(2e-4, 1.5 x float32 moments)' % r)] if r else []
                out.append(pytest.param(mean, std, M, C, marks=marks))
    return out


@pytest.mark.parametrize('mean,std,M,C', _epilogue_cases())
def test_bn_stats_ill_conditioned_from_conv_epilogue(mean, std, M, C):
    """The statistics a conv launch delivers (conv_forward(..., bn=...)): a 1x1 conv with the identity as its filter hands the
    biased input through, so the same means reach the epilogue's column sums."""
    h = hip()
    x, scale, offset, g = _bn_input(mean, std, M, C)
    n, hh, ww = BN_EPI_SHAPES[M]
    xd = x.cuda().reshape(n, hh, ww, C)
    w = torch.eye(C, device='cuda').reshape(1, 1, C, C).contiguous()
    out = nan(n, hh, ww, C)
    ab, st = nan(2 * C), nan(2 * C)
    h.conv_forward(h.View(xd), w, 1, 0, out, bn=(scale.cuda(), offset.cuda(), ab, st))
    assert _rel(out.reshape(M, C), x) <= 1e-6          # the conv itself hands x through
    y = nan(M, C)
    h.call('ssc_affine_act', out, C, ab, C, 0, y, C, M, C)
    r = dict(mean=st[:C], rstd=st[C:], y=y)
    _bn_judge('bn_stats_ill_conditioned_epilogue', dict(mean=mean, std=std, M=M, C=C), r, _bn_refs(x, scale, offset, None))


# ------------------------------------------------------------------ the folds of per-block rows
@pytest.mark.parametrize('nblk,C', [(3, 5), (600, 64)])
@pytest.mark.parametrize('with_grads', [True, False])
def test_bn_bwd_finalize(nblk, C, with_grads):
    """Rows [nblk][2][C] of (sum dz | sum dz*xhat) -> coef = the two means over M rows, dscale = sum dz*xhat, doffset = sum dz:
    the two sums of the norm's backward (the autograd of T.batchnorm w.r.t. offset and scale)."""
    h = hip()
    M = 4000
    partial = rnd(nblk, 2, C, seed=60)
    coef = nan(2 * C)
    ds, do = (nan(C), nan(C)) if with_grads else (None, None)
    h.call('ssc_bn_bwd_finalize', partial.cuda(), nblk, C, M, coef, ds, do)
    tot = partial.double().sum(0)
    cfg = dict(nblk=nblk, C=C, grads=with_grads)
    check('bn_bwd_finalize', cfg, coef, (tot / M).reshape(-1), what='coef')
    if with_grads:
        check('bn_bwd_finalize', cfg, do, tot[0], what='doffset')
        check('bn_bwd_finalize', cfg, ds, tot[1], what='dscale')


@pytest.mark.parametrize('nsplit,N,C', [(1, 2, 5), (37, 3, 130)])
def test_minmax_finalize(nsplit, N, C):
    """Rows [N][nsplit][2][C] (min row, max row) -> [N][2][C]: tf.reduce_min / reduce_max over the splits (mru.py:414-415)."""
    h = hip()
    lo = rnd(N, nsplit, C, seed=61)
    part = torch.stack([lo, lo + rnd(N, nsplit, C, seed=62).abs()], 2).contiguous()
    mnmx = nan(N, 2, C)
    h.call('ssc_minmax_finalize', part.cuda(), nsplit, N, C, mnmx)
    ref = torch.stack([part[:, :, 0].min(1).values, part[:, :, 1].max(1).values], 1)
    assert torch.equal(mnmx.cpu(), ref)
