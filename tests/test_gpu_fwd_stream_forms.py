"""Every form of the seven streaming kernels ssc_conv_forward dispatches before the tiled ones -- fewchan_conv_kernel<4 / 8>,
pw1x1_kernel<K, NARROW>, c3x3n16_kernel and c3x3_kernel<C, TCW>, s2n16_kernel<STRIDE>, tr4_tiny_kernel, fewchan7_conv_kernel,
tr4n16_kernel (csrc/fewchan.hip, pw1x1.hip, c3x3.hip, s2n16.hip, tr4tiny.hip, fewchan7.hip, tr4n16.hip) -- against the float64
reference of tests/fwd_oracle.py (its table STREAM_CASES) under the any-order dot-product bound (kernel_check.check_dot with
extra_terms=0), per element:

    |got - ref| <= (K + 8) * 2^-24 * S

K the non-zero products of the element, S the float64 sum of the absolute products.  These kernels are exact-fp32 MFMA or FMA
chains: each product and each addition rounds once, in whatever order (gamma_K); the split of K over the four waves of s2n16 /
tr4n16 followed by ((a + b) + c) + d is one more summation tree of the same K terms; the folded norm (one fma), the slope
product and the float32 slope constant are inside the 8.  tr4tiny's activated epilogues (epi 1 tanh, 2 lrelu 0.2) are 1-Lipschitz:
the same bound holds behind them, plus 8 * 2^-24 * |f(ref)| for the evaluation of f itself, as in
tests/test_gpu_fwd_bf16_forms.py.  Nothing in the bound is measured.
One probe per windowed kernel has one non-zero channel in the whole gathered tensor (K <= taps) and pw1x1's has one non-zero
channel per pixel (K = 1): there the bound is a few ulp of single products, and a wrong tap or channel index cannot hide.

Every launch goes through the hip.py wrapper (conv_forward, deconv_forward, conv_dgrad, deconv_dgrad).  A spy stands in front
of ssc_conv_forward, ssc_conv_forward_bn and ssc_conv_forward_bnbwd: with the wrapper's own descriptor it asks
ssc_conv_stream_plan -- computed by the functions that make the launch -- and ssc_conv_forward_kernel_name before the launch,
and asserts the kernel, the instantiation and whether some persistent workgroup takes two tiles or more (tiles > workgroups;
the table's expectations are for the MI355X's 256 CUs).

Every source and the filter are views inside larger device buffers that hold 1.0e3 on both sides, as the padding lanes do (finite:
fewchan, fewchan7 and tr4n16 multiply a padding lane by a zero filter row); the output lies inside a NaN buffer.  After the launch
the inputs and their guards are bit-identical, the output columns outside [coff, coff + Nstore) of every row hold what they
held, columns [Nn, Nstore) are exactly 0 and the guards of the output are still NaN.

Riders.  A case with `bn` runs again through conv_forward / deconv_forward(bn=...): the rider plan must say 'stream', the output
must equal the launch without the rider bit for bit, and (mean, 1/std, a, b) must agree with float64 statistics of the stored
output to 1e-5 of the largest value (the criterion of tests/test_gpu_round4_kernels.py) -- on the walking cases rows of
walkers with one tile and with two fold into the same sums.  A case with `bnbwd` runs its data gradient again with
conv_dgrad(bnbwd=...): same bits, and hip.bn_act_backward from those rows equals the separate pass to 1e-4, as that file does it.

Filter orientation and tap direction of c3x3 (the only kernel here that admits more than one pair): conv_forward gives (KN,
forward), conv_forward(w_nk=) (NK, forward), conv_dgrad (NK, flipped); the predicate also admits (KN, flipped), which no wrapper
produces."""
import contextlib
import ctypes

import pytest
import torch

import fwd_oracle as O
from kernel_check import GUARD, NAN, U_FP32, all_nan, bits, check, check_dot, inside, rnd

pytestmark = pytest.mark.gpu

KERNEL_ID = {'conv_fewchan': 4, 'conv_pw1x1': 5, 'conv_c3x3': 6, 'conv_s2n16': 7, 'deconv_tr4_tiny': 8, 'conv_fewchan7': 9,
             'deconv_tr4n16': 10}       # the dispatch order: the ids of ssc_conv_rider_plan and ssc_conv_stream_plan
ENTRY = {None: 'ssc_conv_forward', 'bn': 'ssc_conv_forward_bn', 'bnbwd': 'ssc_conv_forward_bnbwd'}
REACHED = set()         # (kernel id, instantiation, tiles > workgroups, bmode, kstep) of this session's launches
_REF = {}


def _hip():
    from sketchyscenecolorization_amd import hip
    return hip


def _reference(c):
    """Inputs and the float64 reference of a case: computed once, shared by its launches, never modified (the one before it
    is dropped: the references of the walking cases are hundreds of megabytes together)."""
    if c['name'] not in _REF:
        _REF.clear()
        inp = O.make_inputs(c)
        _REF[c['name']] = (inp,) + O.ref_taps(c, inp)
    return _REF[c['name']]


def _plan(hip, d):
    """(return code, the four values) of ssc_conv_stream_plan."""
    out4 = (ctypes.c_int * 4)(*([-99] * 4))
    rc = hip.lib().ssc_conv_stream_plan(ctypes.byref(d), out4)
    return rc, tuple(out4)


class _Spy(object):
    """Stands in front of ssc_conv_forward, ssc_conv_forward_bn and ssc_conv_forward_bnbwd while a wrapper runs: the descriptor
    the wrapper made is handed to `before` with the entry point's name, which asks the queries and asserts, and then to the
    library."""

    def __init__(self, hip, before):
        self.lib, self.before, self.calls, self.real = hip.lib(), before, [], {}

    def _stand_in(self, entry):
        def call(dref, *rest):
            self.calls.append(entry)
            self.before(entry, dref._obj)
            return self.real[entry](dref, *rest)
        return call

    def __enter__(self):
        for entry in ENTRY.values():
            self.real[entry] = getattr(self.lib, entry)
            setattr(self.lib, entry, self._stand_in(entry))
        return self

    def __exit__(self, *exc):
        for entry, real in self.real.items():
            setattr(self.lib, entry, real)


@contextlib.contextmanager
def _rider_log(hip):
    """[(rider, path)] of the launches made inside: what ssc_conv_rider_plan says of each, asked before it launches."""
    hip.RIDER_LOG = log = []
    try:
        yield log
    finally:
        hip.RIDER_LOG = None


def _wrapper(hip, c, dev, out, bn=None, bnbwd=None):
    """The hip.py wrapper of the case's op."""
    kind, geo = c['kind'], O.geometry(c)
    _, act, _, act1 = c['tf']
    v = hip.View(dev['s0'], dev['s1'], dev['ab0'], act, dev['ab1'], act1)
    if kind == 'conv':
        same = c['pad'] == 'same'
        hip.conv_forward(v, dev['w'], c['stride'], 0 if same else c['pad'], out, coff=c['coff'], nstore=c['nstore'], epi=c['epi'],
                         same=same, w_nk=dev['w_nk'], bn=bn)
    elif kind == 'deconv':
        hip.deconv_forward(v, dev['w'], out, coff=c['coff'], nstore=c['nstore'], epi=c['epi'], bn=bn)
    elif kind == 'conv_dgrad':
        hip.conv_dgrad(v, dev['w'], c['stride'], geo.get('pad_before', c['pad']), out, n_off=c['n_off'], nn=geo['nn'],
                       nstore=c['nstore'], coff=c['coff'], bnbwd=bnbwd)
    else:
        assert kind == 'deconv_dgrad' and c['coff'] == 0 and c['nstore'] is None
        hip.deconv_dgrad(v, dev['w'], out, n_off=c['n_off'], nn=geo['nn'], bnbwd=bnbwd)


def _run(hip, c, inp, rider=None):
    """One launch, without a rider or with 'bn' / 'bnbwd': the plan the query reports for it in front of the launch, the output
    [n, OH, OW, nn] (Nstore columns checked and cut to Nn), the stored columns [rows, Nstore], and what the rider left."""
    name, geo, e = c['name'], O.geometry(c), c['expect']
    nn = geo['nn']
    nstore, coff = c['nstore'] or nn, c['coff']
    ldc = c['ldc'] or (coff + nstore)
    assert nn <= nstore and coff + nstore <= ldc and not c['acc'] and not c['bias']
    keep, dev = [], {}
    for k in ('s0', 's1', 'w'):
        dev[k] = None
        if inp[k] is not None:
            buf, dev[k] = inside(inp[k], O.PAD_LANE)
            keep.append((k, buf, buf.clone()))
    dev['w_nk'] = None
    if c['nk']:
        buf, dev['w_nk'] = inside(inp['w'].permute(0, 1, 3, 2).contiguous(), O.PAD_LANE)
        keep.append(('w_nk', buf, buf.clone()))
    for k in ('ab0', 'ab1'):
        dev[k] = inp[k].cuda() if inp[k] is not None else None
    held = torch.full((c['n'], geo['OH'], geo['OW'], ldc), NAN)
    obuf, out = inside(held, NAN)
    M = c['n'] * geo['OH'] * geo['OW']
    left, bn, bnbwd = {}, None, None
    if rider == 'bn':
        assert coff == 0 and ldc == nstore
        left['scale'], left['offset'] = (1.0 + 0.1 * rnd(nstore, seed=c['seed'] + 1)).cuda(), (0.1 * rnd(nstore, seed=c['seed'] + 2)).cuda()
        left['ab'], left['stats'] = torch.full((2 * nstore,), NAN, device='cuda'), torch.full((2 * nstore,), NAN, device='cuda')
        bn = (left['scale'], left['offset'], left['ab'], left['stats'])
    elif rider == 'bnbwd':      # the output is the gradient w.r.t. act(norm(x)) of a tensor x laid out like it
        assert coff == 0 and ldc == nstore == nn
        left['x2d'] = rnd(M, nn, seed=c['seed'] + 3).cuda()
        left['scale'], left['offset'] = (1.0 + 0.1 * rnd(nn, seed=c['seed'] + 1)).cuda(), (0.1 * rnd(nn, seed=c['seed'] + 2)).cuda()
        left['ab'], left['stats'] = torch.empty(2 * nn, device='cuda'), torch.empty(2 * nn, device='cuda')
        hip.bn_stats(left['x2d'], left['scale'], left['offset'], left['ab'], left['stats'])
        left['sums'] = hip.BnBwdSums(left['x2d'], left['ab'], left['stats'],
                                     torch.zeros(hip.BnBwdSums.rows_needed(M), 2 * nn, device='cuda'))
        bnbwd = left['sums'].take(c['bnbwd'])
    seen = []

    def before(entry, d):
        rc, plan = _plan(hip, d)
        got_name = hip._kernel_name('ssc_conv_forward_kernel_name', d)
        assert got_name == e['kernel'], (name, 'kernel', got_name, 'expected', e['kernel'], rc, plan)
        if e['inst'] is None:
            assert rc == -10, (name, 'ssc_conv_stream_plan', rc, plan)
        else:
            assert rc == 0 and plan[0] == KERNEL_ID[got_name.split('<')[0]] and plan[1] == e['inst'], (name, rc, plan, e)
            assert plan[2] >= 1 and plan[3] >= 1 and (plan[2] > plan[3]) == e['walk'], (name, 'tiles, workgroups', plan, e)
        seen.append((entry, rc, plan, d.bmode, d.kstep))

    with _rider_log(hip) as log:
        with _Spy(hip, before) as spy:
            _wrapper(hip, c, dev, out, bn=bn, bnbwd=bnbwd)
        torch.cuda.synchronize()
    assert spy.calls == [ENTRY[rider]] and len(seen) == 1, (name, spy.calls)
    _, rc, plan, bmode, kstep = seen[0]
    if rider is not None and rc == 0:
        assert log == [(rider, 'stream')], (name, log)
    assert hip.sk_timeouts() == 0, (name, 'a hand-off timed out')
    for k, buf, before_bits in keep:        # the launch wrote nothing into its inputs or around them
        assert torch.equal(bits(buf), bits(before_bits)), (name, 'an input or its guard changed', k)
    assert all_nan(obuf[:GUARD]) and all_nan(obuf[GUARD + out.numel():]), (name, 'a store outside the output tensor')
    heldd = held.cuda()
    for lo, hi in ((0, coff), (coff + nstore, ldc)):
        assert torch.equal(bits(out[..., lo:hi].contiguous()), bits(heldd[..., lo:hi].contiguous())), \
            (name, 'a store outside the columns of the launch', lo, hi)
    assert bool((out[..., coff + nn:coff + nstore] == 0).all()), (name, 'columns [Nn, Nstore) are not zero')
    if rc == 0:
        REACHED.add((plan[0], plan[1], plan[2] > plan[3], bmode, kstep))
    left['log'], left['wgs'] = log, plan[3]
    return plan if rc == 0 else None, out[..., coff:coff + nn].clone(), out[..., coff:coff + nstore].reshape(M, nstore).clone(), left


def _check(c, plan, got, ref, S, K, rider=None):
    cfg = dict(case=c['name'], kernel=c['expect']['kernel'], inst=c['expect']['inst'], walk=int(c['expect']['walk']), rider=rider or '-')
    if c['epi']:
        f = O.epilogue(c, ref)
        return check_dot('fwd_stream_forms', cfg, got, f, S, K, plan=plan, extra_terms=0, allow=8 * U_FP32 * f.abs())
    return check_dot('fwd_stream_forms', cfg, got, ref, S, K, plan=plan, extra_terms=0)


def _check_statistics(c, stored, left):
    """(mean, 1/std, a, b) of the rider against float64 statistics of the stored output: 1e-5 of the largest value each."""
    o = stored.double()
    co = o.shape[1]
    mean, var = o.mean(0), o.var(0, unbiased=False)
    rstd = 1.0 / torch.sqrt(var + 1e-5)
    scale, offset = left['scale'].double(), left['offset'].double()
    cfg = dict(case=c['name'], rows=o.shape[0])
    check('fwd_stream_forms_bn', cfg, left['stats'][:co], mean, tol=1e-5, what='mean')
    check('fwd_stream_forms_bn', cfg, left['stats'][co:], rstd, tol=1e-5, what='rstd')
    check('fwd_stream_forms_bn', cfg, left['ab'][:co], rstd * scale, tol=1e-5, what='a')
    check('fwd_stream_forms_bn', cfg, left['ab'][co:], offset - mean * rstd * scale, tol=1e-5, what='b')


def _check_norm_backward(hip, c, stored, left):
    """The rows of sums the data gradient's epilogue left against the separate pass over the stored gradient."""
    sums, M, nn = left['sums'], stored.shape[0], stored.shape[1]
    assert sums.sources == 1 and sums.missed == 0 and 0 < sums.rows <= left['wgs'], (c['name'], sums.sources, sums.missed, sums.rows)
    outs = []
    for pre in (sums, None):
        dx = torch.full((M, nn), NAN, device='cuda')
        ds, do = torch.empty(nn, device='cuda'), torch.empty(nn, device='cuda')
        hip.bn_act_backward(left['x2d'], left['ab'], left['stats'], stored, c['bnbwd'], dx, dscale=ds, doffset=do, pre=pre)
        outs.append((dx, ds, do))
    for what, a, b in zip(('dx', 'dscale', 'doffset'), *outs):
        check('fwd_stream_forms_bnbwd', dict(case=c['name']), a, b, tol=1e-4, what=what)


@pytest.mark.parametrize('name', [c['name'] for c in O.STREAM_CASES])
def test_form(name):
    hip = _hip()
    c = O.lookup(name)
    inp, ref, S, K = _reference(c)
    plan, got, stored, _ = _run(hip, c, inp)
    _check(c, plan, got, ref, S, K)
    for rider in (['bn'] if c['bn'] else []) + (['bnbwd'] if c['bnbwd'] else []):
        plan2, got2, stored2, left = _run(hip, c, inp, rider=rider)
        assert plan2 == plan and torch.equal(bits(stored2), bits(stored)), (name, 'the rider changed the output', rider, plan2)
        if rider == 'bn':
            _check_statistics(c, stored2, left)
        else:
            _check_norm_backward(hip, c, stored2, left)


def test_zz_every_form_was_reached():
    """Runs last in the file.  Every instantiation ssc_conv_stream_plan can report, for all seven kernels; a launch with
    tiles > workgroups for each persistent instantiation of pw1x1 (both NARROW values), c3x3 (all four), s2n16 (both),
    fewchan<4>, fewchan<8>, fewchan7 and tr4n16; for c3x3 both filter orientations and both tap directions.
    Not reachable, by the code: a second tile in tr4tiny (a workgroup per block of 256 pixels, nothing is walked);
    s2n16_kernel<2> and tr4n16 without a second tile (their row minima, 32768 and 16384, are at least 1024 / 512 tiles of 2 x 16
    pixels on 512 / 128 walkers; s2n16_kernel<1> has at least 512 tiles of 4 x 16 on 512: one each only in a lattice of
    exactly 32768 pixels that its tiles divide); c3x3_kernel<32, *> with 4 outputs, s2n16_kernel<1> with 4 and tr4n16 with 4 outputs of one source or of
    32 + 224, ... channels, all real (narrow.hip is earlier in the dispatch order and takes <= 4 outputs of whole 32-channel
    chunks at stride 1 and in the transposed form); c3x3 from 16 channels to more than 16 (the predicate refuses it:
    c3x3_kernel<16, TCW> stages 16 filter columns); n_off > 0 on pw1x1 (refused), tr4n16 and tr4tiny (deconv_forward has none);
    c3x3's (KN, flipped) pair (no wrapper produces it)."""
    R = REACHED
    want = {4: (0, 1), 5: range(8), 6: range(4), 7: (0, 1), 8: (0,), 9: (0,), 10: (0,)}
    walked = {(r[0], r[1] & 1 if r[0] == 5 else r[1]) for r in R if r[2]}       # pw1x1: per NARROW value
    for kernel, insts in sorted(want.items()):
        for inst in insts:
            assert any(r[:2] == (kernel, inst) for r in R), ('kernel', kernel, 'instantiation', inst, 'never ran', sorted(R))
            if kernel != 8:
                assert (kernel, inst & 1 if kernel == 5 else inst) in walked, \
                    ('kernel', kernel, 'instantiation', inst, 'no walker took a second tile', sorted(R))
    assert not any(r[0] == 6 and r[1] > 3 for r in R) and not any(r[0] == 8 and r[2] for r in R)
    c3 = [r for r in R if r[0] == 6]
    assert {r[3] for r in c3} == {0, 1} and {r[4] for r in c3} == {1, -1}, ('c3x3 orientations / tap directions', sorted(c3))
