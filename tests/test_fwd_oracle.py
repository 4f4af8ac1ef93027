"""The float64 reference of the forward bf16x6 tests (tests/fwd_oracle.py) against itself, the probes' float32 chain against
their bound, the comparison rule (kernel_check.check_dot) against results that lost a plane or a term, and the edges of the
library's fwd_is_bf predicate through the host-only plan query; the same agreement over the table of the streaming kernels
(STREAM_CASES), and the row minima and column ends of their predicates (ssc_conv_*_supported, ssc_conv_stream_plan).  No GPU."""
import ctypes

import pytest
import torch

import fwd_oracle as O
from kernel_check import U_FP32, check_dot

_ALL = O.all_cases()


@pytest.mark.parametrize('name', [c['name'] for c in _ALL])
def test_tf_reference_equals_tap_loop_reference(name):
    """(a) the op of oracle/tf_ops.py (the data gradients by autograd) == (b) shifted slices + einsum, to 1e-12 of the largest
    value; S >= |ref| and K counts at least one product wherever ref is not zero."""
    c = O.lookup(name)
    inp = O.make_inputs(c)
    a = O.ref_tf(c, inp)
    pre, S, K = O.ref_taps(c, inp)
    b = O.epilogue(c, pre)
    assert a.shape == b.shape == S.shape == K.shape and a.dtype == b.dtype == torch.float64
    scale = float(b.abs().max())
    assert scale > 0 and bool(torch.isfinite(a).all()) and bool((S >= pre.abs() * (1 - 1e-12)).all())
    assert float((a - b).abs().max()) <= 1e-12 * scale, (float((a - b).abs().max()), scale)
    assert bool((K[pre != 0] >= 1).all()) and float(K.max()) <= len(O.geometry(c)['taps']) * c['src'][2] + 2


@pytest.mark.parametrize('name', [c['name'] for c in O.STREAM_CASES])
def test_stream_tf_reference_equals_tap_loop_reference(name):
    """The same agreement over the table of the streaming kernels (tests/test_gpu_fwd_stream_forms.py); the probes' counts: one
    product per output (one-hot), at most one per tap (one channel)."""
    c = O.lookup(name)
    inp = O.make_inputs(c)
    a = O.ref_tf(c, inp)
    pre, S, K = O.ref_taps(c, inp)
    b = O.epilogue(c, pre)
    assert a.shape == b.shape == S.shape == K.shape and a.dtype == b.dtype == torch.float64
    scale = float(b.abs().max())
    assert scale > 0 and bool(torch.isfinite(a).all()) and bool((S >= pre.abs() * (1 - 1e-12)).all())
    assert float((a - b).abs().max()) <= 1e-12 * scale, (float((a - b).abs().max()), scale)
    taps = len(O.geometry(c)['taps'])
    assert bool((K[pre != 0] >= 1).all()) and float(K.max()) <= taps * c['src'][2]
    if c['probe'] == 'onehot':
        assert float(K.max()) == 1 and bool((S == pre.abs()).all())
    elif c['probe'] == 'channel':       # the transposed forms: four of the sixteen taps per output
        assert 1 <= float(K.max()) <= (taps if c['kind'] != 'deconv' else 4)
    if c['src'][2] < c['src'][0] + c['src'][1]:         # padding lanes never reach the reference
        assert float(S.max()) < O.PAD_LANE


def test_every_case_has_a_seed_of_its_own():
    every = _ALL + O.STREAM_CASES
    seeds = [c['seed'] for c in every]
    assert len(set(seeds)) == len(seeds) and len({c['name'] for c in every}) == len(every)


def test_padding_lanes_do_not_reach_the_reference():
    for name, lane in (('km_36_35', O.PAD_LANE), ('km_132_130_nan_lanes', None)):
        c = O.lookup(name)
        inp = O.make_inputs(c)
        pad = inp['s0'][..., c['src'][2]:]
        assert bool((pad == lane).all()) if lane is not None else bool(torch.isnan(pad).all())
        ref, S, _ = O.ref_taps(c, inp)
        assert bool(torch.isfinite(ref).all()) and float(S.max()) < 1e3


@pytest.mark.parametrize('kind,src,p', O.PROBE_FORMS, ids=['%s-%s-%s' % f for f in O.PROBE_FORMS])
def test_probe_float32_chain_is_inside_its_bound(kind, src, p):
    """The one-hot probe's outputs are single products (K = 1: the bound is 11 * 2^-24 * |a*b|), the one-channel probe's sums of
    at most nine; what a CPU computes in float32 passes the device test's rule, so the probe cannot fail by construction.  The
    same values with the filter's third bf16 plane dropped (w rounded to 16 significant bits: the loss of the h*l product,
    ~2^-16 |a*b|) do not pass."""
    c = O.probe(kind, src, p)
    inp = O.make_inputs(c)
    ref, S, K = O.ref_taps(c, inp)
    assert float(K.max()) == (1 if kind == 'onehot' else 9)        # (0 where a relu on load cleared the pixel's one value)
    if kind == 'onehot':
        assert bool((S == ref.abs()).all())
    got = O.ref_taps(c, inp, torch.float32)[0]
    check_dot('fwd_probe_rule', dict(case=c['name']), got, ref, S, K, what='float32 CPU', extra_terms=2)
    lost = dict(inp, w=(inp['w'].view(torch.int32) & ~0xff).view(torch.float32))        # 16 of 24 significant bits kept
    assert float(((O.ref_taps(c, lost)[0] - ref).abs() / S.clamp(min=1e-300)).max()) > 64 * U_FP32
    with pytest.raises(AssertionError):
        check_dot('fwd_probe_rule', dict(case=c['name']), O.ref_taps(c, lost)[0], ref, S, K, what='l plane lost', extra_terms=2)


def test_rule_takes_a_count_per_element_and_an_allowance():
    """check_dot with K a tensor bounds every element by its own count; `allow` adds a per-element absolute allowance (the
    activated epilogues: 8 * 2^-24 * |f(ref)|); without either the bound is the one the filter-gradient tests use."""
    ref = torch.tensor([1.0, 2.0], dtype=torch.float64)
    S = ref.clone()
    off = torch.tensor([1.0 + 12 * U_FP32, 2.0], dtype=torch.float64)
    check_dot('fwd_rule', {}, off, ref, S, 4)
    check_dot('fwd_rule', {}, off, ref, S, torch.tensor([4.0, 1.0]))
    with pytest.raises(AssertionError):
        check_dot('fwd_rule', {}, off, ref, S, torch.tensor([1.0, 4.0]))
    check_dot('fwd_rule', {}, off, ref, S, torch.tensor([1.0, 4.0]), allow=torch.tensor([3 * U_FP32, 0.0]))


def _plan(hip, d, ws_bytes):
    """(return code, the ten values) of ssc_conv_bf_plan."""
    out10 = (ctypes.c_int * 10)(*([-99] * 10))
    rc = hip.lib().ssc_conv_bf_plan(ctypes.byref(d), ws_bytes, out10)
    return rc, tuple(out10)


def _edge(hip, C0=64, C1=0, HW=(12, 12), NB=2, T=(3, 3), n_off=0, Nn=68, nstore=None, bmode=1, k_real=None, ws_kc=None, wsplit=1 << 32,
          wC=None):
    """ssc_conv_bf_plan of a stride-1 SAME conv descriptor made of dummy aligned pointers (host only: nothing is dereferenced):
    (return code, the ten values)."""
    d = hip.ConvDesc()
    d.x.s0, d.x.s1, d.x.ab0, d.x.ab1 = 1 << 30, (1 << 31 if C1 else None), None, None
    d.x.C0, d.x.C1, (d.x.H, d.x.W), d.x.act, d.x.act1 = C0, C1, HW, 0, -1
    d.w, d.bias, d.out = 1 << 33, None, 1 << 34
    d.NB, (d.PH, d.PW), (d.TH, d.TW) = NB, HW, T
    d.in_stride, d.ioff_y, d.ioff_x, d.nphase, d.ky0, d.kx0, d.kstep = 1, -(T[0] // 2), -(T[1] // 2), 1, 0, 0, 1
    d.KH, d.KW = T
    k_real = C0 + C1 if k_real is None else k_real
    wN = n_off + Nn if wC is None else wC
    d.wC0, d.wC1 = (wN, k_real) if bmode else (k_real, wN)
    d.bmode, d.k_real, d.n_off, d.Nn = bmode, k_real, n_off, Nn
    d.Nstore = Nn if nstore is None else nstore
    (d.OH, d.OW), d.ldc, d.out_stride, d.ooff_y, d.ooff_x = HW, d.Nstore, 1, 0, 0
    d.sk_flags, d.wsplit, d.ws_nbp = 1 << 35, wsplit, 8
    d.ws_kc = 2 * (-(-C0 // 32) + C1 // 32) if ws_kc is None else ws_kc
    return _plan(hip, d, 256 << 20)


def test_predicate_edges():
    """The edges of fwd_is_bf through ssc_conv_bf_plan, host only (no GPU: the query launches nothing and the planner takes 256 CUs
    where it finds no device): 0 and a source form on one side, -10 on the other."""
    from sketchyscenecolorization_amd import hip
    if not hip.ARITH_BF16:      # SSC_ARITH=fp32: the library selects the bf16 kernels for nothing
        assert _edge(hip)[0] == -10
        return
    rc, plan = _edge(hip)
    assert rc == 0 and plan[3] == 1 and plan[2] == 1 and plan[5] == 1, (rc, plan)
    assert _edge(hip, wsplit=None)[0] == -10                                            # no filter planes
    assert _edge(hip, n_off=32)[0] == 0 and _edge(hip, n_off=31)[0] == -10 and _edge(hip, n_off=64)[0] == 0
    assert _edge(hip, Nn=33)[0] == 0 and _edge(hip, Nn=32)[0] == -10 and _edge(hip, Nn=30, nstore=33)[0] == 0
    assert _edge(hip, T=(4, 8))[0] == 0 and _edge(hip, T=(3, 11))[0] == -10             # 32 / 33 taps
    assert _edge(hip, C0=32)[1][3] == 1 and _edge(hip, C0=36)[1][3] == 2                # uniform / the partly empty last chunk
    assert _edge(hip, C0=36, k_real=33)[1][3] == 2 and _edge(hip, C0=36, k_real=0)[0] == -10 and _edge(hip, C0=36, k_real=37)[0] == -10
    assert _edge(hip, C0=36, ws_kc=4)[0] == 0 and _edge(hip, C0=36, ws_kc=2)[0] == -10 and _edge(hip, C0=36, ws_kc=6)[0] == -10
    assert _edge(hip, C0=32, C1=36)[0] == -10 and _edge(hip, C0=32, C1=64)[1][3] == 0   # two sources: whole chunks only
    # the gathered tensor: NB * H * W * C < 0x1fffffff elements
    assert 32 * 16777215 < 0x1fffffff < 32 * 16777216 and 36 * 14913080 < 0x1fffffff < 36 * 14913081
    assert _edge(hip, C0=32, NB=1, HW=(16777215, 1))[0] == 0 and _edge(hip, C0=32, NB=1, HW=(16777216, 1))[0] == -10
    assert _edge(hip, C0=36, NB=1, HW=(14913080, 1))[0] == 0 and _edge(hip, C0=36, NB=1, HW=(14913081, 1))[0] == -10
    # the filter: KH * KW * wC0 * wC1 < 0x1fffffff elements
    assert 9 * 64 * 932064 < 0x1fffffff < 9 * 64 * 932068 and 9 * 36 * 1657008 < 0x1fffffff < 9 * 36 * 1657012
    assert _edge(hip, wC=932064)[0] == 0 and _edge(hip, wC=932068)[0] == -10
    assert _edge(hip, C0=36, wC=1657008)[0] == 0 and _edge(hip, C0=36, wC=1657012)[0] == -10


def _stream_desc(hip, kernel, NB=1, HW=None, Nn=None, C=None, nstore=None, k_real=None):
    """A descriptor the streaming kernel `kernel` takes, as the hip.py wrapper of its op makes it, of dummy aligned pointers (host
    only: nothing is dereferenced).  HW: the output lattice."""
    geo = dict(pw1x1=dict(C=32, T=1, s=1, off=0, Nn=128, HW=(2048, 1)), c3x3=dict(C=16, T=3, s=1, off=-1, Nn=16, HW=(16384, 1)),
               s2n16=dict(C=64, T=4, s=2, off=-1, Nn=16, HW=(32768, 1)), fewchan=dict(C=8, T=4, s=2, off=-1, Nn=64, HW=(4, 32)),
               fewchan7=dict(C=4, T=7, s=2, off=-2, Nn=64, HW=(4, 32)), tr4n16=dict(C=256, T=2, s=1, off=0, Nn=16, HW=(16384, 1)),
               tr4_tiny=dict(C=4, T=2, s=1, off=0, Nn=3, HW=(9, 7)))[kernel]
    transposed = kernel in ('tr4n16', 'tr4_tiny')
    C = geo['C'] if C is None else C
    Nn = geo['Nn'] if Nn is None else Nn
    PH, PW = geo['HW'] if HW is None else HW
    K = 4 if transposed else geo['T']
    d = hip.ConvDesc()
    d.x.s0, d.x.s1, d.x.ab0, d.x.ab1 = 1 << 30, None, None, None
    d.x.C0, d.x.C1, d.x.H, d.x.W, d.x.act, d.x.act1 = C, 0, geo['s'] * PH, geo['s'] * PW, 0, -1
    d.w, d.bias, d.out = 1 << 33, None, 1 << 34
    d.NB, d.PH, d.PW, d.TH, d.TW, d.in_stride, d.ioff_y, d.ioff_x = NB, PH, PW, geo['T'], geo['T'], geo['s'], geo['off'], geo['off']
    d.nphase, d.ky0, d.kx0, d.kstep, d.KH, d.KW = (4, 0, 0, -2, 4, 4) if transposed else (1, 0, 0, 1, K, K)
    d.k_real = C if k_real is None else k_real
    d.bmode = int(transposed)
    d.wC0, d.wC1 = (Nn, d.k_real) if transposed else (d.k_real, Nn)
    d.n_off, d.Nn, d.Nstore = 0, Nn, Nn if nstore is None else nstore
    d.out_stride = 2 if transposed else 1
    d.OH, d.OW, d.ldc, d.ooff_y, d.ooff_x = d.out_stride * PH, d.out_stride * PW, d.Nstore, 0, 0
    return d


def test_stream_predicate_edges():
    """The row minima and the column ends of the streaming kernels' predicates, host only, and the plan query's answer on either
    side of one of them."""
    from sketchyscenecolorization_amd import hip
    l = hip.lib()

    def ok(kernel, **kw):
        return getattr(l, 'ssc_conv_%s_supported' % kernel)(ctypes.byref(_stream_desc(hip, kernel, **kw)))

    for kernel in ('fewchan', 'pw1x1', 'c3x3', 's2n16', 'tr4_tiny', 'fewchan7', 'tr4n16'):
        assert ok(kernel) == 1, kernel
    # rows: M = NB * PH * PW
    for kernel, m in (('pw1x1', 2048), ('c3x3', 16384), ('s2n16', 32768), ('tr4n16', 16384)):
        assert ok(kernel, HW=(m, 1)) == 1 and ok(kernel, HW=(m - 1, 1)) == 0, (kernel, m)
        assert ok(kernel, NB=2, HW=(m // 2, 1)) == 1 and ok(kernel, NB=2, HW=(m // 2 - 1, 1)) == 0, (kernel, m)
    assert ok('tr4_tiny', HW=(1, 1)) == 1
    # columns
    assert ok('pw1x1', Nn=64) == 1 and ok('pw1x1', Nn=32) == 0 and ok('pw1x1', Nn=96) == 1 and ok('pw1x1', Nn=80) == 0
    assert ok('pw1x1', Nn=128, nstore=132) == 0
    for kernel in ('c3x3', 's2n16', 'tr4n16'):
        assert ok(kernel, Nn=4) == 1 and ok(kernel, Nn=3) == 0 and ok(kernel, Nn=16) == 1, kernel
        assert ok(kernel, Nn=12, nstore=16) == 0, kernel
    assert ok('s2n16', Nn=17) == 0 and ok('tr4n16', Nn=17) == 0
    assert ok('c3x3', C=32, Nn=32) == 1 and ok('c3x3', C=32, Nn=33) == 0 and ok('c3x3', C=32, Nn=4) == 1
    # 16 channels to more than 16: c3x3_kernel<16, TCW> stages 16 columns of the filter (K * C / 256 = 9 elements per thread)
    assert ok('c3x3', C=16, Nn=17) == 0 and ok('c3x3', C=16, Nn=32) == 0 and ok('c3x3', C=32, Nn=17) == 1
    for kernel in ('fewchan', 'fewchan7'):
        assert ok(kernel, Nn=33) == 1 and ok(kernel, Nn=32) == 0 and ok(kernel, Nn=64) == 1 and ok(kernel, Nn=65) == 0, kernel
    assert ok('fewchan', Nn=33, nstore=36) == 1 and ok('fewchan7', Nn=33, nstore=36) == 0
    assert ok('fewchan', C=4, k_real=3) == 1 and ok('fewchan', C=8, k_real=9) == 0 and ok('fewchan', C=12) == 0
    assert ok('fewchan7', k_real=1) == 1 and ok('fewchan7', k_real=0) == 0 and ok('fewchan7', k_real=5) == 0
    assert ok('tr4_tiny', Nn=1, nstore=4) == 1 and ok('tr4_tiny', Nn=0, nstore=4) == 0 and ok('tr4_tiny', Nn=4) == 1
    assert ok('tr4_tiny', Nn=5) == 0 and ok('tr4_tiny', k_real=1) == 1 and ok('tr4_tiny', k_real=0) == 0
    assert ok('tr4n16', k_real=254) == 1 and ok('tr4n16', k_real=3) == 0 and ok('tr4n16', k_real=257) == 0
    # the plan query: {kernel, instantiation, tiles, workgroups} where one of the seven takes the launch, -10 where none does
    out4 = (ctypes.c_int * 4)(*([-99] * 4))
    # a lattice of 16384 x 1: the 8 x 16 tile wastes fewer pixels (c3x3_kernel<16, 16>), 2048 tiles on 3 x 256 walkers
    assert l.ssc_conv_stream_plan(ctypes.byref(_stream_desc(hip, 'c3x3')), out4) == 0 and tuple(out4) == (6, 1, 2048, 768)
    assert l.ssc_conv_stream_plan(ctypes.byref(_stream_desc(hip, 'c3x3', HW=(16383, 1))), out4) == -10
    assert l.ssc_conv_stream_plan(ctypes.byref(_stream_desc(hip, 'c3x3', C=16, Nn=17)), out4) == -10
    assert l.ssc_conv_stream_plan(ctypes.byref(_stream_desc(hip, 'pw1x1', Nn=160)), out4) == 0 and tuple(out4) == (5, 2, 64, 64)
    d = _stream_desc(hip, 'pw1x1')
    d.nphase = 2
    assert l.ssc_conv_stream_plan(ctypes.byref(d), out4) == -2      # ssc_conv_forward's own error
