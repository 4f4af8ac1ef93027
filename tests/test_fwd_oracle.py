"""The float64 reference of the forward bf16x6 tests (tests/fwd_oracle.py) against itself, the probes' float32 chain against
their bound, the comparison rule (kernel_check.check_dot) against results that lost a plane or a term, and the edges of the
library's fwd_is_bf predicate through the host-only plan query.  No GPU."""
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


def test_every_case_has_a_seed_of_its_own():
    seeds = [c['seed'] for c in _ALL]
    assert len(set(seeds)) == len(seeds) and len({c['name'] for c in _ALL}) == len(_ALL)


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
