"""Every form of the two bf16x6 forward kernels -- conv_bf_kernel<WM, WN, SM, SN, PLAIN, ONE, KM, SS> (32-k stages) and
conv_bfh_kernel<WM, WN, PLAIN, ONE, KM> (the 128 x 128 tile on 16-k stages), csrc/igemm_bf16.hip -- against the float64 reference
of tests/fwd_oracle.py under the any-order dot-product bound (kernel_check.check_dot with extra_terms=2), per element:

    |got - ref| <= (K + 10) * 2^-24 * S

K the non-zero products of the element (+ 1 for a bias, + 1 for an accumulate base: each one more term of ref and S), S the
float64 sum of the absolute products.  The 3-way split x = h + m + l of both operands is exact; the three dropped products
(m*l, l*m, l*l) are together below 2^-23 |a*b|: two more roundings per term.  K slices and split-K slabs are
only another summation tree and cost nothing extra.  Nothing in the bound is measured; it assumes that each addition in the
matrix pipe errs by at most one fp32 rounding of its result.  The forward kernels' two-accumulator K loop keeps that: the h*h
products go into one accumulator (K / 16 additions of 16 exact bf16 products each), the five correction products into a second
one whose values -- and therefore roundings -- are 2^-8 of the first's and below, and the two are added once behind the loop: far
fewer roundings of the large value than the K + 8 the bound pays for.
An activated epilogue (epi 1 tanh, 2 lrelu 0.2) is 1-Lipschitz: the same bound holds behind it, plus 8 * 2^-24 * |f(ref)| for the
evaluation of f itself (tanhf four ulp: the allowance of kernel_check.check_fp32).

At K in the hundreds that bound is wider than one lost correction product (a missing h*l pass costs ~2^-16 |a*b| per term), so
every kernel, source form and PLAIN value also runs two probes whose outputs are sums of ONE product (a 1x1 conv over a tensor
with one non-zero channel per pixel: the bound is 11 * 2^-24 * |a*b|) and of at most nine (a 3x3 conv over a tensor with one
non-zero channel in all, through the tap walk).  tests/test_fwd_oracle.py shows on the CPU that a float32 chain passes them and
that a filter without its third plane does not.

Every launch goes through the hip.py wrapper with hip.ARITH_BF16 set.  In front of it ssc_conv_bf_plan -- computed by the
functions that make the launch -- says which kernel runs and in which form: {kernel, tile, PLAIN, source form, SS, korder, grid
layout, split-K slabs, whole tiles, K slices}; the case asserts what it expects of them (for the MI355X's 256 CUs), and
ssc_conv_forward_kernel_name must agree.  The last test asserts that parent and child processes together reached every
instantiation ssc_launch_conv_bf can select.  (The edges of fwd_is_bf are asked through the query on the CPU:
tests/test_fwd_oracle.py.)  The forms the planner does not choose by itself at small shapes -- a pinned tile
(SSC_FWD_CFG), the 32-k 128 x 128 tile (SSC_BF_HK=0), in-launch K slices of 4 and 8 (SSC_TS_FORCE) -- run in child processes.

Every input source is a view inside a larger device buffer that holds 1.0e3 on both sides, as the padding lanes do (or NaN); the
output lies inside a NaN buffer.  After the launch the inputs and their guards are unchanged, the output columns outside
[coff, coff + Nstore) of every row hold what they held, columns [Nn, Nstore) are exactly 0 and no hand-off timed out."""
import ctypes
import json
import os
import subprocess
import sys

import pytest
import torch

import fwd_oracle as O
from conftest import parity_log
from kernel_check import GUARD, NAN, U_FP32, all_nan, check_dot
from kernel_check import bits as _bits, inside as _inside

pytestmark = pytest.mark.gpu

TILE = {0: (128, 128), 1: (64, 128), 2: (128, 64), 4: (64, 64)}
NAMES = {0: 'conv_bf16x6<128x128>', 1: 'conv_bf16x6<64x128>', 2: 'conv_bf16x6<128x64>', 4: 'conv_bf16x6<64x64>'}
_CARRIERS = [O.carrier(*f)['name'] for f in O.CARRIER_FORMS]
_PROBES = [O.probe(*f)['name'] for f in O.PROBE_FORMS]
# Child processes: the switches a process reads once, the tile they pin (None: the planner's), and what runs there -- (test,
# case, expected grid layout).  test 'form': test_form; 'stage': test_one_stage (CO_RUN: one LDS stage, the 32-k tiles).
# (the planner cuts the carriers' 18 to 27 K-tiles into split-K slabs under every tile: layout 4; the one-hot probes have one or two)
_PINNED = [('form', n, 4) for n in _CARRIERS] + [('form', n, 0) for n in _PROBES[:6]]
_STAGES = [('stage', n, 4) for n in _CARRIERS]
CHILDREN = {
    # the 128 x 128 tile on 16-k stages (conv_bfh_kernel): every source form, korder, layout 0 / 1 / 2 / 4, orientation, accumulate
    'cfg0': (dict(SSC_FWD_CFG='0'), 0, _PINNED + [('form', 'probe_channel_two_T', 4), ('form', 'probe_channel_km_P', 4),
             ('form', 'g_4x4s2_odd', 4), ('form', 'km_68_67_4x4s2', 4), ('form', 'l_xcd_1x1_acc', 1), ('form', 't_deconv_32_nn132', 2), ('form', 'l_slabs_dgrad_acc', 4)]),
    'cfg1': (dict(SSC_FWD_CFG='1'), 1, _PINNED + _STAGES),
    'cfg2': (dict(SSC_FWD_CFG='2'), 2, _PINNED + _STAGES),
    'cfg4': (dict(SSC_FWD_CFG='4'), 4, _PINNED + _STAGES),
    # the 128 x 128 tile on 32-k stages (conv_bf_kernel<2, 2, 2, 2>)
    'hk0': (dict(SSC_DEV_SWITCHES='1', SSC_BF_HK='0', SSC_FWD_CFG='0'), 0, _PINNED + [('form', 'g_4x4s2_odd', 4), ('form', 'l_slabs_4x4', 4)]),
    # K slices inside the launch, no whole tiles: 4 per tile on the 16-k kernel, 8 per tile on the 64 x 128 tile.  Where a range
    # begins in the middle of a tap row (korder 1) or of a parity class (korder 2), kt_decode hands over to kt_advance in mid
    # walk: _mid_start works that out for every launch and the last test asserts it happened for both orders in both kernels.
    # With 4x4 taps a class is 4 K-tiles and 4 slices of 16 * tpt K-tiles always begin at a class, so the korder-2 ranges in mid
    # class are km_68_67_4x4s2's: 12 slabs of 7 of its 80 16-k K-tiles under cfg0, 8 slices of 6 of its 48 32-k K-tiles under ts8
    # (and l_xcd_4x4s2_nk's 8 slices of 2).
    'ts4': (dict(SSC_TS_FORCE='0,4', SSC_FWD_CFG='0'), 0, [('form', n, 3) for n in (
        'carrier_two_T', 'carrier_km_P', 'g_4x4s2_odd', 'g_4x4s2_same_asym', 't_deconv_two', 'd_dgrad_4x4_same_acc', 'g_nk_3x3',
        'd_deconv_dgrad_noff32', 'probe_channel_one_P', 'g_fc')]),
    'ts8': (dict(SSC_TS_FORCE='0,8', SSC_FWD_CFG='1'), 1, [('form', n, 3) for n in (
        'carrier_two_T', 'carrier_km_P', 'carrier_one_T', 'g_4x4s2_odd', 'g_4x4s2_same_asym', 't_deconv_two', 'd_dgrad_4x4_same_acc',
        'g_nk_3x3', 'd_deconv_dgrad_noff32', 'probe_channel_two_P', 'l_xcd_4x4s2_nk', 'km_68_67_4x4s2')]),
}
CHILD = os.environ.get('SSC_FWD_FORMS_CHILD')       # set by test_child_process for the process it starts, never in this one
REACHED = set()         # (kernel, tile, PLAIN, source form, SS, korder, layout, bmode, accumulate) of this session's launches
MID = set()             # (kernel, korder) of the launches with a K range that begins in the middle of a tap class / a tap row
REDUCE = set()          # of the launches with slabs: 1 summed by slab_reduce4_kernel, 0 by slab_reduce_kernel
_REF = {}


def _hip():
    from sketchyscenecolorization_amd import hip
    return hip


def _reference(c):
    """Inputs and the float64 reference of a case: computed once, shared by all its variants, never modified."""
    if c['name'] not in _REF:
        inp = O.make_inputs(c)
        _REF[c['name']] = (inp,) + O.ref_taps(c, inp)
    return _REF[c['name']]


def _plan(hip, d, ws_bytes):
    """(return code, the ten values)."""
    out10 = (ctypes.c_int * 10)(*([-99] * 10))
    rc = hip.lib().ssc_conv_bf_plan(ctypes.byref(d), ws_bytes, out10)
    return rc, tuple(out10)


class _Spy(object):
    """Stands in front of ssc_conv_forward while a wrapper runs: the descriptor the wrapper made is handed to `before`, which
    asks the plan query and asserts, and then to the library."""

    def __init__(self, hip, before):
        self.lib, self.before, self.calls = hip.lib(), before, 0

    def __enter__(self):
        self.real = self.lib.ssc_conv_forward
        self.lib.ssc_conv_forward = self
        return self

    def __exit__(self, *exc):
        self.lib.ssc_conv_forward = self.real

    def __call__(self, dref, ws, ws_bytes, stream):
        self.calls += 1
        self.before(dref._obj, getattr(ws, 'value', ws) or 0, ws_bytes if ws else 0)
        return self.real(dref, ws, ws_bytes, stream)


def _mid_start(d, plan):
    """1 when a K slice or slab of the launch begins where kt_decode hands over to kt_advance in mid walk.  For korder 1 and 2
    the K-tile sequence is chunk-major, kt = chunk * ntaps + sidx, over tpt chunks of 32 (conv_bf_kernel) or 16 (conv_bfh_kernel)
    channels per source; range ks begins at ks * ceil(nkt / ranges).  korder 2 walks the taps in four parity classes of
    ntaps / 4: in the middle of a class when sidx % (ntaps / 4) != 0; korder 1 row by row: in mid row when sidx % TW != 0."""
    kernel, korder, lay, slabs, slices = plan[0], plan[5], plan[6], plan[7], plan[9]
    ranges = slices if lay == 3 else slabs
    if korder == 0 or ranges <= 1:
        return 0
    ck = 16 if kernel else 32
    ntaps, nkt = d.TH * d.TW, d.TH * d.TW * (-(-d.x.C0 // ck) + d.x.C1 // ck)
    per = -(-nkt // ranges)
    unit = ntaps // 4 if korder == 2 else d.TW
    return int(any((b % ntaps) % unit for b in range(per, nkt, per)))


def _reduce4(d, ws):
    """launch_slab_reduce's choice (igemm.hip) for a launch with slabs and no statistics rider: 1 slab_reduce4_kernel (float4:
    every count a multiple of 4, every pointer 16-byte aligned), 0 the scalar slab_reduce_kernel."""
    assert not d.stat_partial
    out_count = d.NB * d.OH * d.OW * d.ldc
    return int(out_count % 4 == 0 and d.ldc % 4 == 0 and d.Nn % 4 == 0 and d.Nstore % 4 == 0 and
               ((ws | (d.out or 0) | (d.bias or 0)) & 15) == 0)


def _wrapper(hip, c, dev, out):
    """The hip.py wrapper of the case's op."""
    kind, geo = c['kind'], O.geometry(c)
    _, act, _, act1 = c['tf']
    v = hip.View(dev['s0'], dev['s1'], dev['ab0'], act, dev['ab1'], act1)
    if kind == 'conv':
        same = c['pad'] == 'same'
        hip.conv_forward(v, dev['w'], c['stride'], 0 if same else c['pad'], out, coff=c['coff'], nstore=c['nstore'], bias=dev['bias'],
                         epi=c['epi'], accumulate=c['acc'], same=same, w_nk=dev['w_nk'])
    elif kind == 'deconv':
        hip.deconv_forward(v, dev['w'], out, coff=c['coff'], nstore=c['nstore'], epi=c['epi'])
    elif kind == 'conv_dgrad':
        hip.conv_dgrad(v, dev['w'], c['stride'], geo.get('pad_before', c['pad']), out, n_off=c['n_off'], nn=geo['nn'],
                       nstore=c['nstore'], accumulate=c['acc'], coff=c['coff'])
    elif kind == 'deconv_dgrad':
        hip.deconv_dgrad(v, dev['w'], out, n_off=c['n_off'], nn=geo['nn'], accumulate=c['acc'])
    elif kind == 'matmul':
        hip.matmul(dev['s0'].view(c['w'], -1), dev['w'], out.view(c['w'], -1), bias=dev['bias'], accumulate=c['acc'], a_ab=dev['ab0'],
                   a_act=act)
    else:
        assert kind == 'matmul_nt'
        hip.matmul_nt(dev['s0'].view(c['w'], -1), dev['w'], out.view(c['w'], -1), accumulate=c['acc'])


def _expected(c, layout):
    """What the plan must say: (tile or None, PLAIN, source form, korder, layout)."""
    C0, C1, _ = c['src']
    src = 0 if C1 else (2 if C0 % 32 else 1)
    tile = c['expect'].get('tile')
    nstore = c['nstore'] or O.geometry(c)['nn']
    if CHILD:           # the pinned tile where the planner allows it: the 128-column tiles from 65 stored columns on
        tile = CHILDREN[CHILD][1]
        if tile in (0, 1) and nstore <= 64:
            tile = None
    return tile, int(c['tf'] == O.PLAIN), src, c['expect']['korder'], layout


def _run(hip, c, inp, layout, corun=False):
    """One launch: the plan the query reports for it in front of the launch, and the output [n, OH, OW, nn] (Nstore columns
    checked and cut to Nn)."""
    name, geo = c['name'], O.geometry(c)
    nn = geo['nn']
    nstore, coff = c['nstore'] or nn, c['coff']
    ldc = c['ldc'] or (coff + nstore)
    assert nn <= nstore and coff + nstore <= ldc
    keep, dev = [], {}
    for k in ('s0', 's1'):
        dev[k] = None
        if inp[k] is not None:
            buf, dev[k] = _inside(inp[k], O.PAD_LANE)
            keep.append((buf, buf.clone()))
    for k in ('ab0', 'ab1', 'w', 'bias'):
        dev[k] = inp[k].cuda() if inp[k] is not None else None
    dev['w_nk'] = inp['w'].permute(0, 1, 3, 2).contiguous().cuda() if c['nk'] else None
    if c['acc']:        # what the output tensor holds before the launch: the base in the launch's columns, more noise around them
        held = torch.randn((c['n'], geo['OH'], geo['OW'], ldc), generator=torch.Generator().manual_seed(7))
        held[..., coff:coff + nn] = inp['base']
    else:
        held = torch.full((c['n'], geo['OH'], geo['OW'], ldc), NAN)
    obuf, out = _inside(held, NAN)
    seen = []

    def before(d, ws, ws_bytes):
        rc, plan = _plan(hip, d, ws_bytes)
        assert rc == 0, (name, 'ssc_conv_bf_plan', rc)
        kernel, tile, plain, src, ss, korder, lay, slabs, whole, slices = plan
        e_tile, e_plain, e_src, e_korder, e_layout = _expected(c, layout)
        assert (plain, src, korder, lay) == (e_plain, e_src, e_korder, e_layout) and tile in TILE and (e_tile is None or tile == e_tile), \
            (name, CHILD, 'plan', plan, 'expected tile, PLAIN, source form, korder, layout', _expected(c, layout))
        assert kernel == int(tile == 0 and CHILD != 'hk0') and ss == int(corun and tile != 0), (name, CHILD, plan)
        assert d.lds_hint == int(corun) and d.ws_kc > 0 and d.wsplit, (name, 'the wrapper attached no filter planes')
        BM, BN = TILE[tile]
        tiles = -(-(d.NB * d.PH * d.PW) // BM) * -(-d.Nstore // BN) * d.nphase
        assert (slabs > 1) == (lay == 4) and (slices > 1) == (lay == 3) and whole == (tiles if lay != 3 else whole), (name, plan, tiles)
        wgs = tiles * slabs if lay != 3 else whole + (tiles - whole) * slices
        if CHILD in ('ts4', 'ts8'):     # every workgroup resident: no owner waits for a workgroup that was not dispatched
            assert lay == 3 and whole == 0 and slices == int(CHILD[2]) and wgs <= 256, (name, CHILD, plan, wgs)
        if not CHILD:       # the parent's split layouts: as many slabs / whole tiles and slices as the case says
            want = (c['expect'].get('slabs', 1), c['expect'].get('whole', tiles), c['expect'].get('slices', 1))
            assert (slabs, whole, slices) == want and (lay in (3, 4)) == (want != (1, tiles, 1)), (name, plan, want)
        assert hip._kernel_name('ssc_conv_forward_kernel_name', d) == NAMES[tile], (name, plan)
        seen.append((plan, d.bmode, d.accumulate, _mid_start(d, plan), _reduce4(d, ws) if lay == 4 else -1))

    saved = hip.ARITH_BF16, hip.CO_RUN
    hip.ARITH_BF16, hip.CO_RUN = True, corun
    try:
        with _Spy(hip, before) as spy:
            _wrapper(hip, c, dev, out)
        torch.cuda.synchronize()
    finally:
        hip.ARITH_BF16, hip.CO_RUN = saved
    assert spy.calls == 1 and len(seen) == 1, (name, spy.calls)
    plan, bmode, acc, mid, red4 = seen[0]
    assert acc == int(c['acc'])
    assert hip.sk_timeouts() == 0, (name, 'a hand-off timed out')
    for buf, before_bits in keep:       # the launch wrote nothing into its inputs or around them
        assert torch.equal(_bits(buf), _bits(before_bits)), (name, 'an input or its guard changed')
    assert all_nan(obuf[:GUARD]) and all_nan(obuf[GUARD + out.numel():]), (name, 'a store outside the output tensor')
    heldd = held.cuda()
    for lo, hi in ((0, coff), (coff + nstore, ldc)):
        assert torch.equal(_bits(out[..., lo:hi].contiguous()), _bits(heldd[..., lo:hi].contiguous())), \
            (name, 'a store outside the columns of the launch', lo, hi)
    assert bool((out[..., coff + nn:coff + nstore] == 0).all()), (name, 'columns [Nn, Nstore) are not zero')
    REACHED.add(plan[:7] + (bmode, acc))
    if mid:
        MID.add((plan[0], plan[5]))
    if red4 >= 0:
        REDUCE.add(red4)
    return plan, out[..., coff:coff + nn].clone(), dict(bmode=bmode, mid_start=mid, reduce4=red4)


def _check(c, plan, got, launch, ref, S, K, corun=False):
    cfg = dict(launch, case=c['name'], accumulate=int(c['acc']), corun=int(corun))
    if CHILD:
        cfg['child'] = CHILD
    if c['epi']:
        f = O.epilogue(c, ref)
        check_dot('fwd_bf16_forms', cfg, got, f, S, K, plan=plan, extra_terms=2, allow=8 * U_FP32 * f.abs())
    else:
        check_dot('fwd_bf16_forms', cfg, got, ref, S, K, plan=plan, extra_terms=2)


def _layout(test, name):
    """The grid layout the case must plan: its own in the parent process, the child's table in a child."""
    if not CHILD:
        return O.lookup(name)['expect']['layout']
    mine = [l for t, n, l in CHILDREN[CHILD][2] if (t, n) == (test, name)]
    assert len(mine) == 1, (CHILD, test, name, 'not a case of this child process')
    return mine[0]


_FORM_PARAMS = [c['name'] for c in O.all_cases()]


@pytest.mark.parametrize('name', _FORM_PARAMS)
def test_form(name):
    hip = _hip()
    c = O.lookup(name)
    inp, ref, S, K = _reference(c)
    layout = _layout('form', name)
    plan, got, launch = _run(hip, c, inp, layout)
    _check(c, plan, got, launch, ref, S, K)
    if plan[6] in (3, 4):       # no atomics anywhere in the split paths: the same bits again
        plan2, got2, _ = _run(hip, c, inp, layout)
        assert plan2 == plan and torch.equal(got, got2), (name, 'two runs differ', plan)


@pytest.mark.parametrize('name', _CARRIERS)
def test_one_stage(name):
    """hip.CO_RUN: the launch says it shares the chip (lds_hint) and the 32-k tiles take one LDS stage per operand (SS).  The
    summation order is the same: the output must equal the two-stage one bit for bit, as the planner's comment promises."""
    hip = _hip()
    c = O.lookup(name)
    inp, ref, S, K = _reference(c)
    layout = _layout('stage', name)
    plan, got, _ = _run(hip, c, inp, layout)
    plan1, got1, launch = _run(hip, c, inp, layout, corun=True)
    assert plan[1] != 0 and plan1[4] == 1 and plan1[:4] + plan1[5:] == plan[:4] + plan[5:], (name, plan, plan1)
    _check(c, plan1, got1, launch, ref, S, K, corun=True)
    assert torch.equal(got, got1), (name, 'one LDS stage changed the result', plan1)


def _key(x):
    return tuple(x['plan'][:7]) + (x['config']['bmode'], x['config']['accumulate'])


@pytest.mark.parametrize('child', sorted(CHILDREN))
def test_child_process(child, tmp_path):
    """The forms behind switches a process reads once, each in a fresh pytest process on this file with a selection of about a
    dozen cases (CHILDREN).  The child asserts its own plans; its parity log must show the pinned form on every launch, and its
    records join this session's."""
    if CHILD:
        return
    env_add, tile, tests = CHILDREN[child]
    here = os.path.dirname(os.path.abspath(__file__))
    log = str(tmp_path / 'parity.jsonl')
    env = dict(os.environ, SSC_PARITY_LOG=log, SSC_FWD_FORMS_CHILD=child, **env_add)
    sel = ' or '.join('test_%s[%s]' % ('form' if t == 'form' else 'one_stage', n) for t, n, _ in tests)
    r = subprocess.run([sys.executable, '-m', 'pytest', os.path.abspath(__file__), '-m', 'gpu', '-q', '-x', '-k', sel],
                       env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True, cwd=os.path.dirname(here))
    assert r.returncode == 0, r.stdout[-3000:]
    recs = [json.loads(l) for l in open(log)]
    recs = [x for x in recs if x['test'] == 'fwd_bf16_forms']
    assert {x['config']['case'] for x in recs} == {n for _, n, _ in tests}, sorted({x['config']['case'] for x in recs})
    for x in recs:
        assert x['config'].get('child') == child, x
        if child in ('cfg0', 'hk0', 'ts4'):
            assert x['plan'][1] == 0 and x['plan'][0] == int(child != 'hk0'), x
        if child in ('ts4', 'ts8'):
            assert x['plan'][6] == 3 and x['plan'][9] == int(child[2]), x
        REACHED.add(_key(x))
        if x['config']['mid_start']:
            MID.add((x['plan'][0], x['plan'][5]))
        if x['config']['reduce4'] >= 0:
            REDUCE.add(x['config']['reduce4'])
        parity_log(x['test'], x['config'], x['max_abs_err'], x['bound'], variant='kernel', ratio=x['ratio'], K=x['K'], plan=x['plan'])
    assert any(x['plan'][1] == tile for x in recs)


def test_zz_every_form_was_reached():
    """Runs last in the file.  Every instantiation ssc_launch_conv_bf can select, and per kernel every K-tile order, grid
    layout, filter orientation and accumulate value, over the parent process and its children together.
    Not reachable, by the code: SS on a 128 x 128 tile (bf_form: f.ss = cfg != 0 && ..., and the 32-k 128 x 128 tile is
    launch_bf_form<2, 2, 2, 2, false>); the 128 x 32 tile (plan_fwd: allowed_bf[3] = false, ssc_launch_conv_bf answers -4); of the
    kernels that sum slabs, slab_reduce4_stats_kernel (launch_slab_reduce: `d.stat_partial != nullptr && ...`, a pointer only
    the batch-statistics rider ssc_conv_forward_bn sets; ssc_conv_forward's own launches get slab_reduce4_kernel or
    slab_reduce_kernel, and both must have run).
    Per kernel, too: a K slice or slab that begins in the middle of a tap row (korder 1) and one that begins in the middle of a
    parity class (korder 2), where kt_decode hands over to kt_advance (_mid_start)."""
    if CHILD:
        return      # a child process runs a part of the table; the parent asserts over all
    R = REACHED
    for plain in (0, 1):
        for src in (0, 1, 2):
            for kernel in (1, 0):       # conv_bfh_kernel, and the 32-k 128 x 128 tile
                assert any(r[:5] == (kernel, 0, plain, src, 0) for r in R), ('128x128, kernel', kernel, plain, src, sorted(R))
            for tile in (1, 2, 4):
                for ss in (0, 1):
                    assert any(r[:5] == (0, tile, plain, src, ss) for r in R), ('tile', tile, plain, src, 'SS', ss, sorted(R))
    assert not any(r[1] == 0 and r[4] for r in R)
    for kernel in (0, 1):
        mine = [r for r in R if r[0] == kernel]
        for korder in (0, 1, 2):
            assert any(r[5] == korder for r in mine), ('kernel', kernel, 'korder', korder, sorted(mine))
        for layout in (0, 1, 2, 3, 4):
            assert any(r[6] == layout for r in mine), ('kernel', kernel, 'layout', layout, sorted(mine))
        for bmode in (0, 1):
            assert any(r[7] == bmode for r in mine), ('kernel', kernel, 'orientation', bmode, sorted(mine))
        for acc in (0, 1):
            assert any(r[8] == acc for r in mine), ('kernel', kernel, 'accumulate', acc, sorted(mine))
        for korder in (1, 2):
            assert (kernel, korder) in MID, ('kernel', kernel, 'korder', korder, 'no K range begins in mid walk', sorted(MID))
    assert REDUCE == {0, 1}, ('slabs summed by slab_reduce4_kernel (1) and slab_reduce_kernel (0)', sorted(REDUCE))
