"""Every form of the generic filter-gradient kernel (conv_wgrad_kernel of csrc/igemm.hip: 5 tile shapes x 5 view forms, split-K
into one of 4 reduce kernels) against the float64 reference of tests/wgrad_oracle.py under the any-order dot-product bound
(kernel_check.check_dot).  For every launch ssc_conv_wgrad_plan says which tile, split, view form and reduce kernel run; the
case asserts them, and the last test asserts that the table as a whole reached every one.

Every input is a view inside a larger device buffer that holds 1.0e3 on both sides, as the padding lanes do: a read past the
last pixel or a lane the kernel should have masked shows up as error.  The output lies inside a NaN buffer that must stay NaN
around it."""
import ctypes
import json
import os
import subprocess
import sys

import pytest
import torch

import wgrad_oracle as O
from conftest import parity_log
from kernel_check import NAN, all_nan, check_dot

pytestmark = pytest.mark.gpu

GUARD = 16384           # floats on either side of a tensor: more than a K-tile (32 pixel rows) of the widest side
TILES = ['128x128', '64x128', '128x64', '64x64', '128x32']
VIEWS = ['TTT', 'FTT', 'TTF', 'FTF', 'FFF']
REDUCES = ['none', 'reduce4', 'reduce<1>', 'reduce<4>', 'reduce<16>']
# cases the planner splits over the pixels on the MI355X: NULL and normal workspace, accumulate 0 and 1, each twice
SPLIT_CASES = ('t4_3x3x3x3', 't4_1x1_16_24', 't3_mm_48_40_p300', 't1_mm_dense_norm', 't0_3x3_two_gathered', 't0_conv_split')
# the tile a developer switch pins in this process (the child process of test_128x128_tile_in_a_pinned_process)
PINNED_TILE = int(os.environ['SSC_WG_CFG']) if os.environ.get('SSC_DEV_SWITCHES') == '1' and 'SSC_WG_CFG' in os.environ else None
REACHED = set()         # (tile, view form, reduce form) the query reported for the launches of this session
_REF = {}


def _hip():
    from sketchyscenecolorization_amd import hip
    return hip


def _reference(name):
    """Inputs and the float64 reference of a case: computed once, never modified."""
    if name not in _REF:
        c = O.BY_NAME[name]
        inp = O.make_inputs(c)
        ref, S = O.ref_taps(c, inp)
        _REF[name] = (inp, ref, S)
    return _REF[name]


def _inside(t, fill):
    """(buffer, view): a copy of the CPU tensor t inside a device buffer that holds `fill` on both sides."""
    buf = torch.full((GUARD + t.numel() + GUARD,), fill, device='cuda')
    view = buf[GUARD:GUARD + t.numel()].view(t.shape)
    view.copy_(t)
    return buf, view


def _view(hip, c, inp, side, keep):
    _, act, _, act1 = c[side + 't']
    dev = {}
    for k in ('0', '1', 'ab0', 'ab1'):
        t = inp[side + k]
        if t is None:
            dev[k] = None
        elif k in ('0', '1'):
            buf, dev[k] = _inside(t, O.PAD_LANE)
            keep.append(buf)
        else:
            dev[k] = t.cuda()
    return hip.View(dev['0'], dev['1'], dev['ab0'], act, dev['ab1'], act1)


def _desc(hip, c, gv, dv, out, accumulate):
    geo = O.geometry(c)
    d = hip.WgradDesc()
    d.g, d.d = gv.c(), dv.c()
    d.out = out.data_ptr()
    d.NB, d.PH, d.PW, d.TH, d.TW = geo['NB'], geo['PH'], geo['PW'], geo['TH'], geo['TW']
    d.in_stride, d.ioff_y, d.ioff_x = geo['stride'], geo['oy'], geo['ox']
    d.Cg_real, d.Nn, d.ldc, d.accumulate = c['g'][2], c['d'][2], c['d'][2], int(accumulate)
    d.exact = 0 if hip.ARITH_BF16 else 1
    return d


def _plan(hip, d, ws_bytes):
    out4 = (ctypes.c_int * 4)()
    assert hip.lib().ssc_conv_wgrad_plan(ctypes.byref(d), ws_bytes, out4) == 0
    return tuple(out4)


def _launch(hip, c, gv, dv, out, accumulate, d, null_ws):
    if null_ws:
        hip.check(hip.lib().ssc_conv_wgrad(ctypes.byref(d), None, 0, hip.stream_ptr()), 'ssc_conv_wgrad')
    elif c['kind'] == 'deconv':
        hip.deconv_wgrad(dv, gv, out, accumulate=accumulate)
    elif c['kind'] == 'mm' and gv.C1 == 0 and dv.C1 == 0 and dv.ab0 is None and dv.act == 0 and c['d'][2] == dv.C:
        M = gv.W
        hip.matmul_tn(gv.s0.view(M, gv.C0), dv.s0.view(M, dv.C0), out.view(out.shape[2], out.shape[3]), accumulate=accumulate,
                      a_ab=gv.ab0, a_act=gv.act)
    else:
        hip.conv_wgrad(gv, dv, out, c['stride'], -O.geometry(c)['oy'], accumulate=accumulate)
    torch.cuda.synchronize()


def _run(hip, c, inp, ref, S, null_ws, accumulate):
    """One launch: the plan the query reports for it, and the output."""
    name = c['name']
    keep = []
    gv, dv = _view(hip, c, inp, 'g', keep), _view(hip, c, inp, 'd', keep)
    base = torch.randn(ref.shape, generator=torch.Generator().manual_seed(7)) if accumulate else torch.full(ref.shape, NAN)
    obuf, out = _inside(base, NAN)
    d = _desc(hip, c, gv, dv, out, accumulate)
    ws_bytes = 0 if null_ws else hip.workspace().numel() * 4
    plan = _plan(hip, d, ws_bytes)
    tile, split, view, reduce = plan
    e = c['expect']
    tiles = e['tile'] if isinstance(e['tile'], tuple) else (e['tile'],)
    if PINNED_TILE is not None and PINNED_TILE in tiles:
        tiles = (PINNED_TILE,)
    assert tile in tiles and view == e['view'], (name, 'plan', plan, 'expected tile', tiles, 'view', e['view'])
    assert split >= 1 and (reduce == 0) == (split == 1), (name, plan)
    if null_ws:
        assert split == 1, (name, 'split-K without a workspace', plan)
    _launch(hip, c, gv, dv, out, accumulate, d, null_ws)
    for b in keep:      # the launch wrote nothing into its inputs or around them
        assert float(b[:GUARD].min()) == O.PAD_LANE and float(b[-GUARD:].max()) == O.PAD_LANE
    assert all_nan(obuf[:GUARD]) and all_nan(obuf[GUARD + out.numel():]), (name, 'a store outside the filter gradient')
    REACHED.add((tile, view, reduce))
    return plan, out.clone(), base


def _check(c, plan, got, base, ref, S, null_ws, accumulate):
    K = O.pixels(c)
    if accumulate:      # the base is one more term of every sum
        ref, S, K = ref + base.double(), S + base.double().abs(), K + 1
    cfg = dict(case=c['name'], ws='null' if null_ws else 'normal', accumulate=int(accumulate), tile=TILES[plan[0]], split=plan[1],
               view=VIEWS[plan[2]], reduce=REDUCES[plan[3]])
    if PINNED_TILE is not None:
        cfg['pinned'] = 'SSC_WG_CFG=%d' % PINNED_TILE
    check_dot('wgrad_forms', cfg, got, ref, S, K, plan=plan)


@pytest.mark.parametrize('name', [c['name'] for c in O.CASES])
def test_case(name):
    hip = _hip()
    c = O.BY_NAME[name]
    inp, ref, S = _reference(name)
    split_case = name in SPLIT_CASES
    variants = [(False, False), (True, True)] + ([(False, True), (True, False)] if split_case else [])
    for null_ws, accumulate in variants:
        plan, got, base = _run(hip, c, inp, ref, S, null_ws, accumulate)
        if split_case and not null_ws and PINNED_TILE is None:
            assert plan[1] > 1, (name, 'the planner no longer splits this case', plan)
        _check(c, plan, got, base, ref, S, null_ws, accumulate)
        if split_case:      # no atomics anywhere in this path: the same bits again
            plan2, got2, _ = _run(hip, c, inp, ref, S, null_ws, accumulate)
            assert plan2 == plan and torch.equal(got, got2), (name, 'two runs differ', plan)


def test_query_leaves_the_other_kernels_alone():
    """Tile id -1 for the launches wgrad128.hip and head1.hip take, as ssc_conv_wgrad_kernel_name names them."""
    hip = _hip()
    for ci, co, k, h in ((128, 256, 4, 20), (512, 1, 4, 23)):
        pad, stride = 1, (2 if co > 1 else 1)
        oh = (h + 2 * pad - k) // stride + 1
        x = torch.zeros(3, h, h, ci, device='cuda')
        dy = torch.zeros(3, oh, oh, max(co, 4), device='cuda')
        dw = torch.zeros(k, k, ci, co, device='cuda')
        d = hip.WgradDesc()
        d.g, d.d = hip.View(x).c(), hip.View(dy).c()
        d.out = dw.data_ptr()
        d.NB, d.PH, d.PW, d.TH, d.TW, d.in_stride, d.ioff_y, d.ioff_x = 3, oh, oh, k, k, stride, -pad, -pad
        d.Cg_real, d.Nn, d.ldc, d.accumulate = ci, co, co, 0
        buf = ctypes.create_string_buffer(64)
        hip.lib().ssc_conv_wgrad_kernel_name(ctypes.byref(d), buf, 64)
        assert not buf.value.decode().startswith('conv_wgrad<'), buf.value
        assert _plan(hip, d, hip.workspace().numel() * 4) == (-1, 1, 0, 0)
        # without a workspace the patch head's launch is the general kernel's (Nn = 1: the 128x32 tile), the large layer's is not
        assert _plan(hip, d, 0)[0] == (4 if co == 1 else -1)


def test_128x128_tile_in_a_pinned_process(tmp_path):
    """Where 128x128, 64x128 and 128x64 are all allowed the planner chooses by cost, and at these sizes never 128x128: those
    cases run once more in a process whose tile choice is pinned (SSC_WG_CFG=0, read once per process); its parity log must
    show that the query reported tile 0 for each of them.  Its records join this session's log."""
    names = [c['name'] for c in O.CASES if isinstance(c['expect']['tile'], tuple)]
    assert len(names) >= 5
    here = os.path.dirname(os.path.abspath(__file__))
    log = str(tmp_path / 'parity.jsonl')
    env = dict(os.environ, SSC_DEV_SWITCHES='1', SSC_WG_CFG='0', SSC_PARITY_LOG=log)
    r = subprocess.run([sys.executable, '-m', 'pytest', os.path.abspath(__file__), '-m', 'gpu', '-q', '-x', '-k', 'test_case and t0_'],
                       env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True, cwd=os.path.dirname(here))
    assert r.returncode == 0, r.stdout[-3000:]
    recs = [json.loads(l) for l in open(log)]
    for n in names:
        mine = [x for x in recs if x['config'].get('case') == n]
        assert mine and all(x['plan'][0] == 0 and x['config'].get('pinned') == 'SSC_WG_CFG=0' for x in mine), (n, mine)
    for x in recs:
        REACHED.add((x['plan'][0], x['plan'][2], x['plan'][3]))
        parity_log(x['test'], x['config'], x['max_abs_err'], x['bound'], variant='kernel', ratio=x['ratio'], K=x['K'], plan=x['plan'])


def test_zz_every_form_was_reached():
    """Runs last in the file: all 5 tiles, all 5 view forms -- each on at least two tiles -- and all 4 reduce kernels."""
    tiles = {t for t, _, _ in REACHED}
    assert tiles == {0, 1, 2, 3, 4}, sorted(REACHED)
    for v in range(5):
        on = {t for t, vv, _ in REACHED if vv == v}
        assert len(on) >= 2, (VIEWS[v], 'ran on tiles', sorted(on))
    assert {r for _, _, r in REACHED} == {0, 1, 2, 3, 4}, sorted(REACHED)
