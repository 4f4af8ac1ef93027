"""Which kernel a launch takes and with which plan, pinned: the library's host-only queries (kernel name, forward plan, bf16x6
plan, filter-gradient plans, every *_supported predicate) over a fixed list of descriptors, compared with
tests/golden/dispatch_table.json; the SSC_DEV_SWITCHES gate in front of a developer switch and of a planner constant; the
switch list of DESIGN.md section 7 against the names the code reads.  No GPU: the queries launch nothing, the descriptors are
made of dummy aligned pointers, and the planner takes 256 CUs where it finds no device.

Switches are read once per process, so every query runs in a child process of its own environment (all started together).
`python tests/test_dispatch_table.py --write` regenerates the fixture from the library that SSC_LIB_PATH names (with
SSC_ALLOW_STALE_LIB=1 a build of other sources: the fixture in the tree was written by the build of the commit before the
switches were retired)."""
import ctypes as C
import json
import os
import re
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLDEN = os.path.join(HERE, 'golden', 'dispatch_table.json')
WS = 256 << 20

# every kernel ssc_conv_forward / ssc_conv_wgrad dispatch in front of (or instead of) the exact-fp32 tiles
SPECIALISED = ['head1_fwd', 'head1_dgrad', 'head1_wgrad', 'narrow_fwd<conv>', 'narrow_fwd<transposed>', 'conv_fewchan<4>',
               'conv_fewchan<8>', 'conv_fewchan7', 'conv_pw1x1', 'conv_c3x3<KN>', 'conv_c3x3<NK>', 'conv_s2n16', 'deconv_tr4n16',
               'deconv_tr4_tiny', 'conv_wgn16<3x3>', 'conv_wgn16<4x4>', 'conv_wgrad128<128x128>', 'conv_wgrad128_bf16x6<128x128>',
               'conv_bf16x6<128x128>', 'conv_bf16x6<64x128>']

RETIRED = ['SSC_PW1X1', 'SSC_HEAD1', 'SSC_C3X3', 'SSC_C3X3_N16', 'SSC_S2N16', 'SSC_TR4N16', 'SSC_TR4_TINY', 'SSC_FEWCHAN',
           'SSC_FEWCHAN7', 'SSC_WGN16', 'SSC_WGRAD128', 'SSC_WGRAD_BF16', 'SSC_ROWTAP', 'SSC_UTG', 'SSC_SLAB_STATS',
           'SSC_FUSE_STATS', 'SSC_FUSE_BNBWD', 'SSC_FUSE_MINMAX', 'SSC_WG128_XCD', 'SSC_WG128_SPAN', 'SSC_LSTM_K2', 'SSC_FOLD_WPC',
           'SSC_UTG_WASTE', 'SSC_TS_MAXS', 'SSC_PLAN_BF_SCALE', 'SSC_WG128_OCC1', 'SSC_WG_SPLITK', 'SSC_DEBUG_BNPATH',
           'SSC_DIAG_SKIP_WGRAD_REDUCE', 'SSC_SPLIT_ALWAYS', 'SSC_BF_PARTIAL', 'SSC_WGRAD_SIDE_PIXELS', 'SSC_ADMA', 'SSC_BDMA',
           'SSC_UT_SGB', 'SSC_WG128_BK']

CONV_PREDICATES = ['ssc_head1_forward_supported', 'ssc_head1_dgrad_supported', 'ssc_conv_narrow_supported',
                   'ssc_conv_fewchan_supported', 'ssc_conv_pw1x1_supported', 'ssc_conv_c3x3_supported', 'ssc_conv_s2n16_supported',
                   'ssc_conv_tr4_tiny_supported', 'ssc_conv_fewchan7_supported', 'ssc_conv_tr4n16_supported']
WGRAD_PREDICATES = ['ssc_head1_wgrad_supported', 'ssc_conv_wgrad128_supported', 'ssc_conv_wgn16_supported']


# ---- descriptors (the forms of hip.conv_forward, deconv_forward, conv_dgrad, conv_wgrad, deconv_wgrad) ----
def _p(i):
    return i << 32      # distinct, 16-byte aligned, never dereferenced


def _view(hip, C0, C1, H, W, act=0, ab=False):
    v = hip.GView()
    v.s0, v.s1, v.ab0, v.ab1 = _p(1), (_p(2) if C1 else None), (_p(3) if ab else None), (_p(4) if ab and C1 else None)
    v.C0, v.C1, v.H, v.W, v.act, v.act1 = C0, C1, H, W, act, -1
    return v


def _finish(hip, d, flags, planes):
    d.w, d.bias, d.out = _p(5), None, _p(6)
    d.sk_flags = _p(7) if flags else None
    if planes:      # the filter's bf16 planes, as hip._attach_split sets them
        kc, nbp = C.c_int(0), C.c_int(0)
        assert hip.lib().ssc_filter_split_geom(d.KH * d.KW, d.wC0, d.wC1, 1 if d.bmode else 0, C.byref(kc), C.byref(nbp), None, None) == 0
        d.wsplit, d.ws_kc, d.ws_nbp = _p(8), kc.value, nbp.value
    return d


def conv(hip, N, H, W, C0, C1, k, stride, pad, co, k_real=None, act=0, ab=False, flags=True, planes=False, same=False):
    """pad: padding before; same: tf SAME, ceil(in / stride) outputs (the extra padding element goes after)."""
    d = hip.ConvDesc()
    d.x = _view(hip, C0, C1, H, W, act, ab)
    d.NB, d.PH, d.PW = N, (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    if same:
        d.PH, d.PW = -(-H // stride), -(-W // stride)
    d.TH, d.TW, d.in_stride, d.ioff_y, d.ioff_x, d.nphase = k, k, stride, -pad, -pad, 1
    d.ky0, d.kx0, d.kstep = 0, 0, 1
    ci = C0 + C1 if k_real is None else k_real
    d.KH, d.KW, d.wC0, d.wC1, d.bmode, d.k_real = k, k, ci, co, 0, ci
    d.n_off, d.Nn, d.Nstore = 0, co, co
    d.OH, d.OW, d.ldc, d.out_stride, d.ooff_y, d.ooff_x = d.PH, d.PW, co, 1, 0, 0
    return _finish(hip, d, flags, planes)


def deconv(hip, N, H, W, C0, C1, co, k_real=None, act=0, ab=False, flags=True, planes=False):
    d = hip.ConvDesc()
    d.x = _view(hip, C0, C1, H, W, act, ab)
    d.NB, d.PH, d.PW = N, H, W
    d.TH, d.TW, d.in_stride, d.ioff_y, d.ioff_x, d.nphase = 2, 2, 1, 0, 0, 4
    d.ky0, d.kx0, d.kstep = 0, 0, -2
    ci = C0 + C1 if k_real is None else k_real
    d.KH, d.KW, d.wC0, d.wC1, d.bmode, d.k_real = 4, 4, co, ci, 1, ci
    d.n_off, d.Nn, d.Nstore = 0, co, co
    d.OH, d.OW, d.ldc, d.out_stride, d.ooff_y, d.ooff_x = 2 * H, 2 * W, co, 2, 0, 0
    return _finish(hip, d, flags, planes)


def dgrad1(hip, N, OH, OW, Cdy, k, pad, ci, k_real=None, flags=True, planes=False):
    """Data gradient of a stride-1 k x k conv ci -> Cdy (dy as large as the input: SAME)."""
    d = hip.ConvDesc()
    d.x = _view(hip, Cdy, 0, OH + 2 * pad - k + 1, OW + 2 * pad - k + 1)
    d.NB, d.PH, d.PW, d.TH, d.TW, d.in_stride, d.nphase, d.kstep, d.out_stride = N, OH, OW, k, k, 1, 1, -1, 1
    d.ky0 = d.kx0 = k - 1
    d.ioff_y = d.ioff_x = pad - (k - 1)
    d.KH, d.KW, d.wC0, d.wC1, d.bmode = k, k, ci, (Cdy if k_real is None else k_real), 1
    d.k_real = Cdy if k_real is None else k_real
    d.n_off, d.Nn, d.Nstore = 0, ci, ci
    d.OH, d.OW, d.ldc, d.ooff_y, d.ooff_x = OH, OW, ci, 0, 0
    return _finish(hip, d, flags, planes)


def wgrad(hip, N, PH, PW, g, dd, k, stride, pad, Cg_real, Nn, exact=0):
    d = hip.WgradDesc()
    d.g, d.d, d.out = g, dd, _p(6)
    d.NB, d.PH, d.PW = N, PH, PW
    d.TH, d.TW, d.in_stride, d.ioff_y, d.ioff_x = k, k, stride, -pad, -pad
    d.Cg_real, d.Nn, d.ldc, d.accumulate, d.exact = Cg_real, Nn, Nn, 0, exact
    return d


def conv_wgrad(hip, N, H, W, C0, C1, k, stride, pad, co, exact=0, act=0, ab=False, Cg_real=None):
    PH, PW = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    return wgrad(hip, N, PH, PW, _view(hip, C0, C1, H, W, act, ab), _view(hip, co, 0, PH, PW), k, stride, pad,
                 C0 + C1 if Cg_real is None else Cg_real, co, exact)


def deconv_wgrad(hip, N, H, W, C0, C1, co, exact=0):
    """Filter gradient of the k = 4 stride-2 transposed conv C0 + C1 -> co: dy [N,2H,2W,co] is the gathered side."""
    return wgrad(hip, N, H, W, _view(hip, co, 0, 2 * H, 2 * W), _view(hip, C0, C1, H, W, 1), 4, 2, 1, co, C0 + C1, exact)


# the conv layers of the Pix2Pix train step as scripts/plan_table.py lists them: (name, PH, PW, C0, C1, Nn, transposed)
PIX2PIX = [('enc2', 48, 48, 64, 0, 128, 0), ('enc3', 24, 24, 128, 0, 256, 0), ('enc4', 12, 12, 256, 0, 512, 0),
           ('enc5', 6, 6, 512, 0, 512, 0), ('dec5', 6, 6, 512, 64, 512, 1), ('dec4', 12, 12, 512, 512, 256, 1),
           ('dec3', 24, 24, 256, 256, 128, 1), ('dec2', 48, 48, 128, 128, 64, 1), ('d_l4', 23, 23, 256, 0, 512, 0)]


def conv_cases(hip):
    """[(name, descriptor)]: forward-form launches."""
    cs = []
    for name, PH, PW, C0, C1, Nn, tr in PIX2PIX:      # batch 32; with / without hand-off flags; exact-fp32 / with bf16 planes
        for flags in (True, False):
            for planes in (False, True):
                tag = '%s%s%s' % (name, '' if flags else '_noflags', '_bf' if planes else '')
                if tr:
                    cs.append((tag, deconv(hip, 32, PH, PW, C0, C1, Nn, act=1, ab=True, flags=flags, planes=planes)))
                elif name == 'd_l4':        # 4x4 stride 1 (24 -> 23)
                    cs.append((tag, conv(hip, 32, PH + 1, PW + 1, C0, C1, 4, 1, 1, Nn, act=2, ab=True, flags=flags, planes=planes)))
                else:
                    cs.append((tag, conv(hip, 32, 2 * PH, 2 * PW, C0, C1, 4, 2, 1, Nn, act=2, ab=True, flags=flags, planes=planes)))
    # one small descriptor per specialised kernel, and beside each one that the same predicate refuses by shape alone
    cs += [('head1_fwd', conv(hip, 2, 8, 8, 512, 0, 4, 1, 1, 1, act=2, ab=True)),
           ('head1_fwd_256ch', conv(hip, 2, 8, 8, 256, 0, 4, 1, 1, 1, act=2, ab=True)),
           ('head1_dgrad', dgrad1(hip, 2, 8, 8, 4, 4, 1, 512, k_real=1)),
           ('head1_dgrad_5x5', dgrad1(hip, 2, 8, 8, 4, 5, 2, 512, k_real=1)),
           ('narrow_conv', conv(hip, 2, 16, 16, 64, 0, 3, 1, 1, 3)),
           ('narrow_conv_5out', conv(hip, 2, 16, 16, 64, 0, 3, 1, 1, 5)),
           ('narrow_transposed', deconv(hip, 2, 16, 16, 64, 0, 3)),
           ('narrow_transposed_48ch', deconv(hip, 2, 16, 16, 48, 0, 3)),
           ('fewchan4', conv(hip, 2, 64, 64, 4, 0, 4, 2, 1, 64, k_real=3)),
           ('fewchan8', conv(hip, 2, 64, 64, 8, 0, 4, 2, 1, 64)),
           ('fewchan8_48wide', conv(hip, 2, 64, 96, 8, 0, 4, 2, 1, 64)),
           ('fewchan7', conv(hip, 2, 64, 64, 4, 0, 7, 2, 2, 64, k_real=3, same=True)),
           ('fewchan7_48wide', conv(hip, 2, 64, 96, 4, 0, 7, 2, 2, 64, k_real=3, same=True)),
           ('pw1x1', conv(hip, 2, 32, 32, 16, 0, 1, 1, 0, 64, act=1, ab=True)),
           ('pw1x1_few_rows', conv(hip, 2, 16, 16, 16, 0, 1, 1, 0, 64, act=1, ab=True)),
           ('c3x3', conv(hip, 4, 64, 64, 32, 0, 3, 1, 1, 32, act=1, ab=True)),
           ('c3x3_dgrad', dgrad1(hip, 4, 64, 64, 32, 3, 1, 32)),
           ('c3x3_n16', conv(hip, 4, 64, 64, 16, 0, 3, 1, 1, 16, act=1, ab=True)),
           ('c3x3_few_rows', conv(hip, 4, 32, 32, 32, 0, 3, 1, 1, 32, act=1, ab=True)),
           ('c3x3_n16_few_rows', conv(hip, 4, 32, 32, 16, 0, 3, 1, 1, 16, act=1, ab=True)),
           ('s2n16', conv(hip, 2, 256, 256, 64, 0, 4, 2, 1, 16)),
           ('s2n16_few_rows', conv(hip, 2, 128, 128, 64, 0, 4, 2, 1, 16)),
           ('tr4n16', deconv(hip, 4, 64, 64, 256, 0, 16, act=1, ab=True)),
           ('tr4n16_few_rows', deconv(hip, 4, 32, 32, 256, 0, 16, act=1, ab=True)),
           ('tr4_tiny', deconv(hip, 2, 32, 32, 4, 0, 3, k_real=3)),
           ('tr4_tiny_8ch', deconv(hip, 2, 32, 32, 8, 0, 3)),
           ('rowtap', conv(hip, 4, 64, 64, 8, 0, 4, 2, 1, 128)),                 # TW * C == 32, too many outputs for conv_fewchan
           ('rowtap_16ch', conv(hip, 4, 64, 64, 16, 0, 4, 2, 1, 128)),
           ('utg_48ch', conv(hip, 4, 32, 32, 48, 0, 3, 1, 1, 64)),               # chunks of 32 + 16: padded <= 1.5 x real
           ('utg_40ch', conv(hip, 4, 32, 32, 40, 0, 3, 1, 1, 64)),               # 1.6 x: the general kernel
           ('bf_partial_36ch', conv(hip, 4, 32, 32, 36, 0, 3, 1, 1, 68, planes=True)),
           ('bf_partial_36ch_two_sources', conv(hip, 4, 32, 32, 32, 36, 3, 1, 1, 68, planes=True))]
    return cs


def wgrad_cases(hip):
    """[(name, descriptor)]: filter gradients."""
    cs = []
    for name, PH, PW, C0, C1, Nn, tr in PIX2PIX:
        for exact in (0, 1):
            tag = '%s_wgrad%s' % (name, '_exact' if exact else '')
            if tr:
                cs.append((tag, deconv_wgrad(hip, 32, PH, PW, C0, C1, Nn, exact)))
            elif name == 'd_l4':
                cs.append((tag, conv_wgrad(hip, 32, PH + 1, PW + 1, C0, C1, 4, 1, 1, Nn, exact, act=2, ab=True)))
            else:
                cs.append((tag, conv_wgrad(hip, 32, 2 * PH, 2 * PW, C0, C1, 4, 2, 1, Nn, exact, act=2, ab=True)))
    h1 = conv_wgrad(hip, 2, 8, 8, 512, 0, 4, 1, 1, 1, act=2, ab=True)
    h1.d = _view(hip, 4, 0, 7, 7)           # the one-channel dy in a 4-float row
    h1_256 = conv_wgrad(hip, 2, 8, 8, 256, 0, 4, 1, 1, 1, act=2, ab=True)
    h1_256.d = _view(hip, 4, 0, 7, 7)
    cs += [('head1_wgrad', h1), ('head1_wgrad_256ch', h1_256),
           ('wgn16_3x3', conv_wgrad(hip, 8, 64, 64, 16, 0, 3, 1, 1, 16, act=1, ab=True)),
           ('wgn16_4x4', wgrad(hip, 8, 64, 64, _view(hip, 64, 0, 64, 64), _view(hip, 16, 0, 64, 64), 4, 1, 1, 64, 16)),
           ('wgn16_3x3_few_rows', conv_wgrad(hip, 4, 64, 64, 16, 0, 3, 1, 1, 16, act=1, ab=True)),
           ('wgrad128_span_580ch', conv_wgrad(hip, 4, 32, 32, 580, 0, 3, 1, 1, 128, Cg_real=579)),     # bf16 form only: tap-spanning tiles
           ('wgrad128_span_580ch_exact', conv_wgrad(hip, 4, 32, 32, 580, 0, 3, 1, 1, 128, exact=1, Cg_real=579)),
           ('wgrad128_96out', conv_wgrad(hip, 4, 32, 32, 128, 0, 3, 1, 1, 96)),                        # < 128 dense channels
           ('wgrad_96ch', conv_wgrad(hip, 4, 32, 32, 96, 0, 3, 1, 1, 96, exact=1)),
           ('wgrad_64x64', conv_wgrad(hip, 4, 32, 32, 64, 0, 1, 1, 0, 64, exact=1)),
           ('wgrad_32out', conv_wgrad(hip, 4, 32, 32, 96, 0, 3, 1, 1, 32, exact=1))]
    return cs


def _name(fn, d):
    buf = C.create_string_buffer(64)
    assert fn(C.byref(d), buf, 64) == 0
    return buf.value.decode()


def _ints(fn, d, n):
    out = (C.c_int * n)(*([-99] * n))
    rc = fn(C.byref(d), WS, out)
    return [rc] + list(out)


def table(hip):
    """{case: what the library would do with it}; pure host queries."""
    l = hip.lib()
    t = {}
    for name, d in conv_cases(hip):
        t[name] = {'kernel': _name(l.ssc_conv_forward_kernel_name, d), 'plan': _ints(l.ssc_conv_forward_plan, d, 5),
                   'bf_plan': _ints(l.ssc_conv_bf_plan, d, 10),
                   'supported': [int(getattr(l, p)(C.byref(d))) for p in CONV_PREDICATES]}
    for name, d in wgrad_cases(hip):
        assert name not in t
        t[name] = {'kernel': _name(l.ssc_conv_wgrad_kernel_name, d), 'plan': _ints(l.ssc_conv_wgrad_plan, d, 4),
                   'plan128': _ints(l.ssc_conv_wgrad128_plan, d, 7),
                   'supported': [int(getattr(l, p)(C.byref(d))) for p in WGRAD_PREDICATES]}
    return t


def gate_probe(hip):
    """The two plans the gate tests look at: a filter gradient on the general kernel whose tile SSC_WG_CFG can move, a forward
    conv of at most one workgroup per CU (32 tiles of 128 x 32, no split-K) whose price SSC_PLAN_OCC1 sets."""
    l = hip.lib()
    return {'wgrad': _ints(l.ssc_conv_wgrad_plan, dict(wgrad_cases(hip))['wgrad_96ch'], 4),
            'fwd': _ints(l.ssc_conv_forward_plan, dict(conv_cases(hip))['c3x3_few_rows'], 5)}


def _main(argv):
    sys.path.insert(0, ROOT)
    from sketchyscenecolorization_amd import hip
    if '--gate' in argv:
        print(json.dumps(gate_probe(hip)))
    elif '--write' in argv:
        with open(GOLDEN, 'w') as fh:
            json.dump(table(hip), fh, indent=0, sort_keys=True, separators=(',', ':'))
            fh.write('\n')
        print('wrote', GOLDEN)
    else:
        print(json.dumps(table(hip)))


# ---- the tests ----
# (name, arguments, environment): every SSC_* variable of the caller is dropped first -- a pinned table needs a pinned environment
_RUNS = [('table', [], {}), ('plain', ['--gate'], {}),
         ('wg_cfg_locked', ['--gate'], {'SSC_WG_CFG': '2'}), ('wg_cfg', ['--gate'], {'SSC_WG_CFG': '2', 'SSC_DEV_SWITCHES': '1'}),
         ('occ1_locked', ['--gate'], {'SSC_PLAN_OCC1': '9'}), ('occ1', ['--gate'], {'SSC_PLAN_OCC1': '9', 'SSC_DEV_SWITCHES': '1'})]


@pytest.fixture(scope='module')
def runs():
    base = {k: v for k, v in os.environ.items() if not k.startswith('SSC_')}
    procs = [(name, subprocess.Popen([sys.executable, os.path.abspath(__file__)] + args, env=dict(base, **env), cwd=ROOT,
                                     stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)) for name, args, env in _RUNS]
    out = {}
    for name, p in procs:
        so, se = p.communicate()
        assert p.returncode == 0, (name, se[-2000:])
        out[name] = json.loads(so.strip().splitlines()[-1])
    return out


def test_dispatch_and_plans_match_the_fixture(runs):
    with open(GOLDEN) as fh:
        want = json.load(fh)
    got = runs['table']
    assert sorted(got) == sorted(want)
    diff = {k: (want[k], got[k]) for k in want if got[k] != want[k]}
    assert not diff, diff


def test_fixture_covers_every_specialised_kernel_and_a_refusal_beside_it():
    with open(GOLDEN) as fh:
        want = json.load(fh)
    names = {v['kernel'] for v in want.values()}
    assert not [n for n in SPECIALISED if n not in names], sorted(names)
    assert want['wgrad128_span_580ch']['plan128'][:3] == [0, 1, 2] and want['wgrad128_span_580ch_exact']['plan128'][0] == -10
    assert want['bf_partial_36ch']['bf_plan'][0] == 0 and want['bf_partial_36ch']['bf_plan'][4] == 2        # source form KM
    assert want['bf_partial_36ch_two_sources']['bf_plan'][0] == -10
    # rowtap: 4 K-tiles (one per filter row); 16 channels: 8 K-tiles of the general kernel -- the modelled cost tells them apart
    assert want['rowtap']['plan'][5] < want['rowtap_16ch']['plan'][5]
    # each predicate accepts its own case and refuses the one beside it (position in CONV_PREDICATES / WGRAD_PREDICATES)
    for yes, no, i in (('head1_fwd', 'head1_fwd_256ch', 0), ('head1_dgrad', 'head1_dgrad_5x5', 1), ('narrow_conv', 'narrow_conv_5out', 2),
                       ('narrow_transposed', 'narrow_transposed_48ch', 2), ('fewchan4', 'fewchan8_48wide', 3),
                       ('fewchan8', 'fewchan8_48wide', 3), ('pw1x1', 'pw1x1_few_rows', 4), ('c3x3', 'c3x3_few_rows', 5),
                       ('c3x3_dgrad', 'c3x3_few_rows', 5), ('c3x3_n16', 'c3x3_n16_few_rows', 5), ('s2n16', 's2n16_few_rows', 6),
                       ('tr4_tiny', 'tr4_tiny_8ch', 7), ('fewchan7', 'fewchan7_48wide', 8), ('tr4n16', 'tr4n16_few_rows', 9),
                       ('head1_wgrad', 'head1_wgrad_256ch', 0), ('enc3_wgrad', 'wgrad128_96out', 1),
                       ('wgn16_3x3', 'wgn16_3x3_few_rows', 2), ('wgn16_4x4', 'wgn16_3x3_few_rows', 2)):
        assert want[yes]['supported'][i] == 1 and want[no]['supported'][i] == 0, (yes, no)


def test_developer_switch_needs_the_gate(runs):
    """SSC_WG_CFG moves the tile of a general filter gradient only under SSC_DEV_SWITCHES=1.  (Configuration 2, 128 x 64, beside
    the planner's 64 x 128: configuration 3, 64 x 64, is allowed only where no other tile is -- <= 64 rows and columns -- so
    pinning it can never change a plan.)"""
    assert runs['plain']['wgrad'][1] == 1       # what the planner takes by itself: 64 x 128
    assert runs['wg_cfg_locked'] == runs['plain']
    assert runs['wg_cfg']['wgrad'][1] == 2 and runs['wg_cfg']['fwd'] == runs['plain']['fwd']


def test_planner_constant_needs_the_gate(runs):
    """SSC_PLAN_OCC1 (the price of one workgroup per CU) is a developer switch like the others: ignored without the gate."""
    assert runs['occ1_locked'] == runs['plain']
    assert runs['occ1']['fwd'] != runs['plain']['fwd']


def _sources():
    pkg = os.path.join(ROOT, 'sketchyscenecolorization_amd')
    for base, exts in ((os.path.join(pkg, 'csrc'), ('.hip', '.h')), (pkg, ('.py',)), (HERE, ('.py', '.sh')),
                       (os.path.join(ROOT, 'scripts'), ('.py', '.sh'))):
        for dirpath, _, files in os.walk(base):
            if base == pkg and dirpath != pkg:
                continue            # the package's own modules; csrc/ is walked above
            for f in sorted(files):
                fp = os.path.join(dirpath, f)
                if f.endswith(exts) and os.path.abspath(fp) != os.path.abspath(__file__):
                    with open(fp, errors='replace') as fh:
                        yield fp, fh.read()


def test_switch_list_and_code_agree():
    with open(os.path.join(ROOT, 'DESIGN.md')) as fh:
        design = fh.read()
    row = [l for l in design[design.index('\n## 7. Switches'):design.index('\n## 8. ')].splitlines() if l.startswith('| `SSC_DEV_SWITCHES=1`')]
    assert len(row) == 1
    listed = set(re.findall(r'SSC_[A-Z0-9_]+', row[0])) - {'SSC_DEV_SWITCHES'}
    read = {}
    pkg = os.path.join(ROOT, 'sketchyscenecolorization_amd')
    for fp, text in _sources():
        if fp.startswith(pkg):
            for m in re.finditer(r'(?:ssc_dev_getenv|ssc_dev_int|ssc_dev_double|_dev_env)\(\s*["\'](SSC_[A-Z0-9_]+)["\']', text):
                read.setdefault(m.group(1), fp)
    assert len(read) >= 20, sorted(read)
    assert listed == set(read), (sorted(listed - set(read)), sorted(set(read) - listed))      # the row lists exactly what the code reads
    left = [(n, fp) for fp, text in _sources() for n in RETIRED if re.search(r'\b%s\b' % n, text)]
    assert not left, left


if __name__ == '__main__':
    _main(sys.argv[1:])
