"""Which way a conv with a reduction on its epilogue goes (ssc_conv_forward_bn, _bnbwd, _bnbwd2, _minmax), pinned: the host-only
query ssc_conv_rider_plan over a fixed list of descriptors, workspaces and partial-row capacities, compared with
tests/golden/rider_table.json.  No GPU: the query launches nothing and the descriptors are the dummy-pointer ones of
test_dispatch_table.py.

The fixture is a record of the four entry points as they were BEFORE the query existed, made without a device by running them
dry (profiles/conv_route_once.txt says how and carries the patch); it cannot be regenerated from this tree, only extended by
the same procedure.  `python tests/test_rider_table.py` prints what this tree's query says of every case, as JSON.

The kernel table of DESIGN.md section 3 is held to the code as well: a kernel's predicate refuses a rider's fields exactly
where the table says it neither carries nor overlooks that rider, and the query streams exactly where it says "carries"."""
import ctypes as C
import json
import os
import re
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
from test_dispatch_table import CONV_PREDICATES, _p, conv, conv_cases, deconv, dgrad1  # noqa: E402,F401

GOLDEN = os.path.join(HERE, 'golden', 'rider_table.json')
RIDERS = ['bn', 'bnbwd', 'bnbwd2', 'minmax']                       # SSC_RIDER_*
PATHS = ['plain', 'stream', 'tile', 'slab']                        # SSC_RIDER_PATH_*
KERNELS = ['tiled', 'head1_fwd', 'head1_dgrad', 'narrow', 'fewchan', 'pw1x1', 'c3x3', 's2n16', 'tr4_tiny', 'fewchan7', 'tr4n16']
HOMES = ['none', 'ws_head', 'ws_tail', 'caller']                   # SSC_RIDER_ROWS_*
WORKSPACES = [('nows', 0), ('1M', 1 << 20), ('256M', 256 << 20)]
AMPLE = 1 << 30
# the case of conv_cases() that each early kernel accepts
ACCEPTING = {'head1_fwd': 'head1_fwd', 'head1_dgrad': 'head1_dgrad', 'narrow': 'narrow_conv', 'fewchan': 'fewchan8', 'pw1x1': 'pw1x1',
             'c3x3': 'c3x3', 's2n16': 's2n16', 'tr4_tiny': 'tr4_tiny', 'fewchan7': 'fewchan7', 'tr4n16': 'tr4n16'}


def site(hip, i, ldx, cap, x_off=0):
    s = hip.BnBwdSite()
    s.x, s.ab, s.stats, s.partial = _p(11 + 4 * i) + x_off, _p(12 + 4 * i), _p(13 + 4 * i), _p(14 + 4 * i)
    s.partial_bytes, s.ldx, s.act = cap, ldx, 1
    return s


def sites_for(hip, d, rider, C0=None, cap=(AMPLE, AMPLE), ldx=None):
    """(site0, site1, C0) as the rider's entry point takes them."""
    if rider == 'bnbwd':
        return site(hip, 0, d.ldc if ldx is None else ldx, cap[0]), None, 0
    if rider == 'bnbwd2':
        return site(hip, 0, C0 if ldx is None else ldx, cap[0]), site(hip, 1, d.Nstore - C0, cap[1]), C0
    return None, None, 0


def rider_descs(hip):
    """[(name, descriptor, riders, site keywords)]: the cases made for the riders; each accepting one has refusals beside it that
    differ in one field."""
    def base(h=96, **kw):        # 3x3 SAME conv 64 -> 256 over 2 samples: uniform taps, whole 16-byte rows, no early kernel
        return conv(hip, 2, h, h, 64, 0, 3, 1, 1, 256, **kw)

    def edit(d, **kw):
        for k, v in kw.items():
            setattr(d, k, v)
        return d

    cs = [('base', base(), RIDERS, {}),
          ('out_off_4_bytes', edit(base(), out=_p(6) + 4), RIDERS, {}),
          ('ldc_wider', edit(base(), ldc=260), RIDERS, {}),
          ('accumulate', edit(base(), accumulate=1), RIDERS, {}),
          ('bias', edit(base(), bias=_p(19)), RIDERS, {}),
          ('epi2', edit(base(), epi=2, bias=_p(19)), RIDERS, {}),
          ('sample_12x12', base(12), RIDERS, {}),                     # a sample is not whole row tiles
          ('c0_64', base(), ['bnbwd2'], {'C0': 64}),
          ('site_ldx_odd', base(), ['bnbwd', 'bnbwd2'], {'ldx': 258}),
          ('site_x_off_4_bytes', base(), ['bnbwd'], {'x_off': 4}),
          ('enc5_like', conv(hip, 2, 12, 12, 512, 0, 4, 2, 1, 512), RIDERS, {}),       # few rows, long K: split-K
          ('rowtap_128', conv(hip, 4, 64, 64, 8, 0, 4, 2, 1, 128), RIDERS, {}),        # the row-tap form: bn and bnbwd only
          ('pw1x1_256', conv(hip, 2, 32, 32, 64, 0, 1, 1, 0, 256, act=1, ab=True), RIDERS, {}),
          ('c3x3_ldc_wider', edit(conv(hip, 4, 64, 64, 32, 0, 3, 1, 1, 32, act=1, ab=True), ldc=36), RIDERS, {})]
    # every early kernel under bnbwd2 as well (conv_cases() x bnbwd2 keeps to Nstore > 128)
    table = dict(conv_cases(hip))
    cs += [('%s_two_sites' % k, table[name], ['bnbwd2'], {'C0': max(4, table[name].Nstore // 8 * 4)}) for k, name in ACCEPTING.items()]
    return cs


def cases(hip, rows_of):
    """[(case name, descriptor, rider, workspace bytes, site0, site1, C0)].  rows_of(case name) -> the rows that case
    reported: the "short" cases give the caller's buffer one row less than the ample run asked for."""
    out = []

    def add(name, d, rider, kw, workspaces):
        C0 = kw.get('C0', 128)
        for wn, wb in workspaces:
            full = '%s|%s|%s' % (name, rider, wn)
            s = sites_for(hip, d, rider, C0, ldx=kw.get('ldx'))
            if kw.get('x_off'):
                s[0].x += kw['x_off']
            out.append((full,) + (d, rider, wb) + s)
            if rider in ('bnbwd', 'bnbwd2') and rows_of(full) > 0:
                short = (rows_of(full) - 1) * 2 * (d.Nstore if rider == 'bnbwd' else C0) * 4
                out.append((full + '|short',) + (d, rider, wb) + sites_for(hip, d, rider, C0, cap=(short, AMPLE), ldx=kw.get('ldx')))

    for name, d in conv_cases(hip):
        for rider in RIDERS:
            if rider != 'bnbwd2' or d.Nstore > 128:
                add(name, d, rider, {}, WORKSPACES)
    for name, d, riders, kw in rider_descs(hip):
        for rider in riders:
            add('r_' + name, d, rider, kw, WORKSPACES + ([('64K', 64 << 10)] if name == 'enc5_like' else []))
    return out


def query(hip, d, rider, ws_bytes, s0, s1, C0):
    out = (C.c_int64 * 5)(*([-99] * 5))
    rc = hip.lib().ssc_conv_rider_plan(C.byref(d), RIDERS.index(rider), ws_bytes, C.byref(s0) if s0 is not None else None,
                                       C.byref(s1) if s1 is not None else None, C0, out)
    assert rc == 0, rc
    return list(out)


def table(hip, rows_of=None):
    got = {}
    for c in cases(hip, rows_of or (lambda name: got[name][2])):
        assert c[0] not in got, c[0]
        got[c[0]] = query(hip, *c[1:])
    return got


def _hip():
    sys.path.insert(0, ROOT)
    from sketchyscenecolorization_amd import hip
    return hip


def _golden():
    with open(GOLDEN) as fh:
        return json.load(fh)


# ---- the tests ----
def test_riders_decide_as_the_recorded_entry_points_did():
    want = _golden()
    got = table(_hip(), lambda name: want[name][2])
    assert sorted(got) == sorted(want)
    diff = {k: (want[k], got[k]) for k in want if got[k] != want[k]}
    assert not diff, diff


def test_fixture_shows_every_path_and_every_kernel_under_every_rider():
    want = _golden()
    seen = {(k.split('|')[1], PATHS[v[0]]) for k, v in want.items()}
    paths = {'bn': ['plain', 'stream', 'tile', 'slab'], 'bnbwd': ['plain', 'stream', 'tile'], 'bnbwd2': ['plain', 'tile'],
             'minmax': ['plain', 'tile']}
    assert seen == {(r, p) for r in RIDERS for p in paths[r]}, sorted(seen)
    under = {(k.split('|')[1], KERNELS[v[1]]) for k, v in want.items()}
    assert not [(r, k) for r in RIDERS for k in KERNELS if (r, k) not in under], sorted(under)
    # the rows' homes: the workspace's start for a streaming kernel's statistics, its tail for the tiles', the caller's otherwise
    homes = {(k.split('|')[1], PATHS[v[0]]): HOMES[v[3]] for k, v in want.items()}
    assert homes == {('bn', 'plain'): 'none', ('bn', 'stream'): 'ws_head', ('bn', 'tile'): 'ws_tail', ('bn', 'slab'): 'ws_tail',
                     ('bnbwd', 'plain'): 'none', ('bnbwd', 'stream'): 'caller', ('bnbwd', 'tile'): 'caller',
                     ('bnbwd2', 'plain'): 'none', ('bnbwd2', 'tile'): 'caller', ('minmax', 'plain'): 'none',
                     ('minmax', 'tile'): 'ws_tail'}, homes

    def path(name):
        return PATHS[want[name][0]]

    # each accepting case and the refusal beside it that differs in one field
    for r in RIDERS:
        assert path('r_base|%s|256M' % r) == 'tile', r
        for no in ('out_off_4_bytes', 'ldc_wider', 'accumulate'):
            assert path('r_%s|%s|256M' % (no, r)) == 'plain', (no, r)
        assert path('r_base|%s|nows' % r) == 'plain', r
    assert path('r_bias|bnbwd|256M') == 'plain' and path('r_bias|bnbwd2|256M') == 'plain'
    assert path('r_bias|bn|256M') == 'tile' and path('r_bias|minmax|256M') == 'tile'
    assert path('r_epi2|minmax|256M') == 'tile' and path('r_epi2|bn|256M') == 'plain'
    assert path('r_sample_12x12|minmax|256M') == 'plain'
    assert path('r_c0_64|bnbwd2|256M') == 'plain'
    assert path('r_site_ldx_odd|bnbwd|256M') == 'plain' and path('r_site_ldx_odd|bnbwd2|256M') == 'plain'
    assert path('r_site_x_off_4_bytes|bnbwd|256M') == 'plain'
    assert path('r_base|bnbwd|256M|short') == 'plain' and path('r_base|bnbwd2|256M|short') == 'plain'
    assert path('r_enc5_like|bn|256M') == 'slab' and path('r_enc5_like|bn|64K') != 'slab'
    assert path('r_rowtap_128|bn|256M') == 'tile' and path('r_rowtap_128|bnbwd|256M') == 'tile'
    assert path('r_rowtap_128|minmax|256M') == 'plain'
    assert path('c3x3|bnbwd|256M') == 'stream' and path('c3x3|bnbwd|256M|short') == 'plain'
    assert path('r_c3x3_ldc_wider|bn|256M') == 'plain'


def _design_table():
    """{kernel: (carries, overlooks)} from the table of DESIGN.md section 3 (columns: order, kernel, takes, carries, overlooks)."""
    with open(os.path.join(ROOT, 'DESIGN.md')) as fh:
        design = fh.read()
    sec = design[design.index('\n## 3. '):design.index('\n## 4. ')]
    rows = {}
    for line in sec.splitlines():
        m = re.match(r'\| (\d+) \| `(\w+)` \|[^|]*\|([^|]*)\|([^|]*)\|$', line)
        if m:
            assert int(m.group(1)) == len(rows) + 1, line           # in dispatch order
            rows[m.group(2)] = tuple({r for r in RIDERS if re.search(r'`%s`' % r, m.group(g))} for g in (3, 4))
    return rows


def test_kernel_table_predicates_and_query_agree():
    hip = _hip()
    l = hip.lib()
    doc = _design_table()
    assert list(doc) == KERNELS[1:], list(doc)
    table_ = dict(conv_cases(hip))
    fields = {'bn': ['stat_partial'], 'bnbwd': ['stat_partial', 'sb_x'], 'bnbwd2': ['stat_partial', 'sb_x', 'sb2_x'],
              'minmax': ['stat_partial', 'stat_mode']}
    for i, k in enumerate(KERNELS[1:]):
        pred = getattr(l, CONV_PREDICATES[i])
        carries, overlooks = doc[k]
        assert not (carries & overlooks), k
        for r in RIDERS:
            d = table_[ACCEPTING[k]]
            assert pred(C.byref(d)) == 1, k
            for f in fields[r]:
                setattr(d, f, 1 if f == 'stat_mode' else _p(20))
            refused = pred(C.byref(d)) == 0
            for f in fields[r]:
                setattr(d, f, 0 if f == 'stat_mode' else None)
            assert refused == (r not in carries | overlooks), (k, r, refused)
            # ample workspace and rows: the kernel itself takes the rider exactly where the table says it carries it
            C0 = 128 if d.Nstore > 128 else max(4, d.Nstore // 8 * 4)
            got = query(hip, d, r, 256 << 20, *sites_for(hip, d, r, C0))
            assert (PATHS[got[0]] == 'stream') == (r in carries), (k, r, got)
            if r in carries or r in overlooks:
                assert KERNELS[got[1]] == k, (k, r, got)


if __name__ == '__main__':
    print(json.dumps(table(_hip()), sort_keys=True))
