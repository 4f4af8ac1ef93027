"""The float64 reference of the filter-gradient tests (tests/wgrad_oracle.py) against itself, and the comparison rule
(kernel_check.check_dot) against results that miss one term.  No GPU."""
import pytest
import torch

import wgrad_oracle as O
from kernel_check import check_dot


def _agree(c):
    inp = O.make_inputs(c)
    a = O.ref_autograd(c, inp)
    b, S = O.ref_taps(c, inp)
    assert a.shape == b.shape == S.shape and a.dtype == b.dtype == torch.float64
    scale = float(b.abs().max())
    assert scale > 0 and bool((S >= b.abs() * (1 - 1e-12)).all())
    assert float((a - b).abs().max()) <= 1e-12 * scale, (float((a - b).abs().max()), scale)


@pytest.mark.parametrize('name', [c['name'] for c in O.CASES])
def test_autograd_reference_equals_tap_loop_reference(name):
    """(a) autograd through oracle/tf_ops.py == (b) shifted slices + einsum, to 1e-12 of the largest value."""
    _agree(O.BY_NAME[name])


@pytest.mark.parametrize('name', [c['name'] for c in O.CASES128])
def test_autograd_reference_equals_tap_loop_reference_128(name):
    """The same on the table of the 128 x 128 kernels, its 65 536-pixel case included."""
    _agree(O.BY_NAME128[name])


@pytest.mark.parametrize('name,gt,dt', O.CARRIER_FORMS, ids=['%s-g%s-d%s' % f for f in O.CARRIER_FORMS])
def test_autograd_reference_equals_tap_loop_reference_carriers(name, gt, dt):
    """... and on the carrier cases with either side plain or transformed."""
    _agree(O.carrier(name, gt, dt))


def test_tables_do_not_share_inputs():
    """CASES seeds from its index (1000 + i), CASES128 and the carrier forms from bases of their own."""
    seeds = [1000 + i for i in range(len(O.CASES))] + [c['seed'] for c in O.CASES128] + \
            [O.carrier(*f)['seed'] for f in O.CARRIER_FORMS]
    assert len(set(seeds)) == len(seeds)
    assert all('seed' not in c for c in O.CASES)


def test_padding_lanes_hold_1e3_and_do_not_reach_the_reference():
    c = O.BY_NAME['t4_nn3_dy4_deconv']
    inp = O.make_inputs(c)
    assert float(inp['g0'][..., 3].min()) == O.PAD_LANE and float(inp['d0'][..., 3].min()) == O.PAD_LANE
    assert float(O.ref_taps(c, inp)[1].max()) < 1e3


def _border_tap(c):
    """A pixel and a tap that lies inside the gathered image while another tap of the same pixel lies outside."""
    geo = O.geometry(c)
    for py in (0, geo['PH'] - 1):       # SAME over an even size pads after only: the border is the bottom row
        pixel = (geo['NB'] - 1, py, geo['PW'] // 2)
        inside = [(ty, tx) for ty in range(geo['TH']) for tx in range(geo['TW'])
                  if 0 <= py * geo['stride'] + geo['oy'] + ty < geo['GH']]
        if 0 < len(inside) < geo['TH'] * geo['TW']:
            break
    else:
        raise AssertionError('no pixel at a border')
    return pixel, inside[0]


@pytest.mark.parametrize('name', ['t4_first_layer_4x4s2', 't2_3x3same_s2_even', 't0_3x3_two_gathered'])
def test_rule_rejects_a_result_that_misses_one_term(name):
    """check_dot accepts what a CPU computes in float32 and rejects the float64 reference with the last pixel removed, with one
    border tap of one pixel removed, and with one padding-lane value (1.0e3) taken into channel 0."""
    c = O.BY_NAME[name]
    inp = O.make_inputs(c)
    geo = O.geometry(c)
    K = O.pixels(c)
    ref, S = O.ref_taps(c, inp)
    cfg = dict(case=name)
    check_dot('wgrad_rule', cfg, O.ref_taps(c, inp, torch.float32)[0], ref, S, K, what='float32 CPU')
    last = (geo['NB'] - 1, geo['PH'] - 1, geo['PW'] - 1)
    no_last = ref.clone()
    for ty in range(geo['TH']):
        for tx in range(geo['TW']):
            no_last[ty, tx] -= O.term(c, inp, last, (ty, tx))
    pixel, tap = _border_tap(c)
    no_tap = ref.clone()
    no_tap[tap] -= O.term(c, inp, pixel, tap)
    assert float((no_tap - ref).abs().max()) > 0
    leaked = ref.clone()
    D = O.transformed(c, inp, 'd')[..., :c['d'][2]]
    leaked[tap[0], tap[1], 0] += O.PAD_LANE * D[pixel]
    for what, damaged in (('last pixel removed', no_last), ('border tap removed', no_tap), ('padding lane leaked', leaked)):
        with pytest.raises(AssertionError):
            check_dot('wgrad_rule', cfg, damaged.float(), ref, S, K, what=what)
