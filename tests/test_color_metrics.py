"""The colour scores without a GPU: the oracle's anchors, the condition that makes the histograms exact
-- no byte colour near a cell boundary --, the host formulas of metrics.py from hand-made rows, and the command lines' flag."""
import json
import math

import numpy as np
import pytest

import color_metrics_oracle as CO
from sketchyscenecolorization_amd import metrics as M


@pytest.fixture(scope='module')
def all_ab():
    """a* and b* of all 2^24 byte colours, float64 [2^24] each (index r << 16 | g << 8 | b), computed once and read only."""
    lin = CO.linear(np.arange(256))
    a, b = np.empty(1 << 24, np.float64), np.empty(1 << 24, np.float64)
    g_, b_ = np.meshgrid(lin, lin, indexing='ij')
    g_, b_ = g_.ravel(), b_.ravel()
    for r in range(256):        # 65536 colours at a time
        xyz = [(CO.M[k, 0] * lin[r] + CO.M[k, 1] * g_ + CO.M[k, 2] * b_) / CO.WHITE[k] for k in range(3)]
        fx, fy, fz = CO.f(xyz[0]), CO.f(xyz[1]), CO.f(xyz[2])
        a[r << 16:(r + 1) << 16] = 500.0 * (fx - fy)
        b[r << 16:(r + 1) << 16] = 200.0 * (fy - fz)
    a.setflags(write=False)
    b.setflags(write=False)
    return a, b


# ------------------------------------------------------------------ the oracle
def test_oracle_anchors(all_ab):
    a, b = all_ab
    for got, want in ((a.min(), -86.18303), (a.max(), 98.23305), (b.min(), -107.85730), (b.max(), 94.47812)):
        assert abs(got - want) <= 1e-4, (got, want)
    grey = np.arange(256) * 0x010101
    for got, want in ((np.abs(a[grey]).max(), 0.00245), (np.abs(b[grey]).max(), 0.00465)):      # (quoted to five decimals)
        assert abs(got - want) <= 1e-4, (got, want)
    assert np.array_equal(CO.lab(np.zeros(3, np.uint8)), np.zeros(3))
    assert abs(CO.lab(np.full(3, 255, np.uint8))[0] - 100.0) <= 1e-9
    t = CO.DELTA ** 3
    assert abs(float(CO.f(np.nextafter(t, 1.0))) - float(CO.f(t))) <= 1e-12
    assert abs(float(CO.f(t)) - CO.DELTA) <= 1e-12      # both branches meet at 6/29
    # the sweep's own arithmetic is the oracle's
    rng = np.random.RandomState(3)
    px = rng.randint(0, 256, (500, 3)).astype(np.uint8)
    idx = (px[:, 0].astype(np.int64) << 16) | (px[:, 1].astype(np.int64) << 8) | px[:, 2]
    lab = CO.lab(px)
    assert np.abs(lab[:, 1] - a[idx]).max() <= 1e-12 and np.abs(lab[:, 2] - b[idx]).max() <= 1e-12
    assert np.array_equal(M.lab_lin_table(), CO.linear(np.arange(256)))


def test_no_byte_colour_lies_near_a_cell_boundary(all_ab):
    """What makes the device's histograms the oracle's: over all 2^24 colours the least distance of a* or b* to a boundary
    (4.2e-8) is far above any float64 rounding difference, the clamp never acts, and the greys sit in the centre cell."""
    a, b = all_ab
    least = min(float(CO.boundary_distance(a).min()), float(CO.boundary_distance(b).min()))
    print('least distance to a cell boundary: %.3e' % least)
    assert least >= 1e-9
    for v in (a, b):
        c = CO.cell_unclamped(v)
        assert c.min() >= 0 and c.max() <= CO.BINS - 1, (c.min(), c.max())
    grey = np.arange(256) * 0x010101
    assert (CO.cell(a[grey]) == 11).all() and (CO.cell(b[grey]) == 11).all()


# ------------------------------------------------------------------ the host formulas
def _row(pa, pb, hist_common=None):
    """The [13] row of two lists of byte colours with as many pixels, dE sums set to 0."""
    pa, pb = np.asarray(pa, np.uint8).reshape(-1, 3), np.asarray(pb, np.uint8).reshape(-1, 3)
    r = [0.0, 0.0, 0.0, float(len(pa))] + CO.opponent_sums(pa) + CO.opponent_sums(pb)
    if hist_common is None:
        hist_common = np.minimum(CO.histogram(CO.lab(pa)), CO.histogram(CO.lab(pb))).sum()
    return r + [float(hist_common)]


def test_colourfulness_of_hand_made_images():
    c = (200, 40, 90)
    rg, yb = c[0] - c[1], (c[0] + c[1]) / 2.0 - c[2]
    s = M.color_scores([_row([c] * 7, [c] * 7)])[0]
    want = 0.3 * math.sqrt(rg * rg + yb * yb)
    assert abs(s['colourfulness'] - want) <= 1e-12 * want and s['colourfulness_target'] == s['colourfulness']
    # p pixels of colour 1 and q of colour 2: var = p q (x1 - x2)^2 / (p + q)^2, mean = (p x1 + q x2) / (p + q)
    c1, c2, p, q = (250, 10, 30), (20, 180, 240), 3, 5
    op = lambda c: (c[0] - c[1], (c[0] + c[1]) / 2.0 - c[2])      # noqa: E731
    (rg1, yb1), (rg2, yb2), n = op(c1), op(c2), p + q
    var = p * q * ((rg1 - rg2) ** 2 + (yb1 - yb2) ** 2) / float(n * n)
    mean2 = ((p * rg1 + q * rg2) / n) ** 2 + ((p * yb1 + q * yb2) / n) ** 2
    want = math.sqrt(var) + 0.3 * math.sqrt(mean2)
    s = M.color_scores([_row([c1] * p + [c2] * q, [c] * n)])[0]
    assert abs(s['colourfulness'] - want) <= 1e-12 * want
    assert abs(s['colourfulness'] - CO.colourfulness(np.array([c1] * p + [c2] * q, np.uint8))) <= 1e-12 * want
    assert abs(s['colourfulness_target'] - 0.3 * math.sqrt(rg * rg + yb * yb)) <= 1e-10


def test_scores_of_hand_made_rows():
    px = [(255, 0, 0), (0, 255, 0), (12, 200, 90), (12, 200, 90)]
    s = M.color_scores([_row(px, px)])[0]
    assert s['hist_intersection'] == 1.0 and s['de76'] == 0.0 and s['dab'] == 0.0 and s['dl'] == 0.0
    s = M.color_scores([_row([(255, 0, 0)] * 4, [(0, 0, 255)] * 4)])[0]      # red and blue share no cell
    assert s['hist_intersection'] == 0.0
    row = _row(px, px)
    row[0:3] = [8.0, 6.0, 2.0]
    s = M.color_scores([row])[0]
    assert (s['de76'], s['dab'], s['dl']) == (2.0, 1.5, 0.5)
    nothing = M.color_scores([[0.0] * 13])[0]
    assert set(nothing) == set(M.COLOR_KEYS) and all(v is None for v in nothing.values())


def test_summary_does_not_depend_on_the_order_of_the_images():
    rng = np.random.RandomState(5)
    rows = []
    for _ in range(6):
        pa, pb = rng.randint(0, 256, (9, 3)), rng.randint(0, 256, (9, 3))
        r = _row(pa, pb)
        r[0:3] = sorted(rng.rand(3) * 300, reverse=True)
        rows.append(r)
    rows[4] = [0.0] * 13
    names = ['car_b', 'car_a', 'tree_x', 'bus_9', 'bus_1', 'tree_c']
    groups = [n.split('_')[0] for n in names]
    text = M.dumps(M.summarise_color(names, groups, np.array(rows)))
    for perm in ([5, 4, 3, 2, 1, 0], [2, 0, 4, 1, 5, 3]):
        again = M.dumps(M.summarise_color([names[i] for i in perm], [groups[i] for i in perm], np.array([rows[i] for i in perm])))
        assert again == text
    s = json.loads(text)
    assert sorted(s) == ['all', 'groups', 'images'] and sorted(s['groups']) == ['bus', 'car', 'tree']
    assert s['all']['n'] == 6 and s['groups']['bus']['n'] == 2
    assert s['images']['bus_1'] == dict.fromkeys(M.COLOR_KEYS)       # nothing counted: no value, and it enters no mean
    assert s['groups']['bus']['de76'] == s['images']['bus_9']['de76']
    assert sorted(s['images']['car_a']) == sorted(M.COLOR_KEYS)
    assert M.color_line(s).startswith('colour: n 6  dE76 ')
    assert 'n/a' in M.color_line(M.summarise_color(['a'], ['g'], np.zeros((1, 13))))


# ------------------------------------------------------------------ the flag
def test_flag_rule():
    assert M.checked_color_flag(0, 0, 0, 'scene') == 0 and M.checked_color_flag(1, 1, 0, 'test') == 1
    assert M.checked_color_flag(1, 0, 5, 'train') == 1
    with pytest.raises(ValueError, match=r'--color_metrics 1 .* --mode test needs --metrics 1'):
        M.checked_color_flag(1, 0, 0, 'test')
    with pytest.raises(ValueError, match=r'--color_metrics 1 .* --mode train needs --val_freq F > 0'):
        M.checked_color_flag(1, 0, 0, 'train')
    with pytest.raises(ValueError, match=r'--color_metrics 1 .*--metrics 1.* this is --mode scene'):
        M.checked_color_flag(1, 1, 5, 'scene')


def test_foreground_command_line(monkeypatch):
    import obj_colorization_main as cli
    from sketchyscenecolorization_amd.obj_lib import main_procedure as mp
    assert cli.build_parser().parse_args([]).color_metrics == 0
    assert cli.build_parser().parse_args(['-cm', '1']).color_metrics == 1
    assert {name: key for name, _s, _t, _d, _c, key, _h in cli.FLAGS}['color_metrics'] == 'color_metrics'
    reached = []
    monkeypatch.setattr(mp, 'train', lambda **kw: reached.append('train'))
    monkeypatch.setattr(mp, 'validation', lambda **kw: reached.append(('val', kw['color_metrics'])))
    monkeypatch.setattr(mp, 'inference', lambda *a: reached.append('inference'))
    monkeypatch.setattr(mp, 'scene', lambda *a, **kw: reached.append('scene'))
    monkeypatch.setattr(cli, 'start_or_resume_training', lambda params: reached.append(('start', params['color_metrics'])) or (0, 's'))
    stamp = '2024-01-02-03-04-05'
    for argv, match in ((['-cm', '1'], r'--color_metrics 1 .* needs --val_freq \(-vf\) F > 0'),
                        (['-cm', '1', '--mode', 'val', '-rf', stamp], r'--color_metrics 1 .* --mode val needs --metrics \(-mt\) 1'),
                        (['-cm', '1', '--mode', 'test', '-rf', stamp], r'--color_metrics 1 .* --mode test needs --metrics \(-mt\) 1'),
                        (['-cm', '1', '-mt', '1', '--mode', 'inference', '-rf', stamp, '-in', 'car.png', '-ins', 'the car is red'],
                         r'--color_metrics 1 .*--metrics \(-mt\) 1.* this is --mode inference'),
                        (['-cm', '1', '-vf', '2', '--mode', 'scene', '-rf', stamp], r'--color_metrics 1 .* this is --mode scene')):
        with pytest.raises(ValueError, match=match):
            cli.main(argv)
    assert not reached
    cli.main(['-cm', '1', '-vf', '3'])
    cli.main(['-cm', '1', '-mt', '1', '--mode', 'val', '-rf', stamp])
    assert reached == [('start', 1), ('val', 1)]


def test_background_command_line(monkeypatch):
    import bg_colorization_main as bgcli
    assert bgcli.build_parser().parse_args([]).color_metrics == 0
    built = []
    monkeypatch.setattr(bgcli, 'bg_colorization', lambda **p: built.append(p))
    monkeypatch.setattr(bgcli, 'new_trainer', lambda p: built.append('trainer'))
    for argv, match in ((['--mode', 'train', '--color_metrics', '1'], r'--color_metrics 1 .* needs --val_freq F > 0'),
                        (['--mode', 'test', '--resume_from', 's', '--color_metrics', '1'],
                         r'--color_metrics 1 .* --mode test needs --metrics 1'),
                        (['--mode', 'scene', '--resume_from', 's', '--image_id', '1', '--instruction', 'the sky is pink',
                          '--color_metrics', '1'], r'--color_metrics 1 .* this is --mode scene')):
        with pytest.raises(ValueError, match=match):
            bgcli.main(argv)
    assert not built
    bgcli.main(['--mode', 'train', '--color_metrics', '1', '--val_freq', '3'])
    bgcli.main(['--mode', 'test', '--resume_from', 's', '--color_metrics', '1', '--metrics', '1'])
    assert [b['color_metrics'] for b in built] == [1, 1] and built[1]['metrics'] == 1


def test_flag_off_leaves_the_validation_lines_as_they_are():
    from sketchyscenecolorization_amd import bg_validation, train_validation
    rows = np.array([[30.0, 400.0, 16.0, 2.5, 1.0], [0.0, 0.0, 16.0, 3.0, 1.0]])
    color = np.array([_row([(1, 2, 3)] * 16, [(9, 2, 3)] * 16), _row([(200, 2, 3)] * 16, [(200, 2, 3)] * 16)])
    names, groups = ['car_a', 'bus_b'], ['car', 'bus']
    line, _ = train_validation.validation_line(7, names, groups, rows, 0.5)
    assert sorted(line) == ['all', 'groups', 'images', 'seconds', 'step']
    with_color, _ = train_validation.validation_line(7, names, groups, rows, 0.5, color_rows=color)
    assert sorted(with_color) == ['all', 'color', 'groups', 'images', 'seconds', 'step']
    assert {k: v for k, v in with_color.items() if k != 'color'} == line
    assert sorted(with_color['color']) == ['all', 'groups'] and sorted(with_color['color']['groups']) == ['bus', 'car']
    assert with_color['color']['groups']['bus']['hist_intersection'] == 1.0
    conf = np.array([[5, 1, 2, 6, 0], [4, 0, 0, 8, 2]], np.int64)
    line, _ = bg_validation.validation_line(7, names, rows, conf, 0.5)
    assert sorted(line) == ['all', 'groups', 'images', 'region', 'seconds', 'step']
    with_color, _ = bg_validation.validation_line(7, names, rows, conf, 0.5, color)
    assert {k: v for k, v in with_color.items() if k != 'color'} == line and sorted(with_color['color']) == ['all', 'groups']
