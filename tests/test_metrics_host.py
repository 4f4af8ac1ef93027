"""--metrics, the host side (no GPU): the SSIM window, the step from the kernel's five sums per image to MAE / PSNR / SSIM and
to metrics.json, the flag of both command lines, and the float64 oracle of the kernel tests checked against itself."""
import json
import math

import numpy as np
import pytest

import metrics_oracle as MO


class _Reached(Exception):
    pass


def test_ssim_window():
    from sketchyscenecolorization_amd import metrics as M
    w = M.ssim_window()
    assert w.dtype == np.float64 and w.shape == (11,)
    assert abs(w.sum() - 1.0) <= 1e-15
    assert np.array_equal(w, w[::-1]) and w.argmax() == 5 and (w > 0).all()
    i = np.arange(11) - 5.0
    assert np.allclose(w / w[5], np.exp(-i * i / 4.5), rtol=1e-15, atol=0)


def test_scores():
    from sketchyscenecolorization_amd import metrics as M
    rows = np.array([[0, 0, 100, 90.0 * 3, 90],          # identical images
                     [600, 2400, 100, 0, 0],             # 0 windows
                     [300, 1200, 50, 45.0 * 3 * 0.5, 45]], np.float64)
    s = M.scores(rows)
    assert s[0]['mae'] == 0.0 and s[0]['mse'] == 0.0 and s[0]['psnr'] is None and s[0]['ssim'] == 1.0
    assert s[1]['mae'] == 2.0 and s[1]['mse'] == 8.0 and s[1]['ssim'] is None
    assert s[1]['psnr'] == 10.0 * math.log10(255.0 ** 2 / 8.0)
    assert s[2] == {'mae': 2.0, 'mse': 8.0, 'psnr': s[1]['psnr'], 'ssim': 0.5}
    assert json.loads(json.dumps(s[0]))['psnr'] is None         # JSON null


def test_summarise():
    from sketchyscenecolorization_amd import metrics as M
    rows = np.array([[300, 1200, 100, 150.0, 100],      # mae 1, mse 4, ssim 0.5
                     [0, 0, 100, 300.0, 100],           # identical: psnr infinite, ssim 1
                     [900, 4800, 100, 0, 0],            # mae 3, mse 16, no window
                     [600, 2400, 100, 75.0, 100]], np.float64)      # mae 2, mse 8, ssim 0.25
    names, groups = ['car_b', 'car_a', 'bus_x', 'tree_y'], ['car', 'car', 'bus', 'tree']
    s = M.summarise(names, groups, rows)
    p = lambda mse: 10.0 * math.log10(255.0 ** 2 / mse)        # noqa: E731
    assert list(s) == sorted(s) == ['all', 'groups', 'images']
    assert list(s['images']) == ['bus_x', 'car_a', 'car_b', 'tree_y'] and list(s['groups']) == ['bus', 'car', 'tree']
    assert s['images']['car_b'] == {'mae': 1.0, 'psnr': p(4.0), 'ssim': 0.5}
    assert s['images']['car_a'] == {'mae': 0.0, 'psnr': None, 'ssim': 1.0}
    assert s['images']['bus_x'] == {'mae': 3.0, 'psnr': p(16.0), 'ssim': None}
    # a group's psnr is the mean of the finite ones, its ssim the mean of the images that have one
    assert s['groups']['car'] == {'n': 2, 'mae': 0.5, 'psnr': p(4.0), 'psnr_infinite': 1, 'ssim': 0.75}
    assert s['groups']['bus'] == {'n': 1, 'mae': 3.0, 'psnr': p(16.0), 'psnr_infinite': 0, 'ssim': None}
    a = s['all']
    assert a['n'] == 4 and a['mae'] == 1.5 and a['psnr_infinite'] == 1
    assert a['psnr'] == (p(4.0) + p(16.0) + p(8.0)) / 3 and a['ssim'] == (0.5 + 1.0 + 0.25) / 3
    # the file is the same whatever order the images came in
    order = [2, 0, 3, 1]
    t = M.summarise([names[i] for i in order], [groups[i] for i in order], rows[order])
    assert M.dumps(s) == M.dumps(s) and json.loads(M.dumps(s)) == json.loads(json.dumps(s))
    assert json.loads(M.dumps(t))['images'] == json.loads(M.dumps(s))['images']
    assert M.dumps(M.summarise(names, groups, rows)) == M.dumps(s)
    assert 'n 4' in M.all_line(s) and '(1 infinite)' in M.all_line(s)


def test_both_parsers_accept_metrics():
    import bg_colorization_main as bgcli
    import obj_colorization_main as cli
    assert cli.build_parser().parse_args([]).metrics == 0
    assert cli.build_parser().parse_args(['-mt', '1']).metrics == 1
    assert cli.build_parser().parse_args(['--metrics', '1']).metrics == 1
    assert [f[5] for f in cli.FLAGS if f[0] == 'metrics'] == ['metrics']        # Config.metrics
    assert bgcli.build_parser().parse_args([]).metrics == 0
    assert bgcli.build_parser().parse_args(['--metrics', '1']).metrics == 1
    for parser in (cli.build_parser(), bgcli.build_parser()):
        with pytest.raises(SystemExit):
            parser.parse_args(['--metrics', '2'])
        assert '--metrics' in parser.format_help()


def test_bg_metrics_in_train_mode_is_refused_before_the_trainer(tmp_path, monkeypatch):
    import bg_colorization_main as bgcli
    from sketchyscenecolorization_amd import bg_colorization
    built = []

    class FakeTrainer(object):
        def __init__(self, **kw):
            built.append(kw)
            raise _Reached()

    monkeypatch.setattr(bg_colorization, 'BGTrainer', FakeTrainer)
    monkeypatch.chdir(tmp_path)
    with pytest.raises(ValueError, match='--metrics 1'):
        bgcli.main(['--mode', 'train', '--metrics', '1', '--image_size', '32', '--max_steps', '2'])
    assert not built
    with pytest.raises(_Reached):
        bgcli.main(['--mode', 'train', '--metrics', '0', '--image_size', '32', '--max_steps', '2'])
    assert len(built) == 1


def test_the_two_oracles_agree():
    """13 x 12 x 3 random bytes: the separable pass and the direct 121-term windows, 3 x 2 windows, to 1e-12; and on a pair
    that differs by small noise, where SSIM is near 1 and the variances are differences of large terms."""
    from sketchyscenecolorization_amd import metrics as M
    win = M.ssim_window()
    rng = np.random.RandomState(3)
    a = rng.randint(0, 256, (13, 12, 3)).astype(np.uint8)
    b = rng.randint(0, 256, (13, 12, 3)).astype(np.uint8)
    near = np.clip(a.astype(np.int32) + rng.randint(-2, 3, a.shape), 0, 255).astype(np.uint8)
    for x, y in ((a, b), (a, near), (a, a)):
        s, d = MO.ssim_map_separable(x, y, win), MO.ssim_map_direct(x, y, win)
        assert s.shape == d.shape == (3, 2, 3)
        assert np.abs(s - d).max() <= 1e-12, np.abs(s - d).max()
    assert np.abs(MO.ssim_map_separable(a, a, win) - 1.0).max() <= 1e-12
    assert MO.ssim_map_separable(a, near, win).min() > 0.9 > MO.ssim_map_separable(a, b, win).max()
    mask = (rng.randint(0, 3, (1, 13, 12)) != 0).astype(np.uint8) * 200
    r1, r2 = (MO.rows(a[None], b[None], win, mask, f) for f in (MO.ssim_map_separable, MO.ssim_map_direct))
    assert np.array_equal(r1[:, [0, 1, 2, 4]], r2[:, [0, 1, 2, 4]]) and abs(r1[0, 3] - r2[0, 3]) <= 1e-11
    d = a.astype(np.int64) - b.astype(np.int64)
    keep = mask[0] != 0
    assert r1[0, 0] == np.abs(d)[keep].sum() and r1[0, 2] == keep.sum() and r1[0, 4] == keep[5:8, 5:7].sum()
    assert np.array_equal(MO.rows(a[None, :10], b[None, :10], win)[0, 3:], [0.0, 0.0])       # 10 rows: no window
