"""The host side of the scene's instance colorization (sketchyscenecolorization_amd/fg_scene.py, obj_colorization_main.py --mode
scene) and the NumPy + PIL oracle the device tests compare with (tests/fg_scene_oracle.py): text segmentation, the class map, the
road test's closed form against the reference's loop, the loader and the command line's refusals.  No GPU."""
import os

import numpy as np
import pytest

import fg_scene_oracle as O


# ---------------------------------------------------------------------------------------------------------------
# the instruction
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('text, want', [
    ('the bus on the left is yellow with blue windows', 'the bus is yellow with blue windows'),       # the docstring's case
    # judging_preposition's three sentences, about a category the lists know
    ('a person has red shirt with blue pants', 'the person has red shirt with blue pants'),
    ('a person with blue pants has red shirt', 'a person with blue pants has red shirt'),             # 'with' before the verb
    ('a person in red shirt has blue pants', 'a person in red shirt has blue pants'),                 # a colour before the verb
    ('the yellow bus on the left is big', 'the yellow bus on the left is big'),                       # a colour before the verb
    ('the two cars on the right are red', 'the car are red'),                                          # plural -> the singular
    ('all the buses have blue windows', 'the bus have blue windows'),
    ('the bus on the left', 'the bus on the left'),                                                   # no verb
    ('the bus on the left is big', 'the bus on the left is big'),                                     # no colour at all
    ('The Bus On The Left is Yellow', 'the bus is Yellow'),                                           # words are lowered, the cut is not
    # the substring trap: 'is' is found inside 'this', and the text is cut there
    ('this bus is yellow', 'the bus is bus is yellow'),
    ('the chase car is red', 'the car hase car is red'),                                              # 'has' inside 'chase'
])
def test_segment_user_input_text(text, want):
    from sketchyscenecolorization_amd import fg_scene
    assert fg_scene.segment_user_input_text(text) == want


def test_judging_preposition_sentences():
    from sketchyscenecolorization_amd import fg_scene
    assert fg_scene.judging_preposition('a man has red shirt with blue pants', 'has') is True
    assert fg_scene.judging_preposition('a man with blue pants has red shirt', 'has') is False
    assert fg_scene.judging_preposition('a man in red shirt has blue pants', 'has') is True


@pytest.mark.parametrize('text, why', [
    ('this bus with blue windows', 'inside another word'),      # 'is' only inside 'this', 'with' a word: list.index fails
    ('a man has red shirt with blue pants', 'no category'),     # 'man' is in neither category list: 'the ' + None
])
def test_segment_user_input_text_refuses(text, why):
    from sketchyscenecolorization_amd import fg_scene
    with pytest.raises(ValueError) as e:
        fg_scene.segment_user_input_text(text)
    assert why in str(e.value)


def test_class_map_and_word_lists():
    from sketchyscenecolorization_amd import fg_scene
    from sketchyscenecolorization_amd.obj_lib.main_procedure import CATEGORIES
    m = fg_scene.CLASS_TO_COLOR_ID
    assert len(m) == 25 and sorted(m.values()) == list(range(25)) and list(m) == sorted(m)
    assert (m[7], m[27], m[36], m[41], m[43], m[44]) == (0, 12, 19, 22, 23, 24) and 41 in m and 40 not in m and 0 not in m
    assert fg_scene.ROAD_LABEL == 36 and fg_scene.GRASS_LABEL == 27
    # the generator's labels are positions in the sorted category list: grass 12, road 19
    assert CATEGORIES[m[fg_scene.GRASS_LABEL]] == 'grass' and CATEGORIES[m[fg_scene.ROAD_LABEL]] == 'road'
    assert len(fg_scene.CATEGORIES) == len(fg_scene.CATEGORIES_PLURAL) == 25 and sorted(fg_scene.CATEGORIES) == sorted(CATEGORIES)
    assert fg_scene.CATEGORIES_PLURAL[fg_scene.CATEGORIES.index('person')] == 'people' and fg_scene.self_category('two people') == 'person'
    assert fg_scene.SIMPLE_COLORS[:2] == ['brown', 'gray'] and len(fg_scene.SIMPLE_COLORS) == 12


# ---------------------------------------------------------------------------------------------------------------
# the oracle: the road test's closed form against the loop
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('s, pw', [(8, 2), (33, 2), (33, 25), (48, 25)])
def test_road_closed_form_equals_the_loop(s, pw):
    cases = O.road_cases(s, pw)
    rng = np.random.RandomState(s * 100 + pw)
    for i in range(15):
        density = rng.choice([0.02, 0.1, 0.3, 0.6])
        a = np.where(rng.rand(s, s) < density, rng.choice([0, 100, 234], (s, s)), rng.choice([235, 255], (s, s)))
        cases['random_%d' % i] = O.grey(a)
    verdicts = set()
    for name, sk in cases.items():
        before = sk.copy()
        assert O.road_counts(sk) == O.road_loop(sk, pw, counts=True), name
        assert O.road_closed(sk, pw) == O.road_loop(sk, pw), name
        assert np.array_equal(sk, before), name
        verdicts.add(O.road_loop(sk, pw))
    assert verdicts == {True, False}
    assert O.road_counts(cases['white']) == (0, 0) and O.road_counts(cases['one_line']) == (0, 0)
    assert O.road_counts(cases['two_lines_%d' % pw])[0] == pw and O.road_loop(cases['two_lines_%d' % pw], pw)
    assert O.road_counts(cases['two_lines_%d' % (pw - 1)]) == (pw - 1, 0) and not O.road_loop(cases['two_lines_%d' % (pw - 1)], pw)
    assert O.road_counts(cases['two_vertical']) == (0, s) and O.road_counts(cases['thick']) == (s, 0)
    # every column but the last crosses the first and the last row (two runs); the last column and every row are one run
    assert O.road_counts(cases['last_row_and_column']) == (s - 1, 0)
    assert O.road_counts(cases['grey_234_235']) == (0, 0) and O.road_counts(cases['grey_234_234']) == (s, 0)


def test_oracle_mask_image_and_paste_by_hand():
    small = np.array([[1, 0, 2, 1], [0, 1, 1, 1], [1, 1, 1, 1]], np.uint8)      # bh = 2, bw = 3
    img = O.mask_image(small)
    assert img.shape == (2, 3, 3) and img[:, :, 0].tolist() == [[0, 255, 255], [255, 0, 0]] and (img[:, :, 0] == img[:, :, 2]).all()
    result = np.arange(5 * 4 * 3, dtype=np.uint8).reshape(5, 4, 3)
    inner = np.array([[0, 0, 0, 0], [0, 2, 1, 0], [0, 2, 2, 2], [0, 0, 2, 0], [2, 0, 0, 0]], np.uint8)
    inst = np.full((2, 3, 3), 200, np.uint8) + np.arange(6, dtype=np.uint8).reshape(2, 3, 1)
    out = O.paste(result, inner, inst, (1, 1, 3, 4), 2)
    changed = (out != result).any(-1)
    assert changed.tolist() == [[False] * 4, [False, True, False, False], [False, True, True, True], [False] * 4, [False] * 4]
    assert out[1, 1].tolist() == [200] * 3 and out[2, 3].tolist() == [205] * 3


def test_fixture_holds_what_the_chain_tests_need():
    from sketchyscenecolorization_amd import fg_scene
    import bg_scene_oracle as B
    scenes = O.load_scenes()
    ex, sy = scenes['example'], scenes['synthetic']
    assert ex['class_ids'].tolist() == [36, 43, 43, 43, 43, 43, 43, 15, 32] and ex['boxes'][4, 3] == 191
    fg_scene.check_instances('example', ex['boxes'], ex['masks'], ex['class_ids'], 192, 192)
    fg_scene.check_instances('synthetic', sy['boxes'], sy['masks'], sy['class_ids'], 96, 96)
    for sc, ks in ((ex, range(1, 9)), (sy, range(5))):
        drawn = B.drawn_region(sc['sketch'], sc['inner'], B.grass_table(sc['class_ids']))
        for k in ks:
            y1, x1, y2, x2 = sc['boxes'][k]
            own = np.zeros(sc['inner'].shape, bool)
            own[y1:y2, x1:x2] = sc['inner'][y1:y2, x1:x2] == k + 1
            assert own.sum() >= 200, k
            if sc['class_ids'][k] != O.GRASS_LABEL:
                assert (drawn & own).sum() >= 40, k
    # the road of the example has no pixel of its own and is a single line, at both generator sizes
    y1, x1, y2, x2 = ex['boxes'][0]
    assert not (ex['inner'][y1:y2, x1:x2] == 1).any()
    assert O.road_counts(O.instance_sketch(ex, 0, 64)) == (0, 1) and not O.road_loop(O.instance_sketch(ex, 0, 64))
    assert not O.road_loop(O.instance_sketch(ex, 0, 192))
    # the synthetic scene
    assert sy['class_ids'].tolist() == [27, 36, 15, 40, 43] and 40 not in fg_scene.CLASS_TO_COLOR_ID
    assert O.road_loop(O.instance_sketch(sy, 1, 64)) and O.road_counts(O.instance_sketch(sy, 1, 64))[0] >= 25
    assert tuple(sy['boxes'][2, 2:] - sy['boxes'][2, :2]) == (64, 64) and tuple(sy['boxes'][4, 2:]) == (96, 96)
    assert {int(b[1]) % 2 for b in sy['boxes']} == {0, 1}
    assert all(set(np.unique(m)) == {0, 1, 2} for m in sy['masks'])
    moved = B.moved(sy['sketch'])[:, :, 0] == 0
    assert (moved & (sy['inner'] == 1)).sum() >= 1 and not (B.drawn_region(sy['sketch'], sy['inner'], B.grass_table(sy['class_ids']))
                                                           & (sy['inner'] == 1)).any()
    # the exact-size box goes in without a resize: the sketch is the mask image itself
    assert np.array_equal(O.instance_sketch(sy, 2, 64), O.mask_image(sy['masks'][2]))


# ---------------------------------------------------------------------------------------------------------------
# the loader
# ---------------------------------------------------------------------------------------------------------------
def test_load_instances_and_its_refusals(tmp_path):
    from sketchyscenecolorization_amd import fg_scene
    sy = O.load_scenes()['synthetic']
    base = str(tmp_path)
    O.write_scene(base, 5, sy)
    got = fg_scene.load_instances(base, 5, 96)
    assert got['image_id'] == '5' and np.array_equal(got['sketch'], sy['sketch']) and np.array_equal(got['inner'], sy['inner'])
    assert got['boxes'].dtype == np.int32 and np.array_equal(got['boxes'], sy['boxes']) and got['class_ids'].tolist() == sy['class_ids'].tolist()
    assert len(got['masks']) == 5 and all(a.dtype == np.uint8 and np.array_equal(a, b) for a, b in zip(got['masks'], sy['masks']))
    bad_mask = [m.copy() for m in sy['masks']]
    bad_mask[3] = bad_mask[3][:-1]                      # (bh, bw + 1): the expanded slice would not take it
    for name, boxes, masks in (('mask', None, bad_mask),
                               ('below', np.array(sy['boxes'].tolist()[:4] + [[66, 61, 97, 96]]), None),
                               ('right', np.array(sy['boxes'].tolist()[:4] + [[66, 61, 96, 97]]), None),
                               ('negative', np.array([[-1, 5, 29, 51]] + sy['boxes'].tolist()[1:]), None),
                               ('empty', np.array(sy['boxes'].tolist()[:3] + [[2, 3, 2, 25]] + sy['boxes'].tolist()[4:]), None)):
        if boxes is not None:       # the masks follow the boxes, so that it is the box that is refused
            masks = [np.zeros((max(b[2] - b[0], 0) + 1, max(b[3] - b[1], 0) + 1), np.uint8) for b in boxes.tolist()]
        O.write_scene(base, 6, sy, boxes, masks)
        with pytest.raises(ValueError) as e:
            fg_scene.load_instances(base, 6, 96)
        assert ('mask of instance 3' if name == 'mask' else 'box') in str(e.value), name


# ---------------------------------------------------------------------------------------------------------------
# the command line
# ---------------------------------------------------------------------------------------------------------------
def test_scene_flags_and_their_defaults():
    import obj_colorization_main as cli
    a = cli.build_parser().parse_args([])
    assert (a.scene_dir, a.scene_size, a.image_id, a.inst_indices, a.previous_image, a.noise_seed) == ('examples', 768, None, None, '', -1)
    a = cli.build_parser().parse_args(['--mode', 'scene', '-rf', 's', '--image_id', '9203', '--inst_indices', '7,8', '--instruction',
                                       'the bus is red', '--previous_image', 'p.png', '--scene_dir', 'd', '--noise_seed', '3'])
    assert (a.mode, a.image_id, a.inst_indices, a.instruction, a.previous_image, a.scene_dir, a.noise_seed) == \
        ('scene', '9203', '7,8', 'the bus is red', 'p.png', 'd', 3)
    shorts = [f[1] for f in cli.FLAGS] + [f[1] for f in cli.SCENE_FLAGS]
    assert len(shorts) == len(set(shorts))
    assert cli.scene_arguments(a) == dict(scene_dir='d', scene_size=768, image_id='9203', inst_indices=[7, 8], previous_image='p.png',
                                          noise_seed=3)


SCENE = ['--mode', 'scene', '-rf', '2018-01-02-03-04-05', '--image_id', '1', '--inst_indices', '7,8', '--instruction', 'the bus is red']


@pytest.mark.parametrize('argv', [
    SCENE[:2] + SCENE[4:],                                          # no -rf
    SCENE[:4] + SCENE[6:],                                          # no --image_id
    SCENE[:6] + SCENE[8:],                                          # no --inst_indices
    SCENE[:8],                                                      # no --instruction
    SCENE[:7] + ['7,x'] + SCENE[8:], SCENE[:7] + [''] + SCENE[8:], SCENE[:7] + ['-1'] + SCENE[8:],
    SCENE + ['--scene_size', '0'],
] + [['--mode', mode] + rest + flag
     for mode, rest in (('train', []), ('val', ['-rf', '2018-01-02-03-04-05']), ('test', ['-rf', '2018-01-02-03-04-05']),
                        ('inference', ['-rf', '2018-01-02-03-04-05', '--infer_name', 'car.png', '--instruction', 'the car is red']))
     for flag in (['--scene_dir', 'elsewhere'], ['--image_id', '1'], ['--inst_indices', '7'], ['--previous_image', 'p.png'],
                  ['--noise_seed', '3'], ['--scene_size', '192'])],
    ids=lambda a: ' '.join(a))
def test_command_line_refuses(argv, tmp_path, monkeypatch):
    """Every one of them is refused before anything is loaded, written or run."""
    import obj_colorization_main as cli
    monkeypatch.chdir(tmp_path)
    for name in ('evaluate', 'start_or_resume_training'):
        monkeypatch.setattr(cli, name, lambda *a, **k: pytest.fail('the run was started'))
    with pytest.raises(ValueError):
        cli.main(argv)
    assert os.listdir(str(tmp_path)) == []


def test_scene_mode_reaches_the_procedure_with_checked_arguments(tmp_path, monkeypatch, capsys):
    import obj_colorization_main as cli
    from sketchyscenecolorization_amd.obj_lib import main_procedure
    monkeypatch.chdir(tmp_path)
    seen = []
    monkeypatch.setattr(main_procedure, 'scene', lambda instruction, **kw: seen.append((instruction, kw)))
    cli.main(SCENE + ['-si', '1', '-bt', 'Pix2Pix'])
    assert seen == [('the bus is red', dict(scene_dir='examples', scene_size=768, image_id='1', inst_indices=[7, 8],
                                            previous_image='', noise_seed=-1))]
    from sketchyscenecolorization_amd.obj_lib.config import Config
    assert Config.results_dir == os.path.join('outputs', '2018-01-02-03-04-05', 'scene_results') and Config.small_img == 1
    # a stamp that is none is reported as the other modes report it, and nothing runs
    cli.main(SCENE[:3] + ['nope'] + SCENE[4:])
    assert 'Invalid resume folder' in capsys.readouterr().out and len(seen) == 1
    assert os.listdir(str(tmp_path)) == []
