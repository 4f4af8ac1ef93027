"""bg_colorization_main.py --batch_size N, the host side (no GPU): the flag is honoured up to the point where the trainer is
built, and the draws of a step are batch_size calls of random.randint in order."""
import random

import numpy as np
import pytest


class _Reached(Exception):
    pass


def test_bg_cli_accepts_batch_size(tmp_path, monkeypatch):
    import bg_colorization_main as bgcli
    from sketchyscenecolorization_amd import bg_colorization
    assert bgcli.build_parser().parse_args(['--batch_size', '4']).batch_size == 4
    assert bgcli.build_parser().parse_args([]).batch_size == 1
    seen = {}

    class FakeTrainer(object):
        def __init__(self, **kw):
            seen.update(kw)
            raise _Reached()

    monkeypatch.setattr(bg_colorization, 'BGTrainer', FakeTrainer)
    monkeypatch.chdir(tmp_path)
    with pytest.raises(_Reached):       # not the NotImplementedError that used to refuse every batch but 1
        bgcli.main(['--mode', 'train', '--batch_size', '4', '--image_size', '64', '--max_steps', '2'])
    assert seen['image_size'] == 64 and seen['max_steps'] == 2
    with pytest.raises(ValueError):
        bgcli.main(['--mode', 'train', '--batch_size', '0'])
    text = bgcli.build_parser().format_help()
    assert 'test mode' in text and 'one image per pass' in ' '.join(text.split())


@pytest.mark.parametrize('nb', [1, 3])
def test_bg_cli_batches_are_drawn_one_randint_per_scene(tmp_path, monkeypatch, nb):
    """A fake trainer records what train_step_u8 is fed: per step batch_size scenes, stacked in draw order, uint8 / int32;
    the draws are the sequence of one draw per step, cut into groups of batch_size."""
    import torch
    import bg_colorization_main as bgcli
    from sketchyscenecolorization_amd import bg_colorization
    fed = []

    class FakeScope(object):
        name = 'x'

    class FakeStore(object):
        generator = discriminator = FakeScope()

        def parameter_count(self, scope):
            return 0

    class FakeTrainer(object):
        def __init__(self, **kw):
            self.store, self.global_step = FakeStore(), 0

        def train_step_u8(self, fg, bg, tok, lab):
            fed.append((fg.numpy().copy(), bg.numpy().copy(), np.array(tok), lab.numpy().copy(), fg.dtype, lab.dtype))
            self.global_step += 1

    class FakeEvent(object):
        def synchronize(self):
            pass

        def record(self):
            pass

    monkeypatch.setattr(bg_colorization, 'BGTrainer', FakeTrainer)
    monkeypatch.setattr(torch.cuda, 'Event', FakeEvent)
    monkeypatch.setattr(torch.Tensor, 'pin_memory', lambda self: self)
    monkeypatch.chdir(tmp_path)
    steps = 6        # more steps than the staging ring has buffers
    random.seed(5)
    bgcli.main(['--mode', 'train', '--batch_size', str(nb), '--image_size', '32', '--max_steps', str(steps), '--save_freq', '0',
                '--progress_freq', '0', '--summary_freq', '0'])
    random.seed(5)
    random.randint(0, 2 ** 31 - 1)      # the trainer's seed
    scenes = bgcli.Scenes({'image_size': 32, 'text_len': 8, 'data_base_dir': 'data', 'mode': 'train', 'vocab_size': 18})
    assert len(fed) == steps
    for fg, bg, tok, lab, fg_dtype, lab_dtype in fed:
        want = [scenes.get(random.randint(0, len(scenes) - 1)) for _ in range(nb)]
        assert fg.shape == (nb, 32, 32, 3) and lab.shape == (nb, 32, 32) and tok.shape == (nb, 8)
        assert fg_dtype == torch.uint8 and lab_dtype == torch.int32
        for i, w in enumerate(want):
            assert np.array_equal(fg[i], w[0][0]) and np.array_equal(bg[i], w[1][0])
            assert np.array_equal(tok[i], w[2][0]) and np.array_equal(lab[i], w[3][0])
