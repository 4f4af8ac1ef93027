"""The colour augmentation of the Background module's training set as a table and three small functions.

Restates Background_Colorization/data_preparation/bg_data_generation.py:10-15, 57-59 and 120-160: a base scene has a 'blue' sky
and a 'green' ground; an augmented record keeps its foreground and segment map and paints the sky (segment value 128) and the
ground (255) with one of 11 x 5 colours.  tests/golden/bg_aug/ (written by that reference script) pins the table, the caption
and the formula byte for byte.
"""
import numpy as np

SKY_COLOR = ('blue', 'green', 'cyan', 'red', 'orange', 'yellow', 'brown', 'purple', 'pink', 'black', 'gray')
GROUND_COLOR = ('yellow', 'green', 'black', 'gray', 'brown')
COLOR_MAP = {'blue': (153, 217, 234), 'green': (181, 230, 29), 'cyan': (128, 255, 215), 'red': (237, 28, 36),
             'orange': (255, 127, 39), 'yellow': (255, 242, 0), 'brown': (185, 122, 87), 'purple': (163, 73, 164),
             'pink': (255, 174, 201), 'black': (30, 30, 30), 'gray': (127, 127, 127)}
BASE_PAIR = ('blue', 'green')
# every (sky, ground) with sky != ground, sky-major in the order of the two lists above: 50 pairs, BASE_PAIR is PAIRS[1].
# --recolor 1 draws an index into this tuple per sample.
PAIRS = tuple((s, g) for s in SKY_COLOR for g in GROUND_COLOR if s != g)
SEG_SKY, SEG_GROUND = 128, 255


def caption(sky, ground):
    return 'the sky is ' + sky + ' and the ground is ' + ground


def recolor_record(sky, ground):
    """The 8 bytes hip.bg_stage_cached_u8 takes per sample: {enable, sky r, g, b, ground r, g, b, 0}."""
    return np.array((1,) + COLOR_MAP[sky] + COLOR_MAP[ground] + (0,), dtype=np.uint8)


def recolor(base_bg, seg, sky, ground):
    """The augmented background of (sky, ground) from the base one: base_bg uint8 [..., 3], seg uint8 [...] (the segment png's
    red channel)."""
    out = np.array(base_bg, dtype=np.uint8, copy=True)
    out[seg == SEG_SKY] = COLOR_MAP[sky]
    out[seg == SEG_GROUND] = COLOR_MAP[ground]
    return out
