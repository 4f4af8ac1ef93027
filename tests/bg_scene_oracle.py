"""Float64 NumPy restatement of the scene pipeline's background finishing (Pipeline_utils/bg_utils.py:96-166, 215-224, 290-319),
written from the definitions of DESIGN.md section 8.4: crop, compose and the sky gradient.  rgb2hsv / hsv2rgb are skimage's
formulas array operation by array operation; tests/test_bg_scene.py holds them against matplotlib's."""
import numpy as np

GRASS_LABEL = 27
F = np.float32


def grass_table(class_ids):
    """uint8 [256]: 1 at mask value k + 1 when instance k has class 27; 0 at mask value 0."""
    t = np.zeros(256, np.uint8)
    for k, c in enumerate(np.asarray(class_ids).reshape(-1)[:255]):
        if int(c) == GRASS_LABEL:
            t[k + 1] = 1
    return t


def crop(prev, inner):
    out = np.full(prev.shape, 255, np.uint8)
    out[inner != 0] = prev[inner != 0]
    return out


def unit_to_u8(x):
    """floor(clamp((x + 1) / 2, 0, 1) * 255 + 0.5) clamped to 0..255, each operation rounded to fp32, NaN to 0."""
    x = np.asarray(x, F)
    with np.errstate(invalid='ignore'):
        h = (x + F(1)) / F(2)
        y = np.fmin(np.fmax(h, F(0)), F(1)) * F(255)        # fmax / fmin drop a NaN operand
        q = np.floor(y + F(0.5))
    return np.fmin(np.fmax(q, F(0)), F(255)).astype(np.uint8)


def moved(sketch):
    m = sketch.copy()
    m[1:, 1:] = sketch[:-1, :-1]
    return m


def drawn_region(sketch, inner, grass):
    return (moved(sketch)[:, :, 0] == 0) & (grass[inner] == 0)


def overlay(image, sketch, inner, grass):
    out = image.copy()
    region = drawn_region(sketch, inner, grass)
    out[region] = moved(sketch)[region]
    return out


def compose(img, fg, inner, grass, sketch):
    """img float [H,W,>=3] -> (out, fg_marked)."""
    out = unit_to_u8(img[..., :3])
    out[inner != 0] = fg[inner != 0]
    return overlay(out, sketch, inner, grass), overlay(fg, sketch, inner, grass)


def rgb2hsv(arr):
    """arr float64 [...,3] -> hsv float64 [...,3]."""
    arr = np.asarray(arr, np.float64)
    out = np.zeros_like(arr)
    v = arr.max(-1)
    delta = v - arr.min(-1)
    with np.errstate(invalid='ignore', divide='ignore'):
        s = delta / v
        s[delta == 0.] = 0.
        h = np.zeros_like(v)
        idx = arr[..., 0] == v
        h[idx] = (arr[idx, 1] - arr[idx, 2]) / delta[idx]
        idx = arr[..., 1] == v
        h[idx] = 2. + (arr[idx, 2] - arr[idx, 0]) / delta[idx]
        idx = arr[..., 2] == v
        h[idx] = 4. + (arr[idx, 0] - arr[idx, 1]) / delta[idx]
        h = (h / 6.) % 1.
    h[delta == 0.] = 0.
    out[..., 0], out[..., 1], out[..., 2] = h, s, v
    return out


def hsv2rgb(hsv):
    hsv = np.asarray(hsv, np.float64)
    h, s, v = hsv[..., 0], hsv[..., 1], hsv[..., 2]
    hi = np.floor(h * 6)
    f = h * 6 - hi
    p = v * (1 - s)
    q = v * (1 - f * s)
    t = v * (1 - (1 - f) * s)
    hi = np.stack([hi, hi, hi], -1).astype(np.uint8) % 6
    return np.choose(hi, [np.stack((v, t, p), -1), np.stack((q, v, p), -1), np.stack((p, v, t), -1),
                          np.stack((p, q, v), -1), np.stack((t, p, v), -1), np.stack((v, p, q), -1)])


def sky_gradient(color, inner, search_from=5, search_height=2):
    """-> (out uint8 [H,W,3], status, info) with info = dict(sky_color, sky_bottom, start_height) (None entries where the status
    says they do not exist).  Status 1 and 2 return color unchanged."""
    H, W = inner.shape
    assert search_height >= 1 and search_from >= 0 and search_from + search_height - 1 <= H // 2
    info = {'sky_color': None, 'sky_bottom': None, 'start_height': None}
    img_bg = np.full(color.shape, 255, np.uint8)
    img_bg[inner == 0] = color[inner == 0]
    colours, counts = [], []
    for i in range(search_from, search_from + search_height):
        for j in range(W):
            if inner[i, j] == 0:
                rgb = img_bg[i, j].tolist()
                if rgb in colours:
                    counts[colours.index(rgb)] += 1
                else:
                    colours.append(rgb)
                    counts.append(1)
    if not colours:
        return color.copy(), 1, info
    sky = colours[int(np.argmax(counts))]
    info['sky_color'] = sky
    has = (img_bg == np.array(sky, np.uint8)).all(-1).any(-1)
    sky_bottom = max(i for i in range(H // 2 + 1) if has[i])
    info['sky_bottom'] = sky_bottom
    sh = (3 * sky_bottom) // 4
    if sh == 0:
        return color.copy(), 2, info
    info['start_height'] = sh
    sky_hsv = rgb2hsv((np.array(sky, F) / F(255)).astype(np.float64)[None, None])[0, 0]
    hsv = rgb2hsv(img_bg / 255.)
    end_s = sky_hsv[1] / 3.
    end_v = min(1., sky_hsv[2] * 1.5)
    for i in range(sh, -1, -1):
        hsv[i, :, 1] = (sh - i) / sh * end_s + i / sh * sky_hsv[1]
        hsv[i, :, 2] = (sh - i) / sh * end_v + i / sh * sky_hsv[2]
    rgb = hsv2rgb(hsv)
    rgb *= 255.
    out = rgb.astype(np.uint8)
    out[inner != 0] = color[inner != 0]
    return out, 0, info


def finish(img, prev, inner, class_ids, sketch, color_gradient=True):
    """The whole finishing of build_background_colorization from the generator's float image on -> (background, fg_marked,
    status, info)."""
    grass = grass_table(class_ids)
    fg = crop(prev, inner)
    out, marked = compose(img, fg, inner, grass, sketch)
    status, info = 0, {'sky_color': None, 'sky_bottom': None, 'start_height': None}
    if color_gradient:
        out, status, info = sky_gradient(out, inner)
        if status == 0:
            out = overlay(out, sketch, inner, grass)
    return out, marked, status, info
