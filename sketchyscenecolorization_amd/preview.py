"""Preview sheets of the held-out passes (--val_preview K): what the generator paints, or the matcher
picks, for the first K records of a pass, as one PNG beside a JSON file that names the rows.

A sheet is one uint8 [SH,SW,3] image on the device, filled with 255 once.  Tile (row, column) of th x tw pixels lies at
(PAD + row*(th+PAD), PAD + column*(tw+PAD)); every pass overwrites the same tiles (csrc/preview.hip: ssc_sheet_tiles_u8 reduces
uint8 images by an s x s box mean into a column of tiles, ssc_sheet_overlay_u8 colours a sketch by (predicted, target) first).
The sheet comes to the host once per pass, behind the read-back the pass does anyway.

A preview reads the pass's buffers and writes only its own: the sheet, a uint8 scratch and the matcher's ``up`` / ``predicts``
copies under tags of its own.  It draws from no random generator, so a run with it is the run without it, bit for bit.

The layout arithmetic, the argument checks and the file writing import no torch (the CPU tests read them); the classes that hold
a sheet import it when they are built."""
import json
import os

PAD = 4                 # pixels between tiles and around them
MAX_TILE = 384          # a tile's side is at most this: preview_scale
MAX_PREVIEW = 32        # rows of a sheet: it stays a few MB
SCALES = (1, 2, 4, 6, 8)        # what ssc_sheet_tiles_u8 reduces by
GREEN, RED, BLUE = (0, 170, 0), (230, 0, 0), (0, 90, 255)       # predicted and target, predicted only, target only


def preview_scale(side):
    """What an image of ``side`` pixels is reduced by: 1 up to MAX_TILE, above it the smallest power of two s with
    side / s <= MAX_TILE.  ValueError for a side that s does not divide, or that would need more than 8."""
    side = int(side)
    if side < 1:
        raise ValueError('a preview of an image of %d pixels' % side)
    s = 1
    while side > s * MAX_TILE:
        s *= 2
    if s > 8:
        raise ValueError('an image of %d pixels needs a reduction by %d for a preview tile of at most %d: 8 is the most' % (side, s, MAX_TILE))
    if side % s:
        raise ValueError('an image of %d pixels is not a whole number of %d x %d boxes: no preview tile' % (side, s, s))
    return s


def tile_origin(row, column, th, tw):
    """(top, left) of tile (row, column) of a sheet of th x tw tiles."""
    return PAD + int(row) * (int(th) + PAD), PAD + int(column) * (int(tw) + PAD)


def sheet_shape(rows, columns, th, tw):
    """(SH, SW) of the sheet that holds rows x columns tiles of th x tw pixels."""
    return PAD + int(rows) * (int(th) + PAD), PAD + int(columns) * (int(tw) + PAD)


def grid(tiles, columns=4):
    """(rows, columns) of a sheet of ``tiles`` tiles laid out row by row, ``columns`` to a row (fewer when there are fewer)."""
    tiles = int(tiles)
    c = max(1, min(int(columns), tiles))
    return (tiles + c - 1) // c, c


def checked_count(k, freq, mode='train', flag='--val_preview', freq_flag='--val_freq'):
    """The K of --val_preview: ValueError for a negative one, one above MAX_PREVIEW, one outside --mode train and one without
    held-out passes to draw from.  -> K."""
    k = int(k)
    if k < 0:
        raise ValueError('%s %d: a count of records, 0 for no preview' % (flag, k))
    if k > MAX_PREVIEW:
        raise ValueError('%s %d: at most %d rows (the sheet stays a few MB)' % (flag, k, MAX_PREVIEW))
    if k and mode != 'train':
        raise ValueError('%s %d previews the held-out passes of --mode train, this is --mode %s' % (flag, k, mode))
    if k and not freq:
        raise ValueError('%s %d previews the held-out passes: it needs %s F > 0' % (flag, k, freq_flag))
    return k


def checked_visualized(v, mode):
    """--visualized of match_main.py: 0 or 1, and 1 in --mode eval only.  -> bool."""
    if v not in (0, 1):
        raise ValueError('--visualized %r: 0 or 1' % (v,))
    if v and mode != 'eval':
        raise ValueError("--visualized 1 writes every caption's overlays in --mode eval, this is --mode %s" % mode)
    return bool(v)


def write_png(path, array):
    """uint8 [H,W,3] -> a PNG file."""
    from PIL import Image
    Image.fromarray(array, 'RGB').save(path, 'PNG')


def write_json(path, record):
    with open(path, 'w') as f:
        json.dump(record, f, indent=1, sort_keys=True)
        f.write('\n')


def sheet_record(kind, step, columns, th, tw, scale, rows):
    """The JSON beside a sheet: what it shows, where its tiles lie and one entry per row (or tile)."""
    return {'kind': kind, 'step': int(step), 'columns': list(columns), 'tile': [int(th), int(tw)], 'pad': PAD, 'scale': int(scale),
            'rows': list(rows)}


def write_sheet(directory, stem, image, record):
    """<directory>/<stem>.png and .json -> the PNG's path."""
    os.makedirs(directory, exist_ok=True)
    path = os.path.join(directory, stem + '.png')
    write_png(path, image)
    write_json(os.path.join(directory, stem + '.json'), record)
    return path


# ---------------------------------------------------------------------------------------------------------------------------
# the device side
# ---------------------------------------------------------------------------------------------------------------------------
class Sheet(object):
    """rows x columns tiles of th x tw pixels on ``device``, white."""

    def __init__(self, rows, columns, th, tw, device):
        import torch
        self.rows, self.columns, self.th, self.tw = int(rows), int(columns), int(th), int(tw)
        self.SH, self.SW = sheet_shape(rows, columns, th, tw)
        self.d = torch.full((self.SH, self.SW, 3), 255, dtype=torch.uint8, device=device)

    def tiles(self, src_u8, s, row, column):
        """src uint8 [N,H,W,3] -> the tiles (row .. row + N - 1, column)."""
        from . import hip
        top, left = tile_origin(row, column, self.th, self.tw)
        hip.sheet_tiles_u8(src_u8, s, self.d, top, left, self.th + PAD)

    def overlay(self, sketch_u8, pred_u8, labels_u8, lut_u8, s, row, column):
        from . import hip
        top, left = tile_origin(row, column, self.th, self.tw)
        hip.sheet_overlay_u8(sketch_u8, pred_u8, labels_u8, lut_u8, s, self.d, top, left)

    def host(self):
        """The sheet on the host (it waits for what was launched)."""
        return self.d.cpu().numpy()


class ForegroundPreview(object):
    """The sheet of obj_colorization_main.py --val_preview K over a record cache: a row per record, the columns sketch (left
    out under --distance_map 1, whose cache keeps no sketch bytes), output, target."""

    def __init__(self, cache, count):
        import torch
        self.cache, self.n = cache, min(int(count), len(cache))
        R = int(cache.img.shape[1])
        self.size, self.scale = int(cache.size), R // int(cache.size)
        if self.scale not in SCALES or R % self.size:
            raise ValueError('records of %d pixels for a generator of %d: no preview tile' % (R, self.size))
        self.columns = (['sketch'] if cache.sk is not None else []) + ['output', 'target']
        self.sheet = Sheet(self.n, len(self.columns), self.size, self.size, cache.device)
        self.out_u8 = torch.empty((self.n, self.size, self.size, 3), dtype=torch.uint8, device=cache.device)

    def start(self):
        """The columns that the weights do not touch."""
        if self.cache.sk is not None:
            self.sheet.tiles(self.cache.sk[:self.n], self.scale, 0, 0)
        self.sheet.tiles(self.cache.img[:self.n], self.scale, 0, len(self.columns) - 1)

    def batch(self, out_nhwc, coff, first, end):
        """The generator's NHWC output rows of the records first .. end - 1, straight behind the pass's own forward."""
        from . import hip
        end = min(end, self.n)
        if first >= end:
            return
        hip.image_postprocess_u8(out_nhwc[:end - first], coff, out=self.out_u8[first:end])
        self.sheet.tiles(self.out_u8[first:end], 1, first, len(self.columns) - 2)

    def rows(self, names, groups):
        return [{'name': names[i], 'category': groups[i], 'caption_indices': [int(v) for v in self.cache.text[i]]}
                for i in range(self.n)]

    def write(self, log_dir, step, names, groups):
        record = sheet_record('foreground', step, self.columns, self.size, self.size, self.scale, self.rows(names, groups))
        return write_sheet(os.path.join(log_dir, 'previews'), 'step_%d' % step, self.sheet.host(), record)


class BackgroundPreview(object):
    """The sheet of bg_colorization_main.py --val_preview K over a scene cache: a row per scene, the columns foreground (the
    generator's input), output (the bytes --mode test would write) and background (the target)."""
    COLUMNS = ['foreground', 'output', 'background']

    def __init__(self, cache, count):
        import torch
        self.cache, self.n = cache, min(int(count), len(cache))
        H, W = (int(v) for v in cache.fg.shape[1:3])
        self.scale = preview_scale(max(H, W))
        if H % self.scale or W % self.scale:
            raise ValueError('scenes of %d x %d pixels: no preview tile at a reduction by %d' % (H, W, self.scale))
        self.th, self.tw = H // self.scale, W // self.scale
        self.sheet = Sheet(self.n, 3, self.th, self.tw, cache.device)
        self.out_u8 = torch.empty((1, H, W, 3), dtype=torch.uint8, device=cache.device)

    def scene(self, i, image):
        """Scene i of the pass, straight behind its forward: ``image`` is the generator's float image."""
        from . import hip
        if i >= self.n:
            return
        c = self.cache
        sf, sb, ss = (int(v) for v in c.slots[i])
        hip.bg_finish_u8(image, c.fg[sf:sf + 1], c.seg[ss:ss + 1], out=self.out_u8)
        self.sheet.tiles(c.fg[sf:sf + 1], self.scale, i, 0)
        self.sheet.tiles(self.out_u8, self.scale, i, 1)
        self.sheet.tiles(c.bg[sb:sb + 1], self.scale, i, 2)

    def rows(self, names):
        return [{'name': names[i], 'caption_indices': [int(v) for v in self.cache.tokens[i]]} for i in range(self.n)]

    def write(self, log_dir, step, names):
        record = sheet_record('background', step, self.COLUMNS, self.th, self.tw, self.scale, self.rows(names))
        return write_sheet(os.path.join(log_dir, 'previews'), 'step_%d' % step, self.sheet.host(), record)


class MatchPreview(object):
    """The sheet of match_main.py --mode train --val_preview K: a tile per caption, the first K of a pass, laid out row by row:
    the scene's sketch with the caption's prediction and target over it."""
    UP, PREDICTS = 'preview_up', 'preview_predicts'      # the model's buffer tags that only the preview writes

    def __init__(self, model, captions, count):
        import torch
        self.model, self.n = model, min(int(count), int(captions))
        self.size = int(model.cfg.size)
        self.scale = preview_scale(self.size)
        self.tile = self.size // self.scale
        self.grid = grid(self.n)
        self.sheet = Sheet(self.grid[0], self.grid[1], self.tile, self.tile, model.device)
        self.up = model._buf(self.UP, (self.size, self.size))
        self.predicts = model._buf(self.PREDICTS, (self.size, self.size), torch.uint8)

    def caption(self, k, pred, stroke, sketch, labels, lut):
        """Caption k of the pass, straight behind its head: ``pred`` is the pass's 1/8 map."""
        from . import hip
        if k >= self.n:
            return
        hip.match_finish(pred, stroke, up=self.up, predicts=self.predicts)
        self.sheet.overlay(sketch, self.predicts, labels, lut, self.scale, k // self.grid[1], k % self.grid[1])

    def write(self, log_root, iteration, entries):
        """entries: per caption {scene, caption, I, P, A}."""
        record = sheet_record('match', iteration, ['overlay'], self.tile, self.tile, self.scale, entries[:self.n])
        record['grid'] = list(self.grid)
        record['colours'] = {'predicted_and_target': list(GREEN), 'predicted_only': list(RED), 'target_only': list(BLUE)}
        return write_sheet(os.path.join(log_root, 'match_previews'), 'iter_%d' % iteration, self.sheet.host(), record)


class EvalVisualizer(object):
    """match_main.py --mode eval --visualized 1: per caption <base>/<split>/<image id>/<k>_gt.png (the target over the sketch) and
    <k>_out.png (the prediction over it), full size, and one captions.json per scene."""

    def __init__(self, base_dir, split, size, device):
        import torch
        self.root, self.size, self.device = os.path.join(base_dir, split), int(size), device
        self.sheet = torch.empty((self.size, self.size, 3), dtype=torch.uint8, device=device)
        self.scene_id, self.entries = None, []

    def scene(self, image_id, sketch_host):
        import numpy as np
        import torch
        self.finish()
        self.scene_id, self.entries = str(image_id), []
        self.sketch = torch.from_numpy(np.ascontiguousarray(sketch_host, dtype=np.uint8)).to(self.device)
        os.makedirs(os.path.join(self.root, self.scene_id), exist_ok=True)

    def caption(self, k, caption, text, predicts, labels, lut_host):
        import torch
        from . import hip
        lut = torch.from_numpy(lut_host).to(self.device)
        d = os.path.join(self.root, self.scene_id)
        hip.sheet_overlay_u8(self.sketch, None, labels, lut, 1, self.sheet, 0, 0)
        write_png(os.path.join(d, '%d_gt.png' % k), self.sheet.cpu().numpy())
        hip.sheet_overlay_u8(self.sketch, predicts, None, None, 1, self.sheet, 0, 0)
        write_png(os.path.join(d, '%d_out.png' % k), self.sheet.cpu().numpy())
        self.entries.append({'k': int(k), 'caption': caption, 'text': text, 'gt': '%d_gt.png' % k, 'out': '%d_out.png' % k})

    def finish(self):
        if self.scene_id is not None:
            write_json(os.path.join(self.root, self.scene_id, 'captions.json'), {'image_id': self.scene_id, 'captions': self.entries})
        self.scene_id = None
