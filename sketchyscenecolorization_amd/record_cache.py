"""Device-resident record cache of Foreground training (obj_colorization_main.py --record_cache device).

A record of data/tfrecord/train holds two 384 x 384 x 3 uint8 images (884 KB) and never changes.  ``RecordCache`` reads every
record once -- CRC-checked and parsed like the training queue does -- and keeps the images on the device as uint8, with the
minimum and maximum the decode normalises by and, under --distance_map 1, the distance map in place of the sketch.  A train
step then uploads record numbers only and one launch gathers and decodes the batch (hip.decode_paired_cached_u8, called by
obj_lib.input_pipeline.PairedQueue(record_cache=...)): no image crosses the host-device link after start-up.

0.88 MB per record; 2.2 MB with the distance maps (float, instead of the uint8 sketch).

--val_freq keeps a second cache, over data/tfrecord/val, beside the training one (train_validation.py): ``get_record_cache``
keeps one cache per directory, and a cache built while others are held counts their bytes against the same half of the device.
"""
import os
import time

import numpy as np
import torch

from . import tfrecord

RECORD_HW = 384         # the records hold 384 x 384 x 3 uint8 images (obj_lib/input_pipeline.py)
T_STEPS = 15
CHUNK = 32              # records per pinned staging buffer and upload
DM_CHUNK = 4            # records per distance-transform call (its workspace is twice its float output)


def list_record_files(data_dir):
    """The files of a record directory in the order the training queue numbers them."""
    return sorted(os.path.join(data_dir, f) for f in os.listdir(data_dir) if os.path.isfile(os.path.join(data_dir, f)))


def files_key(files):
    return tuple((p, os.path.getsize(p), os.stat(p).st_mtime_ns) for p in files)


class RecordCache(object):
    """img, sk uint8 [S,384,384,3] on ``device``, records numbered in (sorted file, position) order; ``class_id`` int32 [S],
    ``text`` int32 [S,15], ``category`` and ``name`` (lists) on the host; ``file_range[path]`` = (first, end) record number of a
    file.  On a GPU also ``mnmx`` float [S,2], the minimum and maximum of each image resized to ``size`` (exact, so computed
    once), and with ``distance_map`` ``skf`` float [S,384,384,3] from hip.distance_map_u8 -- ``sk`` is then not kept.
    ``device='cpu'`` holds everything but ``mnmx`` and ``skf`` (the host logic without a GPU).
    ``max_records``: the first that many records only, in the same order (--val_records).  ``reserved``: bytes of the caches
    already held on the device -- the limit of half the free memory applies to all of them together."""

    def __init__(self, files, size, distance_map=False, device='cuda', max_records=None, reserved=0):
        t0 = time.time()
        self.device = torch.device(device)
        self.files, self.size, self.distance_map = list(files), int(size), bool(distance_map)
        on_gpu = self.device.type == 'cuda'
        R = RECORD_HW
        assert R % self.size == 0
        counts = [tfrecord.count_records(p) for p in self.files]
        if max_records is not None:     # the first max_records records: whole files, then the head of one, then nothing
            left = int(max_records)
            for i, c in enumerate(counts):
                counts[i] = min(c, left)
                left -= counts[i]
        S = int(sum(counts))
        if S == 0:
            raise ValueError('no records in %s' % (self.files,))
        ends = np.cumsum(counts)
        self.file_range = {p: (int(e - c), int(e)) for p, c, e in zip(self.files, counts, ends)}
        per_record = R * R * 3 * (5 if self.distance_map and on_gpu else 2) + 8
        self.nbytes = S * per_record
        if on_gpu:
            free = torch.cuda.mem_get_info(self.device)[0]
            if self.nbytes + reserved > (free + reserved) // 2:
                raise RuntimeError('the record cache needs %d bytes (%d records of %d bytes%s), more than half of the %d bytes free '
                                   'on the device%s: run with --record_cache off%s'
                                   % (self.nbytes, S, per_record, ' with their distance maps' if self.distance_map else '', free,
                                      ' once the %d bytes of the caches already held are counted with it' % reserved if reserved else '',
                                      ' or hold fewer held-out records with --val_records' if (reserved or max_records is not None)
                                      else ''))
        keep_sk = not (self.distance_map and on_gpu)
        self.img = torch.empty((S, R, R, 3), dtype=torch.uint8, device=self.device)
        self.sk = torch.empty((S, R, R, 3), dtype=torch.uint8, device=self.device) if keep_sk else None
        self.skf = None if keep_sk else torch.empty((S, R, R, 3), dtype=torch.float32, device=self.device)
        self.mnmx = torch.empty((S, 2), dtype=torch.float32, device=self.device) if on_gpu else None
        self.class_id = np.zeros(S, np.int32)
        self.text = np.zeros((S, T_STEPS), np.int32)
        self.category, self.name = [], []
        stage = torch.empty((2, min(CHUNK, S), R, R, 3), dtype=torch.uint8)
        if on_gpu:
            stage = stage.pin_memory()
        raw, self._first, k = stage.numpy(), 0, 0
        for path in self.files:
            for rec in tfrecord.read_records(path, views=True):
                if self._first + k == self.file_range[path][1]:     # (max_records: the rest of this file is not held)
                    break
                feat = tfrecord.parse_example(rec, views=True)
                raw[0, k] = np.frombuffer(feat['cartoon_data'][0], dtype=np.uint8).reshape(R, R, 3)
                raw[1, k] = np.frombuffer(feat['sketch_data'][0], dtype=np.uint8).reshape(R, R, 3)
                s = self._first + k
                self.class_id[s] = int(feat['Category_id'][0])
                self.text[s] = np.frombuffer(feat['Text_vocab_indices'][0], dtype=np.uint8).reshape(T_STEPS)
                self.category.append(feat.get('Category', [b''])[0].decode('utf-8', 'replace'))
                self.name.append(feat.get('ImageName', [b''])[0].decode('utf-8', 'replace'))
                k += 1
                if k == stage.shape[1]:
                    self._flush(stage, k)
                    k = 0
            if self._first + k != self.file_range[path][1]:
                raise IOError('%s changed while it was read' % path)
        if k:
            self._flush(stage, k)
        del self._first
        if on_gpu:
            torch.cuda.synchronize(self.device)
        self.build_seconds = time.time() - t0

    def _flush(self, stage, k):
        """The k staged records onto the device, behind them their min / max (and distance maps); the staging buffer is free
        again when this returns."""
        a, b = self._first, self._first + k
        self.img[a:b].copy_(stage[0, :k], non_blocking=True)
        if self.sk is not None:
            self.sk[a:b].copy_(stage[1, :k], non_blocking=True)
        if self.device.type == 'cuda':
            from . import hip
            with torch.cuda.device(self.device):
                hip.decode_minmax_u8(self.img[a:b], self.size, out=self.mnmx[a:b])
                if self.skf is not None:
                    sk = stage[1, :k].to(self.device, non_blocking=True)
                    for j in range(0, k, DM_CHUNK):
                        hip.distance_map_u8(sk[j:j + DM_CHUNK], out=self.skf[a + j:min(a + j + DM_CHUNK, b)])
                torch.cuda.current_stream().synchronize()
        self._first = b

    def __len__(self):
        return int(self.img.shape[0])


_MEMO = {}              # key -> cache, one per directory: a restart after a NaN loss calls train() again in the same process
BUILDS = 0              # caches built by get_record_cache in this process


def get_record_cache(data_dir, size, distance_map=False, device='cuda', max_records=None):
    """The cache of ``data_dir`` for this image size, built on the first call and found again by later ones as long as the
    files (names, sizes, modification times), the size, the distance-map flag, the device and the record limit are the same.
    One cache is kept per directory (the training set and the held-out set live side by side): another key for the same
    directory frees that directory's earlier cache first.  A cache is built with the bytes of the others on its device
    counted against the same limit (``RecordCache(reserved=...)``)."""
    global BUILDS
    files = list_record_files(data_dir)
    where = os.path.abspath(data_dir)
    key = (where, files_key(files), int(size), bool(distance_map), str(torch.device(device)),
           None if max_records is None else int(max_records))
    if key not in _MEMO:
        for k in [k for k in _MEMO if k[0] == where]:
            del _MEMO[k]
        reserved = sum(c.nbytes for c in _MEMO.values() if c.device == torch.device(device) and c.device.type == 'cuda')
        _MEMO[key] = RecordCache(files, size, distance_map, device, max_records=max_records, reserved=reserved)
        BUILDS += 1
    return _MEMO[key]
