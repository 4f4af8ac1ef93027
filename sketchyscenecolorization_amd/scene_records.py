"""The records of a scene's instructions (Pipeline_utils/customization_util.py): which network an instruction goes to, the list
of the instructions that were run on a scene, and taking the last one back.  Host only: nothing here imports torch.

    <results_base_dir>/update_records/<id>_records.json     the list, one record per instruction
    <results_base_dir>/results/<id>/<id>_<k>.png            the result of the k-th instruction, k from 1
    <results_base_dir>/results/<id>/<id>_<k>.json           its report (scene_session.py; the reference has none)

The JSON file has the reference's bytes (indent 4, its key order, no newline at the end), so a directory written here can be
gone on with, or withdrawn from, by the reference, and the other way round.  One deliberate difference:
``append`` is called only after the instruction's PNG is on the disk, so a turn that fails leaves no record."""
import json
import os
from collections import OrderedDict

from .fg_scene import self_category

KEYS = ('colorization_type', 'result_name', 'input_text', 'proc_bg_text')


def colorize_type(text):
    """'FG' when the text names one of the 25 categories (the instance generator's turn), 'BG' otherwise
    (judge_colorize_type): 'the moon in the sky is yellow' is FG, 'make it red' and '' are BG."""
    return 'BG' if self_category(text) is None else 'FG'


def records_path(image_id, results_base_dir):
    return os.path.join(results_base_dir, 'update_records', str(image_id) + '_records.json')


def results_dir(image_id, results_base_dir):
    return os.path.join(results_base_dir, 'results', str(image_id))


def result_name(image_id, k):
    return '%s_%d.png' % (image_id, k)


def report_name(image_id, k):
    return '%s_%d.json' % (image_id, k)


def _ordered(record):
    return OrderedDict((key, record[key]) for key in KEYS)


def read(image_id, results_base_dir):
    """The records of the file, oldest first; [] without a file.  Nothing is created."""
    path = records_path(image_id, results_base_dir)
    if not os.path.isfile(path):
        return []
    with open(path, 'r') as fp:
        return [_ordered(r) for r in json.loads(fp.read())]


def _write(image_id, results_base_dir, records):
    os.makedirs(os.path.join(results_base_dir, 'update_records'), exist_ok=True)
    with open(records_path(image_id, results_base_dir), 'w') as fp:
        fp.write(json.dumps(records, indent=4))


def fetch(image_id, results_base_dir):
    """-> (name of the next result, name of the last one or '', the last record's proc_bg_text or '', the records)
    (fetch_records; the update_records directory is not made here but when a record is written).  As in the reference every
    record's proc_bg_text is the one it was written with: '' until the first BG turn, carried on by the FG turns after it."""
    records = read(image_id, results_base_dir)
    last_name = records[-1]['result_name'] if records else ''
    last_bg_text = records[-1]['proc_bg_text'] if records else ''
    return result_name(image_id, len(records) + 1), last_name, last_bg_text, records


def append(image_id, input_text, results_base_dir, colorization_type, new_name, proc_bg_text, records):
    """Write the records with one more at the end (update_records) -> the new list.  ``records`` is fetch's; an FG turn hands
    fetch's last_bg_text on as ``proc_bg_text``.  Called after <new_name> has been written."""
    if colorization_type not in ('FG', 'BG'):
        raise ValueError("colorization_type %r: 'FG' or 'BG'" % (colorization_type,))
    records = [_ordered(r) for r in records]
    records.append(OrderedDict(zip(KEYS, (colorization_type, new_name, input_text, proc_bg_text))))
    _write(image_id, results_base_dir, records)
    return records


def withdraw(image_id, results_base_dir):
    """Take the last record back (withdraw_records): <id>_<n>.png and, where there is one, its report <id>_<n>.json are removed;
    the records file loses its last entry, and is removed with the only one.  -> the records that are left.
    ValueError without a records file."""
    path = records_path(image_id, results_base_dir)
    if not os.path.isfile(path):
        raise ValueError('No record to withdraw for image %s under %s' % (image_id, results_base_dir))
    records = read(image_id, results_base_dir)
    n = len(records)
    if n == 0:
        raise ValueError('No record to withdraw for image %s: %s holds an empty list' % (image_id, path))
    out_dir = results_dir(image_id, results_base_dir)
    os.remove(os.path.join(out_dir, result_name(image_id, n)))
    report = os.path.join(out_dir, report_name(image_id, n))
    if os.path.isfile(report):
        os.remove(report)
    if n == 1:
        os.remove(path)
        return []
    _write(image_id, results_base_dir, records[:-1])
    return records[:-1]
