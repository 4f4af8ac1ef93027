"""Generate tests/golden/system/ by IMPORTING the reference's pure-Python Pipeline_utils/customization_util.py and by reading
the argument parser of its sketchyscene_colorization_main.py (only possible where the reference lies; its root is the one
argument, as make_text_goldens.py has it built in).  The committed fixtures hold recorded results and settings only:

    records.json    a sequence of turns (FG, BG, FG, withdraw, withdraw, withdraw, FG) run through fetch_records /
                    update_records / withdraw_records in a scratch directory, the colourizers replaced by an empty PNG of the
                    result's name: after every step what fetch_records returned, the bytes of the records file (null: no file)
                    and the listing of results/<id>/; and judge_colorize_type's answer for a list of sentences
    parser.json     the flags of the command line: names, short forms, types, defaults and choices, in the order they are added

    python tests/golden/make_system_goldens.py /path/to/reference"""
import ast
import contextlib
import io
import json
import os
import sys
import tempfile

if len(sys.argv) != 2:
    raise SystemExit(__doc__)
REF = sys.argv[1]
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'system')
sys.path.insert(0, REF)
from Pipeline_utils import customization_util as ref   # noqa: E402

IMAGE_ID = 9996
STEPS = [('color', 'the bus on the left is yellow with blue windows', ''),
         ('color', 'the sky is pink and the ground is yellow', 'the sky is pink and the ground is yellow'),
         ('color', 'all the trees are dark green', ''),
         ('withdraw', '', ''), ('withdraw', '', ''), ('withdraw', '', ''),
         ('color', 'the sky is red', 'the sky is red and the ground is green')]
SENTENCES = ['the moon in the sky is yellow', 'make it red', '', 'the sky is blue and the ground is green',
             'the bus on the left is yellow with blue windows', 'all the people have red shirts', 'The ground is brown',
             'the Sheep are white', 'a semi-truck is cyan', 'the land is orange and the sky is purple']


def records_state(base):
    path = os.path.join(base, 'update_records', '%d_records.json' % IMAGE_ID)
    text = None
    if os.path.isfile(path):
        with open(path, 'rb') as fp:
            text = fp.read().decode('utf-8')
    res = os.path.join(base, 'results', str(IMAGE_ID))
    return text, sorted(os.listdir(res)) if os.path.isdir(res) else []


def run_records():
    steps = []
    with tempfile.TemporaryDirectory() as base, contextlib.redirect_stdout(io.StringIO()):
        for op, text, proc_bg in STEPS:
            step = {'op': op}
            if op == 'color':
                kind = ref.judge_colorize_type(text)
                new_name, last_name, last_bg_text, summary = ref.fetch_records(IMAGE_ID, base)
                os.makedirs(os.path.join(base, 'results', str(IMAGE_ID)), exist_ok=True)
                open(os.path.join(base, 'results', str(IMAGE_ID), new_name), 'wb').close()     # the colourizer's part
                proc = last_bg_text if kind == 'FG' else proc_bg
                ref.update_records(IMAGE_ID, text, base, kind, new_name, proc, summary)
                step.update(input_text=text, colorization_type=kind, proc_bg_text=proc, new_name=new_name, last_name=last_name,
                            last_bg_text=last_bg_text)
            else:
                ref.withdraw_records(IMAGE_ID, base)
            step['records_file'], step['listing'] = records_state(base)
            steps.append(step)
        try:
            ref.withdraw_records(IMAGE_ID, os.path.join(base, 'nothing_here'))
            refused = False
        except Exception:
            refused = True
    return {'image_id': IMAGE_ID, 'steps': steps, 'withdraw_without_a_file_raises': refused,
            'sentences': [{'text': s, 'colorization_type': ref.judge_colorize_type(s)} for s in SENTENCES]}


def read_parser():
    """The add_argument calls of the reference's command line, read from its syntax tree: nothing of it is run."""
    with open(os.path.join(REF, 'sketchyscene_colorization_main.py')) as fp:
        tree = ast.parse(fp.read())
    flags = []
    for node in ast.walk(tree):
        if isinstance(node, ast.Call) and isinstance(node.func, ast.Attribute) and node.func.attr == 'add_argument':
            names = [ast.literal_eval(a) for a in node.args]
            kw = {k.arg: k.value for k in node.keywords}
            flags.append({'long': [n for n in names if n.startswith('--')][0], 'short': [n for n in names if not n.startswith('--')][0],
                          'type': kw['type'].id, 'default': ast.literal_eval(kw['default']),
                          'choices': ast.literal_eval(kw['choices']) if 'choices' in kw else None, 'line': node.lineno})
    flags.sort(key=lambda f: f.pop('line'))
    return {'flags': flags}


if __name__ == '__main__':
    os.makedirs(OUT, exist_ok=True)
    for name, data in (('records.json', run_records()), ('parser.json', read_parser())):
        with open(os.path.join(OUT, name), 'w') as fp:
            json.dump(data, fp, indent=1)
            fp.write('\n')
        print('wrote', os.path.join(OUT, name))
