#!/usr/bin/env python
"""What an instruction costs through the system command line (sketchyscene_colorization_main.py).

The released configuration with random weights -- the DeepLab matcher at 768 x 768, the MRU instance generator at 192 x 192,
the background generator at 768 x 768 -- on the synthetic scene of fg_scene_rate.py (a house and a road), the house's mask laid
where the matcher predicts, so that the FG instruction paints one instance.  Measured, one configuration after the other:

  session   one SceneSession: per repetition an FG turn and a BG turn (SceneSession.color, files and record included), each
            between device events on the stream and by the wall clock; the two records are withdrawn again outside the timing
  process   the same two instructions as two runs of the command line in fresh processes, snapshots read from a scratch
            directory, wall clock of the whole process
  kernel    hip.scene_change_hist_u8 at 768 x 768 alone, between device events
  host      what is left on the host in a session turn, each alone by the wall clock: the PNG encoding of one 768 x 768 image,
            the read-back of the result

Writes --out (default profiles/system.txt)."""
import argparse
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'scripts'))
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import numpy as np
import torch

S, FG_S, ID = 768, 192, '9996'
FG_TEXT = 'the house is red with a brown roof'
BG_TEXT = 'the sky is pink and the ground is yellow'
CHILD_LIMIT = 420
BIAS = 'text_sketchyscene/m_lstm_output_projection/biases'


def _row(name, values):
    v = np.array(values, dtype=np.float64)
    return '%-100s median %9.3f ms   min %9.3f   max %9.3f' % (name, np.median(v), v.min(), v.max())


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'system.txt'))
    args = ap.parse_args()
    import fg_scene_oracle as FO
    from fg_scene_rate import synthetic_scene
    from sketchyscenecolorization_amd import hip, matching, scene_session, tf_checkpoint
    from sketchyscenecolorization_amd.bg_colorization import BGTrainer
    from sketchyscenecolorization_amd.data_processing.default_vocab import default_vocab_dict
    from sketchyscenecolorization_amd.data_processing.text_processing import load_vocab_dict_from_file
    from sketchyscenecolorization_amd.obj_lib.main_procedure import save_checkpoint
    from sketchyscenecolorization_amd.trainer import GanTrainer
    match_vocab_path = os.path.join(ROOT, 'tests', 'golden', 'match', 'vocab.txt')
    bg_vocab_path = os.path.join(ROOT, 'tests', 'golden', 'bg_aug', 'bg_vocab.txt')
    vocabs = {'match': matching.load_vocab(match_vocab_path), 'fg': default_vocab_dict(), 'bg': load_vocab_dict_from_file(bg_vocab_path)}
    cfg = matching.MatchConfig(size=S)
    need = scene_session.required_bytes(cfg, 'MRU', 58, FG_S, 18, S)
    total = scene_session.check_budget(need, torch.cuda.mem_get_info()[0])
    scene = synthetic_scene(S, np.random.RandomState(S))
    scene['image_id'] = ID
    # the matcher: random weights, the projection's bias at minus the median of up, the house's mask where it predicts
    variables = matching.random_variables(cfg, 1)
    matcher = matching.MatchModel(cfg)
    idx, n = matching.preprocess_sentence(FG_TEXT, vocabs['match'], 15)
    variables[BIAS][:] = 0
    matcher.load_dict(variables)
    variables[BIAS][:] = -float(np.median(matcher.forward(scene['sketch'], idx, n)[0].cpu().numpy()))
    matcher.load_dict(variables)
    predicts = matcher.forward(scene['sketch'], idx, n)[1].cpu().numpy() != 0
    y1, x1, y2, x2 = scene['boxes'][0].tolist()
    assert predicts[y1:y2 + 1, x1:x2 + 1].sum() >= 4, 'the random matcher predicts nothing on the house'
    scene['masks'][0] = np.ascontiguousarray(predicts[y1:y2 + 1, x1:x2 + 1].astype(np.uint8))
    fg = GanTrainer(img=FG_S, seed=1, block_type='MRU')
    bg = BGTrainer(image_size=S, seed=1)
    lines = ['system_rate.py: matcher deeplab %d x %d, instance generator MRU %d x %d, background generator %d x %d, random weights, '
             '%d repetitions after a warm-up, %s, library %s' % (S, S, FG_S, FG_S, S, S, args.reps, torch.cuda.get_device_name(0),
                                                                  hip.build_hash()),
             'budgeted before allocation: %d bytes (%s)' % (total, ', '.join('%s %d' % kv for kv in sorted(need.items()))), '']
    with tempfile.TemporaryDirectory() as base:
        FO.write_scene(os.path.join(base, 'data'), ID, scene)
        # ---------------------------------------------------------------- session
        session = scene_session.SceneSession(matcher, fg, bg, vocabs, os.path.join(base, 'data'), os.path.join(base, 'session'), S,
                                             noise_seed=3)
        t0 = time.perf_counter()
        session.open(ID)
        torch.cuda.synchronize()
        open_ms = (time.perf_counter() - t0) * 1e3
        t = {k: [] for k in ('fg dev', 'fg wall', 'bg dev', 'bg wall')}
        reports = {}
        for rep in range(args.reps + 1):
            for kind, text in (('fg', FG_TEXT), ('bg', BG_TEXT)):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                w0 = time.perf_counter()
                e0.record()
                reports[kind] = session.color(text)
                e1.record()
                torch.cuda.synchronize()
                w1 = time.perf_counter()
                if rep:
                    t[kind + ' dev'].append(e0.elapsed_time(e1))
                    t[kind + ' wall'].append((w1 - w0) * 1e3)
            session.withdraw()
            session.withdraw()
        lines.append('session: open (files, uploads, backbone once) %.1f ms; the FG turn matched %s and changed %d pixels, the BG turn %d'
                     % (open_ms, reports['fg']['matched_inst_indices'], sum(reports['fg']['changed']['instances'].values())
                        + reports['fg']['changed']['background'], sum(reports['bg']['changed']['instances'].values())
                        + reports['bg']['changed']['background']))
        lines.append(_row('FG turn in a session (head of the matcher, one instance, files and record), device events', t['fg dev']))
        lines.append(_row('FG turn in a session, wall clock', t['fg wall']))
        lines.append(_row('BG turn in a session (one forward pass at 768 x 768, two PNGs, report and record), device events', t['bg dev']))
        lines.append(_row('BG turn in a session, wall clock', t['bg wall']))
        # ---------------------------------------------------------------- kernel and the host's share
        prev, new = session.resident['sketch'], session.current.clone()
        new[100:300, 50:400] = 7
        out = torch.empty(256, dtype=torch.int64, device='cuda')
        tk = []
        for rep in range(21):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            hip.scene_change_hist_u8(prev, new, session.resident['inner'], out=out)
            e1.record()
            torch.cuda.synchronize()
            if rep:
                tk.append(e0.elapsed_time(e1))
        lines.append(_row('ssc_scene_change_hist_u8 at 768 x 768 (its memset included), device events', tk))
        th = {'png': [], 'read': []}
        for rep in range(args.reps + 1):
            w0 = time.perf_counter()
            host = new.cpu().numpy()
            w1 = time.perf_counter()
            scene_session._write_png(os.path.join(base, 'probe.png'), host)
            w2 = time.perf_counter()
            if rep:
                th['read'].append((w1 - w0) * 1e3)
                th['png'].append((w2 - w1) * 1e3)
        lines.append(_row('host: read-back of one 768 x 768 result, wall clock', th['read']))
        lines.append(_row('host: PNG encoding of one 768 x 768 image (a BG turn writes two), wall clock', th['png']))
        # ---------------------------------------------------------------- fresh processes
        os.makedirs(os.path.join(base, 'match'))
        tf_checkpoint.write_checkpoint(os.path.join(base, 'match', 'model-1'), variables)
        with open(os.path.join(base, 'match', 'checkpoint'), 'w') as fp:
            fp.write('model_checkpoint_path: "model-1"\n')
        save_checkpoint(fg.store, os.path.join(base, 'fg'), 'model_9.ckpt', 9)
        os.makedirs(os.path.join(base, 'bg'))
        torch.save(bg.store.state_dict(), os.path.join(base, 'bg', 'snapshot-2'))
        with open(os.path.join(base, 'bg', 'checkpoint'), 'w') as fp:
            fp.write('model_checkpoint_path: "snapshot-2"\n')
        with open(os.path.join(base, 'fg_vocab.txt'), 'w') as fp:
            fp.write('\n'.join(sorted(vocabs['fg'], key=vocabs['fg'].get)))
        session.close()
        del session, matcher, fg, bg
        torch.cuda.empty_cache()
        common = [sys.executable, os.path.join(ROOT, 'sketchyscene_colorization_main.py'), '--image_id', ID, '--data_base_dir',
                  os.path.join(base, 'data'), '--results_base_dir', os.path.join(base, 'process'), '--match_snapshot_root',
                  os.path.join(base, 'match'), '--match_vocab_path', match_vocab_path, '--fgcolor_snapshot_root', os.path.join(base, 'fg'),
                  '--fgcolor_vocab_path', os.path.join(base, 'fg_vocab.txt'), '--bg_snapshot_root', os.path.join(base, 'bg'),
                  '--bg_vocab_path', bg_vocab_path, '--noise_seed', '3']
        for kind, text in (('FG', FG_TEXT), ('BG', BG_TEXT)):
            w0 = time.perf_counter()
            run = subprocess.run(common + ['--instruction', text], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                                 universal_newlines=True, timeout=CHILD_LIMIT, cwd=base)
            w1 = time.perf_counter()
            if run.returncode != 0:
                raise SystemExit('the %s process failed:\n%s' % (kind, run.stdout[-3000:]))
            line = [ln for ln in run.stdout.splitlines() if ln.startswith(kind + ' ')]
            lines.append('%-100s once   %9.1f ms   (%s)' % ('%s instruction as the command line in a fresh process (three snapshots read), wall clock'
                                                           % kind, (w1 - w0) * 1e3, line[0] if line else 'no turn line'))
    lines.append('')
    lines.append('left on the host in a session turn: the read-back and PNG encoding above, the report and the record (two small JSON')
    lines.append('files), the tokenisers, the per-instance resize tables and, for the report, the host copies of the instance sketches')
    text = '\n'.join(lines) + '\n'
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as fp:
        fp.write(text)
    print(text, end='')


if __name__ == '__main__':
    main()
