"""Digest of a short Foreground or Background training run, for comparing two trees bit for bit.

One configuration = 5 calls of ``GanTrainer.train_iteration`` at img 64, batch 2, on fixed synthetic batches with
``next_batch_d`` passed (the first call of a step shape runs eagerly, the second captures it, three replay).  After each
iteration the two losses are printed as ``float.hex``; at the end the SHA-256 of the generator's and the discriminator's
weights, of both second-moment buffers and of every spectral-norm ``u``.  Only the trainer's constructor arguments,
``train_iteration`` and ``synthetic.synthetic_batch`` are used, so the file runs unchanged in an older checkout.
``background``: 4 calls of ``BGTrainer.train_step`` at image size 64 (the smallest the generator's depth takes), batch 2, on
fixed random tensors; the five losses as ``float.hex`` per step, then the same hashes plus both first-moment buffers.
``background_inline`` is that run with SSC_BG_OVERLAP_REAL=0 (no side stream), ``background_eager`` with ``use_graphs=False``;
``background_u8`` feeds ``train_step_u8`` fixed random uint8 scenes and int32 labels; ``background_cached`` feeds
``train_step_cached`` from a ``SceneCache`` over the command line's eight synthetic scenes, the slots of each step and the
recolour record of the second drawn from the same seeded generator.  Only the three entry points and their documented arguments
are used.

    python scripts/train_state_digest.py                    every configuration, each a process of its own, three at a time
    python scripts/train_state_digest.py --config NAME      one configuration in this process (two ranks: two children)
    python scripts/train_state_digest.py --list
"""
import argparse
import hashlib
import os
import socket
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
IMG, NB, ITERS = 64, 2, 5

# name -> (world, GanTrainer arguments, environment).  "Default" is what bench.py and the command line run: captured steps.
CONFIGS = {
    'pix2pix': (1, dict(use_graphs=True), {}),
    'pix2pix_eager_inline': (1, dict(use_graphs=False, overlap_real=False), {}),
    'pix2pix_dbwd_inline': (1, dict(use_graphs=True), {'SSC_DBWD_CONCURRENT': '0'}),
    'pix2pix_no_real_ahead': (1, dict(use_graphs=True, real_ahead=False), {}),
    'residual': (1, dict(use_graphs=True, block_type='Residual'), {}),
    'mru': (1, dict(use_graphs=True, block_type='MRU'), {}),
    'world2_pix2pix': (2, dict(use_graphs=True), {}),
    'world2_pix2pix_inline': (2, dict(use_graphs=True, overlap_real=False), {}),
    'background': (1, None, {}),        # BGTrainer: run_background, BACKGROUND
    'background_inline': (1, None, {'SSC_BG_OVERLAP_REAL': '0'}),
    'background_eager': (1, None, {}),
    'background_u8': (1, None, {}),
    'background_cached': (1, None, {}),
}
# name -> (the entry point that is fed, BGTrainer arguments)
BACKGROUND = {
    'background': ('train_step', {}),
    'background_inline': ('train_step', {}),
    'background_eager': ('train_step', dict(use_graphs=False)),
    'background_u8': ('train_step_u8', {}),
    'background_cached': ('train_step_cached', {}),
}


def _sha(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def run(name, rank=0, process_group=None):
    import torch
    from sketchyscenecolorization_amd.synthetic import synthetic_batch
    from sketchyscenecolorization_amd.trainer import GanTrainer
    _, kw, _ = CONFIGS[name]
    tr = GanTrainer(img=IMG, seed=5, max_iter_step=50, process_group=process_group, **kw)
    bd, bg = synthetic_batch(NB, 11 + rank, IMG), synthetic_batch(NB, 21 + rank, IMG)
    out = []
    for it in range(ITERS):
        lg, ld = tr.train_iteration(bd, bg, it, next_batch_d=bd)
        out.append('%s rank %d it %d loss_g %s loss_d %s' % (name, rank, it, float(lg).hex(), float(ld).hex()))
    torch.cuda.synchronize()
    st = tr.store
    for label, t in [('generator.flat', st.generator.flat), ('discriminator.flat', st.discriminator.flat),
                     ('generator.adam_v', st.generator.adam_v), ('discriminator.adam_v', st.discriminator.adam_v)] + \
                    [(n, st[n]) for n in st.names() if n.endswith('/u')]:
        out.append('%s rank %d sha256 %s %s' % (name, rank, _sha(t), label))
    return out


def run_background(name):
    import torch
    from sketchyscenecolorization_amd.bg_colorization import BGTrainer
    feed, kw = BACKGROUND[name]
    tr = BGTrainer(image_size=IMG, max_steps=50, seed=5, **kw)
    g = torch.Generator().manual_seed(31)
    if feed == 'train_step':
        x, y = (torch.rand(NB, IMG, IMG, 3, generator=g) * 2 - 1).cuda(), (torch.rand(NB, IMG, IMG, 3, generator=g) * 2 - 1).cuda()
    elif feed == 'train_step_u8':
        x, y = [torch.randint(0, 256, (NB, IMG, IMG, 3), generator=g, dtype=torch.uint8) for _ in range(2)]
    text = torch.randint(1, 18, (NB, 8), generator=g).numpy()
    labels = torch.randint(0, 3, (NB, IMG, IMG), generator=g, dtype=torch.int32).cuda()
    if feed == 'train_step_cached':     # the eight synthetic scenes of the command line, as tests/test_gpu_bg_scene_cache.py caches them
        import contextlib
        import bg_colorization_main as bgcli
        from sketchyscenecolorization_amd.scene_cache import SceneCache
        with contextlib.redirect_stdout(sys.stderr):
            scenes = bgcli.Scenes({'image_size': IMG, 'text_len': 8, 'data_base_dir': 'no_such_dir', 'mode': 'train', 'vocab_size': 18})
        cache = SceneCache(scenes, device='cuda')
        draws = torch.randint(0, len(cache), (4, NB), generator=g).tolist()
        paint = torch.randint(0, 256, (NB, 8), generator=g, dtype=torch.uint8).numpy()
        paint[:, 0], paint[:, 7] = 1, 0     # {enable, sky rgb, ground rgb, 0} per sample: the record of the second step
    out = []
    for it in range(4):
        if feed == 'train_step':
            tr.train_step(x, y, text, labels)
        elif feed == 'train_step_u8':
            tr.train_step_u8(x, y, text, labels)
        else:
            tr.train_step_cached(cache, cache.slots[draws[it]], paint if it == 1 else None, cache.tokens[draws[it]])
        out.append('%s rank 0 it %d losses %s' % (name, it, ' '.join(float(v).hex() for v in tr.losses.cpu())))
    torch.cuda.synchronize()
    st = tr.store
    for label, t in [('generator.flat', st.generator.flat), ('discriminator.flat', st.discriminator.flat),
                     ('generator.adam_v', st.generator.adam_v), ('discriminator.adam_v', st.discriminator.adam_v),
                     ('generator.adam_m', st.generator.adam_m), ('discriminator.adam_m', st.discriminator.adam_m)]:
        out.append('%s rank 0 sha256 %s %s' % (name, _sha(t), label))
    return out


def _rank(rank, name, port, out_dir):
    import torch
    import torch.distributed as dist
    os.environ['MASTER_ADDR'], os.environ['MASTER_PORT'] = '127.0.0.1', str(port)
    dist.init_process_group('gloo', rank=rank, world_size=CONFIGS[name][0])
    torch.cuda.set_device(0)
    lines = run(name, rank, dist.group.WORLD)
    with open(os.path.join(out_dir, 'rank%d.txt' % rank), 'w') as fh:
        fh.write('\n'.join(lines) + '\n')
    dist.barrier()
    dist.destroy_process_group()


def one(name):
    world, _, env = CONFIGS[name]
    os.environ.update(env)
    if world == 1:
        print('\n'.join(run(name) if CONFIGS[name][1] is not None else run_background(name)), flush=True)
        return
    # two gloo ranks on one device (RCCL refuses two ranks on one device), spawned as tests/two_rank_gloo_gpu_check.py does
    import tempfile
    import torch.multiprocessing as mp
    os.environ['SSC_DIST_ONE_DEVICE'] = '1'
    with socket.socket() as sock:
        sock.bind(('127.0.0.1', 0))
        port = sock.getsockname()[1]
    with tempfile.TemporaryDirectory() as tmp:
        mp.spawn(_rank, args=(name, port, tmp), nprocs=world, join=True)
        for r in range(world):
            with open(os.path.join(tmp, 'rank%d.txt' % r)) as fh:
                print(fh.read(), end='', flush=True)


def every(names, at_a_time=3):
    """Each configuration in a child process, at most ``at_a_time`` at once; output in the order of ``names``."""
    failed = []
    for i in range(0, len(names), at_a_time):
        group = [(n, subprocess.Popen([sys.executable, os.path.abspath(__file__), '--config', n], stdout=subprocess.PIPE,
                                      universal_newlines=True)) for n in names[i:i + at_a_time]]
        for n, p in group:
            text, _ = p.communicate()
            print(text, end='', flush=True)
            if p.returncode != 0:
                failed.append((n, p.returncode))
        if failed:      # nothing further is started after a failure
            break
    if failed:
        raise SystemExit('failed: %r' % failed)


if __name__ == '__main__':
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--config', choices=sorted(CONFIGS))
    ap.add_argument('--world', type=int, choices=[1, 2], help='only the configurations of that many ranks')
    ap.add_argument('--list', action='store_true')
    args = ap.parse_args()
    names = [n for n, c in CONFIGS.items() if args.world in (None, c[0])]
    if args.list:
        print('\n'.join(names))
    elif args.config:
        one(args.config)
    else:
        every(names)
