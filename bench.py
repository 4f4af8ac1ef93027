#!/usr/bin/env python
"""Headline benchmark: train images/sec of the Foreground_Instance_Colorization GAN step
(192x192, generator + PatchGAN discriminator, forward + backward + TF-Adam), Pix2Pix variant,
batch 32 per GPU (BASELINE.json configs[2]; with --gpus N it is configs[3], weak scaling).

One "step" = one D-step + one G-step on two independent resident batches, exactly the work of
one iteration of main_procedure.train (reference main_procedure.py:178-232).

Prints ONE JSON line on rank 0 (contract in the task statement).  A plain run sets up, warms up, times
--steps steps and prints the headline (`metric`, `value`, `unit`, `ms_per_step`, ...).  --full adds what
takes runs of its own:
  roofline     : the dominant implicit-GEMM kernel's algorithmic TFLOP/s from HIP events, vs the
                 157.3 TFLOP/s fp32 MFMA peak of MI355X
  cpu_baseline : the torch-CPU fp32 oracle (a port of the reference arithmetic; TensorFlow is not
                 installable here) timed on this host's cores on a bounded sample
  generator_fwd_bwd, the exact-fp32 step and the secondary workloads (see main()).
--dump-outputs DIR writes what the last timed step computed as DIR/<name>.npy (see dump_outputs()).
"""
import argparse
import json
import os

os.environ.setdefault('HIP_FORCE_DEV_KERNARG', '1')     # kernel arguments in device memory (measured: 1570 vs 1540 images/s with 0)
os.environ.setdefault('SSC_KEEP_GRAPHS', '1')           # captured graphs stay readable: kernel launches per step are counted from them
import sys
import time

import torch

T_START = time.time()
# Optional sections of a --full run (larger-batch generator graphs, the exact-fp32 step, the secondary workloads) start only
# while the run is younger than this: on a box where every fresh process takes a minute to page in, the headline line still
# arrives within minutes.  What was skipped is named in the line (`skipped_for_time`).
TIME_BUDGET_S = float(os.environ.get('SSC_BENCH_TIME_BUDGET_S', '420'))
PHASES = {}                 # phase -> wall seconds (reported as `phase_wall_s`)
SKIPPED = []


def _phase(name, t0):
    PHASES[name] = round(PHASES.get(name, 0.0) + time.time() - t0, 2)


def _in_budget(what):
    if time.time() - T_START <= TIME_BUDGET_S:
        return True
    SKIPPED.append(what)
    return False

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

PEAK_FP32_MFMA_TFLOPS = 157.3      # MI355X_MICROARCH.md: v_mfma_f32_32x32x2_f32, dense
PEAK_BF16_MFMA_TFLOPS = 2500.0     # v_mfma_f32_32x32x16_bf16, dense: six bf16 products per fp32 product -> 416.7 fp32-equivalent


def _dtype_label():
    """What the contractions compute in: fp32 values, fp32 accumulation; by default the layers whose channel counts allow it run
    as a 3-way bf16 split of both operands on the bf16 matrix pipe (six products per fp32 product, igemm_bf16.hip)."""
    if os.environ.get('SSC_ARITH', 'bf16x6').lower() in ('fp32', 'f32', 'float32'):
        return 'fp32'
    return 'fp32 (bf16x6 split on the bf16 MFMA, fp32 accumulate; filter gradients and few-channel layers on the exact-fp32 MFMA)'

F_G, F_D = 10.84e9, 3.55e9         # forward FLOPs per image as written in the reference


def cpu_baseline(img, n=4):
    """Reference arithmetic on the host CPU: one D-step + one G-step of the torch-fp32 oracle, (i) on all host cores
    and (ii) on 4 threads, the reference's own intra_op = inter_op = 4 (main_procedure.py:149-150)."""
    from oracle import pix2pix as O

    def one(threads, nb):
        torch.set_num_threads(threads)
        torch.manual_seed(0)
        p = O.init_params(0, img=img)
        st = O.TrainState(p)
        b1, b2 = O.synthetic_batch(nb, seed=1, img=img), O.synthetic_batch(nb, seed=2, img=img)
        t0 = time.time()
        O.d_step(p, st, b1, 1e-4, 0, 100000)
        O.g_step(p, st, b2, 2e-4, 0, 100000)
        return nb / (time.time() - t0), time.time() - t0

    all_cores = torch.get_num_threads()
    by_threads = {}
    for th in sorted(set([4, 16, 64, all_cores])):
        if th > all_cores:
            continue
        one(th, 1)                      # untimed: thread pool, primitive caches
        by_threads[th] = one(th, n)
    torch.set_num_threads(all_cores)
    best = max(by_threads, key=lambda th: by_threads[th][0])
    nb = 32                              # the bench batch, ~10-20 s at the best thread count
    v1, dt1 = one(best, nb)
    v2, dt2 = one(best, nb)
    v, dt = 2 * nb / (dt1 + dt2), dt1 + dt2
    torch.set_num_threads(all_cores)
    return {'value': v, 'unit': 'images/sec', 'cores': best, 'kind': 'port',
            'sample': '2 train iterations (D-step + G-step) at batch %d, %dx%d, torch-CPU fp32 oracle '
                      '(oracle/pix2pix.py) on %d threads (the fastest of the thread counts scanned at batch %d), %.1f s'
                      % (nb, img, img, best, n, dt),
            'images_per_sec_by_threads': {str(th): r[0] for th, r in by_threads.items()},
            'host_cores': all_cores}


def _graph_launches(graphs):
    """Kernel nodes over the hipGraphs one step replays (a segmented step is a list of ops)."""
    from sketchyscenecolorization_amd import hip
    tot = 0
    for g in graphs:
        if isinstance(g, list):
            part = [hip.graph_kernel_nodes(op[1]) for op in g if op[0] == 'graph']
        else:
            part = [hip.graph_kernel_nodes(g)]
        if any(v is None for v in part):
            return None
        tot += sum(part)
    return tot


def run_forward_workload(args):
    """Secondary workloads (not the headline metric): generator-only forward passes.
      fg_infer  : BASELINE configs[1], Pix2Pix generator inference, batch 16, 192x192
      fg_resid  : the same for --block_type Residual
      fg_mru    : the same for the default --block_type MRU (configs[1] 'MRU second')
      bg768     : BASELINE configs[4], Background_Colorization 768x768 residual generator, batch 4
      bg768_train: one BG training step (batch 1 as in the reference), generator + residual discriminator."""
    from sketchyscenecolorization_amd import hip
    from sketchyscenecolorization_amd.params import Buffers, ParamStore
    wl = args.workload
    torch.manual_seed(0)
    if wl == 'bg768_train':
        from sketchyscenecolorization_amd.bg_colorization import BGTrainer
        n, img = 1, (args.img if args.img != 192 else 768)      # the reference graph is built for batch 1
        tr = BGTrainer(image_size=img)
        x = torch.rand(n, img, img, 3, device='cuda') * 2 - 1
        y = torch.rand(n, img, img, 3, device='cuda') * 2 - 1
        text = torch.randint(1, 18, (n, 8), dtype=torch.int32).numpy()
        lab = torch.randint(0, 3, (n, img, img), dtype=torch.int32, device='cuda')
        step = lambda: tr.train_step(x, y, text, lab)
        # FLOP figure: generator only (fwd + bwd = 3 x the 439.6 GFLOP forward of SURVEY 8a A13); the discriminator's
        # share is not in SURVEY and is left out, so step_tflops_as_written under-counts this workload
        flop_img, name = 3 * 439.6e9, 'Background_Colorization train step (G + residual D, fwd + bwd + Adam)'
    elif wl == 'bg768':
        from sketchyscenecolorization_amd.residual import ResidualGenerator
        n, img = (args.batch if args.batch != 32 else 4), (args.img if args.img != 192 else 768)
        store = ParamStore('BG', 18, img, 'cuda', 0)
        gen = ResidualGenerator(store, Buffers('cuda'), 'bg')
        x = torch.rand(n, img, img, 3, device='cuda') * 2 - 1
        text = torch.randint(1, 18, (n, 8), dtype=torch.int32).numpy()
        prep = gen.text.prepare(text, 'bg')         # caption tokens on the device: the captured pass holds no H2D copy
        eager = lambda: gen.forward(x, prep, None, 'bg')
        step = eager
        if not args.no_graphs:
            eager()
            torch.cuda.synchronize()
            graph = hip.new_graph()
            with torch.cuda.graph(graph, capture_error_mode='thread_local'):
                eager()
            step = lambda: (graph.replay() if hip.PROFILE is None else eager())
        flop_img, name = 439.6e9, 'Background_Colorization create_residual_generator forward'
    else:
        n, img = (args.batch if args.batch != 32 else 16), args.img
        z = torch.rand(n, 3, img, img, device='cuda') * 2 - 1
        text = torch.randint(1, 58, (n, 15), dtype=torch.int32).numpy()
        nv = torch.randn(n, 256, device='cuda')
        # the inference entry point of build_single_graph (training=False): GanTrainer.generate, NCHW float in / out,
        # hipGraph replay after the first two calls (--no-graphs: every launch issued eagerly)
        from sketchyscenecolorization_amd.trainer import GanTrainer
        bt, flop_img, name = {'fg_mru': ('MRU', 62.6e9, 'Foreground generate_mru forward'),
                              'fg_resid': ('Residual', 21.1e9, 'Foreground generate_residual forward'),
                              'fg_infer': ('Pix2Pix', 10.84e9, 'Foreground generate_pix2pix forward')}[wl]
        tower = GanTrainer(img=img, seed=0, block_type=bt)
        tower.use_graphs_infer = not args.no_graphs
        labels = torch.randint(0, 25, (n,), dtype=torch.int32, device='cuda') if wl == 'fg_mru' else None
        if not args.no_graphs:
            # resident inputs live in the tensors the replayed graph reads (what a serving loop would fill) and the result is
            # read from the graph's output tensor: no per-call device copies inside the timed region; the caption tokens
            # likewise on the device already
            z, nv, labels = tower.infer_buffers(z, nv, labels)
            text = tower.G.text.prepare(text, 'gi') if tower.G.lstm_hybrid else text
        step = lambda: tower.generate(z, text, nv, labels=labels, clone=args.no_graphs)
    for _ in range(max(args.warmup, 1)):
        step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        step()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    if wl == 'bg768_train':
        launches = _graph_launches(list(tr._graphs.values()))
    elif wl == 'bg768':
        launches = None if args.no_graphs else _graph_launches([graph])
    else:
        launches = _graph_launches(list(tower._graphs.values()))
    prof = []
    hip.PROFILE = prof
    step()
    torch.cuda.synchronize()
    hip.PROFILE = None
    hip.check_sk('bench.py ' + wl)
    agg = {}
    for kname, fl, e0, e1, _shape, _nb in prof:
        a = agg.setdefault(kname, [0.0, 0.0, 0])
        a[0] += fl
        a[1] += e0.elapsed_time(e1) * 1e-3
        a[2] += 1
    tot = sum(v[1] for v in agg.values())
    ms = dt / args.steps * 1e3
    out = {'metric': 'generator forward images/sec', 'value': n * args.steps / dt, 'unit': 'images/sec', 'n_gpus': 1,
           'steps': args.steps, 'warmup': args.warmup, 'ms_per_step': ms, 'higher_is_better': True, 'scaling': 'weak',
           'vs_baseline': None, 'dtype': _dtype_label(), 'data': 'synthetic',
           'config': {'workload': '%s, %dx%d, batch %d' % (name, img, img, n),
                      'launch': 'eager' if args.no_graphs else 'hipGraph replay'},
           'launches_per_step': launches,
           'step_tflops_executed': sum(v[0] for v in agg.values()) / (ms * 1e-3) / 1e12,
           'step_frac_of_fp32_peak': sum(v[0] for v in agg.values()) / (ms * 1e-3) / 1e12 / PEAK_FP32_MFMA_TFLOPS,
           'step_tflops_as_written': flop_img * n / (ms * 1e-3) / 1e12,
           'step_frac_of_fp32_peak_as_written': flop_img * n / (ms * 1e-3) / 1e12 / PEAK_FP32_MFMA_TFLOPS,
           'igemm_ms_per_step': tot * 1e3,
           'per_kernel': {k: {'tflops': v[0] / v[1] / 1e12, 'ms_per_step': v[1] * 1e3, 'launches_per_step': v[2]}
                          for k, v in sorted(agg.items(), key=lambda kv: -kv[1][1])}}
    print(json.dumps(out))


# A run that writes its outputs preheats a fixed number of steps instead of a wall time: every step updates the model, so the
# outputs of the last timed step depend only on the arguments (75 steps per second, about the headline step's rate).
DUMP_PREHEAT_STEPS_PER_S = 75
DUMP_SAMPLE = 1 << 22       # at most this many elements per output array (16 MB in float32): a fixed, seeded sample beyond it


def _sample(t, seed):
    """``t`` flattened when it has at most DUMP_SAMPLE elements, else the elements at DUMP_SAMPLE sorted indices drawn with
    ``seed`` (the same indices for the same size in every run)."""
    import numpy as np
    a = t.detach().reshape(-1)
    if a.numel() <= DUMP_SAMPLE:
        return a.cpu().numpy()
    idx = np.sort(np.random.RandomState(seed).choice(a.numel(), DUMP_SAMPLE, replace=False))
    return a[torch.from_numpy(idx).to(a.device)].cpu().numpy()


def dump_outputs(tr, directory):
    """What the last timed train step computed, as a caller of GanTrainer.train_iteration receives it: the two losses it
    returns, the generator output of its G-step and the variables it updated (float32; losses float64).  Arrays above
    DUMP_SAMPLE elements are written as a fixed, seeded sample of their flattened values (`*_sample`): about 42 MB in all
    at batch 32, 192x192."""
    import numpy as np
    torch.cuda.synchronize()
    loss_g, loss_d = tr.loss.detach().cpu().numpy().astype(np.float64)
    fake = tr.G.output_nchw(tr.last['gctx'])            # [N, 3, H, W] of the last G-step (its buffers are the graph's)
    s = tr.store
    arrays = {'loss_g': np.array([loss_g]), 'loss_d': np.array([loss_d])}
    for name, t, seed in (('generated_images', fake, 1), ('generator_variables', s.generator.flat, 2),
                          ('discriminator_variables', s.discriminator.flat, 3)):
        a = _sample(t, seed).astype(np.float32)
        if a.size == t.numel():
            arrays[name] = a.reshape(t.shape)
        else:
            arrays[name + '_sample'] = a
    if s.nontrainable:
        arrays['spectral_norm_u'] = np.concatenate([v.detach().reshape(-1).cpu().numpy() for v in s.nontrainable.values()])
    os.makedirs(directory, exist_ok=True)
    for name, a in arrays.items():
        np.save(os.path.join(directory, name + '.npy'), np.ascontiguousarray(a))
    return sorted(arrays)


def generator_fwd_bwd(tr, batch, args, iters=30):
    """The quantity BASELINE.json's target is stated on: generator forward + backward alone (no discriminator, no
    optimizer), batch and image size of the train step, one hipGraph of G.forward + G.backward replayed ``iters`` times.
    FLOPs as written in the reference: 3 x F_G per image (forward + data and filter gradients)."""
    import torch
    from sketchyscenecolorization_amd import hip
    N, _, H, W = batch['sketches'].shape
    text = batch['text'] if isinstance(batch['text'], dict) else tr.G.text.prepare(batch['text'], 'gfb')
    out = torch.zeros(N, H, W, 8, device='cuda')
    dpre = torch.randn(N, H, W, 4, device='cuda') * 1e-3
    dpre[..., 3] = 0.0

    def body():
        ctx = tr.G.forward(batch['sketches'], text, batch['noise_vec'], 'gfb', out=out, out_coff=3)
        tr.G.backward(ctx, dpre, side_stream=tr._aux_stream)

    body()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, capture_error_mode='thread_local'):
        body()
    for _ in range(5):
        g.replay()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        g.replay()
    e1.record()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / iters
    tf = 3 * F_G * N / (ms * 1e-3) / 1e12
    # executed: the caption branch's algebraic split does 1.2 instead of 4.53 GFLOP per image
    f_exec = F_G - 4.53e9 + 1.2e9
    tfx = 3 * f_exec * N / (ms * 1e-3) / 1e12
    return {'what': 'generator forward + backward only (hipGraph replay), batch %d, %dx%d' % (N, H, W), 'ms': ms,
            'images_per_sec': N / (ms * 1e-3), 'tflops_as_written': tf, 'frac_of_fp32_mfma_peak': tf / PEAK_FP32_MFMA_TFLOPS,
            'flops_per_image_as_written': 3 * F_G, 'tflops_executed': tfx,
            'frac_of_fp32_mfma_peak_executed': tfx / PEAK_FP32_MFMA_TFLOPS}


def secondary_workloads(args):
    """The other BASELINE.json configurations and block types, each in a process of its own (``python bench.py --workload ...``
    / ``--block-type ...``; a failure there cannot take the headline line down), summarised under ``secondary``:
      fg_infer       configs[1]: Pix2Pix generator inference, batch 16, 192x192
      fg_infer_mru   configs[1] for the reference's default --block_type MRU ('MRU second'), batch 16
      bg768          configs[4]: Background_Colorization 768x768 generator forward, batch 4
      train_mru      configs[2] for the reference's default --block_type MRU, batch 32
      train_residual configs[2] for --block_type Residual, batch 32
      bg768_train    Background_Colorization train step, batch 1, 768x768
    frac_executed / frac_as_written: fraction of the fp32-MFMA peak on the FLOPs the launches execute / on SURVEY's count."""
    import subprocess
    runs = [('fg_infer', ['--workload', 'fg_infer', '--steps', '100', '--warmup', '10']),
            ('fg_infer_mru', ['--workload', 'fg_mru', '--steps', '30', '--warmup', '5']),
            ('bg768', ['--workload', 'bg768', '--steps', '30', '--warmup', '5']),
            ('train_mru', ['--block-type', 'MRU', '--steps', '10', '--warmup', '3', '--preheat-seconds', '1']),
            ('train_residual', ['--block-type', 'Residual', '--steps', '20', '--warmup', '3', '--preheat-seconds', '1']),
            ('bg768_train', ['--workload', 'bg768_train', '--steps', '30', '--warmup', '5'])]
    out = {}
    for name, extra in runs:
        if not _in_budget('secondary.' + name):
            out[name] = {'error': 'skipped: the run was older than SSC_BENCH_TIME_BUDGET_S = %.0f s' % TIME_BUDGET_S}
            continue
        # --full: the train steps' lines carry their executed-FLOP fraction (eager, event-timed steps after the timed ones)
        cmd = [sys.executable, os.path.abspath(__file__), '--full', '--no-cpu-baseline', '--no-secondary'] + extra
        t0 = time.time()
        try:
            r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300, universal_newlines=True)
            line = [l for l in r.stdout.splitlines() if l.startswith('{')]
            if r.returncode != 0 or not line:
                out[name] = {'error': 'rc %d: %s' % (r.returncode, r.stderr[-300:])}
                continue
            j = json.loads(line[-1])
            out[name] = {'workload': j['config']['workload'], 'images_per_sec': j['value'], 'ms': j['ms_per_step'],
                         'frac_executed': j.get('step_frac_of_fp32_peak'),
                         'frac_as_written': j.get('step_frac_of_fp32_peak_as_written'),
                         'steps': j['steps'], 'launch': j['config'].get('launch'),
                         'launches_per_step': j.get('launches_per_step'), 'wall_s': time.time() - t0}
        except Exception as e:     # noqa: BLE001 -- a secondary workload must never cost the headline line
            out[name] = {'error': repr(e)[:300]}
    out['cli_train'] = cli_train_rate(args)
    return out


def cli_train_rate(args):
    """What a user of the reference's command line gets for the headline configuration: ``obj_colorization_main.py --mode train
    -bt Pix2Pix -bs 32`` (its synthetic queue: no dataset on the bench box) in a process of its own, seconds per iteration over
    its last 100 of 300 iterations as the procedure itself prints them.  Not a bench step: the loop dequeues, reads its losses
    (one launch late), logs -- beside ``ms_per_step`` it says what the host side of the drop-in costs."""
    import re
    import subprocess
    import tempfile
    if not _in_budget('secondary.cli_train'):
        return {'error': 'skipped: the run was older than SSC_BENCH_TIME_BUDGET_S = %.0f s' % TIME_BUDGET_S}
    t0 = time.time()
    try:
        with tempfile.TemporaryDirectory() as d:
            cmd = [sys.executable, os.path.join(ROOT, 'obj_colorization_main.py'), '--mode', 'train', '-bt', 'Pix2Pix', '-si', '0',
                   '-bs', str(args.batch), '-mi', '300', '-smf', '100000', '-swf', '100', '-clt', '100']
            r = subprocess.run(cmd, cwd=d, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300, universal_newlines=True)
        ts = [float(m) for m in re.findall(r'Now at iteration \d+\. Elapsed time: ([0-9.]+)s', r.stdout)]
        if r.returncode != 0 or not ts:
            return {'error': 'rc %d: %s' % (r.returncode, r.stderr[-300:])}
        ms = ts[-1] / 100.0 * 1e3
        return {'workload': 'obj_colorization_main.py --mode train -bt Pix2Pix -bs %d (synthetic queue), iterations 200-300' % args.batch,
                'ms': ms, 'images_per_sec': args.batch / (ms * 1e-3), 'wall_s': time.time() - t0}
    except Exception as e:     # noqa: BLE001
        return {'error': repr(e)[:300]}


def arithmetic_error_table():
    """The bf16-split kernels beside the exact-fp32 kernels against float64, live on this GPU: three layer-sized contractions
    (max-abs error; `scale` = max |float64 result|).  The split form keeps the hh products and the correction products in separate
    fp32 accumulators and is the more exact of the two (profiles/NOTEBOOK_r05.md section 2)."""
    import torch
    import torch.nn.functional as F
    from sketchyscenecolorization_amd import hip
    g = torch.Generator(device='cuda').manual_seed(7)
    r = lambda *s: torch.randn(*s, device='cuda', generator=g)
    cases = {}
    a, b = r(1152, 2048), r(2048, 512) * 0.03
    cases['matmul 1152x2048x512'] = (lambda out: hip.matmul(a, b, out), (1152, 512), a.double() @ b.double())
    x, w = r(4, 48, 48, 128), r(4, 4, 128, 256) * 0.03
    cols = F.unfold(F.pad(x.double().permute(0, 3, 1, 2), (1, 1, 1, 1)), 4, stride=2)           # [N, c*16, P], index c*16 + tap
    ref = torch.einsum('nkp,kc->npc', cols, w.double().permute(2, 0, 1, 3).reshape(128 * 16, 256)).reshape(4, 24, 24, 256)
    cases['conv 4x4 s2 128->256 @48^2, batch 4'] = (lambda out: hip.conv_forward(hip.View(x), w, 2, 1, out), (4, 24, 24, 256), ref)
    a2, b2 = r(4608, 4096), r(4096, 512) * 0.02
    cases['matmul 4608x4096x512 (encoder_4)'] = (lambda out: hip.matmul(a2, b2, out), (4608, 512), a2.double() @ b2.double())
    table = {}
    for name, (fn, shape, ref64) in cases.items():
        row = {'scale': float(ref64.abs().max())}
        for mode in ('bf16x6', 'exact_fp32'):
            hip.ARITH_BF16 = mode == 'bf16x6'
            try:
                out = torch.empty(shape, device='cuda')
                fn(out)
                torch.cuda.synchronize()
            finally:
                hip.ARITH_BF16 = True
            row[mode] = float((out.double() - ref64).abs().max())
        table[name] = row
    return table


def exact_fp32_step(args):
    """The same train step with SSC_ARITH=fp32 (every contraction on the exact-fp32 MFMA), in a process of its own."""
    import subprocess
    cmd = [sys.executable, os.path.abspath(__file__), '--no-cpu-baseline', '--no-secondary', '--no-kernel-events', '--no-gen-fb',
           '--steps', '10', '--warmup', '3', '--preheat-seconds', '1']
    try:
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300, universal_newlines=True,
                           env=dict(os.environ, SSC_ARITH='fp32'))
        line = [l for l in r.stdout.splitlines() if l.startswith('{')]
        if r.returncode != 0 or not line:
            return {'error': 'rc %d: %s' % (r.returncode, r.stderr[-300:])}
        j = json.loads(line[-1])
        return {'ms_per_step': j['ms_per_step'], 'images_per_sec': j['value'], 'dtype': j['dtype'], 'steps': j['steps']}
    except Exception as e:     # noqa: BLE001
        return {'error': repr(e)[:300]}


def _free_port():
    import socket
    with socket.socket() as so:
        so.bind(('127.0.0.1', 0))
        return so.getsockname()[1]


def self_launch(args, argv):
    """``python bench.py --gpus N`` outside torchrun: start N ranks (one per GPU) under torch.distributed.run and pass
    their output through; rank 0 prints the one JSON line.  Under torchrun (WORLD_SIZE set) this is a no-op except for
    the consistency check --gpus == WORLD_SIZE (the reference's tower loop, graph_single.py:128-173, is one process per
    GPU here)."""
    import subprocess
    if 'WORLD_SIZE' in os.environ:
        w = int(os.environ['WORLD_SIZE'])
        if w != args.gpus:
            raise SystemExit('bench.py: --gpus %d but the launcher started WORLD_SIZE=%d ranks' % (args.gpus, w))
        return
    if args.gpus == 1 and not args.launcher:
        return
    if not args.stub_cpu and os.environ.get('SSC_BENCH_ONE_DEVICE') != '1':
        n_dev = torch.cuda.device_count()
        if n_dev < args.gpus:
            raise SystemExit('bench.py: --gpus %d but only %d GPU(s) visible' % (args.gpus, n_dev))
    cmd = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node', str(args.gpus),
           '--master-addr', '127.0.0.1', '--master-port', str(_free_port()), os.path.abspath(__file__)] + argv
    env = dict(os.environ)
    env.setdefault('HSA_ENABLE_IPC_MODE_LEGACY', '0')       # dmabuf IPC (RCCL across processes)
    env.setdefault('OMP_NUM_THREADS', '8')
    raise SystemExit(subprocess.call(cmd, env=env))


def _csrc_hash():
    """Hash of the kernel sources + the C-ABI header, as compiled into the library that is RUNNING (hip.lib() has already
    refused a binary whose hash is not the tree's): PMC figures are only attached to a bench line measured on the same kernels
    (profiles/*.json carry the hash of the binary they were collected on)."""
    from sketchyscenecolorization_amd import build, hip
    have, tree = hip.build_hash(), build.tree_hash()
    assert have == tree, (have, tree)
    return have


def run_stub_cpu(args, rank, world):
    """Launcher self-test on CPU (tests/test_bench_launcher.py): the real rank bootstrap, barrier, max-over-ranks
    timing and one JSON line from rank 0, with the GradReducer all-reduce of a flat buffer as the "step" on gloo.
    Not a measurement of anything: the metric name says so."""
    import torch.distributed as dist
    from sketchyscenecolorization_amd.dist_utils import GradReducer
    os.environ.setdefault('MASTER_ADDR', '127.0.0.1')
    os.environ.setdefault('MASTER_PORT', '29500')
    dist.init_process_group('gloo', rank=rank, world_size=world)
    red = GradReducer(dist.group.WORLD)
    flat = torch.full((1 << 16,), float(rank + 1))
    ones = torch.ones(1)
    dist.all_reduce(ones)
    for _ in range(args.warmup):
        red.reduce_async(flat, 0, flat.numel()); red.wait(); flat.mul_(red.grad_scale)
    dist.barrier()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        red.reduce_async(flat, 0, flat.numel()); red.wait(); flat.mul_(red.grad_scale)
    dist.barrier()
    t = torch.tensor([time.perf_counter() - t0], dtype=torch.float64)
    dist.all_reduce(t, op=dist.ReduceOp.MAX)
    dt = float(t)
    if rank == 0:
        print(json.dumps({'metric': 'launcher self-test (CPU stub, no GPU work)', 'value': args.batch * world * args.steps / dt,
                          'unit': 'stub steps*batch/sec', 'n_gpus': world, 'steps': args.steps, 'warmup': args.warmup,
                          'ms_per_step': dt / args.steps * 1e3, 'higher_is_better': True, 'scaling': 'weak',
                          'vs_baseline': None, 'dtype': 'fp32', 'data': 'stub',
                          'config': {'workload': 'launcher self-test', 'global_batch': args.batch * world,
                                     'parallelism': 'dp%d' % world, 'ranks_observed': int(ones.item()),
                                     'backend': 'gloo', 'mean_value': float(flat.mean())}}))
    dist.destroy_process_group()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--workload', default='train', choices=['train', 'fg_infer', 'fg_resid', 'fg_mru', 'bg768', 'bg768_train'],
                    help='train = the headline metric (default); the others are secondary forward-only workloads')
    ap.add_argument('--gpus', type=int, default=1,
                    help='ranks = GPUs of this node; >1 outside torchrun starts the ranks itself (torch.distributed.run)')
    ap.add_argument('--steps', type=int, default=50)
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--batch', type=int, default=32, help='per-GPU batch (reference --batch_size is per GPU)')
    ap.add_argument('--img', type=int, default=192)
    ap.add_argument('--block-type', default='Pix2Pix', choices=['Pix2Pix', 'Residual', 'MRU'],
                    help='train workload: Pix2Pix = the headline metric; Residual (108.8 GFLOP/img-iteration) and MRU (767) '
                         'are secondary')
    ap.add_argument('--full', action='store_true',
                    help='train workload: after the headline also measure what takes runs of its own -- eager event-timed '
                         'steps (roofline, per-kernel figures), the generator forward + backward graph, the arithmetic error '
                         'table, the exact-fp32 step, the secondary workloads and the CPU baseline (each can be left out with '
                         'the --no-* options below)')
    ap.add_argument('--dump-outputs', metavar='DIR', default=None,
                    help='train workload: after the timed steps write what the last one computed as DIR/<name>.npy '
                         '(losses, generator output, updated variables; the untimed preheat then runs a fixed step count)')
    ap.add_argument('--no-cpu-baseline', action='store_true')
    ap.add_argument('--no-secondary', action='store_true',
                    help='skip the secondary workloads (fg_infer, bg768, MRU / Residual train steps, BG train step) that a '
                         '--full single-GPU run times after the headline and reports under "secondary"')
    ap.add_argument('--no-kernel-events', action='store_true')
    ap.add_argument('--no-gen-fb', action='store_true', help='skip the generator forward + backward graph (kernel-trace runs)')
    ap.add_argument('--no-graphs', action='store_true', help='launch every kernel eagerly (no hipGraph replay)')
    ap.add_argument('--preheat-seconds', type=float, default=2.0,
                    help='extra UNTIMED steps after the warmup until this much wall time has passed: the first GPU '
                         'process on a fresh box runs ~7%% slow for about a second (clock ramp / first touch)')
    ap.add_argument('--prof-steps', type=int, default=2, help='eager, HIP-event-instrumented steps for the roofline leg')
    ap.add_argument('--launcher', action='store_true',
                    help='go through the self-launch path (torch.distributed.run) even for --gpus 1')
    ap.add_argument('--stub-cpu', action='store_true', help=argparse.SUPPRESS)     # launcher self-test, no GPU
    args = ap.parse_args()
    self_launch(args, sys.argv[1:])

    rank = int(os.environ.get('RANK', 0))
    local_rank = int(os.environ.get('LOCAL_RANK', 0))
    world = int(os.environ.get('WORLD_SIZE', 1))
    under_launcher = 'WORLD_SIZE' in os.environ
    if args.stub_cpu:
        return run_stub_cpu(args, rank, world)
    if args.dump_outputs and args.workload != 'train':
        raise SystemExit('bench.py: --dump-outputs writes the outputs of the train workload only')
    if args.workload != 'train':
        assert world == 1, 'forward workloads are single-GPU'
        torch.cuda.set_device(0)
        return run_forward_workload(args)
    assert torch.cuda.is_available(), 'bench.py needs MI355X GPUs'
    # SSC_BENCH_ONE_DEVICE=1 (test hook, tests/test_bench_launcher.py): every rank on cuda:0 over gloo -- a REHEARSAL of the N-rank
    # bench on a single-GPU box (RCCL refuses two ranks on one device); the JSON line says so and its value is not a measurement
    rehearsal = under_launcher and os.environ.get('SSC_BENCH_ONE_DEVICE') == '1'
    torch.cuda.set_device(0 if rehearsal else local_rank)
    pg, ranks_observed = None, 1
    if under_launcher:      # one process per GPU; backend "nccl" is RCCL on ROCm.  Also with 1 rank: proves the bootstrap
        import torch.distributed as dist
        os.environ.setdefault('MASTER_ADDR', '127.0.0.1')
        os.environ.setdefault('MASTER_PORT', '29500')
        if rehearsal:
            dist.init_process_group('gloo', rank=rank, world_size=world)
        else:
            dist.init_process_group('nccl', rank=rank, world_size=world, device_id=torch.device('cuda', local_rank))
        pg = dist.group.WORLD if world > 1 else None
        one = torch.ones(1, device='cuda')
        dist.all_reduce(one)                # RCCL rank count as the collective itself sees it
        ranks_observed = int(one.item())
        assert ranks_observed == world == dist.get_world_size(), (ranks_observed, world)

    from sketchyscenecolorization_amd import hip
    from sketchyscenecolorization_amd.synthetic import synthetic_batch
    from sketchyscenecolorization_amd.trainer import GanTrainer

    tr = GanTrainer(img=args.img, seed=0, process_group=pg, use_graphs=not args.no_graphs, block_type=args.block_type)
    assert tr.world == world
    allreduce_plan = tr.allreduce_plan() if world > 1 else None
    # every rank on a GPU of its own (PCI bus ids gathered from all ranks): a launcher that put two ranks on one device would
    # still "scale" on paper
    devices_by_rank = [torch.cuda.get_device_properties(torch.cuda.current_device()).pci_bus_id
                       if hasattr(torch.cuda.get_device_properties(torch.cuda.current_device()), 'pci_bus_id')
                       else torch.cuda.current_device()]
    if under_launcher and world > 1:
        box = [None] * world
        torch.distributed.all_gather_object(box, (devices_by_rank[0], torch.cuda.current_device()))
        devices_by_rank = [b[0] if b[0] is not None else b[1] for b in box]
        if not rehearsal and len(set(box)) != world:
            raise SystemExit('bench.py: %d ranks but only %d distinct devices: %s' % (world, len(set(box)), box))
    bd = synthetic_batch(args.batch, 1234 + rank, args.img)
    bg = synthetic_batch(args.batch, 5678 + rank, args.img)
    if not args.no_graphs:
        # resident inputs live in the buffers the replayed graphs read (what an input pipeline would fill): no per-step copies
        bd, bg = tr.input_buffers('d', bd), tr.input_buffers('g', bg)

    def barrier():
        if world > 1:
            torch.distributed.barrier()
        torch.cuda.synchronize()

    # every iteration also hands over the NEXT iteration's discriminator batch (here: the same resident one), as an input
    # pipeline that is one batch ahead does: its real pass runs inside this iteration's G-step (trainer.real_ahead)
    PHASES['import_and_setup'] = round(time.time() - T_START, 2)       # interpreter start -> trainer built, inputs resident
    _t = time.time()
    for i in range(max(args.warmup, 0 if args.no_graphs else 5)):   # graphs: eager, capture, first replay (of every variant)
        tr.train_iteration(bd, bg, counter=i, next_batch_d=bd)
    barrier()
    _phase('warmup_and_capture', _t)
    preheat_steps = 0
    if args.dump_outputs:           # a fixed count: the model the timed steps start from depends on the arguments alone
        for _ in range(int(round(args.preheat_seconds * DUMP_PREHEAT_STEPS_PER_S / 10.0)) * 10):
            tr.train_iteration(bd, bg, counter=args.warmup, next_batch_d=bd)
            preheat_steps += 1
        barrier()
    t_pre = time.perf_counter()
    while not args.dump_outputs and time.perf_counter() - t_pre < args.preheat_seconds:   # untimed; same step count on every rank
        for _ in range(10):
            tr.train_iteration(bd, bg, counter=args.warmup, next_batch_d=bd)
        preheat_steps += 10
        barrier()
        if world > 1:       # agree on continuing so that no rank leaves the loop alone
            flag = torch.tensor([1.0 if time.perf_counter() - t_pre < args.preheat_seconds else 0.0], device='cuda')
            torch.distributed.all_reduce(flag, op=torch.distributed.ReduceOp.MIN)
            if float(flag) == 0.0:
                break
    # timed region.  With hipGraph replay individual kernels cannot be bracketed by events, so the per-kernel
    # roofline leg (--full) runs `--prof-steps` extra EAGER steps (same kernels, same shapes) right after the timed
    # region; with --no-graphs the events are recorded inside the timed region itself.
    prof = None if (args.no_kernel_events or not args.full) else []
    if args.no_graphs:
        hip.PROFILE = prof
    # one event per step boundary on the launch stream (no host sync inside the region): per-step durations for the median
    marks = [torch.cuda.Event(enable_timing=True) for _ in range(args.steps + 1)]
    barrier()
    t0 = time.perf_counter()
    marks[0].record()
    for i in range(args.steps):
        tr.train_iteration(bd, bg, counter=args.warmup + i, next_batch_d=bd)
        marks[i + 1].record()
    barrier()
    dt = time.perf_counter() - t0
    PHASES['timed_region'] = round(dt, 3)
    step_ms = sorted(marks[i].elapsed_time(marks[i + 1]) for i in range(args.steps))
    dumped = None
    if args.dump_outputs and rank == 0:         # before anything else runs a step
        keep, hip.PROFILE = hip.PROFILE, None
        _t = time.time()
        dumped = dump_outputs(tr, args.dump_outputs)
        _phase('dump_outputs', _t)
        hip.PROFILE = keep
    prof_steps = args.steps
    if not args.no_graphs and prof is not None:
        hip.PROFILE = prof
        for i in range(args.prof_steps):
            tr.train_iteration(bd, bg, counter=args.warmup + args.steps + i, next_batch_d=bd)
        torch.cuda.synchronize()
        prof_steps = args.prof_steps
    hip.PROFILE = None
    loss_g, loss_d = [float(v) for v in tr.loss.tolist()]
    # kernel launches of one iteration: the kernel nodes of the graphs a train_iteration replays (one D-step, one G-step)
    launches_per_step = None if args.no_graphs else _graph_launches(list(tr._graphs.values()))
    hip.check_sk('bench.py timed region')       # a conv launch that stored a partial sum (hand-off timeout) fails the run
    gen_fb = None
    if args.full and args.block_type == 'Pix2Pix' and not args.no_graphs and world == 1 and not args.no_gen_fb:
        _t = time.time()
        gen_fb = generator_fwd_bwd(tr, bg, args)
        _phase('generator_fwd_bwd', _t)
        if args.batch == 32 and not args.no_secondary and _in_budget('generator_fwd_bwd.by_batch'):
            # the same graph at larger batches: BASELINE.json's 70 % target names the generator forward + backward at 192x192
            # without a batch; the train step's batch (32) is the one reported above, these show where the kernels go once a
            # launch holds more tiles per CU (labelled by batch, never merged into the batch-32 figure)
            from sketchyscenecolorization_amd.synthetic import synthetic_batch as _sb
            by_batch = {}
            for nb in (64, 128):
                r = generator_fwd_bwd(tr, _sb(nb, 4321, args.img), args, iters=10)
                by_batch[str(nb)] = {k: r[k] for k in ('ms', 'images_per_sec', 'tflops_executed', 'frac_of_fp32_mfma_peak_executed')}
            gen_fb['by_batch'] = by_batch
            _phase('generator_fwd_bwd_by_batch', _t)
    if world > 1:
        t = torch.tensor([dt], dtype=torch.float64, device='cuda')
        torch.distributed.all_reduce(t, op=torch.distributed.ReduceOp.MAX)
        dt = float(t)

    if rank == 0:
        global_batch = args.batch * world
        ms = dt / args.steps * 1e3
        value = global_batch * args.steps / dt
        f_g, f_d = {'Pix2Pix': (F_G, F_D), 'Residual': (21.1e9, 3.05e9), 'MRU': (62.6e9, 64.6e9)}[args.block_type]
        flops_step = (4 * f_g + 8 * f_d) * args.batch       # per GPU, as-written reference FLOPs
        out = {'metric': 'train images/sec (192x192, gen+disc fwd+bwd)', 'value': value, 'unit': 'images/sec',
               'n_gpus': world, 'steps': args.steps, 'warmup': args.warmup, 'preheat_steps': preheat_steps,
               'ms_per_step': ms, 'launches_per_step': launches_per_step,
               'ms_per_step_median': step_ms[len(step_ms) // 2] if step_ms else None,
               'ms_per_step_min_max': [step_ms[0], step_ms[-1]] if step_ms else None,
               'higher_is_better': True, 'scaling': 'weak', 'vs_baseline': None, 'dtype': _dtype_label(),
               'data': 'synthetic (the same two resident batches every step: loss_d collapses, throughput is unaffected)',
               'config': {'workload': 'Foreground_Instance_Colorization ' + args.block_type + ' GAN train step '
                                      '(D-step + G-step, TF-Adam), %dx%d, batch %d per GPU' % (args.img, args.img,
                                                                                             args.batch),
                          'global_batch': global_batch, 'parallelism': 'dp%d' % world,
                          'ranks_observed_by_allreduce': ranks_observed,
                          'launcher': ('torch.distributed.run, REHEARSAL: all ranks on one GPU over gloo (not a measurement)'
                                       if rehearsal else
                                       'torch.distributed.run, backend nccl (RCCL)' if under_launcher else 'in-process'),
                          'allreduce': allreduce_plan, 'devices_by_rank': devices_by_rank,
                          'block_type': args.block_type, 'loss_g': loss_g, 'loss_d': loss_d,
                          'launch': 'eager' if args.no_graphs else 'hipGraph replay'},
               'step_tflops_as_written': flops_step / (ms * 1e-3) / 1e12,
               'step_frac_of_fp32_peak_as_written': flops_step / (ms * 1e-3) / 1e12 / PEAK_FP32_MFMA_TFLOPS}
        if prof:
            agg = {}
            for name, fl, e0, e1, _shape, nbytes in prof:
                a = agg.setdefault(name, [0.0, 0.0, 0, 0.0])
                a[0] += fl
                a[1] += e0.elapsed_time(e1) * 1e-3
                a[2] += 1
                a[3] += nbytes
            dom = max(agg.items(), key=lambda kv: kv[1][1])
            name, (fl, sec, cnt, nb) = dom
            tot_sec = sum(v[1] for v in agg.values())
            ach = fl / sec / 1e12
            # FLOPs the implicit-GEMM launches of one iteration actually execute (the caption branch's algebraic split
            # does ~1.2 instead of 4.5 GFLOP/img): the figure that bounds time
            exec_flops_step = sum(v[0] for v in agg.values()) / prof_steps
            out['step_tflops_executed'] = exec_flops_step / (ms * 1e-3) / 1e12
            out['step_frac_of_fp32_peak'] = out['step_tflops_executed'] / PEAK_FP32_MFMA_TFLOPS
            traffic = mfma_busy = valu_busy = traffic_note = in_step = None
            tree = _csrc_hash()
            cands = sorted(f for f in os.listdir(os.path.join(ROOT, 'profiles')) if f.endswith('_pmc.json') and f[0] == 'r')
            tpath = os.path.join(ROOT, 'profiles', cands[-1] if cands else 'r03_pmc.json')      # the latest round's passes
            if os.path.exists(tpath) and args.batch == 32 and args.img == 192 and args.block_type == 'Pix2Pix':
                with open(tpath) as f:
                    pm = json.load(f)
                if pm.get('csrc_hash') == tree:
                    tk = pm['kernels'].get(name)
                    if tk:
                        traffic = tk.get('hbm_bytes_per_launch')
                        mfma_busy, valu_busy = tk.get('mfma_busy_frac'), tk.get('valu_busy_frac')
                        if tk.get('in_step_tflops'):
                            # the same kernel inside the replayed step (kernel trace of the graph-replayed bench, same binary):
                            # there its launches share the chip with the step's other chains
                            in_step = {'tflops': tk['in_step_tflops'], 'frac': tk['in_step_tflops'] / PEAK_FP32_MFMA_TFLOPS,
                                       'ms_per_step': tk['in_step_ms_per_step'],
                                       'source': os.path.basename(tpath) + ' (rocprofv3 --kernel-trace of the replayed bench)'}
                else:
                    traffic_note = ('%s was collected on kernel tree %s, this run is %s: not attached'
                                    % (os.path.basename(tpath), pm.get('csrc_hash'), tree))
            out['roofline'] = {'bound': 'mfma', 'kernel': name, 'achieved': ach, 'peak': PEAK_FP32_MFMA_TFLOPS,
                               'unit': 'TFLOP/s', 'frac': ach / PEAK_FP32_MFMA_TFLOPS, 'traffic': traffic,
                               'traffic_unit': 'HBM bytes per launch (FETCH_SIZE x2 + WRITE_SIZE, separate rocprofv3 --pmc '
                                               'passes, profiles/rNN_pmc.json of the latest round; attached only when its csrc_hash matches)',
                               'traffic_note': traffic_note, 'csrc_hash': tree,
                               'algorithmic_bytes_per_launch': nb / cnt,
                               'traffic_ratio': (traffic / (nb / cnt)) if traffic else None,
                               'mfma_busy_frac_pmc': mfma_busy, 'valu_busy_frac_pmc': valu_busy,
                               'achieved_is': 'the dominant kernel alone on the chip (eager launches bracketed by HIP events)',
                               'in_step': in_step,
                               'flop_per_launch': fl / cnt,
                               'launches': cnt, 'avg_launch_ms': sec / cnt * 1e3,
                               'igemm_ms_per_step': tot_sec / prof_steps * 1e3,
                               'events': ('timed region (eager launches)' if args.no_graphs else
                                          '%d eager steps after the hipGraph-replayed timed region' % prof_steps),
                               'all_igemm_tflops': sum(v[0] for v in agg.values()) / tot_sec / 1e12,
                               'executed_flops_per_step': exec_flops_step,
                               'per_kernel': {k: {'tflops': v[0] / v[1] / 1e12, 'ms_per_step': v[1] / prof_steps * 1e3,
                                                  'launches_per_step': v[2] / prof_steps,
                                                  'flop_per_launch': v[0] / v[2],
                                                  'algorithmic_bytes_per_launch': v[3] / v[2]}
                                              for k, v in sorted(agg.items(), key=lambda kv: -kv[1][1])}}
        if args.full:       # everything beyond the headline: runs of its own
            # The quantities BASELINE.json's target is stated on go INSIDE `roofline` (a record of the line may keep that object
            # whole and only the names of other extra keys): the train step's and the generator forward + backward graph's fraction
            # of the fp32-MFMA peak on executed FLOPs at the configured batch, and one line per secondary workload.
            rl = out.setdefault('roofline', {'bound': 'mfma', 'peak': PEAK_FP32_MFMA_TFLOPS, 'unit': 'TFLOP/s'})
            rl['peak_is'] = ('the fp32-MFMA dense peak, as in rounds 1-4: FLOPs are fp32-equivalent (2 x MAC of the fp32 contraction).  The '
                             'bf16x6 kernels run on the bf16 pipe (%.0f TFLOP/s dense = %.1f fp32-equivalent at six products), so a fraction '
                             'above 1.0 of this peak would be legitimate for them' % (PEAK_BF16_MFMA_TFLOPS, PEAK_BF16_MFMA_TFLOPS / 6))
            # ... and beside it the fraction of the pipe the dominant kernel actually runs on: the bf16 MFMA at six products per
            # fp32 product (the issue-bound staging beside the MFMAs, not the matrix pipe, is what bounds these kernels: DESIGN 3.0)
            if 'bf16x6' in str(rl.get('kernel', '')) and rl.get('achieved'):
                rl['peak_bf16x6_fp32_equivalent'] = PEAK_BF16_MFMA_TFLOPS / 6
                rl['frac_of_bf16x6_peak'] = rl['achieved'] / (PEAK_BF16_MFMA_TFLOPS / 6)
            rl['arithmetic'] = out['dtype']
            if world == 1 and not under_launcher:
                _t = time.time()
                try:
                    rl['arithmetic_error_vs_f64'] = arithmetic_error_table()
                except Exception as e:     # noqa: BLE001 -- never cost the headline line
                    rl['arithmetic_error_vs_f64'] = {'error': repr(e)[:200]}
                _phase('arithmetic_error_table', _t)
            tg = rl['targets'] = {'step_frac_of_fp32_peak_executed': out.get('step_frac_of_fp32_peak'),
                                  'step_ms': ms, 'step_images_per_sec': value, 'batch_per_gpu': args.batch}
            if gen_fb is not None:
                out['generator_fwd_bwd'] = gen_fb
                tg['generator_fwd_bwd_frac_executed'] = gen_fb['frac_of_fp32_mfma_peak_executed']
                tg['generator_fwd_bwd_ms'] = gen_fb['ms']
                tg['generator_fwd_bwd_tflops_executed'] = gen_fb['tflops_executed']
                if 'by_batch' in gen_fb:
                    tg['generator_fwd_bwd_frac_executed_by_batch'] = {
                        k: v['frac_of_fp32_mfma_peak_executed'] for k, v in gen_fb['by_batch'].items()}
            if (not args.no_secondary and world == 1 and not under_launcher and args.block_type == 'Pix2Pix' and
                    args.batch == 32 and args.img == 192 and not args.no_graphs):
                del tr
                torch.cuda.empty_cache()
                if _dtype_label() != 'fp32' and _in_budget('exact_fp32_step'):
                    _t = time.time()
                    tg['exact_fp32_step'] = exact_fp32_step(args)       # SSC_ARITH=fp32: the same step on the exact-fp32 MFMA
                    _phase('exact_fp32_step', _t)
                _t = time.time()
                out['secondary'] = secondary_workloads(args)
                _phase('secondary', _t)
                rl['secondary'] = {k: ({'images_per_sec': v['images_per_sec'], 'ms': v['ms'], 'frac_executed': v.get('frac_executed'),
                                        'launches_per_step': v.get('launches_per_step')}
                                       if 'error' not in v else {'error': v['error'][:120]})
                                   for k, v in out['secondary'].items()}
            if not args.no_cpu_baseline and world == 1 and args.block_type == 'Pix2Pix':
                _t = time.time()
                out['cpu_baseline'] = cpu_baseline(args.img)
                _phase('cpu_baseline', _t)
        if dumped is not None:
            out['outputs_dumped'] = {'dir': os.path.abspath(args.dump_outputs), 'arrays': dumped}
        PHASES['total'] = round(time.time() - T_START, 2)
        out['phase_wall_s'] = PHASES
        out['skipped_for_time'] = SKIPPED
        print(json.dumps(out), flush=True)
    if under_launcher:
        torch.distributed.destroy_process_group()


if __name__ == '__main__':
    main()
