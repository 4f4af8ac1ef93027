"""The float64 reference of the forward implicit GEMM (conv_bf_kernel / conv_bfh_kernel of csrc/igemm_bf16.hip), written twice,
and the table of cases tests/test_gpu_fwd_bf16_forms.py runs on the device.

    out[n, py, px][c] = epi( sum over taps (ty, tx) and channels k of  act(a*X + b)[n, py*s + oy + ty, px*s + ox + tx][k] * F[ty, tx][k, c]
                             (+ bias[c]) (+ what out held: accumulate) )

with a tap outside the gathered image contributing nothing and k below the real gathered channels.

  ref_tf    (a) the TF op of oracle/tf_ops.py on double tensors; the data gradients by autograd
  ref_taps  (b) a loop over the taps with shifted slices and einsum; per output element also S = the same sum over |products|
            and K = the number of non-zero products, which the comparison rule (kernel_check.check_dot) makes its bound of.  A
            bias is one more term of ref, S and K, and so is an accumulate base.  The epilogue's activation is applied by
            epilogue(), behind the sum.

tests/test_fwd_oracle.py holds (a) against (b) on every case of the table, without a GPU.

A case describes the launch the way the hip.py wrappers see it:
  kind  'conv'          gathered x [n, h, w, *], filter [k, k, real, co]; stride, pad (an int: tf.pad + VALID; 'same': TF SAME);
                        nk: the launch reads a transposed copy [k, k, co, real] (conv_forward(w_nk=...))
        'deconv'        gathered x [n, h, w, *], filter [4, 4, co, real] -> [n, 2h, 2w, co]: nphase 4, the [n][k] orientation
        'conv_dgrad'    gathered dy [n, h, w, *], filter [k, k, ci, real] -> dx [.., nn] of input channels [n_off, n_off + nn):
                        stride 1 with flipped taps, stride 2 (k = 4, pad 1) with nphase 4
        'deconv_dgrad'  gathered dy [n, h, w, *] (h, w even), filter [4, 4, real, ci] -> dx [n, h/2, w/2, nn]
        'matmul'        gathered a [w rows, *] (n = h = 1), b [real, co]
        'matmul_nt'     the same with b [co, real]
  src   (C0, C1, real): stored channels of the two sources and how many of C0 + C1 are real; the others are padding lanes
  tf    (norm0, act, norm1, act1): folded norm on source 0 / 1, activation of source 0, of source 1 (-1: the same)
  co    output channels Nn of a forward op; ci / n_off / nn: the filter's input channels and the sub-range of a data gradient
  nstore, ldc, coff: stored columns (>= Nn, the rest zeros), row pitch of the output tensor, first column
  probe 'onehot': one non-zero gathered channel per pixel (K = 1 per tap); 'channel': one non-zero channel in the whole tensor
  bn, bnbwd: riders a case of the second table carries on a second launch (see STREAM_CASES)

A second table, STREAM_CASES, holds the cases of the seven streaming kernels ssc_conv_forward dispatches before the tiled ones
(csrc/fewchan.hip, pw1x1.hip, c3x3.hip, s2n16.hip, tr4tiny.hip, fewchan7.hip, tr4n16.hip), which
tests/test_gpu_fwd_stream_forms.py runs; the same two references serve it.
"""
import torch

from oracle import tf_ops as T

PAD_LANE = 1.0e3        # what padding channels and everything around a tensor hold: the kernel may not rely on zeros there
NAN = float('nan')
PLAIN = (False, 0, False, -1)
LRELU = (False, 2, False, -1)
NORM_LRELU = (True, 2, False, -1)
NORM_RELU = (True, 1, False, -1)
TWO_T = (True, 2, True, 1)          # two sources: norm + lrelu, norm + relu
TWO_A = (False, 2, False, 1)        # two sources, activations only (keeps zeros: the probes)

DEFAULTS = dict(k=1, stride=1, pad=0, tf=PLAIN, co=None, ci=None, n_off=0, nn=None, bias=False, epi=0, acc=False, nstore=None,
                ldc=None, coff=0, nk=False, lane=PAD_LANE, probe=None, seed=None, bn=False, bnbwd=0)


def _case(name, kind, n, h, w, src, **kw):
    c = dict(DEFAULTS, name=name, kind=kind, n=n, h=h, w=w, src=src)
    expect = {k: kw.pop(k) for k in list(kw) if k not in DEFAULTS}
    c.update(kw)
    c['expect'] = dict(dict(tile=4), **expect)
    return c


# expect: what ssc_conv_bf_plan must report on the MI355X (256 CUs) in the parent process, where no switch is set: tile (0 128x128,
# 1 64x128, 2 128x64, 4 64x64; the planner takes 64x64 for every launch this small, so 4 unless the case says otherwise), korder
# and grid layout (0 3-D grid, 1 XCD order, 2 XCD order with the phases adjacent, 3 whole tiles + K slices, 4 split-K slabs: the
# planner cuts K into slabs wherever a few tiles meet nine or more K-tiles); with layout 4 the number of slabs, with layout 3 the
# whole tiles and the K slices of every other tile
# --- the carriers: a 3x3 SAME conv over 2 x 9 x 7 pixels (M = 126: below one 128-row tile, no multiple of 64) with every source
# form; tests run each plain and transformed, under every pinned tile, and with one LDS stage (CO_RUN)
CARRIER_SRC = dict(two=(64, 32, 96), one=(64, 0, 64), km=(68, 0, 66))
CARRIER_TF = dict(two=TWO_T, one=NORM_LRELU, km=NORM_LRELU)
CARRIER_FORMS = [(s, p) for s in ('two', 'one', 'km') for p in 'PT']
CARRIER_SLABS = dict(two=6, one=4, km=6)     # of their 27 / 18 / 27 K-tiles on the 64x64 tile


def carrier(src, p):
    """The carrier case with source form `src` ('two', 'one', 'km'), plain ('P') or transformed ('T')."""
    return _case('carrier_%s_%s' % (src, p), 'conv', 2, 9, 7, CARRIER_SRC[src], co=128, k=3, pad='same', nstore=132, ldc=140, coff=4,
                 tf=CARRIER_TF[src] if p == 'T' else PLAIN, bias=(p == 'T'), seed=7000 + CARRIER_FORMS.index((src, p)),
                 korder=1, layout=4, slabs=CARRIER_SLABS[src])


def probe(kind, src, p):
    """A probe with power against a lost plane, source form `src`, plain ('P') or activated on load ('T': no norm, zeros stay
    zeros).  kind 'onehot': a 1x1 conv whose gathered tensor has one non-zero channel per pixel (K = 1: every output is ONE
    product); 'channel': a 3x3 SAME conv over a tensor with one non-zero channel in all (K <= 9, through the tap walk)."""
    tf = PLAIN if p == 'P' else (TWO_A if src == 'two' else LRELU)
    i = 2 * ('two', 'one', 'km').index(src) + 'PT'.index(p)
    if kind == 'onehot':
        return _case('probe_onehot_%s_%s' % (src, p), 'conv', 2, 9, 7, CARRIER_SRC[src], co=132, tf=tf, probe='onehot', seed=7100 + i,
                     korder=0, layout=0)
    return _case('probe_channel_%s_%s' % (src, p), 'conv', 2, 9, 7, CARRIER_SRC[src], co=132, k=3, pad='same', tf=tf, probe='channel',
                 seed=7200 + i, korder=1, layout=4, slabs=CARRIER_SLABS[src])


PROBE_FORMS = [(kind, s, p) for kind in ('onehot', 'channel') for s, p in CARRIER_FORMS]

CASES = [
    # --- geometry: odd and non-square sizes, PW = 1, PH * PW = 1, SAME with asymmetric padding, taps off every edge
    _case('g_4x4s2_odd', 'conv', 4, 11, 9, (64, 0, 64), co=68, k=4, stride=2, pad=1, tf=NORM_LRELU, korder=2, layout=4, slabs=8),       # M = 80
    _case('g_4x4s2_same_asym', 'conv', 3, 11, 9, (32, 32, 64), co=68, k=4, stride=2, pad='same', tf=TWO_T, bias=True, epi=2,
          korder=2, layout=4, slabs=8),                                                                                  # SAME over odd sizes: pad 1 before, 2 after
    _case('g_4x4s1_same_asym', 'conv', 2, 9, 5, (64, 0, 64), co=36, k=4, pad='same', korder=1, layout=4, slabs=8),      # pad 1 before, 2 after
    _case('g_3x3_column', 'conv', 2, 70, 1, (32, 0, 32), co=64, k=3, pad=1, tf=LRELU, epi=1, korder=1, layout=0),  # PW = 1
    _case('g_fc', 'conv', 130, 1, 1, (64, 0, 64), co=132, bias=True, epi=1, korder=0, layout=1),               # PH * PW = 1
    _case('g_5x5_taps_off_every_edge', 'conv', 6, 3, 4, (32, 0, 32), co=68, k=5, pad=2, korder=1, layout=4, slabs=5),   # the window wider than the image
    _case('g_nk_3x3', 'conv', 2, 9, 7, (64, 0, 64), co=68, k=3, pad=1, nk=True, bias=True, korder=1, layout=4, slabs=4),       # [n][k] filter
    _case('g_nk_1x1_two', 'conv', 2, 9, 7, (32, 64, 96), co=130, nk=True, tf=TWO_T, korder=0, layout=0),
    # --- the partly empty last chunk (KM): k_real one to three below C0; garbage and NaN in the padding lanes
    _case('km_36_35', 'conv', 2, 9, 7, (36, 0, 35), co=64, k=3, pad='same', bias=True, epi=2, korder=1, layout=0),
    _case('km_68_65_norm', 'conv', 2, 9, 7, (68, 0, 65), co=68, k=3, pad='same', tf=NORM_LRELU, korder=1, layout=4, slabs=6),
    _case('km_132_130_nan_lanes', 'conv', 2, 9, 7, (132, 0, 130), co=130, k=3, pad='same', lane=NAN, nstore=132, korder=1, layout=4, slabs=8),
    _case('km_260_259_1x1', 'conv', 2, 9, 7, (260, 0, 259), co=36, tf=NORM_RELU, korder=0, layout=0),
    _case('km_68_67_4x4s2', 'conv', 3, 12, 10, (68, 0, 67), co=68, k=4, stride=2, pad=1, lane=NAN, tf=LRELU, korder=2, layout=4, slabs=12),
    _case('km_dgrad_36_33', 'conv_dgrad', 2, 9, 7, (36, 0, 33), ci=64, k=3, pad=1, acc=True, korder=1, layout=0),
    _case('km_mm_36', 'matmul', 1, 1, 70, (36, 0, 36), co=68, bias=True, korder=0, layout=0),
    # --- columns: Nstore 36 / 64 / 68 / 130 / 132, Nstore > Nn, ldc > Nstore with coff
    _case('n_36', 'conv', 2, 9, 7, (64, 0, 64), co=36, k=3, pad=1, korder=1, layout=4, slabs=4),
    _case('n_64_of_60', 'conv', 2, 9, 7, (64, 0, 64), co=60, nstore=64, k=3, pad=1, bias=True, korder=1, layout=4, slabs=4),
    _case('n_68_coff', 'conv', 2, 9, 7, (32, 0, 32), co=64, nstore=68, ldc=80, coff=8, k=3, pad=1, epi=2, korder=1, layout=0),
    _case('n_130_of_128', 'conv', 2, 9, 7, (32, 0, 32), co=128, nstore=130, ldc=131, k=3, pad=1, korder=1, layout=0),
    _case('n_132_of_129_deconv', 'deconv', 2, 5, 3, (64, 0, 64), co=129, nstore=132, ldc=136, coff=4, tf=NORM_RELU, epi=1,
          korder=1, layout=2),
    # --- the transposed forms: nphase 4, 2x2 taps, kstep -2
    _case('t_deconv_two', 'deconv', 2, 5, 4, (64, 32, 96), co=68, tf=TWO_T, korder=1, layout=4, slabs=3),               # 2 x 5 x 4 = 40 rows x 4 phases
    _case('t_deconv_32_nn132', 'deconv', 2, 5, 4, (32, 0, 32), co=132, korder=1, layout=2),                   # one K-tile per tap: no slabs
    _case('t_deconv_few_tiles', 'deconv', 1, 4, 4, (32, 0, 32), co=36, korder=1, layout=0),                    # 4 tiles: the 3-D grid
    _case('t_dgrad_s2', 'conv_dgrad', 2, 5, 4, (64, 0, 64), ci=68, k=4, stride=2, pad=1, korder=1, layout=2),
    _case('t_dgrad_s2_acc_noff', 'conv_dgrad', 2, 6, 5, (32, 0, 32), ci=132, n_off=64, nn=36, k=4, stride=2, pad=1, acc=True,
          korder=1, layout=0),
    # --- the data gradients: flipped taps, n_off / nn sub-ranges, accumulate
    _case('d_dgrad_3x3', 'conv_dgrad', 2, 9, 7, (64, 0, 64), ci=68, k=3, pad=1, korder=1, layout=4, slabs=4),
    _case('d_dgrad_4x4_same_acc', 'conv_dgrad', 2, 9, 7, (32, 32, 64), ci=130, n_off=32, nn=96, k=4, pad='same', tf=TWO_T, acc=True,
          korder=1, layout=4, slabs=8),
    _case('d_dgrad_1x1', 'conv_dgrad', 2, 9, 7, (64, 0, 64), ci=36, korder=0, layout=0),
    _case('d_deconv_dgrad_noff32', 'deconv_dgrad', 3, 12, 10, (64, 0, 64), ci=132, n_off=32, nn=68, korder=2, layout=4, slabs=8),
    _case('d_deconv_dgrad_noff64_acc', 'deconv_dgrad', 2, 10, 14, (32, 32, 64), ci=132, n_off=64, nn=36, acc=True, korder=2, layout=4, slabs=8),
    # --- the dense forms
    _case('m_mm_norm', 'matmul', 1, 1, 100, (96, 0, 96), co=132, tf=NORM_LRELU, bias=True, acc=True, korder=0, layout=0),
    _case('m_mm_nt', 'matmul_nt', 1, 1, 70, (64, 0, 64), co=68, acc=True, korder=0, layout=0),
    # --- grid layouts: at least 8 tiles in the XCD order; split-K slabs (small M, long K); whole tiles + K slices in the launch
    # (the slabs are summed by slab_reduce4_kernel where Nn, Nstore, ldc are multiples of 4 and the pointers 16-byte aligned --
    # l_slabs_4x4 with bias and lrelu, l_slabs_dgrad_acc onto a base, l_slabs_deconv with tanh into strided phases -- and by the scalar
    # slab_reduce_kernel otherwise: l_slabs_mm_130 here, km_132_130_nan_lanes and n_130_of_128 above)
    _case('l_xcd_3x3', 'conv', 2, 21, 19, (32, 0, 32), co=68, k=3, pad=1, korder=1, layout=1),                 # 798 rows
    _case('l_xcd_4x4s2_nk', 'conv', 2, 42, 38, (32, 0, 32), co=68, k=4, stride=2, pad=1, nk=True, korder=2, layout=4, slabs=4),
    _case('l_xcd_1x1_acc', 'conv', 2, 21, 19, (64, 0, 64), co=132, acc=True, korder=0, layout=1),
    _case('l_slabs_4x4', 'conv', 2, 6, 6, (512, 0, 512), co=68, k=4, pad='same', tf=NORM_LRELU, bias=True, epi=2, korder=1, layout=4, slabs=16),
    _case('l_slabs_4x4s2', 'conv', 2, 12, 12, (256, 256, 512), co=36, k=4, stride=2, pad=1, korder=2, layout=4, slabs=16),
    _case('l_slabs_mm_130', 'matmul_nt', 1, 1, 70, (2048, 0, 2048), co=130, korder=0, layout=4, slabs=16),
    _case('l_slabs_dgrad_acc', 'conv_dgrad', 2, 6, 6, (512, 0, 512), ci=68, k=4, pad='same', acc=True, korder=1, layout=4, slabs=16),
    _case('l_slabs_deconv', 'deconv', 2, 3, 3, (512, 0, 512), co=68, epi=1, korder=1, layout=4, slabs=16),
    _case('l_slices_3x3', 'conv', 2, 96, 96, (32, 0, 32), co=128, k=3, pad='same', tf=LRELU, korder=1, layout=3, whole=512, slices=2),      # 288 tiles of 64x128
    # --- the 128 x 128 tile on 16-k stages where the planner takes it by itself: at least 256 such tiles
    _case('h_1x1_big', 'conv', 2, 128, 128, (32, 0, 32), co=128, nstore=130, ldc=132, tf=NORM_LRELU, bias=True, tile=0, korder=0, layout=1),
]
for _i, _c in enumerate(CASES):
    _c['seed'] = 6000 + _i          # every case a fixed seed of its own
BY_NAME = {c['name']: c for c in CASES}
assert len(BY_NAME) == len(CASES)


def all_cases():
    return CASES + [carrier(*f) for f in CARRIER_FORMS] + [probe(*f) for f in PROBE_FORMS]


# --- the streaming kernels ssc_conv_forward dispatches before the tiled ones (tests/test_gpu_fwd_stream_forms.py): the smallest
# shapes that still reach each form.  expect: kernel, the name ssc_conv_forward_kernel_name must give; inst, the instantiation
# ssc_conv_stream_plan must report (None: none of the seven takes the launch, the query answers -10); walk, whether some
# persistent workgroup takes two tiles or more on the MI355X's 256 CUs (tiles > workgroups in the query's words).
# bn: a second launch carries the batch-statistics rider (conv_forward / deconv_forward(bn=...)); bnbwd: a second launch of the
# data gradient carries the norm-backward sums for a consumer with that activation (conv_dgrad(bnbwd=...)).
def _s(name, kind, n, h, w, src, kernel, inst, walk=False, **kw):
    return _case(name, kind, n, h, w, src, kernel=kernel, inst=inst, walk=walk, **kw)


def _pw(name, K, co, tf, shape=(2, 33, 35), **kw):      # M = 2310: 37 row tiles of 64, the last with 6 rows
    inst = 2 * (16, 32, 64, 128).index(K) + int(co <= 64)
    return _s(name, 'conv', shape[0], shape[1], shape[2], (K, 0, K), 'conv_pw1x1', inst, co=co, tf=tf, **kw)


def _c3(name, shape, C, co, inst, tf, kind='conv', **kw):
    orient = 'NK' if (kind == 'conv_dgrad' or kw.get('nk')) else 'KN'
    geo = dict(pad=1) if kind == 'conv_dgrad' else dict(pad='same', co=co)
    return _s(name, kind, shape[0], shape[1], shape[2], (C, 0, C), 'conv_c3x3<%s>' % orient, inst, k=3, tf=tf, **dict(geo, **kw))


def _s2(name, co, tf, stride=2, **kw):
    # stride 2: lattice (9, 63, 66), 1440 tiles of 2 x 16; stride 1 (4x4 SAME): (3, 101, 119), 624 tiles of 4 x 16; 512 walkers
    n, h, w = (9, 126, 132) if stride == 2 else (3, 101, 119)
    return _s(name, 'conv', n, h, w, (64, 0, 64), 'conv_s2n16', 0 if stride == 2 else 1, walk=True, co=co, k=4, stride=stride,
              pad=1 if stride == 2 else 'same', tf=tf, **kw)


def _t16(name, src, co, tf, **kw):      # lattice (4, 61, 70): 620 tiles of 2 x 16 per phase on 128 walkers
    return _s(name, 'deconv', 4, 61, 70, src, 'deconv_tr4n16', 0, walk=True, co=co, tf=tf, **kw)


def _f7(name, shape, ci, co, **kw):
    return _s(name, 'conv', shape[0], shape[1], shape[2], (4, 0, ci), 'conv_fewchan7', 0, co=co, k=7, stride=2, pad='same', **kw)


def _fc(name, shape, src, co, **kw):
    return _s(name, 'conv', shape[0], shape[1], shape[2], src, 'conv_fewchan<%d>' % src[0], int(src[0] == 8), co=co, k=4, stride=2,
              pad=1, **kw)


def _tt(name, shape, ci, co, tf=PLAIN, **kw):
    return _s(name, 'deconv', shape[0], shape[1], shape[2], (4, 0, ci), 'deconv_tr4_tiny', 0, co=co, nstore=4, tf=tf, **kw)


STREAM_CASES = [
    # --- pw1x1: all eight pw1x1_kernel<K, NARROW>; 96 and 160 outputs (a partly filled column block / column group); columns
    # inside a wider row; the four source forms; walkers with two tiles (1055 row tiles on 1024 walkers, 149 on 128)
    _pw('pw_k16_n64', 16, 64, PLAIN),
    _pw('pw_k16_n96', 16, 96, LRELU),
    _pw('pw_k32_n64', 32, 64, NORM_RELU),
    _pw('pw_k32_n128_coff', 32, 128, NORM_LRELU, coff=4, ldc=136),
    _pw('pw_k32_n160', 32, 160, LRELU),
    _pw('pw_k64_n64', 64, 64, NORM_LRELU),
    _pw('pw_k64_n256', 64, 256, PLAIN),
    _pw('pw_k128_n64', 128, 64, LRELU),
    _pw('pw_k128_n512', 128, 512, NORM_RELU),
    _pw('pw_walk_k16_n64', 16, 64, NORM_LRELU, shape=(3, 149, 151), walk=True, bn=True),
    _pw('pw_walk_k128_n512', 128, 512, NORM_RELU, shape=(2, 67, 71), walk=True, bn=True),
    _pw('pw_probe_onehot', 64, 256, LRELU, probe='onehot'),
    # --- c3x3: c3x3n16_kernel (16 -> <= 16 on the 4 x 32 tile), c3x3_kernel<16, 16>, <32, 32>, <32, 16> (the 8 x 16 tile where it wastes
    # fewer pixels); once each at 17296 / 22500 pixels and once with tiles > walkers (768 at 16 channels, 512 at 32); KN, NK and
    # the flipped NK of the data gradient with n_off > 0 and nn < ci
    _c3('c3_n16_nn16', (2, 90, 125), 16, 16, 0, NORM_RELU),
    _c3('c3_n16_nn12_coff', (2, 90, 125), 16, 12, 0, LRELU, coff=4, ldc=20),
    _c3('c3_n16_nn4', (2, 90, 125), 16, 4, 0, PLAIN),
    _c3('c3_16x16_nk', (8, 47, 46), 16, 16, 1, NORM_LRELU, nk=True),
    _c3('c3_32x32', (2, 90, 125), 32, 32, 2, LRELU),
    _c3('c3_32x16_nk', (8, 47, 46), 32, 32, 3, NORM_RELU, nk=True),
    _c3('c3_32x32_dgrad_noff', (2, 90, 125), 32, None, 2, PLAIN, kind='conv_dgrad', ci=40, n_off=8, nn=20),
    _c3('c3_walk_n16', (17, 61, 90), 16, 16, 0, NORM_LRELU, walk=True, bn=True),                 # 816 tiles
    _c3('c3_walk_16x16', (43, 47, 46), 16, 16, 1, NORM_RELU, walk=True, bn=True),                # 774
    _c3('c3_walk_32x32', (12, 61, 90), 32, 32, 2, NORM_RELU, walk=True, bn=True),                # 576
    _c3('c3_walk_32x16', (29, 47, 46), 32, 32, 3, LRELU, walk=True, bn=True),                    # 522
    _c3('c3_walk_n16_dgrad_noff', (17, 61, 90), 16, None, 0, PLAIN, kind='conv_dgrad', ci=24, n_off=4, nn=16, walk=True, bnbwd=2),
    _c3('c3_probe_channel', (2, 90, 125), 16, 16, 0, LRELU, probe='channel'),
    # 16 channels to more than 16: c3x3_kernel<16, *> stages 16 filter columns only, so the predicate refuses them and the
    # exact-fp32 tiled kernel runs (at most 32 stored columns: the 128 x 32 tile, no bf16 form)
    _s('c3_16_to_20', 'conv', 2, 90, 125, (16, 0, 16), 'conv_fwd<128x32,KN>', None, co=20, k=3, pad='same', tf=NORM_LRELU),
    _s('c3_16_to_32', 'conv', 2, 90, 125, (16, 0, 16), 'conv_fwd<128x32,KN>', None, co=32, k=3, pad='same', tf=NORM_LRELU),
    # --- s2n16: both strides, 16 / 10 / 4 columns, the data gradient of a transposed conv with 24 input channels
    _s2('s2_nn16', 16, NORM_LRELU, bn=True),
    _s2('s2_nn10_coff', 10, LRELU, coff=3, ldc=16),
    _s2('s2_nn4', 4, PLAIN),
    _s2('s2_stride1_nn16', 16, NORM_RELU, stride=1, bn=True),
    _s2('s2_stride1_nn10', 10, PLAIN, stride=1),
    _s('s2_deconv_dgrad_noff', 'deconv_dgrad', 9, 126, 132, (64, 0, 64), 'conv_s2n16', 0, walk=True, ci=24, n_off=8, nn=16),
    _s2('s2_probe_channel', 16, LRELU, probe='channel'),
    # --- tr4n16: two sources with a norm and an activation each, one, 100 + 156; two padding lanes; 16 / 10 / 4 columns
    _t16('t16_two', (128, 128, 256), 16, TWO_T, bn=True),
    _t16('t16_one_nn10', (256, 0, 256), 10, NORM_LRELU),
    _t16('t16_100_156_nn4_coff', (100, 156, 256), 4, TWO_A, coff=4, ldc=12),
    _t16('t16_kreal254', (128, 128, 254), 16, TWO_T),
    _t16('t16_probe_channel', (256, 0, 256), 16, LRELU, probe='channel'),
    # --- fewchan7: one tile, eight, 544 on 512 walkers; 64 / 48 / 33 columns; 1 to 4 filter input channels
    _f7('f7_one_tile_ci2', (1, 8, 64), 2, 64),
    _f7('f7_eight_ci4_nn48', (2, 16, 128), 4, 48),
    _f7('f7_ci1_nn33_coff', (2, 16, 128), 1, 33, coff=2, ldc=40),
    _f7('f7_walk', (17, 128, 128), 3, 64, walk=True, bn=True),
    _f7('f7_probe_channel', (2, 16, 128), 3, 64, probe='channel'),
    # --- fewchan: <4> with 3 real channels, <8> with 6 and 8; 64 and 33 columns, 36 stored over 33; 576 tiles on 512 walkers
    # (<8>), 832 on 768 (<4>)
    _fc('fc4_3', (1, 8, 64), (4, 0, 3), 64),
    _fc('fc8_6_nn33_of_36', (1, 8, 64), (8, 0, 6), 33, nstore=36),
    _fc('fc8_8_coff', (1, 8, 64), (8, 0, 8), 64, coff=4, ldc=72),
    _fc('fc8_walk', (9, 128, 256), (8, 0, 6), 64, walk=True),
    _fc('fc4_walk', (13, 128, 256), (4, 0, 3), 64, walk=True),
    _fc('fc_probe_channel', (2, 16, 128), (8, 0, 6), 64, probe='channel'),
    # --- tr4tiny: 126 pixels in one block and 5883 in 23; 1..4 columns of 4 stored, 1..4 filter input channels, every epilogue
    _tt('tt_one_block', (2, 9, 7), 3, 3),
    _tt('tt_23_blocks_bn', (3, 37, 53), 3, 3, NORM_RELU, bn=True),
    _tt('tt_ci1_co4_tanh', (2, 9, 7), 1, 4, LRELU, epi=1),
    _tt('tt_ci4_co1_lrelu', (3, 37, 53), 4, 1, epi=2),
    _tt('tt_ci2_co2_coff', (2, 9, 7), 2, 2, NORM_LRELU, coff=2, ldc=8),
    _tt('tt_probe_channel', (3, 37, 53), 3, 3, LRELU, probe='channel'),
]
for _i, _c in enumerate(STREAM_CASES):
    _c['seed'] = 8000 + _i
STREAM_BY_NAME = {c['name']: c for c in STREAM_CASES}
assert len(STREAM_BY_NAME) == len(STREAM_CASES)


def lookup(name):
    if name in STREAM_BY_NAME:
        return STREAM_BY_NAME[name]
    for c in all_cases():
        if c['name'] == name:
            return c
    raise KeyError(name)


def geometry(c):
    """Output height / width / channels of a case, the filter's shape as the wrapper takes it, and the taps: a list of
    (ky, kx, in_stride, oy, ox, out_stride, ry, rx): lattice pixel (py, px) of the PH x PW lattice reads the gathered pixel
    (py * in_stride + oy, px * in_stride + ox) through filter tap (ky, kx) and writes (py * out_stride + ry, px * out_stride + rx)."""
    kind, n, h, w, k, s = c['kind'], c['n'], c['h'], c['w'], c['k'], c['stride']
    real = c['src'][2]
    if kind in ('matmul', 'matmul_nt'):
        assert n == 1 and h == 1 and k == 1
        return dict(OH=1, OW=w, PH=1, PW=w, nn=c['co'], fshape=(real, c['co']) if kind == 'matmul' else (c['co'], real),
                    taps=[(0, 0, 1, 0, 0, 1, 0, 0)])
    if kind == 'conv':
        if c['pad'] == 'same':
            py, px = T.same_pads(h, k, s)[0], T.same_pads(w, k, s)[0]
            PH, PW = -(-h // s), -(-w // s)
        else:
            py = px = c['pad']
            PH, PW = (h + 2 * py - k) // s + 1, (w + 2 * px - k) // s + 1
        return dict(OH=PH, OW=PW, PH=PH, PW=PW, nn=c['co'], fshape=(k, k, real, c['co']),
                    taps=[(ky, kx, s, ky - py, kx - px, 1, 0, 0) for ky in range(k) for kx in range(k)])
    if kind == 'deconv' or (kind == 'conv_dgrad' and s == 2):
        # out[2q + r] takes x[q + (r + 1 - ky) / 2] through tap ky where r + 1 - ky is even (o = 2i - 1 + k)
        taps = [(ky, kx, 1, ((ky + 1) % 2 + 1 - ky) // 2, ((kx + 1) % 2 + 1 - kx) // 2, 2, (ky + 1) % 2, (kx + 1) % 2)
                for ky in range(4) for kx in range(4)]
        if kind == 'deconv':
            return dict(OH=2 * h, OW=2 * w, PH=h, PW=w, nn=c['co'], fshape=(4, 4, c['co'], real), taps=taps)
        assert k == 4 and c['pad'] == 1
        return dict(OH=2 * h, OW=2 * w, PH=h, PW=w, nn=_nn(c), fshape=(4, 4, c['ci'], real), taps=taps)
    if kind == 'conv_dgrad':        # stride 1: dx[i] takes dy[i + p - ky] through tap ky
        p = (k - 1) // 2 if c['pad'] == 'same' else c['pad']
        OH, OW = (h, w) if c['pad'] == 'same' else (h - 2 * p + k - 1, w - 2 * p + k - 1)
        return dict(OH=OH, OW=OW, PH=OH, PW=OW, nn=_nn(c), fshape=(k, k, c['ci'], real), pad_before=p,
                    taps=[(ky, kx, 1, p - ky, p - kx, 1, 0, 0) for ky in range(k) for kx in range(k)])
    assert kind == 'deconv_dgrad' and h % 2 == 0 and w % 2 == 0       # dx[i] takes dy[2i - 1 + ky]
    return dict(OH=h // 2, OW=w // 2, PH=h // 2, PW=w // 2, nn=_nn(c), fshape=(4, 4, real, c['ci']),
                taps=[(ky, kx, 2, ky - 1, kx - 1, 1, 0, 0) for ky in range(4) for kx in range(4)])


def _nn(c):
    return c['ci'] - c['n_off'] if c['nn'] is None else c['nn']


def rows(c):
    geo = geometry(c)
    return c['n'] * geo['OH'] * geo['OW']


def _rnd(gen, *shape):
    return torch.randn(*shape, generator=gen)


def make_inputs(c):
    """Seeded float32 CPU tensors of a case: s0, s1 NHWC sources (None where C1 == 0) with c['lane'] in the padding lanes (the
    last lanes of the last source), ab0, ab1 folded norms [a; b] (None: no norm), w the filter as the wrapper takes it, bias and
    base (what the output holds before an accumulating launch) or None."""
    gen = torch.Generator().manual_seed(c['seed'])
    geo = geometry(c)
    n, h, w = c['n'], c['h'], c['w']
    C0, C1, real = c['src']
    norm0, _, norm1, _ = c['tf']
    assert C0 % 4 == 0 and C1 % 4 == 0 and 0 < real <= C0 + C1 and (C1 == 0 or real > C0)
    full = _rnd(gen, n, h, w, C0 + C1)
    if c['probe'] == 'onehot':          # one non-zero channel per pixel, at a seeded random channel
        ch = torch.randint(0, real, (n, h, w, 1), generator=gen)
        full = full * (torch.arange(C0 + C1).view(1, 1, 1, -1) == ch)
    elif c['probe'] == 'channel':       # one non-zero channel in the whole tensor
        ch = int(torch.randint(0, real, (1,), generator=gen))
        full = full * (torch.arange(C0 + C1).view(1, 1, 1, -1) == ch)
    else:
        assert c['probe'] is None
    full[..., real:] = c['lane']
    out = dict(s0=full[..., :C0].contiguous(), s1=full[..., C0:].contiguous() if C1 else None)
    out['ab0'] = torch.cat([1.0 + 0.1 * _rnd(gen, C0), 0.2 * _rnd(gen, C0)]) if norm0 else None
    out['ab1'] = torch.cat([1.0 + 0.1 * _rnd(gen, C1), 0.2 * _rnd(gen, C1)]) if (norm1 and C1) else None
    out['w'] = _rnd(gen, *geo['fshape']) * 0.1
    out['bias'] = _rnd(gen, geo['nn']) * 0.3 if c['bias'] else None
    out['base'] = _rnd(gen, n, geo['OH'], geo['OW'], geo['nn']) if c['acc'] else None
    return out


def _act(t, act):
    if act == 1:
        return torch.relu(t)
    if act == 2:
        return T.lrelu(t, 0.2)
    assert act == 0
    return t


def transformed(c, inp, dtype=torch.float64):
    """act(a*x + b) of the gathered tensor, its real channels: [n, h, w, real]."""
    _, act, _, act1 = c['tf']
    parts = []
    for i, a in ((0, act), (1, act if act1 < 0 else act1)):
        s, ab = inp['s%d' % i], inp['ab%d' % i]
        if s is None:
            continue
        t = s.to(dtype)
        if ab is not None:
            C = s.shape[3]
            t = t * ab[:C].to(dtype) + ab[C:].to(dtype)
        parts.append(_act(t, a))
    return torch.cat(parts, 3)[..., :c['src'][2]].contiguous()


def _tap_matrix(c, w, ky, kx):
    """The [real, nn] matrix of filter tap (ky, kx)."""
    kind = c['kind']
    if kind == 'matmul':
        return w
    if kind == 'matmul_nt':
        return w.t()
    if kind == 'conv':
        return w[ky, kx]
    if kind == 'deconv':
        return w[ky, kx].t()
    if kind == 'conv_dgrad':
        return w[ky, kx, c['n_off']:c['n_off'] + _nn(c)].t()
    return w[ky, kx][:, c['n_off']:c['n_off'] + _nn(c)]


def epilogue(c, t):
    """The launch's epilogue activation: 0 none, 1 tanh, 2 lrelu 0.2."""
    return torch.tanh(t) if c['epi'] == 1 else (T.lrelu(t, 0.2) if c['epi'] == 2 else t)


def ref_taps(c, inp, dtype=torch.float64):
    """(b): (ref, S, K) [n, OH, OW, nn] in front of the epilogue's activation; S the sum of the absolute products, K the number
    of non-zero products of every element (both float64).  dtype float32 gives what a CPU computes in the kernel's own precision."""
    geo = geometry(c)
    X = transformed(c, inp, dtype)
    w = inp['w'].to(dtype)
    shape = (c['n'], geo['OH'], geo['OW'], geo['nn'])
    ref, S, K = torch.zeros(shape, dtype=dtype), torch.zeros(shape, dtype=torch.float64), torch.zeros(shape, dtype=torch.float64)
    X64 = X.double()
    Xa, Xn = X64.abs(), (X64 != 0).float()
    GH, GW = X.shape[1:3]
    for ky, kx, s, oy, ox, os, ry, rx in geo['taps']:
        ys = [py for py in range(geo['PH']) if 0 <= py * s + oy < GH]
        xs = [px for px in range(geo['PW']) if 0 <= px * s + ox < GW]
        if not ys or not xs:
            continue
        y0, y1, x0, x1 = ys[0], ys[-1] + 1, xs[0], xs[-1] + 1
        assert ys == list(range(y0, y1)) and xs == list(range(x0, x1))
        src = (slice(None), slice(y0 * s + oy, (y1 - 1) * s + oy + 1, s), slice(x0 * s + ox, (x1 - 1) * s + ox + 1, s))
        dst = (slice(None), slice(y0 * os + ry, (y1 - 1) * os + ry + 1, os), slice(x0 * os + rx, (x1 - 1) * os + rx + 1, os))
        Wm = _tap_matrix(c, w, ky, kx)
        W64 = Wm.double()
        ref[dst] += torch.einsum('nyxk,kc->nyxc', X[src], Wm)
        S[dst] += torch.einsum('nyxk,kc->nyxc', Xa[src], W64.abs())
        K[dst] += torch.einsum('nyxk,kc->nyxc', Xn[src], (W64 != 0).float()).double()
    for extra in (inp['bias'], inp['base']):        # one more term each
        if extra is not None:
            ref += extra.to(dtype)
            S += extra.double().abs()
            K += 1
    return ref, S, K


def ref_tf(c, inp):
    """(a): the op of oracle/tf_ops.py on double tensors, epilogue included: [n, OH, OW, nn]."""
    geo = geometry(c)
    kind, k, s = c['kind'], c['k'], c['stride']
    X = transformed(c, inp).permute(0, 3, 1, 2).contiguous()       # NCHW, real channels
    w = inp['w'].double()
    if kind == 'matmul':
        y = (X[0, :, 0].t() @ w).view(1, 1, c['w'], -1)
    elif kind == 'matmul_nt':
        y = (X[0, :, 0].t() @ w.t()).view(1, 1, c['w'], -1)
    elif kind == 'conv':
        y = T.conv2d_same(X, w, s) if c['pad'] == 'same' else T.conv2d_valid_pad(X, w, s, c['pad'])
        y = y.permute(0, 2, 3, 1)
    elif kind == 'deconv':
        y = T.conv2d_transpose_same_s2(X, w).permute(0, 2, 3, 1)
    else:
        x = torch.zeros(c['n'], c['ci'], geo['OH'], geo['OW'], dtype=torch.float64, requires_grad=True)
        if kind == 'deconv_dgrad':
            f = T.conv2d_transpose_same_s2(x, w)
        else:
            f = T.conv2d_same(x, w, s) if c['pad'] == 'same' else T.conv2d_valid_pad(x, w, s, c['pad'])
        assert f.shape == X.shape, (f.shape, X.shape)
        (f * X).sum().backward()
        y = x.grad[:, c['n_off']:c['n_off'] + geo['nn']].permute(0, 2, 3, 1)
    if inp['bias'] is not None:
        y = y + inp['bias'].double()
    if inp['base'] is not None:
        y = y + inp['base'].double()
    return epilogue(c, y.contiguous())
