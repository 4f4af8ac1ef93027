"""The float64 reference of the filter-gradient form (conv_wgrad_kernel of csrc/igemm.hip), written twice, and the tables of
cases tests/test_gpu_wgrad_forms.py (CASES) and tests/test_gpu_wgrad128_forms.py (CASES128: the 128 x 128 kernels) run on the
device.

    dF[(ty, tx), cg, cd] = sum over pixels (n, py, px) of  act(a*G + b)[n, py*s + oy + ty, px*s + ox + tx][cg] * act(a*D + b)[n, py, px][cd]

with a tap outside the gathered image contributing nothing, cg below the real gathered channels and cd below the real dense ones.

  ref_autograd  (a) the TF op of oracle/tf_ops.py on double tensors, the filter's gradient by autograd
  ref_taps      (b) a loop over the taps with shifted slices and einsum; also S = the same sum over |products|, which the
                comparison rule (kernel_check.check_dot) scales its bound with

tests/test_wgrad_oracle.py holds (a) against (b) on every case of the table, without a GPU.

A case describes the launch the way the hip.py wrappers see it:
  kind    'conv'   gathered = x [n, h, w, *], dense = dy; k x k taps, stride, pad (an int: tf.pad + VALID; 'same': TF SAME)
          'deconv' gathered = dy [n, 2h, 2w, *], dense = x [n, h, w, *]: the k = 4 stride-2 transposed conv
          'mm'     gathered = a [h*w rows, *], dense = b: the 1 x 1 form of hip.matmul_tn (n = h = 1)
  g, d    (C0, C1, real): stored channels of the two sources and how many of C0 + C1 are real; the others are padding lanes
  gt, dt  (norm0, act, norm1, act1): folded norm on source 0 / 1, activation of source 0, of source 1 (-1: the same)
"""
import torch

from oracle import tf_ops as T

PAD_LANE = 1.0e3        # what padding channels and everything around a tensor hold: the kernel may not rely on zeros there
PLAIN = (False, 0, False, -1)


def _case(name, kind, n, h, w, g, d, k=1, stride=1, pad=0, gt=PLAIN, dt=PLAIN, **expect):
    return dict(name=name, kind=kind, n=n, h=h, w=w, k=k, stride=stride, pad=pad, g=g, d=d, gt=gt, dt=dt, expect=expect)


# expect: tile (0 128x128, 1 64x128, 2 128x64, 3 64x64, 4 128x32) and view form (0 TTT, 1 FTT, 2 TTF, 3 FTF, 4 FFF) as
# ssc_conv_wgrad_plan must report them; tile is a tuple where the planner chooses by cost (Nn > 64 and more than 64 gathered
# columns: 128x128, 64x128 or 128x64)
NORM_LRELU = (True, 2, False, -1)
CASES = [
    # --- 128x32: Nn <= 32
    _case('t4_first_layer_4x4s2', 'conv', 2, 12, 12, (4, 0, 3), (24, 0, 24), k=4, stride=2, pad=1, tile=4, view=0),
    _case('t4_7x7s2_p33', 'conv', 1, 6, 22, (4, 0, 3), (16, 0, 16), k=7, stride=2, pad=3, tile=4, view=0),      # 196 gathered rows, P = 3 x 11
    _case('t4_nn1_dy4', 'conv', 2, 5, 6, (16, 0, 16), (4, 0, 1), k=3, stride=1, pad=1, gt=NORM_LRELU, tile=4, view=1),
    _case('t4_nn3_dy4_deconv', 'deconv', 2, 5, 4, (4, 0, 3), (4, 0, 3), tile=4, view=0),
    _case('t4_3x3x3x3', 'conv', 2, 20, 20, (4, 0, 3), (4, 0, 3), k=3, stride=1, pad=1, tile=4, view=0),         # 81 elements: reduce<1>
    _case('t4_1x1_16_24', 'conv', 4, 32, 32, (16, 0, 16), (24, 0, 24), tile=4, view=0),                        # 384 elements: reduce<16>
    _case('t4_two_dense_plain', 'deconv', 1, 4, 5, (8, 0, 8), (12, 8, 20), tile=4, view=2),                    # P = 20
    # --- 64x64: 32 < Nn <= 64, at most 64 gathered columns
    _case('t3_mm_48_40_p300', 'mm', 1, 1, 300, (48, 0, 48), (40, 0, 40), tile=3, view=0),                      # ragged last K-tile
    _case('t3_mm_p20_norm', 'mm', 1, 1, 20, (36, 0, 36), (64, 0, 64), gt=NORM_LRELU, tile=3, view=1),
    _case('t3_mm_two_gathered', 'mm', 1, 1, 33, (20, 24, 44), (36, 0, 33), gt=(True, 2, True, 1), tile=3, view=1),
    # --- 128x64: 32 < Nn <= 64, more than 64 gathered columns
    _case('t2_3x3same_32_48', 'conv', 2, 8, 8, (32, 0, 32), (48, 0, 48), k=3, stride=1, pad='same', tile=2, view=0),
    _case('t2_3x3same_s2_even', 'conv', 2, 8, 8, (20, 16, 36), (40, 0, 40), k=3, stride=2, pad='same', gt=NORM_LRELU,
          tile=2, view=1),                                                                                     # SAME pad 0 before, 1 after
    _case('t2_deconv_two_dense_plain', 'deconv', 2, 5, 3, (12, 0, 12), (40, 24, 64), tile=2, view=2),
    _case('t2_deconv_two_dense_g_norm', 'deconv', 2, 3, 5, (12, 0, 10), (24, 16, 40), gt=(True, 1, False, -1), tile=2, view=3),
    _case('t2_deconv_dense_norm_relu', 'deconv', 2, 4, 4, (8, 0, 8), (32, 16, 48), dt=(True, 1, True, 2), tile=2, view=4),
    # --- 64x128: Nn > 64, at most 64 gathered columns
    _case('t1_1x1_64_96', 'conv', 1, 15, 20, (64, 0, 64), (96, 0, 96), tile=1, view=0),                        # P = 300
    _case('t1_mm_p33_two_gathered', 'mm', 1, 1, 33, (36, 28, 64), (132, 0, 130), tile=1, view=0),
    _case('t1_mm_dense_norm', 'mm', 1, 1, 300, (40, 0, 40), (72, 0, 72), dt=(True, 2, False, -1), tile=1, view=4),
    _case('t1_mm_two_dense_plain', 'mm', 1, 1, 20, (48, 0, 48), (64, 32, 96), gt=NORM_LRELU, tile=1, view=3),
    # --- Nn > 64, more than 64 gathered columns: 128x128 where the planner or the pinned child process says so
    _case('t0_4x4s2_odd_96', 'conv', 2, 9, 7, (32, 0, 32), (96, 0, 96), k=4, stride=2, pad=1, gt=NORM_LRELU,
          tile=(0, 1, 2), view=1),                                                                             # odd size: taps off the bottom / right
    _case('t0_nn130_p200', 'conv', 2, 10, 10, (128, 0, 128), (132, 0, 130), tile=(0, 1, 2), view=0),           # wgrad128's shape below its 256 pixels
    _case('t0_3x3_two_gathered', 'conv', 3, 10, 10, (40, 24, 64), (96, 0, 96), k=3, stride=1, pad=1, gt=(True, 2, True, 1),
          tile=(0, 1, 2), view=1),                                                                             # C0 = 40: no multiple of a tile width
    _case('t0_deconv_dense_norm', 'deconv', 2, 6, 6, (16, 0, 16), (64, 32, 96), dt=(True, 1, True, 2), tile=(0, 1, 2), view=4),
    _case('t0_deconv_two_dense_plain', 'deconv', 1, 5, 4, (8, 0, 8), (64, 32, 96), tile=(0, 1, 2), view=2),
    _case('t0_conv_split', 'conv', 2, 64, 64, (32, 0, 32), (96, 0, 96), k=3, stride=1, pad=1, gt=NORM_LRELU,
          tile=(0, 1, 2), view=1),                                                                             # 8192 pixels: split-K
]
BY_NAME = {c['name']: c for c in CASES}
assert len(BY_NAME) == len(CASES)


# --- the 128 x 128 kernels (csrc/wgrad128.hip exact fp32, csrc/wgrad128_bf16.hip bf16x6): tests/test_gpu_wgrad128_forms.py.
# expect: tpt, the taps per tile ssc_conv_wgrad128_plan must report; bf_only: the exact kernel does not take the launch (the
# generic one does).  P = NB * PH * PW >= 256, Nn >= 128 and even, two dense sources only with C0 % 128 == 0.
LRELU = (False, 2, False, -1)
NORM_RELU = (True, 1, False, -1)
CASES128 = [
    # --- both kernels
    _case('w1_1x1_p256', 'conv', 1, 16, 16, (128, 0, 128), (128, 0, 128), tpt=1),                              # P exactly 256; TW = 1
    _case('w1_4x4s2_p300', 'conv', 3, 20, 20, (128, 0, 128), (256, 0, 256), k=4, stride=2, pad=1, gt=NORM_LRELU, tpt=1),   # 300 = 9 * 32 + 12
    _case('w1_two_gathered', 'conv', 2, 12, 12, (128, 128, 256), (128, 0, 128), k=3, stride=1, pad=1, gt=(True, 2, True, 1), tpt=1),
    _case('w1_nn130', 'conv', 2, 12, 12, (128, 0, 128), (132, 0, 130), k=3, stride=1, pad=1, tpt=1),           # a column tile of 2 columns
    _case('w1_deconv_two_dense_norm', 'deconv', 2, 12, 12, (128, 0, 128), (128, 128, 256), dt=(True, 1, True, 2), tpt=1),
    _case('w1_deconv_512_64_plain', 'deconv', 2, 12, 12, (128, 0, 128), (512, 64, 576), tpt=1),                # last column tile half empty
    _case('w1_odd_s2', 'conv', 2, 33, 23, (128, 0, 128), (128, 0, 128), k=4, stride=2, pad=1, gt=LRELU, tpt=1),
    _case('w1_same_4x4s1', 'conv', 2, 12, 12, (256, 0, 256), (128, 0, 128), k=4, stride=1, pad='same', gt=NORM_LRELU, tpt=1),  # pad 1 before, 2 after
    _case('w1_column_image', 'conv', 2, 160, 1, (128, 0, 128), (128, 0, 128), k=3, stride=1, pad=1, tpt=1),    # PW = 1
    _case('w1_fc', 'conv', 300, 1, 1, (128, 0, 128), (128, 0, 128), dt=NORM_LRELU, tpt=1),                      # PH * PW = 1
    _case('w1_mm_1000', 'mm', 1, 1, 1000, (128, 0, 128), (256, 0, 256), gt=NORM_LRELU, tpt=1),
    _case('w1_split', 'conv', 2, 64, 64, (128, 0, 128), (128, 0, 128), k=3, stride=1, pad=1, gt=NORM_LRELU, tpt=1),        # 8192 pixels: split-K
    _case('w1_split_xcd', 'conv', 2, 64, 64, (128, 0, 128), (128, 0, 128), k=4, stride=2, pad=1, gt=NORM_LRELU, tpt=1),   # 2048 pixels, 16 row
                                                                                        # tiles: 10 slices of 7 K-tiles, a grid of 160 in XCD order
    _case('w2_4x4s2', 'conv', 2, 24, 24, (64, 0, 64), (128, 0, 128), k=4, stride=2, pad=1, gt=LRELU, tpt=2),
    _case('w2_9taps', 'conv', 2, 15, 15, (64, 0, 64), (192, 0, 192), k=3, stride=1, pad=1, gt=NORM_RELU, tpt=2),           # last row tile: ONE tap
    _case('w2_div64', 'conv', 1, 256, 256, (64, 0, 64), (128, 0, 128), k=3, stride=1, pad=1, tpt=2),           # P * PH * PW = 2^32
    # --- the bf16 kernel alone: tiles over the padded row space that span two or three taps
    _case('b2_132_131', 'conv', 2, 12, 12, (132, 0, 131), (128, 0, 128), k=3, stride=1, pad='same', tpt=2, bf_only=True),
    _case('b2_260_259_norm', 'conv', 2, 12, 12, (260, 0, 259), (256, 0, 256), k=3, stride=1, pad='same', gt=NORM_LRELU, tpt=2, bf_only=True),
    _case('b2_192', 'conv', 2, 12, 12, (192, 0, 192), (128, 0, 128), k=3, stride=1, pad='same', tpt=2, bf_only=True),
    _case('b2_1x1_516_515', 'conv', 3, 12, 12, (516, 0, 515), (256, 0, 256), tpt=2, bf_only=True),             # one tap, 4.03 row tiles
    _case('b3_68_67', 'conv', 2, 12, 12, (68, 0, 67), (128, 0, 128), k=3, stride=1, pad='same', tpt=3, bf_only=True),
    _case('b3_96', 'conv', 2, 12, 12, (96, 0, 96), (128, 0, 128), k=3, stride=1, pad='same', tpt=3, bf_only=True),
    _case('b3_124_121', 'conv', 2, 12, 12, (124, 0, 121), (128, 0, 128), k=3, stride=1, pad='same', gt=NORM_LRELU, tpt=3, bf_only=True),
]
for _i, _c in enumerate(CASES128):
    _c['seed'] = 5000 + _i          # a seed base of its own: CASES seeds from its index, and its inputs do not move
BY_NAME128 = {c['name']: c for c in CASES128}
assert len(BY_NAME128) == len(CASES128) and not set(BY_NAME128) & set(BY_NAME)

# The full product of forms: one carrier per taps-per-tile, each with the gathered and the dense side plain (P) or transformed (T)
CARRIERS = ('w1_two_gathered', 'w2_4x4s2', 'b3_96')
CARRIER_FORMS = [(n, gt, dt) for n in CARRIERS for gt in 'PT' for dt in 'PT']


def carrier(name, gt, dt):
    """The carrier case `name` with its gathered / dense side plain ('P') or transformed ('T'): norm + lrelu, on a second
    gathered source norm + relu."""
    base = BY_NAME128[name]
    two = base['g'][1] > 0
    c = dict(base, name='%s/g%s_d%s' % (name, gt, dt), gt=((True, 2, True, 1) if two else NORM_LRELU) if gt == 'T' else PLAIN,
             dt=NORM_LRELU if dt == 'T' else PLAIN, seed=9000 + CARRIER_FORMS.index((name, gt, dt)))
    return c


def geometry(c):
    """NB, gathered H W, lattice PH PW, TH TW, stride, offset of tap 0 (y, x)."""
    n, h, w, k, s = c['n'], c['h'], c['w'], c['k'], c['stride']
    if c['kind'] == 'deconv':
        return dict(NB=n, GH=2 * h, GW=2 * w, PH=h, PW=w, TH=4, TW=4, stride=2, oy=-1, ox=-1)
    if c['kind'] == 'mm':
        return dict(NB=1, GH=1, GW=h * w, PH=1, PW=h * w, TH=1, TW=1, stride=1, oy=0, ox=0)
    if c['pad'] == 'same':
        py, px = T.same_pads(h, k, s)[0], T.same_pads(w, k, s)[0]
        return dict(NB=n, GH=h, GW=w, PH=-(-h // s), PW=-(-w // s), TH=k, TW=k, stride=s, oy=-py, ox=-px)
    p = c['pad']
    return dict(NB=n, GH=h, GW=w, PH=(h + 2 * p - k) // s + 1, PW=(w + 2 * p - k) // s + 1, TH=k, TW=k, stride=s, oy=-p, ox=-p)


def pixels(c):
    g = geometry(c)
    return g['NB'] * g['PH'] * g['PW']


def _rnd(gen, *shape):
    return torch.randn(*shape, generator=gen)


def make_inputs(c):
    """Seeded float32 CPU tensors of a case: g0, g1, d0, d1 NHWC sources (None where C1 == 0) with 1.0e3 in the padding lanes
    (the last lanes of the last source), gab0, gab1, dab0, dab1 folded norms [a; b] (None: no norm)."""
    gen = torch.Generator().manual_seed(c['seed'] if 'seed' in c else 1000 + CASES.index(BY_NAME[c['name']]))
    geo = geometry(c)
    out = {}
    for side, (H, W) in (('g', (geo['GH'], geo['GW'])), ('d', (geo['PH'], geo['PW']))):
        C0, C1, real = c[side]
        norm0, _, norm1, _ = c[side + 't']
        assert C0 % 4 == 0 and C1 % 4 == 0 and 0 < real <= C0 + C1 and (C1 == 0 or real > C0)
        s0 = _rnd(gen, geo['NB'], H, W, C0)
        s1 = _rnd(gen, geo['NB'], H, W, C1) if C1 else None
        if real < C0 + C1:
            (s1 if C1 else s0)[..., real - (C0 if C1 else 0):] = PAD_LANE
        out[side + '0'], out[side + '1'] = s0, s1
        out[side + 'ab0'] = torch.cat([1.0 + 0.1 * _rnd(gen, C0), 0.2 * _rnd(gen, C0)]) if norm0 else None
        out[side + 'ab1'] = torch.cat([1.0 + 0.1 * _rnd(gen, C1), 0.2 * _rnd(gen, C1)]) if (norm1 and C1) else None
    return out


def _act(t, act):
    if act == 1:
        return torch.relu(t)
    if act == 2:
        return T.lrelu(t, 0.2)
    assert act == 0
    return t


def transformed(c, inp, side, dtype=torch.float64):
    """act(a*x + b) of one side over all its stored lanes: [NB, H, W, C0 + C1]."""
    norm0, act, norm1, act1 = c[side + 't']
    parts = []
    for i, a in ((0, act), (1, act if act1 < 0 else act1)):
        s, ab = inp['%s%d' % (side, i)], inp['%sab%d' % (side, i)]
        if s is None:
            continue
        t = s.to(dtype)
        if ab is not None:
            C = s.shape[3]
            t = t * ab[:C].to(dtype) + ab[C:].to(dtype)
        parts.append(_act(t, a))
    return torch.cat(parts, 3)


def ref_taps(c, inp, dtype=torch.float64):
    """(b): (dF, S) [TH, TW, real gathered, real dense], S the sum of |products|; dtype float32 gives what a CPU computes in
    the kernel's own precision."""
    geo = geometry(c)
    G, D = transformed(c, inp, 'g', dtype)[..., :c['g'][2]], transformed(c, inp, 'd', dtype)[..., :c['d'][2]]
    s, PH, PW = geo['stride'], geo['PH'], geo['PW']
    dF = torch.zeros(geo['TH'], geo['TW'], G.shape[3], D.shape[3], dtype=dtype)
    S = torch.zeros_like(dF)
    for ty in range(geo['TH']):
        for tx in range(geo['TW']):
            # lattice rows / columns whose tap lies inside the gathered image
            ys = [py for py in range(PH) if 0 <= py * s + geo['oy'] + ty < geo['GH']]
            xs = [px for px in range(PW) if 0 <= px * s + geo['ox'] + tx < geo['GW']]
            if not ys or not xs:
                continue
            y0, y1, x0, x1 = ys[0], ys[-1] + 1, xs[0], xs[-1] + 1
            assert ys == list(range(y0, y1)) and xs == list(range(x0, x1))
            gy, gx = y0 * s + geo['oy'] + ty, x0 * s + geo['ox'] + tx
            Gs = G[:, gy:gy + (y1 - y0 - 1) * s + 1:s, gx:gx + (x1 - x0 - 1) * s + 1:s]
            Ds = D[:, y0:y1, x0:x1]
            dF[ty, tx] = torch.einsum('nyxg,nyxd->gd', Gs, Ds)
            S[ty, tx] = torch.einsum('nyxg,nyxd->gd', Gs.abs(), Ds.abs())
    return dF, S


def ref_autograd(c, inp):
    """(a): the gradient of the TF op's filter by autograd on double tensors."""
    geo = geometry(c)
    G = transformed(c, inp, 'g')[..., :c['g'][2]].permute(0, 3, 1, 2).contiguous()        # NCHW, real channels
    D = transformed(c, inp, 'd')[..., :c['d'][2]].permute(0, 3, 1, 2).contiguous()
    if c['kind'] == 'deconv':
        f = torch.zeros(4, 4, G.shape[1], D.shape[1], dtype=torch.float64, requires_grad=True)
        y = T.conv2d_transpose_same_s2(D, f)
        assert y.shape == G.shape
        (y * G).sum().backward()
        return f.grad
    w = torch.zeros(geo['TH'], geo['TW'], G.shape[1], D.shape[1], dtype=torch.float64, requires_grad=True)
    if c['kind'] == 'conv' and c['pad'] == 'same':
        y = T.conv2d_same(G, w, c['stride'])
    else:
        y = T.conv2d_valid_pad(G, w, geo['stride'], -geo['oy'])
    assert y.shape == D.shape, (y.shape, D.shape)
    (y * D).sum().backward()
    return w.grad


def term(c, inp, pixel, tap):
    """The products of one pixel (n, py, px) at one tap (ty, tx): [real gathered, real dense] in float64, zeros when the tap
    lies outside the gathered image."""
    geo = geometry(c)
    n, py, px = pixel
    gy, gx = py * geo['stride'] + geo['oy'] + tap[0], px * geo['stride'] + geo['ox'] + tap[1]
    G, D = transformed(c, inp, 'g')[..., :c['g'][2]], transformed(c, inp, 'd')[..., :c['d'][2]]
    if not (0 <= gy < geo['GH'] and 0 <= gx < geo['GW']):
        return torch.zeros(G.shape[3], D.shape[3], dtype=torch.float64)
    return torch.outer(G[n, gy, gx], D[n, py, px])
