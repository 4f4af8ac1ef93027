"""Helpers of the kernel-level tests of the small kernels (tests/test_gpu_small_kernels*.py): seeded CPU inputs, NaN-filled
device outputs, the raw return code of an entry point, and the two comparison rules those tests use.

  check      |device - float64 oracle| <= tol * max(1, max|oracle|)            (the close() convention of test_gpu_igemm.py)
  check_fp32 per element max(that floor, 4 x |float32 oracle - float64 oracle|): for formulas that lose digits in float32 by
             construction, the same way in the reference (the factor 4 allows for expf / logf / tanhf a few ulp off libm)
  check_dot  per element |device - float64 oracle| <= (K + 8) * 2^-24 * S for sums of K fp32 products, S the float64 sum of the
             absolute products: the any-order dot-product bound, nothing measured in it (tests/test_gpu_wgrad_forms.py,
             tests/test_gpu_wgrad128_forms.py)

All print the measured distance before they assert and log it with conftest.parity_log (variant='kernel', never forward=True:
these are not network outputs)."""
import torch

from conftest import parity_log

NAN = float('nan')


def hip():
    from sketchyscenecolorization_amd import hip as h
    return h


def rnd(*shape, seed=0, std=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * std


def randint(lo, hi, *shape, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(lo, hi, shape, generator=g, dtype=torch.int32)


def nan(*shape):
    return torch.full(shape, NAN, device='cuda')


def acc(*values):
    """A loss accumulator: double device scalars that the kernels add into."""
    return torch.tensor(values, dtype=torch.float64, device='cuda')


def rc(name, *args):
    """The return code of an entry point called through lib() directly (argument checks answer without launching)."""
    h = hip()
    conv = [h.ptr(a) if isinstance(a, torch.Tensor) else a for a in args]
    code = getattr(h.lib(), name)(*conv, h.stream_ptr())
    torch.cuda.synchronize()
    return code


def all_nan(t):
    return bool(torch.isnan(t).all().item())


GUARD = 16384           # floats on either side of a guarded tensor: more than a K-tile of the widest source


def bits(t):
    """The tensor's float32 bit patterns (NaN compares equal to the same NaN)."""
    return t.view(torch.int32)


def inside(t, fill):
    """(buffer, view): a copy of the CPU tensor t inside a device buffer that holds `fill` on both sides."""
    buf = torch.full((GUARD + t.numel() + GUARD,), fill, device='cuda')
    view = buf[GUARD:GUARD + t.numel()].view(t.shape)
    view.copy_(t)
    return buf, view


def _f64(t):
    return t.detach().cpu().double()


def check(test, config, got, ref, tol=1e-5, what=''):
    got, ref = _f64(got), _f64(ref)
    assert got.shape == ref.shape, (test, what, got.shape, ref.shape)
    assert bool(torch.isfinite(got).all()), (test, what, config, 'non-finite output')
    bound = tol * max(1.0, float(ref.abs().max()) if ref.numel() else 0.0)
    err = float((got - ref).abs().max()) if ref.numel() else 0.0
    print('%s %s %s: err %.3e bound %.3e' % (test, what, config, err, bound))
    parity_log(test, dict(config, what=what), err, bound, variant='kernel')
    assert err <= bound, (test, what, config, err, bound)
    return err


def check_scalar(test, config, got, ref, tol=1e-5, what='loss'):
    """Loss scalars: relative to the oracle's value."""
    got, ref = float(got), float(ref)
    bound = tol * abs(ref)
    err = abs(got - ref)
    print('%s %s %s: got %.9g ref %.9g err %.3e bound %.3e' % (test, what, config, got, ref, err, bound))
    parity_log(test, dict(config, what=what), err, bound, variant='kernel')
    assert err == err and err <= bound, (test, what, config, got, ref)
    return err


def check_fp32(test, config, got, ref64, ref32, tol=1e-5, what=''):
    got, ref64, ref32 = _f64(got), _f64(ref64), _f64(ref32)
    assert got.shape == ref64.shape == ref32.shape, (test, what, got.shape, ref64.shape, ref32.shape)
    assert bool(torch.isfinite(got).all()), (test, what, config, 'non-finite output')
    floor = tol * max(1.0, float(ref64.abs().max()))
    cpu = (ref32 - ref64).abs()
    bound = torch.clamp(4.0 * cpu, min=floor)
    err = (got - ref64).abs()
    k = int(torch.argmax(err / bound))
    e, b, c = float(err.reshape(-1)[k]), float(bound.reshape(-1)[k]), float(cpu.max())
    print('%s %s %s: err %.3e (bound there %.3e, max err %.3e), fp32 oracle vs f64 %.3e' % (test, what, config, e, b, float(err.max()), c))
    parity_log(test, dict(config, what=what), e, b, variant='kernel', cpu_fp32_vs_f64=c, max_err_anywhere=float(err.max()))
    assert bool((err <= bound).all()), (test, what, config, e, b)


U_FP32 = 2.0 ** -24        # unit roundoff of fp32


def check_dot(test, config, got, ref64, S, K, plan=None, what='', extra_terms=0, allow=None):
    """An fp32 sum of K products, added up in any order: per element |got - ref64| <= (K + 8) * 2^-24 * S, where S is the float64
    sum of the absolute products of that element.  gamma_K = K*u / (1 - K*u) bounds the rounding of the products and of the K - 1
    additions in whatever order (Higham, Accuracy and Stability of Numerical Algorithms, section 3.1); the 8 more roundings per
    term allow for the folded norm (one fma), the activation's slope product and the float32 slope constant on either factor, and
    the additions of split-K slabs and of an accumulate base, which the caller counts as one more term of S.  (K + 8) * u stands
    for gamma_(K+8): the quotient 1 - (K+8)*u is within 1e-3 of 1 for every K the tests use, K <= 8192.)
    Beyond K + 8 = 16384 (up to 2^17) the bound is gamma_(K+8) = (K+8)*u / (1 - (K+8)*u) itself.
    extra_terms: further roundings per term a kernel's arithmetic costs by construction, added to the 8 (the bf16x6 filter
    gradient: 2, its three dropped products, together below 2^-23 |a*b|).
    K may be a tensor of S's shape: the terms of every element (the forward tests count the non-zero products per element).
    allow: an absolute allowance per element, added to the bound (tests/test_gpu_fwd_bf16_forms.py: a 1-Lipschitz epilogue
    activation evaluated to a few ulp, 8 * 2^-24 * |f(ref)|).  Without either the bound is the one above.
    plan: what ssc_conv_wgrad_plan reported for the launch, logged with the worst err / bound ratio."""
    got, ref64, S = _f64(got), _f64(ref64), _f64(S)
    assert got.shape == ref64.shape == S.shape, (test, what, got.shape, ref64.shape, S.shape)
    if isinstance(K, torch.Tensor):
        K = _f64(K)
        assert K.shape == S.shape and float(K.max()) + 8 + extra_terms <= 16384 and extra_terms >= 0, (test, what, K.shape)
        bound = (K + 8 + extra_terms) * U_FP32 * S
        K = int(K.max())
    else:
        n = K + 8 + extra_terms
        assert extra_terms >= 0 and n <= 2 ** 17, (K, extra_terms)
        bound = (n * U_FP32 if K + 8 <= 16384 else n * U_FP32 / (1.0 - n * U_FP32)) * S
    assert bool(torch.isfinite(got).all()), (test, what, config, 'non-finite output')
    if allow is not None:
        allow = _f64(allow)
        assert allow.shape == S.shape and bool((allow >= 0).all()), (test, what, allow.shape)
        bound = bound + allow
    err = (got - ref64).abs()
    ratio = torch.where(err > 0, err / torch.clamp(bound, min=1e-300), torch.zeros_like(err))
    k = int(torch.argmax(ratio))
    r, e, b = float(ratio.reshape(-1)[k]), float(err.reshape(-1)[k]), float(bound.reshape(-1)[k])
    print('%s %s %s plan %s: worst err/bound %.3e (err %.3e, bound there %.3e), max err %.3e' %
          (test, what, config, plan, r, e, b, float(err.max())))
    parity_log(test, dict(config, what=what), e, b, variant='kernel', ratio=r, K=int(K), plan=list(plan) if plan is not None else None)
    assert bool((err <= bound).all()), (test, what, config, 'err/bound', r, 'at', k)
    return r
