// match_backbone_train.hip -- what the backward pass of the matcher's DeepLab-ResNet backbone lacks beside the data-gradient and
// filter-gradient kernels (sketchyscenecolorization_amd/match_backbone_train.py).  The backbone's norms
// are frozen (deeplab_model.py: beta, gamma, factor, mean, variance are not trainable and the stored moments are used), so the
// backward of relu(a * r + b) needs no statistics:
//   ssc_frozen_act_bwd     dr = g * a * (a*r + b > 0)
//   ssc_unit_merge_bwd     the unit's closing relu(a3*r3 + b3 + shortcut): one mask, both branches
//   ssc_zero_stuff2        the data gradient of a 1x1 stride-2 conv from the stride-1 one: the even pixels, zero elsewhere
//   ssc_max_pool3s2_bwd    tf.nn.max_pool(3x3, 2, SAME) of relu(a*r0 + b), gather form
// At an activation of exactly 0 the mask is 0.  All of it is memory-bound: a thread owns four channels of one pixel, 16-byte
// accesses, grid-stride loops over at most 2048 workgroups, no LDS, no atomics: the same bits on every run.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "sketchycolor_hip.h"

#define CHECK_LAUNCH() ((int)hipGetLastError())
#define MAX_FLOATS (0x7fffffffL * 4L)

static inline unsigned blocks_for(long n) {
    long blocks = (n + 255) / 256;
    if (blocks < 1) blocks = 1;
    return (unsigned)(blocks > 2048 ? 2048 : blocks);
}

static __device__ __forceinline__ float4 ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }
static __device__ __forceinline__ void st4(float* p, float4 v) { *reinterpret_cast<float4*>(p) = v; }

// ---------------------------------------------------------------------------------------------------------------------------
// dr[p, c] = g[p, c] * a[c] * (a[c]*r[p, c] + b[c] > 0).  dr may be g (every element is read before it is written).
// ---------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void frozen_act_bwd_kernel(const float* g, const float* __restrict__ r,
                                                             const float* __restrict__ ab, int C, long total, float* dr) {
    const int c4n = C >> 2;
    for (long t = (long)blockIdx.x * 256 + threadIdx.x; t < total; t += (long)gridDim.x * 256) {
        const int c = (int)(t % c4n) * 4;
        const float4 a = ld4(ab + c), b = ld4(ab + C + c), x = ld4(r + t * 4), gg = ld4(g + t * 4);
        float4 o;
        o.x = fmaf(a.x, x.x, b.x) > 0.f ? gg.x * a.x : 0.f;
        o.y = fmaf(a.y, x.y, b.y) > 0.f ? gg.y * a.y : 0.f;
        o.z = fmaf(a.z, x.z, b.z) > 0.f ? gg.z * a.z : 0.f;
        o.w = fmaf(a.w, x.w, b.w) > 0.f ? gg.w * a.w : 0.f;
        st4(dr + t * 4, o);
    }
}

extern "C" int ssc_frozen_act_bwd(const float* g, const float* r, const float* ab, int64_t M, int C, float* dr, void* stream) {
    if (M < 1 || C < 4 || (C & 3) || M * (int64_t)C > MAX_FLOATS) return -1;
    if (g == nullptr || r == nullptr || ab == nullptr || dr == nullptr || dr == r) return -1;
    if (((uintptr_t)g | (uintptr_t)r | (uintptr_t)ab | (uintptr_t)dr) & 15) return -3;
    const long total = (long)M * (C / 4);
    hipLaunchKernelGGL(frozen_act_bwd_kernel, dim3(blocks_for(total)), dim3(256), 0, (hipStream_t)stream, g, r, ab, C, total, dr);
    return CHECK_LAUNCH();
}

// ---------------------------------------------------------------------------------------------------------------------------
// out = relu(a3*r3 + b3 + (ab_add ? a_add*sc + b_add : x)) (ssc_residual_merge), g = d loss / d out, m = out > 0:
//   dr3 = g * m * a3;   d2 = ab_add ? g * m * a_add (the gradient of sc) : g * m (the gradient of x)
// ---------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void unit_merge_bwd_kernel(const float* __restrict__ g, const float* __restrict__ out,
                                                             const float* __restrict__ ab3, const float* __restrict__ ab_add, int C,
                                                             long total, float* __restrict__ dr3, float* __restrict__ d2) {
    const int c4n = C >> 2;
    for (long t = (long)blockIdx.x * 256 + threadIdx.x; t < total; t += (long)gridDim.x * 256) {
        const int c = (int)(t % c4n) * 4;
        const float4 a3 = ld4(ab3 + c), o = ld4(out + t * 4);
        float4 gm = ld4(g + t * 4);
        gm.x = o.x > 0.f ? gm.x : 0.f;
        gm.y = o.y > 0.f ? gm.y : 0.f;
        gm.z = o.z > 0.f ? gm.z : 0.f;
        gm.w = o.w > 0.f ? gm.w : 0.f;
        st4(dr3 + t * 4, make_float4(gm.x * a3.x, gm.y * a3.y, gm.z * a3.z, gm.w * a3.w));
        if (ab_add != nullptr) {
            const float4 a = ld4(ab_add + c);
            gm = make_float4(gm.x * a.x, gm.y * a.y, gm.z * a.z, gm.w * a.w);
        }
        st4(d2 + t * 4, gm);
    }
}

extern "C" int ssc_unit_merge_bwd(const float* g, const float* out, const float* ab3, const float* ab_add, int64_t M, int C,
                                  float* dr3, float* d2, void* stream) {
    if (M < 1 || C < 4 || (C & 3) || M * (int64_t)C > MAX_FLOATS) return -1;
    if (g == nullptr || out == nullptr || ab3 == nullptr || dr3 == nullptr || d2 == nullptr) return -1;
    if (dr3 == d2 || dr3 == g || dr3 == out || d2 == g || d2 == out) return -1;
    if (((uintptr_t)g | (uintptr_t)out | (uintptr_t)ab3 | (uintptr_t)ab_add | (uintptr_t)dr3 | (uintptr_t)d2) & 15) return -3;
    const long total = (long)M * (C / 4);
    hipLaunchKernelGGL(unit_merge_bwd_kernel, dim3(blocks_for(total)), dim3(256), 0, (hipStream_t)stream, g, out, ab3, ab_add, C,
                       total, dr3, d2);
    return CHECK_LAUNCH();
}

// ---------------------------------------------------------------------------------------------------------------------------
// out [N, H, W, C] (H in {2h - 1, 2h}, W in {2w - 1, 2w}): out[n, 2y, 2x] = src[n, y, x], zero at every pixel with an odd
// coordinate.  A 1x1 SAME conv of stride 2 reads the pixels (2y, 2x) and nothing else.
// ---------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void zero_stuff2_kernel(const float* __restrict__ src, int h, int w, int C, int H, int W,
                                                          long total, float* __restrict__ out) {
    const int c4n = C >> 2;
    for (long t = (long)blockIdx.x * 256 + threadIdx.x; t < total; t += (long)gridDim.x * 256) {
        const int c = (int)(t % c4n) * 4;
        long q = t / c4n;
        const int x = (int)(q % W);
        q /= W;
        const int y = (int)(q % H);
        const long n = q / H;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (!((x | y) & 1)) v = ld4(src + ((n * h + (y >> 1)) * w + (x >> 1)) * C + c);
        st4(out + t * 4, v);
    }
}

extern "C" int ssc_zero_stuff2(const float* src, int N, int h, int w, int C, int H, int W, float* out, void* stream) {
    if (N < 1 || h < 1 || w < 1 || C < 4 || (C & 3)) return -1;
    if ((H + 1) / 2 != h || (W + 1) / 2 != w) return -1;
    if ((int64_t)N * H * W * C > MAX_FLOATS) return -1;
    if (src == nullptr || out == nullptr || src == out) return -1;
    if (((uintptr_t)src | (uintptr_t)out) & 15) return -3;
    const long total = (long)N * H * W * (C / 4);
    hipLaunchKernelGGL(zero_stuff2_kernel, dim3(blocks_for(total)), dim3(256), 0, (hipStream_t)stream, src, h, w, C, H, W, total, out);
    return CHECK_LAUNCH();
}

// ---------------------------------------------------------------------------------------------------------------------------
// The backward of ssc_max_pool3s2 with its fused relu(a*r0 + b): g [N, OH, OW, C] -> dr0 [N, H, W, C].  Gather form: an input
// pixel looks at the up-to-four windows that hold it; a window hands its gradient to the FIRST of its taps in row-major order
// that attains its maximum (torch's rule and that of TF's NHWC kernel); taps in the padding never take part.  The window sums
// are added in the fixed order (oy, ox) ascending.  dr0 = that sum * a * (a*r0 + b > 0).
// ---------------------------------------------------------------------------------------------------------------------------
static __device__ __forceinline__ float4 relu_affine4(float4 a, float4 v, float4 b) {
    return make_float4(fmaxf(fmaf(a.x, v.x, b.x), 0.f), fmaxf(fmaf(a.y, v.y, b.y), 0.f), fmaxf(fmaf(a.z, v.z, b.z), 0.f),
                       fmaxf(fmaf(a.w, v.w, b.w), 0.f));
}

__global__ __launch_bounds__(256) void max_pool3s2_bwd_kernel(const float* __restrict__ g, const float* __restrict__ r0,
                                                              const float* __restrict__ ab, int H, int W, int C, int OH, int OW,
                                                              int py, int px, long total, float* __restrict__ dr0) {
    const int c4n = C >> 2;
    for (long t = (long)blockIdx.x * 256 + threadIdx.x; t < total; t += (long)gridDim.x * 256) {
        const int c = (int)(t % c4n) * 4;
        long q = t / c4n;
        const int x = (int)(q % W);
        q /= W;
        const int y = (int)(q % H);
        const long n = q / H;
        const float4 a = ld4(ab + c), b = ld4(ab + C + c);
        const float4 raw = ld4(r0 + t * 4);
        const float4 me = relu_affine4(a, raw, b);
        float4 sum = make_float4(0.f, 0.f, 0.f, 0.f);
        // the windows oy with oy*2 - py <= y <= oy*2 - py + 2
        const int oy_lo = (y + py - 2 + 1) >> 1, oy_hi = (y + py) >> 1;        // ceil((y + py - 2) / 2): y + py - 1 >= -1, >> floors
        const int ox_lo = (x + px - 2 + 1) >> 1, ox_hi = (x + px) >> 1;
        for (int oy = oy_lo < 0 ? 0 : oy_lo; oy <= oy_hi && oy < OH; ++oy) {
            for (int ox = ox_lo < 0 ? 0 : ox_lo; ox <= ox_hi && ox < OW; ++ox) {
                // is (y, x) the first tap of this window that attains its maximum?  It is unless a tap before it is >= me or a
                // tap behind it is > me.
                bool wx = true, wy = true, wz = true, ww = true;
                for (int ky = 0; ky < 3; ++ky) {
                    const int yy = oy * 2 - py + ky;
                    if (yy < 0 || yy >= H) continue;
                    for (int kx = 0; kx < 3; ++kx) {
                        const int xx = ox * 2 - px + kx;
                        if (xx < 0 || xx >= W || (yy == y && xx == x)) continue;
                        const float4 v = relu_affine4(a, ld4(r0 + ((n * H + yy) * W + xx) * C + c), b);
                        const bool before = yy < y || (yy == y && xx < x);
                        wx = wx && (before ? v.x < me.x : v.x <= me.x);
                        wy = wy && (before ? v.y < me.y : v.y <= me.y);
                        wz = wz && (before ? v.z < me.z : v.z <= me.z);
                        ww = ww && (before ? v.w < me.w : v.w <= me.w);
                    }
                }
                const float4 gg = ld4(g + ((n * OH + oy) * OW + ox) * C + c);
                sum.x += wx ? gg.x : 0.f;
                sum.y += wy ? gg.y : 0.f;
                sum.z += wz ? gg.z : 0.f;
                sum.w += ww ? gg.w : 0.f;
            }
        }
        float4 o;
        o.x = fmaf(a.x, raw.x, b.x) > 0.f ? sum.x * a.x : 0.f;
        o.y = fmaf(a.y, raw.y, b.y) > 0.f ? sum.y * a.y : 0.f;
        o.z = fmaf(a.z, raw.z, b.z) > 0.f ? sum.z * a.z : 0.f;
        o.w = fmaf(a.w, raw.w, b.w) > 0.f ? sum.w * a.w : 0.f;
        st4(dr0 + t * 4, o);
    }
}

extern "C" int ssc_max_pool3s2_bwd(const float* g, const float* r0, const float* ab, int N, int H, int W, int C, float* dr0,
                                   void* stream) {
    if (N < 1 || H < 1 || W < 1 || C < 4 || (C & 3)) return -1;
    if ((int64_t)N * H * W * C > MAX_FLOATS) return -1;
    if (g == nullptr || r0 == nullptr || ab == nullptr || dr0 == nullptr || dr0 == r0 || dr0 == g) return -1;
    if (((uintptr_t)g | (uintptr_t)r0 | (uintptr_t)ab | (uintptr_t)dr0) & 15) return -3;
    const int OH = (H + 1) / 2, OW = (W + 1) / 2;
    const int ph = (OH - 1) * 2 + 3 - H, pw = (OW - 1) * 2 + 3 - W;
    const long total = (long)N * H * W * (C / 4);
    hipLaunchKernelGGL(max_pool3s2_bwd_kernel, dim3(blocks_for(total)), dim3(256), 0, (hipStream_t)stream, g, r0, ab, H, W, C, OH, OW,
                       (ph > 0 ? ph : 0) / 2, (pw > 0 ? pw : 0) / 2, total, dr0);
    return CHECK_LAUNCH();
}
