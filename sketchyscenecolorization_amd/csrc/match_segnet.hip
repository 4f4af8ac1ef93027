// match_segnet.hip -- the two operations the matcher's SegNet backbone (Instance_Matching/segnet_model.py, is_intermediate) adds to
// the convs the library has: tf.nn.max_pool_with_argmax(2 x 2, stride 2) and _unpool_2d, the scatter that puts a pooled value
// back where its maximum was.  DESIGN.md section 8.12.
// The argmax is kept as a code 2 * dy + dx of one byte per pooled element instead of TF's flat int64 index
// ((2y + dy) * W + 2x + dx) * C + c: the window is known from the element's own position, only the tap within it is not.
// Each is the other's backward: the pool's is the unpool scatter of the gradient, the unpool's the gather by the same codes.
// Both are memory-bound: a thread owns four channels of one pooled pixel, 16-byte accesses along the channel axis, the four codes
// as one 4-byte access, grid-stride loops over at most 2048 workgroups, no LDS, no atomics, 64-bit element offsets.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "sketchycolor_hip.h"

#define CHECK_LAUNCH() ((int)hipGetLastError())

typedef unsigned char u8;

static inline unsigned blocks_for(long n) {
    long blocks = (n + 255) / 256;
    if (blocks < 1) blocks = 1;
    return (unsigned)(blocks > 2048 ? 2048 : blocks);
}

// ---------------------------------------------------------------------------------------------------------------------------
// out = max over the 2 x 2 window of relu(a * x + b) (of x itself without ab); code = 2 * dy + dx of the first tap in row-major
// order that attains it
// ---------------------------------------------------------------------------------------------------------------------------
// A later tap replaces the running maximum only when it is strictly greater: of equal taps the first one stays, which is TF's
// choice and the tie rule of ssc_max_pool3s2_bwd.
__device__ __forceinline__ void pool_take(float v, int k, float& m, unsigned& code) {
    if (v > m) {
        m = v;
        code = (unsigned)k;
    }
}

__global__ __launch_bounds__(256) void max_pool2_argmax_kernel(const float* __restrict__ x, const float* __restrict__ ab, int H, int W,
                                                               int C, long total, float* __restrict__ out, u8* __restrict__ code) {
    const int c4n = C >> 2, OH = H >> 1, OW = W >> 1;
    for (long t = (long)blockIdx.x * 256 + threadIdx.x; t < total; t += (long)gridDim.x * 256) {
        const int c = (int)(t % c4n) * 4;
        long q = t / c4n;
        const int ox = (int)(q % OW);
        q /= OW;
        const int oy = (int)(q % OH);
        const long n = q / OH;
        float4 a = make_float4(1.f, 1.f, 1.f, 1.f), b = make_float4(0.f, 0.f, 0.f, 0.f);
        if (ab != nullptr) {
            a = *reinterpret_cast<const float4*>(ab + c);
            b = *reinterpret_cast<const float4*>(ab + C + c);
        }
        const long row0 = ((n * H + 2 * oy) * W + 2 * ox) * C + c;      // tap (0, 0); (0, 1) is C further, the next row W * C
        float4 v[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            v[k] = *reinterpret_cast<const float4*>(x + row0 + (long)(k >> 1) * W * C + (long)(k & 1) * C);
            if (ab != nullptr) {
                v[k].x = fmaxf(fmaf(a.x, v[k].x, b.x), 0.f);
                v[k].y = fmaxf(fmaf(a.y, v[k].y, b.y), 0.f);
                v[k].z = fmaxf(fmaf(a.z, v[k].z, b.z), 0.f);
                v[k].w = fmaxf(fmaf(a.w, v[k].w, b.w), 0.f);
            }
        }
        float4 m = v[0];
        unsigned kx = 0, ky = 0, kz = 0, kw = 0;
#pragma unroll
        for (int k = 1; k < 4; ++k) {
            pool_take(v[k].x, k, m.x, kx);
            pool_take(v[k].y, k, m.y, ky);
            pool_take(v[k].z, k, m.z, kz);
            pool_take(v[k].w, k, m.w, kw);
        }
        *reinterpret_cast<float4*>(out + t * 4) = m;
        *reinterpret_cast<uchar4*>(code + t * 4) = make_uchar4((u8)kx, (u8)ky, (u8)kz, (u8)kw);
    }
}

extern "C" int ssc_max_pool2_argmax(const float* x, const float* ab, int N, int H, int W, int C, float* out, uint8_t* code,
                                    void* stream) {
    if (N < 1 || H < 2 || W < 2 || (H & 1) || (W & 1) || C < 4 || (C & 3)) return -1;
    if (x == nullptr || out == nullptr || code == nullptr || x == out) return -1;
    if ((int64_t)N * H * W * C > 0x7fffffffL * 4L) return -1;
    if ((((uintptr_t)x | (uintptr_t)out | (uintptr_t)ab) & 15) || ((uintptr_t)code & 3)) return -3;
    const long total = (long)N * (H / 2) * (W / 2) * (C / 4);
    hipLaunchKernelGGL(max_pool2_argmax_kernel, dim3(blocks_for(total)), dim3(256), 0, (hipStream_t)stream, x, ab, H, W, C, total,
                       out, code);
    return CHECK_LAUNCH();
}

// ---------------------------------------------------------------------------------------------------------------------------
// out[n, 2y + dy, 2x + dx, c] = x[n, y, x, c] where code[n, y, x, c] & 3 == 2 * dy + dx, 0 at the window's three other positions
// ---------------------------------------------------------------------------------------------------------------------------
// The thread of a pooled pixel writes all four positions of its window, so every output element is written exactly once.
__global__ __launch_bounds__(256) void unpool2_kernel(const float* __restrict__ x, const u8* __restrict__ code, int h, int w, int C,
                                                      long total, float* __restrict__ out) {
    const int c4n = C >> 2, W = w * 2;
    for (long t = (long)blockIdx.x * 256 + threadIdx.x; t < total; t += (long)gridDim.x * 256) {
        const int c = (int)(t % c4n) * 4;
        long q = t / c4n;
        const int px = (int)(q % w);
        q /= w;
        const int py = (int)(q % h);
        const long n = q / h;
        const float4 v = *reinterpret_cast<const float4*>(x + t * 4);
        const uchar4 k4 = *reinterpret_cast<const uchar4*>(code + t * 4);
        const int kx = k4.x & 3, ky = k4.y & 3, kz = k4.z & 3, kw = k4.w & 3;
        const long row0 = ((n * (2L * h) + 2 * py) * W + 2 * px) * C + c;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            float4 o;
            o.x = kx == k ? v.x : 0.f;
            o.y = ky == k ? v.y : 0.f;
            o.z = kz == k ? v.z : 0.f;
            o.w = kw == k ? v.w : 0.f;
            *reinterpret_cast<float4*>(out + row0 + (long)(k >> 1) * W * C + (long)(k & 1) * C) = o;
        }
    }
}

extern "C" int ssc_unpool2(const float* x, const uint8_t* code, int N, int h, int w, int C, float* out, void* stream) {
    if (N < 1 || h < 1 || w < 1 || C < 4 || (C & 3)) return -1;
    if (x == nullptr || code == nullptr || out == nullptr || x == out) return -1;
    if ((int64_t)N * h * w * C > 0x7fffffffL) return -1;      // the output is four times that
    if ((((uintptr_t)x | (uintptr_t)out) & 15) || ((uintptr_t)code & 3)) return -3;
    const long total = (long)N * h * w * (C / 4);
    hipLaunchKernelGGL(unpool2_kernel, dim3(blocks_for(total)), dim3(256), 0, (hipStream_t)stream, x, code, h, w, C, total, out);
    return CHECK_LAUNCH();
}
