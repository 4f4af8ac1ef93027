// match_attn.hip -- the matcher's word attention (Instance_Matching/RMI_model.py:202-217 with use_attn):
// a softmax over the word LSTM's outputs weighs the multimodal LSTM's outputs of every word.
//   ssc_attn_scores_fwd    the T weights from the L real rows of the word LSTM's outputs (a padded row's logit is the bias)
//   ssc_dev_scaled_add     y = (overwrite ? 0 : y) + s[k] * x with the scale read on the device: the weighted sum, one plane per
//                          step, and the injection of its gradient into every step of the backward
//   ssc_attn_plane_dots    dattn[t] = <dacc, H[t]> over a whole [R, cm] plane, float64 partial sums in two stages
//   ssc_attn_scores_bwd    the softmax rule, the gradients of the two variables and of the word LSTM's outputs
// All are memory-bound or tiny.  Every sum runs in a fixed order -- lanes by butterfly, wavefronts and workgroups one after the
// other through LDS or the workspace -- and nothing is added with an atomic: the same bits on every run.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "sketchycolor_hip.h"

#define CHECK_LAUNCH() ((int)hipGetLastError())
#define ATTN_MAX_T 64           // words a sentence may have: the logits of one sentence live in the LDS of one workgroup
#define DOTS_MAX_BLOCKS 512     // workgroups per plane of the first stage of ssc_attn_plane_dots

// ---------------------------------------------------------------------------------------------------------------------------
// attn = softmax over t < T of (t < L ? <hs[t], w> : 0) + b
// ---------------------------------------------------------------------------------------------------------------------------
// One workgroup of four wavefronts.  Wavefront v owns the rows v, v + 4, ..: lane l adds the columns l, l + 64, .. in order, the
// lanes are added by butterfly.  The rows >= L are never read.  Thread 0 then walks the T logits: the maximum, the exponentials,
// their sum (in double: the weights then add up to 1 within one rounding each) and the quotients.
__global__ __launch_bounds__(256) void attn_scores_fwd_kernel(const float* __restrict__ hs, int ld, const float* __restrict__ w,
                                                              const float* __restrict__ b, int C, int L, int T,
                                                              float* __restrict__ attn) {
    __shared__ float logit[ATTN_MAX_T];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const float bias = b[0];
    for (int t = wave; t < T; t += 4) {
        float s = 0.f;
        if (t < L) {        // the same for the whole wavefront
            const float* row = hs + (long)t * ld;
            for (int c = lane; c < C; c += 64) s = fmaf(row[c], w[c], s);
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
        }
        if (lane == 0) logit[t] = s + bias;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        float m = logit[0];
        for (int t = 1; t < T; ++t) m = fmaxf(m, logit[t]);
        double sum = 0.0;
        for (int t = 0; t < T; ++t) {
            const float e = expf(logit[t] - m);
            logit[t] = e;
            sum += (double)e;
        }
        for (int t = 0; t < T; ++t) attn[t] = (float)((double)logit[t] / sum);
    }
}

extern "C" int ssc_attn_scores_fwd(const float* hs, int ld, const float* w, const float* b, int C, int L, int T, float* attn,
                                   void* stream) {
    if (T < 1 || T > ATTN_MAX_T || L < 1 || L > T || C < 1 || ld < C) return -1;
    if (hs == nullptr || w == nullptr || b == nullptr || attn == nullptr) return -1;
    hipLaunchKernelGGL(attn_scores_fwd_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, hs, ld, w, b, C, L, T, attn);
    return CHECK_LAUNCH();
}

// ---------------------------------------------------------------------------------------------------------------------------
// y = (overwrite ? 0 : y) + s[k] * x
// ---------------------------------------------------------------------------------------------------------------------------
// vec: both pointers on 16 bytes -- a thread owns four neighbouring floats, the n % 4 last ones go to the first workgroup.
__global__ __launch_bounds__(256) void dev_scaled_add_kernel(float* __restrict__ y, const float* __restrict__ x,
                                                             const float* __restrict__ s, int k, long n, int overwrite, int vec) {
    const float a = s[k];
    const long first = (long)blockIdx.x * 256 + threadIdx.x, step = (long)gridDim.x * 256;
    if (vec) {
        const long n4 = n >> 2;
        for (long i = first; i < n4; i += step) {
            const float4 v = reinterpret_cast<const float4*>(x)[i];
            float4 o = overwrite ? make_float4(0.f, 0.f, 0.f, 0.f) : reinterpret_cast<const float4*>(y)[i];
            o.x = fmaf(a, v.x, o.x);
            o.y = fmaf(a, v.y, o.y);
            o.z = fmaf(a, v.z, o.z);
            o.w = fmaf(a, v.w, o.w);
            reinterpret_cast<float4*>(y)[i] = o;
        }
        const long i = (n4 << 2) + first;
        if (blockIdx.x == 0 && i < n) y[i] = fmaf(a, x[i], overwrite ? 0.f : y[i]);
    } else {
        for (long i = first; i < n; i += step) y[i] = fmaf(a, x[i], overwrite ? 0.f : y[i]);
    }
}

extern "C" int ssc_dev_scaled_add(float* y, const float* x, const float* s, int ns, int k, int64_t n, int overwrite, void* stream) {
    if (n < 1 || ns < 1 || k < 0 || k >= ns) return -1;
    if (y == nullptr || x == nullptr || s == nullptr) return -1;
    const int vec = (((uintptr_t)y | (uintptr_t)x) & 15) == 0;
    const int64_t items = vec ? (n + 3) / 4 : n;
    int64_t blocks = (items + 255) / 256;
    if (blocks > 2048) blocks = 2048;
    hipLaunchKernelGGL(dev_scaled_add_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, y, x, s, k, (long)n,
                       overwrite != 0, vec);
    return CHECK_LAUNCH();
}

// ---------------------------------------------------------------------------------------------------------------------------
// dattn[t] = sum over i < n of dacc[i] * H[t * stride + i]
// ---------------------------------------------------------------------------------------------------------------------------
// First stage: workgroup (b, t) adds its threads' elements of plane t -- a product of two floats is exact in double -- thread by
// thread in order, the lanes by butterfly, the four wavefronts in order: part[t][b].  Second stage: one workgroup per plane adds
// part[t][0 ..] (thread j the entries j, j + 256, .., then pairwise through LDS) and rounds once to float.
__global__ __launch_bounds__(256) void attn_plane_dots_kernel(const float* __restrict__ dacc, const float* __restrict__ H, long stride,
                                                              long n, int vec, double* __restrict__ part) {
    __shared__ double sh[4];
    const float* __restrict__ h = H + (long)blockIdx.y * stride;
    const long first = (long)blockIdx.x * 256 + threadIdx.x, step = (long)gridDim.x * 256;
    double s = 0.0;
    if (vec) {
        const long n4 = n >> 2;
        for (long i = first; i < n4; i += step) {
            const float4 a = reinterpret_cast<const float4*>(dacc)[i];
            const float4 v = reinterpret_cast<const float4*>(h)[i];
            s += (double)a.x * (double)v.x;
            s += (double)a.y * (double)v.y;
            s += (double)a.z * (double)v.z;
            s += (double)a.w * (double)v.w;
        }
        const long i = (n4 << 2) + first;
        if (blockIdx.x == 0 && i < n) s += (double)dacc[i] * (double)h[i];
    } else {
        for (long i = first; i < n; i += step) s += (double)dacc[i] * (double)h[i];
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) part[(long)blockIdx.y * gridDim.x + blockIdx.x] = ((sh[0] + sh[1]) + sh[2]) + sh[3];
}

__global__ __launch_bounds__(256) void attn_plane_dots_finish_kernel(const double* __restrict__ part, int blocks,
                                                                     float* __restrict__ dattn) {
    __shared__ double sl[256];
    const double* __restrict__ p = part + (long)blockIdx.x * blocks;
    double s = 0.0;
    for (int j = threadIdx.x; j < blocks; j += 256) s += p[j];
    sl[threadIdx.x] = s;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) sl[threadIdx.x] += sl[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) dattn[blockIdx.x] = (float)sl[0];
}

// workgroups per plane: a thread of the first stage adds about four float4 of either operand
static inline int dots_blocks(int64_t n) {
    int64_t b = (n + 4095) / 4096;
    return (int)(b < 1 ? 1 : (b > DOTS_MAX_BLOCKS ? DOTS_MAX_BLOCKS : b));
}

extern "C" int ssc_attn_plane_dots(const float* dacc, const float* H, int64_t stride, int64_t n, int L, float* dattn, float* ws,
                                   int64_t ws_bytes, void* stream) {
    if (n < 1 || L < 1 || L > ATTN_MAX_T || stride < n) return -1;
    if (dacc == nullptr || H == nullptr || dattn == nullptr || ws == nullptr) return -1;
    const int blocks = dots_blocks(n);
    if (ws_bytes < (int64_t)L * blocks * (int64_t)sizeof(double)) return -1;
    if ((uintptr_t)ws & 7) return -3;
    const int vec = (((uintptr_t)dacc | (uintptr_t)H) & 15) == 0 && (stride & 3) == 0;
    hipLaunchKernelGGL(attn_plane_dots_kernel, dim3((unsigned)blocks, (unsigned)L), dim3(256), 0, (hipStream_t)stream, dacc, H,
                       (long)stride, (long)n, vec, (double*)ws);
    int rc = CHECK_LAUNCH();
    if (rc != 0) return rc;
    hipLaunchKernelGGL(attn_plane_dots_finish_kernel, dim3((unsigned)L), dim3(256), 0, (hipStream_t)stream, (const double*)ws, blocks,
                       dattn);
    return CHECK_LAUNCH();
}

// ---------------------------------------------------------------------------------------------------------------------------
// the backward of ssc_attn_scores_fwd
// ---------------------------------------------------------------------------------------------------------------------------
// One workgroup.  Thread 0 walks the softmax rule in index order: dot = sum over s < L of attn[s] * dattn[s] (in double),
// dlogit[t] = attn[t] * ((t < L ? dattn[t] : 0) - dot), db = their sum in index order.  Then thread c owns the columns c, c + 256, ..:
// dw[c] = sum over t < L of dlogit[t] * hs[t][c] in order, and dhs[t][c] += dlogit[t] * w[c].  The rows >= L are never read.
__global__ __launch_bounds__(256) void attn_scores_bwd_kernel(const float* __restrict__ attn, const float* __restrict__ dattn,
                                                              const float* __restrict__ hs, int ld, const float* __restrict__ w, int C,
                                                              int L, int T, float* __restrict__ dlogit, float* __restrict__ dw,
                                                              float* __restrict__ db, float* __restrict__ dhs, int ldd) {
    __shared__ float dl[ATTN_MAX_T];
    if (threadIdx.x == 0) {
// every product here has a rounding of its own: contracted into the sum below it, db would not be the sum of the stored values
#pragma clang fp contract(off)
        double dot = 0.0;
        for (int s = 0; s < L; ++s) dot += (double)attn[s] * (double)dattn[s];
        float sum = 0.f;
        for (int t = 0; t < T; ++t) {
            const float d = attn[t] * (float)((t < L ? (double)dattn[t] : 0.0) - dot);
            dl[t] = d;
            dlogit[t] = d;
            sum += d;
        }
        db[0] = sum;
    }
    __syncthreads();
    for (int c = threadIdx.x; c < C; c += 256) {
        const float wc = w[c];
        float s = 0.f;
        for (int t = 0; t < L; ++t) {
            s = fmaf(dl[t], hs[(long)t * ld + c], s);
            dhs[(long)t * ldd + c] = fmaf(dl[t], wc, dhs[(long)t * ldd + c]);
        }
        dw[c] = s;
    }
}

extern "C" int ssc_attn_scores_bwd(const float* attn, const float* dattn, const float* hs, int ld, const float* w, int C, int L, int T,
                                   float* dlogit, float* dw, float* db, float* dhs, int ldd, void* stream) {
    if (T < 1 || T > ATTN_MAX_T || L < 1 || L > T || C < 1 || ld < C || ldd < C) return -1;
    if (attn == nullptr || dattn == nullptr || hs == nullptr || w == nullptr || dlogit == nullptr || dw == nullptr || db == nullptr ||
        dhs == nullptr)
        return -1;
    hipLaunchKernelGGL(attn_scores_bwd_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, attn, dattn, hs, ld, w, C, L, T, dlogit, dw,
                       db, dhs, ldd);
    return CHECK_LAUNCH();
}
