// bg_io.hip -- the Background module's uint8 boundary (bg_colorization_main.py:30-39, 100-113, 765-768, 785-786, 861-871):
// one streaming pass from the loader's uint8 arrays -- or from device-resident scene caches, gathered by entry -- to everything
// a train step reads, and one from the generator's image back to uint8 with the foreground pasted over it.  All are pure HBM
// streaming: a thread owns 4 pixels, so that the 3-byte pixels of a uint8 source are three whole dwords and every float row is
// written with 16-byte stores.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "sketchycolor_hip.h"
#include "bg_u8.h"

#define CHECK_LAUNCH() ((int)hipGetLastError())

// convert_image_dtype + preprocess: u8 / 255 * 2 - 1, every operation rounded to fp32 on its own.  The __f*_rn intrinsics are
// inline functions compiled with contraction allowed, and the compiler does fuse them: plain operators with contraction
// switched off for the function instead (the build keeps the correctly rounded fp32 division, no fast-math).
__device__ __forceinline__ float u8_to_unit(unsigned v) {
#pragma clang fp contract(off)
    const float q = (float)v / 255.f;
    const float d = q * 2.f;
    return d - 1.f;
}

// state[0]: high 32 bits = workgroups that have added, low 32 bits = labels != 0 so far (zeroed by the launcher on the stream).
// The workgroup whose add completes the ticket count holds the total in the value the atomic returned: an integer sum, exact
// and the same for every grid.
__global__ __launch_bounds__(256) void bg_stage_u8_kernel(const unsigned char* __restrict__ fg,
                                                           const unsigned char* __restrict__ bg,
                                                           const int* __restrict__ labels, long M,
                                                           float* __restrict__ inputs, float* __restrict__ targets,
                                                           float* __restrict__ xd, float* __restrict__ count,
                                                           unsigned long long* __restrict__ state) {
    __shared__ unsigned sh[4];
    const long groups = (M + 3) >> 2;
    unsigned nz = 0;
    for (long g = (long)blockIdx.x * 256 + threadIdx.x; g < groups; g += (long)gridDim.x * 256) {
        const long r0 = g * 4;
        if (r0 + 4 <= M) {
            unsigned a[3], b[3];
            const unsigned* pa = reinterpret_cast<const unsigned*>(fg + r0 * 3);
            const unsigned* pb = reinterpret_cast<const unsigned*>(bg + r0 * 3);
#pragma unroll
            for (int k = 0; k < 3; ++k) { a[k] = pa[k]; b[k] = pb[k]; }
            const int4 l = *reinterpret_cast<const int4*>(labels + r0);
            nz += (l.x != 0) + (l.y != 0) + (l.z != 0) + (l.w != 0);
            float x[12], y[12];
#pragma unroll
            for (int i = 0; i < 12; ++i) { x[i] = u8_to_unit(byte_of(a, i)); y[i] = u8_to_unit(byte_of(b, i)); }
            float4* pi = reinterpret_cast<float4*>(inputs + r0 * 3);
            float4* pt = reinterpret_cast<float4*>(targets + r0 * 3);
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                pi[k] = make_float4(x[4 * k], x[4 * k + 1], x[4 * k + 2], x[4 * k + 3]);
                pt[k] = make_float4(y[4 * k], y[4 * k + 1], y[4 * k + 2], y[4 * k + 3]);
            }
            float4* px = reinterpret_cast<float4*>(xd + r0 * 8);
#pragma unroll
            for (int p = 0; p < 4; ++p) {
                px[2 * p] = make_float4(x[3 * p], x[3 * p + 1], x[3 * p + 2], y[3 * p]);
                px[2 * p + 1] = make_float4(y[3 * p + 1], y[3 * p + 2], 0.f, 0.f);
            }
        } else {        // the last, short group
            for (long r = r0; r < M; ++r) {
                nz += labels[r] != 0;
                float x[3], y[3];
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    x[c] = u8_to_unit(fg[r * 3 + c]);
                    y[c] = u8_to_unit(bg[r * 3 + c]);
                    inputs[r * 3 + c] = x[c];
                    targets[r * 3 + c] = y[c];
                }
                float4* px = reinterpret_cast<float4*>(xd + r * 8);
                px[0] = make_float4(x[0], x[1], x[2], y[0]);
                px[1] = make_float4(y[1], y[2], 0.f, 0.f);
            }
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) nz += __shfl_down(nz, o, 64);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = nz;
    __syncthreads();
    if (threadIdx.x == 0) {
        const unsigned long long mine = (1ull << 32) | (unsigned long long)(sh[0] + sh[1] + sh[2] + sh[3]);
        const unsigned long long seen = atomicAdd(state, mine) + mine;
        if ((unsigned)(seen >> 32) == gridDim.x) count[0] = (float)(unsigned)(seen & 0xffffffffull);
    }
}

extern "C" int ssc_bg_stage_u8(const uint8_t* fg, const uint8_t* bg, const int32_t* labels, int64_t M, float* inputs,
                               float* targets, float* xd_real, float* count, void* workspace, int64_t workspace_bytes,
                               void* stream) {
    if (M < 1 || M > (1 << 24)) return -1;         // the count is handed on as a float: exact up to 2^24 pixels
    if (workspace_bytes < 8 || ((uintptr_t)workspace & 7)) return -2;
    if ((((uintptr_t)fg | (uintptr_t)bg) & 3) || (((uintptr_t)labels | (uintptr_t)inputs | (uintptr_t)targets | (uintptr_t)xd_real) & 15))
        return -3;
    if (hipMemsetAsync(workspace, 0, 8, (hipStream_t)stream) != hipSuccess) return (int)hipGetLastError();
    long blocks = ((M + 3) / 4 + 255) / 256;
    if (blocks > 2048) blocks = 2048;
    hipLaunchKernelGGL(bg_stage_u8_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, fg, bg, labels, (long)M,
                       inputs, targets, xd_real, count, (unsigned long long*)workspace);
    return CHECK_LAUNCH();
}

// The same pass fed from device-resident scene caches instead of a batch uploaded for the step: sample n reads entry slot[n][0]
// of fg_cache, slot[n][1] of bg_cache and slot[n][2] of seg_cache (the raw red channel of the segment png), and writes the
// labels too (image_processing.py:14-25: 128 -> 1, 255 -> 2, anything else 0).  recolor[n] = {enable, sky rgb, ground rgb, 0}
// replaces the background's sky / ground pixels (data_preparation/bg_data_generation.py:145-147 on the segment map of :121-125).
// A group of 4 pixels never straddles two samples.  An entry starts entry * P * 3 bytes into its cache and sample n's float rows
// n * P * 3 floats into theirs: neither is aligned when P is no multiple of 4, so a group takes the dword loads and 16-byte
// stores only where its own addresses allow them and goes byte by byte, float by float otherwise (as the short last group of
// a sample does).  A slot outside its cache reads nothing: NaN images, labels 0 and, through the state word, a NaN count.
// state[0]: bits 48.. = workgroups that have added, bits 32..47 = workgroups that met a bad slot, low 32 bits = labels != 0.
__global__ __launch_bounds__(256) void bg_stage_cached_u8_kernel(
    const unsigned char* __restrict__ fg_cache, int S_fg, const unsigned char* __restrict__ bg_cache, int S_bg,
    const unsigned char* __restrict__ seg_cache, int S_seg, const int* __restrict__ slot,
    const unsigned char* __restrict__ recolor, int N, int P, float* __restrict__ inputs, float* __restrict__ targets,
    float* __restrict__ xd, int* __restrict__ labels, float* __restrict__ count, unsigned long long* __restrict__ state) {
    __shared__ unsigned sh[4];
    const unsigned gps = ((unsigned)P + 3u) >> 2;       // groups per sample
    const unsigned groups = gps * (unsigned)N;          // <= N * P <= 2^24
    unsigned nz = 0;
    int bad = 0;
    for (unsigned g = blockIdx.x * 256u + threadIdx.x; g < groups; g += gridDim.x * 256u) {
        const unsigned n = g / gps;
        const int r0 = (int)(g - n * gps) * 4;
        const int cnt = P - r0 < 4 ? P - r0 : 4;
        const long o = (long)n * P + r0;                // the group's first pixel in the outputs
        const int sf = slot[n * 3], sb = slot[n * 3 + 1], ss = slot[n * 3 + 2];
        float x[12], y[12];
        int lab[4];
        bool fast = cnt == 4 && (o & 3) == 0;
        if (sf < 0 || sf >= S_fg || sb < 0 || sb >= S_bg || ss < 0 || ss >= S_seg) {
            bad = 1;
            fast = false;
#pragma unroll
            for (int i = 0; i < 12; ++i) x[i] = y[i] = __builtin_nanf("");
#pragma unroll
            for (int p = 0; p < 4; ++p) lab[p] = 0;
        } else {
            const unsigned char* pf = fg_cache + ((long)sf * P + r0) * 3;
            const unsigned char* pb = bg_cache + ((long)sb * P + r0) * 3;
            const unsigned char* ps = seg_cache + ((long)ss * P + r0);
            unsigned a[12], b[12], s[4];
            if (fast && (((uintptr_t)pf | (uintptr_t)pb | (uintptr_t)ps) & 3) == 0) {
                unsigned wa[3], wb[3];
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    wa[k] = reinterpret_cast<const unsigned*>(pf)[k];
                    wb[k] = reinterpret_cast<const unsigned*>(pb)[k];
                }
                const unsigned ws = *reinterpret_cast<const unsigned*>(ps);
#pragma unroll
                for (int i = 0; i < 12; ++i) { a[i] = byte_of(wa, i); b[i] = byte_of(wb, i); }
#pragma unroll
                for (int p = 0; p < 4; ++p) s[p] = (ws >> (8 * p)) & 0xffu;
            } else {
#pragma unroll
                for (int p = 0; p < 4; ++p) {
                    const bool in = p < cnt;
                    s[p] = in ? ps[p] : 0u;
#pragma unroll
                    for (int c = 0; c < 3; ++c) {
                        a[3 * p + c] = in ? pf[3 * p + c] : 0u;
                        b[3 * p + c] = in ? pb[3 * p + c] : 0u;
                    }
                }
            }
            unsigned rc[2] = {0u, 0u};
            if (recolor != nullptr) {
                const uint2 w = *reinterpret_cast<const uint2*>(recolor + (long)n * 8);
                rc[0] = w.x;
                rc[1] = w.y;
            }
            const bool paint = (rc[0] & 0xffu) != 0;
#pragma unroll
            for (int p = 0; p < 4; ++p) {
                lab[p] = s[p] == 128u ? 1 : (s[p] == 255u ? 2 : 0);
                nz += lab[p] != 0;
                if (paint && lab[p] != 0) {
                    // bytes 1..3 of the record are the sky colour, 4..6 the ground colour
                    const unsigned col = lab[p] == 1 ? rc[0] >> 8 : rc[1];
#pragma unroll
                    for (int c = 0; c < 3; ++c) b[3 * p + c] = (col >> (8 * c)) & 0xffu;
                }
            }
#pragma unroll
            for (int i = 0; i < 12; ++i) { x[i] = u8_to_unit(a[i]); y[i] = u8_to_unit(b[i]); }
        }
        if (fast) {
            float4* pi = reinterpret_cast<float4*>(inputs + o * 3);
            float4* pt = reinterpret_cast<float4*>(targets + o * 3);
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                pi[k] = make_float4(x[4 * k], x[4 * k + 1], x[4 * k + 2], x[4 * k + 3]);
                pt[k] = make_float4(y[4 * k], y[4 * k + 1], y[4 * k + 2], y[4 * k + 3]);
            }
            *reinterpret_cast<int4*>(labels + o) = make_int4(lab[0], lab[1], lab[2], lab[3]);
        }
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            if (p < cnt) {
                if (!fast) {
#pragma unroll
                    for (int c = 0; c < 3; ++c) {
                        inputs[(o + p) * 3 + c] = x[3 * p + c];
                        targets[(o + p) * 3 + c] = y[3 * p + c];
                    }
                    labels[o + p] = lab[p];
                }
                float4* px = reinterpret_cast<float4*>(xd + (o + p) * 8);      // a pixel's 8 floats: 32-byte aligned always
                px[0] = make_float4(x[3 * p], x[3 * p + 1], x[3 * p + 2], y[3 * p]);
                px[1] = make_float4(y[3 * p + 1], y[3 * p + 2], 0.f, 0.f);
            }
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) nz += __shfl_down(nz, o, 64);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = nz;
    const int any_bad = __syncthreads_or(bad);
    if (threadIdx.x == 0) {
        const unsigned long long mine = (1ull << 48) | ((unsigned long long)(any_bad != 0) << 32) |
                                        (unsigned long long)(sh[0] + sh[1] + sh[2] + sh[3]);
        const unsigned long long seen = atomicAdd(state, mine) + mine;
        if ((unsigned)(seen >> 48) == gridDim.x)
            count[0] = ((seen >> 32) & 0xffffull) != 0 ? __builtin_nanf("") : (float)(unsigned)(seen & 0xffffffffull);
    }
}

extern "C" int ssc_bg_stage_cached_u8(const uint8_t* fg_cache, int64_t S_fg, const uint8_t* bg_cache, int64_t S_bg,
                                      const uint8_t* seg_cache, int64_t S_seg, const int32_t* slot, const uint8_t* recolor,
                                      int64_t N, int64_t P, float* inputs, float* targets, float* xd_real, int32_t* labels,
                                      float* count, void* workspace, int64_t workspace_bytes, void* stream) {
    const int64_t lim = 1 << 24;                   // the count is handed on as a float: exact up to 2^24 pixels
    if (N < 1 || P < 1 || N > lim || P > lim || N * P > lim) return -1;
    if (S_fg < 1 || S_bg < 1 || S_seg < 1 || S_fg > INT32_MAX || S_bg > INT32_MAX || S_seg > INT32_MAX) return -1;
    if (workspace_bytes < 8 || ((uintptr_t)workspace & 7)) return -2;
    if ((((uintptr_t)fg_cache | (uintptr_t)bg_cache | (uintptr_t)seg_cache | (uintptr_t)slot) & 3) || ((uintptr_t)recolor & 7) ||
        (((uintptr_t)labels | (uintptr_t)inputs | (uintptr_t)targets | (uintptr_t)xd_real) & 15))
        return -3;
    if (hipMemsetAsync(workspace, 0, 8, (hipStream_t)stream) != hipSuccess) return (int)hipGetLastError();
    long blocks = (N * ((P + 3) / 4) + 255) / 256;
    if (blocks > 2048) blocks = 2048;
    hipLaunchKernelGGL(bg_stage_cached_u8_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, fg_cache, (int)S_fg,
                       bg_cache, (int)S_bg, seg_cache, (int)S_seg, slot, recolor, (int)N, (int)P, inputs, targets, xd_real, labels,
                       count, (unsigned long long*)workspace);
    return CHECK_LAUNCH();
}

// LOADS: 4 = rows of 4 floats, one 16-byte load per pixel; 3 = dense rows of 3 floats on a 16-byte aligned image, the 12 floats
// of a thread's 4 pixels as three 16-byte loads; 0 = any other row length or alignment, one float at a time.
template <int LOADS>
__global__ __launch_bounds__(256) void bg_finish_u8_kernel(const float* __restrict__ img, int ldc,
                                                            const unsigned char* __restrict__ fg,
                                                            const unsigned char* __restrict__ mask, long M,
                                                            unsigned char* __restrict__ out) {
    const long groups = (M + 3) >> 2;
    for (long g = (long)blockIdx.x * 256 + threadIdx.x; g < groups; g += (long)gridDim.x * 256) {
        const long r0 = g * 4;
        if (r0 + 4 <= M) {
            unsigned v[12];
            if (LOADS == 4) {
#pragma unroll
                for (int p = 0; p < 4; ++p) {
                    const float4 t = *reinterpret_cast<const float4*>(img + (r0 + p) * 4);
                    v[3 * p] = unit_to_u8(t.x); v[3 * p + 1] = unit_to_u8(t.y); v[3 * p + 2] = unit_to_u8(t.z);
                }
            } else if (LOADS == 3) {
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    const float4 t = *reinterpret_cast<const float4*>(img + r0 * 3 + 4 * k);
                    v[4 * k] = unit_to_u8(t.x); v[4 * k + 1] = unit_to_u8(t.y);
                    v[4 * k + 2] = unit_to_u8(t.z); v[4 * k + 3] = unit_to_u8(t.w);
                }
            } else {
#pragma unroll
                for (int p = 0; p < 4; ++p)
#pragma unroll
                    for (int c = 0; c < 3; ++c) v[3 * p + c] = unit_to_u8(img[(r0 + p) * ldc + c]);
            }
            if (mask != nullptr) {
                const unsigned m = *reinterpret_cast<const unsigned*>(mask + r0);
                if ((m & 0xffu) == 0 || (m & 0xff00u) == 0 || (m & 0xff0000u) == 0 || (m & 0xff000000u) == 0) {
                    unsigned f[3];
                    const unsigned* pf = reinterpret_cast<const unsigned*>(fg + r0 * 3);
#pragma unroll
                    for (int k = 0; k < 3; ++k) f[k] = pf[k];
#pragma unroll
                    for (int p = 0; p < 4; ++p)
                        if (((m >> (8 * p)) & 0xffu) == 0) {
#pragma unroll
                            for (int c = 0; c < 3; ++c) v[3 * p + c] = byte_of(f, 3 * p + c);
                        }
                }
            }
            unsigned* po = reinterpret_cast<unsigned*>(out + r0 * 3);
#pragma unroll
            for (int k = 0; k < 3; ++k) po[k] = v[4 * k] | (v[4 * k + 1] << 8) | (v[4 * k + 2] << 16) | (v[4 * k + 3] << 24);
        } else {
            for (long r = r0; r < M; ++r) {
                const bool paste = mask != nullptr && mask[r] == 0;
#pragma unroll
                for (int c = 0; c < 3; ++c)
                    out[r * 3 + c] = paste ? fg[r * 3 + c] : (unsigned char)unit_to_u8(img[r * ldc + c]);
            }
        }
    }
}

extern "C" int ssc_bg_finish_u8(const float* img, int ldc, const uint8_t* fg, const uint8_t* mask, int64_t M, uint8_t* out,
                                void* stream) {
    if (M < 1 || ldc < 3) return -1;
    if (mask != nullptr && fg == nullptr) return -1;
    if ((((uintptr_t)out | (uintptr_t)fg | (uintptr_t)mask) & 3) || (ldc == 4 && ((uintptr_t)img & 15))) return -3;
    long blocks = ((M + 3) / 4 + 255) / 256;
    if (blocks > 2048) blocks = 2048;
    if (ldc == 4)
        hipLaunchKernelGGL(bg_finish_u8_kernel<4>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, img, ldc, fg,
                           mask, (long)M, out);
    else if (ldc == 3 && ((uintptr_t)img & 15) == 0)
        hipLaunchKernelGGL(bg_finish_u8_kernel<3>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, img, ldc, fg,
                           mask, (long)M, out);
    else
        hipLaunchKernelGGL(bg_finish_u8_kernel<0>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, img, ldc, fg,
                           mask, (long)M, out);
    return CHECK_LAUNCH();
}
