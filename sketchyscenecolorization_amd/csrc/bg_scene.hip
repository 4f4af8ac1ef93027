// bg_scene.hip -- the background of a user scene, finished on the device as the scene pipeline finishes it (Pipeline_utils/
// bg_utils.py:96-166, 215-224, 290-319): the crop of the previous result by the instance mask, the composition of the generator's
// image with the cropped instances and the sketch strokes, and the sky gradient in HSV.  All images are uint8 [H,W,3], the
// instance mask ("inner") uint8 [H,W] = 0 for background, k + 1 for instance k.  Streaming kernels: a thread owns 4 pixels (three
// dwords of an image, one of the mask) and the last, short group goes byte by byte.  The gradient is float64 with contraction
// off for the whole file: every operation below is one NumPy operation of skimage's rgb2hsv / hsv2rgb.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "sketchycolor_hip.h"
#include "bg_u8.h"

#pragma clang fp contract(off)

#define CHECK_LAUNCH() ((int)hipGetLastError())

typedef unsigned char u8;

static inline unsigned blocks_for(long M) {
    long blocks = ((M + 3) / 4 + 255) / 256;
    return (unsigned)(blocks > 2048 ? 2048 : blocks);
}

// ---------------------------------------------------------------------------------------------------------------------------
// crop: white where inner == 0, else the previous image
// ---------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void bg_scene_crop_kernel(const u8* __restrict__ prev, const u8* __restrict__ inner, int M,
                                                            u8* __restrict__ out) {
    const int groups = (M + 3) >> 2;
    for (int g = blockIdx.x * 256 + threadIdx.x; g < groups; g += gridDim.x * 256) {
        const int r0 = g * 4;
        if (r0 + 4 <= M) {
            const unsigned m = *reinterpret_cast<const unsigned*>(inner + r0);
            unsigned a[3], v[12];
            const unsigned* pa = reinterpret_cast<const unsigned*>(prev + r0 * 3);
#pragma unroll
            for (int k = 0; k < 3; ++k) a[k] = pa[k];
#pragma unroll
            for (int p = 0; p < 4; ++p)
#pragma unroll
                for (int c = 0; c < 3; ++c) v[3 * p + c] = ((m >> (8 * p)) & 0xffu) != 0 ? byte_of(a, 3 * p + c) : 255u;
            unsigned* po = reinterpret_cast<unsigned*>(out + r0 * 3);
#pragma unroll
            for (int k = 0; k < 3; ++k) po[k] = v[4 * k] | (v[4 * k + 1] << 8) | (v[4 * k + 2] << 16) | (v[4 * k + 3] << 24);
        } else {
            for (int r = r0; r < M; ++r)
#pragma unroll
                for (int c = 0; c < 3; ++c) out[r * 3 + c] = inner[r] != 0 ? prev[r * 3 + c] : (u8)255;
        }
    }
}

extern "C" int ssc_bg_scene_crop_u8(const uint8_t* prev, const uint8_t* inner, int64_t M, uint8_t* fg_out, void* stream) {
    if (M < 1 || M > (1 << 24)) return -1;
    if (prev == nullptr || inner == nullptr || fg_out == nullptr) return -1;
    if (((uintptr_t)prev | (uintptr_t)inner | (uintptr_t)fg_out) & 3) return -3;
    hipLaunchKernelGGL(bg_scene_crop_kernel, dim3(blocks_for(M)), dim3(256), 0, (hipStream_t)stream, prev, inner, (int)M, fg_out);
    return CHECK_LAUNCH();
}

// ---------------------------------------------------------------------------------------------------------------------------
// compose: the generator's image under bg_finish_u8's cast, the cropped instances over it, the sketch strokes over both
// ---------------------------------------------------------------------------------------------------------------------------
// The strokes are the sketch moved one pixel down and right: moved[i][j] = sketch[i-1][j-1] for i, j >= 1, and row 0 and column 0
// keep sketch[i][j].  A pixel is drawn where the moved sketch's red byte is 0 and grass[inner] is 0.  OVERLAY (the second pass,
// behind the gradient): out is read, only the drawn pixels change, and img, fg and fg_marked are not touched.
// LOADS as in bg_finish_u8_kernel: 4 = rows of 4 floats on a 16-byte aligned base, 3 = dense rows of 3 floats on one, 0 = the rest.
template <int LOADS, bool OVERLAY>
__global__ __launch_bounds__(256) void bg_scene_compose_kernel(const float* __restrict__ img, int ldc, const u8* __restrict__ fg,
                                                               const u8* __restrict__ inner, const u8* __restrict__ grass,
                                                               const u8* __restrict__ sketch, int W, int M, u8* out,
                                                               u8* __restrict__ fg_marked) {
    __shared__ u8 gr[256];
    gr[threadIdx.x] = grass[threadIdx.x];
    __syncthreads();
    const int groups = (M + 3) >> 2;
    for (int g = blockIdx.x * 256 + threadIdx.x; g < groups; g += gridDim.x * 256) {
        const int r0 = g * 4;
        const int cnt = M - r0 < 4 ? M - r0 : 4;
        const bool whole = cnt == 4;
        unsigned v[12], f[12], m[4];
        if (whole) {
            const unsigned w = *reinterpret_cast<const unsigned*>(inner + r0);
#pragma unroll
            for (int p = 0; p < 4; ++p) m[p] = (w >> (8 * p)) & 0xffu;
        } else {
#pragma unroll
            for (int p = 0; p < 4; ++p) m[p] = p < cnt ? inner[r0 + p] : 0u;
        }
        // the strokes first: in the overlay pass a group without one is left alone
        int i = r0 / W, j = r0 - i * W;
        unsigned stroke[4];
        bool drawn[4], any = false;
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            drawn[p] = false;
            stroke[p] = 0u;
            if (p < cnt) {
                const int src = (i >= 1 && j >= 1 ? r0 + p - W - 1 : r0 + p) * 3;
                if (sketch[src] == 0 && gr[m[p]] == 0) {
                    drawn[p] = any = true;
                    stroke[p] = ((unsigned)sketch[src + 1] << 8) | ((unsigned)sketch[src + 2] << 16);
                }
            }
            if (++j == W) { j = 0; ++i; }
        }
        if (OVERLAY) {
            if (!any) continue;
            if (whole) {
                unsigned a[3];
                const unsigned* pa = reinterpret_cast<const unsigned*>(out + r0 * 3);
#pragma unroll
                for (int k = 0; k < 3; ++k) a[k] = pa[k];
#pragma unroll
                for (int q = 0; q < 12; ++q) v[q] = byte_of(a, q);
            } else {
#pragma unroll
                for (int q = 0; q < 12; ++q) v[q] = q < 3 * cnt ? out[r0 * 3 + q] : 0u;
            }
        } else {
            if (whole) {
                unsigned a[3];
                const unsigned* pa = reinterpret_cast<const unsigned*>(fg + r0 * 3);
#pragma unroll
                for (int k = 0; k < 3; ++k) a[k] = pa[k];
#pragma unroll
                for (int q = 0; q < 12; ++q) f[q] = byte_of(a, q);
            } else {
#pragma unroll
                for (int q = 0; q < 12; ++q) f[q] = q < 3 * cnt ? fg[r0 * 3 + q] : 0u;
            }
            if (whole && LOADS == 4) {
#pragma unroll
                for (int p = 0; p < 4; ++p) {
                    const float4 t = *reinterpret_cast<const float4*>(img + (long)(r0 + p) * 4);
                    v[3 * p] = unit_to_u8(t.x); v[3 * p + 1] = unit_to_u8(t.y); v[3 * p + 2] = unit_to_u8(t.z);
                }
            } else if (whole && LOADS == 3) {
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    const float4 t = *reinterpret_cast<const float4*>(img + (long)r0 * 3 + 4 * k);
                    v[4 * k] = unit_to_u8(t.x); v[4 * k + 1] = unit_to_u8(t.y);
                    v[4 * k + 2] = unit_to_u8(t.z); v[4 * k + 3] = unit_to_u8(t.w);
                }
            } else {
#pragma unroll
                for (int p = 0; p < 4; ++p)
#pragma unroll
                    for (int c = 0; c < 3; ++c) v[3 * p + c] = p < cnt ? unit_to_u8(img[(long)(r0 + p) * ldc + c]) : 0u;
            }
#pragma unroll
            for (int p = 0; p < 4; ++p)
                if (m[p] != 0) {
#pragma unroll
                    for (int c = 0; c < 3; ++c) v[3 * p + c] = f[3 * p + c];
                }
        }
#pragma unroll
        for (int p = 0; p < 4; ++p)
            if (drawn[p]) {
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    v[3 * p + c] = (stroke[p] >> (8 * c)) & 0xffu;
                    f[3 * p + c] = v[3 * p + c];
                }
            }
        if (whole) {
            unsigned* po = reinterpret_cast<unsigned*>(out + r0 * 3);
#pragma unroll
            for (int k = 0; k < 3; ++k) po[k] = v[4 * k] | (v[4 * k + 1] << 8) | (v[4 * k + 2] << 16) | (v[4 * k + 3] << 24);
            if (!OVERLAY) {
                unsigned* pm = reinterpret_cast<unsigned*>(fg_marked + r0 * 3);
#pragma unroll
                for (int k = 0; k < 3; ++k) pm[k] = f[4 * k] | (f[4 * k + 1] << 8) | (f[4 * k + 2] << 16) | (f[4 * k + 3] << 24);
            }
        } else {
#pragma unroll
            for (int q = 0; q < 12; ++q)
                if (q < 3 * cnt) {
                    out[r0 * 3 + q] = (u8)v[q];
                    if (!OVERLAY) fg_marked[r0 * 3 + q] = (u8)f[q];
                }
        }
    }
}

extern "C" int ssc_bg_scene_compose_u8(const float* img, int ldc, const uint8_t* fg, const uint8_t* inner, const uint8_t* grass,
                                       const uint8_t* sketch, int H, int W, uint8_t* out, uint8_t* fg_marked, int overlay_only,
                                       void* stream) {
    if (H < 1 || W < 1 || (int64_t)H * W > (1 << 24)) return -1;
    if (inner == nullptr || grass == nullptr || sketch == nullptr || out == nullptr) return -1;
    if (!overlay_only && (img == nullptr || fg == nullptr || fg_marked == nullptr || ldc < 3)) return -1;
    if (((uintptr_t)inner | (uintptr_t)out) & 3) return -3;
    if (!overlay_only && ((((uintptr_t)fg | (uintptr_t)fg_marked | (uintptr_t)img) & 3))) return -3;
    const int M = H * W;
    const dim3 grid(blocks_for(M)), block(256);
    hipStream_t s = (hipStream_t)stream;
    if (overlay_only)
        hipLaunchKernelGGL((bg_scene_compose_kernel<0, true>), grid, block, 0, s, img, ldc, fg, inner, grass, sketch, W, M, out,
                           fg_marked);
    else if (ldc == 4 && ((uintptr_t)img & 15) == 0)
        hipLaunchKernelGGL((bg_scene_compose_kernel<4, false>), grid, block, 0, s, img, ldc, fg, inner, grass, sketch, W, M, out,
                           fg_marked);
    else if (ldc == 3 && ((uintptr_t)img & 15) == 0)
        hipLaunchKernelGGL((bg_scene_compose_kernel<3, false>), grid, block, 0, s, img, ldc, fg, inner, grass, sketch, W, M, out,
                           fg_marked);
    else
        hipLaunchKernelGGL((bg_scene_compose_kernel<0, false>), grid, block, 0, s, img, ldc, fg, inner, grass, sketch, W, M, out,
                           fg_marked);
    return CHECK_LAUNCH();
}

// ---------------------------------------------------------------------------------------------------------------------------
// the sky gradient (add_color_gradient): three launches, workspace int32 [4] = {sky colour r | g<<8 | b<<16, sky_bottom,
// start_height, 1 when the search rows hold no background pixel}
// ---------------------------------------------------------------------------------------------------------------------------
#define SKY_SEARCH_MAX 8192     // pixels of the search rows: their colours sit in LDS (32 KB)
#define NOT_BACKGROUND 0xffffffffu

__device__ __forceinline__ unsigned rgb_at(const u8* __restrict__ color, int r) {
    return (unsigned)color[r * 3] | ((unsigned)color[r * 3 + 1] << 8) | ((unsigned)color[r * 3 + 2] << 16);
}

// One workgroup.  Every background pixel of the search rows counts the pixels of its colour; the key (count, -position) is
// largest for the most frequent colour at its first position in row-major order: the reference's insertion-ordered list and
// argmax.  Integer compares only: the same answer on every run.
__global__ __launch_bounds__(256) void bg_sky_colour_kernel(const u8* __restrict__ color, const u8* __restrict__ inner, int first,
                                                            int n, int* __restrict__ ws) {
    __shared__ unsigned px[SKY_SEARCH_MAX];
    __shared__ unsigned long long best[4];
    for (int k = threadIdx.x; k < n; k += 256) px[k] = inner[first + k] != 0 ? NOT_BACKGROUND : rgb_at(color, first + k);
    __syncthreads();
    unsigned long long mine = 0;
    for (int k = threadIdx.x; k < n; k += 256) {
        const unsigned c = px[k];
        if (c == NOT_BACKGROUND) continue;
        unsigned count = 0;
        for (int q = 0; q < n; ++q) count += px[q] == c;
        const unsigned long long key = ((unsigned long long)count << 32) | (unsigned long long)(0xffffffffu - (unsigned)k);
        mine = key > mine ? key : mine;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long other = __shfl_down(mine, o, 64);
        mine = other > mine ? other : mine;
    }
    if ((threadIdx.x & 63) == 0) best[threadIdx.x >> 6] = mine;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long b = best[0];
#pragma unroll
        for (int k = 1; k < 4; ++k) b = best[k] > b ? best[k] : b;
        const bool none = b == 0;
        ws[0] = none ? 0 : (int)px[0xffffffffu - (unsigned)(b & 0xffffffffull)];
        ws[1] = -1;
        ws[2] = 0;
        ws[3] = none ? 1 : 0;
    }
}

// One workgroup per row 0 .. H/2 of img_bg (white where inner != 0, else color): the largest row that holds the sky colour.
__global__ __launch_bounds__(256) void bg_sky_bottom_kernel(const u8* __restrict__ color, const u8* __restrict__ inner, int W,
                                                            int* ws) {
    if (ws[3] != 0) return;
    const unsigned sky = (unsigned)ws[0];
    const int row = blockIdx.x;
    int found = 0;
    for (int j = threadIdx.x; j < W; j += 256) {
        const int r = row * W + j;
        found |= (inner[r] != 0 ? 0xffffffu : rgb_at(color, r)) == sky;
    }
    if (__syncthreads_or(found) && threadIdx.x == 0) atomicMax(ws + 1, row);
}

// skimage.color.rgb2hsv on one pixel, operation by operation (float64).
__device__ __forceinline__ void rgb2hsv(double r, double g, double b, double& h, double& s, double& v) {
    v = fmax(fmax(r, g), b);
    const double delta = v - fmin(fmin(r, g), b);
    s = delta == 0. ? 0. : delta / v;
    double t = 0.;
    if (delta != 0.) {
        if (r == v) t = (g - b) / delta;            // red, then green, then blue: on a tie for the maximum the later branch wins
        if (g == v) t = 2. + (b - r) / delta;
        if (b == v) t = 4. + (r - g) / delta;
        t = t / 6.;
        t = t < 0. ? t + 1. : t;                     // % 1. of a value in (-1, 1)
    }
    h = t;
}

// skimage.color.hsv2rgb on one pixel, then * 255. and the truncating cast.
__device__ __forceinline__ void hsv2rgb_u8(double h, double s, double v, unsigned (&out)[3]) {
    const double h6 = h * 6.;
    const double hi = floor(h6);
    const double f = h6 - hi;
    const double p = v * (1. - s);
    const double q = v * (1. - f * s);
    const double t = v * (1. - (1. - f) * s);
    double r, g, b;
    switch ((int)hi % 6) {
        case 0: r = v; g = t; b = p; break;
        case 1: r = q; g = v; b = p; break;
        case 2: r = p; g = v; b = t; break;
        case 3: r = p; g = q; b = v; break;
        case 4: r = t; g = p; b = v; break;
        default: r = v; g = p; b = q; break;
    }
    out[0] = (unsigned)(int)(r * 255.);
    out[1] = (unsigned)(int)(g * 255.);
    out[2] = (unsigned)(int)(b * 255.);
}

__global__ __launch_bounds__(256) void bg_sky_gradient_kernel(const u8* __restrict__ color, const u8* __restrict__ inner, int W,
                                                              int M, u8* __restrict__ out, int* __restrict__ status, int* ws) {
    const unsigned sky = (unsigned)ws[0];
    const int sh = (3 * ws[1]) / 4;                 // start_height
    const int st = ws[3] != 0 ? 1 : (sh == 0 ? 2 : 0);
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        status[0] = st;
        ws[2] = st == 0 ? sh : 0;
    }
    // the sky colour's HSV: float32(c) / float32(255) widened to float64
    double h_sky, s_sky, v_sky;
    rgb2hsv((double)((float)(sky & 0xffu) / 255.f), (double)((float)((sky >> 8) & 0xffu) / 255.f),
            (double)((float)((sky >> 16) & 0xffu) / 255.f), h_sky, s_sky, v_sky);
    const double end_s = s_sky / 3.;
    const double end_v = fmin(1., v_sky * 1.5);
    const int groups = (M + 3) >> 2;
    for (int g = blockIdx.x * 256 + threadIdx.x; g < groups; g += gridDim.x * 256) {
        const int r0 = g * 4;
        const int cnt = M - r0 < 4 ? M - r0 : 4;
        const bool whole = cnt == 4;
        unsigned v[12], m[4];
        if (whole) {
            unsigned a[3];
            const unsigned* pa = reinterpret_cast<const unsigned*>(color + r0 * 3);
#pragma unroll
            for (int k = 0; k < 3; ++k) a[k] = pa[k];
#pragma unroll
            for (int q = 0; q < 12; ++q) v[q] = byte_of(a, q);
            const unsigned w = *reinterpret_cast<const unsigned*>(inner + r0);
#pragma unroll
            for (int p = 0; p < 4; ++p) m[p] = (w >> (8 * p)) & 0xffu;
        } else {
#pragma unroll
            for (int q = 0; q < 12; ++q) v[q] = q < 3 * cnt ? color[r0 * 3 + q] : 0u;
#pragma unroll
            for (int p = 0; p < 4; ++p) m[p] = p < cnt ? inner[r0 + p] : 1u;
        }
        if (st == 0) {
            int i = r0 / W, j = r0 - i * W;
#pragma unroll
            for (int p = 0; p < 4; ++p) {
                if (m[p] == 0) {                    // an instance pixel keeps color's bytes (the paste-back)
                    double h, s, val;
                    rgb2hsv((double)v[3 * p] / 255., (double)v[3 * p + 1] / 255., (double)v[3 * p + 2] / 255., h, s, val);
                    if (i <= sh) {
                        const double up = (double)(sh - i) / (double)sh;
                        const double down = (double)i / (double)sh;
                        s = up * end_s + down * s_sky;
                        val = up * end_v + down * v_sky;
                    }
                    unsigned c[3];
                    hsv2rgb_u8(h, s, val, c);
#pragma unroll
                    for (int k = 0; k < 3; ++k) v[3 * p + k] = c[k];
                }
                if (++j == W) { j = 0; ++i; }
            }
        }
        if (whole) {
            unsigned* po = reinterpret_cast<unsigned*>(out + r0 * 3);
#pragma unroll
            for (int k = 0; k < 3; ++k) po[k] = v[4 * k] | (v[4 * k + 1] << 8) | (v[4 * k + 2] << 16) | (v[4 * k + 3] << 24);
        } else {
#pragma unroll
            for (int q = 0; q < 12; ++q)
                if (q < 3 * cnt) out[r0 * 3 + q] = (u8)v[q];
        }
    }
}

extern "C" int ssc_bg_sky_gradient_u8(const uint8_t* color, const uint8_t* inner, int H, int W, int search_from, int search_height,
                                      uint8_t* out, int32_t* status, void* workspace, int64_t workspace_bytes, void* stream) {
    if (H < 1 || W < 1 || (int64_t)H * W > (1 << 24)) return -1;
    if (search_from < 0 || search_height < 1) return -1;
    if ((int64_t)search_from + search_height - 1 > H / 2) return -1;        // the sky colour must lie where sky_bottom is sought
    if ((int64_t)search_height * W > SKY_SEARCH_MAX) return -1;
    if (color == nullptr || inner == nullptr || out == nullptr || status == nullptr) return -1;
    if (workspace == nullptr || workspace_bytes < 16 || ((uintptr_t)workspace & 3)) return -2;
    if ((((uintptr_t)color | (uintptr_t)inner | (uintptr_t)out | (uintptr_t)status) & 3)) return -3;
    hipStream_t s = (hipStream_t)stream;
    int* ws = (int*)workspace;
    const int M = H * W;
    hipLaunchKernelGGL(bg_sky_colour_kernel, dim3(1), dim3(256), 0, s, color, inner, search_from * W, search_height * W, ws);
    hipLaunchKernelGGL(bg_sky_bottom_kernel, dim3((unsigned)(H / 2 + 1)), dim3(256), 0, s, color, inner, W, ws);
    hipLaunchKernelGGL(bg_sky_gradient_kernel, dim3(blocks_for(M)), dim3(256), 0, s, color, inner, W, M, out, status, ws);
    return CHECK_LAUNCH();
}
