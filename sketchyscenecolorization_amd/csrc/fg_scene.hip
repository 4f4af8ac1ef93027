// fg_scene.hip -- the instances of a user scene, painted into it on the device as the scene pipeline paints them (Pipeline_utils/
// fg_color_utils.py::build_instance_colorization, :80-134, 292-296, 342-345): the instance's mask image cut from the small
// segmentation mask, the test that a road is more than a single line, and the masked paste of the generated instance into the
// scene.  All images are uint8 and every step is an integer compare or a copy: the same bytes on every run.  A box starts at an
// arbitrary byte of its row (x1 * 3), so the box kernels go byte by byte and never widen a pointer.  The resizes between these
// steps are ssc_resample_u8, the strokes at the end ssc_bg_scene_compose_u8's overlay.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "sketchycolor_hip.h"

#define CHECK_LAUNCH() ((int)hipGetLastError())
#define MAX_PIXELS (1 << 24)
#define ROAD_MAX_S 4096

typedef unsigned char u8;

static inline unsigned blocks_for(long n) {
    long blocks = (n + 255) / 256;
    return (unsigned)(blocks > 2048 ? 2048 : blocks);
}

// ---------------------------------------------------------------------------------------------------------------------------
// the mask image: 0 where the small mask is 1, 255 for every other byte; the small mask's last row and column are not read
// ---------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void fg_scene_mask_kernel(const u8* __restrict__ small, int bw, int n, u8* __restrict__ out) {
    for (int p = blockIdx.x * 256 + threadIdx.x; p < n; p += gridDim.x * 256) {
        const int i = p / bw, j = p - i * bw;
        out[p] = small[i * (bw + 1) + j] == 1 ? (u8)0 : (u8)255;
    }
}

extern "C" int ssc_fg_scene_mask_u8(const uint8_t* small_mask, int bh, int bw, uint8_t* out, void* stream) {
    if (bh < 1 || bw < 1 || (int64_t)(bh + 1) * (bw + 1) > MAX_PIXELS) return -1;
    if (small_mask == nullptr || out == nullptr) return -1;
    const int n = bh * bw;
    hipLaunchKernelGGL(fg_scene_mask_kernel, dim3(blocks_for(n)), dim3(256), 0, (hipStream_t)stream, small_mask, bw, n, out);
    return CHECK_LAUNCH();
}

// ---------------------------------------------------------------------------------------------------------------------------
// is_road_not_single_line: out int32 [3] = {verdict, V, Hc}
// ---------------------------------------------------------------------------------------------------------------------------
// The reference binarises in two steps: a pixel whose three bytes are all >= 235 becomes white, then a pixel whose three bytes
// all differ from 255 becomes black, and the red byte is read: 0 -> 1 (stroke), 255 -> 0.  The instance sketch is grey (one
// channel replicated), so a pixel is either >= 235 in all three bytes (white, 0) or below 235 in all three (not 255: black, 1):
// both steps together are s = (red byte < 235).  Its in-place loop clears s[i][j] where s[i+1][j] is set, reading only entries it
// has not changed yet, so what it sums per column is the number of run ends: s[i][j] && !s[i+1][j] for i < S-1, and s[S-1][j].
// A column counts when that number is positive and even; its early return after each column is V >= parallel_width, which is
// monotone in the columns seen.  Rows the same.  One workgroup: a thread scans whole columns and rows (2 S scans of S bytes),
// integer sums over the wavefront and the four wavefronts.
__device__ __forceinline__ int road_scan(const u8* __restrict__ sketch, int S, long first, long step) {
    int ends = 0;
    bool cur = sketch[first] < 235;
    for (int k = 1; k < S; ++k) {
        const bool next = sketch[first + k * step] < 235;
        ends += cur && !next;
        cur = next;
    }
    return ends + cur;
}

__global__ __launch_bounds__(256) void road_parallel_kernel(const u8* __restrict__ sketch, int S, int parallel_width,
                                                            int* __restrict__ out) {
    __shared__ int part[2][4];
    int v = 0, h = 0;
    for (int t = threadIdx.x; t < 2 * S; t += 256) {
        const bool column = t < S;
        const int line = column ? t : t - S;
        const int ends = column ? road_scan(sketch, S, (long)line * 3, (long)S * 3) : road_scan(sketch, S, (long)line * S * 3, 3);
        const int valid = ends > 0 && (ends & 1) == 0;
        v += column ? valid : 0;
        h += column ? 0 : valid;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        v += __shfl_down(v, o, 64);
        h += __shfl_down(h, o, 64);
    }
    if ((threadIdx.x & 63) == 0) {
        part[0][threadIdx.x >> 6] = v;
        part[1][threadIdx.x >> 6] = h;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        const int V = part[0][0] + part[0][1] + part[0][2] + part[0][3];
        const int Hc = part[1][0] + part[1][1] + part[1][2] + part[1][3];
        out[0] = V >= parallel_width || Hc >= parallel_width;
        out[1] = V;
        out[2] = Hc;
    }
}

extern "C" int ssc_road_parallel_u8(const uint8_t* sketch, int S, int parallel_width, int32_t* out, void* stream) {
    if (S < 1 || S > ROAD_MAX_S || parallel_width < 1) return -1;
    if (sketch == nullptr || out == nullptr) return -1;
    if ((uintptr_t)out & 3) return -3;
    hipLaunchKernelGGL(road_parallel_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, sketch, S, parallel_width, out);
    return CHECK_LAUNCH();
}

// ---------------------------------------------------------------------------------------------------------------------------
// the paste: result[y1+i][x1+j] = inst[i][j] where inner[y1+i][x1+j] == value; nothing else is written
// ---------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void fg_scene_paste_kernel(u8* __restrict__ result, const u8* __restrict__ inner, int W,
                                                             const u8* __restrict__ inst, int y1, int x1, int bw, int n,
                                                             unsigned value) {
    for (int p = blockIdx.x * 256 + threadIdx.x; p < n; p += gridDim.x * 256) {
        const int i = p / bw, j = p - i * bw;
        const int r = (y1 + i) * W + x1 + j;
        if (inner[r] == value) {
#pragma unroll
            for (int c = 0; c < 3; ++c) result[r * 3 + c] = inst[p * 3 + c];
        }
    }
}

extern "C" int ssc_fg_scene_paste_u8(uint8_t* result, const uint8_t* inner, int H, int W, const uint8_t* inst, int y1, int x1,
                                     int bh, int bw, int value, void* stream) {
    if (H < 1 || W < 1 || (int64_t)H * W > MAX_PIXELS) return -1;
    if (bh < 1 || bw < 1 || y1 < 0 || x1 < 0 || (int64_t)y1 + bh > H || (int64_t)x1 + bw > W) return -1;
    if (value < 1 || value > 255) return -1;
    if (result == nullptr || inner == nullptr || inst == nullptr) return -1;
    const int n = bh * bw;
    hipLaunchKernelGGL(fg_scene_paste_kernel, dim3(blocks_for(n)), dim3(256), 0, (hipStream_t)stream, result, inner, W, inst, y1,
                       x1, bw, n, (unsigned)value);
    return CHECK_LAUNCH();
}
