// scene_system.hip -- the per-turn change report of a scene session (scene_session.py): which pixels an
// instruction changed, counted per value of the scene's inner mask (0: background, k + 1: instance k).
//   ssc_scene_change_hist_u8   out[g] = #{p : inner[p] == g and (prev[3p], prev[3p+1], prev[3p+2]) != (next[3p], next[3p+1], next[3p+2])}
// The comparison is fused into the gated histogram of match_eval.hip (ssc_label_hist_u8 reads its gate from memory): a workgroup
// keeps 256 bins in LDS behind 32-bit LDS atomics (it sees at most 2^24 pixels) and adds its non-empty ones to out as 64-bit
// integers.  Only integers are added, so the order of the adds does not show: the same bits on every run.  Memory-bound.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "sketchycolor_hip.h"

#define CHECK_LAUNCH() ((int)hipGetLastError())
#define MAX_PIXELS (1 << 24)
#define BINS 256
#define GROUP 16            // pixels per lane and step: 16 bytes of the mask, 48 bytes (three 16-byte vectors) of each image

typedef unsigned char u8;

// A pixel is 3 bytes, so no pixel but every GROUP-th starts on a 16-byte boundary: a lane takes GROUP pixels, whose 48 bytes do
// when the image does.  WIDE: the three pointers are on 16-byte boundaries and the lane reads 7 vectors; otherwise it reads its
// 112 bytes one by one (a view into a larger tensor).  The n % GROUP pixels at the end are read bytewise by workgroup 0.
template <bool WIDE>
__global__ __launch_bounds__(256) void scene_change_hist_kernel(const u8* __restrict__ prev, const u8* __restrict__ next,
                                                                const u8* __restrict__ inner, long n, long ngroups,
                                                                unsigned long long* __restrict__ out) {
    __shared__ unsigned hist[BINS];
    hist[threadIdx.x] = 0;
    __syncthreads();
    for (long g = (long)blockIdx.x * 256 + threadIdx.x; g < ngroups; g += (long)gridDim.x * 256) {
        const long p0 = g * GROUP;
        unsigned lw[4], dw[12];
        if (WIDE) {
            const uint4 lv = *reinterpret_cast<const uint4*>(inner + p0);
            lw[0] = lv.x, lw[1] = lv.y, lw[2] = lv.z, lw[3] = lv.w;
#pragma unroll
            for (int v = 0; v < 3; ++v) {
                const uint4 a = *reinterpret_cast<const uint4*>(prev + 3 * p0 + 16 * v);
                const uint4 b = *reinterpret_cast<const uint4*>(next + 3 * p0 + 16 * v);
                dw[4 * v] = a.x ^ b.x, dw[4 * v + 1] = a.y ^ b.y, dw[4 * v + 2] = a.z ^ b.z, dw[4 * v + 3] = a.w ^ b.w;
            }
        } else {
#pragma unroll
            for (int k = 0; k < 16; ++k) {
                const unsigned b = inner[p0 + k];
                lw[k >> 2] = (k & 3) == 0 ? b : (lw[k >> 2] | (b << ((k & 3) * 8)));
            }
#pragma unroll
            for (int k = 0; k < 48; ++k) {
                const unsigned b = (unsigned)(prev[3 * p0 + k] ^ next[3 * p0 + k]);
                dw[k >> 2] = (k & 3) == 0 ? b : (dw[k >> 2] | (b << ((k & 3) * 8)));
            }
        }
        // a scene is made of runs of one instance: a run of changed pixels of one label inside the group is one LDS atomic
        unsigned run_label = 0, run = 0;
#pragma unroll
        for (int k = 0; k < GROUP; ++k) {
            unsigned d = 0;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const int byte = 3 * k + c;
                d |= (dw[byte >> 2] >> ((byte & 3) * 8)) & 255u;
            }
            if (d == 0) continue;
            const unsigned l = (lw[k >> 2] >> ((k & 3) * 8)) & 255u;
            if (l != run_label && run != 0) {
                atomicAdd(&hist[run_label], run);
                run = 0;
            }
            run_label = l;
            ++run;
        }
        if (run != 0) atomicAdd(&hist[run_label], run);
    }
    if (blockIdx.x == 0) {
        for (long p = ngroups * GROUP + threadIdx.x; p < n; p += 256) {
            const unsigned d = (unsigned)(prev[3 * p] ^ next[3 * p]) | (unsigned)(prev[3 * p + 1] ^ next[3 * p + 1]) |
                               (unsigned)(prev[3 * p + 2] ^ next[3 * p + 2]);
            if (d != 0) atomicAdd(&hist[inner[p]], 1u);
        }
    }
    __syncthreads();
    const unsigned c = hist[threadIdx.x];
    if (c != 0) atomicAdd(&out[threadIdx.x], (unsigned long long)c);
}

extern "C" int ssc_scene_change_hist_u8(const uint8_t* prev, const uint8_t* next, const uint8_t* inner, int H, int W, int64_t* out,
                                        void* stream) {
    if (H < 1 || W < 1 || (int64_t)H * W > MAX_PIXELS) return -1;
    if (prev == nullptr || next == nullptr || inner == nullptr || out == nullptr) return -1;
    if ((uintptr_t)out & 7) return -3;
    const long n = (long)H * W;
    const long ngroups = n / GROUP;
    const bool wide = (((uintptr_t)prev | (uintptr_t)next | (uintptr_t)inner) & 15) == 0;
    const hipError_t e = hipMemsetAsync(out, 0, BINS * sizeof(int64_t), (hipStream_t)stream);
    if (e != hipSuccess) return (int)e;
    long blocks = (ngroups + 255) / 256;
    if (blocks < 1) blocks = 1;
    if (blocks > 2048) blocks = 2048;
    const dim3 grid((unsigned)blocks), block(256);
    unsigned long long* o = reinterpret_cast<unsigned long long*>(out);
    if (wide)
        hipLaunchKernelGGL((scene_change_hist_kernel<true>), grid, block, 0, (hipStream_t)stream, prev, next, inner, n, ngroups, o);
    else
        hipLaunchKernelGGL((scene_change_hist_kernel<false>), grid, block, 0, (hipStream_t)stream, prev, next, inner, n, ngroups, o);
    return CHECK_LAUNCH();
}
