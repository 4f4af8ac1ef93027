// match_eval.hip -- the two integer histograms that the evaluation of the instance matcher reduces to (Instance_Matching/
// matching_main.py --mode eval: compute_mask_IU, compute_overlaps_masks; match_eval.py).  A scene's ground
// truth is one uint8 label map (0: background, k + 1: the k-th instance); every pixel count the metrics ask for is a bin of
//   ssc_label_hist_u8        out[g]    = #{p : labels[p] == g and (gate == NULL or gate[p] != 0)}            (area, P)
//   ssc_instance_label_hist  out[k][g] = #{p in the box of instance k : mask_k[p] != 0 and labels[p] == g}    (H)
// Both keep a workgroup's 256 bins in LDS behind 32-bit LDS atomics (a workgroup sees at most 2^24 pixels); only integers are
// added, so the order of the adds does not show: the same bits on every run.  Memory-bound, 16-byte loads along the pixels.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "sketchycolor_hip.h"

#define CHECK_LAUNCH() ((int)hipGetLastError())
#define MAX_PIXELS (1 << 24)
#define BINS 256

typedef unsigned char u8;

// ---------------------------------------------------------------------------------------------------------------------------
// out[g] = #{p < n : labels[p] == g and (gate == NULL or gate[p] != 0)}
// ---------------------------------------------------------------------------------------------------------------------------
// The first `head` bytes bring labels to a 16-byte boundary; then nvec 16-byte vectors; then the rest.  Head and rest are read
// bytewise by workgroup 0.  The gate is read 16 bytes at a time where it shares the labels' misalignment (GATE_WIDE), bytewise
// otherwise.  A label map is made of runs: a thread adds a run of equal labels inside its vector with one LDS atomic.
template <bool GATED, bool GATE_WIDE>
__global__ __launch_bounds__(256) void label_hist_kernel(const u8* __restrict__ labels, const u8* __restrict__ gate, long n, int head,
                                                         long nvec, unsigned long long* __restrict__ out) {
    __shared__ unsigned hist[BINS];
    hist[threadIdx.x] = 0;
    __syncthreads();
    for (long v = (long)blockIdx.x * 256 + threadIdx.x; v < nvec; v += (long)gridDim.x * 256) {
        const long p0 = head + v * 16;
        const uint4 lv = *reinterpret_cast<const uint4*>(labels + p0);
        const unsigned lw[4] = {lv.x, lv.y, lv.z, lv.w};
        unsigned gw[4] = {0x01010101u, 0x01010101u, 0x01010101u, 0x01010101u};
        if (GATED) {
            if (GATE_WIDE) {
                const uint4 gv = *reinterpret_cast<const uint4*>(gate + p0);
                gw[0] = gv.x, gw[1] = gv.y, gw[2] = gv.z, gw[3] = gv.w;
            } else {
#pragma unroll
                for (int k = 0; k < 16; ++k) {
                    const unsigned b = gate[p0 + k];
                    gw[k >> 2] = (k & 3) == 0 ? b : (gw[k >> 2] | (b << ((k & 3) * 8)));
                }
            }
        }
        unsigned run_label = 0, run = 0;
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            const unsigned l = (lw[k >> 2] >> ((k & 3) * 8)) & 255u;
            const unsigned g = (gw[k >> 2] >> ((k & 3) * 8)) & 255u;
            if (g == 0) continue;
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
        const long body_end = head + nvec * 16;
        const long edge = head + (n - body_end);
        for (long e = threadIdx.x; e < edge; e += 256) {
            const long p = e < head ? e : body_end + (e - head);
            if (!GATED || gate[p] != 0) atomicAdd(&hist[labels[p]], 1u);
        }
    }
    __syncthreads();
    const unsigned c = hist[threadIdx.x];
    if (c != 0) atomicAdd(&out[threadIdx.x], (unsigned long long)c);
}

extern "C" int ssc_label_hist_u8(const uint8_t* labels, const uint8_t* gate, int64_t n, int64_t* out, void* stream) {
    if (n < 1 || n > MAX_PIXELS) return -1;
    if (labels == nullptr || out == nullptr) return -1;
    if ((uintptr_t)out & 7) return -3;
    long head = (long)((16 - ((uintptr_t)labels & 15)) & 15);
    if (head > n) head = n;
    const long nvec = (n - head) / 16;
    const bool wide = gate != nullptr && (((uintptr_t)gate ^ (uintptr_t)labels) & 15) == 0;
    const hipError_t e = hipMemsetAsync(out, 0, BINS * sizeof(int64_t), (hipStream_t)stream);
    if (e != hipSuccess) return (int)e;
    long blocks = (nvec + 255) / 256;
    if (blocks < 1) blocks = 1;
    if (blocks > 2048) blocks = 2048;
    const dim3 grid((unsigned)blocks), block(256);
    unsigned long long* o = reinterpret_cast<unsigned long long*>(out);
    if (gate == nullptr)
        hipLaunchKernelGGL((label_hist_kernel<false, false>), grid, block, 0, (hipStream_t)stream, labels, gate, (long)n, (int)head, nvec, o);
    else if (wide)
        hipLaunchKernelGGL((label_hist_kernel<true, true>), grid, block, 0, (hipStream_t)stream, labels, gate, (long)n, (int)head, nvec, o);
    else
        hipLaunchKernelGGL((label_hist_kernel<true, false>), grid, block, 0, (hipStream_t)stream, labels, gate, (long)n, (int)head, nvec, o);
    return CHECK_LAUNCH();
}

// ---------------------------------------------------------------------------------------------------------------------------
// out[k][g] = #{pixels of instance k's box with mask byte != 0 and labels == g}
// ---------------------------------------------------------------------------------------------------------------------------
// The boxes, offsets and masks of ssc_instance_occupancy (matching.hip): the small mask of instance k is masks[offsets[k] ..],
// (y2 - y1 + 1) rows of (x2 - x1 + 1) bytes, laid at (y1, x1), both ends of the box included.  One workgroup per instance, so
// boxes that overlap do not meet.  A box that is empty, leaves the image, or whose mask leaves the buffer gives a row of -1 and
// reads nothing.
__global__ __launch_bounds__(256) void instance_label_hist_kernel(const u8* __restrict__ labels, int S, const u8* __restrict__ masks,
                                                                  long mask_bytes, const int* __restrict__ boxes,
                                                                  const long* __restrict__ offsets, long* __restrict__ out) {
    __shared__ unsigned hist[BINS];
    const int k = blockIdx.x;
    const int y1 = boxes[k * 4], x1 = boxes[k * 4 + 1], y2 = boxes[k * 4 + 2], x2 = boxes[k * 4 + 3];
    const long off = offsets[k];
    const long bh = (long)y2 - y1 + 1, bw = (long)x2 - x1 + 1;
    if (y1 < 0 || x1 < 0 || y2 >= S || x2 >= S || bh < 1 || bw < 1 || off < 0 || off > mask_bytes || bh * bw > mask_bytes - off) {
        out[(long)k * BINS + threadIdx.x] = -1;
        return;
    }
    hist[threadIdx.x] = 0;
    __syncthreads();
    const long n = bh * bw;
    for (long p = threadIdx.x; p < n; p += 256) {
        const long i = p / bw, j = p - i * bw;
        if (masks[off + p] != 0) atomicAdd(&hist[labels[(y1 + i) * S + x1 + j]], 1u);
    }
    __syncthreads();
    out[(long)k * BINS + threadIdx.x] = (long)hist[threadIdx.x];
}

extern "C" int ssc_instance_label_hist(const uint8_t* labels, int S, const uint8_t* masks, int64_t mask_bytes, const int32_t* boxes,
                                       const int64_t* offsets, int N, int64_t* out, void* stream) {
    if (S < 1 || (int64_t)S * S > MAX_PIXELS || N < 1 || N > 65535 || mask_bytes < 1) return -1;
    if (labels == nullptr || masks == nullptr || boxes == nullptr || offsets == nullptr || out == nullptr) return -1;
    if (((uintptr_t)boxes & 3) || ((uintptr_t)offsets & 7) || ((uintptr_t)out & 7)) return -3;
    hipLaunchKernelGGL(instance_label_hist_kernel, dim3((unsigned)N), dim3(256), 0, (hipStream_t)stream, labels, S, masks,
                       (long)mask_bytes, boxes, (const long*)offsets, (long*)out);
    return CHECK_LAUNCH();
}
