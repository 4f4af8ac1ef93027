// match_val.hip -- scoring a held-out caption while the matcher trains (match_validation.py, match_main.py --val_freq; DESIGN.md
// section 8.9): one pass over the S x S pixels from the head's 1/8-resolution map gives the five numbers that the overall IoU,
// precision@X and the class loss of a caption are made of.  Neither the up-sampled map nor predicts is written.
//   u = the legacy bilinear value of ssc_match_finish (match_up.h), b = sketch[3p], z = lut[labels[p]] != 0
//   I = #{u >= 1e-9f && b != 255 && z}   P = #{u >= 1e-9f && b != 255}   A = #{z}   live = #{b <= 104}
//   loss = sum over the live pixels of max(u,0) - u*z + log1p(exp(-|u|))     (the fp32 terms of ssc_match_loss_grad, added in double)
// Memory-bound (4 bytes per pixel read).  A thread owns four neighbouring pixels of a row.  Every sum runs in a fixed order:
// a thread over its pixels, the 64 lanes by butterfly, the four wavefronts through LDS, the workgroups by a second launch of
// one workgroup over the partial rows in the workspace.  No float atomic; the grid is a function of S alone: the same bits on
// every run and every machine.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "sketchycolor_hip.h"
#include "match_up.h"

#define CHECK_LAUNCH() ((int)hipGetLastError())
#define MAX_PIXELS (1 << 24)
#define SCORE_MAX_BLOCKS 2048

typedef unsigned char u8;

struct score_part {
    double loss;
    long long inter, pred, area, live;
};

static inline unsigned score_blocks(int S) {
    long blocks = ((long)S * (S / 4) + 255) / 256;
    if (blocks < 1) blocks = 1;
    return (unsigned)(blocks > SCORE_MAX_BLOCKS ? SCORE_MAX_BLOCKS : blocks);
}

// WIDE: sketch and labels both start on a 4-byte boundary -- the 12 sketch bytes and the 4 labels of a thread are four 4-byte
// loads; otherwise they are read byte by byte.
template <bool WIDE>
__global__ __launch_bounds__(256) void match_score_kernel(const float* __restrict__ pred, int h, int w, const u8* __restrict__ sketch,
                                                          const u8* __restrict__ labels, const u8* __restrict__ lut, int S, float sy,
                                                          float sx, score_part* __restrict__ part) {
    __shared__ double sh_l[4];
    __shared__ long long sh_n[4][4];
    const int q4 = S >> 2;
    const long total = (long)S * q4;
    double loss = 0.0;
    int n_i = 0, n_p = 0, n_a = 0, n_live = 0;      // a thread sees at most 4 * ceil(2^22 / (2048 * 256)) pixels
    for (long t = (long)blockIdx.x * 256 + threadIdx.x; t < total; t += (long)gridDim.x * 256) {
        const int y = (int)(t / q4), x0 = (int)(t - (long)y * q4) * 4;
        const long p0 = (long)y * S + x0;
        int ylo, yhi;
        float wy;
        match_up_axis(y, sy, h, ylo, yhi, wy);
        u8 sb[4], lb[4];
        if (WIDE) {
            const unsigned* s32 = reinterpret_cast<const unsigned*>(sketch + p0 * 3);
            const unsigned s0 = s32[0], s1 = s32[1], s2 = s32[2];
            const unsigned l32 = *reinterpret_cast<const unsigned*>(labels + p0);
            sb[0] = (u8)(s0 & 255u), sb[1] = (u8)(s0 >> 24), sb[2] = (u8)((s1 >> 16) & 255u), sb[3] = (u8)((s2 >> 8) & 255u);
            lb[0] = (u8)(l32 & 255u), lb[1] = (u8)((l32 >> 8) & 255u), lb[2] = (u8)((l32 >> 16) & 255u), lb[3] = (u8)(l32 >> 24);
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                sb[k] = sketch[(p0 + k) * 3];
                lb[k] = labels[p0 + k];
            }
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float u = match_up_value(pred, w, ylo, yhi, wy, x0 + k, sx);
            const bool zb = lut[lb[k]] != 0;
            const bool on = u >= 1e-9f && sb[k] != 255;
            n_p += on ? 1 : 0;
            n_i += (on && zb) ? 1 : 0;
            n_a += zb ? 1 : 0;
            if (sb[k] <= 104) {
                const float z = zb ? 1.f : 0.f;
                const float e = expf(-fabsf(u));
                loss += (double)(fmaxf(u, 0.f) - u * z + log1pf(e));
                n_live += 1;
            }
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        loss += __shfl_xor(loss, o, 64);
        n_i += __shfl_xor(n_i, o, 64);
        n_p += __shfl_xor(n_p, o, 64);
        n_a += __shfl_xor(n_a, o, 64);
        n_live += __shfl_xor(n_live, o, 64);
    }
    if ((threadIdx.x & 63) == 0) {
        const int wv = threadIdx.x >> 6;
        sh_l[wv] = loss;
        sh_n[wv][0] = n_i, sh_n[wv][1] = n_p, sh_n[wv][2] = n_a, sh_n[wv][3] = n_live;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        score_part c;
        c.loss = ((sh_l[0] + sh_l[1]) + sh_l[2]) + sh_l[3];
        c.inter = sh_n[0][0] + sh_n[1][0] + sh_n[2][0] + sh_n[3][0];
        c.pred = sh_n[0][1] + sh_n[1][1] + sh_n[2][1] + sh_n[3][1];
        c.area = sh_n[0][2] + sh_n[1][2] + sh_n[2][2] + sh_n[3][2];
        c.live = sh_n[0][3] + sh_n[1][3] + sh_n[2][3] + sh_n[3][3];
        part[blockIdx.x] = c;
    }
}

// one workgroup: thread t adds the partial rows t, t + 256, .. in order, then the 256 sums pairwise through LDS
__global__ __launch_bounds__(256) void match_score_finish_kernel(const score_part* __restrict__ part, int rows, double* __restrict__ out) {
    __shared__ double sl[256];
    __shared__ long long sn[4][256];
    double l = 0.0;
    long long c[4] = {0, 0, 0, 0};
    for (int t = threadIdx.x; t < rows; t += 256) {
        const score_part r = part[t];
        l += r.loss;
        c[0] += r.inter, c[1] += r.pred, c[2] += r.area, c[3] += r.live;
    }
    sl[threadIdx.x] = l;
#pragma unroll
    for (int k = 0; k < 4; ++k) sn[k][threadIdx.x] = c[k];
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) {
            sl[threadIdx.x] += sl[threadIdx.x + o];
#pragma unroll
            for (int k = 0; k < 4; ++k) sn[k][threadIdx.x] += sn[k][threadIdx.x + o];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        out[0] = sl[0];
        long long* oi = reinterpret_cast<long long*>(out);
        oi[1] = sn[0][0], oi[2] = sn[1][0], oi[3] = sn[2][0], oi[4] = sn[3][0];
    }
}

extern "C" int ssc_match_score(const float* pred, int h, int w, const uint8_t* sketch, const uint8_t* labels, const uint8_t* lut, int S,
                               double* out, float* ws, int64_t ws_bytes, void* stream) {
    if (h < 1 || w < 1 || S < 4 || (S & 3) || (int64_t)S * S > MAX_PIXELS || h > S || w > S) return -1;
    if (pred == nullptr || sketch == nullptr || labels == nullptr || lut == nullptr || out == nullptr || ws == nullptr) return -1;
    const unsigned blocks = score_blocks(S);
    if (ws_bytes < (int64_t)blocks * (int64_t)sizeof(score_part)) return -1;
    if (((uintptr_t)out & 7) || ((uintptr_t)ws & 7) || ((uintptr_t)pred & 3)) return -3;
    const float sy = (float)h / (float)S, sx = (float)w / (float)S;
    if ((((uintptr_t)sketch | (uintptr_t)labels) & 3) == 0)
        hipLaunchKernelGGL((match_score_kernel<true>), dim3(blocks), dim3(256), 0, (hipStream_t)stream, pred, h, w, sketch, labels, lut,
                           S, sy, sx, (score_part*)ws);
    else
        hipLaunchKernelGGL((match_score_kernel<false>), dim3(blocks), dim3(256), 0, (hipStream_t)stream, pred, h, w, sketch, labels, lut,
                           S, sy, sx, (score_part*)ws);
    const int rc = CHECK_LAUNCH();
    if (rc != 0) return rc;
    hipLaunchKernelGGL(match_score_finish_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, (const score_part*)ws, (int)blocks, out);
    return CHECK_LAUNCH();
}
