// match_train.hip -- what training the matcher's fusion head (Instance_Matching/RMI_model.py::train_op with
// train_fusion_var_only, utils/loss.py) needs beyond the caption branch's backward kernels: the loss on
// the up-sampled logits with its gradient brought back to the head's map, and the backward of ssc_squash_project.
// Both are memory-bound.  Every sum runs in a fixed order -- lanes by butterfly, wavefronts and workgroups one after the other
// through LDS or the workspace -- and nothing is added with a float atomic: the same bits on every run.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "sketchycolor_hip.h"

#define CHECK_LAUNCH() ((int)hipGetLastError())
#define MAX_PIXELS (1 << 24)

typedef unsigned char u8;

// ---------------------------------------------------------------------------------------------------------------------------
// sum over the live pixels of sigmoid_cross_entropy_with_logits(up, target), up = the legacy bilinear up-sampling of pred
// ---------------------------------------------------------------------------------------------------------------------------
// A gather: workgroup (i, j) owns the cell pred[i][j].  The pixels whose interpolation can read the cell lie in the rows
// k (i - 1) .. k (i + 1) and the columns k (j - 1) .. k (j + 1), clipped to the image (one row and column more than the 2k the
// exact quotient needs: the kernel asks the pixel's own lower / upper index, worked out as ssc_match_finish works it out, whether
// it names the cell).  In the last k rows the upper index is clamped onto the lower one and both weights fall on the cell h - 1.
// The loss and the count of a pixel go to the cell of its lower indices, so that every pixel is counted once.
struct cell_part {
    double loss;
    long long live;
};

__global__ __launch_bounds__(256) void match_loss_grad_kernel(const float* __restrict__ pred, int h, int w, const u8* __restrict__ sketch,
                                                              const u8* __restrict__ labels, const u8* __restrict__ lut, int S, int k,
                                                              float sy, float sx, float* __restrict__ dpred,
                                                              cell_part* __restrict__ part) {
    __shared__ float sh_g[4];
    __shared__ double sh_l[4];
    __shared__ int sh_n[4];
    const int cell = blockIdx.x;
    const int i = cell / w, j = cell - i * w;
    const int y0 = max(k * (i - 1), 0), y1 = min(k * (i + 1), S - 1);
    const int x0 = max(k * (j - 1), 0), x1 = min(k * (j + 1), S - 1);
    const int nx = x1 - x0 + 1, n = (y1 - y0 + 1) * nx;
    float g_sum = 0.f;
    double l_sum = 0.0;
    int n_live = 0;
    for (int p = threadIdx.x; p < n; p += 256) {
        const int y = y0 + p / nx, x = x0 + p % nx;
        const long q = (long)y * S + x;
        if (sketch[q * 3] > 104) continue;
        const float fy = (float)y * sy;
        const int ylo = min((int)floorf(fy), h - 1);
        const int yhi = ylo + 1 < h ? ylo + 1 : h - 1;
        const float wy = fy - (float)ylo;
        const float fx = (float)x * sx;
        const int xlo = min((int)floorf(fx), w - 1);
        const int xhi = xlo + 1 < w ? xlo + 1 : w - 1;
        const float wx = fx - (float)xlo;
        const float cy = (ylo == i ? 1.f - wy : 0.f) + (yhi == i ? wy : 0.f);
        const float cx = (xlo == j ? 1.f - wx : 0.f) + (xhi == j ? wx : 0.f);
        if ((ylo != i && yhi != i) || (xlo != j && xhi != j)) continue;
        const float tl = pred[ylo * w + xlo], tr = pred[ylo * w + xhi], bl = pred[yhi * w + xlo], br = pred[yhi * w + xhi];
        const float top = tl + (tr - tl) * wx, bot = bl + (br - bl) * wx;
        const float u = top + (bot - top) * wy;
        const float z = lut[labels[q]] != 0 ? 1.f : 0.f;
        const float e = expf(-fabsf(u));
        const float sig = u >= 0.f ? 1.f / (1.f + e) : e / (1.f + e);
        g_sum += (sig - z) * (cy * cx);
        if (ylo == i && xlo == j) {
            l_sum += (double)(fmaxf(u, 0.f) - u * z + log1pf(e));
            n_live += 1;
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        g_sum += __shfl_xor(g_sum, o, 64);
        l_sum += __shfl_xor(l_sum, o, 64);
        n_live += __shfl_xor(n_live, o, 64);
    }
    if ((threadIdx.x & 63) == 0) {
        sh_g[threadIdx.x >> 6] = g_sum;
        sh_l[threadIdx.x >> 6] = l_sum;
        sh_n[threadIdx.x >> 6] = n_live;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        dpred[cell] = ((sh_g[0] + sh_g[1]) + sh_g[2]) + sh_g[3];
        cell_part c;
        c.loss = ((sh_l[0] + sh_l[1]) + sh_l[2]) + sh_l[3];
        c.live = (long long)sh_n[0] + sh_n[1] + sh_n[2] + sh_n[3];
        part[cell] = c;
    }
}

// one workgroup: thread t adds the cells t, t + 256, .. in order, then the 256 partial sums pairwise through LDS
__global__ __launch_bounds__(256) void match_loss_finish_kernel(const cell_part* __restrict__ part, int cells,
                                                                double* __restrict__ loss_acc, long long* __restrict__ live) {
    __shared__ double sl[256];
    __shared__ long long sn[256];
    double l = 0.0;
    long long c = 0;
    for (int t = threadIdx.x; t < cells; t += 256) {
        l += part[t].loss;
        c += part[t].live;
    }
    sl[threadIdx.x] = l;
    sn[threadIdx.x] = c;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) {
            sl[threadIdx.x] += sl[threadIdx.x + o];
            sn[threadIdx.x] += sn[threadIdx.x + o];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        loss_acc[0] += sl[0];
        live[0] = sn[0];
    }
}

extern "C" int ssc_match_loss_grad(const float* pred, int h, int w, const uint8_t* sketch, const uint8_t* labels, const uint8_t* lut,
                                   int S, double* loss_acc, int64_t* live, float* dpred, float* ws, int64_t ws_bytes, void* stream) {
    if (h < 1 || w < 1 || S < 1 || (int64_t)S * S > MAX_PIXELS || h > S || w > S) return -1;
    const int k = S / h;
    if (k * h != S || k * w != S) return -1;
    if (pred == nullptr || sketch == nullptr || labels == nullptr || lut == nullptr || loss_acc == nullptr || live == nullptr ||
        dpred == nullptr || ws == nullptr)
        return -1;
    const int64_t cells = (int64_t)h * w;
    if (ws_bytes < cells * (int64_t)sizeof(cell_part)) return -1;
    if (((uintptr_t)ws & 7) || ((uintptr_t)loss_acc & 7) || ((uintptr_t)live & 7)) return -3;
    hipLaunchKernelGGL(match_loss_grad_kernel, dim3((unsigned)cells), dim3(256), 0, (hipStream_t)stream, pred, h, w, sketch, labels,
                       lut, S, k, (float)h / (float)S, (float)w / (float)S, dpred, (cell_part*)ws);
    int rc = CHECK_LAUNCH();
    if (rc != 0) return rc;
    hipLaunchKernelGGL(match_loss_finish_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, (const cell_part*)ws, (int)cells,
                       loss_acc, (long long*)live);
    return CHECK_LAUNCH();
}

// ---------------------------------------------------------------------------------------------------------------------------
// the backward of ssc_squash_project: pred[r] = sum_c max(s(hh[r][c]), 0) * w[c] + b, s(v) = 0.5 (log(1.001 + v) - log(1.001 - v))
// ---------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float squash_s(float v) { return 0.5f * (logf(1.0f + 1e-3f + v) - logf(1.0f + 1e-3f - v)); }
__device__ __forceinline__ float squash_d(float v) { return 0.5f * (1.f / (1.0f + 1e-3f + v) + 1.f / (1.0f + 1e-3f - v)); }

// dh: a thread owns four neighbouring columns of a row, pad columns included (they are written as 0)
__global__ __launch_bounds__(256) void squash_project_dh_kernel(const float* __restrict__ hh, int ldh, const float* __restrict__ w,
                                                                const float* __restrict__ dpred, long rows, int C,
                                                                float* __restrict__ dh) {
    const int q4 = ldh >> 2;
    const long total = rows * q4;
    for (long t = (long)blockIdx.x * 256 + threadIdx.x; t < total; t += (long)gridDim.x * 256) {
        const long r = t / q4;
        const int c = (int)(t - r * q4) * 4;
        float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
        if (c < C) {        // C % 4 == 0: the four columns are real or pad together
            const float4 v = *reinterpret_cast<const float4*>(hh + r * ldh + c);
            const float4 k = *reinterpret_cast<const float4*>(w + c);
            const float g = dpred[r];
            o.x = squash_s(v.x) > 0.f ? g * k.x * squash_d(v.x) : 0.f;
            o.y = squash_s(v.y) > 0.f ? g * k.y * squash_d(v.y) : 0.f;
            o.z = squash_s(v.z) > 0.f ? g * k.z * squash_d(v.z) : 0.f;
            o.w = squash_s(v.w) > 0.f ? g * k.w * squash_d(v.w) : 0.f;
        }
        *reinterpret_cast<float4*>(dh + r * ldh + c) = o;
    }
}

// dw, db, first stage: workgroup (column chunk, row group) = 64 columns x 4 row lanes over the group's rows; row lane l adds the
// rows l, l + 4, .. of the group in order, the four lanes are added in order through LDS.  part[g][0 .. C - 1] = the group's share
// of dw, part[g][C] = its share of db (the column chunk 0 adds it, on the threads of column 0).
__global__ __launch_bounds__(256) void squash_project_dw_kernel(const float* __restrict__ hh, int ldh, const float* __restrict__ dpred,
                                                                long rows, int C, int grp, float* __restrict__ part) {
    __shared__ float sh[256], sb[4];
    const int cl = threadIdx.x & 63, rl = threadIdx.x >> 6;
    const int c = blockIdx.x * 64 + cl;
    const long g = blockIdx.y;
    const long r0 = g * grp, r1 = min(r0 + grp, rows);
    float s = 0.f, b = 0.f;
    for (long r = r0 + rl; r < r1; r += 4) {
        const float d = dpred[r];
        if (c < C) s += d * fmaxf(squash_s(hh[r * ldh + c]), 0.f);
        b += d;
    }
    sh[threadIdx.x] = s;
    if (cl == 0) sb[rl] = b;
    __syncthreads();
    if (rl == 0) {
        if (c < C) part[g * (C + 1) + c] = ((sh[cl] + sh[64 + cl]) + sh[128 + cl]) + sh[192 + cl];
        if (blockIdx.x == 0 && cl == 0) part[g * (C + 1) + C] = ((sb[0] + sb[1]) + sb[2]) + sb[3];
    }
}

// second stage: a thread owns a column (thread C: db) and adds the row groups in order
__global__ __launch_bounds__(256) void squash_project_dw_finish_kernel(const float* __restrict__ part, int groups, int C,
                                                                       float* __restrict__ dw, float* __restrict__ db) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c > C) return;
    float s = 0.f;
    for (int g = 0; g < groups; ++g) s += part[(long)g * (C + 1) + c];
    if (c < C) dw[c] = s;
    else db[0] = s;
}

// rows per group of the first stage: at most 64 groups, at least 16 rows each
static inline int spb_group_rows(int64_t rows) {
    int64_t grp = (rows + 63) / 64;
    return (int)(grp < 16 ? 16 : grp);
}

extern "C" int ssc_squash_project_bwd(const float* hh, int ldh, const float* w, const float* dpred, int64_t rows, int C, float* dh,
                                      float* dw, float* db, float* ws, int64_t ws_bytes, void* stream) {
    if (rows < 1 || C < 4 || (C & 3) || (ldh & 3) || ldh < C) return -1;
    if (rows > 0x7fffffffL / ldh) return -1;
    if (hh == nullptr || w == nullptr || dpred == nullptr || dh == nullptr || dw == nullptr || db == nullptr || ws == nullptr) return -1;
    const int grp = spb_group_rows(rows);
    const int groups = (int)((rows + grp - 1) / grp);
    if (ws_bytes < (int64_t)groups * (C + 1) * (int64_t)sizeof(float)) return -1;
    if (((uintptr_t)hh | (uintptr_t)w | (uintptr_t)dh) & 15) return -3;
    const long total = (long)rows * (ldh / 4);
    long blocks = (total + 255) / 256;
    if (blocks > 2048) blocks = 2048;
    hipLaunchKernelGGL(squash_project_dh_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, hh, ldh, w, dpred,
                       (long)rows, C, dh);
    int rc = CHECK_LAUNCH();
    if (rc != 0) return rc;
    hipLaunchKernelGGL(squash_project_dw_kernel, dim3((unsigned)((C + 63) / 64), (unsigned)groups), dim3(256), 0, (hipStream_t)stream,
                       hh, ldh, dpred, (long)rows, C, grp, ws);
    rc = CHECK_LAUNCH();
    if (rc != 0) return rc;
    hipLaunchKernelGGL(squash_project_dw_finish_kernel, dim3((unsigned)((C + 1 + 255) / 256)), dim3(256), 0, (hipStream_t)stream, ws,
                       groups, C, dw, db);
    return CHECK_LAUNCH();
}
