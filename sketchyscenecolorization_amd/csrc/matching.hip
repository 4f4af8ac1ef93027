// matching.hip -- the data movement and the finishing steps of the instance matcher (Instance_Matching/RMI_model.py in eval mode
// on the DeepLab-ResNet backbone, Pipeline_utils/fg_matching_utils.py::build_instance_matching).  The convs,
// the matmuls and the two LSTMs are the kernels the generators already use; what is here is what they lack: the sketch bytes
// to the backbone's input, the backbone's max-pool, the rearrangement that turns an atrous conv into a plain one, the 500 -> 1
// projection of the squashed state, the legacy bilinear upsampling with the threshold, and the per-instance counts.
// All of it is memory-bound: 16-byte accesses along the channel axis (or along a row of pixels), grid-stride loops over at most
// 2048 workgroups, no LDS beyond the two small reductions.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "sketchycolor_hip.h"
#include "match_up.h"

#define CHECK_LAUNCH() ((int)hipGetLastError())
#define MAX_PIXELS (1 << 24)

typedef unsigned char u8;

static inline unsigned blocks_for(long n) {
    long blocks = (n + 255) / 256;
    if (blocks < 1) blocks = 1;
    return (unsigned)(blocks > 2048 ? 2048 : blocks);
}

// ---------------------------------------------------------------------------------------------------------------------------
// sketch bytes -> the backbone's input: out[p] = (byte_r - mu_0, byte_g - mu_1, byte_b - mu_2, 0); stroke[p] = byte_r != 255
// ---------------------------------------------------------------------------------------------------------------------------
// mu is subtracted from the channels in RGB order, as the reference does (its constants are the BGR means of the Caffe model).
__global__ __launch_bounds__(256) void match_preprocess_kernel(const u8* __restrict__ src, long n, float* __restrict__ out,
                                                               u8* __restrict__ stroke) {
    for (long p = (long)blockIdx.x * 256 + threadIdx.x; p < n; p += (long)gridDim.x * 256) {
        const u8 r = src[p * 3], g = src[p * 3 + 1], b = src[p * 3 + 2];
        float4 v;
        v.x = (float)r - 104.00698793f;
        v.y = (float)g - 116.66876762f;
        v.z = (float)b - 122.67891434f;
        v.w = 0.f;
        *reinterpret_cast<float4*>(out + p * 4) = v;
        stroke[p] = r != 255 ? (u8)1 : (u8)0;
    }
}

extern "C" int ssc_match_preprocess_u8(const uint8_t* src, int H, int W, float* out, uint8_t* stroke, void* stream) {
    if (H < 1 || W < 1 || (int64_t)H * W > MAX_PIXELS) return -1;
    if (src == nullptr || out == nullptr || stroke == nullptr) return -1;
    if ((uintptr_t)out & 15) return -3;
    const long n = (long)H * W;
    hipLaunchKernelGGL(match_preprocess_kernel, dim3(blocks_for(n)), dim3(256), 0, (hipStream_t)stream, src, n, out, stroke);
    return CHECK_LAUNCH();
}

// ---------------------------------------------------------------------------------------------------------------------------
// tf.nn.max_pool(relu(a * x + b), 3 x 3, stride 2, SAME), NHWC; a thread owns four channels of one output pixel
// ---------------------------------------------------------------------------------------------------------------------------
// SAME: OH = ceil(H / 2), padding max((OH - 1) * 2 + 3 - H, 0) with the smaller half in front -- one row at the bottom for an
// even H and none on top, one on either side for an odd H.  Taps in the padding do not take part in the maximum.
__global__ __launch_bounds__(256) void max_pool3s2_kernel(const float* __restrict__ x, const float* __restrict__ ab, int H, int W,
                                                          int C, int OH, int OW, int py, int px, long total,
                                                          float* __restrict__ out) {
    const int c4n = C >> 2;
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
        float4 m = make_float4(-INFINITY, -INFINITY, -INFINITY, -INFINITY);
#pragma unroll
        for (int ky = 0; ky < 3; ++ky) {
            const int y = oy * 2 - py + ky;
            if (y < 0 || y >= H) continue;
#pragma unroll
            for (int kx = 0; kx < 3; ++kx) {
                const int xx = ox * 2 - px + kx;
                if (xx < 0 || xx >= W) continue;
                float4 v = *reinterpret_cast<const float4*>(x + ((n * H + y) * W + xx) * C + c);
                if (ab != nullptr) {
                    v.x = fmaxf(fmaf(a.x, v.x, b.x), 0.f);
                    v.y = fmaxf(fmaf(a.y, v.y, b.y), 0.f);
                    v.z = fmaxf(fmaf(a.z, v.z, b.z), 0.f);
                    v.w = fmaxf(fmaf(a.w, v.w, b.w), 0.f);
                }
                m.x = fmaxf(m.x, v.x);
                m.y = fmaxf(m.y, v.y);
                m.z = fmaxf(m.z, v.z);
                m.w = fmaxf(m.w, v.w);
            }
        }
        *reinterpret_cast<float4*>(out + t * 4) = m;
    }
}

extern "C" int ssc_max_pool3s2(const float* x, const float* ab, int N, int H, int W, int C, float* out, void* stream) {
    if (N < 1 || H < 1 || W < 1 || C < 4 || (C & 3)) return -1;
    if (x == nullptr || out == nullptr) return -1;
    if (((uintptr_t)x | (uintptr_t)out | (uintptr_t)ab) & 15) return -3;
    const int OH = (H + 1) / 2, OW = (W + 1) / 2;
    const int ph = (OH - 1) * 2 + 3 - H, pw = (OW - 1) * 2 + 3 - W;
    const int64_t total = (int64_t)N * OH * OW * (C / 4);
    if ((int64_t)N * H * W * C > 0x7fffffffL * 4L) return -1;
    hipLaunchKernelGGL(max_pool3s2_kernel, dim3(blocks_for(total)), dim3(256), 0, (hipStream_t)stream, x, ab, H, W, C, OH, OW,
                       (ph > 0 ? ph : 0) / 2, (pw > 0 ? pw : 0) / 2, (long)total, out);
    return CHECK_LAUNCH();
}

// ---------------------------------------------------------------------------------------------------------------------------
// space_to_batch / batch_to_space: [N, H, W, C] <-> [N * r * r, H / r, W / r, C]; sub-image n * r * r + i * r + j holds the pixels
// (y = i mod r, x = j mod r) of image n.  Pure moves of 16 bytes; the same index walk either way.
// ---------------------------------------------------------------------------------------------------------------------------
template <bool TO_BATCH>
__global__ __launch_bounds__(256) void space_batch_kernel(const float* __restrict__ src, int H, int W, int C, int r, long total,
                                                          float* __restrict__ dst) {
    const int c4n = C >> 2, h = H / r, w = W / r;
    for (long t = (long)blockIdx.x * 256 + threadIdx.x; t < total; t += (long)gridDim.x * 256) {
        // t walks the batched tensor [N * r * r][h][w][C / 4]
        const int c = (int)(t % c4n) * 4;
        long q = t / c4n;
        const int xs = (int)(q % w);
        q /= w;
        const int ys = (int)(q % h);
        q /= h;
        const int j = (int)(q % r);
        q /= r;
        const int i = (int)(q % r);
        const long n = q / r;
        const long sp = ((n * H + (long)ys * r + i) * W + (long)xs * r + j) * C + c;
        if (TO_BATCH)
            *reinterpret_cast<float4*>(dst + t * 4) = *reinterpret_cast<const float4*>(src + sp);
        else
            *reinterpret_cast<float4*>(dst + sp) = *reinterpret_cast<const float4*>(src + t * 4);
    }
}

static int space_batch_check(const float* a, const float* b, int N, int H, int W, int C, int r) {
    if (N < 1 || H < 1 || W < 1 || C < 4 || (C & 3)) return -1;
    if (r != 2 && r != 4) return -1;
    if ((H % r) || (W % r)) return -1;
    if ((int64_t)N * H * W * C > 0x7fffffffL * 4L) return -1;
    if (a == nullptr || b == nullptr || a == b) return -1;
    if (((uintptr_t)a | (uintptr_t)b) & 15) return -3;
    return 0;
}

extern "C" int ssc_space_to_batch(const float* x, int N, int H, int W, int C, int r, float* out, void* stream) {
    const int rc = space_batch_check(x, out, N, H, W, C, r);
    if (rc != 0) return rc;
    const long total = (long)N * H * W * (C / 4);
    hipLaunchKernelGGL((space_batch_kernel<true>), dim3(blocks_for(total)), dim3(256), 0, (hipStream_t)stream, x, H, W, C, r, total,
                       out);
    return CHECK_LAUNCH();
}

// x [N * r * r, H / r, W / r, C] -> out [N, H, W, C]  (N, H, W: the shape of the OUTPUT)
extern "C" int ssc_batch_to_space(const float* x, int N, int H, int W, int C, int r, float* out, void* stream) {
    const int rc = space_batch_check(x, out, N, H, W, C, r);
    if (rc != 0) return rc;
    const long total = (long)N * H * W * (C / 4);
    hipLaunchKernelGGL((space_batch_kernel<false>), dim3(blocks_for(total)), dim3(256), 0, (hipStream_t)stream, x, H, W, C, r,
                       total, out);
    return CHECK_LAUNCH();
}

// ---------------------------------------------------------------------------------------------------------------------------
// out[row] = sum_c relu(0.5 * (log(1 + 1e-3 + h) - log(1 + 1e-3 - h))) * w[c] + bias[0]: the squash and the m_lstm_output_projection
// ---------------------------------------------------------------------------------------------------------------------------
// One wavefront per row: lane l adds the channels 4 l, 4 l + 1, .. of every 256-channel stretch in order, then the butterfly
// over the 64 lanes -- the same order on every run.
__global__ __launch_bounds__(256) void squash_project_kernel(const float* __restrict__ h, int ldh, const float* __restrict__ w,
                                                             const float* __restrict__ bias, long rows, int C,
                                                             float* __restrict__ out) {
    const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (row >= rows) return;
    float s = 0.f;
    for (int c = lane * 4; c < C; c += 256) {
        const float4 v = *reinterpret_cast<const float4*>(h + row * ldh + c);
        const float4 k = *reinterpret_cast<const float4*>(w + c);
        s += fmaxf(0.5f * (logf(1.0f + 1e-3f + v.x) - logf(1.0f + 1e-3f - v.x)), 0.f) * k.x;
        s += fmaxf(0.5f * (logf(1.0f + 1e-3f + v.y) - logf(1.0f + 1e-3f - v.y)), 0.f) * k.y;
        s += fmaxf(0.5f * (logf(1.0f + 1e-3f + v.z) - logf(1.0f + 1e-3f - v.z)), 0.f) * k.z;
        s += fmaxf(0.5f * (logf(1.0f + 1e-3f + v.w) - logf(1.0f + 1e-3f - v.w)), 0.f) * k.w;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    if (lane == 0) out[row] = s + bias[0];
}

extern "C" int ssc_squash_project(const float* h, int ldh, const float* w, const float* bias, int64_t rows, int C, float* out,
                                  void* stream) {
    if (rows < 1 || C < 4 || (C & 3) || (ldh & 3) || ldh < C) return -1;
    if (rows > 0x7fffffffL / ldh) return -1;
    if (h == nullptr || w == nullptr || bias == nullptr || out == nullptr) return -1;
    if (((uintptr_t)h | (uintptr_t)w) & 15) return -3;
    hipLaunchKernelGGL(squash_project_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, (hipStream_t)stream, h, ldh, w, bias,
                       (long)rows, C, out);
    return CHECK_LAUNCH();
}

// ---------------------------------------------------------------------------------------------------------------------------
// tf.image.resize_bilinear(pred, [S, S]) in the legacy form (align_corners = False) and predicts = (up >= 1e-9) * stroke
// ---------------------------------------------------------------------------------------------------------------------------
// The value of a pixel is match_up.h's match_up_value, which ssc_match_score (match_val.hip) calls too.  A thread owns four
// neighbouring pixels of a row: one 16-byte store of up, one 4-byte store of predicts.
__global__ __launch_bounds__(256) void match_finish_kernel(const float* __restrict__ pred, int h, int w, const u8* __restrict__ stroke,
                                                           int S, float sy, float sx, float* __restrict__ up,
                                                           u8* __restrict__ predicts) {
    const int q4 = S >> 2;
    const long total = (long)S * q4;
    for (long t = (long)blockIdx.x * 256 + threadIdx.x; t < total; t += (long)gridDim.x * 256) {
        const int y = (int)(t / q4), x0 = (int)(t - (long)y * q4) * 4;
        int ylo, yhi;
        float wy;
        match_up_axis(y, sy, h, ylo, yhi, wy);
        const uchar4 st = *reinterpret_cast<const uchar4*>(stroke + (long)y * S + x0);
        const u8 sb[4] = {st.x, st.y, st.z, st.w};
        float o[4];
        u8 p[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            o[k] = match_up_value(pred, w, ylo, yhi, wy, x0 + k, sx);
            p[k] = (o[k] >= 1e-9f && sb[k] != 0) ? (u8)1 : (u8)0;
        }
        *reinterpret_cast<float4*>(up + (long)y * S + x0) = make_float4(o[0], o[1], o[2], o[3]);
        *reinterpret_cast<uchar4*>(predicts + (long)y * S + x0) = make_uchar4(p[0], p[1], p[2], p[3]);
    }
}

extern "C" int ssc_match_finish(const float* pred, int h, int w, const uint8_t* stroke, int S, float* up, uint8_t* predicts,
                                void* stream) {
    if (h < 1 || w < 1 || S < 4 || (S & 3) || (int64_t)S * S > MAX_PIXELS || h > S || w > S) return -1;
    if (pred == nullptr || stroke == nullptr || up == nullptr || predicts == nullptr) return -1;
    if (((uintptr_t)up & 15) || ((uintptr_t)stroke & 3) || ((uintptr_t)predicts & 3)) return -3;
    hipLaunchKernelGGL(match_finish_kernel, dim3(blocks_for((long)S * (S / 4))), dim3(256), 0, (hipStream_t)stream, pred, h, w, stroke,
                       S, (float)h / (float)S, (float)w / (float)S, up, predicts);
    return CHECK_LAUNCH();
}

// ---------------------------------------------------------------------------------------------------------------------------
// compute_mask_occupied_percentage's two sums per instance: out[k] = {#(predicts != 0 and mask != 0), sum of the mask's bytes}
// ---------------------------------------------------------------------------------------------------------------------------
// The small mask of instance k is masks[offsets[k] ..], (y2 - y1 + 1) rows of (x2 - x1 + 1) bytes, laid at (y1, x1).  One
// workgroup per instance; integer sums over the lanes, the wavefronts in a fixed order.  A box that is empty, leaves the image or
// whose mask leaves the buffer gives {-1, -1} and reads nothing.
__global__ __launch_bounds__(256) void instance_occupancy_kernel(const u8* __restrict__ predicts, int S, const u8* __restrict__ masks,
                                                                 long mask_bytes, const int* __restrict__ boxes,
                                                                 const long* __restrict__ offsets, long* __restrict__ out) {
    __shared__ unsigned long long part[2][4];
    const int k = blockIdx.x;
    const int y1 = boxes[k * 4], x1 = boxes[k * 4 + 1], y2 = boxes[k * 4 + 2], x2 = boxes[k * 4 + 3];
    const long off = offsets[k];
    const long bh = (long)y2 - y1 + 1, bw = (long)x2 - x1 + 1;
    if (y1 < 0 || x1 < 0 || y2 >= S || x2 >= S || bh < 1 || bw < 1 || off < 0 || off + bh * bw > mask_bytes) {
        if (threadIdx.x == 0) out[k * 2] = out[k * 2 + 1] = -1;
        return;
    }
    unsigned long long inter = 0, area = 0;
    const long n = bh * bw;
    for (long p = threadIdx.x; p < n; p += 256) {
        const long i = p / bw, j = p - i * bw;
        const unsigned m = masks[off + p];
        area += m;
        inter += (m != 0 && predicts[(y1 + i) * S + x1 + j] != 0) ? 1 : 0;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        inter += __shfl_down(inter, o, 64);
        area += __shfl_down(area, o, 64);
    }
    if ((threadIdx.x & 63) == 0) {
        part[0][threadIdx.x >> 6] = inter;
        part[1][threadIdx.x >> 6] = area;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        out[k * 2] = (long)(part[0][0] + part[0][1] + part[0][2] + part[0][3]);
        out[k * 2 + 1] = (long)(part[1][0] + part[1][1] + part[1][2] + part[1][3]);
    }
}

extern "C" int ssc_instance_occupancy(const uint8_t* predicts, int S, const uint8_t* masks, int64_t mask_bytes, const int32_t* boxes,
                                      const int64_t* offsets, int N, int64_t* out, void* stream) {
    if (S < 1 || (int64_t)S * S > MAX_PIXELS || N < 1 || N > 65535 || mask_bytes < 1) return -1;
    if (predicts == nullptr || masks == nullptr || boxes == nullptr || offsets == nullptr || out == nullptr) return -1;
    if (((uintptr_t)boxes & 3) || ((uintptr_t)offsets & 7) || ((uintptr_t)out & 7)) return -3;
    hipLaunchKernelGGL(instance_occupancy_kernel, dim3((unsigned)N), dim3(256), 0, (hipStream_t)stream, predicts, S, masks,
                       (long)mask_bytes, boxes, (const long*)offsets, (long*)out);
    return CHECK_LAUNCH();
}
