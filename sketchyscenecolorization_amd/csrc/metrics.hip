// metrics.hip -- full-reference scores of the evaluation modes: sum |a-b|, sum (a-b)^2 and the SSIM sum (Wang et al. 2004) of
// two uint8 [N,H,W,3] batches, per image, optionally under a pixel mask (definitions: include/sketchycolor_hip.h).
//
// A workgroup owns a TH x TW tile of one image's pixels: their absolute and squared differences, and the windows whose CENTRE
// lies in the tile.  It loads the tile with a 5-pixel halo of both images into LDS as bytes, de-interleaved into three planes,
// then per channel runs the horizontal 11-tap pass of the five moments (a, b, a^2, b^2, ab) into LDS and the vertical pass into
// registers, all in double.  Its five sums go to ws; a second launch adds the tiles of an image in a fixed order.  Integers are
// carried as doubles (every one far below 2^53: exact in any order); the SSIM sum is ordered by construction, never by arrival.
//
// Three loaders fill the byte planes, one body reads them.  U8Loader takes the uint8 images of the evaluation modes; F32Loader takes
// float images (the generator's NHWC output buffer, the decode kernel's planar target) and quantises every value on its way into
// the planes with the arithmetic of image_postprocess_u8_kernel (elementwise.hip), so that the uint8 forms never exist in memory.
// BgLoader is the Background module's: the generator's float image, rounded as bg_finish_u8_kernel (bg_io.hip) rounds it, with the
// foreground bytes pasted where the mask is 0, against a uint8 target.
//
// ssc_seg_confusion (the region branch's score) is at the end of the file: integer counts, per-workgroup partials, a fixed fold.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "sketchycolor_hip.h"

#define CHECK_LAUNCH() ((int)hipGetLastError())

namespace {

constexpr int TH = 24, TW = 32;             // the tile, in pixels (256 threads = 8 rows x 32 columns, TH / 8 rows each)
constexpr int R = 5;                        // window radius
constexpr int LR = TH + 2 * R;              // rows with the halo
constexpr int LC = TW + 2 * R;              // columns with the halo
constexpr int LCP = 48;                     // row pitch of a byte plane
constexpr int LANES_PER_ROW = 8;            // lanes that load one row: one 16-byte piece each
static_assert(LC <= LCP && (LC * 3 + 15) / 16 <= LANES_PER_ROW, "a row of the tile is at most LANES_PER_ROW 16-byte pieces");
static_assert(TW == 32 && TH % 8 == 0, "thread (tid >> 5, tid & 31) owns rows tid >> 5 + 8 * i");
static_assert((3 * LR * LCP) % 16 == 0, "the planes are cleared with 16-byte stores");

typedef unsigned char plane_t[LR][LCP];

// One row of the tile (nbytes interleaved bytes at g, the first of them byte p0 of the tile's row) into the three planes.
// The 16-byte aligned middle goes one 16-byte load per lane, what lies in front of it and behind it byte by byte.
__device__ __forceinline__ void load_row(const unsigned char* __restrict__ g, int nbytes, plane_t* s, int r, int p0, int lane) {
    int head = (int)((16u - (unsigned)((uintptr_t)g & 15u)) & 15u);
    if (head > nbytes) head = nbytes;
    const int pieces = (nbytes - head) >> 4;
    const int tail = head + (pieces << 4);
    if (lane < pieces) {
        const int o = head + (lane << 4);
        const uint4 v = *reinterpret_cast<const uint4*>(g + o);
        const unsigned w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int p = p0 + o + i;
            s[p % 3][r][p / 3] = (unsigned char)((w[i >> 2] >> ((i & 3) * 8)) & 0xffu);
        }
    }
    for (int i = lane; i < head; i += LANES_PER_ROW) {
        const int p = p0 + i;
        s[p % 3][r][p / 3] = g[i];
    }
    for (int i = tail + lane; i < nbytes; i += LANES_PER_ROW) {
        const int p = p0 + i;
        s[p % 3][r][p / 3] = g[i];
    }
}

struct U8Loader {
    const unsigned char* a;
    const unsigned char* b;
    // the tile at (y0, x0) of image n with its halo, clipped to the image, into the planes (cleared by the caller)
    __device__ __forceinline__ void operator()(plane_t* sa, plane_t* sb, long n, int y0, int x0, int H, int W, int tid) const {
        const int gx0 = x0 - R < 0 ? 0 : x0 - R;
        const int gx1 = x0 + TW + R > W ? W : x0 + TW + R;
        const int nbytes = (gx1 - gx0) * 3;
        const int p0 = (gx0 - (x0 - R)) * 3;
        for (int r = tid / LANES_PER_ROW; r < LR; r += 256 / LANES_PER_ROW) {
            const int gy = y0 - R + r;
            if (gy < 0 || gy >= H) continue;
            const long off = ((n * H + gy) * W + gx0) * 3;
            load_row(a + off, nbytes, sa, r, p0, tid % LANES_PER_ROW);
            load_row(b + off, nbytes, sb, r, p0, tid % LANES_PER_ROW);
        }
    }
};

// image_postprocess_u8_kernel's value (elementwise.hip): (x + 1) / 2 * 255, each operation rounded to fp32, NaN and what lies
// below 0 to 0, what lies above 255 to 255, then the truncating cast
__device__ __forceinline__ unsigned char quantise(float x) {
    float v = (x + 1.f) / 2.f * 255.f;
    v = fminf(fmaxf(v, 0.f), 255.f);
    return (unsigned char)(int)v;
}

constexpr int F32_ROW_LANES = 16;           // lanes per row of a plane: <= 10 float4 pieces + <= 3 floats in front + <= 3 behind
static_assert((LC + 3) / 4 - 1 + 3 + 3 <= F32_ROW_LANES, "a plane's row is loaded in one pass");

struct F32Loader {
    const float* a;
    int lda, coff_a;
    const float* b;
    int ldb, coff_b;        // (not read when b is planar)
    int b_planar;

    // NHWC rows of ld floats, the image in channels [coff, coff + 3).  ld 4 or 8 on a 16-byte aligned base: the pixel's one
    // or two float4 (which hold the padding channels as well: loaded, never selected); else three floats.
    static __device__ __forceinline__ void nhwc(const float* __restrict__ g, int ld, int coff, plane_t* s, long n, int y0, int x0,
                                                 int H, int W, int tid) {
        const bool wide = (ld == 4 || ld == 8) && ((uintptr_t)g & 15u) == 0;
        for (int it = tid; it < LR * LC; it += 256) {
            const int r = it / LC, x = it - r * LC;
            const int gy = y0 - R + r, gx = x0 - R + x;
            if (gy < 0 || gy >= H || gx < 0 || gx >= W) continue;
            const float* p = g + ((n * H + gy) * W + gx) * ld;
            float v0, v1, v2;
            if (wide) {
                const int first = coff >> 2, last = (coff + 2) >> 2;        // the float4s that hold the image's channels
                const float4 lo = *reinterpret_cast<const float4*>(p + (first << 2));
                float4 hi = make_float4(0.f, 0.f, 0.f, 0.f);
                if (last != first) hi = *reinterpret_cast<const float4*>(p + (last << 2));
                const int o = coff & 3;     // (selects, not an indexed array: the values stay in registers)
                v0 = o == 0 ? lo.x : o == 1 ? lo.y : o == 2 ? lo.z : lo.w;
                v1 = o == 0 ? lo.y : o == 1 ? lo.z : o == 2 ? lo.w : hi.x;
                v2 = o == 0 ? lo.z : o == 1 ? lo.w : o == 2 ? hi.x : hi.y;
            } else {
                v0 = p[coff]; v1 = p[coff + 1]; v2 = p[coff + 2];
            }
            s[0][r][x] = quantise(v0);
            s[1][r][x] = quantise(v1);
            s[2][r][x] = quantise(v2);
        }
    }

    // planar [N,3,H,W]: a row of a plane is count consecutive floats.  Its 16-byte aligned middle goes four pixels per lane,
    // what lies in front of it and behind it float by float.
    static __device__ __forceinline__ void planar(const float* __restrict__ g, plane_t* s, long n, int y0, int x0, int H, int W,
                                                   int tid) {
        const int gx0 = x0 - R < 0 ? 0 : x0 - R;
        const int gx1 = x0 + TW + R > W ? W : x0 + TW + R;
        const int count = gx1 - gx0;
        const int c0 = gx0 - (x0 - R);              // column of the plane the first float goes to
        const int lane = tid % F32_ROW_LANES;
        for (int row = tid / F32_ROW_LANES; row < 3 * LR; row += 256 / F32_ROW_LANES) {
            const int c = row / LR, r = row - c * LR;
            const int gy = y0 - R + r;
            if (gy < 0 || gy >= H) continue;
            const float* p = g + (((n * 3 + c) * H + gy) * W + gx0);
            int head = (int)(((16u - (unsigned)((uintptr_t)p & 15u)) & 15u) >> 2);      // (p is 4-byte aligned)
            if (head > count) head = count;
            const int pieces = (count - head) >> 2;
            const int tail = head + (pieces << 2);
            if (lane < pieces) {
                const int o = head + (lane << 2);
                const float4 v = *reinterpret_cast<const float4*>(p + o);
                s[c][r][c0 + o] = quantise(v.x);
                s[c][r][c0 + o + 1] = quantise(v.y);
                s[c][r][c0 + o + 2] = quantise(v.z);
                s[c][r][c0 + o + 3] = quantise(v.w);
            } else if (lane < pieces + head) {
                const int o = lane - pieces;
                s[c][r][c0 + o] = quantise(p[o]);
            } else if (lane < pieces + head + (count - tail)) {
                const int o = tail + (lane - pieces - head);
                s[c][r][c0 + o] = quantise(p[o]);
            }
        }
    }

    __device__ __forceinline__ void operator()(plane_t* sa, plane_t* sb, long n, int y0, int x0, int H, int W, int tid) const {
        nhwc(a, lda, coff_a, sa, n, y0, x0, H, W, tid);
        if (b_planar) planar(b, sb, n, y0, x0, H, W, tid);
        else nhwc(b, ldb, coff_b, sb, n, y0, x0, H, W, tid);
    }
};

// bg_finish_u8_kernel's value (bg_io.hip: unit_to_u8): floor(clamp((x + 1) / 2, 0, 1) * 255 + 0.5) clamped to 0..255, every
// operation rounded to fp32 on its own (no fused y * 255 + 0.5); fminf / fmaxf drop a NaN operand, so a NaN comes out as 0
__device__ __forceinline__ unsigned char quantise_round(float x) {
#pragma clang fp contract(off)
    const float h = (x + 1.f) / 2.f;
    const float y = fminf(fmaxf(h, 0.f), 1.f) * 255.f;
    const float r = y + 0.5f;
    return (unsigned char)(int)fminf(fmaxf(floorf(r), 0.f), 255.f);
}

// Plane a = bg_finish_u8 of (img, fg, mask), made while it is loaded: the fg pixel where the mask byte is 0, else the rounded
// img pixel (img: rows of ldc floats, the image in channels 0..2; ldc 4 on a 16-byte aligned base: one float4 per pixel).
// Plane b = the uint8 target, row by row as U8Loader loads it.
struct BgLoader {
    const float* img;
    int ldc;
    const unsigned char* fg;
    const unsigned char* target;
    const unsigned char* mask;      // may be null: nothing is pasted, fg is not read

    __device__ __forceinline__ void operator()(plane_t* sa, plane_t* sb, long n, int y0, int x0, int H, int W, int tid) const {
        const int gx0 = x0 - R < 0 ? 0 : x0 - R;
        const int gx1 = x0 + TW + R > W ? W : x0 + TW + R;
        const int nbytes = (gx1 - gx0) * 3;
        const int p0 = (gx0 - (x0 - R)) * 3;
        for (int r = tid / LANES_PER_ROW; r < LR; r += 256 / LANES_PER_ROW) {
            const int gy = y0 - R + r;
            if (gy < 0 || gy >= H) continue;
            load_row(target + ((n * H + gy) * W + gx0) * 3, nbytes, sb, r, p0, tid % LANES_PER_ROW);
        }
        const bool wide = ldc == 4 && ((uintptr_t)img & 15u) == 0;
        for (int it = tid; it < LR * LC; it += 256) {
            const int r = it / LC, x = it - r * LC;
            const int gy = y0 - R + r, gx = x0 - R + x;
            if (gy < 0 || gy >= H || gx < 0 || gx >= W) continue;
            const long pix = (n * H + gy) * W + gx;
            if (mask != nullptr && mask[pix] == 0) {
                const unsigned char* f = fg + pix * 3;
                sa[0][r][x] = f[0];
                sa[1][r][x] = f[1];
                sa[2][r][x] = f[2];
                continue;
            }
            const float* p = img + pix * ldc;
            float v0, v1, v2;
            if (wide) {
                const float4 v = *reinterpret_cast<const float4*>(p);
                v0 = v.x; v1 = v.y; v2 = v.z;
            } else {
                v0 = p[0]; v1 = p[1]; v2 = p[2];
            }
            sa[0][r][x] = quantise_round(v0);
            sa[1][r][x] = quantise_round(v1);
            sa[2][r][x] = quantise_round(v2);
        }
    }
};

// The body all three kernels share: the loader fills the planes, everything behind it reads bytes.
template <class Loader>
__device__ __forceinline__ void image_metrics_tile(const Loader& load, const unsigned char* __restrict__ mask, int H, int W,
                                                   int tiles_x, int tiles_y, const double* __restrict__ win,
                                                   double* __restrict__ partial) {
    __shared__ __attribute__((aligned(16))) unsigned char sa[3][LR][LCP];
    __shared__ __attribute__((aligned(16))) unsigned char sb[3][LR][LCP];
    __shared__ double hb[5][LR][TW];        // the horizontal pass of one channel
    __shared__ double sw[2 * R + 1];
    __shared__ double red[4][5];
    const int tid = threadIdx.x;
    const unsigned blk = blockIdx.x;
    const int tx_i = (int)(blk % (unsigned)tiles_x);
    const int ty_i = (int)((blk / (unsigned)tiles_x) % (unsigned)tiles_y);
    const long n = (long)(blk / ((unsigned)tiles_x * (unsigned)tiles_y));
    const int y0 = ty_i * TH, x0 = tx_i * TW;

    // what lies outside the image reads 0: only windows that are not counted reach it
    for (int i = tid; i < 3 * LR * LCP / 16; i += 256) {
        reinterpret_cast<uint4*>(&sa[0][0][0])[i] = make_uint4(0, 0, 0, 0);
        reinterpret_cast<uint4*>(&sb[0][0][0])[i] = make_uint4(0, 0, 0, 0);
    }
    if (tid < 2 * R + 1) sw[tid] = win[tid];
    __syncthreads();
    load(sa, sb, n, y0, x0, H, W, tid);
    __syncthreads();

    const int tx = tid & 31, tr = tid >> 5;
    unsigned sad = 0, sse = 0, cnt = 0, wcnt = 0;
    bool window[TH / 8];
#pragma unroll
    for (int i = 0; i < TH / 8; ++i) {
        const int ty = tr + 8 * i;
        const int cy = y0 + ty, cx = x0 + tx;
        bool counted = cy < H && cx < W;
        if (counted && mask != nullptr) counted = mask[(n * H + cy) * W + cx] != 0;
        if (counted) {
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const int d = (int)sa[c][ty + R][tx + R] - (int)sb[c][ty + R][tx + R];
                sad += (unsigned)(d < 0 ? -d : d);
                sse += (unsigned)(d * d);
            }
            ++cnt;
        }
        window[i] = counted && cy >= R && cy < H - R && cx >= R && cx < W - R;
        wcnt += window[i];
    }

    const double C1 = (0.01 * 255) * (0.01 * 255), C2 = (0.03 * 255) * (0.03 * 255);
    double ssum = 0.0;
    for (int c = 0; c < 3; ++c) {
        for (int it = tid; it < LR * TW; it += 256) {
            const int r = it >> 5, x = it & 31;
            double ma = 0.0, mb = 0.0, maa = 0.0, mbb = 0.0, mab = 0.0;
#pragma unroll
            for (int k = 0; k < 2 * R + 1; ++k) {
                const int ia = sa[c][r][x + k], ib = sb[c][r][x + k];
                const double w = sw[k];
                ma += w * (double)ia;
                mb += w * (double)ib;
                maa += w * (double)(ia * ia);       // the products are integers: exact
                mbb += w * (double)(ib * ib);
                mab += w * (double)(ia * ib);
            }
            hb[0][r][x] = ma; hb[1][r][x] = mb; hb[2][r][x] = maa; hb[3][r][x] = mbb; hb[4][r][x] = mab;
        }
        __syncthreads();
#pragma unroll
        for (int i = 0; i < TH / 8; ++i) {
            if (!window[i]) continue;
            const int ty = tr + 8 * i;
            double ma = 0.0, mb = 0.0, maa = 0.0, mbb = 0.0, mab = 0.0;
#pragma unroll
            for (int k = 0; k < 2 * R + 1; ++k) {
                const double w = sw[k];
                ma += w * hb[0][ty + k][tx];
                mb += w * hb[1][ty + k][tx];
                maa += w * hb[2][ty + k][tx];
                mbb += w * hb[3][ty + k][tx];
                mab += w * hb[4][ty + k][tx];
            }
            const double va = maa - ma * ma, vb = mbb - mb * mb, cov = mab - ma * mb;
            ssum += ((2.0 * ma * mb + C1) * (2.0 * cov + C2)) / ((ma * ma + mb * mb + C1) * (va + vb + C2));
        }
        __syncthreads();
    }

    double v[5] = {(double)sad, (double)sse, (double)cnt, ssum, (double)wcnt};
#pragma unroll
    for (int k = 0; k < 5; ++k)
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) v[k] += __shfl_down(v[k], o, 64);
    if ((tid & 63) == 0) {
#pragma unroll
        for (int k = 0; k < 5; ++k) red[tid >> 6][k] = v[k];
    }
    __syncthreads();
    if (tid < 5) partial[(long)blk * 5 + tid] = ((red[0][tid] + red[1][tid]) + red[2][tid]) + red[3][tid];
}

__global__ __launch_bounds__(256) void image_metrics_u8_kernel(const unsigned char* __restrict__ a,
                                                                const unsigned char* __restrict__ b,
                                                                const unsigned char* __restrict__ mask, int H, int W,
                                                                int tiles_x, int tiles_y, const double* __restrict__ win,
                                                                double* __restrict__ partial) {
    image_metrics_tile(U8Loader{a, b}, mask, H, W, tiles_x, tiles_y, win, partial);
}

__global__ __launch_bounds__(256) void image_metrics_f32_kernel(F32Loader load, int H, int W, int tiles_x, int tiles_y,
                                                                 const double* __restrict__ win, double* __restrict__ partial) {
    image_metrics_tile(load, nullptr, H, W, tiles_x, tiles_y, win, partial);
}

__global__ __launch_bounds__(256) void image_metrics_bg_f32_kernel(BgLoader load, int H, int W, int tiles_x, int tiles_y,
                                                                    const double* __restrict__ win, double* __restrict__ partial) {
    image_metrics_tile(load, load.mask, H, W, tiles_x, tiles_y, win, partial);
}

// out[n][k] = the sum of image n's tile partials: thread t adds tiles t, t + 256, ... in turn, then the 256 threads are added
// by the same tree every time.
__global__ __launch_bounds__(256) void image_metrics_sum_kernel(const double* __restrict__ partial, int tiles,
                                                                 double* __restrict__ out) {
    __shared__ double red[4][5];
    const int tid = threadIdx.x;
    const double* p = partial + (long)blockIdx.x * tiles * 5;
    double v[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
    for (int t = tid; t < tiles; t += 256) {
#pragma unroll
        for (int k = 0; k < 5; ++k) v[k] += p[(long)t * 5 + k];
    }
#pragma unroll
    for (int k = 0; k < 5; ++k)
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) v[k] += __shfl_down(v[k], o, 64);
    if ((tid & 63) == 0) {
#pragma unroll
        for (int k = 0; k < 5; ++k) red[tid >> 6][k] = v[k];
    }
    __syncthreads();
    if (tid < 5) out[(long)blockIdx.x * 5 + tid] = ((red[0][tid] + red[1][tid]) + red[2][tid]) + red[3][tid];
}

// ---------------------------------------------------------------------------------------------------------------------
// Confusion counts of the region branch.  A workgroup takes every gridDim.x-th run of 256 pixels of one sample; a thread keeps
// the K * K + 1 counts of its pixels in registers (the cell of a pixel is compared against every cell number: no indexed
// array), the 64 lanes of a wave and then the 4 waves are added, and the workgroup's counts go to ws.  A second launch adds a
// sample's workgroups in order.  Integers throughout: any order gives the same counts.
constexpr int CONF_MAX_K = 4;
constexpr int CONF_CELLS = CONF_MAX_K * CONF_MAX_K + 1;
constexpr int CONF_MAX_BLOCKS = 256;        // workgroups per sample
constexpr int CONF_PIXELS = 1024;           // pixels a workgroup takes before a sample gets another one

__host__ __device__ inline long conf_blocks(long P) {
    const long b = (P + CONF_PIXELS - 1) / CONF_PIXELS;
    return b < 1 ? 1 : (b > CONF_MAX_BLOCKS ? CONF_MAX_BLOCKS : b);
}

__global__ __launch_bounds__(256) void seg_confusion_kernel(const float* __restrict__ logits, int ld, int K,
                                                             const int* __restrict__ labels, long P,
                                                             long long* __restrict__ partial) {
    __shared__ unsigned red[4][CONF_CELLS];
    const int tid = threadIdx.x;
    const long n = blockIdx.y;
    const int cells = K * K + 1;
    const bool wide = ld == 4 && ((uintptr_t)logits & 15u) == 0;
    unsigned cnt[CONF_CELLS];
#pragma unroll
    for (int c = 0; c < CONF_CELLS; ++c) cnt[c] = 0;
    for (long i = (long)blockIdx.x * 256 + tid; i < P; i += (long)gridDim.x * 256) {
        const long r = n * P + i;
        const float* z = logits + r * ld;
        float z0, z1 = 0.f, z2 = 0.f, z3 = 0.f;
        if (wide) {
            const float4 v = *reinterpret_cast<const float4*>(z);
            z0 = v.x; z1 = v.y; z2 = v.z; z3 = v.w;
        } else {
            z0 = z[0];
            if (K > 1) z1 = z[1];
            if (K > 2) z2 = z[2];
            if (K > 3) z3 = z[3];
        }
        // the lowest index among the largest logits; strict > from index 0 against -inf: a NaN never wins
        float best = -INFINITY;
        int pred = 0;
        if (z0 > best) { best = z0; pred = 0; }
        if (K > 1 && z1 > best) { best = z1; pred = 1; }
        if (K > 2 && z2 > best) { best = z2; pred = 2; }
        if (K > 3 && z3 > best) { best = z3; pred = 3; }
        const int t = labels[r];
        const int cell = (unsigned)t < (unsigned)K ? t * K + pred : K * K;
#pragma unroll
        for (int c = 0; c < CONF_CELLS; ++c) cnt[c] += (unsigned)(cell == c);
    }
#pragma unroll
    for (int c = 0; c < CONF_CELLS; ++c)
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) cnt[c] += __shfl_down(cnt[c], o, 64);
    if ((tid & 63) == 0) {
#pragma unroll
        for (int c = 0; c < CONF_CELLS; ++c) red[tid >> 6][c] = cnt[c];
    }
    __syncthreads();
    if (tid < cells)
        partial[(n * gridDim.x + blockIdx.x) * cells + tid] =
            (long long)red[0][tid] + (long long)red[1][tid] + (long long)red[2][tid] + (long long)red[3][tid];
}

// out[n][c] = the sum of sample n's workgroup counts (thread c adds them in order)
__global__ __launch_bounds__(64) void seg_confusion_sum_kernel(const long long* __restrict__ partial, int blocks, int cells,
                                                                long long* __restrict__ out) {
    const int c = threadIdx.x;
    if (c >= cells) return;
    const long long* p = partial + (long)blockIdx.x * blocks * cells;
    long long s = 0;
    for (int b = 0; b < blocks; ++b) s += p[(long)b * cells + c];
    out[(long)blockIdx.x * cells + c] = s;
}

}  // namespace

extern "C" int ssc_image_metrics_u8(const uint8_t* a, const uint8_t* b, const uint8_t* mask, int N, int H, int W,
                                    const double* win11, double* out, void* ws, int64_t ws_bytes, void* stream) {
    if (N < 1 || H < 1 || W < 1 || H > (1 << 20) || W > (1 << 20)) return -1;
    const int64_t tiles_y = (H + TH - 1) / TH, tiles_x = (W + TW - 1) / TW;
    const int64_t tiles = tiles_x * tiles_y;
    if (tiles > INT32_MAX || tiles * N > INT32_MAX) return -1;
    if (a == nullptr || b == nullptr || win11 == nullptr || out == nullptr) return -1;
    if (ws == nullptr || ((uintptr_t)ws & 7) || ws_bytes < tiles * N * 5 * (int64_t)sizeof(double)) return -2;
    if (((uintptr_t)win11 & 7) || ((uintptr_t)out & 7)) return -3;
    hipLaunchKernelGGL(image_metrics_u8_kernel, dim3((unsigned)(tiles * N)), dim3(256), 0, (hipStream_t)stream, a, b, mask, H, W,
                       (int)tiles_x, (int)tiles_y, win11, (double*)ws);
    const int rc = CHECK_LAUNCH();
    if (rc != 0) return rc;
    hipLaunchKernelGGL(image_metrics_sum_kernel, dim3((unsigned)N), dim3(256), 0, (hipStream_t)stream, (const double*)ws,
                       (int)tiles, out);
    return CHECK_LAUNCH();
}

extern "C" int ssc_image_metrics_f32(const float* a, int lda, int coff_a, const float* b, int ldb, int coff_b, int b_planar,
                                     int N, int H, int W, const double* win11, double* out, void* ws, int64_t ws_bytes,
                                     void* stream) {
    if (N < 1 || H < 1 || W < 1 || H > (1 << 20) || W > (1 << 20)) return -1;
    if (coff_a < 0 || lda < 3 || coff_a + 3 > lda) return -1;
    if (!b_planar && (coff_b < 0 || ldb < 3 || coff_b + 3 > ldb)) return -1;
    const int64_t tiles_y = (H + TH - 1) / TH, tiles_x = (W + TW - 1) / TW;
    const int64_t tiles = tiles_x * tiles_y;
    if (tiles > INT32_MAX || tiles * N > INT32_MAX) return -1;
    if (a == nullptr || b == nullptr || win11 == nullptr || out == nullptr) return -1;
    if (ws == nullptr || ((uintptr_t)ws & 7) || ws_bytes < tiles * N * 5 * (int64_t)sizeof(double)) return -2;
    if (((uintptr_t)win11 & 7) || ((uintptr_t)out & 7) || ((uintptr_t)a & 3) || ((uintptr_t)b & 3)) return -3;
    const F32Loader load{a, lda, coff_a, b, b_planar ? 0 : ldb, b_planar ? 0 : coff_b, b_planar ? 1 : 0};
    hipLaunchKernelGGL(image_metrics_f32_kernel, dim3((unsigned)(tiles * N)), dim3(256), 0, (hipStream_t)stream, load, H, W,
                       (int)tiles_x, (int)tiles_y, win11, (double*)ws);
    const int rc = CHECK_LAUNCH();
    if (rc != 0) return rc;
    hipLaunchKernelGGL(image_metrics_sum_kernel, dim3((unsigned)N), dim3(256), 0, (hipStream_t)stream, (const double*)ws,
                       (int)tiles, out);
    return CHECK_LAUNCH();
}

extern "C" int ssc_image_metrics_bg_f32(const float* img, int ldc, const uint8_t* fg, const uint8_t* target, const uint8_t* mask,
                                        int N, int H, int W, const double* win11, double* out, void* ws, int64_t ws_bytes,
                                        void* stream) {
    if (N < 1 || H < 1 || W < 1 || H > (1 << 20) || W > (1 << 20)) return -1;
    if (ldc < 3) return -1;
    const int64_t tiles_y = (H + TH - 1) / TH, tiles_x = (W + TW - 1) / TW;
    const int64_t tiles = tiles_x * tiles_y;
    if (tiles > INT32_MAX || tiles * N > INT32_MAX) return -1;
    if (img == nullptr || target == nullptr || win11 == nullptr || out == nullptr) return -1;
    if (mask != nullptr && fg == nullptr) return -1;
    if (ws == nullptr || ((uintptr_t)ws & 7) || ws_bytes < tiles * N * 5 * (int64_t)sizeof(double)) return -2;
    if (((uintptr_t)win11 & 7) || ((uintptr_t)out & 7) || ((uintptr_t)img & 3)) return -3;
    const BgLoader load{img, ldc, fg, target, mask};
    hipLaunchKernelGGL(image_metrics_bg_f32_kernel, dim3((unsigned)(tiles * N)), dim3(256), 0, (hipStream_t)stream, load, H, W,
                       (int)tiles_x, (int)tiles_y, win11, (double*)ws);
    const int rc = CHECK_LAUNCH();
    if (rc != 0) return rc;
    hipLaunchKernelGGL(image_metrics_sum_kernel, dim3((unsigned)N), dim3(256), 0, (hipStream_t)stream, (const double*)ws,
                       (int)tiles, out);
    return CHECK_LAUNCH();
}

extern "C" int ssc_seg_confusion(const float* logits, int ld, int K, const int32_t* labels, int64_t N, int64_t P, int64_t* out,
                                 void* ws, int64_t ws_bytes, void* stream) {
    if (K < 1 || K > CONF_MAX_K || ld < K) return -1;
    if (N < 1 || P < 1 || N > 65535 || P > INT32_MAX) return -1;
    if (logits == nullptr || labels == nullptr || out == nullptr) return -1;
    const int64_t blocks = conf_blocks((long)P), cells = (int64_t)K * K + 1;
    if (ws == nullptr || ((uintptr_t)ws & 7) || ws_bytes < N * blocks * cells * (int64_t)sizeof(int64_t)) return -2;
    if (((uintptr_t)logits & 3) || ((uintptr_t)labels & 3) || ((uintptr_t)out & 7)) return -3;
    hipLaunchKernelGGL(seg_confusion_kernel, dim3((unsigned)blocks, (unsigned)N), dim3(256), 0, (hipStream_t)stream, logits, ld,
                       K, labels, (long)P, (long long*)ws);
    const int rc = CHECK_LAUNCH();
    if (rc != 0) return rc;
    hipLaunchKernelGGL(seg_confusion_sum_kernel, dim3((unsigned)N), dim3(64), 0, (hipStream_t)stream, (const long long*)ws,
                       (int)blocks, (int)cells, (long long*)out);
    return CHECK_LAUNCH();
}
