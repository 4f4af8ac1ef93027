// color_metrics.hip -- colour scores of two uint8 [N,H,W,3] batches, per image, optionally under a pixel mask: the sums of the
// CIELAB errors dE (CIE76), dab and |dL|, the integer sums colourfulness (Hasler & Suesstrunk 2003) is made of, and the
// intersection of the two 23 x 23 histograms of (a*, b*) (definitions: include/sketchycolor_hip.h).
//
// No pixel looks at its neighbours, so an image is a run of H * W pixels and a workgroup owns CHUNK consecutive ones: thread t
// takes pixels t, t + 256, ... of the chunk in turn.  sRGB -> linear is a 256-entry double table the host makes (no pow on the
// device); XYZ, f and Lab are double with every operation rounded on its own (no contraction: the three kernels run the same
// arithmetic whatever the compiler inlines).  The three float sums and the nine integer sums (carried as doubles, all far below
// 2^53) go to ws per chunk; a second launch adds an image's chunks in a fixed order: the same bits from run to run.  The
// histograms are counted in LDS per workgroup and added to the image's counts in ws with integer atomics -- any order gives the
// same counts -- and the second launch forms sum min(hist_a, hist_b).
//
// Three loaders hand a pixel's six bytes to one body.  U8Pixel reads the uint8 images of the evaluation modes; F32Pixel reads float
// images and quantises with the arithmetic of image_postprocess_u8_kernel (elementwise.hip); BgPixel quantises the Background
// generator's float image as bg_finish_u8_kernel (bg_io.hip) rounds it, against a uint8 target.  These restate the loaders of
// metrics.hip one pixel at a time (no halo, no planes).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "sketchycolor_hip.h"

#pragma clang fp contract(off)

#define CHECK_LAUNCH() ((int)hipGetLastError())

namespace {

constexpr int CHUNK = 1024;                 // pixels a workgroup owns (256 threads, CHUNK / 256 pixels each)
constexpr int SUMS = 12;                    // slots 0..11 of out: what a chunk writes to ws
constexpr int BINS = 23;                    // cells per axis of the ab histogram
constexpr int CELLS = BINS * BINS;
static_assert(CHUNK % 256 == 0, "thread t takes pixels t + 256 * i of its chunk");
static_assert((long)CHUNK * 510 * 510 < (1l << 31), "a thread's integer sums fit an int");

struct Bytes {
    int r, g, b;
};

struct U8Pixel {
    const unsigned char* a;
    const unsigned char* b;
    __device__ __forceinline__ void operator()(long pix, long, long, Bytes& pa, Bytes& pb) const {
        const unsigned char* x = a + pix * 3;
        const unsigned char* y = b + pix * 3;
        pa = Bytes{x[0], x[1], x[2]};
        pb = Bytes{y[0], y[1], y[2]};
    }
};

// image_postprocess_u8_kernel's value (elementwise.hip): (x + 1) / 2 * 255, each operation rounded to fp32, NaN and what lies
// below 0 to 0, what lies above 255 to 255, then the truncating cast
__device__ __forceinline__ int quantise(float x) {
    float v = (x + 1.f) / 2.f * 255.f;
    v = fminf(fmaxf(v, 0.f), 255.f);
    return (int)(unsigned char)(int)v;
}

// bg_finish_u8_kernel's value (bg_io.hip: unit_to_u8): floor(clamp((x + 1) / 2, 0, 1) * 255 + 0.5) clamped to 0..255, every
// operation rounded to fp32 on its own; fminf / fmaxf drop a NaN operand, so a NaN comes out as 0
__device__ __forceinline__ int quantise_round(float x) {
    const float h = (x + 1.f) / 2.f;
    const float y = fminf(fmaxf(h, 0.f), 1.f) * 255.f;
    const float r = y + 0.5f;
    return (int)(unsigned char)(int)fminf(fmaxf(floorf(r), 0.f), 255.f);
}

struct F32Pixel {
    const float* a;
    int lda, coff_a;
    const float* b;
    int ldb, coff_b;        // (not read when b is planar)
    int b_planar;

    // a pixel of NHWC rows of ld floats, the image in channels [coff, coff + 3).  ld 4 or 8 on a 16-byte aligned base: the
    // pixel's one or two float4 (the padding channels are loaded, never selected); else three floats.
    static __device__ __forceinline__ Bytes nhwc(const float* __restrict__ g, int ld, int coff, long pix) {
        const float* p = g + pix * ld;
        float v0, v1, v2;
        if ((ld == 4 || ld == 8) && ((uintptr_t)g & 15u) == 0) {
            const int first = coff >> 2, last = (coff + 2) >> 2;
            const float4 lo = *reinterpret_cast<const float4*>(p + (first << 2));
            float4 hi = make_float4(0.f, 0.f, 0.f, 0.f);
            if (last != first) hi = *reinterpret_cast<const float4*>(p + (last << 2));
            const int o = coff & 3;
            v0 = o == 0 ? lo.x : o == 1 ? lo.y : o == 2 ? lo.z : lo.w;
            v1 = o == 0 ? lo.y : o == 1 ? lo.z : o == 2 ? lo.w : hi.x;
            v2 = o == 0 ? lo.z : o == 1 ? lo.w : o == 2 ? hi.x : hi.y;
        } else {
            v0 = p[coff]; v1 = p[coff + 1]; v2 = p[coff + 2];
        }
        return Bytes{quantise(v0), quantise(v1), quantise(v2)};
    }

    // pix = n * P + i: pixel i of image n of P pixels
    __device__ __forceinline__ void operator()(long pix, long n, long P, Bytes& pa, Bytes& pb) const {
        pa = nhwc(a, lda, coff_a, pix);
        if (b_planar) {
            const float* p = b + n * 3 * P + (pix - n * P);     // planar [N,3,H,W]: the planes of image n lie P floats apart
            pb = Bytes{quantise(p[0]), quantise(p[P]), quantise(p[2 * P])};
        } else {
            pb = nhwc(b, ldb, coff_b, pix);
        }
    }
};

// Image a = bg_finish_u8 of (img, fg, mask) at a COUNTED pixel.  bg_finish_u8 writes the fg byte exactly where the mask byte is
// 0, and those are the pixels the mask leaves uncounted: no pixel of fg can enter a sum, and fg is not read.
struct BgPixel {
    const float* img;
    int ldc;
    const unsigned char* target;
    __device__ __forceinline__ void operator()(long pix, long, long, Bytes& pa, Bytes& pb) const {
        const float* p = img + pix * ldc;
        float v0, v1, v2;
        if (ldc == 4 && ((uintptr_t)img & 15u) == 0) {
            const float4 v = *reinterpret_cast<const float4*>(p);
            v0 = v.x; v1 = v.y; v2 = v.z;
        } else {
            v0 = p[0]; v1 = p[1]; v2 = p[2];
        }
        pa = Bytes{quantise_round(v0), quantise_round(v1), quantise_round(v2)};
        const unsigned char* y = target + pix * 3;
        pb = Bytes{y[0], y[1], y[2]};
    }
};

struct Lab {
    double L, a, b;
};

__device__ __forceinline__ double lab_f(double t) {
    const double d = 6.0 / 29.0;
    return t > d * d * d ? cbrt(t) : t / (3.0 * d * d) + 4.0 / 29.0;
}

__device__ __forceinline__ Lab lab_of(const Bytes& p, const double* lin) {
    const double r = lin[p.r], g = lin[p.g], b = lin[p.b];
    const double X = (0.412453 * r + 0.357580 * g + 0.180423 * b) / 0.95047;
    const double Y = (0.212671 * r + 0.715160 * g + 0.072169 * b) / 1.0;
    const double Z = (0.019334 * r + 0.119193 * g + 0.950227 * b) / 1.08883;
    const double fx = lab_f(X), fy = lab_f(Y), fz = lab_f(Z);
    return Lab{116.0 * fy - 16.0, 500.0 * (fx - fy), 200.0 * (fy - fz)};
}

// clamp(floor((v + 115) / 10), 0, 22)
__device__ __forceinline__ int ab_cell(double v) {
    const double c = floor((v + 115.0) / 10.0);
    return c < 0.0 ? 0 : (c > (double)(BINS - 1) ? BINS - 1 : (int)c);
}

// The body all three kernels share: the loader hands over bytes, everything behind it reads bytes.
// partial: [blocks][SUMS] doubles; hist: [N][2][CELLS] counts, zero before the launch.
template <class Loader>
__device__ __forceinline__ void color_metrics_chunk(const Loader& load, const unsigned char* __restrict__ mask, long P,
                                                    int chunks, const double* __restrict__ lin256,
                                                    double* __restrict__ partial, unsigned long long* __restrict__ hist) {
    __shared__ double slin[256];
    __shared__ unsigned sh[2][CELLS];
    __shared__ double red[4][SUMS];
    const int tid = threadIdx.x;
    const unsigned blk = blockIdx.x;
    const long n = (long)(blk / (unsigned)chunks);
    const long first = (long)(blk % (unsigned)chunks) * CHUNK;

    slin[tid] = lin256[tid];
    for (int i = tid; i < 2 * CELLS; i += 256) (&sh[0][0])[i] = 0u;
    __syncthreads();

    double sde = 0.0, sdab = 0.0, sdl = 0.0;
    int cnt = 0, s[8] = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
    for (int i = 0; i < CHUNK / 256; ++i) {
        const long in_image = first + i * 256 + tid;
        if (in_image >= P) continue;
        const long pix = n * P + in_image;
        if (mask != nullptr && mask[pix] == 0) continue;
        Bytes pa, pb;
        load(pix, n, P, pa, pb);
        const Lab la = lab_of(pa, slin), lb = lab_of(pb, slin);
        const double dL = la.L - lb.L, da = la.a - lb.a, db = la.b - lb.b;
        const double ab2 = da * da + db * db;
        sde += sqrt(dL * dL + ab2);
        sdab += sqrt(ab2);
        sdl += fabs(dL);
        ++cnt;
        const int rga = pa.r - pa.g, yba = pa.r + pa.g - 2 * pa.b;
        const int rgb = pb.r - pb.g, ybb = pb.r + pb.g - 2 * pb.b;
        s[0] += rga; s[1] += rga * rga; s[2] += yba; s[3] += yba * yba;
        s[4] += rgb; s[5] += rgb * rgb; s[6] += ybb; s[7] += ybb * ybb;
        atomicAdd(&sh[0][ab_cell(la.a) * BINS + ab_cell(la.b)], 1u);
        atomicAdd(&sh[1][ab_cell(lb.a) * BINS + ab_cell(lb.b)], 1u);
    }

    double v[SUMS] = {sde, sdab, sdl, (double)cnt, (double)s[0], (double)s[1], (double)s[2], (double)s[3],
                      (double)s[4], (double)s[5], (double)s[6], (double)s[7]};
#pragma unroll
    for (int k = 0; k < SUMS; ++k)
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) v[k] += __shfl_down(v[k], o, 64);
    if ((tid & 63) == 0) {
#pragma unroll
        for (int k = 0; k < SUMS; ++k) red[tid >> 6][k] = v[k];
    }
    __syncthreads();        // (the LDS histograms are complete behind it as well)
    if (tid < SUMS) partial[(long)blk * SUMS + tid] = ((red[0][tid] + red[1][tid]) + red[2][tid]) + red[3][tid];
    unsigned long long* h = hist + n * 2 * CELLS;
    for (int i = tid; i < 2 * CELLS; i += 256) {
        const unsigned c = (&sh[0][0])[i];
        if (c != 0) atomicAdd(&h[i], (unsigned long long)c);
    }
}

__global__ __launch_bounds__(256) void color_metrics_u8_kernel(const unsigned char* __restrict__ a,
                                                               const unsigned char* __restrict__ b,
                                                               const unsigned char* __restrict__ mask, long P, int chunks,
                                                               const double* __restrict__ lin256, double* __restrict__ partial,
                                                               unsigned long long* __restrict__ hist) {
    color_metrics_chunk(U8Pixel{a, b}, mask, P, chunks, lin256, partial, hist);
}

__global__ __launch_bounds__(256) void color_metrics_f32_kernel(F32Pixel load, long P, int chunks,
                                                                const double* __restrict__ lin256, double* __restrict__ partial,
                                                                unsigned long long* __restrict__ hist) {
    color_metrics_chunk(load, nullptr, P, chunks, lin256, partial, hist);
}

__global__ __launch_bounds__(256) void color_metrics_bg_f32_kernel(BgPixel load, const unsigned char* __restrict__ mask, long P,
                                                                   int chunks, const double* __restrict__ lin256,
                                                                   double* __restrict__ partial,
                                                                   unsigned long long* __restrict__ hist) {
    color_metrics_chunk(load, mask, P, chunks, lin256, partial, hist);
}

// out[n][k], k < 12 = the sum of image n's chunk partials: thread t adds chunks t, t + 256, ... in turn, then the 256 threads are
// added by the same tree every time.  out[n][12] = sum over the cells of min(hist_a, hist_b); hist_out (may be null) = the counts.
__global__ __launch_bounds__(256) void color_metrics_sum_kernel(const double* __restrict__ partial, int chunks,
                                                                const unsigned long long* __restrict__ hist,
                                                                double* __restrict__ out, long long* __restrict__ hist_out) {
    __shared__ double red[4][SUMS];
    __shared__ unsigned long long common;
    const int tid = threadIdx.x;
    const long n = blockIdx.x;
    if (tid == 0) common = 0ull;
    const double* p = partial + n * chunks * SUMS;
    double v[SUMS];
#pragma unroll
    for (int k = 0; k < SUMS; ++k) v[k] = 0.0;
    for (int t = tid; t < chunks; t += 256) {
#pragma unroll
        for (int k = 0; k < SUMS; ++k) v[k] += p[(long)t * SUMS + k];
    }
#pragma unroll
    for (int k = 0; k < SUMS; ++k)
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) v[k] += __shfl_down(v[k], o, 64);
    if ((tid & 63) == 0) {
#pragma unroll
        for (int k = 0; k < SUMS; ++k) red[tid >> 6][k] = v[k];
    }
    __syncthreads();
    const unsigned long long* h = hist + n * 2 * CELLS;
    unsigned long long mine = 0ull;
    for (int c = tid; c < CELLS; c += 256) {
        const unsigned long long ca = h[c], cb = h[CELLS + c];
        mine += ca < cb ? ca : cb;
        if (hist_out != nullptr) {
            hist_out[n * 2 * CELLS + c] = (long long)ca;
            hist_out[n * 2 * CELLS + CELLS + c] = (long long)cb;
        }
    }
    if (mine != 0ull) atomicAdd(&common, mine);
    __syncthreads();
    if (tid < SUMS) out[n * (SUMS + 1) + tid] = ((red[0][tid] + red[1][tid]) + red[2][tid]) + red[3][tid];
    if (tid == SUMS) out[n * (SUMS + 1) + SUMS] = (double)common;
}

// What every entry checks and computes before its launch: 0, or the refusal code.
struct Plan {
    int64_t P, chunks, blocks;
    double* partial;
    unsigned long long* hist;
};

inline int plan(int N, int H, int W, const void* lin256, const void* out, const void* hist_out, void* ws, int64_t ws_bytes,
                Plan* pl) {
    if (N < 1 || H < 1 || W < 1 || H > (1 << 20) || W > (1 << 20)) return -1;
    pl->P = (int64_t)H * W;
    pl->chunks = (pl->P + CHUNK - 1) / CHUNK;
    pl->blocks = pl->chunks * N;
    if (pl->chunks > INT32_MAX || pl->blocks > INT32_MAX) return -1;
    if (lin256 == nullptr || out == nullptr) return -1;
    const int64_t need = (pl->blocks * SUMS + (int64_t)N * 2 * CELLS) * 8;
    if (ws == nullptr || ((uintptr_t)ws & 7) || ws_bytes < need) return -2;
    if (((uintptr_t)lin256 & 7) || ((uintptr_t)out & 7) || ((uintptr_t)hist_out & 7)) return -3;
    pl->partial = (double*)ws;
    pl->hist = (unsigned long long*)ws + pl->blocks * SUMS;
    return 0;
}

inline int clear_hist(const Plan& pl, int N, hipStream_t st) {
    const hipError_t e = hipMemsetAsync(pl.hist, 0, (size_t)N * 2 * CELLS * 8, st);
    return e == hipSuccess ? 0 : (int)e;
}

inline int finish(const Plan& pl, int N, double* out, int64_t* hist_out, hipStream_t st) {
    const int rc = CHECK_LAUNCH();
    if (rc != 0) return rc;
    hipLaunchKernelGGL(color_metrics_sum_kernel, dim3((unsigned)N), dim3(256), 0, st, (const double*)pl.partial, (int)pl.chunks,
                       (const unsigned long long*)pl.hist, out, (long long*)hist_out);
    return CHECK_LAUNCH();
}

}  // namespace

extern "C" int ssc_color_metrics_u8(const uint8_t* a, const uint8_t* b, const uint8_t* mask, int N, int H, int W,
                                    const double* lin256, double* out, int64_t* hist, void* ws, int64_t ws_bytes, void* stream) {
    Plan pl;
    if (a == nullptr || b == nullptr) return -1;
    int rc = plan(N, H, W, lin256, out, hist, ws, ws_bytes, &pl);
    if (rc != 0) return rc;
    if ((rc = clear_hist(pl, N, (hipStream_t)stream)) != 0) return rc;
    hipLaunchKernelGGL(color_metrics_u8_kernel, dim3((unsigned)pl.blocks), dim3(256), 0, (hipStream_t)stream, a, b, mask,
                       (long)pl.P, (int)pl.chunks, lin256, pl.partial, pl.hist);
    return finish(pl, N, out, hist, (hipStream_t)stream);
}

extern "C" int ssc_color_metrics_f32(const float* a, int lda, int coff_a, const float* b, int ldb, int coff_b, int b_planar,
                                     int N, int H, int W, const double* lin256, double* out, int64_t* hist, void* ws,
                                     int64_t ws_bytes, void* stream) {
    Plan pl;
    if (a == nullptr || b == nullptr) return -1;
    if (coff_a < 0 || lda < 3 || coff_a + 3 > lda) return -1;
    if (!b_planar && (coff_b < 0 || ldb < 3 || coff_b + 3 > ldb)) return -1;
    int rc = plan(N, H, W, lin256, out, hist, ws, ws_bytes, &pl);
    if (rc != 0) return rc;
    if (((uintptr_t)a & 3) || ((uintptr_t)b & 3)) return -3;
    if ((rc = clear_hist(pl, N, (hipStream_t)stream)) != 0) return rc;
    const F32Pixel load{a, lda, coff_a, b, b_planar ? 0 : ldb, b_planar ? 0 : coff_b, b_planar ? 1 : 0};
    hipLaunchKernelGGL(color_metrics_f32_kernel, dim3((unsigned)pl.blocks), dim3(256), 0, (hipStream_t)stream, load, (long)pl.P,
                       (int)pl.chunks, lin256, pl.partial, pl.hist);
    return finish(pl, N, out, hist, (hipStream_t)stream);
}

extern "C" int ssc_color_metrics_bg_f32(const float* img, int ldc, const uint8_t* fg, const uint8_t* target, const uint8_t* mask,
                                        int N, int H, int W, const double* lin256, double* out, int64_t* hist, void* ws,
                                        int64_t ws_bytes, void* stream) {
    Plan pl;
    if (img == nullptr || target == nullptr || ldc < 3) return -1;
    if (mask != nullptr && fg == nullptr) return -1;
    int rc = plan(N, H, W, lin256, out, hist, ws, ws_bytes, &pl);
    if (rc != 0) return rc;
    if ((uintptr_t)img & 3) return -3;
    if ((rc = clear_hist(pl, N, (hipStream_t)stream)) != 0) return rc;
    const BgPixel load{img, ldc, target};
    hipLaunchKernelGGL(color_metrics_bg_f32_kernel, dim3((unsigned)pl.blocks), dim3(256), 0, (hipStream_t)stream, load, mask,
                       (long)pl.P, (int)pl.chunks, lin256, pl.partial, pl.hist);
    return finish(pl, N, out, hist, (hipStream_t)stream);
}
