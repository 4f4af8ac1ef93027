// preview.hip -- the preview sheets of the held-out passes (preview.py): uint8 images reduced by an
// s x s box mean into tiles of one uint8 sheet [SH,SW,3].
//   ssc_sheet_tiles_u8     image n of src [N,H,W,3] -> the tile of H/s x W/s pixels at row top + n*pitch, column left
//   ssc_sheet_overlay_u8   a sketch [S,S,3], coloured per pixel by (predicted, target), -> one tile
// Every byte of a tile is (sum of its s*s source bytes + s*s/2) / (s*s) in integers: the same bits on every run, never outside
// 0..255.  Nothing outside the tiles is written.  Memory-bound, one pass over the source.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "sketchycolor_hip.h"

#define CHECK_LAUNCH() ((int)hipGetLastError())
#define MAX_SIDE 65536
#define GROUP 4             // output pixels per lane: 12 bytes (three 4-byte words) of a tile row

typedef unsigned char u8;

struct SheetArgs {
    const u8* src;          // [N,H,W,3]
    const u8* pred;         // [H,W] or null (overlay)
    const u8* labels;       // [H,W] or null (overlay)
    const u8* lut;          // [256], with labels
    u8* sheet;              // [SH,SW,3]
    int N, H, W, th, tw, gpr;       // gpr: lanes per tile row = ceil(tw / GROUP)
    int SW, top, left, pitch;
};

// the colour of a source pixel of the overlay: p predicted, t target; without one of the two arrays the other one paints green
__device__ __forceinline__ void overlay_colour(bool p, bool t, bool has_pred, bool has_labels, unsigned& r, unsigned& g, unsigned& b) {
    if ((p && t) || (p && !has_labels) || (t && !has_pred)) {
        r = 0, g = 170, b = 0;
    } else if (p) {
        r = 230, g = 0, b = 0;
    } else if (t) {
        r = 0, g = 90, b = 255;
    }
}

// A pixel is 3 bytes, so a tile row starts on any byte offset: a lane takes GROUP output pixels, whose 12 bytes (and the 12*SC
// source bytes of each of their SC source rows) start on a 4-byte boundary when the row does.  WIDE: every source row, every
// pred / labels row and every tile row starts on a 4-byte boundary (the entry point checks bases and row lengths) and a lane
// with a whole group moves 4-byte words; the last lane of a row whose width is no multiple of GROUP, and every lane without
// WIDE, moves single bytes.
template <int SC, bool WIDE, bool OVERLAY>
__global__ __launch_bounds__(256) void sheet_kernel(const SheetArgs a) {
    const long total = (long)a.N * a.th * a.gpr;
    const bool has_pred = OVERLAY && a.pred != nullptr, has_labels = OVERLAY && a.labels != nullptr;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const int g = (int)(i % a.gpr);
        const long r = i / a.gpr;
        const int ty = (int)(r % a.th), n = (int)(r / a.th);
        const int x0 = GROUP * g;
        const int npix = a.tw - x0 < GROUP ? a.tw - x0 : GROUP;
        const bool wide = WIDE && npix == GROUP;
        unsigned acc[3 * GROUP];
#pragma unroll
        for (int k = 0; k < 3 * GROUP; ++k) acc[k] = 0;
#pragma unroll
        for (int dy = 0; dy < SC; ++dy) {
            const long p0 = ((long)n * a.H + (long)ty * SC + dy) * a.W + (long)x0 * SC;     // the row's first source pixel
            if (wide) {
                unsigned w[3 * SC], pw[SC], lw[SC];
#pragma unroll
                for (int v = 0; v < 3 * SC; ++v) w[v] = reinterpret_cast<const unsigned*>(a.src + 3 * p0)[v];
                if (OVERLAY) {
#pragma unroll
                    for (int v = 0; v < SC; ++v) {
                        pw[v] = has_pred ? reinterpret_cast<const unsigned*>(a.pred + p0)[v] : 0u;
                        lw[v] = has_labels ? reinterpret_cast<const unsigned*>(a.labels + p0)[v] : 0u;
                    }
                }
#pragma unroll
                for (int k = 0; k < GROUP * SC; ++k) {
                    unsigned c[3];
#pragma unroll
                    for (int ch = 0; ch < 3; ++ch) {
                        const int byte = 3 * k + ch;
                        c[ch] = (w[byte >> 2] >> ((byte & 3) * 8)) & 255u;
                    }
                    if (OVERLAY) {
                        const bool p = ((pw[k >> 2] >> ((k & 3) * 8)) & 255u) != 0;
                        const bool t = has_labels && a.lut[(lw[k >> 2] >> ((k & 3) * 8)) & 255u] != 0;
                        overlay_colour(p, t, has_pred, has_labels, c[0], c[1], c[2]);
                    }
#pragma unroll
                    for (int ch = 0; ch < 3; ++ch) acc[3 * (k / SC) + ch] += c[ch];
                }
            } else {
                for (int k = 0; k < npix * SC; ++k) {
                    unsigned c[3];
#pragma unroll
                    for (int ch = 0; ch < 3; ++ch) c[ch] = a.src[3 * (p0 + k) + ch];
                    if (OVERLAY) {
                        const bool p = has_pred && a.pred[p0 + k] != 0;
                        const bool t = has_labels && a.lut[a.labels[p0 + k]] != 0;
                        overlay_colour(p, t, has_pred, has_labels, c[0], c[1], c[2]);
                    }
                    const int o = k / SC;
#pragma unroll
                    for (int j = 0; j < GROUP; ++j)         // a constant index keeps acc in registers
                        if (j == o) {
                            acc[3 * j] += c[0];
                            acc[3 * j + 1] += c[1];
                            acc[3 * j + 2] += c[2];
                        }
                }
            }
        }
        u8* dst = a.sheet + (((long)a.top + (long)n * a.pitch + ty) * a.SW + a.left + x0) * 3;
#pragma unroll
        for (int k = 0; k < 3 * GROUP; ++k) acc[k] = (acc[k] + SC * SC / 2) / (SC * SC);
        if (wide) {
#pragma unroll
            for (int v = 0; v < 3; ++v)
                reinterpret_cast<unsigned*>(dst)[v] = acc[4 * v] | (acc[4 * v + 1] << 8) | (acc[4 * v + 2] << 16) | (acc[4 * v + 3] << 24);
        } else {
#pragma unroll
            for (int j = 0; j < GROUP; ++j)
                if (j < npix) {
                    dst[3 * j] = (u8)acc[3 * j];
                    dst[3 * j + 1] = (u8)acc[3 * j + 1];
                    dst[3 * j + 2] = (u8)acc[3 * j + 2];
                }
        }
    }
}

static bool overlaps(const void* a, int64_t na, const void* b, int64_t nb) {
    const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
    return a != nullptr && b != nullptr && a0 < b0 + (uintptr_t)nb && b0 < a0 + (uintptr_t)na;
}

template <int SC, bool OVERLAY>
static int launch_scale(const SheetArgs& a, bool wide, hipStream_t stream) {
    const long total = (long)a.N * a.th * a.gpr;
    long blocks = (total + 255) / 256;
    if (blocks > 4096) blocks = 4096;
    const dim3 grid((unsigned)blocks), block(256);
    if (wide)
        hipLaunchKernelGGL((sheet_kernel<SC, true, OVERLAY>), grid, block, 0, stream, a);
    else
        hipLaunchKernelGGL((sheet_kernel<SC, false, OVERLAY>), grid, block, 0, stream, a);
    return CHECK_LAUNCH();
}

// the checks the two entry points share, then the launch; a.src .. a.sheet, N, H, W and the placement are filled in by the caller
template <bool OVERLAY>
static int sheet_launch(SheetArgs a, int s, int SH, void* stream) {
    if (a.src == nullptr || a.sheet == nullptr) return -1;
    if (a.N < 1 || a.N > 65535 || a.H < 1 || a.W < 1 || a.H > MAX_SIDE || a.W > MAX_SIDE) return -1;
    if (SH < 1 || a.SW < 1 || SH > MAX_SIDE || a.SW > MAX_SIDE) return -1;
    if (s != 1 && s != 2 && s != 4 && s != 6 && s != 8) return -1;
    if (a.H % s != 0 || a.W % s != 0) return -1;
    a.th = a.H / s, a.tw = a.W / s, a.gpr = (a.tw + GROUP - 1) / GROUP;
    if (a.top < 0 || a.left < 0 || a.pitch < 0) return -1;
    if (a.N > 1 && a.pitch < a.th) return -1;
    if ((int64_t)a.left + a.tw > a.SW || (int64_t)a.top + (int64_t)(a.N - 1) * a.pitch + a.th > SH) return -1;
    const int64_t pixels = (int64_t)a.N * a.H * a.W, sheet_bytes = (int64_t)SH * a.SW * 3;
    if (overlaps(a.src, pixels * 3, a.sheet, sheet_bytes) || overlaps(a.pred, pixels, a.sheet, sheet_bytes) ||
        overlaps(a.labels, pixels, a.sheet, sheet_bytes) || overlaps(a.lut, 256, a.sheet, sheet_bytes))
        return -1;
    // rows of 3*W source bytes, W pred / labels bytes and 3*SW sheet bytes keep a 4-byte boundary when W and SW are multiples of 4
    bool wide = a.W % 4 == 0 && a.SW % 4 == 0 && ((uintptr_t)a.src & 3) == 0 && (((uintptr_t)a.sheet + 3 * (uintptr_t)a.left) & 3) == 0;
    if (OVERLAY) wide = wide && (((uintptr_t)a.pred | (uintptr_t)a.labels) & 3) == 0;
    const hipStream_t st = (hipStream_t)stream;
    switch (s) {
    case 1: return launch_scale<1, OVERLAY>(a, wide, st);
    case 2: return launch_scale<2, OVERLAY>(a, wide, st);
    case 4: return launch_scale<4, OVERLAY>(a, wide, st);
    case 6: return launch_scale<6, OVERLAY>(a, wide, st);
    default: return launch_scale<8, OVERLAY>(a, wide, st);
    }
}

extern "C" int ssc_sheet_tiles_u8(const uint8_t* src, int N, int H, int W, int s, uint8_t* sheet, int SH, int SW, int top, int left,
                                  int pitch, void* stream) {
    SheetArgs a = {};
    a.src = src, a.sheet = sheet, a.N = N, a.H = H, a.W = W, a.SW = SW, a.top = top, a.left = left, a.pitch = pitch;
    return sheet_launch<false>(a, s, SH, stream);
}

extern "C" int ssc_sheet_overlay_u8(const uint8_t* sketch, const uint8_t* pred, const uint8_t* labels, const uint8_t* lut, int S, int s,
                                    uint8_t* sheet, int SH, int SW, int top, int left, void* stream) {
    if ((labels == nullptr) != (lut == nullptr)) return -1;
    SheetArgs a = {};
    a.src = sketch, a.pred = pred, a.labels = labels, a.lut = lut, a.sheet = sheet;
    a.N = 1, a.H = S, a.W = S, a.SW = SW, a.top = top, a.left = left, a.pitch = 0;
    return sheet_launch<true>(a, s, SH, stream);
}
