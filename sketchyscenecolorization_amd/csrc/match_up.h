// match_up.h -- one pixel of tf.image.resize_bilinear(pred, [S, S]) in the legacy form (align_corners = False), shared by
// ssc_match_finish (matching.hip) and ssc_match_score (match_val.hip) so that the two give the same bits for the same pixel.
// src = dst * (in / out); lower = floor(src), upper = min(lower + 1, in - 1), the fraction weighs them: first along x on the two
// rows, then along y.
#ifndef SSC_MATCH_UP_H
#define SSC_MATCH_UP_H
#include <hip/hip_runtime.h>

// the two source indices of destination index i along an axis of n source cells, and the weight of the upper one
__device__ __forceinline__ void match_up_axis(int i, float scale, int n, int& lo, int& hi, float& wt) {
    const float f = (float)i * scale;
    lo = min((int)floorf(f), n - 1);
    hi = lo + 1 < n ? lo + 1 : n - 1;
    wt = f - (float)lo;
}

// the up-sampled value at column x of a row whose source rows are ylo / yhi with the weight wy
__device__ __forceinline__ float match_up_value(const float* __restrict__ pred, int w, int ylo, int yhi, float wy, int x, float sx) {
    int xlo, xhi;
    float wx;
    match_up_axis(x, sx, w, xlo, xhi, wx);
    const float tl = pred[ylo * w + xlo], tr = pred[ylo * w + xhi], bl = pred[yhi * w + xlo], br = pred[yhi * w + xhi];
    const float top = tl + (tr - tl) * wx, bot = bl + (br - bl) * wx;
    return top + (bot - top) * wy;
}
#endif
