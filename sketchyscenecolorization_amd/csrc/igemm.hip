// igemm.hip -- implicit-GEMM convolution kernels for gfx950 (MI355X, CDNA4).
//
// fp32 in / fp32 accumulate on the matrix cores (v_mfma_f32_32x32x2_f32: exact
// f32, 157 TFLOP/s peak), 64-wide wavefronts, 4 waves per workgroup, LDS-staged
// tiles with register prefetch of the next K-tile (one barrier per K-tile).
//
// Two kernels share the tile loaders:
//   conv_fwd_kernel  : out[pix][n]      = sum_{tap,k} X[pix@tap][k] * F(tap,k,n)
//   conv_wgrad_kernel: dF[(tap,cg)][cd] = sum_pix     G[pix@tap][cg] * D[pix][cd]
// X/G/D are "gather views" (ssc_gview): NHWC tensors (optionally the channel
// concat of two) with the folded batch-stat norm a*x+b and the activation
// applied while the tile is loaded, zero outside the image.  This is how the
// reference's  lrelu -> conv -> batchnorm  /  relu(concat) -> deconv -> batchnorm
// blocks (models_collection.py:434-439, 510-526) are fused: the norm+activation
// of layer L is evaluated inside the loads of layer L+1, so normalised tensors
// are never written to HBM.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include "sketchycolor_hip.h"
#include "igemm_util.h"
#include "igemm_epilogue.h"
#include "host_util.h"

// wgrad128.hip
extern "C" int ssc_conv_wgrad128_supported(const ssc_wgrad_desc* dp);
extern "C" int ssc_conv_wgrad128(const ssc_wgrad_desc* dp, float* ws, int64_t ws_bytes, void* stream);
int ssc_conv_wgrad128_bf_selected(const ssc_wgrad_desc* dp);
// wgn16.hip
extern "C" int ssc_conv_wgn16_supported(const ssc_wgrad_desc* dp);
int ssc_conv_wgn16(const ssc_wgrad_desc* dp, float* ws, int64_t ws_bytes, void* stream);
int ssc_conv_wgn16_fits(const ssc_wgrad_desc* dp, int64_t ws_bytes);
// narrow.hip
int ssc_conv_narrow_forward_ws(const ssc_conv_desc* dp, float* ws, int64_t ws_bytes, void* stream, int* csplit_out);
// fewchan.hip
int ssc_conv_fewchan_forward(const ssc_conv_desc* dp, int num_cu, void* stream);
// pw1x1.hip
extern "C" int ssc_conv_pw1x1_supported(const ssc_conv_desc* dp);
int ssc_conv_pw1x1_walkers(const ssc_conv_desc* dp);
int ssc_conv_pw1x1_forward(const ssc_conv_desc* dp, float* stat, void* stream);
// tr4n16.hip
extern "C" int ssc_conv_tr4n16_supported(const ssc_conv_desc* dp);
int ssc_conv_tr4n16_rows(const ssc_conv_desc* dp);
int ssc_conv_tr4n16_forward(const ssc_conv_desc* dp, float* stat, void* stream);
// fewchan7.hip
extern "C" int ssc_conv_fewchan7_supported(const ssc_conv_desc* dp);
int ssc_conv_fewchan7_walkers(const ssc_conv_desc* dp);
int ssc_conv_fewchan7_forward(const ssc_conv_desc* dp, float* stat, void* stream);
// tr4tiny.hip
extern "C" int ssc_conv_tr4_tiny_supported(const ssc_conv_desc* dp);
int ssc_conv_tr4_tiny_blocks(const ssc_conv_desc* dp);
int ssc_conv_tr4_tiny_forward(const ssc_conv_desc* dp, float* stat, void* stream);
// s2n16.hip
extern "C" int ssc_conv_s2n16_supported(const ssc_conv_desc* dp);
int ssc_conv_s2n16_walkers(const ssc_conv_desc* dp);
int ssc_conv_s2n16_forward(const ssc_conv_desc* dp, float* stat, void* stream);
// c3x3.hip
extern "C" int ssc_conv_c3x3_supported(const ssc_conv_desc* dp);
int ssc_conv_c3x3_walkers(const ssc_conv_desc* dp);
int ssc_conv_c3x3_forward(const ssc_conv_desc* dp, float* stat, void* stream);
// what each of those launchers decides (host_util.h): the launches read it and so does ssc_conv_stream_plan
ssc_stream_plan ssc_conv_fewchan_plan(const ssc_conv_desc* dp, int num_cu);
ssc_stream_plan ssc_conv_pw1x1_plan(const ssc_conv_desc* dp);
ssc_stream_plan ssc_conv_c3x3_plan(const ssc_conv_desc* dp);
ssc_stream_plan ssc_conv_s2n16_plan(const ssc_conv_desc* dp);
ssc_stream_plan ssc_conv_tr4_tiny_plan(const ssc_conv_desc* dp);
ssc_stream_plan ssc_conv_fewchan7_plan(const ssc_conv_desc* dp);
ssc_stream_plan ssc_conv_tr4n16_plan(const ssc_conv_desc* dp);

// igemm_bf16.hip
bool ssc_bf_hk_enabled();       // igemm_bf16.hip
int ssc_launch_conv_bf(int cfg, bool plain, const ssc_conv_desc& d, int splitk, float* ws, hipStream_t st, long ts_full, int ts_s,
                       int64_t ws_bytes, int xcd);
int ssc_conv_bf_form(int cfg, bool plain, const ssc_conv_desc& d, int splitk, bool have_ws, long ts_full, int ts_s, int64_t ws_bytes,
                     int xcd, int* out10);
int ssc_sk_configure_bf(const unsigned* cfg4);

#define BK 32
// in-launch K-slice hand-off (conv_ut_kernel): {wait bound in ticks of the 100 MHz wall clock (lo, hi), test hook: producers
// withhold their flags, -}.  ssc_sk_configure writes it.
__device__ unsigned g_sk_cfg[4] = {2000000000u, 0u, 0u, 0u};

// ---------------------------------------------------------------------------------------------
// forward form
// ---------------------------------------------------------------------------------------------
// General form: any channel counts (K-tiles may straddle taps and sources: per-thread tap decode), scalar or float4
// filter loads.  Phases per wave: issue the next K-tile's loads | MFMAs of the current one | transform + LDS write |
// barrier.  The layers whose K-tiles lie inside one tap and one source take conv_ut_kernel below instead.
template <int WM, int WN, int SM, int SN, int BMODE, bool VECB>
__global__ __launch_bounds__(256) void conv_fwd_kernel(const ssc_conv_desc d, const Magics mg,
                                                        float* __restrict__ slab_base, long slab_stride,
                                                        int splitk) {
    constexpr int BM = WM * SM * 32;
    constexpr int BN = WN * SN * 32;
    constexpr int A_LD = BK + 1;
    constexpr int A_SZ = BM * A_LD;
    constexpr int B_LD = (BMODE == 0) ? BN : (BK + 1);
    constexpr int B_SZ = (BMODE == 0) ? BK * BN : BN * (BK + 1);
    constexpr int A_ROWS = BM / 32;   // rows of the A tile per thread
    constexpr int B_SLOTS = BN / 32;  // float4 slots of the B tile per thread
    constexpr int B_RP = 1024 / BN;   // filter rows per pass (KN)
    static_assert(WM * WN == 4, "4 waves per workgroup");

    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* As = smem;                 // [2][A_SZ]
    float* Bs = smem + 2 * A_SZ;      // [2][B_SZ]
    long* rowpix = reinterpret_cast<long*>(smem + 2 * A_SZ + 2 * B_SZ);   // [BM] output pixel of each tile row

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int wm = wave / WN, wn = wave % WN;

    const int C = d.x.C0 + d.x.C1;
    const int Ktot = d.TH * d.TW * C;
    const long M = (long)d.NB * d.PH * d.PW;
    const int PHW = d.PH * d.PW;
    const int phase = blockIdx.z / splitk;
    const int ks = blockIdx.z % splitk;
    const FwdPhase ph = fwd_phase(d, phase);

    const long m0 = (long)blockIdx.x * BM;
    const int n0 = blockIdx.y * BN;

    // ---- per-thread A rows: pixel decode (fixed for the whole kernel) ----
    const int a_col4 = tid & 7;            // float4 column inside the K tile
    int a_iyb[A_ROWS], a_ixb[A_ROWS];
    long a_nb[A_ROWS];
    bool a_mv[A_ROWS];
#pragma unroll
    for (int i = 0; i < A_ROWS; ++i) {
        const int row = (tid >> 3) + 32 * i;
        const long m = m0 + row;
        a_mv[i] = m < M;
        const long mm = a_mv[i] ? m : 0;
        const int n = (int)div64(mm, mg.mPHPW, mg.onePHPW);
        const int rem = (int)(mm - (long)n * PHW);
        const int py = (int)div64(rem, mg.mPW, mg.onePW), px = rem - py * d.PW;
        a_iyb[i] = py * d.in_stride + ph.ioff_y;
        a_ixb[i] = px * d.in_stride + ph.ioff_x;
        a_nb[i] = (long)n * d.x.H * d.x.W;
        if (a_col4 == 0)
            rowpix[row] = ((long)n * d.OH + py * d.out_stride + ph.ooff_y) * d.OW + px * d.out_stride + ph.ooff_x;
    }

    const int nkt = (Ktot + BK - 1) / BK;
    const int per = (nkt + splitk - 1) / splitk;
    const int kt_begin = ks * per;
    const int kt_end = min(nkt, kt_begin + per);

    f32x16 acc[SM][SN];
#pragma unroll
    for (int i = 0; i < SM; ++i)
#pragma unroll
        for (int j = 0; j < SN; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    // staging registers
    float4 ra[A_ROWS];
    float rav[A_ROWS];    // 1.0 / 0.0 validity of each staged A row
    float4 raa, rab;
    float ra_slope = 1.f;    // activation slope of the source this K-tile reads
    float4 rb[B_SLOTS];
    float4 rbm[B_SLOTS];  // per-element 1.0 / 0.0 validity of the staged filter values
    const float x_slope0 = act_slope(d.x.act), x_slope1 = act_slope(d.x.act1 >= 0 ? d.x.act1 : d.x.act);

    auto load_tile = [&](int kt) {
        // A (gather view): every load unconditional from a clamped address
        {
            const int kcol = kt * BK + a_col4 * 4;
            const bool kv = kcol < Ktot;
            const int kk = kv ? kcol : 0;
            const int tap = div32(kk, mg.mC, mg.oneC);
            const int c = kk - tap * C;
            const int ty = div32(tap, mg.mTW, mg.oneTW), tx = tap - ty * d.TW;
            gview_affine4(d.x, c, raa, rab);
            ra_slope = c < d.x.C0 ? x_slope0 : x_slope1;
            const float* base;
            int cs;
            gview_src(d.x, c, base, cs);
#pragma unroll
            for (int i = 0; i < A_ROWS; ++i) {
                const int iy = a_iyb[i] + ty, ix = a_ixb[i] + tx;
                const bool v = kv && a_mv[i] && iy >= 0 && iy < d.x.H && ix >= 0 && ix < d.x.W;
                const long pix = v ? a_nb[i] + (long)iy * d.x.W + ix : 0;
                rav[i] = v ? 1.f : 0.f;
                ra[i] = *reinterpret_cast<const float4*>(base + pix * cs);
            }
        }
        if (BMODE == 0) {           // KN: tile [BK rows k][BN cols n], n contiguous in memory
            const int n = n0 + (tid % (BN / 4)) * 4;
#pragma unroll
            for (int s = 0; s < B_SLOTS; ++s) {
                const int krow = kt * BK + tid / (BN / 4) + B_RP * s;
                const bool kv = krow < Ktot;
                const int kk = kv ? krow : 0;
                const int tp = div32(kk, mg.mC, mg.oneC);
                const int kc = kk - tp * C;
                const int tty = div32(tp, mg.mTW, mg.oneTW), ttx = tp - tty * d.TW;
                const int ky = ph.ky0 + tty * d.kstep, kx = ph.kx0 + ttx * d.kstep;
                const bool rowv = kv && kc < d.k_real;
                const float* wp = d.w + ((long)(ky * d.KW + kx) * d.wC0 + (rowv ? kc : 0)) * d.wC1 + d.n_off;
                if (VECB) {
                    const bool cv = n < d.Nn;       // Nn % 4 == 0: the whole float4 is in or out
                    rb[s] = *reinterpret_cast<const float4*>(wp + (cv ? n : 0));
                    const float m = (rowv && cv) ? 1.f : 0.f;
                    rbm[s] = make_float4(m, m, m, m);
                } else {
                    const bool v0 = rowv && n + 0 < d.Nn, v1 = rowv && n + 1 < d.Nn;
                    const bool v2 = rowv && n + 2 < d.Nn, v3 = rowv && n + 3 < d.Nn;
                    rb[s].x = wp[v0 ? n + 0 : 0];
                    rb[s].y = wp[v1 ? n + 1 : 0];
                    rb[s].z = wp[v2 ? n + 2 : 0];
                    rb[s].w = wp[v3 ? n + 3 : 0];
                    rbm[s] = make_float4(v0 ? 1.f : 0.f, v1 ? 1.f : 0.f, v2 ? 1.f : 0.f, v3 ? 1.f : 0.f);
                }
            }
        } else {                    // NK: tile [BN rows n][BK cols k], k contiguous in memory
            const int kc4 = kt * BK + (tid & 7) * 4;
            const bool kvb = kc4 < Ktot;
            const int kk = kvb ? kc4 : 0;
            const int tp = div32(kk, mg.mC, mg.oneC);
            const int kc = kk - tp * C;
            const int tty = div32(tp, mg.mTW, mg.oneTW), ttx = tp - tty * d.TW;
            const int ky = ph.ky0 + tty * d.kstep, kx = ph.kx0 + ttx * d.kstep;
            const long tapoff = (long)(ky * d.KW + kx) * d.wC0 + d.n_off;
#pragma unroll
            for (int s = 0; s < B_SLOTS; ++s) {
                const int n = n0 + (tid >> 3) + 32 * s;
                const bool nv = kvb && n < d.Nn;
                const float* wp = d.w + (tapoff + (nv ? n : 0)) * d.wC1;
                if (VECB) {
                    const bool cv = kc < d.k_real;  // k_real % 4 == 0
                    rb[s] = *reinterpret_cast<const float4*>(wp + (cv ? kc : 0));
                    const float m = (nv && cv) ? 1.f : 0.f;
                    rbm[s] = make_float4(m, m, m, m);
                } else {
                    const bool v0 = nv && kc + 0 < d.k_real, v1 = nv && kc + 1 < d.k_real;
                    const bool v2 = nv && kc + 2 < d.k_real, v3 = nv && kc + 3 < d.k_real;
                    rb[s].x = wp[v0 ? kc + 0 : 0];
                    rb[s].y = wp[v1 ? kc + 1 : 0];
                    rb[s].z = wp[v2 ? kc + 2 : 0];
                    rb[s].w = wp[v3 ? kc + 3 : 0];
                    rbm[s] = make_float4(v0 ? 1.f : 0.f, v1 ? 1.f : 0.f, v2 ? 1.f : 0.f, v3 ? 1.f : 0.f);
                }
            }
        }
    };

    auto store_tile = [&](int buf) {
        float* Ab = As + buf * A_SZ;
        float* Bb = Bs + buf * B_SZ;
#pragma unroll
        for (int i = 0; i < A_ROWS; ++i) {
            const float4 v = xform4(ra[i], raa, rab, ra_slope, rav[i]);
            float* p = Ab + ((tid >> 3) + 32 * i) * A_LD + a_col4 * 4;
            p[0] = v.x; p[1] = v.y; p[2] = v.z; p[3] = v.w;
        }
#pragma unroll
        for (int s = 0; s < B_SLOTS; ++s) {
            float4 v = rb[s];
            v.x *= rbm[s].x; v.y *= rbm[s].y; v.z *= rbm[s].z; v.w *= rbm[s].w;
            if (BMODE == 0) {
                *reinterpret_cast<float4*>(Bb + (tid / (BN / 4) + B_RP * s) * B_LD + (tid % (BN / 4)) * 4) = v;
            } else {
                float* p = Bb + ((tid >> 3) + 32 * s) * B_LD + (tid & 7) * 4;
                p[0] = v.x; p[1] = v.y; p[2] = v.z; p[3] = v.w;
            }
        }
    };

    if (kt_begin < kt_end) {
        load_tile(kt_begin);
        store_tile(0);
    }
    __syncthreads();

    // main loop: the global loads of K-tile kt+1 are issued before the 64 MFMAs of K-tile kt and written to
    // the other LDS buffer after them (one barrier per K-tile)
    const int l31 = lane & 31, lhi = lane >> 5;
    int cur = 0;
    for (int kt = kt_begin; kt < kt_end; ++kt) {
        const bool more = (kt + 1) < kt_end;
        if (more) load_tile(kt + 1);
        const float* Ab = As + cur * A_SZ + (wm * SM * 32 + l31) * A_LD + lhi;
        const float* Bb = (BMODE == 0) ? (Bs + cur * B_SZ + lhi * B_LD + wn * SN * 32 + l31)
                                       : (Bs + cur * B_SZ + (wn * SN * 32 + l31) * B_LD + lhi);
        // LDS -> register operand fetch, software-pipelined by groups of FG k-steps: the ds_reads of group g+1 are
        // issued before the MFMAs of group g (the compiler otherwise places every read directly in front of its
        // MFMA pair behind an s_waitcnt lgkmcnt(0), exposing the LDS latency 16 times per K-tile)
        constexpr int FG = 4, NFG = BK / 2 / FG;
        float av[2][FG][SM], bv[2][FG][SN];
        auto fetch = [&](int g, int buf) {
#pragma unroll
            for (int q = 0; q < FG; ++q) {
                const int kk = g * FG + q;
#pragma unroll
                for (int i = 0; i < SM; ++i) av[buf][q][i] = Ab[i * 32 * A_LD + kk * 2];
#pragma unroll
                for (int j = 0; j < SN; ++j)
                    bv[buf][q][j] = (BMODE == 0) ? Bb[kk * 2 * B_LD + j * 32] : Bb[j * 32 * B_LD + kk * 2];
            }
        };
        fetch(0, 0);
#pragma unroll
        for (int g = 0; g < NFG; ++g) {
            if (g + 1 < NFG) fetch(g + 1, (g + 1) & 1);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int q = 0; q < FG; ++q)
#pragma unroll
                for (int i = 0; i < SM; ++i)
#pragma unroll
                    for (int j = 0; j < SN; ++j)
                        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[g & 1][q][i], bv[g & 1][q][j], acc[i][j], 0, 0, 0);
            __builtin_amdgcn_sched_barrier(0);
        }
        if (more) store_tile(cur ^ 1);
        __syncthreads();
        cur ^= 1;
    }

    // ---- epilogue ----
    float* outp = (splitk > 1) ? (slab_base + (long)ks * slab_stride) : d.out;
    const bool final_pass = (splitk == 1);
#pragma unroll
    for (int i = 0; i < SM; ++i) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = wm * SM * 32 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * lhi;
            if (m0 + row >= M) continue;
            const long opix = rowpix[row];
#pragma unroll
            for (int j = 0; j < SN; ++j) {
                const int col = n0 + wn * SN * 32 + j * 32 + l31;
                if (col >= d.Nstore) continue;
                float v = acc[i][j][r];
                float* o = outp + opix * d.ldc + col;
                if (final_pass) {
                    if (d.bias != nullptr && col < d.Nn) v += d.bias[col];
                    if (d.epi == 1) v = tanhf(v);
                    else if (d.epi == 2) v = fmaxf(v, 0.2f * v);
                    if (d.accumulate) v += *o;
                }
                *o = v;
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------
// uniform-tap form with the staging of later K-tiles interleaved into the MFMA stream of the same wave
// ---------------------------------------------------------------------------------------------
// conv_fwd_kernel alternates phases per wave (issue loads | 32-64 MFMAs | transform + LDS writes | barrier) and relies on
// the 2-3 co-resident waves of a SIMD being in different phases to keep the matrix pipe fed; measured, the pipe sits at
// 60-70 %.  Here one K-tile step is a single branch-free block: the registers that hold K-tile kt+1 (loaded one step
// ago) go to the free LDS buffer and are refilled with the global loads of K-tile kt+2 while the MFMAs of K-tile kt
// issue, so address arithmetic, memory issue and LDS traffic sit in the 64-cycle shadow of each MFMA.
//   * no per-step branches: the K-tile index is clamped instead of tested, selects are arithmetic, the filter columns
//     beyond Nn are zeroed in the epilogue instead of masked every step;
//   * PLAIN (no folded norm, no activation on any source: every data-gradient launch) is a template flag.
#define UT_AV(BM, BN) (!((BM) == 128 && (BN) <= 64))
// KMASK: channel counts that are not multiples of 32 (the MRU concats: 576 + 4, of which 579 real).  K-tiles are then
// enumerated per (tap, source, 32-channel chunk), mg.mC holding the magic of chunks-per-tap, so a tile still lies inside
// one tap and one source; the last chunk of a source is partly empty: its A float4s beyond the source's channels are
// not loaded and its filter rows beyond the real channels are zeroed (the A padding channels need not hold zeros).
// KM = 2 ("row tap"): few channels, TW * C == 32 (the discriminator's first conv: 4 taps x 8 channels).  A filter ROW is
// then one K-tile: its TW taps x C channels are 32 contiguous floats both in the NHWC input (consecutive pixels) and in
// the filter, so the launch runs as TH taps of "32 channels" (the host sets TW = 1); only the x bound differs per thread.
template <int WM, int WN, int SM, int SN, int BMODE, bool PLAIN, int KM>
__global__ __launch_bounds__(256) void conv_ut_kernel(const ssc_conv_desc d, const Magics mg,
                                                       float* __restrict__ slab_base, long slab_stride, int splitk,
                                                       int ts_full, int ts_s, unsigned* __restrict__ flags) {
    constexpr int BM = WM * SM * 32;
    constexpr int BN = WN * SN * 32;
    // AV: A rows padded to 36 floats (16-byte aligned, b128 accesses conflict-free) and the K index of MFMA step kk on
    // lane half lhi permuted to k = 16*lhi + kk (any bijection works when A and B agree): a lane's 16 A operands of a
    // K-tile are then contiguous, 4 ds_read_b128 instead of 16 ds_read_b32 per row block, and each staged float4 is one
    // ds_write_b128.  Not for the 128-row x <=64-column tiles, whose 3 workgroups per CU would no longer fit the LDS.
    constexpr bool KMASK = (KM == 1), ROWTAP = (KM == 2);
    // BDMA: the filter tile goes global memory -> LDS directly (global_load_lds_dwordx4: 1 KiB per wave instruction, lane L
    // lands at +16 L), no staging registers, no ds_write, no vector ALU work per K-tile.  A wave instruction covers
    // 256 / BN consecutive k rows of the [k][n] image (KN) or 8 rows of the swizzled [n][32] image (NK: each lane fetches the
    // 16-byte chunk whose swizzled position is its own slot).  Not with KMASK, whose partial chunks need zeroed rows.
    // (The gathered tile by LDS-DMA too, for the launches without norm / activation, measured equal to the register path --
    // 1714-1720 images/s either way -- and is not kept.)
    constexpr bool BDMA = !KMASK;
    constexpr int B_IPW = BK * BN / 1024;          // DMA instructions per wave and K-tile
    constexpr bool AV = UT_AV(BM, BN);
    constexpr int A_LD = AV ? BK + 4 : BK + 1;
    constexpr int A_SZ = BM * A_LD;
    // NK filters (k contiguous in memory): the B tile is [n][32] with the 16-byte chunk c of row n stored at chunk
    // c ^ ((n >> 1) & 7) -- b128 writes and b128 operand reads, both conflict-free, no padding (the scalar [n][33] image it
    // replaces cost 34 address adds per K-tile and wave)
    constexpr int B_LD = (BMODE == 0) ? BN : BK;
    constexpr int B_SZ = (BMODE == 0) ? BK * BN : BN * BK;
    constexpr int A_ROWS = BM / 32;
    constexpr int B_SLOTS = BN / 32;
    constexpr int B_RP = 1024 / BN;
    static_assert(WM * WN == 4, "4 waves per workgroup");

    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* As = smem;
    float* Bs = smem + 2 * A_SZ;
    long* rowpix = reinterpret_cast<long*>(smem + 2 * A_SZ + 2 * B_SZ);

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int wm = wave / WN, wn = wave % WN;
    const int l31 = lane & 31, lhi = lane >> 5;

    // descriptor fields the K loop needs, in registers (the loop must not go back to the kernarg segment)
    const float* const xs0 = d.x.s0;
    const float* const xs1 = d.x.s1;
    const float* const xab0 = d.x.ab0;
    const float* const xab1 = d.x.ab1;
    const float* const wbase = d.w;
    const int xC0 = d.x.C0, xC1 = d.x.C1, xH = d.x.H, xW = d.x.W;
    const int TWv = d.TW, kstep = d.kstep, KWv = d.KW, wC0 = d.wC0, wC1 = d.wC1;
    const float slope0 = act_slope(d.x.act), slope1 = act_slope(d.x.act1 >= 0 ? d.x.act1 : d.x.act);

    const int C = xC0 + xC1;
    const int nch0 = ROWTAP ? 1 : (xC0 + BK - 1) / BK, nch1 = ROWTAP ? 0 : (xC1 + BK - 1) / BK;   // 32-channel chunks per source
    const int tpt = nch0 + nch1;                                          // K-tiles per tap
    const int kreal0 = min(xC0, d.k_real), kreal1 = d.k_real - xC0;        // real filter channels of each source
    const long M = (long)d.NB * d.PH * d.PW;
    const int PHW = d.PH * d.PW;
    // workgroup -> (tile, K range).  Legacy grid: x = row tile, y = column tile, z = phase * splitk + K slice.
    // Tail split (ts_s > 0, 1-D grid, launches without split-K): tiles [0, ts_full) fill whole rounds of the chip and are
    // finished in place; each of the remaining tiles -- the partly filled last round -- is cut into ts_s K slices that
    // together fill that round.  The slices of a tile are combined INSIDE the launch: slices 0 .. ts_s-2 write raw partial
    // tiles (accumulator order, write-through stores) and raise a flag each; the last slice -- the highest workgroup id of
    // the tile, so everything it waits for was dispatched before it -- adds them to its accumulators in slice order (a
    // fixed summation order) and runs the epilogue.  Agent-scope release / acquire as the CDNA4 guide prescribes: sc1
    // stores, every storing wave drains, one lane stores the flag relaxed; the owner polls relaxed, one acquire fence,
    // then plain loads.  The owner leaves the flags zero; its waits are bounded (flag word SSC_SK_FLAG_WORDS-1 = timeout).
    int phase, ks, sk, n0, slot = 0;
    long m0;
    float* part = nullptr;
    if (ts_s > 0) {
        const int bid = blockIdx.x;
        int tile;
        if (bid < ts_full) {
            tile = bid; ks = 0; sk = 1;
        } else {
            const int r = bid - ts_full;
            const int q = r / (ts_s & 0xffff);
            tile = ts_full + q; ks = r - q * (ts_s & 0xffff); sk = ts_s & 0xffff;
            part = slab_base + (long)r * (BM * BN);
            slot = r;
        }
        const int mt = (int)((M + BM - 1) / BM), nt = (d.Nstore + BN - 1) / BN;
        if (ts_s & 0x10000) {
            // XCD-aware order (ts_s high half set by the host): tiles are numbered column tile fastest, then row tile, then
            // phase, and the whole tiles are dealt so that workgroup ids with the same id % 8 -- the same XCD, the same L2
            // -- walk a contiguous run of that order: the column tiles of a row tile (same gathered rows) and spatially
            // neighbouring row tiles (overlapping taps) meet in one L2 instead of eight
            if (bid < ts_full) tile = (bid & 7) * (ts_full >> 3) + (bid >> 3);
            const int r2 = tile / nt;
            n0 = (tile - r2 * nt) * BN;
            if (ts_s & 0x20000) {       // 4 sub-pixel phases of a row tile next to each other: they gather the same 3x3 input
                phase = r2 & 3;         // neighbourhoods (16 (phase, tap) pairs, 9 distinct pixels), so they share them in one L2
                m0 = (long)(r2 >> 2) * BM;
            } else {
                phase = r2 / mt;
                m0 = (long)(r2 - phase * mt) * BM;
            }
            ts_s &= 0xffff;
            sk = bid < ts_full ? 1 : ts_s;
        } else {
            const int rest = tile / mt;
            m0 = (long)(tile - rest * mt) * BM;
            phase = rest / nt;
            n0 = (rest - phase * nt) * BN;
        }
    } else {
        phase = blockIdx.z / splitk;
        ks = blockIdx.z % splitk;
        sk = splitk;
        m0 = (long)blockIdx.x * BM;
        n0 = blockIdx.y * BN;
    }
    const FwdPhase ph = fwd_phase(d, phase);

    const int a_kx = ROWTAP ? ((tid & 7) * 4) / xC0 : 0;    // row tap: this thread's float4 belongs to pixel ix + a_kx
    int a_iyb[A_ROWS], a_ixb[A_ROWS], a_off0[A_ROWS], a_off1[A_ROWS];
    bool a_mv[A_ROWS];
#pragma unroll
    for (int i = 0; i < A_ROWS; ++i) {
        const int row = (tid >> 3) + 32 * i, col4 = tid & 7;        // tile row (32 rows per pass) and 16-byte chunk of this thread's i-th float4
        const long m = m0 + row;
        a_mv[i] = m < M;
        const long mm = a_mv[i] ? m : 0;
        int n, rem, py;
        if (mg.use32) {     // wave-uniform: every numerator x divisor fits 32 bits
            n = (int)__umulhi((unsigned)mm, mg.mPHPW32) + (int)((unsigned)mm & (unsigned)mg.onePHPW);
            rem = (int)mm - n * PHW;
            py = (int)__umulhi((unsigned)rem, mg.mPW32) + (int)((unsigned)rem & (unsigned)mg.onePW);
        } else {
            n = (int)div64(mm, mg.mPHPW, mg.onePHPW);
            rem = (int)(mm - (long)n * PHW);
            py = (int)div64(rem, mg.mPW, mg.onePW);
        }
        const int px = rem - py * d.PW;
        a_iyb[i] = py * d.in_stride + ph.ioff_y;
        a_ixb[i] = px * d.in_stride + ph.ioff_x;
        const int pix0 = (n * xH + a_iyb[i]) * xW + a_ixb[i];
        a_off0[i] = (pix0 * xC0 + col4 * 4) * 4;        // BYTE offsets from a wave-uniform base: the loads then take the
        a_off1[i] = (pix0 * xC1 + col4 * 4) * 4;        // scalar-base + 32-bit vector-offset form, no 64-bit address arithmetic
        if ((tid & 7) == 0)
            rowpix[row] = ((long)n * d.OH + py * d.out_stride + ph.ooff_y) * d.OW + px * d.out_stride + ph.ooff_x;
    }
    const int a_col4 = tid & 7;     // chunk of this thread's float4s
    // filter offsets of this thread's float4 slots, split into the part along K (b_k: filter rows of the tile for KN,
    // element offset along the row for NK) and the rest (b_n), so that KMASK can drop the K part of an empty slot
    int b_k[B_SLOTS], b_n[B_SLOTS], b_kk[B_SLOTS];     // b_kk: k index inside the tile
#pragma unroll
    for (int s = 0; s < B_SLOTS; ++s) {
        if (BMODE == 0) {
            const int n = n0 + (tid % (BN / 4)) * 4;
            const bool nv = n < d.Nn;
            b_kk[s] = tid / (BN / 4) + B_RP * s;
            b_k[s] = nv ? b_kk[s] * wC1 * 4 : 0;            // bytes
            b_n[s] = nv ? (d.n_off + n) * 4 : 0;
        } else {
            const int n = n0 + (tid >> 3) + 32 * s;
            const bool nv = n < d.Nn;
            b_kk[s] = (tid & 7) * 4;
            b_k[s] = nv ? b_kk[s] * 4 : 0;
            b_n[s] = nv ? (d.n_off + n) * wC1 * 4 : 0;
        }
    }

    unsigned bd_off[B_IPW];     // BDMA: this lane's byte offset inside the filter for each of its wave's instructions
    if (BDMA) {
#pragma unroll
        for (int q = 0; q < B_IPW; ++q) {
            const int ins = wave * B_IPW + q;
            if (BMODE == 0) {
                constexpr int RPI = 256 / BN;           // k rows per instruction
                const int r = ins * RPI + lane / (BN / 4), n = n0 + (lane % (BN / 4)) * 4;
                bd_off[q] = n < d.Nn ? (unsigned)((r * wC1 + d.n_off + n) * 4) : (unsigned)(r * wC1 * 4);
            } else {
                const int r = ins * 8 + (lane >> 3), n = n0 + r;
                const int c = (lane & 7) ^ ((r >> 1) & 7);      // the chunk whose swizzled slot is lane & 7
                bd_off[q] = n < d.Nn ? (unsigned)(((d.n_off + n) * wC1 + c * 4) * 4) : (unsigned)(c * 16);
            }
        }
    }

    const int nkt = d.TH * d.TW * tpt;
    const int per = (nkt + sk - 1) / sk;
    const int kt_begin = ks * per;
    const int kt_end = min(nkt, kt_begin + per);

    f32x16 acc[SM][SN];
#pragma unroll
    for (int i = 0; i < SM; ++i)
#pragma unroll
        for (int j = 0; j < SN; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    float4 ra[A_ROWS];
    float rav[A_ROWS];
    float4 raa, rab;
    float ra_slope = 1.f;
    float4 rb[B_SLOTS];
    float rbv[B_SLOTS];      // KMASK: 1.0 / 0.0 validity of each staged filter float4

    auto issue_loads = [&](int kt) {
        const int tap = div32(kt, mg.mC, mg.oneC);      // mC: magic of tpt
        const int chunk = kt - tap * tpt;
        const int ty = div32(tap, mg.mTW, mg.oneTW), tx = tap - ty * TWv;
        const bool first = chunk < nch0;
        const int cs = first ? xC0 : xC1;
        const int cc = (first ? chunk : chunk - nch0) * BK;     // channel offset inside the source
        const int cch = first ? cc : xC0 + cc;                  // channel offset inside the filter's K rows
        const int kreal = (first ? kreal0 : kreal1) - cc;       // real channels left in this source from cc on
        const int cchf = (!KMASK || kreal > 0) ? cch : 0;       // a chunk without real channels reads (and drops) row 0
        const char* sbase = reinterpret_cast<const char*>((first ? xs0 : xs1) + cc);
        const int tapshift = (ty * xW + tx) * cs * 4;
        const int fmask = first ? -1 : 0;
        if (!PLAIN) {
            const float* abp = first ? xab0 : xab1;
            const bool has = abp != nullptr;
            const bool hc = has & (!KMASK || cc + a_col4 * 4 < cs);     // KMASK: no table entries beyond the source
            const float* pa = hc ? abp + cc + a_col4 * 4 : xs0;       // a valid address either way
            const float* pb = hc ? abp + cs + cc + a_col4 * 4 : xs0;
            const float4 va = *reinterpret_cast<const float4*>(pa);
            const float4 vb = *reinterpret_cast<const float4*>(pb);
            raa = has ? va : make_float4(1.f, 1.f, 1.f, 1.f);
            rab = has ? vb : make_float4(0.f, 0.f, 0.f, 0.f);
            ra_slope = first ? slope0 : slope1;
        }
#pragma unroll
        for (int i = 0; i < A_ROWS; ++i) {
            const int iy = a_iyb[i] + ty, ix = a_ixb[i] + tx;
            const bool v = a_mv[i] & ((unsigned)iy < (unsigned)xH) & ((unsigned)(ix + a_kx) < (unsigned)xW) &
                           (!KMASK || cc + a_col4 * 4 < cs);
            const int osel = (a_off0[i] & fmask) | (a_off1[i] & ~fmask);    // bit select: a ?: here became a scratch array
            // unsigned 32-bit element offset from a wave-uniform base: one shift, no 64-bit vector address arithmetic
            const unsigned off = v ? (unsigned)(osel + tapshift) : (unsigned)(a_col4 * 16);
            rav[i] = v ? 1.f : 0.f;
            ra[i] = *reinterpret_cast<const float4*>(sbase + off);
        }
        if (BDMA) return;
        const int ky = ph.ky0 + ty * kstep, kx = ph.kx0 + tx * kstep;
        const char* wtap = reinterpret_cast<const char*>((BMODE == 0) ? wbase + ((long)(ky * KWv + kx) * wC0 + cchf) * wC1
                                                                      : wbase + (long)(ky * KWv + kx) * wC0 * wC1 + cchf);
#pragma unroll
        for (int s = 0; s < B_SLOTS; ++s) {
            if (KMASK) {
                const bool bv = b_kk[s] < kreal;        // k_real % 4 == 0 for NK: the float4 is all in or all out
                rbv[s] = bv ? 1.f : 0.f;
                rb[s] = *reinterpret_cast<const float4*>(wtap + (unsigned)((bv ? b_k[s] : 0) + b_n[s]));
            } else {
                rb[s] = *reinterpret_cast<const float4*>(wtap + (unsigned)(b_k[s] + b_n[s]));
            }
        }
    };

    // BDMA: filter K-tile kt straight into LDS buffer `buf`
    auto dma_b = [&](int kt, int buf) {
        const int tap = div32(kt, mg.mC, mg.oneC);
        const int chunk = kt - tap * tpt;
        const int ty = div32(tap, mg.mTW, mg.oneTW), tx = tap - ty * TWv;
        const int cch = ROWTAP ? 0 : (chunk < nch0 ? chunk * BK : xC0 + (chunk - nch0) * BK);
        const int ky = ph.ky0 + ty * kstep, kx = ph.kx0 + tx * kstep;
        const char* wtap = reinterpret_cast<const char*>((BMODE == 0) ? wbase + ((long)(ky * KWv + kx) * wC0 + cch) * wC1
                                                                      : wbase + (long)(ky * KWv + kx) * wC0 * wC1 + cch);
        // LDS byte address of this wave's first slot (the dynamic LDS segment starts at 0: the kernel has no static LDS)
        const unsigned dst = __builtin_amdgcn_readfirstlane((unsigned)(((Bs - smem) + buf * B_SZ + wave * B_IPW * 256) * 4));
#pragma unroll
        for (int q = 0; q < B_IPW; ++q) glds16(wtap, bd_off[q], dst + q * 1024);
    };

    auto stage = [&](int buf) {
        float* Ab = As + buf * A_SZ;
        float* Bb = Bs + buf * B_SZ;
#pragma unroll
        for (int i = 0; i < A_ROWS; ++i) {
            const float4 v = PLAIN ? mask4(ra[i], rav[i]) : xform4(ra[i], raa, rab, ra_slope, rav[i]);
            float* p = Ab + ((tid >> 3) + 32 * i) * A_LD + a_col4 * 4;
            if (AV) {
                *reinterpret_cast<float4*>(p) = v;
            } else {
                p[0] = v.x; p[1] = v.y; p[2] = v.z; p[3] = v.w;
            }
        }
        if (BDMA) return;
#pragma unroll
        for (int s = 0; s < B_SLOTS; ++s) {
            const float4 v = KMASK ? mask4(rb[s], rbv[s]) : rb[s];
            if (BMODE == 0) {
                *reinterpret_cast<float4*>(Bb + (tid / (BN / 4) + B_RP * s) * B_LD + (tid % (BN / 4)) * 4) = v;
            } else {
                *reinterpret_cast<float4*>(Bb + ((tid >> 3) + 32 * s) * B_LD + (((tid & 7) ^ ((tid >> 4) & 7)) * 4)) = v;
            }
        }
    };

    if (kt_begin < kt_end) {
        const int last = kt_end - 1;
        if (BDMA) dma_b(kt_begin, 0);
        issue_loads(kt_begin);
        stage(0);
        issue_loads(min(kt_begin + 1, last));
        if (BDMA) asm volatile("s_waitcnt vmcnt(%0)" :: "n"(A_ROWS) : "memory");   // the first DMA tile has landed
        __syncthreads();
        int cur = 0;
        for (int kt = kt_begin; kt < kt_end; ++kt) {
            // K index of MFMA step kk on lane half lhi: 16*lhi + kk (any bijection works when A and B agree; this one makes
            // a lane's 16 operands of a K-tile contiguous in the [row][k] images)
            constexpr int KS = 1;                       // k stride between consecutive steps
            const int kl = lhi * (BK / 2);              // k of step 0
            const float* Ab = As + cur * A_SZ + (wm * SM * 32 + l31) * A_LD + kl;
            const float* Bb = (BMODE == 0) ? (Bs + cur * B_SZ + kl * B_LD + wn * SN * 32 + l31)
                                           : (Bs + cur * B_SZ + (wn * SN * 32 + l31) * B_LD);
            const int bsw = (l31 >> 1) & 7;         // NK: chunk swizzle of this lane's rows (the same for every j)
            constexpr int FG = 4, NFG = BK / 2 / FG;
            float av[2][FG][SM], bv[2][FG][SN];
            auto fetch = [&](int g, int buf) {
                if (AV) {
#pragma unroll
                    for (int i = 0; i < SM; ++i) {
                        const float4 v = *reinterpret_cast<const float4*>(Ab + i * 32 * A_LD + g * FG);
                        av[buf][0][i] = v.x; av[buf][1][i] = v.y; av[buf][2][i] = v.z; av[buf][3][i] = v.w;
                    }
                }
                if (BMODE == 1) {       // K index of MFMA step kk on lane half lhi is 16*lhi + kk (as for A when AV): chunk 4*lhi + g
#pragma unroll
                    for (int j = 0; j < SN; ++j) {
                        const float4 v = *reinterpret_cast<const float4*>(Bb + j * 32 * B_LD + (((lhi * 4 + g) ^ bsw) * 4));
                        bv[buf][0][j] = v.x; bv[buf][1][j] = v.y; bv[buf][2][j] = v.z; bv[buf][3][j] = v.w;
                    }
                }
#pragma unroll
                for (int q = 0; q < FG; ++q) {
                    const int kk = g * FG + q;
                    if (!AV) {
#pragma unroll
                        for (int i = 0; i < SM; ++i) av[buf][q][i] = Ab[i * 32 * A_LD + kk * KS];
                    }
                    if (BMODE == 0) {
#pragma unroll
                        for (int j = 0; j < SN; ++j) bv[buf][q][j] = Bb[kk * KS * B_LD + j * 32];
                    }
                }
            };
            auto mfmas = [&](int g) {
#pragma unroll
                for (int q = 0; q < FG; ++q)
#pragma unroll
                    for (int i = 0; i < SM; ++i)
#pragma unroll
                        for (int j = 0; j < SN; ++j)
                            acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[g & 1][q][i], bv[g & 1][q][j], acc[i][j], 0, 0, 0);
            };
            fetch(0, 0);
            fetch(1, 1);
            mfmas(0);
            stage(cur ^ 1);                         // K-tile kt+1: registers -> the LDS buffer nobody reads now
            // the filter tile of K-tile kt+1 into the same free buffer; issued after the staging (whose wait on the register
            // loads would otherwise also wait for the DMA) and before the loads of K-tile kt+2 (so that the counted wait
            // at the end of the step can leave exactly those outstanding)
            if (BDMA) dma_b(min(kt + 1, last), cur ^ 1);
            fetch(2, 0);
            mfmas(1);
            issue_loads(min(kt + 2, last));         // K-tile kt+2 into the registers just drained
            fetch(3, 1);
            mfmas(2);
            mfmas(3);
            // interleave hint: one MFMA, then a few of the independent staging instructions (+1-2 % over the compiler's own order)
#pragma unroll
            for (int q = 0; q < NFG * FG * SM * SN; ++q) {
                __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
                __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
                __builtin_amdgcn_sched_group_barrier(0x002, 3, 0);
                __builtin_amdgcn_sched_group_barrier(0x004, 2, 0);
                __builtin_amdgcn_sched_group_barrier(0x220, 1, 0);
            }
            if (BDMA) {
                // counted wait instead of __syncthreads(): its fence would wait vmcnt(0) and drain the register prefetch of
                // K-tile kt+2 with the DMA.  vmcnt retires in order and the A_ROWS gather loads are the last vector-memory
                // operations issued after the DMA on every path (the norm-table loads, when a source has a table, come before
                // them): at most A_ROWS outstanding means the DMA has landed.  lgkmcnt(0): this wave's ds_writes of the A tile.
                asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)" :: "n"(A_ROWS) : "memory");
                __builtin_amdgcn_s_barrier();
            } else {
                __syncthreads();
            }
            cur ^= 1;
        }
    }

    // ---- epilogue ----
    ut_epilogue<BM, BN, WM, WN, SM, SN, 2 * (A_SZ + B_SZ)>(acc, d, smem, rowpix, part, ks, sk, slot, flags, ts_s, splitk, slab_base,
                                                          slab_stride, m0, n0, phase, M, g_sk_cfg);
}


// streaming 16-byte load (split-K slabs are read once)
typedef float nt_f32x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ float4 ntload4(const float4* p) {
    const nt_f32x4 v = __builtin_nontemporal_load(reinterpret_cast<const nt_f32x4*>(p));
    return make_float4(v.x, v.y, v.z, v.w);
}

// sum split-K slabs; applies the epilogue that the partial passes skipped
__global__ void slab_reduce_kernel(const float* __restrict__ slabs, long slab_stride, int splitk,
                                   float* __restrict__ out, long count, int ldc, int Nn, int Nstore,
                                   const float* bias, int epi, int accumulate) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    const int col = (int)(i % ldc);
    if (col >= Nstore) return;   // columns the partial passes never wrote
    float v = 0.f;
    for (int s = 0; s < splitk; ++s) v += slabs[(long)s * slab_stride + i];
    if (bias != nullptr && col < Nn) v += bias[col];
    if (epi == 1) v = tanhf(v);
    else if (epi == 2) v = fmaxf(v, 0.2f * v);
    if (accumulate) v += out[i];
    out[i] = v;
}

// the same sum, four columns per thread (16-byte loads, four slabs in flight; the additions keep the scalar kernel's order,
// so both give the same bits): ldc, Nn, Nstore multiples of 4 and 16-byte aligned bases
__global__ __launch_bounds__(256) void slab_reduce4_kernel(const float4* __restrict__ slabs, long slab_stride4, int splitk,
                                                            float4* __restrict__ out, long count4, int ldc4, int Nn4,
                                                            int Nstore4, const float4* bias, int epi, int accumulate) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count4) return;
    const int col = (int)(i % ldc4);
    if (col >= Nstore4) return;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    const float4* p = slabs + i;
    int s = 0;
    for (; s + 4 <= splitk; s += 4) {
        const float4 a = ntload4(p), b = ntload4(p + slab_stride4),
                     c = ntload4(p + 2 * slab_stride4), e = ntload4(p + 3 * slab_stride4);
        p += 4 * slab_stride4;
        v.x += a.x; v.y += a.y; v.z += a.z; v.w += a.w;
        v.x += b.x; v.y += b.y; v.z += b.z; v.w += b.w;
        v.x += c.x; v.y += c.y; v.z += c.z; v.w += c.w;
        v.x += e.x; v.y += e.y; v.z += e.z; v.w += e.w;
    }
    for (; s < splitk; ++s, p += slab_stride4) {
        const float4 a = ntload4(p);
        v.x += a.x; v.y += a.y; v.z += a.z; v.w += a.w;
    }
    if (bias != nullptr && col < Nn4) {
        const float4 b = bias[col];
        v.x += b.x; v.y += b.y; v.z += b.z; v.w += b.w;
    }
    if (epi == 1) { v.x = tanhf(v.x); v.y = tanhf(v.y); v.z = tanhf(v.z); v.w = tanhf(v.w); }
    else if (epi == 2) { v.x = fmaxf(v.x, 0.2f * v.x); v.y = fmaxf(v.y, 0.2f * v.y); v.z = fmaxf(v.z, 0.2f * v.z); v.w = fmaxf(v.w, 0.2f * v.w); }
    if (accumulate) {
        const float4 o = out[i];
        v.x += o.x; v.y += o.y; v.z += o.z; v.w += o.w;
    }
    out[i] = v;
}

// The slab sum of a conv whose output feeds a batch-statistics norm: the sum touches every output element once, so it takes
// the per-column sum and sum of squares on the way (rows of partials per block, folded by bn_stats_finalize) instead of a
// statistics pass of its own over the tensor.  A thread keeps one group of 4 columns (256 % (ldc / 4) == 0) and walks rows;
// the additions over the slabs keep slab_reduce4_kernel's order (same output bits).
__global__ __launch_bounds__(256) void slab_reduce4_stats_kernel(const float4* __restrict__ slabs, long slab_stride4, int splitk,
                                                                  float4* __restrict__ out, long rows, int cg,
                                                                  float* __restrict__ stat) {
    __shared__ float4 sh[2][256];
    const int R = 256 / cg;
    const int c = threadIdx.x % cg, rl = threadIdx.x / cg;
    float4 s = make_float4(0.f, 0.f, 0.f, 0.f), q = s;
    for (long r = (long)blockIdx.x * R + rl; r < rows; r += (long)gridDim.x * R) {
        const long i = r * cg + c;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        const float4* p = slabs + i;
        int k = 0;
        for (; k + 4 <= splitk; k += 4) {
            const float4 a = ntload4(p), b = ntload4(p + slab_stride4), c2 = ntload4(p + 2 * slab_stride4),
                         e = ntload4(p + 3 * slab_stride4);
            p += 4 * slab_stride4;
            v.x += a.x; v.y += a.y; v.z += a.z; v.w += a.w;
            v.x += b.x; v.y += b.y; v.z += b.z; v.w += b.w;
            v.x += c2.x; v.y += c2.y; v.z += c2.z; v.w += c2.w;
            v.x += e.x; v.y += e.y; v.z += e.z; v.w += e.w;
        }
        for (; k < splitk; ++k, p += slab_stride4) {
            const float4 a = ntload4(p);
            v.x += a.x; v.y += a.y; v.z += a.z; v.w += a.w;
        }
        out[i] = v;
        s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
        q.x += v.x * v.x; q.y += v.y * v.y; q.z += v.z * v.z; q.w += v.w * v.w;
    }
    sh[0][threadIdx.x] = s;
    sh[1][threadIdx.x] = q;
    __syncthreads();
    if (rl == 0) {
        for (int k = 1; k < R; ++k) {
            const float4 a = sh[0][k * cg + c], b = sh[1][k * cg + c];
            s.x += a.x; s.y += a.y; s.z += a.z; s.w += a.w;
            q.x += b.x; q.y += b.y; q.z += b.z; q.w += b.w;
        }
        float* sp = stat + (long)blockIdx.x * 2 * (4 * cg);
        *reinterpret_cast<float4*>(sp + 4 * c) = s;
        *reinterpret_cast<float4*>(sp + 4 * cg + 4 * c) = q;
    }
}

static bool slab_stats_ok(const ssc_conv_desc& d) {
    const int cg = d.ldc / 4;
    return (d.ldc & 3) == 0 && cg >= 1 && cg <= 256 && (256 % cg) == 0 && d.Nn == d.ldc && d.Nstore == d.ldc &&
           d.bias == nullptr && d.epi == 0 && !d.accumulate && ((uintptr_t)d.out & 15) == 0;
}
// rows of partial sums the statistics form of the slab sum writes (one per block)
static int slab_stats_blocks(long rows, int ldc) {
    const int R = 256 / (ldc / 4);
    long b = ((rows + R - 1) / R + 3) / 4;
    if (b > 1024) b = 1024;
    if (b < 1) b = 1;
    return (int)b;
}

static void launch_slab_reduce(const float* ws, long out_count, int splitk, const ssc_conv_desc& d, hipStream_t st) {
    const int thr = 256;
    if (d.stat_partial != nullptr && slab_stats_ok(d) && ((uintptr_t)ws & 15) == 0 && (out_count % 4) == 0) {
        const long rows = out_count / d.ldc;
        hipLaunchKernelGGL(slab_reduce4_stats_kernel, dim3((unsigned)slab_stats_blocks(rows, d.ldc)), dim3(256), 0, st,
                           (const float4*)ws, out_count / 4, splitk, (float4*)d.out, rows, d.ldc / 4, d.stat_partial);
        return;
    }
    const bool v4 = (out_count % 4) == 0 && (d.ldc % 4) == 0 && (d.Nn % 4) == 0 && (d.Nstore % 4) == 0 &&
                    (((uintptr_t)ws | (uintptr_t)d.out | (uintptr_t)d.bias) & 15) == 0;
    if (v4) {
        const long c4 = out_count / 4;
        hipLaunchKernelGGL(slab_reduce4_kernel, dim3((unsigned)((c4 + thr - 1) / thr)), dim3(thr), 0, st, (const float4*)ws,
                           c4, splitk, (float4*)d.out, c4, d.ldc / 4, d.Nn / 4, d.Nstore / 4, (const float4*)d.bias, d.epi,
                           d.accumulate);
    } else {
        hipLaunchKernelGGL(slab_reduce_kernel, dim3((unsigned)((out_count + thr - 1) / thr)), dim3(thr), 0, st, ws,
                           out_count, splitk, d.out, out_count, d.ldc, d.Nn, d.Nstore, d.bias, d.epi, d.accumulate);
    }
}

// igemm_bf16.hip sums its split-K slabs with the same kernels
void ssc_launch_slab_reduce(const float* ws, long out_count, int splitk, const ssc_conv_desc& d, hipStream_t st) {
    launch_slab_reduce(ws, out_count, splitk, d, st);
}

// ---------------------------------------------------------------------------------------------
// filter-gradient form
// ---------------------------------------------------------------------------------------------
// One K-tile step is a single branch-free block, as in conv_ut_kernel: K-tile kt+1 goes from registers to the free LDS
// buffer and K-tile kt+2 is loaded into the drained registers between the MFMAs of K-tile kt.  GPLAIN / DPLAIN: the
// gathered / dense view has no folded norm and no activation on any source (decided per launch).
template <int WM, int WN, int SM, int SN, bool GPLAIN, bool DPLAIN, bool DDMA>
__global__ __launch_bounds__(256) void conv_wgrad_kernel(const ssc_wgrad_desc d, const Magics mg,
                                                          float* __restrict__ slab_base, long slab_stride,
                                                          int splitk, int xcd) {
    constexpr int BM = WM * SM * 32;
    constexpr int BN = WN * SN * 32;
    constexpr int A_LD = BM;
    constexpr int B_LD = BN;
    constexpr int A_SZ = BK * BM;
    constexpr int B_SZ = BK * BN;
    constexpr int A_SLOTS = BM / 32;
    constexpr int B_SLOTS = BN / 32;
    constexpr int A_RP = 1024 / BM;   // pixel rows per pass
    constexpr int B_RP = 1024 / BN;
    // DDMA (dense side = one tensor without norm / activation, e.g. every dy): its [pixel][channel] tile goes to LDS by
    // LDS-DMA as the filter tiles of conv_ut_kernel do -- a wave instruction covers 256 / BN pixel rows
    constexpr int B_IPW = BK * BN / 1024;
    static_assert(!DDMA || DPLAIN, "DMA tiles cannot be transformed");

    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* As = smem;
    float* Bs = smem + 2 * A_SZ;
    // per-pixel decode of the K-tile after next, shared by the whole workgroup: {pixel index of (n, iy0, ix0) in the
    // gathered tensor, iy0, ix0} with iy0 = py*stride + ioff_y (tap offsets are per-thread constants)
    int4* ptab = reinterpret_cast<int4*>(smem + 2 * A_SZ + 2 * B_SZ);      // [2][BK]

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int wm = wave / WN, wn = wave % WN;

    const int Cg = d.g.C0 + d.g.C1;
    const int Cd = d.d.C0 + d.d.C1;
    const int Mtot = d.TH * d.TW * Cg;
    const long P = (long)d.NB * d.PH * d.PW;
    const int PHW = d.PH * d.PW;
    // workgroup -> (row tile, column tile, K slice).  All tiles of a K slice read the same pixels (every (tap, channel) block of
    // the gathered side and every block of the dense side of that pixel range), so they should meet in ONE L2: with the plain
    // grid order a slice's tiles are dealt round-robin to the 8 XCDs and each of them fetches the range.  xcd (host flag): ids
    // with the same id % 8 walk a contiguous run of (row tile, column tile, slice) order -- whole slices per XCD.
    int ks = blockIdx.z, mtile = blockIdx.x, ntile = blockIdx.y;
    if (xcd) {
        const unsigned total = gridDim.x * gridDim.y * gridDim.z;
        const unsigned lin = blockIdx.x + gridDim.x * (blockIdx.y + gridDim.y * blockIdx.z);
        const unsigned t2 = (lin & 7u) * (total >> 3) + (lin >> 3);
        const unsigned per_slice = gridDim.x * gridDim.y;
        ks = (int)(t2 / per_slice);
        const unsigned r = t2 - (unsigned)ks * per_slice;
        ntile = (int)(r / gridDim.x);
        mtile = (int)(r - (unsigned)ntile * gridDim.x);
    }
    const int m0 = mtile * BM;
    const int n0 = ntile * BN;

    // fixed per-thread columns: (tap, channel) of the gathered side, channel of the dense side
    const int a_col = m0 + (tid % (BM / 4)) * 4;
    const bool a_cv = a_col < Mtot;
    const int a_cc = a_cv ? a_col : 0;
    const int a_tap = div32(a_cc, mg.mC, mg.oneC);
    const int a_c = a_cc - a_tap * Cg;
    const int a_ty = div32(a_tap, mg.mTW, mg.oneTW), a_tx = a_tap - a_ty * d.TW;
    float4 aa, ab;
    gview_affine4(d.g, a_c, aa, ab);
    const float* a_base;
    int a_cs;
    gview_src(d.g, a_c, a_base, a_cs);
    const int a_act = (a_c >= d.g.C0 && d.g.act1 >= 0) ? d.g.act1 : d.g.act;
    const int b_col = n0 + (tid % (BN / 4)) * 4;
    const bool b_cv = b_col < Cd;
    const int b_c = b_cv ? b_col : 0;
    float4 ba, bb;
    gview_affine4(d.d, b_c, ba, bb);
    const float* b_base;
    int b_cs;
    gview_src(d.d, b_c, b_base, b_cs);
    const int b_act = (b_c >= d.d.C0 && d.d.act1 >= 0) ? d.d.act1 : d.d.act;

    // 32-bit K-tile arithmetic (the host checks P < 2^31 and every tensor < 2^29 elements: byte offsets fit 32 bits)
    const int nkt = (int)((P + BK - 1) / BK);
    const int per = (nkt + splitk - 1) / splitk;
    const int kt_begin = ks * per;
    const int kt_end = min(nkt, kt_begin + per);

    f32x16 acc[SM][SN];
#pragma unroll
    for (int i = 0; i < SM; ++i)
#pragma unroll
        for (int j = 0; j < SN; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    float4 ra[A_SLOTS], rb[B_SLOTS];
    float rav[A_SLOTS];
    const float g_slope = act_slope(a_act), d_slope = act_slope(b_act);

    // one thread per pixel of K-tile `kt` fills ptab[kt & 1] (threads 0..BK-1): {byte offset of (n, iy0, ix0) in source 0,
    // iy0, ix0, byte offset in source 1} with iy0 = py*stride + ioff_y (tap offsets are per-thread constants)
    const int gC0b = d.g.C0 * 4, gC1b = d.g.C1 * 4;
    const unsigned Pu = (unsigned)P;
    auto fill_ptab = [&](int kt) {
        // the waves take turns (K-tile kt is decoded by wave kt & 3): the decode is ~35 vector instructions that only
        // 32 lanes need, and a wave that did it every step would be the one the barrier waits for
        if ((wave == (kt & 3)) & (lane < BK)) {
            const unsigned p = (unsigned)kt * BK + lane;
            const bool pv = p < Pu;
            const long pp = pv ? (long)p : 0;
            int n, py, px;
            if (mg.use32) {     // wave-uniform: numerators fit the 32-bit multiply-high
                n = (int)__umulhi((unsigned)pp, mg.mPHPW32) + (int)((unsigned)pp & (unsigned)mg.onePHPW);
                const int rem = (int)pp - n * PHW;
                py = (int)__umulhi((unsigned)rem, mg.mPW32) + (int)((unsigned)rem & (unsigned)mg.onePW);
                px = rem - py * d.PW;
            } else {
                n = (int)div64(pp, mg.mPHPW, mg.onePHPW);
                const int rem = (int)(pp - (long)n * PHW);
                py = (int)div64(rem, mg.mPW, mg.onePW);
                px = rem - py * d.PW;
            }
            const int iy0 = py * d.in_stride + d.ioff_y, ix0 = px * d.in_stride + d.ioff_x;
            const int pix = (n * d.g.H + iy0) * d.g.W + ix0;
            // an invalid pixel gets coordinates no tap can bring inside the image
            ptab[(kt & 1) * BK + lane] = make_int4(pix * gC0b, pv ? iy0 : -(1 << 20), ix0, pix * gC1b);
        }
    };
    // per-thread constants of the gathered side: which ptab word holds this thread's source offset, the tap's byte shift
    const bool a_first = a_c < d.g.C0;
    const int a_tapb = (a_ty * d.g.W + a_tx) * a_cs * 4;
    const char* const a_bytes = reinterpret_cast<const char*>(a_base);
    const int gH = d.g.H, gW = d.g.W;
    // dense side: rows beyond the last pixel are CLAMPED to it, not masked -- the gathered side of those rows is staged as
    // zeros (ptab marks them invalid), so what they hold never reaches a sum; every load is unconditional and unmasked
    const char* const b_bytes = reinterpret_cast<const char*>(b_base);
    const unsigned b_rowb = (unsigned)b_cs * 4u;
    const unsigned b_last = (unsigned)(P - 1) * b_rowb;
    unsigned b_off[B_SLOTS];
#pragma unroll
    for (int s = 0; s < B_SLOTS; ++s) b_off[s] = (unsigned)(tid / (BN / 4) + B_RP * s) * b_rowb;
    const unsigned b_step = (unsigned)BK * b_rowb;
    unsigned d_row[B_IPW];      // DDMA: byte offset of this lane's pixel row inside a K-tile, per instruction of its wave
    const unsigned d_col = (n0 + (lane % (BN / 4)) * 4) < Cd ? (unsigned)((n0 + (lane % (BN / 4)) * 4) * 4) : 0u;
#pragma unroll
    for (int q = 0; q < B_IPW; ++q) d_row[q] = (unsigned)((wave * B_IPW + q) * (256 / BN) + lane / (BN / 4)) * b_rowb;
    auto dma_d = [&](int kt, int buf) {
        const unsigned kb = (unsigned)kt * b_step;
        const unsigned dst = __builtin_amdgcn_readfirstlane((unsigned)((2 * A_SZ + buf * B_SZ + wave * B_IPW * 256) * 4));
#pragma unroll
        for (int q = 0; q < B_IPW; ++q)
            glds16(reinterpret_cast<const char*>(d.d.s0), min(kb + d_row[q], b_last) + d_col, dst + q * 1024);
    };
    auto load_tile = [&](int kt) {
#pragma unroll
        for (int s = 0; s < A_SLOTS; ++s) {
            const int4 e = ptab[(kt & 1) * BK + tid / (BM / 4) + A_RP * s];
            const int iy = e.y + a_ty, ix = e.z + a_tx;
            const bool v = a_cv & ((unsigned)iy < (unsigned)gH) & ((unsigned)ix < (unsigned)gW);
            const unsigned off = v ? (unsigned)((a_first ? e.x : e.w) + a_tapb) : 0u;
            rav[s] = v ? 1.f : 0.f;
            ra[s] = *reinterpret_cast<const float4*>(a_bytes + off);
        }
        if (DDMA) return;
        const unsigned kb = (unsigned)kt * b_step;
#pragma unroll
        for (int s = 0; s < B_SLOTS; ++s) {
            const unsigned off = min(kb + b_off[s], b_last);
            rb[s] = *reinterpret_cast<const float4*>(b_bytes + (b_cv ? off : 0u));
        }
    };
    auto store_tile = [&](int buf) {
        float* Ab = As + buf * A_SZ;
        float* Bb = Bs + buf * B_SZ;
#pragma unroll
        for (int s = 0; s < A_SLOTS; ++s) {
            const int row = tid / (BM / 4) + A_RP * s;
            *reinterpret_cast<float4*>(Ab + row * A_LD + (tid % (BM / 4)) * 4) =
                GPLAIN ? mask4(ra[s], rav[s]) : xform4(ra[s], aa, ab, g_slope, rav[s]);
        }
        if (DDMA) return;
#pragma unroll
        for (int s = 0; s < B_SLOTS; ++s) {
            const int row = tid / (BN / 4) + B_RP * s;
            *reinterpret_cast<float4*>(Bb + row * B_LD + (tid % (BN / 4)) * 4) =
                DPLAIN ? rb[s] : xform4(rb[s], ba, bb, d_slope, 1.f);
        }
    };

    const int l31 = lane & 31, lhi = lane >> 5;
    if (kt_begin < kt_end) {
        // K-tiles past kt_end (another split's, or past the last pixel: every row masked) are staged but never multiplied
        if (DDMA) dma_d(kt_begin, 0);
        fill_ptab(kt_begin);
        fill_ptab(kt_begin + 1);
        __syncthreads();
        load_tile(kt_begin);
        store_tile(0);
        load_tile(kt_begin + 1);
        if (DDMA) asm volatile("s_waitcnt vmcnt(%0)" :: "n"(A_SLOTS) : "memory");      // the first dense tile has landed
        __syncthreads();                    // every thread has read ptab slots kt_begin, kt_begin + 1
        fill_ptab(kt_begin + 2);
        __syncthreads();
        int cur = 0;
        for (int kt = kt_begin; kt < kt_end; ++kt) {
            const float* Ab = As + cur * A_SZ + lhi * A_LD + wm * SM * 32 + l31;
            const float* Bb = Bs + cur * B_SZ + lhi * B_LD + wn * SN * 32 + l31;
            constexpr int FG = 4, NFG = BK / 2 / FG;
            float av[2][FG][SM], bv[2][FG][SN];
            auto fetch = [&](int g, int buf) {
#pragma unroll
                for (int q = 0; q < FG; ++q) {
                    const int kk = g * FG + q;
#pragma unroll
                    for (int i = 0; i < SM; ++i) av[buf][q][i] = Ab[kk * 2 * A_LD + i * 32];
#pragma unroll
                    for (int j = 0; j < SN; ++j) bv[buf][q][j] = Bb[kk * 2 * B_LD + j * 32];
                }
            };
            auto mfmas = [&](int g) {
#pragma unroll
                for (int q = 0; q < FG; ++q)
#pragma unroll
                    for (int i = 0; i < SM; ++i)
#pragma unroll
                        for (int j = 0; j < SN; ++j)
                            acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[g & 1][q][i], bv[g & 1][q][j], acc[i][j], 0, 0, 0);
            };
            fill_ptab(kt + 3);              // overwrites ptab[(kt+1)&1], last read before the previous barrier; its
                                            // lane-divergent branch stays in front of the MFMA block, not inside it
            fetch(0, 0);
            fetch(1, 1);
            mfmas(0);
            store_tile(cur ^ 1);            // K-tile kt+1: registers -> the LDS buffer nobody reads now
            if (DDMA) dma_d(kt + 1, cur ^ 1);       // its dense tile: DMA into the same free buffer (see conv_ut_kernel)
            fetch(2, 0);
            mfmas(1);
            load_tile(kt + 2);              // reads ptab[(kt+2)&1], published by the previous barrier
            fetch(3, 1);
            mfmas(2);
            mfmas(3);
#pragma unroll
            for (int q = 0; q < NFG * FG * SM * SN; ++q) {      // interleave hint, as in conv_ut_kernel
                __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
                __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
                __builtin_amdgcn_sched_group_barrier(0x002, 3, 0);
                __builtin_amdgcn_sched_group_barrier(0x004, 2, 0);
                __builtin_amdgcn_sched_group_barrier(0x220, 1, 0);
            }
            if (DDMA) {     // counted wait + bare barrier: the gathered loads of K-tile kt+2 stay in flight (conv_ut_kernel)
                asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)" :: "n"(A_SLOTS) : "memory");
                __builtin_amdgcn_s_barrier();
            } else {
                __syncthreads();
            }
            cur ^= 1;
        }
    }

    float* outp = (splitk > 1) ? (slab_base + (long)ks * slab_stride) : d.out;
#pragma unroll
    for (int i = 0; i < SM; ++i) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int m = m0 + wm * SM * 32 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * lhi;
            if (m >= Mtot) continue;
            const int tap = div32(m, mg.mC, mg.oneC);
            const int c = m - tap * Cg;
            if (c >= d.Cg_real) continue;
            const long orow = (long)tap * d.Cg_real + c;
#pragma unroll
            for (int j = 0; j < SN; ++j) {
                const int col = n0 + wn * SN * 32 + j * 32 + l31;
                if (col >= d.Nn) continue;
                float v = acc[i][j][r];
                float* o = outp + orow * d.ldc + col;
                if (splitk == 1 && d.accumulate) v += *o;
                *o = v;
            }
        }
    }
}

// Sum of the split-K slabs of a filter gradient.  Small filters (1x1 / 3x3 convs of the residual blocks: 10^4-10^5
// elements) are split hundreds of ways over the pixels, so one thread per element would leave a few dozen workgroups
// walking hundreds of slabs each: L threads share an element (slabs s, s+L, ...) and combine through LDS in a fixed order.
template <int L>
__global__ __launch_bounds__(256) void wgrad_reduce_kernel(const float* __restrict__ slabs, long slab_stride, int splitk,
                                                           float* __restrict__ out, long count, int accumulate) {
    constexpr int EPB = 256 / L;        // elements per block
    __shared__ float part[256];
    const int e = threadIdx.x % EPB, ls = threadIdx.x / EPB;
    const long i = (long)blockIdx.x * EPB + e;
    float v = 0.f;
    if (i < count)
        for (int s = ls; s < splitk; s += L) v += slabs[(long)s * slab_stride + i];
    if (L > 1) {
        part[threadIdx.x] = v;
        __syncthreads();
        if (ls == 0)
            for (int l = 1; l < L; ++l) v += part[l * EPB + e];
    }
    if (ls == 0 && i < count) {
        if (accumulate) v += out[i];
        out[i] = v;
    }
}

// one thread per four elements: 16-byte loads, four slabs in flight, the scalar kernel's order of additions (same bits)
__global__ __launch_bounds__(256) void wgrad_reduce4_kernel(const float4* __restrict__ slabs, long slab_stride4, int splitk,
                                                             float4* __restrict__ out, long count4, int accumulate) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= count4) return;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    const float4* p = slabs + i;
    int s = 0;
    for (; s + 4 <= splitk; s += 4) {
        const float4 a = ntload4(p), b = ntload4(p + slab_stride4),
                     c = ntload4(p + 2 * slab_stride4), e = ntload4(p + 3 * slab_stride4);
        p += 4 * slab_stride4;
        v.x += a.x; v.y += a.y; v.z += a.z; v.w += a.w;
        v.x += b.x; v.y += b.y; v.z += b.z; v.w += b.w;
        v.x += c.x; v.y += c.y; v.z += c.z; v.w += c.w;
        v.x += e.x; v.y += e.y; v.z += e.z; v.w += e.w;
    }
    for (; s < splitk; ++s, p += slab_stride4) {
        const float4 a = ntload4(p);
        v.x += a.x; v.y += a.y; v.z += a.z; v.w += a.w;
    }
    if (accumulate) {
        const float4 o = out[i];
        v.x += o.x; v.y += o.y; v.z += o.z; v.w += o.w;
    }
    out[i] = v;
}

// which kernel sums the slabs: 1 wgrad_reduce4_kernel, 2 wgrad_reduce_kernel<1>, 3 <4>, 4 <16>
static int wgrad_reduce_form(const float* ws, long count, int splitk, const float* out) {
    if (count >= 262144 || splitk < 8)
        return ((count % 4) == 0 && (((uintptr_t)ws | (uintptr_t)out) & 15) == 0) ? 1 : 2;
    return (count >= 65536 || splitk < 32) ? 3 : 4;
}

static void launch_wgrad_reduce(const float* ws, long count, int splitk, float* out, int accumulate, hipStream_t st) {
    switch (wgrad_reduce_form(ws, count, splitk, out)) {
        case 1: {
            const long c4 = count / 4;
            hipLaunchKernelGGL(wgrad_reduce4_kernel, dim3((unsigned)((c4 + 255) / 256)), dim3(256), 0, st, (const float4*)ws, c4,
                               splitk, (float4*)out, c4, accumulate);
            break;
        }
        case 2:
            hipLaunchKernelGGL(wgrad_reduce_kernel<1>, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, st, ws, count,
                               splitk, out, count, accumulate);
            break;
        case 3:
            hipLaunchKernelGGL(wgrad_reduce_kernel<4>, dim3((unsigned)((count + 63) / 64)), dim3(256), 0, st, ws, count, splitk,
                               out, count, accumulate);
            break;
        default:
            hipLaunchKernelGGL(wgrad_reduce_kernel<16>, dim3((unsigned)((count + 15) / 16)), dim3(256), 0, st, ws, count, splitk,
                               out, count, accumulate);
            break;
    }
}

// wgrad128.hip sums its split-K slabs with the same kernels
void ssc_launch_wgrad_reduce(const float* ws, long count, int splitk, float* out, int accumulate, hipStream_t st) {
    launch_wgrad_reduce(ws, count, splitk, out, accumulate, st);
}

#ifdef SSC_ISA_ONLY
// scripts/isa_one.sh: compile a single instantiation to look at its ISA (the whole file takes over a minute)
template __global__ void conv_ut_kernel<2, 2, 1, 2, 0, false, 0>(const ssc_conv_desc, const Magics, float*, long, int, int, int, unsigned*);
template __global__ void conv_ut_kernel<2, 2, 1, 2, 1, true, 0>(const ssc_conv_desc, const Magics, float*, long, int, int, int, unsigned*);
template __global__ void conv_wgrad_kernel<1, 4, 2, 1, false, true, true>(const ssc_wgrad_desc, const Magics, float*, long, int, int);
#else
// ---------------------------------------------------------------------------------------------
// host launchers (C ABI)
// ---------------------------------------------------------------------------------------------
static int num_cu() { return ssc_num_cu(); }

// Tile configurations.  `res` = workgroups resident per CU (LDS-limited), `penalty` = relative cost of the
// staging instructions per MFMA (fp32 MFMA does not overlap VALU on gfx950).
struct TileCfg { int id, BM, BN, res; double penalty; };
// penalties from the measured instruction mix: ~16 VALU per staged A row-float4 (bounds + transform), ~3 per
// filter float4, 4 cycles each, against 64 cycles per MFMA: (MFMA + VALU) / MFMA, normalised to 128x128
static const TileCfg FWD_CFGS[5] = {{0, 128, 128, 2, 1.00}, {1, 64, 128, 3, 1.03}, {2, 128, 64, 3, 1.11}, {3, 128, 32, 3, 1.33},
                                    {4, 64, 64, 4, 1.30}};    // 64x64: small-M GEMMs (LSTM steps) that leave CUs under-filled
// the bf16-split form (igemm_bf16.hip): larger LDS images (fewer resident workgroups), the same ids; 128x32 is not built
static const TileCfg BF_CFGS[5] = {{0, 128, 128, 1, 1.05}, {1, 64, 128, 2, 1.00}, {2, 128, 64, 2, 1.12}, {3, 128, 32, 1, 9.9},
                                   {4, 64, 64, 3, 1.40}};     // measured on the batch-32 layers: 64x128 ahead of 128x128 / 128x64 by ~9 %, 64x64 behind by ~15 %
static const TileCfg WG_CFGS[5] = {{0, 128, 128, 2, 1.00}, {1, 64, 128, 3, 1.00}, {2, 128, 64, 3, 1.10}, {3, 64, 64, 4, 1.2},
                                   {4, 128, 32, 4, 1.3}};

// Makespan model of one launch: `blocks` equal workgroups of `w` MFMA-cycles each on ncu CUs that hold `res`
// of them at a time and are matrix-pipe bound (co-resident workgroups share the pipe).  Split-K by s divides w
// and multiplies the block count, at the price of writing + re-reading s partial copies of the output.
// The planner's constants are developer switches while tuning (SSC_PLAN_*, read once).
static double makespan(long blocks, double w, int res, int ncu) {
    const long slots = (long)ncu * res;
    const long full = blocks / slots, rem = blocks % slots;
    double t = (double)(full * res + (rem + ncu - 1) / ncu) * w;
    // a lone wave per SIMD cannot hide its own LDS / barrier / load waits (measured: 1 workgroup per CU runs
    // ~25 % below 3 per CU at equal work)
    const long per_cu = (blocks + ncu - 1) / ncu;
    const long occ = per_cu < res ? per_cu : res;
    static const double occ1 = ssc_dev_double("SSC_PLAN_OCC1", 1.30), occ2 = ssc_dev_double("SSC_PLAN_OCC2", 1.08);
    if (occ <= 1) t *= occ1;
    else if (occ == 2) t *= occ2;
    return t;
}

// cycles charged for the launch that sums split-K slabs
static double plan_reduce_cost() {
    static const double c = ssc_dev_double("SSC_PLAN_REDUCE", 6000.0);
    return c;
}

struct Plan { int cfg; int splitk; double cost; long ts_full; int ts_s; };
constexpr long TS_MAX_SLICES = 8;       // most in-launch K slices per tile of the tail split

static Plan plan_launch(const TileCfg* cfgs, int ncfg, const bool* allowed, long M, long N, long nphase, long nkt,
                        long out_elems, int64_t ws_bytes, bool have_ws, bool can_ts = false, double cyc_scale = 1.0) {
    const int ncu = num_cu();
    Plan best = {-1, 1, 1e300, 0, 1};
    // SSC_FWD_CFG=n (tests, tuning) restricts the search to tile configuration n where allowed
    static const int force = [] { const char* e = getenv("SSC_FWD_CFG"); return e != nullptr ? atoi(e) : -1; }();
    for (int c = 0; c < ncfg; ++c) {
        if (!allowed[c]) continue;
        if (force >= 0 && c != force && allowed[force]) continue;
        const TileCfg& t = cfgs[c];
        const long mt = (M + t.BM - 1) / t.BM, nt = (N + t.BN - 1) / t.BN;
        const long blocks = mt * nt * nphase;
        const double wfull = (double)nkt * 16.0 * (t.BM / 32) * (t.BN / 32) / 4.0 * 64.0 * t.penalty * cyc_scale;  // cycles
        for (int sk = 1; sk <= 16; ++sk) {
            if (sk > 1 && (!have_ws || nkt / sk < 4 || (int64_t)sk * out_elems * 4 > ws_bytes)) break;
            const long per = (nkt + sk - 1) / sk;
            if ((nkt + per - 1) / per != sk) continue;      // would leave empty trailing splits
            double cost = makespan(blocks * sk, wfull * (double)per / (double)nkt, t.res, ncu) + 2500.0;
            if (sk > 1) cost += 2.0 * sk * (double)out_elems * 4.0 / 1500.0 + plan_reduce_cost();   // slab traffic + reduce launch
            const long bf = blocks;
            const int bs = 1;
            if (cost < best.cost) best = {c, sk, cost, bf, bs};
        }
    }
    // Whole tiles + K slices combined inside the launch (launch_fwd_ut).  Measured on the batch-32 layers with 64x128 tiles
    // (scripts/ts_sweep.sh): the best layout is as many whole tiles as fill whole rounds of one workgroup per CU, the rest
    // cut into about (CUs / remaining tiles) slices, i.e. one more workgroup per CU -- encoder_3 (576 tiles) 97 -> 115
    // TFLOP/s as 512 + 64 x 4, encoder_2 (1152) 105 -> 115 as 1024 + 128 x 2.  Slicing more tiles than that loses to the
    // fixed cost of a workgroup (first loads, epilogue, hand-off), split-K slabs + reduce kernel lose to both.
    if (can_ts && have_ws && best.cfg >= 0) {
        const TileCfg& t = cfgs[best.cfg];
        const long blocks = ((M + t.BM - 1) / t.BM) * ((N + t.BN - 1) / t.BN) * nphase;
        long full = (blocks / ncu) * ncu, tail = blocks - full;
        long sl = 1;
        struct TsForce { int full = -1, slices = -1; };
        static const TsForce force_ts = [] {       // SSC_TS_FORCE="whole tiles per CU,slices" pins the layout (tests, tuning)
            TsForce f;
            const char* e = getenv("SSC_TS_FORCE");
            if (e != nullptr) sscanf(e, "%d,%d", &f.full, &f.slices);
            return f;
        }();
        const int ff = force_ts.full, fs = force_ts.slices;
        if (ff >= 0 && fs >= 1) {
            full = (long)ff * ncu;
            if (full > blocks) full = (blocks / ncu) * ncu;
            tail = blocks - full;
            sl = tail > 0 ? fs : 1;
        } else if (full > 0 && tail > 0 && tail * 4 <= (long)ncu * 3) {
            sl = (ncu + tail / 2) / tail;
            if (sl > TS_MAX_SLICES) sl = TS_MAX_SLICES;
            while (sl > 1 && nkt / sl < 4) --sl;
        }
        if (sl > 1 && tail * sl < SSC_SK_FLAG_WORDS - 1 && (int64_t)tail * sl * t.BM * t.BN * 4 <= ws_bytes) {
            best.splitk = 1;
            best.ts_full = full;
            best.ts_s = (int)sl;
        }
    }
    return best;
}

template <int WM, int WN, int SM, int SN, int BMODE, bool VECB>
static int launch_fwd_v(const ssc_conv_desc& d, int splitk, float* ws, hipStream_t st) {
    constexpr int BM = WM * SM * 32, BN = WN * SN * 32;
    constexpr int A_SZ = BM * (BK + 1);
    constexpr int B_SZ = (BMODE == 0) ? BK * BN : BN * (BK + 1);
    constexpr size_t lds = 2 * (A_SZ + B_SZ) * sizeof(float) + BM * sizeof(long);
    const long M = (long)d.NB * d.PH * d.PW;
    const int C = d.x.C0 + d.x.C1;
    const Magics mg = make_magics((unsigned)C, (unsigned)d.TW, (unsigned long)d.PW, (unsigned long)d.PH * d.PW,
                                  (unsigned long)M);
    const long mt = (M + BM - 1) / BM;
    const int nt = (d.Nstore + BN - 1) / BN;
    const long out_count = (long)d.NB * d.OH * d.OW * d.ldc;
    static unsigned long long attr_done = 0;
    {
        const int arc = ssc_set_max_lds(reinterpret_cast<const void*>(&conv_fwd_kernel<WM, WN, SM, SN, BMODE, VECB>), (int)lds, &attr_done);
        if (arc != 0) return arc;
    }
    dim3 grid((unsigned)mt, (unsigned)nt, (unsigned)(d.nphase * splitk));
    hipLaunchKernelGGL((conv_fwd_kernel<WM, WN, SM, SN, BMODE, VECB>), grid, dim3(256), lds, st, d, mg, ws,
                       out_count, splitk);
    if (splitk > 1) {
        launch_slab_reduce(ws, out_count, splitk, d, st);
    }
    return (int)hipGetLastError();
}

// set by ssc_conv_forward for the launch it is about to make: resident workgroups per CU of the chosen tile, workspace size
static thread_local int g_launch_res = 2;
static thread_local int64_t g_launch_ws_bytes = 0;
static thread_local long g_launch_ts_full = 0;      // the planner's tail split: whole tiles, slices per remaining tile
static thread_local int g_launch_ts_s = 1;
static int tail_split_mode() {
    static const int mode = ssc_dev_int("SSC_TAIL_SPLIT", 1);
    return mode;
}

// float4 filter loads need 16-byte aligned, fully in-range groups of 4
static bool fwd_is_vec(const ssc_conv_desc& d) {
    return (d.bmode == 0) ? (((d.wC1 | d.n_off) & 3) == 0 && (d.Nn & 3) == 0) : ((d.wC1 & 3) == 0 && (d.k_real & 3) == 0);
}

// uniform-tap fast path: every 32-wide K-tile inside one tap and one source, no channel padding
static bool fwd_is_ut(const ssc_conv_desc& d) {
    const bool vec = fwd_is_vec(d);
    const int C = d.x.C0 + d.x.C1;
    return vec && (C % BK) == 0 && (d.x.C0 % BK) == 0 && d.k_real == C &&
           (long)d.NB * d.x.H * d.x.W * (d.x.C0 > d.x.C1 ? d.x.C0 : d.x.C1) < 0x1fffffffL &&
           (long)d.KH * d.KW * d.wC0 * d.wC1 < 0x1fffffffL;
}

// row-tap form (conv_ut_kernel<KM = 2>): plain single-source view, TW * C == 32, unflipped taps, vector filter loads
static bool fwd_is_rowtap(const ssc_conv_desc& d) {
    return d.bmode == 0 && d.nphase == 1 && d.kstep == 1 && d.kx0 == 0 && d.x.C1 == 0 && d.TW * d.x.C0 == BK &&
           d.TW == d.KW && d.k_real == d.x.C0 && d.wC0 == d.x.C0 && fwd_is_vec(d) && d.x.ab0 == nullptr &&
           d.x.act == SSC_ACT_NONE && (long)d.NB * d.x.H * d.x.W * d.x.C0 < 0x1fffffffL &&
           (long)d.KH * d.KW * d.wC0 * d.wC1 < 0x1fffffffL;
}

// chunked uniform-tap form (conv_ut_kernel<KMASK>): vector filter loads possible and at most a third of the K-tiles' width
// wasted on the partly empty last chunk of each source (padded <= 1.5 x real)
static bool fwd_is_utg(const ssc_conv_desc& d) {
    const bool vec = fwd_is_vec(d);
    const int C = d.x.C0 + d.x.C1;
    const int padded = ((d.x.C0 + BK - 1) / BK + (d.x.C1 + BK - 1) / BK) * BK;
    // largest padded / real K width taken.  Measured 1.2 / 1.25 / 1.5: MRU train 258.9 / 257.8 / 256.9 ms, MRU forward 13.47 / - / 13.20 ms
    constexpr double waste = 1.5;
    // ... or no more K-tiles than the generic kernel's walk over taps * C would take (few channels: one chunk per tap either way)
    const long kt_chunks = (long)d.TH * d.TW * (padded / BK), kt_flat = ((long)d.TH * d.TW * C + BK - 1) / BK;
    return vec && d.k_real >= 1 && d.k_real <= C && ((double)padded <= waste * (double)C || kt_chunks <= kt_flat) &&
           (long)d.NB * d.x.H * d.x.W * (d.x.C0 > d.x.C1 ? d.x.C0 : d.x.C1) < 0x1fffffffL &&
           (long)d.KH * d.KW * d.wC0 * d.wC1 < 0x1fffffffL;
}

static int xcd_order() {
    static const int on = ssc_dev_int("SSC_XCD_ORDER", 2);      // 0: off, 1: XCD-aware order, 2: + the 4 phases of a row tile adjacent
    return on;
}

template <int WM, int WN, int SM, int SN, int BMODE, bool PLAIN, int KM>
static int launch_fwd_ut(const ssc_conv_desc& d, int splitk, float* ws, hipStream_t st) {
    constexpr int BM = WM * SM * 32, BN = WN * SN * 32;
    constexpr int A_SZ = BM * (UT_AV(BM, BN) ? BK + 4 : BK + 1);
    constexpr int B_SZ = BK * BN;
    constexpr size_t lds = 2 * (A_SZ + B_SZ) * sizeof(float) + BM * sizeof(long);
    const long M = (long)d.NB * d.PH * d.PW;
    const int C = d.x.C0 + d.x.C1;
    const int tpt = (KM == 2) ? 1 : (d.x.C0 + BK - 1) / BK + (d.x.C1 + BK - 1) / BK;   // K-tiles per tap (mg.mC divides by it)
    const Magics mg = make_magics((unsigned)tpt, (unsigned)d.TW, (unsigned long)d.PW, (unsigned long)d.PH * d.PW,
                                  (unsigned long)M);
    const long mt = (M + BM - 1) / BM;
    const int nt = (d.Nstore + BN - 1) / BN;
    const long out_count = (long)d.NB * d.OH * d.OW * d.ldc;
    static unsigned long long attr_done = 0;
    {
        const int arc = ssc_set_max_lds(reinterpret_cast<const void*>(&conv_ut_kernel<WM, WN, SM, SN, BMODE, PLAIN, KM>), (int)lds, &attr_done);
        if (arc != 0) return arc;
    }
    // whole tiles + K slices combined inside the launch, as the planner laid them out (plan_launch / cu_timeline)
    if (splitk == 1 && ws != nullptr && d.sk_flags != nullptr && g_launch_ts_s > 1) {
        const long tiles = mt * nt * d.nphase;
        const long full = g_launch_ts_full, tail = tiles - full, s = g_launch_ts_s;
        if (full >= 0 && tail > 0 && (int64_t)tail * s * BM * BN * 4 <= g_launch_ws_bytes && tail * s < SSC_SK_FLAG_WORDS - 1 &&
            full + tail * s < 0x7fffffffL) {
            hipLaunchKernelGGL((conv_ut_kernel<WM, WN, SM, SN, BMODE, PLAIN, KM>), dim3((unsigned)(full + tail * s)),
                               dim3(256), lds, st, d, mg, ws, out_count, 1, (int)full,
                               (int)s | ((xcd_order() && (full & 7) == 0) ? (0x10000 | ((xcd_order() >= 2 && d.nphase == 4) ? 0x20000 : 0)) : 0),
                               d.sk_flags);
            return (int)hipGetLastError();
        }
    }
    if (splitk == 1 && xcd_order()) {        // whole tiles only, 1-D grid in the XCD-aware order (no flags needed)
        const long tiles = mt * nt * d.nphase;
        const long full = tiles & ~7L;
        if (tiles < 0x7fffffffL && full > 0) {
            hipLaunchKernelGGL((conv_ut_kernel<WM, WN, SM, SN, BMODE, PLAIN, KM>), dim3((unsigned)tiles), dim3(256), lds, st, d,
                               mg, ws, out_count, 1, (int)full, 1 | 0x10000 | ((xcd_order() >= 2 && d.nphase == 4) ? 0x20000 : 0),
                               (unsigned*)nullptr);
            return (int)hipGetLastError();
        }
    }
    dim3 grid((unsigned)mt, (unsigned)nt, (unsigned)(d.nphase * splitk));
    hipLaunchKernelGGL((conv_ut_kernel<WM, WN, SM, SN, BMODE, PLAIN, KM>), grid, dim3(256), lds, st, d, mg, ws, out_count,
                       splitk, 0, 0, (unsigned*)nullptr);
    if (splitk > 1) {
        launch_slab_reduce(ws, out_count, splitk, d, st);
    }
    return (int)hipGetLastError();
}

template <int WM, int WN, int SM, int SN, int BMODE>
static int launch_fwd(const ssc_conv_desc& d, int splitk, float* ws, hipStream_t st) {
    const bool vec = fwd_is_vec(d);
    const bool ut = fwd_is_ut(d);
    if (ut || fwd_is_utg(d)) {
        const bool plain0 = d.x.ab0 == nullptr && d.x.act == SSC_ACT_NONE;
        const bool plain1 = d.x.C1 == 0 || (d.x.ab1 == nullptr && (d.x.act1 >= 0 ? d.x.act1 : d.x.act) == SSC_ACT_NONE);
        const bool plain = plain0 && plain1;
        if (ut) return plain ? launch_fwd_ut<WM, WN, SM, SN, BMODE, true, 0>(d, splitk, ws, st)
                             : launch_fwd_ut<WM, WN, SM, SN, BMODE, false, 0>(d, splitk, ws, st);
        return plain ? launch_fwd_ut<WM, WN, SM, SN, BMODE, true, 1>(d, splitk, ws, st)
                     : launch_fwd_ut<WM, WN, SM, SN, BMODE, false, 1>(d, splitk, ws, st);
    }
    if (BMODE == 0 && fwd_is_rowtap(d)) {       // a filter row per K-tile: run as TH taps of 32 "channels"
        ssc_conv_desc dr = d;
        dr.TW = 1;
        return launch_fwd_ut<WM, WN, SM, SN, 0, true, 2>(dr, splitk, ws, st);
    }
    return vec ? launch_fwd_v<WM, WN, SM, SN, BMODE, true>(d, splitk, ws, st)
               : launch_fwd_v<WM, WN, SM, SN, BMODE, false>(d, splitk, ws, st);
}

// bf16-split form (igemm_bf16.hip): the caller supplied the filter's planes, every K-tile lies inside one tap and one source,
// the column range starts at a 32-column block.  SSC_ARITH=fp32 keeps everything on the exact-fp32 MFMA.
static bool fwd_is_bf(const ssc_conv_desc& d) {
    // ... or ONE source whose channel count is any multiple of 4 above 32 (MRU's materialised concats: state + image channels),
    // the partly empty last chunk of every tap masked in the staging (conv_bf_kernel<KM>); the planes pad k >= K with zeros
    const bool km = d.x.C1 == 0 && (d.x.C0 & 3) == 0 && d.x.C0 > BK && (d.x.C0 % BK) != 0 && d.k_real >= 1 && d.k_real <= d.x.C0 &&
                    d.ws_kc == 2 * ((d.x.C0 + BK - 1) / BK) && (long)d.NB * d.x.H * d.x.W * d.x.C0 < 0x1fffffffL &&
                    (long)d.KH * d.KW * d.wC0 * d.wC1 < 0x1fffffffL;
    return !ssc_arith_fp32() && d.wsplit != nullptr && d.ws_kc > 0 && d.ws_nbp > 0 && (fwd_is_ut(d) || km) && (d.n_off & 31) == 0 && d.Nstore > 32 &&
           d.TH * d.TW <= 32;
}

static Plan plan_fwd(const ssc_conv_desc& d, int64_t ws_bytes, bool have_ws) {
    const long M = (long)d.NB * d.PH * d.PW;
    const int C = d.x.C0 + d.x.C1;
    long nkt = ((long)d.TH * d.TW * C + BK - 1) / BK;
    if (fwd_is_ut(d) || fwd_is_utg(d))       // conv_ut_kernel walks whole chunks per tap and source
        nkt = (long)d.TH * d.TW * ((d.x.C0 + BK - 1) / BK + (d.x.C1 + BK - 1) / BK);
    else if (d.bmode == 0 && fwd_is_rowtap(d))
        nkt = d.TH;
    // column tile no wider than needed: <=32 -> 128x32, <=64 -> 128x64, else 128x128 / 64x128 / 128x64
    const bool allowed[5] = {d.Nstore > 64, d.Nstore > 64, d.Nstore > 32, d.Nstore <= 32, d.Nstore > 32};
    const bool can_ts = d.sk_flags != nullptr && tail_split_mode() != 0 &&
                        (fwd_is_ut(d) || fwd_is_utg(d) || (d.bmode == 0 && fwd_is_rowtap(d)));
    if (fwd_is_bf(d)) {
        const bool allowed_bf[5] = {d.Nstore > 64, d.Nstore > 64, true, false, true};
        // six bf16 passes = 6/16 of the fp32 MFMA's cycles; the staging beside them and the shorter K steps make it ~0.45
        constexpr double BF_SCALE = 0.45;
        static const double hk_min = ssc_dev_double("SSC_PLAN_BF_HK_MIN", 0.5), hk_penalty = ssc_dev_double("SSC_PLAN_BF_HK", 0.78);
        // 128 x 128 on 16-k stages (round 6): two workgroups per CU, measured 3-10 % ahead of 64 x 128 on launches of whole
        // rounds (d4 +9.5 %, dec3 +6.5 %, enc2 +6 %); the uniform form only (the partial-chunk launches keep the 32-k kernel)
        TileCfg cfgs[5];
        for (int i = 0; i < 5; ++i) cfgs[i] = BF_CFGS[i];
        // (Also for launches that share the chip with other streams' -- lds_hint, the Pix2Pix train step -- although the 42 KB
        // one-stage 64 x 128 form is what lets three workgroups of different chains share a CU: 13.13 / 12.91 vs 13.00 / 13.05 ms
        // per step, equal.  The tile choice must not depend on the hint: it changes the summation order, and a trainer that
        // overlaps its chains must stay bit-identical with one that does not.)
        if (ssc_bf_hk_enabled()) {
            // ... for launches of at least SSC_PLAN_BF_HK_MIN x (2 x CUs) such tiles (below that the 64 x 128 tile's twice as many
            // workgroups balance better).  Swept over 0 / 0.5 / 1 / 2 / never (scripts/hk_min_sweep.sh, same box, twice): generator
            // inference at batch 16 1.325 / 1.300 / 1.300 / 1.308 / 1.293 ms, Background train step 22.3 / 21.8 / 22.1 / 22.1 / 22.0,
            // Pix2Pix train step 12.35 / 12.38 / 12.54 / 12.84 / 12.90, MRU 183.9 / 183.6 / 182.9 / 184.0 / 190.2
            const long t128 = ((M + 127) / 128) * ((d.Nstore + 127) / 128) * d.nphase;
            if ((double)t128 < hk_min * 2.0 * num_cu()) {
                return plan_launch(cfgs, 5, allowed_bf, M, d.Nstore, d.nphase, nkt, (long)d.NB * d.OH * d.OW * d.ldc, ws_bytes,
                                   have_ws, can_ts, BF_SCALE);
            }
            cfgs[0].res = 2;
            // 0.78: swept on the train steps (scripts/hk_plan_sweep.sh): Pix2Pix 12.57 -> 12.2 ms between 0.86 and 0.78 (the tile then
            // takes most whole-round launches), MRU / Residual / Background flat from 0.62 to 0.86
            cfgs[0].penalty = hk_penalty;
            // the partial-chunk form walks ceil(C / 16) chunks of 16 per tap there, 2 * ceil(C / 32) on the 32-k tiles
            if (!fwd_is_ut(d)) cfgs[0].penalty *= (double)((d.x.C0 + 15) / 16) / (double)(2 * ((d.x.C0 + 31) / 32));
        }
        return plan_launch(cfgs, 5, allowed_bf, M, d.Nstore, d.nphase, nkt, (long)d.NB * d.OH * d.OW * d.ldc, ws_bytes,
                           have_ws, can_ts, BF_SCALE);
    }
    return plan_launch(FWD_CFGS, 5, allowed, M, d.Nstore, d.nphase, nkt, (long)d.NB * d.OH * d.OW * d.ldc, ws_bytes,
                       have_ws, can_ts);
}

static void copy_name(const char* src, char* dst, int len) {
    int i = 0;
    for (; i < len - 1 && src[i]; ++i) dst[i] = src[i];
    if (len > 0) dst[i] = 0;
}

// ---- the kernels in front of the tiled ones, in dispatch order: the launch, the name and plan queries and
// the riders all ask this table ----
enum { FWD_TILED = 0, FWD_HEAD1, FWD_HEAD1_DGRAD, FWD_NARROW, FWD_FEWCHAN, FWD_PW1X1, FWD_C3X3, FWD_S2N16, FWD_TR4_TINY, FWD_FEWCHAN7,
       FWD_TR4N16 };
constexpr unsigned R_BN = 1u << SSC_RIDER_BN, R_BNBWD = 1u << SSC_RIDER_BNBWD, R_ALL = 15u;
struct FwdKernel {
    int id;
    int (*supported)(const ssc_conv_desc*);
    const char* (*name)(const ssc_conv_desc&);
    int (*rows)(const ssc_conv_desc*);      // rows of partial sums a launch with a rider writes (one per walker or block)
    unsigned carries;                       // riders (1 << SSC_RIDER_*) the kernel takes on its own epilogue
    unsigned blind;                         // riders whose fields the predicate does not look at: they keep away from the kernel
};                                          // every other rider's fields the predicate refuses
static const FwdKernel FWD_EARLY[] = {
    // the one-output patch head over a 512-channel tensor and its data gradient (head1.hip): streaming kernels
    {FWD_HEAD1, ssc_head1_forward_supported, [](const ssc_conv_desc&) { return "head1_fwd"; }, nullptr, 0, 0},
    {FWD_HEAD1_DGRAD, ssc_head1_dgrad_supported, [](const ssc_conv_desc&) { return "head1_dgrad"; }, nullptr, 0, 0},
    // <= 4 output channels
    {FWD_NARROW, ssc_conv_narrow_supported,
     [](const ssc_conv_desc& d) { return d.nphase == 4 ? "narrow_fwd<transposed>" : "narrow_fwd<conv>"; }, nullptr, 0, R_ALL},
    // 4x4 stride-2 over 4 or 8 input channels
    {FWD_FEWCHAN, ssc_conv_fewchan_supported,
     [](const ssc_conv_desc& d) { return d.x.C0 == 8 ? "conv_fewchan<8>" : "conv_fewchan<4>"; }, nullptr, 0, R_ALL},
    // 1x1 expansion of a bottleneck: K <= 128, streaming kernel
    {FWD_PW1X1, ssc_conv_pw1x1_supported, [](const ssc_conv_desc&) { return "conv_pw1x1"; }, ssc_conv_pw1x1_walkers, R_BN, 0},
    // 3x3 of a bottleneck at 16 / 32 channels (either filter orientation)
    {FWD_C3X3, ssc_conv_c3x3_supported, [](const ssc_conv_desc& d) { return d.bmode ? "conv_c3x3<NK>" : "conv_c3x3<KN>"; },
     ssc_conv_c3x3_walkers, R_BN | R_BNBWD, 0},
    // 4x4 stride-2 conv 64 -> <= 16 channels: 16-column MFMA, K split over the waves
    {FWD_S2N16, ssc_conv_s2n16_supported, [](const ssc_conv_desc&) { return "conv_s2n16"; }, ssc_conv_s2n16_walkers, R_BN | R_BNBWD, 0},
    // k = 4 stride-2 transposed conv, <= 4 channels in and out: a thread per lattice pixel
    {FWD_TR4_TINY, ssc_conv_tr4_tiny_supported, [](const ssc_conv_desc&) { return "deconv_tr4_tiny"; }, ssc_conv_tr4_tiny_blocks, R_BN, 0},
    // 7x7 stride-2 conv over the (padded) image channels
    {FWD_FEWCHAN7, ssc_conv_fewchan7_supported, [](const ssc_conv_desc&) { return "conv_fewchan7"; }, ssc_conv_fewchan7_walkers, R_BN, 0},
    // k = 4 stride-2 transposed conv 256 -> <= 16 channels: 16-column MFMA, a phase per workgroup
    {FWD_TR4N16, ssc_conv_tr4n16_supported, [](const ssc_conv_desc&) { return "deconv_tr4n16"; }, ssc_conv_tr4n16_rows, R_BN, 0}};
static_assert(sizeof(FWD_EARLY) / sizeof(FWD_EARLY[0]) == FWD_TR4N16, "one row per FWD_* id, in the enum's order");
// the first kernel of the table that takes the launch.  under_riders: with the fields of these riders set, which the rows that
// neither carry nor overlook them refuse
static int fwd_early_kernel(const ssc_conv_desc* dp, bool have_ws, int64_t ws_bytes, unsigned under_riders = 0) {
    for (const FwdKernel& k : FWD_EARLY) {
        if ((under_riders & ~(k.carries | k.blind)) != 0 || !k.supported(dp)) continue;
        // head1 forward keeps 16 dot products per input pixel in the workspace
        if (k.id == FWD_HEAD1 && !(have_ws && (int64_t)dp->NB * dp->x.H * dp->x.W * 16 * 4 <= ws_bytes)) continue;
        return k.id;
    }
    return FWD_TILED;
}

extern "C" int ssc_conv_forward_kernel_name(const ssc_conv_desc* dp, char* buf, int len) {
    const int early = fwd_early_kernel(dp, true, (int64_t)1 << 40);       // the ample workspace the plan below assumes too
    if (early != FWD_TILED) {
        copy_name(FWD_EARLY[early - 1].name(*dp), buf, len);
        return 0;
    }
    static const char* names[2][5] = {
        {"conv_fwd<128x128,KN>", "conv_fwd<64x128,KN>", "conv_fwd<128x64,KN>", "conv_fwd<128x32,KN>", "conv_fwd<64x64,KN>"},
        {"conv_fwd<128x128,NK>", "conv_fwd<64x128,NK>", "conv_fwd<128x64,NK>", "conv_fwd<128x32,NK>", "conv_fwd<64x64,NK>"}};
    const Plan p = plan_fwd(*dp, (int64_t)1 << 40, true);
    if (fwd_is_bf(*dp)) {
        static const char* bfn[5] = {"conv_bf16x6<128x128>", "conv_bf16x6<64x128>", "conv_bf16x6<128x64>", "conv_bf16x6<128x32>",
                                     "conv_bf16x6<64x64>"};
        copy_name(bfn[p.cfg < 0 ? 0 : p.cfg], buf, len);
        return 0;
    }
    copy_name(names[dp->bmode ? 1 : 0][p.cfg < 0 ? 0 : p.cfg], buf, len);
    return 0;
}

// elementwise.hip
extern "C" int ssc_bn_stats(const float* x, int64_t M, int C, int ldx, const float* scale, const float* offset, float eps,
                            float* ab, float* stats, float* ws, int64_t ws_bytes, void* stream);
extern "C" int ssc_bn_finalize(const float* partial, int nblk, int C, int64_t M, const float* scale, const float* offset,
                               float eps, float* ab, float* stats, void* stream);
// mru_ops.hip
extern "C" int ssc_minmax_hw(const float* x, int ld, int N, int P, int C, float* mnmx, float* workspace, int64_t workspace_bytes,
                             void* stream);
extern "C" int ssc_minmax_finalize(const float* part, int nsplit, int N, int C, float* mnmx, void* stream);

// ---- riders: a reduction over the output that a launch takes along (ssc_conv_forward_bn, _bnbwd, _bnbwd2, _minmax).  One
// decision, rider_decide, for the four entry points and for ssc_conv_rider_plan ----
static int fwd_launch(int early, const ssc_conv_desc* dp, float* ws, int64_t ws_bytes, void* stream);
static int fwd_desc_error(const ssc_conv_desc& d);

// what the tile epilogue needs of a launch before it carries a rider, beyond the uniform-tap form, whole 16-byte aligned
// rows (Nstore == ldc), no accumulation and a plan without split-K
struct RiderReq {
    bool rowtap;        // the row-tap form will do as well
    bool epi2;          // the lrelu epilogue (epi 2) beside none
    bool bias;          // a bias
    bool all_real;      // Nn == Nstore required
    bool whole_tiles;   // nphase == 1 and a sample's positions whole row tiles (P % BM == 0)
    bool bn128;         // column tile of at most 128
    bool caller_rows;   // the rows go to the caller's buffers (else to the end of the workspace)
    bool round256;      // the workspace tail is reserved in multiples of 256 bytes
};
static const RiderReq RIDER_REQ[4] = {
    /* SSC_RIDER_BN     */ {true, false, true, false, false, false, false, true},
    /* SSC_RIDER_BNBWD  */ {true, false, false, true, false, false, true, false},
    /* SSC_RIDER_BNBWD2 */ {false, false, false, true, false, true, true, false},
    /* SSC_RIDER_MINMAX */ {false, true, true, true, true, false, false, false}};

// the norm-backward sites of a launch: all there (and the column split a legal one), rows of x addressable by float4, columns
// and capacity in bytes of either site's rows.  The riders without sites: {true, true}
struct RiderSites {
    bool present, aligned;
    int cols[2];
    int64_t cap[2];
};
static RiderSites rider_sites(const ssc_conv_desc& d, int rider, const ssc_bnbwd_site* s0, const ssc_bnbwd_site* s1, int C0) {
    auto there = [](const ssc_bnbwd_site* s) { return s != nullptr && s->x && s->ab && s->stats && s->partial; };
    auto al = [](const ssc_bnbwd_site* s) { return (s->ldx & 3) == 0 && (reinterpret_cast<unsigned long>(s->x) & 15) == 0; };
    if (rider == SSC_RIDER_BNBWD) {
        if (!there(s0)) return {false, false, {0, 0}, {0, 0}};
        return {true, al(s0), {d.Nstore, 0}, {s0->partial_bytes, 0}};
    }
    if (rider == SSC_RIDER_BNBWD2) {
        const int C1 = d.Nstore - C0;
        if (!there(s0) || !there(s1) || C0 <= 0 || C1 <= 0 || (C0 % 128) != 0 || (C1 & 3) != 0) return {false, false, {0, 0}, {0, 0}};
        return {true, al(s0) && al(s1), {C0, C1}, {s0->partial_bytes, s1->partial_bytes}};
    }
    return {true, true, {0, 0}, {0, 0}};
}

static bool tile_epilogue_ok(const ssc_conv_desc& d, const RiderReq& q) {
    return (d.epi == 0 || (q.epi2 && d.epi == 2)) && !d.accumulate && (q.bias || d.bias == nullptr) && d.Nstore == d.ldc &&
           (!q.all_real || d.Nn == d.Nstore) && (d.Nstore & 3) == 0 && (reinterpret_cast<unsigned long>(d.out) & 15) == 0 &&
           (!q.whole_tiles || d.nphase == 1) && (fwd_is_ut(d) || fwd_is_utg(d) || (q.rowtap && d.bmode == 0 && fwd_is_rowtap(d)));
}

struct RiderPlan {
    int path, kernel, rows, home;       // SSC_RIDER_PATH_*, FWD_*, rows of partial results, SSC_RIDER_ROWS_*
    int64_t ws_conv;                    // workspace bytes left to the conv
};
// d: the launch with no rider field set.  Pure: the entry points and the query get the same answer.
static RiderPlan rider_decide(const ssc_conv_desc& d, int rider, bool have_ws, int64_t ws_bytes, const RiderSites& s) {
    const RiderReq& q = RIDER_REQ[rider];
    const int k = fwd_early_kernel(&d, have_ws, ws_bytes);
    const RiderPlan plain = {SSC_RIDER_PATH_PLAIN, k, 0, SSC_RIDER_ROWS_NONE, ws_bytes};
    auto caller_fits = [&](long rows) {
        return (int64_t)rows * 2 * s.cols[0] * 4 <= s.cap[0] && (int64_t)rows * 2 * s.cols[1] * 4 <= s.cap[1];
    };
    // the kernel once the rider's fields are set: rows of the table that refuse them stand aside
    const int under = fwd_early_kernel(&d, have_ws, ws_bytes, 1u << rider);
    if (under != FWD_TILED) {
        const FwdKernel& e = FWD_EARLY[under - 1];
        if (under != k || !(e.carries & (1u << rider)) || d.Nstore != d.ldc || !s.present) return plain;
        // a streaming kernel: per-lane sums over the tiles a workgroup walks, one row per walker
        const int rows = e.rows(&d);
        if (q.caller_rows ? caller_fits(rows) : have_ws && (int64_t)rows * 2 * d.Nstore * 4 <= ws_bytes)
            return {SSC_RIDER_PATH_STREAM, k, rows, q.caller_rows ? SSC_RIDER_ROWS_CALLER : SSC_RIDER_ROWS_WS_HEAD, ws_bytes};
        return plain;
    }
    // the tiles.  Split-K launches (few rows, long K: encoder_5, the bottlenecks' convs at the low resolutions) take batch
    // statistics in the slab sum instead (slab_reduce4_stats_kernel)
    const bool tile_ok = s.present && s.aligned && tile_epilogue_ok(d, q);
    const bool slab_ok = rider == SSC_RIDER_BN && k == FWD_TILED && slab_stats_ok(d);
    if (!have_ws || !(tile_ok || slab_ok)) return plain;
    const Plan p = plan_fwd(d, ws_bytes, true);
    if (p.cfg < 0 || !(p.splitk == 1 ? tile_ok : slab_ok && p.ts_s <= 1)) return plain;
    const long P = (long)d.PH * d.PW, M = (long)d.NB * P;
    const TileCfg& t = FWD_CFGS[p.cfg];
    if (p.splitk == 1 && ((q.whole_tiles && (P % t.BM) != 0) || (q.bn128 && t.BN > 128))) return plain;
    const long rows = p.splitk == 1 ? (M + t.BM - 1) / t.BM * d.nphase : slab_stats_blocks(M * d.nphase, d.ldc);
    if (q.caller_rows)
        return caller_fits(rows) ? RiderPlan{SSC_RIDER_PATH_TILE, FWD_TILED, (int)rows, SSC_RIDER_ROWS_CALLER, ws_bytes} : plain;
    // the rows sit at the end of the workspace and the conv plans again with the rest: it must keep its tile and its split
    // (the two fit rules are the riders' own: unifying them would change which launches fuse)
    const int64_t need = (int64_t)rows * 2 * d.Nstore * 4;
    const int64_t reserve = (q.round256 || p.splitk > 1) ? (need + 255) & ~(int64_t)255 : need;
    if (p.splitk == 1 && reserve * 4 > ws_bytes) return plain;
    const int64_t ws_conv = (ws_bytes - reserve) & ~(int64_t)255;
    const Plan p2 = plan_fwd(d, ws_conv, true);
    if (p2.cfg != p.cfg || p2.splitk != p.splitk || (p.splitk > 1 && (ws_conv <= 0 || p2.ts_s > 1))) return plain;
    return {p.splitk == 1 ? SSC_RIDER_PATH_TILE : SSC_RIDER_PATH_SLAB, FWD_TILED, (int)rows, SSC_RIDER_ROWS_WS_TAIL, ws_conv};
}

// the launch's own copy with the rider fields clear (callers leave them so; a stale one must not reach a kernel)
static ssc_conv_desc rider_clean(const ssc_conv_desc* dp) {
    ssc_conv_desc d = *dp;
    d.stat_partial = nullptr;
    d.sb_x = nullptr;
    d.sb2_x = nullptr;
    d.stat_mode = 0;
    return d;
}
static float* rider_ws_rows(const RiderPlan& r, float* ws) {
    if (r.home == SSC_RIDER_ROWS_WS_HEAD) return ws;
    return r.home == SSC_RIDER_ROWS_WS_TAIL ? reinterpret_cast<float*>(reinterpret_cast<char*>(ws) + r.ws_conv) : nullptr;
}

extern "C" int ssc_conv_rider_plan(const ssc_conv_desc* dp, int rider, int64_t ws_bytes, const ssc_bnbwd_site* site0,
                                   const ssc_bnbwd_site* site1, int C0, int64_t* out5) {
    if (rider < SSC_RIDER_BN || rider > SSC_RIDER_MINMAX) return -1;
    const ssc_conv_desc d = rider_clean(dp);
    const int err = fwd_desc_error(d);
    if (err != 0) return err;
    const RiderPlan r = rider_decide(d, rider, ws_bytes > 0, ws_bytes, rider_sites(d, rider, site0, site1, C0));
    out5[0] = r.path; out5[1] = r.kernel; out5[2] = r.rows; out5[3] = r.home; out5[4] = r.ws_conv;
    return 0;
}

// conv + batch-statistics norm fold of its output: the per-column sums out of the launch where rider_decide finds a way,
// otherwise the output is read back once
extern "C" int ssc_conv_forward_bn(const ssc_conv_desc* dp, float* ws, int64_t ws_bytes, const float* scale,
                                   const float* offset, float eps, float* ab, float* stats, void* stream) {
    ssc_conv_desc d = rider_clean(dp);
    const RiderPlan r = rider_decide(d, SSC_RIDER_BN, ws != nullptr, ws_bytes, rider_sites(d, SSC_RIDER_BN, nullptr, nullptr, 0));
    const long Mall = (long)d.NB * d.PH * d.PW * d.nphase;
    d.stat_partial = rider_ws_rows(r, ws);
    const int rc = fwd_launch(r.kernel, &d, ws, r.ws_conv, stream);
    if (rc != 0) return rc;
    if (r.path == SSC_RIDER_PATH_PLAIN)
        return ssc_bn_stats(d.out, Mall, d.Nstore, d.ldc, scale, offset, eps, ab, stats, ws, ws_bytes, stream);
    return ssc_bn_finalize(d.stat_partial, r.rows, d.Nstore, Mall, scale, offset, eps, ab, stats, stream);
}

static void rider_fill_site(ssc_conv_desc& d, const ssc_bnbwd_site& s) {
    d.stat_partial = s.partial;
    d.sb_x = s.x; d.sb_ldx = s.ldx; d.sb_ab = s.ab; d.sb_stats = s.stats; d.sb_act = s.act;
}

// conv whose output g is the gradient w.r.t. act(a*x+b) of a batch-statistics-normed tensor x ([rows][ldx], laid out like
// the output): the two per-channel sums of the norm's backward come out of the launch as rows of `partial` ([rows][2][Nstore])
// and *nrows is their count; or *nrows = 0 and the caller takes the sums with the separate pass (ssc_bn_act_backward).
extern "C" int ssc_conv_forward_bnbwd(const ssc_conv_desc* dp, float* ws, int64_t ws_bytes, const float* x, int ldx,
                                      const float* ab, const float* stats, int act, float* partial, int64_t partial_bytes,
                                      int* nrows, void* stream) {
    ssc_conv_desc d = rider_clean(dp);
    const ssc_bnbwd_site s = {x, ab, stats, partial, partial_bytes, ldx, act};
    const RiderPlan r = rider_decide(d, SSC_RIDER_BNBWD, ws != nullptr, ws_bytes, rider_sites(d, SSC_RIDER_BNBWD, &s, nullptr, 0));
    if (r.path != SSC_RIDER_PATH_PLAIN) rider_fill_site(d, s);
    *nrows = r.rows;
    return fwd_launch(r.kernel, &d, ws, r.ws_conv, stream);
}

// conv (+ bias + lrelu) whose output's per-sample, per-channel extrema are wanted (the MRU gates): the per-tile minima / maxima
// out of the epilogue where no tile straddles two samples
extern "C" int ssc_conv_forward_minmax(const ssc_conv_desc* dp, float* ws, int64_t ws_bytes, float* mnmx, void* stream) {
    ssc_conv_desc d = rider_clean(dp);
    const RiderPlan r = rider_decide(d, SSC_RIDER_MINMAX, ws != nullptr, ws_bytes, rider_sites(d, SSC_RIDER_MINMAX, nullptr, nullptr, 0));
    d.stat_partial = rider_ws_rows(r, ws);
    d.stat_mode = r.path == SSC_RIDER_PATH_TILE ? 1 : 0;
    const int rc = fwd_launch(r.kernel, &d, ws, r.ws_conv, stream);
    if (rc != 0) return rc;
    if (r.path == SSC_RIDER_PATH_TILE) return ssc_minmax_finalize(d.stat_partial, r.rows / d.NB, d.NB, d.Nstore, mnmx, stream);
    return ssc_minmax_hw(d.out, d.ldc, d.NB, d.PH * d.PW, d.Nstore, mnmx, ws, ws_bytes, stream);
}

extern "C" int ssc_conv_forward_bnbwd2(const ssc_conv_desc* dp, float* ws, int64_t ws_bytes, const ssc_bnbwd_site* s0,
                                       const ssc_bnbwd_site* s1, int C0, int* nrows, void* stream) {
    ssc_conv_desc d = rider_clean(dp);
    const RiderPlan r = rider_decide(d, SSC_RIDER_BNBWD2, ws != nullptr, ws_bytes, rider_sites(d, SSC_RIDER_BNBWD2, s0, s1, C0));
    if (r.path != SSC_RIDER_PATH_PLAIN) {
        rider_fill_site(d, *s0);
        d.stat_partial2 = s1->partial; d.sb2_col0 = C0;
        d.sb2_x = s1->x; d.sb2_ldx = s1->ldx; d.sb2_ab = s1->ab; d.sb2_stats = s1->stats; d.sb2_act = s1->act;
    }
    *nrows = r.rows;
    return fwd_launch(r.kernel, &d, ws, r.ws_conv, stream);
}

extern "C" int ssc_sk_configure(int timeout_ms, int test_withhold) {
    const unsigned long long ticks = (unsigned long long)(timeout_ms > 0 ? timeout_ms : 20000) * 100000ull;     // 100 MHz
    const unsigned cfg[4] = {(unsigned)(ticks & 0xffffffffu), (unsigned)(ticks >> 32), test_withhold ? 1u : 0u, 0u};
    const int rc = ssc_sk_configure_bf(cfg);
    if (rc != 0) return rc;
    return (int)hipMemcpyToSymbol(HIP_SYMBOL(g_sk_cfg), cfg, sizeof(cfg), 0, hipMemcpyHostToDevice);
}

extern "C" int ssc_conv_forward_plan(const ssc_conv_desc* dp, int64_t ws_bytes, int* out5) {
    // host only: {tile configuration, split-K slabs, whole tiles, K slices per remaining tile, modelled cycles / 1000}
    if (ssc_conv_narrow_supported(dp) || ssc_conv_fewchan_supported(dp)) {
        out5[0] = -1; out5[1] = 1; out5[2] = 0; out5[3] = 1; out5[4] = 0;
        return 0;
    }
    const Plan p = plan_fwd(*dp, ws_bytes, true);
    out5[0] = p.cfg; out5[1] = p.splitk; out5[2] = (int)p.ts_full; out5[3] = p.ts_s; out5[4] = (int)(p.cost / 1000.0);
    return 0;
}

// ---- what ssc_conv_forward does with a descriptor: the launch itself and ssc_conv_bf_plan both ask these ----
static int fwd_desc_error(const ssc_conv_desc& d) {
    if ((d.x.C0 & 3) || (d.x.C1 & 3) || d.Nstore < d.Nn || d.Nstore > d.ldc) return -1;
    if (d.nphase != 1 && d.nphase != 4) return -2;
    if (d.nphase == 4 && (d.TH != 2 || d.TW != 2 || d.KH != 4 || d.KW != 4 || d.kstep != -2 || d.out_stride != 2 ||
                          d.in_stride != 1))
        return -3;
    return 0;
}
static bool fwd_bf_plain(const ssc_conv_desc& d) {
    const bool plain0 = d.x.ab0 == nullptr && d.x.act == SSC_ACT_NONE;
    const bool plain1 = d.x.C1 == 0 || (d.x.ab1 == nullptr && (d.x.act1 >= 0 ? d.x.act1 : d.x.act) == SSC_ACT_NONE);
    return plain0 && plain1;
}

extern "C" int ssc_conv_bf_plan(const ssc_conv_desc* dp, int64_t ws_bytes, int* out10) {
    // host only: {kernel, tile, PLAIN, source form, SS, korder, grid layout, split-K slabs, whole tiles, K slices per remaining
    // tile}; ws_bytes <= 0 stands for a NULL workspace
    const ssc_conv_desc& d = *dp;
    const bool have_ws = ws_bytes > 0;
    const int err = fwd_desc_error(d);
    if (err != 0) return err;
    if (fwd_early_kernel(dp, have_ws, ws_bytes) != FWD_TILED || !fwd_is_bf(d)) return -10;
    const Plan p = plan_fwd(d, ws_bytes, have_ws);
    if (p.cfg < 0) return -4;
    return ssc_conv_bf_form(p.cfg, fwd_bf_plain(d), d, p.splitk, have_ws, p.ts_full, p.ts_s, ws_bytes, xcd_order(), out10);
}

extern "C" int ssc_conv_stream_plan(const ssc_conv_desc* dp, int* out4) {
    // host only: {kernel (FWD_*), instantiation, tiles, workgroups} of a launch one of the seven streaming kernels takes
    const int err = fwd_desc_error(*dp);
    if (err != 0) return err;
    ssc_stream_plan p;
    const int k = fwd_early_kernel(dp, true, (int64_t)1 << 40);
    switch (k) {
        case FWD_FEWCHAN: p = ssc_conv_fewchan_plan(dp, num_cu()); break;
        case FWD_PW1X1: p = ssc_conv_pw1x1_plan(dp); break;
        case FWD_C3X3: p = ssc_conv_c3x3_plan(dp); break;
        case FWD_S2N16: p = ssc_conv_s2n16_plan(dp); break;
        case FWD_TR4_TINY: p = ssc_conv_tr4_tiny_plan(dp); break;
        case FWD_FEWCHAN7: p = ssc_conv_fewchan7_plan(dp); break;
        case FWD_TR4N16: p = ssc_conv_tr4n16_plan(dp); break;
        default: return -10;
    }
    out4[0] = k; out4[1] = p.inst; out4[2] = p.tiles; out4[3] = p.grid_x * p.grid_y;
    return 0;
}

extern "C" int ssc_conv_forward(const ssc_conv_desc* dp, float* ws, int64_t ws_bytes, void* stream) {
    return fwd_launch(fwd_early_kernel(dp, ws != nullptr, ws_bytes), dp, ws, ws_bytes, stream);
}

// the launch on the kernel the route chose (FWD_*)
static int fwd_launch(int early, const ssc_conv_desc* dp, float* ws, int64_t ws_bytes, void* stream) {
    const ssc_conv_desc& d = *dp;
    hipStream_t st = (hipStream_t)stream;
    const int err = fwd_desc_error(d);
    if (err != 0) return err;
    switch (early) {
        case FWD_HEAD1: return ssc_head1_forward(dp, ws, ws_bytes, stream);
        case FWD_HEAD1_DGRAD: return ssc_head1_dgrad(dp, stream);
        case FWD_NARROW: {
            int csplit = 1;
            const int rc = ssc_conv_narrow_forward_ws(dp, ws, ws_bytes, stream, &csplit);
            if (rc != 0 || csplit == 1) return rc;
            const long out_count = (long)d.NB * d.OH * d.OW * d.ldc;
            hipLaunchKernelGGL(slab_reduce_kernel, dim3((unsigned)((out_count + 255) / 256)), dim3(256), 0, st, ws, out_count,
                               csplit, d.out, out_count, d.ldc, d.Nn, d.Nstore, d.bias, d.epi, d.accumulate);
            return (int)hipGetLastError();
        }
        case FWD_FEWCHAN: return ssc_conv_fewchan_forward(dp, num_cu(), stream);
        case FWD_PW1X1: return ssc_conv_pw1x1_forward(dp, d.stat_partial, stream);
        case FWD_C3X3: return ssc_conv_c3x3_forward(dp, d.stat_partial, stream);
        case FWD_S2N16: return ssc_conv_s2n16_forward(dp, d.stat_partial, stream);
        case FWD_TR4_TINY: return ssc_conv_tr4_tiny_forward(dp, d.stat_partial, stream);
        case FWD_FEWCHAN7: return ssc_conv_fewchan7_forward(dp, d.stat_partial, stream);
        case FWD_TR4N16: return ssc_conv_tr4n16_forward(dp, d.stat_partial, stream);
        default: break;
    }
    const Plan p = plan_fwd(d, ws_bytes, ws != nullptr);
    if (p.cfg < 0) return -4;
    if (fwd_is_bf(d)) return ssc_launch_conv_bf(p.cfg, fwd_bf_plain(d), d, p.splitk, ws, st, p.ts_full, p.ts_s, ws_bytes, xcd_order());
    g_launch_res = FWD_CFGS[p.cfg].res;
    g_launch_ws_bytes = ws_bytes;
    g_launch_ts_full = p.ts_full;
    g_launch_ts_s = p.ts_s;
    if (d.bmode == 0) {
        switch (p.cfg) {
            case 0: return launch_fwd<2, 2, 2, 2, 0>(d, p.splitk, ws, st);
            case 1: return launch_fwd<2, 2, 1, 2, 0>(d, p.splitk, ws, st);
            case 2: return launch_fwd<2, 2, 2, 1, 0>(d, p.splitk, ws, st);
            case 4: return launch_fwd<2, 2, 1, 1, 0>(d, p.splitk, ws, st);
            default: return launch_fwd<4, 1, 1, 1, 0>(d, p.splitk, ws, st);
        }
    } else {
        switch (p.cfg) {
            case 0: return launch_fwd<2, 2, 2, 2, 1>(d, p.splitk, ws, st);
            case 1: return launch_fwd<2, 2, 1, 2, 1>(d, p.splitk, ws, st);
            case 2: return launch_fwd<2, 2, 2, 1, 1>(d, p.splitk, ws, st);
            case 4: return launch_fwd<2, 2, 1, 1, 1>(d, p.splitk, ws, st);
            default: return launch_fwd<4, 1, 1, 1, 1>(d, p.splitk, ws, st);
        }
    }
}

static bool gview_plain(const ssc_gview& g) {
    return g.ab0 == nullptr && g.act == SSC_ACT_NONE &&
           (g.C1 == 0 || (g.ab1 == nullptr && (g.act1 >= 0 ? g.act1 : g.act) == SSC_ACT_NONE));
}

template <int WM, int WN, int SM, int SN, bool GPLAIN, bool DPLAIN, bool DDMA>
static int launch_wgrad_v(const ssc_wgrad_desc& d, int splitk, float* ws, hipStream_t st) {
    constexpr int BM = WM * SM * 32, BN = WN * SN * 32;
    constexpr size_t lds = 2 * (BK * BM + BK * BN) * sizeof(float) + 2 * BK * sizeof(int4);
    const int Cg = d.g.C0 + d.g.C1;
    const int Mtot = d.TH * d.TW * Cg;
    const long P = (long)d.NB * d.PH * d.PW;
    const Magics mg = make_magics((unsigned)Cg, (unsigned)d.TW, (unsigned long)d.PW, (unsigned long)d.PH * d.PW,
                                  (unsigned long)P);
    const int mt = (Mtot + BM - 1) / BM;
    const int nt = (d.Nn + BN - 1) / BN;
    const long out_count = (long)d.TH * d.TW * d.Cg_real * d.ldc;
    static unsigned long long attr_done = 0;
    {
        const int arc = ssc_set_max_lds(reinterpret_cast<const void*>(&conv_wgrad_kernel<WM, WN, SM, SN, GPLAIN, DPLAIN, DDMA>), (int)lds, &attr_done);
        if (arc != 0) return arc;
    }
    dim3 grid((unsigned)mt, (unsigned)nt, (unsigned)splitk);
    // SSC_WG_XCD=1 (developer switch): whole K slices per XCD.  Measured (scripts/wg_xcd_ab.sh): FETCH_SIZE of the encoder_3 filter gradient 113 ->
    // 35 MB, the launch itself unchanged (94.5 vs 94.9 TFLOP/s), the train step 0.4 % SLOWER (18.05 vs 17.98 ms) -- the re-reads
    // of the plain order are served by the Infinity Cache while all XCDs walk the same pixel range -- so it stays off
    static const int wg_xcd = ssc_dev_int("SSC_WG_XCD", 0);
    const int xcd = (wg_xcd && splitk > 1 && (((long)mt * nt * splitk) & 7) == 0) ? 1 : 0;
    hipLaunchKernelGGL((conv_wgrad_kernel<WM, WN, SM, SN, GPLAIN, DPLAIN, DDMA>), grid, dim3(256), lds, st, d, mg, ws, out_count,
                       splitk, xcd);
    if (splitk > 1) launch_wgrad_reduce(ws, out_count, splitk, d.out, d.accumulate, st);
    return (int)hipGetLastError();
}

// the view form (GPLAIN, DPLAIN, DDMA) of a launch: 0 TTT, 1 FTT, 2 TTF, 3 FTF, 4 FFF
static int wgrad_view_form(const ssc_wgrad_desc& d) {
    const bool gp = gview_plain(d.g), dp = gview_plain(d.d);
    static const int ddma_on = ssc_dev_int("SSC_WGRAD_DMA", 1);       // 0: dense tiles through registers (A/B)
    // LDS-DMA of the dense tile: one plain tensor whose byte offsets fit 32 bits
    const bool ddma = ddma_on && dp && d.d.C1 == 0 && (long)d.NB * d.PH * d.PW * d.d.C0 < 0x1fffffffL;
    if (dp && ddma) return gp ? 0 : 1;
    if (dp) return gp ? 2 : 3;
    return 4;       // the full transform covers a plain side
}

template <int WM, int WN, int SM, int SN>
static int launch_wgrad(const ssc_wgrad_desc& d, int splitk, float* ws, hipStream_t st) {
    switch (wgrad_view_form(d)) {
        case 0: return launch_wgrad_v<WM, WN, SM, SN, true, true, true>(d, splitk, ws, st);
        case 1: return launch_wgrad_v<WM, WN, SM, SN, false, true, true>(d, splitk, ws, st);
        case 2: return launch_wgrad_v<WM, WN, SM, SN, true, true, false>(d, splitk, ws, st);
        case 3: return launch_wgrad_v<WM, WN, SM, SN, false, true, false>(d, splitk, ws, st);
        default: return launch_wgrad_v<WM, WN, SM, SN, false, false, false>(d, splitk, ws, st);
    }
}

// split over the pixel (K) dimension: many more choices than the forward form, so search a wider range
static Plan plan_wgrad(const ssc_wgrad_desc& d, int64_t ws_bytes, bool have_ws) {
    const int Cg = d.g.C0 + d.g.C1;
    const long Mtot = (long)d.TH * d.TW * Cg;
    const long P = (long)d.NB * d.PH * d.PW;
    const long nkt = (P + BK - 1) / BK;
    const long out_elems = (long)d.TH * d.TW * d.Cg_real * d.ldc;
    bool allowed[5];
    allowed[0] = d.Nn > 64 && Mtot > 64;
    allowed[1] = d.Nn > 64;                     // 64 gathered columns x 128: the gathered side is the costly one
    allowed[2] = d.Nn > 32 && Mtot > 64;
    allowed[3] = d.Nn > 32 && d.Nn <= 64 && Mtot <= 64;
    allowed[4] = d.Nn <= 32;
    const int ncu = num_cu();
    Plan best = {-1, 1, 1e300, 0, 1};
    static const int force_cfg = ssc_dev_int("SSC_WG_CFG", -1);        // restricts the search to tile configuration n where allowed
    for (int c = 0; c < 5; ++c) {
        if (!allowed[c]) continue;
        if (force_cfg >= 0 && c != force_cfg && allowed[force_cfg]) continue;
        const TileCfg& t = WG_CFGS[c];
        const long mt = (Mtot + t.BM - 1) / t.BM, nt = (d.Nn + t.BN - 1) / t.BN;
        const long blocks = mt * nt;
        const double wfull = (double)nkt * 16.0 * (t.BM / 32) * (t.BN / 32) / 4.0 * 64.0 * t.penalty;
        for (long sk = 1; sk <= 512; sk = (sk < 16 ? sk + 1 : sk + sk / 8)) {
            if (sk > 1 && (!have_ws || nkt / sk < 4 || (int64_t)sk * out_elems * 4 > ws_bytes)) break;
            const long per = (nkt + sk - 1) / sk;
            if ((nkt + per - 1) / per != sk) continue;
            double cost = makespan(blocks * sk, wfull * (double)per / (double)nkt, t.res, ncu) + 2500.0;
            if (sk > 1) cost += 2.0 * sk * (double)out_elems * 4.0 / 1500.0 + plan_reduce_cost();
            if (cost < best.cost) best = {c, (int)sk, cost, 0, 1};
        }
    }
    return best;
}

// which kernel takes a filter-gradient launch: 0 conv_wgrad_kernel, 1 head1, 2 wgrad128, 3 wgn16
static int wgrad_route(const ssc_wgrad_desc* dp, bool have_ws, int64_t ws_bytes) {
    if (have_ws && ws_bytes >= (int64_t)16 * 512 * 4 && ssc_head1_wgrad_supported(dp)) return 1;     // the one-output patch head
    if (ssc_conv_wgrad128_supported(dp)) return 2;                                                  // the large layers
    // 16 output channels, 3x3 x 16 or 4x4 x 64 gathered: 16-column MFMA, when the workspace can hold a slab
    if (have_ws && ssc_conv_wgn16_supported(dp) && ssc_conv_wgn16_fits(dp, ws_bytes)) return 3;
    return 0;
}

extern "C" int ssc_conv_wgrad_kernel_name(const ssc_wgrad_desc* dp, char* buf, int len) {
    static const char* names[5] = {"conv_wgrad<128x128>", "conv_wgrad<64x128>", "conv_wgrad<128x64>",
                                   "conv_wgrad<64x64>", "conv_wgrad<128x32>"};
    const int64_t ample = (int64_t)1 << 40;
    switch (wgrad_route(dp, true, ample)) {
        case 1: copy_name("head1_wgrad", buf, len); break;
        case 2: copy_name(ssc_conv_wgrad128_bf_selected(dp) ? "conv_wgrad128_bf16x6<128x128>" : "conv_wgrad128<128x128>", buf, len); break;
        case 3: copy_name(dp->TH == 3 ? "conv_wgn16<3x3>" : "conv_wgn16<4x4>", buf, len); break;
        default: {
            const Plan p = plan_wgrad(*dp, ample, true);
            copy_name(names[p.cfg < 0 ? 0 : p.cfg], buf, len);
        }
    }
    return 0;
}

extern "C" int ssc_conv_wgrad_plan(const ssc_wgrad_desc* dp, int64_t ws_bytes, int* out4) {
    // host only: {tile configuration, split-K slabs, view form, reduce form}; ws_bytes <= 0 stands for a NULL workspace, any
    // other workspace is taken to be 16-byte aligned
    const ssc_wgrad_desc& d = *dp;
    const bool have_ws = ws_bytes > 0;
    out4[0] = -1; out4[1] = 1; out4[2] = 0; out4[3] = 0;
    if (wgrad_route(dp, have_ws, ws_bytes) != 0) return 0;
    const Plan p = plan_wgrad(d, ws_bytes, have_ws);
    out4[0] = p.cfg;
    out4[1] = p.splitk;
    out4[2] = wgrad_view_form(d);
    if (p.splitk > 1)
        out4[3] = wgrad_reduce_form(nullptr, (long)d.TH * d.TW * d.Cg_real * d.ldc, p.splitk, d.out);
    return 0;
}

extern "C" int ssc_conv_wgrad(const ssc_wgrad_desc* dp, float* ws, int64_t ws_bytes, void* stream) {
    const ssc_wgrad_desc& d = *dp;
    hipStream_t st = (hipStream_t)stream;
    if ((d.g.C0 & 3) || (d.g.C1 & 3) || (d.d.C0 & 3) || (d.d.C1 & 3)) return -1;
    if (d.d.H != d.PH || d.d.W != d.PW) return -2;
    // the filter-gradient slab is dense [TH*TW*Cg_real][ldc]; rows/cols skipped by the kernel
    // (padding channels) do not exist in it, so every slab entry is written when ldc == Nn.
    if (d.ldc != d.Nn) return -3;
    switch (wgrad_route(dp, ws != nullptr, ws_bytes)) {
        case 1: return ssc_head1_wgrad(dp, ws, ws_bytes, stream);
        case 2: return ssc_conv_wgrad128(dp, ws, ws_bytes, stream);
        case 3: return ssc_conv_wgn16(dp, ws, ws_bytes, stream);
        default: break;
    }
    const Plan p = plan_wgrad(d, ws_bytes, ws != nullptr);
    switch (p.cfg) {
        case 0: return launch_wgrad<2, 2, 2, 2>(d, p.splitk, ws, st);
        case 1: return launch_wgrad<1, 4, 2, 1>(d, p.splitk, ws, st);
        case 2: return launch_wgrad<2, 2, 2, 1>(d, p.splitk, ws, st);
        case 3: return launch_wgrad<2, 2, 1, 1>(d, p.splitk, ws, st);
        case 4: return launch_wgrad<4, 1, 1, 1>(d, p.splitk, ws, st);
        default: return -4;
    }
}
#endif  // SSC_ISA_ONLY
