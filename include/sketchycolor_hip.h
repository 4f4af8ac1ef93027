/*
 * sketchycolor_hip.h -- C ABI of libsketchycolor_hip.so (gfx950 / MI355X).
 *
 * The reference (SketchyScene/SketchySceneColorization) has no FFI: every op of
 * its hot path is a stock TensorFlow-1 op invoked from Python.  Each entry point
 * below therefore names the TF op / reference call site it replaces
 * (paths relative to Foreground_Instance_Colorization/obj_lib/).
 *
 * Conventions: every pointer is a DEVICE pointer unless it is a descriptor
 * struct (host memory, read during the call); `stream` is a hipStream_t passed
 * as void*; return value 0 = ok, non-zero = hipError_t or a negative argument
 * error.  No ownership is transferred, no global state is kept, nothing is
 * allocated: callers hand in workspaces.  Activations are NHWC fp32 internally
 * (channel counts padded to a multiple of 4 where noted); filters keep the TF
 * layouts ([kh,kw,Cin,Cout] for conv, [kh,kw,Cout,Cin] for conv-transpose).
 */
#ifndef SKETCHYCOLOR_HIP_H
#define SKETCHYCOLOR_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* activation codes applied on load (after the per-channel affine) */
#define SSC_ACT_NONE 0
#define SSC_ACT_RELU 1   /* tf.nn.relu                 models_collection.py:518,531 */
#define SSC_ACT_LRELU 2  /* tf.maximum(0.2*x, x)       models_collection.py:51-53   */
#define SSC_ACT_TANH 3   /* only for ssc_affine_act / ssc_residual_merge outputs, never on load */
#define SSC_ACT_PRELU 5  /* tf.maximum(leak*x, x) with a trainable scalar leak (models_collection.py:56-60); ssc_concat_parts only,
                            the part's `ab` pointer then addresses the leak */
#define SSC_ACT_MIU 4    /* miu_relu (x + sqrt(0.09 + x^2))/2, models_collection.py:63-65; pointwise kernels only */

/*
 * A "gather view": one or two NHWC tensors seen as a single [N,H,W,C0+C1]
 * tensor (tf.concat on channels, models_collection.py:512-516), with an
 * optional per-channel affine a*x+b (the folded batch-statistics norm,
 * models_collection.py:36-46) followed by an activation, evaluated while the
 * tile is loaded.  Out-of-image taps read 0 (tf.pad CONSTANT, :388).
 */
typedef struct ssc_gview {
    const float* s0;   /* [N,H,W,C0] */
    const float* s1;   /* [N,H,W,C1] or NULL */
    const float* ab0;  /* [2][C0]: a then b for s0; NULL = identity */
    const float* ab1;  /* [2][C1]: a then b for s1; NULL = identity */
    int32_t C0, C1;    /* both multiples of 4 */
    int32_t H, W;
    int32_t act;       /* activation of s0 (and of s1 when act1 < 0) */
    int32_t act1;      /* activation of s1, or -1 = same as act (residual generators concatenate an already
                          activated block output with a raw+norm+lrelu encoder tensor, models_collection.py:660-664) */
} ssc_gview;

/*
 * Implicit-GEMM convolution, forward form:
 *   out[pix][n] = sum_{tap,k} X[pix@tap][k] * F(tap,k,n)
 * Replaces tf.nn.conv2d (models_collection.py:389, residual_util.py:24,33),
 * tf.nn.conv2d_transpose (models_collection.py:402; nphase=4 sub-pixel form)
 * and the data-gradient of both, plus tf.matmul (1x1 form; BasicLSTMCell and
 * fully_connected, models_collection.py:184-236, mru.py:52-92).
 */
typedef struct ssc_conv_desc {
    ssc_gview x;
    const float* w;       /* filter [KH][KW][wC0][wC1] */
    const float* bias;    /* [Nn] or NULL */
    float* out;           /* [NB,OH,OW,ldc] */
    int32_t NB, PH, PW;   /* output lattice: M = NB*PH*PW */
    int32_t TH, TW;       /* taps per lattice point */
    int32_t in_stride;    /* iy = py*in_stride + ioff_y + ty */
    int32_t ioff_y, ioff_x;
    int32_t nphase;       /* 1, or 4 = stride-2 transposed conv (k=4, pad 1) */
    int32_t ky0, kx0, kstep;  /* filter row = ky0 + ty*kstep */
    int32_t KH, KW, wC0, wC1;
    int32_t bmode;        /* 0: k->wC0, n->wC1 ("KN"); 1: n->wC0, k->wC1 ("NK") */
    int32_t k_real;       /* real K channels in the filter (<= x.C0+x.C1).  The stored channels past k_real (padding lanes) must
                             hold FINITE values: the tiled kernels, narrow and tr4_tiny mask the lane, but fewchan, fewchan7 and
                             tr4n16 multiply it by a zero filter row, so a NaN or an infinity there would reach the output */
    int32_t n_off, Nn;    /* first filter n index, number of real outputs */
    int32_t Nstore;       /* columns stored (>= Nn; extra ones are written 0) */
    int32_t OH, OW, ldc;
    int32_t out_stride, ooff_y, ooff_x; /* oy = py*out_stride + ooff_y */
    int32_t epi;          /* 0 none, 1 tanh (models_collection.py:533), 2 lrelu 0.2 (MRU gates, mru.py:407-413) */
    int32_t accumulate;   /* 1: out += result */
    float* stat_partial;  /* set by ssc_conv_forward_bn (callers leave it NULL): per row tile [2][Nstore] sums / sums of squares
                             of the output columns, written by the epilogue */
    uint32_t* sk_flags;   /* stream-K hand-off flags (device): SSC_SK_FLAG_WORDS words, zero before the first launch that
                             uses them and private to the launch stream (the kernel leaves them zero); NULL = the launch
                             may not split tiles across workgroups inside the kernel (split-K slabs + reduce kernel instead) */
    /* set by ssc_conv_forward_bnbwd (callers leave sb_x NULL): the output of this launch is the gradient g w.r.t. act(a*x+b)
       of a batch-statistics-normed tensor x laid out like the output; the rows of stat_partial then hold
       [sum dz | sum dz*xhat], dz = g * act'(a*x+b), xhat = (x - mean) * rstd -- the two sums of the norm's backward */
    const float* sb_x;
    const float* sb_ab;   /* [2][Nstore]: a, b */
    const float* sb_stats;/* [2][Nstore]: mean, 1/std */
    int32_t sb_ldx;       /* row stride of x */
    int32_t sb_act;       /* SSC_ACT_* of the consumer */
    int32_t sk_tag;       /* caller's id of this launch (31 bits): a hand-off that times out reports 0x80000000 | sk_tag */
    /* set by ssc_conv_forward_bnbwd2 (callers leave sb2_x NULL): the output columns [sb2_col0, Nstore) are the gradient w.r.t. a
       SECOND normed tensor (the data gradient of a layer that reads concat[x, x2] -- relu(concat[decoder_{k+1}, encoder_k]),
       models_collection.py:512-531 -- in one launch); the sb_* set then describes columns [0, sb2_col0) only (tables of
       sb2_col0 entries), this set the remaining Nstore - sb2_col0, its rows of sums going to stat_partial2 */
    int32_t sb2_col0;
    const float* sb2_x;
    const float* sb2_ab;
    const float* sb2_stats;
    float* stat_partial2;
    int32_t sb2_ldx;
    int32_t sb2_act;
    int32_t stat_mode;    /* set by ssc_conv_forward_minmax (callers leave 0): 1 = the rows of stat_partial hold the per-column
                             MINIMUM and MAXIMUM of the tile's (activated) outputs instead of sum and sum of squares */
    int32_t ws_kc;
    /* Filter pre-split into three bf16 planes (ssc_filter_split; orientation = bmode), or NULL.  When set and the launch
       qualifies (every 32-wide K-tile inside one tap and one source, n_off a multiple of 32, more than 32 stored columns) the
       contraction runs on the bf16 matrix pipe as six bf16 products per fp32 product with fp32 accumulation (igemm_bf16.hip:
       fp32-grade results at 6/16 of the fp32 MFMA's cycles); `w` must still point at the fp32 filter.  ws_kc / ws_nbp: the
       planes' chunk and block counts as ssc_filter_split_geom reports them. */
    const void* wsplit;
    int32_t ws_nbp;
    int32_t lds_hint;     /* 0: the form that is fastest alone.  1: the launch shares the chip with launches of other streams (a train
                             step's side-by-side chains): prefer the form with the smaller LDS footprint -- the bf16-split kernel on
                             ONE operand stage (42 KB instead of 75 KB: a filter-gradient workgroup fits beside two conv workgroups),
                             3-5 % slower alone, 2.5 % faster per Pix2Pix train iteration */
} ssc_conv_desc;
#define SSC_SK_FLAG_WORDS 8192   /* >= resident workgroups of the largest grid; the last word reports a hand-off timeout:
                                    0 = none, else 0x80000000 | sk_tag of the first launch whose owner workgroup gave up
                                    waiting for a K slice.  The output of that launch is WRONG (a partial sum): callers must
                                    read the word wherever they read results back (losses, snapshots) and fail; the flags
                                    are to be zeroed before the array is used again. */
/*
 * 3-way bf16 split of a filter W[taps][c0][c1] (fp32, c1 contiguous) for the bf16 form of ssc_conv_forward: x = h + m + l
 * exactly, each part a bf16, stored as the B operands of v_mfma_f32_32x32x16_bf16 (fragment-major, zero padded).
 * orient 0: GEMM k = c0, n = c1 (ssc_conv_desc.bmode 0);  orient 1: k = c1, n = c0 (bmode 1).
 * The planes must be refreshed whenever the fp32 filter changes (once per optimizer step).
 */
typedef struct ssc_split_job {
    const float* w;
    void* dst;              /* ssc_filter_split_bytes bytes, 16-byte aligned */
    int32_t taps, c0, c1, orient;
    int64_t first_thread;   /* batch form: running sum of the preceding jobs' `threads` (ssc_filter_split_geom) */
} ssc_split_job;
/* kc, nbp: the planes' chunk / block counts (ssc_conv_desc.ws_kc, ws_nbp); bytes: size of the planes buffer; threads: the
   job's share of a batch launch (whole blocks of 256) */
int ssc_filter_split_geom(int taps, int c0, int c1, int orient, int* kc, int* nbp, int64_t* bytes, int64_t* threads);
int ssc_filter_split(const float* w, int taps, int c0, int c1, int orient, void* dst, void* stream);
/* allocates the bf16 form's per-device constants (a hipMalloc + a copy: call once OUTSIDE any stream capture, before the first
   launch that carries `wsplit`; the launches call it too) */
int ssc_bf16_prepare(void);
/* jobs_dev: DEVICE array; total_threads = sum of the jobs' `threads` */
int ssc_filter_split_batch(const ssc_split_job* jobs_dev, int njobs, int64_t total_threads, void* stream);

/* hand-off wait bound in milliseconds (default 20000: only a deadlock guard -- the owner waits for workgroups that were
 * dispatched before it) and a test hook that makes the producers withhold their flags so that the bound is reached */
int ssc_sk_configure(int timeout_ms, int test_withhold);

/*
 * Implicit-GEMM filter gradient:
 *   dF[(tap,cg)][cd] = sum_pix G[pix@tap][cg] * D[pix][cd]
 * G is the gathered (higher-resolution) side, D the 1x1 side at the lattice.
 * Replaces the filter-gradient of tf.nn.conv2d / conv2d_transpose / matmul
 * produced by optim.compute_gradients (graph_single.py:24-30, 309-312).
 */
typedef struct ssc_wgrad_desc {
    ssc_gview g;
    ssc_gview d;
    float* out;           /* [(tap*Cg_real + cg)][ldc] */
    int32_t NB, PH, PW;
    int32_t TH, TW, in_stride, ioff_y, ioff_x;
    int32_t Cg_real;      /* real gathered channels (<= g.C0+g.C1) */
    int32_t Nn;           /* real dense channels (<= d.C0+d.C1) */
    int32_t ldc;
    int32_t accumulate;
    int32_t exact;        /* 1: the exact-fp32 MFMA kernels only; 0: the large layers may run as a 3-way bf16 split of both operands on
                             the bf16 matrix pipe (wgrad128_bf16.hip: six products per fp32 product, fp32 accumulate) */
    int32_t _pad;
} ssc_wgrad_desc;

/* library / device info */
int ssc_version(void);
/* the 16-hex-digit sha256 prefix of the sources (csrc + this header) the binary was built from: callers compare it with the hash
 * of the tree they run from (sketchyscenecolorization_amd/build.py tree_hash) and refuse a stale binary */
int ssc_build_hash(char* buf, int len);
int ssc_device_info(int* cu_count, int* wave_size, char* arch, int arch_len);

/* implicit GEMM (igemm.hip).  ws: split-K slab workspace (may be NULL). */
int ssc_conv_forward(const ssc_conv_desc* d, float* ws, int64_t ws_bytes, void* stream);
int ssc_conv_wgrad(const ssc_wgrad_desc* d, float* ws, int64_t ws_bytes, void* stream);
/* filter gradients of the large layers on a 128 x 128 accumulator tile (wgrad128.hip); ssc_conv_wgrad dispatches to it when
 * _supported: the gathered channels a multiple of 128 inside one source (or exactly 64: two taps per tile), no channel
 * padding on the gathered side, >= 128 real dense channels, every tensor below 2 GiB */
int ssc_conv_wgrad128_supported(const ssc_wgrad_desc* d);
int ssc_conv_wgrad128(const ssc_wgrad_desc* d, float* ws, int64_t ws_bytes, void* stream);
/* filter gradients with 16 dense channels of the 3x3 conv over 16 and the 4x4 stride-1 conv over 64 gathered channels
 * (residual_util.py:92-96, 147-151) on the 16-column MFMA (wgn16.hip); ssc_conv_wgrad dispatches to it when _supported */
int ssc_conv_wgn16_supported(const ssc_wgrad_desc* d);
/* conv + the batch-statistics norm of its output [M*nphase rows, Nstore == ldc columns] folded to ab = [a; b] (y = a*x + b)
 * and stats = [mean; rstd] (models_collection.py:36-46 after :389 / :402): the column sums come out of the conv epilogue
 * when the launch allows it, else ssc_bn_stats reads the output back */
int ssc_conv_forward_bn(const ssc_conv_desc* d, float* ws, int64_t ws_bytes, const float* scale, const float* offset,
                        float eps, float* ab, float* stats, void* stream);
/* the one-output patch head over a 512-channel tensor (discriminate_pix2pix layer_5, models_collection.py:833-835: 4x4,
 * stride 1, 512 -> 1) as streaming kernels (head1.hip): forward (ws: 64 B per input pixel), its data gradient (the
 * hip.conv_dgrad descriptor: one-channel dy, "NK" filter, flipped taps) and its filter gradient (ws: up to 256 x 32 KB slabs).
 * ssc_conv_forward / ssc_conv_wgrad dispatch to them when _supported. */
int ssc_head1_forward_supported(const ssc_conv_desc* d);
int ssc_head1_forward(const ssc_conv_desc* d, float* ws, int64_t ws_bytes, void* stream);
int ssc_head1_dgrad_supported(const ssc_conv_desc* d);
int ssc_head1_dgrad(const ssc_conv_desc* d, void* stream);
int ssc_head1_wgrad_supported(const ssc_wgrad_desc* d);
int ssc_head1_wgrad(const ssc_wgrad_desc* d, float* ws, int64_t ws_bytes, void* stream);
/* the head's data gradient fused with the backward of the batch norm + activation of its input tensor x [pixels][512]
 * (layer_4: models_collection.py:823-830): the gradient w.r.t. act(norm(x)) is recomputed in both passes of the norm backward
 * and never stored.  d = the hip.conv_dgrad descriptor (out ignored), ab = [a; b], stats = [mean; rstd], rowb [NB][512] or
 * NULL = a per-image term (the class head's gradient through its spatial mean) added with rowb_scale; dx [pixels][512];
 * dscale / doffset [512] or NULL; ws >= (2 * 512 + 2) * 512 floats.  -1: not this shape (callers then use ssc_conv_forward +
 * ssc_bn_act_backward_pre) */
int ssc_head1_dgrad_bn_backward(const ssc_conv_desc* d, const float* x, const float* ab, const float* stats, int act,
                                const float* rowb, float rowb_scale, float* dx, float* dscale, float* doffset, float* ws,
                                int64_t ws_bytes, void* stream);
/* rows of partial sums [nblk][2][C] of a norm backward -> coef [2][C] = [mean dz; mean dz*xhat], dscale / doffset (may be NULL) */
int ssc_bn_bwd_finalize(const float* partial, int nblk, int C, int64_t M, float* coef, float* dscale, float* doffset,
                        void* stream);
/* direct (vector-ALU, LDS patch) form for <= 4 output channels; ssc_conv_forward dispatches to it (narrow.hip) */
int ssc_conv_narrow_supported(const ssc_conv_desc* d);
int ssc_conv_narrow_forward(const ssc_conv_desc* d, void* stream);
/* 1 when ssc_conv_forward runs the launch on the few-input-channel kernel (fewchan.hip): 4x4 stride-2 pad-1 conv over a
 * single 4- or 8-channel raw source to 33..64 outputs, output lattice a multiple of 4 x 32 -- generator encoder_1
 * (models_collection.py:454-458), discriminator layer_1 (:798-801), the data gradient of decoder_1 (:529-534) */
/* the 1x1 expansion conv of the bottleneck blocks (K = 16 .. 128 input channels, N = 4 K outputs): streaming kernel (pw1x1.hip) */
int ssc_conv_pw1x1_supported(const ssc_conv_desc* d);
/* the 3x3 stride-1 conv of the bottleneck blocks at 16 / 32 channels and its data gradient (residual_util.py:92-96): streaming
   kernel (c3x3.hip); the batch statistics (ssc_conv_forward_bn) / norm-backward sums (ssc_conv_forward_bnbwd) ride as per-lane sums.
   At most as many outputs as channels (4 .. C): the kernels stage C columns of the filter */
int ssc_conv_c3x3_supported(const ssc_conv_desc* d);
/* the 4x4 stride-2 conv 64 -> <= 16 channels (block_1 of the first encoder bottleneck, residual_util.py:87-91) on the 16-column
   MFMA with K split over the four wavefronts (s2n16.hip) */
int ssc_conv_s2n16_supported(const ssc_conv_desc* d);
/* the k = 4 stride-2 transposed conv 256 -> <= 16 channels (block_1 of the last decoder bottleneck) on the 16-column MFMA, one
   sub-pixel phase per workgroup (tr4n16.hip) */
int ssc_conv_tr4n16_supported(const ssc_conv_desc* d);
/* the Residual / Background generators' first conv, 7x7 stride 2 over the padded image channels -> 64 (fewchan7.hip) */
int ssc_conv_fewchan7_supported(const ssc_conv_desc* d);
/* the k = 4 stride-2 transposed convs of the Background generator's region branch (<= 4 channels in and out,
   bg_colorization_main.py:392-397): a thread per lattice pixel (tr4tiny.hip) */
int ssc_conv_tr4_tiny_supported(const ssc_conv_desc* d);
int ssc_conv_fewchan_supported(const ssc_conv_desc* d);
/* name of the tile configuration the launcher picks for a descriptor (host only; for profiling) */
int ssc_conv_forward_kernel_name(const ssc_conv_desc* d, char* buf, int len);
int ssc_conv_wgrad_kernel_name(const ssc_wgrad_desc* d, char* buf, int len);
/* the launch plan for a descriptor (host only; tuning and tests): out5 = {tile configuration, split-K slabs, whole
 * tiles, K slices per remaining tile (combined inside the launch), modelled kilo-cycles} */
int ssc_conv_forward_plan(const ssc_conv_desc* d, int64_t ws_bytes, int* out5);
/* what ssc_conv_forward_bn / _bnbwd / _bnbwd2 / _minmax (rider = SSC_RIDER_*) would do with a descriptor (host only, launches
 * nothing; computed by the function those entry points decide with): out5 = {path (SSC_RIDER_PATH_*), the kernel that runs
 * (0 the tiled ones, 1 head1 forward, 2 head1 dgrad, 3 narrow, 4 fewchan, 5 pw1x1, 6 c3x3, 7 s2n16, 8 tr4_tiny, 9 fewchan7,
 * 10 tr4n16: the dispatch order), rows of partial results (*nrows of _bnbwd / _bnbwd2), where they lie (SSC_RIDER_ROWS_*), the
 * workspace bytes the conv itself keeps}.  ws_bytes <= 0 stands for a NULL workspace.  site0 (_bnbwd) / site0, site1, C0
 * (_bnbwd2) as those entry points take them, never dereferenced beyond the structs; NULL, NULL, 0 for the other riders. */
#define SSC_RIDER_BN 0
#define SSC_RIDER_BNBWD 1
#define SSC_RIDER_BNBWD2 2
#define SSC_RIDER_MINMAX 3
#define SSC_RIDER_PATH_PLAIN 0  /* the launch as ssc_conv_forward makes it: separate pass (_bn, _minmax) or *nrows = 0 */
#define SSC_RIDER_PATH_STREAM 1 /* a streaming kernel that carries the rider: a row per walker */
#define SSC_RIDER_PATH_TILE 2   /* the tile epilogue: a row per row tile and phase */
#define SSC_RIDER_PATH_SLAB 3   /* _bn of a split-K launch: the statistics ride in the slab sum */
#define SSC_RIDER_ROWS_NONE 0
#define SSC_RIDER_ROWS_WS_HEAD 1   /* at the workspace's start (the streaming kernels use no workspace) */
#define SSC_RIDER_ROWS_WS_TAIL 2   /* behind the conv's share of the workspace */
#define SSC_RIDER_ROWS_CALLER 3    /* in the sites' partial buffers */
struct ssc_bnbwd_site;
int ssc_conv_rider_plan(const ssc_conv_desc* d, int rider, int64_t ws_bytes, const struct ssc_bnbwd_site* site0,
                        const struct ssc_bnbwd_site* site1, int C0, int64_t* out5);
/* the launch plan of a filter gradient that reaches the general kernel (conv_wgrad_kernel of igemm.hip; host only, launches
 * nothing): out4 = {tile configuration (0 128x128, 1 64x128, 2 128x64, 3 64x64, 4 128x32; -1: the patch head, the 128 x 128 or
 * the 16-column kernel takes the launch), split-K slabs, view form (gathered side plain, dense side plain, dense tile by LDS-DMA:
 * 0 TTT, 1 FTT, 2 TTF, 3 FTF, 4 FFF), the kernel that sums the slabs (0 none, 1 reduce4, 2 reduce<1>, 3 reduce<4>, 4 reduce<16>)}.
 * ws_bytes <= 0 stands for a NULL workspace; any other workspace is taken to be 16-byte aligned.  Computed by the functions
 * that make the launch. */
int ssc_conv_wgrad_plan(const ssc_wgrad_desc* d, int64_t ws_bytes, int* out4);
/* the launch plan of a filter gradient on the 128 x 128 kernels (wgrad128.hip, wgrad128_bf16.hip; host only, launches nothing):
 * -10 when neither takes the launch (ssc_conv_wgrad128_supported says no), else 0 and out7 = {arithmetic (0 exact fp32, 1 bf16x6),
 * taps per tile (the kernels' TPT), gathered side plain (0 / 1), dense path (0 plain by LDS-DMA, 1 plain through registers,
 * 2 folded norm / activation; the bf16 kernel: 0 plain, 2 transformed), split-K slabs, workgroups in XCD order (0 / 1),
 * the bf16 kernel's two LDS stages DB (0 / 1; 0 for the exact kernel)}: seven values, DB is the seventh.  ws_bytes <= 0 stands
 * for a NULL workspace.  Computed by the functions that make the launch. */
int ssc_conv_wgrad128_plan(const ssc_wgrad_desc* d, int64_t ws_bytes, int* out7);
/* the launch plan of a forward conv / data gradient / matmul on the bf16x6 kernels (conv_bf_kernel, conv_bfh_kernel of
 * igemm_bf16.hip; host only, launches nothing): -10 when they do not take the launch (no filter planes, a shape outside the
 * bf16 form, SSC_ARITH=fp32, or one of the kernels ssc_conv_forward dispatches earlier takes it), ssc_conv_forward's own error
 * for a descriptor it rejects, else 0 and out10 = {kernel (0 conv_bf_kernel on 32-k stages, 1 conv_bfh_kernel on 16-k stages),
 * tile configuration (0 128x128, 1 64x128, 2 128x64, 4 64x64), PLAIN (0 / 1), source form (0 two uniform sources, 1 one uniform,
 * 2 one with a partly empty last chunk: KM), SS (one LDS stage per operand, 0 / 1), korder (0 one tap, 1 tap by tap, 2 the four
 * parity classes), grid layout (0 3-D grid, 1 1-D XCD order, 2 XCD order with the four phases adjacent, 3 whole tiles + K slices
 * combined in the launch, 4 split-K slabs + reduce), split-K slabs, whole tiles (layout 3: the tiles one workgroup computes
 * alone; otherwise all tiles), K slices per remaining tile}: ten values.  ws_bytes <= 0 stands for a NULL workspace.  Computed by
 * the functions that make the launch. */
int ssc_conv_bf_plan(const ssc_conv_desc* d, int64_t ws_bytes, int* out10);
/* the launch plan of a forward conv / data gradient on one of the seven streaming kernels ssc_conv_forward dispatches before the
 * tiled ones (fewchan.hip, pw1x1.hip, c3x3.hip, s2n16.hip, tr4tiny.hip, fewchan7.hip, tr4n16.hip; host only, launches nothing):
 * -10 when none of them takes the descriptor, ssc_conv_forward's own error for a descriptor it rejects, else 0 and out4 = {the
 * kernel in the dispatch order (the ids of ssc_conv_rider_plan: 4 fewchan, 5 pw1x1, 6 c3x3, 7 s2n16, 8 tr4_tiny, 9 fewchan7,
 * 10 tr4n16), the instantiation within that kernel, tiles, workgroups launched}.  Instantiations:
 *   fewchan   0 fewchan_conv_kernel<4>, 1 fewchan_conv_kernel<8> (stored input channels)
 *   pw1x1     2 * log2(K / 16) + NARROW of pw1x1_kernel<K, NARROW>: K = 16, 32, 64, 128 input channels; NARROW = 1 at 64 outputs
 *             (two row blocks x two column blocks per workgroup), 0 above (column groups of 128 on the grid's second axis)
 *   c3x3      0 c3x3n16_kernel (16 channels -> <= 16 on the 4 x 32 tile), 1 c3x3_kernel<16, 16>, 2 c3x3_kernel<32, 32>,
 *             3 c3x3_kernel<32, 16> (<channels, tile width>: the 8 x 16 tile where it wastes fewer pixels than 4 x 32)
 *   s2n16     0 s2n16_kernel<2> (stride 2), 1 s2n16_kernel<1> (stride 1)
 *   tr4_tiny, fewchan7, tr4n16   0
 * tiles: row tiles of 64 over the column groups (pw1x1: a column group per grid row), output tiles (fewchan, c3x3, s2n16,
 * fewchan7), blocks of 256 lattice pixels (tr4_tiny: nothing is walked, tiles == workgroups), lattice tiles over the four phases
 * (tr4n16: a phase per grid row).  tiles > workgroups means that some persistent workgroup walks two tiles or more.  Computed
 * by the functions that make the launch. */
int ssc_conv_stream_plan(const ssc_conv_desc* d, int* out4);

/* --- layout (elementwise.hip) --- */
/* dst[n,hw,coff+c] = src[n,c,hw]; tf.transpose NCHW->NHWC (models_collection.py:381) */
int ssc_nchw_to_nhwc(const float* src, float* dst, int N, int C, int HW, int ldc, int coff, void* stream);
/* dst[n,c,hw] = src[n,hw,coff+c] */
int ssc_nhwc_to_nchw(const float* src, float* dst, int N, int C, int HW, int ldc, int coff, void* stream);
/* Device-side image pre / post-processing of the inference, test and validation procedures
 * (main_procedure.py:361-621).  src uint8 [N,H,W,3] -> dst float [N,H,W,4] = src/255*2-1 (channel 3 = 0), optionally
 * after thicken_drawings (input_pipeline.py:242-257: 2x2 grey dilation of the dark strokes of channel 0). */
int ssc_sketch_preprocess_u8(const uint8_t* src, int N, int H, int W, int thicken, float* dst, void* stream);
/* src float NHWC rows of ldc floats, image in channels [coff, coff+3) -> dst uint8 [M,3] = ((x+1)/2*255) truncated */
int ssc_image_postprocess_u8(const float* src, int ldc, int coff, int64_t M, uint8_t* dst, void* stream);
/* --- the Background module's uint8 boundary (bg_io.hip) ---
 * One pass from the loader's arrays to what a train step reads (bg_colorization_main.py:30-33, 100-113, 765-768): fg, bg uint8
 * [M,3], labels int32 [M] -> inputs, targets float [M,3] = u8/255*2-1 (divide, multiply, subtract, each rounded to fp32),
 * xd_real float [M,8] = [inputs | targets | 0 0] (the discriminator's real pair, :596-600) and count[0] = #(labels != 0) as a
 * float (:612-616), summed as an integer: exact and the same for every launch geometry.  M <= 2^24.  workspace: 8 bytes,
 * 8-byte aligned (zeroed on the stream by this call).  fg / bg 4-byte, the other arrays 16-byte aligned. */
int ssc_bg_stage_u8(const uint8_t* fg, const uint8_t* bg, const int32_t* labels, int64_t M, float* inputs, float* targets,
                    float* xd_real, float* count, void* workspace, int64_t workspace_bytes, void* stream);
/* The same pass for a batch of N samples of P pixels gathered from device-resident caches: fg_cache uint8 [S_fg,P,3], bg_cache
 * uint8 [S_bg,P,3], seg_cache uint8 [S_seg,P] = the red channel of the segment png; slot int32 [N,3] = the fg, bg and seg entry
 * of each sample.  Writes what ssc_bg_stage_u8 writes and labels int32 [N,P] = 1 where seg == 128, 2 where seg == 255, else 0
 * (data_processing/image_processing.py:14-25).  recolor uint8 [N,8] = {enable, sky r, g, b, ground r, g, b, 0} (may be NULL):
 * where enable != 0 the background is seg == 128 ? sky : seg == 255 ? ground : bg, the augmented background of
 * data_preparation/bg_data_generation.py:120-160 made from the base one.  A sample whose slot lies outside its cache reads
 * nothing: its float outputs are NaN (the pair's two pad lanes stay 0), its labels 0, and count[0] is NaN.  N * P <= 2^24.
 * workspace: 8 bytes, 8-byte aligned (zeroed on the stream by this call).  Caches and slot 4-byte, recolor 8-byte, the outputs
 * 16-byte aligned; entries and float rows inside them need no alignment (P may be any number).
 * Returns -1 for sizes out of range, -2 for the workspace, -3 for a misaligned pointer. */
int ssc_bg_stage_cached_u8(const uint8_t* fg_cache, int64_t S_fg, const uint8_t* bg_cache, int64_t S_bg, const uint8_t* seg_cache,
                           int64_t S_seg, const int32_t* slot, const uint8_t* recolor, int64_t N, int64_t P, float* inputs,
                           float* targets, float* xd_real, int32_t* labels, float* count, void* workspace,
                           int64_t workspace_bytes, void* stream);
/* img float rows of ldc >= 3 floats (the generator's tanh image) -> out uint8 [M,3] = floor(clamp((x+1)/2, 0, 1)*255 + 0.5)
 * clamped to 0..255 (deprocess + convert_image_dtype(saturate=True), :36-39, 785-786); where mask uint8 [M] (may be NULL) is 0
 * the pixel of fg uint8 [M,3] is written instead (the paste-back of test mode, :861-871).  fg may be NULL without a mask. */
int ssc_bg_finish_u8(const float* img, int ldc, const uint8_t* fg, const uint8_t* mask, int64_t M, uint8_t* out,
                     void* stream);
/* --- full-reference image scores of the evaluation modes (metrics.hip) ---
 * a, b uint8 [N,H,W,3] (the arrays --mode val / --mode test write as PNG), mask uint8 [N,H,W] or NULL: a pixel is counted when
 * mask is NULL or its mask byte is not 0.  out double [N,5], per image:
 *   0  sum |a-b| over the counted pixels and the 3 channels        1  sum (a-b)^2 over the same
 *   2  the number of counted pixels
 *   3  the SSIM sum over the counted windows and the 3 channels    4  the number of counted windows, per channel
 * 0, 1, 2 and 4 are integers and exact.  SSIM (Wang et al. 2004) per channel on the byte values: 11x11 separable window,
 * "valid" positions only ((H-10)*(W-10) windows; none, and no error, when H < 11 or W < 11), weights win11 double [11]
 * (device; exp(-(i-5)^2 / (2*1.5^2)) normalised to sum 1, made once by the host in float64), mu = sum w*x, var = sum w*x^2 -
 * mu^2 (biased), cov likewise, C1 = (0.01*255)^2, C2 = (0.03*255)^2, ssim = (2 mu_a mu_b + C1)(2 cov + C2) / ((mu_a^2 + mu_b^2
 * + C1)(var_a + var_b + C2)).  With a mask a window is counted when its centre pixel is; it still reads all 121 pixels.
 * The moments and the SSIM sum are formed in double: the variance is a difference of terms near 65025 set against C2 = 58.5.
 * One workgroup per 24x32 tile writes its five partial sums to ws, a second launch adds an image's tiles in a fixed order: no
 * floating-point atomics, the same bits from run to run.  ws: N * ceil(H/24) * ceil(W/32) * 5 doubles, 8-byte aligned.
 * Returns -1 for sizes out of range, -2 for a workspace that is too small or misaligned, -3 for a misaligned win11 / out;
 * nothing is launched and out is not written then. */
int ssc_image_metrics_u8(const uint8_t* a, const uint8_t* b, const uint8_t* mask, int N, int H, int W, const double* win11,
                         double* out, void* ws, int64_t ws_bytes, void* stream);
/* The same five sums for two FLOAT images whose uint8 forms are never written: scoring a held-out set during training, in place
 * of the checkpoint scoring the reference meant to have (graph_single.py:557-559: its Inception call, commented out).
 * a float NHWC, rows of lda floats, the image in channels [coff_a, coff_a + 3) (the generator's output buffer: lda 4 or 8);
 * b the same form (ldb, coff_b) or, with b_planar != 0, planar NCHW [N,3,H,W] (what ssc_decode_paired_cached_u8 writes; ldb and
 * coff_b are then not read).  No mask.  Every value is quantised while the tile is loaded, with the arithmetic of
 * ssc_image_postprocess_u8: (x+1)/2*255, each operation rounded to fp32, fmaxf(v, 0) then fminf(.., 255) (NaN becomes 0),
 * truncating cast; from there on it is ssc_image_metrics_u8's code.  out is therefore bit-identical to ssc_image_metrics_u8 of
 * the two postprocessed images, and the same bits from run to run.  16-byte loads where the layout allows (NHWC with ld 4 or 8
 * on a 16-byte aligned base; four consecutive pixels of a plane), single floats elsewhere; padding channels are never part of
 * a result and nothing outside [N,H,W] is read.  ws as for ssc_image_metrics_u8.
 * Returns -1 for sizes out of range (N < 1, coff + 3 > ld, ...), -2 for a workspace that is too small or misaligned, -3 for a
 * misaligned pointer (a, b: 4 bytes; win11, out: 8); nothing is launched and out is not written then. */
int ssc_image_metrics_f32(const float* a, int lda, int coff_a, const float* b, int ldb, int coff_b, int b_planar, int N, int H,
                          int W, const double* win11, double* out, void* ws, int64_t ws_bytes, void* stream);
/* The same five sums for the Background generator's FLOAT image against a uint8 target: scoring a held-out set during Background
 * training.  img float rows of ldc >= 3 floats, the tanh image in channels 0..2; fg, target uint8 [N,H,W,3]; mask uint8 [N,H,W] or
 * NULL (fg may then be NULL too).  While the tile is loaded, image a of a pixel becomes the fg byte where the mask byte is 0 and
 * otherwise the img value quantised with the arithmetic of ssc_bg_finish_u8: floor(clamp((x+1)/2, 0, 1)*255 + 0.5) clamped to
 * 0..255, each operation rounded to fp32, NaN to 0.  Image b is the target, and the mask counts pixels as in
 * ssc_image_metrics_u8.  out is therefore bit-identical to ssc_image_metrics_u8(ssc_bg_finish_u8(img, fg, mask), target, mask),
 * and the same bits from run to run; the uint8 image is never written.  16-byte loads where ldc is 4 on a 16-byte aligned base,
 * single floats elsewhere; nothing outside [N,H,W] is read.  ws as for ssc_image_metrics_u8.
 * Returns -1 for sizes out of range (N < 1, ldc < 3, a mask without fg, ...), -2 for a workspace that is too small or misaligned,
 * -3 for a misaligned pointer (img: 4 bytes; win11, out: 8); nothing is launched and out is not written then. */
int ssc_image_metrics_bg_f32(const float* img, int ldc, const uint8_t* fg, const uint8_t* target, const uint8_t* mask, int N, int H,
                             int W, const double* win11, double* out, void* ws, int64_t ws_bytes, void* stream);
/* --- colour scores of the same images (color_metrics.hip) ---
 * a, b, mask and the rule that counts a pixel as for ssc_image_metrics_u8.  A byte colour goes to CIELAB in double: c = byte/255,
 * lin = c/12.92 where c <= 0.04045, else ((c+0.055)/1.055)^2.4 -- lin256 double [256] (device), that table, made once by the host
 * in float64, so the device evaluates no pow --, XYZ = [[0.412453, 0.357580, 0.180423], [0.212671, 0.715160, 0.072169],
 * [0.019334, 0.119193, 0.950227]] lin, each component divided by the white point (0.95047, 1, 1.08883), f(t) = cbrt(t) where
 * t > (6/29)^3, else t / (3 (6/29)^2) + 4/29, L = 116 f(Y) - 16, a* = 500 (f(X) - f(Y)), b* = 200 (f(Y) - f(Z)).
 * out double [N,13], per image, over the counted pixels:
 *   0  sum dE = sqrt(dL^2 + da^2 + db^2) (CIE76) between a and b      1  sum dab = sqrt(da^2 + db^2)      2  sum |dL|
 *   3  the number of counted pixels
 *   4..7   of image a: sum rg, sum rg^2, sum yb2, sum yb2^2 with rg = R - G, yb2 = R + G - 2 B on the bytes (what colourfulness,
 *          Hasler & Suesstrunk 2003, is made of; the host forms it)              8..11  the same four sums of image b
 *   12 sum over the 23 x 23 cells of min(hist_a, hist_b): the histograms of (a*, b*), cells of width 10, the cell of a coordinate
 *      v = clamp(floor((v + 115) / 10), 0, 22), cell number = cell(a*) * 23 + cell(b*)
 * 3..12 are integers and exact: no byte colour lies within 4e-8 of a cell boundary, far above any rounding of the double formulas.
 * hist int64 [N,2,529] or NULL: the counts of image a and of image b.  Every operation of the float formulas is rounded on its
 * own (no contraction).  One workgroup per run of 1024 pixels writes its twelve sums to ws and adds its cell counts to the
 * image's with integer atomics; a second launch adds an image's runs in a fixed order: no floating-point atomics, the same bits
 * from run to run.  ws: N * ceil(H*W/1024) * 12 doubles + N * 2 * 529 int64, 8-byte aligned.
 * Returns -1 for sizes out of range, -2 for a workspace that is too small or misaligned, -3 for a misaligned lin256 / out / hist;
 * nothing is launched and out is not written then. */
int ssc_color_metrics_u8(const uint8_t* a, const uint8_t* b, const uint8_t* mask, int N, int H, int W, const double* lin256,
                         double* out, int64_t* hist, void* ws, int64_t ws_bytes, void* stream);
/* The same thirteen numbers for two FLOAT images, the arguments and the quantisation of ssc_image_metrics_f32 (the arithmetic of
 * ssc_image_postprocess_u8, NHWC with lda / ldb and channel offsets, or a planar b): out and hist are bit-identical to
 * ssc_color_metrics_u8 of the two postprocessed images.  Returns as ssc_color_metrics_u8; -3 also for a, b off 4 bytes. */
int ssc_color_metrics_f32(const float* a, int lda, int coff_a, const float* b, int ldb, int coff_b, int b_planar, int N, int H,
                          int W, const double* lin256, double* out, int64_t* hist, void* ws, int64_t ws_bytes, void* stream);
/* The same thirteen numbers for the Background generator's FLOAT image against a uint8 target, the arguments and the quantisation
 * of ssc_image_metrics_bg_f32: out and hist are bit-identical to ssc_color_metrics_u8(ssc_bg_finish_u8(img, fg, mask), target,
 * mask).  ssc_bg_finish_u8 writes a pixel of fg exactly where the mask leaves the pixel uncounted, so fg is never read; it is
 * an argument for the sake of the pair, and a mask without it is refused as there.
 * Returns as ssc_color_metrics_u8; -1 also for ldc < 3 and a mask without fg, -3 also for img off 4 bytes. */
int ssc_color_metrics_bg_f32(const float* img, int ldc, const uint8_t* fg, const uint8_t* target, const uint8_t* mask, int N, int H,
                             int W, const double* lin256, double* out, int64_t* hist, void* ws, int64_t ws_bytes, void* stream);
/* Confusion counts of the region branch (metrics.hip): logits float rows of ld >= K floats, 1 <= K <= 4 (ssc_seg_ce_loss's limit),
 * labels int32 [N,P] -> out int64 [N][K*K+1]: out[n][t*K+p] = the pixels of sample n with label t and prediction p; the last slot
 * = the pixels whose label lies outside [0, K), which are in no other cell.  The prediction is the lowest index among the largest
 * logits, found with strict > from index 0 against -inf: a NaN never wins and a row of NaN predicts 0.  Integer counts: one
 * workgroup per run of pixels writes its counts to ws, a second launch adds a sample's workgroups in order; no atomics.
 * ws: N * min(max(ceil(P/1024), 1), 256) * (K*K+1) int64, 8-byte aligned.  N <= 65535, P < 2^31.
 * Returns -1 for sizes out of range, -2 for a workspace that is too small or misaligned, -3 for a misaligned pointer (logits,
 * labels: 4 bytes; out: 8); nothing is launched and out is not written then. */
int ssc_seg_confusion(const float* logits, int ld, int K, const int32_t* labels, int64_t N, int64_t P, int64_t* out, void* ws,
                      int64_t ws_bytes, void* stream);
/* --- the background of a user scene (bg_scene.hip; Pipeline_utils/bg_utils.py::build_background_colorization) ---
 * All images uint8 [H,W,3]; inner uint8 [H,W] = 0 for background, k + 1 for instance k.  Nothing returns to the host between
 * the launches of a scene.  Returns -1 for sizes out of range or a missing array, -2 for the workspace, -3 for a misaligned
 * pointer (every uint8 array but sketch and grass: 4 bytes; img: 4 bytes); nothing is launched then.
 * Crop (:222-224): fg_out uint8 [M,3] = prev where inner != 0, white elsewhere.  M <= 2^24. */
int ssc_bg_scene_crop_u8(const uint8_t* prev, const uint8_t* inner, int64_t M, uint8_t* fg_out, void* stream);
/* Compose (:290-314).  (1) out = img under the cast of ssc_bg_finish_u8 (img float rows of ldc >= 3 floats); (2) where inner != 0,
 * out = fg; (3) with moved[i][j] = sketch[i-1][j-1] for i, j >= 1 and sketch[i][j] in row 0 and column 0: where moved's red byte
 * is 0 and grass[inner] == 0, out and fg_marked take moved's pixel; elsewhere fg_marked = fg.  grass uint8 [256]: grass[v] = 1
 * when instance v - 1 is grass (class 27), grass[0] = 0.  overlay_only != 0 (:319, behind the gradient): step 3 alone on the
 * image already in out; img, fg and fg_marked are not touched and may be NULL.  H * W <= 2^24. */
int ssc_bg_scene_compose_u8(const float* img, int ldc, const uint8_t* fg, const uint8_t* inner, const uint8_t* grass,
                            const uint8_t* sketch, int H, int W, uint8_t* out, uint8_t* fg_marked, int overlay_only,
                            void* stream);
/* add_color_gradient (:96-166) in three launches.  img_bg = white where inner != 0, else color.  The sky colour is the most
 * frequent RGB triple among the pixels with inner == 0 of rows search_from .. search_from + search_height - 1, the one met first
 * in row-major order on a tie; sky_bottom the largest row <= H/2 of img_bg that holds it; start_height = floor(3 * sky_bottom /
 * 4).  Every pixel goes u8 / 255. -> HSV -> RGB -> * 255. -> truncating cast in float64, one IEEE operation per NumPy operation
 * of skimage's rgb2hsv / hsv2rgb, no contraction; rows i <= start_height get S = ((sh-i)/sh) * (s_sky/3) + (i/sh) * s_sky and
 * V = ((sh-i)/sh) * min(1, 1.5 * v_sky) + (i/sh) * v_sky, the sky colour's HSV taken from float32(c) / float32(255).  Where
 * inner != 0 out is color.  status int32 [1]: 0 ok; 1 no pixel with inner == 0 in the search rows; 2 start_height == 0 (the
 * reference fails in both); with a non-zero status out is color unchanged.  workspace: 16 bytes, 4-byte aligned; it holds int32
 * {sky colour r | g << 8 | b << 16, sky_bottom, start_height, 0} afterwards.  Integer compares and an integer atomic maximum
 * decide everything: the same bytes on every run.
 * -1 as well for search_height < 1, search_from < 0, search_from + search_height - 1 > H/2 (sky_bottom might not exist) and
 * search_height * W > 8192 (the search rows' colours sit in LDS). */
int ssc_bg_sky_gradient_u8(const uint8_t* color, const uint8_t* inner, int H, int W, int search_from, int search_height,
                           uint8_t* out, int32_t* status, void* workspace, int64_t workspace_bytes, void* stream);
/* --- the instances of a user scene (fg_scene.hip; Pipeline_utils/fg_color_utils.py::build_instance_colorization) ---
 * uint8 images, integer compares and copies only: the same bytes on every run.  Every access is a byte access, so no pointer but
 * the road test's out needs an alignment.  Returns -1 for sizes out of range or a missing array, -3 for a misaligned out of the
 * road test; nothing is launched then.
 * The mask image (:292-296): small_mask uint8 [bh+1, bw+1] (pred_masks[k], row stride bw + 1) -> out uint8 [bh, bw], one channel:
 * 0 where the mask byte equals 1, 255 for every other value.  The mask's last row and column lie outside the box slice
 * [y1:y2, x1:x2] and are not read.  (bh + 1) * (bw + 1) <= 2^24.  ssc_resample_u8 with chan = 0 replicates the channel. */
int ssc_fg_scene_mask_u8(const uint8_t* small_mask, int bh, int bw, uint8_t* out, void* stream);
/* is_road_not_single_line (:80-134) on the instance sketch uint8 [S,S,3], a grey image.  s = (red byte < 235), which is what the
 * reference's two binarisation steps leave of a grey image.  A run end of column j: s[i][j] && !s[i+1][j] for i < S-1, and
 * s[S-1][j]; the column is valid when it has a positive, even number of them; V = valid columns, Hc = valid rows.  out int32 [3]
 * = {V >= parallel_width || Hc >= parallel_width, V, Hc} in device memory.  One workgroup, integer sums.  1 <= S <= 4096,
 * parallel_width >= 1 (the reference's default: 25). */
int ssc_road_parallel_u8(const uint8_t* sketch, int S, int parallel_width, int32_t* out, void* stream);
/* The paste (:342-345), in place: for i < bh, j < bw, where inner[y1+i][x1+j] == value, result[y1+i][x1+j] = inst[i][j].  result
 * uint8 [H,W,3], inner uint8 [H,W], inst uint8 [bh,bw,3] contiguous, value = instance index + 1.  Nothing else is written.
 * -1 as well for a box that leaves the image (y1, x1 < 0, y1 + bh > H, x1 + bw > W), bh < 1, bw < 1, value outside 1..255,
 * H * W > 2^24. */
int ssc_fg_scene_paste_u8(uint8_t* result, const uint8_t* inner, int H, int W, const uint8_t* inst, int y1, int x1, int bh, int bw,
                          int value, void* stream);
/* PIL.Image.resize of an 8-bit image on the device (resize_and_padding_mask_image, input_pipeline.py:199-239: ANTIALIAS =
 * LANCZOS; reverse_resize_image, Pipeline_utils/fg_color_utils.py:137-160: scipy.misc.imresize = PIL bilinear): Pillow's
 * two-pass 8-bit resampler, horizontal then vertical, bit for bit.  src uint8 [H,W,C]; chan >= 0: only that channel,
 * replicated over the OC channels of dst; chan < 0: all C channels (OC == C).  bnd_* [new][2] = {first tap, taps}, k_* [new][ks]
 * 22-bit fixed-point coefficients (host: obj_lib/input_pipeline.py::resample_coeffs); NULL tables = that axis keeps its size.
 * The result fills [top, top+new_h) x [left, left+new_w) of dst uint8 [OH,OW,OC], the rest of dst is `fill`.
 * tmp: H * new_w * (chan >= 0 ? 1 : C) bytes. */
int ssc_resample_u8(const uint8_t* src, int H, int W, int C, int chan, const int32_t* bnd_h, const int32_t* k_h, int ks_h,
                    int new_w, const int32_t* bnd_v, const int32_t* k_v, int ks_v, int new_h, uint8_t* tmp, uint8_t* dst,
                    int OH, int OW, int OC, int top, int left, int fill, void* stream);
/* Training-queue decode (get_paired_input, input_pipeline.py:77-131) of N raw records: img / sk uint8 [N,R,R,3] ->
 * img_out / sk_out float NCHW [N,3,size,size], R = f * size.  Image: pixel (f*y, f*x) (TF1 bilinear at an integer
 * factor), (v - min)/(max - min + 1) over the resized image, + noise [N,size,size,3] (uniform [0,1/256), may be NULL),
 * * 2 - 1.  Sketch: mean of the f x f block (TF1 area), / 255 * 2 - 1; read from sk_f32 [N,R,R,3] instead of sk when
 * that is not NULL (distance maps).  mnmx: [N,2] scratch (per-image min, max). */
int ssc_decode_paired_u8(const uint8_t* img, const uint8_t* sk, const float* sk_f32, int N, int R, int size,
                         const float* noise, float* img_out, float* sk_out, float* mnmx, void* stream);
/* The first half of ssc_decode_paired_u8 alone: mnmx [N,2] = the minimum and maximum of each image of img uint8 [N,R,R,3]
 * resized to size x size (its pixels (f*y, f*x)).  Exact; the record cache computes it once per record.
 * Returns -1 for sizes out of range (R % size != 0, N < 0); N == 0 returns 0. */
int ssc_decode_minmax_u8(const uint8_t* img, int N, int R, int size, float* mnmx, void* stream);
/* ssc_decode_paired_u8 for N samples gathered from a device-resident record cache, in one launch: img_cache / sk_cache uint8
 * [S,R,R,3], skf_cache float [S,R,R,3] = the cached distance maps (when it is not NULL, sk_cache may be NULL), mnmx_cache float
 * [S,2] from ssc_decode_minmax_u8 at the same size, idx int32 [N] (device memory, read by the kernel: the host does not wait).
 * Output n is bit for bit what ssc_decode_paired_u8 writes for record idx[n] with noise [N,size,size,3] (may be NULL).
 * sk_out == NULL: the sketch is neither read nor written.  An idx[n] outside [0,S) reads nothing and makes the outputs of
 * sample n NaN.  No scratch.  Returns -1 for sizes out of range (R % size != 0, N < 0, S <= 0 or S >= 2^31), -2 for sk_out
 * without a sketch cache; N == 0 returns 0. */
int ssc_decode_paired_cached_u8(const uint8_t* img_cache, const uint8_t* sk_cache, const float* skf_cache,
                                const float* mnmx_cache, int64_t S, const int32_t* idx, int N, int R, int size,
                                const float* noise, float* img_out, float* sk_out, void* stream);
/* --distance_map 1 (input_pipeline.py:86-96): sk uint8 [N,R,R,3] -> out float [N,R,R,3] = exact Euclidean distance of
 * every voxel to the nearest stroke voxel (sk < 250; scipy.ndimage.distance_transform_edt over [R,R,3]) / max * 255.
 * Pass it to ssc_decode_paired_u8 as sk_f32 (then sk may be NULL).  ws: (2*N*R*R*3 + N) int32 of scratch. */
int ssc_distance_map_u8(const uint8_t* sk, int N, int R, float* out, int32_t* ws, int64_t ws_bytes, void* stream);
/* host-side CRC-32C (Castagnoli) of n bytes: TFRecord record framing (tf.TFRecordReader, input_pipeline.py:57-59) */
uint32_t ssc_crc32c(const uint8_t* data, int64_t n);
int ssc_fill(float* dst, float value, int64_t n, void* stream);
/* profiling aid: *dst = the device's 100 MHz wall clock at the time the launch runs (a one-lane kernel; capturable) */
int ssc_timestamp(uint64_t* dst, void* stream);
/* ---- MRU blocks (mru.py:353-461 mru_conv_block_v3, :527-591 mru_deconv_block_v2), NHWC fp32 -------------------- */
/* mean_pool (mru.py:15-19): out[n, y, x, c] = mean of the 2x2 block */
int ssc_mean_pool2(const float* x, int ldx, float* out, int ldo, int N, int H, int W, int C, void* stream);
/* conditional batch norm (models_collection.py:22-35): stats = [mean(C); rstd(C)] (ssc_bn_stats), scale_m/offset_m
 * [n_labels, C]; abn[n] = [a(C); b(C)] with a = scale[label_n]*rstd, b = offset[label_n] - mean*a */
int ssc_cbn_fold(const float* stats, const float* scale_m, const float* offset_m, const int32_t* labels, int N, int C,
                 float* abn, void* stream);
/* the fold of per-split rows [N][nsplit][2][C] (min row, max row) to mnmx [N][2][C] */
int ssc_minmax_finalize(const float* part, int nsplit, int N, int C, float* mnmx, void* stream);
/* ssc_conv_forward + ssc_minmax_hw of its output (the MRU gates: conv + bias + lrelu, then reduce_min / reduce_max over the
 * positions of every sample and channel, mru.py:407-415): when the launch qualifies (uniform-tap kernel, whole tiles finished
 * in one workgroup, a sample's positions a multiple of the tile's rows) the per-tile minima / maxima come out of the conv
 * epilogue and only the fold remains; otherwise the output is read back once. */
int ssc_conv_forward_minmax(const ssc_conv_desc* d, float* ws, int64_t ws_bytes, float* mnmx, void* stream);
/* mnmx[n] = [min(C); max(C)] over the P = H*W rows of sample n (tf.reduce_min/max(axis=[2,3]), mru.py:414-415) */
int ssc_minmax_hw(const float* x, int ld, int N, int P, int C, float* mnmx, float* workspace, int64_t workspace_bytes,
                  void* stream);
/* channel-concat writer: out[row, :] = [part0 | part1 | part2], each part = act(a*x+b) (per-sample a,b when
 * ab_sample_stride != 0), optionally read through a nearest 2x upsample (mru.py:22-28) and multiplied by a min-max
 * normalised gate (rg * ht, mru.py:571) */
typedef struct {
    const float* x;
    const float* ab;      /* NULL or [a(C); b(C)] (+ n*ab_sample_stride) */
    const float* gate;    /* NULL or raw gate [N,H,W,C] */
    const float* mnmx;    /* [N,2,C] when gate != NULL */
    int32_t ld, C, ab_sample_stride, act, upsample, _pad;
} ssc_cat_part;
typedef struct {
    ssc_cat_part p[3];
    float* out;
    int32_t nparts, ldo, N, H, W, _pad;
} ssc_cat_desc;
int ssc_concat_parts(const ssc_cat_desc* d, void* stream);
/* out = ht + (rg - min)/(max - min) * img      (mru.py:422) */
int ssc_mru_gate_merge(const float* ht, const float* rg, const float* mnmx, const float* img, float* out, int N,
                       int64_t P, int C, void* stream);
/* out = hp*(1 - z) + miu(a2*h2+b2)*z, z = (zg - min)/(max - min), hp = ht_ab ? miu(a*ht+b) : ht, ht read at
 * (y/2, x/2) when ht_lowres      (mru.py:583-589) */
/* ---- their backward passes ---- */
/* out[c] (+)= sum_r x[r, c]: bias gradients */
int ssc_colsum(const float* x, int ld, int64_t M, int C, float* out, int accumulate, float* workspace,
               int64_t workspace_bytes, void* stream);
/* dst[r, 0:C] (+)= src[r, 0:C] with independent row strides (splitting a concat gradient) */
int ssc_strided_copy(const float* src, int lds, float* dst, int ldd, int64_t M, int C, int accumulate, void* stream);
/* out (+)= scale * (sum of each 2x2 block): gradient of the nearest upsample (scale 1) / forward mean_pool (0.25) */
int ssc_pool2(const float* x, int ldx, float* out, int ldo, int N, int H, int W, int C, float scale, int accumulate,
              void* stream);
/* backward of y = act(cond_batchnorm(x)) (act = SSC_ACT_MIU or NONE): dx (+)= ..., table gradients
 * dscale_m/doffset_m [n_labels, C] (may be NULL).  gy rows have stride ldg (a channel slice of a concat gradient). */
int ssc_cbn_act_backward(const float* x, const float* abn, const float* stats, const float* scale_m,
                         const int32_t* labels, int n_labels, const float* gy, int ldg, int act, int N, int P, int C,
                         float* dx, int lddx, int accumulate_dx, float* dscale_m, float* doffset_m,
                         int accumulate_params, float* workspace, int64_t workspace_bytes, void* stream);
/* backward of prelu: dx (+)= gy * (leak*x >= x ? leak : 1) (dx may be NULL), dleak (+)= sum gy*x over that set */
int ssc_prelu_backward(const float* x, int ldx, const float* leak, const float* gy, int ldg, int64_t M, int C, float* dx,
                       int lddx, int accumulate_dx, float* dleak, int accumulate_leak, float* workspace,
                       int64_t workspace_bytes, void* stream);
/* backward of r = (g - min)/(max - min) with g = lrelu(pre) stored: dpre from gr = d loss / d r (TF tie rule) */
int ssc_minmax_gate_backward(const float* g, const float* mnmx, const float* gr, int N, int P, int C, float* dpre,
                             float* workspace, int64_t workspace_bytes, void* stream);
/* ht_plus = ht + r*img: gr = g*img, gimg = g*r */
int ssc_mru_gate_merge_backward(const float* ghtp, const float* rg, const float* mnmx, const float* img, float* gr,
                                float* gimg, int N, int64_t P, int C, void* stream);
/* out = hp*(1-z) + h*z: ghp = g*(1-z), gh = g*z, gz = g*(h - hp) (arguments as ssc_mru_blend) */
int ssc_mru_blend_backward(const float* gout, const float* ht, const float* ht_ab, int ht_lowres, const float* h2,
                           const float* h2_ab, const float* zg, const float* mnmx, float* ghp, float* gh, float* gz,
                           int N, int H, int W, int C, void* stream);
/* G[:, 0:C] = d loss / d (r * up(ht)): gr = G*up(ht); G[:, 0:C] <- G*r in place */
int ssc_mru_in2_gate_backward(float* G, int ldG, const float* rg, const float* mnmx, const float* ht_low, float* gr,
                              int N, int H, int W, int C, void* stream);
int ssc_mru_blend(const float* ht, const float* ht_ab, int ht_lowres, const float* h2, const float* h2_ab,
                  const float* zg, const float* mnmx, float* out, int N, int H, int W, int C, void* stream);

/* out[r, c] = act(ab[c]*x[r, c] + ab[ldab + c])  (ab may be NULL): materialises a normalised tensor (final
 * tanh(batchnorm(.)), models_collection.py:664-667) or re-strides a channel-padded one (ldx != ldo) */
int ssc_affine_act(const float* x, int ldx, const float* ab, int ldab, int act, float* out, int ldo, int64_t M, int C,
                   void* stream);
/* bottleneck_residual_{en,de,pu} 'block_add' (residual_util.py:103-109, 138-146, 165-167):
 * out = act(a1*x1+b1 + (ab2 ? a2*x2+b2 : x2)) */
int ssc_residual_merge(const float* x1, const float* ab1, const float* x2, const float* ab2, int act, float* out,
                       int64_t M, int C, void* stream);

/* --- batch-statistics norm (tf.nn.moments + tf.nn.batch_normalization,
 *     models_collection.py:36-46) --- */
/* per-channel mean/biased var over M rows of x[M,ldx] (C channels) folded with
 * scale/offset into ab=[a;b] (y = a*x+b); stats = [mean; rstd].  ws >= nblk*2*C floats. */
int ssc_bn_stats(const float* x, int64_t M, int C, int ldx, const float* scale, const float* offset,
                 float eps, float* ab, float* stats, float* ws, int64_t ws_bytes, void* stream);
/* the second half of ssc_bn_stats: partial [nblk][2][C] column sums / sums of squares over M rows -> ab, stats */
int ssc_bn_finalize(const float* partial, int nblk, int C, int64_t M, const float* scale, const float* offset, float eps,
                    float* ab, float* stats, void* stream);
/*
 * Backward of y = act(a*x+b) for up to two consumers (g1 through act1, g2
 * through act2):  dz = g1*act1'(z) + g2*act2'(z).
 * has_bn=1: dx = a*(dz - mean(dz) - xhat*mean(dz*xhat)), dscale = sum(dz*xhat),
 * doffset = sum(dz).  has_bn=0: dx = dz (ab/stats ignored, z = x).
 */
int ssc_bn_act_backward(const float* x, int64_t M, int C, int ldx, const float* ab, const float* stats,
                        const float* scale, const float* g1, int ldg1, int act1, const float* g2, int ldg2,
                        int act2, int has_bn, float* dx, int lddx, float* dscale, float* doffset, float* ws,
                        int64_t ws_bytes, void* stream);
/*
 * The same with the two per-channel sums taken elsewhere: `pre` = nrows rows [2][C] of partial sums
 * [sum dz | sum dz*xhat] written by the epilogues of the launches that produced g1 (and g2) -- see
 * ssc_conv_forward_bnbwd; pre = NULL: as ssc_bn_act_backward.  Saves the pass over x, g1, g2 of
 * the gradient chain generate_pix2pix -> batchnorm -> lrelu/relu (models_collection.py:36-46, 434-439).
 * rowb != NULL (only with pre == NULL): g1[r][c] += rowb[r / rowb_P][c] * rowb_scale on the fly -- the gradient of the
 * discriminator's class head through its spatial mean (models_collection.py:836-840), one row per image.
 */
int ssc_bn_act_backward_pre(const float* x, int64_t M, int C, int ldx, const float* ab, const float* stats,
                            const float* g1, int ldg1, int act1, const float* g2, int ldg2, int act2, int has_bn,
                            float* dx, int lddx, float* dscale, float* doffset, const float* pre, int nrows,
                            const float* rowb, float rowb_scale, int rowb_P, float* ws, int64_t ws_bytes, void* stream);
/*
 * The norm backward in two steps (sums, streaming apply pass).  `job` describes the site exactly
 * as the arguments of ssc_bn_act_backward_pre do (host memory, read during the call).
 *   ssc_bn_bwd_sums     partial sums (from `pre` / nrows when given, else a pass over x, g1, g2) -> coef [2][C] = mean dz,
 *                       mean dz*xhat, and the scale / offset gradients.  coef is the caller's buffer: it must stay untouched
 *                       until the apply pass has run (the workspace is not a place for it).
 *   ssc_bn_bwd_apply    dx = a*(dz - coef0 - xhat*coef1) (has_bn) or dx = dz, as a launch of its own.
 * Same bits as ssc_bn_act_backward_pre.  (Round 4's ssc_conv_wgrad_hosting, the apply pass inside the filter-gradient launch of
 * the layer above, measured slower in the step and was removed in round 5.)
 */
typedef struct ssc_bn_apply_job {
    const float* x;       /* the normed tensor (raw), [M][ldx] */
    int64_t M;
    int32_t C, ldx;
    const float* ab;      /* [2][C] folded norm (has_bn) */
    const float* stats;   /* [2][C] mean, 1/std (has_bn) */
    const float* g1;      /* gradient w.r.t. act1(z) */
    const float* g2;      /* second consumer's gradient (through act2) or NULL */
    int32_t ldg1, act1, ldg2, act2;
    int32_t has_bn;       /* 0: dx = dz (activation only) */
    int32_t rowb_P;       /* with rowb: g1[r] += rowb[r / rowb_P] * rowb_scale */
    const float* rowb;
    float rowb_scale;
    int32_t lddx;
    const float* coef;    /* [2][C], written by ssc_bn_bwd_sums (has_bn) */
    float* dx;            /* [M][lddx] */
} ssc_bn_apply_job;
int ssc_bn_bwd_sums(const ssc_bn_apply_job* job, const float* pre, int nrows, float* coef, float* dscale, float* doffset,
                    float* ws, int64_t ws_bytes, void* stream);
int ssc_bn_bwd_apply(const ssc_bn_apply_job* job, void* stream);
/*
 * Backward through the output of a bottleneck block, out = act(norm_A(xa) + shortcut) (residual_util.py:103-109, 138-146,
 * 165-167): dz = g * act'(out) and, with that one dz, the backward of block_3's norm (site A: dxa, scale / offset gradients)
 * and -- en / de blocks, xb != NULL -- of the projection shortcut's norm (site B).  Three launches for what is an activation
 * pass + two ssc_bn_act_backward otherwise.  dz_out != NULL: dz is also written (the identity shortcut of a pu block needs
 * it).  All tensors dense [M][C]; coef: [3][C] scratch of the caller.
 */
int ssc_block_out_backward(const float* out, const float* g, int64_t M, int C, int act, const float* xa, const float* aba,
                           const float* sta, const float* xb, const float* abb, const float* stb, float* dz_out, float* dxa,
                           float* dxb, float* dscale_a, float* doffset_a, float* dscale_b, float* doffset_b, float* coef,
                           float* ws, int64_t ws_bytes, void* stream);
/*
 * ssc_conv_forward for a launch whose output g is the gradient w.r.t. act(a*x+b) of a batch-statistics-normed
 * tensor x ([rows][ldx], addressed like the output): when the launch qualifies (uniform-tap kernel, no split-K
 * slabs, whole 16-byte aligned rows) its epilogue also writes rows of `partial` ([2][Nstore] each: sum dz,
 * sum dz*xhat with dz = g*act'(a*x+b)) and *nrows is their count; else *nrows = 0 (take the sums with
 * ssc_bn_act_backward).  partial_bytes >= nphase * ceil(M / 64) * 2 * Nstore * 4 always suffices.
 */
int ssc_conv_forward_bnbwd(const ssc_conv_desc* d, float* ws, int64_t ws_bytes, const float* x, int ldx,
                           const float* ab, const float* stats, int act, float* partial, int64_t partial_bytes,
                           int* nrows, void* stream);

/*
 * The same for a launch whose output columns are the gradients w.r.t. TWO normed tensors side by side: columns [0, C0) belong to
 * x0 ([rows][ldx0], C0 channels), columns [C0, Nstore) to x1.  C0 must be a multiple of 128 (a column tile never straddles the
 * two).  Each tensor gets its own rows of partial sums ([2][C0] / [2][Nstore - C0] each); *nrows is the row count of either
 * (0: the launch did not qualify, take the sums with ssc_bn_act_backward).
 */
typedef struct ssc_bnbwd_site {
    const float* x;       /* the normed tensor (raw values), rows addressed like the launch's output */
    const float* ab;      /* [2][C]: a, b */
    const float* stats;   /* [2][C]: mean, 1/std */
    float* partial;       /* rows of [2][C] sums */
    int64_t partial_bytes;
    int32_t ldx;
    int32_t act;          /* SSC_ACT_* of the consumer whose gradient the columns are */
} ssc_bnbwd_site;
int ssc_conv_forward_bnbwd2(const ssc_conv_desc* d, float* ws, int64_t ws_bytes, const ssc_bnbwd_site* site0,
                            const ssc_bnbwd_site* site1, int C0, int* nrows, void* stream);

/* --- caption branch (text_lstm.hip): encode_feat_with_text, models_collection.py:150-248 --- */
/* tf.nn.embedding_lookup (:182) and its (dense) gradient; tok rows are time-major [T*N] */
int ssc_embedding_gather(const float* table, const int* tok, int rows, int C, float* out, void* stream);
int ssc_embedding_scatter_add(float* dtable, int vocab, const int* tok, int rows, int C, const float* g, void* stream);
/* tf.nn.l2_normalize over channels (:202,216); z = a*x+b when ab != NULL; ss[row] = sum z^2 */
int ssc_row_l2norm_fwd(const float* x, int ldx, const float* ab, int64_t M, int C, float* y, float* ss, void* stream);
int ssc_row_l2norm_bwd(const float* y, const float* ss, const float* dy, int64_t M, int C, float* dz, int accumulate,
                       void* stream);
/* BasicLSTMCell gate math (state_is_tuple=False, forget_bias=1) with the tf.cond pad-token skip (:235).
 * gates[row] = g0[row] + g1[row] + g2[row/div2]; acts = activated i,j,f,o kept for the backward pass. */
int ssc_lstm_pointwise_fwd(const float* g0, const float* g1, const float* g2, int div2, const int* mask, int mdiv,
                           const float* c_in, const float* h_in, int64_t rows, int C, float* c_out, float* h_out,
                           float* acts, void* stream);
/* One recurrent step in one launch: gates = h_in @ Kh (Kh: [C rows][4C], row stride ldk; skipped when with_gemm == 0,
 * i.e. h_in = 0) + g1[row] + g2[row/div2], then the cell above (tf.matmul + BasicLSTMCell of models_collection.py:230-236). */
int ssc_lstm_step_fwd(const float* h_in, const float* Kh, int ldk, const float* g1, const float* g2, int div2,
                      const int* mask, int mdiv, const float* c_in, int64_t rows, int C, int with_gemm, float* c_out,
                      float* h_out, float* acts, void* stream);
/* The same step on the bf16 matrix pipe, six bf16 products per fp32 product (fp32-grade results); C % 128 == 0.
 * Kp = the planes of Kh [C, 4C] from ssc_filter_split(Kh, 1, C, 4 * C, 0, ...), nbp = their blocks per plane
 * (ssc_filter_split_geom).  hp_in = the bf16 planes of h_in in the A-operand fragment layout (ssc_lstm_hsplit, or the previous
 * step's hp_out: ceil(rows / 64) * 2 * (C / 16) * 3 KiB -- whole 64-row tiles); NULL = h_in is zero, no product (with_gemm = 0 above).  hp_out (may be
 * NULL) receives the planes of h_out; acts may be NULL (inference: nobody reads the activated gates). */
int ssc_lstm_step_fwd_bf(const float* h_in, const void* hp_in, const void* Kp, int nbp, const float* g1, const float* g2,
                         int div2, const int* mask, int mdiv, const float* c_in, int64_t rows, int C, float* c_out,
                         float* h_out, void* hp_out, float* acts, void* stream);
int ssc_lstm_hsplit(const float* h, int64_t rows, int C, void* hp, void* stream);
int ssc_lstm_pointwise_bwd(const float* dh, const float* dc, const float* acts, const float* c_in, const float* c_out,
                           const int* mask, int mdiv, int64_t rows, int C, float* dg, float* dc_in, float* dh_pass,
                           float* gacc, void* stream);
/* relu(0.5*(log(1+1e-3+h) - log(1+1e-3-h)))  (:238-242) */
int ssc_squash_fwd(const float* h, int64_t n, float* o, void* stream);
int ssc_squash_bwd(const float* h, const float* o, const float* go, int64_t n, float* dh, void* stream);
/* out[g][c] (+)= sum of G consecutive rows (bias gradients, 6x6 tile reduction) */
int ssc_group_rowsum(const float* x, int ldx, int64_t groups, int G, int C, float* out, int accumulate, void* stream);
/* tf.reduce_mean over H,W of act(a*x+b) (:838) and the broadcast of its gradient */
int ssc_act_mean_hw(const float* x, const float* ab, int act, int N, int P, int C, float* out, void* stream);
int ssc_add_row_bcast(float* g, const float* v, float scale, int N, int P, int C, void* stream);
/* miu_relu (:63-65) fused with the [N,C*P] -> [N,P,C] reshape of the noise head (:493-499) */
int ssc_miu_permute_fwd(const float* pre, int N, int Cc, int P, float* out, void* stream);
int ssc_miu_permute_bwd(const float* pre, const float* g, int N, int Cc, int P, float* dpre, void* stream);

/* --- losses / optimizer (losses_optim.hip): graph_single.py:317-593 ---
 * loss_acc points to a DOUBLE device scalar that the kernels add into (zero it first). */
/* loss_acc += scale*sum softplus(sign*x[r*ld]); grad[r*ld] = gscale*sign*sigmoid(sign*x)   (:401-402) */
int ssc_softplus_loss(const float* x, int ld, int64_t rows, float sign, float scale, double* loss_acc, float* grad,
                      float gscale, void* stream);
/* sparse softmax CE (focal=0) or (1-p_true)^2 * CE (focal=1), mean over N, times coef   (:340-353) */
int ssc_acgan_loss(const float* logits, const int* labels, int N, int K, int focal, float coef, double* loss_acc,
                   float* dlogits, void* stream);
/* smooth-L1(img - gen) mean * coef (:551-555) + incoming discriminator gradient, through tanh' */
int ssc_gen_output_grad(const float* gen, int ldg, const float* img, int ldi, const float* gd, int ldd, int64_t npix,
                        float coef, double* loss_acc, float* dpre, void* stream);
/* ly.l2_regularizer: loss_acc += rate*sum(w^2)/2; grad += rate*w   (mru.py:55,60) */
int ssc_l2_reg(const float* w, int64_t n, float rate, double* loss_acc, float* grad, void* stream);
/* ---- Background_Colorization losses (bg_colorization_main.py:596-627), vanilla GAN on sigmoid(z) ------------------ */
/* mode 0: loss += scale*sum -log(sigmoid(z)+1e-12); mode 1: -log(1-sigmoid(z)+1e-12); dz = gscale * d/dz (may be NULL) */
int ssc_bg_gan_loss(const float* z, int64_t n, int mode, float scale, double* loss_acc, float* dz, float gscale,
                    void* stream);
/* count[0] = #(labels != 0): the pixels the masked L1 averages over (:612-616) */
int ssc_count_nonzero_i32(const int32_t* labels, int64_t n, float* count, float* workspace, int64_t workspace_bytes,
                          void* stream);
/* img = tanh(pre) [M,3]: loss += l1w * mean_{label != 0} |tgt - img|; dpre [M,4] = (dL1 + dgan [M,4]) * (1 - img^2) */
int ssc_bg_output_grad(const float* img, const float* tgt, const int32_t* labels, const float* count, float l1w,
                       const float* dgan, double* loss_acc, float* dpre, int64_t M, void* stream);
/* region-mask loss (:589-591): loss += w * mean softmax-CE(logits [M,K<=4], labels); dlogits [M, ldg] (pad columns 0) */
int ssc_seg_ce_loss(const float* logits, int K, const int32_t* labels, int64_t M, float w, double* loss_acc,
                    float* dlogits, int ldg, void* stream);
/* tf.train.AdamOptimizer dense apply (graph_single.py:588); lr_t = lr*sqrt(1-b2^t)/(1-b1^t) from the host, or read
 * from the device scalar lr_dev when it is not NULL (so a captured hipGraph can be replayed with a new step size) */
int ssc_adam_tf(float* var, const float* grad, float* m, float* v, int64_t n, float lr_t, const float* lr_dev,
                float beta1, float beta2, float eps, float gscale, void* stream);
/* the other optimizers get_optimizer offers (graph_single.py:584-593), TF dense-apply formulas: kind 1 RMSProp
 * (h0 = decay, h1 = momentum, h2 = epsilon; s1 = ms, s2 = mom), 2 Adagrad (s1 = accumulator), 3 Adadelta (h0 = rho,
 * h2 = epsilon; s1 = accum, s2 = accum_update).  lr is read from device memory; grad is scaled by gscale first. */
int ssc_optimizer_step(int kind, float* var, const float* grad, float* s1, float* s2, int64_t n, const float* lr_dev,
                       float h0, float h1, float h2, float gscale, void* stream);
/* spectral_normed_weight, one power iteration (sn.py:12-52) and its full gradient */
int ssc_sn_forward(const float* W, const float* u, int m, int n, float* v, float* u_new, float* wbar, float* aux,
                   void* stream);
int ssc_sn_backward(const float* W, const float* u, const float* v, const float* u_new, const float* aux,
                    const float* G, int m, int n, float* dW, int accumulate, float* scratch, void* stream);
/* the same for weights of any size (every conv / FC weight of the MRU discriminator): multi-workgroup, two-stage
 * fixed-order reductions.  forward workspace >= 64*n floats; backward workspace >= 1024+n floats, scratch m floats */
int ssc_sn_forward_any(const float* W, const float* u, int m, int n, float* v, float* u_new, float* wbar, float* aux,
                       float* workspace, int64_t workspace_bytes, void* stream);
int ssc_sn_backward_any(const float* W, const float* u, const float* v, const float* u_new, const float* aux,
                        const float* G, int m, int n, float* dW, int accumulate, float* scratch, float* workspace,
                        int64_t workspace_bytes, void* stream);
int ssc_axpy(float* y, const float* x, float a, int64_t n, void* stream);
/* fully_connected with <= 64 outputs (class logits, models_collection.py:839): y = x W + b, and its gradients */
int ssc_fc_small_fwd(const float* x, const float* W, const float* b, int N, int K, int J, float* y, void* stream);
int ssc_fc_small_bwd(const float* x, const float* W, const float* dy, int N, int K, int J, float* dx, float* dW,
                     float* db, int accumulate, void* stream);

/* --- instance matcher (matching.hip): Instance_Matching/RMI_model.py in eval mode on deeplab_model.py, and
 *     Pipeline_utils/fg_matching_utils.py::build_instance_matching; DESIGN.md section 8.6 --- */
/* src uint8 [H,W,3] -> out float [H,W,4] = (byte - (104.00698793, 116.66876762, 122.67891434), 0), the means taken off the
 * channels in RGB order as the reference does; stroke uint8 [H,W] = 1 where the first byte is not 255 */
int ssc_match_preprocess_u8(const uint8_t* src, int H, int W, float* out, uint8_t* stroke, void* stream);
/* tf.nn.max_pool(3x3, stride 2, SAME) of relu(ab[c]*x + ab[C+c]), NHWC, C % 4 == 0: out [N, ceil(H/2), ceil(W/2), C].  Taps in
 * the padding do not take part.  ab == NULL: the plain max-pool of x (no relu). */
int ssc_max_pool3s2(const float* x, const float* ab, int N, int H, int W, int C, float* out, void* stream);
/* x [N,H,W,C] -> out [N*r*r, H/r, W/r, C]: sub-image n*r*r + i*r + j holds the pixels (y % r == i, x % r == j) of image n;
 * r = 2 or 4, H and W multiples of r, C % 4 == 0.  A rate-r 3x3 SAME conv of x is the plain 3x3 SAME conv of out. */
int ssc_space_to_batch(const float* x, int N, int H, int W, int C, int r, float* out, void* stream);
/* the way back: x [N*r*r, H/r, W/r, C] -> out [N,H,W,C] */
int ssc_batch_to_space(const float* x, int N, int H, int W, int C, int r, float* out, void* stream);
/* out[row] = sum_c relu(0.5*(log(1+1e-3+h[row*ldh+c]) - log(1+1e-3-h[row*ldh+c]))) * w[c] + bias[0]: ssc_squash_fwd and the
 * 1x1 conv to one channel in one pass; one wavefront per row, fixed summation order.  C % 4 == 0, ldh % 4 == 0 */
int ssc_squash_project(const float* h, int ldh, const float* w, const float* bias, int64_t rows, int C, float* out,
                       void* stream);
/* up [S,S] = tf.image.resize_bilinear(pred [h,w], [S,S]) (legacy form, align_corners = False: src = dst * (in / out));
 * predicts uint8 [S,S] = (up >= 1e-9) && stroke != 0.  S % 4 == 0 */
int ssc_match_finish(const float* pred, int h, int w, const uint8_t* stroke, int S, float* up, uint8_t* predicts,
                     void* stream);
/* out int64 [N,2]: per instance {#(predicts != 0 && mask != 0), sum of the mask's bytes} over its box; boxes int32 [N,4] =
 * (y1, x1, y2, x2), both ends included; the mask of instance k is masks[offsets[k] ..], (y2-y1+1) x (x2-x1+1) bytes.  A box that
 * is empty or leaves the S x S image, or a mask that leaves the mask_bytes of the buffer, gives {-1, -1}. */
int ssc_instance_occupancy(const uint8_t* predicts, int S, const uint8_t* masks, int64_t mask_bytes, const int32_t* boxes,
                           const int64_t* offsets, int N, int64_t* out, void* stream);

/* --- the matcher's evaluation (match_eval.hip): Instance_Matching/matching_main.py --mode eval; DESIGN.md section 8.7 --- */
/* out int64 [256]: out[g] = #{p < n : labels[p] == g && (gate == NULL || gate[p] != 0)}.  The entry point zeroes out on the
 * stream; every workgroup keeps 256 bins in LDS and adds its non-empty ones to out as 64-bit integers: the same bits on every
 * run.  16-byte loads where the addresses allow them (any alignment of labels and gate is taken), 1 <= n <= 2^24 */
int ssc_label_hist_u8(const uint8_t* labels, const uint8_t* gate, int64_t n, int64_t* out, void* stream);
/* out int64 [N,256]: out[k][g] = #{pixels of instance k's box with mask byte != 0 && labels == g}; labels uint8 [S,S]; boxes,
 * offsets and masks as for ssc_instance_occupancy (both ends of a box included; boxes may overlap).  A box that is empty or
 * leaves the S x S image, or a mask that leaves the mask_bytes of the buffer, gives a row of -1. */
int ssc_instance_label_hist(const uint8_t* labels, int S, const uint8_t* masks, int64_t mask_bytes, const int32_t* boxes,
                            const int64_t* offsets, int N, int64_t* out, void* stream);

/* --- training the matcher's fusion head (match_train.hip): RMI_model.py::train_op, utils/loss.py; DESIGN.md section 8.8 --- */
/* The class loss on the up-sampled logits and its gradient on the head's map.  pred float [h,w]; S = k*h = k*w; up = the legacy
 * bilinear up-sampling ssc_match_finish computes; a pixel p is live when sketch[3p] <= 104 (sketch uint8 [S,S,3]); its target is
 * z = lut[labels[p]] != 0 (labels uint8 [S,S], lut uint8 [256]).  loss_acc += sum over the live pixels of max(u,0) - u*z +
 * log1p(exp(-|u|)) (fp32 terms, added in double); live[0] = their number; dpred[i][j] = sum over the live pixels of
 * (sigmoid(u) - z) * (the weight of pred[i][j] in that pixel's interpolation).  A gather, one workgroup per cell; fixed-order sums,
 * the same bits on every run.  ws: 16 bytes per cell of pred.  -1 for sizes that do not fit or too small a workspace */
int ssc_match_loss_grad(const float* pred, int h, int w, const uint8_t* sketch, const uint8_t* labels, const uint8_t* lut, int S,
                        double* loss_acc, int64_t* live, float* dpred, float* ws, int64_t ws_bytes, void* stream);
/* The backward of ssc_squash_project: with s = 0.5*(log(1.001+v) - log(1.001-v)), v = hh[r*ldh+c]:
 * dh[r][c] = s > 0 ? dpred[r]*w[c]*0.5*(1/(1.001+v) + 1/(1.001-v)) : 0 (columns C .. ldh-1: 0); dw[c] = sum_r dpred[r]*max(s,0);
 * db[0] = sum_r dpred[r].  The sums in two stages of a fixed order through ws: ceil(rows / max(16, ceil(rows / 64))) * (C + 1)
 * floats.  C % 4 == 0, ldh % 4 == 0 */
int ssc_squash_project_bwd(const float* hh, int ldh, const float* w, const float* dpred, int64_t rows, int C, float* dh, float* dw,
                           float* db, float* ws, int64_t ws_bytes, void* stream);

/* --- scoring a held-out caption while the matcher trains (match_val.hip): match_validation.py; DESIGN.md section 8.9 --- */
/* One pass over the S x S pixels from pred float [h,w]; neither up nor predicts is written.  With u = the value ssc_match_finish
 * computes for the pixel p (the same inline function: the same bits), b = sketch[3p] (sketch uint8 [S,S,3]) and
 * z = lut[labels[p]] != 0 (labels uint8 [S,S], lut uint8 [256]), out is five 8-byte slots:
 *   out[0] (a double)  sum over the pixels with b <= 104 of max(u,0) - u*z + log1p(exp(-|u|)): ssc_match_loss_grad's fp32 terms,
 *                      added in double
 *   out[1 .. 4] (int64, stored through the same pointer)  I = #{u >= 1e-9f && b != 255 && z}, P = #{u >= 1e-9f && b != 255},
 *                      A = #{z}, live = #{b <= 104};  the union of compute_mask_IU is P + A - I
 * A thread owns four neighbouring pixels of a row; 4-byte loads of sketch and labels when both start on a 4-byte boundary, byte
 * loads for any other base.  Fixed-order sums (lanes, wavefronts, then a second launch of one workgroup over the workgroups'
 * partial rows in ws), no float atomic, a grid that depends on S alone: the same bits on every run.
 * ws: 40 bytes per workgroup of the first launch, min(2048, ceil(S*S/4 / 256)) of them (40 bytes at S = 24, 160 at 64, 23040 at 768).
 * The domain is ssc_match_finish's (S % 4 == 0, S*S <= 2^24, 1 <= h, w <= S): -1 outside it, for a NULL pointer and for a
 * workspace that is too small; -3 for out or ws off an 8-byte boundary (or pred off a 4-byte one) */
int ssc_match_score(const float* pred, int h, int w, const uint8_t* sketch, const uint8_t* labels, const uint8_t* lut, int S,
                    double* out /* [5] */, float* ws, int64_t ws_bytes, void* stream);

/* --- the backward of the matcher's backbone (match_backbone_train.hip).  Its norms are frozen
 * (deeplab_model.py:176-231), so relu(a*r + b) goes backward without statistics.  NHWC floats, C a multiple of 4, every pointer
 * on a 16-byte boundary (-3), at most 2^33 - 4 floats per tensor; -1 for any other bad argument, nothing is launched then.  At an
 * activation of exactly 0 the mask is 0.  No atomics: the same bits on every run. */
/* dr[p, c] = g[p, c] * a[c] * (a[c]*r[p, c] + b[c] > 0), ab = [a | b] of 2C floats, M pixels.  dr may be g, never r. */
int ssc_frozen_act_bwd(const float* g, const float* r, const float* ab, int64_t M, int C, float* dr, void* stream);
/* the backward of ssc_residual_merge(r3, ab3, x2, ab_add, relu) from its output: m = out > 0, dr3 = g*m*a3, and
 * d2 = g*m*a_add (ab_add given: the gradient of the projection shortcut's raw output) or g*m (ab_add NULL: the gradient of the
 * identity shortcut).  The four tensors are distinct. */
int ssc_unit_merge_bwd(const float* g, const float* out, const float* ab3, const float* ab_add, int64_t M, int C, float* dr3,
                       float* d2, void* stream);
/* the data gradient of a 1x1 SAME conv of stride 2 from that of the stride-1 conv on its lattice: src [N, h, w, C] ->
 * out [N, H, W, C], h = ceil(H/2), w = ceil(W/2): out[n, 2y, 2x] = src[n, y, x], zero wherever a coordinate is odd */
int ssc_zero_stuff2(const float* src, int N, int h, int w, int C, int H, int W, float* out, void* stream);
/* the backward of ssc_max_pool3s2(r0, ab): g [N, ceil(H/2), ceil(W/2), C] -> dr0 [N, H, W, C].  Gather form: every input pixel
 * looks at the up-to-four windows that hold it; a window's gradient goes to the first of its taps in row-major order that attains
 * its maximum of relu(a*r0 + b), taps in the padding never take part; dr0 = (sum over those windows of g) * a * (a*r0 + b > 0) */
int ssc_max_pool3s2_bwd(const float* g, const float* r0, const float* ab, int N, int H, int W, int C, float* dr0, void* stream);

/* --- the matcher's word attention (match_attn.hip): RMI_model.py:202-217 with use_attn; DESIGN.md section 8.11 --- */
/* attn[t] = softmax over t < T of (t < L ? sum_c hs[t*ld+c]*w[c] : 0) + b[0].  The rows >= L of hs are not read.  One workgroup,
 * fixed summation order.  -1 for L < 1, L > T, T > 64, ld < C */
int ssc_attn_scores_fwd(const float* hs, int ld, const float* w, const float* b, int C, int L, int T, float* attn, void* stream);
/* y[i] = fmaf(s[k], x[i], overwrite ? 0 : y[i]) for i < n: ssc_axpy with the scale read from device memory (s holds ns floats;
 * -1 for k outside of them) */
int ssc_dev_scaled_add(float* y, const float* x, const float* s, int ns, int k, int64_t n, int overwrite, void* stream);
/* dattn[t] = sum_i dacc[i]*H[t*stride+i] for t < L (<= 64), i < n: float64 partial sums in two stages of a fixed order through
 * ws (8-byte aligned, L * min(512, ceil(n / 4096)) doubles), rounded to float once; no atomics */
int ssc_attn_plane_dots(const float* dacc, const float* H, int64_t stride, int64_t n, int L, float* dattn, float* ws,
                        int64_t ws_bytes, void* stream);
/* The backward of ssc_attn_scores_fwd: dlogit[t] = attn[t]*((t < L ? dattn[t] : 0) - sum_{s<L} attn[s]*dattn[s]) for t < T;
 * dw[c] = sum_{t<L} dlogit[t]*hs[t*ld+c]; db[0] = sum_{t<T} dlogit[t] in index order; dhs[t*ldd+c] += dlogit[t]*w[c] for t < L,
 * c < C.  One workgroup; the rows >= L of hs, dattn and dhs are not touched */
int ssc_attn_scores_bwd(const float* attn, const float* dattn, const float* hs, int ld, const float* w, int C, int L, int T,
                        float* dlogit, float* dw, float* db, float* dhs, int ldd, void* stream);

/* --- the matcher's SegNet backbone (match_segnet.hip): Instance_Matching/segnet_model.py with is_intermediate; DESIGN.md
 *     section 8.12.  NHWC floats, C a multiple of 4, float pointers on a 16-byte boundary and code on a 4-byte one (-3); -1 for any
 *     other bad argument, nothing is launched then.  No atomics: the same bits on every run.  Each is the other's backward. --- */
/* tf.nn.max_pool_with_argmax(2x2, stride 2) of relu(ab[c]*x + ab[C+c]) (ab == NULL: of x itself, no relu): x [N,H,W,C], H and W
 * even -> out [N,H/2,W/2,C] and code uint8 of that shape = 2*dy + dx of the first tap in row-major order that attains the maximum
 * (TF's choice; the tie rule of ssc_max_pool3s2_bwd).  TF's flat index of the element is ((2y+dy)*W + 2x+dx)*C + c. */
int ssc_max_pool2_argmax(const float* x, const float* ab, int N, int H, int W, int C, float* out, uint8_t* code, void* stream);
/* segnet_model.py::_unpool_2d: x, code [N,h,w,C] -> out [N,2h,2w,C]; out[n,2y+dy,2x+dx,c] = x[n,y,x,c] where
 * (code[n,y,x,c] & 3) == 2*dy + dx and 0 at the window's three other positions.  Every element of out is written. */
int ssc_unpool2(const float* x, const uint8_t* code, int N, int h, int w, int C, float* out, void* stream);

/* --- the scene session's turn report (scene_system.hip): scene_session.py; DESIGN.md section 8.14 --- */
/* out int64 [256]: out[g] = #{p < H*W : inner[p] == g && the three bytes of prev at 3p differ from those of next in at least one
 * channel}; prev, next uint8 [H,W,3], inner uint8 [H,W].  The entry point zeroes out on the stream; every workgroup keeps 256
 * bins in LDS and adds its non-empty ones to out as 64-bit integers: the same bits on every run.  16-byte loads when the three
 * pointers are on 16-byte boundaries, bytewise ones otherwise.  1 <= H*W <= 2^24; -1 for a null pointer or a bad size, -3 for
 * an out off its 8-byte boundary: nothing is launched then */
int ssc_scene_change_hist_u8(const uint8_t* prev, const uint8_t* next, const uint8_t* inner, int H, int W, int64_t* out,
                             void* stream);

/* --- the preview sheets of the held-out passes (preview.hip): preview.py; DESIGN.md section 8.15 --- */
/* src uint8 [N,H,W,3], sheet uint8 [SH,SW,3]: image n becomes a tile of H/s x W/s pixels whose first pixel is sheet pixel
 * (top + n*pitch, left).  Every byte of a tile is the mean of its s x s source bytes, rounded half up in integers:
 * (sum + s*s/2) / (s*s); s = 1 copies; s = 6 is what a 384-pixel record is reduced by for a 64-pixel generator.  Nothing
 * outside the N tiles is written; integers only: the same bits on every run.
 * 4-byte loads and stores when src and the tile's first byte are on 4-byte boundaries and W and SW are multiples of 4 (then
 * every row is), single bytes otherwise and for the W/s % 4 pixels at the end of a tile row.
 * -1, and nothing is launched: a null pointer; N < 1 (or > 65535); a side outside 1 .. 65536; s not one of 1, 2, 4, 6, 8 or not a
 * divisor of H and of W; a negative top, left or pitch; a tile that leaves the sheet; pitch < H/s with N > 1; src overlapping
 * sheet.  No pointer needs an alignment (the library's -3 does not occur). */
int ssc_sheet_tiles_u8(const uint8_t* src, int N, int H, int W, int s, uint8_t* sheet, int SH, int SW, int top, int left, int pitch,
                       void* stream);
/* One tile from a sketch uint8 [S,S,3] whose pixels are coloured first.  pred uint8 [S,S] or NULL (ssc_match_finish's predicts:
 * a pixel is predicted when its byte is not 0); labels uint8 [S,S] with lut uint8 [256], or both NULL (a pixel is a target when
 * lut[labels[p]] != 0, as in ssc_match_score).  Predicted and target: (0,170,0); predicted only: (230,0,0); target only:
 * (0,90,255); neither: the sketch's three bytes.  With pred NULL a target pixel is (0,170,0), with labels NULL a predicted one.
 * The coloured image is reduced as by ssc_sheet_tiles_u8 (N = 1, H = W = S) into the tile at (top, left).  Refusals as there,
 * also for labels without lut or lut without labels and for pred, labels or lut overlapping sheet. */
int ssc_sheet_overlay_u8(const uint8_t* sketch, const uint8_t* pred, const uint8_t* labels, const uint8_t* lut, int S, int s,
                         uint8_t* sheet, int SH, int SW, int top, int left, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SKETCHYCOLOR_HIP_H */
