/* bodyslam_hip.h -- C ABI of libbodyslam_hip.so (gfx950 / MI355X only).
 *
 * The reference (GuidoManni/BodySLAM) is pure Python with no FFI of its own: every op on its hot
 * path is a PyTorch-CUDA dispatch.  Each entry point below names the reference call it replaces
 * (paths relative to the reference repo; "HF" = transformers 5.15.0, the installed restatement of
 * the un-vendored isl-org/ZoeDepth network the reference pulls through torch.hub at
 * BodySLAM_Refactored/src/depth_estimation/interface.py:46).
 *
 * Conventions: plain pointers are DEVICE pointers unless marked host; `stream` is a hipStream_t
 * passed as void*; every function returns 0 or a negative bs_status and never throws; the library
 * allocates nothing per call (callers own every buffer; bs_init allocates one 4 KiB zero page).
 * INTEGRATION.md shows the ctypes binding a reference maintainer would add.
 */
#ifndef BODYSLAM_HIP_H
#define BODYSLAM_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
    BS_OK = 0,
    BS_ERR_INVALID = -1,   /* bad argument / unsupported shape */
    BS_ERR_HIP = -2,       /* a HIP runtime call failed; see bs_last_error() */
    BS_ERR_NOT_INIT = -3
} bs_status;

enum { BS_F32 = 0, BS_F16 = 1, BS_BF16 = 2, BS_F64 = 3 /* bs_similarity_fit and bs_pc_transform only */ };
/* BS_ACT_SOFTPLUS: torch.nn.Softplus(beta = 1, threshold = 20) through libm (log1pf(expf(x))), what the oracle computes.
 * BS_ACT_SOFTPLUS_FAST: the same function on v_exp / v_log (relative error <= 4e-6): the attractor MLPs only, whose epilogue was bound by
 * libm's arithmetic and whose inputs are 16-bit hidden units anyway; the seed regressors (bin start values) and the reference
 * precision use the exact form. */
enum { BS_ACT_NONE = 0, BS_ACT_RELU = 1, BS_ACT_GELU = 2, BS_ACT_SOFTPLUS = 3, BS_ACT_SOFTPLUS_FAST = 4 };
enum { BS_OUT_PLAIN = 0, BS_OUT_SHUFFLE = 1, BS_OUT_QKV = 2 };

/* library ------------------------------------------------------------------------------------ */
int bs_init(int device);                 /* replaces .to("cuda") at interface.py:49-51, mpem_interface.py:34,60 */
const char* bs_last_error(void);
int bs_version(void);

/* implicit GEMM on MFMA ---------------------------------------------------------------------- *
 * out[m, n] = epilogue( sum_k A(m, k) * W[n, k] ),  A/W fp16 or bf16, fp32 accumulate.
 * Replaces every nn.Linear / nn.Conv2d / nn.ConvTranspose2d(k == stride) on the path:
 *   BEiT q/k/v/o_proj, fc1, fc2           HF modeling_beit.py:296-357
 *   patch embedding Conv16x16 s16         HF modeling_beit.py:63-90
 *   DPT readout / 1x1 / ConvT / 3x3 convs HF modeling_zoedepth.py:55-149,153-329,332-373
 *   metric-head 1x1 convs                 HF modeling_zoedepth.py:494-547,665-772
 *   CyclePose Conv7x7 / Conv3x3 s2        MPEM/architecture_v3.py:120-147
 * conv == 0: A is [M, K] with row stride lda.   conv == 1: A is an NHWC batch [B, Hin, Win, lda>=Cin],
 * K = KH*KW*Cin, M = B*Hout*Wout, zero padding pad_h/pad_w (may be negative: a crop).  K order, conv mode:
 * 64-channel chunk outermost, then the filter tap, then the chunk's channels -- W is [N][Cin/64][KH][KW][64]
 * (bodyslam_amd/_lib.py conv_weight()); this keeps the taps that re-read one input row a few K-steps apart, inside
 * the XCD's L2.  Cin (conv) / K (plain) must be a multiple of 64.
 * epilogue: y = acc + bias[(m / bias_group_rows) * N + n]  (bias_group_rows == 0: bias[n]);
 *           y = act(y); y *= scale[n]; y += res[orow * ldr + n] (orow = m unless regrouped, below); store.
 * out_mode BS_OUT_PLAIN  : out[orow * ldo + n], orow = (m / out_group_rows) * out_group_stride
 *                          + m % out_group_rows + out_row_offset (out_group_rows == 0: orow = m)
 *          BS_OUT_SHUFFLE: ConvTranspose2d(kernel == stride == shuffle_s): n = (ky*s + kx)*Cout + co,
 *                          out is NHWC [B, Hout*s, Wout*s, shuffle_cout]
 *          BS_OUT_QKV    : n = which*hidden + head*64 + d; tokens_per_image rows per image;
 *                          out -> Q [B,nh,Sp,64] (scaled by q_scale), out2 -> K [B,nh,Sp,64],
 *                          out3 -> V^T [B,nh,64,Sp]
 */
/* The (hi16 | hi8 | lo8) operand format of accurate mode's FP8 correction passes: a row of C features is
 * [round16(y) x C | e4m3(y * 2^BS_F8_ACT_HI_EXP) x C | e4m3((y - round16(y)) * 2^BS_F8_ACT_LO_EXP) x C] = 4C bytes.
 * Producers take the flag `| 32` on their dtype argument (bs_layernorm, bs_attention, bs_preprocess_patches; bs_layernorm also
 * `| (rows << 8)`: only rows below `rows` write the planes; bs_attention_table `| 64`: only the cls rows do) or
 * bs_gemm_desc.out_f8; the consumer is bs_gemm with f8_seg = 2C. */
#define BS_F8_ACT_HI_EXP 0
#define BS_F8_ACT_LO_EXP 11
typedef struct bs_gemm_desc {
    const void* A;
    const void* W;
    int32_t dtype;                 /* BS_F16 | BS_BF16 */
    int32_t M, N, K;
    int32_t lda;
    int32_t conv;
    int32_t Hin, Win, Cin, Hout, Wout, KH, KW, stride, pad_h, pad_w;
    int32_t relu_a;                /* ReLU on A while loading (pre-activation residual unit) */
    const float* bias;
    int32_t bias_group_rows;
    int32_t act;
    const float* scale;
    const void* res;
    int32_t res_dtype;             /* BS_F32 | BS_F16 | BS_BF16 */
    int32_t ldr;
    const void* res2;              /* optional second residual, operand dtype, same ldr */
    void* out;
    void* out2;
    void* out3;
    int32_t out_dtype;
    int32_t ldo;
    int32_t out_mode;
    int32_t out_group_rows, out_group_stride, out_row_offset;
    int32_t shuffle_s, shuffle_cout;
    int32_t qkv_hidden, qkv_tokens, qkv_sp;
    float q_scale;
    int32_t tile;                  /* 0 = auto; else forces a tile variant (tests / tuning) */
    /* split-precision support (Numerics).  The K axis may consist of two segments that walk the SAME rows of A:
     * segment 0 (Cin channels per tap for conv, K - seg1 for plain) then segment 1 (seg1 channels per tap / K columns);
     * W holds both segments back to back along K.  With A = [hi | lo] and W = [W_hi | W_hi | W_lo] one launch evaluates
     * A_hi W_hi + A_lo W_hi + A_hi W_lo.  out_split_off > 0 stores the 16-bit output as a (hi, lo) pair, lo at that
     * element offset; res_split_off > 0 reads the 16-bit residual(s) as such pairs. */
    int32_t seg1;
    int32_t out_split_off;
    int32_t res_split_off;
    /* FP8 correction segment (plain GEMMs).  f8_seg > 0: every A row and every W row continues, after its K 16-bit values, with
     * f8_seg bytes of OCP e4m3 values that are multiplied on the block-scaled FP8 MFMA (2x the 16-bit rate).  They come in
     * two halves of f8_seg / 2 (a multiple of 128) each; half h contributes 2^(sa_h - 127 + sb_h - 127) * sum_k A8[k] W8[k].
     * f8_scales packs the four E8M0 exponents: sa0 | sb0 << 8 | sa1 << 16 | sb1 << 24.  With A = [hi16 | hi8 | lo8] and
     * W = [W_hi16 | W_lo8 | W_hi8] this is A_hi W_hi + A_hi W_lo + A_lo W_hi at 2 pass-equivalents instead of 3.
     * Conv mode: the pixel vector is [hi16 x Cin | hi8 x Cin | lo8 x Cin] (f8_seg = 2*Cin, Cin % 128 == 0) and W is
     * [W_hi16: chunk64, tap, 64][W_lo8: chunk128, tap, 128][W_hi8: ...] (bodyslam_amd/_lib.py f8_conv_weight()).
     * out_f8 != 0 (with out_split_off = channels, ldo = 2*channels, channels % 8 == 0): the output row / pixel is written in that A format,
     * [hi16 x N | e4m3(y * 2^ea) x N | e4m3((y - hi) * 2^el) x N], out_f8 = ea | el << 8. */
    int32_t f8_seg;
    uint32_t f8_scales;
    int32_t out_f8;
    int32_t res_f8;                /* != 0: res / res2 are rows in that format too (N channels, ldr >= 2N) */
    int32_t qkv_cls_last;          /* BS_OUT_QKV: token 0 of an image (cls) is stored at position tokens-1 of Q / K / V^T and token t
                                    * at position t-1 (patches first: the layout bs_attention_table reads) */
    int32_t qkv_cls_rows;          /* BS_OUT_QKV, > 0: the rows are GROUPED -- rows [0, qkv_cls_rows) are the cls tokens of the images,
                                    * row qkv_patch_row0 + b*(tokens-1) + t is patch t of image b (needs qkv_cls_last); the rows
                                    * in between are padding and are not stored */
    int32_t qkv_patch_row0;        /* >= qkv_cls_rows; M = qkv_patch_row0 + qkv_cls_rows * (tokens-1) */
    int32_t f8_wonly_from;         /* with f8_seg: 0 = every row gets both correction products; k > 0 = the 256-row tiles that start at
                                    * a row >= k evaluate only the first FP8 half (A_hi8 W_lo8, the weight-rounding correction) and
                                    * stop before the second (A_lo8 W_hi8, the activation-rounding correction); -1 = all rows.
                                    * Activation rounding is per-row noise that stays incoherent in the depth map except on the
                                    * cls-token rows, whose error shifts the whole map (Numerics): grouped cls rows + this
                                    * switch run the backbone at 1.5 instead of 2 pass-equivalents. */
    int32_t out_lo8_rows;          /* with out_f8, > 0: only output rows below this index store their lo8 plane (their consumer is a
                                    * GEMM with f8_wonly_from = this value, which never reads it on the other rows) */
    int32_t f8_skip_from;          /* with f8_seg, k > 0: tiles that start at a row >= k run NO FP8 stage (one 16-bit pass); their
                                    * weight-rounding error is corrected by its token-independent part instead, see bias2.  -1 = no tile
                                    * runs one (a neck product the calibration took down to one pass; also with conv) */
    int32_t bias2_row0;            /* bias2 applies to rows m >= bias2_row0 ... */
    int32_t bias2_group_rows;      /* ... with group (m - bias2_row0) / bias2_group_rows (> 0 when bias2 is given) */
    int32_t out_planes_rows;       /* with out_f8, > 0: 256-row tiles that start at a row >= this store the hi16 values only (no FP8
                                    * plane: their consumer sets f8_skip_from to this value, or -1 with 256 here) */
    const float* bias2;            /* optional fp32 [groups, N], added like the bias: y = acc + bias[n] + bias2[group, n].  The backbone
                                    * uses it for the rank-1 part of the weight-rounding error of a single-pass product:
                                    * A dW^T ~ 1 (mean_tokens(A) dW^T) per image (Numerics); excludes bias_group_rows */
    int32_t qkv_lo_off;            /* BS_OUT_QKV, > 0: the rounding residuals of Q, K and V^T (y - round16(y) as a second 16-bit value, unscaled)
                                    * are stored too, this many ELEMENTS behind the respective value in out / out2 / out3 (each tensor
                                    * allocated twice over): the operands of bs_attention_table_corr */
    int32_t out2_relu;             /* BS_OUT_PLAIN with out_f8, != 0: out2 receives relu(y) in the same (hi16 | hi8 | lo8) row format and geometry as
                                    * out (a second output of the epilogue).  The fusion stage's pre-activation residual units read both x (the skip)
                                    * and relu(x) (their first convolution's input): the producing convolution writes the two instead of a
                                    * bs_relu_split launch re-reading x (HF modeling_zoedepth.py:262-297) */
} bs_gemm_desc;
int bs_gemm(const bs_gemm_desc* d, void* stream);
/* the tile variant bs_gemm will pick for this descriptor (BM x BN x BK: 1: 128x128x64, 2: 128x64x64, 3: 128x32x64, 9: 256x256x64,
 * 10: 256x256x32 ping-pong, 11: 256x128x32; csrc/igemm.hip).  The main-loop schedule of tile 9 is not part of the id. */
int bs_gemm_tile(const bs_gemm_desc* d);

/* column means over a sample of the rows of each group: out[g, k] = mean_{j < rows_per_group, j % row_step == 0} A[row0 + g*rows_per_group + j, k]
 * for the 16-bit matrix A (row stride lda elements; the hi16 plane of a pair row), written as bf16 [groups, K] -- the A operand of
 * bs_rank1_bias, which forms bias2 above (mean over the patch tokens of an image; a sample of every 8th token changes the depth
 * result by < 1e-6 m, tools/probes/weight_mean_correction.py). */
int bs_col_mean(const void* A, int64_t lda, int32_t row0, int32_t rows_per_group, int32_t groups, int32_t row_step, int32_t K,
                void* out_bf16, float* zero_out, int64_t zero_n, int32_t dtype, void* stream);
/* out[g, n] += sum_k abar[g, k] * dW[n, k]: bf16 [G, K] x bf16 [N, K]^T accumulated into fp32 [G, N], which the caller has zeroed
 * (bs_col_mean clears `zero_out[0 .. zero_n)` for it).  With dW = W - round16(W) this is bias2 of the backbone's single-pass
 * products.  The K axis is cut in two halves that meet by atomics: two addends, so the result is order-independent. */
int bs_rank1_bias(const void* abar_bf16, const void* dw_bf16, float* out, int32_t G, int32_t N, int32_t K, void* stream);

/* BEiT attention: softmax(Q K^T + relpos_bias) V -------------------------------------------- *
 * HF modeling_beit.py:268-341 (eager_attention_forward with the additive relative-position bias
 * of :179-265).  The softmax is evaluated in the log2 domain: q [B,nh,Sp,64] must be pre-scaled by
 * log2(e)/sqrt(64) and bias pre-multiplied by log2(e).  k [B,nh,Sp,64], vt [B,nh,64,Sp], Sp % 64 == 0,
 * rows/cols >= S zero; bias fp32 [nh,Sp,Sp] with <= -1e30 in key columns >= S.
 * out [B*S, nh*64] token-major (the o_proj GEMM's A operand).
 * dtype | 16: out holds (hi | lo) pairs, [B*S, 2*nh*64]; dtype | 32: (hi16 | hi8 | lo8) rows of the same size. */
int bs_attention(const void* q, const void* k, const void* vt, const float* bias, void* out,
                 int32_t B, int32_t nh, int32_t S, int32_t Sp, int32_t dtype, void* stream);
/* The same attention for a window of hp x wp patches + cls with the bias taken from the per-head TABLE instead of a
 * materialised [nh,Sp,Sp] tensor: table fp32 [nh, (2hp-1)(2wp-1)+3], pre-multiplied by log2(e): HF's entries
 * (modeling_beit.py:194-218: (dy+hp-1)*(2wp-1) + (dx+wp-1) for patch pairs, then cls->patch, patch->cls, cls->cls) with the
 * (2hp-1)(2wp-1) patch-pair entries stored in REVERSED order (entry i at index nbody-1-i: the 8 consecutive keys a lane
 * handles are then 8 ascending words), the three cls entries last, unchanged.
 * q / k / vt hold the tokens of an image patches first, cls LAST (S = hp*wp + 1; bs_gemm_desc.qkv_cls_last); out rows are in
 * the usual order (cls first per image), or with grouped > 0 the B cls rows first and the hp*wp patch rows of image b from row
 * grouped + b*hp*wp on (bs_gemm_desc.qkv_cls_rows / qkv_patch_row0).  Built for wp == 32 (every 512-wide network input). */
int bs_attention_table(const void* q, const void* k, const void* vt, const float* table, void* out,
                       int32_t B, int32_t nh, int32_t hp, int32_t wp, int32_t Sp, int32_t grouped, int32_t dtype, void* stream);
/* The same with SPLIT-PRECISION operands: q_lo / k_lo / vt_lo hold x - round16(x) of the respective tensor (same shapes; written by
 * bs_gemm with qkv_lo_off), and the kernel evaluates  S = Q K^T + Q_lo K^T + Q K_lo^T,  O = V P + V P_lo + V_lo P  on the 16-bit MFMA
 * (three passes into the same fp32 accumulators; P split in registers).  For weights whose LayerNorm outputs carry outlier channels
 * -- trained BEiT checkpoints -- the single 16-bit Q / K / V / P of bs_attention_table cost 1-3e-4 m of depth
 * (tools/probes/outlier_rounding_study.py); ZoeDepthEngine.calibrate chooses between the two per weight set.  hp must be even. */
int bs_attention_table_corr(const void* q, const void* k, const void* vt, const void* q_lo, const void* k_lo, const void* vt_lo,
                            const float* table, void* out, int32_t B, int32_t nh, int32_t hp, int32_t wp, int32_t Sp, int32_t grouped,
                            int32_t dtype, void* stream);

/* LayerNorm over the last dim, fp32 in; out16 (fp16/bf16, nullable) and out32 (fp32, nullable, may
 * alias x) -- HF modeling_beit.py:418,432; post-norm of the router HF modeling_zoedepth.py:876-881
 * dtype | 16: out16 holds (hi | lo) pairs, [rows, 2*cols] (bs_cast_split's format); dtype | 32: (hi16 | hi8 | lo8) rows. */
int bs_layernorm(const float* x, const float* gamma, const float* beta, void* out16, float* out32, int32_t rows,
                 int32_t cols, float eps, int32_t dtype, void* stream);

/* device-to-device copy on the stream (re-arming the router's positional-encoding buffer) */
int bs_copy_f32(const float* src, float* dst, int64_t n, void* stream);

/* split-precision helpers: fp32 [rows, cols] -> 16-bit (hi | lo) pairs [rows, 2*cols] with x = hi + lo to ~22 bits; ReLU of such a
 * tensor (the pre-activation residual units, HF modeling_zoedepth.py:225-241).  bs_resize_bilinear_nhwc takes such tensors when
 * bit 1 of align_corners is set; bs_logbinom_depth takes a (hi | lo) `last` when bit 4 of dtype is set.
 * With `| 32` on the dtype argument (bit 2 of align_corners for the resize) the same calls work on the (hi16 | hi8 | lo8)
 * format of the FP8 correction passes (BS_F8_ACT_*_EXP above); bs_relu_split with `| 32 | 64` leaves the lo8 plane alone (neither read
 * nor written: an output whose only reader runs the weight-rounding correction only), with `| 32 | 128` both FP8 planes (its only reader
 * runs one 16-bit pass). */
int bs_cast_split(const float* x, void* out, int64_t rows, int32_t cols, int32_t out_dtype, void* stream);
int bs_relu_split(const void* x, void* out, int64_t rows, int32_t cols, int32_t dtype, void* stream);

/* fp32 -> fp16/bf16 cast (tap copies of the residual stream) */
int bs_cast(const float* x, void* out, int64_t n, int32_t out_dtype, void* stream);

/* MDEM pre-processing: uint8 frames -> im2col'ed patch matrix --------------------------------- *
 * HF image_processing_pil_zoedepth.py:181-232 (upstream depth_model.py#L57): /255, reflect pad,
 * bilinear align_corners=True resize to (nh, nw), (x-0.5)/0.5; fused with the 16x16 patch gather
 * of HF modeling_beit.py:83-90.  frames [B,H,W,3] u8; out [2B or B][(nh/16)*(nw/16)][3*16*16]
 * (k = c*256 + ky*16 + kx); images B..2B-1 are the W-flipped copies when flip != 0.
 * out_dtype | 16: rows are (hi | lo) pairs, [., 2*768]; out_dtype | 32: (hi16 | hi8 | lo8) rows. */
int bs_preprocess_patches(const uint8_t* frames, void* out, int32_t B, int32_t H, int32_t W, int32_t nh,
                          int32_t nw, int32_t flip, int32_t out_dtype, void* stream);
/* the same pre-processing to a plain NCHW fp32 image (tests) */
int bs_preprocess_image(const uint8_t* frames, float* out, int32_t B, int32_t H, int32_t W, int32_t nh,
                        int32_t nw, int32_t flip, void* stream);

/* rows[b*rows_per_image + 0, :] = v  (cls token, HF modeling_beit.py:166-167) */
int bs_fill_rows(float* x, const float* v, int32_t B, int32_t rows_per_image, int32_t cols, void* stream);

/* bilinear resize of an NHWC fp16/bf16 map -- F.interpolate calls at HF modeling_zoedepth.py:259,319,360.  `align_corners`: bit 0 the flag itself,
 * bit 1 the tensors hold (hi | lo) 16-bit pairs, bit 2 (hi16 | hi8 | lo8) rows, bit 3 (with bit 2) the OUTPUT's lo8 plane is not written (for a map
 * whose every consumer runs the weight-rounding correction only: nobody reads that plane), bit 4 (with bit 2) neither FP8 plane is (every consumer
 * runs one 16-bit pass) */
int bs_resize_bilinear_nhwc(const void* x, void* out, int32_t B, int32_t Hin, int32_t Win, int32_t C,
                            int32_t Hout, int32_t Wout, int32_t align_corners, int32_t dtype, void* stream);

/* out = relu(bilinear resize(x, align_corners) + bias[c]): the second half of a 1x1 convolution + ReLU whose input is an upsampled map -- the
 * bins head's projectors read the fusion stage's x2 outputs (HF modeling_zoedepth.py:749-772 on :316-322's maps); the convolution is linear and
 * commutes with the resize, so it runs at the LOW resolution (a quarter of the pixels, bs_gemm without bias) and this call upsamples its output.
 * x, out: NHWC 16-bit rows of C values, or (hi | lo) pairs (flags bit 1); flags bit 0 (align_corners) is required; bias fp32 [C]. */
int bs_resize_bias_relu_nhwc(const void* x, const float* bias, void* out, int32_t B, int32_t Hin, int32_t Win, int32_t C, int32_t Hout,
                             int32_t Wout, int32_t flags, int32_t dtype, void* stream);

/* conv3x3(pad 1)(interpolate x2(x)) evaluated from tap products taken at the low resolution -- the relative head's
 * `upsample` + `conv2` (+ ReLU), HF modeling_zoedepth.py:358-362.  y fp32 [B, Hin, Win, 9*Cout] holds, per low-resolution pixel,
 * y[(ky*3+kx)*Cout + o] = sum_c W[o, c, ky, kx] x[c] (one bs_gemm over the low-resolution map); this call gathers, per output pixel
 * p and tap d, the bilinear sample of y's tap plane at p + d (zero when p + d lies outside the Hout x Wout map: the conv's zero
 * padding), adds bias fp32 [Cout], applies ReLU when `relu`, and writes an NHWC 16-bit map [B, Hout, Wout, Cout] (`align_corners`
 * bits 1 / 2 select the (hi | lo) / (hi16 | hi8 | lo8) pair formats as for bs_resize_bilinear_nhwc). */
int bs_upconv_tapsum(const float* y, const float* bias, void* out, int32_t B, int32_t Hin, int32_t Win, int32_t Cout,
                     int32_t Hout, int32_t Wout, int32_t align_corners, int32_t relu, int32_t dtype, void* stream);

/* The same relu(conv3x3(pad 1)(interpolate x2, align_corners(x))) in ONE launch, from the low-resolution input itself (round 5): the tap
 * products exist only as LDS tiles (bodyslam_amd/csrc/upconv_fused.hip).  Replaces bs_gemm (the tap products) + bs_upconv_tapsum for the
 * relative head's geometry: Cin = 128, Cout = 32, Hout = 2 Hin, Wout = 2 Win.  x: NHWC rows of Cin 16-bit values (mode 0) or
 * (hi16 | hi8 | lo8) rows (mode 1: weight-rounding correction only, mode 2: both corrections); w: [9*Cout] rows, n = (ky*3+kx)*Cout + o, of
 * Cin 16-bit values (mode 0) or [W_hi16 | W_lo8 | W_hi8] (bs_gemm's FP8 correction packing; sa0, sb0, sa1, sb1 = its f8_scales bytes).
 * flags: bit 0 align_corners (required), bits 1 / 2 the output pair format as for bs_upconv_tapsum (modes 1, 2 need one). */
int bs_upconv_fused(const void* x, const void* w, const float* bias, void* out, int32_t B, int32_t Hin, int32_t Win, int32_t Cin,
                    int32_t Cout, int32_t Hout, int32_t Wout, int32_t flags, int32_t relu, int32_t mode, int32_t sa0, int32_t sb0,
                    int32_t sa1, int32_t sb1, int32_t dtype, void* stream);

/* metric-bins head ---------------------------------------------------------------------------- *
 * Both heads (nyu | kitti) are carried side by side as channel groups; `route` int32 [B] (from
 * bs_route_argmax) says which group an image uses -- per image, because the reference always runs
 * the network with batch 1 (interface.py:61), never HF's batch-summed vote (modeling_zoedepth.py:1063-1067).
 *
 * attractor step, HF modeling_zoedepth.py:665-746 (unnormed, memory_efficient, kind "mean",
 * inv_attractor defaults alpha=300 gamma=2): bins_out[b,y,x,g,:] = c + mean_a dx/(1+300 dx^2),
 * c = bilinear(align_corners=True) resample of bins_prev to (H, W), dx = A[b,y,x,g,a] - c.
 * A fp32 [B,H,W,groups*n_attr] (softplus already applied), bins fp32 NHWC [.,groups*n_bins];
 * route nullable (null: every group is computed). */
int bs_attractor_step(const float* A, const float* bins_prev, float* bins_out, const int32_t* route, int32_t B,
                      int32_t Hp, int32_t Wp, int32_t H, int32_t W, int32_t groups, int32_t n_bins, int32_t n_attr,
                      void* stream);
/* The attractor MLP in one launch, HF modeling_zoedepth.py:665-700 (`Conv2d(E, 2E, 1)`, ReLU, `Conv2d(2E, n_attractors, 1)`, softplus;
 * both metric heads' MLPs stacked):  out = act2(round16(relu(x W1^T + b1)) W2^T + b2).
 * x rows of ldx 16-bit values (the first K1 are read), W1 [N1, K1], W2 [N2, N1] 16-bit, b1 / b2 fp32, out fp32 [M, N2].
 * Built for K1 = 128, N1 = 256, N2 a multiple of 4 up to 32; bit-identical to bs_gemm(act = ReLU, 16-bit out) followed by
 * bs_gemm(act = act2, fp32 out) -- the hidden map (M x 256) never reaches memory. */
int bs_mlp2(const void* x, int32_t ldx, const void* W1, const float* b1, const void* W2, const float* b2, float* out, int32_t M,
            int32_t K1, int32_t N1, int32_t N2, int32_t act2, int32_t dtype, void* stream);
/* bs_add_resized + bs_mlp2 in one launch (an attractor level, HF modeling_zoedepth.py:726-730 then :665-700): the MLP's input row is
 * formed in the kernel, x[m] = round16(emb[m] + bilinear_align_corners(prev)[m]), and never stored.  emb [B,H,W,K1] and prev [B,Hp,Wp,K1]
 * 16-bit NHWC; dtype bit 4 (| 16): both hold (hi | lo) pairs of K1 channels each (pixel stride 2 K1), the sum uses hi + lo.
 * Bit-identical to bs_add_resized followed by bs_mlp2 on its hi half. */
int bs_mlp2_add(const void* emb, const void* prev, const void* W1, const float* b1, const void* W2, const float* b2, float* out,
                int32_t B, int32_t Hp, int32_t Wp, int32_t H, int32_t W, int32_t K1, int32_t N1, int32_t N2, int32_t act2, int32_t dtype,
                void* stream);
/* One level of the bins head's projector path in one launch (round 6; replaces, for that level, bs_resize_bias_relu_nhwc + the projector's
 * second 1x1 convolution as a 3-pass bs_gemm + the sum inside bs_mlp2_add + -- at the last level -- the log-binomial embedding bs_gemm; HF
 * modeling_zoedepth.py:749-772 (Projector), :726-730 (the attractor level's input), :376-491 (the conditional log-binomial MLP's first layer):
 *   e1 = relu(bilinear_align_corners(z) + b_c1);  emb = W_c2 e1 + b_c2;  x = round16(emb + bilinear_align_corners(emb_prev));  Eh = W_e e1 + b_e
 * z [B,Hl,Wl,2 PM] and emb_prev [B,Hl,Wl,2 E]: (hi | lo) 16-bit pairs on the SAME low-resolution grid; W_c2 [E, 3 PM], W_e [NE, 3 PM]: rows
 * [W_hi | W_hi | W_lo] (the 3-pass pair packing of bs_gemm's seg1 form); biases fp32.  Outputs: x_out [B,H,W,E] 16-bit (the attractor MLP's
 * input: bs_mlp2 with ldx = E), emb_out [B,H,W,2 E] (hi | lo) pairs or null (the last level hands no embedding on), eh_out fp32 [B,H,W,NE] or
 * null (then W_e / b_e are null too).  Built for PM = 64, E = 128, NE a multiple of 16 up to 80, W a multiple of 32.  The products run the K
 * order of the bs_gemm they replace: Eh carries the same bits; x differs from the two-launch path by the pair rounding of emb it no longer makes. */
int bs_projector_level(const void* z, const float* b_c1, const void* emb_prev, const void* Wc2, const float* b_c2, const void* We,
                       const float* b_e, void* x_out, void* emb_out, float* eh_out, int32_t B, int32_t Hl, int32_t Wl, int32_t H, int32_t W,
                       int32_t PM, int32_t E, int32_t NE, int32_t dtype, void* stream);
/* out[b,y,x,:] = x[b,y,x,:] + bilinear_align_corners(prev)[b,y,x,:] (fp16/bf16 NHWC); HF :726-730.
 * dtype bit 4 (| 16): x, prev and out hold (hi | lo) pairs of C channels each (pixel stride 2C), see bs_cast_split. */
int bs_add_resized(const void* x, const void* prev, void* out, int32_t B, int32_t Hp, int32_t Wp, int32_t H,
                   int32_t W, int32_t C, int32_t dtype, void* stream);
/* conditional log-binomial + expectation, HF modeling_zoedepth.py:376-491,1086-1101, per output pixel:
 *   h = gelu(bilinear(Eh)[g] + W0_last[g] . last)     Eh fp32 [B,He,We,2*40] = W0_emb . emb + b0 (a bs_gemm; the
 *                                                      1x1 conv commutes with the bilinear resample)
 *   pt = softplus(W2[g] h + b2[g]); p, T; y_k = logC(63,k) + k log p + (63-k) log(1-p)
 *   depth = sum_k softmax(y/T)_k * bilinear(bins)[g,k]
 * last 16-bit [B,H,W,32]; bins fp32 [B,He,We,2*64]; w0_last [2,40,32], w2 [2,4,40], b2 [2,4] fp32. */
int bs_logbinom_depth(const void* last, const float* Eh, const float* bins, const float* w0_last, const float* w2,
                      const float* b2, const int32_t* route, float* depth, int32_t B, int32_t H, int32_t W,
                      int32_t He, int32_t We, float min_temp, float max_temp, int32_t dtype, void* stream);
/* The same with the hidden width as an argument (40: NK head, 80: the single-head ZoeD_N / ZoeD_K models, whose Eh is
 * [B,He,We,2*80] and w0_last / w2 are [2,hid,32] / [2,4,hid]) and the single head's 33rd MLP input, the relative depth
 * relu(conv3(last)) (HF modeling_zoedepth.py:367-371,1186-1191): rel_w (nullable) = per group
 * [W0 column of that input x hid | conv3 weight x 32 | conv3 bias]. */
int bs_logbinom_depth_ex(const void* last, const float* Eh, const float* bins, const float* w0_last, const float* w2,
                         const float* b2, const float* rel_w, int32_t hid, const int32_t* route, float* depth, int32_t B,
                         int32_t H, int32_t W, int32_t He, int32_t We, float min_temp, float max_temp, int32_t dtype,
                         void* stream);
/* domain router pieces, HF modeling_zoedepth.py:775-962: multi-head attention of the 4-layer patch
 * transformer (head_dim 32, S = 1 + h*w tokens, no mask) on fused fp32 qkv [B*S, 3*D] -> out 16-bit
 * [B*S, D]; the linear layers run on bs_gemm and the post-norms on bs_layernorm. */
int bs_small_attention(const float* qkv, void* out, int32_t B, int32_t S, int32_t nheads, int32_t dtype, void* stream);
/* route[b] = argmax(logits[b, 0:2]) (first maximal index, as torch.argmax), HF :1066-1067 */
int bs_route_argmax(const float* logits, int32_t ld, int32_t* route, int32_t B, void* stream);

/* MDEM post-processing: HF image_processing_pil_zoedepth.py:234-341 + upstream infer_pil:
 * average d[b] with the un-flipped d[B+b], bicubic (A=-0.75, align_corners=False) resize of the
 * (nh, nw) map to the padded size, crop, write metres fp32 [B,H,W] and (nullable) uint16 = trunc(m*256). */
int bs_postprocess_depth(const float* depth_net, float* depth_m, uint16_t* depth_u16, int32_t B, int32_t H,
                         int32_t W, int32_t nh, int32_t nw, int32_t flip, void* stream);

/* MPEM (CyclePose pose branch) ---------------------------------------------------------------- */
/* mpem_interface.py:40-44,85-94 + architecture_v3.py:120-122: center-crop 128, /255, (x-.5)/.5, pair
 * concat, ReflectionPad(3) and 7x7 im2col: out [P*128*128, 320] (k = (ky*7+kx)*6 + c, zero padded 294..319) */
int bs_cyclepose_im2col(const uint8_t* frames, const int32_t* pairs, void* out, int32_t P, int32_t H, int32_t W,
                        int32_t dtype, void* stream);
/* the same over an arbitrary CH x CW window at (top, left) of every frame (type_of_trans='resize', mpem_interface.py:45-50,88-90:
 * the frames arrive already resized to 128 x W' by PIL and the window is the whole frame); rows [P*CH*CW, 320 (x2 with | 16)] */
int bs_cyclepose_im2col_window(const uint8_t* frames, const int32_t* pairs, void* out, int32_t P, int32_t H, int32_t W,
                               int32_t top, int32_t left, int32_t CH, int32_t CW, int32_t dtype, void* stream);
/* InstanceNorm2d(eps, no affine) + ReLU on an NHWC map, fp32 in -> fp16/bf16 out (+ optional fp32 copy)
 * architecture_v3.py:123-124,134-137.  scratch: >= P * ceil(HW/256) * 2 * C floats (per-chunk mean / M2). */
int bs_instnorm_relu_nhwc(const float* x, void* out, float* out_f32, float* scratch, int32_t P, int32_t HW, int32_t C,
                          float eps, int32_t dtype, void* stream);
/* AdaptiveAvgPool2d(1) of an NHWC fp32 map -> [P, C] fp32 (architecture_v3.py:146) */
int bs_avgpool_nhwc(const float* x, float* out, int32_t P, int32_t HW, int32_t C, void* stream);
/* pose head: skip_linear(cat[pooled, flatten_NCHW(x2)]) + pose_dense(pooled) -> quaternion normalise
 * -> 4x4 (architecture_v3.py:205-226, geometry_utils.py:230-265).  x2 is NHWC fp32 [P,32,32,256]; w_skip_x2 is
 * the skip weight re-laid to [7][HW][C]; outputs pose7 [P,7] and T [P,16] fp32.  The 262 144-long dot
 * products are split-K partial sums combined in a fixed order (bitwise reproducible). */
int bs_cyclepose_head(const float* pooled, const float* x2, const float* w_skip_pool, const float* w_skip_x2,
                      const float* b_skip, const float* w1, const float* b1, const float* w2, const float* b2,
                      float* pose7, float* T, float* scratch /* >= P*ceil(HW*C/4096)*8 floats */, int32_t P,
                      int32_t HW, int32_t C, void* stream);

/* 3DM ----------------------------------------------------------------------------------------- */
/* 3DM/scaling_system.py:72-77 pixel_to_3d + RGBD constants of 3DM/slam_utils.py:173,212-220,232.
 * depth u16 [B,H,W]; K = fx,fy,cx,cy (host); poses fp64 [B,16] device, nullable; xyz fp32 [B,H*W,3],
 * idx int32 [B,H*W] (row-major order of the valid pixels), count int32 [B]; scratch int32 >= B*(H*W/256+2). */
int bs_backproject(const uint16_t* depth, int32_t B, int32_t H, int32_t W, const double* K_host, double depth_scale,
                   double depth_trunc, const double* poses, float* xyz, int32_t* idx, int32_t* count,
                   int32_t* scratch, void* stream);
/* 3DM/scaling_system.py:72-77 pixel_to_3d verbatim on n (u, v, depth) fp64 triples -> (x, y, z) fp64 */
int bs_pixel_to_3d(const double* uvd, int64_t n, const double* K_host, double* out, void* stream);
/* 3DM/slam_utils.py:110-122 compute_curr_estimate_global_pose chained over N relatives (fp32 [N,16]) from
 * g0 (fp64 [16], host, nullable = identity) -> g_abs fp64 [N+1,16]; per-step SO(3) projection
 * (slam_utils.py:93-108).  With G_{i-1} a rotation, proj(G_{i-1}.R R_i) = G_{i-1}.R proj(R_i): every relative pose is
 * projected independently (one lane per pose), then the chain is a wave-shuffle prefix product over SE(3); matrices whose
 * bottom row is not [0 0 0 1] take the strict one-lane recurrence. */
int bs_pose_chain(const float* t_rel, int32_t N, const double* g0_host, double* g_abs, void* stream);
/* the same with g0 on the DEVICE (fp64 [16]; it may be the last pose of a previous call's g_abs: a sequence processed in
 * steps continues its chain without a host round trip -- 3DM/slam.py:148-153 keeps current_global_extrinsic_matrix) */
int bs_pose_chain_from(const float* t_rel, int32_t N, const double* g0_dev, double* g_abs, void* stream);

/* TSDF map (N4) ---------------------------------------------------------------------------------- *
 * Open3D ScalableTSDFVolume as wrapped by BodySLAM_not_refactored/3DM/tsdf.py:5-52 (voxel_length 0.001, sdf_trunc 0.1, RGB8,
 * volume_unit_resolution 32, depth_sampling_stride 8; integrate per frame at 3DM/slam.py:117,179, extract_point_cloud at :126,195).
 * State, all in device memory and owned by the caller:
 *   blocks      one per volume unit: res^3 voxels x 5 fp32 (tsdf, weight, r, g, b), voxel x*res^2 + y*res + z, zero-filled; block s
 *               lives at slab_base[s / slab_units] + (s % slab_units) * res^3 * 20 bytes (slab_base: int64 device array)
 *   unit table  open addressing: table_keys int64 [table_cap] (-1 = empty; table_cap a power of two), table_slots int32 [table_cap]
 *               (-1 until a block is assigned), table_fmask uint64 [table_cap] (bit f = record f of the pass under way touches the
 *               unit; zero between passes); unit_index int32 [max_units, 3]; unit_mask uint64 [max_units] and touched int32
 *               [max_units] (scratch of a pass: the records that reach a block, the blocks of the pass)
 *   counters    int32 [3]: number of units (persists across calls), units updated by the last integrate or update call, overflow
 *               flag (1: table full, 2: more new units than blocks, 3: see the update call -- sticky: set by any call since the
 *               caller last cleared it, so a stream of frames can be checked once at its end)
 *
 * There is one integration path, and a single frame is a batch of one record (n_frames = 1).  The reference integrates frame by
 * frame (3DM/slam.py:179); a voxel's running mean takes the frames in order and nothing else orders them, so up to
 * BS_TSDF_BATCH_MAX frames are integrated by loading every touched voxel once, applying the frames that touch its unit in
 * ascending order in registers and storing it once -- bit for bit what that many calls with one record each leave in the blocks,
 * in three launches.
 *   bs_tsdf_frames_upload    writes the batch's frame records (BS_TSDF_FRAME_BYTES each) to frames_dev: depth[f] / color[f] = the frames' device
 *                            images (depth fp32 [H, W] metres, <= 0 invalid; color u8 [H, W, 3]; color NULL or all entries NULL: no
 *                            colours), K = (fx, fy, cx, cy), extrinsics / poses = host doubles [n_frames, 16]: the world->camera 4x4
 *                            of every frame and its inverse
 *   bs_tsdf_touch_batch      ScalableTSDFVolume::Integrate's unit discovery for all frames: every unit that meets the +-sdf_trunc box of
 *                            a point of frame f's depth image sampled every `stride` pixels is inserted and gets bit f in table_fmask.
 *                            No blocks are handed out: a caller that can wait reads counters[0] and counts the entries with a mask but
 *                            no slot, makes the missing blocks, then calls
 *   bs_tsdf_integrate_batch  block assignment (max_units = the blocks that exist: overflow flag 2 is raised rather than a block handed
 *                            out that does not exist, so a stream of frames may be enqueued against blocks allocated ahead and
 *                            checked once at its end), the per-frame frustum test (a unit whose bounding sphere lies wholly outside
 *                            a frame's view holds no voxel that frame updates), unit_mask and `touched`, then
 *                            UniformTSDFVolume::IntegrateWithDepthToCameraDistanceMultiplier on those units; counters[1] = the
 *                            units updated; table_fmask is zero again afterwards */
#define BS_TSDF_BATCH_MAX 64
#define BS_TSDF_FRAME_BYTES 256
int bs_tsdf_frames_upload(const float* const* depth, const uint8_t* const* color, const double* K, const double* extrinsics, const double* poses,
                          int32_t n_frames, void* frames_dev, void* stream);
int bs_tsdf_touch_batch(const void* frames_dev, int32_t n_frames, int32_t H, int32_t W, int32_t stride, double unit_length, double sdf_trunc,
                        void* table_keys, void* table_fmask, int32_t table_cap, int32_t* counters, void* stream);
int bs_tsdf_integrate_batch(const void* frames_dev, int32_t n_frames, int32_t H, int32_t W, const void* table_keys, int32_t* table_slots,
                            void* table_fmask, int32_t table_cap, int32_t* unit_index, int32_t max_units, int32_t* counters, int32_t* touched,
                            void* unit_mask, const int64_t* slab_base, int32_t slab_units, int32_t res, double voxel_length, double sdf_trunc,
                            void* stream);
/* Frames taken out again (map correction after a pose-graph update; Open3D has no such operation): bs_tsdf_integrate_batch
 * with a sign per record.  Bit f of remove_mask set = record f is removed from the running means, clear = it is added; records are
 * applied to a voxel in ascending order in registers, the voxel is loaded once and stored once.  A removed record must carry the
 * extrinsic and images it was integrated with: the observation is then recomputed bit for bit and undone (w1 = w - 1; values
 * (v w - x) / w1).  A voxel whose weight returns to 0 becomes five +0.0f, as in a fresh block; a removal that finds weight < 1 is
 * skipped and sets counters[2] = 3 (sticky, like 1 and 2).  Units are never freed.  Preceded by bs_tsdf_frames_upload and
 * bs_tsdf_touch_batch exactly as bs_tsdf_integrate_batch is. */
int bs_tsdf_update_batch(const void* frames_dev, int32_t n_frames, int32_t H, int32_t W, const void* table_keys, int32_t* table_slots,
                         void* table_fmask, int32_t table_cap, int32_t* unit_index, int32_t max_units, int32_t* counters, int32_t* touched,
                         void* unit_mask, const int64_t* slab_base, int32_t slab_units, int32_t res, double voxel_length, double sdf_trunc,
                         uint64_t remove_mask, void* stream);
/* ScalableTSDFVolume::ExtractPointCloud (points, colours, normals) over blocks 0 .. units-1 in two passes: points == NULL counts into
 * unit_count int32 [units]; otherwise unit_offset int64 [units] (exclusive prefix sums of the counts) places each unit's points,
 * points / colors fp32 [total, 3]; normals fp32 [total, 3] or NULL: ScalableTSDFVolume::GetNormalAt, the normalised central
 * difference of the trilinearly interpolated tsdf (GetTSDFAt) at +-0.99 voxel_length. */
int bs_tsdf_extract(const int32_t* unit_index, int32_t units, const void* table_keys, const int32_t* table_slots, int32_t table_cap,
                    const int64_t* slab_base, int32_t slab_units, int32_t res, double voxel_length, int32_t* unit_count,
                    const int64_t* unit_offset, float* points, float* colors, float* normals, void* stream);

/* ScalableTSDFVolume::ExtractTriangleMesh (BodySLAM_not_refactored/3DM/tsdf.py:42-52, called on the last frame at 3DM/slam.py:189-193):
 * marching cubes over every voxel cube of blocks 0 .. units-1, in two passes like bs_tsdf_extract.  mc_tab (device int32) = the case
 * table [256][tri_width] (-1 terminated lists of cube-edge ids, three per triangle) followed by the edge corners [12][2]
 * (bodyslam_amd/marching_cubes.py: corner c at offset (c & 1, c >> 1 & 1, c >> 2 & 1), bit c of the case = tsdf < 0).  Count pass
 * (vertices == NULL): unit_count int32 [units] = triangles per unit.  Write pass: unit_offset int64 [units] (exclusive prefix sums,
 * in triangles); per triangle corner k of triangle t: vertices / colors fp32 [3 * total, 3] and vertex_keys int64 [3 * total], the
 * identity of the cube edge the vertex lies on -- equal keys are one vertex of the mesh.  *err is set when a voxel coordinate does
 * not fit the key's 20 bits per axis. */
int bs_tsdf_mesh(const int32_t* unit_index, int32_t units, const void* table_keys, const int32_t* table_slots, int32_t table_cap,
                 const int64_t* slab_base, int32_t slab_units, int32_t res, double voxel_length, const int32_t* mc_tab, int32_t tri_width,
                 int32_t* unit_count, const int64_t* unit_offset, float* vertices, float* colors, int64_t* vertex_keys, int32_t* err, void* stream);

/* The model seen from a camera: a ray cast of the map.  The reference asks for it in three places: the MAP class
 * (BodySLAM_not_refactored/3DM/tsdf.py:56-107) calls Open3D's synthesize_model_frame after every integrate (:81-83) -- a ray cast of the
 * voxel grid at the current pose into its raycast_frame; 3DM/synthetic_depth_generator.py:74-97 (compute_synthetic_depth) and
 * 3DM/mapping_module.py:204-228 (_compute_synthetic_depth) cast pinhole rays against the extracted mesh and keep t_hit as the depth
 * image.  Open3D is not vendored: the marching scheme (KinectFusion's / VoxelBlockGrid::RayCast's in outline: sphere tracing on the
 * nearest voxel, trilinear samples near the surface, linear zero crossing; csrc/tsdf.hip and tests/_raycast_ref.py state it in full)
 * is pinned against analytic scenes, parity with Open3D itself is unpinned.
 *   K = (fx, fy, cx, cy) and extrinsics = n_views world->camera 4x4 (row-major fp64), both host pointers: the entry inverts them
 *   (a singular one is refused) and hands the camera records to the kernel itself, BS_TSDF_RAYCAST_VIEWS views per launch -- the
 *   caller sees no view limit.  Rays run from depth_min to depth_max (metres of camera-frame z, 0 <= depth_min < depth_max).
 *   Outputs, device memory: depth fp32 [n_views, H, W] (camera-frame z of the surface point, 0 = no surface); vertex fp32
 *   [n_views, H, W, 3] (world), normal fp32 [n_views, H, W, 3] (GetNormalAt of the point, as bs_tsdf_extract writes it), color u8
 *   [n_views, H, W, 3]; zeros where there is no hit; vertex, normal and color may each be NULL and are then not computed.
 *   The map is only read, through the unit table (an entry without a block is empty space): neither the unit count nor a host
 *   round trip is needed, so the call may follow un-synchronised bs_tsdf_touch_batch / bs_tsdf_integrate_batch calls on the same stream.
 *   n_views == 0 returns BS_OK. */
#define BS_TSDF_RAYCAST_VIEWS 32
int bs_tsdf_raycast(const double* K, const double* extrinsics, int32_t n_views, int32_t H, int32_t W, double depth_min, double depth_max,
                    const void* table_keys, const int32_t* table_slots, int32_t table_cap, const int64_t* slab_base, int32_t slab_units,
                    int32_t res, double voxel_length, double sdf_trunc, float* depth, float* vertex, float* normal, uint8_t* color, void* stream);

/* dense RGB-D odometry (N3) -------------------------------------------------------------------- *
 * The role of Open3D's rgbd_odometry_multi_scale (Method.Hybrid, 20 / 10 / 5 iterations) at
 * BodySLAM_not_refactored/3DM/visual_odometry.py:97-120; the algorithm is stated in oracle/rgbd_odometry_ref.py (parity with Open3D
 * unpinned).  Images are fp32 [H, W] in device memory, NaN = invalid depth; K = (fx, fy, cx, cy) and T (rows 0..2 of the
 * source -> target 4x4) are host doubles.
 *   bs_odo_prepare     intensity = (0.299 R + 0.587 G + 0.114 B) / 255 of color u8 [H, W, 3]; depth metres, <= 0 or > depth_max -> NaN
 *   bs_odo_pyrdown     next pyramid level [(H+1)/2, (W+1)/2]: [1 4 6 4 1]^2 / 256 at the even pixels, replicate borders; is_depth: the
 *                      weights run over the neighbours within depth_threshold of the centre, NaN where the centre is invalid
 *   bs_odo_sobel       3x3 Sobel / 8 in x and y, replicate borders, NaN propagates
 *   bs_odo_accumulate  the sums of one Gauss-Newton step at pose T: out29 = [21 upper-triangle terms of sum w J^T J (row-major),
 *                      6 terms of sum w J^T r, the weighted cost, the inlier count]; hybrid residuals (intensity + depth), Huber
 *                      weights, target sampled bilinearly; partial = scratch double [min(ceil(H*W/256), 256), 29]; deterministic.
 *                      flags bit 0: the target images are read at the NEAREST pixel of the projected point (round half away from zero),
 *                      Open3D's association; bit 1: Open3D's robust step -- sum J^T J unweighted, sum J^T huber'(r) with
 *                      huber'(r) = r clipped to +-delta, cost = sum huber(r)
 * `batch` (prepare / pyrdown / sobel / step): the images are `batch` contiguous [H, W] images, processed by ONE launch per stage.  The
 * frame-to-frame pairs of a sequence are independent of each other (every pair starts from the identity), so a batch of frames
 * is tracked as `batch` simultaneous pairs: bs_odo_step's pair p reads source image p of the src_* stacks and target image p of the
 * tgt_* stacks (for consecutive frames held in one [slots, H, W] stack: src = the stack + H*W, tgt = the stack), its pose is
 * T_dev[12 p ..], its scratch partial[p][.][29], its sums out29[29 p ..].  The sums of a pair do not depend on the batch. */
/* the pseudo-RGBD depth of the 3DM loop (3DM/slam_utils.py:212-220): out = u16 / depth_scale as fp32 metres, values >= depth_trunc -> 0 */
int bs_depth_u16_to_m(const uint16_t* depth_u16, int64_t n, double depth_scale, double depth_trunc, float* out, void* stream);
/* `iterations` Gauss-Newton steps of one pyramid level entirely on the device: bs_odo_accumulate's sums at the pose in T_dev (12
 * doubles in device memory, rows 0..2 of source -> target), delta = -(A + 1e-12 I)^-1 b, T_dev <- exp(delta) T_dev; a step with
 * fewer than 6 inliers leaves T_dev alone.  No host round trip between steps. */
int bs_odo_step(const float* src_intensity, const float* src_depth, const float* tgt_intensity, const float* tgt_depth,
                const float* tgt_dIx, const float* tgt_dIy, const float* tgt_dDx, const float* tgt_dDy, int32_t batch, int32_t H, int32_t W,
                const double* K, double* T_dev, int32_t iterations, double depth_outlier_trunc, double depth_huber,
                double intensity_huber, double* partial, double* out29, int32_t flags, void* stream);
int bs_odo_prepare(const uint8_t* color, const float* depth, int32_t batch, int32_t H, int32_t W, double depth_max, float* intensity,
                   float* depth_out, void* stream);
int bs_odo_pyrdown(const float* src, int32_t batch, int32_t H, int32_t W, float* dst, int32_t is_depth, double depth_threshold, void* stream);
int bs_odo_sobel(const float* img, int32_t batch, int32_t H, int32_t W, float* gx, float* gy, void* stream);
int bs_odo_accumulate(const float* src_intensity, const float* src_depth, const float* tgt_intensity, const float* tgt_depth,
                      const float* tgt_dIx, const float* tgt_dIy, const float* tgt_dDx, const float* tgt_dDy, int32_t H, int32_t W,
                      const double* K, const double* T, double depth_outlier_trunc, double depth_huber, double intensity_huber,
                      double* partial, double* out29, int32_t flags, void* stream);

/* frame-to-model tracking: point-to-plane odometry on the ray-cast map --------------------------- *
 * The role of Open3D's Model.track_frame_to_model(input_frame, raycast_frame, depth_scale = 1000, depth_max = 3.0, depth_diff = 0.07)
 * (point-to-plane, 6 / 3 / 1 iterations) behind the reference's MAP (BodySLAM_not_refactored/3DM/tsdf.py:56-107).  Open3D is not
 * vendored: those defaults restate its published interface, the algorithm is stated in tests/_point_to_plane_ref.py, and parity with
 * Open3D itself is UNPINNED.  The source is the input frame's depth pyramid, the target the pyramid of the model's ray-cast depth
 * (bs_tsdf_raycast); both use bs_odo_pyrdown in depth mode with threshold 2 * depth_diff, intrinsics halved per level.
 *   bs_odo_p2p_prepare     level 0 of a pyramid: depth metres fp32 [batch, H, W], <= 0 or > depth_max -> NaN (the ray cast's 0 = no
 *                          surface becomes NaN with any depth_max)
 *   bs_odo_p2p_target      the target maps of one level: target = fp32 [batch, H, W, 4], 16-byte aligned, one record (nx, ny, nz, z)
 *                          per pixel: z = the depth as given (NaN = invalid) and n = the unit normal of the vertex map
 *                          V(u, v) = ((u - cx) z / fx, (v - cy) z / fy, z), n = normalise((V(u+1, v) - V(u, v)) x (V(u, v+1) - V(u, v))),
 *                          computed in fp64 and stored as fp32; NaN on the last row and column, where one of the three depths is
 *                          invalid, or where the cross product has zero length.  The step rebuilds the target vertex from (u, v, z),
 *                          so its scattered nearest-pixel read is one aligned 16-byte load.  K = (fx, fy, cx, cy) of the level, host
 *   bs_odo_p2p_accumulate  the sums of one step at the host pose T (rows 0..2 of source -> target), bs_odo_accumulate's out29 layout:
 *                          for every valid source pixel p = T v_s (p.z > 0), the NEAREST target pixel of its projection (round half
 *                          away from zero, inside the image), q and n there (both valid), r = (p - q) . n with |r| <= depth_diff,
 *                          J = [p x n, n] for the left twist (omega, nu); out29 = [sum J J^T (21, unweighted), sum J clip(r, +-depth_huber)
 *                          (6), sum huber(r), the inlier count]; partial = scratch double [min(ceil(H*W/256), 256), 29]; deterministic
 *   bs_odo_p2p_step        `iterations` such steps of one level on the device, as bs_odo_step: pair p of `batch` reads source image p,
 *                          target record image p, pose T_dev[12 p ..], scratch partial[p][.][29], sums out29[29 p ..]; the same kernel
 *                          (fixed-order finish, 6x6 solve, pose update) as bs_odo_step; fewer than 6 inliers leave the pose alone */
int bs_odo_p2p_prepare(const float* depth, int32_t batch, int32_t H, int32_t W, double depth_max, float* depth_out, void* stream);
int bs_odo_p2p_target(const float* depth, int32_t batch, int32_t H, int32_t W, const double* K, float* target, void* stream);
int bs_odo_p2p_accumulate(const float* src_depth, const float* target, int32_t H, int32_t W, const double* K, const double* T,
                          double depth_diff, double depth_huber, double* partial, double* out29, void* stream);
int bs_odo_p2p_step(const float* src_depth, const float* target, int32_t batch, int32_t H, int32_t W, const double* K, double* T_dev,
                    int32_t iterations, double depth_diff, double depth_huber, double* partial, double* out29, void* stream);

/* ---- depth evaluation with the reference's MDEM protocol ----------------------------------------------------------------------------
 * Replaces the per-frame body of compute_metrics_for (BodySLAM_not_refactored/EVALUATION/MDEM_eval.py:179-197 masking and median
 * scaling with compute_median_scale_factor :114-127; the MDEM_Metrics functions of EVALUATION/evaluation_metrics.py:24-102).
 * pred, gt: uint16 [B, H, W] (device; pred = depth in metres*256 as bs_zoedepth_forward writes it, gt in dataset units).  Per frame, fp64:
 *   mask      gt_lo < gt < gt_hi on GT only (Hamlyn (1, 300), SCARED (0, inf), EndoSlam no mask: (-inf, inf); NaN bounds: empty)
 *   scale     BS_DEPTH_SCALE_MEDIAN: s = median(gt[mask]) / median(pred[mask]), numpy's median (the mean of the two middle values for an
 *             even count); BS_DEPTH_SCALE_FIXED: s = `scale`.  p = s * pred
 *   metrics   over the masked pixels: abs_rel = mean |g - p| / g, sq_rel = mean (g - p)^2 / g, rmse = sqrt(mean (g - p)^2) over
 *             g != 0 with p not NaN (np.nanmean skips NaN terms); rmse_log = sqrt(mean (log g - log p)^2) and delta_k = the fraction
 *             with max(g / p, p / g) < 1.25^(2k) (the reference squares its criterion 1.25^k) over g > 0 and p > 0.  log g is the
 *             fp32 logarithm of g (numpy takes np.log of a uint16 array in fp32), log p fp64.  An empty mask gives NaN medians and NaN
 *             metrics; median(pred) = 0 gives s = inf, IEEE arithmetic as numpy's
 * out: fp64 [B, BS_DEPTH_METRICS_FIELDS] (device), per frame: 0 abs_rel, 1 sq_rel, 2 rmse, 3 rmse_log, 4 delta_1, 5 delta_2, 6 delta_3,
 *   7 scale, 8 median(gt[mask]), 9 median(pred[mask]), 10 n_mask (masked pixels), 11 n_valid (terms of 0-2), 12 n_pos (terms of 3-6),
 *   13-15 zero.  A frame's record has the same bits in every run, alone or at any position of any batch (fixed summation order).
 * workspace: device memory of bs_depth_metrics_workspace(B, H, W) bytes (>= workspace_bytes is checked), reused across calls on one
 * stream.  Six launches and one memset on `stream`, nothing else. */
enum { BS_DEPTH_SCALE_MEDIAN = 0, BS_DEPTH_SCALE_FIXED = 1 };
#define BS_DEPTH_METRICS_FIELDS 16
int64_t bs_depth_metrics_workspace(int32_t B, int32_t H, int32_t W);
int bs_depth_metrics(const uint16_t* pred, const uint16_t* gt, int32_t B, int32_t H, int32_t W, double gt_lo, double gt_hi, int32_t scale_mode,
                     double scale, void* workspace, int64_t workspace_bytes, double* out, void* stream);

/* ---- trajectory evaluation with the reference's MPEM metrics ------------------------------------------------------------------------
 * bs_similarity_fit replaces estimate_similarity_transformation (BodySLAM_not_refactored/3DM/slam_utils.py:138-169; evo's
 * umeyama_alignment is the same arithmetic): the similarity (R, s, t) with target ~ s R source + t, Umeyama's least-squares fit.
 *   source, target   [n, 3] row-major points (device), both BS_F32 or both BS_F64, 1 <= n <= 2^31 - 1; arithmetic in fp64
 *   out              16 doubles (device): 0-8 R row-major, 9 s, 10-12 t, 13 sigma_x = mean |x - mean x|^2, 14 the number of singular values
 *                    of Sxy = mean (y - mean y)(x - mean x)^T above DBL_EPSILON, 15 n.  S = diag(1, 1, -1) when det(Sxy) < 0, as the
 *                    reference writes it; with exactly two singular values above DBL_EPSILON (planar points), where that determinant is
 *                    round-off, evo's det(U) det(V) < 0 on a completed U: R is then the proper rotation.  Fewer than two (or sigma_x = 0):
 *                    the fit is degenerate and R, s, t mean nothing
 *   workspace        BS_SIMILARITY_FIT_WORKSPACE_BYTES of device memory, reused across calls on one stream
 * Two passes over the points (means, then moments about them), each a grid that writes per-block partials, each followed by a
 * one-block kernel that adds the partials in block order: four launches on `stream`, no atomics, the same bits in every run.
 *
 * bs_trajectory_metrics replaces MPEM_Metrics.compute_pose_metrics (EVALUATION/evaluation_metrics.py:136-165, which goes through evo) and
 * TrainingLoss.compute_scale_factor / compute_ARE_and_ATE / compute_RRE_and_RTE (MPEM/training_utils.py:473-585) for S trajectory pairs.
 *   gt, pred      fp64 [total_poses, 16] (device): 4x4 row-major poses, pair p being rows offsets[p] .. offsets[p + 1] - 1 of both (the
 *                 layout of bs_pose_chain's g_abs); the bottom row of a pose is not read.  Neither array is written
 *   offsets       int32 [S + 1] (device), non-decreasing, offsets[S] <= total_poses
 *   protocol      BS_TRAJ_EVO (Q = gt, P = pred; restated from evo's published definitions):
 *                   BS_TRAJ_ALIGN_ORIGIN   P_i <- Q_0 P_0^-1 P_i
 *                   BS_TRAJ_ALIGN / BS_TRAJ_CORRECT_SCALE   (R, s, t) = the similarity fit of the positions of P to those of Q (s = 1
 *                                          without CORRECT_SCALE; R = I, t = 0 without ALIGN); trans P_i <- s trans P_i, then P_i <- [R|t] P_i
 *                   ATE_i = |trans Q_i - trans P_i|; ARE_i = the angle of Q_i^-1 P_i in degrees; over the pairs (i, i + delta),
 *                   i = 0, delta, 2 delta, ... (every i with BS_TRAJ_ALL_PAIRS): E = (Q_i^-1 Q_j)^-1 (P_i^-1 P_j), RTE = |trans E|,
 *                   RRE = the angle of rot E in degrees.  Inverses are [R^T | -R^T t]; angles are acos(clip((tr - 1) / 2, -1, 1))
 *                 BS_TRAJ_TRAINING (flags are ignored, every i < n - delta is a pair):
 *                   s = sum trans Q_i . trans P_i / sum |trans P_i|^2; ATE_i = |trans Q_i - s trans P_i|; ARE_i = the angle of
 *                   rot Q_i rot P_i^T in radians; RTE / RRE: the same two errors between Q_i^-1 Q_j and P_i^-1 P_j of the unscaled poses
 *                   (general inverses, as np.linalg.inv)
 *   out           fp64 [S, BS_TRAJ_FIELDS] (device), per pair: 0 n, 1 the number of pose pairs, 2 status, 3 s, 4-12 R row-major, 13-15 t,
 *                 then rmse, mean, std (population), min, max of ATE (16-20), ARE (21-25), RTE (26-30), RRE (31-35); 36 sigma_x (training:
 *                 sum |trans P_i|^2), 37 singular values above DBL_EPSILON, 38-39 zero.  Status BS_TRAJ_DEGENERATE (fewer than two such
 *                 singular values or sigma_x = 0, where evo raises; training: sum |trans P_i|^2 = 0), BS_TRAJ_TOO_SHORT (n < delta + 1) or
 *                 BS_TRAJ_BAD_OFFSETS (the pair's offsets leave [0, total_poses]; nothing of it is read): fields 3-35 are NaN
 * The degenerate criterion is evo's absolute one.  The round-off that stands in for a vanishing singular value is about 1e-16 of the largest,
 * so a collinear path whose covariance is of order 1 (steps of metres) sits at the threshold and may report BS_TRAJ_OK, in evo as here: the
 * status is no collinearity test (field 37 and field 36 are there for a caller's own).
 * One launch on `stream` for any S (one block per pair, which walks its poses in strided loops), no workspace, no allocation, no
 * synchronisation.  A pair's record has the same bits in every run, alone or at any position of any batch. */
enum { BS_TRAJ_EVO = 0, BS_TRAJ_TRAINING = 1 };
enum { BS_TRAJ_ALIGN_ORIGIN = 1, BS_TRAJ_ALIGN = 2, BS_TRAJ_CORRECT_SCALE = 4, BS_TRAJ_ALL_PAIRS = 8 };
enum { BS_TRAJ_OK = 0, BS_TRAJ_DEGENERATE = 1, BS_TRAJ_TOO_SHORT = 2, BS_TRAJ_BAD_OFFSETS = 3 };
#define BS_TRAJ_FIELDS 40
#define BS_SIMILARITY_FIT_WORKSPACE_BYTES 131136
int bs_similarity_fit(const void* source, const void* target, int64_t n, int32_t dtype, void* workspace, int64_t workspace_bytes, double* out,
                      void* stream);
int bs_trajectory_metrics(const double* gt, const double* pred, const int32_t* offsets, int32_t S, int64_t total_poses, int32_t protocol,
                          int32_t delta, int32_t flags, double* out, void* stream);

/* ---- reconstruction evaluation: cloud-to-cloud distances ----------------------------------------------------------------------------------
 * bs_pc_query_grid / bs_pc_query_brute replace Open3D's PointCloud.compute_point_cloud_distance, the exact nearest-neighbour distance from
 * every point of one cloud to another cloud, which the reference calls at BodySLAM_not_refactored/3DM/mapping_module.py:45,48,62.  Restated
 * from Open3D's documented meaning; parity with Open3D is UNPINNED.  The statement is tests/_pointcloud_ref.py.
 * Arithmetic, fp32, no contraction: dx = s.x - t.x, dy, dz alike, d2 = (dx dx + dy dy) + dz dz; the neighbour of s is the lexicographic
 * minimum of (d2, original target index) over the finite target points; distance = sqrtf(d2), correctly rounded; index int32.  The result
 * depends on neither the order of the candidates, nor the order of the points inside a cell, nor the cell size.  A source point with a
 * non-finite coordinate gets (NaN, -1); no finite target point gives (+inf, -1).  max_distance (+inf: none; fp32): a source whose
 * distance is > max_distance gets (+inf, -1).
 *   bs_pc_bounds        replaces PointCloud.get_min_bound / get_max_bound over the finite points [n, 3] fp32 (device).  out: 8 uint32
 *                       (device): 0-2 o(min x, y, z), 3-5 ~o(max x, y, z), 6 the number of finite points, 7 zero; o(v) maps fp32 bit
 *                       patterns to uint32 in order: b | 0x80000000 for b >= 0, ~b otherwise.  No finite point: 0-5 are 0xffffffff
 *   the grid            lo, hi: host float [3], the bounds; cell_size h > 0; dims: host int32 [3] = cells per axis, their product at most
 *                       BS_PC_MAX_CELLS.  Cell coordinate along an axis: (int) min(max(floorf((x - lo) / h), 0), n - 1) in fp32; cell
 *                       index (cz ny + cy) nx + cx
 *   bs_pc_grid_count    (the build step of Open3D's KDTreeFlann, as a uniform grid) counts int32 [cells] (device, zeroed by the caller) +=
 *                       the finite points per cell.  The caller scans: cell_start int32 [cells + 1] (exclusive, cell_start[cells] =
 *                       n_records), and hands a copy of it as `cursor` to
 *   bs_pc_grid_scatter  records [n_records] of 16 bytes (x, y, z, the bit pattern of the original index), in cell order; the order inside a
 *                       cell is whatever the atomics gave
 *   bs_pc_query_grid    (KDTreeFlann.search_knn_vector_3d with k = 1, per source point) one thread per source [m, 3] fp32 (device) over
 *                       the Chebyshev shells of cells around its (clamped) cell until the best d2 is below the square of a conservative
 *                       bound on everything unvisited (csrc/pointcloud.hip derives it), every cell has been seen, or the shell covers
 *                       max_distance.  A source still searching after shell `shell_cap` is appended to fallback_list int32 [m] (device),
 *                       fallback_count int32 [1] (device, zeroed by the call) counts them; their dist / index are NOT written:
 *   bs_pc_query_brute   finishes them -- list int32 [m] (device) of source indices, or NULL for the sources 0 .. m - 1 -- by brute force
 *                       over the records (LDS tiles of 1024 records, 16-byte LDS reads).  keys: m * 8 bytes of device scratch
 *   bs_pc_transform     (PointCloud.transform / scale) out fp32 [n, 3] = the rows of [A | t] (affine: 12 host doubles, row-major 3 x 4)
 *                       applied to source [n, 3] (BS_F32 or BS_F64) in fp64, ((a0 p0 + a1 p1) + a2 p2) + t, rounded once to fp32
 *   bs_pc_stats         (np.mean / np.median / ... over the distance array the reference gets back) over dist fp32 [n] (device), out
 *                       BS_PC_STATS_FIELDS doubles (device): 0 n, 1 finite entries, 2 infinite entries (unmatched), 3 NaN entries, and over
 *                       the finite ones 4 the sum, 5 the sum of squares (fp64), 6 the max, 7 the exact median (for an even count
 *                       ((double) a + (double) b) / 2; radix selection on the bit patterns), 8-15 the count of d < thresholds[k] compared
 *                       in fp32 (host float [n_thresholds <= BS_PC_MAX_THRESHOLDS]); 6 and 7 are NaN without a finite entry.  The sums are
 *                       added in an order fixed by n alone: the same bits in every run.  workspace: BS_PC_STATS_WORKSPACE_BYTES of
 *                       device memory, 128-byte aligned.  Six launches and one memset
 * 1 <= n, m < 2^31.  No floating-point atomics anywhere. */
#define BS_PC_MAX_CELLS (1 << 24)
#define BS_PC_MAX_THRESHOLDS 8
#define BS_PC_STATS_FIELDS 16
#define BS_PC_STATS_WORKSPACE_BYTES 163968
int bs_pc_bounds(const float* points, int64_t n, uint32_t* out, void* stream);
int bs_pc_grid_count(const float* points, int64_t n, const float* lo, const float* hi, float cell_size, const int32_t* dims, int32_t* counts,
                     void* stream);
int bs_pc_grid_scatter(const float* points, int64_t n, const float* lo, const float* hi, float cell_size, const int32_t* dims, int32_t* cursor,
                       int64_t n_records, void* records, void* stream);
int bs_pc_query_grid(const void* records, const int32_t* cell_start, int64_t n_records, const float* lo, const float* hi, float cell_size,
                     const int32_t* dims, const float* source, int64_t m, float max_distance, int32_t shell_cap, float* dist, int32_t* index,
                     int32_t* fallback_list, int32_t* fallback_count, void* stream);
int bs_pc_query_brute(const void* records, int64_t n_records, const float* source, const int32_t* list, int64_t m, float max_distance, void* keys,
                      float* dist, int32_t* index, void* stream);
int bs_pc_transform(const void* source, int32_t dtype, int64_t n, const double* affine, float* out, void* stream);
int bs_pc_stats(const float* dist, int64_t n, const float* thresholds, int32_t n_thresholds, void* workspace, int64_t workspace_bytes, double* out,
                void* stream);

/* ---- k nearest neighbours, normal estimation, statistical outlier removal --------------------------------------------------------------
 * bs_pc_query_knn replaces Open3D's KDTreeFlann.search_knn_vector_3d and search_hybrid_vector_3d, bs_pc_normals PointCloud.estimate_normals
 * (the reference calls it at BodySLAM_not_refactored/3DM/mapping_module.py:184; Open3D's default search there is k-NN with k = 30), and
 * bs_pc_knn_mean_distance with bs_pc_stats PointCloud.remove_statistical_outlier (mapping_module.py:87, nb_neighbors = 20, std_ratio = 2).
 * Restated from Open3D's documented meaning; parity with Open3D is UNPINNED.  The statement is tests/_knn_ref.py.
 *   neighbours      the arithmetic of the block above: d2 = (dx dx + dy dy) + dz dz in fp32, no contraction; the neighbours of a source are
 *                   the k lexicographically smallest (d2, original target index) among the finite target points, ascending.  With a radius
 *                   (hybrid search; +inf: none) a candidate counts only when sqrtf(d2) <= radius, compared in fp32 -- the comparison
 *                   max_distance uses; a target at exactly the radius is in.  A source that is the target's own point finds itself first
 *                   (d2 = 0), as in Open3D.  1 <= k <= BS_PC_KNN_MAX.  For k = 1 the result is bs_pc_query_grid's.  Every neighbour
 *                   within a radius, however many: bs_pc_radius_* below
 *   bs_pc_query_knn one thread per source [m, 3] fp32 (device) over the index of bs_pc_grid_scatter: the Chebyshev shells of
 *                   bs_pc_query_grid (the same device function) keeping the k best in registers, until the list is full and its worst d2
 *                   is strictly below the square of the bound on everything unvisited, every cell has been seen, or the shell covers
 *                   the radius.  No shell cap and no brute-force fallback: a source far from every target, or a k above the number of
 *                   targets in reach, walks on until one of the three holds (time, never the result).  index int32 [m, k] padded with
 *                   -1, d2 fp32 [m, k] padded with +inf, count int32 [m] (all device); a source with a non-finite coordinate gets count
 *                   0, index -1 and d2 NaN.  The radius becomes an fp32 cut-off on d2 on the host: the largest d2 with
 *                   sqrtf(d2) <= radius
 *   bs_pc_normals   one thread per point of points [n, 3] fp32 (device) with the lists index / count [n, k] of the cloud's query on
 *                   itself, in fp64 over the neighbours j = 0 .. count - 1 in list order: q_j = (double) t[idx_j] - (double) p,
 *                   S = sum q_j, M = sum q_j q_j^T added sequentially (one product and one add each, no contraction),
 *                   C = M / count - (S / count)(S / count)^T, the 3 x 3 Jacobi SVD of C (symmetric PSD: its singular triplets are the
 *                   eigenpairs); the normal is the normalised column of V with the smallest singular value (ties: the lowest column),
 *                   rounded to fp32 once at the end.  Zero when count < 3 or the largest eigenvalue is not positive and finite (the
 *                   convention of bs_icp_step: a zero normal leaves its pairs out); for exactly collinear neighbours the direction is
 *                   unspecified (finite, and unit or zero).  Sign: BS_PC_ORIENT_DIRECTION flips when n . v < 0, BS_PC_ORIENT_CAMERA when
 *                   n . (v - p) < 0 (fp64; vector: 3 host doubles), BS_PC_ORIENT_AXIS makes the component of largest magnitude positive
 *                   (the first such on ties).  eigenvalues: NULL, or fp64 [n, 3] (device), ascending (zeros for an empty list)
 *   bs_pc_knn_mean_distance   one thread per row: avg fp32 [m] = fl32((sum_j (double) sqrtf(d2[i, j])) / count[i]), j = 0 .. count - 1 in
 *                   order; NaN for an empty list.  The outlier rule is the caller's: bs_pc_stats over avg gives n, sum and sum of squares;
 *                   mean = sum / n, std = sqrt(max(sumsq - n mean^2, 0) / (n - 1)) (0 for n < 2), a point is kept when
 *                   (double) avg < mean + std_ratio std
 * No floating-point atomics: the same bits in every run, for every cell size. */
#define BS_PC_KNN_MAX 32
enum { BS_PC_ORIENT_AXIS = 0, BS_PC_ORIENT_DIRECTION = 1, BS_PC_ORIENT_CAMERA = 2 };
int bs_pc_query_knn(const void* records, const int32_t* cell_start, int64_t n_records, const float* lo, const float* hi, float cell_size,
                    const int32_t* dims, const float* source, int64_t m, int32_t k, float radius, int32_t* index, float* d2, int32_t* count,
                    void* stream);
int bs_pc_normals(const float* points, int64_t n, const int32_t* index, const int32_t* count, int32_t k, int32_t orientation,
                  const double* vector, float* normals, double* eigenvalues, void* stream);
int bs_pc_knn_mean_distance(const float* d2, const int32_t* count, int64_t m, int32_t k, float* avg, void* stream);

/* ---- radius search: neighbour lists, radius outliers, DBSCAN ----------------------------------------------------------------------------
 * bs_pc_radius_* replace Open3D's KDTreeFlann.search_radius_vector_3d and, with the caller's comparison, PointCloud.remove_radius_outlier;
 * bs_pc_dbscan_* replace PointCloud.cluster_dbscan.  Restated from Open3D's documented meaning; parity with Open3D is UNPINNED.  The
 * statement is tests/_radius_ref.py, DESIGN section 3.22 the argument.
 *   neighbours      the arithmetic of the blocks above: d2 = (dx dx + dy dy) + dz dz in fp32, no contraction; a finite target point is a
 *                   neighbour of a finite source when sqrtf(d2) <= radius in fp32 (a target at exactly the radius is in), decided as
 *                   d2 <= cut-off with the largest such d2 found on the host, as bs_pc_query_knn does.  A source with a non-finite
 *                   coordinate has no neighbours.  Indices refer to the target as given.  Every kernel here runs one thread per source
 *                   over the index of bs_pc_grid_scatter with the walk of bs_pc_query_grid (the same device function), no shell cap: it
 *                   ends when the shell covers the radius or every cell has been seen, so a source far from every target costs a few
 *                   shells and the cell size changes the time only
 *   bs_pc_radius_count    count int32 [m]: the neighbours of every source
 *   bs_pc_radius_fill     row_start int64 [m + 1] is the caller's exclusive scan of the counts, total = row_start[m] < 2^31; every source
 *                   writes the keys (d2 bits << 32 | index) of its neighbours to keys [row_start[i], row_start[i + 1]) in walk order.
 *                   A row whose bounds are not 0 <= row_start[i] <= row_start[i + 1] <= total, or that finds more neighbours than its
 *                   segment holds, writes nothing beyond it and sets BS_PC_RADIUS_OVERRUN in status int32 [1] (the caller zeroes it);
 *                   with counts from the same index and radius this does not happen
 *   bs_pc_radius_sort     one wave per row: keys_out [row] = the row's keys ascending -- ascending (d2, index), d2 >= 0, the order of
 *                   bs_pc_query_knn.  The keys of a row are distinct (the index half), so the order is total and does not depend on the
 *                   walk.  Rows of at most 64 keys go through a compare-exchange network over the wave, longer ones by rank counting
 *                   (keys_out[number of keys below mine] = mine).  keys_out must not alias keys
 *   bs_pc_radius_unpack   index int32 [total], d2 fp32 [total] from the keys
 *   DBSCAN          over a cloud queried on itself with count = bs_pc_radius_count(points, eps): a point is CORE when
 *                   count >= min_points (itself included; a non-finite point has count 0).  Clusters are the connected components of
 *                   the core points under "d2 <= cut-off", numbered 0, 1, ... in ascending order of their smallest core index.  A finite
 *                   non-core point with a core neighbour is a BORDER and takes the smallest cluster number among its core neighbours;
 *                   everything else is noise, label -1.  Deterministic: it is what the sequential scan in ascending index order gives
 *   bs_pc_dbscan_hook     parent int32 [n] starts as 0 .. n - 1; one thread per core point walks its neighbourhood and, for every core
 *                   neighbour of lower index, hooks the two roots by minimum as bs_mesh_cc_hook does (the same device function) and sets
 *                   changed int32 [1]
 *   bs_pc_dbscan_compress parent[i] = root(i).  The caller repeats (zero changed, hook, compress) until changed stays 0: at most n rounds
 *                   report a change.  Then parent[i] of a core point is the smallest core index of its component
 *   bs_pc_dbscan_roots    is_root int32 [n] = (i is core and parent[i] == i); the caller scans it inclusively: rank int32 [n], C = rank[n - 1]
 *   bs_pc_dbscan_labels   labels int32 [n]: a core point rank[parent[i]] - 1; any other finite point walks its neighbourhood and takes the
 *                   minimum of rank[parent[j]] - 1 over its core neighbours j, -1 without one; a non-finite point -1
 * No floating-point atomics and no LDS; every index read from memory is checked before it is used: the same bits in every run, for every
 * cell size. */
#define BS_PC_RADIUS_OVERRUN 1
int bs_pc_radius_count(const void* records, const int32_t* cell_start, int64_t n_records, const float* lo, const float* hi, float cell_size,
                       const int32_t* dims, const float* source, int64_t m, float radius, int32_t* count, void* stream);
int bs_pc_radius_fill(const void* records, const int32_t* cell_start, int64_t n_records, const float* lo, const float* hi, float cell_size,
                      const int32_t* dims, const float* source, int64_t m, float radius, const int64_t* row_start, int64_t total, void* keys,
                      int32_t* status, void* stream);
int bs_pc_radius_sort(const void* keys, const int64_t* row_start, int64_t m, int64_t total, void* keys_out, void* stream);
int bs_pc_radius_unpack(const void* keys, int64_t total, int32_t* index, float* d2, void* stream);
int bs_pc_dbscan_hook(const void* records, const int32_t* cell_start, int64_t n_records, const float* lo, const float* hi, float cell_size,
                      const int32_t* dims, const float* points, int64_t n, float eps, const int32_t* count, int32_t min_points, int32_t* parent,
                      int32_t* changed, void* stream);
int bs_pc_dbscan_compress(int32_t* parent, int64_t n, void* stream);
int bs_pc_dbscan_roots(const int32_t* parent, const int32_t* count, int32_t min_points, int64_t n, int32_t* is_root, void* stream);
int bs_pc_dbscan_labels(const void* records, const int32_t* cell_start, int64_t n_records, const float* lo, const float* hi, float cell_size,
                        const int32_t* dims, const float* points, int64_t n, float eps, const int32_t* count, int32_t min_points,
                        const int32_t* parent, const int32_t* rank, int64_t n_clusters, int32_t* labels, void* stream);

/* ---- consistent orientation of normals along a minimum spanning tree ---------------------------------------------------------------------
 * bs_pc_orient_* replace Open3D's PointCloud.orient_normals_consistent_tangent_plane (Hoppe et al. 1992).  Restated from Open3D's documented
 * meaning; parity with Open3D is UNPINNED, and no Delaunay edges are added: a disconnected k-NN graph gives several trees, each oriented on
 * its own.  The statement is tests/_orient_ref.py, DESIGN section 3.24 the argument.  All pointers are device pointers; n <= 2^30.
 *   graph           index int32 [n, k], count int32 [n]: bs_pc_query_knn of the cloud on itself.  A point is VALID when its coordinates are
 *                   finite and its normal is finite and not all zero.  The undirected edge {i, j}, i != j, exists when j is in row i or i in
 *                   row j and both are valid.  In fp64 without contraction d = (ax bx + ay by) + az bz on the fp32 normals; the weight is
 *                   w = fl32(max(1 - |d|, 0)), the sign link s = (d < 0): flip(i) xor flip(j) = s.  Edges are ordered by (the bits of w,
 *                   min(i, j), max(i, j)): a total order, so the minimum spanning forest is unique
 *   word            uint32 [n]: parent << 1 | parity, parity = flip(x) xor flip(parent); the caller starts it as x << 1.  parent <= x always:
 *                   a root walk strictly descends, at most n steps.  Every stored word is a relation implied by the links hooked so far
 *   bs_pc_orient_edges      keys [n k] of 64-bit words: w_bits << 32 | min(i, j) for a slot that is an edge, ~0 for any other; valid int32 [n]
 *   bs_pc_orient_clear      best [n] of 64-bit words = ~0; best_hi int32 [n] (NULL: none) = 0x7fffffff
 *   bs_pc_orient_select     every slot whose ends have different roots offers its key to best[] of both roots by 64-bit integer atomic
 *                   minimum and sets crossing int32 [1] (zeroed by the caller).  Offers of one wave to one root are merged into one atomic
 *   bs_pc_orient_select_hi  the crossing slots whose key equals their root's best offer max(i, j) to best_hi[] by integer atomic minimum
 *   bs_pc_orient_hook       every root r with best[r] != ~0 hooks the link (lo, hi, s) of its edge: the parities pa, pb of the walks to the
 *                   two roots, then an integer atomic minimum of (smaller root << 1 | pa ^ pb ^ s) into the larger root's word.  A hook
 *                   that loses to a smaller root is not an error: the edge is selected again in the next round
 *   bs_pc_orient_compress   word[x] = root(x) << 1 | parity to the root.  The caller repeats (zero crossing, clear, select, select_hi, hook,
 *                   compress) until a select leaves crossing 0: at most n rounds find a crossing edge
 *   bs_pc_orient_seed       seed [n] of 64-bit words (cleared to ~0 by bs_pc_orient_clear): per root the integer atomic minimum of
 *                   (~ordered bits of z) << 32 | i over its valid points -- the point of largest fp32 z (-0 as +0), ties to the lowest index
 *   bs_pc_orient_flip       the seed of a tree is flipped when (nx dx + ny dy) + nz dz < 0 in fp64; flip(x) = the seed's flip xor the parity
 *                   of x to the root xor that of the seed to the root.  out fp32 [n, 3] (not `normals`): the normal with its three sign
 *                   bits toggled where flipped, every other row bit for bit; flipped uint8 [n]
 * Integer atomics only and no retry loops: the same bits in every run, for every order of the atomics. */
int bs_pc_orient_edges(const float* points, const float* normals, int64_t n, const int32_t* index, const int32_t* count, int32_t k, void* keys,
                       int32_t* valid, void* stream);
int bs_pc_orient_clear(void* best, int32_t* best_hi, int64_t n, void* stream);
int bs_pc_orient_select(const void* keys, const int32_t* index, const uint32_t* word, int64_t n, int32_t k, void* best, int32_t* crossing,
                        void* stream);
int bs_pc_orient_select_hi(const void* keys, const int32_t* index, const uint32_t* word, int64_t n, int32_t k, const void* best, int32_t* best_hi,
                           void* stream);
int bs_pc_orient_hook(const float* normals, uint32_t* word, int64_t n, const void* best, const int32_t* best_hi, void* stream);
int bs_pc_orient_compress(uint32_t* word, int64_t n, void* stream);
int bs_pc_orient_seed(const float* points, const int32_t* valid, const uint32_t* word, int64_t n, void* seed, void* stream);
int bs_pc_orient_flip(const float* normals, const int32_t* valid, const uint32_t* word, int64_t n, const void* seed, double dx, double dy, double dz,
                      float* out, uint8_t* flipped, void* stream);

/* ---- voxel down-sampling -----------------------------------------------------------------------------------------------------------------
 * The four bs_pc_voxel_* launches replace Open3D's PointCloud.voxel_down_sample, which the reference calls at
 * BodySLAM_not_refactored/3DM/mapping_module.py:72,156,187 (0.005, 0.009 and 0.05 m), and return what voxel_down_sample_and_trace is used
 * for as three index arrays.  Restated from Open3D's documented meaning; parity with Open3D is UNPINNED, and Open3D's own trace format (the
 * [m, 8] cubic-id matrix) is not built.  The statement is tests/_voxel_ref.py.  points [n, 3] fp32 (device); a point with a non-finite
 * coordinate belongs to no voxel.  The caller computes, on the host, from bs_pc_bounds' lo and hi and the voxel size h (a double):
 * origin o = (double) lo - 0.5 h (3 host doubles); that floor(((double) hi - o) / h) < 2^BS_PC_VOXEL_AXIS_BITS on every axis; and the
 * shift s = 32 - e, where max over the axes of (double) hi - o = f 2^e with 0.5 <= f < 1.
 *   voxel           v = floor(((double) p - o) / h) per axis in fp64, one subtraction and one division, no contraction;
 *                   key = vz << 42 | vy << 21 | vx
 *   rows            in order of first appearance: row r is the voxel whose lowest point index is the r-th smallest
 *   position        Q = rint(ldexp((double) p - o, s)) as int64, 0 <= Q <= 2^32; S = sum Q over the voxel, exact;
 *                   fl32(o + ldexp((double) S / (double) count, -s)).  A voxel of exactly one point returns that point's bits (and its
 *                   colour's and normal's; unit_normals excepted)
 *   colours, normals   Q = rint((double) a 2^30); every component of a point in a voxel must be finite with |a| <= 2, else the status bit
 *                   BS_PC_VOXEL_BAD_ATTRIBUTE; fl32(ldexp((double) S / (double) count, -30)), the plain mean.  unit_normals: the three
 *                   means d scaled by 1 / sqrt((d0 d0 + d1 d1) + d2 d2) in fp64 before the rounding, zero when the length is not positive
 *   bs_pc_voxel_assign      one thread per point inserts its key into the table keys [slots] of 64-bit words (device; filled with
 *                   BS_PC_VOXEL_EMPTY_KEY by the caller) by compare-and-swap with linear probing, takes the minimum of its index into
 *                   first int32 [slots] (device; filled with BS_PC_VOXEL_NO_POINT by the caller) and stores slot_of_point int32 [n]
 *                   (-1: in no voxel).  slots: a power of two above n.  After `slots` probes without a free slot or a match the thread sets
 *                   BS_PC_VOXEL_TABLE_FULL and gives up: no loop is unbounded.  A voxel coordinate outside [0, 2^21) -- an origin that
 *                   does not belong to the points -- sets BS_PC_VOXEL_OUT_OF_RANGE.  status int32 [1] (device, zeroed by the caller)
 *   bs_pc_voxel_flags       leader int32 [n] = first[slot_of_point] (-1: none), is_first int32 [n] = (leader == the point's index).  The
 *                   caller scans is_first inclusively: rank int32 [n]; the voxel led by point j is row rank[j] - 1, and m = rank[n - 1]
 *   bs_pc_voxel_accumulate  one thread per point adds its 3, 6 or 9 terms (position, then colours, then normals; colors / normals NULL when
 *                   absent) to sums [m, terms] of 64-bit words and 1 to counts int32 [m] (device, both zeroed by the caller) with integer
 *                   atomics; a run of adjacent lanes of a wave with the same row is summed in the wave first and its last lane issues the
 *                   atomics (integer addition is associative: the same sums).  Writes row_of_point int32 [n] (-1: in no voxel) and
 *                   first_index int32 [m]
 *   bs_pc_voxel_finish      one thread per row: out_points fp32 [m, 3], out_colors / out_normals fp32 [m, 3] or NULL with their inputs
 * No floating-point atomics, and the phases are separate launches: the same bits in every run, for every table size and every slot. */
#define BS_PC_VOXEL_AXIS_BITS 21
#define BS_PC_VOXEL_EMPTY_KEY 0xffffffffffffffffull
#define BS_PC_VOXEL_NO_POINT 0x7fffffff
enum { BS_PC_VOXEL_TABLE_FULL = 1, BS_PC_VOXEL_OUT_OF_RANGE = 2, BS_PC_VOXEL_BAD_ATTRIBUTE = 4 };
int bs_pc_voxel_assign(const float* points, int64_t n, const double* origin, double voxel_size, void* keys, int32_t* first, int64_t slots,
                       int32_t* slot_of_point, int32_t* status, void* stream);
int bs_pc_voxel_flags(const int32_t* slot_of_point, const int32_t* first, int64_t slots, int64_t n, int32_t* leader, int32_t* is_first,
                      void* stream);
int bs_pc_voxel_accumulate(const float* points, const float* colors, const float* normals, int64_t n, const double* origin, int32_t shift,
                           const int32_t* leader, const int32_t* rank, int64_t m, void* sums, int32_t* counts, int32_t* first_index,
                           int32_t* row_of_point, int32_t* status, void* stream);
int bs_pc_voxel_finish(const float* points, const float* colors, const float* normals, int64_t n, const void* sums, const int32_t* counts,
                       const int32_t* first_index, int64_t m, const double* origin, int32_t shift, int32_t unit_normals, float* out_points,
                       float* out_colors, float* out_normals, void* stream);

/* ---- triangle-mesh scene: ray casting, closest points, surface samples -----------------------------------------------------------------
 * The bs_mesh_* launches replace Open3D's t.geometry.RaycastingScene (add_triangles, cast_rays, compute_closest_points, compute_distance)
 * and TriangleMesh.sample_points_uniformly, which the reference calls at BodySLAM_not_refactored/3DM/mapping_module.py:204-237,289 and
 * 3DM/synthetic_depth_generator.py:24-97.  Restated from Open3D's documented interface; parity with Open3D / Embree is UNPINNED.  The
 * statement is tests/_mesh_scene_ref.py; the arithmetic is at the top of csrc/mesh_scene.hip, and every result is bit-equal to the statement.
 * All pointers are device pointers.  A scene is the concatenation of its geometries: vertices fp32 [V, 3], triangles int32 [T, 3] with the
 * indices of later geometries already offset; geom_start int32 [n_geom + 1] holds the first global triangle of every geometry and T.
 *   bs_mesh_records        records: 3 T 16-byte words -- (v0, bit-cast global index, -1 when the triangle is not kept), (v1, 0), (v2, 0).
 *                          Not kept: a non-finite vertex, a non-finite or zero fp32 cross product, an index outside [0, V) (the caller
 *                          refuses those first; the kernel never reads outside `vertices`).  kept int32 [1]: how many are
 *   bs_mesh_cast_brute     rays fp32 [*, 6] (origin, direction; the direction is not normalised); list int32 [m] of ray rows or NULL for the
 *                          rows 0 .. m - 1; keys: m 64-bit words of scratch.  Per listed ray, the minimum of (t, global index) over the kept
 *                          triangles: t_hit fp32 in units of |d| (+inf: a miss), geometry_ids and primitive_ids int32 (-1, the bit pattern
 *                          0xFFFFFFFF: a miss; primitive ids are local to their geometry), primitive_uvs fp32 [*, 2] with
 *                          p = (1 - u - v) v0 + u v1 + v v2, primitive_normals fp32 [*, 3] = the unit (v1 - v0) x (v2 - v0), not turned
 *                          towards the ray, zero for a miss.  A ray with a non-finite component or a zero direction is a miss
 *   bs_mesh_closest_brute  query fp32 [*, 3]; list and keys as above.  Per listed point, the minimum of (d2, global index): points fp32
 *                          [*, 3], distance = sqrt(d2), the ids and uvs as above.  Nothing within max_distance (compared with the fp32
 *                          distance; +inf for none), or no kept triangle: points NaN, distance +inf, ids -1, uvs 0.  A non-finite query:
 *                          points and distance NaN, ids -1
 *   bs_mesh_sample_weights area fp64 [T] and top (one 64-bit word) are scratch; weights int64 [T] = floor(area / max area 2^40), 0 for a
 *                          triangle that is not kept.  The caller scans them inclusively (integers: exact): cum int64 [T]
 *   bs_mesh_sample         samples first .. first + n - 1 of the stream `seed`: points, normals fp32 [n, 3], index int32 [n] (the global
 *                          triangle), and colors fp32 [n, 3] from vertex_colors fp32 [V, 3] through triangles (all three NULL together).
 *                          cum[T - 1] must be positive.  A sample depends on (seed, its number) alone
 *   bs_mesh_grid_count / _scatter   the index: a uniform grid over lo, hi (host float [3]: the bounds of the kept triangles' vertices) with the
 *                          point grid's cell function (bs_pc_grid_count); a kept triangle is referenced from every cell between
 *                          cell(min - pad) and cell(max + pad) per axis.  counts int32 [cells] zeroed by the caller, who scans them; cursor: a
 *                          copy of the exclusive scan; refs int32 [n_refs].  The order of the references in a cell is not fixed and no result
 *                          depends on it.  pad >= 2^-9 of the largest extent + 2^-14 (max |lo|, |hi| + that extent): the bound at the top of
 *                          csrc/mesh_scene.hip stands on it
 *   bs_mesh_cast_grid      one thread per ray walks the cells from the ray's entry into the box (a 3-D DDA, at most nx + ny + nz + 3 steps) and
 *                          writes bs_mesh_cast_brute's outputs, the same bits; a ray with an origin coordinate beyond origin_limit (8 times
 *                          max |lo|, |hi| + the extent) or a direction component outside 2^-60 .. 2^60 goes onto fallback_list int32 [m]
 *                          (fallback_count int32 [1]) for bs_mesh_cast_brute with that list
 *   bs_mesh_closest_grid   one thread per point walks the Chebyshev shells of the point grid (pc_walk) over the references; a point still
 *                          searching after shell_cap goes onto the list for bs_mesh_closest_brute
 *   bs_mesh_hits_grid      every hit of a ray, not the nearest -- Open3D's RaycastingScene.count_intersections, list_intersections and
 *                          test_occlusions (compute_occupancy and compute_signed_distance are composed from the counts); parity UNPINNED, the
 *                          statement is tests/_mesh_hits_ref.py.  The walk of bs_mesh_cast_grid without its early stop; a triangle is tested
 *                          only in the first visited cell of its cell range, so every hit is met exactly once.  tnear <= t <= tfar (not NaN).
 *                          mode BS_MESH_HITS_COUNT: out int32 [m] = the hits of the COUNTING predicate -- cast_rays' arithmetic, except that an
 *                          edge value of exactly 0 takes the sign it would have with the ray moved by (eps, eps^2) in the sheared plane, so
 *                          that exactly one of the triangles at a shared edge or vertex claims the ray.  BS_MESH_HITS_ANY: out = 1 when the
 *                          CLOSED predicate of bs_mesh_cast_grid has a hit (Open3D's test_occlusions; with tnear 0, tfar +inf it is
 *                          t_hit < inf of that call), else 0.  BS_MESH_HITS_FILL: row_start int64 [m + 1] is the caller's exclusive scan of
 *                          COUNT's out, total = row_start[m] in [1, 2^31); the keys (t bits << 32 | global index) of a ray's hits go to keys
 *                          [row_start[i], row_start[i + 1]) in walk order, nothing beyond the segment.  The caller sorts the rows with
 *                          bs_pc_radius_sort (t >= +0: the key order is the order of (t, index)).  The pointers a mode does not use may be NULL.
 *                          Rays the padding does not cover go onto fallback_list with out = 0, as in bs_mesh_cast_grid
 *   bs_mesh_hits_brute     the same three modes for the rays of list (or the rows 0 .. m - 1) against every triangle: COUNT adds to out [n_rows]
 *                          (integer atomics; zeroed here without a list, by bs_mesh_hits_grid with one), FILL takes slots from cursor int32 [m]
 *                          (zeroed here), so the order inside a row is not fixed before the sort.  Parity UNPINNED as above
 *   bs_mesh_hits_unpack    row j of the sorted keys, ray_ids int64 [total] (the ray of every row): the triangle is evaluated again under the
 *                          counting predicate -- t_hit, geometry_ids, primitive_ids [total], primitive_uvs [total, 2] as bs_mesh_cast_brute
 *                          writes them (Open3D's list_intersections; parity UNPINNED)
 * list rows are checked against n_rows, the rows of the ray / query array.  No floating-point atomics: the same bits in every run, for every
 * cell size.  Not built: BVHs, a fused pinhole kernel. */
enum { BS_MESH_HITS_COUNT = 0, BS_MESH_HITS_ANY = 1, BS_MESH_HITS_FILL = 2 };
#define BS_MESH_MAX_TRIANGLES 536870912         /* 2^29 */
#define BS_MESH_MAX_SAMPLED_TRIANGLES (1 << 22)
int bs_mesh_records(const float* vertices, int64_t n_vertices, const int32_t* triangles, int64_t n_triangles, void* records, int32_t* kept,
                    void* stream);
int bs_mesh_cast_brute(const void* records, int64_t n_triangles, const float* rays, int64_t n_rows, const int32_t* list, int64_t m, void* keys,
                       const int32_t* geom_start, int32_t n_geom, float* t_hit, int32_t* geometry_ids, int32_t* primitive_ids,
                       float* primitive_uvs, float* primitive_normals, void* stream);
int bs_mesh_closest_brute(const void* records, int64_t n_triangles, const float* query, int64_t n_rows, const int32_t* list, int64_t m,
                          float max_distance,
                          void* keys, const int32_t* geom_start, int32_t n_geom, float* points, float* distance, int32_t* geometry_ids,
                          int32_t* primitive_ids, float* primitive_uvs, void* stream);
int bs_mesh_grid_count(const void* records, int64_t n_triangles, const float* lo, const float* hi, float cell_size, const int32_t* dims, float pad,
                       int32_t* counts, void* stream);
int bs_mesh_grid_scatter(const void* records, int64_t n_triangles, const float* lo, const float* hi, float cell_size, const int32_t* dims, float pad,
                         int32_t* cursor, int64_t n_refs, int32_t* refs, void* stream);
int bs_mesh_cast_grid(const void* records, int64_t n_triangles, const int32_t* refs, const int32_t* cell_start, const float* lo, const float* hi,
                      float cell_size, const int32_t* dims, float pad, float origin_limit, const float* rays, int64_t m, const int32_t* geom_start,
                      int32_t n_geom, float* t_hit, int32_t* geometry_ids, int32_t* primitive_ids, float* primitive_uvs, float* primitive_normals,
                      int32_t* fallback_list, int32_t* fallback_count, void* stream);
int bs_mesh_closest_grid(const void* records, int64_t n_triangles, const int32_t* refs, const int32_t* cell_start, const float* lo, const float* hi,
                         float cell_size, const int32_t* dims, float pad, const float* query, int64_t m, float max_distance, int32_t shell_cap,
                         const int32_t* geom_start, int32_t n_geom, float* points, float* distance, int32_t* geometry_ids, int32_t* primitive_ids,
                         float* primitive_uvs, int32_t* fallback_list, int32_t* fallback_count, void* stream);
int bs_mesh_hits_grid(const void* records, int64_t n_triangles, const int32_t* refs, const int32_t* cell_start, const float* lo, const float* hi,
                      float cell_size, const int32_t* dims, float pad, float origin_limit, const float* rays, int64_t m, int32_t mode, float tnear,
                      float tfar, int32_t* out, const int64_t* row_start, int64_t total, void* keys, int32_t* fallback_list,
                      int32_t* fallback_count, void* stream);
int bs_mesh_hits_brute(const void* records, int64_t n_triangles, const float* rays, int64_t n_rows, const int32_t* list, int64_t m, int32_t mode,
                       float tnear, float tfar, int32_t* out, const int64_t* row_start, int64_t total, void* keys, int32_t* cursor, void* stream);
int bs_mesh_hits_unpack(const void* records, int64_t n_triangles, const float* rays, int64_t n_rows, const void* keys, const int64_t* ray_ids,
                        int64_t total, const int32_t* geom_start, int32_t n_geom, float* t_hit, int32_t* geometry_ids, int32_t* primitive_ids,
                        float* primitive_uvs, void* stream);
int bs_mesh_sample_weights(const void* records, int64_t n_triangles, double* area, void* top, int64_t* weights, void* stream);
int bs_mesh_sample(const void* records, int64_t n_triangles, const int64_t* cum, const int32_t* triangles, const float* vertex_colors,
                   int64_t n_vertices, uint64_t seed, uint64_t first, int64_t n, float* points, float* colors, float* normals, int32_t* index,
                   void* stream);

/* ---- mesh topology and clean-up: edges, components, normals, smoothing -----------------------------------------------------------------
 * These launches replace Open3D's TriangleMesh.cluster_connected_triangles, get_non_manifold_edges / is_edge_manifold,
 * compute_triangle_normals, compute_vertex_normals, get_surface_area, filter_smooth_laplacian and filter_smooth_taubin: what everyone runs on
 * a TSDF mesh before reporting a number.  Restated from Open3D's documented meaning; parity with Open3D is UNPINNED.  The statement is
 * tests/_mesh_ops_ref.py, and every result is bit-equal to it.  All pointers are device pointers.  vertices fp32 [V, 3], triangles int32
 * [T, 3], T <= BS_MESH_MAX_TRIANGLES.  A triangle is VALID when its three indices lie in [0, V) and are pairwise distinct; an invalid one
 * takes part in nothing.  A valid triangle is KEPT under bs_mesh_records' rule (finite vertices, a finite non-zero fp32 cross product).
 * Half-edge h = 3 t + c runs from a = tri[t][c] to b = tri[t][(c + 1) % 3]; its key is min(a, b) << 32 | max(a, b).
 *   bs_mesh_edge_insert    one thread per half-edge of a valid triangle inserts its key into keys [slots] of 64-bit words (filled with
 *                          BS_MESH_EDGE_EMPTY_KEY by the caller) by compare-and-swap with linear probing, then, integer atomics on the slot:
 *                          first_half int32 [slots] (filled with BS_MESH_EDGE_NO_HALF) takes the minimum of h, count int32 [slots] (zeroed)
 *                          one, forward int32 [slots] (zeroed) one when a < b.  slot_of_half int32 [3 T] (-1: an invalid triangle, or no
 *                          slot).  slots: a power of two; the default is the smallest above 3 T.  After `slots` probes without a free slot or
 *                          a match the thread sets BS_MESH_EDGE_TABLE_FULL in status[0] and gives up: no loop is unbounded.  status int32 [2]
 *                          (zeroed by the caller); status[1] counts the invalid triangles
 *   bs_mesh_edge_flags     leader int32 [3 T] = first_half[slot_of_half] (-1: none), is_first int32 [3 T] = (leader == h).  The caller scans
 *                          is_first inclusively: rank int32 [3 T]; the edge led by half-edge j is row rank[j] - 1, E = rank[3 T - 1]: edges in
 *                          the order of their first half-edge
 *   bs_mesh_edge_rows      edges int32 [E, 2] (min, max), edge_count, edge_forward, edge_first_triangle int32 [E], edge_of_half int32 [3 T]
 *                          (-1 for the half-edges of an invalid triangle)
 *   bs_mesh_cc_hook        components of valid triangles that share an edge.  parent int32 [T] starts as 0 .. T - 1 and only decreases, so
 *                          parent[x] <= x and a root walk strictly descends (at most T steps).  One thread per half-edge: the roots of its
 *                          triangle and of its edge's first triangle; when they differ, an integer atomic minimum of the smaller root into
 *                          the larger root's parent, and changed int32 [1] = 1
 *   bs_mesh_cc_compress    parent[t] = root(t).  The caller repeats (zero changed, hook, compress) until changed stays 0: every round that
 *                          reports a change turns a root into a non-root for good, so at most T rounds report one.  Then parent[t] is the
 *                          smallest triangle index of t's component, whatever the schedule
 *   bs_mesh_cc_roots       is_root int32 [T] = (t is valid and parent[t] == t); the caller scans it inclusively: rank int32 [T], C = rank[T - 1]
 *   bs_mesh_cc_clusters    triangle_clusters int32 [T] = rank[parent[t]] - 1 (-1: invalid): clusters in the order of their first triangle;
 *                          cluster_n_triangles int32 [C] (zeroed) by integer atomics
 *   bs_mesh_segment_sum    out[s] = the sum of values[start[s] .. start[s + 1]) (fp64; start int64 [n_segments + 1]) by one wave: lane l adds
 *                          elements l, l + 64, ... in order from +0.0, then lanes are added across by xor 32, 16, 8, 4, 2, 1.  Cluster areas
 *                          (the areas gathered by a stable sort of the clusters) and the surface area (one segment)
 *   bs_mesh_triangle_geometry   any of (NULL: not wanted) flags int32 [T] (BS_MESH_TRIANGLE_VALID | BS_MESH_TRIANGLE_KEPT), normals fp32 [T, 3]
 *                          (bs_mesh_sample's unit normal, zero when not kept), cross fp64 [T, 3] (the fp64 cross product of the fp64 differences
 *                          of the fp32 vertices, zero when not kept) and area fp64 [T] = 0.5 sqrt((nx nx + ny ny) + nz nz) of it
 *   bs_mesh_vertex_normals corner_order int64 [3 T]: the corners 3 t + c stably sorted by vertex (those of invalid triangles last);
 *                          vertex_start int64 [V + 1].  One thread per vertex adds `cross` of its corners' triangles in that order in fp64,
 *                          scales by the largest |component|, normalises and rounds once: normals fp32 [V, 3], zero when the sum is zero
 *   bs_mesh_laplacian_step one thread per vertex: mean = (the fp64 sum of in[nbr[nbr_start[v] .. nbr_start[v + 1])] in order) / count,
 *                          out = fl32(v + lambda (mean - v)) in fp64, clamped to [0, 1] before the rounding when `clamp`; a vertex without
 *                          neighbours is copied.  in and out fp32 [V, 3], distinct buffers
 *   bs_mesh_orient_*       the winding (Open3D's is_orientable / orient_triangles; the statement is tests/_orient_ref.py, DESIGN section
 *                          3.24).  Every edge with edge_count == 2 links its two triangles with s = (edge_forward != 1): flip(t) xor
 *                          flip(u) = s.  Edges with any other count link nothing and connect nothing.  word uint32 [T] = parent << 1 |
 *                          parity as for bs_pc_orient_hook (the same device functions), started as t << 1 by the caller
 *   bs_mesh_orient_hook    one thread per half-edge hooks the link of its triangle and its edge's first triangle; changed int32 [1] = 1
 *                          when the roots differed
 *   bs_mesh_orient_compress word[t] = root(t) << 1 | parity to the root.  The caller repeats (zero changed, hook, compress) until changed
 *                          stays 0, at most T rounds report a change
 *   bs_mesh_orient_check   re-tests every link against the stored parities: a violated link sets bad int32 [T] (zeroed by the caller) at
 *                          its root -- that component is not orientable
 *   bs_mesh_orient_flip    out int32 [T, 3] (not `triangles`): [a, c, b] for a valid triangle of an orientable component whose parity to the
 *                          component's smallest triangle is 1, every other row unchanged; flipped uint8 [T]
 * No floating-point atomics and no retry loops: the same bits in every run, for every table size and every order of the atomics.  Not built:
 * simplification, subdivision, hole filling. */
#define BS_MESH_EDGE_EMPTY_KEY 0xffffffffffffffffull
#define BS_MESH_EDGE_NO_HALF 0x7fffffff
enum { BS_MESH_EDGE_TABLE_FULL = 1 };
enum { BS_MESH_TRIANGLE_VALID = 1, BS_MESH_TRIANGLE_KEPT = 2 };
int bs_mesh_edge_insert(const int32_t* triangles, int64_t n_triangles, int64_t n_vertices, void* keys, int32_t* first_half, int32_t* count,
                        int32_t* forward, int64_t slots, int32_t* slot_of_half, int32_t* status, void* stream);
int bs_mesh_edge_flags(const int32_t* slot_of_half, const int32_t* first_half, int64_t slots, int64_t n_half, int32_t* leader, int32_t* is_first,
                       void* stream);
int bs_mesh_edge_rows(const int32_t* triangles, int64_t n_triangles, const int32_t* slot_of_half, const int32_t* count, const int32_t* forward,
                      int64_t slots, const int32_t* leader, const int32_t* rank, int64_t n_edges, int32_t* edges, int32_t* edge_count,
                      int32_t* edge_forward, int32_t* edge_first_triangle, int32_t* edge_of_half, void* stream);
int bs_mesh_cc_hook(const int32_t* edge_of_half, const int32_t* edge_first_triangle, int64_t n_triangles, int64_t n_edges, int32_t* parent,
                    int32_t* changed, void* stream);
int bs_mesh_cc_compress(int32_t* parent, int64_t n_triangles, void* stream);
int bs_mesh_cc_roots(const int32_t* parent, const int32_t* edge_of_half, int64_t n_triangles, int32_t* is_root, void* stream);
int bs_mesh_cc_clusters(const int32_t* parent, const int32_t* edge_of_half, const int32_t* rank, int64_t n_triangles, int64_t n_clusters,
                        int32_t* triangle_clusters, int32_t* cluster_n_triangles, void* stream);
int bs_mesh_orient_hook(const int32_t* edge_of_half, const int32_t* edge_count, const int32_t* edge_forward, const int32_t* edge_first_triangle,
                        int64_t n_triangles, int64_t n_edges, uint32_t* word, int32_t* changed, void* stream);
int bs_mesh_orient_compress(uint32_t* word, int64_t n_triangles, void* stream);
int bs_mesh_orient_check(const int32_t* edge_of_half, const int32_t* edge_count, const int32_t* edge_forward, const int32_t* edge_first_triangle,
                         int64_t n_triangles, int64_t n_edges, const uint32_t* word, int32_t* bad, void* stream);
int bs_mesh_orient_flip(const int32_t* triangles, const int32_t* edge_of_half, const uint32_t* word, const int32_t* bad, int64_t n_triangles,
                        int32_t* out, uint8_t* flipped, void* stream);
int bs_mesh_segment_sum(const double* values, int64_t n_values, const int64_t* start, int64_t n_segments, double* out, void* stream);
int bs_mesh_triangle_geometry(const float* vertices, int64_t n_vertices, const int32_t* triangles, int64_t n_triangles, int32_t* flags,
                              float* normals, double* cross, double* area, void* stream);
int bs_mesh_vertex_normals(const double* cross, int64_t n_triangles, const int64_t* corner_order, const int64_t* vertex_start, int64_t n_vertices,
                           float* normals, void* stream);
int bs_mesh_laplacian_step(const float* in, int64_t n_vertices, const int64_t* nbr_start, const int32_t* nbr, int64_t n_nbr, double lambda,
                           int32_t clamp, float* out, void* stream);

/* ---- is this mesh a solid (csrc/mesh_solid.hip) ----------------------------------------------------------------------------------------
 * The roles of Open3D's TriangleMesh.get_non_manifold_vertices, is_vertex_manifold, get_self_intersecting_triangles, is_self_intersecting,
 * is_intersecting, is_watertight and get_volume.  Restated from Open3D's documented meaning; parity with Open3D is UNPINNED.  The statement
 * is tests/_mesh_solid_ref.py and every result equals it, in every run and for every grid; DESIGN section 3.26 is the argument.  All
 * pointers are device pointers; VALID and KEPT are those of the mesh clean-up above.
 *   bs_mesh_fan_hook       the elements are the corners 3 t + c of the valid triangles.  parent int32 [3 T] starts as 0 .. 3 T - 1.  One
 *                          thread per half-edge h = 3 t + c (a = tri[t][c] -> b = tri[t][(c + 1) % 3]) of edge e with first triangle u =
 *                          edge_first_triangle[e] hooks the corner of a in t with the corner of a in u, and likewise for b, by minimum as
 *                          bs_mesh_cc_hook does (the same device function); changed int32 [1] = 1 when two roots differed.  An edge of three
 *                          or more triangles joins them all
 *   bs_mesh_fan_compress   parent[x] = root(x).  The caller repeats (zero changed, hook, compress) until changed stays 0: at most 3 T rounds
 *                          report a change
 *   bs_mesh_fan_count      count int32 [V] (zeroed) += 1 for every root corner of a valid triangle at the vertex: a vertex is NON-MANIFOLD iff
 *                          its count exceeds 1 (a vertex in no valid triangle has count 0; a boundary fan has one class)
 *   bs_mesh_solid_records  records [T, 3] of 16 bytes like bs_mesh_records', with the vertex rows in the fourth lanes: (x, y, z, row) per
 *                          corner, and -1 in the first corner's lane of a triangle that is not kept, which is all bs_mesh_grid_count and
 *                          bs_mesh_grid_scatter read of it.  kept int32 [1] = the kept triangles
 *   bs_mesh_pairs_grid     the pairs (query triangle i of q_records, triangle j of records) of kept triangles that intersect as closed sets.
 *                          self != 0: one mesh (q_records == records), pairs i < j without a common vertex row; else every pair of the two
 *                          meshes.  Candidates: the closed fp32 boxes overlap.  The predicate is a function of the signs of orient3d -- each
 *                          computed once, in the order of the four vertex ids (mesh, row): fp64 differences u, v, w to the lowest id, det =
 *                          (ux (vy wz - vz wy) + uy (vz wx - vx wz)) + uz (vx wy - vy wx) without contraction, sign times the parity of the
 *                          sort -- as in Guigue & Devillers' test, and of orient2d (likewise) when all three vertices of one triangle have
 *                          sign 0 against the other's plane: the plane drops the axis of the largest component of triangle i's fp64 normal.
 *                          One thread per query triangle walks the cells of its own cell box in the triangle grid of `records` (refs [n_refs],
 *                          cell_start [cells + 1]: bs_mesh_grid_count / _scatter) and tests a pair only in the cell whose index per axis is
 *                          the larger of the two boxes' first cells: each pair is met once.  A query triangle whose box has more than
 *                          cell_cap cells goes onto fallback_list int32 [>= n_q] (fallback_count int32 [1]) for bs_mesh_pairs_brute.
 *                          mode BS_MESH_PAIRS_COUNT: out int32 [n_q] = the pairs of each query triangle (0 for one on the list);
 *                          BS_MESH_PAIRS_FILL: row_start int64 [n_q + 1] is the caller's exclusive scan of the counts, total = row_start[n_q]
 *                          in [1, 2^31); the keys i << 32 | j go to keys [row_start[i], row_start[i + 1]), nothing beyond the segment; the
 *                          caller sorts the rows (bs_pc_radius_sort).  BS_MESH_PAIRS_ANY: any int32 [1] (zeroed by the caller) is set when a
 *                          pair exists; threads leave once it is set
 *   bs_mesh_pairs_brute    the query triangles of list int32 [m] (NULL: all, m = n_q) against every triangle through LDS tiles, each pair in
 *                          exactly one wave of one block, into the same sinks: COUNT adds to out (zeroed here when list is NULL), FILL takes
 *                          slots from cursor int32 [>= m] (zeroed here)
 *   bs_mesh_signed_volume  vol6 fp64 [T] = a . (b x c) = (ax (by cz - bz cy) + ay (bz cx - bx cz)) + az (bx cy - by cx) with a, b, c the fp64
 *                          differences of a kept triangle's vertices to v[tri[parent[t]][0]] (parent: bs_mesh_cc_compress' fixed point), 0
 *                          for any other triangle.  The caller sums a cluster with bs_mesh_segment_sum and multiplies by 1 / 6
 * Integer atomics only.  Not built: exact arithmetic beyond fp64, pairs that share a vertex, welding, hole filling, booleans. */
enum { BS_MESH_PAIRS_COUNT = 0, BS_MESH_PAIRS_ANY = 1, BS_MESH_PAIRS_FILL = 2 };
int bs_mesh_fan_hook(const int32_t* triangles, int64_t n_triangles, const int32_t* edge_of_half, const int32_t* edge_first_triangle, int64_t n_edges,
                     int32_t* parent, int32_t* changed, void* stream);
int bs_mesh_fan_compress(int32_t* parent, int64_t n_corners, void* stream);
int bs_mesh_fan_count(const int32_t* triangles, int64_t n_triangles, int64_t n_vertices, const int32_t* edge_of_half, const int32_t* parent,
                      int32_t* count, void* stream);
int bs_mesh_solid_records(const float* vertices, int64_t n_vertices, const int32_t* triangles, int64_t n_triangles, void* records, int32_t* kept,
                          void* stream);
int bs_mesh_pairs_grid(const void* q_records, int64_t n_q, const void* records, int64_t n_triangles, const int32_t* refs, int64_t n_refs,
                       const int32_t* cell_start, const float* lo, const float* hi, float cell_size, const int32_t* dims, float pad, int32_t self,
                       int64_t cell_cap, int32_t mode, int32_t* out, const int64_t* row_start, int64_t total, void* keys, int32_t* any,
                       int32_t* fallback_list, int32_t* fallback_count, void* stream);
int bs_mesh_pairs_brute(const void* q_records, int64_t n_q, const int32_t* list, int64_t m, const void* records, int64_t n_triangles, int32_t self,
                        int32_t mode, int32_t* out, const int64_t* row_start, int64_t total, void* keys, int32_t* cursor, int32_t* any, void* stream);
int bs_mesh_signed_volume(const float* vertices, int64_t n_vertices, const int32_t* triangles, int64_t n_triangles, const int32_t* parent,
                          double* vol6, void* stream);

/* ---- rigid ICP registration ------------------------------------------------------------------------------------------------------------
 * bs_icp_step + bs_icp_finish replace Open3D's pipelines.registration.registration_icp with TransformationEstimationPointToPlane or
 * TransformationEstimationPointToPoint (no scale) and ICPConvergenceCriteria, and, in BS_ICP_EVALUATE mode, evaluate_registration: what
 * everyone runs before comparing a reconstruction with a scan.  The reference does not call them; they are restated from Open3D's
 * published interface, parity with Open3D is UNPINNED.  The statement is tests/_icp_ref.py.  One iteration at T (source -> target):
 *   point           p = fl32(((a0 s0 + a1 s1) + a2 s2) + t) per row of T, in fp64, rounded once: bs_pc_transform's arithmetic
 *   correspondence  the exact nearest target point of p under the contract above (ties to the lower index), valid when the fp32 distance
 *                   d <= max_distance; a non-finite row has none.  count = the valid pairs, fitness = count / m,
 *                   inlier_rmse = sqrt(sum d^2 / count) with d widened to fp64 (0 without a pair)
 *   coordinates     every sum is over coordinates relative to c = ((double) lo + (double) hi) / 2, the midpoint of the grid's box
 *   point-to-plane  target normals n fp32 [n_target, 3] (device), indexed as the target was given; a pair whose normal is non-finite or
 *                   zero counts for fitness and rmse and is left out of the sums.  r = (p - q) . n, J = [(p - c) x n, n], A = sum J J^T
 *                   (unweighted, 21 upper entries), b = sum J r; delta = -A^-1 b by Cholesky; T <- C exp(delta) C^-1 T with C the
 *                   translation by c and exp the SE(3) exponential of the left twist (omega, nu) as in bs_odo_p2p_step.  Fewer than 6
 *                   usable pairs or a non-positive pivot: BS_ICP_DEGENERATE, T unchanged.  No robust kernel
 *   point-to-point  sum (p - c), sum (q - c), sum (p - c)(q - c)^T; the Kabsch rotation from the 3 x 3 SVD of the centred covariance with
 *                   the sign fix on the smallest singular direction, t = mean q - R mean p, T <- [R | t] T.  Fewer than 3 pairs or a second
 *                   singular value that is not positive: BS_ICP_DEGENERATE.  No scale
 *   stopping        iteration k logs (fitness_k, rmse_k, count_k, usable_k) at the current T; for k >= 1, |fitness_k - fitness_(k-1)| <
 *                   relative_fitness and |rmse_k - rmse_(k-1)| < relative_rmse set BS_ICP_CONVERGED before any update; otherwise T is
 *                   updated, and after max_iteration updates the status is BS_ICP_MAX_ITERATION
 *   state           BS_ICP_STATE_FIELDS + BS_ICP_LOG_FIELDS * max_iteration doubles (device, 16-byte aligned), written by the caller before
 *                   the first call: 0 the status (0 = running), 1 the iterations logged so far (0), 2-13 the rows of [R | t] of T, the rest 0.
 *                   bs_icp_finish keeps 14-15 (the previous fitness and rmse), writes 16-19 in BS_ICP_EVALUATE mode (fitness, rmse,
 *                   count, usable count of the T in the state, which it leaves alone), 32-63 the last call's summed row, and from
 *                   BS_ICP_STATE_FIELDS on the log rows.  Once the status is set both entries return at their first instruction in
 *                   BS_ICP_ITERATE mode: iterations can be enqueued in chunks and the state read once per chunk
 *   bs_icp_step     one thread per source row (BS_F32 or BS_F64 [m, 3], device) over the index of bs_pc_grid_scatter and the target it was
 *                   built from: the shells of bs_pc_query_grid (the same device function) with no shell cap and no brute-force fallback
 *                   -- the radius is mandatory -- so the correspondence does not depend on the cell size.  partial: one row of
 *                   BS_ICP_PARTIAL_FIELDS doubles per block of 256 rows (device, ceil(m / 256) rows): 0 count, 1 usable count, 2 sum d^2,
 *                   then the 27 (plane: A, b) or 15 (point) sums; fp64, the xor butterfly in the wave, the waves in order
 *   bs_icp_finish   one block: adds the rows in an order fixed by m, logs, tests the stopping rule, solves and updates T, sets the status
 * No floating-point atomics: the same bits in every run, for every cell size. */
enum { BS_ICP_POINT_TO_POINT = 0, BS_ICP_POINT_TO_PLANE = 1 };
enum { BS_ICP_ITERATE = 0, BS_ICP_EVALUATE = 1 };
enum { BS_ICP_RUNNING = 0, BS_ICP_CONVERGED = 1, BS_ICP_MAX_ITERATION = 2, BS_ICP_DEGENERATE = 3 };
#define BS_ICP_PARTIAL_FIELDS 32
#define BS_ICP_STATE_FIELDS 64
#define BS_ICP_LOG_FIELDS 4
#define BS_ICP_MAX_ITERATIONS 65536
int bs_icp_step(const void* records, const int32_t* cell_start, int64_t n_records, const float* lo, const float* hi, float cell_size,
                const int32_t* dims, const float* target, const float* normals, int64_t n_target, const void* source, int32_t dtype, int64_t m,
                float max_distance, int32_t estimation, int32_t mode, const double* state, double* partial, void* stream);
int bs_icp_finish(const double* partial, int64_t m, const float* lo, const float* hi, int32_t estimation, int32_t mode, int32_t max_iteration,
                  double relative_fitness, double relative_rmse, double* state, void* stream);

/* ---- global registration: FPFH features, feature matching, RANSAC over correspondences --------------------------------------------------
 * The roles of Open3D's compute_fpfh_feature and registration_ransac_based_on_feature_matching / _on_correspondence: a pose between two
 * clouds that share no frame, the init of bs_icp_step.  The reference only calls Open3D.  Restated from Rusu, Blodow & Beetz 2009 (FPFH),
 * Fischler & Bolles 1981 (RANSAC), Kabsch / Arun et al. (the fit) and Open3D's documented meaning; parity with Open3D is UNPINNED.  The
 * statement is tests/_global_registration_ref.py.  Every pointer is a device pointer.
 *   lists             row_start int64 [m + 1], index int32 [total], d2 fp32 [total]: the SORTED rows of bs_pc_radius_* for the points
 *                     first .. first + m - 1 of a cloud of n points queried on itself; entries with d2 == 0 (the point itself, coincident
 *                     points) are left out
 *   bs_fpfh_spfh      table fp32 [n, 8] = (x, y, z, ., nx, ny, nz, .); for every pair (i, neighbour) in fp64 without contraction:
 *                     a1 = n1 . dp / d, a2 = n2 . dp / d; when |a1| < |a2| the roles swap (n1 <-> n2, dp -> -dp, f3 = -a2), else f3 = a1;
 *                     v = dp x n1 normalised (|v| = 0: the pair is skipped), w = n1 x v, f2 = v . n2, f1 = the angle of (n1 . n2, w . n2).
 *                     Eleven bins each: floor(11 (f + 1) / 2) clipped for f2 and f3; for f1 the sector of the vector among the ten edge
 *                     directions +-(2 j + 1) pi / 11, half-open, no transcendental function.  A zero or non-finite normal at either end
 *                     skips the pair.  spfh int32 [n, BS_FPFH_ROW]: 33 counts (f1, f2, f3), then k = the counted pairs, then zeros
 *   bs_fpfh_features  acc = sum_j (100 count_j / k_j) / (double) d2_ij: lane l of the row's wave adds entries l, l + 64, ... in order, then
 *                     the xor butterfly 32 .. 1; each block of eleven scaled to sum 100 when its sum is positive; + 100 count_i / k_i;
 *                     rounded to fp32 once.  k_i = 0 (no counted pair, a non-finite point): a zero row.  features fp32 [n, 33]
 *   bs_feature_match  source fp32 [m, 33], target fp32 [n, 33]; distance = sum_k (a_k - b_k)^2 in fp32, sequential, no contraction.
 *                     best uint64 [m], filled with ~0 by the caller: the minimum of (distance bits << 32 | target row) over the target
 *                     rows without a non-finite value, merged over `splits` target splits by a 64-bit atomicMin; a source row with a
 *                     non-finite value keeps ~0
 *   bs_gr_*           corr fp64 [c, 6] = (source xyz, target xyz), 16-byte aligned, c >= 3.
 *     _hypotheses     hypothesis h = h0 + i, i < count: three distinct rows from bs_loop_register's counter-based draw of (seed, pair 0,
 *                     h, draw); rejected unless every pair of the three has |ps| >= s |pt| and |pt| >= s |ps| (s =
 *                     edge_length_threshold, before any fit); Kabsch with its rank test; the three residuals^2 < tau^2.  fits fp64
 *                     [count, 12] (rows of [R | t]), valid int32 [count]
 *     _score          list int32 [n_valid]: the valid i ascending (the caller's compaction); score int32 [count], zeroed by the caller,
 *                     += #(residual^2 < tau^2) by integer atomics over `splits` splits of the correspondences
 *     _winner         best uint64 [1], zeroed before the first chunk: atomicMax of (score << 32 | ~h) over the scores > 0
 *     _winner_fit     state fp64 [BS_GR_STATE_FIELDS]: 0-11 the rows of [R | t] of hypothesis h, 12 status (1 / 0), 13 inliers, 14 RMSE,
 *                     15 rounds done
 *     _refit_step     mask int32 [c] = residual^2 < tau^2 at the state's transform; partial fp64 [ceil(c / 256), BS_GR_PARTIAL_FIELDS]:
 *                     count, Kabsch's 15 sums over the inliers, the sum of their squared residuals
 *     _refit_finish   one wave adds the partials in a fixed order; final_round = 0: Kabsch over the inliers replaces the transform (fewer
 *                     than 3 inliers or a collinear set: status 0); 1: writes the inlier count and the RMSE.  Status 0 makes both return
 *                     at once
 * No floating-point atomics: the same input gives the same bits in every call. */
#define BS_FPFH_DIM 33
#define BS_FPFH_ROW 36
#define BS_GR_STATE_FIELDS 16
#define BS_GR_PARTIAL_FIELDS 17
int bs_fpfh_spfh(const void* table, int64_t n, const int64_t* row_start, const int32_t* index, const float* d2, int64_t m, int64_t first,
                 int64_t total, int32_t* spfh, void* stream);
int bs_fpfh_features(const int32_t* spfh, int64_t n, const int64_t* row_start, const int32_t* index, const float* d2, int64_t m, int64_t first,
                     int64_t total, float* features, void* stream);
int bs_feature_match(const float* source, int64_t m, const float* target, int64_t n, int32_t splits, void* best, void* stream);
int bs_gr_hypotheses(const double* corr, int32_t c, uint64_t seed, uint32_t h0, int32_t count, double edge_length_threshold, double tau,
                     double* fits, int32_t* valid, void* stream);
int bs_gr_score(const double* corr, int32_t c, const double* fits, const int32_t* list, int32_t n_valid, int32_t count, int32_t splits, double tau,
                int32_t* score, void* stream);
int bs_gr_winner(const int32_t* score, int32_t count, uint32_t h0, void* best, void* stream);
int bs_gr_winner_fit(const double* corr, int32_t c, uint64_t seed, uint32_t h, double edge_length_threshold, double tau, double* state,
                     void* stream);
int bs_gr_refit_step(const double* corr, int32_t c, const double* state, double tau, int32_t* mask, double* partial, void* stream);
int bs_gr_refit_finish(const double* partial, int32_t c, int32_t final_round, double* state, void* stream);

/* ---- sparse-feature scale path: ORB match displacement (N3, rgbd_odo = False) ---------------------------------------------------------
 * The role of scaling_system.compute_scaling_factor (BodySLAM_not_refactored/3DM/scaling_system.py:107-137), which
 * VO.estimate_relative_pose_between calls with rgbd_odo = False (3DM/visual_odometry.py:70-79): cv2.ORB_create() on both frames,
 * BFMatcher(NORM_HAMMING, crossCheck = True), the matches sorted by distance, associate_depth twice, calculate_displacements, the mean.
 * OpenCV is not vendored: ORB (Rublee et al. 2011), FAST-9/16 (Rosten & Drummond 2006), the Harris measure and BRIEF's test pairs
 * (Calonder et al. 2010) are restated from their publications with cv2.ORB_create()'s default parameters in tests/_orb_ref.py, which also
 * lists every departure from OpenCV (test pairs, fixed-point resize, 30 orientation bins, tie rules); parity with OpenCV is UNPINNED.
 * What follows the match is the reference's own code and is restated with its quirks (pinned: tests/golden/sparse_scale.npz).
 * Every entry takes `batch` frames and runs each of its stages as ONE launch over them; a frame's result does not depend on the batch.
 *   levels      host int32 [n_levels, 3] = (W_l, H_l, offset_l): the levels of one frame lie in a flat byte buffer of `stride` bytes per
 *               frame; offsets and stride are multiples of 16 and a level is followed by at least its padding to 16 bytes
 *   bs_orb_pyramid        color u8 [batch, H, W, 3] (RGB; bgr != 0: BGR) -> grey = (4899 R + 9617 G + 1868 B + 8192) >> 14 at level 0,
 *                         level l from level l - 1 by a bilinear resize with 11-bit fixed-point weights (pixel centres aligned), and
 *                         smooth = [1 6 15 20 15 6 1]^2 / 4096 of every level, reflect-101, rounded once
 *   bs_orb_fast           score u8: the FAST-9/16 score (the largest threshold at which the pixel is still a corner, >= 20) where the
 *                         pixel beats its 8 neighbours strictly and lies 31 pixels inside the level, else 0; hist int32
 *                         [batch, BS_ORB_MAX_LEVELS, 256]: the histogram of the non-zero scores (zeroed by the call)
 *   bs_orb_select         per level the best 2 n_l by score, of those the best n_l by Harris response (7 x 7 block of 3 x 3 Sobel
 *                         products in int64, det - 0.04 tr^2 in fp64); every ranking key is (value descending, row-major pixel index
 *                         ascending).  keypoints int32 [batch, BS_ORB_MAX_FEATURES, 8] = (level, x, y, score, m10, m01, bin, 0), fields
 *                         0-3 written here; response fp64 [batch, BS_ORB_MAX_FEATURES]; counts int32 [batch, BS_ORB_MAX_LEVELS + 1] =
 *                         keypoints per level and their sum.  features_per_level: host int32 [n_levels], each <= 128, sum <= 500
 *   bs_orb_describe       fields 4-6: the moments over the radius-15 disc of the grey level and the first maximum of
 *                         m10 cos_sin[k] + m01 cos_sin[30 + k] over the 30 bins; pt fp32 [batch, BS_ORB_MAX_FEATURES, 2] =
 *                         (x level_scale[l], y level_scale[l]); desc u32 [batch, BS_ORB_MAX_FEATURES, 8]: bit i = smooth(p + a_i) <
 *                         smooth(p + b_i) with (a_i, b_i) = pattern[bin][i] (int8 [30, 256, 4] = x1, y1, x2, y2, device; |offset| <= 22)
 *                         level_scale: host doubles; cos_sin: 60 device doubles
 *   bs_orb_match          pair p = (query: frame p, train: frame p + 1), p < batch - 1: best train per query and best query per train
 *                         (the lowest index among equals), cross-check, stable sort by distance.  matches int32
 *                         [batch - 1, BS_ORB_MAX_FEATURES, 4] = (queryIdx, trainIdx, distance, 0); match_counts int32 [batch - 1]
 *   bs_orb_displacement   depth fp32 [batch, H, W]; K = (fx, fy, cx, cy) host doubles.  BS_ORB_ASSOC_REFERENCE: the reference's two
 *                         associate_depth calls (the second indexes the current frame's keypoints by queryIdx) and the zip of the two
 *                         independently filtered lists; BS_ORB_ASSOC_MATCHED: depth of the current frame at the matched keypoint,
 *                         pairs kept aligned.  out fp64 [batch - 1, BS_ORB_OUT_FIELDS]: 0-2 the mean of pixel_to_3d(current) -
 *                         pixel_to_3d(previous) summed in list order (NaN without a pair), 3 / 4 keypoints of the previous / current
 *                         frame, 5 matches, 6 / 7 associations of the previous / current side, 8 pairs used */
#define BS_ORB_MAX_FEATURES 500
#define BS_ORB_MAX_LEVELS 8
#define BS_ORB_OUT_FIELDS 9
enum { BS_ORB_ASSOC_REFERENCE = 0, BS_ORB_ASSOC_MATCHED = 1 };
int bs_orb_pyramid(const uint8_t* color, int32_t batch, int32_t H, int32_t W, int32_t bgr, const int32_t* levels, int32_t n_levels,
                   int64_t stride, uint8_t* grey, uint8_t* smooth, void* stream);
int bs_orb_fast(const uint8_t* grey, int32_t batch, int32_t H, int32_t W, const int32_t* levels, int32_t n_levels, int64_t stride,
                uint8_t* score, int32_t* hist, void* stream);
int bs_orb_select(const uint8_t* grey, const uint8_t* score, const int32_t* hist, int32_t batch, int32_t H, int32_t W, const int32_t* levels,
                  int32_t n_levels, int64_t stride, const int32_t* features_per_level, int32_t* keypoints, double* response, int32_t* counts,
                  void* stream);
int bs_orb_describe(const uint8_t* grey, const uint8_t* smooth, int32_t batch, int32_t H, int32_t W, const int32_t* levels, int32_t n_levels,
                    int64_t stride, const double* level_scale, const double* cos_sin, const int8_t* pattern, int32_t* keypoints,
                    const int32_t* counts, float* pt, uint32_t* desc, void* stream);
int bs_orb_match(const uint32_t* desc, const int32_t* counts, int32_t batch, int32_t* matches, int32_t* match_counts, void* stream);
int bs_orb_displacement(const float* pt, const int32_t* counts, const int32_t* matches, const int32_t* match_counts, const float* depth,
                        int32_t batch, int32_t H, int32_t W, const double* K, int32_t mode, double* out, void* stream);

/* ---- loop closure: one frame against many keyframes, RANSAC rigid registration of the matched 3-D points --------------------------------
 * The reference declares the step (3DM/slam.py:30,41,42: perform_loop_closure, num_closure, global_key_frame_indices) and calls an
 * undefined self._loop_closure() (:79-80); nothing here is its code.  RANSAC (Fischler & Bolles 1981) over three-point Kabsch fits
 * (Kabsch 1976; Arun et al. 1987), restated from the publications; the information matrix is the form of Open3D's
 * get_information_matrix_from_point_clouds, restated from its documentation: sum G^T G, G = [ -[q]x | I3 ] over the inlier points q of
 * the train frame, rotation parameters first.  Parity with Open3D is UNPINNED.  The statement is tests/_loop_closure_ref.py.
 *   bs_orb_lift           xyz fp64 [batch, BS_ORB_MAX_FEATURES, 4] = (x, y, z, valid 0.0 / 1.0) of every keypoint: depth fp32 [batch, H, W]
 *                         at (int(y), int(x)) as bs_orb_displacement reads it; valid = inside the image, depth != 0 and finite;
 *                         x = (u - cx) depth / fx, y = (v - cy) depth / fy, z = depth in fp64.  K = (fx, fy, cx, cy) host doubles.
 *                         Invalid rows and rows behind the frame's count are zero.
 *   bs_orb_match_pairs    bs_orb_match's match (the same device code) for P pairs = device int32 [P, 2] = (query frame, train frame),
 *                         indices into desc / counts of n_frames frames; a pair with an index outside [0, n_frames) gets 0 matches.
 *                         matches int32 [P, BS_ORB_MAX_FEATURES, 4], match_counts int32 [P].  bs_orb_match is pairs = (p, p + 1).
 *   bs_loop_register      per pair, one block: (1) the matches with distance <= max_hamming whose two points are valid, in match
 *                         order: C correspondences; C < max(3, min_matches) rejects.  (2) hypothesis h < n_hyp: three distinct
 *                         indices i0 = r0 % C, i1 = r1 % (C - 1), i2 = r2 % (C - 2), each shifted past the earlier picks, with
 *                         r_d = the high 32 bits of splitmix64's finaliser applied to
 *                         (seed ^ pair * 0xD6E8FEB86659FD93) + 0x9E3779B97F4A7C15 * (3 h + d + 1)   (64-bit wrap-around);
 *                         Kabsch in fp64; a sample whose summed 3 x 3 cross-covariance has a second singular value below 1e-12 m^2
 *                         scores 0; score = #(|R p + t - q| < tau).  (3) the highest score wins, the lowest h among equals; a best
 *                         score below 3 rejects.  (4) n_refit rounds of Kabsch over the inliers + recount, sums in a fixed order (no
 *                         atomics: the same bits in every run); fewer than 3 inliers or a collinear inlier set rejects.
 *                         records fp64 [P, BS_LOOP_FIELDS]: 0-15 T row-major (X_train = T X_query), 16 inliers, 17 C, 18 winning h,
 *                         19 RMSE over the inliers, 20 status (1 registered, 0 rejected), 21 matches, 22-57 the information matrix
 *                         row-major, 58-63 zero.  Rejected: T = identity, information zero, inliers 0, h = -1.
 *                         mask int32 [P, BS_ORB_MAX_FEATURES]: 1 at the match rows that are inliers. */
#define BS_LOOP_FIELDS 64
int bs_orb_lift(const float* pt, const int32_t* counts, const float* depth, int32_t batch, int32_t H, int32_t W, const double* K, double* xyz,
                void* stream);
int bs_orb_match_pairs(const uint32_t* desc, const int32_t* counts, int32_t n_frames, const int32_t* pairs, int32_t P, int32_t* matches,
                       int32_t* match_counts, void* stream);
int bs_loop_register(const double* xyz, int32_t n_frames, const int32_t* pairs, int32_t P, const int32_t* matches, const int32_t* match_counts,
                     int32_t max_hamming, double tau, int32_t n_hyp, int32_t n_refit, int32_t min_matches, uint64_t seed, double* records,
                     int32_t* mask, void* stream);

/* ---- pose graph: the numerical pieces of the line-process Levenberg-Marquardt (Choi, Zhou, Koltun, CVPR 2015) ---------------------------
 * The algorithm is the one bodyslam_amd/posegraph.py and oracle/posegraph_ref.py state (parity with Open3D UNPINNED); the LM control flow
 * stays on the host (PoseGraph(solver="device")), these four calls are what it evaluates.  Everything is fp64, device memory, row-major;
 * poses are 4 x 4 rigid transforms whose inverse is taken in closed form ([R^T | -R^T t]; the host path calls a general inverse).  No LDS,
 * no atomics, every sum in a fixed order: the same bits in every run.  The statement is tests/_posegraph_solve_ref.py.
 *   bs_pg_linearise   one lane per edge e = (src, tgt, T, info [6, 6], uncertain):  z = lin6(T^-1 X_tgt^-1 X_src),  q = z^T info z;
 *                     with BS_PG_LINE_PROCESS  lw = (mu / (mu + q))^2 for an uncertain edge and 1 otherwise is written, else lw is read;
 *                     cterm = lw q (+ mu (sqrt(lw) - 1)^2, uncertain);  with BS_PG_SYSTEM  Js[:, i] = lin6(T^-1 X_tgt^-1 G_i X_src),
 *                     Hss = Js^T (lw info) Js [E, 36] and g = Js^T (lw info) z [E, 6].  Without BS_PG_SYSTEM Hss and g are not touched
 *                     (the trial step's "cost only" mode).  cost (may be null): the sum of cterm, one wave: lane l adds l, l + 64, ..., then
 *                     the xor butterfly 32 .. 1.  An edge whose endpoints leave [0, N) reads nothing and writes zeros.
 *   bs_pg_assemble    one lane per node, a gather over its incident edges: row_ptr int32 [N + 1], adj int32 [nnz, 3] = (edge, the other
 *                     endpoint, -1 as the edge's source / +1 as its target) in ascending edge order, self-edges left out.
 *                     D [N, 36] = sum Hss, b [N, 6] = sum (source: -g, target: +g), Cc [N, 36]: Cc[i] = H[i][i + 1] = -sum Hss over the
 *                     edges between i and i + 1 (Cc[N - 1] = 0).  The reference node: D = I, b = 0, its couplings zero.
 *                     maxes (may be null) [2] = max b, max diag H.
 *   bs_pg_solve       (H + lambda I) delta = b by one level of substructuring over a plan made on the host (posegraph.solve_plan):
 *                     sep_node int32 [S] (ascending), node_slot int32 [N] (the separator's slot, -1 otherwise), segments int32 [n, 2] =
 *                     (first node, length) of every maximal run of non-separators, adjacent int32 [n_adjacent] = nodes i with i and i + 1
 *                     both separators, long_edges int32 [n_long, 3] = (edge, slot of its source, slot of its target) of the edges with
 *                     |src - tgt| >= 2 that do not touch the reference node.  stages: BS_PG_STAGE_SWEEP (one lane per segment: block
 *                     Cholesky over the interior in index order, the fill column to the left separator carried along; writes node_ws
 *                     [N, BS_PG_NODE_WORKSPACE] = L | L^-1 U | L^-1 F | L^-1 b~ and slots [n, BS_PG_SLOT_FIELDS] = the Schur contributions
 *                     (a, a) | (c, a) | (c, c) | r_a | r_c to the left (a) and right (c) separator), BS_PG_STAGE_REDUCED (one workgroup: M
 *                     [6 S, 6 S] and vec[0 : 6 S] = the separators' D + lambda I and b, the couplings of adjacent separators, the long edges
 *                     in edge order, the slots in segment order), BS_PG_STAGE_DENSE_SOLVE (the same workgroup: left-looking Cholesky in
 *                     place -- L(i, k) at M[k, i] --, two triangular solves, delta of the separators), BS_PG_STAGE_BACKSUB (one lane per
 *                     segment: the interiors' delta; sums (may be null) [2] = |delta|^2, delta . (lambda delta + b), one wave as above).
 *                     vec: 24 S doubles.  S <= BS_PG_MAX_SEPARATORS; a larger graph is the host path's.  information matrices are taken as
 *                     symmetric.  A pivot that is not positive gives NaN in delta and the sums.
 *   bs_pg_update      one lane per node: Xn = exp6(delta) X (exp6 = [Rz(d2) Ry(d1) Rx(d0) | d3:6], the bottom row copied), terms [N] =
 *                     |lin6(X)|^2 of the INPUT pose, xnorm2 (may be null) = their sum, one wave as above.  X and Xn are different arrays. */
#define BS_PG_MAX_SEPARATORS 128
#define BS_PG_MAX_NODES (1 << 24)
#define BS_PG_MAX_EDGES (1 << 24)
#define BS_PG_NODE_WORKSPACE 114
#define BS_PG_SLOT_FIELDS 120
enum { BS_PG_LINE_PROCESS = 1, BS_PG_SYSTEM = 2 };
enum { BS_PG_STAGE_SWEEP = 1, BS_PG_STAGE_REDUCED = 2, BS_PG_STAGE_DENSE_SOLVE = 4, BS_PG_STAGE_BACKSUB = 8, BS_PG_STAGE_ALL = 15 };
int bs_pg_linearise(const double* X, int32_t N, const double* T, const double* info, const int32_t* src, const int32_t* tgt,
                    const int32_t* uncertain, int32_t E, double mu, int32_t flags, double* lw, double* z, double* q, double* Hss, double* g,
                    double* cterm, double* cost, void* stream);
int bs_pg_assemble(const double* Hss, const double* g, int32_t E, int32_t N, const int32_t* row_ptr, const int32_t* adj, int32_t nnz,
                   int32_t reference_node, double* D, double* b, double* Cc, double* maxes, void* stream);
int bs_pg_solve(const double* D, const double* b, const double* Cc, const double* Hss, int32_t N, int32_t E, double lambda, const int32_t* segments,
                int32_t n_segments, const int32_t* sep_node, int32_t S, const int32_t* node_slot, const int32_t* adjacent, int32_t n_adjacent,
                const int32_t* long_edges, int32_t n_long, int32_t stages, double* node_ws, double* slots, double* M, double* vec, double* delta,
                double* sums, void* stream);
int bs_pg_update(const double* X, const double* delta, int32_t N, double* Xn, double* terms, double* xnorm2, void* stream);

/* ---- engine files: the forward of a whole model for a host without Python ------------------------------------
 * The reference's hosts are DepthEstimator.infer_depth_map (BodySLAM_Refactored/src/depth_estimation/interface.py:39-45) and
 * MPEMInterface.infer_relative_pose_between (BodySLAM_not_refactored/MPEM/mpem_interface.py:61-99), both Python.  A plan -- the launch
 * sequence of one (model, batch, frame size, precision, dtype) over static device buffers -- is compiled once by the Python builder and
 * written to an engine file (python -m bodyslam_amd.engine_export); any host then runs it with the calls below.  bs_engine_load
 * allocates every buffer and uploads the constants (weights in their packed device form); nothing is allocated per call.
 *   bs_engine_io          the device address / size of a named static input or output ("frames", "depth_m", "depth_u16"; "pairs", "T")
 *   bs_engine_run         issues the launches on `stream` (and the engine's own side stream, forked from and joined to it)
 *   bs_engine_upload / _download   host <-> named buffer, synchronous: for hosts that do not link the HIP runtime themselves
 *   bs_zoedepth_forward   frames u8 [B,H,W,3] (device) -> depth metres fp32 [B,H,W] and / or uint16 metres*256 [B,H,W] (either may be
 *                         NULL); flip augmentation, routing, post-processing as the engine was exported
 *   bs_cyclepose_forward  frames u8 [n_frames,H,W,3], pairs int32 [P,2] (indices into frames) -> T fp32 [P,16] (row-major 4x4)
 * Shapes must be the ones the engine was exported for (checked). */
typedef struct bs_engine bs_engine;
int bs_engine_load(const char* path, bs_engine** out);
int bs_engine_destroy(bs_engine* e);
int bs_engine_io(const bs_engine* e, const char* name, void** dev_ptr, int64_t* nbytes);
int64_t bs_engine_device_bytes(const bs_engine* e);
int bs_engine_run(bs_engine* e, void* stream);
int bs_engine_upload(bs_engine* e, const char* name, const void* host, int64_t nbytes);
int bs_engine_download(bs_engine* e, const char* name, void* host, int64_t nbytes);
int bs_zoedepth_forward(bs_engine* e, const uint8_t* frames_dev, int32_t B, int32_t H, int32_t W, float* depth_m_dev, uint16_t* depth_u16_dev,
                        void* stream);
int bs_cyclepose_forward(bs_engine* e, const uint8_t* frames_dev, int32_t n_frames, int32_t H, int32_t W, const int32_t* pairs_dev, int32_t P,
                         float* T_rel_dev, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* BODYSLAM_HIP_H */
