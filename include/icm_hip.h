/* icm_hip.h -- C ABI of libicm_hip.so: the MI355X (gfx950) hot path of the `cnn` (WACNN) codec.
 *
 * Drop-in boundary.  The reference has no FFI on this path: every op below
 * replaces a call the reference makes into ATen from Python.  Each entry point cites the
 * reference call site it stands in for (paths relative to the reference tree).
 *
 * Conventions
 *   - all tensors are device pointers to IEEE f32, NCHW, contiguous planes (H*W); the batch
 *     stride of every tensor is explicit (in floats) so channel-slices of a larger buffer
 *     (torch.cat / chunk in compressai/models/cnn.py:157-183) are addressed without copies;
 *   - `stream` is a hipStream_t; kernels are enqueued on it; nothing allocates, frees or
 *     synchronises (graph-capture safe); scratch memory is always a caller-owned workspace;
 *   - every reduction (bias / LayerNorm / table gradients, loss sums, gradient norm, split-K
 *     weight gradients) adds its partial sums in a FIXED order -- no float atomics -- so equal inputs
 *     give bit-identical outputs on every rank of a data-parallel job;
 *   - return value: 0 = ok, ICM_ERR_* otherwise (icm_strerror()).
 */
#ifndef ICM_HIP_H
#define ICM_HIP_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ICM_OK 0
#define ICM_ERR_ARG 1      /* bad argument (mirrors the reference's ValueError / assert sites) */
#define ICM_ERR_LAUNCH 2   /* hipLaunch failed */
#define ICM_ERR_UNSUPPORTED 3

/* activation applied to an operand while it is staged into LDS ("virtual" activations: the
 * framework stores pre-activations only; nn.GELU at layers/layers.py:59-63, cnn.py:54-127) */
#define ICM_ACT_NONE 0
#define ICM_ACT_GELU 1     /* exact erf GELU */
#define ICM_ACT_SQUARE 2   /* x*x: GDN's conv2d(x**2, gamma) (layers/gdn.py:68) */

/* epilogues of the implicit-GEMM kernels */
#define ICM_EPI_NONE 0        /* y = acc + bias.  NONE / RES / RES_GELU with y2 != NULL (forward): y2 = gelu(y) as well --
                               * the activation materialised once for every consumer of this pre-activation */
#define ICM_EPI_RES 1         /* y = acc + bias + res              (out += identity, layers.py:69) */
#define ICM_EPI_RES_GELU 2    /* y = acc + bias + gelu(res)        (identity is a virtual GELU output) */
#define ICM_EPI_GDN 3         /* y2 = n = acc + bias; y = aux * rsqrt(n)   (gdn.py:68-75) */
#define ICM_EPI_IGDN 4        /* y2 = n;              y = aux * sqrt(n)    (gdn.py:70-71) */
#define ICM_EPI_MUL_DGELU 5   /* y = acc * gelu'(aux)              (backward through a virtual GELU) */
#define ICM_EPI_AXPY2 6       /* y = aux2 + 2*aux*acc              (GDN backward dx) */
#define ICM_EPI_LRP 7         /* y = aux + 0.5*tanh(acc + bias); y2 = tanh(...)  (cnn.py:175-178) */
#define ICM_EPI_RES_MUL_DGELU 8 /* y = (acc + res) * gelu'(aux)   (dgrad into a ResidualUnit input: conv path + identity path) */

const char* icm_strerror(int code);
int icm_version(void);

/* ---- implicit-GEMM convolution family (f32 MFMA) ------------------------------------------
 * Replaces nn.Conv2d / nn.ConvTranspose2d / nn.Linear forward and backward:
 *   models/utils.py:114-132 (conv, deconv), layers/layers.py:29-43 (conv3x3, subpel_conv3x3, conv1x1),
 *   layers/gdn.py:68 (the CxC contraction), layers/win_attention.py:77-79,91,112 (qkv / proj Linear).
 *
 * transposed = 0  "gather":  y[n,o,p]        = sum_{i,t} Wg[o][i][t] * act(x[n,i,p*stride - pad + t])
 * transposed = 1  "scatter": y[n,o,q]        = sum_{i,t,p : p*stride - pad + t == q} Ws[i][o][t] * act(x[n,i,p])
 * conv fwd = gather with W; conv dgrad = scatter with W; convT fwd = scatter with Wt;
 * convT dgrad = gather with Wt.  Weights are passed pre-packed (icm_pack_weights).
 */
typedef struct icm_conv_args {
  const float* x; int64_t x_bs; int N, Cin, H, W;
  const float* wp;
  const float* bias;
  float* y; int64_t y_bs; int Cout, OH, OW;
  int KH, KW, stride, pad;
  int transposed;
  int pro_act;
  int epi;
  const float* res; int64_t res_bs;
  const float* aux; int64_t aux_bs;
  const float* aux2; int64_t aux2_bs;
  float* y2; int64_t y2_bs;   /* second output (epi NONE / RES / RES_GELU: gelu(y); GDN: the norm; LRP: tanh); y2 == y with
                               * y2_bs == y_bs: store ONLY gelu(y), in y (inference: nobody reads the pre-activation) */
  int accum;          /* y += result instead of y = result (gradient accumulation; with y2: y2 = gelu(y after the add)) */
  int pixel_shuffle;  /* 2: fuse nn.PixelShuffle(2) into the store (layers.py:34-38); y plane is (2*OH,2*OW), Cout/4 channels */
  /* blocked input-channel map (0 = none): logical channel c reads plane c + (c / x_seg_len) * x_seg_gap of x -- the
   * K-concatenation of equally long channel runs that lie x_seg_len + x_seg_gap planes apart (the first-layer input
   * gradients of all slice chains of one family, cnn.py:89-127, contracted in ONE launch) */
  int x_seg_len, x_seg_gap;
  /* ICM_ALGO_DIRECT (0): implicit GEMM over the spatial taps.  ICM_ALGO_WINOGRAD (1): F(2x2, 3x3) -- 3x3 stride-1 pad-1
   * launches only (icm_conv_winograd_ok), forward or input gradient; wp must then hold the Winograd-domain weights
   * (icm_pack_job.wino: 1 for the forward orientation, 2 for the input-gradient orientation).  Same f32 arithmetic
   * type, 4/9 of the multiply-adds; results agree with the direct form to summation-order noise. */
  int algo;
  /* ICM_ALGO_WINOGRAD only, optional: the input pre-transformed by icm_wino_transform (icm_wino_transform_floats
   * floats, caller-owned).  When set, icm_conv_run reads xv instead of x (operand activation and channel map were
   * applied by the transform): one transform per input tensor serves every launch and co-block that reads it, and
   * the convolution kernel stages its operand by 16-byte LDS-DMA with no vector work next to the matrix pipe. */
  float* xv;
} icm_conv_args;
#define ICM_ALGO_DIRECT 0
#define ICM_ALGO_WINOGRAD 1
/* 1 if icm_conv_run accepts these arguments with algo = ICM_ALGO_WINOGRAD (geometry and epilogue kind supported) */
int icm_conv_winograd_ok(const icm_conv_args* a);
/* size of the pre-transformed operand of these arguments (-1 if unsupported), and the transform itself: fills
 * arr[i].xv from arr[i].x for up to 12 same-geometry members in one launch */
int64_t icm_wino_transform_floats(const icm_conv_args* a);
int icm_wino_transform(const icm_conv_args* arr, int ngroups, void* stream);

int icm_conv_run(const icm_conv_args* a, void* stream);
/* up to 3 problems of identical geometry in one launch (cc_mean || cc_scale chains, cnn.py:164-168) */
int icm_conv_run_grouped(const icm_conv_args* a, int ngroups, void* stream);
/* named views of icm_conv_run, one per reference op */
int icm_conv2d_fwd(const icm_conv_args* a, void* stream);     /* F.conv2d forward            */
int icm_conv2d_dgrad(const icm_conv_args* a, void* stream);   /* its input gradient          */
int icm_convT2d_fwd(const icm_conv_args* a, void* stream);    /* F.conv_transpose2d forward  */
int icm_convT2d_dgrad(const icm_conv_args* a, void* stream);  /* its input gradient          */

/* number of floats of a packed weight buffer for GEMM-M `Cout`, GEMM-K channels `Cin` */
int64_t icm_packed_weight_floats(int Cout, int Cin, int KH, int KW);
/* w: canonical weights. src_out_major=1: w is [Cout][Cin][KH][KW] (Conv2d.weight seen by conv fwd,
 * ConvTranspose2d.weight seen by convT dgrad); 0: w is [Cin][Cout][KH][KW].  transposed/stride/pad
 * select the tap order the consuming icm_conv_run call expects.  nonneg=1 applies
 * NonNegativeParametrizer (ops/parametrizers.py:46-49): max(w,bound)^2 - pedestal while packing. */
int icm_pack_weights(const float* w, float* wp, int Cout, int Cin, int KH, int KW, int src_out_major,
                     int transposed, int stride, int pad, int nonneg, float bound, float pedestal,
                     void* stream);

/* many packing jobs in few launches (the trainer re-packs every weight once per step, forward and dgrad forms) */
typedef struct icm_pack_job {
  const float* w; float* wp;
  int Cout, Cin, KH, KW, src_out_major, transposed, stride, pad, nonneg;
  float bound, pedestal;
  /* sub-matrix of a wider canonical weight: the source rows hold src_ld (0 = natural) entries of the INNER matrix index
   * (Cin when src_out_major, else Cout) and the job takes the entries [src_off, src_off + count) -- the input-channel
   * blocks of the slice chains' first layers (cnn.py:89-127: latent | support slices | own slice) */
  int src_ld, src_off;
  /* concatenation along GEMM-M: the destination holds dst_ncot (0 = natural) 32-row tiles per (chunk, tap) step and
   * this job's tiles start at dst_cot_off.  (Concatenation along GEMM-K needs no field: consecutive jobs write
   * consecutive chunk ranges, i.e. wp advanced by icm_packed_weight_floats of the preceding jobs.) */
  int dst_ncot, dst_cot_off;
  /* 0: spatial taps (in the order transposed / stride / pad select).  1 / 2: Winograd F(2x2,3x3) weights G g G^T of a
   * 3x3 stride-1 pad-1 kernel, 16 transform points per (Cout, Cin) pair: 1 = forward orientation, 2 = input-gradient
   * orientation (kernel rotated by 180 degrees; pass the transposed matrix roles as for the direct dgrad pack).
   * Buffer size: icm_packed_weight_floats(Cout, Cin, 4, 4). */
  int wino;
} icm_pack_job;
int icm_pack_weights_batch(const icm_pack_job* jobs, int n, void* stream);

/* weight gradient: dW[a][b][t] = sum_{n,p} actS(gs[n,a,p]) * actB(gb[n,b,p*stride - pad + t])
 * conv:  gs = dY (a = Cout), gb = x  (b = Cin) -> Conv2d.weight.grad
 * convT: gs = x  (a = Cin),  gb = dY (b = Cout) -> ConvTranspose2d.weight.grad
 * ws: workspace of icm_wgrad_workspace_floats(...) floats. accum: dw += result. */
typedef struct icm_wgrad_args {
  const float* gs; int64_t gs_bs; int Ca, OH, OW; int act_s;
  const float* gb; int64_t gb_bs; int Cb, H, W; int act_b;
  int N, KH, KW, stride, pad;
  float* dw; float* ws; int accum;
  float* dbias; int accum_bias;   /* optional: dbias[a] (+)= sum_{n,p} actS(gs[n,a,p]) (conv bias gradient, fused) */
  int64_t ws_floats;              /* capacity of ws in floats; 0 = unchecked. Too small -> ICM_ERR_ARG, nothing launched */
  int dw_ld;                      /* 0 = Cb; else the gradient lands in a [Ca][dw_ld][KH][KW] tensor whose b-columns
                                   * start at dw (an input-channel block of a wider weight); may differ per group member */
  int algo;                       /* ICM_ALGO_DIRECT, or ICM_ALGO_WINOGRAD for 3x3 stride-1 pad-1 problems (fewer than
                                   * 65 536 2x2 tiles): dU = (A dY A^T)(.)(B^T d B) summed over tiles, dW = G^T dU G;
                                   * the workspace size depends on it (icm_wgrad_workspace_floats*) */
} icm_wgrad_args;
int64_t icm_wgrad_workspace_floats(const icm_wgrad_args* a);
/* workspace PER PROBLEM when n problems of this geometry are issued by one icm_conv_wgrad_grouped call (the pixel
 * split count, hence the slab size, depends on how many problems share the launch) */
int64_t icm_wgrad_workspace_floats_grouped(const icm_wgrad_args* a, int n);
int icm_conv_wgrad(const icm_wgrad_args* a, void* stream);
/* up to 32 weight-gradient problems of identical geometry in one launch pair (deferred, batched wgrads: a
 * weight gradient has no consumer but the optimiser, so the 150 small slice-chain wgrads are collected during
 * backward and issued together); every arr[i].ws is that problem's own workspace */
int icm_conv_wgrad_grouped(const icm_wgrad_args* arr, int n, void* stream);

/* out[c] (+)= sum_{n,p} x[n,c,p]   (bias gradients; GDN d_beta).  ws (optional, ws_floats >= 32*C for full
 * parallelism): partial sums of the pixel splits, added in split order; ws = NULL -> one workgroup per channel */
int icm_channel_sum(const float* x, int64_t x_bs, int N, int C, int HW, float* out, int accum, float* ws,
                    int64_t ws_floats, void* stream);

/* ---- GDN helpers (layers/gdn.py:62-75, ops/parametrizers.py:46-49, ops/bound_ops.py:25-27) ---- */
int icm_nonneg_fwd(const float* p, float* out, int64_t n, float bound, float pedestal, void* stream);
/* dp (+)= lb_bwd(2*max(p,bound)*g_eff) */
int icm_nonneg_bwd(const float* p, const float* g_eff, float* dp, int64_t n, float bound, int accum, void* stream);
/* dn = g*x*(-/+ 1/2)*n^(-/+1/2 - 1), t1 = g*n^(-/+ 1/2) */
int icm_gdn_bwd_pre(const float* g, const float* x, const float* nrm, float* dn, float* t1, int64_t n, int inverse, void* stream);

/* ---- elementwise pieces of Win_noShift_Attention (layers/layers.py:83-89) and cnn.py:150-152 ---- */
int icm_gelu_fwd(const float* x, float* y, int64_t n, void* stream);
/* out = gelu(a) * sigmoid(b) + x  (a is the virtual-GELU pre-activation of conv_a) */
int icm_gate_fwd(const float* a_pre, const float* b, const float* x, float* out, int64_t n, void* stream);
/* da_pre (+)= g*sig(b)*gelu'(a_pre); db = g*gelu(a_pre)*sig(b)*(1-sig(b)); dx (+)= g */
int icm_gate_bwd(const float* g, const float* a_pre, const float* b, float* da_pre, float* db, float* dx,
                 int64_t n, int accum_da, int accum_dx, void* stream);
/* dst (+)= src * (mul_dgelu_of ? gelu'(mul_dgelu_of) : 1) */
int icm_add_grad(const float* src, const float* mul_dgelu_of, float* dst, int64_t n, int accum, void* stream);
/* z_hat[n,c,p] = rint(z - med[c]) - (z-med[c]) + (z-med[c]) + med[c]   (ops/ops.py:34, cnn.py:150-152) */
int icm_ste_round_offset(const float* z, const float* quantiles, float* z_hat, int N, int C, int HW, void* stream);
/* LRP tail backward (cnn.py:177-178): dpre = g * 0.5 * (1 - t*t), t = tanh saved by ICM_EPI_LRP */
int icm_lrp_bwd(const float* g, int64_t g_bs, const float* t, int64_t t_bs, float* dpre, int64_t d_bs, int N, int C,
                int HW, void* stream);
/* inverse of nn.PixelShuffle(2) (layers.py:34-38) for the subpel conv backward: src [N][C][2H][2W] -> dst [N][4C][H][W] */
int icm_pixel_unshuffle2(const float* src, float* dst, int N, int C, int H, int W, void* stream);
/* dst[i*len + e] = srcs[i][e], i < n <= 64 (srcs: HOST array of device pointers): small parameter vectors laid end
 * to end -- the first-layer biases of the slice chains whose first layers run as one concatenated GEMM */
int icm_gather_vectors(const float* const* srcs, int n, int len, float* dst, void* stream);
/* strided 4-D copy (chunk/cat plumbing): dst[n,c,p] (+)= src[n,c,p] */
int icm_copy_strided(const float* src, int64_t src_bs, float* dst, int64_t dst_bs, int N, int C, int HW, int accum, void* stream);
/* dst[b][a][k] (+)= src[a][b][K-1-k]  (src [A][B][K], dst [B][A][K]): a Conv2d weight [Cout][Cin][KH*KW] (reference:
 * torch.nn.Conv2d in stf.py:401-404 `end_conv`) rewritten as the ConvTranspose2d weight of the same stride-1 map, and
 * that weight's gradient carried back; used by the thin-output path (very few output channels) of the host layer. */
int icm_permute_flip(const float* src, float* dst, int A, int B, int K, int accum, void* stream);

/* ---- zigzag block ordering of the stf6 / oj_ICM variants (compressai/models/stf6.py:654-762; fasterRCNN_ICM.py:103-293)
 * The latent x [B,C,H,W] (batch stride x_bs) is a grid of num_slices x num_h x num_w contiguous blocks; the zigzag
 * tensor z [B, N, C/num_slices, H/num_h, W/num_w] (contiguous, N = num_slices*num_h*num_w <= 64) lists them shell by
 * shell.  C, H, W must divide exactly (the reference's view() needs the same).  icm_zigzag_order fills `order` with
 * (c*num_h + h)*num_w + w per output block and returns N (order == NULL: just N; -1 on bad arguments / capacity).
 * Each function is its own inverse's adjoint: backward of splits = reverse on the gradient, and vice versa. */
int icm_zigzag_order(int num_slices, int num_h, int num_w, int32_t* order, int capacity);
int icm_zigzag_splits(const float* x, int64_t x_bs, float* z, int B, int C, int H, int W, int num_slices, int num_h,
                      int num_w, void* stream);
int icm_zigzag_reverse(const float* z, float* x, int64_t x_bs, int B, int C, int H, int W, int num_slices, int num_h,
                       int num_w, void* stream);

/* ---- stf (Swin) pieces on NCHW tensors ------------------------------------------------------------------
 * nn.LayerNorm(C) over the channel axis per pixel (compressai/models/stf.py:136,142,209,250,372): y = (x-mean)*rstd*gamma+beta;
 * mean/rstd [N*HW] are saved for backward (may be NULL in inference) */
int icm_layernorm_fwd(const float* x, int64_t x_bs, const float* gamma, const float* beta, float* y, int64_t y_bs,
                      float* mean, float* rstd, int N, int C, int HW, float eps, void* stream);
/* dx_extra (optional, [N,C,HW] with its own batch stride): added to dx -- the identity-path gradient of the residual
 * add around the norm (x + f(LN(x)), stf.py:190-191) without a separate elementwise pass */
int icm_layernorm_bwd(const float* x, int64_t x_bs, const float* dy, int64_t dy_bs, const float* gamma,
                      const float* mean, const float* rstd, float* dx, int64_t dx_bs, float* dgamma, float* dbeta,
                      int N, int C, int HW, int accum_dx, int accum_params, const float* dx_extra, int64_t dx_extra_bs,
                      float* ws, int64_t ws_floats /* optional split partials of dgamma / dbeta: 2*(2048 + C) floats */,
                      void* stream);
/* PatchMerging's 2x2 gather (stf.py:224-228): dst[n][k*C+c][y][x] = src[n][c][2y+(k&1)][2x+(k>>1)]; inverse=1 scatters
 * a [N,4C,H/2,W/2] gradient back into [N,C,H,W] */
int icm_space_to_depth2(const float* src, float* dst, int N, int C, int H, int W, int inverse, int accum, void* stream);
/* DropPath residual (stf.py:190-191): out[n] = shortcut[n] + scale[n]*branch[n] (shortcut may be NULL) */
int icm_residual_scale(const float* shortcut, const float* branch, const float* scale, float* out, int N,
                       int64_t per_sample, void* stream);

/* ---- thin-channel convolutions (the 3-channel ends g_a.0 / g_s.8, cnn.py:32,51) as 1x1 GEMM + column passes ----
 * im2col: cols[n][c*K*K + kh*K + kw][oy][ox] = x[n][c][oy*stride - pad + kh][ox*stride - pad + kw] (0 outside);
 *   x [N,C,H,W] -> cols [N, C*K*K, OH, OW], OH = (H + 2*pad - K)/stride + 1.  Forward of a Conv2d with few input
 *   channels (then a 1x1 GEMM over C*K*K channels), and the gradient of icm_col2im.
 * col2im (adjoint): out[n][c][y][x] (+)= bias[c] + sum over taps with (y+pad-kh) % stride == 0 of
 *   cols[n][c*K*K + t][(y+pad-kh)/stride][(x+pad-kw)/stride]; cols [N, C*K*K, OH, OW] -> out [N,C,H,W].  Tail of a
 *   ConvTranspose2d with few output channels (models/utils.py:124-132), and the gradient of icm_im2col. */
int icm_im2col(const float* x, float* cols, int N, int C, int H, int W, int K, int stride, int pad, void* stream);
int icm_col2im(const float* cols, const float* bias, float* out, int N, int C, int H, int W, int K, int stride, int pad,
               int accum, void* stream);

/* ---- window attention core (layers/win_attention.py:84-115,153-207) --------------------------
 * qkv: [N][3*C][H][W] (output of the qkv Linear run as a 1x1 conv on NCHW; channel = which*C + head*hd + d)
 * out: [N][C][H][W] (channel = head*hd + d), input of the proj Linear.  Cyclic shift, window partition,
 * relative-position bias gather, the 0/-100 shift mask and the softmax are folded into addressing.
 * table: relative_position_bias_table [(2ws-1)^2][heads]. */
int icm_winattn_fwd(const float* qkv, const float* table, float* out, int N, int C, int H, int W,
                    int heads, int ws, int shift, void* stream);
/* dqkv = gradient wrt qkv (overwritten); dtable (+)= gradient wrt table (accum_table = 0 overwrites).  wsp: workspace
 * of icm_winattn_bwd_workspace_floats() floats holding one partial table per (window, head), reduced in window order */
int64_t icm_winattn_bwd_workspace_floats(int N, int C, int H, int W, int heads, int ws);
int icm_winattn_bwd(const float* qkv, const float* table, const float* dout, float* dqkv, float* dtable,
                    int accum_table, float* wsp, int64_t ws_floats, int N, int C, int H, int W, int heads, int ws,
                    int shift, void* stream);

/* ---- EntropyBottleneck (entropy_models.py:395-433,446-489) ---------------------------------
 * params: the 13 tensors concatenated per channel is NOT required; pointers are passed separately.
 * z [N][C][HW]; noise NULL -> eval (dequantize around medians) else z + noise.
 * lik out [N][C][HW]; zt (z tilde) optional out. */
typedef struct icm_eb_params {
  const float* matrix[5]; const float* bias[5]; const float* factor[4]; const float* quantiles;
} icm_eb_params;
typedef struct icm_eb_grads {
  float* matrix[5]; float* bias[5]; float* factor[4];
  float* dmedian; /* [C], eval mode only (z~ = round(z-med)+med passes gradient to med, not z); may be NULL */
} icm_eb_grads;
int icm_eb_likelihood_fwd(const float* z, const float* noise, const icm_eb_params* p, float* lik, float* zt,
                          int N, int C, int HW, float lik_bound, void* stream);
/* dz (+)= ..., param grads overwritten (one workgroup owns a channel: deterministic) */
int icm_eb_likelihood_bwd(const float* z, const float* noise, const icm_eb_params* p, const float* dlik,
                          float* dz, const icm_eb_grads* g, int N, int C, int HW, float lik_bound,
                          int accum_dz, void* stream);
/* aux loss = sum |F(quantiles) - target| and its gradient wrt quantiles (entropy_models.py:395-398) */
int icm_eb_aux_loss(const icm_eb_params* p, float* loss /*1 float, overwritten*/, float* dquantiles, int C,
                    float target, void* stream);

/* ---- GaussianConditional likelihood fused with ste_round (entropy_models.py:626-659, cnn.py:171-173)
 * y slice [N][C][HW] with batch stride y_bs; mu/scale [N][C][HW] with strides; noise may be NULL (eval).
 * lik -> [N][C][HW] (lik_bs); y_hat = ste_round(y-mu)+mu -> (yh_bs), optional second copy yh2. */
int icm_gc_likelihood_ste_fwd(const float* y, int64_t y_bs, const float* mu, int64_t mu_bs, const float* scale,
                              int64_t sc_bs, const float* noise, int64_t nz_bs, float* lik, int64_t lik_bs,
                              float* yh, int64_t yh_bs, float* yh2, int64_t yh2_bs, int N, int C, int HW,
                              float scale_bound, float lik_bound, void* stream);
/* inputs: dlik, dyh (gradient wrt y_hat_pre; may be NULL). outputs: dy (+)=, dmu =, dscale = */
int icm_gc_likelihood_ste_bwd(const float* y, int64_t y_bs, const float* mu, int64_t mu_bs, const float* scale,
                              int64_t sc_bs, const float* noise, int64_t nz_bs, const float* dlik, int64_t dl_bs,
                              const float* dyh, int64_t dyh_bs, float* dy, int64_t dy_bs, float* dmu, int64_t dmu_bs,
                              float* dscale, int64_t dsc_bs, int N, int C, int HW, float scale_bound,
                              float lik_bound, int accum_dy, void* stream);

/* ---- entropy coding: CDF tables and the rANS stream -----------------------------------------
 * Replaces the calls entropy_models.py:60-63,172-290 makes into the reference's binary-only extensions
 * `compressai._CXX.pmf_to_quantized_cdf` and `compressai.ans.{RansEncoder,RansDecoder,BufferedRansEncoder}`
 * (CompressAI 1.1.6dev0 cpp_exts, sources absent from the tree; state machine = third_party/ryg_rans/rans64.h).
 * HOST functions: pointers are host memory, nothing touches the GPU.
 *
 * cdf[0..n]: quantised cumulative table of pmf[0..n-1] with cdf[n] = 2^precision and no zero-width symbol. */
int icm_pmf_to_quantized_cdf(const float* pmf, int n, int precision, int32_t* cdf);
/* cdfs: ncdf tables of cdf_stride int32 each (row i valid for cdf_sizes[i] entries, last bin = escape);
 * symbol i is coded with table indexes[i] after subtracting offsets[indexes[i]].  Returns the stream length in bytes
 * (a multiple of 4), -1 on bad arguments / capacity; out = NULL only measures. */
int64_t icm_rans_encode_with_indexes(const int32_t* symbols, const int32_t* indexes, int64_t n, const int32_t* cdfs,
                                     int cdf_stride, const int32_t* cdf_sizes, const int32_t* offsets, int ncdf,
                                     uint8_t* out, int64_t out_capacity);
int icm_rans_decode_with_indexes(const uint8_t* stream, int64_t nbytes, const int32_t* indexes, int64_t n,
                                 const int32_t* cdfs, int cdf_stride, const int32_t* cdf_sizes, const int32_t* offsets,
                                 int ncdf, int32_t* out);
/* RansDecoder.set_stream / decode_stream (cnn.py:300-318): one stream consumed by successive calls */
void* icm_rans_decoder_create(const uint8_t* stream, int64_t nbytes);
int icm_rans_decoder_decode(void* decoder, const int32_t* indexes, int64_t n, const int32_t* cdfs, int cdf_stride,
                            const int32_t* cdf_sizes, const int32_t* offsets, int ncdf, int32_t* out);
void icm_rans_decoder_destroy(void* decoder);

/* ---- lane streams: the second, opt-in stream format (`coder="lanes"`), made for the GPU -------------------------
 * Parity unpinned: no counterpart in the reference.  Layout and state machine: icm_amd/bitstream.py ("lane stream").
 * A stream codes nruns runs of (symbol, CDF index) pairs with the tables of the host coder above; G = clamp(ceil(max
 * run length / symbols_per_wave), 1, 4096) wave bodies of 64 interleaved 32-bit rANS states each, flushed once per
 * stream.  The host functions are the executable definition of the format; the *_gpu functions (csrc/rans_lanes.hip)
 * produce and consume the same bytes from device memory, one wave per body. */
#define ICM_LANES_ST_OVERRUN 1   /* a word was wanted past the end of a body */
#define ICM_LANES_ST_SYMBOL 2    /* no table bin holds the decoded cumulative value */
#define ICM_LANES_ST_ESCAPE 4    /* an escape decodes to a symbol outside int32 */
#define ICM_LANES_ST_INDEX 8     /* a CDF index outside [0, ncdf), or a table size outside [2, cdf_stride] */
#define ICM_LANES_ST_STATE 16    /* finish: a lane did not end at 2^16 */
#define ICM_LANES_ST_CURSOR 32   /* finish: words of a body were left unread */
/* G of a stream of these runs; -1 on bad arguments (negative length, symbols_per_wave < 1) */
int icm_rans_lanes_waves(const int64_t* run_lengths, int nruns, int64_t symbols_per_wave);
/* symbols / indexes: the runs back to back.  Returns the stream length in bytes, -1 on bad arguments / capacity;
 * out = NULL only measures. */
int64_t icm_rans_lanes_encode(const int32_t* symbols, const int32_t* indexes, const int64_t* run_lengths, int nruns,
                              const int32_t* cdfs, int cdf_stride, const int32_t* cdf_sizes, const int32_t* offsets,
                              int ncdf, int64_t symbols_per_wave, uint8_t* out, int64_t out_capacity);
/* create: NULL unless the header and the length table describe exactly nbytes.  decode_run: the next run, in stream
 * order; always writes n symbols (0 where a lane failed) and reads no byte outside the stream; ICM_ERR_ARG once any
 * status bit is set.  finish: the ICM_LANES_ST_* bits of the whole stream, 0 = every body ended at its last word
 * with every lane at 2^16. */
void* icm_rans_lanes_decoder_create(const uint8_t* stream, int64_t nbytes);
int icm_rans_lanes_decoder_decode_run(void* decoder, const int32_t* indexes, int64_t n, const int32_t* cdfs,
                                      int cdf_stride, const int32_t* cdf_sizes, const int32_t* offsets, int ncdf,
                                      int32_t* out);
int icm_rans_lanes_decoder_finish(void* decoder);
void icm_rans_lanes_decoder_destroy(void* decoder);
/* A range of waves (the bodies of a stream share nothing, so any of them can be decoded alone).
 * waves: G of the decoder's stream, -1 for NULL.
 * decode_run_waves: waves g0 <= g < g1 decode their elements of a run of length n -- n is the whole run's length, which
 *   fixes c = 64 ceil(ceil(n / G) / 64); wave g owns the elements [g c, min(n, (g + 1) c)).  Element e reads
 *   indexes[e - elem0] and writes out[e - elem0], so the two buffers hold the elements [elem0, min(n, g1 c)) and need
 *   not start at the run's first; a range that owns no element of the run (g0 = g1, or g0 c >= n) needs none and does
 *   nothing.  Requires 0 <= g0 <= g1 <= G and 0 <= elem0 <= g0 c, otherwise ICM_ERR_ARG before anything is done;
 *   ICM_ERR_ARG also once a status bit of one of these waves is set.  State, cursor and status of every other wave are
 *   untouched.  decode_run is decode_run_waves(0, G, 0).
 * finish_waves: the ICM_LANES_ST_* bits of the waves g0 <= g < g1 only; end = 1 adds the end checks (cursor at the
 *   body's last word, every lane at 2^16), end = 0 is for waves that stop before their last run.  -1 for NULL or a bad
 *   range.  It leaves the decoder as it is, usable and still to be destroyed.  finish is finish_waves(0, G, 1).
 * The caller's contract: a wave is given the runs of the stream in their order, none skipped -- a wave that is to
 * decode its part of run r must have decoded its parts of the runs 0 .. r - 1 (parts that own no element included: they
 * are no work).  Different waves may stand at different runs. */
int icm_rans_lanes_decoder_waves(void* decoder);
int icm_rans_lanes_decoder_decode_run_waves(void* decoder, int g0, int g1, int64_t elem0, const int32_t* indexes,
                                            int64_t n, const int32_t* cdfs, int cdf_stride, const int32_t* cdf_sizes,
                                            const int32_t* offsets, int ncdf, int32_t* out);
int icm_rans_lanes_decoder_finish_waves(void* decoder, int g0, int g1, int end);

/* Device side.  symbols / indexes / tables / ws are DEVICE memory, run_lengths is host memory.
 * encode: ws = icm_rans_lanes_encode_gpu_workspace(...) bytes, 16-byte aligned.  worst_case = 0 gives every wave one
 * word per symbol (enough for any input without escapes), 1 the four words per symbol no input exceeds.  Launches on
 * `stream`, waits for it, and returns the stream length: the string then lies at ws + *string_offset.  -1: bad
 * arguments, or an index / table the coder cannot use (the host coder's refusals); -2: worst_case = 0 was too small,
 * call again with 1; -3: a launch or copy failed. */
int64_t icm_rans_lanes_encode_gpu_workspace(const int64_t* run_lengths, int nruns, int64_t symbols_per_wave,
                                            int worst_case);
int64_t icm_rans_lanes_encode_gpu(const int32_t* symbols, const int32_t* indexes, const int64_t* run_lengths, int nruns,
                                  const int32_t* cdfs, int cdf_stride, const int32_t* cdf_sizes, const int32_t* offsets,
                                  int ncdf, int64_t symbols_per_wave, int worst_case, void* ws, int64_t ws_bytes,
                                  int64_t* string_offset, void* stream);
/* create: stream = HOST bytes; validates header and length table before anything touches the device, then uploads
 * the string with the per-wave state, cursor and status (one allocation, one copy).  decode_run: one launch on
 * `stream`, no host sync; indexes / out / tables are device memory.  finish: one small launch, one copy of G status
 * words and a wait on `stream`; returns the ICM_LANES_ST_* bits, or -1 if the runtime failed. */
void* icm_rans_lanes_decoder_gpu_create(const uint8_t* stream_bytes, int64_t nbytes, void* stream);
int icm_rans_lanes_decoder_gpu_decode_run(void* decoder, const int32_t* indexes, int64_t n, const int32_t* cdfs,
                                          int cdf_stride, const int32_t* cdf_sizes, const int32_t* offsets, int ncdf,
                                          int32_t* out, void* stream);
int icm_rans_lanes_decoder_gpu_finish(void* decoder, void* stream);
void icm_rans_lanes_decoder_gpu_destroy(void* decoder);
/* The ranged forms of the host decoder above, same arguments, contract and symbols bit for bit; indexes / out are
 * device memory that holds the elements [elem0, min(n, g1 c)).  decode_run_waves launches g1 - g0 waves (none for a
 * range that owns nothing) and, like decode_run, does not wait: the status is finish_waves' to report, which copies
 * back the status words of the range alone and waits on `stream`. */
int icm_rans_lanes_decoder_gpu_waves(void* decoder);
int icm_rans_lanes_decoder_gpu_decode_run_waves(void* decoder, int g0, int g1, int64_t elem0, const int32_t* indexes,
                                                int64_t n, const int32_t* cdfs, int cdf_stride,
                                                const int32_t* cdf_sizes, const int32_t* offsets, int ncdf,
                                                int32_t* out, void* stream);
int icm_rans_lanes_decoder_gpu_finish_waves(void* decoder, int g0, int g1, int end, void* stream);
/* CDF search of the decode kernel: 1 probes outward from the table's centre bin, 0 = plain binary search; the
 * default is the form DESIGN.md 5 measured faster */
void icm_debug_lanes_search(int centre);

/* device side of update() / compress() / decompress() (stream-ordered like every other kernel entry point) */
/* EntropyBottleneck.update (entropy_models.py:354-393): minima / maxima [C] int32, then pmf [C][max_length] and
 * tail_mass [C] on the integer grid median - minima + k */
int icm_eb_table_bounds(const float* quantiles, int C, int32_t* minima, int32_t* maxima, void* stream);
int icm_eb_pmf_table(const icm_eb_params* p, const int32_t* minima, int C, int max_length, float* pmf, float* tail_mass,
                     void* stream);
/* GaussianConditional.update (entropy_models.py:598-624): centers = ceil(scale_table * multiplier); pmf [ns][max_length] */
int icm_gc_table_centers(const float* scale_table, int ns, float multiplier, int32_t* centers, void* stream);
int icm_gc_pmf_table(const float* scale_table, const int32_t* centers, int ns, int max_length, float* pmf,
                     float* tail_mass, void* stream);
/* GaussianConditional.build_indexes (entropy_models.py:661-666) */
int icm_gc_build_indexes(const float* scale, int64_t scale_bs, const float* scale_table, int ns, float scale_bound,
                         int32_t* indexes, int N, int C, int HW, void* stream);
/* EntropyModel.quantize "symbols" / "dequantize" (entropy_models.py:126-150) and dequantize (:159-166); the mean of
 * element (n,c,p) is means[n*m_bs + c*m_cs + p*m_ps] (means NULL = 0): full tensors or per-channel medians */
int icm_quantize(const float* x, int64_t x_bs, const float* means, int64_t m_bs, int64_t m_cs, int64_t m_ps,
                 int32_t* symbols, float* dequantized, int N, int C, int HW, void* stream);
int icm_dequantize(const int32_t* symbols, const float* means, int64_t m_bs, int64_t m_cs, int64_t m_ps, float* out,
                   int64_t out_bs, int N, int C, int HW, void* stream);

/* ---- quantiser step on y: the codec's quality knob (csrc/qstep.hip).  Parity unpinned: no counterpart in the
 * reference.  `step` = 2^(k/8) and `inv` = 1 / step as f32, both from icm_amd/bitstream.py:step_of.  All f32, every
 * operation rounded once, no FMA:
 *   symbol = (int)clamp(rint((y - mu) * inv), -2^30, 2^30);  y_hat = ((float)symbol * step) + mu;
 *   index = (ns - 1) - #{ j < ns - 1 : max(scale, scale_bound) * inv <= scale_table[j] }
 * Operands are [N][C][HW] with an element batch stride per float operand (channel slices of wider buffers); symbols
 * and indexes are dense int32.  code_q is the encoder's one launch per slice; indexes_q and dequantize_q are the
 * decoder's steps before and after the entropy decoder's run, and compute index and y_hat through the device
 * functions code_q uses.  With step = inv = 1: icm_quantize's symbols, icm_gc_build_indexes' indexes and the y_hat of
 * icm_gc_likelihood_ste_fwd.  NaN inputs are outside the contract, as for icm_quantize.
 * ICM_ERR_ARG before any launch, outputs untouched: a null pointer, step or inv not finite or <= 0, ns < 1, N, C or
 * HW < 1. */
int icm_gc_code_q(const float* y, int64_t y_bs, const float* mu, int64_t mu_bs, const float* scale, int64_t sc_bs,
                  const float* scale_table, int ns, float scale_bound, float step, float inv, int32_t* symbols,
                  int32_t* indexes, float* yh, int64_t yh_bs, int N, int C, int HW, void* stream);
int icm_gc_indexes_q(const float* scale, int64_t sc_bs, const float* scale_table, int ns, float scale_bound, float inv,
                     int32_t* indexes, int N, int C, int HW, void* stream);
int icm_dequantize_q(const int32_t* symbols, const float* mu, int64_t mu_bs, float step, float* yh, int64_t yh_bs, int N,
                     int C, int HW, void* stream);
/* The same three with a quality map: a step per latent position, shared by every n and c.  `qmap`: HW step indexes k
 * (int8, dense); `step_table`: 256 (step, inv) pairs of f32, 8-byte aligned, indexed by the map byte read as uint8_t
 * (icm_amd/bitstream.py:step_table; bytes that are no valid k hold (1, 1)).  The element at position p of any (n, c)
 * is coded with the pair of qmap[p], through the device functions the scalar kernels use: a map whose every entry is
 * k gives the outputs of the scalar entry points at step_of(k).  The kernels neither clamp nor check the map; the
 * callers refuse an invalid one.  ICM_ERR_ARG before any launch, outputs untouched: a null pointer (qmap and
 * step_table included), ns < 1, N, C or HW < 1. */
int icm_gc_code_qmap(const float* y, int64_t y_bs, const float* mu, int64_t mu_bs, const float* scale, int64_t sc_bs,
                     const float* scale_table, int ns, float scale_bound, const int8_t* qmap, const float* step_table,
                     int32_t* symbols, int32_t* indexes, float* yh, int64_t yh_bs, int N, int C, int HW, void* stream);
int icm_gc_indexes_qmap(const float* scale, int64_t sc_bs, const float* scale_table, int ns, float scale_bound,
                        const int8_t* qmap, const float* step_table, int32_t* indexes, int N, int C, int HW,
                        void* stream);
int icm_dequantize_qmap(const int32_t* symbols, const float* mu, int64_t mu_bs, const int8_t* qmap,
                        const float* step_table, float* yh, int64_t yh_bs, int N, int C, int HW, void* stream);
/* Rate-distortion optimised quantisation: icm_gc_code_q / icm_gc_code_qmap with a choice, per element, between the
 * nearest symbol s0 and its neighbour toward zero s1 = s0 - sign(s0).  Encoder only: the symbols are ordinary symbols
 * and indexes_q / dequantize_q (or the map pair, or the plain pair at step = inv = 1) decode them.  `qmap` and
 * `step_table` are both NULL (the scalar pair `step`, `inv` for every position) or both set (the pair of each
 * position, as icm_gc_code_qmap; `step` and `inv` are then unused but still checked).  `cdfs` [ncdf][cdf_stride],
 * `cdf_sizes` [ncdf] and `offsets` [ncdf] are the coder's device tables (int32; `cdfs` fixes the layout of `bits` and
 * is not read); `bits` [ncdf][cdf_stride] f32 is the code-length table of icm_amd/bitstream.py:code_length_table,
 * bits[r][v] = 16 - log2(cdfs[r][v + 1] - cdfs[r][v]) for v < cdf_sizes[r] - 2; `w` weighs the squared error in symbol
 * units.  With u = (y - mu) * inv, off = offsets[index], ov = cdf_sizes[index] - 2, v_j = s_j - off, all f32, one
 * rounding per operation, no FMA:
 *   e_j = u - (float)s_j;  J_j = (w * (e_j * e_j)) + bits[index][v_j]
 * and s1 is coded iff s0 != 0, all of v0, v1 lie in 0 .. ov - 1 (an escaped symbol is kept, no candidate becomes one)
 * and J1 < J0 strictly; y_hat is that of the symbol coded, the index is unchanged.  One launch.
 * ICM_ERR_ARG before any launch, outputs untouched: a null pointer (qmap / step_table excepted as above, one of the two
 * without the other included), N, C or HW < 1, N > 65535 (an image is a workgroup row of the grid), ns != ncdf or < 1,
 * cdf_stride < 3, step, inv or w not finite or <= 0. */
int icm_gc_code_rdo(const float* y, int64_t y_bs, const float* mu, int64_t mu_bs, const float* scale, int64_t sc_bs,
                    const float* scale_table, int ns, float scale_bound, float step, float inv, const int8_t* qmap,
                    const float* step_table, const int32_t* cdfs, int cdf_stride, const int32_t* cdf_sizes,
                    const int32_t* offsets, int ncdf, const float* bits, float w, int32_t* symbols, int32_t* indexes,
                    float* yh, int64_t yh_bs, int N, int C, int HW, void* stream);

/* Training and estimation at a step (variable-rate training; parity unpinned like the rest of this section): the pair
 * icm_gc_likelihood_ste_fwd / _bwd with a (step, inv) pair per IMAGE, `steps` [N][2] f32 in DEVICE memory, 8-byte
 * aligned (a captured training graph is replayed with fresh steps; the kernels do not check the pairs).  Per element
 * of image n, f32, through the device functions of the codec kernels above:
 *   t = (y - mu) * inv;  s = symbol;  v = noise ? t + noise : (float)s;  se = max(scale, scale_bound) * inv;
 *   lik = max(Phi((1/2 - |v|) / se) - Phi((-1/2 - |v|) / se), lik_bound);  y_hat = ((float)s * step) + mu
 * so the likelihood is that of the symbol the codec codes under the scale it codes it with, and y_hat (-> yh, optional
 * second copy yh2; either may be NULL) is icm_gc_code_q's bit for bit, with or without noise.
 * bwd: inputs dlik, dyh (gradient wrt y_hat; may be NULL); dy (+)= (accum_dy), dmu =, dscale =.  The likelihood reaches
 * y and mu through t (factor inv; nothing without noise) and scale through se (factor inv); both LowerBound gates are
 * those of icm_gc_likelihood_ste_bwd; dyh passes to dy unchanged and not to dmu.
 * ICM_ERR_ARG before any launch, outputs untouched: what the scalar pair refuses, and a null `steps`. */
int icm_gc_likelihood_ste_qs_fwd(const float* y, int64_t y_bs, const float* mu, int64_t mu_bs, const float* scale,
                                 int64_t sc_bs, const float* noise, int64_t nz_bs, const float* steps, float* lik,
                                 int64_t lik_bs, float* yh, int64_t yh_bs, float* yh2, int64_t yh2_bs, int N, int C,
                                 int HW, float scale_bound, float lik_bound, void* stream);
int icm_gc_likelihood_ste_qs_bwd(const float* y, int64_t y_bs, const float* mu, int64_t mu_bs, const float* scale,
                                 int64_t sc_bs, const float* noise, int64_t nz_bs, const float* steps, const float* dlik,
                                 int64_t dl_bs, const float* dyh, int64_t dyh_bs, float* dy, int64_t dy_bs, float* dmu,
                                 int64_t dmu_bs, float* dscale, int64_t dsc_bs, int N, int C, int HW, float scale_bound,
                                 float lik_bound, int accum_dy, void* stream);

/* The same pair with a step per (image, latent position) (quality-map training): `steps` is replaced by
 *   qmap        [N][HW] int8, dense, DEVICE memory: a step index per image and position, shared by the channels;
 *   step_table  the 256 (step, inv) pairs of icm_gc_code_qmap, indexed by the map byte read as unsigned.
 * Per element the arithmetic is that of the _qs pair with the pair of the element's position: a map that is uniform
 * over an image gives that image the _qs pair's bits, and y_hat is icm_gc_code_qmap's bit for bit.  No kernel clamps
 * the map byte or branches on its validity: the caller checks maps.
 * ICM_ERR_ARG before any launch, outputs untouched: what the _qs pair refuses, a null `qmap`, a null `step_table`
 * (and N > 65535: an image is a workgroup row of the grid). */
int icm_gc_likelihood_ste_qm_fwd(const float* y, int64_t y_bs, const float* mu, int64_t mu_bs, const float* scale,
                                 int64_t sc_bs, const float* noise, int64_t nz_bs, const int8_t* qmap,
                                 const float* step_table, float* lik, int64_t lik_bs, float* yh, int64_t yh_bs,
                                 float* yh2, int64_t yh2_bs, int N, int C, int HW, float scale_bound, float lik_bound,
                                 void* stream);
int icm_gc_likelihood_ste_qm_bwd(const float* y, int64_t y_bs, const float* mu, int64_t mu_bs, const float* scale,
                                 int64_t sc_bs, const float* noise, int64_t nz_bs, const int8_t* qmap,
                                 const float* step_table, const float* dlik, int64_t dl_bs, const float* dyh,
                                 int64_t dyh_bs, float* dy, int64_t dy_bs, float* dmu, int64_t dmu_bs, float* dscale,
                                 int64_t dsc_bs, int N, int C, int HW, float scale_bound, float lik_bound, int accum_dy,
                                 void* stream);

/* Painting quality maps on the device (quality-map training), one launch: qmap [N][h][w] int8 (written); every cell of
 * image n holds base[n] ([N] int8), then the R rectangles rects[n][r] = (y0, x0, y1, x1, k) ([N][R][5] int32; cells,
 * half open) of image n are painted in order, later ones winning.  All three in DEVICE memory.  R = 0 paints the
 * base alone (rects is still non-null); an empty rectangle paints nothing; a rectangle is clipped to the map; k and
 * the coordinates are not range-checked otherwise.
 * ICM_ERR_ARG before the launch: a null pointer, N, h or w < 1, R < 0 (and h * w > 2^30 or N > 65535). */
int icm_qmap_paint(const int8_t* base, const int32_t* rects, int R, int8_t* qmap, int N, int h, int w, void* stream);

/* The quality maps of variance-adaptive quantisation for a training batch, two launches: what `codec encode --aq S`
 * derives from an image (icm_amd/codec.py: cell_stats, aq_activity, aq_reference, aq_offsets, quality_map), for planar
 * f32 crops x [N][3][H][W] of whole 16 x 16 cells (H, W multiples of 16; x 16-byte aligned), h = H / 16, w = W / 16:
 *   8-bit value of a sample: (int)(min(max(v, 0), 1) * 255.0f), the rule of icm_image_f32_to_u8 (NaN unspecified)
 *   Y = (77 R + 150 G + 29 B + 128) >> 8;  per cell s1 = sum Y, s2 = sum Y^2 over its 256 pixels (integers)
 *   L = log2(1 + (256 s2 - s1^2) / 65536) in double, the numerator a 64-bit integer
 *   ref[n] = mean of L over the h w cells of image n, summed in double in an order fixed by the cell index
 *   d = clip(rint(4 (double)strength[n] (L - ref[n])), -16, 16), ties to even;  cell = clamp(base[n] + d, -16, 32)
 *   then the R rectangles rects[n][r] of image n over it, exactly as icm_qmap_paint paints them (k as given).
 * base [N] int8, strength [N] f32, rects [N][R][5] int32 (may be null with R = 0), qmap [N][h][w] int8 and ref [N]
 * double (8-byte aligned) are DEVICE memory; every entry of qmap and ref is written exactly once, the same bits on
 * every run and whatever else is in the batch.  ws: icm_qmap_aq_workspace_bytes(N, H, W) bytes, 8-byte aligned, need
 * not be cleared.  No allocation, synchronisation or host read: the launches can be captured in a graph.
 * ICM_ERR_ARG before any launch: a null pointer (rects only with R > 0), N, H or W < 1, H or W no multiple of 16,
 * R < 0, a workspace too small, a misaligned x, ref or ws, and icm_qmap_paint's limits (h w > 2^30, N > 65535). */
int64_t icm_qmap_aq_workspace_bytes(int N, int H, int W);   /* 0 = bad geometry */
int icm_qmap_aq(const float* x, int N, int H, int W, const int8_t* base, const float* strength, const int32_t* rects,
                int R, int8_t* qmap, double* ref, void* ws, int64_t ws_bytes, void* stream);

/* ---- R-D loss (train.py:53-61, train_czigzag.py:63,71) --------------------------------------
 * out[0]=bpp, out[1]=mse, out[2]=loss, out[3]=sum log(lik_y), out[4]=sum log(lik_z) (5 floats, overwritten);
 * ws: ICM_REDUCE_WS_FLOATS floats of scratch (per-workgroup partial sums, added in workgroup order). */
#define ICM_REDUCE_WS_FLOATS 8192
int icm_rd_loss_fwd(const float* x, const float* x_hat, int64_t n_img_elems, const float* lik_y, int64_t n_y,
                    const float* lik_z, int64_t n_z, int64_t num_pixels, float lmbda, float* out, float* ws,
                    void* stream);
/* dx_hat = gscale * lmbda*255^2*2*(x_hat-x)/n ; dlik = gscale * -1/(lik*ln2*num_pixels) */
int icm_rd_loss_bwd(const float* x, const float* x_hat, int64_t n_img_elems, const float* lik_y, int64_t n_y,
                    const float* lik_z, int64_t n_z, int64_t num_pixels, float lmbda, float gscale,
                    float* dx_hat, float* dlik_y, float* dlik_z, void* stream);
/* The same with a distortion weight per image (variable-rate training): x / x_hat hold N images of img_elems floats,
 * lmbda_n [N] f32 in DEVICE memory.  out[0..4] as above, out[1] the plain mse, and
 *   out[2] = 255^2 * (1/N) * sum_n lmbda_n * mse_n + bpp;   dx_hat of image n = gscale * lmbda_n*255^2*2*(x_hat-x)/(N*img_elems)
 * Sums are fixed-order per image, then over images in index order (no float atomics: equal inputs give bit-identical
 * results).  ICM_ERR_ARG: a null pointer, N, img_elems or num_pixels < 1, or 3 * N > ICM_REDUCE_WS_FLOATS (every image
 * needs a workgroup's three partial sums in ws). */
int icm_rd_loss_w_fwd(const float* x, const float* x_hat, int N, int64_t img_elems, const float* lik_y, int64_t n_y,
                      const float* lik_z, int64_t n_z, int64_t num_pixels, const float* lmbda_n, float* out, float* ws,
                      void* stream);
int icm_rd_loss_w_bwd(const float* x, const float* x_hat, int N, int64_t img_elems, const float* lik_y, int64_t n_y,
                      const float* lik_z, int64_t n_z, int64_t num_pixels, const float* lmbda_n, float gscale,
                      float* dx_hat, float* dlik_y, float* dlik_z, void* stream);
/* The same with a distortion weight per cell x cell block of pixels (quality-map training): x / x_hat are [N][C][H][W],
 * qmap [N][H/cell][W/cell] int8 step indexes and lmbda_table 256 f32 weights indexed by the map byte read as unsigned,
 * both in DEVICE memory.  With lmbda_i the table entry of the cell that holds pixel i:
 *   out[2] = 255^2 * (sum_i lmbda_i * (x_hat_i - x_i)^2) / (N*C*H*W) + bpp;   out[1] the plain mse;
 *   dx_hat_i = gscale * lmbda_i * 255^2 * 2 / (N*C*H*W) * (x_hat_i - x_i);   dlik as above.
 * Sums are fixed-order (no float atomics: equal inputs give bit-identical results).  Every workgroup writes four
 * partial sums to ws (plain and weighted squared error, the two log-likelihood sums), and every image has a workgroup
 * at least, so ICM_ERR_ARG for 4 * N > ICM_REDUCE_WS_FLOATS; also for a null pointer, N, C, H, W or num_pixels < 1,
 * cell < 1, H or W no multiple of cell, C * H > 2^30 -- all before any launch. */
int icm_rd_loss_m_fwd(const float* x, const float* x_hat, int N, int C, int H, int W, int cell, const int8_t* qmap,
                      const float* lmbda_table, const float* lik_y, int64_t n_y, const float* lik_z, int64_t n_z,
                      int64_t num_pixels, float* out, float* ws, void* stream);
int icm_rd_loss_m_bwd(const float* x, const float* x_hat, int N, int C, int H, int W, int cell, const int8_t* qmap,
                      const float* lmbda_table, const float* lik_y, int64_t n_y, const float* lik_z, int64_t n_z,
                      int64_t num_pixels, float gscale, float* dx_hat, float* dlik_y, float* dlik_z, void* stream);

/* ---- MS-SSIM (Wang, Simoncelli, Bovik 2003; the defaults of pytorch_msssim.ms_ssim, which the reference's evaluation
 * CLI imports at compressai/utils/eval_model/__main__.py:32 and reports under the key "ms-ssim", :135) ------------
 * x, y: contiguous [N,C,H,W] in [0, data_range]; 11-tap Gaussian window (sigma 1.5), valid filtering, five levels with
 * weights {0.0448, 0.2856, 0.3001, 0.2363, 0.1333}, 2x2 average pooling (padding = size % 2) between levels,
 * relu on every level value.  min(H, W) must exceed 160 (ICM_ERR_ARG otherwise, like the package's assert).
 * ws: icm_msssim_workspace_floats(N, C, H, W) floats (0 = geometry refused); it holds the image pyramid, the
 * per-workgroup partial sums (added in tile order: no float atomics, equal inputs give bit-identical results), the
 * per-level upstream factors and the three coefficient maps per level the backward filters -- so icm_msssim_bwd must
 * follow icm_msssim_fwd of the same inputs on the same ws, with no host read in between (graph-capture safe).
 * fwd: ms[N*C] = prod_l v_l^w_l per plane; out[0] = mean(ms), out[1] = 1 - mean(ms);
 *      loss_io != NULL: *loss_io += lmbda * (1 - mean(ms))   (the trainer's loss scalar, which holds bpp by then).
 * bwd: dx = d(sum_p up[p] * ms[p]) / dx with up[p] = gscale * gplane[p], or gscale / (N*C) when gplane == NULL
 *      (the gradient of gscale * mean(ms)); a plane with a non-positive level value gets an all-zero gradient.
 *      Only x (the reconstruction) receives a gradient. */
int64_t icm_msssim_workspace_floats(int N, int C, int H, int W);
int icm_msssim_fwd(const float* x, const float* y, int N, int C, int H, int W, float data_range, float* ms, float* out,
                   float lmbda, float* loss_io, float* ws, int64_t ws_floats, void* stream);
int icm_msssim_bwd(const float* x, const float* y, int N, int C, int H, int W, const float* gplane, float gscale,
                   float* dx, float* ws, int64_t ws_floats, void* stream);

/* ---- optimiser (train.py:105-169,199-214) ---------------------------------------------------- */
/* out[0] = sum g^2; ws: ICM_REDUCE_WS_FLOATS floats of scratch (fixed-order two-stage sum: every rank of a
 * data-parallel job derives the same clip coefficient from the same all-reduced gradient) */
int icm_grad_sqnorm(const float* g, int64_t n, float* out, float* ws, void* stream);
/* Adam step with fused clip: coef = min(1, max_norm/(sqrt(*sqnorm)+1e-6)) if sqnorm!=NULL else 1;
 * g is scaled by gscale (1/world_size) then coef; torch.optim.Adam defaults semantics. */
int icm_adam_step(float* p, const float* g, float* m, float* v, int64_t n, double lr, double beta1, double beta2,
                  double eps, int step, const float* sqnorm, float max_norm, float gscale, void* stream);
/* the same update with the two step-dependent scalars read from DEVICE memory -- hyper[0] = lr / (1 - beta1^step),
 * hyper[1] = sqrt(1 - beta2^step), formed by the caller in double and rounded to f32 exactly as icm_adam_step forms
 * them -- so that a captured hipGraph of the training step can be replayed (kernel arguments are frozen at capture) */
int icm_adam_step_hyper(float* p, const float* g, float* m, float* v, int64_t n, double beta1, double beta2, double eps,
                        const float* hyper, const float* sqnorm, float max_norm, float gscale, void* stream);
int icm_fill(float* p, int64_t n, float v, void* stream);
/* x_hat.clamp_(0, 1) of decompress() (cnn.py:330) */
int icm_clamp(float* p, int64_t n, float lo, float hi, void* stream);
/* F.pad(x, (left, ., top, .), value) / its negative-pad crop around the codec (utils/eval_model/__main__.py:102-117,
 * 129-131): dst [N,C,OH,OW], dst[y][x] = src[y - top][x - left] inside the source, `value` outside */
int icm_pad2d(const float* src, int N, int C, int H, int W, float* dst, int OH, int OW, int top, int left, float value,
              void* stream);

/* ---- 8-bit image boundary of the codec (icm_amd/codec.py; no counterpart in the reference, whose evaluation loop does
 * this work on the host: torchvision ToTensor + F.pad before compress(), crop + clamp + ToPILImage after decompress(),
 * utils/eval_model/__main__.py:83-117,89-94,129-131).  Images are single, RGB, at most 32768 pixels a side.
 * u8_to_f32: src = interleaved [H, W, 3] bytes; dst = planar [1, 3, OH, OW] f32 with dst[c][top + y][left + x] =
 *   src[y][x][c] / 255 (the correctly rounded quotient, ToTensor's value bit for bit) and +0.0 everywhere else: every
 *   element of dst is written exactly once, the caller does not clear it.  Needs top, left >= 0, top + H <= OH,
 *   left + W <= OW.
 * f32_to_u8: src = planar [1, 3, PH, PW] f32; dst = interleaved [H, W, 3] bytes of the window at (top, left),
 *   dst[y][x][c] = (uint8)(min(max(src[c][top + y][left + x], 0), 1) * 255), truncated (ToPILImage); NaN input is
 *   unspecified.  ref != NULL (interleaved [H, W, 3] bytes): the same pass leaves one 64-bit partial sum of
 *   (dst - ref)^2 per workgroup in ws (icm_image_workspace_bytes(H, W) bytes, 8-byte aligned) and a second launch adds
 *   them in index order into *sse (device memory, 8-byte aligned).  Integer sums: exact and order-independent; no
 *   atomics, no host read in between.  ref == NULL: sse / ws are not touched and may be NULL.
 * No pointer needs more than its natural alignment: runs whose bytes are not 16-byte aligned take a per-pixel path. */
int64_t icm_image_workspace_bytes(int H, int W);   /* 0 = bad geometry */
int icm_image_u8_to_f32(const uint8_t* src, int H, int W, float* dst, int OH, int OW, int top, int left, void* stream);
int icm_image_f32_to_u8(const float* src, int PH, int PW, int top, int left, uint8_t* dst, int H, int W,
                        const uint8_t* ref, int64_t* sse, void* ws, int64_t ws_bytes, void* stream);

/* ---- luma statistics per latent cell (icm_amd/codec.py, variance-adaptive quality maps of the encoder; no counterpart
 * in the reference).  img = interleaved [H, W, 3] bytes; the grid of gh x gw cells of 16 x 16 pixels is that of the
 * image padded by top rows and left columns: pixel (y, x) lies in cell ((top + y) / 16, (left + x) / 16).  With the
 * integer luma Y = (77 R + 150 G + 29 B + 128) >> 8 (0..255), stats = [gh][gw][3] int32 = (n, s1, s2) per cell: n the
 * image pixels in the cell (0..256; pad pixels are no pixels, a cell wholly in the padding holds 0, 0, 0), s1 the sum
 * of Y (<= 65 280), s2 the sum of Y^2 (<= 16 646 400).  Integer sums: exact, whatever the order.  Every entry of stats
 * is written exactly once, the caller does not clear it.  One launch, no atomics, no allocation, no synchronisation
 * (graph-capturable); one streaming read of the 3 H W bytes.  No pointer needs more than its natural alignment.
 * ICM_ERR_ARG before the launch: null pointers, H, W, gh or gw < 1, top or left < 0, a grid that does not cover the
 * image (top + H > 16 gh or left + W > 16 gw), gh or gw above 2^26 (or more than 2^31 - 1 workgroups). */
int icm_image_cell_stats(const uint8_t* img, int H, int W, int top, int left, int gh, int gw, int32_t* stats,
                         void* stream);

/* ---- assembly of a tiled image (icm_amd/codec.py, ICMT streams; no counterpart in the reference).  One decoded tile
 * is added into the zero-filled f32 canvas of the image, its overlap bands weighted by a ramp:
 *   canvas[c][y0 + y][x0 + x] = canvas[c][y0 + y][x0 + x] + (wy(y) * wx(x)) * src[c][top + y][left + x]
 * for 0 <= y < h, 0 <= x < w, c < 3; src = planar [3, PH, PW], canvas = planar [3, H, W].  The two products and the sum
 * are evaluated in that association, each rounded once (no FMA).  edges names the sides of the window that have a
 * neighbouring tile (ICM_TILE_EDGE_*).  wx(x) = ramp[x] if the left side has a neighbour and x < m; otherwise
 * ramp[w - 1 - x] if the right side has one and w - 1 - x < m; otherwise 1.  wy(y) likewise with top / bottom / h.
 * ramp = m floats in device memory, by convention (i + 0.5) / m formed in f32 on the host; m = 0: ramp is not read.
 * Elements outside the window are not touched.  Tiles issued on one stream add in issue order: no atomics, two runs
 * are bit-identical.  Plane offsets are 64-bit (3 H W may exceed 2^31); no pointer needs more than float alignment.
 * ICM_ERR_ARG before any launch: null src / canvas, a size outside 1..32768, negative top / left / y0 / x0, a window
 * outside src or outside the canvas, m < 0, m > 0 with a null ramp, edges outside 0..15, m > w with a left or right
 * neighbour, m > h with a top or bottom one. */
#define ICM_TILE_EDGE_LEFT 1
#define ICM_TILE_EDGE_RIGHT 2
#define ICM_TILE_EDGE_TOP 4
#define ICM_TILE_EDGE_BOTTOM 8
int icm_image_tile_blend(const float* src, int PH, int PW, int top, int left, int h, int w,
                         float* canvas, int H, int W, int y0, int x0,
                         const float* ramp, int m, int edges, void* stream);

/* ---- error-bounded residual layer of the codec (icm_amd/residual.py, ICMR streams; no counterpart in the reference).
 * x = the original image, xhat = the decoder's reconstruction of the base stream, both interleaved [H, W, 3] bytes;
 * D = the bound, 0..32, s = 2 D + 1.  Integer arithmetic only:
 *   q = sign(x - xhat) ((|x - xhat| + D) div s),   xtilde = min(max(xhat + q s, 0), 255),   |x - xtilde| <= D.
 * Symbols, indexes = planar [3, H, W] int32, image pixels only.  Classes = [gh, gw] int32 over the 16 x 16-pixel cells
 * of the grid anchored at pixel (0, 0), gh = ceil(H / 16), gw = ceil(W / 16), edge cells partial, one class for the
 * three channels: with N the samples of the cell (3 x its pixels) and S the sum of |q| over them, the class is the
 * number of thresholds T_j = round(2^(1 + j / 2)), j = 0..17, with 16 S > N T_j (an integer comparison): 0..18.
 * residual_code: one wave per cell forms q from the cell's two blocks of bytes, reduces S across the wave and writes
 *   the cell's symbols, its indexes (= its class) and classes[cell].
 * residual_indexes: the decoder's expansion, indexes[c][y][x] = classes[y / 16][x / 16], the value as found (classes as
 *   decoded, in device memory; a value outside the tables is the entropy decoder's to flag).
 * residual_apply: out = interleaved [h, w, 3] bytes, xtilde of the window (y0, x0, h, w) of the image from xhat =
 *   interleaved [h, w, 3] bytes of that window and the whole image's symbols; the full image is the window
 *   (0, 0, H, W).  Any int32 symbol gives the value of the exact integers (no overflow).
 * Each: one launch, no atomics, no allocation, no synchronisation (graph-capturable); every output element is written
 * exactly once, the caller does not clear it.  No pointer needs more than its natural alignment: runs of four pixels
 * whose bytes are not dword-aligned, or whose int32 are not 16-byte aligned, move one at a time.
 * ICM_ERR_ARG before the launch: null pointers, H, W, h or w outside 1..32768, D outside 0..32, y0 or x0 < 0, a window
 * outside the image. */
int icm_residual_code(const uint8_t* x, const uint8_t* xhat, int H, int W, int D, int32_t* symbols, int32_t* indexes,
                      int32_t* classes, void* stream);
int icm_residual_indexes(const int32_t* classes, int H, int W, int32_t* indexes, void* stream);
int icm_residual_apply(const uint8_t* xhat, const int32_t* symbols, int H, int W, int y0, int x0, int h, int w, int D,
                       uint8_t* out, void* stream);
/* The same two operations under a bound per cell (ICME streams): dmap = [gh, gw] bytes in DEVICE memory over the grid
 * of the classes, anchored at pixel (0, 0) of the whole image; a sample of cell (cy, cx) is coded and applied with
 * D = min(dmap[cy][cx], 32) by the rule above, and the class of a cell is taken from its own q.  The entries cannot
 * look into a device map before the launch, hence the min: a byte above 32 counts as 32 in both kernels.  A uniform
 * map gives bit for bit the outputs of the scalar entries of that D.
 * residual_code_map: a wave owns a cell and reads its byte once.
 * residual_apply_map: the cell of a window pixel is that of its image position (y0 + y, x0 + x); a run of four window
 *   pixels that straddles a cell boundary of the image takes each pixel's own bound.
 * Launch, alignment and ICM_ERR_ARG as above (no D to check; dmap must not be null). */
int icm_residual_code_map(const uint8_t* x, const uint8_t* xhat, int H, int W, const uint8_t* dmap, int32_t* symbols,
                          int32_t* indexes, int32_t* classes, void* stream);
int icm_residual_apply_map(const uint8_t* xhat, const int32_t* symbols, int H, int W, int y0, int x0, int h, int w,
                           const uint8_t* dmap, uint8_t* out, void* stream);
/* The decoder's operations on a band of the planes, what a region decode has of the symbols: indexes / symbols =
 * [3, e_hi - e_lo] int32, plane c's elements e_lo <= e < e_hi of the row-major [H, W] plane at c (e_hi - e_lo) + e -
 * e_lo.  A band starts and ends anywhere in a row (it is a range of a lane stream's waves, not of rows).
 * residual_indexes_band: writes every element of the band, from the whole image's classes [gh, gw] (only the cell rows
 *   the band touches are read).
 * residual_apply_band / residual_apply_map_band: as residual_apply / residual_apply_map; every sample of the window
 *   must lie inside the band.
 * The same kernels and element bodies: the entries above are the band [0, H W) and keep their results bit for bit.
 * Launch, alignment and ICM_ERR_ARG as above; also ICM_ERR_ARG unless 0 <= e_lo < e_hi <= H W and, for the two apply
 * entries, y0 W + x0 >= e_lo and (y0 + h - 1) W + x0 + w <= e_hi. */
int icm_residual_indexes_band(const int32_t* classes, int H, int W, int64_t e_lo, int64_t e_hi, int32_t* indexes,
                              void* stream);
int icm_residual_apply_band(const uint8_t* xhat, const int32_t* symbols, int H, int W, int64_t e_lo, int64_t e_hi,
                            int y0, int x0, int h, int w, int D, uint8_t* out, void* stream);
int icm_residual_apply_map_band(const uint8_t* xhat, const int32_t* symbols, int H, int W, int64_t e_lo, int64_t e_hi,
                                int y0, int x0, int h, int w, const uint8_t* dmap, uint8_t* out, void* stream);

/* ---- device-resident training data (icm_amd/datasets.py DeviceImageCache; stands in for the reference's per-step
 * CenterCrop / RandomCrop(pad_if_needed) + ToTensor + collate on the host, train.py:393-425).  A training batch cut out
 * of an arena of 8-bit images in one launch: sample b is the interleaved [H, W, 3] byte image at arena + offset, and
 *   dst[b][c][y][x] = src[y0 + y][x0 + x][c] / 255   (the same table as icm_image_u8_to_f32: ToTensor's value)
 * with +0.0 wherever (y0 + y, x0 + x) lies outside the image; y0 / x0 are signed (padding crops start at negative
 * coordinates) and lie in [-2^30, 2^30].  dst = planar [B, 3, CH, CW] f32, every element written exactly once, the
 * caller does not clear it.  desc = B descriptors in DEVICE memory, produced and checked by the caller: the kernel
 * trusts them and reads only inside [offset, offset + 3 H W) of each image.  One launch, no atomics, no allocation, no
 * synchronisation (graph-capturable).  No pointer needs more than its natural alignment (desc: 8 bytes).
 * ICM_ERR_ARG before any launch: null pointers, B < 1, CH or CW outside 1..32768 (or more than 2^31 - 1 workgroups). */
typedef struct { int64_t offset; int32_t H, W, y0, x0; } icm_crop_desc;   /* 24 bytes */
int icm_image_batch_u8_to_f32(const uint8_t* arena, const icm_crop_desc* desc, int B, float* dst /* [B,3,CH,CW] */,
                              int CH, int CW, void* stream);

/* ---- test hooks (process-global; used by the parity tests, the recorded-plan tests and tools/tune_conv.py only) ----
 * force the implicit-GEMM tile configuration: a row of the kernel table of conv_igemm.hip (0-12), one of the two block
 * shapes of the 8-wave K-split kernel of conv_ks8.hip where it is eligible (ICM_CONV_CFG_KS8_*), or
 * ICM_CONV_CFG_AUTO (any negative value).  While a configuration is forced no launch takes the pointwise kernel.
 * icm_debug_force_wgrad_cfg: the weight-gradient
 * kernel variant (0-2 general kernel <2,1,7> / <2,2,9> / <4,4,4>; 3-6 three-by-three tiles per wave <3,3> / <6,6> /
 * <3,6> / <6,3>; 7 its tap-per-wave form; 8 / 9 nine taps from one DMA staging, 96 / 64-wide blocks; 10 the 25-tap
 * 5x5 form; 11-14 the DMA-only 1x1 kernel <6,6> / <3,6> / <6,3> / <3,3>; -1 = automatic) and its XCD-aware
 * workgroup order (0 / 1, -1 = automatic) */
#define ICM_CONV_CFG_AUTO (-1)
#define ICM_CONV_CFG_KS8_64X64 100    /* 64 co x 64 px blocks */
#define ICM_CONV_CFG_KS8_32X128 101   /* 32 co x 128 px blocks */
void icm_debug_force_conv_cfg(int idx);
/* the value in force (ICM_CONV_CFG_AUTO = automatic): callers that choose between the direct and the Winograd form keep
 * the direct one while a tile configuration is forced */
int icm_debug_forced_conv_cfg(void);
/* pointwise (1x1 stride-1, Cin % 8 == 0) convolutions: -1 = automatic (the barrier-free direct-operand kernel when the
 * launch has >= 1024 waves), 0 = always the LDS-staged kernel, 1 = the direct kernel whenever eligible */
void icm_debug_force_conv1x1(int mode);
/* what a forward / input-gradient launch of these ngroups members would be, for tap class cls (a transposed stride-2
 * launch has four classes, every other launch one): validation, the member-agreement check and the plan step of
 * icm_conv_run_grouped, and nothing else -- pure host code, pointers are looked at for null-ness and alignment only.
 * Honours icm_debug_force_conv_cfg, icm_debug_force_conv1x1 and a->algo.  Returns the code the launch would return and
 * fills (all 0 unless ICM_OK)
 *   out = {classes, family, cfg row or co tiles per block, lgTW|lgTX, lgTH|lgTY, lgTI, ckm|nsteps, co blocks, workgroups
 *          per member (0: an empty class, nothing launched), dynamic LDS bytes, block threads, vec4|vpre, dma|px_fast,
 *          offset of the class in the packed weights in floats, 0, 0}
 * family: 0 LDS-staged implicit GEMM (cfg row of its table), 1 8-wave K-split (co tiles per block), 2 pointwise (row of
 * its table), 3 Winograd 4 + 4 waves, 4 Winograd eight MFMA waves (both: co tiles per workgroup; the | alternatives). */
int icm_debug_conv_plan(const icm_conv_args* a, int ngroups, int cls, int64_t out[16]);
void icm_debug_force_wgrad_cfg(int variant, int xcd_order);
/* what the planner of the direct weight-gradient kernels decides for n problems of geometry *a (pure host code; honours
 * the forced variant): returns its code and fills out = {variant, lgNPX, lgTW, lgTH, lgTI, taps per group, pixel
 * splits, dynamic LDS bytes} (all 0 unless ICM_OK) */
int icm_debug_wgrad_plan(const icm_wgrad_args* a, int n, int32_t out[8]);
/* 1: window attention always runs the generic VALU kernels (the matrix-core kernels cover 8x8 windows) */
void icm_debug_force_winattn_valu(int on);
/* which kernel family icm_winattn_fwd (backward = 0) / icm_winattn_bwd (backward = 1) gives this geometry to: 0 the
 * generic VALU kernels, 1 the matrix-core kernels for 8x8 windows, 2 the matrix-core kernels for 4x4 windows; or, for a
 * geometry the call refuses, minus its ICM_ERR_* code (the codes are small positive integers too, so they come back
 * negated: -ICM_ERR_ARG, -ICM_ERR_UNSUPPORTED).  The decision the launches use, not a restatement; pure host code, no
 * HIP call; honours icm_debug_force_winattn_valu. */
int icm_debug_winattn_route(int N, int C, int H, int W, int heads, int ws, int shift, int backward);

#ifdef __cplusplus
}
#endif
#endif
