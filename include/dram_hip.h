/*
 * dram_hip.h -- C ABI of libdram_hip.so: the MI355X (gfx950) kernels under the
 * DRAM DC3D forward/backward hot path.
 *
 * The reference (DIAGNijmegen/bodyct-dram) has no FFI: its hot path is the set
 * of ATen ops that dram/parts.py and dram/models.py dispatch.  Each entry point
 * below replaces one of those dispatches; the comment above it cites the
 * reference line that issues the op.  The Python host side
 * (bodyct-dram_amd/dram_amd/) binds these with ctypes; INTEGRATION.md shows the
 * stub.
 *
 * Conventions
 *   - every tensor is fp32, NCDHW, contiguous, in device (HBM) memory;
 *   - S = D*H*W; "row" = one (n, c) pair = S contiguous floats;
 *   - `stream` is a hipStream_t passed as void*; every call is asynchronous on
 *     it and performs no allocation and no host synchronisation;
 *   - `ws` is caller-provided device scratch of at least the size returned by
 *     the matching *_ws_bytes() query (may be NULL when that size is 0);
 *   - return value: 0 on success, a negative DRAM_E* code otherwise (nothing is
 *     launched on an argument error); dram_last_error() gives the message of
 *     the calling thread's last failure.
 */
#ifndef DRAM_HIP_H
#define DRAM_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DRAM_OK 0
#define DRAM_EINVAL (-1)  /* bad shape / null pointer / unsupported argument */
#define DRAM_EWS (-2)     /* workspace too small */
#define DRAM_EHIP (-3)    /* HIP runtime error at launch */

/* norm kinds for dram_norm_* (reference parts.py:17-35 normal_wrapper) */
#define DRAM_NORM_BATCH 0 /* statistics per channel over (N, D, H, W): "bn", "bnt", "bntna", "sbn" */
#define DRAM_NORM_GROUP 1 /* statistics per (sample, group): "ln"/"lnna" (G=1), "in" (G=C) */

const char* dram_last_error(void);
int dram_abi_version(void);

/* ---- 3x3x3 convolution, stride 1, zero padding 1 (nn.Conv3d at parts.py:95,105,133,142,177,185) ----
 *
 * The kernels take the filter in a packed, GEMM-friendly form of dram_conv3d_k3_packed_floats(Cout, Cin)
 * floats that dram_conv3d_k3_pack_weights builds from the reference's [Cout][Cin][3][3][3] parameter:
 *   wt[27][Cin][Cout] (tap-major, Cout fastest) for the direct kernel, followed by
 *   wz[9*4][Cin][Cout], the Winograd F(2,3)-along-z transformed filters ((ky,kx) column x 4 transformed taps).
 *   mode 0 (forward):  wt[t][ci][co] = w[co][ci][t]
 *   mode 1 (backward-data): wt[t][co][ci] = w[co][ci][26-t], i.e. the filter
 *          of the transposed convolution -- run dram_conv3d_k3_fwd_ex on dy with
 *          Cin/Cout swapped to obtain dx.
 * Which kernel runs is the library's choice (Winograd-z for Cin >= 8; exact fp32 arithmetic either way).
 */
size_t dram_conv3d_k3_packed_floats(int Cout, int Cin);
int dram_conv3d_k3_pack_weights(const float* w, float* wt, int Cout, int Cin, int mode, void* stream);

/* y = conv3d(x, w) (+ bias[Co1+Co2] when bias != NULL), forward and backward-data.  The INPUT is the channel
 * concatenation of two tensors that is never materialised: channels [0,C1) come from x1[N,C1,D,H,W]; channels
 * [C1,C1+C2) from x2[N,C2,D2,H2,W2] centre-cropped with start offsets (oz,oy,ox) -- crop_concat_5d of
 * parts.py:37-46 fused into the consumer conv (parts.py:153-154); x2 == NULL: x1 only.  The OUTPUT
 * channels are split the same way over y1[N,Co1,D,H,W] and, when y2 != NULL, the crop window
 * (yoz,yoy,yox) of y2[N,Co2,yD2,yH2,yW2] (elements of y2 outside the window are not written:
 * zero them first when the window is smaller than y2).  wt is [27][C1+C2][Co1+Co2]. */
int dram_conv3d_k3_fwd_ex(const float* x1, int C1, const float* x2, int C2, int D2, int H2, int W2,
                          int oz, int oy, int ox, const float* wt, const float* bias,
                          float* y1, int Co1, float* y2, int Co2, int yD2, int yH2, int yW2,
                          int yoz, int yoy, int yox, int N, int D, int H, int W, void* stream);

/* Workspace of backward-weights (dram_conv3d_k3_wgrad_fused below): per-block partial slabs of dw, summed in a fixed
 * order.  Cin = C1 + C2 of a virtual concatenation. */
size_t dram_conv3d_k3_wgrad_ws_bytes(int N, int Cin, int Cout, int D, int H, int W);

/* dbias[Cout] = sum over (n,z,y,x) of dy (conv_bias=True when norm_method is None, models.py:78). */
size_t dram_channel_sum_ws_bytes(int N, int C, int64_t S);
int dram_channel_sum(const float* dy, float* dbias, void* ws, size_t ws_bytes, int N, int C, int64_t S, void* stream);

/* ---- general 3-D convolution: kernel 1..7, zero padding 0..max(k-1, 1), stride 1 or 2 per axis; dilation 1, groups 1
 * (nn.Conv3d of parts.py:66-196 / models.py:54-112 with kernel_sizes, padding_list, conv_strides other than 3x3x3/pad 1
 * and 1x1x1/pad 0) ----
 * Shapes: x[N,Cin,D,H,W], w[Cout,Cin,kz,ky,kx] (the parameter's own layout), y[N,Cout,OD,OH,OW] with
 * O = (I + 2p - k) / s + 1 per axis (>= 1, else DRAM_EINVAL).  Geometry outside the limits above is DRAM_EINVAL, checked
 * before anything is launched. */
int dram_conv3d_fwd(const float* x, const float* w, const float* bias, float* y, int N, int Cin, int Cout, int D, int H,
                    int W, int kz, int ky, int kx, int sz, int sy, int sx, int pz, int py, int px, void* stream);
/* dx[N,Cin,D,H,W] from dy[N,Cout,OD,OH,OW]; D,H,W are the sizes of x (they fix OD,OH,OW as above). */
int dram_conv3d_bwd_data(const float* dy, const float* w, float* dx, int N, int Cin, int Cout, int D, int H, int W,
                         int kz, int ky, int kx, int sz, int sy, int sx, int pz, int py, int px, void* stream);
/* dw[Cout,Cin,kz,ky,kx] = sum over (n, output voxel) of dy * x at the tap; deterministic (per-block partial slabs in
 * `ws`, summed in a fixed order).  _ws_bytes returns 0 for an unsupported geometry. */
size_t dram_conv3d_wgrad_ws_bytes(int N, int Cin, int Cout, int D, int H, int W, int kz, int ky, int kx, int sz, int sy,
                                  int sx, int pz, int py, int px);
int dram_conv3d_wgrad(const float* x, const float* dy, float* dw, void* ws, size_t ws_bytes, int N, int Cin, int Cout,
                      int D, int H, int W, int kz, int ky, int kx, int sz, int sy, int sx, int pz, int py, int px,
                      void* stream);
/* launches per kernel family (index = DRAM_CONV_GEN_*) since the library was loaded, into counts[0..n) */
#define DRAM_CONV_GEN_FWD 0       /* conv3d_gen_fwd_kernel, forward */
#define DRAM_CONV_GEN_BWD_DATA 1  /* conv3d_gen_fwd_kernel, one launch per backward-data output phase */
#define DRAM_CONV_GEN_WGRAD 2     /* conv3d_gen_wgrad_kernel (+ slab reduce) */
#define DRAM_CONV_GEN_KINDS 3
int dram_conv3d_gen_launch_counts(unsigned long long* counts, int n);

/* ---- normalisation (+ fused ReLU) (normal_wrapper parts.py:17-35, act_wrapper parts.py:48-54) ----
 *
 * Training-mode forward: computes statistics of x (two-level Chan/Welford
 * combination, fp64 finalise), writes y = act(gamma * (x - mean) * rstd + beta).
 *   kind = DRAM_NORM_BATCH: one statistic per channel; save_mean/save_rstd have
 *          C entries; when running_mean != NULL the running statistics are
 *          updated in place with `momentum` (unbiased variance), as
 *          nn.BatchNorm3d does.
 *   kind = DRAM_NORM_GROUP: one statistic per (n, group); save_* have N*G entries.
 * gamma/beta may be NULL (affine=False).  relu != 0 fuses nn.ReLU.
 * Also fills rowcoef[2*N*C] = {a,b} with y_pre = a*x + b per row, which the
 * backward entry point reuses.
 */
size_t dram_norm_ws_bytes(int N, int C, int64_t S);
int dram_norm_fwd_train(const float* x, const float* gamma, const float* beta, float* y,
                        float* save_mean, float* save_rstd, float* rowcoef,
                        float* running_mean, float* running_var, float momentum, float eps,
                        int kind, int G, int relu, int N, int C, int64_t S,
                        void* ws, size_t ws_bytes, void* stream);

/* Eval-mode BatchNorm: y = act(gamma * (x - running_mean) / sqrt(running_var + eps) + beta);
 * fills save_mean/save_rstd/rowcoef like the training entry so backward works. */
int dram_bn_fwd_eval(const float* x, const float* gamma, const float* beta,
                     const float* running_mean, const float* running_var, float* y,
                     float* save_mean, float* save_rstd, float* rowcoef,
                     float eps, int relu, int N, int C, int64_t S, void* stream);

/* Backward of the above.  dy is the gradient w.r.t. the (activated) output; x is
 * the saved input; the ReLU mask is recomputed from rowcoef.  Outputs dx (may
 * alias dy), dgamma[C], dbeta[C] (either may be NULL).  `batch_stats` = 1 when
 * the forward used the statistics of x itself (training), 0 for eval-mode BN. */
int dram_norm_bwd(const float* dy, const float* x, const float* gamma,
                  const float* save_mean, const float* save_rstd, const float* rowcoef,
                  float* dx, float* dgamma, float* dbeta,
                  int kind, int G, int relu, int batch_stats, int N, int C, int64_t S,
                  void* ws, size_t ws_bytes, void* stream);

/* dram_norm_bwd with the incoming gradient taken from where it comes from instead of from a tensor someone wrote first.
 * Same workspace, same kernels but for the load of dy, same dgamma / dbeta; dx, bit for bit, what dram_norm_bwd gives on
 * the materialised gradient (the 16-byte row kernels are chosen as dram_norm_bwd chooses them, with g resp. dy in the place of
 * its dy, so the sums run in the same order; _head: for a g that is 16-byte aligned when dx is).
 *   _head:     dy[n,c,e] = sum_o w[o,c] * g[n,o,e], the input gradient of a 1x1x1 conv (dram_conv3d_k1_bwd's dx, formed
 *              with that kernel's fmaf chain) with weight w[Cout,C] and output gradient g[N,Cout,S].  dx must not alias g.
 *              Cout within dram_norm_bwd_head_ok (one pass of the 1x1x1 kernels); otherwise DRAM_EINVAL, nothing launched.
 *   _pool_add: dy + dram_maxpool3d_2_bwd(gp, idx), the sum dram_maxpool3d_2_bwd_acc leaves in dy; S = D*H*W,
 *              gp / idx [N,C,D/2,H/2,W/2].  dx may alias dy. */
int dram_norm_bwd_head_ok(int Cout);
int dram_norm_bwd_head(const float* g, const float* w, int Cout, const float* x, const float* gamma,
                       const float* save_mean, const float* save_rstd, const float* rowcoef,
                       float* dx, float* dgamma, float* dbeta,
                       int kind, int G, int relu, int batch_stats, int N, int C, int64_t S,
                       void* ws, size_t ws_bytes, void* stream);
int dram_norm_bwd_pool_add(const float* dy, const float* gp, const uint8_t* idx, int D, int H, int W,
                           const float* x, const float* gamma,
                           const float* save_mean, const float* save_rstd, const float* rowcoef,
                           float* dx, float* dgamma, float* dbeta,
                           int kind, int G, int relu, int batch_stats, int N, int C,
                           void* ws, size_t ws_bytes, void* stream);

/* ---- cross-rank BatchNorm (normal_wrapper "sbn" = nn.SyncBatchNorm, dram/parts.py:32-33, under data parallelism) ----
 * The statistics and the backward sums leave the device between two stages so that the host can exchange them
 * (all-gather / all-reduce over RCCL); every stage is the same row kernels as above.
 *   forward:  dram_bn_stats -> {mean, M2} per channel (fp64) of the local batch; combine over ranks on the host
 *             side (Chan); then dram_bn_fwd_eval with the global mean / biased variance.
 *   backward: dram_bn_bwd_sums -> {sum dy', sum dy'*xhat} per channel (= dbeta, dgamma of the local batch);
 *             all-reduce; dram_bn_bwd_apply_sums with the global sums and element count.
 * Workspace: dram_norm_ws_bytes(N, C, S). */
int dram_bn_stats(const float* x, double* mean_m2, int N, int C, int64_t S, void* ws, size_t ws_bytes, void* stream);
int dram_bn_bwd_sums(const float* dy, const float* x, const float* save_mean, const float* save_rstd,
                     const float* rowcoef, double* sums, int relu, int N, int C, int64_t S, void* ws,
                     size_t ws_bytes, void* stream);
int dram_bn_bwd_apply_sums(const float* dy, const float* x, const float* gamma, const float* save_mean,
                           const float* save_rstd, const float* rowcoef, const double* sums, double count,
                           float* dx, int relu, int N, int C, int64_t S, void* ws, size_t ws_bytes, void* stream);

/* Stand-alone activations (act_wrapper parts.py:48-54 when no norm precedes them). */
int dram_relu_fwd(const float* x, float* y, int64_t n, void* stream);
int dram_relu_bwd(const float* dy, const float* y, float* dx, int64_t n, void* stream);

/* ---- nn.MaxPool3d(2, 2, 0) (parts.py:191) ----
 * out[N,C,D/2,H/2,W/2]; idx (uint8, 0..7 = dz*4+dy*2+dx) records the first
 * maximum in (z,y,x) scan order -- the element ATen routes the gradient to. */
int dram_maxpool3d_2_fwd(const float* x, float* out, uint8_t* idx, int N, int C, int D, int H, int W, void* stream);
int dram_maxpool3d_2_bwd(const float* dout, const uint8_t* idx, float* dx, int N, int C, int D, int H, int W, void* stream);

/* ---- nn.MaxPool3d(kernel, stride, padding), dilation 1, floor mode (pool_ksize / pool_strides / pool_pad of
 * ConvPoolBlock5d, parts.py:157-196) ----
 * Per axis: kernel 1..5, stride 1..5, padding 0..kernel/2 (torch's rule), output extent (n + 2p - k) / s + 1 >= 1;
 * anything else is DRAM_EINVAL and nothing is launched.  out, idx: [N,C,Do,Ho,Wo].  The window is scanned in (z,y,x) order
 * and positions in the padding are skipped; idx (uint8) = (dz*kh + dy)*kw + dx inside the unclipped window (<= 124) of the
 * first maximum -- a NaN propagates and the last NaN of the scan takes the index -- the element ATen routes the gradient to.
 * _bwd is the gather form (one thread per input element, ascending (zo,yo,xo) over the windows that hold it, deterministic,
 * no atomics) and writes all of dx: elements that no window covers (stride > kernel, floor remainder) get +0.
 * A 2 / 2 / 0 pool runs dram_maxpool3d_2_* above. */
int dram_maxpool3d_fwd(const float* x, float* out, uint8_t* idx, int N, int C, int D, int H, int W, int kd, int kh, int kw,
                       int sd, int sh, int sw, int pd, int ph, int pw, void* stream);
int dram_maxpool3d_bwd(const float* dout, const uint8_t* idx, float* dx, int N, int C, int D, int H, int W, int kd, int kh,
                       int kw, int sd, int sh, int sw, int pd, int ph, int pw, void* stream);

/* ---- nn.Upsample(mode='trilinear', align_corners=True) (parts.py:149 scale 2; models.py:146 to input size) ----
 * Arbitrary (D,H,W) -> (Do,Ho,Wo); source index = dst * (in-1)/(out-1) as ATen computes it.
 * The backward is the exact adjoint in gather form (deterministic, no atomics). */
int dram_upsample_trilinear_ac_fwd(const float* x, float* y, int N, int C, int D, int H, int W,
                                   int Do, int Ho, int Wo, void* stream);
int dram_upsample_trilinear_ac_bwd(const float* dy, float* dx, int N, int C, int D, int H, int W,
                                   int Do, int Ho, int Wo, void* stream);
/* The same adjoint in two stages (reduce z with 16-byte loads, then y/x) through a workspace: any size >= 8
 * planes of D*Ho*Wo floats works (planes are processed in groups that fit); _ws_bytes returns the size for all
 * planes at once, 0 when the shape does not qualify (then, or with too small a workspace, this is _bwd). */
size_t dram_upsample_trilinear_ac_bwd_ws_bytes(int N, int C, int D, int H, int W, int Do, int Ho, int Wo);
int dram_upsample_trilinear_ac_bwd_ws(const float* dy, float* dx, void* ws, size_t ws_bytes, int N, int C,
                                      int D, int H, int W, int Do, int Ho, int Wo, void* stream);
/* Which kernels such a call launches (the same choice both entry points above go through; host arithmetic only, no HIP
 * call).  *_mis: that pointer is NOT 16-byte aligned; ws_bytes = 0: no workspace (dram_upsample_trilinear_ac_bwd).
 * Returns 0 = two-stage, trilinear_bwd_z_kernel + trilinear_bwd_yx4_kernel; 1 = two-stage, trilinear_bwd_z_kernel +
 * trilinear_bwd_kernel on the z-reduced copy; 2 = trilinear_bwd_kernel alone; 3 = trilinear_bwd_general_kernel (an axis
 * with more than 6 taps per input); negative on bad sizes.  *group: planes per workspace round of the two-stage routes
 * (a multiple of 8), 0 on the others. */
int dram_upsample_trilinear_ac_bwd_choice(int dy_mis, int dx_mis, int ws_mis, size_t ws_bytes, int N, int C, int D, int H,
                                          int W, int Do, int Ho, int Wo, int64_t* group);

/* ---- crop_concat_5d (parts.py:37-46) ----
 * out[N,C1+C2,D,H,W] = cat(t1[N,C1,D,H,W], t2[N,C2,D2,H2,W2][..., oz:oz+D, oy:oy+H, ox:ox+W]). */
int dram_crop_concat_fwd(const float* t1, const float* t2, float* out, int N, int C1, int C2,
                         int D, int H, int W, int D2, int H2, int W2, int oz, int oy, int ox, void* stream);
/* dt1 = dout[:, :C1]; dt2 = 0 outside the crop window, dout[:, C1:] inside.  Either output may be NULL. */
int dram_crop_concat_bwd(const float* dout, float* dt1, float* dt2, int N, int C1, int C2,
                         int D, int H, int W, int D2, int H2, int W2, int oz, int oy, int ox, void* stream);

/* ---- 1x1x1 convolution with bias: the regression head top_layer (models.py:109-110, 145) ---- */
int dram_conv3d_k1_fwd(const float* x, const float* w, const float* bias, float* y,
                       int N, int Cin, int Cout, int64_t S, void* stream);
size_t dram_conv3d_k1_bwd_ws_bytes(int N, int Cin, int Cout, int64_t S);
/* dx[N,Cin,S], dw[Cout,Cin], dbias[Cout]: each may be NULL and is then not computed; the others do not depend on which are
 * asked for.  dx is overwritten, whatever it held.  ws is needed (non-NULL, at least dram_conv3d_k1_bwd_ws_bytes) when dw or
 * dbias is asked for; a smaller one returns DRAM_EWS before anything is launched.  The call writes per-block partial sums to
 * the front of ws and nothing behind dram_conv3d_k1_bwd_ws_bytes; on the multi-output route (choice 4 below) they are
 * N * ceil(S / 8192) * Cout * (Cin + 1) floats and the rest of ws is not written.  dw and dbias are fp64 sums of those partials in a fixed order: the same call
 * gives the same bits. */
int dram_conv3d_k1_bwd(const float* dy, const float* x, const float* w, float* dx, float* dw, float* dbias,
                       void* ws, size_t ws_bytes, int N, int Cin, int Cout, int64_t S, void* stream);
/* Which kernel the 1x1x1 conv entry points (plain and lazy) launch: host arithmetic only, the rule the launches go through.
 * *_mis: non-zero when that tensor's base pointer is not 16-byte aligned (y / dx: the tensor written).
 *   _fwd_choice: 0 = conv1x1_fwd_kernel<false> (scalar), 1 = conv1x1_fwd_kernel<true> (float4).
 *   _bwd_choice: which = 0, backward-data (x_mis, Cin, Cout unused): 0 = conv1x1_dgrad_kernel<false>, 1 = <true>;
 *                which = 1, backward-weights (dx_mis unused): 2 = conv1x1_wgrad_kernel (scalar), 3 = conv1x1_wgrad_vec_kernel
 *                (one output channel), 4 = conv1x1_wgrad_multi_kernel.
 * Negative on bad sizes or an unknown `which`. */
int dram_conv3d_k1_fwd_choice(int x_mis, int y_mis, int64_t S);
int dram_conv3d_k1_bwd_choice(int dy_mis, int x_mis, int dx_mis, int Cin, int Cout, int64_t S, int which);

/* ---- lobe-masked mean: pooling_dense_features (models.py:37-49, default branch) ----
 * out[n,c] = sum_s x[n,c,s]*m[n,s] / sum_s m[n,s];  msum[n] = sum_s m[n,s] is also returned. */
size_t dram_masked_mean_ws_bytes(int N, int C, int64_t S);
int dram_masked_mean_fwd(const float* x, const float* mask, float* out, float* msum,
                         void* ws, size_t ws_bytes, int N, int C, int64_t S, void* stream);
/* dx[n,c,s] = dout[n,c] * m[n,s] / msum[n]. */
int dram_masked_mean_bwd(const float* dout, const float* mask, const float* msum, float* dx,
                         int N, int C, int64_t S, void* stream);

/* ---- per-lobe whole-scan inference helpers: LesionSegChunkTrain.evaluate_scan,
 *      dram/job_runner.py:729-770; thresholding of LesionSegTest.run, job_runner.py:1003-1005 ----
 * scan: int16 [D,H,W] HU, lobe: uint8 [D,H,W] label map, both resident in HBM.
 * `chunks` is a HOST array of L x {z0,y0,x0,dz,dy,dx,label} (L <= 8). */

/* boxes[(label-1)*6 + {0,1,2}] = min z,y,x; {3,4,5} = max z,y,x (inclusive); min > max if the label is absent
 * (find_crops without the border, dram/utils.py:244-254). */
int dram_label_bboxes(const uint8_t* lobe, int* boxes, int nlabels, int D, int H, int W, void* stream);

/* out[L,1,R,R,R]: crop, set voxels outside the lobe to the window minimum (-2048 HU clips to it), window
 * [wmin,wmax] -> [0,1] (data_transforms.py:37-54), resample to R^3 (trilinear, align_corners=True). */
int dram_lobe_chunks(const int16_t* scan, const uint8_t* lobe, float* out, const int* chunks, int L,
                     int D, int H, int W, int R, float wmin, float wmax, void* stream);

/* htp[v] = resize(sigmoid(dense[l]))(v) for every voxel of chunk l with lobe == label (job_runner.py:765-770). */
int dram_lobe_paste(const float* dense, const uint8_t* lobe, float* htp, const int* chunks, int L,
                    int D, int H, int W, int R, void* stream);

/* 256-bin histogram of uint8(clip(htp,0,1)*255) over voxels with lobe > 0 (input of Otsu, binary_cam
 * dram/utils.py:226-242) and the fp64 sum of htp over the same voxels.  hist: 256 x uint64, sum: 1 x double. */
int dram_lung_hist256(const float* htp, const uint8_t* lobe, unsigned long long* hist, double* sum,
                      int64_t n, void* stream);

/* mask[v] = htp[v] > th. */
int dram_threshold_mask(const float* htp, uint8_t* mask, float th, int64_t n, void* stream);

/* ---- the lobe-wise class head of LesionSegTest.run (dram/job_runner.py:985-1004; csrc/infer_cam.hip): what the reference's
 *      inference entry point runs per lobe in place of evaluate_scan's sigmoid -- pool the dense output over the resampled
 *      lobe mask (dram_masked_mean_fwd), class = arg-max, resize every channel to the crop, ReLU, take the class's channel,
 *      divide by its maximum over the crop, zero when the class is 0, paste where the lobe is.  `chunks` as above.
 * dram_lobe_chunk_masks: out[L,1,R,R,R] = 1.0 where the nearest-neighbour sample of (lobe == label) on the crop -> R^3 grid of
 *   dram_lobe_chunks is set, else 0.0; 0.0 beyond the crop's buffer (ITK's default value).  Nearest = round half up, as in
 *   dram_resample_volume.
 * dram_lobe_cam_max: dense [L,C,R,R,R], pool [L,C] (device).  cls_out[l] (int32) = argmax_c pool[l,c] by torch.max's CPU rule:
 *   the first occurrence of the maximum wins and a NaN counts as the maximum (the first NaN wins).  max_out[l] (float, zeroed
 *   here) = max over ALL dz*dy*dx voxels of the crop box, outside-lobe voxels included, of relu(resize(dense[l,cls_out[l]])),
 *   resize = trilinear with align_corners=True as in dram_lobe_paste; the order is the reference's (resize, ReLU, select, max).
 * dram_lobe_cam_paste: for every voxel of chunk l with lobe == label: htp = 0 if cls[l] == 0, else
 *   relu(resize(dense[l,cls[l]])) / max[l], the IEEE quotient: 0/0 = NaN when the whole channel is <= 0 over the box, as in the
 *   reference.  cls, max: device arrays (those of dram_lobe_cam_max; no host round trip).  Each voxel is written by the chunk
 *   whose label it carries, so boxes of different labels may overlap.
 * Only channel cls[l] of dense[l] is read.  `dense` is finite by contract: ReLU and the maximum drop a NaN (fmaxf), so a voxel
 *   that a NaN reaches is pasted as 0 and is left out of the maximum, where the reference's lobe would turn NaN as a whole. */
int dram_lobe_chunk_masks(const uint8_t* lobe, float* out, const int* chunks, int L, int D, int H, int W, int R, void* stream);
int dram_lobe_cam_max(const float* dense, const float* pool, const int* chunks, int L, int C, int R, int* cls_out,
                      float* max_out, void* stream);
int dram_lobe_cam_paste(const float* dense, const uint8_t* lobe, float* htp, const int* chunks, const int* cls, const float* max,
                        int L, int C, int D, int H, int W, int R, void* stream);

/* ---- the post-processing tail of LesionSegTest.run (dram/job_runner.py:1003-1012, 1033-1037) ----
 * w_scan = windowing(scan, from_span=(wmin, wmax), to_span=(0, 1)) (utils.py:189-198; the reference calls it with the default
 * span (-1150, 350), job_runner.py:1006), in fp64 exactly as numpy evaluates it.
 * dram_scan_hist256: 256-bin histogram of binary_cam's 8-bit view of w_scan over voxels with lobe > 0 (the input of the
 *   brightness gate's Otsu threshold, `binary_cam(w_scan[lobe > 0], 0.75)`, job_runner.py:1007).  hist: 256 x uint64.
 * dram_lesion_post: pred = htp > th (job_runner.py:1004; pred may be NULL), post = pred & (w_scan > th_scan) & ~(vessel > 0)
 *   (job_runner.py:1008-1010; vessel may be NULL = no vessel mask).
 * dram_mask_overlap: counts[4] (uint64) = {|a & b|, |a | b|, |a|, |b|} of two uint8 masks (non-zero = set): IOU =
 *   (counts[0] + s) / (counts[1] + s), Dice = (2 counts[0] + s) / (counts[2] + counts[3] + s) (utils.py:437-446). */
int dram_scan_hist256(const int16_t* scan, const uint8_t* lobe, unsigned long long* hist, int wmin, int wmax, int64_t n,
                      void* stream);
int dram_lesion_post(const float* htp, const int16_t* scan, const uint8_t* vessel, uint8_t* pred, uint8_t* post, float th,
                     int wmin, int wmax, double th_scan, int64_t n, void* stream);
int dram_mask_overlap(const uint8_t* a, const uint8_t* b, unsigned long long* counts, int64_t n, void* stream);

/* ---- utils.resample(narray, spacing, required_spacing=, new_size=, interpolator=) (dram/utils.py:414-434 -> 299-381), the way
 *      LesionSegTest.run takes its masks (nearest), the scan and the heat map (linear) back to the scan's original grid
 *      (dram/job_runner.py:1016-1032): sitk.ResampleImageFilter, identity transform, same origin / direction, default value 0,
 *      output pixel type = input pixel type.  Restated from ITK's published semantics (SimpleITK absent: parity unpinned) --
 *      output voxel o samples continuous index o * spacing_out / spacing_in; zero beyond size_in - 0.5; nearest = round half up;
 *      linear in double with the upper neighbour clamped, integer pixels by clamp + truncation.
 *      kind: 0 uint8, 1 int16, 2 float32; linear: 0 / 1; in: [Di][Hi][Wi], out: [Do][Ho][Wo]; spacing_*: 3 doubles (z, y, x),
 *      HOST pointers. ---- */
int dram_resample_volume(const void* in, void* out, int kind, int linear, int Di, int Hi, int Wi, int Do, int Ho, int Wo,
                         const double* spacing_in, const double* spacing_out, void* stream);

/* ---- nn.PReLU (act_wrapper "prelu", dram/parts.py:51-52): y = x > 0 ? x : a*x, a[nparam], nparam in {1, C};
 *      x: [N,C,S].  bwd: dx (may be NULL), da[nparam] = sum dy*x over x <= 0 (deterministic) ---- */
int dram_prelu_fwd(const float* x, const float* a, float* y, int N, int C, int nparam, int64_t S, void* stream);
size_t dram_prelu_bwd_ws_bytes(int N, int C, int64_t S);
int dram_prelu_bwd(const float* dy, const float* x, const float* a, float* dx, float* da, void* ws,
                   size_t ws_bytes, int N, int C, int nparam, int64_t S, void* stream);

/* ---- F.adaptive_max_pool3d(x, 1) (pooling_dense_features 'global_max', dram/models.py:41-42): per (n,c) row
 *      the maximum and the index of its first occurrence; bwd routes dout to that element ---- */
int dram_global_max_fwd(const float* x, float* out, int64_t* idx, int NC, int64_t S, void* stream);
int dram_global_max_bwd(const float* dout, const int64_t* idx, float* dx, int NC, int64_t S, void* stream);

/* ---- nn.Dropout (the trailing module of a conv stage, dram/parts.py:95-96), forward and backward in one entry.
 * For element i of the n contiguous floats: g = i / 4, r = philox4x32_10(counter = {g lo, g hi, offset lo, offset hi},
 * key = {seed lo, seed hi}); the element is kept iff (r[i % 4] >> 8) >= threshold24, and
 * y[i] = keep ? x[i] * scale (one fp32 rounding) : +0.  The mask is a function of (seed, offset, i) only -- not of
 * alignment, grid or tensor shape -- so the backward is the same call with dy in and dx out and no mask is stored.
 * threshold24 in [0, 1 << 24]: the kept share is exactly 1 - threshold24 / 2^24.  y may be x.  n == 0 is a no-op. */
int dram_dropout(const float* x, float* y, int64_t n, unsigned threshold24, float scale, unsigned long long seed,
                 unsigned long long offset, void* stream);

/* ---- on-device OneShot transforms (dram/data_transforms.py:1140-1239, used by the affine-consistency
 *      losses dram/metrics.py:213-310 on [N,C,D,H,W] device tensors) ----
 * Rescale3DOneShot: F.interpolate(mode='trilinear') with align_corners=False on "#image" tensors (+ its adjoint, the
 * probabilities are resized inside the loss) and mode='nearest' on "#reference" tensors.  scale_* <= 0: the default
 * in/out; > 0: the 1/scale_factor ATen uses when the caller passed scale factors. */
int dram_resize_trilinear_fwd(const float* x, float* y, int N, int C, int D, int H, int W, int Do, int Ho, int Wo,
                              float scale_z, float scale_y, float scale_x, void* stream);
int dram_resize_trilinear_bwd(const float* dy, float* dx, int N, int C, int D, int H, int W, int Do, int Ho, int Wo,
                              float scale_z, float scale_y, float scale_x, void* stream);
int dram_resize_nearest(const float* x, float* y, int N, int C, int D, int H, int W, int Do, int Ho, int Wo,
                        float scale_z, float scale_y, float scale_x, void* stream);
/* Flip3DOneShot / Rotate903DOneShot (torch.flip, torch.rot90 over spatial axes): out[o] = in[i] with
 * i[perm[k]] = flip[k] ? n-1-o[k] : o[k]; perm, flip: HOST arrays of 3 ints; (D,H,W) = input extents,
 * output extents = (in[perm[0]], in[perm[1]], in[perm[2]]).  The adjoint is the inverse signed permutation. */
int dram_spatial_permute_flip(const float* x, float* y, int N, int C, int D, int H, int W, const int* perm,
                              const int* flip, void* stream);

/* ---- IntRegRefineLoss, fused and device resident: dram/metrics.py:158-177 (interval hinge on
 *      the lobe-mean probability), 331-358 + 17-51 (pseudo label + BootBinCrossEntropy), 360-373 ----
 * dense, refined, lobes, lesions: [N,1,D,H,W] (S = D*H*W).  refined = the model's second output
 * (DC3DATGeneric); NULL or == dense for DC3D, whose outputs are one tensor.  The regression term and the
 * pseudo label use dense, the segmentation term uses refined (metrics.py:333-357, 362-364).
 * keep[N] = 0 where the CT severity score is 0 (pseudo label forced to background, metrics.py:326-327),
 * 1 otherwise; targets[N][2] = regression band (get_labels, metrics.py:122-138); weight[N] =
 * clamp(frequency, 0.2, 0.8) (metrics.py:172-174).
 * out[2] = {reg_loss, seg_loss}; state (dram_intreg_loss_state_floats(N) floats) feeds the backward. */
size_t dram_intreg_loss_ws_bytes(int N, int64_t S);
int dram_intreg_loss_state_floats(int N);
int dram_intreg_loss_fwd(const float* dense, const float* refined, const float* lobes, const float* lesions,
                         const float* keep, const float* targets, const float* weight, float smoothing,
                         float* out, float* state, void* ws, size_t ws_bytes, int N, int64_t S, void* stream);
/* d(gout[0]*reg + gout[1]*seg) / d dense -> ddense and / d refined -> drefined (NULL when refined is
 * NULL or == dense: the sum goes to ddense); gout is a DEVICE array of 2 floats. */
int dram_intreg_loss_bwd(const float* dense, const float* refined, const float* lobes, const float* lesions,
                         const float* keep, const float* targets, const float* weight, const float* state,
                         const float* gout, float smoothing, float* ddense, float* drefined, int N, int64_t S,
                         void* stream);

/* ---- IntRegLoss / IntRegAffLoss, the losses without the pseudo-label refinement: dram/metrics.py:158-177 (the same
 *      interval hinge on the lobe-mean probability) and 154-156 (compute_enc_loss: the mean over all N*S elements of
 *      -p log(p + 1e-7) + (p - 1) log(1 - p + 1e-7), p = sigmoid(dense), in fp32 and in that order); 204-210, 245-308 ----
 * dense, lobes: [N,1,D,H,W] (S = D*H*W); targets[N][2], weight[N] as for dram_intreg_loss_fwd (the lesion mask enters
 * through targets alone).  One pass reads dense and lobes once; fp64 per-block partials added in a fixed order, no atomics.
 * out[2] = {reg_loss, enc_loss}; state (dram_intreg_enc_loss_state_floats(N) floats) feeds the backward; ws: 8-byte aligned. */
size_t dram_intreg_enc_loss_ws_bytes(int N, int64_t S);
int dram_intreg_enc_loss_state_floats(int N);
int dram_intreg_enc_loss_fwd(const float* dense, const float* lobes, const float* targets, const float* weight,
                             float* out, float* state, void* ws, size_t ws_bytes, int N, int64_t S, void* stream);
/* d(gout[0]*reg + gout[1]*enc) / d dense -> ddense; gout is a DEVICE array of 2 floats. */
int dram_intreg_enc_loss_bwd(const float* dense, const float* lobes, const float* targets, const float* weight,
                             const float* state, const float* gout, float* ddense, int N, int64_t S, void* stream);

/* ---- the regression targets of a batch on the device: IntRegLoss.get_labels (dram/metrics.py:122-138), the class weight
 *      (172-174) and the pseudo-label switch (326-327), for a batch whose masks were made on the device (the transformed
 *      copy of the affine-consistency losses) ----
 * lobes, lesions: [N,1,D,H,W] (S = D*H*W); ctss: DEVICE int32[N], the CT severity scores 0..5; freq: HOST array of the six
 * class frequencies (copied into the launch); band_width: the half width of the band.
 * ratio = fp32(sum lesions*lobes) / fp32(sum lobes), one fp32 division of sums that are exact for 0/1 masks (fp64 partials
 * added in a fixed order, no atomics); the band arithmetic in fp64 on that value, rounded once to fp32.
 * targets[N][2] = the band, weight[N] = clamp(freq[ctss], 0.2, 0.8), keep[N] = ctss > 0 ? 1 : 0.  A sample with an empty
 * lobe (0/0) gets NaN targets, a score outside 0..5 NaN targets and a NaN weight; the other samples are unaffected.
 * ws: 8-byte aligned, dram_intreg_targets_ws_bytes(N, S) bytes. */
size_t dram_intreg_targets_ws_bytes(int N, int64_t S);
int dram_intreg_targets(const float* lobes, const float* lesions, const int* ctss, const float* freq, double band_width,
                        float* targets, float* weight, float* keep, void* ws, size_t ws_bytes, int N, int64_t S,
                        void* stream);

/* ---- PCM local attention on the voxel grid: dram/models.py PCM.init_graph 221-258 (the
 *      neighbour graph becomes E stencil offsets), merge_func 259-331 (dot-product and geo families), compute_cross_x
 *      365-397, forward / update_all 333-363.
 * theta, phi: [B,F,D,H,W]; offsets: HOST array of E*3 ints (dz,dy,dx), E <= 128; node i receives from
 * i + offset (in-grid offsets only).  attn: [B,E,D,H,W] = softmax over the node's edges of
 * scale * normalise(act(theta_i . phi_j)); flags: DRAM_PCM_RELU | DRAM_PCM_L2NORM;
 * scale_mode: 0 none, 1 1/sqrt(#edges of the node), 2 1/0.01. */
#define DRAM_PCM_RELU 1
#define DRAM_PCM_L2NORM 2
/* The geo variants of merge_func (models.py:287-299: scaled_dot_product_geo, scaled_dot_product_geo_relu, att_is_all) add a
 * positional-encoding term to the appearance term.  On feature planes concatenated as [appearance ; positional] the
 * activation is confined to the first F_relu planes:
 *     logit = act(sum_{f < F_relu} theta_f phi_f) + sum_{f >= F_relu} theta_f phi_f       (F_relu == F: the plain forms).
 * ds: scratch [B,E,D,H,W] (receives d loss / d raw dot products); ds2: second scratch [B,E,D,H,W], needed when F_relu < F
 * and DRAM_PCM_RELU is set (NULL otherwise); dtheta, dphi: [B,F,D,H,W]. */
int dram_pcm_attention_split_fwd(const float* theta, const float* phi, const int* offsets, int E, int flags,
                                 int scale_mode, int F_relu, float* attn, int B, int F, int D, int H, int W, void* stream);
int dram_pcm_attention_split_bwd(const float* theta, const float* phi, const float* attn, const float* dattn,
                                 const int* offsets, int E, int flags, int scale_mode, int F_relu, float* ds, float* ds2,
                                 float* dtheta, float* dphi, int B, int F, int D, int H, int W, void* stream);
/* The merge types without a softmax (models.py:300-302 cosine, 307-320 heu1 / heu2): a per-edge similarity v_e of
 * (theta_i, phi_j), normalised by its sum over the node's edges: attn_e = v_e / (eps + sum_k v_k).
 * mode 0 cosine: v = F.cosine_similarity (eps 1e-8; sum eps 0); 1 heu1: u = theta.phi / (1 + |theta - phi|_1), v = u if
 * u >= 0.03 else 0; 2 heu2: v = relu(u); sum eps 1e-7.  F <= 64.  ds: scratch [B,E,D,H,W].  (The reference forms heu1's masked
 * similarities under torch.no_grad(), models.py:311-314: its attention is a constant of the graph, and the host side does not
 * call the backward entry for mode 1; the entry itself differentiates through the unmasked pairs.) */
int dram_pcm_attention_sum_fwd(const float* theta, const float* phi, const int* offsets, int E, int mode, float* attn,
                               int B, int F, int D, int H, int W, void* stream);
int dram_pcm_attention_sum_bwd(const float* theta, const float* phi, const float* attn, const float* dattn,
                               const int* offsets, int E, int mode, float* ds, float* dtheta, float* dphi, int B, int F,
                               int D, int H, int W, void* stream);
/* out[b,c,i] = sum_e attn[b,e,i] * v[b,c,i+offset_e]   (torch.matmul(f_sm, x_g), models.py:394) */
int dram_pcm_aggregate_fwd(const float* attn, const float* v, const int* offsets, int E, float* out,
                           int B, int C, int D, int H, int W, void* stream);
int dram_pcm_aggregate_bwd(const float* attn, const float* v, const float* dout, const int* offsets, int E,
                           float* dattn, float* dv, int B, int C, int D, int H, int W, void* stream);

/* ---- fused conv -> norm -> ReLU -> conv chains (parts.py:177-187 conv -> norm -> act) ----
 *
 * "Lazy" tensors: between two convolutions the reference materialises norm(y) and relu_(norm(y)) (parts.py:19-31,
 * 49-50).  Here a conv writes its RAW output y once, its epilogue leaves the BatchNorm / GroupNorm moments of y
 * as partials, dram_norm_finalize_parts turns them into the per-row coefficients {a, b} (y_norm = a*y + b), and
 * every consumer of the activated tensor -- the next conv (forward and backward-weights), the 2x2x2 max-pool,
 * the trilinear upsample, the 1x1x1 head -- takes (y, coef, relu) and applies max(a*y + b, relu ? 0 : -inf)
 * while loading.  The activated tensor never exists in HBM; values are bit-identical to dram_row_affine_act's.
 *   coefK: [N*CK][2] floats, NULL = that source is an ordinary tensor;  reluK: apply ReLU after the affine map.
 */

/* number of statistics partials per (n, c) row that dram_conv3d_k3_fwd_fused writes for this shape (0: bad shape) */
int dram_conv3d_k3_stats_parts(int Cin, int Cout, int D, int H, int W);

/* y = conv3d(act1(x1) ++ crop(act2(x2)), w) as dram_conv3d_k3_fwd_ex, each source lazily normalised (above), and --
 * when stats != NULL -- per (row of y, part) {mean, M2, count} of the outputs into stats[N*Cout][nparts][3]
 * (nparts = dram_conv3d_k3_stats_parts; two-pass moments per 64 outputs, no E[x^2]-E[x]^2).  stats and bias
 * exclude each other (a conv followed by a norm has no bias, models.py:78). */
int dram_conv3d_k3_fwd_fused(const float* x1, int C1, const float* coef1, int relu1, const float* x2, int C2,
                             const float* coef2, int relu2, int D2, int H2, int W2, int oz, int oy, int ox,
                             const float* wt, const float* bias, float* y, float* stats, int nparts, int N,
                             int Cout, int D, int H, int W, void* stream);

/* 1 if backward-weights of this shape has the lazy-operand path (the Winograd kernel runs), else materialise x */
int dram_conv3d_k3_wgrad_lazy_ok(int N, int C1, int C2, int Cout, int D, int H, int W);

/* Backward-weights: dw[Cout,C1+C2,3,3,3] = sum over (n,z,y,x) of dy[n,co,z,y,x] * xpad[n,ci,z+dz,y+dy,x+dx], x the virtual
 * concatenation act1(x1) ++ crop(act2(x2)) of dram_conv3d_k3_fwd_fused (x2 == NULL: x1 only; coefK == NULL: a plain
 * source).  Deterministic: per-block partial slabs in `ws` (dram_conv3d_k3_wgrad_ws_bytes), summed in a fixed order. */
int dram_conv3d_k3_wgrad_fused(const float* x1, int C1, const float* coef1, int relu1, const float* x2, int C2,
                               const float* coef2, int relu2, int D2, int H2, int W2, int oz, int oy, int ox,
                               const float* dy, float* dw, void* ws, size_t ws_bytes, int N, int Cout, int D,
                               int H, int W, void* stream);

/* ---- which 3x3x3 conv kernel the library launches (the reference leaves this choice to cuDNN's heuristics behind
 * nn.Conv3d, parts.py:95..185; here it is a pure function of the shape, exposed so that benchmarks attribute time to
 * the right kernel and tests assert that the kernel they mean to verify is the one that ran) ----
 * Kernel families; the *_choice queries return one of these and write the instantiation's name as rocprofv3 prints
 * it (without namespace and argument list, e.g. "conv3d_k3_wgrad_wz_kernel<16, 2, 4, 2, true>") to name[cap]. */
#define DRAM_K3_FWD_DIRECT 0    /* conv3d_k3_fwd_kernel: direct 27-tap form (first layer, DRAM_CONV_DIRECT=1) */
#define DRAM_K3_FWD_WZ 1        /* conv3d_k3_fwd_wz_kernel: Winograd F(2,3) along z */
#define DRAM_K3_FWD_WZY 2       /* conv3d_k3_fwd_wzy_kernel: Winograd F(2x2,3x3) over (z,y) */
#define DRAM_K3_WGRAD_DIRECT 3  /* conv3d_k3_wgrad_kernel */
#define DRAM_K3_WGRAD_VEC 4     /* conv3d_k3_wgrad_vec_kernel: direct form, 16-byte staging */
#define DRAM_K3_WGRAD_WZ 5      /* conv3d_k3_wgrad_wz_kernel<.., false>: transposed F(2,3) along z, plain x operand */
#define DRAM_K3_WGRAD_WZ_LAZY 6 /* conv3d_k3_wgrad_wz_kernel<.., true>: x normalised + rectified on load */
#define DRAM_K3_WGRAD_C1 7      /* conv3d_k3_wgrad_c1_kernel: first layer (Cin = 1) */
#define DRAM_K3_FWD_C1 8        /* conv3d_k3_fwd_c1_kernel: first layer (Cin = 1), HBM-bound vector kernel */
#define DRAM_K3_WGRAD_WZY 9     /* conv3d_k3_wgrad_wzy_kernel: transposed F(2x2,3x3) over (z,y) */
#define DRAM_K3_KINDS 10

/* forward / backward-data of [N,Cin,D,H,W] -> Cout channels; the destination may be split over two tensors as in
 * dram_conv3d_k3_fwd_ex (dstC2 = 0: one tensor); fused != 0: the dram_conv3d_k3_fwd_fused variant.  The SOURCE of the
 * launch counts as well: a cropped second source tensor [., srcC2, srcD2, srcH2, srcW2] (srcC2 = 0: none) whose window
 * starts at x offset srcox, and whether a source base pointer is off 16-byte alignment.  The (z,y) kernel fetches rows as
 * aligned 16-byte pieces: such a launch runs the z-only kernel on the same 32x4x2 boxes instead (the count of statistics
 * partials, dram_conv3d_k3_stats_parts, does not depend on it). */
int dram_conv3d_k3_fwd_choice_src(int Cin, int Cout, int D, int H, int W, int dstC1, int dstC2, int dstD2, int dstH2,
                                  int dstW2, int fused, int srcC2, int srcD2, int srcH2, int srcW2, int srcox,
                                  int src_misaligned, char* name, size_t cap);
/* backward-weights with x = x1[.,C1,..] ++ crop(x2[.,C2,..]) (C2 = 0: one tensor); lazy != 0: the *_fused variant
 * with at least one lazily normalised source. */
int dram_conv3d_k3_wgrad_choice(int N, int C1, int C2, int Cout, int D, int H, int W, int lazy, char* name, size_t cap);
/* every instantiation the two queries above can name, one per line in the same spelling, into buf[cap]; returns their
 * number (DRAM_EINVAL: cap too small).  Needs no device. */
int dram_conv3d_k3_kernel_rows(char* buf, size_t cap);
/* launches per kernel family (index = DRAM_K3_*) since the library was loaded, into counts[0..n) */
int dram_conv3d_k3_launch_counts(unsigned long long* counts, int n);

/* Training-mode BatchNorm / GroupNorm statistics (parts.py:19-31) from the conv epilogue's partials: save_mean,
 * save_rstd per statistic, rowcoef[N*C][2], running statistics updated as dram_norm_fwd_train does.  Chan's
 * combine in fp64; a total count that differs from the statistic's population poisons it with NaN: save_mean, save_rstd
 * and the {a, b} of every row of the statistic. */
size_t dram_norm_parts_ws_bytes(int N, int C, int nparts);
int dram_norm_finalize_parts(const float* parts, int nparts, const float* gamma, const float* beta,
                             float* save_mean, float* save_rstd, float* rowcoef, float* running_mean,
                             float* running_var, float momentum, float eps, int kind, int G, int N, int C,
                             int64_t S, void* ws, size_t ws_bytes, void* stream);

/* this rank's per-channel {mean, M2} in fp64 (mean_m2[2c], [2c+1]: the layout of dram_bn_stats) from the same partials: what
 * nn.SyncBatchNorm (parts.py:32-33) exchanges between ranks; ws as dram_norm_parts_ws_bytes */
int dram_bn_parts_stats(const float* parts, int nparts, double* mean_m2, int N, int C, int64_t S, void* ws,
                        size_t ws_bytes, void* stream);

/* eval-mode BatchNorm: rowcoef (and save_mean / save_rstd) from the running statistics, no pass over a tensor */
int dram_bn_eval_coef(const float* gamma, const float* beta, const float* running_mean, const float* running_var,
                      float* save_mean, float* save_rstd, float* rowcoef, float eps, int N, int C, void* stream);

/* y = act(rowcoef[row][0] * x + rowcoef[row][1]): materialise a lazy tensor (rows = N*C) */
int dram_row_affine_act(const float* x, const float* rowcoef, float* y, int relu, int64_t rows, int64_t S,
                        void* stream);

/* nn.MaxPool3d(2,2,0) (parts.py:191) of a lazy tensor; and its backward ADDED onto dx (the skip branch's gradient) */
int dram_maxpool3d_2_fwd_lazy(const float* x, const float* coef, int relu, float* out, uint8_t* idx, int N, int C,
                              int D, int H, int W, void* stream);
int dram_maxpool3d_2_bwd_acc(const float* dout, const uint8_t* idx, float* dx, int N, int C, int D, int H,
                             int W, void* stream);

/* nn.Upsample(trilinear, align_corners=True) (parts.py:149) of a lazy tensor */
int dram_upsample_trilinear_ac_fwd_lazy(const float* x, const float* coef, int relu, float* y, int N, int C, int D,
                                        int H, int W, int Do, int Ho, int Wo, void* stream);

/* top_layer 1x1x1 conv (models.py:109,145) of a lazy tensor, and its backward (dx = gradient w.r.t. act(x)) */
int dram_conv3d_k1_fwd_lazy(const float* x, const float* coef, int relu, const float* w, const float* bias, float* y,
                            int N, int Cin, int Cout, int64_t S, void* stream);
int dram_conv3d_k1_bwd_lazy(const float* dy, const float* x, const float* coef, int relu, const float* w, float* dx,
                            float* dw, float* dbias, void* ws, size_t ws_bytes, int N, int Cin, int Cout, int64_t S,
                            void* stream);

/* ---- affine-consistency losses (IntRegAffRefineLoss, dram/metrics.py:376-462): the two ops they add ----
 * F.sigmoid (metrics.py:434,445) as a differentiable op: y = sigmoid(x); dx = dy * p * (1 - p) recomputed from x. */
int dram_sigmoid_fwd(const float* x, float* y, int64_t n, void* stream);
int dram_sigmoid_bwd(const float* dy, const float* x, float* dx, int64_t n, void* stream);
/* F.smooth_l1_loss(a[m > 0], b[m > 0]) (metrics.py:449,451-452: beta 1, mean) for a, b [N,C,S] and the mask m[N,1,S]
 * expanded over C.  out[0] = loss, out[1] = number of selected elements; deterministic (fp64, fixed order).
 * Backward: da (and/or db = -da) for the upstream gradient gout[0]. */
size_t dram_masked_smooth_l1_ws_bytes(int N, int C, int64_t S);
int dram_masked_smooth_l1_fwd(const float* a, const float* b, const float* mask, float* out, void* ws,
                              size_t ws_bytes, int N, int C, int64_t S, void* stream);
int dram_masked_smooth_l1_bwd(const float* a, const float* b, const float* mask, const float* out,
                              const float* gout, float* da, float* db, int N, int C, int64_t S, void* stream);

/* ---- the two voxel-wise segmentation losses with a target that is GIVEN: BootBinCrossEntropy (dram/metrics.py:10-51) and
 *      BinaryCrossEntropySmooth (metrics.py:53-72), over n contiguous elements (the reference flattens too).
 * p: float32.  t, voi: float32 (kind DRAM_SEG_MASK_F32) or uint8 (kind DRAM_SEG_MASK_U8: the kinds of dram_resample_volume),
 * each with its own kind; any base address (a base aligned for it is read 16 bytes, or four uint8, per lane and access).
 * BootBinCrossEntropy, eps = 1e-7, s = smoothing, every per-element value in fp32 and every sum in fp64:
 *   pt      = p t + (1 - p)(1 - t),      nll     = -log(clamp(pt, eps, 1 - eps))
 *   p_hat   = p > 0.5 ? p : 1 - p,       nll_hat = -log(clamp(p_hat, eps, 1 - eps))
 *   outside = {voi < 1e-7}, inside = {voi > 0}  (the two tests as written: an element with 0 < voi < 1e-7 is in both)
 *   n_out, n_in = their sizes;  T = sum_in t,  A = sum_in t nll,  B = sum_in (1 - t) nll
 *   alpha   = clamp(1 - T / n_in, 0.25, 0.75),   W = alpha T + (1 - alpha)(n_in - T)
 *   loss    = sum_out nll / n_out  +  [n_in > 0] ((1 - s)(alpha A + (1 - alpha) B) / W  +  s sum_in nll_hat / n_in)
 *   n_out = 0 gives 0 / 0 = NaN (torch's mean of an empty tensor); n_in = 0 gives the outside term alone.  That branch,
 *   which the reference takes on the host, is taken on the device: no entry point reads anything back.
 *   d loss / d p = [out] d nll / n_out + [in] ((1 - s)(alpha t + (1 - alpha)(1 - t)) d nll / W + s d nll_hat / n_in),
 *   d nll = (1 - 2 t) / pt where eps <= pt <= 1 - eps (bounds included: torch.clamp's rule) and 0 elsewhere, d nll_hat
 *   = -+ 1 / p_hat under the same rule; t_hat and alpha are constants; t and voi get no gradient.
 * BinaryCrossEntropySmooth, s = smooth, pc = clamp(p, 1e-6, 1 - 1e-6), 1 - pc formed in fp32 from the clamped pc:
 *   T = sum t,  alpha = clamp(1 - T / n, 0.3, 0.7),  w = alpha t + (1 - alpha)(1 - t),  W = alpha T + (1 - alpha)(n - T)
 *   loss = -s (alpha sum t log pc + (1 - alpha) sum (1 - t) log(1 - pc)) / W
 *   d loss / d p = -s w (t / pc - (1 - t) / (1 - pc)) / W where 1e-6 <= p <= 1 - 1e-6, and 0 elsewhere.
 * fwd: out = the loss (one device float); state = dram_seg_loss_state_floats() device floats for the backward
 *   (boot: 1 / n_out or 0, alpha, 1 / W, 1 / n_in, 1 if n_in > 0 -- the last four 0 otherwise; smooth: alpha, 1 / W);
 *   ws = dram_seg_loss_ws_bytes(n) bytes, 8-byte aligned; on return its first 8 doubles are the totals
 *   (boot: n_out, sum_out nll, n_in, T, A, B, sum_in nll_hat; smooth: T, sum t log pc, sum (1 - t) log(1 - pc)).
 *   One block per dram_seg_loss_chunk() elements writes one tuple of fp64 partials, one block adds them in a fixed order:
 *   no atomics, the bits depend on the values alone -- not on alignment, mask kind or run.
 * bwd: dp = gout[0] * d loss / d p, the multiplication by gout[0] last (one fp32 rounding).
 * Negative n, an unknown kind and (for n > 0) a null pointer are DRAM_EINVAL before anything is launched; n == 0 launches
 * nothing and leaves out, state and dp alone (the loss of no elements is NaN in the reference: the caller's to supply). */
#define DRAM_SEG_MASK_U8 0
#define DRAM_SEG_MASK_F32 2
size_t dram_seg_loss_ws_bytes(int64_t n);
int dram_seg_loss_state_floats(void);
int dram_seg_loss_chunk(void);
int dram_boot_bce_fwd(const float* p, const void* t, const void* voi, int t_kind, int voi_kind, int64_t n,
                      double smoothing, float* out, float* state, void* ws, size_t ws_bytes, void* stream);
int dram_boot_bce_bwd(const float* p, const void* t, const void* voi, int t_kind, int voi_kind, int64_t n,
                      double smoothing, const float* state, const float* gout, float* dp, void* stream);
int dram_bce_smooth_fwd(const float* p, const void* t, int t_kind, int64_t n, double smooth, float* out, float* state,
                        void* ws, size_t ws_bytes, void* stream);
int dram_bce_smooth_bwd(const float* p, const void* t, int t_kind, int64_t n, double smooth, const float* state,
                        const float* gout, float* dp, void* stream);

/* ---- SegOverlap: a per-sample Tversky (soft Dice) term and a focal term on LOGITS, for a target that is given.  No
 *      reference counterpart: this is the supervised loss that fits the data-parallel trainer's two-term contract.
 * z[N][S]: float32 logits, one channel, S = D*H*W.  t[N][S]: the target, voi[N][S]: the volume of interest, each float32
 * (DRAM_SEG_MASK_F32) or uint8 (DRAM_SEG_MASK_U8) with its own kind; "set" means non-zero.  voi may be NULL: every voxel
 * counts (voi_kind is then ignored).  Any base address, any S.
 * Parameters: a, b >= 0 the Tversky weights of false positives and false negatives (a = b = 0.5: soft Dice); s > 0 the
 * smoothing term; alpha in [0, 1] and gamma >= 0 the focal term (gamma = 0, alpha = 0.5: half the plain BCE).
 * Per voxel, never forming 1 - p by subtraction:
 *   p = sigmoid(z),   log p = -softplus(-z),   log(1 - p) = -softplus(z)
 * Per sample n, with V_n = {v : voi[n][v] set}:
 *   TP = sum_V p [t],   SP = sum_V p,   ST = sum_V [t],   M = |V_n|
 *   TI_n = (TP + s) / ((1 - a - b) TP + a SP + b ST + s)
 *   F_n  = (1 / M) sum_V -alpha_t (1 - p_t)^gamma log p_t,   t set: p_t = p, alpha_t = alpha;  t unset: p_t = 1 - p,
 *          alpha_t = 1 - alpha;   (1 - p_t)^gamma = exp(gamma log(1 - p_t))
 *   M = 0:  TI_n = 1 and F_n = 0 (the sample contributes nothing; no NaN)
 * out[0] = sum_n (1 - TI_n)      a SUM over samples (the trainer's rule for a first term)
 * out[1] = (1 / N) sum_n F_n     a MEAN over samples (its rule for every later term)
 * Every quantity is per sample, so micro-batches and ranks add up exactly: sum_k out_k[0] = out[0] and
 * sum_k (N_k / N) out_k[1] = out[1] for any split of the batch into parts k.
 * Per-voxel values are fp32 (|z| up to 100 and beyond gives finite values and gradients), every sum is fp64: one block per
 * dram_seg_loss_chunk() elements OF ONE SAMPLE writes one tuple of fp64 partials, one block adds them in a fixed order.  No
 * atomics: the bits depend on the values alone -- not on alignment, mask kind or run.
 * fwd: out[2] as above; state = dram_seg_overlap_state_floats(N) device floats for the backward, five per sample:
 *   1 - TI_n, F_n, d(1 - TI_n)/d(TP + SP) (a voxel with t set), d(1 - TI_n)/d SP (t unset), 1 / (N M) (0 where M = 0);
 *   ws = dram_seg_overlap_ws_bytes(N, S) bytes, 8-byte aligned; on return it starts with 8 doubles per sample:
 *   TP, SP, ST, M, sum_V of the focal terms, 1 - TI_n, F_n, 0.
 * bwd: dz = gout[0] d out[0]/dz + gout[1] d out[1]/dz in closed form,
 *   d out[0]/dz = p (1 - p) ([t] c_set + [not t] c_unset),   c_set = -(Den - (TP + s)(1 - b)) / Den^2,  c_unset = (TP + s) a / Den^2
 *   d out[1]/dz = -+ alpha_t (1 - p_t)^gamma (gamma p_t (-log p_t) + 1 - p_t) / (N M)      (- where t is set)
 *   each product with gout formed last (one fp32 rounding), then one addition; exactly +0 outside V_n.  t, voi: no gradient.
 * Negative N or S, N > 65535, S > 2^40, an unknown kind, a, b or gamma negative or not finite, s <= 0 or not finite, alpha
 * outside [0, 1] and (for N S > 0) a null required pointer are DRAM_EINVAL, a short workspace DRAM_EWS, all before anything
 * is launched or written; N S == 0 launches nothing and leaves out, state and dz alone.  The two size queries need no
 * device. ---- */
size_t dram_seg_overlap_ws_bytes(int N, int64_t S);
int dram_seg_overlap_state_floats(int N);
int dram_seg_overlap_fwd(const float* z, const void* t, const void* voi, int t_kind, int voi_kind, int N, int64_t S,
                         double a, double b, double smooth, double alpha, double gamma, float* out, float* state, void* ws,
                         size_t ws_bytes, void* stream);
int dram_seg_overlap_bwd(const float* z, const void* t, const void* voi, int t_kind, int voi_kind, int N, int64_t S,
                         double alpha, double gamma, const float* state, const float* gout, float* dz, void* stream);

/* Rotate3DXOneShot (data_transforms.py:1186-1208): F.grid_sample(x, F.affine_grid(theta, x.size())) with the defaults
 * (trilinear, zeros padding, align_corners=False); theta12 = HOST pointer to the row-major [3][4] matrix shared by all
 * samples.  Backward = the scatter adjoint (float atomics: summation order not fixed, like ATen's). */
int dram_affine_sample_fwd(const float* x, float* y, const float* theta12, int N, int C, int D, int H, int W,
                           void* stream);
int dram_affine_sample_bwd(const float* dy, float* dx, const float* theta12, int N, int C, int D, int H, int W,
                           void* stream);

/* ---- measured ceilings of the device ("calibrate both peaks on the box with a copy kernel and an FMA
 * loop"); no reference counterpart.  Both only launch: the caller brackets them with HIP events on `stream`.
 * dram_calibrate_hbm_copy: dst = src, 16 bytes per lane (2 x nbytes of HBM traffic).
 * dram_calibrate_mfma_f32: a register-only v_mfma_f32_32x32x2_f32 loop, `blocks` x 8 waves x iters x 32 MFMAs; *flops (may be
 *   NULL) receives the launch's FLOP count; sink: blocks * 512 floats. ---- */
int dram_calibrate_hbm_copy(const void* src, void* dst, size_t nbytes, void* stream);
int dram_calibrate_mfma_f32(float* sink, int blocks, int iters, double* flops, void* stream);

/* ---- training-time augmentation pool on a device batch: LesionSegChunkTrain.ensemble_scan_augmentation,
 *      dram/job_runner.py:548-581, over GaussianBlur / RandomMaskOut / RandomFlip / RandomRotate90 / GaussianAddictive of
 *      dram/data_transforms.py:365-406, 507-535, 756-800, 935-992 ----
 * x, y: [N, D, H, W] (S = D*H*W; permute_flip: [N, C, D, H, W]).  One launch serves the whole batch; each sample's parameters
 * come from DEVICE tables of n_table entries (n_table must equal N).  flag[N] (device ints): 1 = transform the sample,
 * 0 = pass it through unchanged (copied when y != x), < 0 = skip it (y is not written for that sample).
 *
 * dram_aug_minmax: minmax[n] = {min, max} of row n, fp32, exact and independent of the launch geometry; flag may be NULL
 *   (every row); rows whose flag is not 1 are left as they are.  Three launches, no workspace.
 * dram_aug_gaussian_blur: scipy.ndimage.gaussian_filter(x[n], sigma_n): separable z, y, x, mode 'reflect', intermediates rounded
 *   to fp32.  weights[n][DRAM_AUG_MAX_RADIUS + 1]: weights[n][j] multiplies the taps at distance j, zero beyond the sample's own
 *   radius; radius = the largest radius of the batch, 0..DRAM_AUG_MAX_RADIUS.  Not in place.
 * dram_aug_mask_out: RandomMaskOut._mask_out: `times` (1..DRAM_AUG_MAX_BOXES) boxes per sample, boxes[n][k] = {z0, z1, y0, y1,
 *   x0, x1} half-open (empty boxes allowed), each filled with fp32(min + (max - min) * u[n][k]) evaluated in fp64, min / max read
 *   from minmax[n] (dram_aug_minmax of x); later boxes overwrite earlier ones.  y may be x.
 * dram_aug_gaussian_noise: GaussianAddictive._gaussian_addictive: ((x - min) / (range + 1e-7) + noise) clamped to [0, 1],
 *   times range, plus min, every step rounded to fp32.  noise == NULL: N(0, sigma[n]) from Philox4x32-10 keyed by seeds[n] with the
 *   element index as counter, then Box-Muller (a function of seed and element only).  noise != NULL: [N][S] fp64 values added in
 *   fp64 as numpy does (sigma, seeds unused).  y may be x.
 * dram_aug_permute_flip: out[o] = in[i], i[perm[n][k]] = flip[n][k] ? n_k-1-o[k] : o[k] per sample; the permutation must keep
 *   the shape (D, H, W).  elem_size 4 (float32) or 1 (uint8).  Not in place. */
#define DRAM_AUG_MAX_RADIUS 4
#define DRAM_AUG_MAX_BOXES 16
int dram_aug_minmax(const float* x, float* minmax, const int* flag, int N, int64_t S, void* stream);
int dram_aug_gaussian_blur(const float* x, float* y, const float* weights, const int* flag, int n_table, int radius, int N, int D,
                           int H, int W, void* stream);
int dram_aug_mask_out(const float* x, float* y, const float* minmax, const int* boxes, const double* u, const int* flag,
                      int n_table, int times, int N, int D, int H, int W, void* stream);
int dram_aug_gaussian_noise(const float* x, float* y, const float* minmax, const float* sigma, const unsigned long long* seeds,
                            const int* flag, int n_table, const double* noise, int N, int64_t S, void* stream);
int dram_aug_permute_flip(const void* x, void* y, int elem_size, const int* perm, const int* flip, const int* flag, int n_table,
                          int N, int C, int D, int H, int W, void* stream);

/* Point-wise intensity transforms of dram/data_transforms.py over ROWS of L floats: x, y hold R rows back to back, a row being a
 * sample (R = N, L = D*H*W) or one z-slice of it (R = N*D, L = H*W); flag, the tables and n_table (= R) are per row.  A row need
 * not start on a 16-byte boundary.
 *
 * dram_aug_row_mean: mean[r] = fp32(sum of row r in fp64 / L), the same bits for the same row whatever R and the row's position;
 *   flag may be NULL; rows whose flag is not 1 are left as they are.  ws: dram_aug_row_mean_ws_bytes(R, L) bytes, 8-byte aligned.
 * dram_aug_intensity_map: with {min, max} = minmax[r] (dram_aug_minmax over the same rows), range = max - min and
 *   t = (x - min) / (range + 1e-7), every operation rounded to fp32 as numpy rounds it, powers by powf:
 *   DRAM_AUG_MAP_INVERSE (IntensityInverse, 213-248):  ((1 - t) - (1 - t at x = max)) * range + min; params unused
 *   DRAM_AUG_MAP_GAMMA (GammaTransform, 279-315):      t ** params[r][0] * range + min
 *   DRAM_AUG_MAP_STRETCH (ContrastStretchingTransform, 318-362): 1 / (1 + (params[r][1] / (t + 1e-7)) ** params[r][0]) * range + min
 *   DRAM_AUG_MAP_JITTER (ContrastJitter, 538-579):     (x - mean[r]) * params[r][0] + mean[r], clamped to [min, max] when keep_range
 *   DRAM_AUG_MAP_STANDARDIZE (StandarizeChannel, 873-899): (x - params[r][0]) / params[r][1], params = dram_aug_row_mean_std's
 *     output; minmax and mean unused.  (The value 4 is no mode and stays rejected.)
 *   params: [R][2] fp32 {factor, middle point}; mean: [R] fp32 (dram_aug_row_mean), jitter only; minmax may be NULL for a jitter
 *   without keep_range.  y may be x.
 * dram_aug_row_mean_std: mean_std[r] = {fp32 mean as dram_aug_row_mean, fp32 std of d = fp32(x - mean): sqrt(sum d^2 / L -
 *   (sum d / L)^2)}, fp64 sums added in a fixed order (deterministic, the same bits wherever the row stands); a constant row has
 *   std 0.  flag may be NULL; rows whose flag is not 1 are left as they are.  ws: dram_aug_row_mean_std_ws_bytes(R, L) bytes,
 *   8-byte aligned. */
#define DRAM_AUG_MAP_INVERSE 0
#define DRAM_AUG_MAP_GAMMA 1
#define DRAM_AUG_MAP_STRETCH 2
#define DRAM_AUG_MAP_JITTER 3
#define DRAM_AUG_MAP_STANDARDIZE 5
size_t dram_aug_row_mean_ws_bytes(int R, int64_t L);
int dram_aug_row_mean(const float* x, float* mean, const int* flag, int R, int64_t L, void* ws, size_t ws_bytes, void* stream);
size_t dram_aug_row_mean_std_ws_bytes(int R, int64_t L);
int dram_aug_row_mean_std(const float* x, float* mean_std, const int* flag, int R, int64_t L, void* ws, size_t ws_bytes,
                          void* stream);
int dram_aug_intensity_map(const float* x, float* y, int mode, const float* minmax, const float* mean, const float* params,
                           int keep_range, const int* flag, int n_table, int R, int64_t L, void* stream);

/* Slab projections, region masks (dram/data_transforms.py:409-504, 639-678, 840-870); tables and flags as for the pool above.
 *
 * dram_aug_slab_project: MinimalIntensityProjection / MaximumIntensityProjection / MinimalIntensityAxialProjection `maip`: with
 *   t = thickness[n] (0..DRAM_AUG_MAX_SLAB) and a = axis[n] (0 = z, 1 = y, 2 = x), y[.., i, ..] = min (is_max == 0) or max of
 *   x[.., max(0, i - t) .. i, ..] along axis a: a causal window of t + 1 elements, clipped at the start of the axis; t = 0 copies.
 *   x, y: [N, D, H, W] fp32.  Min and max are exact, so finite inputs give numpy's bits; which operand a NaN in the window yields
 *   is unspecified (numpy propagates it, fminf / fmaxf drop it).  Not in place.
 * dram_aug_keep_region: DiskMaskOut / RandomCubeMask._mask: y = x where the voxel (z, y, x) lies in the half-open box boxes[n] =
 *   {z0, z1, y0, y1, x0, x1} and, when disk[n] = {cy, cx, r2} has r2 >= 0, also (y - cy)^2 + (x - cx)^2 <= r2; 0 elsewhere (an
 *   empty box zeroes the sample).  x, y: [N, C, D, H, W], elem_size 4 (float32) or 1 (uint8).  y may be x. */
#define DRAM_AUG_MAX_SLAB 16
int dram_aug_slab_project(const float* x, float* y, const int* thickness, const int* axis, int is_max, const int* flag,
                          int n_table, int N, int D, int H, int W, void* stream);
int dram_aug_keep_region(const void* x, void* y, int elem_size, const int* boxes, const int* disk, const int* flag, int n_table,
                         int N, int C, int D, int H, int W, void* stream);

/* RandomCrop(keep_size=True) (dram/data_transforms.py:582-636): np.pad where the drawn window leaves the chunk, the window sliced
 * out, then Resample('fixed_size', 1, data_shape) back to the chunk's size on the ITK grid of dram_chunk_prepare.  x, y:
 * [N, D, H, W], elem_size 4 (float32) or 1 (uint8); W <= 2048, D <= 65535, D*H*W < 2^29.
 *
 * dram_aug_pad_min: what np.pad(mode='minimum') puts outside the chunk: the sample's minimum over every non-empty subset of its
 *   axes, the other coordinates held fixed (np.pad pads axis by axis with the minimum along that axis of the array as padded so
 *   far).  Per sample, in elements: Pz [H][W], Py [D][W], Px [D][H], Pzy [W], Pzx [H], Pyx [D], Pzyx [1], rounded up to a multiple
 *   of four.  Only samples whose flag is 1 are read and written.  Exact in any order; which operand a NaN yields is unspecified.
 *   ws: dram_aug_pad_min_ws_bytes(N, D, H, W, elem_size) bytes, 16-byte aligned; H, W <= 2048.  Three launches.
 * dram_aug_crop_resample: table: N records of 56 bytes on the DEVICE, {int z0, y0, x0: the window's first voxel in chunk
 *   coordinates, negative where it starts in the pad; int cd, ch, cw: the crop's actual size; int mode (DRAM_AUG_PAD_*); int pad;
 *   double sz, sy, sx: required_spacing / spacing, the output-to-crop index step}.  Output voxel o reads crop index c = o * step
 *   per axis; 0 where c >= size - 0.5; linear != 0: fp64 lerps along x, y, z with the upper neighbour clamped to the crop, cast
 *   to fp32 (float32 only); otherwise the voxel at (int)(c + 0.5).  A crop voxel outside the chunk is 0 (CONSTANT), the chunk's
 *   voxel at the clamped coordinate (EDGE) or pad_ws's projection (MINIMUM; pad_ws = dram_aug_pad_min of x).  flag as above: 0
 *   copies the sample.  Not in place.
 *   THE CALLER'S RESPONSIBILITY: the modes live in the device table, which the host side of this entry cannot read, so it
 *   cannot tell whether a workspace is needed.  pad_ws may be NULL only when no MINIMUM sample's window leaves the chunk; a
 *   MINIMUM sample that does pad without a workspace gets 0 there (wrong values, no error), and a workspace must have been
 *   filled by dram_aug_pad_min for every such sample (flag 1 there) of this very x. */
#define DRAM_AUG_PAD_CONSTANT 0
#define DRAM_AUG_PAD_EDGE 1
#define DRAM_AUG_PAD_MINIMUM 2
size_t dram_aug_pad_min_ws_bytes(int N, int D, int H, int W, int elem_size);
int dram_aug_pad_min(const void* x, int elem_size, const int* flag, int N, int D, int H, int W, void* ws, size_t ws_bytes,
                     void* stream);
int dram_aug_crop_resample(const void* x, void* y, int elem_size, int linear, const void* table, const void* pad_ws,
                           size_t pad_ws_bytes, const int* flag, int n_table, int N, int D, int H, int W, void* stream);

/* RandomAffineTransform3D and RandomRotate (dram/data_transforms.py:995-1102): scipy.ndimage.affine_transform / rotate with
 * mode="constant", order 3 (float32) or order 0 (float32 or uint8), cval = the sample's own minimum.  x, y: [N, D, H, W];
 * D*H*W < 2^29.  Per-sample flags as above.
 *
 * dram_aug_minmax_u8: dram_aug_minmax for uint8 samples; minmax[n] = {min, max} as fp32 (exact).
 * dram_aug_spline_prefilter: the fp64 cubic B-spline coefficients of every sample whose flag is 1 into ws [N][D][H][W] doubles
 *   (dram_aug_spline_ws_bytes(N, D, H, W) bytes, 8-byte aligned): per axis in turn, z first, the mirror-boundary filter with
 *   the pole sqrt(3) - 2 along every line of more than one element.  axes[n]: bit 0 = filter along z, bit 1 = y, bit 2 = x (7 for
 *   an affine transform, the two plane axes for a rotation, which scipy runs plane by plane).  Up to three launches.
 * dram_aug_spline_resample: table: N records of 104 bytes on the DEVICE, {double m[9]: row-major 3 x 3; double off[3]; int fixed:
 *   -1 for a 3-d transform, or the axis (0 = z, 1 = y, 2 = x) that a plane transform leaves alone, whose row of m is the unit
 *   row and whose off is 0; int pad}.  Output voxel idx reads source coordinate x_h = off[h] + sum_l m[h][l] * idx[l] (fp64, added
 *   left to right, products rounded on their own).  Any x_h outside [0, n_h - 1]: minmax[n][0] (dram_aug_minmax or
 *   dram_aug_minmax_u8 of x).  order 3 (float32 only): the taps floor(x) - 1 .. floor(x) + 2 per axis (one tap on the fixed
 *   axis) of ws = dram_aug_spline_prefilter of this x, indices mirrored with period 2n - 2, cubic B-spline weights, added in
 *   fp64 with z slowest, cast to fp32.  order 0: the voxel of x at floor(x_h + 0.5); ws may be NULL.  Not in place. */
int dram_aug_minmax_u8(const unsigned char* x, float* minmax, const int* flag, int N, int64_t S, void* stream);
size_t dram_aug_spline_ws_bytes(int N, int D, int H, int W);
int dram_aug_spline_prefilter(const float* x, const int* axes, const int* flag, int n_table, int N, int D, int H, int W, void* ws,
                              size_t ws_bytes, void* stream);
int dram_aug_spline_resample(const void* x, void* y, int elem_size, int order, const void* table, const float* minmax,
                             const void* ws, size_t ws_bytes, const int* flag, int n_table, int N, int D, int H, int W,
                             void* stream);

/* ---- device chunk loader: what the reference does per chunk on the host before a training step, for a whole ragged batch.
 *      RadboudCOVIDLobeVesselChunk.get_data (dram/dataset.py:450-486): w_scan = windowing(scan, to_span=(0, 1)) (utils.py:189-198,
 *      default span (-1150, 350)); _, th = binary_cam(w_scan[lobe > 0], 0.75) (utils.py:226-242); pseudo lesion = (w_scan > th) &
 *      (lobe > 0); vessel = (vessel > 0) & (lobe > 0).  LesionSegChunkTrain.preprocessing (dram/job_runner.py:586-597):
 *      Windowing(min, max) of the image as float32 (data_transforms.py:37-54), then Resample (data_transforms.py:65-211): linear
 *      for the image, nearest neighbour for every "...reference" key, on the grid of sitk.ResampleImageFilter as
 *      dram_resample_volume restates it (SimpleITK absent: parity unpinned).
 *      The N chunks lie back to back in one DEVICE buffer per kind (scans int16, lobes uint8, vessels uint8; bases 16-byte
 *      aligned), every chunk with its own size.  table: N records of 48 bytes on the DEVICE, {int64 offset in elements; int Di,
 *      Hi, Wi; int pad; double sz, sy, sx}, s* = required_spacing / spacing per axis (the output-to-input index step).  No entry
 *      point reads per-sample data from the host, synchronises or allocates.
 * dram_chunk_hist256: hist[n][256] (uint64, zeroed here) of binary_cam's 8-bit view of windowing(scan_n, (wmin, wmax), (0, 1))
 *   over voxels with lobe_n > 0: the fp64 arithmetic of dram_scan_hist256, one launch for the batch, integer atomics.
 * dram_otsu256: th[n] = binary_cam's threshold of hist[n] (th / 255, the value dram_amd.inference.binary_cam_threshold returns,
 *   bit for bit): Otsu over the occupied bin range with fp64 running sums in bin order, first maximum, min(t * scaler, 255) /
 *   255; fewer than two occupied bins: bin / 255.  An all-zero histogram (empty lobe; the reference raises IndexError there):
 *   th = +inf, so that the sample gets no candidates.
 * dram_chunk_prepare: outputs [N][Do][Ho][Wo] float32.  image = Windowing(wmin, wmax) in fp32 exactly as numpy evaluates it on a
 *   float32 array, resampled linearly (lerps x, y, z in double, cast to fp32; 0 beyond size_in - 0.5).  lobe_out = the lobe
 *   value at the nearest voxel.  lesion_out (may be NULL; needs th) = (w_scan > th[n]) & (lobe > 0) at the nearest voxel, w_scan
 *   in fp64 from (pwmin, pwmax) as dram_lesion_post evaluates it; never materialised at source resolution.  vessel_out (may be
 *   NULL; needs vessels) = (vessel > 0) & (lobe > 0) at the nearest voxel.  wmin / wmax are fp32 values.  Wo <= 2048. ---- */
int dram_chunk_hist256(const int16_t* scans, const uint8_t* lobes, const void* table, int N, unsigned long long* hist, int wmin,
                       int wmax, void* stream);
int dram_otsu256(const unsigned long long* hist, int N, double scaler, double* th, void* stream);
int dram_chunk_prepare(const int16_t* scans, const uint8_t* lobes, const uint8_t* vessels, const void* table, const double* th,
                       int N, int Do, int Ho, int Wo, float wmin, float wmax, int pwmin, int pwmax, float* image,
                       float* lobe_out, float* lesion_out, float* vessel_out, void* stream);

/* ---- lesion-wise report at inference: what a consumer of the final lesion mask otherwise does on the host with
 *      scipy.ndimage.label / find_objects, and the CT severity score of IntRegLoss.ctss_ratio_map (dram/metrics.py:76-83) per
 *      lobe.  Volumes are contiguous [D,H,W] on the DEVICE, D*H*W < 2^31; masks and lobes uint8 (non-zero = set), labels int32.
 *      Null pointers, non-positive sizes and D*H*W >= 2^31 are DRAM_EINVAL before anything is launched.  None of the entries
 *      synchronises, allocates or reads device memory from the host.
 * dram_cc_label: labels = 0 on the background, 1..n on the components of `mask` under `connectivity` 1, 2 or 3 (6, 18 or 26
 *   neighbours, scipy.ndimage.generate_binary_structure(3, connectivity)), numbered by the raster order of their first voxel
 *   (scipy.ndimage.label's numbering); *count (device int32) = n.  Union-find on the linear index: six launches whatever the
 *   data, integer min-atomics, the result does not depend on their order (the same bits every run).  ws: dram_cc_ws_bytes(D, H,
 *   W) bytes, 4-byte aligned (too small: DRAM_EWS); dram_cc_ws_bytes answers without a GPU, 0 for sizes that dram_cc_label
 *   refuses.  labels doubles as the parent array while the call runs.
 * dram_cc_stats: for k in 1..n (n >= 1): voxels[k-1] = the number of voxels with labels == k, bbox[(k-1)*6 ..] = {z0, z1, y0, y1,
 *   x0, x1} half-open (the slices of scipy.ndimage.find_objects; {D, 0, H, 0, W, 0} for a k without voxels), hits[k-1] = how many
 *   of them have other != 0.  other and hits are NULL together.  The outputs are initialised here.  A voxel whose label lies
 *   outside 0..n is the caller's error: it is skipped.
 * dram_cc_relabel: out_labels[i] = lut[labels[i]], lut: n + 1 device int32 with lut[0] = 0 (a label outside 0..n maps to 0);
 *   out_mask[i] = out_labels[i] != 0.  Either output may be NULL; out_labels may be labels.  1 <= nvox < 2^31, n >= 0.
 * dram_lobe_burden: counts[v*2 + 0] = voxels with lobe == v, counts[v*2 + 1] = those of them with mask != 0, v in 0..255 (512
 *   int64, zeroed here).  16-byte loads where mask and lobe are 16-byte aligned, any alignment works.  1 <= nvox < 2^31. ---- */
size_t dram_cc_ws_bytes(int D, int H, int W);
int dram_cc_label(const uint8_t* mask, int32_t* labels, int32_t* count, int connectivity, int D, int H, int W, void* ws,
                  size_t ws_bytes, void* stream);
int dram_cc_stats(const int32_t* labels, const uint8_t* other, int n, int64_t* voxels, int32_t* bbox, int64_t* hits, int D, int H,
                  int W, void* stream);
int dram_cc_relabel(const int32_t* labels, const int32_t* lut, int n, int32_t* out_labels, uint8_t* out_mask, int64_t nvox,
                    void* stream);
int dram_lobe_burden(const uint8_t* mask, const uint8_t* lobe, int64_t* counts, int64_t nvox, void* stream);

/* ---- lesion density report at inference (csrc/density.hip): the Hounsfield statistics of a lesion or a lobe, what a consumer
 *      otherwise does on the host with scipy.ndimage.sum_labels / minimum / maximum / histogram over the whole scan.  Volumes
 *      are contiguous on the DEVICE, 1 <= nvox < 2^31; the scan int16, masks uint8 (non-zero = set), labels uint8 or int32.
 *      Null pointers and refused sizes are DRAM_EINVAL before anything is launched.  None of the entries synchronises, allocates
 *      or reads device memory from the host; every output is initialised by the entry.  Everything is integers, accumulated by
 *      integer atomics and integer reductions: no result depends on their order (the same bits every run).
 * dram_label_density: voxel v contributes to label k = labels[v] iff 1 <= k <= n and (mask == NULL or mask[v] != 0); a label
 *   outside 0..n is skipped.  labels: uint8 (label_kind 0, n <= 255) or int32 (label_kind 1).  Per label (n each):
 *   count[k-1], sum[k-1] = sum of scan, sumsq[k-1] = sum of scan^2 (exact int64: at most 2^30 * 2^31), vmin[k-1], vmax[k-1];
 *   a label without voxels gets {0, 0, 0, 32767, -32768}.  hist (n rows of nbins + 2 int64, NULL iff nbins == 0): row k-1, entry 0
 *   counts scan < lo, entry 1 + (scan - lo) / width counts lo <= scan < lo + nbins * width, entry nbins + 1 the rest (the
 *   below-range test comes first: no negative dividend is divided).  Refused: n < 1; label_kind 0 with n > 255; nbins outside
 *   0..4096; width < 1 with nbins > 0; n * (nbins + 2) >= 2^31; lo + nbins * width above int32; hist and nbins not NULL / 0
 *   together; a scan or int32 labels off their natural alignment.  16-byte loads where scan, labels and mask are 16-byte aligned,
 *   any alignment and any nvox work.
 * dram_label_density_plan: which of the entry's two kernels a call takes, a function of these three arguments alone, answered
 *   without a GPU: 0 = the table of the call (n * (7 + nbins + 2) words, n * 7 without a histogram) fits in LDS and is kept per
 *   block; 1 = runs of equal labels are reduced within a wave and sent to global memory.  Negative (DRAM_EINVAL) for arguments
 *   that dram_label_density refuses.
 * dram_hist_summary: per row k of such a histogram (total c = the sum of the row, below 2^52):
 *   pct[k*nq + i]: rank = max(1, (q[i] * c + 999) / 1000) in int64 (nearest rank, q per mille in 0..1000); the lower edge
 *     lo + (b-1) * width of the first in-range bin b at which the running count reaches rank; INT32_MIN if it is reached in the
 *     underflow entry, INT32_MAX if only in the overflow entry, INT32_MAX for c == 0.  With width 1: the exact percentile.
 *   bands[k*(ne+1) + i]: the count of values in [edges[i-1], edges[i]), band 0 from the underflow entry on and band ne up to and
 *     including the overflow entry; the bands of a row sum to c.  Every edge is lo + j * width for some 0 <= j <= nbins, strictly
 *     ascending, else DRAM_EINVAL.  q_permille (nq <= 16) and edges (ne <= 15) are HOST arrays and travel in the kernel arguments;
 *     nq and ne may be 0 with pct / bands NULL (bands given with ne == 0: the row totals).  One block per row, one launch. ---- */
int dram_label_density_plan(int label_kind, int n, int nbins);
int dram_label_density(const int16_t* scan, const void* labels, int label_kind, const uint8_t* mask, int n, int64_t* count,
                       int64_t* sum, int64_t* sumsq, int32_t* vmin, int32_t* vmax, int64_t* hist, int lo, int width, int nbins,
                       int64_t nvox, void* stream);
int dram_hist_summary(const int64_t* hist, int n, int lo, int width, int nbins, const int32_t* q_permille, int nq,
                      const int32_t* edges, int ne, int32_t* pct, int64_t* bands, void* stream);

/* ---- lesion distribution report at inference (csrc/distribution.hip): where in the lung the lesions lie -- per label of a label
 *      volume the reduction of a depth map (the distance of every voxel from the lung surface, dram_edt of the non-lung voxels)
 *      and of the voxel positions, what a consumer otherwise does on the host with scipy.ndimage.sum_labels / minimum /
 *      center_of_mass over a distance transform.  Volumes are contiguous [D,H,W] on the DEVICE, D * H * W < 2^31; depth fp32,
 *      labels uint8 (label_kind 0, n <= 255) or int32 (label_kind 1), mask uint8 or NULL.  Null pointers and refused sizes are
 *      DRAM_EINVAL before anything is launched.  The entry does not synchronise, allocate or read device memory from the host;
 *      every output is initialised by the entry.  Everything is integers, accumulated by integer atomics and integer
 *      reductions: no result depends on their order (the same bits every run).
 * dram_label_depth: voxel v = (z*H + y)*W + x with depth d = depth[v] contributes to label k = labels[v] iff
 *     1 <= k <= n (a label outside 0..n is skipped),  mask == NULL or mask[v] != 0,  and  d >= 0.0f
 *   (NaN and negative depths are skipped entirely; -0.0f and +inf pass).  Per label, over its contributing voxels:
 *   count[k-1]   their number.
 *   qsum[k-1]    the sum of q = (uint32)(fminf(d, 2097152.0f) * 1024.0f): the depth in 1/1024 mm, the fp32 product exact and then
 *                truncated; q <= 2^31, so the sums stay below 2^62.
 *   dmin[k-1], dmax[k-1]  the minimum and the maximum of the bit pattern of d taken as an unsigned integer, which orders
 *                depths as their values do for every d >= +0.0f (-0.0f counts with its own pattern 0x80000000, above +inf).
 *                A label without contributing voxels gets {count, qsum, dmin, dmax} = {0, 0, 0x7f800000, 0}.
 *   possum[(k-1)*3 + a]  the sums of the voxel indices z, y, x (a = 0, 1, 2).
 *   hist (n rows of nbins + 2 int64; NULL iff nbins == 0): the row layout that dram_hist_summary takes with lo = 0, width = 1.
 *                Entry 0 is always 0.  With b = d * bins_per_mm in fp32 (bins_per_mm one of 1, 2, 4, 8, 16: the product is
 *                exact) the voxel counts in entry nbins + 1 if b >= (float)nbins -- the comparison comes before the conversion,
 *                so +inf lands there -- else in entry 1 + (int)b.  nbins in 0..4096.
 *   zones (n rows of nz*ny*nx int64): the positional zone of index i along an axis with the pair [a0, a1) of the HOST array
 *                box = {z0, z1, y0, y1, x0, x1} and nzones_axis zones is
 *                    ((clamp(i, a0, a1 - 1) - a0) * nzones_axis) / (a1 - a0)        (integer division),
 *                the zone of a voxel (zz*ny + zy)*nx + zx, and the voxel counts in that entry of its label's row.  Index 0 is
 *                the low-index end of an axis.  nz, ny, nx each in 1..8.  zones is NULL iff nz*ny*nx == 1 and box == NULL; zones
 *                given without a box takes the whole volume {0, D, 0, H, 0, W} as the box.
 *   Refused: n < 1; label_kind other than 0, 1, or 0 with n > 255; nbins outside 0..4096; bins_per_mm not one of the five when
 *   nbins > 0; hist and nbins not NULL / 0 together; nz, ny or nx outside 1..8; zones and box not together as above; a0 >= a1 on
 *   an axis; n * (nbins + 2), n * nz*ny*nx or n * 3 at or above 2^31; D, H or W < 1 or D * H * W >= 2^31; depth or int32 labels
 *   off their natural alignment.  16-byte loads where depth, labels and mask are 16-byte aligned; any alignment and any size
 *   work.
 * dram_label_depth_plan: which of the entry's two kernels a call takes, a function of these four arguments alone (nzones = the
 *   entries of a zones row, nz*ny*nx, or 0 for zones == NULL; 0..512), answered without a GPU: 0 = the table of the call
 *   (n * (11 + nbins + 2 + nzones) 32-bit words, without the nbins + 2 when nbins == 0) fits in LDS, is kept per block and
 *   flushed once; 1 = runs of equal labels are reduced within a wave and sent to global memory with integer atomics.  Negative
 *   (DRAM_EINVAL) for arguments that dram_label_depth refuses. ---- */
int dram_label_depth_plan(int label_kind, int n, int nbins, int nzones);
int dram_label_depth(const float* depth, const void* labels, int label_kind, const uint8_t* mask, int n, int64_t* count,
                     int64_t* qsum, uint32_t* dmin, uint32_t* dmax, int64_t* possum, int64_t* hist, int bins_per_mm, int nbins,
                     int64_t* zones, const int32_t* box, int nz, int ny, int nx, int D, int H, int W, void* stream);

/* ---- lesion shape report at inference (csrc/shape.hip; host arithmetic in dram_amd/shape.py): per label k = 1..n of a label
 *      volume the histogram of its 2x2x2 neighbourhood configurations and the moments of its voxel positions up to second order,
 *      from which surface area, Euler number, sphericity and principal axes are host arithmetic -- what a consumer otherwise
 *      does on the host with a regionprops-style pass.  labels is a contiguous [D,H,W] volume on the DEVICE, uint8 (label_kind 0,
 *      n <= 255) or int32 (label_kind 1); a voxel with a label outside 0..n belongs to nobody.  Null pointers and refused sizes
 *      are DRAM_EINVAL before anything is launched.  The entry does not synchronise, allocate or read device memory from the
 *      host; both outputs are initialised by the entry.  Everything is integers, accumulated by integer atomics: no result
 *      depends on their order (the same bits every run).
 * dram_label_shape:
 *   cfg (n rows of 256 int64): cells lie over the zero-padded volume, cell (z, y, x) for z in -1..D-1, y in -1..H-1, x in
 *                -1..W-1, (D+1)(H+1)(W+1) of them; a cell covers the eight voxels (z+dz, y+dy, x+dx), dz, dy, dx in {0, 1}.  Bit
 *                dz*4 + dy*2 + dx of the cell's configuration c for label k is set iff that voxel lies inside the volume and
 *                carries k.  cfg[(k-1)*256 + c] counts the cells whose configuration for k is c, c in 1..255; entry 0 is always
 *                0.  A cell whose corners carry several labels counts once in the row of each, with that label's
 *                configuration.  Entry 255 is not counted cell by cell: it is solved from
 *                sum_c popcount(c) * cfg[c] = 8 * count, which holds because every voxel lies in eight cells.
 *   mom (n rows of 10 int64): {count, sum z, sum y, sum x, sum z^2, sum y^2, sum x^2, sum zy, sum zx, sum yx} over the label's
 *                voxels, in voxel indices.  A label without voxels gets zeros in both tables.
 *   Refused: n < 1; label_kind other than 0, 1, or 0 with n > 255; D, H or W < 1 or > 32768 (every sum then stays below 2^62);
 *   D * H * W >= 2^31; n * 256 >= 2^31; int32 labels off their natural alignment.  16-byte loads for every piece of a row that
 *   is 16-byte aligned and wholly inside the row; any alignment and any size work.
 * dram_label_shape_plan: which of the entry's two kernels a call takes, a function of these two arguments alone, answered
 *   without a GPU: 0 = the table of the call (n <= 24: n * 276 32-bit words) fits in LDS beside the staged rows, is kept per
 *   block and flushed once; 1 = contributions are reduced within a wave over runs of equal (label, configuration) and of equal
 *   labels and sent to global memory with integer atomics.  Negative (DRAM_EINVAL) for arguments that dram_label_shape
 *   refuses. ---- */
int dram_label_shape_plan(int label_kind, int n);
int dram_label_shape(const void* labels, int label_kind, int n, int64_t* cfg, int64_t* mom, int D, int H, int W, void* stream);

/* ---- lesion texture report at inference (csrc/texture.hip; host arithmetic in dram_amd/texture.py): per label k = 1..n of a
 *      label volume and per direction of the half 26-neighbourhood the grey-level co-occurrence table (GLCM) of the scan, from
 *      which Haralick's second-order statistics (angular second moment, entropy, contrast, correlation, ...) are host
 *      arithmetic -- what a consumer otherwise does on the host with 13 shifted copies of the scan and a scatter-add per label.
 *      scan (int16) and labels are contiguous [D,H,W] volumes on the DEVICE, labels uint8 (label_kind 0, n <= 255) or int32
 *      (label_kind 1), mask uint8 or NULL; a voxel with a label outside 1..n, or with mask == 0, belongs to nobody.  Null
 *      pointers and refused sizes are DRAM_EINVAL before anything is launched.  The entry does not synchronise, allocate or
 *      read device memory from the host; the output is initialised by the entry.  Everything is integers, accumulated by
 *      integer atomics: no result depends on their order (the same bits every run).
 * dram_label_glcm:
 *   grey level   a voxel of value v has level g = min(max((v - lo) / width, 0), levels - 1) in integer arithmetic: values below
 *                lo fall in level 0, values at or above lo + levels * width in level levels - 1.
 *   directions   the 13 offsets (dz, dy, dx) of the half 26-neighbourhood in lexicographic order, the first non-zero component
 *                positive: 0 (0,0,1)  1 (0,1,-1)  2 (0,1,0)  3 (0,1,1)  4 (1,-1,-1)  5 (1,-1,0)  6 (1,-1,1)  7 (1,0,-1)  8 (1,0,0)
 *                9 (1,0,1)  10 (1,1,-1)  11 (1,1,0)  12 (1,1,1); each is multiplied by `distance`.  They are VOXEL offsets: under
 *                anisotropic spacing the directions have different physical lengths.
 *   glcm (n x 13 x levels x levels int64): entry [(k-1), dir, g(p), g(q)] counts the ordered pairs (p, q = p + distance *
 *                offset[dir]) of voxels that both lie inside the volume, both carry label k and both pass the mask.  The table
 *                is not symmetrised: the host adds the transpose.  A label without pairs gets zeros.
 *   Refused: n < 1; label_kind other than 0, 1, or 0 with n > 255; levels outside 2..32; distance outside 1..4; width < 1; D, H
 *   or W < 1 or > 32768; D * H * W >= 2^31; n * 13 * levels^2 >= 2^31; int32 labels or the int16 scan off their natural
 *   alignment.  16-byte loads of the scan and of int32 labels (8-byte loads of uint8 labels and of the mask) for every piece of
 *   eight voxels of a row that is so aligned and wholly inside the row; any alignment and any size work.
 * dram_label_glcm_plan: which of the entry's two kernels a call takes, a function of these four arguments alone, answered
 *   without a GPU: 0 = the table of the call (n * 13 * levels^2 <= 24576 32-bit words) fits in LDS beside the staged planes,
 *   is kept per block and flushed once; 1 = runs of equal (label, direction, g(p), g(q)) are reduced within a wave and sent to
 *   global memory with integer atomics.  Negative (DRAM_EINVAL) for arguments that dram_label_glcm refuses. ---- */
int dram_label_glcm_plan(int label_kind, int n, int levels, int distance);
int dram_label_glcm(const int16_t* scan, const void* labels, int label_kind, const uint8_t* mask, int n, int lo, int width,
                    int levels, int distance, int64_t* glcm, int D, int H, int W, void* stream);

/* ---- heat-map evaluation curves at inference (csrc/curves.hip): the joint histogram of score bin x class x region of a
 *      probability map against a reference mask, from which ROC, precision / recall, the Dice sweep and a calibration table are
 *      exact host arithmetic (dram_amd/curves.py) -- what a consumer otherwise does with sklearn on every lung voxel.  Volumes are
 *      contiguous on the DEVICE, 1 <= nvox < 2^31; score fp32, ref / region / gate uint8.  Null score, ref or hist and refused
 *      sizes are DRAM_EINVAL before anything is launched.  Neither entry synchronises, allocates or reads device memory from the
 *      host; every output is initialised by the entry.  Everything is integers, accumulated by integer atomics and integer
 *      reductions: the same bits every run.
 * dram_score_hist: voxel v goes to region r = region[v] iff 1 <= r <= nregions (label 0 and labels above nregions are skipped;
 *   region == NULL requires nregions == 1 and puts every voxel in region 1), class c = (ref[v] != 0), and with s = score[v] bin
 *     0                         if gate != NULL && gate[v] == 0, or if !(s >= 0.0f) (NaN and negative scores; -0.0f passes),
 *     nbins                     if s >= 1.0f (+inf too),
 *     1 + (int)(s * nbins)      otherwise (nbins is a power of two: the fp32 product is exact, so this is 1 + floor(s * nbins)).
 *   hist: int64 [nregions][2][nbins + 1], the counts.  conf (may be NULL): the same shape; entry b >= 1 is the sum over the
 *   voxels of bin b of q = (uint32)(fminf(s, 1.0f) * 16777216.0f) (exact product, truncated, q <= 2^24, sums below 2^55); entry
 *   0 of every row is 0.  gate may be NULL (every voxel on).  Refused: nregions outside 1..255; nbins not a power of two in
 *   2..4096; region == NULL with nregions != 1; a score off its natural alignment.  16-byte loads where score, ref, region and
 *   gate are 16-byte aligned, any alignment and any nvox work.
 * dram_score_hist_plan: which of the entry's two paths a call takes, a function of these three arguments alone, answered
 *   without a GPU: 0 = the table (nregions * 2 * (nbins + 1) words, three times that with conf) fits in 128 KiB of LDS and is
 *   kept per block; 1 = it does not, and the aggregated updates go to global memory.  Negative (DRAM_EINVAL) for the nregions
 *   and nbins that dram_score_hist refuses. ---- */
int dram_score_hist_plan(int nregions, int nbins, int with_conf);
int dram_score_hist(const float* score, const uint8_t* ref, const uint8_t* region, const uint8_t* gate, int nregions, int nbins,
                    int64_t* hist, int64_t* conf, int64_t nvox, void* stream);

/* ---- surface-distance metrics at inference (Hausdorff, its percentiles, average symmetric surface distance, surface Dice):
 *      what a consumer otherwise does on the host with scipy.ndimage.distance_transform_edt and binary_erosion.  Volumes are
 *      contiguous [D,H,W] on the DEVICE, D*H*W < 2^31; masks uint8 (non-zero = set).  Null pointers and refused sizes are
 *      DRAM_EINVAL before anything is launched.  None of the entries synchronises, allocates or reads device memory from the host.
 * dram_edt: dist[v] = the distance in mm from voxel v to the nearest voxel with feature != 0 under the voxel spacing (sz, sy, sx)
 *   (each in (0, 1e6]): 0 on a feature, +inf everywhere when there is none.  Defined bit for bit:
 *     dist = (float) sqrt(d2),  d2 = min over features of  fl(fl(fl(dx^2 * wx) + fl(dy^2 * wy)) + fl(dz^2 * wz))  in fp64,
 *   wz = fl(sz * sz), wy, wx likewise and dx, dy, dz the integer offsets; computed by three separable passes (x: nearest feature of
 *   the row; y, z: the plain minimum over the line), which give exactly that value because rounded addition is monotone.  Every
 *   dimension at most dram_edt_max_dim() (>= 1024).  ws: dram_edt_ws_bytes(D, H, W) bytes, 8-byte aligned (too small: DRAM_EWS);
 *   dram_edt_ws_bytes and dram_edt_max_dim answer without a GPU, the former 0 for sizes that dram_edt refuses.
 * dram_mask_surface: surf[v] = 1 where mask[v] is set and one of its six face neighbours is unset or outside the volume, else 0
 *   (mask & ~scipy.ndimage.binary_erosion(mask, generate_binary_structure(3, 1), border_value=0)); *count (device int64, zeroed
 *   here) = the number of surface voxels.
 * dram_surface_gather: out[0 .. n) = dist[v] for the n voxels with surf[v] != 0, in no particular order; *cursor (device int64,
 *   zeroed here) = n.  Slots at or past `capacity` (the floats that out holds) are not written.  1 <= nvox < 2^31. ---- */
int dram_edt_max_dim(void);
size_t dram_edt_ws_bytes(int D, int H, int W);
int dram_edt(const uint8_t* feature, float* dist, double sz, double sy, double sx, int D, int H, int W, void* ws, size_t ws_bytes,
             void* stream);
int dram_mask_surface(const uint8_t* mask, uint8_t* surf, int64_t* count, int D, int H, int W, void* stream);
int dram_surface_gather(const uint8_t* surf, const float* dist, float* out, int64_t* cursor, int64_t capacity, int64_t nvox,
                        void* stream);

/* ---- pseudo-vessel mask (csrc/vessel.hip): Frangi's multi-scale Hessian vesselness, the producer of the `vessel` input of
 *      dram_lesion_post (the reference reads one pseudo_vessels .mha file per scan, dram/dataset.py:379-383, and does not say how they were made).
 *      Volumes are contiguous [D,H,W] on the DEVICE, S = D*H*W < 2^31.  Null pointers, refused sizes and a radius over the cap
 *      are DRAM_EINVAL, a workspace that is too small DRAM_EWS, both before anything is launched.  None of the entries
 *      synchronises, allocates or reads device memory from the host.
 * Scales and taps: for a scale s in mm and the spacing (z, y, x) the caller forms, per axis a, sv[a] = s / spacing[a], the radius
 *   radius[a] = int(4.0 * sv[a] + 0.5) (scipy's truncate = 4.0) and the 1-D taps of order 0, 1, 2 of
 *   scipy.ndimage.gaussian_filter1d(sigma = sv[a], order = o) in fp64, rounds them once to fp32 and hands them over as the DEVICE
 *   table taps[3 axes z, y, x][3 orders][dram_vessel_max_radius() + 1]: taps[a][o][j] multiplies the sample at distance +j, the
 *   sample at -j gets the same weight (orders 0, 2) or its negative (order 1); entries past radius[a] must be zero.
 *   dram_vessel_max_radius() = 32 serves s = 4 mm at 0.5 mm spacing; a larger radius is refused, not clamped.
 * dram_hessian: h6[6][S] fp32 in the order zz, yy, xx, zy, zx, yx,  H_ab = fl(sv[a] * sv[b]) * (d^2/da db of G * I) in voxel units, the
 *   scale-normalised second derivative per mm^2.  scan: dtype DRAM_VESSEL_INT16 or DRAM_VESSEL_FLOAT32; every voxel is converted
 *   to fp32 and clamped to [clip_lo, clip_hi] on load (-inf, +inf: no clamp; a NaN stays).  Boundary: scipy's mode='reflect'
 *   (d c b a | a b c d), index i -> i mod 2n, then 2n-1-i when >= n, so an axis shorter than the radius is legal.  Three separable
 *   passes x, y, z (x: orders 0, 1, 2; y: the six combinations; z: one order per output), each output rounded to fp32; one
 *   output of one pass is, with w = taps[a][o], v the line and m = 4 * ceil(radius[a] / 4):
 *       acc = fl(w[0] * v[i]) (order 1: 0);  for j = 1 .. m:  acc = fma(w[j], fl(v[i+j] + v[i-j]), acc)   (order 1: fl(v[i+j] - v[i-j]))
 *   and the z pass multiplies by fl(sv[a] * sv[b]) (the product in fp64) last; a zero result is stored as +0.  No value depends on the launch geometry, the tile
 *   or the size of the volume around it beyond the reflection.  ws: dram_hessian_ws_bytes(D, H, W) bytes (nine fp32 volumes),
 *   4-byte aligned; the x pass moves 16 bytes per lane when W % 4 == 0 and ws is 16-byte aligned.  dram_hessian_ws_bytes and
 *   dram_vessel_max_radius answer without a GPU, the former 0 for sizes that dram_hessian refuses.
 * dram_hessian_norm_max: c_out[0] (device fp32) = Frangi's c: half the largest Frobenius norm of H over the voxels with lobe != 0
 *   (lobe == NULL: all voxels), 1 when that maximum is 0 (also: no voxel).  The norm is
 *   (float) sqrt(zz^2 + yy^2 + xx^2 + 2 (zy^2 + zx^2 + yx^2)) in fp64, summed left to right without fused multiply-adds; the maximum
 *   is an integer max-atomic on the bit patterns: exact and order-free.
 * dram_vesselness: per voxel the eigenvalues l1, l2, l3 of H by ascending magnitude, equal magnitudes by ascending value
 *   (numpy.linalg.eigvalsh, then a stable argsort of the magnitudes), solved in fp64 from the fp32 entries by five cyclic Jacobi
 *   sweeps, and with Ra = |l2| / |l3|, Rb = |l1| / sqrt(|l2 l3|), S2 = l1^2 + l2^2 + l3^2, c = c_dev[0] (device fp32):
 *       V = (1 - exp(-Ra^2 / 2 alpha^2)) * exp(-Rb^2 / 2 beta^2) * (1 - exp(-S2 / 2 c^2))      (bright tube on dark)
 *   in fp64 (1 - exp(-x) as -expm1(-x)), rounded once to fp32; exactly 0 when l2 >= 0 or l3 >= 0 or the expression is not finite.
 *   vmax[i] = accumulate ? max(vmax[i], V) : V -- the running maximum over scales.  eig ([3][S] fp64, may be NULL) receives
 *   l1, l2, l3.
 * dram_vessel_mask: mask[i] = (vmax[i] >= threshold) && (lobe == NULL || lobe[i] != 0).  (dram_threshold_mask is a strict > and
 *   has no lobe gate.) ---- */
#define DRAM_VESSEL_INT16 0
#define DRAM_VESSEL_FLOAT32 1
int dram_vessel_max_radius(void);
size_t dram_hessian_ws_bytes(int D, int H, int W);
int dram_hessian(const void* scan, int dtype, float clip_lo, float clip_hi, const float* taps, const int* radius, const double* sv,
                 int D, int H, int W, float* h6, void* ws, size_t ws_bytes, void* stream);
int dram_hessian_norm_max(const float* h6, const uint8_t* lobe, int64_t S, float* c_out, void* stream);
int dram_vesselness(const float* h6, int64_t S, double alpha, double beta, const float* c_dev, float* vmax, int accumulate,
                    double* eig, void* stream);
int dram_vessel_mask(const float* vmax, const uint8_t* lobe, float threshold, uint8_t* mask, int64_t n, void* stream);

/* ---- heat-map refinement (csrc/guided.hip; no counterpart in the reference): the masked 3-D guided filter (He, Sun and Tang)
 *      of the heat map, guided by the scan and restricted to a region (the lung).  Closed form, deterministic, nothing trained.
 *      Volumes are contiguous [D,H,W] on the DEVICE, S = D*H*W < 2^31.  The entry does not synchronise, allocate or read device
 *      memory from the host.
 * Inputs: guide G, either the int16 scan (DRAM_GUIDE_INT16) or a float32 volume (DRAM_GUIDE_FLOAT32); input P, float32, the heat
 *   map; region M, uint8, nonzero = inside; radius r = (rz, ry, rx) in voxels (a HOST array), each 0 <= r <=
 *   dram_guided_max_radius(); eps > 0.
 *   The guide value of an int16 scan is formed on load in fp64 as g = clamp((hu - lo) / (hi - lo), 0, 1); it is never
 *   materialised.  A float32 guide is taken as it is (lo and hi are not read).
 *   The window W(c) is the box c +- r, cut at the volume's edge.  All arithmetic is fp64 on the fp32 or int16 inputs; the
 *   products g*g and g*p are formed in fp64, where they are exact; no operation is fused into a multiply-add.
 *   1. For every c, over q in W(c) with M(q) != 0:  N = count, Sg = sum g, Sp = sum p, Sgg = sum g*g, Sgp = sum g*p.  Voxels with
 *      M = 0 are selected out, not multiplied by zero: a NaN or Inf outside the region reaches no output.
 *   2. Where M(c) != 0 (there N >= 1):  mg = Sg/N, mp = Sp/N, a = (Sgp/N - mg*mp) / ((Sgg/N - mg*mg) + eps), b = mp - a*mg.
 *      Elsewhere a and b are not defined and are never read.
 *   3. Where M(c) != 0:  A = (sum of a over W(c), M != 0) / N, B the same for b, q(c) = (float)(A*g(c) + B).  Elsewhere q(c) = 0.
 *      Every voxel of q is written.
 *   Every sum is a direct window sum, separable x, then y, then z, each axis added in ascending order from +0 with +0 for a
 *   voxel outside M or outside the volume; so a value depends on nothing but its window, and the call on any box that holds
 *   every voxel of M gives the bits of the whole-volume call.  No floating-point atomics: two calls on the same input give the
 *   same bits.  Everything that crosses memory between the passes is fp64.
 * dram_guided_max_radius() = 16 serves 8 mm at 0.5 mm spacing; a larger radius is refused, not clamped.
 * dram_guided_filter: ab ([2][S] fp64, may be NULL) receives a and b of step 2, 0 where M == 0.  ws: dram_guided_ws_bytes(D, H,
 *   W) bytes (twelve fp64 volumes); ws and ab 16-byte aligned.  Refused before anything is launched: a null required pointer,
 *   an unknown guide_kind, refused sizes, eps <= 0 or not finite, a radius negative or above the cap, DRAM_GUIDE_INT16 with
 *   hi <= lo or a window that is not finite, a misaligned pointer (all DRAM_EINVAL); a workspace that is too small (DRAM_EWS).
 *   dram_guided_ws_bytes and dram_guided_max_radius answer without a GPU, the former 0 for sizes that the filter refuses. ---- */
#define DRAM_GUIDE_INT16 0
#define DRAM_GUIDE_FLOAT32 1
int dram_guided_max_radius(void);
size_t dram_guided_ws_bytes(int D, int H, int W);
int dram_guided_filter(const void* guide, int guide_kind, double lo, double hi, const float* p, const uint8_t* mask, const int* radius,
                       double eps, int D, int H, int W, float* q, double* ab, void* ws, size_t ws_bytes, void* stream);

/* ---- result contact sheet (csrc/sheet.hip): the screenshot sheet of archive_results (job_runner.py:897-904), written by
 *      draw_mask_tile_singleview_heatmap (utils.py:542-620) and, with contours, draw_mask_tile_single_view (utils.py:464-539).
 *      Volumes are contiguous [D,H,W] on the DEVICE, n = (D, H, W), D*H*W < 2^31.  ca = coord_axis in 0..2; a < b are the two other
 *      axes: a tile's rows run along a, its columns along b (np.take along ca).  flip_axis in 0..2, or -1 for none.  zoom_size
 *      > 0, or 0 for none (the reference's zoom_size=None).  Everything below the drawing step is the reference's numpy / scipy
 *      geometry and is reproduced exactly; all outputs are integers.
 * 1. Flip (utils.py:547-552).  F[p] = V[p'] with p'[flip_axis] = n[flip_axis] - 1 - p[flip_axis]: the image, every layer and the
 *    coordinate mask.  Plane numbers (the flags of dram_sheet_occupancy, the slice ids of dram_sheet_render) count in F.
 * 2. Zoom (utils.py:556-577, ndimage.zoom(v, ratio, order), mode "constant", grid_mode off).  ratio = 1 along ca and zoom_size /
 *    max(n[a], n[b]) (one fp64 division) along a and b.  Per axis the output extent is zn = round-half-even(n * ratio) (one fp64
 *    product); a zoomed extent of 0 is refused.  Output index o reads the input coordinate c = o * step with step = (n - 1) /
 *    (zn - 1), the quotient rounded to fp64 before the product, and c = 0 when zn == 1.  The mode is "constant": where the
 *    rounded product exceeds n - 1 -- only the last index can, by one rounding -- that output index reads nothing and is 0 in
 *    either order, whatever the other axis does (scipy 1.15.3 blanks the last row or column of such a zoom; so does this).
 *      order 0 (coordinate mask, every layer): the voxel min(floor(c + 0.5), n - 1).
 *      order 1 (image): i0 = min(floor(c), n - 1), i1 = min(i0 + 1, n - 1), t = c - i0; v = v0 * (1 - t) + v1 * t in fp64, both
 *        products rounded on their own; separable, axis a first, then axis b on the unrounded fp64 results; the sum becomes uint8
 *        as floor(v + 0.5).  Along ca the map is the identity (t = 0, the lerp returns v0): plane k of the result depends on
 *        plane k of the source alone.
 * 3. Pad (utils.py:566-569).  Each zoomed plane is centred in a zoom_size x zoom_size tile of zeros: (zoom_size - zn) / 2 (floor)
 *    in front, the rest behind; zn <= zoom_size always, so the reference's crop never cuts.  Without a zoom a tile is the raw
 *    plane n[a] x n[b].  The pad comes before the drawing: a heat-map row shows the colour of value 0 there.
 * 4. Slice choice (utils.py:579-592) is the host's (dram_amd.sheet.pick_slices) from the flags of dram_sheet_occupancy: flag[k] !=
 *    0 iff plane k of the ZOOMED coordinate mask holds a non-zero voxel -- under a nearest-neighbour down-zoom a plane's only
 *    voxel can be skipped.
 * 5. Layout (utils.py:595-614).  Slice j gives column j: the grey tile (the zoomed image on three channels) on top, below it one
 *    rendered tile per row; columns left to right; the sheet is padded with zeros to sheet_width, (sheet_width - cur) / 2 (floor)
 *    on the left (sheet_width 0: no pad).  Sheet: uint8 [(1 + n_rows) * th][max(sheet_width, num_slices * tw)][3].
 * 6. 8-bit sources, formed on load, before the zoom (job_runner.py:897-901):
 *      image DRAM_SHEET_INT16  windowing(scan, (wmin, wmax), (0, 255)).astype(uint8) (utils.py:189-198): clip, fp64 quotient, * 255,
 *                              + 0, truncation (windowed_scan and scan_bin of csrc/volume_math.h); DRAM_SHEET_U8: as it is.
 *      layer DRAM_SHEET_MASK   uint8, 255 where non-zero (the reference passes mask * 255)
 *            DRAM_SHEET_U8     uint8, as it is
 *            DRAM_SHEET_UNIT   float32 through windowing(h, (0, 1)): numpy stays in fp32 there -- clip to [0, 1], / 1.0f, * 255.0f
 *                              (one fp32 product), + 0.0f, truncation.  NaN maps to 0: OUR definition, numpy's cast of NaN is
 *                              undefined.
 * 7. Drawing.  PARITY UNPINNED: OpenCV is not available here, so nothing of this step is checked against it; it is defined here.
 *    With a = (float)alpha and b = (float)(1.0 - alpha) (the difference in fp64), blend(x, y) = sat(rne((float)x * a + (float)y * b)):
 *    fp32, the two products rounded on their own, one addition, round half to even, clamped to 0..255.
 *      DRAM_SHEET_HEATMAP (draw_2d_heatmap, utils.py:634-644: applyColorMap + addWeighted): per channel, start from the grey value
 *        and for every layer of the row in order  value = blend(map[layer value][channel], value).  The colour map is a
 *        256-entry table from a closed form, t = i / 255.0 in fp64, entry = rne(255.0 * c):
 *          DRAM_SHEET_JET     c = clamp(1.5 - |4 t - k|, 0, 1), k = 3, 2, 1 for r, g, b
 *          DRAM_SHEET_SUMMER  (r, g, b) = (t, 0.5 + 0.5 t, 0.4)
 *        every operation in fp64, rounded on its own, in the order written (t first, then 4 t, the difference, the absolute value,
 *        1.5 minus it, the clamp, the product with 255): on jet's ramps 255 c is a half-integer in exact arithmetic, so the
 *        entry is what these roundings leave.
 *        not OpenCV's tables.
 *      DRAM_SHEET_CONTOUR (draw_2d, utils.py:623-631): painted = the grey value on three channels; every layer of the row in order
 *        paints its colour over it: thickness -1 at every pixel of the zoomed, padded layer that is non-zero; thickness 1 at
 *        those of them that have a 4-neighbour which is zero or lies outside the tile.  value = blend(painted, grey).  This is
 *        OUR definition of an outline, not OpenCV's findContours / drawContours.
 *    Other deviations: channels are stored in RGB order (the reference builds BGR for cv2.imwrite), and titles are not
 *    rasterised (cv2.putText's Hershey font is not reproduced); the host returns every tile's rectangle instead.
 * dram_sheet_occupancy: up to DRAM_SHEET_MAX_MASKS uint8 masks (`masks`: a HOST array of n_masks device pointers), ORed on load;
 *   flags: n[ca] device int32, every one written (0 or 1).  Planes, rows and, along x, bytes that the order-0 zoom does not
 *   sample are not looked at; rows that it skips are not read.  The flags are cleared and then set with plain vector stores of
 *   the value 1, so concurrent writers agree.  W <= DRAM_SHEET_MAX_W.
 * dram_sheet_render: the whole sheet in one launch, every byte written.  `layers`: a HOST array of the rows' layers, row after
 *   row; row_layers[r] = the number of layers of row r (>= 1); slice_ids: num_slices plane numbers in F.  Both tables travel in
 *   the kernel arguments.  A layer's colour and thickness are read by DRAM_SHEET_CONTOUR only.
 * Refused before anything is launched (DRAM_EINVAL): a null required pointer, sizes not positive or D*H*W >= 2^31, W above the
 *   cap (occupancy), an axis, kind, style, colour map or thickness not listed here, zoom_size < 0, a zoomed extent of 0, wmax
 *   <= wmin for an int16 image, alpha outside [0, 1] or not finite, counts outside 1 .. their caps, a slice id outside
 *   0 .. n[ca] - 1, 0 < sheet_width < num_slices * tw, a float32 layer that is not 4-byte or an int16 image that is not 2-byte
 *   aligned.  Neither entry synchronises, allocates or reads device memory from the host. ---- */
#define DRAM_SHEET_MAX_MASKS 4
#define DRAM_SHEET_MAX_W 32768
#define DRAM_SHEET_MAX_ROWS 8
#define DRAM_SHEET_MAX_LAYERS 16
#define DRAM_SHEET_MAX_SLICES 16
#define DRAM_SHEET_INT16 0
#define DRAM_SHEET_U8 1
#define DRAM_SHEET_MASK 2
#define DRAM_SHEET_UNIT 3
#define DRAM_SHEET_HEATMAP 0
#define DRAM_SHEET_CONTOUR 1
#define DRAM_SHEET_JET 0
#define DRAM_SHEET_SUMMER 1
typedef struct dram_sheet_layer {
    const void* data;          /* device, [D,H,W] */
    int kind;                  /* DRAM_SHEET_MASK | DRAM_SHEET_U8 | DRAM_SHEET_UNIT */
    int thickness;             /* -1 or 1 */
    unsigned char color[4];    /* r, g, b, unused */
} dram_sheet_layer;
int dram_sheet_occupancy(const void* const* masks, int n_masks, int D, int H, int W, int coord_axis, int flip_axis, int zoom_size,
                         int* flags, void* stream);
int dram_sheet_render(const void* image, int image_kind, int wmin, int wmax, const dram_sheet_layer* layers, const int* row_layers,
                      int n_rows, const int* slice_ids, int num_slices, int D, int H, int W, int coord_axis, int flip_axis,
                      int zoom_size, int sheet_width, int style, int colormap, double alpha, uint8_t* sheet, void* stream);

/* ---- test-time augmentation for the per-lobe inference (csrc/infer_tta.hip; no counterpart in the reference): the chunks go
 *      through the model in V orientations, the heat map is the mean of the V sigmoid maps and the spread map their standard
 *      deviation.
 * A VIEW is a signed permutation {perm[3], flip[3]} of the spatial axes of an R^3 chunk in dram_spatial_permute_flip's convention:
 *   xv[o] = x[i] with i[perm[k]] = flip[k] ? R-1-o[k] : o[k].  `views` is a HOST array of V x 6 ints {perm[0..2], flip[0..2]},
 *   1 <= V <= DRAM_TTA_MAX_VIEWS; a view may occur more than once and then counts that many times.
 * For chunk l and a point i of the canonical (unviewed) grid, with o_v(i) the point of view v that shows i (o[k] = flip[k] ?
 *   R-1-i[perm[k]] : i[perm[k]], the inverse of the move above):
 *       p_v(i) = 1 / (1 + expf(-dense[v][l][o_v(i)]))                        (dram_lobe_paste's sigmoid expression)
 *       m(i)   = (p_0 + p_1 + ... + p_{V-1}) / (float)V                      fp32 additions in view order, pairwise
 *       s(i)   = sqrtf(((p_0 - m)^2 + ... + (p_{V-1} - m)^2) / (float)V)     the POPULATION standard deviation, same order,
 *   every operation rounded on its own (no fused multiply-add).  Both sums run over the binary tree of the view index: views
 *   2j and 2j+1 are added first, then pairs of pairs and so on, the earlier views on the left; V's binary digits leave complete
 *   blocks ([0,32) and [32,48) for V = 48; [0,2) and {2} for V = 3), which are joined from the last one upwards
 *   (B_1 + (B_2 + (B_3 + ...))).  Added this way 2, 4 or 8 equal probabilities give m equal to that probability bit for bit and
 *   s == 0, and 3 or 48 equal ones are off by the two roundings of 3p and of the division at most; added left to right the
 *   partial sums 3p, 5p, 6p, 7p, ... each round and 48 equal values end up to 11 ulp off.
 * The ensemble is formed at the chunk's resolution; the heat map is m resized to the crop and pasted by dram_lobe_paste's rule,
 *   the spread map is s resized and pasted the same way.  The resize is linear, so the pasted mean is the mean of the pasted
 *   views up to rounding; the pasted spread is the RESIZED chunk-level deviation, NOT the deviation of the resized views.
 * dram_tta_expand: x [L,1,R,R,R] -> xv [V,L,1,R,R,R], every view of every chunk in one launch; xv[v] equals
 *   dram_spatial_permute_flip(x, perm_v, flip_v) bit for bit (data movement only).
 * dram_tta_combine: dense [V,L,1,R,R,R] -> mean [L,R^3] and spread [L,R^3] (spread may be NULL) in one pass: every element of
 *   dense is read once and the V probabilities of a point stay in registers.  A block owns an 8 x 8 x 16 box of the canonical
 *   grid: views that keep x in place (perm[2] == 2) are read along their rows, ascending or descending; views that move x are
 *   read in their own order in runs of 8 or 16 consecutive floats and turned through LDS.
 * dram_lobe_paste_prob: dram_lobe_paste without the sigmoid, on one or two fields [L,R^3] in one walk over the crop: for every
 *   voxel of chunk l with lobe == label, htp = resize(prob[l]) and, when given, htp2 = resize(prob2[l]) (prob2 and htp2 are both
 *   NULL or both set); the same align-corners indices, weights and 8-term combination; every other voxel is left untouched.
 *   `chunks` as for dram_lobe_paste (L <= 8).
 * V outside 1..DRAM_TTA_MAX_VIEWS, a perm that is not a permutation of {0,1,2}, a flip other than 0 or 1, L outside 1..8, R < 2
 *   and a null required pointer are DRAM_EINVAL before anything is launched.  None of the entries synchronises, allocates or
 *   reads device memory from the host. ---- */
#define DRAM_TTA_MAX_VIEWS 48
int dram_tta_expand(const float* x, float* xv, int L, int R, const int* views, int V, void* stream);
int dram_tta_combine(const float* dense, float* mean, float* spread, int L, int R, const int* views, int V, void* stream);
int dram_lobe_paste_prob(const float* prob, const float* prob2, const uint8_t* lobe, float* htp, float* htp2, const int* chunks,
                         int L, int D, int H, int W, int R, void* stream);

/* ---- the optimiser update (st_dram_ref.py: torch.optim.Adam(lr=1e-4) under ExponentialLR; the SGD block beside it):
 *      multi-tensor Adam / AdamW / SGD on fp32 tensors, one launch per table of up to DRAM_OPTIM_TABLE_CAPACITY tensors.
 * `table` is HOST memory, read before the call returns (it travels to the device in the kernel arguments): per tensor the
 *   device pointers p (parameter), g (gradient), m, v, vmax of n contiguous floats each (1 <= n < 2^31; 4-byte aligned, any
 *   offset: a tensor whose pointers are all 16-byte aligned moves as 16-byte accesses, any other one element per lane) and two
 *   per-tensor scalars.  The tensors of a table must not overlap.  Neither entry synchronises, allocates or reads device memory
 *   from the host.
 * dram_optim_adam: per element, t = the tensor's own step count after increment, bc1 = 1 - beta1^t, bc2 = 1 - beta2^t:
 *     g' = maximize ? -g : g;  decoupled (AdamW): p *= 1 - lr * weight_decay;  else: g' += weight_decay * p;
 *     m = beta1 * m + (1 - beta1) * g';  v = beta2 * v + (1 - beta2) * g'^2;  vuse = amsgrad ? (vmax = max(vmax, v)) : v;
 *     p -= s0 * m / (sqrt(vuse) / s1 + eps)        with s0 = lr / bc1 and s1 = sqrt(bc2) formed by the caller in double.
 *   m, v: exp_avg, exp_avg_sq; vmax: max_exp_avg_sq (read only with amsgrad).  `lr` enters only the AdamW decay.
 * dram_optim_sgd (torch.optim.SGD's rule): g' = maximize ? -g : g;  g' += weight_decay * p;  with momentum != 0:
 *     buf = s0 != 0 ? g' : momentum * buf + (1 - dampening) * g';  g' = nesterov ? g' + momentum * buf : buf;   p -= lr * g'.
 *   m: momentum_buffer (ignored when momentum == 0; s0 != 0 marks the tensor's first step, where buf need not be initialised);
 *   v, vmax, s1 unused.
 * dram_optim_radam (torch.optim.RAdam's rule; st_dram_ref.py:99 "engine.models.optimizer.RAdam", whose rectified branch it is):
 *     g', the weight decay (decoupled or not), m and v as for dram_optim_adam;
 *     p -= s0 * (s1 != 0 ? m / (sqrt(v) + eps) : m)       eps joins the RAW root (Adam: sqrt(v) / sqrt(bc2) + eps)
 *   with, formed by the caller in double: rho_inf = 2 / (1 - beta2) - 1, rho_t = rho_inf - 2 t beta2^t / bc2; rectified
 *   (rho_t > 5, a function of t alone): s0 = lr * rect * sqrt(bc2) / bc1, rect = sqrt((rho_t - 4)(rho_t - 2) rho_inf /
 *   ((rho_inf - 4)(rho_inf - 2) rho_t)), s1 != 0; otherwise s0 = lr / bc1, s1 = 0.  vmax unused.
 * dram_optim_adabound (Luo et al. 2019 as the adabound package 0.0.5 evaluates it; st_dram_ref.py:81 "adabound.AdaBound"):
 *     g' = g + weight_decay * p;  m, v as above;  vuse = amsbound ? (vmax = max(vmax, v)) : v;
 *     p -= clamp(s0 / (sqrt(vuse) + eps), lower, upper) * m      with s0 = lr * sqrt(bc2) / bc1 formed by the caller in double.
 *   lower = final (1 - 1 / (gamma t + 1)) and upper = final (1 + 1 / (gamma t)), final = final_lr * lr / base_lr, depend on t and
 *   are launch scalars (lower <= upper): the caller issues one launch per distinct step count.  A NaN quotient stays a NaN. ---- */
#define DRAM_OPTIM_TABLE_CAPACITY 64
typedef struct dram_optim_tensor {
    float* p;
    const float* g;
    float* m;
    float* v;
    float* vmax;
    int64_t n;
    float s0;
    float s1;
} dram_optim_tensor;
int dram_optim_table_capacity(void);
int dram_optim_adam(const dram_optim_tensor* table, int count, double lr, double beta1, double beta2, double eps,
                    double weight_decay, int decoupled, int amsgrad, int maximize, void* stream);
int dram_optim_sgd(const dram_optim_tensor* table, int count, double lr, double momentum, double dampening,
                   double weight_decay, int nesterov, int maximize, void* stream);
int dram_optim_radam(const dram_optim_tensor* table, int count, double lr, double beta1, double beta2, double eps,
                     double weight_decay, int decoupled, int maximize, void* stream);
int dram_optim_adabound(const dram_optim_tensor* table, int count, double beta1, double beta2, double eps, double weight_decay,
                        int amsbound, double lower, double upper, void* stream);

/* ---- global-norm gradient clipping (torch.nn.utils.clip_grad_norm_) over the same tables: of every entry only g and n are
 *      read (1 <= n < 2^31, g 4-byte aligned at any offset: 16-byte accesses where g is 16-byte aligned, one element per lane
 *      otherwise); p, m, v, vmax, s0, s1 may be anything.  A tensor of n elements takes cdiv(n, 4096) consecutive blocks.
 * dram_optim_grad_norm_partials: the number of partials (= blocks) a table needs; 0 and dram_last_error() for a table that
 *   dram_optim_grad_norm would refuse.  Answers without a GPU.
 * dram_optim_grad_norm: block b of the table writes partials[partial_offset + b] (device doubles): kind DRAM_OPTIM_NORM_2 the
 *   sum of its elements' squares, every square exact and the sum in fp64 (within n 2^-53 relative of the exact sum: 1e20 does
 *   not overflow, 1e-30 does not vanish); kind DRAM_OPTIM_NORM_INF the maximum of |g|, NaN if any element is.  Every partial is
 *   written by exactly one block, in a fixed order of additions: no atomics, the same bits every run.  A second table of the
 *   same gradient set continues at partial_offset = the partials of the tables before it.
 * dram_optim_grad_norm_finish: one block over partials[0 .. n_partials) in a fixed order; out (device, 2 floats):
 *     out[0] = total_norm = kind 2: (float)sqrt(sum), kind inf: max;
 *     out[1] = clip_coef  = c > 1 ? 1 : c  with c = (float)max_norm / (total_norm + 1e-6f), every operation in fp32;
 *   a NaN norm gives a NaN coefficient and an infinite norm the coefficient 0, as torch.clamp(max=1) leaves them.
 * dram_optim_adam_scaled / dram_optim_sgd_scaled / dram_optim_radam_scaled / dram_optim_adabound_scaled: the entry of the same
 *   name without the suffix, with every gradient element replaced by the
 *   fp32 product g * gscale[0] before anything else (maximize, weight decay, ...); gscale is a DEVICE pointer (out + 1 above),
 *   read once per block; the gradient buffer is not written.  gscale == NULL: bit for bit the unscaled entry.
 * dram_optim_grad_scale: g[i] = g[i] * gscale[0] in place (the table's g is written despite its const).
 * None of them synchronises, allocates or reads device memory from the host. ---- */
#define DRAM_OPTIM_NORM_2 2
#define DRAM_OPTIM_NORM_INF 0
size_t dram_optim_grad_norm_partials(const dram_optim_tensor* table, int count);
int dram_optim_grad_norm(const dram_optim_tensor* table, int count, int kind, double* partials, int64_t partial_offset,
                         void* stream);
int dram_optim_grad_norm_finish(const double* partials, int64_t n_partials, int kind, double max_norm, float* out, void* stream);
int dram_optim_adam_scaled(const dram_optim_tensor* table, int count, double lr, double beta1, double beta2, double eps,
                           double weight_decay, int decoupled, int amsgrad, int maximize, const float* gscale, void* stream);
int dram_optim_sgd_scaled(const dram_optim_tensor* table, int count, double lr, double momentum, double dampening,
                          double weight_decay, int nesterov, int maximize, const float* gscale, void* stream);
int dram_optim_radam_scaled(const dram_optim_tensor* table, int count, double lr, double beta1, double beta2, double eps,
                            double weight_decay, int decoupled, int maximize, const float* gscale, void* stream);
int dram_optim_adabound_scaled(const dram_optim_tensor* table, int count, double beta1, double beta2, double eps,
                               double weight_decay, int amsbound, double lower, double upper, const float* gscale, void* stream);
int dram_optim_grad_scale(const dram_optim_tensor* table, int count, const float* gscale, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* DRAM_HIP_H */
