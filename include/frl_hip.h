/* frl_hip.h -- C ABI of libfrlhip.so: the MI355X (gfx950) VQ-VAE training hot path.
 *
 * The reference (nnnagle/vq-vae) is pure Python/PyTorch and has NO native plugin interface; the boundary these
 * entry points replace is the set of torch ops the reference's hot path executes.  Each
 * declaration cites the reference call site (file:line under /root/reference) whose forward and autograd backward
 * it stands in for.
 *
 * Conventions
 *   - every function returns 0 on success, a negative code on failure; frl_last_error() gives the thread-local text;
 *   - all pointers are BORROWED DEVICE pointers (owned by the caller, e.g. torch tensors); the library allocates
 *     nothing user-visible; scratch comes from a caller-provided workspace sized by *_workspace_bytes();
 *   - explicit hipStream_t (void*) argument, no global state: functions are re-entrant and graph-capturable;
 *   - activations are NHWC rows [P][C] (C contiguous) of `dtype` (FRL_F32 = 0 | FRL_BF16 = 1);
 *     parameters and their gradients are float32 in the reference's own layouts (OIHW / [Cout][Cin][k]);
 *   - act: 0 none, 1 relu, 2 sigmoid.  Backward entry points take the activation OUTPUT y to apply act'(y).
 */
#ifndef FRL_HIP_H
#define FRL_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* frl_stream_t; /* hipStream_t */

enum { FRL_F32 = 0, FRL_BF16 = 1, FRL_F16 = 2 /* raw chunk-store rows of frl_normalize_tiles only */ };
enum { FRL_ACT_NONE = 0, FRL_ACT_RELU = 1, FRL_ACT_SIGMOID = 2 };

/* ---- library ------------------------------------------------------------------------------------------------- */
int frl_version(void);
const char* frl_last_error(void);
int frl_device_arch(char* buf, int n); /* must report gfx950 */
/* Live per-kernel timing (bench.py): with the switch on, every kernel the library launches is bracketed by a HIP event pair recorded on
 * its launch stream; the report synchronises them and writes "kernel expression \t calls \t total ms \n" lines. */
int frl_kernel_timing_enable(int on);
int frl_kernel_timing_report(char* buf, int n);

/* ---- weight-image cache ------------------------------------------------------------------------------------------------------
 * Every conv-like call first rewrites its float32 weights into a packed MFMA fragment image (a small prologue launch per call).  A
 * caller that knows when the weights change (the trainer: once per optimizer step) keeps the images in an arena of its own:
 *   h = frl_pack_cache_create(arena, bytes)   arena: device memory owned by the caller, at least frl_pack_cache_table_bytes() + images
 *   frl_pack_cache_activate(h)                calls made from now on (any thread) find / register their image in cache h and skip the
 *                                             prologue on a hit; frl_pack_cache_activate(0) restores the default (pack per call)
 *   frl_pack_cache_refresh(h, stream)         rewrites EVERY registered image from the current weights with ONE launch
 *   frl_pack_cache_destroy(h)
 * An image is valid from its registration (or the last refresh) until its weights change: refresh right after the optimizer. */
size_t frl_pack_cache_table_bytes(void);
int frl_pack_cache_create(void* arena, size_t bytes);
int frl_pack_cache_destroy(int handle);
int frl_pack_cache_activate(int handle);      /* returns the previously active handle */
int frl_pack_cache_images(int handle);        /* number of registered images */
int frl_pack_cache_refresh(int handle, frl_stream_t stream);

/* ---- pointwise (1x1) convolution --------------------------------------------------------------------------------
 * nn.Conv2d(.,.,1): frl/models/conv2d_encoder.py:106-114; spatial.py:262-263; representation.py:169;
 * conditioning.py:55-67; decoder template heads.py:128-198.  w [Cout][Cin], bias [Cout] or NULL. */
/* every forward / bwd_data convolution entry point takes a workspace of frl_conv_workspace_bytes(Cin, Cout, taps) bytes
 * (taps = 1 pointwise, 3 temporal, 9 spatial; 6 covers a whole TCN block) for the packed MFMA weight image it builds. */
size_t frl_conv_workspace_bytes(int Cin, int Cout, int taps);
int frl_conv1x1_fwd(const void* x, const float* w, const float* bias, void* y, int64_t P, int Cin, int Cout, int act,
                    int dtype, void* ws, size_t ws_bytes, frl_stream_t stream);
int frl_conv1x1_bwd_data(const void* dy, const void* y, int act, const float* w, void* dx, int64_t P, int Cin, int Cout,
                         int dtype, void* ws, size_t ws_bytes, frl_stream_t stream);
/* Backward-pass accumulation in the epilogue (autograd's sum of the gradients of a tensor with two consumers, fused into the
 * kernel that produces one of them): dx = (dy .* act'(y)) W + add.  add [P][Cin] must not alias dx. */
int frl_conv1x1_bwd_data_add(const void* dy, const void* y, int act, const float* w, void* dx, const void* add, int64_t P,
                             int Cin, int Cout, int dtype, void* ws, size_t ws_bytes, frl_stream_t stream);
/* Tuning hook (no reference counterpart): upper bound of the workgroups, i.e. float32 partial slabs, of a 1x1 weight-gradient launch;
 * returns the previous bound.  frl_conv1x1_bwd_weight_workspace_bytes follows it: size workspaces after changing it. */
int frl_wgrad_set_max_workgroups(int n);
/* A/B hook: 1 (default) = bf16 weight gradients with Cin = 64, Cout in {4, 8, 12, 16}, no mask, no time shift, whole 64-row tiles and
 * 16-byte aligned operands (the 64 -> 12 phase head) take the streaming kernel pw_wgrad_thin_kernel, 0 = every call takes the generic
 * kernel; same workgroups, slabs and bits either way.  Returns the previous setting. */
int frl_wgrad_thin(int on);
size_t frl_conv1x1_bwd_weight_workspace_bytes(int64_t P, int Cin, int Cout);
int frl_conv1x1_bwd_weight(const void* dy, const void* y, int act, const void* x, float* dw, float* dbias, int64_t P,
                           int Cin, int Cout, int dtype, void* ws, size_t ws_bytes, frl_stream_t stream);
/* generalised weight gradient: rows are (b, t, hw); x is read at time t + toff (zero outside [0,T));
 * dw destination strides (dso, dsi) address one tap of a [Cout][Cin][ntap] tensor (nn.Conv1d, tcn.py:56-62).
 * flags bit0: scalar LDS fragment reads (debug), bit1: accumulate into dbias. */
int frl_conv_tap_bwd_weight(const void* dy, const void* y, int act, const void* x, float* dw, int64_t dso, int64_t dsi,
                            float* dbias, int64_t P, int Cin, int Cout, int HW, int T, int toff, int dtype, void* ws,
                            size_t ws_bytes, int flags, frl_stream_t stream);

/* ---- 3x3 convolution, pad 1 ------------------------------------------------------------------------------------
 * nn.Conv2d(.,.,3,padding=1): frl/models/spatial.py:258-261 (mix_backbone), :266-272 (gate_net).
 * x [B][H][W][Cin], w [Cout][Cin][3][3]. */
int frl_conv3x3_fwd(const void* x, const float* w, const float* bias, void* y, int B, int H, int W, int Cin, int Cout,
                    int act, int dtype, void* ws, size_t ws_bytes, frl_stream_t stream);
/* gate_net's second convolution with the blend in its epilogue (spatial.py:332-335 at min_gate = 0): gate = sigmoid(conv3x3(x) + bias),
 * out = smoothed + gate * residual.  One launch instead of the convolution + frl_gate_blend_fwd. */
int frl_conv3x3_fwd_gate_blend(const void* x, const float* w, const float* bias, const void* smoothed, const void* residual, void* gate,
                               void* out, int B, int H, int W, int Cin, int Cout, int dtype, void* ws, size_t ws_bytes,
                               frl_stream_t stream);
int frl_conv3x3_bwd_data(const void* dy, const void* y, int act, const float* w, void* dx, int B, int H, int W, int Cin,
                         int Cout, int dtype, void* ws, size_t ws_bytes, frl_stream_t stream);
/* frl_conv3x3_bwd_data with epilogue extras: dx = conv(...) + add (add may be null); with the pair sub_from / out2 (both or neither)
 * also out2 = sub_from - dx.  EdgeAwareSmoothingConv2D's backward uses both: the residual's two gradient streams are summed here and
 * d_smoothed - d_residual leaves in the same launch (spatial.py:331-339: residual = x - smoothed feeds the gate net and the blend). */
int frl_conv3x3_bwd_data_fused(const void* dy, const void* y, int act, const float* w, void* dx, const void* add,
                               const void* sub_from, void* out2, int B, int H, int W, int Cin, int Cout, int dtype, void* ws,
                               size_t ws_bytes, frl_stream_t stream);
/* frl_conv3x3_bwd_data_fused whose add operand is the gate blend's d_residual, formed in the epilogue instead of read: dx = conv(...) +
 * round(dout * gate) (rounded to the tensor dtype, as frl_gate_blend_bwd stores it with min_gate <= 0), out2 = dout - dx.  gate, dout and
 * out2 [B][H][W][Cin] are all required; same bits as the two-step form. */
int frl_conv3x3_bwd_data_blend(const void* dy, const void* y, int act, const float* w, void* dx, const void* gate, const void* dout,
                               void* out2, int B, int H, int W, int Cin, int Cout, int dtype, void* ws, size_t ws_bytes,
                               frl_stream_t stream);
/* dx = conv^T(dy .* act'(y)) .* out_act'(out_y): out_y [B][H][W][Cin] is the output of the ReLU / sigmoid (out_act) that the NEXT backward
 * step differentiates through at the same pixels; that step's calls then take dx with act = FRL_ACT_NONE (no mask pass over their input:
 * 16-35 us per 3x3 backward-data call and 6-15 us per weight-gradient call at BASELINE configs[1]). */
int frl_conv3x3_bwd_data_outmask(const void* dy, const void* y, int act, const float* w, void* dx, const void* out_y, int out_act, int B,
                                 int H, int W, int Cin, int Cout, int dtype, void* ws, size_t ws_bytes, frl_stream_t stream);
size_t frl_conv3x3_bwd_weight_workspace_bytes(int B, int H, int W, int Cin, int Cout);
int frl_conv3x3_bwd_weight(const void* dy, const void* y, int act, const void* x, float* dw, float* dbias, int B, int H,
                           int W, int Cin, int Cout, int dtype, void* ws, size_t ws_bytes, int flags, frl_stream_t stream);
/* Up to 4 weight gradients over images of ONE shape [B][H][W] in one call (the three 3x3 convolutions of a smoothing block's backward):
 * dy, y, x, dw, dbias, act, cin, cout are arrays of njobs entries; y[j] (with act[j] == 0), dw[j] and dbias[j] may be null.  Gradients
 * are bit for bit those of frl_conv3x3_bwd_weight.  When every job is bf16 with H % 8 == 0, W % 32 == 0, Cin % 64 == 0 and Cout == 64,
 * ONE launch of the band kernel serves all jobs in two cases (tiles = B * H / 8 * W / 32): the jobs' tiles together fit 256 workgroups
 * (one tile per workgroup); or tiles >= 256 and the jobs have at most 8 64-channel chunks in all: every (job, chunk) gets 64 workgroups,
 * workgroup k runs the four tile ranges that workgroups k, k + 64, k + 128, k + 192 of the single call own, each accumulated from zero,
 * and adds them up in ONE slab in that order -- the chain in which the fixed-order reduction adds the single call's 256 slabs -- so a job
 * leaves 64 slabs instead of 256 in its region of `ws`, reduced (deferrably) on their own.  Any other set of jobs runs job by job as
 * frl_conv3x3_bwd_weight.  The workspace size depends on the route, so on frl_conv3x3_wgrad_multi: ask for it under the setting the
 * call runs with. */
size_t frl_conv3x3_bwd_weight_multi_workspace_bytes(int njobs, int B, int H, int W, const int* cin, const int* cout, int dtype);
int frl_conv3x3_bwd_weight_multi(int njobs, const void* const* dy, const void* const* y, const int* act, const void* const* x,
                                 float* const* dw, float* const* dbias, int B, int H, int W, const int* cin, const int* cout, int dtype,
                                 void* ws, size_t ws_bytes, frl_stream_t stream);
/* A/B hook: 0 = frl_conv3x3_bwd_weight_multi always runs job by job (default 1); returns the previous setting. */
int frl_conv3x3_wgrad_multi(int on);
/* Test / A-B hook (no reference counterpart): 1 routes every 3x3 weight gradient through the generic kernel instead of the bf16
 * band kernel; returns the previous setting. */
int frl_conv3x3_wgrad_force_generic(int on);
/* Test / A-B hook: 0 = conv3x3 forward / bwd-data on 16-row tiles only (default 1: bf16 images of >= 32 rows take 32 x 16 tiles); returns the previous setting. */
int frl_conv3x3_tile32(int on);

/* ---- GroupNorm over NHWC rows ----------------------------------------------------------------------------------
 * nn.GroupNorm(G, C), eps 1e-5, per-sample statistics: frl/models/conv2d_encoder.py:117 (ReLU fused when relu=1,
 * :119-121).  mean/rstd [B][G] f32 are saved for the backward. */
int frl_groupnorm_fwd(const void* x, const float* gamma, const float* beta, void* y, float* mean, float* rstd, int B,
                      int HW, int C, int G, float eps, int relu, int dtype, frl_stream_t stream);
size_t frl_groupnorm_bwd_workspace_bytes(int B, int C, int G);
int frl_groupnorm_bwd(const void* dy, const void* x, const float* gamma, const float* beta, const float* mean,
                      const float* rstd, void* dx, float* dgamma, float* dbeta, int B, int HW, int C, int G, int relu,
                      int dtype, void* ws, size_t ws_bytes, frl_stream_t stream);

/* ---- loss head (csrc/elementwise.hip) ----------------------------------------------------------------------------
 * out[0] = sum_i coef[i] * *terms[i] (device scalars, host coefficients, n <= 8), ok_out[0] (optional) = 1 if out[0] is finite else 0: the weighted
 * sum of the loss terms (scripts/train_vqvae.py:236-248) and the isfinite guard (step.py:1057-1074) in one launch; its backward. */
int frl_scalar_combine(const float* const* terms_host, const float* coef_host, int n, float* out, float* ok_out, frl_stream_t stream);
int frl_scalar_fanout(const float* g, const float* coef_host, int n, float* out, frl_stream_t stream);
/* the same with optional device multipliers (mult_host: n device pointers, entries or the array may be NULL): term i is weighted by
 * coef[i] * *mult[i] -- a loss weight on a per-step schedule (lambda_vq(step), scripts/train_vqvae.py:236-248,324) stays a device word
 * that a captured graph reads at replay time */
int frl_scalar_combine_dev(const float* const* terms_host, const float* coef_host, const float* const* mult_host, int n, float* out,
                           float* ok_out, frl_stream_t stream);
/* frl_scalar_combine_dev plus a second, un-scheduled combination of the same terms: aux_out[0] = sum_i aux_coef[i] * *terms[i] (a reported
 * sub-total such as vq_loss = L_codebook + beta L_commit of scripts/train_vqvae.py:236-248) in the same launch. */
int frl_scalar_combine_aux(const float* const* terms_host, const float* coef_host, const float* const* mult_host, const float* aux_coef_host,
                           int n, float* out, float* ok_out, float* aux_out, frl_stream_t stream);
int frl_scalar_fanout_dev(const float* g, const float* coef_host, const float* const* mult_host, int n, float* out, frl_stream_t stream);
/* frl_scalar_fanout_dev plus the check of a promise: promise_host (n device pointers, entries or the array may be NULL) names, per term, the
 * gradient the term was promised at forward time (frl_decoder_mse_fwd_bwd computed its gradients with it); flag[0] (device int) is set to 1
 * when a term's gradient differs from its promise and is left alone otherwise -- a sticky word the host polls where it synchronises anyway. */
int frl_scalar_fanout_guard(const float* g, const float* coef_host, const float* const* mult_host, const float* const* promise_host, int n,
                            float* out, int* flag, frl_stream_t stream);

/* ---- fused two-layer type encoder (csrc/enc_fused.hip) -----------------------------------------------------------
 * conv1x1 C0->C1 (no bias) -> GroupNorm(G1) -> ReLU -> conv1x1 C1->C2 (no bias) -> GroupNorm(G2): Conv2DEncoder with two layers
 * (frl/models/conv2d_encoder.py:100-159) as ONE launch per direction, one workgroup per sample; the 128-channel intermediates never
 * reach HBM in the forward.  frl_encoder2_supported: 1 for (64, 128, 64, 8, 8, HW % 16 == 0, FRL_BF16), else compose
 * frl_conv1x1_* / frl_groupnorm_*.  stats [B][32] f32 = mean1[8] rstd1[8] mean2[8] rstd2[8].
 * Backward (parameters only: the encoder's input is data): dw1 [C1][C0], dw2 [C2][C1] and the GroupNorm parameter gradients; the chain
 * is recomputed per pass and the weight gradients are contracted inside the kernel, so no intermediate tensor reaches HBM. */
int frl_encoder2_supported(int C0, int C1, int C2, int G1, int G2, int HW, int dtype);
size_t frl_encoder2_workspace_bytes(int B);
int frl_encoder2_fwd(const void* x, const float* w1, const float* g1, const float* b1, const float* w2, const float* g2, const float* b2,
                     void* z, float* stats, int B, int HW, float eps, void* ws, size_t ws_bytes, frl_stream_t stream);
int frl_encoder2_bwd(const void* x, const void* dz, const float* w1, const float* g1, const float* b1, const float* w2, const float* g2,
                     const float* b2, const float* stats, float* dw1, float* dg1, float* db1, float* dw2, float* dg2, float* db2,
                     int B, int HW, void* ws, size_t ws_bytes, frl_stream_t stream);

/* ---- EdgeAwareSmoothingConv2D fixed stencils -------------------------------------------------------------------
 * Sobel/4 depthwise gradients (frl/models/spatial.py:240-249,295-296): g [B][H][W][2C] = cat[dx, dy]. */
int frl_sobel_fwd(const void* x, void* g, int B, int H, int W, int C, int dtype, frl_stream_t stream);
int frl_sobel_bwd(const void* dg, void* dx, int B, int H, int W, int C, int dtype, frl_stream_t stream);
/* dx = sobel^T(dg) + dx_add (dx_add [B][H][W][C] or null): x also feeds the filter bank, whose dx arrives through dx_add */
int frl_sobel_bwd_add(const void* dg, void* dx, const void* dx_add, int B, int H, int W, int C, int dtype, frl_stream_t stream);
/* A/B hook: 1 (default) = bf16 Sobel calls whose image row is one workgroup of 16-byte channel vectors (W * C / 8 == 256: 32 x 64) take the
 * row-band streaming kernels, 0 = every call takes the gather kernels; same bits either way.  Returns the previous setting. */
int frl_sobel_stream(int on);
/* Tuning hook: rows per workgroup of the streaming route (1..64, default 8; other values change nothing).  Returns the previous height. */
int frl_sobel_stream_band(int rows);
/* directional bank + rank-R mixing (spatial.py:224-237,300-331): a_logit [P][8R] (k*R+r), b_logit [P][C*R] (c*R+r);
 * outputs smoothed, residual = x - smoothed, and the softmaxed maps a_soft / b_soft saved for the backward. */
int frl_edge_smooth_stencil_fwd(const void* x, const void* a_logit, const void* b_logit, void* smoothed, void* residual,
                                void* a_soft, void* b_soft, int B, int H, int W, int C, int R, int coarse_dilation,
                                int dtype, frl_stream_t stream);
int frl_edge_smooth_stencil_bwd(const void* d_smoothed, const void* x, const void* a_soft, const void* b_soft, void* dx,
                                void* da_logit, void* db_logit, const void* dx_add /* optional: added to dx in the store */, int B, int H,
                                int W, int C, int R, int coarse_dilation, int dtype, frl_stream_t stream);
/* Fused mixing heads + softmaxes + directional bank for the hot configuration (bf16, C = 64, 64 hidden features, rank 4; replaces
 * mix_head_A / mix_head_B (nn.Conv2d 1x1, spatial.py:262-263), the two softmaxes (:300-307) and the bank + mix (:314-331) in one launch;
 * the [P,32] / [P,256] logits and their soft-maxed copies never reach memory).  feat = relu(mix_backbone(cat[dx,dy])) [B][H][W][64];
 * wa [32][64], ba [32], wb [256][64], bb [256] float32 with output channels k*R+r resp. c*R+r. */
int frl_smooth_heads_supported(int C, int hidden, int rank, int dtype);
size_t frl_smooth_heads_workspace_bytes(int64_t npix);
int frl_smooth_heads_fwd(const void* x, const void* feat, const float* wa, const float* ba, const float* wb, const float* bb,
                         void* smoothed, void* residual, int B, int H, int W, int coarse_dilation, void* ws, size_t ws_bytes,
                         frl_stream_t stream);
/* backward: d_smoothed already carries the residual path (d smoothed - d residual); dx_add (optional) is added to dx.  The heads are
 * recomputed from feat; outputs dx, dfeat [P][64] (bf16) and the four head parameter gradients (float32).  scratch: exchange tensors of
 * the two launches (u = ds * softmax B [P][256], softmax A [P][32], bf16), frl_smooth_heads_bwd_scratch_bytes(npix) bytes. */
size_t frl_smooth_heads_bwd_scratch_bytes(int64_t npix);
int frl_smooth_heads_force_gather(int on);     /* test hook: d x of the backward by the gather kernel instead of the LDS-tiled one; returns the previous setting */
int frl_smooth_heads_bwd(const void* d_smoothed, const void* x, const void* feat, const float* wa, const float* ba, const float* wb,
                         const float* bb, const void* dx_add, void* dx, void* dfeat, float* dwa, float* dba, float* dwb, float* dbb,
                         void* scratch, size_t scratch_bytes, int B, int H, int W, int coarse_dilation, void* ws, size_t ws_bytes,
                         frl_stream_t stream);
/* The same with dfeat_relu != 0: dfeat is returned multiplied by [feat > 0] (feat is the output of the ReLU convolution mix_backbone,
 * spatial.py:258-261), so that convolution's backward-data / backward-weight calls take it with act = FRL_ACT_NONE. */
int frl_smooth_heads_bwd_masked(const void* d_smoothed, const void* x, const void* feat, const float* wa, const float* ba, const float* wb,
                                const float* bb, const void* dx_add, void* dx, void* dfeat, float* dwa, float* dba, float* dwb, float* dbb,
                                void* scratch, size_t scratch_bytes, int B, int H, int W, int dil, int dfeat_relu, void* ws,
                                size_t ws_bytes, frl_stream_t stream);
/* ---- FiLM conditioning of the phase path, fused (bf16, 64 conditioning channels, hidden 32, 12 target channels) ----------------------
 * Replaces FiLMLayer.forward (frl/models/conditioning.py:82-102: two conv1x1 -> ReLU -> conv1x1 nets) and the modulation
 * gamma * h + beta broadcast over T (frl/models/representation.py:369-372) with one launch per direction.  z_type [B][HW][64] is a
 * stop-gradient input (representation.py:350-351); h, z, dz, dh [B][T][HW][12]; gamma, beta [B][HW][12]; w1* [32][64], w2* [12][32]. */
int frl_film_fused_supported(int cond_dim, int hidden, int target_dim, int dtype);
size_t frl_film_fused_workspace_bytes(void);
int frl_film_fused_fwd(const void* z_type, const void* h, const float* w1g, const float* b1g, const float* w2g, const float* b2g,
                       const float* w1b, const float* b1b, const float* w2b, const float* b2b, void* z, void* gamma, void* beta, int B,
                       int T, int HW, void* ws, size_t ws_bytes, frl_stream_t stream);
int frl_film_fused_bwd(const void* z_type, const void* h, const void* dz, const float* w1g, const float* b1g, const float* w2g,
                       const float* b2g, const float* w1b, const float* b1b, const float* w2b, const float* b2b, void* dh, float* dw1g,
                       float* db1g, float* dw2g, float* db2g, float* dw1b, float* db1b, float* dw2b, float* db2b, int B, int T, int HW,
                       void* ws, size_t ws_bytes, frl_stream_t stream);
/* out = smoothed + max(gate_raw, min_gate) * residual (spatial.py:333-335); n = element count */
int frl_gate_blend_fwd(const void* smoothed, const void* residual, const void* gate_raw, float min_gate, void* out,
                       void* gate_out, int64_t n, int dtype, frl_stream_t stream);
/* d_residual may be null (both forms): only d_gate_raw is stored then (frl_conv3x3_bwd_data_blend forms d_residual itself). */
int frl_gate_blend_bwd(const void* dout, const void* dgate_ext, const void* residual, const void* gate_raw, float min_gate,
                       void* d_residual, void* d_gate_raw, int64_t n, int dtype, frl_stream_t stream);
/* The same with sigmoid_mask != 0: d_gate_raw is returned multiplied by gate_raw (1 - gate_raw), the derivative of the sigmoid that produced
 * gate_raw (gate_net, spatial.py:266-272): the convolution's backward calls take it with act = FRL_ACT_NONE. */
int frl_gate_blend_bwd_masked(const void* dout, const void* dgate_ext, const void* residual, const void* gate_raw, float min_gate,
                              void* d_residual, void* d_gate_raw, int64_t n, int dtype, int sigmoid_mask, frl_stream_t stream);

/* ---- fused TCN GatedResidualBlock ------------------------------------------------------------------------------
 * frl/models/tcn.py:78-111 on x [B][T][HW][Cin] (npix = B*HW); conv_w [Cout][Cin][3], gate_w [Cout][Cout],
 * proj_w [Cout][Cin] or NULL (identity residual, tcn.py:71-76). */
int frl_tcn_block_fwd(const void* x, const float* conv_w, const float* conv_b, const float* gn_w, const float* gn_b,
                      const float* gate_w, const float* gate_b, const float* proj_w, const float* proj_b, void* y,
                      int64_t npix, int HW, int T, int Cin, int Cout, int dilation, int G, float eps, int dtype, void* ws,
                      size_t ws_bytes, frl_stream_t stream);
size_t frl_tcn_block_bwd_workspace_bytes(int64_t npix, int Cout);
int frl_tcn_block_bwd(const void* x, const void* dy, const float* conv_w, const float* conv_b, const float* gn_w,
                      const float* gn_b, const float* gate_w, const float* gate_b, const float* proj_w,
                      const float* proj_b, void* dconv, void* dgpre, void* normed, void* dres, float* dgamma, float* dbeta,
                      int64_t npix, int HW, int T, int Cin, int Cout, int dilation, int G, float eps, int dtype, void* ws,
                      size_t ws_bytes, frl_stream_t stream);
int frl_tcn_block_bwd_data(const void* dconv, const void* dres, const float* conv_w, const float* proj_w, void* dx,
                           int64_t npix, int HW, int T, int Cin, int Cout, int dilation, int dtype, void* ws, size_t ws_bytes,
                           frl_stream_t stream);

/* fully fused backward (bf16, Cin = Cout = 64, T <= 5, identity residual): one launch reads x, dy and writes dx and every
 * parameter gradient of the block; weight gradients are contracted inside the kernel (no HBM side outputs). */
int frl_tcn_block_bwd_fused_supported(int T, int Cin, int Cout, int G, int has_proj, int dtype);
size_t frl_tcn_block_bwd_fused_workspace_bytes(int64_t npix);
int frl_tcn_block_bwd_fused(const void* x, const void* dy, const float* conv_w, const float* conv_b, const float* gn_w,
                            const float* gn_b, const float* gate_w, const float* gate_b, void* dx, float* d_conv_w,
                            float* d_conv_b, float* d_gn_w, float* d_gn_b, float* d_gate_w, float* d_gate_b, int64_t npix,
                            int HW, int T, int dilation, int G, float eps, void* ws, size_t ws_bytes, frl_stream_t stream);

/* ---- deferred weight-gradient reductions (csrc/defer.hip) -------------------------------------------------------------------------
 * Every weight-gradient kernel leaves per-workgroup float32 slabs that a small fixed-order reduction turns into the gradient tensors.
 * Between frl_defer_begin() and frl_defer_flush(stream) those reductions (of frl_tcn_hot_bwd, frl_conv3x3_bwd_weight,
 * frl_decoder_mse_bwd, frl_encoder2_bwd, frl_film_fused_bwd, frl_smooth_heads_bwd, frl_conv1x1_bwd_weight and frl_vq_bwd without per-code
 * sums -- whose epilogue reads `counts`, the codebook and `gscale` when it runs: those three stay alive and unchanged until the flush;
 * calls that cut their output channels into several slices are not deferred) are parked and the flush runs them all in ONE launch: same summation order, bit-identical gradients, ~12 launches fewer per
 * train step.  The caller owns two promises: the workspaces handed to the deferred calls stay untouched until the flush (hand every
 * call its own), and nothing reads the gradient tensors before it.  frl_defer_destinations lists the gradient pointers of the parked
 * jobs so that the caller can check they still are the tensors its optimizer reads.  Process-wide state (any thread's calls are
 * parked); at most 24 jobs, further ones run undeferred.  frl_defer_flush returns the number of jobs run. */
int frl_defer_begin(void);
int frl_defer_pending(void);
int frl_defer_destinations(void** out, int max);
int frl_defer_flush(frl_stream_t stream);
int frl_defer_abort(void);

/* hot-configuration block kernels (bf16, Cin = Cout = 64, T = 5, G = 8, identity residual, dilation 1/2/4: the three phase-path
 * blocks of configs/vae_v0.yaml): (T, dilation) are compile-time, the pixel's time series stays in registers, the temporal
 * conv is evaluated once per tile.  frl_tcn_hot_bwd is one launch for dx + every parameter gradient (tcn.py:78-111). */
int frl_tcn_hot_supported(int T, int Cin, int Cout, int G, int dilation, int has_proj, int dtype);
size_t frl_tcn_hot_fwd_workspace_bytes(void);
size_t frl_tcn_hot_bwd_workspace_bytes(int64_t npix);
/* drop_mask: NULL, or the training-mode Dropout1d mask of the block (tcn.py:53) as [B][HW][64] bf16 holding 0 or 1/(1-p) per
 * (pixel series, channel): the temporal conv sees x .* mask, the residual path the untouched x (tcn.py:89-90). */
int frl_tcn_hot_fwd(const void* x, const void* drop_mask, const float* conv_w, const float* conv_b, const float* gn_w, const float* gn_b,
                    const float* gate_w, const float* gate_b, void* y, int64_t npix, int HW, int dilation, float eps, void* ws,
                    size_t ws_bytes, frl_stream_t stream);
/* 1: frl_tcn_hot_bwd takes dx = NULL for this shape (block input without gradient: no conv^T GEMM, no dx store; drop_mask must be NULL) */
int frl_tcn_hot_bwd_nodx_supported(int64_t npix, int HW);
int frl_tcn_hot_bwd(const void* x, const void* drop_mask, const void* dy, const float* conv_w, const float* conv_b, const float* gn_w,
                    const float* gn_b, const float* gate_w, const float* gate_b, void* dx, float* d_conv_w, float* d_conv_b,
                    float* d_gn_w, float* d_gn_b, float* d_gate_w, float* d_gate_b, int64_t npix, int HW, int dilation,
                    float eps, void* ws, size_t ws_bytes, frl_stream_t stream);
/* The dense phase chain forward in ONE launch (hot configuration, three blocks with dilation 1, 2, 4: TCNEncoder.forward, tcn.py:242-290)
 * followed by the 1x1 phase head (representation.py:169,362-366): x [B][5][HW][64] -> y1, y2, y3 (the blocks' outputs, kept for the
 * backward) and h [B][5][HW][Ch] = head_w y3 + head_b, Ch in {4, 8, 12, 16}.  conv_w .. gate_b: arrays of three pointers (block 0, 1, 2). */
size_t frl_tcn_chain_fwd_workspace_bytes(void);
int frl_tcn_chain_static_tiles(int on);   /* A/B hook: 1 = fixed tile sequence per wave, 0 (default) = tiles handed out by an LDS counter; returns the previous setting */
int frl_tcn_chain_fwd(const void* x, const float* const* conv_w, const float* const* conv_b, const float* const* gn_w,
                      const float* const* gn_b, const float* const* gate_w, const float* const* gate_b, const float* head_w,
                      const float* head_b, void* y1, void* y2, void* y3, void* h, int64_t npix, int HW, int Ch, float eps, void* ws,
                      size_t ws_bytes, frl_stream_t stream);
/* y1 = y2 = y3 = NULL: inference variant of the same launch (h only, bitwise the same h); a mix of NULL and non-NULL is an argument error. */
/* The same launch with the side output xt [B][HW][64] bf16 = mean over t of x, bit for bit what frl_mean_time_fwd writes: the tile is
 * in registers there anyway, so the train step needs no separate pass over it.  xt = NULL: frl_tcn_chain_fwd. */
int frl_tcn_chain_fwd_xt(const void* x, const float* const* conv_w, const float* const* conv_b, const float* const* gn_w,
                         const float* const* gn_b, const float* const* gate_w, const float* const* gate_b, const float* head_w,
                         const float* head_b, void* y1, void* y2, void* y3, void* h, void* xt, int64_t npix, int HW, int Ch, float eps,
                         void* ws, size_t ws_bytes, frl_stream_t stream);
/* The last block of the phase encoder together with the backward-data of the 1x1 phase head behind it (representation.py:169): `dh`
 * [B][5][HW][Ch] bf16 is the head's output gradient, head_w [Ch][64] float32, Ch in {4, 8, 12, 16}; dy = dh head_w is formed inside the
 * kernel on the matrix cores (float32, never written).  Same outputs as frl_tcn_hot_bwd; needs the two-subgroup kernel: no mask,
 * HW % 64 == 0, dilation 4, dx != NULL.  Workspace: frl_tcn_hot_bwd_head_workspace_bytes(npix). */
int frl_tcn_hot_bwd_head_supported(int64_t npix, int HW, int Ch);
size_t frl_tcn_hot_bwd_head_workspace_bytes(int64_t npix);
int frl_tcn_hot_bwd_head(const void* x, const void* dh, const float* head_w, int Ch, const float* conv_w, const float* conv_b,
                         const float* gn_w, const float* gn_b, const float* gate_w, const float* gate_b, void* dx, float* d_conv_w,
                         float* d_conv_b, float* d_gn_w, float* d_gn_b, float* d_gate_w, float* d_gate_b, int64_t npix, int HW,
                         int dilation, float eps, void* ws, size_t ws_bytes, frl_stream_t stream);
/* Two kernels stand behind frl_tcn_hot_bwd: tcn_hot_bwd4_kernel (no mask, HW a multiple of 64: two independent 4-wave subgroups per
 * workgroup, each staging x of its 32-pixel tiles once in LDS by LDS-DMA with the next tile prefetched) and tcn_hot_bwd2_kernel, the
 * 8-wave kernel that also takes a mask and ragged pixel counts.  They agree up to the bf16 rounding of dx and of dres inside.  Test hook: on != 0
 * routes every call through the latter so that the two can be compared on the same inputs. */
int frl_tcn_hot_force_generic_tiles(int on);   /* returns the previous setting */
/* Tuning hook of tcn_hot_bwd4: subgroup 0's share (in 32nds, 1..31) of a workgroup's tiles for variant 0 (with dx), 1 (without dx), 2 (head);
 * returns the previous value (share outside 1..31: query only).  Any value gives the same gradients up to float32 summation order. */
int frl_tcn_hot_bwd4_share(int variant, int share);

/* ---- optimizer step (frl/training/representation/step.py:1081-1087: clip_grad_norm_(1.0) then AdamW.step()) ---------------
 * Two launches for the whole parameter set.  desc: HOST table of ntensors records {float* p; const float* g; float* m; float* v;
 * int64_t n; float weight_decay; int slot} (48 bytes; slot = the tensor's entry in tensor_steps) -- it travels in the kernel-argument
 * segment, so moved gradient buffers cost no copy or sync; chunks: DEVICE table of nchunks int32 pairs {tensor index,
 * 4096-element window} sorted by tensor, chunk_tensor: its tensor column on the HOST.  step is the 1-based update count (bias
 * corrections in float64 as torch.optim.AdamW); max_norm <= 0 disables clipping; norm_out (device float, may be NULL) receives
 * the pre-clip global gradient norm.  ok (device float, may be NULL): the reference's isfinite guard evaluated ON THE DEVICE --
 * ok[0] <= 0 leaves parameters and moments untouched; counters (device int[2], may be NULL) = {updates applied, updates skipped},
 * and when given, counters[0] + 1 replaces `step` as the update number (exact under skipped batches, no host sync).
 * tensor_steps (device int [nsteps], may be NULL): per-tensor update counts as torch.optim.AdamW's state["step"].  The step bumps
 * entry `slot` of every record when -- and only when -- the device applies the update, and the bias corrections of that tensor use the
 * entry; slots must be distinct and in [0, nsteps).  A tensor outside the table, a skipped batch and a graph replay leave it exact.
 * lr_dev (device float, may be NULL): when given, lr_dev[0] replaces `lr` -- the learning rate of a train step captured in a
 * hipGraph is written to that word before every replay (per-batch scheduler.step() of loops.py:110 without re-capturing). */
size_t frl_adamw_workspace_bytes(void);
int frl_adamw_clip_step(const void* desc_host, int ntensors, const void* chunks, const int* chunk_tensor, int nchunks, float max_norm,
                        float lr, double beta1, double beta2, float eps, int step, float* norm_out, const float* ok, int* counters,
                        const float* lr_dev, int* tensor_steps, int nsteps, void* ws, size_t ws_bytes, frl_stream_t stream);
/* dst[i] = scale * src[i] over a HOST table of {const float* src; float* dst; int64_t n} records (24 bytes; src NULL -> zeros):
 * flattens the scattered gradients of a bucket for the data-parallel all-reduce in one launch. */
int frl_multi_tensor_scale_copy(const void* desc_host, int ntensors, const void* chunks, const int* chunk_tensor, int nchunks, float scale,
                                frl_stream_t stream);

/* ---- FiLM modulation, time mean, add ---------------------------------------------------------------------------
 * z = gamma * h + beta broadcast over T (frl/models/representation.py:369-372); h [B][T][HW][C], gamma [B][HW][C]. */
int frl_film_modulate_fwd(const void* h, const void* gamma, const void* beta, void* out, int64_t B, int T, int64_t HW,
                          int C, int dtype, frl_stream_t stream);
int frl_film_modulate_bwd(const void* dout, const void* h, const void* gamma, void* dh, void* dgamma, void* dbeta,
                          int64_t B, int T, int64_t HW, int C, int dtype, frl_stream_t stream);
int frl_mean_time_fwd(const void* tile, void* out, int64_t B, int T, int64_t HWC, int dtype, frl_stream_t stream);
int frl_add(const void* a, const void* b, float scale_b, void* out, int64_t n, int dtype, frl_stream_t stream); /* out = a + scale_b*b */

/* ---- tile ingest: chunk-store rows -> normalised training rows -------------------------------
 * Replaces the per-channel numpy normalisation + masking of FeatureBuilder on the host
 * (frl/data/loaders/builders/feature_builder.py:402-462 _apply_normalization, :487-548 _normalize_array, :709-737
 * _apply_mask_to_data; presets of frl/data/normalization/normalization.py:116-254) by one pass on the device over the
 * (time,y,x,feature) rows as stored (utils/data_stack.py:271-309).  Per feature f:
 *     r = (x - sub) / div;  if (flags & 1) r = r * mul + add;  if (flags & 2) r = max(r, lo);  if (flags & 4) r = min(r, hi)
 * (float32, that operation order, no fused multiply-add).  A row is valid iff valid[row] != 0 (when given) and all its F raw
 * values are finite; invalid rows are written as zeros and mask_out[row] = 0.
 * raw [rows][F] FRL_F32 | FRL_F16, table [F] device records, out [rows][F] FRL_F32 | FRL_BF16, F in {8,16,...,512}. */
typedef struct FrlNormRec {
  float sub, div, mul, add, lo, hi;
  int flags; /* 1 rescale, 2 clamp below, 4 clamp above */
  int pad;
} FrlNormRec;
int frl_normalize_tiles(const void* raw, int raw_dtype, const uint8_t* valid, const void* table, void* out, int out_dtype,
                        uint8_t* mask_out, int64_t rows, int F, frl_stream_t stream);
/* Same arithmetic with the tile cut done on the device: `chunk` is one whole stored chunk [T][CY][CX][F] (uploaded with ONE
 * contiguous copy; batches are chunk-locked, utils/samplers.py:42-108), desc [ntiles] = int32 {y0, x0, h, w} per tile (device).
 * Replaces the window read + zero padding of partial patches on the host (forest_dataset_v2.py:328-369): rows/columns beyond
 * h/w are written as zeros with mask 0.  out [ntiles][T][tile][tile][F], mask_out [ntiles][T][tile][tile]. */
int frl_normalize_chunk_tiles(const void* chunk, int raw_dtype, int T, int CY, int CX, int F, const int32_t* desc, int ntiles,
                              int tile, const void* table, void* out, int out_dtype, uint8_t* mask_out, frl_stream_t stream);

/* Host-side helper of the tile loader: multi-threaded memcpy of one stored chunk into the pinned upload buffer (no GPU work). */
int frl_host_parallel_copy(void* dst, const void* src, size_t nbytes, int nthreads);

/* ---- masked L2 reconstruction loss -----------------------------------------------------------------------------
 * frl/losses/reconstruction.py:95-139 (loss_type "l2", reduction "mean"); out = {mean, n_valid_elements}. */
size_t frl_mse_workspace_bytes(void);
int frl_mse_fwd(const void* pred, const void* target, const uint8_t* mask, int64_t P, int C, float* out, int dtype,
                void* ws, size_t ws_bytes, frl_stream_t stream);
int frl_mse_bwd(const void* pred, const void* target, const uint8_t* mask, const float* gscale, const float* stats,
                int64_t P, int C, void* dpred, int dtype, frl_stream_t stream);

/* fused decoder + loss (bf16, hidden 128, 64 features, latent <= 64 ch): xhat = W2 relu(W1 z + b1) + b2, L = mean_valid (xhat - x)^2.
 * Replaces the conv1x1 -> ReLU -> conv1x1 -> reconstruction_loss chain (heads.py:128-198 template, reconstruction.py:95-139) and its
 * backward with two launches; the hidden tensor and xhat stay on chip (xhat is written only when a buffer is passed). */
int frl_decoder_mse_fused_supported(int Cz, int hidden, int F, int dtype);
size_t frl_decoder_mse_workspace_bytes(int64_t P, int Cz);
int frl_decoder_mse_fwd(const void* z, const float* w1, const float* b1, const float* w2, const float* b2, const void* target,
                        const uint8_t* mask, void* xhat, float* out, int64_t P, int Cz, void* ws, size_t ws_bytes,
                        frl_stream_t stream);
int frl_decoder_mse_bwd(const void* z, const float* w1, const float* b1, const float* w2, const float* b2, const void* target,
                        const uint8_t* mask, const float* gscale, const float* stats, void* dz, float* dw1, float* db1,
                        float* dw2, float* db2, int64_t P, int Cz, void* ws, size_t ws_bytes, frl_stream_t stream);
/* Train step: loss AND gradients from ONE pass over (z, target).  The backward kernel recomputes all the forward computes, so when the
 * gradient the loss will receive is known before the forward runs (gscale: device scalar, null = 1; the loss enters the total with a fixed
 * coefficient and the total is differentiated with upstream 1) it also accumulates the loss: no forward kernel, one pass over the data less.
 * out = {loss, n_valid} and dz are what frl_decoder_mse_fwd / frl_decoder_mse_bwd write (dz and the weight gradients bit for bit).  The
 * weight-gradient slabs stay unreduced in `buf` (frl_decoder_mse_onepass_bytes; the caller's own, untouched until the reduction has run)
 * and *nslab receives their number; frl_decoder_mse_reduce turns them into dw1 [128][Cz], db1 [128], dw2 [64][128], db2 [64] -- parked
 * when a deferral is open (csrc/defer.hip), a launch of its own otherwise.  ctl: 4 zeroed 32-bit device words that no concurrent call
 * shares (used by the mask count); every call leaves them zero.  With a mask, n_valid comes from a count over the mask bytes (one small
 * launch in front of the pass); the loss record is written by the small finalize launch behind it. */
size_t frl_decoder_mse_onepass_bytes(int64_t P, int Cz);
int frl_decoder_mse_fwd_bwd(const void* z, const float* w1, const float* b1, const float* w2, const float* b2, const void* target,
                            const uint8_t* mask, const float* gscale, float* out, void* dz, void* buf, size_t buf_bytes, void* ctl,
                            int* nslab, int64_t P, int Cz, frl_stream_t stream);
int frl_decoder_mse_reduce(const void* buf, int nslab, float* dw1, float* db1, float* dw2, float* db2, int Cz, frl_stream_t stream);
int frl_decoder_mse_bwd_subgroups(int on);   /* A/B hook: 1 (default) = two independent 4-wave subgroups per workgroup, 0 = lockstep workgroups; returns the previous setting */

/* ---- vector quantizer ------------------------------------------------------------------------------------------
 * Not in the reference tree; constants frl/config/frl_model_v0.yaml:29-35,
 * scripts/train_vqvae.py:410-436.  idx bit-exact vs float64 argmin (first index on ties). */
size_t frl_vq_workspace_bytes(int64_t N, int K, int d);
int frl_vq_assign_fwd(const void* z, const float* E, int64_t N, int K, int d, int32_t* idx_out, void* zq_out,
                      float* stats_out, int32_t* counts_out, int dtype, void* ws, size_t ws_bytes, frl_stream_t stream);
/* Prepared codebook (||e||^2 + the packed MFMA fragment image of -2 e): it depends on the codebook content and dtype only, so a
 * caller that knows when the codebook changes (once per optimizer step; never during inference) builds it once and the assignment
 * itself is ONE kernel launch with nothing to zero beforehand: arg-min on the matrix cores, exact float64 re-evaluation of near-ties
 * while the codebook is still in LDS, z_q, squared error, code histogram (integer atomics) and the statistics (folded by the workgroup
 * that arrives last) -- when the codebook fits one LDS chunk (K * d_pad * sizeof(dtype) <= 64 KB), else as frl_vq_assign_fwd.
 * The image also holds the kernel's arrival counter and histogram accumulator (zeroed by frl_vq_prepare and left zeroed by every
 * call), so at most ONE assignment may be in flight per prepared image. */
size_t frl_vq_prepared_bytes(int K, int d);
/* A/B hook for the resident-codebook assignment of bf16 rows with d = 64 whose row count is a whole number of batches: nt = 1 / 2 / 4
 * selects the streaming kernel (one 16-wave workgroup per CU, 16 * nt * 16 rows per batch, no workgroup barrier in the batch loop),
 * 0 the kernel of round 2, -1 the default (environment variable FRL_VQ_STREAM, else the built-in choice).  Returns the previous
 * setting; outputs are the same bit for bit (the squared-error sum up to float32 summation order). */
int frl_vq_stream_tiles(int nt);
int frl_vq_prepare(const float* E, int64_t N, int K, int d, int dtype, void* prep, size_t prep_bytes, frl_stream_t stream);
int frl_vq_assign_fwd_prepared(const void* z, const float* E, void* prep /* NULL: prepare inside the call */, int64_t N, int K, int d,
                               int32_t* idx_out, void* zq_out, float* stats_out, int32_t* counts_out, int dtype, void* ws,
                               size_t ws_bytes, frl_stream_t stream);
/* As frl_vq_assign_fwd_prepared; stats_copy (NULL or 4 floats): the kernel that writes stats_out stores the same record there too, for a
 * caller that differentiates its own copy of the statistics (no device-to-device copy behind the call). */
int frl_vq_assign_fwd_stats2(const void* z, const float* E, void* prep, int64_t N, int K, int d, int32_t* idx_out, void* zq_out,
                             float* stats_out, float* stats_copy, int32_t* counts_out, int dtype, void* ws, size_t ws_bytes,
                             frl_stream_t stream);
/* The prepared image as a job of the weight-image cache `handle`: every frl_pack_cache_refresh(handle) then rewrites `prep` (norms,
 * fragments, zeroed control block) from E inside its one launch, by the device functions frl_vq_prepare runs -- the same bits.  A caller
 * that refreshes right behind every codebook update launches no frl_vq_prepare of its own; E and prep outlive the cache, and no
 * assignment is in flight on the image while the refresh runs.  Registering the same image twice changes nothing. */
int frl_pack_cache_add_vq(int handle, const float* E, int K, int d, int dtype, void* prep, size_t prep_bytes);
/* Returns -2 for N, K or d <= 0, for bf16 rows with d > 128 (the widest matrix-core instance covers 128 channels, as the forward), and for
 * float32 rows when one code row (d * 4 bytes) exceeds the 96 KiB LDS chunk. */
int frl_vq_bwd(const void* g_out, const void* z, const void* zq /* optional */, const float* E, const int32_t* idx, const int32_t* counts,
               const float* gscale, float beta, int64_t N, int K, int d, void* g_z_out, float* g_E_out, float* sums_out,
               int dtype, void* ws, size_t ws_bytes, frl_stream_t stream);
/* As frl_vq_bwd with the two upstream gradients as two device scalars (g_commit of L_commit, g_codebook of L_codebook) that need not be
 * adjacent.  NULL means that NO gradient arrives for that term: its factor is formed as coefficient * 0, the bits a zero scalar gives
 * (a NULL gscale of frl_vq_bwd means {1, 1}).  Deferred: g_codebook stays alive and unchanged until the flush. */
int frl_vq_bwd_scalars(const void* g_out, const void* z, const void* zq /* optional */, const float* E, const int32_t* idx,
                       const int32_t* counts, const float* g_commit, const float* g_codebook, float beta, int64_t N, int K, int d,
                       void* g_z_out, float* g_E_out, float* sums_out, int dtype, void* ws, size_t ws_bytes, frl_stream_t stream);
/* ok: NULL, or a device float -- ok[0] <= 0 (or NaN) skips the update on the device (the train step's isfinite guard, evaluated
 * without a host synchronisation; frl/training/representation/step.py:1057-1074 "skip the batch"). */
int frl_vq_ema_update(const float* sums, const int32_t* counts, int K, int d, float decay, float eps, float* ema_count,
                      float* ema_sum, float* E, const float* ok, frl_stream_t stream);
/* Dead-code revival of the legacy trainer's CodebookManager (scripts/train_vqvae.py:92,196-198 constructs and attaches it; the
 * module is not in the reference tree -- build definition): codes with window_counts[k] < min_count are re-seeded with the
 * encoder row z[splitmix64(seed + k) mod N], their AdamW moment rows m / v (optional) are cleared, *revived += number of codes. */
int frl_vq_revive_dead_codes(float* E, const int64_t* window_counts, int64_t min_count, const void* z, int64_t N, int K, int d,
                             uint64_t seed, float* m, float* v, int32_t* revived, int dtype, frl_stream_t stream);

/* ---- sparse-location gather + InfoNCE over mined pairs (csrc/contrastive.hip) -----------------------------
 * frl_gather_locations_fwd: extract_at_locations of frl/utils/spatial.py:132-173 -- out[n][c] = feat[c*sC + row_n*sH + col_n*sW] for
 * coords [N][2] int64 (row, col; negative counts from the end), any element strides (NHWC rows and the reference's [C,H,W] view alike).
 * frl_segment_sum_rows: out[key][:] (+)= sum over each run of equal keys_sorted of vals[order[i]][:], rows added in list order -- the
 * bit-reproducible scatter-add behind both backward passes (order NULL = identity).
 * frl_infonce_fwd / frl_infonce_pair_grads: contrastive_loss of frl/losses/contrastive.py:29-212 over T pairs SORTED by anchor
 * (pairs [T][2] int64 rows of emb [.][D] f32, weights [T] or NULL, is_pos [T] bytes, seg [nseg+1] segment bounds; similarity 0 = l2
 * (-|a-b|^2/D), 1 = cosine, 2 = dot): per-anchor loss_a = -log(sum_pos + 1e-8) + log(sum_all + 1e-8) relative to the anchor's largest
 * logit, loss[0] = mean; coef[p] = d loss_a / d logit_p; the gradient rows ga / gb [T][D] carry gscale[0] / (nseg * temperature). */
int frl_gather_locations_fwd(const void* feat, int64_t sC, int64_t sH, int64_t sW, int C, int H, int W, const int64_t* coords, int64_t N,
                             void* out, int dtype, frl_stream_t stream);
int frl_segment_sum_rows(const float* vals, const int64_t* order, const int64_t* keys_sorted, int64_t M, int D, float* out, int64_t out_stride,
                         int accumulate, frl_stream_t stream);
int frl_infonce_fwd(const float* emb, int D, const int64_t* pairs, const float* weights, const unsigned char* is_pos, int64_t T,
                    const int64_t* seg, int64_t nseg, float temperature, int similarity, float* sims, float* logits, float* loss_a, float* coef,
                    float* loss, frl_stream_t stream);
int frl_infonce_pair_grads(const float* emb, int D, const int64_t* pairs, const float* sims, const float* coef, const float* gscale, int64_t T,
                           int64_t nseg, float temperature, int similarity, float* ga, float* gb, frl_stream_t stream);

/* ---- VICReg variance-covariance loss (csrc/vicreg.hip) ----------------------------------------------------------------------
 * variance_covariance_loss of frl/losses/variance_covariance.py:14-88 over rows x [N][D] (dtype 0 = float32, 1 = bfloat16; N >= 2,
 * 1 <= D <= 128; f32 statistics): cov = Xc^T Xc / (N-1) with the moments taken about a pivot p = the mean of the first min(N, 64) rows
 * (no cancellation against the mean), losses [3] = (total, variance_loss, covariance_loss).  cov [D][D] and centre [2][D] = p | mean - p
 * are written when both are non-NULL (a gradient is wanted) and are what frl_vicreg_bwd reads:  dx = ((x - p) - (mean - p)) A,  A built on the device from cov and
 * g3 [3] = the upstream gradients of (total, variance_loss, covariance_loss); dx has the dtype of x.  No float atomics: both calls are
 * bit-reproducible.  Workspace: frl_vicreg_workspace_bytes(N, D). */
size_t frl_vicreg_workspace_bytes(int64_t N, int D);
int frl_vicreg_fwd(const void* x, int64_t N, int D, int dtype, float variance_weight, float covariance_weight, float variance_target,
                   float eps, float* losses, float* cov, float* centre, void* ws, size_t ws_bytes, frl_stream_t stream);
int frl_vicreg_bwd(const void* x, const float* cov, const float* centre, const float* g3, int64_t N, int D, int dtype, float variance_weight,
                   float covariance_weight, float variance_target, float eps, void* dx, frl_stream_t stream);

/* ---- soft-neighbourhood matching loss (csrc/soft_neighborhood.hip) -----------------------------------------------------------
 * soft_neighborhood_matching_loss of frl/losses/soft_neighborhood.py:46-208 (the two terms of phase_neighborhood_loss,
 * frl/losses/phase_neighborhood.py:458-630): per pair b and row t over the unmasked entries t' only, lp = log_softmax(-d_ref / tau_ref),
 * lq = log_softmax(-d_learned / tau_learned), kl = sum p (lp - lq); rows with fewer than min_valid unmasked entries are skipped,
 * L_b = mean kl over the rows_b contributing rows, loss = sum w_b L_b / sum w_b over the pairs with rows_b > 0 (0 when there is none or
 * the weights sum to 0).  The temperatures are passed as reciprocals.  pairstat [B][6] = L_b, rows_b, sum of the contributing rows'
 * unmasked counts, sum H(p), sum H(q), sum kl;  out2 [2] = loss, sum_w;  stats [8] doubles = loss, sum_w, active pairs, contributing
 * rows, sum of unmasked counts, sum H(p), sum H(q), 0.  Fixed reduction order, no float atomics: both forms are bit-reproducible.
 * Matrix form: d_ref, d_learned [B][M][M] f32, mask [B][M][M] bytes, weights [B] or NULL, any M >= 1; coef [B][M][M] (NULL = no gradient
 * wanted) = (p - q) / tau_learned, and frl_soft_nbr_bwd gives grad = gup[0] * w_b / (sum_w * rows_b) * coef (gup: device float).
 * Gathered form: the blocks are formed on chip from rows of ref [R][C] f32 and emb [R][D] (dtype 0 = float32, 1 = bfloat16):
 * d_ref[t][t'] = |ref[ref_rows_a[b][t]] - ref[ref_rows_b[b][t']]|_2, likewise emb; mask = t < K_b and t' < K_b (lengths [B] int64), minus
 * the diagonal when exclude_diagonal.  The four [B][M] int64 index arrays must lie in [0, R).  M <= 32, C <= 256, D <= 256.
 * frl_soft_nbr_gathered_bwd writes grad_rows [2][B][M][D] f32 (role a, then role b; zero where the distance is zero, torch.cdist's
 * convention, and beyond K_b) for frl_segment_sum_rows to fold into d emb. */
int frl_soft_nbr_fwd(const float* d_ref, const float* d_learned, const unsigned char* mask, const float* weights, int64_t B, int M,
                     float inv_tau_ref, float inv_tau_learned, int min_valid, float* pairstat, float* coef, float* out2, double* stats,
                     frl_stream_t stream);
int frl_soft_nbr_bwd(const float* coef, const float* pairstat, const float* weights, const float* out2, const float* gup, int64_t B, int M,
                     float* grad, frl_stream_t stream);
int frl_soft_nbr_gathered_fwd(const float* ref, int C, const void* emb, int D, int emb_dtype, const int64_t* ref_rows_a, const int64_t* ref_rows_b,
                              const int64_t* emb_rows_a, const int64_t* emb_rows_b, const int64_t* lengths, const float* weights, int64_t B, int M,
                              int exclude_diagonal, float inv_tau_ref, float inv_tau_learned, int min_valid, float* pairstat, float* out2,
                              double* stats, frl_stream_t stream);
int frl_soft_nbr_gathered_bwd(const float* ref, int C, const void* emb, int D, int emb_dtype, const int64_t* ref_rows_a, const int64_t* ref_rows_b,
                              const int64_t* emb_rows_a, const int64_t* emb_rows_b, const int64_t* lengths, const float* weights, int64_t B, int M,
                              int exclude_diagonal, float inv_tau_ref, float inv_tau_learned, int min_valid, const float* pairstat,
                              const float* out2, const float* gup, float* grad_rows, frl_stream_t stream);

/* ---- EVT soft-neighbourhood loss (csrc/evt_soft_neighborhood.hip) -------------------------------------------------------------
 * evt_soft_neighborhood_loss of frl/losses/evt_soft_neighborhood.py:266-440 for every segment (one sample's anchors) of emb [N][D]
 * (dtype 0 = float32, 1 = bfloat16, D <= 256) at once, all pairs of a segment, no [M][M] array in memory.  idx [N] int32 = the anchors'
 * code indices, -1 = unknown code (an idx >= K is treated as unknown and sets *index_flag to 1; the pointer may be NULL); S [K][K] f32 the
 * diffused similarity (not symmetric), w [K] f32 the code weights; seg [nseg + 1] int32 row offsets on the device and the same offsets
 * on the host, validated there (0 = seg[0] <= .. <= seg[nseg] = N, any length including 0; nseg <= 65535).  Anchor i is valid iff
 * idx[i] >= 0; pair (i, j) is in the mask iff both are valid and idx[i] != idx[j]; a row is active with >= 2 pairs; a_ij =
 * -(1 - S[idx_i][idx_j]) * inv_tau_ref, b_ij = -|e_i - e_j|_2 * inv_tau_learned, KL_i = KL(softmax_j a || softmax_j b) over the mask,
 * loss_s = sum w[idx_i] KL_i / W_s over the active rows (W_s = their weights); 0 with fewer than min_valid_anchors valid anchors or W_s <= 0.
 * rowstat [N][10] f32 = KL, log sum e^a, max b, log sum e^(b - max), H(p), H(q), pairs in the mask, confused pairs (1 - S < 1 - 1e-6),
 * sum of d over confused pairs, over the others.  segout [nseg][2] f32 = loss_s, W_s (0 when the segment contributes nothing).
 * segstat [nseg][12] f64 = loss_s, live, valid anchors, active rows, sum H(p), sum H(q), confused pairs of active rows, confused pairs,
 * sum d confused, sum d others, other pairs, W_s.  frl_evt_soft_nbr_bwd recomputes the distances and writes grad [N][D] in emb's dtype,
 * = gup[s] * seg_weights[s] (NULL = 1) * d loss_s / d emb, every row once (zero where a distance is zero: torch.cdist's convention).
 * Fixed reduction order, no float atomics: loss and gradients are bit-reproducible. */
int frl_evt_soft_nbr_fwd(const void* emb, int emb_dtype, int64_t N, int D, const int32_t* idx, const float* S, const float* w, int K,
                         const int32_t* seg, const int32_t* seg_host, int nseg, float inv_tau_ref, float inv_tau_learned, int min_valid_anchors,
                         float* rowstat, float* segout, double* segstat, int32_t* index_flag, frl_stream_t stream);
int frl_evt_soft_nbr_bwd(const void* emb, int emb_dtype, int64_t N, int D, const int32_t* idx, const float* S, const float* w, int K,
                         const int32_t* seg, const int32_t* seg_host, int nseg, float inv_tau_ref, float inv_tau_learned, const float* rowstat,
                         const float* segout, const float* gup, const float* seg_weights, void* grad, frl_stream_t stream);

/* ---- phase margin losses (csrc/phase_margin.hip) ------------------------------------------------------------------------------
 * The two remaining losses of the reference's cross-batch phase block (frl/training/representation/step.py:969-1006).  Distances are
 * d = |a - b|_2 from exact differences with a compensated float32 sum of squares; softplus is torch's (x > 20 ? x : log1p(exp(x))).
 * Recovery discrimination (phase_recovery_discrimination_loss, frl/losses/triplet_phase.py:352-426): z [N][T][D] (dtype 0 = float32,
 * 1 = bfloat16), ysfc [N][T] f32 (NaN, infinite or negative = invalid).  Per pixel low[t] = valid && ysfc <= low_ysfc_max, high[t] =
 * valid && ysfc >= high_ysfc_min, pairs = {(tl, th): low[tl] && high[th]}, d = sqrt(max(|z_tl - z_th|^2, 1e-12)),
 * loss = sum softplus(margin - d) / n_pairs over all pixels and pairs (0 without pairs).  partial [N][2] f32 = per-pixel sum, pair count;
 * out2 [2] = loss, n_pairs;  stats [4] doubles = loss, n_pairs, active pixels (both classes present), 0.  frl_recovery_disc_bwd recomputes
 * the distances and writes grad [N][T][D] in z's dtype = gup[0] (device float) * d loss / d z, every row once (zeros for inactive pixels,
 * without pairs, and from pairs whose sum of squares is under the clamp).  T <= 32, D <= 256.
 * Spread ranking (compute_phase_spread_ranking, frl/losses/phase_neighborhood.py:637-740): per pair b, n_b = max(1, unmasked entries),
 * spread_i = sum mask d_i / n_b, spread_j likewise, r_b = ref_diff [B] f32, term_b = softplus(spread_j - spread_i + margin) [r_b > delta]
 * + softplus(spread_i - spread_j + margin) [r_b < -delta], loss = sum term_b / B.  pairstat [B][3] = spread_i, spread_j, n_b;  out2 [2] =
 * loss, B;  stats [8] doubles = loss, pairs constrained with i the more dynamic, with j, satisfied constraints, sum spread_i, sum
 * spread_j, sum |r_b|, B.  Matrix form: d_i, d_j [B][M][M] f32, mask [B][M][M] bytes, any M >= 1; frl_spread_rank_bwd writes
 * grad_i = gup[0] c_b / (B n_b) on the unmasked entries (c_b = d term_b / d spread_i, 0 elsewhere) and grad_j = -grad_i.  Gathered form:
 * the blocks are the self-distances of the rows emb[rows_i[b][t]] and emb[rows_j[b][t]] of emb [R][D] (dtype 0 / 1), mask = t, t' < K_b
 * (lengths [B] int64, clamped into [0, M]) and t != t'; the [B][M] int64 index arrays must lie in [0, R); M <= 32, D <= 256.
 * frl_spread_rank_gathered_bwd writes grad_rows [2][B][M][D] f32 (role i, then role j; zero where a distance is zero, beyond K_b and
 * for unconstrained pairs) for frl_segment_sum_rows to fold into d emb.  Fixed reduction order, no float atomics: bit-reproducible. */
int frl_recovery_disc_fwd(const void* z, int dtype, const float* ysfc, int64_t N, int T, int D, float margin, float low_ysfc_max,
                          float high_ysfc_min, float* partial, float* out2, double* stats, frl_stream_t stream);
int frl_recovery_disc_bwd(const void* z, int dtype, const float* ysfc, int64_t N, int T, int D, float margin, float low_ysfc_max,
                          float high_ysfc_min, const float* out2, const float* gup, void* grad, frl_stream_t stream);
int frl_spread_rank_fwd(const float* d_i, const float* d_j, const unsigned char* mask, const float* ref_diff, int64_t B, int M, float margin,
                        float delta, float* pairstat, float* out2, double* stats, frl_stream_t stream);
int frl_spread_rank_bwd(const unsigned char* mask, const float* pairstat, const float* ref_diff, const float* gup, int64_t B, int M,
                        float margin, float delta, float* grad_i, float* grad_j, frl_stream_t stream);
int frl_spread_rank_gathered_fwd(const void* emb, int D, int emb_dtype, const int64_t* rows_i, const int64_t* rows_j, const int64_t* lengths,
                                 const float* ref_diff, int64_t B, int M, float margin, float delta, float* pairstat, float* out2,
                                 double* stats, frl_stream_t stream);
int frl_spread_rank_gathered_bwd(const void* emb, int D, int emb_dtype, const int64_t* rows_i, const int64_t* rows_j, const int64_t* lengths,
                                 const float* ref_diff, int64_t B, int M, float margin, float delta, const float* pairstat, const float* gup,
                                 float* grad_rows, frl_stream_t stream);

/* ---- code-map decoding (csrc/codes.hip) --------------------------------------------------------------------------------------
 * frl_decode_codes: out[p][:] = table[idx[p]][:] for a decoded-code table [K][F] (dtype 0 = float32, 1 = bfloat16; the VQ-VAE decoder
 * applied to the K codebook rows), idx [P] int32.  Indices in [-K, 0) wrap to idx + K; any other out-of-range index is clamped into
 * [0, K) and ORs 1 into *index_flag (may be NULL).  P = 0 is a no-op.  Argument errors (P < 0, K <= 0, F <= 0, bad dtype, a NULL
 * idx / table / out with P > 0) return a negative code before any HIP call.  16-byte copies whenever F * sizeof(T) is a multiple of 16. */
int frl_decode_codes(const int32_t* idx, const void* table, void* out, int64_t P, int K, int F, int dtype, int32_t* index_flag,
                     frl_stream_t stream);

/* ---- mutual k-nearest-neighbour pair mining -----------------------------------------------------
 * frl/losses/pairs.py:531-610 pairs_mutual_knn_chunked: per anchor the k nearest anchors by L2 distance in feature space, excluding
 * itself and same-patch anchors closer than pos_min_spatial pixels; knn_idx [N][k] in ascending distance (ties: lower index),
 * -1 where fewer than k candidates remain; mutual[i][r] = 1 iff i is also among the neighbours of knn_idx[i][r].
 * feat [N][D] float32 with D in {16, 32, 48, 64, 96, 128, 256} (pad narrower features with zero columns), patch_id [N] int32,
 * coords [N][2] float32 (row, col).  N is bounded by frl_mutual_knn_max_points(D) (four distance rows share the LDS). */
size_t frl_mutual_knn_max_points(int D);
int frl_mutual_knn(const float* feat, int N, int D, const int32_t* patch_id, const float* coords, float pos_min_spatial, int k,
                   int32_t* knn_idx, uint8_t* mutual, frl_stream_t stream);

/* ---- phase pair mining (csrc/phase_pairs.hip) ---------------------------------------------------------------------------------
 * frl/losses/phase_pairs.py:74-253 build_phase_pairs for every segment (sample) of a batch in one launch pair.  spec [N][D] float32 with
 * D in {16, 32, 48, 64, 96, 128, 256} (pad narrower features with zero columns), ysfc [N][T] float32, seg_host / seg: the S + 1 segment
 * offsets rising from 0 to N on the host (checked, sizes the grid) and the same on the device (read by the kernel); segments may be empty.
 * Per anchor i of segment s (n_s rows): the min(k, n_s - 1) nearest anchors of s by squared L2 (float32 sum of squared differences),
 * never i itself, in ascending (distance, index); overlap = number of distinct trunc(ysfc) values in 0..255 both pixels carry;
 * keep_overlap = overlap >= min_overlap; anchor_ok = at least min_pairs of its neighbours pass; keep = keep_overlap and anchor_ok;
 * dist = sqrtf(squared distance), weight = expf(-dist / sigma).  1 <= k <= 64.
 * out: knn_idx [N][k] int32 row numbers (-1 beyond n_s - 1 neighbours, where overlap, keep, keep_overlap, weight and dist are 0),
 * overlap [N][k] int32, keep / keep_overlap [N][k] bytes, weight / dist [N][k] float32, anchor_ok [N] bytes; counters [S][4] int32
 * (candidates, passing the overlap, cross pairs kept, anchors surviving) are ADDED to and *flag is OR-ed with 1 when ysfc holds a NaN, an
 * infinity, a negative value or a value >= 256 (such a value sets no bit): the caller zeroes both.  masks: workspace of N * 4 64-bit words.
 * A segment longer than frl_phase_pairs_max_points(D) (four distance rows share the LDS with the staging tile) returns -3. */
size_t frl_phase_pairs_max_points(int D);
int frl_phase_pairs(const float* spec, const float* ysfc, int N, int D, int T, const int32_t* seg_host, const int32_t* seg, int S, int k,
                    int min_overlap, int min_pairs, float sigma, uint64_t* masks, int32_t* knn_idx, int32_t* overlap, uint8_t* keep,
                    uint8_t* keep_overlap, float* weight, float* dist, uint8_t* anchor_ok, int32_t* counters, int32_t* flag,
                    frl_stream_t stream);

/* ---- spatial InfoNCE pair mining (csrc/spatial_pairs.hip) -------------------------------------------------------------------------
 * frl/training/representation/step.py:323-401 with frl/utils/spatial.py:176-332 (spatial_knn_pairs, spatial_negative_pairs) for every
 * segment (sample) of a batch per launch.  masks [S][H][W] bool bytes, anchors [N][2] int32 (row, col) concatenated over the samples,
 * seg_host / seg: the S + 1 offsets rising from 0 to N on the host (checked, sizes the grid) and on the device; segments may be empty.
 * 1 <= S <= 4096, 1 <= H, W <= frl_spatial_pairs_max_hw() (1024), 1 <= N <= 2^24; anything else returns a negative code before a launch.
 * An anchor outside [0, H) x [0, W) ORs 1 into *flag, reads nothing and gets no neighbour, no negative and no index.
 * counters [S] are ADDED to and *flag is OR-ed: the caller zeroes both.
 * frl_spatial_pack_mask: bits [S][H][ceil(W / 32)] 32-bit words, bit c % 32 of word c / 32 = pixel (r, c); the bits beyond W are 0.
 * frl_spatial_knn: offsets [k][2] int32 (dr, dc) on the device, 1 <= k <= 64 -> pos_rc [N][k][2] = anchor + offset, pos_valid [N][k] = 1
 *   iff that pixel is inside the grid and its bit is set; counters[s] += valid slots of segment s.
 * frl_spatial_negatives: the candidates of anchor (r, c) are the set pixels (y, x) of its segment's mask with
 *   lo <= (y - r)^2 + (x - c)^2 <= hi, in row-major order (lo > hi: none; hi is capped at (H - 1)^2 + (W - 1)^2); cnt is their number
 *   (popcounts of mask rows under at most two column intervals per row, integer square roots only).  draws [N][n_per_anchor] int32 in
 *   [0, 2^31), 1 <= n_per_anchor <= 64; a negative draw ORs 2 into *flag and is taken without its sign bit.  With m = min(n_per_anchor, cnt)
 *   draw j < m has the rank q = (uint64(draw) * (cnt - j)) >> 31 among the remaining candidates; going through the earlier picks in
 *   ascending order, q += 1 while q >= the pick, gives its rank among all candidates: uniform without replacement.
 *   neg_rc [N][n_per_anchor][2] holds the picks in draw order (-1 beyond m), neg_count [N] = m, counters[s] += the m of segment s.
 * frl_spatial_pair_index: per segment the sorted unique list of the anchors, the valid neighbours and the negatives (what
 *   torch.unique(dim=0) returns: ascending r * W + c), as set bits of a bitmap of H * W bits; the index of a coordinate is the number of
 *   set bits below its key.  unique_seg [S + 1] = offsets of the segments in unique_rc [N * (1 + k + n_per_anchor)][2] (capacity; the
 *   first unique_seg[S] rows are written); anchor_idx [N], pos_idx [N][k], neg_idx [N][n_per_anchor] = rows of unique_rc (shifted by the
 *   segment's offset), -1 for a slot that holds nothing.  feat [S][C][H][W] float32 (1 <= C <= 256, tau > 0):
 *   per pair slot d = sqrtf(sum_c (f_anchor - f_other)^2) in float32, channels ascending; pos_w = clamp(expf(-d / tau), min_w, 1),
 *   neg_w = clamp(1 - expf(-d / tau), min_w, 1); 0 for a slot that holds nothing.  Workspaces: bitmap S * ceil(H * W / 32) words
 *   (zeroed by the call), wordpre S * (ceil(H * W / 32) + 1) int32. */
int frl_spatial_pairs_max_hw(void);
int frl_spatial_pack_mask(const uint8_t* mask, int S, int H, int W, uint32_t* bits, frl_stream_t stream);
int frl_spatial_knn(const uint32_t* bits, int S, int H, int W, const int32_t* anchors, int N, const int32_t* seg_host, const int32_t* seg,
                    const int32_t* offsets, int k, int32_t* pos_rc, uint8_t* pos_valid, int32_t* counters, int32_t* flag, frl_stream_t stream);
int frl_spatial_negatives(const uint32_t* bits, int S, int H, int W, const int32_t* anchors, int N, const int32_t* seg_host, const int32_t* seg,
                          int lo, int hi, int n_per_anchor, const int32_t* draws, int32_t* neg_rc, int32_t* neg_count, int32_t* counters,
                          int32_t* flag, frl_stream_t stream);
int frl_spatial_pair_index(int S, int H, int W, const int32_t* anchors, int N, const int32_t* seg_host, const int32_t* seg, const int32_t* pos_rc,
                           const uint8_t* pos_valid, int k, const int32_t* neg_rc, const int32_t* neg_count, int n_per_anchor, const float* feat,
                           int C, float tau, float min_w, uint32_t* bitmap, int32_t* wordpre, int32_t* unique_seg, int32_t* unique_rc,
                           int32_t* anchor_idx, int32_t* pos_idx, int32_t* neg_idx, float* pos_w, float* pos_d, float* neg_w, float* neg_d,
                           frl_stream_t stream);

/* ---- anchor sampling (csrc/anchors.hip) -------------------------------------------------------------------------------------------
 * frl/data/sampling/anchor_sampling.py for S samples per launch, one workgroup per sample.  bits: the packed masks of
 * frl_spatial_pack_mask.  1 <= S <= 4096, 1 <= H, W <= frl_spatial_pairs_max_hw(); anything outside the stated limits returns a negative
 * code before a launch.  *flag is OR-ed (the caller zeroes it): 1 a jitter outside [-jitter_radius, jitter_radius], 2 a non-finite weight
 * at a masked pixel, 4 a negative or NaN noise at a masked pixel, 8 more than 4096 distinct values.
 * frl_anchor_grid_max: the largest number of grid points of a sample over all allowed jitters (the jitter -jitter_radius on both axes);
 *   stride >= 1, 0 <= jitter_radius <= border <= 1024, at most 16384 points.
 * frl_anchor_grid (sample_anchors_grid, :69-113): jitter [S][2] int32 (row, col) on the device.  The grid points of sample s are
 *   (border + jr + i stride, border + jc + j stride) for all rows < H - border and cols < W - border; those whose mask bit is set are
 *   written in row-major order to grid_rc [S][gmax][2] (gmax >= frl_anchor_grid_max; -1 beyond the count), their number to counts [S].
 *   A sample whose jitter is out of range gets no point and raises flag 1.
 * frl_anchor_supplement (:150-178): weights [S][H][W] float32 or NULL, noise [S][H][W] float32 >= 0 (Exp(1) variates), 0 <= supplement_n
 *   <= 1024.  A pixel is eligible when its mask bit is set and, with weights, w > 0; a sample with weights but no eligible pixel falls
 *   back to every masked pixel and ignores the weights.  The key of an eligible pixel is noise (no weights, or the fallback), otherwise
 *   noise / w rounded to nearest in float32; its sign bit is dropped.  The m = min(supplement_n, eligible) eligible pixels with the smallest
 *   (key, row * W + col) are written in ascending order of that pair to sup_rc [S][supplement_n][2] (-1 beyond m); counts [S] = m,
 *   n_valid [S] = set mask bits.  With iid Exp(1) noise this is sampling without replacement, uniform or proportional to the weights
 *   (the law of torch.multinomial(replacement=False)), in random order.  keys [S][H][W] 32-bit words is a workspace (the key patterns).
 *   supplement_n = 0: noise, keys and sup_rc may be NULL.
 * frl_anchor_inverse_frequency (_apply_inverse_frequency, :235-281): data [S][H][W] float32, valid_values a sorted int32 list on the device
 *   (0 <= n_values <= 4096) or NULL for no list.  A pixel is eligible when its bit is set, data is finite and, with a list,
 *   (int32) rintf(data) is in it (a rounded value beyond int32 is not).  out [S][H][W] = 1.0f / (float) count for an eligible pixel, count
 *   = the eligible pixels of the sample whose value compares equal (-0.0 and 0.0 are one value), 0 elsewhere; a sample without an eligible
 *   pixel gets 1.0 at the set bits.  More than 4096 distinct values in a sample raises flag 8 (the output is then not to be used). */
int frl_anchor_grid_max(int H, int W, int stride, int border, int jitter_radius);
int frl_anchor_grid(const uint32_t* bits, int S, int H, int W, int stride, int border, int jitter_radius, const int32_t* jitter, int gmax,
                    int32_t* grid_rc, int32_t* counts, int32_t* flag, frl_stream_t stream);
int frl_anchor_supplement(const uint32_t* bits, int S, int H, int W, const float* weights, const float* noise, int supplement_n,
                          uint32_t* keys, int32_t* sup_rc, int32_t* counts, int32_t* n_valid, int32_t* flag, frl_stream_t stream);
int frl_anchor_inverse_frequency(const float* data, const uint32_t* bits, int S, int H, int W, const int32_t* valid_values, int n_values,
                                 float* out, int32_t* flag, frl_stream_t stream);

/* ---- cross-patch spectral negatives and pair similarities (csrc/spectral_negatives.hip) --------------------------------------------
 * frl_spectral_negatives replaces frl/training/representation/step.py:743-773 (the double loop over ordered patch pairs with two
 *   torch.randint calls each, the concatenations, the two row gathers, the norm and the weight) by one launch.  spec [N][C] float32,
 *   1 <= C <= 256; offsets [S + 1] int32 on the device, rising from 0 to N with no empty patch, S >= 2; draws [Q][2] int32 in
 *   [0, 2^31), Q = n_per * S * (S - 1) < 2^31.  Negative q belongs to block b = q / n_per of the reference's loop order: pi = b / (S - 1),
 *   r = b % (S - 1), pj = r + (r >= pi).  With count_p = offsets[p + 1] - offsets[p]:
 *     i = offsets[pi] + ((uint64) draws[q][0] * count_pi >> 31),  j = offsets[pj] + ((uint64) draws[q][1] * count_pj >> 31)
 *   (uniform over the patch to within count / 2^31, never reaching count).  pairs [Q][2] int64 = (i, j); dist [Q] = sqrtf(sum_c
 *   (spec[i][c] - spec[j][c])^2) in float32 (lane-strided partial sums over 16 lanes, channels ascending, then a butterfly);
 *   weights [Q] = clamp(1 - expf(-dist / tau), min_w, 1), tau > 0.  A negative draw is taken as 0 and ORs 1 into *index_flag (may be
 *   NULL; the word behind ops.index_errors()); patch bounds that are not 0 <= offsets[p] < offsets[p + 1] <= N are clamped to a non-empty
 *   range inside spec and OR 2: no row outside spec is ever read.  Q = 0 is a no-op.
 * frl_pair_sims replaces the gathers of step.py:569-574 and :798-807: sims [T] = -sum_d (emb[a_t][d] - emb[b_t][d])^2 / D for pairs [T][2]
 *   int64 over emb [N][D] float32, 1 <= D <= 256 (same summation order).  A row in [-N, 0) wraps, any other row outside [0, N) is clamped
 *   and ORs 1 into *index_flag (may be NULL).  stats (may be NULL) receives 4 doubles: T, the mean of sims, their unbiased standard
 *   deviation (NaN when T < 2, as torch.std) and 0; the sums are kept in double, per-workgroup partials in ws
 *   (frl_pair_sims_workspace_bytes(T), 8-byte aligned; unused without stats), then one workgroup adds them in index order.  No float
 *   atomics: sims and stats are bit-reproducible.  T = 0 is a no-op (stats is left untouched).
 * Argument errors (C or D out of range, S < 2 with Q > 0, Q != n_per * S * (S - 1), tau <= 0, a NULL pointer with a non-zero count, a
 * workspace that is too small) return a negative code before any HIP call. */
int frl_spectral_negatives(const float* spec, int64_t N, int C, const int32_t* offsets, int S, int n_per, const int32_t* draws, int64_t Q,
                           float tau, float min_w, int64_t* pairs, float* dist, float* weights, int32_t* index_flag, frl_stream_t stream);
size_t frl_pair_sims_workspace_bytes(int64_t T);
int frl_pair_sims(const float* emb, int64_t N, int D, const int64_t* pairs, int64_t T, float* sims, double* stats, int32_t* index_flag, void* ws,
                  size_t ws_bytes, frl_stream_t stream);

/* ---- type-local spectral baseline (csrc/type_baseline.hip)----------------------------------------------------------------------
 * frl/training/representation/step.py:920-928.  z_k [N][K] float32 (the rank-K projection of the type embeddings, 1 <= K <= 64),
 * spec [N][T][C] float32 (T >= 1, 1 <= C <= 256, T * C < 2^31), N >= 2, 1 <= k <= min(64, N - 1).  Per anchor i: sim(i, j) =
 * sum_c z_k[i][c] z_k[j][c] in float32 (a NaN ranks as -inf); idx [N][k] int64 = the k rows j != i of largest sim in (sim descending,
 * index ascending) order; s_hat [N][C] = (sum over those rows, in rank order, of mean_t spec[j][t][c]) / k; out [N][T][C] =
 * spec - s_hat.  No [N][N] array is formed, no float atomics: bit-reproducible.  Workspace: frl_type_baseline_workspace_bytes(N, C)
 * (the time means). */
size_t frl_type_baseline_workspace_bytes(int N, int C);
int frl_type_baseline(const float* z_k, const float* spec, int N, int K, int T, int C, int k, float* out, float* s_hat, int64_t* idx, void* ws,
                      size_t ws_bytes, frl_stream_t stream);

/* ---- phase-type leakage loss (csrc/leakage.hip) -----------------------------------------------------------------------------------
 * frl/training/representation/step.py:1015-1021 over rows h [N][P] and z [N][Dz] (dtypes 0 = float32, 1 = bfloat16, independently;
 * N >= 1, 1 <= P <= 64, 1 <= Dz <= 128; f32 statistics): C = h_c^T z_c / max(N-1, 1) with the moments taken about a pivot (the mean of
 * the first min(N, 64) rows), stats [2] = (loss = sqrt(sum C^2), 1 / (max(N-1, 1) loss) or 0 where loss == 0).  cmat [P][Dz] = C and
 * centre [2][Dz] = pivot_z | mean_z - pivot_z are written when both are non-NULL and are what frl_leakage_bwd reads:
 * dh[n][p] = g[0] stats[1] sum_d z_c[n][d] C[p][d], in h_dtype; exactly zero where loss == 0 (the reference gives NaN there).
 * No float atomics: both calls are bit-reproducible.  Workspace: frl_leakage_workspace_bytes(N, P, Dz). */
size_t frl_leakage_workspace_bytes(int64_t N, int P, int Dz);
int frl_leakage_fwd(const void* h, int h_dtype, const void* z, int z_dtype, int64_t N, int P, int Dz, float* stats, float* cmat, float* centre,
                    void* ws, size_t ws_bytes, frl_stream_t stream);
int frl_leakage_bwd(const void* z, int z_dtype, const float* cmat, const float* centre, const float* stats, const float* g, int64_t N, int P,
                    int Dz, void* dh, int h_dtype, frl_stream_t stream);

/* ---- diagonal-covariance Gaussian mixtures and the phase summary (csrc/gmm.hip) ---------------------------------------------------
 * sklearn.mixture.GaussianMixture(covariance_type="diag") as frl/training/fit_gmm_clusters.py and fit_landscape_categories.py use it.
 * All data float32, contiguous: X [N][D], optional row weights w [N] >= 0 (NULL: ones), weights pi [K], means mu [K][D], variances
 * [K][D].  1 <= K <= 128, 1 <= D <= 128, K D <= 8192, K <= N < 2^31 (else -2).
 * The iteration works on y = x - pivot (pivot [D]: the column mean of X, frl_gmm_pivot, once per fit) and carries the centred means
 * means_c = mu - pivot next to mu, so data far from the origin loses nothing; the caller forms means_c once for initial parameters.
 * frl_gmm_em_step (E): one pass over X.  lp[n][k] = log pi_k - (D log 2 pi + sum_d log var_kd + sum_d (x_nd - mu_kd)^2 / var_kd) / 2,
 * lse_n = logsumexp_k lp, r = exp(lp - lse); each workgroup leaves sum w r, sum w r y, sum w r y^2, sum w lse and sum w in its slab of the
 * workspace.  hard != 0: r is one-hot at argmax_k lp (ties: the lowest k) -- with unit variances and equal weights a Lloyd step.
 * workgroups: 0 = the library's choice, else 1..4096 (the same value goes to frl_gmm_m_step; the workspace is sized for it).
 * frl_gmm_m_step (M): adds the slabs in slab order in double, nk = sum w r + 10 * 2^-52, mu = pivot + S1 / nk,
 * var = S2 / nk - (S1 / nk)^2 + reg_covar, pi = nk / sum nk.  mode 0 (EM) also appends lower_bound = sum w lse / sum w to
 * history [max_iter] at index state[0], increments state[0] (iterations done) and sets state[1] (converged) when the bound moved by less
 * than tol since the previous iteration; mode 1 (Lloyd) writes the means only, a component without a row keeps its mean; mode 2 writes
 * all parameters from whatever responsibilities the last E pass used and leaves history and state alone.
 * state: int32 [2], zeroed by the caller before a fit.  Once state[1] is set both calls leave every buffer untouched, so iterations
 * may be enqueued without reading anything back and the result does not depend on when the host looks.
 * frl_gmm_score: lse [N], labels [N] int32 (argmax_k lp, ties: the lowest k), optional resp [N][K].
 * No float atomics: every result is bit-identical from run to run.  Workspace (16-byte aligned): frl_gmm_workspace_bytes.
 * frl_phase_summary (_compute_phase_summary of fit_landscape_categories.py): z_phase [N][T][D] (T, D <= 64), ysfc [N][T] (NaN: not
 * observed) -> summary [N][3 D] = mean over t with ysfc <= low_max | mean over t with ysfc >= high_min | mean over all t, the first two
 * falling back to the third where no timestep matches; temporal_var [N] = the unbiased variance over t averaged over d (NaN at T = 1). */
size_t frl_gmm_workspace_bytes(int64_t N, int D, int K, int workgroups);
int frl_gmm_pivot(const float* X, int64_t N, int D, float* pivot, void* ws, size_t ws_bytes, frl_stream_t stream);
int frl_gmm_em_step(const float* X, const float* w, int64_t N, int D, int K, const float* pivot, const float* weights, const float* means_c,
                    const float* vars, int hard, int workgroups, const int* state, void* ws, size_t ws_bytes, frl_stream_t stream);
int frl_gmm_m_step(int64_t N, int D, int K, const float* pivot, float* weights, float* means, float* means_c, float* vars, double reg_covar,
                   double tol, int mode, double* history, int max_iter, int* state, int workgroups, void* ws, size_t ws_bytes,
                   frl_stream_t stream);
int frl_gmm_score(const float* X, int64_t N, int D, int K, const float* pivot, const float* weights, const float* means_c, const float* vars,
                  float* lse, int* labels, float* resp, frl_stream_t stream);
int frl_phase_summary(const float* z_phase, const float* ysfc, int64_t N, int T, int D, float low_max, float high_min, float* summary,
                      float* temporal_var, frl_stream_t stream);

/* ---- closed-form linear probes (csrc/probe.hip) ----------------------------------------------------------------------------------
 * The streamed ridge fit and the evaluation of frl/training/fit_linear_probe.py and fit_phase_linear_probe.py.
 * An observation is (b, t, p) with b < B, t < T, p < P.  Feature columns come from A [B][Ta][P][Da] and, when Db > 0, Bs [B][Tb][P][Db]
 * (Bs NULL exactly when Db = 0), targets from Y [B][Ty][P][Cy]; all row-major float32 with Ta, Tb, Ty each 1 (the row is shared by all
 * t) or T.  mask [B][P] uint8 is shared over t; an observation counts where it is non-zero.
 * Limits (else -2): D = Da + Db <= 128, 1 <= Cy <= 16, B T P < 2^31.  C = D + Cy.
 * frl_probe_pivot: pivot [C] = the masked column means of [x | y] of this call, summed in double in a fixed order, rounded to float32
 * (zeros when nothing is unmasked).
 * frl_probe_accumulate: with v = [x - pivot_x | y - pivot_y | m] (subtracted in float32; the whole row is zero where the mask is),
 * S [C+1][C+1] (double, both triangles) += v^T v and *n (int64) += the number of unmasked observations.  Tiles of 64 pixels whose
 * mask is all zero are not read.  The products are exact float32 fmaf chains inside a workgroup; the workgroups' slabs are added in a
 * fixed order in double.  workgroups: 0 = the library's choice, else 1..4096.  S and n are zeroed by the caller before the first call.
 * frl_probe_evaluate: pred_c = bc_c + sum_d (x_d - pivot_d) Wc[d][c], a float32 fmaf chain in d order (Wc [D][Cy], bc [Cy]); over the
 * unmasked observations E [Cy][3] (double) += (sum (pred - y)^2, sum (y - pivot_y), sum (y - pivot_y)^2) and *n += their number.
 * pred (optional) [B][T][P][Cy] receives the prediction of every observation, masked or not; without it all-zero mask tiles are skipped.
 * No float atomics: every result is bit-identical from run to run.  Workspace (16-byte aligned): frl_probe_workspace_bytes. */
size_t frl_probe_workspace_bytes(int D, int Cy, int workgroups);
int frl_probe_pivot(const float* A, int Ta, int Da, const float* Bs, int Tb, int Db, const float* Y, int Ty, int Cy, const unsigned char* mask,
                    int B, int T, int64_t P, float* pivot, void* ws, size_t ws_bytes, frl_stream_t stream);
int frl_probe_accumulate(const float* A, int Ta, int Da, const float* Bs, int Tb, int Db, const float* Y, int Ty, int Cy,
                         const unsigned char* mask, int B, int T, int64_t P, const float* pivot, int workgroups, double* S, int64_t* n, void* ws,
                         size_t ws_bytes, frl_stream_t stream);
int frl_probe_evaluate(const float* A, int Ta, int Da, const float* Bs, int Tb, int Db, const float* Y, int Ty, int Cy, const unsigned char* mask,
                       int B, int T, int64_t P, const float* pivot, const float* Wc, const float* bc, int workgroups, double* E, int64_t* n,
                       float* pred, void* ws, size_t ws_bytes, frl_stream_t stream);

/* ---- the phase probe's "full" design (csrc/probe_full.hip) --------------------------------------------------------------------------
 * [z_type | z_phase | z_type (x) z_phase] of fit_phase_linear_probe.py.  The inputs are those of the frl_probe_* calls with A = z_type
 * (Da = Dt) and Bs = z_phase (Db = Dp), both required.  Limits (else -2): 1 <= Dt <= 64, 1 <= Dp <= 16, Dq = Dt Dp <= 768,
 * 1 <= Cy <= 16, Ta, Tb, Ty each 1 or T, B T P < 2^31, workgroups 0 (the library's choice) or 1..4096.  C = Dt + Dp + Cy.
 * frl_probe_full_accumulate: with x' = x - pivot_x, p' = p - pivot_p, y' = y - pivot_y (float32 subtractions of the frl_probe_pivot of
 * the fit; zero rows where the mask is), c = [x' | p' | y' | m] and q' = x' (x) p' (column i Dp + a = x'_i p'_a, one float32 product),
 * Scq [C+1][Dq] += c^T q' and Sqq [Dq][Dq] += q'^T q' (double, both triangles).  c^T c and the count are frl_probe_accumulate's, called
 * with the same inputs and pivot.  Exact float32 fmaf chains inside a workgroup, the workgroups' slabs added in double in a fixed
 * order; all-zero mask tiles are not read.  Scq and Sqq are zeroed by the caller before the first call.
 * frl_probe_full_evaluate: pred_c = beta_c + x' . u_c + p' . v_c + x'^T Omega_c p' with beta [Cy], u [Cy][Dt], v [Cy][Dp],
 * omega [Cy][Dt][Dp], as a float32 fmaf chain: h_a = sum_i x'_i Omega_c[i][a] in i order from 0, then from beta_c the x'_i u_c[i] in i
 * order, the p'_a v_c[a] in a order, the h_a p'_a in a order.  E, n and pred are those of frl_probe_evaluate.
 * No float atomics: every result is bit-identical from run to run.  Workspace (16-byte aligned): frl_probe_full_workspace_bytes. */
size_t frl_probe_full_workspace_bytes(int Dt, int Dp, int Cy, int workgroups);
int frl_probe_full_accumulate(const float* A, int Ta, int Dt, const float* Bs, int Tb, int Dp, const float* Y, int Ty, int Cy,
                              const unsigned char* mask, int B, int T, int64_t P, const float* pivot, int workgroups, double* Scq, double* Sqq,
                              void* ws, size_t ws_bytes, frl_stream_t stream);
int frl_probe_full_evaluate(const float* A, int Ta, int Dt, const float* Bs, int Tb, int Dp, const float* Y, int Ty, int Cy,
                            const unsigned char* mask, int B, int T, int64_t P, const float* pivot, const float* beta, const float* u, const float* v,
                            const float* omega, int workgroups, double* E, int64_t* n, float* pred, void* ws, size_t ws_bytes, frl_stream_t stream);

/* ---- EVT-stratified diagnostics (csrc/strata.hip) ----------------------------------------------------------------------------------
 * The grouped accumulation of frl/training/compare_gmm_evt.py, phase_evt_diagnostics.py and ysfc_evt_histograms.py.
 * An observation is (b, t, p) with b < B, t < T, p < P (B T P < 2^31).  Its key is codes [B][P], int32 (codes_float = 0) or float32
 * (codes_float = 1), looked up in vocab [G] (int32, strictly increasing, 1 <= G <= 4095).  A code is valid when it is finite and > 0; a
 * valid float code is truncated towards zero (2^31 and above: INT_MAX).  mask (uint8 [B][Tm][P], Tm 1 or T; NULL: every observation)
 * says whether an observation counts.  In this order: a masked observation is skipped; one with an invalid code is skipped; one whose
 * valid code is not in vocab is skipped and *unmatched (int64) += 1.
 * frl_strata_contingency: rows int32 [B][Tr][P] (Tr 1 or T), 1 <= R <= 4096, R G <= 2^24.  A label outside [0, R) is skipped and
 * *rejected (int64) += 1; else table [R][G] (int64) += 1 at (label, column of the code).  Integer atomics only (in LDS up to 8192 cells,
 * 64-bit in memory beyond): the table is exact and order-independent.  table, unmatched and rejected are zeroed by the caller before the
 * first call; calls accumulate.
 * frl_strata_moments: X float32 [B][T][P][D], pivot [D], over the groups [g0, g0 + Gc) of the vocabulary (observations of other groups
 * are skipped, so a long vocabulary is walked in windows; unmatched may be NULL, for all windows but one).  1 <= D <= 128,
 * 1 <= Gc <= 128, Gc D <= 8192.  With y = x - pivot in float32:
 *   temporal = 0: per unmasked observation, count [G] (int64) += 1, S1 [G][D] (double) += y, S2 [G][D] += y^2.  SW is not touched.
 *   temporal = 1: one row per unmasked pixel (the mask is [B][1][P]): mu = (sum_t y_t, float32 in t order) / T and
 *   w = sum_t (y_t - mu)^2 / T (the population variance, exactly 0 at T = 1); count += 1, S1 += mu, S2 += mu^2, SW [G][D] += w.
 * The sums are exact float32 fmaf chains inside a workgroup; the workgroups' slabs are added in slab order in double, so every result is
 * bit-identical from run to run for one value of workgroups (0 = the library's choice, else 1..4096).  X must be finite in every row that
 * is not skipped.  Tiles of 64 pixels with nothing to add are not read.  count, S1, S2, SW are zeroed by the caller before the first call.
 * Limits: else -2.  Workspace (16-byte aligned) for frl_strata_moments: frl_strata_workspace_bytes(Gc, D, temporal, workgroups), which is
 * enough for every window of at most Gc groups (else -4); the table call needs none. */
size_t frl_strata_workspace_bytes(int Gc, int D, int temporal, int workgroups);
int frl_strata_contingency(const int32_t* rows, int Tr, const void* codes, int codes_float, const unsigned char* mask, int Tm, const int32_t* vocab,
                           int G, int B, int T, int64_t P, int R, int workgroups, int64_t* table, int64_t* unmatched, int64_t* rejected,
                           frl_stream_t stream);
int frl_strata_moments(const float* X, const void* codes, int codes_float, const unsigned char* mask, int Tm, const int32_t* vocab, int G, int g0,
                       int Gc, int B, int T, int64_t P, int D, const float* pivot, int temporal, int workgroups, int64_t* count, double* S1,
                       double* S2, double* SW, int64_t* unmatched, void* ws, size_t ws_bytes, frl_stream_t stream);

/* ---- exact grouped quantiles (csrc/quantile.hip) ------------------------------------------------------------------------------------
 * Exact order statistics of float32 values per cell, by radix select on a monotone key: the quartiles of
 * frl/training/phase_recovery_curves.py, ysfc_evt_histograms.py, representation/step.py (compute_stats) and data/stats, over every
 * observation where the reference samples.  key(x) is a uint32 whose unsigned order is the order of x, with -0.0 folded into +0.0 and
 * every NaN mapped to the largest key.  Four passes of 8-bit digits, most significant first: a pass counts, per (cell, column[, rank]),
 * the digit of the keys that match the prefix found so far; a small kernel picks the digit that holds the rank.  Integer atomics only
 * (32-bit, in LDS where the slots of a window fit, else in memory, added once per wave and target): results are exact, bit-identical
 * from run to run and under any permutation of the input.  Nothing is read back to the host.
 * frl_quantile_append: keyed as frl_strata_contingency (codes [B][P] against vocab [G], mask [B][Tm][P], rows [B][Tr][P] in [0, R) or
 * NULL with R = 1; the same order of tests, the same *unmatched and *rejected), R G <= 65535.  X float32 [B][T][P][D], 1 <= D <= 16.  A
 * surviving observation with a value that is not finite is skipped and *nonfinite += 1; every other one appends a record at a slot taken
 * from *cursor (int64, one add per workgroup and 1024 observations): cells [capacity] int32 = r G + g, keys [D][capacity] uint32.  Past capacity (< 2^31) nothing is
 * stored and *dropped += 1 per record.  cursor and the four counters are zeroed by the caller before the first call; calls accumulate.
 * frl_quantile_select: either the records (cells, keys, capacity, cursor: min(*cursor, capacity) of them, read on the device; X NULL) or
 * X float32 [N][D] with mask uint8 [N] or NULL, every unmasked row in cell 0 (cells NULL, C = 1, 1 <= N < 2^31).  probs: Q doubles in
 * [0, 1] on the host.  Per cell of n rows and probability q: v = (n - 1) q in double, k = floor(v), frac [C][Q] (double) = v - k,
 * lo [C][D][Q] and hi [C][D][Q] (float32) the order statistics of rank k and min(k + 1, n - 1), count [C] (int64) = n.  An empty cell:
 * count 0, frac 0, lo and hi NaN.  Outputs are overwritten.
 * Limits: 1 <= D <= 16, 1 <= Q <= 8, 1 <= C <= 65535, C D 2Q <= 2^23, workgroups 0 (the library's choice) or 1..4096: else -2.  Workspace (16-byte
 * aligned) for frl_quantile_select: frl_quantile_workspace_bytes(C, D, Q) (else -4; 0 beyond the limits); append needs none. */
size_t frl_quantile_workspace_bytes(int C, int D, int Q);
int frl_quantile_append(const float* X, const void* codes, int codes_float, const int32_t* rows, int Tr, const unsigned char* mask, int Tm,
                        const int32_t* vocab, int G, int B, int T, int64_t P, int D, int R, int workgroups, int32_t* cells, uint32_t* keys,
                        int64_t capacity, int64_t* cursor, int64_t* unmatched, int64_t* rejected, int64_t* nonfinite, int64_t* dropped,
                        frl_stream_t stream);
int frl_quantile_select(const int32_t* cells, const uint32_t* keys, int64_t capacity, const int64_t* cursor, const float* X,
                        const unsigned char* mask, int64_t N, int C, int D, const double* probs, int Q, int workgroups, int64_t* count, float* lo,
                        float* hi, double* frac, void* ws, size_t ws_bytes, frl_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* FRL_HIP_H */
