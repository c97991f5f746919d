/*
 * roma_hip.h — C ABI of libroma_hip.so: the MI355X (gfx950) kernels behind the RoMa dense-matching hot path
 * `RegressionMatcher.match()`.
 *
 * The reference (techshoww/RoMa) is pure Python/PyTorch and has NO FFI of its own; its seams are the Python call
 * signatures listed in SURVEY.md §8(b).  Every entry point below replaces the chain of stock ATen ops behind one of
 * those seams and cites it (file:line under the reference root).  A maintainer binds them with `ctypes`
 * (INTEGRATION.md shows the stubs); roma_amd/_lib.py is that binding for this repository.
 *
 * Conventions
 *   - plain C: pointers, ints, floats.  No torch / C++ types cross the boundary.
 *   - every pointer is DEVICE memory owned by the caller; the library allocates nothing and keeps no state
 *     except a thread-local error string.
 *   - every launch is asynchronous on `stream` (a hipStream_t passed as void*; NULL = the default stream).
 *   - return 0 = ok; <0 = bad argument (ROMA_E_*), roma_last_error() has the text; >0 = a hipError_t.
 *   - dtype codes ROMA_F32/F16/BF16 describe feature/logit storage; accumulation is always fp32.
 *     flow / certainty maps are always fp32 (as in the reference, matcher.py:141,397-402).
 *   - feature layouts: ROMA_NCHW = (B,C,H,W) contiguous; ROMA_NHWC = (B,H,W,pitch) with the C channels of interest
 *     starting at the pointer and `pitch` >= C elements between consecutive pixels (so a channel slice of a wider
 *     channels-last buffer — e.g. the ConvRefiner concat buffer — can be read or written in place).
 *     For ROMA_NCHW `pitch` is the number of channels of the enclosing (B,pitch,H,W) buffer.
 */
#ifndef ROMA_HIP_H
#define ROMA_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ROMA_ABI_VERSION 5

enum { ROMA_F32 = 0, ROMA_F16 = 1, ROMA_BF16 = 2 };
enum { ROMA_NCHW = 0, ROMA_NHWC = 1 };
/* roma_local_corr kernel selection for 16-bit channels-last inputs with r <= 3 (other inputs have one kernel): AUTO picks by launch size */
enum { ROMA_LC_AUTO = 0, ROMA_LC_TILE8X4 = 1, ROMA_LC_TILE8X8 = 2, ROMA_LC_ROWS8 = 3 };
enum { ROMA_E_ARG = -1, ROMA_E_DTYPE = -2, ROMA_E_SHAPE = -3, ROMA_E_ALIGN = -4, ROMA_E_UNSUPPORTED = -5 };

int roma_abi_version(void);
const char* roma_last_error(void);

/* local_correlation — romatch/utils/local_correlation.py:4-48, called from ConvRefiner.forward (matcher.py:121-125).
 *   out[b,k,y,x] = C^-1/2 * sum_c f0[b,c,y,x] * bilinear(f1[b,c], flow[b,:,y,x] + delta_k),  zeros padding,
 *   align_corners=False, k = iy*(2r+1)+ix, delta_k = ((ix-r)*2/W, (iy-r)*2/H).
 *   flow: (B,2,H,W) fp32 planar, (x,y) in [-1,1]; NULL = identity grid (local_correlation.py:16-27).
 *   f0,f1: `dtype`, `layout`, pitches f0_pitch/f1_pitch.  out: K=(2r+1)^2 channels, `dtype`, out_layout/out_pitch.
 *   r in {1..7}.  f1_batch_shift: f0's item b is correlated with f1's item (b + f1_batch_shift) % B — B/2 for
 *   forward_symmetric (matcher.py:516-528), whose second operand is the first with its batch halves swapped; 0 otherwise.
 *   variant: ROMA_LC_AUTO, or one of the kernels for 16-bit channels-last inputs with r <= 3 (8x4 / 8x8 tiles staged in 32-channel
 *   chunks; ROWS8 = the row-streaming kernel on 8x8 tiles, C = 256 or 512, else the 8x8 chunk kernel).  Same results
 *   to fp32 summation order; ignored where only one kernel applies. */
int roma_local_corr(const void* f0, const void* f1, const float* flow, void* out,
                    int B, int C, int H, int W, int r, int dtype,
                    int layout, int f0_pitch, int f1_pitch, int out_layout, int out_pitch, int f1_batch_shift, int variant,
                    void* stream);

/* F.grid_sample(y, flow^T, mode=bilinear, padding zeros, align_corners=False) — matcher.py:109 (ConvRefiner warp),
 * tiny.py:357,363.  src: (B,C,Hs,Ws); flow (B,2,H,W) fp32 planar; dst: (B,C,H,W).  Layout/pitch rules as above.
 * dst item b samples src item (b + src_batch_shift) % B (see roma_local_corr). */
int roma_warp_bilinear(const void* src, const float* flow, void* dst,
                       int B, int C, int Hs, int Ws, int H, int W, int dtype,
                       int layout, int src_pitch, int dst_layout, int dst_pitch, int src_batch_shift, void* stream);

/* displacement embedding — matcher.py:111-120: emb = Conv1x1(2->E)(gain * (flow - identity_grid)), gain = 40/32*scale_factor.
 *   weight (E,2) fp32, bias (E) fp32, flow (B,2,H,W) fp32, dst E channels of `dtype` in dst_layout/dst_pitch. */
int roma_disp_emb(const float* flow, const float* weight, const float* bias, void* dst,
                  int B, int E, int H, int W, float gain, int dtype, int dst_layout, int dst_pitch, void* stream);

/* F.interpolate(x, size=(Ho,Wo), mode="bilinear", align_corners=False) on fp32 planar maps — matcher.py:349-360,
 * 408-417, 657-659.  x: (N,Hi,Wi) planes, y: (N,Ho,Wo).  Optional fused flow update of Decoder.forward
 * (matcher.py:397-399): not here; see roma_flow_update. */
int roma_interp_bilinear(const float* x, float* y, int N, int Hi, int Wi, int Ho, int Wo, void* stream);

/* The same resize of TWO maps of one size in one launch — matcher.py:408-417, where the decoder upsamples flow and certainty
 * between levels: x0 (N0,Hi,Wi) -> y0 (N0,Ho,Wo) and x1 (N1,Hi,Wi) -> y1 (N1,Ho,Wo).  Every element is computed as by
 * roma_interp_bilinear. */
int roma_interp_bilinear_pair(const float* x0, float* y0, int N0, const float* x1, float* y1, int N1, int Hi, int Wi, int Ho, int Wo,
                              void* stream);

/* Input assembly of a ConvRefiner — matcher.py:109-120 and the channel padding of the concat buffer, in one launch:
 *   buf[.., C:2C]      = grid_sample(src, flow)           as roma_warp_bilinear, with src_batch_shift
 *   buf[.., 2C:2C+E]   = Conv1x1(2->E)(gain * (flow - identity_grid))   as roma_disp_emb
 *   buf[.., D:pitch]   = 0
 * buf: (B,H,W,pitch) channels-last of `dtype` (fp16 / bf16); src: (B,Hs,Ws,src_pitch) channels-last, C channels used, and may be
 * buf itself (x in channels [0, C), sampled with a batch shift); flow (B,2,H,W) fp32; weight (E,2), bias (E) fp32.  Every element
 * has the bits the two separate calls give.  Channels [0, C) are never written.  Channels [2C+E, D) are left alone except those that
 * share a 16-byte packet with channel D, which are zeroed: the local correlation, written afterwards, owns that slice.
 * Supported: C and E multiples of 8, or (C, E, D, pitch) = (9, 6, 24, 24) with src_pitch >= 16; pitches multiples of 8. */
int roma_refiner_assemble(const void* src, const float* flow, const float* weight, const float* bias, void* buf, int B, int C, int E,
                          int D, int pitch, int Hs, int Ws, int H, int W, int src_pitch, int src_batch_shift, float gain, int dtype,
                          void* stream);

/* Decoder.forward update step — matcher.py:397-402:
 *   flow[b,0] += ins*delta[b,0]/(4*Wf); flow[b,1] += ins*delta[b,1]/(4*Hf); cert[b] += delta[b,2]
 *   delta: (B,3,H,W) fp32 planar (the refiner's out_conv result); cert may be NULL-initialised via cert_in==NULL (=0). */
int roma_flow_update(float* flow, float* cert, const float* cert_in, const float* delta,
                     int B, int H, int W, float sx, float sy, void* stream);

/* cls_to_flow_refine — romatch/utils/utils.py:301-323 (softmax over res^2 anchors, mode, 5-point refinement with
 * CLAMPED neighbour indices).  logits element (b, c, p) at logits[b*stride_b + c*stride_c + p*stride_p], p = y*W+x,
 * C = res*res classes (C a multiple of 64).  flow out: (B,2,H,W) fp32 planar (the caller's permute(0,3,1,2),
 * matcher.py:383-385).  If cert_out != NULL the extra logit c == C (transformer/__init__.py:45) is copied to
 * cert_out (B,1,H,W) fp32. */
int roma_cls_to_flow_refine(const void* logits, float* flow_out, float* cert_out,
                            int B, int C, int HW, long stride_b, long stride_c, long stride_p,
                            int dtype, void* stream);

/* CosKernel — matcher.py:154-163:  K[b,n,m] = exp((<x_n,y_m>/(|x_n||y_m| + eps) - 1)/T), fp32 arithmetic / fp32 out on the
 * exact-fp32 MFMA (v_mfma_f32_32x32x2_f32).  x: (B,N,·) rows of `dtype` with x_pitch elements between rows (so the D feature
 * channels of a channels-last map can be read in place; 16-bit storage is widened exactly, i.e. the result equals the fp32
 * kernel on x.float(), matcher.py:254), y: (B,M,·) likewise; item b of x meets item (b + y_batch_shift) % B of y.
 * K: (B,N,M) fp32.  D a multiple of 16.  `diag_add` is added to K[b,i,i] (GP.forward's K_yy + sigma*I, matcher.py:259-261). */
int roma_cos_kernel(const void* x, const void* y, float* K, int B, int N, int M, int D, int dtype, int x_pitch, int y_pitch,
                    int y_batch_shift, float T, float eps, float diag_add, void* stream);

/* One diagonal-block step of the blocked Cholesky solve that replaces GP.forward's inv(K_yy + sigma I) @ f —
 * matcher.py:259-263.  For each of the B matrices: the nb x nb block at A (row-major, leading dimension lda, batch stride
 * strideA; only its lower triangle is read) is replaced by its Cholesky factor L (lower), and W (nb x nb, ldw, strideW)
 * receives L^-1.  A non-positive or NaN pivot p (0-based, within the block) is clamped and recorded: if info[b] == 0 it
 * becomes info_base + p + 1, so a zero-initialised info keeps the FIRST failing pivot of a whole blocked solve (the
 * reference's torch.linalg.inv raises in that case, matcher.py:261).  nb <= 64.  spd_solve (roma_amd/ops.py) calls it once, for the
 * first block; every later diagonal block is factored inside roma_chol_step, and the substitutions are roma_chol_subst_step. */
int roma_chol_diag_block(float* A, int lda, long strideA, float* W, int ldw, long strideW, int nb, int B, int* info,
                         int info_base, void* stream);

/* One fused forward step of the same blocked solve (matcher.py:259-263) on the augmented matrix A = [K | F] (B matrices, n rows,
 * ncols = n + m columns, row-major, lda, strideA): for the block rows [j, j+nb) whose diagonal block has already been factored
 * (W = the inverse of its Cholesky factor, from roma_chol_diag_block or from the previous call), with e = j + nb:
 *   R (nb x (ncols - e), ldr, strideR)  <-  W A[j:j+nb, e:]            (= [L[e:, j:j+nb]^T | Y[j:j+nb]]: needed by the back substitution)
 *   A[e:n, e:ncols]                     -=  R[:, :n-e]^T R             (only the 64 x 64 tiles on or right of the diagonal are updated)
 *   the next diagonal block A[e:e+nbn, e:e+nbn], nbn = min(64, n - e), is replaced by its Cholesky factor (lower triangle) and
 *   Wn (nbn x nbn, ldwn, strideWn) receives its inverse; info as in roma_chol_diag_block with info_base for THAT block.
 * Wn may be NULL (no factorisation; the last block).  One launch instead of the three per block of the GEMM formulation. */
int roma_chol_step(float* A, int lda, long strideA, int n, int ncols, int j, int nb, const float* W, int ldw, long strideW, float* R,
                   int ldr, long strideR, float* Wn, int ldwn, long strideWn, int* info, int info_base, int B, void* stream);

/* One fused step of a triangular substitution with the finished factor of the same solve.  R holds ALL panels written by
 * roma_chol_step: panel k of matrix b starts at R + b*strideRb + k*strideRs (nb rows, leading dimension ldr); its first
 * n - e_k columns, e_k = min((k+1) nb, n), are L[e_k:, block k]^T.  T is the right-hand side, consumed in place: block row i of
 * matrix b at T + b*strideTb + i*strideTs (leading dimension ldt), shifted by n - e_i columns when t_in_panel != 0 (the layout in
 * which roma_chol_step leaves Y: T = R, strideTs = strideRs, ldt = ldr).  W = the inverse factor of diagonal block s.
 *   dir < 0 (back substitution L^T X = T; call with s = S-1 down to 0):
 *       X[s nb : s nb + w_s, :] <- W^T T_s;   T_i -= L[block s, block i]^T X_s  for every i < s
 *   dir > 0 (forward substitution L Y = T for a NEW right-hand side — iterative refinement; call with s = 0 up to S-1):
 *       X[s nb : s nb + w_s, :] <- W T_s;     T_i -= L[block i, block s] Y_s    for every i > s
 * X: n x m, ldx, strideX.  nb = 64 (a single-block solve may use any nb <= 64).  One launch per block row instead of the two
 * GEMMs of the GEMM formulation. */
int roma_chol_subst_step(int dir, const float* W, int ldw, long strideW, const float* R, long strideRb, long strideRs, int ldr, float* T,
                         long strideTb, long strideTs, int ldt, int t_in_panel, float* X, int ldx, long strideX, int n, int m, int nb,
                         int s, int B, void* stream);

/* Multi-head attention forward, softmax(q k^T * scale) v, for the transformers of the path (DINOv2 blocks,
 * romatch/models/transformer/layers/attention.py:48-60; the decoder transformer, transformer/__init__.py:30-46): fp16 / bf16, head
 * dimension 64, no mask except "the first Nk tokens are keys / values" (the callers row-pad the sequence; padded tokens query only).
 * q, k, v, o are addressed as base + b*sb + token*sn + head*sh (element strides; each a multiple of 8, bases 16-byte aligned), so
 * the (B, N, 3, H, 64) output of the qkv projection is read in place and o can be the (B, N, H*64) input of the output projection.
 * Flash-style (no Nq x Nk matrix), fp32 softmax statistics, P rounded to the storage dtype before the second product. */
int roma_attention_fwd(const void* q, const void* k, const void* v, void* o, int B, int H, int Nq, int Nk, int head_dim, long q_sb,
                       long q_sn, long q_sh, long k_sb, long k_sn, long k_sh, long v_sb, long v_sn, long v_sh, long o_sb, long o_sn,
                       long o_sh, float scale, int dtype, void* stream);

/* match() post-processing — matcher.py:656-662, 684-718: certainty attenuation by the coarse scale-16 certainty,
 * sigmoid, zeroing where |flow|>1, clamp, symmetric concat.
 *   flow (2P,2,H,W), cert (2P,1,H,W) fp32 planar: first P = A->B, last P = B->A (forward_symmetric, matcher.py:516-528)
 *   cert16 (2P,1,H16,W16) or NULL (no attenuation).
 *   warp (P,H,2W,4) fp32, certainty (P,H,2W) fp32.   symmetric=0: flow (P,..), warp (P,H,W,4), certainty (P,H,W). */
int roma_match_finalize(const float* flow, const float* cert, const float* cert16, float* warp, float* certainty,
                        int P, int H, int W, int H16, int W16, int symmetric, void* stream);

/* kde — romatch/utils/kde.py:4-12: density[i] = sum_j exp(-|x_i - x_j|^2 / (2 std^2)), x: (N,4) fp32, ref points every
 * `down`-th row, density (N) fp32.  half_mode = 0: fp32 arithmetic (kde(half=False)).  half_mode = 1: x already holds
 * fp16-representable values (the caller's x.half()) and every term goes through the rounding points of the reference's fp16
 * evaluation (torch.cdist's matmul route in fp16, then fp16 **2, /, exp), summed in fp32 (the caller rounds the sum to fp16). */
int roma_kde_density(const float* x, float* density, int N, int down, float std, int half_mode, void* stream);

/* Exponential-race keys for sampling WITHOUT replacement — RegressionMatcher.sample (matcher.py:474-493), both of its
 * torch.multinomial(..., replacement=False) draws:  w_i = (thresh >= 0 && p_i > thresh) ? 1 : p_i  (the "threshold" sample
 * mode, matcher.py:474-477);  key_i = w_i / E_i with E_i = -ln(u_i) i.i.d. Exp(1); the k largest keys are a draw of k items
 * without replacement with probabilities proportional to w (what multinomial does internally).  u_i comes from a counter
 * hash of (seed, stage, c_i) — u = ((fmix32(fmix32(seed ^ stage * 0x9E3779B9) + c_i * 0x9E3779B1) >> 8) + 0.5) / 2^24, fmix32 = the
 * MurmurHash3 finaliser — so a CPU oracle reproduces the draw.  `stage` separates the draws of one sample() call (0 = the
 * certainty draw, 1 = the balanced draw): mixed non-linearly, so no (seed, stage) stream is a shifted copy of another.  c_i = counter[i] (int64, e.g. the item's index in the
 * population the first draw came from: the second draw then does not depend on the ORDER of the first) or i when counter
 * is NULL.  p, keys: (N) fp32; w_i <= 0 (or NaN) gives key 0. */
int roma_race_keys(const float* p, const long* counter, float* keys, long N, float thresh, unsigned seed, unsigned stage,
                   void* stream);

/* The k best items of each of P rows under the exponential race above, for sample_batch: row r ranks its N items by
 * (key descending, c ascending), key = the roma_race_keys key of (p[r,i], thresh, seeds[r], stage, c) bit for bit and
 * c = counter[r,i] or i when counter is NULL.  The c of one row must be distinct and below 2^32; the order is then total, so the
 * selected set and its order do not depend on P, on the other rows, on launch geometry or on a library's handling of equal keys
 * (thousands of items share a key: every weight above thresh is 1 and u has 24 bits; every weight <= 0 has key 0).
 * Radix select over the 64-bit value  sortkey = monotone(key bits) << 32 | (0xFFFFFFFF - c),  11 bits per pass, one launch per
 * pass (8 launches in all), keys recomputed from the hash in every pass; integer atomics only, no host synchronisation; the
 * library allocates nothing.
 *   p (P,N) fp32, counter (P,N) int64 or NULL, seeds (P) int64 (the low 32 bits are used), all device; 1 <= k <= N <= 2^24.
 *   sel_key (P,k) int64: the selected items' sortkey with the top bit flipped, so that SIGNED descending order is draw order;
 *   sel_idx (P,k) int64: their positions i, in the same slots.  The slots of a row are filled in arrival order: sort each row by
 *   sel_key, descending, to get the draw order (the values of a row are distinct, so any sort gives the same result).
 *   workspace: device, 8-byte aligned, at least roma_race_select_workspace(P, N, k) bytes (host function; < 0 on a bad shape);
 *   need not be initialised. */
long roma_race_select_workspace(int P, long N, int k);
int roma_race_select(const float* p, const long* counter, const long* seeds, int P, long N, int k, float thresh, unsigned stage,
                     long* sel_key, long* sel_idx, void* workspace, long workspace_bytes, void* stream);

/* roma_kde_density for P independent sets of n points in one launch (the pair on the grid's second axis), same term arithmetic
 * and summation order per query, so density[r] is bitwise what roma_kde_density gives for set r alone.  The points of set r are
 * rows of x (P,N,4) fp32: row index[r,j] when index (P,n) int64 is given (out-of-range values are clamped into the pair), else
 * row j (then N == n).  half_mode = 1 rounds the coordinates to fp16 in the load (no separate x.half() pass); density (P,n) fp32. */
int roma_kde_density_batch(const float* x, const long* index, float* density, int P, long N, int n, int down, float std,
                           int half_mode, void* stream);

/* Nearest neighbours for RegressionMatcher.match_keypoints (matcher.py:576-591): idx[i] = arg min_j |q_i - r_j|^2 over 2-D points
 * (lowest j on exact ties).  The reference materialises cdist(x_A_to_B, x_B) and compares it with its row / column minima;
 * mutual nearest neighbours only need this arg-min in both directions.  q: (NQ,2), r: (NR,2) fp32; idx: (NQ) int32. */
int roma_nn_argmin(const float* q, const float* r, int* idx, int NQ, int NR, void* stream);

/* Pre-processing on the device — utils.py:165-261 (TupleResize = PIL bicubic, ToTensorScaled, TupleNormalize), bit-identical
 * to the host path.  One pass of PIL's 8-bit resampling (Pillow Resample.c): out = clip8((2^21 + sum_k in[lo+k] * coef[k]) >> 22).
 *   in: uint8 (H, W, C);  axis 1: out (H, out_size, C), axis 0: out (out_size, W, C);
 *   bounds: int32 (out_size, 2) = (first input index, tap count); coef: int32 (out_size, ksize) 22-bit fixed point
 *   (computed on the host like precompute_coeffs / normalize_coeffs_8bpc: roma_amd/preproc.py). */
int roma_resample_u8(const void* in, void* out, int H, int W, int C, int out_size, int axis, const int* bounds,
                     const int* coef, int ksize, void* stream);
/*   uint8 (H, W, 3) -> fp32 (3, H, W): ((v / 255) - mean[c]) / std[c];  mean3, std3 are HOST pointers to 3 floats. */
int roma_normalize_u8(const void* in, float* out, int H, int W, const float* mean3, const float* std3, void* stream);

/* VGG19-BN layer epilogue with BatchNorm folded into the convolution — encoders.py:68-78 (conv -> BN -> ReLU):
 *   x[b,c,:] = max(x[b,c,:] + bias[c], 0) in place on a planar (B,C,HW) map of `dtype`; bias (C) of `dtype`.  B*C <= 65535. */
int roma_bias_relu_nchw(void* x, const void* bias, int B, int C, int HW, int dtype, void* stream);

/* The same epilogue for the VGG19-BN layers that are followed by MaxPool2d(2, 2) (encoders.py:68-78; the feature is captured before
 * each pool): x is updated in place as above and pooled[b,c,y,x] = max of the 2x2 block of the result, (B,C,H/2,W/2) of `dtype`.
 * H and W even. */
int roma_bias_relu_pool2_nchw(void* x, const void* bias, void* pooled, int B, int C, int H, int W, int dtype, void* stream);

/* The same two epilogues on channels-last maps (x: npix x C rows, C a multiple of 8 (16-bit) / 4 (fp32), in place; pooled:
 * (B, H/2, W/2, C)): the layout the VGG19 stack runs in (encoders.py:68-78). */
int roma_bias_relu_nhwc(void* x, const void* bias, long npix, int C, int dtype, void* stream);
int roma_bias_relu_pool2_nhwc(void* x, const void* bias, void* pooled, int B, int C, int H, int W, int dtype, void* stream);

/* MaxPool2d(2, 2) alone on a channels-last map: pooled (B, H/2, W/2, C) = max of each 2x2 block of x (B, H, W, C); H and W even, C a
 * multiple of 8 (16-bit) / 4 (fp32).  For a layer whose convolution already stored bias + ReLU (roma_conv3x3_bias_relu); on the same
 * map the result has the bits of roma_bias_relu_pool2_nhwc's pooled output. */
int roma_maxpool2_nhwc(const void* x, void* pooled, int B, int C, int H, int W, int dtype, void* stream);

/* One VGG19-BN layer in one kernel — encoders.py:68-78 (conv -> BN -> ReLU) with BatchNorm folded into w and bias:
 *   y[b,h,w,k] = max(round16(sum_{r,s,c} x[b,h+r-1,w+s-1,c] * w[k,r,s,c]) + bias[k], 0), 3x3, stride 1, zero pad 1, fp32 accumulation.
 * x: (B,H,W) pixels of Cin channels, x_pitch elements apart; w: (Cout,3,3,Cin) dense; bias: (Cout); y: (B,H,W) pixels of Cout channels,
 * y_pitch apart (channels past Cout of a wider row are left untouched).  dtype ROMA_F16 only (others: ROMA_E_UNSUPPORTED).  Cin, Cout
 * and the pitches multiples of 8, every buffer 16-byte aligned, each map below 2^31 elements.  The convolution is a Composable
 * Kernel grouped-forward-convolution instance with the epilogue as its CDE functor; `instance` in [0, count) selects the tile
 * configuration and ROMA_E_UNSUPPORTED is returned if that instance cannot run the shape.  Nothing is searched or timed. */
int roma_conv3x3_bias_relu(const void* x, const void* w, const void* bias, void* y, int B, int Cin, int Cout, int H, int W, int dtype,
                           int x_pitch, int y_pitch, int instance, void* stream);
/*   Returns the number of instances; with name != NULL also writes instance `index`'s CK type string (at most cap - 1 characters). */
int roma_conv3x3_bias_relu_instances(int index, char* name, int cap);

/* ConvRefiner block front half — matcher.py:77-103 (create_block: depthwise 5x5 conv, BatchNorm(eval), ReLU),
 * fused, channels-last.  BN is folded by the caller: y = relu(dwconv(x, w) * scale + shift).
 *   x,y: (B,H,W,pitch) `dtype`; w: (25, C) fp32 tap-major; scale, shift: (C) fp32. */
int roma_dwconv5x5_bn_relu(const void* x, const float* w, const float* scale, const float* shift, void* y,
                           int B, int C, int H, int W, int dtype, int x_pitch, int y_pitch, void* stream);

/* One whole ConvRefiner block, fused, for widths C <= 160 in fp16 / bf16 — matcher.py:77-103 (create_block) as applied
 * 9x per refiner at matcher.py:139-140:  y = bias + relu(dwconv5x5(x, w25) * scale + shift) @ wt^T.
 *   x, y: (B,H,W,pitch) channels-last `dtype` (C channels used; x and y must not alias);
 *   kpad: 32 or 160, the zero-padded channel count of the weight buffers (>= C);
 *   w25: (25, kpad) `dtype` tap-major; scale, shift, bias: (kpad) fp32; wt: (kpad, kpad) `dtype`, wt[n][k] = weight of
 *   input channel k for output channel n (the Conv2d(D, D, 1) weight itself), all zero-padded. */
int roma_refiner_block(const void* x, const void* w25, const float* scale, const float* shift, const void* wt,
                       const float* bias, void* y, int B, int C, int H, int W, int kpad, int dtype, int x_pitch, int y_pitch,
                       void* stream);

/* The same block at D = 576 (the scale-4 refiner), fp16, as ONE kernel: a 128-pixel x 576-channel output tile per workgroup, the
 * depthwise result computed once per pixel and fed to the matrix cores through LDS, the 1x1 weights streamed panel by panel.
 * matcher.py:77-103, 139-140.  x, y: (B,H,W,pitch) channels-last fp16 (must not alias); w25p: the depthwise taps in fp16 (the
 * reference's autocast convolution weights) as laid out by roma_refiner_wide_taps; scale, shift, bias: (D) fp32; wp: the
 * Conv2d(D, D, 1) weight [out][in] re-tiled by roma_refiner_wide_pack.  Both packers are HOST functions (all pointers in host memory):
 *   roma_refiner_wide_pack: wt, wp: D*D 16-bit elements each;
 *   roma_refiner_wide_taps: w25 (25, D) tap-major 16-bit -> w25p, 60*D elements: [D/32 panels][5 tap rows][4 packets][2 half-packets]
 *     [6 pair sets][4 channels][2] — the kernel multiplies horizontally adjacent PIXEL PAIRS with tap pairs (v_dot2_f32_f16): of a tap
 *     row (w0..w4) the even output column takes (w0,w1) (w2,w3) (w4,0), the odd one (0,w0) (w1,w2) (w3,w4). */
int roma_refiner_wide_pack(const void* wt, void* wp, int D);
int roma_refiner_wide_taps(const void* w25, void* w25p, int D);
int roma_refiner_block_wide(const void* x, const void* w25p, const float* scale, const float* shift, const void* wp,
                            const float* bias, void* y, int B, int H, int W, int D, int x_pitch, int y_pitch, int dtype,
                            void* stream);

/* ConvRefiner block back half at mid widths — matcher.py:102 (Conv2d(D, D, 1)) for 32 < D <= 160, fp16 / bf16, on the
 * matrix cores:  y[m][n] = bias[n] + sum_k x[m][k] * wt[n][k];  x, y: (M, pitch) channels-last rows (C used, may alias
 * only if identical); wt: (kpad, kpad) `dtype`, the Conv2d weight itself ([out][in]) zero-padded; bias (kpad) fp32. */
int roma_pointwise_mfma(const void* x, const void* wt, const float* bias, void* y, long M, int C, int kpad, int dtype,
                        int x_pitch, int y_pitch, void* stream);

/* The whole ConvRefiner block at mid widths in ONE launch — matcher.py:77-103, 139-140 — for 32 < C <= 160 (C a multiple of 8),
 * fp16 / bf16: roma_dwconv5x5_bn_relu and roma_pointwise_mfma (kpad 160) joined through on-chip memory, with their operands and
 * their bits:  y = bias + relu(dwconv5x5(x, w25) * scale + shift) @ wt^T, the intermediate rounded to `dtype`.
 *   x, y: (B,H,W,pitch) channels-last `dtype`, pitches multiples of 8 and >= C, bases 16-byte aligned, each below 4 GB; the two
 *   must not overlap.  Channels [C, y_pitch) of y are not written.
 *   w25: (25, C) fp32 tap-major; scale, shift: (C) fp32; wt: (160, 160) `dtype`, wt[n][k] zero-padded; bias: (160) fp32. */
int roma_refiner_block_mid(const void* x, const float* w25, const float* scale, const float* shift, const void* wt,
                           const float* bias, void* y, int B, int C, int H, int W, int dtype, int x_pitch, int y_pitch,
                           void* stream);

/* ConvRefiner head + Decoder update fused — matcher.py:141 (out_conv, D -> 3, fp32 on d.float()) and :397-402:
 *   d = bo + x[m,:] @ wo;  flow[b,0] += sx*d0;  flow[b,1] += sy*d1;  cert_out = (cert_in ? cert_in : 0) + d2
 *   x: (B*H*W, pitch) channels-last rows of `dtype` (C channels used), wo (C,3) fp32 row-major, bo (3) fp32,
 *   flow (B,2,H,W) fp32 updated in place, cert_in (B,1,H,W) or NULL, cert_out (B,1,H,W), delta_out (B,3,H,W) or NULL
 *   (the raw out_conv result, for callers that want the reference's (displacement, certainty) return values). */
int roma_refiner_head(const void* x, const float* wo, const float* bo, float* flow, const float* cert_in, float* cert_out,
                      float* delta_out, int B, int H, int W, int C, int pitch, int dtype, float sx, float sy, void* stream);

/* ConvRefiner block back half for NARROW activations — matcher.py:102 (Conv2d(D, D, 1) of create_block) at D <= 32:
 *   y[m][n] = bias[n] + sum_k x[m][k] * wt[k][n],  x,y: (M, pitch) channels-last rows of `dtype`, wt (C,C) fp32 row-major
 *   (in, out), bias (C) fp32.  C a multiple of 8 (fp16/bf16) or 4 (fp32), C <= 32. */
int roma_pointwise_small(const void* x, const float* wt, const float* bias, void* y, long M, int C, int dtype,
                         int x_pitch, int y_pitch, void* stream);

/* The decoder's folded 1x1 projection (Conv2d + BatchNorm, matcher.py:366-371) at the two finest scales, as a streaming kernel:
 *   y[m][n] = bias[n] + sum_k x[m][k] * wt[n][k],  n < N;   (K, N) = (64, 9) or (128, 64), fp16 / bf16, fp32 accumulation.
 *   x: (M, x_pitch) channels-last pixels; y: (M, y_pitch) rows of which only columns [0, N) are written (a slice of the refiner's
 *   concat buffer); wt: (N rounded up to 16, K) of `dtype`, out-major, rows >= N zero; bias: (N rounded up to 16) fp32.
 *   Pitches multiples of 8, bases 16-byte aligned. */
int roma_project_skinny(const void* x, const void* wt, const float* bias, void* y, long M, int K, int N, int dtype, int x_pitch,
                        int y_pitch, void* stream);

/* Residual add (+ LayerScale) fused with the following LayerNorm — the seam between two transformer half-blocks
 * (transformer/layers/block.py:87-107) and the fp32 token stream of the decoder transformer under autocast
 * (transformer/__init__.py:30-46: cat(fp32 GP posterior, fp16 features) promotes to fp32; LayerNorm is fp32; GEMMs take
 * 16-bit casts):
 *     if (y) x[r,:] = round_to_x_dtype(x[r,:] + ls[:] * y[r,:])      (ls == NULL: plain add), written back in place
 *     out[r,:] = gamma ? LayerNorm(x[r,:]; eps) * gamma + beta : x[r,:]     cast to out_dtype
 *   x (rows, x_stride) of x_dtype; y (rows, y_stride) of y_dtype or NULL; ls, gamma, beta (C) fp32 or NULL; out (rows,
 *   out_stride) of out_dtype.  Supported: fp32 stream with fp32/16-bit branch, 16-bit stream with a branch of the same
 *   dtype.  C a multiple of 8, <= 2048; strides multiples of 8. */
int roma_add_layernorm(void* x, int x_dtype, long x_stride, const void* y, int y_dtype, long y_stride, const float* ls,
                       const float* gamma, const float* beta, void* out, int out_dtype, long out_stride, long rows, int C,
                       float eps, void* stream);

/* TinyRoMa corr_volume + pos_embed fused — tiny.py:241-254, 178-203: for every source pixel the soft-argmax target
 * coordinate over the full correlation row, without materialising the (H1W1 x H0W0) volume.
 *   f0: (B,H0*W0,C), f1: (B,H1*W1,C) row-major fp32 (C a multiple of 16); out (B,2,H0,W0) fp32.
 *   exact != 0: full softmax expectation (tiny.py:201-202); exact == 0: reference fast path (tiny.py:187-198). */
int roma_tiny_corr_posembed(const float* f0, const float* f1, float* out, int B, int C,
                            int H0, int W0, int H1, int W1, int exact, void* stream);

/* JPEG decoding for match() on file paths — romatch/models/matcher.py:606-637, 667-676 (`Image.open(path).convert("RGB")`:
 * PIL -> libjpeg-turbo with its defaults, JDCT_ISLOW + fancy up-sampling).  The entropy-coded segment is decoded on the HOST
 * (roma_jpeg_info, roma_jpeg_entropy_decode: host functions, all pointers in host memory); de-quantisation + inverse DCT, chroma
 * up-sampling and YCbCr -> RGB run on the device (roma_jpeg_reconstruct) and leave a uint8 (height, width, 3) image for
 * roma_resample_u8 / roma_normalize_u8.  Bit-identical to PIL.  Supported: 8-bit sequential (one interleaved scan) and progressive
 * (spectral selection + successive approximation) Huffman streams, 1 or 3 components, 4:4:4 / 4:2:2 / 4:2:0, restart intervals; anything
 * else (CMYK, RGB-stored, 12-bit, arithmetic, lossless) returns ROMA_E_UNSUPPORTED (decode with PIL on the host then).
 *   info[8]: width, height, components, sub-sampling (0: 4:4:4, 1: 4:2:0, 2: 4:2:2, -1: grey), luma blocks per row, luma block rows, chroma
 *            blocks per row, chroma block rows;
 *   coef: int16, (luma + 2 x chroma blocks) x 64, natural order inside a block, blocks of a component in raster order, components
 *         one after the other; qt: 3 x 64 uint16, the component's de-quantisation table in natural order;
 *   planes: device scratch, (luma + 2 x chroma blocks) x 64 bytes; rgb: device, height x width x 3 bytes. */
int roma_jpeg_info(const void* data, long nbytes, int* info);
int roma_jpeg_entropy_decode(const void* data, long nbytes, int16_t* coef, uint16_t* qt);
int roma_jpeg_reconstruct(const int16_t* coef, const uint16_t* qt, void* planes, void* rgb, const int* info, void* stream);

/* Robust two-view geometry (RANSAC with MSAC scoring and least-squares local optimisation) — replaces the
 * estimator callers run on the output of match -> sample -> to_pixel_coordinates:
 *   kind 0, fundamental matrix (7-point):  cv2.findFundamentalMat(..., USAC_MAGSAC, maxIters=10000) of demo/demo_fundamental.py:28-34
 *                                          and of estimate_pose_uncalibrated, romatch/utils/utils.py:54-62;
 *   kind 1, homography (4-point DLT):      cv2.findHomography(..., RANSAC) of romatch/benchmarks/hpatches_sequences_homog_benchmark.py:72-86.
 * xa, xb: (P,N,2) fp64 pixel coordinates of P pairs.  `iters` minimal samples per pair, all drawn and scored (no early stop);
 * the draw is a pure function of (seed, p0 + p, sample), p0 = index of this call's first pair in a larger batch (geometry.hip
 * pins the hash).  threshold in pixels: inlier when the squared error (Sampson for F, forward transfer for H) < threshold^2.
 * Workspace: ws of at least roma_ransac_workspace(kind, P, N, iters, NULL) bytes, owned by the caller; the library allocates nothing.
 *
 * roma_ransac_workspace: host function; returns the workspace size in bytes (<0 on bad arguments) and, if offsets != NULL, the
 *   byte offsets of its 9 regions: [0] per-pair normalisation (P,8) fp64 = (cx, cy, s, 0) of A then of B, x_hat = (x - c) * s;
 *   [1] normalised points (P,N,4) fp32; [2] samples (P,iters,S) int32, S = 7 / 4, -1 = invalid sample; [3] minimal models
 *   (P,iters,R,3,3) fp64 in normalised coordinates, R = 3 / 1 slots per sample; [4] valid (P,iters,R) int32; [5], [6] the scoring
 *   slab; [7] MSAC cost per slot (P,iters,R) fp64 (+inf when invalid); [8] inlier count per slot (P,iters,R) int32.
 * roma_ransac_hypotheses: normalisation, samples, minimal solvers and scoring into the workspace (regions 0-8).
 * roma_ransac_select: the lowest-cost slot per pair, lo_iters rounds of local optimisation, de-normalisation.  model: (P,3,3) fp64
 *   (F: unit Frobenius norm, largest-magnitude entry positive; H: H[2,2] = 1), all zeros when no sample gave a model;
 *   mask: (P,N) uint8 inliers of the returned model. */
long roma_ransac_workspace(int kind, int P, int N, int iters, long* offsets);
int roma_ransac_hypotheses(int kind, const double* xa, const double* xb, int P, int N, int iters, float threshold, unsigned seed,
                           int p0, void* ws, long ws_bytes, void* stream);
int roma_ransac_select(int kind, const double* xa, const double* xb, int P, int N, int iters, float threshold, int lo_iters,
                       const void* ws, long ws_bytes, double* model, unsigned char* mask, void* stream);

/* The same with the scoring chosen by the caller: scoring 0 = MSAC (what the two calls above run, bit for bit), 1 = MAGSAC++
 * ("MAGSAC++ scoring"); any other value returns ROMA_E_ARG.  `threshold` keeps its meaning — the residual above which
 * a match is an outlier, mask = error < threshold^2 — and is the UPPER BOUND of the noise scale: with u = error / threshold^2 a slot
 * costs threshold^2 * sum of L(u) (L = 1 beyond the threshold) and the local optimisation is iteratively re-weighted least squares
 * with weights W(u), L and W the piecewise-linear interpolants of the 1 025 nodes u_j = j / 1024 that roma_magsac_table copies.  Both
 * calls of one estimate take the same scoring.  Workspace layout, regions and outputs are unchanged (region [7] is the chosen cost).
 * roma_magsac_table: host function; copies the nodes L(u_j) and W(u_j) into two caller arrays of 1 025 floats. */
int roma_ransac_hypotheses_ex(int kind, const double* xa, const double* xb, int P, int N, int iters, float threshold, int scoring,
                              unsigned seed, int p0, void* ws, long ws_bytes, void* stream);
int roma_ransac_select_ex(int kind, const double* xa, const double* xb, int P, int N, int iters, float threshold, int scoring,
                          int lo_iters, const void* ws, long ws_bytes, double* model, unsigned char* mask, void* stream);
int roma_magsac_table(float* loss, float* weight);

/* Calibrated two-view geometry — replaces estimate_pose of the reference (romatch/utils/utils.py:31-52:
 * cv2.findEssentialMat on calibrated points, then cv2.recoverPose), which its MegaDepth-1500 and ScanNet-1500 benchmarks call.
 * xa, xb: (P,N,2) fp64 PIXEL coordinates; Ka, Kb: (P,3,3) fp64 intrinsics, upper triangular with last row 0 0 1.  The estimator
 * works on x_hat = K^-1 x (no Hartley normalisation); `threshold` is in those calibrated units (the reference's norm_thresh): inlier
 * when the Sampson error < threshold^2.  `iters` 5-point samples per pair, all drawn and scored, up to 10 models each; the draw is
 * the hash of the RANSAC block above with stage 4 (essential.hip pins the solver and its tolerances).  A K with fx * fy == 0 or a
 * non-finite entry makes every sample of its pair invalid.  The library allocates nothing.
 *
 * roma_essential_workspace: host function; the workspace size in bytes (<0 on bad arguments) and, if offsets != NULL, the byte
 *   offsets of its 10 regions: [0]-[8] as roma_ransac_workspace with S = 5 and R = 10 ([0] is (0, 0, 1, 0) twice; [1] and [3] are in
 *   calibrated coordinates), [9] calibrated points (P,N,4) fp64 = (xa, ya, xb, yb), NaN where a match is not usable.
 * roma_essential_hypotheses: calibration, samples, 5-point solver and MSAC scoring into the workspace (regions 0-9).
 * roma_essential_select: the lowest-cost slot per pair, then lo_iters rounds of least squares on the inliers projected onto the
 *   essential manifold, each kept only if the cost drops.  E: (P,3,3) fp64 in calibrated coordinates (x_hat_B^T E x_hat_A = 0),
 *   singular values (1, 1, 0) / sqrt 2, largest-magnitude entry positive, all zeros when no sample gave a model; mask: (P,N) uint8.
 * roma_recover_pose: the four (R, t) of E — from roma_essential_select, or K_B^T F K_A — and the cheirality vote: for each
 *   candidate, the matches of mask_in ((P,N) uint8, NULL = all) whose least-squares depths in lambda_B x_B = lambda_A R x_A + t are
 *   finite and positive in both cameras; the candidate with the most wins (lowest index on ties, order (W,+) (W,-) (W^T,+) (W^T,-)).
 *   R: (P,3,3), t: (P,3) unit, count: (P) int32 votes of the winner, mask_out: (P,N) uint8 = mask_in narrowed to the matches that
 *   voted for it (what cv2.recoverPose leaves in its mask).  A zero or non-finite E (or K): R = I, t = 0, count 0, empty mask. */
long roma_essential_workspace(int P, int N, int iters, long* offsets);
int roma_essential_hypotheses(const double* xa, const double* xb, const double* Ka, const double* Kb, int P, int N, int iters,
                              float threshold, unsigned seed, int p0, void* ws, long ws_bytes, void* stream);
int roma_essential_select(const double* xa, const double* xb, const double* Ka, const double* Kb, int P, int N, int iters,
                          float threshold, int lo_iters, const void* ws, long ws_bytes, double* E, unsigned char* mask, void* stream);
int roma_recover_pose(const double* xa, const double* xb, const double* Ka, const double* Kb, const double* E,
                      const unsigned char* mask_in, int P, int N, double* R, double* t, int* count, unsigned char* mask_out,
                      void* stream);

/* roma_essential_hypotheses / roma_essential_select with the scoring chosen by the caller, as roma_ransac_*_ex above (0 = MSAC, 1 =
 * MAGSAC++; the re-weighted refit is projected onto the essential manifold as the unweighted one is). */
int roma_essential_hypotheses_ex(const double* xa, const double* xb, const double* Ka, const double* Kb, int P, int N, int iters,
                                 float threshold, int scoring, unsigned seed, int p0, void* ws, long ws_bytes, void* stream);
int roma_essential_select_ex(const double* xa, const double* xb, const double* Ka, const double* Kb, int P, int N, int iters,
                             float threshold, int scoring, int lo_iters, const void* ws, long ws_bytes, double* E, unsigned char* mask,
                             void* stream);

/* Non-linear refinement of a relative pose (csrc/pose_refine.hip) — the Levenberg-Marquardt stage behind the RANSAC
 * of poselib.estimate_relative_pose, which the reference's PoseLib benchmark calls.  Points and intrinsics as roma_recover_pose
 * (xa, xb 16-byte aligned); R_in (P,3,3), t_in (P,3): the pose to start from, e.g. of roma_recover_pose; mask_in: (P,N) uint8, the
 * matches that may carry weight (NULL = all).  Minimises the sum over the usable matches of min(r^2, threshold^2), r the Sampson
 * residual of x_hat = K^-1 x under E = [t]x R, threshold in calibrated units (fp64 here: the kernel compares fp64 residuals with
 * it), by at most `iters` damped Gauss-Newton steps over 3 rotation and 2 translation-direction parameters.  A step is kept only if
 * it lowers the cost, so the cost of the output is never above that of the input.
 * R: (P,3,3) orthonormal, t: (P,3) unit; mask: (P,N) uint8, r^2 < threshold^2 under the returned pose; cost: (P) fp64 its cost;
 * count: (P) int32 its inliers; steps: (P) int32 the steps kept.  A pair with fewer than 5 weighted matches, a singular normal
 * matrix, or an input pose that is not finite or has t = 0 gets its input pose back unchanged (steps = 0).  Outputs must not
 * overlap inputs.  One launch, no workspace, no host synchronisation; bitwise reproducible, and independent of the other pairs. */
int roma_refine_pose(const double* xa, const double* xb, const double* Ka, const double* Kb, const double* R_in, const double* t_in,
                     const unsigned char* mask_in, int P, int N, double threshold, int iters, double* R, double* t,
                     unsigned char* mask, double* cost, int* count, int* steps, void* stream);

/* Non-linear refinement of a fundamental matrix (csrc/fundamental_refine.hip) — the polish cv2.findFundamentalMat
 * runs after consensus, behind roma_ransac_select(kind 0).  xa, xb: (P,N,2) fp64 pixels, 16-byte aligned; F_in: (P,3,3), the model
 * to start from, any scale; mask_in: (P,N) uint8, the matches that may carry weight (NULL = all).  Minimises the sum over the usable
 * matches of min(r^2, threshold^2), r the Sampson residual in pixels (threshold in pixels, fp64), by at most `iters` damped
 * Gauss-Newton steps over the 7 parameters of F^ = U diag(1, s, 0) V^T in Hartley-normalised coordinates (the normalisation is
 * computed in the kernel).  A step is kept only if it lowers the cost.
 * F: (P,3,3), per pair EITHER a rank-2 model of unit Frobenius norm, largest-magnitude entry positive, of strictly lower cost than
 * F_in (steps >= 1), OR F_in bit for bit (steps = 0): no step lowered the cost, fewer than 8 weighted matches under F_in, a singular
 * normal matrix, an F_in that is not finite or has rank below 2.  mask: (P,N) uint8, r^2 < threshold^2 under the returned model;
 * cost: (P) fp64 its cost; count: (P) int32 its inliers (= the sum of mask); steps: (P) int32 the steps kept.  Outputs must not
 * overlap inputs.  One launch, no workspace, no host synchronisation; bitwise reproducible, and independent of the other pairs. */
int roma_refine_fundamental(const double* xa, const double* xb, const double* F_in, const unsigned char* mask_in, int P, int N,
                            double threshold, int iters, double* F, unsigned char* mask, double* cost, int* count, int* steps,
                            void* stream);

/* Non-linear refinement of a homography (csrc/homography_refine.hip) — the polish cv2.findHomography(..., RANSAC)
 * runs on the inliers after consensus, behind roma_ransac_select(kind 1).  xa, xb: (P,N,2) fp64 pixels, 16-byte aligned; H_in:
 * (P,3,3), the model to start from (x_B ~ H x_A), any scale; mask_in: (P,N) uint8, the matches that may carry weight (NULL = all).
 * Minimises the sum over the usable matches of min(e, threshold^2), e the squared forward transfer error in the pixels of image B
 * (threshold in pixels, fp64), by at most `iters` damped Gauss-Newton steps over 8 entries of H^ = T_B H T_A^-1 in Hartley-normalised
 * coordinates (the normalisation is computed in the kernel), scaled to unit Frobenius norm with its largest-magnitude entry held.  A
 * step is kept only if it lowers the cost.
 * H: (P,3,3), per pair EITHER a model with H[2,2] = 1 (unit Frobenius norm where |H[2,2]| < 1e-12 |H|) of strictly lower cost than
 * H_in (steps >= 1), OR H_in bit for bit (steps = 0): no step lowered the cost, fewer than 4 weighted matches under H_in, a singular
 * normal matrix, an H_in that is not finite or is all zero.  mask: (P,N) uint8, e < threshold^2 under the returned model; cost: (P)
 * fp64 its cost; count: (P) int32 its inliers (= the sum of mask); steps: (P) int32 the steps kept.  Outputs must not overlap
 * inputs.  One launch, no workspace, no host synchronisation; bitwise reproducible, and independent of the other pairs. */
int roma_refine_homography(const double* xa, const double* xb, const double* H_in, const unsigned char* mask_in, int P, int N,
                           double threshold, int iters, double* H, unsigned char* mask, double* cost, int* count, int* steps,
                           void* stream);

/* Absolute pose from 2D-3D matches (csrc/absolute_pose.hip): RANSAC with a P3P minimal solver, and the non-linear
 * refinement behind it — what places a further image against the points of roma_triangulate or of a depth map, where a host path
 * calls cv2.solvePnPRansac or poselib.estimate_absolute_pose.  Convention x ~ K (R X + t).
 * X: (P,N,3) fp64 world points (any frame); x: (P,N,2) fp64 PIXEL coordinates of the image being placed (16-byte aligned for
 * roma_absolute_pose_select and roma_refine_absolute_pose); K: (P,3,3) fp64, upper triangular with last row 0 0 1.  `threshold` is in
 * pixels: a match is an inlier when its squared reprojection error is below threshold^2 and it lies in front of the camera.
 * `scoring`: 0 = MSAC, 1 = MAGSAC++ (the tables of roma_magsac_table).  `iters` samples of 3 matches per pair, all drawn and scored, up
 * to 4 poses each; the draw is the hash of the RANSAC block above with stage 5 and p = p0 + pair (absolute_pose.hip pins the solver
 * and its tolerances).  A row with a non-finite X or x is never sampled and never an inlier; a K with fx * fy == 0 or a non-finite
 * entry makes every sample of its pair invalid.  The world points are normalised per pair (X' = s (X - c): centroid c, mean distance
 * sqrt 3), so the fp32 scoring does not depend on where the world's origin is.  The library allocates nothing.
 *
 * roma_absolute_pose_workspace: host function; the workspace size in bytes (<0 on bad arguments) and, if offsets != NULL, the byte
 *   offsets of its 12 regions: [0]-[8] as roma_ransac_workspace with S = 3 and R = 4, where [0] is (c_x, c_y, c_z, s, 0, 0, 0, 0) per
 *   pair, [1] the scoring records (P,N,4) fp32 = (X'_x, X'_y, X'_z, u), NaN where a match is not usable, and [3] the rotations
 *   (P,iters,4,3,3) fp64; [9] t' (P,iters,4,3) fp64, the translation in the normalised frame, t = t' / s - R c; [10] v (P,N) fp32 of
 *   the scoring records; [11] (P,N,5) fp64 = (X', K^-1 x), the solver's copy.
 * roma_absolute_pose_hypotheses: normalisation, samples, P3P and scoring into the workspace (all regions).
 * roma_absolute_pose_select: the lowest-cost slot per pair (lowest slot on ties), then lo_iters rounds of local optimisation: one damped
 *   Gauss-Newton step of roma_refine_absolute_pose on the inliers (weighted by W for MAGSAC++), kept only if the cost drops.
 *   R: (P,3,3) orthonormal, det +1; t: (P,3); mask: (P,N) uint8.  A pair without a valid slot: R and t all zero, empty mask.
 * roma_refine_absolute_pose: Levenberg-Marquardt from (R_in, t_in) on the sum over the usable matches (finite, allowed by mask_in —
 *   (P,N) uint8, NULL = all —, in front of the camera) of min(e, threshold^2), at most `iters` steps over 3 rotation and 3 translation
 *   parameters; the schedule and the outputs are those of roma_refine_pose.  A pair with fewer than 4 weighted matches, a singular
 *   normal matrix, an input pose that is not finite, or no step that lowers the cost gets its input pose back bit for bit (steps = 0)
 *   with its own mask, cost and count.  One launch, no workspace. */
long roma_absolute_pose_workspace(int P, int N, int iters, long* offsets);
int roma_absolute_pose_hypotheses(const double* X, const double* x, const double* K, int P, int N, int iters, float threshold,
                                  int scoring, unsigned seed, int p0, void* ws, long ws_bytes, void* stream);
int roma_absolute_pose_select(const double* X, const double* x, const double* K, int P, int N, int iters, float threshold, int scoring,
                              int lo_iters, const void* ws, long ws_bytes, double* R, double* t, unsigned char* mask, void* stream);
int roma_refine_absolute_pose(const double* X, const double* x, const double* K, const double* R_in, const double* t_in,
                              const unsigned char* mask_in, int P, int N, double threshold, int iters, double* R, double* t,
                              unsigned char* mask, double* cost, int* count, int* steps, void* stream);

/* 3-D similarity registration from 3D-3D correspondences (csrc/similarity.hip): RANSAC with a 3-point minimal sample
 * and the iterated closed-form refinement behind it — what puts two reconstructions, each in units of its own baseline, into one frame.
 * Model Y ~ s R X + t: s > 0, R orthonormal with det +1; with_scale = 0 is the rigid model, s = 1.
 * X, Y: (P,N,3) fp64, 8-byte aligned.  `threshold` is a distance in the units of Y: a correspondence is an inlier when
 * |Y - (s R X + t)|^2 < threshold^2.  `scoring`: 0 = MSAC, 1 = MAGSAC++.  `iters` samples of 3 rows per pair, all drawn and scored, one
 * model each (Umeyama's closed form, the rotation by Horn's quaternion); the draw is the hash of the RANSAC block above with stage 6
 * and p = p0 + pair.  A row with a non-finite number is never sampled and never an inlier.  Both clouds are normalised per pair
 * (X' = sX (X - cX), Y' = sY (Y - cY): centroids, mean distance sqrt 3; with_scale = 0: sX = sY), so the fp32 scoring depends neither on
 * where the origins are nor on the ratio of the scales.  The library allocates nothing.
 *
 * roma_similarity_workspace: host function; the workspace size in bytes (<0 on bad arguments) and, if offsets != NULL, the byte offsets
 *   of its 12 regions: [0]-[8] as roma_ransac_workspace with S = 3 and R = 1, where [0] is (cX, sX, cY, sY) per pair, [1] the scoring
 *   records (P,N,4) fp32 = (X', Y'_x), NaN where a row is not usable, and [3] the rotations (P,iters,3,3) fp64; [9] (t', s')
 *   (P,iters,4) fp64, the model of the normalised clouds: s = s' sX / sY, t = t' / sY + cY - s R cX; [10] (Y'_y, Y'_z) (P,N,2) fp32 of
 *   the scoring records; [11] (P,N,6) fp64 = (X', Y'), the solver's copy.  The workspace must be 16-byte aligned.
 * roma_similarity_hypotheses: normalisation, samples, the closed form and scoring into the workspace (all regions).
 * roma_similarity_select: the lowest-cost slot per pair (lowest slot on ties), then lo_iters rounds of local optimisation: the closed
 *   form on the inliers (weighted by W for MAGSAC++), kept only if the cost drops.  It reads the workspace roma_similarity_hypotheses
 *   left (same P, N, iters, threshold, scoring), not X and Y again.  s: (P); R: (P,3,3); t: (P,3); mask: (P,N) uint8; valid: (P) int32.
 *   A pair without a valid slot: s, R and t all zero, empty mask, valid = 0.
 * roma_refine_similarity: from (s_in, R_in, t_in), at most `iters` rounds of the closed form on the matches with e < threshold^2, on the
 *   sum over the usable matches (finite, allowed by mask_in — (P,N) uint8, NULL = all) of min(e, threshold^2) in fp64.  A round is kept
 *   when cost' < cost (1 - 1e-12); the first that is not ends the loop.  A pair with fewer than 3 weighted matches, a configuration that
 *   does not fix the rotation, an input that is not finite, or no round kept gets its input back bit for bit (steps = 0) with its own
 *   mask, cost and count.  cost: (P) fp64 in squared Y units; count, steps: (P) int32.  One launch, no workspace. */
long roma_similarity_workspace(int P, int N, int iters, long* offsets);
int roma_similarity_hypotheses(const double* X, const double* Y, int P, int N, int iters, float threshold, int scoring, int with_scale,
                               unsigned seed, int p0, void* ws, long ws_bytes, void* stream);
int roma_similarity_select(const double* X, const double* Y, int P, int N, int iters, float threshold, int scoring, int with_scale,
                           int lo_iters, const void* ws, long ws_bytes, double* s, double* R, double* t, unsigned char* mask, int* valid,
                           void* stream);
int roma_refine_similarity(const double* X, const double* Y, const double* s_in, const double* R_in, const double* t_in,
                           const unsigned char* mask_in, int P, int N, double threshold, int iters, int with_scale, double* s, double* R,
                           double* t, unsigned char* mask, double* cost, int* count, int* steps, void* stream);

/* Two-view triangulation of matches under a known relative pose (csrc/triangulate.hip) — what a caller does with
 * the (R, t) of roma_recover_pose / roma_refine_pose: a point cloud of the sampled matches, or a depth map per image from every row of
 * the dense warp.  Convention of roma_recover_pose: x_B ~ K_B (R X_A + t).  Points are expressed in camera A's frame, in units of
 * |t|: with the unit t of roma_recover_pose, depths are in baselines.
 *   m: (P,N,4) fp32 device, contiguous, 16-byte aligned, rows [xa, ya, xb, yb] — the layout of the warp of match(), of what sample()
 *     returns, of cat(kptsA, kptsB);
 *   to_px: 8 floats in HOST memory, read during the call, or NULL: (sx_A, ox_A, sy_A, oy_A, sx_B, ox_B, sy_B, oy_B), pixel = s * c + o.
 *     NULL: the rows are pixels already.  For the normalised coordinates of a warp: (W_A/2, W_A/2, H_A/2, H_A/2, W_B/2, ...);
 *   Ka, Kb: (P,3,3) fp64 intrinsics as roma_recover_pose; R: (P,3,3) fp64; t: (P,3) fp64, of any length;
 *   mask_in: (P,N) uint8 or NULL (= all); method: 0 = optimal, 1 = midpoint; max_reproj: pixels, +inf = no gate; max_cos_parallax:
 *     1 = no gate (the caller turns a smallest parallax angle into its cosine).
 * Per pair, in fp64: F = K_B^-T [t]x R K_A^-1 scaled to unit Frobenius norm and the two inverse intrinsics; then, per match, in fp32:
 *   method 0: Lindstrom's closed-form two-step correction (niter2) in pixel space moves (x_A, x_B) by the smallest |d_A|^2 + |d_B|^2
 *     onto x_B^T F x_A = 0; the corrected rays a, b meet, lambda_B b = lambda_A R a + t, X_A = lambda_A a, the depths are lambda_A and
 *     lambda_B, reproj = sqrt(|d_A|^2 + |d_B|^2);
 *   method 1: the same depths on the uncorrected rays; X_A is the midpoint of the two closest points, the depths are its z in A and
 *     in B, reproj is the root of the sum over both images of the squared pixel distance from its projection to the match;
 *   cos_parallax = (R a . b) / (|R a| |b|).
 * Outputs, device, each may be NULL but not all: points (P,N,3) fp32; depth_a, depth_b, reproj, cos_parallax (P,N) fp32; valid (P,N)
 * uint8 = input finite, mask_in set, solution finite, both depths > 0, reproj <= max_reproj, cos_parallax <= max_cos_parallax.  Every
 * requested element is written: exact zeros everywhere for a match whose input or solution is not finite (a singular K, t = 0 or
 * parallel rays among them), the computed values for any other match, valid or not; never NaN or inf.  An output does not depend on
 * which other outputs are requested, nor a pair on the other pairs.  One launch, no workspace, no atomics, no host synchronisation. */
int roma_triangulate(const float* m, const float* to_px, const double* Ka, const double* Kb, const double* R, const double* t,
                     const unsigned char* mask_in, int P, int N, int method, float max_reproj, float max_cos_parallax, float* points,
                     float* depth_a, float* depth_b, float* reproj, float* cos_parallax, unsigned char* valid, void* stream);

/* N-view triangulation (csrc/triangulate_nview.hip): a point seen in V posed views, triangulated from all of them, with
 * the views that disagree left out — a cloud of tracks after the absolute-pose calls above, or ONE depth map of a reference image from
 * its k warps against k others.  Convention of the absolute-pose calls: x_v ~ K_v (R_v X + t_v), v = 0 .. V-1, 2 <= V <= 32.  ONE
 * reconstruction per call: there is no P dimension, the views are the batch.
 *   obs: V device pointers in HOST memory, read during the call.  The observations are read in place: with n = r * row_len + c, r <
 *     rows, c < row_len, point n of view v is the two fp32 at obs[v] + r * row_stride + c * point_stride (strides in floats, common to
 *     all views).  Packed (V,N,2): rows = 1, row_len = N, point_stride = 2.  The A half of a symmetric warp (H,2W,4): rows = H,
 *     row_len = W, row_stride = 8 W, point_stride = 4, the base offset by 2 floats for the predicted x_B and by 0 for the grid of A.
 *     Pointers 8-byte aligned; strides even, row_stride >= 0, point_stride >= 2; rows <= 65535, rows * row_len <= 2^28;
 *   to_px: V x 4 floats in HOST memory, (sx, ox, sy, oy) per view, pixel = s * c + o, or NULL: the coordinates are pixels already;
 *   visible: NULL, or V device pointers in HOST memory to uint8 (rows, row_len) with row stride vis_row_stride (bytes), non-zero =
 *     view v may see point n; a single entry may be NULL (always visible).  An observation that is not finite is not observed;
 *   K, R: (V,3,3) fp64 device, K upper triangular with last row 0 0 1; t: (V,3) fp64 device.  A view whose K is singular or whose
 *     pose is not finite observes nothing;
 *   max_view_error: pixels, +inf = use every observed view.  Otherwise (robust): every pair of observed views gives the midpoint of its
 *     two rays; a view is an inlier of it with positive depth and a pixel error <= max_view_error; a hypothesis counts if its own two
 *     views are inliers and scores sum over observed views of (inlier ? e^2 : max_view_error^2); the lowest score wins, the first pair
 *     (a, b), a < b, on a tie; the point's view set is the winner's inliers (empty without a hypothesis that counts);
 *   iters: 0 .. 10 Levenberg-Marquardt steps on the sum over the set of the squared pixel error, from the point closest to the set's
 *     rays; a step is kept only if the cost drops.  min_views: 2 .. V.  ref_view: the view whose z `depth` reports.
 * Per call, in fp64: K_v^-1, the centres C_v = -R_v^T t_v and their mean c0 over the usable views in view order; everything per point
 * is fp32 relative to c0 (the result does not depend on where the world's origin is), and c0 is added back in fp64.
 * Outputs, device, each may be NULL but not all: points (N,3) fp32, world frame; depth (N) fp32; reproj (N) fp32 = the root of the
 * MEAN over the used views of the squared pixel error (roma_triangulate reports the root of the SUM over its two images);
 * cos_parallax (N) fp32 = the smallest cosine over pairs of used views between the rays from the point to their centres; views (N)
 * uint32, bit v = view v used; valid (N) uint8 = at least min_views used, everything finite, positive depth in every used view,
 * reproj <= max_reproj, cos_parallax <= max_cos_parallax.  Every requested element is written: exact zeros (views = 0) for a point
 * with fewer than two views in its set or without a finite solution, the computed values for any other, valid or not; never NaN or
 * inf.  An output does not depend on which others are requested.  One launch, no workspace, no atomics, no host synchronisation. */
int roma_triangulate_nview(const float* const* obs, const float* to_px, const unsigned char* const* visible, long vis_row_stride,
                           const double* K, const double* R, const double* t, int V, int rows, int row_len, long row_stride,
                           long point_stride, float max_view_error, int iters, int min_views, int ref_view, float max_reproj,
                           float max_cos_parallax, float* points, float* depth, float* reproj, float* cos_parallax, unsigned* views,
                           unsigned char* valid, void* stream);

/* Tracks from pairwise matches (csrc/tracks.hip): the sampled matches of M image pairs over V views (2 <= V <= 32),
 * joined into tracks in the form roma_triangulate_nview reads.  tests/tracks_ref.py restates the definition; outputs are exact.
 *   matches: (M,k,4) fp32 device, 16-byte aligned, normalised [xA, yA, xB, yB]; certainty: (M,k) fp32 device; mask: (M,k) uint8 device
 *     or NULL; pairs: (M,2) int32 device, the views (a_m, b_m) of pair m; sizes: V x 2 ints in HOST memory, (H_v, W_v), 1 to 65536;
 *   cell: 1 .. 64 pixels.  View v has ceil(H_v / cell) x ceil(W_v / cell) cells with global ids base_v + cy * Wc_v + cx, base the
 *     running sum; their number C must be below 2^31.  M * k < 2^31; max_tracks >= 1, V * max_tracks < 2^30; 2 <= min_views <= V;
 *     certainty_thresh finite, >= 0.
 * An endpoint in view v is at px = (x + 1.0f) * (0.5f * W_v), py likewise, in cell ((int)floorf(px * inv), (int)floorf(py * inv)), inv
 * = 1.0f / cell, and inside when 0 <= px < W_v, 0 <= py < H_v and the cell exists.  A match is usable when both endpoints are inside,
 * its certainty is finite and > certainty_thresh, its mask is not 0, both views are in [0, V) and differ.  A cell with a usable
 * endpoint is a node; its keypoint is the endpoint of the highest certainty, the lowest endpoint index (m * k + j) * 2 + side on a
 * tie.  Usable matches are edges; a component's label is its lowest node id; it is conflicting with two nodes in one view and
 * qualifies when it is not and sees at least min_views views.  Qualifying components get rows 0, 1, ... in ascending label order;
 * rows >= max_tracks are dropped.
 * Outputs, device, all required: x (V,max_tracks,2) fp32 pixels, NaN where a view does not see a track; visible (V,max_tracks) uint8;
 * views (max_tracks) int32, bit v = view v sees the track; num_views (max_tracks) uint8; track_of_match (M,k) int32, the row of a
 * usable match's track or -1; counts (4) int32: qualifying components before truncation, conflicting ones, ones below min_views, and a
 * status word: 0, or 1 if an edge gave up after 2^20 rounds of the union's retry loop (never in correct operation).  Rows from
 * min(counts[0], max_tracks) on stay empty.
 * workspace: roma_tracks_workspace(V, sizes, cell, &cells) bytes (21 per cell and 12 per 256 cells), 16-byte aligned; the function
 * returns a negative code for bad arguments and stores C in *cells (may be NULL).  Eight launches on `stream`, integer atomics only, no
 * host synchronisation; nothing depends on the order in which threads arrive. */
long roma_tracks_workspace(int V, const int* sizes, int cell, long* cells);
int roma_build_tracks(const float* matches, const float* certainty, const unsigned char* mask, const int* pairs, const int* sizes, int M,
                      int k, int V, int cell, float certainty_thresh, int min_views, int max_tracks, float* x, unsigned char* visible,
                      int* views, unsigned char* num_views, int* track_of_match, int* counts, void* workspace, long workspace_size,
                      void* stream);

/* Bundle adjustment (csrc/bundle.hip): the V views (2 <= V <= 32) and N points (1 <= N <= 2^24) of ONE reconstruction
 * refined together by Levenberg-Marquardt on the truncated reprojection cost, the cameras through the Schur complement of the points.
 * Convention of roma_triangulate_nview: x_v ~ K_v (R_v X + t_v).  tests/bundle_ref.py restates the definition with the full normal
 * equations.  A polish: it needs a start within a few pixels of the observations.
 *   obs, to_px, visible: as roma_triangulate_nview with one row (rows = 1, row_len = N): point n of view v is the two fp32 at obs[v] +
 *     n * point_stride (floats, even, >= 2; pointers 8-byte aligned), visible[v] (N) uint8 or NULL.  A (V,T,2) tensor of
 *     roma_build_tracks is read in place with obs[v] = x + 2 T v, point_stride = 2;
 *   K, R_in: (V,3,3) fp64 device; t_in: (V,3); X_in: (N,3) fp64 device, the points in the world frame; 16-byte aligned;
 *   fixed: bit v = view v is held; at least one view and not all of them; threshold: pixels, positive; iters: 0 .. 50.
 * Observation (v, n) is OBSERVED when its pixel is finite, visible[v][n] is not 0, view v is usable (K upper triangular with fx fy != 0,
 * K, R, t finite) and X[n] is finite.  Under a state it is WEIGHTED when it is observed, its depth is positive and its squared pixel
 * error e < threshold^2.  cost = sum over the observed of (weighted ? e : threshold^2).
 * Parameters: 6 per free view, R' = exp([w]x) R, t' = exp([w]x) t + tau (the series of the other refinements, rows re-orthonormalised);
 * 3 per point.  Held for a step: the fixed views, the views that are not usable, a free view without a weighted observation; a point
 * with fewer than 2 weighted observations or whose damped 3 x 3 block has a pivot that is not positive.  A held point's weighted
 * observations still enter the camera blocks, the point as a constant.  Gauss-Newton normal equations over the weighted observations,
 * damped A + lambda diag A on the camera and the point blocks; lambda_0 = 1e-3, / 10 on a kept step (floor 1e-10), * 10 otherwise; a
 * step is kept when cost' < cost (1 - 1e-12).  Everything is fp64 and relative to the mean of the centres of the usable views.
 * Outputs, device, all required: R (V,3,3), t (V,3), X (N,3) fp64, 16-byte aligned; mask (V,N) uint8, the weighted observations under
 * the returned state; cost (2) fp64, of the input and of the returned state; count (1) int32, the number of weighted observations;
 * steps (1) int32, the steps kept; status (1) int32: 0, or bit 0 = a pivot of the reduced camera system was not positive, bit 1 = no
 * usable free view, bit 2 = the cost of the input is not finite.  cost[1] <= cost[0] always.  With no step kept, or a status that is
 * not 0, R, t, X are the input bit for bit, steps = 0, and cost[1], mask, count are the input's; a view or a point that was held at
 * every kept step comes back bit for bit as well.
 * workspace: roma_bundle_workspace(V, N, offsets) bytes, 16-byte aligned, need not be initialised; the function (host only) stores
 * the byte offsets of its 11 regions in offsets (may be NULL) — the state record, the view constants, c0 and the camera step, the two
 * pose buffers, the two point buffers, the moved flags, the reduced system, its per-block partials, the partial costs — each a
 * multiple of 256, and returns a negative code for bad V or N.  With n = 6 V and M = n (n + 1) / 2 + 2 n + V the partials take
 * 8 M min(ceil(N / 64), 256) bytes and the points 50 N.
 * 5 + 6 iters launches on `stream`: per step accumulate, reduce, solve, propose, evaluate, decide.  The accept / reject decision is
 * taken on the device; once the state record says finished, every later launch returns at once.  Sums are per-block partials added
 * in block order: no floating-point atomics (count uses an integer one), bitwise reproducible.  No block waits for another, no host
 * synchronisation: the call can be captured in a graph. */
long roma_bundle_workspace(int V, int N, long* offsets);
int roma_bundle_adjust(const float* const* obs, const float* to_px, const unsigned char* const* visible, long point_stride, const double* K,
                       const double* R_in, const double* t_in, const double* X_in, int V, int N, unsigned fixed, double threshold, int iters,
                       double* R, double* t, double* X, unsigned char* mask, double* cost, int* count, int* steps, int* status,
                       void* workspace, long workspace_size, void* stream);

/* Motion averaging (csrc/motion_average.hip): the V cameras of ONE reconstruction from the pairwise poses of its pose
 * graph and its tracks — the start that roma_bundle_adjust polishes.  Two stages, fp64.  A view is x_v ~ K_v (R_v X + t_v)
 * (roma_triangulate_nview); edge m, pairs[m] = (a, b), carries X_b = R_rel X_a + t_rel (roma_recover_pose).  tests/motion_ref.py
 * restates both.
 *
 * roma_rotation_average: the rotations, 2 <= V <= 32 views, 1 <= M <= 4096 edges.
 *   R_rel: (M,3,3) fp64 device, 16-byte aligned; pairs: (M,2) int32; weights: (M) fp64 or NULL (all 1); root: the view whose
 *   rotation is the identity; sigma_deg > 0; iters: 0 .. 50.
 * Edge m is USABLE when a != b, both are in [0, V), R_rel[m] is finite and its weight is finite and positive.  Start: the maximum-
 * weight spanning tree grown from the root — repeatedly the usable edge with exactly one end in the tree and the largest weight, the
 * lowest index on a tie, gives R_b = R_rel R_a or R_a = R_rel^T R_b; R_root = I.  A view that is never reached comes back as NaN with
 * valid = 0.  Then `iters` rounds over the usable edges between reached views:
 *   r_m = log(R_b^T R_rel,m R_a): w = vee(D - D^T) / 2, theta = atan2(|w|, (tr D - 1) / 2), r = w theta / |w| (r = w where |w| < 1e-12);
 *   omega_m = weight_m / max(|r_m|, 1e-3) in the rounds below iters / 2 (integer division: the L1 phase), afterwards
 *     weight_m (s^2 / (s^2 + |r_m|^2))^2 with s = sigma_deg in radians;
 *   the weighted graph Laplacian over the reached views without the root, L[b][b] += omega, L[a][a] += omega, L[a][b] -= omega,
 *     L[b][a] -= omega, rhs[b] += omega r, rhs[a] -= omega r (the rows and columns of the root are left out), solved by Cholesky for
 *     delta (a pivot must be positive and finite);
 *   R_v <- R_v exp([delta_v]x): the series of the other refinements (a delta longer than 1 rad is scaled to 1), rows re-orthonormalised.
 * Outputs, device, all required: R (V,3,3) fp64, 16-byte aligned; valid (V) uint8; residual (M) fp64, |r_m| under the returned state,
 * NaN for an edge that is not usable or not reached (it is the kernel's scratch while it runs); status (1) int32: 0, or bit 0 = a pivot
 * was not positive, and the start comes back.
 * ONE launch of one workgroup of 128 threads (a view x 4 slices of the edges; a Laplacian entry is the sum of its four slices, each in
 * edge order), no workspace, no atomics, no host synchronisation.
 *
 * roma_global_positions: the camera centres and the points under those rotations — the linear known-rotation problem, 3 <= V <= 32
 * views, 1 <= N <= 2^24 points, 1 <= M <= 4096 edges.
 *   obs, to_px, visible, point_stride: the observation table of roma_bundle_adjust, read the same way;
 *   K, R: (V,3,3) fp64 device (R: the output of roma_rotation_average); pairs: (M,2) int32; t_rel: (M,3) fp64, only its direction is
 *   used; root: the view at the origin; threshold: pixels, positive; rounds: 2 .. 8.
 * View v is usable when K_v is upper triangular with fx fy != 0 and K_v, R_v are finite; an observation is SEEN when its pixel is finite,
 * visible[v][n] is not 0 and the view is usable.  Bearing d = R_v^T h / |h| with h = K_v^-1 (x, y, 1); a_v = threshold / sqrt(|fx fy|);
 * P = I - d d^T.  Edge m is usable when a != b are usable views and t_rel[m] is finite and not 0; b_m = -R_b^T t_rel,m / |t_rel,m|.
 * Round-0 weights, a majority vote: for a seen (v, n), every usable edge m that joins v to a view u that also sees n counts (cnt += 1,
 * duplicates too) and agrees (vote += 1) when |(d_vn x d_un) . b_m| < 2 max(a_v, a_u), the cross product left as it is; w = 1 when
 * vote >= 1 and 2 vote >= cnt, else 0.
 * Round r = 0 .. rounds - 1:
 *   A_n = sum_v w P; point n is SOLVED when it was solved in every earlier round, at least two of its weights are positive and
 *     det A_n > 1e-12 (tr A_n)^3; otherwise its weights are 0 from then on;
 *   over the solved points S (3 V x 3 V) gets S_vv += w P and, for all v, u, S_vu -= (w P)_v A_n^-1 (w P)_u; a view is PLACED when it has
 *     a positive weight on a solved point; the rows and columns of the root and of the views that are not placed are taken out;
 *   C = the eigenvector of the smallest eigenvalue (unit norm), C_root = 0;  X_n = A_n^-1 sum_v w P C_v;
 *   when sum w depth < 0 over the weighted observations, C and X change sign (rel = X_n - C_v, depth = rel . d);
 *   dist = |rel|, ang = |P rel| / dist; the next weight = good / (1 + (ang / (a_v 2^max(rounds - 2 - r, 0)))^2) with good = seen, solved,
 *     depth > 0, dist > 1e-12 and, in the rounds r >= rounds - 2 only, ang < a_v.
 * Outputs, device, all required: t (V,3) = -R_v C_v and centres (V,3) fp64, NaN for a view that is not placed; points (N,3) fp64, NaN
 * where not solved in the last round; mask (V,N) uint8, weight > 0 after the last round; count (1) int32, the set mask entries;
 * eigenvalues (2) fp64, the two smallest of the last round; status (1) int32: bit 0 = the second eigenvalue is not positive or not
 * finite, bit 1 = a view was not placed in the last round, bit 2 = the root or all but one view is not placed.  On bit 0 or bit 2
 * every output is NaN or 0.  t, centres, points, eigenvalues 16-byte aligned.
 * workspace: roma_positions_workspace(V, N, M, offsets) bytes, 16-byte aligned, need not be initialised; the function (host only)
 * stores the byte offsets of its 11 regions in offsets (may be NULL) — the state record, the view constants, the centres of two
 * rounds, the edge records, the points of two rounds, the round-0 weights (a bit per view), the solved flags, the reduced matrix, its
 * per-block partials, the partial depth sums — each a multiple of 256, and returns a negative code for a bad V, N or M.  With
 * Ms = 3 V (3 V + 1) / 2 + V the partials take 8 Ms min(ceil(N / 64), 256) bytes and the points 53 N: no weight is ever stored, a
 * weight is a function of the round before.
 * 3 + 5 rounds launches on `stream`: init, vote, per round accumulate, reduce, solve, points, sign, then final.  The sums over the points
 * are per-block partials (kept in LDS while a block walks its points) added in block order: no floating-point atomics (count uses an
 * integer one), bitwise reproducible.  The eigen-solve is one workgroup: two-sided Jacobi in the round-robin order on at most 94 rows,
 * the matrix and its eigenvectors in 141 KB of LDS.  No block waits for another, no host synchronisation: the call can be captured
 * in a graph. */
int roma_rotation_average(const double* R_rel, const int* pairs, const double* weights, int V, int M, int root, double sigma_deg, int iters,
                          double* R, unsigned char* valid, double* residual, int* status, void* stream);
long roma_positions_workspace(int V, int N, int M, long* offsets);
int roma_global_positions(const float* const* obs, const float* to_px, const unsigned char* const* visible, long point_stride, const double* K,
                          const double* R, const int* pairs, const double* t_rel, int V, int N, int M, int root, double threshold, int rounds,
                          double* t, double* centres, double* points, unsigned char* mask, int* count, double* eigenvalues, int* status,
                          void* workspace, long workspace_size, void* stream);

/* Multi-view depth-map fusion (csrc/depth_fuse.hip): the depth maps of V posed views (2 <= V <= 32) checked against
 * one another by forward-backward reprojection, one owner chosen per surface point, and the owners compacted into one cloud.
 * Convention of roma_triangulate_nview: x_v ~ K_v (R_v X + t_v); pixel (row i, column j) of a map is at (u, v) = (j + 0.5, i + 0.5) in
 * the pixels K_v refers to (the caller folds a map-to-image scale into K_v).  tests/fuse_depth_ref.py restates the definition.
 *   depths: HOST table of V device pointers, map v is (H_v, W_v) fp32 contiguous, 4-byte aligned, read in place; a depth that is not a
 *     finite positive number is a hole;  dims: HOST table of 2 V ints, H_v, W_v (1 to 32768 each; all maps together at most 2^31 - 1
 *     pixels);  K, R: (V,3,3), t: (V,3) fp64 device.  A view is usable when K_v is upper triangular with fx fy k22 != 0 and K_v, R_v,
 *     t_v are finite; an unusable view sees nothing and is seen by nothing.
 *   max_reproj_error (pixels of the reference map) and max_depth_error (relative) positive; 2 <= min_views <= V; max_points >= 1.
 * Pass 1, per pixel (r, i, j) with a depth d, every usable s != r in ascending order: X = R_r^T (K_r^-1 (u d, v d, d) - t_r), q = K_s
 * (R_s X + t_s), skip s unless q.z > 0; (u_s, v_s) = q.xy / q.z; d_s = the bilinear sample of map s there (taps floor(u_s - 0.5) and
 * the next, likewise v), skip s unless all four taps are inside the map and none is a hole; p = the projection into r of (u_s, v_s,
 * d_s) lifted from s, skip s unless p.z > 0; s is consistent when |p.xy / p.z - (u, v)| < max_reproj_error and |p.z - d| / d <
 * max_depth_error.  The kernel evaluates q = d M_rs (u, v, 1) + e_rs with M_rs = K_s R_s R_r^T K_r^-1 and e_rs = K_s (t_s - R_s R_r^T
 * t_r) prepared once per pair, everything in fp64: the world's origin cancels in e_rs.
 * Pass 2: a valid pixel is a duplicate when for some s < r with bit s in its views the pixel (floor v_s, floor u_s) of s is valid and
 * has bit r in its views.  Pass 3: the valid pixels that are not duplicates, in the order (view, row, column), fill the cloud.
 * Outputs, device, all required.  Per pixel, flat over the views (view v starts at the sum of the pixel counts before it): depth fp32,
 * the mean of d and the consistent p.z added in view order, 0 where not valid; valid uint8, num_views >= min_views; views int32, bit r
 * and the consistent views' bits (0 for a hole or an unusable view); num_views uint8, its popcount.  The cloud, max_points rows:
 * points (·,3) fp32 = R_r^T (K_r^-1 (u, v, 1) depth - t_r) in fp64 from the fused fp32 depth; view uint8; pixel int32 = i W_r + j;
 * point_views int32; rows from min(counts[0], max_points) on are 0 with pixel = -1.  counts (4) int32: pixels emitted before
 * truncation, valid pixels, duplicates, and a status word that is 0.
 * workspace: roma_depth_fuse_workspace(V, total_pixels, out_bytes) bytes, 16-byte aligned, need not be initialised: one flag per pixel
 * and 12 bytes per block of 1024 pixels (at most total_pixels / 1024 + V blocks), each rounded up to 256; the function (host only)
 * stores the two sizes in out_bytes (may be NULL) and returns a negative code for bad V or total_pixels.
 * Five launches on `stream`: consistency, ownership, the scan of the per-block counts by one workgroup, clear, cloud.  No atomics, no
 * block waits for another, no host synchronisation: bitwise reproducible, and the call can be captured in a graph. */
long roma_depth_fuse_workspace(int V, long total_pixels, long* out_bytes);
int roma_depth_fuse(const float* const* depths, const int* dims, const double* K, const double* R, const double* t, int V,
                    double max_reproj_error, double max_depth_error, int min_views, int max_points, float* depth, unsigned char* valid,
                    int* views, unsigned char* num_views, float* points, unsigned char* view, int* pixel, int* point_views, int* counts,
                    void* workspace, long workspace_size, void* stream);

/* Point-cloud rendering (csrc/render_points.hip): N points drawn into the depth maps of V posed views (1 <= V <= 32) by
 * a z-buffered splat, and per point the views that see it.  Convention of roma_depth_fuse: x_v ~ K_v (R_v X + t_v); pixel (row i,
 * column j) covers [j, j+1) x [i, i+1).  tests/render_points_ref.py restates the definition.
 *   points: (N,3) fp32 device, 4-byte aligned, read in place, 1 <= N <= 2^31 - 1;  mask: (N) uint8 device or NULL.  A point is live
 *     when its three coordinates are finite and mask is NULL or mask[n] != 0;
 *   K, R: (V,3,3), t: (V,3) fp64 device.  A view is usable when K_v is upper triangular with fx fy k22 != 0 and K_v, R_v, t_v are
 *     finite; an unusable view gets an empty map and its bit is never set;
 *   H, W: the shape of every map, 1 to 32768 each, V H W <= 2^31 - 1;  radius: 0 to 4;  depth_tol: finite, >= 0.
 * Projection of a live point into a usable view, fp64 with explicit fused multiply-adds: q = P_v (X, 1) with P_v = K_v [R_v | t_v];
 * skip unless q.z > 0 and q is finite; (u, w) = q.xy (1 / q.z); skip unless 0 <= u < W and 0 <= w < H (tested in floating point before
 * anything becomes an integer); z32 = (float) q.z, skip unless it is finite and > 0; (j, i) = (floor u, floor w).
 * Splat: key = bits(z32) << 32 | n; every pixel (i + di, j + dj), |di|, |dj| <= radius, inside the map takes the unsigned 64-bit
 * minimum of its word (all ones at first) and key: the winner is the nearest point and, on exactly equal z32, the lowest index,
 * whatever order the points arrive in.
 * Outputs, device, all required.  depth (V,H,W) fp32 = the winner's z32, index (V,H,W) int32 = its n; 0.0f and -1 where nothing was
 * drawn.  visible (N) int32: bit v is set when the point projects inside the map of the usable view v and (double) z32 <= (double)
 * depth[v, i, j] (1 + depth_tol) at its own pixel (i, j); num_views (N) uint8 = its popcount; both 0 for a point that is not live.
 * counts (4) int32: projections inside a map, covered pixels, set visibility bits, points that are not live (each modulo 2^32).
 * workspace: roma_render_points_workspace(V, H, W, out_bytes) bytes, 16-byte aligned, need not be initialised: the V H W 64-bit keys,
 * rounded up to 256; the counters are `counts` itself, cleared by the first launch.  The function (host only) stores the size of
 * that one region in out_bytes (may be NULL) and returns a negative code for a bad shape.
 * Four launches on `stream`: clear, splat (grid (ceil(N / 1024), V), four points per thread), resolve, visible.  The only atomics are
 * the 64-bit unsigned min and one integer add per block and count: both commute, so the result is bitwise the same from run to run
 * and under any permutation of the points' arrival.  No block waits for another, no host synchronisation: the call can be captured
 * in a graph. */
long roma_render_points_workspace(int V, int H, int W, long* out_bytes);
int roma_render_points(const float* points, const unsigned char* mask, long N, const double* K, const double* R, const double* t, int V,
                       int H, int W, int radius, double depth_tol, float* depth, int* index, int* visible, unsigned char* num_views,
                       int* counts, void* workspace, long workspace_bytes, void* stream);

/* Ground-truth warp of key-points from two depth maps and a relative pose (csrc/depth_warp.hip): warp_kpts of the
 * reference (romatch/utils/utils.py:358-455; get_gt_warp is this on the pixel grid).  Convention: X_B = R X_A + t, T = [R | t].
 *   x: (P,N,·) fp32 device, 8-byte aligned, normalised key-points of image A in columns 0-1 of rows `x_stride` floats apart: 2 for
 *     packed (P,N,2), 4 to read the first two columns of a (P,N,4) warp; any other stride returns ROMA_E_ARG;
 *   depth_a: (P,Ha,Wa), depth_b: (P,Hb,Wb) fp32, contiguous, 0 = no depth; sides 1 to 32768;
 *   T: (P,3,4) fp64 row major; Ka, Kb: (P,3,3) fp64, any 3x3 (Ka is inverted by its adjugate);
 *   mode: 0 = bilinear, 1 = nearest, 2 = combined; threshold: on the relative depth error, not NaN.
 * Per point, in fp64 from the fp32 inputs widened (the reference casts exactly these to double):
 *   d = depth_a sampled at (x, y) as grid_sample does with align_corners=False and zero padding: ix = ((x + 1) Wa - 1) / 2; bilinear
 *     taps outside the map contribute 0; nearest rounds ix, iy to the nearest integer, ties to even, and gives 0 outside the map;
 *   (px, py) = (Wa (x + 1) / 2, Ha (y + 1) / 2);  X_A = Ka^-1 (px d, py d, d);  X_B = R X_A + t;  z = X_B.z;
 *   (u, v) = (Kb X_B).xy / ((Kb X_B).z + 1e-4);  covisible = 0 < u < Wb - 1 and 0 < v < Hb - 1, all strict;
 *   x2 = (2 u / Wb - 1, 2 v / Hb - 1);  d_B = depth_b sampled at x2 with the same sampler;  rel_err = |(d_B - z) / d_B|;
 *   valid = d != 0 and covisible and rel_err < threshold.
 * IEEE semantics only: a comparison with NaN is false, a zero d_B gives rel_err = inf (NaN when z = 0 too), and such a point is not
 * valid.  A key-point that is NaN, inf or far outside samples 0 (the sampler range-checks in floating point before it forms an index)
 * and is not valid; a singular Ka makes every point of its pair not valid.  mode 2 computes both samplers' results and returns the
 * nearest one (x2 and rel_err) where the bilinear one is not valid and the nearest one is, the bilinear one elsewhere; valid is the OR.
 * Outputs, device, each may be NULL but not all: x2 (P,N,2) fp64, 16-byte aligned, normalised in B; valid (P,N) uint8; rel_err (P,N)
 * fp64.  Every requested element is written (x2 and rel_err may be inf / NaN where valid is 0); an output does not depend on which
 * others are requested, nor a pair on the other pairs.  One launch, no workspace, no atomics, no host synchronisation. */
int roma_warp_kpts(const float* x, int x_stride, const float* depth_a, const float* depth_b, const double* T, const double* Ka,
                   const double* Kb, int P, int N, int Ha, int Wa, int Hb, int Wb, int mode, double threshold, double* x2,
                   unsigned char* valid, double* rel_err, void* stream);

/* End-point error and PCK of a dense warp against that ground truth, fused (csrc/depth_warp.hip): geometric_dist of the reference's
 * MegadepthDenseBenchmark (romatch/benchmarks/megadepth_dense_benchmark.py:17-42).
 *   warp: (P,H,W,4) fp32 device, 16-byte aligned, rows [x_A, y_A, predicted x_B, y_B] normalised; `pitch` is the distance in floats
 *     between image rows (a multiple of 4, >= 4 W; else ROMA_E_ARG) and a pair is H * pitch floats: pitch = 8 W reads the left half
 *     of a symmetric (P,H,2W,4) warp in place.  H, W: 1 to 32768, H * W <= 2^28;
 *   depth_a, depth_b, T, Ka, Kb, Ha, Wa, Hb, Wb, mode, threshold: as roma_warp_kpts.
 * Per pixel: (x2, valid) = the chain of roma_warp_kpts on columns 0-1; x2_px = (W (x2 + 1) / 2, H (y2 + 1) / 2) in fp64 with the W, H
 * of the WARP (as the reference; not those of depth_b); xhat_px = ((W (c2 + 1)) / 2, (H (c3 + 1)) / 2) of columns 2-3 in fp32 in
 * exactly this order (dense_matches is fp32 in the reference), then widened; gd = |xhat_px - x2_px| in fp64.
 * Per pair: epe_sum (P) fp64 = the sum of gd over the valid pixels; counts (P,4) int64 = the number of valid pixels and of those with
 * gd < 1, gd < 3, gd < 5, all strict.  The mean end-point error is epe_sum / counts[0], PCK@k counts[k] / counts[0]; over a batch,
 * the sums of both.  A valid pixel whose prediction is NaN puts NaN into epe_sum and into no count, as the reference's mean would.
 * Optional per-pixel outputs, NULL to skip: gd (P,H,W) fp64 (of every pixel; inf / NaN possible where valid is 0), valid (P,H,W) uint8.
 *   workspace: device, 8-byte aligned, workspace_bytes >= P * ceil(H * W / 1024) * 40 (else ROMA_E_ARG): one 40-byte partial (fp64
 *     sum, four int64 counts) per workgroup of 1024 pixels; need not be initialised.
 * Two launches: the first leaves the partials (wave butterfly, the waves through LDS in order), the second adds each pair's in a
 * fixed order.  No atomics, no host synchronisation; bitwise reproducible, and a pair does not depend on the other pairs. */
int roma_dense_match_metrics(const float* warp, long pitch, const float* depth_a, const float* depth_b, const double* T,
                             const double* Ka, const double* Kb, int P, int H, int W, int Ha, int Wa, int Hb, int Wb, int mode,
                             double threshold, void* workspace, long workspace_bytes, double* epe_sum, long long* counts, double* gd,
                             unsigned char* valid, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* ROMA_HIP_H */
