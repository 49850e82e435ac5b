/* ccst_instnorm.h -- C ABI extension of libccst_hip.so: instance normalisation (InstanceNorm2d, track_running_stats=False) on the
 * ResNet path, fused with the affine map, the residual add and ReLU the way the BatchNorm entry points of ccst_hip.h are
 * (nets/resnet.py:193-232 ResNetIN; federated/fed_run.py:218-229 --IN_test of the reference).
 *
 * Versioned on its own (CCST_INSTNORM_ABI_VERSION), so that the core ABI of ccst_hip.h stays as it is.  The symbols are exported
 * from the same libccst_hip.so and follow the core conventions: int return codes (CCST_OK / CCST_EINVAL / CCST_EWORKSPACE, message
 * in ccst_last_error()), caller-owned device buffers and workspace, `stream` a hipStream_t (NULL = the null stream), nothing
 * synchronises with the host.
 *
 * Tensors are NHWC fp32 [N][HW][C], C % 4 == 0, 16-byte aligned.  Statistics are per (image, channel) over HW: the mean and the
 * BIASED variance, as F.instance_norm takes them, invstd = 1 / sqrt(var + eps).  They are accumulated in fp64 about a per-(image,
 * channel) pivot (the image's first pixel), in split partials summed in a fixed order: results are bitwise reproducible, and an
 * image's statistics, y and dx do not depend on its batch-mates (the split count is a function of HW and C only).  Only dgamma /
 * dbeta sum over the batch, in image order.
 *
 * Bytes moved: the forward reads x twice (statistics, apply) and writes y once, plus the residual read and the mask write where
 * used; the backward reads dy and x twice each and writes dx once, plus d_residual.
 */
#ifndef CCST_INSTNORM_H
#define CCST_INSTNORM_H

#include "ccst_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define CCST_INSTNORM_ABI_VERSION 1

int ccst_instnorm_abi_version(void);

/* Workspace of both entry points for an [N][HW][C] tensor (the per-split fp64 partials and the per-(image, channel) sums). */
int64_t ccst_instnorm_workspace_bytes(int N, int HW, int C);

/* y = [ReLU]((x - mu_nc) * invstd_nc [* gamma_c + beta_c] [+ residual]), evaluated as fma(x - mu, invstd * gamma, beta).
 * gamma = beta = NULL: the non-affine norm (both or neither).  residual: NULL or [N][HW][C].
 * relu_mask: NULL, or [N*HW*C/4] bytes (needs relu = 1): bit j of byte i <-> element 4 i + j is positive before the ReLU, the layout
 *   of ccst_bn_train_fwd_mask_f32.
 * save_mean / save_invstd [N*C] (outputs): the statistics the backward takes.
 * y_absmax: NULL, or zeroed per-tensor |max| words (CCST_ABSMAX_WORDS) receiving max |y| -- what the next half-piece conv scales by.
 * Training and evaluation are the same call (instance statistics in both).  Three launches: split partials, fp64 finalize, apply. */
int ccst_instnorm_fwd_f32(const float* x, const float* gamma, const float* beta, const float* residual, int relu, float* y,
                          uint8_t* relu_mask, float* save_mean, float* save_invstd, int N, int HW, int C, float eps, void* ws,
                          int64_t ws_bytes, uint32_t* y_absmax, void* stream);

/* Backward of ccst_instnorm_fwd_f32.  g = dy masked by the forward's ReLU (relu = 1), the mask taken from relu_mask, else from the saved
 * output y (y > 0), else recomputed from x (fma(x - mu, invstd * gamma, beta) > 0, the forward's own arithmetic: only valid when the
 * forward added no residual; beta is then needed for an affine norm).  With x^ = (x - mu) invstd:
 *     dx = invstd gamma (g - mean_HW(g) - x^ mean_HW(g x^))        (gamma = 1 when NULL)
 *     d_residual = g (NULL: not written)
 *     dgamma_c = sum_n sum_HW g x^,  dbeta_c = sum_n sum_HW g       (NULL: not written; accumulate = 1 adds to them)
 * dx_absmax: NULL, or zeroed |max| words receiving max |dx| -- what the half-piece weight-gradient kernel scales dy by.
 * Four launches: split partials, fp64 finalize per (image, channel), dgamma / dbeta over the batch, apply. */
int ccst_instnorm_bwd_f32(const float* dy, const float* x, const float* y, const uint8_t* relu_mask, int relu, const float* gamma,
                          const float* beta, const float* save_mean, const float* save_invstd, float* dx, float* d_residual,
                          float* dgamma, float* dbeta, int accumulate, int N, int HW, int C, void* ws, int64_t ws_bytes,
                          uint32_t* dx_absmax, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* CCST_INSTNORM_H */
