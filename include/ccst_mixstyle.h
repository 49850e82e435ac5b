/* ccst_mixstyle.h -- C ABI extension of libccst_hip.so: MixStyle (Zhou et al., ICLR 2021; nets/layers.py:6-73 of the reference)
 * on the ResNet training path.
 *
 * Versioned on its own (CCST_MIXSTYLE_ABI_VERSION), so that the core ABI of ccst_hip.h -- and the ctypes stubs written against
 * it -- stays as it is.  The symbols are exported from the same libccst_hip.so and follow the core conventions: int return codes
 * (CCST_OK / CCST_EINVAL / CCST_EWORKSPACE, message in ccst_last_error()), caller-owned device buffers, `stream` a hipStream_t
 * (NULL = the null stream), nothing synchronises with the host.
 *
 * Tensors are NHWC fp32 [N][HW][C], C % 4 == 0, 16-byte aligned.  Per-image mixing draws, on the device:
 *   lam  [N] float -- lambda_n ~ Beta(alpha, alpha)
 *   perm [N] int32 -- the batch-mate image n takes its target statistics from, 0 <= perm[n] < N.  The entry points cannot read
 *                     device memory without a host synchronisation, so the caller validates perm; an index outside [0, N)
 *                     never reads out of bounds: image n's output becomes NaN.
 */
#ifndef CCST_MIXSTYLE_H
#define CCST_MIXSTYLE_H

#include "ccst_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define CCST_MIXSTYLE_ABI_VERSION 1

int ccst_mixstyle_abi_version(void);

/* Training forward.  mean / stdv [N*C] (outputs, kept for the backward): per-(image, channel) mean and sqrt(unbiased variance + eps)
 * over HW, as ccst_calc_mean_std_f32 computes them (HW == 1 gives NaN, as the reference does); a sample's statistics do not depend
 * on its batch-mates.  Then, with mu_mix = mean[n] lam[n] + mean[perm[n]] (1 - lam[n]) and sigma_mix likewise (separately rounded
 * fp32 operations),
 *     y = ((x - mean) / stdv) * sigma_mix + mu_mix
 * ws: ccst_stats_workspace_bytes(N, C, HW) bytes.  y_absmax: NULL, or zeroed per-TENSOR |max| words (CCST_ABSMAX_WORDS) receiving
 * max |y|.  Three launches: split partials, fp64 finalize, one streaming pass (read x, write y). */
int ccst_mixstyle_fwd_f32(const float* x, const float* lam, const int32_t* perm, float* y, float* mean, float* stdv, int N, int C,
                          int HW, float eps, void* ws, int64_t ws_bytes, uint32_t* y_absmax, void* stream);

/* Backward (mean and stdv are detached in the reference): dx = (dy * sigma_mix) / stdv, sigma_mix recomputed from the forward's
 * stdv, lam and perm.  One streaming launch. */
int ccst_mixstyle_bwd_f32(const float* dy, const float* stdv, const float* lam, const int32_t* perm, float* dx, int N, int C, int HW,
                          void* stream);

#ifdef __cplusplus
}
#endif

#endif /* CCST_MIXSTYLE_H */
