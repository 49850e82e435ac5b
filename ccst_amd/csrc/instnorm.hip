// Instance normalisation on NHWC fp32 [N][HW][C] (include/ccst_instnorm.h): InstanceNorm2d of the reference's ResNetIN
// (nets/resnet.py:193-232) and of --IN_test (federated/fed_run.py:218-229), fused with the affine map, the residual add and ReLU.
//
// Both directions are (split partials) -> (fixed-order fp64 finalize per image and channel) -> (one streaming apply pass):
//   forward : partials of (x - p, (x - p)^2) in fp64 about the pivot p = x[n][0][c]  -- no E[x^2] - mu^2 cancellation for the large-mean
//             post-ReLU maps -- then y = fma(x - mu, invstd gamma, beta) [+ residual] [ReLU];       x read twice, y written once
//   backward: partials of (g, g x^) in fp64, the finalize per (image, channel), dgamma / dbeta summed over the images in order, then
//             dx = invstd gamma (g - mean(g) - x^ mean(g x^));                                      dy and x read twice, dx written once
// The split count is a function of (HW, C) only and the workgroup sums run in a fixed order: bitwise reproducible, and image n's
// statistics, y and dx do not depend on its batch-mates.  No float atomics (the |max| words are integer maxima of the output bits).
#include "common.h"
#include "../../include/ccst_instnorm.h"

namespace {

constexpr int TPB = 256;
constexpr int IN_CGB = 16;          // channel groups (float4) per partials workgroup: 256 B of a pixel's record
constexpr int IN_ROWS = 8;          // target rows per row lane and split
constexpr int IN_MAX_SPLITS = 128;
constexpr int IN_UNROLL = 4;

struct InSplit {
    int cgb, PL, gy, S, rows;       // channel groups per workgroup, row lanes, channel blocks, splits, rows per split
};

// a function of (HW, C) only: the partial sums of an image never depend on N
static InSplit in_split(int HW, int C) {
    InSplit s;
    const int cg = C / 4;
    s.cgb = cg < IN_CGB ? cg : IN_CGB;
    s.PL = TPB / s.cgb;
    s.gy = (cg + s.cgb - 1) / s.cgb;
    long long S = ((long long)HW + (long long)s.PL * IN_ROWS - 1) / ((long long)s.PL * IN_ROWS);
    S = S < 1 ? 1 : (S > IN_MAX_SPLITS ? IN_MAX_SPLITS : S);
    s.rows = (int)(((long long)HW + S - 1) / S);
    s.S = (int)((HW + s.rows - 1) / s.rows);            // (no empty split)
    return s;
}

// workgroups per image of the apply kernels: ~IN_UNROLL float4 per thread, and grid x 256 a multiple of the channel-group count
// whenever that is possible (then a thread's channel constants stay in registers)
static int in_apply_blocks(int HW, int C) {
    const int cg = C / 4;
    const long long total4 = (long long)HW * cg;
    long long b = (total4 + (long long)TPB * IN_UNROLL - 1) / ((long long)TPB * IN_UNROLL);
    b = b < 1 ? 1 : (b > 256 ? 256 : b);
    if (cg > TPB && cg % TPB == 0) {
        const long long m = cg / TPB;
        b = (b + m - 1) / m * m;
    }
    return (int)b;
}

// The ReLU mask of the backward.  MASK 0: none, 1: saved output y > 0, 2: recomputed from x (the forward's own fma, no residual),
// 3: the forward's byte mask.
template <int MASK>
__device__ __forceinline__ f32x4 in_masked(f32x4 g, const f32x4 v, const f32x4 o, unsigned bits, const f32x4 mu, const f32x4 a,
                                           const f32x4 b) {
    if (MASK == 3) {
#pragma unroll
        for (int j = 0; j < 4; ++j) g[j] = ((bits >> j) & 1u) ? g[j] : 0.f;
    } else if (MASK == 2) {
#pragma unroll
        for (int j = 0; j < 4; ++j) g[j] = fmaf(v[j] - mu[j], a[j], b[j]) > 0.f ? g[j] : 0.f;
    } else if (MASK == 1) {
#pragma unroll
        for (int j = 0; j < 4; ++j) g[j] = o[j] > 0.f ? g[j] : 0.f;
    }
    return g;
}

// per-(image, channel) constants: mu, a = invstd * gamma, b = beta (gamma / beta NULL: 1 / 0), invstd
__device__ __forceinline__ void in_chan(const float* __restrict__ mean, const float* __restrict__ invstd, const float* __restrict__ gamma,
                                        const float* __restrict__ beta, long long nc, int c, f32x4& mu, f32x4& a, f32x4& b, f32x4& is) {
    mu = *reinterpret_cast<const f32x4*>(mean + nc);
    is = *reinterpret_cast<const f32x4*>(invstd + nc);
    a = gamma ? is * *reinterpret_cast<const f32x4*>(gamma + c) : is;
    b = beta ? *reinterpret_cast<const f32x4*>(beta + c) : f32x4{0.f, 0.f, 0.f, 0.f};
}

// ------------------------------------------------------------------------------------------
// split partials.  grid (S, gy, N), 256 threads = cgb channel groups x PL row lanes.  part: [N][S][2][C] doubles.
// MODE 0 (forward): (sum (x - p), sum (x - p)^2), p = x[n][0][c].
// MODE 1 (backward): (sum g, sum g x^), g = masked dy, x^ = (x - mu) invstd in fp32 (as the apply kernel forms it).
// ------------------------------------------------------------------------------------------
template <int MODE, int MASK>
__global__ __launch_bounds__(TPB) void instnorm_partials_kernel(const float* __restrict__ x, const float* __restrict__ dy,
                                                                const float* __restrict__ y, const unsigned char* __restrict__ rmask,
                                                                const float* __restrict__ mean, const float* __restrict__ invstd,
                                                                const float* __restrict__ gamma, const float* __restrict__ beta,
                                                                double* __restrict__ part, int HW, int C, int S, int rows, int cgb,
                                                                int PL) {
    __shared__ double red[2][4][TPB];
    const int t = threadIdx.x, cl = t % cgb, rl = t / cgb;
    const int cg = C / 4, c4 = blockIdx.y * cgb + cl, s = blockIdx.x, n = blockIdx.z;
    const bool live = rl < PL && c4 < cg;
    double s0[4] = {0., 0., 0., 0.}, s1[4] = {0., 0., 0., 0.};
    if (live) {
        const long long img = (long long)n * HW;
        const int r_end = min(HW, (s + 1) * rows);
        const int c = c4 * 4;
        if (MODE == 0) {
            const f32x4 p = *reinterpret_cast<const f32x4*>(x + img * C + c);
            for (int r = s * rows + rl; r < r_end; r += PL) {
                const f32x4 v = *reinterpret_cast<const f32x4*>(x + (img + r) * C + c);
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const double d = (double)v[j] - (double)p[j];
                    s0[j] += d;
                    s1[j] = fma(d, d, s1[j]);
                }
            }
        } else {
            f32x4 mu, a, b, is;
            in_chan(mean, invstd, gamma, beta, (long long)n * C + c, c, mu, a, b, is);
            const f32x4 z4 = {0.f, 0.f, 0.f, 0.f};
            for (int r = s * rows + rl; r < r_end; r += PL) {
                const long long e = (img + r) * C + c;
                const f32x4 v = *reinterpret_cast<const f32x4*>(x + e);
                const f32x4 g = in_masked<MASK>(*reinterpret_cast<const f32x4*>(dy + e), v,
                                                MASK == 1 ? *reinterpret_cast<const f32x4*>(y + e) : z4,
                                                MASK == 3 ? (unsigned)rmask[e >> 2] : 0u, mu, a, b);
                const f32x4 xh = (v - mu) * is;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    s0[j] += (double)g[j];
                    s1[j] += (double)(g[j] * xh[j]);
                }
            }
        }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        red[0][j][t] = s0[j];
        red[1][j][t] = s1[j];
    }
    __syncthreads();
    if (rl == 0 && c4 < cg) {           // fixed order over the row lanes
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            double a0 = 0., a1 = 0.;
            for (int l = 0; l < PL; ++l) {
                a0 += red[0][j][l * cgb + cl];
                a1 += red[1][j][l * cgb + cl];
            }
            double* o = part + (((long long)n * S + s) * 2) * C + c4 * 4 + j;
            o[0] = a0;
            o[C] = a1;
        }
    }
}

// forward finalize, one thread per (image, channel): mean = p + E[x - p], biased var = E[(x - p)^2] - E[x - p]^2 (fp64)
__global__ __launch_bounds__(TPB) void instnorm_fwd_finalize_kernel(const float* __restrict__ x, const double* __restrict__ part,
                                                                    float* __restrict__ mean, float* __restrict__ invstd, int N, int HW,
                                                                    int C, int S, float eps) {
    const long long i = (long long)blockIdx.x * TPB + threadIdx.x;
    if (i >= (long long)N * C) return;
    const int n = (int)(i / C), c = (int)(i % C);
    double a = 0., q = 0.;
    for (int s = 0; s < S; ++s) {
        const double* p = part + (((long long)n * S + s) * 2) * C + c;
        a += p[0];
        q += p[C];
    }
    const double m = a / HW;
    double var = q / HW - m * m;
    var = var > 0. ? var : 0.;
    mean[i] = (float)((double)x[(long long)n * HW * C + c] + m);
    invstd[i] = (float)(1.0 / sqrt(var + (double)eps));
}

// backward finalize, one thread per (image, channel): sums [N][2][C] doubles = (sum g, sum g x^)
__global__ __launch_bounds__(TPB) void instnorm_bwd_finalize_kernel(const double* __restrict__ part, double* __restrict__ sums, int N,
                                                                    int C, int S) {
    const long long i = (long long)blockIdx.x * TPB + threadIdx.x;
    if (i >= (long long)N * C) return;
    const int n = (int)(i / C), c = (int)(i % C);
    double a = 0., b = 0.;
    for (int s = 0; s < S; ++s) {
        const double* p = part + (((long long)n * S + s) * 2) * C + c;
        a += p[0];
        b += p[C];
    }
    sums[((long long)n * 2) * C + c] = a;
    sums[((long long)n * 2 + 1) * C + c] = b;
}

// dgamma / dbeta, one thread per channel: the images in order
__global__ __launch_bounds__(TPB) void instnorm_dgamma_kernel(const double* __restrict__ sums, float* __restrict__ dgamma,
                                                              float* __restrict__ dbeta, int N, int C, int accumulate) {
    const int c = blockIdx.x * TPB + threadIdx.x;
    if (c >= C) return;
    double g = 0., b = 0.;
    for (int n = 0; n < N; ++n) {
        b += sums[((long long)n * 2) * C + c];
        g += sums[((long long)n * 2 + 1) * C + c];
    }
    if (dgamma) dgamma[c] = accumulate ? dgamma[c] + (float)g : (float)g;
    if (dbeta) dbeta[c] = accumulate ? dbeta[c] + (float)b : (float)b;
}

// ------------------------------------------------------------------------------------------
// streaming apply passes: grid (blocks per image, N); a thread walks float4 index i of its image with the grid's stride
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(TPB) void instnorm_fwd_apply_kernel(const float* __restrict__ x, const float* __restrict__ mean,
                                                                 const float* __restrict__ invstd, const float* __restrict__ gamma,
                                                                 const float* __restrict__ beta, const float* __restrict__ residual,
                                                                 int relu, float* __restrict__ y, unsigned char* __restrict__ rmask,
                                                                 int HW, int C, unsigned* __restrict__ ymax) {
    const int cg = C / 4, n = blockIdx.y;
    const long long total4 = (long long)HW * cg, base4 = (long long)n * total4;
    const long long stride = (long long)gridDim.x * TPB;
    const long long i0 = (long long)blockIdx.x * TPB + threadIdx.x;
    float amax = 0.f;
    const f32x4 z4 = {0.f, 0.f, 0.f, 0.f};
    auto finish = [&](const f32x4 v, const f32x4 r, const f32x4 mu, const f32x4 a, const f32x4 b, long long i) {
        f32x4 o;
#pragma unroll
        for (int j = 0; j < 4; ++j) o[j] = fmaf(v[j] - mu[j], a[j], b[j]);
        if (residual) o += r;
        if (relu) {
            if (rmask) rmask[base4 + i] = (unsigned char)((o[0] > 0.f ? 1u : 0u) | (o[1] > 0.f ? 2u : 0u) | (o[2] > 0.f ? 4u : 0u) | (o[3] > 0.f ? 8u : 0u));
#pragma unroll
            for (int j = 0; j < 4; ++j) o[j] = fmaxf(o[j], 0.f);
        }
        amax = fmaxf(fmaxf(fmaxf(amax, fabsf(o[0])), fmaxf(fabsf(o[1]), fabsf(o[2]))), fabsf(o[3]));
        *reinterpret_cast<f32x4*>(y + (base4 + i) * 4) = o;
    };
    auto load = [&](const float* p, long long i) { return *reinterpret_cast<const f32x4*>(p + (base4 + i) * 4); };
    if (stride % cg == 0) {         // (uniform) this thread's channels are fixed
        f32x4 mu, a, b, is;
        const int c = (int)(i0 % cg) * 4;
        in_chan(mean, invstd, gamma, beta, (long long)n * C + c, c, mu, a, b, is);
        long long i = i0;
        for (; i + (IN_UNROLL - 1) * stride < total4; i += IN_UNROLL * stride) {
            f32x4 v[IN_UNROLL], r[IN_UNROLL];
#pragma unroll
            for (int u = 0; u < IN_UNROLL; ++u) v[u] = load(x, i + u * stride);
#pragma unroll
            for (int u = 0; u < IN_UNROLL; ++u) r[u] = residual ? load(residual, i + u * stride) : z4;
#pragma unroll
            for (int u = 0; u < IN_UNROLL; ++u) finish(v[u], r[u], mu, a, b, i + u * stride);
        }
        for (; i < total4; i += stride) finish(load(x, i), residual ? load(residual, i) : z4, mu, a, b, i);
    } else {
        for (long long i = i0; i < total4; i += stride) {
            f32x4 mu, a, b, is;
            const int c = (int)(i % cg) * 4;
            in_chan(mean, invstd, gamma, beta, (long long)n * C + c, c, mu, a, b, is);
            finish(load(x, i), residual ? load(residual, i) : z4, mu, a, b, i);
        }
    }
    if (ymax != nullptr) ccst_absmax_publish(ymax, amax, blockIdx.y * gridDim.x + blockIdx.x);
}

template <int MASK>
__global__ __launch_bounds__(TPB) void instnorm_bwd_apply_kernel(const float* __restrict__ dy, const float* __restrict__ x,
                                                                 const float* __restrict__ y, const unsigned char* __restrict__ rmask,
                                                                 const float* __restrict__ mean, const float* __restrict__ invstd,
                                                                 const float* __restrict__ gamma, const float* __restrict__ beta,
                                                                 const double* __restrict__ sums, float* __restrict__ dx,
                                                                 float* __restrict__ dres, int HW, int C, unsigned* __restrict__ dxmax) {
    const int cg = C / 4, n = blockIdx.y;
    const long long total4 = (long long)HW * cg, base4 = (long long)n * total4;
    const long long stride = (long long)gridDim.x * TPB;
    const long long i0 = (long long)blockIdx.x * TPB + threadIdx.x;
    float amax = 0.f;
    const f32x4 z4 = {0.f, 0.f, 0.f, 0.f};
    struct Chan {
        f32x4 mu, a, b, is, k1, k2;         // k1 = mean(g), k2 = mean(g x^)
    };
    auto chan = [&](int c, Chan& k) {
        in_chan(mean, invstd, gamma, beta, (long long)n * C + c, c, k.mu, k.a, k.b, k.is);
        const double* sg = sums + ((long long)n * 2) * C + c;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            k.k1[j] = (float)(sg[j] / HW);
            k.k2[j] = (float)(sg[C + j] / HW);
        }
    };
    auto one = [&](long long i, const Chan& k) {
        const long long e = (base4 + i) * 4;
        const f32x4 v = *reinterpret_cast<const f32x4*>(x + e);
        const f32x4 g = in_masked<MASK>(*reinterpret_cast<const f32x4*>(dy + e), v, MASK == 1 ? *reinterpret_cast<const f32x4*>(y + e) : z4,
                                        MASK == 3 ? (unsigned)rmask[base4 + i] : 0u, k.mu, k.a, k.b);
        if (dres) *reinterpret_cast<f32x4*>(dres + e) = g;
        const f32x4 xh = (v - k.mu) * k.is;
        const f32x4 d = k.a * (g - k.k1 - xh * k.k2);
        amax = fmaxf(fmaxf(fmaxf(amax, fabsf(d[0])), fmaxf(fabsf(d[1]), fabsf(d[2]))), fabsf(d[3]));
        *reinterpret_cast<f32x4*>(dx + e) = d;
    };
    if (stride % cg == 0) {
        Chan k;
        chan((int)(i0 % cg) * 4, k);
        for (long long i = i0; i < total4; i += stride) one(i, k);
    } else {
        for (long long i = i0; i < total4; i += stride) {
            Chan k;
            chan((int)(i % cg) * 4, k);
            one(i, k);
        }
    }
    if (dxmax != nullptr) ccst_absmax_publish(dxmax, amax, blockIdx.y * gridDim.x + blockIdx.x);
}

static int instnorm_check(const void* x, const void* y, int N, int HW, int C, const float* gamma, const float* beta, const char* what) {
    CCST_REQUIRE(x && y, "%s: null pointer", what);
    CCST_REQUIRE(N > 0 && N <= 65535 && HW > 0 && C > 0 && C % 4 == 0, "%s: bad shape N=%d HW=%d C=%d (NHWC, C %% 4 == 0)", what, N, HW, C);
    CCST_REQUIRE((long long)N * HW * C < (1LL << 40), "%s: tensor too large", what);
    CCST_REQUIRE(((uintptr_t)x | (uintptr_t)y | (uintptr_t)gamma | (uintptr_t)beta) % 16 == 0, "%s: tensors must be 16-byte aligned", what);
    return CCST_OK;
}

}  // namespace

extern "C" int ccst_instnorm_abi_version(void) { return CCST_INSTNORM_ABI_VERSION; }

extern "C" int64_t ccst_instnorm_workspace_bytes(int N, int HW, int C) {
    if (N <= 0 || HW <= 0 || C <= 0 || C % 4 != 0) return 0;
    const InSplit sp = in_split(HW, C);
    return ((int64_t)N * sp.S * 2 * C + (int64_t)N * 2 * C) * (int64_t)sizeof(double);
}

extern "C" int ccst_instnorm_fwd_f32(const float* x, const float* gamma, const float* beta, const float* residual, int relu, float* y,
                                     uint8_t* relu_mask, float* save_mean, float* save_invstd, int N, int HW, int C, float eps, void* ws,
                                     int64_t ws_bytes, uint32_t* y_absmax, void* stream) {
    int rc = instnorm_check(x, y, N, HW, C, gamma, beta, "instnorm_fwd");
    if (rc) return rc;
    CCST_REQUIRE((gamma == nullptr) == (beta == nullptr), "instnorm_fwd: gamma and beta come together (affine) or not at all");
    CCST_REQUIRE(save_mean && save_invstd && ws, "instnorm_fwd: null pointer");
    CCST_REQUIRE(((uintptr_t)save_mean | (uintptr_t)save_invstd | (uintptr_t)residual | (uintptr_t)ws) % 16 == 0,
                 "instnorm_fwd: statistics, residual and workspace must be 16-byte aligned");
    CCST_REQUIRE(!relu_mask || relu, "instnorm_fwd: a ReLU mask needs relu=1");
    if (ws_bytes < ccst_instnorm_workspace_bytes(N, HW, C)) {
        ccst_set_error("instnorm_fwd: workspace %lld < %lld", (long long)ws_bytes, (long long)ccst_instnorm_workspace_bytes(N, HW, C));
        return CCST_EWORKSPACE;
    }
    hipStream_t st = (hipStream_t)stream;
    const InSplit sp = in_split(HW, C);
    double* part = (double*)ws;
    hipLaunchKernelGGL((instnorm_partials_kernel<0, 0>), dim3(sp.S, sp.gy, N), dim3(TPB), 0, st, x, nullptr, nullptr, nullptr, nullptr,
                       nullptr, nullptr, nullptr, part, HW, C, sp.S, sp.rows, sp.cgb, sp.PL);
    const long long nc = (long long)N * C;
    hipLaunchKernelGGL(instnorm_fwd_finalize_kernel, dim3((unsigned)((nc + TPB - 1) / TPB)), dim3(TPB), 0, st, x, part, save_mean,
                       save_invstd, N, HW, C, sp.S, eps);
    hipLaunchKernelGGL(instnorm_fwd_apply_kernel, dim3(in_apply_blocks(HW, C), N), dim3(TPB), 0, st, x, save_mean, save_invstd, gamma, beta,
                       residual, relu, y, relu_mask, HW, C, y_absmax);
    return ccst_launch_status("instnorm_fwd");
}

extern "C" int ccst_instnorm_bwd_f32(const float* dy, const float* x, const float* y, const uint8_t* relu_mask, int relu, const float* gamma,
                                     const float* beta, const float* save_mean, const float* save_invstd, float* dx, float* d_residual,
                                     float* dgamma, float* dbeta, int accumulate, int N, int HW, int C, void* ws, int64_t ws_bytes,
                                     uint32_t* dx_absmax, void* stream) {
    int rc = instnorm_check(dy, dx, N, HW, C, gamma, beta, "instnorm_bwd");
    if (rc) return rc;
    CCST_REQUIRE(x && save_mean && save_invstd && ws, "instnorm_bwd: null pointer");
    CCST_REQUIRE(((uintptr_t)x | (uintptr_t)y | (uintptr_t)save_mean | (uintptr_t)save_invstd | (uintptr_t)d_residual | (uintptr_t)ws) % 16 == 0,
                 "instnorm_bwd: tensors, statistics and workspace must be 16-byte aligned");
    CCST_REQUIRE(!relu || relu_mask || y || !gamma || beta,
                 "instnorm_bwd: relu=1 needs the forward's mask, the saved output y, or beta to recompute the mask from x");
    CCST_REQUIRE(!(relu && d_residual && !y && !relu_mask),
                 "instnorm_bwd: with a residual the ReLU mask must come from the forward (mask or saved output y)");
    CCST_REQUIRE(!((dgamma || dbeta) && !gamma), "instnorm_bwd: dgamma / dbeta of a non-affine norm");
    if (ws_bytes < ccst_instnorm_workspace_bytes(N, HW, C)) {
        ccst_set_error("instnorm_bwd: workspace %lld < %lld", (long long)ws_bytes, (long long)ccst_instnorm_workspace_bytes(N, HW, C));
        return CCST_EWORKSPACE;
    }
    hipStream_t st = (hipStream_t)stream;
    const InSplit sp = in_split(HW, C);
    double* part = (double*)ws;
    double* sums = part + (int64_t)N * sp.S * 2 * C;
    const int mask = !relu ? 0 : (relu_mask ? 3 : (y ? 1 : 2));
#define CCST_IN_PARTIALS(MK)                                                                                                           \
    hipLaunchKernelGGL((instnorm_partials_kernel<1, MK>), dim3(sp.S, sp.gy, N), dim3(TPB), 0, st, x, dy, y, relu_mask, save_mean,        \
                       save_invstd, gamma, beta, part, HW, C, sp.S, sp.rows, sp.cgb, sp.PL)
    if (mask == 0) CCST_IN_PARTIALS(0);
    else if (mask == 1) CCST_IN_PARTIALS(1);
    else if (mask == 2) CCST_IN_PARTIALS(2);
    else CCST_IN_PARTIALS(3);
#undef CCST_IN_PARTIALS
    const long long nc = (long long)N * C;
    hipLaunchKernelGGL(instnorm_bwd_finalize_kernel, dim3((unsigned)((nc + TPB - 1) / TPB)), dim3(TPB), 0, st, part, sums, N, C, sp.S);
    if (dgamma || dbeta)
        hipLaunchKernelGGL(instnorm_dgamma_kernel, dim3((C + TPB - 1) / TPB), dim3(TPB), 0, st, sums, dgamma, dbeta, N, C, accumulate);
#define CCST_IN_APPLY(MK)                                                                                                              \
    hipLaunchKernelGGL((instnorm_bwd_apply_kernel<MK>), dim3(in_apply_blocks(HW, C), N), dim3(TPB), 0, st, dy, x, y, relu_mask, save_mean, \
                       save_invstd, gamma, beta, sums, dx, d_residual, HW, C, dx_absmax)
    if (mask == 0) CCST_IN_APPLY(0);
    else if (mask == 1) CCST_IN_APPLY(1);
    else if (mask == 2) CCST_IN_APPLY(2);
    else CCST_IN_APPLY(3);
#undef CCST_IN_APPLY
    return ccst_launch_status("instnorm_bwd");
}
