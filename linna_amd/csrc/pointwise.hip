// Element-wise and reduction kernels of the LINNA hot path for gfx950: prior map + input
// transform, Gaussian log-likelihood reductions (wavefront-shuffle), chi^2-ratio loss
// pieces, AdamW, bias-gradient column sums, Philox-driven ensemble / HMC moves.
// All HBM-bound: coalesced row reads, 64-lane shuffle reductions, no LDS round trips
// except the cross-wave column sum.
#include "common.h"
#include <string.h>
#include <math.h>

namespace linna {

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

static inline dim3 grid1d(size_t n, int block) { return dim3((unsigned)((n + block - 1) / block)); }

// ------------------------------------------------------------------ prior map (util.py:339-347, 483-497)
__device__ __forceinline__ float prior_theta(float z, int flat, float a1, float a2) {
    if (flat) return (0.5f * (1.f + erff(z / 1.41421356237309515f))) * a2 + a1;   // a2 = hi - lo
    return z * a2 + a1;
}

__global__ void prior_map_fwd_kernel(const float* __restrict__ Z, int ldz, int B, int nin,
                                     const int* __restrict__ is_flat, const float* __restrict__ a1,
                                     const float* __restrict__ a2, const int* __restrict__ lg,
                                     const float* __restrict__ xmean, const float* __restrict__ xstd,
                                     float* __restrict__ X, int ldx, float* __restrict__ TH, int ldt) {
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (size_t)B * ldx) return;
    const int row = (int)(idx / ldx), col = (int)(idx % ldx);
    if (col >= nin) { X[idx] = 0.f; return; }
    const float z = Z[(size_t)row * ldz + col];
    const float th = prior_theta(z, is_flat[col], a1[col], a2[col]);
    if (TH) TH[(size_t)row * ldt + col] = th;
    const float t = (lg && lg[col]) ? log10f(th) : th;
    const float x = (t - xmean[col]) / xstd[col];
    X[idx] = isfinite(x) ? x : __builtin_nanf("");   // log10 of theta <= 0: a NaN reaches every output of the row (lnP = -inf)
}

__global__ void prior_map_bwd_kernel(const float* __restrict__ Z, int ldz, int B, int nin,
                                     const int* __restrict__ is_flat, const float* __restrict__ a1,
                                     const float* __restrict__ a2, const int* __restrict__ lg,
                                     const float* __restrict__ xstd, const float* __restrict__ dX, int lddx,
                                     float* __restrict__ dZ, int lddz) {
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (size_t)B * nin) return;
    const int row = (int)(idx / nin), col = (int)(idx % nin);
    const float z = Z[(size_t)row * ldz + col];
    const int flat = is_flat[col];
    float g = dX[(size_t)row * lddx + col] / xstd[col];
    if (lg && lg[col]) g = g / (prior_theta(z, flat, a1[col], a2[col]) * 2.30258509299404568f);
    const float dth = flat ? a2[col] * (expf(-0.5f * z * z) * 0.398942280401432678f) : a2[col];
    dZ[(size_t)row * lddz + col] = g * dth - z;
}

// ------------------------------------------------------------------ Gaussian log-likelihood
// LPR lanes per walker row (a power of two: 64 for wide rows, down to 1): a wavefront covers 64/LPR
// rows, so a 33-wide row costs 16 lanes, not a whole wavefront of mostly idle ones.  Coalesced
// 16-byte reads of d, w and z when the rows are 16-byte aligned (ld multiple of 4), shuffle
// reduction over the LPR lanes of a row.
// out = (-0.5 * sum_j (d_j w_j) d_j)/T - 0.5 sum z^2 ; NaN -> -inf (util.py:953-955,1013-1016,1165)
template <int LPR>
__global__ __launch_bounds__(256) void loglike_diag_kernel(const float* __restrict__ D, int ldd, int B, int nout,
                                                           const float* __restrict__ w,
                                                           const float* __restrict__ Z, int ldz, int nin,
                                                           float T, float* __restrict__ out) {
    constexpr int RPW = 64 / LPR;                                  // rows per wavefront
    const int lane = threadIdx.x & 63, sub = lane % LPR;
    const int row = (blockIdx.x * 4 + (threadIdx.x >> 6)) * RPW + lane / LPR;
    const bool rok = row < B;
    const int r = rok ? row : B - 1;                               // idle lanes read a valid row, store nothing
    const float* d = D + (size_t)r * ldd;
    const float* z = Z + (size_t)r * ldz;
    float acc = 0.f, zz = 0.f;
    const bool al = (ldd & 3) == 0 && ((reinterpret_cast<uintptr_t>(D) | reinterpret_cast<uintptr_t>(w)) & 15) == 0;
    if (al) {
        for (int j = sub * 4; j < nout; j += LPR * 4) {
            const f32x4 dv = *reinterpret_cast<const f32x4*>(d + j);   // (row padded to a multiple of 4: in bounds)
            if (j + 3 < nout) {
                const f32x4 wv = *reinterpret_cast<const f32x4*>(w + j);
#pragma unroll
                for (int e = 0; e < 4; ++e) acc += (dv[e] * wv[e]) * dv[e];
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e) if (j + e < nout) acc += (dv[e] * w[j + e]) * dv[e];
            }
        }
    } else {
        for (int j = sub; j < nout; j += LPR) { const float dv = d[j]; acc += (dv * w[j]) * dv; }
    }
    if ((ldz & 3) == 0 && (reinterpret_cast<uintptr_t>(Z) & 15) == 0) {
        for (int j = sub * 4; j < nin; j += LPR * 4) {
            const f32x4 zv = *reinterpret_cast<const f32x4*>(z + j);
#pragma unroll
            for (int e = 0; e < 4; ++e) if (j + e < nin) zz += zv[e] * zv[e];
        }
    } else {
        for (int j = sub; j < nin; j += LPR) { const float zv = z[j]; zz += zv * zv; }
    }
#pragma unroll
    for (int o = LPR / 2; o >= 1; o >>= 1) { acc += __shfl_xor(acc, o, 64); zz += __shfl_xor(zz, o, 64); }
    if (sub == 0 && rok) {
        const float v = (-0.5f * acc) / T + (-0.5f * zz);
        out[row] = isnan(v) ? -INFINITY : v;
    }
}

__global__ __launch_bounds__(256) void loglike_finish_kernel(const float* __restrict__ partial, int slots_ld, int nslots,
                                                             int B, const float* __restrict__ Z, int ldz, int nin,
                                                             float T, float* __restrict__ out) {
    const int lane = threadIdx.x & 63, row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= B) return;
    float acc = 0.f, zz = 0.f;
    for (int s = lane; s < nslots; s += 64) acc += partial[(size_t)row * slots_ld + s];
    for (int j = lane; j < nin; j += 64) { const float zv = Z[(size_t)row * ldz + j]; zz += zv * zv; }
    acc = wave_sum(acc);
    zz = wave_sum(zz);
    if (lane == 0) {
        const float v = (-0.5f * acc) / T + (-0.5f * zz);
        out[row] = isnan(v) ? -INFINITY : v;
    }
}

// dH = -(1/T) * gscale_j * w_j * d_j   (gradient of the diagonal log-likelihood wrt raw net output)
__global__ void loglike_diag_grad_kernel(const float* __restrict__ D, int ldd, int B, int nout,
                                         const float* __restrict__ w, const float* __restrict__ gscale,
                                         float T, float* __restrict__ dH, int lddh) {
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (size_t)B * lddh) return;
    const int row = (int)(idx / lddh), col = (int)(idx % lddh);
    dH[idx] = col < nout ? -(D[(size_t)row * ldd + col] * w[col]) * gscale[col] / T : 0.f;
}

// ------------------------------------------------------------------ chi^2-ratio loss pieces (util.py:1070-1088)
// mode 0: delta = ynorm - pred ; mode 1: ynorm - data_norm ; mode 2: pred - data_norm ; masked -> 0
__global__ void loss_delta_kernel(int mode, const float* __restrict__ PRED, int ldp, const float* __restrict__ Y, int ldy,
                                  const int* __restrict__ ROWS, int B, int nout, const float* __restrict__ sigma,
                                  const float* __restrict__ ymean, const float* __restrict__ ystd, int ylog,
                                  const float* __restrict__ data_norm, float* __restrict__ DELTA, int ldd) {
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (size_t)B * ldd) return;
    const int i = (int)(idx / ldd), j = (int)(idx % ldd);
    if (j >= nout) { DELTA[idx] = 0.f; return; }
    const int r = ROWS ? ROWS[i] : i;
    const float y = Y[(size_t)r * ldy + j];
    const float dn = data_norm[j];
    const bool masked = (y == 1e-30f) | (y == 1e10f) | (dn == 1e-30f);
    const float yn = ((ylog ? logf(y / sigma[j]) : y / sigma[j]) - ymean[j]) / ystd[j];   // ylog: util.py:567-571 (ypositive)
    float v;
    if (mode == 0) v = yn - PRED[(size_t)i * ldp + j];
    else if (mode == 1) v = yn - dn;
    else v = PRED[(size_t)i * ldp + j] - dn;
    DELTA[idx] = masked ? 0.f : v;
}

// Normalised targets of a whole data set, once: YN = (y / sigma - ymean) / ystd (loss_delta_kernel's formula), NaN where
// the element is masked (util.py:1072) -- what the one-launch training forward subtracts its prediction from.
__global__ void loss_targets_kernel(const float* __restrict__ Y, int ldy, int n, int nout, const float* __restrict__ sigma,
                                    const float* __restrict__ ymean, const float* __restrict__ ystd, int ylog,
                                    const float* __restrict__ data_norm, float* __restrict__ YN, int ldyn) {
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (size_t)n * ldyn) return;
    const int i = (int)(idx / ldyn), j = (int)(idx % ldyn);
    if (j >= nout) { YN[idx] = 0.f; return; }
    const float y = Y[(size_t)i * ldy + j];
    const bool masked = (y == 1e-30f) | (y == 1e10f) | (data_norm[j] == 1e-30f);
    YN[idx] = masked ? __builtin_nanf("") : ((ylog ? logf(y / sigma[j]) : y / sigma[j]) - ymean[j]) / ystd[j];
}

// chi2_b = sum_s partial[b][s]; mode 0: out[b] = max(chi2, floor) (denominator, util.py:1086)
// mode 1: out[b] = chi2 / den[r]
__global__ void loss_rows_kernel(int mode, const float* __restrict__ partial, int slots_ld, int nslots, int B,
                                 const float* __restrict__ den, const int* __restrict__ ROWS, float floorv,
                                 float* __restrict__ out) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    float c = 0.f;
    for (int s = 0; s < nslots; ++s) c += partial[(size_t)b * slots_ld + s];
    if (mode == 0) out[b] = c < floorv ? floorv : c;
    else out[b] = c / den[ROWS ? ROWS[b] : b];
}

// dPRED[i][j] = masked ? 0 : -2 * U[i][j] * inv_batch / den   (U = delta Cinv, Cinv symmetric)
__global__ void loss_grad_kernel(const float* __restrict__ U, int ldu, const float* __restrict__ Y, int ldy,
                                 const int* __restrict__ ROWS, int B, int nout, const float* __restrict__ data_norm,
                                 const float* __restrict__ den, float inv_batch, float* __restrict__ dP, int lddp) {
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (size_t)B * lddp) return;
    const int i = (int)(idx / lddp), j = (int)(idx % lddp);
    if (j >= nout) { dP[idx] = 0.f; return; }
    const int r = ROWS ? ROWS[i] : i;
    const float y = Y[(size_t)r * ldy + j];
    const bool masked = (y == 1e-30f) | (y == 1e10f) | (data_norm[j] == 1e-30f);
    dP[idx] = masked ? 0.f : (-2.f * U[(size_t)i * ldu + j]) * inv_batch / den[r];
}

// The whole chi2-ratio loss of a minibatch (util.py:1070-1116) for nout <= 64 in ONE launch: one wave per row, lane j
// owns column j.  delta (loss_delta_kernel, mode 0), U = delta Cinv from a copy of Cinv in LDS (k-loop, delta_k by
// shuffle), chi2 = delta . U (wave sum), loss_b = chi2 / den, d loss / d pred (loss_grad_kernel), and the batch mean:
// the block that arrives last sums loss_rows in index order (same value whatever the arrival order).
// `counter` is a zeroed int that wraps back to zero by itself (atomicInc).
__global__ __launch_bounds__(256) void loss_fused_small_kernel(
        const float* __restrict__ PRED, int ldp, const float* __restrict__ Y, int ldy, const int* __restrict__ ROWS, int B,
        int nout, const float* __restrict__ sigma, const float* __restrict__ ymean, const float* __restrict__ ystd, int ylog,
        const float* __restrict__ data_norm, const float* __restrict__ Cinv, int ldc, const float* __restrict__ den,
        float inv_batch, float* __restrict__ loss_rows, float* __restrict__ loss_mean, float* __restrict__ dP, int lddp,
        unsigned* counter) {
    __shared__ float C[64 * 65];
    __shared__ float part[4];
    __shared__ int last;
    for (int i = threadIdx.x; i < nout * nout; i += 256) C[(i / nout) * 65 + (i % nout)] = Cinv[(size_t)(i / nout) * ldc + (i % nout)];
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int b = blockIdx.x * 4 + wave;
    if (b < B) {
        const int r = ROWS ? ROWS[b] : b;
        const bool in = lane < nout;
        const int j = in ? lane : 0;
        const float y = Y[(size_t)r * ldy + j], dn = data_norm[j];
        const bool masked = !in | (y == 1e-30f) | (y == 1e10f) | (dn == 1e-30f);
        const float yn = ((ylog ? logf(y / sigma[j]) : y / sigma[j]) - ymean[j]) / ystd[j];
        const float delta = masked ? 0.f : yn - PRED[(size_t)b * ldp + j];
        float u = 0.f;
        for (int k = 0; k < nout; ++k) u += __shfl(delta, k, 64) * C[k * 65 + j];
        const float chi = wave_sum(in ? delta * u : 0.f);
        const float dr = den[r];
        if (lane == 0) loss_rows[b] = chi / dr;
        if (dP && lane < lddp) dP[(size_t)b * lddp + lane] = masked ? 0.f : (-2.f * u) * inv_batch / dr;
        if (dP) for (int c = 64 + lane; c < lddp; c += 64) dP[(size_t)b * lddp + c] = 0.f;   // pad columns past the wave: zero, as loss_grad_kernel leaves them
    }
    if (!loss_mean) return;
    __threadfence();
    __syncthreads();
    if (threadIdx.x == 0) last = atomicInc(counter, gridDim.x - 1) == gridDim.x - 1;
    __syncthreads();
    if (!last) return;
    __threadfence();
    float acc = 0.f;
    for (int i = threadIdx.x; i < B; i += 256) acc += __builtin_nontemporal_load(loss_rows + i);
    acc = wave_sum(acc);
    if (lane == 0) part[wave] = acc;
    __syncthreads();
    if (threadIdx.x == 0) loss_mean[0] = (((part[0] + part[1]) + part[2]) + part[3]) * inv_batch;
}

// deterministic single-block sum: out[0] = scale * sum_i v[i]
__global__ __launch_bounds__(1024) void sum_scale_kernel(const float* __restrict__ v, int n, float scale, float* __restrict__ out) {
    __shared__ float part[16];
    float acc = 0.f;
    for (int i = threadIdx.x; i < n; i += 1024) acc += v[i];
    acc = wave_sum(acc);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        float t = 0.f;
        for (int w = 0; w < 16; ++w) t += part[w];
        out[0] = t * scale;
    }
}
// The same with the AdamW step counter and bias corrections advanced on the side (adamw_prepare_kernel): both are
// single-thread jobs of every optimiser step, one launch instead of two.
__global__ __launch_bounds__(1024) void sum_scale_prepare_kernel(const float* __restrict__ v, int n, float scale, float* __restrict__ out,
                                                                 int* step, float* hyper, float beta1, float beta2) {
    __shared__ float part[16];
    float acc = 0.f;
    for (int i = threadIdx.x; i < n; i += 1024) acc += v[i];
    acc = wave_sum(acc);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        float t = 0.f;
        for (int w = 0; w < 16; ++w) t += part[w];
        out[0] = t * scale;
    }
    if (threadIdx.x == 64) {
        const int t = ++step[0];
        hyper[2] = (float)(1.0 - pow((double)beta1, (double)t));
        hyper[3] = (float)sqrt(1.0 - pow((double)beta2, (double)t));
    }
}

// frac[b] = |nnd_b / den_b - 1|  (util.py:1126)
__global__ void val_frac_kernel(const float* __restrict__ partial, int slots_ld, int nslots, int B,
                                const float* __restrict__ den, float* __restrict__ frac) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    float c = 0.f;
    for (int s = 0; s < nslots; ++s) c += partial[(size_t)b * slots_ld + s];
    frac[b] = fabsf(c / den[b] - 1.f);
}

// The three validation metrics of an epoch (util.py:1124-1127: torch.median(loss), torch.max(frac), torch.median(frac)) on the
// device, so that the epoch's controller reads ONE small record instead of two row vectors: out[0] = *last (the epoch's last
// training loss, NaN if null), out[1] = lower median of loss[n], out[2] = max of frac[n], out[3] = lower median of frac[n].
// Selection by rank counting (thread i counts the elements before x_i in sorted order; n <= a few 10^4: n^2 compares spread over
// n threads); a NaN anywhere makes the statistic NaN, as torch.median / torch.max do.
__global__ __launch_bounds__(256) void val_metrics_kernel(const float* __restrict__ loss, const float* __restrict__ frac, int n,
                                                          const float* __restrict__ last, float* __restrict__ out) {
    __shared__ float tl[256], tf[256];
    const int i = blockIdx.x * 256 + threadIdx.x;
    const bool in = i < n;
    const float xl = in ? loss[i] : 0.f, xf = in ? frac[i] : 0.f;
    int rl = 0, rf = 0, nanl = 0, nanf = 0;
    for (int j0 = 0; j0 < n; j0 += 256) {
        const int j = j0 + threadIdx.x;
        tl[threadIdx.x] = j < n ? loss[j] : INFINITY;
        tf[threadIdx.x] = j < n ? frac[j] : INFINITY;
        __syncthreads();
        const int m = min(256, n - j0);
        for (int k = 0; k < m; ++k) {
            const float a = tl[k], b = tf[k];
            rl += (a < xl) | ((a == xl) & (j0 + k < i));
            rf += (b < xf) | ((b == xf) & (j0 + k < i));
            nanl |= a != a;
            nanf |= b != b;
        }
        __syncthreads();
    }
    if (!in) return;
    const int mid = (n - 1) / 2;
    if (i == 0) {
        out[0] = last ? last[0] : __builtin_nanf("");
        if (nanl) out[1] = __builtin_nanf("");
        if (nanf) { out[2] = __builtin_nanf(""); out[3] = __builtin_nanf(""); }
    }
    if (!nanl && rl == mid) out[1] = xl;
    if (!nanf && rf == n - 1) out[2] = xf;
    if (!nanf && rf == mid) out[3] = xf;
}

// ------------------------------------------------------------------ minibatch gather + X transform
__global__ void gather_xform_kernel(const float* __restrict__ X, int ldx, const int* __restrict__ ROWS, int B, int nin,
                                    const int* __restrict__ lg, const float* __restrict__ xmean,
                                    const float* __restrict__ xstd, float* __restrict__ XB, int ldxb) {
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (size_t)B * ldxb) return;
    const int i = (int)(idx / ldxb), j = (int)(idx % ldxb);
    if (j >= nin) { XB[idx] = 0.f; return; }
    const int r = ROWS ? ROWS[i] : i;
    float t = X[(size_t)r * ldx + j];
    if (lg && lg[j]) t = log10f(t);
    XB[idx] = (t - xmean[j]) / xstd[j];
}

// ------------------------------------------------------------------ bias gradient: db[n] = scale * sum_b dZ[b][n]
// One block per 64 columns, 16 waves: wave w sums rows w, w+16, ... with four independent
// accumulators (four row loads in flight per lane), then a fixed-order LDS reduction over the
// waves -- deterministic, and ~30 row loads deep instead of 125.
__global__ __launch_bounds__(1024) void colsum_kernel(const float* __restrict__ dZ, int ld, int B, int N, float scale,
                                                      float* __restrict__ db) {
    __shared__ float part[16][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int col = blockIdx.x * 64 + lane;
    float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
    if (col < N) {
        const float* p = dZ + col;
        int b = wave;
        for (; b + 48 < B; b += 64) {
            a0 += p[(size_t)b * ld]; a1 += p[(size_t)(b + 16) * ld];
            a2 += p[(size_t)(b + 32) * ld]; a3 += p[(size_t)(b + 48) * ld];
        }
        for (; b < B; b += 16) a0 += p[(size_t)b * ld];
    }
    part[wave][lane] = (a0 + a1) + (a2 + a3);
    __syncthreads();
    if (wave == 0 && col < N) {
        float t = 0.f;
#pragma unroll
        for (int w = 0; w < 16; ++w) t += part[w][lane];
        db[col] = scale * t;
    }
}

// ------------------------------------------------------------------ AdamW (torch.optim.AdamW single-tensor update)
// hyper = [lr, weight_decay, bc1 = 1-b1^t, sqrt(bc2) = sqrt(1-b2^t)]
__global__ void adamw_prepare_kernel(int* step, float* hyper, float beta1, float beta2) {
    const int t = ++step[0];
    hyper[2] = (float)(1.0 - pow((double)beta1, (double)t));
    hyper[3] = (float)sqrt(1.0 - pow((double)beta2, (double)t));
}

__global__ void adamw_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                             float* __restrict__ v, size_t n, const float* __restrict__ hyper, float beta1,
                             float beta2, float eps) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float lr = hyper[0], wd = hyper[1], bc1 = hyper[2], sbc2 = hyper[3];
    const float gi = g[i];
    float pi = p[i] * (1.f - lr * wd);
    float mi = m[i];
    mi = mi + (gi - mi) * (1.f - beta1);
    const float vi = v[i] * beta2 + (1.f - beta2) * gi * gi;
    const float denom = sqrtf(vi) / sbc2 + eps;
    pi = pi - (lr / bc1) * (mi / denom);
    p[i] = pi; m[i] = mi; v[i] = vi;
}

// Philox4x32-10 and the per-walker counter convention live in common.h (shared with net_stream.hip)

// ------------------------------------------------------------------ stretch move (emcee StretchMove / RedBlueMove)
__global__ void stretch_propose_kernel(const float* __restrict__ coords, int ldc, int ndim, const int* __restrict__ S,
                                       int ns, const float* __restrict__ ccoords, int ldcc, const int* __restrict__ C,
                                       int nc, uint64_t seed,
                                       const int* __restrict__ step_dev, int stream_id, float a,
                                       float* __restrict__ Q, int ldq, float* __restrict__ factors) {
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (size_t)ns * ldq) return;
    const int k = (int)(idx / ldq), d = (int)(idx % ldq);
    if (d >= ndim) { Q[idx] = 0.f; return; }
    const int wk = S[k];
    const U4 r = walker_bits(seed, (uint32_t)wk, (uint32_t)step_dev[0], (uint32_t)stream_id, 0u);
    const float t = (a - 1.f) * u01(r.x) + 1.f;
    const float zz = t * t / a;
    int j = (int)(((uint64_t)r.y * (uint64_t)nc) >> 32);
    const int wc = C[j];
    const float cr = ccoords[(size_t)wc * ldcc + d], s = coords[(size_t)wk * ldc + d];
    Q[idx] = cr - (cr - s) * zz;
    if (d == 0) factors[k] = ((float)ndim - 1.f) * logf(zz);
}

__global__ void stretch_accept_kernel(float* __restrict__ coords, int ldc, int ndim, float* __restrict__ logp,
                                      const int* __restrict__ S, int ns, const float* __restrict__ Q, int ldq,
                                      const float* __restrict__ lp_new, const float* __restrict__ factors,
                                      uint64_t seed, const int* __restrict__ step_dev, int stream_id,
                                      int* __restrict__ naccept) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= ns) return;
    const int wk = S[k];
    const U4 r = walker_bits(seed, (uint32_t)wk, (uint32_t)step_dev[0], (uint32_t)stream_id, 0u);
    const float lnpdiff = factors[k] + lp_new[k] - logp[wk];
    if (lnpdiff > logf(u01(r.z))) {
        for (int d = 0; d < ndim; ++d) coords[(size_t)wk * ldc + d] = Q[(size_t)k * ldq + d];
        logp[wk] = lp_new[k];
        if (naccept) atomicAdd(naccept + wk, 1);
    }
}

// ------------------------------------------------------------------ batched per-walker HMC (HMCSampler.py:26-59)
__device__ __forceinline__ float normal_draw(uint64_t seed, uint32_t w, uint32_t step, uint32_t stream, int d) {
    const U4 r = walker_bits(seed, w, step, stream, (uint32_t)(d >> 1) + 1u);
    const float u1 = (d & 1) ? u01(r.z) : u01(r.x), u2 = (d & 1) ? u01(r.w) : u01(r.y);
    return sqrtf(-2.f * logf(u1)) * cosf(6.28318530717958648f * u2);
}

// One WAVE per chain, lane = dimension (a thread per chain walked its row with a stride of a row: 20-29 us per launch at
// 4096 chains x 33, more than four of the leapfrog's own launches); the kinetic energy is summed in dimension order.
__device__ __forceinline__ float wave_ordered_sum(float t, int n) {
    float acc = 0.f;
    for (int j = 0; j < n; ++j) acc += __shfl(t, j, 64);
    return acc;
}

// sum_d P[b][d]^2 / mass[d] of chain b, by the chain's wave: the ONE place this sum is written, since its order (64
// dimensions at a time, each group in dimension order) is what makes every route through the Metropolis test bit-equal.
// hmc_start_kernel keeps a loop of its own: it forms t from the momentum it has just drawn.
__device__ __forceinline__ float wave_kinetic(const float* __restrict__ P, int ldp, const float* __restrict__ mass, int ndim,
                                              int b, int lane) {
    float ke = 0.f;
    for (int d0 = 0; d0 < ndim; d0 += 64) {
        const int d = d0 + lane;
        float t = 0.f;
        if (d < ndim) { const float p = P[(size_t)b * ldp + d]; t = p * p / mass[d]; }
        ke += wave_ordered_sum(t, min(64, ndim - d0));
    }
    return ke;
}

// P ~ N(0, m), H0 = P^2 / 2m - lnP; G != nullptr: also the first half kick and the first drift of the leapfrog,
// P += ek G, Q = X + ed P / m (hmc_kick_drift_kernel's arithmetic).  eps != nullptr: a step size per chain, ek and ed are
// its multipliers (1, 0.5 or 0); the Philox step is step_dev[0] + step_off.
__global__ void hmc_start_kernel(int B, int ndim, const float* __restrict__ mass, uint64_t seed,
                                 const int* __restrict__ step_dev, const float* __restrict__ lnp,
                                 const float* __restrict__ P0, int ldp0, const float* __restrict__ G, int ldg, float ek, float ed,
                                 const float* __restrict__ X, int ldx, float* __restrict__ P, int ldp, float* __restrict__ Q,
                                 int ldq, float* __restrict__ H0, const float* __restrict__ eps, int step_off) {
    const int b = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (b >= B) return;
    const bool kick = ek != 0.f, drift = ed != 0.f;
    if (eps) { const float e = eps[b]; ek *= e; ed *= e; }
    float ke = 0.f;
    for (int d0 = 0; d0 < ndim; d0 += 64) {
        const int d = d0 + lane;
        float t = 0.f;
        if (d < ndim) {
            const float m = mass[d];
            const float n01 = P0 ? P0[(size_t)b * ldp0 + d] : normal_draw(seed, (uint32_t)b, (uint32_t)(step_dev[0] + step_off), 1u, d);
            float p = n01 * sqrtf(m);
            t = p * p / m;
            if (G) {
                if (kick) p += ek * G[(size_t)b * ldg + d];
                const float x = X[(size_t)b * ldx + d];
                Q[(size_t)b * ldq + d] = drift ? x + ed * (p / m) : x;
            }
            P[(size_t)b * ldp + d] = p;
        }
        ke += wave_ordered_sum(t, min(64, ndim - d0));
    }
    if (lane == 0) H0[b] = 0.5f * ke - lnp[b];
}

// P += eps_kick * G ; Q += eps_drift * P / m   (either eps may be 0); eps != nullptr: eps_kick = ek eps[b], eps_drift = ed eps[b]
__global__ void hmc_kick_drift_kernel(int B, int ndim, const float* __restrict__ mass, float ek, float ed,
                                      const float* __restrict__ G, int ldg, float* __restrict__ P, int ldp,
                                      float* __restrict__ Q, int ldq, const float* __restrict__ eps) {
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (size_t)B * ndim) return;
    const int b = (int)(idx / ndim), d = (int)(idx % ndim);
    const bool kick = ek != 0.f, drift = ed != 0.f;
    if (eps) { const float e = eps[b]; ek *= e; ed *= e; }
    float p = P[(size_t)b * ldp + d];
    if (kick) { p += ek * G[(size_t)b * ldg + d]; P[(size_t)b * ldp + d] = p; }
    if (drift) Q[(size_t)b * ldq + d] += ed * (p / mass[d]);
}

// The Metropolis test of one transition at Philox step step_dev[0] + step_off (U != nullptr: the uniforms given), a wave
// per chain: accept where lnp_new is finite and u < exp(min(H0 - H1, 0)); X, G, lnp and naccept change on acceptance only.
// Behind it what a run of transitions enqueued in one go needs from the host otherwise, each part off when its pointer is
// null (linna_hmc_accept runs this kernel with all of them null and step_off 0):
//  * alpha[b] = exp(min(H0 - H1, 0)), 0 where lnp_new or an energy is not finite;
//  * chain / logps != nullptr: the chain's row and log-probability after the test, to chain[b][ndim] / logps[b];
//  * ad.m != nullptr: m += 1, and for ad.Madapt > 0 the dual averaging of the step size per chain (Hoffman & Gelman 2014,
//    algorithm 5, as the reference's NUTSMove runs it at sampler.py:229-240 with nalpha = 1): while m <= Madapt
//      Hbar = (1 - 1/(m + t0)) Hbar + (delta - alpha) / (m + t0);  eps = exp(mu - sqrt(m) / gamma Hbar);
//      epsbar = exp((1 - m^-kappa) log epsbar + m^-kappa log eps),
//    at m == Madapt + 1 eps = epsbar, later nothing.  This launch follows every leapfrog launch of its transition: eps[b]
//    has no reader left;
//  * en (HmcEnergy, every pointer nullable; estate and ndiv come together): the energy diagnostics of the transition, by
//    lane 0 behind the test.  E = acc ? H1 : H0 (the energy of the state the transition ends in, H1 the value the test
//    used) to en.energy[b]; the energy ERROR H1 - H0 (not the test's H0 - H1) to en.dH[b]; the transition is divergent
//    unless lnp_new is finite and H1 - H0 <= en.max_dH (a NaN error is; equality is not; a divergent transition never
//    accepts), ndiv[b] += 1 then -- a plain store, this wave owns the chain; and the chain's float64 accumulators
//    estate[b] = {n, mean, M2, D2, Eprev} (zeros = empty): for a finite E Welford's update of n, mean, M2, for n >= 1 before it
//    D2 += (E - Eprev)^2, then Eprev = E; a non-finite E changes nothing.  One writer, one order: the same input gives
//    the same bits.  hmc_energy_finish_kernel turns them into E-BFMI.
__global__ void hmc_accept_kernel(int B, int ndim, const float* __restrict__ mass, uint64_t seed,
                                  const int* __restrict__ step_dev, int step_off, const float* __restrict__ H0,
                                  const float* __restrict__ P, int ldp, const float* __restrict__ Qn, int ldq,
                                  const float* __restrict__ lnp_new, const float* __restrict__ Gn, int ldg,
                                  const float* __restrict__ U,
                                  float* __restrict__ X, int ldx, float* __restrict__ lnp, float* __restrict__ G,
                                  int* __restrict__ naccept, float* __restrict__ alpha, HmcAdapt ad,
                                  float* __restrict__ chain, float* __restrict__ logps, HmcEnergy en) {
    const int b = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6), lane = threadIdx.x & 63;   // a wave per chain
    if (b >= B) return;
    const float ke = wave_kinetic(P, ldp, mass, ndim, b, lane);
    const float ln = lnp_new[b];
    const float H1 = 0.5f * ke - ln;
    const U4 r = walker_bits(seed, (uint32_t)b, (uint32_t)(step_dev[0] + step_off), 2u, 0u);
    const float h0 = H0[b];
    const float dH = h0 - H1;
    const float ratio = expf(dH > 0.f ? 0.f : dH);   // a NaN energy stays NaN and rejects (np.minimum; fminf would return 0)
    const float u = U ? U[b] : u01(r.x);
    const bool acc = isfinite(ln) && u < ratio;
    for (int d = lane; d < ndim; d += 64) {
        float x = 0.f;
        if (acc) {
            x = Qn[(size_t)b * ldq + d];
            X[(size_t)b * ldx + d] = x;
            G[(size_t)b * ldg + d] = Gn[(size_t)b * ldg + d];
        } else if (chain) x = X[(size_t)b * ldx + d];
        if (chain) chain[(size_t)b * ndim + d] = x;
    }
    if (lane != 0) return;
    if (acc) {
        lnp[b] = ln;
        if (naccept) atomicAdd(naccept + b, 1);
    }
    if (logps) logps[b] = acc ? ln : lnp[b];
    const float al = isfinite(ln) && isfinite(dH) ? ratio : 0.f;
    if (alpha) alpha[b] = al;
    if (en.energy || en.dH || en.estate) {
        const float E = acc ? H1 : h0, err = H1 - h0;
        if (en.energy) en.energy[b] = E;
        if (en.dH) en.dH[b] = err;
        if (en.estate) {
            if (!(isfinite(ln) && err <= en.max_dH)) en.ndiv[b] += 1;
            if (isfinite(E)) {
                double* s = en.estate + (size_t)LINNA_HMC_ENERGY_DOUBLES * b;
                const double e = (double)E, n0 = s[0], n1 = n0 + 1.0, d = e - s[1], mean = s[1] + d / n1;
                s[2] += d * (e - mean);
                if (n0 >= 1.0) { const double t = e - s[4]; s[3] += t * t; }
                s[0] = n1; s[1] = mean; s[4] = e;
            }
        }
    }
    if (!ad.m) return;
    const int m = ad.m[b];
    ad.m[b] = m + 1;
    if (ad.Madapt <= 0) return;
    if (m <= ad.Madapt) {
        const float fm = (float)m, sm = sqrtf(fm);
        float eta = 1.f / (fm + 10.f);                                  // t0 = 10
        const float Hb = (1.f - eta) * ad.Hbar[b] + eta * (ad.delta - al);
        const float e = expf(ad.mu[b] - sm / 0.05f * Hb);               // gamma = 0.05
        eta = 1.f / (sm * sqrtf(sm));                                   // m^-kappa, kappa = 0.75
        ad.Hbar[b] = Hb;
        ad.eps[b] = e;
        ad.epsbar[b] = expf((1.f - eta) * logf(ad.epsbar[b]) + eta * logf(e));
    } else if (m == ad.Madapt + 1) {
        ad.eps[b] = ad.epsbar[b];
    }
}

// The finish of the energy diagnostics hmc_accept_kernel accumulates: bfmi[b] = D2 / M2 (Stan's E-BFMI,
// sum_{n>=1} (E_n - E_{n-1})^2 / sum_n (E_n - mean)^2, no N / (N - 1) factor), NaN for n < 2 or M2 == 0, and
// pooled = {the smallest E-BFMI over the chains, NaN ones ignored (NaN if all are), sum_b ndiv[b], the chains with ndiv[b] > 0}.
// ONE workgroup, a thread per chain striding over B; the three values of a thread meet by shuffles over the wave and by
// LDS over the waves, in wave order (a minimum has no order; the counts are integers in a double: exact).  Nothing atomic.
constexpr int ENERGY_WAVES = 4;
__device__ __forceinline__ double wave_min_f64(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmin(v, __shfl_xor(v, o, 64));      // (fmin returns the operand that is a number)
    return v;
}
__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__global__ __launch_bounds__(ENERGY_WAVES * 64) void hmc_energy_finish_kernel(int B, const double* __restrict__ estate,
                                                                              const int* __restrict__ ndiv, float* __restrict__ bfmi,
                                                                              double* __restrict__ pooled) {
    __shared__ double red[3][ENERGY_WAVES];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const double nan = __longlong_as_double(0x7ff8000000000000LL);
    double mn = nan, total = 0.0, chains = 0.0;
    for (int b = threadIdx.x; b < B; b += ENERGY_WAVES * 64) {
        const double* s = estate + (size_t)LINNA_HMC_ENERGY_DOUBLES * b;
        const double r = s[0] >= 2.0 && s[2] != 0.0 ? s[3] / s[2] : nan;
        bfmi[b] = (float)r;
        mn = fmin(mn, r);
        const int k = ndiv[b];
        total += (double)k;
        chains += k > 0 ? 1.0 : 0.0;
    }
    mn = wave_min_f64(mn); total = wave_sum_f64(total); chains = wave_sum_f64(chains);
    if (lane == 0) { red[0][wave] = mn; red[1][wave] = total; red[2][wave] = chains; }
    __syncthreads();
    if (threadIdx.x == 0) {
        mn = red[0][0]; total = red[1][0]; chains = red[2][0];
        for (int w = 1; w < ENERGY_WAVES; ++w) { mn = fmin(mn, red[0][w]); total += red[1][w]; chains += red[2][w]; }
        pooled[0] = mn; pooled[1] = total; pooled[2] = chains;
    }
}

// find_reasonable_epsilon of the reference (sampler.py:151-184), every chain at once and in a bounded number of rounds.
// A chain's state: 0 = still halving eps from 1 until the one-step leapfrog gives a finite lnP' and gradient; +1 / -1 = the
// direction a in which eps doubles / halves while a logaccept > -a log 2; 2 = finished (nothing of it changes any more).
// The set-up: eps = 1, state 0, and the ONE momentum draw r0 ~ N(0, 1) every trial of the chain uses (Philox stream 3).
__global__ void hmc_find_eps_init_kernel(int B, int ndim, uint64_t seed, const int* __restrict__ step_dev, int step_off,
                                         float* __restrict__ R0, int ldr, float* __restrict__ eps, int* __restrict__ state) {
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (size_t)B * ndim) return;
    const int b = (int)(idx / ndim), d = (int)(idx % ndim);
    R0[(size_t)b * ldr + d] = normal_draw(seed, (uint32_t)b, (uint32_t)(step_dev[0] + step_off), 3u, d);
    if (d == 0) { eps[b] = 1.f; state[b] = 0; }
}
// One round: the trial of every chain was hmc_start_kernel with P0 = r0, a half kick and a drift of eps[b], then the
// gradient at Q with the closing half kick -- H0, P, lnp_new, Gn are what they left.  logaccept = H0 - H1 (sampler.py:172).
// A comparison with a NaN is false, as in numpy: such a chain stops where it is.  nactive != nullptr (the last round):
// += the chains this round leaves unfinished.
__global__ void hmc_find_eps_kernel(int B, int ndim, const float* __restrict__ mass, const float* __restrict__ H0,
                                    const float* __restrict__ P, int ldp, const float* __restrict__ lnp_new,
                                    const float* __restrict__ Gn, int ldg, float* __restrict__ eps, int* __restrict__ state,
                                    int* __restrict__ nactive) {
    const int b = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6), lane = threadIdx.x & 63;   // a wave per chain
    if (b >= B) return;
    int st = state[b];
    if (st == 2) return;
    const float ke = wave_kinetic(P, ldp, mass, ndim, b, lane);
    int bad = 0;
    for (int d = lane; d < ndim; d += 64) bad |= !isfinite(Gn[(size_t)b * ldg + d]);
    const float ln = lnp_new[b];
    bad = __any(bad) || !isfinite(ln);
    if (lane != 0) return;
    const float la = H0[b] - (0.5f * ke - ln);
    const float LN2 = 0.693147180559945f;
    float e = eps[b];
    if (st == 0) {
        if (bad) e *= 0.5f;                                   // k *= 0.5 (:165)
        else {
            e *= 0.5f;                                        // epsilon = 0.5 k epsilon (:168)
            st = la > -LN2 ? 1 : -1;                          // (:173)
            if ((float)st * la > -(float)st * LN2) e = st > 0 ? e * 2.f : e * 0.5f;   // the loop's first pass rests on this trial (:176)
            else st = 2;
        }
    } else if ((float)st * la > -(float)st * LN2) e = st > 0 ? e * 2.f : e * 0.5f;
    else st = 2;
    eps[b] = e;
    state[b] = st;
    if (nactive && st != 2) atomicAdd(nactive, 1);
}

// Running moments of the chain positions pooled over chains, mom = {n, mean[ndim], M2[ndim]} in float64 (linna_hip.h): what
// the windowed mass adaptation accumulates behind every transition.  ONE workgroup of 16 waves: every merge reads n and one
// thread writes it, which workgroups of their own could not order.  Lane = parameter (a row is one coalesced read), 64
// parameters at a time; the waves stride over the chains 16 rows at a time.  The 16 loads of a round are unconditional -- row
// and column indices clamped into the matrix, the value masked afterwards -- so that all of them are in flight before the
// first add: behind a bounds test each load waited for the one before it, a cache miss of latency per row (126 us per launch
// at 4096 chains).  Two passes over X, the batch mean and then the batch M2 about it; the per-wave partials meet in LDS and
// are added in wave order by every thread alike.  The order of every sum is fixed by (B, ndim) alone: no atomics, the same bits each time.
constexpr int MOM_WAVES = 16, MOM_ROWS = 16;

__device__ __forceinline__ double mom_block_sum(double (*part)[64], double s, int wave, int lane) {
    __syncthreads();                                          // (the totals of the pass before have been read)
    part[wave][lane] = s;
    __syncthreads();
    double t = 0.0;
    for (int w = 0; w < MOM_WAVES; ++w) t += part[w][lane];
    return t;
}
// rows b0 .. b0 + MOM_ROWS - 1 of column dc (< ndim); a row past the end re-reads the last one
__device__ __forceinline__ void mom_load(float (&v)[MOM_ROWS], const float* __restrict__ X, int ldx, int B, int b0, int dc) {
#pragma unroll
    for (int u = 0; u < MOM_ROWS; ++u) v[u] = X[(size_t)min(b0 + u, B - 1) * ldx + dc];
}

__global__ __launch_bounds__(MOM_WAVES * 64) void hmc_moments_kernel(int B, int ndim, const float* __restrict__ X, int ldx,
                                                                     double* __restrict__ mom) {
    __shared__ double part[MOM_WAVES][64];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const double n = mom[0], nb = (double)B, n1 = n + nb;
    for (int d0 = 0; d0 < ndim; d0 += 64) {
        const int d = d0 + lane, dc = min(d, ndim - 1);       // (the pad of a row is never read)
        const bool on = d < ndim;
        float v[MOM_ROWS];
        double s = 0.0;
        for (int b0 = wave * MOM_ROWS; b0 < B; b0 += MOM_WAVES * MOM_ROWS) {
            mom_load(v, X, ldx, B, b0, dc);
#pragma unroll
            for (int u = 0; u < MOM_ROWS; ++u) s += on && b0 + u < B ? (double)v[u] : 0.0;
        }
        const double mb = mom_block_sum(part, s, wave, lane) / nb;
        s = 0.0;
        for (int b0 = wave * MOM_ROWS; b0 < B; b0 += MOM_WAVES * MOM_ROWS) {
            mom_load(v, X, ldx, B, b0, dc);
#pragma unroll
            for (int u = 0; u < MOM_ROWS; ++u) {
                const double t = on && b0 + u < B ? (double)v[u] - mb : 0.0;
                s += t * t;
            }
        }
        const double M2b = mom_block_sum(part, s, wave, lane);
        if (wave == 0 && on) {                                // Chan, Golub & LeVeque's merge of (nb, mb, M2b) into (n, mean, M2)
            const double mean = mom[1 + d], delta = mb - mean;
            mom[1 + d] = mean + delta * nb / n1;
            mom[1 + ndim + d] += M2b + delta * delta * n * nb / n1;
        }
    }
    if (threadIdx.x == 0) mom[0] = n1;                        // (behind the barriers above: every thread has read n)
}

// mass = 1 / variance of the moments, with Stan's shrinkage towards 1e-3 (var n / (n + 5) + 1e-3 * 5 / (n + 5)); a parameter
// whose result is not finite and positive keeps its mass, and so does every parameter while n < 2.  One workgroup: the zeroing
// of mom (reset) follows a barrier behind every read of it.
__global__ void hmc_mass_from_moments_kernel(int ndim, double* __restrict__ mom, float* __restrict__ mass, int reset) {
    const double n = mom[0];
    if (n >= 2.0) {
        for (int d = threadIdx.x; d < ndim; d += blockDim.x) {
            const double var = mom[1 + ndim + d] / (n - 1.0);
            const double shrunk = var * n / (n + 5.0) + 1e-3 * 5.0 / (n + 5.0);
            const float m = (float)(1.0 / shrunk);
            if (isfinite(m) && m > 0.f) mass[d] = m;
        }
    }
    __syncthreads();
    if (reset) for (int i = threadIdx.x; i < 1 + 2 * ndim; i += blockDim.x) mom[i] = 0.0;
}

// ------------------------------------------------------------------ a dense mass: co-moments, their Cholesky factor, the whitened leapfrog
// Shifted raw sums of the chain positions, mom = {n, c[nd], SLOTS x {S1[nd], S2[nd][nd] (j <= i)}} in float64 (linna_hip.h),
// t = (double)X - c.  Every output word depends on its own old value, X and c alone, so the grid is (tile of the lower
// triangle, slot): a tile is 8 x 8 pairs (lane = pair), a slot a fixed share of the rows, ceil(B / SLOTS) of them in row
// order.  The four waves of a workgroup stride over the slot's rows 16 at a time; the loads of a round are unconditional
// (indices clamped, values masked: hmc_moments_kernel's lesson); the per-wave partials meet in LDS and are added in wave
// order.  n is written by one thread of the launch and read by none.  No atomics: the same input gives the same bits.
constexpr int COMOM_SLOTS = LINNA_HMC_COMOMENT_SLOTS, COMOM_T = 8, COMOM_WAVES = 4, COMOM_ROWS = 16;
static_assert(COMOM_T * COMOM_T == 64, "a lane per pair of a tile");

__global__ __launch_bounds__(COMOM_WAVES * 64) void hmc_comoments_kernel(int B, int ndim, const float* __restrict__ X, int ldx,
                                                                         double* __restrict__ mom) {
    __shared__ double part[2][COMOM_WAVES][64];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    // tile blockIdx.x of the lower triangle, rows of tiles in order: (ti, tj), tj <= ti
    int ti = 0;
    while ((ti + 1) * (ti + 2) / 2 <= (int)blockIdx.x) ++ti;
    const int tj = (int)blockIdx.x - ti * (ti + 1) / 2;
    const int i = ti * COMOM_T + (lane >> 3), j = tj * COMOM_T + (lane & 7);
    const int ic = min(i, ndim - 1), jc = min(j, ndim - 1);   // (the pad of a row is never read)
    const bool on = i < ndim && j <= i;
    const int per = (B + COMOM_SLOTS - 1) / COMOM_SLOTS, slot = blockIdx.y;
    const int lo = min(slot * per, B), hi = min(lo + per, B);
    const double ci = mom[1 + ic], cj = mom[1 + jc];
    double s1 = 0.0, s2 = 0.0;
    for (int b0 = lo + wave * COMOM_ROWS; b0 < hi; b0 += COMOM_WAVES * COMOM_ROWS) {
        float vi[COMOM_ROWS], vj[COMOM_ROWS];
#pragma unroll
        for (int u = 0; u < COMOM_ROWS; ++u) {
            const size_t row = (size_t)min(b0 + u, B - 1) * ldx;
            vi[u] = X[row + ic];
            vj[u] = X[row + jc];
        }
#pragma unroll
        for (int u = 0; u < COMOM_ROWS; ++u) {
            const bool in = b0 + u < hi;
            const double a = in ? (double)vi[u] - ci : 0.0, b = in ? (double)vj[u] - cj : 0.0;
            s1 += a;
            s2 += a * b;
        }
    }
    part[0][wave][lane] = s1;
    part[1][wave][lane] = s2;
    __syncthreads();
    if (wave == 0 && on) {
        double t1 = 0.0, t2 = 0.0;
        for (int w = 0; w < COMOM_WAVES; ++w) { t1 += part[0][w][lane]; t2 += part[1][w][lane]; }
        double* S = mom + 1 + ndim + (size_t)slot * ((size_t)ndim + (size_t)ndim * ndim);
        if (i == j) S[i] += t1;
        S[ndim + (size_t)i * ndim + j] += t2;
    }
    if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) mom[0] += (double)B;
}

// One workgroup: the slots summed in slot order, cov = (S2 - S1 S1^T / n) / (n - 1), Stan's shrinkage for a dense metric
// (cov n / (n + 5) + 1e-3 * 5 / (n + 5) I) and its Cholesky factor in float64 -- the packed lower triangle in LDS, 66 KB at
// ndim = 128.  Right-looking with ONE barrier per column: step k subtracts L[i][k] L[j][k] / pivot_k from the trailing
// triangle and leaves column k unscaled (C[i][k] = L[i][k] / sqrt(pivot_k) at the end), so that a step reads only what the
// step before wrote.  info[0] = 0: C as float32 into Cm[nd][ldc] and C^T behind it, zeros outside the triangles and in the
// pad; a pivot k that is not finite and positive: info[0] = k + 1, Cm untouched; n < 2 (or NaN): info[0] = -1, Cm untouched.
// reset: behind a barrier after the last read of mom, c <- the mean (kept where n < 1), n and the slots <- 0.
constexpr int CHOL_MAX = LINNA_HMC_DENSE_MAX_NDIM, CHOL_THREADS = 1024;
__device__ __forceinline__ int tri(int i, int j) { return i * (i + 1) / 2 + j; }

__global__ __launch_bounds__(CHOL_THREADS) void hmc_chol_from_comoments_kernel(int ndim, double* __restrict__ mom, float* __restrict__ Cm,
                                                                               int ldc, int* __restrict__ info, int reset) {
    __shared__ double L[CHOL_MAX * (CHOL_MAX + 1) / 2];
    __shared__ double s1[CHOL_MAX];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, nwaves = CHOL_THREADS / 64;
    const size_t slotw = (size_t)ndim + (size_t)ndim * ndim;
    const double* slots = mom + 1 + ndim;
    const double n = mom[0];
    const bool have = n >= 2.0;                               // (false for a NaN)
    for (int d = tid; d < ndim; d += CHOL_THREADS) {
        double t = 0.0;
        for (int s = 0; s < COMOM_SLOTS; ++s) t += slots[s * slotw + d];
        s1[d] = t;
    }
    __syncthreads();
    int fail = have ? 0 : -1;
    if (have) {
        const double shr = n / (n + 5.0), add = 1e-3 * 5.0 / (n + 5.0);
        for (int i = wave; i < ndim; i += nwaves)
            for (int j = lane; j <= i; j += 64) {
                double t = 0.0;
                for (int s = 0; s < COMOM_SLOTS; ++s) t += slots[s * slotw + ndim + (size_t)i * ndim + j];
                const double cov = (t - s1[i] * s1[j] / n) / (n - 1.0);
                L[tri(i, j)] = cov * shr + (i == j ? add : 0.0);
            }
        for (int k = 0; k < ndim; ++k) {
            __syncthreads();
            const double piv = L[tri(k, k)];                  // (every thread reads the same word: the branch is uniform)
            if (!(piv > 0.0 && isfinite(piv))) { fail = k + 1; break; }
            const double inv = 1.0 / piv;
            for (int i = k + 1 + wave; i < ndim; i += nwaves) {
                const double lik = L[tri(i, k)] * inv;
                for (int j = k + 1 + lane; j <= i; j += 64) L[tri(i, j)] -= lik * L[tri(j, k)];
            }
        }
        __syncthreads();
        if (!fail) {
            for (int i = wave; i < ndim; i += nwaves)
                for (int j = lane; j < ldc; j += 64) {
                    const float c = j <= i ? (float)(L[tri(i, j)] / sqrt(L[tri(j, j)])) : 0.f;
                    Cm[(size_t)i * ldc + j] = c;
                    if (j < ndim) Cm[((size_t)ndim + j) * ldc + i] = c;
                    else Cm[((size_t)ndim + i) * ldc + j] = 0.f;
                }
        }
    }
    if (tid == 0) info[0] = fail;
    if (!reset) return;
    __syncthreads();                                          // (every read of mom is behind us)
    if (n >= 1.0) for (int d = tid; d < ndim; d += CHOL_THREADS) mom[1 + d] += s1[d] / n;
    for (size_t e = tid; e < COMOM_SLOTS * slotw; e += CHOL_THREADS) mom[1 + ndim + e] = 0.0;
    if (tid == 0) mom[0] = 0.0;
}

// The leapfrog's kick and drift under the dense mass M = (C C^T)^-1 in the whitened momentum w = C^T p:
//   W[b] += (ek e) C^T G[b];   Q[b] = (X ? X[b] : Q[b]) + (ed e) C W[b],   e = EPS ? EPS[b] : 1
// (either multiplier may be 0: that half is off; without a drift Q = X where X is given and is left alone otherwise).
// A wave per chain, lane = dimension, a lane holds dimensions lane and lane + 64 (ndim <= 128).  Both matrix-vector
// products read rows -- (C^T g)_d = sum_{j >= d} Ct[d][j] g_j from the transposed copy behind C, (C w)_d = sum_{j <= d}
// C[d][j] w_j -- over the triangle only, j ascending, a float32 product and then a float32 add.  Pad columns are not written.
__device__ __forceinline__ float wave_pick(float v0, float v1, int j) { return j < 64 ? __shfl(v0, j, 64) : __shfl(v1, j - 64, 64); }
// a0 / a1 = the triangle product of rows r0 / r1 (dimensions d0 / d1 of this lane) with the wave's vector {v0, v1}: j <= d
// (LOWER) or j >= d.  Eight columns a round, their loads unconditional (the column index clamped into the row, the product
// masked) so that all of them are in flight before the first add: one load a column waited out a cache access each.
template <bool LOWER>
__device__ __forceinline__ void wave_tri_dot(const float* __restrict__ r0, const float* __restrict__ r1, float v0, float v1, int d0,
                                             int d1, bool on0, bool on1, int ndim, float& a0, float& a1) {
    constexpr int U = 8;
    a0 = 0.f; a1 = 0.f;
    for (int j0 = 0; j0 < ndim; j0 += U) {
        float c0[U], c1[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int jc = min(j0 + u, ndim - 1);
            c0[u] = r0[jc];
            c1[u] = ndim > 64 ? r1[jc] : 0.f;
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int j = j0 + u;
            const float vj = wave_pick(v0, v1, min(j, ndim - 1));
            if (j < ndim && on0 && (LOWER ? j <= d0 : j >= d0)) a0 += c0[u] * vj;
            if (j < ndim && on1 && (LOWER ? j <= d1 : j >= d1)) a1 += c1[u] * vj;
        }
    }
}

__global__ void hmc_kick_drift_dense_kernel(int B, int ndim, const float* __restrict__ Cm, int ldc, const float* __restrict__ eps,
                                            float ek, float ed, const float* __restrict__ G, int ldg, float* __restrict__ W, int ldw,
                                            const float* __restrict__ X, int ldx, float* __restrict__ Q, int ldq) {
    const int b = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (b >= B) return;
    const bool kick = ek != 0.f, drift = ed != 0.f;
    if (eps) { const float e = eps[b]; ek *= e; ed *= e; }
    const int d0 = lane, d1 = lane + 64;
    const bool on0 = d0 < ndim, on1 = d1 < ndim;
    float w0 = on0 ? W[(size_t)b * ldw + d0] : 0.f, w1 = on1 ? W[(size_t)b * ldw + d1] : 0.f;
    if (kick) {
        const float* Ct = Cm + (size_t)ndim * ldc;
        const float g0 = on0 ? G[(size_t)b * ldg + d0] : 0.f, g1 = on1 ? G[(size_t)b * ldg + d1] : 0.f;
        const float* r0 = Ct + (size_t)min(d0, ndim - 1) * ldc;
        const float* r1 = Ct + (size_t)min(d1, ndim - 1) * ldc;
        float a0, a1;
        wave_tri_dot<false>(r0, r1, g0, g1, d0, d1, on0, on1, ndim, a0, a1);
        w0 += ek * a0;
        w1 += ek * a1;
        if (on0) W[(size_t)b * ldw + d0] = w0;
        if (on1) W[(size_t)b * ldw + d1] = w1;
    }
    if (!drift && !X) return;
    float q0 = 0.f, q1 = 0.f;
    if (on0) q0 = X ? X[(size_t)b * ldx + d0] : Q[(size_t)b * ldq + d0];
    if (on1) q1 = X ? X[(size_t)b * ldx + d1] : Q[(size_t)b * ldq + d1];
    if (drift) {
        const float* r0 = Cm + (size_t)min(d0, ndim - 1) * ldc;
        const float* r1 = Cm + (size_t)min(d1, ndim - 1) * ldc;
        float a0, a1;
        wave_tri_dot<true>(r0, r1, w0, w1, d0, d1, on0, on1, ndim, a0, a1);
        q0 += ed * a0;
        q1 += ed * a1;
    }
    if (on0) Q[(size_t)b * ldq + d0] = q0;
    if (on1) Q[(size_t)b * ldq + d1] = q1;
}

// ------------------------------------------------------------------ the trajectory length adapted on the device (ChEES-HMC)
// Hoffman, Radul & Sountsov 2021: all chains share one step size eps and one jittered trajectory length T; log T climbs the
// gradient of the "change in the estimator of the expected square" criterion, which is a sum over the chains.  Two launches
// around a warm-up transition, state = {12 words, m0[ndim], m1[ndim]} in float64 (linna_hip.h):
//   begin: m0 = the mean position of all chains, r0[b] = |x_b - m0|^2;
//   end:   m1 = the mean proposal of the valid chains, c_b = h_t (|q'_b - m1|^2 - r0[b]) (q'_b - m1) . v'_b, g = sum alpha c / sum alpha,
//          Adam on log T, dual averaging of log eps on the harmonic mean of alpha, eps[b] for the next transition.
// ONE workgroup of 16 waves each (the cross-chain sums need every chain and the state one writer), a wave per chain, lane =
// parameter, 64 parameters at a time.  The waves stride over the chains 8 rows at a time with the loads of a round
// unconditional -- indices clamped into the matrix, values masked or selected afterwards (hmc_moments_kernel's lesson).  A
// chain's dot products are summed over the wave in float64 (wave_sum8_f64, a butterfly in the dense instantiation), the per-wave partials meet in LDS and are added in wave
// order: every sum's order is fixed by (B, ndim), no atomics, the same input gives the same bits.
constexpr int CHEES_U = 8, CHEES_V = 4, CHEES_HEAD = LINNA_HMC_CHEES_HEAD;    // rows a round: CHEES_V where a row keeps two float64 sums
enum { CH_T = 0, CH_LOGT, CH_LOGTBAR, CH_A, CH_V, CH_MU, CH_HBAR, CH_LOGEPS, CH_LOGEPSBAR, CH_G, CH_HM, CH_NVALID };
static_assert(CH_NVALID + 1 == CHEES_HEAD, "the layout of linna_hip.h");
static_assert(CHEES_U == 8 && 2 * CHEES_V == 8, "wave_sum8_f64 takes eight sums");

// Eight sums over the wave at once: three halving steps (lanes 32, 16, 8 apart) in each of which a lane hands half of its values
// to its partner and adds the partner's share of the half it keeps, then a butterfly of the one value left over lanes 4, 2
// and 1 apart -- 10 exchanges of a double where eight butterflies take 48 (hmc_chees_begin_kernel at 4096 chains x 33: 157 ->
// 122 us; the end kernel did not move, it waits for its loads).  The sum of value j ends in the lanes with lane >> 3 == j and
// is read from lane 8 j; the order is fixed.
__device__ __forceinline__ double lane_f64(double v, int src) {
    const int lo = __builtin_amdgcn_readlane(__double2loint(v), src), hi = __builtin_amdgcn_readlane(__double2hiint(v), src);
    return __hiloint2double(hi, lo);
}
__device__ __forceinline__ void wave_sum8_f64(double (&v)[8], int lane) {
#pragma unroll
    for (int n = 4, o = 32; n >= 1; n >>= 1, o >>= 1) {
        const bool up = lane & o;
#pragma unroll
        for (int i = 0; i < n; ++i) {
            const double send = up ? v[i] : v[i + n], keep = up ? v[i + n] : v[i];
            v[i] = keep + __shfl_xor(send, o, 64);
        }
    }
    double t = v[0];
#pragma unroll
    for (int o = 4; o > 0; o >>= 1) t += __shfl_xor(t, o, 64);
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = lane_f64(t, 8 * j);
}
// rows b0 .. b0 + U - 1 of column dc (< ndim); a row past the end re-reads the last one
template <int U>
__device__ __forceinline__ void chees_load(float (&v)[U], const float* __restrict__ X, int ldx, int B, int b0, int dc) {
#pragma unroll
    for (int u = 0; u < U; ++u) v[u] = X[(size_t)min(b0 + u, B - 1) * ldx + dc];
}
// the base-2 van der Corput number of t: 1/2, 1/4, 3/4, 1/8, ...
__device__ __forceinline__ double chees_halton(long long t) {
    double h = 0.0, f = 0.5;
    for (; t > 0; t >>= 1, f *= 0.5) if (t & 1) h += f;
    return h;
}

__global__ __launch_bounds__(MOM_WAVES * 64) void hmc_chees_begin_kernel(int B, int ndim, const float* __restrict__ X, int ldx,
                                                                         double* state, double* __restrict__ r0) {
    __shared__ double part[MOM_WAVES][64];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    double* m0 = state + CHEES_HEAD;
    for (int d0 = 0; d0 < ndim; d0 += 64) {                   // the means: lane = parameter, as hmc_moments_kernel's first pass
        const int d = d0 + lane, dc = min(d, ndim - 1);
        float v[MOM_ROWS];
        double s = 0.0;
        for (int b0 = wave * MOM_ROWS; b0 < B; b0 += MOM_WAVES * MOM_ROWS) {
            mom_load(v, X, ldx, B, b0, dc);
#pragma unroll
            for (int u = 0; u < MOM_ROWS; ++u) s += b0 + u < B ? (double)v[u] : 0.0;
        }
        const double t = mom_block_sum(part, s, wave, lane);
        if (wave == 0 && d < ndim) m0[d] = t / (double)B;
    }
    __syncthreads();                                          // (m0 is read back by every wave)
    for (int b0 = wave * CHEES_U; b0 < B; b0 += MOM_WAVES * CHEES_U) {
        double a[CHEES_U];
#pragma unroll
        for (int u = 0; u < CHEES_U; ++u) a[u] = 0.0;
        for (int d0 = 0; d0 < ndim; d0 += 64) {
            const int dc = min(d0 + lane, ndim - 1);
            const bool on = d0 + lane < ndim;
            const double m = m0[dc];
            float v[CHEES_U];
            chees_load(v, X, ldx, B, b0, dc);
#pragma unroll
            for (int u = 0; u < CHEES_U; ++u) {
                const double t = on ? (double)v[u] - m : 0.0;
                a[u] += t * t;
            }
        }
        wave_sum8_f64(a, lane);
#pragma unroll
        for (int u = 0; u < CHEES_U; ++u)
            if (lane == 0 && b0 + u < B) r0[b0 + u] = a[u];
    }
}

// what the waves of hmc_chees_end_kernel hand to its one finishing thread
__device__ __forceinline__ void chees_wave_out(double (*red)[MOM_WAVES], int k, double s, int wave, int lane) {
    if (lane == 0) red[k][wave] = s;
}
__device__ __forceinline__ double chees_red_sum(const double (*red)[MOM_WAVES], int k) {
    double t = 0.0;
    for (int w = 0; w < MOM_WAVES; ++w) t += red[k][w];
    return t;
}

// A chain is valid when alpha[b] > 0 and r0[b] and every q'[b][d], p'[b][d] are finite; an invalid chain is selected out of
// every sum (0 x NaN is NaN) and counts as alpha = 0 in the harmonic mean.  Cm != nullptr: P holds the whitened momentum w'
// and the velocity is C w' (hmc_kick_drift_dense_kernel's drift product, ndim <= 128: a lane holds dimensions lane and
// lane + 64; an instantiation of its own, DENSE), else p' / mass.  The velocity is the float32 one the leapfrog moved the chain with.  On the launch with
// t == M the averaged step size and length are put in place (the freeze).
template <bool DENSE>
__global__ __launch_bounds__(MOM_WAVES * 64) void hmc_chees_end_kernel(int B, int ndim, const float* __restrict__ mass,
                                                                       const float* __restrict__ Cm, int ldc,
                                                                       const float* __restrict__ Q, int ldq,
                                                                       const float* __restrict__ P, int ldp,
                                                                       const float* __restrict__ alpha, const double* __restrict__ r0,
                                                                       double* state, float* __restrict__ eps, int M, double delta,
                                                                       int max_steps) {
    __shared__ double part[MOM_WAVES][64];
    __shared__ double red[4][MOM_WAVES];
    __shared__ float eps_out;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    double* m1 = state + CHEES_HEAD + ndim;
    double nvalid = 0.0;
    for (int d0 = 0; d0 < ndim; d0 += 64) {                   // m1: the column sums of q' over the valid chains
        const int d = d0 + lane, dc = min(d, ndim - 1);
        double s = 0.0, nv = 0.0;
        for (int b0 = wave * CHEES_U; b0 < B; b0 += MOM_WAVES * CHEES_U) {
            float qv[CHEES_U], pv[CHEES_U], al[CHEES_U];
            double rr[CHEES_U];
            chees_load(qv, Q, ldq, B, b0, dc);
            chees_load(pv, P, ldp, B, b0, dc);
#pragma unroll
            for (int u = 0; u < CHEES_U; ++u) { const int bc = min(b0 + u, B - 1); al[u] = alpha[bc]; rr[u] = r0[bc]; }
            unsigned elsewhere = 0u;                                  // bit u: row u is not finite in another group of 64 (ndim > 64 only)
            for (int e0 = 0; e0 < ndim; e0 += 64) {
                if (e0 == d0) continue;
                const int ec = min(e0 + lane, ndim - 1);
                for (int u = 0; u < CHEES_U; ++u) {
                    const size_t bc = (size_t)min(b0 + u, B - 1);
                    if (!(isfinite(Q[bc * ldq + ec]) && isfinite(P[bc * ldp + ec]))) elsewhere |= 1u << u;
                }
            }
#pragma unroll
            for (int u = 0; u < CHEES_U; ++u) {
                // (a clamped column is an element of the row too)
                const int bad = !(isfinite(qv[u]) && isfinite(pv[u])) || ((elsewhere >> u) & 1u);
                const bool ok = b0 + u < B && al[u] > 0.f && isfinite(rr[u]) && !__any(bad);
                s += ok && d < ndim ? (double)qv[u] : 0.0;
                nv += ok ? 1.0 : 0.0;
            }
        }
        if (d0 == 0) chees_wave_out(red, 0, nv, wave, lane);
        const double t = mom_block_sum(part, s, wave, lane);
        if (d0 == 0) nvalid = chees_red_sum(red, 0);
        if (wave == 0 && d < ndim) m1[d] = nvalid > 0.0 ? t / nvalid : 0.0;
    }
    __syncthreads();                                          // (m1 is read back by every wave)
    double Sac = 0.0, Sa = 0.0, Sh = 0.0;                     // sum alpha c / h_t, sum alpha, sum 1 / max(alpha, floor): wave-uniform
    if constexpr (DENSE) {
        const int d0 = lane, d1 = lane + 64;
        const bool on0 = d0 < ndim, on1 = d1 < ndim;
        const float* c0 = Cm + (size_t)min(d0, ndim - 1) * ldc;
        const float* c1 = Cm + (size_t)min(d1, ndim - 1) * ldc;
        const double ma = on0 ? m1[d0] : 0.0, mb = on1 ? m1[d1] : 0.0;
        for (int b = wave; b < B; b += MOM_WAVES) {
            const float q0 = on0 ? Q[(size_t)b * ldq + d0] : 0.f, q1 = on1 ? Q[(size_t)b * ldq + d1] : 0.f;
            const float w0 = on0 ? P[(size_t)b * ldp + d0] : 0.f, w1 = on1 ? P[(size_t)b * ldp + d1] : 0.f;
            const float al = alpha[b];
            const double rr = r0[b];
            const int bad = !(isfinite(q0) && isfinite(q1) && isfinite(w0) && isfinite(w1));
            float v0, v1;
            wave_tri_dot<true>(c0, c1, w0, w1, d0, d1, on0, on1, ndim, v0, v1);
            const double e0 = on0 ? (double)q0 - ma : 0.0, e1 = on1 ? (double)q1 - mb : 0.0;
            const double a = wave_sum_f64(e0 * e0 + e1 * e1);
            const double bq = wave_sum_f64((on0 ? e0 * (double)v0 : 0.0) + (on1 ? e1 * (double)v1 : 0.0));
            const bool ok = al > 0.f && isfinite(rr) && !__any(bad);
            const double aa = ok ? (double)al : 0.0;
            if (ok) { Sac += aa * ((a - rr) * bq); Sa += aa; }
            Sh += 1.0 / fmax(aa, LINNA_HMC_CHEES_ALPHA_FLOOR);
        }
    } else {
        for (int b0 = wave * CHEES_V; b0 < B; b0 += MOM_WAVES * CHEES_V) {
            double AB[2 * CHEES_V];                           // per row: sum (q' - m1)^2, then sum (q' - m1) v'
            int bad[CHEES_V];
#pragma unroll
            for (int u = 0; u < CHEES_V; ++u) { AB[u] = 0.0; AB[CHEES_V + u] = 0.0; bad[u] = 0; }
            for (int d0 = 0; d0 < ndim; d0 += 64) {
                const int dc = min(d0 + lane, ndim - 1);
                const bool on = d0 + lane < ndim;
                const double m = m1[dc];
                const float ms = mass[dc];
                float qv[CHEES_V], pv[CHEES_V];
                chees_load<CHEES_V>(qv, Q, ldq, B, b0, dc);
                chees_load<CHEES_V>(pv, P, ldp, B, b0, dc);
#pragma unroll
                for (int u = 0; u < CHEES_V; ++u) {
                    bad[u] |= !(isfinite(qv[u]) && isfinite(pv[u]));
                    const double e = on ? (double)qv[u] - m : 0.0;
                    AB[u] += e * e;
                    AB[CHEES_V + u] += on ? e * (double)(pv[u] / ms) : 0.0;
                }
            }
            wave_sum8_f64(AB, lane);
#pragma unroll
            for (int u = 0; u < CHEES_V; ++u) {
                const int bc = min(b0 + u, B - 1);
                const float al = alpha[bc];
                const double rr = r0[bc];
                const double a = AB[u], bq = AB[CHEES_V + u];
                const bool in = b0 + u < B, ok = in && al > 0.f && isfinite(rr) && !__any(bad[u]);
                const double aa = ok ? (double)al : 0.0;
                if (ok) { Sac += aa * ((a - rr) * bq); Sa += aa; }
                if (in) Sh += 1.0 / fmax(aa, LINNA_HMC_CHEES_ALPHA_FLOOR);
            }
        }
    }
    chees_wave_out(red, 1, Sac, wave, lane);
    chees_wave_out(red, 2, Sa, wave, lane);
    chees_wave_out(red, 3, Sh, wave, lane);
    __syncthreads();
    if (threadIdx.x == 0) {                                   // the state: one thread, float64
        const double t = state[CH_T];
        double logT = state[CH_LOGT], logTbar = state[CH_LOGTBAR], logepsbar = state[CH_LOGEPSBAR];
        if (nvalid > 0.0) {                                   // Adam ascent on log T with the gradient g T
            const double g = chees_halton((long long)t) * chees_red_sum(red, 1) / chees_red_sum(red, 2), G = g * exp(logT);
            const double b1 = LINNA_HMC_CHEES_BETA1, b2 = LINNA_HMC_CHEES_BETA2;
            const double a = b1 * state[CH_A] + (1.0 - b1) * G, v = b2 * state[CH_V] + (1.0 - b2) * G * G;
            const double ahat = a / (1.0 - exp(t * log(b1))), vhat = v / (1.0 - exp(t * log(b2)));
            logT += LINNA_HMC_CHEES_LR * ahat / (sqrt(vhat) + LINNA_HMC_CHEES_ADAM_EPS);
            state[CH_A] = a;
            state[CH_V] = v;
            state[CH_G] = g;
        }
        // dual averaging of the shared step size on the harmonic mean of alpha (t0 = 10, gamma = 0.05, kappa = 0.75)
        const double hm = (double)B / chees_red_sum(red, 3), eta = 1.0 / (t + 10.0);
        const double Hbar = (1.0 - eta) * state[CH_HBAR] + eta * (delta - hm);
        const double logeps = state[CH_MU] - sqrt(t) / 0.05 * Hbar, w = exp(-0.75 * log(t));
        logepsbar = (1.0 - w) * logepsbar + w * logeps;
        if (nvalid > 0.0) logTbar = (1.0 - w) * logTbar + w * logT;
        logT = fmin(fmax(logT, logeps), logeps + log((double)max_steps));
        const bool freeze = (long long)t == (long long)M;
        if (freeze) logT = logTbar;
        state[CH_T] = t + 1.0;
        state[CH_LOGT] = logT;
        state[CH_LOGTBAR] = logTbar;
        state[CH_HBAR] = Hbar;
        state[CH_LOGEPS] = logeps;
        state[CH_LOGEPSBAR] = logepsbar;
        state[CH_HM] = hm;
        state[CH_NVALID] = nvalid;
        eps_out = (float)exp(freeze ? logepsbar : logeps);
    }
    __syncthreads();
    const float e = eps_out;
    for (int b = threadIdx.x; b < B; b += MOM_WAVES * 64) eps[b] = e;
}

__global__ void step_increment_kernel(int* step) { step[0] += 1; }

// ------------------------------------------------------------------ ensemble slice sampling (zeus, Karamanis & Beutler 2021)
// state per active walker k: direction DIR[k][:], slice height Z0, bracket [L, R] in units of the
// direction, flags aL/aR (still stepping out) and aS (still shrinking).  The rules are common.h's wave-per-walker routines;
// every logic kernel below gives each wave of a block one walker and sums the block's counts before they reach the counters.
constexpr int SLICE_WAVES = 16;                        // waves (walkers) per block of the slice logic kernels
static dim3 slice_grid(int ns) { return dim3((ns + SLICE_WAVES - 1) / SLICE_WAVES); }

// the set-up of a half step: linna_slice_init, and linna_slice_half_step where its first evaluation does not do it in its
// prologue; with b.counters also the roll of that entry's usage counters
__global__ void slice_begin_kernel(const SliceBegin b, const int* __restrict__ S, int ns, int ndim, float* __restrict__ W) {
    const int k = blockIdx.x * SLICE_WAVES + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (b.counters && blockIdx.x == 0 && threadIdx.x == 0) {
        for (int i = 0; i < b.nslots; ++i) {           // [4 + nslots + i]: the same counts summed over the calls so far (usage statistics)
            b.counters[4 + b.nslots + i] += b.counters[4 + i];
            b.counters[4 + i] = 0;
        }
        b.counters[4 + 2 * b.nslots] += 1;             // calls
        if (b.zero_totals) { b.counters[0] = 0; b.counters[1] = 0; }
    }
    if (k < ns) slice_setup_wave(b, S, ns, ndim, W, k, lane);
}

// Q[j*ns + k][:] = X[S[k]][:] + w[j*ns + k] * DIR[k][:]   for j < nrep
__global__ void slice_points_kernel(const float* __restrict__ coords, int ldc, int ndim, const int* __restrict__ S, int ns,
                                    const float* __restrict__ DIR, int ldd, const float* __restrict__ w,
                                    float* __restrict__ Q, int ldq, int nrep) {
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (size_t)nrep * ns * ldq) return;
    const int row = (int)(idx / ldq), d = (int)(idx % ldq), k = row % ns;
    Q[idx] = d < ndim ? coords[(size_t)S[k] * ldc + d] + w[row] * DIR[(size_t)k * ldd + d] : 0.f;
}

// ---- the round-by-round entries: one bracket end per side, or `ntrial` trials, per launch; the host loops on counters[slot]
// stepping out: while the density at an end is above the slice, push that end out by one unit
__global__ void slice_expand_kernel(const float* __restrict__ Z0, const float* __restrict__ ZL, const float* __restrict__ ZR,
                                    float* __restrict__ L, float* __restrict__ R, int* __restrict__ flags, int ns,
                                    int* __restrict__ counters, int slot) {
    __shared__ int sums[2];
    const int k = blockIdx.x * SLICE_WAVES + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    int nexp = 0, active = 0;
    if (k < ns) {
        int fl = flags[3 * k], fr = flags[3 * k + 1];                       // steps left of the budget; 0: that side is closed
        if (fl | fr) {
            float l = L[k], r = R[k];
            slice_expand_wave(lane, k, ns, 1, Z0[k], ZL, ZR, l, r, fl, fr, flags, nexp);
            if (lane == 0) { L[k] = l; R[k] = r; }
            active = (fl | fr) != 0;
        }
    }
    block_add_counter(counters + 0, nexp, sums);                            // [0] expansions
    block_add_counter(counters + slot, active, sums + 1);                   // [slot] still-active count
}

// ntrial <= 64 trials per launch, W[j*ns + k]; Philox sub-counter round + j + 1 (the stream of single-trial rounds)
__global__ void slice_draw_kernel(const float* __restrict__ L, const float* __restrict__ R, const int* __restrict__ S,
                                  float* __restrict__ W, const int* __restrict__ flags, int ns, uint64_t seed,
                                  const int* __restrict__ step_dev, int stream_id, int round, int ntrial) {
    const int k = blockIdx.x * SLICE_WAVES + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (k >= ns || !flags[3 * k + 2]) return;
    const float w = slice_draw_wave(lane, S[k], L[k], R[k], seed, (uint32_t)step_dev[0], stream_id, round, ntrial);
    if (lane < ntrial) W[(size_t)lane * ns + k] = w;
}

// shrinking: accept the first trial inside the slice, otherwise pull the bracket in to each rejected trial
__global__ void slice_shrink_kernel(const float* __restrict__ Z0, const float* __restrict__ Zt, float* __restrict__ L,
                                    float* __restrict__ R, const float* __restrict__ W, int* __restrict__ flags,
                                    float* __restrict__ Wacc, float* __restrict__ Zacc, int ns, int* __restrict__ counters,
                                    int slot, int ntrial) {
    __shared__ int sums[2];
    const int k = blockIdx.x * SLICE_WAVES + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    int ncon = 0, active = 0;
    if (k < ns && flags[3 * k + 2]) {
        const bool in = lane < ntrial;
        const float w = in ? W[(size_t)lane * ns + k] : 0.f, zt = in ? Zt[(size_t)lane * ns + k] : 0.f;
        float l = L[k], r = R[k], wacc = 0.f, zacc = 0.f;
        active = slice_judge_wave(lane, ntrial, Z0[k], w, zt, l, r, ncon, wacc, zacc);
        if (lane == 0) {
            L[k] = l; R[k] = r;
            if (!active) { flags[3 * k + 2] = 0; Wacc[k] = wacc; Zacc[k] = zacc; }
        }
    }
    block_add_counter(counters + 1, ncon, sums);                            // [1] contractions
    block_add_counter(counters + slot, active, sums + 1);                   // [slot] still-active count
}

__global__ void slice_commit_kernel(float* __restrict__ coords, int ldc, int ndim, float* __restrict__ logp,
                                    const int* __restrict__ S, int ns, const float* __restrict__ DIR, int ldd,
                                    const float* __restrict__ Wacc, const float* __restrict__ Zacc) {
    const int k = blockIdx.x * SLICE_WAVES + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (k < ns) slice_commit_wave(lane, k, S[k], false, nullptr, Wacc[k], Zacc[k], coords, ldc, ndim, logp, DIR, ldd);
}

// ---- one-call half step (linna_slice_half_step): the same procedure with SPECULATIVE rounds, so that a half step is a
// fixed sequence of launches the host enqueues in one call and never waits for.  Stepping out: a round evaluates the
// bracket ends the sequential loop would visit next, L, L-1, ..., L-(m-1) and R, R+1, ..., R+(m-1), in ONE launch, and
// the logic below walks them in the loop's order; shrinking: `ntrial` trials per round, each placed as if its
// predecessors were rejected (slice_draw_wave's rule).  Same Philox counters, same comparisons, same accepted point
// as the one-point-per-round procedure -- only the count of evaluated-and-discarded points differs.  Rounds after the
// one that finishes the last walker are gated off on the device (the evaluation leaves at once on a zero count, the logic
// kernels return per walker on its flags).
// counters: [0] expansions, [1] contractions, [2] walkers left unfinished by the rounds of a call (sticky),
//           [3] evaluated points, [4 + r] walkers still active after round r (expand rounds first, then shrink rounds)
// Zt[j*ns + k]: lnP at L - j (j < m) and at R + (j - m) (m <= j < 2m) of the bracket this round started from; the next
// round looks at m_next ends per side (0: this is the last stepping-out round)
__device__ __forceinline__ int slice_expand_multi_wave(const float* __restrict__ Z0, const float* __restrict__ Zt, float* __restrict__ L,
                                                       float* __restrict__ R, const int* __restrict__ S, int* __restrict__ flags, int ns,
                                                       int m, int m_next, int* __restrict__ counters, int slot, int prev_slot, float* __restrict__ W,
                                                       float* __restrict__ Wd, int* __restrict__ list, uint64_t seed,
                                                       const int* __restrict__ step_dev, int stream_id_shrink, int ntrial, int k, int lane) {
    if (k == 0 && lane == 0) atomicAdd(counters + 3, 2 * m * (prev_slot < 0 ? ns : counters[prev_slot]));   // the points this round evaluated
    if (k >= ns) return 0;
    int fl = flags[3 * k], fr = flags[3 * k + 1];
    if (!(fl | fr)) return 0;
    if (prev_slot >= 0 && counters[prev_slot] == 0) return 0;     // (never: a walker with a flag set was counted)
    const float z0 = Z0[k];
    float l = L[k], r = R[k];
    int nexp = 0;
    slice_expand_wave(lane, k, ns, m, z0, Zt, Zt + (size_t)m * ns, l, r, fl, fr, flags, nexp);
    if (lane == 0) { L[k] = l; R[k] = r; }
    if (fl | fr) {
        int pos = 0;
        if (lane == 0) pos = atomicAdd(counters + slot, 1);      // rank among the walkers still stepping out: its rows of the next launch
        pos = __builtin_amdgcn_readfirstlane(pos);
        const int side = lane >> 5, j = lane & 31;
        if (j < m_next) W[(size_t)(side * m_next + j) * ns + k] = side ? r + (float)j : l - (float)j;
        if (lane < 2 * m_next) list[(size_t)pos * 2 * m_next + lane] = lane * ns + k;
    } else {
        const float w = slice_draw_wave(lane, S[k], l, r, seed, (uint32_t)step_dev[0], stream_id_shrink, 0, ntrial);   // first shrink round's trials
        if (lane < ntrial) Wd[(size_t)lane * ns + k] = w;
    }
    return nexp;
}
__global__ void slice_expand_multi_kernel(const float* __restrict__ Z0, const float* __restrict__ Zt, float* __restrict__ L,
                                          float* __restrict__ R, const int* __restrict__ S, int* __restrict__ flags, int ns,
                                          int m, int m_next, int* __restrict__ counters, int slot, int prev_slot, float* __restrict__ W,
                                          float* __restrict__ Wd, int* __restrict__ list, uint64_t seed,
                                          const int* __restrict__ step_dev, int stream_id_shrink, int ntrial) {
    __shared__ int sums[1];
    const int k = blockIdx.x * SLICE_WAVES + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    const int nexp = slice_expand_multi_wave(Z0, Zt, L, R, S, flags, ns, m, m_next, counters, slot, prev_slot, W, Wd, list, seed, step_dev,
                                             stream_id_shrink, ntrial, k, lane);
    block_add_counter(counters + 0, nexp, sums);
}

// one shrinking round (SliceRound / slice_round_wave in common.h); with `coords` the call's LAST one: the move of every
// finished walker is applied and `bump` advances the device step counter -- two launches less per iteration
__global__ void slice_shrink_multi_kernel(const SliceRound a) {
    __shared__ int sums[2];
    int nexp = 0, ncon = 0;
    slice_round_wave(a, blockIdx.x * SLICE_WAVES + (threadIdx.x >> 6), threadIdx.x & 63, nexp, ncon);
    block_add_counter(a.counters + 0, nexp, sums);
    block_add_counter(a.counters + 1, ncon, sums + 1);
}

// ------------------------------------------------------------------ host-side launchers (namespace-internal)
#define LAUNCH_CHECK(name) return check_hip(hipGetLastError(), name)

int launch_prior_map_fwd(const float* Z, int ldz, int B, int nin, const int* is_flat, const float* a1, const float* a2,
                         const int* lg, const float* xmean, const float* xstd, float* X, int ldx, float* TH, int ldt,
                         hipStream_t s) {
    hipLaunchKernelGGL(prior_map_fwd_kernel, grid1d((size_t)B * ldx, 256), dim3(256), 0, s, Z, ldz, B, nin, is_flat, a1,
                       a2, lg, xmean, xstd, X, ldx, TH, ldt);
    LAUNCH_CHECK("prior_map_fwd");
}
int launch_prior_map_bwd(const float* Z, int ldz, int B, int nin, const int* is_flat, const float* a1, const float* a2,
                         const int* lg, const float* xstd, const float* dX, int lddx, float* dZ, int lddz, hipStream_t s) {
    hipLaunchKernelGGL(prior_map_bwd_kernel, grid1d((size_t)B * nin, 256), dim3(256), 0, s, Z, ldz, B, nin, is_flat, a1,
                       a2, lg, xstd, dX, lddx, dZ, lddz);
    LAUNCH_CHECK("prior_map_bwd");
}
template <int LPR>
static void launch_loglike_diag_lpr(const float* D, int ldd, int B, int nout, const float* w, const float* Z, int ldz, int nin,
                                    float T, float* out, hipStream_t s) {
    constexpr int rows_per_block = 4 * (64 / LPR);
    hipLaunchKernelGGL(loglike_diag_kernel<LPR>, dim3((B + rows_per_block - 1) / rows_per_block), dim3(256), 0, s, D, ldd, B,
                       nout, w, Z, ldz, nin, T, out);
}
int launch_loglike_diag(const float* D, int ldd, int B, int nout, const float* w, const float* Z, int ldz, int nin,
                        float T, float* out, hipStream_t s) {
    const int q = ((nout > nin ? nout : nin) + 3) / 4;            // 16-byte chunks of the longer of the two rows
    if (q > 32) launch_loglike_diag_lpr<64>(D, ldd, B, nout, w, Z, ldz, nin, T, out, s);
    else if (q > 16) launch_loglike_diag_lpr<32>(D, ldd, B, nout, w, Z, ldz, nin, T, out, s);
    else if (q > 8) launch_loglike_diag_lpr<16>(D, ldd, B, nout, w, Z, ldz, nin, T, out, s);
    else if (q > 4) launch_loglike_diag_lpr<8>(D, ldd, B, nout, w, Z, ldz, nin, T, out, s);
    else launch_loglike_diag_lpr<4>(D, ldd, B, nout, w, Z, ldz, nin, T, out, s);
    LAUNCH_CHECK("loglike_diag");
}
int launch_loglike_finish(const float* partial, int slots_ld, int nslots, int B, const float* Z, int ldz, int nin,
                          float T, float* out, hipStream_t s) {
    hipLaunchKernelGGL(loglike_finish_kernel, dim3((B + 3) / 4), dim3(256), 0, s, partial, slots_ld, nslots, B, Z, ldz,
                       nin, T, out);
    LAUNCH_CHECK("loglike_finish");
}
int launch_loglike_diag_grad(const float* D, int ldd, int B, int nout, const float* w, const float* gscale, float T,
                             float* dH, int lddh, hipStream_t s) {
    hipLaunchKernelGGL(loglike_diag_grad_kernel, grid1d((size_t)B * lddh, 256), dim3(256), 0, s, D, ldd, B, nout, w,
                       gscale, T, dH, lddh);
    LAUNCH_CHECK("loglike_diag_grad");
}
int launch_loss_delta(int mode, const float* PRED, int ldp, const float* Y, int ldy, const int* ROWS, int B,
                      const linna_loss_desc_t& d, float* DELTA, int ldd, hipStream_t s) {
    hipLaunchKernelGGL(loss_delta_kernel, grid1d((size_t)B * ldd, 256), dim3(256), 0, s, mode, PRED, ldp, Y, ldy, ROWS,
                       B, d.nout, d.sigma, d.ymean, d.ystd, d.ylog, d.data_norm, DELTA, ldd);
    LAUNCH_CHECK("loss_delta");
}
int launch_loss_targets(const float* Y, int ldy, int n, const linna_loss_desc_t& d, float* YN, int ldyn, hipStream_t s) {
    hipLaunchKernelGGL(loss_targets_kernel, grid1d((size_t)n * ldyn, 256), dim3(256), 0, s, Y, ldy, n, d.nout, d.sigma, d.ymean,
                       d.ystd, d.ylog, d.data_norm, YN, ldyn);
    LAUNCH_CHECK("loss_targets");
}
int launch_loss_fused_small(const float* PRED, int ldp, const float* Y, int ldy, const int* ROWS, int B,
                            const linna_loss_desc_t& d, const float* den, float inv_batch, float* loss_rows, float* loss_mean,
                            float* dP, int lddp, unsigned* counter, hipStream_t s) {
    hipLaunchKernelGGL(loss_fused_small_kernel, dim3((B + 3) / 4), dim3(256), 0, s, PRED, ldp, Y, ldy, ROWS, B, d.nout, d.sigma,
                       d.ymean, d.ystd, d.ylog, d.data_norm, d.Cinv, d.ldc, den, inv_batch, loss_rows, loss_mean, dP, lddp, counter);
    LAUNCH_CHECK("loss_fused_small");
}
int launch_loss_rows(int mode, const float* partial, int slots_ld, int nslots, int B, const float* den, const int* ROWS,
                     float floorv, float* out, hipStream_t s) {
    hipLaunchKernelGGL(loss_rows_kernel, grid1d(B, 256), dim3(256), 0, s, mode, partial, slots_ld, nslots, B, den, ROWS,
                       floorv, out);
    LAUNCH_CHECK("loss_rows");
}
int launch_loss_grad(const float* U, int ldu, const float* Y, int ldy, const int* ROWS, int B, int nout,
                     const float* data_norm, const float* den, float inv_batch, float* dP, int lddp, hipStream_t s) {
    hipLaunchKernelGGL(loss_grad_kernel, grid1d((size_t)B * lddp, 256), dim3(256), 0, s, U, ldu, Y, ldy, ROWS, B, nout,
                       data_norm, den, inv_batch, dP, lddp);
    LAUNCH_CHECK("loss_grad");
}
int launch_sum_scale(const float* v, int n, float scale, float* out, hipStream_t s) {
    hipLaunchKernelGGL(sum_scale_kernel, dim3(1), dim3(1024), 0, s, v, n, scale, out);
    LAUNCH_CHECK("sum_scale");
}
int launch_sum_scale_prepare(const float* v, int n, float scale, float* out, int* step_dev, float* hyper, float b1, float b2,
                             hipStream_t s) {
    hipLaunchKernelGGL(sum_scale_prepare_kernel, dim3(1), dim3(1024), 0, s, v, n, scale, out, step_dev, hyper, b1, b2);
    LAUNCH_CHECK("sum_scale_prepare");
}
int launch_val_frac(const float* partial, int slots_ld, int nslots, int B, const float* den, float* frac, hipStream_t s) {
    hipLaunchKernelGGL(val_frac_kernel, grid1d(B, 256), dim3(256), 0, s, partial, slots_ld, nslots, B, den, frac);
    LAUNCH_CHECK("val_frac");
}
int launch_val_metrics(const float* loss, const float* frac, int n, const float* last, float* out, hipStream_t s) {
    hipLaunchKernelGGL(val_metrics_kernel, grid1d(n, 256), dim3(256), 0, s, loss, frac, n, last, out);
    LAUNCH_CHECK("val_metrics");
}
int launch_gather_xform(const float* X, int ldx, const int* ROWS, int B, int nin, const int* lg, const float* xmean,
                        const float* xstd, float* XB, int ldxb, hipStream_t s) {
    hipLaunchKernelGGL(gather_xform_kernel, grid1d((size_t)B * ldxb, 256), dim3(256), 0, s, X, ldx, ROWS, B, nin, lg,
                       xmean, xstd, XB, ldxb);
    LAUNCH_CHECK("gather_xform");
}
int launch_colsum(const float* dZ, int ld, int B, int N, float scale, float* db, hipStream_t s) {
    hipLaunchKernelGGL(colsum_kernel, dim3((N + 63) / 64), dim3(1024), 0, s, dZ, ld, B, N, scale, db);
    LAUNCH_CHECK("colsum");
}
int launch_adamw(float* p, const float* g, float* m, float* v, size_t n, float* hyper, int* step_dev, float b1, float b2,
                 float eps, hipStream_t s) {
    if (step_dev) hipLaunchKernelGGL(adamw_prepare_kernel, dim3(1), dim3(1), 0, s, step_dev, hyper, b1, b2);   // null: already advanced
    hipLaunchKernelGGL(adamw_kernel, grid1d(n, 256), dim3(256), 0, s, p, g, m, v, n, hyper, b1, b2, eps);
    LAUNCH_CHECK("adamw");
}
int launch_adamw_prepare(float* hyper, int* step_dev, float b1, float b2, hipStream_t s) {
    hipLaunchKernelGGL(adamw_prepare_kernel, dim3(1), dim3(1), 0, s, step_dev, hyper, b1, b2);
    LAUNCH_CHECK("adamw_prepare");
}
int launch_stretch_propose(const float* coords, int ldc, int ndim, const int* S, int ns, const float* ccoords, int ldcc,
                           const int* C, int nc, uint64_t seed, const int* step_dev, int stream_id, float a, float* Q,
                           int ldq, float* factors, hipStream_t s) {
    hipLaunchKernelGGL(stretch_propose_kernel, grid1d((size_t)ns * ldq, 256), dim3(256), 0, s, coords, ldc, ndim, S, ns,
                       ccoords, ldcc, C, nc, seed, step_dev, stream_id, a, Q, ldq, factors);
    LAUNCH_CHECK("stretch_propose");
}
int launch_stretch_accept(float* coords, int ldc, int ndim, float* logp, const int* S, int ns, const float* Q, int ldq,
                          const float* lp_new, const float* factors, uint64_t seed, const int* step_dev, int stream_id,
                          int* naccept, hipStream_t s) {
    hipLaunchKernelGGL(stretch_accept_kernel, grid1d(ns, 256), dim3(256), 0, s, coords, ldc, ndim, logp, S, ns, Q, ldq,
                       lp_new, factors, seed, step_dev, stream_id, naccept);
    LAUNCH_CHECK("stretch_accept");
}
int launch_hmc_start(int B, int ndim, const float* mass, uint64_t seed, const int* step_dev, const float* lnp, const float* P0,
                     int ldp0, const float* G, int ldg, float ek, float ed, const float* X, int ldx, float* P, int ldp, float* Q,
                     int ldq, float* H0, hipStream_t s, const float* eps, int step_off) {
    hipLaunchKernelGGL(hmc_start_kernel, dim3((B + 3) / 4), dim3(256), 0, s, B, ndim, mass, seed, step_dev, lnp, P0, ldp0, G, ldg, ek,
                       ed, X, ldx, P, ldp, Q, ldq, H0, eps, step_off);
    LAUNCH_CHECK("hmc_start");
}
int launch_hmc_kick_drift(int B, int ndim, const float* mass, float ek, float ed, const float* G, int ldg, float* P,
                          int ldp, float* Q, int ldq, hipStream_t s, const float* eps) {
    hipLaunchKernelGGL(hmc_kick_drift_kernel, grid1d((size_t)B * ndim, 256), dim3(256), 0, s, B, ndim, mass, ek, ed, G,
                       ldg, P, ldp, Q, ldq, eps);
    LAUNCH_CHECK("hmc_kick_drift");
}
int launch_hmc_accept(int B, int ndim, const float* mass, uint64_t seed, const int* step_dev, int step_off, const float* H0,
                      const float* P, int ldp, const float* Qn, int ldq, const float* lnp_new, const float* Gn, int ldg,
                      const float* U, float* X, int ldx, float* lnp, float* G, int* naccept, float* alpha,
                      const HmcAdapt& ad, float* chain, float* logps, const HmcEnergy& en, hipStream_t s) {
    hipLaunchKernelGGL(hmc_accept_kernel, dim3((B + 3) / 4), dim3(256), 0, s, B, ndim, mass, seed, step_dev, step_off, H0, P,
                       ldp, Qn, ldq, lnp_new, Gn, ldg, U, X, ldx, lnp, G, naccept, alpha, ad, chain, logps, en);
    LAUNCH_CHECK("hmc_accept");
}
int launch_hmc_energy_finish(int B, const double* estate, const int* ndiv, float* bfmi, double* pooled, hipStream_t s) {
    hipLaunchKernelGGL(hmc_energy_finish_kernel, dim3(1), dim3(ENERGY_WAVES * 64), 0, s, B, estate, ndiv, bfmi, pooled);
    LAUNCH_CHECK("hmc_energy_finish");
}
int launch_hmc_find_eps_init(int B, int ndim, uint64_t seed, const int* step_dev, int step_off, float* R0, int ldr, float* eps,
                             int* state, hipStream_t s) {
    hipLaunchKernelGGL(hmc_find_eps_init_kernel, grid1d((size_t)B * ndim, 256), dim3(256), 0, s, B, ndim, seed, step_dev, step_off,
                       R0, ldr, eps, state);
    LAUNCH_CHECK("hmc_find_eps_init");
}
int launch_hmc_find_eps(int B, int ndim, const float* mass, const float* H0, const float* P, int ldp, const float* lnp_new,
                        const float* Gn, int ldg, float* eps, int* state, int* nactive, hipStream_t s) {
    hipLaunchKernelGGL(hmc_find_eps_kernel, dim3((B + 3) / 4), dim3(256), 0, s, B, ndim, mass, H0, P, ldp, lnp_new, Gn, ldg, eps,
                       state, nactive);
    LAUNCH_CHECK("hmc_find_eps");
}
int launch_hmc_moments(int B, int ndim, const float* X, int ldx, double* mom, hipStream_t s) {
    hipLaunchKernelGGL(hmc_moments_kernel, dim3(1), dim3(MOM_WAVES * 64), 0, s, B, ndim, X, ldx, mom);
    LAUNCH_CHECK("hmc_moments");
}
int launch_hmc_mass_from_moments(int ndim, double* mom, float* mass, int reset, hipStream_t s) {
    hipLaunchKernelGGL(hmc_mass_from_moments_kernel, dim3(1), dim3(256), 0, s, ndim, mom, mass, reset);
    LAUNCH_CHECK("hmc_mass_from_moments");
}
int launch_hmc_comoments(int B, int ndim, const float* X, int ldx, double* mom, hipStream_t s) {
    const int nt = (ndim + COMOM_T - 1) / COMOM_T;
    hipLaunchKernelGGL(hmc_comoments_kernel, dim3(nt * (nt + 1) / 2, COMOM_SLOTS), dim3(COMOM_WAVES * 64), 0, s, B, ndim, X, ldx, mom);
    LAUNCH_CHECK("hmc_comoments");
}
int launch_hmc_chol_from_comoments(int ndim, double* mom, float* Cm, int ldc, int* info, int reset, hipStream_t s) {
    hipLaunchKernelGGL(hmc_chol_from_comoments_kernel, dim3(1), dim3(CHOL_THREADS), 0, s, ndim, mom, Cm, ldc, info, reset);
    LAUNCH_CHECK("hmc_chol_from_comoments");
}
int launch_hmc_kick_drift_dense(int B, int ndim, const float* Cm, int ldc, const float* eps, float ek, float ed, const float* G,
                                int ldg, float* W, int ldw, const float* X, int ldx, float* Q, int ldq, hipStream_t s) {
    hipLaunchKernelGGL(hmc_kick_drift_dense_kernel, dim3((B + 3) / 4), dim3(256), 0, s, B, ndim, Cm, ldc, eps, ek, ed, G, ldg, W,
                       ldw, X, ldx, Q, ldq);
    LAUNCH_CHECK("hmc_kick_drift_dense");
}
int launch_hmc_chees_begin(int B, int ndim, const float* X, int ldx, double* state, double* r0, hipStream_t s) {
    hipLaunchKernelGGL(hmc_chees_begin_kernel, dim3(1), dim3(MOM_WAVES * 64), 0, s, B, ndim, X, ldx, state, r0);
    LAUNCH_CHECK("hmc_chees_begin");
}
int launch_hmc_chees_end(int B, int ndim, const float* mass, const float* Cm, int ldc, const float* Q, int ldq, const float* P, int ldp,
                         const float* alpha, const double* r0, double* state, float* eps, int M, double delta, int max_steps,
                         hipStream_t s) {
    if (Cm) hipLaunchKernelGGL(hmc_chees_end_kernel<true>, dim3(1), dim3(MOM_WAVES * 64), 0, s, B, ndim, mass, Cm, ldc, Q, ldq, P, ldp,
                               alpha, r0, state, eps, M, delta, max_steps);
    else hipLaunchKernelGGL(hmc_chees_end_kernel<false>, dim3(1), dim3(MOM_WAVES * 64), 0, s, B, ndim, mass, Cm, ldc, Q, ldq, P, ldp,
                            alpha, r0, state, eps, M, delta, max_steps);
    LAUNCH_CHECK("hmc_chees_end");
}
int launch_slice_points(const float* coords, int ldc, int ndim, const int* S, int ns, const float* DIR, int ldd,
                        const float* w, float* Q, int ldq, int nrep, hipStream_t s) {
    hipLaunchKernelGGL(slice_points_kernel, grid1d((size_t)nrep * ns * ldq, 256), dim3(256), 0, s, coords, ldc, ndim, S, ns, DIR,
                       ldd, w, Q, ldq, nrep);
    LAUNCH_CHECK("slice_points");
}
#define SLICE_LAUNCH(kernel, ns, ...) hipLaunchKernelGGL(kernel, slice_grid(ns), dim3(64 * SLICE_WAVES), 0, s, __VA_ARGS__)
int launch_slice_begin(const SliceBegin& b, const int* S, int ns, int ndim, float* W, hipStream_t s) {
    SLICE_LAUNCH(slice_begin_kernel, ns, b, S, ns, ndim, W);
    LAUNCH_CHECK("slice_begin");
}
int launch_slice_expand(const float* Z0, const float* ZL, const float* ZR, float* L, float* R, int* flags, int ns,
                        int* counters, int slot, hipStream_t s) {
    SLICE_LAUNCH(slice_expand_kernel, ns, Z0, ZL, ZR, L, R, flags, ns, counters, slot);
    LAUNCH_CHECK("slice_expand");
}
int launch_slice_draw(const float* L, const float* R, const int* S, float* W, const int* flags, int ns, uint64_t seed,
                      const int* step_dev, int stream_id, int round, int ntrial, hipStream_t s) {
    SLICE_LAUNCH(slice_draw_kernel, ns, L, R, S, W, flags, ns, seed, step_dev, stream_id, round, ntrial);
    LAUNCH_CHECK("slice_draw");
}
int launch_slice_shrink(const float* Z0, const float* Zt, float* L, float* R, const float* W, int* flags, float* Wacc,
                        float* Zacc, int ns, int* counters, int slot, int ntrial, hipStream_t s) {
    SLICE_LAUNCH(slice_shrink_kernel, ns, Z0, Zt, L, R, W, flags, Wacc, Zacc, ns, counters, slot, ntrial);
    LAUNCH_CHECK("slice_shrink");
}
int launch_slice_commit(float* coords, int ldc, int ndim, float* logp, const int* S, int ns, const float* DIR, int ldd,
                        const float* Wacc, const float* Zacc, hipStream_t s) {
    SLICE_LAUNCH(slice_commit_kernel, ns, coords, ldc, ndim, logp, S, ns, DIR, ldd, Wacc, Zacc);
    LAUNCH_CHECK("slice_commit");
}
int launch_slice_expand_multi(const float* Z0, const float* Zt, float* L, float* R, const int* S, int* flags, int ns, int m,
                              int m_next, int* counters, int slot, int prev_slot, float* W, float* Wd, int* list, uint64_t seed,
                              const int* step_dev, int stream_id_shrink, int ntrial, hipStream_t s) {
    SLICE_LAUNCH(slice_expand_multi_kernel, ns, Z0, Zt, L, R, S, flags, ns, m, m_next, counters, slot, prev_slot, W, Wd, list, seed,
                 step_dev, stream_id_shrink, ntrial);
    LAUNCH_CHECK("slice_expand_multi");
}
int launch_slice_shrink_multi(const SliceRound& a, hipStream_t s) {
    SLICE_LAUNCH(slice_shrink_multi_kernel, a.ns, a);
    LAUNCH_CHECK("slice_shrink_multi");
}
int launch_step_increment(int* step, hipStream_t s) {
    hipLaunchKernelGGL(step_increment_kernel, dim3(1), dim3(1), 0, s, step);
    LAUNCH_CHECK("step_increment");
}

}  // namespace linna
