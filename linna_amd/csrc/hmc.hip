// Hamiltonian Monte Carlo on gfx950, one file for the subsystem: its kernels (momentum draw, leapfrog kick and drift, the
// Metropolis test with step-size adaptation and energy diagnostics, find_reasonable_epsilon, diagonal and dense mass
// adaptation, the ChEES trajectory length), their launch code and the linna_hmc_* entries of include/linna_hip.h, the ones
// that run whole transitions per call included.  The gradient is not here: the driver sees of a log-probability object
// what common.h declares next to NsLeap (logprob_nin, logprob_grad_ready, logprob_grad_impl) and nothing else, and api.hip's
// layered gradient route calls launch_hmc_kick_drift, the one launcher of this file that is not static.
#include "common.h"
#include <math.h>

namespace linna {

// the dual-averaging state of hmc_accept_kernel, one entry per chain (sampler.py:198-240 of the reference)
struct HmcAdapt { float* eps; float* epsbar; float* Hbar; const float* mu; int* m; int Madapt; float delta; };
// the energy diagnostics of hmc_accept_kernel (linna_hip.h, linna_hmc_accept_energy): estate[B][LINNA_HMC_ENERGY_DOUBLES] with
// ndiv[B] (both or neither), energy[B] and dH[B] each nullable; HmcEnergy{}: the kernel does what it did before the group
struct HmcEnergy { double* estate; int* ndiv; float max_dH; float* energy; float* dH; };

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

// ------------------------------------------------------------------ launch code
// Only the launches with more than one caller below have a function: every other kernel is launched by its entry.
// eps (nullable, here and below): a step size per chain in device memory, ek / ed then multiply it; step_off: added to step_dev[0].
// G == nullptr (X, Q then unused): only the momenta and H0, what linna_hmc_init asks for
static int launch_hmc_start(int B, int ndim, const float* mass, uint64_t seed, const int* step_dev, const float* lnp, const float* P0,
                            int ldp0, const float* G, int ldg, float ek, float ed, const float* X, int ldx, float* P, int ldp, float* Q,
                            int ldq, float* H0, hipStream_t s, const float* eps = nullptr, int step_off = 0) {
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
// the one Metropolis launcher: alpha, chain, logps, ad.m and en's pointers are each nullable (linna_hmc_accept passes all of them null)
static int launch_hmc_accept(int B, int ndim, const float* mass, uint64_t seed, const int* step_dev, int step_off, const float* H0,
                             const float* P, int ldp, const float* Qn, int ldq, const float* lnp_new, const float* Gn, int ldg,
                             const float* U, float* X, int ldx, float* lnp, float* G, int* naccept, float* alpha,
                             const HmcAdapt& ad, float* chain, float* logps, const HmcEnergy& en, hipStream_t s) {
    hipLaunchKernelGGL(hmc_accept_kernel, dim3((B + 3) / 4), dim3(256), 0, s, B, ndim, mass, seed, step_dev, step_off, H0, P,
                       ldp, Qn, ldq, lnp_new, Gn, ldg, U, X, ldx, lnp, G, naccept, alpha, ad, chain, logps, en);
    LAUNCH_CHECK("hmc_accept");
}
static int launch_hmc_moments(int B, int ndim, const float* X, int ldx, double* mom, hipStream_t s) {
    hipLaunchKernelGGL(hmc_moments_kernel, dim3(1), dim3(MOM_WAVES * 64), 0, s, B, ndim, X, ldx, mom);
    LAUNCH_CHECK("hmc_moments");
}
static int launch_hmc_comoments(int B, int ndim, const float* X, int ldx, double* mom, hipStream_t s) {
    const int nt = (ndim + COMOM_T - 1) / COMOM_T;
    hipLaunchKernelGGL(hmc_comoments_kernel, dim3(nt * (nt + 1) / 2, COMOM_SLOTS), dim3(COMOM_WAVES * 64), 0, s, B, ndim, X, ldx, mom);
    LAUNCH_CHECK("hmc_comoments");
}
static int launch_hmc_kick_drift_dense(int B, int ndim, const float* Cm, int ldc, const float* eps, float ek, float ed, const float* G,
                                       int ldg, float* W, int ldw, const float* X, int ldx, float* Q, int ldq, hipStream_t s) {
    hipLaunchKernelGGL(hmc_kick_drift_dense_kernel, dim3((B + 3) / 4), dim3(256), 0, s, B, ndim, Cm, ldc, eps, ek, ed, G, ldg, W,
                       ldw, X, ldx, Q, ldq);
    LAUNCH_CHECK("hmc_kick_drift_dense");
}

}  // namespace linna

using namespace linna;

// ------------------------------------------------------------------ whole HMC transitions per call (linna_hip.h)
static bool hmc_state_ok(const linna_hmc_state_t* st) {
    return st && st->B >= 1 && st->ld >= 1 && st->X && st->lnp && st->G && st->P && st->Q && st->lnp_new && st->Gnew && st->H0 &&
           st->mass && st->step_dev;
}
// what the entries that run whole transitions check of their state before they enqueue anything
static int hmc_entry_check(const linna_logprob_t* lp, const linna_hmc_state_t* st, const char* who) {
    CHECK_STRUCT(st, linna_hmc_state_t, who);
    if (!hmc_state_ok(st)) { set_error("%s: incomplete state", who); return LINNA_ERR_INVALID; }
    const int nd = logprob_nin(lp);
    if (st->ld < nd) { set_error("%s: ld %d < %d parameters", who, st->ld, nd); return LINNA_ERR_INVALID; }
    return logprob_grad_ready(lp);
}
// a dense mass's factor {C, C^T} (linna_hip.h); C == nullptr: the diagonal route
struct HmcDense { const float* C; int ldc; };
// what every entry that takes a dense mass checks of its width; ldc (nullable): and of the factor's leading dimension
static int hmc_dense_check(int ndim, const int* ldc, const char* who) {
    if (ndim > LINNA_HMC_DENSE_MAX_NDIM) {
        set_error("%s: a dense mass holds at most %d parameters, not %d", who, LINNA_HMC_DENSE_MAX_NDIM, ndim); return LINNA_ERR_UNSUPPORTED;
    }
    if (ldc && *ldc < ndim) { set_error("%s: ldc %d < %d parameters", who, *ldc, ndim); return LINNA_ERR_INVALID; }
    return LINNA_OK;
}
// one trajectory from st->X with the momenta hmc_start draws (P0 == nullptr) or is given: start, num_steps gradient launches.
// dn.C: st->P is the whitened momentum (st->mass an array of ones), the gradient launch runs without a leapfrog in its finish
// and the dense kick and drift follow it as a launch of their own
static int hmc_trajectory(linna_logprob_t* lp, const linna_hmc_state_t* st, void* ws, const float* P0, const float* EPS, int step_off,
                          int num_steps, void* stream, const HmcDense& dn = HmcDense{nullptr, 0}) {
    const int B = st->B, nd = logprob_nin(lp), ld = st->ld;
    if (dn.C) {
        TRY(launch_hmc_start(B, nd, st->mass, st->seed, st->step_dev, st->lnp, P0, ld, nullptr, 0, 0.f, 0.f, nullptr, 0, st->P, ld,
                             nullptr, 0, st->H0, S(stream), nullptr, step_off));
        TRY(launch_hmc_kick_drift_dense(B, nd, dn.C, dn.ldc, EPS, 0.5f, 1.f, st->G, ld, st->P, ld, st->X, ld, st->Q, ld, S(stream)));
        for (int i = 0; i < num_steps; ++i) {
            const bool last = i == num_steps - 1;
            TRY(logprob_grad_impl(lp, st->Q, ld, B, ws, st->lnp_new, st->Gnew, ld, nullptr, stream));
            TRY(launch_hmc_kick_drift_dense(B, nd, dn.C, dn.ldc, EPS, last ? 0.5f : 1.f, last ? 0.f : 1.f, st->Gnew, ld, st->P, ld,
                                            nullptr, 0, st->Q, ld, S(stream)));
        }
        return LINNA_OK;
    }
    TRY(launch_hmc_start(B, nd, st->mass, st->seed, st->step_dev, st->lnp, P0, ld, st->G, ld, 0.5f, 1.f, st->X, ld, st->P, ld, st->Q, ld,
                         st->H0, S(stream), EPS, step_off));
    for (int i = 0; i < num_steps; ++i) {
        const bool last = i == num_steps - 1;                                      // a half kick behind the last step, no drift
        const NsLeap leap{st->P, ld, st->Q, st->mass, last ? 0.5f : 1.f, last ? 0.f : 1.f, EPS};
        TRY(logprob_grad_impl(lp, st->Q, ld, B, ws, st->lnp_new, st->Gnew, ld, &leap, stream));
    }
    return LINNA_OK;
}

// what the entries that take the energy diagnostics check of them (linna_hip.h): estate with ndiv, and then max_dH > 0
static int hmc_energy_check(const HmcEnergy& en, const char* who) {
    if ((en.estate != nullptr) != (en.ndiv != nullptr)) { set_error("%s: estate and ndiv come together", who); return LINNA_ERR_INVALID; }
    if (en.estate && !(en.max_dH > 0.f)) { set_error("%s: max_dH %g is not positive", who, (double)en.max_dH); return LINNA_ERR_INVALID; }
    return LINNA_OK;
}
// linna_hmc_run, linna_hmc_run_moments, linna_hmc_run_dense and linna_hmc_run_energy: mom != nullptr adds the moments launch on
// st->X behind every Metropolis launch (under a dense mass the co-moments launch); en: the energy diagnostics in that launch,
// its energy / dH rows [ntrans][B]
static int hmc_run_impl(linna_logprob_t* lp, const linna_hmc_state_t* st, void* ws, float* EPS, float* EPSBAR, float* HBAR, const float* MU,
                        int* M, int Madapt, float delta, int step_offset, int num_steps, int ntrans, int* naccept, float* alpha,
                        float* chain, float* logps, double* mom, void* stream, const HmcDense& dn = HmcDense{nullptr, 0},
                        const HmcEnergy& en = HmcEnergy{}) {
    if (!lp || !st || !ws || !EPS || num_steps < 1 || ntrans < 1 || Madapt < 0 || (chain != nullptr) != (logps != nullptr)) {
        set_error("hmc_run: bad arguments"); return LINNA_ERR_INVALID;
    }
    if (Madapt > 0 && (!EPSBAR || !HBAR || !MU || !M)) { set_error("hmc_run: Madapt > 0 needs the adaptation state"); return LINNA_ERR_INVALID; }
    TRY(hmc_energy_check(en, "hmc_run_energy"));
    TRY(hmc_entry_check(lp, st, "hmc_run"));
    const int B = st->B, nd = logprob_nin(lp), ld = st->ld;
    if (dn.C) TRY(hmc_dense_check(nd, &dn.ldc, "hmc_run_dense"));
    const HmcAdapt ad{EPS, EPSBAR, HBAR, MU, M, Madapt, delta};
    for (int i = 0; i < ntrans; ++i) {
        TRY(hmc_trajectory(lp, st, ws, nullptr, EPS, step_offset + i, num_steps, stream, dn));
        const HmcEnergy row{en.estate, en.ndiv, en.max_dH, en.energy ? en.energy + (size_t)i * B : nullptr,
                            en.dH ? en.dH + (size_t)i * B : nullptr};
        TRY(launch_hmc_accept(B, nd, st->mass, st->seed, st->step_dev, step_offset + i, st->H0, st->P, ld, st->Q, ld, st->lnp_new,
                              st->Gnew, ld, nullptr, st->X, ld, st->lnp, st->G, naccept, alpha, ad,
                              chain ? chain + (size_t)i * B * nd : nullptr, logps ? logps + (size_t)i * B : nullptr, row, S(stream)));
        if (mom) TRY(dn.C ? launch_hmc_comoments(B, nd, st->X, ld, mom, S(stream)) : launch_hmc_moments(B, nd, st->X, ld, mom, S(stream)));
    }
    return LINNA_OK;
}

int linna_hmc_run(linna_logprob_t* lp, const linna_hmc_state_t* st, void* ws, float* EPS, float* EPSBAR, float* HBAR, const float* MU,
                  int* M, int Madapt, float delta, int step_offset, int num_steps, int ntrans, int* naccept, float* alpha,
                  float* chain, float* logps, void* stream) try {
    return hmc_run_impl(lp, st, ws, EPS, EPSBAR, HBAR, MU, M, Madapt, delta, step_offset, num_steps, ntrans, naccept, alpha, chain,
                        logps, nullptr, stream);
} LINNA_CATCH_INT

int linna_hmc_run_moments(linna_logprob_t* lp, const linna_hmc_state_t* st, void* ws, float* EPS, float* EPSBAR, float* HBAR,
                          const float* MU, int* M, int Madapt, float delta, int step_offset, int num_steps, int ntrans,
                          int* naccept, float* alpha, float* chain, float* logps, double* mom, void* stream) try {
    return hmc_run_impl(lp, st, ws, EPS, EPSBAR, HBAR, MU, M, Madapt, delta, step_offset, num_steps, ntrans, naccept, alpha, chain,
                        logps, mom, stream);
} LINNA_CATCH_INT

static int hmc_find_epsilon_impl(linna_logprob_t* lp, const linna_hmc_state_t* st, void* ws, float* R0, float* EPS, int* state, int* nactive,
                                 int step_offset, int max_rounds, void* stream, const HmcDense& dn) {
    if (!lp || !st || !ws || !R0 || !EPS || !state || !nactive || max_rounds < 1) { set_error("hmc_find_epsilon: bad arguments"); return LINNA_ERR_INVALID; }
    TRY(hmc_entry_check(lp, st, "hmc_find_epsilon"));
    const int B = st->B, nd = logprob_nin(lp), ld = st->ld;
    if (dn.C) TRY(hmc_dense_check(nd, &dn.ldc, "hmc_find_epsilon_dense"));
    TRY(check_hip(hipMemsetAsync(nactive, 0, sizeof(int), S(stream)), "hipMemsetAsync"));
    hipLaunchKernelGGL(hmc_find_eps_init_kernel, grid1d((size_t)B * nd, 256), dim3(256), 0, S(stream), B, nd, st->seed, st->step_dev,
                       step_offset, R0, ld, EPS, state);
    TRY(check_hip(hipGetLastError(), "hmc_find_eps_init"));
    for (int r = 0; r < max_rounds; ++r) {
        TRY(hmc_trajectory(lp, st, ws, R0, EPS, step_offset, 1, stream, dn));
        hipLaunchKernelGGL(hmc_find_eps_kernel, dim3((B + 3) / 4), dim3(256), 0, S(stream), B, nd, st->mass, st->H0, st->P, ld,
                           st->lnp_new, st->Gnew, ld, EPS, state, r + 1 == max_rounds ? nactive : nullptr);
        TRY(check_hip(hipGetLastError(), "hmc_find_eps"));
    }
    return LINNA_OK;
}

int linna_hmc_find_epsilon(linna_logprob_t* lp, const linna_hmc_state_t* st, void* ws, float* R0, float* EPS, int* state, int* nactive,
                           int step_offset, int max_rounds, void* stream) try {
    return hmc_find_epsilon_impl(lp, st, ws, R0, EPS, state, nactive, step_offset, max_rounds, stream, HmcDense{nullptr, 0});
} LINNA_CATCH_INT

int linna_hmc_run_dense(linna_logprob_t* lp, const linna_hmc_state_t* st, void* ws, const float* Cm, int ldc, float* EPS, float* EPSBAR,
                        float* HBAR, const float* MU, int* M, int Madapt, float delta, int step_offset, int num_steps, int ntrans,
                        int* naccept, float* alpha, float* chain, float* logps, double* mom, void* stream) try {
    if (!Cm) { set_error("hmc_run_dense: no factor"); return LINNA_ERR_INVALID; }
    return hmc_run_impl(lp, st, ws, EPS, EPSBAR, HBAR, MU, M, Madapt, delta, step_offset, num_steps, ntrans, naccept, alpha, chain,
                        logps, mom, stream, HmcDense{Cm, ldc});
} LINNA_CATCH_INT

int linna_hmc_run_energy(linna_logprob_t* lp, const linna_hmc_state_t* st, void* ws, const float* Cm, int ldc, float* EPS, float* EPSBAR,
                         float* HBAR, const float* MU, int* M, int Madapt, float delta, int step_offset, int num_steps, int ntrans,
                         int* naccept, float* alpha, float* chain, float* logps, double* mom, double* estate, int* ndiv, float max_dH,
                         float* energy, float* dH, void* stream) try {
    return hmc_run_impl(lp, st, ws, EPS, EPSBAR, HBAR, MU, M, Madapt, delta, step_offset, num_steps, ntrans, naccept, alpha, chain,
                        logps, mom, stream, HmcDense{Cm, Cm ? ldc : 0}, HmcEnergy{estate, ndiv, max_dH, energy, dH});
} LINNA_CATCH_INT

int linna_hmc_find_epsilon_dense(linna_logprob_t* lp, const linna_hmc_state_t* st, void* ws, const float* Cm, int ldc, float* R0,
                                 float* EPS, int* state, int* nactive, int step_offset, int max_rounds, void* stream) try {
    if (!Cm) { set_error("hmc_find_epsilon_dense: no factor"); return LINNA_ERR_INVALID; }
    return hmc_find_epsilon_impl(lp, st, ws, R0, EPS, state, nactive, step_offset, max_rounds, stream, HmcDense{Cm, ldc});
} LINNA_CATCH_INT

// ------------------------------------------------------------------ a transition launch by launch, and the adaptations' own entries
int linna_hmc_init(linna_ctx_t*, int B, int ndim, const float* mass, uint64_t seed, const int* step_dev, const float* lnp,
                   const float* P0, int ldp0, float* P, int ldp, float* H0, void* stream) try {
    return launch_hmc_start(B, ndim, mass, seed, step_dev, lnp, P0, ldp0, nullptr, 0, 0.f, 0.f, nullptr, 0, P, ldp, nullptr, 0, H0, S(stream));
} LINNA_CATCH_INT
int linna_hmc_start(linna_ctx_t*, int B, int ndim, const float* mass, uint64_t seed, const int* step_dev, const float* lnp,
                    const float* P0, int ldp0, const float* G, int ldg, float eps_kick, float eps_drift, const float* X, int ldx,
                    float* P, int ldp, float* Q, int ldq, float* H0, void* stream) try {
    if (B < 1 || ndim < 1 || !mass || !step_dev || !lnp || !G || !X || !P || !Q || !H0) { set_error("hmc_start: bad arguments"); return LINNA_ERR_INVALID; }
    return launch_hmc_start(B, ndim, mass, seed, step_dev, lnp, P0, ldp0, G, ldg, eps_kick, eps_drift, X, ldx, P, ldp, Q, ldq, H0, S(stream));
} LINNA_CATCH_INT
int linna_hmc_kick_drift(linna_ctx_t*, int B, int ndim, const float* mass, float ek, float ed, const float* G, int ldg,
                         float* P, int ldp, float* Q, int ldq, void* stream) try {
    return launch_hmc_kick_drift(B, ndim, mass, ek, ed, G, ldg, P, ldp, Q, ldq, S(stream));
} LINNA_CATCH_INT
int linna_hmc_moments(linna_ctx_t*, int B, int ndim, const float* X, int ldx, double* mom, void* stream) try {
    if (B < 1 || ndim < 1 || !X || ldx < ndim || !mom) { set_error("hmc_moments: bad arguments"); return LINNA_ERR_INVALID; }
    return launch_hmc_moments(B, ndim, X, ldx, mom, S(stream));
} LINNA_CATCH_INT
int linna_hmc_mass_from_moments(linna_ctx_t*, int ndim, double* mom, float* mass, int reset, void* stream) try {
    if (ndim < 1 || !mom || !mass) { set_error("hmc_mass_from_moments: bad arguments"); return LINNA_ERR_INVALID; }
    hipLaunchKernelGGL(hmc_mass_from_moments_kernel, dim3(1), dim3(256), 0, S(stream), ndim, mom, mass, reset);
    LAUNCH_CHECK("hmc_mass_from_moments");
} LINNA_CATCH_INT
size_t linna_hmc_comoments_doubles(int ndim) try {
    if (ndim < 1 || ndim > LINNA_HMC_DENSE_MAX_NDIM) return 0;
    return 1 + (size_t)ndim + LINNA_HMC_COMOMENT_SLOTS * ((size_t)ndim + (size_t)ndim * ndim);
} LINNA_CATCH_SIZE
int linna_hmc_comoments(linna_ctx_t*, int B, int ndim, const float* X, int ldx, double* mom, void* stream) try {
    if (B < 1 || ndim < 1 || !X || ldx < ndim || !mom) { set_error("hmc_comoments: bad arguments"); return LINNA_ERR_INVALID; }
    TRY(hmc_dense_check(ndim, nullptr, "hmc_comoments"));
    return launch_hmc_comoments(B, ndim, X, ldx, mom, S(stream));
} LINNA_CATCH_INT
int linna_hmc_chol_from_comoments(linna_ctx_t*, int ndim, double* mom, float* Cm, int ldc, int* info, int reset, void* stream) try {
    if (ndim < 1 || !mom || !Cm || ldc < ndim || !info) { set_error("hmc_chol_from_comoments: bad arguments"); return LINNA_ERR_INVALID; }
    TRY(hmc_dense_check(ndim, nullptr, "hmc_chol_from_comoments"));
    hipLaunchKernelGGL(hmc_chol_from_comoments_kernel, dim3(1), dim3(CHOL_THREADS), 0, S(stream), ndim, mom, Cm, ldc, info, reset);
    LAUNCH_CHECK("hmc_chol_from_comoments");
} LINNA_CATCH_INT
int linna_hmc_kick_drift_dense(linna_ctx_t*, int B, int ndim, const float* Cm, int ldc, const float* EPS, float mul_kick, float mul_drift,
                               const float* G, int ldg, float* W, int ldw, const float* X, int ldx, float* Q, int ldq, void* stream) try {
    if (B < 1 || ndim < 1 || !Cm || ldc < ndim || !G || ldg < ndim || !W || ldw < ndim || !Q || ldq < ndim || (X && ldx < ndim)) {
        set_error("hmc_kick_drift_dense: bad arguments"); return LINNA_ERR_INVALID;
    }
    TRY(hmc_dense_check(ndim, nullptr, "hmc_kick_drift_dense"));
    return launch_hmc_kick_drift_dense(B, ndim, Cm, ldc, EPS, mul_kick, mul_drift, G, ldg, W, ldw, X, ldx, Q, ldq, S(stream));
} LINNA_CATCH_INT
size_t linna_hmc_chees_doubles(int ndim) try {
    if (ndim < 1) return 0;
    return LINNA_HMC_CHEES_HEAD + 2 * (size_t)ndim;
} LINNA_CATCH_SIZE
int linna_hmc_chees_begin(linna_ctx_t*, int B, int ndim, const float* X, int ldx, double* state, double* r0, void* stream) try {
    if (B < 1 || ndim < 1 || !X || ldx < ndim || !state || !r0) { set_error("hmc_chees_begin: bad arguments"); return LINNA_ERR_INVALID; }
    hipLaunchKernelGGL(hmc_chees_begin_kernel, dim3(1), dim3(MOM_WAVES * 64), 0, S(stream), B, ndim, X, ldx, state, r0);
    LAUNCH_CHECK("hmc_chees_begin");
} LINNA_CATCH_INT
int linna_hmc_chees_end(linna_ctx_t*, int B, int ndim, const float* mass, const float* Cm, int ldc, const float* Q, int ldq,
                        const float* P, int ldp, const float* alpha, const double* r0, double* state, float* EPS, int M, double delta,
                        int max_steps, void* stream) try {
    if (B < 1 || ndim < 1 || (!mass && !Cm) || (Cm && ldc < ndim) || !Q || ldq < ndim || !P || ldp < ndim || !alpha || !r0 || !state ||
        !EPS || max_steps < 1 || !(delta > 0.0 && delta < 1.0)) {
        set_error("hmc_chees_end: bad arguments"); return LINNA_ERR_INVALID;
    }
    if (Cm) TRY(hmc_dense_check(ndim, nullptr, "hmc_chees_end"));
    hipStream_t s = S(stream);
    if (Cm) hipLaunchKernelGGL(hmc_chees_end_kernel<true>, dim3(1), dim3(MOM_WAVES * 64), 0, s, B, ndim, mass, Cm, ldc, Q, ldq, P, ldp,
                               alpha, r0, state, EPS, M, delta, max_steps);
    else hipLaunchKernelGGL(hmc_chees_end_kernel<false>, dim3(1), dim3(MOM_WAVES * 64), 0, s, B, ndim, mass, Cm, ldc, Q, ldq, P, ldp,
                            alpha, r0, state, EPS, M, delta, max_steps);
    LAUNCH_CHECK("hmc_chees_end");
} LINNA_CATCH_INT
int linna_hmc_start_eps(linna_ctx_t*, int B, int ndim, const float* mass, uint64_t seed, const int* step_dev, int step_offset,
                        const float* lnp, const float* P0, int ldp0, const float* G, int ldg, const float* EPS, float mul_kick,
                        float mul_drift, const float* X, int ldx, float* P, int ldp, float* Q, int ldq, float* H0, void* stream) try {
    if (B < 1 || ndim < 1 || !mass || !step_dev || !lnp || !G || !EPS || !X || !P || !Q || !H0) { set_error("hmc_start_eps: bad arguments"); return LINNA_ERR_INVALID; }
    return launch_hmc_start(B, ndim, mass, seed, step_dev, lnp, P0, ldp0, G, ldg, mul_kick, mul_drift, X, ldx, P, ldp, Q, ldq, H0, S(stream),
                            EPS, step_offset);
} LINNA_CATCH_INT
int linna_hmc_kick_drift_eps(linna_ctx_t*, int B, int ndim, const float* mass, const float* EPS, float mul_kick, float mul_drift,
                             const float* G, int ldg, float* P, int ldp, float* Q, int ldq, void* stream) try {
    if (B < 1 || ndim < 1 || !mass || !EPS || !G || !P || !Q) { set_error("hmc_kick_drift_eps: bad arguments"); return LINNA_ERR_INVALID; }
    return launch_hmc_kick_drift(B, ndim, mass, mul_kick, mul_drift, G, ldg, P, ldp, Q, ldq, S(stream), EPS);
} LINNA_CATCH_INT
int linna_hmc_accept_adapt(linna_ctx_t*, int B, int ndim, const float* mass, uint64_t seed, const int* step_dev, int step_offset,
                           const float* H0, const float* P, int ldp, const float* Qn, int ldq, const float* lnp_new, const float* Gn,
                           int ldg, const float* U, float* X, int ldx, float* lnp, float* G, int* naccept, float* alpha, float* EPS,
                           float* EPSBAR, float* HBAR, const float* MU, int* M, int Madapt, float delta, float* chain, float* logps,
                           void* stream) try {
    if (B < 1 || ndim < 1 || !mass || !step_dev || !H0 || !P || !Qn || !lnp_new || !Gn || !X || !lnp || !G || Madapt < 0 ||
        (Madapt > 0 && (!EPS || !EPSBAR || !HBAR || !MU || !M))) {
        set_error("hmc_accept_adapt: bad arguments"); return LINNA_ERR_INVALID;
    }
    const HmcAdapt ad{EPS, EPSBAR, HBAR, MU, M, Madapt, delta};
    return launch_hmc_accept(B, ndim, mass, seed, step_dev, step_offset, H0, P, ldp, Qn, ldq, lnp_new, Gn, ldg, U, X, ldx, lnp, G,
                             naccept, alpha, ad, chain, logps, HmcEnergy{}, S(stream));
} LINNA_CATCH_INT
size_t linna_hmc_energy_doubles(int B) try {
    if (B < 1) return 0;
    return (size_t)LINNA_HMC_ENERGY_DOUBLES * (size_t)B;
} LINNA_CATCH_SIZE
int linna_hmc_accept_energy(linna_ctx_t*, int B, int ndim, const float* mass, uint64_t seed, const int* step_dev, int step_offset,
                            const float* H0, const float* P, int ldp, const float* Qn, int ldq, const float* lnp_new, const float* Gn,
                            int ldg, const float* U, float* X, int ldx, float* lnp, float* G, int* naccept, float* alpha, float* EPS,
                            float* EPSBAR, float* HBAR, const float* MU, int* M, int Madapt, float delta, float* chain, float* logps,
                            double* estate, int* ndiv, float max_dH, float* energy, float* dH, void* stream) try {
    if (B < 1 || ndim < 1 || !mass || !step_dev || !H0 || !P || !Qn || !lnp_new || !Gn || !X || !lnp || !G || Madapt < 0 ||
        (Madapt > 0 && (!EPS || !EPSBAR || !HBAR || !MU || !M))) {
        set_error("hmc_accept_energy: bad arguments"); return LINNA_ERR_INVALID;
    }
    const HmcEnergy en{estate, ndiv, max_dH, energy, dH};
    TRY(hmc_energy_check(en, "hmc_accept_energy"));
    const HmcAdapt ad{EPS, EPSBAR, HBAR, MU, M, Madapt, delta};
    return launch_hmc_accept(B, ndim, mass, seed, step_dev, step_offset, H0, P, ldp, Qn, ldq, lnp_new, Gn, ldg, U, X, ldx, lnp, G,
                             naccept, alpha, ad, chain, logps, en, S(stream));
} LINNA_CATCH_INT
int linna_hmc_energy_finish(linna_ctx_t*, int B, const double* estate, const int* ndiv, float* bfmi, double* pooled, void* stream) try {
    if (B < 1 || !estate || !ndiv || !bfmi || !pooled) { set_error("hmc_energy_finish: bad arguments"); return LINNA_ERR_INVALID; }
    hipLaunchKernelGGL(hmc_energy_finish_kernel, dim3(1), dim3(ENERGY_WAVES * 64), 0, S(stream), B, estate, ndiv, bfmi, pooled);
    LAUNCH_CHECK("hmc_energy_finish");
} LINNA_CATCH_INT
int linna_hmc_accept(linna_ctx_t*, int B, int ndim, const float* mass, uint64_t seed, const int* step_dev, const float* H0,
                     const float* P, int ldp, const float* Qn, int ldq, const float* lnp_new, const float* Gn, int ldg,
                     const float* U, float* X, int ldx, float* lnp, float* G, int* naccept, void* stream) try {
    // the Metropolis test alone: no acceptance rate, no chain row, no adaptation state
    return launch_hmc_accept(B, ndim, mass, seed, step_dev, 0, H0, P, ldp, Qn, ldq, lnp_new, Gn, ldg, U, X, ldx, lnp, G, naccept, nullptr,
                             HmcAdapt{}, nullptr, nullptr, HmcEnergy{}, S(stream));
} LINNA_CATCH_INT
