// Rank-normalised, folded split-R-hat (Vehtari, Gelman, Simpson, Carpenter, Buerkner 2021) of a walker chain on gfx950;
// include/linna_hip.h states the definition.  Plain split-R-hat (autocorr.hip) compares the means of the split chains with
// their pooled variance: chains that agree in location but not in scale pass it.  Here every value of a parameter is
// replaced by the normal score of its rank in the pooled set of all split chains (bulk), and then the same is done with the
// absolute deviations from the pooled median (folded: a chain that is too narrow or too wide has ranks that are too small
// or too large).  That needs a sort of the S = 2 n nw pooled values per parameter and check, which this file builds:
//
//   keys     an order-preserving 32-bit key per float32 (sign bit flipped for non-negatives, all bits for negatives, -0 = +0)
//            with the element index e = i nw + w (i: index among the 2 n pooled rows) as the payload;
//   sort     least-significant-digit radix sort, 8-bit digits, 4 passes, each pass three launches: digit counts per
//            workgroup tile, a scan of the counts, a STABLE scatter.  The in-workgroup rank of an element among the equal
//            digits in front of it comes from wavefront ballots (the lanes of a wavefront that hold the same digit) and
//            per-wavefront digit counts added in wave order; the only atomics are integer LDS adds of the count kernel,
//            whose sum does not depend on their order.  No workgroup waits for another inside a kernel;
//   ranks    every sorted position finds its run of equal keys by a lower-bound and an upper-bound binary search of the
//            sorted keys and writes rank2 = 2 x (average 1-based rank) = lb + ub + 1 to its element's index: ties (rejected
//            HMC transitions repeat rows bit for bit) cost what distinct keys cost;
//   moments  per split chain the sum and the sum of squares of z = Phi^-1((rank2 / 2 - 3/8) / (S + 1/4)) (AS 241 by hand),
//            taken relative to the chain's first z, rows dealt to 16 wavefronts and added in wave order; a finishing
//            wavefront per parameter turns the chains' means and variances into W, B / n, var+ and R-hat with wave_sum_f64.
//
// The parameters of a round share every launch (blockIdx.y): the launch count of a check does not grow with ndim while the
// caller's scratch holds them.  All element counts are < 2^31 (the entry refuses more); byte offsets are size_t.
// Bound: the scatter's uncoalesced writes (one (key, index) pair per element and pass): 54-58e9 keys per second and pass
// measured, the sort 54-57 % of a check, the binary searches 30 %.
//
// The file ends with that paper's rank-normalised bulk-ESS and tail-ESS: one sort of the same keys, a float32 image of the
// normal scores and of two quantile indicators written from the sorted order, and autocorr.hip's lagged products and Geyer
// finish on that image.
#include "common.h"
#include <math.h>

namespace linna {

constexpr int RK_THREADS = 256;                  // threads of a sort workgroup = radix (one digit per thread)
constexpr int RK_WAVES = RK_THREADS / 64;
constexpr int RK_CHUNKS = 16;                    // chunks of RK_THREADS elements a workgroup scatters in turn
constexpr int RK_TILE = RK_THREADS * RK_CHUNKS;  // elements per workgroup and pass
constexpr int RK_MW = 16;                        // wavefronts of the moments workgroup

__device__ __forceinline__ uint32_t rk_key(uint32_t bits) {
    if ((bits << 1) == 0u) bits = 0u;                                   // -0 = +0
    return (bits & 0x80000000u) ? ~bits : (bits | 0x80000000u);
}
__device__ __forceinline__ float rk_unkey(uint32_t key) {
    return __uint_as_float((key & 0x80000000u) ? (key ^ 0x80000000u) : ~key);
}

// element e of parameter d -> its value: e = i nw + w, pooled row i < n: chain row lo + i, else hi - 2 n + i
__device__ __forceinline__ float rk_value(const float* __restrict__ CT, size_t ns, int nwp, int nw, int d, int64_t lo, int64_t hi,
                                          int64_t n, uint32_t e) {
    const uint32_t i = e / (uint32_t)nw, w = e - i * (uint32_t)nw;
    const int64_t row = (int64_t)i < n ? lo + (int64_t)i : hi - 2 * n + (int64_t)i;
    return CT[(size_t)row * ns + (size_t)d * nwp + w];
}

// ------------------------------------------------------------------ keys
// FOLD = 0: keys of x, and the parameter's flag when a value is not finite.  FOLD = 1: keys of float32(|double(x) - med|).
template <int FOLD>
__global__ __launch_bounds__(RK_THREADS) void rank_keys_kernel(const float* __restrict__ CT, int nd, int nwp, int nw, int d0,
                                                               int64_t lo, int64_t hi, uint32_t S, const double* __restrict__ med,
                                                               uint32_t* __restrict__ K, uint32_t* __restrict__ I,
                                                               uint32_t* __restrict__ flag) {
    const uint32_t e = blockIdx.x * RK_THREADS + threadIdx.x;
    const int p = blockIdx.y;
    if (e >= S) return;
    const float x = rk_value(CT, (size_t)nd * nwp, nwp, nw, d0 + p, lo, hi, (hi - lo) / 2, e);
    uint32_t bits = __float_as_uint(x);
    if (FOLD) bits = __float_as_uint((float)fabs((double)x - med[p]));
    else if ((bits & 0x7f800000u) == 0x7f800000u) flag[p] = 1u;         // (every writer stores the same word)
    K[(size_t)p * S + e] = rk_key(bits);
    I[(size_t)p * S + e] = e;
}

// ------------------------------------------------------------------ radix pass
// counts C[p][tile][256] of the digit (key >> shift) & 255 over the tile's elements
__global__ __launch_bounds__(RK_THREADS) void rank_count_kernel(const uint32_t* __restrict__ K, uint32_t S, int shift, uint32_t ntiles,
                                                                uint32_t* __restrict__ C) {
    __shared__ uint32_t hist[RK_THREADS];
    const int p = blockIdx.y;
    const uint32_t* k = K + (size_t)p * S;
    hist[threadIdx.x] = 0u;
    __syncthreads();
    const uint32_t base = blockIdx.x * (uint32_t)RK_TILE;
#pragma unroll 4
    for (int c = 0; c < RK_CHUNKS; ++c) {
        const uint32_t i = base + c * RK_THREADS + threadIdx.x;
        if (i < S) atomicAdd(&hist[(k[i] >> shift) & 255u], 1u);
    }
    __syncthreads();
    C[((size_t)p * ntiles + blockIdx.x) * RK_THREADS + threadIdx.x] = hist[threadIdx.x];
}

// in place: counts -> the first output position of (digit, tile): every smaller digit's total, then the tiles in front.
// One workgroup per parameter, thread = digit; rows of 256 counts are read and written coalesced.
__global__ __launch_bounds__(RK_THREADS) void rank_scan_kernel(uint32_t ntiles, uint32_t* __restrict__ C) {
    __shared__ uint32_t tot[RK_THREADS];
    uint32_t* c = C + (size_t)blockIdx.x * ntiles * RK_THREADS + threadIdx.x;
    uint32_t sum = 0u;
#pragma unroll 4
    for (uint32_t t = 0; t < ntiles; ++t) sum += c[(size_t)t * RK_THREADS];
    tot[threadIdx.x] = sum;
    __syncthreads();
    uint32_t run = 0u;
    for (int j = 0; j < (int)threadIdx.x; ++j) run += tot[j];
#pragma unroll 4
    for (uint32_t t = 0; t < ntiles; ++t) {
        const uint32_t v = c[(size_t)t * RK_THREADS];
        c[(size_t)t * RK_THREADS] = run;
        run += v;
    }
}

// stable scatter of the tile's (key, index) pairs.  Per chunk of 256 elements: the lanes of a wavefront holding the same digit
// find each other by 8 ballots; an element's place is the digit's running position + the counts of the wavefronts in front
// + the number of lower lanes with that digit.
__global__ __launch_bounds__(RK_THREADS) void rank_scatter_kernel(const uint32_t* __restrict__ Kin, const uint32_t* __restrict__ Iin,
                                                                  uint32_t S, int shift, uint32_t ntiles, const uint32_t* __restrict__ C,
                                                                  uint32_t* __restrict__ Kout, uint32_t* __restrict__ Iout) {
    __shared__ uint32_t pos[RK_THREADS];
    __shared__ uint32_t wcount[RK_WAVES][RK_THREADS];
    const int p = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const size_t off = (size_t)p * S;
    pos[tid] = C[((size_t)p * ntiles + blockIdx.x) * RK_THREADS + tid];
#pragma unroll
    for (int q = 0; q < RK_WAVES; ++q) wcount[q][tid] = 0u;
    __syncthreads();
    const uint32_t base = blockIdx.x * (uint32_t)RK_TILE;
    const unsigned long long below = (1ull << lane) - 1ull;
    for (int c = 0; c < RK_CHUNKS; ++c) {
        const uint32_t i = base + c * RK_THREADS + tid;
        if (base + c * RK_THREADS >= S) break;                          // (uniform over the workgroup)
        const bool valid = i < S;
        const uint32_t key = valid ? Kin[off + i] : 0xffffffffu;
        const uint32_t idx = valid ? Iin[off + i] : 0u;
        const uint32_t digit = (key >> shift) & 255u;
        unsigned long long same = __ballot(valid);
#pragma unroll
        for (int b = 0; b < 8; ++b) {
            const bool bit = (digit >> b) & 1u;
            const unsigned long long bal = __ballot(bit);
            same &= bit ? bal : ~bal;
        }
        const uint32_t before = (uint32_t)__popcll(same & below);
        if (valid && before == 0u) wcount[wave][digit] = (uint32_t)__popcll(same);
        __syncthreads();
        if (valid) {
            uint32_t o = pos[digit] + before;
            for (int q = 0; q < wave; ++q) o += wcount[q][digit];
            if (o < S) { Kout[off + o] = key; Iout[off + o] = idx; }    // (o < S always; the guard keeps a wrong count table in bounds)
        }
        __syncthreads();
        uint32_t add = 0u;
#pragma unroll
        for (int q = 0; q < RK_WAVES; ++q) { add += wcount[q][tid]; wcount[q][tid] = 0u; }
        pos[tid] += add;
        __syncthreads();
    }
}

// ------------------------------------------------------------------ ranks of ties, median
// sorted position j: run of equal keys [lb, ub) -> rank2 = lb + ub + 1 at the element's index, and in rank2_out (tests).
// MED: position 0 writes the median of the pooled set, the float64 mean of the two middle sorted values.
template <int MED>
__global__ __launch_bounds__(RK_THREADS) void rank_ties_kernel(const uint32_t* __restrict__ K, const uint32_t* __restrict__ I, uint32_t S,
                                                               int nw, int nwp, uint32_t* __restrict__ R2, uint32_t* __restrict__ r2out,
                                                               size_t r2stride, double* __restrict__ med) {
    const uint32_t j = blockIdx.x * RK_THREADS + threadIdx.x;
    const int p = blockIdx.y;
    if (j >= S) return;
    const uint32_t* k = K + (size_t)p * S;
    const uint32_t key = k[j];
    uint32_t a = 0u, b = j;                                             // lower bound in [0, j]
    while (a < b) { const uint32_t m = a + ((b - a) >> 1); if (k[m] < key) a = m + 1u; else b = m; }
    const uint32_t lb = a;
    a = j + 1u; b = S;                                                  // upper bound in [j + 1, S]
    while (a < b) { const uint32_t m = a + ((b - a) >> 1); if (k[m] <= key) a = m + 1u; else b = m; }
    const uint32_t r2 = lb + a + 1u;
    const uint32_t e = I[(size_t)p * S + j];
    if (e < S) {
        R2[(size_t)p * S + e] = r2;
        if (r2out) { const uint32_t i = e / (uint32_t)nw, w = e - i * (uint32_t)nw; r2out[(size_t)p * r2stride + (size_t)i * nwp + w] = r2; }
    }
    if (MED && j == 0u) med[p] = 0.5 * ((double)rk_unkey(k[S / 2u - 1u]) + (double)rk_unkey(k[S / 2u]));
}

// ------------------------------------------------------------------ moments of the normal scores
// Phi^-1 in float64: Wichura's algorithm AS 241 (Applied Statistics 37, 1988), routine PPND16, relative error about 1e-16.
// Written out by hand: the device library's normcdfinv needs 1.1 KB of private memory per lane in this kernel.
__device__ __forceinline__ double rk_poly8(double r, double c0, double c1, double c2, double c3, double c4, double c5, double c6,
                                           double c7) {
    return (((((((c7 * r + c6) * r + c5) * r + c4) * r + c3) * r + c2) * r + c1) * r + c0);
}
__device__ double rk_ndtri(double p) {
    const double q = p - 0.5;
    if (fabs(q) <= 0.425) {
        const double r = 0.180625 - q * q;
        return q * rk_poly8(r, 3.3871328727963666080e0, 1.3314166789178437745e+2, 1.9715909503065514427e+3, 1.3731693765509461125e+4,
                            4.5921953931549871457e+4, 6.7265770927008700853e+4, 3.3430575583588128105e+4, 2.5090809287301226727e+3) /
               rk_poly8(r, 1.0, 4.2313330701600911252e+1, 6.8718700749205790830e+2, 5.3941960214247511077e+3, 2.1213794301586595867e+4,
                        3.9307895800092710610e+4, 2.8729085735721942674e+4, 5.2264952788528545610e+3);
    }
    double r = sqrt(-log(q < 0.0 ? p : 1.0 - p));
    double v;
    if (r <= 5.0) {
        r -= 1.6;
        v = rk_poly8(r, 1.42343711074968357734e0, 4.63033784615654529590e0, 5.76949722146069140550e0, 3.64784832476320460504e0,
                     1.27045825245236838258e0, 2.41780725177450611770e-1, 2.27238449892691845833e-2, 7.74545014278341407640e-4) /
            rk_poly8(r, 1.0, 2.05319162663775882187e0, 1.67638483018380384940e0, 6.89767334985100004550e-1, 1.48103976427480074590e-1,
                     1.51986665636164571966e-2, 5.47593808499534494600e-4, 1.05075007164441684324e-9);
    } else {
        r -= 5.0;
        v = rk_poly8(r, 6.65790464350110377720e0, 5.46378491116411436990e0, 1.78482653991729133580e0, 2.96560571828504891230e-1,
                     2.65321895265761230930e-2, 1.24266094738807843860e-3, 2.71155556874348757815e-5, 2.01033439929228813265e-7) /
            rk_poly8(r, 1.0, 5.99832206555887937690e-1, 1.36929880922735805310e-1, 1.48753612908506148525e-2, 7.86869131145613259100e-4,
                     1.84631831751005468180e-5, 1.42151175831644588870e-7, 2.04426310338993978564e-15);
    }
    return q < 0.0 ? -v : v;
}

// M[p][2 w + h][2] = mean and variance (ddof 1) of z over split chain h of walker w.  Wave q takes the rows q, q + 16, ...
__global__ __launch_bounds__(64 * RK_MW) void rank_moments_kernel(const uint32_t* __restrict__ R2, uint32_t S, int nw, int64_t n,
                                                                  double* __restrict__ M) {
    __shared__ double part[RK_MW][2][64];
    const int lane = threadIdx.x & 63, q = threadIdx.x >> 6, h = blockIdx.y, p = blockIdx.z;
    const int w = blockIdx.x * 64 + lane;
    const bool live = w < nw;
    const uint32_t* r2 = R2 + (size_t)p * S + (size_t)h * (size_t)n * nw + (live ? w : 0);
    const double den = (double)S + 0.25;
    auto zof = [&](uint32_t r) { return rk_ndtri((0.5 * (double)r - 0.375) / den); };
    const double z0 = zof(r2[0]);
    double s1 = 0.0, s2 = 0.0;
    for (int64_t r = q; r < n; r += RK_MW) {
        const double v = zof(r2[(size_t)r * nw]) - z0;
        s1 += v; s2 = __builtin_fma(v, v, s2);
    }
    part[q][0][lane] = s1; part[q][1][lane] = s2;
    __syncthreads();
    if (q == 0 && live) {
        s1 = 0.0; s2 = 0.0;
        for (int j = 0; j < RK_MW; ++j) { s1 += part[j][0][lane]; s2 += part[j][1][lane]; }
        const double mrel = s1 / (double)n;
        double* m = M + ((size_t)p * 2 * nw + 2 * (size_t)w + h) * 2;
        m[0] = z0 + mrel;
        m[1] = (s2 - s1 * mrel) / (double)(n - 1);
    }
}

// one wavefront per parameter: W, B / n, var+, R-hat from the split chains' means and variances.  STAT 0: bulk -> out[d][1].
// STAT 1: folded -> out[d][2], and out[d][0] = max(bulk, folded) (NaN if either is), out[d][3] = the median.
template <int STAT>
__global__ __launch_bounds__(64) void rank_finish_kernel(const double* __restrict__ M, int nw, int64_t n, const uint32_t* __restrict__ flag,
                                                         const double* __restrict__ med, int d0, double* __restrict__ out) {
    const int lane = threadIdx.x, p = blockIdx.x;
    const double* m = M + (size_t)p * 2 * nw * 2;
    double am = 0.0, am2 = 0.0, av = 0.0;
    for (int c = lane; c < 2 * nw; c += 64) {
        const double mean = m[2 * (size_t)c], var = m[2 * (size_t)c + 1];
        am += mean; am2 = __builtin_fma(mean, mean, am2); av += var;
    }
    am = wave_sum_f64(am); am2 = wave_sum_f64(am2); av = wave_sum_f64(av);
    if (lane != 0) return;
    const double nc = 2.0 * (double)nw;
    const double W = av / nc;
    const double Bn = (am2 - am * am / nc) / (nc - 1.0);
    const double vp = (double)(n - 1) / (double)n * W + Bn;
    const bool ok = flag[p] == 0u && W > 0.0 && isfinite(W) && isfinite(vp);
    const double r = ok ? sqrt(vp / W) : NAN;
    double* o = out + 4 * (size_t)(d0 + p);
    if (STAT == 0) { o[1] = r; return; }
    const double bulk = o[1];
    o[2] = r;
    o[0] = (bulk != bulk || r != r) ? NAN : (bulk > r ? bulk : r);
    o[3] = med[p];
}

// ------------------------------------------------------------------ launcher
// scratch of a round of npar parameters: doubles first (chain moments, medians), then the 32-bit words
struct RankLayout {
    size_t moments, med, flag, keys, counts, per;       // byte offsets for npar parameters; per: bytes per parameter
    uint32_t ntiles;
};
static RankLayout rank_layout(int nw, int64_t rows, int npar) {
    const size_t S = (size_t)rows * nw;
    RankLayout L;
    L.ntiles = (uint32_t)((S + RK_TILE - 1) / RK_TILE);
    const size_t bm = (size_t)2 * nw * 2 * sizeof(double), bmed = sizeof(double), bflag = 8;
    const size_t bkeys = 4 * S * sizeof(uint32_t), bcounts = (size_t)L.ntiles * RK_THREADS * sizeof(uint32_t);
    L.per = bm + bmed + bflag + bkeys + bcounts;
    L.moments = 0;
    L.med = L.moments + bm * npar;
    L.flag = L.med + bmed * npar;
    L.keys = L.flag + bflag * npar;
    L.counts = L.keys + bkeys * npar;
    return L;
}
static size_t chain_rank_rhat_scratch_bytes(int nw, int64_t rows, int npar) { return rank_layout(nw, rows, npar).per * (size_t)npar; }

static void rank_sort(uint32_t* KA, uint32_t* IA, uint32_t* KB, uint32_t* IB, uint32_t* C, uint32_t S, uint32_t ntiles, int npar,
                      hipStream_t s) {
    for (int pass = 0; pass < 4; ++pass) {
        const int shift = 8 * pass;
        hipLaunchKernelGGL(rank_count_kernel, dim3(ntiles, npar), dim3(RK_THREADS), 0, s, KA, S, shift, ntiles, C);
        hipLaunchKernelGGL(rank_scan_kernel, dim3(npar), dim3(RK_THREADS), 0, s, ntiles, C);
        hipLaunchKernelGGL(rank_scatter_kernel, dim3(ntiles, npar), dim3(RK_THREADS), 0, s, KA, IA, S, shift, ntiles, C, KB, IB);
        uint32_t* t = KA; KA = KB; KB = t;
        t = IA; IA = IB; IB = t;
    }                                                                   // (4 passes: the sorted pairs are back in KA, IA)
}

static int launch_chain_rank_rhat(const float* CT, int ndim, int nwp, int nw, int64_t lo, int64_t hi, void* scratch, size_t scratch_bytes,
                                  uint32_t* rank2_out, double* out, hipStream_t s) {
    const int64_t n = (hi - lo) / 2;
    const uint32_t S = (uint32_t)(2 * n * nw);
    const size_t per = rank_layout(nw, 2 * n, 1).per;
    int npar = (int)(scratch_bytes / per < (size_t)ndim ? scratch_bytes / per : (size_t)ndim);
    if (npar > 65535) npar = 65535;
    const RankLayout L = rank_layout(nw, 2 * n, npar);
    char* base = (char*)scratch;
    double* M = (double*)(base + L.moments);
    double* med = (double*)(base + L.med);
    uint32_t* flag = (uint32_t*)(base + L.flag);
    uint32_t* KA = (uint32_t*)(base + L.keys);
    uint32_t* IA = KA + (size_t)npar * S;
    uint32_t* KB = IA + (size_t)npar * S;
    uint32_t* IB = KB + (size_t)npar * S;
    uint32_t* C = (uint32_t*)(base + L.counts);
    const size_t r2stride = (size_t)2 * n * nwp;                        // words of one parameter in rank2_out
    if (rank2_out) {
        int rc = check_hip(hipMemsetAsync(rank2_out, 0, 2 * (size_t)ndim * r2stride * sizeof(uint32_t), s), "chain_rank_rhat");
        if (rc) return rc;
    }
    const uint32_t eblocks = (S + RK_THREADS - 1) / RK_THREADS;
    for (int d0 = 0; d0 < ndim; d0 += npar) {
        const int np = ndim - d0 < npar ? ndim - d0 : npar;
        int rc = check_hip(hipMemsetAsync(flag, 0, (size_t)np * 8, s), "chain_rank_rhat");
        if (rc) return rc;
        const dim3 eg(eblocks, np), mg((nw + 63) / 64, 2, np);
        uint32_t* r2a = rank2_out ? rank2_out + (size_t)d0 * r2stride : nullptr;
        uint32_t* r2b = rank2_out ? rank2_out + ((size_t)ndim + d0) * r2stride : nullptr;
        // with np < npar parameters the arrays keep the stride S per parameter: every kernel indexes p S
        hipLaunchKernelGGL((rank_keys_kernel<0>), eg, dim3(RK_THREADS), 0, s, CT, ndim, nwp, nw, d0, lo, hi, S, med, KA, IA, flag);
        rank_sort(KA, IA, KB, IB, C, S, L.ntiles, np, s);
        hipLaunchKernelGGL((rank_ties_kernel<1>), eg, dim3(RK_THREADS), 0, s, KA, IA, S, nw, nwp, KB, r2a, r2stride, med);
        hipLaunchKernelGGL(rank_moments_kernel, mg, dim3(64 * RK_MW), 0, s, KB, S, nw, n, M);
        hipLaunchKernelGGL((rank_finish_kernel<0>), dim3(np), dim3(64), 0, s, M, nw, n, flag, med, d0, out);
        hipLaunchKernelGGL((rank_keys_kernel<1>), eg, dim3(RK_THREADS), 0, s, CT, ndim, nwp, nw, d0, lo, hi, S, med, KA, IA, flag);
        rank_sort(KA, IA, KB, IB, C, S, L.ntiles, np, s);
        hipLaunchKernelGGL((rank_ties_kernel<0>), eg, dim3(RK_THREADS), 0, s, KA, IA, S, nw, nwp, KB, r2b, r2stride, med);
        hipLaunchKernelGGL(rank_moments_kernel, mg, dim3(64 * RK_MW), 0, s, KB, S, nw, n, M);
        hipLaunchKernelGGL((rank_finish_kernel<1>), dim3(np), dim3(64), 0, s, M, nw, n, flag, med, d0, out);
    }
    return check_hip(hipGetLastError(), "chain_rank_rhat");
}

// ------------------------------------------------------------------ rank-normalised bulk-ESS and tail-ESS
// include/linna_hip.h states the definition.  One sort (the bulk order) per parameter; then the SCORES IMAGE, a chain of its
// own in the layout of autocorr.hip: rows 0 .. n - 1, per parameter three series (float32 normal score, indicator of the 5 %
// quantile, indicator of the 95 % quantile), the C = 2 nw split chains as lanes (first halves, then second halves) padded
// with zeros to a multiple of 64.  The image's lagged products and their Geyer finish are autocorr.hip's, unchanged.
//
// sorted position j: run of equal keys [lb, ub) -> z = float32(Phi^-1((rank2 / 2 - 3/8) / (S + 1/4))) and the two indicators of
// the value (the key's float32) to the element's row and lane of the image.  The quantiles are read from the sorted keys by
// integer position: every thread forms both (uniform loads).
__global__ __launch_bounds__(RK_THREADS) void rank_scores_kernel(const uint32_t* __restrict__ K, const uint32_t* __restrict__ I, uint32_t S,
                                                                 int nw, int64_t n, int np, int cp, float* __restrict__ img) {
    const uint32_t j = blockIdx.x * RK_THREADS + threadIdx.x;
    const int p = blockIdx.y;
    if (j >= S) return;
    const uint32_t* k = K + (size_t)p * S;
    double qv[2];
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        const uint64_t pos = (uint64_t)(t ? 19 : 1) * (uint64_t)(S - 1u);
        const uint32_t jq = (uint32_t)(pos / 20u), j1 = jq + 1u < S ? jq + 1u : S - 1u;
        const double g = (double)(uint32_t)(pos - (uint64_t)jq * 20u) / 20.0;
        const double sj = (double)rk_unkey(k[jq]);
        qv[t] = sj + g * ((double)rk_unkey(k[j1]) - sj);
    }
    const uint32_t key = k[j];
    uint32_t a = 0u, b = j;                                             // lower bound in [0, j]
    while (a < b) { const uint32_t m = a + ((b - a) >> 1); if (k[m] < key) a = m + 1u; else b = m; }
    const uint32_t lb = a;
    a = j + 1u; b = S;                                                  // upper bound in [j + 1, S]
    while (a < b) { const uint32_t m = a + ((b - a) >> 1); if (k[m] <= key) a = m + 1u; else b = m; }
    const uint32_t r2 = lb + a + 1u;
    const uint32_t e = I[(size_t)p * S + j];
    if (e >= S) return;
    const uint32_t i = e / (uint32_t)nw, w = e - i * (uint32_t)nw;
    const bool second = (int64_t)i >= n;
    const size_t row = second ? (size_t)i - (size_t)n : (size_t)i;
    const int lane = (second ? nw : 0) + (int)w;
    const double x = (double)rk_unkey(key);
    float* o = img + (row * 3 * (size_t)np + 3 * (size_t)p) * cp + lane;
    o[0] = (float)rk_ndtri((0.5 * (double)r2 - 0.375) / ((double)S + 0.25));
    o[cp] = x <= qv[0] ? 1.f : 0.f;
    o[2 * (size_t)cp] = x <= qv[1] ? 1.f : 0.f;
}

// one thread per parameter: the three series' estimates G[3][3 np] (ESS | last pair | more lags needed) -> out[d][8]
__global__ __launch_bounds__(64) void rank_ess_finish_kernel(const double* __restrict__ G, const uint32_t* __restrict__ flag, int np, int d0,
                                                             double* __restrict__ out) {
    const int p = blockIdx.x * 64 + threadIdx.x;
    if (p >= np) return;
    const bool bad = flag[p] != 0u;
    double* o = out + 8 * (size_t)(d0 + p);
    double status = 0.0;
#pragma unroll
    for (int t = 0; t < 3; ++t) {
        const double e = bad ? NAN : G[3 * p + t];
        const bool nan = e != e;
        o[t == 0 ? 0 : 1 + t] = e;
        o[4 + t] = nan ? -1.0 : G[3 * np + 3 * p + t];
        if (!nan && G[6 * np + 3 * p + t] > 0.0) status = 1.0;
    }
    o[1] = (o[2] != o[2] || o[3] != o[3]) ? NAN : (o[2] < o[3] ? o[2] : o[3]);
    o[7] = status;
}

// scratch of a round of npar parameters: doubles first (lagged products, series sums, the estimator's scratch, the series'
// estimates), then the 32-bit words (flags, the sort's buffers, digit counts, the image)
struct RankEssLayout {
    size_t sums, tsum, est, g, flag, keys, counts, img, per;   // byte offsets for npar parameters; per: bytes per parameter
    uint32_t ntiles;
    int cp, k1;
};
static RankEssLayout rank_ess_layout(int nw, int64_t rows, int kuse, int npar) {
    const size_t S = (size_t)rows * nw, n = (size_t)rows / 2;
    RankEssLayout L;
    L.ntiles = (uint32_t)((S + RK_TILE - 1) / RK_TILE);
    L.cp = (2 * nw + 63) & ~63;
    L.k1 = (kuse + 32) & ~31;                                           // lags 0 .. kuse in whole blocks of 32
    const size_t bs = (size_t)L.k1 * 3 * L.cp * sizeof(double), bt = (size_t)3 * L.cp * sizeof(double);
    const size_t be = linna_acorr_ess_scratch_bytes(3, L.cp, kuse), bg = 9 * sizeof(double), bflag = 8;
    const size_t bkeys = 4 * S * sizeof(uint32_t), bcounts = (size_t)L.ntiles * RK_THREADS * sizeof(uint32_t);
    const size_t bimg = 3 * n * L.cp * sizeof(float);
    L.per = bs + bt + be + bg + bflag + bkeys + bcounts + bimg;
    L.sums = 0;
    L.tsum = L.sums + bs * npar;
    L.est = L.tsum + bt * npar;
    L.g = L.est + be * npar;
    L.flag = L.g + bg * npar;
    L.keys = L.flag + bflag * npar;
    L.counts = L.keys + bkeys * npar;
    L.img = L.counts + bcounts * npar;
    return L;
}
static size_t chain_rank_ess_scratch_bytes(int nw, int64_t rows, int kuse, int npar) {
    return rank_ess_layout(nw, rows, kuse, npar).per * (size_t)npar;
}

static int launch_chain_rank_ess(const float* CT, int ndim, int nwp, int nw, int64_t lo, int64_t hi, int kuse, void* scratch,
                                 size_t scratch_bytes, double* out, hipStream_t s) {
    const int64_t n = (hi - lo) / 2;
    const uint32_t S = (uint32_t)(2 * n * nw);
    const RankEssLayout one = rank_ess_layout(nw, 2 * n, kuse, 1);
    const size_t per = one.per;
    const int cp = one.cp;
    int npar = (int)(scratch_bytes / per < (size_t)ndim ? scratch_bytes / per : (size_t)ndim);
    if (npar > 21845) npar = 21845;                                     // (the 3 npar series are a grid dimension of the estimator)
    if (npar > 0x7fffffff / (3 * cp)) npar = 0x7fffffff / (3 * cp);     // (its series index is an int; nw <= 2^24: at least one)
    const RankEssLayout L = rank_ess_layout(nw, 2 * n, kuse, npar);
    char* base = (char*)scratch;
    double* Ssum = (double*)(base + L.sums);
    double* Tsum = (double*)(base + L.tsum);
    double* est = (double*)(base + L.est);
    double* G = (double*)(base + L.g);
    uint32_t* flag = (uint32_t*)(base + L.flag);
    uint32_t* KA = (uint32_t*)(base + L.keys);
    uint32_t* IA = KA + (size_t)npar * S;
    uint32_t* KB = IA + (size_t)npar * S;
    uint32_t* IB = KB + (size_t)npar * S;
    uint32_t* C = (uint32_t*)(base + L.counts);
    float* img = (float*)(base + L.img);
    const uint32_t eblocks = (S + RK_THREADS - 1) / RK_THREADS;
    for (int d0 = 0; d0 < ndim; d0 += npar) {
        const int np = ndim - d0 < npar ? ndim - d0 : npar;
        // the sort's arrays keep the stride S per parameter; the image, the sums and the estimates are packed for np parameters
        int rc = check_hip(hipMemsetAsync(flag, 0, (size_t)np * 8, s), "chain_rank_ess");
        if (rc) return rc;
        rc = check_hip(hipMemsetAsync(img, 0, (size_t)3 * np * n * L.cp * sizeof(float), s), "chain_rank_ess");
        if (rc) return rc;
        rc = check_hip(hipMemsetAsync(Ssum, 0, (size_t)L.k1 * 3 * np * L.cp * sizeof(double), s), "chain_rank_ess");
        if (rc) return rc;
        rc = check_hip(hipMemsetAsync(Tsum, 0, (size_t)3 * np * L.cp * sizeof(double), s), "chain_rank_ess");
        if (rc) return rc;
        const dim3 eg(eblocks, np);
        hipLaunchKernelGGL((rank_keys_kernel<0>), eg, dim3(RK_THREADS), 0, s, CT, ndim, nwp, nw, d0, lo, hi, S, (const double*)nullptr, KA, IA, flag);
        rank_sort(KA, IA, KB, IB, C, S, L.ntiles, np, s);
        hipLaunchKernelGGL(rank_scores_kernel, eg, dim3(RK_THREADS), 0, s, KA, IA, S, nw, n, np, L.cp, img);
        // the image is a chain like any other: its lagged products and their Geyer finish through autocorr.hip's own entries
        rc = linna_acorr_update(nullptr, img, 3 * np, L.cp, L.cp, 0, n, 0, n, 0, L.k1, Ssum, Tsum, 0, s);
        if (rc) return rc;
        rc = linna_acorr_ess(nullptr, img, 3 * np, L.cp, L.cp, 2 * nw, 0, n, kuse, Ssum, Tsum, est, G, s);
        if (rc) return rc;
        hipLaunchKernelGGL(rank_ess_finish_kernel, dim3((np + 63) / 64), dim3(64), 0, s, G, flag, np, d0, out);
    }
    return check_hip(hipGetLastError(), "chain_rank_ess");
}

}  // namespace linna

using namespace linna;

// ------------------------------------------------------------------ the entries (include/linna_hip.h)
size_t linna_chain_rank_rhat_scratch_bytes(int ndim, int nw, int64_t rows, int npar) try {
    if (ndim < 1 || nw < 1 || rows < 2 || (rows & 1) || npar < 1 || rows > 0x7fffffff / nw) return 0;
    return chain_rank_rhat_scratch_bytes(nw, rows, npar < ndim ? npar : ndim);
} LINNA_CATCH_SIZE
int linna_chain_rank_rhat(linna_ctx_t*, const float* CT, int ndim, int nwp, int nw, int64_t lo, int64_t hi, void* scratch,
                          size_t scratch_bytes, uint32_t* rank2_out, double* out, void* stream) try {
    if (!CT || !out || !scratch || ((uintptr_t)scratch & 7) || !ac_shape_ok(ndim, nwp) || nw < 1 || nw > nwp || lo < 0 || hi < lo ||
        (hi - lo) / 2 < 2 || hi > 0x7fffff00) {
        set_error("chain_rank_rhat: bad arguments (the window [lo, hi) needs two halves of at least 2 rows; scratch 8-byte aligned)");
        return LINNA_ERR_INVALID;
    }
    const int64_t rows = (hi - lo) / 2 * 2;
    if (rows > 0x7fffffff / nw) {
        set_error("chain_rank_rhat: %lld pooled values per parameter; the sort's 32-bit element indices hold fewer than 2^31",
                  (long long)rows * nw);
        return LINNA_ERR_UNSUPPORTED;
    }
    if (scratch_bytes < chain_rank_rhat_scratch_bytes(nw, rows, 1)) {
        set_error("chain_rank_rhat: scratch of %zu bytes, one parameter needs %zu (linna_chain_rank_rhat_scratch_bytes)", scratch_bytes,
                  chain_rank_rhat_scratch_bytes(nw, rows, 1));
        return LINNA_ERR_INVALID;
    }
    return launch_chain_rank_rhat(CT, ndim, nwp, nw, lo, hi, scratch, scratch_bytes, rank2_out, out, S(stream));
} LINNA_CATCH_INT
size_t linna_chain_rank_ess_scratch_bytes(int ndim, int nw, int64_t rows, int kuse, int npar) try {
    if (ndim < 1 || nw < 1 || rows < 4 || (rows & 1) || npar < 1 || rows > 0x7fffffff / nw || kuse < 1 || (int64_t)kuse > rows / 2 - 1 ||
        kuse / 32 + 1 > 65535 || nw > (1 << 24))
        return 0;
    return chain_rank_ess_scratch_bytes(nw, rows, kuse, npar < ndim ? npar : ndim);
} LINNA_CATCH_SIZE
int linna_chain_rank_ess(linna_ctx_t*, const float* CT, int ndim, int nwp, int nw, int64_t lo, int64_t hi, int kuse, void* scratch,
                         size_t scratch_bytes, double* out, void* stream) try {
    if (!CT || !out || !scratch || ((uintptr_t)scratch & 7) || !ac_shape_ok(ndim, nwp) || nw < 1 || nw > nwp || lo < 0 || hi < lo ||
        (hi - lo) / 2 < 2 || hi > 0x7fffff00 || kuse < 1 || (int64_t)kuse > (hi - lo) / 2 - 1 || kuse / 32 + 1 > 65535 || nw > (1 << 24)) {
        set_error("chain_rank_ess: bad arguments (the window [lo, hi) needs two halves of n >= 2 rows; 1 <= kuse <= n - 1; scratch "
                  "8-byte aligned)");
        return LINNA_ERR_INVALID;
    }
    const int64_t rows = (hi - lo) / 2 * 2;
    if (rows > 0x7fffffff / nw) {
        set_error("chain_rank_ess: %lld pooled values per parameter; the sort's 32-bit element indices hold fewer than 2^31",
                  (long long)rows * nw);
        return LINNA_ERR_UNSUPPORTED;
    }
    if (scratch_bytes < chain_rank_ess_scratch_bytes(nw, rows, kuse, 1)) {
        set_error("chain_rank_ess: scratch of %zu bytes, one parameter needs %zu (linna_chain_rank_ess_scratch_bytes)", scratch_bytes,
                  chain_rank_ess_scratch_bytes(nw, rows, kuse, 1));
        return LINNA_ERR_INVALID;
    }
    return launch_chain_rank_ess(CT, ndim, nwp, nw, lo, hi, kuse, scratch, scratch_bytes, out, S(stream));
} LINNA_CATCH_INT
