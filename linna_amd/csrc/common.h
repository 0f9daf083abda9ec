// Internal declarations shared by the HIP translation units of liblinna_hip.so.
// gfx950 (MI355X / CDNA4) only: 64-lane wavefronts, fp32-input MFMA, 160 KiB LDS per CU.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <exception>
#include "../../include/linna_hip.h"


typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

namespace linna {

// ------------------------------------------------------------------ Philox4x32-10 (Salmon et al. 2011)
struct U4 { uint32_t x, y, z, w; };
__device__ __forceinline__ U4 philox4x32_10(U4 c, uint32_t k0, uint32_t k1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c.x;
        const uint64_t p1 = (uint64_t)0xCD9E8D57u * c.z;
        U4 n;
        n.x = (uint32_t)(p1 >> 32) ^ c.y ^ k0;
        n.y = (uint32_t)p1;
        n.z = (uint32_t)(p0 >> 32) ^ c.w ^ k1;
        n.w = (uint32_t)p0;
        c = n;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    return c;
}
__device__ __forceinline__ float u01(uint32_t b) { return ((float)(b >> 8) + 0.5f) * (1.0f / 16777216.0f); }

// draws for walker w at (step, stream): counter = (w, step, stream, sub), key = seed
__device__ __forceinline__ U4 walker_bits(uint64_t seed, uint32_t w, uint32_t step, uint32_t stream, uint32_t sub) {
    U4 c = {w, step, stream, sub};
    return philox4x32_10(c, (uint32_t)seed, (uint32_t)(seed >> 32));
}

// the float64 sum over a wave's 64 lanes, in every lane (a butterfly: one fixed order)
__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// ---- ensemble slice sampling: the rules of one half step, each written ONCE below with a WAVE per walker -- the set-up
// (slice_setup_wave), stepping out (slice_expand_wave), trial placement (slice_draw_wave), judging a round's trials
// (slice_judge_wave) and the commit (slice_commit_wave).  Every slice logic kernel of pointwise.hip is a thin wrapper of them:
// those of the round-by-round entries and those of linna_slice_half_step (pointwise.hip's comment block "one-call half step"
// has its procedure; slice_round_wave below is one of its shrinking rounds).  The ONLY other statements of these rules are the
// per-row forms in the prologue of the whole-network kernel (net_stream_body.inc, MOVE == 2), which forms its trial points
// itself: the set-up at lines 153-188 (row j ns + k forms its walker's direction and bracket end; the rows j = 0 also write
// them for the later launches) and, for the first shrinking round behind ONE stepping-out round, stepping out and trial
// placement at lines 190-215 (NsArgs::sl_*).  A change to a rule is made here and there.
// counters: [0] expansions, [1] contractions, [2] walkers left unfinished by the rounds of a call (sticky),
//           [3] evaluated points, [4 + r] walkers still active after round r (expand rounds first, then shrink rounds)
// What a set-up needs besides the walkers (S, ns, ndim) and, where a launch of its own does it, the first round's bracket ends
// W; `m`, `counters` (with nslots, zero_totals: the usage counters' roll) are used by linna_slice_half_step only.
struct SliceBegin {
    const float* logp; const float* cc; int ldcc; const int* C; int nc; const float* mu; uint64_t seed; const int* step; int half, m;
    float* DIR; int ldd; float* Z0; float* L; float* R; int* flags; int* counters; int nslots, zero_totals;
    int maxsteps;                                       // zeus' stepping-out budget (slice_budget)
};
// zeus' stepping-out budget (Neal 2003, Fig. 3; zeus ensemble.py: J = floor(maxsteps U), K = (maxsteps - 1) - J): at most J steps
// to the left and K to the right.  flags[3k] / flags[3k + 1] hold what is LEFT of them while that side is still stepping out and
// 0 once it is closed (an end below the slice, or the budget spent); flags[3k + 2]: still shrinking.
__device__ __forceinline__ void slice_budget(uint64_t seed, uint32_t wk, uint32_t step, uint32_t stream, int maxsteps, int& J, int& K) {
    const U4 b = walker_bits(seed, wk, step, stream, 1u);
    J = min((int)floorf((float)maxsteps * u01(b.x)), maxsteps - 1);       // (the fp32 product may round up to maxsteps itself)
    K = maxsteps - 1 - J;
}
// a side with `f` steps left saw `above` leading bracket ends over the slice among the m evaluated: steps taken; f becomes what is left
__device__ __forceinline__ int slice_side_steps(int& f, int above, int m) {
    const int n = min(above, f);
    f = (n == m && n < f) ? f - n : 0;
    return n;
}
struct SliceRound {
    const float* Z0; const float* Zt;                  // slice heights [ns]; lnP of this round's trials, [j ns + k]
    float* L; float* R; const int* S; float* W;        // brackets, the half ensemble's walkers, trial weights [j ns + k] (read; the next round's written)
    int* flags; float* Wacc; float* Zacc; int ns;
    int* counters; int slot, prev_slot, ntrial, nt_next, trials_so_far;
    int* list; uint64_t seed; int* step_dev; int stream_id;
    float* coords; int ldc, ndim; float* logp; const float* DIR; int ldd, bump;   // coords != null: the call's last round commits
    // m_derive > 0: this is the first shrinking round behind ONE stepping-out round of m_derive ends per side whose logic kernel
    // was not launched (the evaluation derived its trials itself, NsArgs::sl_*): its bookkeeping is done here first, from Ze
    const float* Ze; int m_derive, eslot;
};
// counters[i] += the sum over the block's waves of v (wave-uniform); every thread of the block calls
__device__ __forceinline__ void block_add_counter(int* __restrict__ counter, int v, int* lds_slot) {
    if (threadIdx.x == 0) *lds_slot = 0;
    __syncthreads();
    if ((threadIdx.x & 63) == 0 && v) atomicAdd(lds_slot, v);
    __syncthreads();
    if (threadIdx.x == 0 && *lds_slot) atomicAdd(counter, *lds_slot);
}
// ---- the rules, a WAVE per walker (all 64 lanes call with the same k, in wave-uniform control flow): the bracket ends / trials of
// a round are loaded, and the Philox draws of the next round made, one per lane; what is sequential in the procedure (a bracket
// shrinking trial by trial) is a short uniform loop over register values.  One thread per walker ran 16-32 dependent Philox
// draws and as many dependent loads: 5-10 us per logic kernel, a third of a 128-walker iteration.  A round therefore holds at
// most 32 bracket ends per side and 64 trials (the entries reject more).
__device__ __forceinline__ float wave_lane_f(float v, int j) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), j)); }
// the set-up of walker k: the differential move's direction between two DISTINCT complementary walkers, a uniform height under
// the density, a unit bracket placed uniformly around 0, the stepping-out budget into the flags; W (nullable): the b.m bracket
// ends per side the first stepping-out round evaluates, L - j and R + j
__device__ __forceinline__ void slice_setup_wave(const SliceBegin& b, const int* __restrict__ S, int ns, int ndim, float* __restrict__ W,
                                                 int k, int lane) {
    const int wk = S[k];
    const uint32_t step = (uint32_t)b.step[0];
    const U4 r = walker_bits(b.seed, (uint32_t)wk, step, (uint32_t)b.half, 0u);
    const int ia = (int)(((uint64_t)r.x * (uint64_t)b.nc) >> 32);
    int ib = (int)(((uint64_t)r.y * (uint64_t)(b.nc - 1)) >> 32);
    ib += (ib >= ia);
    const float* ca = b.cc + (size_t)b.C[ia] * b.ldcc;
    const float* cb = b.cc + (size_t)b.C[ib] * b.ldcc;
    const float mu = b.mu[0];
    for (int d = lane; d < b.ldd; d += 64) b.DIR[(size_t)k * b.ldd + d] = d < ndim ? mu * (ca[d] - cb[d]) : 0.f;
    const float l = -u01(r.w);
    if (lane == 0) {
        b.Z0[k] = b.logp[wk] + logf(u01(r.z));           // log of a uniform height under the density
        b.L[k] = l; b.R[k] = l + 1.f;
        int J, K;
        slice_budget(b.seed, (uint32_t)wk, step, (uint32_t)b.half, b.maxsteps, J, K);
        b.flags[3 * k] = J; b.flags[3 * k + 1] = K; b.flags[3 * k + 2] = 1;
    }
    if (W && lane < b.m) { W[(size_t)lane * ns + k] = l - (float)lane; W[(size_t)(b.m + lane) * ns + k] = l + 1.f + (float)lane; }
}
// trial placement: trial j + 1 of (round0 ...) placed as if its predecessors were rejected -- the bracket after a rejection depends
// on where the trial fell, not on its density; Philox sub-counter round0 + j + 1; lane j < cnt returns w_j
__device__ __forceinline__ float slice_draw_wave(int lane, int wk, float l, float r, uint64_t seed, uint32_t step, int stream_id,
                                                 int round0, int cnt) {
    const U4 b = walker_bits(seed, (uint32_t)wk, step, (uint32_t)stream_id, (uint32_t)(round0 + lane + 1));
    const float u = u01(b.x);
    float mine = 0.f;
    for (int j = 0; j < cnt; ++j) {
        const float w = l + wave_lane_f(u, j) * (r - l);
        if (lane == j) mine = w;
        if (w < 0.f) l = w; else r = w;
    }
    return mine;
}
// stepping out over the m <= 32 ends per side one round evaluated (ZL[j ns + k]: lnP at L - j, ZR[j ns + k]: at R + j): an end
// moves out by one unit while the density there is above the slice and its budget lasts.  Lanes 0..m-1 the left ends,
// 32..32+m-1 the right ones; l / r, fl / fr (and the flags in memory) updated, the steps taken added to nexp
__device__ __forceinline__ void slice_expand_wave(int lane, int k, int ns, int m, float z0, const float* __restrict__ ZL,
                                                  const float* __restrict__ ZR, float& l, float& r, int& fl, int& fr,
                                                  int* __restrict__ flags, int& nexp) {
    const int side = lane >> 5, j = lane & 31;
    const float ze = j < m ? (side ? ZR : ZL)[(size_t)j * ns + k] : 0.f;
    const unsigned long long bal = __ballot(j < m && ze > z0);
    const int fl0 = fl, fr0 = fr;
    const int nl = slice_side_steps(fl, __builtin_ctzll(~(unsigned long long)(uint32_t)bal), m);
    const int nr = slice_side_steps(fr, __builtin_ctzll(~(unsigned long long)(uint32_t)(bal >> 32)), m);
    for (int i = 0; i < nl; ++i) l -= 1.f;
    for (int i = 0; i < nr; ++i) r += 1.f;
    if (lane == 0 && fl != fl0) flags[3 * k] = fl;
    if (lane == 0 && fr != fr0) flags[3 * k + 1] = fr;
    nexp += nl + nr;
}
// judging a round's trials (lane j < ntrial holds trial j: its weight w and lnP zt): the bracket is pulled in to every trial
// before the first one inside the slice (counted in ncon).  Returns whether the walker is still shrinking; if not, wacc / zacc
// are the accepted weight and its lnP -- 0 and z0 where the bracket became degenerate (the walker stays put)
__device__ __forceinline__ bool slice_judge_wave(int lane, int ntrial, float z0, float w, float zt, float& l, float& r, int& ncon,
                                                 float& wacc, float& zacc) {
    const unsigned long long okm = __ballot(lane < ntrial && z0 < zt);       // zeus accepts iff Z0 < lnP(x'); NaN rejects
    const int ja = okm ? __builtin_ctzll(okm) : ntrial;                      // the first trial inside the slice
    for (int j = 0; j < ja; ++j) {
        const float wj = wave_lane_f(w, j);
        if (wj < 0.f) l = wj; else r = wj;
        ++ncon;
        if (r - l < 1e-30f) { wacc = 0.f; zacc = z0; return false; }
    }
    if (ja == ntrial) return true;
    wacc = wave_lane_f(w, ja); zacc = wave_lane_f(zt, ja);
    return false;
}
// the commit of walker k (= walker wk of the ensemble): x += Wacc DIR and its lnP; Wacc == 0 stays put.  `unfinished` (a caller
// with flags: one of the walker's is still set): the walker stays where it is and is counted in counters[2]
__device__ __forceinline__ void slice_commit_wave(int lane, int k, int wk, bool unfinished, int* __restrict__ counters, float wacc,
                                                  float zacc, float* __restrict__ coords, int ldc, int ndim, float* __restrict__ logp,
                                                  const float* __restrict__ DIR, int ldd) {
    if (unfinished) {
        if (lane == 0) atomicAdd(counters + 2, 1);
    } else if (wacc != 0.f) {
        for (int d = lane; d < ndim; d += 64) coords[(size_t)wk * ldc + d] += wacc * DIR[(size_t)k * ldd + d];
        if (lane == 0) logp[wk] = zacc;
    }
}
// one shrinking round of linna_slice_half_step for walker k.  nexp / ncon: this walker's expansions / contractions, which the
// caller adds to counters[0] / [1] (summed over the block first: one atomic per walker on one address cost 10-15 us of a
// 4096-walker round)
__device__ __forceinline__ void slice_round_wave(const SliceRound& a, int k, int lane, int& nexp, int& ncon) {
    const int ns = a.ns;
    if (k == 0 && lane == 0) {
        if (a.m_derive) atomicAdd(a.counters + 3, 2 * a.m_derive * ns);
        atomicAdd(a.counters + 3, a.ntrial * (a.prev_slot < 0 ? ns : a.counters[a.prev_slot]));      // the points this round evaluated
    }
    if (k >= ns) return;
    const uint32_t step = (uint32_t)a.step_dev[0];
    const int wk = a.S[k];
    const float z0 = a.Z0[k];
    int fl = a.flags[3 * k], fr = a.flags[3 * k + 1], fs = a.flags[3 * k + 2];
    float l = a.L[k], r = a.R[k];
    float w = 0.f;                                     // lane j: trial j of this round
    bool have_w = false;
    if (a.m_derive) {
        slice_expand_wave(lane, k, ns, a.m_derive, z0, a.Ze, a.Ze + (size_t)a.m_derive * ns, l, r, fl, fr, a.flags, nexp);
        if (lane == 0) { a.L[k] = l; a.R[k] = r; }
        if (fl | fr) {
            if (lane == 0) atomicAdd(a.counters + a.eslot, 1);
        } else {
            w = slice_draw_wave(lane, wk, l, r, a.seed, step, a.stream_id, 0, a.ntrial);   // the trials the evaluation derived
            if (lane < a.ntrial) a.W[(size_t)lane * ns + k] = w;
            have_w = true;
        }
    }
    const bool mine = fs && !(fl | fr) && !(a.prev_slot >= 0 && a.counters[a.prev_slot] == 0);   // not done, and its bracket closed
    float wacc = 0.f, zacc = 0.f;
    bool done_now = false;
    if (mine) {
        const bool in = lane < a.ntrial;
        const float zt = in ? a.Zt[(size_t)lane * ns + k] : 0.f;
        if (!have_w) w = in ? a.W[(size_t)lane * ns + k] : 0.f;
        const bool active = slice_judge_wave(lane, a.ntrial, z0, w, zt, l, r, ncon, wacc, zacc);
        if (lane == 0) { a.L[k] = l; a.R[k] = r; }
        if (active) {
            int pos = 0;
            if (lane == 0) pos = atomicAdd(a.counters + a.slot, 1);
            pos = __builtin_amdgcn_readfirstlane(pos);
            const float wn = slice_draw_wave(lane, wk, l, r, a.seed, step, a.stream_id, a.trials_so_far, a.nt_next);   // the next round's trials
            if (lane < a.nt_next) {
                a.W[(size_t)lane * ns + k] = wn;
                a.list[(size_t)pos * a.nt_next + lane] = lane * ns + k;
            }
        } else {
            done_now = true;
            fs = 0;
            if (lane == 0) { a.flags[3 * k + 2] = 0; a.Wacc[k] = wacc; a.Zacc[k] = zacc; }
        }
    }
    if (a.coords) {
        // the call's last round: the move of every finished walker (the last round draws no further trials: no thread of this
        // launch uses the step counter's value, whichever it reads, so `bump` may advance it here)
        if (!done_now) { wacc = a.Wacc[k]; zacc = a.Zacc[k]; }
        slice_commit_wave(lane, k, wk, (fl | fr | fs) != 0, a.counters, wacc, zacc, a.coords, a.ldc, a.ndim, a.logp, a.DIR, a.ldd);
        if (a.bump && k == 0 && lane == 0) a.step_dev[0] = (int)step + 1;
    }
}

void set_error(const char* fmt, ...);
int check_hip(hipError_t e, const char* what);
// The exception barrier of the C ABI (include/linna_hip.h: "No C++ exception crosses the boundary").  Every extern "C"
// entry is a function-try-block closed by one of these: the host side uses std::vector / std::string / std::unordered_map
// (program planning, descriptor tables), so bad_alloc / length_error can be thrown under an entry; it becomes a return
// code and a text in linna_last_error() instead of unwinding into ctypes (= std::terminate in the caller's process).
int caught_exception(const char* what) noexcept;      // sets the text, returns LINNA_ERR_INTERNAL (api.hip)
#define LINNA_CATCH_INT \
    catch (const std::exception& e_) { return ::linna::caught_exception(e_.what()); } \
    catch (...) { return ::linna::caught_exception(nullptr); }
#define LINNA_CATCH_SIZE \
    catch (const std::exception& e_) { (void)::linna::caught_exception(e_.what()); return 0; } \
    catch (...) { (void)::linna::caught_exception(nullptr); return 0; }
// What the files that hold extern "C" entries share (api.hip, comm.hip and a subsystem's own file -- hmc.hip, autocorr.hip,
// chain_rank.hip: its kernels, its launch code and its entries)
inline hipStream_t S(void* s) { return reinterpret_cast<hipStream_t>(s); }
inline dim3 grid1d(size_t n, int block) { return dim3((unsigned)((n + block - 1) / block)); }
#define TRY(expr) do { int rc__ = (expr); if (rc__ != LINNA_OK) return rc__; } while (0)
#define LAUNCH_CHECK(name) return check_hip(hipGetLastError(), name)
// a descriptor struct filled against another layout of include/linna_hip.h is refused, not read at wrong offsets
#define CHECK_STRUCT(ptr, T, who) do { if ((ptr)->struct_size != sizeof(T)) { \
        set_error("%s: " #T "::struct_size is %u, this library's sizeof is %zu -- set it to sizeof(" #T ") of the header you built against; " \
                  "a mismatch means that header is not this library's (LINNA_ABI_VERSION %d)", who, (unsigned)(ptr)->struct_size, sizeof(T), LINNA_ABI_VERSION); \
        return LINNA_ERR_INVALID; } } while (0)
// the (parameters, padded walkers) shape every chain-statistics entry demands of the transposed chain CT
inline bool ac_shape_ok(int ndim, int nwp) { return ndim >= 1 && nwp >= 64 && (nwp & 63) == 0; }

// Operand storage seen by the GEMM: LAY_K = contraction index contiguous
// (A as [M][K], B as [N][K]); LAY_MN = k-major (A as [K][M], B as [K][N]).
enum { LAY_K = 0, LAY_MN = 1 };

typedef linna_gemm_pair_t GemmPair;
typedef linna_gemm_t GemmArgs;   // the public descriptor is passed to the kernel by value

// pointwise.hip launchers
int launch_prior_map_fwd(const float* Z, int ldz, int B, int nin, const int* is_flat, const float* a1, const float* a2,
                         const int* lg, const float* xmean, const float* xstd, float* X, int ldx, float* TH, int ldt,
                         hipStream_t s);
int launch_prior_map_bwd(const float* Z, int ldz, int B, int nin, const int* is_flat, const float* a1, const float* a2,
                         const int* lg, const float* xstd, const float* dX, int lddx, float* dZ, int lddz, hipStream_t s);
int launch_loglike_diag(const float* D, int ldd, int B, int nout, const float* w, const float* Z, int ldz, int nin,
                        float T, float* out, hipStream_t s);
int launch_loglike_finish(const float* partial, int slots_ld, int nslots, int B, const float* Z, int ldz, int nin,
                          float T, float* out, hipStream_t s);
int launch_loglike_diag_grad(const float* D, int ldd, int B, int nout, const float* w, const float* gscale, float T,
                             float* dH, int lddh, hipStream_t s);
int launch_loss_delta(int mode, const float* PRED, int ldp, const float* Y, int ldy, const int* ROWS, int B,
                      const linna_loss_desc_t& d, float* DELTA, int ldd, hipStream_t s);
int launch_loss_fused_small(const float* PRED, int ldp, const float* Y, int ldy, const int* ROWS, int B,
                            const linna_loss_desc_t& d, const float* den, float inv_batch, float* loss_rows, float* loss_mean,
                            float* dP, int lddp, unsigned* counter, hipStream_t s);
int launch_loss_rows(int mode, const float* partial, int slots_ld, int nslots, int B, const float* den, const int* ROWS,
                     float floorv, float* out, hipStream_t s);
int launch_loss_grad(const float* U, int ldu, const float* Y, int ldy, const int* ROWS, int B, int nout,
                     const float* data_norm, const float* den, float inv_batch, float* dP, int lddp, hipStream_t s);
int launch_sum_scale(const float* v, int n, float scale, float* out, hipStream_t s);
int launch_sum_scale_prepare(const float* v, int n, float scale, float* out, int* step_dev, float* hyper, float b1, float b2,
                             hipStream_t s);
int launch_val_frac(const float* partial, int slots_ld, int nslots, int B, const float* den, float* frac, hipStream_t s);
int launch_val_metrics(const float* loss, const float* frac, int n, const float* last, float* out, hipStream_t s);
int launch_gather_xform(const float* X, int ldx, const int* ROWS, int B, int nin, const int* lg, const float* xmean,
                        const float* xstd, float* XB, int ldxb, hipStream_t s);
int launch_colsum(const float* dZ, int ld, int B, int N, float scale, float* db, hipStream_t s);
int launch_adamw(float* p, const float* g, float* m, float* v, size_t n, float* hyper, int* step_dev, float b1, float b2,
                 float eps, hipStream_t s);
int launch_adamw_prepare(float* hyper, int* step_dev, float b1, float b2, hipStream_t s);
int launch_stretch_propose(const float* coords, int ldc, int ndim, const int* S, int ns, const float* ccoords, int ldcc,
                           const int* C, int nc, uint64_t seed, const int* step_dev, int stream_id, float a, float* Q,
                           int ldq, float* factors, hipStream_t s);
int launch_stretch_accept(float* coords, int ldc, int ndim, float* logp, const int* S, int ns, const float* Q, int ldq,
                          const float* lp_new, const float* factors, uint64_t seed, const int* step_dev, int stream_id,
                          int* naccept, hipStream_t s);
// hmc.hip: the leapfrog's kick and drift as a launch of its own, P += ek G; Q += ed P / mass -- what the layered gradient route
// of api.hip enqueues behind its last launch.  eps (nullable): a step size per chain in device memory, ek / ed then multiply it
int launch_hmc_kick_drift(int B, int ndim, const float* mass, float ek, float ed, const float* G, int ldg, float* P,
                          int ldp, float* Q, int ldq, hipStream_t s, const float* eps = nullptr);
int launch_slice_points(const float* coords, int ldc, int ndim, const int* S, int ns, const float* DIR, int ldd,
                        const float* w, float* Q, int ldq, int nrep, hipStream_t s);
int launch_slice_expand(const float* Z0, const float* ZL, const float* ZR, float* L, float* R, int* flags, int ns,
                        int* counters, int slot, hipStream_t s);
int launch_slice_draw(const float* L, const float* R, const int* S, float* W, const int* flags, int ns, uint64_t seed,
                      const int* step_dev, int stream_id, int round, int ntrial, hipStream_t s);
int launch_slice_shrink(const float* Z0, const float* Zt, float* L, float* R, const float* W, int* flags, float* Wacc,
                        float* Zacc, int ns, int* counters, int slot, int ntrial, hipStream_t s);
// the one set-up launcher: W (the first round's bracket ends) and b.counters (the usage counters' roll) are each nullable
int launch_slice_begin(const SliceBegin& b, const int* S, int ns, int ndim, float* W, hipStream_t s);
int launch_slice_expand_multi(const float* Z0, const float* Zt, float* L, float* R, const int* S, int* flags, int ns, int m,
                              int m_next, int* counters, int slot, int prev_slot, float* W, float* Wd, int* list, uint64_t seed,
                              const int* step_dev, int stream_id_shrink, int ntrial, hipStream_t s);
int launch_slice_shrink_multi(const SliceRound& a, hipStream_t s);
int launch_slice_commit(float* coords, int ldc, int ndim, float* logp, const int* S, int ns, const float* DIR, int ldd,
                        const float* Wacc, const float* Zacc, hipStream_t s);
int launch_step_increment(int* step, hipStream_t s);

// Dense inverse covariance for the whole-network kernel: the output map d = raw * cscale + cshift is folded into the last
// layer of the weight stream and S (symmetric, [nout][lds]) is appended as one more segment, chi2 = d . (d S).
struct NsDense { const float* S; int lds; const float* cscale; const float* cshift; int factored = 0;   // factored: S holds L (S = L L^T), chi2 = |d L|^2
                 int tri = 2; };         // how the factor's zero upper triangle is skipped (net_stream_dense_tri): 0 not, 1 short second pass, 2 balanced blocks
// process-wide default of NsDense::tri for log-probability objects created afterwards (LINNA_DENSE_TRI); returns the previous value
int net_stream_dense_tri(int mode);
// net_stream.hip (program-driven whole-network kernel: residual blocks, widths up to 1024) and its planner net_program.hip.  The programs it runs, one
// weight stream each:
enum NsKind {
    NS_SERVE,          // log-probability: prior map, network, output map, diagonal likelihood (+ the fused MLP gradient)
    NS_SERVE_DENSE,    // ... with the output map folded into the last layer and the dense inverse covariance (NsDense) behind it
    NS_SERVE_BF16,     // the opt-in bf16 serving engine (linna_logprob_set_precision): diagonal likelihood, no gradient
    NS_STORE,          // training / validation forward: every op's output stored for the backward
    NS_TRAIN_FWD,      // training forward + chi^2-ratio loss (NsDense: the loss's inverse covariance)
    NS_DX,             // the dX chain of a training step: ops nl-1..1
    NS_DX_INPUT,       // ... down to op 0
    NS_GRAD_INPUT,     // forward + dX chain down to the input: lnP and its gradient in one launch, any network it covers
    NS_TRAIN_STEP,     // forward + loss + dX chain down to op 1: the merged training step (4-row engine)
    NS_TRAIN_STEP_BF16,   // ... in bf16 (linna_net_set_train_precision): bf16 runs, the loss segment an fp32 run, first layer [W | W]
    NS_GRAD_INPUT_BF16,   // NS_GRAD_INPUT in bf16 (linna_logprob_set_grad_precision): every run bf16, first layer [W | W], no SIDE segments
    NS_GRAD_INPUT_WIDE,   // NS_GRAD_INPUT for networks of MORE than 64 outputs (net_stream_wide_kernel): the same program, fitted to the LDS per engine
    NS_GRAD_INPUT_DENSE,  // lnP and its gradient for a DENSE inverse covariance S = L L^T (net_stream_dense_kernel; opt-in): forward with the
                          // output map folded into the last layer, U = d L, turnaround in U-space, the transposed dense map, dX chain; any
                          // number of outputs, fitted to the LDS per engine
};
// the serving programs are built from the layer list with the trailing input skip, the training ones from the list without
inline bool ns_kind_full_layers(NsKind k) { return k == NS_SERVE || k == NS_SERVE_DENSE || k == NS_SERVE_BF16; }
// Planning query (no GPU): ok: the network has this program (NS_GRAD_INPUT, NS_GRAD_INPUT_BF16: and its sign-bit gates fit
// the LDS; NS_TRAIN_STEP: with the dX chain); packed_floats: the size of a copy of its weight stream, for every engine;
// grad_ok: the serving program holds the fused MLP gradient; why: the reason when a bf16 kind is refused.
struct NsPlan { bool ok; size_t packed_floats; bool grad_ok; const char* why; };
NsPlan net_stream_plan(NsKind kind, const linna_layer_t* layers, int nl, int in_size, const NsDense* dn = nullptr);
// rows per workgroup for a batch of B rows: 16 (v_mfma_f32_16x16x4_f32), or 8 / 4 (v_mfma_f32_4x4x1_16b_f32) when 16-row
// workgroups would leave CUs idle.  The 16-row engine and the small ones read different orders of the weight stream.
int net_stream_rows(int B);
int net_stream_force_rows(int rows);   // 0 automatic, 4 / 8 / 16 forced; returns the previous setting, -1 for an invalid value
// The fp32 one-launch gradient's program kind for this op list: NS_GRAD_INPUT up to 64 outputs (it fits every engine or
// none), NS_GRAD_INPUT_WIDE beyond
inline NsKind ns_grad_kind(const linna_layer_t* layers, int nl) { return nl >= 1 && layers[nl - 1].N > 64 ? NS_GRAD_INPUT_WIDE : NS_GRAD_INPUT; }
// Whether that program runs on the engine of `rows` rows: it and its sign bits fit the LDS (host-side planning only).  A
// batch whose engine it does not fit takes the layered route.
bool net_stream_grad_fits(const linna_layer_t* layers, int nl, int in_size, int rows);
// The same for the dense one-launch gradient (NS_GRAD_INPUT_DENSE with the factored `dn`)
bool net_stream_grad_dense_fits(const linna_layer_t* layers, int nl, int in_size, const NsDense* dn, int rows);
int launch_net_stream_pack(NsKind kind, const linna_layer_t* layers, int nl, int in_size, float* packed, int rows, const NsDense* dn,
                           hipStream_t s);
int net_stream_describe(NsKind kind, const linna_layer_t* layers, int nl, int in_size, const NsDense* dn, int rows, char* buf, size_t n);
// The PLAIN instantiation of the serving kernel (net_stream_plain_kernel).  net_stream_serve_plain: the process-wide switch
// (1 default: eligible launches take it; 0: every launch the generic instantiation; -1 queries; returns the previous value).
// net_stream_program_plain: whether the serving program of this op list on the engine of `rows` rows is a plain one
// (ns_program_plain, net_program.hip: host-side planning only).  net_stream_launch_plain_ok: whether a launch of that program
// with this output map and these outputs takes it when the switch is on.
int net_stream_serve_plain(int on);
// The step of a plain launch: 1 (default) net_stream_placed_kernel, the step placed by hand; 0 net_stream_plain_kernel, the
// compiler-scheduled one (same lnP bit for bit; interleaved A/B); -1 queries; returns the previous value.
int net_stream_serve_plain_sched(int hand);
// A hand-placed plain launch without the MFMAs that multiply zero padding: 1 (default) net_stream_trim_kernel, 0
// net_stream_placed_kernel (same lnP bit for bit; interleaved A/B); -1 queries; returns the previous value.
// net_stream_trim_describe: the liveness the launcher hands that kernel, as text (host-side planning only).
int net_stream_serve_plain_trim(int on);
int net_stream_trim_describe(const linna_layer_t* layers, int nl, int in_size, int rows, char* buf, size_t n);
bool net_stream_program_plain(NsKind kind, const linna_layer_t* layers, int nl, int in_size, const NsDense* dn, int rows);
bool net_stream_launch_plain_ok(bool cscale, bool cshift, bool w, bool cexp, bool lnP, bool D, bool TH, bool gate);
// What always travels together into the launchers of the whole-network kernel: plain records, copied field by field into
// NsArgs.  NsNet: the op list a program is planned from (with or without the trailing input skip: ns_kind_full_layers) and
// the network's input width.  NsInput: the prior map and the input transform.  NsOutput: the output map and the diagonal
// likelihood (cpost / cshift2: the exp output map's second half, or null).
struct NsNet { const linna_layer_t* layers; int nl, in_size; };
struct NsInput { int nin; const int* is_flat; const float* a1; const float* a2; const int* lg; const float* xmean; const float* xstd; };
struct NsOutput { const float* cscale; const float* cshift; const float* cpost; const float* cshift2; const float* w; float T; };
// What the entries vary in a serving launch: the rows Z[B][ldz], lnP[B], the device gate (linna_logprob_eval_if), the
// physical parameters TH and the residuals D (null: not written)
struct NsRun { const float* Z; int ldz; int B; float* lnP; const int* gate = nullptr; float* TH = nullptr; int ldt = 0; float* D = nullptr; int ldd = 0; };
// Where a training step's activations and their gradients live, per op (api.hip: net_bufs): y its output, t the hidden h
// of a residual block, x its input and `gate` = x where x went through a ReLU (else null; leading dimension ldx); dprev
// d/d(op input), dt d/dh of a residual block.
struct NsOpBufs { float* y; int ldy; float* t; int ldt; const float* x; int ldx; const float* gate; float* dprev; int ldp; float* dt; int lddt; };
// A small job that rides in the dX-chain launch as one extra workgroup (linna_net_train_step): the batch mean of the loss
// rows (out = scale * sum rows[n], sum_scale_prepare_kernel's order) and AdamW's step counter / bias corrections
struct NsPost { const float* rows; int n; float scale; float* out; int* step; float* hyper; float b1, b2; };
int launch_net_stream_dx(const NsNet& net, const float* packed, const float* dOUT, int lddo, int B, const NsOpBufs* ops, int with_input,
                         int rows, hipStream_t s, const NsPost* post = nullptr);
// sampler moves fused around the evaluation.  slice == 0: stretch half step, rows of the batch are the walkers
// S[0..B).  slice == 1: rows are the slice sampler's trial points coords[S[k]] + cc[row] * DIR[k], k = row % nc
// (DIR is passed as the launch's Z / ldz; cc = w[nrep * ns], nc = ns; nothing is written back).
struct NsMove {
    float* coords; int ldc; float* logp; const int* S;
    const float* cc; int ldcc; const int* C; int nc;
    unsigned long long seed; const int* step; int step_off; int stream; float a; int* naccept;
    int slice;
    float* chain = nullptr; float* lps = nullptr;      // stretch move: this iteration's row of the chain block ([nw][ndim], [nw]); null: none
    // slice == 1, sl_Zt != null: the trial weights are derived in the kernel from the one stepping-out round's results (NsArgs::sl_*)
    const float* sl_Z0 = nullptr; const float* sl_L = nullptr; const float* sl_R = nullptr; const float* sl_Zt = nullptr;
    int sl_m = 0, sl_nt = 0; unsigned long long sl_seed = 0; const int* sl_step = nullptr; int sl_stream = 0;
    const int* sl_flags = nullptr;                      // the stepping-out budgets left (flags[3k], flags[3k + 1])
    const SliceBegin* sb = nullptr;                     // slice == 1: this evaluation is the half step's first and sets it up (SliceBegin)
};
// training / validation forward: every op's output stored for the backward (STORE instantiation)
int launch_net_stream_store(const NsNet& net, const float* packed, const float* X, int ldx, int B, const NsOpBufs* ops,
                            const float* cscale, const float* cshift, int rows, hipStream_t s);
// training forward + chi^2-ratio loss in one launch (STORE == 3)
struct NsTrainLoss { const float* YN; int ldyn;      // normalised targets of the whole set, NaN where masked
                     const float* den; float inv_batch; float* loss_rows; float* dP; int lddp; };
// the batch of a training step: rows ROWS[B] (null: 0..B-1) of the resident set X, gathered and X-transformed into XB
struct NsBatch { const float* X; int ldx; const int* ROWS; int B; const int* lg; const float* xmean; const float* xstd; float* XB; int ldxb; };
int launch_loss_targets(const float* Y, int ldy, int n, const linna_loss_desc_t& d, float* YN, int ldyn, hipStream_t s);
int launch_net_stream_train(const NsNet& net, const float* packed, const NsBatch& b, const NsOpBufs* ops, const NsTrainLoss& L,
                            const NsDense& dn, int rows, hipStream_t s);
// the same followed by the dX chain down to op 1 in the SAME launch (GRAD + STORE == 3; NS_TRAIN_STEP)
int launch_net_stream_train_bwd(const NsNet& net, const float* packed, const NsBatch& b, const NsOpBufs* ops, const NsTrainLoss& L,
                                const NsDense& dn, int rows, hipStream_t s, const NsPost* post,
                                bool bf = false);     // bf: NS_TRAIN_STEP_BF16 (net_stream_train_bf16_kernel)
// gradient fused behind the evaluation (plain ReLU MLPs, diagonal covariance): G = d lnP / d z
// NsLeap: a leapfrog kick and drift riding behind the gradient (HMCSampler.py:35-49): P += ek G; Q += ed P / mass, Q the
// launch's own input rows (P == nullptr: none rides); eps (nullable): a step size per row, ek and ed are then its multipliers
struct NsLeap { float* P; int ldp; float* Q; const float* mass; float ek, ed; const float* eps; };
struct NsGrad { const float* gscale; float* G; int ldg; NsLeap leap; };
// ALL that hmc.hip's whole-transition driver sees of a log-probability object (api.hip; struct linna_logprob stays private to
// it): its input width; LINNA_OK where a gradient route exists, else the refusal with its text; and lnP[B] with G = d lnP / d z
// at Z enqueued on `stream`, with `leap` (nullable) the leapfrog's kick and drift behind it -- linna_logprob_grad's checks
int logprob_nin(const linna_logprob_t* lp);
int logprob_grad_ready(const linna_logprob_t* lp);
int logprob_grad_impl(linna_logprob_t* lp, const float* Z, int ldz, int B, void* ws, float* lnP, float* G, int ldg,
                      const NsLeap* leap, void* stream);
// AdamW that also writes the two weight streams of a training step (net_stream.hip: adamw_streams_kernel; gemm.hip: the
// update epilogue of the grouped parameter-gradient launch).  An AsPlace says where the elements of a weight matrix sit
// in one fragment-order stream (segment type 0 = WIDE, 1 = SPLIT; see net_stream.hip).
constexpr int AS_MAXR = 26, AS_MAXW = 14, AS_MAXB = 12;
struct AsPlace { float* out; float scale; int trans, koff, ncols, type, ncg, steps, G, first0, first1; };
struct AsMat { int N, ld; AsPlace pl[2]; };            // pl[0]: forward(+loss) stream, pl[1]: dX-chain stream
struct AsBias { float* out; float scale; int N; };
struct AsRange { unsigned off4, n4, blk0; short kind, idx; };   // a tensor of the flat buffer, in units of 4 floats
struct AsArgs { AsRange r[AS_MAXR]; AsMat w[AS_MAXW]; AsBias b[AS_MAXB]; int nr, small; unsigned nblocks; };
// float index of element (column nn, depth kk) of a segment in its stream (4 step tiles per wave and step, 64 lanes x 4 floats each)
__device__ __forceinline__ size_t as_slot(const AsPlace& q, int small, int nn, int kk) {
    const int nl = nn & 63, ks = kk >> 4, kr = kk & 15;
    int w, g;
    if (q.type == 0) { w = (nn & 511) >> 6; g = ((nn >> 9) ? q.first1 : q.first0) + ks; }
    else { const int kp = ks / q.steps; w = kp * q.ncg + (nn >> 6); g = q.first0 + (ks - kp * q.steps); }
    const int t = small ? kr >> 2 : nl >> 4, lane = small ? nl : (nl & 15) + 16 * (kr >> 2);
    return ((((size_t)w * q.G + g) * 4 + t) * 64 + lane) * 4 + (kr & 3);
}
// the same for a bf16 stream of the small-batch engines (NS_TRAIN_STEP_BF16): the bf16 element index of (nn, kk) -- a step is 32 k,
// each 16-byte vector eight bf16 (lane = column, load t = k chunk of 8)
__device__ __forceinline__ size_t as_slot_bf16(const AsPlace& q, int nn, int kk) {
    const int nl = nn & 63, ks = kk >> 5, kr = kk & 31;
    int w, g;
    if (q.type == 0) { w = (nn & 511) >> 6; g = ((nn >> 9) ? q.first1 : q.first0) + ks; }
    else { const int kp = ks / q.steps; w = kp * q.ncg + (nn >> 6); g = q.first0 + (ks - kp * q.steps); }
    return ((((size_t)w * q.G + g) * 4 + (kr >> 3)) * 64 + nl) * 8 + (kr & 7);
}
typedef __bf16 bf16x4_t __attribute__((ext_vector_type(4)));
// torch.optim.AdamW's single-tensor update of one element (pointwise.hip adamw_kernel's arithmetic, operation for operation)
__device__ __forceinline__ void adamw_one(float& pi, float gi, float& mi, float& vi, float lr, float wd, float bc1, float sbc2,
                                          float beta1, float beta2, float eps) {
    pi = pi * (1.f - lr * wd);
    mi = mi + (gi - mi) * (1.f - beta1);
    vi = vi * beta2 + (1.f - beta2) * gi * gi;
    const float denom = sqrtf(vi) / sbc2 + eps;
    pi = pi - (lr / bc1) * (mi / denom);
}
// merged = 2: the bf16 training stream (NS_TRAIN_STEP_BF16): the places say where the bf16 elements go (as_slot_bf16, ncols = the
// matrix's columns K), and the first layer's [W | W] is two places of one matrix (pl[0] and pl[1]: it has no dX-chain place)
int net_stream_adamw_args(const linna_layer_t* layers, int nl, int in_size, int rows, const float* params, size_t nflat,
                          float* s_fwd, const NsDense* dn, float* s_dx, AsArgs* out, int merged = 0);
int launch_adamw_streams(const AsArgs& a, float* p, const float* g, float* m, float* v, const float* hyper, float b1, float b2,
                         float eps, hipStream_t s, bool bf = false);
// forward + dX chain down to the input in one launch (NS_GRAD_INPUT, or bf: NS_GRAD_INPUT_BF16; diagonal covariance)
int launch_net_stream_grad2(const NsNet& net, const float* packed, const NsRun& r, const NsInput& in, const NsOutput& out, const NsGrad& gr,
                            int rows, hipStream_t s, bool bf = false);
// the same for a dense inverse covariance in its factored form (NS_GRAD_INPUT_DENSE: the output map and L are in the stream;
// gr.gscale is not read)
int launch_net_stream_grad_dense(const NsNet& net, const float* packed, const NsRun& r, const NsInput& in, float T, const NsGrad& gr,
                                 int rows, const NsDense& dn, hipStream_t s);
// a serving launch (kind NS_SERVE, NS_SERVE_DENSE with dn, or NS_SERVE_BF16)
bool net_stream_takes_plain(NsKind kind, const NsNet& net, const NsOutput& out, const NsRun& r, const NsMove* mv, const NsGrad* gr, int rows,
                            const NsDense* dn);   // what launch_net_stream decides
int launch_net_stream(NsKind kind, const NsNet& net, const float* packed, const NsRun& r, const NsInput& in, const NsOutput& out,
                      const NsMove* mv, const NsGrad* gr, int rows, const NsDense* dn, hipStream_t s);

int gemm_slots(int M, int N);            // number of row-dot partial slots gemm_launch will write
int gemm_launch(const GemmArgs& a, hipStream_t stream);
// several independent k-major x k-major problems in ONE grid (gemm.hip: gemm_group_kernel): C[M][N] = alpha * A^T B over
// K (the batch), db[M] = alpha * column sums of A (null: none); descriptors by value in the kernel arguments
struct GemmGroupProb { const float* A; const float* B; float* C; float* db; int lda, ldb, ldc, K, M, N; float alpha; int first; };
constexpr int GEMM_GROUP_MAX = 48;
struct GemmGroupArgs { GemmGroupProb p[GEMM_GROUP_MAX]; int nprob; };
// The same launch with the optimiser in its epilogue (linna_net_train_step_update): every tile applies AdamW to the block of
// the weight matrix whose gradient it has just formed (parameters / moments at fixed distances from the gradient buffer)
// and puts the updated block into the two weight streams of the next step -- no AdamW launch, no re-layout.
constexpr int GEMM_UPD_MAX = 16;
struct GemmGroupArgsS { GemmGroupProb p[GEMM_UPD_MAX]; int nprob; };
struct GemmUpdate { long long pdiff, mdiff, vdiff;           // parameter / moment pointers = gradient pointer + these (floats)
                    const float* hyper; float beta1, beta2, eps; int small;
                    AsPlace pl[GEMM_UPD_MAX][2]; AsBias bias[GEMM_UPD_MAX]; };
struct GemmUpd1 { long long pdiff, mdiff, vdiff; const float* hyper; float beta1, beta2, eps; int small; AsPlace pl[2]; AsBias bias; };
struct GemmPost { const float* rows; int n; float scale; float* out; };   // batch mean of the loss rows riding as one extra workgroup
// bf: the places are those of a bf16 training stream (net_stream_adamw_args, merged = 2)
int gemm_launch_group_update(const GemmGroupArgsS& g, const GemmUpdate& u, int nblocks, hipStream_t stream, const GemmPost* post = nullptr,
                             bool bf = false);
bool gemm_group_ok(const GemmArgs& a);
int gemm_group_blocks(const GemmArgs& a);
int gemm_launch_group(const GemmGroupArgs& g, int nblocks, hipStream_t stream, const GemmPost* post = nullptr);

}  // namespace linna
