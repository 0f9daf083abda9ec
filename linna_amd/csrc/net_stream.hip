// Whole-network serving kernel ("network stream"): ONE launch evaluates util.Log_prob.__call__
// (util.py:990-1021) for 16 walkers per workgroup -- prior map + input transform (util.py:339-347,
// 483-497), every layer, the output transform and the diagonal Gaussian log-likelihood
// (util.py:953-955) -- for the reference's own architectures, ChtoModelv2 / ChtoModelsimple
// (nn.py:59-133, 300-374: Linear + three residual blocks + three Linears), and for plain MLPs of
// any width up to 1024 (BASELINE configs 2/5: 33 -> 512 x 4 -> 33).
//
// MI355X mapping
//  * one 512-thread workgroup (8 waves, two per SIMD) per CU owns 16 walker rows; activations stay
//    in LDS for the whole network, double-buffered [2][16][LD] fp32 (LD = widest row + 4: the
//    stride makes ds_read_b128 and the epilogue's ds_write_b32 conflict-free);
//  * weights never touch LDS.  With 16 rows per workgroup no wave shares a weight with another
//    wave, so they are re-laid ONCE per weight update into MFMA FRAGMENT ORDER (ns_pack_kernel):
//    the B operand of a step's column tile is 1 KiB contiguous, lane-linear, and one coalesced
//    global_load_dwordx4 puts it straight into the registers the MFMA reads.  Every wave owns ONE
//    contiguous stream over the whole network; a ring of R register sets keeps R-1 steps (20 KiB
//    per wave) in flight across layer boundaries with counted s_waitcnt vmcnt;
//  * v_mfma_f32_16x16x4_f32 (exact fp32) with the k-permutation trick: lane group kq owns 4
//    consecutive k, element s of the 128-bit A and B fragments feeds MFMA s;
//  * ONE copy of the step loop serves every layer: the network is a small PROGRAM of segments.
//
// Program = list of segments, each a GEMM over the activation rows held in LDS:
//   WIDE    (N > 256, or a short K): the N columns are split over the 8 waves in passes of 512 (wave w owns column
//           tiles 4w..4w+3 of a pass), every wave runs all K steps; epilogue bias(+ReLU) -> the
//           OTHER activation buffer; one barrier after the last pass.
//   SPLIT   N <= 256: the columns form ncg = 1, 2 or 4 groups of 64 and K is split over the
//           8/ncg waves of a group (wave = kpart*ncg + group), partial sums are reduced through
//           LDS, bias(+ReLU) -> the CURRENT buffer at a column offset (two barriers).  Keeps all
//           eight waves on real columns where WIDE would leave most of its 32 tiles empty.
// A residual block  y = relu(0.1 (W2 relu(W1 x + b1) + b2) + Ws x)  (nn.py:45-56) is SPLIT
// (h = relu(W1 x + b1), written right behind x in the same buffer) + ONE GEMM over the
// concatenated K = [x ; h] with the concatenated weight [Ws | 0.1 W2] and bias 0.1 b2.
// One step = 16 k x 64 columns = 1 ds_read_b128 (A) + 4 coalesced 1-KiB global loads (B, fragment
// order, see pack below) + 16 v_mfma_f32_16x16x4_f32.
// After the last segment the output row block sits in LDS: output transform, optional store of
// d, diagonal Gaussian log-likelihood (util.py:953-955) with 32-lane shuffles.
//
// Small batches (ROWS = 8 or 4 instantiations).  With 16 rows per workgroup a batch of B rows occupies B/16 of
// the 256 CUs and the launch lasts as long as one workgroup needs for the whole network, whatever B is: an
// ensemble half step of 2048 proposals (128 workgroups), a training batch of 500 (32), the reference's own
// ensembles of 4..128 walkers (1..8).  The same program runs with 8 or 4 rows per workgroup on
// v_mfma_f32_4x4x1_16b_f32: one instruction multiplies 4 rows by the wave's 64 columns at k = 1 (lane = column;
// CBSZ = 4 broadcasts the A values of block ABID to all 16 blocks, so the ONE ds_read_b128 per step still fetches
// 16 k of every row: block b of the read holds row set b & 3, k chunk b >> 2), at the same flop rate per
// instruction cycle as 16x16x4 (measured: tools/probe/mfma4_probe.hip).  Four accumulator chains per row set (one
// per k chunk) keep dependent instructions 32 cycles apart.  The weight stream is the same bytes in another order
// (lane = column, see ns_pack_kernel), so a workgroup of 8 (4) rows needs 2x (4x) the weight bandwidth per flop:
// 64 (128) B/clk/CU at full MFMA rate against the 64 B/clk a CU's vector L1 delivers -- the small engines are
// L1-fill bound, which still halves the time of a launch that cannot fill the chip.
#include "common.h"
#include <stdlib.h>
#include <type_traits>
#include <vector>
#include <cstring>
#include <algorithm>
#include <atomic>
#include <memory>
#include <mutex>
#include <string>
#include <unordered_map>

namespace linna {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));   // B (and A) operand of v_mfma_f32_16x16x32_bf16
typedef short s16x4 __attribute__((ext_vector_type(4)));     // ... of v_mfma_f32_4x4x4_16b_bf16 (the builtin takes the bits)

constexpr int NS_ROWS = 16;                // rows per workgroup of the large-batch engine (and the LDS layout bound)
constexpr int NS_NW = 8;                 // waves per workgroup
constexpr int NS_NT = 4;                 // 16-column tiles per wave and step
constexpr int NS_MAXSEG = 20;
constexpr int NS_MAXRUN = 40;
constexpr unsigned NS_STEP_B = NS_NT * 1024;
constexpr int NS_LDS_BYTES = 160 * 1024;
#ifndef NS_R
#define NS_R 6
#endif
#ifndef NS_PRE
#define NS_PRE 2
#endif
enum { NS_WIDE = 0, NS_SPLIT = 1, NS_SIDE = 2 };

struct NsSeg {            // kernel-side view of a segment
    int type, steps, passes, bias_off;
    int dst_col, relu, kslice, zext;   // SPLIT: kslice = k offset between K parts (16*steps), zext = columns written
                                       // WIDE with a SHORT second pass (zext > 0): pass 1 runs zext steps from k offset kslice -- the
                                       // lower-triangular factor of a dense inverse covariance has no rows k < 512 in columns >= 512
    int ncg_log2;                      // SPLIT: log2 of the number of 64-column groups
    int mask_store, mask_apply;        // GRAD: 1 + LDS slot of the ReLU sign bits this WIDE segment records / applies (0: none)
    int x0_n;                          // ... that many columns of them (a multiple of 16)
    int x0_col;                        // > 0: the network INPUT rows (kept aside in LDS) are copied to this column of the segment's
                                       // input buffer before it runs (ChtoModelv2_linear's input skip, nn.py:160-163,195)
    int kcl, side_off;                 // SIDE: log2 of the k chunks per wave and step; float offset of its weights from `packed`
};

struct NsArgs {
    const float* Z; int ldz; int B; int nin;
    const int* is_flat; const float* a1; const float* a2; const int* lg;
    const float* xmean; const float* xstd;
    const float* packed;                // [8 waves][G][4][64 lanes][4] then the packed biases
    int G, nseg, LD, kpad0, nout, bias_total;
    int Gstride, nseg_f;                // steps per wave in the packed stream; forward segments (GRAD: the rest is the backward)
    const float* gscale; float* Gout; int ldg;   // GRAD: d(d)/d(raw output); d lnP / d z
    float* hm_p; int hm_ldp; float* hm_q; const float* hm_mass; float hm_ek, hm_ed;   // GRAD: leapfrog kick + drift in the finish
    const float* cscale; const float* cshift; const float* w; float T;
    const float* cpost; const float* cshift2;   // ypositive output map (util.py:540): d = exp(raw cscale + cshift) cpost + cshift2
    float* lnP; float* D; int ldd; float* TH; int ldt;
    unsigned long long* stamps;
    const int* gate;                    // optional: every workgroup leaves at once when gate[0] == 0 (speculatively queued rounds)
    // STORE instantiation (training / validation forward, nn.py:110-133): the input rows are taken as they are
    // (already X-transformed), every segment's output ALSO goes to global memory for the backward, no likelihood
    float* gout[NS_MAXSEG]; int gld[NS_MAXSEG]; int gn[NS_MAXSEG];
    // STORE == 2 (the dX chain of a training step): a segment's output is zeroed where gmask (the stored forward
    // activation whose gradient it is) is not positive, before it is stored and handed to the next segment
    const float* gmask[NS_MAXSEG]; int gmld[NS_MAXSEG];
    // GRAD + STORE == 2 (lnP and its gradient in one launch, any network): the backward needs the SIGN of the forward
    // activations only, and it needs it in this very workgroup -- one bit per (row, column) in LDS ([ROWS][nbw] words at
    // float offset bits_off) instead of the activations in global memory.  gbit / mbit: the first bit column (a multiple of
    // 64) of the tensor a segment writes / is gated by, -1 = none.  The merged training launch (GRAD + STORE == 3) gates the
    // same way -- its activations still go to global memory, the parameter gradients need them.
    int nbw, bits_off;
    int gbit[NS_MAXSEG], mbit[NS_MAXSEG];
    // STORE == 3 (one launch = gather + input transform + training forward + chi^2-ratio loss and its gradient,
    // predictor_gpu.py:274-285 with util.py:1070-1116): Z is the RESIDENT training set X[n][ldz], row `t_rows[b]` is
    // transformed in the prologue (and stored to t_xb for the first layer's parameter gradient); the last network layer's
    // epilogue turns pred into delta = mask ? 0 : ynorm - pred in LDS (ynorm, with its mask, precomputed for the whole
    // set: one load per element); the program's last segment is U = delta Cinv; the finish writes
    // loss_b = delta.U / den and d loss / d pred = -2 U inv_batch / den
    const int* t_rows; float* t_xb; int t_ldxb;
    const float* t_Y; int t_ldy;            // NORMALISED targets of the whole set, NaN where masked (linna_loss_targets)
    const float* t_den; float t_inv_batch; float* t_loss_rows; float* t_dP; int t_lddp;
    // dense inverse covariance as the program's last segment: U = d S sits at column u_col of the current buffer
    // (u_same) or at column 0 with d in the other buffer; the finish takes chi2 = d . U
    int dense, u_col, u_same;
    int x0_keep;                        // the program copies the input rows somewhere later (NsSeg::x0_col): keep them in LDS
    // STORE == 2 rider (linna_net_train_step): ONE extra workgroup of the launch takes the batch mean of the loss rows the
    // forward + loss launch wrote and advances AdamW's step counter / bias corrections -- sum_scale_prepare_kernel's job,
    // on a CU the dX chain leaves idle instead of a launch of its own between the two
    const float* p_rows; int p_n; float p_scale; float* p_out; int* p_step; float* p_hyper; float p_b1, p_b2;
    // stretch move fused around the evaluation (MOVE instantiation; emcee StretchMove behind sampler.py:493-495)
    float* mv_coords; int mv_ldc; float* mv_logp; const int* mv_S;
    const float* mv_cc; int mv_ldcc; const int* mv_C; int mv_nc;
    unsigned long long mv_seed; const int* mv_step; int mv_step_off; int mv_stream; float mv_a; int* mv_naccept;
    float* mv_chain; float* mv_lps;     // MOVE == 1: row of the chain block this iteration fills (linna_stretch_run), [nw][nin] / [nw]
    // MOVE == 2, sl_Zt != null: the FIRST shrinking round of a half step whose stepping-out was one round of sl_m bracket ends per
    // side -- the trial weight of row j ns + k is derived here from that round's results instead of being read: bracket
    // [L, R] pushed out while lnP at the ends exceeds Z0 (slice_expand_multi_kernel), then trial j placed as if its
    // predecessors were rejected (slice_draw_dev: Philox (walker, step, stream, sub j + 1)).  Saves the launch between them.
    const float* sl_Z0; const float* sl_L; const float* sl_R; const float* sl_Zt; int sl_m, sl_nt;
    unsigned long long sl_seed; const int* sl_step; int sl_stream; const int* sl_flags;
    SliceBegin sb;                      // MOVE == 2, sb.logp != null: the half step's set-up in this launch's prologue (common.h)
    NsSeg seg[NS_MAXSEG];
};

// ------------------------------------------------------------------ weight re-layout
struct NsPackSeg {
    const float* Wa; int lda, Ka, Kapad;          // first K part (Wa NULL: identity)
    const float* Wb; int ldb, Kb; float alpha;    // second K part, scaled (residual blocks)
    const float* b; float bscale;
    const float* b2; float b2scale;                // second bias term (input skip: alpha * bl)
    int N, type, steps, passes, bias_off, bias_pad, ncg;
    int transA;                                   // Wa is read transposed: value(n, k) = Wa[k][n] (backward segments)
    int transB;                                   // the same for Wb
    const float* rscale; const float* rshift;     // per output column: weights and bias * rscale, bias + rshift (folded output map)
    int kc, side_off;                             // SIDE segments: k chunks per wave and step (2 or 4), float offset of their block
    int koff2;                                    // WIDE with a short second pass: k offset of pass 1 (NsSeg::kslice)
};
// SIDE segments (serving programs of the 16-row engine): a SPLIT segment of <= 32 output columns -- the hidden
// h = relu(W1 x + b1) of a residual block, 1000 -> 16 and 500 -> 32 in ChtoModelv2 -- costs the step loop 8 + 4 steps of
// which three quarters / half multiply zero weights (a wave's four 16-column tiles need 64 columns).  As a SIDE segment it
// leaves the weight stream: its weights sit in a block of their own behind the biases, laid out so that a wave's four tiles
// are (column tile, k chunk) pairs -- kc = 4 chunks of 16 columns, or 2 chunks of 32 -- and the whole segment is at most
// two steps per wave, run inside the run-end code of the segment before it (loads issued before that segment's epilogue,
// by inline asm: the compiler's counted waits for the ring never see them).  The step loop itself is untouched.
//   side[w][s][t][lane][e]:  n = 16 (t % (4 / kc)) + li,  k = 16 (kc (w steps + s) + t / (4 / kc)) + 4 kq + e
struct NsPackArgs {
    NsPackSeg seg[NS_MAXSEG];
    int run_seg[NS_MAXRUN], run_pass[NS_MAXRUN], run_first[NS_MAXRUN + 1];
    int nseg, nrun, G, bias_total;
    int small;                                     // layout of the 4x4x1 engines: lane = column, load t = k chunk
    int bf;                                        // bf16 stream (NsProgram::bf): 32 k per step, eight bf16 per 16-byte vector
    float* out;                                    // weights, then biases
    int f32seg;                                    // bf: this segment's runs are fp32 all the same (NsProgram::f32seg; -1: none)
};
// stream[w][g][t][lane][e], run r = (segment, pass), s = g - first[r], li = lane & 15, kq = lane >> 4:
//   WIDE   n = 16 (32 pass + 4 w + t) + li,  k = 16 s + 4 kq + e
//   SPLIT  n = 64 (w % ncg) + 16 t + li,     k = 16 ((w / ncg) steps + s) + 4 kq + e
// value = [Wa | alpha Wb](n, k), zero outside.  Small-batch engines (p.small): the same 64 columns x 16 k per
// (w, g) with lane = column and load t = k chunk:  n = ... + lane,  k = ... + 4 t + e.
// bf16 stream (p.bf): a step is 32 k, each 16-byte vector eight bf16 -- 16 k in the formulas above becomes 32 and
// 4 kq (4 t) becomes 8 kq (8 t), e < 8.  The fp32 value (alpha Wb with alpha folded, rscale applied) is rounded to
// nearest-even by a plain cast (v_cvt_pk_bf16_f32: a NaN stays a NaN).
__device__ __forceinline__ float ns_pack_value(const NsPackSeg& S, int n, int k) {
    float v = 0.f;
    if (k < S.Kapad) {
        if (k < S.Ka) v = !S.Wa ? (k == n ? 1.f : 0.f) : S.transA ? S.Wa[(size_t)k * S.lda + n] : S.Wa[(size_t)n * S.lda + k];
    } else if (k - S.Kapad < S.Kb) {
        v = S.alpha * (S.transB ? S.Wb[(size_t)(k - S.Kapad) * S.ldb + n] : S.Wb[(size_t)n * S.ldb + (k - S.Kapad)]);
    }
    return S.rscale ? v * S.rscale[n] : v;
}
__device__ __forceinline__ void ns_pack_bf16(const NsPackArgs& p, size_t idx) {
    const int lane = (int)(idx & 63);
    size_t q = idx >> 6;
    const int t = (int)(q % NS_NT); q /= NS_NT;
    const int g = (int)(q % p.G);
    const int w = (int)(q / p.G);
    int r = 0;
    while (r + 1 < p.nrun && g >= p.run_first[r + 1]) ++r;
    const NsPackSeg& S = p.seg[p.run_seg[r]];
    const int s = g - p.run_first[r];
    const int nl = p.small ? lane : 16 * t + (lane & 15), kl = p.small ? 8 * t : 8 * (lane >> 4);
    int n, k0;
    if (S.type == NS_WIDE) { n = 512 * p.run_pass[r] + 64 * w + nl; k0 = 32 * s + kl + (p.run_pass[r] ? S.koff2 : 0); }
    else { n = 64 * (w % S.ncg) + nl; k0 = 32 * ((w / S.ncg) * S.steps + s) + kl; }
    bf16x8 v;
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = (__bf16)(n < S.N ? ns_pack_value(S, n, k0 + e) : 0.f);
    reinterpret_cast<bf16x8*>(p.out)[idx] = v;
}
// the segment whose run holds vector idx of the stream
__device__ __forceinline__ int ns_pack_seg_of(const NsPackArgs& p, size_t idx) {
    const int g = (int)((idx >> 6) / NS_NT % p.G);
    int r = 0;
    while (r + 1 < p.nrun && g >= p.run_first[r + 1]) ++r;
    return p.run_seg[r];
}
__global__ void ns_pack_kernel(NsPackArgs p) {
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t nw4 = (size_t)NS_NW * p.G * NS_NT * 64;
    if (idx < nw4 && p.bf && ns_pack_seg_of(p, idx) != p.f32seg) { ns_pack_bf16(p, idx); return; }
    if (idx < nw4) {
        const int lane = (int)(idx & 63);
        size_t q = idx >> 6;
        const int t = (int)(q % NS_NT); q /= NS_NT;
        const int g = (int)(q % p.G);
        const int w = (int)(q / p.G);
        int r = 0;
        while (r + 1 < p.nrun && g >= p.run_first[r + 1]) ++r;
        const NsPackSeg& S = p.seg[p.run_seg[r]];
        const int s = g - p.run_first[r];
        const int nl = p.small ? lane : 16 * t + (lane & 15), kl = p.small ? 4 * t : 4 * (lane >> 4);
        int n, k0;
        if (S.type == NS_WIDE && S.koff2 < 0) {        // balanced triangular factor: block w from row 64 w, then block 15 - w
            const int n0 = S.steps - 4 * w, blk = s < n0 ? w : 15 - w;
            n = 64 * blk + nl; k0 = 16 * (s < n0 ? s : s - n0) + 64 * blk + kl;
        } else if (S.type == NS_WIDE) { n = 512 * p.run_pass[r] + 64 * w + nl; k0 = 16 * s + kl + (p.run_pass[r] ? S.koff2 : 0); }
        else { n = 64 * (w % S.ncg) + nl; k0 = 16 * ((w / S.ncg) * S.steps + s) + kl; }
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (n < S.N && S.Wa && !S.transA && k0 + 3 < S.Ka && (S.lda & 3) == 0 && (reinterpret_cast<uintptr_t>(S.Wa) & 15) == 0) {
            // the common case: four consecutive k of one weight row, 16 bytes aligned (rows are padded to 4 floats)
            v = *reinterpret_cast<const f32x4*>(S.Wa + (size_t)n * S.lda + k0);
            if (S.rscale) { const float r = S.rscale[n]; v = f32x4{v[0] * r, v[1] * r, v[2] * r, v[3] * r}; }
        } else if (n < S.N) {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int k = k0 + e;
                if (k < S.Kapad) {
                    if (k < S.Ka) v[e] = !S.Wa ? (k == n ? 1.f : 0.f) : S.transA ? S.Wa[(size_t)k * S.lda + n] : S.Wa[(size_t)n * S.lda + k];
                } else if (k - S.Kapad < S.Kb) {
                    v[e] = S.alpha * (S.transB ? S.Wb[(size_t)(k - S.Kapad) * S.ldb + n] : S.Wb[(size_t)n * S.ldb + (k - S.Kapad)]);
                }
            }
            if (S.rscale) { const float r = S.rscale[n]; v = f32x4{v[0] * r, v[1] * r, v[2] * r, v[3] * r}; }
        }
        reinterpret_cast<f32x4*>(p.out)[idx] = v;
        return;
    }
    const size_t j = idx - nw4;                       // packed biases, one float per thread
    if (j >= (size_t)p.bias_total) return;
    int si = 0;
    while (si + 1 < p.nseg && (int)j >= p.seg[si + 1].bias_off) ++si;
    const NsPackSeg& S = p.seg[si];
    const int c = (int)j - S.bias_off;
    float bv = (c < S.N && S.b) ? S.bscale * S.b[c] : 0.f;
    if (c < S.N && S.b2) bv += S.b2scale * S.b2[c];
    if (c < S.N && S.rscale) bv *= S.rscale[c];
    if (c < S.N && S.rshift) bv += S.rshift[c];
    p.out[nw4 * 4 + j] = bv;
}

__global__ void ns_pack_side_kernel(NsPackArgs p) {
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;      // one f32x4 of one SIDE segment's block
    size_t base = 0;
    for (int si = 0; si < p.nseg; ++si) {
        const NsPackSeg& S = p.seg[si];
        if (S.type != NS_SIDE) continue;
        const size_t n4 = (size_t)NS_NW * S.steps * NS_NT * 64;
        if (idx >= base + n4) { base += n4; continue; }
        size_t q = idx - base;
        const int lane = (int)(q & 63); q >>= 6;
        const int t = (int)(q % NS_NT); q /= NS_NT;
        const int st = (int)(q % S.steps);
        const int w = (int)(q / S.steps);
        const int tpc = NS_NT / S.kc;
        const int n = 16 * (t % tpc) + (lane & 15);
        const int k0 = 16 * (S.kc * (w * S.steps + st) + t / tpc) + 4 * (lane >> 4);
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (n < S.N) {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int k = k0 + e;
                if (S.Wa) { if (k < S.Ka) v[e] = S.Wa[(size_t)n * S.lda + k]; }
                else if (k < S.Kb) v[e] = S.alpha * (S.transB ? S.Wb[(size_t)k * S.ldb + n] : S.Wb[(size_t)n * S.ldb + k]);   // d/dh: the second K part alone
            }
        }
        reinterpret_cast<f32x4*>(p.out + S.side_off)[idx - base] = v;
        return;
    }
}

__device__ __forceinline__ float ns_prior_theta(float z, int flat, float a1, float a2) {
    float u = 0.5f * (1.f + erff(z / 1.41421356237309515f));
    asm volatile("" : "+v"(u));                    // computed unconditionally: no branch on the loaded flag
    return (flat ? u : z) * a2 + a1;
}

// ------------------------------------------------------------------ the kernel
// MOVE: one ensemble half step in the launch.  Row k of the batch is walker S[k]: the prologue draws the
// stretch proposal q = c + z (s - c) from the complementary walkers (what linna_stretch_propose writes
// to memory), the network evaluates lnP(q), the finish applies the Metropolis test of
// linna_stretch_accept and updates coords / logp / naccept in place.  Same Philox counters, same
// arithmetic: bit-identical to the three-launch sequence.
// GRAD: lnP AND d lnP / d z in the launch (what torch.autograd.grad(lnP, x) yields at HMCSampler.py:32,40,48),
// for ReLU MLPs: every hidden layer records the sign bits of its output in LDS (one word per lane: the
// backward GEMM of the next layer has the same lane <-> (row, column) map), after the last layer the
// finish turns the output rows into d lnP / d out in place, and the SAME step loop runs on through the
// backward segments -- W^T in fragment order, streamed right behind the forward weights -- ending in the
// prior map's derivative.
// STORE: the forward pass of a training step in one launch.  The activations the backward needs (every op's
// output, every residual block's hidden h) are written to global memory from the epilogues with inline-asm
// stores: the compiler does not see them, so its counted vmcnt waits for the weight stream stay counted
// (stores only ever make the hardware counter read higher, i.e. the waits conservative).
// BF: the opt-in bf16 serving engine (linna_logprob_set_precision; MOVE 0 / 1, no GRAD, no STORE; MOVE 2 is the same engine
// in a kernel of its own, net_stream_slice_bf16_kernel).  The stream holds bf16
// weights (ns_pack_kernel, p.bf) and one step covers 32 k x 64 columns -- the same 4 KiB per wave and step, so the ring,
// its four 1-KiB loads and the counted waits keep their shape and a segment takes half the steps.  Activations stay fp32
// in LDS and are rounded to bf16 (nearest-even) where the A operand is read: two ds_read_b128 per step (8 k per lane).
// 16 rows: v_mfma_f32_16x16x32_bf16, one per column tile and step (lane group kq owns k 8 kq .. 8 kq + 7 of the step in
// A and B alike); 8 / 4 rows: v_mfma_f32_4x4x4_16b_bf16 with the CBSZ / ABID broadcast of the fp32 4x4x1 form, block b of
// the A read holding row set b & 3 and k chunk b >> 2 (8 k), two instructions (halves of the chunk) per (row set, chunk).
// The network input goes in as x_hi = bf16(x) at column c and x_lo = x - x_hi at column nin + c, and the first layer is
// packed [W | W] (ns_build_one): the input is not quantised to 8 bits.  Epilogues, the finish and the prior map are the
// fp32 kernel's.  SIDE segments are off in bf16 (K4 = false; the program builder plans none).
// BF + TRB: the opt-in bf16 training step (net_stream_train_bf16_kernel, 4-row engine).  The forward segments and the dX
// chain consume bf16 steps as above; the loss segment (the dense inverse covariance behind the last layer) stays an fp32
// run inside the same stream -- both formats move 4 KiB per wave and step, so only the consumer differs.  It is chosen
// once per run (begin_run: f32run); inside `step` the choice selects between two MFMA sequences and touches no memory.
// The kernel body is net_stream_body.inc, the text of the kernels below: the whole-network kernel, the opt-in bf16 slice
// evaluation (MOVE == 2 on a bf16 stream, described at net_stream_slice_bf16_kernel), and the opt-in bf16
// training step (linna_net_set_train_precision) -- the merged training launch (GRAD + STORE == 3, 4-row engine) on a bf16
// stream whose loss segment stays fp32, a kernel of its own rather than a net_stream_kernel specialisation.  (One text
// included twice instead of a device function both call: inlined into a wrapper, the same body compiles to other
// instructions for every existing instantiation.)
template <int R, int MOVE, bool GRAD, int STORE, int ROWS, bool BF = false>
__global__ __launch_bounds__(64 * NS_NW, 1) void net_stream_kernel(NsArgs a) {
#include "net_stream_body.inc"
}
template <int R, int MOVE, bool GRAD, int STORE, int ROWS, bool BF>
__global__ __launch_bounds__(64 * NS_NW, 1) void net_stream_train_bf16_kernel(NsArgs a) {
    static_assert(BF && GRAD && STORE == 3 && ROWS == 4 && MOVE == 0, "the bf16 training step only");
#include "net_stream_body.inc"
}
// BF + MOVE == 2: the ensemble slice move's evaluation on the bf16 serving engine (linna_slice_half_step,
// linna_logprob_eval_slice_points on a bf16 handle; 16-, 8- and 4-row engines).  Everything the slice move adds happens in
// fp32 before the network input reaches LDS (row list and device-side count, the fused set-up, the derived trial points)
// and in the finish; the input split, the bf16 steps and the epilogues are the serving engine's.  A kernel of its own
// for the same reason as the training step.
template <int R, int MOVE, bool GRAD, int STORE, int ROWS, bool BF>
__global__ __launch_bounds__(64 * NS_NW, 1) void net_stream_slice_bf16_kernel(NsArgs a) {
    static_assert(BF && !GRAD && STORE == 0 && MOVE == 2, "the bf16 slice evaluation only");
#define NS_BODY_SLICE_BF16
#include "net_stream_body.inc"
#undef NS_BODY_SLICE_BF16
}

// ---------------------------------------------------------------------------- host side: the program
struct NsProgram {
    std::vector<NsPackSeg> pack;
    std::vector<NsSeg> seg;
    int G = 0, LD = 0, kpad0 = 0, nout = 0, bias_total = 0;
    int Gstride = 0, nseg_f = 0, mask_slots = 0;            // G: forward steps; Gstride: forward + backward steps
    size_t lds_bytes = 0, lds_bytes_grad = 0, packed_floats = 0;   // LDS of the 16-row engine (lds_for: any engine)
    int dense = 0, u_col = 0, u_same = 0;                   // dense inverse covariance appended as the last segment
    int x0_keep = 0;                                        // an input-skip segment copies the network input later
    size_t side_f4 = 0;                                     // 16-byte vectors of all SIDE blocks
    bool bf = false;                                        // bf16 stream: 32 k per step, first layer [W | W] over [x_hi ; x_lo]
    int f32seg = -1;                                        // ... but for this segment, an fp32 run (the training step's loss)
    size_t lds_for(int rows, bool grad) const {
        size_t b = (size_t)(2 * rows * LD + ((bias_total + 3) & ~3)) * sizeof(float) + 128 + (x0_keep ? 4096 : 0);   // + [16] set rows, [16] den (STORE == 3), kept input rows
#ifdef NS_STAMPS
        b += NS_NW * 32 * 8;
#endif
        return b + (grad ? (size_t)mask_slots * 64 * NS_NW * sizeof(unsigned) : 0);
    }
    bool ok = false, grad_ok = false;                       // grad_ok: backward segments appended (ReLU MLPs)
    bool dxi_ok = false;                                    // the dX chain down to the input appended (NS_PROG_FWD_DXI)
    bool train_ok = false;                                  // forward + loss + dX chain (NS_PROG_TRAIN)
    std::vector<int> seg_op, seg_hidden;                    // forward segments: op index; 1 = the hidden h of a residual block
                                                            // (dX-chain program: 1 = d/dh of a residual block, else d/d(input) of the op)
};

static int ceil16(int k) { return (k + 15) & ~15; }
// steps of a segment in every wave's stream (a WIDE segment's second pass may be shorter: NsSeg::zext)
// zext < 0: the BALANCED triangular assignment of a 16-block lower-triangular factor -- wave w multiplies column block w
// (rows from 64 w) and then block 15 - w (rows from 64 (15 - w)): steps - 4 w and steps - 4 (15 - w) steps, 2 steps - 60 in
// every wave
static int ns_seg_steps(const NsSeg& s) {
    if (s.type == NS_WIDE && s.zext < 0) return 2 * s.steps - 60;
    return s.type == NS_WIDE && s.zext > 0 ? s.steps + (s.passes - 1) * s.zext : s.steps * s.passes;
}
static std::atomic<int> g_dense_tri{-1};
static int ns_dense_tri_resolved() {
    int m = g_dense_tri.load(std::memory_order_relaxed);
    if (m < 0) {
        const char* env = getenv("LINNA_DENSE_TRI");
        int v = env ? atoi(env) : 2;
        if (v < 0 || v > 2) v = 2;
        int expect = -1;
        g_dense_tri.compare_exchange_strong(expect, v);
        m = g_dense_tri.load(std::memory_order_relaxed);
    }
    return m;
}
int net_stream_dense_tri(int mode) {
    const int prev = ns_dense_tri_resolved();
    if (mode >= 0 && mode <= 2) g_dense_tri.store(mode);
    return prev;
}

// Translate the op list into segments; ok = false when something does not fit this kernel.  The builder's modes (the
// programs of NsKind are built from these in ns_build_kind):
enum { NS_PROG_FWD = 0, NS_PROG_FWD_NOGRAD = 1, NS_PROG_DX = 2, NS_PROG_DX_INPUT = 3, NS_PROG_FWD_DENSE = 4, NS_PROG_FWD_DXI = 5,
       NS_PROG_TRAIN = 6 };   // TRAIN: forward + loss segment (FWD_DENSE with the loss's inverse covariance) followed by the dX chain down to op 1
// mode NS_PROG_DX: the dX chain of a training step as a program of its own (linna_net_backward's order): the rows are
// d loss / d output, the segments run over the transposed weights from the last op down to op 1 (NS_PROG_DX_INPUT: op 0).
// A residual block y = relu(0.1 (W2 h + b2) + Ws x), h = relu(W1 x + b1) comes back as  dh = 0.1 (dy W2) [h > 0],
// written behind dy, and ONE GEMM over [dy ; dh] with [Ws^T | W1^T]; the gate of every output (the stored forward
// activation) is applied by the kernel's STORE == 2 epilogue.
// mode NS_PROG_FWD_DENSE: the forward program with the output map (d = raw * cscale + cshift) folded into the last
// layer's weights and bias, and the dense inverse covariance appended as one more bias-free segment U = d S -- the
// Gaussian log-likelihood (util.py:953-955) with a dense covariance then needs no GEMM launch of its own.
// k4: SPLIT segments of <= 32 columns become SIDE segments where they fit (see NsPackArgs): the kernel's K4 path, i.e. the
// 16-row engine of the programs ns_side names.
// bf: the bf16 serving program (NS_PROG_FWD_NOGRAD only, no dense segment, no SIDE segments): a step is 32 k, and the
// first layer (a plain linear map) is [W | W] over K' = 2 nin -- its input rows are x_hi = bf16(x) and x_lo = x - x_hi.
static NsProgram ns_build_one(const linna_layer_t* layers, int nl, int in_size, int mode, const NsDense* dn = nullptr,
                              bool k4 = false, bool bf = false) {
    NsProgram p;
    if (bf && ((mode != NS_PROG_FWD_NOGRAD && mode != NS_PROG_TRAIN) || (mode == NS_PROG_FWD_NOGRAD && dn) || k4)) return p;
    const bool allow_grad = mode == NS_PROG_FWD, dx_prog = mode == NS_PROG_DX || mode == NS_PROG_DX_INPUT;
    const bool train = mode == NS_PROG_TRAIN;
    if ((mode == NS_PROG_FWD_DENSE || train) && (!dn || !dn->S)) return p;
    if (nl < 1 || in_size < 1 || in_size > 256) return p;
    // 1. linear maps: [Wa | alpha Wb] over K = [Kapad ; Kb], N outputs, written to dst_col (same_buf: into the input's buffer)
    struct Lin { const float* Wa; int lda, Ka, Kapad; const float* Wb; int ldb, Kb; float alpha; const float* b; float bscale;
                 int N, relu, dst_col; bool same_buf; int transA = 0; int force_wide = 0; int mask_apply_of = -1; int op = -1;
                 int transB = 0; const float* rscale = nullptr; const float* rshift = nullptr;
                 const float* b2 = nullptr; float b2scale = 0.f; int x0_col = 0; };
    std::vector<Lin> lins;
    int width = in_size;
    // NS_PROG_FWD_DXI: the forward program followed by the dX chain down to the network input in ONE stream -- lnP and
    // d lnP / d z in one launch for ANY network (residual blocks, SPLIT segments): the forward segments store their
    // activations, the backward segments gate on them (the kernel's GRAD + STORE == 2 instantiation)
    const bool fwd_dxi = mode == NS_PROG_FWD_DXI;
    for (int i = 0; i < nl && (dx_prog || fwd_dxi || train); ++i) {      // shape checks as in the forward program
        const linna_layer_t& l = layers[i];
        if (l.K != width || l.N < 1 || l.N > 1024 || l.K > 1024) return p;
        if (l.op == LINNA_OP_LINEAR) { if (l.alpha != 1.f) return p; }
        else if (l.op == LINNA_OP_RESBLOCK) { if (l.C < 1 || l.C > 64 || (!l.Ws && l.K != l.N)) return p; }
        else return p;
        width = l.N;
    }
    auto push_dx = [&](int first) {
      for (int i = nl - 1; i >= first; --i) {
        const linna_layer_t& l = layers[i];
        const int npad = ceil16(l.N);
        if (l.op == LINNA_OP_LINEAR) {
            Lin B{l.W, (l.K + 3) & ~3, l.N, npad, nullptr, 0, 0, 0.f, nullptr, 0.f, l.K, 0, 0, false};
            B.transA = 1; B.op = i;
            lins.push_back(B);
        } else {
            Lin A{nullptr, 0, 0, 0, l.W2, (l.C + 3) & ~3, l.N, 0.1f, nullptr, 0.f, l.C, 0, npad, true};     // dh behind dy
            A.transB = 1; A.op = i;
            lins.push_back(A);
            Lin B{l.Ws, (l.K + 3) & ~3, l.N, npad, l.W1, (l.K + 3) & ~3, l.C, 1.f, nullptr, 0.f, l.K, 0, 0, false};
            B.transA = 1; B.transB = 1; B.op = i;
            lins.push_back(B);
        }
      }
    };
    if (dx_prog) push_dx(mode == NS_PROG_DX_INPUT ? 0 : 1);
    width = in_size;
    for (int i = 0; i < nl && !dx_prog; ++i) {
        const linna_layer_t& l = layers[i];
        if (l.K != width && l.op != LINNA_OP_INSKIP) return p;
        if (l.op == LINNA_OP_LINEAR) {
            if (l.alpha != 1.f || l.N < 1 || l.N > 1024) return p;
            lins.push_back(Lin{l.W, (l.K + 3) & ~3, l.K, ceil16(l.K), nullptr, 0, 0, 0.f, l.b, 1.f, l.N, l.relu, 0, false});
            lins.back().op = i;
        } else if (l.op == LINNA_OP_RESBLOCK) {
            if (l.C < 1 || l.C > 64 || l.N < 1 || l.N > 1024 || (!l.Ws && l.K != l.N)) return p;
            const int inpad = ceil16(l.K);
            lins.push_back(Lin{l.W1, (l.K + 3) & ~3, l.K, inpad, nullptr, 0, 0, 0.f, l.b1, 1.f, l.C, 1, inpad, true});   // h behind x
            lins.back().op = i;
            lins.push_back(Lin{l.Ws, (l.K + 3) & ~3, l.K, inpad, l.W2, (l.C + 3) & ~3, l.C, 0.1f, l.b2, 0.1f, l.N, 1, 0, false});
            lins.back().op = i;
        } else if (l.op == LINNA_OP_INSKIP) {
            // out = last(h) + alpha (x0 Wl^T + bl) (nn.py:195): the last layer becomes ONE GEMM over [h ; x0] with [W | alpha Wl]
            // and bias b + alpha bl; x0 (the network input, kept in LDS) is copied behind h before the segment runs
            if (i != nl - 1 || lins.empty() || l.K != in_size || l.N != width || in_size > 64 || mode == NS_PROG_FWD) return p;
            Lin& last = lins.back();
            if (last.Wb || last.same_buf || last.relu || !last.Wa) return p;
            last.Wb = l.W; last.ldb = (l.K + 3) & ~3; last.Kb = l.K; last.alpha = l.alpha;
            last.b2 = l.b; last.b2scale = l.alpha; last.x0_col = last.Kapad;
            p.x0_keep = 1;
            continue;
        } else {
            return p;
        }
        width = l.N;
    }
    if (dx_prog) in_size = layers[nl - 1].N;                   // the rows of this program are d loss / d output
    if (lins.empty() || lins.back().relu || (int)lins.size() > NS_MAXSEG) return p;
    if (bf) {                                               // [x_hi ; x_lo]: the first layer twice, no padding between the halves
        Lin& f = lins[0];
        if (f.Wb || f.same_buf || f.transA || !f.Wa || f.Ka != in_size || f.x0_col) return p;
        f.Kapad = in_size; f.Wb = f.Wa; f.ldb = f.lda; f.Kb = f.Ka; f.alpha = 1.f;
    }
    if (mode == NS_PROG_FWD_DENSE || train) {
        Lin& last = lins.back();
        if (last.Wb || last.same_buf || last.dst_col) return p;               // the last op must be a plain linear layer
        last.rscale = dn->cscale; last.rshift = dn->cshift;
        const int no = last.N, npad = ceil16(no);
        if ((int)lins.size() + 1 > NS_MAXSEG) return p;
        const bool behind = no <= 256;                                          // SPLIT: U behind d in the same buffer
        Lin Q{dn->S, dn->lds, no, npad, nullptr, 0, 0, 0.f, nullptr, 0.f, no, 0, behind ? npad : 0, behind};
        Q.op = nl;
        // factored: the matrix is L (S = L L^T, not symmetric) and the segment must produce d L: U_n = sum_k d_k L[k][n] -- the
        // pack kernel reads it transposed (the row-dot GEMM of the layered path reads S[k][n] as it is)
        if (dn->factored) Q.transA = 1;
        lins.push_back(Q);
        p.dense = 1; p.u_col = Q.dst_col; p.u_same = behind ? 1 : 0;
    }
    const int nfwd = (int)lins.size();
    // k per step of segment i: 32 in a bf16 stream, but for the training step's loss segment (the dense inverse covariance
    // behind the last layer), an fp32 run inside it
    const int f32seg = bf && train ? nfwd - 1 : -1;
    auto seg_ks = [&](int i) { return bf && i != f32seg ? 32 : 16; };
    if (fwd_dxi) {
        if (in_size > 64 || lins.back().N > 64) return p;      // (prologue / turnaround constants are held for <= 64 columns)
        push_dx(0);
        if ((int)lins.size() > NS_MAXSEG) return p;
    }
    if (train) {                                               // the turnaround works on the rows in LDS: any width
        if (nl < 2) return p;
        push_dx(1);
        if ((int)lins.size() > NS_MAXSEG) return p;
    }
    // Backward (d lnP / d z) for plain ReLU MLPs whose hidden layers come out as WIDE segments: the backward
    // GEMM of layer l is a forward-shaped segment over W_l^T (contraction N_l, K_l outputs); for l >= 1 it is
    // forced WIDE so that its lane <-> (row, column) map equals that of the layer whose sign bits it applies.
    bool want_grad = allow_grad && in_size <= 64 && lins.back().N <= 64 && 2 * nfwd <= NS_MAXSEG;
    for (int i = 0; i < nfwd && want_grad; ++i) {
        const Lin& L = lins[i];
        if (L.Wb || L.same_buf || L.dst_col || !L.Wa) want_grad = false;
        if (i < nfwd - 1 && (!L.relu || L.N <= 256)) want_grad = false;       // hidden layers must be WIDE (N > 256)
    }
    if (want_grad) {
        for (int i = nfwd - 1; i >= 0; --i) {
            const Lin F = lins[i];
            Lin Bk{F.Wa, F.lda, F.N, ceil16(F.N), nullptr, 0, 0, 0.f, nullptr, 0.f, F.Ka, 0, 0, false};
            Bk.transA = 1; Bk.force_wide = i >= 1; Bk.mask_apply_of = i - 1;
            lins.push_back(Bk);
        }
    }

    // 2. segment shapes.  SPLIT when it must write into its own input buffer (h of a residual block) or when
    //    splitting K over the idle waves saves at least three steps; WIDE otherwise.
    int bias_off = 0, G = 0, zero_off = -1, zero_pad = 0;
    std::vector<int> in_ext(lins.size());
    for (size_t i = 0; i < lins.size(); ++i) {
        const Lin& L = lins[i];
        const int KS = seg_ks((int)i);
        const int ksteps = KS == 32 ? (L.Kapad + L.Kb + 31) / 32 : (L.Kapad + ceil16(L.Kb)) / 16;
        NsSeg s; NsPackSeg q;
        std::memset(&s, 0, sizeof(s));
        s.relu = L.relu; s.dst_col = L.dst_col; s.bias_off = bias_off;
        const int passes = (L.N + 511) / 512;
        int ncg = L.N <= 64 ? 1 : L.N <= 128 ? 2 : L.N <= 256 ? 4 : 0;
        const int split_steps = ncg ? (ksteps + NS_NW / ncg - 1) / (NS_NW / ncg) : 0;
        const bool split = ncg && !L.force_wide && (L.same_buf || split_steps + 3 <= ksteps * passes);
        if (L.same_buf && !ncg) return p;
        const int kc = L.N <= 16 ? 4 : L.N <= 32 ? 2 : 1;
        const int side_steps = (ksteps + NS_NW * kc - 1) / (NS_NW * kc);
        // (never the first segment nor the last forward one: the kernel runs a SIDE segment between two runs of the step loop;
        // kc = 1, <= 64 columns: the SPLIT mapping itself, run out of the stream -- 250 -> 64 is two steps per wave)
        // ... and, in the one-launch gradient, d/dh of a residual block (0.1 dy W2 gated by h: 500 / 250 / 125 -> 16 / 32 / 64,
        // the second K part alone, read transposed): one SIDE step each instead of 4 / 2 / 1 SPLIT steps and a SPLIT boundary
        // (the LAST forward segment too where nothing follows it in the launch -- serving programs without a backward half:
        // ChtoModelv2's 33 -> 33 last layer is one SIDE step instead of a three-step WIDE run)
        const bool last_ok = (int)i == nfwd - 1 && !want_grad && !fwd_dxi && !train && !dx_prog;
        const bool side_fwd = ((int)i < nfwd - 1 || last_ok) && !L.Wb && !L.transA && L.Wa;
        const bool side_bwd = fwd_dxi && (int)i > nfwd && !L.Wa && L.Wb && L.transB && L.Kapad == 0 && !L.relu;
        const bool side_pays = split || (side_fwd && !L.force_wide && side_steps < ksteps * passes);   // (a short WIDE run of <= 64 columns)
        const bool side = k4 && side_pays && ncg == 1 && side_steps <= 2 && i > 0 && (side_fwd || side_bwd) && p.seg.back().type != NS_SIDE &&
                          !L.rscale && !L.rshift && !L.b2 && !L.x0_col;
        if (side) {
            s.type = NS_SIDE; s.steps = side_steps; s.passes = 1; s.kslice = 16 * kc * s.steps;
            s.ncg_log2 = 0; s.kcl = kc == 4 ? 2 : kc == 2 ? 1 : 0;
            s.zext = 64;
            in_ext[i] = NS_NW * s.kslice;
            q.bias_pad = 64; q.ncg = 1;
        } else if (split) {
            s.type = NS_SPLIT; s.steps = split_steps; s.passes = 1; s.kslice = KS * s.steps;
            s.ncg_log2 = ncg == 1 ? 0 : ncg == 2 ? 1 : 2;
            s.zext = 64 * ncg;
            in_ext[i] = (NS_NW / ncg) * s.kslice;
            q.bias_pad = 64 * ncg; q.ncg = ncg;
        } else {
            s.type = NS_WIDE; s.steps = ksteps; s.passes = passes;
            in_ext[i] = KS * ksteps;
            q.bias_pad = 512 * passes; q.ncg = 1;
        }
        q.Wa = L.Wa; q.lda = L.lda; q.Ka = L.Ka; q.Kapad = L.Kapad; q.Wb = L.Wb; q.ldb = L.ldb; q.Kb = L.Kb; q.alpha = L.alpha;
        q.b = L.b; q.bscale = L.bscale; q.N = L.N; q.type = s.type; q.steps = s.steps; q.passes = s.passes; q.bias_off = bias_off;
        q.transA = L.transA; q.transB = L.transB; q.rscale = L.rscale; q.rshift = L.rshift; q.b2 = L.b2; q.b2scale = L.b2scale;
        q.kc = side ? kc : 1; q.side_off = 0;
        s.x0_col = L.x0_col; s.x0_n = L.x0_col ? ceil16(L.Kb) : 0;
        if (L.transA && !dx_prog) {                                     // backward segments have no bias: ONE shared block of zeros
            if (zero_off < 0) { zero_off = bias_off; zero_pad = 0; }
            s.bias_off = q.bias_off = zero_off;
            const int grow = std::max(0, q.bias_pad - zero_pad);
            zero_pad += grow; q.bias_pad = grow;            // (the first backward segment's record carries the block; later ones extend it)
        }
        bias_off += q.bias_pad;
        // the Cholesky factor of a dense inverse covariance (NsDense::factored) is lower triangular: in the second pass (columns
        // >= 512) the rows k < 512 are zero -- that pass starts at k = 512 (bit-identical: the skipped products are zeros)
        // tri = 2 and exactly 16 column blocks (960 < nout <= 1024): the balanced assignment instead (ns_seg_steps) -- the zero
        // rows of EVERY 64-column block are skipped, not only those of the second pass, and every wave runs the same number
        // of steps: 66 instead of 94 at nout = 1000
        if (dn && dn->tri > 0 && s.type == NS_WIDE && dn->factored && L.Wa == dn->S && passes == 2 && ksteps > 32 && !train) {
            if (dn->tri == 2 && (L.N + 63) / 64 == 16 && ksteps > 60) s.zext = -1;
            else { s.kslice = 512; s.zext = ksteps - 32; }
        }
        q.koff2 = s.type == NS_WIDE ? (s.zext < 0 ? -1 : s.kslice) : 0;
        if (!side) G += ns_seg_steps(s);           // (a SIDE segment is not part of the weight stream)
        p.seg.push_back(s); p.pack.push_back(q);
    }
    if (want_grad) {
        // sign-bit slots: one per pass of every hidden forward segment; the backward segment of layer i+1 applies them
        int slot = 0;
        for (int i = 0; i < nfwd - 1; ++i) {
            if (p.seg[i].type != NS_WIDE) { want_grad = false; break; }
            p.seg[i].mask_store = 1 + slot;
            slot += p.seg[i].passes;
        }
        for (size_t j = nfwd; j < lins.size() && want_grad; ++j) {
            const int of = lins[j].mask_apply_of;
            if (of < 0) continue;
            if (p.seg[j].type != NS_WIDE || p.seg[j].passes != p.seg[of].passes) { want_grad = false; break; }
            p.seg[j].mask_apply = p.seg[of].mask_store;
        }
        if (want_grad) p.mask_slots = slot;
        else {   // drop the backward half again
            for (size_t j = lins.size(); j-- > (size_t)nfwd;) { G -= ns_seg_steps(p.seg[j]); bias_off -= p.pack[j].bias_pad; }
            p.seg.resize(nfwd); p.pack.resize(nfwd); lins.resize(nfwd); in_ext.resize(nfwd);
            for (int i = 0; i < nfwd; ++i) p.seg[i].mask_store = 0;
        }
    }
    int Gf = 0;
    for (int i = 0; i < nfwd; ++i) if (p.seg[i].type != NS_SIDE) Gf += ns_seg_steps(p.seg[i]);

    // 3. every column a segment reads must have been WRITTEN (finite; zero where the weights are zero):
    //    track the defined prefix [0, def) of the current buffer and widen the zero fill of the last
    //    SPLIT writer (or of the prologue) where a consumer reads further.
    p.kpad0 = in_ext[0];
    int def = p.kpad0, writer = -1;                         // writer: segment whose write ends at `def` (-1 prologue, -2 fixed)
    int maxext = 64;
    for (size_t i = 0; i < p.seg.size(); ++i) {
        NsSeg& s = p.seg[i];
        if (in_ext[i] > def) {
            if (writer == -1) p.kpad0 = def = in_ext[i];
            else if (writer >= 0) { NsSeg& w = p.seg[writer]; w.zext = in_ext[i] - w.dst_col; def = in_ext[i]; }
            else return p;
        }
        maxext = std::max(maxext, in_ext[i]);
        if (s.type == NS_WIDE) {
            if (s.dst_col != 0) return p;
            def = 512 * s.passes; writer = -2;
            maxext = std::max(maxext, def);
        } else {
            if (s.dst_col > def) return p;
            if (s.dst_col == 0) def = s.zext;               // overwrites its input from column 0
            else def = std::max(def, s.dst_col + s.zext);
            writer = (int)i;
        }
    }
    for (const NsSeg& s : p.seg) if (s.type != NS_WIDE) maxext = std::max(maxext, s.dst_col + s.zext);
    if (p.kpad0 > (dx_prog ? 1024 : bf ? 512 : 256)) return p;
    p.bf = bf; p.f32seg = f32seg;
    p.nout = lins[nfwd - 1].N;
    p.G = Gf; p.Gstride = G; p.nseg_f = nfwd; p.grad_ok = want_grad;
    for (size_t i = 0; i < lins.size(); ++i) { p.seg_op.push_back(lins[i].op); p.seg_hidden.push_back(lins[i].same_buf ? 1 : 0); }
    p.dxi_ok = fwd_dxi;
    p.train_ok = train;
    p.bias_total = bias_off;
    p.LD = std::max(((maxext + 63) & ~63) + 4, 516);        // >= 516: SPLIT partials need [8][rows][64] floats in one buffer
    if (bias_off > 3 * 64 * NS_NW * 4) return p;            // BMAX rounds of float4 per thread
    p.lds_bytes = (size_t)(2 * NS_ROWS * p.LD + ((bias_off + 3) & ~3)) * sizeof(float) + 128 + (p.x0_keep ? 4096 : 0);
#ifdef NS_STAMPS
    p.lds_bytes += NS_NW * 32 * 8;
#endif
    if (p.lds_bytes > (size_t)NS_LDS_BYTES) return p;
    p.lds_bytes_grad = p.lds_bytes + (size_t)p.mask_slots * 64 * NS_NW * sizeof(unsigned);
    if (p.grad_ok && p.lds_bytes_grad > (size_t)NS_LDS_BYTES) return p;   // (never for the eligible shapes)
    int nrun = 0;
    for (const NsSeg& s : p.seg) nrun += s.passes;
    if (nrun > NS_MAXRUN) return p;
    p.packed_floats = (size_t)NS_NW * G * NS_NT * 256 + (size_t)((bias_off + 3) & ~3);
    for (size_t i = 0; i < p.seg.size(); ++i)
        if (p.seg[i].type == NS_SIDE) {            // blocks of their own behind the biases
            p.seg[i].side_off = p.pack[i].side_off = (int)p.packed_floats;
            p.packed_floats += (size_t)NS_NW * p.seg[i].steps * NS_NT * 256;
            p.side_f4 += (size_t)NS_NW * p.seg[i].steps * NS_NT * 64;
        }
    p.ok = true;
    return p;
}

// Engine for a batch of B rows: the fewest rows per workgroup that still fit the batch into one workgroup per CU
// (linna_engine_rows forces one for tests and measurements; LINNA_NS_ROWS in the environment sets the initial value,
// read ONCE -- the launch path reads an atomic, not the environment).
static std::atomic<int> g_forced_rows{-1};
static int ns_forced_rows_resolved() {             // -1 (never read) -> the environment's value, once
    int forced = g_forced_rows.load(std::memory_order_relaxed);
    if (forced < 0) {
        const char* const env = getenv("LINNA_NS_ROWS");
        const int v = env ? atoi(env) : 0;
        forced = (v == 4 || v == 8 || v == 16) ? v : 0;
        int expect = -1;
        g_forced_rows.compare_exchange_strong(expect, forced);
        forced = g_forced_rows.load(std::memory_order_relaxed);
    }
    return forced;
}
int net_stream_force_rows(int rows) {
    if (rows != 0 && rows != 4 && rows != 8 && rows != 16) return -1;
    (void)ns_forced_rows_resolved();               // the environment's value is what `prev = engine_rows(4); ...; engine_rows(prev)` must restore
    return g_forced_rows.exchange(rows);
}
int net_stream_rows(int B) {
    const int forced = ns_forced_rows_resolved();
    if (forced) return forced;
    static int ncu = 0;
    if (!ncu) {
        int dev = 0; hipDeviceProp_t pr;
        ncu = (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&pr, dev) == hipSuccess && pr.multiProcessorCount > 0)
                  ? pr.multiProcessorCount : 256;
    }
    return B <= 4 * ncu ? 4 : B <= 8 * ncu ? 8 : 16;
}

// SIDE segments (the kernel's K4 path) run on the 16-row engine of the serving programs and the one-launch gradient.  In the
// gradient's forward half they were measured slower in round 3 (with the activations stored for the gates); with the gates
// as sign bits in LDS and the per-segment tables read through the kernel-argument segment (without that the instantiation
// spilled 2.5 KB per lane): 151.4 -> 148.7 us at ChtoModelv2(33,33), 4096 chains (NOTES R4).  Not in bf16.
static bool ns_side(NsKind kind, int rows) {
    return rows == 16 && (kind == NS_SERVE || kind == NS_SERVE_DENSE || kind == NS_GRAD_INPUT);
}

static NsProgram ns_build_kind(NsKind kind, const linna_layer_t* layers, int nl, int in_size, const NsDense* dn, bool side) {
    NsProgram p;
    switch (kind) {
    case NS_SERVE: case NS_STORE:
        p = ns_build_one(layers, nl, in_size, NS_PROG_FWD, nullptr, side);
        if (!p.ok) p = ns_build_one(layers, nl, in_size, NS_PROG_FWD_NOGRAD, nullptr, side);   // the backward half may be what did not fit
        break;
    case NS_SERVE_DENSE: case NS_TRAIN_FWD: p = ns_build_one(layers, nl, in_size, NS_PROG_FWD_DENSE, dn, side); break;
    case NS_SERVE_BF16: p = ns_build_one(layers, nl, in_size, NS_PROG_FWD_NOGRAD, dn, false, true); break;
    case NS_DX: p = ns_build_one(layers, nl, in_size, NS_PROG_DX); break;
    case NS_DX_INPUT: p = ns_build_one(layers, nl, in_size, NS_PROG_DX_INPUT); break;
    case NS_GRAD_INPUT: p = ns_build_one(layers, nl, in_size, NS_PROG_FWD_DXI, nullptr, side); break;
    case NS_TRAIN_STEP: p = ns_build_one(layers, nl, in_size, NS_PROG_TRAIN, dn); break;
    case NS_TRAIN_STEP_BF16: p = ns_build_one(layers, nl, in_size, NS_PROG_TRAIN, dn, false, true); break;
    }
    // the SIDE program where it fits, the plain one otherwise
    if (side && !(p.ok && (kind != NS_GRAD_INPUT || p.dxi_ok))) return ns_build_kind(kind, layers, nl, in_size, dn, false);
    return p;
}
// Kernel-configuration cache: a program is a pure function of the op list (shapes AND parameter pointers:
// the pack descriptors carry them), the program kind, the engine (SIDE segments or not) and the dense descriptor, so it
// is built once and looked up by those bytes on every later launch -- no segment planning, no vector allocation on the
// launch path.  Entries live for the life of the library (a handful per network; the table is cleared if it ever reaches
// 256 entries).  A lookup hands out shared ownership: a clear by a later lookup never frees a program a caller still
// holds.  rows: the engine that runs it (0: any; no SIDE segments).
typedef std::shared_ptr<const NsProgram> NsProgramRef;
static NsProgramRef ns_program(NsKind kind, const linna_layer_t* layers, int nl, int in_size, const NsDense* dn, int rows) {
    static std::mutex mu;
    static std::unordered_map<std::string, NsProgramRef> cache;
    const bool side = ns_side(kind, rows);
    std::string key;
    key.reserve((size_t)nl * sizeof(linna_layer_t) + 64);
    key.append(reinterpret_cast<const char*>(layers), (size_t)nl * sizeof(linna_layer_t));
    const int hdr[4] = {nl, in_size, (int)kind, side ? 1 : 0};
    key.append(reinterpret_cast<const char*>(hdr), sizeof(hdr));
    if (dn) {                                               // field by field: the struct has padding bytes
        const void* const ptrs[3] = {dn->S, dn->cscale, dn->cshift};
        key.append(reinterpret_cast<const char*>(ptrs), sizeof(ptrs));
        key.append(reinterpret_cast<const char*>(&dn->lds), sizeof(int));
        key.append(reinterpret_cast<const char*>(&dn->factored), sizeof(int));
        key.append(reinterpret_cast<const char*>(&dn->tri), sizeof(int));
    }
    std::lock_guard<std::mutex> lock(mu);
    auto it = cache.find(key);
    if (it != cache.end()) return it->second;
    if (cache.size() >= 256) cache.clear();
    NsProgramRef p = std::make_shared<const NsProgram>(ns_build_kind(kind, layers, nl, in_size, dn, side));
    cache.emplace(std::move(key), p);
    return p;
}

// columns of what segment i of a one-launch forward + backward program (NS_GRAD_INPUT, NS_TRAIN_STEP) writes: the hidden h
// of a residual block, a forward op's output, or (the backward half) d/d(op input)
static int ns_seg_cols(const NsProgram& p, const linna_layer_t* layers, int i) {
    const linna_layer_t& l = layers[p.seg_op[i]];
    return p.seg_hidden[i] ? l.C : i < p.nseg_f ? l.N : l.K;
}
// The gates of a one-launch backward half (NS_GRAD_INPUT, NS_TRAIN_STEP): what the backward gates on is the SIGN of a
// forward activation, and the workgroup that needs it is the one that computed it -- one bit per (row, column) in LDS
// behind the program's own LDS (NsArgs::nbw, bits_off).  gbit[i]: the first bit column of forward segment i's signs (-1:
// no gate asks for them; every tensor rounded up to 64 columns); mbit[i]: the columns backward segment i gates on (-1:
// none).  ok = false when a gate has no producer.
struct NsGates {
    int gbit[NS_MAXSEG], mbit[NS_MAXSEG];
    int ncols = 0;
    bool ok = true;
    size_t lds0 = 0, lds = 0;                               // the program's LDS (8-byte aligned), and with the bits
};
static NsGates ns_gates(const NsProgram& p, const linna_layer_t* layers, int nl, int rows) {
    NsGates g;
    for (int i = 0; i < NS_MAXSEG; ++i) g.gbit[i] = g.mbit[i] = -1;
    for (int i = 0; i < p.nseg_f; ++i) {                    // forward: keep the signs a gate will ask for
        const int op = p.seg_op[i];
        if (op >= nl || (!p.seg_hidden[i] && op == nl - 1)) continue;   // the loss segment and the network output gate nothing
        g.gbit[i] = g.ncols;
        g.ncols += (ns_seg_cols(p, layers, i) + 63) & ~63;
    }
    for (int i = p.nseg_f; i < (int)p.seg.size(); ++i) {
        // d/dh of a residual block: gated by its h; d/d(input of op): by the producing op's output, if it went through a ReLU
        const int op = p.seg_op[i];
        const bool hidden = p.seg_hidden[i] != 0;
        if (!hidden && !(op > 0 && (layers[op - 1].op == LINNA_OP_RESBLOCK || layers[op - 1].relu))) continue;
        const int src = hidden ? op : op - 1;
        for (int j = 0; j < p.nseg_f; ++j)
            if (p.seg_op[j] == src && (p.seg_hidden[j] != 0) == hidden) g.mbit[i] = g.gbit[j];
        if (g.mbit[i] < 0) g.ok = false;
    }
    g.lds0 = (p.lds_for(rows, true) + 7) & ~(size_t)7;
    g.lds = g.lds0 + (size_t)rows * (g.ncols / 32) * sizeof(unsigned);
    return g;
}

// why the bf16 program does not exist for this network (null: it does)
static const char* ns_bf16_refusal(const NsProgram& p, const linna_layer_t* layers, int nl, int in_size) {
    int width = 0;
    for (int i = 0; i < nl; ++i) width = std::max(width, std::max(layers[i].N, layers[i].op == LINNA_OP_RESBLOCK ? layers[i].C : 0));
    if (in_size > 256) return "more than 256 network inputs: outside the whole-network kernel";
    if (width > 1024) return "a layer wider than 1024: outside the whole-network kernel";
    if (nl < 1 || layers[0].op != LINNA_OP_LINEAR) return "the first op is not a linear layer (the bf16 input split needs one)";
    if (!p.ok) return "the network does not fit the bf16 program of the whole-network kernel";
    return nullptr;
}
NsPlan net_stream_plan(NsKind kind, const linna_layer_t* layers, int nl, int in_size, const NsDense* dn) {
    const NsProgramRef pref = ns_program(kind, layers, nl, in_size, dn, 0);
    const NsProgram& p = *pref;
    NsPlan r{p.ok, p.packed_floats, p.grad_ok, nullptr};
    if (kind == NS_TRAIN_STEP) r.ok = p.ok && p.train_ok;
    if (kind == NS_TRAIN_STEP_BF16) {
        r.why = ns_bf16_refusal(p, layers, nl, in_size);
        if (!r.why && !p.train_ok) r.why = "the network has no merged training step (one layer only)";
        r.ok = r.why == nullptr;
    }
    if (kind == NS_GRAD_INPUT) {
        r.ok = p.ok && p.dxi_ok && ns_gates(p, layers, nl, NS_ROWS).lds <= (size_t)NS_LDS_BYTES;
        // one copy serves every engine: the 16-row one reads the SIDE program
        r.packed_floats = std::max(r.packed_floats, ns_program(kind, layers, nl, in_size, dn, 16)->packed_floats);
    }
    if (kind == NS_SERVE_BF16) { r.why = ns_bf16_refusal(p, layers, nl, in_size); r.ok = r.why == nullptr; }
    return r;
}

// Text form of a program (tests, diagnostics): one line per segment, "type steps passes ncg kc dst_col zext".
int net_stream_describe(NsKind kind, const linna_layer_t* layers, int nl, int in_size, const NsDense* dn, int rows, char* buf, size_t n) {
    const NsProgramRef pref = ns_program(kind, layers, nl, in_size, dn, rows);
    const NsProgram& p = *pref;
    std::string out = p.ok ? "ok" : "not eligible";
    char line[160];
    snprintf(line, sizeof line, " G %d Gstride %d nseg_f %d LD %d kpad0 %d packed_floats %zu grad %d\n", p.G, p.Gstride, p.nseg_f, p.LD,
             p.kpad0, p.packed_floats, (int)p.grad_ok);
    out += line;
    for (size_t i = 0; p.ok && i < p.seg.size(); ++i) {
        const NsSeg& g = p.seg[i];
        snprintf(line, sizeof line, "%s steps %d passes %d ncg %d kc %d dst %d zext %d N %d\n",
                 g.type == NS_WIDE ? "WIDE" : g.type == NS_SPLIT ? "SPLIT" : "SIDE", g.steps, g.passes, 1 << g.ncg_log2, 1 << g.kcl, g.dst_col,
                 g.zext, p.pack[i].N);
        out += line;
    }
    if (p.ok && kind == NS_GRAD_INPUT) {            // the one-launch gradient: its LDS with the sign-bit matrix, on the 16-row engine
        const NsGates g = ns_gates(p, layers, nl, NS_ROWS);
        snprintf(line, sizeof line, "lds %zu of %d bytes with %d sign-bit columns: %s\n", g.lds, NS_LDS_BYTES, g.ncols,
                 g.lds <= (size_t)NS_LDS_BYTES && p.dxi_ok ? "one launch" : "layered");
        out += line;
    }
    if (buf && n) { snprintf(buf, n, "%s", out.c_str()); }
    return p.ok ? (int)p.seg.size() : 0;
}

int launch_net_stream_pack(NsKind kind, const linna_layer_t* layers, int nl, int in_size, float* packed, int rows, const NsDense* dn,
                           hipStream_t s) {
    const NsProgramRef pref = ns_program(kind, layers, nl, in_size, dn, rows);
    const NsProgram& p = *pref;
    if (!p.ok) { set_error("net_stream: network not eligible"); return LINNA_ERR_UNSUPPORTED; }
    NsPackArgs a;
    ::memset(static_cast<void*>(&a), 0, sizeof(a));
    a.nseg = (int)p.seg.size(); a.G = p.Gstride; a.bias_total = p.bias_total; a.out = packed;
    a.small = rows < 16;
    a.bf = p.bf ? 1 : 0; a.f32seg = p.f32seg;
    int nrun = 0, first = 0;
    for (int i = 0; i < a.nseg; ++i) {
        a.seg[i] = p.pack[i];
        if (p.seg[i].type == NS_SIDE) continue;                 // not in the stream: ns_pack_side_kernel below
        if (p.seg[i].type == NS_WIDE && p.seg[i].zext < 0) {     // balanced triangular: ONE run of the stream, split per wave (ns_pack_kernel)
            a.run_seg[nrun] = i; a.run_pass[nrun] = 0; a.run_first[nrun] = first;
            first += ns_seg_steps(p.seg[i]); ++nrun;
            continue;
        }
        for (int ps = 0; ps < p.seg[i].passes; ++ps) {
            a.run_seg[nrun] = i; a.run_pass[nrun] = ps; a.run_first[nrun] = first;
            first += (ps > 0 && p.seg[i].type == NS_WIDE && p.seg[i].zext > 0) ? p.seg[i].zext : p.seg[i].steps; ++nrun;
        }
    }
    a.run_first[nrun] = first; a.nrun = nrun;
    const size_t total = (size_t)NS_NW * p.Gstride * NS_NT * 64 + (size_t)p.bias_total;
    hipLaunchKernelGGL(ns_pack_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, a);
    if (p.side_f4) hipLaunchKernelGGL(ns_pack_side_kernel, dim3((unsigned)((p.side_f4 + 255) / 256)), dim3(256), 0, s, a);
    return check_hip(hipGetLastError(), "net_stream pack launch");
}

template <int MOVE, bool GRAD, int STORE, int ROWS, bool BF = false>
static int ns_launch_rows(const NsArgs& a, int B, size_t lds_bytes, hipStream_t s, int extra = 0) {
    static bool attr_set = false;
    if (!attr_set) {
        const int rc = check_hip(hipFuncSetAttribute(reinterpret_cast<const void*>(&net_stream_kernel<NS_R, MOVE, GRAD, STORE, ROWS, BF>),
                                                     hipFuncAttributeMaxDynamicSharedMemorySize, NS_LDS_BYTES), "hipFuncSetAttribute");
        if (rc != LINNA_OK) return rc;
        attr_set = true;
    }
    hipLaunchKernelGGL((net_stream_kernel<NS_R, MOVE, GRAD, STORE, ROWS, BF>), dim3((B + ROWS - 1) / ROWS + extra), dim3(64 * NS_NW), lds_bytes, s, a);
    return check_hip(hipGetLastError(), "net_stream launch");
}
template <int MOVE, bool GRAD, int STORE = 0, bool BF = false>
static int ns_launch_kernel(const NsArgs& a0, int B, const NsProgram& p, int rows, hipStream_t s, int extra = 0, size_t lds_extra = 0) {
    const size_t lds = p.lds_for(rows, GRAD) + lds_extra;
#ifdef NS_STAMPS
    // diagnostic build: every launch writes its phase stamps to the buffer LINNA_FUSED_STAMPS names (tools/ns_stamps*.py)
    NsArgs a = a0;
    a.stamps = getenv("LINNA_FUSED_STAMPS") ? reinterpret_cast<unsigned long long*>(strtoull(getenv("LINNA_FUSED_STAMPS"), nullptr, 16)) : nullptr;
    if (!a.stamps) { set_error("net_stream: NS_STAMPS build needs LINNA_FUSED_STAMPS"); return LINNA_ERR_INVALID; }
#else
    const NsArgs& a = a0;
#endif
    if (rows == 4) return ns_launch_rows<MOVE, GRAD, STORE, 4, BF>(a, B, lds, s, extra);
    if constexpr (BF) {
        if (rows == 8) return ns_launch_rows<MOVE, GRAD, STORE, 8, BF>(a, B, lds, s, extra);
        if (rows == 16) return ns_launch_rows<MOVE, GRAD, STORE, 16, BF>(a, B, lds, s, extra);
    } else if constexpr (STORE == 3 && GRAD) {
        // the one-launch training step exists for the 4-row engine only (batches up to 1024 rows; the caller checks): on the
        // 8-row engine it was measured SLOWER than its two halves (batch 1500 at (26,457): 218.5 against 210.9 us per step)
    } else {
        if (rows == 8) return ns_launch_rows<MOVE, GRAD, STORE, 8>(a, B, lds, s, extra);
        if (rows == 16) return ns_launch_rows<MOVE, GRAD, STORE, 16>(a, B, lds, s, extra);
    }
    set_error("net_stream: %d rows per workgroup", rows);
    return LINNA_ERR_INVALID;
}
// the slice evaluation of a bf16 serving program: net_stream_slice_bf16_kernel, one instantiation per engine
template <int ROWS>
static int ns_launch_slice_bf16_rows(const NsArgs& a, int B, size_t lds_bytes, hipStream_t s) {
    static bool attr_set = false;
    if (!attr_set) {
        const int rc = check_hip(hipFuncSetAttribute(reinterpret_cast<const void*>(&net_stream_slice_bf16_kernel<NS_R, 2, false, 0, ROWS, true>),
                                                     hipFuncAttributeMaxDynamicSharedMemorySize, NS_LDS_BYTES), "hipFuncSetAttribute");
        if (rc != LINNA_OK) return rc;
        attr_set = true;
    }
    hipLaunchKernelGGL((net_stream_slice_bf16_kernel<NS_R, 2, false, 0, ROWS, true>), dim3((B + ROWS - 1) / ROWS), dim3(64 * NS_NW), lds_bytes, s, a);
    return check_hip(hipGetLastError(), "net_stream bf16 slice launch");
}
static int ns_launch_slice_bf16(const NsArgs& a, int B, const NsProgram& p, int rows, hipStream_t s) {
#ifdef NS_STAMPS
    set_error("net_stream: the NS_STAMPS build has no bf16 slice evaluation"); return LINNA_ERR_UNSUPPORTED;
#endif
    const size_t lds = p.lds_for(rows, false);
    if (rows == 4) return ns_launch_slice_bf16_rows<4>(a, B, lds, s);
    if (rows == 8) return ns_launch_slice_bf16_rows<8>(a, B, lds, s);
    if (rows == 16) return ns_launch_slice_bf16_rows<16>(a, B, lds, s);
    set_error("net_stream: %d rows per workgroup", rows);
    return LINNA_ERR_INVALID;
}

// ------------------------------------------------------------------ AdamW that writes the weight streams itself
// A training step ends with AdamW over the flat parameter buffer and begins with two re-layouts of the updated weights
// (ns_pack_kernel: the forward + loss stream and the dX-chain stream): three launches that each read or write every
// parameter.  Here the update runs once, in the flat buffer's own order, and every thread puts its four updated values
// where the two streams want them: the forward stream holds four consecutive k of one weight row as ONE 16-byte vector
// (one store), the dX-chain stream holds the transposed matrix (four 4-byte stores; neighbouring lanes fill
// neighbouring vectors).  Biases go to the forward stream's bias block.  Constant parts of a stream (zero padding, the
// loss's inverse covariance) are written by the ordinary re-layout once and never touched here.
constexpr int AS_BLOCK = 64;               // one wave per block: ~1200 blocks for 1.3 M parameters, five per CU
__device__ __forceinline__ void as_update(f32x4& P4, const f32x4& G4, f32x4& M4, f32x4& V4, float lr, float wd, float bc1,
                                          float sbc2, float beta1, float beta2, float eps) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {                   // adamw_kernel's arithmetic, operation for operation
        const float gi = G4[e];
        float pi = P4[e] * (1.f - lr * wd);
        float mi = M4[e];
        mi = mi + (gi - mi) * (1.f - beta1);
        const float vi = V4[e] * beta2 + (1.f - beta2) * gi * gi;
        const float denom = sqrtf(vi) / sbc2 + eps;
        pi = pi - (lr / bc1) * (mi / denom);
        P4[e] = pi; M4[e] = mi; V4[e] = vi;
    }
}

// One work item = a 4 x 4 block of a weight matrix (rows n0..n0+3, columns k0..k0+3; 16-byte loads and stores throughout:
// the forward stream takes the block's rows as four vectors, the dX-chain stream its columns) or four bias elements.
// BF: the places are in a bf16 training stream (as_slot_bf16): each value the nearest-even rounding of the fp32 one, the
// columns past the matrix's K not written (the first layer's second half starts right behind them)
template <bool BF = false>
__global__ __launch_bounds__(AS_BLOCK) void adamw_streams_kernel(AsArgs a, float* __restrict__ p, const float* __restrict__ g,
                                                            float* __restrict__ m, float* __restrict__ v,
                                                            const float* __restrict__ hyper, float beta1, float beta2, float eps) {
    int ri = 0;
    while (ri + 1 < a.nr && blockIdx.x >= a.r[ri + 1].blk0) ++ri;
    const AsRange R = a.r[ri];
    const unsigned it = (blockIdx.x - R.blk0) * AS_BLOCK + threadIdx.x;
    if (it >= R.n4) return;
    const float lr = hyper[0], wd = hyper[1], bc1 = hyper[2], sbc2 = hyper[3];
    if (R.kind == 1) {
        const size_t i = ((size_t)R.off4 + it) * 4;
        const f32x4 G4 = *reinterpret_cast<const f32x4*>(g + i);
        f32x4 P4 = *reinterpret_cast<const f32x4*>(p + i), M4 = *reinterpret_cast<const f32x4*>(m + i), V4 = *reinterpret_cast<const f32x4*>(v + i);
        as_update(P4, G4, M4, V4, lr, wd, bc1, sbc2, beta1, beta2, eps);
        *reinterpret_cast<f32x4*>(p + i) = P4; *reinterpret_cast<f32x4*>(m + i) = M4; *reinterpret_cast<f32x4*>(v + i) = V4;
        const AsBias B = a.b[R.idx];
        if (B.out) {
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if ((int)(4 * it) + e < B.N) B.out[4 * it + e] = B.scale * P4[e];
        }
        return;
    }
    const AsMat& W = a.w[R.idx];
    const unsigned ld4 = (unsigned)W.ld >> 2;
    const int n0 = 4 * (int)(it / ld4), k0 = 4 * (int)(it % ld4);
    f32x4 P4[4], G4[4], M4[4], V4[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const size_t i = (size_t)R.off4 * 4 + (size_t)min(n0 + r, W.N - 1) * W.ld + k0;     // (rows past N: reread the last, not stored)
        G4[r] = *reinterpret_cast<const f32x4*>(g + i); P4[r] = *reinterpret_cast<const f32x4*>(p + i);
        M4[r] = *reinterpret_cast<const f32x4*>(m + i); V4[r] = *reinterpret_cast<const f32x4*>(v + i);
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        as_update(P4[r], G4[r], M4[r], V4[r], lr, wd, bc1, sbc2, beta1, beta2, eps);
        if (n0 + r < W.N) {
            const size_t i = (size_t)R.off4 * 4 + (size_t)(n0 + r) * W.ld + k0;
            *reinterpret_cast<f32x4*>(p + i) = P4[r]; *reinterpret_cast<f32x4*>(m + i) = M4[r]; *reinterpret_cast<f32x4*>(v + i) = V4[r];
        } else {
            P4[r] = f32x4{0.f, 0.f, 0.f, 0.f};      // the streams' padding
        }
    }
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const AsPlace& q = W.pl[j];
        if (!q.out) continue;
        if constexpr (BF) {
            __bf16* const ob = reinterpret_cast<__bf16*>(q.out);
            if (!q.trans) {
#pragma unroll
                for (int r = 0; r < 4; ++r)
#pragma unroll
                    for (int e = 0; e < 4; ++e)
                        if (n0 + r < W.N && k0 + e < q.ncols) ob[as_slot_bf16(q, n0 + r, q.koff + k0 + e)] = (__bf16)(q.scale * P4[r][e]);
            } else {
                // column k0 + e, rows n0..n0+3: four consecutive k of one vector (koff and n0 are multiples of 4)
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (k0 + e < q.ncols)
                        *reinterpret_cast<bf16x4_t*>(ob + as_slot_bf16(q, k0 + e, q.koff + n0)) =
                            bf16x4_t{(__bf16)(q.scale * P4[0][e]), (__bf16)(q.scale * P4[1][e]), (__bf16)(q.scale * P4[2][e]), (__bf16)(q.scale * P4[3][e])};
            }
            continue;
        }
        if (!q.trans) {
            // row n0 + r, columns k0..k0+3: one vector of the stream (koff and k0 are multiples of 4; pad columns hold zeros)
#pragma unroll
            for (int r = 0; r < 4; ++r)
                if (n0 + r < W.N)
                    *reinterpret_cast<f32x4*>(q.out + as_slot(q, a.small, n0 + r, q.koff + k0)) =
                        f32x4{q.scale * P4[r][0], q.scale * P4[r][1], q.scale * P4[r][2], q.scale * P4[r][3]};
        } else {
            // column k0 + e, rows n0..n0+3: one vector of the transposed stream (rows past N: the zeros of its padding)
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (k0 + e < q.ncols)
                    *reinterpret_cast<f32x4*>(q.out + as_slot(q, a.small, k0 + e, q.koff + n0)) =
                        f32x4{q.scale * P4[0][e], q.scale * P4[1][e], q.scale * P4[2][e], q.scale * P4[3][e]};
        }
    }
}

// Descriptor table of adamw_streams_kernel for the flat buffer `params[nflat]` the layers' parameters live in, the
// forward + loss stream `s_fwd` (NS_TRAIN_FWD with `dn`) and the dX-chain stream `s_dx` (NS_DX).  LINNA_ERR_UNSUPPORTED
// when the buffer is not exactly the layers' tensors back to back, or a stream folds something into the weights that
// an element-wise scatter cannot reproduce (output maps, a second bias).
int net_stream_adamw_args(const linna_layer_t* layers, int nl, int in_size, int rows, const float* params, size_t nflat,
                          float* s_fwd, const NsDense* dn, float* s_dx, AsArgs* out, int merged) {
    // merged: ONE stream holds the forward + loss segments [0, nseg_f) and the dX chain [nseg_f, nseg) (NS_TRAIN_STEP)
    const bool bf = merged == 2;
    if (bf && rows != 4) { set_error("adamw_streams: the bf16 training stream is the 4-row engine's"); return LINNA_ERR_UNSUPPORTED; }
    const NsProgramRef pf_ref = ns_program(bf ? NS_TRAIN_STEP_BF16 : merged ? NS_TRAIN_STEP : NS_TRAIN_FWD, layers, nl, in_size, dn, rows);
    const NsProgramRef pd_ref = merged ? pf_ref : ns_program(NS_DX, layers, nl, in_size, nullptr, rows);
    const NsProgram& pf = *pf_ref;
    const NsProgram& pd = *pd_ref;
    if (merged) s_dx = s_fwd;
    if (!pf.ok || !pd.ok || !s_fwd || !s_dx || (merged && !pf.train_ok)) { set_error("adamw_streams: no forward / dX-chain program"); return LINNA_ERR_UNSUPPORTED; }
    const size_t f_lo = 0, f_hi = merged ? (size_t)pf.nseg_f : pf.pack.size();
    const size_t d_lo = merged ? (size_t)pf.nseg_f : 0, d_hi = pd.pack.size();
    ::memset(static_cast<void*>(out), 0, sizeof(*out));
    out->small = rows < 16;
    struct T { const float* ptr; int N, K, bias; };
    std::vector<T> ts;
    for (int i = 0; i < nl; ++i) {
        const linna_layer_t& l = layers[i];
        if (l.op == LINNA_OP_LINEAR) { ts.push_back({l.W, l.N, l.K, 0}); ts.push_back({l.b, l.N, 0, 1}); }
        else if (l.op == LINNA_OP_RESBLOCK) {
            ts.push_back({l.W1, l.C, l.K, 0}); ts.push_back({l.b1, l.C, 0, 1});
            ts.push_back({l.W2, l.N, l.C, 0}); ts.push_back({l.b2, l.N, 0, 1});
            if (l.Ws) ts.push_back({l.Ws, l.N, l.K, 0});
        } else { set_error("adamw_streams: op %d", l.op); return LINNA_ERR_UNSUPPORTED; }
    }
    std::sort(ts.begin(), ts.end(), [](const T& x, const T& y) { return x.ptr < y.ptr; });
    if ((int)ts.size() > AS_MAXR) { set_error("adamw_streams: %d tensors", (int)ts.size()); return LINNA_ERR_UNSUPPORTED; }
    auto runs_first = [](const NsProgram& p, int seg, int pass) {
        int first = 0;
        for (int i = 0; i < seg; ++i) first += ns_seg_steps(p.seg[i]);
        return first + pass * p.seg[seg].steps;
    };
    // q2 (bf16 stream): where the second half of the first layer's [W | W] goes
    auto place = [&](const NsProgram& p, float* base, const float* W, int K, AsPlace* q, size_t lo, size_t hi, AsPlace* q2) -> int {
        for (size_t i = lo; i < hi; ++i) {
            const NsPackSeg& S = p.pack[i];
            const bool isA = S.Wa == W, isB = S.Wb == W;
            if (!isA && !isB) continue;
            if (q->out) { set_error("adamw_streams: a weight matrix twice in one stream"); return LINNA_ERR_UNSUPPORTED; }
            if (S.rscale || S.rshift || S.b2) { set_error("adamw_streams: folded output map"); return LINNA_ERR_UNSUPPORTED; }
            if (p.seg[i].passes > 2) { set_error("adamw_streams: %d passes", p.seg[i].passes); return LINNA_ERR_UNSUPPORTED; }
            auto fill = [&](AsPlace* d, bool a_part) {
                d->out = base; d->scale = a_part ? 1.f : S.alpha; d->trans = a_part ? S.transA : S.transB; d->koff = a_part ? 0 : S.Kapad;
                d->ncols = S.N; d->type = S.type; d->ncg = S.ncg; d->steps = S.steps; d->G = p.Gstride;
                d->first0 = runs_first(p, (int)i, 0); d->first1 = p.seg[i].passes > 1 ? runs_first(p, (int)i, 1) : d->first0;
                if (bf && !d->trans) d->ncols = K;         // (bf16: the bound on the columns of W a writer stores)
            };
            if (isA && isB) {                               // the bf16 first layer [W | W]
                if (!bf || !q2 || q2->out) { set_error("adamw_streams: a weight matrix twice in one segment"); return LINNA_ERR_UNSUPPORTED; }
                fill(q, true); fill(q2, false);
            } else {
                fill(q, isA);
            }
        }
        return LINNA_OK;
    };
    size_t off = 0;
    unsigned blk = 0;
    int nw = 0, nb = 0;
    for (size_t i = 0; i < ts.size(); ++i) {
        const T& t = ts[i];
        if (!t.ptr || t.ptr != params + off) { set_error("adamw_streams: the parameters are not one contiguous buffer"); return LINNA_ERR_UNSUPPORTED; }
        const int ld = t.bias ? 0 : (t.K + 3) & ~3;
        const size_t nf = t.bias ? (size_t)((t.N + 3) & ~3) : (size_t)t.N * ld;
        AsRange& R = out->r[i];
        R.off4 = (unsigned)(off / 4); R.blk0 = blk; R.kind = (short)t.bias;
        R.n4 = t.bias ? (unsigned)(nf / 4) : (unsigned)((t.N + 3) / 4) * (unsigned)(ld / 4);      // work items (see the kernel)
        blk += (R.n4 + AS_BLOCK - 1) / AS_BLOCK;
        if (t.bias) {
            if (nb >= AS_MAXB) { set_error("adamw_streams: biases"); return LINNA_ERR_UNSUPPORTED; }
            R.idx = (short)nb;
            AsBias& B = out->b[nb++];
            B.N = t.N;
            for (size_t j = f_lo; j < f_hi; ++j) {
                const NsPackSeg& S = pf.pack[j];
                if (S.b != t.ptr) continue;
                if (B.out || S.rscale || S.rshift || S.b2) { set_error("adamw_streams: bias folded or used twice"); return LINNA_ERR_UNSUPPORTED; }
                B.out = s_fwd + (size_t)NS_NW * pf.Gstride * NS_NT * 256 + S.bias_off; B.scale = S.bscale;
            }
            for (size_t j = d_lo; j < d_hi; ++j) if (pd.pack[j].b == t.ptr) { set_error("adamw_streams: bias in the dX program"); return LINNA_ERR_UNSUPPORTED; }
        } else {
            if (nw >= AS_MAXW) { set_error("adamw_streams: weight matrices"); return LINNA_ERR_UNSUPPORTED; }
            R.idx = (short)nw;
            AsMat& W = out->w[nw++];
            W.N = t.N; W.ld = ld;
            int rc = place(pf, s_fwd, t.ptr, t.K, &W.pl[0], f_lo, f_hi, &W.pl[1]);
            if (rc == LINNA_OK) rc = place(pd, s_dx, t.ptr, t.K, &W.pl[1], d_lo, d_hi, nullptr);
            if (rc != LINNA_OK) return rc;
            if (!W.pl[0].out) { set_error("adamw_streams: a weight matrix outside the forward stream"); return LINNA_ERR_UNSUPPORTED; }
        }
        off += nf;
    }
    if (off != nflat) { set_error("adamw_streams: %zu of %zu floats covered", off, nflat); return LINNA_ERR_UNSUPPORTED; }
    // every pack segment's weights must have been found among the tensors (the loss's constant matrix excepted)
    out->nr = (int)ts.size(); out->nblocks = blk;
    return LINNA_OK;
}

int launch_adamw_streams(const AsArgs& a, float* p, const float* g, float* m, float* v, const float* hyper, float b1, float b2,
                         float eps, hipStream_t s, bool bf) {
    if (bf) hipLaunchKernelGGL(adamw_streams_kernel<true>, dim3(a.nblocks), dim3(AS_BLOCK), 0, s, a, p, g, m, v, hyper, b1, b2, eps);
    else hipLaunchKernelGGL(adamw_streams_kernel<false>, dim3(a.nblocks), dim3(AS_BLOCK), 0, s, a, p, g, m, v, hyper, b1, b2, eps);
    return check_hip(hipGetLastError(), "adamw_streams launch");
}

// The launch header every program shares: rows Z[B][ldz] of nin columns, the weight stream and the program's steps and
// segment table.  full: the whole program (forward and backward halves), else its forward segments only.
static NsArgs ns_args(const NsProgram& p, const float* packed, const float* Z, int ldz, int B, int nin, bool full) {
    NsArgs a;
    ::memset(static_cast<void*>(&a), 0, sizeof(a));
    a.Z = Z; a.ldz = ldz; a.B = B; a.nin = nin;
    a.packed = packed;
    a.Gstride = p.Gstride; a.nseg_f = p.nseg_f;
    a.G = full ? p.Gstride : p.G;
    a.nseg = full ? (int)p.seg.size() : p.nseg_f;
    a.LD = p.LD; a.kpad0 = p.kpad0; a.nout = p.nout; a.bias_total = p.bias_total;
    a.T = 1.f;
    for (int i = 0; i < (int)p.seg.size(); ++i) a.seg[i] = p.seg[i];
    return a;
}
// The store table of segments [lo, hi) from the caller's per-op buffers: forward segments (dx = false) write op i's output
// y or the hidden h t of its residual block; dX-chain segments write d/d(op input) dprev gated by that input (`gate`), or
// d/dh dt gated by h.  The loss segment stores nothing.
static void ns_store_table(NsArgs& a, const NsProgram& p, const linna_layer_t* layers, int nl, const NsOpBufs* ops, int lo, int hi,
                           bool dx) {
    for (int i = lo; i < hi; ++i) {
        const int op = p.seg_op[i];
        if (op >= nl) continue;
        const NsOpBufs& b = ops[op];
        a.gn[i] = p.seg_hidden[i] ? layers[op].C : dx ? layers[op].K : layers[op].N;   // (a dX-chain program's segments are all nseg_f)
        if (!dx) { a.gout[i] = p.seg_hidden[i] ? b.t : b.y; a.gld[i] = p.seg_hidden[i] ? b.ldt : b.ldy; }
        else if (p.seg_hidden[i]) { a.gout[i] = b.dt; a.gld[i] = b.lddt; a.gmask[i] = b.t; a.gmld[i] = b.ldt; }
        else { a.gout[i] = b.dprev; a.gld[i] = b.ldp; a.gmask[i] = b.gate; a.gmld[i] = b.ldx; }
    }
}
// the sign-bit gates (ns_gates) into the launch; false when they do not fit the LDS or a gate has no producer (*lds_extra:
// the launch's LDS beyond the program's own)
static bool ns_set_gates(NsArgs& a, const NsGates& g, const NsProgram& p, int rows, size_t* lds_extra) {
    for (int i = 0; i < NS_MAXSEG; ++i) { a.gbit[i] = g.gbit[i]; a.mbit[i] = g.mbit[i]; }
    a.nbw = g.ncols / 32;
    a.bits_off = (int)(g.lds0 / sizeof(float));
    *lds_extra = g.lds - p.lds_for(rows, true);
    return g.ok && g.lds <= (size_t)NS_LDS_BYTES;
}

int launch_net_stream(NsKind kind, const linna_layer_t* layers, int nl, int in_size, const float* packed, const float* Z, int ldz, int B,
                      int nin, const int* is_flat, const float* a1, const float* a2, const int* lg, const float* xmean,
                      const float* xstd, const float* cscale, const float* cshift, const float* w, float T, float* lnP,
                      float* D, int ldd, float* TH, int ldt, const NsMove* mv, const NsGrad* gr, const int* gate, int rows,
                      const NsDense* dn, hipStream_t s, const float* cpost, const float* cshift2) {
    const bool bf = kind == NS_SERVE_BF16;
    if ((kind == NS_SERVE_DENSE) != (dn != nullptr) || !(kind == NS_SERVE || kind == NS_SERVE_DENSE || bf)) {
        set_error("net_stream: not a serving program"); return LINNA_ERR_INVALID;
    }
    const NsProgramRef pref = ns_program(kind, layers, nl, in_size, dn, rows);
    const NsProgram& p = *pref;
    if ((cpost != nullptr) != (cshift2 != nullptr) || (cpost && (dn || gr))) {
        set_error("net_stream: the exp output map needs cpost and cshift2, and has no dense / gradient program"); return LINNA_ERR_INVALID;
    }
    if (!p.ok) { set_error("net_stream: network not eligible"); return LINNA_ERR_UNSUPPORTED; }
    if (dn && (w || gr || cscale || cshift)) { set_error("net_stream: the dense program carries its own output map and has no fused gradient"); return LINNA_ERR_INVALID; }
    if (mv && (nin > 64 || (!w && !dn))) { set_error("net_stream: fused sampler moves need <= 64 parameters and a log-likelihood in the launch"); return LINNA_ERR_UNSUPPORTED; }
    if (gr && (!p.grad_ok || !w || !lnP || !gr->gscale || !gr->G || mv)) { set_error("net_stream: no fused gradient for this network / likelihood"); return LINNA_ERR_UNSUPPORTED; }
    NsArgs a = ns_args(p, packed, Z, ldz, B, nin, gr != nullptr);    // forward only: stop after the forward segments
    a.is_flat = is_flat; a.a1 = a1; a.a2 = a2; a.lg = lg; a.xmean = xmean; a.xstd = xstd;
    a.cscale = cscale; a.cshift = cshift; a.w = w; a.T = T;
    a.cpost = cpost; a.cshift2 = cshift2;
    a.dense = p.dense ? (dn && dn->factored ? 2 : 1) : 0; a.u_col = p.u_col; a.u_same = p.u_same; a.x0_keep = p.x0_keep;
    a.lnP = lnP; a.D = D; a.ldd = ldd; a.TH = TH; a.ldt = ldt;
    a.gate = gate;
    if (mv) {
        a.mv_coords = mv->coords; a.mv_ldc = mv->ldc; a.mv_logp = mv->logp; a.mv_S = mv->S;
        a.mv_cc = mv->cc; a.mv_ldcc = mv->ldcc; a.mv_C = mv->C; a.mv_nc = mv->nc;
        a.mv_seed = mv->seed; a.mv_step = mv->step; a.mv_step_off = mv->step_off; a.mv_stream = mv->stream; a.mv_a = mv->a; a.mv_naccept = mv->naccept;
        a.mv_chain = mv->chain; a.mv_lps = mv->lps;
        a.sl_Z0 = mv->sl_Z0; a.sl_L = mv->sl_L; a.sl_R = mv->sl_R; a.sl_Zt = mv->sl_Zt; a.sl_m = mv->sl_m; a.sl_nt = mv->sl_nt;
        a.sl_seed = mv->sl_seed; a.sl_step = mv->sl_step; a.sl_stream = mv->sl_stream; a.sl_flags = mv->sl_flags;
        if (mv->sb) a.sb = *mv->sb;
        if (mv->slice) {
            if (bf) return ns_launch_slice_bf16(a, B, p, rows, s);
            return ns_launch_kernel<2, false>(a, B, p, rows, s);
        }
        if (bf) return ns_launch_kernel<1, false, 0, true>(a, B, p, rows, s);
        return ns_launch_kernel<1, false>(a, B, p, rows, s);
    }
    if (bf && gr) { set_error("net_stream: no bf16 gradient"); return LINNA_ERR_UNSUPPORTED; }
    if (bf) return ns_launch_kernel<0, false, 0, true>(a, B, p, rows, s);
    if (gr) {
        a.gscale = gr->gscale; a.Gout = gr->G; a.ldg = gr->ldg;
        a.hm_p = gr->hm_p; a.hm_ldp = gr->hm_ldp; a.hm_q = gr->hm_q; a.hm_mass = gr->hm_mass; a.hm_ek = gr->hm_ek; a.hm_ed = gr->hm_ed;
        return ns_launch_kernel<0, true>(a, B, p, rows, s);
    }
    return ns_launch_kernel<0, false>(a, B, p, rows, s);
}

// Training / validation forward: X[B][ldx] (transformed inputs) -> every op's output (`ops[i].y`, the hidden h of a
// residual block `ops[i].t`) in global memory.
int launch_net_stream_store(const linna_layer_t* layers, int nl, int in_size, const float* packed, const float* X, int ldx,
                            int B, const NsOpBufs* ops, const float* cscale, const float* cshift, int rows, hipStream_t s) {
    const NsProgramRef pref = ns_program(NS_STORE, layers, nl, in_size, nullptr, rows);
    const NsProgram& p = *pref;
    if (!p.ok) { set_error("net_stream: network not eligible"); return LINNA_ERR_UNSUPPORTED; }
    NsArgs a = ns_args(p, packed, X, ldx, B, in_size, false);
    // the prologue's transform constants are loaded (and ignored): any readable arrays of >= in_size entries
    a.is_flat = reinterpret_cast<const int*>(X); a.a1 = X; a.a2 = X; a.lg = nullptr; a.xmean = X; a.xstd = X;
    a.cscale = cscale; a.cshift = cshift;                   // column affine of the last output (Y transforms), or null
    ns_store_table(a, p, layers, nl, ops, 0, p.nseg_f, false);
    return ns_launch_kernel<0, false, 1>(a, B, p, rows, s);
}


// lnP and d lnP / d z in ONE launch for any network the forward and dX-chain programs cover (GRAD + STORE == 2): the
// forward segments keep the signs of the activations the gates need (ns_gates; round 2 kept the activations themselves in
// the caller's workspace: 40 MB written and read back per 4096-chain launch of ChtoModelv2(33,33), in bursts at the run
// ends of 256 workgroups in step, each read an exposed L2 round trip behind a drained weight ring), the turnaround forms
// d lnP / d out, the dX chain runs down to the network input gating on those signs, the finish applies the prior map's
// derivative.  Diagonal covariance.
int launch_net_stream_grad2(const linna_layer_t* layers, int nl, int in_size, const float* packed, const float* Z, int ldz, int B,
                            int nin, const int* is_flat, const float* a1, const float* a2, const int* lg, const float* xmean,
                            const float* xstd, const float* cscale, const float* cshift, const float* w, float T, float* lnP,
                            const NsGrad& gr, int rows, hipStream_t s) {
    const NsProgramRef pref = ns_program(NS_GRAD_INPUT, layers, nl, in_size, nullptr, rows);
    const NsProgram& p = *pref;
    if (!p.ok || !p.dxi_ok) { set_error("net_stream: no forward + dX program for this network"); return LINNA_ERR_UNSUPPORTED; }
    if (!w || !lnP || !gr.gscale || !gr.G) { set_error("net_stream: the one-launch gradient needs a diagonal covariance"); return LINNA_ERR_INVALID; }
    NsArgs a = ns_args(p, packed, Z, ldz, B, nin, true);
    a.is_flat = is_flat; a.a1 = a1; a.a2 = a2; a.lg = lg; a.xmean = xmean; a.xstd = xstd;
    a.cscale = cscale; a.cshift = cshift; a.w = w; a.T = T; a.lnP = lnP;
    a.gscale = gr.gscale; a.Gout = gr.G; a.ldg = gr.ldg;
    a.hm_p = gr.hm_p; a.hm_ldp = gr.hm_ldp; a.hm_q = gr.hm_q; a.hm_mass = gr.hm_mass; a.hm_ek = gr.hm_ek; a.hm_ed = gr.hm_ed;
    const NsGates g = ns_gates(p, layers, nl, rows);
    for (int i = 0; i < (int)p.seg.size(); ++i) if (i >= p.nseg_f || g.gbit[i] >= 0) a.gn[i] = ns_seg_cols(p, layers, i);
    size_t lds_extra = 0;
    if (!ns_set_gates(a, g, p, rows, &lds_extra)) {
        set_error(g.ok ? "net_stream: the one-launch gradient's sign bits do not fit the LDS" : "net_stream: a gate of the one-launch gradient has no producer");
        return LINNA_ERR_UNSUPPORTED;
    }
    return ns_launch_kernel<0, true, 2>(a, B, p, rows, s, 0, lds_extra);
}

// the forward + loss half of a training launch (STORE == 3): the batch rows ROWS (null: 0..B-1) of X gathered and
// X-transformed into XB, every activation stored, the loss rows and d loss / d pred written
static NsArgs ns_train_args(const NsProgram& p, bool full, const linna_layer_t* layers, int nl, int in_size, const float* packed,
                            const float* X, int ldx, const int* ROWS, int B, const int* lg, const float* xmean, const float* xstd,
                            float* XB, int ldxb, const NsOpBufs* ops, const NsTrainLoss& L) {
    NsArgs a = ns_args(p, packed, X, ldx, B, in_size, full);
    a.is_flat = reinterpret_cast<const int*>(xmean); a.a1 = xmean; a.a2 = xmean;     // loaded and ignored
    a.lg = lg; a.xmean = xmean; a.xstd = xstd;
    a.dense = p.dense; a.u_col = p.u_col; a.u_same = p.u_same;
    ns_store_table(a, p, layers, nl, ops, 0, p.nseg_f, false);
    a.t_rows = ROWS; a.t_xb = XB; a.t_ldxb = ldxb;
    a.t_Y = L.YN; a.t_ldy = L.ldyn;
    a.t_den = L.den; a.t_inv_batch = L.inv_batch; a.t_loss_rows = L.loss_rows; a.t_dP = L.dP; a.t_lddp = L.lddp;
    return a;
}

// Training forward + loss in one launch (STORE == 3); `dn` = {Cinv, ldc, null, null}: the inverse covariance in the
// network's normalised output space as the last segment.
int launch_net_stream_train(const linna_layer_t* layers, int nl, int in_size, const float* packed, const float* X, int ldx,
                            const int* ROWS, int B, const int* lg, const float* xmean, const float* xstd, float* XB, int ldxb,
                            const NsOpBufs* ops, const NsTrainLoss& L, const NsDense& dn, int rows, hipStream_t s) {
    const NsProgramRef pref = ns_program(NS_TRAIN_FWD, layers, nl, in_size, &dn, rows);
    const NsProgram& p = *pref;
    if (!p.ok || !p.dense) { set_error("net_stream: network + loss not eligible"); return LINNA_ERR_UNSUPPORTED; }
    const NsArgs a = ns_train_args(p, false, layers, nl, in_size, packed, X, ldx, ROWS, B, lg, xmean, xstd, XB, ldxb, ops, L);
    return ns_launch_kernel<0, false, 3>(a, B, p, rows, s);
}

// A training step's network work in ONE launch (TRB: GRAD + STORE == 3): launch_net_stream_train's forward + loss, its
// finish as the turnaround, then launch_net_stream_dx's chain down to op 1 -- same arguments as the two of them; the gates
// of the backward half are sign bits in LDS (ns_gates: the activations go to memory all the same, the parameter
// gradients read them, but no gate is read back from there).  `post`: only the AdamW step constants ride here (the loss
// rows are not complete before every workgroup's turnaround: the batch mean rides in the parameter-gradient launch instead).
int launch_net_stream_train_bwd(const linna_layer_t* layers, int nl, int in_size, const float* packed, const float* X, int ldx,
                                const int* ROWS, int B, const int* lg, const float* xmean, const float* xstd, float* XB, int ldxb,
                                const NsOpBufs* ops, const NsTrainLoss& L, const NsDense& dn, int rows, hipStream_t s,
                                const NsPost* post, bool bf) {
    const NsProgramRef pref = ns_program(bf ? NS_TRAIN_STEP_BF16 : NS_TRAIN_STEP, layers, nl, in_size, &dn, rows);
    const NsProgram& p = *pref;
    if (!p.ok || !p.train_ok || !p.dense) { set_error("net_stream: network + loss have no one-launch training program"); return LINNA_ERR_UNSUPPORTED; }
    if (rows != 4) { set_error(bf ? "net_stream: the bf16 training step runs on the 4-row engine (batches of up to 1024 rows)"
                                  : "net_stream: the one-launch training step runs on the 4-row engine"); return LINNA_ERR_UNSUPPORTED; }
    NsArgs a = ns_train_args(p, true, layers, nl, in_size, packed, X, ldx, ROWS, B, lg, xmean, xstd, XB, ldxb, ops, L);
    ns_store_table(a, p, layers, nl, ops, p.nseg_f, (int)p.seg.size(), true);
    const NsGates g = ns_gates(p, layers, nl, rows);
    size_t lds_extra = 0;
    if (!ns_set_gates(a, g, p, rows, &lds_extra)) {
        set_error(g.ok ? "net_stream: the training step's sign bits do not fit the LDS" : "net_stream: a gate of the one-launch training step has no producer");
        return LINNA_ERR_UNSUPPORTED;
    }
    int extra = 0;
    if (post && post->step) { a.p_step = post->step; a.p_hyper = post->hyper; a.p_b1 = post->b1; a.p_b2 = post->b2; extra = 1; }
    if (bf) {
        static bool attr_set = false;
#ifdef NS_STAMPS
        set_error("net_stream: the NS_STAMPS build has no bf16 training step"); return LINNA_ERR_UNSUPPORTED;
#endif
        if (!attr_set) {
            const int rc = check_hip(hipFuncSetAttribute(reinterpret_cast<const void*>(&net_stream_train_bf16_kernel<NS_R, 0, true, 3, 4, true>),
                                                         hipFuncAttributeMaxDynamicSharedMemorySize, NS_LDS_BYTES), "hipFuncSetAttribute");
            if (rc != LINNA_OK) return rc;
            attr_set = true;
        }
        hipLaunchKernelGGL((net_stream_train_bf16_kernel<NS_R, 0, true, 3, 4, true>), dim3((B + 3) / 4 + extra), dim3(64 * NS_NW), p.lds_for(rows, true) + lds_extra, s, a);
        return check_hip(hipGetLastError(), "net_stream bf16 training launch");
    }
    return ns_launch_kernel<0, true, 3>(a, B, p, rows, s, extra, lds_extra);
}

// The dX chain of a training step in one launch (what linna_net_backward otherwise runs as one GEMM per op):
// dOUT[B][lddo] -> for every op i >= first (1, or 0 with_input) the gradient with respect to its input, gated by that input
// where it went through a ReLU, into ops[i].dprev; for residual blocks also d/dh into ops[i].dt, gated by the stored h.
int launch_net_stream_dx(const linna_layer_t* layers, int nl, int in_size, const float* packed, const float* dOUT, int lddo,
                         int B, const NsOpBufs* ops, int with_input, int rows, hipStream_t s, const NsPost* post) {
    const NsProgramRef pref = ns_program(with_input ? NS_DX_INPUT : NS_DX, layers, nl, in_size, nullptr, rows);
    const NsProgram& p = *pref;
    if (!p.ok) { set_error("net_stream: no dX-chain program for this network"); return LINNA_ERR_UNSUPPORTED; }
    NsArgs a = ns_args(p, packed, dOUT, lddo, B, layers[nl - 1].N, false);
    a.is_flat = reinterpret_cast<const int*>(dOUT); a.a1 = dOUT; a.a2 = dOUT; a.lg = nullptr; a.xmean = dOUT; a.xstd = dOUT;
    ns_store_table(a, p, layers, nl, ops, 0, p.nseg_f, true);
    if (post && post->n > 0) {                    // the rider (see NsArgs::p_rows): one more workgroup
        a.p_rows = post->rows; a.p_n = post->n; a.p_scale = post->scale; a.p_out = post->out;
        a.p_step = post->step; a.p_hyper = post->hyper; a.p_b1 = post->b1; a.p_b2 = post->b2;
        return ns_launch_kernel<0, false, 2>(a, B, p, rows, s, 1);
    }
    return ns_launch_kernel<0, false, 2>(a, B, p, rows, s);
}
}  // namespace linna
