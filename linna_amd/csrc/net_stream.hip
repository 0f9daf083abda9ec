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
#include "net_program.h"
#include <stdlib.h>
#include <type_traits>
#include <cstring>
#include <algorithm>

namespace linna {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));   // B (and A) operand of v_mfma_f32_16x16x32_bf16
typedef short s16x4 __attribute__((ext_vector_type(4)));     // ... of v_mfma_f32_4x4x4_16b_bf16 (the builtin takes the bits)

#ifndef NS_R
#define NS_R 6
#endif
#ifndef NS_PRE
#define NS_PRE 2
#endif
// the launch's arguments: the program's segment table (net_program.h) behind everything the prologue and the finish read
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
    float* gout[NS_SEGCAP]; int gld[NS_SEGCAP]; int gn[NS_SEGCAP];
    // STORE == 2 (the dX chain of a training step): a segment's output is zeroed where gmask (the stored forward
    // activation whose gradient it is) is not positive, before it is stored and handed to the next segment
    const float* gmask[NS_SEGCAP]; int gmld[NS_SEGCAP];
    // GRAD + STORE == 2 (lnP and its gradient in one launch, any network): the backward needs the SIGN of the forward
    // activations only, and it needs it in this very workgroup -- one bit per (row, column) in LDS ([ROWS][nbw] words at
    // float offset bits_off) instead of the activations in global memory.  gbit / mbit: the first bit column (a multiple of
    // 64) of the tensor a segment writes / is gated by, -1 = none.  The merged training launch (GRAD + STORE == 3) gates the
    // same way -- its activations still go to global memory, the parameter gradients need them.
    int nbw, bits_off;
    int gbit[NS_SEGCAP], mbit[NS_SEGCAP];
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
    // predecessors were rejected (slice_draw_wave's rule: Philox (walker, step, stream, sub j + 1)).  Saves the launch between them.
    const float* sl_Z0; const float* sl_L; const float* sl_R; const float* sl_Zt; int sl_m, sl_nt;
    unsigned long long sl_seed; const int* sl_step; int sl_stream; const int* sl_flags;
    SliceBegin sb;                      // MOVE == 2, sb.logp != null: the half step's set-up in this launch's prologue (common.h)
    NsSeg seg[NS_SEGCAP];
    const float* hm_eps;                // GRAD: the leapfrog in the finish with a step size per row (the EPS instantiations: hm_ek, hm_ed then multiply it)
};

// ------------------------------------------------------------------ weight re-layout
// SIDE segments (serving programs of the 16-row engine): a SPLIT segment of <= 32 output columns -- the hidden
// h = relu(W1 x + b1) of a residual block, 1000 -> 16 and 500 -> 32 in ChtoModelv2 -- costs the step loop 8 + 4 steps of
// which three quarters / half multiply zero weights (a wave's four 16-column tiles need 64 columns).  As a SIDE segment it
// leaves the weight stream: its weights sit in a block of their own behind the biases, laid out so that a wave's four tiles
// are (column tile, k chunk) pairs -- kc = 4 chunks of 16 columns, or 2 chunks of 32 -- and the whole segment is at most
// two steps per wave, run inside the run-end code of the segment before it (loads issued before that segment's epilogue,
// by inline asm: the compiler's counted waits for the ring never see them).  The step loop itself is untouched.
//   side[w][s][t][lane][e]:  n = 16 (t % (4 / kc)) + li,  k = 16 (kc (w steps + s) + t / (4 / kc)) + 4 kq + e
struct NsPackArgs {
    NsPackSeg seg[NS_SEGCAP];
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
        if (k < S.Ka && S.kscale) v *= S.kscale[k];
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
        if (n < S.N && S.Wa && !S.transA && !S.kscale && k0 + 3 < S.Ka && (S.lda & 3) == 0 && (reinterpret_cast<uintptr_t>(S.Wa) & 15) == 0) {
            // the common case: four consecutive k of one weight row, 16 bytes aligned (rows are padded to 4 floats)
            v = *reinterpret_cast<const f32x4*>(S.Wa + (size_t)n * S.lda + k0);
            if (S.rscale) { const float r = S.rscale[n]; v = f32x4{v[0] * r, v[1] * r, v[2] * r, v[3] * r}; }
        } else if (n < S.N) {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int k = k0 + e;
                if (k < S.Kapad) {
                    if (k < S.Ka) v[e] = !S.Wa ? (k == n ? 1.f : 0.f) : S.transA ? S.Wa[(size_t)k * S.lda + n] : S.Wa[(size_t)n * S.lda + k];
                    if (k < S.Ka && S.kscale) v[e] *= S.kscale[k];      // (the same product the forward segment's rscale makes of this weight)
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
// in a kernel of its own, net_stream_slice_bf16_kernel; so is GRAD + STORE == 2, net_stream_grad_bf16_kernel).  The stream holds bf16
// weights (ns_pack_kernel, p.bf) and one step covers 32 k x 64 columns -- the same 4 KiB per wave and step, so the ring,
// its four 1-KiB loads and the counted waits keep their shape and a segment takes half the steps.  Activations stay fp32
// in LDS and are rounded to bf16 (nearest-even) where the A operand is read: two ds_read_b128 per step (8 k per lane).
// 16 rows: v_mfma_f32_16x16x32_bf16, one per column tile and step (lane group kq owns k 8 kq .. 8 kq + 7 of the step in
// A and B alike); 8 / 4 rows: v_mfma_f32_4x4x4_16b_bf16 with the CBSZ / ABID broadcast of the fp32 4x4x1 form, block b of
// the A read holding row set b & 3 and k chunk b >> 2 (8 k), two instructions (halves of the chunk) per (row set, chunk).
// The network input goes in as x_hi = bf16(x) at column c and x_lo = x - x_hi at column nin + c, and the first layer is
// packed [W | W] (net_program.hip, ns_lower): the input is not quantised to 8 bits.  Epilogues, the finish and the prior map are the
// fp32 kernel's.  SIDE segments are off in bf16 (K4 = false; the program builder plans none).
// BF + TRB: the opt-in bf16 training step (net_stream_train_bf16_kernel, 4-row engine).  The forward segments and the dX
// chain consume bf16 steps as above; the loss segment (the dense inverse covariance behind the last layer) stays an fp32
// run inside the same stream -- both formats move 4 KiB per wave and step, so only the consumer differs.  It is chosen
// once per run (begin_run: f32run); inside `step` the choice selects between two MFMA sequences and touches no memory.
// The kernel body is net_stream_body.inc, the text of the kernels below: the whole-network kernel, the opt-in bf16 slice
// evaluation (MOVE == 2 on a bf16 stream, described at net_stream_slice_bf16_kernel), the opt-in bf16 one-launch gradient
// (described at net_stream_grad_bf16_kernel), and the opt-in bf16
// training step (linna_net_set_train_precision) -- the merged training launch (GRAD + STORE == 3, 4-row engine) on a bf16
// stream whose loss segment stays fp32, a kernel of its own rather than a net_stream_kernel specialisation.  (One text
// included twice instead of a device function both call: inlined into a wrapper, the same body compiles to other
// instructions for every existing instantiation.)
template <int R, int MOVE, bool GRAD, int STORE, int ROWS, bool BF = false>
__global__ __launch_bounds__(64 * NS_NW, 1) void net_stream_kernel(NsArgs a) {
    constexpr bool EPS = false, PLAIN = false, WOUT = false, DGR = false;
#include "net_stream_body.inc"
}
// EPS: the fp32 gradient programs (GRAD, STORE 0 or 2) whose finish runs the leapfrog with a step size per row, a.hm_eps
// (linna_logprob_grad_leapfrog_eps).  Kernels of their own, here and for the bf16 gradient below: a run-time test of the
// pointer in the shared finish slowed the launches without one (net_stream_body.inc), and the instantiations
// above keep their names.
template <int R, int MOVE, bool GRAD, int STORE, int ROWS, bool BF>
__global__ __launch_bounds__(64 * NS_NW, 1) void net_stream_eps_kernel(NsArgs a) {
    static_assert(!BF && GRAD && (STORE == 0 || STORE == 2) && MOVE == 0, "the fp32 one-launch gradients only");
    constexpr bool EPS = true, PLAIN = false, WOUT = false, DGR = false;
#include "net_stream_body.inc"
}
// WOUT: the fp32 one-launch gradient (GRAD + STORE == 2) of a network with MORE than 64 outputs, with and without EPS.  The
// turnaround holds the output map, the likelihood weights and gscale of 64 columns per row in registers, loaded up front;
// here it walks the rest of the row with those constants read from memory (net_stream_body.inc).  Kernels of their own for
// the same reason as EPS: the <= 64-output instantiations keep their instructions.  Everything else -- the poisoned prior
// term of a non-finite row, the dX chain, the leapfrog in the finish -- is the shared text.
template <int R, int MOVE, bool GRAD, int STORE, int ROWS, bool BF, bool EPSV>
__global__ __launch_bounds__(64 * NS_NW, 1) void net_stream_wide_kernel(NsArgs a) {
    static_assert(!BF && GRAD && STORE == 2 && MOVE == 0, "the fp32 one-launch gradient of any network only");
    constexpr bool EPS = EPSV, PLAIN = false, WOUT = true, DGR = false;
#include "net_stream_body.inc"
}
// DGR: lnP and d lnP / d z in one launch for a DENSE inverse covariance S = L L^T (NS_GRAD_INPUT_DENSE; opt-in,
// linna_logprob_set_dense_grad), with and without EPS.  The program's forward half ends in U = d L (the output map folded
// into the last layer, as the dense serving program has it), so the likelihood is the trivial diagonal one in U-space:
// the turnaround takes chi2 = sum U_c^2 over the row in LDS at any width and leaves d lnP / dU_c = -U_c / T at column c
// of the first backward segment's input, the transposed dense map; behind it runs the ordinary dX chain.  Nothing of the
// output map, the likelihood weights or gscale is loaded.  Kernels of their own for the same reason as EPS and WOUT.
template <int R, int MOVE, bool GRAD, int STORE, int ROWS, bool BF, bool EPSV>
__global__ __launch_bounds__(64 * NS_NW, 1) void net_stream_dense_kernel(NsArgs a) {
    static_assert(!BF && GRAD && STORE == 2 && MOVE == 0, "the fp32 one-launch gradient of any network only");
    constexpr bool EPS = EPSV, PLAIN = false, WOUT = false, DGR = true;
#include "net_stream_body.inc"
}
// PLAIN: the serving launch of a plain MLP (ns_program_plain, net_program.hip: WIDE and SPLIT segments only, diagonal
// likelihood with its whole output map, lnP the only output, no gate) on the 16-row fp32 engine.  The same body with
// everything such a launch never uses compiled out -- SIDE prefetch and its register zeroing at every run end, the input
// skip, the dense and exp finishes, the gate test, the selects on optional pointers -- and the next segment's descriptor
// requested at the START of a run, so that no run end begins with a scalar round trip.  Same MFMAs on the same fragments in
// the same order: lnP is bit-identical to net_stream_kernel<R, 0, false, 0, 16>'s (linna_serve_plain switches between them).
template <int R>
__global__ __launch_bounds__(64 * NS_NW, 1) void net_stream_plain_kernel(NsArgs a) {
    constexpr int MOVE = 0, STORE = 0, ROWS = 16;
    constexpr bool GRAD = false, BF = false, EPS = false, PLAIN = true, WOUT = false, DGR = false;
#include "net_stream_body.inc"
}
// The plain instantiation with its step placed by hand (net_stream_body.inc, HAND): the sixteen MFMAs, four refill loads, the
// A read and the counted waits of a step as one block of assembly text, at most one filler per MFMA gap, the stream address
// advanced on the scalar unit.  Prologue, run ends and finish are the compiled text of the kernel above; same MFMAs on the
// same fragments in the same order, so lnP is bit-identical to both.  The default of a plain launch;
// linna_serve_plain_sched(0) keeps net_stream_plain_kernel, whose instructions this kernel's existence does not change.  (A
// kernel of its own name rather than a flag of the one above: that one's symbol is part of what the host tests pin.)
#if NS_R == 6
#define NS_HAVE_PLACED 1
template <int R>
__global__ __launch_bounds__(64 * NS_NW, 1) void net_stream_placed_kernel(NsArgs a) {
    constexpr int MOVE = 0, STORE = 0, ROWS = 16;
    constexpr bool GRAD = false, BF = false, EPS = false, PLAIN = true, WOUT = false, DGR = false;
#define NS_BODY_HAND
#include "net_stream_body.inc"
#undef NS_BODY_HAND
}
// The hand-placed launch without the MFMAs that multiply zero padding (net_stream_body.inc, TRIM): two shorter texts of the
// step -- T3, a wave whose fourth column tile is padding (a 33-column last layer); S1, the last step of a run whose K ends
// one k into it (a 33-input first layer) -- chosen per run by one scalar the wave derives from what the launcher folds into
// NsSeg::type (ns_trim_fold, net_program.hip).  The skipped products are zeros added to accumulators that are not -0, or
// columns nobody reads: lnP is bit-identical to the kernel above, which linna_serve_plain_trim(0) keeps and whose
// instructions this kernel's existence does not change.
#define NS_HAVE_TRIM 1
template <int R>
__global__ __launch_bounds__(64 * NS_NW, 1) void net_stream_trim_kernel(NsArgs a) {
    constexpr int MOVE = 0, STORE = 0, ROWS = 16;
    constexpr bool GRAD = false, BF = false, EPS = false, PLAIN = true, WOUT = false, DGR = false;
#define NS_BODY_HAND
#define NS_BODY_TRIM
#include "net_stream_body.inc"
#undef NS_BODY_TRIM
#undef NS_BODY_HAND
}
#endif
template <int R, int MOVE, bool GRAD, int STORE, int ROWS, bool BF>
__global__ __launch_bounds__(64 * NS_NW, 1) void net_stream_train_bf16_kernel(NsArgs a) {
    static_assert(BF && GRAD && STORE == 3 && ROWS == 4 && MOVE == 0, "the bf16 training step only");
    constexpr bool EPS = false, PLAIN = false, WOUT = false, DGR = false;
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
    constexpr bool EPS = false, PLAIN = false, WOUT = false, DGR = false;
#define NS_BODY_SLICE_BF16
#include "net_stream_body.inc"
#undef NS_BODY_SLICE_BF16
}
// BF + GRAD + STORE == 2: lnP and d lnP / d z in one launch on the bf16 engine (linna_logprob_set_grad_precision; 16-, 8-
// and 4-row engines).  The forward half is the bf16 serving step with the signs of the activations kept as bits in LDS,
// as the fp32 one-launch gradient keeps them; the turnaround (d lnP / d out from the fp32 output map and the diagonal
// likelihood) is fp32 and leaves its rows in LDS; the dX chain consumes bf16 steps as the bf16 training step's chain does
// -- the transposed weights rounded after the same folding as the forward ones, delta rounded where the A operand is read,
// fp32 accumulators, fp32 epilogues gated by the LDS bits -- and the finish (the prior map's derivative, the leapfrog's
// kick and drift) is the fp32 gradient's.  No SIDE segments.  A kernel of its own for the same reason as the two above.
template <int R, int MOVE, bool GRAD, int STORE, int ROWS, bool BF>
__global__ __launch_bounds__(64 * NS_NW, 1) void net_stream_grad_bf16_kernel(NsArgs a) {
    static_assert(BF && GRAD && STORE == 2 && MOVE == 0, "the bf16 one-launch gradient only");
    constexpr bool EPS = false, PLAIN = false, WOUT = false, DGR = false;
#define NS_BODY_GRAD_BF16
#include "net_stream_body.inc"
#undef NS_BODY_GRAD_BF16
}
template <int R, int MOVE, bool GRAD, int STORE, int ROWS, bool BF>
__global__ __launch_bounds__(64 * NS_NW, 1) void net_stream_eps_bf16_kernel(NsArgs a) {      // ... with a step size per row (EPS)
    static_assert(BF && GRAD && STORE == 2 && MOVE == 0, "the bf16 one-launch gradient only");
    constexpr bool EPS = true, PLAIN = false, WOUT = false, DGR = false;
#define NS_BODY_GRAD_BF16
#include "net_stream_body.inc"
#undef NS_BODY_GRAD_BF16
}

// ---------------------------------------------------------------------------- host side: the launches
// Engine for a batch of B rows: the fewest rows per workgroup that still fit the batch into one workgroup per CU, unless
// one is forced (ns_forced_rows_resolved, net_program.hip).
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

// ---- one table from launch variant to kernel.  A launcher names WHAT it launches, a variant and its flags; every
// net_stream*_kernel instantiation of the library is named in this table and nowhere else.  A row: the 16-, 8- and 4-row
// engines' kernels (null: no such engine -- the plain instantiations are 16-row kernels; the one-launch training step has the
// 4-row engine only: on the 8-row one it was measured SLOWER than its two halves, batch 1500 at (26,457): 218.5 against 210.9 us
// per step), the launch's name for the error text, and what the NS_STAMPS diagnostic build lacks it as (null: it has it).
typedef void (*NsKernel)(NsArgs);
enum NsVariant { NV_SERVE, NV_STRETCH, NV_SLICE, NV_GRAD_MLP, NV_GRAD2, NV_STORE, NV_DX, NV_TRAIN_FWD, NV_TRAIN_STEP };
// a bf16 stream; the leapfrog in the finish with a step size per row; more than 64 outputs; the plain MLP's lean serving kernel; ... hand-placed
enum : unsigned { NF_BF16 = 1, NF_EPS = 2, NF_WIDE = 4, NF_PLAIN = 8, NF_PLACED = 16, NF_DENSE = 32,     // ... a dense covariance's one-launch gradient
                  NF_TRIM = 64 };                                                                          // ... hand-placed, no MFMA on zero padding
struct NsEntry { NsVariant v; unsigned flags; NsKernel k[3]; const char* what; const char* stamps_lacks; bool attr_set[3]; };
// the three engines of one kernel template: <R, MOVE, GRAD, STORE, rows, BF (, EPS)>
#define NS_ENGINES(K, MOVE, GRAD, STORE, ...) \
    {K<NS_R, MOVE, GRAD, STORE, 16, __VA_ARGS__>, K<NS_R, MOVE, GRAD, STORE, 8, __VA_ARGS__>, K<NS_R, MOVE, GRAD, STORE, 4, __VA_ARGS__>}
static NsEntry ns_table[] = {
    {NV_SERVE, 0, NS_ENGINES(net_stream_kernel, 0, false, 0, false), "net_stream launch"},
    {NV_SERVE, NF_BF16, NS_ENGINES(net_stream_kernel, 0, false, 0, true), "net_stream launch"},
    {NV_SERVE, NF_PLAIN, {net_stream_plain_kernel<NS_R>, nullptr, nullptr}, "net_stream plain launch"},
#ifdef NS_HAVE_PLACED
    {NV_SERVE, NF_PLAIN | NF_PLACED, {net_stream_placed_kernel<NS_R>, nullptr, nullptr}, "net_stream plain launch (hand-placed step)"},
#endif
#ifdef NS_HAVE_TRIM
    {NV_SERVE, NF_PLAIN | NF_PLACED | NF_TRIM, {net_stream_trim_kernel<NS_R>, nullptr, nullptr}, "net_stream plain launch (hand-placed step, trimmed)"},
#endif
    {NV_STRETCH, 0, NS_ENGINES(net_stream_kernel, 1, false, 0, false), "net_stream launch"},
    {NV_STRETCH, NF_BF16, NS_ENGINES(net_stream_kernel, 1, false, 0, true), "net_stream launch"},
    {NV_SLICE, 0, NS_ENGINES(net_stream_kernel, 2, false, 0, false), "net_stream launch"},
    {NV_SLICE, NF_BF16, NS_ENGINES(net_stream_slice_bf16_kernel, 2, false, 0, true), "net_stream bf16 slice launch", "bf16 slice evaluation"},
    {NV_GRAD_MLP, 0, NS_ENGINES(net_stream_kernel, 0, true, 0, false), "net_stream launch"},
    {NV_GRAD_MLP, NF_EPS, NS_ENGINES(net_stream_eps_kernel, 0, true, 0, false), "net_stream launch"},
    {NV_GRAD2, 0, NS_ENGINES(net_stream_kernel, 0, true, 2, false), "net_stream launch"},
    {NV_GRAD2, NF_EPS, NS_ENGINES(net_stream_eps_kernel, 0, true, 2, false), "net_stream launch"},
    {NV_GRAD2, NF_WIDE, NS_ENGINES(net_stream_wide_kernel, 0, true, 2, false, false), "net_stream wide-output gradient launch"},
    {NV_GRAD2, NF_WIDE | NF_EPS, NS_ENGINES(net_stream_wide_kernel, 0, true, 2, false, true), "net_stream wide-output gradient launch"},
    {NV_GRAD2, NF_DENSE, NS_ENGINES(net_stream_dense_kernel, 0, true, 2, false, false), "net_stream dense-covariance gradient launch"},
    {NV_GRAD2, NF_DENSE | NF_EPS, NS_ENGINES(net_stream_dense_kernel, 0, true, 2, false, true), "net_stream dense-covariance gradient launch"},
    {NV_GRAD2, NF_BF16, NS_ENGINES(net_stream_grad_bf16_kernel, 0, true, 2, true), "net_stream bf16 gradient launch", "bf16 gradient"},
    {NV_GRAD2, NF_BF16 | NF_EPS, NS_ENGINES(net_stream_eps_bf16_kernel, 0, true, 2, true), "net_stream bf16 gradient launch", "bf16 gradient"},
    {NV_STORE, 0, NS_ENGINES(net_stream_kernel, 0, false, 1, false), "net_stream launch"},
    {NV_DX, 0, NS_ENGINES(net_stream_kernel, 0, false, 2, false), "net_stream launch"},
    {NV_TRAIN_FWD, 0, NS_ENGINES(net_stream_kernel, 0, false, 3, false), "net_stream launch"},
    {NV_TRAIN_STEP, 0, {nullptr, nullptr, net_stream_kernel<NS_R, 0, true, 3, 4, false>}, "net_stream launch"},
    {NV_TRAIN_STEP, NF_BF16, {nullptr, nullptr, net_stream_train_bf16_kernel<NS_R, 0, true, 3, 4, true>}, "net_stream bf16 training launch", "bf16 training step"},
};
#undef NS_ENGINES
// the kernel of (variant, flags) on the engine of `rows` rows: its table row and the engine's slot in it
static int ns_kernel(NsVariant v, unsigned flags, int rows, NsEntry** entry, int* slot) {
    for (NsEntry& e : ns_table) {
        if (e.v != v || e.flags != flags) continue;
#ifdef NS_STAMPS
        if (e.stamps_lacks) { set_error("net_stream: the NS_STAMPS build has no %s", e.stamps_lacks); return LINNA_ERR_UNSUPPORTED; }
#endif
        const int i = rows == 16 ? 0 : rows == 8 ? 1 : rows == 4 ? 2 : -1;
        if (i < 0 || !e.k[i]) break;
        *entry = &e; *slot = i;
        return LINNA_OK;
    }
    set_error("net_stream: %d rows per workgroup", rows);
    return LINNA_ERR_INVALID;
}
// One launch of the whole-network kernel instantiation in slot `i` of table row `e`: 64 NS_NW threads per workgroup and
// `lds_bytes` of dynamic LDS, which the instantiation is allowed up to the CU's whole LDS before its first launch.
static int ns_launch(NsEntry& e, int i, const NsArgs& a, int nblocks, size_t lds_bytes, hipStream_t s) {
    if (!e.attr_set[i]) {
        const int rc = check_hip(hipFuncSetAttribute(reinterpret_cast<const void*>(e.k[i]), hipFuncAttributeMaxDynamicSharedMemorySize, NS_LDS_BYTES),
                                 "hipFuncSetAttribute");
        if (rc != LINNA_OK) return rc;
        e.attr_set[i] = true;
    }
    hipLaunchKernelGGL(e.k[i], dim3(nblocks), dim3(64 * NS_NW), lds_bytes, s, a);
    return check_hip(hipGetLastError(), e.what);
}
// The launch of program `p` over B rows as (variant, flags) on the engine of `rows` rows: one workgroup per `rows` rows and
// `extra` more (riders), the program's LDS (with the backward's masks for the variants that run one) and `lds_extra`.
static int ns_launch_program(NsVariant v, unsigned flags, const NsArgs& a0, int B, const NsProgram& p, int rows, hipStream_t s, int extra = 0,
                             size_t lds_extra = 0) {
    NsEntry* e = nullptr; int i = 0;
    const int rc = ns_kernel(v, flags, rows, &e, &i);
    if (rc != LINNA_OK) return rc;
#ifdef NS_STAMPS
    // diagnostic build: every launch writes its phase stamps to the buffer LINNA_FUSED_STAMPS names (tools/ns_stamps*.py)
    NsArgs a = a0;
    a.stamps = getenv("LINNA_FUSED_STAMPS") ? reinterpret_cast<unsigned long long*>(strtoull(getenv("LINNA_FUSED_STAMPS"), nullptr, 16)) : nullptr;
    if (!a.stamps) { set_error("net_stream: NS_STAMPS build needs LINNA_FUSED_STAMPS"); return LINNA_ERR_INVALID; }
#else
    const NsArgs& a = a0;
#endif
    const bool grad = v == NV_GRAD_MLP || v == NV_GRAD2 || v == NV_TRAIN_STEP;
    return ns_launch(*e, i, a, (B + rows - 1) / rows + extra, p.lds_for(rows, grad) + lds_extra, s);
}

// ------------------------------------------------------------------ AdamW that writes the weight streams itself
// A training step ends with AdamW over the flat parameter buffer and begins with two re-layouts of the updated weights
// (ns_pack_kernel: the forward + loss stream and the dX-chain stream): three launches that each read or write every
// parameter.  Here the update runs once, in the flat buffer's own order, and every thread puts its four updated values
// where the two streams want them: the forward stream holds four consecutive k of one weight row as ONE 16-byte vector
// (one store), the dX-chain stream holds the transposed matrix (four 4-byte stores; neighbouring lanes fill
// neighbouring vectors).  Biases go to the forward stream's bias block.  Constant parts of a stream (zero padding, the
// loss's inverse covariance) are written by the ordinary re-layout once and never touched here.
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
static void ns_store_table(NsArgs& a, const NsProgram& p, const NsNet& net, const NsOpBufs* ops, int lo, int hi, bool dx) {
    for (int i = lo; i < hi; ++i) {
        const int op = p.seg_op[i];
        if (op >= net.nl) continue;
        const NsOpBufs& b = ops[op];
        const linna_layer_t& l = net.layers[op];
        a.gn[i] = p.seg_hidden[i] ? l.C : dx ? l.K : l.N;   // (a dX-chain program's segments are all nseg_f)
        if (!dx) { a.gout[i] = p.seg_hidden[i] ? b.t : b.y; a.gld[i] = p.seg_hidden[i] ? b.ldt : b.ldy; }
        else if (p.seg_hidden[i]) { a.gout[i] = b.dt; a.gld[i] = b.lddt; a.gmask[i] = b.t; a.gmld[i] = b.ldt; }
        else { a.gout[i] = b.dprev; a.gld[i] = b.ldp; a.gmask[i] = b.gate; a.gmld[i] = b.ldx; }
    }
}
// the sign-bit gates (ns_gates) into the launch; false when they do not fit the LDS or a gate has no producer (*lds_extra:
// the launch's LDS beyond the program's own)
static bool ns_set_gates(NsArgs& a, const NsGates& g, const NsProgram& p, int rows, size_t* lds_extra) {
    for (int i = 0; i < NS_SEGCAP; ++i) { a.gbit[i] = g.gbit[i]; a.mbit[i] = g.mbit[i]; }
    a.nbw = g.ncols / 32;
    a.bits_off = (int)(g.lds0 / sizeof(float));
    *lds_extra = g.lds - p.lds_for(rows, true);
    return g.ok && g.lds <= (size_t)NS_LDS_BYTES;
}
static void ns_set_input(NsArgs& a, const NsInput& in) {
    a.is_flat = in.is_flat; a.a1 = in.a1; a.a2 = in.a2; a.lg = in.lg; a.xmean = in.xmean; a.xstd = in.xstd;
}
// a launch that takes its rows as they are: the prologue's transform constants are loaded and ignored -- `any` readable array
// of at least as many entries as the rows have columns stands for all of them
static void ns_set_input_ignored(NsArgs& a, const float* any) {
    a.is_flat = reinterpret_cast<const int*>(any); a.a1 = any; a.a2 = any; a.lg = nullptr; a.xmean = any; a.xstd = any;
}
static void ns_set_grad(NsArgs& a, const NsGrad& gr) {
    a.gscale = gr.gscale; a.Gout = gr.G; a.ldg = gr.ldg;
    const NsLeap& l = gr.leap;          // the one place that writes NsArgs::hm_*
    a.hm_p = l.P; a.hm_ldp = l.ldp; a.hm_q = l.Q; a.hm_mass = l.mass; a.hm_ek = l.ek; a.hm_ed = l.ed; a.hm_eps = l.eps;
}

// Whether a serving launch with these arguments takes the plain instantiation: the one decision, made here for the launch
// below and for whoever asks what it would do (linna_logprob_serve_plain).
bool net_stream_takes_plain(NsKind kind, const NsNet& net, const NsOutput& out, const NsRun& r, const NsMove* mv, const NsGrad* gr, int rows,
                            const NsDense* dn) {
    if (kind != NS_SERVE || rows != 16 || mv || gr || dn || !net_stream_serve_plain(-1)) return false;
    if (!net_stream_launch_plain_ok(out.cscale, out.cshift, out.w, out.cpost, r.lnP, r.D, r.TH, r.gate)) return false;
    return ns_program_plain(*ns_program(kind, net.layers, net.nl, net.in_size, dn, rows));
}

int launch_net_stream(NsKind kind, const NsNet& net, const float* packed, const NsRun& r, const NsInput& in, const NsOutput& out,
                      const NsMove* mv, const NsGrad* gr, int rows, const NsDense* dn, hipStream_t s) {
    const bool bf = kind == NS_SERVE_BF16;
    if ((kind == NS_SERVE_DENSE) != (dn != nullptr) || !(kind == NS_SERVE || kind == NS_SERVE_DENSE || bf)) {
        set_error("net_stream: not a serving program"); return LINNA_ERR_INVALID;
    }
    const NsProgramRef pref = ns_program(kind, net.layers, net.nl, net.in_size, dn, rows);
    const NsProgram& p = *pref;
    if ((out.cpost != nullptr) != (out.cshift2 != nullptr) || (out.cpost && (dn || gr))) {
        set_error("net_stream: the exp output map needs cpost and cshift2, and has no dense / gradient program"); return LINNA_ERR_INVALID;
    }
    if (!p.ok) { set_error("net_stream: network not eligible"); return LINNA_ERR_UNSUPPORTED; }
    if (dn && (out.w || gr || out.cscale || out.cshift)) { set_error("net_stream: the dense program carries its own output map and has no fused gradient"); return LINNA_ERR_INVALID; }
    if (mv && (in.nin > 64 || (!out.w && !dn))) { set_error("net_stream: fused sampler moves need <= 64 parameters and a log-likelihood in the launch"); return LINNA_ERR_UNSUPPORTED; }
    if (gr && (!p.grad_ok || !out.w || !r.lnP || !gr->gscale || !gr->G || mv)) { set_error("net_stream: no fused gradient for this network / likelihood"); return LINNA_ERR_UNSUPPORTED; }
    NsArgs a = ns_args(p, packed, r.Z, r.ldz, r.B, in.nin, gr != nullptr);    // forward only: stop after the forward segments
    ns_set_input(a, in);
    a.cscale = out.cscale; a.cshift = out.cshift; a.w = out.w; a.T = out.T;
    a.cpost = out.cpost; a.cshift2 = out.cshift2;
    a.dense = p.dense ? (dn && dn->factored ? 2 : 1) : 0; a.u_col = p.u_col; a.u_same = p.u_same; a.x0_keep = p.x0_keep;
    a.lnP = r.lnP; a.D = r.D; a.ldd = r.ldd; a.TH = r.TH; a.ldt = r.ldt;
    a.gate = r.gate;
    const unsigned fbf = bf ? NF_BF16 : 0;
    if (mv) {
        a.mv_coords = mv->coords; a.mv_ldc = mv->ldc; a.mv_logp = mv->logp; a.mv_S = mv->S;
        a.mv_cc = mv->cc; a.mv_ldcc = mv->ldcc; a.mv_C = mv->C; a.mv_nc = mv->nc;
        a.mv_seed = mv->seed; a.mv_step = mv->step; a.mv_step_off = mv->step_off; a.mv_stream = mv->stream; a.mv_a = mv->a; a.mv_naccept = mv->naccept;
        a.mv_chain = mv->chain; a.mv_lps = mv->lps;
        a.sl_Z0 = mv->sl_Z0; a.sl_L = mv->sl_L; a.sl_R = mv->sl_R; a.sl_Zt = mv->sl_Zt; a.sl_m = mv->sl_m; a.sl_nt = mv->sl_nt;
        a.sl_seed = mv->sl_seed; a.sl_step = mv->sl_step; a.sl_stream = mv->sl_stream; a.sl_flags = mv->sl_flags;
        if (mv->sb) a.sb = *mv->sb;
        return ns_launch_program(mv->slice ? NV_SLICE : NV_STRETCH, fbf, a, r.B, p, rows, s);
    }
    if (bf && gr) { set_error("net_stream: no bf16 gradient"); return LINNA_ERR_UNSUPPORTED; }
    if (bf) return ns_launch_program(NV_SERVE, NF_BF16, a, r.B, p, rows, s);
    if (gr) {
        ns_set_grad(a, *gr);
        return ns_launch_program(NV_GRAD_MLP, a.hm_p && a.hm_eps ? NF_EPS : 0, a, r.B, p, rows, s);
    }
    // the plain MLP's serving launch: its own lean instantiation (net_stream_plain_kernel), unless linna_serve_plain(0) --
    // with the step placed by hand (net_stream_placed_kernel) where the build has it, unless linna_serve_plain_sched(0) --
    // and without the MFMAs on zero padding (net_stream_trim_kernel: N and the live k slices of each segment's last step
    // folded in beside ncg_log2), unless linna_serve_plain_trim(0)
    if (!net_stream_takes_plain(kind, net, out, r, mv, gr, rows, dn)) return ns_launch_program(NV_SERVE, 0, a, r.B, p, rows, s);
    for (int i = 0; i < a.nseg; ++i) a.seg[i].type |= a.seg[i].ncg_log2 << 8;      // (the eight fields it reads: net_stream_body.inc)
#ifdef NS_HAVE_TRIM
    if (net_stream_serve_plain_sched(-1) && net_stream_serve_plain_trim(-1)) {
        for (int i = 0; i < a.nseg; ++i) a.seg[i].type |= ns_trim_fold(p, i);
        return ns_launch_program(NV_SERVE, NF_PLAIN | NF_PLACED | NF_TRIM, a, r.B, p, rows, s);
    }
#endif
#ifdef NS_HAVE_PLACED
    if (net_stream_serve_plain_sched(-1)) return ns_launch_program(NV_SERVE, NF_PLAIN | NF_PLACED, a, r.B, p, rows, s);
#endif
    return ns_launch_program(NV_SERVE, NF_PLAIN, a, r.B, p, rows, s);
}

// Training / validation forward: X[B][ldx] (transformed inputs) -> every op's output (`ops[i].y`, the hidden h of a
// residual block `ops[i].t`) in global memory.
int launch_net_stream_store(const NsNet& net, const float* packed, const float* X, int ldx, int B, const NsOpBufs* ops,
                            const float* cscale, const float* cshift, int rows, hipStream_t s) {
    const NsProgramRef pref = ns_program(NS_STORE, net.layers, net.nl, net.in_size, nullptr, rows);
    const NsProgram& p = *pref;
    if (!p.ok) { set_error("net_stream: network not eligible"); return LINNA_ERR_UNSUPPORTED; }
    NsArgs a = ns_args(p, packed, X, ldx, B, net.in_size, false);
    ns_set_input_ignored(a, X);
    a.cscale = cscale; a.cshift = cshift;                   // column affine of the last output (Y transforms), or null
    ns_store_table(a, p, net, ops, 0, p.nseg_f, false);
    return ns_launch_program(NV_STORE, 0, a, B, p, rows, s);
}


// lnP and d lnP / d z in ONE launch for any network the forward and dX-chain programs cover (GRAD + STORE == 2): the
// forward segments keep the signs of the activations the gates need (ns_gates; round 2 kept the activations themselves in
// the caller's workspace: 40 MB written and read back per 4096-chain launch of ChtoModelv2(33,33), in bursts at the run
// ends of 256 workgroups in step, each read an exposed L2 round trip behind a drained weight ring), the turnaround forms
// d lnP / d out, the dX chain runs down to the network input gating on those signs, the finish applies the prior map's
// derivative.  Diagonal covariance.  bf: the same on a bf16 stream (NS_GRAD_INPUT_BF16, net_stream_grad_bf16_kernel).
int launch_net_stream_grad2(const NsNet& net, const float* packed, const NsRun& r, const NsInput& in, const NsOutput& out, const NsGrad& gr,
                            int rows, hipStream_t s, bool bf) {
    const NsProgramRef pref = ns_program(bf ? NS_GRAD_INPUT_BF16 : ns_grad_kind(net.layers, net.nl), net.layers, net.nl, net.in_size, nullptr, rows);
    const NsProgram& p = *pref;
    if (!p.ok || !p.dxi_ok) { set_error("net_stream: no forward + dX program for this network"); return LINNA_ERR_UNSUPPORTED; }
    if (!out.w || !r.lnP || !gr.gscale || !gr.G) { set_error("net_stream: the one-launch gradient needs a diagonal covariance"); return LINNA_ERR_INVALID; }
    NsArgs a = ns_args(p, packed, r.Z, r.ldz, r.B, in.nin, true);
    ns_set_input(a, in);
    a.cscale = out.cscale; a.cshift = out.cshift; a.w = out.w; a.T = out.T; a.lnP = r.lnP;     // (no exp output map here)
    ns_set_grad(a, gr);
    const NsGates g = ns_gates(p, net.layers, net.nl, rows);
    for (int i = 0; i < (int)p.seg.size(); ++i) if (i >= p.nseg_f || g.gbit[i] >= 0) a.gn[i] = ns_seg_cols(p, net.layers, i);
    size_t lds_extra = 0;
    if (!ns_set_gates(a, g, p, rows, &lds_extra)) {
        set_error(g.ok ? "net_stream: the one-launch gradient's sign bits do not fit the LDS" : "net_stream: a gate of the one-launch gradient has no producer");
        return LINNA_ERR_UNSUPPORTED;
    }
    // wide: the turnaround's tail over the columns past its registers (fp32 only: the bf16 program keeps the 64-output limit)
    const unsigned flags = (bf ? NF_BF16 : p.nout > 64 ? NF_WIDE : 0) | (a.hm_p && a.hm_eps ? NF_EPS : 0);
    return ns_launch_program(NV_GRAD2, flags, a, r.B, p, rows, s, 0, lds_extra);
}

// The same for a dense inverse covariance S = L L^T (NS_GRAD_INPUT_DENSE, net_stream_dense_kernel): the stream carries the
// output map (folded into the last layer, forward and backward) and L twice -- U = d L in front of the turnaround, its
// transpose behind it -- so the launch takes no output map, no likelihood weights and no gscale.
int launch_net_stream_grad_dense(const NsNet& net, const float* packed, const NsRun& r, const NsInput& in, float T, const NsGrad& gr,
                                 int rows, const NsDense& dn, hipStream_t s) {
    const NsProgramRef pref = ns_program(NS_GRAD_INPUT_DENSE, net.layers, net.nl, net.in_size, &dn, rows);
    const NsProgram& p = *pref;
    if (!p.ok || !p.dxi_ok || !p.dense || !dn.factored) { set_error("net_stream: no dense forward + dX program for this network"); return LINNA_ERR_UNSUPPORTED; }
    if (!r.lnP || !gr.G) { set_error("net_stream: the dense one-launch gradient needs lnP and G"); return LINNA_ERR_INVALID; }
    NsArgs a = ns_args(p, packed, r.Z, r.ldz, r.B, in.nin, true);
    ns_set_input(a, in);
    a.T = T; a.lnP = r.lnP;
    a.dense = 2; a.u_col = p.u_col; a.u_same = p.u_same;
    ns_set_grad(a, gr);
    a.gscale = nullptr;
    const NsGates g = ns_gates(p, net.layers, net.nl, rows);
    for (int i = 0; i < (int)p.seg.size(); ++i) if (i >= p.nseg_f || g.gbit[i] >= 0) a.gn[i] = ns_seg_cols(p, net.layers, i);
    size_t lds_extra = 0;
    if (!ns_set_gates(a, g, p, rows, &lds_extra)) {
        set_error(g.ok ? "net_stream: the dense one-launch gradient does not fit the LDS of this engine" : "net_stream: a gate of the dense one-launch gradient has no producer");
        return LINNA_ERR_UNSUPPORTED;
    }
    return ns_launch_program(NV_GRAD2, NF_DENSE | (a.hm_p && a.hm_eps ? NF_EPS : 0), a, r.B, p, rows, s, 0, lds_extra);
}

// the forward + loss half of a training launch (STORE == 3): the batch rows ROWS (null: 0..B-1) of X gathered and
// X-transformed into XB, every activation stored, the loss rows and d loss / d pred written
static NsArgs ns_train_args(const NsProgram& p, bool full, const NsNet& net, const float* packed, const NsBatch& b, const NsOpBufs* ops,
                            const NsTrainLoss& L) {
    NsArgs a = ns_args(p, packed, b.X, b.ldx, b.B, net.in_size, full);
    ns_set_input_ignored(a, b.xmean);              // (the prior map's constants; the input transform is real)
    a.lg = b.lg; a.xstd = b.xstd;
    a.dense = p.dense; a.u_col = p.u_col; a.u_same = p.u_same;
    ns_store_table(a, p, net, ops, 0, p.nseg_f, false);
    a.t_rows = b.ROWS; a.t_xb = b.XB; a.t_ldxb = b.ldxb;
    a.t_Y = L.YN; a.t_ldy = L.ldyn;
    a.t_den = L.den; a.t_inv_batch = L.inv_batch; a.t_loss_rows = L.loss_rows; a.t_dP = L.dP; a.t_lddp = L.lddp;
    return a;
}

// Training forward + loss in one launch (STORE == 3); `dn` = {Cinv, ldc, null, null}: the inverse covariance in the
// network's normalised output space as the last segment.
int launch_net_stream_train(const NsNet& net, const float* packed, const NsBatch& b, const NsOpBufs* ops, const NsTrainLoss& L,
                            const NsDense& dn, int rows, hipStream_t s) {
    const NsProgramRef pref = ns_program(NS_TRAIN_FWD, net.layers, net.nl, net.in_size, &dn, rows);
    const NsProgram& p = *pref;
    if (!p.ok || !p.dense) { set_error("net_stream: network + loss not eligible"); return LINNA_ERR_UNSUPPORTED; }
    const NsArgs a = ns_train_args(p, false, net, packed, b, ops, L);
    return ns_launch_program(NV_TRAIN_FWD, 0, a, b.B, p, rows, s);
}

// A training step's network work in ONE launch (TRB: GRAD + STORE == 3): launch_net_stream_train's forward + loss, its
// finish as the turnaround, then launch_net_stream_dx's chain down to op 1 -- same arguments as the two of them; the gates
// of the backward half are sign bits in LDS (ns_gates: the activations go to memory all the same, the parameter
// gradients read them, but no gate is read back from there).  `post`: only the AdamW step constants ride here (the loss
// rows are not complete before every workgroup's turnaround: the batch mean rides in the parameter-gradient launch instead).
int launch_net_stream_train_bwd(const NsNet& net, const float* packed, const NsBatch& b, const NsOpBufs* ops, const NsTrainLoss& L,
                                const NsDense& dn, int rows, hipStream_t s, const NsPost* post, bool bf) {
    const NsProgramRef pref = ns_program(bf ? NS_TRAIN_STEP_BF16 : NS_TRAIN_STEP, net.layers, net.nl, net.in_size, &dn, rows);
    const NsProgram& p = *pref;
    if (!p.ok || !p.train_ok || !p.dense) { set_error("net_stream: network + loss have no one-launch training program"); return LINNA_ERR_UNSUPPORTED; }
    if (rows != 4) { set_error(bf ? "net_stream: the bf16 training step runs on the 4-row engine (batches of up to 1024 rows)"
                                  : "net_stream: the one-launch training step runs on the 4-row engine"); return LINNA_ERR_UNSUPPORTED; }
    NsArgs a = ns_train_args(p, true, net, packed, b, ops, L);
    ns_store_table(a, p, net, ops, p.nseg_f, (int)p.seg.size(), true);
    const NsGates g = ns_gates(p, net.layers, net.nl, rows);
    size_t lds_extra = 0;
    if (!ns_set_gates(a, g, p, rows, &lds_extra)) {
        set_error(g.ok ? "net_stream: the training step's sign bits do not fit the LDS" : "net_stream: a gate of the one-launch training step has no producer");
        return LINNA_ERR_UNSUPPORTED;
    }
    int extra = 0;
    if (post && post->step) { a.p_step = post->step; a.p_hyper = post->hyper; a.p_b1 = post->b1; a.p_b2 = post->b2; extra = 1; }
    return ns_launch_program(NV_TRAIN_STEP, bf ? NF_BF16 : 0, a, b.B, p, rows, s, extra, lds_extra);
}

// The dX chain of a training step in one launch (what linna_net_backward otherwise runs as one GEMM per op):
// dOUT[B][lddo] -> for every op i >= first (1, or 0 with_input) the gradient with respect to its input, gated by that input
// where it went through a ReLU, into ops[i].dprev; for residual blocks also d/dh into ops[i].dt, gated by the stored h.
int launch_net_stream_dx(const NsNet& net, const float* packed, const float* dOUT, int lddo, int B, const NsOpBufs* ops, int with_input,
                         int rows, hipStream_t s, const NsPost* post) {
    const NsProgramRef pref = ns_program(with_input ? NS_DX_INPUT : NS_DX, net.layers, net.nl, net.in_size, nullptr, rows);
    const NsProgram& p = *pref;
    if (!p.ok) { set_error("net_stream: no dX-chain program for this network"); return LINNA_ERR_UNSUPPORTED; }
    NsArgs a = ns_args(p, packed, dOUT, lddo, B, net.layers[net.nl - 1].N, false);
    ns_set_input_ignored(a, dOUT);
    ns_store_table(a, p, net, ops, 0, p.nseg_f, true);
    const bool rider = post && post->n > 0;       // the rider (see NsArgs::p_rows): one more workgroup
    if (rider) {
        a.p_rows = post->rows; a.p_n = post->n; a.p_scale = post->scale; a.p_out = post->out;
        a.p_step = post->step; a.p_hyper = post->hyper; a.p_b1 = post->b1; a.p_b2 = post->b2;
    }
    return ns_launch_program(NV_DX, 0, a, B, p, rows, s, rider ? 1 : 0);
}
}  // namespace linna
