// The planner of the whole-network kernel: pure host code that turns a linna_layer_t list into the segment program
// net_stream.hip's kernels run (net_program.h).  No kernel and no launch here: everything in this file runs on a box
// without a GPU (linna_program_describe, tests/test_net_program_host.py).
#include "net_program.h"
#include <stdlib.h>
#include <algorithm>
#include <atomic>
#include <cstring>
#include <mutex>
#include <string>
#include <unordered_map>

namespace linna {

size_t NsProgram::lds_for(int rows, bool grad) const {
    size_t b = (size_t)(2 * rows * LD + ((bias_total + 3) & ~3)) * sizeof(float) + 128 + (x0_keep ? 4096 : 0);   // + [16] set rows, [16] den (STORE == 3), kept input rows
#ifdef NS_STAMPS
    b += NS_NW * 32 * 8;                                    // (the diagnostic build: net_stream.hip is compiled with the same definition)
#endif
    return b + (grad ? (size_t)mask_slots * 64 * NS_NW * sizeof(unsigned) : 0);
}

static int ceil16(int k) { return (k + 15) & ~15; }
int ns_seg_steps(const NsSeg& s) {
    if (s.type == NS_WIDE && s.zext < 0) return 2 * s.steps - 60;
    return s.type == NS_WIDE && s.zext > 0 ? s.steps + (s.passes - 1) * s.zext : s.steps * s.passes;
}
// A process-wide switch whose initial value is the environment's, read ONCE (-1: not read yet; anything but `valid`: dflt)
// -- the launch path reads an atomic, not the environment.
static int ns_switch(std::atomic<int>& sw, const char* name, int dflt, bool (*valid)(int)) {
    int v = sw.load(std::memory_order_relaxed);
    if (v < 0) {
        const char* const env = getenv(name);
        v = env && valid(atoi(env)) ? atoi(env) : dflt;
        int expect = -1;
        sw.compare_exchange_strong(expect, v);
        v = sw.load(std::memory_order_relaxed);
    }
    return v;
}
static std::atomic<int> g_dense_tri{-1};
int net_stream_dense_tri(int mode) {
    const int prev = ns_switch(g_dense_tri, "LINNA_DENSE_TRI", 2, [](int v) { return v >= 0 && v <= 2; });
    if (mode >= 0 && mode <= 2) g_dense_tri.store(mode);
    return prev;
}

// ---------------------------------------------------------------------------- building a program
// The backward half behind the forward segments, in the same stream
enum NsBackward {
    NS_BWD_NONE,
    NS_BWD_MLP,      // the fused gradient of plain ReLU MLPs, gated by sign-bit slots; a network without one gets the forward-only program
    NS_BWD_INPUT,    // the dX chain down to the network input -- lnP and d lnP / d z in one launch for ANY network (residual
                     // blocks, SPLIT segments): the backward segments gate on the forward ones' signs (GRAD + STORE == 2)
    NS_BWD_TRAIN     // the dX chain down to op 1 behind the loss segment: the merged training step
};
// What ns_build_one is asked for; ns_build_kind fills one per NsKind.
struct NsBuildOpts {
    // forward = false: the dX chain of a training step as a program of its own (linna_net_backward's order): the rows are
    // d loss / d output, the segments run over the transposed weights from the last op down to op dx_first (1, or 0: the
    // network input).  A residual block y = relu(0.1 (W2 h + b2) + Ws x), h = relu(W1 x + b1) comes back as
    // dh = 0.1 (dy W2) [h > 0], written behind dy, and ONE GEMM over [dy ; dh] with [Ws^T | W1^T]; the gate of every output
    // (the stored forward activation) is applied by the kernel's STORE == 2 epilogue.
    bool forward = true; int dx_first = 1;
    // the output map (d = raw * cscale + cshift) folded into the last layer's weights and bias, and the dense inverse
    // covariance (NsDense) appended as one more bias-free segment U = d S -- the Gaussian log-likelihood (util.py:953-955)
    // with a dense covariance, or the training loss, then needs no GEMM launch of its own
    bool dense = false;
    NsBackward bwd = NS_BWD_NONE;
    // SPLIT segments of <= 32 columns become SIDE segments where they fit (see NsPackArgs): the kernel's K4 path, i.e. the
    // 16-row engine of the programs ns_side names
    bool side = false;
    // the bf16 programs (serving without a dense segment, the merged training step, the one-launch gradient; no SIDE segments): a step is 32 k, and the
    // first layer (a plain linear map) is [W | W] over K' = 2 nin -- its input rows are x_hi = bf16(x) and x_lo = x - x_hi
    bool bf = false;
    // NS_GRAD_INPUT_WIDE: more than 64 network outputs behind the forward half of an NS_BWD_INPUT program
    bool wide_out = false;
};

// One linear map of a program: [Wa | alpha Wb] over K = [Kapad ; Kb], N outputs, written to dst_col (same_buf: into the
// input's buffer)
struct Lin {
    const float* Wa = nullptr; int lda = 0, Ka = 0, Kapad = 0;
    const float* Wb = nullptr; int ldb = 0, Kb = 0; float alpha = 0.f;
    const float* b = nullptr; float bscale = 0.f;
    int N = 0, relu = 0, dst_col = 0; bool same_buf = false;
    int transA = 0, transB = 0, force_wide = 0, mask_apply_of = -1, op = -1;
    const float* rscale = nullptr; const float* rshift = nullptr;
    const float* b2 = nullptr; float b2scale = 0.f; int x0_col = 0;
    const float* kscale = nullptr;     // NsPackSeg::kscale
    bool no_bias = false;              // a bias-free map that is not read transposed: it shares the block of zeros all the same
};
static int ld4(int k) { return (k + 3) & ~3; }              // row stride of a [N][k] weight matrix (LINNA_LD)
static Lin lin_over(const float* W, int ldw, int K, int N, int op) {   // the first K part alone: N outputs of W over K input columns
    Lin L; L.Wa = W; L.lda = ldw; L.Ka = K; L.Kapad = ceil16(K); L.N = N; L.op = op; return L;
}
static Lin lin_layer(const linna_layer_t& l, int op) {   // y = [relu](W x + b)
    Lin L = lin_over(l.W, ld4(l.K), l.K, l.N, op); L.b = l.b; L.bscale = 1.f; L.relu = l.relu; return L;
}
static Lin lin_block_hidden(const linna_layer_t& l, int op) {   // h = relu(W1 x + b1), written behind x
    Lin L = lin_over(l.W1, ld4(l.K), l.K, l.C, op); L.b = l.b1; L.bscale = 1.f; L.relu = 1; L.dst_col = L.Kapad; L.same_buf = true; return L;
}
static Lin lin_block_out(const linna_layer_t& l, int op) {   // y = relu([Ws | 0.1 W2] [x ; h] + 0.1 b2)
    Lin L = lin_over(l.Ws, ld4(l.K), l.K, l.N, op); L.Wb = l.W2; L.ldb = ld4(l.C); L.Kb = l.C; L.alpha = 0.1f; L.b = l.b2; L.bscale = 0.1f; L.relu = 1; return L;
}
// backward maps (no bias): dx = W^T dy over the N columns of dy; a block's dh = 0.1 W2^T dy behind dy, its dx = [Ws^T | W1^T] [dy ; dh]
static Lin lin_transposed(const float* W, int ldw, int N, int K, int op) { Lin L = lin_over(W, ldw, N, K, op); L.transA = 1; return L; }
static Lin lin_block_dh(const linna_layer_t& l, int op) {
    Lin L; L.Wb = l.W2; L.ldb = ld4(l.C); L.Kb = l.N; L.alpha = 0.1f; L.transB = 1; L.N = l.C; L.dst_col = ceil16(l.N); L.same_buf = true; L.op = op; return L;
}
static Lin lin_block_dx(const linna_layer_t& l, int op) {
    Lin L = lin_transposed(l.Ws, ld4(l.K), l.N, l.K, op); L.Wb = l.W1; L.ldb = ld4(l.K); L.Kb = l.C; L.alpha = 1.f; L.transB = 1; return L;
}
// U = d S behind the last layer (SPLIT, <= 256 columns: behind d in the same buffer).  factored: the matrix is L (S = L L^T,
// not symmetric) and the segment must produce d L: U_n = sum_k d_k L[k][n] -- the pack kernel reads it transposed (the
// row-dot GEMM of the layered path reads S[k][n] as it is)
static Lin lin_dense(const NsDense& dn, int nout, int op) {
    Lin L = lin_over(dn.S, dn.lds, nout, nout, op); L.same_buf = nout <= 256; L.dst_col = L.same_buf ? L.Kapad : 0; L.transA = dn.factored ? 1 : 0; return L;
}
// its transpose behind the turnaround of NS_GRAD_INPUT_DENSE: d/dd_k = sum_n (d/dU_n) L[k][n], from column 0 of the current
// buffer (where the turnaround put d/dU) like every other backward map -- L as it lies in memory, no bias
static Lin lin_dense_back(const NsDense& dn, int nout, int op) {
    Lin L = lin_over(dn.S, dn.lds, nout, nout, op); L.no_bias = true; return L;
}

// ---- 1. lowering: layer list -> linear maps
struct NsLowered {
    std::vector<Lin> lins;
    int nfwd = 0;                      // forward maps (a dX chain on its own: all of them)
    int f32seg = -1;                   // bf16 stream: the map that stays an fp32 run (the training step's loss segment)
    int x0_keep = 0, dense = 0, u_col = 0, u_same = 0;      // as in NsProgram
    bool mlp_grad = false;             // the maps allow the fused MLP gradient (ns_append_mlp_grad decides on their segments)
    bool ok = false;
};
static bool ns_layer_ok(const linna_layer_t& l, int width) {       // a LINEAR or RESBLOCK op over `width` input columns that fits
    if (l.K != width || l.N < 1 || l.N > 1024) return false;
    if (l.op == LINNA_OP_LINEAR) return l.alpha == 1.f;
    return l.op == LINNA_OP_RESBLOCK && l.C >= 1 && l.C <= 64 && (l.Ws || l.K == l.N);
}
static void ns_push_dx(std::vector<Lin>& lins, const linna_layer_t* layers, int nl, int first) {
    for (int i = nl - 1; i >= first; --i) {
        const linna_layer_t& l = layers[i];
        if (l.op == LINNA_OP_LINEAR) lins.push_back(lin_transposed(l.W, ld4(l.K), l.N, l.K, i));
        else { lins.push_back(lin_block_dh(l, i)); lins.push_back(lin_block_dx(l, i)); }
    }
}
static bool ns_push_forward(std::vector<Lin>& lins, int* x0_keep, const linna_layer_t* layers, int nl, int in_size) {
    int width = in_size;
    for (int i = 0; i < nl; ++i) {
        const linna_layer_t& l = layers[i];
        if (l.op != LINNA_OP_INSKIP) {
            if (!ns_layer_ok(l, width)) return false;
            if (l.op == LINNA_OP_LINEAR) lins.push_back(lin_layer(l, i));
            else { lins.push_back(lin_block_hidden(l, i)); lins.push_back(lin_block_out(l, i)); }
        } else {
            // out = last(h) + alpha (x0 Wl^T + bl) (nn.py:195): the last layer becomes ONE GEMM over [h ; x0] with [W | alpha Wl]
            // and bias b + alpha bl; x0 (the network input, kept in LDS) is copied behind h before the segment runs
            if (i != nl - 1 || lins.empty() || l.K != in_size || l.N != width || in_size > 64) return false;
            Lin& last = lins.back();
            if (last.Wb || last.same_buf || last.relu || !last.Wa) return false;
            last.Wb = l.W; last.ldb = ld4(l.K); last.Kb = l.K; last.alpha = l.alpha;
            last.b2 = l.b; last.b2scale = l.alpha; last.x0_col = last.Kapad;
            *x0_keep = 1;
            continue;
        }
        width = l.N;
    }
    return true;
}
// Backward (d lnP / d z) for plain ReLU MLPs whose hidden layers come out as WIDE segments: the backward GEMM of layer l is
// a forward-shaped segment over W_l^T (contraction N_l, K_l outputs); for l >= 1 it is forced WIDE so that its lane <->
// (row, column) map equals that of the layer whose sign bits it applies.
static bool ns_mlp_grad_maps_ok(const std::vector<Lin>& lins, int in_size) {
    const int nfwd = (int)lins.size();
    if (in_size > 64 || lins.back().N > 64 || 2 * nfwd > NS_MAXSEG) return false;
    for (int i = 0; i < nfwd; ++i) {
        const Lin& L = lins[i];
        if (L.Wb || L.same_buf || L.dst_col || !L.Wa) return false;
        if (i < nfwd - 1 && (!L.relu || L.N <= 256)) return false;            // hidden layers must be WIDE (N > 256)
    }
    return true;
}
static NsLowered ns_lower(const linna_layer_t* layers, int nl, int in_size, const NsBuildOpts& o, const NsDense* dn) {
    NsLowered r;
    std::vector<Lin>& lins = r.lins;
    const bool train = o.bwd == NS_BWD_TRAIN, dxi = o.bwd == NS_BWD_INPUT;
    if (o.dense && (!dn || !dn->S)) return r;
    if (nl < 1 || in_size < 1 || in_size > 256) return r;
    if (!o.forward || dxi || train)                         // (a program with a dX chain takes no input skip)
        for (int i = 0, width = in_size; i < nl; width = layers[i++].N) if (!ns_layer_ok(layers[i], width)) return r;
    if (!o.forward) {
        ns_push_dx(lins, layers, nl, o.dx_first);
        in_size = layers[nl - 1].N;                         // the rows of this program are d loss / d output
    } else if (!ns_push_forward(lins, &r.x0_keep, layers, nl, in_size)) return r;
    // (the dense one-launch gradient alone may fill the tables: ChtoModelv2's is 22 segments; every other kind keeps its limit)
    const int maxseg = o.dense && dxi ? NS_SEGCAP : NS_MAXSEG;
    if (lins.empty() || lins.back().relu || (int)lins.size() > maxseg) return r;
    if (o.bf) {                                             // [x_hi ; x_lo]: the first layer twice, no padding between the halves
        Lin& f = lins[0];
        if (f.Wb || f.same_buf || f.transA || !f.Wa || f.Ka != in_size || f.x0_col) return r;
        f.Kapad = in_size; f.Wb = f.Wa; f.ldb = f.lda; f.Kb = f.Ka; f.alpha = 1.f;
    }
    if (o.dense) {
        Lin& last = lins.back();
        if (last.Wb || last.same_buf || last.dst_col) return r;               // the last op must be a plain linear layer
        last.rscale = dn->cscale; last.rshift = dn->cshift;
        if ((int)lins.size() + 1 > maxseg) return r;
        const Lin Q = lin_dense(*dn, last.N, nl);
        lins.push_back(Q);
        r.dense = 1; r.u_col = Q.dst_col; r.u_same = Q.same_buf ? 1 : 0;
    }
    r.nfwd = (int)lins.size();
    if (o.bf && train) r.f32seg = r.nfwd - 1;
    if (dxi) {
        // the prologue / turnaround constants are held for <= 64 columns; the wide-output instantiations of the fp32 kernel
        // (net_stream_wide_kernel) read the output's beyond 64 from memory -- a program kind of its own
        if (in_size > 64) return r;
        if (o.dense) {
            // NS_GRAD_INPUT_DENSE: the turnaround works on U = d L in LDS at any width and leaves d lnP / dU at column 0; the
            // transposed dense map takes it back to d lnP / dd, and the chain's first map (the last layer's transpose) carries
            // the folded output map's scale per contraction index, as the forward one carries it per column
            if (!dn->factored) return r;
            lins.push_back(lin_dense_back(*dn, lins.back().N, nl));
        } else if ((lins.back().N > 64) != o.wide_out) return r;
        const size_t first_dx = lins.size();
        ns_push_dx(lins, layers, nl, 0);
        if (o.dense) lins[first_dx].kscale = dn->cscale;
    }
    if (train) {                                               // the turnaround works on the rows in LDS: any width
        if (nl < 2) return r;
        ns_push_dx(lins, layers, nl, 1);
    }
    if ((int)lins.size() > maxseg) return r;
    r.mlp_grad = o.bwd == NS_BWD_MLP && ns_mlp_grad_maps_ok(lins, in_size);
    r.ok = true;
    return r;
}

// ---- 2. shaping: one linear map -> its segment, its pack record and the extent of the input it reads.  SPLIT when it must
//      write into its own input buffer (h of a residual block) or when splitting K over the idle waves saves at least three
//      steps; WIDE otherwise; SIDE as NsBuildOpts says.
struct NsShaper {                      // the segment list so far: bias block in floats, weight stream in steps, the shared block of zeros
    std::vector<NsSeg> seg; std::vector<NsPackSeg> pack; std::vector<int> in_ext;
    int bias_off = 0, G = 0, zero_off = -1, zero_pad = 0;
};
struct NsShapeCtx { const NsBuildOpts& o; const NsDense* dn; int nfwd, f32seg;
                    bool last_side;      // the last forward segment may be a SIDE one: nothing follows it in the launch
                    int x0_seg; };       // the input-skip segment (-1: none).  Its predecessor is never a SIDE one: the kernel copies the kept
                                         // input rows behind a segment's input at the end of the step-loop run before it, and a SIDE run in
                                         // between would leave that segment without them (and overwrite the columns with zeros)
static bool ns_shape(NsShaper& sh, const Lin& L, const NsShapeCtx& c) {
    const int i = (int)sh.seg.size();
    // k per step: 32 in a bf16 stream, but for the training step's loss segment (the dense inverse covariance behind the
    // last layer), an fp32 run inside it
    const int KS = c.o.bf && i != c.f32seg ? 32 : 16;
    const int ksteps = KS == 32 ? (L.Kapad + L.Kb + 31) / 32 : (L.Kapad + ceil16(L.Kb)) / 16;
    NsSeg s; NsPackSeg q;
    std::memset(&s, 0, sizeof(s));
    s.relu = L.relu; s.dst_col = L.dst_col; s.bias_off = sh.bias_off;
    const int passes = (L.N + 511) / 512;
    const int ncg = L.N <= 64 ? 1 : L.N <= 128 ? 2 : L.N <= 256 ? 4 : 0;
    const int split_steps = ncg ? (ksteps + NS_NW / ncg - 1) / (NS_NW / ncg) : 0;
    const bool split = ncg && !L.force_wide && (L.same_buf || split_steps + 3 <= ksteps * passes);
    if (L.same_buf && !ncg) return false;
    const int kc = L.N <= 16 ? 4 : L.N <= 32 ? 2 : 1;
    const int side_steps = (ksteps + NS_NW * kc - 1) / (NS_NW * kc);
    // (never the first segment nor the last forward one: the kernel runs a SIDE segment between two runs of the step loop;
    // kc = 1, <= 64 columns: the SPLIT mapping itself, run out of the stream -- 250 -> 64 is two steps per wave)
    // ... and, in the one-launch gradient, d/dh of a residual block (0.1 dy W2 gated by h: 500 / 250 / 125 -> 16 / 32 / 64,
    // the second K part alone, read transposed): one SIDE step each instead of 4 / 2 / 1 SPLIT steps and a SPLIT boundary
    // (the LAST forward segment too where nothing follows it in the launch -- serving programs without a backward half:
    // ChtoModelv2's 33 -> 33 last layer is one SIDE step instead of a three-step WIDE run)
    const bool side_fwd = (i < c.nfwd - 1 || (i == c.nfwd - 1 && c.last_side)) && !L.Wb && !L.transA && L.Wa;
    const bool side_bwd = c.o.bwd == NS_BWD_INPUT && i > c.nfwd && !L.Wa && L.Wb && L.transB && L.Kapad == 0 && !L.relu;
    const bool side_pays = split || (side_fwd && !L.force_wide && side_steps < ksteps * passes);   // (a short WIDE run of <= 64 columns)
    const bool side = c.o.side && side_pays && ncg == 1 && side_steps <= 2 && i > 0 && (side_fwd || side_bwd) && sh.seg.back().type != NS_SIDE &&
                      !L.rscale && !L.rshift && !L.b2 && !L.x0_col && i + 1 != c.x0_seg;
    int in_ext;
    if (side) {
        s.type = NS_SIDE; s.steps = side_steps; s.passes = 1; s.kslice = 16 * kc * s.steps;
        s.ncg_log2 = 0; s.kcl = kc == 4 ? 2 : kc == 2 ? 1 : 0;
        s.zext = 64;
        in_ext = NS_NW * s.kslice;
        q.bias_pad = 64; q.ncg = 1;
    } else if (split) {
        s.type = NS_SPLIT; s.steps = split_steps; s.passes = 1; s.kslice = KS * s.steps;
        s.ncg_log2 = ncg == 1 ? 0 : ncg == 2 ? 1 : 2;
        s.zext = 64 * ncg;
        in_ext = (NS_NW / ncg) * s.kslice;
        q.bias_pad = 64 * ncg; q.ncg = ncg;
    } else {
        s.type = NS_WIDE; s.steps = ksteps; s.passes = passes;
        in_ext = KS * ksteps;
        q.bias_pad = 512 * passes; q.ncg = 1;
    }
    q.Wa = L.Wa; q.lda = L.lda; q.Ka = L.Ka; q.Kapad = L.Kapad; q.Wb = L.Wb; q.ldb = L.ldb; q.Kb = L.Kb; q.alpha = L.alpha;
    q.b = L.b; q.bscale = L.bscale; q.N = L.N; q.type = s.type; q.steps = s.steps; q.passes = s.passes; q.bias_off = sh.bias_off;
    q.transA = L.transA; q.transB = L.transB; q.rscale = L.rscale; q.rshift = L.rshift; q.b2 = L.b2; q.b2scale = L.b2scale;
    q.kc = side ? kc : 1; q.side_off = 0; q.kscale = L.kscale;
    s.x0_col = L.x0_col; s.x0_n = L.x0_col ? ceil16(L.Kb) : 0;
    if ((L.transA || L.no_bias) && c.o.forward) {           // transposed segments have no bias (a dX chain on its own: none has one)
        if (sh.zero_off < 0) { sh.zero_off = sh.bias_off; sh.zero_pad = 0; }
        s.bias_off = q.bias_off = sh.zero_off;
        const int grow = std::max(0, q.bias_pad - sh.zero_pad);
        sh.zero_pad += grow; q.bias_pad = grow;             // (the first backward segment's record carries the block; later ones extend it)
    }
    sh.bias_off += q.bias_pad;
    // the Cholesky factor of a dense inverse covariance (NsDense::factored) is lower triangular: in the second pass (columns
    // >= 512) the rows k < 512 are zero -- that pass starts at k = 512 (bit-identical: the skipped products are zeros)
    // tri = 2 and exactly 16 column blocks (960 < nout <= 1024): the balanced assignment instead (ns_seg_steps) -- the zero
    // rows of EVERY 64-column block are skipped, not only those of the second pass, and every wave runs the same number
    // of steps: 66 instead of 94 at nout = 1000
    if (c.dn && c.dn->tri > 0 && s.type == NS_WIDE && c.dn->factored && L.Wa == c.dn->S && L.transA && passes == 2 && ksteps > 32 && c.o.bwd != NS_BWD_TRAIN) {
        if (c.dn->tri == 2 && (L.N + 63) / 64 == 16 && ksteps > 60) s.zext = -1;
        else { s.kslice = 512; s.zext = ksteps - 32; }
    }
    q.koff2 = s.type == NS_WIDE ? (s.zext < 0 ? -1 : s.kslice) : 0;
    if (!side) sh.G += ns_seg_steps(s);                     // (a SIDE segment is not part of the weight stream)
    sh.seg.push_back(s); sh.pack.push_back(q); sh.in_ext.push_back(in_ext);
    return true;
}

// ---- the fused MLP gradient: the backward maps of ns_mlp_grad_maps_ok's network, appended only where every hidden forward
//      segment and the backward segment that applies its sign bits came out WIDE with the same passes (one slot per pass of
//      every hidden forward segment; the backward segment of layer i + 1 applies them).  Returns the slots, -1: not appended.
static int ns_append_mlp_grad(NsShaper& sh, std::vector<Lin>& lins, const NsShapeCtx& c) {
    const int nfwd = c.nfwd;
    NsShaper t = sh;                                        // shaped on a copy: the program keeps it whole or not at all
    std::vector<Lin> bwd;
    int slot = 0;
    for (int i = 0; i < nfwd - 1; ++i) {
        if (t.seg[i].type != NS_WIDE) return -1;
        t.seg[i].mask_store = 1 + slot;
        slot += t.seg[i].passes;
    }
    for (int i = nfwd - 1; i >= 0; --i) {
        Lin Bk = lin_transposed(lins[i].Wa, lins[i].lda, lins[i].N, lins[i].Ka, -1);
        Bk.force_wide = i >= 1; Bk.mask_apply_of = i - 1;
        if (!ns_shape(t, Bk, c)) return -1;
        NsSeg& s = t.seg.back();
        if (i >= 1) {
            if (s.type != NS_WIDE || s.passes != t.seg[i - 1].passes) return -1;
            s.mask_apply = t.seg[i - 1].mask_store;
        }
        bwd.push_back(Bk);
    }
    sh = std::move(t);
    lins.insert(lins.end(), bwd.begin(), bwd.end());
    return slot;
}

// ---- 3. every column a segment reads must have been WRITTEN (finite; zero where the weights are zero): track the defined
//      prefix [0, def) of the current buffer and widen the zero fill of the last SPLIT writer (or of the prologue: kpad0)
//      where a consumer reads further.  *maxext: the widest row any segment reads or writes.
static bool ns_written_columns(NsProgram& p, const std::vector<int>& in_ext, int* maxext) {
    p.kpad0 = in_ext[0];
    int def = p.kpad0, writer = -1;                         // writer: segment whose write ends at `def` (-1 prologue, -2 fixed)
    *maxext = 64;
    for (size_t i = 0; i < p.seg.size(); ++i) {
        NsSeg& s = p.seg[i];
        if (in_ext[i] > def) {
            if (writer == -1) p.kpad0 = def = in_ext[i];
            else if (writer >= 0) { NsSeg& w = p.seg[writer]; w.zext = in_ext[i] - w.dst_col; def = in_ext[i]; }
            else return false;
        }
        *maxext = std::max(*maxext, in_ext[i]);
        if (s.type == NS_WIDE) {
            if (s.dst_col != 0) return false;
            def = 512 * s.passes; writer = -2;
            *maxext = std::max(*maxext, def);
        } else {
            if (s.dst_col > def) return false;
            if (s.dst_col == 0) def = s.zext;               // overwrites its input from column 0
            else def = std::max(def, s.dst_col + s.zext);
            writer = (int)i;
        }
    }
    for (const NsSeg& s : p.seg) if (s.type != NS_WIDE) *maxext = std::max(*maxext, s.dst_col + s.zext);
    return true;
}

// ---- 4. sizes and limits: the LDS row stride, what the kernel's tables and the CU's LDS hold, the packed stream with the
//      SIDE blocks behind its biases
static bool ns_sizes(NsProgram& p, int maxext) {
    p.LD = std::max(((maxext + 63) & ~63) + 4, 516);        // >= 516: SPLIT partials need [8][rows][64] floats in one buffer
    if (p.bias_total > 3 * 64 * NS_NW * 4) return false;    // BMAX rounds of float4 per thread
    // (the sign-bit slots' share: never for the eligible shapes.  The wide-output one-launch gradient is fitted per engine, with its
    // sign bits, by net_stream_grad_fits: here it only has to fit the smallest one)
    if (p.lds_for(p.dxi_ok && (p.nout > 64 || p.dense) ? 4 : NS_ROWS, true) > (size_t)NS_LDS_BYTES) return false;
    int nrun = 0;
    for (const NsSeg& s : p.seg) nrun += s.passes;
    if (nrun > NS_MAXRUN) return false;
    p.packed_floats = (size_t)NS_NW * p.Gstride * NS_NT * 256 + (size_t)((p.bias_total + 3) & ~3);
    for (size_t i = 0; i < p.seg.size(); ++i)
        if (p.seg[i].type == NS_SIDE) {            // blocks of their own behind the biases
            p.seg[i].side_off = p.pack[i].side_off = (int)p.packed_floats;
            p.packed_floats += (size_t)NS_NW * p.seg[i].steps * NS_NT * 256;
            p.side_f4 += (size_t)NS_NW * p.seg[i].steps * NS_NT * 64;
        }
    return true;
}

// Translate the op list into segments; ok = false when something does not fit this kernel.
static NsProgram ns_build_one(const linna_layer_t* layers, int nl, int in_size, const NsBuildOpts& o, const NsDense* dn) {
    NsProgram p;
    NsLowered lo = ns_lower(layers, nl, in_size, o, dn);
    p.x0_keep = lo.x0_keep; p.dense = lo.dense; p.u_col = lo.u_col; p.u_same = lo.u_same;
    if (!lo.ok) return p;
    const int nfwd = lo.nfwd;
    int x0_seg = -1;
    for (int i = 0; i < (int)lo.lins.size(); ++i) if (lo.lins[i].x0_col) x0_seg = i;
    const NsShapeCtx ctx{o, o.dense ? dn : nullptr, nfwd, lo.f32seg, o.forward && !lo.mlp_grad && o.bwd != NS_BWD_INPUT && o.bwd != NS_BWD_TRAIN, x0_seg};
    NsShaper sh;
    for (const Lin& L : lo.lins) if (!ns_shape(sh, L, ctx)) return p;
    const int slots = lo.mlp_grad ? ns_append_mlp_grad(sh, lo.lins, ctx) : -1;
    p.seg = std::move(sh.seg); p.pack = std::move(sh.pack);
    int maxext = 0;
    if (!ns_written_columns(p, sh.in_ext, &maxext)) return p;
    if (p.kpad0 > (!o.forward ? 1024 : o.bf ? 512 : 256)) return p;
    p.bf = o.bf; p.f32seg = lo.f32seg;
    p.nout = lo.lins[nfwd - 1].N;
    p.Gstride = sh.G; p.nseg_f = nfwd; p.grad_ok = slots >= 0; p.mask_slots = std::max(slots, 0);
    for (int i = 0; i < nfwd; ++i) if (p.seg[i].type != NS_SIDE) p.G += ns_seg_steps(p.seg[i]);
    for (const Lin& L : lo.lins) { p.seg_op.push_back(L.op); p.seg_hidden.push_back(L.same_buf ? 1 : 0); }
    p.dxi_ok = o.bwd == NS_BWD_INPUT; p.nops = nl;
    p.train_ok = o.bwd == NS_BWD_TRAIN;
    p.bias_total = sh.bias_off;
    p.ok = ns_sizes(p, maxext);
    return p;
}

// The engine (rows per workgroup) net_stream_rows picks for a batch can be forced: linna_engine_rows does it for tests and
// measurements; LINNA_NS_ROWS in the environment sets the initial value.
static std::atomic<int> g_forced_rows{-1};
int ns_forced_rows_resolved() { return ns_switch(g_forced_rows, "LINNA_NS_ROWS", 0, [](int v) { return v == 4 || v == 8 || v == 16; }); }
int net_stream_force_rows(int rows) {
    if (rows != 0 && rows != 4 && rows != 8 && rows != 16) return -1;
    (void)ns_forced_rows_resolved();               // the environment's value is what `prev = engine_rows(4); ...; engine_rows(prev)` must restore
    return g_forced_rows.exchange(rows);
}

// SIDE segments (the kernel's K4 path) run on the 16-row engine of the serving programs and the one-launch gradient.  In the
// gradient's forward half they were measured slower in round 3 (with the activations stored for the gates); with the gates
// as sign bits in LDS and the per-segment tables read through the kernel-argument segment (without that the instantiation
// spilled 2.5 KB per lane): 151.4 -> 148.7 us at ChtoModelv2(33,33), 4096 chains (NOTES R4).  Not in bf16.
static bool ns_side(NsKind kind, int rows) {
    return rows == 16 && (kind == NS_SERVE || kind == NS_SERVE_DENSE || kind == NS_GRAD_INPUT || kind == NS_GRAD_INPUT_WIDE || kind == NS_GRAD_INPUT_DENSE);
}

static NsProgram ns_build_kind(NsKind kind, const linna_layer_t* layers, int nl, int in_size, const NsDense* dn, bool side) {
    NsBuildOpts o;
    o.side = side;
    switch (kind) {
    case NS_SERVE: case NS_STORE: o.bwd = NS_BWD_MLP; break;
    case NS_SERVE_DENSE: case NS_TRAIN_FWD: o.dense = true; break;
    case NS_SERVE_BF16: o.bf = true; if (dn) return NsProgram(); break;      // (no bf16 program with a dense segment)
    case NS_DX: o.forward = false; break;
    case NS_DX_INPUT: o.forward = false; o.dx_first = 0; break;
    case NS_GRAD_INPUT: o.bwd = NS_BWD_INPUT; break;
    case NS_GRAD_INPUT_WIDE: o.bwd = NS_BWD_INPUT; o.wide_out = true; break;
    case NS_GRAD_INPUT_DENSE: o.bwd = NS_BWD_INPUT; o.dense = true; break;
    case NS_GRAD_INPUT_BF16: o.bwd = NS_BWD_INPUT; o.bf = true; if (dn) return NsProgram(); break;
    case NS_TRAIN_STEP: case NS_TRAIN_STEP_BF16: o.dense = true; o.bwd = NS_BWD_TRAIN; o.bf = kind == NS_TRAIN_STEP_BF16; break;
    }
    NsProgram p = ns_build_one(layers, nl, in_size, o, dn);
    if (!p.ok && o.bwd == NS_BWD_MLP) {                     // the backward half may be what did not fit
        o.bwd = NS_BWD_NONE;
        p = ns_build_one(layers, nl, in_size, o, dn);
    }
    // the SIDE program where it fits, the plain one otherwise
    if (side && !(p.ok && ((kind != NS_GRAD_INPUT && kind != NS_GRAD_INPUT_WIDE && kind != NS_GRAD_INPUT_DENSE) || p.dxi_ok))) return ns_build_kind(kind, layers, nl, in_size, dn, false);
    return p;
}
NsProgramRef ns_program(NsKind kind, const linna_layer_t* layers, int nl, int in_size, const NsDense* dn, int rows) {
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

bool ns_program_plain(const NsProgram& p) {
    if (!p.ok || p.bf || p.dense || p.x0_keep || p.side_f4 || p.nseg_f < 1) return false;
    for (int i = 0; i < p.nseg_f; ++i) {
        const NsSeg& g = p.seg[i];
        if (g.type != NS_WIDE && g.type != NS_SPLIT) return false;
        if (g.x0_col || (g.type == NS_WIDE && (g.zext || g.kslice))) return false;
    }
    return true;
}
bool net_stream_program_plain(NsKind kind, const linna_layer_t* layers, int nl, int in_size, const NsDense* dn, int rows) {
    return kind == NS_SERVE && rows == 16 && ns_program_plain(*ns_program(kind, layers, nl, in_size, dn, rows));
}
// A plain launch has the diagonal likelihood with both halves of the linear output map (nothing optional left to select in
// the kernel), no exp map, lnP as its only output and no gate.
bool net_stream_launch_plain_ok(bool cscale, bool cshift, bool w, bool cexp, bool lnP, bool D, bool TH, bool gate) {
    return cscale && cshift && w && !cexp && lnP && !D && !TH && !gate;
}
static std::atomic<int> g_serve_plain{1};
int net_stream_serve_plain(int on) { return on < 0 ? g_serve_plain.load() : g_serve_plain.exchange(on ? 1 : 0); }
static std::atomic<int> g_serve_plain_sched{1};
int net_stream_serve_plain_sched(int hand) { return hand < 0 ? g_serve_plain_sched.load() : g_serve_plain_sched.exchange(hand ? 1 : 0); }
static std::atomic<int> g_serve_plain_trim{1};
int net_stream_serve_plain_trim(int on) { return on < 0 ? g_serve_plain_trim.load() : g_serve_plain_trim.exchange(on ? 1 : 0); }

int ns_trim_slive(const NsProgram& p, int i, int kp) {
    const NsSeg& g = p.seg[i];
    const NsPackSeg& q = p.pack[i];
    if (q.Kb) return 4;
    const int k0 = (g.type == NS_SPLIT ? kp * g.kslice : 0) + 16 * (g.steps - 1);     // first k of the part's last step
    return std::min(std::max(q.Ka - k0, 0), 4);
}
int ns_trim_tlive(const NsProgram& p, int i, int pass, int wave) {
    const NsSeg& g = p.seg[i];
    const int c0 = 64 * (g.type == NS_WIDE ? 8 * pass + wave : wave & ((1 << g.ncg_log2) - 1));
    return std::min(std::max((p.pack[i].N - c0 + 15) / 16, 0), 4);
}
static int ns_trim_slive_folded(const NsProgram& p, int i) {
    const int nkp = p.seg[i].type == NS_SPLIT ? NS_NW >> p.seg[i].ncg_log2 : 1;
    const int s0 = ns_trim_slive(p, i, 0);
    for (int kp = 1; kp < nkp; ++kp)
        if (ns_trim_slive(p, i, kp) != s0) return 4;
#ifdef NS_TRIM_NO_S1                                        // (a diagnostic build: T3 alone, for the stamps that gate S1 by itself)
    return 4;
#endif
    return s0 ? s0 : 4;
}
int ns_trim_fold(const NsProgram& p, int i) { return (std::min(p.pack[i].N, 4095) << 12) | ((ns_trim_slive_folded(p, i) - 1) << 24); }

// Text form of a plain serving program's liveness (tests, diagnostics): per forward segment "type steps passes", the live k
// slices of each K part's last step, the live tiles of every (pass, wave) and the step text each of them runs -- full, T3
// (every step), S1 (the last step), T3+S1 -- as net_stream_trim_kernel derives it from ns_trim_fold.  The `text` column repeats
// the kernel's arithmetic (begin_run, net_stream_body.inc) on the host: a host test of it pins this copy, and only the GPU
// test (tests/test_gpu_serve_trim.py: bit-identical lnP over the same shapes) checks the kernel's own derivation.
int net_stream_trim_describe(const linna_layer_t* layers, int nl, int in_size, int rows, char* buf, size_t n) {
    const NsProgramRef pref = ns_program(NS_SERVE, layers, nl, in_size, nullptr, rows);
    const NsProgram& p = *pref;
    const bool plain = rows == 16 && ns_program_plain(p);
    std::string out = plain ? "plain" : "not plain";
    char line[96];
    snprintf(line, sizeof line, " G %d nseg_f %d\n", p.G, p.nseg_f);
    out += line;
    for (int i = 0; plain && i < p.nseg_f; ++i) {
        const NsSeg& g = p.seg[i];
        const int nkp = g.type == NS_SPLIT ? NS_NW >> g.ncg_log2 : 1;
        snprintf(line, sizeof line, "%s steps %d passes %d slive", g.type == NS_WIDE ? "WIDE" : "SPLIT", g.steps, g.passes);
        out += line;
        for (int kp = 0; kp < nkp; ++kp) { snprintf(line, sizeof line, " %d", ns_trim_slive(p, i, kp)); out += line; }
        out += " tlive";
        for (int w = 0; w < g.passes * NS_NW; ++w) { snprintf(line, sizeof line, " %d", ns_trim_tlive(p, i, w / NS_NW, w % NS_NW)); out += line; }
        out += " text";
        const int fold = ns_trim_fold(p, i), N = (fold >> 12) & 4095;
        const bool s1 = ((fold >> 24) & 3) == 0;
        for (int w = 0; w < g.passes * NS_NW; ++w) {        // the kernel's own arithmetic (begin_run)
            const int c0 = 64 * (g.type == NS_WIDE ? w : (w % NS_NW) & ((1 << g.ncg_log2) - 1));
            const bool t3 = N - c0 > 32 && N - c0 <= 48;
            out += t3 && s1 ? " T3+S1" : t3 ? " T3" : s1 ? " S1" : " full";
        }
        out += "\n";
    }
    if (buf && n) snprintf(buf, n, "%s", out.c_str());
    return plain ? p.nseg_f : 0;
}

int ns_seg_cols(const NsProgram& p, const linna_layer_t* layers, int i) {
    if (p.seg_op[i] >= p.nops) return p.nout;               // the dense pair of NS_GRAD_INPUT_DENSE (op == nl): U, d lnP / dd
    const linna_layer_t& l = layers[p.seg_op[i]];
    return p.seg_hidden[i] ? l.C : i < p.nseg_f ? l.N : l.K;
}
NsGates ns_gates(const NsProgram& p, const linna_layer_t* layers, int nl, int rows) {
    NsGates g;
    for (int i = 0; i < NS_SEGCAP; ++i) g.gbit[i] = g.mbit[i] = -1;
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
        if (op >= nl) continue;                              // the transposed dense map: d lnP / dd, the gradient of an output nobody gated
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

// LDS of the fp32 one-launch gradient on the `rows` engine, sign bits included (0: no such program).  Each engine has its
// own figure: the activations and the bits scale with the rows, and the 16-row engine reads the SIDE program.
static size_t ns_grad_lds(const linna_layer_t* layers, int nl, int in_size, int rows) {
    const NsProgramRef pref = ns_program(ns_grad_kind(layers, nl), layers, nl, in_size, nullptr, rows);
    return pref->ok && pref->dxi_ok ? ns_gates(*pref, layers, nl, rows).lds : 0;
}
// Whether the fp32 one-launch gradient runs on the `rows` engine: program and sign bits within its LDS.  Networks of <= 64
// outputs fit every engine; wide outputs may not fit 16 rows (ChtoModelv2(26,457): 165 632 B with 3136 sign-bit columns).
// A batch whose engine the program does not fit takes the layered route, NOT a smaller engine: a smaller engine means more
// workgroups than CUs, i.e. two rounds of them -- measured at 4096 rows on the 8-row engine against the layered route on
// the 16-row one: 259.7 against 230.6 us at (26,457), 438.0 against 371.2 us at (40,1000) (wide outputs).
bool net_stream_grad_fits(const linna_layer_t* layers, int nl, int in_size, int rows) {
    const size_t lds = ns_grad_lds(layers, nl, in_size, rows);
    return lds && lds <= (size_t)NS_LDS_BYTES;
}

// The same two for the dense one-launch gradient (NS_GRAD_INPUT_DENSE): its program holds the dense pair and the folded
// output map, so it is fitted with its own descriptor; every width is fitted per engine
static size_t ns_grad_dense_lds(const linna_layer_t* layers, int nl, int in_size, const NsDense* dn, int rows) {
    const NsProgramRef pref = ns_program(NS_GRAD_INPUT_DENSE, layers, nl, in_size, dn, rows);
    if (!pref->ok || !pref->dxi_ok) return 0;
    const NsGates g = ns_gates(*pref, layers, nl, rows);
    return g.ok ? g.lds : 0;
}
bool net_stream_grad_dense_fits(const linna_layer_t* layers, int nl, int in_size, const NsDense* dn, int rows) {
    const size_t lds = ns_grad_dense_lds(layers, nl, in_size, dn, rows);
    return lds && lds <= (size_t)NS_LDS_BYTES;
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
    if (kind == NS_GRAD_INPUT || kind == NS_GRAD_INPUT_WIDE) {
        r.ok = p.ok && p.dxi_ok && ns_gates(p, layers, nl, NS_ROWS).lds <= (size_t)NS_LDS_BYTES;
        // wide outputs: on SOME engine -- a launch asks for its own (net_stream_grad_fits)
        for (int rows = 8; kind == NS_GRAD_INPUT_WIDE && rows >= 4; rows >>= 1) r.ok = r.ok || net_stream_grad_fits(layers, nl, in_size, rows);
        // one copy serves every engine: the 16-row one reads the SIDE program
        r.packed_floats = std::max(r.packed_floats, ns_program(kind, layers, nl, in_size, dn, 16)->packed_floats);
    }
    if (kind == NS_GRAD_INPUT_DENSE) {
        // the reasons of its own first (ns_lower refuses them all as "does not fit"); ok: on SOME engine, as for wide outputs
        bool inskip = false;
        for (int i = 0; i < nl; ++i) inskip = inskip || layers[i].op == LINNA_OP_INSKIP;
        bool fits = false;
        for (int rows = 16; rows >= 4; rows >>= 1) fits = fits || net_stream_grad_dense_fits(layers, nl, in_size, dn, rows);
        if (inskip) r.why = "an input-skip network has no one-launch gradient";
        else if (in_size > 64) r.why = "more than 64 network inputs: outside the one-launch gradient";
        else if (!dn || !dn->S || !dn->factored) r.why = "the dense one-launch gradient needs the factored inverse covariance";
        else if (!fits) r.why = "the program of the dense one-launch gradient fits no engine (segments, LDS or widths)";
        r.ok = r.why == nullptr;
        r.packed_floats = std::max(r.packed_floats, ns_program(kind, layers, nl, in_size, dn, 16)->packed_floats);
    }
    if (kind == NS_SERVE_BF16) { r.why = ns_bf16_refusal(p, layers, nl, in_size); r.ok = r.why == nullptr; }
    if (kind == NS_GRAD_INPUT_BF16) {
        // the reasons of its own first: ns_lower refuses them all as "does not fit"
        bool inskip = false;
        for (int i = 0; i < nl; ++i) inskip = inskip || layers[i].op == LINNA_OP_INSKIP;
        if (inskip) r.why = "an input-skip network has no one-launch gradient";
        else if (in_size > 64 || (nl >= 1 && layers[nl - 1].N > 64)) r.why = "more than 64 network inputs or outputs: outside the one-launch gradient";
        else r.why = ns_bf16_refusal(p, layers, nl, in_size);
        if (!r.why && !p.dxi_ok) r.why = "the network has no forward + dX program";
        if (!r.why && ns_gates(p, layers, nl, NS_ROWS).lds > (size_t)NS_LDS_BYTES) r.why = "the sign bits of the one-launch gradient do not fit the LDS";
        r.ok = r.why == nullptr;
    }
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
    if (p.ok && (kind == NS_GRAD_INPUT || kind == NS_GRAD_INPUT_BF16 || kind == NS_GRAD_INPUT_WIDE)) {            // the one-launch gradient: its LDS with the sign-bit matrix, on the 16-row engine
        const NsGates g = ns_gates(p, layers, nl, NS_ROWS);
        size_t lds[3]; int fits = 0;                        // the wide-output program is fitted per engine (net_stream_grad_fits)
        for (int e = 0; e < 3; ++e) {
            lds[e] = kind == NS_GRAD_INPUT_WIDE ? ns_grad_lds(layers, nl, in_size, 16 >> e) : 0;
            fits += lds[e] && lds[e] <= (size_t)NS_LDS_BYTES;
        }
        if (kind != NS_GRAD_INPUT_WIDE || fits == 3) {
            snprintf(line, sizeof line, "lds %zu of %d bytes with %d sign-bit columns: %s\n", g.lds, NS_LDS_BYTES, g.ncols,
                     g.lds <= (size_t)NS_LDS_BYTES && p.dxi_ok ? "one launch" : "layered");
            out += line;
        } else {                                            // not on every engine: each engine's bytes, then the engines that fit
            snprintf(line, sizeof line, "lds 16:%zu 8:%zu 4:%zu of %d bytes with %d sign-bit columns: %s", lds[0], lds[1], lds[2], NS_LDS_BYTES,
                     g.ncols, fits ? "one launch (rows" : "layered");
            out += line;
            for (int e = 0; fits && e < 3; ++e)
                if (lds[e] && lds[e] <= (size_t)NS_LDS_BYTES) { snprintf(line, sizeof line, " %d", 16 >> e); out += line; }
            out += fits ? ")\n" : "\n";
        }
    }
    if (p.ok && kind == NS_GRAD_INPUT_DENSE) {             // the dense one-launch gradient: every engine's bytes, always, then those that fit
        const NsGates g = ns_gates(p, layers, nl, rows ? rows : NS_ROWS);
        size_t lds[3]; int fits = 0;
        for (int e = 0; e < 3; ++e) {
            lds[e] = ns_grad_dense_lds(layers, nl, in_size, dn, 16 >> e);
            fits += lds[e] && lds[e] <= (size_t)NS_LDS_BYTES;
        }
        snprintf(line, sizeof line, "u_same %d u_col %d\nlds 16:%zu 8:%zu 4:%zu of %d bytes with %d sign-bit columns: %s", p.u_same, p.u_col, lds[0],
                 lds[1], lds[2], NS_LDS_BYTES, g.ncols, fits ? "one launch (rows" : "layered");
        out += line;
        for (int e = 0; fits && e < 3; ++e)
            if (lds[e] && lds[e] <= (size_t)NS_LDS_BYTES) { snprintf(line, sizeof line, " %d", 16 >> e); out += line; }
        out += fits ? ")\n" : "\n";
    }
    if (buf && n) { snprintf(buf, n, "%s", out.c_str()); }
    return p.ok ? (int)p.seg.size() : 0;
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
}  // namespace linna
