// The segment program of the whole-network kernel (net_stream.hip), as both sides see it: the planner (net_program.hip:
// pure host code, no kernel and no launch -- it turns a linna_layer_t list into the program) and the kernels with their
// launchers (net_stream.hip), which run it.
#pragma once
#include "common.h"
#include <memory>
#include <vector>

namespace linna {

constexpr int NS_ROWS = 16;                // rows per workgroup of the large-batch engine (and the LDS layout bound)
constexpr int NS_NW = 8;                 // waves per workgroup
constexpr int NS_NT = 4;                 // 16-column tiles per wave and step
constexpr int NS_MAXSEG = 20;              // segments of a program of every kind but NS_GRAD_INPUT_DENSE: what those kinds are checked against
constexpr int NS_SEGCAP = 22;              // capacity of the per-segment tables (NsArgs, NsPackArgs, NsGates): ChtoModelv2's NS_GRAD_INPUT_DENSE program
constexpr int NS_MAXRUN = 40;
constexpr unsigned NS_STEP_B = NS_NT * 1024;
constexpr int NS_LDS_BYTES = 160 * 1024;
constexpr int AS_BLOCK = 64;               // threads per block of adamw_streams_kernel (one wave: ~1200 blocks for 1.3 M parameters, five per CU)
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

// what ns_pack_kernel (net_stream.hip: the weight re-layout, where the stream's order is described) reads of a segment
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
    const float* kscale;                          // per contraction index of the first K part: Wa(n, k) * kscale[k] -- the transposed last
                                                  // layer behind a folded output map (NS_GRAD_INPUT_DENSE: the forward one carries rscale)
};

// ---------------------------------------------------------------------------- host side: the program
struct NsProgram {
    std::vector<NsPackSeg> pack;
    std::vector<NsSeg> seg;
    int G = 0, LD = 0, kpad0 = 0, nout = 0, bias_total = 0;
    int Gstride = 0, nseg_f = 0, mask_slots = 0;            // G: forward steps; Gstride: forward + backward steps
    size_t packed_floats = 0;                               // floats of the packed stream: weights, biases, SIDE blocks
    int dense = 0, u_col = 0, u_same = 0;                   // dense inverse covariance appended as the last segment
    int x0_keep = 0;                                        // an input-skip segment copies the network input later
    size_t side_f4 = 0;                                     // 16-byte vectors of all SIDE blocks
    bool bf = false;                                        // bf16 stream: 32 k per step, first layer [W | W] over [x_hi ; x_lo]
    int f32seg = -1;                                        // ... but for this segment, an fp32 run (the training step's loss)
    bool ok = false, grad_ok = false;                       // grad_ok: backward segments appended (ReLU MLPs)
    bool dxi_ok = false;                                    // the dX chain down to the input appended (NS_GRAD_INPUT)
    bool train_ok = false;                                  // forward + loss + dX chain (NS_TRAIN_STEP)
    int nops = 0;                                           // ops of the layer list: a segment of op index nops is a dense map, not a layer's
    std::vector<int> seg_op, seg_hidden;                    // forward segments: op index; 1 = the hidden h of a residual block
                                                            // (dX-chain program: 1 = d/dh of a residual block, else d/d(input) of the op)
    size_t lds_for(int rows, bool grad) const;              // dynamic LDS of a launch on the engine of `rows` rows per workgroup
};

// steps of a segment in every wave's stream (a WIDE segment's second pass may be shorter: NsSeg::zext)
// zext < 0: the BALANCED triangular assignment of a 16-block lower-triangular factor -- wave w multiplies column block w
// (rows from 64 w) and then block 15 - w (rows from 64 (15 - w)): steps - 4 w and steps - 4 (15 - w) steps, 2 steps - 60 in
// every wave
int ns_seg_steps(const NsSeg& s);
int ns_forced_rows_resolved();   // linna_engine_rows / LINNA_NS_ROWS: 0 automatic, else the engine every batch runs on (net_stream_rows)
// Kernel-configuration cache: a program is a pure function of the op list (shapes AND parameter pointers:
// the pack descriptors carry them), the program kind, the engine (SIDE segments or not) and the dense descriptor, so it
// is built once and looked up by those bytes on every later launch -- no segment planning, no vector allocation on the
// launch path.  Entries live for the life of the library (a handful per network; the table is cleared if it ever reaches
// 256 entries).  A lookup hands out shared ownership: a clear by a later lookup never frees a program a caller still
// holds.  rows: the engine that runs it (0: any; no SIDE segments).
typedef std::shared_ptr<const NsProgram> NsProgramRef;
NsProgramRef ns_program(NsKind kind, const linna_layer_t* layers, int nl, int in_size, const NsDense* dn, int rows);

// A serving program is PLAIN when the lean instantiation of the kernel (net_stream_plain_kernel) can run its forward half:
// fp32, every forward segment WIDE or SPLIT with no short or balanced second pass, no SIDE block, no kept input rows (input
// skip), no dense segment.  The launch adds its own conditions (net_stream_launch_plain_ok).
bool ns_program_plain(const NsProgram& p);
// Liveness of the matrix work of a plain program's forward segment i (what net_stream_trim_kernel leaves out; decided here,
// on the host).  ns_trim_slive: how many of the four k slices of the LAST step of K part kp (WIDE: kp = 0) hold a real k,
// 0 .. 4 -- rem = Ka - k of that step's first slice, min(rem, 4); 4 for a segment with a second K part.  ns_trim_tlive: how many
// leading 16-column tiles of the 64-column block of (pass, wave) hold a real column, 0 .. 4.  ns_trim_fold: what the launcher
// ORs into NsSeg::type beside ncg_log2 (bits 8-11): N in bits 12-23 and slive - 1 in bits 24-25 (a SPLIT segment whose K
// parts differ, and slive 0: 3, the full text) -- the wave derives its own tlive from N, its pass and its column group.
int ns_trim_slive(const NsProgram& p, int i, int kp);
int ns_trim_tlive(const NsProgram& p, int i, int pass, int wave);
int ns_trim_fold(const NsProgram& p, int i);
// columns of what segment i of a one-launch forward + backward program (NS_GRAD_INPUT, NS_TRAIN_STEP) writes: the hidden h
// of a residual block, a forward op's output, or (the backward half) d/d(op input)
int ns_seg_cols(const NsProgram& p, const linna_layer_t* layers, int i);
// The gates of a one-launch backward half (NS_GRAD_INPUT, NS_TRAIN_STEP): what the backward gates on is the SIGN of a
// forward activation, and the workgroup that needs it is the one that computed it -- one bit per (row, column) in LDS
// behind the program's own LDS (NsArgs::nbw, bits_off).  gbit[i]: the first bit column of forward segment i's signs (-1:
// no gate asks for them; every tensor rounded up to 64 columns); mbit[i]: the columns backward segment i gates on (-1:
// none).  ok = false when a gate has no producer.
struct NsGates {
    int gbit[NS_SEGCAP], mbit[NS_SEGCAP];
    int ncols = 0;
    bool ok = true;
    size_t lds0 = 0, lds = 0;                               // the program's LDS (8-byte aligned), and with the bits
};
NsGates ns_gates(const NsProgram& p, const linna_layer_t* layers, int nl, int rows);
}  // namespace linna
